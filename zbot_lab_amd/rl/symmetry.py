"""Mirror maps for rsl_rl's ``symmetry_cfg`` (data augmentation and the mirror loss of ``PPO.update``).

``SignedPermutation`` describes ONE mirror of the task (so ``num_aug = 2``) as a signed permutation per
tensor:

    obs_m[k] = obs_sign[k] * obs[obs_perm[k]]        act_m[a] = act_sign[a] * act[act_perm[a]]

with tables of its own for the critic's observation group (they default to the policy's when the two
dims agree). It is callable with rsl_rl's ``data_augmentation_func`` signature,
``(obs=None, actions=None, env=None) -> (obs_aug, actions_aug)`` with the originals first, so the same
object drives the torch statement (``PPO.update_steps``), would drive real rsl_rl, and hands its tables
to the fused kernels (``rl/fused.py``; ``zbp_symmetry`` in ``include/zbot_ppo.h``).

No table for the ZBOT robot ships with the project: whether its left-right symmetry is a signed
permutation of the 23 observations (a world-frame base quaternion, a chain whose reversal swaps the
feet) has to be shown by an equivariance check on the simulator first.
"""
from __future__ import annotations

from collections.abc import Mapping

import torch


def _table(perm, sign, what: str):
    perm, sign = [int(p) for p in perm], [float(s) for s in sign]
    n = len(perm)
    if n < 1 or len(sign) != n:
        raise ValueError(f"{what}: perm and sign must have one entry per column, got {n} and {len(sign)}")
    if sorted(perm) != list(range(n)):
        raise ValueError(f"{what}: perm is not a permutation of 0 .. {n - 1}")
    if any(s not in (1.0, -1.0) for s in sign):
        raise ValueError(f"{what}: signs must be +1 or -1")
    return perm, sign


class SignedPermutation:
    """One mirror map. A plain class of lists (deep-copyable: ``dataclasses.asdict`` copies it); an
    involution is not required."""

    def __init__(self, obs_perm, obs_sign, act_perm, act_sign, critic_obs_perm=None, critic_obs_sign=None):
        self.obs_perm, self.obs_sign = _table(obs_perm, obs_sign, "obs")
        self.act_perm, self.act_sign = _table(act_perm, act_sign, "actions")
        if (critic_obs_perm is None) != (critic_obs_sign is None):
            raise ValueError("critic obs: give both perm and sign, or neither")
        if critic_obs_perm is None:
            self.critic_obs_perm, self.critic_obs_sign = None, None
        else:
            self.critic_obs_perm, self.critic_obs_sign = _table(critic_obs_perm, critic_obs_sign, "critic obs")
        self._tensors: dict = {}

    # -- dims
    @property
    def obs_dim(self) -> int:
        return len(self.obs_perm)

    @property
    def num_actions(self) -> int:
        return len(self.act_perm)

    def critic_tables(self, critic_obs_dim: int):
        """(perm, sign) of the critic group: its own tables, or the policy's when the dims agree."""
        if self.critic_obs_perm is not None:
            perm, sign = self.critic_obs_perm, self.critic_obs_sign
        else:
            perm, sign = self.obs_perm, self.obs_sign
        if len(perm) != critic_obs_dim:
            raise ValueError(f"critic obs: the map has {len(perm)} columns, the group {critic_obs_dim} "
                             "(critic_obs_perm / critic_obs_sign are required when the dims differ)")
        return perm, sign

    def matches(self, obs_dim: int, critic_obs_dim: int, num_actions: int) -> bool:
        """Whether the map's dims are the policy's."""
        critic = len(self.critic_obs_perm) if self.critic_obs_perm is not None else self.obs_dim
        return (self.obs_dim, critic, self.num_actions) == (obs_dim, critic_obs_dim, num_actions)

    # -- tensors
    def device_tables(self, name: str, device, critic_obs_dim: int | None = None):
        """(perm int32, sign float32) of "obs" / "critic" / "actions" on `device`, uploaded once."""
        key = (name, str(device))
        if key not in self._tensors:
            if name == "critic":
                perm, sign = self.critic_tables(self.obs_dim if critic_obs_dim is None else critic_obs_dim)
            else:
                perm, sign = {"obs": (self.obs_perm, self.obs_sign), "actions": (self.act_perm, self.act_sign)}[name]
            self._tensors[key] = (torch.tensor(perm, dtype=torch.int32, device=device),
                                  torch.tensor(sign, dtype=torch.float32, device=device))
        return self._tensors[key]

    def mirror(self, x: torch.Tensor, name: str) -> torch.Tensor:
        """x[..., k] -> sign[k] * x[..., perm[k]] with the tables of "obs" / "critic" / "actions"."""
        if name == "critic":
            self.critic_tables(x.shape[-1])
        perm, sign = self.device_tables(name, x.device, x.shape[-1])
        if x.shape[-1] != perm.numel():
            raise ValueError(f"{name}: the map has {perm.numel()} columns, the tensor {x.shape[-1]}")
        return x.index_select(-1, perm.long()) * sign.to(x.dtype)

    def _augment(self, x, name: str):
        return torch.cat([x, self.mirror(x, name)], dim=0)

    def __call__(self, obs=None, actions=None, env=None):
        """rsl_rl's data_augmentation_func: cat([x, mirror(x)]) of the observations (a tensor, or a mapping
        of observation groups: the group "critic" takes the critic tables, every other the policy's) and of
        the actions; None stays None."""
        obs_aug = None
        if isinstance(obs, Mapping) or hasattr(obs, "keys"):
            obs_aug = {k: self._augment(obs[k], "critic" if k == "critic" else "obs") for k in obs.keys()}
        elif obs is not None:
            obs_aug = self._augment(obs, "obs")
        return obs_aug, None if actions is None else self._augment(actions, "actions")

    def __deepcopy__(self, memo):
        return SignedPermutation(self.obs_perm, self.obs_sign, self.act_perm, self.act_sign, self.critic_obs_perm,
                                 self.critic_obs_sign)

    def to_dict(self) -> dict:
        return {k: getattr(self, k) for k in ("obs_perm", "obs_sign", "act_perm", "act_sign", "critic_obs_perm",
                                              "critic_obs_sign")}

    @classmethod
    def from_dict(cls, d: dict) -> "SignedPermutation":
        return cls(d["obs_perm"], d["obs_sign"], d["act_perm"], d["act_sign"], d.get("critic_obs_perm"),
                   d.get("critic_obs_sign"))

    @classmethod
    def identity(cls, obs_dim: int, num_actions: int, critic_obs_dim: int | None = None) -> "SignedPermutation":
        c = None if critic_obs_dim is None else list(range(critic_obs_dim))
        return cls(list(range(obs_dim)), [1.0] * obs_dim, list(range(num_actions)), [1.0] * num_actions, c,
                   None if c is None else [1.0] * critic_obs_dim)
