"""``EmpiricalNormalization`` as rsl-rl-lib 3.x defines it (``rsl_rl.networks.EmpiricalNormalization``,
what ``actor_obs_normalization`` / ``critic_obs_normalization`` switch on): running mean and biased
variance of the observations, ``forward(x) = (x - mean) / (std + eps)``. rsl_rl is not installed here,
so this is a restatement with the same buffer names (``_mean``, ``_var``, ``_std``, ``count``: the
checkpoint keys) and the same update rule.

Every write is in place: on a GPU the buffers' device pointers are bound into libzbot_ppo's kernels
and into captured graphs (``rl/fused.py``; ``zbp_norm_update`` is this module's ``update`` on the
device), and ``load_state_dict`` copies into them, so they stay valid across a checkpoint load.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn


class EmpiricalNormalization(nn.Module):
    def __init__(self, shape, eps: float = 1e-2, until: Optional[int] = None):
        super().__init__()
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self.eps = eps
        self.until = until
        self.register_buffer("_mean", torch.zeros(shape).unsqueeze(0))
        self.register_buffer("_var", torch.ones(shape).unsqueeze(0))
        self.register_buffer("_std", torch.ones(shape).unsqueeze(0))
        self.register_buffer("count", torch.tensor(0, dtype=torch.long))

    @property
    def mean(self) -> torch.Tensor:
        return self._mean.squeeze(0).clone()

    @property
    def std(self) -> torch.Tensor:
        return self._std.squeeze(0).clone()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """Normalize; the statistics are only ever changed by ``update``."""
        return (x - self._mean) / (self._std + self.eps)

    @torch.jit.unused
    def update(self, x: torch.Tensor) -> None:
        """Merge the batch ``x`` [n, D] into the running statistics (frozen once ``count >= until``).
        No host synchronisation: the ``until`` test selects on the device, so the unfused GPU rollout
        stays capturable."""
        with torch.no_grad():
            n = x.shape[0]
            count = self.count + n
            rate = n / count
            var_x = torch.var(x, dim=0, unbiased=False, keepdim=True)
            mean_x = torch.mean(x, dim=0, keepdim=True)
            delta = mean_x - self._mean
            mean = self._mean + rate * delta
            var = self._var + rate * (var_x - self._var + delta * (mean_x - mean))
            if self.until is not None:
                on = self.count < self.until
                count = torch.where(on, count, self.count)
                mean, var = torch.where(on, mean, self._mean), torch.where(on, var, self._var)
            self.count.copy_(count)
            self._mean.copy_(mean)
            self._var.copy_(var)
            self._std.copy_(torch.sqrt(var))
