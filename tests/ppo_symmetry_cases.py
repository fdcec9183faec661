"""PPO snapshots for the symmetry tests (tests/test_ppo_symmetry.py on the CPU,
tests/test_gpu_ppo_symmetry.py on the GPU): tests/ppo_options_cases.make_alg with a ``symmetry_cfg``, plus

* a random signed permutation per tensor (observations, critic observations, actions) from a fixed seed:
  two fixed points, one with sign -1 and one with sign +1, and one cycle through every other column, so
  the map is no involution; signs mixed;
* the kink condition (ppo_options_cases, TAU = 1e-5) applied to every row AND to its mirror image: a row
  is redrawn when either has a hidden pre-activation of the fp64 forward within TAU of 0, repeated until
  none is left. The redraw cap is 10 % of a tensor's rows (a single pass measures at most 3 %, the union
  of the two at most 6 %); the builder asserts it.

Rows redrawn, measured on the CPU (actor tensor, critic tensor) of the rows of a tensor, seed 0:

    v2 192 elu scalar                 (19, 19) of 768     v2 192 relu log, normalizers      (14, 18) of 768
    standup 192 elu scalar            (28, 29) of 768     partial 96 relu log, normalizers  (3, 4) of 384
    partial 96 elu scalar             (9, 3) of 384       v2 96 elu scalar                  (12, 5) of 384
    v2 192 / partial 96, cases.LOSS   as elu scalar       v2 512 x 24 tanh, seed 3          (306, 296) of 12288
    identity map: v2 192 (6, 8) of 768, partial 96 (4, 3) of 384, v2 96 (4, 4) of 384

the largest 3.8 % (ppo_options_cases itself asserts 5 % on the same union).
"""
from __future__ import annotations

import torch

import ppo_cases as cases
import ppo_options_cases as OC
import ppo_reference as R
import ppo_symmetry_reference as RS

MAX_REDRAWN = 0.10
MODES = {"aug": (True, False), "mirror": (False, True), "both": (True, True)}
MIRROR_COEFF = 0.7


def signed_permutation(n, g):
    """(perm, sign) of n >= 5 columns from the CPU generator g: two fixed points (signs -1 and +1), one
    cycle through the other n - 2 columns (length >= 3: not an involution), mixed signs."""
    order = torch.randperm(n, generator=g).tolist()
    fixed, rest = order[:2], order[2:]
    perm = list(range(n))
    for i, k in enumerate(rest):
        perm[k] = rest[(i + 1) % len(rest)]
    sign = [1.0 if x else -1.0 for x in (torch.rand(n, generator=g) < 0.5).tolist()]
    sign[fixed[0]], sign[fixed[1]] = -1.0, 1.0
    sign[rest[0]], sign[rest[1]] = 1.0, -1.0
    assert any(perm[perm[k]] != k for k in range(n))
    return perm, sign


def random_map(shape, seed=0):
    from zbot_lab_amd.rl.symmetry import SignedPermutation
    g = torch.Generator().manual_seed(1000 + seed)
    (op, os_), (cp, cs), (ap, as_) = (signed_permutation(shape[k], g) for k in ("obs", "cobs", "act"))
    return SignedPermutation(op, os_, ap, as_, cp, cs)


def identity_map(shape):
    from zbot_lab_amd.rl.symmetry import SignedPermutation
    return SignedPermutation.identity(shape["obs"], shape["act"], shape["cobs"])


def make_alg(device, shape, rows, mode, act="elu", std_type="scalar", seed=0, normalizers=False, func=None, **ppo_kw):
    """ppo_options_cases.make_alg with symmetry_cfg = (mode, MIRROR_COEFF, func or the seed's random map):
    no observation row, and no mirror image of one, near a kink (``alg.redrawn``). mode None: the same
    snapshot without a symmetry_cfg (the rows and the map's kink condition are the same)."""
    func = random_map(shape, seed) if func is None else func
    plain = OC.near_kink_rows

    def near_kink_rows(x, weights, biases, norm, act_):
        # (the critic's tensor is the one whose net has one output; none of these shapes has one action)
        name = "critic" if weights[-1].shape[0] == 1 else "obs"
        bad = plain(x, weights, biases, norm, act_)
        if hasattr(func, "mirror"):
            bad |= plain(func.mirror(x.cpu(), name), weights, biases, norm, act_)
        return bad

    OC.near_kink_rows = near_kink_rows
    try:
        kw = dict(ppo_kw)
        if mode is not None:
            aug, mirror = MODES[mode]
            kw["symmetry_cfg"] = dict(use_data_augmentation=aug, use_mirror_loss=mirror, mirror_loss_coeff=MIRROR_COEFF,
                                      data_augmentation_func=func)
        alg = OC.make_alg(device, shape, rows, act=act, std_type=std_type, seed=seed, normalizers=normalizers, **kw)
    finally:
        OC.near_kink_rows = plain
    red, n_rows = alg.redrawn
    assert max(red) <= MAX_REDRAWN * n_rows, (red, n_rows)
    alg.sym_func = func
    return alg


def reference_minibatch(alg, i, act, std_type, mode=None, func=None):
    """ppo_symmetry_reference.minibatch_reference for minibatch i under the algorithm's symmetry cfg (or
    `mode` / `func`): ({parameter name: fp64 gradient}, stats [5]: kl mean, value loss, surrogate, entropy,
    symmetry loss)."""
    pol = alg.policy
    aw, ab, cw, cb, noise = OC.net_tensors(pol)
    na, nc = cases.norms(pol)
    if mode is None:
        sy = alg.symmetry
        aug, mirror, coeff, func = (sy["use_data_augmentation"], sy["use_mirror_loss"], sy["mirror_loss_coeff"],
                                    sy["data_augmentation_func"])
    else:
        (aug, mirror), coeff, func = MODES[mode], MIRROR_COEFF, func or alg.sym_func
    grads, stats = RS.minibatch_reference(aw, ab, cw, cb, noise, cases.gathered_rows(alg, i), func, aug, mirror, coeff,
                                          alg.clip_param, alg.value_loss_coef, alg.entropy_coef,
                                          alg.use_clipped_value_loss, act=act, std_type=std_type, actor_norm=na,
                                          critic_norm=nc)
    named = {OC.noise_name(pol): grads["noise"]}
    for net, seq in (("actor", pol.actor), ("critic", pol.critic)):
        for k, (idx, _) in enumerate(cases.linears(seq)):
            named[f"{net}.{idx}.weight"] = grads[f"{net}_w"][k]
            named[f"{net}.{idx}.bias"] = grads[f"{net}_b"][k]
    vec = torch.stack([stats[k] for k in ("kl_mean", "value_loss", "surrogate", "entropy", "symmetry")])
    return named, vec


def torch_minibatch(alg, i):
    """PPO.minibatch_loss (the project's torch statement, symmetry included) for minibatch i of the first epoch
    in the policy's own precision, backward into .grad; returns the five stats as reference_minibatch."""
    gen = alg.storage.mini_batch_generator(alg.num_mini_batches, 1, alg.mb_indices)
    for k, mbt in enumerate(gen):
        if k == i:
            break
    loss, kl, vl, surr, ent, symm = alg.minibatch_loss(mbt, True)
    alg.optimizer.zero_grad(set_to_none=False)
    loss.backward()
    alg.policy.distribution = None
    return torch.stack([kl, vl.detach(), surr.detach(), ent.detach(),
                        symm.detach() if symm is not None else torch.zeros_like(kl)])
