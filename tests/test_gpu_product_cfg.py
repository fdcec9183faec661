"""Oracle parity and determinism of the step kernels the product launches: the configuration of the
four registered envs (tests/fullstate.product_cfg: TGS, self_manifold 3 for walking v2 and stand-up,
2 for walking v4 and the manager) selects eight instantiations,

    task         <= 4096 envs                            > 4096 envs
    walking v2   zb_step_kernel<true,1,false,true>       zb_step_kernel<true,2,false,true>
    stand-up     zb_su_step_kernel<true,1,false,true>    zb_su_step_kernel<true,2,false,true>
    walking v4   zb_v4_step_kernel<true,1>               zb_v4_step_kernel<true,2>
    manager      zb_m_step_kernel<true,1>                zb_m_step_kernel<true,2>

none of which the PGS / self_manifold 2 default of the other parity tests reaches (outlier counts
move with code generation alone, DESIGN.md §6: a neighbouring instantiation says nothing about
these). Every test here runs inside product(), without ZB_OCC1, asserts ZbotSim.kernel_variant()
against the table before it steps, and uses tests/test_gpu_fullstate._check with the project's
tolerances and caps unchanged: every env inside tolerance or explained, and the contact-active
aggregate against the f64 oracle. The shapes are the smallest that select the kernel in question.
"""
from __future__ import annotations

import numpy as np
import pytest

import test_gpu_fullstate as F
from fullstate import TASKS, base_task, constructed_states, product, random_states, task_cfg
from helpers import perturbed_states

pytestmark = pytest.mark.gpu

# 4126 envs: above the 4096 switch to two waves per SIMD; 1032 workgroups, a multiple of 8 (the XCD
# renumbering is active); the last workgroup holds two envs
N_OCC2 = 4126


def variant(task: str, n: int) -> tuple:
    """(kTgs, kOcc, kRefresh, kRf) of the table above."""
    return (1, 1 if n <= 4096 else 2, 0, 1 if base_task(task) in ("v2", "standup") else 0)


@pytest.fixture(autouse=True)
def _product(monkeypatch):
    monkeypatch.delenv("ZB_OCC1", raising=False)
    with product():
        yield


def _sim(task, n, seed):
    from zbot_lab_amd.sim import ZbotSim
    g = ZbotSim(n, task_cfg(task), device="cuda:0", seed=seed)
    assert g.kernel_variant() == variant(task, n), (task, n, g.kernel_variant())
    return g


def _oracle(task, n, seed):
    from oracle.pyoracle import OracleSim
    return OracleSim(n, task_cfg(task), seed=seed)


def _out(obs, rew, te, tr):
    return obs.cpu().numpy(), rew.cpu().numpy(), te.cpu().numpy().copy(), tr.cpu().numpy().copy()


@pytest.mark.parametrize("task", ["v2", "v2:step0", "standup", "v4", "manager"])
def test_product_one_step(gpu, task):
    """One step from random full states, one wave per SIMD: the handle seed, states and actions of
    test_full_state_tgs (whose self_manifold 2 kernel is the direct neighbour). The f32 oracle's own
    count against f64 on these inputs is 16, 14, 0, 24 and 1 of 2048."""
    import torch
    n, seed = 2048, 19
    st = random_states(task, _oracle(task, n, seed), n, seed=111)
    a = np.random.default_rng(8).normal(size=(n, 6)).astype(np.float32)
    g = _sim(task, n, seed)
    g.set_state(torch.from_numpy(st).cuda())
    g_out = _out(*g.step(torch.from_numpy(a).cuda()))
    nbad = F._check(task, "product cfg: one step from random full states", n, seed, st, [a], g_out,
                    g.get_state().cpu().numpy(), torch)
    assert nbad <= 0.02 * n


@pytest.mark.parametrize("task", TASKS)
def test_product_one_step_two_waves(gpu, task):
    """One step of 4126 envs (two waves per SIMD). Stand-up, v4 and the manager against the oracle on
    every column (their draws are keyed on the env index); walking v2, the slow oracle, on the spread
    1024-column sample of tests/test_gpu_fullsize.py (both ends, the last partial workgroup included;
    envs are independent, so the sample is an exact sub-problem). The f32 oracle's count against f64
    over every column is 43, 0, 32 and 3 of 4126 (v2, stand-up, v4, manager)."""
    import torch
    from test_gpu_fullsize import _sample
    n, seed = N_OCC2, 37
    st = random_states(task, _oracle(task, n, seed), n, seed=500)
    a = np.random.default_rng(n + 1).normal(size=(n, 6)).astype(np.float32)
    g = _sim(task, n, seed)
    g.set_state(torch.from_numpy(st).cuda())
    obs, rew, te, tr = _out(*g.step(torch.from_numpy(a).cuda()))
    sg = g.get_state().cpu().numpy()
    g.close()
    ids = _sample(n) if task == "v2" else np.arange(n)
    sub = lambda x: np.ascontiguousarray(x[:, ids])  # noqa: E731
    nbad = F._check(task, f"product cfg: one step of {n} envs, {len(ids)} columns", len(ids), seed, sub(st),
                    [np.ascontiguousarray(a[ids])], (np.ascontiguousarray(obs[ids]), rew[ids].copy(), te[ids].copy(),
                                                     tr[ids].copy()), sub(sg), torch)
    assert nbad <= 0.02 * len(ids)


@pytest.mark.parametrize("task", TASKS)
def test_product_zero_action_standing(gpu, task):
    """20 zero-action steps from (near-)standing states, every row at the end, with the outlier cap of
    test_full_state_tgs on top of _check. 2048 envs: at 1024 the f32 oracle has 10-25 outliers, too few
    to separate it from the device; here its count against f64 is 46, 0, 49 and 24 of 2048."""
    import torch
    n, seed, steps = 2048, 6, 20
    st = random_states(task, _oracle(task, n, seed), n, seed=212, standing=True)
    g = _sim(task, n, seed)
    g.set_state(torch.from_numpy(st).cuda())
    at = torch.zeros(n, 6, device="cuda:0")
    for _ in range(steps):
        out = g.step(at)
    stats = {}
    nbad = F._check(task, f"product cfg: {steps} zero-action steps from standing", n, seed, st,
                    [np.zeros((n, 6), np.float32)] * steps, _out(*out), g.get_state().cpu().numpy(), torch, stats=stats)
    assert nbad <= F.AGG_FRAC_K_MULTI * stats["nbad_f32"] + 0.005 * n, (nbad, stats["nbad_f32"])


@pytest.mark.parametrize("task,kind", [("v2", "face"), ("v2", "rim"), ("v2", "rimface"), ("standup", "face"),
                                       ("standup", "rim"), ("standup", "rimface"), ("v4", "face"), ("v4", "rim")])
def test_product_self_contact_classes(gpu, task, kind):
    """The self-contact classes (cap on cap, side by side, a link lying on another's cap) under the
    product solve: 512 constructed folds per case (tests/fullstate.constructed_states), one step under
    the full-state rule. (Not the manager task: its robot model differs and the seed folds do not keep
    their class on it; test_full_state_contact_cache exercises its self contacts.)"""
    import torch
    from fullstate import CLASS_COL
    seed, n = 43, 512
    st, which = constructed_states(task, kind, n, seed=606)
    o = _oracle(task, n, seed)
    o.set_state(st)
    pc = o.pair_classes()
    assert (pc[:, CLASS_COL[kind]] > 0).all() and (pc[:, 3] == 0).all()
    F._manifold_step(task, f"{kind} (product cfg)", n, seed, st, which, pc, _sim(task, n, seed), torch)


@pytest.mark.parametrize("task", TASKS)
def test_product_determinism_two_waves(gpu, task):
    """Two handles with the same seed, 40 random-action steps of 4126 envs from a full reset: outputs
    and the final state bit-identical and finite at two waves per SIMD."""
    import torch
    n, steps = N_OCC2, 40
    g1, g2 = _sim(task, n, 7), _sim(task, n, 7)
    for x in (g1, g2):
        x.reset(None)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(7)
    for k in range(steps):
        a = torch.randn(n, 6, device="cuda:0", generator=gen)
        o1, r1, t1, u1 = g1.step(a)
        o2, r2, t2, u2 = g2.step(a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(t1, t2) and torch.equal(u1, u2), k
        assert torch.isfinite(o1).all() and torch.isfinite(r1).all(), k
    s1, s2 = g1.get_state(), g2.get_state()
    assert torch.equal(s1, s2) and torch.isfinite(s1).all()
    g1.close()
    g2.close()


def test_product_permutation_equivariance_4128(gpu):
    """Walking v2, one step of 4128 envs (1032 full workgroups, the smallest grid above 4096 that is
    renumbered XCD-major): permuting the env columns of the state and the action rows permutes every
    output bit for bit (test_permutation_equivariance_65536's property on the product kernel)."""
    import torch
    n = 4128
    st = perturbed_states(n, seed=61)
    a = np.random.default_rng(3).normal(size=(n, 6)).astype(np.float32)
    perm = np.random.default_rng(4).permutation(n)
    g1, g2 = _sim("v2", n, 0), _sim("v2", n, 0)
    g1.set_state(torch.from_numpy(st).cuda())
    g2.set_state(torch.from_numpy(np.ascontiguousarray(st[:, perm])).cuda())
    out1 = _out(*g1.step(torch.from_numpy(a).cuda()))
    out2 = _out(*g2.step(torch.from_numpy(np.ascontiguousarray(a[perm])).cuda()))
    assert not (out1[2] | out1[3]).all()  # no full-reset episode-length draw (that one is keyed by env index)
    for x1, x2 in zip(out1, out2):
        np.testing.assert_array_equal(x1[perm], x2)
    np.testing.assert_array_equal(g1.get_state().cpu().numpy()[:, perm], g2.get_state().cpu().numpy())
    g1.close()
    g2.close()
