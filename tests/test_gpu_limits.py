"""Oracle parity of the step kernels at the action, joint and speed limits (tests/limit_cases.py): the
product runs tanh-saturated actions with p_delta on its +-pi clamp, and the other full-state tests
send N(0, 1) actions from states that never reach a clamp. All four tasks, the product configuration
(tests/fullstate.product_cfg, kernel_variant asserted), 1024 envs, one zb_step each; the inputs, their
coverage conditions and the planted faults these rules catch are in tests/test_limit_cases.py.

test_action_prologue_exact: the stored actions bit-equal to the f32 oracle's and to
float32(tanh(float64(a))) over the whole action table (signed zero, denormals, the 9.0109 boundary,
the |x| <= 20 clamp, FLT_MAX, inf), clamped P_DELTA entries bit-equal to +-float32(pi), the others
within err <= max(4 e32, 2 eps32 max |x64|) per joint (limit_cases.check_prologue).

test_full_state_at_limits: tests/test_gpu_fullstate._check unchanged, the outlier count capped by the
f32 oracle's own count against f64 (nbad <= 2 nbad_f32 + 0.005 n), and the limit branches re-asserted on
the device's own post-step state (joint speed limit and angular cap held, wraps taken).

test_limits_deterministic: the same step twice, bit-identical.

Measured on an MI355X (v2 / v4 / stand-up / manager; nbad_f32, the f32 aggregate and the coverage
conditions are the oracle's alone, the rest is the device's):
* prologue: no env reset on the device (manager 0.7 %); 1106 / 1105 / 1166 P_DELTA entries on the clamp,
  all +-float32(pi), and none in the band that only the fp64 restatement clamps; worst P_DELTA err / e32 over the other entries 1.01 on each task, no column above
  the 2 eps32 floor;
* full state: nbad 13 / 10 / 0 / 0 against nbad_f32 10 / 10 / 0 / 0, every one explained, none sent to
  the deep draw; contact-active outlier fraction against f64 1.60 / 1.04 / 0 / 0 % (f32 oracle 1.26 /
  1.15 / 0 / 0 %), median err/tol 0.0027 / 0.0021 / 0.0015 / 0.0014 (0.0015 / 0.0015 / 0.0009 / 0.0007);
* post-step state of the device: joint speed limit 19-21 % of the surviving entries per sign (the
  manager 0.3 / 0.02 %, not asserted: tests/test_limit_cases.py), angular cap 76 / 75 / 81 / 21 % of the
  surviving envs, wraps 12+25 / 12+23 / 24+19 / 73+65 -- the f64 oracle's figures;
* the whole file takes 3 s.
"""
from __future__ import annotations

import numpy as np
import pytest

import limit_cases as L
import test_gpu_fullstate as F
from fullstate import TASKS, base_task, product, task_cfg

pytestmark = pytest.mark.gpu

# the limit branches on a post-step state (limit_cases.post_step_coverage). The joint speed limit only
# for the tasks whose post-step state holds it: the manager's drive (delta clipped at 0.04 pi, kd 0.5)
# leaves no joint at its velocity_limit after four substeps (tests/test_limit_cases.py)
POST_SPEED, POST_OMEGA, POST_WRAPS = 0.05, 0.10, 8


def assert_post_step(task, cov, label):
    if base_task(task) != "manager":
        assert cov["speed_hi"] >= POST_SPEED and cov["speed_lo"] >= POST_SPEED, (task, label, cov)
    assert cov["omega_cap"] >= POST_OMEGA, (task, label, cov)
    assert cov["wrap_hi"] >= POST_WRAPS and cov["wrap_lo"] >= POST_WRAPS, (task, label, cov)


def full_check(task, c, g_out, sg, label):
    """The full-state rule on a device's step of case ``c`` (kind "full"), the outlier cap against the
    f32 oracle's own count, and the limit branches on the device's post-step state. Inside product()."""
    n = L.N
    stats = {}
    nbad = F._check(task, f"{label}: one step at the limits", n, L.HANDLE_SEED, np.array(c["st"]), [np.array(c["a"])],
                    g_out, sg, None, stats=stats)
    print(f"  [{task} {label}] nbad {nbad}, f32 oracle against f64 {stats['nbad_f32']}")
    assert nbad <= F.AGG_FRAC_K * stats["nbad_f32"] + 0.005 * n, (nbad, stats["nbad_f32"])
    reset = np.asarray(g_out[2]) | np.asarray(g_out[3])
    cov = L.post_step_coverage(c["limits"], c["st"], sg, reset)
    print(f"  [{task} {label}] post-step: {cov}, reset {reset.mean():.1%}")
    assert_post_step(task, cov, label)
    assert np.isfinite(sg).all() and np.isfinite(g_out[0]).all() and np.isfinite(g_out[1]).all()
    return nbad, stats, cov


def _variant(task):
    return (1, 1, 0, 1 if base_task(task) in ("v2", "standup") else 0)


def _step(task, c, monkeypatch):
    import torch
    from zbot_lab_amd.sim import ZbotSim
    monkeypatch.delenv("ZB_OCC1", raising=False)
    g = ZbotSim(L.N, task_cfg(task), device="cuda:0", seed=L.HANDLE_SEED)
    assert g.kernel_variant() == _variant(task), (task, g.kernel_variant())
    g.set_state(torch.from_numpy(np.array(c["st"])).cuda())
    obs, rew, te, tr = g.step(torch.from_numpy(np.array(c["a"])).cuda())
    out = (obs.cpu().numpy(), rew.cpu().numpy(), te.cpu().numpy().copy(), tr.cpu().numpy().copy())
    sg = g.get_state().cpu().numpy()
    g.close()
    return out, sg


@pytest.mark.parametrize("task", TASKS)
def test_action_prologue_exact(gpu, monkeypatch, task):
    c = L.case(task, "prologue")
    with product():
        out, sg = _step(task, c, monkeypatch)
    L.check_prologue(task, c, sg, out[2] | out[3])


@pytest.mark.parametrize("task", TASKS)
def test_full_state_at_limits(gpu, monkeypatch, task):
    c = L.case(task, "full")
    with product():
        out, sg = _step(task, c, monkeypatch)
        full_check(task, c, out, sg, "device")


@pytest.mark.parametrize("task", ["v2", "manager"])
def test_limits_deterministic(gpu, monkeypatch, task):
    """The joint wrap is written twice in the kernel (advance_pose's branches, the substep's selects)
    and both run within one step: the same step twice from the same state, every output and state row
    bit-identical."""
    c = L.case(task, "full")
    with product():
        out1, s1 = _step(task, c, monkeypatch)
        out2, s2 = _step(task, c, monkeypatch)
    for x, y in zip(out1 + (s1,), out2 + (s2,)):
        np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                      y.view(np.uint32) if y.dtype == np.float32 else y)
