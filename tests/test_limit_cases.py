"""CPU side of the limit tests (tests/test_gpu_limits.py): the conditions on their inputs, and that
their rules catch planted faults, with an oracle build standing in for the device (as
tests/test_fullstate_machinery.py does for the full-state rule). Same seeds and sizes as the GPU tests
(tests/limit_cases.case: 1024 envs, product cfg).

Coverage is a condition on the inputs, measured on the f64 oracle (limit_cases.coverage): each p_delta
clamp side >= 5 % of entries, each manager clip side >= 10 %, every joint's drive saturated at each
sign in >= 10 % of envs with all 64 joint masks present, the joint speed limit at each sign in >= 5 %
of surviving entries, the angular cap in >= 10 % of surviving envs, >= 8 wrapped entries per sign,
>= 60 % of envs survive, every output finite. A task that misses a condition at the common planted
shares gets shares of its own (limit_cases.TASK_SHARES: the manager, whose angular cap is held by 4.5 %
of the surviving envs at the common shares and by 21 % at its own). Two conditions no share meets on the
manager. Its drive cannot saturate: the delta is clipped at 0.04 pi, so |tau| <= kp 0.04 pi + kd
velocity_limit = 7.5 of 20. And it damps a planted joint speed below the limit within a substep
(kd 0.5 on light links), so after the step 0.3 % of the entries hold the limit at any share; the speed
clamp acts inside the step only. For the manager the speed condition is therefore asserted on the first
substep, as a count like the wraps': at least 8 entries per sign at +-velocity_limit after one
physics_substeps (measured 210 / 57 of 6144; at 95 % planted 3.2 % / 1.7 % touch it in any substep, so
the 5 % share is out of reach there too). The planted velocity_limit fault below shows the full-state
rule sees that clamp through the physics rows.

Measured (f64 oracle, 1024 envs; v2 / v4 / stand-up / manager): p_delta sides 9.4 / 9.7 % (the three
tanh tasks), clip sides 45.1 / 44.5 %; saturation per joint and sign 29-36 %, 64 masks; speed limit
after the step 19-21 % per sign (manager 0.3 / 0 %; after its first substep 210 / 57 entries); angular
cap 75.9 / 75.2 / 81.3 / 21.0 %; wraps 12+25 / 12+23 / 24+19 / 73+65; terminated 15.2 / 10.7 / 22.6 /
32.0 %. Baseline (f32 against f64 oracle) outliers 1.07 / 0.98 / 0 / 0 %. Planted limit faults:
493-719 unexplained envs on the tanh tasks, 55 (velocity_limit) and 273 (max_angular_velocity) on the
manager.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import limit_cases as L
import test_gpu_limits as G
from fullstate import TASKS, base_task, compare, product, task_cfg

TANH = L.TANH_TASKS


def test_action_table():
    t = L.action_table()
    assert t.dtype == np.float32 and not np.isnan(t).any() and len(t) == 40
    assert (np.sort(t[:20]) == np.sort(-t[20:])).all() and np.signbit(t[20]) and not np.signbit(t[0])
    edge = np.arctanh(1.0 - 2.0 ** -25)  # float32 tanh rounds to 1 from here on
    three = t[9:12].astype(np.float64)
    assert three[0] < three[1] < three[2] and three[0] < edge < three[2]
    assert (L.tanh32(t[9:12]) == [np.nextafter(np.float32(1), np.float32(0)), 1, 1]).all() or \
        (L.tanh32(t[9:12]) == [np.nextafter(np.float32(1), np.float32(0))] * 2 + [1]).all()
    a = L.limit_actions(L.N, 1)
    for j in range(6):  # every table value (bit pattern) in every joint column
        assert set(t.view(np.uint32)) <= set(a[:, j].view(np.uint32))


@pytest.mark.parametrize("kind", ["full", "prologue"])
def test_actions_are_tie_free(oracle_lib, kind):
    """For every action the tests send, tanh(float64(a)) is not within 2^-48 relative of a float32
    rounding tie: its float32 rounding does not depend on the last bits of the double evaluation, which
    entitles test_action_prologue_exact to demand bit equality."""
    for task in TANH:
        a = L.case(task, kind)["a"].astype(np.float64).ravel()
        t = np.tanh(a)
        f = t.astype(np.float32)
        for side in (np.float32(np.inf), np.float32(-np.inf)):
            mid = 0.5 * (f.astype(np.float64) + np.nextafter(f, side).astype(np.float64))
            ok = (np.abs(t - mid) > 2.0 ** -48 * np.abs(t)) | (t == 0)
            assert ok.all(), (task, a[~ok][:4])


@pytest.mark.parametrize("task", TASKS)
def test_coverage(oracle_lib, task):
    c = L.case(task, "full")
    with product():
        cov = L.coverage(task, c["st"], c["a"], seed=L.HANDLE_SEED)
    print(f"\n[{task}] coverage: " + ", ".join(f"{k} {np.round(np.asarray(v, float), 3)}" for k, v in cov.items()))
    assert cov["finite"] and cov["terminated"] <= 0.40
    assert cov["wrap_hi"] >= 8 and cov["wrap_lo"] >= 8
    assert cov["omega_cap"] >= 0.10
    if base_task(task) == "manager":
        assert cov["clip_hi"] >= 0.10 and cov["clip_lo"] >= 0.10
        # the speed clamp inside the step (module docstring): entries at the limit after the first substep
        assert cov["touch_hi"] >= 8 and cov["touch_lo"] >= 8
        G.assert_post_step(task, cov, "f64 oracle")
        return
    assert cov["pdel_hi"] >= 0.05 and cov["pdel_lo"] >= 0.05
    assert (cov["sat_hi"] >= 0.10).all() and (cov["sat_lo"] >= 0.10).all() and cov["sat_masks"] == 64
    assert cov["speed_hi"] >= 0.05 and cov["speed_lo"] >= 0.05
    # the same conditions, as the GPU test re-asserts them on the device's post-step state
    G.assert_post_step(task, cov, "f64 oracle")


@pytest.mark.parametrize("task", TASKS)
def test_prologue_case(oracle_lib, task):
    """The prologue case's conditions: at most 5 % of its envs reset (on the oracle; the GPU test asserts
    it again on the device's flags), both clamp (clip) sides present in every joint column, and the
    f64 oracle passes the exactness rules as the device."""
    c = L.case(task, "prologue")
    te, tr = c["out32"][2:]
    assert (te | tr).mean() <= 0.05
    pro = c["pro"]
    hi, lo = pro["raw"] >= pro["lim"], pro["raw"] <= -pro["lim"]
    assert (hi.mean(axis=1) >= 0.05).all() and (lo.mean(axis=1) >= 0.05).all(), (hi.mean(axis=1), lo.mean(axis=1))
    got = L.check_prologue(task, c, c["s64"], c["out64"][2] | c["out64"][3], "f64 oracle")
    if base_task(task) == "manager":
        # the restated clip against the oracle's own processed actions: clip-side entries exactly +-clip
        from oracle.pyoracle import m_process_actions
        with product():
            proc, _ = m_process_actions(task_cfg(task), c["a"], c["st"][13:19].T)
        clip = np.float32(task_cfg(task).action_clip)
        assert (proc.T[hi] == clip).all() and (proc.T[lo] == -clip).all()
        assert np.abs(proc.T - pro["delta"]).max() <= 2 * L.EPS32 * float(clip)
    else:
        assert got["n_clamped"] >= 0.10 * 6 * L.N


@pytest.mark.parametrize("task", TASKS)
def test_baseline(oracle_lib, task):
    """The f32 oracle against the f64 oracle on the limit states under fullstate.compare: at most 2 %
    of the envs outside tolerance, so the GPU test's relative cap is not run where the reference itself
    is unstable."""
    c = L.case(task, "full")
    with product():
        ob, rw, te, tr = c["out32"]
        od, rd, ted, trd = c["out64"]
        ratio, *_, flags_bad = compare(task, c["s32"], c["s64"], ob, od, rw, rd, (te, tr), (ted, trd), c["st"])
    frac = float((ratio > 1).mean())
    print(f"\n[{task}] f32 against f64 oracle at the limits: {frac:.2%} outside tolerance, flags differ in "
          f"{int(flags_bad.sum())} envs")
    assert not np.isnan(ratio).any()
    assert frac <= 0.02


def _standin(task, c, model_edit=None, a=None):
    """The f64 oracle's step of case ``c`` as the device, with one edit of its model or actions."""
    from oracle.pyoracle import OracleSim
    d = OracleSim(L.N, task_cfg(task), seed=L.HANDLE_SEED, double=True)
    if model_edit:
        model_edit(d._m)
        d.lib.zbo_destroy(d.h)
        d.h = d.lib.zbo_create(C.byref(d._m), C.byref(d._c), L.N, L.HANDLE_SEED)
    d.set_state(np.array(c["st"]))
    out = d.step(np.array(c["a"]) if a is None else a)
    return out, d.get_state()


@pytest.mark.parametrize("task", TASKS)
def test_f64_oracle_passes_at_limits(oracle_lib, task):
    c = L.case(task, "full")
    with product():
        out, sg = _standin(task, c)
        G.full_check(task, c, out, sg, "f64 oracle")


def _vlim(m):
    m.velocity_limit *= 1.01


def _wmax(m):
    m.max_angular_velocity *= 1.01


@pytest.mark.parametrize("fault", ["velocity_limit", "max_angular_velocity"])
@pytest.mark.parametrize("task", TASKS)
def test_planted_limit_faults_are_caught(oracle_lib, task, fault):
    """A stand-in device whose joint speed limit or angular cap is 1 % off fails the full check."""
    c = L.case(task, "full")
    with product():
        out, sg = _standin(task, c, model_edit=_vlim if fault == "velocity_limit" else _wmax)
        with pytest.raises(AssertionError, match="oracle is stable"):
            G.full_check(task, c, out, sg, f"planted {fault} x 1.01")


@pytest.mark.parametrize("task", TASKS)
def test_planted_prologue_faults_are_caught(oracle_lib, task):
    """The exactness rules fail on a stand-in whose tanh is a few ulp off below saturation (its action
    column scaled by 1 + 2^-20) and on one whose P_DELTA clamp sits at pi (1 - 1e-5). The moved clamp
    is planted in the stand-in's P_DELTA rows only (its drive targets and physics are the unedited
    oracle's) and is shown to fail check_prologue's bit rule; that the full-state rule would catch it
    is not shown (3.1e-5 against that rule's 2.6e-5 tolerance on the row)."""
    c = L.case(task, "prologue")
    with product():
        with np.errstate(over="ignore"):  # (FLT_MAX scales to inf)
            a = (c["a"].astype(np.float64) * (1 + 2.0 ** -20)).astype(np.float32)
        out, sg = _standin(task, c, a=a)
        with pytest.raises(AssertionError, match="ACTIONS entries differ"):
            L.check_prologue(task, c, sg, out[2] | out[3], "planted action scale")
        if base_task(task) == "manager":
            return
        D = L._layout(task)
        sg = np.array(c["s64"])
        lim = np.float32(np.pi * (1 - 1e-5))
        sg[D["P_DELTA"]:D["P_DELTA"] + 6] = np.clip(sg[D["P_DELTA"]:D["P_DELTA"] + 6], -lim, lim)
        with pytest.raises(AssertionError, match="off \\+-float32"):
            L.check_prologue(task, c, sg, c["out64"][2] | c["out64"][3], "planted clamp")
