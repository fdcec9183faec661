"""The contact-free dynamics against an independent float64 reference (tests/dynamics_reference.py:
d'Alembert / Kane over the 12 authored links; no composite, no pack_model mass row, nothing of the
oracle). No GPU.

1. The reference against itself: geometric vs finite-difference Jacobians, M symmetric positive
   definite, total mass, Newton's third law (momentum balance under arbitrary joint torques), step-size
   insensitivity.
2. The f64 oracle against the reference, one and four substeps, five models x six case sets (+ gravity
   0), each set's condition asserted on the reference's own outcome. Tolerance per entry:
   2 ulp32(max(|x|, 1)) for the oracle's float32 state interface + 10 x the reference's own step-size
   sensitivity on that case set (its result with the J' u step tripled). The oracle handle gets its mass
   properties and joint frames in double (zbo_set_model_f64): with zb_model's float32 rows the f64 oracle
   is 2^-24 relative off on every model row, which a saturated joint's substep amplifies to 5.5e-6
   (17 x this tolerance) while the generic set stays at 5.1e-7. Measured with the double rows: every
   model, set and substep count at 0.25-0.27 of 2 ulp32, i.e. the float32 rounding of the state read
   back and nothing else.
   The packed path is held separately: the f64 oracle on pack_model's float32 rows (no setter) against
   the reference within that tolerance + 10 x the reference's move under a 2^-24 relative perturbation
   of every model input, on every set and on the GPU test's 130 mixed states.
3. Sensitivity: each planted error of the reference (MUTANTS) misses the f64 oracle by >= 10 x the
   tolerance on at least half the envs.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import dynamics_reference as D
from test_base_inertia_cfg import HEAVY
from zbot_lab_amd import model as zm

S, NPHYS, ND = zm.S, D.NPHYS, zm.NUM_DOF
LIGHT = (0.15, (0.0, 0.03, 0.0))   # tests/test_gpu_base_inertia.py's light / sideways class
NEAR = 1e-5                        # a decision this close (relative) to its threshold may differ by rounding


def _manager(**kw):
    return zm.TaskCfg.manager_flat(**{"solver_mode": 1, "self_manifold": 2, **kw})


# name -> (robot model, task cfg factory, base inertia or None)
MODELS = {
    "walking-v2": (zm.load_model, lambda **kw: zm.TaskCfg(**{"solver_mode": 1, **kw}), None),
    "standup": (zm.standup_model, lambda **kw: zm.TaskCfg.standup(**{"solver_mode": 1, **kw}), None),
    "manager": (zm.load_v09_model, _manager, None),
    "manager-heavy": (zm.load_v09_model, _manager, HEAVY),
    "manager-light-lateral": (zm.load_v09_model, _manager, LIGHT),
}


@functools.lru_cache(maxsize=None)
def robot(name):
    return MODELS[name][0]()


def oracle_robot(name):
    """The model the simulators are built on: the composite re-summed by with_base_inertia."""
    base = MODELS[name][2]
    return robot(name) if base is None else zm.with_base_inertia(robot(name), *base)


def make_cfg(name, **kw):
    return MODELS[name][1](**{"enable_self_collision": False, **kw})


def reference(name, cfg, mutant=None, base="model", round_model=False):
    c = cfg.pack()
    return D.Reference(robot(name), c.sim_dt, c.gravity, base=MODELS[name][2] if base == "model" else base, mutant=mutant,
                       round_model=round_model)


def oracle_substeps(name, cfg, rows, targets, nsubs=(1, 4), double=True, f64_model=True, state_rows=None, forces=None):
    """The physics rows after each of ``nsubs`` substeps (cumulative) and the applied torque of the last
    call, from the C oracle on ``oracle_robot(name)``; the f64 build with the model rows in double unless
    ``f64_model`` is off (then it reads pack_model's float32 rows, as the f32 oracle and the device do).
    ``state_rows`` {first row: [k, n] array} fills further state rows (the per-link friction of the
    stand-up and manager tasks); ``forces``: a dict that receives, per entry of ``nsubs``, the per-link
    net contact force [n, 12, 3] of that call's last substep."""
    from oracle import pyoracle
    lib = pyoracle.lib(double)
    rm = oracle_robot(name)
    m, c = zm.pack_model(rm), cfg.pack()
    n = rows.shape[1]
    h = lib.zbo_create(C.byref(m), C.byref(c), n, 0)
    try:
        if double and f64_model:
            pyoracle.set_model_f64(lib, h, rm)
        st = np.zeros((cfg.state_dim, n), np.float32)
        st[:NPHYS] = rows
        for first, block in (state_rows or {}).items():
            st[first:first + len(block)] = block
        lib.zbo_set_state(h, st)
        out, done = {}, 0
        at = np.zeros((n, ND), np.float32)
        seps = []
        for k in nsubs:
            sep = np.zeros(n, np.float32)
            lib.zbo_self_min_sep(h, sep)
            seps.append(sep)
            nf = np.zeros((n, zm.NUM_LINKS, 3), np.float32)
            lib.zbo_physics_substeps(h, np.ascontiguousarray(targets, np.float32), k - done,
                                     nf.ctypes.data_as(C.c_void_p) if forces is not None else None, at.ctypes.data_as(C.c_void_p))
            if forces is not None:
                forces[k] = nf
            done = k
            got = np.zeros_like(st)
            lib.zbo_get_state(h, got)
            out[k] = got[:NPHYS].copy()
        sep = np.zeros(n, np.float32)
        lib.zbo_self_min_sep(h, sep)
        seps.append(sep)
    finally:
        lib.zbo_destroy(h)
    return out, at, np.array(seps)


@functools.lru_cache(maxsize=None)
def reference_run(name, case, n, gravity=None, seed=0):
    """(rows, targets, reference result of 4 substeps, per-substep step-size sensitivity [4, 25, 1])."""
    cfg = make_cfg(name) if gravity is None else make_cfg(name, gravity=gravity)
    rows, tg = (D.mixed_states(robot(name), n, seed) if case == "mixed" else D.case_states(robot(name), case, n, seed))
    ref = reference(name, cfg)
    r = ref.run(rows, tg, 4)
    r3 = ref.run(rows, tg, 4, eps_jdot=3 * D.EPS_JDOT)
    sens = np.abs(r["states"] - r3["states"]).max(axis=2, keepdims=True)   # per row, over the set
    return rows, tg, r, sens


def tolerance(ref_states, sens):
    return 2.0 * D.ulp32(ref_states) + 10.0 * sens


@functools.lru_cache(maxsize=None)
def rounding_sensitivity(name, case, n, gravity=None, seed=0):
    """Per substep and row, over the set: how far the reference moves when its own model inputs (authored
    mass properties, joint and link frames) are rounded to float32 [4, 25, 1]."""
    cfg = make_cfg(name) if gravity is None else make_cfg(name, gravity=gravity)
    rows, tg, r, _ = reference_run(name, case, n, gravity, seed)
    rr = reference(name, cfg, round_model=True).run(rows, tg, 4)
    return np.abs(r["states"] - rr["states"]).max(axis=2, keepdims=True)


def packed_tolerance(ref_states, sens, rsens):
    """For a float64 computation on pack_model's float32 rows: the tolerance above plus 10 x the reference's
    own sensitivity to float32 rounding of its model inputs (the same factor as for its step size: the
    packed rows are rounded after the composite sum, not link by link, so the two roundings differ in
    detail, not in size)."""
    return tolerance(ref_states, sens) + 10.0 * rsens


def near_share(r, nsub=4):
    """Share of the reference's decisions (saturation, speed clamp, wrap per joint; cap per env) within
    NEAR of their threshold, over the first ``nsub`` substeps."""
    m = np.concatenate([r[k][:nsub].reshape(-1) for k in ("sat_margin", "clamp_margin", "wrap_margin", "cap_margin")])
    return float((m < NEAR).mean())


# ------------------------------------------------------------------ 1. the reference against itself
def _one_state(name, case, e=0):
    rows, tg = D.case_states(robot(name), case, 4, seed=3)
    return rows[:, e].astype(np.float64), tg[e].astype(np.float64)


def _split(x):
    u = np.concatenate([x[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3], x[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3],
                        x[S["JOINT_VEL"]:S["JOINT_VEL"] + ND]])
    return x[S["ROOT_POS"]:S["ROOT_POS"] + 3], zm.qnorm(x[S["ROOT_QUAT"]:S["ROOT_QUAT"] + 4]), x[S["JOINT_POS"]:S["JOINT_POS"] + ND], u


@pytest.mark.parametrize("name", ["walking-v2", "manager-heavy"])
def test_reference_jacobians_mass_matrix_total_mass(name):
    ref = reference(name, make_cfg(name))
    for e in range(2):
        pos, quat, q, u = _split(_one_state(name, "generic", e)[0])
        Jv, Jw, _, _ = ref.jac_geometric(pos, quat, q)
        Fv, Fw, _, _ = ref.jac_fd(pos, quat, q)
        dj = max(np.abs(Jv - Fv).max(), np.abs(Jw - Fw).max())
        d = ref.dynamics(pos, quat, q, u)
        M = d["M"]
        print(f"\n[{name}] geometric vs finite-difference Jacobian {dj:.3g}; M asymmetry {np.abs(M - M.T).max():.3g}, "
              f"smallest eigenvalue {np.linalg.eigvalsh(M).min():.3g}")
        assert dj <= 1e-8
        assert np.abs(M - M.T).max() <= 1e-14 * np.abs(M).max() and np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0
        links = robot(name).raw["links"]
        total = sum(l["mass"] for l in links)
        if MODELS[name][2] is not None:
            total += MODELS[name][2][0] - links[robot(name).base_link]["mass"]
        assert ref.mass.sum() == pytest.approx(total, rel=1e-15)
        np.testing.assert_allclose(M[0:3, 0:3], total * np.eye(3), rtol=0, atol=1e-13)
        assert total == pytest.approx(oracle_robot(name).body_mass.sum(), rel=1e-14)


@pytest.mark.parametrize("case", ["generic", "gyroscopic"])
@pytest.mark.parametrize("name", ["walking-v2", "manager-heavy"])
def test_reference_momentum_balance(name, case):
    """Newton's third law: joint torques are internal, so under any of them the links' summed m a is the
    weight and their summed moment of momentum rate is the weight's moment. Checks C against M."""
    ref = reference(name, make_cfg(name))
    rng = np.random.default_rng(4)
    worst = 0.0
    for e in range(3):
        x, _ = _one_state(name, case, e)
        (f, fw), (mo, mw) = ref.momentum_balance(x, rng.uniform(-20.0, 20.0, ND))
        terms = ref.dynamics(*_split(x))
        scale_f = max(np.linalg.norm(fw), np.abs(ref.mass[:, None] * terms["jdv"]).sum())
        scale_m = max(np.linalg.norm(mw), np.abs(np.cross(terms["c"], ref.mass[:, None] * terms["jdv"])).sum())
        worst = max(worst, np.abs(f - fw).max() / scale_f, np.abs(mo - mw).max() / scale_m)
    print(f"\n[{name} {case}] momentum balance, worst relative residual {worst:.3g}")
    assert worst <= 1e-8


def test_reference_is_insensitive_to_its_difference_steps():
    ref = reference("walking-v2", make_cfg("walking-v2"))
    worst = 0.0
    for e in range(2):
        x, tg = _one_state("walking-v2", "generic", e)
        a, _ = ref.substep(x, tg, jac="fd")
        b, _ = ref.substep(x, tg, jac="fd", eps_j=3 * D.EPS_J, eps_jdot=3 * D.EPS_JDOT)
        worst = max(worst, np.abs(a - b).max())
    print(f"\nsubstep with both difference steps tripled moves by {worst:.3g}")
    assert worst < 1e-9


# ------------------------------------------------------------------ 2. the f64 oracle against the reference
def _conditions(case, r, rows, name):
    pm = zm.pack_model(robot(name))
    if case == "generic":
        assert not r["sat"].any() and not r["clamp"].any() and not r["cap"].any() and not r["wrap"].any()
    if case == "gyroscopic":
        w = np.linalg.norm(rows[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3], axis=0)
        assert w.max() > 0.9 * pm.max_angular_velocity and w.max() < pm.max_angular_velocity
        assert np.abs(rows[S["JOINT_VEL"]:S["JOINT_VEL"] + ND]).max() > 13.0
    if case == "saturated":
        assert (r["sat"] > 0).sum() >= 20 and (r["sat"] < 0).sum() >= 20
    if case == "speed_clamp":
        assert (r["clamp"] > 0).sum() >= 20 and (r["clamp"] < 0).sum() >= 20
    if case == "angular_cap":
        assert r["cap"][0].sum() >= 3 and (~r["cap"][0]).sum() >= 3
    if case == "wrap":
        assert (r["wrap"] > 0).sum() >= 20 and (r["wrap"] < 0).sum() >= 20


def _case_n(case):
    return 64 if case == "saturated" else 16


CASES = [(c, None) for c in D.CASE_SETS] + [("generic", 0.0)]


@pytest.mark.parametrize("case,gravity", CASES, ids=[c if g is None else f"{c}-gravity0" for c, g in CASES])
@pytest.mark.parametrize("name", list(MODELS))
def test_f64_oracle_matches_reference(oracle_lib, name, case, gravity):
    n = _case_n(case)
    rows, tg, r, sens = reference_run(name, case, n, gravity)
    _conditions(case, r, rows, name)
    assert near_share(r) <= 0.02
    cfg = make_cfg(name) if gravity is None else make_cfg(name, gravity=gravity)
    got, at, _ = oracle_substeps(name, cfg, rows, tg)
    worst = {}
    for k in (1, 4):
        ref_state = r["states"][k - 1]
        ratio = np.abs(got[k].astype(np.float64) - ref_state) / tolerance(ref_state, sens[k - 1])
        worst[k] = float(ratio.max())
    t_err = float(np.abs(at.astype(np.float64) - r["applied"]).max() / (2 * D.ulp32(r["applied"])).min())
    print(f"\n[{name} {case}{'' if gravity is None else ' gravity 0'}] f64 oracle vs reference, worst error / tolerance: "
          f"1 substep {worst[1]:.3g}, 4 substeps {worst[4]:.3g}; applied torque {t_err:.3g}; step sensitivity {sens.max():.3g}; "
          f"saturated {int((r['sat'] != 0).sum())}, clamped {int((r['clamp'] != 0).sum())}, capped {int(r['cap'].sum())}, "
          f"wrapped {int((r['wrap'] != 0).sum())}")
    assert worst[1] <= 1.0 and worst[4] <= 1.0
    assert np.abs(at.astype(np.float64) - r["applied"]).max() <= (2 * D.ulp32(np.abs(r["applied"]).max()))


@pytest.mark.parametrize("case", list(D.CASE_SETS) + ["mixed"])
@pytest.mark.parametrize("name", list(MODELS))
def test_packed_model_matches_reference(oracle_lib, name, case):
    """The absolute anchor of load_model / with_base_inertia / pack_model / load_mdl: the f64 oracle on
    pack_model's float32 rows (the rows the f32 oracle and the device read, through the same load_mdl)
    against the reference, on every case set and on the 130 mixed states of tests/test_gpu_dynamics.py."""
    n = 130 if case == "mixed" else _case_n(case)
    rows, tg, r, sens = reference_run(name, case, n)
    rsens = rounding_sensitivity(name, case, n)
    got, _, _ = oracle_substeps(name, make_cfg(name), rows, tg, f64_model=False)
    for k in (1, 4):
        ref_state = r["states"][k - 1]
        err = np.abs(got[k].astype(np.float64) - ref_state)
        ratio = err / packed_tolerance(ref_state, sens[k - 1], rsens[k - 1])
        print(f"\n[{name} {case}] f64 oracle on the packed float32 rows vs reference, {k} substep(s): worst error {err.max():.3g}, "
              f"worst error / bound {ratio.max():.3g} (float32 rounding of the reference's inputs moves it by {rsens[k - 1].max():.3g})")
        assert ratio.max() <= 1.0


def test_model_f64_rows_are_the_packed_rows():
    """zbo_set_model_f64's rows, rounded to float32, are pack_model's rows in pack_model's order."""
    from oracle import pyoracle
    for name in MODELS:
        rm = oracle_robot(name)
        m = zm.pack_model(rm)
        packed = np.concatenate([np.ctypeslib.as_array(getattr(m, f)).reshape(-1) for f in
                                 ("body_mass", "body_com", "body_inertia", "joint_parent_pos", "joint_parent_rot",
                                  "joint_child_pos", "joint_child_rot")])
        np.testing.assert_array_equal(pyoracle.model_f64(rm).astype(np.float32), packed.astype(np.float32))


def test_default_cfg_with_self_collision_on(oracle_lib):
    """The default cfg (self collision on) on near-default poses: no pair within 10 mm before or after, so
    the contact-free statement holds with the detection running."""
    name = "walking-v2"
    rm = robot(name)
    rng = np.random.default_rng(6)
    n = 16
    rows, tg = D.case_states(rm, "generic", n, seed=6)
    q = rm.default_joint_pos[None, :] + rng.uniform(-0.02, 0.02, (n, ND))
    rows[S["JOINT_POS"]:S["JOINT_POS"] + ND] = q.T
    rows[S["JOINT_VEL"]:S["JOINT_VEL"] + ND] *= 0.3
    tg = (q + rng.uniform(-0.05, 0.05, (n, ND))).astype(np.float32)
    cfg = make_cfg(name, enable_self_collision=True)
    ref = reference(name, cfg)
    r = ref.run(rows, tg, 4)
    sens = np.abs(r["states"] - ref.run(rows, tg, 4, eps_jdot=3 * D.EPS_JDOT)["states"]).max(axis=2, keepdims=True)
    got, _, seps = oracle_substeps(name, cfg, rows, tg)
    assert seps.min() > 0.010
    for k in (1, 4):
        ratio = np.abs(got[k].astype(np.float64) - r["states"][k - 1]) / tolerance(r["states"][k - 1], sens[k - 1])
        print(f"\n[default cfg] {k} substep(s): worst error / tolerance {ratio.max():.3g}, min self separation {seps.min() * 1e3:.1f} mm")
        assert ratio.max() <= 1.0


@pytest.mark.parametrize("name", ["walking-v2", "standup", "manager", "manager-heavy"])
def test_mixed_states_leave_few_decisions_near_a_threshold(name):
    """The 130 states of tests/test_gpu_dynamics.py: at most 2 % of the reference's decisions lie within
    1e-5 (relative) of their threshold, and every branch occurs."""
    _, _, r, _ = reference_run(name, "mixed", 130)
    share = near_share(r)
    print(f"\n[{name}] decisions within {NEAR:g} of a threshold: {share:.4%}")
    assert share <= 0.02
    for k in ("sat", "clamp", "wrap"):
        assert (r[k] > 0).any() and (r[k] < 0).any()
    assert r["cap"].any()


# ------------------------------------------------------------------ 3. sensitivity
MUTANT_SET = {"inertia": "saturated", "com": "saturated", "no_gyro": "generic", "no_jdot": "generic",
              "no_armature": "generic", "kd_only": "generic", "root_gravity": "generic"}


@pytest.mark.parametrize("mutant", list(D.MUTANTS))
def test_planted_errors_fail(oracle_lib, mutant):
    name, case = "walking-v2", MUTANT_SET[mutant]
    rows, tg, r, sens = reference_run(name, case, _case_n(case))
    cfg = make_cfg(name)
    got, _, _ = oracle_substeps(name, cfg, rows, tg, nsubs=(1,))
    bad = reference(name, cfg, mutant=mutant).run(rows, tg, 1)["states"][0]
    ratio = (np.abs(got[1].astype(np.float64) - bad) / tolerance(r["states"][0], sens[0])).max(axis=0)   # per env
    print(f"\n[mutant {mutant}: {D.MUTANTS[mutant]}, set {case}] error / tolerance per env: median {np.median(ratio):.3g}, "
          f"min {ratio.min():.3g}, max {ratio.max():.3g}; envs at >= 10: {int((ratio >= 10).sum())} of {len(ratio)}")
    assert (ratio >= 10.0).mean() >= 0.5
