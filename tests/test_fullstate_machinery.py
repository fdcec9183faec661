"""CPU check of the full-state parity machinery (tests/fullstate.py) that test_gpu_fullstate.py runs
against the HIP kernels: with the f64 oracle standing in for the device, every env agrees or is an
explained discontinuity; a planted error of the size a wrong weight / latch / integrator would
cause is reported as unexplained; and a device carrying a planted contact-path bug (one ground
contact's friction x 1.1, one self contact's normal flipped, the push-out cap removed) is caught in
the contact-active envs where the bug acts, however sensitive those envs are; bugs in the rare
branches (rim-manifold ends, face-manifold samples, the overlapping-core axis), which act in a few
envs only, are caught through the deep draw's membership rule."""
from __future__ import annotations

import re

import numpy as np
import pytest

import test_gpu_fullstate as T
from fullstate import TASKS, compare, random_states, row_groups, task_cfg


def _device_f64(task, n, seed, st, actions):
    from oracle.pyoracle import OracleSim
    d = OracleSim(n, task_cfg(task), seed=seed, double=True)
    d.set_state(st)
    for a in actions:
        out = d.step(a)
    return out, d.get_state()


@pytest.mark.parametrize("task", TASKS + ("v2:step0",))
def test_f64_oracle_passes_full_state_check(oracle_lib, task):
    from oracle.pyoracle import OracleSim
    n, seed = 512, 17  # (the 2 % outlier bound over 512 envs: a one-env fluctuation is not a failure)
    st = random_states(task, OracleSim(n, task_cfg(task), seed=seed), n, seed=101)
    a = np.random.default_rng(7).normal(size=(n, 6)).astype(np.float32)
    out, sg = _device_f64(task, n, seed, st, [a])
    assert T._check(task, "f64 oracle as device", n, seed, st, [a], out, sg, None) <= 0.02 * n


@pytest.mark.parametrize("task", TASKS)
def test_planted_errors_are_unexplained(oracle_lib, task):
    from oracle.pyoracle import OracleSim
    n, seed = 256, 17
    st = random_states(task, OracleSim(n, task_cfg(task), seed=seed), n, seed=101)
    a = np.random.default_rng(7).normal(size=(n, 6)).astype(np.float32)
    out, sg = _device_f64(task, n, seed, st, [a])
    g = row_groups(task)
    sg = sg.copy()
    # plant into envs where the oracle is stable (no contact discontinuity nearby) and that do not
    # reset in the step, so every planted error must be reported as unexplained
    so, outs = T._run_oracle(task, n, seed, st, [a])
    ob_o, rw_o, te_o, tr_o = outs[-1]
    fam = T._sensitivity(task, n, seed, st, [a], so, ob_o, rw_o, (te_o, tr_o), st, 1)
    sens = np.max(np.stack(list(fam.values())), axis=0)
    calm = [int(e) for e in np.nonzero((sens < 0.3) & ~(te_o | tr_o))[0]]
    envs = [calm[k] for k in (1, 10, 20, 30)]
    sg[g["sums"][0], envs[0]] += 2e-2            # a per-term episode sum off by a weight-sized error
    sg[g["exact"][0], envs[1]] += 1e-3           # p_delta / raw action carry
    if g["kin"]:
        sg[g["kin"][0], envs[2]] += 5e-3          # a latch / integrator
    sg[g["phys_vel"][3], envs[3]] += 0.1         # a joint velocity
    with pytest.raises(AssertionError, match="oracle is stable") as ei:
        T._check(task, "planted", n, seed, st, [a], out, sg, None)
    listed = {int(v) for v in re.findall(r"\d+", str(ei.value).split(":")[-1].split("\n")[0])}
    for e in envs if g["kin"] else envs[:2] + envs[3:]:
        assert e in listed, (e, listed)


def _plant_states(task, kind, n, seed):
    """States where the planted bug acts: random full states (ground contacts, sliding feet) for the
    friction bug; folded states (links in contact) for the flipped self normal; random states sunk
    2-5 cm into the ground (push-out 0.2 x depth / dt = 0.8-2 m/s, above the 1 m/s cap) for the
    push-out cap."""
    from oracle.pyoracle import OracleSim
    o = OracleSim(n, task_cfg(task), seed=seed)
    st = random_states(task, o, n, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    if kind == 2:  # (the lying stand-up start loads fewer of its folds' pairs: wider folds)
        st[13:19] += rng.normal(0, 3.0 if task == "standup" else 1.5, (6, n)).astype(np.float32)
    if kind == 3:
        st[2] -= rng.uniform(0.02, 0.05, n).astype(np.float32)
    return st


@pytest.mark.parametrize("task", TASKS)
@pytest.mark.parametrize("kind", [1, 2, 3], ids=["ground_mu_x1.1", "self_normal_flipped", "no_pushout_cap"])
def test_planted_contact_bugs_are_caught(oracle_lib, task, kind):
    """The device is the f64 oracle with a planted contact-path bug (oracle zbo_set_plant); the
    checker is the unmodified f32 oracle with its perturbation envelope. The full-state rule must
    fail with unexplained envs, and every unexplained env must be one where the bug can act (a
    loaded contact of the planted kind in the device or the checker run: a flipped normal can
    unload a contact the checker loads): the rule flags contact-path bugs in
    contact-active, sensitive envs, not only calm ones."""
    from oracle.pyoracle import planted_bug
    n, seed = 256, 41
    st = _plant_states(task, kind, n, seed)
    a = np.random.default_rng(seed + 3).normal(size=(n, 6)).astype(np.float32)
    with planted_bug(kind, double=True):
        sg, outs, act = T._run_oracle(task, n, seed, st, [a], double=True, activity=True)
    act = act + T._run_oracle(task, n, seed, st, [a], activity=True)[2]   # either side's contacts
    where = act[:, 1] > 0 if kind == 2 else act[:, 0] > 0
    assert where.sum() >= 20, where.sum()
    with pytest.raises(AssertionError, match="oracle is stable") as ei:
        T._check(task, f"planted contact bug {kind}", n, seed, st, [a], outs[-1], sg, None)
    listed = {int(v) for v in re.findall(r"\d+", str(ei.value).split(": [")[-1])}
    assert listed and all(where[e] for e in listed), (sorted(listed), np.nonzero(where)[0][:20])


@pytest.mark.parametrize("task", ["v2", "standup"])
@pytest.mark.parametrize("kind", [4, 5, 6], ids=["rim_end_normal_flipped", "face_sample_1mm", "sat_no_centre_axis"])
def test_planted_rare_branch_bugs_are_caught(oracle_lib, task, kind):
    """A bug in a rare contact branch acts in a handful of envs only -- the case the deep draw's
    membership rule must not hide. The device is the f64 oracle with the bug planted
    (oracle zbo_set_plant: 4 the rim manifold's end points with flipped normals, 5 every face-manifold
    sample 1 mm off its face, 6 the overlapping-core estimate without the centre-difference axis);
    the batch is 60 standing states (no self contact) plus the first 4 of 64 constructed folds that
    reach the branch (tests/fullstate.constructed_states: rim / face / deep) in which the bug moves the
    step's result past tolerance. The check must fail, every env it lists must be one of those 4
    and each of them must be listed, and the failing envs must have gone through the deep draw."""
    from fullstate import constructed_states
    from oracle.pyoracle import OracleSim, planted_bug
    n_plain, n_cand, seed = 60, 64, 47
    cls = {4: "rim", 5: "face", 6: "deep"}[kind]

    def moved_by_bug(st, a):
        with planted_bug(kind, double=True):
            sg, outs = T._run_oracle(task, st.shape[1], seed, st, [a], double=True)
        clean, oc = T._run_oracle(task, st.shape[1], seed, st, [a], double=True)
        ob, rw, te, tr = outs[-1]
        return sg, outs, compare(task, sg, clean, ob, oc[-1][0], rw, oc[-1][1], (te, tr), oc[-1][2:], st)[0] > 1

    rng = np.random.default_rng(seed + 3)
    cand, _ = constructed_states(task, cls, n_cand, seed=seed + 2)
    ca = rng.normal(size=(n_cand, 6)).astype(np.float32)
    hot = np.nonzero(moved_by_bug(cand, ca)[2])[0][:4]
    assert len(hot) >= 1, f"the planted bug moves none of {n_cand} {cls} folds"
    plain = random_states(task, OracleSim(n_plain, task_cfg(task), seed=seed), n_plain, seed=seed + 1, standing=True)
    st = np.ascontiguousarray(np.concatenate([plain, cand[:, hot]], axis=1))
    n = n_plain + len(hot)
    a = np.concatenate([rng.normal(size=(n_plain, 6)).astype(np.float32), ca[hot]])
    sg, outs, moved = moved_by_bug(st, a)
    assert not moved[:n_plain].any() and moved[n_plain:].all(), np.nonzero(moved)[0]
    stats = {}
    with pytest.raises(AssertionError, match="oracle is stable") as ei:
        T._check(task, f"planted rare-branch bug {kind}", n, seed, st, [a], outs[-1], sg, None, stats=stats)
    listed = {int(v) for v in re.findall(r"\d+", str(ei.value).split(": [")[-1])}
    print(f"  planted bug {kind} ({cls}): hot envs {list(range(n_plain, n))}, unexplained {sorted(listed)}")
    assert listed and listed <= set(range(n_plain, n)), listed
    # (a face sample 1 mm off is a small push: in some folds its effect stays inside what the unplanted
    # oracle reaches under rounding-scale perturbation there -- 2 of 4 caught for v2 and stand-up;
    # the flipped rim-end normal and the missing separating axis are caught in every fold)
    if kind != 5:
        assert listed == set(range(n_plain, n)), listed
    assert stats["deep_draw"] >= len(listed), stats


@pytest.mark.parametrize("task", TASKS + ("v2:step0",))
def test_product_cfg_pins_the_env_defaults(task):
    """tests/fullstate.product_cfg is the TaskCfg of the task's registered env, and the values it
    carries today: TGS (solver_mode 1) everywhere, self_manifold 3 for walking v2 and stand-up and 2
    for v4 and the manager, the reference's 4 position iterations (zbot_cfg.py:637); it differs from
    the PGS configuration the other parity tests build in exactly those fields; product() routes
    task_cfg() to it and back."""
    import dataclasses
    from fullstate import base_task, product, product_cfg
    p, t = product_cfg(task), task_cfg(task)
    four = base_task(task) in ("v2", "standup")
    assert (p.solver_mode, p.self_manifold) == ((1, 3) if four else (1, 2))
    assert p.solver_iterations == 4
    dp, dt = dataclasses.asdict(p), dataclasses.asdict(t)
    assert dp.keys() == dt.keys()
    diff = {k for k in dp if dp[k] != dt[k]}
    assert diff == ({"solver_mode", "self_manifold"} if four else {"solver_mode"}), diff
    with product():
        assert dataclasses.asdict(task_cfg(task)) == dp
    assert dataclasses.asdict(task_cfg(task)) == dt
