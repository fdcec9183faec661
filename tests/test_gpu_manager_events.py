"""Manager task: the interval push event and the yaw / heading commands (include/zbot_manager_events.h)
through the C ABI, product solver cfg (solver_mode 1, manifold 2), both occupancy variants where a test
is parametrised over them. N = 130 (a partial wave and a partial workgroup) unless stated.

The push is checked by composition: a handle without events and one with the push on start from one
state; after one step with the same actions the envs whose timer did not run out are bit-equal, and the
others differ in the root velocity rows only, by one rigid velocity field whose six components
(recovered in float64 from the two states and the model) lie in the configured ranges. step_dt here is
the kernel's own fp32 product sim_dt * decimation.

Tolerance of the recovered components: the kernel adds fl(dv - dw x r) to the root's linear velocity in
fp32, r = c_base - root_pos (|r| about 0.3 m) from fp32 forward kinematics through up to three joints
(|error| <= 8 eps32 |r|), so |recovered - drawn| <= 4 eps32 (|lv_a| + |lv_b|) + |dw| 16 eps32 0.3: TOL
below with |lv| <= 2, |dw| <= 1.
"""
from __future__ import annotations

import math
import os

import numpy as np
import pytest

from zbot_lab_amd import model as zm

pytestmark = pytest.mark.gpu
M, S, ME = zm.M, zm.S, zm.ME
EPS32 = float(np.finfo(np.float32).eps)
TOL = 4 * EPS32 * 4.0 + 16 * EPS32 * 0.3
N = 130
PUSH_LIN = dict(x=(-0.5, 0.5), y=(-0.5, 0.5))
PUSH_ALL = dict(x=(-0.5, 0.5), y=(-0.5, 0.5), z=(-0.1, 0.3), roll=(-0.2, 0.2), pitch=(-0.3, 0.1), yaw=(-0.5, 0.5))


def _events(push=None, interval=(10.0, 15.0), ang=(0.0, 0.0), heading=None, rel=1.0, k=1.0):
    return zm.ManagerEvents(
        push_enabled=push is not None, push_interval_s=interval if push is not None else (0.0, 0.0),
        push_velocity_range=tuple(tuple((push or {}).get(a, (0.0, 0.0))) for a in zm.PUSH_AXES), cmd_ang_vel_z=ang,
        heading_command=heading is not None, cmd_heading=heading or (0.0, 0.0), cmd_rel_heading=rel, heading_stiffness=k)


def _sim(n=N, seed=0, events=None, occ=None, cfg=None, **kw):
    """A manager handle (product solver cfg; feet_close 0.10 m as in tests/test_gpu_manager.py: the
    default sits 1.7e-5 m below the stance). occ: force the one / two waves per SIMD kernels."""
    from zbot_lab_amd.sim import ZbotSim
    old = os.environ.get("ZB_OCC1")
    if occ is not None:
        os.environ["ZB_OCC1"] = "1" if occ == 1 else "0"
    try:
        sim = ZbotSim(n, cfg or zm.TaskCfg.manager_flat(**{**dict(solver_mode=1, self_manifold=2, feet_close_min=0.10), **kw}),
                      device="cuda:0", seed=seed)
    finally:
        if occ is not None:
            os.environ.pop("ZB_OCC1") if old is None else os.environ.__setitem__("ZB_OCC1", old)
    if occ is not None:
        assert sim.kernel_variant() == (1, occ, 0, 0)
    if events is not None:
        sim.set_manager_events(events)
    return sim


def _np(t):
    return t.detach().cpu().numpy()


def _step(sim, a):
    import torch
    obs, rew, te, tr = sim.step(torch.from_numpy(a).cuda())
    return _np(obs).copy(), _np(rew).copy(), _np(te).copy(), _np(tr).copy()


def _step_dt(sim):
    return float(np.float32(sim._c.sim_dt) * np.float32(sim._c.decimation))


# ------------------------------------------------------------------ float64 restatement from state + model
def _qmul(a, b):
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def _qmat(q):
    w, x, y, z = (q[..., k] for k in range(4))
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def _mv(R, v):
    return (R * v[..., None, :]).sum(-1)


def base_kinematics(st, m):
    """float64, per env: r = (COM of the Isaac Lab root link = base link) - root_pos in the world, the
    base link's world quaternion, and its body's world angular velocity (root twist + the joint rates
    before it): the chain's forward kinematics as tests/test_gpu_critic_obs.py states it."""
    arr = lambda a: np.ctypeslib.as_array(a).astype(np.float64)
    st = st.astype(np.float64)
    quat = st[S["ROOT_QUAT"]:S["ROOT_QUAT"] + 4].T
    av = st[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3].T
    jq, jqd = st[S["JOINT_POS"]:S["JOINT_POS"] + 6].T, st[S["JOINT_VEL"]:S["JOINT_VEL"] + 6].T
    jpr, jpp, jcp, jcr = arr(m.joint_parent_rot), arr(m.joint_parent_pos), arr(m.joint_child_pos), arr(m.joint_child_rot)
    q = quat / np.sqrt((quat * quat).sum(-1, keepdims=True))
    R = _qmat(q)
    p = np.zeros((st.shape[1], 3))
    w = av
    l = int(m.api_root_link)
    for j in range((l + 1) // 2):
        qj = _qmul(q, jpr[j])
        org = p + _mv(R, jpp[j])
        ax = _qmat(qj)[..., :, 2]
        half = 0.5 * jq[:, j]
        qz = np.stack([np.cos(half), np.zeros_like(half), np.zeros_like(half), np.sin(half)], -1)
        qa = _qmul(qj, qz)
        p = org + _mv(_qmat(qa), jcp[j])
        q = _qmul(qa, jcr[j])
        q = q / np.sqrt((q * q).sum(-1, keepdims=True))
        R = _qmat(q)
        w = w + ax * jqd[:, j:j + 1]
    r = p + _mv(R, arr(m.link_com)[l])
    return r, _qmul(q, arr(m.link_rot)[l]), w


def recover_push(st_a, st_b, m):
    """(dv, dw) [N, 3] each: the velocity increment of the base link's COM and the angular increment."""
    r, _, _ = base_kinematics(st_b, m)
    a, b = st_a.astype(np.float64), st_b.astype(np.float64)
    dw = (b[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3] - a[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3]).T
    dlv = (b[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3] - a[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3]).T
    return dlv + np.cross(dw, r), dw


def _standing_pair(n, seed, events, occ=None, steps=4):
    """Handles A (events off) and B (events) at one state after a reset and a few standing steps."""
    a, b = _sim(n, seed, occ=occ), _sim(n, seed, events=events, occ=occ)
    assert not a.events_active and b.events_active
    a.reset(None)
    b.reset(None)
    z = np.zeros((n, 6), np.float32)
    for _ in range(steps):
        _step(a, z)
        _step(b, z)
    st, wc = a.get_state(), a.get_contact_cache()
    for s in (a, b):
        s.set_state(st)
        s.set_contact_cache(wc)
    return a, b


# ------------------------------------------------------------------ 1. off is off
@pytest.mark.parametrize("occ", [1, 2])
def test_off_is_off(gpu, occ):
    import torch
    a, b = _sim(seed=11, occ=occ), _sim(seed=11, events=_events(), occ=occ)
    assert not a.events_active and not b.events_active and not a.events_configured
    assert a.lib.zb_manager_event_state_dim(a._h) == zm.ME_STATE_DIM
    acc = [torch.zeros(zm.LOG_LEN + zm.LOG_COUNTS, device="cuda") for _ in range(2)]
    for s, c in zip((a, b), acc):
        s.set_log_accumulator(c)
        s.reset(None)
    rng = np.random.default_rng(3)
    for _ in range(8):
        act = rng.normal(size=(N, 6)).astype(np.float32)
        ra, rb = _step(a, act), _step(b, act)
        for x, y in zip(ra, rb):
            np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(_np(a.get_state()), _np(b.get_state()))
    np.testing.assert_array_equal(_np(a.get_contact_cache()), _np(b.get_contact_cache()))
    np.testing.assert_array_equal(_np(acc[0]), _np(acc[1]))


# ------------------------------------------------------------------ 2. push by composition
@pytest.mark.parametrize("occ", [1, 2])
@pytest.mark.parametrize("ranges", [PUSH_LIN, PUSH_ALL], ids=["linear", "six"])
def test_push_by_composition(gpu, occ, ranges):
    import torch
    interval = (10.0, 15.0)
    a, b = _standing_pair(N, 5, _events(push=ranges, interval=interval), occ=occ)
    dt = _step_dt(b)
    t_in = np.full(N, 1.0, np.float32)
    g_half, g_dt, g_late = np.arange(0, 43), np.arange(43, 53), np.arange(53, 63)
    t_in[g_half], t_in[g_dt], t_in[g_late] = np.float32(0.5 * dt), np.float32(dt), np.float32(dt) + np.float32(1e-4)
    ev = _np(b.get_event_state()).copy()
    ev[ME["PUSH_TIME_LEFT"]] = t_in
    b.set_event_state(torch.from_numpy(ev).cuda())
    st0 = _np(a.get_state()).copy()
    act = (0.3 * np.random.default_rng(9).normal(size=(N, 6))).astype(np.float32)
    ra, rb = _step(a, act), _step(b, act)
    sa, sb, evb = _np(a.get_state()), _np(b.get_state()), _np(b.get_event_state())
    for x, y in zip(ra, rb):   # obs, reward, flags: the push is in none of them
        np.testing.assert_array_equal(x, y)
    reset = ra[2] | ra[3]
    print(f"\n[push {occ}] envs reset in the step: {int(reset.sum())} of {N}")
    assert reset.mean() < 0.10
    due = np.zeros(N, bool)
    due[g_half] = due[g_dt] = True
    fire, quiet = due & ~reset, ~due & ~reset
    vel = np.zeros(sa.shape[0], bool)
    vel[S["ROOT_LINVEL"]:S["ROOT_ANGVEL"] + 3] = True
    np.testing.assert_array_equal(sa[:, quiet], sb[:, quiet])
    np.testing.assert_array_equal(evb[0, quiet], t_in[quiet] - np.float32(dt))
    np.testing.assert_array_equal(sa[~vel][:, fire], sb[~vel][:, fire])
    assert (evb[0, fire] >= interval[0]).all() and (evb[0, fire] <= interval[1]).all()
    # envs reset in the step: a fresh timer, already advanced by this step's interval pass; no push
    np.testing.assert_array_equal(sa[:, reset], sb[:, reset])
    assert (evb[0, reset] >= np.float32(interval[0]) - np.float32(dt)).all()
    assert (evb[0, reset] <= np.float32(interval[1]) - np.float32(dt)).all()
    dv, dw = recover_push(sa, sb, b._m)
    rng6 = [ranges.get(k, (0.0, 0.0)) for k in zm.PUSH_AXES]
    comp = np.concatenate([dv, dw], 1)[fire]
    for k, (lo, hi) in enumerate(rng6):
        assert comp[:, k].min() >= lo - TOL and comp[:, k].max() <= hi + TOL, (zm.PUSH_AXES[k], comp[:, k].min(), comp[:, k].max())
    assert (np.abs(comp[:, :2]).max(1) > 1e-3).all()  # every due env was pushed
    if ranges is PUSH_LIN:  # no angular part: the angular rows are untouched, the root gains the same vector
        av = slice(S["ROOT_ANGVEL"], S["ROOT_ANGVEL"] + 3)
        np.testing.assert_array_equal(sa[av][:, fire], sb[av][:, fire])
        np.testing.assert_array_equal(sa[S["ROOT_LINVEL"] + 2, fire], sb[S["ROOT_LINVEL"] + 2, fire])
    else:  # the lever arm shows: the root's own increment differs from the COM's by dw x (root - c_base)
        r, _, _ = base_kinematics(sb, b._m)
        lever = np.cross(dw, -r)[fire]
        dlv = (sb.astype(np.float64) - sa)[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3].T[fire]
        assert np.abs(lever).max() > 1e-2
        assert np.abs(dlv - (dv[fire] + lever)).max() <= TOL
    # A pushed state is an ordinary state: the unchanged oracle steps it as the device does, held to the project's
    # full-state rule (tests/test_gpu_fullstate._check: every env within tolerance or explained by the
    # perturbed-oracle envelope, the contact-active aggregate within the f64 baseline; at most 2 % of the envs
    # outside tolerance), on the registered env's own task cfg, with the events kernel and timers far from firing.
    import fullstate
    import test_gpu_fullstate as F
    with fullstate.product():
        c = _sim(N, 5, events=_events(push=ranges, interval=interval), occ=occ, cfg=fullstate.product_cfg("manager"))
        assert c.events_active
        c.set_state(torch.from_numpy(sb).cuda())
        g_out = _step(c, act)
        nbad = F._check("manager", f"one step from the pushed state ({occ} wave(s) per SIMD)", N, 5, sb, [act], g_out,
                        _np(c.get_state()), torch)
    assert (_np(c.get_event_state())[0] > 9.0).all()
    assert nbad <= 0.02 * N


# ------------------------------------------------------------------ 3. laws
def obs_noise(obs, st, m):
    """The 16 additive noise values of each env's observation row (draws 16..31: quaternion 4, joint positions 6,
    joint velocities 6, Isaac Lab joint order): the row minus its float64 restatement from the state it shows."""
    _, bq, _ = base_kinematics(st, m)
    s64 = st.astype(np.float64)
    ai = np.ctypeslib.as_array(m.api_joint_index)
    sg = np.ctypeslib.as_array(m.api_joint_sign).astype(np.float64)
    q0 = np.ctypeslib.as_array(m.default_joint_pos).astype(np.float64)
    out = {f"noise quat {k}": obs[:, k] - bq[:, k] for k in range(4)}
    for j in range(6):
        out[f"noise jpos {ai[j]}"] = obs[:, 7 + ai[j]] - sg[j] * (s64[S["JOINT_POS"] + j] - q0[j])
        out[f"noise jvel {ai[j]}"] = obs[:, 13 + ai[j]] - sg[j] * s64[S["JOINT_VEL"] + j]
    return out


LAW_INTERVAL, LAW_ANG, LAW_HEAD = (10.0, 15.0), (-1.0, 0.5), (-math.pi, math.pi)


def _law_scenario(n, seed):
    """One seed's recovered draws: construction, two full resets (call ctr, ctr + 1), then two steps (ctr, ctr + 1)
    in each of which every push timer and every command timer is forced to run out, against an events-off twin
    from the same state. Columns by name; 'live*': the envs that did not reset in that step."""
    import torch
    evc = _events(push=PUSH_ALL, interval=LAW_INTERVAL, ang=LAW_ANG, heading=LAW_HEAD, rel=0.5)
    a, b = _sim(n, seed, obs_corruption=True), _sim(n, seed, events=evc, obs_corruption=True)
    out = {"timer con": _np(b.get_event_state())[0].copy()}
    for k in (1, 2):
        a.reset(None)
        b.reset(None)
        st, ev = _np(b.get_state()).copy(), _np(b.get_event_state()).copy()
        out.update({f"timer reset{k}": ev[0], f"ang z reset{k}": st[M["COMMANDS"] + 2], f"heading reset{k}": ev[1],
                    f"is-heading reset{k}": ev[2]})
    out.update({"lin x reset": st[M["COMMANDS"]], "standing reset": st[M["CMD_STANDING"]], "pos x reset": st[S["ROOT_POS"]],
                "pos y reset": st[S["ROOT_POS"] + 1], "quat w reset": st[S["ROOT_QUAT"]]})
    half = np.float32(0.5 * _step_dt(b))
    act = np.zeros((n, 6), np.float32)
    for k in (1, 2):
        st = _np(b.get_state()).copy()
        st[M["CMD_TIME_LEFT"]] = half
        for s in (a, b):
            s.set_state(torch.from_numpy(st).cuda())
        ev = _np(b.get_event_state()).copy()
        ev[0] = half
        b.set_event_state(torch.from_numpy(ev).cuda())
        _step(a, act)
        rb = _step(b, act)
        sa, sb, ev = _np(a.get_state()).copy(), _np(b.get_state()).copy(), _np(b.get_event_state()).copy()
        dv, dw = recover_push(sa, sb, b._m)
        out.update({f"push {ax} step{k}": c for ax, c in zip(zm.PUSH_AXES, np.concatenate([dv, dw], 1).T)})
        out.update({f"timer step{k}": ev[0], f"heading step{k}": ev[1], f"is-heading step{k}": ev[2],
                    f"ang z step{k}": sb[M["COMMANDS"] + 2], f"lin x step{k}": sb[M["COMMANDS"]],
                    f"live{k}": ~(rb[2] | rb[3]),
                    f"free{k}": ~(rb[2] | rb[3]) & (ev[2] < 0.5) & (sb[M["CMD_STANDING"]] < 0.5)})
        if k == 1:
            out.update(obs_noise(rb[0], sb, b._m))
    a.close()
    b.close()
    return out


def test_laws(gpu):
    """Marginals, pairwise correlation among the new draws and against the env's existing ones (pose, command,
    the 16 noise columns of the same call), call ctr against ctr + 1 and seed against seed + 1 for every new draw."""
    from random_laws import Laws
    n = 16384
    c, d = _law_scenario(n, 7), _law_scenario(n, 8)
    L = Laws()
    live, free = c["live1"], c["free1"]
    assert live.mean() > 0.9 and c["live2"].mean() > 0.9
    L.uniform("timer at construction", c["timer con"], *LAW_INTERVAL)
    L.uniform("timer after reset", c["timer reset2"], *LAW_INTERVAL)
    L.uniform("ang z at reset", c["ang z reset2"], *LAW_ANG)
    L.uniform("heading target at reset", c["heading reset2"], *LAW_HEAD, grain=2.0 ** -22)
    L.bernoulli("is-heading at reset", c["is-heading reset2"], 0.5)
    for ax, (lo, hi) in PUSH_ALL.items():   # recovered through fp32 sums: granularity TOL of a range >= 0.4
        L.uniform(f"push {ax}", c[f"push {ax} step1"][live], lo, hi, grain=TOL / (hi - lo), slack=TOL)
    L.uniform("timer after fire", c["timer step1"][live], *LAW_INTERVAL)
    L.uniform("ang z at resample", c["ang z step1"][free], *LAW_ANG)   # as drawn: not heading-controlled, not standing
    L.uniform("heading target at resample", c["heading step1"][live], *LAW_HEAD, grain=2.0 ** -22)
    L.bernoulli("is-heading at resample", c["is-heading step1"][live], 0.5)
    # independence
    new_reset = {k: c[k + " reset2"] for k in ("timer", "ang z", "heading", "is-heading")}
    old_reset = {k: c[k + " reset"] for k in ("lin x", "standing", "pos x", "pos y", "quat w")}
    new_step = {k: c[k + " step1"][live] for k in ["timer", "heading", "is-heading"] + [f"push {ax}" for ax in zm.PUSH_AXES]}
    noise = {k: v[live] for k, v in c.items() if k.startswith("noise ")}
    assert len(noise) == 16
    L.uncorrelated("new reset draws", new_reset)
    L.cross("new reset draws x existing", new_reset, old_reset)
    L.uncorrelated("new step draws", new_step)
    L.cross("new step draws x reset draws", new_step, {k: v[live] for k, v in {**new_reset, **old_reset}.items()})
    L.cross("new step draws x resampled command", new_step, {"lin x": c["lin x step1"][live]})  # (lin y: U(0, 0), a constant)
    L.cross("new step draws x noise", new_step, noise)
    L.cross("ang z at resample x noise, step draws", {"ang z": c["ang z step1"][free]},
            {k: c[k][free] for k in list(c) if k.startswith("noise ") or k.startswith("push ") and k.endswith("step1")})
    # call ctr against ctr + 1 (one handle), seed against seed + 1 (two handles): every new draw
    def both(x, y, mask):
        return x[mask], y[mask]
    pairs = [("timer at construction seed", c["timer con"], d["timer con"], None)]
    for k in ("timer", "ang z", "heading", "is-heading"):
        pairs.append((f"{k} at reset ctr", c[k + " reset1"], c[k + " reset2"], None))
        pairs.append((f"{k} at reset seed", c[k + " reset2"], d[k + " reset2"], None))
    step_cols = ["timer", "heading", "is-heading"] + [f"push {ax}" for ax in zm.PUSH_AXES]
    for k in step_cols:
        pairs.append((f"{k} at step ctr", c[k + " step1"], c[k + " step2"], c["live1"] & c["live2"]))
        pairs.append((f"{k} at step seed", c[k + " step1"], d[k + " step1"], c["live1"] & d["live1"]))
    pairs.append(("ang z at resample ctr", c["ang z step1"], c["ang z step2"], c["free1"] & c["free2"]))
    pairs.append(("ang z at resample seed", c["ang z step1"], d["ang z step1"], c["free1"] & d["free1"]))
    for name, x, y, mask in pairs:
        if mask is not None:
            x, y = both(x, y, mask)
        L.fresh(name, x, y, p_equal=0.5 if name.startswith("is-heading") else None)
    L.check("manager events")


# ------------------------------------------------------------------ 4. yaw and heading commands
def test_yaw_command(gpu):
    ang = (-1.0, 0.5)
    s = _sim(seed=2, events=_events(ang=ang), obs_corruption=False, cmd_rel_standing=0.3)
    s.reset(None)
    st0 = _np(s.get_state()).copy()
    z = np.zeros((N, 6), np.float32)
    obs1, _, te1, tr1 = _step(s, z)
    st1 = _np(s.get_state()).copy()
    obs3 = obs1
    for _ in range(2):
        obs3, _, te, tr = _step(s, z)
        te1, tr1 = te1 | te, tr1 | tr
    st3 = _np(s.get_state())
    standing = st1[M["CMD_STANDING"]] > 0.5
    assert 0 < standing.sum() < N
    np.testing.assert_array_equal(obs1[:, 6], st1[M["COMMANDS"] + 2])
    np.testing.assert_array_equal(obs3[:, 6], st3[M["COMMANDS"] + 2])
    assert (obs1[:, 6] >= ang[0]).all() and (obs1[:, 6] <= ang[1]).all()
    assert (obs1[standing, 6] == 0).all() and (obs1[~standing, 6] != 0).all()
    keep = ~(te1 | tr1)
    np.testing.assert_array_equal(obs1[keep & ~standing, 6], st0[M["COMMANDS"] + 2][keep & ~standing])  # as drawn at the reset
    np.testing.assert_array_equal(obs3[keep, 6], obs1[keep, 6])   # unchanged between resamples


def _heading_expected(obs, target, k, ang):
    w, x, y, zq = (obs[:, i].astype(np.float64) for i in range(4))
    hw = np.arctan2(2 * (w * zq + x * y), 1 - 2 * (y * y + zq * zq))
    d = target.astype(np.float64) - hw
    wr = (d + math.pi) % (2 * math.pi)
    wr = np.where((wr == 0) & (d > 0), math.pi, wr - math.pi)
    return np.clip(k * wr, *ang)


def test_heading_command_and_reward(gpu):
    import torch
    ang, k = (-0.4, 0.4), 0.5
    s = _sim(seed=4, events=_events(ang=ang, heading=(-math.pi, math.pi), rel=0.5, k=k), obs_corruption=False)
    s.reset(None)
    st = _np(s.get_state()).copy()
    st[M["EP_LEN"], ::7] = s._c.max_episode_length - 1   # these time out and reset inside the step
    s.set_state(torch.from_numpy(st).cuda())
    obs, _, te, tr = _step(s, np.zeros((N, 6), np.float32))
    assert tr[::7].all()
    st1, ev1 = _np(s.get_state()), _np(s.get_event_state())
    ish, standing = ev1[ME["IS_HEADING"]] > 0.5, st1[M["CMD_STANDING"]] > 0.5
    assert 0.3 < ish.mean() < 0.7
    exp = _heading_expected(obs, ev1[ME["HEADING_TARGET"]], k, ang)   # post-reset quaternion, fresh target for reset envs
    sel = ish & ~standing
    err = np.abs(obs[sel, 6] - exp[sel])
    print(f"\n[heading] max |obs[6] - fp64| {err.max():.3g} over {int(sel.sum())} heading envs "
          f"({int((sel & tr).sum())} reset in the step), clipped {int((np.abs(exp[sel]) == 0.4).sum())}")
    assert err.max() <= 1e-5
    assert (sel & tr).any() and (np.abs(exp[sel]) == 0.4).any() and (np.abs(exp[sel]) < 0.4).any()
    free = ~ish & ~standing & ~(te | tr)
    np.testing.assert_array_equal(obs[free, 6], st[M["COMMANDS"] + 2][free])   # the drawn value stays
    assert (obs[standing, 6] == 0).all()
    np.testing.assert_array_equal(obs[:, 6], st1[M["COMMANDS"] + 2])
    # track_ang_vel_z_exp's share of the reward moves with the command: the next step's episode-sum increment is
    # weight step_dt exp(-(command - w_z)^2 / 0.25) with the command this step left and the base's post-step w_z
    # (__expf: 2 ulp + 2 |e| / 0.25 x the fp32 error of w_z, about 1e-6: 1e-4 relative covers both)
    live = ~(te | tr)
    sums0 = st1[M["EP_SUMS"] + 1].copy()
    _, _, te2, tr2 = _step(s, np.zeros((N, 6), np.float32))
    st2 = _np(s.get_state())
    live &= ~(te2 | tr2)
    # w_z of the post-step pose is not in the state after the step's own push-free update: restate from st2
    _, _, w = base_kinematics(st2, s._m)
    e = st1[M["COMMANDS"] + 2].astype(np.float64) - w[:, 2]
    want = 0.5 * _step_dt(s) * np.exp(-e * e / 0.25)
    got = (st2[M["EP_SUMS"] + 1] - sums0).astype(np.float64)
    rel = np.abs(got[live] - want[live]) / want[live]
    print(f"[heading] track_ang_vel_z_exp increment: max relative error {rel.max():.3g}, "
          f"terms from {want[live].min():.3g} to {want[live].max():.3g}")
    assert rel.max() <= 1e-4 + 2 * EPS32 * np.abs(sums0).max() / want[live].min()
    assert want[live].max() / want[live].min() > 1.05   # the command does move the term


# ------------------------------------------------------------------ 5. determinism, graph, wrong task
def _events_all():
    return _events(push=PUSH_ALL, interval=(0.05, 0.2), ang=(-1.0, 0.5), heading=(-math.pi, math.pi), rel=0.5)


def test_deterministic_and_graph(gpu):
    import torch
    acts = torch.from_numpy(np.random.default_rng(1).normal(size=(8, N, 6)).astype(np.float32)).cuda()

    def run(graph):
        s = _sim(seed=6, events=_events_all())
        s.reset(None)
        obs, rew = torch.empty(N, zm.M_OBS_DIM, device="cuda"), torch.empty(N, device="cuda")
        for k in range(4):
            s.step_into(acts[k], obs, rew)
        if graph:
            a = torch.empty(N, 6, device="cuda")
            outs = [torch.empty(N, zm.M_OBS_DIM, device="cuda") for _ in range(4)]
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            snap = s.get_state(), s.get_contact_cache(), s.get_event_state()
            with torch.cuda.graph(g):
                for k in range(4):
                    s.step_into(acts[4 + k], outs[k], rew)
            # (capture runs nothing: the state is still the snapshot's; the call counter is on the device)
            g.replay()
            obs = outs[3]
        else:
            for k in range(4):
                s.step_into(acts[4 + k], obs, rew)
        torch.cuda.synchronize()
        return _np(s.get_state()), _np(s.get_event_state()), _np(obs), _np(rew)

    e1, e2, gr = run(False), run(False), run(True)
    assert (e1[1][0] != _np(torch.zeros(1))).any()
    for x, y, z in zip(e1, e2, gr):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, z)


def test_other_task_is_refused(gpu):
    import ctypes as C
    from zbot_lab_amd.sim import ZbotSim
    from zbot_lab_amd import _native
    s = ZbotSim(8, zm.TaskCfg(solver_mode=1), device="cuda:0")
    ev = _events_all().pack()
    rc = s.lib.zb_set_manager_events(s._h, C.byref(ev), None)
    assert rc == -1 and b"manager-task" in s.lib.zb_last_error()
    assert s.lib.zb_manager_event_state_dim(s._h) == -1 and not s.events_active
    with pytest.raises(_native.ZbotError):
        s.get_event_state()
    bad = _events(push=PUSH_LIN, interval=(0.0, 1.0)).pack()
    m = _sim(8)
    assert m.lib.zb_set_manager_events(m._h, C.byref(bad), None) == -1 and b"push_interval_s" in m.lib.zb_last_error()
    bad = _events(ang=(0.5, -0.5)).pack()
    assert m.lib.zb_set_manager_events(m._h, C.byref(bad), None) == -1 and not m.events_active


# ------------------------------------------------------------------ 6. env level
def test_env_level(gpu):
    import torch
    import zbot_lab_amd
    from zbot_lab_amd.envs.manager_flat import EventTerm
    from zbot_lab_amd.rl import RslRlVecEnvWrapper
    cfg = zbot_lab_amd.tasks.load_cfg("zbot-6b-walking-m-v0")
    cfg.scene.num_envs = 64
    cfg.terminations.feet_close.params["minimum_distance"] = 0.10   # (as _sim: the default stance sits at the threshold)
    cfg.events.push_robot = EventTerm("push_by_setting_velocity", "interval",
                                      {"velocity_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5)}}, interval_range_s=(0.1, 0.2))
    cmd = cfg.commands.base_velocity
    cmd.ranges.ang_vel_z = cmd.limit_ranges.ang_vel_z = (-1.0, 1.0)
    cmd.heading_command, cmd.ranges.heading, cmd.rel_heading_envs = True, (-math.pi, math.pi), 0.5
    env = zbot_lab_amd.make("zbot-6b-walking-m-v0", cfg=cfg)
    assert env.unwrapped.sim.events_active
    w = RslRlVecEnvWrapper(env)
    w.get_observations()
    sim = env.unwrapped.sim
    t_min, fires, v_fire = np.inf, 0, 0.0
    t_prev = sim.get_event_state()[ME["PUSH_TIME_LEFT"]]
    for _ in range(20):
        obs, rew, dones, extras = w.step(torch.zeros(64, 6, device="cuda"))
        t_now = sim.get_event_state()[ME["PUSH_TIME_LEFT"]]
        fired = (t_now > t_prev) & (dones == 0)   # the timer went up without a reset: a push this step
        if fired.any():
            v = sim.get_state()[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 2][:, fired]
            fires, v_fire = fires + int(fired.sum()), max(v_fire, float(v.abs().max()))
        t_min, t_prev = min(t_min, float(t_now.min())), t_now
    assert torch.isfinite(rew).all()
    term = env.unwrapped.command_manager.get_term("base_velocity")
    ev = env.unwrapped.sim.get_event_state()
    torch.testing.assert_close(term.heading_target, ev[ME["HEADING_TARGET"]], rtol=0, atol=0)
    assert (term.is_heading_env == (ev[ME["IS_HEADING"]] > 0.5)).all() and 0 < int(term.is_heading_env.sum()) < 64
    assert term.limit_ranges.ang_vel_z == (-1.0, 1.0) and term.command.shape == (64, 3)
    torch.testing.assert_close(term.command, env.unwrapped.command_manager.get_command("base_velocity"), rtol=0, atol=0)
    t = _np(ev[ME["PUSH_TIME_LEFT"]])
    assert t_min < 0.1 and (t <= 0.2).all() and (t > -0.02).all()   # timers ran down and were redrawn
    assert fires >= 64 and v_fire > 0.25   # 0.4 s at a 0.1-0.2 s interval: every env was pushed, some of them hard


# ------------------------------------------------------------------ 7. curriculum fix-up keeps the yaw command
def test_curriculum_fixup_keeps_yaw(gpu):
    """lin_vel_cmd_levels every 5 steps with a zero threshold and every env terminating in every step (the set-up
    of tests/test_gpu_manager.py::test_curriculum_fixup_parity): on the steps in which the ranges widen, the
    finalize launch redraws lin x of the reset envs and must leave their ang z command, its observation entry
    and the yaw metric (|drawn ang z| / (resample time / step_dt), written by the step kernel) as they were."""
    ang = (-1.0, 0.5)
    n = 256
    s = _sim(n, 2, events=_events(ang=ang), obs_corruption=False, range_period_steps=5, range_threshold=-1e9,
             feet_close_min=0.125)
    z = np.zeros((n, 6), np.float32)
    widened = 0
    lim = np.float32(0.1)
    for k in range(12):
        obs, _, te, tr = _step(s, z)
        assert te.all()
        st = _np(s.get_state())
        cmd, standing = st[M["COMMANDS"]:M["COMMANDS"] + 3], st[M["CMD_STANDING"]] > 0.5
        np.testing.assert_array_equal(obs[:, 4:7], cmd.T)
        assert (cmd[2] >= ang[0]).all() and (cmd[2] <= ang[1]).all()
        assert (cmd[2][~standing] != 0).all() and (cmd[:, standing] == 0).all()
        max_steps = np.float32(s._c.cmd_resample_s) / np.float32(_step_dt(s))
        want = np.abs(cmd[2][~standing]) / max_steps
        np.testing.assert_allclose(st[M["METRICS"] + 1][~standing], want, rtol=4 * EPS32, atol=0)
        new_lim = np.float32(_np(s.log_buffer)[16])
        if new_lim > lim:   # the ranges widened in this step: the fix-up ran, lin x comes from the new range
            widened += 1
            assert np.abs(cmd[0]).max() > lim and np.abs(cmd[0]).max() <= new_lim
            lim = new_lim
    assert widened >= 2 and lim == np.float32(0.3)
