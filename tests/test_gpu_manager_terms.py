"""Manager task: the five restored reward terms (include/zbot_manager_terms.h) through the C ABI and the
env, on the build zb_m_terms_step_kernel (asserted by name). 130 envs (a ragged last wave of the 4 envs per
wave) and 64, one and two waves per SIMD, TGS and PGS.

Parity is held on the device's own state: after every step the float64 statement of the terms
(tests/manager_terms_reference.py, pinned to the reference's code by tests/test_manager_terms_reference.py)
is evaluated on the post-step fp32 state, the term state and the terms' kinematic inputs as the getter
reports them, and the per-step increment of each of the five episode sums is compared. An env that resets
in a step is left out of that step: its rewards were computed on the pre-reset state, which no accessor
shows, and its sums are zeroed.

Tolerance (per term): the same statement in numpy float32 on the same inputs, its largest error against
float64 over the run, times 4 (the factor covers __expf / tanh_r, v_rcp and the summation order). The
increment is sum_after - sum_before with sum_after = fl(sum_before + term * weight * step_dt), so the
float32 statement carries the rounding of the accumulation, as the device's sums do. An env-step outside
the tolerance must have a deciding quantity (gait leg phase, |command|, |command xy|) within 1e-6 of its
threshold, and at most 1 % of the env-steps may be such flips. Measured: see DESIGN.md §6.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import manager_terms_reference as ref
from zbot_lab_amd import model as zm

pytestmark = pytest.mark.gpu
M, MT = zm.M, zm.MT
BASE_WEIGHTS = {"gait": 0.5, "feet_clearance": 1.0, "feet_air_time": 2.5, "base_vel_forward": 1.0,
                "feet_force_pattern": 1.0}
W5 = np.array([BASE_WEIGHTS[k] for k in zm.M_EXTRA_REWARD_TERMS])
SIM_DT = 0.005


def _sim(n, seed=0, terms=None, occ=None, tgs=True, events=None, **kw):
    """A manager handle (feet_close 0.10 m as in tests/test_gpu_manager.py; commands wide enough to sit on
    both sides of the 0.05 / 0.1 gates). occ: force the one / two waves per SIMD kernels."""
    from zbot_lab_amd.sim import ZbotSim
    old = os.environ.get("ZB_OCC1")
    if occ is not None:
        os.environ["ZB_OCC1"] = "1" if occ == 1 else "0"
    try:
        cfg = zm.TaskCfg.manager_flat(**{**dict(
            solver_mode=1 if tgs else 0, self_manifold=2, feet_close_min=0.10, cmd_vel_range=(-0.3, 0.3),
            cmd_yaw_range=(-0.15, 0.15), range_limit_vel=(-0.3, 0.3), range_limit_yaw=(-0.15, 0.15)), **kw})
        sim = ZbotSim(n, cfg, device="cuda:0", seed=seed)
    finally:
        if occ is not None:
            os.environ.pop("ZB_OCC1") if old is None else os.environ.__setitem__("ZB_OCC1", old)
    if occ is not None:
        assert sim.kernel_variant() == (1 if tgs else 0, occ, 0, 0)
    if events is not None:
        sim.set_manager_events(events)
    if terms is not None:
        sim.set_manager_terms(terms)
    return sim


def _np(t):
    return t.detach().cpu().numpy().copy()


def _all_terms():
    return zm.ManagerTerms(weights=dict(BASE_WEIGHTS))


def _step_dt(sim):
    return float(np.float32(sim._c.sim_dt) * np.float32(sim._c.decimation))


def _snapshot(sim):
    return _np(sim.get_state()).astype(np.float64), _np(sim.get_terms_state())


def _inputs(st0, st1, ts0, ts1):
    """The reference's arguments for one step: the command as the previous step left it, everything else
    from the post-step state."""
    fz = st1[M["FEET_FZ_HIST"]:M["FEET_FZ_HIST"] + 6].reshape(3, 2, -1).transpose(2, 0, 1)
    return dict(
        ep_len=st1[M["EP_LEN"]], cmd=st0[M["COMMANDS"]:M["COMMANDS"] + 3].T, contact_time=ts1[MT["CONTACT_CUR"]:MT["CONTACT_CUR"] + 2].T,
        air_time=st1[M["FEET_AIR_CUR"]:M["FEET_AIR_CUR"] + 2].T, foot_z=ts1[MT["D_FOOT_Z"]:MT["D_FOOT_Z"] + 2].T,
        foot_vxy=ts1[MT["D_FOOT_VXY"]:MT["D_FOOT_VXY"] + 4].T.reshape(-1, 2, 2), fwd_xy=ts1[MT["D_FWD_XY"]:MT["D_FWD_XY"] + 2].T,
        root_vel=ts1[MT["D_ROOT_VEL"]:MT["D_ROOT_VEL"] + 3].T, fz_hist=fz, force_sum=ts0[MT["FEET_FORCE_SUM"]])


def _timer_candidates(st0, ts0, fn_hist, dec, thr=1.0):
    """The feet's (air, last air, contact) timers after `dec` sensor updates from the pre-step timers: the
    newest min(dec, 3) contact flags come from the post-step |F| history, an older substep's flag is not
    recorded, so both of its values are candidates."""
    a = st0[M["FEET_AIR_CUR"]:M["FEET_AIR_CUR"] + 2].T.astype(np.float32)
    l = st0[M["FEET_AIR_LAST"]:M["FEET_AIR_LAST"] + 2].T.astype(np.float32)
    c = ts0[MT["CONTACT_CUR"]:MT["CONTACT_CUR"] + 2].T.astype(np.float32)
    known = [fn_hist[:, h, :] > np.float32(thr) for h in range(min(dec, 3) - 1, -1, -1)]   # oldest first
    out = []
    for first in ([None] if dec <= 3 else [np.zeros_like(known[0]), np.ones_like(known[0])]):
        x = (a, l, c)
        for flags in ([] if first is None else [first]) + known:
            x = ref.sensor_update(*x, flags, SIM_DT)
        out.append(x)
    return out


# ------------------------------------------------------------------ 1. per-term parity on the device's state
@pytest.mark.parametrize("n, occ, tgs", [(130, 1, True), (130, 2, False), (64, 2, True), (64, 1, False)],
                         ids=["130-occ1-tgs", "130-occ2-pgs", "64-occ2-tgs", "64-occ1-pgs"])
def test_per_term_parity(gpu, n, occ, tgs):
    """The reference's inputs (foot height and velocity, forward vector, root velocity) are read through
    zb_get_manager_terms_state, i.e. from the library's out-of-line kinematics on the post-step state: the
    test holds the step kernel's in-line kinematics and term arithmetic to those. Which point of the foot
    is read is not pinned here; tests/test_manager_terms_cfg.py pins clearance_point to the link's COM,
    and the out-of-line kinematics are pinned by the tests that came before this file."""
    import torch
    sim = _sim(n, seed=3, terms=_all_terms(), occ=occ, tgs=tgs)
    assert sim.kernel_name() == "zb_m_terms_step_kernel" and sim.terms_active
    sim.reset(None)
    dt = _step_dt(sim)
    rng = np.random.default_rng(11)
    inc_dev, inc64, inc32, near, live = [], [], [], [], []
    st0, ts0 = _snapshot(sim)
    assert not ts0[:zm.MT_STATE_DIM].any()
    for k in range(40):
        act = torch.from_numpy(rng.normal(0, 0.6, (n, 6)).astype(np.float32)).cuda()
        _, rew, te, tr = sim.step(act)
        keep = ~(_np(te) | _np(tr))
        st1, ts1 = _snapshot(sim)
        a = _inputs(st0, st1, ts0, ts1)
        s0 = ts0[MT["EP_SUMS"]:MT["EP_SUMS"] + 5].T
        v64, f64 = ref.terms(**a, step_dt=dt)
        v32, f32 = ref.terms(**a, step_dt=dt, dtype=np.float32)
        inc64.append(ref.sum_update(s0, v64, W5, dt) - s0)
        inc32.append((ref.sum_update(s0, v32, W5, dt, np.float32) - s0.astype(np.float32)).astype(np.float64))
        inc_dev.append(ts1[MT["EP_SUMS"]:MT["EP_SUMS"] + 5].T.astype(np.float64) - s0)
        g = ref.gates(a["ep_len"], dt, a["cmd"], a["contact_time"], ref.Params())
        near.append((np.abs(g["phase"].astype(np.float64) - np.float32(0.55)).min(-1) < 1e-6)
                    | (np.abs(g["norm3"].astype(np.float64) - np.float32(0.05)) < 1e-6)
                    | (np.abs(g["norm2"].astype(np.float64) - np.float32(0.1)) < 1e-6))
        live.append(keep)
        # the integrator, and the timers: exact (fp32 sums of sim_dt), one mode at a time
        np.testing.assert_allclose(ts1[MT["FEET_FORCE_SUM"]][keep], f64[keep], rtol=0, atol=4 * max(np.abs(f32 - f64).max(), 1e-12))
        fn = st1[M["FEET_FN_HIST"]:M["FEET_FN_HIST"] + 6].reshape(3, 2, -1).transpose(2, 0, 1).astype(np.float32)
        got = (a["air_time"].astype(np.float32), st1[M["FEET_AIR_LAST"]:M["FEET_AIR_LAST"] + 2].T.astype(np.float32),
               a["contact_time"].astype(np.float32))
        ok = np.zeros((n, 2), bool)   # (per foot: the unrecorded first substep's flag is the foot's own)
        for cand in _timer_candidates(st0, ts0, fn, 4):
            ok |= np.all([x == y for x, y in zip(got, cand)], axis=0)
        assert ok[keep].all()
        assert (((got[0] > 0) ^ (got[2] > 0)))[keep].all()
        # a reset env's rows are zero
        assert not ts1[:zm.MT_STATE_DIM][:, ~keep].any()
        assert torch.isfinite(rew).all()
        st0, ts0 = st1, ts1
    inc_dev, inc64, inc32, near, live = (np.stack(x) for x in (inc_dev, inc64, inc32, near, live))
    assert live.mean() > 0.5
    flips = np.zeros_like(live)
    for t, name in enumerate(zm.M_EXTRA_REWARD_TERMS):
        tol = 4 * np.abs(inc32[..., t] - inc64[..., t])[live].max()
        err = np.abs(inc_dev[..., t] - inc64[..., t])
        bad = (err > tol) & live
        print(f"{name}: tolerance {tol:.3e}, largest error {err[live & ~near].max():.3e}, outside {int(bad.sum())}, "
              f"largest increment {np.abs(inc64[..., t][live]).max():.3e}")
        assert tol > 0 and np.abs(inc64[..., t][live]).max() > 100 * tol, name   # the term moved, the bound bites
        assert not (bad & ~near).any(), (name, float(err[bad & ~near].max()), tol)
        flips |= bad
    print("gate flips", int(flips.sum()), "of", int(live.sum()), "env-steps; near a threshold:", int((near & live).sum()))
    assert flips.sum() <= 0.01 * live.sum()


# ------------------------------------------------------------------ 2. timers and integrator laws
def test_timer_and_integrator_laws(gpu):
    """decimation 3: the 3-slot |F| history then records every substep of a step, so the ContactSensor
    update is replayed exactly from the device's own forces. A 0.3 s episode forces a time-out reset."""
    import torch
    n = 64
    sim = _sim(n, seed=5, terms=_all_terms(), decimation=3, episode_length_s=0.3)
    sim.reset(None)
    rng = np.random.default_rng(2)
    st0, ts0 = _snapshot(sim)
    resets = contact = air = 0
    for k in range(24):
        act = torch.from_numpy(rng.normal(0, 0.6, (n, 6)).astype(np.float32)).cuda()
        _, _, te, tr = sim.step(act)
        done = _np(te) | _np(tr)
        st1, ts1 = _snapshot(sim)
        fn = st1[M["FEET_FN_HIST"]:M["FEET_FN_HIST"] + 6].reshape(3, 2, -1).transpose(2, 0, 1).astype(np.float32)
        (a, l, c), = _timer_candidates(st0, ts0, fn, 3)
        keep = ~done
        for got, want in ((st1[M["FEET_AIR_CUR"]:M["FEET_AIR_CUR"] + 2].T, a), (st1[M["FEET_AIR_LAST"]:M["FEET_AIR_LAST"] + 2].T, l),
                          (ts1[MT["CONTACT_CUR"]:MT["CONTACT_CUR"] + 2].T, c)):
            np.testing.assert_array_equal(got.astype(np.float32)[keep], want[keep])
        contact += int((c[keep] > 0).sum())
        air += int((a[keep] > 0).sum())
        if done.any():   # ContactSensor.reset, reset_my_data, RewardManager.reset
            assert (np.abs(ts0[MT["FEET_FORCE_SUM"]][done]) > 0).any()
            assert not ts1[:zm.MT_STATE_DIM][:, done].any()
            assert not st1[M["FEET_AIR_CUR"]:M["FEET_AIR_CUR"] + 2][:, done].any()
            resets += int(done.sum())
        st0, ts0 = st1, ts1
    assert resets >= n and contact > 0 and air > 0   # every env timed out once; both modes were seen
    # an explicit reset zeroes the rows and logs the sums
    sim.step(torch.zeros(n, 6, device="cuda"))
    before = _np(sim.get_terms_state())
    assert before[MT["EP_SUMS"]:MT["EP_SUMS"] + 5].any()
    ids = torch.arange(0, n, 2, dtype=torch.int32, device="cuda")
    sim.reset(ids)
    after = _np(sim.get_terms_state())
    assert not after[:zm.MT_STATE_DIM][:, ::2].any()
    np.testing.assert_array_equal(after[:zm.MT_STATE_DIM][:, 1::2], before[:zm.MT_STATE_DIM][:, 1::2])
    want = before[MT["EP_SUMS"]:MT["EP_SUMS"] + 5][:, ::2].astype(np.float64).mean(1) / 0.3
    got = _np(sim.log_buffer)[11:16]
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------ 3. subset
def test_subset_reward_is_the_sum_of_the_active_terms(gpu):
    import torch
    import zbot_lab_amd
    from zbot_lab_amd.envs.manager_flat import base_reward_term
    cfg = zbot_lab_amd.tasks.load_cfg("zbot-6b-walking-m-v0")
    cfg.scene.num_envs = 64
    cfg.seed = 4
    cfg.terminations.feet_close.params["minimum_distance"] = 0.10
    cfg.rewards.foot_forward = None
    cfg.rewards.gait = base_reward_term("gait")
    cfg.commands.base_velocity.ranges.lin_vel_x = cfg.commands.base_velocity.limit_ranges.lin_vel_x
    env = zbot_lab_amd.make("zbot-6b-walking-m-v0", cfg=cfg)
    sim = env.unwrapped.sim
    assert sim.kernel_name() == "zb_m_terms_step_kernel"
    active = cfg.reward_terms()
    assert "foot_forward" not in active and active.index("gait") == 8
    env.reset()
    rng = np.random.default_rng(9)
    st0, ts0 = _snapshot(sim)
    gait_seen = 0.0
    for k in range(12):
        out = env.step(torch.from_numpy(rng.normal(0, 0.6, (64, 6)).astype(np.float32)).cuda())
        rew, done = _np(out[1]).astype(np.float64), _np(out[2]) | _np(out[3])
        st1, ts1 = _snapshot(sim)
        s0 = np.concatenate([st0[M["EP_SUMS"]:M["EP_SUMS"] + 11], ts0[MT["EP_SUMS"]:MT["EP_SUMS"] + 5].astype(np.float64)])
        s1 = np.concatenate([st1[M["EP_SUMS"]:M["EP_SUMS"] + 11], ts1[MT["EP_SUMS"]:MT["EP_SUMS"] + 5].astype(np.float64)])
        keep = ~done
        # every increment carries half an ulp of its sum; the reward its own rounding over 16 adds
        eps = float(np.finfo(np.float32).eps)
        tol = (0.5 * eps * np.abs(s1).sum(0) + 16 * eps * np.abs(s1 - s0).sum(0))[keep]
        np.testing.assert_array_less(np.abs((s1 - s0).sum(0) - rew)[keep], tol + 1e-12)
        slots = [zm.m_log_slot(k_) for k_ in active]
        off = [s for s in range(16) if s not in slots]
        assert not s1[off].any()           # foot_forward (weight 0) and the four absent terms add nothing
        gait_seen = max(gait_seen, float(np.abs(s1[11]).max()))
        st0, ts0 = st1, ts1
    assert gait_seen > 0
    log = out[4]["log"]
    assert [k_ for k_ in log if k_.startswith("Episode_Reward/")] == [f"Episode_Reward/{k_}" for k_ in active]
    assert env.unwrapped.reward_scales == cfg.reward_cfg["reward_scales"] and list(env.unwrapped.reward_scales) == active


# ------------------------------------------------------------------ 4. feature off
def test_feature_off_launches_what_it_launched(gpu):
    import torch
    import zbot_lab_amd
    from zbot_lab_amd.sim import ZbotSim
    plain = _sim(16)
    assert plain.kernel_name() == "zb_m_step_kernel" and not plain.terms_active
    ev = _sim(16, events=zm.ManagerEvents(cmd_ang_vel_z=(-0.5, 0.5)))
    assert ev.kernel_name() == "zb_m_events_step_kernel"
    dr = _sim(16)
    dr.set_base_inertia(torch.full((16,), 0.3), torch.zeros(16, 3))
    assert dr.kernel_name() == "zb_m_dr_step_kernel"
    on = _sim(16, terms=zm.ManagerTerms(weights={"gait": 0.5}))
    assert on.kernel_name() == "zb_m_terms_step_kernel"
    on.set_manager_terms(zm.ManagerTerms())
    assert on.kernel_name() == "zb_m_step_kernel" and not on.terms_active
    v2 = ZbotSim(8, zm.TaskCfg(solver_mode=1), device="cuda:0")
    assert v2.kernel_name() == "zb_step_kernel"
    import ctypes as C
    t = _all_terms().pack(zm.load_v09_model())
    assert v2.lib.zb_set_manager_terms(v2._h, C.byref(t), None) == -1 and b"manager-task" in v2.lib.zb_last_error()
    # the unedited env: the plain kernel and the 11 keys
    cfg = zbot_lab_amd.tasks.load_cfg("zbot-6b-walking-m-v0")
    cfg.scene.num_envs = 16
    env = zbot_lab_amd.make("zbot-6b-walking-m-v0", cfg=cfg)
    assert env.unwrapped.sim.kernel_name() == "zb_m_step_kernel"
    keys = list(env.unwrapped.reward_scales)
    assert len(keys) == 11 and not set(keys) & set(zm.M_EXTRA_REWARD_TERMS)


# ------------------------------------------------------------------ 5. graph safety
def test_graph_replay_equals_eager(gpu):
    import torch
    n = 64
    acts = torch.from_numpy(np.random.default_rng(1).normal(0, 0.6, (6, n, 6)).astype(np.float32)).cuda()

    def run(graph):
        s = _sim(n, seed=6, terms=_all_terms())
        s.reset(None)
        obs, rew = torch.empty(n, zm.M_OBS_DIM, device="cuda"), torch.empty(n, device="cuda")
        for k in range(5):
            s.step_into(acts[k], obs, rew)
        if graph:
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                s.step_into(acts[5], obs, rew)
            g.replay()   # (capture runs nothing: one replay is the sixth step)
        else:
            s.step_into(acts[5], obs, rew)
        torch.cuda.synchronize()
        return _np(s.get_state()), _np(s.get_terms_state()), _np(obs), _np(rew)

    eager, replay = run(False), run(True)
    assert eager[1][MT["EP_SUMS"]:MT["EP_SUMS"] + 5].any()
    for x, y in zip(eager, replay):
        np.testing.assert_array_equal(x, y)
