"""The device's contact-free substeps (ZbotSim.physics_substeps) against the independent float64
reference of tests/dynamics_reference.py, N = 130 (a partial wave and a partial workgroup), 130
distinct states of the six case sets mixed (generic, gyroscopic, saturated, speed clamp, angular cap,
joint wrap; env e is of set e % 6), one and four substeps.

Bound per row class (velocities; position and quaternion; joint angles; applied torque): the device's
largest error against the reference is at most 3 x the f32 oracle's against the same reference on the
same states (the project's contact-free factor, tests/test_gpu_base_inertia.py), with a floor of
2 ulp32. (The rows both read, pack_model's, are held absolutely on these same 130 states by
tests/test_oracle_dynamics.py::test_packed_model_matches_reference[*-mixed], so an error the two share
cannot hide in the ratio.) Discrete outcomes (which joint saturated / was clamped / wrapped and with which sign, whether
the angular cap acted) equal the reference's wherever the reference is not within 1e-5 (relative) of
the threshold; at most 2 % of them are that close. The speed clamp, the cap and the wrap are read off
the device's state; a saturation off the joint torque the device's velocity change implies through the
reference's M and C (one substep, envs without a clamp or cap, whose projection would hide it; the
saturated set holds states built for this: one mid-chain joint saturates and nothing is clamped).
After four substeps the device's state at the start of the last one is not known to better than its
own error, so there a saturation decision is not checked as an outcome: the error bound alone holds it.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import dynamics_reference as D
import test_oracle_dynamics as T
from test_base_inertia_cfg import HEAVY
from zbot_lab_amd import model as zm

pytestmark = pytest.mark.gpu
N, S, ND, NPHYS = 130, zm.S, zm.NUM_DOF, D.NPHYS
VEL = np.r_[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 6, S["JOINT_VEL"]:S["JOINT_VEL"] + ND]
CLASSES = {"velocity": VEL, "position / quaternion": np.r_[S["ROOT_POS"]:S["ROOT_POS"] + 7],
           "joint angle": np.r_[S["JOINT_POS"]:S["JOINT_POS"] + ND]}
# handle -> (model of tests/test_oracle_dynamics.py, solver_mode)
HANDLES = {"walking-v2-pgs": ("walking-v2", 0), "walking-v2-tgs": ("walking-v2", 1), "standup": ("standup", 1),
           "manager": ("manager", 1), "manager-heavy": ("manager-heavy", 1)}


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(rows, targets, the reference's four substeps) of the 130 mixed states; shared, never written to."""
    rows, tg = D.mixed_states(T.robot(name), N)
    return rows, tg, T.reference(name, T.make_cfg(name)).run(rows, tg, 4)


@functools.lru_cache(maxsize=None)
def _f32_oracle(name, mode):
    rows, tg, _ = _reference(name)
    out1, at1, _ = T.oracle_substeps(name, T.make_cfg(name, solver_mode=mode), rows, tg, nsubs=(1,), double=False)
    out4, at4, _ = T.oracle_substeps(name, T.make_cfg(name, solver_mode=mode), rows, tg, nsubs=(4,), double=False)
    return {1: (out1[1], at1), 4: (out4[4], at4)}


def _device(handle, nsub):
    import torch
    from zbot_lab_amd.sim import ZbotSim
    name, mode = HANDLES[handle]
    cfg = T.make_cfg(name, solver_mode=mode)
    rows, tg, _ = _reference(name)
    sim = ZbotSim(N, cfg, device="cuda:0", seed=0)
    if handle == "manager-heavy":
        mass, com = HEAVY
        sim.set_base_inertia(torch.full((N,), float(mass)), torch.tensor([com] * N, dtype=torch.float32))
        assert sim.base_inertia_active
        sim.check_base_inertia()
    st = np.zeros((cfg.state_dim, N), np.float32)
    st[:NPHYS] = rows
    sim.set_state(torch.from_numpy(st).cuda())
    _, tau = sim.physics_substeps(torch.from_numpy(tg).cuda(), nsub)
    torch.cuda.synchronize()
    return sim.get_state().cpu().numpy()[:NPHYS], tau.cpu().numpy()


def _implied_saturation(name, rows, tg, dev):
    """Sign of each joint the device saturated in one substep, from its velocity change: the joint torque
    tau = (M du / dt + C) is +-effort on a saturated joint and the implicit law's value on the others."""
    ref = T.reference(name, T.make_cfg(name))
    out = np.zeros((N, ND), int)
    for e in range(N):
        pos, quat, q, u = T._split(rows[:, e].astype(np.float64))
        d = ref.dynamics(pos, quat, q, u)
        x = dev[:, e].astype(np.float64)
        u1 = np.concatenate([x[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3], x[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3],
                             x[S["JOINT_VEL"]:S["JOINT_VEL"] + ND]])
        tau = (d["M"] @ (u1 - u) / ref.dt + d["C"])[6:]
        arm = ref.dt * ref.kd + ref.dt ** 2 * ref.kp
        law = ref.kp * (tg[e] - q) - (ref.kd + ref.dt * ref.kp) * u[6:] - (arm / ref.dt) * (u1[6:] - u[6:])
        sign = np.sign(tau)
        out[e] = np.where(np.abs(tau - sign * ref.effort) < np.abs(tau - law), sign, 0).astype(int)
    return out


@pytest.mark.parametrize("nsub", [1, 4])
@pytest.mark.parametrize("handle", list(HANDLES))
def test_device_substeps_match_reference(gpu, oracle_lib, handle, nsub):
    name, mode = HANDLES[handle]
    rows, tg, r = _reference(name)
    ref_state = r["states"][nsub - 1]
    # applied torque: the explicit estimate at the start of the last substep
    ref1 = T.reference(name, T.make_cfg(name))
    start = rows.astype(np.float64) if nsub == 1 else r["states"][nsub - 2]
    q0, qd0 = start[S["JOINT_POS"]:S["JOINT_POS"] + ND].T, start[S["JOINT_VEL"]:S["JOINT_VEL"] + ND].T
    ref_tau = np.clip(ref1.kp * (tg.astype(np.float64) - q0) - ref1.kd * qd0, -ref1.effort, ref1.effort)
    f32_state, f32_tau = _f32_oracle(name, mode)[nsub]
    dev, dev_tau = _device(handle, nsub)
    assert np.isfinite(dev).all()

    # ---- error per row class over the 130 states (asserted), and per case set (printed: the largest of
    # some 22 envs' errors is a noisy figure, measured at up to 3.07 x the f32 oracle's for the speed-clamp
    # set of walking-v2 where the class as a whole is at 1.41)
    bounds = {}
    sets = np.arange(N) % len(D.CASE_SETS)
    for cls, idx in CLASSES.items():
        err_dev = np.abs(dev[idx].astype(np.float64) - ref_state[idx])
        err_f32 = np.abs(f32_state[idx].astype(np.float64) - ref_state[idx])
        per_set = ", ".join(f"{case} {err_dev[:, sets == k].max() / err_f32[:, sets == k].max():.3g}"
                            for k, case in enumerate(D.CASE_SETS))
        e_dev, e_f32 = float(err_dev.max()), float(err_f32.max())
        floor = float(2 * D.ulp32(np.abs(ref_state[idx]).max()))
        bounds[cls] = max(3.0 * e_f32, floor)
        print(f"[{handle}, {nsub} substep(s)] {cls}: device vs reference {e_dev:.3g}, f32 oracle vs reference {e_f32:.3g} "
              f"(ratio {e_dev / e_f32:.3g}, bound 3; floor {floor:.3g}); ratio per set: {per_set}")
        assert e_dev <= bounds[cls], cls
    e_dev = float(np.abs(dev_tau.astype(np.float64) - ref_tau).max())
    e_f32 = float(np.abs(f32_tau.astype(np.float64) - ref_tau).max())
    floor = float(2 * D.ulp32(np.abs(ref_tau).max()))
    print(f"[{handle}, {nsub} substep(s)] applied torque: device vs reference {e_dev:.3g}, f32 oracle vs reference {e_f32:.3g} "
          f"(floor {floor:.3g})")
    assert e_dev <= max(3.0 * e_f32, floor)

    # ---- discrete outcomes of the last substep (and the net wrap of all of them)
    k = nsub - 1
    share = T.near_share(r, nsub)
    print(f"[{handle}, {nsub} substep(s)] reference decisions within {T.NEAR:g} of a threshold: {share:.4%}")
    assert share <= 0.02
    pm = zm.pack_model(T.robot(name))
    vlim, wmax = np.float32(pm.velocity_limit), float(pm.max_angular_velocity)
    qd = dev[S["JOINT_VEL"]:S["JOINT_VEL"] + ND].T
    dev_clamp = np.where(qd == vlim, 1, np.where(qd == -vlim, -1, 0))
    far = r["clamp_margin"][k] >= T.NEAR
    assert (dev_clamp == r["clamp"][k])[far].all()
    assert np.abs(qd).max() <= vlim
    w = np.linalg.norm(dev[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3].astype(np.float64), axis=0)
    dev_cap = np.abs(w - wmax) <= 8 * float(np.spacing(np.float32(wmax)))
    far = r["cap_margin"][k] >= T.NEAR
    assert (dev_cap == r["cap"][k])[far].all() and w.max() <= wmax * (1 + 1e-6)
    far = (r["wrap_margin"][:nsub] >= T.NEAR).all(axis=0)
    dq = (dev[S["JOINT_POS"]:S["JOINT_POS"] + ND].astype(np.float64) - ref_state[S["JOINT_POS"]:S["JOINT_POS"] + ND]).T
    assert (np.abs(dq) < 1.0)[far].all()   # a wrap taken by one side only is 4 pi off
    assert (r["wrap"][:nsub] != 0).any() and np.abs(dev[S["JOINT_POS"]:S["JOINT_POS"] + ND]).max() <= 2 * np.pi * (1 + 1e-6)
    if nsub == 1:
        free = ~(r["clamp"][0] != 0).any(axis=1) & ~r["cap"][0]
        got = _implied_saturation(name, rows, tg.astype(np.float64), dev)
        far = (r["sat_margin"][0] >= T.NEAR) & free[:, None]
        print(f"[{handle}] saturation read back on {int(free.sum())} envs without a clamp or cap: "
              f"{int((r['sat'][0][far] != 0).sum())} saturated joints")
        assert (r["sat"][0][far] > 0).sum() >= 1 and (r["sat"][0][far] < 0).sum() >= 1   # each sign, every handle
        assert (got == r["sat"][0])[far].all()

    # ---- a device reading the nominal table cannot pass
    if handle == "manager-heavy":
        assert np.array_equal(_reference("manager")[0], rows)
        nominal = _reference("manager")[2]["states"][nsub - 1]
        Dv = float(np.abs(ref_state[VEL] - nominal[VEL]).max())
        print(f"[{handle}, {nsub} substep(s)] heavy vs nominal reference, velocity rows: D = {Dv:.4g} "
              f"({Dv / bounds['velocity']:.3g} x the bound)")
        assert Dv >= 100.0 * bounds["velocity"]
