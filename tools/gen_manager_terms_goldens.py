"""Generate golden vectors for the manager env's five restored reward terms from the reference's OWN
code (build container only): ``gait``, ``feet_clearance``, ``feet_air_time``, ``base_vel_forward`` and
``feet_force_pattern`` of the base cfg's ``RewardsCfg`` (``zbotlab_env_cfg.py:301-366``).

The reference's ``mdp/rewards.py`` is imported with the stub ``isaaclab`` packages of
``gen_manager_goldens.py`` and every term is called through the cfg's own ``func`` / ``params`` on synthetic
articulation / contact-sensor frames: 32 envs x 16 calls of random frames, then three calls of constructed
rows (the gait phase edges of ``episode_length_buf``, command norms on both sides of 0.05 and 0.1, every
contact pattern, timers above and below 0.3, ``feet_force_sum`` zero / positive / negative), with a
``reset_my_data`` between two random calls and between two constructed ones. ``feet_force_sum`` is the
reference's own buffer (``init_my_data``) carried from call to call.

Output: ``tests/golden/mdp_manager_terms.npz`` (inputs and recorded outputs only).
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_manager_goldens import SceneEntityCfg, _Cfg, _Robot, _Scene, _Sensor, fields, fname, install_stubs  # noqa: E402
from gen_standup_goldens import random_quat  # noqa: E402

OUT = os.path.join(os.path.dirname(__file__), "..", "tests", "golden", "mdp_manager_terms.npz")
N, T = 32, 16
TERMS = ["gait", "feet_clearance", "feet_air_time", "base_vel_forward", "feet_force_pattern"]
FEET = [0, 11]
SIM_DT = 0.005
EDGE_EP_LEN = [0, 27, 28, 49, 50, 55, 77, 78, 99, 100, 155]


def random_call(rng):
    f = {}
    f["ep_len"] = rng.integers(0, 1000, N)
    cmd = np.stack([rng.uniform(-0.3, 0.3, N), rng.choice([0.0, 0.1, -0.2], N), rng.choice([0.0, 0.3], N)], 1)
    cmd[rng.random(N) < 0.2] = 0.0
    f["cmd"] = cmd
    in_c = rng.random((N, 2)) < 0.5
    k = rng.integers(1, 200, (N, 2)) * SIM_DT
    f["contact_time"] = np.where(in_c, k, 0.0)
    f["air_time"] = np.where(in_c, 0.0, k)
    f["foot_z"] = rng.uniform(0.0, 0.12, (N, 2))
    f["foot_vxy"] = rng.normal(0, 0.4, (N, 2, 2))
    f["root_quat"] = random_quat(rng, N)
    f["root_vel"] = rng.normal(0, 0.3, (N, 3))
    hist = rng.normal(0, 0.6, (N, 3, 2))
    # (forces of a few newtons: the recorded fp32 feet_force_pattern, 0.5 x a force difference, then resolves
    # the 1e-6 absolute that tests/test_manager_terms_reference.py holds the float64 statement to; at the
    # robot's 30 N weight one fp32 ulp of the term is already 1e-6)
    hist += np.where(rng.random((N, 3, 2)) < 0.5, rng.uniform(0, 4, (N, 3, 2)), 0)
    f["fz_hist"] = hist
    return f


def constructed_calls(rng):
    """Three calls: the gait phase edges x the contact patterns; the command-norm and timer gates; the
    integrator's sign cases (its value is set before that call)."""
    pats = [(1, 1), (1, 0), (0, 1), (0, 0)]
    a = random_call(rng)
    a["ep_len"] = np.array([EDGE_EP_LEN[i % len(EDGE_EP_LEN)] for i in range(N)])
    a["cmd"] = np.tile([0.2, 0.0, 0.0], (N, 1))
    for i in range(N):
        c = np.array(pats[(i // len(EDGE_EP_LEN) + i) % 4], bool)
        a["contact_time"][i] = np.where(c, 0.1, 0.0)
        a["air_time"][i] = np.where(c, 0.0, 0.1)
    b = random_call(rng)
    norms = [0.0, 0.0499, 0.05, 0.0501, 0.0999, 0.1, 0.1001, 0.2]
    times = [0.005, 0.295, 0.3, 0.305, 0.6]
    for i in range(N):
        v = norms[i % len(norms)]
        b["cmd"][i] = [(v, 0, 0), (0, v, 0), (0, 0, v), (-v, 0, 0)][(i // len(norms)) % 4]
        c = np.array(pats[i % 4], bool)
        t0, t1 = times[i % len(times)], times[(i // 2) % len(times)]
        b["contact_time"][i] = np.where(c, [t0, t1], 0.0)
        b["air_time"][i] = np.where(c, 0.0, [t1, t0])
    c_ = random_call(rng)
    c_["cmd"] = np.tile([0.0, 0.15, 0.0], (N, 1))
    force_sum = np.array([[0.0, 0.02, -0.02, 1e-6, -1e-6, 0.5, -0.5, 0.0][i % 8] for i in range(N)])
    return [a, b, c_], force_sum


def main():
    mdp = install_stubs()
    base = importlib.import_module("zbot.tasks.zbotlab_manager.zbotlab_env_cfg")
    rewards = base.RewardsCfg()
    terms = [(k, getattr(rewards, k)) for k in TERMS]
    order = [k for k, t in fields(rewards).items() if t is not None]
    rec = {k: dict(func=fname(t.func), weight=float(t.weight),
                   params={p: v for p, v in t.params.items() if not isinstance(v, SceneEntityCfg)}) for k, t in terms}

    rng = np.random.default_rng(20261020)
    robot, sensor = _Robot(), _Sensor()
    robot.data.GRAVITY_VEC_W = torch.tensor([0.0, 0.0, -1.0]).repeat(N, 1)
    cmd_now = {}
    step_dt = SIM_DT * 4
    env = types.SimpleNamespace(
        num_envs=N, device="cpu", sim=_Cfg(device="cpu"), scene=_Scene(robot, sensor),
        command_manager=_Cfg(get_command=lambda name: cmd_now["v"]),
        episode_length_buf=torch.zeros(N, dtype=torch.long), step_dt=step_dt)
    mdp.init_my_data(env, None)

    calls = [random_call(rng) for _ in range(T)]
    extra, force_sum_set = constructed_calls(rng)
    calls += extra
    reset_before = {8: [1, 4, 9], T + 2: [3, 5, 30]}   # reset_my_data runs before these calls
    set_before = T + 2                                  # feet_force_sum is set before this call (then the reset)
    out = {k: [] for k in ("terms", "force_sum_before", "force_sum_after")}
    resets = np.zeros((len(calls), N), bool)
    for t, f in enumerate(calls):
        f = {k: (v.astype(np.int64) if k == "ep_len" else v.astype(np.float32)) for k, v in f.items()}
        calls[t] = f
        if t == set_before:
            env.feet_force_sum[:] = torch.from_numpy(force_sum_set.astype(np.float32))
        if t in reset_before:
            ids = torch.tensor(reset_before[t])
            robot.data.body_link_pos_w = torch.zeros(N, 12, 3)
            mdp.reset_my_data(env, ids, SceneEntityCfg("robot", body_names="foot.*"))
            resets[t, reset_before[t]] = True
        pos = torch.zeros(N, 12, 3)
        pos[:, FEET, 2] = torch.from_numpy(f["foot_z"])
        vel = torch.zeros(N, 12, 3)
        vel[:, FEET, :2] = torch.from_numpy(f["foot_vxy"])
        hist = torch.zeros(N, 3, 12, 3)
        hist[:, :, FEET, 2] = torch.from_numpy(f["fz_hist"])
        ct, at = torch.zeros(N, 12), torch.zeros(N, 12)
        ct[:, FEET] = torch.from_numpy(f["contact_time"])
        at[:, FEET] = torch.from_numpy(f["air_time"])
        robot.data.body_pos_w, robot.data.body_lin_vel_w = pos, vel
        robot.data.root_quat_w = torch.from_numpy(f["root_quat"])
        robot.data.root_link_lin_vel_w = torch.from_numpy(f["root_vel"])
        sensor.data.net_forces_w_history = hist
        sensor.data.current_contact_time, sensor.data.current_air_time = ct, at
        env.episode_length_buf[:] = torch.from_numpy(f["ep_len"])
        cmd_now["v"] = torch.from_numpy(f["cmd"].copy())
        out["force_sum_before"].append(env.feet_force_sum.numpy().copy())
        out["terms"].append(torch.stack([tc.func(env, **tc.params).float() for _, tc in terms], 1).numpy())
        out["force_sum_after"].append(env.feet_force_sum.numpy().copy())

    gold = {"config_json": np.array(json.dumps(rec, default=float)), "term_names": np.array(TERMS),
            "reward_field_order": np.array(order), "step_dt": np.float64(step_dt), "resets": resets,
            "num_random_calls": np.int32(T)}
    for k in calls[0]:
        gold["in_" + k] = np.stack([f[k] for f in calls])
    for k, v in out.items():
        gold[k] = np.stack(v)
    np.savez_compressed(OUT, **gold)
    print("wrote", os.path.abspath(OUT), {k: np.asarray(v).shape for k, v in gold.items()})


if __name__ == "__main__":
    main()
