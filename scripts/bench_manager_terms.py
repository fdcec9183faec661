#!/usr/bin/env python
"""Cost of the manager task's five restored reward terms (include/zbot_manager_terms.h) per env step, 4096
envs: warm-up first, interleaved rounds (A B C A B C ...), medians and the run-to-run spread stated.

    python scripts/bench_manager_terms.py --envs 4096 --steps 400 --rounds 7 --out profiles/manager_terms/bench_ab.json

In-process arms, one build: "off" (zb_m_step_kernel), "dr" (zb_m_dr_step_kernel: per-env base inertia, push +
heading events) and "terms" (zb_m_terms_step_kernel: the same inertia and events, all five terms on). The
cost reported is terms over dr. The "off" arm runs the kernels the parent commit runs
(profiles/manager_terms/kernel_resources.txt: instruction-identical). bench.py is the project's benchmark
and enables none of this.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARMS = ("off", "dr", "terms")
KERNEL = {"off": "zb_m_step_kernel", "dr": "zb_m_dr_step_kernel", "terms": "zb_m_terms_step_kernel"}
WEIGHTS = {"gait": 0.5, "feet_clearance": 1.0, "feet_air_time": 2.5, "base_vel_forward": 1.0, "feet_force_pattern": 1.0}


def measure(args, names) -> dict:
    import zbot_lab_amd  # noqa: F401
    import torch
    from zbot_lab_amd import model as zm
    from zbot_lab_amd.sim import ZbotSim
    n = args.envs
    events = zm.ManagerEvents(push_enabled=True, push_interval_s=(10.0, 15.0),
                              push_velocity_range=((-0.5, 0.5), (-0.5, 0.5)) + ((0.0, 0.0),) * 4,
                              cmd_ang_vel_z=(-1.0, 1.0), heading_command=True, cmd_heading=(-math.pi, math.pi))
    g = torch.Generator(device="cuda").manual_seed(0)
    m0 = float(zm.pack_base_link(zm.load_v09_model()).mass)
    mass = m0 + torch.rand(n, device="cuda", generator=g) * 0.4 - 0.1
    com = (torch.rand(n, 3, device="cuda", generator=g) * 2 - 1) * torch.tensor([0.03, 0.02, 0.01], device="cuda")
    arms = {}
    for name in names:
        sim = ZbotSim(n, zm.TaskCfg.manager_flat(solver_mode=1, self_manifold=2), device="cuda:0", seed=0)
        if name != "off":
            sim.set_manager_events(events)
            sim.set_base_inertia(mass, com)
        if name == "terms":
            sim.set_manager_terms(zm.ManagerTerms(weights=dict(WEIGHTS)))
        sim.reset(None)
        assert sim.kernel_name() == KERNEL[name]
        arms[name] = sim
    acts = torch.randn(64, n, zm.ACT_DIM, device="cuda", generator=g)
    obs, rew = torch.empty(n, zm.M_OBS_DIM, device="cuda"), torch.empty(n, device="cuda")

    def run(sim, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            sim.step_into(acts[k % 64], obs, rew)
        torch.cuda.synchronize()
        return n * steps / (time.perf_counter() - t0)

    for sim in arms.values():
        run(sim, args.warmup)
    rates = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, sim in arms.items():
            rates[name].append(run(sim, args.steps))
    return {"device": torch.cuda.get_device_name(0), "env_steps_per_s": rates}


def summarise(rates: dict) -> dict:
    med = {k: statistics.median(v) for k, v in rates.items()}
    return {"median": med, "spread": {k: (max(v) - min(v)) / med[k] for k, v in rates.items()}}


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    res = {"envs": args.envs, "steps": args.steps, "rounds": args.rounds}
    m = measure(args, [a for a in args.arms.split(",") if a])
    res.update(m, **summarise(m["env_steps_per_s"]))
    med = res["median"]
    if "terms" in med and "dr" in med:
        res["terms_over_dr_minus_1"] = med["terms"] / med["dr"] - 1.0
    if "dr" in med and "off" in med:
        res["dr_over_off_minus_1"] = med["dr"] / med["off"] - 1.0
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
