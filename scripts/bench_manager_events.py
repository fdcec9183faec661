#!/usr/bin/env python
"""Cost of the manager task's events (interval push + heading command) per env step: events off against
events on, same process, same build, interleaved rounds (A B A B ...), warm-up first, spread stated.

    python scripts/bench_manager_events.py --envs 4096 --steps 400 --rounds 7 --out profiles/manager_events/bench_ab.json

Prints one JSON line: env-steps/s of each arm per round, the medians, the run-to-run spread (max - min
over rounds, relative to the median) and on / off - 1. bench.py is the project's benchmark and does not
enable events; this script only answers what they cost.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zbot_lab_amd  # noqa: E402,F401
import torch  # noqa: E402

from zbot_lab_amd import model as zm  # noqa: E402
from zbot_lab_amd.sim import ZbotSim  # noqa: E402


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    n = args.envs
    events = zm.ManagerEvents(push_enabled=True, push_interval_s=(10.0, 15.0),
                              push_velocity_range=((-0.5, 0.5), (-0.5, 0.5)) + ((0.0, 0.0),) * 4,
                              cmd_ang_vel_z=(-1.0, 1.0), heading_command=True, cmd_heading=(-math.pi, math.pi))
    arms = {}
    for name in ("off", "on"):
        sim = ZbotSim(n, zm.TaskCfg.manager_flat(solver_mode=1, self_manifold=2), device="cuda:0", seed=0)
        if name == "on":
            sim.set_manager_events(events)
        sim.reset(None)
        arms[name] = sim
    assert arms["on"].events_active and not arms["off"].events_active
    g = torch.Generator(device="cuda").manual_seed(0)
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
    rates = {"off": [], "on": []}
    for _ in range(args.rounds):
        for name, sim in arms.items():
            rates[name].append(run(sim, args.steps))
    med = {k: statistics.median(v) for k, v in rates.items()}
    res = {"envs": n, "steps": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "env_steps_per_s": rates, "median": med,
           "spread": {k: (max(v) - min(v)) / med[k] for k, v in rates.items()},
           "on_over_off_minus_1": med["on"] / med["off"] - 1.0}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
