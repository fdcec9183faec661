"""The device's contact substeps (ZbotSim.physics_substeps) held to Newton's laws on the independent
float64 reference (tests/contact_laws.py), N = 130 (a partial wave and a partial workgroup), env e of
set e % 7, one substep and four.

Four substeps are four calls of ``physics_substeps(..., 1)`` with the state read back in between, on the
device and the f32 oracle alike; L1-L4 are evaluated on each transition from the *device's own* float32
pre-state. Every call invalidates the self-contact cache, so each substep detects its self contacts cold.

Bound: per law and set, the device's largest residual / floor (L1 balance, L2 internal self contact, L3
silence) is at most 3 x the f32 oracle's on the same initial states (the project's contact-free factor),
with a floor of 4 x the rounding floor; the bound is measured on the oracle, never on the device. L3's
exact zeros, L4 (unilateral, Coulomb cone), L5 (kinetic friction; the f64 oracle's measured constants)
and L6 hold outright. L6 is a coarse check: it only says that the moment rows put the ground force at the
one touching link.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import contact_laws as L
from test_base_inertia_cfg import HEAVY

pytestmark = pytest.mark.gpu
N = L.N


@functools.lru_cache(maxsize=None)
def _f32_oracle(config):
    rows, tg = L.case_states(L.CONFIGS[config][0])
    states, forces = L.oracle_chain(config, rows, tg, False)
    return {k: L.evaluate(config, states[:k + 1], forces[:k]) for k in (1, 4)}


def _device(config, nsub):
    import torch
    from zbot_lab_amd.sim import ZbotSim
    name = L.CONFIGS[config][0]
    cfg = L.make_cfg(config)
    rows, tg = L.case_states(name)
    sim = ZbotSim(N, cfg, device="cuda:0", seed=0)
    if config == "manager-heavy":
        mass, com = HEAVY
        sim.set_base_inertia(torch.full((N,), float(mass)), torch.tensor([com] * N, dtype=torch.float32))
        assert sim.base_inertia_active
        sim.check_base_inertia()
    st = np.zeros((cfg.state_dim, N), np.float32)
    st[:L.NPHYS] = rows
    for first, block in L.friction_state_rows(config).items():
        st[first:first + len(block)] = block
    sim.set_state(torch.from_numpy(st).cuda())
    if config == "standup-sd":
        mu_s, mu_d = L.link_friction(config)
        sim.set_link_friction(torch.from_numpy(mu_s), torch.from_numpy(mu_d))
    states, forces = [rows], []
    target = torch.from_numpy(tg).cuda()
    for _ in range(nsub):
        nf, _ = sim.physics_substeps(target, 1)
        torch.cuda.synchronize()
        forces.append(nf.cpu().numpy())
        states.append(sim.get_state().cpu().numpy()[:L.NPHYS])
    return np.stack(states), np.stack(forces)


@pytest.mark.parametrize("nsub", [1, 4])
@pytest.mark.parametrize("config", list(L.CONFIGS))
def test_device_contact_substeps_obey_the_laws(gpu, oracle_lib, config, nsub):
    oracle = _f32_oracle(config)[nsub]
    states, forces = _device(config, nsub)
    assert np.isfinite(states).all() and np.isfinite(forces).all()
    res = L.evaluate(config, states, forces)
    print("\n" + L.describe(f"{config} device, {nsub} substep(s)", res))
    print(L.describe(f"{config} f32 oracle, {nsub} substep(s)", oracle))
    failed = []
    for law, by_set in res["ratio"].items():
        for case, dev in by_set.items():
            f32 = oracle["ratio"][law][case]
            bound = max(L.DEVICE_FACTOR * f32, L.F64_FACTOR)
            print(f"[{config}, {nsub} substep(s)] {law} {case}: device {dev:.3g}, f32 oracle {f32:.3g} floors "
                  f"(ratio {dev / f32 if f32 else float('inf'):.3g}, bound 3; floor 4)")
            if dev > bound:
                failed.append((law, case, dev, bound))
    assert not failed, failed
    assert not res["violations"], res["violations"][:8]
    assert max(res["excluded"].values()) <= L.MAX_EXCLUDED and max(res["self_near"].values()) <= L.MAX_EXCLUDED
    assert res["loaded_folded"] >= 1.0 / 3.0
    L.assert_l5(res, f"{config} device")
