"""The contact substeps of the CPU oracle held to Newton's laws on the independent float64 reference
(tests/contact_laws.py: impulse balance, internal self contact, silence, the Coulomb cone, kinetic
friction, the lever arm). No GPU.

N = 130 states, env e of set e % 7 (resting, impact, sliding, sticking, one link, airborne folded,
airborne free), each set's condition asserted on the float64 geometry; four calls of one substep with the
state read back in between (every call invalidates the self-contact cache, so each substep detects its
self contacts cold), the laws evaluated on each transition from the runner's own float32 pre-state.

The f64 oracle (mass properties and joint frames in double) meets L1-L3 within 4 x the rounding floor and
L4-L6 outright on five configurations; the f32 oracle's largest residual / floor is printed per law,
configuration and set (DESIGN.md §6 holds the table). L6 is a coarse check: it only says that the
moment rows put the ground force at the one touching link, not where on it.

Planted errors, each missing its bound by >= 10 x on >= 90 % of the envs it can act on (the envs that
report a force of the kind it corrupts): the sensor force x 1.01 (the oracle's test hook) and gravity's C
omitted, against L1; the reaction on link b dropped and the reaction applied at link b's origin, against
L2; mu_dynamic in place of mu_static on sticking states under a tangential load, against L4.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import contact_laws as L
import test_oracle_dynamics as T

S = L.S


@functools.lru_cache(maxsize=None)
def _chain(config, double):
    rows, tg = L.case_states(L.CONFIGS[config][0])
    return L.oracle_chain(config, rows, tg, double)


@pytest.mark.parametrize("name", ["walking-v2", "standup", "manager"])
def test_case_sets_meet_their_conditions(name):
    L.assert_conditions(name)
    rows_a, _ = L.case_states("manager")
    rows_b, _ = L.case_states("manager-heavy")
    assert np.array_equal(rows_a, rows_b)


@pytest.mark.parametrize("config", list(L.CONFIGS))
def test_f64_oracle_obeys_the_laws(oracle_lib, config):
    states, forces = _chain(config, True)
    res = L.evaluate(config, states, forces)
    print("\n" + L.describe(f"{config} f64 oracle", res))
    for law, by_set in res["ratio"].items():
        for case, v in by_set.items():
            assert v <= L.F64_FACTOR, (law, case, v)
    assert not res["violations"], res["violations"][:8]
    assert max(res["excluded"].values()) <= L.MAX_EXCLUDED and max(res["self_near"].values()) <= L.MAX_EXCLUDED
    assert res["loaded_folded"] >= 1.0 / 3.0
    for substep in (1, 4):     # the recorded constants are the f64 oracle's: no configuration falls below them
        ratio, cos = L.l5_smallest(res, substep)
        assert ratio >= L.L5_MEASURED[substep][0] and cos >= L.L5_MEASURED[substep][1], (substep, ratio, cos)


@pytest.mark.parametrize("config", list(L.CONFIGS))
def test_f32_oracle_obeys_the_laws(oracle_lib, config):
    """The f32 oracle's residual / floor is recorded (printed), not bounded: it is the yardstick of the
    device's bound in tests/test_gpu_contact_laws.py. L4-L6 hold outright."""
    states, forces = _chain(config, False)
    res = L.evaluate(config, states, forces)
    print("\n" + L.describe(f"{config} f32 oracle", res))
    assert not res["violations"], res["violations"][:8]
    assert max(res["excluded"].values()) <= L.MAX_EXCLUDED and max(res["self_near"].values()) <= L.MAX_EXCLUDED
    assert res["loaded_folded"] >= 1.0 / 3.0
    L.assert_l5(res, f"{config} f32 oracle")


# ------------------------------------------------------------------ planted errors
def _caught(tag, ratio, bound=L.F64_FACTOR, least=10):
    """``ratio``: residual / floor of the envs the error can act on."""
    miss = np.asarray(ratio) / bound
    print(f"\n[planted: {tag}] residual / bound over {len(miss)} env transitions: median {np.median(miss):.3g}, min {miss.min():.3g}; "
          f"at >= 10: {(miss >= 10).mean():.1%}")
    assert len(miss) >= least and (miss >= 10.0).mean() >= 0.9


def test_planted_sensor_force_scale_fails_l1(oracle_lib):
    config = "walking-v2-pgs"
    rows, tg = L.case_states("walking-v2")
    lib = oracle_lib.lib(True)
    lib.zbo_set_sensor_force_scale(1.01)
    try:
        states, forces = L.oracle_chain(config, rows, tg, True)
    finally:
        lib.zbo_set_sensor_force_scale(1.0)
    res = L.evaluate(config, states, forces)
    ground = np.abs(forces.astype(np.float64).sum(axis=2)).max(axis=2) > L.LOADED     # [k, n]: a net ground force
    _caught("sensor force x 1.01 vs L1", res["per_env"]["L1"][ground & np.isfinite(res["per_env"]["L1"])])
    clean = L.evaluate(config, *_chain(config, True))
    assert np.nanmax(clean["per_env"]["L1"]) <= L.F64_FACTOR


def test_planted_gravity_omitted_fails_l1(oracle_lib):
    config = "manager"
    res = L.evaluate(config, *_chain(config, True), mutant="no_gravity_C")
    v = res["per_env"]["L1"]
    _caught("gravity's C omitted vs L1", v[np.isfinite(v)])


@pytest.mark.parametrize("mutant,law", [("drop_reaction", "L2f"), ("reaction_at_origin", "L2r")])
def test_planted_self_contact_errors_fail_l2(oracle_lib, mutant, law):
    """On the recorded per-link forces: link b is the highest loaded link of a folded env (pairs are
    stored a < b). The recorded output has no contact point; the moment is shifted by (p_b - p) x F with
    p the mean of the two hulls' circle centres, a point as far from link b's origin as the contact is."""
    ratios = []
    for config in ("walking-v2-tgs-rf", "manager"):
        states, forces = _chain(config, True)
        res = L.evaluate(config, states, forces, mutant=mutant)
        loaded = (np.abs(forces) > 0).any(axis=3).sum(axis=2) >= 2          # [k, n]: two links report a force
        loaded[:, np.arange(L.N) % L.K != L.SETS.index("airborne_folded")] = False
        v = res["per_env"][law]
        ratios.append(v[loaded & np.isfinite(v)])
    _caught(f"{mutant} vs {law}", np.concatenate(ratios))


def test_planted_dynamic_for_static_friction_fails_l4(oracle_lib):
    """Sticking states under a tangential load: every link mu_s = 1.2, mu_d = 0.2, the lowest hull point
    0.2-1 mm inside the ground (the lower part of the resting set's range, so that every env carries a
    load from the first substep), and the horizontal speed set so that stopping it within the substep
    takes 0.35 x the normal force the same state carries at rest (measured in a first run): outside the
    dynamic cone and far enough inside the static one that no contact breaks. (Nearer the static cone
    Gauss-Seidel loads the first contact of a many-contact env past it; that contact breaks and slides
    at mu_d, the env's friction lies inside the dynamic cone on every link and nothing static is left
    for the planted error to mistake: at 0.9 x and mu_d = 0.6 that happens in 4 of 11 loaded envs.)"""
    config, name = "standup-sd", "standup"
    rows, tg = L.case_states(name)
    mu = (np.full((L.N, L.NL), 1.2, np.float32), np.full((L.N, L.NL), 0.2, np.float32))
    stick = L.envs_of("sticking")
    low = L.geometry_facts(name)[0].min(axis=1)
    for e in stick:
        if low[e] > -0.2e-3:
            rows[S["ROOT_POS"] + 2, e] -= np.float32(low[e] + 0.3e-3)
            low[e] = -0.3e-3
    assert (low[stick] >= -1e-3 - 1e-7).all() and (low[stick] <= -0.2e-3 + 1e-7).all()
    rows[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 2, stick] = 0.0
    _, f0 = L.oracle_chain(config, rows, tg, True, nsub=1, mu=mu)
    fz = f0[0][:, :, 2].astype(np.float64).sum(axis=1)
    ref = T.reference(name, L.make_cfg(config))
    speed = 0.35 * fz * ref.dt / ref.mass.sum()
    a = np.random.default_rng(5).uniform(-np.pi, np.pi, L.N)
    rows[S["ROOT_LINVEL"], stick] = (speed * np.cos(a))[stick]
    rows[S["ROOT_LINVEL"] + 1, stick] = (speed * np.sin(a))[stick]
    states, forces = L.oracle_chain(config, rows, tg, True, nsub=1, mu=mu)
    clean = L.evaluate(config, states, forces, mu=mu, l6=False)
    assert not [v for v in clean["violations"] if v.startswith("L4: sticking")], clean["violations"][:4]
    bad = L.evaluate(config, states, forces, mu=mu, l6=False, mutant="mu_dynamic")
    loaded = fz[stick] > L.LOADED
    print(f"\n[planted: mu_dynamic for mu_static] {int(loaded.sum())} of {len(stick)} sticking envs carry a load")
    assert loaded.all()
    # the bound here is the cone itself + the force's rounding floor: the miss is counted in floors
    _caught("mu_dynamic for mu_static vs L4", bad["cone_miss"][0, stick][loaded], bound=1.0)
