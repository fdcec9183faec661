"""The laws of the counter-based random draws, on the CPU.

1. The statistics helper (tests/random_laws.py) catches planted faults: each fault is planted in numpy
   on synthetic streams of the sizes the device tests use (65 536 envs for reset / observe scenarios,
   3 x 16 384 pooled where a step is needed, 16 384 x 6 action-noise draws) under the same thresholds
   with the whole statistic budget reserved (random_laws.BUDGET, which no scenario exceeds: the plants'
   thresholds are at least as wide as any scenario's). Every plant fails, the clean stream passes: the
   device tests are not vacuous. The observation-noise plants (a half-width off by 2 %) run through the
   scenarios' own check_noise at each scenario's n and number of calls. One plant is below the
   resolution of 65 536 samples and uses 2^20, as does the check it stands for: a Bernoulli parameter
   of 0.02 off by 10 % (the manager's standing flag at reset: 16 pooled resets). The same flag at the
   10 s resample and at the in-step reset has 3 x 16 384 samples at the most (the 3-step limit), which
   resolve about 15 %; 10 % there is resolved at 0.25 only. sigma = 0.98 is resolved at 98 304 draws by
   the variance statistic, not by Kolmogorov-Smirnov, and a range scaled about its centre by the width
   statistic, which is why ``Laws.normal`` and ``Laws.uniform`` carry them.
2. The oracle's streams obey their laws, all four tasks (tests/random_streams.py: the scenarios shared
   with tests/test_gpu_random_streams.py).
3. The numpy restatement of the action-noise draw (ppo_mlp.hip noise_at) obeys the standard normal law
   at 2^20 samples, and its key is injective on the documented range and collides just outside it.

Seeds: fixed below before the first run. None had to be replaced.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import random_streams as rs
from random_laws import LAGS, Laws, chi2_quantile, ks_threshold, kolmogorov_sf, normal_quantile

SEED_PLANTS = 20261020          # numpy generator of the synthetic streams
SEED_ORACLE = 42                # the env seed of rank 0 (ranks run with 42 + rank)
NOISE_SEED, NOISE_COUNTER, NOISE_STEP = 1234567, 3, 7
N_RESET, N_POOLED, N_ACT = rs.N_RESET, 3 * rs.N_STEP, (rs.N_STEP, 6)


# ----------------------------------------------------------------------------- thresholds
def test_threshold_helpers_against_known_quantiles():
    """Textbook values: Kolmogorov 1.358 (5 %), 1.628 (1 %); chi-square(49) 5 % 66.34, chi-square(1)
    5 % 3.841; normal 97.5 % 1.960."""
    assert abs(ks_threshold(0.05) - 1.3581) < 1e-3 and abs(ks_threshold(0.01) - 1.6276) < 1e-3
    assert abs(kolmogorov_sf(1.0) - 0.27) < 1e-3
    assert abs(chi2_quantile(49, 0.05) - 66.339) < 0.05 and abs(chi2_quantile(1, 0.05) - 3.8415) < 1e-3
    assert abs(normal_quantile(0.975) - 1.95996) < 1e-4


# ----------------------------------------------------------------------------- planted faults
def _clean_env_streams(rng, n, cols=4):
    """What a reset scenario collects: ``cols`` uniform columns of two calls and a second seed."""
    return [rng.random((cols, n)) for _ in range(3)]


def _env_laws(call0, call1, seed1, lo=0.0, hi=1.0):
    """The checks every env-event scenario applies (random_streams: marginals, column correlation,
    serial correlation, call / seed freshness)."""
    L = Laws()
    names = [f"c{k}" for k in range(len(call0))]
    for k, nm in enumerate(names):
        L.uniform(nm, call0[k], lo, hi)
        L.serial(nm, call0[k])
        L.fresh(f"call {nm}", call0[k], call1[k])
        L.fresh(f"seed {nm}", call0[k], seed1[k])
    L.uncorrelated("columns", dict(zip(names, call0)))
    L.reserve()
    return L


def _plant_env(fault, rng, n):
    a, b, c = _clean_env_streams(rng, n)
    if fault == "clean":
        pass
    elif fault == "two columns from one draw":
        a[1] = a[0].copy()
    elif fault == "two columns from one draw, affinely mapped":
        a[1] = 1.0 - a[0]
    elif fault == "call repeats the previous call's stream":
        b = a.copy()
    elif fault == "env i+1 reads env i's stream (next call)":
        b[:, 1:] = a[:, :-1]
    elif fault == "env i+1 reads env i's stream (same call)":
        a[:, 1::2] = a[:, 0::2]
    elif fault == "seed ignored":
        c = a.copy()
    elif fault == "u01 in [0, 0.5)":
        a[2] *= 0.5
    elif fault == "Weyl sequence":
        a[3] = np.modf(np.arange(1, n + 1) * ((math.sqrt(5.0) - 1.0) / 2.0))[0]
    elif fault == "range scaled by 0.98":
        a[0] *= 0.98
    elif fault == "range scaled by 0.98 about its centre":
        a[0] = 0.5 + 0.98 * (a[0] - 0.5)
    else:
        raise KeyError(fault)
    return _env_laws(a, b, c)


ENV_FAULTS = ["two columns from one draw", "two columns from one draw, affinely mapped",
              "call repeats the previous call's stream", "env i+1 reads env i's stream (next call)",
              "env i+1 reads env i's stream (same call)", "seed ignored", "u01 in [0, 0.5)", "Weyl sequence",
              "range scaled by 0.98", "range scaled by 0.98 about its centre"]


@pytest.mark.parametrize("n", [N_RESET, N_POOLED], ids=["reset-65536", "step-3x16384"])
def test_clean_env_streams_pass(n):
    L = _plant_env("clean", np.random.default_rng(SEED_PLANTS), n)
    L.check("clean numpy streams")


@pytest.mark.parametrize("n", [N_RESET, N_POOLED], ids=["reset-65536", "step-3x16384"])
@pytest.mark.parametrize("fault", ENV_FAULTS)
def test_planted_env_fault_is_caught(fault, n):
    L = _plant_env(fault, np.random.default_rng(SEED_PLANTS), n)
    print(L.report(fault))
    assert L.failures(), fault


def test_weyl_marginal_passes_ks_and_fails_only_the_serial_test():
    n = N_RESET
    x = np.modf(np.arange(1, n + 1) * ((math.sqrt(5.0) - 1.0) / 2.0))[0]
    L = Laws()
    L.uniform("weyl", x, 0.0, 1.0)
    assert not L.failures()
    L.serial("weyl", x, LAGS)
    assert L.failures() and all("serial" in f for f in L.failures())


@pytest.mark.parametrize("p,n", [(0.25, N_RESET), (0.25, N_POOLED), (0.8, N_RESET), (0.8, N_POOLED), (0.02, 1 << 20)])
def test_planted_bernoulli_parameter_is_caught(p, n):
    """10 % relative. At p = 0.02 and 65 536 samples the shift is 3.6 sd, below a Bonferroni threshold:
    2^20 samples (the device test pools 16 resets for that flag)."""
    rng = np.random.default_rng(SEED_PLANTS)
    for q, bad in ((p, False), (p * 1.1 if p < 0.5 else p * 0.9, True)):
        L = Laws()
        L.bernoulli("flag", rng.random(n) < q, p)
        L.reserve()
        assert bool(L.failures()) == bad, (q, L.report())


def _noise_laws(z):
    L = Laws()
    rs.check_action_noise(L, "noise", z)
    L.reserve()
    return L


@pytest.mark.parametrize("fault", ["clean", "sigma 0.98", "tails cut at 3 sigma", "two actions share a draw",
                                   "row i+1 repeats row i"])
def test_planted_action_noise_fault_is_caught(fault):
    rng = np.random.default_rng(SEED_PLANTS)
    z = rng.standard_normal(N_ACT)
    if fault == "sigma 0.98":
        z *= 0.98
    elif fault == "tails cut at 3 sigma":
        while (np.abs(z) > 3.0).any():
            bad = np.abs(z) > 3.0
            z[bad] = rng.standard_normal(int(bad.sum()))
    elif fault == "two actions share a draw":
        z[:, 4] = -z[:, 1]
    elif fault == "row i+1 repeats row i":
        z[1::2] = z[0::2]
    L = _noise_laws(z)
    print(L.report(fault))
    assert bool(L.failures()) == (fault != "clean")


NOISE_SCENARIOS = {"observe": (rs.N_RESET, 2), "step": (rs.N_STEP, 3), "in-step reset": (rs.N_STEP, 1)}


@pytest.mark.parametrize("scenario", list(NOISE_SCENARIOS))
@pytest.mark.parametrize("cls", [None] + list(rs.NOISE_CLASSES))
def test_planted_noise_half_width_is_caught(scenario, cls):
    """The manager's observation noise through the scenarios' own check_noise, at each scenario's n and
    number of calls: one class's half-width off by 2 % (0.98 U(-1, 1)) fails, the clean noise passes."""
    n, calls = NOISE_SCENARIOS[scenario]
    rng = np.random.default_rng(SEED_PLANTS)
    nz = [{f"noise{c}": rng.uniform(-1.0, 1.0, n) for c in rs.NOISE_COLS} for _ in range(calls)]
    for call in nz:
        for k in (rs.NOISE_CLASSES[cls] if cls else []):
            call[k] *= 0.98
    L = Laws()
    rs.check_noise(L, "noise", nz, 0.0)
    L.reserve()
    print(L.report(f"{scenario}, {cls}"))
    bad = L.failures()
    assert bool(bad) == (cls is not None)
    assert cls is None or any(f"{cls} half-width class" in f for f in bad)   # (the pooled class resolves it)


# ----------------------------------------------------------------------------- action-noise restatement
def test_noise_restatement_obeys_the_normal_law():
    """2^20 draws of the numpy restatement of noise_at (the device is held to it within 1e-4,
    tests/test_gpu_random_streams.py): the laws of one call, and independence across the step, the
    draw counter and the seed."""
    rows, na = (1 << 20) // 8, 8
    z = rs.noise_at(NOISE_SEED, NOISE_COUNTER, NOISE_STEP, rows, na)
    L = Laws()
    rs.check_action_noise(L, "restatement", z)
    for name, other in (("step k / k+1", rs.noise_at(NOISE_SEED, NOISE_COUNTER, NOISE_STEP + 1, rows, na)),
                        ("counter c / c+1", rs.noise_at(NOISE_SEED, NOISE_COUNTER + 1, NOISE_STEP, rows, na)),
                        ("seed s / s+1", rs.noise_at(NOISE_SEED + 1, NOISE_COUNTER, NOISE_STEP, rows, na))):
        L.fresh(f"restatement {name}", z, other)
    L.check("noise_at restatement, 2^20 draws")


def test_noise_key_is_injective_on_its_range_only():
    """include/zbot_ppo.h: 0 <= noise_step < 4096 and draw counter < 2^20. Just outside, two triples
    share a key (which is why zbp_act refuses such a noise_step)."""
    rng = np.random.default_rng(SEED_PLANTS)
    keys = {rs.noise_key(s, c, k) for s in (0, 1, 2 ** 31 - 1) for c in (0, 1, 2 ** 20 - 1) for k in (0, 1, 4095)}
    assert len(keys) == 27
    s, c, k = (int(v) for v in (rng.integers(0, 2 ** 31 - 1), rng.integers(0, 2 ** 20 - 1), rng.integers(0, 4096)))
    assert rs.noise_key(s, c, 4096) == rs.noise_key(s, c ^ 1, 0)            # step 4096 = the counter's bit 0
    assert rs.noise_key(s, (1 << 20) ^ c, k) == rs.noise_key(s ^ 1, c, k)   # counter bit 20 = the seed's bit 0


# ----------------------------------------------------------------------------- the oracle's streams
B = rs.OracleBackend


def test_oracle_standup_reset_pose(oracle_lib):
    L, _ = rs.scenario_pose(B, rs.standup_cfg(), SEED_ORACLE, "stand-up")
    L.check("oracle stand-up reset pose")


def test_oracle_standup_pose_accessor_matches_the_sim(oracle_lib):
    """su_reset_pose(seed, ctr) is the sim's construction (ctr 0) and first reset (ctr 1)."""
    cfg = rs.standup_cfg()
    b = B(cfg, 4096, SEED_ORACLE)
    for ctr in (0, 1):
        if ctr:
            b.reset()
        pos, quat = oracle_lib.su_reset_pose(cfg, seed=SEED_ORACLE, ctr=ctr, n=4096)
        st = b.state()
        np.testing.assert_array_equal(st[0:3].T, pos)
        np.testing.assert_array_equal(st[3:7].T, quat)


def test_oracle_v4_reset(oracle_lib):
    L, _ = rs.scenario_v4_reset(B, SEED_ORACLE)
    L.check("oracle v4 construction and reset")


def test_oracle_v4_interval_resample(oracle_lib):
    L, _ = rs.scenario_v4_interval(B, SEED_ORACLE)
    L.check("oracle v4 interval resample")


@pytest.mark.parametrize("rel_standing,pool", [(0.02, 16), (0.25, 2)])
def test_oracle_manager_reset(oracle_lib, rel_standing, pool):
    L, _ = rs.scenario_manager_reset(B, SEED_ORACLE, rel_standing, pool=pool)
    L.check(f"oracle manager construction and reset, rel_standing {rel_standing}")


@pytest.mark.parametrize("rel_standing", [0.02, 0.25])
def test_oracle_manager_resample_and_step_noise(oracle_lib, rel_standing):
    L, _ = rs.scenario_manager_step(B, SEED_ORACLE, rel_standing)
    L.check(f"oracle manager 10 s resample and step noise, rel_standing {rel_standing}")


def test_oracle_manager_reset_in_step(oracle_lib):
    L, _ = rs.scenario_manager_reset_in_step(B, SEED_ORACLE)
    L.check("oracle manager reset inside a step")


def test_oracle_manager_observe_noise(oracle_lib):
    L, _ = rs.scenario_manager_observe(B, SEED_ORACLE)
    L.check("oracle manager observe() noise")


def test_oracle_v2_full_reset_episode_length(oracle_lib):
    L, _ = rs.scenario_v2_full_reset(B, SEED_ORACLE)
    L.check("oracle v2 full-reset episode length")
