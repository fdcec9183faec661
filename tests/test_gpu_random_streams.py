"""The laws of the counter-based random draws, on the device.

The scenarios of tests/random_streams.py (shared with the oracle tests, tests/test_random_laws.py) run
through ZbotSim: 65 536 envs for the reset- and observe-only ones (past the kOcc switch, every XCD),
16 384 where a step is needed, at most 3 steps, no rollouts. Each test also holds the device's
recovered draws of the first call to the oracle's on a spread sample of 1024 envs: bit-equal for
flags, signs and episode lengths, within the parity tests' tolerances for the continuous draws.

zbp_act's in-kernel action noise (an actor whose last layer is zero, std 1: actions == noise exactly,
16 384 rows x 6 actions): the standard normal law, independence across steps, packs and seeds,
repetition for an equal (seed, counter, step), the two ends of the key's step field, and the numpy
restatement of noise_at (uint64 hash, float64 Box-Muller) within 1e-4 absolute.

Measured on an MI355X: the statistics next to their thresholds are in DESIGN.md section 6 ("Random
streams"). The device against the numpy restatement: max |difference| 1.49e-6. The whole file (14 tests)
runs in 6.1 s, the slowest test in 0.5 s (the GPU suite before it: 142 s).

Seeds: fixed below before the first run. None had to be replaced.
"""
from __future__ import annotations

import numpy as np
import pytest

import random_streams as rs
from random_laws import Laws

pytestmark = pytest.mark.gpu

SEED_ENV = 42                   # rank 0's env seed (ranks run with 42 + rank)
NOISE_SEED = 1234567            # zbp_act noise_seed
ROWS, NA = rs.N_STEP, 6

D, O = rs.DeviceBackend, rs.OracleBackend


def _run(scenario, title, cfg, *args, **kw):
    L, dev = scenario(D, *args, **kw)
    L.check(f"device {title}")
    _, ora = scenario(O, *args, full=False, **kw)
    worst = rs.compare_draws({k: dev[k] for k in ora if k in dev}, ora, cfg)
    print(f"device / oracle {title}: largest continuous difference {worst:.3g}")


def test_standup_reset_pose(gpu):
    cfg = rs.standup_cfg()
    _run(lambda B, **kw: rs.scenario_pose(B, cfg, SEED_ENV, "stand-up", **kw), "stand-up reset pose", cfg)


def test_v4_reset(gpu):
    _run(rs.scenario_v4_reset, "v4 construction and reset", rs.v4_cfg(), SEED_ENV)


def test_v4_interval_resample(gpu):
    _run(rs.scenario_v4_interval, "v4 interval resample", rs.v4_cfg(), SEED_ENV)


@pytest.mark.parametrize("rel_standing,pool", [(0.02, 16), (0.25, 2)])
def test_manager_reset(gpu, rel_standing, pool):
    _run(rs.scenario_manager_reset, f"manager construction and reset, rel_standing {rel_standing}",
         rs.manager_cfg(rel_standing), SEED_ENV, rel_standing, pool=pool)


@pytest.mark.parametrize("rel_standing", [0.02, 0.25])
def test_manager_resample_and_step_noise(gpu, rel_standing):
    _run(rs.scenario_manager_step, f"manager 10 s resample and step noise, rel_standing {rel_standing}",
         rs.manager_cfg(rel_standing), SEED_ENV, rel_standing)


def test_manager_reset_in_step(gpu):
    _run(rs.scenario_manager_reset_in_step, "manager reset inside a step", rs.manager_cfg(0.25), SEED_ENV)


def test_manager_observe_noise(gpu):
    _run(rs.scenario_manager_observe, "manager observe() noise", rs.manager_cfg(0.25), SEED_ENV)


def test_v2_full_reset_episode_length(gpu):
    from zbot_lab_amd import model as zm
    _run(rs.scenario_v2_full_reset, "v2 full-reset episode length", zm.TaskCfg(), SEED_ENV)


# ----------------------------------------------------------------------------- zbp_act
class _Act:
    """zbp_act with the in-kernel draw on an actor whose last layer is zero and std = 1 (mu = 0 and
    sigma = 1 exactly, so the actions are the noise), called at a chosen (seed, step); ``packs`` counts
    the zbp_pack calls on the zeroed workspace, which is the draw counter."""

    def __init__(self):
        import torch
        from zbot_lab_amd.rl import fused
        from zbot_lab_amd.rl.ppo import PPO, ActorCritic
        self.torch, self.fused = torch, fused
        torch.manual_seed(0)
        pol = ActorCritic(23, 23, NA, actor_hidden_dims=[128, 128, 128], critic_hidden_dims=[128, 128, 128])
        self.alg = PPO(pol, device="cuda:0")
        with torch.no_grad():
            last = fused.mlp_layers(pol.actor)[-1]
            last.weight.zero_()
            last.bias.zero_()
            fused.noise_param(pol).fill_(1.0)
        self.fu = fused.FusedUpdate(self.alg, 256)
        z = lambda *s: torch.zeros(*s, device="cuda:0")  # noqa: E731
        self.obs = torch.randn(ROWS, 23, device="cuda:0")
        self.bufs = dict(actions=z(ROWS, NA), st_obs=z(ROWS, 23), st_critic_obs=z(ROWS, 23), st_actions=z(ROWS, NA),
                         st_values=z(ROWS, 1), st_log_prob=z(ROWS, 1), st_mu=z(ROWS, NA), st_sigma=z(ROWS, NA))
        self.packs = 0

    def pack(self):
        self.fu.pack()
        self.packs += 1

    def io(self, seed, step):
        io = self.fused.ActIO()
        io.obs = io.critic_obs = self.obs.data_ptr()
        io.noise = None
        for k, t in self.bufs.items():
            setattr(io, k, t.data_ptr())
        io.rows, io.obs_dim, io.critic_obs_dim, io.num_actions = ROWS, 23, 23, NA
        io.noise_step, io.noise_seed = step, seed
        io.actor_norm, io.critic_norm, io.log_std = self.fu.norm_a, self.fu.norm_c, self.fu.log_std
        return io

    def call(self, seed, step):
        import ctypes as C
        fu, f = self.fu, self.fused
        io = self.io(seed, step)
        return f.lib().zbp_act(C.byref(fu.na), C.byref(fu.nc), f._p(fu.noise), C.byref(io), f._p(fu.ws), fu.rows,
                               fu._stream())

    def draw(self, seed, step):
        assert self.call(seed, step) == 0, self.fused.lib().zbp_last_error()
        self.torch.cuda.synchronize()
        assert float(self.bufs["st_mu"].abs().max()) == 0.0 and float((self.bufs["st_sigma"] - 1.0).abs().max()) == 0.0
        assert self.torch.equal(self.bufs["actions"], self.bufs["st_actions"])
        return self.bufs["actions"].cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def draws(gpu):
    """Every zbp_act draw the tests below read, made once: counter 1 (steps 0, 3, 4, 4095, step 3 again,
    step 3 of the next seed), then after a second pack counter 2 (steps 0, 3)."""
    a = _Act()
    out = {"act": a}
    a.pack()
    for step in (0, 3, 4, 4095):
        out[(NOISE_SEED, 1, step)] = a.draw(NOISE_SEED, step)
    out["repeat"] = a.draw(NOISE_SEED, 3)
    out[(NOISE_SEED + 1, 1, 3)] = a.draw(NOISE_SEED + 1, 3)
    a.pack()
    for step in (0, 3):
        out[(NOISE_SEED, 2, step)] = a.draw(NOISE_SEED, step)
    return out


def test_act_noise_is_standard_normal(draws):
    L = Laws()
    rs.check_action_noise(L, "zbp_act noise", draws[(NOISE_SEED, 1, 3)])
    L.check("zbp_act in-kernel noise, 16 384 x 6")


def test_act_noise_independent_across_step_pack_and_seed(draws):
    z = draws[(NOISE_SEED, 1, 3)]
    L = Laws()
    L.fresh("steps k / k+1", z, draws[(NOISE_SEED, 1, 4)])
    L.fresh("before / after a pack", z, draws[(NOISE_SEED, 2, 3)])
    L.fresh("noise_seed s / s+1", z, draws[(NOISE_SEED + 1, 1, 3)])
    L.check("zbp_act noise across steps, packs, seeds")
    assert np.array_equal(z, draws["repeat"])   # equal (seed, counter, step): bit for bit


def test_act_noise_key_range_ends(draws):
    """Steps 0 and 4095 of one counter against step 0 of the next counter (one past the step field's
    end is where the two would meet), and step 4096 is refused."""
    L = Laws()
    nxt = draws[(NOISE_SEED, 2, 0)]
    L.fresh("counter c step 0 / counter c+1 step 0", draws[(NOISE_SEED, 1, 0)], nxt)
    L.fresh("counter c step 4095 / counter c+1 step 0", draws[(NOISE_SEED, 1, 4095)], nxt)
    L.fresh("counter c step 0 / step 4095", draws[(NOISE_SEED, 1, 0)], draws[(NOISE_SEED, 1, 4095)])
    L.check("zbp_act noise at the ends of the key's step field")
    a = draws["act"]
    assert a.call(NOISE_SEED, 4096) < 0 and b"noise_step" in a.fused.lib().zbp_last_error()


def test_act_noise_matches_the_numpy_restatement(draws):
    """uint64 hash and float64 Box-Muller against the kernel's fp32 logf / cosf: about 1e-5 at |z| <= 5.77;
    a wrong key or bit field is an O(1) difference. Bound: 1e-4 absolute."""
    worst = 0.0
    for (seed, counter, step) in [k for k in draws if isinstance(k, tuple)]:
        ref = rs.noise_at(seed, counter, step, ROWS, NA)
        worst = max(worst, float(np.abs(draws[(seed, counter, step)] - ref).max()))
    print(f"zbp_act noise against the numpy restatement: max |difference| {worst:.3g}")
    assert worst <= 1e-4
