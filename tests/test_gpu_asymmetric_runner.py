"""Asymmetric actor-critic end to end: the env's "critic" observation group (cfg.critic_observations)
through RslRlVecEnvWrapper, OnPolicyRunner, the fused rollout, its graph replay and the torch path.
Walking v2 and the manager task, 64 envs, 8 steps per env, 2 minibatches.

A thin recording wrapper around the vec env copies the live critic buffer into a static [T, N, D] tensor
right before every env step (the copy is part of the captured rollout, so a graph replay records too):
storage.critic_observations[k] must be those rows bit for bit, and storage.values[k] the critic on them,
against torch fp64 within the rule of tests/test_gpu_ppo_shapes.py (its Check helper, imported).
"""
from __future__ import annotations

import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TASKS = {"zbot-6b-walking-v2": "PPORunnerCfgV2", "zbot-6b-walking-m-v0": "Zbot6BFlatPPORunnerCfg"}
T, N = 8, 64


class Recorder:
    """The vec env, plus rec[k] = the critic group as it stood before step k of the rollout."""

    def __init__(self, env, steps):
        self._env, self._steps, self.k, self.rec = env, steps, 0, None

    def __getattr__(self, name):
        return getattr(self._env, name)

    def step(self, actions):
        import torch
        c = self._env.get_observations()["critic"]
        if self.rec is None:
            self.rec = torch.zeros(self._steps, *c.shape, device=c.device)
        self.rec[self.k % self._steps].copy_(c)
        self.k += 1
        return self._env.step(actions)


def _runner(task, critic_obs=True, normalize=False, **kw):
    import zbot_lab_amd
    from zbot_lab_amd import rl
    from zbot_lab_amd.rl import cfg as rl_cfg
    env_cfg = zbot_lab_amd.tasks.load_cfg(task)
    env_cfg.scene.num_envs = N
    env_cfg.critic_observations = critic_obs
    agent = getattr(rl_cfg, TASKS[task])()
    agent.num_steps_per_env = T
    agent.algorithm.num_mini_batches = 2
    agent.policy.critic_obs_normalization = normalize
    env = Recorder(rl.RslRlVecEnvWrapper(zbot_lab_amd.make(task, cfg=env_cfg)), T)
    return env, rl.OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0", **kw)


def _in_features(seq):
    import torch
    return next(m for m in seq if isinstance(m, torch.nn.Linear)).in_features


def _check_storage(task, it, env, r, pol_before):
    import torch
    from test_gpu_ppo_shapes import Check
    st = r.alg.storage
    assert torch.equal(st.critic_observations.view(torch.int32), env.rec.view(torch.int32)), (task, it)
    ck = Check(f"asymmetric runner {task} iteration {it}: values")
    p64 = copy.deepcopy(pol_before).double()
    with torch.no_grad():
        rows = env.rec.reshape(T * N, -1)
        v32 = pol_before.evaluate(rows)
        v64 = p64.evaluate(rows.double())
    ck.close("values", st.values.reshape(T * N, 1), v32, v64)
    ck.done()


@pytest.mark.parametrize("task", list(TASKS))
def test_fused_rollout_and_graph_replay_read_the_env_critic_buffer(gpu, task):
    import torch
    torch.manual_seed(0)
    env, r = _runner(task, use_graph=True, graph_update=True)
    sim = env.unwrapped.sim
    pol = r.alg.policy
    D, P = sim.critic_obs_dim, sim.obs_dim
    assert _in_features(pol.critic) == D and _in_features(pol.actor) == P and D == P + 7
    assert r.alg.storage.critic_observations.shape == (T, N, D) and r.alg.storage.observations.shape == (T, N, P)
    spaces = env.unwrapped.single_observation_space
    assert spaces["critic"].shape == (D,) and spaces["policy"].shape == (P,) and env.unwrapped.state_space.shape == (N, D)
    live = env.unwrapped.get_observations()["critic"]
    assert live.data_ptr() == sim.critic_obs_buffer().data_ptr()
    for it in range(2):
        assert (r._graph is not None) == (it == 1)
        before, start = copy.deepcopy(pol), live.clone()
        r.learn(1)
        torch.cuda.synchronize()
        assert r.alg.fused_rollout() is not None and r._graph is not None
        assert env.k == T * (it + 1) + T * (it == 0)  # (Python ran for the eager rollout and the capture only)
        # the rollout started from the rows the previous one (or the reset) left in the env's buffer, and
        # left the buffer holding the current state's rows
        assert torch.equal(r.alg.storage.critic_observations[0], start), (task, it)
        assert torch.equal(live.view(torch.int32), sim.observe_critic().view(torch.int32))
        _check_storage(task, it, env, r, before)
        assert torch.isfinite(torch.cat([p.detach().flatten() for p in pol.parameters()])).all()
    env.close()


@pytest.mark.parametrize("task", list(TASKS))
def test_torch_path_runs_the_same_cfg(gpu, task, monkeypatch):
    import torch
    monkeypatch.setenv("ZBOT_PPO_FUSED", "0")
    torch.manual_seed(0)
    env, r = _runner(task, use_graph=False)
    D, P = env.unwrapped.sim.critic_obs_dim, env.unwrapped.sim.obs_dim
    before = copy.deepcopy(r.alg.policy)
    r.learn(1)
    torch.cuda.synchronize()
    assert r.alg.fused_rollout() is None
    st = r.alg.storage
    assert st.critic_observations.shape == (T, N, D) and st.observations.shape == (T, N, P)
    # the torch path stores the rows the critic saw, not the buffer the step overwrote meanwhile
    assert torch.equal(st.critic_observations.view(torch.int32), env.rec.view(torch.int32))
    with torch.no_grad():
        v = before.evaluate(env.rec.reshape(T * N, -1)).reshape(T, N, 1)
    assert torch.allclose(st.values, v, rtol=1e-5, atol=1e-6)
    assert np.isfinite(r.log[-1]["loss/value_function"])
    env.close()


def test_symmetric_runner_is_unchanged(gpu):
    """critic_observations off (the default): one group, no registered buffer, the critic on the policy rows."""
    import zbot_lab_amd
    from zbot_lab_amd import rl
    env = rl.RslRlVecEnvWrapper(zbot_lab_amd.make("zbot-6b-walking-v2", num_envs=N))
    assert set(env.get_observations().keys()) == {"policy"} and getattr(env.unwrapped.sim, "_critic", None) is None
    agent = rl.PPORunnerCfgV2()
    agent.num_steps_per_env = T
    r = rl.OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0", use_graph=False)
    assert _in_features(r.alg.policy.critic) == 23
    r.learn(1)
    assert r._critic is None
    env.close()


def test_critic_normalizer_follows_the_critic_rows(gpu):
    """critic_obs_normalization on: after the eager iteration and after the replayed one, the critic
    normalizer's count and statistics are the f64 rules fed with the rollout's post-step critic rows in
    order (storage.critic_observations[1:], then the buffer's final rows), width D, not the policy rows."""
    import torch
    from test_gpu_obs_normalization import F64Norm, _assert_stats
    from zbot_lab_amd.rl.normalizer import EmpiricalNormalization
    torch.manual_seed(0)
    task = "zbot-6b-walking-m-v0"
    env, r = _runner(task, normalize=True, use_graph=True, graph_update=True)
    sim = env.unwrapped.sim
    D = sim.critic_obs_dim
    nz = r.alg.policy.critic_obs_normalizer
    assert nz._mean.shape[-1] == D
    t, ref = EmpiricalNormalization(D).cuda(), F64Norm(D)
    for it in range(2):
        r.learn(1)
        torch.cuda.synchronize()
        for x in list(r.alg.storage.critic_observations[1:]) + [sim.critic_obs_buffer()]:
            t.update(x)
            ref.update(x)
        assert ref.count == (it + 1) * T * N
        _assert_stats(nz, t, ref, f"critic normalizer, iteration {it}")
    env.close()
