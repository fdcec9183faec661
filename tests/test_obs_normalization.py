"""Empirical observation normalization (rsl_rl ``EmpiricalNormalization``, the policy cfg's
``actor_obs_normalization`` / ``critic_obs_normalization``) on the torch path: the module against an
f64 restatement of its rules, the checkpoint keys, the runner on the CPU stand-in env, the actor-only
/ critic-only arms and the TorchScript export."""
from __future__ import annotations

import warnings

import numpy as np
import pytest
import torch
import torch.nn as nn

from zbot_lab_amd.rl import OnPolicyRunner, PPORunnerCfgV2
from zbot_lab_amd.rl.normalizer import EmpiricalNormalization
from zbot_lab_amd.rl.ppo import ActorCritic

NORM_KEYS = {f"{m}.{k}" for m in ("actor_obs_normalizer", "critic_obs_normalizer")
             for k in ("_mean", "_var", "_std", "count")}


class F64Norm:
    """The rules in f64: count += n; rate = n / count; delta = mean_x - mean; mean += rate delta;
    var += rate (var_x - var + delta (mean_x - new mean)); std = sqrt(var); frozen once count >= until."""

    def __init__(self, dim, eps=1e-2, until=None):
        self.mean, self.var, self.std = np.zeros(dim), np.ones(dim), np.ones(dim)
        self.count, self.eps, self.until = 0, eps, until

    def update(self, x):
        if self.until is not None and self.count >= self.until:
            return
        x = np.asarray(x, dtype=np.float64)
        n = x.shape[0]
        self.count += n
        rate = n / self.count
        mean_x, var_x = x.mean(axis=0), x.var(axis=0)  # (numpy's var is the biased one)
        delta = mean_x - self.mean
        self.mean = self.mean + rate * delta
        self.var = self.var + rate * (var_x - self.var + delta * (mean_x - self.mean))
        self.std = np.sqrt(self.var)

    def forward(self, x):
        return (np.asarray(x, dtype=np.float64) - self.mean) / (self.std + self.eps)


class ToyVecEnv:
    """The stand-in env of tests/test_ppo.py: target reaching with time-outs, reward = -mean (action -
    target)^2, the target in the obs."""

    def __init__(self, n=64, obs_dim=23, act_dim=6, max_len=20, seed=0):
        self.num_envs, self.num_actions, self.max_episode_length = n, act_dim, max_len
        self.device = "cpu"
        self.g = torch.Generator().manual_seed(seed)
        self.obs_dim = obs_dim
        self.episode_length_buf = torch.zeros(n, dtype=torch.long)
        self.target = torch.rand(n, act_dim, generator=self.g) * 2 - 1

    def _obs(self):
        o = torch.zeros(self.num_envs, self.obs_dim)
        o[:, :self.num_actions] = self.target
        return {"policy": o}

    def get_observations(self):
        return self._obs()

    def step(self, a):
        rew = -(a - self.target).square().mean(dim=1)
        self.episode_length_buf += 1
        tout = self.episode_length_buf >= self.max_episode_length
        self.episode_length_buf[tout] = 0
        self.target[tout] = torch.rand(int(tout.sum()), self.num_actions, generator=self.g) * 2 - 1
        return self._obs(), rew, tout.long(), {"time_outs": tout, "log": {}}


def _batches(seed, k=6, rows=97, dim=23):
    g = torch.Generator().manual_seed(seed)
    scale = 0.2 + 3.0 * torch.rand(dim, generator=g)
    shift = 4.0 * torch.randn(dim, generator=g)
    return [shift + scale * torch.randn(rows + 5 * i, dim, generator=g) for i in range(k)]


def test_module_matches_f64_restatement():
    xs = _batches(0)
    m, ref = EmpiricalNormalization(23), F64Norm(23)
    assert m._mean.shape == m._var.shape == m._std.shape == (1, 23) and m.count.dtype == torch.int64
    assert m._mean.dtype == torch.float32 and float(m._mean.abs().max()) == 0.0
    assert torch.equal(m._var, torch.ones(1, 23)) and torch.equal(m._std, torch.ones(1, 23)) and int(m.count) == 0
    assert m.eps == 1e-2 and m.until is None
    ptrs = [b.data_ptr() for b in m.buffers()]
    for i, x in enumerate(xs):
        m.update(x)
        ref.update(x.numpy())
        if i == 0:  # from the initial state: exactly the batch's mean and biased variance
            np.testing.assert_allclose(m._mean[0].numpy(), x.double().mean(0).numpy(), rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(m._var[0].numpy(), x.double().var(0, unbiased=False).numpy(), rtol=1e-5)
        assert int(m.count) == ref.count
        np.testing.assert_allclose(m._mean[0].numpy(), ref.mean, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(m._var[0].numpy(), ref.var, rtol=1e-4)
        np.testing.assert_allclose(m._std[0].numpy(), ref.std, rtol=1e-4)
    assert [b.data_ptr() for b in m.buffers()] == ptrs
    # forward: (x - mean) / (std + eps), and it never touches the state
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m.train()
    y = m(xs[0])
    np.testing.assert_allclose(y.numpy(), ref.forward(xs[0].numpy()), rtol=1e-4, atol=1e-4)
    m.eval()
    m(xs[1])
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_until_freezes_the_statistics():
    xs = _batches(1, rows=100)  # 100, 105, 110, ... rows
    m, ref = EmpiricalNormalization(23, until=300), F64Norm(23, until=300)
    for x in xs:
        m.update(x)
        ref.update(x.numpy())
    # updates run while count < until: 100, 205, 315 -- then frozen
    assert int(m.count) == ref.count == 315
    np.testing.assert_allclose(m._mean[0].numpy(), ref.mean, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(m._var[0].numpy(), ref.var, rtol=1e-4)
    frozen = {k: v.clone() for k, v in m.state_dict().items()}
    m.update(xs[0] + 7.0)
    for k, v in m.state_dict().items():
        assert torch.equal(v, frozen[k]), k


def test_load_state_dict_keeps_the_buffers():
    a, b = EmpiricalNormalization(23), EmpiricalNormalization(23)
    for x in _batches(2, k=3):
        a.update(x)
    ptrs = [t.data_ptr() for t in b.buffers()]
    b.load_state_dict(a.state_dict())
    assert [t.data_ptr() for t in b.buffers()] == ptrs
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k


def test_state_dict_keys_and_flags_off_checkpoints():
    on = ActorCritic(23, 23, 6, actor_obs_normalization=True, critic_obs_normalization=True)
    off = ActorCritic(23, 23, 6)
    assert isinstance(off.actor_obs_normalizer, nn.Identity) and isinstance(off.critic_obs_normalizer, nn.Identity)
    assert set(on.state_dict()) - set(off.state_dict()) == NORM_KEYS
    assert not any("normalizer" in k for k in off.state_dict())
    # a checkpoint written without normalization has the keys of the nets and the std alone, and loads
    want = {"std"} | {f"{n}.{2 * l}.{p}" for n in ("actor", "critic") for l in range(4) for p in ("weight", "bias")}
    assert set(off.state_dict()) == want
    other = ActorCritic(23, 23, 6)
    other.load_state_dict({k: v.clone() for k, v in off.state_dict().items()})
    only_actor = ActorCritic(23, 23, 6, actor_obs_normalization=True)
    assert {k for k in only_actor.state_dict() if "normalizer" in k} == {k for k in NORM_KEYS if k.startswith("actor")}


def _cfg(steps=8, **policy):
    cfg = PPORunnerCfgV2()
    cfg.num_steps_per_env = steps
    cfg.device = "cpu"
    for k, v in policy.items():
        setattr(cfg.policy, k, v)
    return cfg


def test_runner_learns_with_actor_normalization_on_cpu():
    torch.manual_seed(0)
    env = ToyVecEnv()
    runner = OnPolicyRunner(env, _cfg(actor_obs_normalization=True).to_dict(), log_dir=None, device="cpu")
    pol = runner.alg.policy
    assert isinstance(pol.actor_obs_normalizer, EmpiricalNormalization)
    assert isinstance(pol.critic_obs_normalizer, nn.Identity)
    log = runner.learn(2)
    assert len(log) == 2
    for rec in log:
        assert all(np.isfinite(rec[k]) for k in ("loss/value_function", "loss/surrogate", "loss/entropy"))
    assert int(pol.actor_obs_normalizer.count) == 2 * 8 * env.num_envs
    # the inference policy normalizes
    obs = env.get_observations()["policy"]
    torch.testing.assert_close(runner.get_inference_policy()(obs), pol.actor(pol.actor_obs_normalizer(obs)))
    assert float(pol.actor_obs_normalizer._mean.abs().max()) > 0.0


def test_legacy_empirical_normalization_switches_both_on():
    torch.manual_seed(0)
    env = ToyVecEnv(n=16)
    cfg = _cfg(steps=4)
    cfg.empirical_normalization = True
    with pytest.warns(DeprecationWarning):
        runner = OnPolicyRunner(env, cfg.to_dict(), log_dir=None, device="cpu")
    pol = runner.alg.policy
    assert isinstance(pol.actor_obs_normalizer, EmpiricalNormalization)
    assert isinstance(pol.critic_obs_normalizer, EmpiricalNormalization)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        runner.learn(2)
    assert int(pol.actor_obs_normalizer.count) == int(pol.critic_obs_normalizer.count) == 2 * 4 * 16
    # both saw the same observations
    assert torch.equal(pol.actor_obs_normalizer._mean, pol.critic_obs_normalizer._mean)
    assert torch.equal(pol.actor_obs_normalizer._var, pol.critic_obs_normalizer._var)


def test_rollout_stores_raw_observations_and_updates_before_the_next_act():
    """The storage keeps raw observations, and the statistics after a rollout are the f64 rules fed
    with the post-step observations in order (the initial observation is not part of them)."""
    torch.manual_seed(0)
    env = ToyVecEnv(n=16)
    runner = OnPolicyRunner(env, _cfg(steps=6, actor_obs_normalization=True).to_dict(), log_dir=None, device="cpu")
    first = env.get_observations()["policy"].clone()
    with torch.no_grad():
        last = runner._rollout(first)
    st = runner.alg.storage
    assert torch.equal(st.observations[0], first)
    ref = F64Norm(23)
    for x in list(st.observations[1:]) + [last]:
        ref.update(x.numpy())
    nz = runner.alg.policy.actor_obs_normalizer
    assert int(nz.count) == ref.count == 6 * 16
    np.testing.assert_allclose(nz._mean[0].numpy(), ref.mean, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(nz._var[0].numpy(), ref.var, rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_one_normalizer_leaves_the_other_net_bit_identical(which):
    torch.manual_seed(3)
    off = ActorCritic(23, 23, 6)
    one = ActorCritic(23, 23, 6, **{f"{which}_obs_normalization": True})
    one.load_state_dict(off.state_dict(), strict=False)
    xs = _batches(4, k=3)
    for x in xs:
        one.update_normalization(x, x)
    obs = xs[0]
    with torch.no_grad():
        if which == "actor":
            assert torch.equal(one.evaluate(obs), off.evaluate(obs))
            assert not torch.equal(one.act_inference(obs), off.act_inference(obs))
            assert int(one.actor_obs_normalizer.count) == sum(x.shape[0] for x in xs)
            torch.testing.assert_close(one.act_inference(obs), off.actor(one.actor_obs_normalizer(obs)))
            one.update_distribution(obs)
            torch.testing.assert_close(one.action_mean, one.act_inference(obs))
        else:
            assert torch.equal(one.act_inference(obs), off.act_inference(obs))
            one.update_distribution(obs), off.update_distribution(obs)
            assert torch.equal(one.action_mean, off.action_mean)
            assert not torch.equal(one.evaluate(obs), off.evaluate(obs))
            assert int(one.critic_obs_normalizer.count) == sum(x.shape[0] for x in xs)
            torch.testing.assert_close(one.evaluate(obs), off.critic(one.critic_obs_normalizer(obs)))


def test_export_applies_the_normalizer(tmp_path):
    from zbot_lab_amd.rl import export_policy_as_jit
    torch.manual_seed(5)
    pol = ActorCritic(23, 23, 6, actor_obs_normalization=True)
    for x in _batches(6, k=3):
        pol.update_normalization(x)
    path = export_policy_as_jit(pol, normalizer=pol.actor_obs_normalizer, path=str(tmp_path), filename="policy.pt")
    mod = torch.jit.load(path)
    obs = _batches(7, k=1)[0]
    with torch.no_grad():
        ref = pol.actor(pol.actor_obs_normalizer(obs))
        assert not torch.allclose(ref, pol.actor(obs))
        torch.testing.assert_close(mod(obs), ref)
