"""Empirical observation normalization on libzbot_ppo.so: the statistics kernels (zbp_norm_update)
against an f64 restatement of rsl_rl's rules, zbp_act / zbp_minibatch / a whole update with the
normalizers on against the torch policy holding the same modules, and the runner's wiring (eager
rollout, graph replay, checkpoint load).

The statistics' tolerance is measured: the kernel's error against the f64 restatement may be at most
4x the error of the fp32 torch module (``rl/normalizer.py``, on the same device and inputs) against
the same restatement, with one fp32 ulp of the statistic as the floor. The other tolerances are the
ones tests/test_gpu_ppo_fused.py holds the same kernels to without normalization."""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class F64Norm:
    """count += n; rate = n / count; delta = mean_x - mean; mean += rate delta; var += rate (var_x -
    var + delta (mean_x - new mean)); std = sqrt(var); frozen once count >= until. All f64."""

    def __init__(self, dim, until=None):
        self.mean, self.var, self.std = np.zeros(dim), np.ones(dim), np.ones(dim)
        self.count, self.until = 0, until

    def update(self, x):
        if self.until is not None and self.count >= self.until:
            return
        x = x.detach().double().cpu().numpy()
        n = x.shape[0]
        self.count += n
        rate = n / self.count
        mean_x, var_x = x.mean(axis=0), x.var(axis=0)  # (biased)
        delta = mean_x - self.mean
        self.mean = self.mean + rate * delta
        self.var = self.var + rate * (var_x - self.var + delta * (mean_x - self.mean))
        self.std = np.sqrt(self.var)


def _errors(nz, ref):
    """Max error of the mean, max relative error of the variance over the columns whose variance is
    not zero, max error of the variance over the constant columns (the simulator's observations have
    some: their exact variance is 0 and a relative error does not exist)."""
    m = nz._mean[0].double().cpu().numpy()
    v = nz._var[0].double().cpu().numpy()
    pos = ref.var > 0
    rel = float((np.abs(v - ref.var)[pos] / ref.var[pos]).max()) if pos.any() else 0.0
    return float(np.abs(m - ref.mean).max()), rel, float(np.abs(v)[~pos].max()) if (~pos).any() else 0.0


def _assert_stats(kernel_nz, torch_nz, ref, what):
    """The kernel's statistics within max(4 x the fp32 torch module's error, 1 ulp) of the f64 rules;
    the count exact; std = sqrt(var) of the kernel's own var to 1 ulp."""
    import torch
    km, kv, kz = _errors(kernel_nz, ref)
    tm, tv, tz = _errors(torch_nz, ref)
    pos = ref.var > 0
    ulp_m = float(np.spacing(np.abs(ref.mean).astype(np.float32)).max())
    ulp_v = float((np.spacing(ref.var.astype(np.float32))[pos] / ref.var[pos]).max()) if pos.any() else 0.0
    ulp_z = float(np.spacing(np.float32(0.0)))
    print(f"\n{what}: mean err kernel {km:.3g} torch {tm:.3g} (ulp {ulp_m:.3g}); "
          f"var rel err kernel {kv:.3g} torch {tv:.3g} (ulp {ulp_v:.3g}); "
          f"var of {int((~pos).sum())} constant columns kernel {kz:.3g} torch {tz:.3g}")
    assert int(kernel_nz.count) == ref.count, what
    assert km <= max(4.0 * tm, ulp_m), (what, km, tm, ulp_m)
    assert kv <= max(4.0 * tv, ulp_v), (what, kv, tv, ulp_v)
    assert kz <= max(4.0 * tz, ulp_z), (what, kz, tz, ulp_z)
    sq = torch.sqrt(kernel_nz._var)
    ulp_s = torch.nextafter(sq, torch.full_like(sq, float("inf"))) - sq
    assert ((kernel_nz._std - sq).abs() <= ulp_s).all(), what


def _norm_update(a, c, obs, cobs, scratch=None):
    """zbp_norm_update on the modules a / c (either may be None)."""
    import torch
    from zbot_lab_amd.rl import fused
    L = fused.lib()
    rows = obs.shape[0]
    if scratch is None:
        scratch = torch.zeros(int(L.zbp_norm_scratch_floats(rows)), device=obs.device)
    na = C.byref(fused.obs_norm(a)) if a is not None else None
    nc = C.byref(fused.obs_norm(c)) if c is not None else None
    fused._check(L.zbp_norm_update(na, nc, fused._p(obs), fused._p(cobs), rows, fused._p(scratch),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), "zbp_norm_update")
    return scratch


def _law(law, rows, dim, seed):
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    xs = [torch.randn(rows, dim, device="cuda:0", generator=g) for _ in range(6)]
    if law == "shifted":  # column mean 1000, std 0.01: E[x^2] - E[x]^2 in fp32 is off by > 1000x here
        xs = [1000.0 + 0.01 * x for x in xs]
    return xs


@pytest.mark.parametrize("law", ["normal", "shifted"])
@pytest.mark.parametrize("dim", [23, 32])
@pytest.mark.parametrize("rows", [40, 200, 4096, 16400])
def test_statistics_kernel_matches_f64(gpu, rows, dim, law):
    import torch
    from zbot_lab_amd.rl.normalizer import EmpiricalNormalization
    xs = _law(law, rows, dim, seed=rows + dim)
    runs = []
    for _ in range(2):
        k = EmpiricalNormalization(dim).cuda()
        ptrs = [b.data_ptr() for b in k.buffers()]
        scratch = None
        for x in xs:
            scratch = _norm_update(k, None, x, x, scratch)
        torch.cuda.synchronize()
        assert [b.data_ptr() for b in k.buffers()] == ptrs
        runs.append(k)
    t, ref = EmpiricalNormalization(dim).cuda(), F64Norm(dim)
    for x in xs:
        t.update(x)
        ref.update(x)
    _assert_stats(runs[0], t, ref, f"rows {rows} dim {dim} {law}")
    for key, v in runs[0].state_dict().items():  # the same sequence from the same state: the same bits
        assert torch.equal(v, runs[1].state_dict()[key]), key


def test_statistics_kernel_first_update_and_until(gpu):
    import torch
    from zbot_lab_amd.rl.normalizer import EmpiricalNormalization
    xs = _law("normal", 200, 23, seed=1)
    xs = [2.0 + 3.0 * x for x in xs]
    k, t, ref = EmpiricalNormalization(23, until=500).cuda(), EmpiricalNormalization(23, until=500).cuda(), F64Norm(23, 500)
    _norm_update(None, k, xs[0], xs[0])  # (the critic slot alone)
    t.update(xs[0])
    ref.update(xs[0])
    torch.cuda.synchronize()
    # from the initial state: the batch's own mean and biased variance
    np.testing.assert_allclose(ref.mean, xs[0].double().mean(0).cpu().numpy(), rtol=1e-12)
    np.testing.assert_allclose(ref.var, xs[0].double().var(0, unbiased=False).cpu().numpy(), rtol=1e-12)
    _assert_stats(k, t, ref, "first update")
    for x in xs[1:]:
        _norm_update(k, None, x, x)
        t.update(x)
        ref.update(x)
    torch.cuda.synchronize()
    assert ref.count == 600  # 200, 400, 600 >= 500: frozen from there
    _assert_stats(k, t, ref, "until")
    frozen = {key: v.clone() for key, v in k.state_dict().items()}
    _norm_update(k, None, xs[0] + 5.0, xs[0])
    torch.cuda.synchronize()
    for key, v in k.state_dict().items():
        assert torch.equal(v, frozen[key]), key


def test_statistics_kernel_two_normalizers(gpu):
    """Both normalizers in one call: on the same rows (one read) they end up identical; on different
    rows each follows its own input."""
    import torch
    from zbot_lab_amd.rl.normalizer import EmpiricalNormalization
    xs = _law("normal", 200, 23, seed=2)
    a, c = EmpiricalNormalization(23).cuda(), EmpiricalNormalization(23).cuda()
    a2, c2 = EmpiricalNormalization(23).cuda(), EmpiricalNormalization(23).cuda()
    ta, tc, ra, rc = EmpiricalNormalization(23).cuda(), EmpiricalNormalization(23).cuda(), F64Norm(23), F64Norm(23)
    for x in xs:
        y = 1.0 - 2.0 * x
        _norm_update(a, c, x, x)
        _norm_update(a2, c2, x, y)
        ta.update(x), tc.update(y), ra.update(x), rc.update(y)
    torch.cuda.synchronize()
    for key, v in a.state_dict().items():
        assert torch.equal(v, c.state_dict()[key]) and torch.equal(v, a2.state_dict()[key]), key
    _assert_stats(a2, ta, ra, "actor of two")
    _assert_stats(c2, tc, rc, "critic of two")


# ---------------------------------------------------------------------------- zbp_act / zbp_minibatch
def _alg(hidden, actor=True, critic=True, obs_dim=23, act=6, envs=512, steps=24, seed=0):
    """tests/test_gpu_ppo_fused.py's snapshot with the normalizers on and their statistics made
    non-trivial (several updates on data of mean 3, std 0.5, the law of the observations here)."""
    import torch
    from zbot_lab_amd.rl.ppo import PPO, ActorCritic
    torch.manual_seed(seed)
    pol = ActorCritic(obs_dim, obs_dim, act, actor_hidden_dims=hidden, critic_hidden_dims=hidden,
                      actor_obs_normalization=actor, critic_obs_normalization=critic)
    alg = PPO(pol, device="cuda:0")
    alg.init_storage(envs, steps, obs_dim, obs_dim, act)
    st = alg.storage
    g = torch.Generator(device="cuda:0").manual_seed(seed + 1)
    for _ in range(4):
        x = 3.0 + 0.5 * torch.randn(256, obs_dim, device="cuda:0", generator=g)
        pol.update_normalization(x, 0.9 * x)
    for t in (st.observations, st.critic_observations, st.actions, st.rewards, st.values, st.mu):
        t.copy_(torch.randn(t.shape, device="cuda:0", generator=g))
    st.observations.copy_(3.0 + 0.5 * st.observations)
    st.critic_observations.copy_(0.9 * st.observations + 0.05 * st.critic_observations)
    st.sigma.copy_(0.5 + torch.rand(st.sigma.shape, device="cuda:0", generator=g))
    st.dones.copy_((torch.rand(st.dones.shape, device="cuda:0", generator=g) < 0.05).float())
    with torch.no_grad():  # old log-probs near the current policy's, so ratios straddle the clip range
        pol.update_distribution(st.observations.flatten(0, 1))
        lp = pol.get_actions_log_prob(st.actions.flatten(0, 1)).view(steps, envs, 1)
        st.actions_log_prob.copy_(lp + 0.3 * torch.randn(lp.shape, device="cuda:0", generator=g))
        st.values.copy_(pol.evaluate(st.critic_observations.flatten(0, 1)).view(steps, envs, 1)
                        + 0.3 * torch.randn(st.values.shape, device="cuda:0", generator=g))
    st.step = steps
    alg.compute_returns(st.critic_observations[-1])
    st.step = steps
    alg.draw_minibatch_indices()
    return alg


def _act_env(rows, monkeypatch):
    if rows == "lds":
        monkeypatch.setenv("ZBP_ROWS", "lds")
        monkeypatch.setenv("ZBP_ACT", "lds")
    if rows in ("reg", "reg-small"):
        monkeypatch.setenv("ZBP_ACT", "reg")
    if rows == "split-small":
        monkeypatch.setenv("ZBP_ACT", "split")


def _check_act(alg, envs):
    """zbp_act on slot 3 against the torch policy (same modules, same noise); raw storage copies."""
    import torch
    from zbot_lab_amd.rl import fused
    fu = fused.FusedUpdate(alg, 256)
    st = alg.storage
    st.clear()
    g = torch.Generator(device="cuda:0").manual_seed(envs)
    obs = 3.0 + 0.5 * torch.randn(envs, 23, device="cuda:0", generator=g)
    cobs = 0.9 * obs + 0.05 * torch.randn(envs, 23, device="cuda:0", generator=g)
    st.step = 3
    fu.pack()
    a = fu.act(obs, cobs, st)
    noise = fu._noise.clone()
    pol = alg.policy
    with torch.no_grad():
        pol.update_distribution(obs)
        mu, sd = pol.action_mean, pol.action_std
        ref_a = mu + sd * noise
        ref_lp = pol.get_actions_log_prob(ref_a)
        ref_v = pol.evaluate(cobs)
    torch.cuda.synchronize()
    tol = lambda r: 1e-5 * max(1.0, float(r.abs().max()))  # noqa: E731
    assert (a - ref_a).abs().max() <= tol(ref_a)
    assert (st.actions[3] - ref_a).abs().max() <= tol(ref_a)
    assert (st.mu[3] - mu).abs().max() <= tol(mu)
    assert torch.equal(st.sigma[3], sd.expand_as(st.sigma[3]))
    assert (st.actions_log_prob[3].view(-1) - ref_lp).abs().max() <= tol(ref_lp)
    assert (st.values[3] - ref_v).abs().max() <= tol(ref_v)
    assert torch.equal(st.observations[3], obs) and torch.equal(st.critic_observations[3], cobs)
    return obs, cobs, mu, ref_v


ACT_ENVS = {"reg": (16400, 4096), "lds": (4096, 200), "reg-small": (200,), "split": (16400, 4096),
            "split-small": (200, 40)}
ACT_CASES = [([128, 128, 128], r) for r in ("reg", "lds", "reg-small", "split", "split-small")] + \
            [([256, 256, 128], r) for r in ("reg", "lds", "reg-small")]  # (k_act_split serves the 128-wide nets)


@pytest.mark.parametrize("hidden,rows", ACT_CASES, ids=[f"{h[0]}-{r}" for h, r in ACT_CASES])
def test_fused_act_with_normalizers_matches_torch_policy(gpu, hidden, rows, monkeypatch):
    _act_env(rows, monkeypatch)
    for envs in ACT_ENVS[rows]:
        alg = _alg(hidden, envs=envs, steps=4)
        assert int(alg.policy.actor_obs_normalizer.count) == 1024
        _check_act(alg, envs)


@pytest.mark.parametrize("which", ["actor", "critic"])
def test_fused_act_with_one_normalizer(gpu, which, monkeypatch):
    """Actor-only at 4096 rows (k_act_split), critic-only at 200 rows forced onto k_act_reg: a
    normalizer bound to the wrong net would show in the other net's output."""
    import torch
    hidden, rows, envs = (([128, 128, 128], "split", 4096) if which == "actor" else ([256, 256, 128], "reg-small", 200))
    _act_env(rows, monkeypatch)
    alg = _alg(hidden, actor=which == "actor", critic=which == "critic", envs=envs, steps=4)
    obs, cobs, mu, v = _check_act(alg, envs)
    pol = alg.policy
    with torch.no_grad():  # the normalized net does not see the raw input, the other one does
        raw_mu, raw_v = pol.actor(obs), pol.critic(cobs)
    if which == "actor":
        assert (raw_mu - mu).abs().max() > 1e-3 and torch.equal(raw_v, v)
    else:
        assert (raw_v - v).abs().max() > 1e-3 and torch.equal(raw_mu, mu)


def _torch_minibatch(alg, i):
    """update_steps' loss for minibatch i of the first epoch, backward into .grad (autograd through
    the normalizer modules)."""
    import torch
    gen = alg.storage.mini_batch_generator(alg.num_mini_batches, 1, alg.mb_indices)
    for k, mbt in enumerate(gen):
        if k == i:
            break
    obs_b, cobs_b, act_b, tv_b, adv_b, ret_b, old_lp_b, old_mu_b, old_sigma_b = mbt
    pol = alg.policy
    pol.update_distribution(obs_b)
    lp_b = pol.get_actions_log_prob(act_b)
    value_b = pol.evaluate(cobs_b)
    mu_b, sigma_b, entropy_b = pol.action_mean, pol.action_std, pol.entropy
    with torch.no_grad():
        kl = torch.sum(torch.log(sigma_b / old_sigma_b + 1e-5)
                       + (old_sigma_b.square() + (old_mu_b - mu_b).square()) / (2.0 * sigma_b.square()) - 0.5, dim=-1)
    ratio = torch.exp(lp_b - torch.squeeze(old_lp_b))
    s1 = -torch.squeeze(adv_b) * ratio
    s2 = -torch.squeeze(adv_b) * torch.clamp(ratio, 1.0 - alg.clip_param, 1.0 + alg.clip_param)
    surr = torch.max(s1, s2).mean()
    vc = tv_b + (value_b - tv_b).clamp(-alg.clip_param, alg.clip_param)
    vl = torch.max((value_b - ret_b).pow(2), (vc - ret_b).pow(2)).mean()
    loss = surr + alg.value_loss_coef * vl - alg.entropy_coef * entropy_b.mean()
    alg.optimizer.zero_grad(set_to_none=False)
    loss.backward()
    return torch.stack([kl.mean(), vl.detach(), surr.detach(), entropy_b.mean().detach()])


def _check_minibatch(alg, i, what):
    import torch
    from zbot_lab_amd.rl import fused
    mb = alg.storage.num_envs * alg.storage.num_transitions_per_env // alg.num_mini_batches
    assert fused.supported(alg.policy, mb)
    ref_stats = _torch_minibatch(alg, i)
    ref = [p.grad.detach().clone() for p in alg.policy.parameters()]
    f = fused.FusedUpdate(alg, mb)
    f.pack()
    stats = f.minibatch(alg.storage, alg.mb_indices, i * mb).clone()
    torch.cuda.synchronize()
    got = [p.grad.detach().clone() for p in alg.policy.parameters()]
    for (n, _), r, g in zip(alg.policy.named_parameters(), ref, got):
        scale = r.abs().max().item()
        err = (g - r).abs().max().item()
        assert err <= 1e-5 * scale + 1e-9, (what, n, err, scale)
    torch.testing.assert_close(stats, ref_stats, rtol=1e-5, atol=1e-7)
    return mb


@pytest.mark.parametrize("rows", ["reg", "lds"])
@pytest.mark.parametrize("hidden", [[128, 128, 128], [256, 256, 128]], ids=["v2-nets", "standup-nets"])
def test_fused_minibatch_with_normalizers_matches_autograd(gpu, hidden, rows, monkeypatch):
    if rows == "lds":
        monkeypatch.setenv("ZBP_ROWS", "lds")
    alg = _alg(hidden)
    _check_minibatch(alg, 3, (hidden, rows))


def test_fused_minibatch_with_normalizers_small_ragged_batch(gpu):
    for hidden in ([256, 256, 128], [128, 128, 128]):
        alg = _alg(hidden, envs=16)
        assert _check_minibatch(alg, 1, hidden) == 96


def test_fused_update_with_normalizers_matches_torch_update(gpu, monkeypatch):
    """A whole update (5 epochs x 4 minibatches) from one snapshot with both normalizers on, at
    test_fused_update_matches_torch_update's tolerances."""
    import torch
    alg_f = _alg([128, 128, 128], seed=3)
    alg_t = copy.deepcopy(alg_f)
    monkeypatch.setenv("ZBOT_PPO_FUSED", "0")
    alg_t.optimizer = torch.optim.Adam(alg_t.policy.parameters(), lr=alg_t.lr_t, fused=True, capturable=True)
    p0 = torch.cat([p.detach().flatten() for p in alg_t.policy.parameters()]).clone()
    alg_t.update_steps()
    monkeypatch.setenv("ZBOT_PPO_FUSED", "1")
    alg_f.update_steps()
    assert alg_f._fused is not None and alg_t._fused is None
    assert alg_f._fused.norm_a.mean and alg_f._fused.norm_c.mean
    torch.cuda.synchronize()
    pf = torch.cat([p.detach().flatten() for p in alg_f.policy.parameters()])
    pt = torch.cat([p.detach().flatten() for p in alg_t.policy.parameters()])
    moved = (pt - p0).abs()
    d = (pf - pt).abs()
    print(f"\nfused vs torch update (normalizers on): max |dp| {d.max().item():.3g} "
          f"(99.9% {d.quantile(0.999).item():.3g}), max move {moved.max().item():.3g}")
    assert moved.max() > 0
    assert d.quantile(0.999) <= 1e-3 * moved.max()
    assert d.max() <= 0.05 * moved.max()
    assert abs(float(alg_f.lr_t) - float(alg_t.lr_t)) <= 1e-7 + 1e-5 * float(alg_t.lr_t)
    torch.testing.assert_close(alg_f.update_sums, alg_t.update_sums, rtol=1e-4, atol=1e-6)
    # the update reads the statistics and leaves them alone
    for k, v in alg_f.policy.state_dict().items():
        if "normalizer" in k:
            assert torch.equal(v, alg_t.policy.state_dict()[k]), k


# ---------------------------------------------------------------------------- runner
def _runner(envs=64, **kw):
    import zbot_lab_amd
    from zbot_lab_amd.rl import OnPolicyRunner, PPORunnerCfgV2, RslRlVecEnvWrapper
    env_cfg = zbot_lab_amd.tasks.load_cfg("zbot-6b-walking-v2")
    env_cfg.scene.num_envs = envs
    agent = PPORunnerCfgV2()
    agent.policy.actor_obs_normalization = agent.policy.critic_obs_normalization = True
    env = RslRlVecEnvWrapper(zbot_lab_amd.make("zbot-6b-walking-v2", cfg=env_cfg))
    return env, OnPolicyRunner(env, agent.to_dict(), log_dir=None, device="cuda:0", **kw)


def test_runner_updates_statistics_eager_and_under_replay(gpu):
    """walking-v2, 64 envs: iteration 1 is the eager rollout plus the capture, iteration 2 a graph
    replay. After each, count grew by T N and the statistics are the f64 rules fed with the rollout's
    post-step observations in order: storage.observations[1:], then the returned last obs."""
    import torch
    from zbot_lab_amd.rl.normalizer import EmpiricalNormalization
    torch.manual_seed(0)
    env, r = _runner(use_graph=True, graph_update=True)
    pol = r.alg.policy
    T, N = r.num_steps_per_env, env.num_envs
    t, ref = EmpiricalNormalization(23).cuda(), F64Norm(23)
    for it in range(2):
        replay = r._graph is not None
        assert replay == (it == 1)
        r.learn(1)
        torch.cuda.synchronize()
        assert r._graph is not None and r.alg._fused is not None and r.alg.fused_rollout() is r.alg._fused
        st = r.alg.storage
        for x in list(st.observations[1:]) + [r._g_obs]:
            t.update(x)
            ref.update(x)
        assert ref.count == (it + 1) * T * N
        for nz in (pol.actor_obs_normalizer, pol.critic_obs_normalizer):
            _assert_stats(nz, t, ref, f"runner iteration {it}")
        assert torch.isfinite(torch.cat([p.detach().flatten() for p in pol.parameters()])).all()
    env.close()


def test_checkpoint_keeps_statistics_and_bound_pointers(gpu, tmp_path):
    import torch
    torch.manual_seed(1)
    env, a = _runner()
    a.learn(1)
    path = str(tmp_path / "model.pt")
    a.save(path)
    want = {k: v.clone() for k, v in a.alg.policy.state_dict().items()}
    env.close()
    assert int(want["actor_obs_normalizer.count"]) == a.num_steps_per_env * 64

    env, b = _runner()
    b.learn(1)  # the fused driver exists and holds the normalizers' pointers
    fu = b.alg._fused
    ptrs = (fu.norm_a.mean, fu.norm_a.std, fu.norm_c.mean, fu.norm_c.std, fu.norm_a.count)
    b.load(path, load_optimizer=False)
    assert b.alg._fused is fu
    pol = b.alg.policy
    for k, v in pol.state_dict().items():
        assert torch.equal(v, want[k]), k
    nz = pol.actor_obs_normalizer
    assert ptrs == (nz._mean.data_ptr(), nz._std.data_ptr(), pol.critic_obs_normalizer._mean.data_ptr(),
                    pol.critic_obs_normalizer._std.data_ptr(), nz.count.data_ptr())
    # zbp_act through the driver bound before the load sees the loaded statistics and parameters
    st = b.alg.storage
    st.clear()
    obs = b._g_obs.clone()
    act = fu.act(obs, obs, st)
    noise = fu._noise.clone()
    with torch.no_grad():
        pol.update_distribution(obs)
        ref_a = pol.action_mean + pol.action_std * noise
        ref_v = pol.evaluate(obs)
    torch.cuda.synchronize()
    tol = lambda r: 1e-5 * max(1.0, float(r.abs().max()))  # noqa: E731
    assert (act - ref_a).abs().max() <= tol(ref_a)
    assert (st.values[0] - ref_v).abs().max() <= tol(ref_v)
    assert torch.equal(st.observations[0], obs)
    st.clear()
    env.close()
