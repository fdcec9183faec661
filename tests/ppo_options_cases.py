"""PPO snapshots for the activation / noise_std_type tests (tests/test_ppo_options.py on the CPU,
tests/test_gpu_ppo_options.py on the GPU): tests/ppo_cases.py's ``make_alg`` with an activation and a
noise type, the references taken from tests/ppo_options_reference.py, and one more condition on the
observations.

Kinked activations. relu, lrelu and selu have a derivative that jumps at 0. A hidden pre-activation
within fp32 rounding of 0 lets any fp32 code, torch's included, land on the other side of the kink and
then differ from fp64 by a whole unit's gradient: not a rounding error, and no error-quotient bound can
absorb it. So the builder redraws, from the CPU generator, every observation row (of the actor's and of
the critic's observations, through the normalizer statistics actually in use) that has a hidden
pre-activation of the fp64 forward within TAU = 1e-5 of 0, until none is left, and asserts that none
is left and that at most 5 % of the rows of either observation tensor were redrawn. It does so for
every activation, smooth ones included, so that one code path serves all. TAU is about 100 x the fp32
error of those pre-activations (|z| of order 1, dot products of up to 256 terms: a few 1e-7); with default-initialised
[128, 128, 128] nets 7 to 18 of a tensor's 768 rows are redrawn (<= 2.4 %), with [256, 256, 128] nets
up to 3 %."""
from __future__ import annotations

import torch

import ppo_cases as cases
import ppo_options_reference as RO
import ppo_reference as R

TAU = 1e-5
MAX_REDRAWN = 0.05


def noise_name(policy):
    return "log_std" if policy.noise_std_type == "log" else "std"


def noise_param(policy):
    return getattr(policy, noise_name(policy))


def near_kink_rows(x, weights, biases, norm, act):
    """Rows of x with a hidden pre-activation of the fp64 forward within TAU of 0."""
    pre = []
    RO.mlp(R.normalize(R.f64(x), norm), [R.f64(w) for w in weights], [R.f64(b) for b in biases], act, pre=pre)
    bad = torch.zeros(x.shape[0], dtype=torch.bool)
    for z in pre:
        bad |= (z.abs() <= TAU).any(dim=1)
    return bad


def redraw_near_kink(x, law, weights, biases, norm, act, g):
    """Redraw (law = (shift, scale) of a standard normal, CPU generator g) the rows of x [rows, dim]
    near a kink until none is left; returns the number of distinct rows redrawn."""
    redrawn = torch.zeros(x.shape[0], dtype=torch.bool)
    for _ in range(100):
        bad = near_kink_rows(x, weights, biases, norm, act)
        if not bad.any():
            break
        redrawn |= bad
        fresh = law[0] + law[1] * torch.randn(int(bad.sum()), x.shape[1], generator=g)
        x[bad.to(x.device)] = fresh.to(x.device)
    assert not near_kink_rows(x, weights, biases, norm, act).any()
    return int(redrawn.sum())


def make_alg(device, shape, rows, act="elu", std_type="scalar", seed=0, normalizers=False, **ppo_kw):
    """ppo_cases.make_alg with ``activation=act`` and ``noise_std_type=std_type``: a PPO object on
    `device` holding one filled rollout of 4 x `rows` transitions, sigma = linspace(0.3, 2.0) per action,
    no observation row near a kink (``alg.redrawn`` = ((actor rows, critic rows) redrawn, rows))."""
    from zbot_lab_amd.rl.ppo import PPO, ActorCritic
    envs, steps = cases.ROWS[rows] if rows in cases.ROWS else rows
    obs_dim, cobs_dim, na_ = shape["obs"], shape["cobs"], shape["act"]
    torch.manual_seed(seed)
    pol = ActorCritic(obs_dim, cobs_dim, na_, actor_hidden_dims=shape["actor"], critic_hidden_dims=shape["critic"],
                      activation=act, noise_std_type=std_type, actor_obs_normalization=normalizers,
                      critic_obs_normalization=normalizers)
    with torch.no_grad():
        sig = torch.linspace(0.3, 2.0, na_)  # (one action: 0.3)
        noise_param(pol).copy_(torch.log(sig) if std_type == "log" else sig)
    alg = PPO(pol, device=device, **ppo_kw)
    alg.init_storage(envs, steps, obs_dim, cobs_dim, na_)
    st = alg.storage
    g = torch.Generator().manual_seed(seed + 1)
    randn = lambda *s: torch.randn(*s, generator=g).to(device)  # noqa: E731
    rand = lambda *s: torch.rand(*s, generator=g).to(device)  # noqa: E731
    o_law, c_law = ((3.0, 0.5), (-2.0, 0.7)) if normalizers else ((0.0, 1.0), (0.0, 1.0))
    if normalizers:  # statistics of a shifted, scaled batch (the law of the observations below)
        for _ in range(4):
            pol.update_normalization(o_law[0] + o_law[1] * randn(256, obs_dim), c_law[0] + c_law[1] * randn(256, cobs_dim))
    st.observations.copy_(o_law[0] + o_law[1] * randn(*st.observations.shape))
    st.critic_observations.copy_(c_law[0] + c_law[1] * randn(*st.critic_observations.shape))
    aw, ab, cw, cb = net_tensors(pol)[:4]
    na, nc = cases.norms(pol)
    # the kink condition (module docstring), on the storage's flat row views
    n_rows = steps * envs
    red = (redraw_near_kink(st.observations.view(n_rows, obs_dim), o_law, aw, ab, na, act, g),
           redraw_near_kink(st.critic_observations.view(n_rows, cobs_dim), c_law, cw, cb, nc, act, g))
    assert max(red) <= MAX_REDRAWN * n_rows, (red, n_rows)
    alg.redrawn = (red, n_rows)
    for t in (st.rewards, st.mu):
        t.copy_(randn(*t.shape))
    st.sigma.copy_(0.5 + rand(*st.sigma.shape))  # distinct per row and per action
    st.dones.copy_((rand(*st.dones.shape) < 0.05).float())
    # actions around the fp64 policy mean with its sigma, old log-probs and values 0.3 off the current
    # ones so every clamp side occurs (ppo_cases.make_alg)
    with torch.no_grad():
        f64 = R.f64
        mu = RO.mlp(R.normalize(f64(st.observations.flatten(0, 1)), na), [f64(w) for w in aw], [f64(b) for b in ab], act)
        val = RO.mlp(R.normalize(f64(st.critic_observations.flatten(0, 1)), nc), [f64(w) for w in cw],
                     [f64(b) for b in cb], act)
        s64 = RO.sigma_of(f64(noise_param(pol)), std_type)
        st.actions.copy_((mu + s64 * torch.randn(mu.shape, generator=g, dtype=torch.float64)).view(st.actions.shape))
        lp = R.log_prob(f64(st.actions.flatten(0, 1)), mu, s64.expand_as(mu)).view(steps, envs, 1)
        st.actions_log_prob.copy_(lp + 0.3 * torch.randn(lp.shape, generator=g, dtype=torch.float64))
        st.values.copy_(val.view(steps, envs, 1) + 0.3 * torch.randn(lp.shape, generator=g, dtype=torch.float64))
    st.step = steps
    alg.compute_returns(st.critic_observations[-1])
    st.step = steps
    alg.mb_indices.copy_(torch.randperm(alg.mb_indices.numel(), generator=g).to(device))
    return alg


def net_tensors(policy):
    """(actor weights, actor biases, critic weights, critic biases, noise parameter) of an ActorCritic."""
    a, c = cases.linears(policy.actor), cases.linears(policy.critic)
    return ([m.weight for _, m in a], [m.bias for _, m in a], [m.weight for _, m in c], [m.bias for _, m in c],
            noise_param(policy))


def reference_minibatch(alg, i, act, std_type):
    """ppo_options_reference.minibatch_reference for minibatch i: ({parameter name: fp64 gradient} with
    the noise gradient under ``std`` or ``log_std``, stats [4] in the library's order, sides)."""
    pol = alg.policy
    aw, ab, cw, cb, noise = net_tensors(pol)
    na, nc = cases.norms(pol)
    grads, stats, sides = RO.minibatch_reference(aw, ab, cw, cb, noise, cases.gathered_rows(alg, i), alg.clip_param,
                                                 alg.value_loss_coef, alg.entropy_coef, alg.use_clipped_value_loss,
                                                 act=act, std_type=std_type, actor_norm=na, critic_norm=nc)
    named = {noise_name(pol): grads["noise"]}
    for net, seq in (("actor", pol.actor), ("critic", pol.critic)):
        for k, (idx, _) in enumerate(cases.linears(seq)):
            named[f"{net}.{idx}.weight"] = grads[f"{net}_w"][k]
            named[f"{net}.{idx}.bias"] = grads[f"{net}_b"][k]
    vec = torch.stack([stats["kl_mean"], stats["value_loss"], stats["surrogate"], stats["entropy"]])
    return named, vec, sides
