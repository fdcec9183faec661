"""PPO snapshots for the fp64-reference tests (tests/test_ppo_reference.py on the CPU,
tests/test_gpu_ppo_shapes.py on the GPU): an ActorCritic of independent actor / critic depth, width
and observation dim with a distinct std per action, a filled rollout storage and a drawn
permutation, built as tests/test_gpu_ppo_fused.py's ``_alg`` does but with every random draw from a
CPU generator, so the same seeds give the same draws on either device and the clamp-side conditions
of the loss-branch cases can be checked without a GPU. The data agree between the devices up to fp32
rounding only: on a GPU the returns and advantages come from zbp_gae and the normalizer statistics
from the device's reductions, so the GPU tests assert the clamp sides again on their own data.

Unlike ``_alg``, actions are drawn around the policy mean with the policy's std (a rollout's law),
not as plain randn: with std = 0.3 and actions several std away the log-probability is in the tens,
the ratio carries its ulp (4e-6) and the torch fp32 statement itself misses the project's 1e-5 bound
on the std gradient (measured: e32 2.3e-05 against a cap of 3.4e-06 on the single-layer nets), so
the large |a - mu| / std regime cannot be held to that bound by any fp32 code and is left out."""
from __future__ import annotations

import torch
import torch.nn as nn

import ppo_reference as R

# the generic shape matrix: what the C ABI admits and the shipped configurations never run
SHAPES = {
    # partial k_wgrad blocks (5 = 4 + 1 and 7 = 4 + 3 tiles), depth 4 against 3, differing input dims
    "partial": dict(actor=[160, 96, 64], critic=[64, 224], obs=23, cobs=31, act=6),
    # every minimum: one-column input (31 padded), 32-wide hidden layer (tile_mma at kp = 32), one action
    "minimum": dict(actor=[32], critic=[32], obs=1, cobs=1, act=1),
    # every maximum: no input padding, 13 actions (the NSTAT - 3 bound), 24 k_wgrad groups
    "maximum": dict(actor=[256, 256, 256], critic=[256, 256, 256], obs=32, cobs=32, act=13),
    # the shipped widths as a mixed pair: no register kernel, one LDS layout for two strides
    "mixed": dict(actor=[128, 128, 128], critic=[256, 256, 128], obs=23, cobs=23, act=6),
    # 2- and 3-layer nets
    "shallow": dict(actor=[192], critic=[96, 160], obs=23, cobs=17, act=3),
    # n_layers == 1
    "linear": dict(actor=[], critic=[], obs=23, cobs=23, act=6),
}
V2 = dict(actor=[128, 128, 128], critic=[128, 128, 128], obs=23, cobs=23, act=6)
STANDUP = dict(actor=[256, 256, 128], critic=[256, 256, 128], obs=23, cobs=23, act=6)
# minibatch rows -> (envs, steps) with four minibatches
ROWS = {96: (16, 24), 160: (32, 20), 192: (32, 24), 1024: (256, 16), 2560: (512, 20)}
# the loss-branch constants: pairwise distinct, none a default
LOSS = dict(clip_param=0.13, value_loss_coef=0.7, entropy_coef=0.02)


def make_alg(device, shape, rows, seed=0, normalizers=False, **ppo_kw):
    """A PPO object on `device` holding one filled rollout of 4 x `rows` transitions."""
    from zbot_lab_amd.rl.ppo import PPO, ActorCritic
    envs, steps = ROWS[rows] if rows in ROWS else rows
    obs_dim, cobs_dim, act = shape["obs"], shape["cobs"], shape["act"]
    torch.manual_seed(seed)
    pol = ActorCritic(obs_dim, cobs_dim, act, actor_hidden_dims=shape["actor"], critic_hidden_dims=shape["critic"],
                      actor_obs_normalization=normalizers, critic_obs_normalization=normalizers)
    with torch.no_grad():
        pol.std.copy_(torch.linspace(0.3, 2.0, act))  # (one action: 0.3)
    alg = PPO(pol, device=device, **ppo_kw)
    alg.init_storage(envs, steps, obs_dim, cobs_dim, act)
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
    for t in (st.rewards, st.mu):
        t.copy_(randn(*t.shape))
    st.sigma.copy_(0.5 + rand(*st.sigma.shape))  # distinct per row and per action
    st.dones.copy_((rand(*st.dones.shape) < 0.05).float())
    # The rollout's actions, old log-probabilities and values from the fp64 statement of the current
    # policy: actions drawn around its mean with its std (as a rollout's are; with actions far from
    # the mean and std = 0.3 the log-probability is in the tens, the ratio carries its ulp and no fp32
    # statement of the std gradient is good to 1e-5), old log-probs and values 0.3 off the current
    # ones so every clamp side occurs. Not from the fp32 torch policy: its rounding would then be part
    # of the data and cancel in the torch side of every comparison, but not in the kernels'.
    aw, ab, cw, cb, std = net_tensors(pol)
    na, nc = norms(pol)
    with torch.no_grad():
        mu = R.mlp(R.normalize(R.f64(st.observations.flatten(0, 1)), na), [R.f64(w) for w in aw], [R.f64(b) for b in ab])
        val = R.mlp(R.normalize(R.f64(st.critic_observations.flatten(0, 1)), nc), [R.f64(w) for w in cw],
                    [R.f64(b) for b in cb])
        s64 = R.f64(std)
        st.actions.copy_((mu + s64 * torch.randn(mu.shape, generator=g, dtype=torch.float64)).view(st.actions.shape))
        lp = R.log_prob(R.f64(st.actions.flatten(0, 1)), mu, s64.expand_as(mu)).view(steps, envs, 1)
        st.actions_log_prob.copy_(lp + 0.3 * torch.randn(lp.shape, generator=g, dtype=torch.float64))
        st.values.copy_(val.view(steps, envs, 1) + 0.3 * torch.randn(lp.shape, generator=g, dtype=torch.float64))
    st.step = steps
    alg.compute_returns(st.critic_observations[-1])
    st.step = steps
    alg.mb_indices.copy_(torch.randperm(alg.mb_indices.numel(), generator=g).to(device))
    return alg


def linears(seq):
    return [(i, m) for i, m in enumerate(seq) if isinstance(m, nn.Linear)]


def net_tensors(policy):
    """(actor weights, actor biases, critic weights, critic biases, std) of an ActorCritic."""
    a, c = linears(policy.actor), linears(policy.critic)
    return ([m.weight for _, m in a], [m.bias for _, m in a], [m.weight for _, m in c], [m.bias for _, m in c],
            policy.std)


def norms(policy):
    """The (mean, std, eps) of the actor's / critic's normalizer, None for nn.Identity."""
    out = []
    for m in (policy.actor_obs_normalizer, policy.critic_obs_normalizer):
        out.append(None if isinstance(m, nn.Identity) else (m._mean, m._std, m.eps))
    return out


def gathered_rows(alg, i):
    """Minibatch i's rows through the permutation, as ppo_reference.minibatch_reference takes them."""
    st = alg.storage
    mb = st.num_envs * st.num_transitions_per_env // alg.num_mini_batches
    b = alg.mb_indices[i * mb:(i + 1) * mb]
    flat = lambda t: t.flatten(0, 1)[b]  # noqa: E731
    return dict(obs=flat(st.observations), critic_obs=flat(st.critic_observations), actions=flat(st.actions),
                values=flat(st.values), advantages=flat(st.advantages), returns=flat(st.returns),
                log_prob=flat(st.actions_log_prob), mu=flat(st.mu), sigma=flat(st.sigma))


def reference_minibatch(alg, i):
    """ppo_reference.minibatch_reference for minibatch i of `alg`: ({parameter name: fp64 gradient},
    stats [4] in the library's order (kl mean, value loss, surrogate, entropy), sides)."""
    pol = alg.policy
    aw, ab, cw, cb, std = net_tensors(pol)
    na, nc = norms(pol)
    grads, stats, sides = R.minibatch_reference(aw, ab, cw, cb, std, gathered_rows(alg, i), alg.clip_param,
                                                alg.value_loss_coef, alg.entropy_coef, alg.use_clipped_value_loss,
                                                actor_norm=na, critic_norm=nc)
    named = {"std": grads["std"]}
    for net, seq in (("actor", pol.actor), ("critic", pol.critic)):
        for k, (idx, _) in enumerate(linears(seq)):
            named[f"{net}.{idx}.weight"] = grads[f"{net}_w"][k]
            named[f"{net}.{idx}.bias"] = grads[f"{net}_b"][k]
    vec = torch.stack([stats["kl_mean"], stats["value_loss"], stats["surrogate"], stats["entropy"]])
    return named, vec, sides


def torch_minibatch(alg, i):
    """PPO.update_steps' loss for minibatch i of the first epoch in the policy's own precision,
    backward into .grad (autograd); returns the stats in the library's order."""
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
    if alg.use_clipped_value_loss:
        vc = tv_b + (value_b - tv_b).clamp(-alg.clip_param, alg.clip_param)
        vl = torch.max((value_b - ret_b).pow(2), (vc - ret_b).pow(2)).mean()
    else:
        vl = (ret_b - value_b).pow(2).mean()
    loss = surr + alg.value_loss_coef * vl - alg.entropy_coef * entropy_b.mean()
    alg.optimizer.zero_grad(set_to_none=False)
    loss.backward()
    pol.distribution = None
    return torch.stack([kl.mean(), vl.detach(), surr.detach(), entropy_b.mean().detach()])


# the loss-branch cases of tests/test_gpu_ppo_shapes.py: (name, shape, minibatch rows); minibatch 1 of
# seed 0 in every one (tests/test_ppo_reference.py checks their clamp sides on the CPU)
LOSS_CASES = [("v2", V2, 192), ("partial", SHAPES["partial"], 96)]
MIN_SIDE = 0.10


def assert_sides(sides, clipped, what):
    """At least 10 % of the minibatch's rows on each side of the surrogate's clamp and max and, with the
    clipped value loss, of the value's."""
    keys = ["ratio_below", "ratio_inside", "ratio_above", "surrogate_plain", "surrogate_clipped"]
    if clipped:
        keys += ["value_below", "value_inside", "value_above", "value_plain", "value_clipped"]
    for k in keys:
        assert sides[k] >= MIN_SIDE, (what, k, sides)
