"""The PPO update, the rollout's policy step, GAE, the post-step bookkeeping and the fused optimizer
step stated once more in fp64 torch, from explicit tensors: the reference the kernels of
libzbot_ppo.so are held to (tests/test_gpu_ppo_shapes.py). Nothing here touches the library or its
binding; tests/test_ppo_reference.py checks every function against the project's own torch code
(PPO.update_steps, RolloutStorage.compute_returns, torch.optim.Adam) in fp64 on the CPU, so the
reference is checked by something other than the kernels.

Formulae (zbot_lab_amd/rl/ppo.py, rsl_rl semantics):
  log p(a)  = sum_a -(a - mu)^2 / (2 s^2) - log s - log sqrt(2 pi)
  entropy   = sum_a 1/2 + log sqrt(2 pi) + log s
  kl        = sum_a log(s / os + 1e-5) + (os^2 + (omu - mu)^2) / (2 s^2) - 1/2
  surrogate = mean max(-adv r, -adv clamp(r, 1 - c, 1 + c)),  r = exp(log p - old log p)
  value     = mean max((v - ret)^2, (tv + clamp(v - tv, -c, c) - ret)^2)   (clipped), mean (ret - v)^2
  loss      = surrogate + value_loss_coef value - entropy_coef mean entropy
"""
from __future__ import annotations

import math

import torch

F64 = torch.float64
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def f64(t):
    """A detached fp64 CPU copy (None stays None)."""
    return None if t is None else torch.as_tensor(t).detach().to("cpu", F64).clone()


def normalize(x, norm):
    """EmpiricalNormalization.forward: norm = (mean, std, eps) or None."""
    if norm is None:
        return x
    mean, std, eps = norm
    return (x - f64(mean).reshape(1, -1)) / (f64(std).reshape(1, -1) + float(eps))


def mlp(x, weights, biases):
    """Linear / ELU(alpha = 1) alternating, no activation after the last layer."""
    for l, (w, b) in enumerate(zip(weights, biases)):
        x = x @ w.t() + b
        if l < len(weights) - 1:
            x = torch.where(x > 0, x, torch.expm1(x))
    return x


def log_prob(actions, mu, std):
    return (-(actions - mu).square() / (2.0 * std.square()) - torch.log(std) - LOG_SQRT_2PI).sum(-1)


def minibatch_reference(actor_w, actor_b, critic_w, critic_b, std, rows, clip_param, value_loss_coef, entropy_coef,
                        use_clipped_value_loss, actor_norm=None, critic_norm=None):
    """One minibatch of PPO.update_steps. rows: the gathered minibatch rows, a dict of obs [B, D],
    critic_obs [B, Dc], actions / mu / sigma [B, A] and values / advantages / returns / log_prob [B]
    (or [B, 1]). Returns (grads, stats, sides): grads = {actor_w, actor_b, critic_w, critic_b: lists,
    std}, stats = {kl_mean, value_loss, surrogate, entropy}, sides = the fraction of rows on each side
    of each clamp and of each max (the tests require every side populated)."""
    aw = [f64(w).requires_grad_() for w in actor_w]
    ab = [f64(b).requires_grad_() for b in actor_b]
    cw = [f64(w).requires_grad_() for w in critic_w]
    cb = [f64(b).requires_grad_() for b in critic_b]
    s = f64(std).requires_grad_()
    r = {k: f64(v) for k, v in rows.items()}
    flat = lambda t: t.reshape(t.shape[0])  # noqa: E731
    adv, ret, tv, old_lp = flat(r["advantages"]), flat(r["returns"]), flat(r["values"]), flat(r["log_prob"])
    c = float(clip_param)

    mu = mlp(normalize(r["obs"], actor_norm), aw, ab)
    value = flat(mlp(normalize(r["critic_obs"], critic_norm), cw, cb))
    sigma = mu * 0.0 + s
    lp = log_prob(r["actions"], mu, sigma)
    entropy = (0.5 + LOG_SQRT_2PI + torch.log(sigma)).sum(-1)
    with torch.no_grad():
        kl = (torch.log(sigma / r["sigma"] + 1e-5)
              + (r["sigma"].square() + (r["mu"] - mu).square()) / (2.0 * sigma.square()) - 0.5).sum(-1)
    ratio = torch.exp(lp - old_lp)
    s1 = -adv * ratio
    s2 = -adv * torch.clamp(ratio, 1.0 - c, 1.0 + c)
    surrogate = torch.max(s1, s2).mean()
    sides = {"ratio_below": (ratio < 1.0 - c), "ratio_inside": ((ratio >= 1.0 - c) & (ratio <= 1.0 + c)),
             "ratio_above": (ratio > 1.0 + c), "surrogate_plain": (s1 > s2), "surrogate_clipped": (s2 > s1)}
    if use_clipped_value_loss:
        vd = value - tv
        vc = tv + vd.clamp(-c, c)
        ea, ec = (value - ret).square(), (vc - ret).square()
        value_loss = torch.max(ea, ec).mean()
        sides.update({"value_below": (vd < -c), "value_inside": ((vd >= -c) & (vd <= c)), "value_above": (vd > c),
                      "value_plain": (ea > ec), "value_clipped": (ec > ea)})
    else:
        value_loss = (ret - value).square().mean()
    loss = surrogate + float(value_loss_coef) * value_loss - float(entropy_coef) * entropy.mean()
    leaves = aw + ab + cw + cb + [s]
    g = torch.autograd.grad(loss, leaves)
    na, nc = len(aw), len(cw)
    grads = {"actor_w": list(g[:na]), "actor_b": list(g[na:2 * na]), "critic_w": list(g[2 * na:2 * na + nc]),
             "critic_b": list(g[2 * na + nc:2 * na + 2 * nc]), "std": g[-1]}
    stats = {"kl_mean": kl.mean().detach(), "value_loss": value_loss.detach(), "surrogate": surrogate.detach(),
             "entropy": entropy.mean().detach()}
    sides = {k: float(v.double().mean()) for k, v in sides.items()}
    return grads, stats, sides


def std_gradient_closed_form(actor_w, actor_b, std, rows, clip_param, entropy_coef, actor_norm=None, exponent=3):
    """d loss / d std written out (what the kernels compute): sum over the rows of
    g (diff^2 / s^exponent - 1 / s) with g = d surrogate / d log p, minus entropy_coef / s; exponent = 3
    is the gradient (tests/test_ppo_reference.py holds it to autograd's), any other value a deliberately
    wrong one for the sensitivity check."""
    with torch.no_grad():
        s = f64(std)
        r = {k: f64(v) for k, v in rows.items()}
        adv, old_lp = r["advantages"].reshape(-1), r["log_prob"].reshape(-1)
        c = float(clip_param)
        mu = mlp(normalize(r["obs"], actor_norm), [f64(w) for w in actor_w], [f64(b) for b in actor_b])
        diff = r["actions"] - mu
        ratio = torch.exp(log_prob(r["actions"], mu, s.expand_as(mu)) - old_lp)
        s1, s2 = -adv * ratio, -adv * torch.clamp(ratio, 1.0 - c, 1.0 + c)
        inside = ((ratio >= 1.0 - c) & (ratio <= 1.0 + c)).double()
        w1 = torch.where(s1 > s2, 1.0, torch.where(s1 < s2, 0.0, 0.5)).double()
        g = (w1 * -adv + (1.0 - w1) * -adv * inside) * ratio / adv.shape[0]
        return (g.unsqueeze(1) * (diff.square() / s.pow(exponent) - 1.0 / s)).sum(0) - float(entropy_coef) / s


def act_reference(actor_w, actor_b, critic_w, critic_b, std, obs, critic_obs, noise, actor_norm=None,
                  critic_norm=None):
    """PPO.act for a given standard-normal draw: {mu, sigma, actions, log_prob, value}."""
    with torch.no_grad():
        s = f64(std)
        mu = mlp(normalize(f64(obs), actor_norm), [f64(w) for w in actor_w], [f64(b) for b in actor_b])
        value = mlp(normalize(f64(critic_obs), critic_norm), [f64(w) for w in critic_w], [f64(b) for b in critic_b])
        sigma = s.expand_as(mu).clone()
        actions = mu + sigma * f64(noise)
        return {"mu": mu, "sigma": sigma, "actions": actions, "log_prob": log_prob(actions, mu, sigma), "value": value}


def gae_reference(rewards, dones, values, last_values, gamma, lam, normalize_advantage):
    """RolloutStorage.compute_returns: rewards / dones / values [T, N] (or [T, N, 1]), last_values [N]
    -> (returns, advantages) [T, N]; the advantages normalised by their mean and unbiased std + 1e-8."""
    rew, done, val = f64(rewards), f64(dones), f64(values)
    T, N = rew.shape[0], rew.shape[1]
    rew, done, val, last = rew.reshape(T, N), done.reshape(T, N), val.reshape(T, N), f64(last_values).reshape(N)
    ret = torch.zeros(T, N, dtype=F64)
    a = torch.zeros(N, dtype=F64)
    for k in reversed(range(T)):
        nxt = last if k == T - 1 else val[k + 1]
        nt = 1.0 - done[k]
        delta = rew[k] + nt * gamma * nxt - val[k]
        a = delta + nt * gamma * lam * a
        ret[k] = a + val[k]
    adv = ret - val
    if normalize_advantage:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    return ret, adv


def env_post_reference(rewards, dones, time_outs, values, gamma, cur_rew, cur_len, ep_stats):
    """PPO.process_env_step's reward (+ gamma V on time-outs; time_outs may be None) and done, and the
    runner's episode bookkeeping: {st_rewards, st_dones, cur_rew, cur_len, ep_stats}."""
    rew, val = f64(rewards).reshape(-1), f64(values).reshape(-1)
    d = torch.as_tensor(dones).detach().cpu().reshape(-1) > 0
    st_rew = rew.clone()
    if time_outs is not None:
        st_rew = st_rew + gamma * val * f64(time_outs).reshape(-1)
    cr, cl = f64(cur_rew) + rew, f64(cur_len) + 1.0
    ep = f64(ep_stats) + torch.stack([cr[d].sum(), cl[d].sum(), d.double().sum()])
    return {"st_rewards": st_rew, "st_dones": f64(dones).reshape(-1), "cur_rew": cr.masked_fill(d, 0.0),
            "cur_len": cl.masked_fill(d, 0.0), "ep_stats": ep}


def adaptive_lr(lr, kl, desired_kl):
    """rsl_rl's adaptive schedule: / 1.5 above 2 desired_kl, x 1.5 below half of it when kl > 0,
    within [1e-5, 1e-2]; desired_kl <= 0: off."""
    if desired_kl > 0.0:
        if kl > 2.0 * desired_kl:
            return max(lr / 1.5, 1e-5)
        if 0.0 < kl < desired_kl / 2.0:
            return min(lr * 1.5, 1e-2)
    return lr


def adam_reference(params, grads, exp_avg, exp_avg_sq, step, lr, kl, desired_kl, max_grad_norm, beta1=0.9,
                   beta2=0.999, eps=1e-8):
    """One zbp_optimizer_step (include/zbot_ppo.h): the rate rule on the minibatch KL, the gradients
    scaled by min(1, max_norm / (||g|| + 1e-6)) over all tensors, step += 1, torch's Adam with the NEW
    rate: m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
    p -= lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps). Lists of tensors in, a dict of lists
    (params, grads: the clipped ones left in .grad, exp_avg, exp_avg_sq) and step, lr, norm, coef out."""
    p, g = [f64(t) for t in params], [f64(t) for t in grads]
    m, v = [f64(t) for t in exp_avg], [f64(t) for t in exp_avg_sq]
    new_lr = adaptive_lr(float(lr), float(kl), float(desired_kl))
    norm = math.sqrt(sum(float(t.square().sum()) for t in g))
    coef = min(1.0, float(max_grad_norm) / (norm + 1e-6))
    t = float(step) + 1.0
    bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
    out = {"params": [], "grads": [], "exp_avg": [], "exp_avg_sq": [], "step": t, "lr": new_lr, "norm": norm,
           "coef": coef}
    for pi, gi, mi, vi in zip(p, g, m, v):
        gi = gi * coef
        mi = beta1 * mi + (1.0 - beta1) * gi
        vi = beta2 * vi + (1.0 - beta2) * gi * gi
        out["params"].append(pi - (new_lr / bc1) * mi / (vi.sqrt() / math.sqrt(bc2) + eps))
        out["grads"].append(gi)
        out["exp_avg"].append(mi)
        out["exp_avg_sq"].append(vi)
    return out
