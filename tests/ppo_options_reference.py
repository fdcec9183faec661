"""The PPO minibatch update and the rollout's policy step stated in fp64 torch once more, with the two
options tests/ppo_reference.py (ELU, std = sigma) does not have: the hidden layers' activation (rsl_rl's
elu / relu / tanh / selu / lrelu, torch's default constants) and the noise parameterisation (rsl_rl's
noise_std_type: "scalar", the parameter is sigma; "log", it is log sigma and sigma = exp(parameter)).
The reference the kernels of libzbot_ppo.so are held to in tests/test_gpu_ppo_options.py; nothing here
touches the library. tests/test_ppo_options.py checks it against PPO.update_steps and autograd in fp64
on the CPU, so it is checked by something other than the kernels.

Besides the autograd statement there is the backward pass written out the way the kernels compute it:
every activation's derivative from its OUTPUT x (the backward passes hold only the stored X_l)

    elu   x > 0 ? 1 : x + 1          relu  x > 0 ? 1 : 0          lrelu  x > 0 ? 1 : 0.01
    tanh  1 - x^2                    selu  x > 0 ? lambda : x + lambda alpha

and the noise gradient in closed form (dL / d log sigma = sigma dL / d sigma, the entropy bonus
contributing -entropy_coef per action), each with a deliberately wrong variant for the sensitivity
check."""
from __future__ import annotations

import torch

import ppo_reference as R

ACTIVATIONS = ("elu", "relu", "tanh", "selu", "lrelu")
STD_TYPES = ("scalar", "log")
SELU_SCALE, SELU_ALPHA = 1.0507009873554805, 1.6732632423543772
LRELU_SLOPE = 0.01


def activation(z, name):
    if name == "elu":
        return torch.where(z > 0, z, torch.expm1(z))
    if name == "relu":
        return torch.where(z > 0, z, torch.zeros_like(z))
    if name == "tanh":
        return torch.tanh(z)
    if name == "selu":
        return SELU_SCALE * torch.where(z > 0, z, SELU_ALPHA * torch.expm1(z))
    if name == "lrelu":
        return torch.where(z > 0, z, LRELU_SLOPE * z)
    raise ValueError(name)


def derivative_from_output(x, name, wrong=False):
    """act'(z) written from x = act(z). wrong: SELU's negative side as lambda, tanh's as 1 - x (the
    sensitivity check's deliberately wrong derivatives)."""
    one = torch.ones_like(x)
    if name == "elu":
        return torch.where(x > 0, one, x + 1.0)
    if name == "relu":
        return torch.where(x > 0, one, 0.0 * one)
    if name == "lrelu":
        return torch.where(x > 0, one, LRELU_SLOPE * one)
    if name == "tanh":
        return 1.0 - x if wrong else 1.0 - x * x
    if name == "selu":
        return torch.where(x > 0, SELU_SCALE * one, SELU_SCALE * one if wrong else x + SELU_SCALE * SELU_ALPHA)
    raise ValueError(name)


def mlp(x, weights, biases, act, pre=None):
    """Linear / activation alternating, no activation after the last layer. pre: a list that receives
    every hidden layer's pre-activation."""
    for l, (w, b) in enumerate(zip(weights, biases)):
        x = x @ w.t() + b
        if l < len(weights) - 1:
            if pre is not None:
                pre.append(x)
            x = activation(x, act)
    return x


def sigma_of(param, std_type):
    if std_type == "scalar":
        return param
    if std_type == "log":
        return torch.exp(param)
    raise ValueError(std_type)


def _losses(r, mu, value, sigma, c, use_clipped_value_loss):
    flat = lambda t: t.reshape(t.shape[0])  # noqa: E731
    adv, ret, tv, old_lp = flat(r["advantages"]), flat(r["returns"]), flat(r["values"]), flat(r["log_prob"])
    lp = R.log_prob(r["actions"], mu, sigma)
    entropy = (0.5 + R.LOG_SQRT_2PI + torch.log(sigma)).sum(-1)
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
    return surrogate, value_loss, entropy, kl, sides


def minibatch_reference(actor_w, actor_b, critic_w, critic_b, noise, rows, clip_param, value_loss_coef, entropy_coef,
                        use_clipped_value_loss, act="elu", std_type="scalar", actor_norm=None, critic_norm=None):
    """ppo_reference.minibatch_reference with the activation `act` and the noise parameter `noise` (sigma
    for "scalar", log sigma for "log"); the noise gradient comes back under grads["noise"]."""
    f64 = R.f64
    aw = [f64(w).requires_grad_() for w in actor_w]
    ab = [f64(b).requires_grad_() for b in actor_b]
    cw = [f64(w).requires_grad_() for w in critic_w]
    cb = [f64(b).requires_grad_() for b in critic_b]
    p = f64(noise).requires_grad_()
    r = {k: f64(v) for k, v in rows.items()}
    mu = mlp(R.normalize(r["obs"], actor_norm), aw, ab, act)
    value = mlp(R.normalize(r["critic_obs"], critic_norm), cw, cb, act)
    value = value.reshape(value.shape[0])
    sigma = mu * 0.0 + sigma_of(p, std_type)
    surrogate, value_loss, entropy, kl, sides = _losses(r, mu, value, sigma, float(clip_param), use_clipped_value_loss)
    loss = surrogate + float(value_loss_coef) * value_loss - float(entropy_coef) * entropy.mean()
    leaves = aw + ab + cw + cb + [p]
    g = torch.autograd.grad(loss, leaves)
    na, nc = len(aw), len(cw)
    grads = {"actor_w": list(g[:na]), "actor_b": list(g[na:2 * na]), "critic_w": list(g[2 * na:2 * na + nc]),
             "critic_b": list(g[2 * na + nc:2 * na + 2 * nc]), "noise": g[-1]}
    stats = {"kl_mean": kl.mean().detach(), "value_loss": value_loss.detach(), "surrogate": surrogate.detach(),
             "entropy": entropy.mean().detach()}
    return grads, stats, {k: float(v.double().mean()) for k, v in sides.items()}


def actor_backward_from_outputs(actor_w, actor_b, noise, rows, clip_param, act, std_type="scalar", actor_norm=None,
                                wrong=False):
    """The actor's weight and bias gradients of the surrogate the way the kernels compute them: dL / dmu
    at the output, then per layer dZ_{l-1} = (dZ_l W_l) * act'(X_l) with act' from the stored output X_l
    (derivative_from_output), dW_l = dZ_l^T X_l, db_l = sum dZ_l. Returns (weight grads, bias grads)."""
    f64 = R.f64
    with torch.no_grad():
        w, b = [f64(t) for t in actor_w], [f64(t) for t in actor_b]
        r = {k: f64(v) for k, v in rows.items()}
        xs = [R.normalize(r["obs"], actor_norm)]
        for l in range(len(w)):
            z = xs[-1] @ w[l].t() + b[l]
            xs.append(activation(z, act) if l < len(w) - 1 else z)
        mu = xs[-1]
        s = sigma_of(f64(noise), std_type).expand_as(mu)
        adv, old_lp = r["advantages"].reshape(-1), r["log_prob"].reshape(-1)
        c = float(clip_param)
        ratio = torch.exp(R.log_prob(r["actions"], mu, s) - old_lp)
        s1, s2 = -adv * ratio, -adv * torch.clamp(ratio, 1.0 - c, 1.0 + c)
        inside = ((ratio >= 1.0 - c) & (ratio <= 1.0 + c)).double()
        w1 = torch.where(s1 > s2, 1.0, torch.where(s1 < s2, 0.0, 0.5)).double()
        g = (w1 * -adv + (1.0 - w1) * -adv * inside) * ratio / adv.shape[0]  # dL / dlog_prob
        dz = g.unsqueeze(1) * (r["actions"] - mu) / s.square()
        gw, gb = [None] * len(w), [None] * len(w)
        for l in reversed(range(len(w))):
            gw[l], gb[l] = dz.t() @ xs[l], dz.sum(0)
            if l > 0:
                dz = (dz @ w[l]) * derivative_from_output(xs[l], act, wrong=wrong)
        return gw, gb


def noise_gradient_closed_form(actor_w, actor_b, noise, rows, clip_param, entropy_coef, act, std_type,
                               actor_norm=None, drop_sigma=False):
    """d loss / d noise parameter written out (what the kernels compute). "scalar": sum over the rows of
    g (diff^2 / s^3 - 1 / s), minus entropy_coef / s. "log": sigma times that sum, minus entropy_coef.
    drop_sigma: the log form without its factor sigma (the sensitivity check's wrong gradient)."""
    f64 = R.f64
    with torch.no_grad():
        s = sigma_of(f64(noise), std_type)
        r = {k: f64(v) for k, v in rows.items()}
        adv, old_lp = r["advantages"].reshape(-1), r["log_prob"].reshape(-1)
        c = float(clip_param)
        mu = mlp(R.normalize(r["obs"], actor_norm), [f64(w) for w in actor_w], [f64(b) for b in actor_b], act)
        diff = r["actions"] - mu
        ratio = torch.exp(R.log_prob(r["actions"], mu, s.expand_as(mu)) - old_lp)
        s1, s2 = -adv * ratio, -adv * torch.clamp(ratio, 1.0 - c, 1.0 + c)
        inside = ((ratio >= 1.0 - c) & (ratio <= 1.0 + c)).double()
        w1 = torch.where(s1 > s2, 1.0, torch.where(s1 < s2, 0.0, 0.5)).double()
        g = (w1 * -adv + (1.0 - w1) * -adv * inside) * ratio / adv.shape[0]
        d_sigma = (g.unsqueeze(1) * (diff.square() / s.pow(3) - 1.0 / s)).sum(0)
        if std_type == "scalar":
            return d_sigma - float(entropy_coef) / s
        return (d_sigma if drop_sigma else s * d_sigma) - float(entropy_coef)


def act_reference(actor_w, actor_b, critic_w, critic_b, noise_param, obs, critic_obs, noise, act="elu",
                  std_type="scalar", actor_norm=None, critic_norm=None):
    """PPO.act for a given standard-normal draw: {mu, sigma, actions, log_prob, value}."""
    f64 = R.f64
    with torch.no_grad():
        mu = mlp(R.normalize(f64(obs), actor_norm), [f64(w) for w in actor_w], [f64(b) for b in actor_b], act)
        value = mlp(R.normalize(f64(critic_obs), critic_norm), [f64(w) for w in critic_w], [f64(b) for b in critic_b],
                    act)
        sigma = sigma_of(f64(noise_param), std_type).expand_as(mu).clone()
        actions = mu + sigma * f64(noise)
        return {"mu": mu, "sigma": sigma, "actions": actions, "log_prob": R.log_prob(actions, mu, sigma), "value": value}
