"""One PPO minibatch with rsl_rl's symmetry option, stated in fp64 torch with autograd: the reference the
torch path (tests/test_ppo_symmetry.py) and the kernels (tests/test_gpu_ppo_symmetry.py) are held to.
Built on ppo_options_reference.mlp and ppo_reference.normalize / log_prob; nothing here touches the
library, and the augmentation function is any callable with rsl_rl's signature
``(obs=None, actions=None, env=None) -> (obs_aug, actions_aug)``, originals first.

rsl_rl's PPO.update with ``symmetry`` set, per minibatch of B rows:

  use_data_augmentation   obs, actions = func(obs, actions): num_aug B rows; old log-prob, target values,
                          advantages and returns are repeated; the surrogate and the value loss are means
                          over all num_aug B rows; the KL statistic and the entropy over the first B rows
  mirror loss (always)    (without augmentation the observations alone are augmented first)
                          mean = actor(normalize(obs_aug)); _, target = func(None, mean[:B]);
                          symmetry = mse(mean[B:], target.detach()[B:]);
                          use_mirror_loss: loss += mirror_loss_coeff symmetry
"""
from __future__ import annotations

import torch

import ppo_options_reference as RO
import ppo_reference as R


def minibatch_reference(actor_w, actor_b, critic_w, critic_b, noise, rows, func, use_data_augmentation,
                        use_mirror_loss, mirror_loss_coeff, clip_param, value_loss_coef, entropy_coef,
                        use_clipped_value_loss, act="elu", std_type="scalar", actor_norm=None, critic_norm=None):
    """rows as ppo_reference.minibatch_reference takes them. Returns (grads, stats): grads = {actor_w,
    actor_b, critic_w, critic_b: lists, noise}, stats = {kl_mean, value_loss, surrogate, entropy,
    symmetry}."""
    f64 = R.f64
    aw = [f64(w).requires_grad_() for w in actor_w]
    ab = [f64(b).requires_grad_() for b in actor_b]
    cw = [f64(w).requires_grad_() for w in critic_w]
    cb = [f64(b).requires_grad_() for b in critic_b]
    p = f64(noise).requires_grad_()
    r = {k: f64(v) for k, v in rows.items()}
    col = lambda t: t.reshape(t.shape[0], 1)  # noqa: E731
    B = r["obs"].shape[0]
    obs, cobs, actions = r["obs"], r["critic_obs"], r["actions"]
    adv, ret, tv, old_lp = col(r["advantages"]), col(r["returns"]), col(r["values"]), col(r["log_prob"])
    if use_data_augmentation:
        aug, actions = func(obs={"policy": obs, "critic": cobs}, actions=actions)
        obs, cobs = aug["policy"], aug["critic"]
        n = obs.shape[0] // B
        adv, ret, tv, old_lp = adv.repeat(n, 1), ret.repeat(n, 1), tv.repeat(n, 1), old_lp.repeat(n, 1)
    adv, ret, tv, old_lp = adv.reshape(-1), ret.reshape(-1), tv.reshape(-1), old_lp.reshape(-1)
    c = float(clip_param)

    mu_all = RO.mlp(R.normalize(obs, actor_norm), aw, ab, act)
    value = RO.mlp(R.normalize(cobs, critic_norm), cw, cb, act).reshape(-1)
    sigma_all = mu_all * 0.0 + RO.sigma_of(p, std_type)
    lp = R.log_prob(actions, mu_all, sigma_all)
    mu, sigma = mu_all[:B], sigma_all[:B]
    entropy = (0.5 + R.LOG_SQRT_2PI + torch.log(sigma)).sum(-1)
    with torch.no_grad():
        kl = (torch.log(sigma / r["sigma"] + 1e-5)
              + (r["sigma"].square() + (r["mu"] - mu).square()) / (2.0 * sigma.square()) - 0.5).sum(-1)
    ratio = torch.exp(lp - old_lp)
    surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - c, 1.0 + c)).mean()
    if use_clipped_value_loss:
        vc = tv + (value - tv).clamp(-c, c)
        value_loss = torch.max((value - ret).square(), (vc - ret).square()).mean()
    else:
        value_loss = (ret - value).square().mean()
    loss = surrogate + float(value_loss_coef) * value_loss - float(entropy_coef) * entropy.mean()

    if not use_data_augmentation:
        obs = func(obs={"policy": obs, "critic": cobs}, actions=None)[0]["policy"]
    mean = RO.mlp(R.normalize(obs.detach(), actor_norm), aw, ab, act)
    _, target = func(obs=None, actions=mean[:B])
    symmetry = (mean[B:] - target.detach()[B:]).square().mean()
    if use_mirror_loss:
        loss = loss + float(mirror_loss_coeff) * symmetry

    leaves = aw + ab + cw + cb + [p]
    g = torch.autograd.grad(loss, leaves)
    na, nc = len(aw), len(cw)
    grads = {"actor_w": list(g[:na]), "actor_b": list(g[na:2 * na]), "critic_w": list(g[2 * na:2 * na + nc]),
             "critic_b": list(g[2 * na + nc:2 * na + 2 * nc]), "noise": g[-1]}
    stats = {"kl_mean": kl.mean().detach(), "value_loss": value_loss.detach(), "surrogate": surrogate.detach(),
             "entropy": entropy.mean().detach(), "symmetry": symmetry.detach()}
    return grads, stats
