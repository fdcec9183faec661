"""tests/ppo_reference.py (the fp64 statement the PPO kernels are held to in
tests/test_gpu_ppo_shapes.py) against the project's own torch code run in fp64 on the CPU:
PPO.update_steps' loss and gradients, ActorCritic's act, RolloutStorage.compute_returns,
PPO.process_env_step, and the rate rule + clip_grad_norm_ + torch.optim.Adam; to 1e-10 relative.
Also: the clamp sides of the GPU file's loss-branch cases (every side of every clamp and max holds
at least 10 % of the rows, for the committed seeds), and how far two deliberately wrong references
(s^2 for s^3 in the std gradient; a weight gradient without its last 32-column tile) move the
compared quantity, against the tolerance the GPU tests apply."""
from __future__ import annotations

import pytest
import torch

import ppo_cases as cases
import ppo_reference as R

RTOL = 1e-10


def _close(got, ref, what):
    got, ref = R.f64(got), R.f64(ref)
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    assert got.shape == ref.shape and err <= RTOL * max(scale, 1e-30), (what, err, scale)


def _double(alg):
    """The snapshot in fp64: policy (normalizer buffers included) and storage."""
    alg.policy.double()
    alg.update_sums = alg.update_sums.double()
    st = alg.storage
    for k, v in vars(st).items():
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(st, k, v.double())
    return alg


@pytest.mark.parametrize("clipped", [True, False], ids=["clipped-value", "plain-value"])
@pytest.mark.parametrize("name,normalizers", [("partial", False), ("partial", True), ("minimum", False),
                                              ("shallow", False), ("linear", False)])
def test_minibatch_reference_matches_update_steps(name, normalizers, clipped):
    """PPO.update_steps itself (torch path, fp64, one epoch of four minibatches at rate 0 so the
    parameters stay): the gradients it leaves are the last minibatch's, its loss sums the four
    minibatches', and the KL it hands to the rate rule each minibatch's."""
    alg = cases.make_alg("cpu", cases.SHAPES[name], 96, normalizers=normalizers, num_learning_epochs=1,
                         learning_rate=0.0, max_grad_norm=1e30, use_clipped_value_loss=clipped, **cases.LOSS)
    _double(alg)
    ref = [cases.reference_minibatch(alg, i) for i in range(alg.num_mini_batches)]
    kls = []
    alg._adapt_learning_rate = lambda kl: kls.append(float(kl))
    before = [p.detach().clone() for p in alg.policy.parameters()]
    alg.update_steps()
    for p, b in zip(alg.policy.parameters(), before):
        assert torch.equal(p, b)
    named, _, _ = ref[-1]
    assert set(named) == {n for n, _ in alg.policy.named_parameters()}
    for n, p in alg.policy.named_parameters():
        _close(p.grad, named[n], n)
    _close(torch.tensor(kls, dtype=torch.float64), torch.stack([r[1][0] for r in ref]), "kl")
    _close(alg.update_sums, torch.stack([r[1][1:] for r in ref]).sum(0), "loss sums")
    # the same through the tests' single-minibatch statement (the GPU file's fp32 comparison side)
    for i in (0, 2):
        stats = cases.torch_minibatch(alg, i)
        _close(stats, ref[i][1], f"stats of minibatch {i}")
        for n, p in alg.policy.named_parameters():
            _close(p.grad, ref[i][0][n], (i, n))


def test_std_gradient_closed_form_matches_autograd():
    alg = _double(cases.make_alg("cpu", cases.SHAPES["partial"], 96, **cases.LOSS))
    named, _, _ = cases.reference_minibatch(alg, 1)
    aw, ab, _, _, std = cases.net_tensors(alg.policy)
    g = R.std_gradient_closed_form(aw, ab, std, cases.gathered_rows(alg, 1), alg.clip_param, alg.entropy_coef)
    _close(g, named["std"], "std gradient")


@pytest.mark.parametrize("name,normalizers", [("partial", False), ("partial", True), ("minimum", False)])
def test_act_reference_matches_policy(name, normalizers):
    alg = _double(cases.make_alg("cpu", cases.SHAPES[name], 96, normalizers=normalizers))
    pol, sh = alg.policy, cases.SHAPES[name]
    g = torch.Generator().manual_seed(11)
    o_law, c_law = ((3.0, 0.5), (-2.0, 0.7)) if normalizers else ((0.0, 1.0), (0.0, 1.0))
    obs = o_law[0] + o_law[1] * torch.randn(33, sh["obs"], generator=g, dtype=torch.float64)
    cobs = c_law[0] + c_law[1] * torch.randn(33, sh["cobs"], generator=g, dtype=torch.float64)
    noise = torch.randn(33, sh["act"], generator=g, dtype=torch.float64)
    with torch.no_grad():
        pol.update_distribution(obs)
        mu, sd = pol.action_mean, pol.action_std
        a = mu + sd * noise
        lp, v = pol.get_actions_log_prob(a), pol.evaluate(cobs)
    na, nc = cases.norms(pol)
    ref = R.act_reference(*cases.net_tensors(pol), obs, cobs, noise, actor_norm=na, critic_norm=nc)
    for k, t in (("mu", mu), ("sigma", sd), ("actions", a), ("log_prob", lp), ("value", v)):
        _close(t, ref[k], k)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("steps,envs", [(1, 1), (3, 7), (24, 5)])
def test_gae_reference_matches_compute_returns(steps, envs, normalize):
    from zbot_lab_amd.rl.ppo import RolloutStorage
    if normalize and steps * envs < 2:
        return  # (the unbiased std of one element does not exist)
    st = RolloutStorage(envs, steps, 1, 1, 1, "cpu")
    g = torch.Generator().manual_seed(steps + envs)
    for k in ("rewards", "values", "dones", "returns", "advantages"):
        setattr(st, k, getattr(st, k).double())
    st.rewards.copy_(torch.randn(st.rewards.shape, generator=g))
    st.values.copy_(torch.randn(st.values.shape, generator=g))
    st.dones.copy_((torch.rand(st.dones.shape, generator=g) < 0.3).double())
    st.dones[-1, 0] = 1.0
    last = torch.randn(envs, 1, generator=g, dtype=torch.float64)
    st.compute_returns(last, 0.99, 0.95, normalize)
    ret, adv = R.gae_reference(st.rewards, st.dones, st.values, last, 0.99, 0.95, normalize)
    _close(st.returns.view(steps, envs), ret, "returns")
    _close(st.advantages.view(steps, envs), adv, "advantages")


@pytest.mark.parametrize("with_time_outs", [True, False])
def test_env_post_reference_matches_process_env_step(with_time_outs):
    """PPO.process_env_step's storage reward / done, and the runner's episode bookkeeping restated as
    tests/test_gpu_ppo_fused.py states it."""
    n, gamma = 37, 0.99
    alg = _double(cases.make_alg("cpu", cases.SHAPES["minimum"], (n, 4)))
    st = alg.storage
    st.clear()
    g = torch.Generator().manual_seed(3)
    dbl = dict(generator=g, dtype=torch.float64)
    rew, val = torch.randn(n, **dbl), torch.randn(n, 1, **dbl)
    dones = (torch.rand(n, generator=g) < 0.3).long()
    tout = (torch.rand(n, generator=g) < 0.5) & (dones > 0)
    cur_rew, cur_len, ep = torch.randn(n, **dbl), torch.randint(0, 100, (n,), generator=g).double(), torch.tensor(
        [1.0, 2.0, 3.0], dtype=torch.float64)
    z = torch.zeros(n, 1, dtype=torch.float64)
    alg._tr = dict(obs=z, critic_obs=z, actions=z, values=val, log_prob=z, mu=z, sigma=z)
    alg.process_env_step(rew, dones, {"time_outs": tout} if with_time_outs else {})
    ref = R.env_post_reference(rew, dones, tout if with_time_outs else None, val, gamma, cur_rew, cur_len, ep)
    _close(st.rewards[0].view(-1), ref["st_rewards"], "reward")
    _close(st.dones[0].view(-1), ref["st_dones"], "done")
    r_cur, r_len, d = cur_rew + rew, cur_len + 1, dones > 0
    r_ep = ep + torch.stack([torch.where(d, r_cur, 0.0).sum(), torch.where(d, r_len, 0.0).sum(), d.sum().double()])
    _close(r_cur.masked_fill(d, 0.0), ref["cur_rew"], "cur_rew")
    _close(r_len.masked_fill(d, 0.0), ref["cur_len"], "cur_len")
    _close(r_ep, ref["ep_stats"], "ep_stats")


@pytest.mark.parametrize("max_norm", [0.05, 1e3], ids=["clipping", "no-clipping"])
@pytest.mark.parametrize("kl,lr,want", [(0.05, 1e-5, 1e-5), (0.002, 1e-2, 1e-2), (0.01, 1e-3, 1e-3),
                                        (0.05, 1e-3, 1e-3 / 1.5), (0.002, 1e-3, 1.5e-3), (-0.001, 1e-3, 1e-3)])
def test_adam_reference_matches_torch(kl, lr, want, max_norm):
    """The rate rule (PPO._adapt_learning_rate), nn.utils.clip_grad_norm_ and torch.optim.Adam in fp64,
    from a mid-training state (step 7, non-zero moments)."""
    alg = _double(cases.make_alg("cpu", cases.SHAPES["shallow"], 96, learning_rate=lr, max_grad_norm=max_norm))
    cases.torch_minibatch(alg, 1)
    ps = list(alg.policy.parameters())
    g = torch.Generator().manual_seed(5)
    for p in ps:
        alg.optimizer.state[p] = {"step": torch.tensor(7.0), "exp_avg": 0.1 * torch.randn(p.shape, generator=g).double(),
                                  "exp_avg_sq": 0.01 * torch.rand(p.shape, generator=g).double()}
    st = alg.optimizer.state
    ref = R.adam_reference(ps, [p.grad for p in ps], [st[p]["exp_avg"] for p in ps], [st[p]["exp_avg_sq"] for p in ps],
                           7.0, lr, kl, alg.desired_kl, max_norm)
    alg.lr_t = torch.tensor(lr, dtype=torch.float64)
    alg._adapt_learning_rate(torch.tensor(kl, dtype=torch.float64))
    torch.nn.utils.clip_grad_norm_(alg.policy.parameters(), alg.max_grad_norm)
    alg.optimizer.step()
    assert (ref["coef"] < 1.0) == (max_norm < 1.0)
    assert abs(ref["lr"] - want) <= RTOL * want and abs(float(alg.lr_t) - want) <= RTOL * want
    for i, p in enumerate(ps):
        _close(p, ref["params"][i], f"param {i}")
        _close(p.grad, ref["grads"][i], f"grad {i}")
        _close(st[p]["exp_avg"], ref["exp_avg"][i], f"exp_avg {i}")
        _close(st[p]["exp_avg_sq"], ref["exp_avg_sq"][i], f"exp_avg_sq {i}")
        assert float(st[p]["step"]) == ref["step"] == 8.0


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("case", cases.LOSS_CASES, ids=[c[0] for c in cases.LOSS_CASES])
def test_loss_branch_cases_populate_every_clamp_side(case, clipped):
    """The data of the GPU file's loss-branch cases (same seeds, fp32 here as there): at least 10 % of
    the rows of the minibatch on each side of each clamp and of each max."""
    name, shape, rows = case
    for ec in (cases.LOSS["entropy_coef"], 0.0):
        kw = dict(cases.LOSS, entropy_coef=ec)
        alg = cases.make_alg("cpu", shape, rows, use_clipped_value_loss=clipped, **kw)
        _, _, sides = cases.reference_minibatch(alg, 1)
        cases.assert_sides(sides, clipped, (name, clipped, ec))


def _gpu_tolerance(ref):
    """The loosest bound tests/test_gpu_ppo_shapes.py ever applies to a tensor (the project cap)."""
    return 1e-5 * float(ref.abs().max()) + 1e-9


def test_wrong_references_move_far_beyond_the_tolerance():
    """A std gradient with s^2 where s^3 belongs, and a weight gradient without its last 32-column
    tile, differ from the reference by far more than the GPU tests' tolerance: a kernel with either
    defect cannot pass them."""
    alg = cases.make_alg("cpu", cases.SHAPES["partial"], 96, **cases.LOSS)
    named, _, _ = cases.reference_minibatch(alg, 1)
    aw, ab, _, _, std = cases.net_tensors(alg.policy)
    rows = cases.gathered_rows(alg, 1)
    wrong = R.std_gradient_closed_form(aw, ab, std, rows, alg.clip_param, alg.entropy_coef, exponent=2)
    d_std, tol_std = float((wrong - named["std"]).abs().max()), _gpu_tolerance(named["std"])
    w = named["actor.2.weight"]  # [96][160]: five 32-column tiles, the last one a k_wgrad block of its own
    assert tuple(w.shape) == (96, 160)
    dropped = w.clone()
    dropped[:, 128:] = 0.0
    d_w, tol_w = float((dropped - w).abs().max()), _gpu_tolerance(w)
    print(f"\nstd gradient with s^2 for s^3: moves {d_std:.3g}, tolerance {tol_std:.3g} ({d_std / tol_std:.3g} x); "
          f"actor.2.weight without its last tile: moves {d_w:.3g}, tolerance {tol_w:.3g} ({d_w / tol_w:.3g} x)")
    assert d_std > 1e3 * tol_std and d_w > 1e3 * tol_w
