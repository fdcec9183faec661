"""libzbot_ppo.so across the space its C ABI admits, against the fp64 statement of the same
operations (tests/ppo_reference.py, itself held to the project's torch code in
tests/test_ppo_reference.py): a distinct std per action on the shipped kernels (k_rows_reg, k_rows,
k_act_reg, k_act, k_act_split), the generic shape matrix (tests/ppo_cases.py SHAPES: partial k_wgrad
blocks, minimum and maximum dims, nets of 1 to 4 layers, actor and critic of different depth, width
and observation dim), both value-loss branches with non-default loss constants, zbp_optimizer_step
on its own in every branch of the rate rule, and the tails of zbp_gae and zbp_env_post. Minibatch 1
of the permutation throughout (a non-zero row offset), and every buffer a kernel has to write is
filled with NaN before the launch.

Tolerance. Every assertion is against fp64. For each compared tensor x the same test also takes the
error of the project's torch fp32 statement on the GPU, e32 = max |x32 - x64|, and requires of the
kernel's err = max |x - x64|

    err <= max(M e32, 2 eps32 max |x64|)   and   err <= 1e-5 max |x64| + 1e-9

with M = 4 (one tensor has a measured exception, see M_MEASURED): both sides are fp32 dot products
of one length in different summation orders (tiled MFMA, row splits), so their rounding errors are
of one size; the floor covers tensors torch happens to round exactly; the second bound is the one
tests/test_gpu_ppo_fused.py applies.

What each bound applies to. The second bound (the project's) holds for every parameter's gradient
as a tensor of its own, one-element ones included, and for each of the four statistics on its own
magnitude (1e-5 |x64| + 1e-7, the existing suite's rtol / atol). The first bound (the quotient)
holds per parameter, except that single numbers are grouped for it: the four statistics (and acc,
the three loss sums) as the tensor the library returns, a one-element gradient with its output
layer's weight gradient, a field of zbp_act over the case's launches. For a single number the
quotient of two rounding errors of one size has no typical value (a quarter of such quotients
exceed 2.4; one measured 26, see _minibatch), while over a tensor's maximum it concentrates near 1.
The fused optimizer takes its betas and eps through the C ABI as fp32, so the reference Adam runs
with those rounded values.

Measured on an MI355X, worst err / e32 per test over the tensors whose error is above the floor
(every run prints the same lines, pytest -s); the whole file takes 7 s:

    per-action std, zbp_minibatch   [128,128,128] k_rows_reg 2.11, k_rows 5.33 (actor.6.bias, see M_MEASURED);
                                    [256,256,128] k_rows_reg 2.41, k_rows 1.57
    per-action std, zbp_act         [128,128,128] reg 1.04, lds 1.03, split 1.04;
                                    [256,256,128] reg 1.17, lds 0.83, split (-> k_act_reg) 1.17
    matrix, zbp_minibatch           partial 3.23, minimum 3.70, maximum 2.47, mixed 1.34, shallow 1.43,
                                    single-layer nets 1.78, partial with normalizers 2.07
    matrix, zbp_act                 partial 1.52, minimum at the floor, maximum 1.25, mixed 1.01, shallow 0.99
    loss branches                   [128,128,128] k_rows_reg 1.38, k_rows 2.22; partial 1.34 (clipped), 1.25 (plain)
    zbp_optimizer_step              all 3168 tensors at the floor
    zbp_gae                         24 x 257: 1.00 (returns bit-equal to torch's); the others at the floor
    zbp_env_post                    5000 envs all done 1.47, some done 0.48 (the sum of returns); the others at the floor
"""
from __future__ import annotations

import copy

import numpy as np
import pytest

import ppo_cases as cases
import ppo_reference as R

pytestmark = pytest.mark.gpu

M = 4.0
# The one tensor M = 4 does not hold for, with its measured quotient (the issue allows up to 8 with
# the figure written next to it): the six-element actor.6.bias of the [128, 128, 128] nets on k_rows at
# 192 rows, err 1.26e-07 against torch's 2.37e-08 = 5.33, 6.6e-07 of its size. That is the error of a
# 192-term fp32 sum in lane order (k_wgrad's bias column), torch's tree sum being on the lucky side; the
# same gradient from k_rows_reg measures 2.41. Every other tensor keeps M = 4.
M_MEASURED = {("per-action std minibatch [128, 128, 128] lds", "192:actor.6.bias"): 8.0}
EPS32 = float(np.finfo(np.float32).eps)


class Check:
    """Collects every comparison of one test; `done` prints the worst quotient and asserts.
    `cap`: err <= 1e-5 max |x64| + atol, the project's existing bound, on a tensor of its own.
    `quotient`: err <= max(M e32, 2 eps32 max |x64|). `close`: both on the same tensor."""

    def __init__(self, what):
        self.what, self.rows, self.fails = what, [], []

    @staticmethod
    def _flat(*ts):
        out = [R.f64(t).reshape(-1) for t in ts]
        assert len({tuple(t.shape) for t in out}) == 1, [t.shape for t in out]
        return out

    def cap(self, name, got, ref64, atol=1e-9):
        got, ref = self._flat(got, ref64)
        err, cap = float((got - ref).abs().max()), 1e-5 * float(ref.abs().max()) + atol
        if not err <= cap:  # (NaN fails)
            self.fails.append((name, f"err {err:.3g}", f"cap {cap:.3g}"))

    def quotient(self, name, got, t32, ref64):
        got, t32, ref = self._flat(got, t32, ref64)
        err, e32 = float((got - ref).abs().max()), float((t32 - ref).abs().max())
        floor = 2.0 * EPS32 * float(ref.abs().max())
        bound = max(M_MEASURED.get((self.what, name), M) * e32, floor)
        self.rows.append((name, err, e32, floor))
        if not err <= bound:
            self.fails.append((name, f"err {err:.3g}", f"e32 {e32:.3g}", f"bound {bound:.3g}"))

    def close(self, name, got, t32, ref64, atol=1e-9):
        self.cap(name, got, ref64, atol)
        self.quotient(name, got, t32, ref64)

    def exact(self, name, got, want):
        import torch
        if not torch.equal(got, want):
            self.fails.append((name, "not bit-equal", float((got.double() - want.double()).abs().max())))

    def done(self):
        above = [(e / e32 if e32 > 0 else float("inf"), n, e, e32) for n, e, e32, fl in self.rows if e > fl]
        if above:
            q, n, e, e32 = max(above)
            print(f"\n[ratio] {self.what}: worst err / e32 {q:.2f} ({n}: err {e:.3g}, e32 {e32:.3g}); "
                  f"{len(self.rows) - len(above)} of {len(self.rows)} tensors at the floor")
        else:
            print(f"\n[ratio] {self.what}: floor (all {len(self.rows)} tensors within 2 eps32)")
        assert not self.fails, (self.what, self.fails)


def _poison(*tensors):
    for t in tensors:
        t.fill_(float("nan"))


def _minibatch(alg, ck, i=1, sides_clipped=None):
    """zbp_minibatch on minibatch i against the fp64 reference: every gradient and the statistics."""
    import torch
    from zbot_lab_amd.rl import fused
    pol = alg.policy
    mb = alg.storage.num_envs * alg.storage.num_transitions_per_env // alg.num_mini_batches
    assert fused.supported(pol, mb)
    ref, ref_stats, sides = cases.reference_minibatch(alg, i)
    if sides_clipped is not None:
        cases.assert_sides(sides, sides_clipped, ck.what)
    stats32 = cases.torch_minibatch(alg, i).clone()
    g32 = {n: p.grad.detach().clone() for n, p in pol.named_parameters()}
    f = fused.FusedUpdate(alg, mb)
    _poison(*[p.grad for p in pol.parameters()], f.stats)
    f.pack()
    stats = f.minibatch(alg.storage, alg.mb_indices, i * mb).clone()
    torch.cuda.synchronize()
    assert set(ref) == set(g32)
    # The project cap on every parameter's gradient as a tensor of its own, one-element ones (the
    # critic's output bias; with one action the std and the actor's output bias) included. The
    # quotient too, except that a one-element gradient joins its output layer's weight gradient for
    # it (the same dZ reduced with X): a single cancelling sum has no typical quotient and no
    # attainable 2 eps32 floor. Measured alone, the 96-row critic.4.bias of "partial": err 2.15e-08 =
    # 2.5 eps32 |x| against torch's 8.3e-10 = 0.1 eps32 |x|, a quotient of 26 between two sound sums.
    groups = {}
    for n, p in pol.named_parameters():
        ck.cap(f"{mb}:{n}", p.grad, ref[n])
        if p.numel() > 1:
            groups[n] = [[R.f64(x).reshape(-1) for x in (p.grad, g32[n], ref[n])]]
    for n, p in pol.named_parameters():
        if p.numel() == 1:
            host = n.replace("bias", "weight") if n != "std" else f"actor.{cases.linears(pol.actor)[-1][0]}.weight"
            groups[host].append([R.f64(x).reshape(-1) for x in (p.grad, g32[n], ref[n])])
    for n, parts in groups.items():
        ck.quotient(f"{mb}:{n}", *[torch.cat([q[j] for q in parts]) for j in range(3)])
    # the statistics: each one to the existing suite's bound on its own magnitude (rtol 1e-5, atol
    # 1e-7); the quotient on the four as the one tensor the library returns (single numbers, as above)
    for k, nm in enumerate(("kl mean", "value loss", "surrogate", "entropy")):
        ck.cap(f"{mb}:stats {nm}", stats[k], ref_stats[k], atol=1e-7)
    ck.quotient(f"{mb}:stats", stats, stats32, ref_stats)
    q = (stats.double().cpu() - ref_stats).abs() / (stats32.double().cpu() - ref_stats).abs().clamp_min(1e-300)
    print(f"\n[stats] {ck.what} {mb} rows: per-statistic err / e32 (kl, value, surrogate, entropy) "
          f"{[round(float(x), 2) for x in q]}")
    return f


def _act(alg_of, rows_list, ck):
    """zbp_act on slot 3 with the caller's noise against the fp64 reference. A field's outputs over the
    case's launches (1, 33, 200 rows) are one compared tensor: the single numbers a 1-row launch
    yields have no scale of their own for a relative bound (a value of 3e-4 with the 1e-7 error of
    its fp32 dot products) and no typical error quotient. Each launch on its own is held to the
    existing act test's 1e-5 max(1, max |x64|), and its sigma and observation copies are bit-exact."""
    import torch
    from zbot_lab_amd.rl import fused
    out = {}
    for rows in rows_list:
        alg = alg_of(rows)
        pol, st = alg.policy, alg.storage
        fu = fused.FusedUpdate(alg, 256)  # (the minibatch size shapes only the update's row buffers)
        st.clear()
        g = torch.Generator().manual_seed(100 + rows)
        norm = cases.norms(pol)[0] is not None
        o_law, c_law = ((3.0, 0.5), (-2.0, 0.7)) if norm else ((0.0, 1.0), (0.0, 1.0))
        obs = (o_law[0] + o_law[1] * torch.randn(rows, st.observations.shape[-1], generator=g)).cuda()
        cobs = (c_law[0] + c_law[1] * torch.randn(rows, st.critic_observations.shape[-1], generator=g)).cuda()
        st.step = 3
        fu.pack()
        _poison(st.observations[3], st.critic_observations[3], st.actions[3], st.values[3], st.actions_log_prob[3],
                st.mu[3], st.sigma[3])
        a = fu.act(obs, cobs, st)
        noise = fu._noise.clone()
        with torch.no_grad():
            pol.update_distribution(obs)
            mu, sd = pol.action_mean, pol.action_std
            a32 = mu + sd * noise
            lp32 = pol.get_actions_log_prob(a32)
            v32 = pol.evaluate(cobs)
        torch.cuda.synchronize()
        na, nc = cases.norms(pol)
        ref = R.act_reference(*cases.net_tensors(pol), obs, cobs, noise, actor_norm=na, critic_norm=nc)
        for k, got, t32 in (("actions", a, a32), ("storage actions", st.actions[3], a32), ("mu", st.mu[3], mu),
                            ("sigma", st.sigma[3], sd), ("log_prob", st.actions_log_prob[3], lp32), ("value", st.values[3], v32)):
            out.setdefault(k, []).append([R.f64(x).reshape(-1) for x in (got, t32, ref[k.replace("storage ", "")])])
            # per launch, the existing act test's bound: 1e-5 max(1, max |x64|)
            r64 = ref[k.replace("storage ", "")]
            ck.cap(f"{rows}:{k}", got, r64, atol=max(0.0, 1e-5 * (1.0 - float(r64.abs().max()))))
        ck.exact(f"{rows}:sigma is std", st.sigma[3], pol.std.detach().expand_as(st.sigma[3]))
        ck.exact(f"{rows}:observations", st.observations[3], obs)
        ck.exact(f"{rows}:critic observations", st.critic_observations[3], cobs)
    for k, parts in out.items():
        ck.close(f"rows {rows_list}:{k}", *[torch.cat([p[j] for p in parts]) for j in range(3)])


# ------------------------------------------------------------------ per-action std, shipped kernels
@pytest.mark.parametrize("rows", ["reg", "lds"])
@pytest.mark.parametrize("shape", [cases.V2, cases.STANDUP], ids=["v2-nets", "standup-nets"])
def test_per_action_std_minibatch(gpu, shape, rows, monkeypatch):
    """k_rows_reg (these shapes' default at 192 rows) and k_rows (ZBP_ROWS=lds) with std = 0.3 .. 2.0."""
    if rows == "lds":
        monkeypatch.setenv("ZBP_ROWS", "lds")
    ck = Check(f"per-action std minibatch {shape['actor']} {rows}")
    _minibatch(cases.make_alg("cuda:0", shape, 192), ck)
    ck.done()


@pytest.mark.parametrize("kernel", ["reg", "lds", "split"])
@pytest.mark.parametrize("shape", [cases.V2, cases.STANDUP], ids=["v2-nets", "standup-nets"])
def test_per_action_std_act(gpu, shape, kernel, monkeypatch):
    """zbp_act with ZBP_ACT = reg / lds / split at 40 and 200 rows (split serves the 128-wide nets; the
    256-wide ones take k_act_reg under it, as the library dispatches)."""
    monkeypatch.setenv("ZBP_ACT", kernel)
    if kernel == "lds":
        monkeypatch.setenv("ZBP_ROWS", "lds")
    ck = Check(f"per-action std act {shape['actor']} {kernel}")
    _act(lambda rows: cases.make_alg("cuda:0", shape, (rows, 4)), (40, 200), ck)
    ck.done()


# ------------------------------------------------------------------ the generic shape matrix
MATRIX = [("partial", (96, 160)), ("minimum", (96, 160)), ("maximum", (96, 160, 1024, 2560)), ("mixed", (96, 160)),
          ("shallow", (96, 160))]


@pytest.mark.parametrize("name,rows", MATRIX, ids=[m[0] for m in MATRIX])
def test_shape_matrix_minibatch(gpu, name, rows):
    ck = Check(f"matrix minibatch {name}")
    for r in rows:
        _minibatch(cases.make_alg("cuda:0", cases.SHAPES[name], r), ck)
    ck.done()


@pytest.mark.parametrize("name", [m[0] for m in MATRIX])
def test_shape_matrix_act(gpu, name):
    ck = Check(f"matrix act {name}")
    _act(lambda rows: cases.make_alg("cuda:0", cases.SHAPES[name], (rows, 4)), (1, 33, 200), ck)
    ck.done()


def test_single_layer_nets(gpu):
    """n_layers == 1 (no hidden layer): whichever answer fused.supported() gives is the library's
    (zbp_workspace_floats agrees), and when it is yes the numbers hold."""
    from zbot_lab_amd.rl import fused
    alg = cases.make_alg("cuda:0", cases.SHAPES["linear"], 96)
    ok = fused.supported(alg.policy, 96)
    na, nc = fused._net(fused.mlp_layers(alg.policy.actor)), fused._net(fused.mlp_layers(alg.policy.critic))
    import ctypes as C
    assert ok == (fused.lib().zbp_workspace_floats(C.byref(na), C.byref(nc), 96) > 0)
    if not ok:
        return
    ck = Check("single-layer nets")
    for r in (96, 160):
        _minibatch(cases.make_alg("cuda:0", cases.SHAPES["linear"], r), ck)
    _act(lambda rows: cases.make_alg("cuda:0", cases.SHAPES["linear"], (rows, 4)), (1, 33, 200), ck)
    ck.done()


def test_shape_matrix_with_normalizers(gpu):
    """The first matrix row with both observation normalizers on (statistics of a shifted, scaled
    batch; different dims and laws for the two nets)."""
    ck = Check("matrix partial, normalizers on")
    for r in (96, 160):
        alg = cases.make_alg("cuda:0", cases.SHAPES["partial"], r, normalizers=True)
        assert int(alg.policy.actor_obs_normalizer.count) == 1024
        f = _minibatch(alg, ck)
        assert f.norm_a.mean and f.norm_c.mean
    _act(lambda rows: cases.make_alg("cuda:0", cases.SHAPES["partial"], (rows, 4), normalizers=True), (33, 200), ck)
    ck.done()


# ------------------------------------------------------------------ loss branches
LOSS_RUNS = [("v2", "reg"), ("v2", "lds"), ("partial", "lds")]


@pytest.mark.parametrize("entropy_coef", [cases.LOSS["entropy_coef"], 0.0])
@pytest.mark.parametrize("clipped", [True, False], ids=["clipped-value", "plain-value"])
@pytest.mark.parametrize("case,rows", LOSS_RUNS, ids=[f"{c}-{r}" for c, r in LOSS_RUNS])
def test_loss_branches(gpu, case, rows, clipped, entropy_coef, monkeypatch):
    """use_clipped_value_loss 0 / 1 with clip_param 0.13, value_loss_coef 0.7, entropy_coef 0.02 / 0 on
    both row kernels; at least 10 % of the rows on each side of each clamp and max (fp64 reference)."""
    if rows == "lds":
        monkeypatch.setenv("ZBP_ROWS", "lds")
    name, shape, mb = {c[0]: c for c in cases.LOSS_CASES}[case]
    kw = dict(cases.LOSS, entropy_coef=entropy_coef)
    alg = cases.make_alg("cuda:0", shape, mb, use_clipped_value_loss=clipped, **kw)
    ck = Check(f"loss branches {name} {rows} clipped {int(clipped)} entropy_coef {entropy_coef}")
    f = _minibatch(alg, ck, sides_clipped=clipped)
    assert (round(f.loss.clip_param, 6), round(f.loss.value_loss_coef, 6), f.loss.use_clipped_value_loss) == (
        0.13, 0.7, int(clipped))
    ck.done()


# ------------------------------------------------------------------ zbp_optimizer_step
# (kl, rate before, rate after or None: compared with the tolerance): desired_kl = 0.01
RATE_STATES = [(0.05, 1e-5, 1e-5), (0.002, 1e-2, 1e-2), (0.01, 1e-3, 1e-3), (-0.001, 1e-3, 1e-3),
               (0.05, 1e-3, None), (0.002, 1e-3, None)]


@pytest.mark.parametrize("nfm", [0, 1], ids=["k_norm", "norm-from-minibatch"])
@pytest.mark.parametrize("max_norm", [0.05, 1e3], ids=["clipping", "no-clipping"])
@pytest.mark.parametrize("name", ["partial", "maximum"])
def test_optimizer_step(gpu, name, max_norm, nfm):
    """zbp_optimizer_step alone (FusedUpdate.optimizer_step) from a mid-training Adam state (step 7,
    the moments of another minibatch's gradients) in every branch of the rate rule: kl above
    2 desired_kl with the rate at 1e-5, 0 < kl < desired_kl / 2 with the rate at 1e-2, kl in between,
    kl <= 0, and both moving branches away from the bounds. Parameters, the clipped gradients left in
    .grad, exp_avg, exp_avg_sq, the step counters, the rate and acc += stats[1..3]."""
    import torch
    from zbot_lab_amd.rl import fused
    alg = cases.make_alg("cuda:0", cases.SHAPES[name], 96, max_grad_norm=max_norm)
    assert alg.desired_kl == 0.01 and alg.schedule == "adaptive"
    alg_t = copy.deepcopy(alg)
    alg_t.optimizer = torch.optim.Adam(alg_t.policy.parameters(), lr=alg_t.lr_t, fused=True, capturable=True)
    pol, mb = alg.policy, 96
    ps, ps_t = list(pol.parameters()), list(alg_t.policy.parameters())
    f = fused.FusedUpdate(alg, mb)
    f.pack()
    f.minibatch(alg.storage, alg.mb_indices, 0)
    p0 = [p.detach().clone() for p in ps]
    m0 = [p.grad.detach().clone() for p in ps]
    v0 = [g.square() + 1e-3 * g.abs().max() ** 2 for g in m0]
    for opt, params in ((alg.optimizer, ps), (alg_t.optimizer, ps_t)):
        for p in params:
            opt.state[p] = {"step": torch.zeros((), device="cuda:0"), "exp_avg": torch.zeros_like(p),
                            "exp_avg_sq": torch.zeros_like(p)}
    b1, b2 = alg.optimizer.param_groups[0]["betas"]
    eps = alg.optimizer.param_groups[0]["eps"]
    as32 = lambda x: float(np.float32(x))  # noqa: E731  (the C ABI's float arguments)
    ck = Check(f"optimizer step {name} max_norm {max_norm} nfm {nfm}")
    for kl, lr, lr_after in RATE_STATES:
        for opt, params in ((alg.optimizer, ps), (alg_t.optimizer, ps_t)):
            with torch.no_grad():
                for p, a, b, c in zip(params, p0, m0, v0):
                    p.copy_(a)
                    opt.state[p]["exp_avg"].copy_(b)
                    opt.state[p]["exp_avg_sq"].copy_(c)
                    opt.state[p]["step"].fill_(7.0)
        alg.lr_t.fill_(lr)
        alg_t.lr_t.fill_(lr)
        f.pack()
        f.minibatch(alg.storage, alg.mb_indices, mb)
        g0 = [p.grad.detach().clone() for p in ps]
        f.stats[0] = kl
        stats = f.stats.clone()
        acc = torch.tensor([0.5, -0.25, 3.0], device="cuda:0")
        acc0 = acc.clone()
        lr0 = alg.lr_t.clone()
        f.optimizer_step(acc, grads_from_minibatch=bool(nfm))
        assert f._norm_ok
        torch.cuda.synchronize()
        ref = R.adam_reference(p0, g0, m0, v0, 7.0, float(lr0), kl, as32(alg.desired_kl), as32(max_norm), as32(b1),
                               as32(b2), as32(eps))
        assert (ref["coef"] < 1.0) == (max_norm < 1.0), ref["norm"]
        # the project's torch statement in fp32 from the same state and gradients
        with torch.no_grad():
            for p, g in zip(ps_t, g0):
                p.grad = g.clone()
        alg_t._adapt_learning_rate(stats[0])
        torch.nn.utils.clip_grad_norm_(ps_t, max_norm)
        alg_t.optimizer.step()
        torch.cuda.synchronize()
        tag = f"kl {kl} lr {lr}"
        for i, (p, pt) in enumerate(zip(ps, ps_t)):
            n = f"{tag}:{i}"
            ck.close(n + " param", p, pt, ref["params"][i])
            ck.close(n + " grad", p.grad, pt.grad, ref["grads"][i])
            ck.close(n + " exp_avg", alg.optimizer.state[p]["exp_avg"], alg_t.optimizer.state[pt]["exp_avg"],
                     ref["exp_avg"][i])
            ck.close(n + " exp_avg_sq", alg.optimizer.state[p]["exp_avg_sq"], alg_t.optimizer.state[pt]["exp_avg_sq"],
                     ref["exp_avg_sq"][i])
            assert float(alg.optimizer.state[p]["step"]) == 8.0 == ref["step"], n
        if lr_after is not None:  # at a bound, or unchanged: exactly
            ck.exact(tag + " lr", alg.lr_t, torch.tensor(lr_after, device="cuda:0"))
        ck.close(tag + " lr", alg.lr_t, alg_t.lr_t, torch.tensor(ref["lr"], dtype=torch.float64))
        ck.close(tag + " acc", acc, acc0 + stats[1:], acc0.double() + stats[1:].double())
    ck.done()


# ------------------------------------------------------------------ zbp_gae, zbp_env_post
# (normalize = 1 needs more than one element: the unbiased std of one does not exist)
GAE_CASES = [(1, 1, 0), (3, 100, 0), (3, 100, 1), (24, 257, 0), (24, 257, 1), (5, 70000, 0), (5, 70000, 1)]


@pytest.mark.parametrize("steps,envs,normalize", GAE_CASES)
def test_gae_edges(gpu, steps, envs, normalize, monkeypatch):
    """zbp_gae below one block, at a ragged block count and beyond one grid pass (256 x 256 threads),
    with and without the normalisation, a done in the last step."""
    import torch
    from zbot_lab_amd.rl import fused
    from zbot_lab_amd.rl.ppo import RolloutStorage
    st = RolloutStorage(envs, steps, 1, 1, 1, "cuda:0")
    g = torch.Generator().manual_seed(steps * 1000 + envs)
    st.rewards.copy_(torch.randn(st.rewards.shape, generator=g))
    st.values.copy_(torch.randn(st.values.shape, generator=g))
    st.dones.copy_((torch.rand(st.dones.shape, generator=g) < 0.1).float())
    st.dones[-1, 0] = 1.0
    last = torch.randn(envs, 1, generator=g).cuda()
    ref_ret, ref_adv = R.gae_reference(st.rewards, st.dones, st.values, last, 0.99, 0.95, bool(normalize))
    monkeypatch.setenv("ZBOT_PPO_FUSED", "0")  # the torch recursion in fp32
    st.compute_returns(last, 0.99, 0.95, bool(normalize))
    ret32, adv32 = st.returns.clone(), st.advantages.clone()
    _poison(st.returns, st.advantages)
    fused.gae(st, last, 0.99, 0.95, bool(normalize))
    torch.cuda.synchronize()
    ck = Check(f"gae {steps} x {envs} normalize {normalize}")
    ck.close("returns", st.returns, ret32, ref_ret)
    ck.close("advantages", st.advantages, adv32, ref_adv)
    ck.done()


@pytest.mark.parametrize("done", ["none", "all", "some"])
@pytest.mark.parametrize("time_outs", [True, False], ids=["time-outs", "no-time-outs"])
@pytest.mark.parametrize("n", [1, 1000, 1025, 4097, 5000])
def test_env_post_edges(gpu, n, time_outs, done):
    """zbp_env_post (one workgroup of 1024 threads, four envs per thread) below one pass, one env into
    the second thread slot, one env into the second pass and a ragged second pass: the clamped loads
    must not leak into the sums. Storage reward / done and cur_rew / cur_len exactly as the torch
    statement in fp32; ep_stats against fp64."""
    import torch
    from zbot_lab_amd.rl import fused
    from zbot_lab_amd.rl.ppo import RolloutStorage
    alg = cases.make_alg("cuda:0", cases.SHAPES["minimum"], 96)
    fu = fused.FusedUpdate(alg, 96)
    st = RolloutStorage(n, 2, 1, 1, 1, "cuda:0")
    g = torch.Generator().manual_seed(n)
    rew = torch.randn(n, generator=g).cuda()
    dones = {"none": torch.zeros(n), "all": torch.ones(n), "some": (torch.rand(n, generator=g) < 0.2).float()}[
        done].long().cuda()
    tout = ((torch.rand(n, generator=g) < 0.5).cuda() & (dones > 0)) if time_outs else None
    cur_rew = torch.randn(n, generator=g).cuda()
    cur_len = torch.randint(0, 100, (n,), generator=g).float().cuda()
    ep = torch.tensor([1.0, 2.0, 3.0], device="cuda:0")
    st.values.copy_(torch.randn(st.values.shape, generator=g))
    st.step = 1
    val = st.values[1].clone()
    ref = R.env_post_reference(rew, dones, tout, val, alg.gamma, cur_rew, cur_len, ep)
    # the torch statement in fp32 (PPO.process_env_step, the runner's bookkeeping)
    r32 = rew.clone()
    if tout is not None:
        r32 += alg.gamma * torch.squeeze(val * tout.unsqueeze(1).float(), 1)
    c32, l32, d = cur_rew + rew, cur_len + 1, dones > 0
    ep32 = ep + torch.stack([torch.where(d, c32, 0.0).sum(), torch.where(d, l32, 0.0).sum(), d.sum().float()])
    c32, l32 = c32.masked_fill(d, 0.0), l32.masked_fill(d, 0.0)
    _poison(st.rewards[1], st.dones[1])
    fu.env_post(st, rew, dones, tout, alg.gamma, cur_rew, cur_len, ep)
    torch.cuda.synchronize()
    assert st.step == 2
    ck = Check(f"env_post n {n} time_outs {time_outs} done {done}")
    ck.exact("reward", st.rewards[1].view(-1), r32)
    ck.exact("done", st.dones[1].view(-1), dones.float())
    ck.exact("cur_rew", cur_rew, c32)
    ck.exact("cur_len", cur_len, l32)
    ck.close("reward", st.rewards[1], r32, ref["st_rewards"])
    ck.close("cur_rew", cur_rew, c32, ref["cur_rew"])
    ck.close("cur_len", cur_len, l32, ref["cur_len"])
    for k, nm in enumerate(("sum of returns", "sum of lengths", "episodes")):
        ck.close(f"ep_stats {nm}", ep[k], ep32[k], ref["ep_stats"][k])
    ck.done()
