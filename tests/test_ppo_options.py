"""The activation and noise_std_type options of the PPO side, on the CPU: tests/ppo_options_reference.py
(the fp64 statement tests/test_gpu_ppo_options.py holds the kernels to) against PPO.update_steps, the
policy's act and autograd run in fp64, to 1e-10 relative, for each of the four new activations x
{scalar, log}; the derivatives written from the activation's output and the closed-form noise gradient
(what the kernels compute) against autograd; the kink condition of the case builder; the module-level
behaviour of ``ActorCritic(noise_std_type=...)``, the cfg dataclass, ``fused.mlp_layers``, a checkpoint
round trip and the TorchScript export of a relu + log policy; the library's host-side rejection of a
mixed or out-of-range activation; and how far three deliberately wrong derivatives move a gradient,
against the tolerance the GPU tests apply.

Sensitivity, measured here (pytest -s prints the line): SELU's negative side as lambda moves
actor.0.weight by 4.8e+04 x the GPU tolerance, tanh's derivative as 1 - x by 1.2e+05 x, d log sigma
without its factor sigma by 6.8e+04 x."""
from __future__ import annotations

import ctypes as C
import os

import pytest
import torch
import torch.nn as nn

import ppo_cases as cases
import ppo_options_cases as ocases
import ppo_options_reference as RO
import ppo_reference as R
from test_ppo_reference import _close, _double, _gpu_tolerance

NEW_ACTS = ("relu", "tanh", "selu", "lrelu")


# ------------------------------------------------------------------ the reference against the torch code
@pytest.mark.parametrize("std_type", RO.STD_TYPES)
@pytest.mark.parametrize("act", NEW_ACTS)
def test_minibatch_reference_matches_update_steps(act, std_type):
    """PPO.update_steps (torch path, fp64, one epoch of four minibatches at rate 0): the gradients it
    leaves are the last minibatch's, its loss sums the four minibatches', the KL each minibatch's; and
    the tests' single-minibatch statement (the GPU file's fp32 side) agrees too. With normalizers on for
    the log cases, so both features are stated together once."""
    normalizers = std_type == "log"
    alg = ocases.make_alg("cpu", cases.SHAPES["partial"], 96, act=act, std_type=std_type, normalizers=normalizers,
                          num_learning_epochs=1, learning_rate=0.0, max_grad_norm=1e30, **cases.LOSS)
    _double(alg)
    ref = [ocases.reference_minibatch(alg, i, act, std_type) for i in range(alg.num_mini_batches)]
    kls = []
    alg._adapt_learning_rate = lambda kl: kls.append(float(kl))
    alg.update_steps()
    named, _, _ = ref[-1]
    assert set(named) == {n for n, _ in alg.policy.named_parameters()}
    assert ("log_std" in named) == (std_type == "log") and ("std" in named) == (std_type == "scalar")
    for n, p in alg.policy.named_parameters():
        _close(p.grad, named[n], n)
    _close(torch.tensor(kls, dtype=torch.float64), torch.stack([r[1][0] for r in ref]), "kl")
    _close(alg.update_sums, torch.stack([r[1][1:] for r in ref]).sum(0), "loss sums")
    for i in (0, 2):
        stats = cases.torch_minibatch(alg, i)
        _close(stats, ref[i][1], f"stats of minibatch {i}")
        for n, p in alg.policy.named_parameters():
            _close(p.grad, ref[i][0][n], (i, n))


@pytest.mark.parametrize("act", NEW_ACTS)
def test_plain_value_loss_branch(act):
    alg = _double(ocases.make_alg("cpu", cases.V2, 96, act=act, std_type="log", use_clipped_value_loss=False,
                                  **cases.LOSS))
    named, vec, _ = ocases.reference_minibatch(alg, 1, act, "log")
    _close(cases.torch_minibatch(alg, 1), vec, "stats")
    for n, p in alg.policy.named_parameters():
        _close(p.grad, named[n], n)


@pytest.mark.parametrize("std_type", RO.STD_TYPES)
@pytest.mark.parametrize("act", RO.ACTIVATIONS)
def test_backward_from_outputs_and_noise_gradient_match_autograd(act, std_type):
    """The kernels' form of the backward pass (every derivative from the stored output) and of the noise
    gradient, against autograd's."""
    alg = _double(ocases.make_alg("cpu", cases.SHAPES["partial"], 96, act=act, std_type=std_type,
                                  entropy_coef=cases.LOSS["entropy_coef"], clip_param=cases.LOSS["clip_param"],
                                  value_loss_coef=0.0))
    named, _, _ = ocases.reference_minibatch(alg, 1, act, std_type)
    aw, ab, _, _, noise = ocases.net_tensors(alg.policy)
    rows = cases.gathered_rows(alg, 1)
    gw, gb = RO.actor_backward_from_outputs(aw, ab, noise, rows, alg.clip_param, act, std_type)
    for k, (idx, _) in enumerate(cases.linears(alg.policy.actor)):
        _close(gw[k], named[f"actor.{idx}.weight"], (act, idx, "weight"))
        _close(gb[k], named[f"actor.{idx}.bias"], (act, idx, "bias"))
    g = RO.noise_gradient_closed_form(aw, ab, noise, rows, alg.clip_param, alg.entropy_coef, act, std_type)
    _close(g, named[ocases.noise_name(alg.policy)], "noise gradient")


@pytest.mark.parametrize("std_type", RO.STD_TYPES)
@pytest.mark.parametrize("act", NEW_ACTS)
def test_act_reference_matches_policy(act, std_type):
    alg = _double(ocases.make_alg("cpu", cases.SHAPES["partial"], 96, act=act, std_type=std_type,
                                  normalizers=std_type == "log"))
    pol, sh = alg.policy, cases.SHAPES["partial"]
    g = torch.Generator().manual_seed(11)
    o_law, c_law = ((3.0, 0.5), (-2.0, 0.7)) if std_type == "log" else ((0.0, 1.0), (0.0, 1.0))
    obs = o_law[0] + o_law[1] * torch.randn(33, sh["obs"], generator=g, dtype=torch.float64)
    cobs = c_law[0] + c_law[1] * torch.randn(33, sh["cobs"], generator=g, dtype=torch.float64)
    noise = torch.randn(33, sh["act"], generator=g, dtype=torch.float64)
    with torch.no_grad():
        pol.update_distribution(obs)
        mu, sd = pol.action_mean, pol.action_std
        a = mu + sd * noise
        lp, v = pol.get_actions_log_prob(a), pol.evaluate(cobs)
    na, nc = cases.norms(pol)
    ref = RO.act_reference(*ocases.net_tensors(pol), obs, cobs, noise, act=act, std_type=std_type, actor_norm=na,
                           critic_norm=nc)
    for k, t in (("mu", mu), ("sigma", sd), ("actions", a), ("log_prob", lp), ("value", v)):
        _close(t, ref[k], k)


def test_elu_scalar_is_the_existing_reference():
    """With the defaults the new statement is tests/ppo_reference.py's."""
    alg = ocases.make_alg("cpu", cases.SHAPES["partial"], 96, **cases.LOSS)
    a, sa, _ = ocases.reference_minibatch(alg, 1, "elu", "scalar")
    b, sb, _ = cases.reference_minibatch(alg, 1)
    assert set(a) == set(b)
    for n in a:
        _close(a[n], b[n], n)
    _close(sa, sb, "stats")


# ------------------------------------------------------------------ the kink condition
@pytest.mark.parametrize("seed", range(6))
def test_kink_condition_redraws_few_rows(seed):
    """Default-initialised [128, 128, 128] nets, 768 rows: no hidden pre-activation within TAU of 0 is
    left, and at most 5 % of either observation tensor's rows were redrawn."""
    alg = ocases.make_alg("cpu", cases.V2, 192, act="relu", seed=seed)
    red, n = alg.redrawn
    print(f"\nseed {seed}: {red} (actor, critic) of {n} rows redrawn")
    assert n == 768 and 0 < sum(red) and max(red) <= 0.05 * n
    pol, st = alg.policy, alg.storage
    aw, ab, cw, cb, _ = ocases.net_tensors(pol)
    assert not ocases.near_kink_rows(st.observations.flatten(0, 1), aw, ab, None, "relu").any()
    assert not ocases.near_kink_rows(st.critic_observations.flatten(0, 1), cw, cb, None, "relu").any()


def test_kink_condition_uses_the_normalizer_statistics():
    alg = ocases.make_alg("cpu", cases.SHAPES["partial"], 96, act="selu", normalizers=True)
    pol, st = alg.policy, alg.storage
    aw, ab, cw, cb, _ = ocases.net_tensors(pol)
    na, nc = cases.norms(pol)
    assert na is not None and nc is not None
    assert not ocases.near_kink_rows(st.observations.flatten(0, 1), aw, ab, na, "selu").any()
    assert not ocases.near_kink_rows(st.critic_observations.flatten(0, 1), cw, cb, nc, "selu").any()


# ------------------------------------------------------------------ ActorCritic, cfg, fused.mlp_layers
def test_log_std_parameter_key_and_value():
    from zbot_lab_amd.rl.ppo import ActorCritic
    pol = ActorCritic(23, 23, 6, init_noise_std=0.7, noise_std_type="log")
    keys = set(pol.state_dict())
    assert "log_std" in keys and "std" not in keys and not hasattr(pol, "std")
    assert torch.allclose(pol.log_std.detach(), torch.log(torch.tensor(0.7)) * torch.ones(6))
    with torch.no_grad():
        pol.log_std.copy_(torch.linspace(-1.0, 0.5, 6))
    obs = torch.randn(5, 23)
    pol.update_distribution(obs)
    assert torch.equal(pol.action_std, torch.exp(pol.log_std).detach().expand(5, 6))
    assert torch.equal(pol.noise_std, torch.exp(pol.log_std))
    # the gradient reaches log_std through exp
    pol.get_actions_log_prob(torch.randn(5, 6)).sum().backward()
    assert pol.log_std.grad is not None and bool(pol.log_std.grad.abs().sum() > 0)


def test_scalar_policies_keep_their_keys():
    from zbot_lab_amd.rl.ppo import ActorCritic
    a, b = ActorCritic(23, 23, 6), ActorCritic(23, 23, 6, noise_std_type="scalar")
    assert list(a.state_dict()) == list(b.state_dict())
    assert "std" in a.state_dict() and "log_std" not in a.state_dict()
    # (the optimizer's order: the noise parameter, then the nets -- the same slot in either mode)
    assert [n for n, _ in a.named_parameters()][0] == "std"
    assert [n for n, _ in ActorCritic(23, 23, 6, noise_std_type="log").named_parameters()][0] == "log_std"
    assert torch.equal(a.noise_std, a.std)


def test_unknown_noise_std_type_raises():
    from zbot_lab_amd.rl.ppo import ActorCritic
    with pytest.raises(ValueError):
        ActorCritic(23, 23, 6, noise_std_type="softplus")


def test_cfg_carries_noise_std_type():
    from zbot_lab_amd.rl.cfg import PPORunnerCfgV2, RslRlPpoActorCriticCfg
    assert PPORunnerCfgV2().to_dict()["policy"]["noise_std_type"] == "scalar"
    cfg = PPORunnerCfgV2(policy=RslRlPpoActorCriticCfg(activation="relu", noise_std_type="log"))
    d = cfg.to_dict()["policy"]
    assert d["noise_std_type"] == "log" and d["activation"] == "relu"
    from zbot_lab_amd.rl.ppo import ActorCritic
    d.pop("class_name")
    pol = ActorCritic(23, 23, 6, **d)
    assert pol.noise_std_type == "log" and isinstance(pol.actor[1], nn.ReLU)


@pytest.mark.parametrize("act,module,code", [("elu", nn.ELU, 0), ("relu", nn.ReLU, 1), ("tanh", nn.Tanh, 2),
                                             ("selu", nn.SELU, 3), ("lrelu", nn.LeakyReLU, 4)])
def test_mlp_layers_accepts_every_activation(act, module, code):
    from zbot_lab_amd.rl import fused
    from zbot_lab_amd.rl.ppo import ActorCritic
    pol = ActorCritic(23, 23, 6, activation=act)
    for seq in (pol.actor, pol.critic):
        lin = fused.mlp_layers(seq)
        assert lin is not None and len(lin) == 4 and all(isinstance(m, nn.Linear) for m in lin)
        assert isinstance(seq[1], module) and fused.mlp_activation(seq) == code
    assert fused._net(fused.mlp_layers(pol.actor), code).activation == code


def test_mlp_layers_rejects_other_constants_and_mixed_modules():
    from zbot_lab_amd.rl import fused
    lin = lambda: nn.Linear(32, 32)  # noqa: E731
    assert fused.mlp_layers(nn.Sequential(lin(), nn.LeakyReLU(0.2), lin())) is None
    assert fused.mlp_layers(nn.Sequential(lin(), nn.ELU(0.5), lin())) is None
    assert fused.mlp_layers(nn.Sequential(lin(), nn.ReLU(), lin(), nn.Tanh(), lin())) is None
    assert fused.mlp_layers(nn.Sequential(lin(), nn.GELU(), lin())) is None
    assert fused.mlp_layers(nn.Sequential(lin(), nn.ReLU(), nn.ReLU(), lin(), lin())) is None
    assert fused.mlp_layers(nn.Sequential(lin(), nn.LeakyReLU(), lin(), nn.LeakyReLU(0.01), lin())) is not None


def test_checkpoint_round_trip_and_export_of_a_relu_log_policy(tmp_path):
    """save / load through the runner's checkpoint keys and the TorchScript export (the actor module)."""
    from zbot_lab_amd.rl import export
    from zbot_lab_amd.rl.ppo import PPO, ActorCritic
    torch.manual_seed(3)
    mk = lambda: ActorCritic(23, 23, 6, activation="relu", noise_std_type="log", init_noise_std=0.8)  # noqa: E731
    pol = mk()
    alg = PPO(pol, device="cpu")
    with torch.no_grad():
        pol.log_std.add_(torch.linspace(-0.2, 0.2, 6))
    path = str(tmp_path / "model_0.pt")
    torch.save({"model_state_dict": pol.state_dict(), "optimizer_state_dict": alg.optimizer.state_dict(), "iter": 0,
                "infos": None}, path)
    d = torch.load(path, map_location="cpu", weights_only=True)
    assert "log_std" in d["model_state_dict"] and "std" not in d["model_state_dict"]
    pol2 = mk()
    alg2 = PPO(pol2, device="cpu")
    pol2.load_state_dict(d["model_state_dict"])
    alg2.optimizer.load_state_dict(d["optimizer_state_dict"])
    assert torch.equal(pol2.log_std, pol.log_std)
    with pytest.raises(RuntimeError):  # a scalar policy does not take a log checkpoint silently
        ActorCritic(23, 23, 6, activation="relu").load_state_dict(d["model_state_dict"])
    obs = torch.randn(7, 23)
    out = str(tmp_path / "exported")
    export.export_policy_as_jit(pol2, None, out, "policy.pt")
    ts = torch.jit.load(os.path.join(out, "policy.pt"))
    assert torch.allclose(ts(obs), pol.act_inference(obs), atol=1e-6)


# ------------------------------------------------------------------ the library's host-side checks
def _nets(act_a, act_c):
    from zbot_lab_amd.rl import fused
    n = fused.Net()
    n.n_layers = 4
    for i, dd in enumerate([23, 128, 128, 128, 6]):
        n.dim[i] = dd
    for i in range(4):
        n.w[i] = n.b[i] = 16  # non-null; not dereferenced by the shape check
    m = fused.Net.from_buffer_copy(n)
    m.dim[4] = 1
    n.activation, m.activation = act_a, act_c
    return n, m


def test_library_rejects_mixed_and_out_of_range_activations():
    from zbot_lab_amd.rl import fused
    L = fused.lib()
    for a in range(5):
        n, m = _nets(a, a)
        assert L.zbp_workspace_floats(C.byref(n), C.byref(m), 192) > 0
    for a, c in ((5, 5), (-1, -1), (0, 5), (1 << 20, 0)):
        n, m = _nets(a, c)
        assert L.zbp_workspace_floats(C.byref(n), C.byref(m), 192) < 0
        assert b"activation" in L.zbp_last_error()
    n, m = _nets(1, 2)
    assert L.zbp_workspace_floats(C.byref(n), C.byref(m), 192) < 0
    assert b"same activation" in L.zbp_last_error()
    # the entry points that launch refuse the same before any launch (no GPU needed to hear it)
    ws = C.c_void_p(16)
    assert L.zbp_pack(C.byref(n), C.byref(m), ws, 192, None) < 0 and b"same activation" in L.zbp_last_error()
    io = fused.ActIO()
    assert L.zbp_act(C.byref(n), C.byref(m), ws, C.byref(io), ws, 192, None) < 0
    assert b"same activation" in L.zbp_last_error()
    b, lc = fused.Batch(), fused.LossCfg()
    assert L.zbp_minibatch(C.byref(n), C.byref(m), ws, ws, C.byref(b), C.byref(lc), ws, ws, None) < 0
    assert b"same activation" in L.zbp_last_error()


def test_struct_mirrors_have_the_new_fields():
    from zbot_lab_amd.rl import fused
    assert fused.Net._fields_[-1][0] == "activation"
    assert fused.LossCfg._fields_[-1][0] == "log_std" and fused.ActIO._fields_[-1][0] == "log_std"
    assert fused.Net().activation == 0 and fused.LossCfg().log_std == 0 and fused.ActIO().log_std == 0


# ------------------------------------------------------------------ sensitivity
def test_wrong_derivatives_move_far_beyond_the_tolerance():
    """SELU's negative side taken as lambda, tanh's derivative as 1 - x, and d log sigma without its
    factor sigma each move the compared gradient by orders of magnitude more than the loosest bound the
    GPU tests apply: a kernel with any of these defects cannot pass them."""
    out = []
    for act in ("selu", "tanh"):
        alg = ocases.make_alg("cpu", cases.V2, 192, act=act, **cases.LOSS)
        named, _, _ = ocases.reference_minibatch(alg, 1, act, "scalar")
        aw, ab, _, _, noise = ocases.net_tensors(alg.policy)
        gw, _ = RO.actor_backward_from_outputs(aw, ab, noise, cases.gathered_rows(alg, 1), alg.clip_param, act,
                                               wrong=True)
        ref = named["actor.0.weight"]
        out.append((f"{act} wrong derivative, actor.0.weight", float((gw[0] - ref).abs().max()), _gpu_tolerance(ref)))
    alg = ocases.make_alg("cpu", cases.V2, 192, act="tanh", std_type="log", **cases.LOSS)
    named, _, _ = ocases.reference_minibatch(alg, 1, "tanh", "log")
    aw, ab, _, _, noise = ocases.net_tensors(alg.policy)
    g = RO.noise_gradient_closed_form(aw, ab, noise, cases.gathered_rows(alg, 1), alg.clip_param, alg.entropy_coef,
                                      "tanh", "log", drop_sigma=True)
    out.append(("d log sigma without sigma, log_std", float((g - named["log_std"]).abs().max()),
                _gpu_tolerance(named["log_std"])))
    print()
    for what, moved, tol in out:
        print(f"{what}: moves {moved:.3g}, tolerance {tol:.3g} ({moved / tol:.3g} x)")
        assert moved > 1e3 * tol, what
