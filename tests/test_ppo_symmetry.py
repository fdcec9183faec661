"""rsl_rl's symmetry option on the CPU: the mirror map (zbot_lab_amd/rl/symmetry.py), and the torch path of
PPO.update_steps against the fp64 statement of tests/ppo_symmetry_reference.py in the three modes. The
policies and the storage run in fp64 here (test_ppo_reference._double), so the comparison is to 1e-10
relative, as the other reference tests'."""
from __future__ import annotations

import copy
import dataclasses

import pytest
import torch

import ppo_cases as cases
import ppo_symmetry_cases as SC
from test_ppo_reference import _close, _double


def _sp():
    from zbot_lab_amd.rl.symmetry import SignedPermutation
    return SignedPermutation


# ------------------------------------------------------------------ SignedPermutation
def test_signed_permutation_semantics():
    SP = _sp()
    m = SP([2, 0, 1, 3], [1, -1, 1, -1], [1, 2, 0], [-1, 1, 1], critic_obs_perm=[1, 0], critic_obs_sign=[1, -1])
    obs = torch.tensor([[10.0, 20.0, 30.0, 40.0], [1.0, 2.0, 3.0, 4.0]])
    act = torch.tensor([[5.0, 6.0, 7.0], [8.0, 9.0, 0.5]])
    cobs = torch.tensor([[1.5, 2.5], [3.5, 4.5]])
    o, a = m(obs=obs, actions=act)
    assert torch.equal(o, torch.cat([obs, torch.tensor([[30.0, -10.0, 20.0, -40.0], [3.0, -1.0, 2.0, -4.0]])]))
    assert torch.equal(a, torch.cat([act, torch.tensor([[-6.0, 7.0, 5.0], [-9.0, 0.5, 8.0]])]))
    g, a2 = m(obs={"policy": obs, "critic": cobs}, actions=None, env=object())
    assert a2 is None and torch.equal(g["policy"], o)
    assert torch.equal(g["critic"], torch.cat([cobs, torch.tensor([[2.5, -1.5], [4.5, -3.5]])]))
    assert m(obs=None, actions=None) == (None, None)
    # not an involution: mirroring twice is another map
    assert not torch.equal(m.mirror(m.mirror(obs, "obs"), "obs"), obs)
    # fp64 in, fp64 out
    assert m(obs=obs.double())[0].dtype == torch.float64


def test_signed_permutation_critic_tables_default_to_the_policys():
    SP = _sp()
    m = SP([1, 0, 2], [1, 1, -1], [0], [-1])
    x = torch.tensor([[1.0, 2.0, 3.0]])
    assert torch.equal(m(obs={"policy": x, "critic": x})[0]["critic"], torch.tensor([[1.0, 2.0, 3.0], [2.0, 1.0, -3.0]]))
    assert m.matches(3, 3, 1) and not m.matches(3, 4, 1)
    with pytest.raises(ValueError, match="critic"):
        m(obs={"policy": x, "critic": torch.zeros(1, 4)})


@pytest.mark.parametrize("args", [
    ([0, 0, 1], [1, 1, 1], [0], [1]),           # not a permutation
    ([0, 1, 3], [1, 1, 1], [0], [1]),           # out of range
    ([0, 1, 2], [1, 0.5, 1], [0], [1]),         # sign not +-1
    ([0, 1, 2], [1, 1], [0], [1]),              # lengths differ
    ([0, 1, 2], [1, 1, 1], [0, 1], [1, 0]),     # action sign 0
    ([], [], [0], [1]),                         # empty
])
def test_signed_permutation_refusals(args):
    with pytest.raises(ValueError):
        _sp()(*args)
    with pytest.raises(ValueError):
        _sp()([0, 1], [1, 1], [0], [1], critic_obs_perm=[0, 1])  # perm without sign


def test_signed_permutation_deep_copies_and_rides_the_cfg():
    from zbot_lab_amd.rl.cfg import PPORunnerCfgV2, RslRlPpoAlgorithmCfg, RslRlSymmetryCfg
    m = SC.random_map(cases.V2)
    m.device_tables("obs", "cpu")
    c = copy.deepcopy(m)
    assert c is not m and c.to_dict() == m.to_dict()
    cfg = PPORunnerCfgV2(algorithm=RslRlPpoAlgorithmCfg(symmetry_cfg=RslRlSymmetryCfg(
        use_data_augmentation=True, use_mirror_loss=True, mirror_loss_coeff=0.5, data_augmentation_func=m)))
    d = cfg.to_dict()["algorithm"]["symmetry_cfg"]
    assert d["use_mirror_loss"] and d["mirror_loss_coeff"] == 0.5
    assert d["data_augmentation_func"].to_dict() == m.to_dict()
    assert dataclasses.asdict(PPORunnerCfgV2())["algorithm"]["symmetry_cfg"] is None
    assert _sp().from_dict(m.to_dict()).to_dict() == m.to_dict()


# ------------------------------------------------------------------ the torch path against fp64
def _alg64(shape, rows, mode, **kw):
    alg = _double(SC.make_alg("cpu", shape, rows, mode, **kw))
    alg.symmetry_sum = alg.symmetry_sum.double()
    return alg


CASES = [("v2", cases.V2, 192, {}), ("partial", cases.SHAPES["partial"], 96, {}),
         ("v2-relu-log-norm", cases.V2, 192, dict(act="relu", std_type="log", normalizers=True))]


@pytest.mark.parametrize("mode", ["aug", "mirror", "both"])
@pytest.mark.parametrize("name,shape,rows,kw", CASES, ids=[c[0] for c in CASES])
def test_torch_path_matches_fp64_reference(name, shape, rows, kw, mode):
    alg = _alg64(shape, rows, mode, **kw)
    assert alg.fused_update() is None
    ref, ref_stats = SC.reference_minibatch(alg, 1, kw.get("act", "elu"), kw.get("std_type", "scalar"))
    stats = SC.torch_minibatch(alg, 1)
    assert float(ref_stats[4]) > 1e-4
    _close(stats, ref_stats, "stats")
    for n, p in alg.policy.named_parameters():
        _close(p.grad, ref[n], n)


def test_update_stats_gains_symmetry_only_with_a_cfg():
    # (one epoch at rate 0: every minibatch sees the snapshot's parameters)
    alg = SC.make_alg("cpu", cases.V2, 96, "both", num_learning_epochs=1, learning_rate=0.0, schedule="fixed")
    ref_stats = [SC.reference_minibatch(alg, i, "elu", "scalar")[1][4] for i in range(4)]
    alg.update_steps()
    out = alg.update_stats()
    assert set(out) == {"value_function", "surrogate", "entropy", "symmetry"}
    assert out["symmetry"] == pytest.approx(float(sum(ref_stats)) / 4, rel=1e-4)
    plain = SC.make_alg("cpu", cases.V2, 96, None)
    plain.update_steps()
    assert set(plain.update_stats()) == {"value_function", "surrogate", "entropy"}


def test_symmetry_cfg_none_is_bit_identical_to_omitting_it():
    a = SC.make_alg("cpu", cases.V2, 96, None)
    b = SC.make_alg("cpu", cases.V2, 96, None, symmetry_cfg=None)
    assert a.symmetry is None and b.symmetry is None
    a.update_steps()
    b.update_steps()
    assert a.update_stats() == b.update_stats()
    for (n, p), q in zip(a.policy.named_parameters(), b.policy.parameters()):
        assert torch.equal(p, q) and torch.equal(p.grad, q.grad), n
    assert float(a.lr_t) == float(b.lr_t)


def test_identity_map_has_zero_mirror_loss_and_the_plain_gradients():
    shape = cases.V2
    alg = _alg64(shape, 96, "both", func=SC.identity_map(shape))
    plain = _alg64(shape, 96, None, func=SC.identity_map(shape))
    stats = SC.torch_minibatch(alg, 1)
    stats0 = SC.torch_minibatch(plain, 1)
    assert float(stats[4]) == 0.0
    _close(stats[:4], stats0[:4], "stats")
    for (n, p), q in zip(alg.policy.named_parameters(), plain.policy.parameters()):
        _close(p.grad, q.grad, n)


def test_any_callable_runs_the_torch_path():
    """A plain function with rsl_rl's signature (no SignedPermutation): three copies per row."""
    shape = cases.V2
    m = SC.random_map(shape)

    def func(obs=None, actions=None, env=None):
        o = None if obs is None else {k: torch.cat([v, m.mirror(v, "critic" if k == "critic" else "obs"), v]) for k, v in obs.items()}
        a = None if actions is None else torch.cat([actions, m.mirror(actions, "actions"), actions])
        return o, a

    alg = _alg64(shape, 96, "both", func=func)
    assert alg.symmetry["data_augmentation_func"] is func
    ref, ref_stats = SC.reference_minibatch(alg, 1, "elu", "scalar")
    stats = SC.torch_minibatch(alg, 1)
    _close(stats, ref_stats, "stats")
    for n, p in alg.policy.named_parameters():
        _close(p.grad, ref[n], n)
    from zbot_lab_amd.rl import fused
    with pytest.warns(UserWarning, match="torch path"):
        fused._warned_symmetry = False
        assert not fused.symmetry_supported(alg.policy, alg.symmetry)
    assert fused.symmetry_supported(alg.policy, SC.make_alg("cpu", shape, 96, "both").symmetry)
    with pytest.raises(ValueError):
        SC.make_alg("cpu", shape, 96, None, symmetry_cfg=dict(use_mirror_loss=True, data_augmentation_func=3))


def test_train_cli_builds_the_symmetry_cfg(tmp_path):
    """scripts/train.py --symmetry FILE.json --symmetry_mode --mirror_loss_coeff -> algorithm.symmetry_cfg."""
    import importlib.util
    import json
    import os
    from zbot_lab_amd.rl import PPORunnerCfgV2
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("train_cli", os.path.join(root, "scripts", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    m = SC.random_map(cases.V2)
    path = tmp_path / "map.json"
    path.write_text(json.dumps(m.to_dict()))
    args = train.build_parser().parse_args(["--symmetry", str(path), "--symmetry_mode", "mirror", "--mirror_loss_coeff", "0.25"])
    sy = train.update_rsl_rl_cfg(PPORunnerCfgV2(), args).to_dict()["algorithm"]["symmetry_cfg"]
    assert (sy["use_data_augmentation"], sy["use_mirror_loss"], sy["mirror_loss_coeff"]) == (False, True, 0.25)
    assert sy["data_augmentation_func"].to_dict() == m.to_dict()
    plain = train.update_rsl_rl_cfg(PPORunnerCfgV2(), train.build_parser().parse_args([]))
    assert plain.algorithm.symmetry_cfg is None
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps(dict(m.to_dict(), obs_sign=[0.0] * 23)))
    with pytest.raises(ValueError):
        train.update_rsl_rl_cfg(PPORunnerCfgV2(), train.build_parser().parse_args(["--symmetry", str(bad)]))
