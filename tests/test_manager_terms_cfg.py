"""Manager env: rewards.gait / feet_clearance / feet_air_time / base_vel_forward / feet_force_pattern compile
from the cfg to the zb_manager_terms struct (include/zbot_manager_terms.h); any of the sixteen reward fields
may be None; the forms that are not compiled raise and say what is; the unedited cfg is "no term active"
with an unchanged TaskCfg and the same 11 log keys; the ctypes mirror has the C layout. No GPU."""
from __future__ import annotations

import ctypes as C
import dataclasses
import importlib.util
import os
import subprocess
import tempfile

import pytest

import zbot_lab_amd
from zbot_lab_amd import model as zm
from zbot_lab_amd.envs.manager_flat import DoneTerm, RewTerm, base_reward_term

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT_11 = ["track_lin_vel_xy_exp", "track_ang_vel_z_exp", "termination_penalty", "dof_torques_l2", "dof_acc_l2",
           "action_rate_l2", "foot_step_length", "foot_downward", "foot_forward", "feet_slide", "air_time_variance"]
BASE_WEIGHTS = {"gait": 0.5, "feet_clearance": 1.0, "feet_air_time": 2.5, "base_vel_forward": 1.0,
                "feet_force_pattern": 1.0}


def _cfg():
    return zbot_lab_amd.tasks.load_cfg("zbot-6b-walking-m-v0")


def _train():
    spec = importlib.util.spec_from_file_location("zbot_train_script", os.path.join(ROOT, "scripts", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    return train


def test_unedited_cfg_is_unchanged():
    cfg = _cfg()
    assert not cfg.manager_terms().enabled and cfg.manager_terms() == zm.ManagerTerms()
    assert dataclasses.asdict(cfg.task_cfg()) == dataclasses.asdict(zm.TaskCfg.manager_flat(solver_mode=1))
    assert cfg.reward_terms() == FLAT_11 == zm.M_REWARD_TERMS
    assert list(cfg.reward_cfg["reward_scales"]) == FLAT_11
    assert [zm.m_log_slot(k) for k in FLAT_11] == list(range(11))
    assert all(getattr(cfg.rewards, k) is None for k in zm.M_EXTRA_REWARD_TERMS + ["undesired_contacts"])
    assert zm.ManagerTerms().pack(zm.load_v09_model()).active == 0


@pytest.mark.parametrize("name", zm.M_EXTRA_REWARD_TERMS)
def test_each_term_compiles_with_the_base_params(name):
    cfg = _cfg()
    setattr(cfg.rewards, name, base_reward_term(name))
    before = dataclasses.asdict(zm.TaskCfg.manager_flat(solver_mode=1))
    assert dataclasses.asdict(cfg.task_cfg()) == before   # TaskCfg is untouched: the term lives beside it
    mt = cfg.manager_terms()
    assert mt.enabled and mt.weights == {name: BASE_WEIGHTS[name]}
    assert (mt.gait_period, mt.gait_offset, mt.gait_threshold) == (2.0, (0.0, 0.5), 0.55)
    assert (mt.clearance_std, mt.clearance_tanh_mult, mt.clearance_target_height) == (0.05, 2.0, 0.01)
    assert mt.air_time_threshold == 0.3 and mt.which_forward == 1
    k = zm.M_EXTRA_REWARD_TERMS.index(name)
    rm = zm.load_v09_model()
    p = mt.pack(rm)
    assert p.active == 1 << k and p.weight[k] == pytest.approx(BASE_WEIGHTS[name]) and sum(p.weight) == p.weight[k]
    assert [list(r) for r in p.clearance_point] == [[pytest.approx(v) for v in rm.link_com[l]] for l in (0, 11)]
    # cfg order among the existing terms, and the log slot behind the 11
    order = cfg.reward_terms()
    assert order == [n for n in zm.M_REWARD_FIELD_ORDER if n in FLAT_11 or n == name]
    assert zm.m_log_slot(name) == 11 + k
    assert list(cfg.reward_cfg["reward_scales"]) == order


def test_all_five_and_changed_params():
    cfg = _cfg()
    for name in zm.M_EXTRA_REWARD_TERMS:
        setattr(cfg.rewards, name, base_reward_term(name))
    cfg.rewards.gait.params.update(period=1.0, offset=(0.25, 0.75), threshold=0.6)
    cfg.rewards.base_vel_forward.params["which_forward"] = -1
    cfg.rewards.feet_air_time.weight = 0.0   # active with weight 0: still a term, still a log key
    mt = cfg.manager_terms()
    assert (mt.gait_period, mt.gait_offset, mt.gait_threshold, mt.which_forward) == (1.0, (0.25, 0.75), 0.6, -1)
    assert mt.pack(zm.load_v09_model()).active == 0b11111 and mt.weights["feet_air_time"] == 0.0
    assert cfg.reward_terms() == zm.M_REWARD_FIELD_ORDER


@pytest.mark.parametrize("edit, says", [
    (lambda c: c.rewards.gait.params.update(offset=[0.0, 0.3, 0.6]), "rewards.gait"),
    (lambda c: c.rewards.gait.params.update(offset=[0.0]), "rewards.gait"),
    (lambda c: c.rewards.gait.params.update(period=0.0), "rewards.gait"),
    (lambda c: c.rewards.gait.params.update(command_name=None), "rewards.gait"),
    (lambda c: setattr(c.rewards.gait, "func", "feet_gait_v2"), "rewards.gait"),
    (lambda c: c.rewards.base_vel_forward.params.update(which_forward=2), "which_forward"),
    (lambda c: c.rewards.base_vel_forward.params.update(which_forward=0), "which_forward"),
    (lambda c: c.rewards.feet_clearance.params.update(std=0.0), "rewards.feet_clearance"),
    (lambda c: c.rewards.feet_clearance.params.pop("tanh_mult"), "rewards.feet_clearance"),
    (lambda c: setattr(c.rewards.feet_air_time, "func", "feet_air_time"), "rewards.feet_air_time"),
    (lambda c: c.rewards.feet_force_pattern.params.update(sensor_cfg="contact_forces:.*"), "rewards.feet_force_pattern"),
    (lambda c: setattr(c.rewards, "undesired_contacts", RewTerm(
        "undesired_contacts", -1.0, {"sensor_cfg": "contact_forces:base|a.*|b.*", "threshold": 1.0})), "undesired_contacts"),
    (lambda c: setattr(c.terminations, "base_contact", DoneTerm(
        "illegal_contact", {"sensor_cfg": "contact_forces:base", "threshold": 1.0})), "base_contact"),
])
def test_uncompiled_forms_raise_and_name_the_compiled_ones(edit, says):
    cfg = _cfg()
    for name in zm.M_EXTRA_REWARD_TERMS:
        setattr(cfg.rewards, name, base_reward_term(name))
    cfg.task_cfg()
    edit(cfg)
    with pytest.raises(NotImplementedError) as e:
        cfg.task_cfg()
    msg = str(e.value)
    assert says in msg and "compiled: rewards.gait = RewTerm('feet_gait'" in msg
    assert "undesired_contacts and terminations.base_contact" in msg


@pytest.mark.parametrize("name", ["foot_forward", "track_ang_vel_z_exp", "air_time_variance"])
def test_subset_compiles_with_weight_zero_and_omits_the_key(name):
    cfg = _cfg()
    setattr(cfg.rewards, name, None)
    tc = cfg.task_cfg()
    k = FLAT_11.index(name)
    full = zm.TaskCfg.manager_flat(solver_mode=1).pack()
    packed = tc.pack()
    for t in range(zm.MAX_REWARD_TERMS):
        assert packed.stage_scales[0][t] == (0.0 if t == k else full.stage_scales[0][t])
    assert cfg.reward_terms() == [n for n in FLAT_11 if n != name]
    assert name not in cfg.reward_cfg["reward_scales"]
    assert not cfg.manager_terms().enabled   # still the plain kernel


def test_subset_with_a_restored_term():
    cfg = _cfg()
    cfg.rewards.foot_forward = None
    cfg.rewards.gait = base_reward_term("gait")
    cfg.task_cfg()
    assert cfg.reward_terms() == ["track_lin_vel_xy_exp", "track_ang_vel_z_exp", "termination_penalty", "dof_torques_l2",
                                  "dof_acc_l2", "action_rate_l2", "foot_step_length", "foot_downward", "gait",
                                  "feet_slide", "air_time_variance"]


def test_a_changed_compiled_term_still_raises():
    cfg = _cfg()
    cfg.rewards.foot_step_length.params["command_name"] = "base_velocity"
    with pytest.raises(NotImplementedError, match="foot_step_length"):
        cfg.task_cfg()


def test_ctypes_mirror_has_the_c_layout():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "zbot.h"\nint main(){printf("%zu %zu %zu %zu %d %d\\n", '
           'sizeof(zb_manager_terms), offsetof(zb_manager_terms, gait_offset), offsetof(zb_manager_terms, clearance_point), '
           'offsetof(zb_manager_terms, which_forward), ZB_MT_STATE_DIM, ZB_MT_GET_DIM);}\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "p.c"), os.path.join(d, "p")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        size, o_off, o_pt, o_wf, sd, gd = map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    T = zm.ZbManagerTerms
    assert (size, o_off, o_pt, o_wf) == (C.sizeof(T), T.gait_offset.offset, T.clearance_point.offset, T.which_forward.offset)
    assert (sd, gd) == (zm.MT_STATE_DIM, zm.MT_GET_DIM)
    assert zm.MT["EP_SUMS"] + len(zm.M_EXTRA_REWARD_TERMS) == zm.MT_STATE_DIM


def test_library_exports_and_refuses_without_a_handle():
    from zbot_lab_amd import _native, build
    out = subprocess.run(["nm", "-D", "--defined-only", build.build()], capture_output=True, text=True, check=True).stdout
    for s in _native.EXPORTED_MANAGER_TERMS:
        assert f" T {s}\n" in out, s
    L = _native.lib()
    t = zm.ManagerTerms().pack(zm.load_v09_model())
    assert L.zb_set_manager_terms(None, C.byref(t), None) < 0 and b"zb_set_manager_terms" in L.zb_last_error()
    assert L.zb_manager_terms_active(None) == 0 and L.zb_kernel_variant_name(None) is None


def test_train_flags():
    train = _train()
    args = train.build_parser().parse_args(["--task", "zbot-6b-walking-m-v0", "--reward", "gait=0.5", "--reward",
                                            "feet_air_time=1.25", "--reward", "feet_slide=-3", "--no_reward", "foot_forward"])
    assert args.reward == ["gait=0.5", "feet_air_time=1.25", "feet_slide=-3"] and args.no_reward == ["foot_forward"]
    cfg = _cfg()
    train.apply_manager_rewards(cfg, args)
    assert cfg.rewards.foot_forward is None and cfg.rewards.feet_slide.weight == -3.0
    assert cfg.rewards.gait == base_reward_term("gait")           # a restored term takes the base cfg's params
    assert cfg.rewards.feet_air_time.weight == 1.25 and cfg.rewards.feet_air_time.params == base_reward_term("feet_air_time").params
    cfg.task_cfg()
    assert cfg.manager_terms().weights == {"gait": 0.5, "feet_air_time": 1.25}
    for flags in (["--reward", "gait"], ["--reward", "gait=x"], ["--reward", "nope=1"], ["--no_reward", "nope"],
                  ["--reward", "undesired_contacts=-1"]):
        with pytest.raises(SystemExit):
            train.apply_manager_rewards(_cfg(), train.build_parser().parse_args(["--task", "zbot-6b-walking-m-v0"] + flags))
    v2 = zbot_lab_amd.tasks.load_cfg("zbot-6b-walking-v2")
    with pytest.raises(SystemExit):
        train.apply_manager_rewards(v2, train.build_parser().parse_args(["--task", "zbot-6b-walking-v2", "--reward", "gait=1"]))
    train.apply_manager_rewards(v2, train.build_parser().parse_args(["--task", "zbot-6b-walking-v2"]))  # no flag: untouched
