"""Manager env: events.push_robot, ranges.ang_vel_z and heading_command compile from the cfg to the
zb_manager_events struct (include/zbot_manager_events.h); the forms that are not compiled raise; the
unedited cfg is "events off" with an unchanged TaskCfg; the ctypes mirror has the C layout. No GPU."""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
import subprocess
import tempfile

import pytest

import zbot_lab_amd
from zbot_lab_amd import model as zm
from zbot_lab_amd.envs.manager_flat import EventTerm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    return zbot_lab_amd.tasks.load_cfg("zbot-6b-walking-m-v0")


def _push(**kw):
    a = dict(func="push_by_setting_velocity", mode="interval",
             params={"velocity_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5)}}, interval_range_s=(10.0, 15.0))
    a.update(kw)
    return EventTerm(a["func"], a["mode"], a["params"], interval_range_s=a["interval_range_s"])


def test_unedited_cfg_is_events_off():
    cfg = _cfg()
    ev = cfg.manager_events()
    assert not ev.enabled and ev == zm.ManagerEvents()
    assert dataclasses.asdict(cfg.task_cfg()) == dataclasses.asdict(zm.TaskCfg.manager_flat(solver_mode=1))
    assert bytes(ev.pack())[:4] == b"\0\0\0\0" and ev.pack().heading_command == 0
    play = zbot_lab_amd.tasks.load_cfg("zbot-6b-walking-m-play-v0")
    assert not play.manager_events().enabled


def test_cfg_edits_compile_to_the_struct():
    cfg = _cfg()
    before = dataclasses.asdict(cfg.task_cfg())
    cfg.events.push_robot = _push(params={"velocity_range": {"x": (-0.5, 0.5), "y": (-0.25, 0.5), "yaw": (-0.1, 0.2)}})
    cmd = cfg.commands.base_velocity
    cmd.ranges.ang_vel_z = cmd.limit_ranges.ang_vel_z = (-1.0, 0.5)
    cmd.heading_command = True
    cmd.ranges.heading = (-math.pi, math.pi)
    cmd.rel_heading_envs = 0.5
    cmd.heading_control_stiffness = 0.75
    assert dataclasses.asdict(cfg.task_cfg()) == before  # TaskCfg / zb_task_cfg carry none of it
    ev = cfg.manager_events()
    assert ev.enabled
    e = ev.pack()
    assert e.push_enabled == 1 and list(e.push_interval_s) == [10.0, 15.0]
    rows = [list(r) for r in e.push_velocity_range]
    assert rows == [[-0.5, 0.5], [-0.25, 0.5], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0],
                    [pytest.approx(-0.1), pytest.approx(0.2)]]
    assert list(e.cmd_ang_vel_z) == [-1.0, 0.5] and e.heading_command == 1
    assert list(e.cmd_heading) == [pytest.approx(-math.pi), pytest.approx(math.pi)]
    assert e.cmd_rel_heading == 0.5 and e.heading_stiffness == 0.75
    # each on its own
    c = _cfg()
    c.commands.base_velocity.ranges.ang_vel_z = c.commands.base_velocity.limit_ranges.ang_vel_z = (-0.5, 0.5)
    ev = c.manager_events()
    assert ev.enabled and not ev.push_enabled and not ev.heading_command and ev.cmd_ang_vel_z == (-0.5, 0.5)
    c = _cfg()
    c.events.push_robot = _push()
    ev = c.manager_events()
    assert ev.enabled and ev.push_enabled and ev.cmd_ang_vel_z == (0.0, 0.0) and ev.heading_stiffness == 1.0


@pytest.mark.parametrize("edit", [
    lambda c: setattr(c.events, "push_robot", _push(interval_range_s=None)),
    lambda c: setattr(c.events, "push_robot", EventTerm("push_by_setting_velocity", "interval")),
    lambda c: setattr(c.events, "push_robot", _push(func="apply_external_force_torque")),
    lambda c: setattr(c.events, "push_robot", _push(mode="reset")),
    lambda c: setattr(c.events, "push_robot", _push(interval_range_s=(0.0, 5.0))),
    lambda c: setattr(c.events, "push_robot", _push(interval_range_s=(6.0, 5.0))),
    lambda c: setattr(c.events, "push_robot", _push(params={"velocity_range": {"x": (0.5, -0.5)}})),
    lambda c: setattr(c.events, "push_robot", _push(params={"velocity_range": {"forward": (0.0, 0.5)}})),
    lambda c: setattr(c.commands.base_velocity, "heading_command", True),
    lambda c: setattr(c.commands.base_velocity.ranges, "ang_vel_z", (-0.5, 0.5)),
    lambda c: setattr(c.commands.base_velocity.limit_ranges, "ang_vel_z", (-0.5, 0.5)),
    lambda c: setattr(c.events, "add_base_mass", EventTerm("randomize_rigid_body_mass", "startup")),
    lambda c: setattr(c.events, "base_com", EventTerm("randomize_rigid_body_com", "startup")),
], ids=["no_interval", "no_params", "other_func", "other_mode", "interval_lo_0", "interval_hi_lt_lo", "range_hi_lt_lo",
        "unknown_axis", "heading_without_range", "ranges_ne_limit", "limit_ne_ranges", "add_base_mass", "base_com"])
def test_malformed_variants_raise(edit):
    c = _cfg()
    edit(c)
    with pytest.raises(NotImplementedError):
        c.task_cfg()


def test_ctypes_mirror_matches_the_header():
    """sizeof and every field offset of zb_manager_events (compiled probe), and the state-row enum."""
    names = [n for n, _ in zm.ZbManagerEvents._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "zbot.h"\nint main(){printf("%zu", sizeof(zb_manager_events));\n'
           + "".join(f'printf(" %zu", offsetof(zb_manager_events, {n}));\n' for n in names)
           + 'printf(" %d %d %d %d\\n", ZB_ME_PUSH_TIME_LEFT, ZB_ME_HEADING_TARGET, ZB_ME_IS_HEADING, ZB_ME_STATE_DIM);}\n')
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "p")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        v = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    assert v[0] == C.sizeof(zm.ZbManagerEvents)
    assert v[1:1 + len(names)] == [getattr(zm.ZbManagerEvents, n).offset for n in names]
    assert v[1 + len(names):] == [zm.ME["PUSH_TIME_LEFT"], zm.ME["HEADING_TARGET"], zm.ME["IS_HEADING"], zm.ME_STATE_DIM]


def test_library_exports_and_refuses_without_a_handle():
    from zbot_lab_amd import _native, build
    path = build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    for s in _native.EXPORTED_MANAGER_EVENTS:
        assert f" T {s}\n" in out, s
    L = _native.lib()
    ev = zm.ManagerEvents().pack()
    assert L.zb_set_manager_events(None, C.byref(ev), None) < 0 and b"zb_set_manager_events" in L.zb_last_error()
    assert L.zb_manager_events_active(None) == 0 and L.zb_manager_event_state_dim(None) == -1


def test_train_flags():
    import importlib.util
    spec = importlib.util.spec_from_file_location("zbot_train_script", os.path.join(ROOT, "scripts", "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    args = train.build_parser().parse_args(["--task", "zbot-6b-walking-m-v0", "--push_robot", "--ang_vel_z", "-0.5", "0.5",
                                            "--heading_command"])
    cfg = _cfg()
    train.apply_manager_events(cfg, args)
    ev = cfg.manager_events()
    assert ev.push_enabled and ev.push_interval_s == (10.0, 15.0)
    assert ev.push_velocity_range[:2] == ((-0.5, 0.5), (-0.5, 0.5)) and ev.push_velocity_range[2:] == ((0.0, 0.0),) * 4
    assert ev.cmd_ang_vel_z == (-0.5, 0.5) and ev.heading_command and ev.cmd_heading == (-math.pi, math.pi)
    v2 = zbot_lab_amd.tasks.load_cfg("zbot-6b-walking-v2")
    for flags in (["--push_robot"], ["--ang_vel_z", "0", "1"], ["--heading_command"]):
        with pytest.raises(SystemExit):
            train.apply_manager_events(v2, train.build_parser().parse_args(["--task", "zbot-6b-walking-v2"] + flags))
    train.apply_manager_events(v2, train.build_parser().parse_args(["--task", "zbot-6b-walking-v2"]))  # no flag: untouched
