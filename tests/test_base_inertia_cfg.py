"""Manager env: the startup events events.add_base_mass / events.base_com (include/zbot_base_inertia.h).
The host statement of the composite body (model.with_base_inertia) against load_model on a hand-edited
asset; the cfg forms that compile and the ones that raise; the laws of the startup draws; and the f64
oracle on a modified model (contact-free), whose difference D from the nominal model the GPU test
relies on. No GPU."""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

import zbot_lab_amd
from zbot_lab_amd import model as zm
from zbot_lab_amd.envs import manager_flat as mf
from zbot_lab_amd.envs.manager_flat import EventTerm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAVY = (0.2504 + 0.2, (0.03, -0.03, 0.01))   # +0.2 kg, COM moved (m, link frame)
S = zm.S


def _cfg():
    return zbot_lab_amd.tasks.load_cfg("zbot-6b-walking-m-v0")


def _mass(lo=0.0, hi=0.3, op="add", **kw):
    return EventTerm("randomize_rigid_body_mass", "startup", {"mass_distribution_params": (lo, hi), "operation": op, **kw})


def _com(**kw):
    return EventTerm("randomize_rigid_body_com", "startup",
                     {"com_range": {"x": (-0.03, 0.03), "y": (-0.02, 0.02), "z": (-0.01, 0.01)}, **kw})


# ------------------------------------------------------------------ the composite
def _edited_asset(tmp_path, mass, offset, recompute):
    """load_model on a copy of the v09 asset whose 'base' entry was edited by hand."""
    raw = json.load(open(zm.V09_ASSET))
    base = next(l for l in raw["links"] if l["name"] == "base")
    if recompute:
        base["diag_inertia"] = [v * mass / base["mass"] for v in base["diag_inertia"]]
    base["mass"] = mass
    base["com"] = [c + o for c, o in zip(base["com"], offset)]
    path = tmp_path / "edited.json"
    path.write_text(json.dumps(raw))
    return zm.load_model(str(path))


@pytest.mark.parametrize("recompute", [True, False])
@pytest.mark.parametrize("mass,offset", [HEAVY, (0.11, (-0.02, 0.04, 0.0)), (0.2504, (0.0, 0.0, 0.02))])
def test_composite_equals_load_model_on_an_edited_asset(tmp_path, mass, offset, recompute):
    rm = zm.load_v09_model()
    a = zm.with_base_inertia(rm, mass, offset, recompute)
    b = _edited_asset(tmp_path, mass, offset, recompute)
    scale = {"body_mass": 1.0, "body_com": np.abs(b.body_com).max(), "body_inertia": np.abs(b.body_inertia).max(),
             "link_com": np.abs(b.link_com).max()}
    for f in dataclasses.fields(rm):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if f.name in scale:
            x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
            assert x.dtype == np.float64
            assert np.abs(x - y).max() <= 1e-12 * max(scale[f.name], np.abs(y).max()), f.name
    # only the four named fields differ from the nominal model, and there only the base body / link
    bb = rm.link_body[rm.base_link]
    other_b = [k for k in range(zm.NUM_BODIES) if k != bb]
    other_l = [k for k in range(zm.NUM_LINKS) if k != rm.base_link]
    for f in dataclasses.fields(rm):
        x, y = getattr(a, f.name), getattr(rm, f.name)
        if f.name in ("body_mass", "body_com", "body_inertia"):
            np.testing.assert_array_equal(np.asarray(x)[other_b], np.asarray(y)[other_b])
        elif f.name == "link_com":
            np.testing.assert_array_equal(x[other_l], y[other_l])
        elif isinstance(y, np.ndarray):
            np.testing.assert_array_equal(x, y)
        else:
            assert x is y or x == y, f.name
    assert bytes(zm.pack_model(a)) != bytes(zm.pack_model(rm))


def test_nominal_arguments_reproduce_the_model():
    rm = zm.load_v09_model()
    link = zm.pack_base_link(rm)
    assert rm.link_names[rm.base_link] == "base" and rm.link_body[rm.base_link] == 3
    assert link.mass == pytest.approx(0.2504, abs=1e-4) and link.rest_mass == pytest.approx(0.2504, abs=1e-4)
    for rec in (True, False):
        a = zm.with_base_inertia(rm, link.mass, (0.0, 0.0, 0.0), rec)
        assert bytes(zm.pack_model(a)) == bytes(zm.pack_model(rm))
        for f in ("body_mass", "body_com", "body_inertia", "link_com"):
            np.testing.assert_array_equal(getattr(a, f), getattr(rm, f))
    # the refactored load_model itself: the other asset too, against its committed packed form's source
    np.testing.assert_allclose(zm.load_model().body_mass.sum(), sum(l["mass"] for l in zm.load_model().raw["links"]), rtol=1e-15)


@pytest.mark.parametrize("bad", [0.0, -0.75, float("nan"), float("inf")])
def test_non_positive_mass_is_refused_by_name(bad):
    with pytest.raises(ValueError, match="mass"):
        zm.with_base_inertia(zm.load_v09_model(), bad, (0.0, 0.0, 0.0))


def test_base_link_struct_has_the_c_layout(tmp_path):
    import subprocess
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "zbot.h"\nint main(){printf("%zu %zu %zu\\n", sizeof(zb_base_link), '
                   'offsetof(zb_base_link, inertia), offsetof(zb_base_link, rest_com));}\n')
    exe = tmp_path / "s"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(zm.ZbBaseLink), zm.ZbBaseLink.inertia.offset, zm.ZbBaseLink.rest_com.offset]


# ------------------------------------------------------------------ cfg compilation
def test_unedited_cfg_is_off():
    cfg = _cfg()
    assert not cfg.base_inertia().enabled and cfg.base_inertia() == mf.BaseInertiaEvents()
    assert dataclasses.asdict(cfg.task_cfg()) == dataclasses.asdict(zm.TaskCfg.manager_flat(solver_mode=1))


def test_the_two_events_compile():
    """Fails on the parent: task_cfg() raised NotImplementedError on either event."""
    cfg = _cfg()
    before = dataclasses.asdict(cfg.task_cfg())
    cfg.events.add_base_mass = _mass(-0.1, 0.3, "add", distribution="uniform", recompute_inertia=False)
    cfg.events.base_com = _com()
    assert dataclasses.asdict(cfg.task_cfg()) == before   # TaskCfg / zb_task_cfg carry none of it
    dr = cfg.base_inertia()
    assert dr.enabled and dr.mass_enabled and dr.com_enabled
    assert dr.mass_range == (-0.1, 0.3) and dr.mass_operation == "add" and dr.recompute_inertia is False
    assert dr.com_range == ((-0.03, 0.03), (-0.02, 0.02), (-0.01, 0.01))
    for op, rng in (("scale", (0.5, 1.5)), ("abs", (0.1, 0.4))):
        cfg.events.add_base_mass = _mass(*rng, op)
        cfg.events.base_com = None
        dr = cfg.base_inertia()
        assert dr.mass_operation == op and dr.recompute_inertia is True and not dr.com_enabled
        cfg.task_cfg()
    cfg.events.add_base_mass = _mass(asset_cfg="robot:base")
    cfg.events.base_com = EventTerm("randomize_rigid_body_com", "startup", {"com_range": {"x": (-0.01, 0.01)}})
    assert cfg.base_inertia().com_range == ((-0.01, 0.01), (0.0, 0.0), (0.0, 0.0))


@pytest.mark.parametrize("which,term", [
    ("add_base_mass", _mass(asset_cfg="robot:foot.*")),
    ("add_base_mass", _mass(distribution="log_uniform")),
    ("add_base_mass", _mass(distribution="gaussian")),
    ("add_base_mass", EventTerm("randomize_rigid_body_mass", "reset", _mass().params)),
    ("add_base_mass", _mass(op="multiply")),
    ("add_base_mass", _mass(buckets=4)),
    ("add_base_mass", EventTerm("randomize_rigid_body_material", "startup", _mass().params)),
    ("base_com", _com(asset_cfg="robot:a7")),
    ("base_com", EventTerm("randomize_rigid_body_com", "interval", _com().params)),
    ("base_com", _com(distribution="uniform")),
    ("base_com", EventTerm("randomize_rigid_body_com", "startup", {"com_range": {"roll": (0.0, 0.1)}})),
])
def test_refused_forms_say_what_is_compiled(which, term):
    cfg = _cfg()
    setattr(cfg.events, which, term)
    with pytest.raises(NotImplementedError, match="randomize_rigid_body_mass.*randomize_rigid_body_com"):
        cfg.task_cfg()


def test_the_reference_range_is_refused_not_simulated():
    cfg = _cfg()
    cfg.events.add_base_mass = _mass(-1.0, 3.0, "add")   # the reference's own range, on a 0.25 kg link
    with pytest.raises(ValueError, match=r"-0\.7496 kg"):
        cfg.task_cfg()
    cfg.events.add_base_mass = _mass(0.0, 2.0, "scale")
    with pytest.raises(ValueError, match="positive mass"):
        cfg.base_inertia()


def test_train_flags_reach_the_cfg():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import train
    args = train.build_parser().parse_args(["--task", "zbot-6b-walking-m-v0", "--add_base_mass", "-0.1", "0.3",
                                            "--base_mass_op", "add", "--base_com", "0.03", "0.02", "0.01"])
    cfg = _cfg()
    train.apply_base_inertia(cfg, args)
    dr = cfg.base_inertia()
    assert dr.mass_range == (-0.1, 0.3) and dr.com_range == ((-0.03, 0.03), (-0.02, 0.02), (-0.01, 0.01))
    v2 = zbot_lab_amd.tasks.load_cfg("zbot-6b-walking-v2")
    with pytest.raises(SystemExit):
        train.apply_base_inertia(v2, train.build_parser().parse_args(["--task", "zbot-6b-walking-v2", "--base_com", "0", "0", "0.01"]))
    train.apply_base_inertia(v2, train.build_parser().parse_args(["--task", "zbot-6b-walking-v2"]))  # no flag: untouched


# ------------------------------------------------------------------ the startup draws
def _friction_draws(cfg, n):
    """EventCfg.physics_material as ZbotManagerBasedRLEnv._startup draws it (the env's own generator)."""
    import torch
    p = cfg.events.physics_material.params
    g = torch.Generator().manual_seed(cfg.seed if cfg.seed is not None else 0)
    ranges = torch.tensor([p["static_friction_range"], p["dynamic_friction_range"], p["restitution_range"]])
    nb = int(p["num_buckets"])
    buckets = torch.rand(nb, 3, generator=g) * (ranges[:, 1] - ranges[:, 0]) + ranges[:, 0]
    return buckets[torch.randint(0, nb, (n, zm.NUM_LINKS), generator=g)].numpy()


def test_draw_laws():
    from random_laws import Laws
    n = 65536
    cfg = _cfg()
    cfg.seed = 7
    cfg.events.add_base_mass = _mass(-0.1, 0.3, "add")
    cfg.events.base_com = _com()
    dr = cfg.base_inertia()
    mass, com = (t.numpy().astype(np.float64) for t in mf.draw_base_inertia(dr, n, cfg.seed))
    m0 = mf.base_link_mass()
    assert mass.shape == (n,) and com.shape == (n, 3) and mass.min() > 0.0
    eps = float(np.finfo(np.float32).eps)
    L = Laws()
    L.uniform("mass sample", mass - m0, -0.1, 0.3, slack=eps)   # (rounded to fp32 once: a range end within 1 ulp)
    for k, (ax, (lo, hi)) in enumerate(zip("xyz", dr.com_range)):
        L.uniform(f"com {ax}", com[:, k], lo, hi, slack=eps * hi)
    fr = _friction_draws(cfg, n)
    L.uncorrelated("columns", {"mass": mass, "com x": com[:, 0], "com y": com[:, 1], "com z": com[:, 2],
                               "friction": fr[:, 0, 0]})
    L.serial("mass", mass)
    L.check("startup base mass / COM draws, 65 536 envs")
    # scale / abs go through the operation
    for op, rng in (("scale", (0.5, 1.5)), ("abs", (0.1, 0.4))):
        cfg.events.add_base_mass = _mass(*rng, op)
        m2 = mf.draw_base_inertia(cfg.base_inertia(), 4096, cfg.seed)[0].numpy().astype(np.float64)
        s = m2 / m0 if op == "scale" else m2
        assert rng[0] - 1e-6 <= s.min() and s.max() <= rng[1] + 1e-6 and s.std() > 0.2 * (rng[1] - rng[0])
    # another seed: other draws; a disabled event leaves its default
    cfg.events.add_base_mass = None
    m3, c3 = mf.draw_base_inertia(cfg.base_inertia(), 256, 8)
    assert (m3.numpy() == np.float32(m0)).all() and not np.array_equal(c3.numpy(), com[:256].astype(np.float32))


def test_friction_draws_do_not_move():
    """The events draw from a generator of their own: the env's friction draws of one seed are the same
    values with the events on and off (the env's _startup, restated in _friction_draws, seeds its
    generator from cfg.seed alone and draw_base_inertia never touches it)."""
    import inspect
    import torch
    src = inspect.getsource(mf.ZbotManagerBasedRLEnv._startup)
    assert "manual_seed(self.cfg.seed if self.cfg.seed is not None else 0)" in src
    cfg = _cfg()
    cfg.seed = 3
    before = _friction_draws(cfg, 512)
    state = torch.random.get_rng_state()
    cfg.events.add_base_mass, cfg.events.base_com = _mass(), _com()
    mf.draw_base_inertia(cfg.base_inertia(), 512, cfg.seed)
    assert torch.equal(state, torch.random.get_rng_state())   # nor the global generator
    np.testing.assert_array_equal(before, _friction_draws(cfg, 512))
    assert (cfg.seed ^ mf.BASE_INERTIA_SEED_SALT) != cfg.seed


# ------------------------------------------------------------------ the new stamp's code-object budget
def test_dr_step_kernel_budget(tmp_path):
    """zb_m_dr_step_kernel<kTgs, kOcc> keeps the manager kernel's budget (registers, LDS, scratch from the
    code object's metadata, as tests/test_kernel_resources.py reads it): kOcc = 2 at most 256 VGPR + AGPR,
    64 B of scratch and 20 KB of LDS; kOcc = 1 no scratch."""
    import re
    import test_kernel_resources as K
    found = 0
    for name, md in K._kernel_metadata(tmp_path).items():
        if "19zb_m_dr_step_kernel" not in name:
            continue
        found += 1
        occ = int(re.search(r"ILb[01]ELi([12])EE", name).group(1))
        regs, lds, scratch = md["vgpr_count"], md["group_segment_fixed_size"], md.get("private_segment_fixed_size", 0)
        print(f"{name[18:48]}: {regs} regs, {lds} B LDS, {scratch} B scratch")
        assert lds <= 20 * 1024
        if occ == 1:
            assert regs <= 512 and scratch == 0
        else:
            assert regs <= 256 and scratch <= 64
    assert found == 4


# ------------------------------------------------------------------ the oracle on a modified model
def lifted_scenario(n=8, lift=1.0):
    """Default-pose manager states lifted by `lift` m (no contact), with offset joint targets."""
    rm = zm.load_v09_model()
    st = zm.default_state(n, rm)
    full = np.zeros((zm.M_STATE_DIM, n), np.float32)
    full[:S["P_DELTA"]] = st[:S["P_DELTA"]]   # the physics rows; the MDP rows play no part in the substeps
    full[S["ROOT_POS"] + 2] += lift
    full[zm.M["LINK_MU"]:zm.M["LINK_MU_D"] + zm.NUM_LINKS] = 0.8
    # eight target rows, repeated over the envs: none of them folds the chain into itself within the ten
    # substeps (a self contact would put the solver's discontinuities into a rounding comparison)
    rng = np.random.default_rng(5)
    rows = rm.default_joint_pos[None, :] + 0.3 * rng.uniform(-1.0, 1.0, (8, zm.NUM_DOF))
    targets = rows[np.arange(n) % 8].astype(np.float32)
    return full, targets


def oracle_substeps(rm, st, targets, nsub=10, double=True):
    """`nsub` physics substeps of the oracle built on `rm`; the physics rows after them."""
    from oracle import pyoracle
    lib = pyoracle.lib(double)
    cfg = zm.TaskCfg.manager_flat(solver_mode=1, self_manifold=2)
    m, c = zm.pack_model(rm), cfg.pack()
    n = st.shape[1]
    h = lib.zbo_create(C.byref(m), C.byref(c), n, 0)
    try:
        lib.zbo_set_state(h, np.ascontiguousarray(st, np.float32))
        lib.zbo_physics_substeps(h, np.ascontiguousarray(targets, np.float32), nsub, None, None)
        out = np.zeros((zm.M_STATE_DIM, n), np.float32)
        lib.zbo_get_state(h, out)
    finally:
        lib.zbo_destroy(h)
    return out[:S["P_DELTA"]]


def test_oracle_moves_differently_on_the_modified_model():
    rm = zm.load_v09_model()
    st, tg = lifted_scenario()
    nominal = oracle_substeps(rm, st, tg)
    heavy = oracle_substeps(zm.with_base_inertia(rm, *HEAVY), st, tg)
    assert np.isfinite(heavy).all()
    assert heavy[S["ROOT_POS"] + 2].min() > 0.9   # still in the air: contact-free
    D = float(np.abs(heavy - nominal).max())
    f32 = oracle_substeps(zm.with_base_inertia(rm, *HEAVY), st, tg, double=False)
    e32 = float(np.abs(f32.astype(np.float64) - heavy).max())
    print(f"\nD = {D:.4g} (max abs over the physics rows, nominal vs +0.2 kg / (0.03, -0.03, 0.01) m, 10 substeps); "
          f"f32 oracle vs f64 oracle on the modified model {e32:.3g}; D / (3 e32) = {D / (3 * e32):.3g}")
    assert D > 1e-2 and 3.0 * e32 < D / 100.0
