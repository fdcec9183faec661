"""Privileged critic observations of libzbot.so (include/zbot_critic_obs.h) through the C ABI: the row
of every task after ~30 seeded random-action steps (contacts, velocities, auto-resets; stand-up and
the manager task with per-env friction), at 64, 67 (a partial wave and a partial row block) and 1 env.

Policy block: bit-identical to zb_observe for walking v2, v4 and stand-up; for the manager task the
noisy observation minus the block lies within each term's noise half-width (plus the fp32 rounding of
the sum, eps32 |noisy|, and of the half-width itself), the noise-free terms are bit-equal, and some term
differs.

Tail: restated in numpy from zb_get_state, the packed model and the friction that was set, once in
float64 and once in float32 (the same statements). Per term (column) the kernel's err = max |x - x64|
must satisfy err <= max(4 e32, 2 eps32 max |x64|) with e32 = max |x32 - x64|: the rule of
tests/test_gpu_ppo_shapes.py (both sides are fp32 evaluations of one formula in different operation
orders; the floor covers terms numpy happens to round exactly). Every run prints the worst err / e32
per task (pytest -s).

Measured on an MI355X, worst err / e32 over the terms above the floor, per task (all three sizes):
walking v2 0.97 (vz), stand-up 1.67 (vy), walking v4 1.85 (vz), manager 1.42 (vz); the manager's noise
reaches 0.99 of its half-width. The whole file takes 3 s.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from zbot_lab_amd import model as zm

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
TAIL = 7
TASKS = {
    "v2": lambda: zm.TaskCfg(solver_mode=1, self_manifold=3),
    "standup": lambda: zm.TaskCfg.standup(),
    "v4": lambda: zm.TaskCfg.walking_v4(),
    "manager": lambda: zm.TaskCfg.manager_flat(),
}
# state rows: the feet's newest vertical force (None: not in the state), the per-link friction (None: uniform)
FZ_ROW = {"v2": zm.S["FEET_FZ_HIST"], "standup": None, "v4": zm.V4["FEET_FZ_HIST"], "manager": zm.M["FEET_FZ_HIST"]}
MU_ROW = {"v2": None, "standup": zm.SU["LINK_MU"], "v4": None, "manager": zm.M["LINK_MU"]}
EP_ROW = {"v2": zm.S["EP_LEN"], "standup": zm.SU["EP_LEN"], "v4": zm.V4["EP_LEN"], "manager": zm.M["EP_LEN"]}


def _sim(task, n, seed=0):
    from zbot_lab_amd.sim import ZbotSim
    return ZbotSim(n, TASKS[task](), device="cuda:0", seed=seed)


def _friction(n, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (0.3 + 0.7 * torch.rand(n, zm.NUM_LINKS, generator=g)).cuda()


def _rollout(task, n, seed=0, steps=30):
    """(sim, mu or None) after `steps` seeded random-action steps."""
    import torch
    sim = _sim(task, n, seed)
    mu = None
    if MU_ROW[task] is not None:
        mu = _friction(n, seed + 1)
        sim.set_link_friction(mu)
    sim.reset(None)
    g = torch.Generator().manual_seed(seed + 2)
    for _ in range(steps):
        sim.step(torch.randn(n, zm.ACT_DIM, generator=g).cuda())
    return sim, mu


@functools.lru_cache(maxsize=None)
def _case(task, n):
    """The compared arrays of one (task, size), computed once: state, rows, zb_observe, friction."""
    import torch
    sim, mu = _rollout(task, n)
    st, rows, obs = sim.get_state(), sim.observe_critic(), sim.observe()
    torch.cuda.synchronize()
    out = dict(st=st.cpu().numpy(), rows=rows.cpu().numpy(), obs=obs.cpu().numpy(),
               mu=None if mu is None else mu.cpu().numpy(), dim=sim.critic_obs_dim, P=sim.obs_dim,
               model=sim._m, cfg=sim._c)
    sim.close()
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------ the tail in numpy, float64 / float32
def _qmul(a, b):
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def _qmat(q):
    w, x, y, z = (q[..., k] for k in range(4))
    one, two = q.dtype.type(1), q.dtype.type(2)
    return np.stack([np.stack([one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)], -1),
                     np.stack([two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)], -1),
                     np.stack([two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)], -1)], -2)


def _qnormalize(q):
    return q * (q.dtype.type(1) / np.sqrt((q * q).sum(-1, keepdims=True)))


def _mv(R, v):
    return (R * v[..., None, :]).sum(-1)


def tail_numpy(task, case, dt):
    """The seven tail terms [N, 7] of include/zbot_critic_obs.h from the state, in dtype dt: forward
    kinematics to the base link's composite body (3: joints 0..2), its twist, the link origin's velocity
    rotated into the link frame, its height, the feet loads over the weight, the feet's friction."""
    m, c = case["model"], case["cfg"]
    arr = lambda a: np.ctypeslib.as_array(a).astype(dt)
    st = case["st"].astype(dt)
    S = zm.S
    pos, quat = st[S["ROOT_POS"]:S["ROOT_POS"] + 3].T, st[S["ROOT_QUAT"]:S["ROOT_QUAT"] + 4].T
    lv, av = st[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3].T, st[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3].T
    jq, jqd = st[S["JOINT_POS"]:S["JOINT_POS"] + 6].T, st[S["JOINT_VEL"]:S["JOINT_VEL"] + 6].T
    jpr, jpp, jcp, jcr = arr(m.joint_parent_rot), arr(m.joint_parent_pos), arr(m.joint_child_pos), arr(m.joint_child_rot)
    q = _qnormalize(quat)
    R = _qmat(q)
    p = np.zeros_like(pos)
    w, v = av, lv
    bl = int(m.base_link)
    for j in range((bl + 1) // 2):
        qj = _qmul(q, jpr[j])
        org = p + _mv(R, jpp[j])
        ax = _qmat(qj)[..., :, 2]
        half = dt(0.5) * jq[:, j]
        qz = np.stack([np.cos(half), np.zeros_like(half), np.zeros_like(half), np.sin(half)], -1)
        qa = _qmul(qj, qz)
        p = org + _mv(_qmat(qa), jcp[j])
        q = _qnormalize(_qmul(qa, jcr[j]))
        R = _qmat(q)
        w = w + ax * jqd[:, j:j + 1]
        v = v + np.cross(org, ax) * jqd[:, j:j + 1]
    bp = p + _mv(R, arr(m.link_pos)[bl])
    bq = _qmul(q, arr(m.link_rot)[bl])
    vw = v + np.cross(w, bp)
    Rb = _qmat(bq)
    out = np.zeros((st.shape[1], TAIL), dt)
    out[:, 0:3] = (Rb * vw[..., :, None]).sum(-2)  # R^T v
    out[:, 3] = pos[:, 2] + bp[:, 2]
    if FZ_ROW[task] is not None:
        weight = arr(m.body_mass).sum() * dt(c.gravity)
        out[:, 4:6] = st[FZ_ROW[task]:FZ_ROW[task] + 2].T / weight
    if MU_ROW[task] is None:
        out[:, 6] = dt(c.friction)
    else:
        mu = case["mu"].astype(dt)
        out[:, 6] = dt(0.5) * (mu[:, m.foot_links[0]] + mu[:, m.foot_links[1]])
    return out


SIZES = [64, 67, 1]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("task", list(TASKS))
def test_row_shape_and_dim(gpu, task, n):
    c = _case(task, n)
    assert c["dim"] == c["P"] + TAIL <= 32
    assert c["rows"].shape == (n, c["dim"]) and np.isfinite(c["rows"]).all()
    if n > 1:  # the trajectory the tests below rely on: motion, contacts (where the state has them)
        assert np.abs(c["rows"][:, c["P"]:c["P"] + 3]).max() > 1e-3
        if FZ_ROW[task] is not None:
            assert c["rows"][:, c["P"] + 4:c["P"] + 6].max() > 0.05


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("task", ["v2", "standup", "v4"])
def test_policy_block_is_zb_observe(gpu, task, n):
    c = _case(task, n)
    assert np.array_equal(c["rows"][:, :c["P"]].view(np.uint32), c["obs"].view(np.uint32))


@pytest.mark.parametrize("n", SIZES)
def test_manager_policy_block_is_the_noise_free_observation(gpu, n):
    c = _case("manager", n)
    clean, noisy = c["rows"][:, :c["P"]].astype(np.float64), c["obs"].astype(np.float64)
    nq, njp, njv = (float(x) for x in c["cfg"].obs_noise)
    hw = np.array([nq] * 4 + [0.0] * 3 + [njp] * 6 + [njv] * 6 + [0.0] * 6)
    d = np.abs(noisy - clean)
    print(f"\n[manager {n}] max |noisy - clean| / half-width per group: quat {d[:, :4].max() / nq:.3f}, "
          f"joint pos {d[:, 7:13].max() / njp:.3f}, joint vel {d[:, 13:19].max() / njv:.3f}")
    assert (d <= hw * (1 + 2 * EPS32) + EPS32 * np.abs(noisy)).all()
    assert np.array_equal(c["rows"][:, :c["P"]][:, hw == 0].view(np.uint32), c["obs"][:, hw == 0].view(np.uint32))
    assert (d > 0).any()


@pytest.mark.parametrize("task", list(TASKS))
def test_tail_against_float64(gpu, task):
    fails, worst = [], (0.0, "floor")
    names = ("vx", "vy", "vz", "height", "load foot_0", "load foot_1", "friction")
    for n in SIZES:
        c = _case(task, n)
        x64, x32 = tail_numpy(task, c, np.float64), tail_numpy(task, c, np.float32).astype(np.float64)
        got = c["rows"][:, c["P"]:].astype(np.float64)
        for k, name in enumerate(names):
            err, e32 = np.abs(got[:, k] - x64[:, k]).max(), np.abs(x32[:, k] - x64[:, k]).max()
            floor = 2 * EPS32 * np.abs(x64[:, k]).max()
            if err > floor:
                worst = max(worst, (err / e32 if e32 > 0 else float("inf"), f"{name} at {n} envs: err {err:.3g}, e32 {e32:.3g}"))
            if not err <= max(4 * e32, floor):
                fails.append((n, name, f"err {err:.3g}", f"e32 {e32:.3g}", f"floor {floor:.3g}"))
    print(f"\n[ratio] critic tail {task}: worst err / e32 {worst[0]:.2f} ({worst[1]})")
    assert not fails, fails


def test_standup_tail_has_no_contact_sensor_and_reads_the_friction(gpu):
    c = _case("standup", 67)
    P, m = c["P"], c["model"]
    assert (c["rows"][:, P + 4:P + 6] == 0).all()
    want = np.float32(0.5) * (c["mu"][:, m.foot_links[0]] + c["mu"][:, m.foot_links[1]])
    assert np.array_equal(c["rows"][:, P + 6], want) and np.ptp(want) > 0.05


def _force_time_outs(sim, task):
    """Every third env one step short of its time-out, so the next steps reset some envs for certain."""
    st = sim.get_state()
    wc = sim.get_contact_cache()
    st[EP_ROW[task], ::3] = float(sim.cfg.max_episode_length - 2)
    sim.set_state(st)
    sim.set_contact_cache(wc)


@pytest.mark.parametrize("task", list(TASKS))
def test_registered_buffer_follows_step_and_reset(gpu, task):
    import torch
    n = 67
    sim, _ = _rollout(task, n, steps=5)
    buf = sim.critic_obs_buffer()
    assert buf.shape == (n, sim.critic_obs_dim) and sim.critic_obs_buffer() is buf
    assert torch.equal(buf, sim.observe_critic())
    _force_time_outs(sim, task)
    g = torch.Generator().manual_seed(9)
    resets = 0
    for _ in range(4):
        _, _, term, trunc = sim.step(torch.randn(n, zm.ACT_DIM, generator=g).cuda())
        resets += int((term | trunc).sum())
        after = sim.observe_critic()
        assert torch.equal(buf.view(torch.int32), after.view(torch.int32))
    assert resets > 0
    sim.reset(None)
    assert torch.equal(buf.view(torch.int32), sim.observe_critic().view(torch.int32))
    sim.reset(torch.tensor([0, 5, 66]))
    assert torch.equal(buf.view(torch.int32), sim.observe_critic().view(torch.int32))
    sim.close()


@pytest.mark.parametrize("task", list(TASKS))
def test_off_by_default_changes_nothing(gpu, task):
    """A handle that used the on-demand call and registered, then unregistered, a buffer steps bit-identically
    to one that never saw the new entry points, with the same step-kernel instantiation."""
    import torch
    from zbot_lab_amd import _native as nat
    n = 64
    a, b = _sim(task, n, seed=3), _sim(task, n, seed=3)
    buf = a.critic_obs_buffer()
    a.observe_critic()
    nat.check(a.lib.zb_set_critic_obs_buffer(a._h, None), "zb_set_critic_obs_buffer")
    assert a.kernel_variant() == b.kernel_variant()
    for s in (a, b):
        s.reset(None)
    torch.cuda.synchronize()
    frozen = buf.clone()
    g = torch.Generator().manual_seed(4)
    for _ in range(10):
        act = torch.randn(n, zm.ACT_DIM, generator=g).cuda()
        oa, ra, ta, ua = a.step(act)
        ob, rb, tb, ub = b.step(act)
        assert torch.equal(oa.view(torch.int32), ob.view(torch.int32)) and torch.equal(ra.view(torch.int32), rb.view(torch.int32))
        assert torch.equal(ta, tb) and torch.equal(ua, ub)
    assert torch.equal(a.get_state().view(torch.int32), b.get_state().view(torch.int32))
    assert torch.equal(buf, frozen)  # unregistered: nothing writes it any more
    a.close()
    b.close()


@pytest.mark.parametrize("task", ["v2", "manager"])
def test_rows_are_deterministic(gpu, task):
    import torch
    sim, _ = _rollout(task, 67)
    again = sim.observe_critic()
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy().view(np.uint32), _case(task, 67)["rows"].view(np.uint32))
    sim.close()
