"""Case builder of the limit tests (tests/test_limit_cases.py on the CPU, tests/test_gpu_limits.py on
the device): actions and states that put one step of every task on the clamps the product runs on --
tanh-saturated actions (the staged recipe's noise std grows from 1 to 8.2), p_delta at
+-pi, joint speeds at the actuator's velocity_limit, the root link's angular speed at
max_angular_velocity, joint angles crossing the +-2 pi wrap, the manager's action clip -- and the
measurement that they do (``coverage``, on the f64 oracle). numpy and the oracle only.

The planted families of ``limit_states`` each draw from a generator of their own (seed, family index),
so a family can be planted alone (``families``) without moving the others' draws.
"""
from __future__ import annotations

import numpy as np

from fullstate import base_task, random_states, task_cfg
from zbot_lab_amd import model as zm

F32 = np.float32
FAMILIES = ("p_delta", "joint_vel", "root_omega", "wrap")
# planted shares per family (limit_states); TASK_SHARES holds a task's own
SHARES = dict(p_delta=0.40, joint_vel=0.20, root_omega=0.20, wrap=0.05)
TANH_TASKS = ("v2", "v4", "standup")


# the cases both test files run: 1024 envs, product cfg (fullstate.product), these seeds
N, HANDLE_SEED = 1024, 17
FULL_SEEDS, PROLOGUE_SEEDS = (301, 302), (303, 304)   # (limit_states, limit_actions)
EPS32 = float(np.finfo(F32).eps)
PI32 = F32(np.pi)
_CASES: dict = {}


# the manager's own planted shares: at the common shares its root link is at the angular cap after the step
# in 4.5 % of the surviving envs (condition: 10 %); with these, 21 %. More planted joint speeds also raise
# the count of entries its speed clamp touches in the first substep (test_limit_cases.test_coverage)
TASK_SHARES = {"manager": dict(root_omega=0.9, joint_vel=0.6)}


def _full_inputs(task: str, cfg):
    """limit_states with every family (the task's shares) and limit_actions; the manager without the
    table values whose square overflows."""
    from oracle.pyoracle import OracleSim
    st = limit_states(task, OracleSim(N, cfg, seed=HANDLE_SEED), N, FULL_SEEDS[0], shares=TASK_SHARES.get(base_task(task)))
    return st, limit_actions(N, FULL_SEEDS[1], overflow=base_task(task) != "manager")


def _prologue_inputs(task: str, cfg):
    """Standing random_states with only the p_delta family and limit_actions with the whole table, on
    envs that survive the step: from a pool of 4 N, the first N the f32 oracle does not reset
    (random_states ends 5 % of the episodes by time-out, a third of the stand-up envs by the
    centre-height drop and half of the manager's by feet_close: its reset stance is 0.2 mm off that
    threshold). The table is written after the selection, so up to 40 envs (3.9 %) may still reset;
    check_prologue sets aside at most 5 %."""
    from oracle.pyoracle import OracleSim
    P = 4 * N
    st = limit_states(task, OracleSim(P, cfg, seed=HANDLE_SEED), P, PROLOGUE_SEEDS[0], standing=True, families=("p_delta",))
    a = limit_actions(P, PROLOGUE_SEEDS[1])
    d = OracleSim(P, cfg, seed=HANDLE_SEED)
    d.set_state(st)
    te, tr = d.step(a)[2:]
    ids = np.nonzero(~(te | tr))[0][:N]
    assert len(ids) == N, len(ids)
    return np.ascontiguousarray(st[:, ids]), plant_table(np.ascontiguousarray(a[ids]))


def _build_case(task: str, kind: str) -> dict:
    from fullstate import product
    from oracle.pyoracle import OracleSim
    with product():
        cfg = task_cfg(task)
        st, a = (_full_inputs if kind == "full" else _prologue_inputs)(task, cfg)
        c = dict(st=st, a=a)
        for name, dbl in (("32", False), ("64", True)):
            d = OracleSim(N, cfg, seed=HANDLE_SEED, double=dbl)
            d.set_state(st)
            c["out" + name] = d.step(a)
            c["s" + name] = d.get_state()
        c["pro"] = prologue64(task, d, st, a)
        c["limits"] = (float(d._m.velocity_limit), float(d._m.max_angular_velocity))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def case(task: str, kind: str) -> dict:
    """The inputs of a test (kind "full": _full_inputs, "prologue": _prologue_inputs) and their
    references, built once per (task, kind) and shared read-only:
    ``st``, ``a``: the state before and the actions;
    ``s32`` / ``s64``: the f32 / f64 oracle's state after one step from them;
    ``out32`` / ``out64``: that step's (obs, reward, died, time_out);
    ``pro``: prologue64; ``limits``: (velocity_limit, max_angular_velocity) of the task's model."""
    if (task, kind) not in _CASES:
        _CASES[(task, kind)] = _build_case(task, kind)
    return _CASES[(task, kind)]


def _layout(task: str) -> dict:
    return {"v2": zm.S, "v4": zm.V4, "standup": zm.SU, "manager": zm.M}[base_task(task)]


def action_table() -> np.ndarray:
    """The planted raw actions, float32 [40]: each value with both signs (+0.0 and -0.0 included).
    Zero, the smallest denormal, a denormal, small values where tanh(x) = x to rounding, the polynomial
    range, 8.5, the three floats around atanh(1 - 2^-25) = 9.0109 (where float32 tanh first rounds to
    1), and the kernel's |x| <= 20 clamp from both sides up to FLT_MAX and inf. No NaN."""
    edge = F32(np.arctanh(1.0 - 2.0 ** -25))
    pos = [F32(0.0), np.nextafter(F32(0), F32(1)), F32(1e-40), F32(1e-8), F32(1e-4), F32(0.5), F32(1), F32(4), F32(8.5),
           np.nextafter(edge, F32(0)), edge, np.nextafter(edge, F32(np.inf)),
           F32(10), np.nextafter(F32(20), F32(0)), F32(20), np.nextafter(F32(20), F32(np.inf)), F32(88), F32(1e4),
           np.finfo(F32).max, F32(np.inf)]
    pos = np.array(pos, F32)
    return np.concatenate([pos, -pos])


def limit_actions(n: int, seed: int, overflow: bool = True) -> np.ndarray:
    """[n, 6] float32: 8 N(0, 1) (the trained policy's scale), with action_table() written over the
    first rows of every joint column, each column rotated by 7 rows against its neighbour so that an
    env mixes table values. ``overflow=False`` leaves out the table values whose square overflows
    float32 (FLT_MAX, inf): the manager task stores the raw action, and its action_rate_l2 reward and
    last_action observation are then not finite in the reference either."""
    return plant_table((8.0 * np.random.default_rng(seed).normal(size=(n, 6))).astype(F32), overflow)


def plant_table(a: np.ndarray, overflow: bool = True) -> np.ndarray:
    """action_table() written over the first rows of ``a`` [n, 6] (limit_actions)."""
    tab = action_table()
    k = len(tab)
    assert len(a) >= k
    keep = np.ones(k, bool) if overflow else np.abs(tab) < F32(1e18)
    for j in range(6):
        rows = (np.arange(k) + 7 * j) % k
        a[rows[keep], j] = tab[keep]
    return a


def limit_states(task: str, o, n: int, seed: int, standing: bool = False, families=FAMILIES, shares=None) -> np.ndarray:
    """fullstate.random_states, then the planted limit states (``families``; ``o`` is a fresh OracleSim
    of the task, whose packed model gives the limits):
    * "p_delta": SHARES of the entries at +-(pi - U(0, 0.05)) (the tasks that have the row);
    * "joint_vel": entries at +-U(0.75, 1) velocity_limit;
    * "root_omega": envs whose root link spins about a random axis at U(0.8, 0.997) max_angular_velocity;
    * "wrap": joint angles at +-(2 pi - U(0.005, 0.05)) moving outwards at U(0.75, 1) velocity_limit,
      so the wrap is crossed inside the step."""
    sh = dict(SHARES, **(shares or {}))
    st = random_states(task, o, n, seed, standing=standing)
    D = _layout(task)
    vlim, wmax = float(o._m.velocity_limit), float(o._m.max_angular_velocity)
    gen = lambda fam: np.random.default_rng((seed, FAMILIES.index(fam)))  # noqa: E731
    if "p_delta" in families and "P_DELTA" in D:
        rng = gen("p_delta")
        hit = rng.random((6, n)) < sh["p_delta"]
        val = np.where(rng.random((6, n)) < 0.5, 1.0, -1.0) * (np.pi - rng.uniform(0, 0.05, (6, n)))
        r = slice(D["P_DELTA"], D["P_DELTA"] + 6)
        st[r] = np.where(hit, val, st[r]).astype(F32)
    if "joint_vel" in families:
        rng = gen("joint_vel")
        hit = rng.random((6, n)) < sh["joint_vel"]
        val = np.where(rng.random((6, n)) < 0.5, 1.0, -1.0) * rng.uniform(0.75, 1.0, (6, n)) * vlim
        st[19:25] = np.where(hit, val, st[19:25]).astype(F32)
    if "root_omega" in families:
        rng = gen("root_omega")
        hit = rng.random(n) < sh["root_omega"]
        ax = rng.normal(size=(3, n))
        ax /= np.linalg.norm(ax, axis=0, keepdims=True)
        val = ax * rng.uniform(0.8, 0.997, n) * wmax
        st[10:13] = np.where(hit, val, st[10:13]).astype(F32)
    if "wrap" in families:
        rng = gen("wrap")
        hit = rng.random((6, n)) < sh["wrap"]
        sgn = np.where(rng.random((6, n)) < 0.5, 1.0, -1.0)
        ang = sgn * (2 * np.pi - rng.uniform(0.005, 0.05, (6, n)))
        vel = sgn * rng.uniform(0.75, 1.0, (6, n)) * vlim
        st[13:19] = np.where(hit, ang, st[13:19]).astype(F32)
        st[19:25] = np.where(hit, vel, st[19:25]).astype(F32)
    return st


def prologue64(task: str, o, st: np.ndarray, actions: np.ndarray) -> dict:
    """The fp64 restatement of the step's prologue from the float32 state, actions and packed cfg.
    tanh tasks: ``act`` = tanh(a), ``raw`` = p + pi act joint_speed_limit step_dt (before the clamp),
    ``p_delta`` = clamp(raw, +-pi), ``target`` = p_delta + default_joint_pos, all [6, n]. Manager:
    ``act`` = a (stored raw, Isaac Lab joint order), ``raw`` = a action_scale, ``delta`` = its clip at
    +-action_clip (Isaac Lab order), ``target`` = jq + sign delta[api index] (chain order)."""
    c, m = o._c, o._m
    a = actions.astype(np.float64).T
    if base_task(task) == "manager":
        raw = a * float(c.action_scale)
        delta = np.clip(raw, -float(c.action_clip), float(c.action_clip))
        idx = [int(m.api_joint_index[j]) for j in range(6)]
        sign = np.array([float(m.api_joint_sign[j]) for j in range(6)])[:, None]
        return dict(act=a, raw=raw, delta=delta, lim=float(c.action_clip),
                    target=st[13:19].astype(np.float64) + sign * delta[idx])
    D = _layout(task)
    step_dt = float(F32(c.sim_dt) * F32(c.decimation))
    act = np.tanh(a)
    raw = st[D["P_DELTA"]:D["P_DELTA"] + 6].astype(np.float64) + np.pi * act * float(c.joint_speed_limit) * step_dt
    pd = np.clip(raw, -np.pi, np.pi)
    q0 = np.array([float(m.default_joint_pos[j]) for j in range(6)])[:, None]
    return dict(act=act, raw=raw, p_delta=pd, lim=np.pi, target=pd + q0)


def post_step_coverage(limits, before: np.ndarray, after: np.ndarray, reset: np.ndarray) -> dict:
    """The limit branches a step took, read from its own post-step state (the oracle's or the
    device's), over the envs that did not reset: the share of (env, joint) entries at +-velocity_limit,
    the share of envs at the angular cap, and the number of entries wrapped from beyond +2 pi / -2 pi."""
    vlim, wmax = limits   # (velocity_limit, max_angular_velocity) of the task's model
    alive = ~np.asarray(reset, bool)
    jqd = after[19:25][:, alive].astype(np.float64)
    w = np.linalg.norm(after[10:13][:, alive].astype(np.float64), axis=0)
    dq = (after[13:19].astype(np.float64) - before[13:19])[:, alive]
    near = max(alive.sum(), 1)
    return dict(speed_hi=float((jqd >= vlim * (1 - 1e-6)).sum() / (6 * near)),
                speed_lo=float((jqd <= -vlim * (1 - 1e-6)).sum() / (6 * near)),
                omega_cap=float((w >= wmax * (1 - 1e-5)).sum() / near),
                wrap_hi=int((dq < -2 * np.pi).sum()), wrap_lo=int((dq > 2 * np.pi).sum()))


def coverage(task: str, st: np.ndarray, actions: np.ndarray, seed: int = 0) -> dict:
    """What one step from ``st`` with ``actions`` exercises, measured on the f64 oracle of
    fullstate.task_cfg(task): one step, and one physics substep from the same state with the targets
    of prologue64. Fractions (wraps: counts):
    pdel_hi / pdel_lo (manager: clip_hi / clip_lo): entries the prologue puts on each clamp side;
    sat_hi / sat_lo [6]: envs whose joint's drive torque is at +-effort_limit (|tau| >= effort - 1e-4)
    in the first substep, and sat_masks, the number of distinct 6-bit saturation patterns;
    touch_hi / touch_lo: the number of (env, joint) entries at +-velocity_limit after that first substep;
    speed_hi / speed_lo, omega_cap, wrap_hi / wrap_lo: post_step_coverage of the surviving envs;
    terminated: envs that reset in the step; finite: every output and state value is finite."""
    from oracle.pyoracle import OracleSim
    n = st.shape[1]
    cfg = task_cfg(task)
    o = OracleSim(n, cfg, seed=seed, double=True)
    o.set_state(st)
    obs, rew, te, tr = o.step(actions)
    after = o.get_state()
    pro = prologue64(task, o, st, actions)
    out = dict(terminated=float((te | tr).mean()),
               finite=bool(np.isfinite(obs).all() and np.isfinite(rew).all() and np.isfinite(after).all()))
    k = "clip" if base_task(task) == "manager" else "pdel"
    out[k + "_hi"] = float((pro["raw"] >= pro["lim"]).mean())
    out[k + "_lo"] = float((pro["raw"] <= -pro["lim"]).mean())
    out.update(post_step_coverage((float(o._m.velocity_limit), float(o._m.max_angular_velocity)), st, after, te | tr))
    o2 = OracleSim(n, cfg, seed=seed, double=True)
    o2.set_state(st)
    _, tau = o2.physics_substeps(pro["target"].T, 1)
    jqd1, vlim = o2.get_state()[19:25].astype(np.float64), float(o._m.velocity_limit)
    out["touch_hi"], out["touch_lo"] = int((jqd1 >= vlim * (1 - 1e-6)).sum()), int((jqd1 <= -vlim * (1 - 1e-6)).sum())
    eff = float(o._m.effort_limit) - 1e-4
    out["sat_hi"] = (tau >= eff).mean(axis=0)
    out["sat_lo"] = (tau <= -eff).mean(axis=0)
    out["sat_masks"] = len(np.unique(((np.abs(tau) >= eff) * (1 << np.arange(6))).sum(axis=1)))
    return out


def _bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, F32).view(np.uint32)


def tanh32(a: np.ndarray) -> np.ndarray:
    """float32(tanh(float64(a))): the correctly rounded float32 tanh wherever tanh(float64(a)) is not
    within double rounding of a float32 tie (test_limit_cases.test_actions_are_tie_free)."""
    return np.tanh(a.astype(np.float64)).astype(F32)


def check_prologue(task: str, c: dict, s_dev: np.ndarray, reset_dev: np.ndarray, label: str = "device") -> dict:
    """The exactness rules of the step's prologue on a device's post-step state ``s_dev`` of case
    ``c`` (kind "prologue"), over the envs where neither the device nor the f32 oracle reset (at most
    5 % may be set aside):
    * the ACTIONS rows are bit-equal to the f32 oracle's, and to float32(tanh(float64(a))) (the tanh
      tasks: -0.0 -> -0.0, denormals unchanged, exactly +-1 from 9.0109 upward, +-inf -> +-1) or to the raw
      action (the manager, which stores it);
    * P_DELTA entries that every fp32 evaluation clamps -- the fp64 value before the clamp beyond
      +-(float32(pi) + 4 eps32 pi) -- equal +-float32(pi) bit for bit (the fp64 restatement clamps at the
      double pi, 8.7e-8 below float32(pi): the entries in that 1.6e-6 band are counted, printed and held
      to the next rule);
    * per joint, the other P_DELTA entries satisfy err <= max(4 e32, 2 eps32 max |x64|), err and e32 the
      device's and the f32 oracle's largest error against the fp64 restatement (the rule of
      tests/test_gpu_critic_obs.py); entries within rounding of the clamp fall here, where float32(pi)
      and its neighbour are both inside the floor.
    The manager has no P_DELTA row, and its clipped delta is no state row either: it reaches the state
    only through the drive targets (test_full_state_at_limits); prologue64's clip sides are checked
    against the oracle's own processed actions on the CPU. Returns the measured figures."""
    D = _layout(task)
    te, tr = c["out32"][2:]
    keep = ~(np.asarray(reset_dev, bool) | te | tr)
    excluded = float((~keep).mean())
    assert excluded <= 0.05, f"{task} {label}: {excluded:.1%} of the envs reset"
    rows = slice(D["ACTIONS"], D["ACTIONS"] + 6)
    got = s_dev[rows][:, keep]
    a = c["a"].T[:, keep]
    for name, want in (("the f32 oracle", c["s32"][rows][:, keep]),
                       ("the raw action", a) if base_task(task) == "manager" else ("float32(tanh(float64(a)))", tanh32(a))):
        bad = np.argwhere(_bits(got) != _bits(want))
        assert not len(bad), (f"{task} {label}: {len(bad)} ACTIONS entries differ from {name}; first (joint, env col) "
                              f"{bad[:4].tolist()}: raw {[float(a[j, e]) for j, e in bad[:4]]} got "
                              f"{[float(got[j, e]) for j, e in bad[:4]]} want {[float(want[j, e]) for j, e in bad[:4]]}")
    out = dict(excluded=excluded, n_clamped=0, worst=0.0)
    if "P_DELTA" not in D:
        return out
    rows = slice(D["P_DELTA"], D["P_DELTA"] + 6)
    got, o32 = s_dev[rows][:, keep], c["s32"][rows][:, keep].astype(np.float64)
    raw, x64 = c["pro"]["raw"][:, keep], c["pro"]["p_delta"][:, keep]
    edge = float(PI32) + 4 * EPS32 * np.pi
    hi, lo = raw >= edge, raw <= -edge
    out["n_clamped"] = int(hi.sum() + lo.sum())
    # entries the fp64 restatement clamps but an fp32 evaluation need not (within 4 eps32 pi of float32(pi))
    out["n_band"] = int(((np.abs(raw) >= np.pi) & ~(hi | lo)).sum())
    assert (_bits(got[hi]) == _bits(PI32)).all() and (_bits(got[lo]) == _bits(-PI32)).all(), \
        f"{task} {label}: clamped P_DELTA entries off +-float32(pi): {got[hi][_bits(got[hi]) != _bits(PI32)][:4]} " \
        f"{got[lo][_bits(got[lo]) != _bits(-PI32)][:4]}"
    free = ~(hi | lo)
    fails = []
    for j in range(6):
        f = free[j]
        err, e32 = np.abs(got[j][f] - x64[j][f]).max(), np.abs(o32[j][f] - x64[j][f]).max()
        floor = 2 * EPS32 * np.abs(x64[j][f]).max()
        out["ratio"] = max(out.get("ratio", 0.0), err / e32 if e32 > 0 else float("inf"))
        if err > floor:
            out["worst"] = max(out["worst"], err / e32 if e32 > 0 else float("inf"))
        if not err <= max(4 * e32, floor):
            fails.append((j, f"err {err:.3g}", f"e32 {e32:.3g}", f"floor {floor:.3g}"))
    print(f"\n[{task} {label}] prologue: {excluded:.2%} envs reset, {out['n_clamped']} P_DELTA entries on the clamp "
          f"(+ {out['n_band']} clamped in fp64 only, under the tolerance rule), "
          f"worst err / e32 {out['ratio']:.2f} (above the floor {out['worst']:.2f})")
    assert not fails, (task, label, fails)
    return out
