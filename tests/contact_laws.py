"""Laws a contact substep obeys whatever impulses its solver settles on, stated in float64 on the
independent reference of tests/dynamics_reference.py. TEST INFRASTRUCTURE ONLY: the case builders and the
law evaluators of tests/test_oracle_contact_laws.py and tests/test_gpu_contact_laws.py.

With u = [v_root(3), omega_root(3), qdot(6)] (the reference's coordinates) and M, C from
``Reference.dynamics`` at the pre-substep state, the generalised contact force of one substep is

    r = M (u+ - u) / dt + C - [0_6; tau_drive]

Only its six root rows are used: there tau_drive, the armature and every self-contact pair drop out, so
r[0:3] is the sum of the external (ground) contact forces and r[3:6] their moment about the root origin.

L1  r[0:3] = sum over the 12 links of the reported net_force (every set).
L2  airborne, links touching each other: r[0:6] = 0 and sum net_force = 0.
L3  nothing near anything: net_force == 0 exactly and r[0:6] = 0 (and every link of the one-link set
    other than the touching one reports exactly zero, in the first substep).
L4  ground-only sets, per link: F_z >= 0 and |F_xy| <= mu_s F_z.
L5  sliding: |F_xy| <= mu_d F_z per loaded link; the summed friction opposes the sliding velocity and
    reaches the cone boundary (L5_MEASURED: measured on the f64 oracle).
L6  one link touching: the line of action implied by the moment rows r[3:6] = (p - P) x F passes, at a
    height between -(penetration + 1 mm) and the margin, within one link radius of that link's lowest
    point (coarse: p is free along the line, so the closest approach inside that slab is taken).
L4 and L5 read a link's net force as its ground force, so they are evaluated on a transition only where
the fp64 geometry of its pre-state rules a self contact out (every non-adjacent pair further apart than
the margin): an impact can bring the feet together within four substeps.

floor_i = sum_j |M_ij| (ulp32(u+_j) + ulp32(u_j)) / dt (+ ulp32 of each reported force component that
enters the law): what the float32 state and force rows alone may round.

An env in which a joint-speed clamp or the root angular cap acted in the substep (|qd| == vlim, |omega|
at the cap in the post-state) is left out of the balance laws: the projection breaks the equality.

The case sets' conditions are asserted on the float64 geometry: ``RobotModel.fk`` and each link's rounded
core (the authored circles shrunk by the rounding radius, tests/test_oracle_selfcollision.py's
``core_circles``). The lowest point of a core circle (centre c, axes E1, E2) swept by the rounding radius
rho is c_z - sqrt(E1_z^2 + E2_z^2) - rho. (The simulators' ground candidates are the authored, sharp rims,
which lie at or up to 0.42 rho = 1.7 mm below that point; every condition here is safe for either.)
Distances between links are bounded from below by the largest separating gap over a fixed set of
directions, and the pair that defines the folded set is measured by ``brute_distance``.
"""
from __future__ import annotations

import functools

import numpy as np

import dynamics_reference as D
import test_oracle_dynamics as T
from test_oracle_selfcollision import CORE_M, brute_distance, core_circles, world
from zbot_lab_amd import model as zm

S, ND, NL, NPHYS = zm.S, zm.NUM_DOF, zm.NUM_LINKS, D.NPHYS
N = 130
SETS = ("resting", "impact", "sliding", "sticking", "one_link", "airborne_folded", "airborne_free")
K = len(SETS)
GROUND_SETS = ("resting", "impact", "sliding", "sticking", "one_link")
MAX_EXCLUDED = 0.10
F64_FACTOR = 4.0          # the f64 oracle: L1-L3 within this many floors (and the GPU bound's floor)
DEVICE_FACTOR = 3.0       # the project's contact-free factor: device <= 3 x the f32 oracle
CONE_REL = 1e-5
LOADED = 1.0              # N: a link counts as loaded (L5, L6) above this normal force
# L5, measured on the f64 oracle over the five configurations, first and fourth substep:
# the smallest |sum F_xy| / sum mu_d F_z and the smallest cosine of sum F_xy against -v. The f32 oracle
# and the device are held to these minus 10 % of their distance to the ideal 1.
# Per substep of the chain {substep: (ratio, cosine)}: in the first one the robot still translates as set
# up; by the fourth the friction at the feet has tipped a standing robot and stopped some of them, the
# contact points no longer move with the root and the two figures say little (kept as measured).
# Measured: substep 1 ratio 0.839108 (manager, heavy base), cosine 0.967957 (stand-up); substep 4 ratio
# 0.303214, cosine -0.990909 (walking v2, PGS); recorded rounded down.
L5_MEASURED = {1: (0.8391, 0.9679), 4: (0.3032, -0.9910)}

# configuration -> (model of tests/test_oracle_dynamics.py, cfg overrides, per-link friction drawn)
CONFIGS = {
    "walking-v2-pgs": ("walking-v2", dict(solver_mode=0), False),
    "walking-v2-tgs-rf": ("walking-v2", dict(solver_mode=1, self_manifold=3), False),
    "standup-sd": ("standup", dict(), True),
    "manager": ("manager", dict(), False),
    "manager-heavy": ("manager-heavy", dict(), False),
}
GEOMETRY = {"walking-v2": "walking-v2", "standup": "standup", "manager": "manager", "manager-heavy": "manager"}


def make_cfg(config):
    name, kw, _ = CONFIGS[config]
    return T.make_cfg(name, enable_self_collision=True, **kw)


def set_of(e):
    return SETS[e % K]


def envs_of(case, n=N):
    return np.arange(SETS.index(case), n, K)


# ------------------------------------------------------------------ geometry (float64)
_DIRS = None


def _dirs(k=1500):
    global _DIRS
    if _DIRS is None:
        i = np.arange(k) + 0.5
        z = 1.0 - 2.0 * i / k
        ph = i * np.pi * (3.0 - np.sqrt(5.0))
        s = np.sqrt(1.0 - z * z)
        _DIRS = np.stack([s * np.cos(ph), s * np.sin(ph), z], axis=1)
    return _DIRS


@functools.lru_cache(maxsize=None)
def _cores(geom):
    rm = T.robot(geom)
    return [core_circles(np.asarray(rm.circles[l], np.float64)) for l in range(NL)]


def hulls(geom, pos, quat, q):
    """World core circles [12, 2, 9] of every link (centre, E1, E2)."""
    rm = T.robot(geom)
    bodies, _ = rm.fk(pos, zm.qnorm(quat), q)
    out = np.zeros((NL, 2, 9))
    for l in range(NL):
        X = bodies[rm.link_body[l]]
        out[l] = world(_cores(geom)[l], zm.qmat(X.q), X.p)
    return out


def lowest(h):
    """Per link: height of the lowest point of the rounded hull [12] and that point [12, 3]."""
    rad = np.hypot(h[:, :, 5], h[:, :, 8])                      # [12, 2]
    z = h[:, :, 2] - rad - CORE_M
    c = np.argmin(z, axis=1)
    i = np.arange(NL)
    hc, r = h[i, c], np.maximum(rad[i, c], 1e-300)
    pt = hc[:, :3] - (hc[:, 5] / r)[:, None] * hc[:, 3:6] - (hc[:, 8] / r)[:, None] * hc[:, 6:9]
    pt[:, 2] -= CORE_M
    return z[i, c], pt


def pair_gaps(geom, h):
    """Lower bound of the separation of the rounded hulls of every non-adjacent pair: the largest
    separating gap over a fixed set of directions, minus the two rounding radii."""
    n = _dirs()
    proj = h[:, :, :3] @ n.T                                        # [12, 2, D]
    rad = np.hypot(h[:, :, 3:6] @ n.T, h[:, :, 6:9] @ n.T)
    lo, hi = (proj - rad).min(axis=1), (proj + rad).max(axis=1)     # [12, D]
    pairs = np.asarray(T.robot(geom).self_pairs)
    return (lo[pairs[:, 0]] - hi[pairs[:, 1]]).max(axis=1) - 2 * CORE_M


def radius(geom, link):
    """The authored radius of a link's circles (core radius + rounding radius)."""
    c = np.asarray(T.robot(geom).circles[link], np.float64)
    return float(max(np.linalg.norm(c[0, 3:6]), np.linalg.norm(c[1, 3:6])))


def _yaw(a):
    return np.array([np.cos(0.5 * a), 0.0, 0.0, np.sin(0.5 * a)])


def _state(pos, quat, v, w, q, qd):
    x = np.zeros(NPHYS)
    x[S["ROOT_POS"]:S["ROOT_POS"] + 3], x[S["ROOT_QUAT"]:S["ROOT_QUAT"] + 4] = pos, zm.qnorm(quat)
    x[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3], x[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3] = v, w
    x[S["JOINT_POS"]:S["JOINT_POS"] + ND], x[S["JOINT_VEL"]:S["JOINT_VEL"] + ND] = q, qd
    return x


def _place(geom, quat, q, height, rng):
    """Root position with the lowest hull point at ``height``."""
    z, _ = lowest(hulls(geom, np.zeros(3), quat, q))
    return np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), height - z.min()])


def _fold(geom, rng, window):
    """Joint angles with the closest non-adjacent pair's gap (lower bound) inside ``window``: a random
    pose, one joint swept and bisected."""
    rm = T.robot(geom)
    quat = D._unit_quats(rng, 1)[0]
    mid = 0.5 * (window[0] + window[1])
    for _ in range(200):
        q = rng.uniform(-np.pi, np.pi, ND)
        j = int(rng.integers(0, ND))
        f = lambda a: pair_gaps(geom, hulls(geom, np.zeros(3), quat, np.r_[q[:j], a, q[j + 1:]])).min()  # noqa: E731
        grid = np.linspace(-np.pi, np.pi, 33)
        vals = np.array([f(a) for a in grid])
        for i in range(len(grid) - 1):
            if vals[i] > mid > vals[i + 1] or vals[i] < mid < vals[i + 1]:
                a, b, fa = grid[i], grid[i + 1], vals[i]
                for _ in range(24):
                    m = 0.5 * (a + b)
                    fm = f(m)
                    if window[0] < fm < window[1]:
                        q[j] = m
                        return quat, q
                    if (fm > mid) == (fa > mid):
                        a, fa = m, fm
                    else:
                        b = m
    raise RuntimeError(f"{geom}: no folded pose found")


@functools.lru_cache(maxsize=None)
def _case_states(geom, n, seed, sticking_speed):
    rm = T.robot(geom)
    cfg = T.make_cfg(geom)
    margin = float(cfg.contact_margin)
    rows = np.zeros((NPHYS, n))
    tg = np.zeros((n, ND))
    for e in range(n):
        case = set_of(e)
        rng = np.random.default_rng([seed, e])
        zero3, zq = np.zeros(3), np.zeros(ND)
        if case in ("resting", "sliding", "sticking"):
            quat = zm.qmul(_yaw(rng.uniform(-np.pi, np.pi)), zm.qnorm(rm.default_root_quat))
            q = rm.default_joint_pos.copy()
            pos = _place(geom, quat, q, rng.uniform(-1e-3, 0.5 * margin), rng)
            speed = {"resting": 0.0, "sliding": rng.uniform(0.5, 1.0), "sticking": sticking_speed}[case]
            a = rng.uniform(-np.pi, np.pi)
            rows[:, e], tg[e] = _state(pos, quat, speed * np.array([np.cos(a), np.sin(a), 0.0]), zero3, q, zq), q
        elif case in ("impact", "one_link"):
            for _ in range(2000):
                quat = D._unit_quats(rng, 1)[0]
                q = rm.default_joint_pos + rng.uniform(-0.5, 0.5, ND)
                h = hulls(geom, zero3, quat, q)
                if pair_gaps(geom, h).min() <= 0.0105:
                    continue
                z, _ = lowest(h)
                height = rng.uniform(0.2e-3, 0.9 * margin)
                if case == "one_link" and np.sort(z)[1] - z.min() + height <= margin + 5.5e-3:
                    continue
                break
            else:
                raise RuntimeError(f"{geom}: no {case} state found")
            pos = _place(geom, quat, q, height, rng)
            v = np.array([*rng.normal(size=2) * 0.1, -rng.uniform(0.1, 1.0)])
            rows[:, e] = _state(pos, quat, v, 0.2 * rng.normal(size=3), q, 0.2 * rng.normal(size=ND))
            tg[e] = q + rng.uniform(-0.3, 0.3, ND)
        elif case == "airborne_folded":
            quat, q = _fold(geom, rng, (-1.4e-3, -0.3e-3))
            pos = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 2.0])
            rows[:, e] = _state(pos, quat, 0.5 * rng.normal(size=3), rng.normal(size=3), q, rng.uniform(-0.05, 0.05, ND))
            tg[e] = q + rng.uniform(-0.3, 0.3, ND)
        else:
            for _ in range(2000):
                quat = D._unit_quats(rng, 1)[0]
                q = rm.default_joint_pos + rng.uniform(-0.5, 0.5, ND)
                if pair_gaps(geom, hulls(geom, zero3, quat, q)).min() > 0.0105:
                    break
            pos = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 2.0])
            rows[:, e] = _state(pos, quat, 0.5 * rng.normal(size=3), rng.normal(size=3), q, rng.normal(size=ND))
            tg[e] = q + rng.uniform(-0.3, 0.3, ND)
    rows, tg = rows.astype(np.float32), tg.astype(np.float32)
    held = [e for e in range(n) if set_of(e) in ("resting", "sliding", "sticking")]   # targets = the float32 angles
    tg[held] = rows[S["JOINT_POS"]:S["JOINT_POS"] + ND].T[held]
    return rows, tg


def case_states(name, n=N, seed=0, sticking_speed=1e-3):
    """(rows [25, n] float32, targets [n, 6] float32): env e is of set e % 7. Cached by geometry (the
    manager robot with the heavy base has the nominal one's states); fresh copies."""
    rows, tg = _case_states(GEOMETRY[name], n, seed, float(sticking_speed))
    return rows.copy(), tg.copy()


@functools.lru_cache(maxsize=None)
def geometry_facts(name, n=N, seed=0):
    """Per env, from the float32 rows in float64: lowest [n, 12], lowest points [n, 12, 3], min pair gap
    (lower bound) [n]."""
    geom = GEOMETRY[name]
    rows, _ = case_states(name, n, seed)
    low, pts, gap = np.zeros((n, NL)), np.zeros((n, NL, 3)), np.zeros(n)
    for e in range(n):
        pos, quat, q, _ = T._split(rows[:, e].astype(np.float64))
        h = hulls(geom, pos, quat, q)
        low[e], pts[e] = lowest(h)
        gap[e] = pair_gaps(geom, h).min()
    return low, pts, gap


def assert_conditions(name, n=N, seed=0):
    """Each set's defining condition, on the float64 geometry of the float32 rows."""
    geom = GEOMETRY[name]
    rm = T.robot(geom)
    margin = float(T.make_cfg(geom).contact_margin)
    rows, tg = case_states(name, n, seed)
    low, _, gap = geometry_facts(name, n, seed)
    x = rows.astype(np.float64)
    v, w = x[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3], x[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3]
    q, qd = x[S["JOINT_POS"]:S["JOINT_POS"] + ND], x[S["JOINT_VEL"]:S["JOINT_VEL"] + ND]
    slack = 1e-7          # float32 rounding of the root height
    for e in range(n):
        case, lo = set_of(e), low[e].min()
        if case in ("resting", "sliding", "sticking"):
            assert -1e-3 - slack <= lo <= 0.5 * margin + slack, (case, e, lo)
            assert np.array_equal(tg[e], rows[S["JOINT_POS"]:S["JOINT_POS"] + ND, e])
            assert np.abs(q[:, e] - rm.default_joint_pos).max() < 1e-6
            assert not w[:, e].any() and not qd[:, e].any() and v[2, e] == 0.0
            speed = np.hypot(v[0, e], v[1, e])
            assert {"resting": speed == 0.0, "sliding": 0.5 <= speed <= 1.0, "sticking": abs(speed - 1e-3) < 1e-6}[case]
        elif case in ("impact", "one_link"):
            assert 0.0 < lo < margin and gap[e] > 0.010 and -1.0 <= v[2, e] <= -0.1, (case, e, lo, gap[e])
            if case == "one_link":
                assert np.sort(low[e])[1] > margin + 5e-3
        else:
            assert low[e].min() > 1.0      # the root 2 m up, the chain under 1 m long
            if case == "airborne_free":
                assert gap[e] > 0.010
    # airborne folded: the closest pair (by the lower bound) is inside the self-contact margin by the
    # brute-force hull distance of tests/test_oracle_selfcollision.py
    pairs = T.robot(geom).self_pairs
    for e in envs_of("airborne_folded", n):
        pos, quat, qq, _ = T._split(x[:, e])
        h = hulls(geom, pos, quat, qq)
        a, b = pairs[int(np.argmin(pair_gaps(geom, h)))]
        d = brute_distance(h[a], h[b]) - 2 * CORE_M
        assert d < margin and gap[e] > -1.5e-3, (e, d, gap[e])


# ------------------------------------------------------------------ friction rows
def link_friction(config, n=N):
    """(mu_static, mu_dynamic) [n, 12] float32 per link, or None where the task has no per-link friction."""
    name, _, drawn = CONFIGS[config]
    if name == "walking-v2":
        return None
    if not drawn:
        one = np.ones((n, NL), np.float32)
        return one, one.copy()
    rng = np.random.default_rng(77)
    a, b = rng.uniform(0.6, 1.2, (n, NL)), rng.uniform(0.6, 1.2, (n, NL))
    return np.maximum(a, b).astype(np.float32), np.minimum(a, b).astype(np.float32)


def friction_state_rows(config, n=N, mu=None):
    name = CONFIGS[config][0]
    mu = link_friction(config, n) if mu is None else mu
    if mu is None:
        return {}
    layout = zm.SU if name == "standup" else zm.M
    return {layout["LINK_MU"]: mu[0].T, layout["LINK_MU_D"]: mu[1].T}


def contact_mu(config, n=N, mu=None):
    """(mu_s, mu_d) [n, 12] float64 of a link against the ground: per-link x the ground's."""
    cfg = make_cfg(config)
    mu = link_friction(config, n) if mu is None else mu
    if mu is None:
        return np.full((n, NL), float(cfg.friction)), np.full((n, NL), float(cfg.friction_dynamic))
    return mu[0].astype(np.float64) * float(cfg.friction), mu[1].astype(np.float64) * float(cfg.friction_dynamic)


# ------------------------------------------------------------------ runners
def oracle_chain(config, rows, tg, double, nsub=4, mu=None):
    """``nsub`` calls of one substep each, the state read back in between. Returns (states [nsub + 1, 25, n]
    float32, pre-state first; forces [nsub, n, 12, 3] float32)."""
    name = CONFIGS[config][0]
    forces = {}
    n = rows.shape[1]
    out, _, _ = T.oracle_substeps(name, make_cfg(config), rows, tg, nsubs=tuple(range(1, nsub + 1)), double=double,
                                  state_rows=friction_state_rows(config, n, mu), forces=forces)
    return (np.stack([rows] + [out[k] for k in range(1, nsub + 1)]), np.stack([forces[k] for k in range(1, nsub + 1)]))


# ------------------------------------------------------------------ the laws
def _u(x):
    return T._split(x)[3]


def residuals(config, pre, post, nf, mutant=None):
    """Per env, in float64 from the float32 rows taken exactly: r [n, 6] (root rows of the generalised
    contact force), floor_r [n, 6], P [n, 3] and the exclusion mask [n] (a clamp or the cap acted)."""
    name = CONFIGS[config][0]
    ref = T.reference(name, make_cfg(config))
    pm = zm.pack_model(T.robot(name))
    vlim, wmax = np.float32(pm.velocity_limit), float(pm.max_angular_velocity)
    n = pre.shape[1]
    r, fl, P = np.zeros((n, 6)), np.zeros((n, 6)), np.zeros((n, 3))
    for e in range(n):
        pos, quat, q, u = T._split(pre[:, e].astype(np.float64))
        d = _dynamics(config, pre[:, e].tobytes())
        u1 = _u(post[:, e].astype(np.float64))
        # planted error: gravity's share of C (C at u = 0) left out
        C = d["C"] - _gravity_C(config, pre[:, e].astype(np.float64)) if mutant == "no_gravity_C" else d["C"]
        r[e] = (d["M"] @ (u1 - u) / ref.dt + C)[:6]
        fl[e] = (np.abs(d["M"][:6]) @ (D.ulp32(u1) + D.ulp32(u))) / ref.dt
        P[e] = pos
    qd = post[S["JOINT_VEL"]:S["JOINT_VEL"] + ND]
    w = np.linalg.norm(post[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3].astype(np.float64), axis=0)
    excluded = (np.abs(qd) == vlim).any(axis=0) | (np.abs(w - wmax) <= 8 * float(np.spacing(np.float32(wmax)))) | (w > wmax)
    return r, fl, P, excluded


_DYN: dict = {}


def _dynamics(config, key):
    """M and C at a float32 pre-state, cached by (model, gravity, state bytes)."""
    name = CONFIGS[config][0]
    k = (name, key)
    if k not in _DYN:
        if len(_DYN) > 6000:
            _DYN.clear()
        ref = T.reference(name, make_cfg(config))
        pos, quat, q, u = T._split(np.frombuffer(key, np.float32).astype(np.float64))
        d = ref.dynamics(pos, quat, q, u)
        _DYN[k] = dict(M=d["M"], C=d["C"])
    return _DYN[k]


def _gravity_C(config, x):
    name = CONFIGS[config][0]
    ref = T.reference(name, make_cfg(config))
    pos, quat, q, _ = T._split(x)
    return ref.dynamics(pos, quat, q, np.zeros(12))["C"]


def force_floor(F):
    """ulp32 of each reported force component, summed over the leading axes given as [..., 3]."""
    return D.ulp32(F)


def evaluate(config, states, forces, mutant=None, mu=None, l6=True):
    """All laws on a chain (states [k + 1, 25, n], forces [k, n, 12, 3]). Returns a dict:
    ``ratio[law][set]`` the largest residual / floor over the set's envs and the chain's transitions
    (L1-L3), ``per_env[law]`` [k, n] the same per env (nan where the law does not apply or the env is
    excluded), ``excluded[set]`` the share left out, ``violations`` a list of strings (L3's exact zeros and
    L4-L6), ``l5`` (ratio, cosine) [k, n] and ``loaded_folded`` the share of folded envs reporting a force."""
    name = CONFIGS[config][0]
    geom = GEOMETRY[name]
    cfg = make_cfg(config)
    margin = float(cfg.contact_margin)
    k, n = forces.shape[0], forces.shape[1]
    sets = np.array([e % K for e in range(n)])
    mu_s, mu_d = contact_mu(config, n, mu)
    low, pts, _ = geometry_facts(name, n) if n == N else (None, None, None)
    per_env = {law: np.full((k, n), np.nan) for law in ("L1", "L2r", "L2f", "L3")}
    l5 = np.full((2, k, n), np.nan)
    violations, excl, unclear = [], np.zeros((k, n), bool), np.zeros((k, n), bool)
    cone_miss = np.zeros((k, n))
    l6_stats = []
    for t in range(k):
        pre, post = states[t], states[t + 1]
        F = forces[t].astype(np.float64)
        if mutant == "drop_reaction" or mutant == "reaction_at_origin":
            F = F.copy()
        r, fl, P, ex = residuals(config, pre, post, forces[t], mutant="no_gravity_C" if mutant == "no_gravity_C" else None)
        excl[t] = ex
        shift = np.zeros((n, 3))
        if mutant in ("drop_reaction", "reaction_at_origin"):
            for e in np.where(sets == SETS.index("airborne_folded"))[0]:
                on = np.where(np.abs(F[e]).sum(axis=1) > 0)[0]
                if len(on) < 2:
                    continue
                b = on[-1]
                if mutant == "drop_reaction":
                    F[e, b] = 0.0
                else:
                    pos, quat, q, _ = T._split(pre[:, e].astype(np.float64))
                    rm = T.robot(geom)
                    _, links = rm.fk(pos, quat, q)
                    h = hulls(geom, pos, quat, q)
                    centre = 0.25 * (h[on[0], :, :3].sum(axis=0) + h[b, :, :3].sum(axis=0))
                    shift[e] = np.cross(links[b].p - centre, F[e, b])
        Fsum = F.sum(axis=1)                                   # [n, 3]
        ffl = force_floor(F).sum(axis=1)                       # [n, 3]
        ok = ~ex
        # L1
        per_env["L1"][t, ok] = (np.abs(r[:, :3] - Fsum) / (fl[:, :3] + ffl)).max(axis=1)[ok]
        # L2
        m = ok & (sets == SETS.index("airborne_folded"))
        rr = r.copy()
        rr[:, 3:6] += shift
        per_env["L2r"][t, m] = (np.abs(rr) / fl).max(axis=1)[m]
        per_env["L2f"][t, m] = (np.abs(Fsum) / ffl).max(axis=1)[m]
        # L3
        free = sets == SETS.index("airborne_free")
        per_env["L3"][t, ok & free] = (np.abs(r) / fl).max(axis=1)[ok & free]
        for e in np.where(free)[0]:
            if F[e].any():
                violations.append(f"L3: airborne free env {e}, substep {t + 1}: net_force {np.abs(F[e]).max():.3g} != 0")
        if t == 0 and low is not None:
            for e in np.where(sets == SETS.index("one_link"))[0]:
                touching = int(np.argmin(low[e]))
                others = np.delete(F[e], touching, axis=0)
                if others.any():
                    violations.append(f"L3: one-link env {e}: another link reports {np.abs(others).max():.3g} N")
        # L4 and L5 read a link's net force as its ground force: only where the pre-state's fp64 geometry
        # rules a self contact out (every non-adjacent pair further apart than the margin)
        clear = np.zeros(n, bool)
        for e in np.where(np.isin(sets, [SETS.index(c) for c in GROUND_SETS]))[0]:
            pos, quat, q, _ = T._split(pre[:, e].astype(np.float64))
            clear[e] = pair_gaps(geom, hulls(geom, pos, quat, q)).min() > margin
        unclear[t] = ~clear
        # L4
        for case in GROUND_SETS:
            for e in np.where(clear & (sets == SETS.index(case)))[0]:
                for l in range(NL):
                    f = F[e, l]
                    if not f.any():
                        continue
                    floor = force_floor(f).sum()
                    mus = mu_d[e, l] if mutant == "mu_dynamic" else mu_s[e, l]
                    lim = mus * f[2] * (1 + CONE_REL) + floor
                    if f[2] < -floor:
                        violations.append(f"L4: {case} env {e} link {l} substep {t + 1}: F_z {f[2]:.6g} < 0")
                    if np.hypot(f[0], f[1]) > lim:
                        cone_miss[t, e] = max(cone_miss[t, e], (np.hypot(f[0], f[1]) - mus * f[2] * (1 + CONE_REL)) / floor)
                        violations.append(f"L4: {case} env {e} link {l} substep {t + 1}: |F_xy| {np.hypot(f[0], f[1]):.6g} "
                                          f"> mu F_z {lim:.6g} (by {cone_miss[t, e]:.3g} floors)")
        # L5
        for e in np.where(clear & (sets == SETS.index("sliding")))[0]:
            v = pre[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 2, e].astype(np.float64)
            loaded = F[e, :, 2] > LOADED
            for l in np.where(loaded)[0]:
                f = F[e, l]
                if np.hypot(f[0], f[1]) > mu_d[e, l] * f[2] * (1 + CONE_REL) + force_floor(f).sum():
                    violations.append(f"L5: sliding env {e} link {l} substep {t + 1}: |F_xy| {np.hypot(f[0], f[1]):.6g} "
                                      f"> mu_d F_z {mu_d[e, l] * f[2]:.6g}")
            if loaded.any():
                fx = F[e, loaded, :2].sum(axis=0)
                l5[0, t, e] = np.linalg.norm(fx) / (mu_d[e, loaded] * F[e, loaded, 2]).sum()
                l5[1, t, e] = -(fx @ v) / (np.linalg.norm(fx) * np.linalg.norm(v))
        # L6
        if t == 0 and l6 and low is not None:
            for e in np.where(ok & (sets == SETS.index("one_link")))[0]:
                touching = int(np.argmin(low[e]))
                f, mo = F[e, touching], r[e, 3:6]
                if f[2] <= LOADED:
                    continue
                # the line of action p0 + s f; its point at height z is p0 + (z - p0_z) / f_z f. The horizontal
                # offset from the lowest point is linear in z: the closest approach within the slab
                p0 = P[e] + np.cross(f, mo) / (f @ f)
                pen = max(0.0, -low[e, touching])
                z_lo, z_hi = -(pen + 1e-3), margin
                a = p0[:2] - pts[e, touching, :2] - p0[2] / f[2] * f[:2]
                b = f[:2] / f[2]
                z = float(np.clip(-(a @ b) / max(b @ b, 1e-300), z_lo, z_hi))
                horiz = float(np.linalg.norm(a + b * z))
                l6_stats.append((e, z, horiz))
                if horiz > radius(geom, touching):
                    violations.append(f"L6: one-link env {e}: the line of action passes {horiz * 1e3:.2f} mm from the lowest point "
                                      f"within the slab (radius {radius(geom, touching) * 1e3:.1f} mm)")
    ratio = {}
    for law, scope in (("L1", SETS), ("L2r", ("airborne_folded",)), ("L2f", ("airborne_folded",)), ("L3", ("airborne_free",))):
        ratio[law] = {}
        for case in scope:
            vals = per_env[law][:, sets == SETS.index(case)]
            ratio[law][case] = float(np.nanmax(vals)) if np.isfinite(vals).any() else 0.0
    excluded = {case: float(excl[:, sets == SETS.index(case)].any(axis=0).mean()) for case in SETS}
    folded = sets == SETS.index("airborne_folded")
    loaded_folded = float((np.abs(forces[:, folded]).sum(axis=(0, 2, 3)) > 0).mean())
    self_near = {case: float(unclear[:, sets == SETS.index(case)].any(axis=0).mean()) for case in GROUND_SETS}
    return dict(ratio=ratio, per_env=per_env, excluded=excluded, violations=violations, l5=l5, loaded_folded=loaded_folded,
                l6=l6_stats, excl=excl, self_near=self_near, cone_miss=cone_miss)


def l5_bounds(substep):
    """What the f32 oracle and the device are held to in the chain's ``substep`` (1 or 4): the f64
    oracle's measured (ratio, cosine) minus 10 % of their distance to the ideal 1."""
    ratio, cos = L5_MEASURED[substep]
    return ratio - 0.1 * (1.0 - ratio), cos - 0.1 * (1.0 - cos)


def l5_smallest(res, substep):
    """(smallest ratio, smallest cosine) of the chain's ``substep``; (1, 1) where no link was loaded."""
    l5 = res["l5"][:, substep - 1]
    return tuple(float(np.nanmin(a)) if np.isfinite(a).any() else 1.0 for a in l5)


def assert_l5(res, tag):
    for substep in (1, 4):
        if res["l5"].shape[1] < substep:
            continue
        (ratio, cos), (rb, cb) = l5_smallest(res, substep), l5_bounds(substep)
        assert ratio >= rb and cos >= cb, f"{tag}: L5 substep {substep}: ratio {ratio:.6f} (>= {rb:.6f}), cosine {cos:.6f} (>= {cb:.6f})"


def describe(tag, res):
    lines = []
    for law, by_set in res["ratio"].items():
        lines.append(f"[{tag}] {law} residual / floor: " + ", ".join(f"{c} {v:.3g}" for c, v in by_set.items()))
    lines.append(f"[{tag}] excluded (clamp or cap): " + ", ".join(f"{c} {v:.1%}" for c, v in res["excluded"].items())
                 + f"; folded envs reporting a force {res['loaded_folded']:.1%}")
    lines.append(f"[{tag}] ground-set envs with a non-adjacent pair inside the margin (L4, L5 not read there): "
                 + ", ".join(f"{c} {v:.1%}" for c, v in res["self_near"].items()))
    for substep in (1, 4):
        if res["l5"].shape[1] >= substep and np.isfinite(res["l5"][0, substep - 1]).any():
            ratio, cos = l5_smallest(res, substep)
            lines.append(f"[{tag}] L5 sliding, substep {substep}: smallest |sum F_xy| / sum mu_d F_z {ratio:.6f}, smallest cosine "
                         f"against -v {cos:.6f} ({int(np.isfinite(res['l5'][0, substep - 1]).sum())} loaded envs)")
    if res["l6"]:
        a = np.array(res["l6"])
        lines.append(f"[{tag}] L6 one link: the line of action passes within {a[:, 2].max() * 1e3:.2f} mm of the lowest point "
                     f"inside the slab ({len(a)} loaded envs)")
    return "\n".join(lines)
