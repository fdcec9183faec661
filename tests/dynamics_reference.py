"""Float64 restatement of one contact-free physics substep from the
authored data alone. TEST INFRASTRUCTURE ONLY.

The equations are d'Alembert's / Kane's over the 12 authored links: each link's mass, COM and inertia
tensor come from ``RobotModel.raw["links"]``, its world COM and rotation from ``RobotModel.fk``. Nothing
is read from the composites (``body_mass`` / ``body_com`` / ``body_inertia``), from ``pack_model``'s
mass rows or from the oracle; the packed model gives only the five actuator / limit scalars, so that
the reference sees the float32 values the simulators see.

Generalised velocity u = [v_root(3), omega_root(3), qdot(6)], world frame, v of the root-link origin:
the state's own convention. With the partial velocities Jv_i, Jw_i of link i's COM and frame,

    M = sum_i m_i Jv_i^T Jv_i + Jw_i^T I_i Jw_i
    C = sum_i Jv_i^T m_i (Jv_i' u - g) + Jw_i^T (I_i Jw_i' u + w_i x I_i w_i)
    M udot + C = tau

J is the plain geometric Jacobian (joint axes and origins from fk's body frames); ``jac="fd"`` takes
central differences of fk along each generalised direction instead (root rotation by the exponential
map) for the J of M and of the projections. J' u is a (five-point) central difference of the geometric J along the
kinematic motion (pose + h u, quaternion exp(h omega) q; h = 1e-4 of pose travel, i.e. 1e-4 / |u| of
time once |u| > 1).

A per-env base inertia is given as ``base=(mass, com_offset, recompute_inertia)`` and applied to the
base link's own authored entry by Isaac Lab's rule (mass replaced, COM moved in the link frame, tensor
about the COM scaled by mass / authored mass when recomputed): not read back from the re-summed
composite of ``with_base_inertia``.

``mutant=`` plants one error (sensitivity tests): see MUTANTS.
"""
from __future__ import annotations

import functools

import numpy as np

from zbot_lab_amd import model as zm

S = zm.S
NL, ND, NV = zm.NUM_LINKS, zm.NUM_DOF, 6 + zm.NUM_DOF
NPHYS = S["P_DELTA"]          # the physics rows ROOT_POS .. JOINT_VEL
TWO_PI = 2.0 * np.pi
EPS_J, EPS_JDOT = 1e-6, 1e-4  # steps of the finite-difference Jacobian and of J' u
MUTANTS = {
    "inertia": "one link's inertia tensor x 1.01",
    "com": "one link's COM moved 1 mm",
    "no_gyro": "w x I w dropped",
    "no_jdot": "J' u dropped",
    "no_armature": "armature omitted",
    "kd_only": "kd in place of kd + dt kp",
    "root_gravity": "gravity on the root link only",
}


def skew(v):
    v = np.asarray(v, np.float64)
    o = np.zeros(v.shape[:-1] + (3, 3))
    o[..., 0, 1], o[..., 0, 2] = -v[..., 2], v[..., 1]
    o[..., 1, 0], o[..., 1, 2] = v[..., 2], -v[..., 0]
    o[..., 2, 0], o[..., 2, 1] = -v[..., 1], v[..., 0]
    return o


def expq(w):
    """Unit quaternion (w, x, y, z) of the rotation vector ``w`` (exact exponential map)."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th < 1e-12:
        return zm.qnorm(np.array([1.0, 0.5 * w[0], 0.5 * w[1], 0.5 * w[2]]))
    return np.concatenate([[np.cos(0.5 * th)], np.sin(0.5 * th) / th * w])


def rotvec(R):
    """Rotation vector of a rotation matrix near the identity (the finite-difference path)."""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(v)
    return v if s < 1e-12 else v * (np.arcsin(min(s, 1.0)) / s)


class Reference:
    def __init__(self, rm: zm.RobotModel, sim_dt: float, gravity: float, base=None, mutant: str | None = None,
                 mutant_link: int | None = None, round_model: bool = False):
        if mutant is not None and mutant not in MUTANTS:
            raise ValueError(f"mutant {mutant!r}: one of {sorted(MUTANTS)}")
        self.rm, self.dt, self.mutant = rm, float(sim_dt), mutant
        pm = zm.pack_model(rm)
        self.kp, self.kd, self.effort = float(pm.kp), float(pm.kd), float(pm.effort_limit)
        self.vlim, self.wmax = float(pm.velocity_limit), float(pm.max_angular_velocity)
        links = rm.raw["links"]
        assert [l["name"] for l in links] == list(rm.link_names)
        self.mass = np.array([l["mass"] for l in links], np.float64)
        self.com = np.array([l["com"] for l in links], np.float64)            # link frame
        self.I = np.zeros((NL, 3, 3))                                        # about the COM, link frame
        for i, l in enumerate(links):
            Rpa = zm.qmat(zm.qnorm(l["principal_axes_wxyz"]))
            self.I[i] = Rpa @ np.diag(np.asarray(l["diag_inertia"], np.float64)) @ Rpa.T
        if base is not None:
            mass, offset, recompute = (*base, True)[:3]
            b = rm.base_link
            if recompute:
                self.I[b] = self.I[b] * (float(mass) / self.mass[b])
            self.mass[b] = float(mass)
            self.com[b] = self.com[b] + np.asarray(offset, np.float64)
        if round_model:
            # every authored value and every frame entry moved by float32's unit roundoff 2^-24 (relative,
            # random sign), the size of the error a float32 model table may carry on each entry: how far
            # that alone moves a substep (the bound of the packed-model tests). Rounding the inputs
            # themselves would say too little: the v2 asset's masses and COMs are float32 values already,
            # while the packed composites are new float64 sums rounded once more.
            import copy
            prng = np.random.default_rng(24)
            r32 = lambda a: np.asarray(a, np.float64) * (1.0 + 2.0 ** -24 * prng.choice([-1.0, 1.0], np.shape(a)))  # noqa: E731
            self.mass, self.com, self.I = r32(self.mass), r32(self.com), r32(self.I)
            self.I = 0.5 * (self.I + np.transpose(self.I, (0, 2, 1)))
            rm = self.rm = copy.copy(rm)
            rm.joints = [{**j, **{k: zm.Xf(r32(j[k].p), zm.qnorm(r32(j[k].q))) for k in ("parent_xf", "child_xf")}}
                         for j in rm.joints]
            rm.link_xf = [zm.Xf(r32(x.p), zm.qnorm(r32(x.q))) for x in rm.link_xf]
        k = rm.base_link + 2 if mutant_link is None else mutant_link
        if mutant == "inertia":
            self.I[k] = 1.01 * self.I[k]
        if mutant == "com":
            self.com[k] = self.com[k] + np.array([1e-3, 0.0, 0.0])
        self.g = np.array([0.0, 0.0, -float(gravity)])
        self.gmask = np.ones(NL)
        if mutant == "root_gravity":   # the chain root: the link of body 0 whose frame is the body's
            root = next(i for i in range(NL) if rm.link_body[i] == 0)
            self.gmask[:] = 0.0
            self.gmask[root] = 1.0
        self.link_body = np.asarray(rm.link_body)
        self.affects = (np.arange(ND)[None, :] < self.link_body[:, None]).astype(np.float64)   # joint j moves link i

    # ------------------------------------------------------------------ kinematics
    def kin(self, pos, quat, q):
        """World COM c [12,3] and rotation R [12,3,3] of every link, joint axes and origins [6,3] (fk)."""
        bodies, links = self.rm.fk(pos, quat, q)
        c = np.zeros((NL, 3))
        R = np.zeros((NL, 3, 3))
        for i, X in enumerate(links):
            R[i] = zm.qmat(X.q)
            c[i] = X.p + R[i] @ self.com[i]
        axis = np.zeros((ND, 3))
        org = np.zeros((ND, 3))
        for j, jt in enumerate(self.rm.joints):
            F = bodies[j] * jt["parent_xf"]
            axis[j], org[j] = zm.qmat(F.q)[:, 2], F.p
        return c, R, axis, org

    @staticmethod
    def advance(pos, quat, q, u, eps):
        """The pose moved along the generalised velocity ``u`` by ``eps``."""
        return (np.asarray(pos, np.float64) + eps * u[0:3], zm.qnorm(zm.qmul(expq(eps * u[3:6]), zm.qnorm(quat))),
                np.asarray(q, np.float64) + eps * u[6:])

    def jac_geometric(self, pos, quat, q):
        c, R, axis, org = self.kin(pos, quat, q)
        Jv = np.zeros((NL, 3, NV))
        Jw = np.zeros((NL, 3, NV))
        Jv[:, :, 0:3] = np.eye(3)
        Jv[:, :, 3:6] = -skew(c - np.asarray(pos, np.float64))
        Jw[:, :, 3:6] = np.eye(3)
        lever = np.cross(axis[None, :, :], c[:, None, :] - org[None, :, :])          # [12, 6, 3]
        Jv[:, :, 6:] = np.transpose(lever, (0, 2, 1)) * self.affects[:, None, :]
        Jw[:, :, 6:] = axis.T[None, :, :] * self.affects[:, None, :]
        return Jv, Jw, c, R

    def jac_fd(self, pos, quat, q, eps=EPS_J):
        c, R, _, _ = self.kin(pos, quat, q)
        Jv = np.zeros((NL, 3, NV))
        Jw = np.zeros((NL, 3, NV))
        for k in range(NV):
            e = np.zeros(NV)
            e[k] = 1.0
            # about the root origin (the differences do not see a translation): |c| stays ~0.3 m
            cp, Rp, _, _ = self.kin(*self.advance(np.zeros(3), quat, q, e, eps))
            cm, Rm, _, _ = self.kin(*self.advance(np.zeros(3), quat, q, e, -eps))
            Jv[:, :, k] = (cp - cm) / (2 * eps)
            for i in range(NL):
                Jw[i, :, k] = rotvec(Rp[i] @ Rm[i].T) / (2 * eps)
        return Jv, Jw, c, R

    def jac(self, pos, quat, q, jac="geometric", eps_j=EPS_J):
        return self.jac_geometric(pos, quat, q) if jac == "geometric" else self.jac_fd(pos, quat, q, eps_j)

    # ------------------------------------------------------------------ M and C
    def dynamics(self, pos, quat, q, u, jac="geometric", eps_j=EPS_J, eps_jdot=EPS_JDOT):
        """M [12,12], C [12] and the per-link terms they were summed from."""
        u = np.asarray(u, np.float64)
        Jv, Jw, c, R = self.jac(pos, quat, q, jac, eps_j)
        # eps_jdot is the pose travel (m, rad) of the difference: at |u| > 1 the time step shrinks with
        # the speed, or the truncation error (step^2 |u|^3) of a 15 rad/s state would reach 1e-5
        h = eps_jdot / max(1.0, float(np.linalg.norm(u)))
        # always of the geometric Jacobian: a difference of finite-difference Jacobians (step 1e-6) would
        # carry their rounding noise, 1e-10, divided by h
        def diff(k):
            Jvp, Jwp, _, _ = self.jac_geometric(*self.advance(pos, quat, q, u, k * h))
            Jvm, Jwm, _, _ = self.jac_geometric(*self.advance(pos, quat, q, u, -k * h))
            return (Jvp - Jvm) @ u, (Jwp - Jwm) @ u

        (v1, w1), (v2, w2) = diff(1), diff(2)          # the five-point central difference
        jdv = (8.0 * v1 - v2) / (12.0 * h)             # [12, 3]
        jdw = (8.0 * w1 - w2) / (12.0 * h)
        Iw = R @ self.I @ np.transpose(R, (0, 2, 1))
        om = Jw @ u
        gyro = np.cross(om, np.einsum("iab,ib->ia", Iw, om))
        M = np.einsum("i,iak,ial->kl", self.mass, Jv, Jv) + np.einsum("iak,iab,ibl->kl", Jw, Iw, Jw)
        jdv_c, jdw_c = (0.0 * jdv, 0.0 * jdw) if self.mutant == "no_jdot" else (jdv, jdw)
        gyro_c = 0.0 * gyro if self.mutant == "no_gyro" else gyro
        lin = self.mass[:, None] * (jdv_c - self.gmask[:, None] * self.g[None, :])
        ang = np.einsum("iab,ib->ia", Iw, jdw_c) + gyro_c
        C = np.einsum("iak,ia->k", Jv, lin) + np.einsum("iak,ia->k", Jw, ang)
        return dict(M=M, C=C, Jv=Jv, Jw=Jw, jdv=jdv, jdw=jdw, c=c, Iw=Iw, om=om, gyro=gyro)

    # ------------------------------------------------------------------ one substep of one env
    def substep(self, x, target, **kw):
        """x: the 25 physics rows of one env (float64). Returns (new rows, info)."""
        dt, kp, kd, eff = self.dt, self.kp, self.kd, self.effort
        x = np.asarray(x, np.float64)
        pos, quat = x[S["ROOT_POS"]:S["ROOT_POS"] + 3], zm.qnorm(x[S["ROOT_QUAT"]:S["ROOT_QUAT"] + 4])
        q, qd = x[S["JOINT_POS"]:S["JOINT_POS"] + ND], x[S["JOINT_VEL"]:S["JOINT_VEL"] + ND]
        u = np.concatenate([x[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3], x[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3], qd])
        target = np.asarray(target, np.float64)
        applied = np.clip(kp * (target - q) - kd * qd, -eff, eff)
        d = self.dynamics(pos, quat, q, u, **kw)
        M, C = d["M"], d["C"]
        arm = 0.0 if self.mutant == "no_armature" else dt * kd + dt * dt * kp
        force = kp * (target - q) - (kd if self.mutant == "kd_only" else kd + dt * kp) * qd

        def solve(sat):
            A = np.zeros(NV)
            A[6:] = np.where(sat != 0, 0.0, arm)
            tau = np.zeros(NV)
            tau[6:] = np.where(sat != 0, sat * eff, force)
            return u + np.linalg.solve(M + np.diag(A), dt * (tau - C))

        u1 = solve(np.zeros(ND))
        tau_impl = force - (arm / dt) * (u1[6:] - qd)
        sat = np.where(tau_impl > eff, 1, np.where(tau_impl < -eff, -1, 0))
        if sat.any():
            u1 = solve(sat)
        # clamps: joint speeds, then the root angular velocity as a vector
        pre_qd, pre_w = u1[6:].copy(), np.linalg.norm(u1[3:6])
        clamp = np.where(pre_qd > self.vlim, 1, np.where(pre_qd < -self.vlim, -1, 0))
        u1[6:] = np.clip(u1[6:], -self.vlim, self.vlim)
        cap = bool(pre_w > self.wmax)
        if cap:
            u1[3:6] *= self.wmax / pre_w
        # pose
        qn = q + dt * u1[6:]
        wrap = np.where(qn > TWO_PI, 1, np.where(qn < -TWO_PI, -1, 0))
        pre_q = qn.copy()
        qn = qn - wrap * 2 * TWO_PI
        y = np.zeros(NPHYS)
        y[S["ROOT_POS"]:S["ROOT_POS"] + 3] = pos + dt * u1[0:3]
        y[S["ROOT_QUAT"]:S["ROOT_QUAT"] + 4] = zm.qnorm(zm.qmul(expq(dt * u1[3:6]), quat))
        y[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3] = u1[0:3]
        y[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3] = u1[3:6]
        y[S["JOINT_POS"]:S["JOINT_POS"] + ND] = qn
        y[S["JOINT_VEL"]:S["JOINT_VEL"] + ND] = u1[6:]
        info = dict(applied=applied, sat=sat, clamp=clamp, cap=cap, wrap=wrap,
                    # relative distance of each decision from its threshold
                    sat_margin=np.abs(np.abs(tau_impl) - eff) / eff, clamp_margin=np.abs(np.abs(pre_qd) - self.vlim) / self.vlim,
                    cap_margin=abs(pre_w - self.wmax) / self.wmax, wrap_margin=np.abs(np.abs(pre_q) - TWO_PI) / TWO_PI)
        return y, info

    # ------------------------------------------------------------------ many envs, many substeps
    def run(self, rows, targets, nsub=1, **kw):
        """rows [25, n] (the physics rows ROOT_POS .. JOINT_VEL), targets [n, 6]. The reference keeps its
        own float64 state between the substeps. Returns a dict of arrays: ``states`` [nsub, 25, n] after
        each substep, ``applied`` [n, 6] at the start of the last one, and per substep ``sat`` / ``clamp`` /
        ``wrap`` [nsub, n, 6] (sign, 0 = not), ``cap`` [nsub, n] and the ``*_margin`` arrays."""
        rows = np.asarray(rows, np.float64)[:NPHYS]
        n = rows.shape[1]
        out = dict(states=np.zeros((nsub, NPHYS, n)), applied=np.zeros((n, ND)),
                   sat=np.zeros((nsub, n, ND), int), clamp=np.zeros((nsub, n, ND), int), wrap=np.zeros((nsub, n, ND), int),
                   cap=np.zeros((nsub, n), bool), sat_margin=np.zeros((nsub, n, ND)), clamp_margin=np.zeros((nsub, n, ND)),
                   wrap_margin=np.zeros((nsub, n, ND)), cap_margin=np.zeros((nsub, n)))
        for e in range(n):
            x = rows[:, e]
            for k in range(nsub):
                x, info = self.substep(x, targets[e], **kw)
                out["states"][k, :, e] = x
                for name in ("sat", "clamp", "wrap", "cap", "sat_margin", "clamp_margin", "wrap_margin", "cap_margin"):
                    out[name][k, e] = info[name]
            out["applied"][e] = info["applied"]
        return out

    # ------------------------------------------------------------------ the reference against itself
    def momentum_balance(self, x, tau_joint):
        """With udot = M^-1 (tau - C) for joint torques ``tau_joint``: (sum m_i a_i, m_total g) and
        (sum c_i x m_i a_i + I_i alpha_i + w_i x I_i w_i, sum c_i x m_i g) about the world origin."""
        x = np.asarray(x, np.float64)
        pos, quat = x[S["ROOT_POS"]:S["ROOT_POS"] + 3], zm.qnorm(x[S["ROOT_QUAT"]:S["ROOT_QUAT"] + 4])
        q, qd = x[S["JOINT_POS"]:S["JOINT_POS"] + ND], x[S["JOINT_VEL"]:S["JOINT_VEL"] + ND]
        u = np.concatenate([x[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3], x[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3], qd])
        d = self.dynamics(pos, quat, q, u)
        tau = np.zeros(NV)
        tau[6:] = tau_joint
        ud = np.linalg.solve(d["M"], tau - d["C"])
        a = d["Jv"] @ ud + d["jdv"]
        al = d["Jw"] @ ud + d["jdw"]
        ma = self.mass[:, None] * a
        force = ma.sum(0)
        moment = (np.cross(d["c"], ma) + np.einsum("iab,ib->ia", d["Iw"], al) + d["gyro"]).sum(0)
        return (force, self.mass.sum() * self.g), (moment, np.cross(d["c"], self.mass[:, None] * self.g[None, :]).sum(0))


def ulp32(x):
    """Spacing of float32 at max(|x|, 1), as float64."""
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float64)), 1.0).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------- case sets
CASE_SETS = ("generic", "gyroscopic", "saturated", "speed_clamp", "angular_cap", "wrap")


def _unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _quiet_saturated(rm, nq, rng, pose, vlim, batch=48, max_batches=40):
    """``nq`` states (poses taken from ``pose`` [25, nq]) in which the reference saturates one mid-chain
    joint, half of them with each sign, at least 1e-3 (relative) past the threshold, and neither clamps a
    joint nor caps the root in the same substep. Returns (rows [25, nq], targets [nq, 6]), float64."""
    ref = Reference(rm, float(np.float32(1.0 / 200.0)), float(np.float32(9.81)))
    rows, tgs, want = [], [], {1: nq - nq // 2, -1: nq // 2}
    for _ in range(max_batches):
        st = np.zeros((NPHYS, batch))
        st[:S["ROOT_LINVEL"]] = pose[:S["ROOT_LINVEL"], rng.integers(0, nq, batch)]
        st[S["ROOT_LINVEL"]:S["JOINT_POS"]] = 0.2 * rng.normal(size=(6, batch))
        q = rm.default_joint_pos[:, None] + rng.uniform(-0.5, 0.5, (ND, batch))
        qd = 0.2 * rng.normal(size=(ND, batch))
        tg = (q + rng.uniform(-0.3, 0.3, (ND, batch))).T
        joint, sign, e = rng.integers(2, 4, batch), rng.choice([-1, 1], batch), np.arange(batch)
        tg[e, joint] = q[joint, e] + sign * rng.uniform(2.0, 3.0, batch)
        qd[joint, e] = -sign * rng.uniform(0.72, 0.9, batch) * vlim
        st[S["JOINT_POS"]:S["JOINT_POS"] + ND], st[S["JOINT_VEL"]:S["JOINT_VEL"] + ND] = q, qd
        st, tg = st.astype(np.float32).astype(np.float64), tg.astype(np.float32).astype(np.float64)
        r = ref.run(st, tg, 1)
        for i in range(batch):
            sat = r["sat"][0, i]
            ok = (sat[joint[i]] == sign[i] and not r["clamp"][0, i].any() and not r["cap"][0, i]
                  and r["sat_margin"][0, i].min() > 1e-3 and r["clamp_margin"][0, i].min() > 1e-3 and r["cap_margin"][0, i] > 1e-3)
            if ok and want[int(sign[i])] > 0:
                want[int(sign[i])] -= 1
                rows.append(st[:, i])
                tgs.append(tg[i])
        if len(rows) == nq:
            return np.array(rows).T, np.array(tgs)
    raise RuntimeError(f"quiet saturated states: {len(rows)} of {nq} found")


@functools.lru_cache(maxsize=None)
def _case_states(rm_key, case, n, seed, lift):
    return _build_case_states(_RM[rm_key], case, n, seed, lift)


_RM: dict = {}


def case_states(rm: zm.RobotModel, case: str, n: int, seed: int = 0, lift: float = 2.0):
    """Cached by model identity; see _build_case_states. Returns fresh copies."""
    _RM[id(rm)] = rm
    st, tg = _case_states(id(rm), case, n, seed, lift)
    return st.copy(), tg.copy()


def _build_case_states(rm: zm.RobotModel, case: str, n: int, seed: int = 0, lift: float = 2.0):
    """(rows [25, n] float32, targets [n, 6] float32) of one case set; the robot is lifted ``lift`` m
    above its default height, so no link reaches the ground. The condition each set is named for is
    asserted by the tests on the reference's own outcome, not assumed here.

    generic      random orientation, root and joint speeds ~ 1, targets within 0.3 rad of the pose
    gyroscopic   root |omega| in (0.6, 0.97) x the cap, joint speeds up to 15 rad/s
    saturated    the two mid-chain joints: targets 2-3 rad away, speeds 3-8 rad/s opposing the offset
                 (a light outer link accelerates out of saturation within the implicit solve)
                 The first quarter of the set: one mid-chain joint alone, at 0.72-0.9 of the speed
                 limit, everything else slow, kept when the reference saturates it without any clamp.
    speed_clamp  the four other joints at 0.975-0.9995 of the speed limit, targets 2.6-3 rad ahead (the drive
                 pushes them past the limit without saturating)
    angular_cap  root |omega| in (0.97, 0.9999) x the cap, joint speeds up to 5 (the bias pushes about
                 half of them past the cap)
    wrap         joints within one substep's travel of +-2 pi, moving outward at 2-6 rad/s
    """
    pm = zm.pack_model(rm)
    vlim, wmax = float(pm.velocity_limit), float(pm.max_angular_velocity)
    rng = np.random.default_rng([seed, CASE_SETS.index(case)])
    st = np.zeros((NPHYS, n))
    st[S["ROOT_POS"]:S["ROOT_POS"] + 3] = rm.default_root_pos[:, None] + rng.uniform(-0.5, 0.5, (3, n))
    st[S["ROOT_POS"] + 2] += lift
    st[S["ROOT_QUAT"]:S["ROOT_QUAT"] + 4] = _unit_quats(rng, n).T
    q = rm.default_joint_pos[None, :] + rng.uniform(-0.5, 0.5, (n, ND))
    v = rng.normal(size=(n, 3))
    w = rng.normal(size=(n, 3))
    qd = rng.normal(size=(n, ND))
    tg = q + rng.uniform(-0.3, 0.3, (n, ND))
    sign = rng.choice([-1.0, 1.0], size=(n, ND))
    direction = w / np.linalg.norm(w, axis=1, keepdims=True)
    inner = np.zeros(ND, bool)
    inner[2:4] = True        # the two mid-chain joints: each carries half the robot
    if case == "gyroscopic":
        w = direction * rng.uniform(0.6, 0.97, (n, 1)) * wmax
        qd = rng.uniform(-15.0, 15.0, (n, ND))
    elif case == "saturated":
        tg = np.where(inner, q + sign * rng.uniform(2.0, 3.0, (n, ND)), tg)
        qd = np.where(inner, -sign * rng.uniform(3.0, 8.0, (n, ND)), qd)
        # the first quarter: one mid-chain joint saturates and nothing is clamped or capped in that
        # substep, so that the saturation can be read back from the velocity change (drawn until the
        # reference on the nominal robot says so: 6 % of the draws on the manager robot)
        nq = max(4, n // 4)
        qs, qt = _quiet_saturated(rm, nq, rng, st[:, :nq], vlim)
        st[:S["ROOT_LINVEL"], :nq] = qs[:S["ROOT_LINVEL"]]
        v[:nq], w[:nq] = qs[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3].T, qs[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3].T
        q[:nq], qd[:nq], tg[:nq] = qs[S["JOINT_POS"]:S["JOINT_POS"] + ND].T, qs[S["JOINT_VEL"]:S["JOINT_VEL"] + ND].T, qt
    elif case == "speed_clamp":
        outer = ~inner
        qd = np.where(outer, sign * rng.uniform(0.975, 0.9995, (n, ND)) * vlim, qd)
        tg = np.where(outer, q + sign * rng.uniform(2.6, 3.0, (n, ND)), tg)
    elif case == "angular_cap":
        w = direction * rng.uniform(0.97, 0.9999, (n, 1)) * wmax
        qd = rng.uniform(-5.0, 5.0, (n, ND))
    elif case == "wrap":
        speed = rng.uniform(2.0, 6.0, (n, ND))
        q = sign * (TWO_PI - rng.uniform(0.05, 0.95, (n, ND)) * speed * 0.005)
        qd = sign * speed
        tg = q + sign * rng.uniform(0.0, 0.2, (n, ND))
    elif case != "generic":
        raise ValueError(case)
    st[S["ROOT_LINVEL"]:S["ROOT_LINVEL"] + 3] = v.T
    st[S["ROOT_ANGVEL"]:S["ROOT_ANGVEL"] + 3] = w.T
    st[S["JOINT_POS"]:S["JOINT_POS"] + ND] = q.T
    st[S["JOINT_VEL"]:S["JOINT_VEL"] + ND] = qd.T
    return st.astype(np.float32), tg.astype(np.float32)


def mixed_states(rm: zm.RobotModel, n: int, seed: int = 0):
    """``n`` distinct states, the six case sets in turn (env e is of set e % 6)."""
    per = -(-n // len(CASE_SETS))
    rows = np.zeros((NPHYS, n), np.float32)
    tg = np.zeros((n, ND), np.float32)
    for k, case in enumerate(CASE_SETS):
        st, t = case_states(rm, case, per, seed)
        idx = np.arange(k, n, len(CASE_SETS))
        rows[:, idx], tg[idx] = st[:, :len(idx)], t[:len(idx)]
    return rows, tg
