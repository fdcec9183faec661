"""The random draws of every task's events, recovered from a simulator's state and observations, and
the law checks on them: shared by the CPU oracle tests (tests/test_random_laws.py) and the device
tests (tests/test_gpu_random_streams.py), which run the same scenarios through two backends.

Draw-index map (``draw(env_hash(seed, ctr, env), k)``; csrc/sim_standup.h and oracle/zbot_oracle.c):
reset pose 1..4 (x, y, roll, yaw); reset command 5..7 (v4: sign, velocity, yaw; manager: lin x,
lin y, standing); v4 command interval 8; interval command 9..11; manager observation noise 16..31;
the full-reset episode length is ``env_hash % max_episode_length`` itself.
"""
from __future__ import annotations

import numpy as np

from random_laws import Laws
from zbot_lab_amd import model as zm

N_RESET, N_STEP = 65536, 16384   # envs of the reset / observe-only scenarios, and where a step is needed
SEED_FLIP = 1 << 32              # seed s against s ^ 2^32: the high word reaches the stream


# ----------------------------------------------------------------------------- backends
class OracleBackend:
    """The CPU oracle. Its noise-free manager observation is a twin sim with obs_corruption off and
    the same seed: the noise never feeds back into the state, so the twin's state is the same."""
    name = "oracle"

    def __init__(self, cfg, n, seed, clean: bool = False):
        from oracle.pyoracle import OracleSim
        self.cfg, self.n = cfg, n
        self.s = OracleSim(n, cfg, seed=seed)
        self.twin = None
        if clean:
            import dataclasses
            self.twin = OracleSim(n, dataclasses.replace(cfg, obs_corruption=False), seed=seed)

    def _both(self):
        return [self.s] + ([self.twin] if self.twin else [])

    def state(self):
        return self.s.get_state()

    def rows(self, lo, hi):
        return self.s.get_state()[lo:hi]

    def set_state(self, st):
        for s in self._both():
            s.set_state(st)

    def reset(self):
        for s in self._both():
            s.reset()

    def step(self, a):
        out = [s.step(a) for s in self._both()]
        obs, _, term, trunc = out[0]
        return obs, (out[1][0] if self.twin else None), term | trunc

    def observe(self):
        return self.s.observe(), (self.twin.observe() if self.twin else None)


class DeviceBackend:
    """libzbot.so on the GPU; the noise-free observation is the policy block of the critic row."""
    name = "device"

    def __init__(self, cfg, n, seed, clean: bool = False):
        from zbot_lab_amd.sim import ZbotSim
        self.cfg, self.n, self.clean = cfg, n, clean
        self.s = ZbotSim(n, cfg, device="cuda:0", seed=seed)

    def state(self):
        return self.s.get_state().cpu().numpy()

    def rows(self, lo, hi):
        return self.s.get_state()[lo:hi].cpu().numpy()

    def set_state(self, st):
        import torch
        self.s.set_state(torch.from_numpy(np.ascontiguousarray(st, np.float32)).cuda())

    def reset(self):
        self.s.reset(None)

    def _clean(self):
        return self.s.observe_critic()[:, :self.cfg.obs_dim].cpu().numpy() if self.clean else None

    def step(self, a):
        import torch
        obs, _, term, trunc = self.s.step(torch.from_numpy(a).cuda())
        done = (term | trunc).cpu().numpy()
        return obs.cpu().numpy(), self._clean(), done

    def observe(self):
        return self.s.observe().cpu().numpy(), self._clean()


# ----------------------------------------------------------------------------- recovery
def _qmul(a, b):
    w1, x1, y1, z1 = a.T
    w2, x2, y2, z2 = b.T
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=1)


def _qconj(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def _robot(cfg):
    return (zm.standup_model() if cfg.task == zm.TASK_STANDUP_V0
            else zm.load_v09_model() if cfg.task == zm.TASK_MANAGER_V0 else zm.load_model())


def pose_draws(cfg, st) -> dict:
    """The samples (x, y, roll, yaw) of reset_root_state_uniform from the root pose rows of a state
    [state_dim][n], as test_reset_draws_in_range does for the roll: the delta rotation is
    quat_from_euler_xyz(roll, 0, yaw) = (cy cr, cy sr, sy sr, sy cr), applied on the Isaac Lab root's
    default pose in the world or the body frame; x and y are added to the position, so they are the
    state's position minus the position the oracle's own pose map gives for (0, 0, roll, yaw)."""
    from oracle import pyoracle
    robot = _robot(cfg)
    pos = st[0:3].T.astype(np.float64)
    quat = st[3:7].T.astype(np.float64)
    n = len(pos)
    _, q0 = pyoracle.su_pose_from_samples(np.zeros((1, 4), np.float32), cfg.reset_pose_body_frame, robot)
    q0 = np.repeat(q0.astype(np.float64), n, axis=0)
    qT = np.repeat(np.asarray(robot.api_root_in_root[1], np.float64)[None], n, axis=0)
    if cfg.reset_pose_body_frame:   # qn = q0 qT dq conj(qT)
        d = _qmul(_qmul(_qconj(qT), _qmul(_qconj(q0), quat)), qT)
    else:                           # qn = dq q0
        d = _qmul(quat, _qconj(q0))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= np.where(d[:, :1] < 0, -1.0, 1.0)
    sgn = np.where(d[:, 1] * d[:, 0] + d[:, 2] * d[:, 3] < 0, -1.0, 1.0)
    roll = 2.0 * np.arctan2(sgn * np.hypot(d[:, 1], d[:, 2]), np.hypot(d[:, 0], d[:, 3]))
    cr, sr = np.cos(0.5 * roll), np.sin(0.5 * roll)
    yaw = 2.0 * np.arctan2(d[:, 3] * cr + d[:, 2] * sr, d[:, 0] * cr + d[:, 1] * sr)
    smp = np.zeros((n, 4), np.float32)
    smp[:, 2], smp[:, 3] = roll, yaw
    p0, _ = pyoracle.su_pose_from_samples(smp, cfg.reset_pose_body_frame, robot)
    return dict(x=pos[:, 0] - p0[:, 0], y=pos[:, 1] - p0[:, 1], roll=roll, yaw=yaw)


POSE_SLACK = 2e-6   # fp32 rounding of the recovered pose samples (the parity tests' state tolerance)


def check_pose(L: Laws, tag, cfg, d):
    """Each sample against U(cfg.reset_pose_range[k]); a degenerate range is a point."""
    live = {}
    for k, name in enumerate(("x", "y", "roll", "yaw")):
        lo, hi = cfg.reset_pose_range[k]
        if hi > lo:
            # x, y: a difference of O(1) fp32 positions; roll, yaw: through a unit quaternion
            L.uniform(f"{tag} {name}", d[name], lo, hi, grain=1.2e-7 / (hi - lo), slack=POSE_SLACK)
            live[name] = d[name]
        else:
            L.exact(f"{tag} {name} is {lo}", bool(np.abs(d[name] - lo).max() <= POSE_SLACK))
    return live


def v4_command_draws(st):
    V = zm.V4
    c0 = st[V["COMMANDS"]].astype(np.float64)
    return dict(speed=np.abs(c0), sign=(c0 > 0).astype(np.float64), cyaw=st[V["COMMANDS"] + 1].astype(np.float64))


def check_v4_commands(L, tag, cfg, prob_pos, d):
    L.uniform(f"{tag} speed", d["speed"], *cfg.cmd_vel_range, grain=1.2e-7)
    L.bernoulli(f"{tag} sign", d["sign"], prob_pos)
    L.uniform(f"{tag} yaw command", d["cyaw"], *cfg.cmd_yaw_range, grain=1.2e-7)


def m_command_draws(st):
    M = zm.M
    return dict(lin_x=st[M["COMMANDS"]].astype(np.float64), lin_y=st[M["COMMANDS"] + 1].astype(np.float64),
                standing=st[M["CMD_STANDING"]].astype(np.float64))


NOISE_COLS = list(range(0, 4)) + list(range(7, 19))   # quat, joint pos, joint vel (draws 16..31)


def m_noise(cfg, obs, clean):
    """{column: noise / half-width} of the 16 noisy columns, and the largest |obs - clean| elsewhere."""
    d = obs.astype(np.float64) - clean.astype(np.float64)
    hw = {c: cfg.obs_noise[0 if c < 4 else 1 if c < 13 else 2] for c in NOISE_COLS}
    quiet = [c for c in range(obs.shape[1]) if c not in NOISE_COLS]
    return {f"noise{c}": d[:, c] / hw[c] for c in NOISE_COLS}, float(np.abs(d[:, quiet]).max())


NOISE_CLASSES = {"quat": [f"noise{c}" for c in range(0, 4)], "joint pos": [f"noise{c}" for c in range(7, 13)],
                 "joint vel": [f"noise{c}" for c in range(13, 19)]}   # one half-width each (cfg.obs_noise)
NOISE_GRAIN = 1.2e-5   # obs and clean are fp32 roundings of O(1) values: 1.2e-7 / half-width 0.01


def check_noise(L, tag, calls, quiet):
    """``calls``: the {column: noise / half-width} dicts of one or more calls. Each column of the first
    call against U(-1, 1) (Kolmogorov-Smirnov and width; the granularity rules the extremes out), its
    16 x 16 correlation, and each half-width class pooled over its columns and over the calls, which is
    what resolves a 2 % error of a half-width (tests/test_random_laws.py plants it under this function)."""
    L.exact(f"{tag}: non-noisy columns carry exactly no noise ({quiet})", quiet == 0.0)
    for name, v in calls[0].items():
        L.uniform(f"{tag} {name}", v, -1.0, 1.0, grain=NOISE_GRAIN, slack=2 * NOISE_GRAIN)
    L.uncorrelated(f"{tag} 16x16", calls[0])
    for cls, cols in NOISE_CLASSES.items():
        pooled = np.concatenate([c[k] for c in calls for k in cols])
        L.uniform(f"{tag} {cls} half-width class, {len(calls)} call(s) pooled", pooled, -1.0, 1.0, grain=NOISE_GRAIN,
                  slack=2 * NOISE_GRAIN)


def fresh_all(L, tag, a: dict, b: dict, p_equal=None):
    """``p_equal``: {discrete column: P(two independent draws are equal)}; the other columns are continuous."""
    for k in a:
        if np.std(a[k]) > 0 and np.std(b[k]) > 0:
            L.fresh(f"{tag} {k}", a[k], b[k], p_equal=(p_equal or {}).get(k))


def p_equal_flag(p):
    return p * p + (1.0 - p) * (1.0 - p)


def serial_all(L, tag, d: dict):
    for k, v in d.items():
        if np.std(v) > 0:
            L.serial(f"{tag} {k}", v)


# ----------------------------------------------------------------------------- scenarios
# Each returns (Laws, draws) where draws is a dict of the recovered columns of the base seed (what
# the device test compares with the oracle's).
def standup_cfg():
    return zm.TaskCfg.standup()


def v4_cfg():
    """The product cfg with the two degenerate laws opened: the registered velocity range is the
    point 0.3 and the stage-0 sign probability is 1; 0.8 is the curriculum's stage-2 value."""
    return zm.TaskCfg.walking_v4(cmd_vel_range=(0.1, 0.3), cmd_prob_pos=0.8)


def manager_cfg(rel_standing=0.02):
    """The product cfg with the lin y range opened (registered: the point 0)."""
    return zm.TaskCfg.manager_flat(cmd_yaw_range=(-0.05, 0.05), cmd_rel_standing=rel_standing)


def _reset_columns(B, cfg, seed, n, extract, calls=2):
    """The draws of construction (counter 0) and of the following ``calls - 1`` full resets."""
    b = B(cfg, n, seed)
    out = [extract(b.state())]
    for _ in range(calls - 1):
        b.reset()
        out.append(extract(b.state()))
    return out


def _seed_and_call_checks(L, tag, B, cfg, seed, n, extract, base):
    """Serial correlation over the env index; call ctr against ctr + 1; seed s against s + 1 and
    against s ^ 2^32 (every column)."""
    serial_all(L, tag, base[0])
    fresh_all(L, f"{tag} call ctr / ctr+1", base[0], base[1])
    for name, s2 in (("seed s / s+1", seed + 1), ("seed s / s^2^32", seed ^ SEED_FLIP)):
        other = _reset_columns(B, cfg, s2, n, extract, calls=1)
        fresh_all(L, f"{tag} {name}", base[0], other[0])


def scenario_pose(B, cfg, seed, tag, n=N_RESET, full=True):
    """A reset pose on its own (stand-up; v4 and the manager check theirs with their commands): marginals, 4x4 correlation, env / call / seed independence.
    (Every scenario: ``full=False`` returns the first call's draws only, for the device / oracle comparison.)"""
    L = Laws()
    extract = lambda st: pose_draws(cfg, st)  # noqa: E731
    base = _reset_columns(B, cfg, seed, n, extract, calls=2 if full else 1)
    if not full:
        return None, base[0]
    live = [check_pose(L, f"{tag} pose call {c}", cfg, d) for c, d in enumerate(base)]
    for c, d in enumerate(live):
        L.uncorrelated(f"{tag} pose call {c}", d)
    names = list(live[0])   # the samples whose range is not a point
    _seed_and_call_checks(L, tag, B, cfg, seed, n, lambda st: {k: extract(st)[k] for k in names}, live)
    return L, base[0]


def scenario_v4_reset(B, seed, n=N_RESET, full=True):
    """v4 construction and reset: pose 1..4, command 5..7, interval 8 (construction only)."""
    cfg = v4_cfg()
    L = Laws()
    V = zm.V4

    def extract(st, roll=False):   # (roll: a point for this task; kept for the marginal check only)
        d = {k: v for k, v in pose_draws(cfg, st).items() if roll or k != "roll"}
        d.update(v4_command_draws(st))
        d["interval"] = st[V["INTERVAL_LEFT"]].astype(np.float64)
        return d
    base = _reset_columns(B, cfg, seed, n, lambda st: extract(st, roll=full), calls=2 if full else 1)
    if not full:
        return None, base[0]
    peq = {"sign": p_equal_flag(cfg.cmd_prob_pos)}
    for c, d in enumerate(base):
        check_pose(L, f"v4 reset call {c}", cfg, d | {"roll": d.pop("roll")})
        check_v4_commands(L, f"v4 reset call {c}", cfg, cfg.cmd_prob_pos, d)
    L.uniform("v4 construction interval", base[0]["interval"], *cfg.cmd_interval_s, grain=4.8e-7 / 3.0)
    L.exact("v4 reset keeps the interval timer", bool((base[1]["interval"] == base[0]["interval"]).all()))
    L.uncorrelated("v4 construction pose x command x interval", base[0])
    L.uncorrelated("v4 reset pose x command", {k: v for k, v in base[1].items() if k != "interval"})
    nointerval = lambda d: {k: v for k, v in d.items() if k != "interval"}  # noqa: E731
    serial_all(L, "v4", base[0])
    fresh_all(L, "v4 call ctr / ctr+1", nointerval(base[0]), nointerval(base[1]), peq)
    for name, s2 in (("seed s / s+1", seed + 1), ("seed s / s^2^32", seed ^ SEED_FLIP)):
        fresh_all(L, f"v4 {name}", base[0], _reset_columns(B, cfg, s2, n, extract, calls=1)[0], peq)
    return L, base[0]


def scenario_v4_interval(B, seed, n=N_STEP, steps=3, full=True):
    """v4 interval resample (draws 8, 9..11): INTERVAL_LEFT below one step's dt, one zero-action step,
    repeated ``steps`` times; envs that the step reset are left out (their commands are the reset's).
    The new commands are independent of the reset draws of the same env and of the previous call's."""
    cfg = v4_cfg()
    V = zm.V4
    L = Laws()
    b = B(cfg, n, seed)
    st0 = b.state()
    reset = {k: v for k, v in pose_draws(cfg, st0).items() if k != "roll"}
    reset.update(v4_command_draws(st0))
    a = np.zeros((n, 6), np.float32)
    calls, keep = [], np.ones(n, bool)
    for k in range(steps):
        st = b.state()
        st[V["INTERVAL_LEFT"]] = 0.5 * cfg.step_dt
        b.set_state(st)
        _, _, done = b.step(a)
        st = b.state()
        d = v4_command_draws(st)
        d["interval"] = st[V["INTERVAL_LEFT"]].astype(np.float64)
        d["live"] = ~done
        keep &= ~done
        calls.append(d)
        if not full:
            return None, d
    # (a sanity gate, not a law: the checks below need most of the envs; from the default pose a zero action
    # terminates a few per cent at the most)
    L.exact(f"v4 interval: most envs survive {steps} zero-action steps ({keep.mean():.3f})", keep.mean() > 0.9)
    cols = [k for k in calls[0] if k != "live"]
    pooled = {k: np.concatenate([c[k][c["live"]] for c in calls]) for k in cols}
    check_v4_commands(L, "v4 interval (pooled)", cfg, cfg.cmd_prob_pos, pooled)
    L.uniform("v4 interval timer (pooled)", pooled["interval"], *cfg.cmd_interval_s, grain=4.8e-7 / 3.0)
    first = {k: calls[0][k][keep] for k in cols}
    L.uncorrelated("v4 interval command x timer", first)
    L.cross("v4 interval x reset draws of the env", first, {k: v[keep] for k, v in reset.items()})
    for k in ("speed", "cyaw"):
        L.fresh(f"v4 interval / reset {k}", first[k], reset[k][keep])
    serial_all(L, "v4 interval", {k: calls[0][k] for k in cols})
    fresh_all(L, "v4 interval call ctr / ctr+1", first, {k: calls[1][k][keep] for k in cols},
              {"sign": p_equal_flag(cfg.cmd_prob_pos)})
    return L, dict(calls[0])


def scenario_manager_reset(B, seed, rel_standing, n=N_RESET, pool=1, full=True):
    """Manager construction and reset: pose 1..4, lin x, lin y, standing 5..7. ``pool``: further full
    resets whose standing flags are pooled (the flag at 0.02 needs 2^20 samples to resolve 10 %)."""
    cfg = manager_cfg(rel_standing)
    L = Laws()

    def extract(st, roll=False):   # (roll: a point for this task; kept for the marginal check only)
        d = {k: v for k, v in pose_draws(cfg, st).items() if roll or k != "roll"}
        d.update(m_command_draws(st))
        return d
    b = B(cfg, n, seed)
    base = [extract(b.state(), roll=full)]
    if not full:
        return None, base[0]
    b.reset()
    base.append(extract(b.state(), roll=True))
    for c, d in enumerate(base):
        check_pose(L, f"manager reset call {c}", cfg, d | {"roll": d.pop("roll")})
    peq = {"standing": p_equal_flag(rel_standing)}
    flags = [d["standing"] for d in base]
    M = zm.M
    for _ in range(pool - 2):
        b.reset()
        flags.append(b.rows(M["CMD_STANDING"], M["CMD_STANDING"] + 1)[0])
    for c, d in enumerate(base):
        L.uniform(f"manager reset call {c} lin x", d["lin_x"], *cfg.cmd_vel_range, grain=1.2e-7)
        L.uniform(f"manager reset call {c} lin y", d["lin_y"], *cfg.cmd_yaw_range, grain=1.2e-7)
        L.uncorrelated(f"manager reset call {c} pose x command", d)
    L.exact("standing flag is 0 or 1", all(bool(np.isin(f, (0.0, 1.0)).all()) for f in flags))
    L.bernoulli(f"manager standing flag at {rel_standing} ({len(flags)} calls)", np.concatenate(flags), rel_standing)
    serial_all(L, "manager reset", base[0])
    fresh_all(L, "manager reset call ctr / ctr+1", base[0], base[1], peq)
    for name, s2 in (("seed s / s+1", seed + 1), ("seed s / s^2^32", seed ^ SEED_FLIP)):
        fresh_all(L, f"manager reset {name}", base[0], _reset_columns(B, cfg, s2, n, extract, calls=1)[0], peq)
    return L, base[0]


def scenario_manager_step(B, seed, rel_standing=0.25, n=N_STEP, steps=3, full=True):
    """The 10 s command resample (draws 9..11) and the step's observation noise (16..31) of one stream:
    CMD_TIME_LEFT below one step's dt, one zero-action step, ``steps`` times. Standing envs get zero
    commands; the others' lin x / lin y are uniform; the noise is independent of the command draws
    of the same call, of the env's reset draws and of the previous call's noise."""
    import dataclasses
    # (the registered feet_close threshold, 0.12 m, sits 1.7e-5 m below the default stance: most envs
    # would terminate in a zero-action step; 0.10 as in the step-level parity tests)
    cfg = dataclasses.replace(manager_cfg(rel_standing), feet_close_min=0.10)
    M = zm.M
    L = Laws()
    b = B(cfg, n, seed, clean=True)
    st0 = b.state()
    reset = {k: v for k, v in pose_draws(cfg, st0).items() if k != "roll"}
    reset.update(m_command_draws(st0))
    a = np.zeros((n, 6), np.float32)
    calls, keep = [], np.ones(n, bool)
    for k in range(steps):
        st = b.state()
        st[M["CMD_TIME_LEFT"]] = 0.5 * cfg.step_dt
        b.set_state(st)
        obs, clean, done = b.step(a)
        st = b.state()
        d = m_command_draws(st)
        nz, quiet = m_noise(cfg, obs, clean)
        L.exact(f"manager step {k}: non-noisy columns carry exactly no noise ({quiet})", quiet == 0.0)
        L.exact(f"manager step {k}: the observation shows the state's command",
                bool((obs[:, 4:7] == st[M["COMMANDS"]:M["COMMANDS"] + 3].T).all()))
        d.update(nz)
        d["live"] = ~done
        keep &= ~done
        calls.append(d)
        if not full:
            return None, d
    # (a sanity gate, not a law, as in scenario_v4_interval)
    L.exact(f"manager step: most envs survive {steps} zero-action steps ({keep.mean():.3f})", keep.mean() > 0.9)
    cols = [k for k in calls[0] if k != "live"]
    pooled = {k: np.concatenate([c[k][c["live"]] for c in calls]) for k in cols}
    stand = pooled["standing"] > 0.5
    # (3 x 16 384 flags: at 0.25 this resolves a 10 % error of the parameter, at 0.02 only about 15 %
    # (4.7 sd of the count); the 0.02 flag's 10 % is resolved by scenario_manager_reset's 2^20 flags alone)
    L.bernoulli(f"manager resample standing flag at {rel_standing} (pooled)", stand, rel_standing)
    L.exact("standing envs have zero commands", bool((pooled["lin_x"][stand] == 0).all() and (pooled["lin_y"][stand] == 0).all()))
    L.uniform("manager resample lin x (pooled, moving envs)", pooled["lin_x"][~stand], *cfg.cmd_vel_range, grain=1.2e-7)
    L.uniform("manager resample lin y (pooled, moving envs)", pooled["lin_y"][~stand], *cfg.cmd_yaw_range, grain=1.2e-7)
    noise_cols = [k for k in cols if k.startswith("noise")]
    first = {k: calls[0][k] for k in cols}
    check_noise(L, "manager step noise", [{k: c[k][c["live"]] for k in noise_cols} for c in calls], 0.0)
    mv = keep & (first["standing"] < 0.5)   # (a standing env's command is zeroed: the draw is not in the state)
    cmd = {k: first[k][mv] for k in ("lin_x", "lin_y")}
    L.cross("manager noise x command draws of the call", {k: first[k][mv] for k in noise_cols}, cmd)
    L.cross("manager noise x standing flag of the call", {k: first[k][keep] for k in noise_cols},
            {"standing": first["standing"][keep]})
    L.cross("manager resample x reset draws of the env", cmd, {k: v[mv] for k, v in reset.items() if np.std(v[mv]) > 0})
    L.cross("manager resample standing flag x reset draws of the env", {"standing": first["standing"][keep]},
            {k: v[keep] for k, v in reset.items() if np.std(v[keep]) > 0})
    L.cross("manager noise x reset draws of the env", {k: first[k][keep] for k in noise_cols},
            {k: v[keep] for k, v in reset.items() if np.std(v[keep]) > 0})
    serial_all(L, "manager step", {k: first[k] for k in noise_cols})
    fresh_all(L, "manager step call ctr / ctr+1", {k: first[k][keep] for k in noise_cols},
              {k: calls[1][k][keep] for k in noise_cols})
    mv2 = mv & (calls[1]["standing"] < 0.5)
    fresh_all(L, "manager resample call ctr / ctr+1", {k: first[k][mv2] for k in ("lin_x", "lin_y")},
              {k: calls[1][k][mv2] for k in ("lin_x", "lin_y")})
    return L, dict(calls[0])


def scenario_manager_reset_in_step(B, seed, n=N_STEP, full=True):
    """Every env terminates in the step (feet_close_min above the default stance), so pose 1..4, reset
    command 5..7 and observation noise 16..31 come from one stream: their joint correlation."""
    import dataclasses
    cfg = dataclasses.replace(manager_cfg(0.25), feet_close_min=0.125)
    L = Laws()
    b = B(cfg, n, seed, clean=True)
    obs, clean, done = b.step(np.zeros((n, 6), np.float32))
    L.exact("every env reset in the step", bool(done.all()))
    st = b.state()
    d = {k: v for k, v in pose_draws(cfg, st).items() if k != "roll"}
    cm = m_command_draws(st)
    if not full:
        nz, _ = m_noise(cfg, obs, clean)
        return None, d | cm | nz | {"live": done}
    check_pose(L, "manager in-step reset", cfg, pose_draws(cfg, st))
    mv = cm["standing"] < 0.5
    L.bernoulli("manager in-step reset standing flag", cm["standing"], 0.25)
    L.exact("standing envs have zero commands", bool((cm["lin_x"][~mv] == 0).all() and (cm["lin_y"][~mv] == 0).all()))
    L.uniform("manager in-step reset lin x (moving envs)", cm["lin_x"][mv], *cfg.cmd_vel_range, grain=1.2e-7)
    L.uniform("manager in-step reset lin y (moving envs)", cm["lin_y"][mv], *cfg.cmd_yaw_range, grain=1.2e-7)
    nz, quiet = m_noise(cfg, obs, clean)
    check_noise(L, "manager in-step reset noise", [nz], quiet)
    L.cross("noise x pose draws of the call", nz, d)
    L.cross("noise x standing flag of the call", nz, {"standing": cm["standing"]})
    L.cross("noise x command draws of the call", {k: v[mv] for k, v in nz.items()},
            {k: cm[k][mv] for k in ("lin_x", "lin_y")})
    out = dict(d)
    out.update(cm)
    out.update(nz)
    out["live"] = done
    return L, out


def scenario_manager_observe(B, seed, n=N_RESET, full=True):
    """observe() noise (draws 16..31 of the next call's stream): marginals, 16x16, against the pose and
    command draws, over envs, calls (a reset in between advances the counter) and seeds."""
    cfg = manager_cfg(0.25)
    L = Laws()

    def one(s, calls):
        b = B(cfg, n, s, clean=True)
        out = []
        for c in range(calls):
            if c:
                b.reset()
            obs, clean = b.observe()
            nz, quiet = m_noise(cfg, obs, clean)
            st = b.state()
            out.append((nz, quiet, {k: v for k, v in pose_draws(cfg, st).items() if k != "roll"} | m_command_draws(st)))
        return out
    if not full:
        return None, one(seed, 1)[0][0]
    base = one(seed, 2)
    check_noise(L, "manager observe", [b[0] for b in base], max(b[1] for b in base))
    L.cross("observe noise x pose and command draws in the state", base[0][0], base[0][2])
    serial_all(L, "manager observe", base[0][0])
    fresh_all(L, "manager observe call ctr / ctr+1", base[0][0], base[1][0])
    for name, s2 in (("seed s / s+1", seed + 1), ("seed s / s^2^32", seed ^ SEED_FLIP)):
        fresh_all(L, f"manager observe {name}", base[0][0], one(s2, 1)[0][0])
    return L, base[0][0]


EP_BINS = 50


def scenario_v2_full_reset(B, seed, n=N_RESET, full=True):
    """walking v2 full reset: EP_LEN ~ U{0 .. max_episode_length - 1}, in 50 equal bins."""
    cfg = zm.TaskCfg()
    L = Laws()
    E = zm.S["EP_LEN"]
    length = cfg.max_episode_length
    assert length % EP_BINS == 0

    def extract(st):
        return dict(ep_len=st[E].astype(np.float64))
    b = B(cfg, n, seed)
    base = []
    for _ in range(2 if full else 1):
        b.reset()
        base.append(extract(b.state()))
    if not full:
        return None, base[0]
    for c, d in enumerate(base):
        e = d["ep_len"]
        L.exact(f"call {c}: EP_LEN is an integer in [0, {length})",
                bool((e == np.round(e)).all() and e.min() >= 0 and e.max() <= length - 1))
        counts = np.bincount((e // (length // EP_BINS)).astype(np.int64), minlength=EP_BINS)
        L.discrete(f"v2 full reset call {c} EP_LEN in {EP_BINS} bins", counts, np.full(EP_BINS, 1.0 / EP_BINS))
    serial_all(L, "v2 full reset", base[0])
    peq = {"ep_len": 1.0 / length}
    fresh_all(L, "v2 full reset call ctr / ctr+1", base[0], base[1], peq)
    for name, s2 in (("seed s / s+1", seed + 1), ("seed s / s^2^32", seed ^ SEED_FLIP)):
        o = B(cfg, n, s2)
        o.reset()
        fresh_all(L, f"v2 full reset {name}", base[0], extract(o.state()), peq)
    return L, base[0]


# ----------------------------------------------------------------------------- action noise
MASK = (1 << 64) - 1


def _mix64(x):
    """splitmix64's finaliser on uint64 arrays (ppo_mlp.hip mix64)."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def noise_key(seed: int, counter: int, step: int) -> int:
    """noise_at's stream key; injective for 0 <= step < 4096 and counter < 2^20 (include/zbot_ppo.h)."""
    return (((seed & 0xFFFFFFFF) << 32) ^ ((counter & 0xFFFFFFFF) << 12) ^ (step & 0xFFFFFFFF)) & MASK


def noise_at(seed: int, counter: int, step: int, rows: int, na: int) -> np.ndarray:
    """numpy restatement of ppo_mlp.hip noise_at: the integer hash in uint64, u1, u2 and Box-Muller
    in float64. [rows][na]."""
    key = np.array([noise_key(seed, counter, step)], np.uint64)
    idx = np.arange(rows * na, dtype=np.uint64)
    h = _mix64(_mix64(key) ^ idx)
    u1 = ((h >> np.uint64(40)).astype(np.float64) + 1.0) * 2.0 ** -24          # (0, 1]
    u2 = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24   # [0, 1)
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).reshape(rows, na)


def check_action_noise(L: Laws, tag, z):
    """One call's [rows][na] standard normals: Kolmogorov-Smirnov and moments, the counts beyond 3 and
    4 sigma against their binomial laws, the na x na correlation, serial correlation over rows."""
    from random_laws import normal_cdf
    n = z.size
    L.normal(tag, z)
    for s in (3.0, 4.0):
        p = 2.0 * float(normal_cdf(np.array([-s]))[0])
        L.binomial(f"{tag} beyond {s:g} sigma", int((np.abs(z) > s).sum()), n, p)
    L.uncorrelated(f"{tag} actions", [z[:, a] for a in range(z.shape[1])])
    for a in range(z.shape[1]):
        L.serial(f"{tag} action {a} over rows", z[:, a])


# ----------------------------------------------------------------------------- device against oracle
DISCRETE = ("sign", "standing", "ep_len", "live")
STATE_TOL = 2e-6   # tests/test_gpu_manager.py: the state after create / reset, device against oracle
OBS_TOL = 1e-5     # tests/test_gpu_manager.py: observe(), device against oracle


def compare_draws(dev: dict, ora: dict, cfg, sample=1024):
    """The device's recovered draws against the oracle's on a spread sample of ``sample`` envs: bit-equal
    for the integer-valued columns (flags, signs, episode lengths: what the parity tests establish
    bit-exactly), within the parity tests' tolerances for the continuous ones (the pose goes through
    sincos, the commands through an FMA). Returns the largest continuous difference."""
    n = len(next(iter(dev.values())))
    idx = np.unique(np.linspace(0, n - 1, sample).astype(np.int64))
    both = np.ones(len(idx), bool)
    if "live" in dev:   # (an env that terminated on one side only holds other draws)
        both = dev["live"][idx] == ora["live"][idx]
        assert both.mean() >= 0.99   # (the parity tests' share of envs whose flags agree)
    worst = 0.0
    for k in dev:
        a, b = np.asarray(dev[k])[idx][both], np.asarray(ora[k])[idx][both]
        if k in DISCRETE:
            np.testing.assert_array_equal(a, b, err_msg=k)
            continue
        tol = STATE_TOL
        if k.startswith("noise"):   # normalised by the half-width
            c = int(k[5:])
            tol = OBS_TOL / cfg.obs_noise[0 if c < 4 else 1 if c < 13 else 2]
        diff = float(np.abs(a - b).max())
        assert diff <= tol, (k, diff, tol)
        if not k.startswith("noise"):
            worst = max(worst, diff)
    return worst
