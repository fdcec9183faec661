"""The manager env's five restored reward terms and the state they keep, stated once in numpy
(include/zbot_manager_terms.h; the reference's mdp/rewards.py:144-287 and Isaac Lab's ContactSensor
timer update). ``dtype`` is the arithmetic of the continuous parts: float64 is the reference, float32 the
same statement at the device's precision (its error against float64 sizes the GPU test's tolerance).
The gates compare float32 quantities computed in the reference's own order whatever ``dtype`` is, since
the recorded outcome of the reference's fp32 arithmetic is the law there (tests/golden/mdp_manager_terms.npz).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

TERMS = ["gait", "feet_clearance", "feet_air_time", "base_vel_forward", "feet_force_pattern"]
F32 = np.float32


@dataclass
class Params:
    """The base cfg's params (zbotlab_env_cfg.py:301-366)."""
    gait_period: float = 2.0
    gait_offset: tuple = (0.0, 0.5)
    gait_threshold: float = 0.55
    clearance_std: float = 0.05
    clearance_tanh_mult: float = 2.0
    clearance_target_height: float = 0.01
    air_time_threshold: float = 0.3
    which_forward: int = 1


def gait_phase(ep_len, step_dt, p: Params):
    """Leg phases [N, 2] in the reference's fp32 order: ((ep * step_dt) % period / period + offset) % 1."""
    t = np.asarray(ep_len).astype(F32) * F32(step_dt)
    g = np.remainder(t, F32(p.gait_period)) / F32(p.gait_period)
    return np.stack([np.remainder(g + F32(o), F32(1.0)) for o in p.gait_offset], axis=-1)


def cmd_norm(cmd, n):
    """|command[:, :n]| in fp32 (torch.norm on the float32 command)."""
    c = np.asarray(cmd, F32)[..., :n]
    return np.sqrt(np.sum(c * c, axis=-1, dtype=F32))


def gates(ep_len, step_dt, cmd, contact_time, p: Params) -> dict:
    """Every decision of the five terms, with the quantity that decides it and its threshold."""
    ph = gait_phase(ep_len, step_dt, p)
    in_c = np.asarray(contact_time, F32) > 0
    return dict(phase=ph, stance=ph < F32(p.gait_threshold), in_contact=in_c,
                norm3=cmd_norm(cmd, 3), moving3=cmd_norm(cmd, 3) > F32(0.05),
                norm2=cmd_norm(cmd, 2), moving2=cmd_norm(cmd, 2) > F32(0.1),
                single_stance=in_c.sum(-1) == 1)


def terms(ep_len, step_dt, cmd, contact_time, air_time, foot_z, foot_vxy, fwd_xy, root_vel, fz_hist, force_sum,
          p: Params = Params(), dtype=np.float64, force_pattern_active=True):
    """(terms [N, 5] in TERMS order, feet_force_sum after [N]). fwd_xy: the forward vector g x quat_apply(
    root_quat, y) (which_forward = +1); fz_hist [N, 3, 2]; force_sum: the integrator before the call."""
    g = gates(ep_len, step_dt, cmd, contact_time, p)
    D = dtype
    ct, at = np.asarray(contact_time, D), np.asarray(air_time, D)
    out = np.zeros((len(ct), 5), D)
    out[:, 0] = (g["stance"] == g["in_contact"]).sum(-1) * g["moving3"]
    z, v = np.asarray(foot_z, D), np.asarray(foot_vxy, D)
    speed = np.sqrt(np.sum(v * v, axis=-1, dtype=D))
    err = np.square(z - D(p.clearance_target_height)) * np.tanh(D(p.clearance_tanh_mult) * speed)
    out[:, 1] = np.exp(-np.sum(err, axis=-1, dtype=D) / D(p.clearance_std))
    mode = np.where(g["in_contact"], ct, at)
    t = np.minimum(np.min(np.where(g["single_stance"][:, None], mode, D(0)), axis=-1), D(p.air_time_threshold))
    out[:, 2] = t * g["moving2"]
    f, rv = np.asarray(fwd_xy, D), np.asarray(root_vel, D)
    out[:, 3] = D(p.which_forward) * (rv[:, 0] * f[:, 0] + rv[:, 1] * f[:, 1])
    F = np.sum(np.asarray(fz_hist, D), axis=1, dtype=D) / D(3)
    s0 = np.asarray(force_sum, D)
    d = (F[:, 1] - F[:, 0]) * np.sign(s0)
    s1 = s0 + D(0.001) * (F[:, 0] - F[:, 1]) if force_pattern_active else s0
    out[:, 4] = D(0.5) * d - D(0.1) * np.abs(s1)
    return out, s1


def forward_xy(root_quat, dtype=np.float64):
    """g x quat_apply(q, (0, 1, 0)) with g = (0, 0, -1): (R11, -R01) of the rotation matrix of q (w, x, y, z)."""
    w, x, y, z = (np.asarray(root_quat, dtype)[:, k] for k in range(4))
    return np.stack([1 - 2 * (x * x + z * z), -2 * (x * y - w * z)], axis=-1)


def sensor_update(air_cur, air_last, contact_cur, in_contact, sim_dt):
    """One ContactSensor update of the feet's timers (fp32, as the sensor accumulates them):
    (current_air_time, last_air_time, current_contact_time) after a physics step whose contact flags are
    in_contact [N, 2]."""
    a, l, c = (np.asarray(v, F32) for v in (air_cur, air_last, contact_cur))
    dt = F32(sim_dt)
    l = np.where((a > 0) & in_contact, a + dt, l)
    a = np.where(in_contact, F32(0), a + dt)
    c = np.where(in_contact, c + dt, F32(0))
    return a, l, c


def sum_update(sums, term_values, weights, step_dt, dtype=np.float64):
    """RewardManager.compute's episode sums: sums + term * weight * step_dt, rounded to dtype."""
    D = dtype
    return np.asarray(sums, D) + np.asarray(term_values, D) * np.asarray(weights, D) * D(step_dt)
