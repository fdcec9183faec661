"""``zbot-6b-walking-m-v0``: the reference's manager-based flat env with the ManagerBasedRLEnv API.

Reference: ``source/zbot/zbot/tasks/zbotlab_manager`` — ``zbotlab_env_cfg.py`` (scene, commands,
actions, observations, events, rewards, terminations, curriculum: ``ZbotLabRoughEnvCfg``),
``config/zbot6b_manager/rough_env_cfg.py`` (``ZBOT_6S_V2_CFG``, events / terminations removed) and
``flat_env_cfg.py`` (``Zbot6BFlatEnvCfg``: plane, reward overrides), registered as
``isaaclab.envs:ManagerBasedRLEnv`` (``config/zbot6b_manager/__init__.py:18-26``).

Isaac Lab's managers evaluate python term functions one by one; here the term *configuration* is
kept (same cfg classes, names, weights and params, so user code that edits ``cfg.rewards.x.weight``
or ``cfg.commands.base_velocity.ranges`` keeps working) and compiled into the fused HIP step kernel
(``zb_m_step_kernel``): action processing, 4 physics substeps with the per-step contact sensor,
terminations, rewards, the reset events, the command manager and the observation group run in one
launch per step. ``task_cfg()`` validates the cfg: a term the kernel does not implement (e.g. one the
flat cfg sets to ``None``, or a different ``func``) raises instead of being ignored.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field, fields

import numpy as np
import torch

from .. import model as zm
from .standup_v0 import EventTermCfg
from .walking_v2 import SimulationCfg, SolverCfg, ZbotDirectEnvV2


# ----------------------------------------------------------------------------- manager term cfgs
@dataclass
class ObsTerm:
    func: str
    noise: tuple | None = None           # AdditiveUniformNoiseCfg(n_min, n_max)
    params: dict = field(default_factory=dict)


@dataclass
class RewTerm:
    func: str
    weight: float
    params: dict = field(default_factory=dict)


@dataclass
class DoneTerm:
    func: str
    params: dict = field(default_factory=dict)
    time_out: bool = False


@dataclass
class CurrTerm:
    func: str
    params: dict = field(default_factory=dict)


EventTerm = EventTermCfg


@dataclass
class Ranges:
    lin_vel_x: tuple = (0.0, 0.0)
    lin_vel_y: tuple = (0.0, 0.0)
    ang_vel_z: tuple = (0.0, 0.0)
    heading: tuple | None = None


@dataclass
class UniformLevelVelocityCommandCfg:
    """mdp/commands/velocity_command.py (UniformVelocityCommandCfg + limit_ranges); mgr.py:99-117."""
    asset_name: str = "robot"
    resampling_time_range: tuple = (10.0, 10.0)
    rel_standing_envs: float = 0.02
    rel_heading_envs: float = 1.0
    heading_command: bool = False
    heading_control_stiffness: float = 1.0
    debug_vis: bool = True
    ranges: Ranges = field(default_factory=lambda: Ranges(lin_vel_x=(-0.1, 0.1)))
    limit_ranges: Ranges = field(default_factory=lambda: Ranges(lin_vel_x=(-0.3, 0.3)))


@dataclass
class CommandsCfg:
    base_velocity: UniformLevelVelocityCommandCfg = field(default_factory=UniformLevelVelocityCommandCfg)


@dataclass
class RelativeJointPositionActionCfg:
    """mgr.py:125-131."""
    asset_name: str = "robot"
    joint_names: list = field(default_factory=lambda: ["joint.*"])
    scale: float = 0.04 * math.pi
    clip: dict = field(default_factory=lambda: {"joint.*": [-0.04 * math.pi, 0.04 * math.pi]})
    use_zero_offset: bool = True


@dataclass
class ActionsCfg:
    joint_pos: RelativeJointPositionActionCfg = field(default_factory=RelativeJointPositionActionCfg)


@dataclass
class PolicyCfg:
    """mgr.py:139-158 (terms in order, corruption on, concatenated)."""
    base_quat: ObsTerm = field(default_factory=lambda: ObsTerm("root_quat_w", (-0.01, 0.01)))
    velocity_commands: ObsTerm = field(default_factory=lambda: ObsTerm(
        "generated_commands", None, {"command_name": "base_velocity"}))
    joint_pos: ObsTerm = field(default_factory=lambda: ObsTerm("joint_pos_rel", (-0.01, 0.01)))
    joint_vel: ObsTerm = field(default_factory=lambda: ObsTerm("joint_vel_rel", (-1.5, 1.5)))
    actions: ObsTerm = field(default_factory=lambda: ObsTerm("last_action"))
    enable_corruption: bool = True
    concatenate_terms: bool = True


@dataclass
class ObservationsCfg:
    policy: PolicyCfg = field(default_factory=PolicyCfg)


def _feet(p=None):
    return dict({"asset_cfg": "robot:foot.*"}, **(p or {}))


def base_reward_term(name: str) -> RewTerm:
    """The reference's base cfg's term for one of the five fields the flat cfg sets to ``None``
    (zbotlab_env_cfg.py:301-366: func, weight and params), e.g. ``cfg.rewards.gait = base_reward_term("gait")``."""
    sensor = {"sensor_cfg": "contact_forces:foot.*"}
    terms = {
        "gait": lambda: RewTerm("feet_gait", 0.5, dict(
            {"period": 2.0, "offset": [0.0, 0.5], "threshold": 0.55, "command_name": "base_velocity"}, **sensor)),
        "feet_clearance": lambda: RewTerm("foot_clearance_reward", 1.0, _feet(
            {"std": 0.05, "tanh_mult": 2.0, "target_height": 0.01})),
        "feet_air_time": lambda: RewTerm("feet_air_time_positive_biped", 2.5, dict(
            {"command_name": "base_velocity", "threshold": 0.3}, **sensor)),
        "base_vel_forward": lambda: RewTerm("base_vel_forward", 1.0, {"which_forward": 1}),
        "feet_force_pattern": lambda: RewTerm("feet_force_pattern", 1.0, dict(sensor)),
    }
    if name not in terms:
        raise KeyError(f"{name!r} is not one of {zm.M_EXTRA_REWARD_TERMS}")
    return terms[name]()


_TERMS_COMPILED = (
    "compiled: rewards.gait = RewTerm('feet_gait', w, {'period': > 0, 'offset': [o0, o1], 'threshold': t, "
    "'command_name': 'base_velocity', 'sensor_cfg': 'contact_forces:foot.*'}); rewards.feet_clearance = RewTerm("
    "'foot_clearance_reward', w, {'std': > 0, 'tanh_mult': m, 'target_height': h, 'asset_cfg': 'robot:foot.*'}); "
    "rewards.feet_air_time = RewTerm('feet_air_time_positive_biped', w, {'command_name': 'base_velocity', "
    "'threshold': t, 'sensor_cfg': 'contact_forces:foot.*'}); rewards.base_vel_forward = RewTerm('base_vel_forward', "
    "w, {'which_forward': 1 | -1}); rewards.feet_force_pattern = RewTerm('feet_force_pattern', w, {'sensor_cfg': "
    "'contact_forces:foot.*'}); beside any subset of the flat cfg's 11 terms with their own func / params. "
    "rewards.undesired_contacts and terminations.base_contact (net contact forces on non-foot links) are not compiled")


@dataclass
class RewardsCfg:
    """mgr.py:261-377 after flat_env_cfg.py:169-182 (weights 5.0 / -6.5 / -15.0, six terms None; five of
    the six compile when restored: ``base_reward_term``)."""
    track_lin_vel_xy_exp: RewTerm | None = field(default_factory=lambda: RewTerm(
        "track_lin_vel_xy_yaw_frame_exp", 1.0, {"command_name": "base_velocity", "std": math.sqrt(0.25)}))
    track_ang_vel_z_exp: RewTerm | None = field(default_factory=lambda: RewTerm(
        "track_ang_vel_z_world_exp", 0.5, {"command_name": "base_velocity", "std": math.sqrt(0.25)}))
    termination_penalty: RewTerm | None = field(default_factory=lambda: RewTerm("is_terminated", -200.0))
    dof_torques_l2: RewTerm | None = field(default_factory=lambda: RewTerm("joint_torques_l2", -1.0e-5))
    dof_acc_l2: RewTerm | None = field(default_factory=lambda: RewTerm("joint_acc_l2", -2.5e-7))
    action_rate_l2: RewTerm | None = field(default_factory=lambda: RewTerm("action_rate_l2", -0.01))
    foot_step_length: RewTerm | None = field(default_factory=lambda: RewTerm(
        "foot_step_length", 5.0, _feet({"sensor_cfg": "contact_forces:foot.*", "command_name": None})))
    foot_downward: RewTerm | None = field(default_factory=lambda: RewTerm("foot_downward", -1.0, _feet()))
    foot_forward: RewTerm | None = field(default_factory=lambda: RewTerm("foot_forward", -0.5, _feet()))
    gait: RewTerm | None = None
    feet_slide: RewTerm | None = field(default_factory=lambda: RewTerm(
        "feet_slide", -6.5, _feet({"sensor_cfg": "contact_forces:foot.*"})))
    feet_clearance: RewTerm | None = None
    feet_air_time: RewTerm | None = None
    air_time_variance: RewTerm | None = field(default_factory=lambda: RewTerm(
        "air_time_balance_penalty", -15.0, {"sensor_cfg": "contact_forces:foot.*"}))
    base_vel_forward: RewTerm | None = None
    feet_force_pattern: RewTerm | None = None
    undesired_contacts: RewTerm | None = None


@dataclass
class TerminationsCfg:
    """mgr.py:379-398; rough_env_cfg.py:45 removes base_contact."""
    time_out: DoneTerm | None = field(default_factory=lambda: DoneTerm("time_out", time_out=True))
    base_contact: DoneTerm | None = None
    base_height: DoneTerm | None = field(default_factory=lambda: DoneTerm(
        "root_height_below_minimum", {"minimum_height": 0.2}))
    feet_close: DoneTerm | None = field(default_factory=lambda: DoneTerm(
        "feet_close", {"minimum_distance": 0.12, "asset_cfg": "robot:foot.*"}))


@dataclass
class EventCfg:
    """mgr.py:164-258; rough_env_cfg.py:37-41 removes add_base_mass, base_com, push_robot (a cfg that
    restores them compiles: Zbot6BFlatEnvCfg.base_inertia() / manager_events())."""
    init_my_data: EventTerm | None = field(default_factory=lambda: EventTerm("init_my_data", "startup"))
    physics_material: EventTerm | None = field(default_factory=lambda: EventTerm(
        "randomize_rigid_body_material", "startup",
        {"static_friction_range": (0.3, 1.0), "dynamic_friction_range": (0.3, 1.0), "restitution_range": (0.0, 0.0),
         "num_buckets": 64}))
    add_base_mass: EventTerm | None = None
    base_com: EventTerm | None = None
    reset_base: EventTerm | None = field(default_factory=lambda: EventTerm(
        "reset_root_state_uniform", "reset",
        {"pose_range": {"x": (-0.5, 0.5), "y": (-0.5, 0.5), "yaw": (-3.14, 3.14)},
         "velocity_range": {k: (0.0, 0.0) for k in ("x", "y", "z", "roll", "pitch", "yaw")}}))
    reset_robot_joints: EventTerm | None = field(default_factory=lambda: EventTerm(
        "reset_joints_by_scale", "reset", {"position_range": (1.0, 1.0), "velocity_range": (1.0, 1.0)}))
    reset_my_data: EventTerm | None = field(default_factory=lambda: EventTerm("reset_my_data", "reset"))
    push_robot: EventTerm | None = None


@dataclass
class CurriculumCfg:
    terrain_levels: CurrTerm | None = None      # flat_env_cfg.py:189
    lin_vel_cmd_levels: CurrTerm | None = field(default_factory=lambda: CurrTerm("lin_vel_cmd_levels"))


@dataclass
class SceneCfg:
    num_envs: int = 4096                         # mgr.py:419
    env_spacing: float = 2.5
    replicate_physics: bool = True
    terrain_type: str = "plane"                  # flat_env_cfg.py:186


@dataclass
class BaseInertiaEvents:
    """What ``Zbot6BFlatEnvCfg.base_inertia()`` compiles ``events.add_base_mass`` / ``events.base_com``
    into: the ranges the env's startup draws from. The default is "off"."""
    mass_enabled: bool = False
    mass_range: tuple = (0.0, 0.0)
    mass_operation: str = "add"
    recompute_inertia: bool = True
    com_enabled: bool = False
    com_range: tuple = ((0.0, 0.0),) * 3

    @property
    def enabled(self) -> bool:
        return self.mass_enabled or self.com_enabled


_BASE_LINK_MASS = None


def base_link_mass() -> float:
    """The authored mass of the manager env's base link (the default the mass event starts from)."""
    global _BASE_LINK_MASS
    if _BASE_LINK_MASS is None:
        _BASE_LINK_MASS = float(zm.pack_base_link(zm.load_v09_model()).mass)
    return _BASE_LINK_MASS


@dataclass
class Zbot6BFlatEnvCfg:
    """Mirror of ``Zbot6BFlatEnvCfg`` (flat_env_cfg.py:89-189 over rough_env_cfg.py / mgr.py:414-452)."""
    scene: SceneCfg = field(default_factory=SceneCfg)
    observations: ObservationsCfg = field(default_factory=ObservationsCfg)
    actions: ActionsCfg = field(default_factory=ActionsCfg)
    commands: CommandsCfg = field(default_factory=CommandsCfg)
    rewards: RewardsCfg = field(default_factory=RewardsCfg)
    terminations: TerminationsCfg = field(default_factory=TerminationsCfg)
    events: EventCfg = field(default_factory=EventCfg)
    curriculum: CurriculumCfg = field(default_factory=CurriculumCfg)
    decimation: int = 4
    episode_length_s: float = 20.0
    sim: SimulationCfg = field(default_factory=SimulationCfg)
    # (the ruling-on-face manifold is compiled into the walking v2 / stand-up kernels only)
    solver: SolverCfg = field(default_factory=lambda: SolverCfg(self_manifold=2))
    seed: int | None = None
    # privileged critic observations (the "critic" group: the policy terms without noise + 7 state terms)
    critic_observations: bool = False

    # the DirectRLEnv-style fields the shared env base reads
    action_space = 6
    observation_space = zm.M_OBS_DIM

    @property
    def reward_cfg(self) -> dict:
        return {"reward_scales": {k: t.weight for k, t in _active(self.rewards)}}

    def reward_terms(self) -> list:
        """The active reward terms' names in cfg order (the ``Episode_Reward/*`` keys)."""
        return [k for k, _ in _active(self.rewards)]

    def task_cfg(self) -> zm.TaskCfg:
        """Compile the manager cfg into the kernel's task parameters (raises on unsupported terms). Any of
        the flat cfg's 11 terms may be ``None`` (weight 0 in the kernel); the five restored terms compile
        beside it (``manager_terms()``)."""
        rew = [(k, t) for k, t in _active(self.rewards) if k not in zm.M_EXTRA_REWARD_TERMS]
        names = [k for k, _ in rew]
        if not set(names) <= set(zm.M_REWARD_TERMS):
            raise NotImplementedError(f"reward terms {sorted(set(names) - set(zm.M_REWARD_TERMS))} are not compiled; "
                                      f"{_TERMS_COMPILED}")
        expect = RewardsCfg()
        for k, t in rew:
            ref = getattr(expect, k)
            if t.func != ref.func or t.params != ref.params:
                raise NotImplementedError(f"reward term {k}: func / params {t.func} {t.params} not compiled")
        self.manager_terms()  # gait, feet_clearance, feet_air_time, base_vel_forward, feet_force_pattern
        term = _active(self.terminations)
        if [k for k, _ in term] != zm.M_TERMINATION_TERMS:
            extra = " (terminations.base_contact needs net contact forces on non-foot links; " + _TERMS_COMPILED + ")" \
                if any(k == "base_contact" for k, _ in term) else ""
            raise NotImplementedError(f"termination terms {[k for k, _ in term]} != {zm.M_TERMINATION_TERMS}{extra}")
        cmd = self.commands.base_velocity
        self.manager_events()  # push_robot, ang_vel_z, heading_command: raises on the forms not compiled
        lo, hi = cmd.resampling_time_range
        if lo != hi:
            raise NotImplementedError("resampling_time_range must be a single value (flat cfg: (10, 10))")
        act = self.actions.joint_pos
        (clo, chi), = act.clip.values()
        if not act.use_zero_offset or clo != -chi:
            raise NotImplementedError("RelativeJointPositionAction: zero offset and a symmetric clip are compiled")
        pol = self.observations.policy
        noise = [getattr(pol, k).noise for k in ("base_quat", "joint_pos", "joint_vel")]
        if [f.name for f in fields(pol)][:5] != ["base_quat", "velocity_commands", "joint_pos", "joint_vel", "actions"] \
                or any(n is not None and n[0] != -n[1] for n in noise):
            raise NotImplementedError("policy observation group: the compiled terms / symmetric noise only")
        ev = self.events
        self.base_inertia()  # add_base_mass, base_com: raises on the forms not compiled
        pr = ev.reset_base.params["pose_range"]
        if any(pr.get(k, (0.0, 0.0)) != (0.0, 0.0) for k in ("z", "pitch")) or \
                any(tuple(v) != (0.0, 0.0) for v in ev.reset_base.params["velocity_range"].values()):
            raise NotImplementedError("reset_base: z / pitch offsets and velocities are not compiled")
        if tuple(ev.reset_robot_joints.params["position_range"]) != (1.0, 1.0):
            raise NotImplementedError("reset_joints_by_scale: only the default (1, 1) scale is compiled")
        if self.curriculum.terrain_levels is not None:
            raise NotImplementedError("terrain_levels needs the rough terrain generator (out of scope)")
        return zm.TaskCfg.manager_flat(
            sim_dt=self.sim.dt, decimation=self.decimation, episode_length_s=self.episode_length_s,
            reward_weights={k: t.weight for k, t in rew},
            termination_height=float(self.terminations.base_height.params["minimum_height"]),
            feet_close_min=float(self.terminations.feet_close.params["minimum_distance"]),
            gravity=-self.sim.gravity[2], friction=self.sim.static_friction,
            friction_dynamic=self.sim.dynamic_friction,
            contact_margin=self.solver.contact_margin, baumgarte=self.solver.baumgarte,
            solver_iterations=self.solver.iterations, enable_self_collision=self.solver.self_collision,
            solver_mode=self.solver.mode, self_manifold=self.solver.self_manifold,
            reset_pose_range=tuple(tuple(pr.get(k, (0.0, 0.0))) for k in ("x", "y", "roll", "yaw")),
            cmd_vel_range=tuple(cmd.ranges.lin_vel_x), cmd_yaw_range=tuple(cmd.ranges.lin_vel_y),
            range_limit_vel=tuple(cmd.limit_ranges.lin_vel_x), range_limit_yaw=tuple(cmd.limit_ranges.lin_vel_y),
            cmd_resample_s=float(lo), cmd_rel_standing=float(cmd.rel_standing_envs),
            action_scale=float(act.scale), action_clip=float(chi),
            obs_corruption=bool(pol.enable_corruption),
            obs_noise=tuple(0.0 if n is None else float(n[1]) for n in noise),
            range_period_steps=None if self.curriculum.lin_vel_cmd_levels is not None else -1,
        )


    def manager_events(self) -> zm.ManagerEvents:
        """Compile ``events.push_robot`` and the ``base_velocity`` command's ``ang_vel_z`` /
        ``heading_command`` into the kernel's event parameters (``zb_set_manager_events``; they live beside
        ``TaskCfg``, which they leave unchanged). The unedited cfg gives "events off". Raises
        ``NotImplementedError`` on a form that is not compiled, saying what is."""
        out = zm.ManagerEvents()
        push = self.events.push_robot
        if push is not None:
            vr = push.params.get("velocity_range") if isinstance(push.params, dict) else None
            if push.func != "push_by_setting_velocity" or push.mode != "interval" or push.interval_range_s is None \
                    or not isinstance(vr, dict) or set(push.params) != {"velocity_range"} or not set(vr) <= set(zm.PUSH_AXES):
                raise NotImplementedError(
                    "events.push_robot: compiled as EventTerm('push_by_setting_velocity', 'interval', "
                    "{'velocity_range': {x / y / z / roll / pitch / yaw: (lo, hi)}}, interval_range_s=(lo, hi)) "
                    "with 0 < lo <= hi")
            ilo, ihi = (float(v) for v in push.interval_range_s)
            rng = tuple(tuple(float(v) for v in vr.get(k, (0.0, 0.0))) for k in zm.PUSH_AXES)
            if not 0.0 < ilo <= ihi or any(a > b for a, b in rng):
                raise NotImplementedError("events.push_robot: interval_range_s needs 0 < lo <= hi, every "
                                          "velocity range lo <= hi")
            out.push_enabled, out.push_interval_s, out.push_velocity_range = True, (ilo, ihi), rng
        cmd = self.commands.base_velocity
        az = tuple(float(v) for v in cmd.ranges.ang_vel_z)
        if az != tuple(float(v) for v in cmd.limit_ranges.ang_vel_z) or az[0] > az[1]:
            raise NotImplementedError("ranges.ang_vel_z must equal limit_ranges.ang_vel_z (lo <= hi): there is no "
                                      "curriculum on the yaw command (ang_vel_cmd_levels is not in CurriculumCfg)")
        out.cmd_ang_vel_z = az
        if cmd.heading_command:
            if cmd.ranges.heading is None:
                raise NotImplementedError("heading_command=True needs ranges.heading=(lo, hi), and an "
                                          "ang_vel_z range for the controller's output to be clipped to")
            hd = tuple(float(v) for v in cmd.ranges.heading)
            if hd[0] > hd[1]:
                raise NotImplementedError("ranges.heading needs lo <= hi")
            out.heading_command, out.cmd_heading = True, hd
            out.cmd_rel_heading = float(cmd.rel_heading_envs)
            out.heading_stiffness = float(cmd.heading_control_stiffness)
        return out

    def manager_terms(self) -> zm.ManagerTerms:
        """Compile ``rewards.gait`` / ``feet_clearance`` / ``feet_air_time`` / ``base_vel_forward`` /
        ``feet_force_pattern`` into the kernel's term parameters (``zb_set_manager_terms``; they live beside
        ``TaskCfg``, which they leave unchanged). The unedited cfg gives "none active". Raises
        ``NotImplementedError`` on a form that is not compiled, saying what is."""
        out = zm.ManagerTerms()
        r = self.rewards

        def params_of(name, func, keys, fixed):
            t = getattr(r, name)
            p = t.params if isinstance(t.params, dict) else None
            if t.func != func or p is None or set(p) != set(keys) | set(fixed) or any(p[k] != v for k, v in fixed.items()):
                raise NotImplementedError(f"rewards.{name}: {t.func!r} / {t.params!r} is not compiled; {_TERMS_COMPILED}")
            out.weights[name] = float(t.weight)
            return p

        def number(name, key, v, positive=False):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or (positive and not v > 0):
                raise NotImplementedError(f"rewards.{name}: {key} = {v!r} is not compiled; {_TERMS_COMPILED}")
            return float(v)

        if r.undesired_contacts is not None:
            raise NotImplementedError("rewards.undesired_contacts needs net contact forces on non-foot links (ground and "
                                      f"self contact, 3-slot history) and is not compiled; {_TERMS_COMPILED}")
        sensor = {"sensor_cfg": "contact_forces:foot.*"}
        if r.gait is not None:
            p = params_of("gait", "feet_gait", ("period", "offset", "threshold"), dict(sensor, command_name="base_velocity"))
            off = p["offset"]
            if not isinstance(off, (list, tuple)) or len(off) != 2:
                raise NotImplementedError(f"rewards.gait: offset = {off!r} needs one entry per foot; {_TERMS_COMPILED}")
            out.gait_period = number("gait", "period", p["period"], positive=True)
            out.gait_offset = tuple(number("gait", "offset", v) for v in off)
            out.gait_threshold = number("gait", "threshold", p["threshold"])
        if r.feet_clearance is not None:
            p = params_of("feet_clearance", "foot_clearance_reward", ("std", "tanh_mult", "target_height"),
                          {"asset_cfg": "robot:foot.*"})
            out.clearance_std = number("feet_clearance", "std", p["std"], positive=True)
            out.clearance_tanh_mult = number("feet_clearance", "tanh_mult", p["tanh_mult"])
            out.clearance_target_height = number("feet_clearance", "target_height", p["target_height"])
        if r.feet_air_time is not None:
            p = params_of("feet_air_time", "feet_air_time_positive_biped", ("threshold",),
                          dict(sensor, command_name="base_velocity"))
            out.air_time_threshold = number("feet_air_time", "threshold", p["threshold"])
        if r.base_vel_forward is not None:
            p = params_of("base_vel_forward", "base_vel_forward", ("which_forward",), {})
            if isinstance(p["which_forward"], bool) or p["which_forward"] not in (1, -1):
                raise NotImplementedError(f"rewards.base_vel_forward: which_forward = {p['which_forward']!r} must be "
                                          f"1 or -1; {_TERMS_COMPILED}")
            out.which_forward = int(p["which_forward"])
        if r.feet_force_pattern is not None:
            params_of("feet_force_pattern", "feet_force_pattern", (), sensor)
        return out

    def base_inertia(self) -> "BaseInertiaEvents":
        """Compile the startup events ``events.add_base_mass`` and ``events.base_com`` into the per-env
        base mass / COM ranges (``zb_set_base_inertia``; beside ``TaskCfg``, which they leave unchanged).
        The unedited cfg gives "off". Raises ``NotImplementedError`` on a form that is not compiled,
        saying what is, and ``ValueError`` when the mass range reaches a mass <= 0."""
        out = BaseInertiaEvents()
        compiled = ("compiled: events.add_base_mass = EventTerm('randomize_rigid_body_mass', 'startup', "
                    "{'mass_distribution_params': (lo, hi), 'operation': 'add' | 'scale' | 'abs'[, 'distribution': "
                    "'uniform'][, 'recompute_inertia': bool]}) and events.base_com = EventTerm("
                    "'randomize_rigid_body_com', 'startup', {'com_range': {'x': (lo, hi), 'y': ..., 'z': ...}}), "
                    "both on body 'base' (asset_cfg absent or 'robot:base')")

        def params_of(name, term, func, required, optional):
            p = term.params if isinstance(term.params, dict) else None
            if term.func != func or term.mode != "startup" or p is None or not required <= set(p) \
                    or not set(p) <= required | optional | {"asset_cfg"} or p.get("asset_cfg", "robot:base") != "robot:base":
                raise NotImplementedError(f"events.{name}: {term.func!r} / {term.mode!r} / "
                                          f"{sorted(p) if p is not None else term.params!r} is not compiled; {compiled}")
            return p

        mass = self.events.add_base_mass
        if mass is not None:
            p = params_of("add_base_mass", mass, "randomize_rigid_body_mass", {"mass_distribution_params", "operation"},
                          {"distribution", "recompute_inertia"})
            if p["operation"] not in ("add", "scale", "abs") or p.get("distribution", "uniform") != "uniform":
                raise NotImplementedError(f"events.add_base_mass: operation {p['operation']!r} / distribution "
                                          f"{p.get('distribution')!r} is not compiled; {compiled}")
            lo, hi = (float(v) for v in p["mass_distribution_params"])
            if lo > hi:
                raise NotImplementedError(f"events.add_base_mass: mass_distribution_params need lo <= hi; {compiled}")
            m0 = base_link_mass()
            least = float(min(zm.base_mass_op(m0, lo, p["operation"]), zm.base_mass_op(m0, hi, p["operation"])))
            if not least > 0.0:
                raise ValueError(f"events.add_base_mass: {p['operation']} {(lo, hi)} on the base link's {m0:.4f} kg "
                                 f"reaches a mass of {least:.4f} kg; a rigid body needs a positive mass")
            out.mass_enabled, out.mass_range, out.mass_operation = True, (lo, hi), p["operation"]
            out.recompute_inertia = bool(p.get("recompute_inertia", True))
        com = self.events.base_com
        if com is not None:
            p = params_of("base_com", com, "randomize_rigid_body_com", {"com_range"}, set())
            cr = p["com_range"]
            if not isinstance(cr, dict) or not set(cr) <= {"x", "y", "z"}:
                raise NotImplementedError(f"events.base_com: com_range {cr!r} is not compiled; {compiled}")
            rng = tuple(tuple(float(v) for v in cr.get(k, (0.0, 0.0))) for k in ("x", "y", "z"))
            if any(a > b for a, b in rng):
                raise NotImplementedError(f"events.base_com: every com_range needs lo <= hi; {compiled}")
            out.com_enabled, out.com_range = True, rng
        return out


@dataclass
class Zbot6BFlatEnvCfg_PLAY(Zbot6BFlatEnvCfg):
    """flat_env_cfg.py:193-204: 64 envs, no corruption, commands over the limit ranges."""

    def __post_init__(self):
        self.scene.num_envs = 64
        self.scene.env_spacing = 2.5
        self.observations.policy.enable_corruption = False
        self.commands.base_velocity.ranges = self.commands.base_velocity.limit_ranges


BASE_INERTIA_SEED_SALT = 0x6261736D  # the startup mass / COM generator: seed ^ this ("basm")


def draw_base_inertia(dr: BaseInertiaEvents, num_envs: int, seed: int | None):
    """(mass [N], com_offset [N, 3]) float32 host tensors of the startup events: four U(0, 1) columns from
    a generator seeded with ``seed ^ BASE_INERTIA_SEED_SALT``, scaled to the ranges (a disabled event
    keeps the authored mass / a zero offset but still consumes its columns)."""
    g = torch.Generator().manual_seed((seed if seed is not None else 0) ^ BASE_INERTIA_SEED_SALT)
    u = torch.rand(num_envs, 4, generator=g, dtype=torch.float64)
    m0 = base_link_mass()
    mass = torch.full((num_envs,), m0, dtype=torch.float64)
    if dr.mass_enabled:
        lo, hi = dr.mass_range
        mass = torch.as_tensor(zm.base_mass_op(m0, (lo + (hi - lo) * u[:, 0]).numpy(), dr.mass_operation))
    com = torch.zeros(num_envs, 3, dtype=torch.float64)
    if dr.com_enabled:
        r = torch.tensor(dr.com_range, dtype=torch.float64)
        com = r[:, 0] + (r[:, 1] - r[:, 0]) * u[:, 1:]
    return mass.float(), com.float()


def _active(group) -> list:
    return [(f.name, getattr(group, f.name)) for f in fields(group) if getattr(group, f.name) is not None]


# ----------------------------------------------------------------------------- manager views
class _CommandManager:
    """The CommandManager accessors the reference's mdp / scripts use (get_command, get_term)."""

    def __init__(self, env: "ZbotManagerBasedRLEnv"):
        self._env = env

    # command_manager
    def get_command(self, name: str) -> torch.Tensor:
        if name != "base_velocity":
            raise KeyError(name)
        st = self._env.sim.get_state()
        return st[zm.M["COMMANDS"]:zm.M["COMMANDS"] + 3].T.contiguous()

    def get_term(self, name: str):
        if name != "base_velocity":
            raise KeyError(name)
        return _VelocityCommandTerm(self._env)


class _VelocityCommandTerm:
    """The ``base_velocity`` command term: its cfg's fields (``ranges``, ``limit_ranges``, ...) and the
    per-env buffers UniformVelocityCommand exposes (``command``, ``heading_target``, ``is_heading_env``)."""

    def __init__(self, env: "ZbotManagerBasedRLEnv"):
        object.__setattr__(self, "_env", env)
        object.__setattr__(self, "cfg", env.cfg.commands.base_velocity)

    def __getattr__(self, name: str):
        return getattr(self.cfg, name)

    def __setattr__(self, name: str, value) -> None:  # the term's fields are the cfg's: writes reach it too
        setattr(self.cfg, name, value)

    @property
    def command(self) -> torch.Tensor:
        return self._env.command_manager.get_command("base_velocity")

    def _event_row(self, row: int) -> torch.Tensor:
        sim = self._env.sim
        if not sim.events_configured:  # events off: UniformVelocityCommand's zero-initialised buffers
            return torch.zeros(sim.num_envs, dtype=torch.float32, device=sim.device)
        return sim.get_event_state()[row].contiguous()

    @property
    def heading_target(self) -> torch.Tensor:
        return self._event_row(zm.ME["HEADING_TARGET"])

    @property
    def is_heading_env(self) -> torch.Tensor:
        return self._event_row(zm.ME["IS_HEADING"]) > 0.5


class ZbotManagerBasedRLEnv(ZbotDirectEnvV2):
    """``ManagerBasedRLEnv`` over ``Zbot6BFlatEnvCfg`` on the MI355X simulator."""

    _ep_len_row = zm.M["EP_LEN"]

    def __init__(self, cfg: Zbot6BFlatEnvCfg | None = None, render_mode: str | None = None, **kwargs):
        cfg = cfg or Zbot6BFlatEnvCfg()
        super().__init__(cfg, render_mode=render_mode, **kwargs)
        self.command_manager = _CommandManager(self)
        self._set_observation_spaces(zm.M_OBS_DIM)

    def _startup(self) -> None:
        """Startup events: init_my_data (the feet buffers live in the state rows) and
        randomize_rigid_body_material over every body shape (64 buckets of static / dynamic
        friction ~ U[0.3, 1.0]; static and dynamic coefficients go to the solver)."""
        events = self.cfg.manager_events()
        if events.enabled:  # right after construction, before the first reset: construction semantics
            self.sim.set_manager_events(events)
        self._startup_base_inertia()
        terms = self.cfg.manager_terms()
        if terms.enabled:  # init_my_data: feet_force_sum, the contact timers and the five sums start at zero
            self.sim.set_manager_terms(terms)
        ev = self.cfg.events.physics_material
        if ev is None:
            return
        p = ev.params
        g = torch.Generator().manual_seed(self.cfg.seed if self.cfg.seed is not None else 0)
        ranges = torch.tensor([p["static_friction_range"], p["dynamic_friction_range"], p["restitution_range"]])
        nb = int(p["num_buckets"])
        self.material_buckets = torch.rand(nb, 3, generator=g) * (ranges[:, 1] - ranges[:, 0]) + ranges[:, 0]
        bucket_ids = torch.randint(0, nb, (self.num_envs, zm.NUM_LINKS), generator=g)
        self.link_materials = self.material_buckets[bucket_ids]
        self.sim.set_link_friction(self.link_materials[..., 0], self.link_materials[..., 1])

    def _startup_base_inertia(self) -> None:
        """Startup events add_base_mass / base_com: one uniform sample per env of the base link's mass
        (through the event's operation, from the authored mass) and of its COM offset, drawn on the host
        from a generator of their own (so the friction draws of the same seed do not move), one call
        into the simulator. ``base_mass`` [N] and ``base_com_offset`` [N, 3] keep what was drawn."""
        dr = self.cfg.base_inertia()
        if not dr.enabled:
            return
        self.base_mass, self.base_com_offset = draw_base_inertia(dr, self.num_envs, self.cfg.seed)
        self.sim.set_base_inertia(self.base_mass, self.base_com_offset, dr.recompute_inertia)

    def _update_log(self) -> None:
        """extras["log"] in ManagerBasedRLEnv._reset_idx order: Episode_Reward/<term> (reward
        manager: mean episodic sum / 20 s), Curriculum/lin_vel_cmd_levels, Metrics/base_velocity/*,
        Episode_Termination/<term> counts (device 0-dim tensors: no per-step host sync)."""
        if getattr(self, "_log", None) is None:
            means, counts = self.sim.read_log()
            buf = self.sim.log_buffer
            log = {f"Episode_Reward/{k}": buf[zm.m_log_slot(k)] for k in self.cfg.reward_terms()}
            if self.cfg.curriculum.lin_vel_cmd_levels is not None:
                log["Curriculum/lin_vel_cmd_levels"] = buf[16]
            log["Metrics/base_velocity/error_vel_xy"] = buf[17]
            log["Metrics/base_velocity/error_vel_yaw"] = buf[18]
            log["Episode_Termination/time_out"] = counts[1]
            log["Episode_Termination/base_height"] = counts[0]
            log["Episode_Termination/feet_close"] = counts[2]
            self._log = log
        self.extras["log"] = self._log

    @property
    def max_episode_length_s(self) -> float:
        return self.cfg.episode_length_s

    @max_episode_length_s.setter
    def max_episode_length_s(self, value) -> None:
        pass

    @property
    def reward_scales(self) -> dict:
        return {k: t.weight for k, t in _active(self.cfg.rewards)}

    @reward_scales.setter
    def reward_scales(self, value) -> None:  # set by the base __init__; the weights live in the cfg
        pass
