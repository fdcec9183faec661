"""Torch-facing handle on the HIP simulator (``libzbot.so``): one handle = N envs on one GPU.

All calls are stream-ordered on the current torch CUDA stream and never synchronise the host.
Persistent state lives in HBM, owned by the library (SoA ``[ZB_STATE_DIM][N]`` fp32).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _native as nat
from . import model as zm


def _stream(device: torch.device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class ZbotSim:
    def __init__(self, num_envs: int, cfg: zm.TaskCfg | None = None, device: str | torch.device = "cuda:0",
                 seed: int = 0, robot: zm.RobotModel | None = None):
        if num_envs < 1:
            raise ValueError("num_envs must be >= 1")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise nat.ZbotError("ZbotSim runs on a ROCm GPU only (device must be cuda:<i>); there is no CPU path")
        if not torch.cuda.is_available():
            raise nat.ZbotError("no ROCm GPU visible: the HIP simulator cannot run here")
        self.lib = nat.lib()
        self.num_envs = int(num_envs)
        self.cfg = cfg or zm.TaskCfg()
        self.task = self.cfg.task
        self.obs_dim, self.state_dim = self.cfg.obs_dim, self.cfg.state_dim
        self.num_terms = len(self.cfg.reward_terms)
        if robot is None:
            robot = (zm.standup_model() if self.task == zm.TASK_STANDUP_V0
                     else zm.load_v09_model() if self.task == zm.TASK_MANAGER_V0 else zm.load_model())
        self.robot = robot
        self._m = zm.pack_model(self.robot)
        self._c = self.cfg.pack()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(self.lib.zb_create(C.byref(self._m), C.byref(self._c), self.num_envs, idx, int(seed) & (2**64 - 1),
                                         C.byref(h)), "zb_create")
        self._h = h
        self.events_configured = False   # set_manager_events has been called (manager task)
        if self.lib.zb_state_dim(h) != self.state_dim:
            raise nat.ZbotError("libzbot state layout does not match zbot_lab_amd.model")
        # persistent outputs (reference: terminated/truncated buffers are mutated in place)
        self.terminated = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
        self.truncated = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
        self._log_means = torch.zeros(zm.LOG_LEN, dtype=torch.float32, device=self.device)  # include/zbot.h ZB_LOG_LEN
        self._log_counts = torch.zeros(zm.LOG_COUNTS, dtype=torch.int32, device=self.device)  # ZB_LOG_COUNTS
        # the library fills these in stream order at every step/reset with resets (no copies)
        nat.check(self.lib.zb_set_log_buffers(self._h, nat.ptr(self._log_means), nat.ptr(self._log_counts)),
                  "zb_set_log_buffers")

    # ------------------------------------------------------------------ lifecycle
    def close(self) -> None:
        if getattr(self, "_h", None):
            self.lib.zb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ ops
    def reset(self, env_ids: torch.Tensor | None = None) -> None:
        if env_ids is None:
            nat.check(self.lib.zb_reset(self._h, None, self.num_envs, _stream(self.device)), "zb_reset")
            return
        ids = env_ids.to(device=self.device, dtype=torch.int32).contiguous()
        if ids.numel() == 0:
            return
        nat.check(self.lib.zb_reset(self._h, nat.ptr(ids), ids.numel(), _stream(self.device)), "zb_reset")

    def step(self, actions: torch.Tensor):
        a = actions.to(device=self.device, dtype=torch.float32).contiguous()
        if a.shape != (self.num_envs, zm.ACT_DIM):
            raise ValueError(f"actions must be [{self.num_envs}, {zm.ACT_DIM}], got {tuple(a.shape)}")
        obs = torch.empty(self.num_envs, self.obs_dim, dtype=torch.float32, device=self.device)
        rew = torch.empty(self.num_envs, dtype=torch.float32, device=self.device)
        nat.check(self.lib.zb_step(self._h, nat.ptr(a), nat.ptr(obs), nat.ptr(rew), nat.ptr(self.terminated),
                                   nat.ptr(self.truncated), _stream(self.device)), "zb_step")
        return obs, rew, self.terminated, self.truncated

    def step_into(self, actions: torch.Tensor, obs: torch.Tensor, rew: torch.Tensor) -> None:
        """Allocation-free variant for benchmarking / graph capture (caller-owned outputs)."""
        nat.check(self.lib.zb_step(self._h, nat.ptr(actions), nat.ptr(obs), nat.ptr(rew), nat.ptr(self.terminated),
                                   nat.ptr(self.truncated), _stream(self.device)), "zb_step")

    def observe(self) -> torch.Tensor:
        obs = torch.empty(self.num_envs, self.obs_dim, dtype=torch.float32, device=self.device)
        nat.check(self.lib.zb_observe(self._h, nat.ptr(obs), _stream(self.device)), "zb_observe")
        return obs

    def kernel_variant(self) -> tuple:
        """(kTgs, kOcc, kRefresh, kRf): the template arguments of the step-kernel instantiation the
        next step() launches (zb_kernel_variant; host only)."""
        v = (C.c_int32 * 4)()
        nat.check(self.lib.zb_kernel_variant(self._h, v), "zb_kernel_variant")
        return tuple(int(x) for x in v)

    def read_log(self):
        """(term_means[num_terms], counts[ZB_LOG_COUNTS]) device tensors of the most recent step that had resets
        (registered with zb_set_log_buffers, so no per-step copy)."""
        return self._log_means[:self.num_terms], self._log_counts

    @property
    def log_buffer(self) -> torch.Tensor:
        """The whole float[ZB_LOG_LEN] log buffer (term means, then the curriculum entries)."""
        return self._log_means

    @property
    def log_count_buffer(self) -> torch.Tensor:
        """The int32[ZB_LOG_COUNTS] termination-count buffer."""
        return self._log_counts

    def done_buffer(self) -> torch.Tensor:
        """A persistent int64 [N] tensor that every later step fills with terminated | truncated from the step
        kernel's own flag stores (zb_set_done_buffer): rsl_rl's dones without the wrapper's two torch
        launches per step. Registered on first use; the same tensor afterwards."""
        if getattr(self, "_dones", None) is None:
            self._dones = torch.zeros(self.num_envs, dtype=torch.long, device=self.device)
            nat.check(self.lib.zb_set_done_buffer(self._h, nat.ptr(self._dones)), "zb_set_done_buffer")
        return self._dones

    @property
    def critic_obs_dim(self) -> int:
        """Width of the privileged critic row of this task (zb_critic_obs_dim; include/zbot_critic_obs.h)."""
        return int(self.lib.zb_critic_obs_dim(self._h))

    def critic_obs_buffer(self) -> torch.Tensor:
        """A persistent float32 [N, critic_obs_dim] tensor that every later step / reset fills with the critic
        rows of the state it leaves, in a launch of its own after the step's (zb_set_critic_obs_buffer).
        Registered and filled on first use; the same tensor afterwards, overwritten by the next step."""
        if getattr(self, "_critic", None) is None:
            self._critic = self.observe_critic()
            nat.check(self.lib.zb_set_critic_obs_buffer(self._h, nat.ptr(self._critic)), "zb_set_critic_obs_buffer")
        return self._critic

    def observe_critic(self) -> torch.Tensor:
        """The critic rows of the current state, on demand (zb_observe_critic)."""
        out = torch.empty(self.num_envs, self.critic_obs_dim, dtype=torch.float32, device=self.device)
        nat.check(self.lib.zb_observe_critic(self._h, nat.ptr(out), _stream(self.device)), "zb_observe_critic")
        return out

    # ------------------------------------------------------------------ manager events
    def set_manager_events(self, events: zm.ManagerEvents) -> None:
        """Manager task: configure the interval push and the yaw / heading commands
        (zb_set_manager_events; include/zbot_manager_events.h). Draws the push timers and the command's
        ang z / heading at the current stream position: call it right after construction."""
        self._events = events.pack()
        nat.check(self.lib.zb_set_manager_events(self._h, C.byref(self._events), _stream(self.device)),
                  "zb_set_manager_events")
        self.events_configured = True

    @property
    def events_active(self) -> bool:
        """Whether the next step launches zb_m_events_step_kernel instead of zb_m_step_kernel."""
        return bool(self.lib.zb_manager_events_active(self._h))

    def get_event_state(self) -> torch.Tensor:
        """The per-env event state [ME_STATE_DIM, N]: push time left, heading target, is-heading flag."""
        ev = torch.empty(zm.ME_STATE_DIM, self.num_envs, dtype=torch.float32, device=self.device)
        nat.check(self.lib.zb_get_manager_event_state(self._h, nat.ptr(ev), _stream(self.device)),
                  "zb_get_manager_event_state")
        return ev

    def set_event_state(self, ev: torch.Tensor) -> None:
        e = ev.to(device=self.device, dtype=torch.float32).contiguous()
        if e.shape != (zm.ME_STATE_DIM, self.num_envs):
            raise ValueError(f"event state must be [{zm.ME_STATE_DIM}, {self.num_envs}]")
        nat.check(self.lib.zb_set_manager_event_state(self._h, nat.ptr(e), _stream(self.device)),
                  "zb_set_manager_event_state")
        torch.cuda.current_stream(self.device).synchronize()  # `e` may be a temporary

    # ------------------------------------------------------------------ per-env base mass and COM
    def set_base_inertia(self, mass: torch.Tensor | None, com_offset: torch.Tensor | None = None,
                         recompute_inertia: bool = True) -> None:
        """Manager task: the base link's mass [N] (kg) and COM offset [N, 3] (m, link frame) per env
        (zb_set_base_inertia; include/zbot_base_inertia.h), Isaac Lab's randomize_rigid_body_mass /
        randomize_rigid_body_com. ``mass=None`` switches the feature off again. Never synchronises: a mass
        that is not positive and finite is refused on the device and reported by check_base_inertia()."""
        if mass is None:
            nat.check(self.lib.zb_set_base_inertia(self._h, None, 0, _stream(self.device)), "zb_set_base_inertia")
            return
        if self.task != zm.TASK_MANAGER_V0:
            raise nat.ZbotError("set_base_inertia: the per-env base mass and COM are manager-task events")
        m = mass.to(device=self.device, dtype=torch.float32).reshape(-1)
        c = (torch.zeros(self.num_envs, 3, device=self.device) if com_offset is None
             else com_offset.to(device=self.device, dtype=torch.float32))
        if m.shape != (self.num_envs,) or c.shape != (self.num_envs, 3):
            raise ValueError(f"mass must be [{self.num_envs}] and com_offset [{self.num_envs}, 3]")
        if getattr(self, "_base_link", None) is None:
            self._base_link = zm.pack_base_link(self.robot)
            nat.check(self.lib.zb_set_base_link(self._h, C.byref(self._base_link)), "zb_set_base_link")
        self._mass_com = torch.cat([m[:, None], c], dim=1).contiguous()  # kept alive: the launch reads it in stream order
        nat.check(self.lib.zb_set_base_inertia(self._h, nat.ptr(self._mass_com), int(bool(recompute_inertia)),
                                               _stream(self.device)), "zb_set_base_inertia")

    @property
    def base_inertia_active(self) -> bool:
        """Whether the next step launches zb_m_dr_step_kernel (per-env base mass properties)."""
        return bool(self.lib.zb_base_inertia_active(self._h))

    def check_base_inertia(self) -> None:
        """Raise if a set_base_inertia so far was given a mass the device refused (synchronises)."""
        nat.check(self.lib.zb_base_inertia_check(self._h, _stream(self.device)), "zb_base_inertia_check")

    def get_base_inertia(self) -> torch.Tensor:
        """The composed rows of the base composite body [12, N]: com xyz, mass, Ixx Iyy Izz Ixy, Ixz Iyz 0 0."""
        out = torch.empty(12, self.num_envs, dtype=torch.float32, device=self.device)
        nat.check(self.lib.zb_get_base_inertia(self._h, nat.ptr(out), _stream(self.device)), "zb_get_base_inertia")
        return out

    def get_base_link_com(self) -> torch.Tensor:
        """The per-env base-link COM in the body frame [3, N]."""
        out = torch.empty(3, self.num_envs, dtype=torch.float32, device=self.device)
        nat.check(self.lib.zb_get_base_link_com(self._h, nat.ptr(out), _stream(self.device)), "zb_get_base_link_com")
        return out

    # ------------------------------------------------------------------ the five more reward terms
    def set_manager_terms(self, terms: zm.ManagerTerms) -> None:
        """Manager task: activate gait / feet_clearance / feet_air_time / base_vel_forward /
        feet_force_pattern (zb_set_manager_terms; include/zbot_manager_terms.h). Zeroes the contact timers,
        the integrator and the five episode sums: call it right after construction."""
        self._terms = terms.pack(self.robot)
        nat.check(self.lib.zb_set_manager_terms(self._h, C.byref(self._terms), _stream(self.device)),
                  "zb_set_manager_terms")

    @property
    def terms_active(self) -> bool:
        """Whether the next step launches zb_m_terms_step_kernel."""
        return bool(self.lib.zb_manager_terms_active(self._h))

    def kernel_name(self) -> str:
        """The step kernel the next step() launches, by name (zb_kernel_variant_name; kernel_variant()
        gives its template arguments)."""
        return self.lib.zb_kernel_variant_name(self._h).decode()

    def get_terms_state(self) -> torch.Tensor:
        """[MT_GET_DIM, N]: the term state (contact timers, feet_force_sum, the five episode sums), then the
        terms' inputs on the current state (feet clearance heights and COM velocities, the forward vector,
        the root link's velocity); rows in ``model.MT``."""
        out = torch.empty(zm.MT_GET_DIM, self.num_envs, dtype=torch.float32, device=self.device)
        nat.check(self.lib.zb_get_manager_terms_state(self._h, nat.ptr(out), _stream(self.device)),
                  "zb_get_manager_terms_state")
        return out

    def set_terms_state(self, ts: torch.Tensor) -> None:
        t = ts.to(device=self.device, dtype=torch.float32).contiguous()
        if t.shape != (zm.MT_STATE_DIM, self.num_envs):
            raise ValueError(f"term state must be [{zm.MT_STATE_DIM}, {self.num_envs}]")
        nat.check(self.lib.zb_set_manager_terms_state(self._h, nat.ptr(t), _stream(self.device)),
                  "zb_set_manager_terms_state")
        torch.cuda.current_stream(self.device).synchronize()  # `t` may be a temporary

    def set_log_accumulator(self, acc: torch.Tensor | None) -> None:
        """Register a device float[ZB_LOG_LEN + ZB_LOG_COUNTS] accumulator that every later step adds the
        log's current values to inside its finalize launch (zb_set_log_accumulator; the PPO runner's
        per-rollout sum of extras["log"]); None unregisters. The tensor must stay alive while registered."""
        if acc is not None and (acc.dtype != torch.float32 or acc.device != self.device or not acc.is_contiguous()
                                or acc.numel() != zm.LOG_LEN + zm.LOG_COUNTS):
            raise ValueError(f"accumulator must be a contiguous float32 [{zm.LOG_LEN + zm.LOG_COUNTS}] tensor on {self.device}")
        self._log_acc_ref = acc
        nat.check(self.lib.zb_set_log_accumulator(self._h, nat.ptr(acc)), "zb_set_log_accumulator")

    def set_link_friction(self, mu: torch.Tensor, mu_dynamic: torch.Tensor | None = None) -> None:
        """Standup / manager: per-link static (and dynamic; default = static) friction [N, 12]
        (randomize_rigid_body_material)."""
        m = mu.to(device=self.device, dtype=torch.float32).contiguous()
        md = m if mu_dynamic is None else mu_dynamic.to(device=self.device, dtype=torch.float32).contiguous()
        for t in (m, md):
            if t.shape != (self.num_envs, zm.NUM_LINKS):
                raise ValueError(f"friction must be [{self.num_envs}, {zm.NUM_LINKS}]")
        nat.check(self.lib.zb_set_link_friction_sd(self._h, nat.ptr(m), nat.ptr(md), _stream(self.device)),
                  "zb_set_link_friction_sd")
        torch.cuda.current_stream(self.device).synchronize()  # `m` may be a temporary

    def read_curriculum(self):
        """(curriculum stage, common_step_counter) from the device (synchronises)."""
        st, n = C.c_int32(), C.c_int64()
        nat.check(self.lib.zb_read_curriculum(self._h, C.byref(st), C.byref(n)), "zb_read_curriculum")
        return int(st.value), int(n.value)

    def get_state(self) -> torch.Tensor:
        st = torch.empty(self.state_dim, self.num_envs, dtype=torch.float32, device=self.device)
        nat.check(self.lib.zb_get_state(self._h, nat.ptr(st), _stream(self.device)), "zb_get_state")
        return st

    def set_state(self, st: torch.Tensor) -> None:
        s = st.to(device=self.device, dtype=torch.float32).contiguous()
        if s.shape != (self.state_dim, self.num_envs):
            raise ValueError(f"state must be [{self.state_dim}, {self.num_envs}]")
        nat.check(self.lib.zb_set_state(self._h, nat.ptr(s), _stream(self.device)), "zb_set_state")
        torch.cuda.current_stream(self.device).synchronize()  # `s` may be a temporary

    def get_contact_cache(self) -> torch.Tensor:
        """the solver's persistent self-contact cache [ZB_WARM_ROWS, N] (include/zbot.h)"""
        wc = torch.empty(16, self.num_envs, dtype=torch.float32, device=self.device)
        nat.check(self.lib.zb_get_contact_cache(self._h, nat.ptr(wc), _stream(self.device)), "zb_get_contact_cache")
        return wc

    def set_contact_cache(self, wc: torch.Tensor) -> None:
        w = wc.to(device=self.device, dtype=torch.float32).contiguous()
        if w.shape != (16, self.num_envs):
            raise ValueError(f"contact cache must be [16, {self.num_envs}]")
        nat.check(self.lib.zb_set_contact_cache(self._h, nat.ptr(w), _stream(self.device)), "zb_set_contact_cache")
        torch.cuda.current_stream(self.device).synchronize()

    def profile_begin(self, max_launches: int, stride: int = 1) -> None:
        """Time the next zb_step_kernel launches with HIP events: every ``stride``-th one, at most
        ``max_launches`` of them (the event dispatch adds ~5.7 us to a step it brackets)."""
        nat.check(self.lib.zb_profile_stride(self._h, int(stride)), "zb_profile_stride")
        nat.check(self.lib.zb_profile_begin(self._h, int(max_launches)), "zb_profile_begin")

    def profile_end(self):
        """(summed zb_step_kernel milliseconds, launches timed)."""
        ms, n = C.c_float(), C.c_int()
        nat.check(self.lib.zb_profile_end(self._h, C.byref(ms), C.byref(n)), "zb_profile_end")
        return float(ms.value), int(n.value)

    def physics_substeps(self, targets: torch.Tensor, nsub: int):
        t = targets.to(device=self.device, dtype=torch.float32).contiguous()
        nf = torch.zeros(self.num_envs, zm.NUM_LINKS, 3, dtype=torch.float32, device=self.device)
        tau = torch.zeros(self.num_envs, zm.NUM_DOF, dtype=torch.float32, device=self.device)
        nat.check(self.lib.zb_physics_substeps(self._h, nat.ptr(t), int(nsub), nat.ptr(nf), nat.ptr(tau),
                                               _stream(self.device)), "zb_physics_substeps")
        return nf, tau
