/*
 * zbot_manager_events.h — the manager task's interval push event and its yaw / heading commands
 * (zbot-6b-walking-m-v0: events.push_robot of the reference's base cfg, zbotlab_env_cfg.py:253-258,
 * and UniformVelocityCommand's ang_vel_z / heading_command, zbotlab_env_cfg.py:86-97). Included by
 * zbot.h; do not include it on its own.
 *
 * Kept out of zbot.h itself because that header is the surface the CPU oracle mirrors (zbo_*) and
 * compiles against: zb_task_cfg, zb_model and the manager state rows (ZB_M_STATE_DIM = 100) do not
 * change. The configuration below and the per-env state it needs live beside them, in a
 * library-owned side buffer like the contact cache. A handle that never enables anything here
 * launches the same step kernels, reads the same draws and computes the same bits as before.
 *
 * Semantics (Isaac Lab's ManagerBasedRLEnv.step order: _reset_idx, CommandManager.compute, the
 * interval events, ObservationManager.compute), per env and per zb_step, with
 * step_dt = sim_dt * decimation:
 *
 *   push timer   drawn U(push_interval_s) when zb_set_manager_events is called (construction) and
 *                again for every env that resets (in-step auto-reset, zb_reset with ids or full:
 *                EventManager.reset of an interval term without global time). Then, for every env,
 *                t -= step_dt; where t < 1e-6 the event fires and t is redrawn U(push_interval_s).
 *                An env that reset in this step has a fresh timer (advanced by this step's step_dt
 *                like every other) and does not fire; should push_interval_s[0] < step_dt let it
 *                run out at once, it fires in the next step.
 *   push         push_by_setting_velocity: six uniform components (dv, dw) ~ U(push_velocity_range)
 *                are added to the velocity of the articulation root, which is the base link
 *                (zb_model.api_root_link) at its centre of mass c; joint rates are unchanged. The
 *                whole robot gains one rigid velocity field: a point x gains dv + dw x (x - c), world
 *                frame. Stored in the chain root's twist: ROOT_ANGVEL += dw,
 *                ROOT_LINVEL += dv + dw x (ROOT_POS - c). The push acts after the step's rewards,
 *                terminations and command update; the observation holds no base velocity.
 *   command      on a resample (reset, and the cmd_resample_s timer) ang z ~ U(cmd_ang_vel_z) beside
 *                the lin x, lin y and standing draws; with heading_command also the heading target
 *                ~ U(cmd_heading) and is-heading = (u <= cmd_rel_heading). Every step after the
 *                resample, for heading envs:
 *                  command[2] = clip(heading_stiffness * wrap_to_pi(target - heading_w), cmd_ang_vel_z)
 *                  heading_w  = atan2(f_y, f_x), f the base link's x axis in the world (the post-reset
 *                               orientation on a reset step)
 *                then standing envs are zeroed, as before. The metric update reads the command as
 *                the previous step left it. A zb_reset stores the drawn ang z; the heading rule
 *                first applies in the next step, like the standing rule.
 *
 * Draw indices added to the manager's per-env counter stream: 8 push timer (reset);
 * 12, 13, 14 ang z, heading target, is-heading (reset); 32, 33, 34 the same three at the timer
 * resample; 35 push timer (redraw on fire); 36..41 the six push components.
 */
#ifndef ZBOT_MANAGER_EVENTS_H_
#define ZBOT_MANAGER_EVENTS_H_

typedef struct zb_manager_events {
  int32_t push_enabled;             /* events.push_robot present */
  float push_interval_s[2];         /* interval_range_s; [0] > 0 */
  float push_velocity_range[6][2];  /* x, y, z, roll, pitch, yaw; keys absent from the dict are (0, 0) */
  float cmd_ang_vel_z[2];           /* ranges.ang_vel_z */
  int32_t heading_command;
  float cmd_heading[2];             /* ranges.heading */
  float cmd_rel_heading;            /* rel_heading_envs */
  float heading_stiffness;          /* heading_control_stiffness */
} zb_manager_events;

/* Rows of the per-env event state, SoA float[ZB_ME_STATE_DIM][N]. */
enum zb_manager_event_state_field {
  ZB_ME_PUSH_TIME_LEFT = 0, /* s */
  ZB_ME_HEADING_TARGET = 1, /* rad */
  ZB_ME_IS_HEADING = 2,     /* 0 / 1 */
  ZB_ME_STATE_DIM = 3
};

/* Manager task only (another task: -1 and zb_last_error, before any launch). Checks lo <= hi for every
 * range and push_interval_s[0] > 0 (when the push is enabled). Draws the initial timers (and the
 * construction command's ang z / heading draws) into the side buffer, which zb_create allocated, at
 * the handle's current stream position, so calling it right after zb_create, before the first
 * zb_reset, gives construction semantics. With push, heading and the ang z range all off the handle
 * goes back to the events-off kernel. Host-side plus one small launch on `stream` (also when
 * everything is off: the state rows are rewritten); no allocation, never synchronises. */
int zb_set_manager_events(zb_handle h, const zb_manager_events* ev, void* stream);

/* 1 while the handle's next zb_step launches the events build of the manager step kernel
 * (zb_m_events_step_kernel in place of zb_m_step_kernel; zb_kernel_variant names the template
 * arguments the two share), else 0. Host only. */
int zb_manager_events_active(zb_handle h);

/* The event state (tests and lock-step tools, the role of zb_get_state / zb_set_state; zb_set_state
 * does not touch it). ZB_ME_STATE_DIM for a manager handle, -1 otherwise; get / set need a manager
 * handle (all zero until zb_set_manager_events). Device pointers float[ZB_ME_STATE_DIM][N]. */
int zb_manager_event_state_dim(zb_handle h);
int zb_get_manager_event_state(zb_handle h, float* dst, void* stream);
int zb_set_manager_event_state(zb_handle h, const float* src, void* stream);

#endif /* ZBOT_MANAGER_EVENTS_H_ */
