/*
 * zbot_manager_terms.h — the manager task's five reward terms that the flat cfg switches off and the
 * reference's base cfg defines (zbot-6b-walking-m-v0; zbotlab_env_cfg.py:261-366 over mdp/rewards.py):
 * gait, feet_clearance, feet_air_time, base_vel_forward, feet_force_pattern. Included by zbot.h; do not
 * include it on its own.
 *
 * Kept out of zbot.h itself for the reason zbot_manager_events.h is: zb_task_cfg, zb_model, the manager
 * state rows (ZB_M_STATE_DIM = 100) and ZB_M_NUM_REWARD_TERMS = 11 are the surface the CPU oracle mirrors,
 * and they do not change. The configuration below and the per-env state the terms need live beside them,
 * in a library-owned side buffer that zb_create allocates for manager handles. A handle that never
 * activates a term here launches the same step kernels and computes the same bits as before.
 *
 * While any term is active zb_step launches zb_m_terms_step_kernel: one more build of the manager step
 * kernel's text with the events (zbot_manager_events.h) and the per-env base inertia
 * (zbot_base_inertia.h) compiled in, so it serves every combination (a handle with those off runs it
 * with all-off event parameters and the nominal base rows). Everything below is computed after the
 * substep loop from data the kernel already holds.
 *
 * Semantics, per env and per zb_step, on the post-step (pre-reset) state, with step_dt = sim_dt *
 * decimation, the command as the previous step left it, and ep = episode_length_buf after this step's
 * increment. The reward is the sum of term * weight * step_dt over the sixteen reward fields in cfg
 * order (track_lin_vel_xy_exp, track_ang_vel_z_exp, termination_penalty, dof_torques_l2, dof_acc_l2,
 * action_rate_l2, foot_step_length, foot_downward, foot_forward, GAIT, feet_slide, FEET_CLEARANCE,
 * FEET_AIR_TIME, air_time_variance, BASE_VEL_FORWARD, FEET_FORCE_PATTERN); a term that is not active
 * contributes nothing and keeps no state.
 *
 *   contact timers     ContactSensor.current_contact_time of the feet: per substep, next to the air
 *                      timers, t = in contact ? t + sim_dt : 0 (in contact: |net force| >
 *                      contact_force_threshold). After any update exactly one of {current_air_time,
 *                      current_contact_time} of a foot is positive; both are zero after a reset.
 *   gait               feet_gait: phase = ((ep * step_dt) % period) / period, leg phase f =
 *                      (phase + offset[f]) % 1, stance f = leg phase f < threshold; the count of feet
 *                      whose (current_contact_time > 0) equals its stance; times (|command| over all
 *                      three components > 0.05). fp32 arithmetic in the reference's order.
 *   feet_clearance     foot_clearance_reward: exp(-sum_f (z_f - target_height)^2 *
 *                      tanh(tanh_mult * |v_f xy|) / std), z_f the world height of the foot's clearance
 *                      point (clearance_point, body frame of the foot's composite body; the caller passes
 *                      the foot link's COM), v_f the foot link's COM velocity.
 *   feet_air_time      feet_air_time_positive_biped: with exactly one foot in contact, the smaller of
 *                      the two feet's time in their current mode (contact time of the one, air time of
 *                      the other), clamped to the threshold; else 0; times (|command xy| > 0.1).
 *   base_vel_forward   root_link_lin_vel_w . (g x quat_apply(root_quat, (0, which_forward, 0))), g the
 *                      unit gravity direction: which_forward times the forward vector of the other terms.
 *   feet_force_pattern with F_f the mean of the foot's 3-slot F_z history:
 *                      d = (F_1 - F_0) * sign(feet_force_sum)   (sign(0) = 0, the integrator before its update)
 *                      feet_force_sum += 0.001 * (F_0 - F_1);  term = 0.5 d - 0.1 |feet_force_sum|.
 *                      The integrator advances only while the term is active; reset_my_data zeroes it.
 *   episode sums       sum += term * weight * step_dt per active term; a reset logs them into
 *                      Episode_Reward slots 11..15 of the episode log (zb_read_log) and zeroes them. A
 *                      step whose physics blew up (non-finite state) adds nothing, as for the 11.
 */
#ifndef ZBOT_MANAGER_TERMS_H_
#define ZBOT_MANAGER_TERMS_H_

enum zb_manager_extra_term {
  ZB_MT_GAIT = 0, ZB_MT_FEET_CLEARANCE, ZB_MT_FEET_AIR_TIME, ZB_MT_BASE_VEL_FORWARD, ZB_MT_FEET_FORCE_PATTERN,
  ZB_MT_NUM_TERMS
};

typedef struct zb_manager_terms {
  uint32_t active;                 /* bit t: term t (zb_manager_extra_term) is in the cfg */
  float weight[ZB_MT_NUM_TERMS];   /* RewTerm.weight; 0 for an absent term */
  float gait_period;               /* 2.0 */
  float gait_offset[2];            /* [0, 0.5] */
  float gait_threshold;            /* 0.55 */
  float clearance_std;             /* 0.05 */
  float clearance_tanh_mult;       /* 2.0 */
  float clearance_target_height;   /* 0.01 */
  float clearance_point[2][3];     /* per foot: the point whose height is read, body frame */
  float air_time_threshold;        /* 0.3 */
  float which_forward;             /* +1 / -1 */
} zb_manager_terms;

/* Rows of the per-env term state, SoA float[ZB_MT_STATE_DIM][N]. */
enum zb_manager_terms_state_field {
  ZB_MT_CONTACT_CUR = 0,    /* 2  ContactSensor current_contact_time[feet] (s) */
  ZB_MT_FEET_FORCE_SUM = 2, /* 1  env.feet_force_sum */
  ZB_MT_EP_SUMS = 3,        /* 5  episode sums of the five terms */
  ZB_MT_STATE_DIM = 8
};
/* What zb_get_manager_terms_state appends to the state rows (tests: the inputs of the terms, evaluated
 * on the handle's current state by the out-of-line kinematics the observation kernels use). */
enum zb_manager_terms_derived_field {
  ZB_MT_D_FOOT_Z = 8,       /* 2  world height of each foot's clearance point */
  ZB_MT_D_FOOT_VXY = 10,    /* 4  [foot][x, y] COM velocity of each foot link */
  ZB_MT_D_FWD_XY = 14,      /* 2  the forward vector g x quat_apply(root_quat, y) (z is 0) */
  ZB_MT_D_ROOT_VEL = 16,    /* 3  root_link_lin_vel_w (the base link's origin) */
  ZB_MT_GET_DIM = 19
};

/* Manager task only (another task: -1 and zb_last_error, before any launch). Needs gait_period > 0,
 * clearance_std > 0, which_forward = +-1 and finite weights. active == 0 switches the feature off again:
 * the next zb_step launches what it launched before. The timers, the integrator and the sums are zeroed
 * and the configuration goes to its device copy (a memset and one small launch on `stream`; no allocation,
 * never synchronises), so call it at construction or
 * right before a reset. */
int zb_set_manager_terms(zb_handle h, const zb_manager_terms* terms, void* stream);

/* 1 while the handle's next zb_step launches zb_m_terms_step_kernel, else 0. Host only. */
int zb_manager_terms_active(zb_handle h);

/* The step kernel the handle's next zb_step launches, by name: "zb_step_kernel", "zb_su_step_kernel",
 * "zb_v4_step_kernel", and for the manager task "zb_m_step_kernel", "zb_m_events_step_kernel",
 * "zb_m_dr_step_kernel" or "zb_m_terms_step_kernel" (zb_kernel_variant gives the template arguments the
 * builds share; the dispatch and this name come from one function). Host only; NULL for a NULL handle. */
const char* zb_kernel_variant_name(zb_handle h);

/* The term state (tests and lock-step tools). get: device float[ZB_MT_GET_DIM][N], the ZB_MT_STATE_DIM
 * state rows then the derived rows of the handle's current state. set: device float[ZB_MT_STATE_DIM][N].
 * Manager handles only. */
int zb_get_manager_terms_state(zb_handle h, float* dst, void* stream);
int zb_set_manager_terms_state(zb_handle h, const float* src, void* stream);

#endif /* ZBOT_MANAGER_TERMS_H_ */
