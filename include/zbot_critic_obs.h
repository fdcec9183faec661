/*
 * zbot_critic_obs.h — privileged critic observations of libzbot.so (asymmetric actor-critic; rsl_rl's
 * "critic" observation group, as the reference's zbot2_env_s2r_v0.py returns it in
 * extras["observations"]["critic"]). Included by zbot.h; do not include it on its own.
 *
 * These entry points are kept out of zbot.h itself because that header is the surface the CPU oracle
 * mirrors symbol for symbol (zbo_*); the critic rows have no oracle mirror. They are checked against
 * an fp64 restatement from zb_get_state and the model (tests/test_gpu_critic_obs.py).
 *
 * One row per env, float[N][D] row-major, D = zb_critic_obs_dim(h) <= ZB_MAX_CRITIC_OBS_DIM (the PPO
 * kernels' input limit): walking v2 23 + 7 = 30, stand-up 22 + 7 = 29, walking v4 24 + 7 = 31,
 * manager 25 + 7 = 32. Row contents, in this order:
 *
 *   [0, P)  the task's policy observation (P = its observation width) without corruption. Walking v2,
 *           v4 and stand-up have no observation noise: the block is bit-identical to zb_observe on the
 *           same state. Manager: the same terms with the additive noise draw omitted (and no RNG use).
 *   P + 0..2  linear velocity of the base link's frame origin, in the base link's frame (m/s)
 *   P + 3     height of the base link's frame origin above the ground plane (m)
 *   P + 4..5  the two feet's newest vertical contact force (the contact sensor's history slot 0,
 *             foot_0 then foot_1), divided by the robot's weight (sum of body_mass x cfg.gravity).
 *             Stand-up keeps no contact sensor in its state: both are 0 there.
 *   P + 6     the env's friction coefficient: the mean of the two feet's static coefficient as
 *             zb_set_link_friction* set it (stand-up, manager; cfg.friction where nothing was set),
 *             cfg.friction for the uniform-material tasks (walking v2, v4)
 *
 * The tail is a function of the state (zb_get_state), the model constants and the per-env friction
 * only. With no buffer registered nothing changes: no extra launch, the same step kernels.
 */
#ifndef ZBOT_CRITIC_OBS_H_
#define ZBOT_CRITIC_OBS_H_

#define ZB_CRITIC_TAIL_DIM 7
#define ZB_MAX_CRITIC_OBS_DIM 32

/* D of the handle's task (host only, no HIP call). */
int zb_critic_obs_dim(zb_handle h);

/* Register a caller-owned device float[N][D]: while registered, every zb_step and zb_reset launches
 * the critic-observation kernel on the call's stream after its step / finalize launches, so the rows
 * describe the post-step state and reset envs show their post-reset state, exactly as the policy
 * observation does. The kernel boundary is the only ordering (no host synchronisation, no fences);
 * capturable in a graph. NULL unregisters. */
int zb_set_critic_obs_buffer(zb_handle h, float* buf);

/* The rows of the current state on demand, beside zb_observe. dst: device float[N][D]. */
int zb_observe_critic(zb_handle h, float* dst, void* stream);

#endif /* ZBOT_CRITIC_OBS_H_ */
