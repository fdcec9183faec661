// zbot-6b-walking-m-v0, the manager-based env. In order: commands and the draw-index map; feature 1, the
// interval push and yaw / heading commands (zbot_manager_events.h); feature 2, the five more reward terms
// (zbot_manager_terms.h); the step kernel, four stamps of zbot_m_step.inc; the terms' kernels; feature 3, the
// per-env base mass and COM (zbot_base_inertia.h); reset / observe. Each part sits under its own banner.
// Included by zbot_sim.hip inside its anonymous namespace; needs everything above the #include (ST / CST /
// OUT defined; zb_m_reset_kernel #undefs them).

// =========================================================================== manager-based env
// zbot-6b-walking-m-v0 (reference tasks/zbotlab_manager: zbotlab_env_cfg.py = "mgr.py",
// config/zbot6b_manager/flat_env_cfg.py, mdp/rewards.py, terminations.py, curriculums.py) on
// ZBOT_6S_V2_CFG (zbot_6s_v09.usd, rooted at the base link). ManagerBasedRLEnv.step order: action
// (RelativeJointPositionAction re-targets q + delta every substep), 4 x (substep, scene.update:
// the contact sensor with history_length 3 > 0 updates every physics step), terminations,
// rewards, resets (curriculum, events, managers), command update, observations with noise.

// world angular velocity of body b (root twist + the joint rates before it)
__device__ __forceinline__ void body_ang_vel_q(const Phys& s, const float S[ND][6], int b, float w[3]) {
  w[0] = s.av[0]; w[1] = s.av[1]; w[2] = s.av[2];
#pragma unroll
  for (int j = 0; j < ND; ++j)
    if (j < b)
#pragma unroll
      for (int a = 0; a < 3; ++a) w[a] += S[j][a] * s.jqd[j];
}

// UniformVelocityCommand._resample_command: lin x ~ U(ranges.lin_vel_x) (cnt->vel), lin y ~
// U(ranges.lin_vel_y) (cnt->yaw holds the lin_vel_y range for this task), ang z ~ U(0, 0),
// standing ~ U(0, 1) <= rel_standing_envs; draws k0 .. k0 + 2
__device__ __forceinline__ void m_resample(const zb_task_cfg& cfg, const Counters* cnt, uint64_t h, int k0, float cmd[3],
                                           float& standing) {
  cmd[0] = draw(h, k0) * (cnt->vel[1] - cnt->vel[0]) + cnt->vel[0];
  cmd[1] = draw(h, k0 + 1) * (cnt->yaw[1] - cnt->yaw[0]) + cnt->yaw[0];
  cmd[2] = 0.f;
  standing = draw(h, k0 + 2) <= cfg.cmd_rel_standing ? 1.f : 0.f;
}
constexpr int M_DRAW_RESET_CMD = 5, M_DRAW_CMD = 9, M_DRAW_NOISE = 16;  // reset_pose uses draws 1..4

// ------------------------------------------------------------- interval push, yaw / heading commands
// include/zbot_manager_events.h. The draws are new indices of the same per-env stream: the push timer
// at a reset, {ang z, heading target, is-heading} at a reset and at the timer resample, the push
// timer redrawn on a fire, the six push components.
constexpr int M_DRAW_RESET_PUSH_T = 8, M_DRAW_RESET_YAW = 12, M_DRAW_YAW = 32, M_DRAW_PUSH_T = 35, M_DRAW_PUSH = 36;
static_assert(M_DRAW_RESET_CMD + 3 <= M_DRAW_RESET_PUSH_T && M_DRAW_CMD + 3 <= M_DRAW_RESET_YAW &&
              M_DRAW_RESET_YAW + 3 <= M_DRAW_NOISE && M_DRAW_NOISE + 4 + 2 * ND <= M_DRAW_YAW &&
              M_DRAW_YAW + 3 <= M_DRAW_PUSH_T && M_DRAW_PUSH_T < M_DRAW_PUSH, "manager draw-index map (DESIGN.md §6)");

// zb_m_events_step_kernel's extra arguments as one record: the configuration and the side buffer
// (SoA [ZB_ME_STATE_DIM][N]); zb_m_step_kernel has an empty one.
template <bool kEvents>
struct MEv {};
template <>
struct MEv<true> {
  zb_manager_events c;
  float* st;
};
// the staging-row entries of the event state, after {reward, terminated, truncated}
constexpr int M_STG_EV = ZB_M_LINK_MU + ZB_M_OBS_DIM + 3;
static_assert(M_STG_EV + ZB_ME_STATE_DIM <= STG_LEN, "staging row");

__device__ __forceinline__ float m_uniform(uint64_t h, int k, const float r[2]) { return draw(h, k) * (r[1] - r[0]) + r[0]; }

// UniformVelocityCommand._resample_command, the part m_resample leaves at 0: ang z ~ U(ranges.ang_vel_z);
// with heading_command the heading target ~ U(ranges.heading) and is_heading_env = u <= rel_heading_envs;
// draws k0 .. k0 + 2
__device__ __forceinline__ void m_resample_yaw(const zb_manager_events& ev, uint64_t h, int k0, float& ang_z,
                                               float& target, float& is_heading) {
  ang_z = m_uniform(h, k0, ev.cmd_ang_vel_z);
  target = ev.heading_command ? m_uniform(h, k0 + 1, ev.cmd_heading) : 0.f;
  is_heading = ev.heading_command && draw(h, k0 + 2) <= ev.cmd_rel_heading ? 1.f : 0.f;
}

// UniformVelocityCommand._update_command for a heading env: ang z from the heading error of the base
// link's x axis (bq: the base link's world quaternion)
__device__ __forceinline__ void m_heading_cmd(const zb_manager_events& ev, const float bq[4], float target,
                                              float is_heading, float cmd[3]) {
  if (ev.heading_command && is_heading > 0.5f) {
    const float hw = atan2f(2.f * (bq[0] * bq[3] + bq[1] * bq[2]), 1.f - 2.f * (bq[2] * bq[2] + bq[3] * bq[3]));
    cmd[2] = clampf(ev.heading_stiffness * wrap_to_pi(target - hw), ev.cmd_ang_vel_z[0], ev.cmd_ang_vel_z[1]);
  }
}

// push_by_setting_velocity: (dv, dw) ~ U(push_velocity_range) added to the velocity of the articulation
// root (the base link, zb_model.api_root_link) at its COM c, joint rates unchanged: one rigid velocity
// field dv + dw x (x - c) over the whole robot, i.e. in the chain root's twist (linear part at
// p.pos) av += dw, lv += dv - dw x (c - p.pos). Reads the published body frames of the current pose.
// kLc: the root link's COM (body frame) from lcp instead of the model (the per-env base-link COM).
template <bool kLc = false>
__device__ __forceinline__ void m_push(MP m, const Q& q, const zb_manager_events& ev, uint64_t h, Phys& p,
                                       const float* lcp = nullptr) {
  float d[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) d[k] = m_uniform(h, M_DRAW_PUSH + k, ev.push_velocity_range[k]);
  const int l = m->api_root_link;
  float R[9], pb[3], lc[3], c[3], wc[3];
  read_frame(q, link_body(l), R, pb);
  if constexpr (kLc) { lc[0] = lcp[0]; lc[1] = lcp[1]; lc[2] = lcp[2]; }
  else ldc(lc, m->link_com[l]);
  mv3(R, lc, c);
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] += pb[a];
  cross3(d + 3, c, wc);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    p.av[a] += d[3 + a];
    p.lv[a] += d[a] - wc[a];
  }
}

// a reset env's event state (EventManager.reset: the push timer; the command term's reset: ang z, the
// heading target and flag), one thread per env: zb_m_reset_kernel and zb_m_events_init_kernel
__device__ __forceinline__ void m_reset_events(const zb_manager_events& evc, uint64_t hs, int N, int i,
                                               float* __restrict__ ev, float& ang_z) {
  float target, is_heading;
  m_resample_yaw(evc, hs, M_DRAW_RESET_YAW, ang_z, target, is_heading);
  ev[(size_t)ZB_ME_PUSH_TIME_LEFT * N + i] = evc.push_enabled ? m_uniform(hs, M_DRAW_RESET_PUSH_T, evc.push_interval_s) : 0.f;
  ev[(size_t)ZB_ME_HEADING_TARGET * N + i] = target;
  ev[(size_t)ZB_ME_IS_HEADING * N + i] = is_heading;
}

// the event-state entries of the staging row out to the side buffer: one store of the wave
__device__ __forceinline__ void m_ev_store(const Q& q, int env0, int N, float* __restrict__ ev) {
  wave_sync();
  const float* S = reinterpret_cast<const float*>(q.b + YG_OFF);
  const int e = q.lane % EPW, f0 = q.lane / EPW;
  const int env = env0 + e;
  if (env < N && f0 < ZB_ME_STATE_DIM) ev[(size_t)f0 * N + env] = S[e * STG_LEN + M_STG_EV + f0];
}

// the policy observation group (mgr.py:136-161, corruption on): root quat, command, joint pos rel,
// joint vel rel (Isaac Lab joint order), last action; additive U(-n, n) noise from draws 16..37
__device__ __forceinline__ void m_write_obs(MP m, const zb_task_cfg& cfg, uint64_t h, const float bq[4],
                                            const float cmd[3], const Phys& p, const float a_obs[ND], float* o) {
  const float cor = cfg.obs_corruption ? 1.f : 0.f;
  auto noise = [&](int k, float n) { return cor * (draw(h, M_DRAW_NOISE + k) * (2.f * n) - n); };
#pragma unroll
  for (int a = 0; a < 4; ++a) o[a] = bq[a] + noise(a, cfg.obs_noise[0]);
#pragma unroll
  for (int a = 0; a < 3; ++a) o[4 + a] = cmd[a];
#pragma unroll
  for (int j = 0; j < ND; ++j) {
    const int ai = m->api_joint_index[j];
    const float sg = m->api_joint_sign[j];
    o[7 + ai] = sg * (p.jq[j] - m->default_joint_pos[j]) + noise(4 + ai, cfg.obs_noise[1]);
    o[13 + ai] = sg * p.jqd[j] + noise(10 + ai, cfg.obs_noise[2]);
  }
#pragma unroll
  for (int a = 0; a < ND; ++a) o[19 + a] = a_obs[a];
}

// ------------------------------------------------------------- the five more reward terms
// include/zbot_manager_terms.h. zb_m_terms_step_kernel's extra arguments as one record (MEv's pattern):
// the configuration and the side buffer (SoA [ZB_MT_STATE_DIM][N]).
template <bool kTerms>
struct MTerms {};
template <>
struct MTerms<true> {
  const zb_manager_terms* c;  // device copy of the configuration: read in the reward epilogue only
  float* st;
};
// the staging-row entries of the term state, after the event state
constexpr int M_STG_TERMS = M_STG_EV + ZB_ME_STATE_DIM;
static_assert(M_STG_TERMS + ZB_MT_STATE_DIM <= STG_LEN && ZB_MT_STATE_DIM <= WGT / EPW, "staging row");
static_assert(ZB_M_NUM_REWARD_TERMS + ZB_MT_NUM_TERMS <= ZB_MAX_REWARD_TERMS, "episode-log slots 11..15");
// RewardsCfg field order (zbotlab_env_cfg.py:261-366 without undesired_contacts): t >= 0 the compiled
// term zb_manager_reward_term t, t < 0 the extra term -1 - t
__device__ constexpr int M_CFG_ORDER[ZB_M_NUM_REWARD_TERMS + ZB_MT_NUM_TERMS] = {
    ZB_M_R_TRACK_LIN_VEL_XY, ZB_M_R_TRACK_ANG_VEL_Z, ZB_M_R_TERMINATION, ZB_M_R_DOF_TORQUES, ZB_M_R_DOF_ACC,
    ZB_M_R_ACTION_RATE, ZB_M_R_FOOT_STEP_LENGTH, ZB_M_R_FOOT_DOWNWARD, ZB_M_R_FOOT_FORWARD, -1 - ZB_MT_GAIT,
    ZB_M_R_FEET_SLIDE, -1 - ZB_MT_FEET_CLEARANCE, -1 - ZB_MT_FEET_AIR_TIME, ZB_M_R_AIR_TIME_BALANCE,
    -1 - ZB_MT_BASE_VEL_FORWARD, -1 - ZB_MT_FEET_FORCE_PATTERN};

// the term state into the carry rows behind the event state, in the prologue's load batch: lane s of the
// team loads row s (carry_prefetch has zeroed these entries; the wave's LDS writes land in program order)
constexpr int M_CST_TERMS = ZB_M_LINK_MU + ZB_ME_STATE_DIM;
static_assert(M_CST_TERMS + ZB_MT_STATE_DIM - CARRY0 <= CARRY_W && ZB_MT_STATE_DIM <= TL, "carry width");
__device__ __forceinline__ void m_terms_prefetch(const Q& q, int N, int i, const float* __restrict__ ts) {
  if (q.s < ZB_MT_STATE_DIM) q.carry()[M_CST_TERMS - CARRY0 + q.s] = ts[(size_t)q.s * N + i];
}

// x mod y for x >= 0, y > 0 and x / y < 2^22, exact like fmodf and without its data-dependent loop: the
// quotient from the approximate division is off by at most one, the fused remainder is exact, and two
// selects put it back into [0, y)
__device__ __forceinline__ float fmod_pos(float x, float y) {
  float r = fmaf(-floorf(x / y), y, x);
  r = r < 0.f ? r + y : r;
  return r >= y ? r - y : r;
}

// the term-state entries of the staging row out to the side buffer: one store of the wave (m_ev_store)
__device__ __forceinline__ void m_terms_store(const Q& q, int env0, int N, float* __restrict__ ts) {
  wave_sync();
  const float* S = reinterpret_cast<const float*>(q.b + YG_OFF);
  const int e = q.lane % EPW, f0 = q.lane / EPW;
  const int env = env0 + e;
  if (env < N && f0 < ZB_MT_STATE_DIM) ts[(size_t)f0 * N + env] = S[e * STG_LEN + M_STG_TERMS + f0];
}

struct PreM {
  float delta[ND], jqd_prev[ND], a_raw[ND], action_rate;
};
static_assert(sizeof(PreM) <= 16 * PRE4, "PreM fits PRE4 granules");

// ------------------------------------------------------------- the step kernel: four stamps of zbot_m_step.inc
// Each stamp states all eight parameters; zbot_m_step.inc refuses a missing one and #undefs them at its end.
// zb_m_step_kernel: no events, the model's base inertia, the eleven compiled terms
#define ZB_M_STEP_KERNEL zb_m_step_kernel
#define ZB_M_EVENTS 0
#define ZB_M_EV_PARAMS
#define ZB_M_EV_INIT {}
#define ZB_M_BI 0
#define ZB_M_BI_ROWS static_cast<const float4*>(nullptr)
#define ZB_M_TERMS 0
#define ZB_M_TERMS_INIT {}
#include "zbot_m_step.inc"
// zb_m_events_step_kernel: the events compiled in (include/zbot_manager_events.h)
#define ZB_M_STEP_KERNEL zb_m_events_step_kernel
#define ZB_M_EVENTS 1
#define ZB_M_EV_PARAMS zb_manager_events evc, float* __restrict__ evst,
#define ZB_M_EV_INIT {evc, evst}
#define ZB_M_BI 0
#define ZB_M_BI_ROWS static_cast<const float4*>(nullptr)
#define ZB_M_TERMS 0
#define ZB_M_TERMS_INIT {}
#include "zbot_m_step.inc"
// zb_m_dr_step_kernel: the events build with the per-env base inertia (include/zbot_base_inertia.h)
#define ZB_M_STEP_KERNEL zb_m_dr_step_kernel
#define ZB_M_EVENTS 1
#define ZB_M_EV_PARAMS zb_manager_events evc, float* __restrict__ evst, const float4* __restrict__ bi,
#define ZB_M_EV_INIT {evc, evst}
#define ZB_M_BI 1
#define ZB_M_BI_ROWS bi
#define ZB_M_TERMS 0
#define ZB_M_TERMS_INIT {}
#include "zbot_m_step.inc"
// zb_m_terms_step_kernel: the dr build with the five more reward terms (include/zbot_manager_terms.h)
#define ZB_M_STEP_KERNEL zb_m_terms_step_kernel
#define ZB_M_EVENTS 1
#define ZB_M_EV_PARAMS \
  zb_manager_events evc, float* __restrict__ evst, const float4* __restrict__ bi, const zb_manager_terms* __restrict__ tmc, \
      float* __restrict__ tmst,
#define ZB_M_EV_INIT {evc, evst}
#define ZB_M_BI 1
#define ZB_M_BI_ROWS bi
#define ZB_M_TERMS 1
#define ZB_M_TERMS_INIT {tmc, tmst}
#include "zbot_m_step.inc"

// ------------------------------------------------------------- the terms' kernels: configuration, reset, read-back
// zb_set_manager_terms: the configuration into its device copy, in stream order (no host-side staging)
__global__ void zb_m_terms_cfg_kernel(zb_manager_terms tc, zb_manager_terms* __restrict__ dst) { *dst = tc; }

// explicit resets while the terms are on (zb_reset; beside zb_m_reset_kernel, which does not change): the
// five episode sums into the log accumulator (init: none), then the env's rows zeroed (ContactSensor.reset,
// reset_my_data, RewardManager.reset); one thread per env
__global__ void zb_m_terms_reset_kernel(int N, const int32_t* __restrict__ ids, int n, float* __restrict__ acc, int init,
                                        float* __restrict__ ts) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int i = ids ? ids[t] : t;
  if (i < 0 || i >= N) return;
  if (!init) {
#pragma unroll
    for (int k = 0; k < ZB_MT_NUM_TERMS; ++k)
      atomicAdd(&acc_slot(acc, t)[ZB_M_NUM_REWARD_TERMS + k], ts[(size_t)(ZB_MT_EP_SUMS + k) * N + i]);
  }
#pragma unroll
  for (int f = 0; f < ZB_MT_STATE_DIM; ++f) ts[(size_t)f * N + i] = 0.f;
}

// zb_get_manager_terms_state: the state rows, then the terms' inputs on the current state by the
// out-of-line kinematics (fk / body_vel, as the observation kernels): one thread per env
__global__ void zb_m_terms_get_kernel(const zb_model* __restrict__ mg, int N, const float* __restrict__ st,
                                      const float* __restrict__ ts, zb_manager_terms tc, float* __restrict__ out) {
  MP m = to_mp(mg);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
#pragma unroll
  for (int f = 0; f < ZB_MT_STATE_DIM; ++f) out[(size_t)f * N + i] = ts[(size_t)f * N + i];
  Phys p;
  load_phys(st, N, i, p);
  Kin k;
  fk(m, p, k);
  float V[NB][6];
  body_vel(k, p, V);
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const int l = f == 0 ? 0 : 11, b = link_body(l);
    float c[3], v[3];
    mv3(k.R[b], tc.clearance_point[f], c);
    out[(size_t)(ZB_MT_D_FOOT_Z + f) * N + i] = p.pos[2] + k.p[b][2] + c[2];
    link_com_vel(m, k, V, l, v);
    out[(size_t)(ZB_MT_D_FOOT_VXY + 2 * f) * N + i] = v[0];
    out[(size_t)(ZB_MT_D_FOOT_VXY + 2 * f + 1) * N + i] = v[1];
  }
  float bp[3], bq[4], Rb[9], wc[3];
  link_pose(m, k, m->base_link, bp, bq);
  qmat(bq, Rb);
  out[(size_t)ZB_MT_D_FWD_XY * N + i] = Rb[4];
  out[(size_t)(ZB_MT_D_FWD_XY + 1) * N + i] = -Rb[1];
  constexpr int b = link_body(6);  // (the base link's body: critic_tail)
  cross3(V[b], bp, wc);
#pragma unroll
  for (int a = 0; a < 3; ++a) out[(size_t)(ZB_MT_D_ROOT_VEL + a) * N + i] = V[b][3 + a] + wc[a];
}

// ------------------------------------------------------------- per-env base mass and COM
// include/zbot_base_inertia.h. The side buffer is float4[N][4]: the base composite body's three table
// rows {com, mass}, {Ixx Iyy Izz Ixy}, {Ixz Iyz 0 0} as q.btab holds them, then the base link's COM (body
// frame). One thread per env sums the body again from the authored base link with the env's mass and
// COM offset and the body's other links, in fp64, rounded once.
__device__ __forceinline__ void bi_shift(double m, const double c[3], const double C[3], double I[6]) {
  const double d[3] = {c[0] - C[0], c[1] - C[1], c[2] - C[2]};
  const double dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  I[0] += m * (dd - d[0] * d[0]); I[1] += m * (dd - d[1] * d[1]); I[2] += m * (dd - d[2] * d[2]);
  I[3] -= m * d[0] * d[1]; I[4] -= m * d[0] * d[2]; I[5] -= m * d[1] * d[2];
}
__global__ void zb_base_inertia_kernel(int N, const float* __restrict__ mass_com, int recompute, zb_base_link L,
                                       float4* __restrict__ out, int* __restrict__ flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float* mc = mass_com + (size_t)i * 4;
  const float4 in = make_float4(mc[0], mc[1], mc[2], mc[3]);
  // positive and finite, on the bits (the build's finite-math flags fold a float test away)
  const uint32_t mb = __float_as_uint(in.x);
  bool ok = mb > 0u && mb < 0x7f800000u;
  const float off[3] = {in.y, in.z, in.w};
#pragma unroll
  for (int a = 0; a < 3; ++a) ok = ok && (__float_as_uint(off[a]) & 0x7f800000u) != 0x7f800000u;
  if (!ok) {  // keep the env's rows; zb_base_inertia_check reports it
    *flag = 1;
    return;
  }
  const double m = (double)in.x;
  const double sc = recompute ? m / L.mass : 1.0;
  double c0[3], C[3], I[6];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    c0[a] = L.com[a] + (L.rot[3 * a] * (double)off[0] + L.rot[3 * a + 1] * (double)off[1] + L.rot[3 * a + 2] * (double)off[2]);
  const double M = m + L.rest_mass;
#pragma unroll
  for (int a = 0; a < 3; ++a) C[a] = (m * c0[a] + L.rest_mass * L.rest_com[a]) / M;
#pragma unroll
  for (int a = 0; a < 6; ++a) I[a] = L.inertia[a] * sc + L.rest_inertia[a];
  bi_shift(m, c0, C, I);
  bi_shift(L.rest_mass, L.rest_com, C, I);
  float4* o = out + (size_t)i * 4;
  o[0] = make_float4((float)C[0], (float)C[1], (float)C[2], (float)M);
  o[1] = make_float4((float)I[0], (float)I[1], (float)I[2], (float)I[3]);
  o[2] = make_float4((float)I[4], (float)I[5], 0.f, 0.f);
  o[3] = make_float4((float)c0[0], (float)c0[1], (float)c0[2], 0.f);
}

// the side buffer's floats [r0, r0 + rows) of every env as SoA float[rows][N] (zb_get_base_inertia)
__global__ void zb_base_inertia_rows_kernel(int N, const float4* __restrict__ bi, int r0, int rows, float* __restrict__ dst) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * rows) return;
  const int r = t / N, i = t % N;
  dst[(size_t)r * N + i] = reinterpret_cast<const float*>(bi)[(size_t)i * 16 + r0 + r];
}

// zb_physics_substeps of a handle with the per-env base inertia on: zb_substeps_kernel<true, kTgs> (the
// manager task's: per-link friction, no refresh) with the env's rows staged for fk_team. A kernel of its
// own, so that zb_substeps_kernel keeps its name and code.
template <bool kTgs>
__global__ __launch_bounds__(WGT, ZB_WAVES_PER_SIMD) void zb_bi_substeps_kernel(
    const zb_model* __restrict__ mg, const float4* __restrict__ links, zb_task_cfg cfg, int N, float* __restrict__ st,
    const float* __restrict__ targets, int nsub, float* __restrict__ net_force, float* __restrict__ tau_out,
    const float4* __restrict__ bi) {
  MP m = to_mp(mg);
  __shared__ float4 lds[LDS4 + BI4];
  const int lane = threadIdx.x;
  const int env = xcd_block(blockIdx.x, gridDim.x) * EPW + lane / TL;
  const int i = env < N ? env : N - 1;
  const Q q = make_q(lds, lane, links);
  for (int t = LNK_G + lane; t < LNK4; t += WGT) lds[LNK_OFF + t] = links[t];
  if (q.s < 3) q.bi()[q.s] = bi[(size_t)i * 4 + q.s];
  if (q.s < NL) {
    q.fric(q.s) = st[(size_t)(ZB_M_LINK_MU + q.s) * N + i];
    q.fricd(q.s) = st[(size_t)(ZB_M_LINK_MU_D + q.s) * N + i];
  }
  Phys p;
  load_phys(st, N, i, p);
  float tg[ND], tau[ND], F[1][3];
#pragma unroll
  for (int j = 0; j < ND; ++j) { tg[j] = targets[(size_t)i * ND + j]; tau[j] = 0.f; }
  SensorOut so;
  Stamps sp;
  for (int k = 0; k < nsub; ++k)
    substep<true, true, kTgs, false, true, true>(m, cfg, p, tg, q, k == nsub - 1, k > 0, so, F, tau, sp);
  if (net_force && q.s < NL)
#pragma unroll
    for (int a = 0; a < 3; ++a) net_force[((size_t)i * NL + q.s) * 3 + a] = F[0][a];
  if (tau_out)
#pragma unroll
    for (int j = 0; j < ND; ++j) tau_out[(size_t)i * ND + j] = tau[j];
#define SV(f, v) st[(size_t)(f) * N + i] = (v)
#pragma unroll
  for (int a = 0; a < 3; ++a) { SV(ZB_S_ROOT_POS + a, p.pos[a]); SV(ZB_S_ROOT_LINVEL + a, p.lv[a]); SV(ZB_S_ROOT_ANGVEL + a, p.av[a]); }
#pragma unroll
  for (int a = 0; a < 4; ++a) SV(ZB_S_ROOT_QUAT + a, p.quat[a]);
#pragma unroll
  for (int j = 0; j < ND; ++j) { SV(ZB_S_JOINT_POS + j, p.jq[j]); SV(ZB_S_JOINT_VEL + j, p.jqd[j]); }
#undef SV
}

// ------------------------------------------------------------- curriculum fix-up, reset, observe
// command of a reset env redrawn after lin_vel_cmd_levels widened the ranges (zb_finalize_kernel):
// the post-reset state has zero velocity, so the first metric update reads |command| only
__device__ __forceinline__ void m_fixup_env(const zb_task_cfg& cfg, int N, float* __restrict__ st, float* __restrict__ obs,
                                            const Counters* cnt, uint64_t hs, int i, int keep_yaw) {
  float cmd[3], standing;
  m_resample(cfg, cnt, hs, M_DRAW_RESET_CMD, cmd, standing);
  const float step_dt = cfg.sim_dt * (float)cfg.decimation;
  const float max_steps = cfg.cmd_resample_s / step_dt;
  const float ex = cmd[0] - 0.f, ey = cmd[1] - 0.f;
  st[(size_t)ZB_M_METRICS * N + i] = 0.f + sqrtf(ex * ex + ey * ey) / max_steps;
  // keep_yaw (zb_m_events_step_kernel ran): ang z has no curriculum, so the step kernel's yaw metric
  // and its ang z command (drawn or heading-controlled, zeroed for a standing env) stand as they are
  if (keep_yaw) cmd[2] = st[(size_t)(ZB_M_COMMANDS + 2) * N + i];
  else st[(size_t)(ZB_M_METRICS + 1) * N + i] = 0.f + fabsf(cmd[2] - 0.f) / max_steps;
  st[(size_t)ZB_M_CMD_STANDING * N + i] = standing;
  if (standing > 0.5f) cmd[0] = cmd[1] = cmd[2] = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    st[(size_t)(ZB_M_COMMANDS + a) * N + i] = cmd[a];
    obs[(size_t)i * ZB_M_OBS_DIM + 4 + a] = cmd[a];
  }
}

// explicit resets / construction (init: also the friction default): one thread per env. The
// command is resampled but not yet zeroed for standing envs (that happens in the next
// CommandManager.compute, i.e. the next step).
__global__ void zb_m_reset_kernel(const zb_model* __restrict__ mg, const float4* __restrict__ links, zb_task_cfg cfg,
                                  int N, float* __restrict__ st, const int32_t* __restrict__ ids, int n,
                                  float* __restrict__ acc, const Counters* __restrict__ cnt, uint64_t seed, int init,
                                  zb_manager_events evc, float* __restrict__ ev) {
  MP m = to_mp(mg);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int i = ids ? ids[t] : t;
  if (i < 0 || i >= N) return;
  if (!init) {
#pragma unroll
    for (int k = 0; k < ZB_M_NUM_REWARD_TERMS; ++k) atomicAdd(&acc_slot(acc, t)[k], ST(ZB_M_EP_SUMS + k));
    atomicAdd(&acc_slot(acc, t)[ACC_NRES], 1.f);
    atomicAdd(&acc_slot(acc, t)[ACC_MET0], ST(ZB_M_METRICS));
    atomicAdd(&acc_slot(acc, t)[ACC_MET1], ST(ZB_M_METRICS + 1));
  }
  float pre[2][3];  // the pre-reset feet (the spawn pose at construction)
  if (!cfg.reset_feet_refresh) {
    Phys p0;
    if (init) phys_default(m, p0);
    else load_phys(st, N, i, p0);
    feet_world(m, p0, pre);
  }
  Phys p;
  const uint64_t hs = env_hash(seed, cnt->calls, i);
  (void)reset_pose(m, cfg, hs, p);
  float cmd[3], standing;
  m_resample(cfg, cnt, hs, M_DRAW_RESET_CMD, cmd, standing);
  if (ev) m_reset_events(evc, hs, N, i, ev, cmd[2]);  // (events on: include/zbot_manager_events.h)
#pragma unroll
  for (int a = 0; a < 3; ++a) { ST(ZB_S_ROOT_POS + a) = p.pos[a]; ST(ZB_S_ROOT_LINVEL + a) = p.lv[a]; ST(ZB_S_ROOT_ANGVEL + a) = p.av[a]; }
#pragma unroll
  for (int a = 0; a < 4; ++a) ST(ZB_S_ROOT_QUAT + a) = p.quat[a];
#pragma unroll
  for (int j = 0; j < ND; ++j) { ST(ZB_S_JOINT_POS + j) = p.jq[j]; ST(ZB_S_JOINT_VEL + j) = p.jqd[j]; ST(ZB_M_ACTIONS + j) = 0.f; }
#pragma unroll
  for (int a = 0; a < 3; ++a) ST(ZB_M_COMMANDS + a) = cmd[a];
  ST(ZB_M_CMD_TIME_LEFT) = cfg.cmd_resample_s;
  ST(ZB_M_CMD_STANDING) = standing;
  ST(ZB_M_METRICS) = 0.f;
  ST(ZB_M_METRICS + 1) = 0.f;
  float R[9];
  qmat(p.quat, R);
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const float4 fr = links[DFLT_OFF + 4 + f];
    const float v[3] = {fr.x, fr.y, fr.z};
    float w3[3];
    mv3(R, v, w3);
#pragma unroll
    for (int a = 0; a < 3; ++a) ST(ZB_M_FEET_DOWN_POS + 3 * f + a) = cfg.reset_feet_refresh ? p.pos[a] + w3[a] : pre[f][a];
    ST(ZB_M_FEET_STEP_LEN + f) = 0.f;
    ST(ZB_M_FEET_F_LAST + f) = 0.f;
    ST(ZB_M_FEET_AIR_CUR + f) = 0.f;
    ST(ZB_M_FEET_AIR_LAST + f) = 0.f;
#pragma unroll
    for (int h = 0; h < 3; ++h) { ST(ZB_M_FEET_FZ_HIST + 2 * h + f) = 0.f; ST(ZB_M_FEET_FN_HIST + 2 * h + f) = 0.f; }
  }
  ST(ZB_M_EP_LEN) = 0.f;
#pragma unroll
  for (int k = 0; k < ZB_M_NUM_REWARD_TERMS; ++k) ST(ZB_M_EP_SUMS + k) = 0.f;
  if (init) {
#pragma unroll
    for (int l = 0; l < NL; ++l) { ST(ZB_M_LINK_MU + l) = cfg.friction; ST(ZB_M_LINK_MU_D + l) = cfg.friction_dynamic; }
  }
#undef ST
#undef CST
#undef OUT
}

// the observation of the current state (reset(): ObservationManager.compute after _reset_idx);
// noise from this call's stream
// m_write_obs of env i's current state into the row o (noise stream h; none when cfg.obs_corruption is 0)
__device__ __forceinline__ void m_observe_row(MP m, const zb_task_cfg& cfg, uint64_t h, const Phys& p,
                                              const float* __restrict__ st, int N, int i, float* o) {
  Kin k;
  fk(m, p, k);
  float bp[3], bq[4];
  link_pose(m, k, m->base_link, bp, bq);
  const float cmd[3] = {st[(size_t)ZB_M_COMMANDS * N + i], st[(size_t)(ZB_M_COMMANDS + 1) * N + i],
                        st[(size_t)(ZB_M_COMMANDS + 2) * N + i]};
  float a_obs[ND];
#pragma unroll
  for (int a = 0; a < ND; ++a) a_obs[a] = st[(size_t)(ZB_M_ACTIONS + a) * N + i];
  m_write_obs(m, cfg, h, bq, cmd, p, a_obs, o);
}

__global__ void zb_m_observe_kernel(const zb_model* __restrict__ mg, zb_task_cfg cfg, int N, const float* __restrict__ st,
                                    float* __restrict__ obs, const Counters* __restrict__ cnt, uint64_t seed) {
  MP m = to_mp(mg);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  Phys p;
  load_phys(st, N, i, p);
  m_observe_row(m, cfg, env_hash(seed, cnt->calls, i), p, st, N, i, obs + (size_t)i * ZB_M_OBS_DIM);
}

// zb_set_manager_events: the event state of every env as a reset at the current stream position draws
// it, and the drawn ang z into the command row (a standing env is zeroed by its next step, as after a reset)
__global__ void zb_m_events_init_kernel(int N, float* __restrict__ st, const Counters* __restrict__ cnt, uint64_t seed,
                                        zb_manager_events evc, float* __restrict__ ev) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float ang_z;
  m_reset_events(evc, env_hash(seed, cnt->calls, i), N, i, ev, ang_z);
  st[(size_t)(ZB_M_COMMANDS + 2) * N + i] = ang_z;
}
