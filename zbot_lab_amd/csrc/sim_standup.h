// zbot-6b-standup-v0: stage weights, the in-kernel random draws (env_hash, draw; the later tasks use them too),
// the lying reset pose, the step, reset, observe and per-link friction kernels. Included by zbot_sim.hip inside
// its anonymous namespace at the text's old place; needs everything above the #include (ST / CST / OUT defined
// with the step-kernel scaffolding).

// =========================================================================== stand-up task
// zbot-6b-standup-v0 (reference zbot_direct_6_standup_env_v0.py = standup.py) on the same robot
// and physics: ZBOT_6S_CFG_2 lying init (zbot_cfg.py:721-763), per-link friction from the
// startup material randomisation, rewards from the post-step link states, died on a height drop,
// reset pose randomised in-kernel (reset_root_state_uniform) and a device-side curriculum.

__host__ __device__ __forceinline__ float u01(uint64_t h) { return (float)(h >> 40) * (1.0f / 16777216.0f); }

// reward weight of term t in curriculum stage `stage` (compile-time indices into the kernarg table)
__device__ __forceinline__ float stage_weight(const zb_task_cfg& cfg, int stage, int t) {
  float w = cfg.stage_scales[0][t];
#pragma unroll
  for (int sg = 1; sg < ZB_MAX_STAGES; ++sg) w = stage == sg ? cfg.stage_scales[sg][t] : w;
  return w;
}

// counter-based random stream of env i at call ctr; draw k of it (shared with the oracle)
__device__ __forceinline__ uint64_t env_hash(uint64_t seed, uint64_t ctr, int i) {
  return hash64(seed ^ hash64(ctr * 0x100000001B3ull + (uint64_t)i));
}
__device__ __forceinline__ float draw(uint64_t h, int k) { return u01(hash64(h + 0x632BE59BD9B4E019ull * (uint64_t)k)); }

// reset_root_state_uniform (standup.py:33-97, v4.py:59-105) from stream h (draws 1..4): x, y,
// roll, yaw ~ U (the cfg ranges; pitch / z / velocities 0), root = default + (x, y, 0), quat =
// quat_from_euler_xyz(roll, 0, yaw) applied in the world frame (delta * default, standup) or the
// body frame (default * delta, v4), normalised; joints default, every velocity zero. Returns the
// yaw sample (the events store it as env.current_yaw).
__device__ __forceinline__ float reset_pose(MP m, const zb_task_cfg& cfg, uint64_t h, Phys& p) {
  float r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    r[k] = draw(h, k + 1) * (cfg.reset_pose_range[k][1] - cfg.reset_pose_range[k][0]) + cfg.reset_pose_range[k][0];
  float sr, cr, sy, cy;
  sincos_r(0.5f * r[2], &sr, &cr);
  sincos_r(0.5f * r[3], &sy, &cy);
  const float dq[4] = {cy * cr, cy * sr, sy * sr, sy * cr};  // quat_from_euler_xyz(roll, 0, yaw)
  // the sampled pose is the Isaac Lab root's (the chain root unless the asset is rooted elsewhere):
  // its default pose is chain-root default * T (T = api_root_in_root, identity for the others)
  const float q0[4] = {m->default_root_quat[0], m->default_root_quat[1], m->default_root_quat[2],
                       m->default_root_quat[3]};
  const float tT[3] = {m->api_root_in_root[0], m->api_root_in_root[1], m->api_root_in_root[2]};
  const float qT[4] = {m->api_root_in_root[3], m->api_root_in_root[4], m->api_root_in_root[5], m->api_root_in_root[6]};
  float qa0[4], ta[3];
  qmul(q0, qT, qa0);
  qrot(q0, tT, ta);
  float qa[4];
  if (cfg.reset_pose_body_frame) qmul(qa0, dq, qa);
  else qmul(dq, qa0, qa);
  qnormalize(qa);
  const float pa[3] = {m->default_root_pos[0] + ta[0] + r[0], m->default_root_pos[1] + ta[1] + r[1],
                       m->default_root_pos[2] + ta[2]};
  // back to the chain root: q = qa * conj(qT), p = pa - R(q) tT
  const float qTc[4] = {qT[0], -qT[1], -qT[2], -qT[3]};
  float qn[4], tq[3];
  qmul(qa, qTc, qn);
  qrot(qn, tT, tq);
#pragma unroll
  for (int a = 0; a < 4; ++a) p.quat[a] = qn[a];
  p.pos[0] = pa[0] - tq[0];
  p.pos[1] = pa[1] - tq[1];
  p.pos[2] = pa[2] - tq[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) { p.lv[a] = 0.f; p.av[a] = 0.f; }
#pragma unroll
  for (int j = 0; j < ND; ++j) { p.jq[j] = m->default_joint_pos[j]; p.jqd[j] = 0.f; }
  return r[3];
}

__device__ __forceinline__ void su_reset_pose(MP m, const zb_task_cfg& cfg, uint64_t seed, uint64_t ctr, int i,
                                              Phys& p) {
  (void)reset_pose(m, cfg, env_hash(seed, ctr, i), p);
}

// One stand-up policy step per team (same mapping as zb_step_kernel; no contact sensor).
template <bool kTgs, int kOcc, bool kRefresh = false, bool kRf = false>
__global__ __launch_bounds__(WGT, kOcc) void zb_su_step_kernel(
    const zb_model* __restrict__ mg, const float4* __restrict__ links, zb_task_cfg cfg, int N, float* __restrict__ st,
    const float* __restrict__ act, float* __restrict__ obs, float* __restrict__ rew, uint8_t* __restrict__ term,
    uint8_t* __restrict__ trunc, int64_t* __restrict__ done, float* __restrict__ acc,
    const Counters* __restrict__ cnt, uint64_t seed, float* __restrict__ wc) {
  MP m = to_mp(mg);
  __shared__ float4 lds[LDS4];
  if (kOcc == 1) asm volatile("" ::: "a255");  // (zb_step_kernel: kOcc)
  const int lane = threadIdx.x;
  const int env = xcd_block(blockIdx.x, gridDim.x) * EPW + lane / TL;
  const int i = env < N ? env : N - 1;
  const bool lead = env < N && lane % TL == 0;
  const Q q = make_q(lds, lane, links);
  for (int t = LNK_G + lane; t < LNK4; t += WGT) lds[LNK_OFF + t] = links[t];
  Stamps sp;
  sp.begin();
  Phys p;
#pragma unroll
  for (int a = 0; a < 3; ++a) { p.pos[a] = ST(ZB_S_ROOT_POS + a); p.lv[a] = ST(ZB_S_ROOT_LINVEL + a); p.av[a] = ST(ZB_S_ROOT_ANGVEL + a); }
#pragma unroll
  for (int a = 0; a < 4; ++a) p.quat[a] = ST(ZB_S_ROOT_QUAT + a);
#pragma unroll
  for (int j = 0; j < ND; ++j) { p.jq[j] = ST(ZB_S_JOINT_POS + j); p.jqd[j] = ST(ZB_S_JOINT_VEL + j); }
  if (q.s < NL) {  // lane l: link l (visible after the first barrier)
    q.fric(q.s) = ST(ZB_SU_LINK_MU + q.s);
    q.fricd(q.s) = ST(ZB_SU_LINK_MU_D + q.s);
  }

  // _pre_physics_step (standup.py:538-551, mode 1)
  const bool writer = q.s == 0;
  const float step_dt = cfg.sim_dt * (float)cfg.decimation;
  float target[ND];
  {
    Pre pr;
    pre_action<ZB_SU_P_DELTA, ZB_SU_ACTIONS, false>(m, cfg, st, N, i, act, q.s, step_dt, pr, target);
    if (writer) q.pre() = pr;
  }

  SensorOut so;
  wc_load(q, wc, N, i);  // the first substep's GJK warm start
  sp.mark(0);
  for (int k = 0; k < cfg.decimation; ++k) {
    substep<false, true, kTgs, kRefresh, kRf>(m, cfg, p, target, q, false, true, so, nullptr, nullptr, sp);
    sp.mark(7);
  }
  Pre pr;
  const float wc_row = after_substeps(m, q, st, pr);
  const float czl0 = ST(ZB_SU_CENTER_Z_LAST);
  const float ep_len = ST(ZB_SU_EP_LEN) + 1.f;
  float sums0[ZB_SU_NUM_REWARD_TERMS];
#pragma unroll
  for (int t = 0; t < ZB_SU_NUM_REWARD_TERMS; ++t) sums0[t] = ST(ZB_SU_EP_SUMS + t);
  const int stage = cnt->stage;

  // post-step link states (_compute_intermediate_values 571-591, body_link_state_w)
  float z4, z6, z8, vz5, vz6, fz[2][3], obs_q[4];
  {
    wave_sync();
    fk_team_pose(p, q);
    wave_sync();
    float S[ND][6], org[ND][3];
    read_joints(q, S, org);
    float lp[3], lq[4], v[3], R[9];
    link_pose_q(m, q, 4, lp, lq);
    z4 = lp[2] + p.pos[2];
    link_pose_q(m, q, 8, lp, lq);
    z8 = lp[2] + p.pos[2];
    link_pose_q(m, q, 6, lp, obs_q);
    z6 = lp[2] + p.pos[2];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      link_pose_q(m, q, f == 0 ? 0 : 11, lp, lq);
      qmat(lq, R);
      const float sg = f == 0 ? 1.f : -1.f;  // axis_z_feet = (0,0,1), (0,0,-1) (standup.py:503-505)
      fz[f][0] = sg * R[2]; fz[f][1] = sg * R[5]; fz[f][2] = sg * R[8];
    }
    link_origin_vel_q(m, q, p, S, 6, v);
    vz6 = v[2];
    link_origin_vel_q(m, q, p, S, 5, v);
    vz5 = v[2];
  }

  // _get_dones (standup.py:634-643)
  const bool time_out = ep_len >= (float)(cfg.max_episode_length - 1);
  const bool blowup = phys_bad(p);  // non-finite guard (phys_bad)
  const bool died = (czl0 - z6) > cfg.center_z_drop || blowup;
  const float czl = ((int)ep_len % cfg.center_z_period == cfg.center_z_period - 1) ? z6 : czl0;

  // _get_rewards (standup.py:620-632): reward_func() * scale * step_dt per term, dict order
  float r[ZB_SU_NUM_REWARD_TERMS];
  {
    const float rh = z6 + 0.5f * z4 + 0.5f * z8 - 0.1f;  // _reward_upward_2 (843-856)
    float up = z6 < 0.22f ? rh + 0.5f * vz6 + 0.5f * vz5 : 1.35f;
    if ((fz[0][2] < 0.5f || fz[1][2] < 0.5f) && z6 > 0.1f) up = -5.f * up;
    r[ZB_SU_R_UPWARD_2] = up;
  }
  r[ZB_SU_R_SHAPE_SYMMETRY] = fabsf(pr.pdel[0] + pr.pdel[5]) + fabsf(pr.pdel[1] + pr.pdel[4]) +
                              fabsf(pr.pdel[2] + pr.pdel[3]);  // 782-789
  {
    float sd = 0.f;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float d[3] = {fz[f][0], fz[f][1], fz[f][2] - 1.f};
      sd += sqrtf(dot3(d, d));
    }
    r[ZB_SU_R_FEET_DOWNWARD] = sd;  // 735-745
  }
  r[ZB_SU_R_FEET_DOWNWARD_4] = z6 < 0.15f ? fz[0][2] + fz[1][2] : 1.6f;  // 827-840
  float w[ZB_SU_NUM_REWARD_TERMS];
#pragma unroll
  for (int t = 0; t < ZB_SU_NUM_REWARD_TERMS; ++t) w[t] = stage_weight(cfg, stage, t);
  float reward = 0.f, sums[ZB_SU_NUM_REWARD_TERMS];
#pragma unroll
  for (int t = 0; t < ZB_SU_NUM_REWARD_TERMS; ++t) {
    const float v = (r[t] * w[t]) * step_dt;
    reward += v;
    sums[t] = sums0[t] + v;
  }
  if (died) reward -= cfg.terminal_penalty;  // 629-630
  if (blowup) {
    reward = -cfg.terminal_penalty;
#pragma unroll
    for (int t = 0; t < ZB_SU_NUM_REWARD_TERMS; ++t) sums[t] = sums0[t];
  }
  const bool reset = died || time_out;

  // _reset_idx (645-703): episode log (sums per second of the env's own episode), new random
  // root pose, default joints; the reset env's observation sees the new pose
  const uint64_t lmask = __ballot(reset && lead);
  if (reset) {
    if (lead) {
      const float dur = fmaxf(ep_len * step_dt, step_dt);
      float* lr = log_row(q);
#pragma unroll
      for (int t = 0; t < ZB_SU_NUM_REWARD_TERMS; ++t) lr[t] = sums[t] / dur;
      lr[ACC_NRES] = 1.f;
      lr[ACC_DIED] = died ? 1.f : 0.f;
      lr[ACC_TOUT] = time_out ? 1.f : 0.f;
    }
    su_reset_pose(m, cfg, seed, cnt->calls, i, p);
    const float4 qr = q.dflt()[3];
    const float qrel[4] = {qr.x, qr.y, qr.z, qr.w};
    qmul(p.quat, qrel, obs_q);
  }
  log_flush(q, lmask, acc);
  store_wc_row(q, wc, N, i, reset, wc_row);
  sp.mark(12);
  if (writer) {
    const Live live{reset};
    stage_phys(q, p);
#pragma unroll
    for (int j = 0; j < ND; ++j) { OUT(ZB_SU_P_DELTA + j) = live(pr.pdel[j]); OUT(ZB_SU_ACTIONS + j) = live(pr.a_now[j]); }
    OUT(ZB_SU_CENTER_Z_LAST) = reset ? cfg.center_z_init : czl;
    OUT(ZB_SU_EP_LEN) = live(ep_len);
#pragma unroll
    for (int t = 0; t < ZB_SU_NUM_REWARD_TERMS; ++t) OUT(ZB_SU_EP_SUMS + t) = live(sums[t]);

    // _get_observations (593-618): base quat, joint_pos - default, joint_vel, actions
    float* o = &q.stg(ZB_SU_LINK_MU);
    o[0] = obs_q[0]; o[1] = obs_q[1]; o[2] = obs_q[2]; o[3] = obs_q[3];
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      o[4 + j] = p.jq[j] - m->default_joint_pos[j];
      o[10 + j] = p.jqd[j];
      o[16 + j] = live(pr.a_now[j]);
    }
    stage_result<ZB_SU_LINK_MU, ZB_SU_OBS_DIM>(q, reward, died, time_out);
  }
  step_finish<ZB_SU_LINK_MU, ZB_SU_OBS_DIM>(q, N, st, obs, rew, term, trunc, done, sp);
}

// explicit resets (env_ids, or all when ids == nullptr): episode log into acc, then the reset
// pose of su_reset_pose; one thread per env
__global__ void zb_su_reset_kernel(const zb_model* __restrict__ mg, zb_task_cfg cfg, int N, float* __restrict__ st,
                                   const int32_t* __restrict__ ids, int n, float* __restrict__ acc,
                                   const Counters* __restrict__ cnt, uint64_t seed) {
  MP m = to_mp(mg);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int i = ids ? ids[t] : t;
  if (i < 0 || i >= N) return;
  const float step_dt = cfg.sim_dt * (float)cfg.decimation;
  const float dur = fmaxf(ST(ZB_SU_EP_LEN) * step_dt, step_dt);
#pragma unroll
  for (int k = 0; k < ZB_SU_NUM_REWARD_TERMS; ++k) atomicAdd(&acc_slot(acc, t)[k], ST(ZB_SU_EP_SUMS + k) / dur);
  atomicAdd(&acc_slot(acc, t)[ACC_NRES], 1.f);
  Phys p;
  su_reset_pose(m, cfg, seed, cnt->calls, i, p);
#pragma unroll
  for (int a = 0; a < 3; ++a) { ST(ZB_S_ROOT_POS + a) = p.pos[a]; ST(ZB_S_ROOT_LINVEL + a) = p.lv[a]; ST(ZB_S_ROOT_ANGVEL + a) = p.av[a]; }
#pragma unroll
  for (int a = 0; a < 4; ++a) ST(ZB_S_ROOT_QUAT + a) = p.quat[a];
#pragma unroll
  for (int j = 0; j < ND; ++j) {
    ST(ZB_S_JOINT_POS + j) = p.jq[j]; ST(ZB_S_JOINT_VEL + j) = p.jqd[j];
    ST(ZB_SU_P_DELTA + j) = 0.f; ST(ZB_SU_ACTIONS + j) = 0.f;
  }
  ST(ZB_SU_CENTER_Z_LAST) = cfg.center_z_init;
  ST(ZB_SU_EP_LEN) = 0.f;
#pragma unroll
  for (int k = 0; k < ZB_SU_NUM_REWARD_TERMS; ++k) ST(ZB_SU_EP_SUMS + k) = 0.f;
}

// the observation of env i's current state (standup.py:593-618) into the row o (out of line: obs_row)
__device__ __noinline__ void su_obs_row(const zb_model* mg, int N, const float* st, int i, float* o) {
  MP m = to_mp(mg);
  Phys p;
  load_phys(st, N, i, p);
  Kin k;
  fk(m, p, k);
  float bp[3], bq[4];
  link_pose(m, k, 6, bp, bq);
  o[0] = bq[0]; o[1] = bq[1]; o[2] = bq[2]; o[3] = bq[3];
#pragma unroll
  for (int j = 0; j < ND; ++j) {
    o[4 + j] = p.jq[j] - m->default_joint_pos[j];
    o[10 + j] = p.jqd[j];
    o[16 + j] = st[(size_t)(ZB_SU_ACTIONS + j) * N + i];
  }
}

__global__ void zb_su_observe_kernel(const zb_model* __restrict__ mg, int N, const float* __restrict__ st,
                                     float* __restrict__ obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  su_obs_row(mg, N, st, i, obs + (size_t)i * ZB_SU_OBS_DIM);
}

// per-link friction [N][NL] -> state rows ZB_SU_LINK_MU (mu == nullptr: fill with `fill`)
__global__ void zb_su_friction_kernel(int N, float* __restrict__ st, const float* __restrict__ mu, float fill, int row) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * NL) return;
  const int i = t / NL, l = t % NL;
  st[(size_t)(row + l) * N + i] = mu ? mu[t] : fill;
}
