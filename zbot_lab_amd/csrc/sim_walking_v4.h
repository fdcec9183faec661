// zbot-6b-walking-v4: command resampling, PreV4, the step, reset and observe kernels. Included by zbot_sim.hip
// inside its anonymous namespace at the text's old place; needs everything above the #include (the draws of
// sim_standup.h, ST / CST / OUT defined with the step-kernel scaffolding).

// =========================================================================== walking v4
// zbot-6b-walking-v4 (reference zbot_direct_6dof_bipedal_env_v4.py = v4.py): v2's robot and
// physics with forward-velocity / heading commands (reset and interval resample events), a
// history-3 contact sensor that also tracks contact time, 15 reward terms evaluated on the
// post-step state, and the two curricula (stage weights + command ranges in the device counters).

__device__ __forceinline__ float wrap_to_pi(float x) {  // isaaclab.utils.math.wrap_to_pi
  float a = fmodf(x, TWO_PI_F);
  if (a < 0.f) a += TWO_PI_F;
  return a > PI_F ? a - TWO_PI_F : a;
}

// resample_commands (v4.py:107-135) from stream h, draws k0 .. k0+2, with the device-side params
__device__ __forceinline__ void v4_resample(const zb_task_cfg& cfg, const Counters* cnt, uint64_t h, int k0,
                                            float cur_yaw, float cmd[2], float& target) {
  const float lo = cnt->vel[0], hi0 = cnt->vel[1];
  if (cfg.cmd_dual_sign) {
    const float sg = draw(h, k0) < cnt->prob_pos ? 1.f : -1.f;  // bernoulli(prob_pos) * 2 - 1
    const float hi = hi0 + cfg.cmd_offset * (sg - 1.f);
    cmd[0] = (draw(h, k0 + 1) * (hi - lo) + lo) * sg;
  } else {
    cmd[0] = draw(h, k0 + 1) * (hi0 - lo) + lo;
  }
  cmd[1] = draw(h, k0 + 2) * (cnt->yaw[1] - cnt->yaw[0]) + cnt->yaw[0];
  target = wrap_to_pi(cur_yaw + cmd[1]);
}

// prologue values parked in LDS across the physics (overlays the Pre record)
struct PreV4 {
  float a_now[ND], pdel[ND], jqd_prev[ND], action_rate;
};
static_assert(sizeof(PreV4) <= 16 * PRE4, "PreV4 fits PRE4 granules");

template <bool kTgs, int kOcc>
__global__ __launch_bounds__(WGT, kOcc) void zb_v4_step_kernel(
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
  const float* cst = carry_prefetch<ZB_V4_STATE_DIM>(q, st, N, i);

  // _pre_physics_step (v4.py:776-804, mode 1)
  const bool writer = q.s == 0;
  const float step_dt = cfg.sim_dt * (float)cfg.decimation;
  PreV4& pv = *reinterpret_cast<PreV4*>(&q.pre());
  float target[ND];
  {
    PreV4 pr;
    pr.action_rate = 0.f;
    float a_tanh[ND];
    actions_tanh(act, i, q.s, a_tanh);
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      const float a_prev = ST(ZB_V4_ACTIONS + j);
      pr.a_now[j] = a_tanh[j];
      pr.pdel[j] = clampf(ST(ZB_V4_P_DELTA + j) + PI_F * pr.a_now[j] * cfg.joint_speed_limit * step_dt, -PI_F, PI_F);
      target[j] = pr.pdel[j] + m->default_joint_pos[j];
      pr.action_rate += (pr.a_now[j] - a_prev) * (pr.a_now[j] - a_prev);
      pr.jqd_prev[j] = 0.f;
    }
    if (writer) pv = pr;
  }

  // 4 substeps, each followed by the contact sensor's update (record parked in LDS); the last one's
  // applied torques feed the torques term, the joint velocities before it give Isaac Lab's
  // finite-difference joint_acc (ArticulationData.update every substep)
  SensorOut so;
  wc_load(q, wc, N, i);  // the first substep's GJK warm start
  sp.mark(0);
  for (int k = 0; k < cfg.decimation; ++k) {
    const bool last = k == cfg.decimation - 1;
    if (last && writer) {
#pragma unroll
      for (int j = 0; j < ND; ++j) pv.jqd_prev[j] = p.jqd[j];
    }
    substep<false, false, kTgs>(m, cfg, p, target, q, true, true, so, nullptr, nullptr, sp);
    sens_record(q, k, so);
    sp.mark(7);
  }
  PreV4 pr;
  const float wc_row = after_substeps(m, q, st, pr);

  // ContactSensor (history 3, updated every physics step; air / contact timers incl.
  // last_contact_time)
  float fz_sum[2], fm_max;
  float air_cur[2], con_cur[2], air_last[2], con_last[2], feetF[2];
  bool in_contact[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    air_cur[f] = CST(ZB_V4_FEET_AIR_CUR + f);
    con_cur[f] = CST(ZB_V4_FEET_CONTACT_CUR + f);
    air_last[f] = CST(ZB_V4_FEET_AIR_LAST + f);
    con_last[f] = CST(ZB_V4_FEET_CONTACT_LAST + f);
  }
  sens_replay<ZB_V4_HIST>(q, cst, 1, 0, ZB_V4_FEET_FZ_HIST, ZB_V4_UNDES_FMAX_HIST, cfg.decimation, cfg.sim_dt,
                          cfg.contact_force_threshold, fz_sum, fm_max, air_cur, air_last, con_cur, con_last);
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    in_contact[f] = con_cur[f] > 0.f;
    feetF[f] = fz_sum[f] / (float)ZB_V4_HIST;  // mean over the history (v4.py:846-849)
  }
  const float ep_len = CST(ZB_V4_EP_LEN) + 1.f;
  float cmd[2] = {CST(ZB_V4_COMMANDS), CST(ZB_V4_COMMANDS + 1)};
  float tgt = CST(ZB_V4_TARGET_YAW);
  float ileft = CST(ZB_V4_INTERVAL_LEFT);
  float f_last[2] = {CST(ZB_V4_FEET_F_LAST), CST(ZB_V4_FEET_F_LAST + 1)};
  float step_len[2] = {CST(ZB_V4_FEET_STEP_LEN), CST(ZB_V4_FEET_STEP_LEN + 1)};
  float down[2][3];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int a = 0; a < 3; ++a) down[f][a] = CST(ZB_V4_FEET_DOWN_POS + 3 * f + a);
  float sums0[ZB_V4_NUM_REWARD_TERMS];
#pragma unroll
  for (int t = 0; t < ZB_V4_NUM_REWARD_TERMS; ++t) sums0[t] = CST(ZB_V4_EP_SUMS + t);
  const int stage = cnt->stage;

  // _compute_intermediate_values (v4.py:809-849) on the post-step state
  float bq[4], sh[3], fwd[3], vb[3], feet[2][3], fzax[2][3], fxax[2][3], fvel[2][3];
  bool died;
  {
    wave_sync();
    fk_team_pose(p, q);
    wave_sync();
    float S[ND][6], org[ND][3];
    read_joints(q, S, org);
    float bp[3], R[9], fq[4];
    link_pose_q(m, q, 6, bp, bq);
    qmat(bq, R);
    sh[0] = R[2]; sh[1] = R[5]; sh[2] = R[8];            // quat_apply(base_quat, z)
    fwd[0] = sh[1]; fwd[1] = -sh[0]; fwd[2] = 0.f;       // GRAVITY_VEC_W x shoulder
    link_origin_vel_q(m, q, p, S, 6, vb);                // body_link_lin_vel_w[base]
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int l = f == 0 ? 0 : 11;
      link_pose_q(m, q, l, feet[f], fq);
#pragma unroll
      for (int a = 0; a < 3; ++a) feet[f][a] += p.pos[a];
      qmat(fq, R);
      const float sg = f == 0 ? 1.f : -1.f;
      fzax[f][0] = sg * R[2]; fzax[f][1] = sg * R[5]; fzax[f][2] = sg * R[8];
      fxax[f][0] = R[0]; fxax[f][1] = R[3]; fxax[f][2] = R[6];
      link_com_vel_q(m, q, p, S, l, fvel[f]);            // body_com_lin_vel_w[feet]
    }
    const float base_z = bp[2] + p.pos[2];
    // _get_dones (v4.py:896-918)
    const float fm = fm_max;
    died = fm > cfg.undesired_force_threshold || base_z < cfg.termination_height;
  }
  const bool time_out = ep_len >= (float)(cfg.max_episode_length - 1);
  const bool blowup = phys_bad(p);  // non-finite guard (phys_bad), as in the walking kernel
  died |= blowup;
  float cur_yaw = atan2f(fwd[1], fwd[0]);
  float he;
  {
    float sn, cs;
    sincos_r(tgt - cur_yaw, &sn, &cs);
    he = atan2f(sn, cs);
  }
  const float vfwd = dot3(vb, fwd);

  // _get_rewards (v4.py:883-894), terms 1003-1171 in dict order
  float r[ZB_V4_NUM_REWARD_TERMS];
  {
    const float e = cmd[0] - vfwd;
    r[ZB_V4_R_TRACK_LIN_VEL_X] = __expf(-e * e / 0.25f);
    r[ZB_V4_R_TRACK_HEADING_YAW] = __expf(-he * he / 0.25f);
    const float vy = dot3(vb, sh);
    r[ZB_V4_R_LIN_VEL_Y] = vy * vy;
    r[ZB_V4_R_ACTION_RATE] = pr.action_rate;
    r[ZB_V4_R_TORQUES] = so.tau2;
    float jv = 0.f, ja = 0.f;
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      jv += p.jqd[j] * p.jqd[j];
      const float aj = (p.jqd[j] - pr.jqd_prev[j]) / cfg.sim_dt;
      ja += aj * aj;
    }
    r[ZB_V4_R_JOINT_VEL] = jv;
    r[ZB_V4_R_JOINT_ACC] = ja;
    float sd = 0.f, sfw = 0.f;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float dz[3] = {fzax[f][0], fzax[f][1], fzax[f][2] - 1.f};
      sd += sqrtf(dot3(dz, dz));
      const float dx[3] = {fxax[f][0] - fwd[0], fxax[f][1] - fwd[1], fxax[f][2] - fwd[2]};
      sfw += sqrtf(dot3(dx, dx));
    }
    r[ZB_V4_R_FEET_DOWNWARD] = sd;
    r[ZB_V4_R_FEET_FORWARD] = sfw;
    // step_length (v4.py:1058-1095): touchdown foot records its step along the heading, signed by
    // the commanded direction; the stored lengths decay by 0.99 per step
    const float csg = cmd[0] > 0.f ? 1.f : (cmd[0] < 0.f ? -1.f : 0.f);
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      if (feetF[f] > 10.f && f_last[f] < 10.f) {
        const float dv[3] = {feet[f][0] - down[f][0], feet[f][1] - down[f][1], feet[f][2] - down[f][2]};
        step_len[f] = dot3(dv, fwd) * csg;
#pragma unroll
        for (int a = 0; a < 3; ++a) down[f][a] = feet[f][a];
      }
    }
    const float mn = fminf(step_len[0], step_len[1]);
    step_len[0] *= 0.99f;
    step_len[1] *= 0.99f;
    f_last[0] = feetF[0];
    f_last[1] = feetF[1];
    r[ZB_V4_R_STEP_LENGTH] = tanh_r(15.f * mn);
    // feet_air_time_biped (1129-1143)
    const bool single = (in_contact[0] ? 1 : 0) + (in_contact[1] ? 1 : 0) == 1;
    float bi = 3.4e38f;
#pragma unroll
    for (int f = 0; f < 2; ++f) bi = fminf(bi, single ? (in_contact[f] ? con_cur[f] : air_cur[f]) : 0.f);
    r[ZB_V4_R_FEET_AIR_TIME_BIPED] = fminf(bi, 2.f);
    // airtime_variance (1097-1103): unbiased variance of two values = (a - b)^2 / 2
    const float da = fminf(air_last[0], 0.5f) - fminf(air_last[1], 0.5f);
    const float dc = fminf(con_last[0], 0.5f) - fminf(con_last[1], 0.5f);
    r[ZB_V4_R_AIRTIME_VARIANCE] = 0.5f * da * da + 0.5f * dc * dc;
    float sl = 0.f;
#pragma unroll
    for (int f = 0; f < 2; ++f)
      sl += sqrtf(fvel[f][0] * fvel[f][0] + fvel[f][1] * fvel[f][1]) * (feetF[f] > 1.f ? 1.f : 0.f);
    r[ZB_V4_R_FEET_SLIDE] = sl;
    r[ZB_V4_R_FEET_HARMONY] = (air_last[0] + air_last[1]) - 3.f * fabsf(air_last[0] - air_last[1]);
    const float dx = feet[0][0] - feet[1][0], dy = feet[0][1] - feet[1][1];
    r[ZB_V4_R_FEET_CLOSE] = fmaxf(0.115f - sqrtf(dx * dx + dy * dy), 0.f);
  }
  float reward = 0.f, sums[ZB_V4_NUM_REWARD_TERMS];
#pragma unroll
  for (int t = 0; t < ZB_V4_NUM_REWARD_TERMS; ++t) {
    const float v = (r[t] * stage_weight(cfg, stage, t)) * step_dt;
    reward += v;
    sums[t] = sums0[t] + v;
  }
  if (died) reward -= cfg.terminal_penalty;  // v4.py:892-893
  if (blowup) {  // finite reward, the episode sums without this step
    reward = -cfg.terminal_penalty;
#pragma unroll
    for (int t = 0; t < ZB_V4_NUM_REWARD_TERMS; ++t) sums[t] = sums0[t];
  }
  const bool reset = died || time_out;
  const uint64_t hs = env_hash(seed, cnt->calls, i);
  float obs_q[4] = {bq[0], bq[1], bq[2], bq[3]};

  // _reset_idx (v4.py:920-1001): log (sum / own duration), reset events (pose, commands), defaults
  const uint64_t lmask = __ballot(reset && lead);
  if (reset) {
    if (lead) {
      const float dur = fmaxf(ep_len * step_dt, step_dt);
      float* lr = log_row(q);
#pragma unroll
      for (int t = 0; t < ZB_V4_NUM_REWARD_TERMS; ++t) lr[t] = sums[t] / dur;
      lr[ACC_NRES] = 1.f;
      lr[ACC_DIED] = died ? 1.f : 0.f;
      lr[ACC_TOUT] = time_out ? 1.f : 0.f;
    }
    cur_yaw = reset_pose(m, cfg, hs, p);
    v4_resample(cfg, cnt, hs, 5, cur_yaw, cmd, tgt);
    const float4 qr = q.dflt()[3];
    const float qrel[4] = {qr.x, qr.y, qr.z, qr.w};
    qmul(p.quat, qrel, obs_q);
    float R[9];
    qmat(p.quat, R);
#pragma unroll
    for (int f = 0; f < 2; ++f) {  // feet_down_pos_last: pre-reset feet (v4.py:996) or reset pose's
      const float4 fr = q.dflt()[4 + f];
      const float v[3] = {fr.x, fr.y, fr.z};
      float w3[3];
      mv3(R, v, w3);
#pragma unroll
      for (int a = 0; a < 3; ++a) down[f][a] = (cfg.reset_feet_refresh || blowup) ? p.pos[a] + w3[a] : feet[f][a];
      f_last[f] = cfg.feet_f_last_init;
      step_len[f] = 0.f;
    }
  }
  // interval_command_resample (mode "interval", 3-6 s per env; after the resets, v4.py:426-439)
  ileft -= step_dt;
  if (ileft < 1e-6f) {
    ileft = draw(hs, 8) * (cfg.cmd_interval_s[1] - cfg.cmd_interval_s[0]) + cfg.cmd_interval_s[0];
    v4_resample(cfg, cnt, hs, 9, cur_yaw, cmd, tgt);
  }
  float he_obs;
  {
    float sn, cs;
    sincos_r(tgt - cur_yaw, &sn, &cs);
    he_obs = atan2f(sn, cs);
  }
  log_flush(q, lmask, acc);
  store_wc_row(q, wc, N, i, reset, wc_row);
  sp.mark(12);
  if (writer) {
    const Live live{reset};
#pragma unroll
    for (int a = 0; a < 3; ++a) { OUT(ZB_S_ROOT_POS + a) = p.pos[a]; OUT(ZB_S_ROOT_LINVEL + a) = p.lv[a]; OUT(ZB_S_ROOT_ANGVEL + a) = p.av[a]; }
#pragma unroll
    for (int a = 0; a < 4; ++a) OUT(ZB_S_ROOT_QUAT + a) = p.quat[a];
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      OUT(ZB_S_JOINT_POS + j) = p.jq[j]; OUT(ZB_S_JOINT_VEL + j) = p.jqd[j];
      OUT(ZB_V4_P_DELTA + j) = live(pr.pdel[j]); OUT(ZB_V4_ACTIONS + j) = live(pr.a_now[j]);
    }
    OUT(ZB_V4_COMMANDS) = cmd[0];
    OUT(ZB_V4_COMMANDS + 1) = cmd[1];
    OUT(ZB_V4_TARGET_YAW) = tgt;
    OUT(ZB_V4_INTERVAL_LEFT) = ileft;
    OUT(ZB_V4_CURRENT_YAW) = cur_yaw;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
#pragma unroll
      for (int a = 0; a < 3; ++a) OUT(ZB_V4_FEET_DOWN_POS + 3 * f + a) = down[f][a];
      OUT(ZB_V4_FEET_STEP_LEN + f) = step_len[f];
      OUT(ZB_V4_FEET_F_LAST + f) = f_last[f];
      OUT(ZB_V4_FEET_AIR_CUR + f) = live(air_cur[f]);
      OUT(ZB_V4_FEET_CONTACT_CUR + f) = live(con_cur[f]);
      OUT(ZB_V4_FEET_AIR_LAST + f) = live(air_last[f]);
      OUT(ZB_V4_FEET_CONTACT_LAST + f) = live(con_last[f]);

    }
    sens_store<ZB_V4_HIST>(q, cst, 1, 0, ZB_V4_FEET_FZ_HIST, ZB_V4_UNDES_FMAX_HIST, cfg.decimation, reset,
                           [&](int row, float v) { OUT(row) = v; });
    OUT(ZB_V4_EP_LEN) = live(ep_len);
#pragma unroll
    for (int t = 0; t < ZB_V4_NUM_REWARD_TERMS; ++t) OUT(ZB_V4_EP_SUMS + t) = live(sums[t]);

    // _get_observations (v4.py:851-881)
    float* o = &q.stg(ZB_V4_STATE_DIM);
    o[0] = obs_q[0]; o[1] = obs_q[1]; o[2] = obs_q[2]; o[3] = obs_q[3];
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      o[4 + j] = p.jq[j] - m->default_joint_pos[j];
      o[10 + j] = p.jqd[j];
      o[16 + j] = live(pr.a_now[j]);
    }
    o[22] = cmd[0];
    o[23] = he_obs;
    stage_result<ZB_V4_STATE_DIM, ZB_V4_OBS_DIM>(q, reward, died, time_out);
  }
  step_finish<ZB_V4_STATE_DIM, ZB_V4_OBS_DIM>(q, N, st, obs, rew, term, trunc, done, sp);
}

// explicit resets / construction (init = 1 also draws the interval-event timers, as Isaac Lab's
// EventManager does when it is created): log, reset events, defaults; one thread per env
__global__ void zb_v4_reset_kernel(const zb_model* __restrict__ mg, const float4* __restrict__ links, zb_task_cfg cfg,
                                   int N, float* __restrict__ st, const int32_t* __restrict__ ids, int n,
                                   float* __restrict__ acc, const Counters* __restrict__ cnt, uint64_t seed, int init) {
  MP m = to_mp(mg);
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int i = ids ? ids[t] : t;
  if (i < 0 || i >= N) return;
  const float step_dt = cfg.sim_dt * (float)cfg.decimation;
  if (!init) {
    const float dur = fmaxf(ST(ZB_V4_EP_LEN) * step_dt, step_dt);
#pragma unroll
    for (int k = 0; k < ZB_V4_NUM_REWARD_TERMS; ++k) atomicAdd(&acc_slot(acc, t)[k], ST(ZB_V4_EP_SUMS + k) / dur);
    atomicAdd(&acc_slot(acc, t)[ACC_NRES], 1.f);
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
  const float cur_yaw = reset_pose(m, cfg, hs, p);
  float cmd[2], tgt;
  v4_resample(cfg, cnt, hs, 5, cur_yaw, cmd, tgt);
#pragma unroll
  for (int a = 0; a < 3; ++a) { ST(ZB_S_ROOT_POS + a) = p.pos[a]; ST(ZB_S_ROOT_LINVEL + a) = p.lv[a]; ST(ZB_S_ROOT_ANGVEL + a) = p.av[a]; }
#pragma unroll
  for (int a = 0; a < 4; ++a) ST(ZB_S_ROOT_QUAT + a) = p.quat[a];
#pragma unroll
  for (int j = 0; j < ND; ++j) {
    ST(ZB_S_JOINT_POS + j) = p.jq[j]; ST(ZB_S_JOINT_VEL + j) = p.jqd[j];
    ST(ZB_V4_P_DELTA + j) = 0.f; ST(ZB_V4_ACTIONS + j) = 0.f;
  }
  ST(ZB_V4_COMMANDS) = cmd[0];
  ST(ZB_V4_COMMANDS + 1) = cmd[1];
  ST(ZB_V4_TARGET_YAW) = tgt;
  ST(ZB_V4_CURRENT_YAW) = cur_yaw;
  if (init) ST(ZB_V4_INTERVAL_LEFT) = draw(hs, 8) * (cfg.cmd_interval_s[1] - cfg.cmd_interval_s[0]) + cfg.cmd_interval_s[0];
  float R[9];
  qmat(p.quat, R);
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const float4 fr = links[DFLT_OFF + 4 + f];
    const float v[3] = {fr.x, fr.y, fr.z};
    float w3[3];
    mv3(R, v, w3);
#pragma unroll
    for (int a = 0; a < 3; ++a) ST(ZB_V4_FEET_DOWN_POS + 3 * f + a) = cfg.reset_feet_refresh ? p.pos[a] + w3[a] : pre[f][a];
    ST(ZB_V4_FEET_STEP_LEN + f) = 0.f;
    ST(ZB_V4_FEET_F_LAST + f) = cfg.feet_f_last_init;
    ST(ZB_V4_FEET_AIR_CUR + f) = 0.f;
    ST(ZB_V4_FEET_CONTACT_CUR + f) = 0.f;
    ST(ZB_V4_FEET_AIR_LAST + f) = 0.f;
    ST(ZB_V4_FEET_CONTACT_LAST + f) = 0.f;
#pragma unroll
    for (int h = 0; h < ZB_V4_HIST; ++h) ST(ZB_V4_FEET_FZ_HIST + 2 * h + f) = 0.f;
  }
#pragma unroll
  for (int h = 0; h < ZB_V4_HIST; ++h) ST(ZB_V4_UNDES_FMAX_HIST + h) = 0.f;
  ST(ZB_V4_EP_LEN) = 0.f;
#pragma unroll
  for (int k = 0; k < ZB_V4_NUM_REWARD_TERMS; ++k) ST(ZB_V4_EP_SUMS + k) = 0.f;
}

// the observation of env i's current state (v4.py _get_observations) into the row o (out of line: obs_row)
__device__ __noinline__ void v4_obs_row(const zb_model* mg, int N, const float* st, int i, float* o) {
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
    o[16 + j] = st[(size_t)(ZB_V4_ACTIONS + j) * N + i];
  }
  o[22] = st[(size_t)ZB_V4_COMMANDS * N + i];
  float sn, cs;
  sincos_r(st[(size_t)ZB_V4_TARGET_YAW * N + i] - st[(size_t)ZB_V4_CURRENT_YAW * N + i], &sn, &cs);
  o[23] = atan2f(sn, cs);
}

__global__ void zb_v4_observe_kernel(const zb_model* __restrict__ mg, int N, const float* __restrict__ st,
                                     float* __restrict__ obs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  v4_obs_row(mg, N, st, i, obs + (size_t)i * ZB_V4_OBS_DIM);
}
