// The manager step kernel's text. sim_manager.h stamps it four times; every stamp #defines the eight
// parameters checked below immediately before its #include, and this file #undefs them at its end, so no
// stamp inherits from another. One text, so the stamps cannot drift; separate kernels, because a shared
// __device__ body does not reproduce the events-off code (profiles/manager_events/kernel_resources.txt).
//
//   kernel                    EVENTS BI TERMS  arguments after seed (ZB_M_EV_PARAMS), before wc
//   zb_m_step_kernel            0    0    0    none: the kernel as it was before the events existed
//   zb_m_events_step_kernel     1    0    0    evc, evst
//   zb_m_dr_step_kernel         1    1    0    evc, evst, bi
//   zb_m_terms_step_kernel      1    1    1    evc, evst, bi, tmc, tmst
//
// ZB_M_EVENTS: the interval push and the yaw / heading commands of include/zbot_manager_events.h (evc the
// configuration, evst the event-state side buffer; ZB_M_EV_INIT builds the MEv record from them).
// ZB_M_BI: the base composite body's mass properties per env, include/zbot_base_inertia.h (bi, named by
// ZB_M_BI_ROWS: the side buffer float4[N][4], the body's three table rows, then the base link's COM in the
// body frame).
// ZB_M_TERMS: the five reward terms of include/zbot_manager_terms.h (tmc the configuration's device copy,
// read in the reward epilogue only; tmst the term-state side buffer float[ZB_MT_STATE_DIM][N], whose rows
// ride in the LDS carry behind the event state; ZB_M_TERMS_INIT builds the MTerms record). The feet's
// contact timers ride in the air timers' registers through the substep loop (a foot is in one mode at a
// time: > 0 air time, < 0 minus the contact time); everything else is in the reward epilogue. What the
// build costs in registers and scratch: profiles/manager_terms/kernel_resources.txt, held by
// tests/test_manager_terms_resources.py (40 / 56 B at two waves per SIMD against the dr build's 40 / 52 B,
// none at one; the TGS two-wave build parks a third per-lane 64-bit detection mask in scratch and reloads
// it inside a detection loop, one in-loop reload more than the dr build; DESIGN.md §9).
#if !defined(ZB_M_STEP_KERNEL) || !defined(ZB_M_EVENTS) || !defined(ZB_M_EV_PARAMS) || !defined(ZB_M_EV_INIT) || \
    !defined(ZB_M_BI) || !defined(ZB_M_BI_ROWS) || !defined(ZB_M_TERMS) || !defined(ZB_M_TERMS_INIT)
#error "zbot_m_step.inc: a stamp must define all eight ZB_M_* parameters (see the stamps in sim_manager.h)"
#endif
template <bool kTgs, int kOcc>
__global__ __launch_bounds__(WGT, kOcc) void ZB_M_STEP_KERNEL(
    const zb_model* __restrict__ mg, const float4* __restrict__ links, zb_task_cfg cfg, int N, float* __restrict__ st,
    const float* __restrict__ act, float* __restrict__ obs, float* __restrict__ rew, uint8_t* __restrict__ term,
    uint8_t* __restrict__ trunc, int64_t* __restrict__ done, float* __restrict__ acc,
    const Counters* __restrict__ cnt, uint64_t seed, ZB_M_EV_PARAMS float* __restrict__ wc) {
  constexpr bool kEvents = ZB_M_EVENTS != 0 && kOcc > 0;  // (value-dependent: the other branch is discarded)
  constexpr bool kBi = ZB_M_BI != 0 && kOcc > 0;
  constexpr bool kTerms = ZB_M_TERMS != 0 && kOcc > 0;
  const MEv<kEvents> ev ZB_M_EV_INIT;
  const MTerms<kTerms> tm ZB_M_TERMS_INIT;
  MP m = to_mp(mg);
  __shared__ float4 lds[LDS4 + (ZB_M_BI ? BI4 : 0)];
  if (kOcc == 1) asm volatile("" ::: "a255");  // (zb_step_kernel: kOcc)
  const int lane = threadIdx.x;
  const int env = xcd_block(blockIdx.x, gridDim.x) * EPW + lane / TL;
  const int i = env < N ? env : N - 1;
  const bool lead = env < N && lane % TL == 0;
  const Q q = make_q(lds, lane, links);
  for (int t = LNK_G + lane; t < LNK4; t += WGT) lds[LNK_OFF + t] = links[t];
  if constexpr (kBi) {  // the env's rows of the base body, read by its lane in every substep's fk_team
    if (q.s < 3) q.bi()[q.s] = ZB_M_BI_ROWS[(size_t)i * 4 + q.s];
  }
  Stamps sp;
  sp.begin();
  Phys p;
#pragma unroll
  for (int a = 0; a < 3; ++a) { p.pos[a] = ST(ZB_S_ROOT_POS + a); p.lv[a] = ST(ZB_S_ROOT_LINVEL + a); p.av[a] = ST(ZB_S_ROOT_ANGVEL + a); }
#pragma unroll
  for (int a = 0; a < 4; ++a) p.quat[a] = ST(ZB_S_ROOT_QUAT + a);
#pragma unroll
  for (int j = 0; j < ND; ++j) { p.jq[j] = ST(ZB_S_JOINT_POS + j); p.jqd[j] = ST(ZB_S_JOINT_VEL + j); }
  const float* cst;  // the friction rows load into FRIC; the event state rides behind the MDP rows
  if constexpr (kEvents) cst = carry_prefetch<ZB_M_LINK_MU, ZB_ME_STATE_DIM>(q, st, N, i, ev.st);
  else cst = carry_prefetch<ZB_M_LINK_MU>(q, st, N, i);
  if constexpr (kTerms) m_terms_prefetch(q, N, i, tm.st);
  if (q.s < NL) {
    q.fric(q.s) = ST(ZB_M_LINK_MU + q.s);
    q.fricd(q.s) = ST(ZB_M_LINK_MU_D + q.s);
  }

  // ActionManager.process_action: RelativeJointPositionAction (scale 0.04 pi, zero offset, clip
  // +-0.04 pi) in the Isaac Lab joint order, mapped onto the chain's joints
  const bool writer = q.s == 0;
  const float step_dt = cfg.sim_dt * (float)cfg.decimation;
  PreM& pv = *reinterpret_cast<PreM*>(&q.pre());
  float delta[ND];
  {
    PreM pr;
    pr.action_rate = 0.f;
#pragma unroll
    for (int a = 0; a < ND; ++a) {
      pr.a_raw[a] = act[(size_t)i * ZB_ACT_DIM + a];
      const float d = pr.a_raw[a] - ST(ZB_M_ACTIONS + a);
      pr.action_rate += d * d;
    }
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      float a = pr.a_raw[0];
#pragma unroll
      for (int b = 1; b < ND; ++b) a = m->api_joint_index[j] == b ? pr.a_raw[b] : a;
      delta[j] = m->api_joint_sign[j] * clampf(a * cfg.action_scale, -cfg.action_clip, cfg.action_clip);
      pr.jqd_prev[j] = 0.f;
    }
    if (writer) pv = pr;
  }

  // 4 x (apply_action: target = q + delta from the current joint positions; physics step;
  // ContactSensor.update: feet net force into the 3-slot history, air-time timers + sim_dt).
  // With 4 substeps the 3 history slots are this step's substeps 2..4.
  SensorOut so;
  float fz_h[3][2], fn_h[3][2];
  float air_cur[2] = {ST(ZB_M_FEET_AIR_CUR), ST(ZB_M_FEET_AIR_CUR + 1)};
  float air_last[2] = {ST(ZB_M_FEET_AIR_LAST), ST(ZB_M_FEET_AIR_LAST + 1)};
  if constexpr (kTerms) {
    wave_sync();  // (the carry rows of m_terms_prefetch)
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float ct = CST(M_CST_TERMS + ZB_MT_CONTACT_CUR + f);
      air_cur[f] = ct > 0.f ? -ct : air_cur[f];
    }
  }
  const bool hist_in = cfg.decimation < 3;  // >= 3 substeps overwrite every slot: no read
#pragma unroll
  for (int h = 0; h < 3; ++h)
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      fz_h[h][f] = hist_in ? ST(ZB_M_FEET_FZ_HIST + 2 * h + f) : 0.f;
      fn_h[h][f] = hist_in ? ST(ZB_M_FEET_FN_HIST + 2 * h + f) : 0.f;
    }
  wc_load(q, wc, N, i);  // the first substep's GJK warm start (DESIGN.md §3.2)
  sp.mark(0);
  for (int k = 0; k < cfg.decimation; ++k) {
    float target[ND];
#pragma unroll
    for (int j = 0; j < ND; ++j) target[j] = p.jq[j] + delta[j];
    if (k == cfg.decimation - 1 && writer) {
#pragma unroll
      for (int j = 0; j < ND; ++j) pv.jqd_prev[j] = p.jqd[j];
    }
    substep<false, true, kTgs, false, false, kBi>(m, cfg, p, target, q, true, true, so, nullptr, nullptr, sp);
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float fn = sqrtf(dot3(so.feet_f[f], so.feet_f[f]));
      fz_h[2][f] = fz_h[1][f]; fz_h[1][f] = fz_h[0][f]; fz_h[0][f] = so.feet_f[f][2];
      fn_h[2][f] = fn_h[1][f]; fn_h[1][f] = fn_h[0][f]; fn_h[0][f] = fn;
      const bool c = fn > cfg.contact_force_threshold;
      air_last[f] = (air_cur[f] > 0.f && c) ? air_cur[f] + cfg.sim_dt : air_last[f];
      if constexpr (kTerms) {  // current_contact_time = c ? t + sim_dt : 0 beside current_air_time, signed
        const float same = (c ? air_cur[f] < 0.f : air_cur[f] > 0.f) ? air_cur[f] : 0.f;
        air_cur[f] = c ? same - cfg.sim_dt : same + cfg.sim_dt;
      } else {
        air_cur[f] = c ? 0.f : air_cur[f] + cfg.sim_dt;
      }
    }
    sp.mark(7);
  }
  PreM pr;
  const float wc_row = after_substeps(m, q, st, pr);

  float con_cur[2] = {0.f, 0.f};  // kTerms: ContactSensor current_contact_time of the feet
  if constexpr (kTerms) {
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      con_cur[f] = fmaxf(-air_cur[f], 0.f);
      air_cur[f] = fmaxf(air_cur[f], 0.f);
    }
  }
  const float ep_len = CST(ZB_M_EP_LEN) + 1.f;
  float cmd[3] = {CST(ZB_M_COMMANDS), CST(ZB_M_COMMANDS + 1), CST(ZB_M_COMMANDS + 2)};
  float tleft = CST(ZB_M_CMD_TIME_LEFT), standing = CST(ZB_M_CMD_STANDING);
  float met[2] = {CST(ZB_M_METRICS), CST(ZB_M_METRICS + 1)};
  float f_last[2] = {CST(ZB_M_FEET_F_LAST), CST(ZB_M_FEET_F_LAST + 1)};
  float step_len[2] = {CST(ZB_M_FEET_STEP_LEN), CST(ZB_M_FEET_STEP_LEN + 1)};
  float down[2][3];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int a = 0; a < 3; ++a) down[f][a] = CST(ZB_M_FEET_DOWN_POS + 3 * f + a);

  // post-step articulation data: root (= base link) pose, link-origin / COM velocity, angular
  // velocity; feet link poses and COM velocities
  float bq[4], bp[3], vb[3], vcom[3], wb[3], feet[2][3], fq[2][4], fvel[2][3];
  float blc[3] = {0.f, 0.f, 0.f};  // kBi: this env's base-link COM (body frame)
  float fcz[2] = {0.f, 0.f};       // kTerms: world height of each foot's clearance point
  if constexpr (kBi) {
    const float4 c = ZB_M_BI_ROWS[(size_t)i * 4 + 3];
    blc[0] = c.x; blc[1] = c.y; blc[2] = c.z;
  }
  {
    wave_sync();
    fk_team_pose(p, q);
    wave_sync();
    float S[ND][6], org[ND][3];
    read_joints(q, S, org);
    const int B = m->base_link;
    link_pose_q(m, q, B, bp, bq);
#pragma unroll
    for (int a = 0; a < 3; ++a) bp[a] += p.pos[a];
    link_origin_vel_q(m, q, p, S, B, vb);
    link_com_vel_q<kBi>(m, q, p, S, B, vcom, blc);
    body_ang_vel_q(p, S, link_body(B), wb);
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int l = f == 0 ? 0 : 11;
      link_pose_q(m, q, l, feet[f], fq[f]);
#pragma unroll
      for (int a = 0; a < 3; ++a) feet[f][a] += p.pos[a];
      link_com_vel_q(m, q, p, S, l, fvel[f]);
      if constexpr (kTerms) {
        const float4 rz = q.frame(link_body(l), 2);  // the body pose's {R row 2, p.z} (read_frame)
        fcz[f] = p.pos[2] + rz.w + (rz.x * tm.c->clearance_point[f][0] + rz.y * tm.c->clearance_point[f][1] +
                                    rz.z * tm.c->clearance_point[f][2]);
      }
    }
  }
  // TerminationManager (flat: time_out, base_height < 0.2, feet_close < 0.12)
  const bool time_out = ep_len >= (float)cfg.max_episode_length;
  const bool low = bp[2] < cfg.termination_height;
  const float fd[3] = {feet[0][0] - feet[1][0], feet[0][1] - feet[1][1], feet[0][2] - feet[1][2]};
  const bool close = sqrtf(dot3(fd, fd)) < cfg.feet_close_min;
  const bool blowup = phys_bad(p);  // non-finite guard (phys_bad), as in the walking kernel
  const bool terminated = low || close || blowup;

  // RewardManager.compute: term * weight * step_dt in cfg order (mgr.py:262-357, flat overrides)
  float r[ZB_M_NUM_REWARD_TERMS];
  float xr[ZB_MT_NUM_TERMS], fsum = 0.f;  // kTerms: the five terms, env.feet_force_sum
  if constexpr (kTerms) fsum = CST(M_CST_TERMS + ZB_MT_FEET_FORCE_SUM);
  {
    float Rb[9];
    qmat(bq, Rb);
    const float fwd[3] = {Rb[4], -Rb[1], 0.f};  // GRAVITY_VEC_W x quat_apply(root_quat, y)
    float vx, vy;
    {  // yaw_quat + quat_apply_inverse on root_link_lin_vel_w
      const float yaw = atan2f(2.f * (bq[0] * bq[3] + bq[1] * bq[2]), 1.f - 2.f * (bq[2] * bq[2] + bq[3] * bq[3]));
      float sy, cy;
      sincos_r(yaw, &sy, &cy);
      vx = cy * vb[0] + sy * vb[1];
      vy = -sy * vb[0] + cy * vb[1];
    }
    const float ex = cmd[0] - vx, ey = cmd[1] - vy;
    r[ZB_M_R_TRACK_LIN_VEL_XY] = __expf(-(ex * ex + ey * ey) / 0.25f);
    const float ez = cmd[2] - wb[2];
    r[ZB_M_R_TRACK_ANG_VEL_Z] = __expf(-(ez * ez) / 0.25f);
    r[ZB_M_R_TERMINATION] = terminated ? 1.f : 0.f;
    r[ZB_M_R_DOF_TORQUES] = so.tau2;
    float ja = 0.f;
#pragma unroll
    for (int j = 0; j < ND; ++j) {
      const float aj = (p.jqd[j] - pr.jqd_prev[j]) / cfg.sim_dt;
      ja += aj * aj;
    }
    r[ZB_M_R_DOF_ACC] = ja;
    r[ZB_M_R_ACTION_RATE] = pr.action_rate;
    // foot_step_length (rewards.py:44-104)
    const float nrm = sqrtf(dot3(fwd, fwd)) + 1e-6f;
    const float fh[3] = {fwd[0] / nrm, fwd[1] / nrm, fwd[2] / nrm};
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float fz = (fz_h[0][f] + fz_h[1][f] + fz_h[2][f]) / 3.f;
      if (fz > 10.f && f_last[f] < 10.f) {
        const float dv[3] = {feet[f][0] - down[f][0], feet[f][1] - down[f][1], feet[f][2] - down[f][2]};
        step_len[f] = fabsf(dot3(dv, fh));
#pragma unroll
        for (int a = 0; a < 3; ++a) down[f][a] = feet[f][a];
      }
      f_last[f] = fz;
    }
    r[ZB_M_R_FOOT_STEP_LENGTH] = tanh_r(15.f * fminf(step_len[0], step_len[1]));
    float sd = 0.f, sfw = 0.f, sl = 0.f;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      float R[9];
      qmat(fq[f], R);
      const float sg = f == 0 ? 1.f : -1.f;  // foot_downward: feet axes (0, 1, 0), (0, -1, 0) vs z
      const float dz[3] = {sg * R[1], sg * R[4], sg * R[7] - 1.f};
      sd += sqrtf(dot3(dz, dz));
      const float dx[3] = {R[0] - fwd[0], R[3] - fwd[1], R[6] - fwd[2]};  // foot_forward
      sfw += sqrtf(dot3(dx, dx));
      const bool c = fmaxf(fn_h[0][f], fmaxf(fn_h[1][f], fn_h[2][f])) > 1.0f;  // feet_slide
      sl += sqrtf(fvel[f][0] * fvel[f][0] + fvel[f][1] * fvel[f][1]) * (c ? 1.f : 0.f);
    }
    r[ZB_M_R_FOOT_DOWNWARD] = sd;
    r[ZB_M_R_FOOT_FORWARD] = sfw;
    r[ZB_M_R_FEET_SLIDE] = sl;
    r[ZB_M_R_AIR_TIME_BALANCE] = fabsf(air_last[0] - air_last[1]);
    if constexpr (kTerms) {
      const zb_manager_terms& tc = *tm.c;
      const bool in_c0 = con_cur[0] > 0.f, in_c1 = con_cur[1] > 0.f;
      {  // feet_gait (rewards.py:155-183): fp32 phase arithmetic in the reference's order
        const float ph = fmod_pos(ep_len * step_dt, tc.gait_period) / tc.gait_period;
        float n = 0.f;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          float lp = ph + tc.gait_offset[f];
          lp -= floorf(lp);  // (% 1, exact)
          n += ((lp < tc.gait_threshold) == (f == 0 ? in_c0 : in_c1)) ? 1.f : 0.f;
        }
        xr[ZB_MT_GAIT] = sqrtf(dot3(cmd, cmd)) > 0.05f ? n : 0.f;
      }
      {  // foot_clearance_reward (rewards.py:144-153)
        float e = 0.f;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const float dz = fcz[f] - tc.clearance_target_height;
          e += dz * dz * tanh_r(tc.clearance_tanh_mult * sqrtf(fvel[f][0] * fvel[f][0] + fvel[f][1] * fvel[f][1]));
        }
        xr[ZB_MT_FEET_CLEARANCE] = __expf(-e / tc.clearance_std);
      }
      {  // feet_air_time_positive_biped (rewards.py:207-226)
        const float t0 = in_c0 ? con_cur[0] : air_cur[0], t1 = in_c1 ? con_cur[1] : air_cur[1];
        const float t = in_c0 != in_c1 ? fminf(fminf(t0, t1), tc.air_time_threshold) : 0.f;
        xr[ZB_MT_FEET_AIR_TIME] = sqrtf(cmd[0] * cmd[0] + cmd[1] * cmd[1]) > 0.1f ? t : 0.f;
      }
      xr[ZB_MT_BASE_VEL_FORWARD] = tc.which_forward * (vb[0] * fwd[0] + vb[1] * fwd[1]);  // (rewards.py:266-275)
      {  // feet_force_pattern (rewards.py:277-287): the sign before the integrator's update, sign(0) = 0
        const float f0 = (fz_h[0][0] + fz_h[1][0] + fz_h[2][0]) / 3.f, f1 = (fz_h[0][1] + fz_h[1][1] + fz_h[2][1]) / 3.f;
        const float sg = fsum > 0.f ? 1.f : fsum < 0.f ? -1.f : 0.f;
        const float nsum = fsum + 0.001f * (f0 - f1);
        fsum = (tc.active >> ZB_MT_FEET_FORCE_PATTERN) & 1u ? nsum : fsum;
        xr[ZB_MT_FEET_FORCE_PATTERN] = 0.5f * (f1 - f0) * sg - 0.1f * fabsf(fsum);
      }
    }
  }
  float reward = 0.f, sums[ZB_M_NUM_REWARD_TERMS];
#pragma unroll
  for (int t = 0; t < ZB_M_NUM_REWARD_TERMS; ++t) {
    const float v = r[t] * cfg.stage_scales[0][t] * step_dt;
    reward += v;
    sums[t] = CST(ZB_M_EP_SUMS + t) + v;
  }
  if constexpr (kTerms) {  // the reward again as the sixteen fields' sum in cfg order
    float xv[ZB_MT_NUM_TERMS];
#pragma unroll
    for (int t = 0; t < ZB_MT_NUM_TERMS; ++t) {
      const float s0 = CST(M_CST_TERMS + ZB_MT_EP_SUMS + t);
      xv[t] = (tm.c->active >> t) & 1u ? xr[t] * tm.c->weight[t] * step_dt : 0.f;
      // the term state leaves for its staging entries at once (region U holds nothing else in the
      // epilogue), so none of it is live through the resets, the command update and the observation
      if (writer) OUT(M_STG_TERMS + ZB_MT_EP_SUMS + t) = blowup ? s0 : s0 + xv[t];
    }
    if (writer) {
      OUT(M_STG_TERMS + ZB_MT_CONTACT_CUR) = con_cur[0];
      OUT(M_STG_TERMS + ZB_MT_CONTACT_CUR + 1) = con_cur[1];
      OUT(M_STG_TERMS + ZB_MT_FEET_FORCE_SUM) = fsum;
    }
    reward = 0.f;
#pragma unroll
    for (int t = 0; t < ZB_M_NUM_REWARD_TERMS + ZB_MT_NUM_TERMS; ++t) {
      const int s = M_CFG_ORDER[t];
      reward += s >= 0 ? r[max(s, 0)] * cfg.stage_scales[0][max(s, 0)] * step_dt : xv[max(-1 - s, 0)];
    }
  }
  if (blowup) {  // finite reward (the is_terminated term alone), the episode sums without this step
    reward = cfg.stage_scales[0][ZB_M_R_TERMINATION] * step_dt;
#pragma unroll
    for (int t = 0; t < ZB_M_NUM_REWARD_TERMS; ++t) sums[t] = CST(ZB_M_EP_SUMS + t);
  }
  const bool reset = terminated || time_out;
  const uint64_t hs = env_hash(seed, cnt->calls, i);
  float a_obs[ND];
#pragma unroll
  for (int a = 0; a < ND; ++a) a_obs[a] = pr.a_raw[a];
  float vcb[3], wcb[3];  // root_lin_vel_b (COM), root_ang_vel_b after the resets

  // _reset_idx: curriculum (finalize), events reset_base / reset_robot_joints / reset_my_data,
  // managers (actions 0, reward sums and metrics logged, command resampled, sensor cleared)
  const uint64_t lmask = __ballot(reset && lead);
  float push_t = 0.f, head_target = 0.f, is_heading = 0.f;  // the event state (kEvents)
  if constexpr (kEvents) {
    push_t = CST(ZB_M_LINK_MU + ZB_ME_PUSH_TIME_LEFT);
    head_target = CST(ZB_M_LINK_MU + ZB_ME_HEADING_TARGET);
    is_heading = CST(ZB_M_LINK_MU + ZB_ME_IS_HEADING);
  }
  if (reset) {
    if (lead) {
      float* lr = log_row(q);
#pragma unroll
      for (int t = 0; t < ZB_M_NUM_REWARD_TERMS; ++t) lr[t] = sums[t];
      if constexpr (kTerms) {
#pragma unroll
        for (int t = 0; t < ZB_MT_NUM_TERMS; ++t) lr[ZB_M_NUM_REWARD_TERMS + t] = OUT(M_STG_TERMS + ZB_MT_EP_SUMS + t);
      }
      lr[ACC_NRES] = 1.f;
      lr[ACC_DIED] = low ? 1.f : 0.f;
      lr[ACC_TOUT] = time_out ? 1.f : 0.f;
      lr[ACC_TERM2] = close ? 1.f : 0.f;
      lr[ACC_MET0] = met[0];
      lr[ACC_MET1] = met[1];
    }
    (void)reset_pose(m, cfg, hs, p);
    const float4 qr = q.dflt()[3];
    const float qrel[4] = {qr.x, qr.y, qr.z, qr.w};
    qmul(p.quat, qrel, bq);
    float R[9];
    qmat(p.quat, R);
#pragma unroll
    for (int f = 0; f < 2; ++f) {  // reset_my_data: pre-reset feet (rewards.py:42, DESIGN.md §4) or reset pose's
      const float4 fr = q.dflt()[4 + f];
      const float v[3] = {fr.x, fr.y, fr.z};
      float w3[3];
      mv3(R, v, w3);
#pragma unroll
      for (int a = 0; a < 3; ++a) down[f][a] = (cfg.reset_feet_refresh || blowup) ? p.pos[a] + w3[a] : feet[f][a];
      f_last[f] = 0.f;
      step_len[f] = 0.f;
    }
    m_resample(cfg, cnt, hs, M_DRAW_RESET_CMD, cmd, standing);
    if constexpr (kEvents) {
      m_resample_yaw(ev.c, hs, M_DRAW_RESET_YAW, cmd[2], head_target, is_heading);
      if (ev.c.push_enabled) push_t = m_uniform(hs, M_DRAW_RESET_PUSH_T, ev.c.push_interval_s);  // EventManager.reset
    }
    tleft = cfg.cmd_resample_s;
    met[0] = met[1] = 0.f;
#pragma unroll
    for (int a = 0; a < ND; ++a) a_obs[a] = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) { vcb[a] = 0.f; wcb[a] = 0.f; }
  } else {
    float R[9];
    qmat(bq, R);
    vcb[0] = R[0] * vcom[0] + R[3] * vcom[1] + R[6] * vcom[2];
    vcb[1] = R[1] * vcom[0] + R[4] * vcom[1] + R[7] * vcom[2];
    vcb[2] = R[2] * vcom[0] + R[5] * vcom[1] + R[8] * vcom[2];
    wcb[0] = R[0] * wb[0] + R[3] * wb[1] + R[6] * wb[2];
    wcb[1] = R[1] * wb[0] + R[4] * wb[1] + R[7] * wb[2];
    wcb[2] = R[2] * wb[0] + R[5] * wb[1] + R[8] * wb[2];
  }
  // CommandManager.compute: metrics (UniformVelocityCommand._update_metrics), timer, resample,
  // standing envs zeroed
  {
    const float max_steps = cfg.cmd_resample_s / step_dt;
    const float ex = cmd[0] - vcb[0], ey = cmd[1] - vcb[1];
    met[0] += sqrtf(ex * ex + ey * ey) / max_steps;
    met[1] += fabsf(cmd[2] - wcb[2]) / max_steps;
    tleft -= step_dt;
    if (tleft <= 0.f) {
      m_resample(cfg, cnt, hs, M_DRAW_CMD, cmd, standing);
      if constexpr (kEvents) m_resample_yaw(ev.c, hs, M_DRAW_YAW, cmd[2], head_target, is_heading);
      tleft = cfg.cmd_resample_s;
    }
    if constexpr (kEvents) m_heading_cmd(ev.c, bq, head_target, is_heading, cmd);
    if (standing > 0.5f) cmd[0] = cmd[1] = cmd[2] = 0.f;
  }
  // EventManager.apply(mode="interval", dt=step_dt): push_robot. A reset env's timer is fresh; should it
  // run out at once (push_interval_s[0] < step_dt) it fires in the next step, from that step's pose.
  if constexpr (kEvents) {
    if (ev.c.push_enabled) {
      push_t -= step_dt;
      if (push_t < 1e-6f && !reset) {
        m_push<kBi>(m, q, ev.c, hs, p, blc);
        push_t = m_uniform(hs, M_DRAW_PUSH_T, ev.c.push_interval_s);
      }
    }
  }
  log_flush(q, lmask, acc);
  store_wc_row(q, wc, N, i, reset, wc_row);
  sp.mark(12);
  if (writer) {
    const Live live{reset};
    stage_phys(q, p);
#pragma unroll
    for (int a = 0; a < ND; ++a) OUT(ZB_M_ACTIONS + a) = a_obs[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) OUT(ZB_M_COMMANDS + a) = cmd[a];
    OUT(ZB_M_CMD_TIME_LEFT) = tleft;
    OUT(ZB_M_CMD_STANDING) = standing;
    OUT(ZB_M_METRICS) = met[0];
    OUT(ZB_M_METRICS + 1) = met[1];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
#pragma unroll
      for (int a = 0; a < 3; ++a) OUT(ZB_M_FEET_DOWN_POS + 3 * f + a) = down[f][a];
      OUT(ZB_M_FEET_STEP_LEN + f) = step_len[f];
      OUT(ZB_M_FEET_F_LAST + f) = f_last[f];
      OUT(ZB_M_FEET_AIR_CUR + f) = live(air_cur[f]);
      OUT(ZB_M_FEET_AIR_LAST + f) = live(air_last[f]);
#pragma unroll
      for (int h = 0; h < 3; ++h) { OUT(ZB_M_FEET_FZ_HIST + 2 * h + f) = live(fz_h[h][f]); OUT(ZB_M_FEET_FN_HIST + 2 * h + f) = live(fn_h[h][f]); }
    }
    OUT(ZB_M_EP_LEN) = live(ep_len);
#pragma unroll
    for (int t = 0; t < ZB_M_NUM_REWARD_TERMS; ++t) OUT(ZB_M_EP_SUMS + t) = live(sums[t]);
    m_write_obs(m, cfg, hs, bq, cmd, p, a_obs, &q.stg(ZB_M_LINK_MU));
    stage_result<ZB_M_LINK_MU, ZB_M_OBS_DIM>(q, reward, terminated, time_out);
    if constexpr (kEvents) {
      OUT(M_STG_EV + ZB_ME_PUSH_TIME_LEFT) = push_t;
      OUT(M_STG_EV + ZB_ME_HEADING_TARGET) = head_target;
      OUT(M_STG_EV + ZB_ME_IS_HEADING) = is_heading;
    }
    if constexpr (kTerms) {  // ContactSensor.reset, reset_my_data and RewardManager.reset zero a reset env's rows
      if (reset) {
#pragma unroll
        for (int f = 0; f < ZB_MT_STATE_DIM; ++f) OUT(M_STG_TERMS + f) = 0.f;
      }
    }
  }
  if constexpr (kEvents) m_ev_store(q, xcd_block(blockIdx.x, gridDim.x) * EPW, N, ev.st);
  if constexpr (kTerms) m_terms_store(q, xcd_block(blockIdx.x, gridDim.x) * EPW, N, tm.st);
  step_finish<ZB_M_LINK_MU, ZB_M_OBS_DIM>(q, N, st, obs, rew, term, trunc, done, sp);
}
#undef ZB_M_STEP_KERNEL
#undef ZB_M_EVENTS
#undef ZB_M_EV_PARAMS
#undef ZB_M_EV_INIT
#undef ZB_M_BI
#undef ZB_M_BI_ROWS
#undef ZB_M_TERMS
#undef ZB_M_TERMS_INIT
