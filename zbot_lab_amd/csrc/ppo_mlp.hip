// ppo_mlp.hip — the PPO minibatch update of rsl_rl's ActorCritic as fp32 MFMA kernels for gfx950
// (libzbot_ppo.so, C ABI include/zbot_ppo.h). Restates zbot_lab_amd/rl/ppo.py:PPO.update_steps
// (rsl_rl PPO, reference agents/rsl_rl_ppo_cfg.py:65-91, ppo_learning_notes.md:521-548) per
// minibatch in a handful of launches instead of ~150 torch kernels:
//
//   k_pack       padded / transposed / lane-ordered weight images in the workspace
//   k_rows_reg   (the shipped net shapes) one wave per 16 minibatch rows, activations in registers:
//                gather through the permutation, actor forward (Linear + the nets' activation, ELU in
//                every shipped cfg, relu / tanh / selu / lrelu as template instantiations, on
//                v_mfma_f32_16x16x4_f32, the previous layer's accumulators as the B operand, weights
//                shared by the workgroup's four waves through LDS), Gaussian log-prob / KL / clipped
//                surrogate and its gradient, actor backward dX; then the critic forward, clipped value
//                loss and backward. Every layer's input X_l and pre-activation gradient dZ_l go to HBM
//                (octet-blocked rows) for the weight gradients.
//   k_rows       the same with the activations in LDS (32-row tiles; any other shape, ZBP_ROWS=lds)
//   k_wgrad      dW_l = dZ_l^T X_l and db_l = sum dZ_l: an LDS-tiled GEMM over the minibatch rows,
//                128 x 128 output blocks, split-K over row ranges sized to one round of the device's
//                resident workgroups; partial tiles to the workspace
//   k_reduce     partial tiles -> every parameter's .grad, the std gradient, the minibatch stats
//   (rsl_rl's symmetry option, zbp_symmetry: the kSym instantiations of k_rows_reg, k_rows_sym and
//   k_reduce_sym run 2 B rows, every original next to its mirror image in one row tile; off, the kernels
//   above are the code they were)
//
// and, on one GPU, k_adam (adaptive learning rate, global-norm clipping from k_reduce's per-tile sums
// of squares, or k_norm's, Adam) + the re-pack (k_pack, which also writes the new rate and step); the rollout's policy step (k_act_reg / k_act), its bookkeeping (k_env_post) and
// GAE (k_gae, k_adv_stats, k_adv_norm). Empirical observation normalization (zbp_obs_norm) is applied
// where a row tile's inputs are gathered, and its running statistics are kept by k_obs_part /
// k_obs_merge (zbp_norm_update). Exact fp32 throughout (the MFMA is a k-ordered fmaf chain);
// results differ from torch's only by summation order. MI355X mapping: the weights (<= 450 KB per
// net) stay L2-resident; design and measurements in DESIGN.md §7 (round 5).
//
// Every formula is stated once, in a __forceinline__ helper that every kernel computing it calls:
// sigma_of, logp_term, kl_term, surrogate, gauss_grad, value_loss (beside act_f), sample_action (the act
// kernels' draw and stores, beside noise_at), rr_input (the register kernels' first-layer operand) and
// rr_forward_chain / rr_backward_chain (a net's pass in the register kernels). Host side: with_act (the one
// switch over the activations, device side too), with_act_norm (the register kernels' instantiation set),
// lds_row_tile (the LDS row tile of k_rows / k_act) and TileMap (the weight tiles, shared by Layout,
// k_wgrad and k_reduce). DESIGN.md §7, "One statement of each PPO formula".
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "zbot_ppo.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int TR = 32;            // rows per tile (the MFMA's M)
constexpr int MAXL = ZBP_MAX_LAYERS;
constexpr int PART = 32 * 32 + 32;  // one weight-gradient partial tile + its bias column
constexpr int NSTAT = 16;           // per-row-tile partial sums (surrogate, value, kl, std grads)
// k_rows workgroup: 8 waves on one 32-row tile (a layer's output tiles dealt over them): with the
// C5 nets' 97 KB of activations one workgroup fits a CU, so two waves share each SIMD and cover each
// other's LDS / L2 waits
constexpr int ROW_THREADS = 512;
// zbp_act's kernel choice by rollout rows: the register-resident forward (k_act_reg / k_act_split) from
// ZBP_ACT_REG_MIN rows, the split-output one (k_act_split, the 128-wide nets) up to ZBP_ACT_SPLIT_MAX
#ifndef ZBP_ACT_REG_MIN
#define ZBP_ACT_REG_MIN 4096
#endif
#ifndef ZBP_ACT_SPLIT_MAX
#define ZBP_ACT_SPLIT_MAX 65536
#endif

thread_local char g_err[256] = "";
int fail(int code, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s", what);
  return code;
}
int hip_fail(hipError_t e, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return -2;
}

inline int pad32(int d) { return (d + 31) & ~31; }

// Row buffers (X_l, dZ_l) in HBM are octet-blocked feature-major: feature f of minibatch row i of a
// P-feature buffer at ((i >> 3) P + f) 8 + (i & 7), i.e. for every octet of rows the features' 8-row
// runs (32 B) back to back. k_wgrad's lanes (one feature each, four rows) then read 1 KB contiguous
// per instruction (8 full lines) instead of one 16-byte piece from each of 32 lines.
__host__ __device__ __forceinline__ int64_t rbo(int P, int f, int i) { return ((int64_t)(i >> 3) * P + f) * 8 + (i & 7); }

// one net in the workspace: dims and float offsets of its images and row buffers
struct NetW {
  int L, d[MAXL + 1], p[MAXL + 1];
  int act;                               // ZBP_ACT_* (the LDS kernels branch on it; the register kernels are instantiated per value)
  int64_t wp[MAXL], wt[MAXL], bp[MAXL];  // padded weights [p(l+1)][p(l)], transposed [p(l)][p(l+1)], bias [p(l+1)]
  int64_t wr[MAXL], wtr[MAXL];           // the same in k_rows_reg's lane order (forward / backward A operands)
  int64_t x[MAXL], dz[MAXL];             // row buffers: X_l [B][p(l)], dZ_l [B][p(l+1)]
};
// the weight tiles of both nets and k_wgrad's launch over them (make_layout fills it; k_wgrad and k_reduce
// get a copy)
struct TileMap {
  int wtiles, tile0[2 * MAXL + 1];  // weight tiles of (net, layer) in order, prefix counts
  int ngroups, grp0[2 * MAXL + 1];  // k_wgrad workgroups (<= 4 x 4 output x reduction tiles) of (net, layer), prefix counts
  int splits;                       // the largest row split count
  int sp_nl[2 * MAXL];              // row splits of (net, layer) (one count for all, see make_layout)
  int ord[2 * MAXL];                // k_wgrad launch order of the (net, layer)s
  int blk0[2 * MAXL + 1];           // k_wgrad launch: first workgroup of the (net, layer) at order position i
};
struct Layout {
  NetW n[2];
  int64_t stats;  // [tiles][NSTAT] per-row-tile partial sums
  int64_t part;   // [splits (the largest)][wtiles][PART] weight-gradient partials
  TileMap tm;
  int64_t scratch;  // [max(64, wtiles + 1)] gradient sums of squares: k_norm's per block, or k_reduce's per weight tile
  int64_t rng;      // [1] uint32: the draw counter of the in-kernel action noise, advanced by every k_pack
  int64_t sym;      // [B / 16] per-row-tile sums of the symmetry loss's squared errors (zbp_symmetry; last, so every other offset is as without it)
  int64_t total;
};

// k_wgrad workgroups resident at once: two per CU (64 KB of LDS each); the CU count of the current
// device (256 on MI355X; 256 when no device is visible)
int wgrad_slots() {
  static const int cus = [] {
    int d = 0, n = 0;
    if (hipGetDevice(&d) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess ||
        n <= 0)
      n = 256;
    (void)hipGetLastError();
    return n;
  }();
  // (ZBP_WGRAD_SLOTS_PER_CU, read once: the split-K A/B; default 2 = the resident k_wgrad workgroups)
  static const int per_cu = [] {
    const char* e = getenv("ZBP_WGRAD_SLOTS_PER_CU");
    const int v = e ? atoi(e) : 2;
    return v >= 1 && v <= 8 ? v : 2;
  }();
  return per_cu * cus;
}

Layout make_layout(const zbp_net* a, const zbp_net* c, int B) {
  Layout lo{};
  TileMap& tm = lo.tm;
  int64_t off = 0;
  auto take = [&](int64_t n) { int64_t o = off; off += (n + 63) & ~int64_t(63); return o; };
  const zbp_net* nets[2] = {a, c};
  int t = 0;
  for (int k = 0; k < 2; ++k) {
    NetW& w = lo.n[k];
    w.L = nets[k]->n_layers;
    w.act = nets[k]->activation;
    for (int l = 0; l <= w.L; ++l) { w.d[l] = nets[k]->dim[l]; w.p[l] = pad32(w.d[l]); }
    for (int l = 0; l < w.L; ++l) {
      w.wp[l] = take((int64_t)w.p[l + 1] * w.p[l]);
      w.wt[l] = take((int64_t)w.p[l] * w.p[l + 1]);
      w.bp[l] = take(w.p[l + 1]);
      w.wr[l] = take((int64_t)w.p[l + 1] * w.p[l]);
      w.wtr[l] = take((int64_t)w.p[l] * w.p[l + 1]);
      w.x[l] = take((int64_t)B * w.p[l]);
      w.dz[l] = take((int64_t)B * w.p[l + 1]);
      tm.tile0[k * MAXL + l] = t;
      t += (w.p[l + 1] / 32) * (w.p[l] / 32);
    }
    for (int l = w.L; l < MAXL; ++l) tm.tile0[k * MAXL + l] = t;
  }
  tm.tile0[2 * MAXL] = t;
  tm.wtiles = t;
  // weight-gradient workgroups: per (net, layer) groups of up to 4 output tiles (one wave each) x up
  // to 4 reduction tiles
  int g = 0;
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < MAXL; ++l) {
      tm.grp0[k * MAXL + l] = g;
      if (l < lo.n[k].L) g += ((lo.n[k].p[l + 1] / 32 + 3) / 4) * ((lo.n[k].p[l] / 32 + 3) / 4);
    }
  tm.grp0[2 * MAXL] = g;
  tm.ngroups = g;
  lo.stats = take((int64_t)(B / 16) * NSTAT);  // (per 32-row tile of k_rows, per 16-row wave of k_rows_reg)
  // row splits of the weight gradients: as many as fill the device's resident k_wgrad workgroups in
  // ONE round (groups x splits <= slots; a second, partly filled round would leave most CUs idle for
  // a whole split's time); a split is a contiguous range of 32-row chunks (k_wgrad's LDS chunks). The
  // same count for every layer: a chunk costs about the same in every group (its copy and barrier
  // latency, not the MFMAs, set the pace: splits weighted by the groups' MFMA work made the launch
  // 66 -> 87 us)
  const int C = B / 32;
  int s = wgrad_slots() / g;
  s = s < 1 ? 1 : (s > C ? C : (s > 1024 ? 1024 : s));
  // launch order: the layers whose blocks keep all four waves' MFMAs busy (2 x 2 tiles per wave)
  // first, then the input / output layers (half the MFMAs per wave): with the launch filling every CU's
  // first slot before its second, a CU then pairs a busy block with a light one instead of two busy ones
  int b = 0, pos = 0;
  for (int pass = 0; pass < 2; ++pass)
    for (int nl = 0; nl < 2 * MAXL; ++nl) {
      const int k = nl / MAXL, l = nl % MAXL;
      const bool busy = l < lo.n[k].L && lo.n[k].p[l + 1] >= 64 && lo.n[k].p[l] >= 64;
      if ((pass == 0) != busy) continue;
      tm.ord[pos] = nl;
      tm.blk0[pos++] = b;
      tm.sp_nl[nl] = s;
      b += (tm.grp0[nl + 1] - tm.grp0[nl]) * s;
    }
  tm.blk0[2 * MAXL] = b;
  tm.splits = s;
  lo.part = take((int64_t)s * t * PART);
  lo.scratch = take(t + 1 > 64 ? t + 1 : 64);
  lo.rng = take(1);
  lo.sym = take(B / 16);
  lo.total = off;
  return lo;
}

const char* check_net(const zbp_net* n) {
  if (!n || n->n_layers < 1 || n->n_layers > MAXL) return "n_layers must be 1..4";
  if (n->dim[0] < 1 || n->dim[0] > 32) return "input dim must be 1..32";
  for (int l = 1; l < n->n_layers; ++l)
    if (n->dim[l] < 32 || n->dim[l] > 256 || n->dim[l] % 32) return "hidden dims must be multiples of 32 up to 256";
  if (n->dim[n->n_layers] < 1 || n->dim[n->n_layers] > 32) return "output dim must be 1..32";
  for (int l = 0; l < n->n_layers; ++l)
    if (!n->w[l] || !n->b[l]) return "null weight / bias";
  if (n->activation < ZBP_ACT_ELU || n->activation > ZBP_ACT_LRELU) return "activation must be one of ZBP_ACT_*";
  return nullptr;
}
// both nets of a call: each within the limits, and one activation for the pair (rsl_rl has one
// `activation`; the paired register kernels are instantiated per activation)
const char* check_nets(const zbp_net* a, const zbp_net* c) {
  if (const char* e = check_net(a)) return e;
  if (const char* e = check_net(c)) return e;
  if (a->activation != c->activation) return "actor and critic must have the same activation";
  return nullptr;
}

// an observation normalizer in use (mean != NULL) has every buffer and the net's input dim
const char* check_norm(const zbp_obs_norm* n, int dim) {
  if (!n || !n->mean) return nullptr;
  if (!n->var || !n->std || !n->count) return "obs normalizer: null var / std / count";
  if (n->dim != dim || dim < 1 || dim > 32) return "obs normalizer: dim must be the net's observation dim";
  return nullptr;
}

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// The hidden layers' activation (zbp_net.activation, torch's default constants, the expressions of
// ATen's kernels) and its derivative written from the OUTPUT x = act(z): the backward passes hold only
// the stored X_l. kAct is a compile-time value in the register kernels (the ELU instantiations keep
// their code and register budget); the LDS kernels switch on a uniform runtime value (act_rt / dact_rt).
constexpr float kSeluScale = 1.0507009873554805f, kSeluAlpha = 1.6732632423543772f;
constexpr float kSeluNeg = kSeluScale * kSeluAlpha;
constexpr float kLreluSlope = 0.01f;
template <int kAct>
__device__ __forceinline__ float act_f(float v) {
  if (kAct == ZBP_ACT_RELU) return v > 0.f ? v : 0.f;
  if (kAct == ZBP_ACT_TANH) return tanhf(v);
  if (kAct == ZBP_ACT_SELU) return v > 0.f ? kSeluScale * v : kSeluNeg * (expf(v) - 1.f);
  if (kAct == ZBP_ACT_LRELU) return v > 0.f ? v : kLreluSlope * v;
  return v > 0.f ? v : expf(v) - 1.f;  // ELU(alpha = 1), as ATen's elu kernel
}
template <int kAct>
__device__ __forceinline__ float dact_f(float x) {
  if (kAct == ZBP_ACT_RELU) return x > 0.f ? 1.f : 0.f;
  if (kAct == ZBP_ACT_TANH) return 1.f - x * x;
  if (kAct == ZBP_ACT_SELU) return x > 0.f ? kSeluScale : x + kSeluNeg;  // lambda alpha exp(z) = x + lambda alpha for z <= 0
  if (kAct == ZBP_ACT_LRELU) return x > 0.f ? 1.f : kLreluSlope;
  return x > 0.f ? 1.f : x + 1.f;  // ELU'(z) = exp(z) = x + 1 for z <= 0
}
// The one switch over the activations: f(std::integral_constant<int, ZBP_ACT_*>) for a runtime value.
// The LDS kernels' act_rt / dact_rt and the host's choice of a register-kernel instantiation go through it.
template <class F>
__host__ __device__ __forceinline__ auto with_act(int act, F&& f) {
  switch (act) {
    case ZBP_ACT_RELU: return f(std::integral_constant<int, ZBP_ACT_RELU>{});
    case ZBP_ACT_TANH: return f(std::integral_constant<int, ZBP_ACT_TANH>{});
    case ZBP_ACT_SELU: return f(std::integral_constant<int, ZBP_ACT_SELU>{});
    case ZBP_ACT_LRELU: return f(std::integral_constant<int, ZBP_ACT_LRELU>{});
    default: return f(std::integral_constant<int, ZBP_ACT_ELU>{});
  }
}
__device__ __forceinline__ float act_rt(int act, float v) {
  return with_act(act, [v](auto a) { return act_f<decltype(a)::value>(v); });
}
__device__ __forceinline__ float dact_rt(int act, float x) {
  return with_act(act, [x](auto a) { return dact_f<decltype(a)::value>(x); });
}

// ---- the PPO arithmetic, each formula stated once (every row / act kernel calls these; the reductions
// over actions and rows stay in the kernels)
constexpr float kLog2Pi = 0.91893853320467274178f;  // log(sqrt(2 pi))
// the Gaussian's sigma and log sigma of one action from the noise parameter p: sigma itself
// (zbp_loss_cfg.log_std == 0), or log sigma (rsl_rl noise_std_type "log": sigma = exp(p), log sigma = p)
__device__ __forceinline__ void sigma_of(float p, int log_std, float& s, float& ls) {
  if (log_std) { s = expf(p); ls = p; }
  else { s = p; ls = logf(p); }
}
// one action's term of the Gaussian log-probability, d = action - mu
__device__ __forceinline__ float logp_term(float d, float s, float ls) { return -(d * d) / (2.f * (s * s)) - ls - kLog2Pi; }
// one action's term of KL(old || new) as rsl_rl writes it: old (om, os) from the storage, new (mu, s)
__device__ __forceinline__ float kl_term(float mu, float s, float om, float os) {
  return logf(s / os + 1e-5f) + (os * os + (om - mu) * (om - mu)) / (2.f * (s * s)) - 0.5f;
}
// a row's clipped surrogate max(-adv ratio, -adv clamp(ratio)) and g = dL / dlog_prob of its mean over the batch
__device__ __forceinline__ void surrogate(float ratio, float adv, float clip, float invB, float& surr, float& g) {
  const float rc = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip);
  const float s1 = -adv * ratio, s2 = -adv * rc;
  surr = fmaxf(s1, s2);
  // d max(s1, s2) / d ratio (torch.max splits a tie evenly; clamp passes the gradient inside
  // [1 - clip, 1 + clip], bounds included)
  const float in = (ratio >= 1.f - clip && ratio <= 1.f + clip) ? 1.f : 0.f;
  const float w1 = s1 > s2 ? 1.f : (s1 < s2 ? 0.f : 0.5f);
  g = (w1 * -adv + (1.f - w1) * -adv * in) * ratio * invB;
}
// one action's dL / dmu and its row's term of dL / dsigma from g = dL / dlog_prob, diff = action - mu
__device__ __forceinline__ void gauss_grad(float g, float diff, float s, float& dmu, float& dsig) {
  dmu = g * diff / (s * s);
  dsig = g * (diff * diff / (s * s * s) - 1.f / s);
}
// a row's value loss (clipped around the stored value tv, or plain) and dv = dL / dvalue of its weighted batch mean
__device__ __forceinline__ void value_loss(float v, float tv, float ret, const zbp_loss_cfg& lc, float invB, float& vl,
                                           float& dv) {
  if (lc.use_clipped_value_loss) {
    const float clip = lc.clip_param, vd = v - tv;
    const float vc = tv + fminf(fmaxf(vd, -clip), clip);
    const float ea = (v - ret) * (v - ret), ec = (vc - ret) * (vc - ret);
    vl = fmaxf(ea, ec);
    const float wa = ea > ec ? 1.f : (ea < ec ? 0.f : 0.5f);  // (a tie split evenly, the clamp's bounds included, as above)
    const float in = (vd >= -clip && vd <= clip) ? 1.f : 0.f;
    dv = wa * 2.f * (v - ret) + (1.f - wa) * 2.f * (vc - ret) * in;
  } else {
    vl = (ret - v) * (ret - v);
    dv = 2.f * (v - ret);
  }
  dv *= lc.value_loss_coef * invB;
}

// C[32 rows][32 cols] = sum_k A[r][k] B[k][c] over k < kp (kp a multiple of 32): A row-major in LDS
// (row stride sa floats), B given as the 32 rows m[(c0 + c) * ldm + k] of a row-major global matrix
// (the reduction index contiguous, L2-resident). Lane (c = lane & 31, h = lane >> 5) feeds
// A[c][.] / B[.][c] on the reduction indices [h kp / 2, (h + 1) kp / 2) (the MFMA's k = 0 / 1
// halves). The B stream runs 16 MFMAs (four float4) ahead of its use: one wave per SIMD has no
// other wave to cover an L2 round trip.
__device__ __forceinline__ f32x16 tile_mma(const float* __restrict__ a, int sa, const float* __restrict__ m, int ldm,
                                           int kp, int c0) {
  const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5, half = kp >> 1;
  const float* ar = a + c * sa + h * half;
  const float4* br = reinterpret_cast<const float4*>(m + (int64_t)(c0 + c) * ldm + h * half);
  const int nq = half >> 2;  // float4 steps (>= 4)
  f32x16 acc = {};
  float4 b0 = br[0], b1 = br[1], b2 = br[2], b3 = br[3];
  for (int q = 0; q < nq; q += 4) {
    const float4 a0 = *reinterpret_cast<const float4*>(ar + 4 * q);
    const float4 a1 = *reinterpret_cast<const float4*>(ar + 4 * q + 4);
    const float4 a2 = *reinterpret_cast<const float4*>(ar + 4 * q + 8);
    const float4 a3 = *reinterpret_cast<const float4*>(ar + 4 * q + 12);
    const float4 u0 = b0, u1 = b1, u2 = b2, u3 = b3;
    if (q + 4 < nq) { b0 = br[q + 4]; b1 = br[q + 5]; b2 = br[q + 6]; b3 = br[q + 7]; }
    acc = mfma(a0.x, u0.x, acc); acc = mfma(a0.y, u0.y, acc); acc = mfma(a0.z, u0.z, acc); acc = mfma(a0.w, u0.w, acc);
    acc = mfma(a1.x, u1.x, acc); acc = mfma(a1.y, u1.y, acc); acc = mfma(a1.z, u1.z, acc); acc = mfma(a1.w, u1.w, acc);
    acc = mfma(a2.x, u2.x, acc); acc = mfma(a2.y, u2.y, acc); acc = mfma(a2.z, u2.z, acc); acc = mfma(a2.w, u2.w, acc);
    acc = mfma(a3.x, u3.x, acc); acc = mfma(a3.y, u3.y, acc); acc = mfma(a3.z, u3.z, acc); acc = mfma(a3.w, u3.w, acc);
  }
  return acc;
}
// row / column of accumulator register r of a 32x32 MFMA tile in this lane: registers 4q .. 4q + 3
// hold rows 8q + 4h .. 8q + 4h + 3 of column lane & 31
__device__ __forceinline__ int acc_row(int r) { return (r & 3) + 8 * (r >> 2) + 4 * ((threadIdx.x & 63) >> 5); }
__device__ __forceinline__ int acc_col() { return threadIdx.x & 31; }

// ------------------------------------------------------------------------------- k_pack
struct PackArgs {
  NetW n[2];
  const float* w[2][MAXL];
  const float* b[2][MAXL];
  float* ws;
  // zbp_optimizer_step's tail (tail != 0; one thread): the new learning rate and step counter, which
  // every k_adam workgroup read as the old ones (so written after that launch), and the loss sums
  int tail, n_params;
  float* lr;
  const float* stats;
  float* acc;
  float desired_kl;
  float* step[ZBP_MAX_PARAMS];
  uint32_t* rng;  // the workspace's noise draw counter: +1 per launch (one thread)
};
__device__ __forceinline__ float adaptive_lr(float lr, float kl, float desired_kl) {
  // rsl_rl's adaptive schedule on the minibatch KL
  if (desired_kl > 0.f) {
    if (kl > desired_kl * 2.f) lr = fmaxf(lr / 1.5f, 1e-5f);
    else if (kl > 0.f && kl < desired_kl / 2.f) lr = fminf(lr * 1.5f, 1e-2f);
  }
  return lr;
}
__global__ void k_pack(PackArgs A) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) *A.rng += 1u;
  if (A.tail && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
    *A.lr = adaptive_lr(*A.lr, A.stats[0], A.desired_kl);
    const float step = A.step[0][0] + 1.f;
    for (int t = 0; t < A.n_params; ++t) A.step[t][0] = step;
    A.acc[0] += A.stats[1];
    A.acc[1] += A.stats[2];
    A.acc[2] += A.stats[3];
  }
  const int net = blockIdx.y, l = blockIdx.z;
  const NetW& w = A.n[net];
  if (l >= w.L) return;
  const int P0 = w.p[l], P1 = w.p[l + 1], D0 = w.d[l], D1 = w.d[l + 1];
  float* wp = A.ws + w.wp[l];
  float* wt = A.ws + w.wt[l];
  float* wr = A.ws + w.wr[l];
  float* wtr = A.ws + w.wtr[l];
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < P0 * P1; e += gridDim.x * blockDim.x) {
    const int n = e / P0, k = e % P0;
    const float v = (n < D1 && k < D0) ? A.w[net][l][n * D0 + k] : 0.f;
    wp[e] = v;
    wt[k * P1 + n] = v;
    // k_rows_reg's A operands (v_mfma_f32_16x16x4_f32): 16 x 16 blocks in its order (reduction
    // tile outer, output tile inner); in a block, lane (output index & 15) + 16 g holds the four
    // reduction indices 4 g + u as one float4 (a block is one contiguous KB: conflict-free
    // ds_read_b128 from the LDS copy)
    {
      const int T1h = P1 / 16, T0h = P0 / 16;
      wr[(int64_t)((k >> 4) * T1h + (n >> 4)) * 256 + ((n & 15) + 16 * ((k >> 2) & 3)) * 4 + (k & 3)] = v;
      wtr[(int64_t)((n >> 4) * T0h + (k >> 4)) * 256 + ((k & 15) + 16 * ((n >> 2) & 3)) * 4 + (n & 3)] = v;
    }
  }
  if (blockIdx.x == 0)
    for (int n = threadIdx.x; n < P1; n += blockDim.x) A.ws[w.bp[l] + n] = n < D1 ? A.b[net][l][n] : 0.f;
}

// ------------------------------------------------------------------------------- k_rows
// Row buffers in HBM are feature-major (X_l [p(l)][B], dZ_l [p(l+1)][B]): a row tile writes whole
// 128-byte lines (32 rows of one feature) as float4 quads of rows, and k_wgrad streams float4 quads
// of rows per lane. In LDS the tile's activations are row-major [32][P + 4]; the backward pass
// writes dZ_{l-1} over X_l in place (each element read once by the thread that overwrites it).
struct RowArgs {
  NetW n[2];
  zbp_batch bt;
  zbp_loss_cfg lc;
  const float* std_param;
  float* ws;
  int64_t stats;
  int B;
  int lds_x[MAXL], lds_dz, lds_out, lds_red;  // LDS float offsets
  // zbp_symmetry on (the kSym kernels only): 1 / rows the losses average, the mirror term's factor
  // mirror_coef 2 / (B num_actions) (0 without mirror_loss), the per-tile squared-error sums
  float sym_inv_loss, sym_grad;
  int64_t sym_part;
};

// ---- zbp_symmetry in the row kernels. Kernel row kr of a tile of TS rows: the tile's first TS / 2 rows are
// originals, the others their mirrors; both are sample (kr / TS) (TS / 2) + (kr mod TS / 2) of the minibatch
template <int TS>
__device__ __forceinline__ int sym_sample(int kr) { return (kr / TS) * (TS / 2) + (kr & (TS / 2 - 1)); }
template <int TS>
__device__ __forceinline__ bool sym_mirrored(int kr) { return (kr & (TS - 1)) >= TS / 2; }
// column k of a row x under the map (perm, sign) when mirrored, x[k] itself otherwise (a perm entry
// outside [0, dim) is clamped: never an out-of-bounds read)
__device__ __forceinline__ float sym_at(const float* x, int k, int dim, bool mir, const int32_t* perm, const float* sign) {
  if (!mir) return x[k];
  const int p = min(max(perm[k], 0), dim - 1);
  return sign[k] * x[p];
}
// a row's weight in the surrogate and the value loss: mirrored rows count only under augmentation
__device__ __forceinline__ float sym_loss_weight(const zbp_symmetry& sy, bool mir) { return (mir && !sy.augment) ? 0.f : 1.f; }

// forward through one net for the row tile; the output layer's pre-activations land in `out`
// ([32][33]). kStore: every hidden layer's input X_l also goes to the HBM row buffers (feature-major,
// B rows) for the weight gradients; the rollout's forward (k_act) keeps them in LDS only.
template <bool kStore>
__device__ void net_forward_t(const NetW& w, float* ws, int B, const int* lds_x, int lds_out, float* lds, int row0) {
  const int wave = threadIdx.x >> 6, h = (threadIdx.x & 63) >> 5, nw = blockDim.x >> 6;
  for (int l = 0; l < w.L; ++l) {
    const int P0 = w.p[l], P1 = w.p[l + 1];
    const bool last = l == w.L - 1;
    const float* xs = lds + lds_x[l];
    const float* wp = ws + w.wp[l];
    const float* bp = ws + w.bp[l];
    for (int t = wave; t < P1 / 32; t += nw) {
      const f32x16 acc = tile_mma(xs, P0 + 4, wp, P0, P0, 32 * t);
      const int n = 32 * t + acc_col();
      const float bias = bp[n];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = 8 * q + 4 * h + u;
          v[u] = acc[4 * q + u] + bias;
          if (last) {
            lds[lds_out + i * 33 + n] = v[u];
          } else {
            v[u] = act_rt(w.act, v[u]);
            lds[lds_x[l + 1] + i * (P1 + 4) + n] = v[u];
          }
        }
        if (kStore && !last)
          *reinterpret_cast<float4*>(ws + w.x[l + 1] + rbo(P1, n, row0 + 8 * q + 4 * h)) =
              make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    __syncthreads();
  }
}
__device__ void net_forward(const RowArgs& A, const NetW& w, float* lds, int row0) {
  net_forward_t<true>(w, A.ws, A.B, A.lds_x, A.lds_out, lds, row0);
}

// backward through one net from dZ of the output layer (lds_dz, [32][p(L) + 4])
__device__ void net_backward(const RowArgs& A, const NetW& w, float* lds, int row0) {
  const int wave = threadIdx.x >> 6, h = (threadIdx.x & 63) >> 5, nw = blockDim.x >> 6;
  for (int l = w.L - 1; l >= 1; --l) {
    const int P0 = w.p[l], P1 = w.p[l + 1];
    const float* dz = lds + (l == w.L - 1 ? A.lds_dz : A.lds_x[l + 1]);
    float* xs = lds + A.lds_x[l];  // X_l, overwritten by dZ_{l-1}
    const float* wt = A.ws + w.wt[l];
    for (int t = wave; t < P0 / 32; t += nw) {
      const f32x16 acc = tile_mma(dz, P1 + 4, wt, P1, P1, 32 * t);
      const int k = 32 * t + acc_col();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = 8 * q + 4 * h + u;
          const float x = xs[i * (P0 + 4) + k];
          g[u] = acc[4 * q + u] * dact_rt(w.act, x);
          xs[i * (P0 + 4) + k] = g[u];
        }
        *reinterpret_cast<float4*>(A.ws + w.dz[l - 1] + rbo(P0, k, row0 + 8 * q + 4 * h)) =
            make_float4(g[0], g[1], g[2], g[3]);
      }
    }
    __syncthreads();
  }
}

// EmpiricalNormalization.forward on column k < dim of a gathered input row (zbp_obs_norm; a division,
// as torch's (x - mean) / (std + eps))
__device__ __forceinline__ float obs_normalize(const zbp_obs_norm& nr, int k, float v) {
  return (v - nr.mean[k]) / (nr.std[k] + nr.eps);
}

// gather the tile's input rows (obs or critic obs) into X_0 (LDS + HBM), zero-padded; normalized
// when the net has a normalizer (nr.mean != NULL)
// (kSym: the tile's rows 16 .. 31 are the mirrors of rows 0 .. 15 under (perm, sign), mapped before the normalizer)
template <bool kSym>
__device__ __forceinline__ void gather_input(const RowArgs& A, const NetW& w, const float* src, int dim, const zbp_obs_norm& nr,
                                             float* lds, int row0, const int32_t* perm = nullptr, const float* sign = nullptr) {
  const int P0 = w.p[0];
  for (int e = threadIdx.x; e < TR * P0; e += blockDim.x) {
    const int k = e / TR, i = e % TR;
    const int64_t row = A.bt.idx[A.bt.idx_offset + (kSym ? sym_sample<TR>(row0 + i) : row0 + i)];
    float v = k < dim ? (kSym ? sym_at(src + row * dim, k, dim, sym_mirrored<TR>(i), perm, sign) : src[row * dim + k]) : 0.f;
    if (nr.mean && k < dim) v = obs_normalize(nr, k, v);
    lds[A.lds_x[0] + i * (P0 + 4) + k] = v;
    A.ws[w.x[0] + rbo(P0, k, row0 + i)] = v;
  }
  __syncthreads();
}

__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <bool kSym>
__device__ __forceinline__ void rows_body(const RowArgs& A, float* lds) {
  const int row0 = blockIdx.x * TR;
  const int tid = threadIdx.x;
  const zbp_batch& bt = A.bt;
  const zbp_symmetry& sy = bt.symmetry;
  const int NA = bt.num_actions;
  const float invB = kSym ? A.sym_inv_loss : 1.f / (float)bt.batch;
  float* red = lds + A.lds_red;  // [NSTAT] per-tile sums
  if (tid < NSTAT) red[tid] = 0.f;

  // ---- actor: forward, Gaussian log-prob, clipped surrogate, KL; dL/dmu into dZ of the output
  const NetW& wa = A.n[0];
  gather_input<kSym>(A, wa, bt.obs, bt.obs_dim, bt.actor_norm, lds, row0, sy.obs_perm, sy.obs_sign);
  net_forward(A, wa, lds, row0);
  {
    float* dz = lds + A.lds_dz;
    const int Pout = wa.p[wa.L];
    float surr = 0.f, kl = 0.f, sg[NSTAT - 3], se = 0.f;
#pragma unroll
    for (int a = 0; a < NSTAT - 3; ++a) sg[a] = 0.f;
    if (tid < TR) {
      const int i = tid;
      const bool mir = kSym && sym_mirrored<TR>(i);
      const float wl = kSym ? sym_loss_weight(sy, mir) : 1.f;
      const int64_t row = bt.idx[bt.idx_offset + (kSym ? sym_sample<TR>(row0 + i) : row0 + i)];
      const float* arow = bt.actions + row * NA;
      float lp = 0.f;
      for (int a = 0; a < NA; ++a) {
        const float mu = lds[A.lds_out + i * 33 + a];
        float s, ls;
        sigma_of(A.std_param[a], A.lc.log_std, s, ls);
        lp += logp_term((kSym ? sym_at(arow, a, NA, mir, sy.act_perm, sy.act_sign) : arow[a]) - mu, s, ls);
        if (!mir) kl += kl_term(mu, s, bt.mu[row * NA + a], bt.sigma[row * NA + a]);  // (the KL: originals only)
      }
      float g;
      surrogate(expf(lp - bt.log_prob[row]), bt.advantages[row], A.lc.clip_param, kSym ? wl * invB : invB, surr, g);
      if (kSym) surr *= wl;
      for (int a = 0; a < Pout; ++a) {
        float d = 0.f;
        if (a < NA) {
          const float mu = lds[A.lds_out + i * 33 + a];
          float s, ls, ds;
          sigma_of(A.std_param[a], A.lc.log_std, s, ls);
          gauss_grad(g, (kSym ? sym_at(arow, a, NA, mir, sy.act_perm, sy.act_sign) : arow[a]) - mu, s, d, ds);
#pragma unroll
          for (int b = 0; b < NSTAT - 3; ++b)
            if (b == a) sg[b] = ds;
          if (mir) {
            // the mirror term: this row's mean against the mapped mean of its original (row i - 16 of the
            // output tile), a constant; its gradient stays in this row
            const float e = mu - sym_at(lds + A.lds_out + (i - TR / 2) * 33, a, NA, true, sy.act_perm, sy.act_sign);
            se += e * e;
            d += A.sym_grad * e;
          }
        }
        dz[i * (Pout + 4) + a] = d;
        A.ws[wa.dz[wa.L - 1] + rbo(Pout, a, row0 + i)] = d;
      }
    }
    if (tid < 64) {
      surr = wave_sum(surr);
      kl = wave_sum(kl);
      if (kSym) {
        se = wave_sum(se);
        if (tid == 0) A.ws[A.sym_part + blockIdx.x] = se;
      }
#pragma unroll
      for (int a = 0; a < NSTAT - 3; ++a) sg[a] = wave_sum(sg[a]);
      if (tid == 0) {
        red[0] = surr;
        red[2] = kl;
#pragma unroll
        for (int a = 0; a < NSTAT - 3; ++a) red[3 + a] = sg[a];
      }
    }
    __syncthreads();
  }
  net_backward(A, wa, lds, row0);

  // ---- critic: forward, clipped value loss, backward
  const NetW& wc = A.n[1];
  gather_input<kSym>(A, wc, bt.critic_obs, bt.critic_obs_dim, bt.critic_norm, lds, row0, sy.critic_perm, sy.critic_sign);
  net_forward(A, wc, lds, row0);
  {
    float* dz = lds + A.lds_dz;
    const int Pout = wc.p[wc.L];
    float vl = 0.f;
    if (tid < TR) {
      const int i = tid;
      const float wl = kSym ? sym_loss_weight(sy, sym_mirrored<TR>(i)) : 1.f;
      const int64_t row = bt.idx[bt.idx_offset + (kSym ? sym_sample<TR>(row0 + i) : row0 + i)];
      float dv;
      value_loss(lds[A.lds_out + i * 33], bt.values[row], bt.returns[row], A.lc, kSym ? wl * invB : invB, vl, dv);
      if (kSym) vl *= wl;
      for (int a = 0; a < Pout; ++a) {
        dz[i * (Pout + 4) + a] = a == 0 ? dv : 0.f;
        A.ws[wc.dz[wc.L - 1] + rbo(Pout, a, row0 + i)] = a == 0 ? dv : 0.f;
      }
    }
    if (tid < 64) {
      vl = wave_sum(vl);
      if (tid == 0) red[1] = vl;
    }
    __syncthreads();
  }
  net_backward(A, wc, lds, row0);
  if (tid < NSTAT) A.ws[A.stats + (int64_t)blockIdx.x * NSTAT + tid] = red[tid];
}
__global__ __launch_bounds__(ROW_THREADS) void k_rows(RowArgs A) {
  extern __shared__ float lds[];
  rows_body<false>(A, lds);
}
// (zbp_symmetry on: 16 originals + their 16 mirrors per tile)
__global__ __launch_bounds__(ROW_THREADS) void k_rows_sym(RowArgs A) {
  extern __shared__ float lds[];
  rows_body<true>(A, lds);
}

// ------------------------------------------------------------------------------- k_rows_reg
// k_rows for the shipped net shapes (three hidden layers of 16 T1, 16 T2, 16 T3 units, inputs and
// outputs <= 32: rsl_rl's [128, 128, 128] and the stand-up / v2 [256, 256, 128]), one WAVE per 16-row
// tile and the activations in registers. A layer is the transposed product Z^T = W X^T on
// v_mfma_f32_16x16x4_f32 with the weights as the A operand and the activations as the B operand
// straight from the previous layer's accumulators: an accumulator tile (4 registers) holds, in lane
// (row r = lane & 15, g = lane >> 4), register u, feature 4 g + u of row r -- exactly the B operand
// of 4 MFMAs whose reduction index runs over the tile's 16 features. A 256-wide layer keeps 16 input
// + 16 output tiles (128 registers) live, so two waves share each SIMD and cover each other's
// epilogues (bias, ELU, the row-buffer stores) and memory waits. The workgroup's four waves share
// the weights through LDS (double-buffered 32 KB chunks of 32 blocks, one barrier per chunk). X_l
// and dZ_l go to HBM octet-blocked (rbo) for k_wgrad; the backward pass reads X_l back for the
// activation's derivative (written from the output, dact_f). kAct: the activation, a compile-time value.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef f32x4 Tile;

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int rr_g() { return (threadIdx.x & 63) >> 4; }
// row buffers (rbo): element (feature 16 o + 4 g + u, row row0 + r) of a P-feature buffer at
// base = buffer + rbo(P, 0, row0) as base[uniform part (16 o + u) 8] + lane part
// ((r >> 3) P 8 + 32 g + (r & 7)): the uniform part stays scalar, the lane part one VGPR offset
__device__ __forceinline__ int rr_lane_off(int P) {
  const int r = threadIdx.x & 15;
  return (r >> 3) * P * 8 + 32 * rr_g() + (r & 7);
}
__device__ __forceinline__ float* rr_base(float* buf, int P, int row0) { return buf + (int64_t)(row0 >> 3) * P * 8; }
__device__ __forceinline__ float* rr_at(float* base, int o, int u) { return base + (16 * o + u) * 8; }

// out[o] = sum_i A(o, i) in[i] over the blocks of a lane-ordered image: block b = (i, o) (reduction
// tile outer: consecutive blocks feed different accumulators) = one float4 per lane, the A operands
// of 4 MFMAs whose B operands are in[i]'s registers, read from the workgroup's LDS copy of the
// current chunk while the next chunk is in flight from L2.
// CB = blocks per chunk: 32 (32 KB chunks, 64 KB of LDS per workgroup: two workgroups per CU) for
// the 256-wide nets; 16 for the 128-wide ones, whose waves fit three to a SIMD (168 registers) and
// whose three workgroups per CU then need 32 KB of LDS each
constexpr int RR_WG = 256;                    // threads per workgroup (4 waves, 4 row tiles)
template <int T1> constexpr int rr_cb() { return T1 <= 8 ? 16 : 32; }
template <int T1> constexpr int rr_occ() { return T1 <= 8 ? 3 : 2; }
template <int CB> using RrStage = float4[CB * 64 / RR_WG];  // this thread's share of a chunk in flight
// chunk `chunk` of an image of NB blocks into the thread's stage registers (zero past the end)
template <int NB, int CB>
__device__ __forceinline__ void rr_fetch(const float* __restrict__ img, int chunk, RrStage<CB>& st) {
  constexpr int NF = NB * 64, PER = CB * 64 / RR_WG;
  const float4* g = reinterpret_cast<const float4*>(img);
#pragma unroll
  for (int m = 0; m < PER; ++m) {
    const int e = chunk * CB * 64 + threadIdx.x + m * RR_WG;
    if (chunk * CB * 64 + m * RR_WG < NF) st[m] = e < NF ? g[e] : float4{};
  }
}
// out[o] = sum_i A(o, i) in[i]; st holds the image's chunk 0 on entry (the caller fetched it, ahead of
// its own epilogue stores: a wait for the weights never waits for those stores to drain)
template <int TI, int TO, int CB>
__device__ __forceinline__ void rr_layer(const float* __restrict__ img, float4* __restrict__ wl, const Tile (&in)[TI],
                                         Tile (&out)[TO], RrStage<CB>& st) {
  constexpr int NB = TI * TO, NC = (NB + CB - 1) / CB;
  constexpr int NF = NB * 64, RR_PER = CB * 64 / RR_WG;
  const int t = threadIdx.x, lane = t & 63;
#pragma unroll
  for (int o = 0; o < TO; ++o) out[o] = Tile{};
#pragma unroll
  for (int m = 0; m < RR_PER; ++m)
    if (m * RR_WG < NF) wl[t + m * RR_WG] = st[m];
  __syncthreads();
  if (NC > 1) rr_fetch<NB, CB>(img, 1, st);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const float4* cb = wl + (c & 1) * CB * 64 + lane;
#pragma unroll
    for (int bb = 0; bb < CB; ++bb) {
      const int b = c * CB + bb;
      if (b < NB) {
        const int i = b / TO, o = b % TO;
        const float4 w = cb[bb * 64];
        Tile a = out[o];
        a = mfma16(w.x, in[i][0], a);
        a = mfma16(w.y, in[i][1], a);
        a = mfma16(w.z, in[i][2], a);
        a = mfma16(w.w, in[i][3], a);
        out[o] = a;
      }
    }
    if (c + 1 < NC) {
      float4* nb = wl + ((c + 1) & 1) * CB * 64;
#pragma unroll
      for (int m = 0; m < RR_PER; ++m)
        if ((c + 1) * CB * 64 + m * RR_WG < NF) nb[t + m * RR_WG] = st[m];
    }
    __syncthreads();  // chunk c consumed by every wave, chunk c + 1 in LDS
    if (c + 2 < NC) rr_fetch<NB, CB>(img, c + 2, st);
  }
}

// forward layer l: + bias, the activation kAct (hidden layers: also X_{l+1} to HBM)
// (NBN > 0: the next layer's image `next` has NBN blocks; its chunk 0 is fetched before this epilogue)
template <int TI, int TO, bool kLast, bool kStore, int NBN, int CB, int kAct>
__device__ __forceinline__ void rr_forward(const NetW& w, int l, float* __restrict__ ws, float4* __restrict__ wl, int row0,
                                           const Tile (&in)[TI], Tile (&out)[TO], RrStage<CB>& st, const float* next) {
  const int lo = rr_lane_off(16 * TO);
  rr_layer<TI, TO, CB>(ws + w.wr[l], wl, in, out, st);
  if (NBN > 0) rr_fetch<NBN, CB>(next, 0, st);
  const float* bp = ws + w.bp[l] + 4 * rr_g();
  float* xb = rr_base(ws + w.x[l + 1], 16 * TO, row0);
#pragma unroll
  for (int o = 0; o < TO; ++o) {
    const float4 bq = *reinterpret_cast<const float4*>(bp + 16 * o);
    const float bv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float v = out[o][u] + bv[u];
      if (!kLast) {
        v = act_f<kAct>(v);
        if (kStore) rr_at(xb, o, u)[lo] = v;
      }
      out[o][u] = v;
    }
  }
}

// backward through layer l >= 1: dZ_{l-1} = (W_l^T dZ_l) * act'(X_l) (from the output, dact_f), to registers and HBM
template <int TI, int TO, int NBN, int CB, int kAct>
__device__ __forceinline__ void rr_backward(const NetW& w, int l, float* __restrict__ ws, float4* __restrict__ wl, int row0,
                                            const Tile (&dz)[TI], Tile (&out)[TO], RrStage<CB>& st, const float* next) {
  const int lo = rr_lane_off(16 * TO);
  float* xb = rr_base(ws + w.x[l], 16 * TO, row0);
  float* db = rr_base(ws + w.dz[l - 1], 16 * TO, row0);
  // X_l for ELU': loaded ahead of the product where the registers allow (its latency then hides
  // under the MFMAs; the 256 x 256 layer has no room at two waves per SIMD and loads it after)
  constexpr int NPRE = TI + 2 * TO <= 40 ? TO : TO / 2;  // tiles of X_l loaded ahead
  Tile xl[TO];
#pragma unroll
  for (int o = 0; o < NPRE; ++o)
#pragma unroll
    for (int u = 0; u < 4; ++u) xl[o][u] = rr_at(xb, o, u)[lo];
  rr_layer<TI, TO, CB>(ws + w.wtr[l], wl, dz, out, st);
  if (NBN > 0) rr_fetch<NBN, CB>(next, 0, st);
#pragma unroll
  for (int o = 0; o < TO; ++o)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float x = o < NPRE ? xl[o][u] : rr_at(xb, o, u)[lo];
      const float gr = out[o][u] * dact_f<kAct>(x);
      out[o][u] = gr;
      rr_at(db, o, u)[lo] = gr;
    }
}

// the tile's input rows (through the permutation) as the first layer's B operand, zero-padded to 32
// (kNorm: normalized when the net has a normalizer; the register kernels are instantiated without it
// for nets that have none, so those keep their code and register budget)
// x[o][u] = feature 16 o + 4 g + u of the input row sr (ok: the row exists), normalized; st != nullptr
// (the rollout's storage slot) gets the row as read
// (kSym: a mirrored row reads through the signed permutation (perm, sign), before the normalizer)
template <bool kNorm, bool kSym = false>
__device__ __forceinline__ void rr_input(const float* sr, int dim, const zbp_obs_norm& nr, bool ok, Tile (&x)[2], float* st,
                                         bool mir = false, const int32_t* perm = nullptr, const float* sign = nullptr) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = 16 * (j >> 2) + 4 * rr_g() + (j & 3);
    const bool in = ok && k < dim;
    const float v = in ? (kSym ? sym_at(sr, k, dim, mir, perm, sign) : sr[k]) : 0.f;
    x[j >> 2][j & 3] = (kNorm && nr.mean && in) ? obs_normalize(nr, k, v) : v;
    if (st && in) st[k] = v;
  }
}
// (the minibatch: the row through the permutation; X_0, normalized, also to its row buffer)
template <bool kNorm, bool kSym = false>
__device__ __forceinline__ void rr_gather(const NetW& w, float* __restrict__ ws, int row0, const float* src, int dim,
                                          const zbp_obs_norm& nr, int64_t row, Tile (&x)[2], bool mir = false,
                                          const int32_t* perm = nullptr, const float* sign = nullptr) {
  const int lo = rr_lane_off(32);
  float* xb = rr_base(ws + w.x[0], 32, row0);
  rr_input<kNorm, kSym>(src + row * dim, dim, nr, true, x, nullptr, mir, perm, sign);
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int u = 0; u < 4; ++u) rr_at(xb, o, u)[lo] = x[o][u];
}

__device__ __forceinline__ void rr_store_dz(const NetW& w, float* __restrict__ ws, int row0, const Tile (&d)[2]) {
  const int lo = rr_lane_off(32);
  float* db = rr_base(ws + w.dz[w.L - 1], 32, row0);
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int u = 0; u < 4; ++u) rr_at(db, o, u)[lo] = d[o][u];
}

// sum over the 16 rows of a wave (lanes with the same g)
__device__ __forceinline__ float rr_row_sum(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
// sum over the 4 feature groups of a row (lanes r, r + 16, r + 32, r + 48)
__device__ __forceinline__ float rr_feat_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// one net's forward, x0 -> z (the output layer's pre-activations). Every layer fetches the next layer's
// first weight chunk before its epilogue; the last one fetches `next`, the backward's first image, in
// the minibatch pass (kStore: X_l also to HBM) and nothing in the rollout's
template <int T1, int T2, int T3, bool kStore, int CB, int kAct>
__device__ __forceinline__ void rr_forward_chain(const NetW& w, float* __restrict__ ws, float4* __restrict__ wl, int row0,
                                                 const Tile (&x0)[2], Tile (&z)[2], RrStage<CB>& st, const float* next) {
  Tile x1[T1], x2[T2], x3[T3];
  rr_forward<2, T1, false, kStore, T1 * T2, CB, kAct>(w, 0, ws, wl, row0, x0, x1, st, ws + w.wr[1]);
  rr_forward<T1, T2, false, kStore, T2 * T3, CB, kAct>(w, 1, ws, wl, row0, x1, x2, st, ws + w.wr[2]);
  rr_forward<T2, T3, false, kStore, T3 * 2, CB, kAct>(w, 2, ws, wl, row0, x2, x3, st, ws + w.wr[3]);
  rr_forward<T3, 2, true, kStore, kStore ? 2 * T3 : 0, CB, kAct>(w, 3, ws, wl, row0, x3, z, st, next);
}
// one net's backward from the output layer's dZ (st holds chunk 0 of W_3^T's image on entry)
template <int T1, int T2, int T3, int CB, int kAct>
__device__ __forceinline__ void rr_backward_chain(const NetW& w, float* __restrict__ ws, float4* __restrict__ wl, int row0,
                                                  const Tile (&dz)[2], RrStage<CB>& st) {
  Tile d3[T3], d2[T2], d1[T1];
  rr_backward<2, T3, T3 * T2, CB, kAct>(w, 3, ws, wl, row0, dz, d3, st, ws + w.wtr[2]);
  rr_backward<T3, T2, T2 * T1, CB, kAct>(w, 2, ws, wl, row0, d3, d2, st, ws + w.wtr[1]);
  rr_backward<T2, T1, 0, CB, kAct>(w, 1, ws, wl, row0, d2, d1, st, nullptr);
}

constexpr int RR_TR = 16;  // rows per wave
// kSym (zbp_symmetry on): the tile's rows 0 .. 7 are originals, rows 8 .. 15 their mirrors; a mirrored row's
// lanes fetch the original's means from lanes (r - 8, any g) with ds_bpermute (the mean of action p sits in
// lane (r, p >> 2), register p & 3 of output tile 0)
template <int T1, int T2, int T3, bool kNorm, int kAct, bool kSym = false>
__global__ __launch_bounds__(RR_WG, rr_occ<T1>()) void k_rows_reg(RowArgs A) {
  constexpr int CB = rr_cb<T1>();
  __shared__ float4 wl[2 * CB * 64];
  const int lane = threadIdx.x & 63, r = lane & 15, gq = lane >> 4;
  // workgroup pairs: even = the actor's pass over four row tiles, odd = the critic's over the same
  // tiles (the two nets share nothing but the tile's statistics slots, which they write apart)
  const int net = blockIdx.x & 1;
  const int tile = (blockIdx.x >> 1) * (RR_WG / 64) + (threadIdx.x >> 6);  // (B a multiple of 64: reg_shape)
  const int row0 = tile * RR_TR;
  const zbp_batch& bt = A.bt;
  const zbp_symmetry& sy = bt.symmetry;
  const int NA = bt.num_actions;
  const float invB = kSym ? A.sym_inv_loss : 1.f / (float)bt.batch;
  const bool mir = kSym && sym_mirrored<RR_TR>(r);
  const float wgt = kSym ? sym_loss_weight(sy, mir) : 1.f;
  const int64_t row = bt.idx[bt.idx_offset + (kSym ? sym_sample<RR_TR>(row0 + r) : row0 + r)];
  float* ws = A.ws;
  float* st = ws + A.stats + (int64_t)tile * NSTAT;
  // the losses' inputs of this lane's row and actions (4 g + u, u < 4: num_actions <= 13 < 16), loaded
  // ahead of the forward passes so their latency hides under them
  const NetW& wa = A.n[0];
  const NetW& wc = A.n[1];
  RrStage<CB> wst;
  Tile z[2], dz[2];
  if (net == 0) {
  const float adv_in = bt.advantages[row], lp_in = bt.log_prob[row];
  float act_in[4], mu_in[4], sig_in[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int n = 4 * gq + u;
    act_in[u] = n < NA ? (kSym ? sym_at(bt.actions + row * NA, n, NA, mir, sy.act_perm, sy.act_sign) : bt.actions[row * NA + n]) : 0.f;
    mu_in[u] = n < NA ? bt.mu[row * NA + n] : 0.f;
    sig_in[u] = n < NA ? bt.sigma[row * NA + n] : 1.f;
  }

  // ---- actor: forward, Gaussian log-prob, clipped surrogate, KL; dL/dmu into dZ of the output
  rr_fetch<2 * T1, CB>(ws + wa.wr[0], 0, wst);
  {
    Tile x0[2];
    rr_gather<kNorm, kSym>(wa, ws, row0, bt.obs, bt.obs_dim, bt.actor_norm, row, x0, mir, sy.obs_perm, sy.obs_sign);
    rr_forward_chain<T1, T2, T3, true, CB, kAct>(wa, ws, wl, row0, x0, z, wst, ws + wa.wtr[3]);
  }
  {
    // lane (r, g) holds actions 4 g + u (tile 0) and 16 + 4 g + u (tile 1) of row r
    float lp = 0.f, kl = 0.f, diff[8], sig[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int n = 16 * (j >> 2) + 4 * gq + (j & 3);
      diff[j] = 0.f;
      sig[j] = 1.f;
      if (n < NA) {
        const float mu = z[j >> 2][j & 3];
        float ls;
        sigma_of(A.std_param[n], A.lc.log_std, sig[j], ls);
        diff[j] = act_in[j & 3] - mu;  // (n < NA only in tile 0: j < 4)
        lp += logp_term(diff[j], sig[j], ls);
        if (!mir) kl += kl_term(mu, sig[j], mu_in[j & 3], sig_in[j & 3]);  // (the KL: originals only)
      }
    }
    lp = rr_feat_sum(lp);
    kl = rr_feat_sum(kl);
    float surr, g;
    surrogate(expf(lp - lp_in), adv_in, A.lc.clip_param, kSym ? wgt * invB : invB, surr, g);
    if (kSym) surr *= wgt;
    // the mirror term (kSym): err[u] = this mirrored row's mean of action 4 g + u minus the mapped mean of its
    // original, a constant (every lane takes part in the exchange; only mirrored rows use the result)
    float err[4] = {0.f, 0.f, 0.f, 0.f};
    if (kSym) {
      float se = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int n = 4 * gq + u;
        const int p = n < NA ? min(max(sy.act_perm[n], 0), NA - 1) : 0;
        const int srcl = (r & 7) + 16 * (p >> 2);
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float c = __shfl(z[0][q], srcl);
          if ((p & 3) == q) t = c;
        }
        if (mir && n < NA) {
          err[u] = z[0][u] - sy.act_sign[n] * t;
          se += err[u] * err[u];
        }
      }
      se = wave_sum(se);
      if (lane == 0) ws[A.sym_part + tile] = se;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int n = 16 * (j >> 2) + 4 * gq + (j & 3);
      float d = 0.f, sg = 0.f;
      if (n < NA) gauss_grad(g, diff[j], sig[j], d, sg);
      if (kSym && j < 4) d += A.sym_grad * err[j];
      dz[j >> 2][j & 3] = d;
      sg = rr_row_sum(sg);  // the std gradient summed over the tile's rows
      if (r == 0 && n < NA) st[3 + n] = sg;
    }
    rr_store_dz(wa, ws, row0, dz);
    const float su = wave_sum(gq == 0 ? surr : 0.f), ks = wave_sum(gq == 0 ? kl : 0.f);
    if (lane == 0) {
      st[0] = su;
      st[2] = ks;
      for (int a = 3 + NA; a < NSTAT; ++a) st[a] = 0.f;
    }
  }
  rr_backward_chain<T1, T2, T3, CB, kAct>(wa, ws, wl, row0, dz, wst);
  } else {
  const float tv_in = bt.values[row], ret_in = bt.returns[row];
  // ---- critic: forward, clipped value loss, backward
  rr_fetch<2 * T1, CB>(ws + wc.wr[0], 0, wst);
  {
    Tile x0[2];
    rr_gather<kNorm, kSym>(wc, ws, row0, bt.critic_obs, bt.critic_obs_dim, bt.critic_norm, row, x0, mir, sy.critic_perm,
                           sy.critic_sign);
    rr_forward_chain<T1, T2, T3, true, CB, kAct>(wc, ws, wl, row0, x0, z, wst, ws + wc.wtr[3]);
  }
  {
    float vl, dv;
    value_loss(__shfl(z[0][0], r), tv_in, ret_in, A.lc, kSym ? wgt * invB : invB, vl, dv);
    if (kSym) vl *= wgt;
#pragma unroll
    for (int j = 0; j < 8; ++j) dz[j >> 2][j & 3] = (gq == 0 && j == 0) ? dv : 0.f;
    rr_store_dz(wc, ws, row0, dz);
    const float vs = wave_sum(gq == 0 ? vl : 0.f);
    if (lane == 0) st[1] = vs;
  }
  rr_backward_chain<T1, T2, T3, CB, kAct>(wc, ws, wl, row0, dz, wst);
  }
}

// ------------------------------------------------------------------------------- k_wgrad
struct WgradArgs {
  NetW n[2];
  TileMap tm;
  int batch;
  float* ws;
  int64_t part;
};
// dW_l = dZ_l^T X_l and db_l = sum dZ_l over the rows of one split. One workgroup = one block of up to
// 128 output rows (n) x 128 reduction columns (k) of one layer; its four waves take 64 x 64 quadrants
// (2 x 2 tiles of 32 x 32, v_mfma_f32_32x32x2_f32). The split's rows stream through LDS in chunks
// of 32 rows (four octets): dZ_l[n0 .. n0 + 127] and X_l[k0 .. k0 + 127] of a chunk are 2 x 4 contiguous
// 4 KB pieces of the octet-blocked row buffers (rbo), copied by all 256 threads into one of two
// buffers while the previous chunk is consumed (one barrier per chunk); every element is read from
// HBM / L2 once per block instead of once per wave. A wave reads its operands as float4 quads of
// rows (conflict-free ds_read_b128: a wave's 64 lanes cover one contiguous KB) and issues 16 MFMAs
// per octet. Partial tiles (and the bias column of the k0 = 0 tiles) go to the workspace in
// k_reduce's layout.
constexpr int WG_CHUNK_F = 2 * 4 * 128 * 8;  // floats of one chunk buffer (dZ + X: 32 KB)
__global__ __launch_bounds__(256, 2) void k_wgrad(WgradArgs A) {
  __shared__ float4 lds4[2 * WG_CHUNK_F / 4];
  float* lds = reinterpret_cast<float*>(lds4);
  // workgroup -> (net, layer) by the launch prefix, then (group, split) inside it, groups interleaved
  const TileMap& M = A.tm;
  int pos = 0;
  while (pos + 1 < 2 * MAXL && M.blk0[pos + 1] <= (int)blockIdx.x) ++pos;
  const int nl = M.ord[pos];
  const int ng = M.grp0[nl + 1] - M.grp0[nl], local = (int)blockIdx.x - M.blk0[pos];
  const int grp = M.grp0[nl] + local % ng, split = local / ng, nsplit = M.sp_nl[nl];
  const NetW& w = A.n[nl / MAXL];
  const int l = nl % MAXL;
  const int P0 = w.p[l], P1 = w.p[l + 1], Tk = P0 / 32, Tn = P1 / 32, KG = (Tk + 3) / 4;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, c = lane & 31, h = lane >> 5;
  const int g = grp - M.grp0[nl], nt0 = 4 * (g / KG), kt0 = 4 * (g % KG);
  const int nb = min(4, Tn - nt0), kb = min(4, Tk - kt0);  // tiles of the block
  const int C = A.batch / 32;  // the split's chunks [c0, c1)
  const int c0 = (int)((int64_t)split * C / nsplit), c1 = (int)((int64_t)(split + 1) * C / nsplit);
  const int r0 = 32 * c0, nch = c1 - c0;
  // chunk copy: per octet, dZ features n0 .. n0 + 32 nb - 1 and X features k0 .. k0 + 32 kb - 1 (8 rows each)
  const int fn = 32 * nb * 8 / 4, fk = 32 * kb * 8 / 4;  // float4s per octet
  const float4* gz = reinterpret_cast<const float4*>(A.ws + w.dz[l] + rbo(P1, 32 * nt0, r0));
  const float4* gx = reinterpret_cast<const float4*>(A.ws + w.x[l] + rbo(P0, 32 * kt0, r0));
  const int64_t oz = (int64_t)P1 * 2, ox = (int64_t)P0 * 2;  // float4 stride of an octet
  // thread t copies float4s t + 256 m, m < 8, of the chunk's 4 x 256 (dZ) + 4 x 256 (X) slots;
  // slot (part, octet o, float4 f = 2 feature + half) -> LDS float4 part 1024 + o 256 + half 128 + feature
  // (a wave's operand read, lane (c, h) at h 128 + feature c: every 16 lanes read 256 contiguous bytes)
  float4 st[8];
  auto fetch = [&](int ch) {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int e = t + 256 * m, part = e >> 10, o = (e >> 8) & 3, f = e & 255;
      const int j = 4 * ch + o;  // octet of the split
      float4 v = float4{};
      if (part == 0) { if (f < fn) v = gz[j * oz + f]; }
      else if (f < fk) v = gx[j * ox + f];
      st[m] = v;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int e = t + 256 * m;
      lds4[buf * (WG_CHUNK_F / 4) + (e & ~255) + (e & 1) * 128 + ((e & 255) >> 1)] = st[m];
    }
  };
  // this wave's quadrant: n tiles 2 (wave >> 1) + {0, 1}, k tiles 2 (wave & 1) + {0, 1}
  const int qn = 2 * (wave >> 1), qk = 2 * (wave & 1);
  const bool on[2][2] = {{qn < nb && qk < kb, qn < nb && qk + 1 < kb}, {qn + 1 < nb && qk < kb, qn + 1 < nb && qk + 1 < kb}};
  const bool any = on[0][0];
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f32x16{};
  float bsum[2] = {0.f, 0.f};
  const bool bias = kt0 == 0 && (wave & 1) == 0;
  fetch(0);
  stash(0);
  __syncthreads();
  if (nch > 1) fetch(1);
  for (int ch = 0; ch < nch; ++ch) {
    const float* bz = lds + (ch & 1) * WG_CHUNK_F;
    const float* bx = bz + 4096;
    if (any) {
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        float4 za[2], xb[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          za[a] = *reinterpret_cast<const float4*>(bz + o * 1024 + (h * 128 + 32 * (qn + a) + c) * 4);
          xb[a] = *reinterpret_cast<const float4*>(bx + o * 1024 + (h * 128 + 32 * (qk + a) + c) * 4);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = mfma(za[a].x, xb[b].x, acc[a][b]);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = mfma(za[a].y, xb[b].y, acc[a][b]);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = mfma(za[a].z, xb[b].z, acc[a][b]);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = mfma(za[a].w, xb[b].w, acc[a][b]);
        if (bias)
#pragma unroll
          for (int a = 0; a < 2; ++a) bsum[a] += (za[a].x + za[a].y) + (za[a].z + za[a].w);
      }
    }
    if (ch + 1 < nch) stash((ch + 1) & 1);
    __syncthreads();  // chunk ch consumed by every wave, chunk ch + 1 in LDS
    if (ch + 2 < nch) fetch(ch + 2);
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const float bs = bsum[a] + __shfl_xor(bsum[a], 32);
#pragma unroll
    for (int b = 0; b < 2; ++b)
      if (on[a][b]) {
        const int nt = nt0 + qn + a, kt = kt0 + qk + b;
        float* out = A.ws + A.part + ((int64_t)split * M.wtiles + M.tile0[nl] + nt * Tk + kt) * PART;
#pragma unroll
        for (int r = 0; r < 16; ++r) out[acc_row(r) * 32 + acc_col()] = acc[a][b][r];  // [n][k]
        if (kt == 0 && h == 0) out[1024 + c] = bs;
      }
  }
}

// ------------------------------------------------------------------------------- k_reduce
struct ReduceArgs {
  NetW n[2];
  TileMap tm;
  int row_tiles, batch, num_actions;
  float* gw[2][MAXL];
  float* gb[2][MAXL];
  const float* std_param;
  float* std_grad;
  float* stats;
  float entropy_coef;
  int log_std;  // std_param holds log sigma (zbp_loss_cfg.log_std)
  const float* ws;
  int64_t part, rstats;
  float* norm2;  // [wtiles + 1]: each tile's sum of squared gradients (the last: the std's), for zbp_optimizer_step
  // zbp_symmetry on (k_reduce_sym only): the samples B the KL averages over, the rows the losses average
  // over (2 B under augmentation), the per-row-tile squared-error sums and the caller's accumulator
  int sym_samples, sym_loss_rows;
  int64_t sym_part;
  float* sym_acc;
};
// one workgroup per weight tile: the split partials summed in order into .grad (weights of the tile,
// and the bias for k0 = 0) and the tile's sum of their squares (fixed order); the last workgroup: the
// scalars. 1024 threads: a thread sums one partial element over the splits with 16 loads in flight
// (with 256 threads and 8 in flight the launch waited on ~30 dependent rounds of partial loads)
constexpr int RED_THREADS = 1024;
template <bool kSym>
__device__ __forceinline__ void reduce_body(const ReduceArgs& A) {
  if (blockIdx.x == (unsigned)A.tm.wtiles) {
    // per-row-tile sums -> stats, the std gradient (+ the entropy bonus term): thread t < 256 sums row
    // tiles t, t + 256, ... (one row = 16 floats = four float4, two rows in flight), then a fixed-order
    // tree over those 256 (deterministic); the other threads only take part in the barriers
    __shared__ float red[256][NSTAT + 1];
    const int t = threadIdx.x;
    float sv[NSTAT];
#pragma unroll
    for (int q = 0; q < NSTAT; ++q) sv[q] = 0.f;
    const float4* rs = reinterpret_cast<const float4*>(A.ws + A.rstats);
    int rt = t < 256 ? t : A.row_tiles;
    for (; rt + 256 < A.row_tiles; rt += 512) {
      float4 v[8];
#pragma unroll
      for (int c = 0; c < 4; ++c) { v[c] = rs[(int64_t)rt * 4 + c]; v[4 + c] = rs[(int64_t)(rt + 256) * 4 + c]; }
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        sv[4 * c] += v[c].x + v[4 + c].x; sv[4 * c + 1] += v[c].y + v[4 + c].y;
        sv[4 * c + 2] += v[c].z + v[4 + c].z; sv[4 * c + 3] += v[c].w + v[4 + c].w;
      }
    }
    for (; rt < A.row_tiles; rt += 256)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float4 v = rs[(int64_t)rt * 4 + c];
        sv[4 * c] += v.x; sv[4 * c + 1] += v.y; sv[4 * c + 2] += v.z; sv[4 * c + 3] += v.w;
      }
    if (t < 256)
#pragma unroll
      for (int q = 0; q < NSTAT; ++q) red[t][q] = sv[q];
    if (kSym && t < 256) {
      // the symmetry loss's per-tile sums, the same way (the spare column of `red`)
      float se = 0.f;
      for (int k = t; k < A.row_tiles; k += 256) se += A.ws[A.sym_part + k];
      red[t][NSTAT] = se;
    }
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (t < st) {
#pragma unroll
        for (int q = 0; q < NSTAT; ++q) red[t][q] += red[t + st][q];
        if (kSym) red[t][NSTAT] += red[t + st][NSTAT];
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      float tot[NSTAT];
      for (int q = 0; q < NSTAT; ++q) tot[q] = red[0][q];
      const float invB = 1.f / (float)(kSym ? A.sym_loss_rows : A.batch);
      float ent = 0.f;
      // (log std: the parameter is log sigma)
      for (int a = 0; a < A.num_actions; ++a)
        ent += 0.5f + kLog2Pi + (A.log_std ? A.std_param[a] : logf(A.std_param[a]));
      if (kSym && A.sym_acc) A.sym_acc[0] += red[0][NSTAT] / ((float)A.sym_samples * (float)A.num_actions);
      A.stats[0] = tot[2] * (kSym ? 1.f / (float)A.sym_samples : invB);  // kl mean (symmetry: over the originals)
      A.stats[1] = tot[1] * invB;  // value loss
      A.stats[2] = tot[0] * invB;  // surrogate loss
      A.stats[3] = ent;            // entropy (every row's)
      float ss = 0.f;
      for (int a = 0; a < A.num_actions; ++a) {
        // tot[3 + a] = dL / d sigma of the surrogate; log std: dL / d log sigma = sigma dL / d sigma, and the
        // entropy bonus -entropy_coef log sigma contributes -entropy_coef
        const float g = A.log_std ? expf(A.std_param[a]) * tot[3 + a] - A.entropy_coef
                                  : tot[3 + a] - A.entropy_coef / A.std_param[a];
        A.std_grad[a] = g;
        ss += g * g;
      }
      A.norm2[A.tm.wtiles] = ss;
    }
    return;
  }
  const int tile = blockIdx.x;
  int nl = 0;
  while (nl + 1 < 2 * MAXL && A.tm.tile0[nl + 1] <= tile) ++nl;
  const int net = nl / MAXL, l = nl % MAXL;
  const NetW& w = A.n[net];
  const int t = tile - A.tm.tile0[nl], kt = w.p[l] / 32;
  const int n0 = 32 * (t / kt), k0 = 32 * (t % kt);
  const int D0 = w.d[l], D1 = w.d[l + 1];
  float ss = 0.f;
  for (int e = threadIdx.x; e < PART; e += blockDim.x) {
    // (sixteen partial sums: sixteen split partials in flight per thread; a fixed order)
    float sv[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) sv[u] = 0.f;
    int sp = 0;
    const float* src = A.ws + A.part + (int64_t)tile * PART + e;
    const int64_t stride = (int64_t)A.tm.wtiles * PART;
    const int nsp = A.tm.sp_nl[nl];  // (this tile's layer's splits)
    for (; sp + 16 <= nsp; sp += 16)
#pragma unroll
      for (int u = 0; u < 16; ++u) sv[u] += src[(int64_t)(sp + u) * stride];
    for (; sp < nsp; ++sp) sv[0] += src[(int64_t)sp * stride];
    float s8[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) s8[u] = sv[u] + sv[u + 8];
    const float s = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
    if (e < 1024) {
      const int n = n0 + e / 32, k = k0 + e % 32;
      if (n < D1 && k < D0) { A.gw[net][l][(int64_t)n * D0 + k] = s; ss += s * s; }
    } else if (k0 == 0) {
      const int n = n0 + e - 1024;
      if (n < D1) { A.gb[net][l][n] = s; ss += s * s; }
    }
  }
  __shared__ float red[RED_THREADS / 64];
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = ss;
  __syncthreads();
  if (threadIdx.x == 0) {
    float v = 0.f;
    for (int k = 0; k < RED_THREADS / 64; ++k) v += red[k];  // fixed order
    A.norm2[tile] = v;
  }
}
__global__ __launch_bounds__(RED_THREADS) void k_reduce(ReduceArgs A) { reduce_body<false>(A); }
__global__ __launch_bounds__(RED_THREADS) void k_reduce_sym(ReduceArgs A) { reduce_body<true>(A); }

// ------------------------------------------------------------------------------- k_optim
struct OptimArgs {
  zbp_params P;
  float* lr;
  const float* stats;
  float* acc;
  float desired_kl, max_norm, b1, b2, eps;
  float* norm2;  // workspace scratch: nparts sums of squares (k_norm's per block or k_reduce's per tile), summed in order by k_adam
  int nparts;
  int64_t total;  // elements over all the tensors
};
// flat element g over the tensors in order -> (tensor t, element e): every thread's elements are
// independent loads (a loop over the tensors per thread would chain one memory round trip per tensor)
__device__ __forceinline__ void flat_elem(const zbp_params& P, int64_t g, int& t, int64_t& e) {
  t = 0;
  while (t + 1 < P.n_params && g >= P.numel[t]) { g -= P.numel[t]; ++t; }
  e = g;
}
__global__ __launch_bounds__(256) void k_norm(OptimArgs A) {
  // global gradient norm^2: per-block partial sums in a fixed order (deterministic)
  __shared__ float red[4];
  float s = 0.f;
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < A.total; f += (int64_t)gridDim.x * blockDim.x) {
    int t;
    int64_t e;
    flat_elem(A.P, f, t, e);
    const float g = A.P.grad[t][e];
    s += g * g;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) A.norm2[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);  // fixed order
}
__global__ __launch_bounds__(256) void k_adam(OptimArgs A) {
  // learning rate rule (rsl_rl adaptive schedule, on the minibatch KL), clip coefficient, Adam
  const float lr = adaptive_lr(*A.lr, A.stats[0], A.desired_kl);
  // the global norm^2 from the partial sums: the first wave loads them lane-parallel and sums with a
  // butterfly (the same fixed order in every block), then shares it through LDS
  __shared__ float n2s;
  if (threadIdx.x < 64) {
    float v = 0.f;
    for (int b = threadIdx.x; b < A.nparts; b += 64) v += A.norm2[b];
    v = wave_sum(v);
    if (threadIdx.x == 0) n2s = v;
  }
  __syncthreads();
  const float total = sqrtf(n2s);
  const float coef = fminf(A.max_norm / (total + 1e-6f), 1.f);
  const float step = A.P.step[0][0] + 1.f;
  const float bc1 = 1.f - powf(A.b1, step), bc2s = sqrtf(1.f - powf(A.b2, step));
  const float step_size = lr / bc1;
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < A.total; f += (int64_t)gridDim.x * blockDim.x) {
    int t;
    int64_t e;
    flat_elem(A.P, f, t, e);
    const float g = A.P.grad[t][e] * coef;
    A.P.grad[t][e] = g;
    const float m = A.b1 * A.P.exp_avg[t][e] + (1.f - A.b1) * g;
    const float v = A.b2 * A.P.exp_avg_sq[t][e] + (1.f - A.b2) * g * g;
    A.P.exp_avg[t][e] = m;
    A.P.exp_avg_sq[t][e] = v;
    A.P.param[t][e] -= step_size * m / (sqrtf(v) / bc2s + A.eps);
  }
  // (every block reads the old lr / step: the k_pack launch after this one writes the new ones)
}

// ------------------------------------------------------------------------------- rollout
// PPO.act (zbot_lab_amd/rl/ppo.py; rsl_rl ActorCritic.act + evaluate + get_actions_log_prob and
// RolloutStorage.add's transition fields) for one policy step of every env: one workgroup per 32
// rows gathers the observations (and writes them into the storage slot), runs the actor forward,
// draws a = mu + std * noise (noise = the caller's torch.randn_like), the Gaussian log-probability
// sum_a (-(a - mu)^2 / (2 std^2) - log std - log sqrt(2 pi)) and the critic's value; every
// transition field lands in the storage slot of this step, the actions also in `actions` (the
// env's input). The forward reads the workspace's weight images (zbp_pack).
struct ActArgs {
  NetW n[2];
  float* ws;
  const float* std_param;
  const float* obs;
  const float* cobs;
  const float* noise;   // the caller's draw, or nullptr: noise_at draws it
  const uint32_t* rng;  // (noise == nullptr) the workspace's draw counter
  int noise_step;
  uint32_t noise_seed;
  int obs_dim, cobs_dim, na, rows;
  int log_std;  // std_param holds log sigma (zbp_act_io.log_std)
  float *actions, *s_obs, *s_cobs, *s_act, *s_val, *s_lp, *s_mu, *s_sig;
  int lds_x[MAXL], lds_out;
  zbp_obs_norm nrm[2];  // the actor's / critic's observation normalizer (mean == nullptr: none)
};
// The in-kernel action noise (zbp_act with io->noise == NULL): a standard normal per (row, action)
// from a counter-based draw -- splitmix64 of (the caller's seed, e.g. per rank; the workspace's draw
// counter, which every k_pack advances, so every rollout and every update; the rollout step; row;
// action), Box-Muller on its
// 24-bit halves. The same distribution as torch.randn, another stream; no launch of its own.
__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
__device__ __forceinline__ float noise_at(const ActArgs& A, int row, int n) {
  if (A.noise) return A.noise[row * A.na + n];
  const uint64_t key = ((uint64_t)A.noise_seed << 32) ^ ((uint64_t)*A.rng << 12) ^ (uint64_t)(uint32_t)A.noise_step;
  const uint64_t h = mix64(mix64(key) ^ (uint64_t)((int64_t)row * A.na + n));
  const float u1 = ((float)(uint32_t)(h >> 40) + 1.f) * 5.9604644775390625e-8f;  // (0, 1]
  const float u2 = (float)(uint32_t)((h >> 16) & 0xFFFFFFu) * 5.9604644775390625e-8f;  // [0, 1)
  return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}
// action n of `row` from the actor's mean: draws a = mu + sigma * noise, writes the transition's four
// per-action fields (the action also into the env's input) and returns the action's log-prob term
__device__ __forceinline__ float sample_action(const ActArgs& A, int64_t row, int n, float mu) {
  float s, ls;
  sigma_of(A.std_param[n], A.log_std, s, ls);
  const float x = mu + s * noise_at(A, row, n), diff = x - mu;
  A.actions[row * A.na + n] = x;
  A.s_act[row * A.na + n] = x;
  A.s_mu[row * A.na + n] = mu;
  A.s_sig[row * A.na + n] = s;
  return logp_term(diff, s, ls);
}

// (the storage slot gets the raw observation, the net the normalized one)
__device__ void act_gather(const NetW& w, const float* src, int dim, const zbp_obs_norm& nr, float* st, int rows,
                           float* lds, int lds_x0, int row0) {
  const int P0 = w.p[0];
  for (int e = threadIdx.x; e < TR * P0; e += blockDim.x) {
    const int i = e / P0, k = e % P0;  // (row-major: the source rows are contiguous)
    const int row = row0 + i;
    const bool in = k < dim && row < rows;
    const float v = in ? src[(int64_t)row * dim + k] : 0.f;
    lds[lds_x0 + i * (P0 + 4) + k] = (in && nr.mean) ? obs_normalize(nr, k, v) : v;
    if (in) st[(int64_t)row * dim + k] = v;
  }
  __syncthreads();
}
__global__ __launch_bounds__(256) void k_act(ActArgs A) {
  extern __shared__ float lds[];
  const int row0 = blockIdx.x * TR, tid = threadIdx.x;
  act_gather(A.n[0], A.obs, A.obs_dim, A.nrm[0], A.s_obs, A.rows, lds, A.lds_x[0], row0);
  net_forward_t<false>(A.n[0], A.ws, 0, A.lds_x, A.lds_out, lds, row0);
  if (tid < TR && row0 + tid < A.rows) {
    const int64_t row = row0 + tid;
    float lp = 0.f;
    for (int a = 0; a < A.na; ++a) lp += sample_action(A, row, a, lds[A.lds_out + tid * 33 + a]);
    A.s_lp[row] = lp;
  }
  __syncthreads();  // (the output tile is reused by the critic)
  act_gather(A.n[1], A.cobs, A.cobs_dim, A.nrm[1], A.s_cobs, A.rows, lds, A.lds_x[0], row0);
  net_forward_t<false>(A.n[1], A.ws, 0, A.lds_x, A.lds_out, lds, row0);
  if (tid < TR && row0 + tid < A.rows) A.s_val[row0 + tid] = lds[A.lds_out + tid * 33];
}

// the register act kernels' input: `row` of the net's observations as the first layer's B operand
// (normalized), the raw row into the storage slot (store: by one wave of the row's workgroup)
template <bool kNorm>
__device__ __forceinline__ void act_rr_gather(const ActArgs& A, int net, int64_t row, bool ok, bool store, Tile (&x0)[2]) {
  const int dim = net ? A.cobs_dim : A.obs_dim;
  float* st = (net ? A.s_cobs : A.s_obs) + row * dim;
  rr_input<kNorm>((net ? A.cobs : A.obs) + row * dim, dim, A.nrm[net], ok, x0, store ? st : nullptr);
}

// k_act on the register-resident forward (k_rows_reg's shapes): one wave per 16 rows, the weights
// shared through LDS
template <int T1, int T2, int T3, bool kNorm, int kAct>
__global__ __launch_bounds__(RR_WG, 2) void k_act_reg(ActArgs A) {
  constexpr int CB = 32;
  __shared__ float4 wl[2 * CB * 64];
  const int lane = threadIdx.x & 63, r = lane & 15, gq = lane >> 4;
  // workgroup pairs: even = the actor over four row tiles, odd = the critic over the same tiles
  const int net = blockIdx.x & 1;
  const int row0 = ((blockIdx.x >> 1) * (RR_WG / 64) + (threadIdx.x >> 6)) * RR_TR;  // (waves past the rows run on zeros, store nothing)
  const int64_t row = row0 + r;
  const bool ok = row < A.rows;
  Tile z[2];
  RrStage<CB> wst;
  rr_fetch<2 * T1, CB>(A.ws + A.n[net].wr[0], 0, wst);
  {
    Tile x0[2];
    act_rr_gather<kNorm>(A, net, row, ok, true, x0);
    rr_forward_chain<T1, T2, T3, false, CB, kAct>(A.n[net], A.ws, wl, 0, x0, z, wst, nullptr);
    if (net == 0) {
      // lane (r, g) holds actions 4 g + u and 16 + 4 g + u of row r
      float lp = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int n = 16 * (j >> 2) + 4 * gq + (j & 3);
        if (ok && n < A.na) lp += sample_action(A, row, n, z[j >> 2][j & 3]);
      }
      lp = rr_feat_sum(lp);
      if (ok && gq == 0) A.s_lp[row] = lp;
    } else if (ok && gq == 0) {
      A.s_val[row] = z[0][0];
    }
  }
}

// k_act for rollouts of the 128-wide nets (rsl_rl's [128, 128, 128], walking v2; round 6): one
// workgroup of four waves per 16-row tile and net, the waves splitting every layer's output tiles
// (a quarter each) and exchanging the layer's activations through LDS (double-buffered, one barrier
// per layer); each wave reads its own output tiles' weight blocks from L2 (no staging). At 4096 rows
// that is 2048 waves (two per SIMD) with a quarter of k_act_reg's MFMAs each, against k_act_reg's 512
// waves holding the whole net. Same statement (same per-lane accumulation order within a tile).
template <int TI, int TO, int kAct>
__device__ __forceinline__ void as_layer(const float* __restrict__ img, const float* __restrict__ bias,
                                         const Tile (&in)[TI], Tile (&out)[TO], Tile* __restrict__ xs, int wv,
                                         int lane) {
  constexpr int TQ = TO / 4;
  const float4* g = reinterpret_cast<const float4*>(img);
  float4 wb[TI][TQ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int q = 0; q < TQ; ++q) wb[i][q] = g[(i * TO + wv * TQ + q) * 64 + lane];
  Tile acc[TQ];
#pragma unroll
  for (int q = 0; q < TQ; ++q) acc[q] = Tile{};
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int q = 0; q < TQ; ++q) {
      Tile a = acc[q];
      a = mfma16(wb[i][q].x, in[i][0], a);
      a = mfma16(wb[i][q].y, in[i][1], a);
      a = mfma16(wb[i][q].z, in[i][2], a);
      a = mfma16(wb[i][q].w, in[i][3], a);
      acc[q] = a;
    }
  const float* bp = bias + 4 * ((lane & 63) >> 4);
#pragma unroll
  for (int q = 0; q < TQ; ++q) {
    const int o = wv * TQ + q;
    const float4 bq = *reinterpret_cast<const float4*>(bp + 16 * o);
    const float bv[4] = {bq.x, bq.y, bq.z, bq.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float v = acc[q][u] + bv[u];
      v = act_f<kAct>(v);
      acc[q][u] = v;
    }
    xs[o * 64 + lane] = acc[q];
  }
  __syncthreads();
#pragma unroll
  for (int o = 0; o < TO; ++o) out[o] = xs[o * 64 + lane];
}

template <int T1, int T2, int T3, bool kNorm, int kAct>
__global__ __launch_bounds__(256, 2) void k_act_split(ActArgs A) {
  static_assert(T1 % 4 == 0 && T2 % 4 == 0 && T3 % 4 == 0, "output tiles split over four waves");
  constexpr int TM = T1 > T2 ? (T1 > T3 ? T1 : T3) : (T2 > T3 ? T2 : T3);
  __shared__ Tile xs[2][TM * 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r = lane & 15, gq = lane >> 4;
  const int net = blockIdx.x & 1;
  const int64_t row = (int64_t)(blockIdx.x >> 1) * 16 + r;
  const bool ok = row < A.rows;
  const NetW& w = A.n[net];
  Tile x0[2], x1[T1], x2[T2], x3[T3];
  act_rr_gather<kNorm>(A, net, row, ok, wv == 0, x0);
  as_layer<2, T1, kAct>(A.ws + w.wr[0], A.ws + w.bp[0], x0, x1, xs[0], wv, lane);
  as_layer<T1, T2, kAct>(A.ws + w.wr[1], A.ws + w.bp[1], x1, x2, xs[1], wv, lane);
  as_layer<T2, T3, kAct>(A.ws + w.wr[2], A.ws + w.bp[2], x2, x3, xs[0], wv, lane);
  if (wv != 0) return;
  // the output layer (2 tiles in the image: num_actions <= 13 and the value live in tile 0), wave 0
  Tile z = Tile{};
  {
    const float4* g = reinterpret_cast<const float4*>(A.ws + w.wr[3]);
#pragma unroll
    for (int i = 0; i < T3; ++i) {
      const float4 wq = g[(i * 2 + 0) * 64 + lane];
      z = mfma16(wq.x, x3[i][0], z);
      z = mfma16(wq.y, x3[i][1], z);
      z = mfma16(wq.z, x3[i][2], z);
      z = mfma16(wq.w, x3[i][3], z);
    }
    const float4 bq = *reinterpret_cast<const float4*>(A.ws + w.bp[3] + 4 * gq);
    z[0] += bq.x; z[1] += bq.y; z[2] += bq.z; z[3] += bq.w;
  }
  if (net == 0) {
    // lane (r, g) holds actions 4 g + u of row r
    float lp = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int n = 4 * gq + u;
      if (ok && n < A.na) lp += sample_action(A, row, n, z[u]);
    }
    lp = rr_feat_sum(lp);
    if (ok && gq == 0) A.s_lp[row] = lp;
  } else if (ok && gq == 0) {
    A.s_val[row] = z[0];
  }
}

// PPO.process_env_step + the runner's episode bookkeeping (zbot_lab_amd/rl/runner.py _rollout) for
// one step, one workgroup: the storage slot's reward (+ gamma * value on time-outs, rsl_rl's
// bootstrap) and done; cur_rew += reward, cur_len += 1; over the done envs ep_stats += {sum cur_rew,
// sum cur_len, count} (a fixed-order block reduction), then their cur_rew / cur_len are cleared.
__global__ __launch_bounds__(1024) void k_env_post(const float* __restrict__ rew, const int64_t* __restrict__ done,
                                                   const uint8_t* __restrict__ tout, const float* __restrict__ val,
                                                   float gamma, float* __restrict__ s_rew, float* __restrict__ s_done,
                                                   float* __restrict__ cur_rew, float* __restrict__ cur_len,
                                                   float* __restrict__ ep_stats, int n) {
  __shared__ float red[3][16];
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  // four envs per thread in flight (the loads of all four issued before the first is used: one
  // memory round trip instead of four); the same envs in the same order per thread as one at a time
  constexpr int U = 4;
  for (int e0 = threadIdx.x; e0 < n; e0 += U * blockDim.x) {
    float r[U], v[U], cr0[U], cl0[U];
    int64_t dd[U];
    uint8_t to[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = min(e0 + u * (int)blockDim.x, n - 1);
      r[u] = rew[e];
      dd[u] = done[e];
      v[u] = val[e];
      to[u] = tout ? tout[e] : 0;
      cr0[u] = cur_rew[e];
      cl0[u] = cur_len[e];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int e = e0 + u * (int)blockDim.x;
      if (e < n) {
        const bool d = dd[u] > 0;
        float t = gamma * v[u];
        asm volatile("" : "+v"(t));  // (torch rounds the product, then the sum: no fma contraction)
        s_rew[e] = to[u] ? r[u] + t : r[u];
        s_done[e] = (float)dd[u];
        const float cr = cr0[u] + r[u], cl = cl0[u] + 1.f;
        if (d) { a0 += cr; a1 += cl; a2 += 1.f; }
        cur_rew[e] = d ? 0.f : cr;
        cur_len[e] = d ? 0.f : cl;
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    a0 += __shfl_xor(a0, o);
    a1 += __shfl_xor(a1, o);
    a2 += __shfl_xor(a2, o);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a0;
    red[1][threadIdx.x >> 6] = a1;
    red[2][threadIdx.x >> 6] = a2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[threadIdx.x][w];
    ep_stats[threadIdx.x] += t;
  }
}

// ------------------------------------------------------------------------------- GAE
// RolloutStorage.compute_returns (zbot_lab_amd/rl/ppo.py; rsl_rl GAE with time-out bootstrapping
// already folded into the rewards): one thread per env runs the backward recursion over T steps;
// advantages = returns - values, then normalised by the mean and the unbiased std over all T x N.
// Partial sums per block in a fixed order (deterministic).
constexpr int GAE_BLOCKS = 256;
__global__ __launch_bounds__(256) void k_gae(const float* __restrict__ rew, const float* __restrict__ done,
                                             const float* __restrict__ val, const float* __restrict__ last,
                                             float* __restrict__ ret, float* __restrict__ adv, int T, int N, float gamma,
                                             float lam, float* __restrict__ part) {
  __shared__ float red[4];
  float s = 0.f;
  for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
    float a = 0.f, next = last[n];
    for (int k = T - 1; k >= 0; --k) {
      const int64_t e = (int64_t)k * N + n;
      const float v = val[e], nt = 1.f - done[e];
      // torch rounds every product and sum of the recursion (one kernel per op): no fma contraction
      float p = nt * gamma * next, q = nt * gamma * lam * a;
      asm volatile("" : "+v"(p), "+v"(q));
      const float delta = rew[e] + p - v;
      a = delta + q;
      const float r = a + v;
      ret[e] = r;
      const float d = r - v;
      adv[e] = d;
      s += d;
      next = v;
    }
  }
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// one block: the mean, then the unbiased variance around it -> part[GAE_BLOCKS .. +2] = {mean, std + 1e-8}
__global__ __launch_bounds__(1024) void k_adv_stats(const float* __restrict__ adv, int64_t M, float* __restrict__ part) {
  __shared__ float red[16];
  __shared__ float mean_s;
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int b = 0; b < GAE_BLOCKS; ++b) t += part[b];
    mean_s = t / (float)M;
  }
  __syncthreads();
  const float mean = mean_s;
  float q = 0.f;
  for (int64_t e = threadIdx.x; e < M; e += blockDim.x) {
    const float d = adv[e] - mean;
    q += d * d;
  }
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = q;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    part[GAE_BLOCKS] = mean;
    part[GAE_BLOCKS + 1] = sqrtf(t / (float)(M - 1)) + 1e-8f;
  }
}
__global__ __launch_bounds__(256) void k_adv_norm(float* __restrict__ adv, int64_t M, const float* __restrict__ part) {
  const float mean = part[GAE_BLOCKS], den = part[GAE_BLOCKS + 1];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < M; e += (int64_t)gridDim.x * blockDim.x)
    adv[e] = (adv[e] - mean) / den;  // (a division, as torch's (adv - mean) / (std + 1e-8))
}

// ------------------------------------------------------------------------------- observation statistics
// EmpiricalNormalization.update (zbot_lab_amd/rl/normalizer.py) for one batch of rows, in two launches
// with the kernel boundary as the only ordering (no grid-wide fence, no atomics):
//   k_obs_part   workgroup b of G takes the fixed row range [b rows / G, (b + 1) rows / G) of a source
//                 and computes per column, in two passes, the range's mean and its sum of squared
//                 deviations from that mean (the range is a few KB: the second pass hits L1 / L2)
//   k_obs_merge  one workgroup per normalizer: the batch mean from the partial means, then the batch's
//                 sum of squared deviations around it (sum_b M2_b + n_b (mean_b - mean)^2: a two-pass
//                 over the partials, no E[x^2] - E[x]^2 anywhere), then count, the `until` test and the
//                 merge into the running statistics
// Every sum runs in a fixed order over fixed ranges, so the result does not depend on the workgroup
// schedule. The arithmetic is fp64 (a few thousand adds per launch); the state stays fp32 / int64.
constexpr int NORM_MAX_PARTS = 256;  // workgroups of k_obs_part per source
constexpr int NORM_PART_ROWS = 64;   // rows per workgroup up to NORM_MAX_PARTS * 64 rows, more beyond
inline int norm_parts(int rows) {
  const int g = (rows + NORM_PART_ROWS - 1) / NORM_PART_ROWS;
  return g < NORM_MAX_PARTS ? g : NORM_MAX_PARTS;
}
struct NormArgs {
  zbp_obs_norm nrm[2];  // targets (mean == nullptr: none)
  int src[2];           // the source each target reads
  const float* x[2];    // sources [rows][dim[s]]
  int dim[2];
  int rows, G;
  double* part;  // [source][G][2][32]: column means, sums of squared deviations
};
__device__ __forceinline__ int norm_row0(int b, int rows, int G) { return (int)((int64_t)b * rows / G); }

__global__ __launch_bounds__(256) void k_obs_part(NormArgs A) {
  __shared__ double red[2][8][32];
  const int s = blockIdx.y, b = blockIdx.x, c = threadIdx.x & 31, j = threadIdx.x >> 5;
  const int D = A.dim[s], r0 = norm_row0(b, A.rows, A.G), r1 = norm_row0(b + 1, A.rows, A.G);
  const float* x = A.x[s];
  double sum = 0.0;
  if (c < D)
    for (int r = r0 + j; r < r1; r += 8) sum += (double)x[(int64_t)r * D + c];
  red[0][j][c] = sum;
  __syncthreads();
  double mean = 0.0;
  for (int k = 0; k < 8; ++k) mean += red[0][k][c];
  mean /= (double)(r1 - r0);
  double q = 0.0;
  if (c < D)
    for (int r = r0 + j; r < r1; r += 8) {
      const double d = (double)x[(int64_t)r * D + c] - mean;
      q += d * d;
    }
  red[1][j][c] = q;
  __syncthreads();
  if (j == 0) {
    double m2 = 0.0;
    for (int k = 0; k < 8; ++k) m2 += red[1][k][c];
    double* p = A.part + ((int64_t)s * A.G + b) * 64;
    p[c] = mean;
    p[32 + c] = m2;
  }
}

__global__ __launch_bounds__(1024) void k_obs_merge(NormArgs A) {
  __shared__ double red[32][32];
  const zbp_obs_norm& nr = A.nrm[blockIdx.x];
  if (!nr.mean) return;
  const int64_t count0 = *nr.count;
  if (nr.until >= 0 && count0 >= nr.until) return;  // (uniform: every thread reads the same count)
  const int c = threadIdx.x & 31, j = threadIdx.x >> 5, G = A.G, rows = A.rows;
  const double* part = A.part + (int64_t)A.src[blockIdx.x] * G * 64;
  double acc = 0.0;
  for (int b = j; b < G; b += 32) acc += (double)(norm_row0(b + 1, rows, G) - norm_row0(b, rows, G)) * part[b * 64 + c];
  red[j][c] = acc;
  __syncthreads();
  double mean_x = 0.0;
  for (int k = 0; k < 32; ++k) mean_x += red[k][c];
  mean_x /= (double)rows;
  __syncthreads();
  acc = 0.0;
  for (int b = j; b < G; b += 32) {
    const double d = part[b * 64 + c] - mean_x;
    acc += part[b * 64 + 32 + c] + (double)(norm_row0(b + 1, rows, G) - norm_row0(b, rows, G)) * d * d;
  }
  red[j][c] = acc;
  __syncthreads();
  if (j == 0 && c < nr.dim) {
    double m2 = 0.0;
    for (int k = 0; k < 32; ++k) m2 += red[k][c];
    const double var_x = m2 / (double)rows;
    const double rate = (double)rows / (double)(count0 + rows);
    const double mean0 = (double)nr.mean[c], var0 = (double)nr.var[c];
    const double delta = mean_x - mean0, mean1 = mean0 + rate * delta;
    const float var1 = (float)(var0 + rate * (var_x - var0 + delta * (mean_x - mean1)));
    nr.mean[c] = (float)mean1;
    nr.var[c] = var1;
    nr.std[c] = sqrtf(var1);
  }
  __syncthreads();  // (every thread has read the old count)
  if (threadIdx.x == 0) *nr.count = count0 + rows;
}

// k_rows_reg instantiation for the nets' shape: 1 = hidden [256, 256, 128], 2 = [128, 128, 128] (both
// nets; inputs / outputs <= 32), 0 = none (k_rows)
int reg_shape(const Layout& lo, int B = 128) {
  if (B % 64) return 0;  // (k_rows_reg: whole workgroups of four 16-row tiles)
  const char* e = getenv("ZBP_ROWS");  // (read per call: tests switch it)
  if (e && strcmp(e, "lds") == 0) return 0;
  const NetW &a = lo.n[0], &c = lo.n[1];
  if (a.L != 4 || c.L != 4) return 0;
  for (int l = 0; l <= 4; ++l)
    if (a.p[l] != c.p[l]) return 0;
  if (a.p[0] != 32 || a.p[4] != 32) return 0;
  if (a.p[1] == 256 && a.p[2] == 256 && a.p[3] == 128) return 1;
  if (a.p[1] == 128 && a.p[2] == 128 && a.p[3] == 128) return 2;
  return 0;
}

int launch_check(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(e, what);
}

// The register kernels per activation. ELU (every shipped cfg) keeps its two instantiations, with and
// without the normalizer's code; the other activations have one each, the kNorm one, which tests the
// normalizer's pointer at run time (half the instantiations to compile).
// f(activation, kNorm), both std::integral_constants, for exactly that set.
template <class F>
void with_act_norm(int act, bool norm, F&& f) {
  with_act(act, [&](auto a) {
    if constexpr (decltype(a)::value == ZBP_ACT_ELU) {
      if (!norm) return f(a, std::false_type{});
    }
    return f(a, std::true_type{});
  });
}
// (sym: the zbp_symmetry instantiations, one per activation: the kNorm ones, as the non-ELU activations above)
template <int T1, int T2, int T3>
void launch_rows_reg(int act, bool norm, bool sym, int grid, hipStream_t s, const RowArgs& R) {
  if (sym) {
    with_act(act, [&](auto a) { k_rows_reg<T1, T2, T3, true, decltype(a)::value, true><<<grid, RR_WG, 0, s>>>(R); });
    return;
  }
  with_act_norm(act, norm, [&](auto a, auto n) {
    k_rows_reg<T1, T2, T3, decltype(n)::value, decltype(a)::value><<<grid, RR_WG, 0, s>>>(R);
  });
}
template <int T1, int T2, int T3>
void launch_act_reg(int act, bool norm, int grid, hipStream_t s, const ActArgs& A) {
  with_act_norm(act, norm, [&](auto a, auto n) {
    k_act_reg<T1, T2, T3, decltype(n)::value, decltype(a)::value><<<grid, RR_WG, 0, s>>>(A);
  });
}
void launch_act_split(int act, bool norm, int grid, hipStream_t s, const ActArgs& A) {
  with_act_norm(act, norm, [&](auto a, auto n) {
    k_act_split<8, 8, 8, decltype(n)::value, decltype(a)::value><<<grid, 256, 0, s>>>(A);
  });
}

// The LDS row tile of k_rows / k_act (float offsets): X_l [32][p(l) + 4] of every layer (the wider of the
// two nets), then (dz != nullptr: the minibatch pass) the output layer's dZ [32][32 + 4], the output
// pre-activations [32][33], and (red != nullptr) the NSTAT per-tile sums. Refuses a tile over the CU's
// 160 KB and raises the kernel's dynamic-LDS limit on its first call (a host-side attribute: set once per
// kernel, outside any stream capture's ops). *bytes: the launch's dynamic LDS.
template <class Args>
int lds_row_tile(const Layout& lo, void (*kernel)(Args), const char* api, const char* name, int (&x)[MAXL], int* dz,
                 int& out, int* red, size_t* bytes) {
  int off = 0;
  for (int l = 0; l < MAXL; ++l) {
    const int p = lo.n[0].p[l] > lo.n[1].p[l] ? lo.n[0].p[l] : lo.n[1].p[l];
    x[l] = off;
    off += TR * (p + 4);
  }
  if (dz) { *dz = off; off += TR * (32 + 4); }
  out = off;
  off += TR * 33;
  if (red) { *red = off; off += NSTAT; }
  *bytes = sizeof(float) * off;
  char what[96];
  if (*bytes > 160 * 1024) {
    snprintf(what, sizeof(what), "%s: nets too wide for the LDS row tile", api);
    return fail(-1, what);
  }
  static const void* lds_set[4] = {};  // (the kernels of this Args type that have the limit raised)
  int slot = 0;
  while (slot < 3 && lds_set[slot] && lds_set[slot] != (const void*)kernel) ++slot;
  if (lds_set[slot] != (const void*)kernel) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) {
      snprintf(what, sizeof(what), "hipFuncSetAttribute %s", name);
      return hip_fail(e, what);
    }
    lds_set[slot] = (const void*)kernel;
  }
  return 0;
}

PackArgs pack_args(const Layout& lo, const zbp_net* a, const zbp_net* c, float* ws) {
  PackArgs P{};
  P.n[0] = lo.n[0];
  P.n[1] = lo.n[1];
  const zbp_net* nets[2] = {a, c};
  for (int k = 0; k < 2; ++k)
    for (int l = 0; l < nets[k]->n_layers; ++l) { P.w[k][l] = nets[k]->w[l]; P.b[k][l] = nets[k]->b[l]; }
  P.ws = ws;
  P.rng = reinterpret_cast<uint32_t*>(ws + lo.rng);
  return P;
}
int do_pack(const Layout& lo, const zbp_net* a, const zbp_net* c, float* ws, hipStream_t s,
            const PackArgs* tail = nullptr) {
  const int L = lo.n[0].L > lo.n[1].L ? lo.n[0].L : lo.n[1].L;
  PackArgs P = pack_args(lo, a, c, ws);
  if (tail) {
    P.tail = 1;
    P.n_params = tail->n_params;
    P.lr = tail->lr;
    P.stats = tail->stats;
    P.acc = tail->acc;
    P.desired_kl = tail->desired_kl;
    for (int t = 0; t < tail->n_params; ++t) P.step[t] = tail->step[t];
  }
  k_pack<<<dim3(64, 2, L), 256, 0, s>>>(P);
  return launch_check("k_pack");
}

}  // namespace

extern "C" {

const char* zbp_last_error(void) { return g_err; }

int64_t zbp_workspace_floats(const zbp_net* actor, const zbp_net* critic, int32_t batch) {
  if (const char* e = check_nets(actor, critic)) return fail(-1, e);
  if (batch < TR || batch % TR) return fail(-1, "zbp_workspace_floats: batch must be a positive multiple of 32");
  return make_layout(actor, critic, batch).total;
}

int zbp_pack(const zbp_net* actor, const zbp_net* critic, float* ws, int32_t batch, void* stream) {
  if (const char* e = check_nets(actor, critic)) return fail(-1, e);
  if (!ws || batch < TR || batch % TR) return fail(-1, "zbp_pack: workspace / batch");
  return do_pack(make_layout(actor, critic, batch), actor, critic, ws, (hipStream_t)stream);
}

int zbp_minibatch(const zbp_net* actor, const zbp_net* critic, const float* std_param, float* std_grad,
                  const zbp_batch* batch, const zbp_loss_cfg* loss, float* ws, float* stats, void* stream) {
  if (const char* e = check_nets(actor, critic)) return fail(-1, e);
  if (!batch || !loss || !ws || !stats || !std_param || !std_grad) return fail(-1, "zbp_minibatch: null argument");
  const int B = batch->batch;
  if (B < TR || B % TR) return fail(-1, "zbp_minibatch: batch must be a positive multiple of 32");
  if (batch->num_actions != actor->dim[actor->n_layers] || batch->num_actions > NSTAT - 3)
    return fail(-1, "zbp_minibatch: num_actions must match the actor output (<= 13)");
  if (batch->obs_dim != actor->dim[0] || batch->critic_obs_dim != critic->dim[0] || critic->dim[critic->n_layers] != 1)
    return fail(-1, "zbp_minibatch: observation dims / critic output");
  if (const char* e = check_norm(&batch->actor_norm, batch->obs_dim)) return fail(-1, e);
  if (const char* e = check_norm(&batch->critic_norm, batch->critic_obs_dim)) return fail(-1, e);
  for (int k = 0; k < 2; ++k) {
    const zbp_net* n = k ? critic : actor;
    for (int l = 0; l < n->n_layers; ++l)
      if (!n->gw[l] || !n->gb[l]) return fail(-1, "zbp_minibatch: null .grad buffer");
  }
  // zbp_symmetry: on with any of its switches; then every table is there, and the workspace was sized and
  // packed for the 2 B kernel rows (include/zbot_ppo.h, the workspace rule)
  const zbp_symmetry& sy = batch->symmetry;
  const bool sym = sy.augment || sy.mirror_loss || sy.loss_acc;
  if (sym) {
    if (!sy.obs_perm || !sy.obs_sign || !sy.critic_perm || !sy.critic_sign || !sy.act_perm || !sy.act_sign)
      return fail(-1, "zbp_minibatch: symmetry on with a null table");
    if (sy.ws_batch != 2 * B) return fail(-1, "zbp_minibatch: symmetry needs a workspace of 2 * batch rows (ws_batch)");
  }
  const int rows = sym ? 2 * B : B;  // kernel rows
  hipStream_t s = (hipStream_t)stream;
  const Layout lo = make_layout(actor, critic, rows);

  RowArgs R{};
  R.n[0] = lo.n[0];
  R.n[1] = lo.n[1];
  R.bt = *batch;
  R.lc = *loss;
  R.std_param = std_param;
  R.ws = ws;
  R.stats = lo.stats;
  R.B = rows;
  if (sym) {
    R.sym_inv_loss = 1.f / (float)(sy.augment ? 2 * B : B);
    R.sym_grad = sy.mirror_loss ? sy.mirror_coef * 2.f / ((float)B * (float)batch->num_actions) : 0.f;
    R.sym_part = lo.sym;
  }
  size_t lds;
  if (int rc = lds_row_tile(lo, sym ? k_rows_sym : k_rows, "zbp_minibatch", sym ? "k_rows_sym" : "k_rows", R.lds_x, &R.lds_dz,
                            R.lds_out, &R.lds_red, &lds))
    return rc;
  // the register-resident row kernel for the shipped shapes (ZBP_ROWS=lds: the LDS one, for A/Bs)
  const int shape = reg_shape(lo, rows);
  const bool norm = batch->actor_norm.mean || batch->critic_norm.mean;
  if (shape == 1)
    launch_rows_reg<16, 16, 8>(actor->activation, norm, sym, 2 * (rows / 64), s, R);
  else if (shape == 2)
    launch_rows_reg<8, 8, 8>(actor->activation, norm, sym, 2 * (rows / 64), s, R);
  else if (sym)
    k_rows_sym<<<rows / TR, ROW_THREADS, lds, s>>>(R);
  else
    k_rows<<<rows / TR, ROW_THREADS, lds, s>>>(R);
  if (int rc = launch_check("k_rows")) return rc;

  WgradArgs W{};
  W.n[0] = lo.n[0];
  W.n[1] = lo.n[1];
  W.tm = lo.tm;
  W.batch = rows;
  W.ws = ws;
  W.part = lo.part;
  k_wgrad<<<lo.tm.blk0[2 * MAXL], 256, 0, s>>>(W);
  if (int rc = launch_check("k_wgrad")) return rc;

  ReduceArgs D{};
  D.n[0] = lo.n[0];
  D.n[1] = lo.n[1];
  D.tm = lo.tm;
  D.row_tiles = shape ? rows / RR_TR : rows / TR;
  D.batch = B;
  if (sym) {
    D.sym_samples = B;
    D.sym_loss_rows = sy.augment ? 2 * B : B;
    D.sym_part = lo.sym;
    D.sym_acc = sy.loss_acc;
  }
  D.num_actions = batch->num_actions;
  for (int k = 0; k < 2; ++k) {
    const zbp_net* n = k ? critic : actor;
    for (int l = 0; l < n->n_layers; ++l) {
      D.gw[k][l] = n->gw[l];
      D.gb[k][l] = n->gb[l];
    }
  }
  D.std_param = std_param;
  D.std_grad = std_grad;
  D.stats = stats;
  D.entropy_coef = loss->entropy_coef;
  D.log_std = loss->log_std;
  D.ws = ws;
  D.part = lo.part;
  D.rstats = lo.stats;
  D.norm2 = ws + lo.scratch;
  if (sym)
    k_reduce_sym<<<lo.tm.wtiles + 1, RED_THREADS, 0, s>>>(D);
  else
    k_reduce<<<lo.tm.wtiles + 1, RED_THREADS, 0, s>>>(D);
  return launch_check("k_reduce");
}

int zbp_optimizer_step(const zbp_params* params, float* lr, const float* stats, float* acc, float desired_kl,
                       float max_grad_norm, float beta1, float beta2, float eps, const zbp_net* actor,
                       const zbp_net* critic, float* ws, int32_t batch, int32_t norm_from_minibatch, void* stream) {
  if (!params || params->n_params < 1 || params->n_params > ZBP_MAX_PARAMS || !lr || !stats || !acc || !ws)
    return fail(-1, "zbp_optimizer_step: bad argument");
  if (const char* e = check_nets(actor, critic)) return fail(-1, e);
  hipStream_t s = (hipStream_t)stream;
  const Layout lo = make_layout(actor, critic, batch);
  OptimArgs O{};
  O.P = *params;
  O.lr = lr;
  O.stats = stats;
  O.acc = acc;
  O.desired_kl = desired_kl;
  O.max_norm = max_grad_norm;
  O.b1 = beta1;
  O.b2 = beta2;
  O.eps = eps;
  O.norm2 = ws + lo.scratch;
  O.total = 0;
  for (int t = 0; t < params->n_params; ++t) O.total += params->numel[t];
  if (norm_from_minibatch) {
    O.nparts = lo.tm.wtiles + 1;  // k_reduce's per-tile sums of the gradients it wrote
  } else {
    O.nparts = 64;
    k_norm<<<64, 256, 0, s>>>(O);
    if (int rc = launch_check("k_norm")) return rc;
  }
  k_adam<<<256, 256, 0, s>>>(O);
  if (int rc = launch_check("k_adam")) return rc;
  PackArgs T{};
  T.n_params = params->n_params;
  T.lr = lr;
  T.stats = stats;
  T.acc = acc;
  T.desired_kl = desired_kl;
  for (int t = 0; t < params->n_params; ++t) T.step[t] = params->step[t];
  return do_pack(lo, actor, critic, ws, s, &T);
}

#define ZBP_STR_(x) #x
#define ZBP_STR(x) ZBP_STR_(x)
int zbp_act(const zbp_net* actor, const zbp_net* critic, const float* std_param, const zbp_act_io* io, float* ws,
            int32_t batch, void* stream) {
  if (const char* e = check_nets(actor, critic)) return fail(-1, e);
  if (!io || !ws || !std_param || !io->obs || !io->critic_obs || !io->actions || !io->st_obs ||
      !io->st_critic_obs || !io->st_actions || !io->st_values || !io->st_log_prob || !io->st_mu || !io->st_sigma)
    return fail(-1, "zbp_act: null argument");
  if (io->rows < 1 || batch < TR || batch % TR) return fail(-1, "zbp_act: rows / batch");
  if (io->num_actions != actor->dim[actor->n_layers] || io->obs_dim != actor->dim[0] ||
      io->critic_obs_dim != critic->dim[0] || critic->dim[critic->n_layers] != 1)
    return fail(-1, "zbp_act: observation / action dims");
  if (const char* e = check_norm(&io->actor_norm, io->obs_dim)) return fail(-1, e);
  if (const char* e = check_norm(&io->critic_norm, io->critic_obs_dim)) return fail(-1, e);
  // (noise_at packs the step into the key's low 12 bits: outside them it would alias the draw counter)
  if (!io->noise && (io->noise_step < 0 || io->noise_step >= ZBP_NOISE_STEPS))
    return fail(-1, "zbp_act: noise_step outside [0, " ZBP_STR(ZBP_NOISE_STEPS) ")");
  const Layout lo = make_layout(actor, critic, batch);
  ActArgs A{};
  A.n[0] = lo.n[0];
  A.n[1] = lo.n[1];
  A.ws = ws;
  A.std_param = std_param;
  A.obs = io->obs;
  A.cobs = io->critic_obs;
  A.noise = io->noise;
  A.rng = reinterpret_cast<const uint32_t*>(ws + lo.rng);
  A.noise_step = io->noise_step;
  A.noise_seed = (uint32_t)io->noise_seed;
  A.obs_dim = io->obs_dim;
  A.cobs_dim = io->critic_obs_dim;
  A.na = io->num_actions;
  A.rows = io->rows;
  A.actions = io->actions;
  A.s_obs = io->st_obs;
  A.s_cobs = io->st_critic_obs;
  A.s_act = io->st_actions;
  A.s_val = io->st_values;
  A.s_lp = io->st_log_prob;
  A.s_mu = io->st_mu;
  A.s_sig = io->st_sigma;
  A.nrm[0] = io->actor_norm;
  A.nrm[1] = io->critic_norm;
  A.log_std = io->log_std;
  size_t lds;
  if (int rc = lds_row_tile(lo, k_act, "zbp_act", "k_act", A.lds_x, nullptr, A.lds_out, nullptr, &lds)) return rc;
  // (the register-resident forward, actor and critic in separate workgroups, from ZBP_ACT_REG_MIN rows
  // (4096): 23.5 us against the LDS kernel's 34.9 at 4096 rows (before the split 42 us: too few
  // workgroups), 146 against 242 at 32 768 (profiles/r5y); ZBP_ACT=lds / reg for A/Bs)
  const char* ea = getenv("ZBP_ACT");
  const bool f_reg = ea && !strcmp(ea, "reg"), f_lds = ea && !strcmp(ea, "lds"), f_split = ea && !strcmp(ea, "split");
  const int reg_min = (f_reg || f_split) ? 0 : (f_lds ? (1 << 30) : ZBP_ACT_REG_MIN);
  const int shape = io->rows >= reg_min ? reg_shape(lo) : 0, wgs = 2 * ((io->rows + 63) / 64);
  // the 128-wide nets (shape 2): the split-output forward (k_act_split, round 6) up to
  // ZBP_ACT_SPLIT_MAX rows; ZBP_ACT=reg / lds / split forces a kernel for A/Bs and tests
  const bool split = shape == 2 && !f_reg && (f_split || io->rows <= ZBP_ACT_SPLIT_MAX);
  const bool norm = A.nrm[0].mean || A.nrm[1].mean;
  hipStream_t s = (hipStream_t)stream;
  if (split)
    launch_act_split(actor->activation, norm, 2 * ((io->rows + 15) / 16), s, A);
  else if (shape == 1)
    launch_act_reg<16, 16, 8>(actor->activation, norm, wgs, s, A);
  else if (shape == 2)
    launch_act_reg<8, 8, 8>(actor->activation, norm, wgs, s, A);
  else
    k_act<<<(io->rows + TR - 1) / TR, 256, lds, s>>>(A);
  return launch_check("k_act");
}

int zbp_env_post(const float* rewards, const int64_t* dones, const uint8_t* time_outs, const float* values, float gamma,
                 float* st_rewards, float* st_dones, float* cur_rew, float* cur_len, float* ep_stats, int32_t n,
                 void* stream) {
  if (!rewards || !dones || !values || !st_rewards || !st_dones || !cur_rew || !cur_len || !ep_stats || n < 1)
    return fail(-1, "zbp_env_post: bad argument");
  k_env_post<<<1, 1024, 0, (hipStream_t)stream>>>(rewards, dones, time_outs, values, gamma, st_rewards, st_dones, cur_rew,
                                                  cur_len, ep_stats, n);
  return launch_check("k_env_post");
}

int64_t zbp_norm_scratch_floats(int32_t rows) {
  if (rows < 1) return -1;
  return (int64_t)2 * norm_parts(rows) * 64 * (int64_t)(sizeof(double) / sizeof(float));
}

int zbp_norm_update(const zbp_obs_norm* actor, const zbp_obs_norm* critic, const float* obs, const float* critic_obs,
                    int32_t rows, float* scratch, void* stream) {
  const zbp_obs_norm* nr[2] = {actor && actor->mean ? actor : nullptr, critic && critic->mean ? critic : nullptr};
  const float* x[2] = {obs, critic_obs};
  if (!nr[0] && !nr[1]) return 0;
  if (rows < 1 || !scratch || ((uintptr_t)scratch & 7)) return fail(-1, "zbp_norm_update: rows / scratch");
  NormArgs A{};
  int nsrc = 0;
  for (int k = 0; k < 2; ++k) {
    if (!nr[k]) continue;
    if (const char* e = check_norm(nr[k], nr[k]->dim)) return fail(-1, e);
    if (!x[k]) return fail(-1, "zbp_norm_update: null observations");
    A.nrm[k] = *nr[k];
    // both normalizers on the same rows (every task here: obs == critic_obs): one read serves both
    if (k == 1 && nsrc == 1 && x[1] == A.x[0] && nr[1]->dim == A.dim[0]) {
      A.src[1] = 0;
      continue;
    }
    A.src[k] = nsrc;
    A.x[nsrc] = x[k];
    A.dim[nsrc++] = nr[k]->dim;
  }
  A.rows = rows;
  A.G = norm_parts(rows);
  A.part = reinterpret_cast<double*>(scratch);
  hipStream_t s = (hipStream_t)stream;
  k_obs_part<<<dim3(A.G, nsrc), 256, 0, s>>>(A);
  if (int rc = launch_check("k_obs_part")) return rc;
  k_obs_merge<<<2, 1024, 0, s>>>(A);
  return launch_check("k_obs_merge");
}

int zbp_gae(const float* rewards, const float* dones, const float* values, const float* last_values, float* returns,
            float* advantages, int32_t steps, int32_t envs, float gamma, float lam, int32_t normalize, float* scratch,
            void* stream) {
  if (!rewards || !dones || !values || !last_values || !returns || !advantages || !scratch || steps < 1 || envs < 1)
    return fail(-1, "zbp_gae: bad argument");
  hipStream_t s = (hipStream_t)stream;
  k_gae<<<GAE_BLOCKS, 256, 0, s>>>(rewards, dones, values, last_values, returns, advantages, steps, envs, gamma, lam,
                                   scratch);
  if (int rc = launch_check("k_gae")) return rc;
  if (!normalize) return 0;
  const int64_t M = (int64_t)steps * envs;
  k_adv_stats<<<1, 1024, 0, s>>>(advantages, M, scratch);
  if (int rc = launch_check("k_adv_stats")) return rc;
  k_adv_norm<<<256, 256, 0, s>>>(advantages, M, scratch);
  return launch_check("k_adv_norm");
}

}  // extern "C"
