/*
 * zbot_ppo.h — C ABI of libzbot_ppo.so: the PPO minibatch update of the rsl_rl ActorCritic on
 * MI355X as hand-written fp32 MFMA kernels (zbot_lab_amd/csrc/ppo_mlp.hip).
 *
 * Replaces, per minibatch of PPO.update (reference: rsl_rl's PPO as configured by
 * source/zbot/zbot/tasks/zbot6b_direct/agents/rsl_rl_ppo_cfg.py:65-91 and walked through in
 * ppo_learning_notes.md:521-548; restated in zbot_lab_amd/rl/ppo.py:PPO.update_steps):
 *   policy.update_distribution(obs_b) -> log_prob / evaluate(critic_obs_b) / entropy -> adaptive-KL
 *   statistic -> clipped surrogate + clipped value loss - entropy bonus -> loss.backward()
 * i.e. the actor and critic MLP forward passes, the loss and its gradient, and the backward pass
 * into every parameter's .grad (weights, biases, the Gaussian std). Gradient averaging across
 * ranks, the learning-rate rule, gradient clipping and Adam stay with the caller (torch), or run
 * fused in zbp_optimizer_step on one GPU.
 *
 * All pointers are device pointers (torch tensors' data_ptr), fp32 unless stated; every call is
 * ordered on `stream` (a hipStream_t) and never synchronises the host, so a sequence of calls can
 * be captured in a HIP graph. Returns 0 on success, a negative code on a bad argument or a HIP
 * error (zbp_last_error() describes it).
 */
#ifndef ZBOT_PPO_H
#define ZBOT_PPO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZBP_MAX_LAYERS 4 /* linear layers per MLP (3 hidden + output, the rsl_rl cfgs here) */

/* The activation after every layer of an MLP but the last (rsl_rl's `activation`), with torch's default
 * constants: ELU alpha = 1; SELU lambda = 1.0507009873554805, alpha = 1.6732632423543772; LeakyReLU
 * negative slope 0.01. The backward passes write each derivative from the stored OUTPUT x of the
 * activation: ELU x > 0 ? 1 : x + 1; ReLU x > 0; Tanh 1 - x^2; SELU x > 0 ? lambda : x + lambda alpha;
 * LeakyReLU x > 0 ? 1 : 0.01. */
enum { ZBP_ACT_ELU = 0, ZBP_ACT_RELU, ZBP_ACT_TANH, ZBP_ACT_SELU, ZBP_ACT_LRELU };

/* One MLP (torch nn.Sequential of Linear / activation): layer l maps dim[l] -> dim[l+1]; the
 * activation after every layer but the last. Limits: dim[0] <= 32 (observations), hidden dims
 * multiples of 32 up to 256, output dim <= 32. */
typedef struct {
  int32_t n_layers;
  int32_t dim[ZBP_MAX_LAYERS + 1];
  const float* w[ZBP_MAX_LAYERS]; /* Linear.weight [dim[l+1]][dim[l]] (row-major, contiguous) */
  const float* b[ZBP_MAX_LAYERS]; /* Linear.bias [dim[l+1]] */
  float* gw[ZBP_MAX_LAYERS];      /* their .grad buffers (overwritten by zbp_minibatch) */
  float* gb[ZBP_MAX_LAYERS];
  int32_t activation; /* ZBP_ACT_*; a zeroed field is ELU. Actor and critic must agree (rsl_rl has one
                         `activation` for both nets); any other value, or a mixed pair, is refused by
                         every entry point before any launch (zbp_workspace_floats returns < 0) */
} zbp_net;

/* Empirical observation normalization (rsl_rl EmpiricalNormalization; zbot_lab_amd/rl/normalizer.py):
 * the running statistics of one net's observations, device buffers owned by the caller. Where a net's
 * input rows are gathered (zbp_minibatch, zbp_act) column k < dim becomes
 *   (x[k] - mean[k]) / (std[k] + eps)
 * before the first layer (so the layer-0 weight gradient is the normalized input's); padded columns
 * stay 0 and the storage-slot copies zbp_act writes stay raw. mean == NULL: identity (a zeroed struct
 * is exactly the behaviour without it). zbp_norm_update maintains the buffers. */
typedef struct {
  float* mean;     /* [dim] running mean (initially 0) */
  float* var;      /* [dim] running biased variance (initially 1) */
  float* std;      /* [dim] sqrt(var) (initially 1) */
  int64_t* count;  /* [1] rows seen so far (initially 0) */
  float eps;       /* rsl_rl: 1e-2 */
  int64_t until;   /* the statistics freeze once count >= until; < 0: never */
  int32_t dim;     /* the net's observation dim (<= 32) */
} zbp_obs_norm;

/* rsl_rl's symmetry option (PPO `symmetry_cfg`; zbot_lab_amd/rl/symmetry.py SignedPermutation) for ONE
 * mirror map, a signed permutation per tensor:
 *   obs_m[k] = obs_sign[k] obs[obs_perm[k]],  cobs_m[k] = critic_sign[k] cobs[critic_perm[k]],
 *   act_m[a] = act_sign[a] act[act_perm[a]].
 * On (augment or mirror_loss or loss_acc != NULL) a minibatch of B = zbp_batch.batch samples is 2 B kernel
 * rows: sample j and its mirror both read row idx[idx_offset + j] of the rollout; the mirror applies the map
 * in the gather, BEFORE the normalizer (column k is normalized with the statistics of column k: rsl_rl's
 * normalizer sits inside the policy), to the observations, the critic observations and the actions, and
 * reuses the sample's log_prob, values, advantages and returns. Terms (rsl_rl PPO.update):
 *   surrogate, value loss   augment: means over the 2 B rows; otherwise over the B originals (the mirrored
 *                           rows get zero weight; they still run the critic's forward and a backward of
 *                           zeros -- the price of one launch shape for the three modes)
 *   KL, entropy             means over the B originals, always
 *   symmetry loss           mean over the B mirrored rows and the actions of (mu_m[a] - act_sign[a]
 *                           mu_o[act_perm[a]])^2, mu_o the original's mean, taken as a constant: with
 *                           mirror_loss, mirror_coef times its gradient goes into the mirrored row only,
 *                           dL / dmu_m[a] += mirror_coef 2 (mu_m[a] - target) / (B num_actions);
 *                           loss_acc[0] += the loss, with or without mirror_loss.
 * The row kernels hold an original next to its mirror in one tile (8 + 8 rows of k_rows_reg's 16-row tile,
 * 16 + 16 of k_rows' 32-row tile), so the pairing costs no launch; row order only changes fp32 summation
 * order. All zero: off, exactly the behaviour without the member.
 * Workspace rule: with symmetry on, the `batch` argument of zbp_workspace_floats, zbp_pack, zbp_act and
 * zbp_optimizer_step is the kernel row count 2 B; ws_batch states it here, and zbp_minibatch refuses
 * ws_batch != 2 * zbp_batch.batch before any launch (off: ws_batch is ignored).
 * The tables are device arrays the caller keeps valid; a perm entry outside [0, dim) is clamped into it
 * (never an out-of-bounds read; the result is then meaningless). */
typedef struct {
  const int32_t* obs_perm;     /* [obs_dim] */
  const float* obs_sign;       /* [obs_dim] +-1 */
  const int32_t* critic_perm;  /* [critic_obs_dim] */
  const float* critic_sign;    /* [critic_obs_dim] */
  const int32_t* act_perm;     /* [num_actions] */
  const float* act_sign;       /* [num_actions] */
  int32_t augment;             /* use_data_augmentation */
  int32_t mirror_loss;         /* use_mirror_loss */
  float mirror_coef;           /* mirror_loss_coeff */
  int32_t ws_batch;            /* the workspace's batch (kernel rows): 2 * zbp_batch.batch */
  float* loss_acc;             /* [1] += the minibatch's symmetry loss, or NULL */
} zbp_symmetry;

/* The rollout (RolloutStorage, flattened [T * N] rows) and this minibatch's rows:
 * rows idx[idx_offset .. idx_offset + batch) of the permutation (int64, rsl_rl's randperm). */
typedef struct {
  const float* obs;          /* [rows][obs_dim] */
  const float* critic_obs;   /* [rows][critic_obs_dim] */
  const float* actions;      /* [rows][num_actions] */
  const float* values;       /* [rows] target values */
  const float* advantages;   /* [rows] */
  const float* returns;      /* [rows] */
  const float* log_prob;     /* [rows] old log-probabilities */
  const float* mu;           /* [rows][num_actions] old action means */
  const float* sigma;        /* [rows][num_actions] old action stds */
  const int64_t* idx;        /* the update's permutation */
  int64_t idx_offset;
  int32_t batch;             /* minibatch rows (a multiple of 32) */
  int32_t obs_dim, critic_obs_dim, num_actions;
  zbp_obs_norm actor_norm;   /* applied to the gathered obs rows (mean == NULL: none) */
  zbp_obs_norm critic_norm;  /* applied to the gathered critic_obs rows */
  zbp_symmetry symmetry;     /* all zero: off */
} zbp_batch;

/* PPO loss constants (RslRlPpoAlgorithmCfg) */
typedef struct {
  float clip_param, value_loss_coef, entropy_coef;
  int32_t use_clipped_value_loss;
  int32_t log_std; /* rsl_rl noise_std_type "log": std_param holds log sigma and sigma = exp(std_param) in
                      the log-prob, the KL and the mean / std gradients; std_grad receives dL / d log sigma =
                      sigma dL / d sigma (the entropy bonus contributes -entropy_coef per action) and the
                      entropy statistic takes the parameter itself as log sigma. 0 ("scalar"): std_param is
                      sigma */
} zbp_loss_cfg;

/* Workspace floats for nets of these shapes and minibatch size (the caller allocates one float
 * buffer of that size, 256-byte aligned, and passes it to every call). `batch` here and in zbp_pack,
 * zbp_act and zbp_optimizer_step is the minibatch's kernel rows: zbp_batch.batch, or twice that with
 * zbp_batch.symmetry on (zbp_symmetry, the workspace rule). */
int64_t zbp_workspace_floats(const zbp_net* actor, const zbp_net* critic, int32_t batch);

/* Copy the current parameters into the workspace's padded / transposed images. Call once before
 * the first zbp_minibatch of an update and after every parameter change made outside
 * zbp_optimizer_step (a torch optimizer step, a checkpoint load). */
int zbp_pack(const zbp_net* actor, const zbp_net* critic, float* ws, int32_t batch, void* stream);

/* One minibatch: forward, loss, backward. Writes every .grad of both nets and std_grad
 * [num_actions], and stats[4] = {kl_mean, value_loss, surrogate_loss, entropy_mean} of the
 * minibatch (the KL statistic of the adaptive learning-rate rule and the loss terms). */
int zbp_minibatch(const zbp_net* actor, const zbp_net* critic, const float* std_param, float* std_grad,
                  const zbp_batch* batch, const zbp_loss_cfg* loss, float* ws, float* stats, void* stream);

/* Adam (torch.optim.Adam semantics, betas b1 / b2, eps, no weight decay) fused with rsl_rl's
 * adaptive learning-rate rule and global-norm gradient clipping, for one GPU:
 *   lr <- adaptive(lr, stats[0]) (desired_kl > 0; lr / 1.5 above 2 desired_kl, x 1.5 below half of
 *   it, within [1e-5, 1e-2]); grads scaled by min(1, max_norm / (||g|| + 1e-6)); step += 1;
 *   m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
 * over the params listed in `params` (the torch optimizer's param order): n_params tensors with
 * numel / param / grad / exp_avg / exp_avg_sq pointers. lr and step are device scalars (torch's
 * capturable Adam keeps `step` as a float tensor; one shared step counter is read from step[0] and
 * every tensor's own counter written). Then re-packs the workspace (zbp_pack). acc[3] += stats[1..3].
 * norm_from_minibatch != 0: the gradient norm comes from the per-tile sums of squares the last
 * zbp_minibatch on this workspace left (one launch fewer); only valid when the .grad buffers and
 * std_grad are still exactly what that call wrote (one GPU, no all-reduce or hook in between);
 * 0: recomputed from params->grad. */
#define ZBP_MAX_PARAMS 24
typedef struct {
  int32_t n_params;
  int64_t numel[ZBP_MAX_PARAMS];
  float* param[ZBP_MAX_PARAMS];
  float* grad[ZBP_MAX_PARAMS];
  float* exp_avg[ZBP_MAX_PARAMS];
  float* exp_avg_sq[ZBP_MAX_PARAMS];
  float* step[ZBP_MAX_PARAMS];
} zbp_params;
int zbp_optimizer_step(const zbp_params* params, float* lr, const float* stats, float* acc, float desired_kl,
                       float max_grad_norm, float beta1, float beta2, float eps, const zbp_net* actor,
                       const zbp_net* critic, float* ws, int32_t batch, int32_t norm_from_minibatch,
                       void* stream);

/* GAE (RolloutStorage.compute_returns): rewards / dones / values [steps][envs] (time-out bootstrap
 * already in the rewards), last_values [envs] -> returns, advantages = returns - values, then (if
 * normalize) advantages normalised by their mean and unbiased std (+1e-8). scratch: >= 258 floats. */
int zbp_gae(const float* rewards, const float* dones, const float* values, const float* last_values, float* returns,
            float* advantages, int32_t steps, int32_t envs, float gamma, float lam, int32_t normalize, float* scratch,
            void* stream);

/* One rollout step of PPO.act (rsl_rl ActorCritic.act / evaluate / get_actions_log_prob and the
 * transition fields of RolloutStorage.add; zbot_lab_amd/rl/ppo.py) for `rows` envs in one launch:
 * actions = mu + std * noise (noise: the caller's standard-normal draw, [rows][num_actions], or NULL:
 * drawn in the kernel, a counter-based standard normal keyed by noise_seed, the workspace's draw
 * counter -- which every zbp_pack / zbp_optimizer_step advances --, noise_step, the row and the
 * action), its
 * Gaussian log-probability summed over the actions, the critic's value; writes actions [rows][na]
 * (the env's input) and the storage slot of this step: observations, critic observations, actions,
 * values, log-probabilities, mu, sigma. Reads the workspace's weight images (zbp_pack must follow
 * every parameter change; zbp_optimizer_step re-packs itself). Replaces the ~30 torch kernels of a
 * policy step (runner._rollout).
 *
 * The in-kernel draw's stream key is (noise_seed << 32) ^ (draw counter << 12) ^ noise_step, 64 bits.
 * It is injective -- distinct (seed, counter, step) triples draw from distinct streams -- for
 * 0 <= noise_step < ZBP_NOISE_STEPS (4096) and a draw counter < 2^20 (packs / optimizer steps of one
 * workspace). Outside that range triples alias: (c, step 4096) is (c ^ 1,
 * step 0), and (seed s, counter 2^20 ^ c) is (s ^ 1, counter c). zbp_act refuses a noise_step outside
 * the range (noise == NULL); the counter lives on the device and is not checked. */
#define ZBP_NOISE_STEPS 4096
typedef struct {
  const float* obs;         /* [rows][obs_dim] */
  const float* critic_obs;  /* [rows][critic_obs_dim] */
  const float* noise;       /* [rows][num_actions], or NULL (in-kernel draw) */
  float* actions;           /* [rows][num_actions] out */
  float* st_obs;            /* storage slot [rows][obs_dim] out */
  float* st_critic_obs;     /* [rows][critic_obs_dim] out */
  float* st_actions;        /* [rows][num_actions] out */
  float* st_values;         /* [rows] out */
  float* st_log_prob;       /* [rows] out */
  float* st_mu;             /* [rows][num_actions] out */
  float* st_sigma;          /* [rows][num_actions] out */
  int32_t rows, obs_dim, critic_obs_dim, num_actions;
  int32_t noise_step;       /* (noise == NULL) the rollout step, in [0, ZBP_NOISE_STEPS): distinct draws per step */
  int32_t noise_seed;       /* (noise == NULL) the caller's stream, e.g. one per rank */
  zbp_obs_norm actor_norm;  /* the actor sees normalized obs (mean == NULL: none); st_obs stays raw */
  zbp_obs_norm critic_norm; /* the critic sees normalized critic_obs; st_critic_obs stays raw */
  int32_t log_std;          /* std_param holds log sigma (zbp_loss_cfg.log_std): the draw and the log-probability
                               use sigma = exp(std_param), and st_sigma receives sigma */
} zbp_act_io;
int zbp_act(const zbp_net* actor, const zbp_net* critic, const float* std_param, const zbp_act_io* io, float* ws,
            int32_t batch, void* stream);
/* PPO.process_env_step + the runner's episode statistics for one step (runner._rollout): storage
 * reward = reward (+ gamma * value where time_outs, rsl_rl's bootstrap; time_outs may be NULL),
 * storage done = done; cur_rew += reward, cur_len += 1, and over the envs with done > 0
 * ep_stats[0..2] += {sum cur_rew, sum cur_len, count} before their cur_rew / cur_len reset to 0.
 * rewards / values / cur_* [n] fp32, dones [n] int64, time_outs [n] uint8 (bool). One launch. */
int zbp_env_post(const float* rewards, const int64_t* dones, const uint8_t* time_outs, const float* values, float gamma,
                 float* st_rewards, float* st_dones, float* cur_rew, float* cur_len, float* ep_stats, int32_t n,
                 void* stream);
/* EmpiricalNormalization.update for one batch of `rows` >= 1 observations ([rows][dim], contiguous),
 * entirely on the device (no host sync: capturable between the env step and the next zbp_act). Per
 * normalizer, unless until >= 0 and count >= until:
 *   count += rows; rate = rows / count; delta = mean_x - mean; mean += rate * delta;
 *   var += rate * (var_x - var + delta * (mean_x - mean_new)); std = sqrt(var)
 * with mean_x / var_x the column mean and biased variance of the batch. Two launches: per-workgroup
 * two-pass partials (mean, sum of squared deviations) over fixed row ranges, then one workgroup per
 * normalizer that combines them around the batch mean in a fixed order and merges into the running
 * statistics -- fp64 inside, no atomics, bit-identical from run to run. Either normalizer may be NULL
 * (or have mean == NULL); with both and obs == critic_obs (same pointer and dim) the batch is read
 * once. scratch: zbp_norm_scratch_floats(rows) floats, 8-byte aligned, private to the call's stream. */
int64_t zbp_norm_scratch_floats(int32_t rows);
int zbp_norm_update(const zbp_obs_norm* actor, const zbp_obs_norm* critic, const float* obs, const float* critic_obs,
                    int32_t rows, float* scratch, void* stream);
const char* zbp_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* ZBOT_PPO_H */
