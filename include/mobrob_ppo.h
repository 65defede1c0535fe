/*
 * mobrob_ppo.h -- C ABI of libmobrob_ppo.so, the MI355X (gfx950) PPO training engine.
 *
 * Drop-in boundary for the ONE hot path of ZikangXiong/mobrob: everything that
 * `PPOCtrl.__init__ -> stable_baselines3.PPO(...)`  (reference src/mobrob/rl_control/ppo.py:50-59),
 * `PPOCtrl.learn -> PPO.learn`                       (reference src/mobrob/rl_control/ppo.py:73-74),
 * `PPOCtrl.save_model -> PPO.save`                   (reference src/mobrob/rl_control/ppo.py:76-77),
 * `load_policy -> PPO.load`                          (reference src/mobrob/utils.py:15-16) and
 * `policy.predict(obs, deterministic=True)`          (reference examples/control.py:39)
 * execute inside stable-baselines3 2.0.0 / torch-CPU (reference requirements.txt:9).
 * Each entry point below cites the reference call site / SB3 routine it replaces.
 *
 * Conventions
 *   - plain C types only; every pointer is a HOST pointer unless its name ends in `_dev`.
 *   - all arithmetic is IEEE float32 ("f32"); GAE carries its accumulator in f64 exactly like
 *     SB3's NumPy loop does (oracle/ppo_oracle.py:gae).
 *   - parameters travel as ONE flat f32 vector in SB3 `policy.state_dict()` order:
 *       log_std[A], pi.0.weight[H1,D], pi.0.bias[H1], pi.2.weight[H2,H1], pi.2.bias[H2],
 *       vf.0.weight[G1,D], vf.0.bias[G1], vf.2.weight[G2,G1], vf.2.bias[G2],
 *       action_net.weight[A,H2], action_net.bias[A], value_net.weight[1,G2], value_net.bias[1]
 *     (weights row-major [out,in]; verified against data/policies/<env>-ppo.zip:policy.pth).
 *     Other depths (one to eight hidden layers per network) continue nn.Sequential's numbering: pi.0, pi.2, pi.4 ... then vf.0 ...;
 *     with use_sde log_std is a matrix [HL,A] (HL = last policy width; [HL,1] without full_std), row-major, still first.
 *   - rollout storage is [T][N][...] on the device; minibatch indices are SB3's ENV-MAJOR flat
 *     index  flat = n*T + t  (SB3 RolloutBuffer.swap_and_flatten).
 *   - every function returns MOBROB_OK (0) or a negative error code; mobrob_ppo_last_error()
 *     returns a thread-local description.  Nothing here ever falls back to a CPU implementation.
 *   - ownership: the caller owns host buffers (pin them with mobrob_ppo_host_alloc for truly
 *     asynchronous H2D/D2H); the engine owns all device memory.
 */
#ifndef MOBROB_PPO_H
#define MOBROB_PPO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: config slot `persistent_train` became `activation`, `forward_x3` added, MOBROB_K_COUNT 6 -> 7 (profile_read arrays),
 *    MOBROB_BUF_COUNT / reserved[] resized -- a binding built against 1 must not load this library
 * 3: pi_hidden_ext / vf_hidden_ext (net_arch depths 4 .. 8), use_sde, sde_sample_freq appended to the config, activation codes 2 .. 11
 * (entry points added since -- the latest: mobrob_ppo_spec_monitor_moving with its own mobrob_spec_moving_t -- change no existing struct and no existing entry point: a binding
 *  built against an earlier 3 loads this library, so the number stays; a binding finds out whether a library has such an entry point by
 *  looking the symbol up) */
#define MOBROB_PPO_ABI_VERSION 3
/* policy_kwargs.activation_fn (SB3 ActorCriticPolicy; the reference splats ppo_kwargs into PPO verbatim, ppo.py:58): the
 * parameter-free element-wise torch.nn modules with torch's default arguments (ELU alpha 1, LeakyReLU slope 0.01, Softplus beta 1 /
 * threshold 20, Hardtanh [-1, 1], GELU approximate='none') */
enum { MOBROB_ACT_TANH = 0, MOBROB_ACT_RELU = 1, MOBROB_ACT_ELU = 2, MOBROB_ACT_LEAKY_RELU = 3, MOBROB_ACT_SIGMOID = 4,
       MOBROB_ACT_SOFTPLUS = 5, MOBROB_ACT_SOFTSIGN = 6, MOBROB_ACT_HARDTANH = 7, MOBROB_ACT_RELU6 = 8, MOBROB_ACT_SILU = 9,
       MOBROB_ACT_GELU = 10, MOBROB_ACT_MISH = 11, MOBROB_ACT_COUNT = 12 };

enum {
  MOBROB_OK = 0,
  MOBROB_ERR_INVALID = -1,     /* bad argument / unsupported shape (-> ValueError)            */
  MOBROB_ERR_HIP = -2,         /* a HIP runtime call failed (-> RuntimeError)                  */
  MOBROB_ERR_STATE = -3,       /* call sequence violated, e.g. train before finish_rollout     */
  MOBROB_ERR_NO_DEVICE = -4    /* no gfx950 device visible                                     */
};

typedef struct mobrob_ppo_engine mobrob_ppo_engine_t;

/* Hyper-parameters = the kwargs the reference splats into PPO(...) (ppo.py:58; data/configs/
 * <env>-ppo.yaml `ppo_kwargs`) plus SB3 2.0.0 defaults for the rest. */
typedef struct mobrob_ppo_config {
  int32_t abi_version;        /* = MOBROB_PPO_ABI_VERSION                                        */
  int32_t obs_dim;            /* D: 14 point, 26 car, 58 doggo, 12 drone, 43 turtlebot3          */
  int32_t act_dim;            /* A:  2,        2,      12,       18,       2                     */
  int32_t pi_hidden[2];       /* policy_kwargs.net_arch.pi  (default [64,64]); one hidden layer: [h, 0]; a third: pi_hidden3 below */
  int32_t vf_hidden[2];       /* policy_kwargs.net_arch.vf  (default [64,64]); likewise with vf_hidden3                         */
  int32_t n_envs;             /* N: vectorised envs owned by THIS rank (yaml n_envs)             */
  int32_t n_steps;            /* T: rollout horizon (ppo_kwargs.n_steps, default 2048)           */
  int32_t batch_size;         /* GLOBAL minibatch size (ppo_kwargs.batch_size, default 64)       */
  int32_t n_epochs;           /* ppo_kwargs.n_epochs (default 10)                                */
  /* python floats are doubles: the engine rounds to f32 exactly where SB3/torch would */
  double gamma;               /* default 0.99                                                    */
  double gae_lambda;          /* default 0.95                                                    */
  double clip_range;          /* constant schedule, default 0.2                                  */
  double ent_coef;            /* default 0.0                                                     */
  double vf_coef;             /* default 0.5                                                     */
  double max_grad_norm;       /* default 0.5                                                     */
  double learning_rate;       /* constant schedule, default 3e-4                                 */
  double adam_beta1, adam_beta2, adam_eps; /* 0.9, 0.999, 1e-5 (SB3 passes eps=1e-5 to Adam)     */
  double action_low, action_high; /* Box bounds used for the clipped action copy (-1, 1)         */
  int32_t normalize_advantage;/* default 1                                                       */
  uint64_t seed;              /* Philox key for eps / synthetic env / Feistel permutations       */
  int32_t device_id;          /* HIP device ordinal                                              */
  int32_t rank, world_size;   /* data-parallel position; batch_size is split batch_size/world    */
  int32_t fast_kernels;       /* 1: use the fused MFMA kernels when the shape allows; 0: generic */
  int32_t rollout_graph;      /* 1: the per-step device rollout (2 launches per step) is replayed as one
                                 captured hipGraph; the persistent rollout needs no graph          */
  int32_t rollout_persistent; /* 1: run the device-resident rollout as one persistent kernel (fused widths) */
  int32_t activation;         /* hidden activation of both networks: MOBROB_ACT_TANH (0; SB3's default for MlpPolicy, every
                                 reference YAML) or another MOBROB_ACT_* (policy_kwargs activation_fn; generic GEMM chain) */
  int32_t forward_x3;         /* 1 (default): the hidden-layer matrix products of 256-wide tanh nets -- rollout policy forward, batched value
                                 pass, and inside the gradient kernel the forward, dh1, dW2, dW1 -- run on the bf16 matrix pipe with every
                                 float32 operand split into three bf16 pieces and six piece products kept, float32 accumulation: float32
                                 RESULTS (error against float64 not larger than v_mfma_f32's, not bit-equal to it) at up to
                                 16/6 of the f32 matrix rate.  0: v_mfma_f32 everywhere.  Heads, loss, GAE, clip and Adam are plain float32
                                 either way; so are the 64-wide kernel families and the generic GEMM chain. */
  int32_t pi_hidden3;         /* width of a THIRD policy hidden layer (0: none).  net_arch depths 1 .. 8 are accepted per network (SB3 takes any
                                 list; the reference's YAMLs use two layers); depths other than two run the generic GEMM chain */
  int32_t vf_hidden3;         /* likewise for the value network */
  int32_t reserved[1];
  int32_t pi_hidden_ext[5];   /* widths of policy hidden layers 4 .. 8 (a width of 0 ends the list) */
  int32_t vf_hidden_ext[5];   /* likewise for the value network */
  int32_t use_sde;            /* PPO(use_sde=True): generalised state-dependent exploration (SB3 StateDependentNoiseDistribution with its
                                 defaults; full_std / use_expln below; no squashing, learn_features=False).  log_std becomes a [HL][A] matrix (HL =
                                 width of the last policy hidden layer); generic GEMM chain.  Default 0 */
  int32_t sde_sample_freq;    /* PPO(sde_sample_freq): new exploration matrices every this many rollout steps (-1: only at the start of a
                                 rollout, SB3's default) */
  int32_t sde_full_std;       /* policy_kwargs full_std (default 1): 0 = one standard deviation per latent unit, log_std is [HL][1] */
  int32_t sde_use_expln;      /* policy_kwargs use_expln (default 0): std = exp(ls) for ls <= 0, log1p(ls + 1e-6) + 1 above       */
} mobrob_ppo_config_t;

/* Fill `cfg` with SB3 2.0.0 defaults (Appendix A.1).  Replaces PPO.__init__'s default kwargs. */
void mobrob_ppo_default_config(mobrob_ppo_config_t* cfg);

/* PPO(...)/_setup_model (ppo.py:50-59): allocate rollout buffer, policy, Adam(eps) on the device;
 * parameters are initialised to zero -- the caller uploads weights (set_params). */
int mobrob_ppo_create(const mobrob_ppo_config_t* cfg, mobrob_ppo_engine_t** out);
void mobrob_ppo_destroy(mobrob_ppo_engine_t* e);

/* Mixed fleet (several robot types = several PPO(...) objects with different obs/act dims trained side by
 * side, the loop of examples/train.py:42-46 run once per env name): every device buffer of an engine is
 * carved out of ONE arena, so the ragged segments of a fleet pack back to back into one rollout allocation,
 * each with its own (obs_dim, act_dim) strides.  device_bytes is a host-only sizing pass (no device needed);
 * create_in_arena builds the engine inside caller-owned device memory (256-byte aligned, >= device_bytes),
 * which must outlive the engine.  mobrob_ppo_create == device_bytes + one private arena. */
int mobrob_ppo_device_bytes(const mobrob_ppo_config_t* cfg, size_t* bytes);
int mobrob_ppo_create_in_arena(const mobrob_ppo_config_t* cfg, void* arena, size_t arena_bytes,
                               mobrob_ppo_engine_t** out);
void* mobrob_ppo_device_alloc(int32_t device_id, size_t bytes);
void mobrob_ppo_device_free(void* p);
const char* mobrob_ppo_last_error(void);
int mobrob_ppo_abi_version(void);

/* Use an externally owned hipStream_t (e.g. torch's current stream, so that RCCL collectives
 * issued through torch.distributed are ordered with the engine's kernels).  NULL -> own stream. */
int mobrob_ppo_set_stream(mobrob_ppo_engine_t* e, void* hip_stream);
int mobrob_ppo_synchronize(mobrob_ppo_engine_t* e);

/* Pinned host memory for the rollout streamer (hipHostMalloc / hipHostFree). */
void* mobrob_ppo_host_alloc(size_t bytes);
void mobrob_ppo_host_free(void* p);
/* Pin and map caller-owned host memory in place (hipHostRegister, mapped + portable): afterwards the range is
 * accepted wherever host_alloc memory is (zero-copy act/store, act_part/store_part, collect_host).  Meant for the
 * POSIX shared-memory block that environment worker PROCESSES write their step results into -- the replacement of
 * the pipes between SubprocVecEnv workers and the learner (/root/reference/src/mobrob/rl_control/ppo.py:30-33 with
 * make_vec_env :37-48): `p` must stay mapped until host_unregister.  Fails (MOBROB_ERR_HIP) if the range cannot be
 * pinned or is not device visible at its host address. */
int mobrob_ppo_host_register(void* p, size_t bytes);
int mobrob_ppo_host_unregister(void* p);

/* policy.state_dict() / load_state_dict() (examples/train.py:31-33) and the optimizer state of
 * policy.optimizer.pth.  n must equal mobrob_ppo_param_count(). */
int64_t mobrob_ppo_param_count(const mobrob_ppo_engine_t* e);
int mobrob_ppo_get_params(mobrob_ppo_engine_t* e, float* out, int64_t n);
int mobrob_ppo_set_params(mobrob_ppo_engine_t* e, const float* in, int64_t n);
int mobrob_ppo_get_optimizer_state(mobrob_ppo_engine_t* e, float* exp_avg, float* exp_avg_sq, int64_t n,
                                   int64_t* step);
int mobrob_ppo_set_optimizer_state(mobrob_ppo_engine_t* e, const float* exp_avg, const float* exp_avg_sq,
                                   int64_t n, int64_t step);

/* ---- rollout: OnPolicyAlgorithm.collect_rollouts (SB3; reached via ppo.py:73-74) ------------- */

/* rollout_buffer.reset(): position -> 0. */
int mobrob_ppo_rollout_begin(mobrob_ppo_engine_t* e);

/* `actions, values, log_probs = policy(obs)` + np.clip for the env.  obs[N*D] is streamed H2D into
 * rollout slot t; eps[N*A] ~ N(0,I) may be NULL -> drawn on device (Philox4x32-10 + Box-Muller).
 * Outputs (any may be NULL): raw actions (what the buffer stores), clipped actions (what the env
 * sees), values, log_probs.  Blocks until the outputs are on the host. */
int mobrob_ppo_act(mobrob_ppo_engine_t* e, const float* obs, const float* eps, float* actions_raw,
                   float* actions_clipped, float* values, float* log_probs);

/* rollout_buffer.add(...) for the step just acted: rewards[N]; dones[N] (terminated|truncated,
 * becomes the NEXT step's episode_start); truncated[N] = infos["TimeLimit.truncated"] (may be
 * NULL); terminal_obs[N*D] = infos["terminal_observation"] rows (only rows with truncated!=0 are
 * read; may be NULL when nothing was truncated).  Applies rewards += gamma * V(terminal_obs). */
int mobrob_ppo_store(mobrob_ppo_engine_t* e, const float* rewards, const uint8_t* dones,
                     const uint8_t* truncated, const float* terminal_obs);

/* ---- pipelined host-environment rollout -------------------------------------------------------------------
 * Same results as act()/store() over all N rows, but the rows are cut into `nparts` contiguous ranges
 * [N*part/nparts, N*(part+1)/nparts) so that the host simulator steps one range while the GPU runs the policy for
 * another (the reference alternates strictly: SubprocVecEnv.step_async/step_wait after policy.forward,
 * ppo.py:30-33 + SB3 collect_rollouts).  Every pointer is the FULL [N][...] array in device-visible pinned memory
 * (mobrob_ppo_host_alloc); a call touches only the rows of its part.
 *   act_part    enqueue: pull the part's obs rows -> policy/value forward + sample -> push its clipped actions;
 *               returns without waiting
 *   wait_part   block until the clipped actions of the part's latest act_part are in actions_clipped
 *   store_part  enqueue rollout_buffer.add for the part (rewards, episode starts, time-limit bootstrap); with
 *               next_obs != NULL the same launch also pulls the part's next observations into slot t+1, so the
 *               following act_part launches the policy kernel only
 * Each part keeps its own step index (part p may act on step t+1 before part q has stored step t);
 * finish_rollout() requires every part to have stored n_steps steps.  nparts is fixed between rollout_begin()
 * and finish_rollout(), 1 <= nparts <= MOBROB_MAX_PARTS. */
#define MOBROB_MAX_PARTS 8
int mobrob_ppo_act_part(mobrob_ppo_engine_t* e, int32_t part, int32_t nparts, const float* obs,
                        float* actions_clipped);
int mobrob_ppo_wait_part(mobrob_ppo_engine_t* e, int32_t part);
int mobrob_ppo_store_part(mobrob_ppo_engine_t* e, int32_t part, int32_t nparts, const float* rewards,
                          const uint8_t* dones, const uint8_t* truncated, const float* terminal_obs,
                          const float* next_obs);

/* The whole pipelined rollout as ONE native call -- SB3's collect_rollouts loop (on_policy_algorithm.py, reached via
 * ppo.py:73-74) without a Python frame per step: rollout_begin, n_steps x nparts x (wait_part, step_range of the
 * part's envs, store_part + act_part), finish_rollout.  `step_range(env, i0, i1, actions, obs, rewards, dones,
 * truncated, terminal_obs)` steps the envs [i0, i1) of a vectorised environment over the FULL pinned arrays (VecEnv
 * semantics: auto-reset, terminal observation of truncated rows) and returns how many of them were truncated (< 0:
 * error).  csrc/host_env.c's mobrob_hostenv_step_range has exactly this signature.  `obs` must hold the current
 * observations (VecEnv.reset() or the previous rollout's last step) on entry and holds the last ones on return.
 *
 * SERVED form (the default where it applies): the step loop contains NO launch, event or other HIP call -- the persistent rollout kernel
 * of the device environments serves the host one (csrc/kernels_rollout.h KIND 3: k_rollout_persistent<.., 3, S8> for 256-wide engines
 * with the split-bf16 forward, k_rollout64_tile<.., 3> for the 64-wide networks of the reference YAMLs).  A workgroup writes its rows'
 * clipped actions into `actions_clipped`, raises a flag word in pinned memory and polls the host's word for its row range; this function
 * waits for the flags of a range, calls step_range on it and raises the range's word; V(obs) comes from the batched value pass.
 * Conditions: a fused engine of one of the two widths; row ranges of whole 32-row tiles (n_envs % (32 nparts) == 0) or ONE range of any
 * size (nparts == 1: the reference's 2 - 16 environments); at most one tile per compute unit; all six buffers in COHERENT pinned host
 * memory over their whole length (mobrob_ppo_host_alloc, or mobrob_ppo_host_register while HIP_HOST_COHERENT is not 0; a non-coherent
 * allocation is refused by name); no announced co-tenant of the device (MOBROB_DP_SAME_DEVICE ranks, a CU mask); every workgroup
 * resident within MOBROB_SERVER_RESIDENCY_S (default 2 s) -- otherwise, and with MOBROB_COLLECT_SERVER=0, the launch-per-step form runs
 * (=2: fail instead, naming the reason).  256-wide: numbers agree with the launch-per-step form to float32 rounding (policy forward on
 * the other matrix pipe); 64-wide: bit for bit.  Every wait on either side is bounded (MOBROB_SERVER_TIMEOUT_S, default 60: the call
 * fails, the queued launches return at once). */
typedef int32_t (*mobrob_env_step_range_fn)(void* env, int32_t i0, int32_t i1, const float* actions, float* obs,
                                            float* rewards, uint8_t* dones, uint8_t* truncated, float* terminal_obs);
int mobrob_ppo_collect_host(mobrob_ppo_engine_t* e, mobrob_env_step_range_fn step_range, void* env, int32_t nparts,
                            float* obs, float* actions_clipped, float* rewards, uint8_t* dones, uint8_t* truncated,
                            float* terminal_obs);

/* `values = policy.predict_values(new_obs)` + RolloutBuffer.compute_returns_and_advantage
 * (GAE(lambda) reverse scan).  last_obs[N*D], dones[N] = dones of the final step. */
int mobrob_ppo_finish_rollout(mobrob_ppo_engine_t* e, const float* last_obs, const uint8_t* dones);

/* Device-resident synthetic env source (SURVEY.md §8d / BASELINE.md §3): the whole T-step rollout
 * (env draw -> act -> store -> bootstrap) runs on the GPU without host round trips, then GAE.
 * obs ~ N(0,1), reward ~ N(0.03,0.1^2) + 5*terminated, terminated ~ Bernoulli(p_term),
 * truncation at time_limit with a terminal observation.  State persists across calls. */
int mobrob_ppo_collect_synthetic(mobrob_ppo_engine_t* e, float p_term, int32_t time_limit);

/* Device-resident GOAL environment: the reference's env-side rules evaluated on the GPU inside the rollout
 * loop -- reward_fn (src/mobrob/envs/wrapper.py:137-154, drone bonus :491-496), step/terminate_on_goal
 * (:156-171), lazy reset + new goal (:173-201), reached (:203-207), TimeLimit truncation as get_env wraps it
 * (:549-571), VecEnv auto-reset with terminal observation and the time-limit bootstrap.  The robot itself is
 * the kinematic stand-in of mobrob_amd/envs/wrapper.py (the reference's MuJoCo / Bullet physics is out of
 * scope): vel <- 0.8 vel + 0.2 mix.clip(a); pos <- clip(pos + dt vel, +-extent); observation =
 * [unit vector to the goal, vel, pos, N(0, obs_noise^2) padding].  init_space = +-extent/2, goal_space =
 * +-extent.  State persists across calls; switching between env kinds restarts the environments. */
typedef struct mobrob_goal_env {
  int32_t pos_dim;            /* 1..3, 3*pos_dim <= obs_dim                                              */
  int32_t terminate_on_goal;  /* PPOCtrl passes True (ppo.py:37-48)                                      */
  int32_t time_limit;         /* max_episode_steps                                                       */
  float dt, extent;
  float reach_radius;         /* 0.3 in the reference                                                    */
  float goal_bonus;           /* +5 on reach                                                             */
  float extra_bonus;          /* +10 more for the drone                                                  */
  float obs_noise;            /* std of the padding features                                             */
  float mix[3][32];           /* [pos_dim][act_dim] action -> velocity command read-out                  */
} mobrob_goal_env_t;
int mobrob_ppo_collect_goal_env(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env);

/* Monitor-style statistics of the episodes the goal environment finished since the last reset of the
 * counters (SB3's rollout/ep_rew_mean, ep_len_mean).  Waits for the engine's stream. */
typedef struct mobrob_episode_stats {
  int64_t episodes;
  double return_sum, length_sum;
  int64_t goals;              /* episodes that ended inside the reach radius */
} mobrob_episode_stats_t;
int mobrob_ppo_episode_stats(mobrob_ppo_engine_t* e, mobrob_episode_stats_t* out, int32_t reset);
/* The Monitor records SB3 keeps in `ep_info_buffer` (what `rollout/ep_rew_mean` averages and PPO.save stores):
 * (return, length) of the episodes the device goal environment finished since the previous call, oldest first,
 * newest `max_records` at most (the device keeps the last 128).  out = [max_records][2] floats; returns the count. */
int mobrob_ppo_episode_records(mobrob_ppo_engine_t* e, float* out, int32_t max_records);

/* ---- update: PPO.train (SB3 ppo/ppo.py) ----------------------------------------------------- */

typedef struct mobrob_ppo_train_stats {
  /* means over the minibatches of the LAST epoch run by the call (SB3 logs the same way) */
  float policy_loss, value_loss, entropy_loss, loss, approx_kl, clip_fraction, grad_norm;
  int32_t n_minibatches; /* optimizer steps taken by the call */
} mobrob_ppo_train_stats_t;

/* ---- data-parallel update: one process per GPU, rank r owns its envs and rollout shard ------------
 * PPO.train() of the reference (reached through PPOCtrl.learn, /root/reference/src/mobrob/rl_control/ppo.py:73-74)
 * across `cfg.world_size` ranks: per epoch ONE all-reduce of the [n_minibatches][4] float64 advantage statistics, per
 * optimizer step ONE all-reduce (sum) of the flat [P + 8] float32 gradient + loss sums, both enqueued on the engine's stream between
 * the kernels -- no host synchronisation and no interpreter in the loop.  Every rank then applies the identical
 * clip + Adam, so replicas stay bit-identical.  batch_size in the config is the GLOBAL minibatch.
 *   comm_unique_id  rank 0 makes the 128-byte RCCL id; the caller ships it to the other ranks (any side channel)
 *   comm_init       collective: ncclCommInitRank(world_size, id, rank) -> the engine's communicator (RCCL over xGMI)
 *   train_dp        the loop.  fn == NULL: RCCL on the communicator.  fn != NULL: the caller's all-reduce, called with
 *                   (ctx, device pointer, element count, dtype 0 = f32 / 1 = f64, hipStream_t of the engine); it must
 *                   leave the SUM over ranks in place, ordered after prior work on that stream, and return 0
 *                   (tests: gloo between two ranks that share one GPU). */
typedef int (*mobrob_allreduce_fn)(void* ctx, void* buf_dev, size_t count, int32_t dtype, void* hip_stream);
int mobrob_ppo_comm_unique_id(uint8_t* out128);
/* comm_prepare  LOCAL, non-collective half of comm_init: RCCL loadable, device selectable, no communicator yet.  Ranks
 *               agree on its outcome (any side channel) BEFORE any of them enters the blocking ncclCommInitRank, so a
 *               rank that cannot take part never leaves the others waiting for it.
 * comm_init_rank  comm_init with the rank / size of the process (sub)group the communicator spans; nranks must equal
 *               cfg.world_size (the minibatch split).  comm_init == comm_init_rank(cfg.rank, cfg.world_size).
 * comm_info     ncclCommCount / ncclCommUserRank of the engine's communicator (0 / -1 without one): what a bench line
 *               reports as the number of ranks that really took part in the collectives. */
int mobrob_ppo_comm_prepare(mobrob_ppo_engine_t* e);
int mobrob_ppo_comm_init(mobrob_ppo_engine_t* e, const uint8_t* id128);
int mobrob_ppo_comm_init_rank(mobrob_ppo_engine_t* e, const uint8_t* id128, int32_t rank, int32_t nranks);
int mobrob_ppo_comm_info(mobrob_ppo_engine_t* e, int32_t* nranks, int32_t* rank);
int mobrob_ppo_comm_destroy(mobrob_ppo_engine_t* e);
/* SB3's target_kl works under data parallel too: the minibatch's approx_kl sum travels with the gradient (the message
 * is [P + 8] floats: gradient + loss sums), every rank reads the same global value and stops at the same step. */
int mobrob_ppo_train_dp(mobrob_ppo_engine_t* e, const int64_t* perms, mobrob_allreduce_fn fn, void* ctx);
/* ---- one-shot all-reduce over peer-mapped memory (opt-in; RCCL stays the default) ------------------------------------
 * The gradient message of a PPO step is 645 KB: latency-bound on the xGMI mesh, where a direct exchange (every rank
 * reads every peer's contribution and adds them up itself, IN RANK ORDER -> the same bits on every rank, deterministic
 * run to run) beats a ring.  Every rank exports an exchange buffer with hipIpcGetMemHandle; the handles travel over any
 * side channel; every rank opens the others' (hipIpcOpenMemHandle: over xGMI between GPUs, the same physical memory for
 * two ranks that share a device).  Afterwards train_dp(fn == NULL) exchanges through it instead of RCCL: one launch per
 * message, per-16-KB-chunk sequence flags with system-scope release / acquire (csrc/oneshot_allreduce.h).  A peer that
 * never publishes raises an error at the next synchronising call (MOBROB_ONESHOT_TIMEOUT_MS, default 20 s) instead of
 * hanging the device.
 *   oneshot_export  allocate the exchange buffer (once) and write its IPC handle (MOBROB_IPC_HANDLE_BYTES bytes)
 *   oneshot_open    handles = [nranks][MOBROB_IPC_HANDLE_BYTES] in rank order (the own entry is ignored)
 *   oneshot_close   unmap the peers, free the buffer (also done by destroy) */
#define MOBROB_IPC_HANDLE_BYTES 64
int mobrob_ppo_oneshot_export(mobrob_ppo_engine_t* e, uint8_t* handle64);
int mobrob_ppo_oneshot_open(mobrob_ppo_engine_t* e, const uint8_t* handles, int32_t rank, int32_t nranks);
int mobrob_ppo_oneshot_close(mobrob_ppo_engine_t* e);
/* Known vectors through the exchange train_dp would use, compared with the rank-ordered sums: run at communicator set-up (collective),
 * before any gradient depends on the exchange.  which: 0 = the engine's RCCL communicator, 1 = the one-shot exchange.  Four
 * messages: the [P + 8]-float gradient message twice and the [n_minibatches][4]-double advantage message twice (both payload slots
 * of the one-shot exchange, slot reuse, both element types), on a scratch buffer of the call's own; MOBROB_ERR_STATE while an
 * epoch is open or a gradient awaits its apply.
 * *mismatches = elements over the four messages that are not bit-equal to the expected sum; 0 = sound.  The reference has one
 * exchange path and trusts it (SubprocVecEnv pipes, /root/reference/src/mobrob/rl_control/ppo.py:30-33); here a peer-mapped
 * exchange is used on real peers only after it has passed, RCCL otherwise (mobrob_amd/parallel.py). */
int mobrob_ppo_exchange_selfcheck(mobrob_ppo_engine_t* e, int32_t which, int32_t* mismatches);
/* all-reduces issued by train_dp since the last reset: how many, and their payload bytes (bench: allreduces_per_step) */
int mobrob_ppo_allreduce_counters(mobrob_ppo_engine_t* e, int64_t* calls, int64_t* bytes, int32_t reset);

/* ---- env-side controllers of the Bullet robots, batched over n robots on the device (csrc/robot_ctrl.h) ----------
 * In the reference the RL action of these two robots corrects controller GAINS and the controller runs inside
 * env.step on the host, one robot at a time.  dev_ptrs != 0: every array pointer is a DEVICE pointer and the call
 * only enqueues the kernel on the engine's stream (a device-resident simulator calls it between physics steps);
 * dev_ptrs == 0: host arrays, copied in and out, the call returns when the results are in place.
 *   turtlebot3  `Turtlebot3.prop_ctrl` (robots/turtlebot3.py:214-238, from Turtlebot3Env.step, envs/wrapper.py:540-546):
 *               pos[n][2], theta[n], goal[n][2], gain_changes[n][2] (the action) -> twist[n][2] = (v, w)
 *   drone       `DronePIDController.control` with `finetune_*_pid_coef` (robots/drone.py:58-159, 175-193, from
 *               DroneEnv.step, envs/wrapper.py:481-489): pos[n][3], rpy[n][3], goal[n][3], action[n][18] (6 x 3 gain
 *               corrections: force P I D, torque P I D), ctrl_state[n][12] in/out (last position error, its integral,
 *               last attitude error, its integral) -> out[n][4] = thrust, torque x y z.  The rotor mixing
 *               (`_compute_rpm`) belongs to Bullet's actuator model and is not part of it. */
typedef struct mobrob_drone_params {
  float mass, g, dt;                                   /* kg, m/s^2, controller period (world.timestep = 1/50) */
  float max_thrust, max_xy_torque, max_z_torque;       /* actuator limits (drone.py:260-267) */
  float max_roll_pitch;                                /* attitude limit, pi/6 in the reference (drone.py:50) */
  float tune_fac;                                      /* gain radius = tune_fac * default gain, 0.3 (drone.py:29) */
} mobrob_drone_params_t;
int mobrob_ctrl_turtlebot3(mobrob_ppo_engine_t* e, int32_t n, int32_t dev_ptrs, const float* pos, const float* theta,
                           const float* goal, const float* gain_changes, float* twist);
int mobrob_ctrl_drone_pid(mobrob_ppo_engine_t* e, int32_t n, int32_t dev_ptrs, const mobrob_drone_params_t* prm,
                          const float* pos, const float* rpy, const float* goal, const float* action, float* ctrl_state,
                          float* out);

/* Hyper-parameters that SB3 lets change or that the reference YAMLs never set, without growing the config struct.
 * `ppo_kwargs` are splatted into stable_baselines3.PPO verbatim (/root/reference/src/mobrob/rl_control/ppo.py:58, README.md:49):
 *   LEARNING_RATE / CLIP_RANGE  the value of a schedule for the coming PPO.train() (SB3 evaluates callables of
 *                               `progress_remaining` once per train())
 *   CLIP_RANGE_VF               value-function clipping: the loss uses old_value + clamp(value - old_value, +-c);
 *                               negative = None (default)
 *   TARGET_KL                   early stop: when a minibatch's approx_kl > 1.5 * target, its optimizer step and the rest
 *                               of train() are dropped (train and train_dp alike); <= 0 = None (default)
 *   ENT_COEF / VF_COEF          loss coefficients */
enum {
  MOBROB_HYPER_LEARNING_RATE = 0, MOBROB_HYPER_CLIP_RANGE = 1, MOBROB_HYPER_CLIP_RANGE_VF = 2, MOBROB_HYPER_TARGET_KL = 3,
  MOBROB_HYPER_ENT_COEF = 4, MOBROB_HYPER_VF_COEF = 5,
  MOBROB_HYPER_EPOCH_KERNEL = 6   /* not an SB3 keyword: 0 keeps three launches per optimizer step where mobrob_ppo_train would run an
                                     epoch as one co-operative launch (csrc/kernels_epoch64.h; the env MOBROB_EPOCH_KERNEL=0 does the
                                     same for every engine of the process).  Engines that update CONCURRENTLY on one device (a fleet's
                                     segments) set 0: co-resident spinning launches must fit the device together. */
};
int mobrob_ppo_set_hyper(mobrob_ppo_engine_t* e, int32_t which, double value);
/* Of the latest mobrob_ppo_train / train_enqueue: epochs started (SB3's `_n_updates` increment), whether target_kl
 * stopped it, optimizer steps applied. */
int mobrob_ppo_last_train_info(const mobrob_ppo_engine_t* e, int32_t* epochs_started, int32_t* stopped_early,
                               int32_t* steps_applied);

/* Whole PPO.train(): n_epochs x ceil(T*N / batch) optimizer steps.  perms = n_epochs concatenated
 * env-major permutations of range(T*N) (what np.random.permutation would have produced), or NULL ->
 * counter-based Feistel permutations keyed by (seed, rank, update counter).  world_size must be 1. */
int mobrob_ppo_train(mobrob_ppo_engine_t* e, const int64_t* perms, mobrob_ppo_train_stats_t* stats);
/* Same update, enqueued on the engine's stream without waiting for it (mobrob_ppo_train == train_enqueue +
 * statistics read-back).  Lets the engines of a mixed fleet overlap their updates on one GPU; `perms`, when
 * given, must stay valid until mobrob_ppo_synchronize. */
int mobrob_ppo_train_enqueue(mobrob_ppo_engine_t* e, const int64_t* perms);

/* The same update split at the two points where data-parallel ranks exchange data:
 *   epoch_begin   -> local (sum adv, sum adv^2, count) per minibatch into advstat_dev
 *   [all-reduce advstat_dev, 3 doubles per minibatch]
 *   minibatch_grad(mb) -> local gradient of the GLOBAL-mean loss into grad_dev (P floats)
 *   [all-reduce grad_dev (sum)]
 *   minibatch_apply -> clip_grad_norm_ + Adam.step on every rank (replicas stay identical)
 * `perm` (also every row of `perms` of mobrob_ppo_train / _train_dp / _train_enqueue) must be a PERMUTATION of [0, T*N) in SB3's env-major
 * flat order (index = n * T + t): it is validated on the host -- every index in range, none twice -- and MOBROB_ERR_INVALID is returned
 * before any kernel scatters through it.  NULL: the engine draws its own (a keyed Feistel permutation on the device). */
int mobrob_ppo_epoch_begin(mobrob_ppo_engine_t* e, const int64_t* perm /* T*N or NULL */);
int mobrob_ppo_num_minibatches(const mobrob_ppo_engine_t* e);
int mobrob_ppo_minibatch_grad(mobrob_ppo_engine_t* e, int32_t mb);
int mobrob_ppo_minibatch_apply(mobrob_ppo_engine_t* e);
/* minibatch_apply with SB3's target_kl check in front of the optimizer step (the approx_kl of the -- all-reduced --
 * loss sums is read back, 4 bytes): *stopped = 1 means the step was NOT taken and the driver must end its train().
 * minibatch_apply itself refuses (MOBROB_ERR_STATE) while target_kl is set, so that no step-wise driver ignores it. */
int mobrob_ppo_minibatch_apply_checked(mobrob_ppo_engine_t* e, int32_t* stopped);
/* per-minibatch stats of every optimizer step since the last call to this function:
 * rows of 8 floats [policy_loss, value_loss, entropy_loss, loss, approx_kl, clip_fraction,
 * grad_norm, 0]; returns rows written (<= max_rows) or a negative error. */
int mobrob_ppo_fetch_step_stats(mobrob_ppo_engine_t* e, float* out, int32_t max_rows);

/* ---- inference: policy.predict (examples/control.py:39) -------------------------------------- */
/* (use_sde engines, deterministic = 0: `eps` is not used -- the noise is latent . exploration matrix, SB3's get_noise: the
 *  environments' own matrices when n == n_envs, the single exploration_mat otherwise) */
int mobrob_ppo_predict(mobrob_ppo_engine_t* e, const float* obs, int32_t n, int32_t deterministic,
                       const float* eps /* n*A or NULL */, float* actions_clipped, float* values);

/* ---- evaluation: SB3 evaluate_policy / examples/control.py:36-46 on the device goal environment ----------------------
 * n_robots independent robots of the goal environment above, driven by the CURRENT policy, all on the device:
 *   start     every robot starts from a fresh reset -- pose from init_space, new goal (reference examples/control.py:37).
 *   stepping  action, then the env step of mobrob_ppo_collect_goal_env (src/mobrob/envs/wrapper.py:156-171); on termination
 *             (goal reached and terminate_on_goal) or truncation (env->time_limit steps; 0 = no limit, the control.py protocol)
 *             the robot resets (wrapper.py:173-201, control.py:41-44): a robot that reached its goal keeps its pose (lazy reset).
 *   actions   deterministic = 1: clip(mean) (policy.predict(obs, deterministic=True), control.py:39); 0: clip(mean + exp(log_std)
 *             N(0,1)) from the evaluation's stream (refused for use_sde).
 *   robot_out [n_robots][4] doubles: reward sum over all steps run, steps run, episodes finished, goals reached.  Rewards are
 *             summed in float64, as SB3's evaluate_policy (`current_rewards += rewards`) and control.py (`cum_reward += r`) do.
 *   episodes  0: every robot runs exactly max_steps steps (control.py).  > 0: the total number of episodes (SB3 n_eval_episodes);
 *             robot i finishes quota[i] episodes -- or, with quota = NULL, SB3's split (episodes + i) / n_robots
 *             (evaluate_policy's episode_count_targets) -- and idles afterwards (max_steps still bounds it).  Needs
 *             time_limit > 0 (MOBROB_ERR_INVALID otherwise: such a run might never finish).
 *   episode_out [n_robots][max_i quota[i]][3] doubles, or NULL: (return, length, success) of the first quota[i] episodes of
 *             robot i, in order; success = the episode ended inside the reach radius (wrapper.py:203-207).  Records beyond an
 *             unfinished quota are zero.
 *   trace_out [trace_steps][trace_robots][9 + obs_dim + act_dim + 4] floats, or NULL (tests: teacher forcing): per step and robot
 *             pos[3] vel[3] goal[3] BEFORE the step, the observation the policy saw, the action applied, the reward, and the
 *             flags reached, terminated, truncated (1.0 / 0.0).  Rows of robots that idle are zero.
 *   streams   the evaluation's own Philox streams (stream constants of its own, key = seed; counter = (robot, component, step)):
 *             it never reads nor advances the engine's draw counter, env step base, env state, episode statistics / records,
 *             rollout, training or gSDE buffers -- evaluating between any two calls leaves training bit-identical.
 *   ordering  enqueued on the engine's stream (it sees the parameters of any pending train_enqueue); reads the flat f32
 *             parameter vector; returns after the results are copied out.  Its device buffers are allocated on first use, grown
 *             when needed and freed by mobrob_ppo_destroy; they are outside the engine's arena (mobrob_ppo_device_bytes and
 *             mobrob_ppo_create_in_arena are unchanged).
 *   kernels   2x64 tanh engines of the fused family: ONE persistent launch (k_goal64_tile); every other engine: the engine's
 *             forward plus one kernel per step (k_goal_task_step).  MOBROB_EVAL_PERSISTENT=0 forces the per-step path.
 * Returns 1 when the persistent kernel ran, 0 for the per-step path, or a negative error. */
typedef struct mobrob_eval_spec {
  int32_t n_robots;        /* >= 1, independent of the engine's n_envs                                        */
  int32_t max_steps;       /* hard bound on steps per robot                                                   */
  int32_t episodes;        /* 0: run every robot for exactly max_steps (control.py protocol);
                              > 0: episode quota (SB3 evaluate_policy), robot idles after its share            */
  int32_t deterministic;   /* 1: clip(mean); 0: mean + exp(log_std) * N(0,1), clipped (refused for use_sde)      */
  uint64_t seed;           /* Philox key of the evaluation streams                                            */
  int32_t trace_robots, trace_steps;   /* optional teacher-forcing trace of the first robots / steps (tests)    */
} mobrob_eval_spec_t;
int mobrob_ppo_evaluate_goal_env(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_eval_spec_t* spec,
                                 const int32_t* quota /* [n_robots] or NULL */, double* robot_out /* [n_robots][4] */,
                                 double* episode_out /* [n_robots][max quota][3] or NULL */, float* trace_out /* or NULL */);

/* ---- waypoint following: the trained policy as a low-level tracker of given goal sequences (planner waypoints) ------------
 * n_robots independent robots of the goal environment above, driven by the CURRENT policy along goals given by the caller instead
 * of goals drawn from the RNG.  Per robot i (the host loop of mobrob_amd/waypoints.py states the same thing on EnvWrapper):
 *   start     at rest on start[i], goal waypoints[i][0] (EnvWrapper.reset(init_pos=start); set_goal(wp[0])).
 *   stepping  action, then the env step of mobrob_ppo_collect_goal_env with NO time limit and NO reset (env->time_limit and
 *             env->terminate_on_goal play no part).  After the step, if the robot is inside the reach radius (tested once per
 *             step, after the step: a robot starting inside the radius of wp[0] counts after its first step), arrival[i][k] =
 *             t + 1 and waypoint k + 1 becomes the goal (pose and velocity kept; progress is measured against the goal in force).
 *             At most one waypoint advances per step.  After its last waypoint the robot has finished and idles.
 *   n_waypoints [n_robots] counts (0 .. max_waypoints), or NULL = max_waypoints each.  A robot with 0 waypoints runs no step.
 *             Waypoints outside the arena's +-extent are allowed (unreachable); non-finite starts or waypoints are refused.
 *   arrival   [n_robots][max_waypoints] int32: arrival step (1-based) of each waypoint, -1 = not reached.
 *   robot_out [n_robots][4] doubles: reward sum (float64, reach bonus included), steps run, waypoints reached, final distance to
 *             the waypoint in force (NaN for a robot without waypoints).
 *   path_out  [max_steps / path_stride + 1][n_robots][pos_dim] floats, or NULL (path_stride 0: none): record r is the position
 *             after r * path_stride steps (record 0 = start); a robot that has finished repeats its last position.
 *   trace_out as mobrob_ppo_evaluate_goal_env's, the four flags being: reward, reached, index of the waypoint in force before
 *             the step, finished after the step.  Rows of robots that have finished are zero.
 *   actions, streams, ordering, buffers and kernels: as mobrob_ppo_evaluate_goal_env (the evaluation's Philox streams keyed by
 *             seed; nothing of the training state is read or advanced).  2x64 tanh engines of the fused family: ONE persistent
 *             launch (k_goal64_tile); every other engine: forward plus one kernel per step.  MOBROB_EVAL_PERSISTENT=0 forces
 *             the per-step path.
 * MOBROB_ERR_INVALID before any launch for: a count outside 0 .. max_waypoints, max_waypoints < 1, a pos_dim / act_dim that
 * evaluate refuses, max_steps < 1, path_stride < 0, a trace larger than the run, stochastic actions of a use_sde engine, non-finite
 * starts or (used) waypoints.  Returns 1 when the persistent kernel ran, 0 for the per-step path, or a negative error. */
typedef struct mobrob_follow_spec {
  int32_t n_robots;        /* >= 1                                                                            */
  int32_t max_waypoints;   /* K >= 1: the row stride of waypoints / arrival                                   */
  int32_t max_steps;       /* steps per robot at most                                                         */
  int32_t deterministic;   /* 1: clip(mean); 0: mean + exp(log_std) * N(0,1), clipped (refused for use_sde)      */
  uint64_t seed;           /* Philox key of the evaluation streams                                            */
  int32_t path_stride;     /* 0: no path; > 0: a path record every path_stride steps                          */
  int32_t trace_robots, trace_steps;   /* optional teacher-forcing trace of the first robots / steps (tests)    */
} mobrob_follow_spec_t;
int mobrob_ppo_follow_waypoints(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                const float* start /* [n][pos_dim] */, const float* waypoints /* [n][K][pos_dim] */,
                                const int32_t* n_waypoints /* [n] or NULL = K */, int32_t* arrival /* [n][K], -1 = not reached */,
                                double* robot_out /* [n][4] */, float* path_out /* or NULL */, float* trace_out /* or NULL */);

/* ---- hazard costs: the reference Engine's constrain_hazards rule on evaluation and waypoint following ----------------------
 * Hazards are circles on the floor (vertical cylinders; src/mobrob/envs/mujoco_robots/robots/engine.py: config :230-244, rule
 * :1329-1345, dist_xy :1037-1043).  After every env step, at the robot's new position p (before any reset), over the hazards
 * (x, y, r) of the robot's scene:
 *   d_h = |p_xy - h_xy| (x and y only, every robot, the 3-D drone included); cost = sum over d_h <= r_h of cost * (r_h - d_h);
 *   indicator: cost = (cost > 0).  A hazard exactly on whose boundary the robot stands contributes 0.  clearance = min_h (d_h - r_h),
 *   +inf for an empty scene.  The cost never changes dynamics, reward, reaching, termination or reset.
 *   Distances are float32 with a correctly rounded sqrt; the step cost is summed in float over four partial sums (hazards
 *   h = q mod 4) combined as (p0 + p1) + (p2 + p3), the same bits on both kernel paths.
 * mobrob_ppo_evaluate_goal_env_hazards / mobrob_ppo_follow_waypoints_hazards return what their counterparts return, in the same
 * arrays with the same meaning, streams and checks, and in addition:
 *   hazard_out [n_robots][4] doubles: cost summed in float64 over the steps run, steps with cost > 0, the first such step
 *             (1-based, as arrival) or -1, minimum clearance over every post-step position (+inf for an empty scene, NaN for a
 *             robot that ran no step).
 *   episode_cost_out [n_robots][max quota] doubles, or NULL (evaluate only): the cost of each recorded episode, beside episode_out.
 *   trace_out the counterpart's row plus two floats, the step's cost and clearance: width 9 + obs_dim + act_dim + 4 + 2.
 *   kernels   k_goal64_tile<DP, HazardTask<...>> (the check on all 64 lanes: four per robot; a shared scene staged in LDS) or the
 *             per-step path with k_goal_task_step<HazardTask<...>>.  max_hazards = 0 gives exactly the counterpart's results plus
 *             zero costs.
 * MOBROB_ERR_INVALID before any launch, besides the counterpart's checks, for: n_scenes < 1, max_hazards outside 0 .. 1024, a count
 * outside 0 .. max_hazards, scene NULL with n_scenes > 1, a scene entry outside 0 .. n_scenes - 1, a non-finite coordinate or
 * radius, a negative radius, a cost that is negative or not finite. */
typedef struct mobrob_hazards {
  int32_t n_scenes;          /* S >= 1                                                  */
  int32_t max_hazards;       /* M, row stride, 0 .. 1024                                */
  const float* hazards;      /* [S][M][3]: x, y, radius (radius >= 0, finite)           */
  const int32_t* n_hazards;  /* [S] counts 0 .. M, or NULL = M                          */
  const int32_t* scene;      /* [n_robots] scene of each robot, or NULL (needs S == 1)  */
  float cost;                /* hazards_cost, >= 0                                      */
  int32_t indicator;         /* constrain_indicator                                     */
} mobrob_hazards_t;
int mobrob_ppo_evaluate_goal_env_hazards(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_eval_spec_t* spec,
                                         const mobrob_hazards_t* hz, const int32_t* quota /* [n_robots] or NULL */,
                                         double* robot_out /* [n_robots][4] */, double* episode_out /* or NULL */,
                                         double* hazard_out /* [n_robots][4] */, double* episode_cost_out /* or NULL */,
                                         float* trace_out /* or NULL */);
int mobrob_ppo_follow_waypoints_hazards(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                        const mobrob_hazards_t* hz, const float* start /* [n][pos_dim] */,
                                        const float* waypoints /* [n][K][pos_dim] */, const int32_t* n_waypoints /* or NULL */,
                                        int32_t* arrival /* [n][K] */, double* robot_out /* [n][4] */,
                                        double* hazard_out /* [n][4] */, float* path_out /* or NULL */, float* trace_out /* or NULL */);

/* ---- resumable waypoint following: a RUN of calls with carried state, leg budgets and replanning between calls ----------------
 * A planner works in rounds: track for a horizon, look where the robots are, replan the stuck ones, continue (the loops around
 * the tracker in the reference's planners; the tracker itself is examples/control.py:36-46, EnvWrapper.set_goal / reached
 * wrapper.py:203-214).  mobrob_ppo_follow_waypoints_resume is mobrob_ppo_follow_waypoints (with hazards when hz is not NULL) as
 * ONE CALL OF A RUN: a sequence of calls over the same n_robots with the same seed, call c covering the global steps
 * step0 .. step0 + max_steps - 1 (the host loop of mobrob_amd/waypoints.py states the same thing on EnvWrapper).
 *   streams   every Philox draw (observation noise, action noise) is keyed by (robot, GLOBAL step); arrival steps and a first
 *             violation step are global and 1-based.
 *   carried   per robot, read at entry and continued (never re-summed), written at exit:
 *               resume->state [n][6] floats: position, velocity (unused components zero);
 *               robot_out [n][0..2]: float64 reward sum, steps run, waypoints reached = the index k of the waypoint in force
 *               ([3], the final distance, is output only);  arrival [n][K];  resume->leg_used [n]: steps spent on the waypoint in
 *               force;  with hazards, hazard_out [n][4].
 *   goal      at entry the goal in force is waypoints[n][k] (the last waypoint for a finished robot).
 *   budget    leg_steps = 0: none.  Otherwise, after a step: on arrival (arrival[k] = g + 1, k += 1, next waypoint) leg_used = 0,
 *             else leg_used += 1.  A robot is active iff k < n_waypoints[n] and (leg_steps == 0 or leg_used < leg_steps).
 *             Without a budget nothing is counted (leg_used stays 0), and leg_used must lie in 0 .. leg_steps at entry: a run
 *             that used a budget goes on without one (leg_steps = 0) only after the caller has zeroed leg_used.
 *   status    resume->status [n], written at exit: 0 going (the call's step cap ended it), 1 finished, 2 stalled (budget spent),
 *             3 no waypoints.
 *   replan    between calls the caller may replace any robot's waypoint row and count; it then sets that robot's reached count to
 *             0, its arrival row to -1 and leg_used to 0.  Everything else is carried.
 *   local     path_out and trace_out are the call's own: path record 0 is the position at entry, trace rows are indexed by the
 *             call's step, the waypoint flag holds k as carried; the rows of idle (finished, stalled) robots are zero.
 * Two invariants: a run started with step0 = 0, state = (start, 0), zeroed robot_out, arrival = -1, leg_used = 0, leg_steps = 0
 * (and hazard_out = 0, 0, -1, NaN) returns the bits of mobrob_ppo_follow_waypoints(_hazards) in every output; and one call of T
 * steps and any chain of calls of T1 + T2 + ... = T steps handing the carried arrays on unchanged end with bit-identical carried
 * arrays on the same kernel path (k_goal64_tile<DP, ResumeFollowTask> / HazardTask<ResumeFollowTask>, or the per-step kernels).
 * MOBROB_ERR_INVALID before any launch or copy (the in/out arrays stay as given), besides the counterpart's checks, for: a NULL
 * resume / state / leg_used / status, hazard_out NULL unless hz is, step0 < 0 or step0 + max_steps beyond int32, leg_steps < 0, a
 * non-finite state, leg_used outside 0 .. leg_steps, a reached count outside 0 .. n_waypoints[n], a non-finite carried reward
 * sum, carried steps outside 0 .. INT32_MAX - max_steps, a carried hazard record no call returns.  The counts that travel as
 * float64 (steps run, reached count, violation steps, first violation) must be whole numbers: a fraction is refused. */
typedef struct mobrob_follow_resume {
  int32_t step0;       /* global step of this call's step 0, >= 0                 */
  int32_t leg_steps;   /* step budget per waypoint, 0 = none                      */
  float* state;        /* [n][6] position, velocity: in / out                     */
  int32_t* leg_used;   /* [n] steps spent on the waypoint in force: in / out      */
  int32_t* status;     /* [n] out: 0 going, 1 finished, 2 stalled, 3 no waypoints */
} mobrob_follow_resume_t;
int mobrob_ppo_follow_waypoints_resume(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                       const mobrob_hazards_t* hz /* or NULL */, const mobrob_follow_resume_t* resume,
                                       const float* waypoints /* [n][K][pos_dim] */, const int32_t* n_waypoints /* or NULL */,
                                       int32_t* arrival /* [n][K] in / out */, double* robot_out /* [n][4] in / out */,
                                       double* hazard_out /* [n][4] in / out, NULL iff hz is */, float* path_out /* or NULL */,
                                       float* trace_out /* or NULL */);

/* ---- moving hazards: time-indexed hazard frames on evaluation and waypoint following --------------------------------------------
 * The hazards of mobrob_hazards_t with a time axis: every scene is n_frames FRAMES of max_hazards rows, hazards
 * [S][n_frames][M][3].  The check after a robot's step with 0-based GLOBAL step number g (rule, sums, trace columns, hazard_out,
 * episode_cost_out exactly as for the *_hazards calls) reads the frame
 *     f(g) = min(g / frame_steps, n_frames - 1)   (loop = 0: hold the last frame)     f(g) = (g / frame_steps) % n_frames  (loop = 1)
 * with g = step0 + t in a waypoint-following run (t: the call's step; step0 = 0 without `resume`) and g = t in an evaluation (the
 * clock is the call's: an episode reset does not reset it).  Frames are piecewise constant, nothing is interpolated; n_hazards is
 * per scene, the same in every frame.  n_frames = 1 gives the bits of the *_hazards call on the same scene in every output.
 * mobrob_ppo_follow_waypoints_hazard_frames is mobrob_ppo_follow_waypoints_hazards when resume is NULL (start given, arrival /
 * robot_out / hazard_out out only) and one call of a run with hazards as mobrob_ppo_follow_waypoints_resume when it is not (start
 * ignored): the invariants of a run hold with frames, since f depends on the global step alone.
 *   kernels   k_goal64_tile<DP, FrameHazardTask<...>>: one frame of a shared scene resident in LDS, replaced by all 64 lanes when
 *             f changes; per-robot scenes and the per-step path (k_goal_task_step<FrameHazardTask<...>>) read the frame from
 *             global memory.
 * MOBROB_ERR_INVALID before any launch or copy, besides every check of the counterpart (those of mobrob_hazards_t on every
 * frame included), for: n_frames < 1, frame_steps < 1, a table of n_scenes * n_frames * max_hazards * 12 bytes above
 * MOBROB_HAZARD_FRAMES_MAX_BYTES. */
#define MOBROB_HAZARD_FRAMES_MAX_BYTES (64u << 20)
typedef struct mobrob_hazard_frames {
  int32_t n_scenes;          /* S >= 1                                                        */
  int32_t max_hazards;       /* M, row stride, 0 .. 1024                                      */
  const float* hazards;      /* [S][n_frames][M][3]: x, y, radius (radius >= 0, finite)       */
  const int32_t* n_hazards;  /* [S] counts 0 .. M (every frame of the scene), or NULL = M     */
  const int32_t* scene;      /* [n_robots] scene of each robot, or NULL (needs S == 1)        */
  float cost;                /* hazards_cost, >= 0                                            */
  int32_t indicator;         /* constrain_indicator                                           */
  int32_t n_frames;          /* F >= 1                                                        */
  int32_t frame_steps;       /* steps per frame, >= 1                                         */
  int32_t loop;              /* after the last frame: 0 hold it, 1 start over                 */
} mobrob_hazard_frames_t;
int mobrob_ppo_evaluate_goal_env_hazard_frames(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_eval_spec_t* spec,
                                               const mobrob_hazard_frames_t* hz, const int32_t* quota /* [n_robots] or NULL */,
                                               double* robot_out /* [n_robots][4] */, double* episode_out /* or NULL */,
                                               double* hazard_out /* [n_robots][4] */, double* episode_cost_out /* or NULL */,
                                               float* trace_out /* or NULL */);
int mobrob_ppo_follow_waypoints_hazard_frames(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                              const mobrob_hazard_frames_t* hz, const mobrob_follow_resume_t* resume /* or NULL */,
                                              const float* start /* [n][pos_dim]; unused with resume */,
                                              const float* waypoints /* [n][K][pos_dim] */, const int32_t* n_waypoints /* or NULL */,
                                              int32_t* arrival /* [n][K] (in / out with resume) */,
                                              double* robot_out /* [n][4] (in / out with resume) */,
                                              double* hazard_out /* [n][4] (in / out with resume) */, float* path_out /* or NULL */,
                                              float* trace_out /* or NULL */);

/* ---- robot teams: pairwise separation costs in waypoint-following runs -------------------------------------------------------
 * One call of a run (mobrob_ppo_follow_waypoints_resume; with hz its hazards, with hzf mobrob_ppo_follow_waypoints_hazard_frames'
 * moving hazards; not both) whose robots are partitioned into TEAMS of team_size consecutive robots: team of robot n = n /
 * team_size, team-local index m = n % team_size.  team_size is 1, 2, 4, 8 or 16 and divides n_robots, so a team never straddles a
 * 16-robot tile; robots of different teams never see each other.  The rule (mobrob_amd/envs/goal_rules.py: team_cost): after the
 * step with 0-based global number g, for every robot i that stepped in it, with p the post-step positions -- x and y only, as for
 * hazards, for drones too -- and the team-mates j != i, a mate that did not step (finished, stalled, without waypoints, parked in
 * an earlier call) counting where it stands:
 *     d_ij = |p_i - p_j|  (float32, correctly rounded)      cost_i = cost * sum over d_ij <= separation of (separation - d_ij)
 *     indicator: cost_i = (cost_i > 0)      clear_i = min_j (d_ij - separation)  (+inf alone)      partner_i = the j attaining it
 * (equal clearances: the lowest j).  d_ij == separation contributes exactly 0 and is no conflict.  The float32 sum runs over four
 * partial sums -- quarter q: the members m = q, q + 4, ... except i -- combined as (p0 + p1) + (p2 + p3), cost applied once
 * afterwards; the minimum over the same quarters and exchanges.  A robot accounts only for steps in which it stepped itself.
 *   team_out  [n][5] float64, in / out, carried like hazard_out: sum of the step costs, steps with cost > 0, the first such step
 *             (global, 1-based, -1 = none), the minimum of clear_i over the run (NaN: no step run yet in the run; +inf with
 *             team_size 1), the partner's global index at that minimum (the first attainment is kept; -1 = none).  A run starts
 *             from 0, 0, -1, NaN, -1.
 * Nothing else changes: dynamics, rewards, arrivals, status, hazard_out, path and trace (rows of the underlying call, same width)
 * are the bits of the call without teams, and a run split into calls ends with the team_out of one long call.
 *   kernels   k_goal64_tile<DP, TeamTask<...>>: every robot's carried position seeds the tile's [16][2] xy block before the step
 *             loop, the check runs on all 64 lanes as (robot, quarter) after the env phase.  Per-step path: k_team_step after every
 *             k_goal_task_step, one thread per robot, the same order of operations, hence the same bits.
 * MOBROB_ERR_INVALID before any launch or copy, besides every check of the underlying run call, for: team_size outside {1, 2, 4,
 * 8, 16}, n_robots % team_size != 0, separation or cost negative or non-finite, a NULL resume, teams or team_out, both hz and hzf,
 * a carried team record no call returns (a sum that is negative or not finite, counts that are not whole, negative or above the
 * steps run, a first step that is not whole, < -1 or > step0, a partner that is neither -1 nor another member of the robot's team,
 * a clearance that is not NaN with zero steps run or NaN with steps run). */
typedef struct mobrob_teams {
  int32_t team_size;   /* 1, 2, 4, 8 or 16; divides n_robots */
  float separation;    /* >= 0, finite                       */
  float cost;          /* >= 0, finite                       */
  int32_t indicator;   /* cost_i = (cost_i > 0)              */
} mobrob_teams_t;
int mobrob_ppo_follow_waypoints_teams(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                      const mobrob_hazards_t* hz /* or NULL */, const mobrob_hazard_frames_t* hzf /* or NULL; not both */,
                                      const mobrob_follow_resume_t* resume, const mobrob_teams_t* teams,
                                      const float* waypoints /* [n][K][pos_dim] */, const int32_t* n_waypoints /* or NULL */,
                                      int32_t* arrival /* [n][K] in / out */, double* robot_out /* [n][4] in / out */,
                                      double* hazard_out /* [n][4] in / out, NULL iff no hazards */,
                                      double* team_out /* [n][5] in / out */, float* path_out /* or NULL */,
                                      float* trace_out /* or NULL */);

/* ---- timed waypoints: release steps and holds in waypoint-following runs ---------------------------------------------------------
 * One call of a run (mobrob_ppo_follow_waypoints_teams, with `teams` optional: NULL = no teams, and team_out is then NULL) whose
 * waypoints carry RELEASE STEPS.  The rule (mobrob_amd/envs/goal_rules.py: Schedule): waypoint k of robot n may not be the goal in
 * force in a step whose 0-based global number g is below release[n][k]; until then the robot HOLDS at its anchor -- the previous
 * waypoint, home[n] for k = 0 -- under the policy.  k keeps its meaning (waypoints reached = index of the waypoint the robot is
 * on) and the goal used in global step g is a pure function of (k, g), so nothing new is carried for it:
 *     hold(k, g) = k < n_waypoints[n] and g < release[n][k]        goal(k, g) = hold ? anchor(k) : waypoint k (the last one for
 *     k >= n_waypoints[n], as without a schedule)
 * set for g = step0 at entry and for g + 1 at the end of step g, after any arrival.  A hold step (hold at the step's entry) runs the
 * env step against the anchor and counts in `steps run`; path, trace, hazard and team checks run as on any step.  It ignores the
 * reach test (no arrival), adds nothing to the reward sum, leaves leg_used as it is, and its trace flags are 0, 0, k, idle.
 *   sched_out [n][2] float64, in / out, carried like hazard_out: hold steps run; the largest distance to the anchor after a hold
 *             step (float32, widened; NaN while no hold step was run).  A run starts from 0, NaN.
 * robot_out[n][3] is the distance to the waypoint the robot is on, released or not.  With every release 0 every output is the
 * bits of the call without a schedule and sched_out stays 0, NaN; a run split into calls ends with the arrays of one long call.
 *   kernels   the task kernels of the run calls with ScheduledFollowTask in ResumeFollowTask's place (csrc/kernels_follow.h).
 * MOBROB_ERR_INVALID before any launch or copy, the in / out arrays left as given, besides every check of the underlying call, for:
 * a NULL schedule, release, home or sched_out, team_out without teams or teams without team_out, a negative release among
 * k < n_waypoints[n], a non-finite home, a carried sched_out[n][0] that is not a whole number in 0 .. steps run, sched_out[n][1]
 * negative or infinite, NaN with [0] > 0, or not NaN with [0] == 0. */
typedef struct mobrob_follow_schedule {
  const int32_t* release;   /* [n][K] first global step in which waypoint k may be the goal in force, >= 0 */
  const float* home;        /* [n][pos_dim] anchor of waypoint 0, finite                                  */
} mobrob_follow_schedule_t;
int mobrob_ppo_follow_waypoints_scheduled(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                          const mobrob_hazards_t* hz /* or NULL */, const mobrob_hazard_frames_t* hzf /* or NULL; not both */,
                                          const mobrob_follow_resume_t* resume, const mobrob_teams_t* teams /* or NULL */,
                                          const mobrob_follow_schedule_t* schedule,
                                          const float* waypoints /* [n][K][pos_dim] */, const int32_t* n_waypoints /* or NULL */,
                                          int32_t* arrival /* [n][K] in / out */, double* robot_out /* [n][4] in / out */,
                                          double* hazard_out /* [n][4] in / out, NULL iff no hazards */,
                                          double* team_out /* [n][5] in / out, NULL iff no teams */,
                                          double* sched_out /* [n][2] in / out */, float* path_out /* or NULL */,
                                          float* trace_out /* or NULL */);

/* ---- walls: box contact and crossing checks in waypoint-following runs -----------------------------------------------------------
 * One call of a run (mobrob_ppo_follow_waypoints_scheduled, with `teams` and `schedule` optional: NULL = none, and team_out /
 * sched_out are then NULL) whose robots are checked against WALLS: axis-aligned boxes (cx, cy, hx, hy), hx, hy >= 0 half extents,
 * up to 1024 per scene, shared or per robot by a scene index exactly as mobrob_hazards_t.  The check is observational (solid walls: mobrob_ppo_follow_waypoints_solid below): dynamics,
 * rewards, arrivals, status, hazard_out, team_out, sched_out, path and trace are the bits of the call without walls.  The rule
 * (mobrob_amd/envs/goal_rules.py: wall_check): after the step with 0-based global number g a robot that stepped has pre-step xy a
 * and post-step xy p (x and y only, for drones too; a is where the previous step ended, or the carried position).  In float32,
 * every operation rounded on its own:
 *     qx = |px - cx| - hx    qy = |py - cy| - hy    sdf = sqrt(max(qx, 0)^2 + max(qy, 0)^2) + min(max(qx, qy), 0)
 *     contact: sdf <= radius adds (radius - sdf) to the step's sum; clear_w = sdf - radius; sdf == radius adds exactly 0
 *     mx = 0.5 (ax + px) - cx, my likewise, ex = 0.5 (px - ax), ey = 0.5 (py - ay)
 *     hit_w = not(|mx| > hx + |ex| or |my| > hy + |ey| or |mx ey - my ex| > hx |ey| + hy |ex|)   (segment against the closed box)
 * The sum runs over four partial sums -- quarter q: walls q, q + 4, ... -- combined as (p0 + p1) + (p2 + p3), `cost` applied once
 * afterwards (indicator: cost > 0); the (clearance, wall) minimum over the same quarters and exchanges, the smaller clearance
 * winning, then the smaller index; the crossing flag is the OR over all walls.
 *   wall_out  [n][7] float64, in / out, carried like hazard_out: cost sum, contact steps (cost > 0), first contact step (global,
 *             1-based, -1 = none), minimum clearance (NaN: no step run yet in the run; +inf without walls), the wall's index at
 *             that minimum (first attainment; -1 = none), crossing steps, first crossing step.  A run starts from 0, 0, -1, NaN,
 *             -1, 0, -1; a run split into calls ends with the wall_out of one long call.
 *   kernels   k_goal64_tile<DP, WallTask<...>>: the robot lane keeps its pre-step xy in a second [16][2] LDS block, the check runs
 *             on all 64 lanes as (robot, quarter), a shared scene is staged in LDS (16 bytes a wall).  Per-step path: the same
 *             operations in one thread inside k_goal_task_step<WallTask<...>>.  Evaluation takes no walls: resets teleport.
 * MOBROB_ERR_INVALID before any launch or copy, the in / out arrays left as given, besides every check of the underlying call,
 * for: a NULL resume, walls or wall_out, team_out / sched_out / hazard_out without their argument or the reverse, n_scenes < 1,
 * max_walls outside 0 .. 1024, a NULL box table with max_walls > 0, several scenes without a scene index, a scene index or a count
 * out of range, a box in use that is not finite or has a negative half extent, radius or cost negative or non-finite, a carried
 * wall record no call returns, a scene whose tile would need more LDS than the device allows a workgroup. */
typedef struct mobrob_walls {
  int32_t n_scenes;          /* S >= 1                                                  */
  int32_t max_walls;         /* M, row stride, 0 .. 1024                                */
  const float* boxes;        /* [S][M][4]: cx, cy, hx, hy (hx, hy >= 0, finite)         */
  const int32_t* n_walls;    /* [S] counts 0 .. M, or NULL = M                          */
  const int32_t* scene;      /* [n_robots] scene of each robot, or NULL (needs S == 1)  */
  float radius;              /* the robot's footprint, >= 0                             */
  float cost;                /* cost per unit of intrusion, >= 0                        */
  int32_t indicator;         /* a step's cost is (cost > 0)                             */
} mobrob_walls_t;
int mobrob_ppo_follow_waypoints_walls(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                      const mobrob_hazards_t* hz /* or NULL */, const mobrob_hazard_frames_t* hzf /* or NULL; not both */,
                                      const mobrob_follow_resume_t* resume, const mobrob_teams_t* teams /* or NULL */,
                                      const mobrob_follow_schedule_t* schedule /* or NULL */, const mobrob_walls_t* walls,
                                      const float* waypoints /* [n][K][pos_dim] */, const int32_t* n_waypoints /* or NULL */,
                                      int32_t* arrival /* [n][K] in / out */, double* robot_out /* [n][4] in / out */,
                                      double* hazard_out /* [n][4] in / out, NULL iff no hazards */,
                                      double* team_out /* [n][5] in / out, NULL iff no teams */,
                                      double* sched_out /* [n][2] in / out, NULL iff no schedule */,
                                      double* wall_out /* [n][7] in / out */, float* path_out /* or NULL */,
                                      float* trace_out /* or NULL */);

/* ---- solid walls: robots stop and slide at the boxes ---------------------------------------------------------------------------
 * mobrob_ppo_follow_waypoints_walls with the walls SOLID: the same arguments plus blocked_out.  Inside every environment step,
 * between the dynamics and the goal test, the proposed position is resolved against the robot's scene (mobrob_amd/envs/
 * goal_rules.py: wall_block).  With a the pre-step xy and p the xy the velocity update and the clamp to +-extent propose, in
 * float32, every operation rounded on its own, Hx = hx + radius, Hy = hy + radius per wall:
 *     a wall with |ax - cx| <= Hx and |ay - cy| <= Hy does not hold in this step (a robot that starts inside an inflated box can
 *     leave it; such a step counts as `inside`);
 *     seg_hit(a, c) = OR over the other walls of the crossing test above on the segment a c, with Hx, Hy for hx, hy;
 *     candidates c0 = (px, py), c1 = (px, ay), c2 = (ax, py), c3 = (ax, ay): the first without a hit is taken (c3 untested), its
 *     number is the step's code; the velocity component of every dropped axis becomes +0.0 (the robot pushes and slides).
 * The reach test, reward, arrival, next waypoint, path, trace and the next observation use the resolved position; wall_out is then
 * accounted on (a, resolved) as in the call above.  z is untouched.  Exact: a robot that never had a step `inside` has 0 crossing
 * steps.  Up to rounding: its minimum clearance is > -1e-6 (contacts are not promised to be exactly 0).  Not promised: the robot is
 * not placed on the wall's surface (a gap of up to one step remains); no friction, no rotation; robots do not block each other;
 * evaluation takes no walls.
 *   blocked_out [n][4] int32, in / out, carried like wall_out: blocked steps (code != 0), first blocked step (global, 1-based, -1 =
 *             none), fully stopped steps (code 3), steps in which a wall did not hold.  A run starts from 0, -1, 0, 0.
 *   kernels   k_goal64_tile / k_goal_task_step<WallTask<[HazardTask<]SolidFollowTask<ResumeFollowTask | ScheduledFollowTask>[>]>>,
 *             with or without TeamTask around them: the resolution runs on the robot's own lane / thread inside the env step,
 *             serially over the scene (one pass when c0 is clean, at most three), on the scene WallTask staged in LDS when shared.
 * MOBROB_ERR_INVALID, besides every check of mobrob_ppo_follow_waypoints_walls, for: a NULL blocked_out, hazard frames (static
 * hazards, teams and schedules compose; moving hazards do not yet), a carried blocked record no call returns. */
int mobrob_ppo_follow_waypoints_solid(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                      const mobrob_hazards_t* hz /* or NULL */, const mobrob_hazard_frames_t* hzf /* must be NULL */,
                                      const mobrob_follow_resume_t* resume, const mobrob_teams_t* teams /* or NULL */,
                                      const mobrob_follow_schedule_t* schedule /* or NULL */, const mobrob_walls_t* walls,
                                      const float* waypoints /* [n][K][pos_dim] */, const int32_t* n_waypoints /* or NULL */,
                                      int32_t* arrival /* [n][K] in / out */, double* robot_out /* [n][4] in / out */,
                                      double* hazard_out /* [n][4] in / out, NULL iff no hazards */,
                                      double* team_out /* [n][5] in / out, NULL iff no teams */,
                                      double* sched_out /* [n][2] in / out, NULL iff no schedule */,
                                      double* wall_out /* [n][7] in / out */, int32_t* blocked_out /* [n][4] in / out */,
                                      float* path_out /* or NULL */, float* trace_out /* or NULL */);

/* ---- solid teams: team-mates block each other --------------------------------------------------------------------------------
 * mobrob_ppo_follow_waypoints_teams with the mates SOLID, alone (walls, wall_out, blocked_out NULL) or together with solid walls
 * (all three given, as mobrob_ppo_follow_waypoints_solid takes them), over plain and scheduled runs.  Inside every environment
 * step, between the dynamics and the goal test, the proposed position is resolved against the robot's team-mates (mobrob_amd/envs/
 * goal_rules.py: team_block, team_block_step).  It is the rule of solid walls over one longer list of inflated boxes:
 *     mate j: the closed square with centre c_j and Hx = Hy = separation exactly;  wall w: Hx = hx + radius, Hy = hy + radius;
 *     a box that holds the pre-step position does not hold in this step (mates that start too close can separate);
 *     candidates c0 .. c3, the segment test and the velocity of a dropped axis (+0.0) as in the call above, against mates and walls
 *     at once -- one resolve over the union, not two in sequence.
 * Where mate j stands (c_j): the order is serial inside a team, by team-local index m = 0 .. team_size - 1, within one global step.
 * Member m resolves against mates with a lower index where they stand AFTER this step's resolve and against mates with a higher
 * index where they stood BEFORE the step; a mate that does not step (finished, held back by its budget, inactive) counts where it
 * stands.  The proposals do not depend on the mates.  The reach test, reward, arrival, next waypoint, path, trace and the next
 * observation use the resolved position; team_out (and wall_out) are then accounted on the resolved positions and stay observational.
 * For a pair of mates that was never inside each other's square in the run -- exact: no step's segment meets the other's closed
 * square; up to rounding: their Chebyshev distance after every step is > separation - 1e-6, so the clearance in team_out[n][3] is
 * > -1e-6.  Not promised: fairness (the lower index goes first), freedom from deadlock (two mates sent to one point: the first to
 * arrive holds the other out; a leg budget and replanning are the remedy), anything across teams, rotation, friction.
 *   team_blocked_out [n][4] int32, in / out, carried like blocked_out: steps blocked by a mate (a rejected candidate met a mate's
 *             square), the first such step (global, 1-based, -1 = none), such steps with no move at all (code 3), steps inside a
 *             mate's square.  A run starts from 0, -1, 0, 0.  With walls, blocked_out counts in the same way the steps in which a
 *             rejected candidate met a wall: a step blocked by walls only is counted there alone, one blocked by both in both.
 *   kernels   k_goal64_tile / k_goal_task_step<TeamTask<[WallTask<]SolidTeamFollowTask<ResumeFollowTask | ScheduledFollowTask,
 *             walls>[>]>> (csrc/kernels_team_solid.h): the resolve is a loop over the team-local index inside the env step, on the
 *             tile's [16][2] block of positions in LDS, on the per-step path on the state rows; a team lies in one wave on both.
 * team_size 1 gives the bits of mobrob_ppo_follow_waypoints_teams / _solid.  MOBROB_ERR_INVALID, besides every check of those two
 * calls, for: a NULL teams, team_out or team_blocked_out, static hazards or hazard frames (hz, hzf and hazard_out must be NULL),
 * walls without blocked_out (observational walls), wall_out or blocked_out without walls, a carried team-blocked record no call
 * returns. */
int mobrob_ppo_follow_waypoints_teams_solid(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                            const mobrob_hazards_t* hz /* must be NULL */, const mobrob_hazard_frames_t* hzf /* must be NULL */,
                                            const mobrob_follow_resume_t* resume, const mobrob_teams_t* teams,
                                            const mobrob_follow_schedule_t* schedule /* or NULL */, const mobrob_walls_t* walls /* or NULL */,
                                            const float* waypoints /* [n][K][pos_dim] */, const int32_t* n_waypoints /* or NULL */,
                                            int32_t* arrival /* [n][K] in / out */, double* robot_out /* [n][4] in / out */,
                                            double* hazard_out /* must be NULL */, double* team_out /* [n][5] in / out */,
                                            double* sched_out /* [n][2] in / out, NULL iff no schedule */,
                                            double* wall_out /* [n][7] in / out, NULL iff no walls */,
                                            int32_t* blocked_out /* [n][4] in / out, NULL iff no walls */,
                                            int32_t* team_blocked_out /* [n][4] in / out */, float* path_out /* or NULL */,
                                            float* trace_out /* or NULL */);

/* ---- grid planner: walls and hazards to waypoints ---------------------------------------------------------------------------
 * Plans waypoints for n_robots robots at once on a grid of cells x cells (32, 64 or 128) over [-extent, extent]^2, x and y only, from
 * the scenes of `walls` and / or `hazards` (neither: an empty grid).  The rule is stated once in mobrob_amd/envs/goal_rules.py
 * (GridSpec, grid_occupancy, grid_field, grid_path) and the device reproduces it bit for bit: a cell is blocked when its centre has
 * the walls' signed distance <= inflate to a wall, or lies within radius + inflate of a hazard (equality blocks); the field of a
 * (scene, goal cell) is the cost-to-go over eight-connected moves (5 orthogonal, 7 diagonal, no corner cutting), -1 where blocked or
 * unreachable; a robot's path descends its field, the previous direction first, else the lowest of E, N, W, S, NE, NW, SW, SE, and
 * its waypoints are the centres of the cells where the direction changes, then the goal itself (z of every waypoint: the goal's).
 * h = 2 extent / cells and inv_h = cells / (2 extent) are computed once by the caller, as floats; host and device use those two.
 * Robots that share a scene and a goal cell share a FIELD: the caller lists the n_fields distinct (scene, goal cell) pairs and gives
 * every robot the index of its own.  With walls and hazards both, the two must agree on n_scenes and on the scene of every robot.
 *   outputs   waypoints_out [n][K][pos_dim] (the first min(count, K), the other slots 0), n_waypoints_out [n] = min(count, K),
 *             count_out [n] waypoints of the full path, cost_out [n] the field at the start cell (-1: unreachable), status_out [n]:
 *             0 planned; 1 unreachable (start or goal cell blocked, or no path; count 0); 2 truncated (count > K); 3 a loop of the
 *             device ran into its bound of cells * cells sweeps or steps (count 0).  Optional copies: occupancy_out [S][G][G] (1
 *             blocked; row iy, column ix), field_out [F][G][G], sweeps_out [F] (relaxation sweeps run, -1: bound hit).
 *   reuse     fields_id_out receives an id > 0 of the occupancy and the fields this call computed; they stay resident until the next
 *             computing call.  A call with spec->reuse_id equal to it (same cells, n_scenes, n_fields) runs the path kernel alone on
 *             them -- a replanning round: new starts, the same goals; walls, hazards, field_goal_cell and field_scene are then unused
 *             but for the scene index per robot.  A stale id is MOBROB_ERR_STATE.
 *   kernels   k_plan_occupancy (a thread per scene and cell, the scene staged in LDS), k_plan_field (a workgroup per field, the field
 *             and a byte of moves per cell in dynamic LDS -- 5 bytes a cell, 80 KB at 128 cells --, in-place relaxation sweeps until
 *             a workgroup-wide "nothing changed"), k_plan_path (a thread per robot).  Runs on the engine's stream, in buffers of its
 *             own outside the arena; nothing a training step reads or writes is touched.
 * MOBROB_ERR_INVALID before any launch or copy for: a NULL argument, n_robots < 1, pos_dim not 2 or 3, cells not 32 / 64 / 128,
 * max_waypoints < 1, n_fields outside 1 .. n_robots, extent, h, inv_h not finite and > 0 or h * inv_h not 1 within 1e-5, inflate
 * negative or non-finite, n_scenes not the scenes' own, a scene that the walls / hazards calls would refuse (radius and costs
 * aside), walls and hazards that disagree on a robot's scene, a non-finite start or goal, field_of outside 0 .. n_fields - 1, a
 * field's scene or goal cell out of range, a robot whose scene or goal cell is not its field's, a field too large for the
 * device's LDS per workgroup. */
typedef struct mobrob_plan_spec {
  int32_t n_robots;       /* n >= 1                                                   */
  int32_t pos_dim;        /* 2 or 3                                                   */
  int32_t cells;          /* G: 32, 64 or 128                                         */
  int32_t max_waypoints;  /* K >= 1                                                   */
  int32_t n_scenes;       /* S: the walls' / hazards' n_scenes, 1 without both        */
  int32_t n_fields;       /* F distinct (scene, goal cell) pairs, 1 .. n              */
  float extent;           /* the grid covers [-extent, extent]^2                      */
  float h, inv_h;         /* float(2 extent / G), float(G / (2 extent))               */
  float inflate;          /* clearance of a blocked cell's centre, >= 0               */
  int64_t reuse_id;       /* 0: compute occupancy and fields; else a fields_id_out    */
} mobrob_plan_spec_t;
int mobrob_ppo_plan_grid(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls /* or NULL */,
                         const mobrob_hazards_t* hazards /* or NULL */, const float* start /* [n][pos_dim] */,
                         const float* goal /* [n][pos_dim] */, const int32_t* field_of /* [n] index into the fields */,
                         const int32_t* field_goal_cell /* [F] iy * G + ix */, const int32_t* field_scene /* [F] */,
                         float* waypoints_out /* [n][K][pos_dim] */, int32_t* n_waypoints_out /* [n] */, int32_t* count_out /* [n] */,
                         int32_t* status_out /* [n] */, int32_t* cost_out /* [n] */, uint8_t* occupancy_out /* [S][G][G] or NULL */,
                         int32_t* field_out /* [F][G][G] or NULL */, int32_t* sweeps_out /* [F] or NULL */,
                         int64_t* fields_id_out /* or NULL */);

/* ---- grid planner: line-of-sight smoothing of the paths, on resident fields ---------------------------------------------------------
 * mobrob_ppo_plan_grid's waypoints are cell centres at every change of direction of an eight-connected walk: a staircase.  This call
 * takes k_plan_path's place on the occupancy and the fields a mobrob_ppo_plan_grid call left resident (spec->reuse_id = its
 * fields_id_out; cells, n_scenes, n_fields as then; 0 or a stale id: MOBROB_ERR_STATE) and keeps of the walk's cells c_0 .. c_L only
 * those a straight leg cannot skip.  The rule, all integers, is stated once in mobrob_amd/envs/goal_rules.py (grid_los, grid_smooth,
 * grid_path_smooth) and reproduced bit for bit:
 *   visible   los(a, b): the supercover of the segment between the centres of cells a and b.  dx = |x1 - x0|, dy = |y1 - y0|, signs sx,
 *             sy, counters ix = iy = 0; false if a is not clear; while ix < dx or iy < dy: t = (1 + 2 ix) dy - (1 + 2 iy) dx; t < 0
 *             steps in x, t > 0 in y, t == 0 (exactly through a cell corner) needs both cells sharing the corner clear and steps in
 *             both; false if the cell stepped into is not clear.  At most dx + dy steps, symmetric in a and b.
 *   clear     margin 0: the cell is not blocked.  margin 1: no in-grid cell of its 3 x 3 neighbourhood is blocked.
 *   smooth    anchor i = 0, j = 1; while j < L: if los(c_i, c_{j+1}) then j += 1, else emit j, i = j, j += 1.  Adjacent cells are never
 *             tested.  Waypoints: the centres of the emitted cells, then the goal itself (z: the goal's).
 *   clearance margin 0: every point of a leg between cell centres lies in a free cell, so it keeps inflate - h / sqrt 2 from walls and
 *             hazards as the unsmoothed path does; the first leg starts at the true start, up to h / sqrt 2 off its cell's centre, and
 *             is covered only to inflate - sqrt 2 h.  margin 1: every point within one cell of a leg of two or more moves lies in a free
 *             cell, which restores inflate - h / sqrt 2 for the first leg.  At margin 0 count is never larger than
 *             mobrob_ppo_plan_grid's; at margin 1 a walk along blocked cells has no clear cell to see from and keeps every cell.
 *   inputs    start, goal, field_of as a reuse call of mobrob_ppo_plan_grid takes them, scene [n] the scene of every robot (NULL: scene
 *             0, one scene only).  spec->inflate is not used.
 *   outputs   waypoints_out, n_waypoints_out, count_out, status_out, cost_out as mobrob_ppo_plan_grid's (status 3: a loop ran into its
 *             bound of cells * cells; count 0, waypoints zeroed, moves 0) and moves_out [n] = L, the moves of the walk (0: none made).
 *   kernels   k_plan_smooth: one wave per robot; the walk (k_plan_path's own step) fills a ring of 128 packed cells in LDS, the 64 lanes
 *             test 64 candidates against the anchor at once, a ballot and a count of trailing zeros find the first that is hidden.
 *             k_plan_dilate: the cells that are not clear at margin 1, once per set of resident fields, kept beside them.  Runs on the
 *             engine's stream in the planner's own buffers; nothing a training step reads or writes is touched.
 * Walls as solid bodies of the run: mobrob_ppo_follow_waypoints_solid (the planner itself is unchanged by it).  Smoothing of a time plan: mobrob_ppo_plan_grid_time_smooth.
 * Team-mates as obstacles: mobrob_ppo_plan_grid_team; smoothed: mobrob_ppo_plan_grid_team_smooth.
 * MOBROB_ERR_INVALID before any launch or copy for: a NULL argument (scene aside), margin not 0 or 1, n_robots < 1, pos_dim not 2 or 3,
 * cells not 32 / 64 / 128, max_waypoints < 1, n_fields outside 1 .. n_robots, n_scenes < 1, extent, h, inv_h not finite and > 0 or
 * h * inv_h not 1 within 1e-5, cells / n_scenes / n_fields not the resident fields', a missing scene index with several scenes, a
 * non-finite start or goal, scene or field_of out of range, a robot whose scene or goal cell is not its field's. */
int mobrob_ppo_plan_smooth(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, int32_t margin /* 0 or 1 */,
                           const float* start /* [n][pos_dim] */, const float* goal /* [n][pos_dim] */,
                           const int32_t* field_of /* [n] */, const int32_t* scene /* [n] or NULL */,
                           float* waypoints_out /* [n][K][pos_dim] */, int32_t* n_waypoints_out /* [n] */, int32_t* count_out /* [n] */,
                           int32_t* status_out /* [n] */, int32_t* cost_out /* [n] */, int32_t* moves_out /* [n] */);

/* ---- grid planner: clearance-aware static plans, a per-cell surcharge near blocked cells ----------------------------------------------
 * mobrob_ppo_plan_grid minimises chamfer length, so its paths hug every obstacle they round.  This call plans on the same grid and the
 * same blocked cells with a SURCHARGE on entering a cell near a blocked one, so a path takes the middle of a corridor where that costs
 * little.  The rule, all integers, is stated once in mobrob_amd/envs/goal_rules.py (grid_clearance, grid_surcharge, grid_field_cost,
 * grid_walk_cost, grid_walk_clearance) and reproduced bit for bit:
 *   clearance the Chebyshev distance in cells of a cell to the nearest blocked cell of the grid, capped at reach + 1; blocked cells 0;
 *             cells outside the grid count as free.
 *   surcharge pen[c] = weight * max(0, reach + 1 - clearance[c]) on free cells, 0 on blocked ones; at most 16 * 8 = 128, a byte.
 *   field     the fixed point of d[c] = min_k(w(k) + pen[c'] + d[c']) over mobrob_ppo_plan_grid's moves from c into c', d[goal] = 0: the
 *             goal cell's own surcharge is paid on entry like any cell's, the start cell's never.  -1 blocked or unreachable.
 *   path      mobrob_ppo_plan_grid's walk with the step to a neighbour with w + pen[c'] + d[c'] == d[c], the same tie order; waypoints,
 *             count and status as there.  cost_out: d at the start cell, the moves plus the surcharges paid.
 *   outputs   mobrob_ppo_plan_grid's, and clearance_min_out [n]: the least clearance over the cells the walk enters (reach + 1 for a
 *             start in the goal's cell, -1 without a walk); on request surcharge_out [S][G][G].
 *   reuse     as mobrob_ppo_plan_grid's, in resident buffers of this family's own (occupancy, surcharges, cost fields): a plain plan and
 *             a clearance plan stay resident side by side.  fields_id_out is an id of this family; spec->reuse_id naming fields of the
 *             other family (either way round), or stale ones, is MOBROB_ERR_STATE.  A reuse call gives the resident reach and weight.
 *   kernels   k_plan_occupancy as it is; k_plan_surcharge (a workgroup per scene: `reach` rounds of 3 x 3 dilation between two byte maps
 *             in LDS, a barrier a round, every cell records the round that reached it); k_plan_field_cost (k_plan_field's shape with a
 *             byte of surcharge per cell beside the field and the moves: 6 bytes a cell, 96 KB at 128 cells); k_plan_path_cost.
 * NOT promised: the plan is no longer the shortest; a doorway narrower than 2 reach cells is still used, its surcharge is paid.
 * MOBROB_ERR_INVALID before any launch or copy for reach outside 1 .. 8, weight outside 1 .. 16, a reuse call whose reach or weight is
 * not the resident fields', and everything mobrob_ppo_plan_grid refuses. */
int mobrob_ppo_plan_grid_clear(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls /* or NULL */,
                               const mobrob_hazards_t* hazards /* or NULL */, int32_t reach /* 1 .. 8 */, int32_t weight /* 1 .. 16 */,
                               const float* start /* [n][pos_dim] */, const float* goal /* [n][pos_dim] */,
                               const int32_t* field_of /* [n] */, const int32_t* field_goal_cell /* [F] */,
                               const int32_t* field_scene /* [F] */, float* waypoints_out /* [n][K][pos_dim] */,
                               int32_t* n_waypoints_out /* [n] */, int32_t* count_out /* [n] */, int32_t* status_out /* [n] */,
                               int32_t* cost_out /* [n] */, int32_t* clearance_min_out /* [n] */,
                               uint8_t* occupancy_out /* [S][G][G] or NULL */, int32_t* field_out /* [F][G][G] or NULL */,
                               int32_t* sweeps_out /* [F] or NULL */, uint8_t* surcharge_out /* [S][G][G] or NULL */,
                               int64_t* fields_id_out /* or NULL */);

/* mobrob_ppo_plan_smooth on the fields a mobrob_ppo_plan_grid_clear call left resident (spec->reuse_id = its fields_id_out; any other
 * id: MOBROB_ERR_STATE): the walk is the clearance-aware one, the line-of-sight rule is mobrob_ppo_plan_smooth's own and never reads
 * costs.  k_plan_smooth_cost: k_plan_smooth's wave per robot, ring, ballot window and bounds with the surcharge-aware step.  Outputs
 * and refusals as mobrob_ppo_plan_smooth's, and clearance_min_out [n] as mobrob_ppo_plan_grid_clear's. */
int mobrob_ppo_plan_smooth_clear(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, int32_t margin /* 0 or 1 */,
                                 const float* start /* [n][pos_dim] */, const float* goal /* [n][pos_dim] */,
                                 const int32_t* field_of /* [n] */, const int32_t* scene /* [n] or NULL */,
                                 float* waypoints_out /* [n][K][pos_dim] */, int32_t* n_waypoints_out /* [n] */,
                                 int32_t* count_out /* [n] */, int32_t* status_out /* [n] */, int32_t* cost_out /* [n] */,
                                 int32_t* moves_out /* [n] */, int32_t* clearance_min_out /* [n] */);

/* ---- grid planner over time: moving hazards as layers of occupancy, waits as release steps -----------------------------------------
 * mobrob_ppo_plan_grid for hazards that move (mobrob_hazard_frames_t).  The rule is stated once in mobrob_amd/envs/goal_rules.py
 * (grid_layer_frames, grid_occupancy_time, grid_time_field, grid_walk_time, grid_path_time) and reproduced bit for bit.  A robot is
 * given layer_steps steps for one ACTION, a move or a wait.
 *   layers    layer t < T = `layers` covers the global steps step0 + t layer_steps .. step0 + (t + 1) layer_steps - 1, the tail layer T
 *             every step from step0 + T layer_steps on.  A layer's frames are the distinct f(g) of its steps, a cyclically contiguous
 *             run; the tail's are all frames with loop, else f(step0 + T layer_steps) .. n_frames - 1.  They are computed here.
 *   blocked   layer t's map blocks a cell that mobrob_ppo_plan_grid's test blocks for the walls or for the rows of ANY frame of the layer.
 *   field     d[T + 1][G][G] per field: d_T is mobrob_ppo_plan_grid's field on the tail's map.  For t < T: d_t[c] = -1 if layer t blocks
 *             c; 0 in the goal cell; else the minimum of d_{t+1}[nb] + w over the moves layer t allows with d_{t+1}[nb] >= 0 (w = 5, 7)
 *             and of the wait d_{t+1}[c] + 4 where d_{t+1}[c] >= 0; -1 if nothing qualifies.
 *   walk      from the start's cell at t = 0; unreachable (count 0, cost -1) iff d_0[start cell] < 0.  While not in the goal's cell and
 *             t < T: the previous move if it qualifies (allowed by layer t, d_{t+1}[nb] >= 0, d_{t+1}[nb] + w == d_t[c]), else the lowest
 *             such move of E, N, W, S, NE, NW, SW, SE, else the wait (d_{t+1}[c] + 4 == d_t[c]); every action advances t.  From t = T on
 *             the walk is mobrob_ppo_plan_grid's on (d_T, the tail's map).  A cell entered by a move is a waypoint when the move leaving
 *             it differs from the move entering it or when the walk waited there; the last waypoint is the goal itself.
 *   outputs   waypoints_out .. cost_out as mobrob_ppo_plan_grid's (cost: d_0 at the start cell; status 3: the tail's relaxation or a walk
 *             of more than T + cells * cells actions ran into its bound).  waits_out [n][K]: the waits made at waypoint k's anchor (the
 *             previous waypoint's cell; the start cell for k = 0); leave_out [n][K]: the actions made before the move that leaves that
 *             anchor -- a hold there until step0 + leave * layer_steps is mobrob_follow_schedule_t's release step of waypoint k;
 *             arrive_out [n]: the actions of the whole walk.  Slots from min(count, K) on are 0.  Optional copies: occ_time_out
 *             [S][T + 1][G][G], fields_time_out [F][T + 1][G][G], sweeps_out [F] (the tail's relaxation sweeps, -1: bound hit).
 *   kernels   k_plan_occupancy_time (a thread per scene, layer and cell; the walls staged in LDS once, then each frame of the layer),
 *             k_plan_field_time (a workgroup per field: the tail relaxed in place in LDS, then T Jacobi steps between two LDS layers,
 *             one barrier each; 9 bytes a cell, 144 KB at 128 cells), k_plan_path_time (a thread per robot).  Every call computes and
 *             keeps nothing resident: the buffers are this call's own, so fields left resident by mobrob_ppo_plan_grid stay valid.
 *             Runs on the engine's stream; nothing a training step reads or writes is touched.
 * MOBROB_ERR_INVALID before any launch or copy for everything mobrob_ppo_plan_grid refuses (spec->reuse_id must be 0) and everything the
 * *_hazard_frames calls refuse of the frames, and for: layers outside 1 .. MOBROB_PLAN_LAYERS_MAX, layer_steps < 1, step0 < 0, step0 +
 * (layers + 1) * layer_steps above INT32_MAX, time fields of n_fields * (layers + 1) * cells * cells * 4 bytes above
 * MOBROB_PLAN_TIME_MAX_BYTES, a field too large for the device's LDS per workgroup. */
#define MOBROB_PLAN_LAYERS_MAX 256
#define MOBROB_PLAN_TIME_MAX_BYTES (256u << 20)
typedef struct mobrob_plan_time {
  int32_t step0;        /* g0 >= 0: the global step at which the plan starts */
  int32_t layer_steps;  /* steps a robot is given for one action, >= 1      */
  int32_t layers;       /* T: 1 .. MOBROB_PLAN_LAYERS_MAX                    */
} mobrob_plan_time_t;
int mobrob_ppo_plan_grid_time(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls /* or NULL */,
                              const mobrob_hazard_frames_t* hazards, const mobrob_plan_time_t* time,
                              const float* start /* [n][pos_dim] */, const float* goal /* [n][pos_dim] */,
                              const int32_t* field_of /* [n] */, const int32_t* field_goal_cell /* [F] */,
                              const int32_t* field_scene /* [F] */, float* waypoints_out /* [n][K][pos_dim] */,
                              int32_t* n_waypoints_out /* [n] */, int32_t* count_out /* [n] */, int32_t* status_out /* [n] */,
                              int32_t* cost_out /* [n] */, int32_t* waits_out /* [n][K] */, int32_t* leave_out /* [n][K] */,
                              int32_t* arrive_out /* [n] */, uint8_t* occ_time_out /* [S][T + 1][G][G] or NULL */,
                              int32_t* fields_time_out /* [F][T + 1][G][G] or NULL */, int32_t* sweeps_out /* [F] or NULL */);

/* ---- line-of-sight smoothing of a time plan: a straight leg is tested against every layer it spans ------------------------------
 * mobrob_ppo_plan_grid_time with mobrob_ppo_plan_smooth's waypoints.  The rule, all integers, is stated once in
 * mobrob_amd/envs/goal_rules.py (grid_next_blocked, grid_los_time, grid_smooth_time, grid_path_smooth_time) and reproduced bit for bit.
 *   clear     as mobrob_ppo_plan_smooth's, per layer: blk_t is layer t's map at margin 0, its 3 x 3 dilation at margin 1.
 *   table     nb[T + 1][G][G] int16 per scene: nb[T][c] = T if blk_T[c] else 32767; for t = T - 1 .. 0, nb[t][c] = t if blk_t[c] else
 *             nb[t + 1][c].  Cell c is clear in all of the layers lo .. hi (lo <= hi <= T) exactly when nb[lo][c] > hi.
 *   visible   los_time(a, b, lo, hi): mobrob_ppo_plan_smooth's los on the map nb[lo] <= hi.
 *   smooth    the walk's cells c[0 .. A], one per action boundary (a wait repeats its cell).  Anchor i = 0, j = 1; while j < A: if
 *             los_time(c[i], c[j + 1], min(i, T), min(j + 1, T)) then j += 1, else emit j, i = j, j += 1.  A leg of one action is never
 *             tested.  Waypoints: the centres of the emitted cells, then the goal itself (z: the goal's).
 *   guarantee a kept leg from action index a to b with b - a >= 2: every cell of the supercover between c[a] and c[b], both ends
 *             included, is clear at the margin in each of the layers min(a, T) .. min(b, T) -- whatever the robot's speed along the
 *             leg, as long as it leaves c[a] no earlier and reaches c[b] no later than the walk does.  A leg of one action carries
 *             mobrob_ppo_plan_grid_time's promise only.  Not promised: fewer waypoints than the unsmoothed plan.
 *   outputs   waypoints_out .. cost_out, arrive_out and the optional copies as mobrob_ppo_plan_grid_time's.  leave_out [n][K]: the
 *             action index of waypoint k's anchor, 0 for k = 0, the emitted index of waypoint k - 1 otherwise -- a hold at EVERY anchor
 *             but the start until step0 + leave * layer_steps is the release step of waypoint k (a straight leg is shorter than the
 *             walk it replaces; the robot must not enter the next leg before the first layer that leg was tested in).  waits_out
 *             [n][K] or NULL: zeroed.  moves_out [n]: the actions of the walk that are moves.  next_blocked_out [S][T + 1][G][G] or
 *             NULL: the table.  Status 3: the tail's relaxation, a walk of more than T + cells * cells actions or as many rounds of
 *             the window ran into the bound; count 0, cost -1, arrive 0, moves 0, waypoints and leave zeroed.
 *   kernels   k_plan_occupancy_time and k_plan_field_time as they are; at margin 1 k_plan_dilate as it is over the S * (T + 1) layer
 *             maps; k_plan_next_blocked (a thread per scene and cell scans the layers from the tail down); k_plan_smooth_time in
 *             k_plan_path_time's place: one wave per robot, the walk's cells in a ring of 128 packed cells in LDS indexed by action,
 *             lane l tests c[i] against c[base + l] on nb[min(i, T)] with the threshold min(base + l, T) (base = i + 2 at first,
 *             + 64 after a window without a hidden cell), a ballot and a count of trailing zeros find the first hidden index.  Every call computes in the time plans' own buffer and keeps nothing
 *             resident; runs on the engine's stream; nothing a training step reads or writes is touched.
 * Smoothing of a team plan: mobrob_ppo_plan_grid_team_smooth.  Solid walls: mobrob_ppo_follow_waypoints_solid.
 * MOBROB_ERR_INVALID before any launch or copy for everything mobrob_ppo_plan_grid_time refuses (waits_out aside, moves_out included
 * in "a NULL argument"), and for: margin not 0 or 1, time fields plus the table of n_scenes * (layers + 1) * cells * cells * 2 bytes
 * above MOBROB_PLAN_TIME_MAX_BYTES. */
int mobrob_ppo_plan_grid_time_smooth(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls /* or NULL */,
                                     const mobrob_hazard_frames_t* hazards, const mobrob_plan_time_t* time, int32_t margin /* 0 or 1 */,
                                     const float* start /* [n][pos_dim] */, const float* goal /* [n][pos_dim] */,
                                     const int32_t* field_of /* [n] */, const int32_t* field_goal_cell /* [F] */,
                                     const int32_t* field_scene /* [F] */, float* waypoints_out /* [n][K][pos_dim] */,
                                     int32_t* n_waypoints_out /* [n] */, int32_t* count_out /* [n] */, int32_t* status_out /* [n] */,
                                     int32_t* cost_out /* [n] */, int32_t* waits_out /* [n][K] or NULL */, int32_t* leave_out /* [n][K] */,
                                     int32_t* arrive_out /* [n] */, int32_t* moves_out /* [n] */,
                                     uint8_t* occ_time_out /* [S][T + 1][G][G] or NULL */,
                                     int32_t* fields_time_out /* [F][T + 1][G][G] or NULL */, int32_t* sweeps_out /* [F] or NULL */,
                                     int16_t* next_blocked_out /* [S][T + 1][G][G] or NULL */);

/* ---- prioritised planning inside a team: a mate's planned walk as one more moving obstacle ---------------------------------------
 * mobrob_ppo_plan_grid_time for robots in teams of team_size consecutive robots (mobrob_teams_t's partition).  The rule is stated
 * once in mobrob_amd/envs/goal_rules.py (grid_reserve, grid_team_field, grid_walk_team, grid_plan_team) and reproduced bit for bit.
 *   order     inside a team the member with local index m plans after the members 0 .. m - 1, on the map occ_t = base_t OR res_t;
 *             teams never see each other.  base: the layers of mobrob_ppo_plan_grid_time; hazards NULL: the walls' map in every layer.
 *   reserve   a walk with cells c[0 .. A] (A = arrive, c[a] = c[A] beyond) reserves in layer t < T every cell within Chebyshev distance
 *             `reserve` of c[t] or c[t + 1], in the tail layer T every cell within it of any c[a], a >= min(T, A).  A member whose plan
 *             is unreachable or ran into a loop bound reserves its start cell in every layer.
 *   field     mobrob_ppo_plan_grid_time's, one per robot, with one change: the goal cell is terminal (0) only where it is free in
 *             layer t and in every later layer up to T; otherwise it is an ordinary cell.
 *   walk      mobrob_ppo_plan_grid_time's, with one change: it ends where d_t[c] == 0, not on entering the goal's cell.
 *   outputs   waypoints_out .. arrive_out as mobrob_ppo_plan_grid_time's.  Optional: sweeps_out [n] (the tail's relaxation sweeps per
 *             robot, -1: bound hit), walk_out [n][walk_cap] (the cells c[0 .. min(A, walk_cap - 1)] of every walk, iy * 128 + ix, the
 *             other slots 0; a robot without a walk: its start cell), occ_time_out [S][T + 1][G][G] (the BASE layers),
 *             fields_team_out [n][T + 1][G][G], workgroups_out (the workgroups launched).
 *   kernels   k_plan_occupancy_time for the base layers, as it is; k_plan_team: one workgroup of 1024 threads takes one team at a
 *             time, min(teams, compute units, MOBROB_PLAN_TIME_MAX_BYTES / bytes of one field) workgroups loop over the teams.  Per
 *             member: the layer maps in LDS (the base layer and a Chebyshev test against the earlier members' cells), the tail relaxed
 *             in place, T Jacobi steps, the field in the workgroup's scratch, one thread walks it.  LDS: 9 bytes a cell + 32 (T + 1) + 16.
 *             Runs on the engine's stream in buffers of its own; nothing resident changes, nothing a training step reads is touched.
 * guarantee: two PLANNED (or truncated) mates are more than `reserve` cells apart (Chebyshev, between cell centres, over both cells
 * of each action) and never cross diagonally inside a 2 x 2 block.  Prioritised planning is incomplete: in this call a member never
 * yields; mobrob_ppo_plan_grid_team_rounds plans a team again with its failed members first.
 * MOBROB_ERR_INVALID before any launch or copy for everything mobrob_ppo_plan_grid_time refuses of the spec, the scenes, the frames and
 * the time (spec->n_fields must be n_robots), and for: team_size not 1, 2, 4, 8 or 16, n_robots % team_size != 0, reserve outside 0 .. 4,
 * mates in different scenes, walk_cap < 1 with walk_out, one field above MOBROB_PLAN_TIME_MAX_BYTES or n_robots fields above it with
 * fields_team_out, a workgroup's LDS above the device's limit. */
int mobrob_ppo_plan_grid_team(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls /* or NULL */,
                              const mobrob_hazard_frames_t* hazards /* or NULL */, const mobrob_plan_time_t* time, int32_t team_size,
                              int32_t reserve, const float* start /* [n][pos_dim] */, const float* goal /* [n][pos_dim] */,
                              float* waypoints_out /* [n][K][pos_dim] */, int32_t* n_waypoints_out /* [n] */, int32_t* count_out /* [n] */,
                              int32_t* status_out /* [n] */, int32_t* cost_out /* [n] */, int32_t* waits_out /* [n][K] */,
                              int32_t* leave_out /* [n][K] */, int32_t* arrive_out /* [n] */, int32_t* sweeps_out /* [n] or NULL */,
                              uint16_t* walk_out /* [n][walk_cap] or NULL */, int32_t walk_cap, uint8_t* occ_time_out /* or NULL */,
                              int32_t* fields_team_out /* [n][T + 1][G][G] or NULL */, int32_t* workgroups_out /* or NULL */);

/* ---- priority reordering rounds of a team plan: the members that stayed parked plan first ------------------------------------------
 * mobrob_ppo_plan_grid_team, planned again inside the call with the failed members in front.  The rule is stated once in
 * mobrob_amd/envs/goal_rules.py (grid_plan_team(order=), plan_team_next_order, grid_plan_team_rounds) and reproduced bit for bit.
 *   rounds    every team on its own.  Round 0 plans in index order.  After a round the team's parked members are those without a walk
 *             (status 1 or 3; 2, truncated, has one).  Nobody parked: stop.  Otherwise the next order is the parked members, then the
 *             others, each in the relative order of this round; stop without planning it after `retries` (0 .. 8) reorderings or if that
 *             order was already planned for this team (which includes: the parked members are in front already).
 *   result    the round with the fewest parked members, the earliest on a tie: every output of mobrob_ppo_plan_grid_team is that
 *             round's, indexed by robot.  In a round, position p of the order plans member order[p] on the base layers OR the
 *             reservations of the members at the positions before p.  retries = 0: mobrob_ppo_plan_grid_team's outputs.
 *   outputs   mobrob_ppo_plan_grid_team's (the cells of walk_out beyond arrive are unspecified), and team_order_out [n_teams][team_size]
 *             (the result's order), team_rounds_out [n_teams] (rounds planned, >= 1), team_parked_out and team_parked_first_out
 *             [n_teams] (parked members of the result and of round 0).
 *   kernels   k_plan_occupancy_time as it is; k_plan_team_rounds: k_plan_team's workgroup, field and walk with the loop of rounds
 *             around the member loop.  Between two rounds one thread counts the parked, builds the next order and looks it up among
 *             the orders planned; a member's waits, leave and waypoints are zeroed before it walks again; where the last round planned
 *             is not the best, the team is planned once more in the best order (the plan is a function of the order), which
 *             team_rounds_out does not count: a call costs between 1 and retries + 2 team plans.  LDS: k_plan_team's + 16 +
 *             20 (retries + 1) bytes.  Workgroups: min(teams, compute units, MOBROB_PLAN_TIME_MAX_BYTES / bytes of one field); an
 *             environment variable MOBROB_PLAN_TIME_MAX_BYTES (decimal) lowers that cap on the scratch fields for this call, never
 *             below one field, and nothing else.
 * Not repaired: two mates whose start cells, or whose goal cells, are within `reserve` of each other fail in every order; an earlier
 * member still does not know a later member's start cell; the orders tried are one chain, not all of them.
 * MOBROB_ERR_INVALID before any launch or copy for everything mobrob_ppo_plan_grid_team refuses (the four team outputs included in "a
 * NULL argument"), and for retries outside 0 .. 8. */
int mobrob_ppo_plan_grid_team_rounds(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls /* or NULL */,
                                     const mobrob_hazard_frames_t* hazards /* or NULL */, const mobrob_plan_time_t* time,
                                     int32_t team_size, int32_t reserve, int32_t retries /* 0 .. 8 */,
                                     const float* start /* [n][pos_dim] */, const float* goal /* [n][pos_dim] */,
                                     float* waypoints_out /* [n][K][pos_dim] */, int32_t* n_waypoints_out /* [n] */,
                                     int32_t* count_out /* [n] */, int32_t* status_out /* [n] */, int32_t* cost_out /* [n] */,
                                     int32_t* waits_out /* [n][K] */, int32_t* leave_out /* [n][K] */, int32_t* arrive_out /* [n] */,
                                     int32_t* sweeps_out /* [n] or NULL */, uint16_t* walk_out /* [n][walk_cap] or NULL */,
                                     int32_t walk_cap, uint8_t* occ_time_out /* or NULL */,
                                     int32_t* fields_team_out /* [n][T + 1][G][G] or NULL */, int32_t* workgroups_out /* or NULL */,
                                     int32_t* team_order_out /* [n_teams][team_size] */, int32_t* team_rounds_out /* [n_teams] */,
                                     int32_t* team_parked_out /* [n_teams] */, int32_t* team_parked_first_out /* [n_teams] */);

/* ---- smoothing of a team plan: capped line-of-sight legs, reserved as swept regions ------------------------------------------------
 * mobrob_ppo_plan_grid_team with mobrob_ppo_plan_grid_time_smooth's waypoints.  The rule is stated once in
 * mobrob_amd/envs/goal_rules.py (grid_leg_cells, grid_smooth_time(max_leg), grid_reserve_legs, grid_team_clearance_legs,
 * grid_plan_team(smooth=True)) and reproduced bit for bit.
 *   map       member m plans on occ_t = base_t OR the swept reservations of the members 0 .. m - 1.  Field and walk are
 *             mobrob_ppo_plan_grid_team's, unchanged, on that map; the table nb is mobrob_ppo_plan_grid_time_smooth's built on that
 *             same map at `margin`, so it is the member's own.
 *   smooth    mobrob_ppo_plan_grid_time_smooth's loop with one more condition: the leg from anchor i to j + 1 is kept only if it is
 *             visible AND j + 1 - i <= max_leg.  max_leg = 1 keeps every cell of the walk (the reservation is then
 *             mobrob_ppo_plan_grid_team's); INT32_MAX: no cap.
 *   legs      the anchors are 0, the kept indices, A.  A leg (a, b) of one action has the cells {c[a], c[b]}; a longer one every cell
 *             the sight line visits: both ends, every cell stepped into, both cells that share a corner the line passes through.
 *   reserve   P_t, where the member can be during action t: the cells of the leg with a <= t < b for t < A, {c[A]} from A on.  Layer
 *             t < T holds every cell within Chebyshev distance `reserve` of P_t, the tail layer T of any P_t, t >= min(T, A).  A member
 *             without a walk reserves its start cell in every layer.
 *   guarantee two mates that keep to their legs -- leaving no anchor before its release step (leave, as
 *             mobrob_ppo_plan_grid_time_smooth's) and reaching the next no later than the walk does -- are in cells more than
 *             `reserve` apart whatever their speeds.  Not promised: more planned robots than mobrob_ppo_plan_grid_team plans (a long leg
 *             reserves all of itself for all of its span: hence max_leg), fewer waypoints, anything about a later member whose start
 *             cell an earlier member's leg covers (status 1).
 *   outputs   mobrob_ppo_plan_grid_team's, with leave_out and moves_out as mobrob_ppo_plan_grid_time_smooth's, waits_out zeroed, and
 *             keep_out [n][keep_cap] or NULL: the first min(count - 1, keep_cap) kept indices of every robot, the other slots 0 (count - 1
 *             of them exist: ask again with more room where that is above keep_cap).  Status 3: a loop bound (cells * cells sweeps,
 *             T + cells * cells actions or window rounds): count 0, cost -1, arrive 0, moves 0, waypoints, leave and kept indices zeroed,
 *             and the member reserves its start cell.
 *   kernels   k_plan_occupancy_time for the base layers, as it is; k_plan_team_smooth: a workgroup of 1024 threads per team at a time,
 *             per member four phases: field and table (the layer's blocked bytes in LDS: the byte at margin 0, the OR of its 3 x 3
 *             neighbours at margin 1), the walk by one thread, the smoothing by one wave (64 candidates at once, ballot and count of
 *             trailing zeros), the stamps by all threads (a wave per leg, a lane per layer of its span).  Scratch per workgroup: 7 bytes
 *             a cell and layer (field 4, table 2, reservation 1) plus the walk; the workgroups are min(teams, compute units,
 *             MOBROB_PLAN_TIME_MAX_BYTES / that).  LDS: 9 bytes a cell + 64.
 * MOBROB_ERR_INVALID before any launch or copy for everything mobrob_ppo_plan_grid_team refuses (moves_out included in "a NULL
 * argument"), and for: margin not 0 or 1, max_leg < 1, keep_cap < 1 with keep_out, one workgroup's scratch above
 * MOBROB_PLAN_TIME_MAX_BYTES, a workgroup's LDS above the device's limit. */
int mobrob_ppo_plan_grid_team_smooth(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls /* or NULL */,
                                     const mobrob_hazard_frames_t* hazards /* or NULL */, const mobrob_plan_time_t* time,
                                     int32_t team_size, int32_t reserve, int32_t margin /* 0 or 1 */, int32_t max_leg /* >= 1 */,
                                     const float* start /* [n][pos_dim] */, const float* goal /* [n][pos_dim] */,
                                     float* waypoints_out /* [n][K][pos_dim] */, int32_t* n_waypoints_out /* [n] */,
                                     int32_t* count_out /* [n] */, int32_t* status_out /* [n] */, int32_t* cost_out /* [n] */,
                                     int32_t* waits_out /* [n][K] */, int32_t* leave_out /* [n][K] */, int32_t* arrive_out /* [n] */,
                                     int32_t* moves_out /* [n] */, int32_t* sweeps_out /* [n] or NULL */,
                                     uint16_t* walk_out /* [n][walk_cap] or NULL */, int32_t walk_cap,
                                     int32_t* keep_out /* [n][keep_cap] or NULL */, int32_t keep_cap, uint8_t* occ_time_out /* or NULL */,
                                     int32_t* fields_team_out /* [n][T + 1][G][G] or NULL */, int32_t* workgroups_out /* or NULL */);

/* ---- goal assignment inside a team: who takes which goal, a minimum-cost matching ---------------------------------------------------
 * In front of the team planners, a call of its own: it changes their INPUT (goal[n]) and nothing of theirs.  The rule is stated once in
 * mobrob_amd/envs/goal_rules.py (grid_assign, plan_assign_match, plan_assign_team) and reproduced bit for bit, the potentials included.
 *   map       a static scene (hazards, or neither): mobrob_ppo_plan_grid's occupancy; hazard frames (with `time`): the tail layer T of
 *             mobrob_ppo_plan_grid_time's layers.  Reservations play no part: the matching is a function of (scene, starts, goals).
 *   matrix    per team C[i][j] = the cost-to-go of member i's start cell to member j's goal cell on that map (mobrob_ppo_plan_grid's
 *             field), MOBROB_PLAN_ASSIGN_NONE where there is no path: above any total of real costs, so a minimum-sum matching first
 *             minimises the pairs without a path.
 *   matching  objective 0 (sum): the minimum-total perfect matching by the shortest-augmenting-path Hungarian method, rows in index
 *             order, the unused column of least slack with the lowest index on a tie.  Objective 1 (makespan): L, the least value with a
 *             perfect matching among the entries <= L, then that method on C with the entries above L as MOBROB_PLAN_ASSIGN_FORBID: the
 *             largest member cost first, then the total.  Identity first: where the identity's total (makespan: its largest entry and
 *             total) equals the matching's, the identity is the result.
 *   outputs   assign_out [n]: the robot, a mate or itself, whose goal robot i is given; goal_out [n][pos_dim] = goal[assign];
 *             assign_cost_out [n] (-1: no path); total_out [2][n_teams] int64: the result's total, the identity's (NONE counted as NONE);
 *             team_out [4][n_teams]: the result's largest entry, the identity's, changed (0 / 1), status (0; 3: a field hit its sweep
 *             bound or a loop its bound -- the team keeps the identity, potentials 0); u_out, v_out [n] int64: the row and column
 *             potentials of the last matching run, u[i] + v[j] <= C'[i][j] with equality on the matched pairs; matrix_out
 *             [n_teams][team_size][team_size] or NULL: C with -1 for NONE; sweeps_out [n] or NULL: the relaxation sweeps of each field.
 *   kernels   k_plan_occupancy or k_plan_occupancy_time as they are; k_plan_assign_cost: a workgroup of 1024 threads per robot, its
 *             goal's field in LDS (5 bytes a cell, as k_plan_field's), of which only the team_size words at the mates' start cells are
 *             written out; k_plan_assign: a wave per team, lanes as columns.  It works in the team plans' buffer; nothing stays resident.
 * MOBROB_ERR_INVALID before any launch or copy for: a NULL argument, hazards and frames both, `time` without frames or frames without
 * it, an objective other than 0 or 1, reuse_id != 0, n_fields != n_robots, a team_size other than 1, 2, 4, 8, 16 or one that does not
 * divide n_robots, mates in different scenes, non-finite starts or goals, everything mobrob_ppo_plan_grid refuses of the spec and the
 * scenes and mobrob_ppo_plan_grid_time of the frames and the time, a field too large for the device's LDS per workgroup. */
#define MOBROB_PLAN_ASSIGN_NONE (1 << 21)
#define MOBROB_PLAN_ASSIGN_FORBID (1 << 26)
int mobrob_ppo_plan_assign(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls /* or NULL */,
                           const mobrob_hazards_t* hazards /* or NULL */, const mobrob_hazard_frames_t* frames /* or NULL */,
                           const mobrob_plan_time_t* time /* with frames, else NULL */, int32_t team_size, int32_t objective /* 0 sum, 1 makespan */,
                           const float* start /* [n][pos_dim] */, const float* goal /* [n][pos_dim] */, int32_t* assign_out /* [n] */,
                           float* goal_out /* [n][pos_dim] */, int32_t* assign_cost_out /* [n] */, int64_t* total_out /* [2][n_teams] */,
                           int32_t* team_out /* [4][n_teams] */, int64_t* u_out /* [n] */, int64_t* v_out /* [n] */,
                           int32_t* matrix_out /* [n_teams][team_size][team_size] or NULL */, int32_t* sweeps_out /* [n] or NULL */);

/* ---- run specifications: reach / avoid / until robustness per robot, from the positions of a run ----------------------------------
 * The rule is stated once in mobrob_amd/envs/goal_rules.py (Regions, region_margins, spec_predicate, spec_fold) and k_spec_monitor
 * (csrc/kernels_spec.h) reproduces it bit for bit.  A scene is up to MOBROB_SPEC_REGIONS_MAX regions: kind 0 a box (cx, cy, hx, hy),
 * kind 1 a circle (cx, cy, r, 0); only x and y count.  The specification is the conjunction of n_clauses clauses; clause c is
 * (op[c], window [a[c], b[c]] in sample time tau = global steps completed, predicate 1, and for UNTIL predicate 2); a predicate is
 * the range of regions [lo, hi) read as their union and `out` (0: inside, 1: outside).  Per robot and clause the call carries
 * val = (rho, guard) and wit = the witness sample; the state before a robot's first sample is rho = +inf (ALWAYS) or -inf, guard =
 * +inf, wit = -1 (the caller's to set).
 *   path      host [T + 1][n][P], time-major, as mobrob_ppo_follow_waypoints* writes it with path_stride 1: record 0 the position at
 *             entry.  step0 == 0: records 0 .. T are the samples tau = 0 .. T; step0 > 0: record 0 is skipped (the previous call
 *             folded it) and records 1 .. T are tau = step0 + 1 .. step0 + T.
 *   val, wit  host [n][n_clauses][2] float and [n][n_clauses] int32, in and out.
 * The path is uploaded into a buffer of the monitor's own, outside the arena: rollout, training and evaluation buffers are untouched.
 * MOBROB_ERR_INVALID before any launch or copy, naming the argument, for: a NULL pointer; n < 1, T < 1, P outside 1 .. 3, n_scenes <
 * 1, max_regions outside 0 .. 64, n_clauses outside 1 .. 16, a scene's count outside 0 .. max_regions, several scenes without a
 * scene index, a scene index outside 0 .. n_scenes - 1, a kind other than 0 or 1, a region that is not finite or has a negative
 * extent; a path above MOBROB_SPEC_PATH_MAX_BYTES; step0 < 0 or step0 + T above INT32_MAX; an op outside 0 .. 2; a window with a < 0
 * or a > b; a region range outside 0 <= lo <= hi <= max_regions; a non-finite position (the robot and the record are named). */
#define MOBROB_SPEC_REGIONS_MAX 64
#define MOBROB_SPEC_CLAUSES_MAX 16
#define MOBROB_SPEC_OPEN 2147483647 /* the right end of an open window */
#define MOBROB_SPEC_ALWAYS 0
#define MOBROB_SPEC_EVENTUALLY 1
#define MOBROB_SPEC_UNTIL 2
#define MOBROB_SPEC_PATH_MAX_BYTES (256u << 20)
typedef struct {
  int32_t n_scenes, max_regions;
  const float* regions;      /* [n_scenes][max_regions][4]                                 */
  const int32_t* kinds;      /* [n_scenes][max_regions]: 0 box, 1 circle                   */
  const int32_t* n_regions;  /* [n_scenes] regions in use                                  */
  const int32_t* scene;      /* [n] scene of each robot, or NULL (n_scenes must be 1)      */
  int32_t n_clauses;
  int32_t op[MOBROB_SPEC_CLAUSES_MAX];
  int32_t a[MOBROB_SPEC_CLAUSES_MAX], b[MOBROB_SPEC_CLAUSES_MAX];
  int32_t lo1[MOBROB_SPEC_CLAUSES_MAX], hi1[MOBROB_SPEC_CLAUSES_MAX], out1[MOBROB_SPEC_CLAUSES_MAX];
  int32_t lo2[MOBROB_SPEC_CLAUSES_MAX], hi2[MOBROB_SPEC_CLAUSES_MAX], out2[MOBROB_SPEC_CLAUSES_MAX];   /* UNTIL only */
} mobrob_spec_t;
int mobrob_ppo_spec_monitor(mobrob_ppo_engine_t* e, const mobrob_spec_t* spec, const float* path /* [T + 1][n][P] */, int32_t n,
                            int32_t T, int32_t P, int32_t step0, float* val /* [n][n_clauses][2] */, int32_t* wit /* [n][n_clauses] */);

/* ---- nested run specifications: stay-for and recurring visits ----------------------------------------------------------------------
 * mobrob_ppo_spec_monitor with two more ops, each over the sliding window of the last hold + 1 values of predicate 1 (the rule:
 * goal_rules.spec_fold; k_spec_monitor_nested, csrc/kernels_spec_nested.h, reproduces it bit for bit):
 *   MOBROB_SPEC_STAY   eventually_[a,b] always_[0,hold]:  at tau >= hold with a <= tau - hold <= b, s = the window's minimum;
 *                      s > rho: rho = s, witness = tau - hold.  rho starts at -inf.
 *   MOBROB_SPEC_RECUR  always_[a,b] eventually_[0,hold]:  s = the window's maximum; s < rho: rho = s, witness = tau - hold.  rho
 *                      starts at +inf.
 * [a, b] bounds the START of the inner window.  The window's extremum is taken under the total order on float bits (key = i ^ ((i >>
 * 31) & 0x7fffffff) on the int32 view: -0.0 < +0.0), the outer comparison is the float comparison.  guard is not used and stays
 * +inf.  A window the run ends before completing is not folded.  hold = 0 is EVENTUALLY / ALWAYS bit for bit.  The flat ops are
 * folded exactly as mobrob_ppo_spec_monitor folds them.
 *   hold      per clause, 0 .. MOBROB_SPEC_HOLD_MAX for STAY / RECUR and 0 for a flat op; the sum of (hold + 1) over the nested
 *             clauses is at most MOBROB_SPEC_WINDOW_SLOTS.
 *   tail, W   host [n][W] float, in and out, W the sum of the holds: for each nested clause, in clause order, the last `hold` values
 *             of its predicate, oldest first.  Before a robot's first sample every entry is +inf (STAY) or -inf (RECUR), the caller's
 *             to set.  NULL is allowed when W == 0.
 * The call uses the monitor's own buffer outside the arena, as mobrob_ppo_spec_monitor does.  MOBROB_ERR_INVALID before any launch or
 * copy, val, wit and tail untouched, for everything mobrob_ppo_spec_monitor refuses (an op outside 0 .. 4 here) and for: a hold
 * outside 0 .. 255; a hold other than 0 on a flat op; windows above the slot cap; a W that is not the sum of the holds; a NULL tail
 * with W > 0. */
#define MOBROB_SPEC_STAY 3
#define MOBROB_SPEC_RECUR 4
#define MOBROB_SPEC_HOLD_MAX 255
#define MOBROB_SPEC_WINDOW_SLOTS 512
typedef struct {
  int32_t n_scenes, max_regions;   /* mobrob_spec_t's fields, in its order ...                   */
  const float* regions;
  const int32_t* kinds;
  const int32_t* n_regions;
  const int32_t* scene;
  int32_t n_clauses;
  int32_t op[MOBROB_SPEC_CLAUSES_MAX];
  int32_t a[MOBROB_SPEC_CLAUSES_MAX], b[MOBROB_SPEC_CLAUSES_MAX];
  int32_t lo1[MOBROB_SPEC_CLAUSES_MAX], hi1[MOBROB_SPEC_CLAUSES_MAX], out1[MOBROB_SPEC_CLAUSES_MAX];
  int32_t lo2[MOBROB_SPEC_CLAUSES_MAX], hi2[MOBROB_SPEC_CLAUSES_MAX], out2[MOBROB_SPEC_CLAUSES_MAX];
  int32_t hold[MOBROB_SPEC_CLAUSES_MAX];   /* ... then the inner window of each clause             */
} mobrob_spec_nested_t;
int mobrob_ppo_spec_monitor_nested(mobrob_ppo_engine_t* e, const mobrob_spec_nested_t* spec, const float* path /* [T + 1][n][P] */,
                                   int32_t n, int32_t T, int32_t P, int32_t step0, float* val /* [n][n_clauses][2] */,
                                   int32_t* wit /* [n][n_clauses] */, float* tail /* [n][W] or NULL */, int32_t W);

/* ---- run specifications over things that move: moving regions and predicates on team-mates -----------------------------------------
 * mobrob_ppo_spec_monitor_nested with a frame axis on the region table and two more kinds of predicate (the rule: goal_rules.py,
 * MovingRegions, spec_mate_predicate, spec_fold; k_spec_monitor_moving, csrc/kernels_spec_moving.h, reproduces it bit for bit):
 *   frames    regions is [n_scenes][n_frames][max_regions][4]; kinds and n_regions have no frame axis.  The sample at tau reads the
 *             frame f(max(tau - 1, 0)), f(g) = min(g / frame_steps, n_frames - 1), or (g / frame_steps) % n_frames with loop = 1:
 *             the frame that mobrob_ppo_follow_waypoints_hazard_frames used in the check of the step before the sample.
 *   kind1, kind2   what predicate 1 / 2 of a clause reads: MOBROB_SPEC_PRED_REGIONS its region range, as before;
 *             MOBROB_SPEC_PRED_TOGETHER / _APART the robot's team-mates at this sample's record (the region range is ignored and
 *             must be a legal one, [0, 0) for instance).  Robot i has the mates j = (i / team_size) * team_size + m, m ascending,
 *             j != i; g_j = rad - sqrt(dx * dx + dy * dy), dx = px_i - px_j, every operation rounded on its own.  TOGETHER is the
 *             minimum of the g_j by explicit < from +inf, APART minus their maximum by explicit > from -inf; a team of one reads
 *             +inf for both.  kind2 and rad2 count for UNTIL only.
 *   rad1, rad2     the distance d of a mate predicate; finite and >= 0 in every clause (0 for a region predicate).
 * n_frames = 1, team_size = 1 and kinds of 0 give mobrob_ppo_spec_monitor_nested's bits.  The call uses the monitor's own buffer
 * outside the arena.  MOBROB_ERR_INVALID before any launch or copy, val, wit and tail untouched, for everything
 * mobrob_ppo_spec_monitor_nested refuses and for: a team_size other than 1, 2, 4, 8, 16; n not a multiple of team_size; a kind
 * outside 0 .. 2; a radius that is negative or not finite; n_frames < 1; frame_steps < 1; loop other than 0 or 1; a region table
 * above MOBROB_SPEC_FRAMES_MAX_BYTES; a region that is not finite or has a negative extent in any frame. */
#define MOBROB_SPEC_PRED_REGIONS 0
#define MOBROB_SPEC_PRED_TOGETHER 1
#define MOBROB_SPEC_PRED_APART 2
#define MOBROB_SPEC_FRAMES_MAX_BYTES (64u << 20)
typedef struct {
  int32_t n_scenes, max_regions;   /* mobrob_spec_nested_t's fields, in its order ...            */
  const float* regions;            /* [n_scenes][n_frames][max_regions][4]                       */
  const int32_t* kinds;
  const int32_t* n_regions;
  const int32_t* scene;
  int32_t n_clauses;
  int32_t op[MOBROB_SPEC_CLAUSES_MAX];
  int32_t a[MOBROB_SPEC_CLAUSES_MAX], b[MOBROB_SPEC_CLAUSES_MAX];
  int32_t lo1[MOBROB_SPEC_CLAUSES_MAX], hi1[MOBROB_SPEC_CLAUSES_MAX], out1[MOBROB_SPEC_CLAUSES_MAX];
  int32_t lo2[MOBROB_SPEC_CLAUSES_MAX], hi2[MOBROB_SPEC_CLAUSES_MAX], out2[MOBROB_SPEC_CLAUSES_MAX];
  int32_t hold[MOBROB_SPEC_CLAUSES_MAX];
  int32_t kind1[MOBROB_SPEC_CLAUSES_MAX], kind2[MOBROB_SPEC_CLAUSES_MAX];   /* ... then what each predicate reads ... */
  float rad1[MOBROB_SPEC_CLAUSES_MAX], rad2[MOBROB_SPEC_CLAUSES_MAX];       /* ... a mate predicate's distance ...    */
  int32_t team_size, n_frames, frame_steps, loop;                           /* ... the teams and the frames           */
} mobrob_spec_moving_t;
int mobrob_ppo_spec_monitor_moving(mobrob_ppo_engine_t* e, const mobrob_spec_moving_t* spec, const float* path /* [T + 1][n][P] */,
                                   int32_t n, int32_t T, int32_t P, int32_t step0, float* val /* [n][n_clauses][2] */,
                                   int32_t* wit /* [n][n_clauses] */, float* tail /* [n][W] or NULL */, int32_t W);

/* ---- a plan from a specification: the order of the stations and the stitched waypoints ----------------------------------------------
 * The planner and the specifications meet here: the avoid clauses of a specification become obstacles, its reach clauses stations, and
 * per robot the device chooses the order of the stations and stitches the waypoints, for all robots in one call.  The rule is stated once
 * in mobrob_amd/envs/goal_rules.py (spec_plan_parse, spec_plan_occupancy, spec_plan_stations, spec_plan_tour, spec_plan) and reproduced bit
 * for bit.  The caller has sorted the clauses: here a station is a range of regions [lo, hi) read as their union, an avoid clause likewise.
 *   spec      mobrob_ppo_plan_grid's, with n_scenes the REGIONS' scenes (which the walls' and hazards' must equal where those exist),
 *             n_fields the distinct (scene, goal cell) pairs of `goal` (0 without a goal) and reuse_id 0.
 *   regions   the region table as mobrob_ppo_spec_monitor takes it: n_scenes, max_regions, regions, kinds, n_regions, scene are read, the
 *             clauses are not.
 *   map       mobrob_ppo_plan_grid's occupancy (zeros without walls and hazards), OR-ed per scene with the avoid regions: a cell is
 *             blocked when a region r of an avoid range, r below the scene's count, has an inside margin >= -inflate at the cell's centre.
 *   anchors   per scene and station, over the unblocked cells, the cell of the largest inside margin m of the station's range (the total
 *             order on float bits, the lowest cell on a tie): station_margin_out [S][M] is that m (-inf without an unblocked cell) and
 *             station_cell_out [S][M] the cell where m > 0, else -1 -- every robot of such a scene has status 1.
 *   costs     one mobrob_ppo_plan_grid field per (scene, anchor) and per goal field, all in ONE launch; matrix_out [S][M][M]: the field
 *             of station j at the anchor of station i, -1 none.
 *   order     in ticks (5 an orthogonal move, 7 a diagonal): open_c, close_c, dwell_c [M] are the stations' windows and dwells in ticks.
 *             dep(j, arr) = max(arr, open_c[j]) + dwell_c[j], feasible iff max(arr, open_c[j]) <= close_c[j]; Held-Karp over the subsets
 *             of stations, every minimum that of the pair (value, predecessor), the end station minimising (ticks + the goal leg, j).
 *   outputs   mobrob_ppo_plan_grid's waypoints, n_waypoints, count, status (0 planned, 1 no feasible tour, 2 truncated to the first K,
 *             3 a loop hit its bound) and cost (the ticks at the end, waits included; -1); tour_order_out [n][M]: the station at each
 *             position; tour_eta_out [n][M]: ticks on arrival, before the wait for the opening; station_waypoint_out [n][M]: the index
 *             in the full path of each position's anchor waypoint; release_out [n][K]: at the slot of the waypoint after a station whose
 *             departure exceeds its arrival, min(ceil(departure * pace / 5), INT32_MAX), else 0 (a mobrob_follow_schedule_t's release);
 *             the -1 of a robot without a tour fills its tour_order, tour_eta and station_waypoint.  z of every waypoint: the goal's,
 *             else the start's.  occupancy_out [S][G][G] and sweeps_out [S * M + n_fields] or NULL.
 *   kernels   k_plan_occupancy and k_plan_field as they are; csrc/kernels_plan_spec.h: k_plan_region_occupancy (a thread per scene and
 *             cell), k_plan_station (a workgroup per scene and station, which writes the anchor into the field list), k_plan_tour_matrix,
 *             k_plan_tour (a wave per robot, the table of 256 x 8 values in LDS), k_plan_tour_path (a thread per robot).  The call works
 *             in a buffer of its own, outside the arena; mobrob_ppo_plan_grid's resident fields stay valid across it.
 * MOBROB_ERR_INVALID before any launch or copy, outputs untouched, for: a NULL argument; a goal without its field lists; reuse_id != 0;
 * n_fields != 0 without a goal; n_stations outside 1 .. MOBROB_PLAN_TOUR_STATIONS_MAX; n_avoid outside 0 .. MOBROB_SPEC_CLAUSES_MAX; pace
 * outside 1 .. 2^20; everything mobrob_ppo_plan_grid refuses of the spec, the scenes, the robots and the goal fields, and
 * mobrob_ppo_spec_monitor of the region table; n_scenes not the regions'; regions that disagree with the walls / hazards on a robot's
 * scene; a station's or an avoid clause's range outside 0 <= lo <= hi <= max_regions; ticks negative or above
 * MOBROB_PLAN_TOUR_TICKS_MAX; open_c > close_c; fields above MOBROB_PLAN_TIME_MAX_BYTES in total; a field too large for the device's LDS. */
#define MOBROB_PLAN_TOUR_STATIONS_MAX 8
#define MOBROB_PLAN_TOUR_TICKS_MAX (1 << 24)
int mobrob_ppo_spec_plan(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls /* or NULL */,
                         const mobrob_hazards_t* hazards /* or NULL */, const mobrob_spec_t* regions, int32_t n_stations,
                         const int32_t* station_lo /* [M] */, const int32_t* station_hi /* [M] */, int32_t n_avoid,
                         const int32_t* avoid_lo /* [n_avoid] or NULL */, const int32_t* avoid_hi /* [n_avoid] or NULL */,
                         const int32_t* open_c /* [M] */, const int32_t* close_c /* [M] */, const int32_t* dwell_c /* [M] */, int32_t pace,
                         const float* start /* [n][pos_dim] */, const float* goal /* [n][pos_dim] or NULL */,
                         const int32_t* field_of /* [n], with a goal */, const int32_t* field_goal_cell /* [n_fields], with a goal */,
                         const int32_t* field_scene /* [n_fields], with a goal */, float* waypoints_out /* [n][K][pos_dim] */,
                         int32_t* n_waypoints_out /* [n] */, int32_t* count_out /* [n] */, int32_t* status_out /* [n] */,
                         int32_t* cost_out /* [n] */, int32_t* tour_order_out /* [n][M] */, int32_t* tour_eta_out /* [n][M] */,
                         int32_t* station_waypoint_out /* [n][M] */, int32_t* release_out /* [n][K] */,
                         int32_t* station_cell_out /* [S][M] */, float* station_margin_out /* [S][M] */, int32_t* matrix_out /* [S][M][M] */,
                         uint8_t* occupancy_out /* [S][G][G] or NULL */, int32_t* sweeps_out /* [S * M + n_fields] or NULL */);

/* The same plan from the middle of a run (goal_rules.spec_plan with state=, step0=, partial=; csrc/kernels_plan_spec_resume.h).  Every
 * argument of mobrob_ppo_spec_plan means what it means there, and the same checks are made; in addition
 *   todo         [n]: bit j set = robot r still has to visit station j (the caller reads the monitor's carried state: a station is done
 *                when the rho of its clause is > 0).  The tour table is filled for the subsets of todo[r] only -- enumerated, not filtered.
 *   step0_ticks  t0 = ceil(5 * step0 / pace), the tick the plan starts at: t[{j}][j] = dep(j, t0 + d0[j]).  Windows, cost, tour_eta and
 *                release stay absolute.
 *   partial      0: the tour visits all of todo[r], or the status is 1 (with todo[r] == 0 the plan is the goal leg alone, cost t0 + its
 *                ticks, and without a goal planned with count 0).  1: the visited set V, a subset of todo[r], and its last station j
 *                are the lexicographic minimum of (popcount(todo) - popcount(V), t[V][j] + E[j], V, j) over the feasible entries, V = 0
 *                an entry with the total t0 + the goal leg from the start and j = -1; status 1 only without any feasible entry.
 *   outputs      tour_len_out [n] = |V| and dropped_out [n] = todo & ~V (0 and todo without a feasible entry); tour_order, tour_eta and
 *                station_waypoint are -1 at the positions >= tour_len.
 *   kernels      k_plan_tour_resume (a wave per robot; the submasks of todo sorted by level in LDS, the selection a wave-wide minimum)
 *                and k_plan_tour_path_legs (16 lanes a robot, a lane a leg: count, prefix sum across the lanes, emit) in place of
 *                k_plan_tour and k_plan_tour_path; everything before them as mobrob_ppo_spec_plan runs it.
 * MOBROB_ERR_INVALID, outputs untouched, for everything mobrob_ppo_spec_plan refuses and for: todo, tour_len_out or dropped_out NULL;
 * step0_ticks outside 0 .. MOBROB_PLAN_TOUR_TICKS_MAX; a todo with a bit at or above n_stations (or negative); partial not 0 / 1. */
int mobrob_ppo_spec_replan(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls /* or NULL */,
                           const mobrob_hazards_t* hazards /* or NULL */, const mobrob_spec_t* regions, int32_t n_stations,
                           const int32_t* station_lo /* [M] */, const int32_t* station_hi /* [M] */, int32_t n_avoid,
                           const int32_t* avoid_lo /* [n_avoid] or NULL */, const int32_t* avoid_hi /* [n_avoid] or NULL */,
                           const int32_t* open_c /* [M] */, const int32_t* close_c /* [M] */, const int32_t* dwell_c /* [M] */, int32_t pace,
                           const float* start /* [n][pos_dim] */, const float* goal /* [n][pos_dim] or NULL */,
                           const int32_t* field_of /* [n], with a goal */, const int32_t* field_goal_cell /* [n_fields], with a goal */,
                           const int32_t* field_scene /* [n_fields], with a goal */, const int32_t* todo /* [n] */, int32_t step0_ticks,
                           int32_t partial, float* waypoints_out /* [n][K][pos_dim] */, int32_t* n_waypoints_out /* [n] */,
                           int32_t* count_out /* [n] */, int32_t* status_out /* [n] */, int32_t* cost_out /* [n] */,
                           int32_t* tour_order_out /* [n][M] */, int32_t* tour_eta_out /* [n][M] */,
                           int32_t* station_waypoint_out /* [n][M] */, int32_t* release_out /* [n][K] */,
                           int32_t* station_cell_out /* [S][M] */, float* station_margin_out /* [S][M] */,
                           int32_t* matrix_out /* [S][M][M] */, uint8_t* occupancy_out /* [S][G][G] or NULL */,
                           int32_t* sweeps_out /* [S * M + n_fields] or NULL */, int32_t* tour_len_out /* [n] */,
                           int32_t* dropped_out /* [n] */);

/* The same plan with the stations shared within a team (goal_rules.spec_plan with share=, objective=; csrc/kernels_plan_spec_share.h).
 * Every argument of mobrob_ppo_spec_replan means what it means there, and the same checks are made; in addition
 *   team_size    1, 2, 4, 8 or 16 consecutive robots: team r / team_size, member r % team_size; n_robots is a multiple of it.  T, the
 *                stations the team still has to visit, is the bitwise AND of its members' todo (reduced on the host).
 *   objective    0 makespan: the smallest largest member cost and under it the smallest sum of the member costs; 1 sum.
 *   partial      0: the team covers all of T, or every member has status 1 with count 0, cost -1, orders -1 and share 0.  1: the covered
 *                set C is the lexicographic minimum of (popcount(T) - popcount(U), f[U], U) over the feasible U, f the primary pass.
 *   outputs      share_out [n]: the stations of member r, a partition of C within the team.  The member's tour, waypoints and releases
 *                are those of mobrob_ppo_spec_replan with todo = share and partial 0; cost_out is best[r][share[r]]; dropped_out is 0
 *                for a member of a team with an allotment (with team_size 1 the team's loss) and T without one.  Per team, [n /
 *                team_size]: team_cover_out = C, team_dropped_out = T & ~C, team_makespan_out the largest member cost,
 *                team_total_out (int64) their sum; 0, T, -1 and -1 for a team without an allotment.
 *   kernels      after the tour matrix k_plan_tour_best (a wave per robot, k_plan_tour_resume's table over the subsets of T -> best
 *                [n][256]) and k_plan_team_share (a wave per team: best in LDS, the partition DP over the members with the lanes on
 *                the sets U and their submasks enumerated ascending, the covered set a wave-wide minimum, the backtrack by lane 0);
 *                then k_plan_tour_resume over the shares, k_plan_team_void (a thread per robot: the members of a team without an
 *                allotment) and k_plan_tour_path_legs.
 * With team_size 1 every output it shares with mobrob_ppo_spec_replan equals that call's, for both objectives.
 * MOBROB_ERR_INVALID, outputs untouched, for everything mobrob_ppo_spec_replan refuses and for: a team_size not 1, 2, 4, 8 or 16;
 * n_robots % team_size != 0; an objective not 0 / 1; share_out or a team output NULL. */
int mobrob_ppo_spec_plan_share(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls /* or NULL */,
                               const mobrob_hazards_t* hazards /* or NULL */, const mobrob_spec_t* regions, int32_t n_stations,
                               const int32_t* station_lo /* [M] */, const int32_t* station_hi /* [M] */, int32_t n_avoid,
                               const int32_t* avoid_lo /* [n_avoid] or NULL */, const int32_t* avoid_hi /* [n_avoid] or NULL */,
                               const int32_t* open_c /* [M] */, const int32_t* close_c /* [M] */, const int32_t* dwell_c /* [M] */,
                               int32_t pace, const float* start /* [n][pos_dim] */, const float* goal /* [n][pos_dim] or NULL */,
                               const int32_t* field_of /* [n], with a goal */, const int32_t* field_goal_cell /* [n_fields], with a goal */,
                               const int32_t* field_scene /* [n_fields], with a goal */, const int32_t* todo /* [n] */,
                               int32_t step0_ticks, int32_t partial, int32_t team_size, int32_t objective,
                               float* waypoints_out /* [n][K][pos_dim] */, int32_t* n_waypoints_out /* [n] */,
                               int32_t* count_out /* [n] */, int32_t* status_out /* [n] */, int32_t* cost_out /* [n] */,
                               int32_t* tour_order_out /* [n][M] */, int32_t* tour_eta_out /* [n][M] */,
                               int32_t* station_waypoint_out /* [n][M] */, int32_t* release_out /* [n][K] */,
                               int32_t* station_cell_out /* [S][M] */, float* station_margin_out /* [S][M] */,
                               int32_t* matrix_out /* [S][M][M] */, uint8_t* occupancy_out /* [S][G][G] or NULL */,
                               int32_t* sweeps_out /* [S * M + n_fields] or NULL */, int32_t* tour_len_out /* [n] */,
                               int32_t* dropped_out /* [n] */, int32_t* share_out /* [n] */,
                               int32_t* team_cover_out /* [n / team_size] */, int32_t* team_dropped_out /* [n / team_size] */,
                               int32_t* team_makespan_out /* [n / team_size] */, int64_t* team_total_out /* [n / team_size] */);

/* ---- gSDE (use_sde = 1) ------------------------------------------------------------------------
 * policy.reset_noise(n_envs) (SB3 ActorCriticPolicy.reset_noise -> sample_weights): new exploration matrices for every environment
 * and the single matrix predict() uses for batches of another size, from the CURRENT log_std.  The rollout collectors call it
 * themselves at the start of a rollout and every sde_sample_freq steps (OnPolicyAlgorithm.collect_rollouts). */
int mobrob_ppo_sde_reset_noise(mobrob_ppo_engine_t* e);
/* The exploration matrices as an INPUT (tests, the oracle; like `eps` of mobrob_ppo_act): z = standard normals [n_envs][HL][A] ->
 * matrices z * exp(log_std), kept until the next call -- the collectors stop resampling on their own.  z = NULL: back to the
 * engine's own draws. */
int mobrob_ppo_sde_set_noise(mobrob_ppo_engine_t* e, const float* z);

/* ---- device buffers (tests, DP collectives, profiling) --------------------------------------- */
enum {
  MOBROB_BUF_OBS = 0,        /* f32 [T+1][N][Dp]  (Dp = D rounded up to 8; slot T = last_obs)     */
  MOBROB_BUF_ACTIONS = 1,    /* f32 [T][N][A]                                                    */
  MOBROB_BUF_REWARDS = 2,    /* f32 [T][N]                                                       */
  MOBROB_BUF_EPISODE_STARTS = 3, /* f32 [T][N]                                                   */
  MOBROB_BUF_VALUES = 4,     /* f32 [T][N]                                                       */
  MOBROB_BUF_LOG_PROBS = 5,  /* f32 [T][N]                                                       */
  MOBROB_BUF_ADVANTAGES = 6, /* f32 [T][N]                                                       */
  MOBROB_BUF_RETURNS = 7,    /* f32 [T][N]                                                       */
  MOBROB_BUF_PARAMS = 8,     /* f32 [P]                                                          */
  MOBROB_BUF_GRADS = 9,      /* f32 [P]   -- all-reduce target                                   */
  MOBROB_BUF_ADVSTAT = 10,   /* f64 [n_minibatches][4] (sum, sumsq, count, pad) -- all-reduce    */
  MOBROB_BUF_LAST_VALUES = 11, /* f32 [N]                                                        */
  MOBROB_BUF_LAST_DONES = 12,  /* f32 [N] (0/1)                                                  */
  MOBROB_BUF_CLIPPED_ACTIONS = 13, /* f32 [N][A] of the most recent act                          */
  MOBROB_BUF_EPISODE_START_STATE = 14, /* f32 [N] `_last_episode_starts` carried between rollouts   */
  MOBROB_BUF_TERMINAL_OBS = 15,    /* f32 [N][Dp] terminal observations of the rows truncated in the latest step */
  MOBROB_BUF_TERMINAL_VALUES = 16, /* f32 [N] V(terminal_obs) of those rows (time-limit bootstrap)              */
  MOBROB_BUF_TRUNCATED = 17,       /* u8  [N] TimeLimit.truncated flags of the latest step                       */
  MOBROB_BUF_ENV_STATE = 18,       /* f32 [N][12] goal-env state: pos[3] vel[3] goal[3] return length pad         */
  MOBROB_BUF_GRAD_EXCHANGE = 19,   /* f32 [P + 8]: the gradient followed by the eight loss sums of the minibatch (policy, value,
                                      approx_kl, clip fraction, row count, ...) -- what a data-parallel step sums across ranks */
  MOBROB_BUF_SDE_NOISE = 20,       /* f32 [N][HL][A] the environments' gSDE exploration matrices (use_sde engines only)          */
  MOBROB_BUF_COUNT = 21
};
/* Device pointer and size of a buffer.  Asking for the POINTER of ACTIONS / VALUES / LOG_PROBS / ADVANTAGES / RETURNS tells the
 * engine that the caller may write those arrays behind its back: the packed per-row training records the 256-wide gradient
 * kernel reads are then re-packed before every gradient launch instead of once per rollout (ptr_dev == NULL
 * queries the size only and changes nothing).  write_buffer needs no such care: it invalidates the records itself. */
int mobrob_ppo_buffer_info(mobrob_ppo_engine_t* e, int32_t which, void** ptr_dev, size_t* bytes);
/* copy with host layout [..][D] <-> device layout [..][Dp] handled for MOBROB_BUF_OBS */
int mobrob_ppo_read_buffer(mobrob_ppo_engine_t* e, int32_t which, void* host_out, size_t bytes);
int mobrob_ppo_write_buffer(mobrob_ppo_engine_t* e, int32_t which, const void* host_in, size_t bytes);
/* mark the rollout as complete (tests that inject a rollout with write_buffer) */
int mobrob_ppo_mark_rollout_ready(mobrob_ppo_engine_t* e);

/* Which matrix products of this engine run on the bf16 pipe with three-way split float32 operands (config.forward_x3, 256-wide tanh
 * nets): bit 0 = rollout policy forward and batched value pass, bit 1 = the hidden-layer products inside the gradient kernel (forward,
 * dh1, dW2, dW1; heads <= 16 wide, observation rows of 16 / 32 / 64 padded columns), bit 2 = that gradient kernel is the register-chained
 * k_chain_train (csrc/kernels_chain.h; MOBROB_NO_CHAIN=1 keeps k_fused_train<.., X3>).  0: everything on v_mfma_f32.  Measurement code
 * prices the kernels against the matrix peak of the pipe each product ran on (bench.py). */
int mobrob_ppo_x3_mode(const mobrob_ppo_engine_t* e);
/* How the latest mobrob_ppo_train / train_enqueue ran SB3's PPO.train (/root/reference/src/mobrob/rl_control/ppo.py:73-74): bit 0 = every
 * epoch as ONE co-operative launch (k_epoch64: gradient -> grid barrier -> fixed-order slab reduction -> grid barrier -> clip + Adam + packs
 * -> grid barrier, per minibatch; single rank, 64-wide networks, minibatches of at most 64 tiles, no target_kl), 0 = three launches per
 * optimizer step.  Same bits either way.  Every wait of the co-operative form is bounded (MOBROB_EPOCH_TIMEOUT_S, default 10): if a launch
 * gives up (workgroups not resident together), mobrob_ppo_train restores the snapshot it took of parameters and moments and re-runs the
 * update as three launches per step -- the call succeeds, the engine keeps that form, this query returns 0 from then on;
 * mobrob_ppo_train_enqueue (no snapshot) fails at the next synchronising call instead. */
int mobrob_ppo_update_mode(const mobrob_ppo_engine_t* e);

/* Switches the one-launch evaluation / waypoint-following kernel of fused 2x256 tanh engines (k_goal256_tile, csrc/kernels_eval256.h)
 * on or off for this engine.  It is OFF unless told: with it on, mobrob_ppo_evaluate_goal_env, mobrob_ppo_follow_waypoints, _resume and
 * _scheduled calls without hazards, teams or walls run as one launch and return 1 (persistent); every other call runs the per-step
 * path as before and returns 0.  The actor of that kernel is f32 MFMA with the fast tanh of the 2x64 tile kernel: results agree with the
 * per-step path to float32 rounding, not bit for bit; the same call repeated, or a run split into calls, gives the same bits.  An engine
 * that was never told follows the environment variable MOBROB_EVAL_TILE256 (1: on), read per call; MOBROB_EVAL_PERSISTENT=0 forces the
 * per-step path whatever is set here.  MOBROB_ERR_INVALID (naming tile256) on an engine that is not fused 2x256 tanh. */
int mobrob_ppo_set_eval_tile256(mobrob_ppo_engine_t* e, int32_t on);

/* The same kernel for calls WITH hazards, static or moving (the *_hazards and *_hazard_frames entry points).  A switch of its own,
 * OFF unless told: such a call runs as one launch and returns 1 only when tile256 is in force (mobrob_ppo_set_eval_tile256 or
 * MOBROB_EVAL_TILE256) AND this switch is (told here, or MOBROB_EVAL_TILE256_WIDE=1 for engines never told, read per call),
 * MOBROB_EVAL_PERSISTENT is not 0, and the task's shared scene fits the LDS left beside the actor (13 424 bytes: every shared hazard
 * scene fits; per-robot scenes are read from global memory).  Served: mobrob_ppo_evaluate_goal_env and mobrob_ppo_follow_waypoints
 * with static or moving hazards, resumed runs with moving hazards, scheduled runs with static hazards.  NOT served, whatever is set
 * here: calls with walls (observational or solid) or teams, resumed runs with static hazards, scheduled runs with moving hazards
 *  -- they run the per-step path as before and return 0; none is refused.  The hazard records are the bits the
 * per-step path gives for the same positions; positions agree with it to float32 rounding, as for the non-wide tasks.
 * MOBROB_ERR_INVALID (naming tile256) on a null engine and on an engine that is not fused 2x256 tanh. */
int mobrob_ppo_set_eval_tile256_wide(mobrob_ppo_engine_t* e, int32_t on);

/* train/explained_variance as SB3's PPO.train logs it (stable_baselines3 2.0.0 ppo.py: explained_variance(rollout_buffer.values.flatten(),
 * rollout_buffer.returns.flatten()) = 1 - Var[returns - values] / Var[returns], NaN when the returns do not vary), over the rollout
 * in the buffer; reached from the reference through PPOCtrl.learn (src/mobrob/rl_control/ppo.py:73-74) with verbose / tensorboard_log
 * (ppo.py:52-56).  Synchronises the engine's stream. */
int mobrob_ppo_explained_variance(mobrob_ppo_engine_t* e, double* out);

/* GAE on the buffers as they are (after write_buffer of rewards/values/episode_starts/
 * last_values/last_dones): RolloutBuffer.compute_returns_and_advantage in isolation. */
int mobrob_ppo_compute_gae(mobrob_ppo_engine_t* e);

/* Feistel permutation used when perm == NULL (bit-exact vs oracle/ppo_oracle.py:feistel_permutation) */
int mobrob_ppo_feistel_permutation(mobrob_ppo_engine_t* e, int64_t n, uint64_t key, int64_t* out);

/* ---- kernel timing with HIP events on the engine's stream (bench.py roofline) ---------------- */
enum {
  MOBROB_K_ACT = 0,          /* rollout policy/value forward + sample                           */
  MOBROB_K_GAE = 1,          /* GAE(lambda) scan                                                */
  MOBROB_K_TRAIN_GRAD = 2,   /* minibatch forward + loss + backward (dominant kernel)           */
  MOBROB_K_APPLY = 3,        /* grad-norm + clip + Adam                                         */
  MOBROB_K_ENV = 4,          /* synthetic env source (+ time-limit bootstrap)                   */
  MOBROB_K_GRAD_REDUCE = 5,  /* deterministic reduction of the per-workgroup gradient slabs     */
  MOBROB_K_ALLREDUCE = 6,    /* data parallel: the all-reduces of train_dp (gradient + statistics) */
  MOBROB_K_COUNT = 7
};
/* on: 0 = off, 1 = bracket every phase with HIP events, otherwise a mask with bit (MOBROB_K_x + 1) set for each phase
 * to bracket.  An event pair costs a few microseconds of GPU time per launch: bracketing all four launches of an
 * optimizer step slows the headline shape by 3.7 %, the dominant kernel alone by under 1 %. */
int mobrob_ppo_profile_enable(mobrob_ppo_engine_t* e, int32_t on);
/* accumulated since enable: total milliseconds and launch-group count per id */
int mobrob_ppo_profile_read(mobrob_ppo_engine_t* e, double* ms /*[K_COUNT]*/, int64_t* calls /*[K_COUNT]*/);

#ifdef __cplusplus
}
#endif
#endif /* MOBROB_PPO_H */
