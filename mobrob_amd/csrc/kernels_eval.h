// Batched on-device policy evaluation of the goal environment (mobrob_ppo_evaluate_goal_env): SB3's evaluate_policy and the
// protocol of the reference examples/control.py:36-46 for thousands of robots at once.
//
// The environment rules are the device functions of kernels_env.h, used unchanged (goal_advance, goal_reset, goal_features), so an
// evaluated robot steps exactly like a training environment.  Randomness comes from streams of the evaluation's own (new stream
// constants, keyed by the caller's seed; counter = (robot, component, step)): nothing here reads or advances a training counter.
//
//
// What runs on the goal env under the policy is a TASK: a small type that names its kernel argument struct (Args), its per-robot
// accumulators (Robot) and supplies start / active / step / finish (+ load / store of Robot for the per-step path).  EvalTask is
// below; FollowTask (waypoint following) is in kernels_follow.h.  The kernels exist once, for every task:
//
//   k_goal_task_init<Task>   start state of every robot, first observation                     (per-step path, one launch)
//   k_goal_task_step<Task>   clip / sample, the task's env step, next observation              (per-step path, one launch per step;
//                            the actor mean comes from the engine's forward() into the evaluation's own buffers)
//   k_goal64_tile<DP, Task>  the whole run in one launch for 2x64 tanh actors: one wave per 16-robot tile, the actor in LDS,
//                            the forward on the f32 16x16x4 MFMA, the tile's state in registers / LDS through the step loop
#pragma once
#include <type_traits>
#include "kernels_fused.h"
#include "kernels_env.h"

namespace mobrob {

constexpr uint32_t kStreamEvalObs = 0x45564F31u;   // 'EVO1' observation noise
constexpr uint32_t kStreamEvalAct = 0x45564131u;   // 'EVA1' action noise (deterministic = 0)
constexpr uint64_t kEvalKeyMix = 0x9E6C63D0676A9A99ull;   // the reset stream's key (goal_reset's constant is the env's own)
constexpr int kEvalTraceFlags = 4;                  // reward, reached, term, tr

struct EvalArgs {
  GoalEnvParams p;            // time_limit 0 (none) already mapped to INT_MAX
  int N, D, Dp, A, Ap;
  int episodes, deterministic, maxq;
  int max_steps;              // step cap of the run
  float lo, hi;
  uint32_t k0, k1;            // Philox key of the evaluation streams
  const int* quota;           // [N] episodes to record (and, with episodes > 0, to finish before idling)
  const float* log_std;       // [A] (deterministic = 0)
  double* robot_out;          // [N][4] reward sum, steps run, episodes finished, goals reached
  double* ep_out;             // [N][maxq][3] return, length, success
  float* trace;               // [trace_steps][trace_robots][9 + D + A + 4] or null
  int trace_robots, trace_steps;
  // per-step path state
  float* st;                  // [N][kGoalStateFloats]
  double* ep_ret;             // [N] float64 return of the running episode
  float* obs;                 // [N][Dp] observation the next step acts on
  float* mu;                  // [N][Ap] actor mean of those observations (written by the engine's forward())
};

// XT: extra columns a wrapping task appends to every row (kernels_hazard.h)
template <int XT = 0>
__device__ __forceinline__ int eval_trace_width(const EvalArgs& a) { return 9 + a.D + a.A + kEvalTraceFlags + XT; }

// observation chunk c (features 4c .. 4c + 3) of state g, seen before step `step`
__device__ __forceinline__ f32x4 eval_features(const GoalState& g, const EvalArgs& a, int n, int c, uint32_t step) {
  float z[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.p.noise != 0.f) box_muller4(philox4x32_10((uint32_t)n, (uint32_t)c, step, kStreamEvalObs, a.k0, a.k1), z);
  return goal_features(g, a.p.P, a.D, c, z, a.p.noise);
}

// the observation of robot n before step `step` -> a.obs (per-step path)
__device__ __forceinline__ void eval_obs_store(const GoalState& g, const EvalArgs& a, int n, uint32_t step) {
  for (int c = 0; c < a.Dp / 4; ++c) reinterpret_cast<f32x4*>(a.obs)[(size_t)n * (a.Dp / 4) + c] = eval_features(g, a, n, c, step);
}

// the trace row of robot n at step t: state before the step, observation, action.  Returns the row's four task-specific flag
// floats for the caller to fill after the step, or null when (n, t) is not traced.
template <int XT = 0>
__device__ __forceinline__ float* eval_trace_row(const GoalState& g, const EvalArgs& a, int n, int t, const float* act,
                                                 const float* obs_row) {
  if (!(a.trace && n < a.trace_robots && t < a.trace_steps)) return nullptr;
  float* tr_row = a.trace + ((size_t)t * a.trace_robots + n) * eval_trace_width<XT>(a);
#pragma unroll
  for (int j = 0; j < 3; ++j) { tr_row[j] = g.pos[j]; tr_row[3 + j] = g.vel[j]; tr_row[6 + j] = g.goal[j]; }
  for (int f = 0; f < a.D; ++f) tr_row[9 + f] = obs_row[f];
  for (int k = 0; k < a.A; ++k) tr_row[9 + a.D + k] = act[k];
  return tr_row + 9 + a.D + a.A;
}

__device__ __forceinline__ void eval_reset0(GoalState& g, const EvalArgs& a, int n) {
  g = GoalState{};
  goal_reset(g, a.p, false, (uint32_t)n, 0xFFFFFFFFu, a.k0, a.k1);
}

// action k of robot n at step t from the actor mean m: clip(mean), or clip(mean + exp(log_std) z) with z from the eval stream
__device__ __forceinline__ void eval_actions(const EvalArgs& a, int n, int t, const float* m, float* act) {
  for (int g4 = 0; 4 * g4 < a.A; ++g4) {
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (!a.deterministic) box_muller4(philox4x32_10((uint32_t)n, (uint32_t)g4, (uint32_t)t, kStreamEvalAct, a.k0, a.k1), z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = 4 * g4 + j;
      if (k < a.A) {
        float v = m[k];
        if (!a.deterministic) v = __fmaf_rn(expf(a.log_std[k]), z[j], v);
        act[k] = fminf(fmaxf(v, a.lo), a.hi);
      }
    }
  }
}

// per-robot accounting of one evaluation
struct EvalRobot {
  double ret_sum, ep_ret;
  int steps, eps, goals, quota;
};

// one step of robot n at step t: trace (state before the step, observation, action), env.step, float64 accounting, episode
// record, reset.  Returns whether the robot is still active afterwards.  obs_row: the D observation features it acted on;
// post: if not null, receives x, y after the env step and before any reset.
template <int XT = 0>
__device__ __forceinline__ bool eval_env_step(GoalState& g, EvalRobot& R, const EvalArgs& a, int n, int t, const float* act,
                                              const float* obs_row, float* post = nullptr) {
  float* f = eval_trace_row<XT>(g, a, n, t, act, obs_row);
  const GoalOutcome o = goal_advance(g, a.p, act, a.A);
  if (post) { post[0] = g.pos[0]; post[1] = g.pos[1]; }
  R.steps += 1;
  R.ret_sum += (double)o.reward;
  R.ep_ret += (double)o.reward;
  if (o.reached) R.goals += 1;
  if (f) {
    f[0] = o.reward; f[1] = o.reached ? 1.f : 0.f; f[2] = o.term ? 1.f : 0.f; f[3] = o.tr ? 1.f : 0.f;
  }
  if (o.done) {
    if (R.eps < R.quota) {
      double* r = a.ep_out + ((size_t)n * a.maxq + R.eps) * 3;
      r[0] = R.ep_ret; r[1] = (double)g.ep_len; r[2] = o.reached ? 1.0 : 0.0;
    }
    R.eps += 1;
    R.ep_ret = 0.0;
    goal_reset(g, a.p, o.reached, (uint32_t)n, (uint32_t)t, a.k0, a.k1);
  }
  return a.episodes == 0 || R.eps < R.quota;
}

__device__ __forceinline__ void eval_robot_out(const EvalArgs& a, int n, const EvalRobot& R) {
  double* o = a.robot_out + (size_t)n * 4;
  o[0] = R.ret_sum; o[1] = (double)R.steps; o[2] = (double)R.eps; o[3] = (double)R.goals;
}

// the evaluation as a task: fresh reset and quota, eval_env_step until the quota is met, robot_out.  Between the launches of the
// per-step path the accumulators live in robot_out / ep_ret.
struct EvalTask {
  using Args = EvalArgs;
  using Robot = EvalRobot;
  static __host__ __device__ __forceinline__ const EvalArgs& eval(const Args& a) { return a; }
  static __device__ __forceinline__ void start(GoalState& g, Robot& R, const Args& a, int n) {
    eval_reset0(g, a, n);
    R = Robot{0.0, 0.0, 0, 0, 0, a.quota[n]};
  }
  static constexpr bool kWide = false;   // k_goal64_tile: step runs on the robot's lane only
  static constexpr bool kResume = false;   // the launch's step 0 is the streams' step 0 (task_step0 below)
  static constexpr bool kFrames = false;   // k_goal64_tile: nothing to restage between steps (kernels_hazard.h: FrameHazardTask)
  static __device__ __forceinline__ bool active(const Args& a, const Robot& R) { return a.episodes == 0 || R.eps < R.quota; }
  // XT / post: for a wrapping task (kernels_hazard.h): trace row width + XT, the post-step x, y
  template <int XT = 0>
  static __device__ __forceinline__ bool step(GoalState& g, Robot& R, const Args& a, int n, int t, const float* act,
                                              const float* obs_row, float* post = nullptr) {
    return eval_env_step<XT>(g, R, a, n, t, act, obs_row, post);
  }
  static __device__ __forceinline__ int episodes(const Robot& R) { return R.eps; }
  static __device__ __forceinline__ int steps(const Robot& R) { return R.steps; }
  static __device__ __forceinline__ bool recorded(const Robot& R, int e) { return e < R.quota; }
  static __device__ __forceinline__ void finish(const Args& a, int n, const Robot& R, const GoalState&) { eval_robot_out(a, n, R); }
  static __device__ __forceinline__ Robot load(const Args& a, int n) {
    const double* o = a.robot_out + (size_t)n * 4;
    return Robot{o[0], a.ep_ret[n], (int)o[1], (int)o[2], (int)o[3], a.quota[n]};
  }
  static __device__ __forceinline__ void store(const Args& a, int n, const Robot& R) {
    a.ep_ret[n] = R.ep_ret;
    eval_robot_out(a, n, R);
  }
};

// the global step of the launch's step 0: the observation and action streams are keyed by (robot, task_step0 + t).  A task of a
// run that spans several calls (kResume: ResumeFollowTask, kernels_follow.h) names it; for every other task it is the constant 0
template <class Task>
__device__ __forceinline__ int task_step0(const typename Task::Args& args) {
  if constexpr (Task::kResume) return Task::step0(args);
  else return 0;
}

// a task that checks robots against their team-mates (kernels_team.h: TeamTask names its TeamBase): k_goal64_tile seeds the xy
// block with every robot's carried position (Task::place), the per-step path launches k_team_step after every step kernel
template <class Task, class = void>
constexpr bool task_teams = false;
template <class Task>
constexpr bool task_teams<Task, std::void_t<typename Task::TeamBase>> = true;

// ------------------------------------------------------------------------------------------------
// per-step path: robot state in st, the task's accumulators wherever Task::store keeps them between launches
// ------------------------------------------------------------------------------------------------
template <class Task>
__global__ __launch_bounds__(256) void k_goal_task_init(typename Task::Args args) {
  const EvalArgs& a = Task::eval(args);
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  GoalState g;
  typename Task::Robot R;
  Task::start(g, R, args, n);
  goal_store(a.st + (size_t)n * kGoalStateFloats, g);
  Task::store(args, n, R);
  eval_obs_store(g, a, n, (uint32_t)task_step0<Task>(args));
}

template <class Task>
__global__ __launch_bounds__(256) void k_goal_task_step(typename Task::Args args, int t) {
  const EvalArgs& a = Task::eval(args);
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  typename Task::Robot R = Task::load(args, n);
  if (!Task::active(args, R)) return;   // idles: quota met / last waypoint reached
  GoalState g = goal_load(a.st + (size_t)n * kGoalStateFloats);
  float* act = &lds[threadIdx.x * 33];   // [256][33]: the thread's clipped actions (LDS, not a dynamically indexed register array)
  const int g0 = task_step0<Task>(args);
  eval_actions(a, n, g0 + t, a.mu + (size_t)n * a.Ap, act);
  (void)Task::step(g, R, args, n, t, act, a.obs + (size_t)n * a.Dp);
  goal_store(a.st + (size_t)n * kGoalStateFloats, g);
  Task::store(args, n, R);
  eval_obs_store(g, a, n, (uint32_t)(g0 + t) + 1u);
}

// the task's finish for every robot, from what the last step stored (a resumable task: robot_out, carried state, status, path)
template <class Task>
__global__ __launch_bounds__(256) void k_goal_task_fin(typename Task::Args args) {
  const EvalArgs& a = Task::eval(args);
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  Task::finish(args, n, Task::load(args, n), goal_load(a.st + (size_t)n * kGoalStateFloats));
}

// ------------------------------------------------------------------------------------------------
// k_goal64_tile<DP, Task>: the persistent path for 2x64 tanh actors (every reference config).
//
// One workgroup = ONE wave = one tile of 16 robots, so every barrier of the step loop is a single-wave s_barrier and the exit test
// (a ballot of the tile's active robots) is uniform across the workgroup.  The actor (~40 KB at DP = 64) is copied from the flat
// parameter vector into LDS once, in the B-fragment order of v_mfma_f32_16x16x4_f32 (lane l of k-step s holds W[col + (l & 15)]
// [4 s + (l >> 4)]: one conflict-free ds_read_b32 per MFMA).  Per step: observation tile -> LDS (goal_features), layer 1 (DP / 4
// k-steps x 4 independent 16-column accumulators), layer 2 (16 x 4), head (16 x 1 or 2), each a chain of 40-cycle dependent MFMAs
// with 4 (2) chains in flight; the env phase (clip / sample, the task's step: goal_advance, float64 accounting, records) runs on
// the tile's 16 lanes, the robots' GoalState and accumulators stay in those lanes' registers for the whole launch.  The loop ends
// at max_steps or when the ballot finds none of the tile's robots active.
// ------------------------------------------------------------------------------------------------
struct Eval64Net {
  const float *W1, *b1, *W2, *b2, *W3, *b3;   // canonical SB3 tensors (pi.0, pi.2, action_net), row-major [out][in]
};
template <int DP>
struct LayEval64 {
  static constexpr int KS1 = DP / 4, LDX = DP + 4, LDH = 68, LDM = 36;
  static constexpr int W1 = 0;                    // [4 col blocks][KS1][64 lanes]
  static constexpr int W2 = W1 + 4 * KS1 * 64;    // [4][16][64]
  static constexpr int W3 = W2 + 4 * 16 * 64;     // [2][16][64]
  static constexpr int B1 = W3 + 2 * 16 * 64;     // [64]
  static constexpr int B2 = B1 + 64;              // [64]
  static constexpr int B3 = B2 + 64;              // [32]
  static constexpr int X = B3 + 32;               // [16][LDX]
  static constexpr int H1 = X + 16 * LDX;         // [16][LDH]
  static constexpr int H2 = H1 + 16 * LDH;        // [16][LDH]
  static constexpr int MU = H2 + 16 * LDH;        // [16][LDM]
  static constexpr int ST = MU + 16 * LDM;        // [16][12] robot state for the observation phase
  static constexpr int END = ST + 16 * 12;
};
inline size_t eval64_lds_bytes(int Dp) {
  switch (Dp) {
    case 16: return LayEval64<16>::END * sizeof(float);
    case 32: return LayEval64<32>::END * sizeof(float);
    case 48: return LayEval64<48>::END * sizeof(float);
    default: return LayEval64<64>::END * sizeof(float);
  }
}

__device__ __forceinline__ void eval64_state_lds(float* s, const GoalState& g) {
#pragma unroll
  for (int j = 0; j < 3; ++j) { s[j] = g.pos[j]; s[3 + j] = g.vel[j]; s[6 + j] = g.goal[j]; }
}

// the actor -> LDS in fragment order (zero beyond D / A), its biases, and a zeroed observation tile
template <int DP>
__device__ __forceinline__ void eval64_load_actor(const Eval64Net& W, int D, int A, int lane) {
  using L = LayEval64<DP>;
  constexpr int KS1 = L::KS1;
  for (int i = lane; i < 4 * KS1 * 64; i += 64) {
    const int l = i & 63, ks = (i >> 6) % KS1, cb = (i >> 6) / KS1;
    const int k = 4 * ks + (l >> 4);
    lds[L::W1 + i] = k < D ? W.W1[(size_t)(16 * cb + (l & 15)) * D + k] : 0.f;
  }
  for (int i = lane; i < 4 * 16 * 64; i += 64) {
    const int l = i & 63, ks = (i >> 6) & 15, cb = i >> 10;
    lds[L::W2 + i] = W.W2[(16 * cb + (l & 15)) * 64 + 4 * ks + (l >> 4)];
  }
  for (int i = lane; i < 2 * 16 * 64; i += 64) {
    const int l = i & 63, ks = (i >> 6) & 15, nb = i >> 10;
    const int col = 16 * nb + (l & 15);
    lds[L::W3 + i] = col < A ? W.W3[col * 64 + 4 * ks + (l >> 4)] : 0.f;
  }
  lds[L::B1 + lane] = W.b1[lane];
  lds[L::B2 + lane] = W.b2[lane];
  if (lane < 32) lds[L::B3 + lane] = lane < A ? W.b3[lane] : 0.f;
  for (int i = lane; i < 16 * L::LDX; i += 64) lds[L::X + i] = 0.f;
}

// one step of the tile's actor: observation tile (goal_features of the robots' LDS state rows + the evaluation's noise, 64 lanes),
// layer 1, layer 2, head; the 16 mean rows land in L::MU.  Every phase ends with the (single-wave) barrier.
template <int DP>
__device__ __forceinline__ void eval64_actor_step(const EvalArgs& a, int row0, int t, int lane, bool wide_head) {
  using L = LayEval64<DP>;
  constexpr int KS1 = L::KS1, per = DP / 4;
  const int r16 = lane & 15, q = lane >> 4;
  // ---- observation tile: lane (r16, q) builds chunks q, q + 4, ... of robot r16 ----
  if (row0 + r16 < a.N) {
    GoalState gs{};
    const float* s = &lds[L::ST + 12 * r16];
#pragma unroll
    for (int j = 0; j < 3; ++j) { gs.pos[j] = s[j]; gs.vel[j] = s[3 + j]; gs.goal[j] = s[6 + j]; }
    for (int c = q; c < per; c += 4)
      *reinterpret_cast<f32x4*>(&lds[L::X + r16 * L::LDX + 4 * c]) = eval_features(gs, a, row0 + r16, c, (uint32_t)t);
  }
  __syncthreads();
  // ---- layer 1: h1 = tanh(W1 x + b1), four 16-column accumulators ----
  {
    f32x4 c[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) { const float b = lds[L::B1 + 16 * cb + r16]; c[cb] = f32x4{b, b, b, b}; }
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
      const float x = lds[L::X + r16 * L::LDX + 4 * ks + q];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) c[cb] = MFMA16(x, lds[L::W1 + (cb * KS1 + ks) * 64 + lane], c[cb]);
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int i = 0; i < 4; ++i) lds[L::H1 + (4 * q + i) * L::LDH + 16 * cb + r16] = fast_tanh(c[cb][i]);
  }
  __syncthreads();
  // ---- layer 2 ----
  {
    f32x4 c[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) { const float b = lds[L::B2 + 16 * cb + r16]; c[cb] = f32x4{b, b, b, b}; }
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const float x = lds[L::H1 + r16 * L::LDH + 4 * ks + q];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) c[cb] = MFMA16(x, lds[L::W2 + (cb * 16 + ks) * 64 + lane], c[cb]);
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int i = 0; i < 4; ++i) lds[L::H2 + (4 * q + i) * L::LDH + 16 * cb + r16] = fast_tanh(c[cb][i]);
  }
  __syncthreads();
  // ---- head: mean = W3 h2 + b3 (one or two 16-column blocks) ----
  {
    const float b0 = lds[L::B3 + r16], b1 = lds[L::B3 + 16 + r16];
    f32x4 c0 = f32x4{b0, b0, b0, b0}, c1 = f32x4{b1, b1, b1, b1};
    if (wide_head) {
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        const float x = lds[L::H2 + r16 * L::LDH + 4 * ks + q];
        c0 = MFMA16(x, lds[L::W3 + ks * 64 + lane], c0);
        c1 = MFMA16(x, lds[L::W3 + (16 + ks) * 64 + lane], c1);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) c0 = MFMA16(lds[L::H2 + r16 * L::LDH + 4 * ks + q], lds[L::W3 + ks * 64 + lane], c0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      lds[L::MU + (4 * q + i) * L::LDM + r16] = c0[i];
      lds[L::MU + (4 * q + i) * L::LDM + 16 + r16] = c1[i];
    }
  }
  __syncthreads();
}

template <int DP, class Task>
__global__ __launch_bounds__(64) void k_goal64_tile(typename Task::Args args, Eval64Net W) {
  using L = LayEval64<DP>;
  const EvalArgs& a = Task::eval(args);
  const int lane = threadIdx.x;
  const int r16 = lane & 15;
  const int row0 = blockIdx.x * 16;
  eval64_load_actor<DP>(W, a.D, a.A, lane);
  if constexpr (Task::kWide) Task::stage(args, &lds[L::END + 32], lane);   // after [16][2] post-step positions at L::END
  // ---- start state of the tile's robots (lanes 0..15 own robot row0 + lane) ----
  const int n = row0 + r16;
  const bool mine = lane < 16 && n < a.N;
  GoalState g{};
  typename Task::Robot R{};
  bool active = false;
  if (mine) {
    Task::start(g, R, args, n);
    active = Task::active(args, R);
    eval64_state_lds(&lds[L::ST + 12 * r16], g);
    if constexpr (task_teams<Task>) Task::place(g, &lds[L::END + 2 * r16]);
  }
  __syncthreads();
  const bool wide_head = a.A > 16;
  const int g0 = task_step0<Task>(args);   // t: step of this launch (trace, path); g0 + t: step of the streams
  [[maybe_unused]] int staged = 0;         // kFrames: the frame of the shared scene resident in LDS (Task::stage: the first used)
  if constexpr (Task::kFrames) staged = Task::frame(args, g0);
  for (int t = 0; t < a.max_steps; ++t) {
    if (__ballot(active) == 0ull) break;   // one wave per workgroup: uniform
    if constexpr (Task::kFrames) {
      // a new frame (uniform: it depends on g0 + t alone) replaces the resident one before the env phase; the previous step's
      // reads ended at its closing barrier, and the actor step's barriers stand between these writes and after_step's reads
      const int f = Task::frame(args, g0 + t);
      if (f != staged) {
        Task::stage_frame(args, &lds[L::END + 32], lane, f);
        staged = f;
      }
    }
    eval64_actor_step<DP>(a, row0, g0 + t, lane, wide_head);
    if constexpr (Task::kWide) {
      // ---- env phase on the tile's 16 lanes, then the task's wide phase on all 64 (robot lane & 15 stepped: bit of `stepping`) ----
      const uint64_t stepping = __ballot(mine && active);
      int e0 = 0;
      if (mine && active) {
        float* act = &lds[L::MU + r16 * L::LDM];
        eval_actions(a, n, g0 + t, act, act);
        active = Task::step_lane(g, R, args, n, t, act, &lds[L::X + r16 * L::LDX], &lds[L::END + 2 * r16], e0);
        eval64_state_lds(&lds[L::ST + 12 * r16], g);
      }
      __syncthreads();
      Task::after_step(args, R, n, t, lane, (stepping >> r16) & 1ull, e0, &lds[L::END], &lds[L::END + 32]);
      __syncthreads();
    } else {
    // ---- env phase: the tile's 16 lanes ----
    if (mine && active) {
      float* act = &lds[L::MU + r16 * L::LDM];   // the mean row becomes the applied action in place
      eval_actions(a, n, g0 + t, act, act);
      active = Task::step(g, R, args, n, t, act, &lds[L::X + r16 * L::LDX]);
      eval64_state_lds(&lds[L::ST + 12 * r16], g);
    }
    __syncthreads();
    }
  }
  if (mine) Task::finish(args, n, R, g);
}

}  // namespace mobrob
