// Hazard costs of the goal environment (mobrob_ppo_evaluate_goal_env_hazards / mobrob_ppo_follow_waypoints_hazards): the
// reference Engine's `constrain_hazards` rule added to a task, without changing anything the task computes.
//
// The rule, stated once in array form in mobrob_amd/envs/goal_rules.py (hazard_cost): after every env step, at the robot's new
// position p (before any reset), with hazards h = (x, y, r) of the robot's scene, coefficient c and the indicator flag,
//   d_h = |p_xy - h_xy|  (x and y only, every robot: hazards are vertical cylinders)
//   cost = sum over d_h <= r_h of c (r_h - d_h);  indicator: cost = (cost > 0)
//   clearance = min_h (d_h - r_h)  (+inf without hazards)
// A hazard on whose boundary the robot stands contributes exactly 0.  The cost never changes dynamics, reward or episodes.
//
// HazardTask<Base> wraps a task of kernels_eval.h (EvalTask, FollowTask): its Robot adds the accumulators, its step runs
// Base::step and then the check at the post-step position, its finish / load / store keep hazard_out.  The sums run in float
// over four partial sums (hazards h = q, q + 4, ... for q = 0..3), combined as (p0 + p1) + (p2 + p3): the tile kernel computes
// the partial sums on four lanes per robot, the per-step path in one thread, and both give the same bits for the same position.
#pragma once
#include "kernels_follow.h"

namespace mobrob {

constexpr int kHazardMax = 1024;       // hazards per scene at most (a shared scene fits in 12 KB of LDS)
constexpr int kHazardTraceExtra = 2;   // trace columns after the task's flags: cost, clearance

template <class BaseArgs>
struct HazardArgs {
  BaseArgs b;              // the wrapped task's arguments
  const float* hz;         // [S][M][3] x, y, radius
  const int* nhz;          // [S] hazards of each scene (<= M)
  const int* scene;        // [N] scene of each robot, or null (S == 1)
  int M;                   // row stride of hz
  float coef;              // hazards_cost
  int indicator;           // constrain_indicator
  double* hazard_out;      // [N][4] cost sum, violation steps, first violation (-1), min clearance; per-step path: live state
  double* ep_cost;         // [N][maxq] cost of each recorded episode, or null (evaluate only)
  double* ep_acc;          // [N] cost of the running episode (per-step path)
};

// one quarter's partial cost / clearance: hazards q, q + 4, ... of the scene `h` (n of them) at (px, py)
__device__ __forceinline__ void hazard_partial(const float* h, int n, int q, float px, float py, float& cost, float& clear) {
  cost = 0.f;
  clear = __builtin_inff();
  for (int i = q; i < n; i += 4) {
    const float dx = px - h[3 * i], dy = py - h[3 * i + 1], r = h[3 * i + 2];
    const float d = __fsqrt_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)));   // correctly rounded, no contraction
    if (d <= r) cost = __fadd_rn(cost, __fsub_rn(r, d));
    clear = fminf(clear, __fsub_rn(d, r));
  }
}

// the combined step cost from the four partial (unscaled) sums: coefficient and indicator applied once
__device__ __forceinline__ float hazard_combine(float p0, float p1, float p2, float p3, float coef, int indicator) {
  const float s = __fmul_rn(coef, __fadd_rn(__fadd_rn(p0, p1), __fadd_rn(p2, p3)));
  return indicator ? (s > 0.f ? 1.f : 0.f) : s;
}

template <class Base>
struct HazardTask {
  using Args = HazardArgs<typename Base::Args>;
  struct Robot {
    typename Base::Robot b;
    double cost_sum, ep_cost;
    int viol, first;
    float min_clear;
  };
  static constexpr bool kWide = true;   // k_goal64_tile: the check runs on all 64 lanes (step_lane + after_step below)
  static constexpr bool kResume = Base::kResume;   // a resumable base: accumulators continue from hazard_out, global steps
  static constexpr bool kFrames = false;           // one scene for the whole run (FrameHazardTask below: a frame per step)
  static __device__ __forceinline__ int step0(const Args& h) { return task_step0<Base>(h.b); }

  static __host__ __device__ __forceinline__ const EvalArgs& eval(const Args& h) { return Base::eval(h.b); }
  // LDS of k_goal64_tile beyond LayEval64::END: [16][2] post-step positions, then a shared scene
  static size_t tile_lds_bytes(const Args& h) { return (size_t)(32 + (h.scene ? 0 : 3 * h.M)) * sizeof(float); }

  // F, f (here and below): frames per scene and the frame in force (FrameHazardTask); a static scene is its only frame
  static __device__ __forceinline__ const float* scene_of(const Args& h, int n, int& count, int F = 1, int f = 0) {
    const int s = h.scene ? h.scene[n] : 0;
    count = h.nhz[s];
    return h.hz + ((size_t)s * F + f) * h.M * 3;
  }

  // the step's cost / clearance -> accumulators, episode record, trace columns.  e0: the base's episodes before the step.
  static __device__ __forceinline__ void account(const Args& h, int n, int t, Robot& R, int e0, float cost, float clear) {
    R.cost_sum += (double)cost;
    R.ep_cost += (double)cost;
    if (cost > 0.f) {
      R.viol += 1;
      if (R.first < 0) R.first = task_step0<Base>(h.b) + t + 1;
    }
    R.min_clear = fminf(R.min_clear, clear);
    if (Base::episodes(R.b) != e0) {   // the step ended an episode: its cost includes this step's
      if (h.ep_cost && Base::recorded(R.b, e0)) h.ep_cost[(size_t)n * eval(h).maxq + e0] = R.ep_cost;
      R.ep_cost = 0.0;
    }
    const EvalArgs& a = eval(h);
    if (a.trace && n < a.trace_robots && t < a.trace_steps) {
      float* f = a.trace + ((size_t)t * a.trace_robots + n) * eval_trace_width<kHazardTraceExtra>(a) + eval_trace_width(a);
      f[0] = cost; f[1] = clear;
    }
  }

  static __device__ __forceinline__ void start(GoalState& g, Robot& R, const Args& h, int n) {
    Base::start(g, R.b, h.b, n);
    R.cost_sum = 0.0; R.ep_cost = 0.0; R.viol = 0; R.first = -1; R.min_clear = __builtin_inff();
    if constexpr (kResume) hazard_load(h, n, R);   // the run's accumulators so far
  }
  static __device__ __forceinline__ bool active(const Args& h, const Robot& R) { return Base::active(h.b, R.b); }
  static __device__ __forceinline__ int steps(const Robot& R) { return Base::steps(R.b); }   // for a wrapping task (kernels_team.h)

  // the whole step in one thread (per-step path): the four partial sums in turn
  static __device__ __forceinline__ bool step(GoalState& g, Robot& R, const Args& h, int n, int t, const float* act,
                                              const float* obs_row, int F = 1, int f = 0) {
    float post[2];
    const int e0 = Base::episodes(R.b);
    const bool going = Base::template step<kHazardTraceExtra>(g, R.b, h.b, n, t, act, obs_row, post);
    int m;
    const float* hs = scene_of(h, n, m, F, f);
    float c[4], cl[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) hazard_partial(hs, m, q, post[0], post[1], c[q], cl[q]);
    account(h, n, t, R, e0, hazard_combine(c[0], c[1], c[2], c[3], h.coef, h.indicator),
            fminf(fminf(cl[0], cl[1]), fminf(cl[2], cl[3])));
    return going;
  }

  // ---- k_goal64_tile: Base::step on the robot's lane (post-step position -> LDS), then after_step on all 64 lanes ----
  // hz_lds: the shared scene (scene == null) staged in LDS by `stage`; xy: [16][2] post-step positions in LDS
  static __device__ __forceinline__ void stage(const Args& h, float* hz_lds, int lane, int f = 0) {
    if (!h.scene)
      for (int i = lane; i < 3 * h.nhz[0]; i += 64) hz_lds[i] = h.hz[(size_t)f * h.M * 3 + i];
  }
  static __device__ __forceinline__ bool step_lane(GoalState& g, Robot& R, const Args& h, int n, int t, const float* act,
                                                   const float* obs_row, float* xy, int& e0) {
    e0 = Base::episodes(R.b);
    return Base::template step<kHazardTraceExtra>(g, R.b, h.b, n, t, act, obs_row, xy);
  }
  // every lane: quarter q = lane >> 4 of robot r16 = lane & 15 (if it stepped); lane r16 < 16 accounts the combined result
  static __device__ __forceinline__ void after_step(const Args& h, Robot& R, int n, int t, int lane, bool stepped, int e0,
                                                    const float* xy, const float* hz_lds, int F = 1, int f = 0) {
    const int r16 = lane & 15, q = lane >> 4;
    float c = 0.f, cl = __builtin_inff();
    if (stepped) {
      int m;
      const float* hs = scene_of(h, n, m, F, f);
      hazard_partial(h.scene ? hs : hz_lds, m, q, xy[2 * r16], xy[2 * r16 + 1], c, cl);
    }
    // lanes r16, r16 + 16, r16 + 32, r16 + 48 hold quarters 0..3: (p0 + p1) + (p2 + p3), the same sum on every one of them
    const float c01 = __fadd_rn(c, __shfl_xor(c, 16, 64));
    const float cs = __fadd_rn(c01, __shfl_xor(c01, 32, 64));
    const float cl01 = fminf(cl, __shfl_xor(cl, 16, 64));
    const float cls = fminf(cl01, __shfl_xor(cl01, 32, 64));
    if (lane < 16 && stepped) {
      const float cost = h.indicator ? (__fmul_rn(h.coef, cs) > 0.f ? 1.f : 0.f) : __fmul_rn(h.coef, cs);
      account(h, n, t, R, e0, cost, cls);
    }
  }

  static __device__ __forceinline__ void hazard_store(const Args& h, int n, const Robot& R) {
    double* o = h.hazard_out + (size_t)n * 4;
    o[0] = R.cost_sum; o[1] = (double)R.viol; o[2] = (double)R.first;
    o[3] = Base::steps(R.b) > 0 ? (double)R.min_clear : __longlong_as_double(0x7FF8000000000000ll);   // NaN: no step run
  }
  static __device__ __forceinline__ void finish(const Args& h, int n, const Robot& R, const GoalState& g) {
    Base::finish(h.b, n, R.b, g);
    hazard_store(h, n, R);
  }
  // R's accumulators from hazard_out (R.b loaded)
  static __device__ __forceinline__ void hazard_load(const Args& h, int n, Robot& R) {
    const double* o = h.hazard_out + (size_t)n * 4;
    R.cost_sum = o[0]; R.viol = (int)o[1]; R.first = (int)o[2];
    R.min_clear = Base::steps(R.b) > 0 ? (float)o[3] : __builtin_inff();
  }
  static __device__ __forceinline__ Robot load(const Args& h, int n) {
    Robot R;
    R.b = Base::load(h.b, n);
    hazard_load(h, n, R);
    R.ep_cost = h.ep_acc[n];
    return R;
  }
  static __device__ __forceinline__ void store(const Args& h, int n, const Robot& R) {
    Base::store(h.b, n, R.b);
    hazard_store(h, n, R);
    h.ep_acc[n] = R.ep_cost;
  }
};

using HazardEvalTask = HazardTask<EvalTask>;
using HazardFollowTask = HazardTask<FollowTask>;

// ------------------------------------------------------------------------------------------------
// Moving hazards (mobrob_ppo_evaluate_goal_env_hazard_frames / mobrob_ppo_follow_waypoints_hazard_frames): every scene is F
// frames, hz [S][F][M][3], and the check after the step with global number g = task_step0 + t reads the frame
//   f(g) = min(g / frame_steps, F - 1)  (hold the last frame)   or, with loop,   f(g) = (g / frame_steps) % F
// (goal_rules.MovingHazards.frame_index).  Frames are piecewise constant: no interpolation, so the check at a frame is exactly
// the static task's, on the same lanes in the same order.  f depends on g alone, hence it is uniform over a wave.
// FrameHazardTask<Base> is HazardTask<Base> with that frame chosen per step: accumulators, trace columns, hazard_out, ep_cost
// are HazardTask's.  k_goal64_tile keeps ONE frame of a shared scene in LDS (tile_lds_bytes is HazardTask's) and restages it
// when f changes (kFrames); per-robot scenes and the per-step path read the frame from global memory.
// ------------------------------------------------------------------------------------------------
template <class BaseArgs>
struct FrameHazardArgs {
  HazardArgs<BaseArgs> h;  // h.hz: [S][F][M][3]; every other field as for the static task
  int F;                   // frames per scene, >= 1
  int frame_steps;         // steps per frame, >= 1
  int loop;                // after the last frame: 0 hold it, 1 start over
};

template <class Base>
struct FrameHazardTask {
  using H = HazardTask<Base>;
  using Args = FrameHazardArgs<typename Base::Args>;
  using Robot = typename H::Robot;
  static constexpr bool kWide = true;
  static constexpr bool kResume = Base::kResume;
  static constexpr bool kFrames = true;   // k_goal64_tile: restage the shared scene whenever frame(g0 + t) changes
  static __device__ __forceinline__ int step0(const Args& a) { return H::step0(a.h); }
  static __host__ __device__ __forceinline__ const EvalArgs& eval(const Args& a) { return H::eval(a.h); }
  static size_t tile_lds_bytes(const Args& a) { return H::tile_lds_bytes(a.h); }   // one frame resident

  // the frame in force at the check after the step with global number g
  static __device__ __forceinline__ int frame(const Args& a, int g) {
    const int k = g / a.frame_steps;
    return a.loop ? k % a.F : min(k, a.F - 1);
  }
  static __device__ __forceinline__ int frame_at(const Args& a, int t) { return frame(a, task_step0<Base>(a.h.b) + t); }

  static __device__ __forceinline__ void start(GoalState& g, Robot& R, const Args& a, int n) { H::start(g, R, a.h, n); }
  static __device__ __forceinline__ bool active(const Args& a, const Robot& R) { return H::active(a.h, R); }
  static __device__ __forceinline__ int steps(const Robot& R) { return H::steps(R); }
  static __device__ __forceinline__ bool step(GoalState& g, Robot& R, const Args& a, int n, int t, const float* act,
                                              const float* obs_row) {
    return H::step(g, R, a.h, n, t, act, obs_row, a.F, frame_at(a, t));
  }
  // ---- k_goal64_tile: `stage` before the loop = the first frame used; stage_frame when the frame changes ----
  static __device__ __forceinline__ void stage_frame(const Args& a, float* hz_lds, int lane, int f) { H::stage(a.h, hz_lds, lane, f); }
  static __device__ __forceinline__ void stage(const Args& a, float* hz_lds, int lane) { stage_frame(a, hz_lds, lane, frame_at(a, 0)); }
  static __device__ __forceinline__ bool step_lane(GoalState& g, Robot& R, const Args& a, int n, int t, const float* act,
                                                   const float* obs_row, float* xy, int& e0) {
    return H::step_lane(g, R, a.h, n, t, act, obs_row, xy, e0);
  }
  static __device__ __forceinline__ void after_step(const Args& a, Robot& R, int n, int t, int lane, bool stepped, int e0,
                                                    const float* xy, const float* hz_lds) {
    H::after_step(a.h, R, n, t, lane, stepped, e0, xy, hz_lds, a.F, frame_at(a, t));
  }
  static __device__ __forceinline__ void finish(const Args& a, int n, const Robot& R, const GoalState& g) { H::finish(a.h, n, R, g); }
  static __device__ __forceinline__ Robot load(const Args& a, int n) { return H::load(a.h, n); }
  static __device__ __forceinline__ void store(const Args& a, int n, const Robot& R) { H::store(a.h, n, R); }
};

// robot_out and the path records of robots that finished early (per-step path; hazard_out is current after every step)
__global__ __launch_bounds__(256) void k_hazard_follow_fin(HazardArgs<FollowArgs> h) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= h.b.e.N) return;
  follow_finish(h.b, n, follow_robot_load(h.b, n), goal_load(h.b.e.st + (size_t)n * kGoalStateFloats));
}

}  // namespace mobrob
