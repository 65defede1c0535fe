// Batched on-device waypoint following (mobrob_ppo_follow_waypoints): n independent robots of the goal environment, each driven by
// the current policy along its own sequence of goals (a planner's path) instead of goals drawn from the RNG.
//
// One robot, stated as the host loop of mobrob_amd/waypoints.py: start at `start` with zero velocity and goal wp[0]; every step
// acts on the observation, steps the env (goal_advance of kernels_env.h, unchanged: no time limit, no reset) and, if the robot is
// then inside the reach radius, records the arrival step (t + 1) and makes the next waypoint the goal in force (pose and velocity
// kept; goal_advance measures progress against the goal in force).  At most one waypoint advances per step; after the last one the
// robot idles.  Observation noise and sampled actions come from the evaluation's streams (kernels_eval.h), keyed by the seed.
//
// FollowTask plugs these rules into the task kernels of kernels_eval.h (k_goal_task_init / k_goal_task_step on the per-step path,
// k_goal64_tile for 2x64 tanh actors: the exit ballot is over the tile's unfinished robots).  One kernel is the task's own:
//
//   k_follow_goal_fin   robot_out and the path records of robots that finished early           (per-step path, one launch)
#pragma once
#include "kernels_eval.h"

namespace mobrob {

struct FollowArgs {
  EvalArgs e;          // env parameters (no time limit, terminate_on_goal 0), dims, streams, trace and per-step buffers;
                       // e.robot_out [N][4]: reward sum, steps run, waypoints reached, final distance to the waypoint in force
  int K;               // waypoint row stride
  int path_stride;     // e.max_steps is the run's step cap
  const float* start;  // [N][P]
  const float* wp;     // [N][K][P]
  const int* nwp;      // [N] waypoints of robot n (<= K)
  int* arrival;        // [N][K] arrival step of waypoint k (1-based), -1 = not reached (filled by the host before the launch)
  float* path;         // [max_steps / path_stride + 1][N][P]: position after r * path_stride steps, or null
};

struct FollowRobot {
  double ret_sum;
  int steps, k, nwp;   // steps run, waypoints reached (= index of the waypoint in force), waypoints of the robot
};

__device__ __forceinline__ void follow_set_goal(GoalState& g, const FollowArgs& f, int n, int k) {
  const float* w = f.wp + ((size_t)n * f.K + k) * f.e.p.P;
#pragma unroll
  for (int j = 0; j < 3; ++j) g.goal[j] = j < f.e.p.P ? w[j] : 0.f;
}

__device__ __forceinline__ void follow_path_store(const FollowArgs& f, int r, int n, const GoalState& g) {
  float* o = f.path + ((size_t)r * f.e.N + n) * f.e.p.P;
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (j < f.e.p.P) o[j] = g.pos[j];
}

// robot n at rest on `start`, goal wp[0] (a robot without waypoints keeps its start as goal: it runs no step); path record 0
__device__ __forceinline__ void follow_start(GoalState& g, FollowRobot& R, const FollowArgs& f, int n) {
  g = GoalState{};
  R = FollowRobot{0.0, 0, 0, f.nwp[n]};
  const float* s = f.start + (size_t)n * f.e.p.P;
#pragma unroll
  for (int j = 0; j < 3; ++j) g.pos[j] = j < f.e.p.P ? s[j] : 0.f;
  if (R.nwp > 0) {
    follow_set_goal(g, f, n, 0);
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) g.goal[j] = g.pos[j];
  }
  if (f.path) follow_path_store(f, 0, n, g);
}

// step t of robot n (unfinished: R.k < R.nwp): trace (state before the step, observation, action), env.step, float64 reward sum,
// arrival and the next waypoint, path record.  Returns whether the robot is still unfinished afterwards.  XT / post: as
// eval_env_step's.
template <int XT = 0>
__device__ __forceinline__ bool follow_env_step(GoalState& g, FollowRobot& R, const FollowArgs& f, int n, int t, const float* act,
                                                const float* obs_row, float* post = nullptr) {
  const EvalArgs& a = f.e;
  float* fl = eval_trace_row<XT>(g, a, n, t, act, obs_row);
  const int k_before = R.k;
  const GoalOutcome o = goal_advance(g, a.p, act, a.A);
  if (post) { post[0] = g.pos[0]; post[1] = g.pos[1]; }
  R.steps += 1;
  R.ret_sum += (double)o.reward;
  if (o.reached) {
    f.arrival[(size_t)n * f.K + R.k] = t + 1;
    R.k += 1;
    if (R.k < R.nwp) follow_set_goal(g, f, n, R.k);
  }
  const bool going = R.k < R.nwp;
  if (fl) {
    fl[0] = o.reward; fl[1] = o.reached ? 1.f : 0.f; fl[2] = (float)k_before; fl[3] = going ? 0.f : 1.f;
  }
  if (f.path && (t + 1) % f.path_stride == 0) follow_path_store(f, (t + 1) / f.path_stride, n, g);
  return going;
}

// robot_out, and the path records after the robot's last step (a robot that finished early stays where it is)
__device__ __forceinline__ void follow_finish(const FollowArgs& f, int n, const FollowRobot& R, const GoalState& g) {
  double* o = f.e.robot_out + (size_t)n * 4;
  o[0] = R.ret_sum; o[1] = (double)R.steps; o[2] = (double)R.k;
  o[3] = R.nwp > 0 ? (double)goal_dist(g.goal, g.pos, f.e.p.P) : __longlong_as_double(0x7FF8000000000000ll);
  if (f.path)
    for (int r = R.steps / f.path_stride + 1; r <= f.e.max_steps / f.path_stride; ++r) follow_path_store(f, r, n, g);
}

// ------------------------------------------------------------------------------------------------
// per-step path: robot state in e.st, (reward sum, steps, waypoints reached) in e.robot_out between launches
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ FollowRobot follow_robot_load(const FollowArgs& f, int n) {
  const double* o = f.e.robot_out + (size_t)n * 4;
  return FollowRobot{o[0], (int)o[1], (int)o[2], f.nwp[n]};
}
__device__ __forceinline__ void follow_robot_store(const FollowArgs& f, int n, const FollowRobot& R) {
  double* o = f.e.robot_out + (size_t)n * 4;
  o[0] = R.ret_sum; o[1] = (double)R.steps; o[2] = (double)R.k;
}

// waypoint following as a task
struct FollowTask {
  using Args = FollowArgs;
  using Robot = FollowRobot;
  static __host__ __device__ __forceinline__ const EvalArgs& eval(const Args& f) { return f.e; }
  static __device__ __forceinline__ void start(GoalState& g, Robot& R, const Args& f, int n) { follow_start(g, R, f, n); }
  static constexpr bool kWide = false;
  static __device__ __forceinline__ bool active(const Args&, const Robot& R) { return R.k < R.nwp; }
  template <int XT = 0>
  static __device__ __forceinline__ bool step(GoalState& g, Robot& R, const Args& f, int n, int t, const float* act,
                                              const float* obs_row, float* post = nullptr) {
    return follow_env_step<XT>(g, R, f, n, t, act, obs_row, post);
  }
  static __device__ __forceinline__ int episodes(const Robot&) { return 0; }   // no episodes: no reset
  static __device__ __forceinline__ int steps(const Robot& R) { return R.steps; }
  static __device__ __forceinline__ bool recorded(const Robot&, int) { return false; }
  static __device__ __forceinline__ void finish(const Args& f, int n, const Robot& R, const GoalState& g) { follow_finish(f, n, R, g); }
  static __device__ __forceinline__ Robot load(const Args& f, int n) { return follow_robot_load(f, n); }
  static __device__ __forceinline__ void store(const Args& f, int n, const Robot& R) { follow_robot_store(f, n, R); }
};

__global__ __launch_bounds__(256) void k_follow_goal_fin(FollowArgs f) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= f.e.N) return;
  follow_finish(f, n, follow_robot_load(f, n), goal_load(f.e.st + (size_t)n * kGoalStateFloats));
}

}  // namespace mobrob
