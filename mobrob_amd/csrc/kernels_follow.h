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
//
// ResumeFollowTask (mobrob_ppo_follow_waypoints_resume) is the same rules as one call of a RUN: a sequence of calls over the same
// robots and seed, call c covering global steps step0 .. step0 + max_steps - 1.  The robot's position, velocity, reward sum, steps,
// waypoint index, arrival row and `leg_used` (steps spent on the waypoint in force) are read at entry and continued, the streams
// and the arrival steps use the global step, and a leg budget (leg_steps > 0) idles a robot that has spent it.  Path and trace
// stay local to the call.  A run split into calls gives the bits of one call (every carried value is continued, never re-summed).
//
// ScheduledFollowTask (mobrob_ppo_follow_waypoints_scheduled) is ResumeFollowTask with timed waypoints: release steps and holds,
// stated at the task below.
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
// eval_env_step's.  g0: the global step of the call's step 0 (a resumed run; arrival steps are global, trace and path local).
template <int XT = 0>
__device__ __forceinline__ bool follow_env_step(GoalState& g, FollowRobot& R, const FollowArgs& f, int n, int t, const float* act,
                                                const float* obs_row, float* post = nullptr, int g0 = 0) {
  const EvalArgs& a = f.e;
  float* fl = eval_trace_row<XT>(g, a, n, t, act, obs_row);
  const int k_before = R.k;
  const GoalOutcome o = goal_advance(g, a.p, act, a.A);
  if (post) { post[0] = g.pos[0]; post[1] = g.pos[1]; }
  R.steps += 1;
  R.ret_sum += (double)o.reward;
  if (o.reached) {
    f.arrival[(size_t)n * f.K + R.k] = g0 + t + 1;
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

// robot_out, and the path records after the robot's last step (a robot that finished early stays where it is).  entry_steps:
// R.steps at the call's entry (a resumed run: the path is the call's own)
__device__ __forceinline__ void follow_finish(const FollowArgs& f, int n, const FollowRobot& R, const GoalState& g,
                                              int entry_steps = 0) {
  double* o = f.e.robot_out + (size_t)n * 4;
  o[0] = R.ret_sum; o[1] = (double)R.steps; o[2] = (double)R.k;
  o[3] = R.nwp > 0 ? (double)goal_dist(g.goal, g.pos, f.e.p.P) : __longlong_as_double(0x7FF8000000000000ll);
  if (f.path)
    for (int r = (R.steps - entry_steps) / f.path_stride + 1; r <= f.e.max_steps / f.path_stride; ++r) follow_path_store(f, r, n, g);
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
  static constexpr bool kResume = false;
  static constexpr bool kFrames = false;
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

// ------------------------------------------------------------------------------------------------
// one call of a resumable run
// ------------------------------------------------------------------------------------------------
constexpr int kFollowGoing = 0, kFollowFinished = 1, kFollowStalled = 2, kFollowNoWaypoints = 3;   // status at exit

struct ResumeArgs {
  FollowArgs f;        // f.start is unused; f.e.robot_out [N][0..2] and f.arrival hold the run's values at entry
  int step0;           // global step of the call's step 0
  int leg_steps;       // step budget per waypoint, 0 = none
  float* state;        // [N][6] position, velocity: in / out
  int* leg_used;       // [N] steps spent on the waypoint in force: in / out
  int* status;         // [N] out
  int* entry_steps;    // [N] steps run at entry (per-step path: kept for the finish kernel's path records)
};

struct ResumeRobot {
  FollowRobot b;
  int leg_used, entry_steps;
};

struct ResumeFollowTask {
  using Args = ResumeArgs;
  using Robot = ResumeRobot;
  static constexpr bool kWide = false;
  static constexpr bool kResume = true;
  static constexpr bool kFrames = false;
  static __host__ __device__ __forceinline__ const EvalArgs& eval(const Args& a) { return a.f.e; }
  static __device__ __forceinline__ int step0(const Args& a) { return a.step0; }
  // the carried robot: pose and velocity from `state`, accumulators from robot_out, goal = the waypoint in force (a finished
  // robot keeps its last waypoint, one without waypoints its position, as after follow_start / follow_env_step); path record 0
  static __device__ __forceinline__ void start(GoalState& g, Robot& R, const Args& a, int n) {
    const FollowArgs& f = a.f;
    // GoalState.ep_len / ep_ret are NOT carried: they restart at 0 every call.  Nothing reads them here (no time limit, no episode
    // output); a task that gives following a time limit must carry them as well, or a split run differs from the unsplit one
    g = GoalState{};
    R.b = follow_robot_load(f, n);
    R.leg_used = a.leg_used[n];
    R.entry_steps = R.b.steps;
    const float* s = a.state + (size_t)n * 6;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      g.pos[j] = j < f.e.p.P ? s[j] : 0.f;
      g.vel[j] = j < f.e.p.P ? s[3 + j] : 0.f;
    }
    if (R.b.nwp > 0) {
      follow_set_goal(g, f, n, R.b.k < R.b.nwp ? R.b.k : R.b.nwp - 1);
    } else {
#pragma unroll
      for (int j = 0; j < 3; ++j) g.goal[j] = g.pos[j];
    }
    if (f.path) follow_path_store(f, 0, n, g);
  }
  static __device__ __forceinline__ bool active(const Args& a, const Robot& R) {
    return R.b.k < R.b.nwp && (a.leg_steps == 0 || R.leg_used < a.leg_steps);
  }
  template <int XT = 0>
  static __device__ __forceinline__ bool step(GoalState& g, Robot& R, const Args& a, int n, int t, const float* act,
                                              const float* obs_row, float* post = nullptr) {
    const int k0 = R.b.k;
    (void)follow_env_step<XT>(g, R.b, a.f, n, t, act, obs_row, post, a.step0);
    R.leg_used = (R.b.k != k0 || a.leg_steps == 0) ? 0 : R.leg_used + 1;   // an arrival starts the next leg; no budget, no count
    return active(a, R);
  }
  static __device__ __forceinline__ int episodes(const Robot&) { return 0; }
  static __device__ __forceinline__ int steps(const Robot& R) { return R.b.steps; }
  static __device__ __forceinline__ bool recorded(const Robot&, int) { return false; }
  static __device__ __forceinline__ void finish(const Args& a, int n, const Robot& R, const GoalState& g) {
    follow_finish(a.f, n, R.b, g, R.entry_steps);
    float* s = a.state + (size_t)n * 6;
#pragma unroll
    for (int j = 0; j < 3; ++j) { s[j] = g.pos[j]; s[3 + j] = g.vel[j]; }
    a.leg_used[n] = R.leg_used;
    a.status[n] = R.b.nwp == 0 ? kFollowNoWaypoints : R.b.k >= R.b.nwp ? kFollowFinished
                  : (a.leg_steps > 0 && R.leg_used >= a.leg_steps) ? kFollowStalled : kFollowGoing;
  }
  static __device__ __forceinline__ Robot load(const Args& a, int n) {
    return Robot{follow_robot_load(a.f, n), a.leg_used[n], a.entry_steps[n]};
  }
  static __device__ __forceinline__ void store(const Args& a, int n, const Robot& R) {
    follow_robot_store(a.f, n, R.b);
    a.leg_used[n] = R.leg_used;
    a.entry_steps[n] = R.entry_steps;
  }
};

// ------------------------------------------------------------------------------------------------
// one call of a run with TIMED waypoints (mobrob_ppo_follow_waypoints_scheduled)
//
// The rule, stated once in mobrob_amd/envs/goal_rules.py (Schedule): waypoint k of robot n may not be the goal in force in a step
// whose 0-based global number g is below release[n][k].  Until then the robot HOLDS at its anchor -- the previous waypoint, `home`
// for k = 0 -- under the policy.  k keeps its meaning (waypoints reached), and the goal used in global step g is a pure function
// of (k, g): nothing is carried for it.
//   hold(k, g) = k < nwp and g < release[n][k]      goal(k, g) = hold ? (k > 0 ? wp[n][k - 1] : home[n]) : wp[n][min(k, nwp - 1)]
// It is set at `start` for g = step0 and at the end of the step g, after any arrival, for g + 1, so the observation of every step
// is computed from the goal of that step.  A hold step (hold at the step's entry) runs goal_advance, steps, path, trace and the
// wrapping tasks' checks as any step; it ignores `reached`, adds nothing to the reward sum, writes flags 0, 0 and leaves leg_used
// as it is.  sched_out [N][2] is carried like hazard_out: hold steps run, the largest float32 distance to the anchor after a hold
// step (NaN: none yet).  robot_out[3] is the distance to the waypoint the robot is on, released or not.  With every release 0 no
// step is a hold step and every step is ResumeFollowTask's.
// ------------------------------------------------------------------------------------------------
struct ScheduledArgs {
  ResumeArgs r;
  const int* release;  // [N][K] first global step in which waypoint k may be the goal in force
  const float* home;   // [N][P] anchor of waypoint 0
  double* sched_out;   // [N][2] in / out; per-step path: live state between launches
};

struct ScheduledRobot : ResumeRobot {   // (derived, not nested: the carried robot is ResumeFollowTask's own object)
  int holds;           // hold steps run
  float drift;         // largest distance to the anchor after one (0 before the first)
};

// the goal of robot n, on waypoint k of nwp, in global step gs (a robot without waypoints keeps the goal `start` gave it)
__device__ __forceinline__ void sched_set_goal(GoalState& g, const ScheduledArgs& a, int n, int k, int nwp, int gs) {
  const FollowArgs& f = a.r.f;
  if (nwp <= 0) return;
  const bool hold = k < nwp && gs < a.release[(size_t)n * f.K + k];
  const int P = f.e.p.P;
  // the row the goal is read from: home for a hold on waypoint 0, else waypoint k - 1 (hold), k, or the last one
  const float* src = (hold && k == 0) ? a.home + (size_t)n * P : f.wp + ((size_t)n * f.K + (hold ? k - 1 : (k < nwp ? k : nwp - 1))) * P;
#pragma unroll
  for (int j = 0; j < 3; ++j) g.goal[j] = j < P ? src[j] : 0.f;
}

// follow_env_step with holds: `hold` names a hold step -- the robot waits at the goal in force: no arrival, no reward sum, flags
// 0 and 0; returns max(held_in, its distance to that goal after the step), held_in on any other step.  The goal of the next step is the caller's to set, arrival or
// not.  With hold = false it performs follow_env_step's operations in follow_env_step's order (minus the goal).  It is a function
// of its own, not a flag on follow_env_step: sharing one template body changed the register allocation of 13 existing tile
// kernels, and the existing tasks keep their instructions.
template <int XT = 0>
__device__ __forceinline__ float sched_env_step(GoalState& g, FollowRobot& R, const FollowArgs& f, int n, int t, const float* act,
                                               const float* obs_row, float* post, int g0, bool hold, float held_in) {
  const EvalArgs& a = f.e;
  float* fl = eval_trace_row<XT>(g, a, n, t, act, obs_row);
  const int k_before = R.k;
  const GoalOutcome o = goal_advance(g, a.p, act, a.A);
  if (post) { post[0] = g.pos[0]; post[1] = g.pos[1]; }
  R.steps += 1;
  const bool arrived = o.reached && !hold;
  const float held_at = hold ? fmaxf(held_in, goal_dist(g.goal, g.pos, a.p.P)) : held_in;
  if (!hold) R.ret_sum += (double)o.reward;
  if (arrived) {
    f.arrival[(size_t)n * f.K + R.k] = g0 + t + 1;
    R.k += 1;
  }
  const bool going = R.k < R.nwp;
  if (fl) {
    fl[0] = hold ? 0.f : o.reward; fl[1] = arrived ? 1.f : 0.f; fl[2] = (float)k_before; fl[3] = going ? 0.f : 1.f;
  }
  if (f.path && (t + 1) % f.path_stride == 0) follow_path_store(f, (t + 1) / f.path_stride, n, g);
  return held_at;
}

struct ScheduledFollowTask {
  using Args = ScheduledArgs;
  using Robot = ScheduledRobot;
  using B = ResumeFollowTask;
  static constexpr bool kWide = false;
  static constexpr bool kResume = true;
  static constexpr bool kFrames = false;
  static __host__ __device__ __forceinline__ const EvalArgs& eval(const Args& a) { return B::eval(a.r); }
  static __device__ __forceinline__ int step0(const Args& a) { return a.r.step0; }
  static __device__ __forceinline__ void sched_load(const Args& a, int n, Robot& R) {
    const double* o = a.sched_out + (size_t)n * 2;
    R.holds = (int)o[0];
    R.drift = R.holds > 0 ? (float)o[1] : 0.f;
  }
  static __device__ __forceinline__ void sched_store(const Args& a, int n, const Robot& R) {
    double* o = a.sched_out + (size_t)n * 2;
    o[0] = (double)R.holds;
    o[1] = R.holds > 0 ? (double)R.drift : __longlong_as_double(0x7FF8000000000000ll);   // NaN: no hold step run
  }
  static __device__ __forceinline__ void start(GoalState& g, Robot& R, const Args& a, int n) {
    B::start(g, R, a.r, n);
    sched_load(a, n, R);
    sched_set_goal(g, a, n, R.b.k, R.b.nwp, a.r.step0);
  }
  static __device__ __forceinline__ bool active(const Args& a, const Robot& R) { return B::active(a.r, R); }
  // an active robot: k < nwp at entry, so release[n][k] is a row in use
  template <int XT = 0>
  static __device__ __forceinline__ bool step(GoalState& g, Robot& R, const Args& a, int n, int t, const float* act,
                                              const float* obs_row, float* post = nullptr) {
    const int gs = a.r.step0 + t, k0 = R.b.k;
    const bool hold = gs < a.release[(size_t)n * a.r.f.K + k0];
    R.drift = sched_env_step<XT>(g, R.b, a.r.f, n, t, act, obs_row, post, a.r.step0, hold, R.drift);
    if (hold) {
      R.holds += 1;                                      // waiting is not charged to the leg
    } else {
      R.leg_used = (R.b.k != k0 || a.r.leg_steps == 0) ? 0 : R.leg_used + 1;
    }
    if (hold || R.b.k != k0) sched_set_goal(g, a, n, R.b.k, R.b.nwp, gs + 1);   // only a hold or an arrival changes the goal
    return active(a, R);
  }
  static __device__ __forceinline__ int episodes(const Robot&) { return 0; }
  static __device__ __forceinline__ int steps(const Robot& R) { return B::steps(R); }
  static __device__ __forceinline__ bool recorded(const Robot&, int) { return false; }
  static __device__ __forceinline__ void finish(const Args& a, int n, const Robot& R, const GoalState& g) {
    B::finish(a.r, n, R, g);
    if (R.b.nwp > 0) {                                 // final distance: to the waypoint the robot is on, released or not
      const FollowArgs& f = a.r.f;
      const float* w = f.wp + ((size_t)n * f.K + (R.b.k < R.b.nwp ? R.b.k : R.b.nwp - 1)) * f.e.p.P;
      f.e.robot_out[(size_t)n * 4 + 3] = (double)goal_dist(w, g.pos, f.e.p.P);
    }
    sched_store(a, n, R);
  }
  static __device__ __forceinline__ Robot load(const Args& a, int n) {
    Robot R;
    static_cast<ResumeRobot&>(R) = B::load(a.r, n);
    sched_load(a, n, R);
    return R;
  }
  static __device__ __forceinline__ void store(const Args& a, int n, const Robot& R) {
    B::store(a.r, n, R);
    sched_store(a, n, R);
  }
};

}  // namespace mobrob
