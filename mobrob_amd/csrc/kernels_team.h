// Robot teams (mobrob_ppo_follow_waypoints_teams): pairwise separation costs between the robots of a waypoint-following run.
//
// The rule, stated once in array form in mobrob_amd/envs/goal_rules.py (team_cost): robots are partitioned into teams of
// team_size consecutive robots (1, 2, 4, 8 or 16; n % team_size == 0, so a team never straddles a 16-robot tile).  After the step
// with global number g, for every robot i that stepped in it, with p the post-step xy positions (x and y only, as for hazards) and
// the team-mates j != i -- a mate that did not step counts where it stands --
//   d_ij = |p_i - p_j|                              (float, every operation correctly rounded on its own, no fma)
//   cost_i = c * sum over d_ij <= sep of (sep - d_ij);  indicator: cost_i = (cost_i > 0)
//   clear_i = min_j (d_ij - sep)  (+inf alone),  partner_i = the j that attains it (equal clearances: the lowest j)
// Robots of different teams never see each other.  The cost never changes dynamics, reward, arrivals or any other output.
//
// The sums run over four partial sums as the hazards' do: quarter q takes the team-local members m = q, q + 4, ... (skipping i),
// combined as (p0 + p1) + (p2 + p3), the coefficient applied once afterwards; the (clearance, partner) minimum runs over the same
// quarters and the same two exchanges (smaller clearance wins, equal clearances go to the smaller index).  The tile kernel computes
// the quarters on four lanes per robot from the tile's [16][2] xy block in LDS, the per-step path in one thread per robot from the
// state rows (k_team_step, launched after k_goal_task_step): both give the same bits for the same positions.
//
// TeamTask<Base> wraps a task of a RUN (ResumeFollowTask, HazardTask<ResumeFollowTask>, FrameHazardTask<ResumeFollowTask>): its
// Robot adds the five accumulators of team_out [N][5] (float64 cost sum, conflict steps, first conflict step (global, 1-based, -1:
// none), minimum clearance (NaN: no step run), the partner's global index at that minimum (first attainment, -1: none)), read at
// entry and continued like hazard_out.
#pragma once
#include "kernels_hazard.h"

namespace mobrob {

template <class BaseArgs>
struct TeamArgs {
  BaseArgs b;              // the wrapped task's arguments
  int team_size;           // 1, 2, 4, 8 or 16
  float sep, coef;         // separation, cost coefficient
  int indicator;
  double* team_out;        // [N][5] in / out; per-step path: live state (k_team_step accumulates into it)
  int* stepped;            // [N] per-step path: the call's last step in which robot n stepped, -1 = none yet
};

struct TeamAcc {
  double cost_sum;
  int conflicts, first, partner;
  float min_clear;
};

// one quarter's partial (unscaled) cost and (clearance, partner) of team-local member mi: mates m = q, q + 4, ... < ts of the team
// whose xy rows start at `xy` (row stride `stride` floats); partner is team-local, -1 without a mate
__device__ __forceinline__ void team_partial(const float* xy, int stride, int ts, int mi, int q, float sep, float& cost,
                                             float& clear, int& partner) {
  cost = 0.f;
  clear = __builtin_inff();
  partner = -1;
  const float px = xy[mi * stride], py = xy[mi * stride + 1];
  for (int m = q; m < ts; m += 4) {
    if (m == mi) continue;
    const float dx = px - xy[m * stride], dy = py - xy[m * stride + 1];
    // every operation rounded on its own: hipcc contracts a product that feeds a sum into one fma unless the product is pinned
    // (kernels_env.h: rounded), and goal_rules.team_cost, which the device is held to bit for bit, has no fma
    // sqrtf is the correctly rounded root (__fsqrt_rn is the hardware's approximate one, within 1 ulp)
    const float d = sqrtf(__fadd_rn(rounded(__fmul_rn(dx, dx)), rounded(__fmul_rn(dy, dy))));
    if (d <= sep) cost = __fadd_rn(cost, __fsub_rn(sep, d));
    const float cl = __fsub_rn(d, sep);
    if (cl < clear) { clear = cl; partner = m; }   // ascending m: equal clearances keep the lower index
  }
}

// (clear, partner) <- the better of it and (c2, p2): smaller clearance, then smaller index
__device__ __forceinline__ void team_closer(float& clear, int& partner, float c2, int p2) {
  if (c2 < clear || (c2 == clear && p2 < partner)) { clear = c2; partner = p2; }
}

// the step's cost / clearance / partner (global index) -> the accumulators.  g1: the step's global 1-based number
__device__ __forceinline__ void team_account(TeamAcc& T, float coef, int indicator, int g1, float sum, float clear, int partner) {
  const float s = __fmul_rn(coef, sum);
  const float cost = indicator ? (s > 0.f ? 1.f : 0.f) : s;
  T.cost_sum += (double)cost;
  if (cost > 0.f) {
    T.conflicts += 1;
    if (T.first < 0) T.first = g1;
  }
  if (clear < T.min_clear) { T.min_clear = clear; T.partner = partner; }   // strict: the first attainment is kept
}

// steps: the steps the robot has run in the RUN (0: nothing measured yet, clearance NaN <-> +inf)
__device__ __forceinline__ TeamAcc team_load(const double* o, int steps) {
  return TeamAcc{o[0], (int)o[1], (int)o[2], (int)o[4], steps > 0 ? (float)o[3] : __builtin_inff()};
}
__device__ __forceinline__ void team_store(double* o, const TeamAcc& T, int steps) {
  o[0] = T.cost_sum; o[1] = (double)T.conflicts; o[2] = (double)T.first;
  o[3] = steps > 0 ? (double)T.min_clear : __longlong_as_double(0x7FF8000000000000ll);   // NaN: no step run
  o[4] = (double)T.partner;
}

template <class Base>
struct TeamTask {
  static_assert(Base::kResume, "teams are a property of a run: the wrapped task must be resumable");
  using TeamBase = Base;   // marks the task for the compile-time hooks of k_goal64_tile / the per-step launch (task_teams)
  using Args = TeamArgs<typename Base::Args>;
  struct Robot {
    typename Base::Robot b;
    TeamAcc team;
    int last;              // per-step path: Args::stepped of the robot
  };
  static constexpr bool kWide = true;
  static constexpr bool kResume = true;
  static constexpr bool kFrames = Base::kFrames;
  static __device__ __forceinline__ int step0(const Args& a) { return Base::step0(a.b); }
  static __host__ __device__ __forceinline__ const EvalArgs& eval(const Args& a) { return Base::eval(a.b); }
  // LDS of k_goal64_tile beyond LayEval64::END: a wide base has the [16][2] xy block already (first, before its scene)
  static size_t tile_lds_bytes(const Args& a) {
    if constexpr (Base::kWide) return Base::tile_lds_bytes(a.b);
    else return 32 * sizeof(float);
  }

  static __device__ __forceinline__ void start(GoalState& g, Robot& R, const Args& a, int n) {
    Base::start(g, R.b, a.b, n);
    R.team = team_load(a.team_out + (size_t)n * 5, Base::steps(R.b));
    R.last = -1;
  }
  static __device__ __forceinline__ bool active(const Args& a, const Robot& R) { return Base::active(a.b, R.b); }

  // per-step path: the base's step; the check needs the mates' post-step positions and runs in k_team_step after the launch
  static __device__ __forceinline__ bool step(GoalState& g, Robot& R, const Args& a, int n, int t, const float* act,
                                              const float* obs_row) {
    R.last = t;
    if constexpr (Base::kWide) return Base::step(g, R.b, a.b, n, t, act, obs_row);
    else return Base::template step<0>(g, R.b, a.b, n, t, act, obs_row);
  }

  // ---- k_goal64_tile ----
  static __device__ __forceinline__ int frame(const Args& a, int g) { return Base::frame(a.b, g); }   // kFrames only
  static __device__ __forceinline__ void stage_frame(const Args& a, float* hz_lds, int lane, int f) { Base::stage_frame(a.b, hz_lds, lane, f); }
  static __device__ __forceinline__ void stage(const Args& a, float* hz_lds, int lane) {
    if constexpr (Base::kWide) Base::stage(a.b, hz_lds, lane);
  }
  // before the step loop, every robot lane (active or not): the carried position -> the robot's row of the xy block, so that a
  // robot that never steps in this call is an obstacle from step 0
  static __device__ __forceinline__ void place(const GoalState& g, float* xy) { xy[0] = g.pos[0]; xy[1] = g.pos[1]; }
  static __device__ __forceinline__ bool step_lane(GoalState& g, Robot& R, const Args& a, int n, int t, const float* act,
                                                   const float* obs_row, float* xy, int& e0) {
    if constexpr (Base::kWide) return Base::step_lane(g, R.b, a.b, n, t, act, obs_row, xy, e0);
    else return Base::template step<0>(g, R.b, a.b, n, t, act, obs_row, xy);
  }
  // every lane: the base's wide phase, then quarter q = lane >> 4 of robot r16 = lane & 15 against its team's rows of xy.
  // Barriers: both phases only READ LDS (xy, the base's scene) and write registers / global memory, so none is needed between
  // them; the kernel's barrier before after_step orders this step's xy writes before these reads, and its barrier after
  // after_step orders these reads before the next step's xy writes (and before a restaged frame).  The rows of robots that do
  // not step keep what `place` or their last step wrote.
  static __device__ __forceinline__ void after_step(const Args& a, Robot& R, int n, int t, int lane, bool stepped, int e0,
                                                    const float* xy, const float* hz_lds) {
    if constexpr (Base::kWide) Base::after_step(a.b, R.b, n, t, lane, stepped, e0, xy, hz_lds);
    const int r16 = lane & 15, q = lane >> 4, ts = a.team_size;
    const int mi = r16 & (ts - 1), tb = r16 - mi;   // team-local index, the team's first row in the tile
    float c = 0.f, cl = __builtin_inff();
    int pt = -1;
    if (stepped) team_partial(xy + 2 * tb, 2, ts, mi, q, a.sep, c, cl, pt);
    // lanes r16, r16 + 16, r16 + 32, r16 + 48 hold quarters 0..3: (p0 + p1) + (p2 + p3) and the same two exchanges for the minimum
    const float c01 = __fadd_rn(c, __shfl_xor(c, 16, 64));
    const float cs = __fadd_rn(c01, __shfl_xor(c01, 32, 64));
    team_closer(cl, pt, __shfl_xor(cl, 16, 64), __shfl_xor(pt, 16, 64));
    team_closer(cl, pt, __shfl_xor(cl, 32, 64), __shfl_xor(pt, 32, 64));
    if (lane < 16 && stepped)
      team_account(R.team, a.coef, a.indicator, Base::step0(a.b) + t + 1, cs, cl, pt < 0 ? -1 : n - mi + pt);
  }

  static __device__ __forceinline__ void finish(const Args& a, int n, const Robot& R, const GoalState& g) {
    Base::finish(a.b, n, R.b, g);
    team_store(a.team_out + (size_t)n * 5, R.team, Base::steps(R.b));
  }
  // per-step path: team_out is k_team_step's between the launches; `store` keeps the base's state and the stepped record
  static __device__ __forceinline__ Robot load(const Args& a, int n) {
    Robot R;
    R.b = Base::load(a.b, n);
    R.team = team_load(a.team_out + (size_t)n * 5, Base::steps(R.b));
    R.last = a.stepped[n];
    return R;
  }
  static __device__ __forceinline__ void store(const Args& a, int n, const Robot& R) {
    Base::store(a.b, n, R.b);
    a.stepped[n] = R.last;
  }
};

// per-step path, after k_goal_task_step of step t on the same stream: the check of every robot that stepped in t, one thread per
// robot, the four quarters in turn in the tile's order; mates' post-step positions from the state rows (a mate that did not step:
// where it stands).  steps run (robot_out[n][1]) already counts step t, so it is > 0 here.
template <class Base>
__global__ __launch_bounds__(256) void k_team_step(TeamArgs<typename Base::Args> a, int t) {
  const EvalArgs& e = Base::eval(a.b);
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= e.N || a.stepped[n] != t) return;
  const int ts = a.team_size, mi = n % ts, tb = n - mi;
  const float* rows = e.st + (size_t)tb * kGoalStateFloats;
  float c[4], cl[4];
  int pt[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) team_partial(rows, kGoalStateFloats, ts, mi, q, a.sep, c[q], cl[q], pt[q]);
  team_closer(cl[0], pt[0], cl[1], pt[1]);
  team_closer(cl[2], pt[2], cl[3], pt[3]);
  team_closer(cl[0], pt[0], cl[2], pt[2]);
  double* o = a.team_out + (size_t)n * 5;
  const int before = (int)e.robot_out[(size_t)n * 4 + 1] - 1;   // steps run before step t
  TeamAcc T = team_load(o, before);
  team_account(T, a.coef, a.indicator, Base::step0(a.b) + t + 1, __fadd_rn(__fadd_rn(c[0], c[1]), __fadd_rn(c[2], c[3])), cl[0],
               pt[0] < 0 ? -1 : tb + pt[0]);
  team_store(o, T, 1);
}

}  // namespace mobrob
