// Solid teams (mobrob_ppo_follow_waypoints_teams_solid): team-mates are obstacles inside the env step.
//
// The rule, stated once in mobrob_amd/envs/goal_rules.py (team_block, team_block_step): a mate is one more box of wall_block's rule,
// the closed square with Hx = Hy = sep exactly around where the mate stands; with solid walls the scene's boxes (Hx = hx + radius,
// Hy = hy + radius) join the same list, so the candidates c0 .. c3 are tested against mates and walls at once.  A box that holds the
// pre-step position does not hold in this step (`inside` for a mate, `wall_inside` for a wall).  A blocked step is by_mate when a
// rejected candidate met a mate's square and by_wall when one met a wall: team_blocked_out [N][4] counts the first kind,
// blocked_out [N][4] the second, each in blocked_out's form (steps, first step (global, 1-based, -1: none), stopped steps (code 3),
// inside steps).
//
// Where a mate stands, and the order: serial inside a team by team-local index m = 0 .. size - 1 within one global step -- member m
// resolves against lower-index mates where they stand AFTER this step's resolve, against higher-index mates where they stood BEFORE
// the step; a mate that does not step counts where it stands.  The proposals (velocity update, clamp) do not depend on the mates.
//
// On the device the team's rows of "where every mate stands" exist already: on the tile the [16][2] xy block in LDS (TeamTask::place
// fills it before the loop, every robot's lane overwrites its own row in its step), on the per-step path the x, y of the state rows
// in global memory (a robot's row holds its pre-step position until the robot stores it).  A team is size <= 16 consecutive robots
// with n % size == 0, so its lanes lie in one wave on both paths: the env phase of k_goal64_tile runs on lanes 0..15 of the
// workgroup's only wave, k_goal_task_step gives consecutive robots consecutive lanes and 64 % size == 0.  The resolve is therefore
// a loop r = 0 .. size - 1 (uniform trip count: the size, not the active mates) inside the env step: the lanes with m == r read
// their team's rows, resolve and write their own row; a fence ends each iteration.  One wave executes the loop in lock step and
// its LDS (and, to one address, its global) accesses complete in issue order, so iteration r + 1 reads what iteration r wrote; the
// rows are accessed as volatile and the fence keeps the compiler from moving them across iterations.  No barrier and no hook of
// k_goal64_tile or k_goal_task_step is added.
//
// SolidTeamFollowTask<B, kWalls> restates B = ResumeFollowTask / ScheduledFollowTask with that step, as SolidFollowTask does for
// walls alone (goal_advance, follow_env_step, sched_env_step, solid_goal_advance, solid_env_step and wall_resolve keep their
// instructions: they are not touched).  It is always wrapped in TeamTask -- TeamTask<SolidTeamFollowTask<B, false>> for solid teams
// alone, TeamTask<WallTask<SolidTeamFollowTask<B, true>>> with solid walls, where WallTask names the robot's scene to it before
// every step --, whose separation check then runs on the resolved positions and stays observational.
#pragma once
#include "kernels_wall.h"

namespace mobrob {

struct TeamResolved {
  float qx, qy;
  int code;
  bool inside, wall_inside, by_mate, by_wall;
};

// the rule for ONE robot: pre-step (ax, ay), proposed (px, py), the team's rows (x, y at rows[j * stride], rows[j * stride + 1];
// its own row mi is skipped), the scene w of m walls (kWalls) -> the resolved position, the code and the flags.  One loop per
// candidate c0, c1, c2 until one is clean; every pass visits every box (the first decides `inside` over all of them).
template <bool kWalls>
__device__ __forceinline__ TeamResolved team_resolve(const volatile float* rows, int stride, int ts, int mi, float sep, const float* w,
                                                     int m, float radius, float ax, float ay, float px, float py) {
  TeamResolved r{px, py, 0, false, false, false, false};
  for (; r.code < 3; ++r.code) {
    r.qx = r.code == 2 ? ax : px;
    r.qy = r.code == 1 ? ay : py;
    const float ex = rounded(__fmul_rn(0.5f, __fsub_rn(r.qx, ax))), ey = rounded(__fmul_rn(0.5f, __fsub_rn(r.qy, ay)));
    const float sx = rounded(__fmul_rn(0.5f, __fadd_rn(ax, r.qx))), sy = rounded(__fmul_rn(0.5f, __fadd_rn(ay, r.qy)));
    const float aex = fabsf(ex), aey = fabsf(ey);
    bool hit_m = false, hit_w = false;
    const float reach_m = __fadd_rn(rounded(__fmul_rn(sep, aey)), rounded(__fmul_rn(sep, aex)));
    for (int j = 0; j < ts; ++j) {   // no branch in the body: a lane-private loop inside the serial resolve
      const float cx = rows[j * stride], cy = rows[j * stride + 1];
      const bool mate = j != mi;
      const bool within = fabsf(__fsub_rn(ax, cx)) <= sep && fabsf(__fsub_rn(ay, cy)) <= sep;   // the mate does not hold in this step
      const float mx = __fsub_rn(sx, cx), my = __fsub_rn(sy, cy);
      const float cross = fabsf(__fsub_rn(rounded(__fmul_rn(mx, ey)), rounded(__fmul_rn(my, ex))));
      const bool apart = fabsf(mx) > __fadd_rn(sep, aex) || fabsf(my) > __fadd_rn(sep, aey) || cross > reach_m;
      r.inside = r.inside || (mate && within);
      hit_m = hit_m || (mate && !within && !apart);
    }
    if constexpr (kWalls) {
      for (int i = 0; i < m; ++i) {   // wall_resolve's body (kernels_wall.h), restated
        const float cx = w[4 * i], cy = w[4 * i + 1];
        const float Hx = __fadd_rn(w[4 * i + 2], radius), Hy = __fadd_rn(w[4 * i + 3], radius);
        const bool within = fabsf(__fsub_rn(ax, cx)) <= Hx && fabsf(__fsub_rn(ay, cy)) <= Hy;
        const float mx = __fsub_rn(sx, cx), my = __fsub_rn(sy, cy);
        const float cross = fabsf(__fsub_rn(rounded(__fmul_rn(mx, ey)), rounded(__fmul_rn(my, ex))));
        const float reach = __fadd_rn(rounded(__fmul_rn(Hx, aey)), rounded(__fmul_rn(Hy, aex)));
        const bool apart = fabsf(mx) > __fadd_rn(Hx, aex) || fabsf(my) > __fadd_rn(Hy, aey) || cross > reach;
        r.wall_inside = r.wall_inside || within;
        hit_w = hit_w || (!within && !apart);
      }
    }
    if (!(hit_m || hit_w)) return r;
    r.by_mate = r.by_mate || hit_m;
    r.by_wall = r.by_wall || hit_w;
  }
  r.qx = ax; r.qy = ay;   // c3, untested
  return r;
}

struct SolidTeamOutcome {
  GoalOutcome o;
  TeamResolved r;
};

// solid_goal_advance (kernels_wall.h) with the serial resolve of the team in the resolution's place: the same operations in the
// same order around it.  rows: the team's first row (LDS on the tile: kTile; the state rows in global memory otherwise).
template <bool kWalls, bool kTile, class GP>
__device__ __forceinline__ SolidTeamOutcome solid_team_goal_advance(GoalState& g, const GP& p, const float* act, int A,
                                                                    volatile float* rows, int stride, int ts, int mi, float sep,
                                                                    const float* ws, int m, float radius) {
  float cmd[3] = {0.f, 0.f, 0.f};
  for (int k = 0; k < A; ++k) {
    const float a = act[k];
#pragma unroll
    for (int j = 0; j < 3; ++j) cmd[j] = __fmaf_rn(p.mix[j][k], a, cmd[j]);
  }
  const float d0 = goal_dist(g.goal, g.pos, p.P);
  const float ax = g.pos[0], ay = g.pos[1];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (j < p.P) {
      g.vel[j] = __fmaf_rn(0.8f, g.vel[j], __fmul_rn(0.2f, cmd[j]));
      g.pos[j] = fminf(fmaxf(__fmaf_rn(p.dt, g.vel[j], g.pos[j]), -p.extent), p.extent);
    }
  }
  const float px = g.pos[0], py = g.pos[1];
  SolidTeamOutcome s;
  s.r = TeamResolved{px, py, 0, false, false, false, false};
  // the serial order: every lane of the team that steps runs all `ts` iterations; the lanes with mi == k resolve and publish
  for (int k = 0; k < ts; ++k) {
    if (k == mi) {
      s.r = team_resolve<kWalls>(rows, stride, ts, mi, sep, ws, m, radius, ax, ay, px, py);
      rows[mi * stride] = s.r.qx;
      rows[mi * stride + 1] = s.r.qy;
    }
    if constexpr (kTile) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    else __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  }
  g.pos[0] = s.r.qx; g.pos[1] = s.r.qy;
  if (s.r.code & 2) g.vel[0] = 0.f;   // x dropped (2, 3)
  if (s.r.code & 1) g.vel[1] = 0.f;   // y dropped (1, 3)
  const float d1 = goal_dist(g.goal, g.pos, p.P);
  GoalOutcome& o = s.o;
  o.reached = d1 < p.reach;
  o.reward = __fadd_rn(__fsub_rn(d0, d1), o.reached ? __fadd_rn(p.bonus, p.extra_bonus) : 0.f);
  o.term = p.terminate_on_goal && o.reached;
  g.ep_len += 1;
  g.ep_ret = __fadd_rn(g.ep_ret, o.reward);
  o.tr = g.ep_len >= p.time_limit && !o.term;
  o.done = o.term || o.tr;
  return s;
}

// a blocked step of the kind `by` -> the record (SolidAcc: kernels_wall.h)
__device__ __forceinline__ void solid_team_account(SolidAcc& S, bool by, int code, bool inside, int g1) {
  if (by) {
    S.blocked += 1;
    if (S.first < 0) S.first = g1;
    if (code == 3) S.stopped += 1;
  }
  if (inside) S.inside += 1;
}

template <class BaseArgs>
struct SolidTeamArgs {
  BaseArgs b;              // ResumeArgs / ScheduledArgs
  int team_size;           // TeamArgs' (the wrapping TeamTask checks with the same two)
  float sep;
  float radius;            // kWalls: the scene itself is WallArgs' (named to the robot by WallTask before every step)
  int* team_blocked_out;   // [N][4] in / out; per-step path: live state between the launches
  int* blocked_out;        // [N][4] in / out, kWalls only
};

template <class BaseRobot>
struct SolidTeamRobot {
  BaseRobot b;
  SolidAcc team, wall;
  const float* ws;         // kWalls: the robot's scene for the step at hand and its wall count
  int m;
};

// solid_env_step (kernels_wall.h) with solid_team_goal_advance; on the tile the robot's row of the xy block is written by the
// resolve itself (it is `post`).
template <int XT, bool kWalls, bool kTile>
__device__ __forceinline__ float solid_team_env_step(GoalState& g, FollowRobot& R, SolidAcc& ST, SolidAcc& SW, const FollowArgs& f, int n,
                                                    int t, const float* act, const float* obs_row, volatile float* rows, int stride,
                                                    int ts, int mi, float sep, int g0, bool hold, float held_in, const float* ws, int m,
                                                    float radius) {
  const EvalArgs& a = f.e;
  float* fl = eval_trace_row<XT>(g, a, n, t, act, obs_row);
  const int k_before = R.k;
  const SolidTeamOutcome so = solid_team_goal_advance<kWalls, kTile>(g, a.p, act, a.A, rows, stride, ts, mi, sep, ws, m, radius);
  const GoalOutcome o = so.o;
  solid_team_account(ST, so.r.by_mate, so.r.code, so.r.inside, g0 + t + 1);
  if constexpr (kWalls) solid_team_account(SW, so.r.by_wall, so.r.code, so.r.wall_inside, g0 + t + 1);
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

template <class B, bool kWalls>
struct SolidTeamFollowTask {
  static constexpr bool kScheduled = std::is_same_v<B, ScheduledFollowTask>;
  static_assert(kScheduled || std::is_same_v<B, ResumeFollowTask>, "solid teams restate the two run tasks");
  using Args = SolidTeamArgs<typename B::Args>;
  using Robot = SolidTeamRobot<typename B::Robot>;
  static constexpr bool kWide = false;
  static constexpr bool kResume = true;
  static constexpr bool kFrames = false;
  static __host__ __device__ __forceinline__ const EvalArgs& eval(const Args& a) { return B::eval(a.b); }
  static __device__ __forceinline__ int step0(const Args& a) { return B::step0(a.b); }
  static __device__ __forceinline__ const ResumeArgs& resume(const Args& a) {
    if constexpr (kScheduled) return a.b.r;
    else return a.b;
  }
  static __device__ __forceinline__ SolidAcc acc_load(const int* out, int n) {
    const int* o = out + (size_t)n * 4;
    return SolidAcc{o[0], o[1], o[2], o[3]};
  }
  static __device__ __forceinline__ void acc_store(int* out, int n, const SolidAcc& S) {
    int* o = out + (size_t)n * 4;
    o[0] = S.blocked; o[1] = S.first; o[2] = S.stopped; o[3] = S.inside;
  }
  static __device__ __forceinline__ void accs_load(const Args& a, int n, Robot& R) {
    R.team = acc_load(a.team_blocked_out, n);
    if constexpr (kWalls) R.wall = acc_load(a.blocked_out, n);
    else R.wall = SolidAcc{0, -1, 0, 0};
    R.ws = nullptr; R.m = 0;
  }
  static __device__ __forceinline__ void accs_store(const Args& a, int n, const Robot& R) {
    acc_store(a.team_blocked_out, n, R.team);
    if constexpr (kWalls) acc_store(a.blocked_out, n, R.wall);
  }
  static __device__ __forceinline__ void start(GoalState& g, Robot& R, const Args& a, int n) {
    B::start(g, R.b, a.b, n);
    accs_load(a, n, R);
  }
  static __device__ __forceinline__ bool active(const Args& a, const Robot& R) { return B::active(a.b, R.b); }
  // ResumeFollowTask::step / ScheduledFollowTask::step with solid_team_env_step.  rows: the team's first row
  template <int XT, bool kTile>
  static __device__ __forceinline__ bool step_on(GoalState& g, Robot& R, const Args& a, int n, int t, const float* act,
                                                 const float* obs_row, volatile float* rows, int stride, int mi) {
    const ResumeArgs& r = resume(a);
    const int k0 = R.b.b.k;
    if constexpr (kScheduled) {
      const int gs = r.step0 + t;
      const bool hold = gs < a.b.release[(size_t)n * r.f.K + k0];
      R.b.drift = solid_team_env_step<XT, kWalls, kTile>(g, R.b.b, R.team, R.wall, r.f, n, t, act, obs_row, rows, stride, a.team_size, mi,
                                                         a.sep, r.step0, hold, R.b.drift, R.ws, R.m, a.radius);
      if (hold) {
        R.b.holds += 1;
      } else {
        R.b.leg_used = (R.b.b.k != k0 || r.leg_steps == 0) ? 0 : R.b.leg_used + 1;
      }
      if (hold || R.b.b.k != k0) sched_set_goal(g, a.b, n, R.b.b.k, R.b.b.nwp, gs + 1);
    } else {
      (void)solid_team_env_step<XT, kWalls, kTile>(g, R.b.b, R.team, R.wall, r.f, n, t, act, obs_row, rows, stride, a.team_size, mi, a.sep,
                                                   r.step0, false, 0.f, R.ws, R.m, a.radius);
      if (R.b.b.k != k0 && R.b.b.k < R.b.b.nwp) follow_set_goal(g, r.f, n, R.b.b.k);
      R.b.leg_used = (R.b.b.k != k0 || r.leg_steps == 0) ? 0 : R.b.leg_used + 1;
    }
    return active(a, R);
  }
  // per-step path (k_goal_task_step): the team's rows are the x, y of its state rows; the robot's own row holds its pre-step
  // position until the resolve writes it (the kernel's goal_store then writes the same values again)
  template <int XT = 0>
  static __device__ __forceinline__ bool step(GoalState& g, Robot& R, const Args& a, int n, int t, const float* act,
                                              const float* obs_row) {
    const int mi = n & (a.team_size - 1);
    return step_on<XT, false>(g, R, a, n, t, act, obs_row, eval(a).st + (size_t)(n - mi) * kGoalStateFloats, kGoalStateFloats, mi);
  }
  // k_goal64_tile: post is the robot's row of the [16][2] xy block in LDS
  template <int XT = 0>
  static __device__ __forceinline__ bool step(GoalState& g, Robot& R, const Args& a, int n, int t, const float* act,
                                              const float* obs_row, float* post) {
    const int mi = n & (a.team_size - 1);
    return step_on<XT, true>(g, R, a, n, t, act, obs_row, post - 2 * mi, 2, mi);
  }
  static __device__ __forceinline__ int episodes(const Robot&) { return 0; }
  static __device__ __forceinline__ int steps(const Robot& R) { return B::steps(R.b); }
  static __device__ __forceinline__ bool recorded(const Robot&, int) { return false; }
  static __device__ __forceinline__ void finish(const Args& a, int n, const Robot& R, const GoalState& g) {
    B::finish(a.b, n, R.b, g);
    accs_store(a, n, R);
  }
  static __device__ __forceinline__ Robot load(const Args& a, int n) {
    Robot R;
    R.b = B::load(a.b, n);
    accs_load(a, n, R);
    return R;
  }
  static __device__ __forceinline__ void store(const Args& a, int n, const Robot& R) {
    B::store(a.b, n, R.b);
    accs_store(a, n, R);
  }
};

// to WallTask and to the host's choice of tile width the task is a solid one (kernels_wall.h): WallTask names the scene to it
template <class B, bool W>
struct wall_solid_inner<SolidTeamFollowTask<B, W>> : std::true_type {};
template <class B, bool W>
__device__ __forceinline__ typename SolidTeamFollowTask<B, W>::Robot& wall_solid_robot(SolidTeamFollowTask<B, W>*,
                                                                                      typename SolidTeamFollowTask<B, W>::Robot& R) {
  return R;
}

}  // namespace mobrob
