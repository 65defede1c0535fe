// A team shares the stations of a specification (mobrob_ppo_spec_plan_share): every station of the team's set T is allotted to one
// member, the team done as early as possible ("makespan") or with the least total ("sum").
//
// The rule is goal_rules.spec_plan_best, spec_plan_share and spec_plan (share=, objective=):
//   best:      best[r][V] = min over the feasible j of V of t[V][j] + E[j], t the tour table of kernels_plan_spec_resume.h over the
//              subsets of T; best[r][0] = t0 + e0; kPlanInf where nothing is feasible and for every V that is no subset of T.
//   primary:   f[0][U] = best[0][U]; f[k][U] = min over the V in U of max (or +) of f[k - 1][U \ V] and best[k][V].
//   covered:   C = T, or with `partial` the lexicographic minimum of (popcount(T) - popcount(U), f[size - 1][U], U) over the feasible U.
//   allotment: the same pass with + under cap = f[size - 1][C] on every member's own cost ("sum": the primary pass is this pass),
//              V ascending and compared by strict <; choice[k][U] = that V; the backtrack from (size - 1, C), member 0 the rest.
// The members' tours are then k_plan_tour_resume's with todo = share and partial off, and k_plan_tour_path_legs; between the two
// k_plan_team_void gives the members of a team without a feasible allotment the outputs the rule gives them.
// Sums are 32-bit unsigned here: a member's cost is below 2^28 (the host's bounds on ticks and t0), sixteen of them below 2^32 - 1,
// which is kPlanShareNone, "no feasible split".  Every loop is bounded; every shuffle is executed by all 64 lanes, outside the
// lane-dependent loops.
#pragma once
#include "kernels_plan_spec_resume.h"

namespace mobrob {

constexpr unsigned kPlanShareNone = 0xFFFFFFFFu;   // kPlanTeamMax (kernels_plan.h) members a team

struct PlanTourBestArgs {
  PlanTourArgs base;   // k_plan_tour's (its outputs are not written)
  const int* team;     // [N] T: the stations the robot's team still has to visit (the same for every member)
  int t0;              // the tick the plan starts at
  int* best;           // [N][256] out
  int* unconv;         // [N] out: 1 where a field this robot's table reads hit its sweep bound (best is then kPlanInf throughout)
};

// A wave per robot, k_plan_tour_resume's shape and table (plan_tour_stage, plan_tour_levels) over the subsets of T; then the lanes
// take the 256 masks, four each.
__global__ __launch_bounds__(64) void k_plan_tour_best(PlanTourBestArgs r) {
  __shared__ int t[kPlanTourMasks * kPlanTourMax];
  __shared__ signed char pred[kPlanTourMasks * kPlanTourMax];
  __shared__ unsigned char list[kPlanTourMasks];
  __shared__ int binom[(kPlanTourMax + 1) * (kPlanTourMax + 1)];
  __shared__ int Dm[kPlanTourMax * kPlanTourMax], d0[kPlanTourMax], E[kPlanTourMax], pos[kPlanTourMax];
  __shared__ int open_c[kPlanTourMax], close_c[kPlanTourMax], dwell_c[kPlanTourMax];
  __shared__ int bad, e0s;
  const PlanTourArgs& a = r.base;
  const int n = blockIdx.x, lane = threadIdx.x, M = a.M;
  const int T = r.team[n] & ((1 << M) - 1), L = __popc(T), t0 = r.t0;
  const PlanTourTable tb{t, pred, list, binom, Dm, d0, E, pos, open_c, close_c, dwell_c, &bad, &e0s};
  plan_tour_stage(a, n, lane, T, tb);
  plan_tour_levels(tb, lane, L, M, t0);
  int* out = r.best + (size_t)n * kPlanTourMasks;
  for (int V = lane; V < kPlanTourMasks; V += 64) {
    int v = kPlanInf;
    if (!bad && (V & ~T) == 0) {
      if (V == 0) {
        if (e0s < kPlanAssignNone) v = t0 + e0s;
      } else {
        for (int j = 0; j < M; ++j) {
          if (!((V >> j) & 1)) continue;
          const int tj = t[V * kPlanTourMax + j];
          if (tj >= kPlanInf || E[j] >= kPlanAssignNone) continue;
          v = min(v, tj + E[j]);
        }
      }
    }
    out[V] = v;
  }
  if (lane == 0) r.unconv[n] = bad;
}

struct PlanTeamShareArgs {
  int size, M, objective, partial;   // objective: 0 makespan, 1 sum
  const int* best;                   // [N][256] k_plan_tour_best's
  const int* team;                   // [N] T
  int* share;                        // [N] out: the member's stations
  int* cover;                        // [N / size] out: C (0: no feasible allotment)
  int* dropped;                      // [N / size] out: T & ~C (T: no feasible allotment)
  int* makespan;                     // [N / size] out: the largest member cost, -1
  long long* total;                  // [N / size] out: the sum of the member costs, -1
};

// One pass of the partition DP, stated once (the primary pass and the allotment are two calls): member 0's row, then the members
// 1 .. size - 1; the 64 lanes take the U's, four each, and enumerate the submasks of their U ascending, V = (V - U) & U, at most 256
// of them; one barrier a member.  A member's own cost above `cap` is no term (kPlanShareNone: no cap).
// -> the row of the last member (one of the two rolling rows)
__device__ __forceinline__ const unsigned* plan_share_pass(const int* best, unsigned* rows, unsigned char* choice, int lane, int size, int T,
                                                           bool add, unsigned cap) {
  unsigned* cur = rows;
  unsigned* nxt = rows + kPlanTourMasks;
  for (int U = lane; U < kPlanTourMasks; U += 64) {   // member 0
    const int b = best[U];
    cur[U] = b < kPlanInf && (unsigned)b <= cap ? (unsigned)b : kPlanShareNone;
  }
  __syncthreads();
  for (int k = 1; k < size; ++k) {
    const int* own = best + k * kPlanTourMasks;
    for (int U = lane; U < kPlanTourMasks; U += 64) {
      unsigned low = kPlanShareNone;
      int pick = 0;
      if ((U & ~T) == 0) {
        int V = 0;
        for (int q = 0; q < kPlanTourMasks; ++q) {   // ascending, strict <: the lowest V of equal values
          const int b = own[V];
          const unsigned prev = cur[U ^ V];
          if (b < kPlanInf && (unsigned)b <= cap && prev != kPlanShareNone) {
            const unsigned v = add ? prev + (unsigned)b : max(prev, (unsigned)b);
            if (v < low) { low = v; pick = V; }
          }
          V = (V - U) & U;
          if (V == 0) break;
        }
      }
      nxt[U] = low;
      choice[k * kPlanTourMasks + U] = (unsigned char)pick;
    }
    __syncthreads();
    unsigned* sw = cur; cur = nxt; nxt = sw;
  }
  return cur;
}

// A workgroup of one wave per team.  LDS: best [size][256] (16 KB at size 16), the two rolling rows (2 KB), choice [size][256] bytes.
__global__ __launch_bounds__(64) void k_plan_team_share(PlanTeamShareArgs a) {
  __shared__ int best[kPlanTeamMax * kPlanTourMasks];
  __shared__ unsigned rows[2 * kPlanTourMasks];
  __shared__ unsigned char choice[kPlanTeamMax * kPlanTourMasks];
  const int team = blockIdx.x, lane = threadIdx.x, size = a.size;
  const int T = a.team[team * size] & ((1 << a.M) - 1), L = __popc(T);
  const int* src = a.best + (size_t)team * size * kPlanTourMasks;
  for (int idx = lane; idx < size * kPlanTourMasks; idx += 64) best[idx] = src[idx];
  __syncthreads();
  const bool add = a.objective == 1;
  const unsigned* f = plan_share_pass(best, rows, choice, lane, size, T, add, kPlanShareNone);
  // the covered set: the wave-wide minimum of (left out, f, U); without partial the one candidate is T itself
  const unsigned long long none = ~0ull;
  unsigned long long key = none;
  for (int U = lane; U < kPlanTourMasks; U += 64) {
    if (a.partial ? (U & ~T) != 0 : U != T) continue;
    if (f[U] == kPlanShareNone) continue;
    const unsigned long long k = ((unsigned long long)(L - __popc(U)) << 40) | ((unsigned long long)f[U] << 8) | (unsigned long long)U;
    if (k < key) key = k;
  }
  for (int m = 32; m > 0; m >>= 1) {   // all 64 lanes, after the loop
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, m), hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), m);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    if (other < key) key = other;
  }
  const bool feasible = key != none;   // the same in every lane
  const int C = feasible ? (int)(key & 0xFF) : 0;
  if (feasible && !add) {              // "makespan": the allotment is the sum pass under the cap
    __syncthreads();                   // every lane has read its f before the rows are written again
    plan_share_pass(best, rows, choice, lane, size, T, true, (unsigned)((key >> 8) & 0xFFFFFFFFu));
  }
  if (lane != 0) return;
  int* share = a.share + team * size;
  if (!feasible) {
    for (int k = 0; k < size; ++k) share[k] = 0;
    a.cover[team] = 0; a.dropped[team] = T; a.makespan[team] = -1; a.total[team] = -1;
    return;
  }
  int U = C, most = 0;
  long long sum = 0;
  for (int k = size - 1; k >= 0; --k) {
    const int V = k > 0 ? choice[k * kPlanTourMasks + U] : U;
    const int c = best[k * kPlanTourMasks + V];
    share[k] = V;
    most = max(most, c);
    sum += c;
    U ^= V;
  }
  a.cover[team] = C; a.dropped[team] = T & ~C; a.makespan[team] = most; a.total[team] = sum;
}

struct PlanTeamVoidArgs {
  int N, M, size;
  const int* team;       // [N] T
  const int* makespan;   // [N / size] k_plan_team_share's: < 0, the team has no feasible allotment
  const int* tdropped;   // [N / size] k_plan_team_share's
  const int* unconv;     // [N] k_plan_tour_best's
  int* status; int* cost; int* order; int* eta; int* depart; int* tour_len; int* dropped;   // k_plan_tour_resume's outputs
};

// A thread per robot, between k_plan_tour_resume and k_plan_tour_path_legs.  A member of a team without a feasible allotment gets
// what the rule gives it: UNREACHABLE (UNCONVERGED where a mate's table read a field that hit its sweep bound), cost -1, no tour,
// dropped = T -- the resume kernel planned its goal leg, for share = 0.  A team of one is the robot: its dropped is the team's.
__global__ __launch_bounds__(256) void k_plan_team_void(PlanTeamVoidArgs a) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= a.N) return;
  const int team = n / a.size;
  if (a.makespan[team] >= 0) {
    if (a.size == 1) a.dropped[n] = a.tdropped[team];
    return;
  }
  int bad = 0;
  for (int k = 0; k < a.size; ++k) bad |= a.unconv[team * a.size + k];
  a.status[n] = bad ? kPlanUnconverged : kPlanUnreachable;
  a.cost[n] = -1;
  a.tour_len[n] = 0;
  a.dropped[n] = a.team[n];
  for (int k = 0; k < a.M; ++k) { a.order[(size_t)n * a.M + k] = -1; a.eta[(size_t)n * a.M + k] = -1; a.depart[(size_t)n * a.M + k] = -1; }
}

}  // namespace mobrob
