// A plan from a specification from the middle of a run (mobrob_ppo_spec_replan): the stations a robot has already visited are left
// out (todo [n], a bit set per robot, made on the host from the monitor's carried state), the plan starts at the tick t0, and with
// `partial` a robot keeps the stations it can still keep instead of losing the whole tour.
//
// The rule is goal_rules.spec_plan_tour_resume and spec_plan (state=, step0=, partial=):
//   table:     only the masks that are subsets of todo; t[{j}][j] = dep(j, t0 + d0[j]); the recurrence and dep as k_plan_tour has them
//              (strict < over ascending i, the pair (value, predecessor)).
//   selection: the lexicographic minimum of (popcount(todo) - popcount(V), t[V][j] + E[j], V, j) over the feasible entries, V = 0 an
//              entry with the total t0 + e0 and j = -1; without `partial` only V == todo is a candidate (and V = 0 where todo == 0).
//   waypoints: k_plan_tour_path's, over the tour_len legs and the goal leg.
// Region occupancy, stations, fields and the tour matrix are the kernels of kernels_plan_spec.h as they are.  Nothing here restates
// a rule of kernels_plan.h: the descent is plan_walk_step, the waypoints plan_emit / plan_close / plan_give_up / plan_result.  Every
// loop is bounded; every shuffle is executed by all 64 lanes, outside the lane-dependent loops.
#pragma once
#include "kernels_plan_spec.h"

namespace mobrob {

struct PlanTourResumeArgs {
  PlanTourArgs base;     // k_plan_tour's
  const int* todo;       // [N] the stations still to visit, bit j = station j (checked on the host: no bit >= M)
  int t0;                // the tick the plan starts at
  int partial;           // 0 / 1
  int* tour_len;         // [N] out: |V|
  int* dropped;          // [N] out: todo & ~V
};

// the real mask of the compact mask c: bit b of c is the b-th station of todo
__device__ __forceinline__ int plan_tour_deposit(int c, int todo) {
  int real = 0, b = 0;
  for (int j = 0; j < kPlanTourMax; ++j)
    if ((todo >> j) & 1) {
      if ((c >> b) & 1) real |= 1 << j;
      ++b;
    }
  return real;
}

// the selection key: (left out, total, V, j + 1) packed so that an unsigned compare is the lexicographic one.  total < 2^30.
__device__ __forceinline__ unsigned long long plan_tour_key(int left, int total, int V, int j) {
  return ((unsigned long long)left << 42) | ((unsigned long long)total << 12) | ((unsigned long long)V << 4) | (unsigned long long)(j + 1);
}

// the LDS of one robot's tour table: the kernel that owns the arrays hands them to the two helpers below
struct PlanTourTable {
  int* t;                  // [256][8] the table
  signed char* pred;       // [256][8]
  unsigned char* list;     // [256] the submasks of todo by (stations visited, value)
  int* binom;              // [9][9]
  int* Dm; int* d0; int* E; int* pos;          // [8][8], [8], [8], [8]
  int* open_c; int* close_c; int* dwell_c;     // [8] each
  int* bad; int* e0s;                          // one int each
};

// The staging of a robot's table, stated once (k_plan_tour_resume, k_plan_tour_best): the binomials, the robot's costs and ticks, the
// unconverged flag, the positions of todo's stations and the list of its submasks.  All 64 lanes call it; it ends on a barrier.
__device__ __forceinline__ void plan_tour_stage(const PlanTourArgs& a, int n, int lane, int todo, const PlanTourTable& m) {
  const int M = a.M, G = a.g.G, cells = G * G, W = kPlanTourMax + 1, L = __popc(todo);
  const int s = a.scene ? a.scene[n] : 0;
  const int* fields = a.field + (size_t)s * M * cells;
  if (lane == 0) *m.bad = 0;
  __syncthreads();
  for (int idx = lane; idx < W * W; idx += 64) {   // C(p, q), exact at every step
    const int p = idx / W, q = idx % W;
    int v = q <= p ? 1 : 0;
    for (int i = 1; i <= q && q <= p; ++i) v = v * (p - q + i) / i;
    m.binom[idx] = v;
  }
  if (lane < M * M) {
    const int v = a.matrix[s * M * M + lane];
    m.Dm[lane] = v < 0 ? kPlanAssignNone : v;
  }
  if (lane < M) {
    const float* st = a.start + (size_t)n * a.P;
    const int sc = plan_cell(a.g, st[1]) * G + plan_cell(a.g, st[0]);
    const int v = fields[(size_t)lane * cells + sc];
    m.d0[lane] = v < 0 ? kPlanAssignNone : v;
    int e = 0;
    if (a.has_goal) {
      const int ci = a.cell[s * M + lane];
      e = ci >= 0 ? a.field[(size_t)(a.S * M + a.field_of[n]) * cells + ci] : -1;
    }
    m.E[lane] = e < 0 ? kPlanAssignNone : e;
    m.open_c[lane] = a.open_c[lane]; m.close_c[lane] = a.close_c[lane]; m.dwell_c[lane] = a.dwell_c[lane];
    if (((todo >> lane) & 1) && a.sweeps[s * M + lane] < 0) *m.bad = 1;
    if (lane == 0) {
      int e0 = 0;
      if (a.has_goal) {
        if (a.sweeps[a.S * M + a.field_of[n]] < 0) *m.bad = 1;
        e0 = a.field[(size_t)(a.S * M + a.field_of[n]) * cells + sc];
      }
      *m.e0s = e0 < 0 ? kPlanAssignNone : e0;
      int b = 0;
      for (int j = 0; j < kPlanTourMax; ++j)
        if ((todo >> j) & 1) m.pos[b++] = j;
    }
  }
  __syncthreads();
  for (int c = lane; c < (1 << L); c += 64) {   // the compact masks into their places: level offset + rank within the level
    const int level = __popc(c);
    int at = 0, i = 0;
    for (int q = 0; q < level; ++q) at += m.binom[L * W + q];
    for (int p = 0; p < L; ++p)
      if ((c >> p) & 1) at += m.binom[p * W + ++i];
    m.list[at] = (unsigned char)plan_tour_deposit(c, todo);
  }
  __syncthreads();
}

// The table fill, stated once: level by level over the list, the 64 lanes on the (mask, station of todo) pairs of a level.
__device__ __forceinline__ void plan_tour_levels(const PlanTourTable& m, int lane, int L, int M, int t0) {
  const int W = kPlanTourMax + 1;
  const auto dep = [&](int j, int arr) {
    const int begin = max(arr, m.open_c[j]);
    return begin <= m.close_c[j] ? begin + m.dwell_c[j] : kPlanInf;
  };
  int first = 1;   // list[0] is the empty set
  for (int level = 1; level <= L; ++level) {
    const int cnt = m.binom[L * W + level];
    for (int idx = lane; idx < cnt * L; idx += 64) {
      const int e = idx / L, j = m.pos[idx - e * L], mask = m.list[first + e];
      if (!((mask >> j) & 1)) continue;
      const int rest = mask ^ (1 << j);
      int best = kPlanInf, via = -1;
      if (rest == 0) {
        if (m.d0[j] < kPlanAssignNone) best = dep(j, t0 + m.d0[j]);
      } else {
        for (int i = 0; i < M; ++i) {   // ascending, strict <: the lowest i of equal values
          if (!((rest >> i) & 1)) continue;
          const int ti = m.t[rest * kPlanTourMax + i], dij = m.Dm[i * M + j];
          if (ti >= kPlanInf || dij >= kPlanAssignNone) continue;
          const int v = dep(j, ti + dij);
          if (v < best) { best = v; via = i; }
        }
      }
      m.t[mask * kPlanTourMax + j] = best;
      m.pred[mask * kPlanTourMax + j] = (signed char)via;
    }
    first += cnt;
    __syncthreads();
  }
}

// A wave per robot, k_plan_tour's shape: t [256][8] and pred in LDS.  The submasks of todo are ENUMERATED: `list` holds them sorted
// by (stations visited, value) -- the rank of a compact mask among those of its popcount is its combinatorial number -- so a level
// is a contiguous run of the list and a robot with three stations left touches 8 masks, not 256.  The 64 lanes take the (mask,
// station of todo) pairs of a level; the selection is a wave-wide minimum of the packed key by xor shuffles.
__global__ __launch_bounds__(64) void k_plan_tour_resume(PlanTourResumeArgs r) {
  __shared__ int t[kPlanTourMasks * kPlanTourMax];
  __shared__ signed char pred[kPlanTourMasks * kPlanTourMax];
  __shared__ unsigned char list[kPlanTourMasks];
  __shared__ int binom[(kPlanTourMax + 1) * (kPlanTourMax + 1)];
  __shared__ int Dm[kPlanTourMax * kPlanTourMax], d0[kPlanTourMax], E[kPlanTourMax], pos[kPlanTourMax];
  __shared__ int open_c[kPlanTourMax], close_c[kPlanTourMax], dwell_c[kPlanTourMax];
  __shared__ int bad, e0s;
  const PlanTourArgs& a = r.base;
  const int n = blockIdx.x, lane = threadIdx.x, M = a.M;
  const int todo = r.todo[n] & ((1 << M) - 1), L = __popc(todo), t0 = r.t0;
  const PlanTourTable tb{t, pred, list, binom, Dm, d0, E, pos, open_c, close_c, dwell_c, &bad, &e0s};
  plan_tour_stage(a, n, lane, todo, tb);
  plan_tour_levels(tb, lane, L, M, t0);
  // the selection: every lane the minimum of its candidates, then the wave's
  const unsigned long long none = ~0ull;
  unsigned long long key = none;
  if (lane == 0 && (r.partial || L == 0) && e0s < kPlanAssignNone) key = plan_tour_key(L, t0 + e0s, 0, -1);
  const int from = r.partial ? 1 : (1 << L) - 1;   // without partial the one candidate set is todo itself, the last of the list
  for (int idx = lane + from * L; idx < (L << L); idx += 64) {
    const int e = idx / L, j = pos[idx - e * L], mask = list[e];
    if (!((mask >> j) & 1)) continue;
    const int tj = t[mask * kPlanTourMax + j];
    if (tj >= kPlanInf || E[j] >= kPlanAssignNone) continue;
    const unsigned long long k = plan_tour_key(L - __popc(mask), tj + E[j], mask, j);
    if (k < key) key = k;
  }
  for (int m = 32; m > 0; m >>= 1) {   // all 64 lanes, after the loop
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)key, m), hi = (unsigned)__shfl_xor((int)(unsigned)(key >> 32), m);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    if (other < key) key = other;
  }
  if (lane != 0) return;
  int* order = a.order + (size_t)n * M;
  int* eta = a.eta + (size_t)n * M;
  int* depart = a.depart + (size_t)n * M;
  for (int k = 0; k < M; ++k) { order[k] = -1; eta[k] = -1; depart[k] = -1; }
  if (bad || key == none) {
    a.status[n] = bad ? kPlanUnconverged : kPlanUnreachable;
    a.cost[n] = -1;
    r.tour_len[n] = 0;
    r.dropped[n] = todo;
    return;
  }
  const int V = (int)(key >> 4) & (kPlanTourMasks - 1), len = __popc(V);
  int mask = V, j = (int)(key & 15) - 1;
  for (int k = len - 1; k >= 0; --k) {
    const int i = pred[mask * kPlanTourMax + j], rest = mask ^ (1 << j);
    order[k] = j;
    depart[k] = t[mask * kPlanTourMax + j];
    eta[k] = i < 0 ? t0 + d0[j] : t[rest * kPlanTourMax + i] + Dm[i * M + j];
    mask = rest;
    j = i;
  }
  a.status[n] = kPlanned;
  a.cost[n] = (int)((key >> 12) & 0x3FFFFFFF);
  r.tour_len[n] = len;
  r.dropped[n] = todo & ~V;
}

struct PlanTourPathLegsArgs {
  PlanTourPathArgs base;   // k_plan_tour_path's
  const int* tour_len;     // [N] k_plan_tour_resume's
};

constexpr int kPlanLegLanes = 16;   // lanes a robot: at most 8 station legs and the goal leg
static_assert(kPlanTourMax + 1 <= kPlanLegLanes, "a robot's legs fit its lane group");

// the walk of one leg from the cell (ix, iy) to (tx, ty) on the field d: the waypoints at the turns go to wp from `count` on when
// Emit, and are counted either way -> the turns, -1: the leg was given up (its bound of G * G steps, or no descent)
template <bool Emit>
__device__ __forceinline__ int plan_leg_walk(const PlanGrid& g, const unsigned char* occ, const int* d, int ix, int iy, int tx, int ty,
                                             float* wp, int count, int K, int P, const float* gl) {
  const int G = g.G, cells = G * G;
  int prev = -1, steps = 0, turns = 0;
  while (ix != tx || iy != ty) {
    if (steps >= cells) return -1;
    const int dir = plan_walk_step<false>(occ, d, G, 0, 0, ix, iy, prev);
    if (dir < 0) return -1;   // not a field of this map: cannot happen after a converged field kernel
    ++steps;
    if (prev >= 0 && dir != prev) {
      if (Emit) plan_emit(wp, count + turns, K, P, g, ix, iy, gl, true);
      ++turns;
    }
    ix += plan_dx(dir); iy += plan_dy(dir);
    prev = dir;
  }
  return turns;
}

// The leg-parallel path kernel: 16 lanes a robot, 16 robots a workgroup of 256.  The start cell of leg k is known without walking
// leg k - 1 (the robot's start cell, else the anchor of order[k - 1]), so every lane walks its own leg twice: once to count, and --
// after the robot's status and the exclusive prefix of the counts have been formed across its 16 lanes by width-16 shuffles that all
// lanes execute -- once more to emit at its offset.  What a robot gets is what k_plan_tour_path gives it.
__global__ __launch_bounds__(256) void k_plan_tour_path_legs(PlanTourPathLegsArgs r) {
  const PlanTourPathArgs& a = r.base;
  const int n = blockIdx.x * (256 / kPlanLegLanes) + threadIdx.x / kPlanLegLanes, k = threadIdx.x % kPlanLegLanes;
  const bool robot = n < a.N;
  const int G = a.g.G, cells = G * G, gs = 31 - __clz(G), P = a.P, K = a.K, M = a.M;
  int status = robot ? a.status[n] : kPlanUnreachable, cost = robot ? a.cost[n] : -1;
  const bool planned = robot && status == kPlanned;
  const int len = planned ? min(max(r.tour_len[n], 0), M) : 0, legs = planned ? len + (a.has_goal ? 1 : 0) : 0;
  const bool mine = k < legs, station = k < len;
  const int nn = robot ? n : 0;   // idle lanes read robot 0's addresses and nothing behind them
  const int s = a.scene ? a.scene[nn] : 0;
  const unsigned char* occ = a.occ + (size_t)s * cells;
  const float* st = a.start + (size_t)nn * P;
  const float* gl = a.has_goal ? a.goal + (size_t)nn * P : st;   // the z of every waypoint: the goal's, else the start's
  float* wp = a.wp + (size_t)nn * K * P;
  int* order = a.order + (size_t)nn * M;
  int* swp = a.swp + (size_t)nn * M;
  int ix = 0, iy = 0, tx = 0, ty = 0;
  const int* d = a.field;
  if (mine) {
    int f, tc;
    if (station) {
      f = s * M + order[k];
      tc = a.cell[f];
    } else {
      f = a.S * M + a.field_of[n];
      tc = plan_cell(a.g, gl[1]) * G + plan_cell(a.g, gl[0]);
    }
    d = a.field + (size_t)f * cells;
    tx = tc & (G - 1); ty = tc >> gs;
    if (k == 0) {
      ix = plan_cell(a.g, st[0]); iy = plan_cell(a.g, st[1]);
    } else {
      const int fc = a.cell[s * M + order[k - 1]];
      ix = fc & (G - 1); iy = fc >> gs;
    }
  }
  // pass 1: count
  int turns = 0;
  if (mine) turns = plan_leg_walk<false>(a.g, occ, d, ix, iy, tx, ty, wp, 0, K, P, gl);
  int failed = turns < 0 ? 1 : 0, incl = mine && turns >= 0 ? turns + 1 : 0;   // + 1: the leg's end, an anchor or the goal
  for (int m = kPlanLegLanes / 2; m > 0; m >>= 1) failed |= __shfl_xor(failed, m, kPlanLegLanes);
  for (int w = 1; w < kPlanLegLanes; w <<= 1) {
    const int up = __shfl_up(incl, w, kPlanLegLanes);
    if (k >= w) incl += up;
  }
  int count = __shfl(incl, kPlanLegLanes - 1, kPlanLegLanes);   // the robot's waypoints
  const int at = incl - (mine && turns >= 0 ? turns + 1 : 0);      // where this leg's begin
  if (failed) status = kPlanUnconverged;
  // pass 2: emit
  if (mine && !failed) {
    plan_leg_walk<true>(a.g, occ, d, ix, iy, tx, ty, wp, at, K, P, gl);
    int c = at + turns;
    if (station) {
      plan_emit(wp, c, K, P, a.g, tx, ty, gl, true);
      swp[k] = c;
      ++c;
      const int dp = a.depart[(size_t)n * M + k];
      if (dp > a.eta[(size_t)n * M + k] && k + 1 < legs && c < K) {   // the next waypoint waits for the departure
        const long long rel = ((long long)dp * a.pace + 4) / 5;
        a.release[(size_t)n * K + c] = (int)min(rel, (long long)INT_MAX);
      }
    } else {
      plan_close(wp, c, K, P, gl, true);
    }
  }
  if (!robot || k != 0) return;
  if (status == kPlanUnconverged) {   // nothing was emitted: the host's zeros stand in wp and release
    count = 0;
    plan_give_up(wp, count, cost, K, P);
    for (int q = 0; q < M; ++q) { order[q] = -1; a.eta[(size_t)n * M + q] = -1; swp[q] = -1; }
  } else if (status == kPlanned && count > K) {
    status = kPlanTruncated;
  }
  if (status != kPlanned && status != kPlanTruncated) cost = -1;
  plan_result(a.nwp + n, a.count + n, a.status + n, a.cost + n, status == kPlanned || status == kPlanTruncated ? count : 0, K, status, cost);
}

}  // namespace mobrob
