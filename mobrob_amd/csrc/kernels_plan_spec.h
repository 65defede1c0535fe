// A plan from a specification (mobrob_ppo_spec_plan): avoid clauses become obstacles, reach clauses stations; per robot the order
// of the stations and the stitched waypoints, for all robots in one call.
//
// The rule, stated once in array form in mobrob_amd/envs/goal_rules.py (spec_plan_occupancy, spec_plan_stations, spec_plan_tour,
// spec_plan):
//   blocked:   k_plan_occupancy's map of the walls and hazards (or a zeroed one), OR-ed with the avoid regions: a cell is blocked when
//              spec_margin(centre, region r) >= -inflate for a region r of an avoid range, r below the scene's count.  Equality blocks.
//   anchor:    per scene and station, over the unblocked cells, m(c) = the largest inside margin of the station's range by explicit > in
//              ascending order (spec_predicate); the best cell has the largest spec key of m, the lowest cell index on a tie; it is the
//              anchor where m > 0, else the anchor is -1.
//   costs:     one k_plan_field field per (scene, station) -- k_plan_station writes the anchor into the field list itself, so the fields
//              of all stations and goals are ONE launch -- and per distinct (scene, goal cell); matrix[s][i][j] = field_j[anchor_i].
//   order:     Held-Karp in ticks (5 orthogonal, 7 diagonal).  dep(j, arr) = max(arr, open[j]) + dwell[j], feasible iff
//              max(arr, open[j]) <= close[j]; t[{j}][j] = dep(j, d0[j]); t[mask + j][j] = min over feasible i in mask of
//              dep(j, t[mask][i] + D[i][j]), the minimum of the pair (value, i); the end j minimises (t[full][j] + E[j], j).
//   waypoints: the legs in tour order, then the goal leg; every leg descends its target's field with plan_step (the previous direction
//              forgotten at the start of a leg) and emits with plan_emit / plan_close what k_plan_path emits.
// Nothing here restates a rule of kernels_plan.h or kernels_spec.h: the cell centre is plan_centre, the margin spec_margin, the
// descent plan_walk_step, the waypoints plan_emit / plan_close / plan_give_up / plan_result.  Every loop is bounded.
#pragma once
#include "kernels_plan.h"
#include "kernels_spec.h"

namespace mobrob {

constexpr int kPlanTourMax = 8;               // stations: 256 subsets, the tour table of one robot is 8 KB + 2 KB of LDS
constexpr int kPlanTourTicksMax = 1 << 24;    // every open, close and dwell: 8 legs of them stay below 2^30
constexpr int kPlanTourMasks = 1 << kPlanTourMax;

// the total order on float bits (goal_rules.spec_key): -0.0 < +0.0 and every bit pattern has its place
__device__ __forceinline__ int plan_spec_key(float v) {
  const int i = __float_as_int(v);
  return i ^ ((i >> 31) & 0x7fffffff);
}

// a scene's regions into LDS: rows [R][4] then kinds [R]; the caller's barrier follows
__device__ __forceinline__ void plan_spec_stage(float* rows, int* kinds, const float* regions, const int* gkinds, int s, int R, int count,
                                                int threads) {
  for (int i = threadIdx.x; i < 4 * count; i += threads) rows[i] = regions[(size_t)s * R * 4 + i];
  for (int i = threadIdx.x; i < count; i += threads) kinds[i] = gkinds[(size_t)s * R + i];
}

struct PlanRegionOccArgs {
  PlanGrid g;
  const float* regions;   // [S][R][4]
  const int* kinds;       // [S][R]
  const int* nreg;        // [S]
  int R;
  int n_avoid;
  int lo[kSpecClausesMax], hi[kSpecClausesMax];   // the avoid ranges
  unsigned char* occ;     // [S][G][G] in / out: k_plan_occupancy's map or zeros; 1 is OR-ed in
};

// grid (cdiv(G * G, 256), S), 256 threads: a thread per scene and cell, the scene's regions staged in LDS
__global__ __launch_bounds__(256) void k_plan_region_occupancy(PlanRegionOccArgs a) {
  __shared__ float rows[kSpecRegionsMax * 4];
  __shared__ int kinds[kSpecRegionsMax];
  const int s = blockIdx.y, G = a.g.G;
  const int count = min(a.nreg[s], min(a.R, kSpecRegionsMax));
  plan_spec_stage(rows, kinds, a.regions, a.kinds, s, a.R, count, 256);
  __syncthreads();
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= G * G) return;
  const float px = plan_centre(a.g, c % G), py = plan_centre(a.g, c / G), edge = -a.g.inflate;
  bool blocked = false;
  for (int v = 0; v < a.n_avoid; ++v)
    for (int r = a.lo[v]; r < min(a.hi[v], count); ++r)
      if (spec_margin(px, py, rows[4 * r], rows[4 * r + 1], rows[4 * r + 2], rows[4 * r + 3], kinds[r]) >= edge) blocked = true;
  if (blocked) a.occ[(size_t)s * G * G + c] = 1;
}

struct PlanStationArgs {
  PlanGrid g;
  const float* regions;   // [S][R][4]
  const int* kinds;       // [S][R]
  const int* nreg;        // [S]
  int R, M;
  int lo[kPlanTourMax], hi[kPlanTourMax];   // the stations' ranges
  const unsigned char* occ;   // [S][G][G]
  int* cell;              // [S][M] out: the anchor, -1 none
  float* margin;          // [S][M] out: the best unblocked cell's margin, -inf without one
  int* field_goal;        // [S][M] out: the anchor again, as the goal cell of the station's field (k_plan_field's list)
};

// grid (M, S), 256 threads: a workgroup per (scene, station), an arg-max over the G * G cells on the pair (key, -cell)
__global__ __launch_bounds__(256) void k_plan_station(PlanStationArgs a) {
  __shared__ float rows[kSpecRegionsMax * 4];
  __shared__ int kinds[kSpecRegionsMax];
  __shared__ int rkey[256], rcell[256];
  __shared__ float rval[256];
  const int j = blockIdx.x, s = blockIdx.y, G = a.g.G, cells = G * G, tid = threadIdx.x;
  const int count = min(a.nreg[s], min(a.R, kSpecRegionsMax));
  plan_spec_stage(rows, kinds, a.regions, a.kinds, s, a.R, count, 256);
  __syncthreads();
  const int lo = a.lo[j], hi = min(a.hi[j], count);
  const unsigned char* occ = a.occ + (size_t)s * cells;
  int bkey = INT_MIN, bcell = INT_MAX;
  float bval = -__builtin_inff();
  for (int c = tid; c < cells; c += 256) {   // ascending per thread: of equal keys the first, the lowest cell, is kept
    if (occ[c]) continue;
    const float px = plan_centre(a.g, c % G), py = plan_centre(a.g, c / G);
    float u = -__builtin_inff();
    for (int r = lo; r < hi; ++r) {
      const float m = spec_margin(px, py, rows[4 * r], rows[4 * r + 1], rows[4 * r + 2], rows[4 * r + 3], kinds[r]);
      if (m > u) u = m;
    }
    const int key = plan_spec_key(u);
    if (bcell == INT_MAX || key > bkey) { bkey = key; bcell = c; bval = u; }
  }
  rkey[tid] = bkey; rcell[tid] = bcell; rval[tid] = bval;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
      const int ok = rkey[tid + w], oc = rcell[tid + w];
      const bool mine = rcell[tid] != INT_MAX, theirs = oc != INT_MAX;
      if (theirs && (!mine || ok > rkey[tid] || (ok == rkey[tid] && oc < rcell[tid]))) {
        rkey[tid] = ok; rcell[tid] = oc; rval[tid] = rval[tid + w];
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool any = rcell[0] != INT_MAX;
    const float m = any ? rval[0] : -__builtin_inff();
    const int anchor = any && m > 0.f ? rcell[0] : -1;
    a.cell[s * a.M + j] = anchor;
    a.margin[s * a.M + j] = m;
    a.field_goal[s * a.M + j] = anchor;   // -1: k_plan_field finds no goal and the field is all -1
  }
}

struct PlanTourMatrixArgs {
  int S, M, cells;
  const int* cell;     // [S][M]
  const int* field;    // [S * M + Fg][cells]
  int* matrix;         // [S][M][M] out: field_j at the anchor of i, -1 none
};

// a thread per (scene, i, j)
__global__ __launch_bounds__(256) void k_plan_tour_matrix(PlanTourMatrixArgs a) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.S * a.M * a.M) return;
  const int j = idx % a.M, i = (idx / a.M) % a.M, s = idx / (a.M * a.M);
  const int ci = a.cell[s * a.M + i];
  a.matrix[idx] = ci >= 0 ? a.field[(size_t)(s * a.M + j) * a.cells + ci] : -1;
}

struct PlanTourArgs {
  PlanGrid g;
  int N, P, M, S;
  int has_goal;
  const float* start;       // [N][P]
  const int* scene;         // [N] or null
  const int* field_of;      // [N] the robot's goal field, counted from S * M (null without a goal)
  const int* cell;          // [S][M]
  const int* matrix;        // [S][M][M]
  const int* field;         // [S * M + Fg][G][G]
  const int* sweeps;        // [S * M + Fg]
  int open_c[kPlanTourMax], close_c[kPlanTourMax], dwell_c[kPlanTourMax];
  int* status;              // [N] out: 0 a tour, 1 none, 3 a field of the robot's did not converge
  int* cost;                // [N] out: ticks at the end, -1
  int* order;               // [N][M] out
  int* eta;                 // [N][M] out
  int* depart;              // [N][M] out
};

// A wave per robot: the tour table t [256][8] and pred in LDS, level-synchronous by the number of stations visited, the 64 lanes
// over the (mask, j) pairs; the backtrack on lane 0.
__global__ __launch_bounds__(64) void k_plan_tour(PlanTourArgs a) {
  __shared__ int t[kPlanTourMasks * kPlanTourMax];
  __shared__ signed char pred[kPlanTourMasks * kPlanTourMax];
  __shared__ int Dm[kPlanTourMax * kPlanTourMax], d0[kPlanTourMax], E[kPlanTourMax];
  __shared__ int open_c[kPlanTourMax], close_c[kPlanTourMax], dwell_c[kPlanTourMax];
  __shared__ int bad;
  const int n = blockIdx.x, lane = threadIdx.x, M = a.M, G = a.g.G, cells = G * G;
  const int s = a.scene ? a.scene[n] : 0;
  const int* fields = a.field + (size_t)s * M * cells;
  if (lane == 0) bad = 0;
  __syncthreads();
  if (lane < M * M) {
    const int v = a.matrix[s * M * M + lane];
    Dm[lane] = v < 0 ? kPlanAssignNone : v;
  }
  if (lane < M) {
    const float* st = a.start + (size_t)n * a.P;
    const int sc = plan_cell(a.g, st[1]) * G + plan_cell(a.g, st[0]);
    const int v = fields[(size_t)lane * cells + sc];
    d0[lane] = v < 0 ? kPlanAssignNone : v;
    int e = 0;
    if (a.has_goal) {
      const int ci = a.cell[s * M + lane];
      e = ci >= 0 ? a.field[(size_t)(a.S * M + a.field_of[n]) * cells + ci] : -1;
    }
    E[lane] = e < 0 ? kPlanAssignNone : e;
    open_c[lane] = a.open_c[lane]; close_c[lane] = a.close_c[lane]; dwell_c[lane] = a.dwell_c[lane];
    if (a.sweeps[s * M + lane] < 0) bad = 1;
    if (lane == 0 && a.has_goal && a.sweeps[a.S * M + a.field_of[n]] < 0) bad = 1;
  }
  __syncthreads();
  const auto dep = [&](int j, int arr) {
    const int begin = max(arr, open_c[j]);
    return begin <= close_c[j] ? begin + dwell_c[j] : kPlanInf;
  };
  for (int level = 1; level <= M; ++level) {
    for (int idx = lane; idx < (kPlanTourMax << M); idx += 64) {
      const int mask = idx >> 3, j = idx & 7;
      if (j >= M || __popc(mask) != level || !((mask >> j) & 1)) continue;
      const int rest = mask ^ (1 << j);
      int best = kPlanInf, via = -1;
      if (rest == 0) {
        if (d0[j] < kPlanAssignNone) best = dep(j, d0[j]);
      } else {
        for (int i = 0; i < M; ++i) {   // ascending, strict <: the lowest i of equal values
          if (!((rest >> i) & 1)) continue;
          const int ti = t[rest * kPlanTourMax + i], dij = Dm[i * M + j];
          if (ti >= kPlanInf || dij >= kPlanAssignNone) continue;
          const int v = dep(j, ti + dij);
          if (v < best) { best = v; via = i; }
        }
      }
      t[idx] = best;
      pred[idx] = (signed char)via;
    }
    __syncthreads();
  }
  if (lane != 0) return;
  const int full = (1 << M) - 1;
  int cost = kPlanInf, last = -1;
  for (int j = 0; j < M; ++j) {
    const int tj = t[full * kPlanTourMax + j];
    if (tj >= kPlanInf || E[j] >= kPlanAssignNone) continue;
    if (tj + E[j] < cost) { cost = tj + E[j]; last = j; }
  }
  int* order = a.order + (size_t)n * M;
  int* eta = a.eta + (size_t)n * M;
  int* depart = a.depart + (size_t)n * M;
  if (bad || last < 0) {
    for (int k = 0; k < M; ++k) { order[k] = -1; eta[k] = -1; depart[k] = -1; }
    a.status[n] = bad ? kPlanUnconverged : kPlanUnreachable;
    a.cost[n] = -1;
    return;
  }
  int mask = full, j = last;
  for (int k = M - 1; k >= 0; --k) {
    const int i = pred[mask * kPlanTourMax + j], rest = mask ^ (1 << j);
    order[k] = j;
    depart[k] = t[mask * kPlanTourMax + j];
    eta[k] = i < 0 ? d0[j] : t[rest * kPlanTourMax + i] + Dm[i * M + j];
    mask = rest;
    j = i;
  }
  a.status[n] = kPlanned;
  a.cost[n] = cost;
}

struct PlanTourPathArgs {
  PlanGrid g;
  int N, K, P, M, S;
  int has_goal, pace;
  const float* start;         // [N][P]
  const float* goal;          // [N][P] (null without a goal)
  const int* scene;           // [N] or null
  const int* field_of;        // [N] (null without a goal)
  const int* cell;            // [S][M]
  const unsigned char* occ;   // [S][G][G]
  const int* field;           // [S * M + Fg][G][G]
  const int* depart;          // [N][M] k_plan_tour's
  int* order;                 // [N][M] k_plan_tour's; -1 where the walk is given up
  int* eta;                   // [N][M] likewise
  float* wp;                  // [N][K][P] out (zeroed by the host)
  int* nwp;                   // [N] out
  int* count;                 // [N] out
  int* status;                // [N] in: k_plan_tour's; out: the plan's
  int* cost;                  // [N] in / out
  int* swp;                   // [N][M] out: the anchor waypoint of each position (-1 from the host)
  int* release;               // [N][K] out (zeroed by the host)
};

// a thread per robot: the legs in turn, each at most G * G steps (status 3 beyond)
__global__ __launch_bounds__(256) void k_plan_tour_path(PlanTourPathArgs a) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= a.N) return;
  const int G = a.g.G, cells = G * G, gs = 31 - __clz(G), P = a.P, K = a.K, M = a.M;
  int status = a.status[n], cost = a.cost[n], count = 0;
  if (status != kPlanned) {
    plan_result(a.nwp + n, a.count + n, a.status + n, a.cost + n, 0, K, status, -1);
    return;
  }
  const int s = a.scene ? a.scene[n] : 0;
  const unsigned char* occ = a.occ + (size_t)s * cells;
  const float* st = a.start + (size_t)n * P;
  const float* gl = a.has_goal ? a.goal + (size_t)n * P : st;   // the z of every waypoint: the goal's, else the start's
  float* wp = a.wp + (size_t)n * K * P;
  int* order = a.order + (size_t)n * M;
  int* swp = a.swp + (size_t)n * M;
  int ix = plan_cell(a.g, st[0]), iy = plan_cell(a.g, st[1]);
  const int legs = M + (a.has_goal ? 1 : 0);
  for (int k = 0; k < legs && status == kPlanned; ++k) {
    const bool station = k < M;
    int f, tc;
    if (station) {
      f = s * M + order[k];
      tc = a.cell[f];
    } else {
      f = a.S * M + a.field_of[n];
      tc = plan_cell(a.g, gl[1]) * G + plan_cell(a.g, gl[0]);
    }
    const int* d = a.field + (size_t)f * cells;
    const int tx = tc & (G - 1), ty = tc >> gs;
    int prev = -1, steps = 0;
    while (ix != tx || iy != ty) {
      if (steps >= cells) { status = kPlanUnconverged; break; }
      const int dir = plan_walk_step<false>(occ, d, G, 0, 0, ix, iy, prev);
      if (dir < 0) { status = kPlanUnconverged; break; }   // not a field of this map: cannot happen after a converged field kernel
      ++steps;
      if (prev >= 0 && dir != prev) {
        plan_emit(wp, count, K, P, a.g, ix, iy, gl, true);
        ++count;
      }
      ix += plan_dx(dir); iy += plan_dy(dir);
      prev = dir;
    }
    if (status != kPlanned) break;
    if (station) {
      plan_emit(wp, count, K, P, a.g, tx, ty, gl, true);
      swp[k] = count;
      ++count;
      const int dp = a.depart[(size_t)n * M + k];
      if (dp > a.eta[(size_t)n * M + k] && k + 1 < legs && count < K) {   // the next waypoint waits for the departure
        const long long rel = ((long long)dp * a.pace + 4) / 5;
        a.release[(size_t)n * K + count] = (int)min(rel, (long long)INT_MAX);
      }
    } else {
      plan_close(wp, count, K, P, gl, true);
    }
  }
  if (status == kPlanUnconverged) {
    plan_give_up(wp, count, cost, K, P);
    for (int k = 0; k < K; ++k) a.release[(size_t)n * K + k] = 0;
    for (int k = 0; k < M; ++k) { order[k] = -1; a.eta[(size_t)n * M + k] = -1; swp[k] = -1; }
  } else if (count > K) {
    status = kPlanTruncated;
  }
  plan_result(a.nwp + n, a.count + n, a.status + n, a.cost + n, count, K, status, cost);
}

}  // namespace mobrob
