// Grid planner (mobrob_ppo_plan_grid and the six entry points built on it): walls and hazards to waypoints, for all robots in one call.
//
// The rule, stated once in array form in mobrob_amd/envs/goal_rules.py (GridSpec, grid_occupancy, grid_field, grid_path): a grid of
// G x G cells (G = 32, 64, 128) over [-extent, extent]^2, x and y only.  The host hands down extent, h = 2 extent / G and inv_h =
// G / (2 extent) as floats; in float, every operation rounded on its own, no fma:
//   cell of x:   clamp(floor((x + extent) * inv_h), 0, G - 1)          centre of cell i:   -extent + (i + 0.5) * h
//   blocked:     wall_sdf(centre, wall) <= inflate for a wall of the scene (kernels_wall.h: the walls' own arithmetic), or
//                sqrt(dx^2 + dy^2) <= radius_k + inflate for a hazard k of the scene (team_partial's distance).  Equality blocks.
//   field:       the cost-to-go to the goal cell over eight-connected moves, 5 orthogonal and 7 diagonal, a diagonal only where both
//                orthogonal cells at the corner are free; -1: blocked or unreachable.  It is the unique fixed point of
//                d[c] = min(d[nb] + w), d[goal] = 0, so the order of the relaxations does not show in it.
//   path:        from the start's cell to a neighbour with d[nb] + w == d[c], the previous direction first, else the lowest of E, N,
//                W, S, NE, NW, SW, SE; a cell's centre is a waypoint where the direction changes; the last waypoint is the goal.
// A loop that runs into its bound reports status 3; nothing here can spin.
//
// Every rule is one device function, and every kernel calls it:
//   plan_centre_blocked   the wall and hazard test of a cell centre          (k_plan_occupancy, k_plan_occupancy_time)
//   plan_moves            the move mask over a "cell is free" predicate      (every field and every walk)
//   plan_tail             the in-place relaxation to a tested fixed point    (k_plan_field, k_plan_field_time, plan_team_field)
//   plan_jacobi           a cell of layer t from layer t + 1                 (k_plan_field_time, plan_team_field)
//   plan_step             the descent step                                   (plan_walk_step: plan_path, plan_smooth; the team walks)
//   plan_los              the supercover sight line over a "cell is hidden" predicate   (plan_smooth, plan_team_smooth_legs)
//   plan_emit, plan_close, plan_give_up, plan_result   a robot's waypoints and outputs  (every walk and window body)
//   plan_path<Time>, plan_smooth<Time>   the bodies of k_plan_path / k_plan_path_time and k_plan_smooth / k_plan_smooth_time
//   plan_team_field<Reserved>   a member's field, over where "reserved" comes from      (k_plan_team, k_plan_team_rounds, k_plan_team_smooth)
//   plan_team_member      field, walk and stamps of one member               (k_plan_team, k_plan_team_rounds)
#pragma once
#include "kernels_wall.h"

namespace mobrob {

constexpr int kPlanInf = 0x3FFFFFFF;   // "no path yet" inside a field kernel (any sum of a path's costs stays far below it)
constexpr int kPlanWait = 4;           // cost of a wait in a time field: cheaper than a move
constexpr short kPlanNeverBlocked = 32767;   // in a next-blocked table: "in no layer" (kPlanLayersMax is 256: a short holds every layer)
constexpr int kPlanFieldThreads = 1024;
// status of a robot's plan
constexpr int kPlanned = 0, kPlanUnreachable = 1, kPlanTruncated = 2, kPlanUnconverged = 3;

struct PlanGrid {
  int G;                   // cells per side, a power of two: cell c is (c & (G - 1), c >> log2 G)
  float extent, h, inv_h;  // the host's floats
  float inflate;
};

__device__ __forceinline__ int plan_cell(const PlanGrid& g, float x) {
  const float c = floorf(__fmul_rn(__fadd_rn(x, g.extent), g.inv_h));
  return (int)fminf(fmaxf(c, 0.f), (float)(g.G - 1));
}
__device__ __forceinline__ float plan_centre(const PlanGrid& g, int i) {
  return __fadd_rn(-g.extent, rounded(__fmul_rn(__fadd_rn((float)i, 0.5f), g.h)));
}
// move k of E, N, W, S, NE, NW, SW, SE, and its cost
__device__ __forceinline__ int plan_dx(int k) { return k == 0 || k == 4 || k == 7 ? 1 : (k == 1 || k == 3 ? 0 : -1); }
__device__ __forceinline__ int plan_dy(int k) { return k == 1 || k == 4 || k == 5 ? 1 : (k == 0 || k == 2 ? 0 : -1); }
__device__ __forceinline__ int plan_w(int k) { return k < 4 ? 5 : 7; }

// "cell c is free" on a map that is nonzero where a cell is blocked: occupancy bytes, or a layer's map in LDS
template <class Occ>
__device__ __forceinline__ auto plan_unblocked(const Occ* occ) {
  return [occ](int c) { return !occ[c]; };
}
template <class Occ>
__device__ __forceinline__ auto plan_blocked(const Occ* occ) {
  return [occ](int c) { return occ[c] != 0; };
}

// the moves a robot in the free cell (ix, iy) may make, bit k for move k: target in the grid and free, a diagonal only with both
// orthogonal cells at the corner free
template <class Free>
__device__ __forceinline__ unsigned plan_moves(Free free, int G, int ix, int iy) {
  const int c = iy * G + ix;
  unsigned free4 = 0;   // E, N, W, S
  if (ix + 1 < G && free(c + 1)) free4 |= 1u;
  if (iy + 1 < G && free(c + G)) free4 |= 2u;
  if (ix > 0 && free(c - 1)) free4 |= 4u;
  if (iy > 0 && free(c - G)) free4 |= 8u;
  unsigned m = free4;
  if ((free4 & 3u) == 3u && free(c + G + 1)) m |= 16u;     // NE: E and N free
  if ((free4 & 6u) == 6u && free(c + G - 1)) m |= 32u;     // NW: N and W
  if ((free4 & 12u) == 12u && free(c - G - 1)) m |= 64u;   // SW: W and S
  if ((free4 & 9u) == 9u && free(c - G + 1)) m |= 128u;    // SE: S and E
  return m;
}

// The descent step of every walk, from the cell c whose value is dc into the layer dn (the same layer on a static field or a tail,
// the next layer in time) over the moves m: to a neighbour with dn[nb] + w == dc, the previous direction first, else the lowest
// index, else -- where `wait` allows it -- the wait (8); -1: none (dn is not a cost-to-go field of these moves).  A neighbour
// qualifies with 0 <= v < kPlanInf: a team's scratch field holds kPlanInf in free cells without a path; on a field that holds only -1
// or finite costs the upper test is vacuous.
__device__ __forceinline__ int plan_step(unsigned m, int dc, const int* dn, int G, int c, int prev, bool wait) {
  const auto fits = [dc](int v, int w) { return v >= 0 && v < kPlanInf && v + w == dc; };
  int dir = -1;
  for (int k = 7; k >= 0; --k)   // descending: the lowest qualifying index is kept
    if ((m & (1u << k)) && fits(dn[c + plan_dy(k) * G + plan_dx(k)], plan_w(k))) dir = k;
  if (prev >= 0 && (m & (1u << prev)) && fits(dn[c + plan_dy(prev) * G + plan_dx(prev)], plan_w(prev))) dir = prev;   // the previous direction first
  if (dir < 0 && wait && fits(dn[c], kPlanWait)) dir = 8;   // the wait last
  return dir;
}

// Action number t of the walk of goal_rules.grid_walk_time from the cell (ix, iy), on the layer maps occ [T + 1][G][G] and their time
// field d: while t < T it descends from d_t to d_{t + 1} over layer t's map and may wait; from t = T on it is goal_rules.grid_walk on
// the tail.  Without Time the map and the field are static ones: goal_rules.grid_walk, and neither T nor t is looked at.
template <bool Time>
__device__ __forceinline__ int plan_walk_step(const unsigned char* occ, const int* d, int G, int T, int t, int ix, int iy, int prev) {
  const int cells = G * G, c = iy * G + ix;
  size_t lo = 0, hi = 0;   // the layer the cell is in, the layer the step descends into
  if constexpr (Time) { lo = (size_t)min(t, T) * cells; hi = (size_t)min(t + 1, T) * cells; }
  return plan_step(plan_moves(plan_unblocked(occ + lo), G, ix, iy), d[lo + c], d + hi, G, c, prev, Time && t < T);
}

// The tail of a field, by a whole workgroup of kPlanFieldThreads threads, cell c on thread c % 1024: the moves of every cell of the
// map `free` into `moves`, d = 0 on a free goal and kPlanInf elsewhere, then sweeps of relaxations until a workgroup-wide "nothing
// changed" -> the sweeps run (the last one changed nothing), -1: the bound of G * G was hit.  The relaxations are IN PLACE: every
// value ever stored in d is the cost of a real path to the goal and values only decrease, so a neighbour's value read while its owner
// replaces it is an upper bound either way, and a sweep that changes nothing has found the fixed point.  A cell is read and written
// as one aligned 32-bit LDS word.  Blocked cells have no moves and stay at kPlanInf.  Whatever `free` reads is in place before the
// call; the last barrier here orders the final d before the caller's loads.
template <class Free>
__device__ __forceinline__ int plan_tail(int* d, unsigned char* moves, Free free, int goal, int G) {
  const int cells = G * G, tid = threadIdx.x, gs = 31 - __clz(G), gm = G - 1;
#pragma unroll 1
  for (int c = tid; c < cells; c += kPlanFieldThreads) {
    const bool blocked = !free(c);
    moves[c] = blocked ? 0 : (unsigned char)plan_moves(free, G, c & gm, c >> gs);
    d[c] = (c == goal && !blocked) ? 0 : kPlanInf;
  }
  __syncthreads();
  for (int sweep = 1; sweep <= cells; ++sweep) {   // the hard bound: a field that needs more is reported, not waited for
    int changed = 0;
#pragma unroll 1
    for (int c = tid; c < cells; c += kPlanFieldThreads) {
      const unsigned m = moves[c];
      if (m == 0 || c == goal) continue;
      const int cur = d[c];
      int best = cur;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (m & (1u << k)) best = min(best, d[c + plan_dy(k) * G + plan_dx(k)] + plan_w(k));
      if (best < cur) { d[c] = best; changed = 1; }
    }
    __syncthreads();   // this sweep's stores before the next sweep's loads
    if (!__syncthreads_or(changed)) return sweep;
  }
  return -1;
}

// One Jacobi step in time: the value of the free cell c in layer t from layer t + 1 (`nxt`) over the moves m of layer t's map and
// the wait.  A pure function of the layer behind it, so there is no order to argue about.
__device__ __forceinline__ int plan_jacobi(const int* nxt, unsigned m, int c, int G) {
  int best = nxt[c] + kPlanWait;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (m & (1u << k)) best = min(best, nxt[c + plan_dy(k) * G + plan_dx(k)] + plan_w(k));
  return min(best, kPlanInf);   // kPlanInf + a cost: still "none"
}

// goal_rules.grid_los over the predicate "cell c is hidden" (not clear): the supercover of the segment between the centres of (x, y)
// and (x1, y1), both in the grid (every cell visited lies in their bounding box).  At most dx + dy <= 2 G - 2 steps; the loop is
// bounded by 2 G on its own.
template <class Hidden>
__device__ __forceinline__ bool plan_los(Hidden hidden, int G, int x, int y, int x1, int y1) {
  if (hidden(y * G + x)) return false;
  const int dx = abs(x1 - x), dy = abs(y1 - y), sx = x1 > x ? 1 : -1, sy = y1 > y ? 1 : -1;
  int ix = 0, iy = 0;
  for (int it = 0; it < 2 * G && (ix < dx || iy < dy); ++it) {
    const int t = (1 + 2 * ix) * dy - (1 + 2 * iy) * dx;
    if (t < 0) {
      x += sx; ++ix;
    } else if (t > 0) {
      y += sy; ++iy;
    } else {   // exactly through a cell corner: both cells that share it must be clear (plan_moves' no corner cutting)
      if (hidden(y * G + x + sx) || hidden((y + sy) * G + x)) return false;
      x += sx; y += sy; ++ix; ++iy;
    }
    if (hidden(y * G + x)) return false;
  }
  return ix == dx && iy == dy;
}

// A robot's waypoints [K][P] and outputs.  `writer`: this thread stores (a wave that plans one robot counts in every lane and stores
// in lane 0).  The z of every waypoint is the goal's.
__device__ __forceinline__ void plan_emit(float* wp, int count, int K, int P, const PlanGrid& g, int ix, int iy, const float* gl, bool writer) {
  if (count < K && writer) {
    wp[count * P] = plan_centre(g, ix);
    wp[count * P + 1] = plan_centre(g, iy);
    if (P == 3) wp[count * P + 2] = gl[2];
  }
}
// the goal itself closes the path -> the status
__device__ __forceinline__ int plan_close(float* wp, int& count, int K, int P, const float* gl, bool writer) {
  if (count < K && writer)
    for (int j = 0; j < P; ++j) wp[count * P + j] = gl[j];
  ++count;
  return count > K ? kPlanTruncated : kPlanned;
}
// nothing of a walk that was given up (status 3) is handed out
__device__ __forceinline__ void plan_give_up(float* wp, int& count, int& cost, int K, int P) {
  for (int j = 0; j < min(count, K) * P; ++j) wp[j] = 0.f;
  count = 0;
  cost = -1;
}
__device__ __forceinline__ void plan_result(int* nwp, int* full, int* stat, int* cst, int count, int K, int status, int cost) {
  *nwp = min(count, K);
  *full = count;
  *stat = status;
  *cst = cost;
}

// ---- the static plan (mobrob_ppo_plan_grid): k_plan_occupancy (a thread per scene and cell), k_plan_field (a workgroup per distinct
// (scene, goal cell), the field in LDS), k_plan_path (a thread per robot, at most G * G steps) ---------------------------------------
struct PlanOccArgs {
  PlanGrid g;
  const float* boxes;   // [S][Mw][4]
  const int* nwall;     // [S]
  int Mw;
  const float* hz;      // [S][Mh][3]
  const int* nhz;       // [S]
  int Mh;
  unsigned char* occ;   // [S][G][G] out: 1 blocked
};

// is the cell centre (px, py) blocked by one of the mw walls wl [mw][4] or the mh hazards hl [mh][3], both staged in LDS?
__device__ __forceinline__ bool plan_centre_blocked(const PlanGrid& g, float px, float py, const float* wl, int mw, const float* hl, int mh) {
  bool blocked = false;
  for (int i = 0; i < mw; ++i)
    if (wall_sdf(px, py, wl[4 * i], wl[4 * i + 1], wl[4 * i + 2], wl[4 * i + 3]) <= g.inflate) blocked = true;
  for (int i = 0; i < mh; ++i) {
    const float dx = __fsub_rn(px, hl[3 * i]), dy = __fsub_rn(py, hl[3 * i + 1]);
    const float d = sqrtf(__fadd_rn(rounded(__fmul_rn(dx, dx)), rounded(__fmul_rn(dy, dy))));   // sqrtf: correctly rounded
    if (d <= __fadd_rn(hl[3 * i + 2], g.inflate)) blocked = true;
  }
  return blocked;
}

// grid (cdiv(G * G, 256), S), 256 threads, LDS 4 Mw + 3 Mh floats: the scene's walls and hazards, staged once per workgroup (at
// the caps of 1024 rows each that is 28 KB: a scene always fits)
__global__ __launch_bounds__(256) void k_plan_occupancy(PlanOccArgs a) {
  extern __shared__ __attribute__((aligned(16))) float plan_scene_lds[];
  const int s = blockIdx.y, G = a.g.G;
  const int mw = a.nwall ? a.nwall[s] : 0, mh = a.nhz ? a.nhz[s] : 0;
  float* wl = plan_scene_lds;
  float* hl = plan_scene_lds + 4 * a.Mw;
  for (int i = threadIdx.x; i < 4 * mw; i += 256) wl[i] = a.boxes[(size_t)s * a.Mw * 4 + i];
  for (int i = threadIdx.x; i < 3 * mh; i += 256) hl[i] = a.hz[(size_t)s * a.Mh * 3 + i];
  __syncthreads();
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= G * G) return;
  a.occ[(size_t)s * G * G + c] = plan_centre_blocked(a.g, plan_centre(a.g, c % G), plan_centre(a.g, c / G), wl, mw, hl, mh) ? 1 : 0;
}

struct PlanFieldArgs {
  int G;
  const unsigned char* occ;   // [S][G][G]
  const int* field_goal;      // [F] goal cell
  const int* field_scene;     // [F]
  int* field;                 // [F][G][G] out: cost-to-go, -1 blocked or unreachable
  int* sweeps;                // [F] out: sweeps run (the last one changed nothing), -1: the bound of G * G was hit
};

// LDS bytes of k_plan_field: the field, then one byte of moves per cell
inline size_t plan_field_lds_bytes(int G) { return (size_t)G * G * (sizeof(int) + 1); }

// One workgroup per field, 1024 threads: plan_tail on the scene's map.
__global__ __launch_bounds__(kPlanFieldThreads) void k_plan_field(PlanFieldArgs a) {
  extern __shared__ __attribute__((aligned(16))) int plan_field_lds[];
  const int f = blockIdx.x, G = a.G, cells = G * G, tid = threadIdx.x;
  int* d = plan_field_lds;
  unsigned char* moves = reinterpret_cast<unsigned char*>(plan_field_lds + cells);
  const int sweeps = plan_tail(d, moves, plan_unblocked(a.occ + (size_t)a.field_scene[f] * cells), a.field_goal[f], G);
  int* out = a.field + (size_t)f * cells;
  for (int c = tid; c < cells; c += kPlanFieldThreads) out[c] = d[c] >= kPlanInf ? -1 : d[c];
  if (tid == 0) a.sweeps[f] = sweeps;
}

struct PlanPathArgs {
  PlanGrid g;
  int N, K, P;
  const float* start;         // [N][P]
  const float* goal;          // [N][P]
  const int* field_of;        // [N]
  const int* field_scene;     // [F]
  const int* sweeps;          // [F] k_plan_field's: -1 = that field did not converge
  const unsigned char* occ;   // [S][G][G]
  const int* field;           // [F][G][G]
  float* wp;                  // [N][K][P] out (zeroed by the host)
  int* nwp;                   // [N] out: min(count, K)
  int* count;                 // [N] out: waypoints of the full path
  int* status;                // [N] out
  int* cost;                  // [N] out: d[start cell], -1 unreachable
};
// the time and the smoothing kernels take k_plan_path's arguments as their member p
__device__ __forceinline__ const PlanPathArgs& plan_path_args(const PlanPathArgs& a) { return a; }
template <class Args>
__device__ __forceinline__ const PlanPathArgs& plan_path_args(const Args& s) { return s.p; }

// Robot n's walk, by one thread: goal_rules.grid_path on a static field, or with Time goal_rules.grid_walk_time with grid_path_time's
// waypoints on a time field (Args: PlanPathArgs, PlanPathTimeArgs).  A centre is a waypoint where the direction changes or a wait
// ended; with Time the waits at a waypoint's anchor and the actions before the move that leaves it are recorded.  At most T + G * G
// actions (T = 0 without Time): status 3 beyond.  A blocked start or goal cell has d < 0 in its field.
template <bool Time, class Args>
__device__ __forceinline__ void plan_path(const Args& s, int n) {
  const PlanPathArgs& a = plan_path_args(s);
  const int T = [&s] { if constexpr (Time) return s.T; else return 0; }();
  const int G = a.g.G, cells = G * G, P = a.P, K = a.K;
  const int f = a.field_of[n];
  const unsigned char* occ = a.occ + (size_t)a.field_scene[f] * (T + 1) * cells;
  const int* d = a.field + (size_t)f * (T + 1) * cells;
  const float* st = a.start + (size_t)n * P;
  const float* gl = a.goal + (size_t)n * P;
  float* wp = a.wp + (size_t)n * K * P;
  int ix = plan_cell(a.g, st[0]), iy = plan_cell(a.g, st[1]);
  const int gx = plan_cell(a.g, gl[0]), gy = plan_cell(a.g, gl[1]);
  int count = 0, status = kPlanned, cost = -1, acts = 0;
  if (a.sweeps[f] < 0) {
    status = kPlanUnconverged;
  } else if (d[iy * G + ix] < 0) {
    status = kPlanUnreachable;
  } else {
    cost = d[iy * G + ix];
    int prev = -1, waited = 0;
    while (ix != gx || iy != gy) {
      if (acts >= T + cells) { status = kPlanUnconverged; break; }
      const int dir = plan_walk_step<Time>(occ, d, G, T, acts, ix, iy, prev);
      if (dir < 0) { status = kPlanUnconverged; break; }   // not a field of these maps: cannot happen after a converged field kernel
      ++acts;
      if (dir == 8) { ++waited; continue; }
      const bool turned = prev >= 0 && (dir != prev || waited > 0);
      if (turned) {
        plan_emit(wp, count, K, P, a.g, ix, iy, gl, true);
        ++count;
      }
      if constexpr (Time)
        if ((prev < 0 || turned) && count < K) {   // this move leaves the anchor of waypoint `count`
          s.waits[(size_t)n * K + count] = waited;
          s.leave[(size_t)n * K + count] = acts - 1;
        }
      ix += plan_dx(dir); iy += plan_dy(dir);
      prev = dir;
      waited = 0;
    }
    if (status == kPlanned) status = plan_close(wp, count, K, P, gl, true);
  }
  if (status == kPlanUnconverged) {
    plan_give_up(wp, count, cost, K, P);
    if constexpr (Time)
      for (int j = 0; j < K; ++j) { s.waits[(size_t)n * K + j] = 0; s.leave[(size_t)n * K + j] = 0; }
    acts = 0;
  }
  plan_result(a.nwp + n, a.count + n, a.status + n, a.cost + n, count, K, status, cost);
  if constexpr (Time) s.arrive[n] = acts;
}

// one thread per robot, 256 to a workgroup
__global__ __launch_bounds__(256) void k_plan_path(PlanPathArgs a) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n < a.N) plan_path<false>(a, n);
}

// ---- line-of-sight smoothing (mobrob_ppo_plan_smooth; the rule: goal_rules.grid_los / grid_smooth / grid_path_smooth) ----------
// "clear" at margin 1: no in-grid cell of the 3 x 3 neighbourhood blocked.  k_plan_dilate writes the cells that are NOT clear
// once per set of resident fields; at margin 0 the occupancy itself is that map.
struct PlanDilateArgs {
  int G;
  const unsigned char* occ;   // [S][G][G]
  unsigned char* dil;         // [S][G][G] out
};

// grid (cdiv(G * G, 256), S), 256 threads
__global__ __launch_bounds__(256) void k_plan_dilate(PlanDilateArgs a) {
  const int G = a.G, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= G * G) return;
  const unsigned char* occ = a.occ + (size_t)blockIdx.y * G * G;
  const int ix = c % G, iy = c / G;
  unsigned char any = 0;
  for (int y = max(iy - 1, 0); y <= min(iy + 1, G - 1); ++y)
    for (int x = max(ix - 1, 0); x <= min(ix + 1, G - 1); ++x) any |= occ[y * G + x];
  a.dil[(size_t)blockIdx.y * G * G + c] = any ? 1 : 0;
}

// goal_rules.grid_los_time on the layer nbl = nb[lo] of a next-blocked table (k_plan_next_blocked) with the threshold hi: a cell is
// hidden where it is not clear in some layer lo .. hi
__device__ __forceinline__ bool plan_los_time(const short* nbl, int hi, int G, int x, int y, int x1, int y1) {
  return plan_los([nbl, hi](int c) { return nbl[c] <= hi; }, G, x, y, x1, y1);
}

constexpr int kPlanRing = 128;   // cells of the walk kept per wave: the window of 64 candidates and the cell before it fit twice

struct PlanSmoothArgs {
  PlanPathArgs p;             // k_plan_path's own inputs and outputs
  const unsigned char* blk;   // [S][G][G] cells that are not clear: occ (margin 0) or k_plan_dilate's map (margin 1)
  int* moves;                 // [N] out: moves of the walk, 0 where none was made
};

// Robot blockIdx.x's smoothed plan, by one wave (grid N, 64 threads: the workgroup IS the wave, so nothing here waits for another wave
// and the trip counts of different robots never meet).  Args: PlanSmoothArgs, or with Time PlanSmoothTimeArgs.  The walk is
// plan_path's (plan_walk_step), wave-uniform -- the robot is blockIdx.x, so its state lives in scalar registers -- and lane 0 stores
// its cells, packed iy * 128 + ix, in `ring`, kPlanRing entries in LDS (256 B).  The ring is indexed by ACTION: c[a] is the cell after
// a actions, a wait repeats its cell, so `walked` counts actions + 1.  With the anchor c[i] and the first untested index `base` (= i +
// 2: the adjacent cell is never tested), lane l tests the leg c[i] .. c[base + l]: plan_los on blk, or with Time plan_los_time on
// nb[min(i, T)] with the threshold min(base + l, T), every layer the leg spans.  The first lane that fails, z = ctz(ballot), is the
// rule's first hidden index: c[base + z - 1] is emitted and becomes the anchor, base = base + z + 1.  No failure: base += 64, same
// anchor.  The walk runs ahead of base by at most 64 cells; the ring holds indices base - 1 .. base + 63 at any time.  Lane 0's
// stores to the ring and the other lanes' loads from it are ordered by wave-level fences: one wave, so no barrier.  Bounds: the walk
// T + G * G actions (plan_path's; T = 0 without Time), the window loop as many rounds (base grows by at least 1 a round and ends beyond
// A <= T + G * G), plan_los 2 G steps: status 3, outputs zeroed.
template <bool Time, class Args>
__device__ __forceinline__ void plan_smooth(const Args& s, unsigned short* ring) {
  const PlanPathArgs& a = s.p;
  const int T = [&s] { if constexpr (Time) return s.T; else return 0; }();
  const int n = blockIdx.x, lane = threadIdx.x;
  const int G = a.g.G, cells = G * G, P = a.P, K = a.K;
  const int f = a.field_of[n];
  const size_t scene_off = (size_t)a.field_scene[f] * (T + 1) * cells;
  const unsigned char* occ = a.occ + scene_off;
  const int* d = a.field + (size_t)f * (T + 1) * cells;
  const float* st = a.start + (size_t)n * P;
  const float* gl = a.goal + (size_t)n * P;
  float* wp = a.wp + (size_t)n * K * P;
  int wx = plan_cell(a.g, st[0]), wy = plan_cell(a.g, st[1]);   // the walker
  const int gx = plan_cell(a.g, gl[0]), gy = plan_cell(a.g, gl[1]);
  int count = 0, status = kPlanned, cost = -1, walked = 1, moves = 0;   // walked: cells c[0 .. walked - 1] are known
  if (a.sweeps[f] < 0) {
    status = kPlanUnconverged;
  } else if (d[wy * G + wx] < 0) {
    status = kPlanUnreachable;
  } else {
    cost = d[wy * G + wx];
    int ax = wx, ay = wy, ai = 0, base = 2, prev = -1;   // the anchor's cell and action index
    bool done = wx == gx && wy == gy;
    if (lane == 0) ring[0] = (unsigned short)(wy * 128 + wx);
    for (int round = 0;; ++round) {
      if (round > T + cells) { status = kPlanUnconverged; break; }
      while (!done && walked <= base + 63) {   // the walk, up to the end of the window
        if (walked > T + cells) { status = kPlanUnconverged; break; }
        const int dir = plan_walk_step<Time>(occ, d, G, T, walked - 1, wx, wy, prev);
        if (dir < 0) { status = kPlanUnconverged; break; }
        if (dir != 8) {
          wx += plan_dx(dir); wy += plan_dy(dir);
          prev = dir;
          ++moves;
        }
        if (lane == 0) ring[walked & (kPlanRing - 1)] = (unsigned short)(wy * 128 + wx);
        ++walked;
        done = wx == gx && wy == gy;
      }
      if (status != kPlanned) break;
      if (done && base >= walked) break;   // no candidate left: A = walked - 1
      // lane 0's stores to the ring before every lane's loads from it
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int idx = base + lane;
      bool hidden = false;
      if (idx < walked) {
        const int c = ring[idx & (kPlanRing - 1)];
        if constexpr (Time) {
          hidden = !plan_los_time(s.nb + scene_off + (size_t)min(ai, T) * cells, min(idx, T), G, ax, ay, c & 127, c >> 7);
        } else {
          hidden = !plan_los(plan_blocked(s.blk + scene_off), G, ax, ay, c & 127, c >> 7);
        }
      }
      const unsigned long long fails = __ballot(hidden);
      if (fails == 0) { base += 64; continue; }
      const int j = base + __builtin_ctzll(fails) - 1;   // the last visible index: emitted, the next anchor
      const int c = __builtin_amdgcn_readfirstlane((int)ring[j & (kPlanRing - 1)]);
      ax = c & 127; ay = c >> 7; ai = j;
      plan_emit(wp, count, K, P, a.g, ax, ay, gl, lane == 0);
      ++count;
      if constexpr (Time)
        if (count < K && lane == 0) s.leave[(size_t)n * K + count] = j;   // the anchor of the waypoint that follows
      base = j + 2;
      // the loads above before the walk's next stores to the ring
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    if (status == kPlanned) status = plan_close(wp, count, K, P, gl, lane == 0);
  }
  if (lane != 0) return;
  int acts = walked - 1;
  if (status == kPlanUnconverged) {
    plan_give_up(wp, count, cost, K, P);
    if constexpr (Time)
      for (int q = 0; q < K; ++q) s.leave[(size_t)n * K + q] = 0;
    acts = 0;
    moves = 0;
  }
  plan_result(a.nwp + n, a.count + n, a.status + n, a.cost + n, count, K, status, cost);
  if constexpr (Time) s.arrive[n] = acts;
  s.moves[n] = moves;
}

__global__ __launch_bounds__(64) void k_plan_smooth(PlanSmoothArgs s) {
  __shared__ unsigned short ring[kPlanRing];
  plan_smooth<false>(s, ring);
}

// ---- planning over time (mobrob_ppo_plan_grid_time; the rule: goal_rules.grid_layer_frames / grid_occupancy_time / grid_time_field /
// grid_walk_time / grid_path_time) ------------------------------------------------------------------------------------------------
// Moving hazards as T + 1 LAYERS of occupancy: layer t < T blocks what any hazard frame in force during the robot's t-th action
// blocks, the tail layer T what any frame from then on blocks.  A layer's frames are a cyclically contiguous run, `number` frames
// from `first` (computed on the host).  The time field d[T + 1][G][G]: d_T is k_plan_field's fixed point on the tail's map; d_t
// for t < T is one Jacobi step from d_{t+1} over the moves of layer t's map and the wait (kPlanWait).
constexpr int kPlanLayersMax = 256;

struct PlanOccTimeArgs {
  PlanGrid g;
  const float* boxes;       // [S][Mw][4]
  const int* nwall;         // [S]
  int Mw;
  const float* hz;          // [S][F][Mh][3]
  const int* nhz;           // [S]
  int Mh, F, T;
  const int* layer_first;   // [T + 1]
  const int* layer_number;  // [T + 1], 1 .. F
  unsigned char* occ;       // [S][T + 1][G][G] out: 1 blocked
};

// grid (G * G / 256, T + 1, S), 256 threads (G * G is a multiple of 256), LDS 4 Mw + 3 Mh floats: the scene's walls staged once,
// then every frame of the layer's set in turn, behind barriers; the walls are tested with the first frame.
__global__ __launch_bounds__(256) void k_plan_occupancy_time(PlanOccTimeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float plan_scene_time_lds[];
  const int s = blockIdx.z, t = blockIdx.y, G = a.g.G;
  const int mw = a.nwall ? a.nwall[s] : 0, mh = a.nhz[s];
  float* wl = plan_scene_time_lds;
  float* hl = plan_scene_time_lds + 4 * a.Mw;
  for (int i = threadIdx.x; i < 4 * mw; i += 256) wl[i] = a.boxes[(size_t)s * a.Mw * 4 + i];
  const int c = blockIdx.x * 256 + threadIdx.x;
  const float px = plan_centre(a.g, c % G), py = plan_centre(a.g, c / G);
  const int first = a.layer_first[t], number = a.layer_number[t];
  bool blocked = false;
  for (int j = 0; j < number; ++j) {
    int fr = first + j;
    if (fr >= a.F) fr -= a.F;
    if (j > 0) __syncthreads();   // the previous frame's loads before this frame's stores
    const float* rows = a.hz + ((size_t)s * a.F + fr) * a.Mh * 3;
    for (int i = threadIdx.x; i < 3 * mh; i += 256) hl[i] = rows[i];
    __syncthreads();
    if (plan_centre_blocked(a.g, px, py, wl, j == 0 ? mw : 0, hl, mh)) blocked = true;
  }
  a.occ[((size_t)s * (a.T + 1) + t) * G * G + c] = blocked ? 1 : 0;
}

struct PlanFieldTimeArgs {
  int G, T;
  const unsigned char* occ;   // [S][T + 1][G][G]
  const int* field_goal;      // [F] goal cell
  const int* field_scene;     // [F]
  int* field;                 // [F][T + 1][G][G] out: cost-to-go, -1 blocked or unreachable
  int* sweeps;                // [F] out: sweeps of the tail's relaxation, -1: the bound of G * G was hit
};

// LDS bytes of k_plan_field_time: two layers of the field, then one byte of moves per cell (144 KB at 128 cells)
inline size_t plan_field_time_lds_bytes(int G) { return (size_t)G * G * (2 * sizeof(int) + 1); }

// One workgroup per field, 1024 threads.  The tail is plan_tail on the tail's map.  Then T backward layers between two LDS layers,
// ping-pong: layer t is written from layer t + 1 alone (plan_jacobi); the one barrier per layer puts a layer's stores before the
// next layer's loads, and the buffer a layer overwrites was last read before that barrier.  A layer's moves come from its own map in
// global memory, each cell once.
__global__ __launch_bounds__(kPlanFieldThreads) void k_plan_field_time(PlanFieldTimeArgs a) {
  extern __shared__ __attribute__((aligned(16))) int plan_field_time_lds[];
  const int f = blockIdx.x, G = a.G, T = a.T, cells = G * G, tid = threadIdx.x, gs = 31 - __clz(G), gm = G - 1;
  int* nxt = plan_field_time_lds;           // layer t + 1
  int* cur = plan_field_time_lds + cells;   // layer t
  unsigned char* moves = reinterpret_cast<unsigned char*>(plan_field_time_lds + 2 * cells);
  const unsigned char* occ_scene = a.occ + (size_t)a.field_scene[f] * (T + 1) * cells;
  const int goal = a.field_goal[f];
  const int sweeps = plan_tail(nxt, moves, plan_unblocked(occ_scene + (size_t)T * cells), goal, G);
  int* out = a.field + (size_t)f * (T + 1) * cells;
  for (int c = tid; c < cells; c += kPlanFieldThreads) out[(size_t)T * cells + c] = nxt[c] >= kPlanInf ? -1 : nxt[c];
  if (tid == 0) a.sweeps[f] = sweeps;
  for (int t = T - 1; t >= 0; --t) {
    const unsigned char* occ_t = occ_scene + (size_t)t * cells;
    for (int c = tid; c < cells; c += kPlanFieldThreads) {
      int best = kPlanInf;
      if (!occ_t[c]) best = c == goal ? 0 : plan_jacobi(nxt, plan_moves(plan_unblocked(occ_t), G, c & gm, c >> gs), c, G);
      cur[c] = best;
      out[(size_t)t * cells + c] = best >= kPlanInf ? -1 : best;
    }
    __syncthreads();
    int* const swap = nxt; nxt = cur; cur = swap;
  }
}

struct PlanPathTimeArgs {
  PlanPathArgs p;   // k_plan_path's inputs and outputs; occ [S][T + 1][G][G], field [F][T + 1][G][G]
  int T;
  int* waits;       // [N][K] out (zeroed by the host): waits at waypoint k's anchor
  int* leave;       // [N][K] out (zeroed by the host): actions before the move that leaves that anchor
  int* arrive;      // [N] out: actions of the whole walk
};

// one thread per robot, 64 to a workgroup
__global__ __launch_bounds__(64) void k_plan_path_time(PlanPathTimeArgs s) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n < s.p.N) plan_path<true>(s, n);
}

// ---- prioritised planning inside a team (mobrob_ppo_plan_grid_team; the rule: goal_rules.grid_reserve / grid_team_field /
// grid_walk_team / grid_plan_team) ------------------------------------------------------------------------------------------------
// A mate's planned walk is one more moving obstacle in the layers.  The member with team-local index m plans after the members
// 0 .. m - 1 on the map occ_t = base_t OR res_t: layer t < T reserves every cell within Chebyshev distance r of an earlier member's
// c[t] or c[t + 1], the tail layer T every cell within r of its c[a], a >= min(T, A).  A member without a walk (unreachable, or a
// loop bound hit) reserves its start cell in every layer.  The field is k_plan_field_time's with one change: the goal cell is
// terminal only where it is free in occ_t and in every later layer; the walk ends where d_t[c] == 0.
constexpr int kPlanTeamMax = 16;     // members of a team
constexpr int kPlanReserveMax = 4;   // r

struct PlanTeamArgs {
  PlanGrid g;
  int N, K, P, T, size, reserve, n_teams;
  int has_scene;              // 0: every robot in scene 0 (all members of a team: one scene)
  int walk_cap;               // cells per robot in `walk`
  const float* in;            // the robots: start [N][P] | goal [N][P] | scene [N] (int)
  const unsigned char* occ;   // [S][T + 1][G][G] the base layers
  int* wg;                    // per workgroup, plan_team_wg_ints(G, T) ints: the member's field [T + 1][G][G] (-1 blocked, kPlanInf free
                              // without a path) | the tail cells of the member that walked last [G * G + 4], packed iy * 128 + ix | the
                              // tail reservations of the team's earlier members, stamped, one byte a cell [G * G]
  int* out;                   // n_waypoints | count | status | cost | arrive | sweeps, [N] each | waits [N][K] | leave [N][K] | waypoints
                              // [N][K][P] (float); from waits on zeroed by the host
  int* fields;                // [N][T + 1][G][G] out or null: the fields as the rule states them (-1 blocked or unreachable)
  unsigned short* walk;       // [N][walk_cap] out or null: the cells c[0 .. min(A, walk_cap - 1)] of the walk, packed
};
// one block of arguments, outputs and scratch each, addressed by offset: a pointer per array would not fit the scalar registers
__host__ __device__ inline size_t plan_team_wg_ints(int G, int T) { return (size_t)(T + 1) * G * G + (size_t)G * G + 4 + (size_t)G * G / 4; }

// LDS bytes of k_plan_team: k_plan_field_time's two layers and one byte per cell, then the walk cells c[0 .. T] of the team's
// members (2 bytes a cell) and two words the walking thread hands over
inline size_t plan_team_lds_bytes(int G, int T) {
  return (size_t)G * G * (2 * sizeof(int) + 1) + (size_t)kPlanTeamMax * (T + 1) * sizeof(unsigned short) + 16;
}

// the per-workgroup block of PlanTeamArgs::wg, and where a workgroup of k_plan_team keeps what one phase hands to the next
__device__ __forceinline__ int* plan_team_wg(const PlanTeamArgs& a) { return a.wg + blockIdx.x * (int)plan_team_wg_ints(a.g.G, a.T); }
struct PlanTeamHand {
  unsigned short* wcell;   // LDS [kPlanTeamMax][T + 1]: the members' c[0 .. T], behind d, e and the byte map
  int* hand;               // LDS, behind wcell (32 (T + 1) bytes on: a word boundary): [0] the number of tail cells
  int* tail;               // scratch: the tail cells of the member that walked last
  unsigned char* tres;     // scratch: the stamped tail reservations
};
__device__ __forceinline__ PlanTeamHand plan_team_hand(const PlanTeamArgs& a, int* lds) {
  const int cells = a.g.G * a.g.G, T = a.T;
  PlanTeamHand h;
  h.wcell = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(lds + 2 * cells) + cells);
  h.hand = reinterpret_cast<int*>(h.wcell + kPlanTeamMax * (T + 1));
  h.tail = plan_team_wg(a) + (T + 1) * cells;
  h.tres = reinterpret_cast<unsigned char*>(h.tail + cells + 4);
  return h;
}

// Where "reserved" comes from in the field of k_plan_team's member m: in layer t < T, within r of the c[t] or c[t + 1] of a member 0 ..
// m - 1 (LDS); in the tail, the stamped bytes.  No next-blocked table.
struct PlanReservedNear {
  using Args = PlanTeamArgs;
  static constexpr bool kNextBlocked = false;
  int* field;
  const unsigned short* wcell;
  const unsigned char* tres;
  int m, T, r, gs, gm;
  __device__ __forceinline__ PlanReservedNear(const Args& a, int m_, int* lds)
      : field(plan_team_wg(a)), m(m_), T(a.T), r(a.reserve), gs(31 - __clz(a.g.G)), gm(a.g.G - 1) {
    const PlanTeamHand h = plan_team_hand(a, lds);
    wcell = h.wcell;
    tres = h.tres;
  }
  __device__ __forceinline__ static const PlanTeamArgs& team(const Args& a) { return a; }
  // is cell c blocked in the tail's map, in layer t's: `base` (the base layer blocks it) OR reserved
  __device__ __forceinline__ bool tail(int c, bool base) const { return base | (tres[c] != 0); }
  __device__ __forceinline__ bool layer(int t, int c, bool base) const {
    const int cx = c & gm, cy = c >> gs;
    bool near = base;
    for (int j = 0; j < m && !near; ++j) {
      const int w0 = wcell[j * (T + 1) + t], w1 = wcell[j * (T + 1) + t + 1];
      near = (abs(cx - (w0 & 127)) <= r && abs(cy - (w0 >> 7)) <= r) || (abs(cx - (w1 & 127)) <= r && abs(cy - (w1 >> 7)) <= r);
    }
    return near;
  }
};

// is a cell within `margin` (0 or 1) of (x, y) that lies in the grid blocked?  (goal_rules.los_blocked, a cell at a time.)  Nine loads
// without a branch: the neighbours are clamped into the grid, where a clamped one repeats a cell of the neighbourhood; at margin 0
// all nine are the cell itself.
template <class Occ>
__device__ __forceinline__ bool plan_near_blocked(const Occ* occ, int G, int x, int y, int margin) {
  const int x0 = max(x - margin, 0), x1 = min(x + margin, G - 1), r0 = max(y - margin, 0) * G, r1 = y * G, r2 = min(y + margin, G - 1) * G;
  return (occ[r0 + x0] | occ[r0 + x] | occ[r0 + x1] | occ[r1 + x0] | occ[r1 + x] | occ[r1 + x1] | occ[r2 + x0] | occ[r2 + x] | occ[r2 + x1]) != 0;
}

// One member's field, by the whole workgroup -> the sweeps of the tail's relaxation (-1: bound hit): the tail's map (base OR reserved)
// into e and plan_tail on it; then T Jacobi layers as k_plan_field_time's, each on a layer map (base OR reserved) built in LDS in
// `moves`, with the goal terminal only while it stays free.  Every layer goes to the workgroup's scratch field (-1 blocked, kPlanInf
// free without a path: the walking thread reads occupancy and cost from one array) and, where asked for, to `fields` as the rule
// states it.  With Reserved::kNextBlocked the same pass over the layers, tail first, writes the member's next-blocked table nb
// (k_plan_next_blocked's meaning) from the layer's blocked bytes in LDS: the byte itself at margin 0, the OR over the 3 x 3
// neighbours at margin 1; nb[t + 1][c] is read back by the thread that wrote it.
// A function of its own, not inlined, and so are the walks: the wave-uniform values of a phase then live in scalar registers only
// while the phase runs (inlined, the phases' loop-invariant values overflowed the scalar file).  For the same reason the cell loops
// are not unrolled, and every phase reads the arguments from memory.
template <class Reserved>
__device__ __noinline__ int plan_team_field(const typename Reserved::Args* __restrict__ ap, int n, int m, int* lds) {
  const PlanTeamArgs& a = Reserved::team(*ap);
  const Reserved rsv(*ap, m, lds);
  const int G = a.g.G, T = a.T, cells = G * G, tid = threadIdx.x;
  const int gs = 31 - __clz(G), gm = G - 1;
  const int scene = a.has_scene ? reinterpret_cast<const int*>(a.in + 2 * a.N * a.P)[n] : 0;
  const float* gl = a.in + (a.N + n) * a.P;
  const int goal = plan_cell(a.g, gl[1]) * G + plan_cell(a.g, gl[0]);
  int* d = lds;
  int* e = lds + cells;
  unsigned char* moves = reinterpret_cast<unsigned char*>(lds + 2 * cells);
  const unsigned char* occ_scene = a.occ + (size_t)scene * (T + 1) * cells;
  int* field = rsv.field;   // (the host's checks: every offset but the base layers' fits an int)
  int* out = a.fields ? a.fields + n * (T + 1) * cells : nullptr;
  // the tail: its map into e (a thread reads the reservations of its own cells only after the fence and barrier that follow their
  // writing), then the moves and the in-place relaxation
  const unsigned char* occ_T = occ_scene + (size_t)T * cells;
#pragma unroll 1
  for (int c = tid; c < cells; c += kPlanFieldThreads) e[c] = rsv.tail(c, occ_T[c] != 0) ? 1 : 0;
  __syncthreads();
  bool terminal = e[goal] == 0;
  const int sweeps = plan_tail(d, moves, plan_unblocked(e), goal, G);
#pragma unroll 1
  for (int c = tid; c < cells; c += kPlanFieldThreads) {
    field[T * cells + c] = e[c] ? -1 : d[c];
    if (out) out[T * cells + c] = d[c] >= kPlanInf ? -1 : d[c];
    if constexpr (Reserved::kNextBlocked)
      rsv.nb[T * cells + c] = plan_near_blocked(e, G, c & gm, c >> gs, rsv.margin) ? (short)T : kPlanNeverBlocked;
  }
  int* nxt = d;   // layer t + 1
  int* cur = e;   // layer t
  for (int t = T - 1; t >= 0; --t) {
    const unsigned char* occ_t = occ_scene + (size_t)t * cells;
    // layer t's map into `moves` (the tail's moves are done with)
#pragma unroll 1
    for (int c = tid; c < cells; c += kPlanFieldThreads) moves[c] = rsv.layer(t, c, occ_t[c] != 0) ? 1 : 0;
    __syncthreads();   // the map before its readers; also e's last readers (the tail's write-out) before the first layer's stores
    terminal = terminal && moves[goal] == 0;
#pragma unroll 1
    for (int c = tid; c < cells; c += kPlanFieldThreads) {
      const bool blocked = moves[c] != 0;
      int best = kPlanInf;
      if (!blocked) best = (c == goal && terminal) ? 0 : plan_jacobi(nxt, plan_moves(plan_unblocked(moves), G, c & gm, c >> gs), c, G);
      cur[c] = best;
      field[t * cells + c] = blocked ? -1 : best;
      if (out) out[t * cells + c] = best >= kPlanInf ? -1 : best;
      if constexpr (Reserved::kNextBlocked)
        rsv.nb[t * cells + c] = plan_near_blocked(moves, G, c & gm, c >> gs, rsv.margin) ? (short)t : rsv.nb[(t + 1) * cells + c];
    }
    __syncthreads();
    int* const swap = nxt; nxt = cur; cur = swap;
  }
  return sweeps;
}

// action number `acts` of a member's walk from (ix, iy) on its scratch field [T + 1][G][G], whose value at the cell in layer min(acts,
// T) is dc: plan_walk_step with the field itself as the map (a cell is blocked where d < 0)
__device__ __forceinline__ int plan_team_step(const int* field, int G, int T, int acts, int dc, int ix, int iy, int prev) {
  const int cells = G * G, t = min(acts, T);
  const int* dt = field + t * cells;
  return plan_step(plan_moves([dt](int c) { return dt[c] >= 0; }, G, ix, iy), dc, field + min(t + 1, T) * cells, G, iy * G + ix, prev, t < T);
}

// The walk of one member, by one thread: plan_path<true>'s loop on this workgroup's scratch field, ending where d_t[c] == 0.  It leaves
// the member's outputs, c[0 .. T] in its row of wcell (LDS), the tail cells in `tail` and their number in hand[0].
__device__ __noinline__ void plan_team_walk(const PlanTeamArgs* __restrict__ ap, int n, int m, int sweeps, int* lds) {
  const PlanTeamArgs& a = *ap;
  const int G = a.g.G, T = a.T, cells = G * G, P = a.P, K = a.K;
  const PlanTeamHand h = plan_team_hand(a, lds);
  const int* field = plan_team_wg(a);
  unsigned short* mine = h.wcell + m * (T + 1);
  const float* st = a.in + n * P;
  const float* gl = a.in + (a.N + n) * P;
  int* waits = a.out + 6 * a.N + n * K;
  int* leave = waits + a.N * K;
  float* wp = reinterpret_cast<float*>(a.out + 6 * a.N + 2 * a.N * K) + n * K * P;
  unsigned short* wout = a.walk ? a.walk + n * a.walk_cap : nullptr;
  const int sx = plan_cell(a.g, st[0]), sy = plan_cell(a.g, st[1]);
  int ix = sx, iy = sy;
  int count = 0, status = kPlanned, cost = -1, acts = 0, ntail = 0;
  const int d0 = field[iy * G + ix];
  if (sweeps < 0) {
    status = kPlanUnconverged;
  } else if (d0 < 0 || d0 >= kPlanInf) {
    status = kPlanUnreachable;
  } else {
    cost = d0;
    int prev = -1, waited = 0;
    mine[0] = (unsigned short)(iy * 128 + ix);
    if (wout) wout[0] = mine[0];
    for (;;) {
      const int dc = field[min(acts, T) * cells + iy * G + ix];
      if (dc == 0) break;
      if (acts >= T + cells) { status = kPlanUnconverged; break; }
      const int dir = plan_team_step(field, G, T, acts, dc, ix, iy, prev);
      if (dir < 0) { status = kPlanUnconverged; break; }   // not a team field of these layers: cannot happen after a converged tail
      ++acts;
      if (dir == 8) {
        ++waited;
      } else {
        const bool turned = prev >= 0 && (dir != prev || waited > 0);
        if (turned) {
          plan_emit(wp, count, K, P, a.g, ix, iy, gl, true);
          ++count;
        }
        if ((prev < 0 || turned) && count < K) {   // this move leaves the anchor of waypoint `count`
          waits[count] = waited;
          leave[count] = acts - 1;
        }
        ix += plan_dx(dir); iy += plan_dy(dir);
        prev = dir;
        waited = 0;
      }
      const unsigned short cell = (unsigned short)(iy * 128 + ix);   // c[acts]
      if (acts <= T) mine[acts] = cell;
      if (acts >= T) h.tail[ntail++] = cell;                           // at most cells + 1 of them (room for cells + 4): acts <= T + cells
      if (wout && acts < a.walk_cap) wout[acts] = cell;
    }
    if (status == kPlanned) status = plan_close(wp, count, K, P, gl, true);
  }
  if (status == kPlanUnconverged) {
    plan_give_up(wp, count, cost, K, P);
    for (int j = 0; j < K; ++j) { waits[j] = 0; leave[j] = 0; }
    acts = 0;
  }
  if (status == kPlanUnreachable || status == kPlanUnconverged) {   // parked: the start cell, in every layer
    ix = sx; iy = sy;
    mine[0] = (unsigned short)(iy * 128 + ix);
    if (wout) wout[0] = mine[0];
    ntail = 0;
  }
  const unsigned short last = (unsigned short)(iy * 128 + ix);
  for (int t = acts + 1; t <= T; ++t) mine[t] = last;   // c[a] = c[A] beyond the walk
  if (acts < T) { h.tail[0] = last; ntail = 1; }
  h.hand[0] = ntail;
  int* o = a.out + n;
  plan_result(o, o + a.N, o + 2 * a.N, o + 3 * a.N, count, K, status, cost);
  o[4 * a.N] = acts;
  o[5 * a.N] = sweeps;
}

// One member of a team, robot n planned in slot m, by the whole workgroup: its field by all threads; thread 0 walks that field and
// leaves the member's c[0 .. T] in LDS and its tail cells in global memory; all threads stamp the tail cells.  Every hand-off through
// global memory -- the field (and what the caller zeroed) to the walking thread, the tail cells and the stamped map to the whole
// workgroup -- is a workgroup-scope fence and then the barrier; c[0 .. T] and the count are in LDS, which the barrier orders.
__device__ __forceinline__ void plan_team_member(const PlanTeamArgs* __restrict__ ap, int n, int m, int* lds) {
  const int G = ap->g.G, r = ap->reserve, tid = threadIdx.x;
  const PlanTeamHand h = plan_team_hand(*ap, lds);
  const int sweeps = plan_team_field<PlanReservedNear>(ap, n, m, lds);
  __threadfence_block();
  __syncthreads();
  if (tid == 0) plan_team_walk(ap, n, m, sweeps, lds);
  __threadfence_block();
  __syncthreads();
  const int ntail = h.hand[0];
#pragma unroll 1
  for (int i = tid; i < ntail; i += kPlanFieldThreads) {
    const int cx = h.tail[i] & 127, cy = h.tail[i] >> 7;
    for (int y = max(cy - r, 0); y <= min(cy + r, G - 1); ++y)
      for (int x = max(cx - r, 0); x <= min(cx + r, G - 1); ++x) h.tres[y * G + x] = 1;
  }
  // the stamps, bytes in global memory written by any thread, before the next member's tail map (and the next team's zeroes)
  __threadfence_block();
  __syncthreads();
}

// A team is sequential inside and parallel outside: one workgroup of 1024 threads takes one team at a time, a fixed number of
// workgroups loops over the teams, member after member (plan_team_member).  Bounds: G * G sweeps, T + G * G actions: status 3 and
// zeroed outputs beyond, the member then reserves its start cell.
__global__ __launch_bounds__(kPlanFieldThreads) void k_plan_team(const PlanTeamArgs* __restrict__ ap) {
  extern __shared__ __attribute__((aligned(16))) int plan_team_lds[];
  const int cells = ap->g.G * ap->g.G, tid = threadIdx.x, size = ap->size, n_teams = ap->n_teams;
  const PlanTeamHand h = plan_team_hand(*ap, plan_team_lds);
  for (int team = blockIdx.x; team < n_teams; team += gridDim.x) {
#pragma unroll 1
    for (int c = tid; c < cells; c += kPlanFieldThreads) h.tres[c] = 0;   // (its last readers and writers: behind the member's last barrier)
    for (int m = 0; m < size; ++m) plan_team_member(ap, team * size + m, m, plan_team_lds);
  }
}

// ---- priority reordering rounds of a team plan (mobrob_ppo_plan_grid_team_rounds; the rule: goal_rules.grid_plan_team_rounds) ---
// k_plan_team with a loop of rounds around the member loop.  Round 0 plans in the identity order; after a round the members without
// a walk (status 1 or 3) are "parked", and the next order is the parked members, then the others, each in this round's relative
// order.  The rounds stop when nobody is parked, after `retries` reorderings, or when the next order was already planned.  The result
// is the round with the fewest parked members, the earliest on a tie: if that is not the round planned last, the team is planned
// once more in its order -- the plan is a function of the order alone, so this replay leaves the best round's bits in the outputs.
// Position p of the order plans robot team * size + order[p] in slot p: plan_team_member takes both.
constexpr int kPlanRetriesMax = 8;

struct PlanTeamRoundsArgs {
  PlanTeamArgs t;   // k_plan_team's
  int retries;      // R, 0 .. kPlanRetriesMax
  int* team;        // out: order [n_teams][size] | rounds [n_teams] | parked [n_teams] | parked_first [n_teams]
};

// LDS bytes of k_plan_team_rounds: k_plan_team's, then 4 control words, the parked count of every round and the orders planned so
// far (16 bytes a round)
inline size_t plan_team_rounds_lds_bytes(int G, int T, int retries) {
  return plan_team_lds_bytes(G, T) + 16 + (size_t)(retries + 1) * (sizeof(int) + kPlanTeamMax);
}

// The bookkeeping between two rounds, by one thread between two barriers.  ctl: [0] the row of `hist` to plan next (-1: the team
// is done), [1] the rounds planned, [2] the best round, [3] 1 while the replay runs.  Not inlined (plan_team_field says why).
__device__ __noinline__ void plan_team_round_next(const PlanTeamRoundsArgs* __restrict__ rp, int team, int* ctl) {
  const int size = rp->t.size, R = rp->retries, N = rp->t.N, n_teams = rp->t.n_teams;
  if (ctl[3]) { ctl[0] = -1; return; }   // that was the replay of the best round
  int* parked = ctl + 4;
  unsigned char* hist = reinterpret_cast<unsigned char*>(parked + R + 1);
  const int k = ctl[1];
  const unsigned char* ord = hist + k * kPlanTeamMax;
  const int* status = rp->t.out + 2 * N + team * size;
  unsigned is_parked = 0;   // bit m: member m has no walk
  for (int m = 0; m < size; ++m)
    if (status[m] == kPlanUnreachable || status[m] == kPlanUnconverged) is_parked |= 1u << m;
  const int np = __popc(is_parked);
  parked[k] = np;
  ctl[1] = k + 1;
  int best = ctl[2];
  if (k == 0 || np < parked[best]) best = k;
  ctl[2] = best;
  bool stop = np == 0 || k == R;
  if (!stop) {   // k < R: row k + 1 of hist exists
    unsigned char* nxt = hist + (k + 1) * kPlanTeamMax;
    int q = 0;
    for (int p = 0; p < size; ++p)
      if (is_parked & (1u << ord[p])) nxt[q++] = ord[p];
    for (int p = 0; p < size; ++p)
      if (!(is_parked & (1u << ord[p]))) nxt[q++] = ord[p];
    for (int j = 0; j <= k && !stop; ++j) {   // planned before (also: the parked members are in front already)
      bool same = true;
      for (int p = 0; p < size; ++p) same = same && hist[j * kPlanTeamMax + p] == nxt[p];
      stop = same;
    }
  }
  if (!stop) { ctl[0] = k + 1; return; }
  int* o = rp->team;
  for (int p = 0; p < size; ++p) o[team * size + p] = hist[best * kPlanTeamMax + p];
  o += n_teams * size;
  o[team] = k + 1;
  o[n_teams + team] = parked[best];
  o[2 * n_teams + team] = parked[0];
  if (best != k) { ctl[0] = best; ctl[3] = 1; } else { ctl[0] = -1; }
}

__global__ __launch_bounds__(kPlanFieldThreads) void k_plan_team_rounds(const PlanTeamRoundsArgs* __restrict__ rp) {
  extern __shared__ __attribute__((aligned(16))) int plan_team_rounds_lds[];
  const PlanTeamArgs* ap = &rp->t;
  const int cells = ap->g.G * ap->g.G, tid = threadIdx.x, size = ap->size, n_teams = ap->n_teams;
  // LDS: k_plan_team's (d | e | moves | wcell | hand, 16 bytes) | ctl [4] | parked [R + 1] | hist [R + 1][16] (bytes)
  const PlanTeamHand h = plan_team_hand(*ap, plan_team_rounds_lds);
  int* ctl = h.hand + 4;
  unsigned char* hist = reinterpret_cast<unsigned char*>(ctl + 4 + rp->retries + 1);
  for (int team = blockIdx.x; team < n_teams; team += gridDim.x) {
    if (tid == 0) {   // round 0: the identity order (the last team's readers of ctl and hist: behind the barrier that ended its rounds)
      ctl[0] = 0; ctl[1] = 0; ctl[2] = 0; ctl[3] = 0;
      for (int p = 0; p < kPlanTeamMax; ++p) hist[p] = (unsigned char)p;
    }
    __syncthreads();
    for (int pass = 0;; ++pass) {   // at most retries + 1 rounds and the replay
      const unsigned char* ord = hist + ctl[0] * kPlanTeamMax;
#pragma unroll 1
      for (int c = tid; c < cells; c += kPlanFieldThreads) h.tres[c] = 0;   // per round (its last readers and writers: behind a barrier)
      for (int m = 0; m < size; ++m) {
        const int n = team * size + ord[m];
        if (pass > 0) {   // plan_team_walk writes only the slots its walk touches: what the member's last walk left goes first
          const int K = ap->K, P = ap->P, N = ap->N;   // (read here: live across the member's phases they would take scalar registers)
          int* waits = ap->out + 6 * N + n * K;
          float* wp = reinterpret_cast<float*>(ap->out + 6 * N + 2 * N * K) + n * K * P;
#pragma unroll 1
          for (int j = tid; j < K; j += kPlanFieldThreads) { waits[j] = 0; waits[N * K + j] = 0; }
#pragma unroll 1
          for (int j = tid; j < K * P; j += kPlanFieldThreads) wp[j] = 0.f;
        }
        plan_team_member(ap, n, m, plan_team_rounds_lds);
      }
      if (tid == 0) plan_team_round_next(rp, team, ctl);   // thread 0 wrote the statuses it reads
      __syncthreads();
      if (ctl[0] < 0) break;
    }
    __syncthreads();   // every thread has read ctl[0] before the next team's thread 0 resets it
  }
}

// ---- line-of-sight smoothing of a time plan (mobrob_ppo_plan_grid_time_smooth; the rule: goal_rules.grid_next_blocked /
// grid_los_time / grid_smooth_time / grid_path_smooth_time) -------------------------------------------------------------------------
// A straight leg is tested against EVERY layer it spans.  nb[t][c]: the first layer from t on in which cell c is not clear
// (kPlanNeverBlocked: none), so "c is clear in the layers lo .. hi" is nb[lo][c] > hi, one load whatever the span.
struct PlanNextBlockedArgs {
  int G, T;
  const unsigned char* blk;   // [S][T + 1][G][G] cells that are not clear: k_plan_occupancy_time's maps (margin 0) or k_plan_dilate's of them
  short* nb;                  // [S][T + 1][G][G] out
};

// grid (G * G / 256, S), 256 threads (G * G is a multiple of 256): a thread scans its cell's T + 1 layers from the tail down
__global__ __launch_bounds__(256) void k_plan_next_blocked(PlanNextBlockedArgs a) {
  const int cells = a.G * a.G, c = blockIdx.x * 256 + threadIdx.x;
  const size_t scene_off = (size_t)blockIdx.y * (a.T + 1) * cells;
  short first = kPlanNeverBlocked;
  for (int t = a.T; t >= 0; --t) {
    if (a.blk[scene_off + (size_t)t * cells + c]) first = (short)t;
    a.nb[scene_off + (size_t)t * cells + c] = first;
  }
}

struct PlanSmoothTimeArgs {
  PlanPathArgs p;    // k_plan_path's inputs and outputs; occ [S][T + 1][G][G], field [F][T + 1][G][G]
  int T;
  const short* nb;   // [S][T + 1][G][G] k_plan_next_blocked's
  int* leave;        // [N][K] out (zeroed by the host): the action index of waypoint k's anchor
  int* arrive;       // [N] out: actions of the whole walk
  int* moves;        // [N] out: those of them that are moves
};

__global__ __launch_bounds__(64) void k_plan_smooth_time(PlanSmoothTimeArgs s) {
  __shared__ unsigned short ring[kPlanRing];
  plan_smooth<true>(s, ring);
}

// ---- smoothing of a team plan (mobrob_ppo_plan_grid_team_smooth; the rule: goal_rules.grid_leg_cells / grid_reserve_legs /
// grid_plan_team(smooth=True)) ------------------------------------------------------------------------------------------------------
// k_plan_team with line-of-sight legs.  A smoothed leg is reserved as a SWEPT region: every cell of its supercover (both ends, every
// cell stepped into, both cells at a corner), dilated by r, in EVERY layer of its span, so the member may be anywhere on the leg at
// any time of the span.  The earlier members' reservations are a byte map of this workgroup in global scratch, res [T + 1][G][G]; it
// replaces k_plan_team's Chebyshev test against c[t], c[t + 1] and its tail stamps.  The member's map occ_t = base_t OR res_t gives
// its field, its walk and ITS next-blocked table nb (k_plan_next_blocked's meaning, at the margin), all in this workgroup's scratch.
// Legs are capped at max_leg actions: a long leg reserves all of itself for all of its span.
struct PlanTeamSmoothArgs {
  PlanTeamArgs t;     // k_plan_team's, with t.wg: per workgroup plan_team_smooth_wg_bytes(G, T) bytes: field int [T + 1][G][G] | nb short
                      // [T + 1][G][G] | res byte [T + 1][G][G] | wk: the walk's cells c[0 .. A], packed iy * 128 + ix, 2 bytes each | kp:
                      // the kept indices, 2 bytes each;  t.out: n_waypoints | count | status | cost | arrive | sweeps | moves, [N] each |
                      // waits [N][K] (left zero) | leave [N][K] | waypoints [N][K][P] (float); from waits on zeroed by the host
  int margin;         // 0 or 1: the cells a leg keeps clear on either side
  int max_leg;        // >= 1: the actions of a leg at most
  int keep_cap;       // entries per robot in `keep`
  int* keep;          // [N][keep_cap] out or null (zeroed by the host): the first min(count - 1, keep_cap) kept indices
};
// entries of wk and of kp: a walk has at most T + G * G actions
__host__ __device__ inline size_t plan_team_smooth_walk_cap(int G, int T) { return ((size_t)T + (size_t)G * G + 8) & ~(size_t)7; }
__host__ __device__ inline size_t plan_team_smooth_wg_bytes(int G, int T) {
  return (size_t)(T + 1) * G * G * 7 + plan_team_smooth_walk_cap(G, T) * 4;
}
// LDS bytes of k_plan_team_smooth: k_plan_field_time's two layers and one byte per cell, then 16 words handed from phase to phase
inline size_t plan_team_smooth_lds_bytes(int G) { return (size_t)G * G * (2 * sizeof(int) + 1) + 64; }

struct PlanTeamSmoothWg {
  int* field;
  short* nb;
  unsigned char* res;
  unsigned short* wk;
  unsigned short* kp;
};
__device__ __forceinline__ PlanTeamSmoothWg plan_team_smooth_wg(const PlanTeamSmoothArgs& s) {
  const int G = s.t.g.G, T = s.t.T;
  const size_t lc = (size_t)(T + 1) * G * G;
  char* base = reinterpret_cast<char*>(s.t.wg) + blockIdx.x * plan_team_smooth_wg_bytes(G, T);
  PlanTeamSmoothWg w;
  w.field = reinterpret_cast<int*>(base);
  w.nb = reinterpret_cast<short*>(base + lc * 4);
  w.res = reinterpret_cast<unsigned char*>(base + lc * 6);
  w.wk = reinterpret_cast<unsigned short*>(base + lc * 7);
  w.kp = w.wk + plan_team_smooth_walk_cap(G, T);
  return w;
}

// Where "reserved" comes from in the field of a member of k_plan_team_smooth: the workgroup's byte map res, tail and layers alike.  The
// field pass also writes the member's next-blocked table.
struct PlanReservedSwept {
  using Args = PlanTeamSmoothArgs;
  static constexpr bool kNextBlocked = true;
  int* field;
  short* nb;
  const unsigned char* res;
  int cells, T, margin;
  __device__ __forceinline__ PlanReservedSwept(const Args& s, int, int*) : cells(s.t.g.G * s.t.g.G), T(s.t.T), margin(s.margin) {
    const PlanTeamSmoothWg wg = plan_team_smooth_wg(s);
    field = wg.field;
    nb = wg.nb;
    res = wg.res;
  }
  __device__ __forceinline__ static const PlanTeamArgs& team(const Args& s) { return s.t; }
  // both bytes are loaded whatever the first holds: two loads in flight, no branch between them
  __device__ __forceinline__ bool tail(int c, bool base) const { return base | (res[T * cells + c] != 0); }
  __device__ __forceinline__ bool layer(int t, int c, bool base) const { return base | (res[t * cells + c] != 0); }
};

// The walk of one member, by one thread: plan_team_walk's loop on this workgroup's scratch field, ending where d_t[c] == 0.  It leaves
// ALL of c[0 .. A] in wk (global scratch: the smoothing reads any of them) and hands over hand[0] = A, [1] = status, [2] = cost,
// [3] = moves.  A member without a walk: c[0] = its start cell, A = 0.
__device__ __noinline__ void plan_team_smooth_walk(const PlanTeamSmoothArgs* __restrict__ sp, int n, int sweeps, int* hand) {
  const PlanTeamArgs& a = sp->t;
  const int G = a.g.G, T = a.T, cells = G * G, P = a.P;
  const PlanTeamSmoothWg wg = plan_team_smooth_wg(*sp);
  const int* field = wg.field;
  unsigned short* wk = wg.wk;
  unsigned short* wout = a.walk ? a.walk + n * a.walk_cap : nullptr;
  const float* st = a.in + n * P;
  int ix = plan_cell(a.g, st[0]), iy = plan_cell(a.g, st[1]);
  int status = kPlanned, cost = -1, acts = 0, moves = 0;
  wk[0] = (unsigned short)(iy * 128 + ix);
  if (wout) wout[0] = wk[0];
  const int d0 = field[iy * G + ix];
  if (sweeps < 0) {
    status = kPlanUnconverged;
  } else if (d0 < 0 || d0 >= kPlanInf) {
    status = kPlanUnreachable;
  } else {
    cost = d0;
    int prev = -1;
    for (;;) {
      const int dc = field[min(acts, T) * cells + iy * G + ix];
      if (dc == 0) break;
      if (acts >= T + cells) { status = kPlanUnconverged; break; }
      const int dir = plan_team_step(field, G, T, acts, dc, ix, iy, prev);
      if (dir < 0) { status = kPlanUnconverged; break; }   // not a team field of these layers: cannot happen after a converged tail
      ++acts;
      if (dir != 8) {
        ix += plan_dx(dir); iy += plan_dy(dir);
        prev = dir;
        ++moves;
      }
      const unsigned short cell = (unsigned short)(iy * 128 + ix);   // c[acts]; acts <= T + cells < plan_team_smooth_walk_cap
      wk[acts] = cell;
      if (wout && acts < a.walk_cap) wout[acts] = cell;
    }
  }
  if (status != kPlanned) {   // parked: the start cell alone; nothing of a walk that was given up is handed out
    if (wout)
      for (int j = 1; j < min(acts + 1, a.walk_cap); ++j) wout[j] = 0;
    acts = 0; moves = 0; cost = -1;
  }
  hand[0] = acts; hand[1] = status; hand[2] = cost; hand[3] = moves;
}

// The smoothing of one member, by the workgroup's first wave: plan_smooth<true>'s window on the finished walk.  With the anchor c[i]
// and base = i + 2, lane l tests the leg to c[base + l] on nb[min(i, T)] against the threshold min(base + l, T), and its length base +
// l - i against max_leg.  The first lane that fails, z = ctz(ballot), is the rule's first hidden or over-cap index: c[base + z - 1] is
// kept and becomes the anchor.  Lane 0 writes the member's outputs and hands over hand[0] = A, hand[4] = the number of kept indices.
__device__ __noinline__ void plan_team_smooth_legs(const PlanTeamSmoothArgs* __restrict__ sp, int n, int sweeps, int* hand) {
  const PlanTeamArgs& a = sp->t;
  const int G = a.g.G, T = a.T, cells = G * G, P = a.P, K = a.K, N = a.N, lane = threadIdx.x;
  const int max_leg = sp->max_leg, keep_cap = sp->keep_cap;
  const PlanTeamSmoothWg wg = plan_team_smooth_wg(*sp);
  const short* nb = wg.nb;
  const unsigned short* wk = wg.wk;
  unsigned short* kp = wg.kp;
  const float* gl = a.in + (N + n) * P;
  int* leave = a.out + 7 * N + N * K + n * K;
  float* wp = reinterpret_cast<float*>(a.out + 7 * N + 2 * N * K) + n * K * P;
  int* keep = sp->keep ? sp->keep + n * keep_cap : nullptr;
  int A = hand[0], status = hand[1], cost = hand[2], moves = hand[3];
  int count = 0;
  if (status == kPlanned) {
    int ai = 0, base = 2;                              // the anchor's action index
    int ax = wk[0] & 127, ay = wk[0] >> 7;             // and its cell
    for (int round = 0; base <= A; ++round) {
      if (round > T + cells) { status = kPlanUnconverged; break; }
      const int idx = base + lane;
      bool hidden = false;
      if (idx <= A) {
        const int c = wk[idx];
        hidden = idx - ai > max_leg || !plan_los_time(nb + min(ai, T) * cells, min(idx, T), G, ax, ay, c & 127, c >> 7);
      }
      const unsigned long long fails = __ballot(hidden);
      if (fails == 0) { base += 64; continue; }
      const int j = base + __builtin_ctzll(fails) - 1;   // the last index within the cap and in sight: kept, the next anchor
      const int c = __builtin_amdgcn_readfirstlane((int)wk[j]);
      ax = c & 127; ay = c >> 7; ai = j;
      if (lane == 0) {
        kp[count] = (unsigned short)j;                   // count <= A - 1 < plan_team_smooth_walk_cap
        if (keep && count < keep_cap) keep[count] = j;
      }
      plan_emit(wp, count, K, P, a.g, ax, ay, gl, lane == 0);
      ++count;
      if (count < K && lane == 0) leave[count] = j;      // the anchor of the waypoint that follows
      base = j + 2;
    }
    if (status == kPlanned) status = plan_close(wp, count, K, P, gl, lane == 0);
  }
  if (lane != 0) return;
  int kept = count > 0 ? count - 1 : 0;
  if (status == kPlanUnconverged) {   // the member parks
    if (keep)
      for (int q = 0; q < min(count, keep_cap); ++q) keep[q] = 0;
    plan_give_up(wp, count, cost, K, P);
    for (int q = 0; q < K; ++q) leave[q] = 0;
    if (a.walk)
      for (int q = 1; q < min(A + 1, a.walk_cap); ++q) a.walk[n * a.walk_cap + q] = 0;
    A = 0; moves = 0; kept = 0;
  }
  hand[0] = A;
  hand[4] = kept;
  int* o = a.out + n;
  plan_result(o, o + N, o + 2 * N, o + 3 * N, count, K, status, cost);
  o[4 * N] = A;
  o[5 * N] = sweeps;
  o[6 * N] = moves;
}

// The reservation of one member, by all threads: a wave per leg, a lane per layer of the leg's span.  The leg (a, b) goes into the layers
// min(a, T) .. min(b - 1, T): a leg of one action as its two cells, a longer one as plan_los's supercover of c[a] .. c[b], cell by
// cell, both cells at a corner.  One more "leg" is the end cell c[A] in the layers min(A, T) .. T; for a parked member (A = 0) that is
// its start cell in every layer.  A round of the walk leaves one cell to stamp, or three at a corner; every cell goes through the one
// loop over the (2 r + 1)^2 cells around it, which writes only those in the grid (the ends are cells of the walk and the supercover
// stays inside their bounding box, so the centres are in the grid themselves).
// The traversal is plan_los's, written out: the stamp funnels the one or three cells of a round through ONE copy of the stamping
// loop, where plan_los's shape (a predicate called at four places) would inline that loop four times.
__device__ __noinline__ void plan_team_smooth_stamp(const PlanTeamSmoothArgs* __restrict__ sp, const int* hand) {
  const PlanTeamArgs& a = sp->t;
  const int G = a.g.G, T = a.T, cells = G * G, r = a.reserve, w = 2 * r + 1, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const PlanTeamSmoothWg wg = plan_team_smooth_wg(*sp);
  const int A = hand[0], kept = hand[4], legs = A > 0 ? kept + 1 : 0;
#pragma unroll 1
  for (int leg = wave; leg <= legs; leg += kPlanFieldThreads / 64) {
    const int la = leg == legs ? A : (leg == 0 ? 0 : (int)wg.kp[leg - 1]);
    const int lb = leg == legs ? A : (leg == kept ? A : (int)wg.kp[leg]);
    const int hi = leg == legs ? T : min(lb - 1, T);
    const int ca = wg.wk[la], cb = wg.wk[lb];
    const int x1 = cb & 127, y1 = cb >> 7;
    const bool line = lb - la > 1;
    const int dx = abs(x1 - (ca & 127)), dy = abs(y1 - (ca >> 7)), sx = x1 > (ca & 127) ? 1 : -1, sy = y1 > (ca >> 7) ? 1 : -1;
#pragma unroll 1
    for (int t = min(la, T) + lane; t <= hi; t += 64) {
      unsigned char* layer = wg.res + t * cells;
      int x = ca & 127, y = ca >> 7, ix = 0, iy = 0;
      int qx1 = x1, qy1 = y1, qx2 = x, qy2 = y, nq = line ? 1 : 2;   // the first round: c[a], and c[b] of a leg of one action
#pragma unroll 1
      for (int it = 0; it <= 2 * G; ++it) {
#pragma unroll 1
        for (int q = 0; q < nq; ++q) {
          const int qx = q == 0 ? x : (q == 1 ? qx1 : qx2), qy = q == 0 ? y : (q == 1 ? qy1 : qy2);
#pragma unroll 1
          for (int k = 0; k < w * w; ++k) {
            const int xx = qx - r + k % w, yy = qy - r + k / w;
            if (xx >= 0 && xx < G && yy >= 0 && yy < G) layer[yy * G + xx] = 1;
          }
        }
        if (!line || !(ix < dx || iy < dy)) break;
        const int s = (1 + 2 * ix) * dy - (1 + 2 * iy) * dx;
        qx1 = x + sx; qy1 = y; qx2 = x; qy2 = y + sy;   // the two cells that share the corner, where s == 0
        nq = s == 0 ? 3 : 1;
        if (s <= 0) { x += sx; ++ix; }
        if (s >= 0) { y += sy; ++iy; }
      }
    }
  }
}

// One workgroup of 1024 threads takes one team at a time, as k_plan_team does.  Per member four phases, each a function that is not
// inlined and reads the arguments from memory (plan_team_field says why): the field and nb by all threads; the walk by thread 0; the
// smoothing by the first wave; the stamps by all threads.  Every hand-off through global memory -- the zeroed and the stamped
// reservation, the field and nb, the walk's cells, the kept indices -- is a workgroup-scope fence and then the barrier; the handed
// words are in LDS, which the barrier orders.  Bounds: G * G sweeps, T + G * G actions, T + G * G window rounds, 2 G steps a sight
// line: status 3 and zeroed outputs beyond, and the member parks.
__global__ __launch_bounds__(kPlanFieldThreads) void k_plan_team_smooth(const PlanTeamSmoothArgs* __restrict__ sp) {
  extern __shared__ __attribute__((aligned(16))) int plan_team_smooth_lds[];
  const int G = sp->t.g.G, T = sp->t.T, cells = G * G, tid = threadIdx.x, size = sp->t.size, n_teams = sp->t.n_teams;
  int* hand = plan_team_smooth_lds + 2 * cells + cells / 4;   // behind d, e and the byte map
  for (int team = blockIdx.x; team < n_teams; team += gridDim.x) {
    int* res4 = reinterpret_cast<int*>(plan_team_smooth_wg(*sp).res);   // (T + 1) * cells bytes, a multiple of 4096, 16-aligned
#pragma unroll 1
    for (int i = tid; i < (T + 1) * (cells / 4); i += kPlanFieldThreads) res4[i] = 0;
    __threadfence_block();
    __syncthreads();
    for (int m = 0; m < size; ++m) {
      const int n = team * size + m;
      const int sweeps = plan_team_field<PlanReservedSwept>(sp, n, m, plan_team_smooth_lds);
      __threadfence_block();
      __syncthreads();
      if (tid == 0) plan_team_smooth_walk(sp, n, sweeps, hand);
      __threadfence_block();
      __syncthreads();
      if (tid < 64) plan_team_smooth_legs(sp, n, sweeps, hand);
      __threadfence_block();
      __syncthreads();
      plan_team_smooth_stamp(sp, hand);
      __threadfence_block();
      __syncthreads();
    }
  }
}

// ---- goal assignment inside a team (mobrob_ppo_plan_assign; the rule: goal_rules.grid_assign / plan_assign_match / plan_assign_team) --
// Who takes which goal: per team the minimum-cost perfect matching on C[i][j] = the static cost-to-go of member i's start cell to
// member j's goal cell, a pair without a path as kPlanAssignNone.  Two kernels behind the base map: k_plan_assign_cost (a workgroup per
// robot: its goal's field in LDS, of which only the mates' start cells leave the workgroup) and k_plan_assign (a wave per team).
constexpr int kPlanAssignNone = 1 << 21;     // above 16 * 7 * 128 * 128, the largest total of real costs
constexpr int kPlanAssignForbid = 1 << 26;   // in a makespan matching: a pair above the bottleneck
constexpr long long kPlanAssignBig = 1ll << 62;   // "no slack yet" in a scan
constexpr int kPlanAssignBisect = 32;        // steps of the bisection for the bottleneck at most: the values lie below 2^27

struct PlanAssignCostArgs {
  PlanGrid g;
  int N, P, size;
  const float* start;         // [N][P]
  const float* goal;          // [N][P]
  const int* scene;           // [N] or null: every robot in scene 0
  const unsigned char* occ;   // the cost map of scene s: occ + s * scene_stride + map_off, [G][G]
  size_t scene_stride, map_off;
  int* cost;                  // [N / size][size][size] out
  int* sweeps;                // [N] out: plan_tail's
};

// Grid N, 1024 threads, LDS plan_field_lds_bytes(G): plan_tail on the map of robot n's scene for robot n's goal cell, k_plan_field's
// field, which stays in LDS.  Out go the `size` words C[team][i][n % size], the field at the start cells of n's team (a blocked
// start cell holds kPlanInf in the field: no path), and the sweeps.  A tail that hit its bound leaves kPlanAssignNone in its column;
// k_plan_assign reads the sweeps and reports the team.
__global__ __launch_bounds__(kPlanFieldThreads) void k_plan_assign_cost(PlanAssignCostArgs a) {
  extern __shared__ __attribute__((aligned(16))) int plan_assign_lds[];
  const int n = blockIdx.x, G = a.g.G, cells = G * G, tid = threadIdx.x, m = n % a.size;
  int* d = plan_assign_lds;
  unsigned char* moves = reinterpret_cast<unsigned char*>(plan_assign_lds + cells);
  const float* gl = a.goal + (size_t)n * a.P;
  const int goal = plan_cell(a.g, gl[1]) * G + plan_cell(a.g, gl[0]);
  const unsigned char* occ = a.occ + (size_t)(a.scene ? a.scene[n] : 0) * a.scene_stride + a.map_off;
  const int sweeps = plan_tail(d, moves, plan_unblocked(occ), goal, G);
  if (tid < a.size) {
    const int i = n - m + tid;   // a mate, or n itself
    const float* st = a.start + (size_t)i * a.P;
    const int v = d[plan_cell(a.g, st[1]) * G + plan_cell(a.g, st[0])];
    a.cost[(size_t)i * a.size + m] = (sweeps < 0 || v >= kPlanInf) ? kPlanAssignNone : v;
  }
  if (tid == 0) a.sweeps[n] = sweeps;
}

struct PlanAssignArgs {
  int N, P, size, objective;   // objective 0: sum, 1: makespan
  const float* goal;           // [N][P]
  const int* sweeps;           // [N] k_plan_assign_cost's
  int* cost;                   // [N / size][size][size] in; out: kPlanAssignNone as -1
  int* assign;                 // [N] out
  float* goal_out;             // [N][P] out
  int* assign_cost;            // [N] out
  long long* total;            // [n_teams] out, then the identity's [n_teams]
  int* team;                   // max | identity max | changed | status, [n_teams] each, out
  long long* u;                // [N] out
  long long* v;                // [N] out
};

// the least (value, lane) over the 16 lanes of a team, the lower lane on equal values, in every one of the 16 lanes
__device__ __forceinline__ void plan_assign_argmin(long long& best, int& at) {
#pragma unroll
  for (int s = 1; s < kPlanTeamMax; s <<= 1) {
    const long long ob = __shfl_xor(best, s);
    const int oa = __shfl_xor(at, s);
    if (ob < best || (ob == best && oa < at)) { best = ob; at = oa; }
  }
}
__device__ __forceinline__ long long plan_assign_sum(long long x) {
#pragma unroll
  for (int s = 1; s < kPlanTeamMax; s <<= 1) x += __shfl_xor(x, s);
  return x;
}
__device__ __forceinline__ int plan_assign_max(int x) {
#pragma unroll
  for (int s = 1; s < kPlanTeamMax; s <<= 1) x = max(x, __shfl_xor(x, s));
  return x;
}

// goal_rules.plan_assign_match by one wave, lane l < size being column l AND row l: u the potential of row l, v of column l, p the row
// matched to column l (-1: none); per inserted row minv, way and used of column l and rowin of row l.  cost(i, l): the entry of row i
// in this lane's column.  The row that is scanned, the column that is taken and delta are the same in every lane (broadcast from lane
// 0), so the loops are wave-uniform.  Bounds, constants of the rule: size rows, size + 1 scans a row (row i reaches at most i + 1
// columns), size + 1 steps back along the way -> false beyond (cannot happen).
template <class Cost>
__device__ __forceinline__ bool plan_assign_match(Cost cost, int size, int lane, long long& u, long long& v, int& p) {
  u = 0; v = 0; p = -1;
  for (int i = 0; i < size; ++i) {
    long long minv = kPlanAssignBig;
    int way = -1, j0 = -1, i0 = i;
    bool used = false, rowin = false;
    for (int scan = 0;; ++scan) {
      if (scan > size) return false;
      if (lane == i0) rowin = true;
      const long long ui0 = __shfl(u, i0);
      const bool open = lane < size && !used;
      if (open) {
        const long long cur = cost(i0, lane) - ui0 - v;
        if (cur < minv) { minv = cur; way = j0; }
      }
      long long delta = open ? minv : kPlanAssignBig;
      int j1 = lane;
      plan_assign_argmin(delta, j1);
      delta = __shfl(delta, 0);
      j1 = __shfl(j1, 0);
      if (rowin) u += delta;
      if (lane < size) {
        if (used) v -= delta; else minv -= delta;
      }
      j0 = j1;
      if (lane == j0) used = true;
      i0 = __shfl(p, j0);
      if (i0 < 0) break;
    }
    for (int step = 0; j0 >= 0; ++step) {   // augment along the way back to the root
      if (step > size) return false;
      const int j1 = __shfl(way, j0);
      const int row = j1 >= 0 ? __shfl(p, j1) : i;
      if (lane == j0) p = row;
      j0 = j1;
    }
  }
  return true;
}

// Grid n_teams, 64 threads: the workgroup IS the wave (as k_plan_smooth's), so nothing here waits for another wave; lane l < size is
// column l and row l of the team's matrix, the other lanes idle along.  The matrix sits in LDS, [16][16] ints, written and read by
// this one wave around wave-level fences.  goal_rules.plan_assign_team: the matching of the sum, or for the makespan first the
// bottleneck L -- a bisection on the VALUE between the largest row minimum (no matching does better) and the identity's largest entry
// (the identity is a matching), a value being feasible where the 0 / 1 matrix C > value has a matching of total 0; the least feasible
// value is an entry, so it is the rule's L -- and then the matching on C with the entries above L as kPlanAssignForbid.  Identity
// first, the totals, the outputs.  A field that did not converge, or a loop beyond its bound: status 3, the identity, potentials 0.
__global__ __launch_bounds__(64) void k_plan_assign(PlanAssignArgs a) {
  __shared__ int cm[kPlanTeamMax * kPlanTeamMax];
  __shared__ int colof[kPlanTeamMax];
  const int team = blockIdx.x, lane = threadIdx.x, size = a.size, base = team * size, n_teams = a.N / size;
  const bool mine = lane < size;
  int* cg = a.cost + (size_t)base * size;
  bool ok = true;
  if (mine) {
    for (int i = 0; i < size; ++i) cm[i * kPlanTeamMax + lane] = cg[i * size + lane];
    ok = a.sweeps[base + lane] >= 0;
  }
  ok = __all(ok);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int* const c16 = cm;   // the matrix, row i at c16 + 16 i
  const auto raw = [c16](int i, int j) { return (long long)c16[i * kPlanTeamMax + j]; };
  const int diag = mine ? cm[lane * kPlanTeamMax + lane] : 0;
  const long long id_total = plan_assign_sum(diag);
  const int id_max = plan_assign_max(diag);
  long long u = 0, v = 0;
  int p = -1;
  if (ok) {
    if (a.objective == 0) {
      ok = plan_assign_match(raw, size, lane, u, v, p);
    } else {
      int rowmin = 0;
      if (mine) {
        rowmin = cm[lane * kPlanTeamMax];
        for (int j = 1; j < size; ++j) rowmin = min(rowmin, cm[lane * kPlanTeamMax + j]);
      }
      int lo = plan_assign_max(rowmin), hi = id_max;
      lo = __shfl(lo, 0); hi = __shfl(hi, 0);
      for (int step = 0; ok && lo < hi; ++step) {
        if (step >= kPlanAssignBisect) { ok = false; break; }
        const int mid = lo + (hi - lo) / 2;
        const auto above = [c16, mid](int i, int j) { return (long long)(c16[i * kPlanTeamMax + j] > mid ? 1 : 0); };
        ok = plan_assign_match(above, size, lane, u, v, p);
        long long over = mine && p >= 0 ? above(p, lane) : 0;
        over = __shfl(plan_assign_sum(over), 0);
        if (over == 0) hi = mid; else lo = mid + 1;
      }
      if (ok) {
        const int L = lo;
        const auto capped = [c16, L](int i, int j) {
          const int c = c16[i * kPlanTeamMax + j];
          return (long long)(c > L ? kPlanAssignForbid : c);
        };
        ok = plan_assign_match(capped, size, lane, u, v, p);
      }
    }
  }
  ok = __all(ok);
  if (!ok) { u = 0; v = 0; p = lane; }
  // the row of column `lane` -> the column of row `lane`
  if (mine) colof[p] = lane;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  int col = mine ? colof[lane] : 0;
  int picked = mine ? cm[lane * kPlanTeamMax + col] : 0;
  long long total = plan_assign_sum(picked);
  int most = plan_assign_max(picked);
  if (total == id_total && (a.objective == 0 || most == id_max)) {   // identity first
    col = lane; picked = diag; most = id_max;
  }
  const bool changed = __any(mine && col != lane);
  if (mine) {
    const int n = base + lane;
    a.assign[n] = base + col;
    for (int j = 0; j < a.P; ++j) a.goal_out[(size_t)n * a.P + j] = a.goal[(size_t)(base + col) * a.P + j];
    a.assign_cost[n] = picked >= kPlanAssignNone ? -1 : picked;
    a.u[n] = u;
    a.v[n] = v;
    for (int i = 0; i < size; ++i)
      if (cm[i * kPlanTeamMax + lane] >= kPlanAssignNone) cg[i * size + lane] = -1;
  }
  if (lane == 0) {
    a.total[team] = total;
    a.total[n_teams + team] = id_total;
    a.team[team] = most;
    a.team[n_teams + team] = id_max;
    a.team[2 * n_teams + team] = changed ? 1 : 0;
    a.team[3 * n_teams + team] = ok ? kPlanned : kPlanUnconverged;
  }
}

// ---- clearance-aware static plans (mobrob_ppo_plan_grid_clear, mobrob_ppo_plan_smooth_clear; the rule: goal_rules.grid_clearance /
// grid_surcharge / grid_field_cost / grid_walk_cost / grid_walk_clearance) ---------------------------------------------------------
// Entering the free cell c' costs the move plus pen[c'] = weight * max(0, reach + 1 - clearance[c']), clearance the Chebyshev distance
// in cells to the nearest blocked cell of the grid.  The kernels above are not touched: plan_tail and plan_step have their cost
// inside their loops, so the relaxation, the step and the two walk bodies are restated here with the surcharge in them (as
// follow_env_step and k_plan_team_rounds restate theirs), and the move mask with them (plan_moves_bytes: why, there); plan_los, plan_emit,
// plan_close, plan_give_up and plan_result are the ones above.
constexpr int kPlanClearReachMax = 8;
constexpr int kPlanClearWeightMax = 16;     // the largest surcharge, 16 * 8 = 128, fits a byte
constexpr unsigned char kPlanClearNone = 255;   // in a clearance map: no round has reached the cell yet

struct PlanSurchargeArgs {
  int G, reach, weight;
  const unsigned char* occ;   // [S][G][G]
  unsigned char* pen;         // [S][G][G] out: the surcharge of entering the cell, 0 on blocked cells
};

// One workgroup per scene, 1024 threads, two byte maps of the scene in LDS (32 KB at 128 cells).  A map holds per cell the round that
// reached it: 0 blocked, kPlanClearNone not yet.  Round r = 1 .. reach writes `nxt` from `cur` alone: a cell not yet reached with a
// reached cell in its 3 x 3 neighbourhood (cells outside the grid count as free) records r -- its Chebyshev distance to the nearest
// blocked cell.  One barrier a round puts nxt's stores before the next round's loads, and the map the next round overwrites was last
// read before that barrier.
__global__ __launch_bounds__(kPlanFieldThreads) void k_plan_surcharge(PlanSurchargeArgs a) {
  __shared__ unsigned char plan_clear_lds[2 * 128 * 128];
  const int G = a.G, cells = G * G, tid = threadIdx.x, gs = 31 - __clz(G), gm = G - 1;
  const unsigned char* occ = a.occ + (size_t)blockIdx.x * cells;
  unsigned char* cur = plan_clear_lds;
  unsigned char* nxt = plan_clear_lds + cells;
  for (int c = tid; c < cells; c += kPlanFieldThreads) cur[c] = occ[c] ? 0 : kPlanClearNone;
  __syncthreads();
  for (int r = 1; r <= a.reach; ++r) {
#pragma unroll 1
    for (int c = tid; c < cells; c += kPlanFieldThreads) {
      unsigned char v = cur[c];
      if (v == kPlanClearNone) {
        const int ix = c & gm, iy = c >> gs;
        bool reached = false;
        for (int y = max(iy - 1, 0); y <= min(iy + 1, G - 1); ++y)
          for (int x = max(ix - 1, 0); x <= min(ix + 1, G - 1); ++x) reached |= cur[y * G + x] != kPlanClearNone;
        if (reached) v = (unsigned char)r;
      }
      nxt[c] = v;
    }
    __syncthreads();
    unsigned char* const swap = cur; cur = nxt; nxt = swap;
  }
  unsigned char* pen = a.pen + (size_t)blockIdx.x * cells;
  for (int c = tid; c < cells; c += kPlanFieldThreads) {
    const int v = cur[c];   // 0 blocked, 1 .. reach, kPlanClearNone: beyond reach, no surcharge
    pen[c] = (v == 0 || v == kPlanClearNone) ? 0 : (unsigned char)(a.weight * (a.reach + 1 - v));
  }
}

struct PlanFieldCostArgs {
  int G;
  const unsigned char* occ;   // [S][G][G]
  const unsigned char* pen;   // [S][G][G] k_plan_surcharge's
  const int* field_goal;      // [F] goal cell
  const int* field_scene;     // [F]
  int* field;                 // [F][G][G] out: cost-to-go with surcharges, -1 blocked or unreachable
  int* sweeps;                // [F] out: sweeps run (the last one changed nothing), -1: the bound of G * G was hit
};

// plan_moves on occupancy bytes, restated without the predicate: instantiating plan_moves and plan_tail once more over plan_unblocked's
// lambda changed the compiled code of k_plan_field_time and of the team kernels' fields and walks (the register allocation, an
// instruction here and there), and the kernels above stay instruction for instruction what they were
__device__ __forceinline__ unsigned plan_moves_bytes(const unsigned char* occ, int G, int ix, int iy) {
  const int c = iy * G + ix;
  unsigned free4 = 0;   // E, N, W, S
  if (ix + 1 < G && !occ[c + 1]) free4 |= 1u;
  if (iy + 1 < G && !occ[c + G]) free4 |= 2u;
  if (ix > 0 && !occ[c - 1]) free4 |= 4u;
  if (iy > 0 && !occ[c - G]) free4 |= 8u;
  unsigned m = free4;
  if ((free4 & 3u) == 3u && !occ[c + G + 1]) m |= 16u;     // NE: E and N free
  if ((free4 & 6u) == 6u && !occ[c + G - 1]) m |= 32u;     // NW: N and W
  if ((free4 & 12u) == 12u && !occ[c - G - 1]) m |= 64u;   // SW: W and S
  if ((free4 & 9u) == 9u && !occ[c - G + 1]) m |= 128u;    // SE: S and E
  return m;
}

// LDS bytes of k_plan_field_cost: the field, one byte of moves and one byte of surcharge per cell (96 KB at 128 cells)
inline size_t plan_field_cost_lds_bytes(int G) { return (size_t)G * G * (sizeof(int) + 2); }

// plan_tail with the surcharge of the cell moved into: d[c] = min(d[nb] + w + pen[nb]).  plan_tail's argument holds as it stands: every
// value ever stored in d is the cost of a real path to the goal under these costs and values only decrease, so the in-place sweeps end
// in the fixed point, whatever the order; the bound of G * G sweeps stays.  `pen_scene` is the scene's map in global memory, staged
// into `pen` here, each cell by the thread that owns it, before the first barrier.
__device__ __forceinline__ int plan_tail_cost(int* d, unsigned char* moves, unsigned char* pen, const unsigned char* pen_scene,
                                              const unsigned char* occ, int goal, int G) {
  const int cells = G * G, tid = threadIdx.x, gs = 31 - __clz(G), gm = G - 1;
#pragma unroll 1
  for (int c = tid; c < cells; c += kPlanFieldThreads) {
    const bool blocked = occ[c] != 0;
    moves[c] = blocked ? 0 : (unsigned char)plan_moves_bytes(occ, G, c & gm, c >> gs);
    pen[c] = pen_scene[c];
    d[c] = (c == goal && !blocked) ? 0 : kPlanInf;
  }
  __syncthreads();
  for (int sweep = 1; sweep <= cells; ++sweep) {   // the hard bound: a field that needs more is reported, not waited for
    int changed = 0;
#pragma unroll 1
    for (int c = tid; c < cells; c += kPlanFieldThreads) {
      const unsigned m = moves[c];
      if (m == 0 || c == goal) continue;
      const int cur = d[c];
      int best = cur;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (m & (1u << k)) {
          const int nb = c + plan_dy(k) * G + plan_dx(k);
          best = min(best, d[nb] + plan_w(k) + (int)pen[nb]);   // kPlanInf + 7 + 128 stays an int
        }
      if (best < cur) { d[c] = best; changed = 1; }
    }
    __syncthreads();   // this sweep's stores before the next sweep's loads
    if (!__syncthreads_or(changed)) return sweep;
  }
  return -1;
}

// One workgroup per field, 1024 threads: plan_tail_cost on the scene's map and surcharges.
__global__ __launch_bounds__(kPlanFieldThreads) void k_plan_field_cost(PlanFieldCostArgs a) {
  extern __shared__ __attribute__((aligned(16))) int plan_field_cost_lds[];
  const int f = blockIdx.x, G = a.G, cells = G * G, tid = threadIdx.x;
  int* d = plan_field_cost_lds;
  unsigned char* moves = reinterpret_cast<unsigned char*>(plan_field_cost_lds + cells);
  unsigned char* pen = moves + cells;
  const size_t scene_off = (size_t)a.field_scene[f] * cells;
  const int sweeps = plan_tail_cost(d, moves, pen, a.pen + scene_off, a.occ + scene_off, a.field_goal[f], G);
  int* out = a.field + (size_t)f * cells;
  for (int c = tid; c < cells; c += kPlanFieldThreads) out[c] = d[c] >= kPlanInf ? -1 : d[c];
  if (tid == 0) a.sweeps[f] = sweeps;
}

// plan_step on a cost field: to a neighbour with d[nb] + w + pen[nb] == dc, the previous direction first, else the lowest index; -1:
// none (d is not the cost field of these moves and surcharges).  The field holds only -1 or finite costs.
__device__ __forceinline__ int plan_step_cost(unsigned m, int dc, const int* d, const unsigned char* pen, int G, int c, int prev) {
  const auto fits = [dc, d, pen](int nb, int w) { const int v = d[nb]; return v >= 0 && v + w + (int)pen[nb] == dc; };
  int dir = -1;
  for (int k = 7; k >= 0; --k)   // descending: the lowest qualifying index is kept
    if ((m & (1u << k)) && fits(c + plan_dy(k) * G + plan_dx(k), plan_w(k))) dir = k;
  if (prev >= 0 && (m & (1u << prev)) && fits(c + plan_dy(prev) * G + plan_dx(prev), plan_w(prev))) dir = prev;
  return dir;
}

struct PlanPathCostArgs {
  PlanPathArgs p;             // k_plan_path's inputs and outputs; field: k_plan_field_cost's
  const unsigned char* pen;   // [S][G][G]
  int reach, weight;
  int* clearance_min;         // [N] out: the least clearance (capped at reach + 1) over the cells entered, -1 without a walk
};

// the clearance of the walk's worst cell from its surcharge (a walk enters free cells only: pen = weight * (reach + 1 - clearance))
__device__ __forceinline__ int plan_clearance_of(int worst_pen, int reach, int weight) { return reach + 1 - worst_pen / weight; }

// Robot n's walk on a cost field, by one thread: plan_path<false> with plan_step_cost, and the largest surcharge met on the way
__device__ __forceinline__ void plan_path_cost(const PlanPathCostArgs& s, int n) {
  const PlanPathArgs& a = s.p;
  const int G = a.g.G, cells = G * G, P = a.P, K = a.K;
  const int f = a.field_of[n];
  const size_t scene_off = (size_t)a.field_scene[f] * cells;
  const unsigned char* occ = a.occ + scene_off;
  const unsigned char* pen = s.pen + scene_off;
  const int* d = a.field + (size_t)f * cells;
  const float* st = a.start + (size_t)n * P;
  const float* gl = a.goal + (size_t)n * P;
  float* wp = a.wp + (size_t)n * K * P;
  int ix = plan_cell(a.g, st[0]), iy = plan_cell(a.g, st[1]);
  const int gx = plan_cell(a.g, gl[0]), gy = plan_cell(a.g, gl[1]);
  int count = 0, status = kPlanned, cost = -1, acts = 0, worst = 0;
  if (a.sweeps[f] < 0) {
    status = kPlanUnconverged;
  } else if (d[iy * G + ix] < 0) {
    status = kPlanUnreachable;
  } else {
    cost = d[iy * G + ix];
    int prev = -1;
    while (ix != gx || iy != gy) {
      if (acts >= cells) { status = kPlanUnconverged; break; }
      const int c = iy * G + ix;
      const int dir = plan_step_cost(plan_moves_bytes(occ, G, ix, iy), d[c], d, pen, G, c, prev);
      if (dir < 0) { status = kPlanUnconverged; break; }   // not a field of these maps: cannot happen after a converged field kernel
      ++acts;
      if (prev >= 0 && dir != prev) {
        plan_emit(wp, count, K, P, a.g, ix, iy, gl, true);
        ++count;
      }
      ix += plan_dx(dir); iy += plan_dy(dir);
      worst = max(worst, (int)pen[iy * G + ix]);
      prev = dir;
    }
    if (status == kPlanned) status = plan_close(wp, count, K, P, gl, true);
  }
  if (status == kPlanUnconverged) plan_give_up(wp, count, cost, K, P);
  plan_result(a.nwp + n, a.count + n, a.status + n, a.cost + n, count, K, status, cost);
  s.clearance_min[n] = (status == kPlanned || status == kPlanTruncated) ? plan_clearance_of(worst, s.reach, s.weight) : -1;
}

// one thread per robot, 256 to a workgroup
__global__ __launch_bounds__(256) void k_plan_path_cost(PlanPathCostArgs s) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n < s.p.N) plan_path_cost(s, n);
}

struct PlanSmoothCostArgs {
  PlanPathCostArgs c;
  const unsigned char* blk;   // [S][G][G] cells that are not clear: occ (margin 0) or k_plan_dilate's map (margin 1)
  int* moves;                 // [N] out: moves of the walk, 0 where none was made
};

// Robot blockIdx.x's smoothed plan on a cost field, by one wave: plan_smooth<false> -- the ring of kPlanRing cells indexed by action,
// the window of 64 candidates tested against the anchor at once, the ballot, the wave-level fences and every bound as stated there --
// with plan_step_cost for the walk and the largest surcharge met on the way.  The sight lines never read costs.
__global__ __launch_bounds__(64) void k_plan_smooth_cost(PlanSmoothCostArgs s) {
  __shared__ unsigned short ring[kPlanRing];
  const PlanPathArgs& a = s.c.p;
  const int n = blockIdx.x, lane = threadIdx.x;
  const int G = a.g.G, cells = G * G, P = a.P, K = a.K;
  const int f = a.field_of[n];
  const size_t scene_off = (size_t)a.field_scene[f] * cells;
  const unsigned char* occ = a.occ + scene_off;
  const unsigned char* pen = s.c.pen + scene_off;
  const int* d = a.field + (size_t)f * cells;
  const float* st = a.start + (size_t)n * P;
  const float* gl = a.goal + (size_t)n * P;
  float* wp = a.wp + (size_t)n * K * P;
  int wx = plan_cell(a.g, st[0]), wy = plan_cell(a.g, st[1]);   // the walker
  const int gx = plan_cell(a.g, gl[0]), gy = plan_cell(a.g, gl[1]);
  int count = 0, status = kPlanned, cost = -1, walked = 1, moves = 0, worst = 0;   // walked: cells c[0 .. walked - 1] are known
  if (a.sweeps[f] < 0) {
    status = kPlanUnconverged;
  } else if (d[wy * G + wx] < 0) {
    status = kPlanUnreachable;
  } else {
    cost = d[wy * G + wx];
    int ax = wx, ay = wy, base = 2, prev = -1;   // the anchor's cell
    bool done = wx == gx && wy == gy;
    if (lane == 0) ring[0] = (unsigned short)(wy * 128 + wx);
    for (int round = 0;; ++round) {
      if (round > cells) { status = kPlanUnconverged; break; }
      while (!done && walked <= base + 63) {   // the walk, up to the end of the window
        if (walked > cells) { status = kPlanUnconverged; break; }
        const int c = wy * G + wx;
        const int dir = plan_step_cost(plan_moves_bytes(occ, G, wx, wy), d[c], d, pen, G, c, prev);
        if (dir < 0) { status = kPlanUnconverged; break; }
        wx += plan_dx(dir); wy += plan_dy(dir);
        worst = max(worst, (int)pen[wy * G + wx]);
        prev = dir;
        ++moves;
        if (lane == 0) ring[walked & (kPlanRing - 1)] = (unsigned short)(wy * 128 + wx);
        ++walked;
        done = wx == gx && wy == gy;
      }
      if (status != kPlanned) break;
      if (done && base >= walked) break;   // no candidate left
      // lane 0's stores to the ring before every lane's loads from it
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int idx = base + lane;
      bool hidden = false;
      if (idx < walked) {
        const int c = ring[idx & (kPlanRing - 1)];
        hidden = !plan_los(plan_blocked(s.blk + scene_off), G, ax, ay, c & 127, c >> 7);
      }
      const unsigned long long fails = __ballot(hidden);
      if (fails == 0) { base += 64; continue; }
      const int j = base + __builtin_ctzll(fails) - 1;   // the last visible index: emitted, the next anchor
      const int c = __builtin_amdgcn_readfirstlane((int)ring[j & (kPlanRing - 1)]);
      ax = c & 127; ay = c >> 7;
      plan_emit(wp, count, K, P, a.g, ax, ay, gl, lane == 0);
      ++count;
      base = j + 2;
      // the loads above before the walk's next stores to the ring
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    if (status == kPlanned) status = plan_close(wp, count, K, P, gl, lane == 0);
  }
  if (lane != 0) return;
  if (status == kPlanUnconverged) {
    plan_give_up(wp, count, cost, K, P);
    moves = 0;
  }
  plan_result(a.nwp + n, a.count + n, a.status + n, a.cost + n, count, K, status, cost);
  s.moves[n] = moves;
  s.c.clearance_min[n] = (status == kPlanned || status == kPlanTruncated) ? plan_clearance_of(worst, s.c.reach, s.c.weight) : -1;
}

}  // namespace mobrob
