// Run specifications (mobrob_ppo_spec_monitor): reach / avoid / until robustness per robot, folded from the positions of a run.
//
// The rule, stated once in array form in mobrob_amd/envs/goal_rules.py (region_margins, spec_predicate, spec_fold): a scene is up to
// 64 regions -- kind 0 a box (cx, cy, hx, hy), kind 1 a circle (cx, cy, r, 0) --, the inside margin of a region at xy p is
//   box: -wall_sdf(p)          circle: r - sqrt(dx * dx + dy * dy),  dx = px - cx  (every operation rounded on its own, no fma)
// a predicate (lo, hi, outside) is u = max of the margins lo .. min(hi, count) - 1 by explicit > in ascending order (-inf when the
// range is empty), negated for `outside`, and a clause (op, a, b, pred1, pred2) folds the sample at tau into (rho, guard, witness):
//   ALWAYS      a <= tau <= b and v1 < rho: rho = v1, witness = tau
//   EVENTUALLY  a <= tau <= b and v1 > rho: rho = v1, witness = tau
//   UNTIL       v1 < guard: guard = v1;  then a <= tau <= b: w = v2 < guard ? v2 : guard;  w > rho: rho = w, witness = tau
// Every comparison is the rule's own (strict, explicit): no fminf / fmaxf where a tie or a signed zero could pick differently.
//
// k_spec_monitor: one lane per robot, one wave per workgroup (4096 robots: 64 workgroups on 64 CUs).  The path is time-major
// [T + 1][N][P], so a record is one coalesced read of the wave; records are fetched kSpecBatch at a time into registers while the
// previous batch, parked in LDS, is folded -- the only latency the wave has to hide is that of its own next batch.  The clause table
// and a shared scene's regions sit in LDS (uniform reads); per-robot scenes are read through scene[i].  Every region margin is
// computed once per sample into the lane's column of an LDS block [64][64] and the predicates read their ranges from it; the
// carried (rho, guard, witness) of all 16 clauses stay in registers across the time loop (the clause loop is unrolled: no dynamic
// register index).
#pragma once
#include "kernels_wall.h"

namespace mobrob {

constexpr int kSpecRegionsMax = 64;   // regions per scene
constexpr int kSpecClausesMax = 16;   // clauses of a specification
constexpr int kSpecBatch = 8;         // records in flight per lane
constexpr int kSpecAlways = 0, kSpecEventually = 1, kSpecUntil = 2;
constexpr int kSpecClauseWords = 9;   // op, a, b, lo1, hi1, out1, lo2, hi2, out2

struct SpecArgs {
  const float* path;      // [T + 1][N][P]
  const float* regions;   // [S][R][4]
  const int* kinds;       // [S][R]
  const int* nreg;        // [S]
  const int* scene;       // [N] or null (S == 1: the scene is staged in LDS)
  const int* clauses;     // [C][kSpecClauseWords]
  float* val;             // [N][C][2] rho, guard: in / out
  int* wit;               // [N][C] in / out
  int N, T, P, R, C;
  int r0;                 // first record to sample (0, or 1 in a continued call)
  int tau0;               // tau of record r is tau0 + r
};

// LDS words of k_spec_monitor: margins [64][64] | batch x [kSpecBatch][64] | batch y | clauses | shared regions [R][4] | kinds [R]
constexpr int kSpecLdsMargins = 0;
constexpr int kSpecLdsX = kSpecLdsMargins + kSpecRegionsMax * 64;
constexpr int kSpecLdsY = kSpecLdsX + kSpecBatch * 64;
constexpr int kSpecLdsClauses = kSpecLdsY + kSpecBatch * 64;
constexpr int kSpecLdsRegions = kSpecLdsClauses + kSpecClausesMax * kSpecClauseWords;
constexpr int kSpecLdsKinds = kSpecLdsRegions + kSpecRegionsMax * 4;
constexpr int kSpecLdsWords = kSpecLdsKinds + kSpecRegionsMax;

// the inside margin of one region at (px, py)
__device__ __forceinline__ float spec_margin(float px, float py, float c0, float c1, float e2, float e3, int kind) {
  if (kind == 0) return -wall_sdf(px, py, c0, c1, e2, e3);
  const float dx = __fsub_rn(px, c0), dy = __fsub_rn(py, c1);
  // kernels_hazard.h's distance with the root taken as wall_sdf takes it: sqrtf is correctly rounded, the root intrinsic is not
  const float d = sqrtf(__fadd_rn(rounded(__fmul_rn(dx, dx)), rounded(__fmul_rn(dy, dy))));
  return __fsub_rn(e2, d);
}

// the value of the predicate (lo, hi, out) from the lane's column of margins; count: the regions of the lane's scene
__device__ __forceinline__ float spec_predicate(const float* mg, int lo, int hi, int out, int count) {
  float u = -__builtin_inff();
  const int end = hi < count ? hi : count;
  for (int r = lo; r < end; ++r) {
    const float m = mg[r * 64];
    if (m > u) u = m;
  }
  return out ? -u : u;
}

__global__ __launch_bounds__(64) void k_spec_monitor(SpecArgs a) {
  __shared__ float lds[kSpecLdsWords];
  const int lane = threadIdx.x;
  const int n = blockIdx.x * 64 + lane;
  const bool live = n < a.N;
  const int i = live ? n : a.N - 1;   // a lane past the last robot folds the last robot's rows and stores nothing
  float* mg = lds + kSpecLdsMargins + lane;
  float* bx = lds + kSpecLdsX + lane;
  float* by = lds + kSpecLdsY + lane;
  int* cl = reinterpret_cast<int*>(lds + kSpecLdsClauses);
  float* sreg = lds + kSpecLdsRegions;
  int* skind = reinterpret_cast<int*>(lds + kSpecLdsKinds);
  for (int w = lane; w < a.C * kSpecClauseWords; w += 64) cl[w] = a.clauses[w];
  const bool shared = a.scene == nullptr;
  if (shared) {
    for (int w = lane; w < a.R * 4; w += 64) sreg[w] = a.regions[w];
    for (int w = lane; w < a.R; w += 64) skind[w] = a.kinds[w];
  }
  const int s = shared ? 0 : a.scene[i];
  const int count = a.nreg[s];
  const float* greg = a.regions + (size_t)s * a.R * 4;
  const int* gkind = a.kinds + (size_t)s * a.R;
  __syncthreads();

  float rho[kSpecClausesMax], guard[kSpecClausesMax];
  int wit[kSpecClausesMax];
#pragma unroll
  for (int c = 0; c < kSpecClausesMax; ++c) {
    if (c < a.C) {
      rho[c] = a.val[((size_t)i * a.C + c) * 2];
      guard[c] = a.val[((size_t)i * a.C + c) * 2 + 1];
      wit[c] = a.wit[(size_t)i * a.C + c];
    } else {
      rho[c] = 0.f; guard[c] = 0.f; wit[c] = -1;
    }
  }

  const size_t stride = (size_t)a.N * a.P;   // floats between two records
  const float* row = a.path + (size_t)i * a.P;
  const bool has_y = a.P > 1;
  float nx[kSpecBatch], ny[kSpecBatch];
#pragma unroll
  for (int u = 0; u < kSpecBatch; ++u) {
    const int r = a.r0 + u;
    nx[u] = 0.f; ny[u] = 0.f;
    if (r <= a.T) {
      nx[u] = row[(size_t)r * stride];
      if (has_y) ny[u] = row[(size_t)r * stride + 1];
    }
  }
  for (int rb = a.r0; rb <= a.T; rb += kSpecBatch) {
    // park the batch that has arrived, then ask for the next one: it travels while this one is folded
#pragma unroll
    for (int u = 0; u < kSpecBatch; ++u) { bx[u * 64] = nx[u]; by[u * 64] = ny[u]; }
#pragma unroll
    for (int u = 0; u < kSpecBatch; ++u) {
      const int r = rb + kSpecBatch + u;
      if (r <= a.T) {
        nx[u] = row[(size_t)r * stride];
        if (has_y) ny[u] = row[(size_t)r * stride + 1];
      }
    }
    const int left = a.T - rb + 1;
    const int cnt = left < kSpecBatch ? left : kSpecBatch;
    for (int u = 0; u < cnt; ++u) {
      const float px = bx[u * 64], py = by[u * 64];
      const int tau = a.tau0 + rb + u;
      if (shared) {
        for (int r = 0; r < count; ++r)
          mg[r * 64] = spec_margin(px, py, sreg[4 * r], sreg[4 * r + 1], sreg[4 * r + 2], sreg[4 * r + 3], skind[r]);
      } else {
        for (int r = 0; r < count; ++r)
          mg[r * 64] = spec_margin(px, py, greg[4 * r], greg[4 * r + 1], greg[4 * r + 2], greg[4 * r + 3], gkind[r]);
      }
#pragma unroll
      for (int c = 0; c < kSpecClausesMax; ++c) {
        if (c < a.C) {
          const int* q = cl + c * kSpecClauseWords;
          const int op = q[0];
          const bool window = q[1] <= tau && tau <= q[2];
          const float v1 = spec_predicate(mg, q[3], q[4], q[5], count);
          if (op == kSpecUntil) {
            if (v1 < guard[c]) guard[c] = v1;
            if (window) {
              const float v2 = spec_predicate(mg, q[6], q[7], q[8], count);
              const float w = v2 < guard[c] ? v2 : guard[c];
              if (w > rho[c]) { rho[c] = w; wit[c] = tau; }
            }
          } else if (window) {
            if (op == kSpecAlways ? v1 < rho[c] : v1 > rho[c]) { rho[c] = v1; wit[c] = tau; }
          }
        }
      }
    }
  }

  if (live) {
#pragma unroll
    for (int c = 0; c < kSpecClausesMax; ++c) {
      if (c < a.C) {
        a.val[((size_t)n * a.C + c) * 2] = rho[c];
        a.val[((size_t)n * a.C + c) * 2 + 1] = guard[c];
        a.wit[(size_t)n * a.C + c] = wit[c];
      }
    }
  }
}

}  // namespace mobrob
