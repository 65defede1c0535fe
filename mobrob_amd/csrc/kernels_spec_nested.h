// Nested run specifications (mobrob_ppo_spec_monitor_nested): stay-for and recurring visits, folded from the positions of a run.
//
// The rule, stated once in mobrob_amd/envs/goal_rules.py (spec_fold, spec_key).  Beside the flat clauses of kernels_spec.h a
// specification may hold nested clauses (op, a, b, pred, h) over the sliding window of the last h + 1 predicate values:
//   STAY   tau >= h and a <= tau - h <= b: s = min of v(tau - h) .. v(tau);  s > rho: rho = s, witness = tau - h
//   RECUR  tau >= h and a <= tau - h <= b: s = max of v(tau - h) .. v(tau);  s < rho: rho = s, witness = tau - h
// The inner extremum is taken under the total order on float32 bits, key = i ^ ((i >> 31) & 0x7fffffff) on the int32 view (-0.0 <
// +0.0), so its bits do not depend on the order a window is visited in; the outer comparison is the flat clauses' float comparison.
// Between calls the last h values of every nested clause travel in `tail` [N][W], oldest first, W the sum of the holds.
//
// k_spec_monitor_nested keeps k_spec_monitor's shape -- a lane per robot, a wave per workgroup, kSpecBatch records in flight, the
// margins once per sample in the lane's LDS column -- and folds the flat clauses with the same statements.  Each nested clause owns a
// ring of h + 1 slots per lane in LDS, lane-minor (no bank conflict), holding the window's values as ORDER KEYS: the key above, with
// every bit flipped for RECUR, so that both extrema are a signed integer minimum.  The ring is loaded from `tail` at entry (its
// slot h, the one the first sample overwrites, holds a filler) and its last h values are stored back at exit.  The window's
// extremum is a running minimum; only when the key that leaves the ring equals it is the ring scanned again (per lane: the other
// lanes wait).  The nested clauses are walked by a loop that is NOT unrolled -- sixteen copies of the ring update overflow the
// register file --, so what it carries per clause lives in LDS as well: the running minimum in the lane's column of [16][64], the
// ring position, the same in every lane, in one word per clause.  It leaves each window's extremum in a second [16][64] block, from
// which the unrolled clause loop folds it into (rho, witness), held in registers like the flat clauses' (no register array is indexed
// dynamically).  The clause table, with each nested clause's hold, ring offset and tail offset, sits in LDS (uniform reads).  The LDS
// block is dynamic and sized by the specification's own slots: 30.1 KB + 256 B per slot, 158.1 KB at the cap of 512 slots.
#pragma once
#include "kernels_spec.h"

namespace mobrob {

constexpr int kSpecStay = 3, kSpecRecur = 4;
constexpr int kSpecHoldMax = 255;           // the longest inner window [t, t + h]
constexpr int kSpecWindowSlots = 512;       // the sum of (h + 1) over the nested clauses
constexpr int kSpecNestedClauseWords = 12;  // the flat clause's nine, then h, the ring's first slot, the tail's first column

struct SpecNestedArgs {
  SpecArgs f;     // clauses: [C][kSpecNestedClauseWords]
  float* tail;    // [N][W] in / out (null when W == 0)
  int W;
};

// LDS words of k_spec_monitor_nested: the flat kernel's blocks with a wider clause table, the nested clauses' carried words, then the
// rings [slots][64]
constexpr int kSpecNestedLdsClauses = kSpecLdsY + kSpecBatch * 64;
constexpr int kSpecNestedLdsRegions = kSpecNestedLdsClauses + kSpecClausesMax * kSpecNestedClauseWords;
constexpr int kSpecNestedLdsKinds = kSpecNestedLdsRegions + kSpecRegionsMax * 4;
constexpr int kSpecNestedLdsExt = kSpecNestedLdsKinds + kSpecRegionsMax;          // running minimum key [16][64]
constexpr int kSpecNestedLdsWin = kSpecNestedLdsExt + kSpecClausesMax * 64;       // this sample's window extremum [16][64]
constexpr int kSpecNestedLdsPos = kSpecNestedLdsWin + kSpecClausesMax * 64;       // ring position [16]
constexpr int kSpecNestedLdsRings = kSpecNestedLdsPos + kSpecClausesMax;
constexpr size_t spec_nested_lds_bytes(int slots) { return ((size_t)kSpecNestedLdsRings + (size_t)slots * 64) * 4; }

// float bits <-> order key (the map is its own inverse)
__device__ __forceinline__ int spec_key(int i) { return i ^ ((i >> 31) & 0x7fffffff); }

__global__ __launch_bounds__(64) void k_spec_monitor_nested(SpecNestedArgs na) {
  extern __shared__ float lds[];
  const SpecArgs& a = na.f;
  const int lane = threadIdx.x;
  const int n = blockIdx.x * 64 + lane;
  const bool live = n < a.N;
  const int i = live ? n : a.N - 1;   // a lane past the last robot folds the last robot's rows and stores nothing
  float* mg = lds + kSpecLdsMargins + lane;
  float* bx = lds + kSpecLdsX + lane;
  float* by = lds + kSpecLdsY + lane;
  int* cl = reinterpret_cast<int*>(lds + kSpecNestedLdsClauses);
  float* sreg = lds + kSpecNestedLdsRegions;
  int* skind = reinterpret_cast<int*>(lds + kSpecNestedLdsKinds);
  int* ext = reinterpret_cast<int*>(lds + kSpecNestedLdsExt) + lane;
  int* win = reinterpret_cast<int*>(lds + kSpecNestedLdsWin) + lane;
  int* pos = reinterpret_cast<int*>(lds + kSpecNestedLdsPos);
  int* ring = reinterpret_cast<int*>(lds + kSpecNestedLdsRings) + lane;
  for (int w = lane; w < a.C * kSpecNestedClauseWords; w += 64) cl[w] = a.clauses[w];
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
  // the rings: the tail's h values, oldest first, in the slots 0 .. h - 1; the next sample goes to slot h
  const int* tail_in = reinterpret_cast<const int*>(na.tail) + (size_t)i * na.W;
#pragma unroll 1
  for (int c = 0; c < a.C; ++c) {
    const int* q = cl + c * kSpecNestedClauseWords;
    if (q[0] < kSpecStay) continue;
    const int h = q[9], flip = q[0] == kSpecRecur ? -1 : 0;
    int* rg = ring + q[10] * 64;
    const int* tl = tail_in + q[11];
    int m = 0x7f800000;   // the filler of slot h: the key of +inf (STAY), of -inf flipped (RECUR); the first sample overwrites it
    rg[h * 64] = m;
    for (int j = 0; j < h; ++j) {
      const int k = spec_key(tl[j]) ^ flip;
      rg[j * 64] = k;
      m = k < m ? k : m;
    }
    ext[c * 64] = m;
    pos[c] = h;           // (every lane writes the same word)
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
      // the nested clauses' windows take this sample's value; win: the extremum of v(tau - h) .. v(tau), as float bits
#pragma unroll 1
      for (int c = 0; c < a.C; ++c) {
        const int* q = cl + c * kSpecNestedClauseWords;
        const int op = q[0];
        if (op < kSpecStay) continue;
        const int h = q[9], flip = op == kSpecRecur ? -1 : 0;
        const int k = spec_key(__float_as_int(spec_predicate(mg, q[3], q[4], q[5], count))) ^ flip;
        int m = k;
        if (h > 0) {
          int* rg = ring + q[10] * 64;
          const int p = pos[c];
          const int gone = rg[p * 64];
          rg[p * 64] = k;
          pos[c] = p == h ? 0 : p + 1;
          m = ext[c * 64];
          if (gone == m) {   // the minimum may have left: scan the ring, the new value included
            m = k;
#pragma unroll 4
            for (int j = 0; j <= h; ++j) {
              const int o = rg[j * 64];
              m = o < m ? o : m;
            }
          } else {
            m = k < m ? k : m;
          }
          ext[c * 64] = m;
        }
        win[c * 64] = spec_key(m ^ flip);
      }
#pragma unroll
      for (int c = 0; c < kSpecClausesMax; ++c) {
        if (c < a.C) {
          const int* q = cl + c * kSpecNestedClauseWords;
          const int op = q[0];
          if (op >= kSpecStay) {
            const int t0 = tau - q[9];   // the window's start; compared in this form: b may be open, b + h would overflow
            if (t0 >= 0 && q[1] <= t0 && t0 <= q[2]) {
              const float sv = __int_as_float(win[c * 64]);
              if (op == kSpecStay ? sv > rho[c] : sv < rho[c]) { rho[c] = sv; wit[c] = t0; }
            }
          } else {
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
    // a ring's h + 1 values start, oldest first, at its position; the tail is the last h of them
    int* tail_out = reinterpret_cast<int*>(na.tail) + (size_t)n * na.W;
#pragma unroll 1
    for (int c = 0; c < a.C; ++c) {
      const int* q = cl + c * kSpecNestedClauseWords;
      if (q[0] < kSpecStay) continue;
      const int h = q[9], flip = q[0] == kSpecRecur ? -1 : 0;
      const int* rg = ring + q[10] * 64;
      int* tl = tail_out + q[11];
      int p = pos[c];
      for (int j = 0; j < h; ++j) {
        p = p == h ? 0 : p + 1;
        tl[j] = spec_key(rg[p * 64] ^ flip);
      }
    }
  }
}

}  // namespace mobrob
