// k_goal256_tile<Task>: a whole evaluation / waypoint-following call of a fused 2x256 tanh actor in ONE launch.
//
// The tasks, the environment rules, the observation features, the action rule and the trace row are those of kernels_eval.h /
// kernels_follow.h, used unchanged; only the actor is new.  Served: the non-wide tasks (EvalTask, FollowTask, ResumeFollowTask,
// ScheduledFollowTask) and, behind a switch of their own, the wide tasks of task_tile256_wide: static and moving hazards over
// most of those four.  The kernel is written for every wide task (walls, solid walls, teams and their stacks too: the hooks below are all
// there), but the tiles of WallTask / TeamTask spill vector registers and are not instantiated (tile256_wide_left_out): they stay
// on the per-step path.  A wide task's hooks are written for one 64-lane wave and take plain LDS pointers: here that
// wave is wave 0, which owns the tile's 16 robots anyway, and its LDS region starts at LayEval256::END, laid out exactly as behind
// LayEval64::END ([16][2] post-step xy, at + 32 what Task::stage fills).
//
// One workgroup = FOUR waves (one per SIMD: __launch_bounds__(256) gives every lane the whole 512-entry register file) = one tile
// of 16 robots.  Wave w owns the output columns 64 w .. 64 w + 63 of both hidden layers.
//   W2 (256 KB) does not fit the CU's LDS: wave w keeps its 64-column slice in REGISTERS for the whole launch, in the B-fragment
//      order of v_mfma_f32_16x16x4_f32 (lane l, column block cb, k-step ks holds W2[64 w + 16 cb + (l & 15)][4 ks + (l >> 4)]):
//      4 x 64 = 256 registers per lane, read from the flat parameter vector once.
//   W1 (fragment order, zero beyond D), W3 (fragment order, zero beyond A), the biases, the observation tile X, H1, H2, the head's
//      per-wave partial sums, the mean rows and the robots' state rows live in LDS: LayEval256::END floats (~147 KB).
// The observation tile is always 64 wide (features beyond Dp stay zero, W1's fragment is zero beyond D: the same sums), so there
// is one kernel per task; layer 1 runs only the Dp / 4 k-steps that can be non-zero.
//
// Per step: observation tile on all 256 lanes (one 4-feature chunk each) | layer 1 (4 column blocks x Dp / 4 k-steps per wave) |
// layer 2 (4 x 64, B from registers) | head: wave w multiplies its K-slice 64 w .. 64 w + 63 of H2 into a partial [16][32] in LDS
// (wave 0's accumulator starts at b3) | env phase on lanes 0 .. 15 of wave 0: the mean is ((p0 + p1) + p2) + p3, a FIXED order, then
// eval_actions and Task::step exactly as in k_goal64_tile; GoalState and the task's accumulators stay in those lanes' registers.
// A wide task: Task::step_lane on those 16 lanes, then Task::after_step on all 64 lanes of wave 0, as in k_goal64_tile.
//
// Barriers.  Every __syncthreads() below is reached by all four waves the same number of times:
//   * the five barriers of a step sit in straight-line code of the loop body, outside every lane- or wave-dependent branch;
//   * the loop's trip count is the same in every wave: max_steps is a kernel argument, and the early exit reads `go`, a word that
//     lane 0 ALONE writes (the ballot of wave 0's active robots, the only robots of the tile) before the step's closing barrier
//     and that every wave reads right after that barrier.  The next write of the word comes at the end of the NEXT env phase,
//     behind four more barriers that no wave passes before all have read it.  So every wave sees the same value in the same
//     iteration and leaves the loop together; none waits at a barrier for a wave that has left.
//   A private test (wave 0's own ballot, as the one-wave kernel uses) would let wave 0 leave while waves 1 .. 3 wait at the next
//   barrier, or the reverse: hence the published word.
// What each barrier orders: (1) X written -> layer 1 reads it; (2) H1 written -> layer 2 reads all 256 columns; (3) H2 written ->
// head reads; (4) partials written -> env lanes sum them; (5) state rows, `go` written, X / partial reads of the env phase done ->
// next step's observation phase.  H1 (H2) of step t + 1 is written behind barrier (1) ((2)) of t + 1, after its readers of step t.
//
// The wide tasks' region (from LayEval256::END: post-step block, the base's scene, pre-step block, wall scene; the teams' xy block is
// the post-step block) is PRIVATE TO WAVE 0: no other wave reads or writes a word of it.  So it needs no workgroup barrier, and none
// is added: the step still has five.  Wave-scoped ordering is used instead.  A wave's LDS instructions execute in the order they
// were issued, so a read sees every earlier write of the same wave; what is left is to keep the compiler from moving them, which
// eval256_wave_sync() does (release fence, wave barrier, acquire fence, all at wavefront scope: no instruction but the ordering).
//   * scene (Task::stage, wave 0) and the xy rows of Task::place: written before the opening barrier, read in the loop behind it.
//   * frame (Task::stage_frame, wave 0, top of a step whose frame differs): after wave 0's own reads of the old frame in the
//     previous step's after_step (program order; barrier (5) lies between), before this step's after_step (barriers (1) - (4) lie
//     between).  The frame index depends on g0 + t alone: the test is uniform, and only wave 0 acts on it.
//   * post-step and pre-step blocks: written by step_lane on lanes 0 .. 15, read by after_step on lanes 0 .. 63 of the same wave
//     behind eval256_wave_sync(); the next step's writes come after these reads in program order (and behind barrier (5)).
//   * teams: a row of the xy block of a robot that does not step keeps what `place` or its last step wrote, as in k_goal64_tile.
// No __syncthreads() sits inside `if (wave == 0)`.  `go` is written after after_step, from wave 0's ballot, before barrier (5).
#pragma once
#include "kernels_eval.h"

namespace mobrob {

struct LayEval256 {
  static constexpr int H = 256, DP = 64, LDX = DP + 4, LDH = H + 4, LDM = 36;
  static constexpr int W1 = 0;                        // [4 waves][4 col blocks][16 k-steps][64 lanes]
  static constexpr int W3 = W1 + 4 * 4 * 16 * 64;     // [2 col blocks][64 k-steps][64 lanes]
  static constexpr int B1 = W3 + 2 * 64 * 64;         // [256]
  static constexpr int B2 = B1 + H;                   // [256]
  static constexpr int B3 = B2 + H;                   // [32]
  static constexpr int X = B3 + 32;                   // [16][LDX]
  static constexpr int H1 = X + 16 * LDX;             // [16][LDH]
  static constexpr int H2 = H1 + 16 * LDH;            // [16][LDH]
  static constexpr int PT = H2 + 16 * LDH;            // [4 waves][16][LDM] the head's partial sums
  static constexpr int MU = PT + 4 * 16 * LDM;        // [16][LDM]
  static constexpr int ST = MU + 16 * LDM;            // [16][12] robot state for the observation phase
  static constexpr int GO = ST + 16 * 12;             // [4] word 0: any robot of the tile active
  static constexpr int END = GO + 4;
};
inline size_t eval256_lds_bytes() { return LayEval256::END * sizeof(float); }

// the non-wide tasks k_goal256_tile is instantiated for (eval_run), under mobrob_ppo_set_eval_tile256 alone
template <class Task>
constexpr bool task_tile256 = std::is_same_v<Task, EvalTask> || std::is_same_v<Task, FollowTask> ||
                              std::is_same_v<Task, ResumeFollowTask> || std::is_same_v<Task, ScheduledFollowTask>;

// the wide tasks it is instantiated for, under mobrob_ppo_set_eval_tile256_wide as well: every wide task eval_run is instantiated
// with, less those named in tile256_wide_left_out (what was left on the per-step path, and why)
template <class Task>
struct tile256_wide_left_out : std::false_type {};
// Left out: every task under WallTask or TeamTask (kernels_wall.h, kernels_team.h).  Their tiles came out of the compiler with 4 .. 8
// spilled vector registers (the correctly rounded sqrtf of wall_sdf / team_partial on top of the resident W2 slice), which the
// build's audit refuses; they stay on the per-step path.  So do HazardTask<ResumeFollowTask> (4 spilled vector registers) and
// FrameHazardTask<ScheduledFollowTask> (a 20-byte private segment, as eval_tile_width's note in engine.hip describes for another
// tile).  Served: HazardTask<> and FrameHazardTask<> over EvalTask and FollowTask, FrameHazardTask<ResumeFollowTask>,
// HazardTask<ScheduledFollowTask>.
template <class Base>
struct WallTask;
template <class Base>
struct TeamTask;
template <class B>
struct tile256_wide_left_out<WallTask<B>> : std::true_type {};
template <class B>
struct tile256_wide_left_out<TeamTask<B>> : std::true_type {};
template <class Base>
struct HazardTask;
template <class Base>
struct FrameHazardTask;
struct ResumeFollowTask;
struct ScheduledFollowTask;
template <>
struct tile256_wide_left_out<HazardTask<ResumeFollowTask>> : std::true_type {};
template <>
struct tile256_wide_left_out<FrameHazardTask<ScheduledFollowTask>> : std::true_type {};
template <class Task>
constexpr bool task_tile256_wide = Task::kWide && !tile256_wide_left_out<Task>::value;

// orders the LDS accesses of ONE wave: writes before it are seen by reads after it, on every lane of the wave (see "Barriers")
__device__ __forceinline__ void eval256_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// W1, W3 -> LDS in fragment order (zero beyond D / A), the biases, a zeroed observation tile
__device__ __forceinline__ void eval256_load_lds(const Eval64Net& W, int D, int A, int tid) {
  using L = LayEval256;
  for (int i = tid; i < 4 * 4 * 16 * 64; i += 256) {
    const int l = i & 63, ks = (i >> 6) & 15, cb = i >> 10;   // cb: 16-column block 0 .. 15 (= 4 wave + block of the wave)
    const int k = 4 * ks + (l >> 4);
    lds[L::W1 + i] = k < D ? W.W1[(size_t)(16 * cb + (l & 15)) * D + k] : 0.f;
  }
  for (int i = tid; i < 2 * 64 * 64; i += 256) {
    const int l = i & 63, ks = (i >> 6) & 63, nb = i >> 12;
    const int col = 16 * nb + (l & 15);
    lds[L::W3 + i] = col < A ? W.W3[col * L::H + 4 * ks + (l >> 4)] : 0.f;
  }
  lds[L::B1 + tid] = W.b1[tid];
  lds[L::B2 + tid] = W.b2[tid];
  if (tid < 32) lds[L::B3 + tid] = tid < A ? W.b3[tid] : 0.f;
  for (int i = tid; i < 16 * L::LDX; i += 256) lds[L::X + i] = 0.f;
}

template <class Task>
__global__ __launch_bounds__(256) void k_goal256_tile(typename Task::Args args, Eval64Net W) {
  static_assert(task_tile256<Task> || task_tile256_wide<Task>, "k_goal256_tile: a task outside both traits");
  using L = LayEval256;
  const EvalArgs& a = Task::eval(args);
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: wave-uniform branches and addresses)
  const int r16 = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * 16;
  eval256_load_lds(W, a.D, a.A, tid);
  if constexpr (Task::kWide) {   // the task's region is wave 0's alone: after [16][2] post-step positions at L::END
    if (wave == 0) Task::stage(args, &lds[L::END + 32], lane);
  }
  // ---- the wave's slice of W2, resident for the launch ----
  float w2[4][64];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int ks = 0; ks < 64; ++ks) w2[cb][ks] = W.W2[(64 * wave + 16 * cb + r16) * L::H + 4 * ks + q];
  // ---- start state of the tile's robots (lanes 0 .. 15 of wave 0 own robot row0 + lane) ----
  const int n = row0 + r16;
  const bool mine = tid < 16 && n < a.N;
  GoalState g{};
  typename Task::Robot R{};
  bool active = false;
  if (mine) {
    Task::start(g, R, args, n);
    active = Task::active(args, R);
    eval64_state_lds(&lds[L::ST + 12 * r16], g);
    if constexpr (task_teams<Task>) Task::place(g, &lds[L::END + 2 * r16]);
  }
  if (wave == 0) {
    const uint64_t any = __ballot(active);
    if (tid == 0) lds[L::GO] = any ? 1.f : 0.f;
  }
  __syncthreads();
  bool go = __builtin_amdgcn_readfirstlane(lds[L::GO] != 0.f ? 1 : 0) != 0;
  const bool wide_head = a.A > 16;
  const int ks1 = a.Dp / 4, per = a.Dp / 4;
  const int g0 = task_step0<Task>(args);   // t: step of this launch (trace, path); g0 + t: step of the streams
  [[maybe_unused]] int staged = 0;         // kFrames: the frame of the shared scene resident in LDS (Task::stage: the first used)
  if constexpr (Task::kFrames) staged = Task::frame(args, g0);
  for (int t = 0; t < a.max_steps && go; ++t) {   // uniform across the four waves: see "Barriers" above
    if constexpr (Task::kFrames) {
      const int f = Task::frame(args, g0 + t);   // uniform over the workgroup; wave 0 alone touches the scene
      if (f != staged) {
        if (wave == 0) Task::stage_frame(args, &lds[L::END + 32], lane, f);
        staged = f;
      }
    }
    // ---- observation tile: thread (r = tid & 15, c = tid >> 4) builds chunk c of robot r ----
    {
      const int r = tid & 15, c = tid >> 4;
      if (row0 + r < a.N && c < per) {
        GoalState gs{};
        const float* s = &lds[L::ST + 12 * r];
#pragma unroll
        for (int j = 0; j < 3; ++j) { gs.pos[j] = s[j]; gs.vel[j] = s[3 + j]; gs.goal[j] = s[6 + j]; }
        *reinterpret_cast<f32x4*>(&lds[L::X + r * L::LDX + 4 * c]) = eval_features(gs, a, row0 + r, c, (uint32_t)(g0 + t));
      }
    }
    __syncthreads();   // (1)
    // ---- layer 1: h1 = tanh(W1 x + b1), the wave's four 16-column accumulators ----
    {
      f32x4 c[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) { const float b = lds[L::B1 + 64 * wave + 16 * cb + r16]; c[cb] = f32x4{b, b, b, b}; }
#pragma unroll 4
      for (int ks = 0; ks < ks1; ++ks) {
        const float x = lds[L::X + r16 * L::LDX + 4 * ks + q];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) c[cb] = MFMA16(x, lds[L::W1 + ((4 * wave + cb) * 16 + ks) * 64 + lane], c[cb]);
      }
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int i = 0; i < 4; ++i) lds[L::H1 + (4 * q + i) * L::LDH + 64 * wave + 16 * cb + r16] = fast_tanh(c[cb][i]);
    }
    __syncthreads();   // (2)
    // ---- layer 2: B operands from the resident registers ----
    {
      f32x4 c[4];
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) { const float b = lds[L::B2 + 64 * wave + 16 * cb + r16]; c[cb] = f32x4{b, b, b, b}; }
#pragma unroll
      for (int ks = 0; ks < 64; ++ks) {
        const float x = lds[L::H1 + r16 * L::LDH + 4 * ks + q];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) c[cb] = MFMA16(x, w2[cb][ks], c[cb]);
      }
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int i = 0; i < 4; ++i) lds[L::H2 + (4 * q + i) * L::LDH + 64 * wave + 16 * cb + r16] = fast_tanh(c[cb][i]);
    }
    __syncthreads();   // (3)
    // ---- head: the wave's K-slice (k-steps 16 wave .. 16 wave + 15) of W3 h2, one or two 16-column blocks ----
    {
      const float b0 = wave == 0 ? lds[L::B3 + r16] : 0.f, b1 = wave == 0 ? lds[L::B3 + 16 + r16] : 0.f;
      f32x4 c0 = f32x4{b0, b0, b0, b0}, c1 = f32x4{b1, b1, b1, b1};
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int ks = 16 * wave + k;
        const float x = lds[L::H2 + r16 * L::LDH + 4 * ks + q];
        c0 = MFMA16(x, lds[L::W3 + ks * 64 + lane], c0);
        if (wide_head) c1 = MFMA16(x, lds[L::W3 + (64 + ks) * 64 + lane], c1);
      }
      float* p = &lds[L::PT + wave * 16 * L::LDM];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        p[(4 * q + i) * L::LDM + r16] = c0[i];
        p[(4 * q + i) * L::LDM + 16 + r16] = c1[i];
      }
    }
    __syncthreads();   // (4)
    // ---- env phase: the tile's 16 lanes (wave 0) ----
    if (wave == 0) {
      if constexpr (Task::kWide) {
        // the 16 robot lanes, then the task's wide phase on all 64 lanes of this wave (robot lane & 15 stepped: bit of `stepping`)
        const uint64_t stepping = __ballot(mine && active);
        int e0 = 0;
        if (mine && active) {
          float* act = &lds[L::MU + r16 * L::LDM];
          const float* p = &lds[L::PT + r16 * L::LDM];
          for (int k = 0; k < a.A; ++k)
            act[k] = ((p[k] + p[16 * L::LDM + k]) + p[2 * 16 * L::LDM + k]) + p[3 * 16 * L::LDM + k];
          eval_actions(a, n, g0 + t, act, act);
          active = Task::step_lane(g, R, args, n, t, act, &lds[L::X + r16 * L::LDX], &lds[L::END + 2 * r16], e0);
          eval64_state_lds(&lds[L::ST + 12 * r16], g);
        }
        eval256_wave_sync();   // step_lane's xy rows -> after_step's reads on the wave's other lanes
        Task::after_step(args, R, n, t, lane, (stepping >> r16) & 1ull, e0, &lds[L::END], &lds[L::END + 32]);
      } else {
      if (mine && active) {
        float* act = &lds[L::MU + r16 * L::LDM];   // the mean row becomes the applied action in place
        const float* p = &lds[L::PT + r16 * L::LDM];
        for (int k = 0; k < a.A; ++k)
          act[k] = ((p[k] + p[16 * L::LDM + k]) + p[2 * 16 * L::LDM + k]) + p[3 * 16 * L::LDM + k];
        eval_actions(a, n, g0 + t, act, act);
        active = Task::step(g, R, args, n, t, act, &lds[L::X + r16 * L::LDX]);
        eval64_state_lds(&lds[L::ST + 12 * r16], g);
      }
      }
      const uint64_t any = __ballot(active);
      if (tid == 0) lds[L::GO] = any ? 1.f : 0.f;
    }
    __syncthreads();   // (5)
    go = __builtin_amdgcn_readfirstlane(lds[L::GO] != 0.f ? 1 : 0) != 0;
  }
  if (mine) Task::finish(args, n, R, g);
}

}  // namespace mobrob
