// libmobrob_ppo.so -- host-side orchestration + C ABI (include/mobrob_ppo.h) of the MI355X PPO engine.
// Reference surface replaced: stable_baselines3.PPO as configured by the reference's
// src/mobrob/rl_control/ppo.py:50-59 and driven by :73-77 (see the header for per-entry citations).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types and prototypes only: the library is dlopen'ed by comm_init (no link-time dependency)
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <climits>
#include <cstring>
#include <ctime>
#include <cstdlib>
#include <string>
#include <vector>

#ifdef MOBROB_POISON_LDS
// Diagnostic build (scratch/build_variant.sh poison -DMOBROB_POISON_LDS; never the product library): every kernel launch is
// preceded by one that fills the LDS of every CU with 0xFFFFFFFF (a NaN as float, -1 as an index).  LDS is not cleared
// between kernels, so a kernel that reads a word it did not write sees whatever the previous tenant of the CU left there:
// right on most runs, wrong once in a while.  Under this build it is wrong every time (scratch/README.md: GPU suite with
// MOBROB_PPO_LIB=scratch/lib_poison.so).
namespace mobrob {
__global__ __launch_bounds__(1024) void k_poison_lds() {
  extern __shared__ unsigned poison_words[];
  volatile unsigned* w = poison_words;
  for (int i = threadIdx.x; i < 160 * 256; i += 1024) w[i] = 0xFFFFFFFFu;
}
inline void poison_lds(hipStream_t st) {
  static bool once = false;
  if (!once) { (void)hipFuncSetAttribute((const void*)k_poison_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); once = true; }
  k_poison_lds<<<dim3(512), dim3(1024), 160 * 1024, st>>>();
}
}  // namespace mobrob
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, nb, nt, mem, st, ...)                    \
  do {                                                                          \
    mobrob::poison_lds(st);                                                     \
    hipLaunchKernelGGLInternal((kernelName), nb, nt, mem, st, __VA_ARGS__);     \
  } while (0)
#endif

#include "../../include/mobrob_ppo.h"
#include "kernels_generic.h"
#include "kernels_fused.h"
#include "fused_dispatch.h"
#include "kernels_env.h"
#include "kernels_eval.h"
#include "kernels_follow.h"
#include "kernels_eval256.h"
#include "kernels_hazard.h"
#include "kernels_team.h"
#include "kernels_wall.h"
#include "kernels_team_solid.h"
#include "kernels_plan.h"
#include "kernels_spec.h"
#include "kernels_spec_nested.h"
#include "kernels_spec_moving.h"
#include "kernels_plan_spec.h"
#include "kernels_plan_spec_resume.h"
#include "kernels_plan_spec_share.h"
#include "kernels_rollout.h"
#include "kernels_epoch64.h"
#include "robot_ctrl.h"
#include "oneshot_allreduce.h"

using namespace mobrob;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPC(expr)                                                                                            \
  do {                                                                                                        \
    hipError_t _e = (expr);                                                                                   \
    if (_e != hipSuccess)                                                                                     \
      return fail(MOBROB_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
#define CHK(expr)                   \
  do {                              \
    int _r = (expr);                \
    if (_r != MOBROB_OK) return _r; \
  } while (0)

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int rup(int a, int b) { return cdiv(a, b) * b; }

// an environment variable as a number, `dflt` when it is not set
inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }
inline double env_double(const char* name, double dflt) { const char* v = getenv(name); return v ? atof(v) : dflt; }
// MOBROB_NO_X3, MOBROB_NO_TRAIN_X3, MOBROB_NO_CHAIN, MOBROB_NO_NORM_RECORDS switch their feature off by being PRESENT: any value, "0" included
inline bool env_switched_off(const char* name) { return getenv(name) != nullptr; }

struct ProfSpan {
  hipEvent_t a, b;
  int id;
};

// Canonical tensors in SB3's registration order: log_std, (W, b) of every policy hidden layer, (W, b) of every value hidden layer,
// action head, value head.  With one to eight hidden layers per network that is 9 .. 37 tensors; the ids are the engine's
// (engine_dims), the names below resolve through `e`.  Two hidden layers per network give the numbering 0 .. 12 the fused
// kernels' argument structs were written for.
// (kMaxHidden = 8: device_utils.h; kMaxTensors = 37: kernels_fused.h)
#define T_LOGSTD 0
#define T_PW1 (e->tPW[0])
#define T_PB1 (e->tPB[0])
#define T_PW2 (e->tPW[1])
#define T_PB2 (e->tPB[1])
#define T_VW1 (e->tVW[0])
#define T_VB1 (e->tVB[0])
#define T_VW2 (e->tVW[1])
#define T_VB2 (e->tVB[1])
#define T_AW (e->tAW)
#define T_AB (e->tAB)
#define T_VW (e->tVWh)
#define T_VB (e->tVBh)

}  // namespace

struct mobrob_ppo_engine {
  mobrob_ppo_config_t cfg;
  int D, Dp, A, Ap, H1, H2, G1, G2, N, T, P;   // H1, H2 / G1, G2: the first two hidden widths (the fused kernels' view; H2 = 0 at depth 1)
  int Lp = 2, Lv = 2;                          // hidden layers of the policy / value network (1 .. kMaxHidden)
  int Hp[kMaxHidden] = {0}, Hv[kMaxHidden] = {0};   // their widths
  int HL = 0, GL = 0;                          // width of the last hidden layer of each network (what the heads read)
  int tPW[kMaxHidden] = {0}, tPB[kMaxHidden] = {0}, tVW[kMaxHidden] = {0}, tVB[kMaxHidden] = {0}, tAW = 0, tAB = 0, tVWh = 0, tVBh = 0;
  int ntens = 13;
  int Bl;        // local minibatch rows (batch_size / world)
  int nmb;       // minibatches per epoch
  int rows_max;  // max rows any forward sees at once
  int offs[kMaxTensors + 1];  // canonical parameter offsets (SB3 order); offs[ntens] = P
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // parameters / optimizer
  float *params = nullptr, *grads = nullptr /* [P] + 8 loss sums */, *m = nullptr, *v = nullptr;
  NormChunk* chunks_dev = nullptr;
  double* chunk_partial = nullptr;
  int nchunks = 0;
  float *pW1p = nullptr, *vW1p = nullptr, *aWp = nullptr, *vWp = nullptr;  // zero-padded compute copies
  int64_t adam_step = 0;
  // rollout storage
  float *obs = nullptr, *actions = nullptr, *rewards = nullptr, *es = nullptr, *values = nullptr, *logp = nullptr,
        *adv = nullptr, *ret = nullptr;
  float *last_values = nullptr, *last_dones = nullptr, *prev_dones = nullptr, *dones_tmp = nullptr;
  float *clip_act = nullptr, *rew_tmp = nullptr, *term_obs = nullptr, *term_val = nullptr, *eps_dev = nullptr;
  uint8_t *trunc_dev = nullptr, *dones_u8 = nullptr;
  int *ep_len = nullptr, *ep_len2 = nullptr;
  uint32_t* ctr_dev = nullptr;  // [0] eps draw base, [1] env step base (device-resident: graph replays and the persistent rollout kernels advance them)
  hipGraph_t ro_graph = nullptr;
  hipGraphExec_t ro_exec = nullptr;
  struct RolloutSpec {  // what the captured rollout graph was built for
    int kind = 0;       // 0 none, 1 synthetic source, 2 goal environment
    float p_term = 0.f;
    int time_limit = 0;
    GoalEnvParams goal{};
  } ro_spec;
  int env_started = 0;  // env kind whose state is live on the device (0 = none)
  hipStream_t vstream = nullptr;          // batched value pass of finished rollout chunks, concurrent with the rollout
  std::vector<hipEvent_t> ev_chunks;      // one event per rollout chunk (an event is recorded once per capture)
  hipEvent_t ev_vdone = nullptr;
  float* gstate[2] = {nullptr, nullptr};  // goal env state, double buffered [N][kGoalStateFloats]
  double* ep_stats = nullptr;             // [4] episode statistics of the goal env + the Monitor ring (kernels_env.h)
  uint64_t ep_ring_read = 0;              // records already handed out by mobrob_ppo_episode_records
  uint32_t draw_counter = 0;  // Philox draw index for eps
  // pipelined host-env rollout (act_part / wait_part / store_part): per-part step indices and completion events
  int nparts = 0;
  int part_act_t[MOBROB_MAX_PARTS] = {0}, part_store_t[MOBROB_MAX_PARTS] = {0};
  int part_obs_t[MOBROB_MAX_PARTS] = {0};  // rollout slot whose observations store_part already pulled (-1: none)
  hipEvent_t ev_part[MOBROB_MAX_PARTS] = {nullptr};
  const void* pinned_seen[8] = {nullptr};  // pointers validated by is_pinned_cached since rollout_begin
  unsigned pinned_seen_n = 0;
  uint32_t draw_ro0 = 0;  // draw_counter at rollout_begin: part p at its step t draws with draw_ro0 + t
  // host-env rollout SERVED by the persistent rollout kernel (collect_host_served): flags in pinned memory, abort word on the device
  unsigned* srv_flags = nullptr;   // [srv_blocks] workgroup flags | [MOBROB_MAX_PARTS][16] host words | [16] error word
  int srv_blocks = 0;
  int* srv_abort = nullptr;
  uint32_t env_step_counter = 0;
  int t = 0;
  bool rollout_ready = false;
  // training records of the H = 256 gradient kernel (kernels_fused.h, k_build_train_records): rebuilt before the next
  // gradient launch whenever one of the five arrays they are packed from may have changed
  bool train_rec_valid = false;
  bool train_rec_external = false;  // a device pointer to one of those arrays was handed out (buffer_info): never trusted again
  // update
  int* rows = nullptr;          // [T*N] device row index per permuted position
  int64_t* perm_dev = nullptr;  // [T*N]
  double* advstat = nullptr;    // [nmb][4]
  double* expvar_part = nullptr;  // [kEvBlocks][4] partial sums of mobrob_ppo_explained_variance
  unsigned long long* advbins = nullptr;  // [nmb][2] fixed-point sums of k_adv_stats_stream (+ 1 word: max |adv| bits)
  uint64_t perm_counter = 0;
  unsigned adv_pass = 0;        // epoch_begin calls so far: which of the two max-|adv| words is live
  bool epoch_open = false;
  float* stats = nullptr;  // [stats_cap][8]
  int stats_cap = 0, stats_n = 0;
  int cur_count = 0;
  bool grad_pending = false;
  double clip_vf = -1.0;      // SB3 clip_range_vf (< 0: None); mobrob_ppo_set_hyper
  double target_kl = -1.0;    // SB3 target_kl (< 0: None): early stop of PPO.train() when a minibatch's approx_kl > 1.5 target
  int last_epochs_started = 0, last_stopped_early = 0, last_steps_applied = 0;  // of the latest mobrob_ppo_train*
  ncclComm_t comm = nullptr;  // RCCL communicator of the data-parallel job (mobrob_ppo_comm_init)
  int64_t allreduce_calls = 0, allreduce_bytes = 0;  // since the last mobrob_ppo_allreduce_counters(reset)
  struct OneShot {  // peer-mapped exchange buffers of the one-shot all-reduce (oneshot_allreduce.h)
    char* xbuf = nullptr;                 // own: [2 slots][payload] + [kOneShotMaxChunks] u64 flags (a hipMalloc of its own: IPC exports whole allocations)
    size_t payload = 0;
    char* peer[kOneShotMaxRanks] = {nullptr};  // every rank's buffer as mapped here (peer[rank] == xbuf)
    int world = 0, rank = -1;
    bool ready = false;
    unsigned long long seq = 0;           // messages exchanged so far: the same number on every rank
    int* error = nullptr;                 // pinned host word the kernel raises when a peer never arrived
    long long timeout_ticks = 0;
  } oneshot;
  // norm records of the reduction kernels (kernels_fused.h: block_norm_records): used inside mobrob_ppo_train only
  double* norm_rec_sum = nullptr; int* norm_rec_t = nullptr; int* fold_idx_dev = nullptr;
  int fold_start[kMaxTensors + 1] = {0};
  bool use_norm_records = false;
  // one co-operative launch per epoch for small minibatches of 64-wide nets (kernels_epoch64.h)
  bool epoch_kernel_on = true;        // MOBROB_EPOCH_KERNEL=0 / mobrob_ppo_set_hyper(MOBROB_HYPER_EPOCH_KERNEL, 0): the three launches per step
  unsigned* epoch_bar = nullptr;      // [0] arrival counter, [1] abort word
  float* epoch_consts = nullptr;      // [nmb][2] per-step Adam constants of the epoch being launched
  int* epoch_idx = nullptr;           // [nmb] statistics rows of the epoch being launched
  char* epoch_stage = nullptr;        // pinned staging of the two (12 bytes per step), one slot per epoch of a train() call
  int* epoch_err_host = nullptr;      // pinned: raised by a launch that gave up at a barrier
  hipEvent_t epoch_ev = nullptr;      // behind the last staging copy of a train() call: the staging may be rewritten after it
  int last_update_mode = 0;           // bit 0: the latest train() ran its epochs as k_epoch64 launches
  float* epoch_snap = nullptr;        // [3][P] parameters and both moments as they were before a mobrob_ppo_train that uses k_epoch64 (restored if it aborts)
  int rollout64_tile_max = 256;  // rollouts of up to this many 32-env tiles use k_rollout64_tile (MOBROB_ROLLOUT64_TILE_MAX)
  int pair64_min_tiles = 65;     // minibatches of at least this many tiles use k_pair64_train (MOBROB_PAIR64_MIN_TILES; 0: never)
  int split64_max_tiles = 64;  // minibatches of up to this many 32-row tiles use k_split64_train (MOBROB_SPLIT64_MAX_TILES)
  // generic-path workspace
  float *Xg = nullptr, *actg = nullptr, *lpg = nullptr, *advg = nullptr, *retg = nullptr, *oldvg = nullptr;
  float *hp[kMaxHidden] = {nullptr}, *hv[kMaxHidden] = {nullptr}, *mu = nullptr, *vout = nullptr;     // activations per hidden layer
  float *dmu = nullptr, *dv = nullptr, *dzp[kMaxHidden] = {nullptr}, *dzv[kMaxHidden] = {nullptr};     // pre-activation gradients
  float *pred_obs = nullptr, *pred_act = nullptr;
  // gSDE (use_sde; generic chain only): per-env exploration matrices [N][HL][A], the single matrix [HL][A], staging for supplied noise,
  // the log_std-gradient GEMM's operands of a minibatch
  int gemm_tiles = 0;   // MOBROB_GEMM_TILES: 0 = by shape (launch_gemm)
  bool sde = false, sde_hold = false;   // hold: the caller supplies the noise (mobrob_ppo_sde_set_noise); no automatic resampling
  float *sde_E = nullptr, *sde_E1 = nullptr, *sde_lat2 = nullptr, *sde_gsig = nullptr, *sde_graw = nullptr;
  float *sde_S2 = nullptr, *sde_var = nullptr;   // std^2 table [HL][A] of the current log_std; variance [rows][Ap] of the rows in flight
  SdeMode sde_mode{1, 0};   // policy_kwargs full_std / use_expln
  // rollout streamer (host-env path): pinned staging + a side stream for the H2D/D2H copies
  hipStream_t cstream = nullptr;
  hipEvent_t ev_in = nullptr, ev_k = nullptr, ev_store = nullptr;
  struct Stage {
    float *obs = nullptr, *eps = nullptr, *rew = nullptr, *term = nullptr;
    uint8_t *dones = nullptr, *trunc = nullptr;
  } stage[2];
  float *o_raw = nullptr, *o_clip = nullptr, *o_val = nullptr, *o_lp = nullptr;  // pinned output staging
  int stage_i = 0;
  // profiling
  bool prof_on = false;
  uint32_t prof_mask = ~0u;  // which MOBROB_K_* phases are bracketed while prof_on
  std::vector<ProfSpan> spans;
  std::vector<hipEvent_t> ev_pool;
  double prof_ms[MOBROB_K_COUNT] = {0};
  int64_t prof_calls[MOBROB_K_COUNT] = {0};
  std::vector<void*> allocs;
  // device arena: every device buffer of the engine is carved out of ONE allocation (owned, or handed in by the
  // caller so that several engines -- the robot types of a mixed fleet -- pack into one rollout buffer)
  char* arena = nullptr;
  size_t arena_bytes = 0, arena_used = 0;
  bool plan_only = false;  // sizing pass: count bytes, touch no device
  std::vector<NormChunk> chunk_table;
  FusedState fused;
  // policy evaluation (mobrob_ppo_evaluate_goal_env): one hipMalloc of its own, outside the arena, grown on demand
  char* eval_buf = nullptr;
  size_t eval_bytes = 0;
  int eval_tile256 = -1;   // mobrob_ppo_set_eval_tile256: 1 on, 0 off, -1 not told (MOBROB_EVAL_TILE256 decides, read per call)
  int eval_tile256_wide = -1;   // mobrob_ppo_set_eval_tile256_wide: likewise (MOBROB_EVAL_TILE256_WIDE); the wide tasks need both
  // grid planner (mobrob_ppo_plan_grid): two allocations of its own, outside the arena, grown on demand.  plan_fields holds what
  // a replanning round reuses (occupancy, fields, their scenes, goal cells and sweep counts), plan_buf a call's inputs and outputs
  char* plan_fields = nullptr;
  char* plan_buf = nullptr;
  size_t plan_fields_bytes = 0, plan_bytes = 0;
  int64_t plan_id = 0;                // id of the resident fields, 0: none
  int plan_G = 0, plan_S = 0, plan_F = 0;
  std::vector<int32_t> plan_field_scene, plan_field_goal;   // the resident fields' (scene, goal cell)
  bool plan_lds_set = false;          // k_plan_field's dynamic-LDS attribute is raised once
  // line-of-sight smoothing (mobrob_ppo_plan_smooth): the cells that are not clear at margin 1 of the resident occupancy, computed
  // by the first margin-1 call on the fields of id plan_dil_id
  char* plan_dil = nullptr;
  size_t plan_dil_bytes = 0;
  int64_t plan_dil_id = 0;
  // clearance-aware plans (mobrob_ppo_plan_grid_clear): resident fields of their own -- occupancy, surcharges, the margin-1 map,
  // cost fields -- beside the plain ones, so neither family evicts the other.  Their ids carry kPlanClearIdBit: an id of one family
  // never equals a resident id of the other, which is how a reuse_id of the wrong family is refused
  char* plan_clear_fields = nullptr;
  size_t plan_clear_fields_bytes = 0;
  int64_t plan_clear_id = 0, plan_clear_dil_id = 0;
  int plan_clear_G = 0, plan_clear_S = 0, plan_clear_F = 0, plan_clear_reach = 0, plan_clear_weight = 0;
  std::vector<int32_t> plan_clear_field_scene, plan_clear_field_goal;
  bool plan_clear_lds_set = false;    // k_plan_field_cost's dynamic-LDS attribute is raised once
  // time plans (mobrob_ppo_plan_grid_time): one allocation of their own and nothing resident, so the static fields above stay
  // valid across time-plan calls
  char* plan_time_buf = nullptr;
  size_t plan_time_bytes = 0;
  bool plan_time_lds_set = false;     // k_plan_field_time's dynamic-LDS attribute is raised once
  // team plans (mobrob_ppo_plan_grid_team): likewise one allocation of their own and nothing resident
  char* plan_team_buf = nullptr;
  size_t plan_team_bytes = 0;
  bool plan_team_lds_set = false;     // k_plan_team's dynamic-LDS attribute is raised once
  bool plan_team_smooth_lds_set = false;   // and k_plan_team_smooth's
  bool plan_team_rounds_lds_set = false;   // and k_plan_team_rounds's
  bool plan_assign_lds_set = false;        // and k_plan_assign_cost's (mobrob_ppo_plan_assign works in plan_team_buf)
  // run specifications (mobrob_ppo_spec_monitor): the uploaded path, the carried state and the tables, one allocation of their own
  char* spec_buf = nullptr;
  size_t spec_bytes = 0;
  bool spec_nested_lds_set = false;   // k_spec_monitor_nested's dynamic-LDS attribute is raised once
  bool spec_moving_lds_set = false;   // k_spec_monitor_moving's likewise
  // plans from a specification (mobrob_ppo_spec_plan): one allocation of their own and nothing resident
  char* plan_spec_buf = nullptr;
  size_t plan_spec_bytes = 0;
};

namespace {

int check_async_error(mobrob_ppo_engine* e);  // defined with the one-shot all-reduce

constexpr size_t kArenaAlign = 256;

template <typename Tp>
int dalloc(mobrob_ppo_engine* e, Tp** p, size_t count) {
  const size_t bytes = (std::max<size_t>(count, 1) * sizeof(Tp) + kArenaAlign - 1) / kArenaAlign * kArenaAlign;
  if (e->plan_only) {
    e->arena_used += bytes;
    *p = nullptr;
    return MOBROB_OK;
  }
  if (e->arena_used + bytes > e->arena_bytes)
    return fail(MOBROB_ERR_INVALID, "device arena too small: need more than %zu bytes", e->arena_bytes);
  void* q = e->arena + e->arena_used;
  e->arena_used += bytes;
  HIPC(hipMemsetAsync(q, 0, bytes, e->stream));
  *p = static_cast<Tp*>(q);
  return MOBROB_OK;
}

hipEvent_t get_event(mobrob_ppo_engine* e) {
  if (!e->ev_pool.empty()) {
    hipEvent_t ev = e->ev_pool.back();
    e->ev_pool.pop_back();
    return ev;
  }
  hipEvent_t ev;
  (void)hipEventCreate(&ev);
  return ev;
}

struct ProfScope {
  mobrob_ppo_engine* e;
  ProfSpan s;
  bool on;
  ProfScope(mobrob_ppo_engine* e_, int id) : e(e_), on(e_->prof_on && ((e_->prof_mask >> id) & 1u)) {
    if (on) {
      s.id = id;
      s.a = get_event(e);
      s.b = get_event(e);
      (void)hipEventRecord(s.a, e->stream);
    }
  }
  ~ProfScope() {
    if (on) {
      (void)hipEventRecord(s.b, e->stream);
      e->spans.push_back(s);
    }
  }
};

void prof_resolve(mobrob_ppo_engine* e) {
  for (auto& s : e->spans) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) {
      e->prof_ms[s.id] += ms;
      e->prof_calls[s.id] += 1;
    }
    e->ev_pool.push_back(s.a);
    e->ev_pool.push_back(s.b);
  }
  e->spans.clear();
}

// ---- GEMM launchers --------------------------------------------------------------------------------
// One GEMM of the generic chain as the launcher takes it: mode / epilogue (template parameters of k_gemm), arguments, batch split
struct GemmOp {
  int mode = 0, epi = 0, ksplit = 1;
  GemmArgs g{};
};
using GemmQueue = std::vector<GemmOp>;

template <int MODE, int EPI, int TM, int TN>
void launch_gemm_tiles(mobrob_ppo_engine* e, const GemmOp& a, const GemmOp* b) {
  // Orientation of a block's four waves, per problem.  Forward / input-gradient GEMMs stream a tall A ([rows][K]) against a small B
  // (weights): with the waves side by side along N the block fetches its A rows ONCE (L1 / one XCD's L2) where four column blocks
  // scattered over the chip fetched them four times -- at 65 536 x 256 x 256 that was 268 MB through L2 per launch against 67.
  // Only where the column tiles fill the four waves; the weight-gradient GEMM (both operands tall) keeps them stacked along M.
  static const bool wn_on = env_int("MOBROB_GEMM_WN", 1) != 0;
  GemmArgs ga = a.g, gb = b ? b->g : a.g;
  int gx = 1, gy = 1;
  for (GemmArgs* g : {&ga, &gb}) {
    const int mt = cdiv(g->M, 32 * TM), nt = cdiv(g->N, 32 * TN);
    g->wn = (wn_on && MODE != MODE_TN && nt % 4 == 0) ? 1 : 0;
    gx = std::max(gx, g->wn ? mt : cdiv(mt, 4));
    gy = std::max(gy, g->wn ? nt / 4 : nt);
  }
  const int ks = b ? std::max(a.ksplit, b->ksplit) : a.ksplit;
  hipLaunchKernelGGL((k_gemm<MODE, EPI, TM, TN>), dim3(gx, gy, b ? 2 * ks : ks), dim3(256), 0, e->stream, ga, gb, b ? 1 : 0);
}
// tiles per wave by shape: 2x2 wherever both extents leave room for it, 2x1 for narrow outputs (heads), 1x1 for tiny ones.
// MOBROB_GEMM_TILES (read when the engine is created): 1 keeps one tile per wave (A/B); 21 / 22 force 2x1 / 2x2 wherever the output
// has more than one tile in that direction, whatever the wave count (the parity tests drive small shapes through every form).
// b: a second problem of the same mode / epilogue for the same launch (the other network's GEMM at this point of the chain).
template <int MODE, int EPI>
void launch_gemm(mobrob_ppo_engine* e, const GemmOp& a, const GemmOp* b = nullptr) {
  const int f = e->gemm_tiles;
  const int M = b ? std::max(a.g.M, b->g.M) : a.g.M, N = b ? std::max(a.g.N, b->g.N) : a.g.N;
  if (f == 22 && M > 32 && N > 32) return launch_gemm_tiles<MODE, EPI, 2, 2>(e, a, b);
  if ((f == 21 || f == 22) && M > 32) return launch_gemm_tiles<MODE, EPI, 2, 1>(e, a, b);
  // fat wave tiles only while they still leave ~8 waves per CU: a rollout step (4096 rows) is 1024 one-tile waves, 256 as 2x2
  auto waves = [&](int tm, int tn) {
    long w = (long)cdiv(a.g.M, 32 * tm) * cdiv(a.g.N, 32 * tn) * a.ksplit;
    if (b) w += (long)cdiv(b->g.M, 32 * tm) * cdiv(b->g.N, 32 * tn) * b->ksplit;
    return w;
  };
  if (f != 0 || M <= 32 || waves(2, 1) < 2048) launch_gemm_tiles<MODE, EPI, 1, 1>(e, a, b);
  else if (N <= 32 || waves(2, 2) < 2048) launch_gemm_tiles<MODE, EPI, 2, 1>(e, a, b);
  else launch_gemm_tiles<MODE, EPI, 2, 2>(e, a, b);
}
void launch_op(mobrob_ppo_engine* e, const GemmOp& a, const GemmOp* b = nullptr) {
  if (a.mode == MODE_NT && a.epi == EPI_BIAS_TANH) launch_gemm<MODE_NT, EPI_BIAS_TANH>(e, a, b);
  else if (a.mode == MODE_NT) launch_gemm<MODE_NT, EPI_BIAS>(e, a, b);
  else if (a.mode == MODE_NN) launch_gemm<MODE_NN, EPI_DTANH_COLSUM>(e, a, b);
  else launch_gemm<MODE_TN, EPI_ATOMIC>(e, a, b);
}
// tile class launch_gemm would pick for one op on its own: 11, 21 or 22
int gemm_tile_class(const mobrob_ppo_engine* e, const GemmOp& a) {
  const int f = e->gemm_tiles, M = a.g.M, N = a.g.N;
  if (f == 22 && M > 32 && N > 32) return 22;
  if ((f == 21 || f == 22) && M > 32) return 21;
  const long w21 = (long)cdiv(M, 64) * cdiv(N, 32) * a.ksplit, w22 = (long)cdiv(M, 64) * cdiv(N, 64) * a.ksplit;
  if (f != 0 || M <= 32 || w21 < 2048) return 11;
  return (N <= 32 || w22 < 2048) ? 21 : 22;
}
// up to four one-tile problems of any kind in ONE launch (k_gemm_multi)
void launch_multi(mobrob_ppo_engine* e, const GemmOp* const* ops, int n) {
  GemmMulti m{};
  int gx = 1, gy = 1, z = 0;
  for (int p = 0; p < 4; ++p) {
    const GemmOp& o = *ops[p < n ? p : n - 1];   // (unused slots repeat the last problem; their z range is empty)
    m.g[p] = o.g; m.mode[p] = o.mode; m.epi[p] = o.epi;
    m.zbeg[p] = z;
    if (p < n) {
      z += o.ksplit;
      gx = std::max(gx, cdiv(cdiv(o.g.M, 32), 4)); gy = std::max(gy, cdiv(o.g.N, 32));
    }
  }
  m.zbeg[4] = z;
  hipLaunchKernelGGL(k_gemm_multi, dim3(gx, gy, z), dim3(256), 0, e->stream, m);
}
// The two networks' chains side by side, in STAGES of `width` consecutive GEMMs per network that depend on earlier stages only
// (forward: 1 -- a layer; backward: 2 -- a layer's weight-gradient and input-gradient GEMM).  A stage whose GEMMs are all of the
// one-tile class (small minibatches, rollout steps of few environments) goes out as ONE launch of up to four problems; otherwise
// the j-th GEMMs of both networks go out pairwise where they are of the same kind (they always are at equal depths; the tails of
// unequal depths, and a head opposite a hidden layer, go alone).  MOBROB_GEMM_PAIR=0: one launch per GEMM; =1: pairs only.
void run_queues(mobrob_ppo_engine* e, const GemmQueue& qa, const GemmQueue& qb, int width) {
  static const int pairing = env_int("MOBROB_GEMM_PAIR", 2);
  const size_t n = std::max(qa.size(), qb.size());
  for (size_t j0 = 0; j0 < n; j0 += width) {
    const GemmOp* st[4];
    int ns = 0;
    bool small = pairing >= 2;
    for (size_t j = j0; j < j0 + width && j < n; ++j)
      for (const GemmQueue* q : {&qa, &qb})
        if (j < q->size()) {
          st[ns++] = &(*q)[j];
          small = small && gemm_tile_class(e, (*q)[j]) == 11;
        }
    if (small && ns >= 2) { launch_multi(e, st, ns); continue; }
    for (size_t j = j0; j < j0 + width && j < n; ++j) {
      const GemmOp* a = j < qa.size() ? &qa[j] : nullptr;
      const GemmOp* b = j < qb.size() ? &qb[j] : nullptr;
      if (a && b && pairing >= 1 && a->mode == b->mode && a->epi == b->epi) { launch_op(e, *a, b); continue; }
      if (a) launch_op(e, *a);
      if (b) launch_op(e, *b);
    }
  }
}
// q: non-null = the GEMM is queued (run_queues pairs it with the other network's), null = launched now

// Y[M x Nn] = act(X[M x K] . W[Nn x K]^T + bias)
void linear_fwd(mobrob_ppo_engine* e, const float* X, int ldx, const float* W, int ldw, const float* bias, float* Y,
                int ldy, int M, int Nn, int K, bool tanh_, float* Z = nullptr, GemmQueue* q = nullptr) {
  GemmOp o;
  GemmArgs& g = o.g;
  g.A = X; g.B = W; g.C = Y; g.M = M; g.N = Nn; g.K = K; g.lda = ldx; g.ldb = ldw; g.ldc = ldy; g.bias = bias;
  g.act = e->cfg.activation;
  g.Z = (tanh_ && act_needs_z(g.act)) ? Z : nullptr; g.ldz = ldy;   // pre-activations for SiLU / GELU / Mish backward (same shape as Y)
  o.mode = MODE_NT; o.epi = tanh_ ? EPI_BIAS_TANH : EPI_BIAS;
  if (q) q->push_back(o); else launch_op(e, o);
}
// dZ[M x Nn] = (dY[M x K] . W[K x Nn]) * act'(.) ; column sums -> bias grad
void linear_bwd_input(mobrob_ppo_engine* e, const float* dY, int ldd, const float* W, int ldw, const float* H, int ldh,
                      float* dZ, int ldz, float* bias_grad, int M, int Nn, int K, GemmQueue* q = nullptr) {
  GemmOp o;
  GemmArgs& g = o.g;
  g.A = dY; g.B = W; g.C = dZ; g.M = M; g.N = Nn; g.K = K; g.lda = ldd; g.ldb = ldw; g.ldc = ldz;
  g.Hact = H; g.ldh = ldh; g.colsum = bias_grad; g.act = e->cfg.activation;
  o.mode = MODE_NN; o.epi = EPI_DTANH_COLSUM;
  if (q) q->push_back(o); else launch_op(e, o);
}
// dW[M x Nn] += dY[rows x M]^T . X[rows x Nn]
void linear_bwd_weight(mobrob_ppo_engine* e, const float* dY, int ldd, const float* X, int ldx, float* dW, int ldw,
                       int M, int Nn, int rows, GemmQueue* q = nullptr) {
  GemmOp o;
  GemmArgs& g = o.g;
  g.A = dY; g.B = X; g.C = dW; g.M = M; g.N = Nn; g.K = rows; g.lda = ldd; g.ldb = ldx; g.ldc = ldw;
  // waves of one pass over the output (launch_gemm's tiling: 64-row / 64-column wave tiles where the extents allow); the batch rows
  // are split until ~2048 waves are in flight (8 per CU) -- every split adds M x Nn float atomics, so not further
  const int wtiles = cdiv(M, M <= 32 ? 32 : 64) * cdiv(Nn, (M <= 32 || Nn <= 32) ? 32 : 64);
  int ksplit = std::max(1, std::min(cdiv(rows, 64), cdiv(2048, wtiles)));   // (launch_gemm then finds >= 2048 waves wherever the rows allow)
  g.kchunk = rup(cdiv(rows, ksplit), 8);
  o.ksplit = cdiv(rows, g.kchunk);
  o.mode = MODE_TN; o.epi = EPI_ATOMIC;
  if (q) q->push_back(o); else launch_op(e, o);
}

float* Pp(mobrob_ppo_engine* e, int t) { return e->params + e->offs[t]; }
float* Gp(mobrob_ppo_engine* e, int t) { return e->grads + e->offs[t]; }

// x3 packs of the hidden layers of both networks from the canonical parameters (kernels_fused.h): one launch
void pack_x3_all(mobrob_ppo_engine* e) {
  if (e->fused.net[0].W2x == nullptr) return;
  PackX3Args a{};
  const int w1[2] = {T_PW1, T_VW1}, w2[2] = {T_PW2, T_VW2};
  int maxthreads = 0;
  for (int n = 0; n < 2; ++n) {
    const int i1 = 3 * n, i2 = 3 * n + 1, i3 = 3 * n + 2;
    a.W[i1] = Pp(e, w1[n]); a.N[i1] = FH; a.K[i1] = e->D; a.ld[i1] = e->D; a.NB[i1] = FH / 32; a.KS[i1] = e->Dp / 16; a.scale[i1] = kTanhScale;
    a.out[i1] = reinterpret_cast<unsigned short*>(const_cast<unsigned*>(e->fused.net[n].W1x));
    a.W[i2] = Pp(e, w2[n]); a.N[i2] = FH; a.K[i2] = FH; a.ld[i2] = FH; a.NB[i2] = FH / 32; a.KS[i2] = FH / 16; a.scale[i2] = kTanhScale;
    a.out[i2] = reinterpret_cast<unsigned short*>(const_cast<unsigned*>(e->fused.net[n].W2x));
    a.W[i3] = Pp(e, w2[n]); a.N[i3] = FH; a.K[i3] = FH; a.ld[i3] = FH; a.NB[i3] = FH / 32; a.KS[i3] = FH / 16; a.scale[i3] = 1.0f; a.trans[i3] = 1;
    a.out[i3] = reinterpret_cast<unsigned short*>(const_cast<unsigned*>(e->fused.net[n].W2bx));
    maxthreads = std::max(maxthreads, std::max(a.NB[i1] * a.KS[i1], a.NB[i2] * a.KS[i2]) * 512);
  }
  hipLaunchKernelGGL(k_pack_x3_multi, dim3(cdiv(maxthreads, 256), 6), dim3(256), 0, e->stream, a);
  if (e->fused.train_chain) {  // chain packs of k_chain_train (kernels_chain.h)
    ChainPackArgs c{};
    const int w3[2] = {T_AW, T_VW};
    for (int n = 0; n < 2; ++n) {
      c.W1[n] = Pp(e, w1[n]); c.W2[n] = Pp(e, w2[n]); c.W3[n] = Pp(e, w3[n]);
      c.w1c[n] = reinterpret_cast<unsigned short*>(const_cast<unsigned*>(e->fused.net[n].W1c));
      c.w2c[n] = reinterpret_cast<unsigned short*>(const_cast<unsigned*>(e->fused.net[n].W2c));
      c.w2bc[n] = reinterpret_cast<unsigned short*>(const_cast<unsigned*>(e->fused.net[n].W2bc));
      c.w3c[n] = const_cast<float*>(e->fused.net[n].W3c); c.w3bc[n] = const_cast<float*>(e->fused.net[n].W3bc);
      c.head[n] = n == 0 ? e->A : 1;
    }
    c.D = e->D; c.Dp = e->Dp;
    hipLaunchKernelGGL(k_pack_chain, dim3(FH * FH / 256, 2), dim3(256), 0, e->stream, c);
  }
}

void repack(mobrob_ppo_engine* e) {
  auto pad = [&](const float* src, float* dst, int r, int c, int rp, int cp) {
    hipLaunchKernelGGL(k_pad_rows, dim3(cdiv(rp * cp, 256)), dim3(256), 0, e->stream, src, dst, r, c, rp, cp);
  };
  pad(Pp(e, T_PW1), e->pW1p, e->H1, e->D, e->H1, e->Dp);
  pad(Pp(e, T_VW1), e->vW1p, e->G1, e->D, e->G1, e->Dp);
  pad(Pp(e, T_AW), e->aWp, e->A, e->HL, e->Ap, e->HL);
  pad(Pp(e, T_VW), e->vWp, 1, e->GL, 8, e->GL);
  fused_repack(e->fused, e->params, e->offs, e->stream);
  pack_x3_all(e);
}

// forward of both networks on `rows` device rows of padded observations (ld = Dp); mu ld = Ap, v ld = 1
void forward_generic(mobrob_ppo_engine* e, const float* X, int rows, bool want_pi, float* mu_out, bool want_v,
                     float* v_out, bool keep_z = false) {
  // layer 0 reads the zero-padded copy of its weights (observation rows are padded to Dp columns); one to eight hidden layers.
  // keep_z (the training forward of a minibatch, rows <= Bl): layer l's pre-activations are left in its dz buffer for the backward
  // epilogue of the activations that need them (act_needs_z).  The two networks' GEMMs are queued and go out pairwise (run_queues).
  GemmQueue qp, qv;
  if (want_pi) {
    linear_fwd(e, X, e->Dp, e->pW1p, e->Dp, Pp(e, e->tPB[0]), e->hp[0], e->Hp[0], rows, e->Hp[0], e->Dp, true, keep_z ? e->dzp[0] : nullptr, &qp);
    for (int l = 1; l < e->Lp; ++l)
      linear_fwd(e, e->hp[l - 1], e->Hp[l - 1], Pp(e, e->tPW[l]), e->Hp[l - 1], Pp(e, e->tPB[l]), e->hp[l], e->Hp[l], rows, e->Hp[l], e->Hp[l - 1], true,
                 keep_z ? e->dzp[l] : nullptr, &qp);
    linear_fwd(e, e->hp[e->Lp - 1], e->HL, e->aWp, e->HL, Pp(e, T_AB), mu_out, e->Ap, rows, e->A, e->HL, false, nullptr, &qp);
  }
  if (want_v) {
    linear_fwd(e, X, e->Dp, e->vW1p, e->Dp, Pp(e, e->tVB[0]), e->hv[0], e->Hv[0], rows, e->Hv[0], e->Dp, true, keep_z ? e->dzv[0] : nullptr, &qv);
    for (int l = 1; l < e->Lv; ++l)
      linear_fwd(e, e->hv[l - 1], e->Hv[l - 1], Pp(e, e->tVW[l]), e->Hv[l - 1], Pp(e, e->tVB[l]), e->hv[l], e->Hv[l], rows, e->Hv[l], e->Hv[l - 1], true,
                 keep_z ? e->dzv[l] : nullptr, &qv);
    linear_fwd(e, e->hv[e->Lv - 1], e->GL, e->vWp, e->GL, Pp(e, T_VB), v_out, 1, rows, 1, e->GL, false, nullptr, &qv);
  }
  run_queues(e, qp, qv, 1);
}

void forward(mobrob_ppo_engine* e, const float* X, int rows, bool want_pi, float* mu_out, bool want_v, float* v_out) {
  if (e->fused.enabled && fused_forward(e->fused, X, rows, want_pi, mu_out, e->Ap, want_v, v_out, e->stream)) return;
  forward_generic(e, X, rows, want_pi, mu_out, want_v, v_out);
}

int value_net_width_sum(const mobrob_ppo_engine* e) {
  int s = 0;
  for (int l = 0; l < e->Lv; ++l) s += e->Hv[l];
  return s;
}
// the value network as the per-row evaluators take it (canonical parameters; layers beyond the network's depth are null)
ValueNetArgs value_net_args(mobrob_ppo_engine* e) {
  ValueNetArgs vn{};
  for (int l = 0; l < e->Lv; ++l) { vn.W[l] = Pp(e, e->tVW[l]); vn.b[l] = Pp(e, e->tVB[l]); vn.G[l] = e->Hv[l]; }
  vn.Wv = Pp(e, T_VW); vn.bv = Pp(e, T_VB);
  vn.L = e->Lv; vn.act = e->cfg.activation; vn.width_sum = value_net_width_sum(e);
  return vn;
}
BootNetArgs boot_args(mobrob_ppo_engine* e) { return BootNetArgs{value_net_args(e), (float)e->cfg.gamma, e->term_val}; }

void value_flagged(mobrob_ppo_engine* e, const float* obs_rows, const uint8_t* flags, float* out,
                   float* bootstrap_rewards = nullptr) {
  const size_t sm = (size_t)(e->D + value_net_width_sum(e) + 16) * sizeof(float);
  hipLaunchKernelGGL(k_value_flagged, dim3(e->N), dim3(256), sm, e->stream, obs_rows, e->Dp, flags, value_net_args(e), e->D, out,
                     bootstrap_rewards, (float)e->cfg.gamma);
}

// Philox key of the action-noise stream: data-parallel ranks must not share it
uint64_t eps_seed(const mobrob_ppo_engine* e) { return e->cfg.seed ^ (0xD1B54A32D192ED03ull * (uint64_t)(e->cfg.rank + 1)); }

void run_gae(mobrob_ppo_engine* e) {
  ProfScope ps(e, MOBROB_K_GAE);
  const double gl = e->cfg.gamma * e->cfg.gae_lambda;  // python: self.gamma * self.gae_lambda (float64)
  hipLaunchKernelGGL(k_gae, dim3(cdiv(e->N, kGaeEnvs)), dim3(kGaeThreads), 0, e->stream, e->rewards, e->values, e->es, e->last_values,
                     e->last_dones, (float)e->cfg.gamma, gl, e->T, e->N, e->adv, e->ret);
}

// gSDE: new exploration matrices for env rows [r0, r0 + n) (and, with `single`, the one matrix predict() uses for foreign batches)
void sde_resample(mobrob_ppo_engine* e, int r0, int n, uint32_t draw, const uint32_t* draw_base, bool single) {
  const int HLA = e->HL * e->A, per = cdiv(HLA, 4);
  hipLaunchKernelGGL(k_sde_resample, dim3(cdiv((n + (single ? 1 : 0)) * per, 256)), dim3(256), 0, e->stream, Pp(e, T_LOGSTD), HLA, e->A, e->sde_mode, r0, n,
                     eps_seed(e) ^ 0x5DE5DE5DE5DE5DEull, draw, draw_base, e->sde_E, single ? e->sde_E1 : (float*)nullptr);
}

// gSDE: variance of `rows` rows of the policy's last hidden activations (the forward has just produced them) into sde_var.
// fresh_table: recompute the std^2 table from log_std first (parameters may have changed since it was last built)
void sde_variance(mobrob_ppo_engine* e, int rows, bool fresh_table, float* lat2 = nullptr) {
  if (fresh_table)
    hipLaunchKernelGGL(k_sde_std2, dim3(cdiv(e->HL * e->A, 256)), dim3(256), 0, e->stream, Pp(e, T_LOGSTD), e->HL, e->A, e->sde_mode, e->sde_S2);
  hipLaunchKernelGGL(k_sde_var, dim3(cdiv(rows, 4)), dim3(256), 0, e->stream, e->hp[e->Lp - 1], e->HL, e->sde_S2, rows, e->HL, e->A, e->sde_var, e->Ap,
                     lat2);
}

// policy forward + sample for rows [r0, r0 + n) of rollout slot t (observations already in the slot).
// draw = Philox draw index of the step (the whole-step callers pass the running counter and advance it).
void act_rows(mobrob_ppo_engine* e, int t, int r0, int n, const float* eps_dev_or_null, uint32_t draw,
              const uint32_t* draw_base, float* clip_out = nullptr) {
  // clip_out: where the clipped actions of the rows go (default: the device staging rows; the pipelined host path
  // passes the caller's pinned buffer -- the sampling epilogue writes them over PCIe itself, no copy kernel)
  ProfScope ps(e, MOBROB_K_ACT);
  if (!clip_out) clip_out = e->clip_act + (size_t)r0 * e->A;
  const size_t row = (size_t)t * e->N + r0;
  const float* X = e->obs + row * e->Dp;
  if (e->fused.enabled) {
    FusedActArgs a{};
    a.X = X; a.rows = n; a.row0 = r0; a.want_pi = 1; a.want_v = 1; a.mu = nullptr; a.ldmu = e->Ap;
    a.v = e->values + row; a.sample = 1; a.A = e->A; a.log_std = Pp(e, T_LOGSTD); a.eps = eps_dev_or_null;
    a.seed = eps_seed(e); a.draw = draw; a.draw_base = draw_base; a.lo = (float)e->cfg.action_low; a.hi = (float)e->cfg.action_high;
    a.act_raw = e->actions + row * e->A; a.act_clip = clip_out; a.logp = e->logp + row;
    fused_launch_act(e->fused, a, e->stream);
    return;
  }
  forward(e, X, n, true, e->mu, true, e->values + row);
  if (e->sde) {
    // collect_rollouts: reset_noise(n_envs) at the start of a rollout and every sde_sample_freq steps (SB3 on_policy_algorithm.py);
    // the rows' matrices at this step's draw index (a function of (env, draw), whichever launch draws them)
    const int freq = e->cfg.sde_sample_freq;
    if (!e->sde_hold && (t == 0 || (freq > 0 && t % freq == 0))) sde_resample(e, r0, n, draw, draw_base, r0 == 0);
    // the std^2 table at the first step of a rollout (every row range's: ranges are enqueued independently; the parameters are
    // fixed from there to the end of the rollout -- and a captured rollout graph must rebuild it on every replay)
    sde_variance(e, n, t == 0);
    hipLaunchKernelGGL(k_sample_sde, dim3(cdiv(n, 4)), dim3(256), 0, e->stream, e->mu, e->Ap, e->hp[e->Lp - 1], e->HL, e->sde_var, e->Ap,
                       e->sde_E, r0, 0, n, e->HL, e->A, (float)e->cfg.action_low, (float)e->cfg.action_high,
                       e->actions + row * e->A, clip_out, e->logp + row);
    return;
  }
  hipLaunchKernelGGL(k_sample, dim3(cdiv(n, 256)), dim3(256), 0, e->stream, e->mu, e->Ap, Pp(e, T_LOGSTD),
                     eps_dev_or_null, n, e->A, (float)e->cfg.action_low, (float)e->cfg.action_high, eps_seed(e),
                     draw, draw_base, e->actions + row * e->A, clip_out, e->logp + row, r0);
}
void act_slot(mobrob_ppo_engine* e, int t, const float* eps_dev_or_null, bool device_counter = false) {
  act_rows(e, t, 0, e->N, eps_dev_or_null, device_counter ? (uint32_t)t : e->draw_counter,
           device_counter ? e->ctr_dev : nullptr);
  if (!device_counter) e->draw_counter++;
}

int upload_obs(mobrob_ppo_engine* e, const float* host, float* dev_rows, int rows) {
  HIPC(hipMemcpy2DAsync(dev_rows, (size_t)e->Dp * 4, host, (size_t)e->D * 4, (size_t)e->D * 4, rows,
                        hipMemcpyHostToDevice, e->stream));
  return MOBROB_OK;
}

// ---- the update's argument structs: one filler each for what does not change from minibatch to minibatch (the callers add rows /
// count / advstat / inv_bg, the slab count and group, b_local, stats_row) ----
template <class Args>   // the loss hyper-parameters, which FusedTrainArgs, Fused64TrainArgs and LossArgs name alike
void fill_loss_hyper(const mobrob_ppo_engine* e, Args& a) {
  a.log_std = e->params + e->offs[T_LOGSTD]; a.normalize = e->cfg.normalize_advantage;
  a.clip = (float)e->cfg.clip_range; a.vf_coef = (float)e->cfg.vf_coef; a.ent_coef = (float)e->cfg.ent_coef; a.clip_vf = (float)e->clip_vf;
}
Fused64TrainArgs train64_args(const mobrob_ppo_engine* e) {
  const FusedState& f = e->fused;
  Fused64TrainArgs a{};
  for (int n = 0; n < 2; ++n) { a.net[n] = f.net[n]; a.wpack[n] = reinterpret_cast<const float*>(f.net[n].W1f); }
  a.obs = e->obs; a.actions = e->actions; a.A = e->A; a.old_logp = e->logp; a.adv = e->adv; a.ret = e->ret; a.old_values = e->values;
  fill_loss_hyper(e, a);
  a.slabs = f.slabs; a.sums = e->grads + e->P; a.stamps = f.stamps;
  return a;
}
FusedTrainArgs train256_args(const mobrob_ppo_engine* e) {
  const FusedState& f = e->fused;
  FusedTrainArgs a{};
  a.net[0] = f.net[0]; a.net[1] = f.net[1];
  a.obs = e->obs; a.Dp = e->Dp; a.A = e->A; a.rec = f.train_rec; a.RW = train_rec_width(e->A);
  fill_loss_hyper(e, a);
  a.slabs = f.slabs; a.slab_floats = f.slab_floats; a.sums = e->grads + e->P; a.stamps = f.stamps;
  return a;
}
template <class Args>   // what SlabReduceArgs and Slab64ReduceArgs name alike
Args reduce_args(const mobrob_ppo_engine* e) {
  Args s{};
  s.slabs = e->fused.slabs; s.grads = e->grads; s.P = e->P;
  for (int i = 0; i < 14; ++i) s.offs[i] = e->offs[i];
  s.D = e->D; s.A = e->A; s.ent_coef = (float)e->cfg.ent_coef; s.sums = e->grads + e->P;
  s.rec_sum = e->use_norm_records ? e->norm_rec_sum : nullptr; s.rec_t = e->norm_rec_t;   // (inside train_loop with records on)
  return s;
}
Slab64ReduceArgs slab64_reduce_args(const mobrob_ppo_engine* e) { return reduce_args<Slab64ReduceArgs>(e); }
SlabReduceArgs slab_reduce_args(const mobrob_ppo_engine* e) {
  SlabReduceArgs s = reduce_args<SlabReduceArgs>(e);
  s.slab_floats = e->fused.slab_floats; s.Dp = e->Dp; s.h16 = e->A <= 16;
  return s;
}
StatsArgs stats_args(const mobrob_ppo_engine* e) {
  StatsArgs st{};
  st.loss_sums = e->grads + e->P; st.log_std = e->params + e->offs[T_LOGSTD]; st.n_act = e->A; st.sde = e->sde;
  st.ent_coef = (float)e->cfg.ent_coef; st.vf_coef = (float)e->cfg.vf_coef;
  return st;
}
// fused_init, step 1: the f32 weight packs of both networks, one allocation carved per network
int fused_carve_packs(mobrob_ppo_engine* e) {
  FusedState& f = e->fused;
  const int H = f.H;
  const size_t nW1 = (size_t)(H / 32) * (e->Dp / 8) * 256, nW2 = (size_t)(H / 32) * (H / 8) * 256;
  const size_t nW3f = (size_t)(H / 8) * 256, nW3b = (size_t)(H / 32) * 4 * 256;
  const size_t nW3h = (size_t)(H / 16) * 256;  // 16x16x4 pack of heads <= 16 wide (H = 256 train kernel)
  const size_t per_net = nW1 + 2 * nW2 + nW3f + nW3h + nW3b + 2 * H;
  f.packed_floats = 2 * per_net;
  CHK(dalloc(e, &f.packed, f.packed_floats));
  const int head_bias[2] = {T_AB, T_VB};
  for (int n = 0; n < 2; ++n) {
    float* p = f.packed + n * per_net;
    f.net[n].W1f = reinterpret_cast<const f32x4*>(p); p += nW1;
    f.net[n].W2f = reinterpret_cast<const f32x4*>(p); p += nW2;
    f.net[n].W3f = reinterpret_cast<const f32x4*>(p); p += nW3f;
    f.net[n].W2b = reinterpret_cast<const f32x4*>(p); p += nW2;
    f.net[n].W3b = reinterpret_cast<const f32x4*>(p); p += nW3b;
    f.net[n].b1s = p; p += H;
    f.net[n].b2s = p; p += H;
    f.net[n].W3h = reinterpret_cast<const f32x4*>(p); p += nW3h;  // last: the H = 64 kernels mirror [W1f, b2s] as one block
    f.net[n].b3 = e->params + e->offs[head_bias[n]];
    f.net[n].head = n == 0 ? e->A : 1;
    f.net[n].W1x = nullptr; f.net[n].W2x = nullptr; f.net[n].W2bx = nullptr;
    f.net[n].W1c = nullptr; f.net[n].W2c = nullptr; f.net[n].W2bc = nullptr; f.net[n].W3c = nullptr; f.net[n].W3bc = nullptr;
  }
  return MOBROB_OK;
}
// step 2, in arena order: gradient slabs; the epoch kernel's buffers (64 wide) or the x3 / chain packs and the training records (256 wide); stamps
int fused_alloc_buffers(mobrob_ppo_engine* e) {
  FusedState& f = e->fused;
  const int H = f.H;
  f.max_grid = 256;
  if (H == 64) {
    f.slab_floats = s64_size();
    // one slab per block (k_fused64_train), per tile (k_split64_train) or per two-wave workgroup (k_pair64_train)
    const int tiles_max = cdiv(std::min(e->Bl, e->N * e->T), GR);
    f.pair_nseq_max = std::min(kPairsPerCu * 256 / 2, tiles_max);
    CHK(dalloc(e, &f.slabs, (size_t)std::max(f.max_grid, 2 * f.pair_nseq_max) * f.slab_floats));
    f.lds_bytes = fused64_train_lds_bytes(e->Dp);
    f.lds_act_bytes = fused64_lds_bytes(e->Dp);
    CHK(dalloc(e, &e->epoch_bar, 1024));
    CHK(dalloc(e, &e->epoch_snap, (size_t)3 * e->P));
    CHK(dalloc(e, &e->epoch_consts, (size_t)2 * e->nmb));
    CHK(dalloc(e, &e->epoch_idx, (size_t)e->nmb));
  } else {
    f.slab_floats = slab_size(e->Dp);
    CHK(dalloc(e, &f.slabs, (size_t)f.max_grid * f.slab_floats));
    if (e->cfg.forward_x3 && e->cfg.activation == MOBROB_ACT_TANH && !env_switched_off("MOBROB_NO_X3")) {
      // x3 packs of the hidden layers of both networks (kernels_fused.h, gemm_x3_r32): rebuilt at the start of every rollout
      for (int n = 0; n < 2; ++n) {
        unsigned* w1 = nullptr; unsigned* w2 = nullptr; unsigned* w2b = nullptr;
        CHK(dalloc(e, &w1, (size_t)(H / 32) * (e->Dp / 16) * 192 * 4));
        CHK(dalloc(e, &w2, (size_t)(H / 32) * (H / 16) * 192 * 4));
        CHK(dalloc(e, &w2b, (size_t)(H / 32) * (H / 16) * 192 * 4));
        f.net[n].W1x = w1; f.net[n].W2x = w2; f.net[n].W2bx = w2b;
      }
      f.train_x3 = e->A <= 16 && e->Dp != 48 && !env_switched_off("MOBROB_NO_TRAIN_X3");
      // the register-chained gradient kernel (kernels_chain.h) takes the same shapes; MOBROB_NO_CHAIN=1 keeps k_fused_train<.., X3>
      f.train_chain = f.train_x3 && !env_switched_off("MOBROB_NO_CHAIN");
      if (f.train_chain) {
        const int K1 = (e->Dp + 31) / 32;
        for (int n = 0; n < 2; ++n) {
          unsigned* w1 = nullptr; unsigned* w2 = nullptr; unsigned* w2b = nullptr; float* w3 = nullptr; float* w3b = nullptr;
          CHK(dalloc(e, &w1, (size_t)K1 * 16 * 768));       // [k step][tile 16][3 pieces][64 lanes] x 16 bytes
          CHK(dalloc(e, &w2, (size_t)8 * 16 * 768));
          CHK(dalloc(e, &w2b, (size_t)8 * 16 * 768));
          CHK(dalloc(e, &w3, (size_t)16 * 64 * 4));
          CHK(dalloc(e, &w3b, (size_t)16 * 64 * 4));
          f.net[n].W1c = w1; f.net[n].W2c = w2; f.net[n].W2bc = w2b; f.net[n].W3c = w3; f.net[n].W3bc = w3b;
        }
        f.lds_chain_bytes = chain_lds_bytes(e->Dp);
      }
    }
    CHK(dalloc(e, &f.train_rec, (size_t)e->N * e->T * train_rec_width(e->A)));
    f.lds_bytes = fused_lds_bytes(e->Dp);
    f.lds_act_bytes = fused_lds_act_bytes(e->Dp);
  }
  return dalloc(e, &f.stamps, 32);
}
// step 3: the norm-record tables -- which (network, block, slot) of the reduction kernel holds which tensor, emulated here exactly
// as block_norm_records forms them (per wave: tensors by first occurrence; adjacent equal ones merge)
int build_norm_record_tables(mobrob_ppo_engine* e) {
  const FusedState& f = e->fused;
  const int nb = cdiv(f.slab_floats, 256);
  CHK(dalloc(e, &e->norm_rec_sum, (size_t)2 * nb * kNormRec));
  CHK(dalloc(e, &e->norm_rec_t, (size_t)2 * nb * kNormRec));
  CHK(dalloc(e, &e->fold_idx_dev, (size_t)2 * nb * kNormRec));
  const SlabReduceArgs s256 = slab_reduce_args(e);
  const Slab64ReduceArgs s64 = slab64_reduce_args(e);
  std::vector<std::vector<int>> per_tensor(13);
  for (int net = 0; net < 2; ++net)
    for (int b = 0; b < nb; ++b) {
      std::vector<int> recs;  // tensors of this block's records, in order
      for (int w = 0; w < 4; ++w) {
        std::vector<int> wave;
        for (int l = 0; l < 64; ++l) {
          const int p = b * 256 + w * 64 + l;
          const int dst = p < f.slab_floats ? (f.H == 64 ? slab64_to_canonical(s64, net, p) : slab_to_canonical(s256, net, p)) : -1;
          const int t = tensor_of_canonical(e->offs, e->P, dst);
          if (t >= 0 && std::find(wave.begin(), wave.end(), t) == wave.end()) wave.push_back(t);
        }
        for (int t : wave)
          if (recs.empty() || recs.back() != t) recs.push_back(t);
      }
      if ((int)recs.size() > kNormRec) return fail(MOBROB_ERR_INVALID, "norm record table: %zu tensors in one reduction block", recs.size());
      for (size_t k = 0; k < recs.size(); ++k) per_tensor[recs[k]].push_back((net * nb + b) * kNormRec + (int)k);
    }
  std::vector<int> fold;
  for (int t = 0; t < 13; ++t) {
    e->fold_start[t] = (int)fold.size();
    fold.insert(fold.end(), per_tensor[t].begin(), per_tensor[t].end());
  }
  e->fold_start[13] = (int)fold.size();
  if (fold.size() > 1024) return fail(MOBROB_ERR_INVALID, "norm record table too large (%zu)", fold.size());
  if (!e->plan_only)
    HIPC(hipMemcpyAsync(e->fold_idx_dev, fold.data(), fold.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  if (!e->plan_only) HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}

int fused_init(mobrob_ppo_engine* e) {
  FusedState& f = e->fused;
  // (every fused kernel's epilogue is tanh: ReLU networks run the generic GEMM chain)
  f.enabled = e->cfg.fast_kernels && e->cfg.activation == MOBROB_ACT_TANH && e->Lp == 2 && e->Lv == 2 && !e->sde &&
              fused_shape_ok(e->D, e->A, e->H1, e->H2, e->G1, e->G2);   // (other depths: generic GEMM chain)
  if (!f.enabled) return MOBROB_OK;
  f.D = e->D; f.Dp = e->Dp; f.A = e->A; f.H = e->H1;
  if ((uint64_t)(e->T + 1) * e->N * e->Dp * 4ull >= (1ull << 32) || (uint64_t)e->T * e->N * e->A * 4ull >= (1ull << 32) ||
      (uint64_t)e->T * e->N * train_rec_width(e->A) * 4ull >= (1ull << 32)) {
    f.enabled = false;  // the fused kernels address rollout rows and training records with 32-bit byte offsets
    return MOBROB_OK;
  }
  CHK(fused_carve_packs(e));
  CHK(fused_alloc_buffers(e));
  if (!e->plan_only) HIPC(fused_set_lds_attr(f));
  return build_norm_record_tables(e);
}
// Which 64-wide gradient kernel a minibatch of B rows takes and how its slabs are reduced: decided here and nowhere else
// (fused64_minibatch_grad launches from it; epoch_kernel_eligible asks it about the largest minibatch of an epoch).
struct Grad64Plan {
  int ntiles, grid;    // 32-row tiles; k_fused64_train's workgroups (g_train_waves one-tile waves each, both networks)
  bool split;          // small: one workgroup per (tile, network) (kernels_split64.h); its per-tile slabs are folded in groups of g_train_waves
                       // tiles, which reproduces the block kernel bit for bit as long as that kernel would have given every wave at most one tile
  bool pair;           // large: persistent two-wave workgroups, four per CU (kernels_pair64.h); one slab per workgroup of two pairs
  int nseq, nbseq;     // k_pair64_train: tile sequences, and workgroups per network
  int nblocks, group;  // the reduction's slab count and fold group (Slab64ReduceArgs)
  bool wide;           // k_slab64_reduce_wide: more than 128 slabs per network
};
Grad64Plan grad64_plan(const mobrob_ppo_engine* e, int B) {
  const FusedState& f = e->fused;
  const int tw = g_train_waves(e->Dp);
  Grad64Plan p{};
  p.ntiles = cdiv(B, GR);
  p.grid = 2 * std::min(f.max_grid / 2, cdiv(p.ntiles, tw));
  p.split = p.ntiles <= e->split64_max_tiles && 2 * p.ntiles <= f.max_grid && p.ntiles <= (p.grid / 2) * tw;
  p.pair = !p.split && e->pair64_min_tiles > 0 && p.ntiles >= e->pair64_min_tiles;
  p.nseq = std::min(p.ntiles, f.pair_nseq_max); p.nbseq = (p.nseq + 1) / 2;
  p.nblocks = p.split ? 2 * p.ntiles : (p.pair ? 2 * p.nbseq : p.grid); p.group = p.split ? tw : 1;
  p.wide = p.pair && p.nbseq > 128;
  return p;
}
// 64-wide networks: one independent wave per 32-row tile (kernels_fused64.h)
void fused64_minibatch_grad(mobrob_ppo_engine* e, int mb, int start, int B, float inv_bg) {
  FusedState& f = e->fused;
  const Grad64Plan pl = grad64_plan(e, B);
  Fused64TrainArgs a = train64_args(e);
  a.rows = e->rows + start; a.count = B; a.advstat = e->advstat + 4 * (size_t)mb; a.inv_bg = inv_bg;
  {
    ProfScope ps(e, MOBROB_K_TRAIN_GRAD);
    if (pl.split) split64_launch_train(f, a, pl.ntiles, e->stream);
    else if (pl.pair) pair64_launch_train(f, a, pl.nseq, pl.nbseq, e->stream);
    else fused64_launch_train(f, a, pl.grid, e->stream);
  }
  ProfScope pr(e, MOBROB_K_GRAD_REDUCE);
  Slab64ReduceArgs s = slab64_reduce_args(e);
  s.nblocks = pl.nblocks; s.group = pl.group; s.b_local = (float)B; s.inv_bg = inv_bg;
  if (pl.wide) hipLaunchKernelGGL(k_slab64_reduce_wide, dim3(cdiv(s64_size(), 256), 2), dim3(1024), 0, e->stream, s);
  else hipLaunchKernelGGL(k_slab64_reduce, dim3(cdiv(s64_size(), 256), 2), dim3(256), 0, e->stream, s);
}

// The training records (kernels_fused.h) are packed once per rollout: every call that can change actions / values /
// log-probs / advantages / returns clears train_rec_valid (rollouts, GAE, write_buffer); a caller that obtained a device
// pointer to one of them (buffer_info) can write without the engine seeing it, so from then on they are re-packed before
// every gradient launch.
void ensure_train_records(mobrob_ppo_engine* e) {
  if (!e->fused.train_rec || (e->train_rec_valid && !e->train_rec_external)) return;
  TrainRecArgs r{};
  r.actions = e->actions; r.old_logp = e->logp; r.adv = e->adv; r.ret = e->ret; r.values = e->values;
  r.A = e->A; r.RW = train_rec_width(e->A); r.rows = e->N * e->T; r.rec = e->fused.train_rec;
  const long long items = (long long)r.rows * (r.RW / 4);
  hipLaunchKernelGGL(k_build_train_records, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, e->stream, r);
  e->train_rec_valid = true;
}

// fused minibatch gradient: one persistent kernel + the deterministic slab reduction
void fused_minibatch_grad(mobrob_ppo_engine* e, int mb, int start, int B, float inv_bg) {
  FusedState& f = e->fused;
  ensure_train_records(e);
  FusedTrainArgs a = train256_args(e);
  a.rows = e->rows + start; a.count = B; a.advstat = e->advstat + 4 * (size_t)mb; a.inv_bg = inv_bg;
  const int grid = 2 * std::min(f.max_grid / 2, cdiv(B, FR));
  // the 8 loss accumulators behind the gradient vector were zeroed by the previous k_adam_pack (or at allocation)
  {
    ProfScope ps(e, MOBROB_K_TRAIN_GRAD);
    fused_launch_train(f, a, grid, e->stream);
  }
  ProfScope pr(e, MOBROB_K_GRAD_REDUCE);
  SlabReduceArgs s = slab_reduce_args(e);
  s.nslabs = grid; s.b_local = (float)B; s.inv_bg = inv_bg;
  hipLaunchKernelGGL(k_slab_reduce, dim3(cdiv(f.slab_floats, 256), 2), dim3(256), 0, e->stream, s);
}

// generic GEMM chain: gather, forward, loss, backward of both networks (kernels_generic.h)
void generic_minibatch_grad(mobrob_ppo_engine* e, int mb, int start, int B, float inv_bg) {
  ProfScope ps(e, MOBROB_K_TRAIN_GRAD);
  // (the gather also zeroes the gradient vector + loss sums and the gSDE GEMM's output: everything this step adds into with atomics)
  hipLaunchKernelGGL(k_gather, dim3(cdiv(B * (e->Dp / 4), 256)), dim3(256), 0, e->stream, e->rows + start, B, e->obs, e->Dp,
                     e->actions, e->A, e->logp, e->adv, e->ret, e->Xg, e->actg, e->lpg, e->advg, e->retg, e->values,
                     e->clip_vf >= 0.0 ? e->oldvg : (float*)nullptr, e->grads, e->P + 8, e->sde ? e->sde_graw : (float*)nullptr,
                     e->sde ? e->HL * e->A : 0);
  forward_generic(e, e->Xg, B, true, e->mu, true, e->vout, true);
  LossArgs L{};
  L.mu = e->mu; L.ldmu = e->Ap; L.v = e->vout; L.actions = e->actg; L.old_logp = e->lpg; L.adv = e->advg;
  L.ret = e->retg; L.advstat = e->advstat + 4 * (size_t)mb; L.B = B; L.A = e->A;
  fill_loss_hyper(e, L);
  L.old_v = e->oldvg; L.inv_bg = inv_bg; L.dmu = e->dmu; L.lddmu = e->Ap; L.dv = e->dv; L.lddv = 8;
  L.sums = e->grads + e->P; L.g_log_std = Gp(e, T_LOGSTD); L.g_b_action = Gp(e, T_AB); L.g_b_value = Gp(e, T_VB);
  if (e->sde) {
    sde_variance(e, B, true, e->sde_lat2);   // (log_std moved in the previous optimizer step; latent^2 for the gradient GEMM on the way)
    L.lat = e->hp[e->Lp - 1]; L.HL = e->HL; L.var = e->sde_var; L.ldvar = e->Ap; L.gsig = e->sde_gsig; L.ldg = e->Ap;
  }
  // (the padding columns of dmu / dv -- K padding of the NN GEMMs -- are zeroed by k_loss itself)
  hipLaunchKernelGGL(k_loss, dim3(cdiv(B, 256)), dim3(256), loss_lds_bytes(e->A), e->stream, L);
  if (e->sde) {   // g_log_std = 2 std (d std / d log_std) * ((latent^2)^T . gsig) (summed over the actions without full_std): the entropy term is inside gsig
    linear_bwd_weight(e, e->sde_lat2, e->HL, e->sde_gsig, e->Ap, e->sde_graw, e->A, e->HL, e->A, B);
    hipLaunchKernelGGL(k_sde_scale_grad, dim3(cdiv(e->HL * e->A, 256)), dim3(256), 0, e->stream, Gp(e, T_LOGSTD), e->sde_graw, Pp(e, T_LOGSTD), e->HL,
                       e->A, e->sde_mode);
  }   // (state-independent log_std: its entropy term is added by k_loss)
  // backward of both networks, last hidden layer first: dW of the layer above, then dz of this layer (dtanh / dReLU + bias sums)
  GemmQueue qp, qv;
  auto backward = [&](GemmQueue* q, int L, const int* Hw, float* const* h, float* const* dz, const float* dhead, int ldd, const float* headWp,
                      int head_rows, int head_pad, int t_headW, const int* tW, const int* tB) {
    const int HLw = Hw[L - 1];
    linear_bwd_weight(e, dhead, ldd, h[L - 1], HLw, Gp(e, t_headW), HLw, head_rows, HLw, B, q);
    linear_bwd_input(e, dhead, ldd, headWp, HLw, h[L - 1], HLw, dz[L - 1], HLw, Gp(e, tB[L - 1]), B, HLw, head_pad, q);
    for (int l = L - 1; l >= 1; --l) {
      linear_bwd_weight(e, dz[l], Hw[l], h[l - 1], Hw[l - 1], Gp(e, tW[l]), Hw[l - 1], Hw[l], Hw[l - 1], B, q);
      linear_bwd_input(e, dz[l], Hw[l], Pp(e, tW[l]), Hw[l - 1], h[l - 1], Hw[l - 1], dz[l - 1], Hw[l - 1], Gp(e, tB[l - 1]), B, Hw[l - 1], Hw[l], q);
    }
    linear_bwd_weight(e, dz[0], Hw[0], e->Xg, e->Dp, Gp(e, tW[0]), e->D, Hw[0], e->D, B, q);
  };
  // both networks' chains alternate weight-gradient and input-gradient GEMMs from the head down: queued, then launched pairwise
  backward(&qp, e->Lp, e->Hp, e->hp, e->dzp, e->dmu, e->Ap, e->aWp, e->A, e->Ap, T_AW, e->tPW, e->tPB);
  backward(&qv, e->Lv, e->Hv, e->hv, e->dzv, e->dv, 8, e->vWp, 1, 8, T_VW, e->tVW, e->tVB);
  run_queues(e, qp, qv, 2);
}

// ---- rollout streamer --------------------------------------------------------------------------------
bool is_pinned(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: clear the sticky error
    return false;
  }
  return at.type == hipMemoryTypeHost;
}
// What the SERVED host collector (collect_host_served) may be handed: the rollout kernel's hand-over is built on system-scope
// write-through stores, relaxed flag words and one acquire per step, which is sound for COHERENT (fine-grained) host memory --
// hipHostMalloc(Coherent) and hipHostRegister blocks while HIP_HOST_COHERENT is not 0.  A non-coherent allocation is refused by
// name, and BOTH ends of the range the kernel reads / writes must lie in device-visible host memory (the first byte alone says
// nothing about an [N][D] array).
const char* served_buffer_problem(const void* p, size_t bytes) {
  if (!p || bytes == 0) return "a null or empty buffer";
  const bool default_noncoherent = env_int("HIP_HOST_COHERENT", 1) == 0;
  const char* ends[2] = {static_cast<const char*>(p), static_cast<const char*>(p) + bytes - 1};
  for (const char* q : ends) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, q) != hipSuccess) {
      (void)hipGetLastError();
      return q == ends[0] ? "pageable buffers" : "a buffer whose end lies outside the pinned block";
    }
    if (at.type != hipMemoryTypeHost) return "buffers that are not pinned host memory";
    if (at.allocationFlags & hipHostMallocNonCoherent) return "a non-coherent host allocation (hipHostMallocNonCoherent)";
    if (default_noncoherent && !(at.allocationFlags & hipHostMallocCoherent))
      return "host memory that is non-coherent by default (HIP_HOST_COHERENT=0) and was not allocated hipHostMallocCoherent";
  }
  return nullptr;
}
// The per-step calls of the pipelined host path see the same few buffers for a whole rollout: a pointer that was
// found pinned is remembered until the next rollout_begin (the driver query costs about a microsecond each time).
bool is_pinned_cached(mobrob_ppo_engine* e, const void* p) {
  for (const void* q : e->pinned_seen)
    if (q == p) return true;
  if (!is_pinned(p)) return false;
  e->pinned_seen[e->pinned_seen_n++ % 8] = p;
  return true;
}
int streamer_init(mobrob_ppo_engine* e) {
  if (e->cstream) return MOBROB_OK;
  const size_t N = e->N, D = e->D, A = e->A;
  HIPC(hipStreamCreateWithFlags(&e->cstream, hipStreamNonBlocking));
  HIPC(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
  HIPC(hipEventCreateWithFlags(&e->ev_k, hipEventDisableTiming));
  HIPC(hipEventCreateWithFlags(&e->ev_store, hipEventDisableTiming));
  for (auto& st : e->stage) {
    HIPC(hipHostMalloc((void**)&st.obs, N * D * 4, hipHostMallocDefault));
    HIPC(hipHostMalloc((void**)&st.eps, N * A * 4, hipHostMallocDefault));
    HIPC(hipHostMalloc((void**)&st.rew, N * 4, hipHostMallocDefault));
    HIPC(hipHostMalloc((void**)&st.term, N * D * 4, hipHostMallocDefault));
    HIPC(hipHostMalloc((void**)&st.dones, N, hipHostMallocDefault));
    HIPC(hipHostMalloc((void**)&st.trunc, N, hipHostMallocDefault));
  }
  HIPC(hipHostMalloc((void**)&e->o_raw, N * A * 4, hipHostMallocDefault));
  HIPC(hipHostMalloc((void**)&e->o_clip, N * A * 4, hipHostMallocDefault));
  HIPC(hipHostMalloc((void**)&e->o_val, N * 4, hipHostMallocDefault));
  HIPC(hipHostMalloc((void**)&e->o_lp, N * 4, hipHostMallocDefault));
  return MOBROB_OK;
}
// source pointer for an async H2D: the caller's buffer if it is pinned (zero copy), else a pinned staging copy
template <typename Tp>
const Tp* stage_in(const Tp* user, Tp* staging, size_t count) {
  if (is_pinned(user)) return user;
  memcpy(staging, user, count * sizeof(Tp));
  return staging;
}
int upload_obs_on(mobrob_ppo_engine* e, hipStream_t st, const float* host, float* dev_rows, int rows) {
  HIPC(hipMemcpy2DAsync(dev_rows, (size_t)e->Dp * 4, host, (size_t)e->D * 4, (size_t)e->D * 4, rows,
                        hipMemcpyHostToDevice, st));
  return MOBROB_OK;
}

// net_arch as the config carries it: pi_hidden[0 .. 1], pi_hidden3, pi_hidden_ext[0 .. 4] (likewise vf); a width of 0 ends the list
void cfg_widths(const mobrob_ppo_config_t* c, int* pw, int* vw) {
  pw[0] = c->pi_hidden[0]; pw[1] = c->pi_hidden[1]; pw[2] = c->pi_hidden3;
  vw[0] = c->vf_hidden[0]; vw[1] = c->vf_hidden[1]; vw[2] = c->vf_hidden3;
  for (int i = 3; i < kMaxHidden; ++i) { pw[i] = c->pi_hidden_ext[i - 3]; vw[i] = c->vf_hidden_ext[i - 3]; }
}

static_assert(ACT_TANH == MOBROB_ACT_TANH && ACT_RELU == MOBROB_ACT_RELU && ACT_ELU == MOBROB_ACT_ELU && ACT_LEAKY_RELU == MOBROB_ACT_LEAKY_RELU &&
              ACT_SIGMOID == MOBROB_ACT_SIGMOID && ACT_SOFTPLUS == MOBROB_ACT_SOFTPLUS && ACT_SOFTSIGN == MOBROB_ACT_SOFTSIGN &&
              ACT_HARDTANH == MOBROB_ACT_HARDTANH && ACT_RELU6 == MOBROB_ACT_RELU6 && ACT_SILU == MOBROB_ACT_SILU &&
              ACT_GELU == MOBROB_ACT_GELU && ACT_MISH == MOBROB_ACT_MISH && ACT_COUNT == MOBROB_ACT_COUNT,
              "kernels_generic.h activation codes are the header's");

int check_cfg(const mobrob_ppo_config_t* c) {
  if (c->abi_version != MOBROB_PPO_ABI_VERSION) return fail(MOBROB_ERR_INVALID, "abi_version %d != %d", c->abi_version, MOBROB_PPO_ABI_VERSION);
  if (c->obs_dim < 1 || c->act_dim < 1) return fail(MOBROB_ERR_INVALID, "obs_dim/act_dim must be >= 1");
  {  // one to eight hidden layers per network: [h1, h2, ...] with trailing zeros, every width a positive multiple of 8
    int pw[kMaxHidden], vw[kMaxHidden];
    cfg_widths(c, pw, vw);
    for (const int* w : {pw, vw}) {
      bool ended = false;
      for (int i = 0; i < kMaxHidden; ++i) {
        if (w[i] == 0 && i > 0) { ended = true; continue; }
        if (ended || w[i] < 8 || w[i] % 8)
          return fail(MOBROB_ERR_INVALID, "hidden widths must be positive multiples of 8, one to %d layers per network (a width of 0 ends the list)", kMaxHidden);
      }
    }
  }
  if (c->n_envs < 1 || c->n_steps < 1 || c->batch_size < 1 || c->n_epochs < 1)
    return fail(MOBROB_ERR_INVALID, "n_envs, n_steps, batch_size, n_epochs must be >= 1");
  if (c->world_size < 1 || c->rank < 0 || c->rank >= c->world_size) return fail(MOBROB_ERR_INVALID, "bad rank/world_size");
  if (c->batch_size % c->world_size) return fail(MOBROB_ERR_INVALID, "batch_size must be divisible by world_size");
  if ((int64_t)c->n_envs * c->n_steps > (int64_t)1 << 30) return fail(MOBROB_ERR_INVALID, "rollout too large");
  if (c->use_sde != 0 && c->use_sde != 1) return fail(MOBROB_ERR_INVALID, "use_sde must be 0 or 1");
  if ((c->sde_full_std != 0 && c->sde_full_std != 1) || (c->sde_use_expln != 0 && c->sde_use_expln != 1))
    return fail(MOBROB_ERR_INVALID, "sde_full_std / sde_use_expln must be 0 or 1");
  if (c->activation < 0 || c->activation >= MOBROB_ACT_COUNT) return fail(MOBROB_ERR_INVALID, "activation must be one of MOBROB_ACT_* (0 .. %d)", MOBROB_ACT_COUNT - 1);
  return MOBROB_OK;
}

}  // namespace

extern "C" {

int mobrob_ppo_abi_version(void) { return MOBROB_PPO_ABI_VERSION; }
const char* mobrob_ppo_last_error(void) { return g_err.c_str(); }

void mobrob_ppo_default_config(mobrob_ppo_config_t* c) {
  memset(c, 0, sizeof *c);
  c->abi_version = MOBROB_PPO_ABI_VERSION;
  c->obs_dim = 58; c->act_dim = 12;
  c->pi_hidden[0] = c->pi_hidden[1] = 64;
  c->vf_hidden[0] = c->vf_hidden[1] = 64;
  c->n_envs = 1; c->n_steps = 2048; c->batch_size = 64; c->n_epochs = 10;
  c->gamma = 0.99; c->gae_lambda = 0.95; c->clip_range = 0.2; c->ent_coef = 0.0; c->vf_coef = 0.5;
  c->max_grad_norm = 0.5; c->learning_rate = 3e-4; c->adam_beta1 = 0.9; c->adam_beta2 = 0.999; c->adam_eps = 1e-5;
  c->action_low = -1.0; c->action_high = 1.0;
  c->normalize_advantage = 1; c->seed = 0; c->device_id = 0; c->rank = 0; c->world_size = 1; c->fast_kernels = 1;
  c->rollout_graph = 1;
  c->rollout_persistent = 1;
  c->forward_x3 = 1;
  c->use_sde = 0; c->sde_sample_freq = -1; c->sde_full_std = 1; c->sde_use_expln = 0;
}

void* mobrob_ppo_host_alloc(size_t bytes) {
  void* p = nullptr;
  // coherent (fine-grained) whatever HIP_HOST_COHERENT says: the zero-copy and served collectors hand data over through it
  if (hipHostMalloc(&p, bytes, hipHostMallocCoherent | hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
    (void)hipGetLastError();
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  }
  return p;
}
void mobrob_ppo_host_free(void* p) { if (p) (void)hipHostFree(p); }

int mobrob_ppo_host_register(void* p, size_t bytes) {
  if (!p || bytes == 0) return fail(MOBROB_ERR_INVALID, "host_register: null pointer or empty range");
  hipError_t r = hipHostRegister(p, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
  if (r != hipSuccess) {
    (void)hipGetLastError();
    return fail(MOBROB_ERR_HIP, "hipHostRegister(%p, %zu): %s", p, bytes, hipGetErrorString(r));
  }
  // the zero-copy kernels dereference the HOST address: it must also be the device address of the mapping
  void* d = nullptr;
  r = hipHostGetDevicePointer(&d, p, 0);
  if (r != hipSuccess || d != p) {
    (void)hipGetLastError();
    (void)hipHostUnregister(p);
    return fail(MOBROB_ERR_HIP, "host_register: the registered range is not device visible at its host address (%p -> %p)", p, d);
  }
  return MOBROB_OK;
}
int mobrob_ppo_host_unregister(void* p) {
  if (!p) return fail(MOBROB_ERR_INVALID, "host_unregister: null pointer");
  hipError_t r = hipHostUnregister(p);
  if (r != hipSuccess) {
    (void)hipGetLastError();
    return fail(MOBROB_ERR_HIP, "hipHostUnregister(%p): %s", p, hipGetErrorString(r));
  }
  return MOBROB_OK;
}

}  // extern "C"

namespace {

// host-only: dimensions, parameter offsets, the norm chunk table
int engine_dims(mobrob_ppo_engine* e, const mobrob_ppo_config_t* cfg) {
  e->cfg = *cfg;
  e->D = cfg->obs_dim; e->Dp = padded_obs_dim(cfg->obs_dim); e->A = cfg->act_dim; e->Ap = rup(cfg->act_dim, 8);
  int pw[kMaxHidden], vw[kMaxHidden];   // (check_cfg has validated the pattern)
  cfg_widths(cfg, pw, vw);
  e->Lp = e->Lv = 0;
  for (int l = 0; l < kMaxHidden; ++l) { e->Hp[l] = e->Hv[l] = 0; }
  for (int l = 0; l < kMaxHidden && pw[l] > 0; ++l) e->Hp[e->Lp++] = pw[l];
  for (int l = 0; l < kMaxHidden && vw[l] > 0; ++l) e->Hv[e->Lv++] = vw[l];
  e->HL = e->Hp[e->Lp - 1]; e->GL = e->Hv[e->Lv - 1];
  e->H1 = e->Hp[0]; e->H2 = e->Hp[1]; e->G1 = e->Hv[0]; e->G2 = e->Hv[1];
  e->N = cfg->n_envs; e->T = cfg->n_steps;
  e->Bl = cfg->batch_size / cfg->world_size;
  const int total = e->N * e->T;
  e->nmb = cdiv(total, e->Bl);
  e->rows_max = std::max(e->N, std::min(e->Bl, total));
  int sizes[kMaxTensors] = {0};
  int nt = 0;
  e->sde = cfg->use_sde != 0;
  e->sde_mode = SdeMode{cfg->sde_full_std != 0, cfg->sde_use_expln != 0};
  sizes[nt++] = e->sde ? e->HL * (e->sde_mode.full ? e->A : 1) : e->A;   // log_std ([A]; gSDE: [HL][A], or [HL][1] without full_std)
  for (int l = 0; l < e->Lp; ++l) { e->tPW[l] = nt; sizes[nt++] = e->Hp[l] * (l ? e->Hp[l - 1] : e->D); e->tPB[l] = nt; sizes[nt++] = e->Hp[l]; }
  for (int l = 0; l < e->Lv; ++l) { e->tVW[l] = nt; sizes[nt++] = e->Hv[l] * (l ? e->Hv[l - 1] : e->D); e->tVB[l] = nt; sizes[nt++] = e->Hv[l]; }
  e->tAW = nt; sizes[nt++] = e->A * e->HL; e->tAB = nt; sizes[nt++] = e->A;
  e->tVWh = nt; sizes[nt++] = e->GL; e->tVBh = nt; sizes[nt++] = 1;
  e->ntens = nt;
  e->offs[0] = 0;
  for (int i = 0; i < nt; ++i) e->offs[i + 1] = e->offs[i] + sizes[i];
  for (int i = nt; i < kMaxTensors; ++i) e->offs[i + 1] = e->offs[nt];
  e->P = e->offs[nt];
  e->stats_cap = std::max(64, 4 * e->nmb * cfg->n_epochs);
  // chunk table for the gradient-norm reduction: <= 4096 elements per block, chunks sorted by tensor
  e->chunk_table.clear();
  for (int tt = 0; tt < e->ntens; ++tt)
    for (int s0 = e->offs[tt]; s0 < e->offs[tt + 1]; s0 += 4096)
      e->chunk_table.push_back(NormChunk{tt, s0, std::min(s0 + 4096, e->offs[tt + 1]), 0});
  e->nchunks = (int)e->chunk_table.size();
  if (e->nchunks > 256) return fail(MOBROB_ERR_INVALID, "parameter vector too large for the norm chunk table (%d chunks)", e->nchunks);
  return MOBROB_OK;
}

// carve every device buffer out of the arena (or, with plan_only, just add up the bytes)
int engine_alloc(mobrob_ppo_engine* e) {
  const size_t P = e->P, N = e->N, T = e->T, Dp = e->Dp, A = e->A, Bl = std::min(e->Bl, e->N * e->T), R = e->rows_max;
  CHK(dalloc(e, &e->params, P)); CHK(dalloc(e, &e->grads, P + 8)); CHK(dalloc(e, &e->m, P)); CHK(dalloc(e, &e->v, P));
  CHK(dalloc(e, &e->pW1p, (size_t)e->H1 * Dp)); CHK(dalloc(e, &e->vW1p, (size_t)e->G1 * Dp));
  CHK(dalloc(e, &e->aWp, (size_t)e->Ap * e->HL)); CHK(dalloc(e, &e->vWp, (size_t)8 * e->GL));
  CHK(dalloc(e, &e->obs, (T + 1) * N * Dp)); CHK(dalloc(e, &e->actions, T * N * A));
  CHK(dalloc(e, &e->rewards, T * N)); CHK(dalloc(e, &e->es, T * N)); CHK(dalloc(e, &e->values, (T + 1) * N));
  e->last_values = e->values + T * N;  // V(last_obs) sits behind the stored values: one batched pass covers both
  CHK(dalloc(e, &e->logp, T * N)); CHK(dalloc(e, &e->adv, T * N)); CHK(dalloc(e, &e->ret, T * N));
  CHK(dalloc(e, &e->last_dones, N)); CHK(dalloc(e, &e->prev_dones, N));
  CHK(dalloc(e, &e->dones_tmp, N)); CHK(dalloc(e, &e->clip_act, N * A)); CHK(dalloc(e, &e->rew_tmp, N));
  CHK(dalloc(e, &e->term_obs, N * Dp)); CHK(dalloc(e, &e->term_val, N)); CHK(dalloc(e, &e->eps_dev, R * A));
  CHK(dalloc(e, &e->trunc_dev, N)); CHK(dalloc(e, &e->dones_u8, N)); CHK(dalloc(e, &e->ep_len, N)); CHK(dalloc(e, &e->ep_len2, N)); CHK(dalloc(e, &e->ctr_dev, 2));
  CHK(dalloc(e, &e->rows, T * N)); CHK(dalloc(e, &e->perm_dev, T * N)); CHK(dalloc(e, &e->advstat, (size_t)e->nmb * 4)); CHK(dalloc(e, &e->advbins, (size_t)e->nmb * 2 + 1)); CHK(dalloc(e, &e->expvar_part, (size_t)kEvBlocks * 4));  // + two 32-bit max words
  CHK(dalloc(e, &e->stats, (size_t)e->stats_cap * 8));
  CHK(dalloc(e, &e->Xg, Bl * Dp)); CHK(dalloc(e, &e->actg, Bl * A)); CHK(dalloc(e, &e->lpg, Bl));
  CHK(dalloc(e, &e->advg, Bl)); CHK(dalloc(e, &e->retg, Bl)); CHK(dalloc(e, &e->oldvg, Bl));
  for (int l = 0; l < e->Lp; ++l) CHK(dalloc(e, &e->hp[l], R * e->Hp[l]));
  for (int l = 0; l < e->Lv; ++l) CHK(dalloc(e, &e->hv[l], R * e->Hv[l]));
  CHK(dalloc(e, &e->mu, R * e->Ap)); CHK(dalloc(e, &e->vout, R));
  CHK(dalloc(e, &e->dmu, Bl * e->Ap)); CHK(dalloc(e, &e->dv, Bl * 8));
  for (int l = 0; l < e->Lp; ++l) CHK(dalloc(e, &e->dzp[l], Bl * e->Hp[l]));
  for (int l = 0; l < e->Lv; ++l) CHK(dalloc(e, &e->dzv[l], Bl * e->Hv[l]));
  CHK(dalloc(e, &e->pred_obs, R * Dp)); CHK(dalloc(e, &e->pred_act, R * A));
  if (e->sde) {
    CHK(dalloc(e, &e->sde_E, N * (size_t)e->HL * A)); CHK(dalloc(e, &e->sde_E1, (size_t)e->HL * A));
    CHK(dalloc(e, &e->sde_lat2, Bl * e->HL)); CHK(dalloc(e, &e->sde_gsig, Bl * e->Ap)); CHK(dalloc(e, &e->sde_graw, (size_t)e->HL * A));
    CHK(dalloc(e, &e->sde_S2, (size_t)e->HL * A)); CHK(dalloc(e, &e->sde_var, R * e->Ap));
  }
  CHK(dalloc(e, &e->gstate[0], N * kGoalStateFloats)); CHK(dalloc(e, &e->gstate[1], N * kGoalStateFloats));
  CHK(dalloc(e, &e->ep_stats, kEpStatsDoubles));
  CHK(dalloc(e, &e->chunks_dev, e->chunk_table.size()));
  CHK(dalloc(e, &e->chunk_partial, e->chunk_table.size()));
  CHK(fused_init(e));
  return MOBROB_OK;
}

int check_device(const mobrob_ppo_config_t* cfg) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(MOBROB_ERR_NO_DEVICE, "no HIP device visible: libmobrob_ppo has no CPU fallback");
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(MOBROB_ERR_INVALID, "device_id %d out of range (%d devices)", cfg->device_id, ndev);
  HIPC(hipSetDevice(cfg->device_id));
  hipDeviceProp_t prop;
  HIPC(hipGetDeviceProperties(&prop, cfg->device_id));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(MOBROB_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", cfg->device_id, prop.gcnArchName);
  return MOBROB_OK;
}

int engine_create(const mobrob_ppo_config_t* cfg, void* arena, size_t arena_bytes, mobrob_ppo_engine_t** out) {
  CHK(check_cfg(cfg));
  CHK(check_device(cfg));
  auto* e = new mobrob_ppo_engine();
  *out = e;  // so that destroy() can clean up after a partial failure
  e->rollout64_tile_max = env_int("MOBROB_ROLLOUT64_TILE_MAX", e->rollout64_tile_max);  // 0: one-wave kernel only
  e->pair64_min_tiles = env_int("MOBROB_PAIR64_MIN_TILES", e->pair64_min_tiles);  // 0: block kernel for large minibatches
  e->split64_max_tiles = env_int("MOBROB_SPLIT64_MAX_TILES", e->split64_max_tiles);  // 0: block kernel only (A/B, tests)
  e->epoch_kernel_on = env_int("MOBROB_EPOCH_KERNEL", e->epoch_kernel_on) != 0; // 0: three launches per optimizer step, always
  e->gemm_tiles = env_int("MOBROB_GEMM_TILES", e->gemm_tiles); // generic chain: tiles per wave (launch_gemm)
  CHK(engine_dims(e, cfg));
  HIPC(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  e->own_stream = true;
  if (arena) {
    if (reinterpret_cast<uintptr_t>(arena) % kArenaAlign) return fail(MOBROB_ERR_INVALID, "arena must be %zu-byte aligned", kArenaAlign);
    e->arena = static_cast<char*>(arena);
    e->arena_bytes = arena_bytes;
  } else {  // one allocation per engine, sized by the same planning pass callers of create_in_arena use
    size_t need = 0;
    CHK(mobrob_ppo_device_bytes(cfg, &need));
    void* q = nullptr;
    HIPC(hipMalloc(&q, need));
    e->allocs.push_back(q);
    e->arena = static_cast<char*>(q);
    e->arena_bytes = need;
  }
  CHK(engine_alloc(e));
  HIPC(hipMemcpyAsync(e->chunks_dev, e->chunk_table.data(), e->chunk_table.size() * sizeof(NormChunk), hipMemcpyHostToDevice, e->stream));
  // `_last_episode_starts` is all-True at _setup_learn (Appendix A.5)
  std::vector<float> ones(e->N, 1.0f);
  HIPC(hipMemcpyAsync(e->prev_dones, ones.data(), (size_t)e->N * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  repack(e);
  if (e->sde) sde_resample(e, 0, e->N, e->draw_counter++, nullptr, true);   // proba_distribution_net samples the first weights at _build
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}

}  // namespace

extern "C" {

int mobrob_ppo_device_bytes(const mobrob_ppo_config_t* cfg, size_t* bytes) {
  if (!cfg || !bytes) return fail(MOBROB_ERR_INVALID, "null argument");
  CHK(check_cfg(cfg));
  mobrob_ppo_engine plan;  // host-only sizing pass: no device is touched
  plan.plan_only = true;
  CHK(engine_dims(&plan, cfg));
  CHK(engine_alloc(&plan));
  *bytes = plan.arena_used;
  return MOBROB_OK;
}

void* mobrob_ppo_device_alloc(int32_t device_id, size_t bytes) {
  void* p = nullptr;
  if (hipSetDevice(device_id) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) {
    fail(MOBROB_ERR_HIP, "device_alloc(%zu bytes) failed", bytes);
    return nullptr;
  }
  return p;
}
void mobrob_ppo_device_free(void* p) { if (p) (void)hipFree(p); }

int mobrob_ppo_create(const mobrob_ppo_config_t* cfg, mobrob_ppo_engine_t** out) {
  if (!cfg || !out) return fail(MOBROB_ERR_INVALID, "null argument");
  return engine_create(cfg, nullptr, 0, out);
}

int mobrob_ppo_create_in_arena(const mobrob_ppo_config_t* cfg, void* arena, size_t arena_bytes, mobrob_ppo_engine_t** out) {
  if (!cfg || !out || !arena) return fail(MOBROB_ERR_INVALID, "null argument");
  return engine_create(cfg, arena, arena_bytes, out);
}

void mobrob_ppo_destroy(mobrob_ppo_engine_t* e) {
  if (!e) return;
  (void)hipStreamSynchronize(e->stream);
  (void)mobrob_ppo_comm_destroy(e);
  (void)mobrob_ppo_oneshot_close(e);
  prof_resolve(e);
  if (e->cstream) {
    (void)hipStreamSynchronize(e->cstream);
    for (auto& st : e->stage) {
      (void)hipHostFree(st.obs); (void)hipHostFree(st.eps); (void)hipHostFree(st.rew); (void)hipHostFree(st.term);
      (void)hipHostFree(st.dones); (void)hipHostFree(st.trunc);
    }
    (void)hipHostFree(e->o_raw); (void)hipHostFree(e->o_clip); (void)hipHostFree(e->o_val); (void)hipHostFree(e->o_lp);
    (void)hipEventDestroy(e->ev_in); (void)hipEventDestroy(e->ev_k); (void)hipEventDestroy(e->ev_store);
    (void)hipStreamDestroy(e->cstream);
  }
  for (hipEvent_t ev : e->ev_part)
    if (ev) (void)hipEventDestroy(ev);
  if (e->srv_flags) (void)hipHostFree(e->srv_flags);
  if (e->srv_abort) (void)hipFree(e->srv_abort);
  if (e->epoch_stage) (void)hipHostFree(e->epoch_stage);
  if (e->epoch_err_host) (void)hipHostFree(e->epoch_err_host);
  if (e->epoch_ev) (void)hipEventDestroy(e->epoch_ev);
  if (e->ro_exec) (void)hipGraphExecDestroy(e->ro_exec);
  if (e->ro_graph) (void)hipGraphDestroy(e->ro_graph);
  if (e->vstream) {
    (void)hipStreamSynchronize(e->vstream);
    for (auto ev : e->ev_chunks) (void)hipEventDestroy(ev);
    (void)hipEventDestroy(e->ev_vdone);
    (void)hipStreamDestroy(e->vstream);
  }
  for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
  for (void* p : e->allocs) (void)hipFree(p);
  if (e->eval_buf) (void)hipFree(e->eval_buf);
  if (e->plan_fields) (void)hipFree(e->plan_fields);
  if (e->plan_buf) (void)hipFree(e->plan_buf);
  if (e->plan_dil) (void)hipFree(e->plan_dil);
  if (e->plan_clear_fields) (void)hipFree(e->plan_clear_fields);
  if (e->plan_time_buf) (void)hipFree(e->plan_time_buf);
  if (e->plan_team_buf) (void)hipFree(e->plan_team_buf);
  if (e->spec_buf) (void)hipFree(e->spec_buf);
  if (e->plan_spec_buf) (void)hipFree(e->plan_spec_buf);
  if (e->own_stream && e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

int mobrob_ppo_set_stream(mobrob_ppo_engine_t* e, void* s) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  HIPC(hipStreamSynchronize(e->stream));
  if (e->ro_exec) { (void)hipGraphExecDestroy(e->ro_exec); e->ro_exec = nullptr; }
  if (e->ro_graph) { (void)hipGraphDestroy(e->ro_graph); e->ro_graph = nullptr; }
  if (e->own_stream && e->stream) HIPC(hipStreamDestroy(e->stream));
  if (s == nullptr) {
    HIPC(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    e->own_stream = true;
  } else {
    e->stream = static_cast<hipStream_t>(s);
    e->own_stream = false;
  }
  return MOBROB_OK;
}

int mobrob_ppo_synchronize(mobrob_ppo_engine_t* e) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  HIPC(hipStreamSynchronize(e->stream));
  return check_async_error(e);
}

int64_t mobrob_ppo_param_count(const mobrob_ppo_engine_t* e) { return e ? e->P : -1; }

int mobrob_ppo_get_params(mobrob_ppo_engine_t* e, float* out, int64_t n) {
  if (!e || !out || n != e->P) return fail(MOBROB_ERR_INVALID, "get_params: n=%lld, expected %d", (long long)n, e ? e->P : -1);
  HIPC(hipMemcpyAsync(out, e->params, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}
int mobrob_ppo_set_params(mobrob_ppo_engine_t* e, const float* in, int64_t n) {
  if (!e || !in || n != e->P) return fail(MOBROB_ERR_INVALID, "set_params: n=%lld, expected %d", (long long)n, e ? e->P : -1);
  HIPC(hipMemcpyAsync(e->params, in, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  repack(e);
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}
int mobrob_ppo_get_optimizer_state(mobrob_ppo_engine_t* e, float* m, float* v, int64_t n, int64_t* step) {
  if (!e || n != e->P) return fail(MOBROB_ERR_INVALID, "get_optimizer_state: bad size");
  if (m) HIPC(hipMemcpyAsync(m, e->m, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  if (v) HIPC(hipMemcpyAsync(v, e->v, (size_t)n * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  if (step) *step = e->adam_step;
  return MOBROB_OK;
}
int mobrob_ppo_set_optimizer_state(mobrob_ppo_engine_t* e, const float* m, const float* v, int64_t n, int64_t step) {
  if (!e || !m || !v || n != e->P || step < 0) return fail(MOBROB_ERR_INVALID, "set_optimizer_state: bad argument");
  HIPC(hipMemcpyAsync(e->m, m, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(e->v, v, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  e->adam_step = step;
  return MOBROB_OK;
}

// ---- rollout ---------------------------------------------------------------------------------------
int mobrob_ppo_rollout_begin(mobrob_ppo_engine_t* e) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  e->t = 0;
  e->rollout_ready = false; e->train_rec_valid = false;
  e->nparts = 0;
  for (auto& q : e->pinned_seen) q = nullptr;
  e->pinned_seen_n = 0;
  e->draw_ro0 = e->draw_counter;
  for (int p = 0; p < MOBROB_MAX_PARTS; ++p) {
    e->part_act_t[p] = e->part_store_t[p] = 0;
    e->part_obs_t[p] = -1;
  }
  return MOBROB_OK;
}

int mobrob_ppo_act(mobrob_ppo_engine_t* e, const float* obs, const float* eps, float* a_raw, float* a_clip,
                   float* values, float* logp) {
  if (!e || !obs) return fail(MOBROB_ERR_INVALID, "act: null argument");
  if (e->t >= e->T) return fail(MOBROB_ERR_STATE, "act: rollout buffer full (t=%d, n_steps=%d)", e->t, e->T);
  CHK(streamer_init(e));
  const size_t N = e->N, A = e->A, D = e->D;
  // Pinned fast path: every buffer of the call is hipHostMalloc memory -> the GPU reads / writes it in place
  // (k_pull_rows, k_copy_f32) on the compute stream; one stream, no events, one synchronisation.
  if (!eps && is_pinned(obs) && (!a_raw || is_pinned(a_raw)) && (!a_clip || is_pinned(a_clip)) &&
      (!values || is_pinned(values)) && (!logp || is_pinned(logp))) {
    hipLaunchKernelGGL(k_pull_rows, dim3(cdiv((int)(N * e->Dp), 256)), dim3(256), 0, e->stream, obs,
                       e->obs + (size_t)e->t * N * e->Dp, (int)N, (int)D, e->Dp);
    act_slot(e, e->t, nullptr);
    auto push = [&](const float* dev, float* host, size_t n) {
      if (host) hipLaunchKernelGGL(k_copy_f32, dim3(cdiv((int)n, 256)), dim3(256), 0, e->stream, dev, host, (int)n);
    };
    push(e->clip_act, a_clip, N * A);
    push(e->actions + (size_t)e->t * N * A, a_raw, N * A);
    push(e->values + (size_t)e->t * N, values, N);
    push(e->logp + (size_t)e->t * N, logp, N);
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(e->stream));
    return MOBROB_OK;
  }
  auto& st = e->stage[e->stage_i];
  // H2D on the side stream (pinned source -> truly asynchronous), compute stream waits on the event
  const float* src = stage_in(obs, st.obs, N * D);
  CHK(upload_obs_on(e, e->cstream, src, e->obs + (size_t)e->t * N * e->Dp, e->N));
  if (eps) {
    const float* es = stage_in(eps, st.eps, N * A);
    HIPC(hipMemcpyAsync(e->eps_dev, es, N * A * 4, hipMemcpyHostToDevice, e->cstream));
  }
  HIPC(hipEventRecord(e->ev_in, e->cstream));
  HIPC(hipStreamWaitEvent(e->stream, e->ev_in, 0));
  act_slot(e, e->t, eps ? e->eps_dev : nullptr);
  HIPC(hipEventRecord(e->ev_k, e->stream));
  HIPC(hipStreamWaitEvent(e->cstream, e->ev_k, 0));
  // D2H of the requested outputs: straight into pinned user buffers, else through pinned staging
  struct Out { float* user; float* stagebuf; const float* dev; size_t n; };
  const Out outs[4] = {{a_clip, e->o_clip, e->clip_act, N * A},
                       {a_raw, e->o_raw, e->actions + (size_t)e->t * N * A, N * A},
                       {values, e->o_val, e->values + (size_t)e->t * N, N},
                       {logp, e->o_lp, e->logp + (size_t)e->t * N, N}};
  bool staged[4] = {false, false, false, false};
  for (int i = 0; i < 4; ++i) {
    if (!outs[i].user) continue;
    staged[i] = !is_pinned(outs[i].user);
    HIPC(hipMemcpyAsync(staged[i] ? outs[i].stagebuf : outs[i].user, outs[i].dev, outs[i].n * 4, hipMemcpyDeviceToHost,
                        e->cstream));
  }
  HIPC(hipStreamSynchronize(e->cstream));
  for (int i = 0; i < 4; ++i)
    if (outs[i].user && staged[i]) memcpy(outs[i].user, outs[i].stagebuf, outs[i].n * 4);
  return MOBROB_OK;
}

namespace {
// does any of the rows [r0, r0 + n) end in a time-limit truncation the caller sent the terminal observation of?
bool any_truncated(const uint8_t* truncated, const float* terminal_obs, int r0, int n) {
  bool any = false;
  if (truncated && terminal_obs)
    for (int i = r0; i < r0 + n; ++i) any |= truncated[i] != 0;
  return any;
}
// rollout_buffer.add of step e->t on the compute stream: V(terminal_obs) of the truncated rows (term_obs / trunc_dev already hold
// them), rewards (+ bootstrap) and episode starts into the slot, then the step's dones become the next step's episode starts.
// rew / dones: device-readable -- the caller's pinned buffers, or rew_tmp / dones_u8
void store_step(mobrob_ppo_engine* e, const float* rew, const uint8_t* dones, bool any_trunc) {
  const size_t o = (size_t)e->t * e->N;
  if (any_trunc) value_flagged(e, e->term_obs, e->trunc_dev, e->term_val);
  hipLaunchKernelGGL(k_store_step, dim3(cdiv(e->N, 256)), dim3(256), 0, e->stream, rew, e->prev_dones,
                     any_trunc ? e->trunc_dev : nullptr, e->term_val, (float)e->cfg.gamma, e->N, e->rewards + o, e->es + o);
  hipLaunchKernelGGL(k_u8_to_f32, dim3(cdiv(e->N, 256)), dim3(256), 0, e->stream, dones, e->prev_dones, e->N);
}
}  // namespace

int mobrob_ppo_store(mobrob_ppo_engine_t* e, const float* rewards, const uint8_t* dones, const uint8_t* truncated,
                     const float* terminal_obs) {
  if (!e || !rewards || !dones) return fail(MOBROB_ERR_INVALID, "store: null argument");
  if (e->t >= e->T) return fail(MOBROB_ERR_STATE, "store: rollout buffer full");
  CHK(streamer_init(e));
  const size_t N = e->N, D = e->D;
  const bool any_trunc = any_truncated(truncated, terminal_obs, 0, e->N);
  if (is_pinned(rewards) && is_pinned(dones) && (!truncated || is_pinned(truncated)) &&
      (!terminal_obs || is_pinned(terminal_obs))) {
    // Pinned fast path: the kernels read the caller's buffers in place.  The caller may overwrite them only after
    // the next act() has returned (act synchronises the compute stream) -- the order every rollout loop has.
    if (any_trunc) {
      hipLaunchKernelGGL(k_pull_rows, dim3(cdiv((int)(N * e->Dp), 256)), dim3(256), 0, e->stream, terminal_obs, e->term_obs,
                         (int)N, (int)D, e->Dp);
      HIPC(hipMemcpyAsync(e->trunc_dev, truncated, N, hipMemcpyHostToDevice, e->stream));
    }
    store_step(e, rewards, dones, any_trunc);
    HIPC(hipGetLastError());
    e->t++;
    return MOBROB_OK;
  }
  auto& st = e->stage[e->stage_i];
  // Fully asynchronous: the scalars are staged in pinned memory (the caller may reuse its buffers immediately),
  // copied on the side stream and consumed by the compute stream behind an event; nothing here waits for the GPU.
  // The staging slot is reused two steps later, after act() of the next step has synchronised the side stream.
  memcpy(st.rew, rewards, N * 4);
  memcpy(st.dones, dones, N);
  HIPC(hipMemcpyAsync(e->rew_tmp, st.rew, N * 4, hipMemcpyHostToDevice, e->cstream));
  HIPC(hipMemcpyAsync(e->dones_u8, st.dones, N, hipMemcpyHostToDevice, e->cstream));
  if (any_trunc) {
    memcpy(st.trunc, truncated, N);
    memcpy(st.term, terminal_obs, N * D * 4);
    HIPC(hipMemcpyAsync(e->trunc_dev, st.trunc, N, hipMemcpyHostToDevice, e->cstream));
    CHK(upload_obs_on(e, e->cstream, st.term, e->term_obs, e->N));
  }
  HIPC(hipEventRecord(e->ev_store, e->cstream));
  HIPC(hipStreamWaitEvent(e->stream, e->ev_store, 0));
  store_step(e, e->rew_tmp, e->dones_u8, any_trunc);
  // the next step's H2D of rew_tmp/dones_u8 must not overtake these kernels
  HIPC(hipEventRecord(e->ev_k, e->stream));
  HIPC(hipStreamWaitEvent(e->cstream, e->ev_k, 0));
  HIPC(hipGetLastError());
  e->stage_i ^= 1;
  e->t++;
  return MOBROB_OK;
}

// ---- pipelined host-env rollout: the same arithmetic as act()/store(), one contiguous row range at a time ----
namespace {
int part_range(mobrob_ppo_engine* e, int part, int nparts, int* r0, int* n) {
  if (nparts < 1 || nparts > MOBROB_MAX_PARTS || nparts > e->N || part < 0 || part >= nparts)
    return fail(MOBROB_ERR_INVALID, "part %d of %d (1..%d parts, at most one per env)", part, nparts, MOBROB_MAX_PARTS);
  if (e->nparts == 0) e->nparts = nparts;
  if (e->nparts != nparts) return fail(MOBROB_ERR_STATE, "nparts changed from %d to %d inside a rollout", e->nparts, nparts);
  *r0 = (int)((int64_t)e->N * part / nparts);
  *n = (int)((int64_t)e->N * (part + 1) / nparts) - *r0;
  return MOBROB_OK;
}
}  // namespace

int mobrob_ppo_act_part(mobrob_ppo_engine_t* e, int32_t part, int32_t nparts, const float* obs, float* a_clip) {
  if (!e || !obs || !a_clip) return fail(MOBROB_ERR_INVALID, "act_part: null argument");
  int r0, n;
  CHK(part_range(e, part, nparts, &r0, &n));
  const int t = e->part_act_t[part];
  if (t >= e->T) return fail(MOBROB_ERR_STATE, "act_part: rollout buffer full (part %d, t=%d)", part, t);
  if (t != e->part_store_t[part]) return fail(MOBROB_ERR_STATE, "act_part: part %d acted on step %d but has not stored it", part, t - 1);
  if (!is_pinned_cached(e, obs) || !is_pinned_cached(e, a_clip))
    return fail(MOBROB_ERR_INVALID, "act_part needs device-visible pinned buffers (mobrob_ppo_host_alloc)");
  if (!e->ev_part[part]) HIPC(hipEventCreateWithFlags(&e->ev_part[part], hipEventDisableTiming));
  const size_t D = e->D, A = e->A;
  if (e->part_obs_t[part] != t)  // not already pulled by the preceding store_part(next_obs)
    hipLaunchKernelGGL(k_pull_rows, dim3(cdiv(n * e->Dp, 256)), dim3(256), 0, e->stream, obs + (size_t)r0 * D,
                       e->obs + ((size_t)t * e->N + r0) * e->Dp, n, (int)D, e->Dp);
  act_rows(e, t, r0, n, nullptr, e->draw_ro0 + (uint32_t)t, nullptr, a_clip + (size_t)r0 * A);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(e->ev_part[part], e->stream));
  e->part_act_t[part] = t + 1;
  if (e->draw_counter < e->draw_ro0 + (uint32_t)t + 1) e->draw_counter = e->draw_ro0 + (uint32_t)t + 1;
  return MOBROB_OK;
}

int mobrob_ppo_wait_part(mobrob_ppo_engine_t* e, int32_t part) {
  if (!e || part < 0 || part >= MOBROB_MAX_PARTS || !e->ev_part[part])
    return fail(MOBROB_ERR_STATE, "wait_part: part %d has no act_part in flight", part);
  HIPC(hipEventSynchronize(e->ev_part[part]));
  return MOBROB_OK;
}

int mobrob_ppo_store_part(mobrob_ppo_engine_t* e, int32_t part, int32_t nparts, const float* rewards,
                          const uint8_t* dones, const uint8_t* truncated, const float* terminal_obs,
                          const float* next_obs) {
  if (!e || !rewards || !dones) return fail(MOBROB_ERR_INVALID, "store_part: null argument");
  int r0, n;
  CHK(part_range(e, part, nparts, &r0, &n));
  const int t = e->part_store_t[part];
  if (t + 1 != e->part_act_t[part]) return fail(MOBROB_ERR_STATE, "store_part: part %d has no acted step to store (t=%d)", part, t);
  if (!is_pinned_cached(e, rewards) || !is_pinned_cached(e, dones) || (truncated && !is_pinned_cached(e, truncated)) ||
      (terminal_obs && !is_pinned_cached(e, terminal_obs)) || (next_obs && !is_pinned_cached(e, next_obs)))
    return fail(MOBROB_ERR_INVALID, "store_part needs device-visible pinned buffers (mobrob_ppo_host_alloc)");
  const bool any = any_truncated(truncated, terminal_obs, r0, n);
  const size_t o = (size_t)t * e->N + r0;
  StorePullArgs a{};
  a.rew_in = rewards + r0; a.dones = dones + r0;
  a.trunc = any ? truncated + r0 : nullptr; a.term_obs = any ? terminal_obs + (size_t)r0 * e->D : nullptr;
  a.vn = value_net_args(e);
  a.D = e->D; a.Dp = e->Dp; a.n = n; a.gamma = (float)e->cfg.gamma;
  a.prev_dones = e->prev_dones + r0; a.rew_out = e->rewards + o; a.es_out = e->es + o; a.term_val = e->term_val + r0;
  if (next_obs) {  // slot t+1 exists for every t < T (slot T holds the last observations)
    a.next_obs = next_obs + (size_t)r0 * e->D;
    a.obs_slot = e->obs + ((size_t)(t + 1) * e->N + r0) * e->Dp;
    e->part_obs_t[part] = t + 1;
  }
  const size_t sm = (size_t)(e->D + value_net_width_sum(e) + 32) * sizeof(float);
  hipLaunchKernelGGL(k_store_pull_part, dim3(cdiv(n, kPartRows)), dim3(256), sm, e->stream, a);
  HIPC(hipGetLastError());
  e->part_store_t[part] = t + 1;
  int tmin = e->T;
  for (int p = 0; p < nparts; ++p) tmin = std::min(tmin, e->part_store_t[p]);
  e->t = tmin;
  return MOBROB_OK;
}

int mobrob_ppo_finish_rollout(mobrob_ppo_engine_t* e, const float* last_obs, const uint8_t* dones) {
  if (!e || !last_obs || !dones) return fail(MOBROB_ERR_INVALID, "finish_rollout: null argument");
  if (e->t != e->T) return fail(MOBROB_ERR_STATE, "finish_rollout: %d of %d steps stored", e->t, e->T);
  CHK(streamer_init(e));
  const size_t N = e->N;
  auto& st = e->stage[e->stage_i];
  float* slot = e->obs + (size_t)e->T * N * e->Dp;
  const float* src = stage_in(last_obs, st.obs, N * e->D);
  CHK(upload_obs_on(e, e->cstream, src, slot, e->N));
  memcpy(st.dones, dones, N);
  HIPC(hipMemcpyAsync(e->dones_u8, st.dones, N, hipMemcpyHostToDevice, e->cstream));
  HIPC(hipEventRecord(e->ev_in, e->cstream));
  HIPC(hipStreamWaitEvent(e->stream, e->ev_in, 0));
  hipLaunchKernelGGL(k_u8_to_f32, dim3(cdiv(e->N, 256)), dim3(256), 0, e->stream, e->dones_u8, e->last_dones, e->N);
  forward(e, slot, e->N, false, nullptr, true, e->last_values);
  run_gae(e);
  HIPC(hipStreamSynchronize(e->stream));
  e->rollout_ready = true; e->train_rec_valid = false;
  return MOBROB_OK;
}

int mobrob_ppo_compute_gae(mobrob_ppo_engine_t* e) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  run_gae(e);
  HIPC(hipStreamSynchronize(e->stream));
  e->rollout_ready = true; e->train_rec_valid = false;
  return MOBROB_OK;
}

int mobrob_ppo_x3_mode(const mobrob_ppo_engine_t* e) {
  if (!e || !e->fused.enabled || e->fused.net[0].W2x == nullptr) return 0;
  return 1 | (e->fused.train_x3 ? 2 : 0) | (e->fused.train_x3 && e->fused.train_chain ? 4 : 0);
}

int mobrob_ppo_update_mode(const mobrob_ppo_engine_t* e) { return e ? e->last_update_mode : 0; }

int mobrob_ppo_set_eval_tile256(mobrob_ppo_engine_t* e, int32_t on) {
  if (!e) return fail(MOBROB_ERR_INVALID, "set_eval_tile256: null engine");
  if (!(e->fused.enabled && e->fused.H == FH))
    return fail(MOBROB_ERR_INVALID, "set_eval_tile256: the tile256 kernel serves fused 2x256 tanh engines only (this one: %s)",
                e->fused.enabled ? "fused 2x64" : "not of the fused family");
  e->eval_tile256 = on != 0;
  return MOBROB_OK;
}

int mobrob_ppo_set_eval_tile256_wide(mobrob_ppo_engine_t* e, int32_t on) {
  if (!e) return fail(MOBROB_ERR_INVALID, "set_eval_tile256_wide: null engine");
  if (!(e->fused.enabled && e->fused.H == FH))
    return fail(MOBROB_ERR_INVALID, "set_eval_tile256_wide: the tile256 kernel serves fused 2x256 tanh engines only (this one: %s)",
                e->fused.enabled ? "fused 2x64" : "not of the fused family");
  e->eval_tile256_wide = on != 0;
  return MOBROB_OK;
}

int mobrob_ppo_explained_variance(mobrob_ppo_engine_t* e, double* out) {
  if (!e || !out) return fail(MOBROB_ERR_INVALID, "explained_variance: null argument");
  if (!e->rollout_ready) return fail(MOBROB_ERR_STATE, "explained_variance: rollout not finished");
  const int n = e->N * e->T;
  hipLaunchKernelGGL(k_explained_variance_partials, dim3(kEvBlocks), dim3(256), 0, e->stream, e->values, e->ret, n, e->expvar_part);
  double part[kEvBlocks * 4];
  HIPC(hipMemcpyAsync(part, e->expvar_part, sizeof part, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < kEvBlocks; ++b)
    for (int k = 0; k < 4; ++k) s[k] += part[b * 4 + k];
  const double var_y = s[1] / n - (s[0] / n) * (s[0] / n), var_d = s[3] / n - (s[2] / n) * (s[2] / n);
  *out = var_y > 0.0 ? 1.0 - var_d / var_y : NAN;  // SB3: nan when the returns do not vary
  return MOBROB_OK;
}

int mobrob_ppo_mark_rollout_ready(mobrob_ppo_engine_t* e) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  e->rollout_ready = true; e->train_rec_valid = false;
  e->t = e->T;
  return MOBROB_OK;
}

namespace {
// enqueue one whole device-resident rollout (T steps + last values + GAE) on the engine stream
uint64_t env_seed_of(const mobrob_ppo_engine* e) {
  return e->cfg.seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(e->cfg.rank + 1));
}

// One persistent launch for all T steps (policy forward + sample + env + store), then the value network over all
// stored observations in one batched pass, then GAE (kernels_rollout.h).
bool rollout_persistent_ok(const mobrob_ppo_engine* e) {
  return e->cfg.rollout_persistent && e->fused.enabled;  // both fused widths (256: kernels_rollout.h top, 64: bottom)
}
// side stream and events of the overlapped value pass: created OUTSIDE any stream capture (resource creation is
// not a capturable operation)
int rollout_side_stream_init(mobrob_ppo_engine* e) {
  if (!e->vstream) {
    HIPC(hipStreamCreateWithFlags(&e->vstream, hipStreamNonBlocking));
    HIPC(hipEventCreateWithFlags(&e->ev_vdone, hipEventDisableTiming));
  }
  while ((int)e->ev_chunks.size() < e->T / 16 + 2) {  // chunks are >= 16 steps
    hipEvent_t ev;
    HIPC(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    e->ev_chunks.push_back(ev);
  }
  return MOBROB_OK;
}

// ---- the persistent rollout kernels in chunks: device rollouts and the served host rollout (collect_host_served) ----
// What a device rollout and a served one pass the kernel alike: the policy's packs, the sampling constants, the value network of
// the time-limit bootstrap, the dims and every arena pointer.  The caller adds its kind, counters and environment.
RolloutArgs rollout_args(mobrob_ppo_engine* e) {
  RolloutArgs a{};
  a.pi = e->fused.net[0];
  a.log_std = Pp(e, T_LOGSTD); a.seed = eps_seed(e);
  a.lo = (float)e->cfg.action_low; a.hi = (float)e->cfg.action_high;
  a.bt = BootArgs{Pp(e, T_VW1), Pp(e, T_VB1), Pp(e, T_VW2), Pp(e, T_VB2), Pp(e, T_VW), Pp(e, T_VB), e->G1, e->G2,
                  (float)e->cfg.gamma, e->term_val};  // (fused path: two tanh layers)
  a.N = e->N; a.D = e->D; a.A = e->A;
  a.obs = e->obs; a.actions = e->actions; a.logp = e->logp; a.rewards = e->rewards; a.es = e->es;
  a.term_obs = e->term_obs; a.trunc = e->trunc_dev; a.clip_act = e->clip_act;
  a.ep_len = e->ep_len; a.prev_dones = e->prev_dones; a.gstate = e->gstate[0]; a.ep_stats = e->ep_stats;
  return a;
}

bool wide_nets(const mobrob_ppo_engine* e) { return e->fused.H == FH; }  // of a fused engine: 256-wide, else 64-wide
// 64-wide: one workgroup per 32-env tile (k_rollout64_tile) while every tile gets a CU of its own, else the one-wave kernel
bool rollout64_tile_kernel(const mobrob_ppo_engine* e) { return cdiv(e->N, 32) <= e->rollout64_tile_max; }
// x3 engines: the eight-wave form with W2's leading pieces stationary in registers (kernels_rollout.h, S8);
// MOBROB_ROLLOUT_S8=0 keeps the four-wave form (A/B and the bit-equality test of the two)
bool rollout_s8(const mobrob_ppo_engine* e) {
  static const bool s8_on = !kRolloutStationary && env_int("MOBROB_ROLLOUT_S8", 1) != 0;
  return s8_on && e->fused.net[0].W2x != nullptr;
}

// A rollout of <= 192 tiles (32 envs each, one workgroup, ~100 KB of LDS at 256 wide) leaves CUs idle for thousands of dependent
// steps: it is cut into chunks, and the observations of a finished chunk are valued on the side stream, behind an event, while the
// next chunk rolls out.  64-wide: the tile kernel only, and only when the value pass is more than a few launches' worth of work.
// vgrid_max: workgroups of a side-stream value pass (256-wide), what the rollout leaves free.
struct ChunkPlan {
  bool overlap;
  int chunk, vgrid_max;
};
ChunkPlan chunk_plan(bool wide, int tiles, bool tile_kernel, int T, int N) {
  const bool overlap = tiles <= 192 && (wide || (tile_kernel && (size_t)T * N >= ((size_t)1 << 18)));  // otherwise the rollout itself fills the device
  return ChunkPlan{overlap, overlap ? std::max(16, cdiv(T, 20)) : T, overlap ? std::max(32, 256 - tiles) : 256};
}

// steps [a.t0, a.t1) of the rollout on the compute stream: the one place that picks the kernel
void launch_rollout_kernel(mobrob_ppo_engine* e, const RolloutArgs& a) {
  const int Dp = e->Dp, tiles = cdiv(a.N, 32);
  if (!wide_nets(e)) {  // 64-wide nets (kernels_rollout.h, bottom half)
    if (a.kind == 3) {  // (served: within the tile kernel's range, collect_host_served)
      FUSED_DISPATCH_DP(Dp, hipLaunchKernelGGL((k_rollout64_tile<DPc, 3>), dim3(tiles), dim3(256), rollout64_tile_lds_bytes(Dp, true), e->stream, a));
    } else if (rollout64_tile_kernel(e)) {
      FUSED_DISPATCH_DP(Dp, hipLaunchKernelGGL((k_rollout64_tile<DPc>), dim3(tiles), dim3(256), rollout64_tile_lds_bytes(Dp), e->stream, a));
    } else {
      const int nwv = rollout64_waves(Dp);
      FUSED_DISPATCH_DP(Dp, hipLaunchKernelGGL((k_rollout64_persistent<DPc>), dim3(cdiv(tiles, nwv)), dim3(nwv * 64), rollout64_lds_bytes(Dp), e->stream, a));
    }
    return;
  }
  const bool s8 = a.kind == 3 || rollout_s8(e);  // (served: eight-wave x3 engines only, collect_host_served)
  const dim3 grid(tiles), block(kRolloutThreads);
  const size_t lds = rollout_lds_bytes(Dp, s8);
  if (a.kind == 3) {
    FUSED_DISPATCH_DP(Dp, hipLaunchKernelGGL((k_rollout_persistent<DPc, 3, true>), grid, block, lds, e->stream, a));
  } else if (s8 && a.kind == 1) {
    FUSED_DISPATCH_DP(Dp, hipLaunchKernelGGL((k_rollout_persistent<DPc, 1, true>), grid, block, lds, e->stream, a));
  } else if (s8) {
    FUSED_DISPATCH_DP(Dp, hipLaunchKernelGGL((k_rollout_persistent<DPc, 2, true>), grid, block, lds, e->stream, a));
  } else if (a.kind == 1) {
    FUSED_DISPATCH_DP(Dp, hipLaunchKernelGGL((k_rollout_persistent<DPc, 1>), grid, block, lds, e->stream, a));
  } else {
    FUSED_DISPATCH_DP(Dp, hipLaunchKernelGGL((k_rollout_persistent<DPc, 2>), grid, block, lds, e->stream, a));
  }
}

// V of the stored observation rows [r0, r1) into values[r0, r1) on stream `st`; grid_max caps the 256-wide kernel's workgroups
void value_rows(mobrob_ppo_engine* e, hipStream_t st, int r0, int r1, int grid_max) {
  const int Dp = e->Dp;
  if (!wide_nets(e)) {
    fused_forward(e->fused, e->obs + (size_t)r0 * Dp, r1 - r0, false, nullptr, e->Ap, true, e->values + r0, st);
    return;
  }
  FUSED_DISPATCH_DP(Dp, hipLaunchKernelGGL((k_value_batch<DPc>), dim3(std::min(grid_max, cdiv(r1 - r0, FR))), dim3(FTHREADS),
                                           e->fused.lds_bytes, st, e->fused.net[1], e->obs + (size_t)r0 * Dp, r1 - r0, e->values + r0));
}

// The T steps as chunks of the plan on the compute stream; V of every chunk but the last on the side stream (chunk_plan).
int enqueue_rollout_chunks(mobrob_ppo_engine* e, RolloutArgs& a, const ChunkPlan& pl) {
  const int N = e->N, T = e->T;
  ProfScope ps(e, MOBROB_K_ENV);
  for (int t0 = 0; t0 < T; t0 += pl.chunk) {
    a.t0 = t0; a.t1 = std::min(T, t0 + pl.chunk);
    launch_rollout_kernel(e, a);
    if (pl.overlap && a.t1 < T) {  // observations [t0, t1) are final: value them on the side stream
      hipEvent_t ev = e->ev_chunks[t0 / pl.chunk];
      HIPC(hipEventRecord(ev, e->stream));
      HIPC(hipStreamWaitEvent(e->vstream, ev, 0));
      value_rows(e, e->vstream, t0 * N, a.t1 * N, pl.vgrid_max);
    }
  }
  return MOBROB_OK;
}
// ... and V of what the side stream did not take, rows up to rows_end, on the compute stream (the rollout is over: the whole
// device), which then waits for the side stream.  rows_end: (T + 1) N for a device rollout (obs[T] is the last observation and
// values[T N ..] = last_values), T N for a served one (V(last_obs) is finish_rollout's).
int value_rollout_tail(mobrob_ppo_engine* e, const ChunkPlan& pl, int rows_end) {
  ProfScope ps(e, MOBROB_K_ACT);
  const int done_rows = pl.overlap ? ((e->T - 1) / pl.chunk) * pl.chunk * e->N : 0;
  value_rows(e, e->stream, done_rows, rows_end, 256);
  if (pl.overlap && done_rows > 0) {  // join the side stream before GAE
    HIPC(hipEventRecord(e->ev_vdone, e->vstream));
    HIPC(hipStreamWaitEvent(e->stream, e->ev_vdone, 0));
  }
  return MOBROB_OK;
}

// Behind the last step of a device rollout: the device-resident counters move on by the T steps taken, and the dones the last
// step left are the rollout's last_dones.  (What follows -- V(last_obs), then run_gae -- differs per caller and keeps its place
// in the launch order.)
int end_device_steps(mobrob_ppo_engine* e) {
  hipLaunchKernelGGL(k_add_counters, dim3(1), dim3(64), 0, e->stream, e->ctr_dev, (uint32_t)e->T, (uint32_t)e->T);
  HIPC(hipMemcpyAsync(e->last_dones, e->prev_dones, (size_t)e->N * 4, hipMemcpyDeviceToDevice, e->stream));
  return MOBROB_OK;
}

int enqueue_rollout_persistent(mobrob_ppo_engine* e, const mobrob_ppo_engine::RolloutSpec& sp) {
  const int N = e->N, T = e->T;
  const size_t slot = (size_t)N * e->Dp;
  HIPC(hipMemcpyAsync(e->obs, e->obs + (size_t)T * slot, slot * 4, hipMemcpyDeviceToDevice, e->stream));
  if (wide_nets(e) && !e->fused.train_x3) pack_x3_all(e);  // otherwise every optimizer step (apply_adam) and set_params keep the x3 packs current
  RolloutArgs a = rollout_args(e);
  a.kind = sp.kind; a.env_seed = env_seed_of(e); a.draw_base = e->ctr_dev; a.step_base = e->ctr_dev + 1;
  a.p_term = sp.p_term; a.time_limit = sp.time_limit; a.goal = sp.goal;
  const ChunkPlan pl = chunk_plan(wide_nets(e), cdiv(N, 32), rollout64_tile_kernel(e), T, N);
  CHK(enqueue_rollout_chunks(e, a, pl));
  CHK(end_device_steps(e));
  CHK(value_rollout_tail(e, pl, (T + 1) * N));
  run_gae(e);
  return MOBROB_OK;
}

int enqueue_rollout(mobrob_ppo_engine* e, const mobrob_ppo_engine::RolloutSpec& sp) {
  if (rollout_persistent_ok(e)) return enqueue_rollout_persistent(e, sp);
  const int N = e->N, Dp = e->Dp, per = Dp / 4;
  const size_t slot = (size_t)N * Dp;
  const uint64_t env_seed = env_seed_of(e);
  // the previous rollout's last observation is this rollout's first
  HIPC(hipMemcpyAsync(e->obs, e->obs + (size_t)e->T * slot, slot * 4, hipMemcpyDeviceToDevice, e->stream));
  const BootNetArgs bt = boot_args(e);
  const size_t sm = env_step_lds_bytes(Dp, value_net_width_sum(e));
  for (int t = 0; t < e->T; ++t) {
    act_slot(e, t, nullptr, true);
    {
      ProfScope ps(e, MOBROB_K_ENV);
      // env step + rollout_buffer.add scalars + time-limit bootstrap of the (rare) truncated rows in one launch
      if (sp.kind == 1) {
        hipLaunchKernelGGL(k_env_step_store, dim3(cdiv(N * per, 256)), dim3(256), sm, e->stream, env_seed, (uint32_t)t,
                           e->ctr_dev + 1, N, e->D, Dp, sp.p_term, sp.time_limit, e->ep_len, e->ep_len2,
                           e->obs + (size_t)(t + 1) * slot, e->term_obs, e->prev_dones, e->dones_tmp, e->trunc_dev,
                           e->rewards + (size_t)t * N, e->es + (size_t)t * N, bt);
        std::swap(e->ep_len, e->ep_len2);
      } else {
        GoalEnvArgs g{};
        g.seed = env_seed; g.step_rel = (uint32_t)t; g.step_base = e->ctr_dev + 1;
        g.N = N; g.D = e->D; g.Dp = Dp; g.A = e->A; g.p = sp.goal;
        g.act = e->clip_act; g.st_in = e->gstate[0]; g.st_out = e->gstate[1];
        g.obs_next = e->obs + (size_t)(t + 1) * slot; g.term_obs = e->term_obs;
        g.prev_dones = e->prev_dones; g.next_dones = e->dones_tmp; g.trunc = e->trunc_dev;
        g.rew_out = e->rewards + (size_t)t * N; g.es_out = e->es + (size_t)t * N; g.ep_stats = e->ep_stats;
        hipLaunchKernelGGL(k_goal_env_step_store, dim3(cdiv(N * per, 256)), dim3(256), sm, e->stream, g, bt);
        std::swap(e->gstate[0], e->gstate[1]);
      }
    }
    std::swap(e->prev_dones, e->dones_tmp);
  }
  CHK(end_device_steps(e));
  forward(e, e->obs + (size_t)e->T * slot, N, false, nullptr, true, e->last_values);
  run_gae(e);
  return MOBROB_OK;
}

// device-resident rollout of either env kind: (re)start the env if needed, then replay / enqueue the T-step loop
int collect_device(mobrob_ppo_engine* e, const mobrob_ppo_engine::RolloutSpec& sp) {
  const int N = e->N, Dp = e->Dp, per = Dp / 4;
  const size_t slot = (size_t)N * Dp;
  if (e->env_started != sp.kind) {
    float* last = e->obs + (size_t)e->T * slot;  // reset writes the "previous last observation"
    if (sp.kind == 1) {
      hipLaunchKernelGGL(k_env_reset, dim3(cdiv(N * per, 256)), dim3(256), 0, e->stream, env_seed_of(e), N, e->D, Dp, last,
                         e->ep_len);
    } else {
      hipLaunchKernelGGL(k_goal_env_reset, dim3(cdiv(N * per, 256)), dim3(256), 0, e->stream, env_seed_of(e), N, e->D, Dp,
                         sp.goal, e->gstate[0], last);
      HIPC(hipMemsetAsync(e->ep_stats, 0, kEpStatsDoubles * sizeof(double), e->stream));
      e->ep_ring_read = 0;
    }
    std::vector<float> ones(N, 1.0f);  // a fresh env starts every episode: `_last_episode_starts` all True
    HIPC(hipMemcpyAsync(e->prev_dones, ones.data(), (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
    HIPC(hipStreamSynchronize(e->stream));
    e->env_started = sp.kind;
  }
  e->rollout_ready = false; e->train_rec_valid = false;
  if (rollout_persistent_ok(e)) CHK(rollout_side_stream_init(e));
  // Graph replay: every kernel argument of the T-step loop is fixed (slot pointers, ping-pong buffers with even T,
  // counters relative to device-resident bases), so the loop is captured once and replayed per rollout.
  // The persistent path is ~45 launches on two streams: enqueued eagerly (the launches hide behind the 18 ms of
  // GPU work; a captured multi-stream graph was both slower to launch and, after many capture / destroy cycles in
  // one process, crashed inside the runtime).  Only the per-step path (thousands of launches) is replayed as a graph.
  bool use_graph = e->cfg.rollout_graph && e->T % 2 == 0 && !rollout_persistent_ok(e);
  if (use_graph && (e->ro_exec == nullptr || memcmp(&e->ro_spec, &sp, sizeof sp) != 0)) {
    HIPC(hipStreamSynchronize(e->stream));  // never destroy an executable graph that may still be running
    if (e->ro_exec) { (void)hipGraphExecDestroy(e->ro_exec); e->ro_exec = nullptr; }
    if (e->ro_graph) { (void)hipGraphDestroy(e->ro_graph); e->ro_graph = nullptr; }
    const bool prof = e->prof_on;
    e->prof_on = false;  // event records cannot be part of the captured graph
    hipError_t be = hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal);
    if (be != hipSuccess) {  // e.g. a stream that does not support capture: run eagerly from now on
      (void)hipGetLastError();
      e->prof_on = prof;
      e->cfg.rollout_graph = 0;
      use_graph = false;
    } else {
      const int rc = enqueue_rollout(e, sp);
      hipError_t ce = hipStreamEndCapture(e->stream, &e->ro_graph);
      e->prof_on = prof;
      if (rc != MOBROB_OK) return rc;
      if (ce != hipSuccess) return fail(MOBROB_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(ce));
      HIPC(hipGraphInstantiate(&e->ro_exec, e->ro_graph, nullptr, nullptr, 0));
      memcpy(&e->ro_spec, &sp, sizeof sp);
    }
  }
  if (!use_graph) {
    CHK(enqueue_rollout(e, sp));
  } else {
    ProfScope ps(e, MOBROB_K_ACT);  // with graph replay the ACT scope covers the whole rollout (forward+env+GAE)
    HIPC(hipGraphLaunch(e->ro_exec, e->stream));
  }
  HIPC(hipGetLastError());
  e->t = e->T;
  e->rollout_ready = true; e->train_rec_valid = false;
  return MOBROB_OK;
}

// Host environments SERVED by the persistent rollout kernel (round 5; kernels_rollout.h, KIND 3).  The launch-per-step collector above
// pays, per row range and step, two kernel launches, an event, the event's completion latency and the weight stream of a fresh
// k_fused_act -- 74 - 76 us of GPU-side time per vector step of 4096 envs against 10 us for the same arithmetic inside the device
// rollout.  Here the device rollout's own kernel runs the policy (weights stationary, S8) and its env phase is the host's: a
// workgroup writes its rows' clipped actions into the caller's pinned buffer, raises its flag word in pinned memory and polls the
// host's word for its row range; the host waits for the flags of a range, steps it, raises its word.  No HIP call inside the step
// loop.  Same Philox counters, same forward / sampling / storage / bootstrap code as the device rollout; against the launch-per-step
// collector the buffers agree to float32 rounding (its k_fused_act runs the policy on the f32 pipe, the rollout kernel on the bf16
// pipe with split operands: the same relation the device rollout has to its per-step form), what the kernel only moves -- clipped
// actions to the host, rewards / observations from it -- is exact (tests/test_engine_gpu.py::test_served_host_rollout_...).
// Conditions (else *served stays false and the caller runs the launch-per-step loop): 256-wide x3 engine with the eight-wave rollout
// kernel, or (round 6) a 64-wide engine within the tile kernel's range (k_rollout64_tile<.., 3>: the shape of every reference config);
// whole 32-row tiles per row range, every workgroup resident at once (tiles <= CUs: a waiting workgroup never yields its CU),
// coherent pinned buffers (served_buffer_problem), no announced co-tenant of the device.  MOBROB_COLLECT_SERVER=0 switches it off; MOBROB_SERVER_TIMEOUT_S (default 60) bounds every wait on either side.
int collect_host_served(mobrob_ppo_engine* e, mobrob_env_step_range_fn step_range, void* env, int nparts, float* obs,
                        float* actions_clipped, float* rewards, uint8_t* dones, uint8_t* truncated, float* terminal_obs, bool* served) {
  *served = false;
  const int mode = env_int("MOBROB_COLLECT_SERVER", 1);   // 0 off, 1 when possible, 2 required (tests); read per rollout
  const int N = e->N, T = e->T, Dp = e->Dp;
  const int rblocks = cdiv(N, 32);
  if (mode == 0) return MOBROB_OK;
  const char* why = nullptr;
  int cus = 0;
  const bool wide = e->fused.enabled && wide_nets(e);   // 256-wide: k_rollout_persistent<.., 3, S8>; 64-wide: k_rollout64_tile<.., 3>
  if (!rollout_persistent_ok(e)) why = "the fused persistent rollout kernels are off for this engine";
  else if (wide && !rollout_s8(e)) why = "not a 256-wide x3 engine with the eight-wave rollout kernel";
  else if (!wide && (e->fused.H != GH || !rollout64_tile_kernel(e))) why = "not a 64-wide engine within the tile kernel's range";
  else if (getenv("MOBROB_COLLECT_TIMING") || env_int("MOBROB_COLLECT_THREADS", 0) != 0) why = "an instrumented / threaded collector was asked for";
  // a 32-row tile must not straddle two row ranges; ONE range takes any number of environments (the reference YAMLs: 2 - 16, half a tile)
  else if (nparts < 1 || nparts > MOBROB_MAX_PARTS || (nparts > 1 && (N % nparts != 0 || (N / nparts) % 32 != 0))) why = "row ranges are not whole 32-row tiles";
  else if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->cfg.device_id) != hipSuccess || rblocks > cus) why = "more tiles than compute units";
  // Other tenants of the device that this process cannot count: ranks rehearsing data parallelism on ONE device, a CU mask.  Every
  // workgroup of a served rollout must be resident at once (a waiting workgroup never yields its CU), so with them the launch-per-step
  // collector -- which always works -- is the one that runs.  (A tenant nobody announced is caught by the residency check below.)
  else if (env_int("MOBROB_DP_SAME_DEVICE", 0) != 0 && e->cfg.world_size > 1) why = "several data-parallel ranks share this device (MOBROB_DP_SAME_DEVICE)";
  else if (getenv("HSA_CU_MASK") || getenv("ROC_GLOBAL_CU_MASK")) why = "a compute-unit mask is set (HSA_CU_MASK / ROC_GLOBAL_CU_MASK)";
  else {
    const size_t N_ = (size_t)N;
    const struct { const void* p; size_t bytes; } bufs[6] = {{obs, N_ * e->D * 4}, {actions_clipped, N_ * e->A * 4}, {rewards, N_ * 4},
                                                              {dones, N_}, {truncated, N_}, {terminal_obs, N_ * e->D * 4}};
    for (const auto& b : bufs)
      if (!why) why = served_buffer_problem(b.p, b.bytes);
  }
  // Every workgroup of a served rollout must be resident at once, and it keeps its compute unit until the host has stepped all n_steps:
  // engines of ONE process that collect at the same time (a fleet's threads) share a DEVICE's compute units through that device's
  // counter -- the one that does not fit takes the launch-per-step path instead of queueing behind a kernel that waits for a host.
  constexpr int kLeaseDevices = 64;
  static std::atomic<int> cus_serving[kLeaseDevices];   // zero-initialised (static storage)
  std::atomic<int>& dev_lease = cus_serving[(unsigned)e->cfg.device_id % kLeaseDevices];
  struct Lease {
    std::atomic<int>& c; int n; bool held;
    ~Lease() { if (held) c.fetch_sub(n); }
  } lease{dev_lease, rblocks, false};
  if (!why) {
    if (dev_lease.fetch_add(rblocks) + rblocks > cus) { dev_lease.fetch_sub(rblocks); why = "the device's compute units are serving another engine's rollout"; }
    else lease.held = true;
  }
  if (why) return mode == 2 ? fail(MOBROB_ERR_STATE, "collect_host: MOBROB_COLLECT_SERVER=2 but %s", why) : MOBROB_OK;
  CHK(rollout_side_stream_init(e));
  CHK(streamer_init(e));
  constexpr int kHostWords = 16 * MOBROB_MAX_PARTS;
  constexpr int kStampWords = 64 * 8 * 2;   // -DMOBROB_SERVE_STAMPS builds: 64 steps x 8 stamps (long long) of workgroup 0
  const int fb = (rblocks + 15) / 16 * 16;
  if (!e->srv_flags || e->srv_blocks < fb) {
    if (e->srv_flags) (void)hipHostFree(e->srv_flags);
    e->srv_flags = nullptr;
    HIPC(hipHostMalloc((void**)&e->srv_flags, (size_t)(fb + kHostWords + 16 + kStampWords) * sizeof(unsigned), hipHostMallocCoherent | hipHostMallocMapped));
    e->srv_blocks = fb;
  }
  if (!e->srv_abort) HIPC(hipMalloc((void**)&e->srv_abort, 256));   // abort word | one 8-byte relay word per row range
  unsigned* gpu_flag = e->srv_flags;
  unsigned* host_flag = e->srv_flags + e->srv_blocks;
  int* err_word = reinterpret_cast<int*>(host_flag + kHostWords);
  memset(e->srv_flags, 0, (size_t)(e->srv_blocks + kHostWords + 16 + kStampWords) * sizeof(unsigned));
  HIPC(hipMemsetAsync(e->srv_abort, 0, 256, e->stream));
  const double timeout_s = env_double("MOBROB_SERVER_TIMEOUT_S", 60.0);

  // slot 0 <- the environments' current observations (the kernel reads its first tile from the slot, like the device rollout)
  hipLaunchKernelGGL(k_pull_rows, dim3(cdiv(N * Dp, 256)), dim3(256), 0, e->stream, obs, e->obs, N, e->D, Dp);
  if (wide && !e->fused.train_x3) pack_x3_all(e);
  RolloutArgs a = rollout_args(e);
  a.kind = 3; a.draw0 = e->draw_ro0;   // (host-side draw counter; no env seed, no device step counter)
  a.clip_act = actions_clipped;        // (the caller's pinned buffer)
  a.h_obs = obs; a.h_rew = rewards; a.h_done = dones; a.h_trunc = truncated; a.h_term = terminal_obs;
  a.h_gpu_flag = gpu_flag; a.h_host_flag = host_flag; a.h_error = err_word; a.abort_dev = e->srv_abort;
  a.rows_per_part = N / nparts; a.timeout_ticks = (long long)(timeout_s * 1e8);
  if (!wide)   // the served tile kernel's dynamic LDS exceeds 64 KB at 64 observation columns (per device and cheap: set per rollout)
    FUSED_DISPATCH_DP(Dp, HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_rollout64_tile<DPc, 3>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)rollout64_tile_lds_bytes(Dp, true))));

  // From the first KIND-3 launch on, EVERY way out of this function but the normal one tells the (possibly resident, possibly
  // waiting) workgroups to stop first: they would otherwise spin for the whole timeout and the next synchronising call with them.
  // The normal way out disarms it: the host has published step T of every row range, so nothing is left waiting.
  struct StopServing {
    mobrob_ppo_engine* e; unsigned* host_flag; int nparts; bool armed;
    ~StopServing() {
      if (!armed) return;
      for (int p = 0; p < nparts; ++p) __atomic_store_n(reinterpret_cast<unsigned long long*>(&host_flag[16 * p]), 0xFFFFFFFFull, __ATOMIC_RELEASE);
      (void)hipStreamSynchronize(e->stream);
      (void)hipStreamSynchronize(e->vstream);
    }
  } stop{e, host_flag, nparts, true};
  // chunks of the step loop on the compute stream, V(obs) of a finished chunk on the side stream: the device rollouts' path
  const ChunkPlan pl = chunk_plan(wide, rblocks, true, T, N);   // (64-wide: within the tile kernel's range, checked above)
  CHK(enqueue_rollout_chunks(e, a, pl));
  CHK(value_rollout_tail(e, pl, T * N));   // V(last_obs) is finish_rollout's
  HIPC(hipGetLastError());

  // ---- the host's side of the step loop: wait for the flags of a row range, step it, raise the range's word ----
  auto now_s = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; };
  const int bpp = nparts == 1 ? rblocks : (N / nparts) / 32;   // workgroups per row range
  {
    // Residency check, before the environment is touched: the clipped actions of step 0 of EVERY workgroup within a short bound
    // (MOBROB_SERVER_RESIDENCY_S, default 2 s; a resident workgroup needs ~25 us).  A workgroup that is not resident -- another
    // process on the device, a CU mask nobody announced -- would leave the resident ones waiting for the host while the host waits
    // for it: instead of stalling for the whole timeout and failing the rollout, the launches are told to stop and the caller runs
    // the launch-per-step collector from the untouched rollout state (nothing has been stepped, no counter has moved).
    const double bound = env_double("MOBROB_SERVER_RESIDENCY_S", 2.0);
    const double r0 = now_s();
    bool all_resident = false;
    for (unsigned spins = 0; bound > 0.0; ++spins) {   // (a bound <= 0 always misses: how the tests reach the fallback below)
      int b = 0;
      while (b < rblocks && __atomic_load_n(&gpu_flag[b], __ATOMIC_ACQUIRE) >= 1u) ++b;
      if (b == rblocks) { all_resident = true; break; }
      __builtin_ia32_pause();
      if ((spins & 0x3FFu) == 0x3FFu && (__atomic_load_n(err_word, __ATOMIC_ACQUIRE) != 0 || now_s() - r0 > bound)) break;
    }
    if (!all_resident) {   // (`stop` tells the launches to stop)
      if (mode == 2) return fail(MOBROB_ERR_STATE, "collect_host: MOBROB_COLLECT_SERVER=2 but not every workgroup of the rollout kernel became resident within %.1f s (another tenant on the device?)", bound);
      return MOBROB_OK;   // *served is false: the caller's launch-per-step loop takes over
    }
  }
  const bool timing = getenv("MOBROB_SERVER_TIMING") != nullptr;   // per-step split of the host thread's time (stderr)
  double tw = 0, te = 0;
  for (int t = 0; t < T; ++t) {
    for (int p = 0; p < nparts; ++p) {
      const unsigned want = (unsigned)(t + 1);
      double t_wait = -1.0;
      const double c0 = timing ? now_s() : 0;
      for (int b = p * bpp; b < (p + 1) * bpp; ++b) {
        unsigned spins = 0;
        while (__atomic_load_n(&gpu_flag[b], __ATOMIC_ACQUIRE) < want) {
          __builtin_ia32_pause();
          if ((++spins & 0xFFFFu) == 0) {   // every ~65 k polls: the device gave up, or nothing moved for the whole timeout
            if (__atomic_load_n(err_word, __ATOMIC_ACQUIRE) != 0)
              return fail(MOBROB_ERR_STATE, "collect_host: the rollout kernel gave up waiting for the host at step %d", *err_word - 1);
            const double tn = now_s();
            if (t_wait < 0) t_wait = tn;
            if (tn - t_wait > timeout_s)
              return fail(MOBROB_ERR_HIP, "collect_host: no actions from the device for %.0f s (step %d, row range %d)", timeout_s, t, p);
          }
        }
      }
      const int r0 = p * (N / nparts);
      const double c1 = timing ? now_s() : 0;
      const int32_t ntrunc = step_range(env, r0, r0 + N / nparts, actions_clipped, obs, rewards, dones, truncated, terminal_obs);
      if (ntrunc < 0) return fail(MOBROB_ERR_STATE, "collect_host: the environment's step_range returned %d", ntrunc);
      __atomic_store_n(reinterpret_cast<unsigned long long*>(&host_flag[16 * p]), ((unsigned long long)(unsigned)ntrunc << 32) | want, __ATOMIC_RELEASE);
      if (timing) { tw += c1 - c0; te += now_s() - c1; }
    }
  }
  stop.armed = false;   // the normal way out: every step of every row range has been published
#ifdef MOBROB_SERVE_STAMPS
  if (timing) {
    (void)hipStreamSynchronize(e->stream);
    const long long* st = reinterpret_cast<const long long*>(err_word + 16);
    double d[8] = {0};
    int n = 0;
    for (int t = 8; t + 1 < 64 && t + 1 < T; ++t, ++n) {
      d[0] += st[8 * t + 1] - st[8 * t + 0];        // publish -> host word seen
      d[1] += st[8 * t + 2] - st[8 * t + 1];        // barrier (4b)
      d[2] += st[8 * t + 3] - st[8 * t + 2];        // pull (this wave)
      d[3] += st[8 * t + 4] - st[8 * t + 3];        // barrier (4c)
      d[4] += st[8 * t + 5] - st[8 * t + 4];        // env phase + state update
      d[5] += st[8 * (t + 1) + 6] - st[8 * t + 5];  // layers, head, sampling (next step)
      d[6] += st[8 * (t + 1) + 7] - st[8 * (t + 1) + 6];  // drain of the action stores
      d[7] += st[8 * (t + 1) + 0] - st[8 * (t + 1) + 7];  // barrier (4)
    }
    fprintf(stderr, "[served stamps, workgroup 0, us] wait for host %.2f | (4b) %.2f | pull %.2f | (4c) %.2f | env+state %.2f | policy %.2f | drain %.2f | (4) %.2f\n",
            d[0] / n / 100, d[1] / n / 100, d[2] / n / 100, d[3] / n / 100, d[4] / n / 100, d[5] / n / 100, d[6] / n / 100, d[7] / n / 100);
  }
#endif
  if (timing)
    fprintf(stderr, "[collect_host served] per step: waiting for the device %.1f us, env %.1f us (%d row ranges)\n", 1e6 * tw / T, 1e6 * te / T, nparts);
  e->t = T;
  e->nparts = nparts;
  for (int p = 0; p < nparts; ++p) { e->part_act_t[p] = e->part_store_t[p] = T; e->part_obs_t[p] = T; }
  if (e->draw_counter < e->draw_ro0 + (uint32_t)T) e->draw_counter = e->draw_ro0 + (uint32_t)T;
  *served = true;
  const int rc = mobrob_ppo_finish_rollout(e, obs, dones);   // last observations / dones, V(last_obs), GAE; synchronises the stream
  if (rc == MOBROB_OK && __atomic_load_n(err_word, __ATOMIC_ACQUIRE) != 0)
    return fail(MOBROB_ERR_STATE, "collect_host: the rollout kernel gave up waiting for the host at step %d", *err_word - 1);
  return rc;
}
}  // namespace

// The whole pipelined rollout in one call: rollout_begin, n_steps x nparts x (wait_part, env step of the range,
// store_part + act_part), finish_rollout -- the collector loop of SB3's collect_rollouts as native code, driving a
// native vectorised environment through one function pointer.
int mobrob_ppo_collect_host(mobrob_ppo_engine_t* e, mobrob_env_step_range_fn step_range, void* env, int32_t nparts,
                            float* obs, float* actions_clipped, float* rewards, uint8_t* dones, uint8_t* truncated,
                            float* terminal_obs) {
  if (!e || !step_range || !obs || !actions_clipped || !rewards || !dones || !truncated || !terminal_obs)
    return fail(MOBROB_ERR_INVALID, "collect_host: null argument");
  CHK(mobrob_ppo_rollout_begin(e));
  {  // fused engines (256-wide x3, 64-wide): the persistent rollout kernel serves the host environment (no launch, no event per step)
    bool served = false;
    const int rc = collect_host_served(e, step_range, env, nparts, obs, actions_clipped, rewards, dones, truncated, terminal_obs, &served);
    if (served || rc != MOBROB_OK) return rc;
  }
  for (int p = 0; p < nparts; ++p) CHK(mobrob_ppo_act_part(e, p, nparts, obs, actions_clipped));
  const bool timing = getenv("MOBROB_COLLECT_TIMING") != nullptr;
  // Two host threads (round 5, OPT-IN: MOBROB_COLLECT_THREADS=1).  The single-thread loop below spends, per vector step of 4096 envs at
  // two parts (MOBROB_COLLECT_TIMING=1, profiles/r5/host_path_timing.txt): 55 us stepping the simulator, 12 us in HIP calls (two
  // launches and an event record per part), 16 - 21 us waiting for the policy's actions.  With a DRIVER thread that owns the stream
  // -- it turns "part p stepped" into store_part + act_part and "act of part p finished" (hipEventQuery, no blocking wait) into
  // "part p ready" -- the calling thread only steps the environment.  Same kernels, same per-part order on the one stream: the rollout
  // is the single-thread loop's bit for bit.  MEASURED (whole iteration, same box, alternating): 198.2 / 198.9 ms single thread,
  // 200.0 - 203.4 ms with the driver thread (16, 15 or 14 env threads): what bounds a part's cycle is sim -> launch latency -> two small
  // kernels -> sim, and the spinning driver takes a core from the simulator's team.  Kept for hosts with cores to spare; off by default.
  const bool threaded = nparts >= 2 && !timing && env_int("MOBROB_COLLECT_THREADS", 0) != 0;
  if (threaded) {
    struct Shared {
      std::atomic<int> ready[MOBROB_MAX_PARTS];     // acts of part p the GPU has finished (actions of step ready - 1 are in host memory)
      std::atomic<int> simdone[MOBROB_MAX_PARTS];   // steps of part p the simulator has finished
      std::atomic<int> ntrunc[MOBROB_MAX_PARTS];    // truncated rows of the part's newest step
      std::atomic<int> err{0};
    } sh;
    for (int p = 0; p < MOBROB_MAX_PARTS; ++p) { sh.ready[p] = 0; sh.simdone[p] = 0; sh.ntrunc[p] = 0; }
    std::string driver_msg;
    int driver_rc = MOBROB_OK;
    const int T = e->T;
    auto driver_body = [&] {
      if (hipSetDevice(e->cfg.device_id) != hipSuccess) { driver_rc = MOBROB_ERR_HIP; driver_msg = "collect_host driver: hipSetDevice failed"; sh.err = 1; return; }
      int acted[MOBROB_MAX_PARTS], synced[MOBROB_MAX_PARTS], stored[MOBROB_MAX_PARTS];
      for (int p = 0; p < nparts; ++p) { acted[p] = 1; synced[p] = 0; stored[p] = 0; }
      for (;;) {
        bool all_done = true, progress = false;
        for (int p = 0; p < nparts && !sh.err.load(std::memory_order_relaxed); ++p) {
          if (synced[p] < acted[p]) {                       // the part's newest act: finished?
            const hipError_t q = hipEventQuery(e->ev_part[p]);
            if (q == hipSuccess) {
              synced[p] = acted[p];
              sh.ready[p].store(synced[p], std::memory_order_release);
              progress = true;
            } else if (q != hipErrorNotReady) {
              driver_rc = MOBROB_ERR_HIP; driver_msg = std::string("collect_host driver: ") + hipGetErrorString(q); sh.err = 1;
            }
          }
          if (stored[p] < T && sh.simdone[p].load(std::memory_order_acquire) > stored[p]) {   // the part was stepped: store, act again
            const int nt = sh.ntrunc[p].load(std::memory_order_relaxed);
            int rc = mobrob_ppo_store_part(e, p, nparts, rewards, dones, nt ? truncated : nullptr, nt ? terminal_obs : nullptr, obs);
            ++stored[p];
            if (rc == MOBROB_OK && stored[p] < T) { rc = mobrob_ppo_act_part(e, p, nparts, obs, actions_clipped); ++acted[p]; }
            if (rc != MOBROB_OK) { driver_rc = rc; driver_msg = g_err; sh.err = 1; }
            progress = true;
          }
          if (stored[p] < T) all_done = false;
        }
        if (all_done || sh.err.load(std::memory_order_relaxed)) break;
        if (!progress) __builtin_ia32_pause();
      }
    };
    std::thread driver;
    try {
      driver = std::thread(driver_body);
    } catch (...) {   // no thread to be had: nothing has been stepped yet, so the single-thread loop below takes over from here
      driver = std::thread();
    }
    if (driver.joinable()) {
    int sim_rc = MOBROB_OK;
    for (int t = 0; t < T && !sh.err.load(std::memory_order_relaxed); ++t) {
      for (int p = 0; p < nparts; ++p) {
        int r0, n;
        if (part_range(e, p, nparts, &r0, &n) != MOBROB_OK) { sim_rc = MOBROB_ERR_INVALID; sh.err = 1; break; }
        while (sh.ready[p].load(std::memory_order_acquire) < t + 1 && !sh.err.load(std::memory_order_relaxed)) __builtin_ia32_pause();
        if (sh.err.load(std::memory_order_relaxed)) break;
        const int32_t ntrunc = step_range(env, r0, r0 + n, actions_clipped, obs, rewards, dones, truncated, terminal_obs);
        if (ntrunc < 0) { sim_rc = MOBROB_ERR_STATE; sh.err = 1; break; }
        sh.ntrunc[p].store(ntrunc, std::memory_order_relaxed);
        sh.simdone[p].store(t + 1, std::memory_order_release);
      }
    }
    driver.join();
    if (driver_rc != MOBROB_OK) return fail(driver_rc, "%s", driver_msg.c_str());
    if (sim_rc != MOBROB_OK) return fail(sim_rc, "collect_host: the environment's step_range failed");
    return mobrob_ppo_finish_rollout(e, obs, dones);
    }
  }
  double tw = 0, te = 0, tq = 0;
  auto now = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; };
  for (int t = 0; t < e->T; ++t) {
    for (int p = 0; p < nparts; ++p) {
      int r0, n;
      CHK(part_range(e, p, nparts, &r0, &n));
      const double t0 = timing ? now() : 0;
      CHK(mobrob_ppo_wait_part(e, p));
      const double t1 = timing ? now() : 0;
      const int32_t ntrunc = step_range(env, r0, r0 + n, actions_clipped, obs, rewards, dones, truncated, terminal_obs);
      const double t2 = timing ? now() : 0;
      if (ntrunc < 0) return fail(MOBROB_ERR_STATE, "collect_host: the environment's step_range returned %d", ntrunc);
      CHK(mobrob_ppo_store_part(e, p, nparts, rewards, dones, ntrunc ? truncated : nullptr,
                                ntrunc ? terminal_obs : nullptr, obs));
      if (t + 1 < e->T) CHK(mobrob_ppo_act_part(e, p, nparts, obs, actions_clipped));
      if (timing) { tw += t1 - t0; te += t2 - t1; tq += now() - t2; }
    }
  }
  if (timing)
    fprintf(stderr, "[collect_host] per step: wait %.1f us, env %.1f us, enqueue %.1f us (%d parts)\n", tw / e->T, te / e->T,
            tq / e->T, nparts);
  return mobrob_ppo_finish_rollout(e, obs, dones);
}

int mobrob_ppo_collect_synthetic(mobrob_ppo_engine_t* e, float p_term, int32_t time_limit) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  mobrob_ppo_engine::RolloutSpec sp;
  memset(&sp, 0, sizeof sp);  // padding bytes too: specs are compared with memcmp
  sp.kind = 1; sp.p_term = p_term; sp.time_limit = time_limit;
  return collect_device(e, sp);
}

int mobrob_ppo_collect_goal_env(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env) {
  if (!e || !env) return fail(MOBROB_ERR_INVALID, "null argument");
  if (env->pos_dim < 1 || env->pos_dim > 3 || 3 * env->pos_dim > e->D)
    return fail(MOBROB_ERR_INVALID, "goal env: pos_dim must be 1..3 and 3*pos_dim <= obs_dim");
  if (e->A > 32) return fail(MOBROB_ERR_INVALID, "goal env: act_dim must be <= 32");
  if (env->time_limit < 1) return fail(MOBROB_ERR_INVALID, "goal env: time_limit must be >= 1");
  mobrob_ppo_engine::RolloutSpec sp;
  memset(&sp, 0, sizeof sp);
  sp.kind = 2; sp.time_limit = env->time_limit;
  GoalEnvParams& g = sp.goal;
  g.P = env->pos_dim; g.terminate_on_goal = env->terminate_on_goal != 0; g.time_limit = env->time_limit;
  g.dt = env->dt; g.extent = env->extent; g.reach = env->reach_radius; g.bonus = env->goal_bonus;
  g.extra_bonus = env->extra_bonus; g.noise = env->obs_noise;
  for (int j = 0; j < 3; ++j)
    for (int k = 0; k < 32; ++k) g.mix[j][k] = (j < env->pos_dim && k < e->A) ? env->mix[j][k] : 0.f;
  return collect_device(e, sp);
}

int mobrob_ppo_episode_stats(mobrob_ppo_engine_t* e, mobrob_episode_stats_t* out, int32_t reset) {
  if (!e || !out) return fail(MOBROB_ERR_INVALID, "null argument");
  double h[4];
  HIPC(hipMemcpyAsync(h, e->ep_stats, sizeof h, hipMemcpyDeviceToHost, e->stream));
  if (reset) HIPC(hipMemsetAsync(e->ep_stats, 0, sizeof h, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  out->episodes = (int64_t)h[0]; out->return_sum = h[1]; out->length_sum = h[2]; out->goals = (int64_t)h[3];
  return MOBROB_OK;
}

int mobrob_ppo_episode_records(mobrob_ppo_engine_t* e, float* out, int32_t max_records) {
  if (!e || !out || max_records < 0) return fail(MOBROB_ERR_INVALID, "episode_records: bad argument");
  std::vector<double> h(kEpStatsDoubles);
  HIPC(hipMemcpyAsync(h.data(), e->ep_stats, h.size() * sizeof(double), hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  const uint64_t written = (uint64_t)h[4];
  uint64_t first = e->ep_ring_read;
  if (written - first > (uint64_t)kEpRing) first = written - kEpRing;           // older ones were overwritten
  if (written - first > (uint64_t)max_records) first = written - max_records;   // the caller wants the newest
  int n = 0;
  for (uint64_t k = first; k < written; ++k, ++n) {
    memcpy(&out[2 * n], &h[5 + k % kEpRing], 2 * sizeof(float));  // one 64-bit record = (return, length) as two floats
  }
  e->ep_ring_read = written;
  return n;
}

// ---- env-side controllers (robot_ctrl.h) -----------------------------------------------------------------
}  // extern "C"
namespace {
// host arrays are staged through temporary device buffers; device arrays (dev_ptrs != 0) are used in place
struct CtrlBuf {
  mobrob_ppo_engine* e; bool dev; std::vector<void*> owned;
  std::vector<std::pair<void*, std::pair<void*, size_t>>> outs;  // device -> host copies to make at the end
  ~CtrlBuf() { for (void* p : owned) (void)hipFree(p); }
  int in(const float* host, size_t count, const float** out) {
    using T = float;
    if (dev) { *out = host; return MOBROB_OK; }
    void* d = nullptr;
    HIPC(hipMalloc(&d, count * sizeof(T)));
    owned.push_back(d);
    HIPC(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, e->stream));
    *out = static_cast<const T*>(d);
    return MOBROB_OK;
  }
  int inout(float* host, size_t count, float** out, bool copy_in) {
    using T = float;
    if (dev) { *out = host; return MOBROB_OK; }
    void* d = nullptr;
    HIPC(hipMalloc(&d, count * sizeof(T)));
    owned.push_back(d);
    if (copy_in) HIPC(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, e->stream));
    outs.push_back({d, {host, count * sizeof(T)}});
    *out = static_cast<T*>(d);
    return MOBROB_OK;
  }
  int finish() {
    for (auto& o : outs) HIPC(hipMemcpyAsync(o.second.first, o.first, o.second.second, hipMemcpyDeviceToHost, e->stream));
    if (!dev) HIPC(hipStreamSynchronize(e->stream));
    return MOBROB_OK;
  }
};
}  // namespace
extern "C" {

int mobrob_ctrl_turtlebot3(mobrob_ppo_engine_t* e, int32_t n, int32_t dev_ptrs, const float* pos, const float* theta,
                           const float* goal, const float* gain_changes, float* twist) {
  if (!e || n < 1 || !pos || !theta || !goal || !gain_changes || !twist)
    return fail(MOBROB_ERR_INVALID, "ctrl_turtlebot3: bad argument");
  CtrlBuf b{e, dev_ptrs != 0, {}, {}};
  const float *dp, *dt, *dg, *da;
  float* dtw;
  CHK(b.in(pos, (size_t)2 * n, &dp)); CHK(b.in(theta, (size_t)n, &dt)); CHK(b.in(goal, (size_t)2 * n, &dg));
  CHK(b.in(gain_changes, (size_t)2 * n, &da)); CHK(b.inout(twist, (size_t)2 * n, &dtw, false));
  hipLaunchKernelGGL(k_ctrl_turtlebot3, dim3(cdiv(n, 256)), dim3(256), 0, e->stream, n, dp, dt, dg, da, dtw);
  HIPC(hipGetLastError());
  return b.finish();
}

int mobrob_ctrl_drone_pid(mobrob_ppo_engine_t* e, int32_t n, int32_t dev_ptrs, const mobrob_drone_params_t* prm,
                          const float* pos, const float* rpy, const float* goal, const float* action, float* ctrl_state,
                          float* out) {
  if (!e || n < 1 || !prm || !pos || !rpy || !goal || !action || !ctrl_state || !out)
    return fail(MOBROB_ERR_INVALID, "ctrl_drone_pid: bad argument");
  if (!(prm->dt > 0.f) || !(prm->mass > 0.f)) return fail(MOBROB_ERR_INVALID, "ctrl_drone_pid: dt and mass must be positive");
  CtrlBuf b{e, dev_ptrs != 0, {}, {}};
  const float *dp, *dr, *dg, *da;
  float *ds, *dout;
  CHK(b.in(pos, (size_t)3 * n, &dp)); CHK(b.in(rpy, (size_t)3 * n, &dr)); CHK(b.in(goal, (size_t)3 * n, &dg));
  CHK(b.in(action, (size_t)18 * n, &da)); CHK(b.inout(ctrl_state, (size_t)12 * n, &ds, true));
  CHK(b.inout(out, (size_t)4 * n, &dout, false));
  DroneCtrlParams p{prm->mass, prm->g, prm->dt, prm->max_thrust, prm->max_xy_torque, prm->max_z_torque, prm->max_roll_pitch,
                    prm->tune_fac};
  hipLaunchKernelGGL(k_ctrl_drone_pid, dim3(cdiv(n, 256)), dim3(256), 0, e->stream, n, p, dp, dr, dg, da, ds, dout);
  HIPC(hipGetLastError());
  return b.finish();
}

// ---- update ----------------------------------------------------------------------------------------
int mobrob_ppo_num_minibatches(const mobrob_ppo_engine_t* e) { return e ? e->nmb : -1; }

int mobrob_ppo_epoch_begin(mobrob_ppo_engine_t* e, const int64_t* perm) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  if (!e->rollout_ready) return fail(MOBROB_ERR_STATE, "epoch_begin: rollout not finished (finish_rollout / collect first)");
  const int total = e->N * e->T;
  if (perm) {
    // a caller's permutation is checked before a kernel scatters through it (k_perm_from_host writes rows[] and the
    // minibatch-of-row table at the indices it holds): every flat index once, none out of range.  FIRST, before any engine
    // state moves (the parity of the max-|adv| words below, the training records): a rejected call leaves nothing behind.
    std::vector<uint64_t> seen(((size_t)total + 63) / 64, 0);
    for (int i = 0; i < total; ++i) {
      const int64_t v = perm[i];
      if (v < 0 || v >= total) return fail(MOBROB_ERR_INVALID, "epoch_begin: perm[%d] = %lld is outside [0, %d)", i, (long long)v, total);
      uint64_t& w = seen[(size_t)v >> 6];
      const uint64_t bit = 1ull << (v & 63);
      if (w & bit) return fail(MOBROB_ERR_INVALID, "epoch_begin: perm holds index %lld twice (not a permutation of [0, %d))", (long long)v, total);
      w |= bit;
    }
  }
  ensure_train_records(e);
  AdvStatArgs as{};
  as.adv = e->adv; as.total = total; as.T = e->T; as.N = e->N; as.bl = e->Bl; as.nmb = e->nmb;
  as.bins = e->advbins;
  unsigned* maxw = reinterpret_cast<unsigned*>(e->advbins + (size_t)2 * e->nmb);  // two words, used alternately
  as.absmax_bits = maxw + (e->adv_pass & 1); as.absmax_next = maxw + ((e->adv_pass + 1) & 1);
  e->adv_pass++;
  if (perm) {
    HIPC(hipMemcpyAsync(e->perm_dev, perm, (size_t)total * 8, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_perm_from_host, dim3(cdiv(total, 256)), dim3(256), 0, e->stream, e->perm_dev, total, e->T,
                       e->N, e->Bl, e->rows);
    as.mb_of_row = reinterpret_cast<const int*>(e->perm_dev);
  } else {
    const uint64_t key = (e->cfg.seed * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)(e->cfg.rank + 1) << 48) ^ (e->perm_counter + 1);
    e->perm_counter++;
    as.half_bits = feistel_half_bits((uint64_t)total); as.k0 = (uint32_t)key; as.k1 = (uint32_t)(key >> 32);
    hipLaunchKernelGGL(k_perm_feistel, dim3(cdiv(total, 256)), dim3(256), 0, e->stream, total, e->T, e->N,
                       as.half_bits, as.k0, as.k1, e->rows, (int64_t*)nullptr);
  }
  // advantage statistics: one coalesced pass in storage order, order-independent integer sums (kernels_generic.h)
  const int sgrid = std::max(1, std::min(256, cdiv(total, 4 * 1024)));  // at most one workgroup per CU (see k_adv_absmax)
  const size_t slds = e->nmb <= kAdvLdsMinibatches ? (size_t)2 * e->nmb * adv_bin_replicas(e->nmb) * sizeof(unsigned long long) : 0;
  hipLaunchKernelGGL(k_adv_absmax, dim3(sgrid), dim3(1024), 0, e->stream, as);
  hipLaunchKernelGGL(k_adv_stats_stream, dim3(sgrid), dim3(1024), slds, e->stream, as);
  hipLaunchKernelGGL(k_adv_fold, dim3(cdiv(e->nmb, 64)), dim3(64), 0, e->stream, as, e->advstat);
  HIPC(hipGetLastError());
  e->epoch_open = true;
  return MOBROB_OK;
}

int mobrob_ppo_minibatch_grad(mobrob_ppo_engine_t* e, int32_t mb) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  if (!e->epoch_open) return fail(MOBROB_ERR_STATE, "minibatch_grad before epoch_begin");
  if (mb < 0 || mb >= e->nmb) return fail(MOBROB_ERR_INVALID, "minibatch %d out of range [0,%d)", mb, e->nmb);
  const int start = mb * e->Bl, B = std::min(e->Bl, e->N * e->T - start);
  const float inv_bg = 1.0f / (float)((int64_t)B * e->cfg.world_size);
  e->cur_count = B;
  if (!e->fused.enabled) generic_minibatch_grad(e, mb, start, B, inv_bg);
  else if (e->fused.H == 64) fused64_minibatch_grad(e, mb, start, B, inv_bg);
  else fused_minibatch_grad(e, mb, start, B, inv_bg);
  HIPC(hipGetLastError());
  e->grad_pending = true;
  return MOBROB_OK;
}

namespace {
// everything of AdamPackArgs that does not change from step to step
void fill_adam_pack_args(mobrob_ppo_engine* e, AdamPackArgs& a) {
  a.p = e->params; a.g = e->grads; a.m = e->m; a.v = e->v; a.P = e->P;
  a.chunks = e->chunks_dev; a.partial = e->chunk_partial; a.nchunks = e->nchunks;
  if (e->use_norm_records) {   // inside train_loop: the reduction kernel left the norm records, k_adam_pack folds them
    a.partial = e->norm_rec_sum; a.fold_idx = e->fold_idx_dev;
    for (int i = 0; i <= kMaxTensors; ++i) a.fold_start[i] = e->fold_start[i];
  }
  a.max_norm = (float)e->cfg.max_grad_norm; a.beta1 = (float)e->cfg.adam_beta1; a.beta2 = (float)e->cfg.adam_beta2;
  a.eps = (float)e->cfg.adam_eps;
  for (int i = 0; i <= kMaxTensors; ++i) a.offs[i] = e->offs[i];
  a.ntens = e->ntens; a.two_by_two = e->Lp == 2 && e->Lv == 2; a.id_pw1 = T_PW1; a.id_vw1 = T_VW1; a.id_aw = T_AW; a.id_vw = T_VW; a.HL = e->HL; a.GL = e->GL;
  a.D = e->D; a.Dp = e->Dp; a.A = e->A; a.Ap = e->Ap; a.H1 = e->H1; a.H2 = e->H2; a.G1 = e->G1; a.G2 = e->G2;
  a.pW1p = e->pW1p; a.vW1p = e->vW1p; a.aWp = e->aWp; a.vWp = e->vWp;
  for (int n = 0; n < 2; ++n) {
    const bool on = e->fused.enabled;
    a.fW1f[n] = on ? (float*)e->fused.net[n].W1f : nullptr;
    a.fW2f[n] = on ? (float*)e->fused.net[n].W2f : nullptr;
    a.fW3f[n] = on ? (float*)e->fused.net[n].W3f : nullptr;
    // k_chain_train reads its own packs only: the backward packs of the other 256-wide gradient kernels (W2b, W3b, W2bx) are not
    // refreshed per step while it is the engine's gradient kernel (set_params / load rebuild every pack: fused_repack, pack_x3_all).
    // W3h stays: k_value_batch's 16-wide head reads it.
    const bool ch = on && e->fused.train_chain;
    a.fW2b[n] = on && !ch ? (float*)e->fused.net[n].W2b : nullptr;
    a.fW3b[n] = on && !ch ? (float*)e->fused.net[n].W3b : nullptr;
    a.fW3h[n] = (on && (n == 1 || e->fused.A <= 16)) ? (float*)e->fused.net[n].W3h : nullptr;
    a.fb1s[n] = on ? (float*)e->fused.net[n].b1s : nullptr;
    a.fb2s[n] = on ? (float*)e->fused.net[n].b2s : nullptr;
    const bool x3 = on && e->fused.train_x3;  // the gradient kernel reads the x3 packs every step: k_adam_pack keeps them current
    a.xW1[n] = x3 ? reinterpret_cast<unsigned short*>(const_cast<unsigned*>(e->fused.net[n].W1x)) : nullptr;
    a.xW2[n] = x3 ? reinterpret_cast<unsigned short*>(const_cast<unsigned*>(e->fused.net[n].W2x)) : nullptr;
    a.xW2b[n] = x3 && !ch ? reinterpret_cast<unsigned short*>(const_cast<unsigned*>(e->fused.net[n].W2bx)) : nullptr;
    // likewise the chain packs of k_chain_train
    a.cW1[n] = ch ? reinterpret_cast<unsigned short*>(const_cast<unsigned*>(e->fused.net[n].W1c)) : nullptr;
    a.cW2[n] = ch ? reinterpret_cast<unsigned short*>(const_cast<unsigned*>(e->fused.net[n].W2c)) : nullptr;
    a.cW2b[n] = ch ? reinterpret_cast<unsigned short*>(const_cast<unsigned*>(e->fused.net[n].W2bc)) : nullptr;
    a.cW3[n] = ch ? const_cast<float*>(e->fused.net[n].W3c) : nullptr;
    a.cW3b[n] = ch ? const_cast<float*>(e->fused.net[n].W3bc) : nullptr;
  }
}
}  // namespace

namespace {
// The optimizer's step counter moves here only: Adam's bias corrections of the step that begins, formed in float64 and rounded once.
struct AdamStep { float step_size, bc2_sqrt; };
AdamStep next_adam_step(mobrob_ppo_engine* e) {
  e->adam_step++;
  const double bc1 = 1.0 - std::pow(e->cfg.adam_beta1, (double)e->adam_step), bc2 = 1.0 - std::pow(e->cfg.adam_beta2, (double)e->adam_step);
  return {(float)(e->cfg.learning_rate / bc1), (float)std::sqrt(bc2)};
}
// the row of the statistics ring the step that begins logs into (the oldest rows are dropped if nobody fetched them)
int next_stats_row(mobrob_ppo_engine* e) {
  if (e->stats_n >= e->stats_cap) e->stats_n = 0;
  return e->stats_n++;
}
// first half of an optimizer step: loss statistics + per-tensor sums of squares of the (reduced) gradient
StatsArgs apply_norms(mobrob_ppo_engine* e) {
  StatsArgs st = stats_args(e);
  st.stats_row = e->stats + (size_t)next_stats_row(e) * 8;
  st.inv_bg = 1.0f / (float)((int64_t)e->cur_count * e->cfg.world_size);
  if (!e->use_norm_records)  // (on: the reduction kernel of this step left the norm records)
    hipLaunchKernelGGL(k_sqnorm_chunks, dim3(e->nchunks), dim3(256), 0, e->stream, e->grads, e->chunks_dev,
                       e->chunk_partial, st);
  return st;
}
// second half: clip coefficient, Adam, re-pack
int apply_adam(mobrob_ppo_engine* e, const StatsArgs& st) {
  const AdamStep step = next_adam_step(e);
  AdamPackArgs a{};
  fill_adam_pack_args(e, a);
  a.step_size = step.step_size; a.bc2_sqrt = step.bc2_sqrt;
  if (e->use_norm_records) a.st = st;   // k_adam_pack logs the step's statistics itself (a fused engine: st.sde is 0)
  a.stats_row = st.stats_row;
  a.loss_sums_zero = e->fused.enabled ? e->grads + e->P : nullptr;
  hipLaunchKernelGGL(k_adam_pack, dim3(cdiv(e->P, 256)), dim3(256), 0, e->stream, a);
  HIPC(hipGetLastError());
  e->grad_pending = false;
  return MOBROB_OK;
}
}  // namespace

namespace {
// clip + Adam of the pending gradient, with SB3's target_kl check in front of it when that option is on: the
// minibatch's approx_kl is known after the loss statistics; above 1.5 x target the optimizer step of THIS minibatch is
// dropped (*stopped = 1; the caller drops the rest of train()).  One 4-byte read-back per step.  Under data parallel
// the value is that of the union minibatch (its sum travelled with the gradient), bit-equal on every rank.
int apply_checked(mobrob_ppo_engine* e, int32_t* stopped) {
  *stopped = 0;
  ProfScope ps(e, MOBROB_K_APPLY);
  const StatsArgs st = apply_norms(e);
  if (e->target_kl > 0.0) {
    float approx_kl = 0.f;
    HIPC(hipMemcpyAsync(&approx_kl, st.stats_row + 4, sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPC(hipStreamSynchronize(e->stream));
    if ((double)approx_kl > 1.5 * e->target_kl) {
      *stopped = 1;
      e->grad_pending = false;
      // the row of the dropped step carries its losses (SB3 appends them before the check) but no gradient norm:
      // all-ones bits = NaN, skipped by the averages
      HIPC(hipMemsetAsync(st.stats_row + 6, 0xFF, sizeof(float), e->stream));
      if (e->fused.enabled) HIPC(hipMemsetAsync(e->grads + e->P, 0, 8 * sizeof(float), e->stream));  // what k_adam_pack would have re-zeroed
      return MOBROB_OK;
    }
  }
  return apply_adam(e, st);
}
}  // namespace

int mobrob_ppo_minibatch_apply(mobrob_ppo_engine_t* e) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  if (!e->grad_pending) return fail(MOBROB_ERR_STATE, "minibatch_apply without a pending gradient");
  if (e->target_kl > 0.0)
    return fail(MOBROB_ERR_STATE, "target_kl is set: a step-wise driver must call mobrob_ppo_minibatch_apply_checked and honour its stop flag");
  int32_t stopped = 0;
  return apply_checked(e, &stopped);
}

int mobrob_ppo_minibatch_apply_checked(mobrob_ppo_engine_t* e, int32_t* stopped) {
  if (!e || !stopped) return fail(MOBROB_ERR_INVALID, "minibatch_apply_checked: null argument");
  if (!e->grad_pending) return fail(MOBROB_ERR_STATE, "minibatch_apply without a pending gradient");
  return apply_checked(e, stopped);
}

int mobrob_ppo_sde_reset_noise(mobrob_ppo_engine_t* e) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  if (!e->sde) return fail(MOBROB_ERR_STATE, "sde_reset_noise: the engine was not created with use_sde");
  sde_resample(e, 0, e->N, e->draw_counter++, nullptr, true);
  HIPC(hipGetLastError());
  return MOBROB_OK;
}

int mobrob_ppo_sde_set_noise(mobrob_ppo_engine_t* e, const float* z) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  if (!e->sde) return fail(MOBROB_ERR_STATE, "sde_set_noise: the engine was not created with use_sde");
  if (e->sde_hold != (z != nullptr) && e->ro_exec) {
    // a captured device rollout has the resampling launches (or their absence) baked in: capture again under the new mode
    HIPC(hipStreamSynchronize(e->stream));
    (void)hipGraphExecDestroy(e->ro_exec); e->ro_exec = nullptr;
    if (e->ro_graph) { (void)hipGraphDestroy(e->ro_graph); e->ro_graph = nullptr; }
  }
  e->sde_hold = z != nullptr;
  if (!z) return MOBROB_OK;
  const size_t HLA = (size_t)e->HL * e->A, n = (size_t)e->N * HLA;
  if (n > (size_t)1 << 30) return fail(MOBROB_ERR_INVALID, "sde_set_noise: too many matrix elements");
  // staged through the matrices' own storage: z is uploaded into it and scaled in place
  HIPC(hipMemcpyAsync(e->sde_E, z, n * 4, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_sde_from_z, dim3(cdiv((int)n, 256)), dim3(256), 0, e->stream, e->sde_E, Pp(e, T_LOGSTD), (int)HLA, e->A, e->sde_mode, (int)n, e->sde_E);
  hipLaunchKernelGGL(k_copy_f32, dim3(cdiv((int)HLA, 256)), dim3(256), 0, e->stream, e->sde_E, e->sde_E1, (int)HLA);   // exploration_mat := env 0's
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(e->stream));   // z may be pageable host memory
  return MOBROB_OK;
}

int mobrob_ppo_set_hyper(mobrob_ppo_engine_t* e, int32_t which, double value) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  switch (which) {
    case MOBROB_HYPER_LEARNING_RATE:
      if (!(value >= 0.0)) return fail(MOBROB_ERR_INVALID, "learning_rate must be >= 0");
      e->cfg.learning_rate = value; break;
    case MOBROB_HYPER_CLIP_RANGE:
      if (!(value >= 0.0)) return fail(MOBROB_ERR_INVALID, "clip_range must be >= 0");
      e->cfg.clip_range = value; break;
    case MOBROB_HYPER_CLIP_RANGE_VF: e->clip_vf = value >= 0.0 ? value : -1.0; break;  // negative / NaN: None
    case MOBROB_HYPER_TARGET_KL: e->target_kl = value > 0.0 ? value : -1.0; break;
    case MOBROB_HYPER_ENT_COEF: e->cfg.ent_coef = value; break;
    case MOBROB_HYPER_VF_COEF: e->cfg.vf_coef = value; break;
    case MOBROB_HYPER_EPOCH_KERNEL: e->epoch_kernel_on = value != 0.0; break;
    default: return fail(MOBROB_ERR_INVALID, "unknown hyper-parameter id %d", which);
  }
  return MOBROB_OK;
}

int mobrob_ppo_last_train_info(const mobrob_ppo_engine_t* e, int32_t* epochs_started, int32_t* stopped_early,
                               int32_t* steps_applied) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  if (epochs_started) *epochs_started = e->last_epochs_started;
  if (stopped_early) *stopped_early = e->last_stopped_early;
  if (steps_applied) *steps_applied = e->last_steps_applied;
  return MOBROB_OK;
}

int mobrob_ppo_fetch_step_stats(mobrob_ppo_engine_t* e, float* out, int32_t max_rows) {
  if (!e || !out || max_rows < 0) return fail(MOBROB_ERR_INVALID, "fetch_step_stats: bad argument");
  const int n = std::min<int>(max_rows, e->stats_n);
  if (n > 0) {
    HIPC(hipMemcpyAsync(out, e->stats + (size_t)(e->stats_n - n) * 8, (size_t)n * 32, hipMemcpyDeviceToHost, e->stream));
  }
  HIPC(hipStreamSynchronize(e->stream));
  e->stats_n = 0;
  CHK(check_async_error(e));
  return n;
}

}  // extern "C"
// ---- data parallel: the whole update loop in C, one RCCL all-reduce per optimizer step on the engine's stream ----
namespace {
struct RcclApi {
  void* lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclCommCount) CommCount = nullptr;
  decltype(&ncclCommUserRank) CommUserRank = nullptr;
};
RcclApi g_rccl;
int rccl_load() {
  if (g_rccl.lib) return MOBROB_OK;
  // by SONAME: a process that already holds RCCL (torch.distributed's "nccl" backend) shares that copy
  void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h) return fail(MOBROB_ERR_STATE, "RCCL not found: %s", dlerror());
#define RSYM(field, name)                                                     \
  g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(h, name));   \
  if (!g_rccl.field) return fail(MOBROB_ERR_STATE, "RCCL symbol %s missing", name);
  RSYM(GetUniqueId, "ncclGetUniqueId")
  RSYM(CommInitRank, "ncclCommInitRank")
  RSYM(CommDestroy, "ncclCommDestroy")
  RSYM(AllReduce, "ncclAllReduce")
  RSYM(GetErrorString, "ncclGetErrorString")
  RSYM(CommCount, "ncclCommCount")
  RSYM(CommUserRank, "ncclCommUserRank")
#undef RSYM
  g_rccl.lib = h;
  return MOBROB_OK;
}
#define NCCLC(expr)                                                                                   \
  do {                                                                                                \
    ncclResult_t _r = (expr);                                                                         \
    if (_r != ncclSuccess) return fail(MOBROB_ERR_HIP, "%s failed: %s", #expr, g_rccl.GetErrorString(_r)); \
  } while (0)

size_t oneshot_payload_bytes(const mobrob_ppo_engine* e) {
  const size_t need = std::max((size_t)(e->P + 8) * sizeof(float), (size_t)e->nmb * 4 * sizeof(double));
  return (need + 255) / 256 * 256;
}
int oneshot_all_reduce(mobrob_ppo_engine* e, void* buf, size_t count, int dtype) {
  auto& o = e->oneshot;
  const size_t bytes = count * (dtype == 1 ? sizeof(double) : sizeof(float));
  if (bytes > o.payload) return fail(MOBROB_ERR_INVALID, "one-shot all-reduce: message of %zu bytes, exchange slot of %zu", bytes, o.payload);
  o.seq++;
  OneShotArgs a{};
  const size_t slot = (size_t)(o.seq & 1) * o.payload;
  a.local = buf; a.mine = o.xbuf + slot; a.my_flags = reinterpret_cast<unsigned long long*>(o.xbuf + 2 * o.payload);
  for (int r = 0; r < o.world; ++r) {
    a.peer[r] = o.peer[r] + slot;
    a.peer_flags[r] = reinterpret_cast<const unsigned long long*>(o.peer[r] + 2 * o.payload);
  }
  a.world = o.world; a.rank = o.rank; a.bytes = bytes; a.seq = o.seq; a.error = o.error; a.timeout_ticks = o.timeout_ticks;
  a.fence_form = env_int("MOBROB_ONESHOT_FENCE", 0) != 0;
  const int chunks = cdiv((int)bytes, kOneShotChunkBytes);
  if (dtype == 1) hipLaunchKernelGGL(k_oneshot_allreduce<double>, dim3(chunks), dim3(256), 0, e->stream, a);
  else hipLaunchKernelGGL(k_oneshot_allreduce<float>, dim3(chunks), dim3(256), 0, e->stream, a);
  HIPC(hipGetLastError());
  return MOBROB_OK;
}
// raised by a one-shot all-reduce whose peer never published (dead rank): reported at the next synchronising call
int check_async_error(mobrob_ppo_engine* e) {
  if (e->epoch_err_host && *(volatile int*)e->epoch_err_host != 0) {
    *(volatile int*)e->epoch_err_host = 0;
    return fail(MOBROB_ERR_STATE, "the co-operative epoch kernel gave up at a grid barrier (a workgroup never arrived: another tenant on the "
                                  "device?); the update of this train() is incomplete -- MOBROB_EPOCH_KERNEL=0 runs the three launches per step");
  }
  if (e->oneshot.error && *(volatile int*)e->oneshot.error != 0) {
    const int v = *(volatile int*)e->oneshot.error;
    *(volatile int*)e->oneshot.error = 0;
    return fail(MOBROB_ERR_STATE, "one-shot all-reduce: a peer rank never published message %d (dead or stalled rank)", v - 1);
  }
  return MOBROB_OK;
}

// sum `count` elements (dtype 0 = f32, 1 = f64) in place across the ranks, ordered on the engine's stream
int dp_all_reduce(mobrob_ppo_engine* e, void* buf, size_t count, int dtype, mobrob_allreduce_fn fn, void* ctx) {
  ProfScope ps(e, MOBROB_K_ALLREDUCE);
  e->allreduce_calls++;
  e->allreduce_bytes += count * (dtype == 1 ? 8 : 4);
  if (fn) {
    const int r = fn(ctx, buf, count, dtype, (void*)e->stream);
    return r == 0 ? MOBROB_OK : fail(MOBROB_ERR_STATE, "all-reduce callback returned %d", r);
  }
  if (e->oneshot.ready) return oneshot_all_reduce(e, buf, count, dtype);
  NCCLC(g_rccl.AllReduce(buf, buf, count, dtype == 1 ? ncclDouble : ncclFloat, ncclSum, e->comm, e->stream));
  return MOBROB_OK;
}
}  // namespace

namespace {
// ---- one co-operative launch per epoch (kernels_epoch64.h) ----
// The norm records (kernels_fused.h: block_norm_records): the reduction kernel leaves per-block (tensor, sum of squares) records and
// k_adam_pack folds them with four wave reductions, so no k_sqnorm_chunks launch.  Never under data parallel: the records are norms of
// the LOCAL gradient, the clip needs those of the summed one.  Never with target_kl (its stop sits between the two).  Asked once per train().
// (Why wave reductions: at 2x256 the table has 712 records; one serial chain per tensor in every k_adam_pack block cost 12.9 instead of 11.4 ms per iteration.)
bool norm_records_wanted(const mobrob_ppo_engine* e, bool dp) {
  return !dp && e->fused.enabled && e->target_kl <= 0.0 && !env_switched_off("MOBROB_NO_NORM_RECORDS");
}
// Eligible: single rank, 64-wide fused engine, every minibatch of the epoch small enough for the split-tile gradient kernel
// (Grad64Plan::split of the largest one), norm records in use (`records`: norm_records_wanted), only the dominant kernel bracketed
// when profiling, grid <= compute units.  *launch (meaningful after `true` only): workgroups of the launch, the reduction's fold group.
struct EpochLaunch { int grid = 0, group = 0; };
bool epoch_kernel_eligible(const mobrob_ppo_engine* e, bool dp, bool records, EpochLaunch* launch) {
  static_assert(kEpochRedBlocks * 256 >= 10 * 1024 + 200 && (kEpochRedBlocks - 1) * 256 < 10 * 1024 + 200, "kEpochRedBlocks = ceil(s64_size() / 256)");
  const FusedState& f = e->fused;
  if (dp || e->cfg.world_size != 1 || !e->epoch_kernel_on || !f.enabled || f.H != GH || e->epoch_bar == nullptr) return false;
  if (e->target_kl > 0.0 || !records || kEpochRedBlocks != cdiv(s64_size(), 256)) return false;
  if (e->prof_on && (e->prof_mask & ((1u << MOBROB_K_GRAD_REDUCE) | (1u << MOBROB_K_APPLY))) != 0) return false;   // --phases: the per-step launches are what gets bracketed
  const Grad64Plan pl = grad64_plan(e, std::min(e->Bl, e->N * e->T));
  if (!pl.split) return false;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->cfg.device_id) != hipSuccess) return false;
  launch->grid = std::max(2 * pl.ntiles, 2 * kEpochRedBlocks); launch->group = pl.group;
  return launch->grid <= cus;
}
constexpr size_t kEpochLdsBytes = 84 * 1024;   // more than half of a CU's 160 KB: one workgroup per CU (the residency the hand-offs were validated in)

int launch_epoch_kernel(mobrob_ppo_engine* e, int ep, const EpochLaunch& launch) {
  if (!e->use_norm_records) return fail(MOBROB_ERR_STATE, "k_epoch64 outside train_loop's norm-record scope");   // the fillers below read the flag
  const int total = e->N * e->T, nmb = e->nmb;
  const size_t slot_bytes = (size_t)nmb * 12;
  if (!e->epoch_stage) {
    HIPC(hipHostMalloc((void**)&e->epoch_stage, slot_bytes * (size_t)std::max(1, e->cfg.n_epochs), hipHostMallocDefault));
    HIPC(hipHostMalloc((void**)&e->epoch_err_host, sizeof(int), hipHostMallocCoherent | hipHostMallocMapped));
    *e->epoch_err_host = 0;
    HIPC(hipEventCreateWithFlags(&e->epoch_ev, hipEventDisableTiming));
  }
  if (ep == 0) HIPC(hipEventSynchronize(e->epoch_ev));   // the previous train()'s staging copies are done (never recorded: returns at once)
  char* slot = e->epoch_stage + slot_bytes * (size_t)(ep % std::max(1, e->cfg.n_epochs));
  float* consts = reinterpret_cast<float*>(slot);
  int* idx = reinterpret_cast<int*>(slot + (size_t)nmb * 8);
  // per-step constants of this epoch: Adam's bias corrections and the statistics rows, advanced as apply_adam / apply_norms advance them
  for (int mb = 0; mb < nmb; ++mb) {
    const AdamStep step = next_adam_step(e);
    consts[2 * mb] = step.step_size; consts[2 * mb + 1] = step.bc2_sqrt;
    idx[mb] = next_stats_row(e);
  }
  HIPC(hipMemcpyAsync(e->epoch_consts, consts, (size_t)nmb * 8, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(e->epoch_idx, idx, (size_t)nmb * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipEventRecord(e->epoch_ev, e->stream));
  HIPC(hipMemsetAsync(e->epoch_bar, 0, 1024 * sizeof(unsigned), e->stream));
  Epoch64Args ea{};   // the three phases take the arguments of the three launches; what varies per minibatch is derived in the kernel
  ea.tr = train64_args(e);
  ea.rd = slab64_reduce_args(e);
  ea.rd.group = launch.group;   // (rec_sum is set: eligibility needs the norm records, and train_loop has switched them on)
  fill_adam_pack_args(e, ea.ad);
  ea.ad.st = stats_args(e);
  ea.ad.loss_sums_zero = e->grads + e->P;
  ea.rows = e->rows; ea.advstat = e->advstat;
  ea.total = total; ea.bl = e->Bl; ea.nmb = nmb; ea.world = e->cfg.world_size;
  ea.step_consts = e->epoch_consts; ea.stats_idx = e->epoch_idx; ea.stats = e->stats;
  ea.barrier = e->epoch_bar; ea.error_host = e->epoch_err_host;
  ea.timeout_ticks = (long long)(env_double("MOBROB_EPOCH_TIMEOUT_S", 10.0) * 1e8);
  void* kargs[1] = {&ea};
  {
    ProfScope ps(e, MOBROB_K_TRAIN_GRAD);   // the whole epoch: gradient, reduction and Adam phases are one launch
    hipError_t le = hipSuccess;
    FUSED_DISPATCH_DP(e->Dp, FUSED64_DISPATCH_NJ(e->A, {
      const void* fn = reinterpret_cast<const void*>(k_epoch64<DPc, NJc>);
      le = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kEpochLdsBytes);
      if (le == hipSuccess) le = hipLaunchCooperativeKernel(fn, dim3(launch.grid), dim3(256), kargs, (unsigned)kEpochLdsBytes, e->stream);
    }));
    if (le != hipSuccess) return fail(MOBROB_ERR_HIP, "k_epoch64 launch (%d workgroups): %s", launch.grid, hipGetErrorString(le));
  }
  e->cur_count = std::min(e->Bl, total - (nmb - 1) * e->Bl);
  e->grad_pending = false;
  e->last_steps_applied += nmb;
  return MOBROB_OK;
}

// PPO.train() [SB3 ppo/ppo.py], single rank (dp == false) or data parallel (dp == true: the advantage statistics are
// all-reduced once per epoch, the gradient TOGETHER WITH the eight loss sums behind it once per optimizer step, so the
// logged statistics and the target_kl decision are those of the union minibatch on every rank alike).
int train_loop(mobrob_ppo_engine* e, const int64_t* perms, bool dp, bool records, mobrob_allreduce_fn fn, void* ctx) {
  if (!dp && e->cfg.world_size != 1)
    return fail(MOBROB_ERR_STATE, "mobrob_ppo_train is the single-rank loop; data-parallel ranks call mobrob_ppo_train_dp "
                                  "(or drive epoch_begin/minibatch_grad/[all-reduce]/minibatch_apply)");
  const size_t total = (size_t)e->N * e->T;
  e->stats_n = 0;
  const bool kl = e->target_kl > 0.0;
  e->last_epochs_started = 0; e->last_stopped_early = 0; e->last_steps_applied = 0;
  struct RecordsOn {  // `records` = norm_records_wanted: nothing can touch the gradient between reduction and clip inside this loop
    mobrob_ppo_engine* e;
    RecordsOn(mobrob_ppo_engine* e_, bool on) : e(e_) { e->use_norm_records = on; }
    ~RecordsOn() { e->use_norm_records = false; }
  } records_on(e, records);
  EpochLaunch epoch_launch;
  const bool epoch_kernel = epoch_kernel_eligible(e, dp, records, &epoch_launch);
  e->last_update_mode = epoch_kernel ? 1 : 0;
  for (int ep = 0; ep < e->cfg.n_epochs; ++ep) {
    CHK(mobrob_ppo_epoch_begin(e, perms ? perms + (size_t)ep * total : nullptr));
    // per-minibatch (sum, sum of squares, count) of the advantages: global statistics for the normalisation
    if (dp) CHK(dp_all_reduce(e, e->advstat, (size_t)e->nmb * 4, 1, fn, ctx));
    e->last_epochs_started = ep + 1;
    if (ep == e->cfg.n_epochs - 1 || kl) e->stats_n = 0;  // the rows kept are those of the last epoch that ran
    if (epoch_kernel) {   // all optimizer steps of the epoch in ONE co-operative launch (kernels_epoch64.h): same arithmetic, same bits
      CHK(launch_epoch_kernel(e, ep, epoch_launch));
      continue;
    }
    for (int mb = 0; mb < e->nmb && !e->last_stopped_early; ++mb) {
      CHK(mobrob_ppo_minibatch_grad(e, mb));
      // THE exchange step, one per optimizer step: [P] gradient + [8] loss sums (policy, value, approx_kl, clip
      // fraction, row count ...) in one message
      if (dp) CHK(dp_all_reduce(e, e->grads, (size_t)e->P + 8, 0, fn, ctx));
      int32_t stopped = 0;  // target_kl [SB3 PPO.train]: this step and everything after it is dropped
      CHK(apply_checked(e, &stopped));
      if (stopped) {
        e->last_stopped_early = 1;
        break;
      }
      e->last_steps_applied++;
    }
    if (e->last_stopped_early) break;
  }
  e->epoch_open = false;
  return MOBROB_OK;
}
// parameters and both Adam moments into epoch_snap ([3][P]), or back (`restore`)
int copy_optimizer_state(mobrob_ppo_engine* e, bool restore) {
  float* const live[3] = {e->params, e->m, e->v};
  for (int i = 0; i < 3; ++i) {
    float* const snap = e->epoch_snap + (size_t)i * e->P;
    HIPC(hipMemcpyAsync(restore ? live[i] : snap, restore ? snap : live[i], (size_t)e->P * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
  }
  return MOBROB_OK;
}
}  // namespace

extern "C" {

int mobrob_ppo_train_enqueue(mobrob_ppo_engine_t* e, const int64_t* perms) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  return train_loop(e, perms, false, norm_records_wanted(e, false), nullptr, nullptr);
}

int mobrob_ppo_comm_unique_id(uint8_t* out128) {
  if (!out128) return fail(MOBROB_ERR_INVALID, "comm_unique_id: null argument");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  CHK(rccl_load());
  ncclUniqueId id;
  NCCLC(g_rccl.GetUniqueId(&id));
  memcpy(out128, &id, sizeof id);
  return MOBROB_OK;
}
int mobrob_ppo_comm_prepare(mobrob_ppo_engine_t* e) {
  if (!e) return fail(MOBROB_ERR_INVALID, "comm_prepare: null engine");
  if (e->comm) return fail(MOBROB_ERR_STATE, "comm_prepare: the engine already has a communicator");
  CHK(rccl_load());
  HIPC(hipSetDevice(e->cfg.device_id));
  return MOBROB_OK;
}
int mobrob_ppo_comm_init_rank(mobrob_ppo_engine_t* e, const uint8_t* id128, int32_t rank, int32_t nranks) {
  if (!e || !id128) return fail(MOBROB_ERR_INVALID, "comm_init: null argument");
  if (nranks != e->cfg.world_size)
    return fail(MOBROB_ERR_INVALID, "comm_init: %d ranks, but the engine splits its minibatch for world_size %d", nranks, e->cfg.world_size);
  if (rank < 0 || rank >= nranks) return fail(MOBROB_ERR_INVALID, "comm_init: rank %d of %d", rank, nranks);
  CHK(mobrob_ppo_comm_prepare(e));
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  NCCLC(g_rccl.CommInitRank(&e->comm, nranks, id, rank));
  return MOBROB_OK;
}
int mobrob_ppo_comm_init(mobrob_ppo_engine_t* e, const uint8_t* id128) {
  if (!e) return fail(MOBROB_ERR_INVALID, "comm_init: null argument");
  return mobrob_ppo_comm_init_rank(e, id128, e->cfg.rank, e->cfg.world_size);
}
int mobrob_ppo_comm_info(mobrob_ppo_engine_t* e, int32_t* nranks, int32_t* rank) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  int n = 0, r = -1;
  if (e->comm) {
    NCCLC(g_rccl.CommCount(e->comm, &n));
    NCCLC(g_rccl.CommUserRank(e->comm, &r));
  }
  if (nranks) *nranks = n;
  if (rank) *rank = r;
  return MOBROB_OK;
}
int mobrob_ppo_comm_destroy(mobrob_ppo_engine_t* e) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  if (e->comm) {
    (void)hipStreamSynchronize(e->stream);
    (void)g_rccl.CommDestroy(e->comm);
    e->comm = nullptr;
  }
  return MOBROB_OK;
}
int mobrob_ppo_oneshot_export(mobrob_ppo_engine_t* e, uint8_t* handle64) {
  if (!e || !handle64) return fail(MOBROB_ERR_INVALID, "oneshot_export: null argument");
  static_assert(sizeof(hipIpcMemHandle_t) == MOBROB_IPC_HANDLE_BYTES, "hipIpcMemHandle_t is 64 bytes");
  auto& o = e->oneshot;
  HIPC(hipSetDevice(e->cfg.device_id));
  if (!o.xbuf) {
    o.payload = oneshot_payload_bytes(e);
    if (cdiv((int)o.payload, kOneShotChunkBytes) > kOneShotMaxChunks)
      return fail(MOBROB_ERR_INVALID, "one-shot all-reduce: a %zu-byte message needs more than %d chunks", o.payload, kOneShotMaxChunks);
    const size_t total = 2 * o.payload + kOneShotMaxChunks * sizeof(unsigned long long);
    HIPC(hipMalloc((void**)&o.xbuf, total));
    // flags = 0 < every sequence number, complete before a peer can hold the handle: ordered on the engine's stream and waited for
    // (hipMemset on device memory is neither guaranteed host-synchronous nor ordered against a non-blocking stream)
    HIPC(hipMemsetAsync(o.xbuf, 0, total, e->stream));
    HIPC(hipStreamSynchronize(e->stream));
    HIPC(hipHostMalloc((void**)&o.error, sizeof(int), hipHostMallocDefault));
    *o.error = 0;
    const char* t = getenv("MOBROB_ONESHOT_TIMEOUT_MS");
    o.timeout_ticks = (long long)(t ? atoll(t) : 20000) * 100000;  // wall_clock64 counts at 100 MHz
  }
  hipIpcMemHandle_t h;
  HIPC(hipIpcGetMemHandle(&h, o.xbuf));
  memcpy(handle64, &h, sizeof h);
  return MOBROB_OK;
}
int mobrob_ppo_oneshot_open(mobrob_ppo_engine_t* e, const uint8_t* handles, int32_t rank, int32_t nranks) {
  if (!e || !handles) return fail(MOBROB_ERR_INVALID, "oneshot_open: null argument");
  auto& o = e->oneshot;
  if (!o.xbuf) return fail(MOBROB_ERR_STATE, "oneshot_open before oneshot_export");
  if (o.ready) return fail(MOBROB_ERR_STATE, "oneshot_open: the exchange is already open");
  if (nranks != e->cfg.world_size || nranks > kOneShotMaxRanks || rank < 0 || rank >= nranks)
    return fail(MOBROB_ERR_INVALID, "oneshot_open: rank %d of %d (engine world_size %d, at most %d ranks)", rank, nranks, e->cfg.world_size, kOneShotMaxRanks);
  HIPC(hipSetDevice(e->cfg.device_id));
  for (int r = 0; r < nranks; ++r) {
    if (r == rank) { o.peer[r] = o.xbuf; continue; }
    hipIpcMemHandle_t h;
    memcpy(&h, handles + (size_t)r * MOBROB_IPC_HANDLE_BYTES, sizeof h);
    void* p = nullptr;
    hipError_t er = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
    if (er != hipSuccess) {
      (void)hipGetLastError();
      for (int q = 0; q < r; ++q)
        if (q != rank && o.peer[q]) { (void)hipIpcCloseMemHandle(o.peer[q]); o.peer[q] = nullptr; }
      return fail(MOBROB_ERR_HIP, "hipIpcOpenMemHandle(rank %d): %s", r, hipGetErrorString(er));
    }
    o.peer[r] = static_cast<char*>(p);
  }
  o.world = nranks; o.rank = rank; o.seq = 0; o.ready = true;
  return MOBROB_OK;
}
int mobrob_ppo_oneshot_close(mobrob_ppo_engine_t* e) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  auto& o = e->oneshot;
  if (!o.xbuf) return MOBROB_OK;
  (void)hipStreamSynchronize(e->stream);
  for (int r = 0; r < o.world; ++r)
    if (r != o.rank && o.peer[r]) (void)hipIpcCloseMemHandle(o.peer[r]);
  (void)hipFree(o.xbuf);
  (void)hipHostFree(o.error);
  o = mobrob_ppo_engine::OneShot{};
  return MOBROB_OK;
}
int mobrob_ppo_train_dp(mobrob_ppo_engine_t* e, const int64_t* perms, mobrob_allreduce_fn fn, void* ctx) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  if (!fn && !e->comm && !e->oneshot.ready)
    return fail(MOBROB_ERR_STATE, "train_dp: no communicator (mobrob_ppo_comm_init), no one-shot exchange (mobrob_ppo_oneshot_open) and no all-reduce callback");
  CHK(train_loop(e, perms, true, norm_records_wanted(e, true), fn, ctx));
  if (!fn && e->oneshot.ready) {
    // A one-shot message whose peer never published leaves this rank's gradient LOCAL: such a step must not pass as a data-parallel
    // one.  The update is awaited here and the error word turned into a failure of this call (the caller ends the job).
    HIPC(hipStreamSynchronize(e->stream));
    CHK(check_async_error(e));
  }
  return MOBROB_OK;
}

extern "C++" {   // templates: C++ linkage inside the C-ABI block
namespace {
// exchange self-check (mobrob_ppo_exchange_selfcheck): small integers -- every partial sum is exact in float32 (and float64) whatever
// the order; `salt` makes every message of a check a different vector
template <typename T>
__device__ __forceinline__ T selfcheck_value(unsigned i, int rank, unsigned salt) {
  const unsigned hsh = ((i + 0x51ED27u * salt) * 2654435761u + (unsigned)(rank + 1) * 0x9E3779B9u) >> 20;
  return (T)((int)(hsh & 0xFFFu) - 2048);
}
template <typename T>
__global__ void k_selfcheck_fill(T* buf, int n, int rank, unsigned salt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) buf[i] = selfcheck_value<T>((unsigned)i, rank, salt);
}
template <typename T>
__global__ void k_selfcheck_compare(const T* buf, int n, int world, unsigned salt, int* mismatches) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  T want = 0;
  for (int r = 0; r < world; ++r) want += selfcheck_value<T>((unsigned)i, r, salt);   // rank order; exact anyway
  if (!(buf[i] == want)) atomicAdd(mismatches, 1);
}
}  // namespace
}  // extern "C++"

// Known vectors through the exchange train_dp would use, compared with the rank-ordered sums -- at communicator set-up, before any
// gradient depends on it.  which: 0 = the engine's RCCL communicator, 1 = the one-shot exchange.  Collective over the ranks.
// The update loop sends two kinds of message -- the [P + 8] float gradient message per optimizer step and the [n_minibatches][4]
// float64 advantage sums per epoch -- and the one-shot exchange alternates between two payload slots: the check sends TWO messages
// of EACH kind (both slots, slot reuse, both element types).  It runs on a scratch buffer of its own, so the gradient vector and
// the loss accumulators behind it are never touched; it is refused while an epoch is open or a gradient awaits its apply.
// *mismatches = elements (over the four messages) that are not bit-equal to the expected sum (0 = the exchange is sound).
int mobrob_ppo_exchange_selfcheck(mobrob_ppo_engine_t* e, int32_t which, int32_t* mismatches) {
  if (!e || !mismatches) return fail(MOBROB_ERR_INVALID, "exchange_selfcheck: null argument");
  *mismatches = -1;
  if (e->epoch_open || e->grad_pending)
    return fail(MOBROB_ERR_STATE, "exchange_selfcheck: an epoch is open or a gradient is pending (call it between updates)");
  int world = 0, rank = -1;
  if (which == 0) {
    if (!e->comm) return fail(MOBROB_ERR_STATE, "exchange_selfcheck: no RCCL communicator");
    NCCLC(g_rccl.CommCount(e->comm, &world));
    NCCLC(g_rccl.CommUserRank(e->comm, &rank));
  } else if (which == 1) {
    if (!e->oneshot.ready) return fail(MOBROB_ERR_STATE, "exchange_selfcheck: the one-shot exchange is not open");
    world = e->oneshot.world; rank = e->oneshot.rank;
  } else {
    return fail(MOBROB_ERR_INVALID, "exchange_selfcheck: which = %d", which);
  }
  const int nf = e->P + 8, nd = e->nmb * 4;
  char* scratch = nullptr;
  int* bad = nullptr;
  const size_t sbytes = std::max((size_t)nf * sizeof(float), (size_t)nd * sizeof(double));
  HIPC(hipMalloc((void**)&scratch, sbytes + 256));
  if (hipMalloc((void**)&bad, sizeof(int)) != hipSuccess) { (void)hipFree(scratch); return fail(MOBROB_ERR_HIP, "exchange_selfcheck: hipMalloc"); }
  (void)hipMemsetAsync(bad, 0, sizeof(int), e->stream);
  int rc = MOBROB_OK;
  for (unsigned msg = 0; msg < 4 && rc == MOBROB_OK; ++msg) {   // float, float, double, double
    const int dtype = msg >> 1, n = dtype ? nd : nf;
    if (dtype) hipLaunchKernelGGL(k_selfcheck_fill<double>, dim3(cdiv(n, 256)), dim3(256), 0, e->stream, reinterpret_cast<double*>(scratch), n, rank, msg);
    else hipLaunchKernelGGL(k_selfcheck_fill<float>, dim3(cdiv(n, 256)), dim3(256), 0, e->stream, reinterpret_cast<float*>(scratch), n, rank, msg);
    if (which == 1) rc = oneshot_all_reduce(e, scratch, (size_t)n, dtype);
    else if (g_rccl.AllReduce(scratch, scratch, (size_t)n, dtype ? ncclDouble : ncclFloat, ncclSum, e->comm, e->stream) != ncclSuccess)
      rc = fail(MOBROB_ERR_HIP, "exchange_selfcheck: ncclAllReduce failed");
    if (rc != MOBROB_OK) break;
    if (dtype) hipLaunchKernelGGL(k_selfcheck_compare<double>, dim3(cdiv(n, 256)), dim3(256), 0, e->stream, reinterpret_cast<const double*>(scratch), n, world, msg, bad);
    else hipLaunchKernelGGL(k_selfcheck_compare<float>, dim3(cdiv(n, 256)), dim3(256), 0, e->stream, reinterpret_cast<const float*>(scratch), n, world, msg, bad);
  }
  if (rc == MOBROB_OK) {
    int h = -1;
    hipError_t er = hipMemcpyAsync(&h, bad, sizeof(int), hipMemcpyDeviceToHost, e->stream);
    if (er == hipSuccess) er = hipStreamSynchronize(e->stream);
    if (er != hipSuccess) rc = fail(MOBROB_ERR_HIP, "exchange_selfcheck: %s", hipGetErrorString(er));
    else *mismatches = h;
  }
  (void)hipStreamSynchronize(e->stream);
  (void)hipFree(bad);
  (void)hipFree(scratch);
  if (rc != MOBROB_OK) return rc;
  // a peer that never published raised the error word: reported here, and LEFT SET for the closing path only if the caller ignores
  // this return value -- check_async_error clears it once it has been turned into a failure
  if (which == 1) CHK(check_async_error(e));
  return MOBROB_OK;
}
int mobrob_ppo_allreduce_counters(mobrob_ppo_engine_t* e, int64_t* calls, int64_t* bytes, int32_t reset) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  if (calls) *calls = e->allreduce_calls;
  if (bytes) *bytes = e->allreduce_bytes;
  if (reset) { e->allreduce_calls = 0; e->allreduce_bytes = 0; }
  return MOBROB_OK;
}

int mobrob_ppo_train(mobrob_ppo_engine_t* e, const int64_t* perms, mobrob_ppo_train_stats_t* st) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  // An update that will run its epochs as co-operative launches (k_epoch64) is taken from a SNAPSHOT of the optimizer's state: should a
  // launch give up at a grid barrier (a workgroup that never became resident: more spinning tenants on the device than it has room for),
  // the state is restored and the whole update runs again as three launches per step -- the same bits, never a failed or half-applied
  // train().  The engine then keeps the three launches (mobrob_ppo_update_mode reports it).  (mobrob_ppo_train_enqueue has no such
  // retry: it returns before the outcome is known; there the abort fails the next synchronising call.)
  const bool records = norm_records_wanted(e, false);
  EpochLaunch launch_unused;
  const bool snap = e->cfg.world_size == 1 && e->epoch_snap != nullptr && epoch_kernel_eligible(e, false, records, &launch_unused);
  const int64_t adam_step0 = e->adam_step; const uint64_t perm_counter0 = e->perm_counter;
  if (snap) CHK(copy_optimizer_state(e, false));
  CHK(train_loop(e, perms, false, records, nullptr, nullptr));
  if (snap && (e->last_update_mode & 1)) {
    HIPC(hipStreamSynchronize(e->stream));
    if (e->epoch_err_host && *(volatile int*)e->epoch_err_host != 0) {
      *(volatile int*)e->epoch_err_host = 0;
      fprintf(stderr, "[mobrob_ppo] the co-operative epoch kernel gave up at a grid barrier (workgroups not resident together: other spinning tenants "
                      "on the device?); the update is re-run as three launches per optimizer step and this engine keeps that form\n");
      CHK(copy_optimizer_state(e, true));
      HIPC(hipMemsetAsync(e->grads + e->P, 0, 8 * sizeof(float), e->stream));
      repack(e);   // every weight pack from the restored parameters
      e->adam_step = adam_step0; e->perm_counter = perm_counter0;   // (the same permutations again; the parity of the max-|adv| words simply goes on)
      e->epoch_kernel_on = false;
      CHK(train_loop(e, perms, false, records, nullptr, nullptr));
    }
  }
  if (st) {
    std::vector<float> rows((size_t)e->nmb * 8);
    const int n = mobrob_ppo_fetch_step_stats(e, rows.data(), e->nmb);
    if (n < 0) return n;
    double acc[7] = {0};
    int n_norm = 0;  // a step dropped by target_kl logs its losses but has no gradient norm (NaN)
    for (int i = 0; i < n; ++i) {
      for (int k = 0; k < 6; ++k) acc[k] += rows[(size_t)i * 8 + k];
      if (!std::isnan(rows[(size_t)i * 8 + 6])) { acc[6] += rows[(size_t)i * 8 + 6]; n_norm++; }
    }
    const double d = n > 0 ? n : 1;
    st->policy_loss = (float)(acc[0] / d); st->value_loss = (float)(acc[1] / d); st->entropy_loss = (float)(acc[2] / d);
    st->loss = (float)(acc[3] / d); st->approx_kl = (float)(acc[4] / d); st->clip_fraction = (float)(acc[5] / d);
    st->grad_norm = (float)(acc[6] / (n_norm > 0 ? n_norm : 1)); st->n_minibatches = e->last_steps_applied;
  } else {
    HIPC(hipStreamSynchronize(e->stream));
  }
  return MOBROB_OK;
}

// ---- inference --------------------------------------------------------------------------------------
int mobrob_ppo_predict(mobrob_ppo_engine_t* e, const float* obs, int32_t n, int32_t deterministic, const float* eps,
                       float* actions, float* values) {
  if (!e || !obs || n < 1) return fail(MOBROB_ERR_INVALID, "predict: bad argument");
  for (int s = 0; s < n; s += e->rows_max) {
    const int c = std::min(e->rows_max, n - s);
    CHK(upload_obs(e, obs + (size_t)s * e->D, e->pred_obs, c));
    forward(e, e->pred_obs, c, actions != nullptr, e->mu, values != nullptr, e->vout);
    if (actions) {
      float* scratch = e->pred_act;
      if (deterministic) {
        hipLaunchKernelGGL(k_clip_mean, dim3(cdiv(c * e->A, 256)), dim3(256), 0, e->stream, e->mu, e->Ap, c, e->A,
                           (float)e->cfg.action_low, (float)e->cfg.action_high, scratch);
      } else {
        if (e->sde) {   // get_noise: the environments' own matrices for a batch of n_envs rows, else the single exploration_mat
          const bool own = n == e->N;
          sde_variance(e, c, true);
          hipLaunchKernelGGL(k_sample_sde, dim3(cdiv(c, 4)), dim3(256), 0, e->stream, e->mu, e->Ap, e->hp[e->Lp - 1], e->HL, e->sde_var, e->Ap,
                             own ? e->sde_E : e->sde_E1, s, own ? 0 : 1, c, e->HL, e->A, (float)e->cfg.action_low, (float)e->cfg.action_high,
                             (float*)nullptr, scratch, (float*)nullptr);
          HIPC(hipMemcpyAsync(actions + (size_t)s * e->A, scratch, (size_t)c * e->A * 4, hipMemcpyDeviceToHost, e->stream));
          if (values) HIPC(hipMemcpyAsync(values + s, e->vout, (size_t)c * 4, hipMemcpyDeviceToHost, e->stream));
          HIPC(hipStreamSynchronize(e->stream));
          continue;
        }
        const float* epsd = nullptr;
        if (eps) {
          HIPC(hipMemcpyAsync(e->eps_dev, eps + (size_t)s * e->A, (size_t)c * e->A * 4, hipMemcpyHostToDevice, e->stream));
          epsd = e->eps_dev;
        }
        hipLaunchKernelGGL(k_sample, dim3(cdiv(c, 256)), dim3(256), 0, e->stream, e->mu, e->Ap, Pp(e, T_LOGSTD), epsd,
                           c, e->A, (float)e->cfg.action_low, (float)e->cfg.action_high, eps_seed(e), e->draw_counter,
                           (const uint32_t*)nullptr, (float*)nullptr, scratch, (float*)nullptr);
        e->draw_counter++;
      }
      HIPC(hipMemcpyAsync(actions + (size_t)s * e->A, scratch, (size_t)c * e->A * 4, hipMemcpyDeviceToHost, e->stream));
    }
    if (values) HIPC(hipMemcpyAsync(values + s, e->vout, (size_t)c * 4, hipMemcpyDeviceToHost, e->stream));
    HIPC(hipStreamSynchronize(e->stream));
  }
  return MOBROB_OK;
}

// ---- policy evaluation: evaluate_policy / examples/control.py on the device ---------------------------------------------
// the evaluation's device buffer (evaluate and follow_waypoints): grown to `need` bytes, outside the arena, freed by destroy
static int grow_eval_buf(mobrob_ppo_engine_t* e, size_t need) {
  if (need > e->eval_bytes) {
    HIPC(hipStreamSynchronize(e->stream));
    if (e->eval_buf) HIPC(hipFree(e->eval_buf));
    e->eval_buf = nullptr;
    e->eval_bytes = 0;
    HIPC(hipMalloc(reinterpret_cast<void**>(&e->eval_buf), need));
    e->eval_bytes = need;
  }
  return MOBROB_OK;
}

static GoalEnvParams eval_env_params(const mobrob_goal_env_t* env, int A, bool terminate_on_goal, int time_limit) {
  GoalEnvParams g{};
  g.P = env->pos_dim; g.terminate_on_goal = terminate_on_goal; g.time_limit = time_limit;
  g.dt = env->dt; g.extent = env->extent; g.reach = env->reach_radius; g.bonus = env->goal_bonus;
  g.extra_bonus = env->extra_bonus; g.noise = env->obs_noise;
  for (int j = 0; j < 3; ++j)
    for (int k = 0; k < 32; ++k) g.mix[j][k] = (j < env->pos_dim && k < A) ? env->mix[j][k] : 0.f;
  return g;
}

extern "C++" {   // templates: C++ linkage inside the C-ABI block
// what evaluate and follow_waypoints take alike from their specs; `who` prefixes their error messages
struct EvalCall {
  const char* who;
  int N, max_steps, deterministic;
  uint64_t seed;
  int trace_robots, trace_steps;
  float* trace_out;
  int trace_extra = 0;        // columns a wrapping task adds to each trace row (hazards: 2)
  bool tracing() const { return trace_out && trace_robots > 0 && trace_steps > 0; }
  size_t trace_floats() const { return (size_t)trace_steps * trace_robots; }
};

// the checks both entry points make, in two groups (evaluate has checks of its own between them)
static int eval_check_dims(const mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const char* who) {
  if (env->pos_dim < 1 || env->pos_dim > 3 || 3 * env->pos_dim > e->D)
    return fail(MOBROB_ERR_INVALID, "%s: pos_dim must be 1..3 and 3*pos_dim <= obs_dim", who);
  if (e->A > 32) return fail(MOBROB_ERR_INVALID, "%s: act_dim must be <= 32", who);
  return MOBROB_OK;
}
static int eval_check_actions_trace(const mobrob_ppo_engine_t* e, const EvalCall& c) {
  if (!c.deterministic && e->sde)
    return fail(MOBROB_ERR_INVALID, "%s: stochastic actions of a use_sde policy are not supported (deterministic only)", c.who);
  if (c.tracing() && (c.trace_robots > c.N || c.trace_steps > c.max_steps))
    return fail(MOBROB_ERR_INVALID, "%s: trace_robots <= n_robots and trace_steps <= max_steps", c.who);
  return MOBROB_OK;
}

// eval_buf's regions, described once: add() every region while sizing, at() the same offsets once the buffer is grown
struct EvalCarve {
  size_t total = 0;
  size_t add(size_t bytes) {
    const size_t off = total;
    total += (bytes + 255) / 256 * 256;
    return off;
  }
};
template <class T>
static T* eval_at(const mobrob_ppo_engine_t* e, size_t off) { return reinterpret_cast<T*>(e->eval_buf + off); }

// The common part of a call: adds the shared regions (robot_out, trace, st, obs, mu) to the task's own in `carve`, grows eval_buf
// (outside the arena: device_bytes / create_in_arena are unchanged), fills the fields of `a` that do not depend on the task and
// zeroes the trace.
static int eval_prepare(mobrob_ppo_engine_t* e, const EvalCall& c, const GoalEnvParams& p, EvalCarve& carve, EvalArgs& a) {
  const int N = c.N, Dp = e->Dp, Ap = e->Ap;
  const bool tracing = c.tracing();
  const size_t n_tr = tracing ? c.trace_floats() * (9 + e->D + e->A + kEvalTraceFlags + c.trace_extra) : 1;
  const size_t o_out = carve.add((size_t)N * 4 * 8), o_tr = carve.add(n_tr * 4), o_st = carve.add((size_t)N * kGoalStateFloats * 4),
               o_obs = carve.add((size_t)cdiv(N, 256) * 256 * Dp * 4), o_mu = carve.add((size_t)cdiv(N, 256) * 256 * Ap * 4);   // whole 256-row tiles
  if (const int rc = grow_eval_buf(e, carve.total)) return rc;
  a.robot_out = eval_at<double>(e, o_out);
  a.st = eval_at<float>(e, o_st);
  a.obs = eval_at<float>(e, o_obs);
  a.mu = eval_at<float>(e, o_mu);
  a.trace = tracing ? eval_at<float>(e, o_tr) : nullptr;
  a.trace_robots = tracing ? c.trace_robots : 0;
  a.trace_steps = tracing ? c.trace_steps : 0;
  a.p = p;
  a.N = N; a.D = e->D; a.Dp = Dp; a.A = e->A; a.Ap = Ap;
  a.deterministic = c.deterministic != 0;
  a.max_steps = c.max_steps;
  a.lo = (float)e->cfg.action_low; a.hi = (float)e->cfg.action_high;
  const uint64_t key = c.seed ^ kEvalKeyMix;
  a.k0 = (uint32_t)key; a.k1 = (uint32_t)(key >> 32);
  a.log_std = Pp(e, T_LOGSTD);
  if (tracing) HIPC(hipMemsetAsync(a.trace, 0, n_tr * 4, e->stream));
  return MOBROB_OK;
}

// The DP instance of k_goal64_tile a task runs at observation width Dp -- the one rule for the launch (eval_run) and for the LDS
// check made before it (follow_waypoints).  Tasks with solid walls never run the 16-wide tile: the 32-wide one serves 16-wide
// observations too (features beyond D are zero in the observation tile and in W1's fragment: the same sums).  Their 16-wide instance
// came out of the compiler with a 20-byte private segment that no instruction touches -- not understood --, which the build's
// audit refuses, so it is not instantiated.
static int eval_tile_width(int Dp, bool solid) { return solid ? std::max(Dp, 32) : Dp; }

// Runs the task for a.max_steps steps: k_goal64_tile on 2x64 tanh engines of the fused family (returns 1), else the per-step path
// (returns 0): the engine's forward() in rows_max chunks + the step kernel per step, then the task's `fin` kernel if it has one.
template <class Task>
static int eval_run(mobrob_ppo_engine_t* e, const typename Task::Args& args, void (*fin)(typename Task::Args)) {
  const EvalArgs& a = Task::eval(args);
  const int N = a.N;
  // MOBROB_EVAL_PERSISTENT=0: the per-step path on every engine (A/B, tests); read per call
  const bool persistent = e->fused.enabled && e->fused.H == 64 && env_int("MOBROB_EVAL_PERSISTENT", 1) != 0;
  // k_goal256_tile (kernels_eval256.h): fused 2x256 tanh engines, and only when switched on.  The non-wide tasks ...
  bool tile256 = false;
  if constexpr (task_tile256<Task>)
    tile256 = e->fused.enabled && e->fused.H == FH && env_int("MOBROB_EVAL_PERSISTENT", 1) != 0 &&
              (e->eval_tile256 >= 0 ? e->eval_tile256 != 0 : env_int("MOBROB_EVAL_TILE256", 0) != 0);
  // ... and the wide tasks of task_tile256_wide (hazards), when the wide switch is in force as well and the task's LDS region
  // fits behind the tile's; a call that does not fit takes the per-step path, as every such call did before
  if constexpr (task_tile256_wide<Task>) {
    if (e->fused.enabled && e->fused.H == FH && env_int("MOBROB_EVAL_PERSISTENT", 1) != 0 &&
        (e->eval_tile256 >= 0 ? e->eval_tile256 != 0 : env_int("MOBROB_EVAL_TILE256", 0) != 0) &&
        (e->eval_tile256_wide >= 0 ? e->eval_tile256_wide != 0 : env_int("MOBROB_EVAL_TILE256_WIDE", 0) != 0)) {
      int limit = 0;
      if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, e->cfg.device_id) != hipSuccess) limit = 64 * 1024;
      tile256 = eval256_lds_bytes() + Task::tile_lds_bytes(args) <= (size_t)limit;
    }
  }
  if (tile256) {
    if constexpr (task_tile256_wide<Task>) {
      const size_t lds_bytes = eval256_lds_bytes() + Task::tile_lds_bytes(args);
      HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_goal256_tile<Task>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
      const Eval64Net W{Pp(e, e->tPW[0]), Pp(e, e->tPB[0]), Pp(e, e->tPW[1]), Pp(e, e->tPB[1]), Pp(e, T_AW), Pp(e, T_AB)};
      hipLaunchKernelGGL(k_goal256_tile<Task>, dim3(cdiv(N, 16)), dim3(256), lds_bytes, e->stream, args, W);
    }
    if constexpr (task_tile256<Task>) {
      const size_t lds_bytes = eval256_lds_bytes();
      int limit = 0;
      if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, e->cfg.device_id) != hipSuccess) limit = 64 * 1024;
      if (lds_bytes > (size_t)limit)
        return fail(MOBROB_ERR_INVALID, "eval tile256: k_goal256_tile needs %zu bytes of LDS, the device allows %d per workgroup (switch it off: mobrob_ppo_set_eval_tile256)",
                    lds_bytes, limit);
      HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_goal256_tile<Task>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
      const Eval64Net W{Pp(e, e->tPW[0]), Pp(e, e->tPB[0]), Pp(e, e->tPW[1]), Pp(e, e->tPB[1]), Pp(e, T_AW), Pp(e, T_AB)};
      hipLaunchKernelGGL(k_goal256_tile<Task>, dim3(cdiv(N, 16)), dim3(256), lds_bytes, e->stream, args, W);
    }
  } else if (persistent) {
    Eval64Net W{Pp(e, e->tPW[0]), Pp(e, e->tPB[0]), Pp(e, e->tPW[1]), Pp(e, e->tPB[1]), Pp(e, T_AW), Pp(e, T_AB)};
    if constexpr (task_solid<Task>) {
      const int Dt = eval_tile_width(a.Dp, true);   // never 16
      const size_t lds_bytes = eval64_lds_bytes(Dt) + Task::tile_lds_bytes(args);
      if (Dt == 32) hipLaunchKernelGGL((k_goal64_tile<32, Task>), dim3(cdiv(N, 16)), dim3(64), lds_bytes, e->stream, args, W);
      else if (Dt == 48) hipLaunchKernelGGL((k_goal64_tile<48, Task>), dim3(cdiv(N, 16)), dim3(64), lds_bytes, e->stream, args, W);
      else hipLaunchKernelGGL((k_goal64_tile<64, Task>), dim3(cdiv(N, 16)), dim3(64), lds_bytes, e->stream, args, W);
    } else {
      size_t lds_bytes = eval64_lds_bytes(a.Dp);
      if constexpr (Task::kWide) lds_bytes += Task::tile_lds_bytes(args);
      FUSED_DISPATCH_DP(a.Dp, hipLaunchKernelGGL((k_goal64_tile<DPc, Task>), dim3(cdiv(N, 16)), dim3(64), lds_bytes, e->stream, args, W));
    }
  } else {
    hipLaunchKernelGGL(k_goal_task_init<Task>, dim3(cdiv(N, 256)), dim3(256), 0, e->stream, args);
    for (int t = 0; t < a.max_steps; ++t) {
      for (int s = 0; s < N; s += e->rows_max) {
        const int c = std::min(e->rows_max, N - s);
        forward(e, a.obs + (size_t)s * a.Dp, c, true, a.mu + (size_t)s * a.Ap, false, nullptr);
      }
      hipLaunchKernelGGL(k_goal_task_step<Task>, dim3(cdiv(N, 256)), dim3(256), 256 * 33 * sizeof(float), e->stream, args, t);
      if constexpr (task_teams<Task>)   // the team check needs every mate's post-step position: a launch of its own
        hipLaunchKernelGGL(k_team_step<typename Task::TeamBase>, dim3(cdiv(N, 256)), dim3(256), 0, e->stream, args, t);
    }
    if (fin) hipLaunchKernelGGL(fin, dim3(cdiv(N, 256)), dim3(256), 0, e->stream, args);
  }
  HIPC(hipGetLastError());
  return persistent || tile256 ? 1 : 0;
}

// robot_out and the trace back to the caller; returns `ran` (eval_run's) once everything enqueued on the stream is done
static int eval_copy_back(mobrob_ppo_engine_t* e, const EvalCall& c, const EvalArgs& a, double* robot_out, int ran) {
  HIPC(hipMemcpyAsync(robot_out, a.robot_out, (size_t)a.N * 4 * 8, hipMemcpyDeviceToHost, e->stream));
  if (a.trace)
    HIPC(hipMemcpyAsync(c.trace_out, a.trace, c.trace_floats() * (9 + a.D + a.A + kEvalTraceFlags + c.trace_extra) * 4,
                        hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  return ran;
}

// ---- hazards (the *_hazards entry points): checks, regions of eval_buf, upload ----
struct HazardIO {
  const mobrob_hazards_t* hz;
  double* hazard_out;         // [N][4]
  double* episode_cost_out;   // [N][max quota] or null (evaluate)
  // the *_hazard_frames entry points: hz->hazards is [S][F][M][3].  frames = 0: a static scene, its own single frame
  int frames = 0, F = 1, frame_steps = 1, loop = 0;
};
// the static fields of a mobrob_hazard_frames_t as a mobrob_hazards_t, and its time axis
static HazardIO hazard_frames_io(const mobrob_hazard_frames_t* hf, mobrob_hazards_t& view, double* hazard_out, double* episode_cost_out) {
  view = mobrob_hazards_t{hf->n_scenes, hf->max_hazards, hf->hazards, hf->n_hazards, hf->scene, hf->cost, hf->indicator};
  return HazardIO{&view, hazard_out, episode_cost_out, 1, hf->n_frames, hf->frame_steps, hf->loop != 0};
}
struct HazardCarve {
  size_t hz, nhz, scene, out, acc;
  std::vector<int32_t> counts;   // [S], n_hazards or M each
};
static int hazard_check(const HazardIO& hio, int N, const char* who, std::vector<int32_t>& counts) {
  const mobrob_hazards_t* hz = hio.hz;
  const int S = hz->n_scenes, M = hz->max_hazards, F = hio.F;
  if (S < 1) return fail(MOBROB_ERR_INVALID, "%s: hazards: n_scenes must be >= 1", who);
  if (M < 0 || M > kHazardMax) return fail(MOBROB_ERR_INVALID, "%s: hazards: max_hazards must lie in 0 .. %d", who, kHazardMax);
  if (hio.frames) {
    if (F < 1) return fail(MOBROB_ERR_INVALID, "%s: hazard frames: n_frames must be >= 1", who);
    if (hio.frame_steps < 1) return fail(MOBROB_ERR_INVALID, "%s: hazard frames: frame_steps must be >= 1", who);
    if ((uint64_t)S * (uint64_t)F * (uint64_t)M * 12u > MOBROB_HAZARD_FRAMES_MAX_BYTES)
      return fail(MOBROB_ERR_INVALID, "%s: hazard frames: %d scenes x %d frames x %d hazards x 12 bytes exceed the cap of %u bytes (64 MiB)",
                  who, S, F, M, (unsigned)MOBROB_HAZARD_FRAMES_MAX_BYTES);
  }
  if (M > 0 && !hz->hazards) return fail(MOBROB_ERR_INVALID, "%s: hazards: null hazard table", who);
  if (!hz->scene && S > 1) return fail(MOBROB_ERR_INVALID, "%s: hazards: %d scenes need a scene index per robot", who, S);
  if (!(std::isfinite(hz->cost) && hz->cost >= 0.f)) return fail(MOBROB_ERR_INVALID, "%s: hazards: cost must be finite and >= 0", who);
  counts.assign(S, M);
  for (int s = 0; s < S; ++s) {
    if (hz->n_hazards) counts[s] = hz->n_hazards[s];
    if (counts[s] < 0 || counts[s] > M)
      return fail(MOBROB_ERR_INVALID, "%s: hazards: n_hazards[%d] = %d outside 0 .. %d", who, s, counts[s], M);
    for (size_t i = 0; i < (size_t)F * M; ++i) {   // every frame's rows in use
      if ((int)(i % M) >= counts[s]) continue;
      const float* h = hz->hazards + ((size_t)s * F * M + i) * 3;
      if (!(std::isfinite(h[0]) && std::isfinite(h[1]) && std::isfinite(h[2]) && h[2] >= 0.f))
        return fail(MOBROB_ERR_INVALID, "%s: hazards: hazard %d of scene %d (frame %d) is not finite or has a negative radius", who,
                    (int)(i % M), s, (int)(i / M));
    }
  }
  if (hz->scene)
    for (int i = 0; i < N; ++i)
      if (hz->scene[i] < 0 || hz->scene[i] >= S)
        return fail(MOBROB_ERR_INVALID, "%s: hazards: scene[%d] = %d outside 0 .. %d", who, i, hz->scene[i], S - 1);
  return MOBROB_OK;
}
static void hazard_carve(EvalCarve& carve, const HazardIO& hio, int N, HazardCarve& hc) {
  const mobrob_hazards_t* hz = hio.hz;
  hc.hz = carve.add(std::max<size_t>((size_t)hz->n_scenes * hio.F * hz->max_hazards * 3, 1) * 4);
  hc.nhz = carve.add((size_t)hz->n_scenes * 4);
  hc.scene = carve.add((size_t)N * 4);
  hc.out = carve.add((size_t)N * 4 * 8);
  hc.acc = carve.add((size_t)N * 8);
}
// the hazard fields of `h` (after eval_prepare grew eval_buf); hazard_out is written by the task itself
template <class BaseArgs>
static int hazard_fill(mobrob_ppo_engine_t* e, const HazardIO& hio, int N, const HazardCarve& hc, HazardArgs<BaseArgs>& h) {
  const mobrob_hazards_t* hz = hio.hz;
  const size_t nf = (size_t)hz->n_scenes * hio.F * hz->max_hazards * 3;
  h.hz = eval_at<float>(e, hc.hz);
  h.nhz = eval_at<int>(e, hc.nhz);
  h.scene = hz->scene ? eval_at<int>(e, hc.scene) : nullptr;
  h.M = hz->max_hazards;
  h.coef = hz->cost;
  h.indicator = hz->indicator != 0;
  h.hazard_out = eval_at<double>(e, hc.out);
  h.ep_acc = eval_at<double>(e, hc.acc);
  h.ep_cost = nullptr;
  if (nf) HIPC(hipMemcpyAsync(const_cast<float*>(h.hz), hz->hazards, nf * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(const_cast<int*>(h.nhz), hc.counts.data(), (size_t)hz->n_scenes * 4, hipMemcpyHostToDevice, e->stream));
  if (hz->scene) HIPC(hipMemcpyAsync(const_cast<int*>(h.scene), hz->scene, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
  return MOBROB_OK;
}
// the time axis of the frames task around the filled static arguments
template <class BaseArgs>
static void hazard_fill_frames(const HazardIO& hio, FrameHazardArgs<BaseArgs>& hf) {
  hf.F = hio.F; hf.frame_steps = hio.frame_steps; hf.loop = hio.loop;
}

// ---- teams (mobrob_ppo_follow_waypoints_teams): checks, the run of a base task wrapped in TeamTask ----
struct TeamIO {
  const mobrob_teams_t* tm;
  double* team_out;           // [N][5] in / out
  int32_t* team_blocked_out = nullptr;   // [N][4] in / out: solid teams (mobrob_ppo_follow_waypoints_teams_solid) when not null
};
struct TeamFill {             // the team fields of TeamArgs (after eval_prepare grew eval_buf)
  int team_size;
  float sep, coef;
  int indicator;
  double* out;
  int* stepped;
};
static int team_check(const TeamIO& tio, int N, int step0, const double* robot_out) {
  const mobrob_teams_t* tm = tio.tm;
  const int ts = tm->team_size;
  if (ts != 1 && ts != 2 && ts != 4 && ts != 8 && ts != 16) return fail(MOBROB_ERR_INVALID, "follow: teams: team_size must be 1, 2, 4, 8 or 16");
  if (N % ts != 0) return fail(MOBROB_ERR_INVALID, "follow: teams: n_robots = %d is not a multiple of team_size = %d", N, ts);
  if (!(std::isfinite(tm->separation) && tm->separation >= 0.f)) return fail(MOBROB_ERR_INVALID, "follow: teams: separation must be finite and >= 0");
  if (!(std::isfinite(tm->cost) && tm->cost >= 0.f)) return fail(MOBROB_ERR_INVALID, "follow: teams: cost must be finite and >= 0");
  for (int i = 0; i < N; ++i) {
    const double* o = tio.team_out + (size_t)i * 5;
    const double steps = robot_out[(size_t)i * 4 + 1];
    const bool sums = std::isfinite(o[0]) && o[0] >= 0.0 && o[1] >= 0.0 && o[1] <= steps && o[1] == std::floor(o[1]);
    const bool first = o[2] >= -1.0 && o[2] <= (double)step0 && o[2] == std::floor(o[2]);
    const bool partner = o[4] == -1.0 || (o[4] == std::floor(o[4]) && o[4] >= (double)(i - i % ts) && o[4] < (double)(i - i % ts + ts) &&
                                          o[4] != (double)i);
    const bool clear = std::isnan(o[3]) == (steps == 0.0);
    if (!(sums && first && partner && clear))
      return fail(MOBROB_ERR_INVALID, "follow: teams: carried team record of robot %d is not one a call returns", i);
  }
  return MOBROB_OK;
}
template <class Base>
static int team_run(mobrob_ppo_engine_t* e, const typename Base::Args& b, const TeamFill& t) {
  const TeamArgs<typename Base::Args> a{b, t.team_size, t.sep, t.coef, t.indicator, t.out, t.stepped};
  return eval_run<TeamTask<Base>>(e, a, k_goal_task_fin<TeamTask<Base>>);
}

// ---- timed waypoints (mobrob_ppo_follow_waypoints_scheduled): checks of the schedule and of the carried record ----
struct SchedIO {
  const mobrob_follow_schedule_t* sc;
  double* sched_out;          // [N][2] in / out
};
static int sched_check(const SchedIO& sio, int N, int K, int P, const std::vector<int32_t>& nw, const double* robot_out) {
  const mobrob_follow_schedule_t* sc = sio.sc;
  if (!sc->release || !sc->home) return fail(MOBROB_ERR_INVALID, "follow: schedule: null argument");
  for (int i = 0; i < N; ++i) {
    for (int k = 0; k < nw[i]; ++k)
      if (sc->release[(size_t)i * K + k] < 0)
        return fail(MOBROB_ERR_INVALID, "follow: schedule: release step of waypoint %d of robot %d is negative", k, i);
    for (int j = 0; j < P; ++j)
      if (!std::isfinite(sc->home[(size_t)i * P + j])) return fail(MOBROB_ERR_INVALID, "follow: schedule: home of robot %d is not finite", i);
    const double* o = sio.sched_out + (size_t)i * 2;
    const double steps = robot_out[(size_t)i * 4 + 1];
    const bool count = o[0] >= 0.0 && o[0] <= steps && o[0] == std::floor(o[0]);
    const bool drift = std::isnan(o[1]) ? o[0] == 0.0 : (o[0] > 0.0 && o[1] >= 0.0 && std::isfinite(o[1]));
    if (!(count && drift))
      return fail(MOBROB_ERR_INVALID, "follow: schedule: carried hold record of robot %d is not one a call returns", i);
  }
  return MOBROB_OK;
}

// ---- walls (mobrob_ppo_follow_waypoints_walls): checks of the scene and of the carried record, the run of a task wrapped in WallTask ----
struct WallIO {
  const mobrob_walls_t* wl;
  double* wall_out;           // [N][7] in / out
  int32_t* blocked_out = nullptr;   // [N][4] in / out: solid walls (mobrob_ppo_follow_waypoints_solid) when not null
};
struct WallFill {           // the wall fields of WallArgs (after eval_prepare grew eval_buf)
  const float* boxes;
  const int* nwall;
  const int* scene;
  int M;
  float radius, coef;
  int indicator;
  double* out;
};
static int wall_check(const WallIO& wio, int N, int step0, const double* robot_out, std::vector<int32_t>& counts) {
  const mobrob_walls_t* wl = wio.wl;
  const int S = wl->n_scenes, M = wl->max_walls;
  if (S < 1) return fail(MOBROB_ERR_INVALID, "follow: walls: n_scenes must be >= 1");
  if (M < 0 || M > kWallMax) return fail(MOBROB_ERR_INVALID, "follow: walls: max_walls must lie in 0 .. %d", kWallMax);
  if (M > 0 && !wl->boxes) return fail(MOBROB_ERR_INVALID, "follow: walls: null box table");
  if (!wl->scene && S > 1) return fail(MOBROB_ERR_INVALID, "follow: walls: %d scenes need a scene index per robot", S);
  if (!(std::isfinite(wl->radius) && wl->radius >= 0.f)) return fail(MOBROB_ERR_INVALID, "follow: walls: radius must be finite and >= 0");
  if (!(std::isfinite(wl->cost) && wl->cost >= 0.f)) return fail(MOBROB_ERR_INVALID, "follow: walls: cost must be finite and >= 0");
  counts.assign(S, M);
  for (int s = 0; s < S; ++s) {
    if (wl->n_walls) counts[s] = wl->n_walls[s];
    if (counts[s] < 0 || counts[s] > M) return fail(MOBROB_ERR_INVALID, "follow: walls: n_walls[%d] = %d outside 0 .. %d", s, counts[s], M);
    for (int i = 0; i < counts[s]; ++i) {
      const float* b = wl->boxes + ((size_t)s * M + i) * 4;
      if (!(std::isfinite(b[0]) && std::isfinite(b[1]) && std::isfinite(b[2]) && std::isfinite(b[3]) && b[2] >= 0.f && b[3] >= 0.f))
        return fail(MOBROB_ERR_INVALID, "follow: walls: box %d of scene %d is not finite or has a negative half extent", i, s);
    }
  }
  if (wl->scene)
    for (int i = 0; i < N; ++i)
      if (wl->scene[i] < 0 || wl->scene[i] >= S)
        return fail(MOBROB_ERR_INVALID, "follow: walls: scene[%d] = %d outside 0 .. %d", i, wl->scene[i], S - 1);
  for (int i = 0; i < N; ++i) {
    const double* o = wio.wall_out + (size_t)i * 7;
    const double steps = robot_out[(size_t)i * 4 + 1];
    const int m = counts[wl->scene ? wl->scene[i] : 0];
    const auto count = [&](double v) { return v >= 0.0 && v <= steps && v == std::floor(v); };
    const auto first = [&](double v) { return v >= -1.0 && v <= (double)step0 && v == std::floor(v); };
    const bool sums = std::isfinite(o[0]) && o[0] >= 0.0 && count(o[1]) && count(o[5]) && first(o[2]) && first(o[6]);
    const bool wall = o[4] == -1.0 || (o[4] == std::floor(o[4]) && o[4] >= 0.0 && o[4] < (double)m);
    const bool clear = std::isnan(o[3]) == (steps == 0.0);
    if (!(sums && wall && clear))
      return fail(MOBROB_ERR_INVALID, "follow: walls: carried wall record of robot %d is not one a call returns", i);
  }
  return MOBROB_OK;
}

// the task Task with teams when `tio`, else on its own
template <class Task>
static int run_with_teams(mobrob_ppo_engine_t* e, const typename Task::Args& a, const TeamIO* tio, const TeamFill& tf) {
  return tio ? team_run<Task>(e, a, tf) : eval_run<Task>(e, a, k_goal_task_fin<Task>);
}
// ... wrapped in WallTask when `wio` (pre_off: where the tile's pre-step block starts, after everything the wrapped task keeps in LDS)
template <class Task>
static int run_with_walls(mobrob_ppo_engine_t* e, const typename Task::Args& a, const WallIO* wio, const WallFill& wf, const TeamIO* tio,
                          const TeamFill& tf) {
  if (!wio) return run_with_teams<Task>(e, a, tio, tf);
  const WallArgs<typename Task::Args> w{a, wf.boxes, wf.nwall, wf.scene, wf.M, wf.radius, wf.coef, wf.indicator,
                                        (int)WallTask<Task>::base_lds_floats(a), wf.out};
  return run_with_teams<WallTask<Task>>(e, w, tio, tf);
}

// One call of a run on the resumable task Base (ResumeFollowTask, ScheduledFollowTask), filled in hf.h.b: with hazards when
// `hio`, with walls when `wio`, with teams when `tio`.  Uploads the carried hazard and team records, runs, and downloads the team
// record (the wall record is the caller's to move: its buffers are filled before the call).
template <class Base>
static int resume_run(mobrob_ppo_engine_t* e, int N, const HazardIO* hio, const HazardCarve& hc, const TeamIO* tio, const TeamFill& tf,
                      FrameHazardArgs<typename Base::Args>& hf, double*& hazard_dev, const WallIO* wio, const WallFill& wf) {
  HazardArgs<typename Base::Args>& h = hf.h;
  if (hio) {
    if (const int rc = hazard_fill(e, *hio, N, hc, h)) return rc;
    hazard_fill_frames(*hio, hf);
    HIPC(hipMemcpyAsync(h.hazard_out, hio->hazard_out, (size_t)N * 4 * 8, hipMemcpyHostToDevice, e->stream));
  }
  hazard_dev = h.hazard_out;
  if (tio) HIPC(hipMemcpyAsync(tf.out, tio->team_out, (size_t)N * 5 * 8, hipMemcpyHostToDevice, e->stream));
  const int ran = !hio ? run_with_walls<Base>(e, h.b, wio, wf, tio, tf)
                  : hio->frames ? run_with_walls<FrameHazardTask<Base>>(e, hf, wio, wf, tio, tf)
                                : run_with_walls<HazardTask<Base>>(e, h, wio, wf, tio, tf);
  if (tio && ran >= 0) HIPC(hipMemcpyAsync(tio->team_out, tf.out, (size_t)N * 5 * 8, hipMemcpyDeviceToHost, e->stream));
  return ran;
}

// run_with_walls for a task that always has them (no instance of the task outside WallTask)
template <class Task>
static int run_in_walls(mobrob_ppo_engine_t* e, const typename Task::Args& a, const WallFill& wf, const TeamIO* tio, const TeamFill& tf) {
  const WallArgs<typename Task::Args> w{a, wf.boxes, wf.nwall, wf.scene, wf.M, wf.radius, wf.coef, wf.indicator,
                                        (int)WallTask<Task>::base_lds_floats(a), wf.out};
  return run_with_teams<WallTask<Task>>(e, w, tio, tf);
}

// the carried blocked record of a run with solid walls: refused before any launch or copy
static int solid_check(const WallIO& wio, int N, int step0, const double* robot_out) {
  for (int i = 0; i < N; ++i) {
    const int32_t* o = wio.blocked_out + (size_t)i * 4;
    const double steps = robot_out[(size_t)i * 4 + 1];
    const auto count = [&](int32_t v) { return v >= 0 && (double)v <= steps; };
    if (!(count(o[0]) && count(o[2]) && count(o[3]) && o[2] <= o[0] && o[1] >= -1 && o[1] <= step0 && (o[1] < 0) == (o[0] == 0)))
      return fail(MOBROB_ERR_INVALID, "follow: solid: carried blocked record of robot %d is not one a call returns", i);
  }
  return MOBROB_OK;
}

// resume_run with solid walls: Base (filled in `b`) restated as SolidFollowTask<Base>, alone or under static hazards, always in
// WallTask, with teams when `tio`.  blocked_dev: the uploaded blocked record (downloaded by the caller).
template <class Base>
static int solid_run(mobrob_ppo_engine_t* e, int N, const HazardIO* hio, const HazardCarve& hc, const TeamIO* tio, const TeamFill& tf,
                     const typename Base::Args& b, double*& hazard_dev, const WallIO* wio, const WallFill& wf, int* blocked_dev) {
  using Solid = SolidFollowTask<Base>;
  HazardArgs<typename Solid::Args> h{};
  h.b = typename Solid::Args{b, wf.radius, blocked_dev};
  if (hio) {
    if (const int rc = hazard_fill(e, *hio, N, hc, h)) return rc;
    HIPC(hipMemcpyAsync(h.hazard_out, hio->hazard_out, (size_t)N * 4 * 8, hipMemcpyHostToDevice, e->stream));
  }
  hazard_dev = h.hazard_out;
  if (tio) HIPC(hipMemcpyAsync(tf.out, tio->team_out, (size_t)N * 5 * 8, hipMemcpyHostToDevice, e->stream));
  const int ran = !hio ? run_in_walls<Solid>(e, h.b, wf, tio, tf) : run_in_walls<HazardTask<Solid>>(e, h, wf, tio, tf);
  if (tio && ran >= 0) HIPC(hipMemcpyAsync(tio->team_out, tf.out, (size_t)N * 5 * 8, hipMemcpyDeviceToHost, e->stream));
  return ran;
}

// the carried team-blocked record of a run with solid teams: refused before any launch or copy
static int team_solid_check(const TeamIO& tio, int N, int step0, const double* robot_out) {
  for (int i = 0; i < N; ++i) {
    const int32_t* o = tio.team_blocked_out + (size_t)i * 4;
    const double steps = robot_out[(size_t)i * 4 + 1];
    const auto count = [&](int32_t v) { return v >= 0 && (double)v <= steps; };
    if (!(count(o[0]) && count(o[2]) && count(o[3]) && o[2] <= o[0] && o[1] >= -1 && o[1] <= step0 && (o[1] < 0) == (o[0] == 0)))
      return fail(MOBROB_ERR_INVALID, "follow: solid teams: carried team-blocked record of robot %d is not one a call returns", i);
  }
  return MOBROB_OK;
}

// one call of a run with solid teams: Base (filled in `b`) restated as SolidTeamFollowTask<Base, walls>, in TeamTask, with solid
// walls (`wio`) in WallTask between the two.  tblk_dev / blocked_dev: the uploaded records (downloaded by the caller).
template <class Base>
static int team_solid_run(mobrob_ppo_engine_t* e, int N, const TeamIO* tio, const TeamFill& tf, const typename Base::Args& b,
                          const WallIO* wio, const WallFill& wf, int* blocked_dev, int* tblk_dev) {
  HIPC(hipMemcpyAsync(tf.out, tio->team_out, (size_t)N * 5 * 8, hipMemcpyHostToDevice, e->stream));
  int ran;
  if (wio) {
    using Solid = SolidTeamFollowTask<Base, true>;
    const typename Solid::Args a{b, tf.team_size, tf.sep, wf.radius, tblk_dev, blocked_dev};
    const WallArgs<typename Solid::Args> w{a, wf.boxes, wf.nwall, wf.scene, wf.M, wf.radius, wf.coef, wf.indicator,
                                           (int)WallTask<Solid>::base_lds_floats(a), wf.out};
    ran = team_run<WallTask<Solid>>(e, w, tf);   // (never without TeamTask: no such instance is built)
  } else {
    using Solid = SolidTeamFollowTask<Base, false>;
    const typename Solid::Args a{b, tf.team_size, tf.sep, 0.f, tblk_dev, nullptr};
    ran = team_run<Solid>(e, a, tf);
  }
  if (ran >= 0) HIPC(hipMemcpyAsync(tio->team_out, tf.out, (size_t)N * 5 * 8, hipMemcpyDeviceToHost, e->stream));
  return ran;
}
}  // extern "C++"

// evaluate, with hazards when `hio` is not null (mobrob_ppo_evaluate_goal_env_hazards)
static int evaluate_goal_env(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_eval_spec_t* spec,
                             const int32_t* quota, double* robot_out, double* episode_out, float* trace_out, const HazardIO* hio) {
  if (!e || !env || !spec || !robot_out) return fail(MOBROB_ERR_INVALID, "evaluate: null argument");
  EvalCall c{"evaluate", spec->n_robots, spec->max_steps, spec->deterministic, spec->seed, spec->trace_robots, spec->trace_steps, trace_out};
  if (hio) c.trace_extra = kHazardTraceExtra;
  const int N = c.N;
  if (N < 1) return fail(MOBROB_ERR_INVALID, "evaluate: n_robots must be >= 1");
  if (spec->max_steps < 1) return fail(MOBROB_ERR_INVALID, "evaluate: max_steps must be >= 1");
  if (spec->episodes < 0) return fail(MOBROB_ERR_INVALID, "evaluate: episodes must be >= 0");
  if (const int rc = eval_check_dims(e, env, c.who)) return rc;
  if (env->time_limit < 0) return fail(MOBROB_ERR_INVALID, "evaluate: time_limit must be >= 0 (0: none)");
  if (spec->episodes > 0 && env->time_limit == 0)
    return fail(MOBROB_ERR_INVALID, "evaluate: an episode quota needs a time limit (the run might never finish)");
  if (const int rc = eval_check_actions_trace(e, c)) return rc;
  std::vector<int32_t> q(N);
  int maxq = 0;
  for (int i = 0; i < N; ++i) {
    q[i] = quota ? quota[i] : (spec->episodes > 0 ? (int32_t)(((int64_t)spec->episodes + i) / N) : 0);
    if (q[i] < 0) return fail(MOBROB_ERR_INVALID, "evaluate: negative quota");
    maxq = std::max(maxq, (int)q[i]);
  }
  HazardCarve hc;
  if (hio)
    if (const int rc = hazard_check(*hio, N, c.who, hc.counts)) return rc;
  EvalCarve carve;
  const size_t o_ep = carve.add(std::max<size_t>((size_t)N * maxq * 3, 1) * 8), o_q = carve.add((size_t)N * 4), o_er = carve.add((size_t)N * 8);
  size_t o_ec = 0;
  if (hio) {
    hazard_carve(carve, *hio, N, hc);
    o_ec = carve.add(std::max<size_t>((size_t)N * maxq, 1) * 8);
  }
  FrameHazardArgs<EvalArgs> hf{};   // the frames task's arguments: its HazardArgs / EvalArgs are the ones filled below
  HazardArgs<EvalArgs>& h = hf.h;
  EvalArgs& a = h.b;
  const GoalEnvParams p = eval_env_params(env, e->A, env->terminate_on_goal != 0, env->time_limit > 0 ? env->time_limit : INT_MAX);   // control.py: no limit
  if (const int rc = eval_prepare(e, c, p, carve, a)) return rc;
  int* q_dev = eval_at<int>(e, o_q);
  a.ep_out = eval_at<double>(e, o_ep);
  a.ep_ret = eval_at<double>(e, o_er);
  a.quota = q_dev;
  a.episodes = spec->episodes; a.maxq = maxq;
  // a robot finishes an episode at least every time_limit steps: with a quota, the run is over after maxq * time_limit steps
  if (spec->episodes > 0) a.max_steps = (int)std::min<int64_t>(a.max_steps, (int64_t)maxq * env->time_limit);
  HIPC(hipMemcpyAsync(q_dev, q.data(), (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
  if (maxq > 0) HIPC(hipMemsetAsync(a.ep_out, 0, (size_t)N * maxq * 3 * 8, e->stream));
  if (hio) {
    if (const int rc = hazard_fill(e, *hio, N, hc, h)) return rc;
    hazard_fill_frames(*hio, hf);
    h.ep_cost = eval_at<double>(e, o_ec);
    if (maxq > 0) HIPC(hipMemsetAsync(h.ep_cost, 0, (size_t)N * maxq * 8, e->stream));
  }
  const int ran = !hio ? eval_run<EvalTask>(e, a, nullptr)
                  : hio->frames ? eval_run<FrameHazardTask<EvalTask>>(e, hf, nullptr) : eval_run<HazardEvalTask>(e, h, nullptr);
  if (ran < 0) return ran;
  if (episode_out && maxq > 0)
    HIPC(hipMemcpyAsync(episode_out, a.ep_out, (size_t)N * maxq * 3 * 8, hipMemcpyDeviceToHost, e->stream));
  if (hio) {
    HIPC(hipMemcpyAsync(hio->hazard_out, h.hazard_out, (size_t)N * 4 * 8, hipMemcpyDeviceToHost, e->stream));
    if (hio->episode_cost_out && maxq > 0)
      HIPC(hipMemcpyAsync(hio->episode_cost_out, h.ep_cost, (size_t)N * maxq * 8, hipMemcpyDeviceToHost, e->stream));
  }
  return eval_copy_back(e, c, a, robot_out, ran);
}

int mobrob_ppo_evaluate_goal_env(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_eval_spec_t* spec,
                                 const int32_t* quota, double* robot_out, double* episode_out, float* trace_out) {
  return evaluate_goal_env(e, env, spec, quota, robot_out, episode_out, trace_out, nullptr);
}

int mobrob_ppo_evaluate_goal_env_hazards(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_eval_spec_t* spec,
                                         const mobrob_hazards_t* hz, const int32_t* quota, double* robot_out, double* episode_out,
                                         double* hazard_out, double* episode_cost_out, float* trace_out) {
  if (!hz || !hazard_out) return fail(MOBROB_ERR_INVALID, "evaluate: null argument");
  const HazardIO hio{hz, hazard_out, episode_cost_out};
  return evaluate_goal_env(e, env, spec, quota, robot_out, episode_out, trace_out, &hio);
}

int mobrob_ppo_evaluate_goal_env_hazard_frames(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_eval_spec_t* spec,
                                               const mobrob_hazard_frames_t* hz, const int32_t* quota, double* robot_out,
                                               double* episode_out, double* hazard_out, double* episode_cost_out, float* trace_out) {
  if (!hz || !hazard_out) return fail(MOBROB_ERR_INVALID, "evaluate: null argument");
  mobrob_hazards_t view;
  const HazardIO hio = hazard_frames_io(hz, view, hazard_out, episode_cost_out);
  return evaluate_goal_env(e, env, spec, quota, robot_out, episode_out, trace_out, &hio);
}

// ---- waypoint following: the policy as a tracker of given goal sequences ------------------------------------------------
// what a call of a resumable run carries in besides arrival / robot_out / hazard_out: refused before any launch or copy
static int follow_resume_check(const mobrob_follow_resume_t* rs, const mobrob_follow_spec_t* spec, const std::vector<int32_t>& nw,
                               const double* robot_out, const double* hazard_out) {
  const int N = spec->n_robots;
  if (!rs->state || !rs->leg_used || !rs->status) return fail(MOBROB_ERR_INVALID, "follow: resume: null argument");
  if (rs->step0 < 0 || (int64_t)rs->step0 + spec->max_steps > INT_MAX)
    return fail(MOBROB_ERR_INVALID, "follow: resume: step0 must be >= 0 and step0 + max_steps fit an int32");
  if (rs->leg_steps < 0) return fail(MOBROB_ERR_INVALID, "follow: resume: leg_steps must be >= 0 (0: no budget)");
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j < 6; ++j)
      if (!std::isfinite(rs->state[(size_t)i * 6 + j])) return fail(MOBROB_ERR_INVALID, "follow: resume: state of robot %d is not finite", i);
    if (rs->leg_used[i] < 0 || rs->leg_used[i] > rs->leg_steps)
      return fail(MOBROB_ERR_INVALID, "follow: resume: leg_used[%d] = %d outside 0 .. %d", i, rs->leg_used[i], rs->leg_steps);
    const double* o = robot_out + (size_t)i * 4;
    if (!std::isfinite(o[0])) return fail(MOBROB_ERR_INVALID, "follow: resume: reward sum of robot %d is not finite", i);
    // the counts travel as float64 and are read back as int32: a value that is not a whole number is refused, not truncated
    if (!(o[1] >= 0.0 && o[1] <= (double)(INT_MAX - spec->max_steps) && o[1] == std::floor(o[1])))
      return fail(MOBROB_ERR_INVALID, "follow: resume: steps run of robot %d not a whole number in 0 .. INT_MAX - max_steps", i);
    if (!(o[2] >= 0.0 && o[2] <= (double)nw[i] && o[2] == std::floor(o[2])))
      return fail(MOBROB_ERR_INVALID, "follow: resume: waypoints reached of robot %d not a whole number in 0 .. %d", i, nw[i]);
    if (hazard_out) {
      const double* h = hazard_out + (size_t)i * 4;
      if (!(std::isfinite(h[0]) && h[1] >= 0.0 && h[1] <= o[1] && h[1] == std::floor(h[1]) && h[2] >= -1.0 &&
            h[2] <= (double)INT_MAX && h[2] == std::floor(h[2])))
        return fail(MOBROB_ERR_INVALID, "follow: resume: carried hazard record of robot %d is not one a call returns", i);
    }
  }
  return MOBROB_OK;
}

// follow, with hazards when `hio` is not null (mobrob_ppo_follow_waypoints_hazards); one call of a resumable run when `rs` is not
// null (mobrob_ppo_follow_waypoints_resume: no `start`, arrival / robot_out / hazard_out in and out), with teams when `tio` is not
// null (mobrob_ppo_follow_waypoints_teams: a call of a run, team_out in and out), with timed waypoints when `sio` is not null
// (mobrob_ppo_follow_waypoints_scheduled: ScheduledFollowTask in ResumeFollowTask's place, sched_out in and out), with walls when
// `wio` is not null (mobrob_ppo_follow_waypoints_walls: WallTask around the run's task, wall_out in and out)
static int follow_waypoints(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                            const float* start, const float* waypoints, const int32_t* n_waypoints, int32_t* arrival,
                            double* robot_out, float* path_out, float* trace_out, const HazardIO* hio,
                            const mobrob_follow_resume_t* rs = nullptr, const TeamIO* tio = nullptr, const SchedIO* sio = nullptr,
                            const WallIO* wio = nullptr) {
  if (!e || !env || !spec || (!start && !rs) || !waypoints || !arrival || !robot_out) return fail(MOBROB_ERR_INVALID, "follow: null argument");
  EvalCall c{"follow", spec->n_robots, spec->max_steps, spec->deterministic, spec->seed, spec->trace_robots, spec->trace_steps, trace_out};
  if (hio) c.trace_extra = kHazardTraceExtra;
  const int N = c.N, K = spec->max_waypoints, P = env->pos_dim;
  if (N < 1) return fail(MOBROB_ERR_INVALID, "follow: n_robots must be >= 1");
  if (K < 1) return fail(MOBROB_ERR_INVALID, "follow: max_waypoints must be >= 1");
  if (spec->max_steps < 1) return fail(MOBROB_ERR_INVALID, "follow: max_steps must be >= 1");
  if (spec->path_stride < 0) return fail(MOBROB_ERR_INVALID, "follow: path_stride must be >= 0 (0: no path)");
  if (const int rc = eval_check_dims(e, env, c.who)) return rc;
  // (a negative trace size is never `tracing`, so the shared trace-bounds check cannot fire in its place)
  if (const int rc = eval_check_actions_trace(e, c)) return rc;
  if (spec->trace_robots < 0 || spec->trace_steps < 0) return fail(MOBROB_ERR_INVALID, "follow: negative trace size");
  std::vector<int32_t> nw(N);
  for (int i = 0; i < N; ++i) {
    nw[i] = n_waypoints ? n_waypoints[i] : K;
    if (nw[i] < 0 || nw[i] > K) return fail(MOBROB_ERR_INVALID, "follow: n_waypoints[%d] = %d outside 0 .. %d", i, nw[i], K);
    for (int j = 0; start && j < P; ++j)   // (a call of a run has no start: its state is checked by follow_resume_check)
      if (!std::isfinite(start[(size_t)i * P + j])) return fail(MOBROB_ERR_INVALID, "follow: start of robot %d is not finite", i);
    for (int k = 0; k < nw[i]; ++k)
      for (int j = 0; j < P; ++j)
        if (!std::isfinite(waypoints[((size_t)i * K + k) * P + j]))
          return fail(MOBROB_ERR_INVALID, "follow: waypoint %d of robot %d is not finite", k, i);
  }
  HazardCarve hc;
  if (hio)
    if (const int rc = hazard_check(*hio, N, c.who, hc.counts)) return rc;
  if (rs)
    if (const int rc = follow_resume_check(rs, spec, nw, robot_out, hio ? hio->hazard_out : nullptr)) return rc;
  if (tio)   // (only with rs: the entry point refuses a call without it)
    if (const int rc = team_check(*tio, N, rs->step0, robot_out)) return rc;
  if (tio && tio->team_blocked_out) {   // solid teams: alone or with solid walls, over both run tasks
    if (hio)
      return fail(MOBROB_ERR_INVALID, hio->frames ? "follow: solid teams: solid teams do not run with hazard frames yet (solid walls and schedules do)"
                                                  : "follow: solid teams: solid teams do not run with static hazards yet (solid walls and schedules do)");
    if (wio && !wio->blocked_out)
      return fail(MOBROB_ERR_INVALID, "follow: solid teams: solid teams do not run with observational walls yet (solid walls do)");
    if (const int rc = team_solid_check(*tio, N, rs->step0, robot_out)) return rc;
  }
  if (sio)   // (only with rs, likewise)
    if (const int rc = sched_check(*sio, N, K, P, nw, robot_out)) return rc;
  std::vector<int32_t> wall_counts;
  if (wio) {   // (only with rs, likewise)
    if (const int rc = wall_check(*wio, N, rs->step0, robot_out, wall_counts)) return rc;
    if (wio->blocked_out) {
      if (hio && hio->frames)
        return fail(MOBROB_ERR_INVALID, "follow: solid: solid walls do not run with hazard frames yet (static hazards, teams and schedules do)");
      if (const int rc = solid_check(*wio, N, rs->step0, robot_out)) return rc;
    }
    if (e->fused.enabled && e->fused.H == 64) {   // the tile kernel's LDS: actor, the hazards' blocks, the walls' blocks
      const size_t hz_floats = hio ? 32 + (hio->hz->scene ? 0 : 3 * (size_t)hio->hz->max_hazards) : 32;
      const size_t tile = eval64_lds_bytes(eval_tile_width(e->Dp, wio->blocked_out != nullptr)) + (hz_floats + 32 + (wio->wl->scene ? 0 : 4 * (size_t)wio->wl->max_walls)) * sizeof(float);
      int limit = 0;
      if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, e->cfg.device_id) != hipSuccess) limit = 64 * 1024;
      if (tile > (size_t)limit)
        return fail(MOBROB_ERR_INVALID, "follow: walls: the tile kernel needs %zu bytes of LDS with this scene, the device allows %d per workgroup",
                    tile, limit);
    }
  }
  const bool pathing = path_out && spec->path_stride > 0;
  const size_t n_rec = pathing ? (size_t)(spec->max_steps / spec->path_stride + 1) : 0;
  EvalCarve carve;
  const size_t o_arr = carve.add((size_t)N * K * 4), o_start = carve.add((size_t)N * P * 4), o_wp = carve.add((size_t)N * K * P * 4),
               o_nw = carve.add((size_t)N * 4), o_path = carve.add(std::max<size_t>(n_rec * N * P, 1) * 4);
  if (hio) hazard_carve(carve, *hio, N, hc);
  const size_t o_state = carve.add(rs ? (size_t)N * 6 * 4 : 0), o_leg = carve.add(rs ? (size_t)N * 4 : 0),
               o_status = carve.add(rs ? (size_t)N * 4 : 0), o_entry = carve.add(rs ? (size_t)N * 4 : 0),
               o_team = carve.add(tio ? (size_t)N * 5 * 8 : 0), o_stepped = carve.add(tio ? (size_t)N * 4 : 0),
               o_rel = carve.add(sio ? (size_t)N * K * 4 : 0), o_home = carve.add(sio ? (size_t)N * P * 4 : 0),
               o_sched = carve.add(sio ? (size_t)N * 2 * 8 : 0),
               o_wbox = carve.add(wio ? std::max<size_t>((size_t)wio->wl->n_scenes * wio->wl->max_walls * 4, 1) * 4 : 0),
               o_wcnt = carve.add(wio ? (size_t)wio->wl->n_scenes * 4 : 0), o_wscene = carve.add(wio ? (size_t)N * 4 : 0),
               o_wout = carve.add(wio ? (size_t)N * 7 * 8 : 0), o_wblk = carve.add(wio && wio->blocked_out ? (size_t)N * 4 * 4 : 0),
               o_tblk = carve.add(tio && tio->team_blocked_out ? (size_t)N * 4 * 4 : 0);
  FrameHazardArgs<FollowArgs> hf{};    // the frames tasks' arguments hold the static tasks'
  FrameHazardArgs<ResumeArgs> hrf{};
  FrameHazardArgs<ScheduledArgs> hsf{};
  HazardArgs<FollowArgs>& h = hf.h;
  // the resumable task's arguments (the scheduled task holds them in turn): its FollowArgs is the one filled below
  ResumeArgs& r = sio ? hsf.h.b.r : hrf.h.b;
  FollowArgs& f = rs ? r.f : h.b;
  // no termination, no time limit: the robot only stops at its last waypoint
  if (const int rc = eval_prepare(e, c, eval_env_params(env, e->A, false, INT_MAX), carve, f.e)) return rc;
  float* start_dev = eval_at<float>(e, o_start);
  float* wp_dev = eval_at<float>(e, o_wp);
  int* nw_dev = eval_at<int>(e, o_nw);
  float* path_dev = eval_at<float>(e, o_path);
  f.arrival = eval_at<int>(e, o_arr);
  f.K = K; f.path_stride = pathing ? spec->path_stride : 0;
  f.start = rs ? nullptr : start_dev; f.wp = wp_dev; f.nwp = nw_dev;
  f.path = pathing ? path_dev : nullptr;
  if (!rs) HIPC(hipMemcpyAsync(start_dev, start, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(wp_dev, waypoints, (size_t)N * K * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(nw_dev, nw.data(), (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
  int ran;
  double* hazard_dev = nullptr;
  if (!rs) {
    HIPC(hipMemsetAsync(f.arrival, 0xFF, (size_t)N * K * 4, e->stream));   // -1: not reached
    if (hio) {
      if (const int rc = hazard_fill(e, *hio, N, hc, h)) return rc;
      hazard_fill_frames(*hio, hf);
    }
    hazard_dev = h.hazard_out;
    ran = !hio ? eval_run<FollowTask>(e, f, k_follow_goal_fin)
          : hio->frames ? eval_run<FrameHazardTask<FollowTask>>(e, hf, k_goal_task_fin<FrameHazardTask<FollowTask>>)
                        : eval_run<HazardFollowTask>(e, h, k_hazard_follow_fin);
  } else {
    // the run so far: arrival rows, accumulators, state
    r.step0 = rs->step0; r.leg_steps = rs->leg_steps;
    r.state = eval_at<float>(e, o_state); r.leg_used = eval_at<int>(e, o_leg);
    r.status = eval_at<int>(e, o_status); r.entry_steps = eval_at<int>(e, o_entry);
    HIPC(hipMemcpyAsync(f.arrival, arrival, (size_t)N * K * 4, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(f.e.robot_out, robot_out, (size_t)N * 4 * 8, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(r.state, rs->state, (size_t)N * 6 * 4, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(r.leg_used, rs->leg_used, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
    TeamFill tf{};
    if (tio)
      tf = TeamFill{tio->tm->team_size, tio->tm->separation, tio->tm->cost, tio->tm->indicator != 0, eval_at<double>(e, o_team),
                    eval_at<int>(e, o_stepped)};
    WallFill wf{};
    if (wio) {
      const mobrob_walls_t* wl = wio->wl;
      const size_t nb = (size_t)wl->n_scenes * wl->max_walls * 4;
      float* box_dev = eval_at<float>(e, o_wbox);
      int* cnt_dev = eval_at<int>(e, o_wcnt);
      int* scene_dev = wl->scene ? eval_at<int>(e, o_wscene) : nullptr;
      wf = WallFill{box_dev, cnt_dev, scene_dev, wl->max_walls, wl->radius, wl->cost, wl->indicator != 0, eval_at<double>(e, o_wout)};
      if (nb) HIPC(hipMemcpyAsync(box_dev, wl->boxes, nb * 4, hipMemcpyHostToDevice, e->stream));
      HIPC(hipMemcpyAsync(cnt_dev, wall_counts.data(), (size_t)wl->n_scenes * 4, hipMemcpyHostToDevice, e->stream));
      if (wl->scene) HIPC(hipMemcpyAsync(scene_dev, wl->scene, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
      HIPC(hipMemcpyAsync(wf.out, wio->wall_out, (size_t)N * 7 * 8, hipMemcpyHostToDevice, e->stream));
    }
    const bool solid = wio && wio->blocked_out;
    int* blocked_dev = solid ? eval_at<int>(e, o_wblk) : nullptr;
    if (solid) HIPC(hipMemcpyAsync(blocked_dev, wio->blocked_out, (size_t)N * 4 * 4, hipMemcpyHostToDevice, e->stream));
    const bool tsolid = tio && tio->team_blocked_out;
    int* tblk_dev = tsolid ? eval_at<int>(e, o_tblk) : nullptr;
    if (tsolid) HIPC(hipMemcpyAsync(tblk_dev, tio->team_blocked_out, (size_t)N * 4 * 4, hipMemcpyHostToDevice, e->stream));
    if (sio) {
      ScheduledArgs& sa = hsf.h.b;
      int* rel_dev = eval_at<int>(e, o_rel);
      float* home_dev = eval_at<float>(e, o_home);
      sa.release = rel_dev; sa.home = home_dev; sa.sched_out = eval_at<double>(e, o_sched);
      HIPC(hipMemcpyAsync(rel_dev, sio->sc->release, (size_t)N * K * 4, hipMemcpyHostToDevice, e->stream));
      HIPC(hipMemcpyAsync(home_dev, sio->sc->home, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
      HIPC(hipMemcpyAsync(sa.sched_out, sio->sched_out, (size_t)N * 2 * 8, hipMemcpyHostToDevice, e->stream));
      ran = tsolid ? team_solid_run<ScheduledFollowTask>(e, N, tio, tf, sa, wio, wf, blocked_dev, tblk_dev)
            : solid ? solid_run<ScheduledFollowTask>(e, N, hio, hc, tio, tf, sa, hazard_dev, wio, wf, blocked_dev)
                  : resume_run<ScheduledFollowTask>(e, N, hio, hc, tio, tf, hsf, hazard_dev, wio, wf);
      if (ran >= 0) HIPC(hipMemcpyAsync(sio->sched_out, sa.sched_out, (size_t)N * 2 * 8, hipMemcpyDeviceToHost, e->stream));
    } else {
      ran = tsolid ? team_solid_run<ResumeFollowTask>(e, N, tio, tf, r, wio, wf, blocked_dev, tblk_dev)
            : solid ? solid_run<ResumeFollowTask>(e, N, hio, hc, tio, tf, r, hazard_dev, wio, wf, blocked_dev)
                  : resume_run<ResumeFollowTask>(e, N, hio, hc, tio, tf, hrf, hazard_dev, wio, wf);
    }
    if (ran >= 0) {
      HIPC(hipMemcpyAsync(rs->state, r.state, (size_t)N * 6 * 4, hipMemcpyDeviceToHost, e->stream));
      HIPC(hipMemcpyAsync(rs->leg_used, r.leg_used, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
      HIPC(hipMemcpyAsync(rs->status, r.status, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
      if (wio) HIPC(hipMemcpyAsync(wio->wall_out, wf.out, (size_t)N * 7 * 8, hipMemcpyDeviceToHost, e->stream));
      if (solid) HIPC(hipMemcpyAsync(wio->blocked_out, blocked_dev, (size_t)N * 4 * 4, hipMemcpyDeviceToHost, e->stream));
      if (tsolid) HIPC(hipMemcpyAsync(tio->team_blocked_out, tblk_dev, (size_t)N * 4 * 4, hipMemcpyDeviceToHost, e->stream));
    }
  }
  if (ran < 0) return ran;
  HIPC(hipMemcpyAsync(arrival, f.arrival, (size_t)N * K * 4, hipMemcpyDeviceToHost, e->stream));
  if (pathing) HIPC(hipMemcpyAsync(path_out, path_dev, n_rec * N * P * 4, hipMemcpyDeviceToHost, e->stream));
  if (hio) HIPC(hipMemcpyAsync(hio->hazard_out, hazard_dev, (size_t)N * 4 * 8, hipMemcpyDeviceToHost, e->stream));
  return eval_copy_back(e, c, f.e, robot_out, ran);
}

int mobrob_ppo_follow_waypoints(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                const float* start, const float* waypoints, const int32_t* n_waypoints, int32_t* arrival,
                                double* robot_out, float* path_out, float* trace_out) {
  return follow_waypoints(e, env, spec, start, waypoints, n_waypoints, arrival, robot_out, path_out, trace_out, nullptr);
}

int mobrob_ppo_follow_waypoints_hazards(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                        const mobrob_hazards_t* hz, const float* start, const float* waypoints,
                                        const int32_t* n_waypoints, int32_t* arrival, double* robot_out, double* hazard_out,
                                        float* path_out, float* trace_out) {
  if (!hz || !hazard_out) return fail(MOBROB_ERR_INVALID, "follow: null argument");
  const HazardIO hio{hz, hazard_out, nullptr};
  return follow_waypoints(e, env, spec, start, waypoints, n_waypoints, arrival, robot_out, path_out, trace_out, &hio);
}

int mobrob_ppo_follow_waypoints_resume(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                       const mobrob_hazards_t* hz, const mobrob_follow_resume_t* resume, const float* waypoints,
                                       const int32_t* n_waypoints, int32_t* arrival, double* robot_out, double* hazard_out,
                                       float* path_out, float* trace_out) {
  if (!resume || (hz == nullptr) != (hazard_out == nullptr)) return fail(MOBROB_ERR_INVALID, "follow: resume: null argument");
  const HazardIO hio{hz, hazard_out, nullptr};
  return follow_waypoints(e, env, spec, nullptr, waypoints, n_waypoints, arrival, robot_out, path_out, trace_out,
                          hz ? &hio : nullptr, resume);
}

int mobrob_ppo_follow_waypoints_hazard_frames(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                              const mobrob_hazard_frames_t* hz, const mobrob_follow_resume_t* resume, const float* start,
                                              const float* waypoints, const int32_t* n_waypoints, int32_t* arrival, double* robot_out,
                                              double* hazard_out, float* path_out, float* trace_out) {
  if (!hz || !hazard_out) return fail(MOBROB_ERR_INVALID, "follow: null argument");
  mobrob_hazards_t view;
  const HazardIO hio = hazard_frames_io(hz, view, hazard_out, nullptr);
  return follow_waypoints(e, env, spec, resume ? nullptr : start, waypoints, n_waypoints, arrival, robot_out, path_out, trace_out, &hio,
                          resume);
}

int mobrob_ppo_follow_waypoints_teams(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                      const mobrob_hazards_t* hz, const mobrob_hazard_frames_t* hzf, const mobrob_follow_resume_t* resume,
                                      const mobrob_teams_t* teams, const float* waypoints, const int32_t* n_waypoints, int32_t* arrival,
                                      double* robot_out, double* hazard_out, double* team_out, float* path_out, float* trace_out) {
  if (!resume || !teams || !team_out) return fail(MOBROB_ERR_INVALID, "follow: teams: null argument");
  if (hz && hzf) return fail(MOBROB_ERR_INVALID, "follow: teams: static hazards or hazard frames, not both");
  if ((hz || hzf) != (hazard_out != nullptr)) return fail(MOBROB_ERR_INVALID, "follow: teams: hazard_out is needed with hazards, and only then");
  const TeamIO tio{teams, team_out};
  mobrob_hazards_t view;
  const HazardIO hio = hzf ? hazard_frames_io(hzf, view, hazard_out, nullptr) : HazardIO{hz, hazard_out, nullptr};
  return follow_waypoints(e, env, spec, nullptr, waypoints, n_waypoints, arrival, robot_out, path_out, trace_out,
                          (hz || hzf) ? &hio : nullptr, resume, &tio);
}

int mobrob_ppo_follow_waypoints_scheduled(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                          const mobrob_hazards_t* hz, const mobrob_hazard_frames_t* hzf,
                                          const mobrob_follow_resume_t* resume, const mobrob_teams_t* teams,
                                          const mobrob_follow_schedule_t* schedule, const float* waypoints, const int32_t* n_waypoints,
                                          int32_t* arrival, double* robot_out, double* hazard_out, double* team_out, double* sched_out,
                                          float* path_out, float* trace_out) {
  if (!resume || !schedule || !sched_out) return fail(MOBROB_ERR_INVALID, "follow: schedule: null argument");
  if ((teams != nullptr) != (team_out != nullptr)) return fail(MOBROB_ERR_INVALID, "follow: schedule: team_out is needed with teams, and only then");
  if (hz && hzf) return fail(MOBROB_ERR_INVALID, "follow: schedule: static hazards or hazard frames, not both");
  if ((hz || hzf) != (hazard_out != nullptr)) return fail(MOBROB_ERR_INVALID, "follow: schedule: hazard_out is needed with hazards, and only then");
  const TeamIO tio{teams, team_out};
  const SchedIO sio{schedule, sched_out};
  mobrob_hazards_t view;
  const HazardIO hio = hzf ? hazard_frames_io(hzf, view, hazard_out, nullptr) : HazardIO{hz, hazard_out, nullptr};
  return follow_waypoints(e, env, spec, nullptr, waypoints, n_waypoints, arrival, robot_out, path_out, trace_out,
                          (hz || hzf) ? &hio : nullptr, resume, teams ? &tio : nullptr, &sio);
}

int mobrob_ppo_follow_waypoints_walls(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                      const mobrob_hazards_t* hz, const mobrob_hazard_frames_t* hzf, const mobrob_follow_resume_t* resume,
                                      const mobrob_teams_t* teams, const mobrob_follow_schedule_t* schedule, const mobrob_walls_t* walls,
                                      const float* waypoints, const int32_t* n_waypoints, int32_t* arrival, double* robot_out,
                                      double* hazard_out, double* team_out, double* sched_out, double* wall_out, float* path_out,
                                      float* trace_out) {
  if (!resume || !walls || !wall_out) return fail(MOBROB_ERR_INVALID, "follow: walls: null argument (a call with walls is a call of a run)");
  if ((teams != nullptr) != (team_out != nullptr)) return fail(MOBROB_ERR_INVALID, "follow: walls: team_out is needed with teams, and only then");
  if ((schedule != nullptr) != (sched_out != nullptr))
    return fail(MOBROB_ERR_INVALID, "follow: walls: sched_out is needed with a schedule, and only then");
  if (hz && hzf) return fail(MOBROB_ERR_INVALID, "follow: walls: static hazards or hazard frames, not both");
  if ((hz || hzf) != (hazard_out != nullptr)) return fail(MOBROB_ERR_INVALID, "follow: walls: hazard_out is needed with hazards, and only then");
  const TeamIO tio{teams, team_out};
  const SchedIO sio{schedule, sched_out};
  const WallIO wio{walls, wall_out};
  mobrob_hazards_t view;
  const HazardIO hio = hzf ? hazard_frames_io(hzf, view, hazard_out, nullptr) : HazardIO{hz, hazard_out, nullptr};
  return follow_waypoints(e, env, spec, nullptr, waypoints, n_waypoints, arrival, robot_out, path_out, trace_out,
                          (hz || hzf) ? &hio : nullptr, resume, teams ? &tio : nullptr, schedule ? &sio : nullptr, &wio);
}

int mobrob_ppo_follow_waypoints_solid(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                      const mobrob_hazards_t* hz, const mobrob_hazard_frames_t* hzf, const mobrob_follow_resume_t* resume,
                                      const mobrob_teams_t* teams, const mobrob_follow_schedule_t* schedule, const mobrob_walls_t* walls,
                                      const float* waypoints, const int32_t* n_waypoints, int32_t* arrival, double* robot_out,
                                      double* hazard_out, double* team_out, double* sched_out, double* wall_out, int32_t* blocked_out,
                                      float* path_out, float* trace_out) {
  if (!resume || !walls || !wall_out || !blocked_out)
    return fail(MOBROB_ERR_INVALID, "follow: solid: null argument (a call with walls is a call of a run)");
  if ((teams != nullptr) != (team_out != nullptr)) return fail(MOBROB_ERR_INVALID, "follow: solid: team_out is needed with teams, and only then");
  if ((schedule != nullptr) != (sched_out != nullptr))
    return fail(MOBROB_ERR_INVALID, "follow: solid: sched_out is needed with a schedule, and only then");
  if (hz && hzf) return fail(MOBROB_ERR_INVALID, "follow: solid: static hazards or hazard frames, not both");
  if ((hz || hzf) != (hazard_out != nullptr)) return fail(MOBROB_ERR_INVALID, "follow: solid: hazard_out is needed with hazards, and only then");
  const TeamIO tio{teams, team_out};
  const SchedIO sio{schedule, sched_out};
  const WallIO wio{walls, wall_out, blocked_out};
  mobrob_hazards_t view;
  const HazardIO hio = hzf ? hazard_frames_io(hzf, view, hazard_out, nullptr) : HazardIO{hz, hazard_out, nullptr};
  return follow_waypoints(e, env, spec, nullptr, waypoints, n_waypoints, arrival, robot_out, path_out, trace_out,
                          (hz || hzf) ? &hio : nullptr, resume, teams ? &tio : nullptr, schedule ? &sio : nullptr, &wio);
}

int mobrob_ppo_follow_waypoints_teams_solid(mobrob_ppo_engine_t* e, const mobrob_goal_env_t* env, const mobrob_follow_spec_t* spec,
                                            const mobrob_hazards_t* hz, const mobrob_hazard_frames_t* hzf,
                                            const mobrob_follow_resume_t* resume, const mobrob_teams_t* teams,
                                            const mobrob_follow_schedule_t* schedule, const mobrob_walls_t* walls, const float* waypoints,
                                            const int32_t* n_waypoints, int32_t* arrival, double* robot_out, double* hazard_out,
                                            double* team_out, double* sched_out, double* wall_out, int32_t* blocked_out,
                                            int32_t* team_blocked_out, float* path_out, float* trace_out) {
  if (!resume || !teams || !team_out || !team_blocked_out)
    return fail(MOBROB_ERR_INVALID, "follow: solid teams: null argument (a call with teams is a call of a run)");
  if ((schedule != nullptr) != (sched_out != nullptr))
    return fail(MOBROB_ERR_INVALID, "follow: solid teams: sched_out is needed with a schedule, and only then");
  if ((walls != nullptr) != (wall_out != nullptr))
    return fail(MOBROB_ERR_INVALID, "follow: solid teams: wall_out is needed with walls, and only then");
  if (walls && !blocked_out)
    return fail(MOBROB_ERR_INVALID, "follow: solid teams: solid teams do not run with observational walls yet (solid walls do: blocked_out)");
  if (!walls && blocked_out) return fail(MOBROB_ERR_INVALID, "follow: solid teams: blocked_out is needed with walls, and only then");
  if (hz && hzf) return fail(MOBROB_ERR_INVALID, "follow: solid teams: static hazards or hazard frames, not both");
  if ((hz || hzf) != (hazard_out != nullptr))
    return fail(MOBROB_ERR_INVALID, "follow: solid teams: hazard_out is needed with hazards, and only then");
  const TeamIO tio{teams, team_out, team_blocked_out};
  const SchedIO sio{schedule, sched_out};
  const WallIO wio{walls, wall_out, blocked_out};
  mobrob_hazards_t view;
  const HazardIO hio = hzf ? hazard_frames_io(hzf, view, hazard_out, nullptr) : HazardIO{hz, hazard_out, nullptr};
  return follow_waypoints(e, env, spec, nullptr, waypoints, n_waypoints, arrival, robot_out, path_out, trace_out,
                          (hz || hzf) ? &hio : nullptr, resume, &tio, schedule ? &sio : nullptr, walls ? &wio : nullptr);
}

// ---- grid planner (mobrob_ppo_plan_grid): walls and hazards to waypoints ---------------------------------------------------
// one of the planner's two device buffers, grown to `need` bytes (outside the arena, freed by destroy)
static int grow_plan_buf(mobrob_ppo_engine_t* e, char*& buf, size_t& bytes, size_t need) {
  if (need > bytes) {
    HIPC(hipStreamSynchronize(e->stream));
    if (buf) HIPC(hipFree(buf));
    buf = nullptr;
    bytes = 0;
    HIPC(hipMalloc(reinterpret_cast<void**>(&buf), need));
    bytes = need;
  }
  return MOBROB_OK;
}

// the resident part of a plan: occupancy | field | field_goal | field_scene | sweeps
struct PlanKeep {
  size_t occ, field, fgoal, fscene, sweeps, total;
  PlanKeep(int S, int F, int cells) {
    EvalCarve keep;
    occ = keep.add((size_t)S * cells); field = keep.add((size_t)F * cells * 4); fgoal = keep.add((size_t)F * 4);
    fscene = keep.add((size_t)F * 4); sweeps = keep.add((size_t)F * 4);
    total = keep.total;
  }
};

// what mobrob_ppo_plan_grid and mobrob_ppo_plan_grid_time check alike of the spec and the scenes (the walls' radius and the costs
// play no part); hz: the hazards, for a time plan the static view of its frames with their time axis in `frames`
static int plan_check_scenes(const char* who, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls, const mobrob_hazards_t* hz,
                             const HazardIO* frames, std::vector<int32_t>& wall_counts, std::vector<int32_t>& hz_counts) {
  const int N = spec->n_robots, P = spec->pos_dim, G = spec->cells, K = spec->max_waypoints, S = spec->n_scenes, F = spec->n_fields;
  if (N < 1) return fail(MOBROB_ERR_INVALID, "%s: n_robots must be >= 1", who);
  if (P != 2 && P != 3) return fail(MOBROB_ERR_INVALID, "%s: pos_dim must be 2 or 3 (the grid is x and y)", who);
  if (G != 32 && G != 64 && G != 128) return fail(MOBROB_ERR_INVALID, "%s: cells must be 32, 64 or 128, got %d", who, G);
  if (K < 1) return fail(MOBROB_ERR_INVALID, "%s: max_waypoints must be >= 1", who);
  if (F < 1 || F > N) return fail(MOBROB_ERR_INVALID, "%s: n_fields = %d outside 1 .. n_robots = %d", who, F, N);
  if (!(std::isfinite(spec->extent) && spec->extent > 0.f && std::isfinite(spec->h) && spec->h > 0.f && std::isfinite(spec->inv_h) &&
        spec->inv_h > 0.f && std::fabs((double)spec->h * (double)spec->inv_h - 1.0) <= 1e-5))
    return fail(MOBROB_ERR_INVALID, "%s: extent, h and inv_h must be finite and > 0 with h * inv_h = 1", who);
  if (!(std::isfinite(spec->inflate) && spec->inflate >= 0.f)) return fail(MOBROB_ERR_INVALID, "%s: inflate must be finite and >= 0", who);
  if ((int64_t)N * K * P > INT_MAX) return fail(MOBROB_ERR_INVALID, "%s: n_robots * max_waypoints * pos_dim must fit an int32", who);
  if (S != (walls ? walls->n_scenes : hz ? hz->n_scenes : 1) || (walls && hz && walls->n_scenes != hz->n_scenes))
    return fail(MOBROB_ERR_INVALID, "%s: n_scenes = %d is not the scenes' own (walls %d, hazards %d)", who, S, walls ? walls->n_scenes : -1,
                hz ? hz->n_scenes : -1);
  // the scenes, by the checks of the calls that take them (the walls' radius and the costs play no part here)
  if (walls) {
    const int M = walls->max_walls;
    if (S < 1) return fail(MOBROB_ERR_INVALID, "%s: walls: n_scenes must be >= 1", who);
    if (M < 0 || M > kWallMax) return fail(MOBROB_ERR_INVALID, "%s: walls: max_walls must lie in 0 .. %d", who, kWallMax);
    if (M > 0 && !walls->boxes) return fail(MOBROB_ERR_INVALID, "%s: walls: null box table", who);
    if (!walls->scene && S > 1) return fail(MOBROB_ERR_INVALID, "%s: walls: %d scenes need a scene index per robot", who, S);
    wall_counts.assign(S, M);
    for (int s = 0; s < S; ++s) {
      if (walls->n_walls) wall_counts[s] = walls->n_walls[s];
      if (wall_counts[s] < 0 || wall_counts[s] > M)
        return fail(MOBROB_ERR_INVALID, "%s: walls: n_walls[%d] = %d outside 0 .. %d", who, s, wall_counts[s], M);
      for (int i = 0; i < wall_counts[s]; ++i) {
        const float* b = walls->boxes + ((size_t)s * M + i) * 4;
        if (!(std::isfinite(b[0]) && std::isfinite(b[1]) && std::isfinite(b[2]) && std::isfinite(b[3]) && b[2] >= 0.f && b[3] >= 0.f))
          return fail(MOBROB_ERR_INVALID, "%s: walls: box %d of scene %d is not finite or has a negative half extent", who, i, s);
      }
    }
    if (walls->scene)
      for (int i = 0; i < N; ++i)
        if (walls->scene[i] < 0 || walls->scene[i] >= S)
          return fail(MOBROB_ERR_INVALID, "%s: walls: scene[%d] = %d outside 0 .. %d", who, i, walls->scene[i], S - 1);
  }
  if (hz) {
    mobrob_hazards_t view = *hz;
    view.cost = 0.f;   // (unused here: not refused)
    HazardIO hio = frames ? *frames : HazardIO{};
    hio.hz = &view; hio.hazard_out = nullptr; hio.episode_cost_out = nullptr;
    if (const int rc = hazard_check(hio, N, who, hz_counts)) return rc;
  }
  if (walls && hz) {
    if ((walls->scene != nullptr) != (hz->scene != nullptr))
      return fail(MOBROB_ERR_INVALID, "%s: walls and hazards must agree on the scene index per robot", who);
    for (int i = 0; walls->scene && i < N; ++i)
      if (walls->scene[i] != hz->scene[i])
        return fail(MOBROB_ERR_INVALID, "%s: walls and hazards disagree on the scene of robot %d (%d and %d)", who, i, walls->scene[i], hz->scene[i]);
  }
  return MOBROB_OK;
}

// ... and of the fields (check_fields: the caller's lists, not resident ones) and the robots
static int plan_check_robots(const char* who, const mobrob_plan_spec_t* spec, const int32_t* scene, const float* start, const float* goal,
                             const int32_t* field_of, const int32_t* field_goal_cell, const int32_t* field_scene, bool check_fields) {
  const int N = spec->n_robots, P = spec->pos_dim, G = spec->cells, S = spec->n_scenes, F = spec->n_fields, cells = G * G;
  if (check_fields)
    for (int f = 0; f < F; ++f) {
      if (field_scene[f] < 0 || field_scene[f] >= S)
        return fail(MOBROB_ERR_INVALID, "%s: field_scene[%d] = %d outside 0 .. %d", who, f, field_scene[f], S - 1);
      if (field_goal_cell[f] < 0 || field_goal_cell[f] >= cells)
        return fail(MOBROB_ERR_INVALID, "%s: field_goal_cell[%d] = %d outside 0 .. %d", who, f, field_goal_cell[f], cells - 1);
    }
  const auto cell_of = [&](float x) {   // plan_cell's arithmetic (kernels_plan.h); volatile: the sum is rounded to float before the product
    volatile float sum = x + spec->extent;
    volatile float c = sum * spec->inv_h;
    return (int)std::fmin(std::fmax(std::floor((float)c), 0.f), (float)(G - 1));
  };
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j < P; ++j)
      if (!std::isfinite(start[(size_t)i * P + j]) || !std::isfinite(goal[(size_t)i * P + j]))
        return fail(MOBROB_ERR_INVALID, "%s: start or goal of robot %d is not finite", who, i);
    const int f = field_of[i];
    if (f < 0 || f >= F) return fail(MOBROB_ERR_INVALID, "%s: field_of[%d] = %d outside 0 .. %d", who, i, f, F - 1);
    if (field_scene[f] != (scene ? scene[i] : 0))
      return fail(MOBROB_ERR_INVALID, "%s: robot %d is in scene %d, its field %d in scene %d", who, i, scene ? scene[i] : 0, f, field_scene[f]);
    const int gc = cell_of(goal[(size_t)i * P + 1]) * G + cell_of(goal[(size_t)i * P]);
    if (gc != field_goal_cell[f])
      return fail(MOBROB_ERR_INVALID, "%s: the goal of robot %d lies in cell %d, its field %d has goal cell %d", who, i, gc, f, field_goal_cell[f]);
  }
  return MOBROB_OK;
}

int mobrob_ppo_plan_grid(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls, const mobrob_hazards_t* hz,
                         const float* start, const float* goal, const int32_t* field_of, const int32_t* field_goal_cell,
                         const int32_t* field_scene, float* waypoints_out, int32_t* n_waypoints_out, int32_t* count_out,
                         int32_t* status_out, int32_t* cost_out, uint8_t* occupancy_out, int32_t* field_out, int32_t* sweeps_out,
                         int64_t* fields_id_out) {
  if (!e || !spec || !start || !goal || !field_of || !waypoints_out || !n_waypoints_out || !count_out || !status_out || !cost_out)
    return fail(MOBROB_ERR_INVALID, "plan: null argument");
  const bool reuse = spec->reuse_id != 0;
  if (!reuse && (!field_goal_cell || !field_scene)) return fail(MOBROB_ERR_INVALID, "plan: null argument");
  const int N = spec->n_robots, P = spec->pos_dim, G = spec->cells, K = spec->max_waypoints, S = spec->n_scenes, F = spec->n_fields;
  const int cells = G * G;
  std::vector<int32_t> wall_counts, hz_counts;
  if (const int rc = plan_check_scenes("plan", spec, walls, hz, nullptr, wall_counts, hz_counts)) return rc;
  const int32_t* scene = walls ? walls->scene : hz ? hz->scene : nullptr;
  if (reuse) {
    if (spec->reuse_id != e->plan_id || e->plan_id == 0)
      return fail(MOBROB_ERR_STATE, "plan: the fields of id %lld are no longer resident (resident: %lld)", (long long)spec->reuse_id,
                  (long long)e->plan_id);
    if (G != e->plan_G || S != e->plan_S || F != e->plan_F)
      return fail(MOBROB_ERR_INVALID, "plan: reuse: cells, n_scenes, n_fields = %d, %d, %d are not the resident fields' %d, %d, %d", G, S, F,
                  e->plan_G, e->plan_S, e->plan_F);
    field_goal_cell = e->plan_field_goal.data();
    field_scene = e->plan_field_scene.data();
  }
  if (const int rc = plan_check_robots("plan", spec, scene, start, goal, field_of, field_goal_cell, field_scene, !reuse)) return rc;
  const size_t field_lds = plan_field_lds_bytes(G);
  const int Mw = walls ? walls->max_walls : 0, Mh = hz ? hz->max_hazards : 0;
  if (!reuse) {   // the per-workgroup LDS limit, as the tile kernels' scenes are checked
    int limit = 0;
    if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, e->cfg.device_id) != hipSuccess) limit = 64 * 1024;
    if (field_lds > (size_t)limit)
      return fail(MOBROB_ERR_INVALID, "plan: k_plan_field needs %zu bytes of LDS at %d cells, the device allows %d per workgroup", field_lds, G, limit);
  }
  const PlanKeep keep(S, F, cells);
  const size_t o_occ = keep.occ, o_field = keep.field, o_fgoal = keep.fgoal, o_fscene = keep.fscene, o_sweeps = keep.sweeps;
  // the call's part
  EvalCarve call;
  const size_t o_start = call.add((size_t)N * P * 4), o_goal = call.add((size_t)N * P * 4), o_fof = call.add((size_t)N * 4),
               o_wp = call.add((size_t)N * K * P * 4), o_nwp = call.add((size_t)N * 4), o_count = call.add((size_t)N * 4),
               o_status = call.add((size_t)N * 4), o_cost = call.add((size_t)N * 4),
               o_box = call.add(std::max<size_t>((size_t)S * Mw * 4, 1) * 4), o_nwall = call.add((size_t)S * 4),
               o_hz = call.add(std::max<size_t>((size_t)S * Mh * 3, 1) * 4), o_nhz = call.add((size_t)S * 4);
  if (!reuse) {
    e->plan_id = 0;   // whatever was resident is gone from here on
    if (const int rc = grow_plan_buf(e, e->plan_fields, e->plan_fields_bytes, keep.total)) return rc;
  }
  if (const int rc = grow_plan_buf(e, e->plan_buf, e->plan_bytes, call.total)) return rc;
  const auto kept = [&](size_t off) { return e->plan_fields + off; };
  const auto mine = [&](size_t off) { return e->plan_buf + off; };
  unsigned char* occ_dev = reinterpret_cast<unsigned char*>(kept(o_occ));
  int* field_dev = reinterpret_cast<int*>(kept(o_field));
  int* fgoal_dev = reinterpret_cast<int*>(kept(o_fgoal));
  int* fscene_dev = reinterpret_cast<int*>(kept(o_fscene));
  int* sweeps_dev = reinterpret_cast<int*>(kept(o_sweeps));
  const PlanGrid grid{G, spec->extent, spec->h, spec->inv_h, spec->inflate};
  if (!reuse) {
    PlanOccArgs oa{};
    oa.g = grid; oa.Mw = Mw; oa.Mh = Mh; oa.occ = occ_dev;
    if (walls) {
      float* box_dev = reinterpret_cast<float*>(mine(o_box));
      int* cnt_dev = reinterpret_cast<int*>(mine(o_nwall));
      if ((size_t)S * Mw) HIPC(hipMemcpyAsync(box_dev, walls->boxes, (size_t)S * Mw * 16, hipMemcpyHostToDevice, e->stream));
      HIPC(hipMemcpyAsync(cnt_dev, wall_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
      oa.boxes = box_dev; oa.nwall = cnt_dev;
    }
    if (hz) {
      float* hz_dev = reinterpret_cast<float*>(mine(o_hz));
      int* cnt_dev = reinterpret_cast<int*>(mine(o_nhz));
      if ((size_t)S * Mh) HIPC(hipMemcpyAsync(hz_dev, hz->hazards, (size_t)S * Mh * 12, hipMemcpyHostToDevice, e->stream));
      HIPC(hipMemcpyAsync(cnt_dev, hz_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
      oa.hz = hz_dev; oa.nhz = cnt_dev;
    }
    HIPC(hipMemcpyAsync(fgoal_dev, field_goal_cell, (size_t)F * 4, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(fscene_dev, field_scene, (size_t)F * 4, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_plan_occupancy, dim3(cdiv(cells, 256), S), dim3(256), ((size_t)4 * Mw + 3 * Mh) * sizeof(float), e->stream, oa);
    if (!e->plan_lds_set) {   // 80 KB at 128 cells: above the 64 KB a kernel gets without asking
      HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_plan_field), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)plan_field_lds_bytes(128)));
      e->plan_lds_set = true;
    }
    const PlanFieldArgs fa{G, occ_dev, fgoal_dev, fscene_dev, field_dev, sweeps_dev};
    hipLaunchKernelGGL(k_plan_field, dim3(F), dim3(kPlanFieldThreads), field_lds, e->stream, fa);
    HIPC(hipGetLastError());
  }
  PlanPathArgs pa{};
  pa.g = grid; pa.N = N; pa.K = K; pa.P = P;
  float* start_dev = reinterpret_cast<float*>(mine(o_start));
  float* goal_dev = reinterpret_cast<float*>(mine(o_goal));
  int* fof_dev = reinterpret_cast<int*>(mine(o_fof));
  pa.start = start_dev; pa.goal = goal_dev; pa.field_of = fof_dev;
  pa.field_scene = fscene_dev; pa.sweeps = sweeps_dev; pa.occ = occ_dev; pa.field = field_dev;
  pa.wp = reinterpret_cast<float*>(mine(o_wp));
  pa.nwp = reinterpret_cast<int*>(mine(o_nwp)); pa.count = reinterpret_cast<int*>(mine(o_count));
  pa.status = reinterpret_cast<int*>(mine(o_status)); pa.cost = reinterpret_cast<int*>(mine(o_cost));
  HIPC(hipMemcpyAsync(start_dev, start, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(goal_dev, goal, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(fof_dev, field_of, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemsetAsync(pa.wp, 0, (size_t)N * K * P * 4, e->stream));
  hipLaunchKernelGGL(k_plan_path, dim3(cdiv(N, 256)), dim3(256), 0, e->stream, pa);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(waypoints_out, pa.wp, (size_t)N * K * P * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(n_waypoints_out, pa.nwp, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(count_out, pa.count, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(status_out, pa.status, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(cost_out, pa.cost, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  if (occupancy_out) HIPC(hipMemcpyAsync(occupancy_out, occ_dev, (size_t)S * cells, hipMemcpyDeviceToHost, e->stream));
  if (field_out) HIPC(hipMemcpyAsync(field_out, field_dev, (size_t)F * cells * 4, hipMemcpyDeviceToHost, e->stream));
  if (sweeps_out) HIPC(hipMemcpyAsync(sweeps_out, sweeps_dev, (size_t)F * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  if (!reuse) {   // resident from here on
    static int64_t next_id = 0;
    e->plan_id = ++next_id;
    e->plan_G = G; e->plan_S = S; e->plan_F = F;
    e->plan_field_goal.assign(field_goal_cell, field_goal_cell + F);
    e->plan_field_scene.assign(field_scene, field_scene + F);
  }
  if (fields_id_out) *fields_id_out = e->plan_id;
  return MOBROB_OK;
}

int mobrob_ppo_plan_smooth(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, int32_t margin, const float* start, const float* goal,
                           const int32_t* field_of, const int32_t* scene, float* waypoints_out, int32_t* n_waypoints_out,
                           int32_t* count_out, int32_t* status_out, int32_t* cost_out, int32_t* moves_out) {
  if (!e || !spec || !start || !goal || !field_of || !waypoints_out || !n_waypoints_out || !count_out || !status_out || !cost_out ||
      !moves_out)
    return fail(MOBROB_ERR_INVALID, "plan_smooth: null argument");
  const int N = spec->n_robots, P = spec->pos_dim, G = spec->cells, K = spec->max_waypoints, S = spec->n_scenes, F = spec->n_fields;
  if (margin != 0 && margin != 1) return fail(MOBROB_ERR_INVALID, "plan_smooth: margin must be 0 or 1, got %d", margin);
  if (N < 1) return fail(MOBROB_ERR_INVALID, "plan_smooth: n_robots must be >= 1");
  if (P != 2 && P != 3) return fail(MOBROB_ERR_INVALID, "plan_smooth: pos_dim must be 2 or 3 (the grid is x and y)");
  if (G != 32 && G != 64 && G != 128) return fail(MOBROB_ERR_INVALID, "plan_smooth: cells must be 32, 64 or 128, got %d", G);
  if (K < 1) return fail(MOBROB_ERR_INVALID, "plan_smooth: max_waypoints must be >= 1");
  if (F < 1 || F > N) return fail(MOBROB_ERR_INVALID, "plan_smooth: n_fields = %d outside 1 .. n_robots = %d", F, N);
  if (S < 1) return fail(MOBROB_ERR_INVALID, "plan_smooth: n_scenes must be >= 1");
  if (!(std::isfinite(spec->extent) && spec->extent > 0.f && std::isfinite(spec->h) && spec->h > 0.f && std::isfinite(spec->inv_h) &&
        spec->inv_h > 0.f && std::fabs((double)spec->h * (double)spec->inv_h - 1.0) <= 1e-5))
    return fail(MOBROB_ERR_INVALID, "plan_smooth: extent, h and inv_h must be finite and > 0 with h * inv_h = 1");
  if ((int64_t)N * K * P > INT_MAX) return fail(MOBROB_ERR_INVALID, "plan_smooth: n_robots * max_waypoints * pos_dim must fit an int32");
  if (spec->reuse_id == 0 || spec->reuse_id != e->plan_id)
    return fail(MOBROB_ERR_STATE, "plan_smooth: the fields of id %lld are no longer resident (resident: %lld)", (long long)spec->reuse_id,
                (long long)e->plan_id);
  if (G != e->plan_G || S != e->plan_S || F != e->plan_F)
    return fail(MOBROB_ERR_INVALID, "plan_smooth: cells, n_scenes, n_fields = %d, %d, %d are not the resident fields' %d, %d, %d", G, S, F,
                e->plan_G, e->plan_S, e->plan_F);
  if (!scene && S > 1) return fail(MOBROB_ERR_INVALID, "plan_smooth: %d scenes need a scene index per robot", S);
  const int cells = G * G;
  const auto cell_of = [&](float x) {   // plan_cell's arithmetic (kernels_plan.h); volatile: the sum is rounded to float before the product
    volatile float sum = x + spec->extent;
    volatile float c = sum * spec->inv_h;
    return (int)std::fmin(std::fmax(std::floor((float)c), 0.f), (float)(G - 1));
  };
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j < P; ++j)
      if (!std::isfinite(start[(size_t)i * P + j]) || !std::isfinite(goal[(size_t)i * P + j]))
        return fail(MOBROB_ERR_INVALID, "plan_smooth: start or goal of robot %d is not finite", i);
    const int sc = scene ? scene[i] : 0;
    if (sc < 0 || sc >= S) return fail(MOBROB_ERR_INVALID, "plan_smooth: scene[%d] = %d outside 0 .. %d", i, sc, S - 1);
    const int f = field_of[i];
    if (f < 0 || f >= F) return fail(MOBROB_ERR_INVALID, "plan_smooth: field_of[%d] = %d outside 0 .. %d", i, f, F - 1);
    if (e->plan_field_scene[f] != sc)
      return fail(MOBROB_ERR_INVALID, "plan_smooth: robot %d is in scene %d, its field %d in scene %d", i, sc, f, e->plan_field_scene[f]);
    const int gc = cell_of(goal[(size_t)i * P + 1]) * G + cell_of(goal[(size_t)i * P]);
    if (gc != e->plan_field_goal[f])
      return fail(MOBROB_ERR_INVALID, "plan_smooth: the goal of robot %d lies in cell %d, its field %d has goal cell %d", i, gc, f,
                  e->plan_field_goal[f]);
  }
  const PlanKeep keep(S, F, cells);
  EvalCarve call;
  const size_t o_start = call.add((size_t)N * P * 4), o_goal = call.add((size_t)N * P * 4), o_fof = call.add((size_t)N * 4),
               o_wp = call.add((size_t)N * K * P * 4), o_nwp = call.add((size_t)N * 4), o_count = call.add((size_t)N * 4),
               o_status = call.add((size_t)N * 4), o_cost = call.add((size_t)N * 4), o_moves = call.add((size_t)N * 4);
  if (const int rc = grow_plan_buf(e, e->plan_buf, e->plan_bytes, call.total)) return rc;
  unsigned char* occ_dev = reinterpret_cast<unsigned char*>(e->plan_fields + keep.occ);
  const unsigned char* blk_dev = occ_dev;
  if (margin == 1) {
    if (e->plan_dil_id != e->plan_id) {   // once per set of resident fields
      e->plan_dil_id = 0;
      if (const int rc = grow_plan_buf(e, e->plan_dil, e->plan_dil_bytes, (size_t)S * cells)) return rc;
      const PlanDilateArgs da{G, occ_dev, reinterpret_cast<unsigned char*>(e->plan_dil)};
      hipLaunchKernelGGL(k_plan_dilate, dim3(cdiv(cells, 256), S), dim3(256), 0, e->stream, da);
      HIPC(hipGetLastError());
      e->plan_dil_id = e->plan_id;
    }
    blk_dev = reinterpret_cast<const unsigned char*>(e->plan_dil);
  }
  const auto mine = [&](size_t off) { return e->plan_buf + off; };
  PlanSmoothArgs sa{};
  PlanPathArgs& pa = sa.p;
  pa.g = PlanGrid{G, spec->extent, spec->h, spec->inv_h, spec->inflate};
  pa.N = N; pa.K = K; pa.P = P;
  float* start_dev = reinterpret_cast<float*>(mine(o_start));
  float* goal_dev = reinterpret_cast<float*>(mine(o_goal));
  int* fof_dev = reinterpret_cast<int*>(mine(o_fof));
  pa.start = start_dev; pa.goal = goal_dev; pa.field_of = fof_dev;
  pa.field_scene = reinterpret_cast<int*>(e->plan_fields + keep.fscene);
  pa.sweeps = reinterpret_cast<int*>(e->plan_fields + keep.sweeps);
  pa.occ = occ_dev;
  pa.field = reinterpret_cast<int*>(e->plan_fields + keep.field);
  pa.wp = reinterpret_cast<float*>(mine(o_wp));
  pa.nwp = reinterpret_cast<int*>(mine(o_nwp)); pa.count = reinterpret_cast<int*>(mine(o_count));
  pa.status = reinterpret_cast<int*>(mine(o_status)); pa.cost = reinterpret_cast<int*>(mine(o_cost));
  sa.blk = blk_dev;
  sa.moves = reinterpret_cast<int*>(mine(o_moves));
  HIPC(hipMemcpyAsync(start_dev, start, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(goal_dev, goal, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(fof_dev, field_of, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemsetAsync(pa.wp, 0, (size_t)N * K * P * 4, e->stream));
  hipLaunchKernelGGL(k_plan_smooth, dim3(N), dim3(64), 0, e->stream, sa);   // a wave per robot
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(waypoints_out, pa.wp, (size_t)N * K * P * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(n_waypoints_out, pa.nwp, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(count_out, pa.count, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(status_out, pa.status, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(cost_out, pa.cost, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(moves_out, sa.moves, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}

// ---- clearance-aware static plans (mobrob_ppo_plan_grid_clear, mobrob_ppo_plan_smooth_clear) ------------------------------------
constexpr int64_t kPlanClearIdBit = (int64_t)1 << 62;   // set in every id of this family, in none of mobrob_ppo_plan_grid's

// the resident part of a clearance-aware plan: occupancy | surcharge | margin-1 map | field | field_goal | field_scene | sweeps
struct PlanClearKeep {
  size_t occ, pen, dil, field, fgoal, fscene, sweeps, total;
  PlanClearKeep(int S, int F, int cells) {
    EvalCarve keep;
    occ = keep.add((size_t)S * cells); pen = keep.add((size_t)S * cells); dil = keep.add((size_t)S * cells);
    field = keep.add((size_t)F * cells * 4); fgoal = keep.add((size_t)F * 4); fscene = keep.add((size_t)F * 4);
    sweeps = keep.add((size_t)F * 4);
    total = keep.total;
  }
};

static int plan_clear_check_costs(const char* who, int reach, int weight) {
  if (reach < 1 || reach > kPlanClearReachMax)
    return fail(MOBROB_ERR_INVALID, "%s: reach must lie in 1 .. %d, got %d", who, kPlanClearReachMax, reach);
  if (weight < 1 || weight > kPlanClearWeightMax)
    return fail(MOBROB_ERR_INVALID, "%s: weight must lie in 1 .. %d, got %d", who, kPlanClearWeightMax, weight);
  return MOBROB_OK;
}

// is spec->reuse_id the resident clearance fields' own, with their shape?
static int plan_clear_check_resident(const char* who, const mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec) {
  if (spec->reuse_id == 0 || spec->reuse_id != e->plan_clear_id)
    return fail(MOBROB_ERR_STATE, "%s: the clearance fields of id %lld are not resident (resident: %lld; an id of mobrob_ppo_plan_grid's "
                "names fields of the other family)", who, (long long)spec->reuse_id, (long long)e->plan_clear_id);
  if (spec->cells != e->plan_clear_G || spec->n_scenes != e->plan_clear_S || spec->n_fields != e->plan_clear_F)
    return fail(MOBROB_ERR_INVALID, "%s: reuse: cells, n_scenes, n_fields = %d, %d, %d are not the resident fields' %d, %d, %d", who, spec->cells,
                spec->n_scenes, spec->n_fields, e->plan_clear_G, e->plan_clear_S, e->plan_clear_F);
  return MOBROB_OK;
}

int mobrob_ppo_plan_grid_clear(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls, const mobrob_hazards_t* hz,
                               int32_t reach, int32_t weight, const float* start, const float* goal, const int32_t* field_of,
                               const int32_t* field_goal_cell, const int32_t* field_scene, float* waypoints_out, int32_t* n_waypoints_out,
                               int32_t* count_out, int32_t* status_out, int32_t* cost_out, int32_t* clearance_min_out, uint8_t* occupancy_out,
                               int32_t* field_out, int32_t* sweeps_out, uint8_t* surcharge_out, int64_t* fields_id_out) {
  const char* who = "plan_grid_clear";
  if (!e || !spec || !start || !goal || !field_of || !waypoints_out || !n_waypoints_out || !count_out || !status_out || !cost_out ||
      !clearance_min_out)
    return fail(MOBROB_ERR_INVALID, "%s: null argument", who);
  const bool reuse = spec->reuse_id != 0;
  if (!reuse && (!field_goal_cell || !field_scene)) return fail(MOBROB_ERR_INVALID, "%s: null argument", who);
  if (const int rc = plan_clear_check_costs(who, reach, weight)) return rc;
  const int N = spec->n_robots, P = spec->pos_dim, G = spec->cells, K = spec->max_waypoints, S = spec->n_scenes, F = spec->n_fields;
  const int cells = G * G;
  std::vector<int32_t> wall_counts, hz_counts;
  if (const int rc = plan_check_scenes(who, spec, walls, hz, nullptr, wall_counts, hz_counts)) return rc;
  const int32_t* scene = walls ? walls->scene : hz ? hz->scene : nullptr;
  if (reuse) {
    if (const int rc = plan_clear_check_resident(who, e, spec)) return rc;
    if (reach != e->plan_clear_reach || weight != e->plan_clear_weight)
      return fail(MOBROB_ERR_INVALID, "%s: reuse: reach, weight = %d, %d are not the resident fields' %d, %d", who, reach, weight,
                  e->plan_clear_reach, e->plan_clear_weight);
    field_goal_cell = e->plan_clear_field_goal.data();
    field_scene = e->plan_clear_field_scene.data();
  }
  if (const int rc = plan_check_robots(who, spec, scene, start, goal, field_of, field_goal_cell, field_scene, !reuse)) return rc;
  const size_t field_lds = plan_field_cost_lds_bytes(G);
  const int Mw = walls ? walls->max_walls : 0, Mh = hz ? hz->max_hazards : 0;
  if (!reuse) {   // the per-workgroup LDS limit, as mobrob_ppo_plan_grid checks k_plan_field's
    int limit = 0;
    if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, e->cfg.device_id) != hipSuccess) limit = 64 * 1024;
    if (field_lds > (size_t)limit)
      return fail(MOBROB_ERR_INVALID, "%s: k_plan_field_cost needs %zu bytes of LDS at %d cells, the device allows %d per workgroup", who,
                  field_lds, G, limit);
  }
  const PlanClearKeep keep(S, F, cells);
  EvalCarve call;
  const size_t o_start = call.add((size_t)N * P * 4), o_goal = call.add((size_t)N * P * 4), o_fof = call.add((size_t)N * 4),
               o_wp = call.add((size_t)N * K * P * 4), o_nwp = call.add((size_t)N * 4), o_count = call.add((size_t)N * 4),
               o_status = call.add((size_t)N * 4), o_cost = call.add((size_t)N * 4), o_cmin = call.add((size_t)N * 4),
               o_box = call.add(std::max<size_t>((size_t)S * Mw * 4, 1) * 4), o_nwall = call.add((size_t)S * 4),
               o_hz = call.add(std::max<size_t>((size_t)S * Mh * 3, 1) * 4), o_nhz = call.add((size_t)S * 4);
  if (!reuse) {
    e->plan_clear_id = 0;   // whatever was resident in this family is gone from here on
    if (const int rc = grow_plan_buf(e, e->plan_clear_fields, e->plan_clear_fields_bytes, keep.total)) return rc;
  }
  if (const int rc = grow_plan_buf(e, e->plan_buf, e->plan_bytes, call.total)) return rc;
  const auto kept = [&](size_t off) { return e->plan_clear_fields + off; };
  const auto mine = [&](size_t off) { return e->plan_buf + off; };
  unsigned char* occ_dev = reinterpret_cast<unsigned char*>(kept(keep.occ));
  unsigned char* pen_dev = reinterpret_cast<unsigned char*>(kept(keep.pen));
  int* field_dev = reinterpret_cast<int*>(kept(keep.field));
  int* fgoal_dev = reinterpret_cast<int*>(kept(keep.fgoal));
  int* fscene_dev = reinterpret_cast<int*>(kept(keep.fscene));
  int* sweeps_dev = reinterpret_cast<int*>(kept(keep.sweeps));
  const PlanGrid grid{G, spec->extent, spec->h, spec->inv_h, spec->inflate};
  if (!reuse) {
    PlanOccArgs oa{};
    oa.g = grid; oa.Mw = Mw; oa.Mh = Mh; oa.occ = occ_dev;
    if (walls) {
      float* box_dev = reinterpret_cast<float*>(mine(o_box));
      int* cnt_dev = reinterpret_cast<int*>(mine(o_nwall));
      if ((size_t)S * Mw) HIPC(hipMemcpyAsync(box_dev, walls->boxes, (size_t)S * Mw * 16, hipMemcpyHostToDevice, e->stream));
      HIPC(hipMemcpyAsync(cnt_dev, wall_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
      oa.boxes = box_dev; oa.nwall = cnt_dev;
    }
    if (hz) {
      float* hz_dev = reinterpret_cast<float*>(mine(o_hz));
      int* cnt_dev = reinterpret_cast<int*>(mine(o_nhz));
      if ((size_t)S * Mh) HIPC(hipMemcpyAsync(hz_dev, hz->hazards, (size_t)S * Mh * 12, hipMemcpyHostToDevice, e->stream));
      HIPC(hipMemcpyAsync(cnt_dev, hz_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
      oa.hz = hz_dev; oa.nhz = cnt_dev;
    }
    HIPC(hipMemcpyAsync(fgoal_dev, field_goal_cell, (size_t)F * 4, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(fscene_dev, field_scene, (size_t)F * 4, hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(k_plan_occupancy, dim3(cdiv(cells, 256), S), dim3(256), ((size_t)4 * Mw + 3 * Mh) * sizeof(float), e->stream, oa);
    const PlanSurchargeArgs ca{G, reach, weight, occ_dev, pen_dev};
    hipLaunchKernelGGL(k_plan_surcharge, dim3(S), dim3(kPlanFieldThreads), 0, e->stream, ca);   // a workgroup per scene
    if (!e->plan_clear_lds_set) {   // 96 KB at 128 cells: above the 64 KB a kernel gets without asking
      HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_plan_field_cost), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)plan_field_cost_lds_bytes(128)));
      e->plan_clear_lds_set = true;
    }
    const PlanFieldCostArgs fa{G, occ_dev, pen_dev, fgoal_dev, fscene_dev, field_dev, sweeps_dev};
    hipLaunchKernelGGL(k_plan_field_cost, dim3(F), dim3(kPlanFieldThreads), field_lds, e->stream, fa);
    HIPC(hipGetLastError());
  }
  PlanPathCostArgs ps{};
  PlanPathArgs& pa = ps.p;
  pa.g = grid; pa.N = N; pa.K = K; pa.P = P;
  float* start_dev = reinterpret_cast<float*>(mine(o_start));
  float* goal_dev = reinterpret_cast<float*>(mine(o_goal));
  int* fof_dev = reinterpret_cast<int*>(mine(o_fof));
  pa.start = start_dev; pa.goal = goal_dev; pa.field_of = fof_dev;
  pa.field_scene = fscene_dev; pa.sweeps = sweeps_dev; pa.occ = occ_dev; pa.field = field_dev;
  pa.wp = reinterpret_cast<float*>(mine(o_wp));
  pa.nwp = reinterpret_cast<int*>(mine(o_nwp)); pa.count = reinterpret_cast<int*>(mine(o_count));
  pa.status = reinterpret_cast<int*>(mine(o_status)); pa.cost = reinterpret_cast<int*>(mine(o_cost));
  ps.pen = pen_dev; ps.reach = reach; ps.weight = weight;
  ps.clearance_min = reinterpret_cast<int*>(mine(o_cmin));
  HIPC(hipMemcpyAsync(start_dev, start, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(goal_dev, goal, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(fof_dev, field_of, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemsetAsync(pa.wp, 0, (size_t)N * K * P * 4, e->stream));
  hipLaunchKernelGGL(k_plan_path_cost, dim3(cdiv(N, 256)), dim3(256), 0, e->stream, ps);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(waypoints_out, pa.wp, (size_t)N * K * P * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(n_waypoints_out, pa.nwp, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(count_out, pa.count, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(status_out, pa.status, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(cost_out, pa.cost, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(clearance_min_out, ps.clearance_min, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  if (occupancy_out) HIPC(hipMemcpyAsync(occupancy_out, occ_dev, (size_t)S * cells, hipMemcpyDeviceToHost, e->stream));
  if (surcharge_out) HIPC(hipMemcpyAsync(surcharge_out, pen_dev, (size_t)S * cells, hipMemcpyDeviceToHost, e->stream));
  if (field_out) HIPC(hipMemcpyAsync(field_out, field_dev, (size_t)F * cells * 4, hipMemcpyDeviceToHost, e->stream));
  if (sweeps_out) HIPC(hipMemcpyAsync(sweeps_out, sweeps_dev, (size_t)F * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  if (!reuse) {   // resident from here on
    static int64_t next_id = 0;
    e->plan_clear_id = kPlanClearIdBit | ++next_id;
    e->plan_clear_G = G; e->plan_clear_S = S; e->plan_clear_F = F;
    e->plan_clear_reach = reach; e->plan_clear_weight = weight;
    e->plan_clear_field_goal.assign(field_goal_cell, field_goal_cell + F);
    e->plan_clear_field_scene.assign(field_scene, field_scene + F);
  }
  if (fields_id_out) *fields_id_out = e->plan_clear_id;
  return MOBROB_OK;
}

int mobrob_ppo_plan_smooth_clear(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, int32_t margin, const float* start, const float* goal,
                                 const int32_t* field_of, const int32_t* scene, float* waypoints_out, int32_t* n_waypoints_out,
                                 int32_t* count_out, int32_t* status_out, int32_t* cost_out, int32_t* moves_out, int32_t* clearance_min_out) {
  const char* who = "plan_smooth_clear";
  if (!e || !spec || !start || !goal || !field_of || !waypoints_out || !n_waypoints_out || !count_out || !status_out || !cost_out ||
      !moves_out || !clearance_min_out)
    return fail(MOBROB_ERR_INVALID, "%s: null argument", who);
  const int N = spec->n_robots, P = spec->pos_dim, G = spec->cells, K = spec->max_waypoints, S = spec->n_scenes, F = spec->n_fields;
  if (margin != 0 && margin != 1) return fail(MOBROB_ERR_INVALID, "%s: margin must be 0 or 1, got %d", who, margin);
  if (N < 1) return fail(MOBROB_ERR_INVALID, "%s: n_robots must be >= 1", who);
  if (P != 2 && P != 3) return fail(MOBROB_ERR_INVALID, "%s: pos_dim must be 2 or 3 (the grid is x and y)", who);
  if (G != 32 && G != 64 && G != 128) return fail(MOBROB_ERR_INVALID, "%s: cells must be 32, 64 or 128, got %d", who, G);
  if (K < 1) return fail(MOBROB_ERR_INVALID, "%s: max_waypoints must be >= 1", who);
  if (F < 1 || F > N) return fail(MOBROB_ERR_INVALID, "%s: n_fields = %d outside 1 .. n_robots = %d", who, F, N);
  if (S < 1) return fail(MOBROB_ERR_INVALID, "%s: n_scenes must be >= 1", who);
  if (!(std::isfinite(spec->extent) && spec->extent > 0.f && std::isfinite(spec->h) && spec->h > 0.f && std::isfinite(spec->inv_h) &&
        spec->inv_h > 0.f && std::fabs((double)spec->h * (double)spec->inv_h - 1.0) <= 1e-5))
    return fail(MOBROB_ERR_INVALID, "%s: extent, h and inv_h must be finite and > 0 with h * inv_h = 1", who);
  if ((int64_t)N * K * P > INT_MAX) return fail(MOBROB_ERR_INVALID, "%s: n_robots * max_waypoints * pos_dim must fit an int32", who);
  if (const int rc = plan_clear_check_resident(who, e, spec)) return rc;
  if (!scene && S > 1) return fail(MOBROB_ERR_INVALID, "%s: %d scenes need a scene index per robot", who, S);
  for (int i = 0; scene && i < N; ++i)
    if (scene[i] < 0 || scene[i] >= S) return fail(MOBROB_ERR_INVALID, "%s: scene[%d] = %d outside 0 .. %d", who, i, scene[i], S - 1);
  if (const int rc = plan_check_robots(who, spec, scene, start, goal, field_of, e->plan_clear_field_goal.data(),
                                       e->plan_clear_field_scene.data(), false))
    return rc;
  const int cells = G * G;
  const PlanClearKeep keep(S, F, cells);
  EvalCarve call;
  const size_t o_start = call.add((size_t)N * P * 4), o_goal = call.add((size_t)N * P * 4), o_fof = call.add((size_t)N * 4),
               o_wp = call.add((size_t)N * K * P * 4), o_nwp = call.add((size_t)N * 4), o_count = call.add((size_t)N * 4),
               o_status = call.add((size_t)N * 4), o_cost = call.add((size_t)N * 4), o_moves = call.add((size_t)N * 4),
               o_cmin = call.add((size_t)N * 4);
  if (const int rc = grow_plan_buf(e, e->plan_buf, e->plan_bytes, call.total)) return rc;
  unsigned char* occ_dev = reinterpret_cast<unsigned char*>(e->plan_clear_fields + keep.occ);
  const unsigned char* blk_dev = occ_dev;
  if (margin == 1) {
    unsigned char* dil_dev = reinterpret_cast<unsigned char*>(e->plan_clear_fields + keep.dil);
    if (e->plan_clear_dil_id != e->plan_clear_id) {   // once per set of resident fields
      const PlanDilateArgs da{G, occ_dev, dil_dev};
      hipLaunchKernelGGL(k_plan_dilate, dim3(cdiv(cells, 256), S), dim3(256), 0, e->stream, da);
      HIPC(hipGetLastError());
      e->plan_clear_dil_id = e->plan_clear_id;
    }
    blk_dev = dil_dev;
  }
  const auto mine = [&](size_t off) { return e->plan_buf + off; };
  PlanSmoothCostArgs sa{};
  PlanPathArgs& pa = sa.c.p;
  pa.g = PlanGrid{G, spec->extent, spec->h, spec->inv_h, spec->inflate};
  pa.N = N; pa.K = K; pa.P = P;
  float* start_dev = reinterpret_cast<float*>(mine(o_start));
  float* goal_dev = reinterpret_cast<float*>(mine(o_goal));
  int* fof_dev = reinterpret_cast<int*>(mine(o_fof));
  pa.start = start_dev; pa.goal = goal_dev; pa.field_of = fof_dev;
  pa.field_scene = reinterpret_cast<int*>(e->plan_clear_fields + keep.fscene);
  pa.sweeps = reinterpret_cast<int*>(e->plan_clear_fields + keep.sweeps);
  pa.occ = occ_dev;
  pa.field = reinterpret_cast<int*>(e->plan_clear_fields + keep.field);
  pa.wp = reinterpret_cast<float*>(mine(o_wp));
  pa.nwp = reinterpret_cast<int*>(mine(o_nwp)); pa.count = reinterpret_cast<int*>(mine(o_count));
  pa.status = reinterpret_cast<int*>(mine(o_status)); pa.cost = reinterpret_cast<int*>(mine(o_cost));
  sa.c.pen = reinterpret_cast<unsigned char*>(e->plan_clear_fields + keep.pen);
  sa.c.reach = e->plan_clear_reach; sa.c.weight = e->plan_clear_weight;
  sa.c.clearance_min = reinterpret_cast<int*>(mine(o_cmin));
  sa.blk = blk_dev;
  sa.moves = reinterpret_cast<int*>(mine(o_moves));
  HIPC(hipMemcpyAsync(start_dev, start, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(goal_dev, goal, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(fof_dev, field_of, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemsetAsync(pa.wp, 0, (size_t)N * K * P * 4, e->stream));
  hipLaunchKernelGGL(k_plan_smooth_cost, dim3(N), dim3(64), 0, e->stream, sa);   // a wave per robot
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(waypoints_out, pa.wp, (size_t)N * K * P * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(n_waypoints_out, pa.nwp, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(count_out, pa.count, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(status_out, pa.status, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(cost_out, pa.cost, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(moves_out, sa.moves, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(clearance_min_out, sa.c.clearance_min, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}

// ---- grid planner over time (mobrob_ppo_plan_grid_time): moving hazards as layers, waits as release steps --------------------
// the frames of every layer, as goal_rules.grid_layer_frames states them (64-bit: step0 + (T + 1) * layer_steps fits an int32)
static void plan_layer_frames(const mobrob_hazard_frames_t* hz, const mobrob_plan_time_t* tm, std::vector<int32_t>& first,
                              std::vector<int32_t>& number) {
  const int64_t F = hz->n_frames, fs = hz->frame_steps, g0 = tm->step0, dl = tm->layer_steps;
  const int T = tm->layers;
  first.assign(T + 1, 0);
  number.assign(T + 1, 0);
  for (int t = 0; t < T; ++t) {
    const int64_t k_lo = (g0 + t * dl) / fs, k_hi = (g0 + (t + 1) * dl - 1) / fs;
    if (hz->loop) {
      first[t] = (int32_t)(k_lo % F);
      number[t] = (int32_t)std::min<int64_t>(k_hi - k_lo + 1, F);
    } else {
      first[t] = (int32_t)std::min<int64_t>(k_lo, F - 1);
      number[t] = (int32_t)(std::min<int64_t>(k_hi, F - 1) - first[t] + 1);
    }
  }
  first[T] = hz->loop ? 0 : (int32_t)std::min<int64_t>((g0 + T * dl) / fs, F - 1);
  number[T] = (int32_t)(F - first[T]);
}

// what mobrob_ppo_plan_grid_time_smooth adds to a time plan; null: mobrob_ppo_plan_grid_time itself
struct PlanTimeSmooth {
  int32_t margin;
  int32_t* moves_out;
  int16_t* next_blocked_out;   // or null
};

// a time plan: the checks, the layers and the fields of both entry points, then k_plan_path_time, or with `sm` the table of
// k_plan_next_blocked and k_plan_smooth_time in its place (waits_out may then be null; it is zeroed)
static int plan_time_run(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls,
                         const mobrob_hazard_frames_t* hzf, const mobrob_plan_time_t* tm, const float* start, const float* goal,
                         const int32_t* field_of, const int32_t* field_goal_cell, const int32_t* field_scene, float* waypoints_out,
                         int32_t* n_waypoints_out, int32_t* count_out, int32_t* status_out, int32_t* cost_out, int32_t* waits_out,
                         int32_t* leave_out, int32_t* arrive_out, uint8_t* occ_time_out, int32_t* fields_time_out, int32_t* sweeps_out,
                         const PlanTimeSmooth* sm) {
  if (!e || !spec || !hzf || !tm || !start || !goal || !field_of || !field_goal_cell || !field_scene || !waypoints_out ||
      !n_waypoints_out || !count_out || !status_out || !cost_out || (!sm && !waits_out) || !leave_out || !arrive_out ||
      (sm && !sm->moves_out))
    return fail(MOBROB_ERR_INVALID, "plan_time: null argument");
  if (spec->reuse_id != 0) return fail(MOBROB_ERR_INVALID, "plan_time: reuse_id must be 0 (a time plan keeps nothing resident)");
  if (sm && sm->margin != 0 && sm->margin != 1) return fail(MOBROB_ERR_INVALID, "plan_time: margin must be 0 or 1, got %d", sm->margin);
  const int N = spec->n_robots, P = spec->pos_dim, G = spec->cells, K = spec->max_waypoints, S = spec->n_scenes, F = spec->n_fields;
  const int cells = G * G, T = tm->layers;
  mobrob_hazards_t view;
  const HazardIO frames = hazard_frames_io(hzf, view, nullptr, nullptr);
  std::vector<int32_t> wall_counts, hz_counts;
  if (const int rc = plan_check_scenes("plan_time", spec, walls, &view, &frames, wall_counts, hz_counts)) return rc;
  if (S > 65535) return fail(MOBROB_ERR_INVALID, "plan_time: n_scenes = %d above 65535", S);
  if (const int rc = plan_check_robots("plan_time", spec, hzf->scene, start, goal, field_of, field_goal_cell, field_scene, true)) return rc;
  if (T < 1 || T > kPlanLayersMax) return fail(MOBROB_ERR_INVALID, "plan_time: layers must lie in 1 .. %d, got %d", kPlanLayersMax, T);
  if (tm->layer_steps < 1) return fail(MOBROB_ERR_INVALID, "plan_time: layer_steps must be >= 1, got %d", tm->layer_steps);
  if (tm->step0 < 0) return fail(MOBROB_ERR_INVALID, "plan_time: step0 must be >= 0, got %d", tm->step0);
  if ((int64_t)tm->step0 + (int64_t)(T + 1) * tm->layer_steps > INT_MAX)
    return fail(MOBROB_ERR_INVALID, "plan_time: step0 + (layers + 1) * layer_steps must fit an int32");
  if ((uint64_t)F * (uint64_t)(T + 1) * (uint64_t)cells * 4u > MOBROB_PLAN_TIME_MAX_BYTES)
    return fail(MOBROB_ERR_INVALID, "plan_time: time fields of %d x %d x %d x %d x 4 bytes exceed the cap of %u bytes (256 MiB)", F, T + 1, G, G,
                (unsigned)MOBROB_PLAN_TIME_MAX_BYTES);
  if (sm && ((uint64_t)F * 4u + (uint64_t)S * 2u) * (uint64_t)(T + 1) * (uint64_t)cells > MOBROB_PLAN_TIME_MAX_BYTES)
    return fail(MOBROB_ERR_INVALID, "plan_time: time fields of %d x %d x %d x %d x 4 bytes and the next-blocked table of %d x %d x %d x %d x 2 "
                "bytes exceed the cap of %u bytes (256 MiB)", F, T + 1, G, G, S, T + 1, G, G, (unsigned)MOBROB_PLAN_TIME_MAX_BYTES);
  const size_t field_lds = plan_field_time_lds_bytes(G);
  {   // the per-workgroup LDS limit, as mobrob_ppo_plan_grid checks k_plan_field's
    int limit = 0;
    if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, e->cfg.device_id) != hipSuccess) limit = 64 * 1024;
    if (field_lds > (size_t)limit)
      return fail(MOBROB_ERR_INVALID, "plan_time: k_plan_field_time needs %zu bytes of LDS at %d cells, the device allows %d per workgroup",
                  field_lds, G, limit);
  }
  std::vector<int32_t> lfirst, lnumber;
  plan_layer_frames(hzf, tm, lfirst, lnumber);
  const int Mw = walls ? walls->max_walls : 0, Mh = hzf->max_hazards, NF = hzf->n_frames;
  const size_t hz_floats = (size_t)S * NF * Mh * 3;
  EvalCarve call;
  const size_t o_occ = call.add((size_t)S * (T + 1) * cells), o_field = call.add((size_t)F * (T + 1) * cells * 4),
               o_fgoal = call.add((size_t)F * 4), o_fscene = call.add((size_t)F * 4), o_sweeps = call.add((size_t)F * 4),
               o_lfirst = call.add((size_t)(T + 1) * 4), o_lnumber = call.add((size_t)(T + 1) * 4),
               o_start = call.add((size_t)N * P * 4), o_goal = call.add((size_t)N * P * 4), o_fof = call.add((size_t)N * 4),
               o_wp = call.add((size_t)N * K * P * 4), o_nwp = call.add((size_t)N * 4), o_count = call.add((size_t)N * 4),
               o_status = call.add((size_t)N * 4), o_cost = call.add((size_t)N * 4), o_waits = call.add((size_t)N * K * 4),
               o_leave = call.add((size_t)N * K * 4), o_arrive = call.add((size_t)N * 4),
               o_box = call.add(std::max<size_t>((size_t)S * Mw * 4, 1) * 4), o_nwall = call.add((size_t)S * 4),
               o_hz = call.add(std::max<size_t>(hz_floats, 1) * 4), o_nhz = call.add((size_t)S * 4);
  const size_t maps = (size_t)S * (T + 1);   // smoothing: the dilated layers (margin 1), the next-blocked table, the moves
  const size_t o_dil = sm && sm->margin == 1 ? call.add(maps * cells) : 0, o_nb = sm ? call.add(maps * cells * 2) : 0,
               o_moves = sm ? call.add((size_t)N * 4) : 0;
  if (const int rc = grow_plan_buf(e, e->plan_time_buf, e->plan_time_bytes, call.total)) return rc;
  const auto mine = [&](size_t off) { return e->plan_time_buf + off; };
  unsigned char* occ_dev = reinterpret_cast<unsigned char*>(mine(o_occ));
  int* field_dev = reinterpret_cast<int*>(mine(o_field));
  int* fgoal_dev = reinterpret_cast<int*>(mine(o_fgoal));
  int* fscene_dev = reinterpret_cast<int*>(mine(o_fscene));
  int* sweeps_dev = reinterpret_cast<int*>(mine(o_sweeps));
  int* lfirst_dev = reinterpret_cast<int*>(mine(o_lfirst));
  int* lnumber_dev = reinterpret_cast<int*>(mine(o_lnumber));
  PlanOccTimeArgs oa{};
  oa.g = PlanGrid{G, spec->extent, spec->h, spec->inv_h, spec->inflate};
  oa.Mw = Mw; oa.Mh = Mh; oa.F = NF; oa.T = T; oa.layer_first = lfirst_dev; oa.layer_number = lnumber_dev; oa.occ = occ_dev;
  if (walls) {
    float* box_dev = reinterpret_cast<float*>(mine(o_box));
    int* cnt_dev = reinterpret_cast<int*>(mine(o_nwall));
    if ((size_t)S * Mw) HIPC(hipMemcpyAsync(box_dev, walls->boxes, (size_t)S * Mw * 16, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(cnt_dev, wall_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
    oa.boxes = box_dev; oa.nwall = cnt_dev;
  }
  float* hz_dev = reinterpret_cast<float*>(mine(o_hz));
  int* nhz_dev = reinterpret_cast<int*>(mine(o_nhz));
  if (hz_floats) HIPC(hipMemcpyAsync(hz_dev, hzf->hazards, hz_floats * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(nhz_dev, hz_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
  oa.hz = hz_dev; oa.nhz = nhz_dev;
  HIPC(hipMemcpyAsync(lfirst_dev, lfirst.data(), (size_t)(T + 1) * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(lnumber_dev, lnumber.data(), (size_t)(T + 1) * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(fgoal_dev, field_goal_cell, (size_t)F * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(fscene_dev, field_scene, (size_t)F * 4, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_plan_occupancy_time, dim3(cells / 256, T + 1, S), dim3(256), ((size_t)4 * Mw + 3 * Mh) * sizeof(float), e->stream, oa);
  if (!e->plan_time_lds_set) {   // 144 KB at 128 cells: above the 64 KB a kernel gets without asking
    HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_plan_field_time), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)plan_field_time_lds_bytes(128)));
    e->plan_time_lds_set = true;
  }
  const PlanFieldTimeArgs fa{G, T, occ_dev, fgoal_dev, fscene_dev, field_dev, sweeps_dev};
  hipLaunchKernelGGL(k_plan_field_time, dim3(F), dim3(kPlanFieldThreads), field_lds, e->stream, fa);
  HIPC(hipGetLastError());
  PlanSmoothTimeArgs sa{};
  if (sm) {   // the cells that are not clear in every layer, then the first layer from t on in which a cell is not clear
    const unsigned char* blk_dev = occ_dev;
    if (sm->margin == 1) {   // k_plan_dilate as it is, a layer a map: at most 65535 maps a launch (the grid's y)
      unsigned char* dil_dev = reinterpret_cast<unsigned char*>(mine(o_dil));
      for (size_t m0 = 0; m0 < maps; m0 += 65535) {
        const PlanDilateArgs da{G, occ_dev + m0 * cells, dil_dev + m0 * cells};
        hipLaunchKernelGGL(k_plan_dilate, dim3(cells / 256, (unsigned)std::min<size_t>(maps - m0, 65535)), dim3(256), 0, e->stream, da);
        HIPC(hipGetLastError());
      }
      blk_dev = dil_dev;
    }
    const PlanNextBlockedArgs na{G, T, blk_dev, reinterpret_cast<short*>(mine(o_nb))};
    hipLaunchKernelGGL(k_plan_next_blocked, dim3(cells / 256, S), dim3(256), 0, e->stream, na);
    HIPC(hipGetLastError());
    sa.T = T; sa.nb = na.nb;
    sa.leave = reinterpret_cast<int*>(mine(o_leave)); sa.arrive = reinterpret_cast<int*>(mine(o_arrive));
    sa.moves = reinterpret_cast<int*>(mine(o_moves));
  }
  PlanPathTimeArgs ta{};
  PlanPathArgs& pa = ta.p;
  pa.g = oa.g; pa.N = N; pa.K = K; pa.P = P;
  float* start_dev = reinterpret_cast<float*>(mine(o_start));
  float* goal_dev = reinterpret_cast<float*>(mine(o_goal));
  int* fof_dev = reinterpret_cast<int*>(mine(o_fof));
  pa.start = start_dev; pa.goal = goal_dev; pa.field_of = fof_dev;
  pa.field_scene = fscene_dev; pa.sweeps = sweeps_dev; pa.occ = occ_dev; pa.field = field_dev;
  pa.wp = reinterpret_cast<float*>(mine(o_wp));
  pa.nwp = reinterpret_cast<int*>(mine(o_nwp)); pa.count = reinterpret_cast<int*>(mine(o_count));
  pa.status = reinterpret_cast<int*>(mine(o_status)); pa.cost = reinterpret_cast<int*>(mine(o_cost));
  ta.T = T;
  ta.waits = reinterpret_cast<int*>(mine(o_waits)); ta.leave = reinterpret_cast<int*>(mine(o_leave));
  ta.arrive = reinterpret_cast<int*>(mine(o_arrive));
  HIPC(hipMemcpyAsync(start_dev, start, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(goal_dev, goal, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(fof_dev, field_of, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemsetAsync(pa.wp, 0, (size_t)N * K * P * 4, e->stream));
  HIPC(hipMemsetAsync(ta.waits, 0, (size_t)N * K * 4, e->stream));
  HIPC(hipMemsetAsync(ta.leave, 0, (size_t)N * K * 4, e->stream));
  if (sm) {
    sa.p = pa;
    hipLaunchKernelGGL(k_plan_smooth_time, dim3(N), dim3(64), 0, e->stream, sa);   // a wave per robot
  } else {
    hipLaunchKernelGGL(k_plan_path_time, dim3(cdiv(N, 64)), dim3(64), 0, e->stream, ta);
  }
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(waypoints_out, pa.wp, (size_t)N * K * P * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(n_waypoints_out, pa.nwp, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(count_out, pa.count, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(status_out, pa.status, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(cost_out, pa.cost, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  if (waits_out) HIPC(hipMemcpyAsync(waits_out, ta.waits, (size_t)N * K * 4, hipMemcpyDeviceToHost, e->stream));   // (smoothed: the zeroes)
  HIPC(hipMemcpyAsync(leave_out, ta.leave, (size_t)N * K * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(arrive_out, ta.arrive, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  if (sm) {
    HIPC(hipMemcpyAsync(sm->moves_out, sa.moves, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
    if (sm->next_blocked_out) HIPC(hipMemcpyAsync(sm->next_blocked_out, sa.nb, maps * cells * 2, hipMemcpyDeviceToHost, e->stream));
  }
  if (occ_time_out) HIPC(hipMemcpyAsync(occ_time_out, occ_dev, (size_t)S * (T + 1) * cells, hipMemcpyDeviceToHost, e->stream));
  if (fields_time_out) HIPC(hipMemcpyAsync(fields_time_out, field_dev, (size_t)F * (T + 1) * cells * 4, hipMemcpyDeviceToHost, e->stream));
  if (sweeps_out) HIPC(hipMemcpyAsync(sweeps_out, sweeps_dev, (size_t)F * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}

int mobrob_ppo_plan_grid_time(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls,
                              const mobrob_hazard_frames_t* hzf, const mobrob_plan_time_t* tm, const float* start, const float* goal,
                              const int32_t* field_of, const int32_t* field_goal_cell, const int32_t* field_scene, float* waypoints_out,
                              int32_t* n_waypoints_out, int32_t* count_out, int32_t* status_out, int32_t* cost_out, int32_t* waits_out,
                              int32_t* leave_out, int32_t* arrive_out, uint8_t* occ_time_out, int32_t* fields_time_out,
                              int32_t* sweeps_out) {
  return plan_time_run(e, spec, walls, hzf, tm, start, goal, field_of, field_goal_cell, field_scene, waypoints_out, n_waypoints_out, count_out,
                       status_out, cost_out, waits_out, leave_out, arrive_out, occ_time_out, fields_time_out, sweeps_out, nullptr);
}

// ---- line-of-sight smoothing of a time plan (mobrob_ppo_plan_grid_time_smooth): a leg is tested against every layer it spans --
int mobrob_ppo_plan_grid_time_smooth(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls,
                                     const mobrob_hazard_frames_t* hzf, const mobrob_plan_time_t* tm, int32_t margin, const float* start,
                                     const float* goal, const int32_t* field_of, const int32_t* field_goal_cell, const int32_t* field_scene,
                                     float* waypoints_out, int32_t* n_waypoints_out, int32_t* count_out, int32_t* status_out,
                                     int32_t* cost_out, int32_t* waits_out, int32_t* leave_out, int32_t* arrive_out, int32_t* moves_out,
                                     uint8_t* occ_time_out, int32_t* fields_time_out, int32_t* sweeps_out, int16_t* next_blocked_out) {
  const PlanTimeSmooth sm{margin, moves_out, next_blocked_out};
  return plan_time_run(e, spec, walls, hzf, tm, start, goal, field_of, field_goal_cell, field_scene, waypoints_out, n_waypoints_out, count_out,
                       status_out, cost_out, waits_out, leave_out, arrive_out, occ_time_out, fields_time_out, sweeps_out, &sm);
}

// ---- prioritised planning inside a team (mobrob_ppo_plan_grid_team): a mate's planned walk as one more moving obstacle ---------
// what mobrob_ppo_plan_grid_team_smooth adds to a team plan
struct PlanTeamSmooth {
  int32_t margin, max_leg;
  int32_t* moves_out;
  int32_t* keep_out;   // [N][keep_cap] or null
  int32_t keep_cap;
};

// what mobrob_ppo_plan_grid_team_rounds adds to a team plan
struct PlanTeamRounds {
  int32_t retries;
  int32_t* order_out;          // [n_teams][team_size]
  int32_t* rounds_out;         // [n_teams]
  int32_t* parked_out;         // [n_teams]
  int32_t* parked_first_out;   // [n_teams]
};

// mobrob_ppo_plan_grid_team (sm and rr null: k_plan_team), mobrob_ppo_plan_grid_team_smooth (sm: k_plan_team_smooth) and
// mobrob_ppo_plan_grid_team_rounds (rr: k_plan_team_rounds): one set of checks
static int plan_team_run(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls,
                         const mobrob_hazard_frames_t* hzf, const mobrob_plan_time_t* tm, int32_t team_size, int32_t reserve,
                         const float* start, const float* goal, float* waypoints_out, int32_t* n_waypoints_out, int32_t* count_out,
                         int32_t* status_out, int32_t* cost_out, int32_t* waits_out, int32_t* leave_out, int32_t* arrive_out,
                         int32_t* sweeps_out, uint16_t* walk_out, int32_t walk_cap, uint8_t* occ_time_out, int32_t* fields_team_out,
                         int32_t* workgroups_out, const PlanTeamSmooth* sm, const PlanTeamRounds* rr = nullptr) {
  if (!e || !spec || !tm || !start || !goal || !waypoints_out || !n_waypoints_out || !count_out || !status_out || !cost_out || !waits_out ||
      !leave_out || !arrive_out)
    return fail(MOBROB_ERR_INVALID, "plan_team: null argument");
  if (sm) {
    if (!sm->moves_out) return fail(MOBROB_ERR_INVALID, "plan_team: null argument");
    if (sm->margin != 0 && sm->margin != 1) return fail(MOBROB_ERR_INVALID, "plan_team: line-of-sight margin must be 0 or 1, got %d", sm->margin);
    if (sm->max_leg < 1) return fail(MOBROB_ERR_INVALID, "plan_team: max_leg must be >= 1, got %d", sm->max_leg);
    if (sm->keep_out && sm->keep_cap < 1) return fail(MOBROB_ERR_INVALID, "plan_team: keep_cap must be >= 1 with keep_out");
    if (sm->keep_out && (int64_t)spec->n_robots * sm->keep_cap > INT_MAX) return fail(MOBROB_ERR_INVALID, "plan_team: n_robots * keep_cap must fit an int32");
  }
  if (rr) {
    if (!rr->order_out || !rr->rounds_out || !rr->parked_out || !rr->parked_first_out) return fail(MOBROB_ERR_INVALID, "plan_team: null argument");
    if (rr->retries < 0 || rr->retries > kPlanRetriesMax)
      return fail(MOBROB_ERR_INVALID, "plan_team: retries must lie in 0 .. %d, got %d", kPlanRetriesMax, rr->retries);
  }
  if (spec->reuse_id != 0) return fail(MOBROB_ERR_INVALID, "plan_team: reuse_id must be 0 (a team plan keeps nothing resident)");
  const int N = spec->n_robots, P = spec->pos_dim, G = spec->cells, K = spec->max_waypoints, S = spec->n_scenes;
  const int cells = G * G, T = tm->layers;
  mobrob_hazards_t view;
  HazardIO frames{};
  if (hzf) frames = hazard_frames_io(hzf, view, nullptr, nullptr);
  std::vector<int32_t> wall_counts, hz_counts;
  if (const int rc = plan_check_scenes("plan_team", spec, walls, hzf ? &view : nullptr, hzf ? &frames : nullptr, wall_counts, hz_counts)) return rc;
  if (S > 65535) return fail(MOBROB_ERR_INVALID, "plan_team: n_scenes = %d above 65535", S);
  if (spec->n_fields != N) return fail(MOBROB_ERR_INVALID, "plan_team: n_fields = %d must be n_robots = %d (every robot has its own field)", spec->n_fields, N);
  if (team_size != 1 && team_size != 2 && team_size != 4 && team_size != 8 && team_size != 16)
    return fail(MOBROB_ERR_INVALID, "plan_team: team_size must be 1, 2, 4, 8 or 16, got %d", team_size);
  if (N % team_size != 0) return fail(MOBROB_ERR_INVALID, "plan_team: %d robots do not split into teams of %d", N, team_size);
  if (reserve < 0 || reserve > kPlanReserveMax) return fail(MOBROB_ERR_INVALID, "plan_team: reserve must lie in 0 .. %d, got %d", kPlanReserveMax, reserve);
  if (walk_out && walk_cap < 1) return fail(MOBROB_ERR_INVALID, "plan_team: walk_cap must be >= 1 with walk_out");
  if (walk_out && (int64_t)N * walk_cap > INT_MAX) return fail(MOBROB_ERR_INVALID, "plan_team: n_robots * walk_cap must fit an int32");
  const int32_t* scene = hzf ? hzf->scene : walls ? walls->scene : nullptr;
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j < P; ++j)
      if (!std::isfinite(start[(size_t)i * P + j]) || !std::isfinite(goal[(size_t)i * P + j]))
        return fail(MOBROB_ERR_INVALID, "plan_team: start or goal of robot %d is not finite", i);
    if (scene && scene[i] != scene[i - i % team_size])
      return fail(MOBROB_ERR_INVALID, "plan_team: all members of a team must be in one scene (robot %d is in scene %d, its team's first member in %d)", i,
                  scene[i], scene[i - i % team_size]);
  }
  if (T < 1 || T > kPlanLayersMax) return fail(MOBROB_ERR_INVALID, "plan_team: layers must lie in 1 .. %d, got %d", kPlanLayersMax, T);
  if (tm->layer_steps < 1) return fail(MOBROB_ERR_INVALID, "plan_team: layer_steps must be >= 1, got %d", tm->layer_steps);
  if (tm->step0 < 0) return fail(MOBROB_ERR_INVALID, "plan_team: step0 must be >= 0, got %d", tm->step0);
  if ((int64_t)tm->step0 + (int64_t)(T + 1) * tm->layer_steps > INT_MAX)
    return fail(MOBROB_ERR_INVALID, "plan_team: step0 + (layers + 1) * layer_steps must fit an int32");
  const uint64_t field_bytes = (uint64_t)(T + 1) * (uint64_t)cells * 4u;
  if (field_bytes > MOBROB_PLAN_TIME_MAX_BYTES || (fields_team_out && (uint64_t)N * field_bytes > MOBROB_PLAN_TIME_MAX_BYTES))
    return fail(MOBROB_ERR_INVALID, "plan_team: time fields of %d x %d x %d x %d x 4 bytes exceed the cap of %u bytes (256 MiB)",
                fields_team_out ? N : 1, T + 1, G, G, (unsigned)MOBROB_PLAN_TIME_MAX_BYTES);
  // one workgroup's scratch: the field alone, or with smoothing the field, the next-blocked table and the reservation (7 bytes a cell and layer)
  const uint64_t wg_bytes = sm ? (uint64_t)plan_team_smooth_wg_bytes(G, T) : (uint64_t)plan_team_wg_ints(G, T) * 4u;
  if (sm && wg_bytes > MOBROB_PLAN_TIME_MAX_BYTES)
    return fail(MOBROB_ERR_INVALID, "plan_team: one team's field, next-blocked table and reservation of %d x %d x %d x 7 bytes exceed the cap of %u bytes (256 MiB)",
                T + 1, G, G, (unsigned)MOBROB_PLAN_TIME_MAX_BYTES);
  const size_t team_lds = sm ? plan_team_smooth_lds_bytes(G) : rr ? plan_team_rounds_lds_bytes(G, T, rr->retries) : plan_team_lds_bytes(G, T);
  int cus = 0;
  {   // the per-workgroup LDS limit, as mobrob_ppo_plan_grid_time checks k_plan_field_time's
    int limit = 0;
    if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, e->cfg.device_id) != hipSuccess) limit = 64 * 1024;
    if (team_lds > (size_t)limit)
      return fail(MOBROB_ERR_INVALID, "plan_team: %s needs %zu bytes of LDS at %d cells and %d layers, the device allows %d per workgroup",
                  sm ? "k_plan_team_smooth" : rr ? "k_plan_team_rounds" : "k_plan_team", team_lds, G, T, limit);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->cfg.device_id) != hipSuccess || cus < 1) cus = 1;
  }
  // the workgroups in flight: at most the teams, the compute units, and what the cap on scratch fields allows
  const int n_teams = N / team_size;
  uint64_t scratch_cap = MOBROB_PLAN_TIME_MAX_BYTES;
  if (rr) {   // the rounds' call takes a smaller cap on the scratch fields from the environment (never a larger one, at least one field's)
    const char* v = getenv("MOBROB_PLAN_TIME_MAX_BYTES");
    const unsigned long long asked = v ? strtoull(v, nullptr, 10) : 0;
    if (asked) scratch_cap = std::max<uint64_t>(std::min<uint64_t>(asked, scratch_cap), field_bytes);
  }
  const int W = (int)std::min<uint64_t>(std::min(n_teams, cus), scratch_cap / (sm ? wg_bytes : field_bytes));
  std::vector<int32_t> lfirst(T + 1, 0), lnumber(T + 1, 1);   // without frames: a static scene, its own single frame in every layer
  if (hzf) plan_layer_frames(hzf, tm, lfirst, lnumber);
  const int Mw = walls ? walls->max_walls : 0, Mh = hzf ? hzf->max_hazards : 0, NF = hzf ? hzf->n_frames : 1;
  if (!hzf) hz_counts.assign(S, 0);
  const size_t hz_floats = (size_t)S * NF * Mh * 3;
  const int heads = sm ? 7 : 6;   // the [N] arrays at the front of the outputs: smoothing adds `moves`
  if ((int64_t)N * (heads + 2 * (int64_t)K + (int64_t)K * P) > INT_MAX)
    return fail(MOBROB_ERR_INVALID, "plan_team: n_robots * (%d + 2 * max_waypoints + max_waypoints * pos_dim) must fit an int32", heads);
  const size_t n_in = (size_t)2 * N * P + N, n_out = (size_t)N * (heads + 2 * K + K * P);
  EvalCarve call;
  const size_t o_occ = call.add((size_t)S * (T + 1) * cells), o_args = call.add(sizeof(PlanTeamArgs)), o_wg = call.add((size_t)W * wg_bytes),
               o_in = call.add(n_in * 4), o_out = call.add(n_out * 4), o_field = call.add(fields_team_out ? (size_t)N * field_bytes : 0),
               o_walk = call.add(walk_out ? (size_t)N * walk_cap * 2 : 0), o_lfirst = call.add((size_t)(T + 1) * 4),
               o_lnumber = call.add((size_t)(T + 1) * 4), o_box = call.add(std::max<size_t>((size_t)S * Mw * 4, 1) * 4),
               o_nwall = call.add((size_t)S * 4), o_hz = call.add(std::max<size_t>(hz_floats, 1) * 4), o_nhz = call.add((size_t)S * 4),
               o_smargs = call.add(sm ? sizeof(PlanTeamSmoothArgs) : 0), o_keep = call.add(sm && sm->keep_out ? (size_t)N * sm->keep_cap * 4 : 0),
               o_rargs = call.add(rr ? sizeof(PlanTeamRoundsArgs) : 0), o_team = call.add(rr ? ((size_t)N + 3 * (size_t)n_teams) * 4 : 0);
  if (const int rc = grow_plan_buf(e, e->plan_team_buf, e->plan_team_bytes, call.total)) return rc;
  const auto mine = [&](size_t off) { return e->plan_team_buf + off; };
  unsigned char* occ_dev = reinterpret_cast<unsigned char*>(mine(o_occ));
  int* lfirst_dev = reinterpret_cast<int*>(mine(o_lfirst));
  int* lnumber_dev = reinterpret_cast<int*>(mine(o_lnumber));
  PlanOccTimeArgs oa{};
  oa.g = PlanGrid{G, spec->extent, spec->h, spec->inv_h, spec->inflate};
  oa.Mw = Mw; oa.Mh = Mh; oa.F = NF; oa.T = T; oa.layer_first = lfirst_dev; oa.layer_number = lnumber_dev; oa.occ = occ_dev;
  if (walls) {
    float* box_dev = reinterpret_cast<float*>(mine(o_box));
    int* cnt_dev = reinterpret_cast<int*>(mine(o_nwall));
    if ((size_t)S * Mw) HIPC(hipMemcpyAsync(box_dev, walls->boxes, (size_t)S * Mw * 16, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(cnt_dev, wall_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
    oa.boxes = box_dev; oa.nwall = cnt_dev;
  }
  float* hz_dev = reinterpret_cast<float*>(mine(o_hz));
  int* nhz_dev = reinterpret_cast<int*>(mine(o_nhz));
  if (hz_floats) HIPC(hipMemcpyAsync(hz_dev, hzf->hazards, hz_floats * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(nhz_dev, hz_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
  oa.hz = hz_dev; oa.nhz = nhz_dev;
  HIPC(hipMemcpyAsync(lfirst_dev, lfirst.data(), (size_t)(T + 1) * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(lnumber_dev, lnumber.data(), (size_t)(T + 1) * 4, hipMemcpyHostToDevice, e->stream));
  // the base layers: the time plan's own kernel, launched as it is (a static scene: one frame)
  hipLaunchKernelGGL(k_plan_occupancy_time, dim3(cells / 256, T + 1, S), dim3(256), ((size_t)4 * Mw + 3 * Mh) * sizeof(float), e->stream, oa);
  HIPC(hipGetLastError());
  if (!sm && !rr && !e->plan_team_lds_set) {   // up to 152 KB at 128 cells and 256 layers: above the 64 KB a kernel gets without asking
    HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_plan_team), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)plan_team_lds_bytes(128, kPlanLayersMax)));
    e->plan_team_lds_set = true;
  }
  // k_plan_team reads its arguments from device memory (kernels_plan.h says why), one block each for inputs, outputs and scratch
  PlanTeamArgs ta{};
  ta.g = oa.g; ta.N = N; ta.K = K; ta.P = P; ta.T = T; ta.size = team_size; ta.reserve = reserve; ta.n_teams = n_teams;
  ta.has_scene = scene ? 1 : 0;
  ta.walk_cap = walk_out ? walk_cap : 0;
  float* in_dev = reinterpret_cast<float*>(mine(o_in));
  int* out_dev = reinterpret_cast<int*>(mine(o_out));
  ta.in = in_dev; ta.occ = occ_dev; ta.wg = reinterpret_cast<int*>(mine(o_wg)); ta.out = out_dev;
  ta.fields = fields_team_out ? reinterpret_cast<int*>(mine(o_field)) : nullptr;
  ta.walk = walk_out ? reinterpret_cast<unsigned short*>(mine(o_walk)) : nullptr;
  PlanTeamArgs* args_dev = reinterpret_cast<PlanTeamArgs*>(mine(o_args));
  PlanTeamSmoothArgs* smargs_dev = reinterpret_cast<PlanTeamSmoothArgs*>(mine(o_smargs));
  PlanTeamSmoothArgs sa{};
  PlanTeamRoundsArgs* rargs_dev = reinterpret_cast<PlanTeamRoundsArgs*>(mine(o_rargs));
  PlanTeamRoundsArgs ra{};
  if (sm) {
    if (!e->plan_team_smooth_lds_set) {   // 144 KB at 128 cells: above the 64 KB a kernel gets without asking
      HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_plan_team_smooth), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)plan_team_smooth_lds_bytes(128)));
      e->plan_team_smooth_lds_set = true;
    }
    sa.t = ta; sa.margin = sm->margin; sa.max_leg = sm->max_leg; sa.keep_cap = sm->keep_out ? sm->keep_cap : 0;
    sa.keep = sm->keep_out ? reinterpret_cast<int*>(mine(o_keep)) : nullptr;
    HIPC(hipMemcpyAsync(smargs_dev, &sa, sizeof(sa), hipMemcpyHostToDevice, e->stream));
    if (sa.keep) HIPC(hipMemsetAsync(sa.keep, 0, (size_t)N * sm->keep_cap * 4, e->stream));
  } else if (rr) {
    if (!e->plan_team_rounds_lds_set) {   // k_plan_team's and 180 bytes at 8 retries
      HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_plan_team_rounds), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)plan_team_rounds_lds_bytes(128, kPlanLayersMax, kPlanRetriesMax)));
      e->plan_team_rounds_lds_set = true;
    }
    ra.t = ta; ra.retries = rr->retries; ra.team = reinterpret_cast<int*>(mine(o_team));
    HIPC(hipMemcpyAsync(rargs_dev, &ra, sizeof(ra), hipMemcpyHostToDevice, e->stream));
  } else {
    HIPC(hipMemcpyAsync(args_dev, &ta, sizeof(ta), hipMemcpyHostToDevice, e->stream));
  }
  HIPC(hipMemcpyAsync(in_dev, start, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(in_dev + (size_t)N * P, goal, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  if (scene) HIPC(hipMemcpyAsync(in_dev + (size_t)2 * N * P, scene, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemsetAsync(out_dev + (size_t)heads * N, 0, (n_out - (size_t)heads * N) * 4, e->stream));   // waits, leave, waypoints
  if (ta.walk) HIPC(hipMemsetAsync(ta.walk, 0, (size_t)N * walk_cap * 2, e->stream));
  if (sm)
    hipLaunchKernelGGL(k_plan_team_smooth, dim3(W), dim3(kPlanFieldThreads), team_lds, e->stream, static_cast<const PlanTeamSmoothArgs*>(smargs_dev));
  else if (rr)
    hipLaunchKernelGGL(k_plan_team_rounds, dim3(W), dim3(kPlanFieldThreads), team_lds, e->stream, static_cast<const PlanTeamRoundsArgs*>(rargs_dev));
  else
    hipLaunchKernelGGL(k_plan_team, dim3(W), dim3(kPlanFieldThreads), team_lds, e->stream, static_cast<const PlanTeamArgs*>(args_dev));
  HIPC(hipGetLastError());
  const auto back = [&](void* dst, size_t off_ints, size_t n_ints) {
    return hipMemcpyAsync(dst, out_dev + off_ints, n_ints * 4, hipMemcpyDeviceToHost, e->stream);
  };
  const size_t n1 = (size_t)N;
  HIPC(back(n_waypoints_out, 0, n1));
  HIPC(back(count_out, n1, n1));
  HIPC(back(status_out, 2 * n1, n1));
  HIPC(back(cost_out, 3 * n1, n1));
  HIPC(back(arrive_out, 4 * n1, n1));
  if (sweeps_out) HIPC(back(sweeps_out, 5 * n1, n1));
  const size_t h1 = (size_t)heads * n1;
  if (sm) HIPC(back(sm->moves_out, 6 * n1, n1));
  HIPC(back(waits_out, h1, n1 * K));
  HIPC(back(leave_out, h1 + n1 * K, n1 * K));
  HIPC(back(waypoints_out, h1 + 2 * n1 * K, n1 * K * P));
  if (sm && sm->keep_out) HIPC(hipMemcpyAsync(sm->keep_out, sa.keep, (size_t)N * sm->keep_cap * 4, hipMemcpyDeviceToHost, e->stream));
  if (rr) {
    const auto team_back = [&](void* dst, size_t off_ints, size_t n_ints) {
      return hipMemcpyAsync(dst, ra.team + off_ints, n_ints * 4, hipMemcpyDeviceToHost, e->stream);
    };
    const size_t g1 = (size_t)n_teams;
    HIPC(team_back(rr->order_out, 0, n1));
    HIPC(team_back(rr->rounds_out, n1, g1));
    HIPC(team_back(rr->parked_out, n1 + g1, g1));
    HIPC(team_back(rr->parked_first_out, n1 + 2 * g1, g1));
  }
  if (walk_out) HIPC(hipMemcpyAsync(walk_out, ta.walk, (size_t)N * walk_cap * 2, hipMemcpyDeviceToHost, e->stream));
  if (occ_time_out) HIPC(hipMemcpyAsync(occ_time_out, occ_dev, (size_t)S * (T + 1) * cells, hipMemcpyDeviceToHost, e->stream));
  if (fields_team_out) HIPC(hipMemcpyAsync(fields_team_out, ta.fields, (size_t)N * field_bytes, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  if (workgroups_out) *workgroups_out = W;
  return MOBROB_OK;
}

int mobrob_ppo_plan_grid_team(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls,
                              const mobrob_hazard_frames_t* hzf, const mobrob_plan_time_t* tm, int32_t team_size, int32_t reserve,
                              const float* start, const float* goal, float* waypoints_out, int32_t* n_waypoints_out, int32_t* count_out,
                              int32_t* status_out, int32_t* cost_out, int32_t* waits_out, int32_t* leave_out, int32_t* arrive_out,
                              int32_t* sweeps_out, uint16_t* walk_out, int32_t walk_cap, uint8_t* occ_time_out, int32_t* fields_team_out,
                              int32_t* workgroups_out) {
  return plan_team_run(e, spec, walls, hzf, tm, team_size, reserve, start, goal, waypoints_out, n_waypoints_out, count_out, status_out, cost_out,
                       waits_out, leave_out, arrive_out, sweeps_out, walk_out, walk_cap, occ_time_out, fields_team_out, workgroups_out, nullptr);
}

// ---- smoothing of a team plan (mobrob_ppo_plan_grid_team_smooth): capped line-of-sight legs, reserved as swept regions --------
int mobrob_ppo_plan_grid_team_smooth(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls,
                                     const mobrob_hazard_frames_t* hzf, const mobrob_plan_time_t* tm, int32_t team_size, int32_t reserve,
                                     int32_t margin, int32_t max_leg, const float* start, const float* goal, float* waypoints_out,
                                     int32_t* n_waypoints_out, int32_t* count_out, int32_t* status_out, int32_t* cost_out,
                                     int32_t* waits_out, int32_t* leave_out, int32_t* arrive_out, int32_t* moves_out, int32_t* sweeps_out,
                                     uint16_t* walk_out, int32_t walk_cap, int32_t* keep_out, int32_t keep_cap, uint8_t* occ_time_out,
                                     int32_t* fields_team_out, int32_t* workgroups_out) {
  const PlanTeamSmooth sm{margin, max_leg, moves_out, keep_out, keep_cap};
  return plan_team_run(e, spec, walls, hzf, tm, team_size, reserve, start, goal, waypoints_out, n_waypoints_out, count_out, status_out, cost_out,
                       waits_out, leave_out, arrive_out, sweeps_out, walk_out, walk_cap, occ_time_out, fields_team_out, workgroups_out, &sm);
}

// ---- priority reordering rounds of a team plan (mobrob_ppo_plan_grid_team_rounds): the parked members first, on the device ------
int mobrob_ppo_plan_grid_team_rounds(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls,
                                     const mobrob_hazard_frames_t* hzf, const mobrob_plan_time_t* tm, int32_t team_size, int32_t reserve,
                                     int32_t retries, const float* start, const float* goal, float* waypoints_out,
                                     int32_t* n_waypoints_out, int32_t* count_out, int32_t* status_out, int32_t* cost_out,
                                     int32_t* waits_out, int32_t* leave_out, int32_t* arrive_out, int32_t* sweeps_out, uint16_t* walk_out,
                                     int32_t walk_cap, uint8_t* occ_time_out, int32_t* fields_team_out, int32_t* workgroups_out,
                                     int32_t* team_order_out, int32_t* team_rounds_out, int32_t* team_parked_out,
                                     int32_t* team_parked_first_out) {
  const PlanTeamRounds rr{retries, team_order_out, team_rounds_out, team_parked_out, team_parked_first_out};
  return plan_team_run(e, spec, walls, hzf, tm, team_size, reserve, start, goal, waypoints_out, n_waypoints_out, count_out, status_out, cost_out,
                       waits_out, leave_out, arrive_out, sweeps_out, walk_out, walk_cap, occ_time_out, fields_team_out, workgroups_out, nullptr,
                       &rr);
}

// ---- goal assignment inside a team (mobrob_ppo_plan_assign): minimum-cost matching on the device ------------------------------
// The base map as the planners launch it (k_plan_occupancy for a static scene, k_plan_occupancy_time for frames, of which layer T is
// read), k_plan_assign_cost, k_plan_assign.  It works in the team plans' buffer and keeps nothing resident.
int mobrob_ppo_plan_assign(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls, const mobrob_hazards_t* hz,
                           const mobrob_hazard_frames_t* hzf, const mobrob_plan_time_t* tm, int32_t team_size, int32_t objective,
                           const float* start, const float* goal, int32_t* assign_out, float* goal_out, int32_t* assign_cost_out,
                           int64_t* total_out, int32_t* team_out, int64_t* u_out, int64_t* v_out, int32_t* matrix_out, int32_t* sweeps_out) {
  if (!e || !spec || !start || !goal || !assign_out || !goal_out || !assign_cost_out || !total_out || !team_out || !u_out || !v_out)
    return fail(MOBROB_ERR_INVALID, "plan_assign: null argument");
  if (hz && hzf) return fail(MOBROB_ERR_INVALID, "plan_assign: static hazards or hazard frames, not both");
  if ((hzf != nullptr) != (tm != nullptr)) return fail(MOBROB_ERR_INVALID, "plan_assign: time (step0, layer_steps, layers) is needed with hazard frames, and only then");
  if (objective != 0 && objective != 1) return fail(MOBROB_ERR_INVALID, "plan_assign: objective must be 0 (sum) or 1 (makespan), got %d", objective);
  if (spec->reuse_id != 0) return fail(MOBROB_ERR_INVALID, "plan_assign: reuse_id must be 0 (an assignment keeps nothing resident)");
  const int N = spec->n_robots, P = spec->pos_dim, G = spec->cells, S = spec->n_scenes;
  const int cells = G * G, T = tm ? tm->layers : 0;
  mobrob_hazards_t view;
  HazardIO frames{};
  if (hzf) frames = hazard_frames_io(hzf, view, nullptr, nullptr);
  std::vector<int32_t> wall_counts, hz_counts;
  if (const int rc = plan_check_scenes("plan_assign", spec, walls, hzf ? &view : hz, hzf ? &frames : nullptr, wall_counts, hz_counts)) return rc;
  if (S > 65535) return fail(MOBROB_ERR_INVALID, "plan_assign: n_scenes = %d above 65535", S);
  if (spec->n_fields != N) return fail(MOBROB_ERR_INVALID, "plan_assign: n_fields = %d must be n_robots = %d (every robot's goal has its own field)", spec->n_fields, N);
  if (team_size != 1 && team_size != 2 && team_size != 4 && team_size != 8 && team_size != 16)
    return fail(MOBROB_ERR_INVALID, "plan_assign: team_size must be 1, 2, 4, 8 or 16, got %d", team_size);
  if (N % team_size != 0) return fail(MOBROB_ERR_INVALID, "plan_assign: %d robots do not split into teams of %d", N, team_size);
  if ((int64_t)N * team_size > INT_MAX) return fail(MOBROB_ERR_INVALID, "plan_assign: n_robots * team_size must fit an int32");
  const int32_t* scene = hzf ? hzf->scene : walls ? walls->scene : hz ? hz->scene : nullptr;
  for (int i = 0; i < N; ++i) {
    for (int j = 0; j < P; ++j)
      if (!std::isfinite(start[(size_t)i * P + j]) || !std::isfinite(goal[(size_t)i * P + j]))
        return fail(MOBROB_ERR_INVALID, "plan_assign: start or goal of robot %d is not finite", i);
    if (scene && scene[i] != scene[i - i % team_size])
      return fail(MOBROB_ERR_INVALID, "plan_assign: all members of a team must be in one scene (robot %d is in scene %d, its team's first member in %d)", i,
                  scene[i], scene[i - i % team_size]);
  }
  std::vector<int32_t> lfirst, lnumber;
  if (hzf) {
    if (T < 1 || T > kPlanLayersMax) return fail(MOBROB_ERR_INVALID, "plan_assign: layers must lie in 1 .. %d, got %d", kPlanLayersMax, T);
    if (tm->layer_steps < 1) return fail(MOBROB_ERR_INVALID, "plan_assign: layer_steps must be >= 1, got %d", tm->layer_steps);
    if (tm->step0 < 0) return fail(MOBROB_ERR_INVALID, "plan_assign: step0 must be >= 0, got %d", tm->step0);
    if ((int64_t)tm->step0 + (int64_t)(T + 1) * tm->layer_steps > INT_MAX)
      return fail(MOBROB_ERR_INVALID, "plan_assign: step0 + (layers + 1) * layer_steps must fit an int32");
    plan_layer_frames(hzf, tm, lfirst, lnumber);
  }
  const size_t field_lds = plan_field_lds_bytes(G);
  {   // the per-workgroup LDS limit, as mobrob_ppo_plan_grid checks k_plan_field's
    int limit = 0;
    if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, e->cfg.device_id) != hipSuccess) limit = 64 * 1024;
    if (field_lds > (size_t)limit)
      return fail(MOBROB_ERR_INVALID, "plan_assign: k_plan_assign_cost needs %zu bytes of LDS at %d cells, the device allows %d per workgroup", field_lds, G, limit);
  }
  const int n_teams = N / team_size;
  const int Mw = walls ? walls->max_walls : 0, Mh = hzf ? hzf->max_hazards : hz ? hz->max_hazards : 0, NF = hzf ? hzf->n_frames : 1;
  const size_t hz_floats = (size_t)S * NF * Mh * 3;
  EvalCarve call;
  const size_t o_occ = call.add((size_t)S * (T + 1) * cells), o_start = call.add((size_t)N * P * 4), o_goal = call.add((size_t)N * P * 4),
               o_scene = call.add((size_t)N * 4), o_cost = call.add((size_t)N * team_size * 4), o_sweeps = call.add((size_t)N * 4),
               o_assign = call.add((size_t)N * 4), o_gout = call.add((size_t)N * P * 4), o_acost = call.add((size_t)N * 4),
               o_total = call.add((size_t)2 * n_teams * 8), o_team = call.add((size_t)4 * n_teams * 4), o_u = call.add((size_t)N * 8),
               o_v = call.add((size_t)N * 8), o_lfirst = call.add((size_t)(T + 1) * 4), o_lnumber = call.add((size_t)(T + 1) * 4),
               o_box = call.add(std::max<size_t>((size_t)S * Mw * 4, 1) * 4), o_nwall = call.add((size_t)S * 4),
               o_hz = call.add(std::max<size_t>(hz_floats, 1) * 4), o_nhz = call.add((size_t)S * 4);
  if (const int rc = grow_plan_buf(e, e->plan_team_buf, e->plan_team_bytes, call.total)) return rc;
  const auto mine = [&](size_t off) { return e->plan_team_buf + off; };
  unsigned char* occ_dev = reinterpret_cast<unsigned char*>(mine(o_occ));
  const PlanGrid grid{G, spec->extent, spec->h, spec->inv_h, spec->inflate};
  float* box_dev = nullptr;
  int* nwall_dev = nullptr;
  if (walls) {
    box_dev = reinterpret_cast<float*>(mine(o_box));
    nwall_dev = reinterpret_cast<int*>(mine(o_nwall));
    if ((size_t)S * Mw) HIPC(hipMemcpyAsync(box_dev, walls->boxes, (size_t)S * Mw * 16, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(nwall_dev, wall_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
  }
  float* hz_dev = reinterpret_cast<float*>(mine(o_hz));
  int* nhz_dev = reinterpret_cast<int*>(mine(o_nhz));
  if (hz || hzf) {
    if (hz_floats) HIPC(hipMemcpyAsync(hz_dev, hzf ? hzf->hazards : hz->hazards, hz_floats * 4, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(nhz_dev, hz_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
  }
  if (hzf) {
    int* lfirst_dev = reinterpret_cast<int*>(mine(o_lfirst));
    int* lnumber_dev = reinterpret_cast<int*>(mine(o_lnumber));
    HIPC(hipMemcpyAsync(lfirst_dev, lfirst.data(), (size_t)(T + 1) * 4, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(lnumber_dev, lnumber.data(), (size_t)(T + 1) * 4, hipMemcpyHostToDevice, e->stream));
    PlanOccTimeArgs oa{};
    oa.g = grid; oa.boxes = box_dev; oa.nwall = nwall_dev; oa.Mw = Mw; oa.hz = hz_dev; oa.nhz = nhz_dev; oa.Mh = Mh; oa.F = NF; oa.T = T;
    oa.layer_first = lfirst_dev; oa.layer_number = lnumber_dev; oa.occ = occ_dev;
    hipLaunchKernelGGL(k_plan_occupancy_time, dim3(cells / 256, T + 1, S), dim3(256), ((size_t)4 * Mw + 3 * Mh) * sizeof(float), e->stream, oa);
  } else {
    PlanOccArgs oa{};
    oa.g = grid; oa.boxes = box_dev; oa.nwall = nwall_dev; oa.Mw = Mw; oa.Mh = Mh; oa.occ = occ_dev;
    if (hz) { oa.hz = hz_dev; oa.nhz = nhz_dev; }
    hipLaunchKernelGGL(k_plan_occupancy, dim3(cdiv(cells, 256), S), dim3(256), ((size_t)4 * Mw + 3 * Mh) * sizeof(float), e->stream, oa);
  }
  HIPC(hipGetLastError());
  if (!e->plan_assign_lds_set) {   // 80 KB at 128 cells: above the 64 KB a kernel gets without asking
    HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_plan_assign_cost), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)plan_field_lds_bytes(128)));
    e->plan_assign_lds_set = true;
  }
  float* start_dev = reinterpret_cast<float*>(mine(o_start));
  float* goal_dev = reinterpret_cast<float*>(mine(o_goal));
  int* scene_dev = reinterpret_cast<int*>(mine(o_scene));
  HIPC(hipMemcpyAsync(start_dev, start, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(goal_dev, goal, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  if (scene) HIPC(hipMemcpyAsync(scene_dev, scene, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
  PlanAssignCostArgs ca{};
  ca.g = grid; ca.N = N; ca.P = P; ca.size = team_size; ca.start = start_dev; ca.goal = goal_dev; ca.scene = scene ? scene_dev : nullptr;
  ca.occ = occ_dev; ca.scene_stride = (size_t)(T + 1) * cells; ca.map_off = (size_t)T * cells;
  ca.cost = reinterpret_cast<int*>(mine(o_cost)); ca.sweeps = reinterpret_cast<int*>(mine(o_sweeps));
  hipLaunchKernelGGL(k_plan_assign_cost, dim3(N), dim3(kPlanFieldThreads), field_lds, e->stream, ca);
  HIPC(hipGetLastError());
  PlanAssignArgs aa{};
  aa.N = N; aa.P = P; aa.size = team_size; aa.objective = objective; aa.goal = goal_dev; aa.sweeps = ca.sweeps; aa.cost = ca.cost;
  aa.assign = reinterpret_cast<int*>(mine(o_assign)); aa.goal_out = reinterpret_cast<float*>(mine(o_gout));
  aa.assign_cost = reinterpret_cast<int*>(mine(o_acost)); aa.total = reinterpret_cast<long long*>(mine(o_total));
  aa.team = reinterpret_cast<int*>(mine(o_team)); aa.u = reinterpret_cast<long long*>(mine(o_u)); aa.v = reinterpret_cast<long long*>(mine(o_v));
  hipLaunchKernelGGL(k_plan_assign, dim3(n_teams), dim3(64), 0, e->stream, aa);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(assign_out, aa.assign, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(goal_out, aa.goal_out, (size_t)N * P * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(assign_cost_out, aa.assign_cost, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(total_out, aa.total, (size_t)2 * n_teams * 8, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(team_out, aa.team, (size_t)4 * n_teams * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(u_out, aa.u, (size_t)N * 8, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(v_out, aa.v, (size_t)N * 8, hipMemcpyDeviceToHost, e->stream));
  if (matrix_out) HIPC(hipMemcpyAsync(matrix_out, aa.cost, (size_t)N * team_size * 4, hipMemcpyDeviceToHost, e->stream));
  if (sweeps_out) HIPC(hipMemcpyAsync(sweeps_out, ca.sweeps, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}

// ---- run specifications (mobrob_ppo_spec_monitor): robustness per robot from the positions of a run -------------------------------
// everything the call refuses, before any launch or copy; counts: the scenes' region counts
// (who: the entry point's name in the messages; max_op: the last op it takes; F: the frames of a region table [S][F][R][4])
// the region table of a specification (its scenes, counts, kinds, rows and scene indices); check_clauses: n_clauses is looked at too
static int spec_check_regions(const char* who, const mobrob_spec_t* spec, int N, std::vector<int32_t>& counts, int F, bool check_clauses) {
  const int S = spec->n_scenes, R = spec->max_regions, C = spec->n_clauses;
  if (S < 1) return fail(MOBROB_ERR_INVALID, "%s: spec: n_scenes must be >= 1", who);
  if (R < 0 || R > kSpecRegionsMax) return fail(MOBROB_ERR_INVALID, "%s: spec: max_regions must lie in 0 .. %d, got %d", who, kSpecRegionsMax, R);
  if (check_clauses && (C < 1 || C > kSpecClausesMax))
    return fail(MOBROB_ERR_INVALID, "%s: spec: n_clauses must lie in 1 .. %d, got %d", who, kSpecClausesMax, C);
  if (!spec->n_regions) return fail(MOBROB_ERR_INVALID, "%s: spec: null n_regions", who);
  if (R > 0 && (!spec->regions || !spec->kinds)) return fail(MOBROB_ERR_INVALID, "%s: spec: null regions or kinds", who);
  if (!spec->scene && S > 1) return fail(MOBROB_ERR_INVALID, "%s: spec: %d scenes need a scene index per robot", who, S);
  counts.assign(spec->n_regions, spec->n_regions + S);
  for (int s = 0; s < S; ++s) {
    if (counts[s] < 0 || counts[s] > R) return fail(MOBROB_ERR_INVALID, "%s: spec: n_regions[%d] = %d outside 0 .. %d", who, s, counts[s], R);
    for (int r = 0; r < counts[s]; ++r) {
      const int kind = spec->kinds[(size_t)s * R + r];
      if (kind != 0 && kind != 1) return fail(MOBROB_ERR_INVALID, "%s: spec: kinds: region %d of scene %d has kind %d (0 box, 1 circle)", who, r, s, kind);
      for (int f = 0; f < F; ++f) {
        const float* b = spec->regions + (((size_t)s * F + f) * R + r) * 4;
        if (std::isfinite(b[0]) && std::isfinite(b[1]) && std::isfinite(b[2]) && std::isfinite(b[3]) && b[2] >= 0.f && (kind == 1 || b[3] >= 0.f))
          continue;
        if (F == 1) return fail(MOBROB_ERR_INVALID, "%s: spec: regions: region %d of scene %d is not finite or has a negative extent", who, r, s);
        return fail(MOBROB_ERR_INVALID, "%s: spec: regions: region %d of scene %d is not finite or has a negative extent in frame %d", who, r, s, f);
      }
    }
  }
  if (spec->scene)
    for (int i = 0; i < N; ++i)
      if (spec->scene[i] < 0 || spec->scene[i] >= S)
        return fail(MOBROB_ERR_INVALID, "%s: spec: scene[%d] = %d outside 0 .. %d", who, i, spec->scene[i], S - 1);
  return MOBROB_OK;
}

static int spec_check(const char* who, int max_op, const mobrob_spec_t* spec, const float* path, int N, int T, int P, int step0,
                      std::vector<int32_t>& counts, int F = 1) {
  if (N < 1) return fail(MOBROB_ERR_INVALID, "%s: n must be >= 1, got %d", who, N);
  if (T < 1) return fail(MOBROB_ERR_INVALID, "%s: T must be >= 1, got %d", who, T);
  if (P < 1 || P > 3) return fail(MOBROB_ERR_INVALID, "%s: P must lie in 1 .. 3, got %d", who, P);
  if (step0 < 0) return fail(MOBROB_ERR_INVALID, "%s: step0 must be >= 0, got %d", who, step0);
  if ((int64_t)step0 + T > INT_MAX) return fail(MOBROB_ERR_INVALID, "%s: step0 + T must fit an int32", who);
  const unsigned long long bytes = (unsigned long long)(T + 1ll) * (unsigned long long)N * P * 4ull;
  if (bytes > (unsigned long long)MOBROB_SPEC_PATH_MAX_BYTES)
    return fail(MOBROB_ERR_INVALID, "%s: path of %llu bytes is above the limit of %u", who, bytes, (unsigned)MOBROB_SPEC_PATH_MAX_BYTES);
  if (const int rc = spec_check_regions(who, spec, N, counts, F, true)) return rc;
  const int R = spec->max_regions, C = spec->n_clauses;
  for (int c = 0; c < C; ++c) {
    if (spec->op[c] < MOBROB_SPEC_ALWAYS || spec->op[c] > max_op)
      return fail(MOBROB_ERR_INVALID, "%s: spec: op[%d] = %d outside 0 .. %d", who, c, spec->op[c], max_op);
    if (spec->a[c] < 0 || spec->a[c] > spec->b[c])
      return fail(MOBROB_ERR_INVALID, "%s: spec: window of clause %d: a = %d, b = %d do not obey 0 <= a <= b", who, c, spec->a[c], spec->b[c]);
    if (spec->lo1[c] < 0 || spec->lo1[c] > spec->hi1[c] || spec->hi1[c] > R)
      return fail(MOBROB_ERR_INVALID, "%s: spec: region range [%d, %d) of clause %d outside 0 .. %d", who, spec->lo1[c], spec->hi1[c], c, R);
    if (spec->op[c] == MOBROB_SPEC_UNTIL && (spec->lo2[c] < 0 || spec->lo2[c] > spec->hi2[c] || spec->hi2[c] > R))
      return fail(MOBROB_ERR_INVALID, "%s: spec: second region range [%d, %d) of clause %d outside 0 .. %d", who, spec->lo2[c], spec->hi2[c], c, R);
  }
  // positions: one pass over the exponent bits, a second one only to name the offender
  const size_t total = (size_t)(T + 1) * N * P;
  uint32_t bad = 0;
  for (size_t k = 0; k < total; ++k) {
    uint32_t w;
    memcpy(&w, path + k, 4);
    bad |= (uint32_t)((w & 0x7F800000u) == 0x7F800000u);
  }
  if (bad)
    for (size_t k = 0; k < total; ++k)
      if (!std::isfinite(path[k]))
        return fail(MOBROB_ERR_INVALID, "%s: path: the position of robot %d in record %d is not finite", who, (int)((k / P) % N), (int)(k / P / N));
  return MOBROB_OK;
}

int mobrob_ppo_spec_monitor(mobrob_ppo_engine_t* e, const mobrob_spec_t* spec, const float* path, int32_t n, int32_t T, int32_t P,
                            int32_t step0, float* val, int32_t* wit) {
  if (!e) return fail(MOBROB_ERR_INVALID, "spec_monitor: null engine");
  if (!spec) return fail(MOBROB_ERR_INVALID, "spec_monitor: null spec");
  if (!path) return fail(MOBROB_ERR_INVALID, "spec_monitor: null path");
  if (!val) return fail(MOBROB_ERR_INVALID, "spec_monitor: null val");
  if (!wit) return fail(MOBROB_ERR_INVALID, "spec_monitor: null wit");
  std::vector<int32_t> counts;
  if (const int rc = spec_check("spec_monitor", MOBROB_SPEC_UNTIL, spec, path, n, T, P, step0, counts)) return rc;
  const int S = spec->n_scenes, R = spec->max_regions, C = spec->n_clauses;
  std::vector<int32_t> clauses((size_t)C * kSpecClauseWords);
  for (int c = 0; c < C; ++c) {
    const bool until = spec->op[c] == MOBROB_SPEC_UNTIL;
    const int32_t row[kSpecClauseWords] = {spec->op[c], spec->a[c], spec->b[c], spec->lo1[c], spec->hi1[c], spec->out1[c] != 0,
                                           until ? spec->lo2[c] : 0, until ? spec->hi2[c] : 0, until ? spec->out2[c] != 0 : 0};
    std::copy(row, row + kSpecClauseWords, clauses.begin() + (size_t)c * kSpecClauseWords);
  }
  const size_t path_bytes = (size_t)(T + 1) * n * P * 4, val_bytes = (size_t)n * C * 8, wit_bytes = (size_t)n * C * 4;
  EvalCarve call;
  const size_t o_path = call.add(path_bytes), o_val = call.add(val_bytes), o_wit = call.add(wit_bytes),
               o_reg = call.add(std::max<size_t>((size_t)S * R * 16, 4)), o_kind = call.add(std::max<size_t>((size_t)S * R * 4, 4)),
               o_cnt = call.add((size_t)S * 4), o_scene = call.add((size_t)n * 4), o_cl = call.add(clauses.size() * 4);
  if (const int rc = grow_plan_buf(e, e->spec_buf, e->spec_bytes, call.total)) return rc;
  const auto mine = [&](size_t off) { return e->spec_buf + off; };
  SpecArgs a{};
  a.path = reinterpret_cast<float*>(mine(o_path));
  a.regions = reinterpret_cast<float*>(mine(o_reg)); a.kinds = reinterpret_cast<int*>(mine(o_kind));
  a.nreg = reinterpret_cast<int*>(mine(o_cnt)); a.scene = spec->scene ? reinterpret_cast<int*>(mine(o_scene)) : nullptr;
  a.clauses = reinterpret_cast<int*>(mine(o_cl));
  a.val = reinterpret_cast<float*>(mine(o_val)); a.wit = reinterpret_cast<int*>(mine(o_wit));
  a.N = n; a.T = T; a.P = P; a.R = R; a.C = C;
  a.r0 = step0 == 0 ? 0 : 1;
  a.tau0 = step0;
  HIPC(hipMemcpyAsync(mine(o_path), path, path_bytes, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(mine(o_val), val, val_bytes, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(mine(o_wit), wit, wit_bytes, hipMemcpyHostToDevice, e->stream));
  if ((size_t)S * R) {
    HIPC(hipMemcpyAsync(mine(o_reg), spec->regions, (size_t)S * R * 16, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(mine(o_kind), spec->kinds, (size_t)S * R * 4, hipMemcpyHostToDevice, e->stream));
  }
  HIPC(hipMemcpyAsync(mine(o_cnt), counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
  if (spec->scene) HIPC(hipMemcpyAsync(mine(o_scene), spec->scene, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(mine(o_cl), clauses.data(), clauses.size() * 4, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_spec_monitor, dim3(cdiv(n, 64)), dim3(64), 0, e->stream, a);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(val, a.val, val_bytes, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(wit, a.wit, wit_bytes, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}

// ---- nested run specifications (mobrob_ppo_spec_monitor_nested): the flat call with stay / recur clauses and their carried tail -----
int mobrob_ppo_spec_monitor_nested(mobrob_ppo_engine_t* e, const mobrob_spec_nested_t* spec, const float* path, int32_t n, int32_t T,
                                   int32_t P, int32_t step0, float* val, int32_t* wit, float* tail, int32_t W) {
  const char* who = "spec_monitor_nested";
  if (!e) return fail(MOBROB_ERR_INVALID, "%s: null engine", who);
  if (!spec) return fail(MOBROB_ERR_INVALID, "%s: null spec", who);
  if (!path) return fail(MOBROB_ERR_INVALID, "%s: null path", who);
  if (!val) return fail(MOBROB_ERR_INVALID, "%s: null val", who);
  if (!wit) return fail(MOBROB_ERR_INVALID, "%s: null wit", who);
  // the flat call's checks on the flat call's fields (mobrob_spec_t is the head of mobrob_spec_nested_t, field by field)
  mobrob_spec_t head;
  head.n_scenes = spec->n_scenes; head.max_regions = spec->max_regions;
  head.regions = spec->regions; head.kinds = spec->kinds; head.n_regions = spec->n_regions; head.scene = spec->scene;
  head.n_clauses = spec->n_clauses;
  memcpy(head.op, spec->op, sizeof head.op); memcpy(head.a, spec->a, sizeof head.a); memcpy(head.b, spec->b, sizeof head.b);
  memcpy(head.lo1, spec->lo1, sizeof head.lo1); memcpy(head.hi1, spec->hi1, sizeof head.hi1); memcpy(head.out1, spec->out1, sizeof head.out1);
  memcpy(head.lo2, spec->lo2, sizeof head.lo2); memcpy(head.hi2, spec->hi2, sizeof head.hi2); memcpy(head.out2, spec->out2, sizeof head.out2);
  std::vector<int32_t> counts;
  if (const int rc = spec_check(who, MOBROB_SPEC_RECUR, &head, path, n, T, P, step0, counts)) return rc;
  const int S = spec->n_scenes, R = spec->max_regions, C = spec->n_clauses;
  int slots = 0;
  long long width = 0;
  std::vector<int32_t> clauses((size_t)C * kSpecNestedClauseWords);
  for (int c = 0; c < C; ++c) {
    const int op = spec->op[c], h = spec->hold[c];
    const bool until = op == MOBROB_SPEC_UNTIL, nested = op >= MOBROB_SPEC_STAY;
    if (h < 0 || h > MOBROB_SPEC_HOLD_MAX)
      return fail(MOBROB_ERR_INVALID, "%s: spec: hold[%d] = %d outside 0 .. %d", who, c, h, MOBROB_SPEC_HOLD_MAX);
    if (!nested && h != 0) return fail(MOBROB_ERR_INVALID, "%s: spec: hold[%d] = %d on the flat op %d (must be 0)", who, c, h, op);
    const int32_t row[kSpecNestedClauseWords] = {op, spec->a[c], spec->b[c], spec->lo1[c], spec->hi1[c], spec->out1[c] != 0,
                                                 until ? spec->lo2[c] : 0, until ? spec->hi2[c] : 0, until ? spec->out2[c] != 0 : 0,
                                                 h, slots, (int32_t)width};
    std::copy(row, row + kSpecNestedClauseWords, clauses.begin() + (size_t)c * kSpecNestedClauseWords);
    if (nested) { slots += h + 1; width += h; }
  }
  if (slots > MOBROB_SPEC_WINDOW_SLOTS)
    return fail(MOBROB_ERR_INVALID, "%s: spec: the nested clauses' windows take %d slots (the sum of hold + 1), above %d", who, slots,
                MOBROB_SPEC_WINDOW_SLOTS);
  if (W != width) return fail(MOBROB_ERR_INVALID, "%s: W = %d is not the sum of the holds, %lld", who, W, width);
  if (W > 0 && !tail) return fail(MOBROB_ERR_INVALID, "%s: null tail with W = %d", who, W);
  const size_t path_bytes = (size_t)(T + 1) * n * P * 4, val_bytes = (size_t)n * C * 8, wit_bytes = (size_t)n * C * 4,
               tail_bytes = (size_t)n * W * 4;
  EvalCarve call;
  const size_t o_path = call.add(path_bytes), o_val = call.add(val_bytes), o_wit = call.add(wit_bytes),
               o_reg = call.add(std::max<size_t>((size_t)S * R * 16, 4)), o_kind = call.add(std::max<size_t>((size_t)S * R * 4, 4)),
               o_cnt = call.add((size_t)S * 4), o_scene = call.add((size_t)n * 4), o_cl = call.add(clauses.size() * 4),
               o_tail = call.add(std::max<size_t>(tail_bytes, 4));
  if (const int rc = grow_plan_buf(e, e->spec_buf, e->spec_bytes, call.total)) return rc;
  if (!e->spec_nested_lds_set) {   // up to 158 KB at the slot cap: above the 64 KB a kernel gets without asking
    HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_spec_monitor_nested), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)spec_nested_lds_bytes(kSpecWindowSlots)));
    e->spec_nested_lds_set = true;
  }
  const auto mine = [&](size_t off) { return e->spec_buf + off; };
  SpecNestedArgs na{};
  SpecArgs& a = na.f;
  a.path = reinterpret_cast<float*>(mine(o_path));
  a.regions = reinterpret_cast<float*>(mine(o_reg)); a.kinds = reinterpret_cast<int*>(mine(o_kind));
  a.nreg = reinterpret_cast<int*>(mine(o_cnt)); a.scene = spec->scene ? reinterpret_cast<int*>(mine(o_scene)) : nullptr;
  a.clauses = reinterpret_cast<int*>(mine(o_cl));
  a.val = reinterpret_cast<float*>(mine(o_val)); a.wit = reinterpret_cast<int*>(mine(o_wit));
  a.N = n; a.T = T; a.P = P; a.R = R; a.C = C;
  a.r0 = step0 == 0 ? 0 : 1;
  a.tau0 = step0;
  na.tail = reinterpret_cast<float*>(mine(o_tail)); na.W = W;
  HIPC(hipMemcpyAsync(mine(o_path), path, path_bytes, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(mine(o_val), val, val_bytes, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(mine(o_wit), wit, wit_bytes, hipMemcpyHostToDevice, e->stream));
  if (tail_bytes) HIPC(hipMemcpyAsync(mine(o_tail), tail, tail_bytes, hipMemcpyHostToDevice, e->stream));
  if ((size_t)S * R) {
    HIPC(hipMemcpyAsync(mine(o_reg), spec->regions, (size_t)S * R * 16, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(mine(o_kind), spec->kinds, (size_t)S * R * 4, hipMemcpyHostToDevice, e->stream));
  }
  HIPC(hipMemcpyAsync(mine(o_cnt), counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
  if (spec->scene) HIPC(hipMemcpyAsync(mine(o_scene), spec->scene, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(mine(o_cl), clauses.data(), clauses.size() * 4, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_spec_monitor_nested, dim3(cdiv(n, 64)), dim3(64), spec_nested_lds_bytes(slots), e->stream, na);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(val, a.val, val_bytes, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(wit, a.wit, wit_bytes, hipMemcpyDeviceToHost, e->stream));
  if (tail_bytes) HIPC(hipMemcpyAsync(tail, na.tail, tail_bytes, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}

// ---- run specifications over things that move (mobrob_ppo_spec_monitor_moving): the nested call with region frames and mate predicates
int mobrob_ppo_spec_monitor_moving(mobrob_ppo_engine_t* e, const mobrob_spec_moving_t* spec, const float* path, int32_t n, int32_t T,
                                   int32_t P, int32_t step0, float* val, int32_t* wit, float* tail, int32_t W) {
  const char* who = "spec_monitor_moving";
  if (!e) return fail(MOBROB_ERR_INVALID, "%s: null engine", who);
  if (!spec) return fail(MOBROB_ERR_INVALID, "%s: null spec", who);
  if (!path) return fail(MOBROB_ERR_INVALID, "%s: null path", who);
  if (!val) return fail(MOBROB_ERR_INVALID, "%s: null val", who);
  if (!wit) return fail(MOBROB_ERR_INVALID, "%s: null wit", who);
  // what is new in this call and sizes the table, before the table is read
  const int F = spec->n_frames, size = spec->team_size;
  if (size != 1 && size != 2 && size != 4 && size != 8 && size != 16)
    return fail(MOBROB_ERR_INVALID, "%s: spec: team_size must be 1, 2, 4, 8 or 16, got %d", who, size);
  if (F < 1) return fail(MOBROB_ERR_INVALID, "%s: spec: n_frames must be >= 1, got %d", who, F);
  if (spec->frame_steps < 1) return fail(MOBROB_ERR_INVALID, "%s: spec: frame_steps must be >= 1, got %d", who, spec->frame_steps);
  if (spec->loop != 0 && spec->loop != 1) return fail(MOBROB_ERR_INVALID, "%s: spec: loop must be 0 or 1, got %d", who, spec->loop);
  if (spec->n_scenes >= 1 && spec->max_regions >= 0 && spec->max_regions <= kSpecRegionsMax) {
    const unsigned long long table = (unsigned long long)spec->n_scenes * (unsigned long long)F * (unsigned long long)spec->max_regions * 16ull;
    if (table > (unsigned long long)MOBROB_SPEC_FRAMES_MAX_BYTES)
      return fail(MOBROB_ERR_INVALID, "%s: spec: region frames of %llu bytes are above the limit of %u", who, table,
                  (unsigned)MOBROB_SPEC_FRAMES_MAX_BYTES);
  }
  // the flat call's checks on the flat call's fields (mobrob_spec_t is the head of mobrob_spec_moving_t, field by field), per frame
  mobrob_spec_t head;
  head.n_scenes = spec->n_scenes; head.max_regions = spec->max_regions;
  head.regions = spec->regions; head.kinds = spec->kinds; head.n_regions = spec->n_regions; head.scene = spec->scene;
  head.n_clauses = spec->n_clauses;
  memcpy(head.op, spec->op, sizeof head.op); memcpy(head.a, spec->a, sizeof head.a); memcpy(head.b, spec->b, sizeof head.b);
  memcpy(head.lo1, spec->lo1, sizeof head.lo1); memcpy(head.hi1, spec->hi1, sizeof head.hi1); memcpy(head.out1, spec->out1, sizeof head.out1);
  memcpy(head.lo2, spec->lo2, sizeof head.lo2); memcpy(head.hi2, spec->hi2, sizeof head.hi2); memcpy(head.out2, spec->out2, sizeof head.out2);
  std::vector<int32_t> counts;
  if (const int rc = spec_check(who, MOBROB_SPEC_RECUR, &head, path, n, T, P, step0, counts, F)) return rc;
  if (n % size != 0) return fail(MOBROB_ERR_INVALID, "%s: %d robots do not split into teams of %d", who, n, size);
  const int S = spec->n_scenes, R = spec->max_regions, C = spec->n_clauses;
  int slots = 0;
  long long width = 0;
  std::vector<int32_t> clauses((size_t)C * kSpecMovingClauseWords);
  for (int c = 0; c < C; ++c) {
    const int op = spec->op[c], h = spec->hold[c];
    const bool until = op == MOBROB_SPEC_UNTIL, nested = op >= MOBROB_SPEC_STAY;
    if (h < 0 || h > MOBROB_SPEC_HOLD_MAX)
      return fail(MOBROB_ERR_INVALID, "%s: spec: hold[%d] = %d outside 0 .. %d", who, c, h, MOBROB_SPEC_HOLD_MAX);
    if (!nested && h != 0) return fail(MOBROB_ERR_INVALID, "%s: spec: hold[%d] = %d on the flat op %d (must be 0)", who, c, h, op);
    if (spec->kind1[c] < MOBROB_SPEC_PRED_REGIONS || spec->kind1[c] > MOBROB_SPEC_PRED_APART)
      return fail(MOBROB_ERR_INVALID, "%s: spec: kind1[%d] = %d outside 0 .. 2", who, c, spec->kind1[c]);
    if (until && (spec->kind2[c] < MOBROB_SPEC_PRED_REGIONS || spec->kind2[c] > MOBROB_SPEC_PRED_APART))
      return fail(MOBROB_ERR_INVALID, "%s: spec: kind2[%d] = %d outside 0 .. 2", who, c, spec->kind2[c]);
    if (!(std::isfinite(spec->rad1[c]) && spec->rad1[c] >= 0.f))
      return fail(MOBROB_ERR_INVALID, "%s: spec: rad1[%d] is negative or not finite", who, c);
    if (until && !(std::isfinite(spec->rad2[c]) && spec->rad2[c] >= 0.f))
      return fail(MOBROB_ERR_INVALID, "%s: spec: rad2[%d] is negative or not finite", who, c);
    int32_t d1, d2 = 0;
    memcpy(&d1, &spec->rad1[c], 4);
    if (until) memcpy(&d2, &spec->rad2[c], 4);
    const int32_t row[kSpecMovingClauseWords] = {op, spec->a[c], spec->b[c], spec->lo1[c], spec->hi1[c], spec->out1[c] != 0,
                                                 until ? spec->lo2[c] : 0, until ? spec->hi2[c] : 0, until ? spec->out2[c] != 0 : 0,
                                                 h, slots, (int32_t)width, spec->kind1[c], until ? spec->kind2[c] : 0, d1, d2};
    std::copy(row, row + kSpecMovingClauseWords, clauses.begin() + (size_t)c * kSpecMovingClauseWords);
    if (nested) { slots += h + 1; width += h; }
  }
  if (slots > MOBROB_SPEC_WINDOW_SLOTS)
    return fail(MOBROB_ERR_INVALID, "%s: spec: the nested clauses' windows take %d slots (the sum of hold + 1), above %d", who, slots,
                MOBROB_SPEC_WINDOW_SLOTS);
  if (W != width) return fail(MOBROB_ERR_INVALID, "%s: W = %d is not the sum of the holds, %lld", who, W, width);
  if (W > 0 && !tail) return fail(MOBROB_ERR_INVALID, "%s: null tail with W = %d", who, W);
  const size_t path_bytes = (size_t)(T + 1) * n * P * 4, val_bytes = (size_t)n * C * 8, wit_bytes = (size_t)n * C * 4,
               tail_bytes = (size_t)n * W * 4, reg_bytes = (size_t)S * F * R * 16;
  EvalCarve call;
  const size_t o_path = call.add(path_bytes), o_val = call.add(val_bytes), o_wit = call.add(wit_bytes),
               o_reg = call.add(std::max<size_t>(reg_bytes, 4)), o_kind = call.add(std::max<size_t>((size_t)S * R * 4, 4)),
               o_cnt = call.add((size_t)S * 4), o_scene = call.add((size_t)n * 4), o_cl = call.add(clauses.size() * 4),
               o_tail = call.add(std::max<size_t>(tail_bytes, 4));
  if (const int rc = grow_plan_buf(e, e->spec_buf, e->spec_bytes, call.total)) return rc;
  if (!e->spec_moving_lds_set) {   // up to 158.3 KB at the slot cap: above the 64 KB a kernel gets without asking
    HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_spec_monitor_moving), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)spec_moving_lds_bytes(kSpecWindowSlots)));
    e->spec_moving_lds_set = true;
  }
  const auto mine = [&](size_t off) { return e->spec_buf + off; };
  SpecMovingArgs ma{};
  SpecNestedArgs& na = ma.n;
  SpecArgs& a = na.f;
  a.path = reinterpret_cast<float*>(mine(o_path));
  a.regions = reinterpret_cast<float*>(mine(o_reg)); a.kinds = reinterpret_cast<int*>(mine(o_kind));
  a.nreg = reinterpret_cast<int*>(mine(o_cnt)); a.scene = spec->scene ? reinterpret_cast<int*>(mine(o_scene)) : nullptr;
  a.clauses = reinterpret_cast<int*>(mine(o_cl));
  a.val = reinterpret_cast<float*>(mine(o_val)); a.wit = reinterpret_cast<int*>(mine(o_wit));
  a.N = n; a.T = T; a.P = P; a.R = R; a.C = C;
  a.r0 = step0 == 0 ? 0 : 1;
  a.tau0 = step0;
  na.tail = reinterpret_cast<float*>(mine(o_tail)); na.W = W;
  ma.F = F; ma.frame_steps = spec->frame_steps; ma.loop = spec->loop; ma.size = size;
  HIPC(hipMemcpyAsync(mine(o_path), path, path_bytes, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(mine(o_val), val, val_bytes, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(mine(o_wit), wit, wit_bytes, hipMemcpyHostToDevice, e->stream));
  if (tail_bytes) HIPC(hipMemcpyAsync(mine(o_tail), tail, tail_bytes, hipMemcpyHostToDevice, e->stream));
  if (reg_bytes) {
    HIPC(hipMemcpyAsync(mine(o_reg), spec->regions, reg_bytes, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(mine(o_kind), spec->kinds, (size_t)S * R * 4, hipMemcpyHostToDevice, e->stream));
  }
  HIPC(hipMemcpyAsync(mine(o_cnt), counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
  if (spec->scene) HIPC(hipMemcpyAsync(mine(o_scene), spec->scene, (size_t)n * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(mine(o_cl), clauses.data(), clauses.size() * 4, hipMemcpyHostToDevice, e->stream));
  hipLaunchKernelGGL(k_spec_monitor_moving, dim3(cdiv(n, 64)), dim3(64), spec_moving_lds_bytes(slots), e->stream, ma);
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(val, a.val, val_bytes, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(wit, a.wit, wit_bytes, hipMemcpyDeviceToHost, e->stream));
  if (tail_bytes) HIPC(hipMemcpyAsync(tail, na.tail, tail_bytes, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}

// ---- a plan from a specification (mobrob_ppo_spec_plan): the order of the stations and the stitched waypoints on the device -------
// k_plan_occupancy as it is (or a zeroed map), k_plan_region_occupancy, k_plan_station (which writes the anchors into the field list),
// ONE k_plan_field launch for the S * M station fields and the goal fields, k_plan_tour_matrix, k_plan_tour, k_plan_tour_path.  It
// works in a buffer of its own and keeps nothing resident: mobrob_ppo_plan_grid's resident fields stay valid across it.
// mobrob_ppo_spec_replan is the same call from the middle of a run (csrc/kernels_plan_spec_resume.h): the same checks, buffer, map,
// stations, fields and matrix, then k_plan_tour_resume and k_plan_tour_path_legs in place of the last two.
// mobrob_ppo_spec_plan_share is the replan with the team's stations shared among its members (csrc/kernels_plan_spec_share.h): after the
// matrix k_plan_tour_best and k_plan_team_share, then k_plan_tour_resume over the shares, k_plan_team_void and k_plan_tour_path_legs.
struct SpecShare {
  int32_t team_size, objective;
  int32_t* share_out;           // [n]
  int32_t* team_cover_out;      // [n / team_size]
  int32_t* team_dropped_out;    // [n / team_size]
  int32_t* team_makespan_out;   // [n / team_size]
  int64_t* team_total_out;      // [n / team_size]
};

struct SpecReplan {
  const int32_t* todo;     // [n]
  int32_t t0, partial;
  int32_t* tour_len_out;   // [n]
  int32_t* dropped_out;    // [n]
  const SpecShare* share;  // null: every robot for itself
};

static int spec_plan_run(const char* who, const SpecReplan* rp, mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls, const mobrob_hazards_t* hz,
                         const mobrob_spec_t* regions, int32_t n_stations, const int32_t* station_lo, const int32_t* station_hi,
                         int32_t n_avoid, const int32_t* avoid_lo, const int32_t* avoid_hi, const int32_t* open_c, const int32_t* close_c,
                         const int32_t* dwell_c, int32_t pace, const float* start, const float* goal, const int32_t* field_of,
                         const int32_t* field_goal_cell, const int32_t* field_scene, float* waypoints_out, int32_t* n_waypoints_out,
                         int32_t* count_out, int32_t* status_out, int32_t* cost_out, int32_t* tour_order_out, int32_t* tour_eta_out,
                         int32_t* station_waypoint_out, int32_t* release_out, int32_t* station_cell_out, float* station_margin_out,
                         int32_t* matrix_out, uint8_t* occupancy_out, int32_t* sweeps_out) {
  if (!e || !spec || !regions || !station_lo || !station_hi || !open_c || !close_c || !dwell_c || !start || !waypoints_out ||
      !n_waypoints_out || !count_out || !status_out || !cost_out || !tour_order_out || !tour_eta_out || !station_waypoint_out ||
      !release_out || !station_cell_out || !station_margin_out || !matrix_out)
    return fail(MOBROB_ERR_INVALID, "%s: null argument", who);
  if (goal && (!field_of || !field_goal_cell || !field_scene)) return fail(MOBROB_ERR_INVALID, "%s: null argument (a goal needs its field lists)", who);
  if (spec->reuse_id != 0) return fail(MOBROB_ERR_INVALID, "%s: reuse_id must be 0 (a plan from a specification keeps nothing resident)", who);
  const int N = spec->n_robots, P = spec->pos_dim, G = spec->cells, K = spec->max_waypoints, S = spec->n_scenes, M = n_stations;
  const int Fg = goal ? spec->n_fields : 0;
  if (!goal && spec->n_fields != 0) return fail(MOBROB_ERR_INVALID, "%s: n_fields = %d must be 0 without a goal", who, spec->n_fields);
  if (M < 1 || M > kPlanTourMax) return fail(MOBROB_ERR_INVALID, "%s: n_stations must lie in 1 .. %d, got %d", who, kPlanTourMax, M);
  if (n_avoid < 0 || n_avoid > kSpecClausesMax) return fail(MOBROB_ERR_INVALID, "%s: n_avoid must lie in 0 .. %d, got %d", who, kSpecClausesMax, n_avoid);
  if (n_avoid > 0 && (!avoid_lo || !avoid_hi)) return fail(MOBROB_ERR_INVALID, "%s: null avoid ranges", who);
  if (pace < 1 || pace > (1 << 20)) return fail(MOBROB_ERR_INVALID, "%s: pace must lie in 1 .. 2^20, got %d", who, pace);
  std::vector<int32_t> wall_counts, hz_counts, region_counts;
  {   // the spec and the scenes, by mobrob_ppo_plan_grid's checks (which count the scenes of walls and hazards, and at least one field)
    mobrob_plan_spec_t chk = *spec;
    if (!walls && !hz) chk.n_scenes = 1;
    if (!goal) chk.n_fields = 1;
    if (const int rc = plan_check_scenes(who, &chk, walls, hz, nullptr, wall_counts, hz_counts)) return rc;
  }
  if (const int rc = spec_check_regions(who, regions, N, region_counts, 1, false)) return rc;
  if (S != regions->n_scenes) return fail(MOBROB_ERR_INVALID, "%s: n_scenes = %d is not the regions' %d", who, S, regions->n_scenes);
  if (S > 65535) return fail(MOBROB_ERR_INVALID, "%s: n_scenes = %d above 65535", who, S);
  if (walls || hz) {   // walls and hazards agree with each other (plan_check_scenes); the regions must agree with them
    const int32_t* other = walls ? walls->scene : hz->scene;
    if ((other != nullptr) != (regions->scene != nullptr))
      return fail(MOBROB_ERR_INVALID, "%s: the regions and the walls / hazards must agree on the scene index per robot", who);
    for (int i = 0; other && i < N; ++i)
      if (other[i] != regions->scene[i])
        return fail(MOBROB_ERR_INVALID, "%s: the regions and the walls / hazards disagree on the scene of robot %d (%d and %d)", who, i,
                    regions->scene[i], other[i]);
  }
  const int R = regions->max_regions;
  for (int j = 0; j < M; ++j) {
    if (station_lo[j] < 0 || station_lo[j] > station_hi[j] || station_hi[j] > R)
      return fail(MOBROB_ERR_INVALID, "%s: region range [%d, %d) of station %d outside 0 .. %d", who, station_lo[j], station_hi[j], j, R);
    for (const int32_t* ticks : {open_c, close_c, dwell_c})
      if (ticks[j] < 0 || ticks[j] > kPlanTourTicksMax)
        return fail(MOBROB_ERR_INVALID, "%s: open, close and dwell ticks of station %d must lie in 0 .. %d", who, j, kPlanTourTicksMax);
    if (open_c[j] > close_c[j])
      return fail(MOBROB_ERR_INVALID, "%s: station %d opens at tick %d, after it closes at tick %d", who, j, open_c[j], close_c[j]);
  }
  for (int v = 0; v < n_avoid; ++v)
    if (avoid_lo[v] < 0 || avoid_lo[v] > avoid_hi[v] || avoid_hi[v] > R)
      return fail(MOBROB_ERR_INVALID, "%s: region range [%d, %d) of avoid clause %d outside 0 .. %d", who, avoid_lo[v], avoid_hi[v], v, R);
  const int32_t* scene = regions->scene;
  if (goal) {
    if (const int rc = plan_check_robots(who, spec, scene, start, goal, field_of, field_goal_cell, field_scene, true)) return rc;
  } else {
    for (size_t k = 0; k < (size_t)N * P; ++k)
      if (!std::isfinite(start[k])) return fail(MOBROB_ERR_INVALID, "%s: start of robot %d is not finite", who, (int)(k / P));
  }
  if ((int64_t)N * K > INT_MAX || (int64_t)S * M * M > INT_MAX) return fail(MOBROB_ERR_INVALID, "%s: n_robots * max_waypoints must fit an int32", who);
  if (rp) {
    if (!rp->todo || !rp->tour_len_out || !rp->dropped_out) return fail(MOBROB_ERR_INVALID, "%s: null argument", who);
    if (rp->t0 < 0 || rp->t0 > kPlanTourTicksMax)
      return fail(MOBROB_ERR_INVALID, "%s: step0_ticks must lie in 0 .. %d, got %d", who, kPlanTourTicksMax, rp->t0);
    if (rp->partial != 0 && rp->partial != 1) return fail(MOBROB_ERR_INVALID, "%s: partial must be 0 or 1, got %d", who, rp->partial);
    for (int i = 0; i < N; ++i)
      if (rp->todo[i] < 0 || rp->todo[i] >= (1 << M))
        return fail(MOBROB_ERR_INVALID, "%s: todo of robot %d is 0x%x, a bit at or above n_stations = %d", who, i, (unsigned)rp->todo[i], M);
  }
  const SpecShare* sh = rp ? rp->share : nullptr;
  if (sh) {
    const int size = sh->team_size;
    if (size != 1 && size != 2 && size != 4 && size != 8 && size != 16)
      return fail(MOBROB_ERR_INVALID, "%s: team_size must be 1, 2, 4, 8 or 16, got %d", who, size);
    if (N % size != 0) return fail(MOBROB_ERR_INVALID, "%s: %d robots do not split into teams of %d", who, N, size);
    if (sh->objective != 0 && sh->objective != 1)
      return fail(MOBROB_ERR_INVALID, "%s: objective must be 0 (makespan) or 1 (sum), got %d", who, sh->objective);
    if (!sh->share_out || !sh->team_cover_out || !sh->team_dropped_out || !sh->team_makespan_out || !sh->team_total_out)
      return fail(MOBROB_ERR_INVALID, "%s: null argument", who);
  }
  const int tsize = sh ? sh->team_size : 1, NT = N / tsize;
  const int cells = G * G, F = S * M + Fg;
  if ((uint64_t)((uint64_t)S * M + Fg) * (uint64_t)cells * 4u > MOBROB_PLAN_TIME_MAX_BYTES)
    return fail(MOBROB_ERR_INVALID, "%s: fields of (%d x %d + %d) x %d x %d x 4 bytes exceed the cap of %u bytes (256 MiB)", who, S, M, Fg, G, G,
                (unsigned)MOBROB_PLAN_TIME_MAX_BYTES);
  const size_t field_lds = plan_field_lds_bytes(G);
  {   // the per-workgroup LDS limit, as mobrob_ppo_plan_grid checks k_plan_field's
    int limit = 0;
    if (hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, e->cfg.device_id) != hipSuccess) limit = 64 * 1024;
    if (field_lds > (size_t)limit)
      return fail(MOBROB_ERR_INVALID, "%s: k_plan_field needs %zu bytes of LDS at %d cells, the device allows %d per workgroup", who, field_lds, G, limit);
  }
  const int Mw = walls ? walls->max_walls : 0, Mh = hz ? hz->max_hazards : 0;
  EvalCarve call;
  const size_t o_occ = call.add((size_t)S * cells), o_field = call.add((size_t)F * cells * 4), o_fgoal = call.add((size_t)F * 4),
               o_fscene = call.add((size_t)F * 4), o_sweeps = call.add((size_t)F * 4), o_start = call.add((size_t)N * P * 4),
               o_goal = call.add((size_t)N * P * 4), o_fof = call.add((size_t)N * 4), o_scene = call.add((size_t)N * 4),
               o_wp = call.add((size_t)N * K * P * 4), o_nwp = call.add((size_t)N * 4), o_count = call.add((size_t)N * 4),
               o_status = call.add((size_t)N * 4), o_cost = call.add((size_t)N * 4), o_order = call.add((size_t)N * M * 4),
               o_eta = call.add((size_t)N * M * 4), o_depart = call.add((size_t)N * M * 4), o_swp = call.add((size_t)N * M * 4),
               o_release = call.add((size_t)N * K * 4), o_cell = call.add((size_t)S * M * 4), o_margin = call.add((size_t)S * M * 4),
               o_matrix = call.add((size_t)S * M * M * 4), o_reg = call.add(std::max<size_t>((size_t)S * R * 16, 4)),
               o_kind = call.add(std::max<size_t>((size_t)S * R * 4, 4)), o_cnt = call.add((size_t)S * 4),
               o_box = call.add(std::max<size_t>((size_t)S * Mw * 4, 1) * 4), o_nwall = call.add((size_t)S * 4),
               o_hz = call.add(std::max<size_t>((size_t)S * Mh * 3, 1) * 4), o_nhz = call.add((size_t)S * 4),
               o_todo = call.add((size_t)N * 4), o_len = call.add((size_t)N * 4), o_drop = call.add((size_t)N * 4);   // a replan's
  const auto shared = [&](size_t bytes) { return sh ? call.add(bytes) : (size_t)0; };   // a shared plan's: the other calls' buffer as it was
  const size_t o_team = shared((size_t)N * 4), o_best = shared((size_t)N * kPlanTourMasks * 4), o_share = shared((size_t)N * 4),
               o_unconv = shared((size_t)N * 4), o_tcover = shared((size_t)NT * 4), o_tdrop = shared((size_t)NT * 4),
               o_tmake = shared((size_t)NT * 4), o_ttotal = shared((size_t)NT * 8);
  if (const int rc = grow_plan_buf(e, e->plan_spec_buf, e->plan_spec_bytes, call.total)) return rc;
  const auto mine = [&](size_t off) { return e->plan_spec_buf + off; };
  const auto ints = [&](size_t off) { return reinterpret_cast<int*>(mine(off)); };
  const auto floats = [&](size_t off) { return reinterpret_cast<float*>(mine(off)); };
  unsigned char* occ_dev = reinterpret_cast<unsigned char*>(mine(o_occ));
  const PlanGrid grid{G, spec->extent, spec->h, spec->inv_h, spec->inflate};
  // the field list: the stations' fields of scene s at s * M + j (their goal cells are k_plan_station's to write), then the goals'
  std::vector<int32_t> fscene(F);
  for (int f = 0; f < S * M; ++f) fscene[f] = f / M;
  for (int f = 0; f < Fg; ++f) fscene[S * M + f] = field_scene[f];
  HIPC(hipMemcpyAsync(ints(o_fscene), fscene.data(), (size_t)F * 4, hipMemcpyHostToDevice, e->stream));
  if (Fg) HIPC(hipMemcpyAsync(ints(o_fgoal) + S * M, field_goal_cell, (size_t)Fg * 4, hipMemcpyHostToDevice, e->stream));
  if ((size_t)S * R) {
    HIPC(hipMemcpyAsync(mine(o_reg), regions->regions, (size_t)S * R * 16, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(mine(o_kind), regions->kinds, (size_t)S * R * 4, hipMemcpyHostToDevice, e->stream));
  }
  HIPC(hipMemcpyAsync(mine(o_cnt), region_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
  HIPC(hipMemcpyAsync(mine(o_start), start, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
  if (goal) {
    HIPC(hipMemcpyAsync(mine(o_goal), goal, (size_t)N * P * 4, hipMemcpyHostToDevice, e->stream));
    HIPC(hipMemcpyAsync(mine(o_fof), field_of, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
  }
  if (scene) HIPC(hipMemcpyAsync(mine(o_scene), scene, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
  if (walls || hz) {
    PlanOccArgs oa{};
    oa.g = grid; oa.Mw = Mw; oa.Mh = Mh; oa.occ = occ_dev;
    if (walls) {
      if ((size_t)S * Mw) HIPC(hipMemcpyAsync(mine(o_box), walls->boxes, (size_t)S * Mw * 16, hipMemcpyHostToDevice, e->stream));
      HIPC(hipMemcpyAsync(mine(o_nwall), wall_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
      oa.boxes = floats(o_box); oa.nwall = ints(o_nwall);
    }
    if (hz) {
      if ((size_t)S * Mh) HIPC(hipMemcpyAsync(mine(o_hz), hz->hazards, (size_t)S * Mh * 12, hipMemcpyHostToDevice, e->stream));
      HIPC(hipMemcpyAsync(mine(o_nhz), hz_counts.data(), (size_t)S * 4, hipMemcpyHostToDevice, e->stream));
      oa.hz = floats(o_hz); oa.nhz = ints(o_nhz);
    }
    hipLaunchKernelGGL(k_plan_occupancy, dim3(cdiv(cells, 256), S), dim3(256), ((size_t)4 * Mw + 3 * Mh) * sizeof(float), e->stream, oa);
  } else {
    HIPC(hipMemsetAsync(occ_dev, 0, (size_t)S * cells, e->stream));
  }
  if (n_avoid > 0) {
    PlanRegionOccArgs ra{};
    ra.g = grid; ra.regions = floats(o_reg); ra.kinds = ints(o_kind); ra.nreg = ints(o_cnt); ra.R = R; ra.n_avoid = n_avoid; ra.occ = occ_dev;
    for (int v = 0; v < n_avoid; ++v) { ra.lo[v] = avoid_lo[v]; ra.hi[v] = avoid_hi[v]; }
    hipLaunchKernelGGL(k_plan_region_occupancy, dim3(cdiv(cells, 256), S), dim3(256), 0, e->stream, ra);
  }
  PlanStationArgs sa{};
  sa.g = grid; sa.regions = floats(o_reg); sa.kinds = ints(o_kind); sa.nreg = ints(o_cnt); sa.R = R; sa.M = M; sa.occ = occ_dev;
  sa.cell = ints(o_cell); sa.margin = floats(o_margin); sa.field_goal = ints(o_fgoal);
  for (int j = 0; j < M; ++j) { sa.lo[j] = station_lo[j]; sa.hi[j] = station_hi[j]; }
  hipLaunchKernelGGL(k_plan_station, dim3(M, S), dim3(256), 0, e->stream, sa);
  if (!e->plan_lds_set) {   // 80 KB at 128 cells: above the 64 KB a kernel gets without asking
    HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(k_plan_field), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)plan_field_lds_bytes(128)));
    e->plan_lds_set = true;
  }
  const PlanFieldArgs fa{G, occ_dev, ints(o_fgoal), ints(o_fscene), ints(o_field), ints(o_sweeps)};
  hipLaunchKernelGGL(k_plan_field, dim3(F), dim3(kPlanFieldThreads), field_lds, e->stream, fa);
  const PlanTourMatrixArgs ma{S, M, cells, ints(o_cell), ints(o_field), ints(o_matrix)};
  hipLaunchKernelGGL(k_plan_tour_matrix, dim3(cdiv(S * M * M, 256)), dim3(256), 0, e->stream, ma);
  PlanTourArgs ta{};
  ta.g = grid; ta.N = N; ta.P = P; ta.M = M; ta.S = S; ta.has_goal = goal ? 1 : 0;
  ta.start = floats(o_start); ta.scene = scene ? ints(o_scene) : nullptr; ta.field_of = goal ? ints(o_fof) : nullptr;
  ta.cell = ints(o_cell); ta.matrix = ints(o_matrix); ta.field = ints(o_field); ta.sweeps = ints(o_sweeps);
  for (int j = 0; j < M; ++j) { ta.open_c[j] = open_c[j]; ta.close_c[j] = close_c[j]; ta.dwell_c[j] = dwell_c[j]; }
  ta.status = ints(o_status); ta.cost = ints(o_cost); ta.order = ints(o_order); ta.eta = ints(o_eta); ta.depart = ints(o_depart);
  std::vector<int32_t> team_todo;   // T: what no member of the team has done yet (alive until the stream is synchronised)
  if (sh) {
    team_todo.resize(N);
    for (int g = 0; g < NT; ++g) {   // the AND over the team's members, then the same T for each of them
      int32_t T = rp->todo[g * tsize];
      for (int k = 1; k < tsize; ++k) T &= rp->todo[g * tsize + k];
      for (int k = 0; k < tsize; ++k) team_todo[g * tsize + k] = T;
    }
    HIPC(hipMemcpyAsync(mine(o_team), team_todo.data(), (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
    const PlanTourBestArgs ba{ta, ints(o_team), rp->t0, ints(o_best), ints(o_unconv)};
    hipLaunchKernelGGL(k_plan_tour_best, dim3(N), dim3(64), 0, e->stream, ba);   // a wave per robot
    const PlanTeamShareArgs ha{tsize, M, sh->objective, rp->partial, ints(o_best), ints(o_team), ints(o_share), ints(o_tcover), ints(o_tdrop),
                               ints(o_tmake), reinterpret_cast<long long*>(mine(o_ttotal))};
    hipLaunchKernelGGL(k_plan_team_share, dim3(NT), dim3(64), 0, e->stream, ha);   // a wave per team
    const PlanTourResumeArgs ra{ta, ints(o_share), rp->t0, 0, ints(o_len), ints(o_drop)};
    hipLaunchKernelGGL(k_plan_tour_resume, dim3(N), dim3(64), 0, e->stream, ra);
    const PlanTeamVoidArgs va{N, M, tsize, ints(o_team), ints(o_tmake), ints(o_tdrop), ints(o_unconv), ta.status, ta.cost, ta.order, ta.eta,
                              ta.depart, ints(o_len), ints(o_drop)};
    hipLaunchKernelGGL(k_plan_team_void, dim3(cdiv(N, 256)), dim3(256), 0, e->stream, va);
  } else if (rp) {
    HIPC(hipMemcpyAsync(mine(o_todo), rp->todo, (size_t)N * 4, hipMemcpyHostToDevice, e->stream));
    const PlanTourResumeArgs ra{ta, ints(o_todo), rp->t0, rp->partial, ints(o_len), ints(o_drop)};
    hipLaunchKernelGGL(k_plan_tour_resume, dim3(N), dim3(64), 0, e->stream, ra);   // a wave per robot
  } else {
    hipLaunchKernelGGL(k_plan_tour, dim3(N), dim3(64), 0, e->stream, ta);   // a wave per robot
  }
  PlanTourPathArgs pa{};
  pa.g = grid; pa.N = N; pa.K = K; pa.P = P; pa.M = M; pa.S = S; pa.has_goal = ta.has_goal; pa.pace = pace;
  pa.start = ta.start; pa.goal = goal ? floats(o_goal) : nullptr; pa.scene = ta.scene; pa.field_of = ta.field_of;
  pa.cell = ta.cell; pa.occ = occ_dev; pa.field = ta.field; pa.depart = ta.depart; pa.order = ta.order; pa.eta = ta.eta;
  pa.wp = floats(o_wp); pa.nwp = ints(o_nwp); pa.count = ints(o_count); pa.status = ta.status; pa.cost = ta.cost;
  pa.swp = ints(o_swp); pa.release = ints(o_release);
  HIPC(hipMemsetAsync(pa.wp, 0, (size_t)N * K * P * 4, e->stream));
  HIPC(hipMemsetAsync(pa.release, 0, (size_t)N * K * 4, e->stream));
  HIPC(hipMemsetAsync(pa.swp, 0xFF, (size_t)N * M * 4, e->stream));   // -1: no anchor waypoint
  if (rp) {
    const PlanTourPathLegsArgs la{pa, ints(o_len)};
    hipLaunchKernelGGL(k_plan_tour_path_legs, dim3(cdiv(N, 256 / kPlanLegLanes)), dim3(256), 0, e->stream, la);   // 16 lanes a robot
  } else {
    hipLaunchKernelGGL(k_plan_tour_path, dim3(cdiv(N, 256)), dim3(256), 0, e->stream, pa);
  }
  HIPC(hipGetLastError());
  if (rp) {
    HIPC(hipMemcpyAsync(rp->tour_len_out, ints(o_len), (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
    HIPC(hipMemcpyAsync(rp->dropped_out, ints(o_drop), (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  }
  if (sh) {
    HIPC(hipMemcpyAsync(sh->share_out, ints(o_share), (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
    HIPC(hipMemcpyAsync(sh->team_cover_out, ints(o_tcover), (size_t)NT * 4, hipMemcpyDeviceToHost, e->stream));
    HIPC(hipMemcpyAsync(sh->team_dropped_out, ints(o_tdrop), (size_t)NT * 4, hipMemcpyDeviceToHost, e->stream));
    HIPC(hipMemcpyAsync(sh->team_makespan_out, ints(o_tmake), (size_t)NT * 4, hipMemcpyDeviceToHost, e->stream));
    HIPC(hipMemcpyAsync(sh->team_total_out, mine(o_ttotal), (size_t)NT * 8, hipMemcpyDeviceToHost, e->stream));
  }
  HIPC(hipMemcpyAsync(waypoints_out, pa.wp, (size_t)N * K * P * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(n_waypoints_out, pa.nwp, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(count_out, pa.count, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(status_out, pa.status, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(cost_out, pa.cost, (size_t)N * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(tour_order_out, pa.order, (size_t)N * M * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(tour_eta_out, pa.eta, (size_t)N * M * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(station_waypoint_out, pa.swp, (size_t)N * M * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(release_out, pa.release, (size_t)N * K * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(station_cell_out, sa.cell, (size_t)S * M * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(station_margin_out, sa.margin, (size_t)S * M * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipMemcpyAsync(matrix_out, ma.matrix, (size_t)S * M * M * 4, hipMemcpyDeviceToHost, e->stream));
  if (occupancy_out) HIPC(hipMemcpyAsync(occupancy_out, occ_dev, (size_t)S * cells, hipMemcpyDeviceToHost, e->stream));
  if (sweeps_out) HIPC(hipMemcpyAsync(sweeps_out, ints(o_sweeps), (size_t)F * 4, hipMemcpyDeviceToHost, e->stream));
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}

int mobrob_ppo_spec_plan(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls, const mobrob_hazards_t* hz,
                         const mobrob_spec_t* regions, int32_t n_stations, const int32_t* station_lo, const int32_t* station_hi,
                         int32_t n_avoid, const int32_t* avoid_lo, const int32_t* avoid_hi, const int32_t* open_c, const int32_t* close_c,
                         const int32_t* dwell_c, int32_t pace, const float* start, const float* goal, const int32_t* field_of,
                         const int32_t* field_goal_cell, const int32_t* field_scene, float* waypoints_out, int32_t* n_waypoints_out,
                         int32_t* count_out, int32_t* status_out, int32_t* cost_out, int32_t* tour_order_out, int32_t* tour_eta_out,
                         int32_t* station_waypoint_out, int32_t* release_out, int32_t* station_cell_out, float* station_margin_out,
                         int32_t* matrix_out, uint8_t* occupancy_out, int32_t* sweeps_out) {
  return spec_plan_run("spec_plan", nullptr, e, spec, walls, hz, regions, n_stations, station_lo, station_hi, n_avoid, avoid_lo, avoid_hi, open_c,
                       close_c, dwell_c, pace, start, goal, field_of, field_goal_cell, field_scene, waypoints_out, n_waypoints_out, count_out,
                       status_out, cost_out, tour_order_out, tour_eta_out, station_waypoint_out, release_out, station_cell_out,
                       station_margin_out, matrix_out, occupancy_out, sweeps_out);
}

int mobrob_ppo_spec_replan(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls, const mobrob_hazards_t* hz,
                           const mobrob_spec_t* regions, int32_t n_stations, const int32_t* station_lo, const int32_t* station_hi,
                           int32_t n_avoid, const int32_t* avoid_lo, const int32_t* avoid_hi, const int32_t* open_c, const int32_t* close_c,
                           const int32_t* dwell_c, int32_t pace, const float* start, const float* goal, const int32_t* field_of,
                           const int32_t* field_goal_cell, const int32_t* field_scene, const int32_t* todo, int32_t step0_ticks,
                           int32_t partial, float* waypoints_out, int32_t* n_waypoints_out, int32_t* count_out, int32_t* status_out,
                           int32_t* cost_out, int32_t* tour_order_out, int32_t* tour_eta_out, int32_t* station_waypoint_out,
                           int32_t* release_out, int32_t* station_cell_out, float* station_margin_out, int32_t* matrix_out,
                           uint8_t* occupancy_out, int32_t* sweeps_out, int32_t* tour_len_out, int32_t* dropped_out) {
  const SpecReplan rp{todo, step0_ticks, partial, tour_len_out, dropped_out, nullptr};
  return spec_plan_run("spec_replan", &rp, e, spec, walls, hz, regions, n_stations, station_lo, station_hi, n_avoid, avoid_lo, avoid_hi, open_c,
                       close_c, dwell_c, pace, start, goal, field_of, field_goal_cell, field_scene, waypoints_out, n_waypoints_out, count_out,
                       status_out, cost_out, tour_order_out, tour_eta_out, station_waypoint_out, release_out, station_cell_out,
                       station_margin_out, matrix_out, occupancy_out, sweeps_out);
}

int mobrob_ppo_spec_plan_share(mobrob_ppo_engine_t* e, const mobrob_plan_spec_t* spec, const mobrob_walls_t* walls, const mobrob_hazards_t* hz,
                               const mobrob_spec_t* regions, int32_t n_stations, const int32_t* station_lo, const int32_t* station_hi,
                               int32_t n_avoid, const int32_t* avoid_lo, const int32_t* avoid_hi, const int32_t* open_c, const int32_t* close_c,
                               const int32_t* dwell_c, int32_t pace, const float* start, const float* goal, const int32_t* field_of,
                               const int32_t* field_goal_cell, const int32_t* field_scene, const int32_t* todo, int32_t step0_ticks,
                               int32_t partial, int32_t team_size, int32_t objective, float* waypoints_out, int32_t* n_waypoints_out,
                               int32_t* count_out, int32_t* status_out, int32_t* cost_out, int32_t* tour_order_out, int32_t* tour_eta_out,
                               int32_t* station_waypoint_out, int32_t* release_out, int32_t* station_cell_out, float* station_margin_out,
                               int32_t* matrix_out, uint8_t* occupancy_out, int32_t* sweeps_out, int32_t* tour_len_out, int32_t* dropped_out,
                               int32_t* share_out, int32_t* team_cover_out, int32_t* team_dropped_out, int32_t* team_makespan_out,
                               int64_t* team_total_out) {
  const SpecShare sh{team_size, objective, share_out, team_cover_out, team_dropped_out, team_makespan_out, team_total_out};
  const SpecReplan rp{todo, step0_ticks, partial, tour_len_out, dropped_out, &sh};
  return spec_plan_run("spec_plan_share", &rp, e, spec, walls, hz, regions, n_stations, station_lo, station_hi, n_avoid, avoid_lo, avoid_hi,
                       open_c, close_c, dwell_c, pace, start, goal, field_of, field_goal_cell, field_scene, waypoints_out, n_waypoints_out,
                       count_out, status_out, cost_out, tour_order_out, tour_eta_out, station_waypoint_out, release_out, station_cell_out,
                       station_margin_out, matrix_out, occupancy_out, sweeps_out);
}

// ---- buffers ----------------------------------------------------------------------------------------
static bool feeds_train_records(int32_t which) {
  return which == MOBROB_BUF_ACTIONS || which == MOBROB_BUF_VALUES || which == MOBROB_BUF_LOG_PROBS ||
         which == MOBROB_BUF_ADVANTAGES || which == MOBROB_BUF_RETURNS;
}

static int buffer_lookup(mobrob_ppo_engine* e, int32_t which, void** ptr, size_t* bytes) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  const size_t N = e->N, T = e->T;
  void* p = nullptr;
  size_t b = 0;
  switch (which) {
    case MOBROB_BUF_OBS: p = e->obs; b = (T + 1) * N * e->Dp * 4; break;
    case MOBROB_BUF_ACTIONS: p = e->actions; b = T * N * e->A * 4; break;
    case MOBROB_BUF_REWARDS: p = e->rewards; b = T * N * 4; break;
    case MOBROB_BUF_EPISODE_STARTS: p = e->es; b = T * N * 4; break;
    case MOBROB_BUF_VALUES: p = e->values; b = T * N * 4; break;
    case MOBROB_BUF_LOG_PROBS: p = e->logp; b = T * N * 4; break;
    case MOBROB_BUF_ADVANTAGES: p = e->adv; b = T * N * 4; break;
    case MOBROB_BUF_RETURNS: p = e->ret; b = T * N * 4; break;
    case MOBROB_BUF_PARAMS: p = e->params; b = (size_t)e->P * 4; break;
    case MOBROB_BUF_GRADS: p = e->grads; b = (size_t)e->P * 4; break;
    case MOBROB_BUF_ADVSTAT: p = e->advstat; b = (size_t)e->nmb * 4 * 8; break;
    case MOBROB_BUF_LAST_VALUES: p = e->last_values; b = N * 4; break;
    case MOBROB_BUF_LAST_DONES: p = e->last_dones; b = N * 4; break;
    case MOBROB_BUF_CLIPPED_ACTIONS: p = e->clip_act; b = N * e->A * 4; break;
    case MOBROB_BUF_EPISODE_START_STATE: p = e->prev_dones; b = N * 4; break;
    case MOBROB_BUF_TERMINAL_OBS: p = e->term_obs; b = N * e->Dp * 4; break;
    case MOBROB_BUF_TERMINAL_VALUES: p = e->term_val; b = N * 4; break;
    case MOBROB_BUF_TRUNCATED: p = e->trunc_dev; b = N; break;
    case MOBROB_BUF_ENV_STATE: p = e->gstate[0]; b = N * kGoalStateFloats * 4; break;
    case MOBROB_BUF_GRAD_EXCHANGE: p = e->grads; b = (size_t)(e->P + 8) * 4; break;
    case MOBROB_BUF_SDE_NOISE:
      if (!e->sde) return fail(MOBROB_ERR_STATE, "the engine was not created with use_sde");
      p = e->sde_E; b = N * (size_t)e->HL * e->A * 4; break;
    default: return fail(MOBROB_ERR_INVALID, "unknown buffer id %d", which);
  }
  if (ptr) *ptr = p;
  if (bytes) *bytes = b;
  return MOBROB_OK;
}

int mobrob_ppo_buffer_info(mobrob_ppo_engine_t* e, int32_t which, void** ptr, size_t* bytes) {
  CHK(buffer_lookup(e, which, ptr, bytes));
  if (ptr && feeds_train_records(which)) e->train_rec_external = true;  // see ensure_train_records
  return MOBROB_OK;
}

int mobrob_ppo_read_buffer(mobrob_ppo_engine_t* e, int32_t which, void* host, size_t bytes) {
  if (!e || !host) return fail(MOBROB_ERR_INVALID, "read_buffer: null argument");
  void* p; size_t b;
  CHK(buffer_lookup(e, which, &p, &b));
  if (which == MOBROB_BUF_OBS) {  // host layout [T+1][N][D]
    const size_t rows = (size_t)(e->T + 1) * e->N;
    if (bytes != rows * e->D * 4) return fail(MOBROB_ERR_INVALID, "read_buffer(OBS): expected %zu bytes", rows * e->D * 4);
    HIPC(hipMemcpy2DAsync(host, (size_t)e->D * 4, p, (size_t)e->Dp * 4, (size_t)e->D * 4, rows, hipMemcpyDeviceToHost, e->stream));
  } else {
    if (bytes != b) return fail(MOBROB_ERR_INVALID, "read_buffer(%d): expected %zu bytes, got %zu", which, b, bytes);
    HIPC(hipMemcpyAsync(host, p, b, hipMemcpyDeviceToHost, e->stream));
  }
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}

int mobrob_ppo_write_buffer(mobrob_ppo_engine_t* e, int32_t which, const void* host, size_t bytes) {
  if (!e || !host) return fail(MOBROB_ERR_INVALID, "write_buffer: null argument");
  void* p; size_t b;
  CHK(buffer_lookup(e, which, &p, &b));
  if (feeds_train_records(which)) e->train_rec_valid = false;
  if (which == MOBROB_BUF_OBS) {
    const size_t rows = (size_t)(e->T + 1) * e->N;
    if (bytes != rows * e->D * 4) return fail(MOBROB_ERR_INVALID, "write_buffer(OBS): expected %zu bytes", rows * e->D * 4);
    HIPC(hipMemcpy2DAsync(p, (size_t)e->Dp * 4, host, (size_t)e->D * 4, (size_t)e->D * 4, rows, hipMemcpyHostToDevice, e->stream));
  } else {
    if (bytes != b) return fail(MOBROB_ERR_INVALID, "write_buffer(%d): expected %zu bytes, got %zu", which, b, bytes);
    HIPC(hipMemcpyAsync(p, host, b, hipMemcpyHostToDevice, e->stream));
    if (which == MOBROB_BUF_PARAMS) repack(e);
  }
  HIPC(hipStreamSynchronize(e->stream));
  return MOBROB_OK;
}

int mobrob_ppo_feistel_permutation(mobrob_ppo_engine_t* e, int64_t n, uint64_t key, int64_t* out) {
  if (!e || !out || n < 1 || n > ((int64_t)1 << 30)) return fail(MOBROB_ERR_INVALID, "feistel_permutation: bad argument");
  int64_t* d = nullptr;
  HIPC(hipMalloc(&d, (size_t)n * 8));
  hipLaunchKernelGGL(k_perm_feistel, dim3(cdiv((int)n, 256)), dim3(256), 0, e->stream, (int)n, 1, (int)n,
                     feistel_half_bits((uint64_t)n), (uint32_t)key, (uint32_t)(key >> 32), (int*)nullptr, d);
  hipError_t r = hipMemcpyAsync(out, d, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(e->stream);
  (void)hipFree(d);
  if (r != hipSuccess) return fail(MOBROB_ERR_HIP, "feistel_permutation: %s", hipGetErrorString(r));
  return MOBROB_OK;
}

// ---- profiling --------------------------------------------------------------------------------------
int mobrob_ppo_profile_enable(mobrob_ppo_engine_t* e, int32_t on) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  HIPC(hipStreamSynchronize(e->stream));
  prof_resolve(e);
  e->prof_on = on != 0;
  e->prof_mask = on == 1 ? ~0u : (uint32_t)on >> 1;  // 1: every phase; otherwise bit (id + 1) selects phase id
  for (int i = 0; i < MOBROB_K_COUNT; ++i) { e->prof_ms[i] = 0; e->prof_calls[i] = 0; }
  return MOBROB_OK;
}
int mobrob_ppo_profile_read(mobrob_ppo_engine_t* e, double* ms, int64_t* calls) {
  if (!e) return fail(MOBROB_ERR_INVALID, "null engine");
  HIPC(hipStreamSynchronize(e->stream));
  prof_resolve(e);
  for (int i = 0; i < MOBROB_K_COUNT; ++i) {
    if (ms) ms[i] = e->prof_ms[i];
    if (calls) calls[i] = e->prof_calls[i];
  }
  return MOBROB_OK;
}

#if defined(MOBROB_STAMPS) || defined(MOBROB_PAIR_STAMPS) || defined(MOBROB_EPOCH_STAMPS)
// diagnostic build only (not part of include/mobrob_ppo.h)
int mobrob_dbg_read_stamps(mobrob_ppo_engine_t* e, unsigned long long* out32, int reset) {
  HIPC(hipStreamSynchronize(e->stream));
  HIPC(hipMemcpy(out32, e->fused.stamps, 32 * 8, hipMemcpyDeviceToHost));
  if (reset) HIPC(hipMemset(e->fused.stamps, 0, 32 * 8));
  return 0;
}
#endif

}  // extern "C"
