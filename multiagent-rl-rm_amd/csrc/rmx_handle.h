// rmx_handle.h — private to the C ABI layer (rmx_capi*.cpp): the handle, its per-subsystem state, the thread's
// last error, and the helpers more than one of those files needs.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "rmx_host.h"
#include "rmx_hoststep.h"
#include "rmx_internal.h"

struct rmx_handle {
  rmx_config cfg;  // scalars only (host table pointers cleared after upload)
  // cfg.device == RMX_DEVICE_HOST: the CPU path (rmx_hoststep.cpp) serves every entry point; nothing below is used
  rmx::HostEngine* host = nullptr;
  // rmx_step_seq (rmx_capi_seq.cpp)
  struct Seq {
    // the recorded window, reused while its inputs are unchanged: the handle's parameter block
    // (fast_params), the call's arguments; key names it to the device queue (its prebuilt packets)
    std::vector<rmx::StepLaunch> window;
    rmx::FastParams base;
    const int32_t* actions = nullptr;
    const double* out = nullptr;
    int64_t stride = 0;
    int32_t k = 0;
    int autoreset = -1;
    uint64_t key = 0;  // 0: nothing recorded
    bool queue_off = false;  // RMX_QUEUE=0 at rmx_create: rmx_step_seq always takes the stream path
    // packed windows (rmx_layout.h "the packed record"): RMX_SEQ_PACKED=0 at rmx_create turns them off; the record
    // buffer is allocated by the first eligible window (a failed allocation is remembered: windows stay unpacked)
    bool packed_off = false;
    // RMX_SEQ_RELEASE=1 at rmx_create: every packet of a packed window keeps its release fence (rmx::seq_handoff)
    bool release_all = false;
    bool pk_failed = false;
    bool pk_refused = false;  // the kernel side did not take the window kernel for this handle: not tried again
    uint32_t* d_pk = nullptr;
    bool is_packed = false;  // the recorded window is a packed one
    int dispatch = RMX_SEQ_NONE;  // how the last rmx_step_seq ran
    int64_t recordings = 0;       // windows recorded (a repeated identical call reuses the last one)
  } seq;
  int device = 0;
  int block = 256;
  // measured on MI355X (scripts/variants.py): thread-per-env is faster for the HBM round-trip step
  // kernel (5.1 vs 4.0 TB/s at 4M envs, equal at 65k); lane-per-agent is 1.6-2.3x faster for the
  // register-resident fused rollout.
  int step_layout = rmx::kLayoutThreadPerEnv;
  int rollout_layout = rmx::kLayoutLanePerAgent;
  void* d_tables = nullptr;
  size_t tables_bytes = 0;  // multiple of 16
  int32_t off_cell = 0, off_ev = 0, off_nq = 0, off_rr = 0, off_sh = 0, off_qrm = 0;
  int32_t n_qrm[RMX_MAX_AGENTS]{}, enc_nq[RMX_MAX_AGENTS]{};
  float* d_disc = nullptr;
  double* d_slab = nullptr;
  int64_t n_waves = 0;
  double* d_stats = nullptr;  // [RMX_NSTATS] scratch for rmx_stats_host
  uint32_t* d_err = nullptr;
  rmx_buffers buf{};
  bool bound = false;
  uint64_t base_seed = 123;  // last rmx_reset seed (autoreset reseeds from it)
  uint64_t digest = 0;       // config_digest at rmx_create (checkpoint identity)
  int32_t diag = 0;          // RMX_DIAG builds only: diagnostic kernel variants
  unsigned long long* d_stamps = nullptr;  // RMX_DIAG builds: in-kernel stamps of the fast kernel
  int32_t init_q[RMX_MAX_AGENTS]{}, final_q[RMX_MAX_AGENTS]{}, start_x[RMX_MAX_AGENTS]{}, start_y[RMX_MAX_AGENTS]{};
  // deterministic fast path (rmx::FastParams): pre-composed move words + packed RM entries
  bool fast = false;  // the thread-per-env fast kernel (step_fast_kernel) runs this handle's steps
  int fast_wave_stats = 0;  // episode stats: 1 per-wave slab (large N), 0 per-env atomics; RMX_FAST_STATS=wave|env
  int fast_skip = 0;        // rmx::kSkipRare / kSkipRareNT (by size; RMX_FAST_SKIP=2|3 forces one)
  int generic_skip = 0;     // 1: the generic kernel skips every unchanged column word (large N)
  int fast_block = 256;     // workgroup size of the fast step kernel: 64 below 1M envs, 256 from there
  int rollout_lds = 1;      // fast rollout: tables staged into LDS (1) or read through L2 (0); RMX_ROLLOUT_LDS
  int fast_tables = rmx::kTblGlobal;  // table mode rmx::kTblGlobal / kTblMerged / kTblMerged4; RMX_FAST_TABLES
  void* d_fast = nullptr;
  void* d_merged = nullptr;  // kTblMerged table (RMX_FAST_TABLES=merged or the default where measured faster)
  size_t merged_bytes = 0;
  int merged_sections = 0;  // agent sections stored in d_merged (identical ones shared)
  // fast-path episode statistics: es_ret [N] f64 | es_cnt [N] u64 | es_succ [N] u32
  unsigned char* d_es = nullptr;
  size_t es_bytes = 0;
  double* es_ret = nullptr;
  unsigned long long* es_cnt = nullptr;
  uint32_t* es_succ = nullptr;
  // rmx_step_report's fused report, in the same allocation: per-block partials [ceil(N/64)][RMX_NSTATS] | ticket
  double* rpt_partial = nullptr;
  unsigned int* rpt_ticket = nullptr;
  int32_t fast_n16 = 0, fast_off_rm = 0, fast_off_info = 0;
  uint8_t fast_qrm_q[RMX_MAX_AGENTS][rmx::kFastMaxQrm]{};  // QRM state lists for the fast kernel
  int32_t mg_base[RMX_MAX_AGENTS]{};                        // merged-table record index of each agent's section
  size_t merged4_off = 0, merged4_bytes = 0;  // kTblMerged4 records, after the 16-B records in d_merged
  uint32_t mg_palb[RMX_MAX_AGENTS]{};  // kTblMerged4: each agent's reward palette as four signed bytes
  // FrozenLake random starts: non-hole cells (x-major) and the per-env shuffle workspace [N][n_free]
  int32_t n_free = 0;
  uint16_t* d_free = nullptr;
  uint16_t* d_start_ws = nullptr;
  // random starts: the step kernel's next-episode shuffle in progress, [4][N] u64 generator | [N] index | [N] tag
  unsigned char* d_nx = nullptr;
  // slip / random starts with seed_episode_stride == 0 (rmx::kRngFixedSeed): every env's post-seed (post-shuffle)
  // generator and start cells for the current base seed (the reset cache, rmx::start_cache_bytes layout), rebuilt
  // whenever the base seed changes
  bool seed_fixed = false;
  unsigned char* d_rsc = nullptr;
  // the base seed changed without a launch on a caller stream (rmx_reset_sync): the start cache and the next-episode
  // precompute tags are brought up to date on the stream of the next fast launch, ahead of it
  bool rs_stale = false;
  // the rng columns may hold generators of another base seed than the cache's (rmx::FastParams::rs_dirty)
  bool rs_dirty = true;
  // resident host-boundary stepper (rmx_reset_sync / rmx_step_sync, rmx_sync.hip; rmx_capi_sync.cpp): the pinned
  // coherent mailbox, its own non-blocking stream, the completion event of the last launch and the request numbering
  struct Sync {
    unsigned char* mb = nullptr;
    size_t bytes = 0;
    rmx::SyncIO io{};
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr, dep = nullptr;
    bool running = false;  // a resident workgroup may be executing (done not yet observed complete)
    bool pending = false;  // a request is posted and not yet acknowledged (rmx_step_sync_begin)
    void* caller = nullptr;  // the caller's stream of the outstanding request (a relaunch orders after it)
    uint32_t seq = 0;      // last request posted
    uint32_t served = 0;   // requests up to this number need no service (seq0 of the next launch)
    int oneshot = 0;       // RMX_SYNC=launch: one launch per request (A/B of the resident workgroup)
    uint64_t idle_ticks = 0, life_ticks = 0;
    bool enc = false;  // the records' enc_state word is meaningful (every agent has an encoder stride)
#ifdef RMX_DIAG
    std::chrono::steady_clock::time_point t_post;  // diag: when the last request was posted
    double wait_ns = 0;                             // diag: post -> acknowledgement seen by the host
#endif
  } sync;
  // the learner bound by rmx_learn_bind to a device handle (a host handle's is host->learn / host->learn_on): the
  // caller's tables and the handle's device copy of phi (rmx_capi_learn.cpp)
  struct Learn {
    rmx::LearnParams params{};
    bool on = false;
    double* d_phi = nullptr;
    uint64_t* rng = nullptr;  // rmx_learn_rng_bind: the learners' numpy generators, caller's [5][A][N]
    // rmx_learn_lambda_bind: the learners are Q(lambda) ones over the caller's trace lists (lam_on)
    rmx::LambdaParams lam{};
    bool lam_on = false;
    // rmx_learn_eps_bind: the per-learner epsilon schedule over the caller's column [A][N] (eps.col == NULL: none)
    rmx::EpsParams eps{};
    // rmx_learn_rmax_bind: the learners are R-max ones over the caller's model arrays (rmax_on); the engine's own
    // hand-over between the step kernel and the solve kernel (one allocation, d_rmax), the solve kernel's grid
    rmx::RMaxParams rmax{};
    bool rmax_on = false;
    rmx::RMaxWork work{};
    unsigned char* d_rmax = nullptr;
    int rmax_grid = rmx::kRMaxGrid;
    // rmx_learn_qrmax_bind: the learners are QR-max ones over the caller's model arrays (qrmax_on); the engine's own
    // worklist between the step kernel and the solve kernel (one allocation, d_qrmax), the solve kernel's grid
    rmx::QRMaxParams qrmax{};
    bool qrmax_on = false;
    rmx::RMaxWork qwork{};
    unsigned char* d_qrmax = nullptr;
    int qrmax_grid = rmx::kRMaxGrid;
  } learn;
};

namespace rmx {
namespace capi {

// Default fast-path table mode (overridable by RMX_FAST_TABLES for tests), chosen by measurement on MI355X at
// 65,536 envs (profiles/r01_ab_log.md c12/c15/c25): the tables read from the global blob (no staging,
// no block barrier); the merged single-lookup table while it is small.
// 128 KiB: config 5's shared-section table (77 KB) beats the global blob (3.74-3.76 vs 3.86-3.87 us, r01_ab_log
// c78); its unshared 233 KB table lost (c26)
constexpr size_t kFastMergedDefaultBytes = 128 * 1024;
// Episode statistics: per-env no-return atomics are off the critical path at small N, but at large N
// their count (3 per finished env) costs 10-15 % of the step (8.4M envs: 173 vs 191-198 us); there the
// per-wave slab (one DPP reduction + one 32-B store per wave) wins.
constexpr int64_t kFastWaveStatsMinEnvs = 1 << 20;
// The same size switches the generic kernel to skipping stores of every unchanged column word and the fast
// kernel to 256-thread workgroups (the bandwidth regime).
constexpr int64_t kFastSkipMinEnvs = 1 << 20;
// Non-temporal column stores from this many env x agent instances on (see rmx_create).
constexpr int64_t kFastNtMinInstances = int64_t(1) << 23;

// the calling thread's last error (rmx_last_error)
inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

inline int hip_fail(hipError_t e, const char* what) {
  return fail(RMX_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr, what)            \
  do {                                 \
    hipError_t _e = (expr);            \
    if (_e != hipSuccess) return rmx::capi::hip_fail(_e, what); \
  } while (0)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline int check_bound(const rmx_handle* h) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (!h->bound) return fail(RMX_E_STATE, "buffers not bound (rmx_bind)");
  return RMX_OK;
}

inline int64_t threads_for(const rmx_handle* h, int layout) {
  return layout == rmx::kLayoutLanePerAgent ? h->cfg.n_envs * rmx::lanes_per_env(h->cfg.n_agents) : h->cfg.n_envs;
}

inline dim3 grid_for(const rmx_handle* h, int layout) {
  return dim3((unsigned)((threads_for(h, layout) + h->block - 1) / h->block));
}

// where the random starts' jump table (rmx_capi_create.cpp RsJumpTable) lies in the handle's d_nx allocation
inline size_t nx_jump_offset(int64_t n_envs) { return (40 * (size_t)n_envs + 255) & ~(size_t)255; }

// rmx_capi.cpp
rmx::KParams base_params(const rmx_handle* h);
rmx::FastParams fast_params(const rmx_handle* h);
bool fast_applies(const rmx_handle* h);
hipError_t reduce_stats(const rmx_handle* h, double* out, hipStream_t st);
hipError_t refresh_starts(rmx_handle* h, hipStream_t st);
int starts_current(rmx_handle* h, void* stream);
rmx::FastParams step_fp(const rmx_handle* h, const int32_t* actions, uint64_t seed, int64_t t_global, int autoreset);
int do_step(rmx_handle* h, const int32_t* actions, int hashed, uint64_t seed, int64_t t_global, int autoreset,
            void* stream);
bool report_fuses(const rmx_handle* h);
rmx::FastParams report_fp(const rmx_handle* h, const int32_t* actions, int autoreset, double* stats_out);

// rmx_capi_learn.cpp.  Empty the Q(lambda) trace lists of the masked envs (NULL: every env) in stream order; nothing
// on a handle without Q(lambda) bound.  A host handle's lists are emptied by HostEngine::reset itself.
int lambda_clear(rmx_handle* h, const uint8_t* env_mask_dev, void* stream);

// rmx_capi_sync.cpp.  End the resident workgroup (if any): the device columns are current afterwards.
int sync_end(rmx_handle* h);

#define SYNC_END_OR_RETURN(h)   \
  do {                          \
    const int _rc = rmx::capi::sync_end(h); \
    if (_rc) return _rc;        \
  } while (0)

}  // namespace capi
}  // namespace rmx
