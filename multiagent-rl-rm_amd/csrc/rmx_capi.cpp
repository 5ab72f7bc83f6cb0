// rmx_capi.cpp — the extern "C" boundary of include/rmx.h (handle lifetime, validation, uploads,
// launches).  Each entry point maps onto one reference call site; see include/rmx.h for the map.
// rmx_create, the mailbox stepper, rmx_step_seq, the learners and the checkpoint blob are in rmx_capi_create.cpp,
// rmx_capi_sync.cpp, rmx_capi_seq.cpp, rmx_capi_learn.cpp and rmx_capi_state.cpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "rmx_handle.h"

using namespace rmx::capi;

rmx::KParams rmx::capi::base_params(const rmx_handle* h) {
  rmx::KParams p;
  std::memset(&p, 0, sizeof(p));
  const rmx_config& c = h->cfg;
  p.tables = reinterpret_cast<const uint4*>(h->d_tables);
  p.tables_n16 = (int32_t)(h->tables_bytes / 16);
  p.skip_same = h->generic_skip;  // the generic thread-per-env kernel: every unchanged word or none
  p.off_cell = h->off_cell;
  p.off_ev = h->off_ev;
  p.off_nq = h->off_nq;
  p.off_rr = h->off_rr;
  p.off_sh = h->off_sh;
  p.off_qrm = h->off_qrm;
  p.reward_modifier = c.reward_modifier;
  p.n_qrm_max = c.n_qrm_max;
  p.stochastic = c.stochastic ? 1 : 0;
  rmx::slip_fill(p, c);
  p.seed_scale = c.seed_scale;
  p.seed_env_stride = c.seed_env_stride;
  p.seed_episode_stride = c.seed_episode_stride;
  p.base_seed = h->base_seed;
  p.rng = h->buf.rng;
  p.episode = h->buf.episode;
  p.rng_on = (c.stochastic || c.random_starts) ? 1 : 0;
  p.random_starts = c.random_starts ? 1 : 0;
  p.n_free = h->n_free;
  p.free_cells = h->d_free;
  p.start_ws = h->d_start_ws;
  if (h->d_rsc) {
    p.rs_cells = reinterpret_cast<uint32_t*>(h->d_rsc);
    p.rs_rng = reinterpret_cast<uint64_t*>(h->d_rsc + rmx::start_cache_rng_off(c.n_agents, c.n_envs));
  }
  for (int a = 0; a < RMX_MAX_AGENTS; ++a) {
    p.n_qrm[a] = h->n_qrm[a];
    p.enc_nq[a] = h->enc_nq[a];
  }
  p.W = c.width;
  p.HW = c.width * c.height;
  p.A = c.n_agents;
  p.Q = c.n_rm_states;
  p.E = c.n_events;
  p.max_t = c.max_t;
  p.N = c.n_envs;
  p.hazard_penalty = c.hazard_penalty;
  p.wall_penalty = c.wall_penalty;
  p.hazard_fail = c.hazard_fail ? 1 : 0;
  p.wall_fail = c.wall_fail ? 1 : 0;
  p.has_shaping = c.has_shaping ? 1 : 0;
  p.gamma_is_one = (c.gamma == 1.0f) ? 1 : 0;
  for (int a = 0; a < RMX_MAX_AGENTS; ++a) {
    p.init_q[a] = h->init_q[a];
    p.final_q[a] = h->final_q[a];
    p.start_x[a] = h->start_x[a];
    p.start_y[a] = h->start_y[a];
  }
  p.disc = h->d_disc;
  p.pos_x = h->buf.pos_x;
  p.pos_y = h->buf.pos_y;
  p.rm_q = h->buf.rm_q;
  p.flags = h->buf.flags;
  p.ep_ret = h->buf.ep_ret;
  p.t = h->buf.t;
  p.reward = h->buf.reward;
  p.shaping = h->buf.shaping;
  p.env_done = h->buf.env_done;
  p.renv = h->buf.renv;
  p.enc_state = h->buf.enc_state;
  if (c.n_qrm_max > 0 && h->buf.qrm_s) {
    p.qrm_s = h->buf.qrm_s;
    p.qrm_sn = h->buf.qrm_sn;
    p.qrm_rq = h->buf.qrm_rq;
    p.qrm_done = h->buf.qrm_done;
  }
  p.env_offset = c.env_offset;
  p.n_global = c.n_envs_global;
  p.slab = h->d_slab;
  p.err = h->d_err;
  p.diag = h->diag;
  return p;
}

rmx::FastParams rmx::capi::fast_params(const rmx_handle* h) {
  rmx::FastParams p;
  std::memset(&p, 0, sizeof(p));
  const rmx_config& c = h->cfg;
  p.tables = reinterpret_cast<const uint4*>(h->d_fast);
  p.n16 = h->fast_n16;
  p.off_rm = h->fast_off_rm;
  p.off_info = h->fast_off_info;
  p.A = c.n_agents;
  p.W = c.width;
  p.E = c.n_events;
  p.max_t = c.max_t;
  p.N = (int32_t)c.n_envs;
  for (int a = 0; a < c.n_agents; ++a) {
    p.mv_base[a] = a * c.width * c.height * 5;
    p.rm_base[a] = a * c.n_rm_states * c.n_events;
    p.final_q[a] = h->final_q[a];
    p.init_q[a] = h->init_q[a];
    p.start_x[a] = h->start_x[a];
    p.start_y[a] = h->start_y[a];
  }
  p.hazard_penalty = c.hazard_penalty;
  p.wall_penalty = c.wall_penalty;
  p.has_shaping = c.has_shaping ? 1 : 0;
  p.gamma_is_one = (c.gamma == 1.0f) ? 1 : 0;
  p.tbl_mode = h->fast_tables;
  p.H = c.height;
  p.hazard_fail = c.hazard_fail ? 1 : 0;
  p.wall_fail = c.wall_fail ? 1 : 0;
  p.merged = reinterpret_cast<const uint4*>(h->d_merged);
  p.merged4 = h->merged4_bytes ? reinterpret_cast<const uint32_t*>(static_cast<unsigned char*>(h->d_merged) + h->merged4_off)
                               : nullptr;
  p.merged4_bytes = (int32_t)h->merged4_bytes;
  std::memcpy(p.mg_palb, h->mg_palb, sizeof(p.mg_palb));
  p.merged_bytes = (int32_t)h->merged_bytes;
  if (c.n_qrm_max > 0 && h->buf.qrm_s) {
    p.qrm_s = h->buf.qrm_s;
    p.qrm_sn = h->buf.qrm_sn;
    p.qrm_rq = h->buf.qrm_rq;
    p.qrm_done = h->buf.qrm_done;
    p.n_qrm_max = c.n_qrm_max;
    for (int a = 0; a < c.n_agents; ++a) {
      p.n_qrm[a] = h->n_qrm[a];
      p.enc_nq[a] = h->enc_nq[a];
      for (int j = 0; j < c.n_qrm_max && j < rmx::kFastMaxQrm; ++j) p.qrm_q[a][j] = h->fast_qrm_q[a][j];
    }
  }
  p.HW = c.width * c.height;
  for (int a = 0; a < c.n_agents; ++a) {
    p.mg_base[a] = h->mg_base[a];
    p.enc_nq[a] = h->enc_nq[a];  // QRM outputs and enc_state
  }
  p.disc = h->d_disc;
  p.pos_x = h->buf.pos_x;
  p.pos_y = h->buf.pos_y;
  p.rm_q = h->buf.rm_q;
  p.flags = h->buf.flags;
  p.ep_ret = h->buf.ep_ret;
  p.t = h->buf.t;
  p.reward = h->buf.reward;
  p.shaping = h->buf.shaping;
  p.env_done = h->buf.env_done;
  p.renv = h->buf.renv;
  p.enc_state = h->buf.enc_state;
  p.env_offset = c.env_offset;
  p.n_global = c.n_envs_global;
  p.wave_stats = h->fast_wave_stats;
  p.skip_same = h->fast_skip;
  p.block = h->fast_block;
  p.slab = h->d_slab;
  p.es_ret = h->es_ret;
  p.es_cnt = h->es_cnt;
  p.es_succ = h->es_succ;
  p.err = h->d_err;
  p.diag = h->diag;
  p.stamps = h->d_stamps;
  p.pk = h->seq.d_pk;  // (in the block rmx_step_seq compares: a window recorded before the buffer existed is recorded again)
  if (c.stochastic || c.random_starts) {  // slip and / or FrozenLake random starts on the fast path
    p.slip = (c.stochastic ? rmx::kRngSlip : 0) | (c.random_starts ? rmx::kRngStarts : 0) |
             (h->seed_fixed ? rmx::kRngFixedSeed : 0);
    p.n_free = h->n_free;
    p.free_cells = h->d_free;
    p.start_ws = h->d_start_ws;
    if (h->d_rsc) {
      p.rs_cells = reinterpret_cast<const uint32_t*>(h->d_rsc);
      p.rs_rng = reinterpret_cast<const uint64_t*>(h->d_rsc + rmx::start_cache_rng_off(c.n_agents, c.n_envs));
      p.rs_dirty = h->rs_dirty ? 1 : 0;
    }
    if (h->d_nx) {
      const size_t N = (size_t)c.n_envs;
      p.nx_rng = reinterpret_cast<uint64_t*>(h->d_nx);
      p.nx_idx = reinterpret_cast<int32_t*>(h->d_nx + 32 * N);
      p.nx_ep = reinterpret_cast<int32_t*>(h->d_nx + 36 * N);
      p.rs_jump = reinterpret_cast<const uint4*>(h->d_nx + nx_jump_offset(c.n_envs));
    }
    rmx::slip_fill(p, c);
    p.seed_scale = c.seed_scale;
    p.seed_env_stride = c.seed_env_stride;
    p.seed_episode_stride = c.seed_episode_stride;
    p.base_seed = h->base_seed;
    p.rng = h->buf.rng;
    p.episode = h->buf.episode;
  }
  return p;
}

// The fast kernels run unless QRM outputs are bound with more experiences per agent than they emit.
// With QRM outputs they run thread-per-env with the global tables (the move word carries the event the
// counterfactual RM lookups need).
bool rmx::capi::fast_applies(const rmx_handle* h) {
  if (h->fast && (h->cfg.stochastic || h->cfg.random_starts)) {  // slip / random starts: the SLIP instantiations only
    const int tm = h->fast_tables;
    return !h->buf.qrm_s && h->fast_skip == rmx::kSkipRare && (tm == rmx::kTblMerged4 || tm == rmx::kTblMerged) &&
           h->cfg.n_envs < ((int64_t)1 << 27) &&
           // the next-episode precompute's one-byte rows (the fixed-start cache has no rows)
           (!h->cfg.random_starts || h->seed_fixed || h->n_free + 8 <= rmx::kRsRowMax);
  }
  const int qmax = h->cfg.n_agents <= 2 ? rmx::kFastMaxQrm : 8;  // register budget of the QRM lookups
  // QRM columns are [A][Qx][N]: their byte offsets must stay 32-bit as well
  return h->fast && (!h->buf.qrm_s || (h->cfg.n_qrm_max <= qmax &&
                                       (int64_t)h->cfg.n_qrm_max * h->cfg.n_agents * h->cfg.n_envs < ((int64_t)1 << 30)));
}

hipError_t rmx::capi::reduce_stats(const rmx_handle* h, double* out, hipStream_t st) {
  double* partial = h->d_slab + (size_t)RMX_NSTATS * h->n_waves;
  unsigned int* ticket = reinterpret_cast<unsigned int*>(partial + (size_t)RMX_NSTATS * 2 * rmx::kStatsPartials);
  return rmx::launch_stats_reduce(h->d_slab, h->n_waves, h->es_ret, h->es_cnt, h->es_succ, h->cfg.n_envs, partial,
                                  ticket, out, st);
}

// random starts: the step kernel's next-episode shuffles belong to the old seed schedule / state: tag them invalid
// (the kernel restarts a precompute whose tag is not the expected episode)
static hipError_t invalidate_next_shuffles(const rmx_handle* h, hipStream_t st) {
  if (!h->d_nx) return hipSuccess;
  const size_t N = (size_t)h->cfg.n_envs;
  return hipMemsetAsync(h->d_nx + 36 * N, 0xFF, 4 * N, st);
}

// A new base seed on stream st: the fixed-start cache rebuilt (every env), the next-episode precompute tags invalidated.
hipError_t rmx::capi::refresh_starts(rmx_handle* h, hipStream_t st) {
  hipError_t e = hipSuccess;
  if (h->d_rsc) e = rmx::launch_reset(base_params(h), nullptr, 0, st);
  if (e == hipSuccess) e = invalidate_next_shuffles(h, st);
  if (e == hipSuccess) h->rs_stale = false;
  return e;
}

// Before a launch on st that reads the start cache / precompute: bring them up to date if the base seed moved
// without a launch on a caller stream (rmx_reset_sync).
int rmx::capi::starts_current(rmx_handle* h, void* stream) {
  if (h->rs_stale) HIP_TRY(refresh_starts(h, as_stream(stream)), "start cache refresh");
  return RMX_OK;
}

// The fast step's parameter block for one step (rmx_step / rmx_step_hashed)
rmx::FastParams rmx::capi::step_fp(const rmx_handle* h, const int32_t* actions, uint64_t seed, int64_t t_global,
                                   int autoreset) {
  rmx::FastParams fp = fast_params(h);
  // slip alone: the step kernel reseeds its resetting lanes (the same generator the cache holds) instead of
  // loading the cached one on every lane: 4.65 vs 4.93 us per step at config 2 (profiles/r04_ab_log.md slipcache);
  // the fused rollout loads it once and keeps it
  if (!h->cfg.random_starts) fp.slip &= ~rmx::kRngFixedSeed;
  fp.actions = actions;
  fp.seed = seed;
  fp.t_global = t_global;
  fp.autoreset = autoreset ? 1 : 0;
  if (fp.qrm_s) fp.tbl_mode = rmx::kTblGlobal;
  return fp;
}

int rmx::capi::do_step(rmx_handle* h, const int32_t* actions, int hashed, uint64_t seed, int64_t t_global, int autoreset,
                       void* stream) {
  int rc = check_bound(h);
  if (rc) return rc;
  if (!hashed && !actions) return fail(RMX_E_INVALID, "actions is NULL");
  if (h->host) {
    h->host->step(actions, autoreset, hashed != 0, seed, t_global);
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  if ((rc = starts_current(h, stream))) return rc;
  if (fast_applies(h)) {
    const rmx::FastParams fp = step_fp(h, actions, seed, t_global, autoreset);
    HIP_TRY(rmx::launch_step_fast(fp, hashed, h->cfg.kind, as_stream(stream)), "step launch");
    return RMX_OK;
  }
  rmx::KParams p = base_params(h);
  p.actions = actions;
  p.seed = seed;
  p.t_global = t_global;
  p.autoreset = autoreset ? 1 : 0;
  HIP_TRY(rmx::launch_step(p, hashed, h->cfg.kind, h->step_layout, grid_for(h, h->step_layout), dim3(h->block), h->tables_bytes, as_stream(stream)),
          "step launch");
  return RMX_OK;
}

// The fused report runs where the handle's step is the thread-per-env fast kernel with 64-thread blocks,
// per-env statistics slots, rm_q / ep_ret skip stores and global / merged tables (the default below 1M envs);
// anywhere else rmx_step_report is the step launch followed by the stats launch, with the same result.
bool rmx::capi::report_fuses(const rmx_handle* h) {
  const int64_t grid = (h->cfg.n_envs + 63) / 64;
  const int tm = h->fast_tables;
  return fast_applies(h) && !h->buf.qrm_s && !h->fast_wave_stats && h->fast_block == 64 &&
         h->fast_skip == rmx::kSkipRare && h->rpt_partial &&
         (tm == rmx::kTblMerged4 || tm == rmx::kTblMerged || tm == rmx::kTblGlobal) && h->n_waves <= 64 * grid;
}

// The fused report step's parameter block (report_fuses(h))
rmx::FastParams rmx::capi::report_fp(const rmx_handle* h, const int32_t* actions, int autoreset, double* stats_out) {
  rmx::FastParams fp = fast_params(h);
  fp.actions = actions;
  fp.autoreset = autoreset ? 1 : 0;
  const int64_t grid = (h->cfg.n_envs + 63) / 64;
  fp.rpt_out = stats_out;
  fp.rpt_partial = h->rpt_partial;
  fp.rpt_ticket = h->rpt_ticket;
  fp.rpt_cs = (int32_t)((h->n_waves + grid - 1) / grid);
  fp.rpt_n_slab = (int32_t)h->n_waves;
  return fp;
}

extern "C" {

int rmx_abi_version(void) { return RMX_ABI_VERSION; }

int rmx_device_count(int32_t* n) {
  if (!n) return fail(RMX_E_INVALID, "n is NULL");
  int c = 0;
  const hipError_t e = hipGetDeviceCount(&c);
  *n = e == hipSuccess ? c : 0;  // no driver / no device: 0 (a host handle still works)
  return RMX_OK;
}

const char* rmx_last_error(void) { return g_err.c_str(); }

void rmx_destroy(rmx_handle* h) {
  if (!h) return;
  if (h->host) {
    delete h->host;
    delete h;
    return;
  }
  (void)hipSetDevice(h->device);
  (void)sync_end(h);
  if (h->sync.mb) (void)hipHostFree(h->sync.mb);
  if (h->sync.done) (void)hipEventDestroy(h->sync.done);
  if (h->sync.dep) (void)hipEventDestroy(h->sync.dep);
  if (h->sync.stream) (void)hipStreamDestroy(h->sync.stream);
  (void)hipFree(h->d_tables);
  (void)hipFree(h->d_disc);
  (void)hipFree(h->d_slab);
  (void)hipFree(h->d_stats);
  (void)hipFree(h->d_err);
  (void)hipFree(h->d_fast);
  (void)hipFree(h->d_merged);
  (void)hipFree(h->d_es);
  (void)hipFree(h->d_stamps);
  (void)hipFree(h->d_free);
  (void)hipFree(h->d_start_ws);
  (void)hipFree(h->d_nx);
  (void)hipFree(h->d_rsc);
  (void)hipFree(h->seq.d_pk);
  (void)hipFree(h->learn.d_phi);
  (void)hipFree(h->learn.d_rmax);
  (void)hipFree(h->learn.d_qrmax);
  delete h;
}

int rmx_bind(rmx_handle* h, const rmx_buffers* b) {
  if (!h || !b) return fail(RMX_E_INVALID, "handle or buffers NULL");
  if (!b->pos_x || !b->pos_y || !b->rm_q || !b->flags || !b->ep_ret || !b->t || !b->reward)
    return fail(RMX_E_STATE, "a required state/output buffer is NULL");
  const bool any_qrm = b->qrm_s || b->qrm_sn || b->qrm_rq || b->qrm_done;
  const bool all_qrm = b->qrm_s && b->qrm_sn && b->qrm_rq && b->qrm_done;
  if (any_qrm && !all_qrm) return fail(RMX_E_STATE, "QRM outputs must be all bound or all NULL");
  if (all_qrm && h->cfg.n_qrm_max == 0) return fail(RMX_E_STATE, "QRM outputs bound but n_qrm_max == 0");
  if ((h->cfg.stochastic || h->cfg.random_starts) && (!b->rng || !b->episode))
    return fail(RMX_E_STATE, "stochastic mode / random starts need the rng and episode buffers");
  if (b->enc_state)
    for (int a = 0; a < h->cfg.n_agents; ++a)
      if (h->enc_nq[a] < 1) return fail(RMX_E_STATE, "enc_state bound but enc_nq not provided at rmx_create");
  if (h->host) {  // host columns
    h->host->bind(*b);
    h->buf = *b;
    h->bound = true;
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  if (h->sync.mb) {  // the mailbox's QRM sections follow the bound buffers: rebuilt at the next sync call
    (void)hipHostFree(h->sync.mb);
    h->sync.mb = nullptr;
  }
  h->buf = *b;
  h->bound = true;
  h->rs_dirty = true;  // the new rng columns hold whatever the caller put there
  return RMX_OK;
}

int rmx_reset(rmx_handle* h, const uint8_t* env_mask_dev, uint64_t seed, void* stream) {
  int rc = check_bound(h);
  if (rc) return rc;
  if (h->host) {
    h->host->reset(env_mask_dev, seed);
    h->base_seed = seed;
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  // every env's generator comes from the new seed after a full reset; after a masked one with a new seed the envs
  // outside the mask keep the old seed's until their next autoreset
  h->rs_dirty = env_mask_dev ? (h->rs_dirty || seed != h->base_seed) : false;
  h->base_seed = seed;  // the seed schedule's base (stochastic mode)
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  rmx::KParams p = base_params(h);
  // (with the fixed-start cache this launch also rebuilds it, for every env whatever the mask)
  HIP_TRY(rmx::launch_reset(p, env_mask_dev, 1, as_stream(stream)), "reset launch");
  HIP_TRY(invalidate_next_shuffles(h, as_stream(stream)), "reset precompute");
  h->rs_stale = false;
  return lambda_clear(h, env_mask_dev, stream);  // env.reset() clears every learner's traces (Q(lambda) bound)
}

int rmx_step(rmx_handle* h, const int32_t* actions_dev, int autoreset, void* stream) {
  return do_step(h, actions_dev, 0, 0, 0, autoreset, stream);
}

int rmx_step_report(rmx_handle* h, const int32_t* actions_dev, int autoreset, double* stats_out_dev, void* stream) {
  int rc = check_bound(h);
  if (rc) return rc;
  if (!actions_dev || !stats_out_dev) return fail(RMX_E_INVALID, "bad rmx_step_report arguments");
  if (h->host) {
    h->host->step(actions_dev, autoreset);
    std::memcpy(stats_out_dev, h->host->stats, sizeof(h->host->stats));
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  if (!report_fuses(h)) {
    if ((rc = do_step(h, actions_dev, 0, 0, 0, autoreset, stream))) return rc;
    HIP_TRY(reduce_stats(h, stats_out_dev, as_stream(stream)), "stats launch");
    return RMX_OK;
  }
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  const rmx::FastParams fp = report_fp(h, actions_dev, autoreset, stats_out_dev);
  HIP_TRY(rmx::launch_step_fast(fp, 0, h->cfg.kind, as_stream(stream)), "step launch");
  return RMX_OK;
}

int rmx_step_report_fused(const rmx_handle* h) { return h && h->bound && report_fuses(h) ? 1 : 0; }

int rmx_step_hashed(rmx_handle* h, uint64_t seed, int64_t t_global, int autoreset, void* stream) {
  if (t_global < 0) return fail(RMX_E_INVALID, "t_global < 0");
  return do_step(h, nullptr, 1, seed, t_global, autoreset, stream);
}

int rmx_fill_actions(rmx_handle* h, uint64_t seed, int64_t t0, int32_t T, int32_t* actions_dev, void* stream) {
  if (!h || !actions_dev || T < 0 || t0 < 0) return fail(RMX_E_INVALID, "bad rmx_fill_actions arguments");
  if (T == 0) return RMX_OK;
  if (h->host) {
    h->host->fill_actions(seed, t0, T, actions_dev);
    return RMX_OK;
  }
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  HIP_TRY(rmx::launch_fill_actions(seed, t0, T, h->cfg.n_envs_global, h->cfg.env_offset, h->cfg.n_envs,
                                   h->cfg.n_agents, actions_dev, as_stream(stream)),
          "fill_actions launch");
  return RMX_OK;
}

int rmx_rollout(rmx_handle* h, uint64_t seed, int64_t t0, int32_t T, float* trace, void* stream) {
  int rc = check_bound(h);
  if (rc) return rc;
  if (T < 0 || t0 < 0) return fail(RMX_E_INVALID, "bad rollout length");
  if (T == 0) return RMX_OK;
  if (h->host) {  // T autoreset steps with hashed actions; the trace [T][A][N] from each step's rewards
    const size_t AN = (size_t)h->cfg.n_agents * (size_t)h->cfg.n_envs;
    for (int32_t it = 0; it < T; ++it) h->host->step(nullptr, 1, true, seed, t0 + it, trace ? trace + (size_t)it * AN : nullptr);
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  if ((rc = starts_current(h, stream))) return rc;
  // the fast-path rollout (merged or global tables): deterministic dynamics, and FrozenLake slip where the step
  // runs the SLIP instantiation (merged tables; fast_params sets p.slip)
  if (h->fast && ((!h->cfg.stochastic && !h->cfg.random_starts) || fast_applies(h))) {
    rmx::FastParams fp = fast_params(h);
    fp.seed = seed;
    fp.t_global = t0;
    fp.autoreset = 1;
    // tables staged into LDS once per 256-thread workgroup (amortised over T steps), merged if present
    const bool merged = fp.tbl_mode == rmx::kTblMerged || fp.tbl_mode == rmx::kTblMerged4;
    // (random starts: the 256-thread workgroup's draw areas share the LDS with the staged table)
    const size_t rs_lds = h->cfg.random_starts ? 4 * (size_t)rmx::kRsWaveLds : 0;
    if (h->rollout_lds && (!merged || ((h->merged_bytes + 15) & ~(size_t)15) + rs_lds <= rmx::kRolloutLdsMax)) {
      fp.tbl_mode = merged ? rmx::kTblMergedLds : rmx::kTblLds;
      fp.block = 256;
    } else {
      fp.tbl_mode = merged ? rmx::kTblMerged : rmx::kTblGlobal;
    }
    HIP_TRY(rmx::launch_rollout_fast(fp, h->cfg.kind, T, trace, as_stream(stream)), "rollout launch");
    return RMX_OK;
  }
  rmx::KParams p = base_params(h);
  p.seed = seed;
  p.t_global = t0;
  p.autoreset = 1;
  HIP_TRY(rmx::launch_rollout(p, h->cfg.kind, h->rollout_layout, T, trace, grid_for(h, h->rollout_layout), dim3(h->block), h->tables_bytes,
                              as_stream(stream)),
          "rollout launch");
  return RMX_OK;
}

int rmx_mdp_states(rmx_handle* h, int32_t agent, int64_t* n_states) {
  if (!h || !n_states || agent < 0 || agent >= h->cfg.n_agents) return fail(RMX_E_INVALID, "bad rmx_mdp_states arguments");
  if (h->enc_nq[agent] < 1) return fail(RMX_E_INVALID, "enc_nq not provided at rmx_create");
  *n_states = (int64_t)h->cfg.width * h->cfg.height * h->enc_nq[agent];
  return RMX_OK;
}

int rmx_mdp(rmx_handle* h, int32_t agent, int32_t fix_frozen_lake, int32_t* next_dev, float* reward_dev,
            uint8_t* done_dev, void* stream) {
  int64_t S = 0;
  int rc = rmx_mdp_states(h, agent, &S);
  if (rc) return rc;
  if (!next_dev || !reward_dev || !done_dev) return fail(RMX_E_INVALID, "rmx_mdp output is NULL");
  if (h->host) {
    h->host->mdp(agent, fix_frozen_lake ? 1 : 0, next_dev, reward_dev, done_dev);
    return RMX_OK;
  }
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  rmx::KParams p = base_params(h);
  HIP_TRY(rmx::launch_mdp(p, h->cfg.kind, agent, fix_frozen_lake ? 1 : 0, S, next_dev, reward_dev, done_dev,
                          h->tables_bytes, as_stream(stream)),
          "mdp launch");
  return RMX_OK;
}

int rmx_stats_device(rmx_handle* h, double* out_dev, void* stream) {
  if (!h || !out_dev) return fail(RMX_E_INVALID, "bad rmx_stats_device arguments");
  if (h->host) {  // a host handle's "device" memory is host memory
    std::memcpy(out_dev, h->host->stats, sizeof(h->host->stats));
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  HIP_TRY(reduce_stats(h, out_dev, as_stream(stream)), "stats launch");
  return RMX_OK;
}

int rmx_stats_host(rmx_handle* h, double* out_host) {
  if (!h || !out_host) return fail(RMX_E_INVALID, "bad rmx_stats_host arguments");
  if (h->host) {
    std::memcpy(out_host, h->host->stats, sizeof(h->host->stats));
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  HIP_TRY(hipDeviceSynchronize(), "sync before stats");
  HIP_TRY(reduce_stats(h, h->d_stats, nullptr), "stats launch");
  HIP_TRY(hipMemcpy(out_host, h->d_stats, sizeof(double) * RMX_NSTATS, hipMemcpyDeviceToHost), "stats copy");
  return RMX_OK;
}

int rmx_stats_clear(rmx_handle* h, void* stream) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (h->host) {
    std::memset(h->host->stats, 0, sizeof(h->host->stats));
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  HIP_TRY(hipMemsetAsync(h->d_slab, 0, sizeof(double) * RMX_NSTATS * h->n_waves, as_stream(stream)), "stats clear");
  if (h->d_es) HIP_TRY(hipMemsetAsync(h->d_es, 0, h->es_bytes, as_stream(stream)), "stats clear");
  return RMX_OK;
}

#ifdef RMX_DIAG
// Diagnostic builds only (not part of include/rmx.h): copy the per-wave stamps of the last fast-kernel
// launch ([wave][2 * kStamps] u64: shader clocks, then real-time clocks) to the host.
int rmx_diag_stamps(rmx_handle* h, unsigned long long* out, int64_t max_words) {
  if (!h || !h->d_stamps) return fail(RMX_E_STATE, "no stamp buffer (set RMX_DIAG_STAMPS at rmx_create)");
  const int64_t n = (h->cfg.n_envs + 255) / 256 * 4 * 2 * rmx::kStamps;
  HIP_TRY(hipDeviceSynchronize(), "sync");
  HIP_TRY(hipMemcpy(out, h->d_stamps, 8 * std::min(n, max_words), hipMemcpyDeviceToHost), "stamps copy");
  return (int)std::min(n, max_words);
}
#endif

int rmx_step_variant(const rmx_handle* h) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (h->host) return RMX_VARIANT_HOST;
  if (fast_applies(h)) return RMX_VARIANT_FAST;
  return h->step_layout == rmx::kLayoutLanePerAgent ? RMX_VARIANT_LANE_PER_AGENT : RMX_VARIANT_GENERIC;
}

int rmx_step_info(const rmx_handle* h, int64_t* out, int32_t n) {
  if (!h || !out || n < 0) return fail(RMX_E_INVALID, "bad rmx_step_info arguments");
  int64_t v[RMX_STEP_INFO_N] = {};
  v[0] = rmx_step_variant(h);
  if (!h->host) {
    const bool fast = fast_applies(h);
    const bool qrm = fast && h->buf.qrm_s && h->cfg.n_qrm_max > 0;
    const int tm = !fast ? 0 : qrm ? rmx::kTblGlobal : h->fast_tables;  // step_fp: QRM outputs read the global blob
    v[1] = tm == rmx::kTblGlobal ? RMX_TABLES_GLOBAL : tm == rmx::kTblMerged ? RMX_TABLES_MERGED
         : tm == rmx::kTblMerged4 ? RMX_TABLES_MERGED4 : RMX_TABLES_NONE;
    v[2] = tm == rmx::kTblMerged ? 16 : tm == rmx::kTblMerged4 ? 4 : 0;
    v[3] = h->merged_sections;
    v[4] = h->merged_sections ? (int64_t)h->merged_bytes : 0;  // (a table that outgrew kMergedMaxBytes is not used)
    v[5] = (int64_t)h->merged4_bytes;
    v[6] = h->fast ? (int64_t)h->fast_n16 * 16 : 0;
    v[7] = (int64_t)h->tables_bytes;
    v[8] = fast ? h->fast_skip : h->generic_skip;
    v[9] = fast ? h->fast_wave_stats : 1;
    v[10] = fast ? h->fast_block : h->block;
    v[11] = qrm ? 1 : 0;
    v[12] = h->seed_fixed ? 1 : 0;
    v[13] = h->rollout_layout;
  }
  for (int32_t i = 0; i < n && i < RMX_STEP_INFO_N; ++i) out[i] = v[i];
  return RMX_OK;
}

static const char kTraceFullMsg[] =
    "a Q(lambda) trace found its list full (rmx_learn_lambda_bind cap): the cell was updated, its trace not kept";

static const char kModelFullMsg[] =
    "an R-max successor found its list full (rmx_learn_rmax_bind cap): the observation was counted, its list entry "
    "dropped";

int rmx_check_errors(rmx_handle* h) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (h->host) {
    const uint32_t err = h->host->err;
    h->host->err = 0;
    if (err & 1u) return fail(RMX_E_ACTION, "an action outside [0,4] was stepped (treated as wait)");
    if (err & rmx::kErrTraceFull) return fail(RMX_E_TRACE, kTraceFullMsg);
    if (err & rmx::kErrModelFull) return fail(RMX_E_MODEL, kModelFullMsg);
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  HIP_TRY(hipDeviceSynchronize(), "sync");
  uint32_t err = 0;
  HIP_TRY(hipMemcpy(&err, h->d_err, sizeof(err), hipMemcpyDeviceToHost), "err copy");
  HIP_TRY(hipMemset(h->d_err, 0, sizeof(uint32_t)), "err clear");
  if (err & 1u) return fail(RMX_E_ACTION, "an action outside [0,4] was stepped (treated as wait)");
  if (err & rmx::kErrTraceFull) return fail(RMX_E_TRACE, kTraceFullMsg);
  if (err & rmx::kErrModelFull) return fail(RMX_E_MODEL, kModelFullMsg);
  return RMX_OK;
}

}  // extern "C"
