// rmx_capi_create.cpp — rmx_create: validation, host handles, and a device handle in three steps (the environment's
// switches, the host-only launch plan, the device allocations and uploads).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "rmx_handle.h"

using namespace rmx::capi;

namespace {

int validate(const rmx_config* c) {
  if (!c) return fail(RMX_E_INVALID, "config is NULL");
  const std::string msg = rmx::validate_config(*c);
  return msg.empty() ? RMX_OK : fail(RMX_E_INVALID, msg);
}

// ---- host handles (cfg.device == RMX_DEVICE_HOST, rmx_hoststep.cpp) ------------------------------------------
int create_host(const rmx_config* cfg, rmx_handle** out) {
  rmx_handle* h = new rmx_handle();
  h->host = new rmx::HostEngine();
  const std::string msg = h->host->init(*cfg);
  if (!msg.empty()) {
    delete h->host;
    delete h;
    return fail(RMX_E_INVALID, msg);
  }
  h->cfg = h->host->cfg;  // scalars only
  h->device = RMX_DEVICE_HOST;
  h->digest = rmx::config_digest(*cfg);
  for (int a = 0; a < cfg->n_agents; ++a) h->enc_nq[a] = h->host->p.enc_nq[a];
  *out = h;
  return RMX_OK;
}

// Random starts, the wave-cooperative finish (rmx_fast.hip rs_coop_finish): output j of a PCG64 generator in one
// jump, state_j = M^j state + (1 + M + ... + M^(j-1)) inc (mod 2^128), for j = 1..64: M^j then the sum, each as
// 4 x u32 (low word first).  Placed after the precompute columns in the handle's d_nx allocation (nx_jump_offset).
struct RsJumpTable {
  uint32_t w[64][2][4];
  RsJumpTable() {
    typedef unsigned __int128 u128;
    const u128 M = ((u128)0x2360ED051FC65DA4ull << 64) | 0x4385DF649FCCF645ull;
    u128 mj = 1, sj = 0;
    for (int j = 0; j < 64; ++j) {
      sj += mj;  // 1 + M + ... + M^j
      mj *= M;   // M^(j+1)
      const u128 v[2] = {mj, sj};
      for (int k = 0; k < 2; ++k)
        for (int q = 0; q < 4; ++q) w[j][k][q] = (uint32_t)(v[k] >> (32 * q));
    }
  }
};
const RsJumpTable rs_jump_table;

}  // namespace

extern "C" {

// ---- rmx_create of a device handle, in three steps: the environment's switches, the host-only launch plan (with
// the test overrides of its defaults beside them), the device allocations and uploads --------------------------
// what the plan builds on the host for the upload step
struct CreateTables {
  std::vector<unsigned char> blob, fast_blob;
  std::vector<uint32_t> merged_tab;
  std::vector<float> disc;
  std::vector<uint16_t> free_cells;
};

// Step 1: the switches the environment sets for the whole handle
static void create_env(rmx_handle* h, const rmx_config* cfg) {
  if (const char* qv = std::getenv("RMX_QUEUE")) h->seq.queue_off = std::strcmp(qv, "0") == 0;
  if (const char* pv = std::getenv("RMX_SEQ_PACKED")) h->seq.packed_off = std::strcmp(pv, "0") == 0;
  if (const char* rv = std::getenv("RMX_SEQ_RELEASE")) h->seq.release_all = std::strcmp(rv, "1") == 0;
  if (const char* b = std::getenv("RMX_BLOCK")) {
    int v = std::atoi(b);
    if (v == 64 || v == 128 || v == 256) h->block = v;
  }
#ifdef RMX_DIAG
  if (const char* d = std::getenv("RMX_DIAG_BITS")) h->diag = std::atoi(d);
#endif
  // per-env rng (slip, random starts): one env rng, agents draw in order -> thread-per-env kernels only
  const bool rng_on = cfg->stochastic || cfg->random_starts;
  if (rng_on) h->rollout_layout = rmx::kLayoutThreadPerEnv;
  if (const char* l = std::getenv("RMX_LAYOUT")) {  // test / tuning override for both kernels
    if (!std::strcmp(l, "tpe")) h->step_layout = h->rollout_layout = rmx::kLayoutThreadPerEnv;
    if (!std::strcmp(l, "lpe") && !rng_on) h->step_layout = h->rollout_layout = rmx::kLayoutLanePerAgent;
  }
}

// Step 2: the launch plan (table mode, store mode, block size, stats mode) and the tables it needs, on the host
// alone; false when the generic kernels' tables do not fit
static bool create_plan(rmx_handle* h, const rmx_config* cfg, CreateTables& tb) {
  const int A = cfg->n_agents;
  for (int a = 0; a < A; ++a) {
    h->init_q[a] = cfg->init_q[a];
    h->final_q[a] = cfg->final_q[a];
    h->start_x[a] = cfg->start_xy[2 * a];
    h->start_y[a] = cfg->start_xy[2 * a + 1];
  }
  // table blob of the generic kernels (rmx_tables.cpp)
  rmx::BlobOffsets bo;
  if (!rmx::build_table_blob(*cfg, tb.blob, bo)) return false;
  h->tables_bytes = tb.blob.size();
  h->digest = rmx::config_digest(*cfg);
  h->off_cell = bo.cell;
  h->off_ev = bo.ev;
  h->off_nq = bo.nq;
  h->off_rr = bo.rr;
  h->off_sh = bo.sh;
  h->off_qrm = bo.qrm;
  if (cfg->n_qrm_max > 0) {
    for (int a = 0; a < A; ++a) {
      h->n_qrm[a] = cfg->n_qrm[a];
      for (int j = 0; j < cfg->n_qrm_max && j < rmx::kFastMaxQrm; ++j)
        h->fast_qrm_q[a][j] = cfg->qrm_states[a * cfg->n_qrm_max + j];
    }
  }
  for (int a = 0; a < A; ++a) h->enc_nq[a] = cfg->enc_nq ? cfg->enc_nq[a] : 0;
  tb.disc = rmx::discount_table(*cfg);
  // FrozenLake random starts: the non-hole cells (x-major) and a per-env shuffle workspace
  if (cfg->random_starts) tb.free_cells = rmx::free_cells(*cfg);
  h->n_free = (int32_t)tb.free_cells.size();
  // one slab slot per wave of the larger of the two launch geometries
  const int64_t gmax = std::max(grid_for(h, h->step_layout).x, grid_for(h, h->rollout_layout).x);
  std::vector<unsigned char>& fast_blob = tb.fast_blob;
  std::vector<uint32_t>& merged_tab = tb.merged_tab;
  {
    // RMX_FAST=0: generic kernels only (tests / A-B timing)
    const char* fe = std::getenv("RMX_FAST");
    // RMX_FAST=0: generic only; default: the fast path wherever it applies
    const bool want = fe ? std::strcmp(fe, "0") != 0 : true;
    rmx::FastLayout fl;
    h->fast = want && h->step_layout == rmx::kLayoutThreadPerEnv && rmx::build_fast_blob(*cfg, fast_blob, fl);
    h->fast_off_rm = fl.off_rm;
    h->fast_off_info = fl.off_info;
    h->fast_n16 = (int32_t)(fast_blob.size() / 16);
    // Default table mode, measured at 65,536 envs (profiles/r01_ab_log.md c25, c26): the merged single
    // lookup while its table is small (<= 64 KiB: config 2 3.06 vs 3.10-3.15 us global, config 3 2.50-2.54
    // vs 2.75-2.78 global and 2.55-2.60 lane-resident), the global blob for larger tables (config 4 equal,
    // config 5 3.67 global vs 3.81-3.87 merged).
    // The size that decides is the deduplicated one (identical agent sections stored once).
    if (h->fast) {
      std::vector<uint32_t> probe;
      const bool ok = rmx::build_merged(*cfg, fast_blob, h->fast_off_rm, h->mg_base, probe);
      h->fast_tables = ok && probe.size() * 4 <= kFastMergedDefaultBytes ? rmx::kTblMerged : rmx::kTblGlobal;
      // 4-B records (reward from a <= 4-entry palette, no shaping): config 2 3.28-3.30 vs 3.36-3.37 us on one
      // box, equal on another; config 3 2.51-2.52 vs 2.68-2.71; config 4 4.18-4.22 vs 4.25-4.28 (r01_ab_log
      // c75, c77; 8-B {word 0, reward} records gain less).  Falls back to the 16-B records below when the
      // config is not eligible.
      // FrozenLake slip keeps the 16-B records: config 2 with slip 4.62-4.64 vs 4.78-4.84 us with 4-B records,
      // config 4 equal (r02_ab_log slipint, r02aq)
      if (h->fast_tables == rmx::kTblMerged && !cfg->stochastic) h->fast_tables = rmx::kTblMerged4;
    }
    // test override of the default (the results do not depend on it): RMX_FAST_TABLES=global|merged|merged4
    if (const char* ft = std::getenv("RMX_FAST_TABLES")) {
      if (!std::strcmp(ft, "global")) h->fast_tables = rmx::kTblGlobal;
      if (!std::strcmp(ft, "merged")) h->fast_tables = rmx::kTblMerged;
      if (!std::strcmp(ft, "merged4")) h->fast_tables = rmx::kTblMerged4;
    }
    const bool want_m4 = h->fast_tables == rmx::kTblMerged4;
    if (h->fast && (h->fast_tables == rmx::kTblMerged || want_m4) &&
        !rmx::build_merged(*cfg, fast_blob, h->fast_off_rm, h->mg_base, merged_tab))
      h->fast_tables = rmx::kTblGlobal;  // table too large: one lookup per stage
    if (want_m4 && h->fast_tables != rmx::kTblGlobal) {  // the compact records follow the 16-B ones
      std::vector<uint32_t> compact;
      // the step kernel reads the palette as signed bytes: integer rewards in [-128, 127] (every BASELINE config's);
      // other palettes take the 16-B records
      if (rmx::build_compact(*cfg, h->mg_base, merged_tab, h->mg_palb, compact)) {
        h->merged4_off = merged_tab.size() * 4;
        h->merged4_bytes = compact.size() * 4;
        merged_tab.insert(merged_tab.end(), compact.begin(), compact.end());
        while (merged_tab.size() % 4) merged_tab.push_back(0u);
      } else {
        h->fast_tables = rmx::kTblMerged;  // shaping or > 4 distinct rewards: the 16-B records
      }
    }
    if (h->fast && h->fast_tables != rmx::kTblGlobal) {
      const size_t sec_words = (size_t)cfg->n_rm_states * cfg->width * cfg->height * 5 * 4;
      const size_t words16 = h->merged4_bytes ? h->merged4_off / 4 : merged_tab.size();
      h->merged_sections = (int)(words16 / sec_words);
    }
    // the 16-B records' bytes (the compact records, if any, follow them in d_merged)
    if (!merged_tab.empty()) h->merged_bytes = h->merged4_bytes ? h->merged4_off : merged_tab.size() * 4;
  }
  // slip / random starts under seed_episode_stride == 0 (the reference FrozenLake runner's reset(args.seed) every
  // episode, frozen_lake_main.py:337): every episode of an env starts from the same generator and shuffle, so the
  // fast kernels copy a cached one at each autoreset instead of reseeding and redrawing (h->fast: A <= 4, cells fit
  // the cache's 8-bit x / y)
  h->seed_fixed = h->fast && (cfg->stochastic || cfg->random_starts) && cfg->seed_episode_stride == 0;
  // one slab slot per wave of the largest launch geometry (the fast kernels use 256-thread blocks)
  h->n_waves = std::max<int64_t>(gmax * (h->block / 64), (cfg->n_envs + 255) / 256 * 4);
  h->fast_wave_stats = cfg->n_envs >= kFastWaveStatsMinEnvs ? 1 : 0;
  if (const char* fs = std::getenv("RMX_FAST_STATS")) h->fast_wave_stats = !std::strcmp(fs, "wave") ? 1 : 0;
  // fast kernel: rm_q / ep_ret stores skipped when unchanged at every size (65,536 envs: 3-5 % faster than
  // storing every word; 8.4M envs: 10-17 % faster than skipping every unchanged word, whose partial-line writes
  // of the x / y / flags columns cost more than they save; profiles/r02_ab_log.md ab3, ab4, abbig).  The generic
  // kernel (slip, random starts, A > 4) skips every unchanged word from 1M envs on (round 1, c55).
  // Once a step's columns outgrow the 256 MB Infinity Cache (>= 2^23 env x agent instances, ~440 MB per step) the
  // same stores carry the non-temporal hint (kSkipRareNT): 8.4M envs 6-24 % faster on all four configs, while at
  // 1-2M envs it is mixed (configs 3 and 5 slower) and at 65,536 envs 7-8 % slower (profiles/r02_ab_log.md pol, nt).
  h->fast_skip = cfg->n_envs * (int64_t)cfg->n_agents >= kFastNtMinInstances ? rmx::kSkipRareNT : rmx::kSkipRare;
  h->generic_skip = cfg->n_envs >= kFastSkipMinEnvs ? 1 : 0;
  // test override: RMX_FAST_SKIP=3 puts the bandwidth regime's non-temporal store mode under test at smaller sizes,
  // 2 the default store mode at larger ones (the other store modes lost their A/Bs and were removed, round 5)
  if (const char* fk = std::getenv("RMX_FAST_SKIP")) {
    const int v = std::atoi(fk);
    if (v == rmx::kSkipRare || v == rmx::kSkipRareNT) h->fast_skip = v;
  }
  // test override of the generic kernel's store mode (every unchanged word skipped: its default from 1M envs)
  if (const char* gk = std::getenv("RMX_GENERIC_SKIP")) h->generic_skip = std::atoi(gk) ? 1 : 0;
  // 64-thread workgroups at the headline size (1-3 % faster on all four configs, r01_ab_log c48), 256 in the
  // bandwidth regime (64: 15-20 % slower at 8.4M envs, c49)
  h->fast_block = cfg->n_envs >= kFastSkipMinEnvs ? 256 : 64;
  if (const char* rl = std::getenv("RMX_ROLLOUT_LDS")) h->rollout_lds = std::atoi(rl) ? 1 : 0;
  return true;
}

// Step 3: the device allocations and uploads, in an order that does not change (device addresses follow from it)
static hipError_t create_upload(rmx_handle* h, const rmx_config* cfg, const CreateTables& tb) {
  hipError_t e = hipSuccess;
  // allocate, then set every byte to fill (fill >= 0), then copy src_bytes from src (src != NULL); after a failure
  // the calls that follow do nothing
  auto put = [&e](auto** p, size_t bytes, int fill, const void* src = nullptr, size_t src_bytes = 0) {
    if (e == hipSuccess) e = hipMalloc(p, bytes);
    if (e == hipSuccess && fill >= 0) e = hipMemset(*p, fill, bytes);
    if (e == hipSuccess && src) e = hipMemcpy(*p, src, src_bytes, hipMemcpyHostToDevice);
  };
  const size_t N = (size_t)cfg->n_envs;
#ifdef RMX_DIAG
  if (std::getenv("RMX_DIAG_STAMPS")) put(&h->d_stamps, (N + 255) / 256 * 4 * 2 * rmx::kStamps * 8, 0);
#endif
  if (h->fast && !h->fast_wave_stats) {  // per-env slots only in the per-env stats mode (wave mode: the slab)
    // one row [N] each: both fast layouts sum an env's agents before its one adder
    const size_t o_cnt = 8 * N, o_succ = o_cnt + 8 * N, o_part = (o_succ + 4 * N + 15) & ~size_t(15);
    const size_t o_ticket = (o_part + sizeof(double) * RMX_NSTATS * ((N + 63) / 64) + 127) & ~size_t(127);
    h->es_bytes = o_ticket + 128 * (1 + 32);  // root + 32 shard counters, one 128-B line each (rmx_fast.hip)
    put(&h->d_es, h->es_bytes, 0);
    if (e == hipSuccess) {
      h->es_ret = reinterpret_cast<double*>(h->d_es);
      h->es_cnt = reinterpret_cast<unsigned long long*>(h->d_es + o_cnt);
      h->es_succ = reinterpret_cast<uint32_t*>(h->d_es + o_succ);
      h->rpt_partial = reinterpret_cast<double*>(h->d_es + o_part);
      h->rpt_ticket = reinterpret_cast<unsigned int*>(h->d_es + o_ticket);
    }
  }
  put(&h->d_tables, h->tables_bytes, -1, tb.blob.data(), h->tables_bytes);
  put(&h->d_disc, sizeof(float) * tb.disc.size(), -1, tb.disc.data(), sizeof(float) * tb.disc.size());
  // slab | 2 * kStatsPartials partial vectors | the stats launch's ticket (zeroed, re-armed by every report)
  put(&h->d_slab, sizeof(double) * (RMX_NSTATS * (h->n_waves + 2 * rmx::kStatsPartials) + 2), 0);
  put(&h->d_stats, sizeof(double) * RMX_NSTATS, -1);
  put(&h->d_err, sizeof(uint32_t), 0);
  if (h->n_free > 0) {
    // (padded to whole dwords: the fast path stages the cells as u16 pairs)
    put(&h->d_free, sizeof(uint16_t) * (tb.free_cells.size() + 1), 0, tb.free_cells.data(),
        sizeof(uint16_t) * tb.free_cells.size());
    put(&h->d_start_ws, sizeof(uint16_t) * (size_t)rmx::shuffle_stride((int32_t)tb.free_cells.size()) * N, -1);
    if (!h->seed_fixed) {  // the next-episode precompute (its tags invalid until a step restarts it)
      put(&h->d_nx, nx_jump_offset(cfg->n_envs) + sizeof(rs_jump_table.w), -1);
      if (e == hipSuccess) e = hipMemset(h->d_nx + 36 * N, 0xFF, 4 * N);
      if (e == hipSuccess)
        e = hipMemcpy(h->d_nx + nx_jump_offset(cfg->n_envs), rs_jump_table.w, sizeof(rs_jump_table.w), hipMemcpyHostToDevice);
    }
  }
  // the reset cache (cells 0 = in range until the first reset fills it)
  if (h->seed_fixed) put(&h->d_rsc, rmx::start_cache_bytes(cfg->n_agents, cfg->n_envs), 0);
  if (h->fast) put(&h->d_fast, tb.fast_blob.size(), -1, tb.fast_blob.data(), tb.fast_blob.size());
  if (!tb.merged_tab.empty())
    put(&h->d_merged, tb.merged_tab.size() * 4, -1, tb.merged_tab.data(), tb.merged_tab.size() * 4);
  return e;
}

int rmx_create(const rmx_config* cfg, rmx_handle** out) {
  if (!out) return fail(RMX_E_INVALID, "out is NULL");
  *out = nullptr;
  int rc = validate(cfg);
  if (rc) return rc;
  if (cfg->device == RMX_DEVICE_HOST) {
    try {
      return create_host(cfg, out);
    } catch (const std::exception& e) {  // allocation: nothing may unwind through the C ABI
      return fail(RMX_E_INVALID, std::string("rmx_create (host): ") + e.what());
    }
  }
  if (cfg->device < 0) return fail(RMX_E_INVALID, "device must be a HIP device ordinal or RMX_DEVICE_HOST");
  HIP_TRY(hipSetDevice(cfg->device), "hipSetDevice");
  rmx_handle* h = new rmx_handle();
  h->cfg = *cfg;
  h->device = cfg->device;
  create_env(h, cfg);
  CreateTables tb;
  if (!create_plan(h, cfg, tb)) {
    delete h;
    return fail(RMX_E_INVALID, "tables exceed 64 KiB of LDS");
  }
  const hipError_t e = create_upload(h, cfg, tb);
  if (e != hipSuccess) {
    rmx_destroy(h);
    return hip_fail(e, "rmx_create allocation/upload");
  }
  h->cfg.cell = nullptr;
  h->cfg.cell_event = nullptr;
  h->cfg.next_q = nullptr;
  h->cfg.rm_reward = nullptr;
  h->cfg.shape = nullptr;
  h->cfg.init_q = h->cfg.final_q = h->cfg.start_xy = nullptr;
  h->cfg.n_qrm = h->cfg.enc_nq = nullptr;
  h->cfg.qrm_states = nullptr;
  *out = h;
  return RMX_OK;
}

}  // extern "C"
