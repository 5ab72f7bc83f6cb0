// rmx_capi_learn.cpp — the tabular Q-learning / QRM learner fused into the step (rmx_learn.h, rmx_learn.hip): the
// rmx_learn_* entry points, the Q(lambda) binding with its trace lists and the epsilon schedule included.  Owns
// rmx_handle::learn.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <exception>
#include <vector>

#include "rmx_handle.h"

using namespace rmx::capi;

static int do_learn_step(rmx_handle* h, const int32_t* actions, rmx::LearnCall lc, uint64_t seed, int64_t t_global,
                         int autoreset, void* stream) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (!h->bound) return fail(RMX_E_STATE, "buffers not bound (rmx_bind)");
  if (!(h->host ? h->host->learn_on : h->learn.on)) return fail(RMX_E_STATE, "no learner bound (rmx_learn_bind)");
  if (!lc.policy && !actions) return fail(RMX_E_INVALID, "actions is NULL");
  if (lc.policy == rmx::kLearnNumpy) {
    lc.rng = h->host ? h->host->learn_rng : h->learn.rng;
    if (!lc.rng) return fail(RMX_E_STATE, "RMX_LEARN_NUMPY needs a generator column (rmx_learn_rng_bind)");
  }
  if (h->host) {  // (a full trace list: HostEngine::err, as the device's error word)
    h->host->step(actions, autoreset, false, seed, t_global, nullptr, &lc);
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  rmx::KParams p = base_params(h);
  p.actions = actions;
  p.seed = seed;
  p.t_global = t_global;
  p.autoreset = autoreset ? 1 : 0;
  if (h->learn.qrmax_on) {  // QR-max: likewise, over the learners with something newly known
    HIP_TRY(rmx::launch_learn_qrmax(p, h->learn.params, lc, h->learn.qrmax, h->learn.qwork, h->learn.qrmax_grid,
                                    h->cfg.kind, h->tables_bytes, as_stream(stream)),
            "QR-max learn step launch");
    if (lc.update) h->learn.qwork.parity ^= 1;  // (the solve kernel has zeroed the other list's length)
    return RMX_OK;
  }
  if (h->learn.rmax_on) {  // R-max: the step kernel, then with an update the solve kernel over the step's worklist
    HIP_TRY(rmx::launch_learn_rmax(p, h->learn.params, lc, h->learn.rmax, h->learn.work, h->learn.rmax_grid, h->cfg.kind,
                                   h->tables_bytes, as_stream(stream)),
            "R-max learn step launch");
    if (lc.update) h->learn.work.parity ^= 1;  // (the solve kernel has zeroed the other list's length)
    return RMX_OK;
  }
  // slip / random starts (a learner bound with RMX_LEARN_DYN_ENV): the kernel reads and writes the env generator and
  // episode columns rmx_bind required, and none of the fast path's caches (the reset cache, the next-episode shuffles)
  HIP_TRY(rmx::launch_learn_step(p, h->learn.params, lc, h->learn.lam_on ? &h->learn.lam : nullptr,
                                 h->learn.eps.col ? &h->learn.eps : nullptr, h->cfg.kind, h->tables_bytes,
                                 as_stream(stream)),
          "learn step launch");
  return RMX_OK;
}

int rmx::capi::lambda_clear(rmx_handle* h, const uint8_t* env_mask_dev, void* stream) {
  if (!h->learn.lam_on) return RMX_OK;
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  HIP_TRY(rmx::launch_traces_clear(h->learn.lam.cnt, env_mask_dev, h->cfg.n_agents, h->cfg.n_envs, as_stream(stream)),
          "trace clear launch");
  return RMX_OK;
}

extern "C" {

int rmx_learn_states(const rmx_handle* h, int64_t* s_max) {
  if (!h || !s_max) return fail(RMX_E_INVALID, "handle or s_max is NULL");
  int32_t m = 0;
  for (int a = 0; a < h->cfg.n_agents; ++a) {
    if (h->enc_nq[a] < 1) return fail(RMX_E_INVALID, "the learner needs enc_nq (the state encoder strides) at rmx_create");
    m = std::max(m, h->enc_nq[a]);
  }
  *s_max = (int64_t)h->cfg.width * h->cfg.height * m;
  return RMX_OK;
}

int rmx_learn_bind(rmx_handle* h, const rmx_learn_config* lc, double* q, double* visits) {
  if (!h || !lc) return fail(RMX_E_INVALID, "handle or learn config is NULL");
  if (!q) return fail(RMX_E_INVALID, "the q table is NULL");
  if (!std::isfinite(lc->gamma) || lc->gamma < 0.0) return fail(RMX_E_INVALID, "gamma must be finite and >= 0");
  if (!std::isfinite(lc->learning_rate) || lc->learning_rate < 0.0)
    return fail(RMX_E_INVALID, "learning_rate must be finite and >= 0 (0: 1 / visits)");
  int64_t s_max = 0;
  int rc = rmx_learn_states(h, &s_max);
  if (rc) return rc;
  if (lc->use_qrm && h->cfg.n_qrm_max == 0) return fail(RMX_E_INVALID, "use_qrm needs the QRM state lists (n_qrm_max == 0)");
  if (lc->use_rsh && !lc->use_qrm)
    return fail(RMX_E_INVALID, "use_rsh without use_qrm is not supported (the reference's non-QRM shaping reads a "
                               "label-keyed dict by index)");
  if (lc->use_rsh && !lc->phi) return fail(RMX_E_INVALID, "use_rsh needs phi (the RM potentials by RM index)");
  if (lc->learning_rate == 0.0 && !visits) return fail(RMX_E_INVALID, "the 1 / visits learning rate needs a visits table");
  if (lc->dynamics != RMX_LEARN_DYN_FIXED && lc->dynamics != RMX_LEARN_DYN_ENV)
    return fail(RMX_E_INVALID, "dynamics must be RMX_LEARN_DYN_FIXED or RMX_LEARN_DYN_ENV");
  if (lc->dynamics == RMX_LEARN_DYN_FIXED && (h->cfg.stochastic || h->cfg.random_starts))
    return fail(RMX_E_INVALID, "the learn step serves deterministic dynamics and fixed starts (cfg.stochastic / "
                               "cfg.random_starts are set)");
  rmx::LearnParams lp{};
  lp.gamma = lc->gamma;
  lp.lr = lc->learning_rate;
  lp.q = q;
  lp.visits = visits;
  lp.s_max = s_max;
  lp.use_qrm = lc->use_qrm ? 1 : 0;
  lp.use_rsh = lc->use_rsh ? 1 : 0;
  lp.trunc_is_terminal = lc->trunc_is_terminal ? 1 : 0;
  const size_t n_phi = (size_t)h->cfg.n_agents * (size_t)h->cfg.n_rm_states;
  if (h->host) {
    try {
      h->host->learn_phi.assign(lc->use_rsh ? lc->phi : nullptr, lc->use_rsh ? lc->phi + n_phi : nullptr);
    } catch (const std::exception& e) {
      return fail(RMX_E_INVALID, std::string("rmx_learn_bind: ") + e.what());
    }
    lp.phi = lc->use_rsh ? h->host->learn_phi.data() : nullptr;
    h->host->learn = lp;
    h->host->learn_on = true;
    h->host->lam_on = false;  // a new learner: Q-learning until rmx_learn_lambda_bind
    h->host->rmax_on = false; // or rmx_learn_rmax_bind
    h->host->qrmax_on = false;  // or rmx_learn_qrmax_bind
    h->host->eps = {};        // and the scalar epsilon until rmx_learn_eps_bind
    return RMX_OK;
  }
  if ((reinterpret_cast<uintptr_t>(q) & 15u) || (reinterpret_cast<uintptr_t>(visits) & 15u))
    return fail(RMX_E_INVALID, "the q and visits tables must be 16-byte aligned");
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  if (lc->use_rsh) {
    if (!h->learn.d_phi) HIP_TRY(hipMalloc(&h->learn.d_phi, sizeof(double) * n_phi), "phi alloc");
    HIP_TRY(hipMemcpy(h->learn.d_phi, lc->phi, sizeof(double) * n_phi, hipMemcpyHostToDevice), "phi upload");
    lp.phi = h->learn.d_phi;
  }
  h->learn.params = lp;
  h->learn.on = true;
  h->learn.lam_on = false;  // a new learner: Q-learning until rmx_learn_lambda_bind
  h->learn.rmax_on = false; // or rmx_learn_rmax_bind
  h->learn.qrmax_on = false;  // or rmx_learn_qrmax_bind
  h->learn.eps = {};        // and the scalar epsilon until rmx_learn_eps_bind
  return RMX_OK;
}

int rmx_learn_rng_bind(rmx_handle* h, uint64_t* rng) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (!(h->host ? h->host->learn_on : h->learn.on))
    return fail(RMX_E_STATE, "no learner bound (rmx_learn_bind comes before rmx_learn_rng_bind)");
  if (reinterpret_cast<uintptr_t>(rng) & 15u) return fail(RMX_E_INVALID, "the generator column must be 16-byte aligned");
  if (h->host)
    h->host->learn_rng = rng;
  else
    h->learn.rng = rng;
  return RMX_OK;
}

int rmx_learn_rng_seed(rmx_handle* h, const uint64_t* seeds, void* stream) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (!(h->host ? h->host->learn_on : h->learn.on))
    return fail(RMX_E_STATE, "no learner bound (rmx_learn_bind comes before rmx_learn_rng_seed)");
  uint64_t* col = h->host ? h->host->learn_rng : h->learn.rng;
  if (!col) return fail(RMX_E_STATE, "no generator column bound (rmx_learn_rng_bind)");
  if (!seeds) return fail(RMX_E_INVALID, "seeds is NULL");
  const int64_t n = (int64_t)h->cfg.n_agents * h->cfg.n_envs;
  if (h->host) {
    rmx::learn_rng_fill(seeds, n, col);
    return RMX_OK;
  }
  std::vector<uint64_t> words;
  try {
    words.resize((size_t)n * 5);
  } catch (const std::exception& e) {
    return fail(RMX_E_INVALID, std::string("rmx_learn_rng_seed: ") + e.what());
  }
  rmx::learn_rng_fill(seeds, n, words.data());
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  // in stream order after the caller's earlier work; the staging copy lives until the copy has been made
  HIP_TRY(hipMemcpyAsync(col, words.data(), sizeof(uint64_t) * words.size(), hipMemcpyHostToDevice, as_stream(stream)),
          "generator column upload");
  HIP_TRY(hipStreamSynchronize(as_stream(stream)), "generator column upload");
  return RMX_OK;
}

int rmx_learn_lambda_slots(const rmx_handle* h, int32_t* l_full) {
  if (!h || !l_full) return fail(RMX_E_INVALID, "handle or l_full is NULL");
  int64_t s_max = 0;
  const int rc = rmx_learn_states(h, &s_max);
  if (rc) return rc;
  if (s_max * 4 > INT32_MAX) return fail(RMX_E_INVALID, "4 * S_max exceeds the int32 cell indices of the trace lists");
  *l_full = (int32_t)(s_max * 4);
  return RMX_OK;
}

int rmx_learn_lambda_bind(rmx_handle* h, double lambd, int32_t cap, int32_t* idx, double* val, int32_t* cnt) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (!(h->host ? h->host->learn_on : h->learn.on))
    return fail(RMX_E_STATE, "no learner bound (rmx_learn_bind comes before rmx_learn_lambda_bind)");
  if (!idx) {  // back to Q-learning
    if (h->host)
      h->host->lam_on = false;
    else
      h->learn.lam_on = false;
    return RMX_OK;
  }
  if (h->host ? h->host->rmax_on : h->learn.rmax_on)
    return fail(RMX_E_STATE, "an R-max model is bound (rmx_learn_rmax_bind): unbind it before Q(lambda) lists");
  if (h->host ? h->host->qrmax_on : h->learn.qrmax_on)
    return fail(RMX_E_STATE, "a QR-max model is bound (rmx_learn_qrmax_bind): unbind it before Q(lambda) lists");
  const rmx::LearnParams& lp = h->host ? h->host->learn : h->learn.params;
  if (lp.use_qrm || lp.use_rsh)
    return fail(RMX_E_INVALID, "Q(lambda) has no QRM and no shaping (the learner was bound with use_qrm / use_rsh)");
  if (!std::isfinite(lambd) || lambd < 0.0 || lambd > 1.0) return fail(RMX_E_INVALID, "lambd must be in [0, 1]");
  int32_t l_full = 0;
  const int rc = rmx_learn_lambda_slots(h, &l_full);
  if (rc) return rc;
  if (cap < 1 || cap > l_full) return fail(RMX_E_INVALID, "cap must be in [1, 4 * S_max] (rmx_learn_lambda_slots)");
  if (!val || !cnt) return fail(RMX_E_INVALID, "trace_val or trace_cnt is NULL");
  if ((reinterpret_cast<uintptr_t>(idx) & 3u) || (reinterpret_cast<uintptr_t>(val) & 7u) ||
      (reinterpret_cast<uintptr_t>(cnt) & 3u))
    return fail(RMX_E_INVALID, "the trace arrays must be aligned to their element types");
  const rmx::LambdaParams lam = {lambd, idx, val, cnt, cap};
  if (h->host) {
    h->host->lam = lam;
    h->host->lam_on = true;
  } else {
    h->learn.lam = lam;
    h->learn.lam_on = true;
  }
  return RMX_OK;
}

int rmx_learn_traces_clear(rmx_handle* h, const uint8_t* env_mask_dev, void* stream) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (!(h->host ? h->host->lam_on : h->learn.lam_on))
    return fail(RMX_E_STATE, "no Q(lambda) trace lists bound (rmx_learn_lambda_bind)");
  if (h->host) {
    h->host->traces_clear(env_mask_dev);
    return RMX_OK;
  }
  return lambda_clear(h, env_mask_dev, stream);
}

int rmx_learn_rmax_slots(const rmx_handle* h, int32_t* cap_full) {
  if (!h || !cap_full) return fail(RMX_E_INVALID, "handle or cap_full is NULL");
  int64_t s_max = 0;
  const int rc = rmx_learn_states(h, &s_max);
  if (rc) return rc;
  if (s_max > INT32_MAX) return fail(RMX_E_INVALID, "S_max exceeds the int32 state indices of the successor lists");
  *cap_full = rmx::kRMaxSlotsFull;
  return RMX_OK;
}

int rmx_learn_rmax_bind(rmx_handle* h, int32_t threshold, double vi_delta, int vi_delta_rel, int32_t max_iter,
                        int32_t cap, double* rsum, int32_t* succ_idx, int32_t* succ_cnt) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (!(h->host ? h->host->learn_on : h->learn.on))
    return fail(RMX_E_STATE, "no learner bound (rmx_learn_bind comes before rmx_learn_rmax_bind)");
  if (!rsum) {  // back to Q-learning steps on the same tables
    if (h->host)
      h->host->rmax_on = false;
    else
      h->learn.rmax_on = false;
    return RMX_OK;
  }
  if (h->host ? h->host->lam_on : h->learn.lam_on)
    return fail(RMX_E_STATE, "Q(lambda) trace lists are bound (rmx_learn_lambda_bind): unbind them before an R-max model");
  if (h->host ? h->host->qrmax_on : h->learn.qrmax_on)
    return fail(RMX_E_STATE, "a QR-max model is bound (rmx_learn_qrmax_bind): unbind it before an R-max model");
  const rmx::LearnParams& lp = h->host ? h->host->learn : h->learn.params;
  if (lp.use_rsh) return fail(RMX_E_INVALID, "R-max has no reward shaping (the learner was bound with use_rsh)");
  if (!lp.visits) return fail(RMX_E_INVALID, "R-max needs the visits table (it serves as s_a_counts)");
  if (!(lp.gamma < 1.0)) return fail(RMX_E_INVALID, "R-max needs gamma < 1 (value iteration on the learned MDP)");
  if (threshold < 1) return fail(RMX_E_INVALID, "threshold (s_a_threshold) must be >= 1");
  if (!std::isfinite(vi_delta) || vi_delta <= 0.0) return fail(RMX_E_INVALID, "vi_delta must be finite and > 0");
  if (max_iter < 1) return fail(RMX_E_INVALID, "max_iter must be >= 1");
  int32_t cap_full = 0;
  const int rc = rmx_learn_rmax_slots(h, &cap_full);
  if (rc) return rc;
  if (cap < 1 || cap > cap_full) return fail(RMX_E_INVALID, "cap must be in [1, the full cap] (rmx_learn_rmax_slots)");
  if (!succ_idx || !succ_cnt) return fail(RMX_E_INVALID, "succ_idx or succ_cnt is NULL");
  if ((reinterpret_cast<uintptr_t>(rsum) & 7u) || (reinterpret_cast<uintptr_t>(succ_idx) & 3u) ||
      (reinterpret_cast<uintptr_t>(succ_cnt) & 3u))
    return fail(RMX_E_INVALID, "the model arrays must be aligned to their element types");
  const int A = h->cfg.n_agents;
  const int64_t N = h->cfg.n_envs, AN = (int64_t)A * N;
  if (AN > INT32_MAX) return fail(RMX_E_INVALID, "A * N exceeds the int32 learner indices of the worklist");
  const rmx::RMaxParams rp = {vi_delta, vi_delta_rel ? 1 : 0, max_iter, threshold, cap, rsum, succ_idx, succ_cnt};
  if (h->host) {
    try {
      h->host->rmax_scratch.assign((size_t)lp.s_max * 5, 0.0);
    } catch (const std::exception& e) {
      return fail(RMX_E_INVALID, std::string("rmx_learn_rmax_bind: ") + e.what());
    }
    h->host->rmax = rp;
    h->host->rmax_on = true;
    h->host->rmax_solves = h->host->rmax_sweeps_max = 0;
    return RMX_OK;
  }
  // the solve kernel keeps v of one learner double-buffered in LDS, 16 B per state: larger worlds are refused here
  if (lp.s_max > rmx::kRMaxStatesMax)
    return fail(RMX_E_INVALID, "S_max = " + std::to_string(lp.s_max) + " exceeds the " +
                                   std::to_string((long long)rmx::kRMaxStatesMax) +
                                   " states whose values the R-max solve kernel holds in LDS (16 B per state)");
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  // the hand-over between the two kernels, one allocation: counters and statistics | records | headers | worklist
  const int32_t n_exp = 1 + h->cfg.n_qrm_max;
  const size_t off_rec = 64, off_hdr = off_rec + sizeof(rmx::RMaxRec) * (size_t)AN * (size_t)n_exp,
               off_list = off_hdr + 8 * (size_t)AN, bytes = off_list + 4 * (size_t)AN;
  (void)hipFree(h->learn.d_rmax);
  h->learn.d_rmax = nullptr;
  HIP_TRY(hipMalloc(&h->learn.d_rmax, bytes), "R-max worklist alloc");
  HIP_TRY(hipMemset(h->learn.d_rmax, 0, bytes), "R-max worklist clear");
  rmx::RMaxWork wk{};
  wk.count = reinterpret_cast<uint32_t*>(h->learn.d_rmax);
  wk.stats = reinterpret_cast<unsigned long long*>(h->learn.d_rmax + 16);
  wk.recs = reinterpret_cast<rmx::RMaxRec*>(h->learn.d_rmax + off_rec);
  wk.hdr = reinterpret_cast<int32_t*>(h->learn.d_rmax + off_hdr);
  wk.list = reinterpret_cast<int32_t*>(h->learn.d_rmax + off_list);
  wk.n_exp = n_exp;
  wk.parity = 0;
  for (int a = 0; a < A; ++a) wk.S[a] = h->cfg.width * h->cfg.height * h->enc_nq[a];
  wk.N = N;
  wk.n_learners = AN;
  wk.err = h->d_err;
  h->learn.work = wk;
  h->learn.rmax = rp;
  h->learn.rmax_grid = rmx::kRMaxGrid;
  if (const char* g = std::getenv("RMX_RMAX_GRID")) {  // tests: a grid smaller than a step's worklist
    const long v = std::strtol(g, nullptr, 10);
    if (v >= 1 && v <= 65536) h->learn.rmax_grid = (int)v;
  }
  h->learn.rmax_on = true;
  return RMX_OK;
}

int rmx_learn_rmax_info(rmx_handle* h, int64_t* solves, int64_t* max_sweeps) {
  if (!h || !solves || !max_sweeps) return fail(RMX_E_INVALID, "handle, solves or max_sweeps is NULL");
  if (!(h->host ? h->host->rmax_on : h->learn.rmax_on))
    return fail(RMX_E_STATE, "no R-max model bound (rmx_learn_rmax_bind)");
  if (h->host) {
    *solves = h->host->rmax_solves;
    *max_sweeps = h->host->rmax_sweeps_max;
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  HIP_TRY(hipDeviceSynchronize(), "sync");
  unsigned long long st[2] = {0, 0};
  HIP_TRY(hipMemcpy(st, h->learn.work.stats, sizeof(st), hipMemcpyDeviceToHost), "R-max statistics copy");
  *solves = (int64_t)st[0];
  *max_sweeps = (int64_t)st[1];
  return RMX_OK;
}

int rmx_learn_qrmax_slots(const rmx_handle* h, int32_t* cap_full) {
  if (!h || !cap_full) return fail(RMX_E_INVALID, "handle or cap_full is NULL");
  int64_t s_max = 0;
  const int rc = rmx_learn_states(h, &s_max);
  if (rc) return rc;
  if (s_max > INT32_MAX) return fail(RMX_E_INVALID, "S_max exceeds the int32 state indices of the QR-max model");
  *cap_full = rmx::kQRMaxSlotsFull;
  return RMX_OK;
}

int rmx_learn_qrmax_bind(rmx_handle* h, int32_t nsamples_te, int32_t nsamples_re, int32_t nsamples_tq,
                         int32_t nsamples_rq, double vi_delta, int vi_delta_rel, int32_t max_iter, int32_t cap,
                         uint8_t* known_tsqa, int32_t* n_tsa, int32_t* n_rsa, double* sum_rsa, int32_t* succ_idx,
                         int32_t* succ_cnt, int32_t* n_tqs, int32_t* tq_next, int32_t* n_rqs, double* sum_rqs,
                         uint8_t* final) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (!(h->host ? h->host->learn_on : h->learn.on))
    return fail(RMX_E_STATE, "no learner bound (rmx_learn_bind comes before rmx_learn_qrmax_bind)");
  if (!known_tsqa) {  // back to Q-learning steps on the same tables
    if (h->host)
      h->host->qrmax_on = false;
    else
      h->learn.qrmax_on = false;
    return RMX_OK;
  }
  if (h->host ? h->host->lam_on : h->learn.lam_on)
    return fail(RMX_E_STATE, "Q(lambda) trace lists are bound (rmx_learn_lambda_bind): unbind them before a QR-max model");
  if (h->host ? h->host->rmax_on : h->learn.rmax_on)
    return fail(RMX_E_STATE, "an R-max model is bound (rmx_learn_rmax_bind): unbind it before a QR-max model");
  const rmx::LearnParams& lp = h->host ? h->host->learn : h->learn.params;
  if (lp.use_rsh) return fail(RMX_E_INVALID, "QR-max has no reward shaping (the learner was bound with use_rsh)");
  if (!lp.visits) return fail(RMX_E_INVALID, "QR-max needs the visits table (it serves as nTSQA)");
  if (!(lp.gamma < 1.0)) return fail(RMX_E_INVALID, "QR-max needs gamma < 1 (value iteration on the learned MDP)");
  if (nsamples_te < 1 || nsamples_re < 1 || nsamples_tq < 1 || nsamples_rq < 1)
    return fail(RMX_E_INVALID, "every threshold (nsamples_te / _re / _tq / _rq) must be >= 1");
  if (!std::isfinite(vi_delta) || vi_delta <= 0.0) return fail(RMX_E_INVALID, "vi_delta must be finite and > 0");
  if (max_iter < 1) return fail(RMX_E_INVALID, "max_iter must be >= 1");
  int32_t cap_full = 0;
  const int rc = rmx_learn_qrmax_slots(h, &cap_full);
  if (rc) return rc;
  if (cap < 1 || cap > cap_full) return fail(RMX_E_INVALID, "cap must be in [1, the full cap] (rmx_learn_qrmax_slots)");
  if (!n_tsa || !n_rsa || !sum_rsa || !succ_idx || !succ_cnt || !n_tqs || !tq_next || !n_rqs || !sum_rqs || !final)
    return fail(RMX_E_INVALID, "a model array is NULL");
  auto mis = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
  if (mis(sum_rsa, 8) || mis(sum_rqs, 8) || mis(n_tsa, 4) || mis(n_rsa, 4) || mis(succ_idx, 4) || mis(succ_cnt, 4) ||
      mis(n_tqs, 4) || mis(tq_next, 4) || mis(n_rqs, 4))
    return fail(RMX_E_INVALID, "the model arrays must be aligned to their element types");
  const int A = h->cfg.n_agents;
  const int64_t N = h->cfg.n_envs, AN = (int64_t)A * N;
  if (AN > INT32_MAX) return fail(RMX_E_INVALID, "A * N exceeds the int32 learner indices of the worklist");
  rmx::QRMaxParams qp{};
  qp.delta = vi_delta;
  qp.delta_rel = vi_delta_rel ? 1 : 0;
  qp.max_iter = max_iter;
  qp.n_te = nsamples_te;
  qp.n_re = nsamples_re;
  qp.n_tq = nsamples_tq;
  qp.n_rq = nsamples_rq;
  qp.cap = cap;
  qp.P = h->cfg.width * h->cfg.height;
  qp.known_tsqa = known_tsqa;
  qp.n_tsa = n_tsa;
  qp.n_rsa = n_rsa;
  qp.sum_rsa = sum_rsa;
  qp.succ_idx = succ_idx;
  qp.succ_cnt = succ_cnt;
  qp.n_tqs = n_tqs;
  qp.tq_next = tq_next;
  qp.n_rqs = n_rqs;
  qp.sum_rqs = sum_rqs;
  qp.fin = final;
  if (h->host) {
    try {
      h->host->qrmax_scratch.assign((size_t)lp.s_max, 0.0);
    } catch (const std::exception& e) {
      return fail(RMX_E_INVALID, std::string("rmx_learn_qrmax_bind: ") + e.what());
    }
    h->host->qrmax = qp;
    h->host->qrmax_on = true;
    h->host->qrmax_solves = h->host->qrmax_sweeps_max = h->host->qrmax_sweeps_total = 0;
    return RMX_OK;
  }
  // the solve kernel keeps V of one learner double-buffered in LDS, 16 B per state: larger worlds are refused here
  if (lp.s_max > rmx::kRMaxStatesMax)
    return fail(RMX_E_INVALID, "S_max = " + std::to_string(lp.s_max) + " exceeds the " +
                                   std::to_string((long long)rmx::kRMaxStatesMax) +
                                   " states whose values the QR-max solve kernel holds in LDS (16 B per state)");
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  // the hand-over between the two kernels, one allocation: counters and statistics | worklist
  const size_t off_list = 64, bytes = off_list + 4 * (size_t)AN;
  (void)hipFree(h->learn.d_qrmax);
  h->learn.d_qrmax = nullptr;
  HIP_TRY(hipMalloc(&h->learn.d_qrmax, bytes), "QR-max worklist alloc");
  HIP_TRY(hipMemset(h->learn.d_qrmax, 0, bytes), "QR-max worklist clear");
  rmx::RMaxWork wk{};  // (recs and hdr stay NULL: no experience is handed over)
  wk.count = reinterpret_cast<uint32_t*>(h->learn.d_qrmax);
  wk.stats = reinterpret_cast<unsigned long long*>(h->learn.d_qrmax + 16);  // solves, longest solve, sweeps in all
  wk.list = reinterpret_cast<int32_t*>(h->learn.d_qrmax + off_list);
  wk.parity = 0;
  for (int a = 0; a < A; ++a) wk.S[a] = h->cfg.width * h->cfg.height * h->enc_nq[a];
  wk.N = N;
  wk.n_learners = AN;
  wk.err = h->d_err;
  h->learn.qwork = wk;
  h->learn.qrmax = qp;
  h->learn.qrmax_grid = rmx::kRMaxGrid;
  if (const char* g = std::getenv("RMX_QRMAX_GRID")) {  // tests: a grid smaller than a step's worklist
    const long v = std::strtol(g, nullptr, 10);
    if (v >= 1 && v <= 65536) h->learn.qrmax_grid = (int)v;
  }
  h->learn.qrmax_on = true;
  return RMX_OK;
}

int rmx_learn_qrmax_info(rmx_handle* h, int64_t* solves, int64_t* max_sweeps, int64_t* total_sweeps) {
  if (!h || !solves || !max_sweeps || !total_sweeps)
    return fail(RMX_E_INVALID, "handle, solves, max_sweeps or total_sweeps is NULL");
  if (!(h->host ? h->host->qrmax_on : h->learn.qrmax_on))
    return fail(RMX_E_STATE, "no QR-max model bound (rmx_learn_qrmax_bind)");
  if (h->host) {
    *solves = h->host->qrmax_solves;
    *max_sweeps = h->host->qrmax_sweeps_max;
    *total_sweeps = h->host->qrmax_sweeps_total;
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  HIP_TRY(hipDeviceSynchronize(), "sync");
  unsigned long long st[3] = {0, 0, 0};
  HIP_TRY(hipMemcpy(st, h->learn.qwork.stats, sizeof(st), hipMemcpyDeviceToHost), "QR-max statistics copy");
  *solves = (int64_t)st[0];
  *max_sweeps = (int64_t)st[1];
  *total_sweeps = (int64_t)st[2];
  return RMX_OK;
}

int rmx_learn_eps_bind(rmx_handle* h, double* eps, double eps_end, double eps_decay) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (!(h->host ? h->host->learn_on : h->learn.on))
    return fail(RMX_E_STATE, "no learner bound (rmx_learn_bind comes before rmx_learn_eps_bind)");
  rmx::EpsParams ep{};
  if (eps) {  // (NULL: back to the call's scalar epsilon; eps_end and eps_decay are not looked at)
    if (reinterpret_cast<uintptr_t>(eps) & 7u) return fail(RMX_E_INVALID, "the epsilon column must be 8-byte aligned");
    if (!(eps_end >= 0.0 && eps_end <= 1.0)) return fail(RMX_E_INVALID, "eps_end must be in [0, 1]");
    if (!(eps_decay >= 0.0 && eps_decay <= 1.0)) return fail(RMX_E_INVALID, "eps_decay must be finite and in [0, 1]");
    ep = {eps, eps_end, eps_decay};
  }
  if (h->host)
    h->host->eps = ep;
  else
    h->learn.eps = ep;
  return RMX_OK;
}

int rmx_learn_eps_decay(rmx_handle* h, const uint8_t* env_mask, void* stream) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (!(h->host ? h->host->learn_on : h->learn.on))
    return fail(RMX_E_STATE, "no learner bound (rmx_learn_bind comes before rmx_learn_eps_decay)");
  if (!(h->host ? h->host->eps.col : h->learn.eps.col))
    return fail(RMX_E_STATE, "no epsilon column bound (rmx_learn_eps_bind)");
  if (h->host) {
    h->host->eps_decay(env_mask);
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  HIP_TRY(rmx::launch_eps_decay(h->learn.eps, env_mask, h->cfg.n_agents, h->cfg.n_envs, as_stream(stream)),
          "epsilon decay launch");
  return RMX_OK;
}

int rmx_learn_step(rmx_handle* h, const int32_t* actions, int autoreset, void* stream) {
  rmx::LearnCall lc{};
  lc.update = 1;
  return do_learn_step(h, actions, lc, 0, 0, autoreset, stream);
}

int rmx_learn_step_policy(rmx_handle* h, double epsilon, int flags, uint64_t seed, int64_t t_global, int autoreset,
                          int32_t* actions_out, void* stream) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (!(epsilon >= 0.0 && epsilon <= 1.0)) return fail(RMX_E_INVALID, "epsilon must be in [0, 1]");
  if (flags & ~(RMX_LEARN_UPDATE | RMX_LEARN_BEST | RMX_LEARN_NUMPY)) return fail(RMX_E_INVALID, "unknown learn step flags");
  rmx::LearnCall lc{};
  lc.epsilon = epsilon;
  lc.policy = (flags & RMX_LEARN_NUMPY) ? rmx::kLearnNumpy : rmx::kLearnHash;
  lc.update = (flags & RMX_LEARN_UPDATE) ? 1 : 0;
  lc.best = (flags & RMX_LEARN_BEST) ? 1 : 0;
  lc.actions_out = actions_out;
  return do_learn_step(h, nullptr, lc, seed, t_global, autoreset, stream);
}

int rmx_learn_run(rmx_handle* h, int32_t T, double epsilon, int flags, uint64_t seed, int64_t t_global,
                  int32_t* actions_out, void* stream) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (T < 1 || T > RMX_LEARN_RUN_MAX) return fail(RMX_E_INVALID, "T must be in [1, RMX_LEARN_RUN_MAX]");
  if (!(epsilon >= 0.0 && epsilon <= 1.0)) return fail(RMX_E_INVALID, "epsilon must be in [0, 1]");
  if (flags & ~(RMX_LEARN_UPDATE | RMX_LEARN_BEST | RMX_LEARN_NUMPY)) return fail(RMX_E_INVALID, "unknown learn step flags");
  if (!h->bound) return fail(RMX_E_STATE, "buffers not bound (rmx_bind)");
  if (!(h->host ? h->host->learn_on : h->learn.on)) return fail(RMX_E_STATE, "no learner bound (rmx_learn_bind)");
  if (h->host ? h->host->rmax_on : h->learn.rmax_on)
    return fail(RMX_E_STATE, "rmx_learn_run does not serve R-max learners (one thread per env cannot run a "
                             "workgroup-wide solve): rmx_learn_model_run runs them, one wave per env");
  if (h->host ? h->host->qrmax_on : h->learn.qrmax_on)
    return fail(RMX_E_STATE, "rmx_learn_run does not serve QR-max learners (one thread per env cannot run a "
                             "workgroup-wide solve): rmx_learn_model_run runs them, one wave per env");
  rmx::LearnCall lc{};
  lc.epsilon = epsilon;
  lc.policy = (flags & RMX_LEARN_NUMPY) ? rmx::kLearnNumpy : rmx::kLearnHash;
  lc.update = (flags & RMX_LEARN_UPDATE) ? 1 : 0;
  lc.best = (flags & RMX_LEARN_BEST) ? 1 : 0;
  lc.actions_out = actions_out;
  if (lc.policy == rmx::kLearnNumpy) {
    lc.rng = h->host ? h->host->learn_rng : h->learn.rng;
    if (!lc.rng) return fail(RMX_E_STATE, "RMX_LEARN_NUMPY needs a generator column (rmx_learn_rng_bind)");
  }
  if (h->host) {  // the same T steps, one after the other
    const int64_t AN = (int64_t)h->cfg.n_agents * h->cfg.n_envs;
    for (int32_t k = 0; k < T; ++k) {
      h->host->step(nullptr, 1, false, seed, t_global + k, nullptr, &lc);
      if (lc.actions_out) lc.actions_out += AN;
    }
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  rmx::KParams p = base_params(h);
  p.actions = nullptr;
  p.seed = seed;
  p.t_global = t_global;
  p.autoreset = 1;
  HIP_TRY(rmx::launch_learn_run(p, h->learn.params, lc, h->learn.lam_on ? &h->learn.lam : nullptr,
                                h->learn.eps.col ? &h->learn.eps : nullptr, T, h->cfg.kind, h->tables_bytes,
                                as_stream(stream)),
          "learn run launch");
  return RMX_OK;
}

int rmx_learn_model_run(rmx_handle* h, int32_t T, int flags, uint64_t seed, int64_t t_global, int32_t* actions_out,
                        void* stream) {
  if (!h) return fail(RMX_E_INVALID, "handle is NULL");
  if (T < 1 || T > RMX_LEARN_MODEL_RUN_MAX) return fail(RMX_E_INVALID, "T must be in [1, RMX_LEARN_MODEL_RUN_MAX]");
  if (flags & ~(RMX_LEARN_UPDATE | RMX_LEARN_BEST | RMX_LEARN_NUMPY)) return fail(RMX_E_INVALID, "unknown learn step flags");
  if (!h->bound) return fail(RMX_E_STATE, "buffers not bound (rmx_bind)");
  if (!(h->host ? h->host->learn_on : h->learn.on)) return fail(RMX_E_STATE, "no learner bound (rmx_learn_bind)");
  const bool rmax = h->host ? h->host->rmax_on : h->learn.rmax_on;
  const bool qrmax = h->host ? h->host->qrmax_on : h->learn.qrmax_on;
  if (!rmax && !qrmax)
    return fail(RMX_E_STATE, "rmx_learn_model_run serves R-max and QR-max learners (rmx_learn_rmax_bind / "
                             "rmx_learn_qrmax_bind): no model is bound; rmx_learn_run is the entry for such handles");
  rmx::LearnCall lc{};
  lc.policy = (flags & RMX_LEARN_NUMPY) ? rmx::kLearnNumpy : rmx::kLearnHash;
  lc.update = (flags & RMX_LEARN_UPDATE) ? 1 : 0;
  lc.best = (flags & RMX_LEARN_BEST) ? 1 : 0;
  lc.actions_out = actions_out;
  if (lc.policy == rmx::kLearnNumpy) {
    lc.rng = h->host ? h->host->learn_rng : h->learn.rng;
    if (!lc.rng) return fail(RMX_E_STATE, "RMX_LEARN_NUMPY needs a generator column (rmx_learn_rng_bind)");
  }
  const int64_t AN = (int64_t)h->cfg.n_agents * h->cfg.n_envs;
  if (h->host) {  // the same T steps, one after the other
    for (int32_t k = 0; k < T; ++k) {
      h->host->step(nullptr, 1, false, seed, t_global + k, nullptr, &lc);
      if (lc.actions_out) lc.actions_out += AN;
    }
    return RMX_OK;
  }
  SYNC_END_OR_RETURN(h);
  HIP_TRY(hipSetDevice(h->device), "hipSetDevice");
  rmx::KParams p = base_params(h);
  p.actions = nullptr;
  p.seed = seed;
  p.t_global = t_global;
  p.autoreset = 1;
  const size_t lds = rmx::model_run_lds(h->tables_bytes, h->learn.params.s_max);
  if (lds <= rmx::kModelRunLdsMax) {  // one launch: one wave per env, the solves in place
    if (qrmax)
      HIP_TRY(rmx::launch_qrmax_run(p, h->learn.params, lc, h->learn.qrmax, h->learn.qwork, T, h->cfg.kind, lds,
                                    as_stream(stream)),
              "QR-max learn run launch");
    else
      HIP_TRY(rmx::launch_rmax_run(p, h->learn.params, lc, h->learn.rmax, h->learn.work, T, h->cfg.kind, lds,
                                   as_stream(stream)),
              "R-max learn run launch");
    return RMX_OK;
  }
  // the tables and v do not fit in the LDS of a plain launch together: the same T steps as T two-launch steps
  for (int32_t k = 0; k < T; ++k) {
    p.t_global = t_global + k;
    if (qrmax) {
      HIP_TRY(rmx::launch_learn_qrmax(p, h->learn.params, lc, h->learn.qrmax, h->learn.qwork, h->learn.qrmax_grid,
                                      h->cfg.kind, h->tables_bytes, as_stream(stream)),
              "QR-max learn step launch");
      if (lc.update) h->learn.qwork.parity ^= 1;  // (the solve kernel has zeroed the other list's length)
    } else {
      HIP_TRY(rmx::launch_learn_rmax(p, h->learn.params, lc, h->learn.rmax, h->learn.work, h->learn.rmax_grid,
                                     h->cfg.kind, h->tables_bytes, as_stream(stream)),
              "R-max learn step launch");
      if (lc.update) h->learn.work.parity ^= 1;  // (the solve kernel has zeroed the other list's length)
    }
    if (lc.actions_out) lc.actions_out += AN;
  }
  return RMX_OK;
}

}  // extern "C"
