// rmx_capi_learn.cpp — the tabular Q-learning / QRM learner fused into the step (rmx_learn.h, rmx_learn.hip): the
// rmx_learn_* entry points, the Q(lambda) binding with its trace lists and the epsilon schedule included.  Owns
// rmx_handle::learn.
#include <algorithm>
#include <cmath>
#include <cstdint>
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

}  // extern "C"
