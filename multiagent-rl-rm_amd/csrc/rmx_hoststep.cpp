// rmx_hoststep.cpp — the host path of the step engine (rmx_hoststep.h): envs stepped on the CPU over the generic
// kernels' table blob, one env after another, agents in order.
//
// The step rules, numpy's generator and the action hash are those of rmx_rules.h, instantiated here over HostParams
// (the reference semantics are cited there).  What this file adds is the host's own: the range clamp on load, the
// column stores, the learner hook, Generator.shuffle as the plain Fisher-Yates it is (random starts), and the slip
// choice without the device's uniform-value form (Generator.choice / .shuffle restated from numpy's _generator.pyx,
// numpy 2.2, the reference's runtime).
#include "rmx_hoststep.h"

#include <cmath>
#include <cstring>

namespace rmx {

// rng.choice(outcomes, p=probs) with the intended action's row: one Generator.random() draw, searchsorted(side="right")
// (agent_step of rmx_rules.h finds it by its arguments)
inline int32_t slip_choice(const HostParams& p, int32_t intended, Pcg& r) {
  const uint64_t m = pcg_next64(r) >> 11;
  int idx = 0;
  for (int i = 0; i + 1 < p.slip_n[intended] && i < 3; ++i) idx += p.slip_thr[intended][i] <= m ? 1 : 0;
  return p.slip_out[intended][idx];
}

namespace {

// env_step's statistics accumulator: the handle's four doubles, added to in env_step's order
struct HostStats {
  double &ret, &episodes, &successes, &length;
};

}  // namespace

void learn_rng_fill(const uint64_t* seeds, int64_t n, uint64_t* col) {
  for (int64_t i = 0; i < n; ++i) {
    const Pcg r = seed_pcg64(seeds[i]);
    col[i] = r.hi;
    col[n + i] = r.lo;
    col[2 * n + i] = r.ihi;
    col[3 * n + i] = r.ilo;
    col[4 * n + i] = 0;  // no 32-bit half buffered
  }
}

std::string HostEngine::init(const rmx_config& c) {
  BlobOffsets bo;
  if (!build_table_blob(c, blob, bo)) return "tables exceed 64 KiB (the generic kernels' LDS blob)";
  cfg = c;
  tv.cell = reinterpret_cast<const uint16_t*>(blob.data() + bo.cell);
  tv.ev = blob.data() + bo.ev;
  tv.nq = blob.data() + bo.nq;
  tv.rr = reinterpret_cast<const float*>(blob.data() + bo.rr);
  tv.sh = reinterpret_cast<const float*>(blob.data() + bo.sh);
  tv.qrm = blob.data() + bo.qrm;
  disc = discount_table(c);
  if (c.random_starts) {
    free_cells = rmx::free_cells(c);
    shuffle.resize(free_cells.size());
  }
  enc_on = c.enc_nq != nullptr;
  p = HostParams{};
  p.W = c.width;
  p.HW = c.width * c.height;
  p.A = c.n_agents;
  p.Q = c.n_rm_states;
  p.E = c.n_events;
  p.max_t = c.max_t;
  p.N = c.n_envs;
  p.hazard_penalty = c.hazard_penalty;
  p.wall_penalty = c.wall_penalty;
  p.hazard_fail = c.hazard_fail;
  p.wall_fail = c.wall_fail;
  p.has_shaping = c.has_shaping;
  p.reward_modifier = c.reward_modifier;
  p.n_qrm_max = c.n_qrm_max;
  p.stochastic = c.stochastic;
  p.seed_scale = c.seed_scale;
  p.seed_env_stride = c.seed_env_stride;
  p.seed_episode_stride = c.seed_episode_stride;
  for (int a = 0; a < c.n_agents; ++a) {
    p.init_q[a] = c.init_q[a];
    p.final_q[a] = c.final_q[a];
    p.start_x[a] = c.start_xy[2 * a];
    p.start_y[a] = c.start_xy[2 * a + 1];
    p.enc_nq[a] = c.enc_nq ? c.enc_nq[a] : 0;
    p.n_qrm[a] = c.n_qrm_max > 0 ? c.n_qrm[a] : 0;
  }
  if (c.stochastic)
    for (int i = 0; i < 4; ++i) {
      p.slip_n[i] = c.slip_n[i];
      for (int j = 0; j < 4; ++j) {
        p.slip_out[i][j] = c.slip_out[i][j];
        p.slip_thr[i][j] = slip_threshold(c.slip_cdf[i][j]);
      }
    }
  const size_t AN = (size_t)c.n_agents * (size_t)c.n_envs, N = (size_t)c.n_envs;
  own_reward.assign(AN, 0.0f);
  own_renv.assign(AN, 0.0f);
  own_shaping.assign(c.has_shaping ? AN : 0, 0.0f);
  own_done.assign(N, 0);
  own_enc.assign(enc_on ? AN : 0, 0);
  cfg.cell = nullptr;
  cfg.cell_event = nullptr;
  cfg.next_q = nullptr;
  cfg.rm_reward = nullptr;
  cfg.shape = nullptr;
  cfg.init_q = cfg.final_q = cfg.start_xy = nullptr;
  cfg.n_qrm = cfg.enc_nq = nullptr;
  cfg.qrm_states = nullptr;
  return std::string();
}

void HostEngine::bind(const rmx_buffers& b) {
  buf = b;
  reward = b.reward;
  renv = b.renv ? b.renv : own_renv.data();
  shaping = !cfg.has_shaping ? nullptr : b.shaping ? b.shaping : own_shaping.data();
  env_done = b.env_done ? b.env_done : own_done.data();
  enc = !enc_on ? nullptr : b.enc_state ? b.enc_state : own_enc.data();
  bound = true;
  pending = false;
}

// _sample_start_positions: rng.shuffle(free_cells) (the untyped Fisher-Yates: for i = n-1 .. 1 swap x[i] with
// x[random_interval(i)], 32-bit draws masked to the smallest all-ones mask >= i and rejected while > i, each 64-bit
// output giving its low half, then its high half), agent a on the a-th cell
void HostEngine::random_starts(Pcg& r, AgentReg* s) {
  const int32_t n = (int32_t)free_cells.size();
  std::memcpy(shuffle.data(), free_cells.data(), sizeof(uint16_t) * (size_t)n);
  bool have_half = false;
  uint32_t half = 0;
  auto next32 = [&]() {
    if (have_half) {
      have_half = false;
      return half;
    }
    const uint64_t o = pcg_next64(r);
    half = (uint32_t)(o >> 32);
    have_half = true;
    return (uint32_t)o;
  };
  for (int32_t i = n - 1; i >= 1; --i) {
    uint32_t mask = (uint32_t)i;
    mask |= mask >> 1;
    mask |= mask >> 2;
    mask |= mask >> 4;
    mask |= mask >> 8;
    mask |= mask >> 16;
    uint32_t j;
    while ((j = next32() & mask) > (uint32_t)i) {
    }
    const uint16_t tmp = shuffle[i];
    shuffle[i] = shuffle[j];
    shuffle[j] = tmp;
  }
  for (int a = 0; a < cfg.n_agents; ++a) {
    s[a].x = shuffle[a] % cfg.width;
    s[a].y = shuffle[a] / cfg.width;
  }
}

void HostEngine::reset(const uint8_t* mask, uint64_t seed) {
  base_seed = seed;
  const int64_t N = cfg.n_envs;
  const int A = cfg.n_agents;
  const bool rng_on = cfg.stochastic || cfg.random_starts;
  for (int64_t e = 0; e < N; ++e) {
    if (mask && !mask[e]) continue;
    AgentReg s[RMX_MAX_AGENTS];
    int32_t t;
    reset_regs(s, t, p);
    if (rng_on) {  // env.reset: self.rng = default_rng(seed); episode 0 of the schedule
      Pcg r = seed_pcg64(schedule_seed(p, base_seed, cfg.env_offset + e, 0));
      if (cfg.random_starts) random_starts(r, s);
      buf.rng[e] = r.hi;
      buf.rng[N + e] = r.lo;
      buf.rng[2 * N + e] = r.ihi;
      buf.rng[3 * N + e] = r.ilo;
      buf.episode[e] = 0;
    }
    buf.t[e] = t;
    for (int a = 0; a < A; ++a) {
      const int64_t k = (int64_t)a * N + e;
      buf.pos_x[k] = s[a].x;
      buf.pos_y[k] = s[a].y;
      buf.rm_q[k] = s[a].q;
      buf.flags[k] = s[a].f;
      buf.ep_ret[k] = s[a].ret;
    }
  }
  traces_clear(mask);  // env.reset() clears every learner's traces
}

void HostEngine::traces_clear(const uint8_t* mask) {
  if (!lam_on) return;
  const int64_t N = cfg.n_envs;
  for (int64_t e = 0; e < N; ++e) {
    if (mask && !mask[e]) continue;
    for (int a = 0; a < cfg.n_agents; ++a) lam.cnt[(int64_t)a * N + e] = 0;
  }
}

uint32_t HostEngine::rmax_agent(const LearnTables& T, const LearnStep& st, int a, int64_t e, int k) {
  const int64_t S = mdp_states(a);
  const RMaxLearner L = rmax_learner(learn, rmax, (int64_t)a * cfg.n_envs + e);
  uint32_t bad = 0;
  const int n = rmax_n_exp(learn, T);
  for (int j = 0; j < n; ++j) {
    LearnExp x;
    if (!rmax_experience(learn, T, st, j, S, x)) continue;
    const int res = rmax_update_q(rmax, L, x, k);
    if (res & kRMaxFull) bad |= (uint32_t)kErrModelFull;
    if (res & kRMaxCross) {  // solved before the next experience of the same step
      const int sweeps = rmax_solve(rmax, learn.gamma, L, S, rmax_scratch.data(), rmax_scratch.data() + learn.s_max);
      ++rmax_solves;
      rmax_sweeps_max = std::max<int64_t>(rmax_sweeps_max, sweeps);
    }
  }
  return bad;
}

uint32_t HostEngine::qrmax_agent(const LearnTables& T, const LearnStep& st, int a, int64_t e, int k) {
  const QRMaxLearner L = qrmax_learner(learn, qrmax, (int64_t)a * cfg.n_envs + e);
  uint32_t bad = 0;
  bool fresh = false;
  const int n = qrmax_n_exp(learn, T);
  for (int j = 0; j < n; ++j) {
    QRMaxExp x;
    if (!qrmax_experience(learn, T, st, j, qrmax.P, x)) continue;
    const int res = qrmax_update(qrmax, L, T.enc_nq, x, k);
    if (res & kQRMaxFull) bad |= (uint32_t)kErrModelFull;
    fresh = fresh || (res & kQRMaxNew);
  }
  if (fresh) {  // one solve behind the last experience of the agent-step
    const int sweeps = qrmax_solve(qrmax, learn.gamma, L, T.enc_nq, qrmax_scratch.data());
    ++qrmax_solves;
    qrmax_sweeps_max = std::max<int64_t>(qrmax_sweeps_max, sweeps);
    qrmax_sweeps_total += sweeps;
  }
  return bad;
}

void HostEngine::eps_decay(const uint8_t* mask) {
  const int64_t N = cfg.n_envs;
  for (int64_t e = 0; e < N; ++e) {
    if (mask && !mask[e]) continue;
    learn_eps_reset(eps, cfg.n_agents, N, e);
  }
}

uint32_t HostEngine::step(const int32_t* actions, int autoreset, bool hashed, uint64_t seed, int64_t t_global,
                          float* trace, const LearnCall* lc) {
  if (cfg.kind == RMX_FROZEN_LAKE)
    return step_kind<RMX_FROZEN_LAKE>(actions, autoreset, hashed, seed, t_global, trace, lc);
  return step_kind<RMX_OFFICE_WORLD>(actions, autoreset, hashed, seed, t_global, trace, lc);
}

template <int KIND>
uint32_t HostEngine::step_kind(const int32_t* actions, int autoreset, bool hashed, uint64_t seed, int64_t t_global,
                               float* trace, const LearnCall* lc) {
  const int64_t N = cfg.n_envs;
  const int A = cfg.n_agents;
  const bool rng_on = cfg.stochastic || cfg.random_starts;
  HostStats ls = {stats[RMX_STAT_SUM_RETURN], stats[RMX_STAT_EPISODES], stats[RMX_STAT_SUCCESSES],
                  stats[RMX_STAT_SUM_LENGTH]};
  uint32_t bad = 0;
  for (int64_t e = 0; e < N; ++e) {
    AgentReg s[RMX_MAX_AGENTS];
    int32_t act[RMX_MAX_AGENTS];
    int32_t t = buf.t[e];
    for (int a = 0; a < A; ++a) {
      const int64_t k = (int64_t)a * N + e;
      s[a] = {buf.pos_x[k], buf.pos_y[k], buf.rm_q[k], buf.flags[k], buf.ep_ret[k]};
      // columns a caller wrote out of range index no table outside it (the kernels' range-checked descriptors give
      // the same guarantee on the device; the values that follow are unspecified, as there)
      if ((uint32_t)s[a].x >= (uint32_t)cfg.width) s[a].x = 0;
      if ((uint32_t)s[a].y >= (uint32_t)cfg.height) s[a].y = 0;
      if ((uint32_t)s[a].q >= (uint32_t)cfg.n_rm_states) s[a].q = 0;
      act[a] = hashed ? hash_action(seed, t_global, cfg.n_envs_global, cfg.env_offset + e, A, a)
               : actions   ? actions[k]
                           : 0;
    }
    Pcg rng = {0, 0, 0, 0};
    if (rng_on) rng = {buf.rng[e], buf.rng[N + e], buf.rng[2 * N + e], buf.rng[3 * N + e]};
    const bool was_reset = autoreset && (s[0].f & RMX_F_ENV_DONE);
    if (was_reset) {  // the loop's reset() before this step
      reset_regs(s, t, p);
      // a learn step's reset is learn_done_episode for every agent's learner: a policy step decays where it reads the
      // learner's epsilon below, a step on the caller's actions here (as the kernel)
      if (lc && !lc->policy && eps.col && !rmax_on && !qrmax_on) learn_eps_reset(eps, A, N, e);
      if (lc && lam_on)  // a learn step's reset clears the traces of every agent's learner
        for (int a = 0; a < A; ++a) lam.cnt[(int64_t)a * N + e] = 0;
      if (rng_on) {  // env.rng = default_rng(seed of the next episode)
        const int32_t k = buf.episode[e] + 1;
        buf.episode[e] = k;
        rng = seed_pcg64(schedule_seed(p, base_seed, cfg.env_offset + e, k));
        if (cfg.random_starts) random_starts(rng, s);  // before any slip draw of the episode
      }
    }
    int32_t q_pre[RMX_MAX_AGENTS];
    for (int a = 0; a < A; ++a) {
      q_pre[a] = s[a].q;
      if (lc && lc->policy) {  // the engine's policy over the row of the state the step is about to leave
        static const double none[4] = {0.0, 0.0, 0.0, 0.0};  // a state outside the agent's table (as on the device)
        const int64_t st = ((int64_t)s[a].y * p.W + s[a].x) * p.enc_nq[a] + s[a].q;
        const double* row = (uint64_t)st < (uint64_t)mdp_states(a)
                                ? learn.q + (((int64_t)a * N + e) * learn.s_max + st) * 4
                                : none;
        // the learner's own epsilon with a schedule bound (decayed under RMX_LEARN_BEST too), else the call's
        if (qrmax_on) {  // QR-max has no epsilon: the shuffle on every numpy call; a flat row picks, any other argmax
          if (lc->policy == kLearnNumpy) {
            const int64_t plane = (int64_t)A * N;
            uint64_t* w = lc->rng + (int64_t)a * N + e;
            LearnRng r = learn_rng_load(w, plane);
            const uint64_t w4 = learn_rng_word4(r);
            act[a] = qrmax_policy_numpy(r, lc->best, row[0], row[1], row[2], row[3]);
            learn_rng_store(w, plane, r, w4);
          } else {
            act[a] = rmax_policy(seed, t_global, cfg.n_envs_global, cfg.env_offset + e, A, a, lc->best, row[0], row[1],
                                 row[2], row[3]);
          }
          if (lc->actions_out) lc->actions_out[(int64_t)a * N + e] = act[a];
          continue;
        }
        if (rmax_on) {  // R-max has no epsilon: a flat row draws, any other takes its first maximum
          if (lc->policy == kLearnNumpy && !lc->best) {
            if (rmax_row_flat(row[0], row[1], row[2], row[3])) {  // (no draw otherwise: the column is not touched)
              const int64_t plane = (int64_t)A * N;
              uint64_t* w = lc->rng + (int64_t)a * N + e;
              LearnRng r = learn_rng_load(w, plane);
              const uint64_t w4 = learn_rng_word4(r);
              act[a] = rmax_policy_numpy(r, row[0], row[1], row[2], row[3]);
              learn_rng_store(w, plane, r, w4);
            } else {
              act[a] = rmax_argmax(row[0], row[1], row[2], row[3]);
            }
          } else {
            act[a] = rmax_policy(seed, t_global, cfg.n_envs_global, cfg.env_offset + e, A, a, lc->best, row[0], row[1],
                                 row[2], row[3]);
          }
          if (lc->actions_out) lc->actions_out[(int64_t)a * N + e] = act[a];
          continue;
        }
        const double epsilon = eps.col ? learn_eps_step(eps, a, N, e, was_reset) : lc->epsilon;
        if (lc->policy == kLearnNumpy && !lc->best) {  // the learner's own numpy generator (RMX_LEARN_NUMPY)
          const int64_t plane = (int64_t)A * N;
          uint64_t* w = lc->rng + (int64_t)a * N + e;
          LearnRng r = learn_rng_load(w, plane);
          const uint64_t w4 = learn_rng_word4(r);
          act[a] = learn_policy_numpy(r, epsilon, row[0], row[1], row[2], row[3]);
          learn_rng_store(w, plane, r, w4);
        } else {
          act[a] = learn_policy(seed, t_global, cfg.n_envs_global, cfg.env_offset + e, A, a, epsilon, lc->best,
                                row[0], row[1], row[2], row[3]);
        }
        if (lc->actions_out) lc->actions_out[(int64_t)a * N + e] = act[a];
      }
    }
    const float d = cfg.gamma == 1.0f ? 1.0f : disc[(size_t)std::min<uint32_t>((uint32_t)t, (uint32_t)cfg.max_t + 1u)];
    AgentOut o[RMX_MAX_AGENTS];
    // agents in order (one env rng), then the episode statistics (the loops' per-episode logging)
    const bool done = env_step<KIND>(s, t, act, tv, p, d, o, ls, &bad, rng_on ? &rng : nullptr);
    if (rng_on) {
      buf.rng[e] = rng.hi;
      buf.rng[N + e] = rng.lo;
      buf.rng[2 * N + e] = rng.ihi;
      buf.rng[3 * N + e] = rng.ilo;
    }
    buf.t[e] = t;
    env_done[e] = (uint8_t)done;
    for (int a = 0; a < A; ++a) {
      const int64_t k = (int64_t)a * N + e;
      buf.pos_x[k] = s[a].x;
      buf.pos_y[k] = s[a].y;
      buf.rm_q[k] = s[a].q;
      buf.flags[k] = s[a].f;
      buf.ep_ret[k] = s[a].ret;
      reward[k] = o[a].reward;
      renv[k] = o[a].renv;
      if (shaping) shaping[k] = o[a].shaping;
      if (enc) enc[k] = enc_index(s[a], p, a);
      if (trace) trace[k] = o[a].reward;
      if (buf.qrm_s)
        qrm_experiences(o[a], a, e, tv, p, buf.qrm_s, buf.qrm_sn, buf.qrm_rq, buf.qrm_done,
                        [](auto* ptr, auto v) { *ptr = v; });
      // the learner's update: every agent, frozen ones included; an action without a table column (wait, or an
      // invalid one, reported above) has nothing to update
      if (lc && lc->update && (uint32_t)act[a] < 4u) {
        const size_t ta = (size_t)a * p.Q * p.E;
        const LearnTables T = {tv.nq + ta,
                               tv.rr + ta,
                               tv.qrm + (size_t)a * p.n_qrm_max,
                               learn.phi ? learn.phi + (size_t)a * p.Q : nullptr,
                               p.E,
                               p.n_qrm[a],
                               p.enc_nq[a],
                               p.final_q[a],
                               p.reward_modifier,
                               p.Q};
        const LearnStep st = {o[a].prev_cell, o[a].cell, o[a].ev,   q_pre[a],  s[a].q,
                              o[a].env_term,  o[a].term, o[a].trunc, o[a].renv};
        const int64_t base = ((int64_t)a * N + e) * learn.s_max * 4;
        double* va = learn.visits ? learn.visits + base : nullptr;
        if (qrmax_on)
          bad |= qrmax_agent(T, st, a, e, act[a]);
        else if (rmax_on)
          bad |= rmax_agent(T, st, a, e, act[a]);
        else if (lam_on)
          bad |= learn_lambda_agent(learn, lam, T, st, learn.q + base, va, act[a], mdp_states(a), a, N, e)
                     ? (uint32_t)kErrTraceFull
                     : 0u;
        else
          learn_agent(learn, T, st, learn.q + base, va, act[a], mdp_states(a));
      }
    }
  }
  err |= bad;
  return bad & 1u;  // (a full trace list is reported by rmx_check_errors only)
}

void HostEngine::fill_actions(uint64_t seed, int64_t t0, int32_t T, int32_t* out) const {
  const int64_t N = cfg.n_envs;
  const int A = cfg.n_agents;
  for (int64_t s = 0; s < T; ++s)
    for (int a = 0; a < A; ++a)
      for (int64_t e = 0; e < N; ++e)
        out[(s * A + a) * N + e] = hash_action(seed, t0 + s, cfg.n_envs_global, cfg.env_offset + e, A, a);
}

int64_t HostEngine::mdp_states(int agent) const {
  return (int64_t)p.HW * p.enc_nq[agent];
}

// get_mdp of one agent (deterministic dynamics): every (encoded state, action), each entry by mdp_entry (rmx_rules.h)
void HostEngine::mdp(int ag, int fix_fl, int32_t* next, float* rew, uint8_t* done) const {
  if (cfg.kind == RMX_FROZEN_LAKE)
    mdp_kind<RMX_FROZEN_LAKE>(ag, fix_fl, next, rew, done);
  else
    mdp_kind<RMX_OFFICE_WORLD>(ag, fix_fl, next, rew, done);
}

template <int KIND>
void HostEngine::mdp_kind(int ag, int fix_fl, int32_t* next, float* rew, uint8_t* done) const {
  const int64_t S = mdp_states(ag);
  for (int64_t i = 0; i < S * 4; ++i) {
    mdp_entry<KIND>(i, ag, fix_fl, tv, p, next, rew, done);
  }
}

std::string HostEngine::copy_out(const rmx_buffers& out) const {
  const int64_t A = cfg.n_agents, N = cfg.n_envs;
  if (out.shaping && !cfg.has_shaping) return "sync output column not computed: shaping";
  if (out.enc_state && !enc_on) return "sync output column not computed: enc_state";
  if ((out.qrm_s || out.qrm_sn || out.qrm_rq || out.qrm_done) && !buf.qrm_s)
    return "sync output columns not computed: QRM (bind the QRM columns)";
  const size_t AN = (size_t)(A * N), AQN = AN * (size_t)(buf.qrm_s ? cfg.n_qrm_max : 0);
  auto cp = [](void* dst, const void* src, size_t n) {
    if (dst && dst != src) std::memcpy(dst, src, n);
  };
  auto zero_or = [&](void* dst, const void* src, size_t n) {  // a reset returns no step outputs: zeros
    if (!dst) return;
    if (last_reset)
      std::memset(dst, 0, n);
    else
      cp(dst, src, n);
  };
  cp(out.pos_x, buf.pos_x, 4 * AN);
  cp(out.pos_y, buf.pos_y, 4 * AN);
  cp(out.rm_q, buf.rm_q, 4 * AN);
  cp(out.flags, buf.flags, 4 * AN);
  cp(out.ep_ret, buf.ep_ret, 4 * AN);
  cp(out.t, buf.t, 4 * (size_t)N);
  zero_or(out.reward, reward, 4 * AN);
  zero_or(out.renv, renv, 4 * AN);
  zero_or(out.shaping, shaping, 4 * AN);
  zero_or(out.env_done, env_done, (size_t)N);
  if (out.enc_state) {  // after a reset too: the encoded start state
    for (int64_t a = 0; a < A; ++a)
      for (int64_t e = 0; e < N; ++e) {
        const int64_t k = a * N + e;
        out.enc_state[k] = enc_index(AgentReg{buf.pos_x[k], buf.pos_y[k], buf.rm_q[k], 0u, 0.0f}, p, (int)a);
      }
  }
  cp(out.qrm_s, buf.qrm_s, 4 * AQN);
  cp(out.qrm_sn, buf.qrm_sn, 4 * AQN);
  cp(out.qrm_rq, buf.qrm_rq, 4 * AQN);
  cp(out.qrm_done, buf.qrm_done, AQN);
  return std::string();
}

}  // namespace rmx
