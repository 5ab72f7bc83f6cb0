// rmx_rules.h — the step rules, stated once: the action hash, numpy's generator, the slip threshold, one agent-step,
// the env-level rule, reset, the QRM counterfactuals, the get_mdp entry rule and the encoded-state index.  The gfx950
// generic kernels (rmx_kernels.hip, rmx_sync.hip, rmx_learn.hip, through rmx_generic.h / rmx_device.h) and the host
// path (rmx_hoststep.cpp) instantiate these templates over their own parameter block (KParams / HostParams), table
// view and statistics accumulator.  Plain C++: hipcc compiles it for both sides, g++ for the sanitizer build.
//
// Reference semantics restated (paths relative to Alee08/multiagent-rl-rm):
//   wrapper step      rm_environment_wrapper.py:43-107 (rewards = Renv + reward_modifier * RQ, term = env OR RM)
//   FrozenLake        ma_frozen_lake.py:96-154 (step; inactive or RM-final agents frozen), :174-187 (holes),
//                     :189-215 (terminations, read before the RM step), :224-242 (move, up = y - 1),
//                     :244-262 (slip: rng.choice per moving agent)
//   OfficeWorld       ma_office.py:122-202 (step; RM-final agents keep moving), :204-220 (plants), :240-257
//                     (terminations), :269-325 (wall collision -> penalty + wait), :327-379 (slip after the wall check)
//   RM step           reward_machine.py:45-59 (missing (q, event) => stay, reward 0)
//   QRM experiences   rm_environment_wrapper.py:140-183
//   get_mdp           rm_environment_wrapper.py:185-283 (terminal self loops, the FrozenLake decode quirk)
//   loop rules        frozen_lake_main.py:336-376, office_main.py:1696-1749 (episode end = all terminated or all
//                     truncated; success evaluation_metrics.py:248-267)
// numpy's default_rng(seed) (SeedSequence -> PCG64) is restated from numpy/random/bit_generator.pyx
// (SeedSequence.mix_entropy / generate_state) and pcg64.h (pcg_setseq_128_srandom_r,
// pcg_setseq_128_xsl_rr_64_random_r), numpy 2.2, the reference's runtime.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RMX_HD __host__ __device__ __forceinline__
#define RMX_UNROLL _Pragma("unroll")
#else
#define RMX_HD inline
#define RMX_UNROLL
#endif

#include "../../include/rmx.h"

namespace rmx {

// ---- hashes ---------------------------------------------------------------------------------------------------------
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

RMX_HD uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + kGolden;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// SURVEY.md §8(d) (include/rmx.h rmx_step_hashed): a = splitmix64(seed ^ (((t*N + e)*A + i) * GR)) >> 62
RMX_HD int32_t hash_action(uint64_t seed, int64_t t, int64_t n_global, int64_t e, int A, int i) {
  uint64_t ctr = (((uint64_t)t * (uint64_t)n_global + (uint64_t)e) * (uint64_t)A + (uint64_t)i) * kGolden;
  return (int32_t)(splitmix64(seed ^ ctr) >> 62);
}

// ---- numpy default_rng(seed): SeedSequence -> PCG64 (XSL-RR 128/64) -------------------------------------------------
// Generator.random = (next64 >> 11) * 2^-53.
struct Pcg {
  uint64_t hi, lo, ihi, ilo;  // 128-bit state, 128-bit increment
};

RMX_HD uint64_t mul64hi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

RMX_HD void pcg_step(Pcg& r) {
  constexpr uint64_t MH = 0x2360ED051FC65DA4ull, ML = 0x4385DF649FCCF645ull;
  const uint64_t nlo = r.lo * ML;
  const uint64_t nhi = mul64hi(r.lo, ML) + r.lo * MH + r.hi * ML;
  const uint64_t slo = nlo + r.ilo;
  r.hi = nhi + r.ihi + (slo < nlo ? 1ull : 0ull);
  r.lo = slo;
}

// pcg64_next64: advance, then XSL-RR of the new state
RMX_HD uint64_t pcg_next64(Pcg& r) {
  pcg_step(r);
  const uint64_t x = r.hi ^ r.lo;
  const unsigned rot = (unsigned)(r.hi >> 58);
  return (x >> rot) | (x << ((64u - rot) & 63u));
}

RMX_HD uint32_t ss_hashmix(uint32_t v, uint32_t& hc) {
  v ^= hc;
  hc *= 0x931e8875u;
  v *= hc;
  return v ^ (v >> 16);
}

RMX_HD uint32_t ss_mix(uint32_t x, uint32_t y) {
  const uint32_t r = 0xca01f9ddu * x - 0x4973f715u * y;
  return r ^ (r >> 16);
}

// SeedSequence(seed).generate_state(4, uint64) -> pcg_setseq_128_srandom_r(v0:v1, v2:v3).  (Not force-inlined: the
// fast kernels call it from several places.)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline Pcg seed_pcg64(uint64_t seed) {
  uint32_t ent0 = (uint32_t)seed, ent1 = (uint32_t)(seed >> 32);
  const int n = (seed >> 32) ? 2 : 1;  // _coerce_to_uint32_array: little-endian 32-bit words (0 -> [0])
  uint32_t pool[4], hc = 0x43b0d7e5u;
  RMX_UNROLL
  for (int i = 0; i < 4; ++i) pool[i] = ss_hashmix(i == 0 ? ent0 : (i == 1 && n == 2) ? ent1 : 0u, hc);
  RMX_UNROLL
  for (int s = 0; s < 4; ++s)
    RMX_UNROLL
    for (int d = 0; d < 4; ++d)
      if (s != d) pool[d] = ss_mix(pool[d], ss_hashmix(pool[s], hc));
  uint32_t w[8], hb = 0x8b51f9ddu;
  RMX_UNROLL
  for (int i = 0; i < 8; ++i) {
    uint32_t x = pool[i & 3] ^ hb;
    hb *= 0x58f38dedu;
    x *= hb;
    w[i] = x ^ (x >> 16);
  }
  const uint64_t v0 = (uint64_t)w[0] | ((uint64_t)w[1] << 32), v1 = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
  const uint64_t v2 = (uint64_t)w[4] | ((uint64_t)w[5] << 32), v3 = (uint64_t)w[6] | ((uint64_t)w[7] << 32);
  Pcg r;
  r.ihi = (v2 << 1) | (v3 >> 63);  // inc = (initseq << 1) | 1
  r.ilo = (v3 << 1) | 1ull;
  r.hi = 0;
  r.lo = 0;
  pcg_step(r);  // state = 0*M + inc
  const uint64_t lo = r.lo + v1;  // state += initstate
  r.hi = r.hi + v0 + (lo < r.lo ? 1ull : 0ull);
  r.lo = lo;
  pcg_step(r);
  return r;
}

// The reset-seed schedule: episode k of global env e under base seed `base` (p: any block with the schedule's strides)
template <typename P>
RMX_HD uint64_t schedule_seed(const P& p, uint64_t base, int64_t e_global, int32_t k) {
  return base * p.seed_scale + (uint64_t)e_global * p.seed_env_stride + (uint64_t)k * p.seed_episode_stride;
}
template <typename P>  // a block that carries its base seed: KParams (generic kernels), FastParams (fast-path slip)
RMX_HD uint64_t seed_of(const P& p, int64_t e_global, int32_t k) {
  return schedule_seed(p, p.base_seed, e_global, k);
}

// Slip choice threshold: Generator.random() = m * 2^-53 with an integer m < 2^53 (m = next64 >> 11), so cdf <= u
// exactly when ceil(cdf * 2^53) <= m (the scaling by 2^53 is exact); NaN never compares true, cdf >= 1 never does
// either
inline uint64_t slip_threshold(double cdf) {
  if (!(cdf == cdf)) return ~0ull;
  if (cdf <= 0.0) return 0ull;
  if (cdf >= 1.0) return (1ull << 53) + (cdf > 1.0 ? 1ull : 0ull);
  return (uint64_t)std::ceil(std::ldexp(cdf, 53));
}

// ---- state and rules ------------------------------------------------------------------------------------------------
// The generic table blob's sections (build_table_blob, rmx_tables.cpp), wherever the blob lies
struct TableView {
  const uint16_t* cell;
  const uint8_t* ev;
  const uint8_t* nq;
  const float* rr;
  const float* sh;
  const uint8_t* qrm;  // [A][Qx] get_all_states()[:-1] order
};

// Per-agent state while its env is stepped (registers on the device).
struct AgentReg {
  int32_t x, y, q;
  uint32_t f;
  float ret;
};

// Outcome of one agent-step (for the env-level rule and the outputs).
struct AgentOut {
  float reward, shaping, renv;
  bool term, trunc;
  bool env_term;
  uint32_t prev_cell, cell, ev;  // for the QRM counterfactuals
};

// The optional encoded observation of agent a: (y*W + x)*enc_nq[a] + q
template <typename P>
RMX_HD int32_t enc_index(const AgentReg& s, const P& p, int a) {
  return (s.y * p.W + s.x) * p.enc_nq[a] + s.q;
}

// One wrapper step for one agent.  t1 = timestep after the env increment.  rng: the env's generator (slip draws) or
// NULL; the draw itself is slip_choice(p, intended, *rng) of whoever instantiates this (found at instantiation: the
// device's uniform-value form in rmx_device.h, the host's in rmx_hoststep.cpp).
template <int KIND, typename L, typename P, typename R = Pcg>
RMX_HD AgentOut agent_step(AgentReg& s, int32_t act, int a, int32_t t1, const L& T, const P& p, uint32_t* bad,
                           R* rng = nullptr) {
  const int32_t fq = p.final_q[a];
  bool active = s.f & RMX_F_ACTIVE;
  bool fail = s.f & RMX_F_FAIL;
  uint32_t steps = s.f >> RMX_F_STEPS_SHIFT;
  if ((uint32_t)act > (uint32_t)RMX_WAIT) {  // invalid action: recorded, treated as wait
    *bad = 1u;
    act = RMX_WAIT;
  }
  float renv = 0.0f;
  bool env_term, trunc;
  const uint32_t prev_cell = (uint32_t)(s.y * p.W + s.x);
  // move deltas in the kind's convention: FL up = y-1, OW up = y+1
  const int32_t up = (KIND == RMX_FROZEN_LAKE) ? -1 : 1;
  if (KIND == RMX_FROZEN_LAKE) {
    if (active && s.q != fq) {  // inactive or RM already final (pre-step) -> frozen, Renv = 0
      uint32_t c = (uint32_t)(s.y * p.W + s.x);
      int32_t mv = act;
      if (rng && p.stochastic) {  // get_stochastic_action: one rng.choice per moving agent
        if (act == RMX_WAIT)
          *bad = 1u;  // the reference's slip map has no "wait" entry (KeyError)
        else
          mv = slip_choice(p, act, *rng);
      }
      if (mv < RMX_WAIT && ((T.cell[c] >> mv) & 1u)) {
        s.x += (mv == RMX_LEFT) ? -1 : (mv == RMX_RIGHT) ? 1 : 0;
        s.y += (mv == RMX_UP) ? up : (mv == RMX_DOWN) ? -up : 0;
      }
      c = (uint32_t)(s.y * p.W + s.x);
      if (T.cell[c] & RMX_CELL_HAZARD) {  // hole: fail, Renv = penalty_amount
        fail = true;
        renv = p.hazard_penalty;
      }
      steps += 1;
    }
    trunc = (steps > (uint32_t)p.max_t) || (t1 > p.max_t);
    env_term = trunc || (s.q == fq) || fail;  // RM state read before the wrapper's RM step
  } else {
    if (active) {  // OfficeWorld: RM-final agents keep moving
      uint32_t c = (uint32_t)(s.y * p.W + s.x);
      int32_t mv = RMX_WAIT;
      if (act < RMX_WAIT) {
        if ((T.cell[c] >> act) & 1u) {
          mv = act;
        } else {  // wall collision -> (wall_penalty, "wait")
          renv = p.wall_penalty;
          fail = fail || p.wall_fail;
        }
      }
      if (rng && p.stochastic && mv != RMX_WAIT) mv = slip_choice(p, mv, *rng);  // ma_office.py:155-156
      if (mv < RMX_WAIT && ((T.cell[c] >> mv) & 1u)) {  // apply_action re-checks can_move
        s.x += (mv == RMX_LEFT) ? -1 : (mv == RMX_RIGHT) ? 1 : 0;
        s.y += (mv == RMX_UP) ? up : (mv == RMX_DOWN) ? -up : 0;
        c = (uint32_t)(s.y * p.W + s.x);
      }
      if (T.cell[c] & RMX_CELL_HAZARD) {  // plant
        renv += p.hazard_penalty;
        fail = fail || p.hazard_fail;
      }
      steps += 1;
    }
    env_term = fail;
    trunc = t1 > p.max_t;
  }
  active = active && !(env_term || trunc);
  // RM step for every agent (active or not) on its current cell
  const uint32_t cell = (uint32_t)(s.y * p.W + s.x);
  const uint32_t ev = T.ev[a * p.HW + cell];
  const uint32_t ti = ((uint32_t)(a * p.Q + s.q)) * (uint32_t)p.E + ev;
  const int32_t nq = T.nq[ti];
  const float rq = T.rr[ti];
  AgentOut o;
  o.renv = renv;
  o.reward = renv + p.reward_modifier * rq;  // rewards[name] += reward_rm * reward_modifier
  o.env_term = env_term;
  o.prev_cell = prev_cell;
  o.cell = cell;
  o.ev = ev;
  o.shaping = p.has_shaping ? T.sh[ti] : 0.0f;
  const bool rm_term = (nq == fq);
  o.term = env_term || rm_term;
  o.trunc = trunc;
  s.q = nq;
  s.f = (steps << RMX_F_STEPS_SHIFT) | (active ? RMX_F_ACTIVE : 0u) | (fail ? RMX_F_FAIL : 0u) |
        (o.term ? RMX_F_TERM : 0u) | (trunc ? RMX_F_TRUNC : 0u) | (env_term ? RMX_F_ENV_TERM : 0u) |
        (rm_term ? RMX_F_RM_TERM : 0u);
  return o;
}

// QRM counterfactual experiences of agent a (rm_environment_wrapper.py:140-183): for every RM state j of
// get_all_states()[:-1], the same detected event; missing transition => stay, reward 0 (raw reward).  Written to the
// columns qs / qsn / qrq / qdone ([A][Qx][N]) through st(pointer, value), the caller's kind of store.
template <typename L, typename P, typename St>
RMX_HD void qrm_experiences(const AgentOut& o, int a, int64_t e, const L& T, const P& p, int32_t* qs, int32_t* qsn,
                            float* qrq, uint8_t* qdone, St st) {
  const int Qx = p.n_qrm_max;
  const int nj = p.n_qrm[a];
  const int32_t nQ = p.enc_nq[a];
  const int32_t fq = p.final_q[a];
  for (int j = 0; j < Qx; ++j) {
    const int64_t off = ((int64_t)a * Qx + j) * p.N + e;
    if (j < nj) {
      const uint32_t qj = T.qrm[a * Qx + j];
      const uint32_t tj = ((uint32_t)(a * p.Q) + qj) * (uint32_t)p.E + o.ev;
      const int32_t nqj = T.nq[tj];
      st(qs + off, (int32_t)o.prev_cell * nQ + (int32_t)qj);
      st(qsn + off, (int32_t)o.cell * nQ + nqj);
      st(qrq + off, T.rr[tj]);
      st(qdone + off, (uint8_t)(o.env_term || nqj == fq));
    } else {
      st(qs + off, (int32_t)-1);
      st(qsn + off, (int32_t)-1);
      st(qrq + off, 0.0f);
      st(qdone + off, (uint8_t)0);
    }
  }
}

// One env step for all A agents of env e.  Returns true if the episode ended this step.  ls: the episode statistics
// accumulator (ret, episodes, successes, length), added to per finished env, then per agent.
template <int KIND, int AMAX, typename L, typename P, typename S, typename R>
RMX_HD bool env_step(AgentReg (&s)[AMAX], int32_t& t, const int32_t (&act)[AMAX], const L& T, const P& p, float disc,
                     AgentOut (&o)[AMAX], S& ls, uint32_t* bad, R* rng) {
  // a caller-written t may be INT32_MAX: the host spells the wrap out; the kernels keep the plain add, whose
  // no-overflow assumption their compare against max_t is compiled with
#if defined(__HIP_DEVICE_COMPILE__)
  const int32_t t1 = t + 1;
#else
  const int32_t t1 = (int32_t)((uint32_t)t + 1u);
#endif
  bool all_term = true, all_trunc = true;
  RMX_UNROLL
  for (int a = 0; a < AMAX; ++a) {
    if (AMAX <= 4 || a < p.A) {
      o[a] = agent_step<KIND>(s[a], act[a], a, t1, T, p, bad, rng);  // agents draw in order (one env rng)
      s[a].ret = fmaf(disc, o[a].reward, s[a].ret);
      all_term = all_term && o[a].term;
      all_trunc = all_trunc && o[a].trunc;
    }
  }
  t = t1;
  const bool done = all_term || all_trunc;
  if (done) {
    ls.episodes += 1;
    ls.length += t1;
    RMX_UNROLL
    for (int a = 0; a < AMAX; ++a) {
      if (AMAX <= 4 || a < p.A) {
        s[a].f |= RMX_F_ENV_DONE;
        ls.ret += (double)s[a].ret;
        ls.successes += (o[a].term && s[a].q == p.final_q[a] && s[a].ret > 0.0f) ? 1 : 0;
      }
    }
  }
  return done;
}

template <int AMAX, typename P>
RMX_HD void reset_regs(AgentReg (&s)[AMAX], int32_t& t, const P& p) {
  t = 0;
  RMX_UNROLL
  for (int a = 0; a < AMAX; ++a) {
    s[a].x = p.start_x[a];
    s[a].y = p.start_y[a];
    s[a].q = p.init_q[a];
    s[a].f = RMX_F_ACTIVE;
    s[a].ret = 0.0f;
  }
}

// RMEnvironmentWrapper.get_mdp, entry i = 4 * (encoded state) + action of agent ag under deterministic dynamics, into
// next / reward / done [S][4]: decode (x, y, q) with the agent's encoder stride, apply the terminal self-loop rule
// (is_terminal_state_mdp), else run agent_step from timestep 0.  done = 255 marks "no entry" (the reference's
// FrozenLake decode quirk: no entries for non-hole states; kept unless fix_fl).
template <int KIND, typename L, typename P>
RMX_HD void mdp_entry(int64_t i, int ag, int fix_fl, const L& T, const P& p, int32_t* next, float* reward,
                      uint8_t* done) {
  const int64_t s = i >> 2;
  const int act = (int)(i & 3);
  const int32_t nQ = p.enc_nq[ag];
  const int32_t q = (int32_t)(s % nQ), pos = (int32_t)(s / nQ);
  const bool hz = (T.cell[pos] & RMX_CELL_HAZARD) != 0;
  bool term_state = false;
  float term_r = 0.0f;
  if (KIND == RMX_FROZEN_LAKE) {
    if (hz) {
      term_state = true;
      term_r = p.hazard_penalty;
    } else if (fix_fl && q == p.final_q[ag]) {
      term_state = true;
    } else if (!fix_fl) {
      next[i] = -1;
      reward[i] = 0.0f;
      done[i] = 255;
      return;
    }
  } else {
    if (hz && p.hazard_fail) {
      term_state = true;
      term_r = p.hazard_penalty;
    } else if (q == p.final_q[ag]) {
      term_state = true;
    }
  }
  if (term_state) {
    next[i] = (int32_t)s;
    reward[i] = term_r;
    done[i] = 1;
    return;
  }
  AgentReg st = {pos % p.W, pos / p.W, q, RMX_F_ACTIVE, 0.0f};
  uint32_t bad = 0;
  const AgentOut o = agent_step<KIND>(st, act, ag, 1, T, p, &bad);
  next[i] = (int32_t)o.cell * nQ + st.q;
  reward[i] = o.reward;
  done[i] = (uint8_t)(o.term || o.trunc);
}

}  // namespace rmx
