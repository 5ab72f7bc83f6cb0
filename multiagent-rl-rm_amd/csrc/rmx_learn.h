// rmx_learn.h — the tabular Q-learning / QRM learner's arithmetic and policy, one source for the gfx950 kernel
// (rmx_learn.hip) and the host path (rmx_hoststep.cpp).  Plain C++, as rmx_rules.h (whose hash and generator it uses):
// hipcc compiles it for both sides, g++ for the sanitizer build.
//
// Reference semantics restated (paths relative to Alee08/multiagent-rl-rm):
//   update_q          learning_algorithms/qlearning.py:70-79 (visits += 1 first; lr fixed or 1 / visits;
//                     max_future_q = 0 when terminated; new = (1 - lr) * cur + lr * (r + gamma * max_future_q))
//   QRM experiences   qlearning.py:82-106 over rm_environment_wrapper.py:140-183 (one update_q per state of
//                     get_all_states()[:-1], in order, on the same table: a later one reads what an earlier one wrote)
//   shaping           qlearning.py:93-105 (r += gamma * Phi(next) - Phi(prev), the learner's gamma)
//   greedy ties       qlearning.py:137-143 (the maxima by equality with the row maximum, in index order), best:
//                     np.argmax (qlearning.py:116-117)
//   choose_action     qlearning.py:112-143 on the learner's own default_rng(seed) (learning_algorithm.py:32): the
//                     explore test, Generator.choice for the explore action and among the maxima (learn_policy_numpy)
// Every operation below is one IEEE float64 operation, in the reference's order: contraction into fused
// multiply-adds is off for this file's arithmetic on both sides (hipcc contracts across statements by default).
#pragma once
#include <stdint.h>

#include <type_traits>

#include "rmx_rules.h"

#if defined(__clang__)
#define RMX_LEARN_NOFMA _Pragma("clang fp contract(off)")
#define RMX_LEARN_NOFMA_ATTR
#else
#define RMX_LEARN_NOFMA
#define RMX_LEARN_NOFMA_ATTR __attribute__((optimize("fp-contract=off")))
#endif

namespace rmx {

// The learner bound to a handle (rmx_learn_bind): caller-owned tables q / visits [A][N][S_max][4] float64, phi [A][Q]
// (the handle's copy; NULL without use_rsh).
struct LearnParams {
  double gamma, lr;  // lr == 0: 1 / visits
  double* q;
  double* visits;
  const double* phi;
  int64_t s_max;  // W * H * max_a enc_nq[a]
  int32_t use_qrm, use_rsh, trunc_is_terminal;
};

// The per-learner epsilon schedule bound by rmx_learn_eps_bind (include/rmx.h, "per-learner epsilon schedules"): the
// caller's column float64 [A][N], learner (a, e) at a * N + e, and QLearning's epsilon_end / epsilon_decay.  col == NULL:
// no schedule, the call's scalar epsilon (LearnCall::epsilon) serves every learner.
struct EpsParams {
  double* col;
  double end, decay;
};

// The learn kernels take the LambdaParams and the EpsParams as trailing arguments of their own, each only in the
// instantiations that use it (a pack, empty for the others): the argument of type T among them.
template <typename T, typename First, typename... Rest>
RMX_HD const T& learn_extra(const First& first, const Rest&... rest) {
  if constexpr (std::is_same_v<T, First>)
    return first;
  else
    return learn_extra<T>(rest...);
}

// Per-call arguments of a learn step.
struct LearnCall {
  double epsilon;
  int32_t policy;  // 0: the caller's actions; 1: the engine's policy; 2: the learners' numpy streams (both below)
  int32_t update;  // RMX_LEARN_UPDATE
  int32_t best;    // RMX_LEARN_BEST
  int32_t* actions_out;  // [A][N] or NULL (policy steps)
  uint64_t* rng;         // policy 2: the generator column bound by rmx_learn_rng_bind, [5][A][N]
};
enum { kLearnActions = 0, kLearnHash = 1, kLearnNumpy = 2 };  // LearnCall::policy

// update_q's arithmetic: a = (1 - lr) * cur; b = gamma * maxq; c = r + b; d = lr * c; new = a + d
RMX_LEARN_NOFMA_ATTR RMX_HD double learn_new_q(double cur, double r, double maxq, double gamma, double lr) {
  RMX_LEARN_NOFMA
  const double a = (1.0 - lr) * cur;
  const double b = gamma * maxq;
  const double c = r + b;
  const double d = lr * c;
  return a + d;
}

// 1 / visits, correctly rounded
RMX_LEARN_NOFMA_ATTR RMX_HD double learn_rate_of(double visits) {
  RMX_LEARN_NOFMA
  return 1.0 / visits;
}

// r + (gamma * Phi(next) - Phi(prev))
RMX_LEARN_NOFMA_ATTR RMX_HD double learn_shaped(double r, double gamma, double phi_next, double phi_prev) {
  RMX_LEARN_NOFMA
  const double g = gamma * phi_next;
  const double sh = g - phi_prev;
  return r + sh;
}

// Renv + reward_modifier * RQ of the wrapper's reward (rm_environment_wrapper.py:69, 92) in float64
RMX_LEARN_NOFMA_ATTR RMX_HD double learn_reward(float renv, float modifier, float rq) {
  RMX_LEARN_NOFMA
  const double m = (double)modifier * (double)rq;
  return (double)renv + m;
}

// learn_done_episode (qlearning.py:153-155): epsilon = max(epsilon_end, epsilon * epsilon_decay).  One multiply, then
// Python's max(end, x): x only where x > end (a NaN product gives end).
RMX_LEARN_NOFMA_ATTR RMX_HD double learn_eps_decay(double eps, double end, double decay) {
  RMX_LEARN_NOFMA
  const double x = eps * decay;
  return x > end ? x : end;
}

// env.reset()'s learn_done_episode of every agent's learner of env e (ma_frozen_lake.py:86-88, ma_office.py:107-108): a
// learn step's auto-reset, before the policy reads the column
RMX_HD void learn_eps_reset(const EpsParams& ep, int A, int64_t N, int64_t e) {
  for (int a = 0; a < A; ++a) {
    double* c = ep.col + (int64_t)a * N + e;
    *c = learn_eps_decay(*c, ep.end, ep.decay);
  }
}

// The epsilon learner (a, e) explores under in a policy step with a schedule bound: its column entry (one 8-B load,
// contiguous over a wave's envs), decayed and stored first when the step has just auto-reset the env.
RMX_HD double learn_eps_step(const EpsParams& ep, int a, int64_t N, int64_t e, bool was_reset) {
  double* c = ep.col + (int64_t)a * N + e;
  double eps = *c;
  if (was_reset) {
    eps = learn_eps_decay(eps, ep.end, ep.decay);
    *c = eps;
  }
  return eps;
}

RMX_HD double learn_max4(double a, double b, double c, double d) {  // np.max of a row
  double m = a;
  m = b > m ? b : m;
  m = c > m ? c : m;
  m = d > m ? d : m;
  return m;
}

// The engine's policy for agent i of global env eg at global step t (include/rmx.h, rmx_learn_step_policy), over the
// row of the state the step is about to leave.
RMX_HD int32_t learn_policy(uint64_t seed, int64_t t, int64_t n_global, int64_t eg, int A, int i, double epsilon,
                                  int best, double r0, double r1, double r2, double r3) {
  const double m = learn_max4(r0, r1, r2, r3);
  if (best) return r0 == m ? 0 : r1 == m ? 1 : r2 == m ? 2 : 3;  // np.argmax: the first maximum
  const uint64_t ctr = (((uint64_t)t * (uint64_t)n_global + (uint64_t)eg) * (uint64_t)A + (uint64_t)i) * kGolden;
  const uint64_t h0 = splitmix64(seed ^ ctr);
  const uint64_t h1 = splitmix64(h0);
  if ((double)(h1 >> 11) * 0x1p-53 < epsilon) return (int32_t)(h0 >> 62);
  const uint64_t h2 = splitmix64(h1);
  const int e0 = r0 == m, e1 = r1 == m, e2 = r2 == m, e3 = r3 == m;
  const uint64_t n_max = (uint64_t)(e0 + e1 + e2 + e3);
  int pick = (int)(((h2 >> 32) * n_max) >> 32);  // maximum number `pick`, in index order
  if (e0 && pick-- == 0) return 0;
  if (e1 && pick-- == 0) return 1;
  if (e2 && pick-- == 0) return 2;
  return 3;
}

// ---- the reference's own action stream: each learner's np.random.default_rng(seed) (learning_algorithm.py:32) as
// QLearning.choose_action draws from it (qlearning.py:112-143) --------------------------------------------------------
// Restated from numpy/random/src/pcg64/pcg64.h (pcg64_next64 / pcg64_next32: a 64-bit output serves two 32-bit draws,
// low half first, the high half buffered in has_uint32 / uinteger; next64 never touches the buffer),
// _generator.pyx (uniform(0, 1) = next_double; choice of a k-sequence = integers(0, k)) and distributions.c
// (random_bounded_uint64 -> buffered_bounded_lemire_uint32 for ranges below 2^32; a range of one value draws nothing).
struct LearnRng : Pcg {  // the generator (rmx_rules.h) and its 32-bit buffer
  uint32_t has, u;       // has_uint32, uinteger
};

// The bound column (rmx_learn_rng_bind): uint64 [5][A][N], word w of learner (a, e) at ((w * A + a) * N + e)
RMX_HD uint64_t learn_rng_word4(const LearnRng& r) { return ((uint64_t)r.has << 32) | r.u; }

// A learner's round trip over the column, around the policy's draws: w = col + a * N + e, plane = A * N, so the five
// words are plane-major and each is a coalesced 8-B access per lane.  The load reads all five; the store writes the
// two state words, and the buffer word only when it changed from w4 = learn_rng_word4 of the loaded generator (the
// increment never changes).  A policy step that draws nothing calls neither: the column is not touched.
RMX_HD LearnRng learn_rng_load(const uint64_t* w, int64_t plane) {
  const uint64_t w4 = w[4 * plane];
  return {{w[0], w[plane], w[2 * plane], w[3 * plane]}, (uint32_t)(w4 >> 32), (uint32_t)w4};
}
RMX_HD void learn_rng_store(uint64_t* w, int64_t plane, const LearnRng& r, uint64_t w4) {
  w[0] = r.hi;
  w[plane] = r.lo;
  const uint64_t n4 = learn_rng_word4(r);
  if (n4 != w4) w[4 * plane] = n4;
}

RMX_HD uint32_t learn_pcg_next32(LearnRng& r) {
  if (r.has) {
    r.has = 0;
    return r.u;
  }
  const uint64_t v = pcg_next64(r);
  r.has = 1;
  r.u = (uint32_t)(v >> 32);
  return (uint32_t)v;
}

// integers(0, k), 1 <= k < 2^32: Lemire's method on buffered 32-bit draws.  The threshold is 2^32 mod k: 0 for k = 2
// and 4, so of a row's tie counts only k = 3 can redraw, and only on a zero low half.
RMX_HD uint32_t learn_bounded(LearnRng& r, uint32_t k) {
  if (k == 1u) return 0u;
  uint64_t m = (uint64_t)learn_pcg_next32(r) * k;
  uint32_t left = (uint32_t)m;
  if (left < k) {
    const uint32_t thr = (0xFFFFFFFFu - (k - 1u)) % k;
    while (left < thr) {
      m = (uint64_t)learn_pcg_next32(r) * k;
      left = (uint32_t)m;
    }
  }
  return (uint32_t)(m >> 32);
}

// choose_action on the learner's own generator (include/rmx.h, RMX_LEARN_NUMPY), over the row of the state the step is
// about to leave.  The explore draw is taken whatever epsilon is; a row with no entry equal to its maximum (a NaN
// maximum, where the reference raises) gives action 3 without a further draw.
RMX_HD int32_t learn_policy_numpy(LearnRng& r, double epsilon, double r0, double r1, double r2, double r3) {
  const double d = (double)(pcg_next64(r) >> 11) * 0x1p-53;
  if (d < epsilon) return (int32_t)learn_bounded(r, 4u);
  const double m = learn_max4(r0, r1, r2, r3);
  const int e0 = r0 == m, e1 = r1 == m, e2 = r2 == m, e3 = r3 == m;
  const uint32_t n_max = (uint32_t)(e0 + e1 + e2 + e3);
  if (n_max == 0u) return 3;
  int pick = (int)learn_bounded(r, n_max);  // maximum number `pick`, in index order
  if (e0 && pick-- == 0) return 0;
  if (e1 && pick-- == 0) return 1;
  if (e2 && pick-- == 0) return 2;
  return 3;
}

// One 32-B table row: two 16-B loads on the device (the maximum is taken in registers, by whoever uses the row)
RMX_HD void learn_load_row(const double* row, double (&out)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const double2* r2 = reinterpret_cast<const double2*>(row);
  const double2 lo = r2[0], hi = r2[1];
  out[0] = lo.x, out[1] = lo.y, out[2] = hi.x, out[3] = hi.y;
#else
  out[0] = row[0], out[1] = row[1], out[2] = row[2], out[3] = row[3];
#endif
}

// One agent-step's outcome as the learner reads it (AgentOut, rmx_rules.h, and the RM state
// before and after the step).
struct LearnStep {
  uint32_t prev_cell, cell, ev;
  int32_t q_pre, q_post;
  bool env_term, term, trunc;
  float renv;
};

// The RM tables of one agent as the step reads them: next_q / rm_reward rows [Q][E] and the QRM state list.
struct LearnTables {
  const uint8_t* nq;   // agent a's [Q][E]
  const float* rr;     // agent a's [Q][E]
  const uint8_t* qrm;  // agent a's [Qx]
  const double* phi;   // agent a's [Q] or NULL
  int32_t E, n_qrm, enc_nq, final_q;
  float reward_modifier;
  int32_t Q;  // cfg.n_rm_states: the length of phi's row
};

// Experience j of one agent-step (qlearning.py:82-108): its table rows s / sn, reward and done flag.  use_qrm: the
// counterfactual of RM state j of get_all_states()[:-1]; else the one real transition (j == 0).  False when there is no
// such experience, or its state falls outside the agent's S = W * H * enc_nq rows (columns a caller overwrote out of
// range): such an experience is dropped, never written.  In such a state the kernel's event and successor come from
// table bytes outside the agent's own, so nq_j can be any byte: it is checked before it indexes phi (global memory).
struct LearnExp {
  int64_t s, sn;
  double r;
  bool done;
};
RMX_HD int learn_n_exp(const LearnParams& lp, const LearnTables& T) { return lp.use_qrm ? T.n_qrm : 1; }
RMX_HD bool learn_experience(const LearnParams& lp, const LearnTables& T, const LearnStep& o, int j, int64_t S,
                                   LearnExp& x) {
  const int32_t nQ = T.enc_nq;
  if (lp.use_qrm) {
    if (j >= T.n_qrm) return false;
    const uint32_t qj = T.qrm[j];
    const uint32_t tj = qj * (uint32_t)T.E + o.ev;
    const int32_t nqj = T.nq[tj];
    x.s = (int64_t)o.prev_cell * nQ + (int64_t)qj;
    x.sn = (int64_t)o.cell * nQ + nqj;
    x.r = learn_reward(o.renv, 1.0f, T.rr[tj]);  // the raw RM reward (rm_environment_wrapper.py:171)
    if (lp.use_rsh) {
      if ((uint32_t)nqj >= (uint32_t)T.Q) return false;
      x.r = learn_shaped(x.r, lp.gamma, T.phi[nqj], T.phi[qj]);
    }
    x.done = o.env_term || nqj == T.final_q;
  } else {
    if (j != 0) return false;
    x.s = (int64_t)o.prev_cell * nQ + o.q_pre;
    x.sn = (int64_t)o.cell * nQ + o.q_post;
    x.r = learn_reward(o.renv, T.reward_modifier, T.rr[(uint32_t)o.q_pre * (uint32_t)T.E + o.ev]);
    x.done = o.term || (lp.trunc_is_terminal && o.trunc);
  }
  return (uint64_t)x.s < (uint64_t)S && (uint64_t)x.sn < (uint64_t)S;
}

// update_q (qlearning.py:70-79) of one experience on learner table qa / va ([S_max][4], one (agent, env)): three
// independent loads (the entry, its visit count, the next state's row unless done), then the two stores
RMX_HD void learn_update_q(const LearnParams& lp, double* qa, double* va, const LearnExp& x, int k) {
  const int64_t i = x.s * 4 + k;
  const double cur = qa[i];
  double lr = lp.lr;
  if (va) {
    const double v = va[i] + 1.0;
    va[i] = v;
    if (lr == 0.0) lr = learn_rate_of(v);
  }
  double maxq = 0.0;
  if (!x.done) {
    double row[4];
    learn_load_row(qa + x.sn * 4, row);
    maxq = learn_max4(row[0], row[1], row[2], row[3]);  // np.max of the row
  }
  qa[i] = learn_new_q(cur, x.r, maxq, lp.gamma, lr);
}

// Every experience of one agent-step, strictly in order on the one table.  k: the action's table column (0..3).
RMX_HD void learn_agent(const LearnParams& lp, const LearnTables& T, const LearnStep& o, double* qa, double* va,
                              int k, int64_t S) {
  const int n = learn_n_exp(lp, T);
  for (int j = 0; j < n; ++j) {
    LearnExp x;
    if (learn_experience(lp, T, o, j, S, x)) learn_update_q(lp, qa, va, x, k);
  }
}

// ---- Watkins Q(lambda) with replacing traces: QLearningLambda.update (learning_algorithms/qlearning_lambda.py:33-84)
// behind AgentRL.update_policy, which never passes next_action: the next action is then the argmax, always greedy, so
// the traces always decay and are never cut (include/rmx.h, "Watkins Q(lambda) learners").
// The reference's e_table is dense and every update sweeps the whole table; here each learner keeps the list of its
// live traces.  Adding c * 0.0 leaves a float64 unchanged for every finite c and every value but -0.0, so the list
// gives the dense update's tables bit for bit.
// The lists bound by rmx_learn_lambda_bind, slot-major: slot j of learner (a, e) at (a * cap + j) * N + e, so that with
// one thread per env a wave's read of slot j is one contiguous run.  Invariant: slots 0 .. cnt - 1 hold distinct cell
// indices i = s * 4 + k, each with a trace that is not 0: a cell is listed iff its dense e would be non-zero.
struct LambdaParams {
  double lambd;
  int32_t* idx;  // [A][cap][N]
  double* val;   // [A][cap][N]
  int32_t* cnt;  // [A][N]
  int32_t cap;
};

// How many list slots one sweep step has in flight.  The read-modify-writes of one list hit distinct cells, so a batch
// is B independent gathers (a wave: 64 * B lines) and B independent scatters, not a chain of dependent round trips.
// Four keeps the kernel's registers where the eight-agent bucket can still hold its agents; the lists of this workload
// are a few tens of entries long, so deeper batches would mostly run empty.
enum { kLambdaBatch = 4 };
// the bit of the handle's error word a full list raises (bit 0: an invalid action); rmx_check_errors: RMX_E_TRACE
enum : uint32_t { kErrTraceFull = 2u };

// c = lr * td, td = (r + gamma * best) - cur: three operations, then the scalar product numpy forms first
RMX_LEARN_NOFMA_ATTR RMX_HD double learn_lambda_c(double cur, double r, double best, double gamma, double lr) {
  RMX_LEARN_NOFMA
  const double b = gamma * best;
  const double t = r + b;
  const double td = t - cur;
  return lr * td;
}

// q + (c * e)
RMX_LEARN_NOFMA_ATTR RMX_HD double learn_lambda_add(double q, double c, double e) {
  RMX_LEARN_NOFMA
  const double d = c * e;
  return q + d;
}

RMX_LEARN_NOFMA_ATTR RMX_HD double learn_lambda_mul(double a, double b) {
  RMX_LEARN_NOFMA
  return a * b;
}

// One update of learner table qa / va over its list (ti / tv: slot 0 of the learner, `stride` elements between slots;
// *tc its length).  Returns true when the cell's trace found the list full: the cell's own update is applied, the trace
// is not kept, and nothing is written at or past slot cap.
RMX_HD bool learn_lambda_update(const LearnParams& lp, double lambd, int32_t cap, double* qa, double* va,
                                const LearnExp& x, int k, int32_t* ti, double* tv, int64_t stride, int32_t* tc) {
  const int64_t i = x.s * 4 + k;
  // 1. the entry, its visit count, the next state's row: read before any write of this update
  const double cur = qa[i];
  double lr = lp.lr;
  if (va) {
    const double v = va[i] + 1.0;
    va[i] = v;
    if (lr == 0.0) lr = learn_rate_of(v);
  }
  double best = 0.0;
  if (!x.done) {
    double row[4];
    learn_load_row(qa + x.sn * 4, row);
    best = learn_max4(row[0], row[1], row[2], row[3]);
  }
  // 2. c and g
  const double c = learn_lambda_c(cur, x.r, best, lp.gamma, lr);
  const double g = learn_lambda_mul(lp.gamma, lambd);
  // 3.-6. one sweep, kLambdaBatch slots at a time: the slot of cell i takes 1.0 first, every slot adds c * val to its
  // cell, and unless done the decayed traces that are not 0 are written back compacted, in order (slot w <= j: a
  // write never lands on a slot still to be read)
  const int32_t n = *tc < cap ? (*tc > 0 ? *tc : 0) : cap;  // (a count the caller did not zero reads no slot past cap)
  int32_t w = 0;
  bool found = false;
  for (int32_t j0 = 0; j0 < n; j0 += kLambdaBatch) {
    int32_t ci[kLambdaBatch];
    double cv[kLambdaBatch], cq[kLambdaBatch];
    RMX_UNROLL
    for (int b = 0; b < kLambdaBatch; ++b)
      if (j0 + b < n) {
        ci[b] = ti[(int64_t)(j0 + b) * stride];
        cv[b] = tv[(int64_t)(j0 + b) * stride];
      }
    RMX_UNROLL
    for (int b = 0; b < kLambdaBatch; ++b)
      if (j0 + b < n) cq[b] = qa[ci[b]];
    RMX_UNROLL
    for (int b = 0; b < kLambdaBatch; ++b)
      if (j0 + b < n) {
        if (ci[b] == (int32_t)i) {
          cv[b] = 1.0;
          found = true;
        }
        qa[ci[b]] = learn_lambda_add(cq[b], c, cv[b]);
        if (!x.done) {
          const double d = learn_lambda_mul(cv[b], g);
          if (d != 0.0) {  // a trace that reached exactly 0 is dropped
            ti[(int64_t)w * stride] = ci[b];
            tv[(int64_t)w * stride] = d;
            ++w;
          }
        }
      }
  }
  // 7. a cell that was not listed: its own update with trace 1.0, and the decayed trace appended
  bool full = false;
  if (!found) {
    qa[i] = learn_lambda_add(cur, c, 1.0);
    if (!x.done && g != 0.0) {
      if (w < cap) {
        ti[(int64_t)w * stride] = (int32_t)i;
        tv[(int64_t)w * stride] = g;
        ++w;
      } else {
        full = true;
      }
    }
  }
  // 8. terminated: every trace of this learner becomes 0
  *tc = x.done ? 0 : w;
  return full;
}

// The one experience of an agent-step under Q(lambda) (no QRM, no shaping: update ignores info).  k: the action's
// table column.  An experience outside the agent's rows touches neither the tables nor the list.
RMX_HD bool learn_lambda_agent(const LearnParams& lp, const LambdaParams& lam, const LearnTables& T,
                               const LearnStep& o, double* qa, double* va, int k, int64_t S, int a, int64_t N,
                               int64_t e) {
  LearnExp x;
  if (!learn_experience(lp, T, o, 0, S, x)) return false;
  const int64_t slot0 = (int64_t)a * lam.cap * N + e;
  return learn_lambda_update(lp, lam.lambd, lam.cap, qa, va, x, k, lam.idx + slot0, lam.val + slot0, N,
                             lam.cnt + (int64_t)a * N + e);
}

}  // namespace rmx
