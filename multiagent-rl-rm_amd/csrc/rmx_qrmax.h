// rmx_qrmax.h — the QR-max learner's rules, one source for the gfx950 kernels (rmx_learn_qrmax.hip) and the host path
// (rmx_hoststep.cpp): the experiences of one agent-step with the environment and the RM reward apart, one update of
// the factored model with its known test, one (s, q, a) Bellman backup and its change, the sequential solve, and the
// policy.  Plain C++, as rmx_rmax.h (whose worklist, error bit and row helpers it uses).
//
// Reference semantics restated (paths relative to Alee08/multiagent-rl-rm):
//   update            learning_algorithms/qrmax_v2.py:414-506 (the real experience, then with use_qrm every
//                     counterfactual of rm_environment_wrapper.py:140-183 with the same action and Renv; each:
//                     update_RSQA_RSA, update_TQS_RQS, check_known; ONE solve_VI behind the last experience when any of
//                     them made something known)
//   check_known       qrmax_v2.py:508-600 (knownTSQA first: its own count, or the shortcut over flags set by EARLIER
//                     calls; then knownTSA, knownTQS, knownRSA, knownRQS)
//   solve_VI          qrmax_v2.py:265-338 (final rows zeroed here; Jacobi sweeps over the known, non-final (s, q, a)
//                     while the largest change of the last sweep exceeds VI_delta; Q = Qnew after every sweep)
//   choose_action     qrmax_v2.py:216-232 (rng.shuffle of the four actions on every call; a flat row, unless best:
//                     rng.choice of the shuffled list; else np.argmax)
// s is the position index y * W + x, q the RM state index; Q[s, q, a] is the bound table's q[(s * nQ + q) * 4 + a].
// With thresholds >= 1 every known flag but knownTSQA equals count >= threshold between two experiences (a count
// stops at its threshold, and check_known tests exactly the pairs the update just counted), so only knownTSQA is
// stored.  The environment model is per (position, action): counts, reward sums and the successors of (s, a) as a list
// in first-seen order (nTSAS_dict's order, which solve_VI sums in).  The RM model is per (RM state, next position),
// indexed by the encoded state s1 * nQ + q; its single successor (the RM is deterministic) is tq_next.
// Every operation is one IEEE float64 operation, never fused (RMX_LEARN_NOFMA); sums start from +0.0 in list order.
#pragma once
#include <stdint.h>

#include "rmx_learn.h"
#include "rmx_rmax.h"

namespace rmx {

// The model bound by rmx_learn_qrmax_bind beside the learner's q / visits (visits serves as nTSQA).  P = W * H.
struct QRMaxParams {
  double delta;                        // VI_delta
  int32_t delta_rel;                   // VI_delta_rel
  int32_t max_iter;                    // sweeps of one solve at most
  int32_t n_te, n_re, n_tq, n_rq;      // nsamplesTE / RE / TQ / RQ
  int32_t cap;                         // bound slots per (s, a)
  int32_t P;                           // positions W * H
  uint8_t* known_tsqa;                 // [A][N][S_max][4]
  int32_t* n_tsa;                      // [A][N][P][4]
  int32_t* n_rsa;                      // [A][N][P][4]
  double* sum_rsa;                     // [A][N][P][4]
  int32_t* succ_idx;                   // [A][N][P][4][cap]
  int32_t* succ_cnt;                   // [A][N][P][4][cap]
  int32_t* n_tqs;                      // [A][N][S_max], at s1 * nQ + q
  int32_t* tq_next;                    // [A][N][S_max]
  int32_t* n_rqs;                      // [A][N][S_max]
  double* sum_rqs;                     // [A][N][S_max]
  uint8_t* fin;                        // [A][N][S_max]: (s, q) seen as the next state of a done experience
};

// what qrmax_update reports
enum { kQRMaxNew = 1, kQRMaxFull = 2 };
// The successors one (s, a) can have on any world of the engine: the cell itself and its four neighbours (include/rmx.h,
// "R-max learners": the derivation, with positions in place of encoded states)
enum { kQRMaxSlotsFull = 5 };

// One learner's slices
struct QRMaxLearner {
  double* q;       // [S_max][4]
  double* n_tsqa;  // [S_max][4]
  uint8_t* known;  // [S_max][4]
  int32_t* n_tsa;  // [P][4]
  int32_t* n_rsa;
  double* sum_rsa;
  int32_t* idx;    // [P][4][cap]
  int32_t* cnt;
  int32_t* n_tqs;  // [S_max]
  int32_t* tq_next;
  int32_t* n_rqs;
  double* sum_rqs;
  uint8_t* fin;
};

RMX_HD QRMaxLearner qrmax_learner(const LearnParams& lp, const QRMaxParams& qp, int64_t learner) {
  const int64_t bq = learner * lp.s_max * 4, bp = learner * qp.P * 4, bs = learner * lp.s_max;
  return {lp.q + bq,         lp.visits + bq,    qp.known_tsqa + bq,         qp.n_tsa + bp,  qp.n_rsa + bp,
          qp.sum_rsa + bp,   qp.succ_idx + bp * qp.cap, qp.succ_cnt + bp * qp.cap, qp.n_tqs + bs, qp.tq_next + bs,
          qp.n_rqs + bs,     qp.sum_rqs + bs,   qp.fin + bs};
}

// Experience j of one agent-step as QR-max sees it: j == 0 the real one (Renv; RQ = reward_modifier * the RM reward;
// the done rule of trunc_is_terminal), then with use_qrm counterfactual j - 1 (the same Renv, the raw RM reward, done =
// env_term or rm_done).  Which experiences exist and their done flag are learn_experience's (rmx_learn.h); here the two
// rewards stay apart and the indices stay unencoded.  False past the last experience, or when a position or an RM
// index falls outside the agent's own (columns a caller overwrote out of range): such an experience is dropped.
struct QRMaxExp {
  int32_t s, q, s1, q1;
  double re, rq;
  bool done;
};
RMX_HD int qrmax_n_exp(const LearnParams& lp, const LearnTables& T) { return 1 + (lp.use_qrm ? T.n_qrm : 0); }

RMX_LEARN_NOFMA_ATTR RMX_HD double qrmax_rq(float modifier, float rq) {
  RMX_LEARN_NOFMA
  return (double)modifier * (double)rq;
}

RMX_HD bool qrmax_experience(const LearnParams& lp, const LearnTables& T, const LearnStep& o, int j, int32_t P,
                             QRMaxExp& x) {
  LearnParams one = lp;
  one.use_rsh = 0;
  LearnExp e;
  const int64_t S = (int64_t)P * T.enc_nq;
  uint32_t q, q1;
  if (j == 0) {
    one.use_qrm = 0;
    if (!learn_experience(one, T, o, 0, S, e)) return false;
    q = (uint32_t)o.q_pre;
    q1 = (uint32_t)o.q_post;
    x.rq = qrmax_rq(T.reward_modifier, T.rr[q * (uint32_t)T.E + o.ev]);
  } else {
    if (!learn_experience(one, T, o, j - 1, S, e)) return false;
    q = T.qrm[j - 1];
    const uint32_t tj = q * (uint32_t)T.E + o.ev;
    q1 = T.nq[tj];
    x.rq = (double)T.rr[tj];
  }
  if (o.prev_cell >= (uint32_t)P || o.cell >= (uint32_t)P || q >= (uint32_t)T.enc_nq || q1 >= (uint32_t)T.enc_nq)
    return false;
  x.s = (int32_t)o.prev_cell;
  x.s1 = (int32_t)o.cell;
  x.q = (int32_t)q;
  x.q1 = (int32_t)q1;
  x.re = (double)o.renv;
  x.done = e.done;
  return true;
}

RMX_LEARN_NOFMA_ATTR RMX_HD double qrmax_add(double a, double b) {
  RMX_LEARN_NOFMA
  return a + b;
}

// One experience with action column k: update_RSQA_RSA, update_TQS_RQS, check_known, in the reference's order.
// kQRMaxNew: something became known (the solve is the caller's, once, behind the agent-step's last experience);
// kQRMaxFull: the successor found the list of (s, a) full (counted in n_tsa, its entry dropped; nothing is written at
// or past cap).  A listed successor outside the positions (arrays the caller did not zero) is read as not known.
RMX_HD int qrmax_update(const QRMaxParams& qp, const QRMaxLearner& L, int32_t nQ, const QRMaxExp& x, int k) {
  const int32_t cap = qp.cap;
  const int64_t sq = (int64_t)x.s * nQ + x.q, i = sq * 4 + k, sa = (int64_t)x.s * 4 + k;
  const int64_t qs1 = (int64_t)x.s1 * nQ + x.q, sn = (int64_t)x.s1 * nQ + x.q1;
  int res = 0;
  if (x.done) L.fin[sn] = 1;  // (its row is zeroed by the next solve, not here)
  // the flags as the reference holds them when this experience arrives
  const bool k_tsqa = L.known[i] != 0;
  const bool k_tsa = L.n_tsa[sa] >= qp.n_te, k_rsa = L.n_rsa[sa] >= qp.n_re;
  const bool k_tqs = L.n_tqs[qs1] >= qp.n_tq, k_rqs = L.n_rqs[qs1] >= qp.n_rq;
  int32_t* si = L.idx + sa * cap;
  int32_t* sc = L.cnt + sa * cap;
  // update_RSQA_RSA
  double n_sqa = L.n_tsqa[i];
  if (!k_tsqa) {
    n_sqa = qrmax_add(n_sqa, 1.0);
    L.n_tsqa[i] = n_sqa;
  }
  int32_t n_sa = L.n_tsa[sa];
  if (!k_tsa) {
    int32_t j = 0;
    for (; j < cap; ++j)
      if (sc[j] == 0 || si[j] == x.s1) break;
    if (j < cap) {
      if (sc[j] == 0) si[j] = x.s1;
      sc[j] += 1;
    } else {
      res |= kQRMaxFull;
    }
    n_sa += 1;
    L.n_tsa[sa] = n_sa;
  }
  int32_t n_ra = L.n_rsa[sa];
  if (!k_rsa) {
    n_ra += 1;
    L.n_rsa[sa] = n_ra;
    L.sum_rsa[sa] = qrmax_add(L.sum_rsa[sa], x.re);
  }
  // update_TQS_RQS
  int32_t n_qs = L.n_tqs[qs1];
  if (!k_tqs) {
    n_qs += 1;
    L.n_tqs[qs1] = n_qs;
    L.tq_next[qs1] = x.q1;
  }
  int32_t n_rq = L.n_rqs[qs1];
  if (!k_rqs) {
    n_rq += 1;
    L.n_rqs[qs1] = n_rq;
    L.sum_rqs[qs1] = qrmax_add(L.sum_rqs[qs1], x.rq);
  }
  // check_known: knownTSQA first, over the flags earlier calls have set (this call's own crossings come after it)
  if (!k_tsqa) {
    bool known = n_sqa >= (double)qp.n_te;
    if (!known && k_tsa) {  // the shortcut: (s, a) known and (q, s') known for every listed successor s'
      known = true;
      for (int32_t j = 0; j < cap && sc[j] != 0; ++j) {
        const int32_t ss1 = si[j];
        bool kq = false;
        if ((uint32_t)ss1 < (uint32_t)qp.P) kq = ss1 == x.s1 ? k_tqs : L.n_tqs[(int64_t)ss1 * nQ + x.q] >= qp.n_tq;
        if (!kq) known = false;
      }
    }
    if (known) {
      L.known[i] = 1;
      res |= kQRMaxNew;
    }
  }
  if ((!k_tsa && n_sa >= qp.n_te) || (!k_tqs && n_qs >= qp.n_tq) || (!k_rsa && n_ra >= qp.n_re) ||
      (!k_rqs && n_rq >= qp.n_rq))
    res |= kQRMaxNew;
  return res;
}

// Does solve_VI back (s, q, a) up?  known(s, q, a) and (s, q) not final.  i = (s * nQ + q) * 4 + a, sa = s * 4 + a.
RMX_HD bool qrmax_solved_entry(const QRMaxParams& qp, const QRMaxLearner& L, int64_t i, int64_t sa) {
  return L.known[i] != 0 && !L.fin[i >> 2] && L.n_tsa[sa] >= qp.n_te && L.n_rsa[sa] >= qp.n_re;
}

// One (s, q, a) backup over v = max_a Q_old (qrmax_v2.py:292-327).  For every listed s1 of (s, a), in list order, whose
// (q, s1) has been observed: tr = (nTQSQ / nTQS) * Pssa, the first factor n / n = 1.0 exactly, so tr = Pssa.  A
// successor whose (q, s1) was never observed contributes nothing (its mass is dropped).
RMX_LEARN_NOFMA_ATTR RMX_HD double qrmax_backup(const QRMaxParams& qp, double gamma, const QRMaxLearner& L, int32_t nQ,
                                                int32_t q, int64_t sa, const double* v) {
  RMX_LEARN_NOFMA
  const int32_t cap = qp.cap;
  const double n_sa = (double)L.n_tsa[sa];
  const double rsa = L.sum_rsa[sa] / (double)L.n_rsa[sa];
  const int32_t* si = L.idx + sa * cap;
  const int32_t* sc = L.cnt + sa * cap;
  double qq1 = 0.0, qq2 = 0.0;
  for (int32_t j = 0; j < cap; ++j) {
    const int32_t c = sc[j];
    if (c == 0) break;
    const int32_t s1 = si[j];
    if ((uint32_t)s1 >= (uint32_t)qp.P) continue;  // (arrays the caller did not zero)
    const int64_t e = (int64_t)s1 * nQ + q;
    if (L.n_tqs[e] <= 0) continue;
    const int32_t q1 = L.tq_next[e];
    if ((uint32_t)q1 >= (uint32_t)nQ) continue;
    const double tr = (double)c / n_sa;
    const int32_t nr = L.n_rqs[e];
    double rqs = 0.0;
    if (nr > 0) rqs = L.sum_rqs[e] / (double)nr;
    const double r = rsa + rqs;
    const double t1 = tr * r;
    qq1 = qq1 + t1;
    const double t2 = tr * v[(int64_t)s1 * nQ + q1];
    qq2 = qq2 + t2;
  }
  const double g = gamma * qq2;
  return qq1 + g;
}

// cdelta of one entry (qrmax_v2.py:329-332): |new - old|, under delta_rel divided by m = |max(new, old)| where m > 0
// (Python's max: old only where old > new).  The sweep goes on when some cdelta > VI_delta; a NaN never is.
RMX_LEARN_NOFMA_ATTR RMX_HD double qrmax_delta(double nw, double old, int delta_rel) {
  RMX_LEARN_NOFMA
  double d = nw - old;
  d = d < 0.0 ? -d : d;
  if (delta_rel) {
    double m = old > nw ? old : nw;
    m = m < 0.0 ? -m : m;
    if (m > 0.0) d = d / m;
  }
  return d;
}

// solve_VI (qrmax_v2.py:265-338) of one learner over its S = P * nQ rows, strictly sequential: the host path's solve,
// and the statement the solve kernel's sweeps are checked against.  An entry reads v (the old values) and its own old
// value only, so the new value is stored in place.  v: scratch of S doubles.  Returns the sweeps made.
inline int qrmax_solve(const QRMaxParams& qp, double gamma, const QRMaxLearner& L, int32_t nQ, double* v) {
  const int64_t S = (int64_t)qp.P * nQ;
  for (int64_t n = 0; n < S; ++n)
    if (L.fin[n]) L.q[n * 4] = L.q[n * 4 + 1] = L.q[n * 4 + 2] = L.q[n * 4 + 3] = 0.0;
  int it = 0;
  bool more = 1.0 > qp.delta;  // delta = 1.0 before the first sweep
  while (more && it < qp.max_iter) {
    for (int64_t n = 0; n < S; ++n) v[n] = learn_max4(L.q[n * 4], L.q[n * 4 + 1], L.q[n * 4 + 2], L.q[n * 4 + 3]);
    more = false;
    for (int64_t i = 0; i < S * 4; ++i) {
      const int64_t sq = i >> 2;
      const int64_t sa = (sq / nQ) * 4 + (i & 3);
      if (!qrmax_solved_entry(qp, L, i, sa)) continue;
      const double nw = qrmax_backup(qp, gamma, L, nQ, (int32_t)(sq % nQ), sa, v);
      if (qrmax_delta(nw, L.q[i], qp.delta_rel) > qp.delta) more = true;
      L.q[i] = nw;
    }
    ++it;
  }
  return it;
}

// ---- the policy (qrmax_v2.py:216-232) ---------------------------------------------------------------------------------
// RMX_LEARN_NUMPY: every call shuffles the list of the four actions first (numpy's untyped Fisher-Yates: for i = 3, 2, 1
// swap a[i] with a[random_interval(i)], buffered 32-bit draws masked to the smallest all-ones mask >= i and rejected
// while > i; rmx_device.h states the same rule for the random starts), under best too.  A flat row, unless best:
// rng.choice(actions) = the shuffled list at integers(0, 4).  Else np.argmax.  (The engine's hashed policy is
// rmax_policy's: a flat row takes the hash pick, nothing is drawn.)
RMX_HD int32_t qrmax_policy_numpy(LearnRng& r, int best, double r0, double r1, double r2, double r3) {
  uint32_t list = 0x3210u;  // the list, four bits per entry (no indexed array in a kernel's registers)
  for (uint32_t i = 3; i >= 1; --i) {
    const uint32_t mask = i | (i >> 1);
    uint32_t j;
    while ((j = learn_pcg_next32(r) & mask) > i) {
    }
    const uint32_t vi = (list >> (4 * i)) & 15u, vj = (list >> (4 * j)) & 15u;
    list &= ~((15u << (4 * i)) | (15u << (4 * j)));
    list |= (vj << (4 * i)) | (vi << (4 * j));
  }
  if (!best && rmax_row_flat(r0, r1, r2, r3)) return (int32_t)((list >> (4 * learn_bounded(r, 4u))) & 15u);
  return rmax_argmax(r0, r1, r2, r3);
}

}  // namespace rmx
