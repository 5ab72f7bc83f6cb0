// rmx_rmax.h — the R-max learner's rules, one source for the gfx950 kernels (rmx_learn_rmax.hip) and the host path
// (rmx_hoststep.cpp): update_q on the learned model, the successor-list insert, one (s, k) Bellman backup and its
// convergence test, and the policy.  Plain C++, as rmx_learn.h (whose experiences, row maximum and generator it uses).
//
// Reference semantics restated (paths relative to Alee08/multiagent-rl-rm):
//   update_q          learning_algorithms/rmax.py:156-170 (a terminal next state becomes a known zero-valued self loop;
//                     a pair below s_a_threshold takes the reward, the count and the successor; the observation that
//                     reaches the threshold solves the learned MDP at once)
//   experiences       rmax.py:174-181 (the real one first, then with use_qrm every counterfactual of
//                     rm_environment_wrapper.py:140-183, the RM state actually held included once more)
//   value_iteration   rmax.py:185-227 (mask = counts >= threshold; new = rewards / counts + gamma * einsum(T / counts,
//                     max_a q); convergence tested before the write; q[mask] = new[mask], a Jacobi sweep)
//   choose_action     rmax.py:108-128 (a row of four equal entries, unless best: rng.choice of the four actions; else
//                     np.argmax)
// The reference's dense transitions[s][k][:] is kept as the list of its non-zero entries in first-seen order
// (succ_idx / succ_cnt, learner-major [A][N][S_max][4][cap]; a slot with succ_cnt == 0 is empty).  Adding 0.0 changes
// no float64 but -0.0, and the sum below starts from +0.0, so the dense einsum over n is the sum of the listed terms.
// Every operation is one IEEE float64 operation, never fused (RMX_LEARN_NOFMA).
#pragma once
#include <stdint.h>

#include "rmx_learn.h"

namespace rmx {

// The model bound by rmx_learn_rmax_bind beside the learner's q / visits (visits serves as s_a_counts).
struct RMaxParams {
  double delta;          // VI_delta
  int32_t delta_rel;     // VI_delta_rel
  int32_t max_iter;      // sweeps of one solve at most
  int32_t threshold;     // s_a_threshold
  int32_t cap;           // bound slots per (s, k)
  double* rsum;          // [A][N][S_max][4]
  int32_t* succ_idx;     // [A][N][S_max][4][cap]
  int32_t* succ_cnt;     // [A][N][S_max][4][cap]
};

// the bit of the handle's error word a full successor list raises; rmx_check_errors: RMX_E_MODEL
enum : uint32_t { kErrModelFull = 4u };
// what rmax_update_q reports
enum { kRMaxCross = 1, kRMaxFull = 2 };
// The successors one (s, k) can have on any world of the engine (include/rmx.h, "R-max learners": the derivation)
enum { kRMaxSlotsFull = 5 };

// One learner's slices: q / counts / rsum [S_max][4], the lists [S_max][4][cap]
struct RMaxLearner {
  double* q;
  double* counts;
  double* rsum;
  int32_t* idx;
  int32_t* cnt;
};

RMX_HD RMaxLearner rmax_learner(const LearnParams& lp, const RMaxParams& rp, int64_t learner) {
  const int64_t base = learner * lp.s_max * 4;
  return {lp.q + base, lp.visits + base, rp.rsum + base, rp.succ_idx + base * rp.cap, rp.succ_cnt + base * rp.cap};
}

// Experience j of one agent-step as R-max sees it: j == 0 the real one (the wrapper's reward, the done rule of
// trunc_is_terminal), then with use_qrm counterfactual j - 1 (learn_experience, rmx_learn.h).  `valid`: inside the
// agent's rows (an experience outside them is dropped).  Returns false past the last experience.
RMX_HD int rmax_n_exp(const LearnParams& lp, const LearnTables& T) { return 1 + (lp.use_qrm ? T.n_qrm : 0); }
RMX_HD bool rmax_experience(const LearnParams& lp, const LearnTables& T, const LearnStep& o, int j, int64_t S,
                            LearnExp& x) {
  LearnParams one = lp;
  one.use_rsh = 0;
  if (j == 0) {
    one.use_qrm = 0;
    return learn_experience(one, T, o, 0, S, x);
  }
  return learn_experience(one, T, o, j - 1, S, x);
}

RMX_LEARN_NOFMA_ATTR RMX_HD double rmax_add(double a, double b) {
  RMX_LEARN_NOFMA
  return a + b;
}

// update_q (rmax.py:156-170) of one experience with action column k.  kRMaxCross: the pair reached the threshold with
// this observation (the count is stored, the solve is the caller's, before the next experience); kRMaxFull: the
// successor found its list full (counted in counts and rsum, its list entry dropped; nothing written at or past cap).
RMX_HD int rmax_update_q(const RMaxParams& rp, const RMaxLearner& L, const LearnExp& x, int k) {
  const double thr = (double)rp.threshold;
  const int32_t cap = rp.cap;
  if (x.done) {  // the terminal next state: q = 0, a known self loop; rsum is left alone
    for (int c = 0; c < 4; ++c) {
      const int64_t i = x.sn * 4 + c;
      L.q[i] = 0.0;
      L.counts[i] = thr;
      L.idx[i * cap] = (int32_t)x.sn;
      L.cnt[i * cap] = rp.threshold;
      for (int32_t j = 1; j < cap; ++j) L.cnt[i * cap + j] = 0;
    }
  }
  const int64_t i = x.s * 4 + k;
  const double c0 = L.counts[i];
  if (!(c0 < thr)) return 0;
  L.rsum[i] = rmax_add(L.rsum[i], x.r);
  const double c1 = rmax_add(c0, 1.0);
  L.counts[i] = c1;
  int res = c1 == thr ? kRMaxCross : 0;
  int32_t* si = L.idx + i * cap;
  int32_t* sc = L.cnt + i * cap;
  int32_t j = 0;
  for (; j < cap; ++j)
    if (sc[j] == 0 || si[j] == (int32_t)x.sn) break;
  if (j < cap) {
    if (sc[j] == 0) si[j] = (int32_t)x.sn;
    sc[j] += 1;
  } else {
    res |= kRMaxFull;
  }
  return res;
}

// One (s, k) Bellman backup over v = max_a q (rmax.py:210-212): rsum / counts + gamma * sum_slots (cnt / counts) * v
RMX_LEARN_NOFMA_ATTR RMX_HD double rmax_backup(double gamma, int32_t cap, double rsum, double count, const int32_t* si,
                                               const int32_t* sc, const double* v) {
  RMX_LEARN_NOFMA
  const double rm = rsum / count;
  double acc = 0.0;
  for (int32_t j = 0; j < cap; ++j) {
    const int32_t c = sc[j];
    if (c == 0) break;
    const double p = (double)c / count;
    const double t = p * v[si[j]];
    acc = acc + t;
  }
  const double g = gamma * acc;
  return rm + g;
}

// Has this entry converged (rmax.py:215-223)?  |q - new| < delta, the difference divided by |q| under delta_rel where
// q != 0 and taken as 0 where q == 0.  (A NaN difference has not converged.)
RMX_LEARN_NOFMA_ATTR RMX_HD bool rmax_converged(double q, double nw, double delta, int delta_rel) {
  RMX_LEARN_NOFMA
  double d = q - nw;
  d = d < 0.0 ? -d : d;
  if (delta_rel) {
    if (q == 0.0) return 0.0 < delta;
    const double aq = q < 0.0 ? -q : q;
    d = d / aq;
  }
  return d < delta;
}

// value_iteration (rmax.py:185-227) of one learner over its S rows, strictly sequential: the host path's solve, and
// the statement the solve kernel's sweeps are checked against.  v / nw: scratch of S and 4 * S doubles.  Returns the
// sweeps made (the converging one included).
inline int rmax_solve(const RMaxParams& rp, double gamma, const RMaxLearner& L, int64_t S, double* v, double* nw) {
  const double thr = (double)rp.threshold;
  int it = 0;
  while (it < rp.max_iter) {
    ++it;
    for (int64_t n = 0; n < S; ++n) v[n] = learn_max4(L.q[n * 4], L.q[n * 4 + 1], L.q[n * 4 + 2], L.q[n * 4 + 3]);
    bool conv = true;
    for (int64_t i = 0; i < S * 4; ++i) {
      if (!(L.counts[i] >= thr)) continue;
      nw[i] = rmax_backup(gamma, rp.cap, L.rsum[i], L.counts[i], L.idx + i * rp.cap, L.cnt + i * rp.cap, v);
      conv = conv && rmax_converged(L.q[i], nw[i], rp.delta, rp.delta_rel);
    }
    if (conv) break;
    for (int64_t i = 0; i < S * 4; ++i)
      if (L.counts[i] >= thr) L.q[i] = nw[i];
  }
  return it;
}

// ---- the device learn step's hand-over (rmx_learn_rmax.hip): engine-owned, allocated by rmx_learn_rmax_bind ---------
// The step kernel's thread applies a learner's experiences until the first crossing, stores the ones it has not
// applied and appends the learner to the step's worklist; the solve kernel runs the pending solve, then the rest.
struct RMaxRec {  // one experience not yet applied
  double r;
  int32_t s, sn, done, pad;
};
struct RMaxWork {
  RMaxRec* recs;              // [A * N][n_exp]
  int32_t* hdr;               // [A * N][2]: records stored, the action's table column
  int32_t* list;              // [A * N]: the learners with a solve pending, in arrival order
  uint32_t* count;            // [2]: the list's length, this step's at `parity` (the solve kernel zeroes the other)
  unsigned long long* stats;  // [2]: solves so far, the longest solve's sweeps
  int32_t n_exp, parity;
  int32_t S[RMX_MAX_AGENTS];  // each agent's rows W * H * enc_nq[a]
  int64_t N, n_learners;     // n_learners = A * N
  uint32_t* err;
};
// Workgroup size of the solve kernel: one wave per learner (the convergence flag costs one wave-wide vote, the
// barriers nothing; the parallelism of a step's solves is across learners), and how many walk the worklist by default
enum { kRMaxBlock = 64, kRMaxGrid = 2048 };
// v of the learner being solved is double-buffered in LDS, 16 B per state, within the 64 KiB of a plain launch (512 B
// of it left to the kernel's own words)
enum : int64_t { kRMaxStatesMax = (65536 - 512) / 16 };

// ---- the policy (rmax.py:108-128): no epsilon ------------------------------------------------------------------------
RMX_HD bool rmax_row_flat(double r0, double r1, double r2, double r3) { return r1 == r0 && r2 == r0 && r3 == r0; }

RMX_HD int32_t rmax_argmax(double r0, double r1, double r2, double r3) {  // np.argmax: the first maximum
  const double m = learn_max4(r0, r1, r2, r3);
  return r0 == m ? 0 : r1 == m ? 1 : r2 == m ? 2 : 3;
}

// the engine's hashed policy: a flat row takes h0 >> 62 of learn_policy's counter hash
RMX_HD int32_t rmax_policy(uint64_t seed, int64_t t, int64_t n_global, int64_t eg, int A, int i, int best, double r0,
                           double r1, double r2, double r3) {
  if (!best && rmax_row_flat(r0, r1, r2, r3)) {
    const uint64_t ctr = (((uint64_t)t * (uint64_t)n_global + (uint64_t)eg) * (uint64_t)A + (uint64_t)i) * kGolden;
    return (int32_t)(splitmix64(seed ^ ctr) >> 62);
  }
  return rmax_argmax(r0, r1, r2, r3);
}

// RMX_LEARN_NUMPY: rng.choice(actions) = integers(0, 4) on the learner's own generator, drawn for a flat row only
RMX_HD int32_t rmax_policy_numpy(LearnRng& r, double r0, double r1, double r2, double r3) {
  if (rmax_row_flat(r0, r1, r2, r3)) return (int32_t)learn_bounded(r, 4u);
  return rmax_argmax(r0, r1, r2, r3);
}

}  // namespace rmx
