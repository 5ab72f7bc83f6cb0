// qrmax_update_main.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone program over the QR-max rules the kernels and the
// host path share (qrmax_update / qrmax_solve / qrmax_policy_numpy of rmx_qrmax.h, included unchanged; compiled with
// -fsanitize=address,undefined by tests/test_qrmax_cpu.py).  Every array is an exactly-sized heap allocation, so an
// index past a table or past slot cap of the last learner lands in the sanitizer's redzone; a write into another
// learner's slices is caught by comparing every other learner's arrays after each update and solve.
// Scenarios: random walks of three learners over a 3 x 2 grid with two RM states under thresholds 1, 2 and 3 with the
// full cap, a cap of 1 that overflows, experiences marked done, and lists a caller did not zero (indices far outside
// the positions, which must be read as unknown and never used as an index).  After every update the counts stay at or
// below their thresholds, the list counts sum to n_tsa where nothing was dropped, and a solve leaves every value finite.
// Exit status 0 and "QRMAX_UPDATE_OK" when everything held.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../multiagent-rl-rm_amd/csrc/rmx_qrmax.h"

namespace {

using namespace rmx;

constexpr int32_t kP = 6, kNQ = 2;
constexpr int64_t kL = 3, kS = kP * kNQ;  // three learners, S_max = 12 rows

uint64_t g_state = 0x9e3779b9ull;
uint32_t rnd(uint32_t n) {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((g_state >> 33) % n);
}

int g_fail = 0;
void expect(bool ok, const char* what) {
  if (!ok) {
    std::printf("FAILED: %s\n", what);
    ++g_fail;
  }
}

struct Run {
  LearnParams lp{};
  QRMaxParams qp{};
  std::vector<double> q, visits, sum_rsa, sum_rqs, v;
  std::vector<uint8_t> known, fin;
  std::vector<int32_t> n_tsa, n_rsa, idx, cnt, n_tqs, tq_next, n_rqs;
  bool any_full = false;
  int solves = 0;

  Run(int32_t thr, int32_t thr_q, int32_t cap, int32_t junk) {
    q.assign(kL * kS * 4, 2.0 * kNQ), visits.assign(kL * kS * 4, 0.0), known.assign(kL * kS * 4, 0);
    n_tsa.assign(kL * kP * 4, 0), n_rsa = n_tsa, sum_rsa.assign(kL * kP * 4, 0.0);
    idx.assign((size_t)kL * kP * 4 * cap, junk), cnt.assign((size_t)kL * kP * 4 * cap, 0);
    n_tqs.assign(kL * kS, 0), tq_next.assign(kL * kS, junk), n_rqs = n_tqs, sum_rqs.assign(kL * kS, 0.0);
    fin.assign(kL * kS, 0), v.assign(kS, 0.0);
    lp.gamma = 0.5, lp.q = q.data(), lp.visits = visits.data(), lp.s_max = kS;
    qp.delta = 1e-3, qp.delta_rel = thr & 1, qp.max_iter = 1000;
    qp.n_te = qp.n_re = thr, qp.n_tq = qp.n_rq = thr_q, qp.cap = cap, qp.P = kP;
    qp.known_tsqa = known.data(), qp.n_tsa = n_tsa.data(), qp.n_rsa = n_rsa.data(), qp.sum_rsa = sum_rsa.data();
    qp.succ_idx = idx.data(), qp.succ_cnt = cnt.data(), qp.n_tqs = n_tqs.data(), qp.tq_next = tq_next.data();
    qp.n_rqs = n_rqs.data(), qp.sum_rqs = sum_rqs.data(), qp.fin = fin.data();
  }

  template <typename T>
  static bool others_same(const std::vector<T>& a, const std::vector<T>& b, int64_t learner) {
    const size_t per = a.size() / kL;
    for (int64_t l = 0; l < kL; ++l)
      if (l != learner && std::memcmp(a.data() + l * per, b.data() + l * per, per * sizeof(T)) != 0) return false;
    return true;
  }

  void step(int64_t learner, bool junk_lists) {
    const Run before = *this;
    const QRMaxLearner L = qrmax_learner(lp, qp, learner);
    const QRMaxExp x = {(int32_t)rnd(kP), (int32_t)rnd(kNQ), (int32_t)rnd(kP), (int32_t)rnd(kNQ),
                        0.25 * (double)rnd(4), 0.5 * (double)rnd(3), rnd(7) == 0};
    const int k = (int)rnd(4);
    if (junk_lists && rnd(5) == 0) {  // a slot the caller did not zero: a count with an index outside the positions
      const int64_t sa = (int64_t)x.s * 4 + k;
      if (L.cnt[sa * qp.cap] == 0) L.cnt[sa * qp.cap] = 1, L.n_tsa[sa] += 1;
    }
    const int res = qrmax_update(qp, L, kNQ, x, k);
    any_full = any_full || (res & kQRMaxFull);
    if (res & kQRMaxNew) {
      const int sweeps = qrmax_solve(qp, lp.gamma, L, kNQ, v.data());
      expect(sweeps >= 1 && sweeps <= qp.max_iter, "the sweeps of a solve");
      ++solves;
    }
    expect(others_same(q, before.q, learner) && others_same(visits, before.visits, learner) &&
               others_same(known, before.known, learner) && others_same(n_tsa, before.n_tsa, learner) &&
               others_same(n_rsa, before.n_rsa, learner) && others_same(sum_rsa, before.sum_rsa, learner) &&
               others_same(idx, before.idx, learner) && others_same(cnt, before.cnt, learner) &&
               others_same(n_tqs, before.n_tqs, learner) && others_same(tq_next, before.tq_next, learner) &&
               others_same(n_rqs, before.n_rqs, learner) && others_same(sum_rqs, before.sum_rqs, learner) &&
               others_same(fin, before.fin, learner),
           "another learner's slices");
    for (int64_t sa = 0; sa < kP * 4; ++sa) {
      expect(L.n_tsa[sa] <= qp.n_te + (junk_lists ? 1 : 0) && L.n_rsa[sa] <= qp.n_re, "a count past its threshold");
      int32_t sum = 0;
      for (int32_t j = 0; j < qp.cap; ++j) sum += L.cnt[sa * qp.cap + j];
      expect(any_full ? sum <= L.n_tsa[sa] : sum == L.n_tsa[sa], "the list counts against n_tsa");
    }
    for (int64_t n = 0; n < kS; ++n) expect(L.n_tqs[n] <= qp.n_tq && L.n_rqs[n] <= qp.n_rq, "an RM count past its threshold");
    for (int64_t i = 0; i < kS * 4; ++i) expect(std::isfinite(L.q[i]) && L.n_tsqa[i] <= (double)qp.n_te, "q or nTSQA");
  }
};

}  // namespace

int main() {
  int solves = 0;
  for (int32_t thr = 1; thr <= 3; ++thr) {
    Run full(thr, 1 + (thr == 3), kQRMaxSlotsFull, 0);
    for (int t = 0; t < 600; ++t) full.step((int64_t)rnd(kL), false);
    expect(!full.any_full && full.solves > 0, "the full cap never overflows here");
    solves += full.solves;
  }
  Run small(2, 1, 1, 0);
  for (int t = 0; t < 400; ++t) small.step((int64_t)rnd(kL), false);
  expect(small.any_full, "cap = 1 overflows");
  Run junk(2, 1, 2, 1 << 28);  // unzeroed slots: indices that must never be used
  for (int t = 0; t < 400; ++t) junk.step((int64_t)rnd(kL), true);
  // the policy: the shuffle draws on every call, and the pick is one of the four actions
  LearnRng r = {seed_pcg64(7), 0, 0};
  for (int t = 0; t < 200; ++t) {
    const LearnRng before = r;
    const int32_t a = qrmax_policy_numpy(r, t & 1, 1.0, 1.0, 1.0, t % 3 ? 1.0 : 2.0);
    expect(a >= 0 && a < 4 && (r.hi != before.hi || r.lo != before.lo), "the policy");
    if (t % 3 == 0) expect(a == 3, "np.argmax of a row that is not flat");
  }
  if (g_fail) return 1;
  std::printf("QRMAX_UPDATE_OK solves=%d\n", solves);
  return 0;
}
