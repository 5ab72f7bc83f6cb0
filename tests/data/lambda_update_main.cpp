// lambda_update_main.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone program over the Q(lambda) update the kernel and the
// host path share (learn_lambda_agent / learn_lambda_update of rmx_learn.h, included unchanged; compiled with
// -fsanitize=address,undefined by tests/test_lambda_cpu.py).  Every array is an exactly-sized heap allocation, so an
// index past a table or past slot cap of the last learner lands in the sanitizer's redzone; a write past slot cap of
// any other learner lands in its neighbour's slots, which are compared after every update.
// The program keeps its own dense restatement (one e per cell, every update sweeps all cells) and compares q, visits
// and the dense traces rebuilt from the lists bit for bit.  Scenarios: lists that fill all 4 * S slots, a small cap
// that overflows, experiences whose s or sn is outside the learner's rows, traces that decay through the subnormals
// to exactly 0 and leave the list, terminal wipes.  Exit status 0 and "LAMBDA_UPDATE_OK" when everything held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../multiagent-rl-rm_amd/csrc/rmx_learn.h"

namespace {

using namespace rmx;

constexpr int kA = 2, kW = 3, kH = 2;  // 6 cells, one RM state: S = 6 rows, 24 table cells
constexpr int64_t kN = 3, kS = kW * kH;

uint64_t g_state = 0x1234567ull;
uint32_t rnd(uint32_t n) {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)((g_state >> 33) % n);
}

bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

struct Run {
  LearnParams lp{};
  LambdaParams lam{};
  std::vector<double> q, v, val, dq, dv, de;  // d*: the dense restatement
  std::vector<int32_t> idx, cnt;
  float rr[1] = {0.5f};
  uint8_t nq[1] = {0};
  bool any_full = false;
  int64_t longest = 0, dropped = 0;

  Run(double gamma, double lambd, double lr, int32_t cap) {
    const size_t cells = (size_t)kA * kN * kS * 4;
    q.assign(cells, 0.0), v.assign(cells, 0.0), dq = q, dv = v, de = q;
    idx.assign((size_t)kA * cap * kN, -1), val.assign((size_t)kA * cap * kN, -1.0), cnt.assign((size_t)kA * kN, 0);
    lp.gamma = gamma, lp.lr = lr, lp.q = q.data(), lp.visits = v.data(), lp.s_max = kS, lp.trunc_is_terminal = 1;
    lam = {lambd, idx.data(), val.data(), cnt.data(), cap};
  }

  // one agent-step of learner (a, e): from cell `from` to cell `to`, action column k
  bool step(int a, int64_t e, uint32_t from, uint32_t to, int k, float renv, bool term) {
    LearnTables T{};
    T.nq = nq, T.rr = rr, T.qrm = nq, T.phi = nullptr, T.E = 1, T.n_qrm = 0, T.enc_nq = 1, T.final_q = 7;
    T.reward_modifier = 1.5f, T.Q = 1;
    const LearnStep st = {from, to, 0u, 0, 0, term, term, false, renv};
    const int64_t base = ((int64_t)a * kN + e) * kS * 4;
    const std::vector<int32_t> idx0 = idx;
    const std::vector<double> val0 = val;
    const std::vector<int32_t> cnt0 = cnt;
    const std::vector<double> q0 = q;
    const bool full = learn_lambda_agent(lp, lam, T, st, q.data() + base, v.data() + base, k, kS, a, kN, e);
    any_full |= full;
    // the other learners' tables, lists and counts are untouched
    for (int b = 0; b < kA; ++b)
      for (int64_t f = 0; f < kN; ++f) {
        if (b == a && f == e) continue;
        if (cnt[b * kN + f] != cnt0[b * kN + f]) return fail("a neighbour's count changed");
        for (int32_t j = 0; j < lam.cap; ++j) {
          const size_t s = ((size_t)b * lam.cap + j) * kN + f;
          if (idx[s] != idx0[s] || !same(val[s], val0[s])) return fail("a neighbour's slot changed");
        }
        for (int64_t c = 0; c < kS * 4; ++c) {
          const size_t i = ((size_t)b * kN + f) * kS * 4 + c;
          if (!same(q[i], q0[i])) return fail("a neighbour's table changed");
        }
      }
    // the dense restatement
    const bool in_range = from < kS && to < kS;
    double* Q = dq.data() + base;
    double* V = dv.data() + base;
    double* E = de.data() + base;
    if (in_range) {
      const int64_t i = (int64_t)from * 4 + k;
      V[i] += 1.0;
      const double lr = lp.lr != 0.0 ? lp.lr : learn_rate_of(V[i]);
      double best = 0.0;
      if (!term) best = learn_max4(Q[to * 4], Q[to * 4 + 1], Q[to * 4 + 2], Q[to * 4 + 3]);
      const double r = learn_reward(renv, 1.5f, 0.5f);
      const double c = learn_lambda_c(Q[i], r, best, lp.gamma, lr);
      const double g = learn_lambda_mul(lp.gamma, lam.lambd);
      E[i] = 1.0;
      for (int64_t j = 0; j < kS * 4; ++j) {
        Q[j] = learn_lambda_add(Q[j], c, E[j]);
        const double before = E[j];
        E[j] = term ? 0.0 : learn_lambda_mul(E[j], g);
        if (!term && before != 0.0 && E[j] == 0.0 && g != 0.0) ++dropped;
      }
    }
    const int32_t n = cnt[a * kN + e];
    if (n < 0 || n > lam.cap) return fail("count outside [0, cap]");
    longest = n > longest ? n : longest;
    if (lam.cap < kS * 4) return true;  // (a small cap drops traces: only the bounds are checked)
    if (full) return fail("a list of 4 * S slots reported full");
    // q, visits and the dense traces rebuilt from the list
    std::vector<double> e2((size_t)kS * 4, 0.0);
    for (int32_t j = 0; j < n; ++j) {
      const size_t s = ((size_t)a * lam.cap + j) * kN + e;
      if (idx[s] < 0 || idx[s] >= kS * 4) return fail("a listed cell outside the table");
      if (val[s] == 0.0 || e2[idx[s]] != 0.0) return fail("a zero or repeated trace in the list");
      e2[idx[s]] = val[s];
    }
    for (int64_t j = 0; j < kS * 4; ++j)
      if (!same(q[base + j], Q[j]) || !same(v[base + j], V[j]) || !same(e2[j], E[j])) return fail("tables differ");
    return true;
  }

  static bool fail(const char* what) {
    std::fprintf(stderr, "lambda_update_main: %s\n", what);
    return false;
  }
};

}  // namespace

int main() {
  // 1. full lists: long episodes over all 24 cells, fixed rate and 1 / visits, rare terminal wipes
  for (double lr : {0.3, 0.0}) {
    Run r(0.9, 0.8, lr, (int32_t)(kS * 4));
    for (int t = 0; t < 4000; ++t)
      if (!r.step((int)rnd(kA), rnd(kN), rnd(kS), rnd(kS), (int)rnd(4), (float)rnd(5) - 2.0f, rnd(97) == 0)) return 1;
    if (r.longest != kS * 4) return Run::fail("the lists never filled"), 1;
  }
  // 2. underflow: gamma * lambd = 9e-4, a trace is gone after ~107 decays; no terminal updates
  {
    Run r(0.9, 0.001, 0.3, (int32_t)(kS * 4));
    for (int t = 0; t < 6000; ++t)
      if (!r.step(0, 0, t % 200 < 4 ? rnd(kS) : 0u, rnd(kS), t % 200 < 4 ? (int)rnd(4) : 0, 1.0f, false)) return 1;
    if (r.dropped < 10) return Run::fail("no trace decayed to 0"), 1;
  }
  // 3. lambd = 0: nothing is ever listed
  {
    Run r(0.9, 0.0, 0.3, 1);
    for (int t = 0; t < 200; ++t)
      if (!r.step((int)rnd(kA), rnd(kN), rnd(kS), rnd(kS), (int)rnd(4), 1.0f, false)) return 1;
    if (r.longest != 0 || r.any_full) return Run::fail("lambd = 0 listed a trace"), 1;
  }
  // 4. cap = 3 overflows: the neighbours' slots (compared in step) and the redzone past the last learner hold
  {
    Run r(0.9, 0.9, 0.3, 3);
    for (int t = 0; t < 600; ++t)
      if (!r.step((int)rnd(kA), rnd(kN), rnd(kS), rnd(kS), (int)rnd(4), 1.0f, rnd(41) == 0)) return 1;
    if (!r.any_full || r.longest != 3) return Run::fail("cap = 3 never overflowed"), 1;
  }
  // 5. s or sn outside the learner's rows: nothing is touched (tables, visits, lists, counts)
  {
    Run r(0.9, 0.8, 0.0, (int32_t)(kS * 4));
    for (int t = 0; t < 50; ++t)
      if (!r.step(1, 2, rnd(kS), rnd(kS), (int)rnd(4), 1.0f, false)) return 1;
    const std::vector<double> q0 = r.q, v0 = r.v, val0 = r.val;
    const std::vector<int32_t> idx0 = r.idx, cnt0 = r.cnt;
    for (uint32_t bad : {(uint32_t)kS, (uint32_t)kS + 100u, 0x7FFFFFFFu, 0xFFFFFFFFu}) {
      if (!r.step(1, 2, bad, 1u, 2, 1.0f, false) || !r.step(1, 2, 1u, bad, 2, 1.0f, false)) return 1;
      if (!r.step(1, 2, bad, bad, 3, 1.0f, true)) return 1;
    }
    if (std::memcmp(q0.data(), r.q.data(), 8 * q0.size()) || std::memcmp(v0.data(), r.v.data(), 8 * v0.size()) ||
        std::memcmp(val0.data(), r.val.data(), 8 * val0.size()) || idx0 != r.idx || cnt0 != r.cnt)
      return Run::fail("an out-of-range experience wrote something"), 1;
  }
  std::printf("LAMBDA_UPDATE_OK\n");
  return 0;
}
