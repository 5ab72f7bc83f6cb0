// The host learn step (csrc/rmx_hoststep.cpp HostEngine::step with a LearnCall) on a slip + random-start world as a
// stand-alone program, for the sanitizer build of tests/test_slearn_cpu.py.  The world comes from a file the test
// writes: the rmx_config bytes, then the host tables in the order cell, cell_event, next_q, rm_reward, init_q, final_q,
// start_xy, n_qrm, qrm_states, enc_nq (no shaping table), their lengths following from the config's scalars.  Every
// column and table is an exactly-sized heap allocation (a read or write past one lands in the sanitizer's redzone).
// Runs `steps` learn steps cycling through the caller's actions, the engine's policy and the learners' numpy streams,
// with `best` and the update switched on and off, and prints an FNV-1a digest of q, visits, the learner generators, the
// env generators, the episode counts and the state columns; the test computes the same digest on a host handle.
//   slearn_host_main WORLD_FILE STEPS SEED
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rmx_host.h"
#include "rmx_hoststep.h"

using namespace rmx;

static std::vector<unsigned char> take(FILE* f, size_t n) {
  std::vector<unsigned char> v(n);
  if (n && fread(v.data(), 1, n, f) != n) {
    fprintf(stderr, "short world file\n");
    exit(2);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const long long steps = atoll(argv[2]);
  const uint64_t seed = strtoull(argv[3], nullptr, 10);
  rmx_config c;
  {
    const std::vector<unsigned char> raw = take(f, sizeof(c));
    std::memcpy(&c, raw.data(), sizeof(c));
  }
  const size_t A = (size_t)c.n_agents, N = (size_t)c.n_envs, AN = A * N, HW = (size_t)c.width * c.height;
  const size_t QE = (size_t)c.n_rm_states * c.n_events, Qx = (size_t)c.n_qrm_max;
  const std::vector<unsigned char> cell = take(f, 2 * HW), cev = take(f, A * HW), nq = take(f, A * QE),
                                   rr = take(f, 4 * A * QE), iq = take(f, 4 * A), fq = take(f, 4 * A),
                                   sxy = take(f, 8 * A), nqrm = take(f, 4 * A), qst = take(f, A * Qx),
                                   enq = take(f, 4 * A);
  fclose(f);
  c.cell = reinterpret_cast<const uint16_t*>(cell.data());
  c.cell_event = cev.data();
  c.next_q = nq.data();
  c.rm_reward = reinterpret_cast<const float*>(rr.data());
  c.shape = nullptr;
  c.init_q = reinterpret_cast<const int32_t*>(iq.data());
  c.final_q = reinterpret_cast<const int32_t*>(fq.data());
  c.start_xy = reinterpret_cast<const int32_t*>(sxy.data());
  c.n_qrm = reinterpret_cast<const int32_t*>(nqrm.data());
  c.qrm_states = qst.data();
  c.enc_nq = reinterpret_cast<const int32_t*>(enq.data());
  if (!validate_config(c).empty() || !(c.stochastic && c.random_starts) || c.has_shaping) return 3;
  HostEngine h;
  if (!h.init(c).empty()) return 4;

  std::vector<int32_t> px(AN), py(AN), q(AN), t(N), enc(AN), qs(AN * Qx), qsn(AN * Qx), ep(N);
  std::vector<uint32_t> fl(AN);
  std::vector<float> ret(AN), rew(AN), renv(AN), qrq(AN * Qx);
  std::vector<uint8_t> done(N), qd(AN * Qx);
  std::vector<uint64_t> rng(4 * N);
  rmx_buffers b;
  std::memset(&b, 0, sizeof(b));
  b.pos_x = px.data(), b.pos_y = py.data(), b.rm_q = q.data(), b.flags = fl.data(), b.ep_ret = ret.data();
  b.t = t.data(), b.reward = rew.data(), b.env_done = done.data(), b.renv = renv.data(), b.enc_state = enc.data();
  if (Qx) b.qrm_s = qs.data(), b.qrm_sn = qsn.data(), b.qrm_rq = qrq.data(), b.qrm_done = qd.data();
  b.rng = rng.data(), b.episode = ep.data();
  h.bind(b);
  h.reset(nullptr, seed);

  // the learner of rmx_learn_bind (QRM, the 1 / visits rate) and the generator column of rmx_learn_rng_bind / _seed
  int32_t m = 0;
  for (size_t a = 0; a < A; ++a) m = c.enc_nq[a] > m ? c.enc_nq[a] : m;
  const size_t s_max = HW * (size_t)m;
  std::vector<double> tq(AN * s_max * 4, 0.5), tv(AN * s_max * 4, 0.0);
  std::vector<uint64_t> seeds(AN), col(5 * AN);
  for (size_t k = 0; k < AN; ++k) seeds[k] = (uint64_t)k * 7919u + 1u;
  learn_rng_fill(seeds.data(), (int64_t)AN, col.data());
  LearnParams lp{};
  lp.gamma = 0.9, lp.lr = 0.0;
  lp.q = tq.data(), lp.visits = tv.data(), lp.phi = nullptr;
  lp.s_max = (int64_t)s_max;
  lp.use_qrm = 1, lp.use_rsh = 0, lp.trunc_is_terminal = 1;
  h.learn = lp;
  h.learn_on = true;
  h.learn_rng = col.data();

  std::vector<int32_t> act(AN), out(AN);
  for (long long s = 0; s < steps; ++s) {
    LearnCall lc{};
    lc.epsilon = 0.25;
    lc.best = s % 11 == 10, lc.update = s % 13 != 12;
    if (s % 3 == 0) {  // the caller's actions (FrozenLake slip has no wait action)
      for (size_t k = 0; k < AN; ++k) act[k] = (int32_t)(((long long)k + s) % 4);
      lc.best = 0, lc.update = 1;
      h.step(act.data(), 1, false, 0, 0, nullptr, &lc);
    } else {
      lc.policy = s % 3 == 1 ? kLearnHash : kLearnNumpy;
      lc.actions_out = out.data();
      lc.rng = col.data();
      h.step(nullptr, 1, false, seed, s, nullptr, &lc);
    }
  }
  if (h.err) return 5;
  uint64_t d = 0xcbf29ce484222325ull;
  auto mix = [&](const void* p, size_t n) {
    const unsigned char* x = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) d = (d ^ x[i]) * 0x100000001b3ull;
  };
  mix(tq.data(), 8 * tq.size()), mix(tv.data(), 8 * tv.size()), mix(col.data(), 8 * col.size());
  mix(rng.data(), 8 * rng.size()), mix(ep.data(), 4 * N);
  mix(px.data(), 4 * AN), mix(py.data(), 4 * AN), mix(q.data(), 4 * AN), mix(t.data(), 4 * N);
  printf("SLEARN_HOST_DIGEST %016llx\n", (unsigned long long)d);
  return 0;
}
