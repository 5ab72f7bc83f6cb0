// learn_host_main.cpp — TEST INFRASTRUCTURE ONLY: a stand-alone program over the engine's host path (rmx_hoststep.cpp,
// rmx_tables.cpp and rmx_learn.h, compiled unchanged next to this file with -fsanitize=address,undefined by
// tests/test_learn_cpu.py).  It reads one compiled scenario from the file named on the command line, runs the host
// learn step on it with q and visits in exactly-sized heap allocations (an index past a learner's table lands in the
// sanitizer's redzone) and prints an FNV digest of the tables, which the test compares with librmx.so's host handle.
//
// File layout (little endian): int32 kind, W, H, A, Q, E, max_t, n_qrm_max; float hazard_penalty, wall_penalty, gamma,
// reward_modifier; int32 hazard_fail, wall_fail, n_envs, n_steps; then cell u16[H*W], cell_event u8[A*H*W],
// next_q u8[A*Q*E], rm_reward f32[A*Q*E], init_q i32[A], final_q i32[A], start_xy i32[2A], n_qrm i32[A],
// qrm_states u8[A*Qx], enc_nq i32[A].
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../multiagent-rl-rm_amd/csrc/rmx_host.h"
#include "../../multiagent-rl-rm_amd/csrc/rmx_hoststep.h"

namespace {

template <typename T>
bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

uint64_t fnv(uint64_t d, const void* p, size_t n) {
  const unsigned char* x = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) d = (d ^ x[i]) * 0x100000001b3ull;
  return d;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hi[8], ti[4];
  float hf[4];
  if (std::fread(hi, 4, 8, f) != 8 || std::fread(hf, 4, 4, f) != 4 || std::fread(ti, 4, 4, f) != 4) return 2;
  const size_t HW = (size_t)hi[1] * hi[2], A = (size_t)hi[3], QE = (size_t)hi[4] * hi[5], Qx = (size_t)hi[7];
  std::vector<uint16_t> cell;
  std::vector<uint8_t> cell_event, next_q, qrm_states;
  std::vector<float> rm_reward;
  std::vector<int32_t> init_q, final_q, start_xy, n_qrm, enc_nq;
  if (!rd(f, cell, HW) || !rd(f, cell_event, A * HW) || !rd(f, next_q, A * QE) || !rd(f, rm_reward, A * QE) ||
      !rd(f, init_q, A) || !rd(f, final_q, A) || !rd(f, start_xy, 2 * A) || !rd(f, n_qrm, A) ||
      !rd(f, qrm_states, A * Qx) || !rd(f, enc_nq, A))
    return 2;
  std::fclose(f);
  rmx_config c;
  std::memset(&c, 0, sizeof(c));
  c.kind = hi[0], c.width = hi[1], c.height = hi[2], c.n_agents = hi[3], c.n_rm_states = hi[4], c.n_events = hi[5];
  c.max_t = hi[6], c.n_qrm_max = hi[7], c.device = RMX_DEVICE_HOST;
  c.hazard_penalty = hf[0], c.wall_penalty = hf[1], c.gamma = hf[2], c.reward_modifier = hf[3];
  c.hazard_fail = ti[0], c.wall_fail = ti[1];
  const size_t N = (size_t)ti[2];
  const int steps = ti[3];
  c.n_envs = c.n_envs_global = (int64_t)N;
  c.seed_scale = c.seed_env_stride = 1;
  c.cell = cell.data(), c.cell_event = cell_event.data(), c.next_q = next_q.data(), c.rm_reward = rm_reward.data();
  c.init_q = init_q.data(), c.final_q = final_q.data(), c.start_xy = start_xy.data(), c.n_qrm = n_qrm.data();
  c.qrm_states = qrm_states.data(), c.enc_nq = enc_nq.data();
  if (!rmx::validate_config(c).empty()) return 3;
  int32_t nq_max = 0;
  for (size_t a = 0; a < A; ++a) nq_max = enc_nq[a] > nq_max ? enc_nq[a] : nq_max;
  const size_t s_max = HW * (size_t)nq_max, AN = A * N;
  uint64_t digest = 0xcbf29ce484222325ull;
  // QRM with a fixed rate and the visit counts, then one update per step with the 1 / visits rate; each on fresh tables
  for (int mode = 0; mode < 2; ++mode) {
    rmx::HostEngine h;
    if (!h.init(c).empty()) return 4;
    std::vector<int32_t> px(AN), py(AN), q(AN), t(N), act(AN), chosen(AN);
    std::vector<uint32_t> fl(AN);
    std::vector<float> ret(AN), rew(AN);
    rmx_buffers b;
    std::memset(&b, 0, sizeof(b));
    b.pos_x = px.data(), b.pos_y = py.data(), b.rm_q = q.data(), b.flags = fl.data(), b.ep_ret = ret.data();
    b.t = t.data(), b.reward = rew.data();
    h.bind(b);
    h.reset(nullptr, 5);
    std::vector<double> qt(AN * s_max * 4, 1.0), vt(AN * s_max * 4, 0.0);  // exactly [A][N][S_max][4]
    rmx::LearnParams lp{};
    lp.gamma = 0.9;
    lp.lr = mode == 0 ? 0.1 : 0.0;
    lp.q = qt.data(), lp.visits = vt.data();
    lp.s_max = (int64_t)s_max;
    lp.use_qrm = mode == 0;
    lp.trunc_is_terminal = c.kind == RMX_FROZEN_LAKE;
    h.learn = lp;
    h.learn_on = true;
    for (int s = 0; s < steps; ++s) {
      rmx::LearnCall lc{};
      lc.update = 1;
      if (s % 4 == 3) {  // the engine's policy, its actions written out
        lc.policy = 1;
        lc.epsilon = 0.3;
        lc.actions_out = chosen.data();
        h.step(nullptr, 1, false, 11, s, nullptr, &lc);
      } else {
        h.fill_actions(11, s, 1, act.data());
        h.step(act.data(), 1, false, 0, 0, nullptr, &lc);
      }
    }
    digest = fnv(fnv(digest, qt.data(), 8 * qt.size()), vt.data(), 8 * vt.size());
  }
  std::printf("LEARN_HOST_DIGEST %016llx\n", (unsigned long long)digest);
  return 0;
}
