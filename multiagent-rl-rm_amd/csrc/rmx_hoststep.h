// rmx_hoststep.h — the engine's host path: a handle created with cfg.device == RMX_DEVICE_HOST steps its envs on
// the CPU, over the same compiled tables the gfx950 generic kernels stage into LDS (build_table_blob, rmx_tables.cpp)
// and through the same rules: it instantiates agent_step / env_step / reset_regs / qrm_experiences / mdp_entry of
// rmx_rules.h, the templates the kernels instantiate, over its own parameter block (HostParams).  It serves BASELINE
// config 1 — the reference's one-env dict API on a CPU (rm_environment_wrapper.py:28-107 under
// frozen_lake_main.py:336-376) — without a GPU and without a PCIe round trip per call, and every other entry point of
// include/rmx.h on host buffers.
// Plain C++ (no HIP): the sanitizer build (oracle/Makefile `asan`) compiles this file with g++.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rmx.h"
#include "rmx_host.h"
#include "rmx_learn.h"
#include "rmx_qrmax.h"
#include "rmx_rmax.h"
#include "rmx_rules.h"

namespace rmx {

// What the rules of rmx_rules.h read from a parameter block, under the names KParams gives them (rmx_internal.h)
struct HostParams {
  int32_t W, HW, A, Q, E, max_t;
  int64_t N;
  float hazard_penalty, wall_penalty;
  int32_t hazard_fail, wall_fail, has_shaping;
  float reward_modifier;
  int32_t n_qrm_max, stochastic;
  int32_t slip_n[4], slip_out[4][4];
  uint64_t slip_thr[4][4];  // slip_threshold(cdf)
  uint64_t seed_scale, seed_env_stride, seed_episode_stride;
  int32_t n_qrm[RMX_MAX_AGENTS], enc_nq[RMX_MAX_AGENTS];
  int32_t init_q[RMX_MAX_AGENTS], final_q[RMX_MAX_AGENTS], start_x[RMX_MAX_AGENTS], start_y[RMX_MAX_AGENTS];
};

struct HostEngine {
  rmx_config cfg{};  // scalars (the table pointers are cleared once the tables are copied)
  HostParams p{};    // the rules' view of it
  // the generic kernels' blob and the view of its sections
  std::vector<unsigned char> blob;
  TableView tv{};
  std::vector<float> disc;           // gamma^t, t = 0 .. max_t + 1
  std::vector<uint16_t> free_cells;  // FrozenLake random starts (x-major non-hole cells)
  std::vector<uint16_t> shuffle;     // the shuffle's working copy of free_cells
  bool enc_on = false;        // every agent has an encoder stride: enc_state is computed
  // bound host columns; outputs the caller did not bind go to the engine's own columns (the synchronous calls
  // return them)
  rmx_buffers buf{};
  bool bound = false;
  std::vector<float> own_reward, own_renv, own_shaping;
  std::vector<uint8_t> own_done;
  std::vector<int32_t> own_enc;
  float* reward = nullptr;
  float* renv = nullptr;
  float* shaping = nullptr;
  uint8_t* env_done = nullptr;
  int32_t* enc = nullptr;
  uint64_t base_seed = 123;
  double stats[RMX_NSTATS]{};
  // bit 0: an invalid action was stepped; kErrTraceFull: a full trace list; kErrModelFull: a full R-max successor
  // list (rmx_check_errors)
  uint32_t err = 0;
  bool pending = false;   // rmx_step_sync_begin ran a step whose outputs rmx_sync_wait has not returned
  uint32_t pending_bad = 0;
  bool last_reset = false;  // the synchronous call before the copy was a reset (no step outputs)
  // the learner bound by rmx_learn_bind (rmx_learn.h): caller tables, the engine's copy of phi
  LearnParams learn{};
  bool learn_on = false;
  std::vector<double> learn_phi;
  uint64_t* learn_rng = nullptr;  // rmx_learn_rng_bind: the learners' numpy generators, caller's [5][A][N]
  // rmx_learn_lambda_bind: Q(lambda) learners over the caller's trace lists (host pointers)
  LambdaParams lam{};
  bool lam_on = false;
  // rmx_learn_eps_bind: the per-learner epsilon schedule over the caller's column [A][N] (col == NULL: none); only
  // learn steps and eps_decay touch it
  EpsParams eps{};
  // rmx_learn_rmax_bind: R-max learners over the caller's model arrays (host pointers); the solve's scratch (v of
  // S_max, new of 4 * S_max doubles).  A learn step's update is then rmax_agent, its policy rmax_policy*, and the
  // epsilon column is left alone.
  RMaxParams rmax{};
  bool rmax_on = false;
  std::vector<double> rmax_scratch;
  int64_t rmax_solves = 0, rmax_sweeps_max = 0;  // solves so far, the longest one's sweeps (tests)
  // every experience of one agent-step in order, each crossing solved at once; kErrModelFull or 0
  uint32_t rmax_agent(const LearnTables& T, const LearnStep& st, int a, int64_t e, int k);
  // rmx_learn_qrmax_bind: QR-max learners over the caller's model arrays (host pointers); the solve's scratch (v of
  // S_max doubles).  A learn step's update is then qrmax_agent, its policy rmax_policy / qrmax_policy_numpy, and the
  // epsilon column is left alone.
  QRMaxParams qrmax{};
  bool qrmax_on = false;
  std::vector<double> qrmax_scratch;
  int64_t qrmax_solves = 0, qrmax_sweeps_max = 0, qrmax_sweeps_total = 0;
  // every experience of one agent-step in order, then one solve if any made something known; kErrModelFull or 0
  uint32_t qrmax_agent(const LearnTables& T, const LearnStep& st, int a, int64_t e, int k);
  // learn_done_episode of every agent's learner of the masked envs (NULL: every env); a column must be bound
  void eps_decay(const uint8_t* mask);
  // cnt[a][e] = 0 for the masked envs (NULL: every env); nothing without Q(lambda) bound
  void traces_clear(const uint8_t* mask);

  // "" or the reason the config cannot run on the host path (after validate_config)
  std::string init(const rmx_config& c);
  void bind(const rmx_buffers& b);
  // rmx_reset (mask: host bytes, NULL = every env)
  void reset(const uint8_t* mask, uint64_t seed);
  // rmx_step / rmx_step_hashed for every env: actions [A][N] host ints, or hashed (seed, t_global); returns 1 if an
  // action outside [0, 4] (or "wait" under FrozenLake slip) was stepped (as wait)
  // lc != NULL: a learn step (rmx_learn_step / rmx_learn_step_policy): the policy's actions when lc->policy (seed,
  // t_global are then the policy hash's; lc->policy == kLearnNumpy: the learners' own generators in lc->rng), the
  // bound learner's update when lc->update (lam_on: the Q(lambda) sweep, and the lists emptied on auto-reset);
  // eps.col: the epsilon schedule, decayed at the env's auto-reset and read per learner by the policy
  uint32_t step(const int32_t* actions, int autoreset, bool hashed = false, uint64_t seed = 0, int64_t t_global = 0,
                float* trace = nullptr, const LearnCall* lc = nullptr);
  void fill_actions(uint64_t seed, int64_t t0, int32_t T, int32_t* out) const;
  int64_t mdp_states(int agent) const;
  void mdp(int agent, int fix_fl, int32_t* next, float* reward, uint8_t* done) const;
  // the synchronous calls' outputs into caller host columns (include/rmx.h: NULL fields skipped); "" or the reason a
  // requested column is not computed
  std::string copy_out(const rmx_buffers& out) const;

 private:
  template <int KIND>
  uint32_t step_kind(const int32_t* actions, int autoreset, bool hashed, uint64_t seed, int64_t t_global, float* trace,
                     const LearnCall* lc);
  template <int KIND>
  void mdp_kind(int agent, int fix_fl, int32_t* next, float* reward, uint8_t* done) const;
  void random_starts(Pcg& r, AgentReg* s);
};

// rmx_learn_rng_seed: default_rng(seeds[i]) of n learners as a generator column [5][n] (state high, state low,
// increment high, increment low, the buffer word: 0), on the host
void learn_rng_fill(const uint64_t* seeds, int64_t n, uint64_t* col);

}  // namespace rmx
