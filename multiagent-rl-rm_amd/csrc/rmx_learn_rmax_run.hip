// rmx_learn_rmax_run.hip — T consecutive R-max learn steps in ONE launch for gfx950 (include/rmx.h,
// rmx_learn_model_run): what learn_run_kernel (rmx_learn_run.hip) is to learn_step_kernel, for the two launches of
// rmx_learn_rmax.hip.
//
// rmax_run_kernel: one WAVE owns one environment (one-wave workgroups, grid = N).  Lane 0 is the thread of
// learn_run_kernel: it keeps the env's state, t, the env generator and the episode count in registers over the T-loop,
// does the auto-reset, the policy (rmax_policy / rmax_policy_numpy over the row of the state the step leaves),
// env_step and the per-step actions_out store, and applies update_q (rmax_update_q, rmx_rmax.h).  The loops over the
// agents and over an agent-step's experiences are wave-uniform: every lane knows their trip counts from the staged
// tables and the uniform parameters, lane 0 alone runs the experience and broadcasts its outcome by wave shuffle, and
// on a crossing the whole wave solves the learner at once (rmax_solve_wg, rmx_model_solve.h), before the next
// experience of the same agent-step: the order of the reference, of the host path and of the two-launch step.  No
// worklist, no record buffer, no atomics between the step and the solve, no second launch; envs never interact, so
// nothing synchronises across waves.
// LDS: the staged tables (tables_n16 * 16 bytes), behind them the solve's double-buffered v (16 * s_max bytes).
// Visibility: the solve's lanes read counts, reward sums and lists lane 0 has just stored, and lane 0's next policy
// reads q rows the other lanes stored: the same-workgroup hand-off of rmax_solve_kernel, a barrier (with the
// workgroup-scope release / acquire it carries) on both edges of every solve.  Nothing leaves the CU: no agent-scope
// fence.
// Episode statistics: summed on lane 0 over the run and added once to the slab slot of the env's group of 64 (the slab
// has one slot per 64 envs; the 64 waves of a group add with f64 atomics: the addends are float32 returns, whose
// float64 sum is exact, and so independent of the order, while their magnitudes span fewer than 29 binary orders).
// The solve statistics are summed per wave and added once at the end.
// The step body's blocks are the ones rmax_step_kernel calls (rmx_learn_body.h); lane 0 runs them, and the
// wave-uniform loops around the update are this kernel's own.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rmx_device.h"
#include "rmx_generic.h"
#include "rmx_internal.h"
#include "rmx_learn.h"
#include "rmx_learn_body.h"
#include "rmx_model_solve.h"
#include "rmx_rmax.h"

namespace rmx {

// POLICY: kLearnHash or kLearnNumpy (a run on the caller's actions is not served); STOCH: as learn_step_kernel's.
// Auto-reset is always on.
template <int KIND, int AMAX, int POLICY, bool STOCH>
__global__ void __launch_bounds__(kRMaxBlock) rmax_run_kernel(KParams p, LearnParams lp, LearnCall lc, RMaxParams rp,
                                                              RMaxWork wk, int32_t T) {
  static_assert(POLICY == kLearnHash || POLICY == kLearnNumpy, "a run chooses its own actions");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int64_t N = p.N;
  const int64_t e = (int64_t)blockIdx.x;  // (the grid is N)
  const bool lead = threadIdx.x == 0;

  AgentReg s[AMAX];
  int32_t t = 0;
#pragma unroll
  for (int a = 0; a < AMAX; ++a) s[a] = {0, 0, 0, 0, 0.0f};
  if (lead) {
    t = p.t[e];
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
      if (AMAX <= 4 || a < p.A) {
        load_agent(p, (int64_t)a * N + e, s[a]);
      }
    }
  }
  stage_tables(lds, p.tables, p.tables_n16);
  __syncthreads();
  const Lds L = lds_view(lds, p);
  double* v = reinterpret_cast<double*>(lds + (size_t)p.tables_n16 * 16);  // [2][s_max]

  LaneStats ls = {0.0, 0, 0, 0};
  bool done = false;
  uint32_t bad = 0;
  bool full = false;  // a successor found its list full
  unsigned long long solves = 0, sweeps_max = 0;
  AgentOut o[AMAX];
  const int64_t eg = p.env_offset + e;
  Pcg rng = {0, 0, 0, 0};
  int32_t episode = 0;
  if constexpr (STOCH) {
    if (lead) {
      rng = {p.rng[e], p.rng[N + e], p.rng[2 * N + e], p.rng[3 * N + e]};
      episode = p.episode[e];
    }
  }
  for (int32_t it = 0; it < T; ++it) {
    int32_t q_pre[AMAX];
    int32_t act[AMAX];
#pragma unroll
    for (int a = 0; a < AMAX; ++a) act[a] = q_pre[a] = 0;
    if (lead) {
      if (s[0].f & RMX_F_ENV_DONE) {  // (env.reset() does nothing to an RMax)
        reset_regs<AMAX>(s, t, p);
        if constexpr (STOCH) {  // env.rng = default_rng(seed of the next episode)
          rng = seed_pcg64(seed_of(p, eg, ++episode));
          if (p.random_starts) random_starts<AMAX>(p, rng, e, s);  // before the policy's row read and any slip draw
        }
      }
      // the RM state the step is about to leave; the policy reads that state's row
#pragma unroll
      for (int a = 0; a < AMAX; ++a) {
        if (AMAX <= 4 || a < p.A) {
          q_pre[a] = s[a].q;
          double2 lo, hi;
          policy_row(p, lp, s[a], a, N, e, lo, hi);
          if constexpr (POLICY == kLearnNumpy) {
            if (lc.best || !rmax_row_flat(lo.x, lo.y, hi.x, hi.y)) {  // no draw: the column is not touched
              act[a] = rmax_argmax(lo.x, lo.y, hi.x, hi.y);
            } else {
              const int64_t plane = (int64_t)p.A * N;
              uint64_t* w = lc.rng + (int64_t)a * N + e;
              LearnRng r = learn_rng_load(w, plane);
              const uint64_t w4 = learn_rng_word4(r);
              act[a] = rmax_policy_numpy(r, lo.x, lo.y, hi.x, hi.y);
              learn_rng_store(w, plane, r, w4);
            }
          } else {
            act[a] = rmax_policy(p.seed, p.t_global + it, p.n_global, eg, p.A, a, lc.best, lo.x, lo.y, hi.x, hi.y);
          }
          if (lc.actions_out) lc.actions_out[((int64_t)it * p.A + a) * N + e] = act[a];
        }
      }
      const float disc = p.gamma_is_one ? 1.0f : p.disc[min((uint32_t)t, (uint32_t)p.max_t + 1u)];
      done = env_step<KIND, AMAX>(s, t, act, L, p, disc, o, ls, &bad, STOCH ? &rng : nullptr);
    }
    // the model update: every agent, frozen ones included; an action without a table column has nothing to update.
    // Wave-uniform from here: lane 0's action decides for the wave
    if (lc.update) {
#pragma unroll
      for (int a = 0; a < AMAX; ++a) {
        const int32_t k = __shfl(act[a], 0);
        if ((AMAX <= 4 || a < p.A) && (uint32_t)k < 4u) {
          LearnTables Tb;
          Tb.nq = L.nq + a * p.Q * p.E;
          Tb.rr = L.rr + a * p.Q * p.E;
          Tb.qrm = L.qrm + a * p.n_qrm_max;
          Tb.phi = nullptr;
          Tb.E = p.E;
          Tb.n_qrm = p.n_qrm[a];
          Tb.enc_nq = p.enc_nq[a];
          Tb.final_q = p.final_q[a];
          Tb.reward_modifier = p.reward_modifier;
          Tb.Q = p.Q;
          const int64_t S = (int64_t)p.HW * p.enc_nq[a];
          const RMaxLearner M = rmax_learner(lp, rp, (int64_t)a * N + e);
          const int n = rmax_n_exp(lp, Tb);
          for (int j = 0; j < n; ++j) {
            int res = 0;
            if (lead) {
              const LearnStep st = {o[a].prev_cell, o[a].cell, o[a].ev,     q_pre[a],
                                    s[a].q,         o[a].env_term, o[a].term, o[a].trunc, o[a].renv};
              LearnExp x;
              if (rmax_experience(lp, Tb, st, j, S, x)) res = rmax_update_q(rp, M, x, k);
              full |= (res & kRMaxFull) != 0;
            }
            if (__shfl(res, 0) & kRMaxCross) {  // solved at once, before the next experience of this agent-step
              __syncthreads();                  // lane 0's stores are the workgroup's
              const int sweeps = rmax_solve_wg(rp, lp.gamma, M, S, v, lp.s_max);
              __syncthreads();  // the lanes' q rows are lane 0's: its next experience and its next policy read them
              ++solves;
              sweeps_max = max(sweeps_max, (unsigned long long)sweeps);
            }
          }
        }
      }
    }
  }
  if (lead) {  // the state, and the last step's outputs (T >= 1: o is that step's)
    p.t[e] = t;
    if (p.env_done) p.env_done[e] = (uint8_t)done;
    if constexpr (STOCH) {
      p.rng[e] = rng.hi;
      p.rng[N + e] = rng.lo;
      p.rng[2 * N + e] = rng.ihi;
      p.rng[3 * N + e] = rng.ilo;
      p.episode[e] = episode;
    }
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
      if (AMAX <= 4 || a < p.A) store_agent(p, (int64_t)a * N + e, a, e, s[a], o[a], L);
    }
    if (bad) atomicOr(p.err, 1u);
    if (full) atomicOr(p.err, kErrModelFull);
    if (solves) {
      atomicAdd(wk.stats, solves);
      atomicMax(wk.stats + 1, sweeps_max);
    }
    flush_env_stats(p, e, ls);
  }
}

template <int KIND, int AMAX, bool STOCH>
static hipError_t launch_rmax_run_t(const KParams& p, const LearnParams& lp, const LearnCall& lc, const RMaxParams& rp,
                                    const RMaxWork& wk, int32_t T, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if (lc.policy == kLearnNumpy)
    hipLaunchKernelGGL((rmax_run_kernel<KIND, AMAX, kLearnNumpy, STOCH>), g, b, lds, st, p, lp, lc, rp, wk, T);
  else
    hipLaunchKernelGGL((rmax_run_kernel<KIND, AMAX, kLearnHash, STOCH>), g, b, lds, st, p, lp, lc, rp, wk, T);
  return hipGetLastError();
}

// One-wave workgroups, workgroup e owns env e.  lds = model_run_lds(tables bytes, s_max) <= kModelRunLdsMax,
// lc.policy is kLearnHash or kLearnNumpy and 1 <= T (the caller has checked all three).
hipError_t launch_rmax_run(const KParams& p, const LearnParams& lp, const LearnCall& lc, const RMaxParams& rp,
                           const RMaxWork& wk, int32_t T, int kind, size_t lds, hipStream_t st) {
  const dim3 g((unsigned)p.N), b(kRMaxBlock);
  return dispatch_env(kind, p.rng_on, p.A, [&](auto K, auto S, auto AM) {
    return launch_rmax_run_t<K.value, AM.value, S.value>(p, lp, lc, rp, wk, T, g, b, lds, st);
  });
}

}  // namespace rmx
