// rmx_learn_qrmax_run.hip — T consecutive QR-max learn steps in ONE launch for gfx950 (include/rmx.h,
// rmx_learn_model_run): rmx_learn_rmax_run.hip's twin for the two launches of rmx_learn_qrmax.hip.
//
// qrmax_run_kernel: one WAVE owns one environment (one-wave workgroups, grid = N), exactly as rmax_run_kernel: lane 0
// keeps the env in registers over the T-loop and does the auto-reset, the policy (rmax_policy / qrmax_policy_numpy),
// env_step and the per-step actions_out store; the loops over the agents and an agent-step's experiences are
// wave-uniform.  Lane 0 applies ALL experiences of an agent-step (qrmax_update, rmx_qrmax.h) and broadcasts whether
// one of them made something known; the wave then solves the learner once behind the last one (qrmax_solve_wg,
// rmx_model_solve.h), as the reference, the host path and the two-launch step do.  LDS, the barriers on both edges of
// a solve, the episode statistics and the solve statistics: as rmx_learn_rmax_run.hip states them.
// The step body's blocks are the ones qrmax_step_kernel calls (rmx_learn_body.h).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rmx_device.h"
#include "rmx_generic.h"
#include "rmx_internal.h"
#include "rmx_learn.h"
#include "rmx_learn_body.h"
#include "rmx_model_solve.h"
#include "rmx_qrmax.h"

namespace rmx {

// POLICY: kLearnHash or kLearnNumpy (a run on the caller's actions is not served); STOCH: as learn_step_kernel's.
// Auto-reset is always on.
template <int KIND, int AMAX, int POLICY, bool STOCH>
__global__ void __launch_bounds__(kRMaxBlock) qrmax_run_kernel(KParams p, LearnParams lp, LearnCall lc, QRMaxParams qp,
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
  unsigned long long solves = 0, sweeps_max = 0, sweeps_total = 0;
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
      if (s[0].f & RMX_F_ENV_DONE) {  // (env.reset() does nothing to a QRMax_v2)
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
          if constexpr (POLICY == kLearnNumpy) {  // the shuffle is drawn on every call, under best too
            const int64_t plane = (int64_t)p.A * N;
            uint64_t* w = lc.rng + (int64_t)a * N + e;
            LearnRng r = learn_rng_load(w, plane);
            const uint64_t w4 = learn_rng_word4(r);
            act[a] = qrmax_policy_numpy(r, lc.best, lo.x, lo.y, hi.x, hi.y);
            learn_rng_store(w, plane, r, w4);
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
          const int32_t nQ = Tb.enc_nq;
          const QRMaxLearner M = qrmax_learner(lp, qp, (int64_t)a * N + e);
          const int n = qrmax_n_exp(lp, Tb);
          bool fresh = false;  // some experience of this agent-step made something known
          if (lead) {
            const LearnStep st = {o[a].prev_cell, o[a].cell, o[a].ev,     q_pre[a],
                                  s[a].q,         o[a].env_term, o[a].term, o[a].trunc, o[a].renv};
            for (int j = 0; j < n; ++j) {
              QRMaxExp x;
              if (!qrmax_experience(lp, Tb, st, j, qp.P, x)) continue;
              const int res = qrmax_update(qp, M, nQ, x, k);
              full |= (res & kQRMaxFull) != 0;
              fresh |= (res & kQRMaxNew) != 0;
            }
          }
          // one solve behind the last experience (the size test is qrmax_solve_kernel's: the engine's own sizes; uniform)
          if (__shfl((int)fresh, 0) && nQ >= 1 && (int64_t)qp.P * nQ <= lp.s_max) {
            __syncthreads();  // lane 0's stores are the workgroup's
            const int sweeps = qrmax_solve_wg(qp, lp.gamma, M, nQ, v, lp.s_max);
            __syncthreads();  // the lanes' q rows are lane 0's: its next policy reads them
            ++solves;
            sweeps_max = max(sweeps_max, (unsigned long long)sweeps);
            sweeps_total += (unsigned long long)sweeps;
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
      atomicAdd(wk.stats + 2, sweeps_total);
    }
    flush_env_stats(p, e, ls);
  }
}

template <int KIND, int AMAX, bool STOCH>
static hipError_t launch_qrmax_run_t(const KParams& p, const LearnParams& lp, const LearnCall& lc, const QRMaxParams& qp,
                                    const RMaxWork& wk, int32_t T, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if (lc.policy == kLearnNumpy)
    hipLaunchKernelGGL((qrmax_run_kernel<KIND, AMAX, kLearnNumpy, STOCH>), g, b, lds, st, p, lp, lc, qp, wk, T);
  else
    hipLaunchKernelGGL((qrmax_run_kernel<KIND, AMAX, kLearnHash, STOCH>), g, b, lds, st, p, lp, lc, qp, wk, T);
  return hipGetLastError();
}

// One-wave workgroups, workgroup e owns env e.  lds = model_run_lds(tables bytes, s_max) <= kModelRunLdsMax,
// lc.policy is kLearnHash or kLearnNumpy and 1 <= T (the caller has checked all three).
hipError_t launch_qrmax_run(const KParams& p, const LearnParams& lp, const LearnCall& lc, const QRMaxParams& qp,
                           const RMaxWork& wk, int32_t T, int kind, size_t lds, hipStream_t st) {
  const dim3 g((unsigned)p.N), b(kRMaxBlock);
  return dispatch_env(kind, p.rng_on, p.A, [&](auto K, auto S, auto AM) {
    return launch_qrmax_run_t<K.value, AM.value, S.value>(p, lp, lc, qp, wk, T, g, b, lds, st);
  });
}

}  // namespace rmx
