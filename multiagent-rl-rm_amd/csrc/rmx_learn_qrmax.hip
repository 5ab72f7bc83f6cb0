// rmx_learn_qrmax.hip — the QR-max learn step for gfx950 (include/rmx.h, "QR-max learners"): at most two launches on
// the caller's stream.
//
// qrmax_step_kernel: one thread owns one environment, exactly as rmax_step_kernel (rmx_learn_rmax.hip): auto-reset, the
// policy (rmax_policy / qrmax_policy_numpy over the row of the state the step leaves: no epsilon), env_step, the column
// stores, then every agent's experiences in order (qrmax_experience) through qrmax_update (rmx_qrmax.h).  The reference
// solves once behind the last experience of an agent-step, so the thread applies ALL of a learner's experiences itself
// and, when one of them made something known, appends the learner to the step's worklist with one atomic add.  No
// experience is handed over.
//
// qrmax_solve_kernel: a fixed grid of one-wave workgroups walks the worklist by grid stride and leaves at once when it
// is empty.  A workgroup solves one learner at a time (qrmax_solve_wg, rmx_model_solve.h, shared with the fused runs):
// the rows of final states are zeroed, V = max_a Q double-buffered
// in LDS (16 B per state), the lanes stride over (s, q, a).  Each entry of a sweep reads V of the sweep before and its
// own old value only, so a sweep is ONE pass: back up, store in place, leave the next sweep's V in the other buffer
// (the four lanes of a state exchange their entries by wave shuffle) and vote on cdelta > VI_delta.  The environment
// model and the RM model of one learner are contiguous, a few tens of KB: they stay in L2 over the sweeps and are not
// staged in LDS.
// Both kernels and the host path run the same functions in the same list order without FMA: the tables agree bit for
// bit.  Every index is int64.
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

// POLICY / STOCH: as learn_step_kernel's.
template <int KIND, int AMAX, int POLICY, bool STOCH>
__global__ void __launch_bounds__(256) qrmax_step_kernel(KParams p, LearnParams lp, LearnCall lc, QRMaxParams qp,
                                                         RMaxWork wk) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int64_t N = p.N;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = e < N;

  AgentReg s[AMAX];
  int32_t act[AMAX];
  int32_t t = 0;
  if (live) {
    t = p.t[e];
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
      if (AMAX <= 4 || a < p.A) {
        const int64_t k = (int64_t)a * N + e;
        load_agent(p, k, s[a]);
        if constexpr (POLICY == kLearnActions) act[a] = p.actions[k];
      }
    }
  }
  const SlabSlot slot = slab_prefetch(p.slab);
  stage_tables(lds, p.tables, p.tables_n16);
  __syncthreads();
  const Lds L = lds_view(lds, p);

  LaneStats ls = {0.0, 0, 0, 0};
  bool done = false;
  uint32_t bad = 0;
  bool full = false;  // a successor found its list full
  AgentOut o[AMAX];
  if (live) {
    Pcg rng = {0, 0, 0, 0};
    if constexpr (STOCH) rng = {p.rng[e], p.rng[N + e], p.rng[2 * N + e], p.rng[3 * N + e]};
    if (p.autoreset && (s[0].f & RMX_F_ENV_DONE)) {  // (env.reset() does nothing to a QRMax_v2)
      reset_regs<AMAX>(s, t, p);
      if constexpr (STOCH) {  // env.rng = default_rng(seed of the next episode)
        const int32_t k = p.episode[e] + 1;
        p.episode[e] = k;
        rng = seed_pcg64(seed_of(p, p.env_offset + e, k));
        if (p.random_starts) random_starts<AMAX>(p, rng, e, s);  // before the policy's row read and any slip draw
      }
    }
    // the RM state the step is about to leave; the policy reads that state's row
    int32_t q_pre[AMAX];
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
      if (AMAX <= 4 || a < p.A) {
        q_pre[a] = s[a].q;
        if constexpr (POLICY) {
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
            act[a] = rmax_policy(p.seed, p.t_global, p.n_global, p.env_offset + e, p.A, a, lc.best, lo.x, lo.y, hi.x,
                                 hi.y);
          }
          if (lc.actions_out) lc.actions_out[(int64_t)a * N + e] = act[a];
        }
      }
    }
    const float disc = p.gamma_is_one ? 1.0f : p.disc[min((uint32_t)t, (uint32_t)p.max_t + 1u)];
    done = env_step<KIND, AMAX>(s, t, act, L, p, disc, o, ls, &bad, STOCH ? &rng : nullptr);
    if constexpr (STOCH) {
      p.rng[e] = rng.hi;
      p.rng[N + e] = rng.lo;
      p.rng[2 * N + e] = rng.ihi;
      p.rng[3 * N + e] = rng.ilo;
    }
    p.t[e] = t;
    if (p.env_done) p.env_done[e] = (uint8_t)done;
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
      if (AMAX <= 4 || a < p.A) store_agent(p, (int64_t)a * N + e, a, e, s[a], o[a], L);
    }
    // the model update: every agent, frozen ones included; an action without a table column has nothing to update
    if (lc.update) {
#pragma unroll
      for (int a = 0; a < AMAX; ++a) {
        if ((AMAX <= 4 || a < p.A) && (uint32_t)act[a] < 4u) {
          LearnTables T;
          T.nq = L.nq + a * p.Q * p.E;
          T.rr = L.rr + a * p.Q * p.E;
          T.qrm = L.qrm + a * p.n_qrm_max;
          T.phi = nullptr;
          T.E = p.E;
          T.n_qrm = p.n_qrm[a];
          T.enc_nq = p.enc_nq[a];
          T.final_q = p.final_q[a];
          T.reward_modifier = p.reward_modifier;
          T.Q = p.Q;
          const LearnStep st = {o[a].prev_cell, o[a].cell, o[a].ev,     q_pre[a],
                                s[a].q,         o[a].env_term, o[a].term, o[a].trunc, o[a].renv};
          const int64_t learner = (int64_t)a * N + e;
          const QRMaxLearner M = qrmax_learner(lp, qp, learner);
          const int n = qrmax_n_exp(lp, T);
          bool fresh = false;  // some experience of this agent-step made something known
          for (int j = 0; j < n; ++j) {
            QRMaxExp x;
            if (!qrmax_experience(lp, T, st, j, qp.P, x)) continue;
            const int res = qrmax_update(qp, M, T.enc_nq, x, act[a]);
            full |= (res & kQRMaxFull) != 0;
            fresh |= (res & kQRMaxNew) != 0;
          }
          if (fresh) {  // one solve behind the last experience; the learner enters the list once per step
            const uint32_t at = atomicAdd(wk.count + wk.parity, 1u);
            if ((int64_t)at < wk.n_learners) wk.list[at] = (int32_t)learner;  // (always: one entry per learner)
          }
        }
      }
    }
  }
  if (__any(bad)) {
    if ((threadIdx.x & 63) == 0) atomicOr(p.err, 1u);
  }
  if (__any(full)) {
    if ((threadIdx.x & 63) == 0) atomicOr(p.err, kErrModelFull);
  }
  wave_flush_slot(p.slab, slot, ls, __any(done));
}

__global__ void __launch_bounds__(kRMaxBlock) qrmax_solve_kernel(LearnParams lp, QRMaxParams qp, RMaxWork wk) {
  extern __shared__ __attribute__((aligned(16))) double vbuf[];
  const uint32_t n = (uint32_t)min((int64_t)wk.count[wk.parity], wk.n_learners);
  if (blockIdx.x == 0 && threadIdx.x == 0) wk.count[wk.parity ^ 1] = 0u;  // the next step's list starts empty
  for (uint32_t wi = blockIdx.x; wi < n; wi += gridDim.x) {
    const int64_t learner = wk.list[wi];
    if ((uint64_t)learner >= (uint64_t)wk.n_learners) continue;  // (the engine's own list; uniform)
    const int a = (int)(learner / wk.N);
    const int32_t nQ = wk.S[a] / qp.P;
    if (nQ < 1 || (int64_t)qp.P * nQ > lp.s_max) continue;  // (the engine's own sizes; uniform)
    const QRMaxLearner M = qrmax_learner(lp, qp, learner);
    const int sweeps = qrmax_solve_wg(qp, lp.gamma, M, nQ, vbuf, lp.s_max);
    if (threadIdx.x == 0) {
      atomicAdd(wk.stats, 1ull);
      atomicMax(wk.stats + 1, (unsigned long long)sweeps);
      atomicAdd(wk.stats + 2, (unsigned long long)sweeps);
    }
    __syncthreads();  // the next learner's V overwrites this one's
  }
}

template <int KIND, int AMAX, bool STOCH>
static hipError_t launch_qrmax_t(const KParams& p, const LearnParams& lp, const LearnCall& lc, const QRMaxParams& qp,
                                 const RMaxWork& wk, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if (lc.policy == kLearnNumpy)
    hipLaunchKernelGGL((qrmax_step_kernel<KIND, AMAX, kLearnNumpy, STOCH>), g, b, lds, st, p, lp, lc, qp, wk);
  else if (lc.policy)
    hipLaunchKernelGGL((qrmax_step_kernel<KIND, AMAX, kLearnHash, STOCH>), g, b, lds, st, p, lp, lc, qp, wk);
  else
    hipLaunchKernelGGL((qrmax_step_kernel<KIND, AMAX, kLearnActions, STOCH>), g, b, lds, st, p, lp, lc, qp, wk);
  return hipGetLastError();
}

// The step kernel (256-thread blocks, one thread per env, as launch_learn_rmax), then with lc.update the solve kernel
// over the step's worklist: `grid` one-wave workgroups, 16 * s_max bytes of LDS each.
hipError_t launch_learn_qrmax(const KParams& p, const LearnParams& lp, const LearnCall& lc, const QRMaxParams& qp,
                              const RMaxWork& wk, int grid, int kind, size_t lds, hipStream_t st) {
  const dim3 g((unsigned)((p.N + 255) / 256)), b(256);
  const hipError_t rc = dispatch_env(kind, p.rng_on, p.A, [&](auto K, auto S, auto AM) {
    return launch_qrmax_t<K.value, AM.value, S.value>(p, lp, lc, qp, wk, g, b, lds, st);
  });
  if (rc != hipSuccess || !lc.update) return rc;
  hipLaunchKernelGGL(qrmax_solve_kernel, dim3((unsigned)grid), dim3(kRMaxBlock), (size_t)(16 * lp.s_max), st, lp, qp, wk);
  return hipGetLastError();
}

}  // namespace rmx
