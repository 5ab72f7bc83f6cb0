// rmx_learn_rmax.hip — the R-max learn step for gfx950 (include/rmx.h, "R-max learners"): at most two launches on the
// caller's stream.
//
// rmax_step_kernel: one thread owns one environment, exactly as learn_step_kernel (rmx_learn.hip): auto-reset, the
// policy (rmax_policy / rmax_policy_numpy over the row of the state the step leaves: no epsilon), env_step, the column
// stores, then every agent's experiences in order (rmax_experience).  The thread applies update_q itself
// (rmax_update_q, rmx_rmax.h) for as long as no pair crosses the threshold: counts, reward sums and the successor
// lists are the learner's own slices, and almost every step of a run is of this kind.  At a learner's first crossing
// the thread stops: the crossing observation is counted, the experiences behind it go to the engine's record buffer
// unapplied, and the learner is appended to the step's worklist with one atomic add.
//
// rmax_solve_kernel: a fixed grid of one-wave workgroups walks the worklist by grid stride and leaves at once when it
// is empty.  A workgroup solves one learner at a time (rmax_solve_wg, rmx_model_solve.h, shared with the fused runs):
// v = max_a q double-buffered in LDS (16 B per state), the lanes
// stride over (s, k), a sweep is a test pass (every masked entry's backup against its q; one vote across the
// workgroup; nothing has been written when the vote says converged) and, if it has not converged, a write pass that
// recomputes the backup from the same v, stores it and leaves the next sweep's v in the other buffer (the four lanes
// of a state exchange their entries by wave shuffle).  No entry of a sweep reads a value written in that sweep.  Lane
// 0 then applies the learner's stored experiences in order; a further crossing is solved by the whole workgroup again.
// q, counts, reward sums and lists of one learner are contiguous, a few tens of KB: they stay in L2 over the sweeps.
// Both kernels and the host path run the same functions in the same slot order without FMA: the tables agree bit for
// bit.  Tables are float64 [A][N][S_max][4]; every index is int64.
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

// POLICY / STOCH: as learn_step_kernel's.
template <int KIND, int AMAX, int POLICY, bool STOCH>
__global__ void __launch_bounds__(256) rmax_step_kernel(KParams p, LearnParams lp, LearnCall lc, RMaxParams rp,
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
    if (p.autoreset && (s[0].f & RMX_F_ENV_DONE)) {  // (env.reset() does nothing to an RMax)
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
          const int64_t S = (int64_t)p.HW * p.enc_nq[a];
          const int64_t learner = (int64_t)a * N + e;
          const RMaxLearner M = rmax_learner(lp, rp, learner);
          const int n = rmax_n_exp(lp, T);
          bool crossed = false;
          int32_t stored = 0;
          for (int j = 0; j < n; ++j) {
            LearnExp x;
            if (!rmax_experience(lp, T, st, j, S, x)) continue;
            if (!crossed) {
              const int res = rmax_update_q(rp, M, x, act[a]);
              full |= (res & kRMaxFull) != 0;
              crossed = (res & kRMaxCross) != 0;
            } else if (stored < wk.n_exp) {  // (n <= 1 + n_qrm_max = n_exp, and one experience crossed)
              wk.recs[learner * wk.n_exp + stored] = {x.r, (int32_t)x.s, (int32_t)x.sn, x.done ? 1 : 0, 0};
              ++stored;
            }
          }
          if (crossed) {  // the solve is pending; the learner enters the list once per step
            wk.hdr[2 * learner] = stored;
            wk.hdr[2 * learner + 1] = act[a];
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

__global__ void __launch_bounds__(kRMaxBlock) rmax_solve_kernel(LearnParams lp, RMaxParams rp, RMaxWork wk) {
  extern __shared__ __attribute__((aligned(16))) double vbuf[];
  __shared__ int sh_next, sh_cross;
  const uint32_t n = (uint32_t)min((int64_t)wk.count[wk.parity], wk.n_learners);
  if (blockIdx.x == 0 && threadIdx.x == 0) wk.count[wk.parity ^ 1] = 0u;  // the next step's list starts empty
  for (uint32_t wi = blockIdx.x; wi < n; wi += gridDim.x) {
    const int64_t learner = wk.list[wi];
    if ((uint64_t)learner >= (uint64_t)wk.n_learners) continue;  // (the engine's own list; uniform)
    const int a = (int)(learner / wk.N);
    const int64_t S = wk.S[a];
    const RMaxLearner M = rmax_learner(lp, rp, learner);
    const int32_t n_rec = min(wk.hdr[2 * learner], wk.n_exp), k = wk.hdr[2 * learner + 1] & 3;
    int32_t next = 0;
    for (;;) {
      const int sweeps = rmax_solve_wg(rp, lp.gamma, M, S, vbuf, lp.s_max);
      if (threadIdx.x == 0) {  // the experiences behind the crossing, in order, up to the next crossing
        atomicAdd(wk.stats, 1ull);
        atomicMax(wk.stats + 1, (unsigned long long)sweeps);
        int cross = 0;
        bool full = false;
        while (next < n_rec && !cross) {
          const RMaxRec r = wk.recs[learner * wk.n_exp + next];
          ++next;
          if ((uint64_t)r.s >= (uint64_t)S || (uint64_t)r.sn >= (uint64_t)S) continue;  // (the engine's own records)
          const LearnExp x = {r.s, r.sn, r.r, r.done != 0};
          const int res = rmax_update_q(rp, M, x, k);
          full |= (res & kRMaxFull) != 0;
          cross = (res & kRMaxCross) != 0;
        }
        if (full) atomicOr(wk.err, kErrModelFull);
        sh_next = next;
        sh_cross = cross;
      }
      __syncthreads();  // lane 0's stores are the workgroup's
      next = sh_next;
      const int cross = sh_cross;
      __syncthreads();
      if (!cross) break;
    }
  }
}

template <int KIND, int AMAX, bool STOCH>
static hipError_t launch_rmax_t(const KParams& p, const LearnParams& lp, const LearnCall& lc, const RMaxParams& rp,
                                const RMaxWork& wk, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if (lc.policy == kLearnNumpy)
    hipLaunchKernelGGL((rmax_step_kernel<KIND, AMAX, kLearnNumpy, STOCH>), g, b, lds, st, p, lp, lc, rp, wk);
  else if (lc.policy)
    hipLaunchKernelGGL((rmax_step_kernel<KIND, AMAX, kLearnHash, STOCH>), g, b, lds, st, p, lp, lc, rp, wk);
  else
    hipLaunchKernelGGL((rmax_step_kernel<KIND, AMAX, kLearnActions, STOCH>), g, b, lds, st, p, lp, lc, rp, wk);
  return hipGetLastError();
}

// The step kernel (256-thread blocks, one thread per env, as launch_learn_step), then with lc.update the solve kernel
// over the step's worklist: `grid` one-wave workgroups, 16 * s_max bytes of LDS each.
hipError_t launch_learn_rmax(const KParams& p, const LearnParams& lp, const LearnCall& lc, const RMaxParams& rp,
                             const RMaxWork& wk, int grid, int kind, size_t lds, hipStream_t st) {
  const dim3 g((unsigned)((p.N + 255) / 256)), b(256);
  const hipError_t rc = dispatch_env(kind, p.rng_on, p.A, [&](auto K, auto S, auto AM) {
    return launch_rmax_t<K.value, AM.value, S.value>(p, lp, lc, rp, wk, g, b, lds, st);
  });
  if (rc != hipSuccess || !lc.update) return rc;
  hipLaunchKernelGGL(rmax_solve_kernel, dim3((unsigned)grid), dim3(kRMaxBlock), (size_t)(16 * lp.s_max), st, lp, rp, wk);
  return hipGetLastError();
}

}  // namespace rmx
