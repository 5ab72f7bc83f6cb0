// rmx_learn.hip — the learn step for gfx950: auto-reset, optional action choice, the wrapper step and the tabular
// Q-learning / QRM update of every (env, agent) learner in ONE launch (include/rmx.h, rmx_learn_step*).
//
// One thread owns one environment, as in step_kernel (rmx_kernels.hip), and runs env_step of rmx_rules.h over its A
// agents in registers: the step rules stay in one place, and the env-level rule (episode end) needs no cross-lane
// work.  The thread then walks its agents' experiences, one agent after the other (learn_agent, rmx_learn.h): the
// counterfactuals are formed from AgentOut and the LDS-staged RM tables and consumed on the spot; they are never
// routed through the QRM columns.  The experiences of one agent are a dependent chain by definition (experience j may
// read the row that j' < j wrote); each is three independent accesses (the 32-B next-state row as two 16-B loads, the
// entry, the visit count) and two 8-B stores.  The step is bound by these sub-line accesses to HBM, not by the chain:
// having experience j of every agent in flight together was measured and was no faster.
// Tables are float64 [A][N][S_max][4]; every index is int64.
// With RMX_LEARN_NUMPY the thread also owns its learners' numpy generators (the column uint64 [5][A][N], plane-major:
// each word a coalesced 8-B load per lane): it draws the reference's choose_action from them and stores the two state
// words, and the buffer word when it changed.  Tail lanes and the agents past A of the 8-bucket touch nothing.
// With STOCH (a handle with slip and / or random starts under RMX_LEARN_DYN_ENV) the thread also owns its env's numpy
// generator, as step_kernel's STOCH does (the rng column uint64 [4][N], the episode column): the auto-reset reseeds it
// from the seed schedule and draws the random starts before the policy reads its rows, the step draws the slips from
// it, and the four words are stored after the step.  The learners' draws all come before the first slip draw and the
// two kinds of generator never mix.  Tail lanes touch neither column.
// With LAMBDA (rmx_learn_lambda_bind: Watkins Q(lambda) learners) the update is learn_lambda_agent's sweep over the
// learner's own list of live traces (rmx_learn.h; slot-major [A][cap][N], so a wave's read of slot j is contiguous), in
// batches of independent read-modify-writes, and the auto-reset empties the env's lists before the policy reads its
// rows.  Tail lanes and the agents past A touch no list.
// With EPS (rmx_learn_eps_bind: a per-learner epsilon schedule) a policy step loads each learner's epsilon from the
// column float64 [A][N] (one coalesced 8-B load per lane, beside the row load it does not depend on); a lane that has
// just auto-reset its env decays the value first and stores it.  A step on the caller's actions decays in the reset
// itself.  The EPS kernels are instantiated in a translation unit of their own (rmx_learn_eps.hip, which includes this
// file): the kernels of a handle without a schedule are the ones it always ran, instruction for instruction.
//
// Reference semantics: rmx_learn.h (update, experiences, policy, the Q(lambda) sweep), rmx_kernels.hip (the step).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rmx_device.h"
#include "rmx_generic.h"
#include "rmx_internal.h"
#include "rmx_learn.h"
#include "rmx_learn_body.h"

namespace rmx {

#ifdef RMX_LEARN_EPS_TU
#define RMX_LAUNCH_LEARN_STEP launch_learn_step_eps
#else
#define RMX_LAUNCH_LEARN_STEP launch_learn_step
#endif

// POLICY: kLearnActions (the caller's actions), kLearnHash (the engine's hash policy) or kLearnNumpy (each learner's
// numpy generator, read from and written back to lc.rng); everything the third adds sits behind if constexpr.
// STOCH: the env's own generator (slip, the per-episode reseed, random starts), likewise behind if constexpr.
// LAMBDA: the Q(lambda) learners (rmx_learn_lambda_bind): the auto-reset empties the env's trace lists and the update
// is learn_lambda_agent's sweep over the learner's list; behind if constexpr, as the other two.
// EPS: the per-learner epsilon schedule (rmx_learn_eps_bind), behind if constexpr as well.
// XP: the LambdaParams argument of the LAMBDA kernels, then the EpsParams argument of the EPS kernels; empty for the
// others, whose signature (and code) is that of the kernel without either (learn_extra<T>, rmx_learn.h, picks one).
template <int KIND, int AMAX, int POLICY, bool STOCH, bool LAMBDA, bool EPS, typename... XP>
__global__ void __launch_bounds__(256) learn_step_kernel(KParams p, LearnParams lp, LearnCall lc, XP... xp) {
  static_assert(sizeof...(XP) == (LAMBDA ? 1 : 0) + (EPS ? 1 : 0), "one argument each for LAMBDA and EPS, else none");
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
  bool full = false;  // LAMBDA: a trace found its list full
  AgentOut o[AMAX];
  if (live) {
    Pcg rng = {0, 0, 0, 0};
    if constexpr (STOCH) rng = {p.rng[e], p.rng[N + e], p.rng[2 * N + e], p.rng[3 * N + e]};
    bool was_reset = false;  // (read by the EPS kernels only)
    if (p.autoreset && (s[0].f & RMX_F_ENV_DONE)) {
      was_reset = true;
      reset_regs<AMAX>(s, t, p);
      // env.reset() is learn_done_episode for every agent's learner (rmx_learn_eps_bind).  A policy step decays where
      // it reads the learner's epsilon below; a step on the caller's actions reads none and decays here.
      if constexpr (EPS && POLICY == kLearnActions) learn_eps_reset(learn_extra<EpsParams>(xp...), p.A, N, e);
      if constexpr (LAMBDA) {  // env.reset() clears the traces of every agent's learner (ma_frozen_lake.py:77-81)
        const LambdaParams& lam = learn_extra<LambdaParams>(xp...);
#pragma unroll
        for (int a = 0; a < AMAX; ++a)
          if (AMAX <= 4 || a < p.A) lam.cnt[(int64_t)a * N + e] = 0;
      }
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
          double eps = lc.epsilon;
          if constexpr (EPS)  // (decays under RMX_LEARN_BEST too)
            eps = learn_eps_step(learn_extra<EpsParams>(xp...), a, N, e, was_reset);
          if constexpr (POLICY == kLearnNumpy) {
            if (lc.best) {  // no draw: the column is not touched
              act[a] = learn_policy(0, 0, 0, 0, p.A, a, eps, 1, lo.x, lo.y, hi.x, hi.y);
            } else {
              const int64_t plane = (int64_t)p.A * N;
              uint64_t* w = lc.rng + (int64_t)a * N + e;
              LearnRng r = learn_rng_load(w, plane);
              const uint64_t w4 = learn_rng_word4(r);
              act[a] = learn_policy_numpy(r, eps, lo.x, lo.y, hi.x, hi.y);
              learn_rng_store(w, plane, r, w4);
            }
          } else {
            act[a] = learn_policy(p.seed, p.t_global, p.n_global, p.env_offset + e, p.A, a, eps, lc.best, lo.x, lo.y,
                                  hi.x, hi.y);
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
    // the update: every agent, frozen ones included; an action without a table column (wait, or an invalid one,
    // which the step has reported) has nothing to update
    if (lc.update) {
#pragma unroll
      for (int a = 0; a < AMAX; ++a) {
        if ((AMAX <= 4 || a < p.A) && (uint32_t)act[a] < 4u) {
          LearnTables T;
          T.nq = L.nq + a * p.Q * p.E;
          T.rr = L.rr + a * p.Q * p.E;
          T.qrm = L.qrm + a * p.n_qrm_max;
          T.phi = lp.phi ? lp.phi + a * p.Q : nullptr;
          T.E = p.E;
          T.n_qrm = p.n_qrm[a];
          T.enc_nq = p.enc_nq[a];
          T.final_q = p.final_q[a];
          T.reward_modifier = p.reward_modifier;
          T.Q = p.Q;
          const LearnStep st = {o[a].prev_cell, o[a].cell, o[a].ev,     q_pre[a],
                                s[a].q,         o[a].env_term, o[a].term, o[a].trunc, o[a].renv};
          const int64_t base = ((int64_t)a * N + e) * lp.s_max * 4;
          if constexpr (LAMBDA)
            full |= learn_lambda_agent(lp, learn_extra<LambdaParams>(xp...), T, st, lp.q + base,
                                       lp.visits ? lp.visits + base : nullptr, act[a], (int64_t)p.HW * p.enc_nq[a], a,
                                       N, e);
          else
            learn_agent(lp, T, st, lp.q + base, lp.visits ? lp.visits + base : nullptr, act[a],
                        (int64_t)p.HW * p.enc_nq[a]);
        }
      }
    }
  }
  if (__any(bad)) {
    if ((threadIdx.x & 63) == 0) atomicOr(p.err, 1u);
  }
  if constexpr (LAMBDA) {
    if (__any(full)) {
      if ((threadIdx.x & 63) == 0) atomicOr(p.err, kErrTraceFull);
    }
  }
  wave_flush_slot(p.slab, slot, ls, __any(done));
}

template <int KIND, int AMAX, int POLICY, bool STOCH>
static void launch_learn_p(const KParams& p, const LearnParams& lp, const LearnCall& lc, const LambdaParams* lam,
                           const EpsParams* eps, dim3 g, dim3 b, size_t lds, hipStream_t st) {
#ifdef RMX_LEARN_EPS_TU  // the EpsParams behind the other arguments
  if (lam)
    hipLaunchKernelGGL((learn_step_kernel<KIND, AMAX, POLICY, STOCH, true, true, LambdaParams, EpsParams>), g, b, lds, st,
                       p, lp, lc, *lam, *eps);
  else
    hipLaunchKernelGGL((learn_step_kernel<KIND, AMAX, POLICY, STOCH, false, true, EpsParams>), g, b, lds, st, p, lp, lc,
                       *eps);
#else
  if (lam)
    hipLaunchKernelGGL((learn_step_kernel<KIND, AMAX, POLICY, STOCH, true, false, LambdaParams>), g, b, lds, st, p, lp, lc,
                       *lam);
  else
    hipLaunchKernelGGL((learn_step_kernel<KIND, AMAX, POLICY, STOCH, false, false>), g, b, lds, st, p, lp, lc);
#endif
}

template <int KIND, int AMAX, bool STOCH>
static hipError_t launch_learn_t(const KParams& p, const LearnParams& lp, const LearnCall& lc, const LambdaParams* lam,
                                 const EpsParams* eps, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if (lc.policy == kLearnNumpy)
    launch_learn_p<KIND, AMAX, kLearnNumpy, STOCH>(p, lp, lc, lam, eps, g, b, lds, st);
  else if (lc.policy)
    launch_learn_p<KIND, AMAX, kLearnHash, STOCH>(p, lp, lc, lam, eps, g, b, lds, st);
  else
    launch_learn_p<KIND, AMAX, kLearnActions, STOCH>(p, lp, lc, lam, eps, g, b, lds, st);
  return hipGetLastError();
}

// 256-thread blocks, one thread per env (the per-wave statistics slab is sized for that geometry at rmx_create).
// p.rng_on (the handle has slip or random starts; the caller has checked the learner's dynamics and the rng / episode
// columns) selects the STOCH instantiations (dispatch_env, rmx_internal.h).
// lam != NULL: the Q(lambda) kernels.  eps != NULL: the EPS kernels (launch_learn_step_eps, this function as
// rmx_learn_eps.hip compiles it).
hipError_t RMX_LAUNCH_LEARN_STEP(const KParams& p, const LearnParams& lp, const LearnCall& lc, const LambdaParams* lam,
                                 const EpsParams* eps, int kind, size_t lds, hipStream_t st) {
#ifndef RMX_LEARN_EPS_TU
  if (eps) return launch_learn_step_eps(p, lp, lc, lam, eps, kind, lds, st);
#endif
  const dim3 g((unsigned)((p.N + 255) / 256)), b(256);
  return dispatch_env(kind, p.rng_on, p.A, [&](auto K, auto S, auto AM) {
    return launch_learn_t<K.value, AM.value, S.value>(p, lp, lc, lam, eps, g, b, lds, st);
  });
}

#ifndef RMX_LEARN_EPS_TU
// rmx_learn_traces_clear and the resets of a handle with Q(lambda) bound: cnt[a][e] = 0 for the masked envs
__global__ void __launch_bounds__(256) traces_clear_kernel(int32_t* cnt, const uint8_t* mask, int A, int64_t N) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N || (mask && !mask[e])) return;
  for (int a = 0; a < A; ++a) cnt[(int64_t)a * N + e] = 0;
}

hipError_t launch_traces_clear(int32_t* cnt, const uint8_t* mask, int A, int64_t N, hipStream_t st) {
  hipLaunchKernelGGL(traces_clear_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, cnt, mask, A, N);
  return hipGetLastError();
}

// rmx_learn_eps_decay: one thread per env decays its agents' column entries (each a coalesced 8-B load and store)
__global__ void __launch_bounds__(256) eps_decay_kernel(EpsParams ep, const uint8_t* mask, int A, int64_t N) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N || (mask && !mask[e])) return;
  learn_eps_reset(ep, A, N, e);
}

hipError_t launch_eps_decay(const EpsParams& ep, const uint8_t* mask, int A, int64_t N, hipStream_t st) {
  hipLaunchKernelGGL(eps_decay_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, ep, mask, A, N);
  return hipGetLastError();
}
#endif  // RMX_LEARN_EPS_TU

}  // namespace rmx
