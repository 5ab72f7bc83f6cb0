// rmx_learn_run.hip — T consecutive learn steps in ONE launch for gfx950 (include/rmx.h, rmx_learn_run): what
// rollout_kernel (rmx_kernels.hip) is to step_kernel, for learn_step_kernel (rmx_learn.hip).
//
// Every learner belongs to one (env, agent) and envs never interact, so T learn steps of one env are a sequential
// program for the one thread that owns the env: no grid-wide synchronisation, no hand-off between workgroups.  The
// tables are staged to LDS once; the env's state, t, its generator and its episode count stay in registers over the
// T-loop and are stored once at the end, with the output columns of the LAST step (reward, renv, shaping, env_done,
// enc_state, the QRM columns: every step writes the same slots, so the last step's values are the stepwise result).
// The learners' tables, their generator column and the trace lists stay in memory: the thread reads back what it
// wrote itself in an earlier step, which learn_step_kernel already relies on inside one launch (experience chains,
// the trace lists).  The learners' five generator words are loaded per step from the coalesced column in every
// bucket: those loads do not depend on the table row the policy waits for and fly beside it, so keeping up to 80
// VGPRs of generator state live across env_step and the sweep would buy no round trip.
// With EPS (rmx_learn_eps_bind: a per-learner epsilon schedule) the env's A epsilons do stay in registers over the
// T-loop, one double per agent: the auto-reset decays them there, the policy reads them there, and a lane whose env
// reset stores them once at the end.  A reload per step cost 6-7 % of the run at 65,536 envs.  The
// EPS kernels are instantiated in a translation unit of their own (rmx_learn_run_eps.hip, which includes this file):
// the kernels of a handle without a schedule are the ones it always ran.
// actions_out is stored per step ([T][A][N], a coalesced 4-B store per lane); the episode statistics are summed per
// lane over the whole run and flushed once per wave, as rollout_kernel's (so the return sum is associated differently
// from T single steps; the integer statistics are equal).
// The step body has the same blocks as learn_step_kernel's, written out: the other five learn kernels call
// rmx_learn_body.h for the blocks they share, but in this kernel each of those calls changed some instantiation's
// instruction count, so its body stays inline (profiles/learn_body_resources.md).  The update, the policy and the sweep
// are rmx_learn.h's.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "rmx_device.h"
#include "rmx_generic.h"
#include "rmx_internal.h"
#include "rmx_learn.h"

namespace rmx {

#ifdef RMX_LEARN_EPS_TU
#define RMX_LAUNCH_LEARN_RUN launch_learn_run_eps
#else
#define RMX_LAUNCH_LEARN_RUN launch_learn_run
#endif

// POLICY: kLearnHash or kLearnNumpy (a run on the caller's actions is not served); STOCH, LAMBDA, EPS, XP: as
// learn_step_kernel's.  Auto-reset is always on.
template <int KIND, int AMAX, int POLICY, bool STOCH, bool LAMBDA, bool EPS, typename... XP>
__global__ void __launch_bounds__(256) learn_run_kernel(KParams p, LearnParams lp, LearnCall lc, int32_t T, XP... xp) {
  static_assert(POLICY == kLearnHash || POLICY == kLearnNumpy, "a run chooses its own actions");
  static_assert(sizeof...(XP) == (LAMBDA ? 1 : 0) + (EPS ? 1 : 0), "one argument each for LAMBDA and EPS, else none");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int64_t N = p.N;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = e < N;

  AgentReg s[AMAX];
  int32_t t = 0;
  if (live) {
    t = p.t[e];
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
      if (AMAX <= 4 || a < p.A) {
        const int64_t k = (int64_t)a * N + e;
        s[a].x = p.pos_x[k];
        s[a].y = p.pos_y[k];
        s[a].q = p.rm_q[k];
        s[a].f = p.flags[k];
        s[a].ret = p.ep_ret[k];
      }
    }
  }
  stage_tables(lds, p.tables, p.tables_n16);
  __syncthreads();
  const Lds L = lds_view(lds, p);

  LaneStats ls = {0.0, 0, 0, 0};
  bool done = false;
  uint32_t bad = 0;
  bool full = false;  // LAMBDA: a trace found its list full
  AgentOut o[AMAX];
  const int64_t eg = p.env_offset + e;
  Pcg rng = {0, 0, 0, 0};
  int32_t episode = 0;
  if constexpr (STOCH) {
    if (live) {
      rng = {p.rng[e], p.rng[N + e], p.rng[2 * N + e], p.rng[3 * N + e]};
      episode = p.episode[e];
    }
  }
  // EPS: the env's learners' epsilons stay in registers over the T-loop as the state does, loaded once and, when the
  // env has reset, stored once at the end (a reload per step beside the row was measured: DESIGN.md 4.10.5)
  double eps[AMAX];
  bool eps_moved = false;
  if constexpr (EPS) {
    if (live) {
#pragma unroll
      for (int a = 0; a < AMAX; ++a)
        if (AMAX <= 4 || a < p.A) eps[a] = learn_extra<EpsParams>(xp...).col[(int64_t)a * N + e];
    }
  }
  for (int32_t it = 0; it < T; ++it) {
    if (live) {
      if (s[0].f & RMX_F_ENV_DONE) {
        reset_regs<AMAX>(s, t, p);
        if constexpr (EPS) {  // env.reset() is learn_done_episode for every agent's learner, before the policy
          const EpsParams& ep = learn_extra<EpsParams>(xp...);
          eps_moved = true;
#pragma unroll
          for (int a = 0; a < AMAX; ++a)
            if (AMAX <= 4 || a < p.A) eps[a] = learn_eps_decay(eps[a], ep.end, ep.decay);
        }
        if constexpr (LAMBDA) {  // env.reset() clears the traces of every agent's learner
          const LambdaParams& lam = learn_extra<LambdaParams>(xp...);
#pragma unroll
          for (int a = 0; a < AMAX; ++a)
            if (AMAX <= 4 || a < p.A) lam.cnt[(int64_t)a * N + e] = 0;
        }
        if constexpr (STOCH) {  // env.rng = default_rng(seed of the next episode)
          rng = seed_pcg64(seed_of(p, eg, ++episode));
          if (p.random_starts) random_starts<AMAX>(p, rng, e, s);  // before the policy's row read and any slip draw
        }
      }
      // the RM state the step is about to leave; the policy reads that state's row
      int32_t q_pre[AMAX];
      int32_t act[AMAX];
#pragma unroll
      for (int a = 0; a < AMAX; ++a) {
        if (AMAX <= 4 || a < p.A) {
          q_pre[a] = s[a].q;
          const int64_t S = (int64_t)p.HW * p.enc_nq[a];
          const int64_t st = ((int64_t)s[a].y * p.W + s[a].x) * p.enc_nq[a] + s[a].q;
          double2 lo = make_double2(0.0, 0.0), hi = lo;
          if ((uint64_t)st < (uint64_t)S) {
            const double2* row = reinterpret_cast<const double2*>(lp.q + (((int64_t)a * N + e) * lp.s_max + st) * 4);
            lo = row[0];
            hi = row[1];
          }
          const double epsilon = EPS ? eps[a] : lc.epsilon;
          if constexpr (POLICY == kLearnNumpy) {
            if (lc.best) {  // no draw: the column is not touched
              act[a] = learn_policy(0, 0, 0, 0, p.A, a, epsilon, 1, lo.x, lo.y, hi.x, hi.y);
            } else {
              // the learner's five words, plane-major: each a coalesced 8-B load per lane
              const int64_t plane = (int64_t)p.A * N;
              uint64_t* w = lc.rng + (int64_t)a * N + e;
              const uint64_t w4 = w[4 * plane];
              LearnRng r = {{w[0], w[plane], w[2 * plane], w[3 * plane]}, (uint32_t)(w4 >> 32), (uint32_t)w4};
              act[a] = learn_policy_numpy(r, epsilon, lo.x, lo.y, hi.x, hi.y);
              w[0] = r.hi;
              w[plane] = r.lo;
              const uint64_t n4 = learn_rng_word4(r);
              if (n4 != w4) w[4 * plane] = n4;  // (the increment never changes)
            }
          } else {
            act[a] = learn_policy(p.seed, p.t_global + it, p.n_global, eg, p.A, a, epsilon, lc.best, lo.x, lo.y,
                                  hi.x, hi.y);
          }
          if (lc.actions_out) lc.actions_out[((int64_t)it * p.A + a) * N + e] = act[a];
        }
      }
      const float disc = p.gamma_is_one ? 1.0f : p.disc[min((uint32_t)t, (uint32_t)p.max_t + 1u)];
      done = env_step<KIND, AMAX>(s, t, act, L, p, disc, o, ls, &bad, STOCH ? &rng : nullptr);
      // the update: every agent, frozen ones included; an action without a table column has nothing to update
      if (lc.update) {
#pragma unroll
        for (int a = 0; a < AMAX; ++a) {
          if ((AMAX <= 4 || a < p.A) && (uint32_t)act[a] < 4u) {
            LearnTables Tb;
            Tb.nq = L.nq + a * p.Q * p.E;
            Tb.rr = L.rr + a * p.Q * p.E;
            Tb.qrm = L.qrm + a * p.n_qrm_max;
            Tb.phi = lp.phi ? lp.phi + a * p.Q : nullptr;
            Tb.E = p.E;
            Tb.n_qrm = p.n_qrm[a];
            Tb.enc_nq = p.enc_nq[a];
            Tb.final_q = p.final_q[a];
            Tb.reward_modifier = p.reward_modifier;
            Tb.Q = p.Q;
            const LearnStep st = {o[a].prev_cell, o[a].cell, o[a].ev,     q_pre[a],
                                  s[a].q,         o[a].env_term, o[a].term, o[a].trunc, o[a].renv};
            const int64_t base = ((int64_t)a * N + e) * lp.s_max * 4;
            if constexpr (LAMBDA)
              full |= learn_lambda_agent(lp, learn_extra<LambdaParams>(xp...), Tb, st, lp.q + base,
                                         lp.visits ? lp.visits + base : nullptr, act[a], (int64_t)p.HW * p.enc_nq[a],
                                         a, N, e);
            else
              learn_agent(lp, Tb, st, lp.q + base, lp.visits ? lp.visits + base : nullptr, act[a],
                          (int64_t)p.HW * p.enc_nq[a]);
          }
        }
      }
    }
  }
  if (live) {  // the state, and the last step's outputs (T >= 1: o is that step's)
    p.t[e] = t;
    if (p.env_done) p.env_done[e] = (uint8_t)done;
    if constexpr (STOCH) {
      p.rng[e] = rng.hi;
      p.rng[N + e] = rng.lo;
      p.rng[2 * N + e] = rng.ihi;
      p.rng[3 * N + e] = rng.ilo;
      p.episode[e] = episode;
    }
    if constexpr (EPS) {
      if (eps_moved) {
#pragma unroll
        for (int a = 0; a < AMAX; ++a)
          if (AMAX <= 4 || a < p.A) learn_extra<EpsParams>(xp...).col[(int64_t)a * N + e] = eps[a];
      }
    }
#pragma unroll
    for (int a = 0; a < AMAX; ++a) {
      if (AMAX <= 4 || a < p.A) {
        const int64_t k = (int64_t)a * N + e;
        p.pos_x[k] = s[a].x;
        p.pos_y[k] = s[a].y;
        p.rm_q[k] = s[a].q;
        p.flags[k] = s[a].f;
        p.ep_ret[k] = s[a].ret;
        p.reward[k] = o[a].reward;
        if (p.shaping) p.shaping[k] = o[a].shaping;
        if (p.renv) p.renv[k] = o[a].renv;
        if (p.enc_state) p.enc_state[k] = enc_index(s[a], p, a);
        if (p.qrm_s) emit_qrm(o[a], a, e, L, p);
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
  wave_flush(p.slab, ls, __any(ls.episodes != 0));
}

template <int KIND, int AMAX, int POLICY, bool STOCH>
static void launch_run_p(const KParams& p, const LearnParams& lp, const LearnCall& lc, const LambdaParams* lam,
                         const EpsParams* eps, int32_t T, dim3 g, dim3 b, size_t lds, hipStream_t st) {
#ifdef RMX_LEARN_EPS_TU  // the EpsParams behind the other arguments
  if (lam)
    hipLaunchKernelGGL((learn_run_kernel<KIND, AMAX, POLICY, STOCH, true, true, LambdaParams, EpsParams>), g, b, lds, st, p,
                       lp, lc, T, *lam, *eps);
  else
    hipLaunchKernelGGL((learn_run_kernel<KIND, AMAX, POLICY, STOCH, false, true, EpsParams>), g, b, lds, st, p, lp, lc, T,
                       *eps);
#else
  if (lam)
    hipLaunchKernelGGL((learn_run_kernel<KIND, AMAX, POLICY, STOCH, true, false, LambdaParams>), g, b, lds, st, p, lp, lc,
                       T, *lam);
  else
    hipLaunchKernelGGL((learn_run_kernel<KIND, AMAX, POLICY, STOCH, false, false>), g, b, lds, st, p, lp, lc, T);
#endif
}

template <int KIND, int AMAX, bool STOCH>
static hipError_t launch_run_t(const KParams& p, const LearnParams& lp, const LearnCall& lc, const LambdaParams* lam,
                               const EpsParams* eps, int32_t T, dim3 g, dim3 b, size_t lds, hipStream_t st) {
  if (lc.policy == kLearnNumpy)
    launch_run_p<KIND, AMAX, kLearnNumpy, STOCH>(p, lp, lc, lam, eps, T, g, b, lds, st);
  else
    launch_run_p<KIND, AMAX, kLearnHash, STOCH>(p, lp, lc, lam, eps, T, g, b, lds, st);
  return hipGetLastError();
}

// The geometry of launch_learn_step (256-thread blocks, one thread per env: the per-wave statistics slab is sized
// for it at rmx_create).  lc.policy is kLearnHash or kLearnNumpy and 1 <= T (the caller has checked both).
hipError_t RMX_LAUNCH_LEARN_RUN(const KParams& p, const LearnParams& lp, const LearnCall& lc, const LambdaParams* lam,
                                const EpsParams* eps, int32_t T, int kind, size_t lds, hipStream_t st) {
#ifndef RMX_LEARN_EPS_TU
  if (eps) return launch_learn_run_eps(p, lp, lc, lam, eps, T, kind, lds, st);
#endif
  const dim3 g((unsigned)((p.N + 255) / 256)), b(256);
  return dispatch_env(kind, p.rng_on, p.A, [&](auto K, auto S, auto AM) {
    return launch_run_t<K.value, AM.value, S.value>(p, lp, lc, lam, eps, T, g, b, lds, st);
  });
}

}  // namespace rmx
