// rmx_learn_body.h — the device-only blocks of the learn-step body that the learn kernels share: learn_step_kernel
// (rmx_learn.hip), rmax_step_kernel / qrmax_step_kernel (rmx_learn_rmax.hip, rmx_learn_qrmax.hip) and rmax_run_kernel /
// qrmax_run_kernel (rmx_learn_rmax_run.hip, rmx_learn_qrmax_run.hip).  learn_run_kernel (rmx_learn_run.hip) has the
// same blocks written out: there each call moved an instantiation's instruction count.
//
// Every function here is element-wise: it takes one env's scalars or ONE agent's AgentReg / AgentOut by reference and
// is called from the kernel's own `#pragma unroll` loop over its AMAX agents (under `AMAX <= 4 || a < p.A`); the arrays
// stay in the kernel.  Only blocks whose move leaves every kernel's resource usage and every translation unit's
// instruction count as they were are here (profiles/learn_body_resources.md lists the ones that did not and stay
// inline).  Each kernel keeps what differs: its policy call (when it draws), the auto-reset with its EPS, LAMBDA and
// STOCH branches, its update, and the wave-uniform structure of the model runs.
// The learners' generator round trip (learn_rng_load / learn_rng_store) is in rmx_learn.h, shared with the host path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rmx_device.h"
#include "rmx_generic.h"
#include "rmx_internal.h"
#include "rmx_learn.h"

namespace rmx {

// Agent a's state columns ([A][N], k = a * N + e: each a coalesced 4-B load per lane) into the env's registers.
__device__ __forceinline__ void load_agent(const KParams& p, int64_t k, AgentReg& s) {
  s.x = p.pos_x[k];
  s.y = p.pos_y[k];
  s.q = p.rm_q[k];
  s.f = p.flags[k];
  s.ret = p.ep_ret[k];
}

// The policy's row: the learner's 32-B table row of the state the step is about to leave, as two 16-B loads.  A state
// outside the agent's S = W * H * enc_nq[a] rows (columns a caller wrote out of range) reads nothing: a zero row.
__device__ __forceinline__ void policy_row(const KParams& p, const LearnParams& lp, const AgentReg& s, int a,
                                           int64_t N, int64_t e, double2& lo, double2& hi) {
  const int64_t S = (int64_t)p.HW * p.enc_nq[a];
  const int64_t st = ((int64_t)s.y * p.W + s.x) * p.enc_nq[a] + s.q;
  lo = make_double2(0.0, 0.0);
  hi = lo;
  if ((uint64_t)st < (uint64_t)S) {
    const double2* row = reinterpret_cast<const double2*>(lp.q + (((int64_t)a * N + e) * lp.s_max + st) * 4);
    lo = row[0];
    hi = row[1];
  }
}

// Agent a's columns after the step (k = a * N + e): the five state columns, the reward, the optional shaping / renv /
// enc_state columns and the QRM columns.  A run stores them once, with the outputs of its last step.
__device__ __forceinline__ void store_agent(const KParams& p, int64_t k, int a, int64_t e, const AgentReg& s,
                                            const AgentOut& o, const Lds& L) {
  p.pos_x[k] = s.x;
  p.pos_y[k] = s.y;
  p.rm_q[k] = s.q;
  p.flags[k] = s.f;
  p.ep_ret[k] = s.ret;
  p.reward[k] = o.reward;
  if (p.shaping) p.shaping[k] = o.shaping;
  if (p.renv) p.renv[k] = o.renv;
  if (p.enc_state) p.enc_state[k] = enc_index(s, p, a);
  if (p.qrm_s) emit_qrm(o, a, e, L, p);
}

// The model runs (one wave per env): lane 0's episode statistics of the whole run, added once to the slab slot of the
// env's group of 64 (rmx_create sizes the slab by 64 envs per wave).  The 64 waves of a group add with f64 atomics:
// the addends are float32 returns, whose float64 sum is exact and so independent of the order.
__device__ __forceinline__ void flush_env_stats(const KParams& p, int64_t e, const LaneStats& ls) {
  if (ls.episodes != 0) {
    double* slot = p.slab + (size_t)(e >> 6) * RMX_NSTATS;
    unsafeAtomicAdd(slot + RMX_STAT_SUM_RETURN, ls.ret);
    unsafeAtomicAdd(slot + RMX_STAT_EPISODES, (double)ls.episodes);
    unsafeAtomicAdd(slot + RMX_STAT_SUCCESSES, (double)ls.successes);
    unsafeAtomicAdd(slot + RMX_STAT_SUM_LENGTH, (double)ls.length);
  }
}

}  // namespace rmx
