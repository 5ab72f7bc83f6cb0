// rmx_model_solve.h — one value iteration of an R-max or a QR-max learner by a one-wave workgroup, device only: the
// solve the two-launch steps run from their worklists (rmax_solve_kernel, rmx_learn_rmax.hip; qrmax_solve_kernel,
// rmx_learn_qrmax.hip) and the fused runs run in place (rmx_learn_model_run.hip).  The sequential statements they are
// checked against are rmax_solve (rmx_rmax.h) and qrmax_solve (rmx_qrmax.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rmx_learn.h"
#include "rmx_qrmax.h"
#include "rmx_rmax.h"

namespace rmx {

// One solve of learner M over its S rows by the whole workgroup (rmax_solve, rmx_rmax.h, is its sequential statement).
// v: [2][s_max] in LDS.  Returns the sweeps made; every thread has passed a barrier behind the last store.
__device__ inline int rmax_solve_wg(const RMaxParams& rp, double gamma, const RMaxLearner& M, int64_t S, double* v,
                                    int64_t s_max) {
  static_assert(kRMaxBlock % 4 == 0 && kRMaxBlock <= 64, "a state's four entries sit in four adjacent lanes of a wave");
  const int tid = (int)threadIdx.x;
  const int64_t S4 = S * 4;
  const double thr = (double)rp.threshold;
  int cur = 0;
  for (int64_t n = tid; n < S; n += kRMaxBlock) {
    double row[4];
    learn_load_row(M.q + n * 4, row);
    v[n] = learn_max4(row[0], row[1], row[2], row[3]);
  }
  __syncthreads();
  int it = 0;
  while (it < rp.max_iter) {
    ++it;
    const double* vc = v + (int64_t)cur * s_max;
    double* vn = v + (int64_t)(cur ^ 1) * s_max;
    // the test pass: nothing is written
    int conv = 1;
    for (int64_t base = 0; base < S4; base += kRMaxBlock) {
      const int64_t i = base + tid;
      if (i < S4) {
        const double c = M.counts[i];
        if (c >= thr) {
          const double nw = rmax_backup(gamma, rp.cap, M.rsum[i], c, M.idx + i * rp.cap, M.cnt + i * rp.cap, vc);
          conv &= rmax_converged(M.q[i], nw, rp.delta, rp.delta_rel) ? 1 : 0;
        }
      }
    }
    if (__syncthreads_and(conv)) break;
    // the write pass: the same backups from the same v, and the next sweep's v into the other buffer
    for (int64_t base = 0; base < S4; base += kRMaxBlock) {  // (a uniform trip count: every lane takes the shuffles)
      const int64_t i = base + tid;
      double val = 0.0;
      if (i < S4) {
        const double c = M.counts[i];
        if (c >= thr) {
          val = rmax_backup(gamma, rp.cap, M.rsum[i], c, M.idx + i * rp.cap, M.cnt + i * rp.cap, vc);
          M.q[i] = val;
        } else {
          val = M.q[i];
        }
      }
      const int l0 = tid & ~3;
      const double a0 = __shfl(val, l0), a1 = __shfl(val, l0 + 1), a2 = __shfl(val, l0 + 2), a3 = __shfl(val, l0 + 3);
      if ((tid & 3) == 0 && i < S4) vn[i >> 2] = learn_max4(a0, a1, a2, a3);
    }
    __syncthreads();
    cur ^= 1;
  }
  return it;
}

// One solve of learner M (nQ RM states, S = P * nQ rows) by the whole workgroup (qrmax_solve, rmx_qrmax.h, is its
// sequential statement).  v: [2][s_max] in LDS.  Returns the sweeps made; every thread has passed a barrier behind the
// last store.
__device__ inline int qrmax_solve_wg(const QRMaxParams& qp, double gamma, const QRMaxLearner& M, int32_t nQ, double* v,
                                     int64_t s_max) {
  static_assert(kRMaxBlock % 4 == 0 && kRMaxBlock <= 64, "a state's four entries sit in four adjacent lanes of a wave");
  const int tid = (int)threadIdx.x;
  const int64_t S = (int64_t)qp.P * nQ, S4 = S * 4;
  for (int64_t n = tid; n < S; n += kRMaxBlock) {  // final rows become zero here, not when they were marked
    double2* row = reinterpret_cast<double2*>(M.q + n * 4);
    double m = 0.0;
    if (M.fin[n]) {
      row[0] = row[1] = make_double2(0.0, 0.0);
    } else {
      const double2 lo = row[0], hi = row[1];
      m = learn_max4(lo.x, lo.y, hi.x, hi.y);
    }
    v[n] = m;
  }
  __syncthreads();
  int cur = 0, it = 0;
  int more = 1.0 > qp.delta ? 1 : 0;  // delta = 1.0 before the first sweep
  while (more && it < qp.max_iter) {
    const double* vc = v + (int64_t)cur * s_max;
    double* vn = v + (int64_t)(cur ^ 1) * s_max;
    int moved = 0;
    for (int64_t base = 0; base < S4; base += kRMaxBlock) {  // (a uniform trip count: every lane takes the shuffles)
      const int64_t i = base + tid;
      double val = 0.0;
      if (i < S4) {
        val = M.q[i];
        const int64_t sq = i >> 2;
        const int64_t sa = (sq / nQ) * 4 + (i & 3);
        if (qrmax_solved_entry(qp, M, i, sa)) {
          const double nw = qrmax_backup(qp, gamma, M, nQ, (int32_t)(sq % nQ), sa, vc);
          if (qrmax_delta(nw, val, qp.delta_rel) > qp.delta) moved = 1;
          M.q[i] = nw;
          val = nw;
        }
      }
      const int l0 = tid & ~3;
      const double a0 = __shfl(val, l0), a1 = __shfl(val, l0 + 1), a2 = __shfl(val, l0 + 2), a3 = __shfl(val, l0 + 3);
      if ((tid & 3) == 0 && i < S4) vn[i >> 2] = learn_max4(a0, a1, a2, a3);
    }
    more = __syncthreads_or(moved);
    cur ^= 1;
    ++it;
  }
  return it;
}

}  // namespace rmx
