// rmx_generic.h — the device-only half of the generic step shared by the generic kernels (rmx_kernels.hip,
// rmx_learn.hip) and the resident host-boundary stepper (rmx_sync.hip): LDS staging and the table view over it, the
// QRM columns' two kinds of store, and FrozenLake random starts over the shuffle workspace.  The rules themselves
// (agent_step, env_step, reset_regs, the QRM enumeration, the get_mdp entry rule) are in rmx_rules.h, shared with the
// host path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rmx_device.h"
#include "rmx_internal.h"
#include "rmx_rules.h"

namespace rmx {

// Stage the table blob (16-B granules) into LDS; every thread of the block participates.
__device__ __forceinline__ void stage_tables(unsigned char* lds, const uint4* __restrict__ src, int n16) {
  uint4* dst = reinterpret_cast<uint4*>(lds);
  for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
}

// the table view (rmx_rules.h) over the LDS-staged blob
typedef TableView Lds;

__device__ __forceinline__ Lds lds_view(const unsigned char* lds, const KParams& p) {
  Lds v;
  v.cell = reinterpret_cast<const uint16_t*>(lds + p.off_cell);
  v.ev = lds + p.off_ev;
  v.nq = lds + p.off_nq;
  v.rr = reinterpret_cast<const float*>(lds + p.off_rr);
  v.sh = reinterpret_cast<const float*>(lds + p.off_sh);
  v.qrm = lds + p.off_qrm;
  return v;
}

// QRM counterfactual experiences of agent a (qrm_experiences, rmx_rules.h), written to the columns qs / qsn / qrq /
// qdone ([A][Qx][N]): the bound device columns (plain stores), or, SYS,
// the host-mapped mailbox of the resident stepper (rmx_sync.hip) as relaxed system-scope stores (write-through to
// host memory, completed by the stepper's s_waitcnt before its acknowledgement).
template <typename T>
__device__ __forceinline__ void sys_store(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void sys_store(float* p, float v) {
  __hip_atomic_store(reinterpret_cast<uint32_t*>(p), __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <bool SYS = false>
__device__ __forceinline__ void emit_qrm_to(const AgentOut& o, int a, int64_t e, const Lds& L, const KParams& p,
                                            int32_t* qs, int32_t* qsn, float* qrq, uint8_t* qdone) {
  qrm_experiences(o, a, e, L, p, qs, qsn, qrq, qdone, [](auto* ptr, auto v) {
    if constexpr (SYS)
      sys_store(ptr, v);
    else
      *ptr = v;
  });
}

__device__ __forceinline__ void emit_qrm(const AgentOut& o, int a, int64_t e, const Lds& L, const KParams& p) {
  emit_qrm_to(o, a, e, L, p, p.qrm_s, p.qrm_sn, p.qrm_rq, p.qrm_done);
}

// FrozenLake random_start_positions (ma_frozen_lake.py:59-64, 156-172): agents start on free_cells[slot[a]] of the
// shuffled list (shuffle_slots, rmx_device.h; env e's workspace row holds its draws).
template <int AMAX>
__device__ void random_starts(const KParams& p, Pcg& r, int64_t e, AgentReg (&s)[AMAX]) {
  const int n = p.n_free;
  int32_t slot[AMAX];
  shuffle_slots<AMAX>(r, n, p.start_ws + e * (int64_t)shuffle_stride(n), AMAX <= 4 ? AMAX : p.A, slot);
#pragma unroll
  for (int a = 0; a < AMAX; ++a) {
    if (AMAX <= 4 || a < p.A) {
      const int32_t c = p.free_cells[slot[a]];
      s[a].x = c % p.W;
      s[a].y = c / p.W;
    }
  }
}

}  // namespace rmx
