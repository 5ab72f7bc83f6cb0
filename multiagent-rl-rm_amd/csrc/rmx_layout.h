// rmx_layout.h — table layouts and constants shared by the host table builders (rmx_tables.cpp, plain
// C++: builds with g++ and the sanitizers) and the gfx950 kernels.  No HIP types here.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rmx {

// ---- deterministic fast path ------------------------------------------------------------------
// The per-cell tile and the per-agent event map are pre-composed on the host into one transition
// word per (agent, cell, action), so an agent-step is two dependent LDS lookups: move word, then the
// RM (q, event) entry.  Used for deterministic dynamics without QRM outputs, A <= 4, W, H <= 255.
//   move word  bits 0-7 x', 8-15 y', 16-23 event at (x', y'), 24 wall hit, 25 hazard at (x', y'),
//              26 the step fails the agent (FL: hole; OW: wall && terminate_hit_walls or plant &&
//              terminate_on_plants)
//   RM entry   uint4 {next_q | (next_q == final_q) << 8, f32 reward_modifier * RQ, f32 shaping, f32 raw RQ}
//   info       uint4 per agent {move-table base, RM-table base, sx | sy<<8 | init_q<<16 | final_q<<24, enc_nq}
//              (final_q 255 = none)
//   merged     uint4 [A][Q][H*W][5] (separate allocation, <= 2 MiB): the move word and the RM entry of
//              (agent, q, cell, action) in ONE lookup: {x' | y'<<8 | next_q<<16 | wall<<24 | hazard<<25 |
//              fails<<26 | (next_q == final)<<27, reward_modifier * RQ, shaping, 0}
// fast-path table modes (the values are part of the step kernels' symbol names).  Round 5 removed the step's
// LDS-staged (0, step only), lane-resident (2, 3), speculative (6) and 8-B (8) modes, which lost their A/Bs.
constexpr int kTblLds = 0;                // rollout only: the blob staged into LDS
constexpr int kTblGlobal = 1, kTblMerged = 4;
constexpr int kTblMergedLds = 5;          // rollout only: the merged table staged into LDS
constexpr int kTblMerged4 = 7;            // step: merged table as 4-B records, reward from a per-agent palette (no shaping)
constexpr size_t kRolloutLdsMax = 64 * 1024;  // LDS bytes a rollout workgroup stages at most
constexpr size_t kMergedMaxBytes = 2u << 20;
constexpr int kFastMaxAgents = 4;
constexpr int kFastMaxQrm = 16;  // QRM experiences per agent the fast kernel emits (Qx); beyond: generic
constexpr size_t kFastBlobMaxBytes = 16 * 1024;  // the fast path's blob (move words, RM entries): <= 16 KiB
constexpr uint32_t kMvWall = 1u << 24, kMvHazard = 1u << 25, kMvFail = 1u << 26;
// fast step kernel store modes (FastParams.skip_same): every column word stored (the QRM-output instantiations only) /
// the rarely-changing rm_q and ep_ret words skipped when unchanged (the default) / the same with non-temporal
// write-through stores (the bandwidth regime, from 2^23 env x agent instances).  (Mode 1, every unchanged word
// skipped, lost its A/B and was removed in round 5.)
constexpr int kSkipNone = 0, kSkipRare = 2, kSkipRareNT = 3;

// ---- the packed record of a queue window (rmx_step_seq, step_fast_kernel_win) -------------------------------------
// Between the steps of one window the state travels in a handle-owned buffer instead of the caller's columns: 3A + 1
// columns of 4-B words, [3A + 1][N], one env per lane as in the public layout:
//   column a           (a < A)  cell word  x | y << 8 | rm_q << 16  (each < 256 on the fast path; bits 24-31 zero)
//   column A + a                the flags word, all 32 bits         (bits 0-6, agent_steps in bits 16-31)
//   column 2A + a               ep_ret, the f32's bits              (stored only when the step changed it, except by
//                                                                    the window's first step)
//   column 3A                   t, all 32 bits
// Per lane and step, A = 2: 9 loads and 5 stores against the public layout's 13 and 9 + a byte.  The form is the one
// that measured fastest as a bare copy (scripts/floor_bench.hip, profiles/r07_packed_window.md): 16-B units per agent
// with the step's write-through stores were SLOWER than today's columns (2.16 vs 2.06 us per launch at config 2),
// these 4-B columns 0.32 us faster.  `t` keeps a word of its own: the spare bits of the other words (8 in the cell
// word, 9 in the flags word) cannot hold 32.
// Out-of-range column words (the caller owns the columns and may write anything there; rmx_set_state refuses them)
// never reach a record: a record is written only AFTER a step, and the merged-table step takes x, y and rm_q of every
// agent, frozen or not, from the bytes of the table record it looked up, so they are < 256 whatever the columns held.
// The first step of a window reads the columns with the code rmx_step runs, the last one writes every column word.
// (tests/test_window_packed_gpu.py runs such words through windows: a step that let a frozen agent keep its column
// word would diverge there.)
// Plain C++ (constexpr: usable from host and device code alike).
constexpr uint32_t pk_cell(uint32_t x, uint32_t y, uint32_t q) {
  return (x & 0xFFu) | ((y & 0xFFu) << 8) | ((q & 0xFFu) << 16);
}
constexpr uint32_t pk_x(uint32_t w) { return w & 0xFFu; }
constexpr uint32_t pk_y(uint32_t w) { return (w >> 8) & 0xFFu; }
constexpr uint32_t pk_q(uint32_t w) { return (w >> 16) & 0xFFu; }
// the record's columns (in words from the buffer's start: column * N + env) and the buffer's size
constexpr int pk_col_cell(int /*A*/, int a) { return a; }
constexpr int pk_col_flags(int A, int a) { return A + a; }
constexpr int pk_col_ret(int A, int a) { return 2 * A + a; }
constexpr int pk_col_t(int A) { return 3 * A; }
constexpr size_t pk_bytes(int A, size_t n_envs) { return (size_t)(3 * A + 1) * n_envs * 4; }
// window I/O modes of step_fast_kernel_win (FastParams::pk_io; part of its symbol name)
constexpr int kIoCols = 0, kIoColsToPk = 1, kIoPkToPk = 2, kIoPkToCols = 3;

}  // namespace rmx
