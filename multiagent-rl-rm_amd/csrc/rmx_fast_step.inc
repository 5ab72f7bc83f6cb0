// rmx_fast_step.inc - the body of the thread-per-env step kernels, included by rmx_fast.hip into step_fast_kernel
// (IO = kIoCols) and step_fast_kernel_win (the packets of a packed rmx_step_seq window).  One text for both: a window
// cannot compute anything else than its steps one by one, and rmx_step's kernel compiles to what it was.  In scope
// at the point of inclusion: the template arguments KIND, A, HASHED, TBL, QXB, SKIP, RPT, SLIP, IO (as constants)
// and the kernel's parameters N_arg, blk_arg, x_arg, y_arg, q_arg, f_arg, t_arg, act_arg, p.
  constexpr bool QRM = QXB > 0;
  constexpr bool IN_PK = IO == kIoPkToPk || IO == kIoPkToCols, OUT_PK = IO == kIoColsToPk || IO == kIoPkToPk;
  static_assert(IO == kIoCols || ((TBL == kTblMerged || TBL == kTblMerged4) && !HASHED && QXB == 0 && SLIP == 0 &&
                                  SKIP == kSkipRare),
                "packed windows: the deterministic merged-table step (x, y, rm_q come out of table bytes)");
  static_assert(!(RPT && OUT_PK), "the report rides in a window's last packet");
  static_assert(TBL == kTblGlobal || TBL == kTblMerged || TBL == kTblMerged4, "step: global or merged tables");
  static_assert(!QRM || TBL == kTblGlobal, "QRM outputs need the move word's event (global tables)");
  // M4: 4-B merged records (move word + palette index of the reward): a b32 gather instead of b128
  constexpr bool M4 = TBL == kTblMerged4;
  constexpr bool MERGED = TBL == kTblMerged || M4;
  constexpr bool STATS_FIRST = KIND == RMX_FROZEN_LAKE && A <= 2;
  // SLIP = kRngSlip | kRngStarts: the env's PCG64 + episode columns (RNG), slip draws (DRAW), FrozenLake random
  // start positions at each autoreset (RSTART)
  constexpr bool RNG = SLIP != 0, DRAW = (SLIP & kRngSlip) != 0;
  constexpr bool RSTART = (SLIP & kRngStarts) != 0 && KIND == RMX_FROZEN_LAKE;
  constexpr int SAUX = SKIP == kSkipRareNT ? kStoreAuxNT : kStoreAux;
  // column store with this instantiation's cache policy (RMX_DIAG diag bit 32: default-policy stores)
  const auto st = [&](__amdgpu_buffer_rsrc_t r, uint32_t lane_bytes, uint32_t sgpr_bytes, int32_t v) {
#ifdef RMX_DIAG
    if (p.diag & 32) {
      __builtin_amdgcn_raw_buffer_store_b32(v, r, lane_bytes, sgpr_bytes, 0);
      return;
    }
#endif
    __builtin_amdgcn_raw_buffer_store_b32(v, r, lane_bytes, sgpr_bytes, SAUX);
  };
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int tid = threadIdx.x;
#ifdef RMX_DIAG
  uint64_t st_clk[kStamps] = {}, st_rt[kStamps] = {};
#endif
  STAMP(0);
  // Preloaded pointers for A >= 3 only: measured (r01_ab_log c80) 9-11 % faster for configs 4 and 5, while for
  // A <= 2 the early load burst made config 2 bimodal (3.11 or 3.55-3.77 us per step with cold actions, vs a
  // steady 3.35-3.40) and config 3 3 % slower; there the kernarg-fetched FastParams pointers are used.
  // Window packets that read the record (IN_PK) take its pointer from the first preloaded slot (x_arg: go_step_win
  // passes p.pk there, these packets never read the columns) for A >= kWinPreMinA, so the record loads issue at wave
  // start as the column loads do here; below that they fetch p.pk from the parameter block like every other pointer
  // (kWinPreMinA and its measurements: rmx_fast.hip).
  constexpr bool PK_PRE = IN_PK && A >= kWinPreMinA;
  constexpr bool PRE = A >= 3 || PK_PRE;
  const int32_t N = PRE ? N_arg : p.N;
#ifdef RMX_DIAG
  // diag 65536: XCD-contiguous env ranges (workgroups are dealt round-robin to the 8 XCDs: give XCD x the
  // x-th eighth of the envs instead of every 8th workgroup's envs)
  uint32_t wg = blockIdx.x;
  if ((p.diag & 65536) && (gridDim.x & 7u) == 0) wg = (wg & 7u) * (gridDim.x >> 3) + (wg >> 3);
  const int32_t e_raw = (int32_t)(wg * blockDim.x) + tid;
#else
  const int32_t e_raw = (int32_t)blockIdx.x * (PRE ? blk_arg : (int32_t)blockDim.x) + tid;  // blk_arg == blockDim.x
#endif
  const bool live = e_raw < N;
  const int32_t e = live ? e_raw : N - 1;  // tail lanes re-read the last env and never store
  const uint32_t off = (uint32_t)e * 4u;
  const uint32_t col = (uint32_t)N * 4u;  // bytes per agent column (A*N*4 < 2^31 on the fast path)
  const uint32_t cols = col * (uint32_t)A;
  // (with PK_PRE the x_arg slot holds the record: the last packet's pos_x stores take the column from the block)
  const auto r_x = col_rsrc(PRE && !PK_PRE ? x_arg : p.pos_x, cols), r_y = col_rsrc(PRE ? y_arg : p.pos_y, cols);
  const auto r_q = col_rsrc(PRE ? q_arg : p.rm_q, cols), r_f = col_rsrc(PRE ? f_arg : p.flags, cols);
  const auto r_t = col_rsrc(PRE ? t_arg : p.t, col);
  const auto r_act = col_rsrc(PRE ? act_arg : p.actions, cols), r_rew = col_rsrc(p.reward, cols);
  AgentIO s[A];
  AgentIO s0[A];  // the values as loaded: a column word that the step leaves unchanged is not stored again
  // (`t` first: issued behind agent 0's lookup it cost config 4 1 %, profiles/r06_ab_log.md "t0")
  int32_t t;
  if constexpr (!IN_PK) t = col_ld(r_t, off, 0);
  __amdgpu_buffer_rsrc_t r_ret;  // built after the preloaded-pointer loads are issued (it needs a kernarg fetch)
  // the window's packed record (rmx_layout.h): [3A + 1][N] words of the handle's buffer
  [[maybe_unused]] const auto r_pk =
      col_rsrc(PK_PRE ? (const void*)x_arg : (const void*)p.pk, IO != kIoCols ? col * (uint32_t)(3 * A + 1) : 0u);
  if constexpr (IN_PK) {
    t = col_ld(r_pk, off, (uint32_t)pk_col_t(A) * col);
    if constexpr (!PK_PRE) r_ret = col_rsrc(p.ep_ret, cols);
#pragma unroll
    for (int a = 0; a < A; ++a) {
      const uint32_t cw = (uint32_t)col_ld(r_pk, off, (uint32_t)pk_col_cell(A, a) * col);
      s[a].x = (int32_t)pk_x(cw);
      s[a].y = (int32_t)pk_y(cw);
      s[a].q = (int32_t)pk_q(cw);
      s[a].f = (uint32_t)col_ld(r_pk, off, (uint32_t)pk_col_flags(A, a) * col);
      s[a].ret = __int_as_float(col_ld(r_pk, off, (uint32_t)pk_col_ret(A, a) * col));
      s[a].act = col_ld(r_act, off, a * col);
      s0[a] = s[a];
    }
    if constexpr (PK_PRE) {  // as below: nothing that needs a kernarg fetch above the record loads
      __builtin_amdgcn_sched_barrier(0);
      r_ret = col_rsrc(p.ep_ret, cols);
    }
  } else if constexpr (!PRE) {
    r_ret = col_rsrc(p.ep_ret, cols);
#pragma unroll
    for (int a = 0; a < A; ++a) {
      s[a].x = col_ld(r_x, off, a * col);
      s[a].y = col_ld(r_y, off, a * col);
      s[a].q = col_ld(r_q, off, a * col);
      s[a].f = (uint32_t)col_ld(r_f, off, a * col);
      s[a].ret = __int_as_float(col_ld(r_ret, off, a * col));
      s[a].act = HASHED ? hash_action(p.seed, p.t_global, p.n_global, p.env_offset + e, A, a) : col_ld(r_act, off, a * col);
      s0[a] = s[a];
    }
  } else {  // the returns last: their column pointer is the only one not preloaded (needed at the end only)
#pragma unroll
    for (int a = 0; a < A; ++a) {
      s[a].x = col_ld(r_x, off, a * col);
      s[a].y = col_ld(r_y, off, a * col);
      s[a].q = col_ld(r_q, off, a * col);
      s[a].f = (uint32_t)col_ld(r_f, off, a * col);
      s[a].act = HASHED ? hash_action(p.seed, p.t_global, p.n_global, p.env_offset + e, A, a) : col_ld(r_act, off, a * col);
      // agent-major load order (loads return in issue order, so agent 0's words land first): FrozenLake (config 4)
      // 2.9 % faster, OfficeWorld (config 5) 2.5 % slower (profiles/r05_ab_log.md "order")
      if constexpr (KIND == RMX_FROZEN_LAKE) __builtin_amdgcn_sched_barrier(0);
    }
    // keep the kernarg-dependent work below this point: the loads above issue at wave start
    __builtin_amdgcn_sched_barrier(0);
    r_ret = col_rsrc(p.ep_ret, cols);
#pragma unroll
    for (int a = 0; a < A; ++a) {
      s[a].ret = __int_as_float(col_ld(r_ret, off, a * col));
      s0[a] = s[a];
    }
  }
  // slip: the env's PCG64 state and episode counter, with the state loads (buffer descriptors: N < 2^27 on host)
  Pcg rng = {0ull, 0ull, 0ull, 0ull};
  int32_t episode = 0;
  // FIXED (seed_episode_stride == 0): an autoreset copies the env's cached generator (post-seed, and with random
  // starts post-shuffle) and, with random starts, its cached start cells (the reset cache, rmx_internal.h).  Without slip the rng columns change only at a reset, and
  // then only when they may hold another seed's generator (p.rs_dirty): read then, after the table lookups
  // (RNG_LATE), by the lanes that reset.  The episode counter rides in the first load burst (a late load of it made
  // the resetting lanes wait for its round trip before the step logic).
  constexpr bool FIXED = RNG && (SLIP & kRngFixedSeed) != 0;
  constexpr bool FCELLS = FIXED && RSTART;
  constexpr bool RNG_LATE = FIXED && !DRAW;  // (implies random starts)
  if constexpr (RNG && !RNG_LATE) {
    rng = ld_pcg(p.rng, N, e);
    episode = col_ld(col_rsrc(p.episode, (uint32_t)N * 4u), off, 0);
  }
  uint32_t fcw[FCELLS ? (A + 1) / 2 : 1] = {};  // FIXED random starts: the cached start cells, two agents per word
  Pcg frng = {0ull, 0ull, 0ull, 0ull};          // FIXED with slip: the cached post-seed (post-shuffle) generator
  if constexpr (FIXED) {
    if constexpr (FCELLS) {
      const auto r_fc = col_rsrc(p.rs_cells, col * (uint32_t)((A + 1) / 2));
#pragma unroll
      for (int w = 0; w < (A + 1) / 2; ++w) fcw[w] = (uint32_t)col_ld(r_fc, off, (uint32_t)w * col);
    }
    if constexpr (RNG_LATE) episode = col_ld(col_rsrc(p.episode, (uint32_t)N * 4u), off, 0);
    if constexpr (DRAW) {  // the state words; the increment words only when they may differ from the env's own
      if (p.rs_dirty) {
        frng = ld_pcg(p.rs_rng, N, e);
      } else {
        const auto r = col_rsrc(p.rs_rng, (uint32_t)N * 16u);
        const auto w0 = __builtin_amdgcn_raw_buffer_load_b64(r, (uint32_t)e * 8u, 0, 0);
        const auto w1 = __builtin_amdgcn_raw_buffer_load_b64(r, (uint32_t)e * 8u, (uint32_t)N * 8u, 0);
        frng.hi = ((uint64_t)w0[1] << 32) | w0[0];
        frng.lo = ((uint64_t)w1[1] << 32) | w1[0];
      }
    }
  }
  RsNext nx = {{0ull, 0ull, 0ull, 0ull}, 0, -1, 0, false};
  if constexpr (RSTART && !FIXED) {  // the next episode's shuffle in progress: generator [4][N] u64, index [N], episode tag [N]
    const auto r_nx = col_rsrc(p.nx_rng, (uint32_t)N * 32u);
    const uint32_t o8 = (uint32_t)e * 8u, c8 = (uint32_t)N * 8u;
    const auto w0 = __builtin_amdgcn_raw_buffer_load_b64(r_nx, o8, 0, 0);
    const auto w1 = __builtin_amdgcn_raw_buffer_load_b64(r_nx, o8, c8, 0);
    const auto w2 = __builtin_amdgcn_raw_buffer_load_b64(r_nx, o8, 2u * c8, 0);
    const auto w3 = __builtin_amdgcn_raw_buffer_load_b64(r_nx, o8, 3u * c8, 0);
    nx.g = {((uint64_t)w0[1] << 32) | w0[0], ((uint64_t)w1[1] << 32) | w1[0], ((uint64_t)w2[1] << 32) | w2[0],
            ((uint64_t)w3[1] << 32) | w3[0]};
    nx.i = col_ld(col_rsrc(p.nx_idx, (uint32_t)N * 4u), off, 0);
    nx.k = col_ld(col_rsrc(p.nx_ep, (uint32_t)N * 4u), off, 0);
    nx.i0 = nx.i;
  }
  // per-wave statistics mode (large N): this wave's slab slot, in flight with the state loads
  SlabSlot slot = {{0.0, 0.0, 0.0, 0.0}};
  if (p.wave_stats) slot = slab_prefetch(p.slab);
  // fused report: this env's statistics slots and this block's share of the slab, also in flight now
  ReportIn rin;
  if constexpr (RPT) rin = report_prefetch(p, e, live);
  const auto mg = col_rsrc(p.merged, MERGED ? (uint32_t)p.merged_bytes : 0u);
  const auto mg4 = col_rsrc(p.merged4, M4 ? (uint32_t)p.merged4_bytes : 0u);
#ifdef RMX_DIAG
  // diag (timing ablations, never correct results): 1 no stats, 4096 no table lookups, 8192 copy-through (the
  // loads and stores only)
  const int diag = p.diag;
  STAMP(1);
  STAMP(2);
#endif
  const auto tb = make_tables<true>(lds, p);

#ifdef RMX_DIAG
  if (diag & 8192) {  // copy-through: the kernel's loads and stores with no step logic
    if (live) {
      st(r_t, off, 0, t + 1);
      if (p.env_done) byte_st<SAUX>(p, (uint32_t)e, (uint32_t)t & 1u);
#pragma unroll
      for (int a = 0; a < A; ++a) {
        st(r_x, off, a * col, s[a].x + s[a].act);
        st(r_y, off, a * col, s[a].y);
        st(r_q, off, a * col, s[a].q);
        st(r_f, off, a * col, (int32_t)s[a].f);
        st(r_ret, off, a * col, __float_as_int(s[a].ret));
        st(r_rew, off, a * col, s[a].act);
      }
    }
    return;
  }
#endif
  // autoreset: the previous step ended this env's episode -> reference loop reset() before the step
  const bool rs = p.autoreset && (s[0].f & RMX_F_ENV_DONE);
  t = rs ? 0 : t;
  const int32_t t1 = t + 1;
  // OfficeWorld (discounted returns): gamma^t is read AFTER stage 1 has issued the table lookups.  Loads return
  // in issue order, so a discount load issued first puts its own round trip in front of the lookup's (config 3:
  // 2.36 vs 2.43 us per step, r03j).  Config 5 (A = 3) measured neutral to 1 % slower and FrozenLake 5 % slower
  // (the deferred form's scheduling barrier), so they keep the early read.
  constexpr bool LATE_DISC = KIND == RMX_OFFICE_WORLD && A == 1;
  float disc = LATE_DISC ? 1.0f : (p.gamma_is_one ? 1.0f : p.disc[min((uint32_t)t, (uint32_t)p.max_t + 1u)]);
  uint32_t bad = 0, all_term = 1u, all_trunc = 1u;
  // the reset's start cells: the configured ones, or (random starts) this episode's shuffle of the free cells
  int32_t sx[A], sy[A];
#pragma unroll
  for (int a = 0; a < A; ++a) sx[a] = p.start_x[a], sy[a] = p.start_y[a];
  if constexpr (RNG) {  // env.rng = default_rng(seed of the next episode) (rm_environment_wrapper reset)
    if constexpr (FIXED) {  // the same seed every episode: the cached generator (and shuffle's cells)
      if (rs) {
        if constexpr (FCELLS) fixed_start_cells<A>(fcw, sx, sy);
        episode += 1;
        if constexpr (DRAW) {
          rng.hi = frng.hi;
          rng.lo = frng.lo;
          if (p.rs_dirty) {
            rng.ihi = frng.ihi;
            rng.ilo = frng.ilo;
          }
        }
      }
    } else if constexpr (RSTART)
      rs_step<A>(p, rng, episode, nx, rs, live, p.env_offset + e,
                 reinterpret_cast<unsigned char*>(p.start_ws) + (size_t)e * (size_t)(2 * shuffle_stride(p.n_free)), lds,
                 (uint32_t)tid, sx, sy);
    else
      random_start_reset<A, false>(p, rng, episode, rs, live, p.env_offset + e, lds, (uint32_t)tid, 0u, sx, sy);
  }
  AgentTmp k[A];
  uint32_t m[A];
  uint32_t prev_cell[A];
  uint2 qe[A][QXB > 0 ? QXB : 1];  // QRM: {next | final << 8, raw RQ} per hypothetical RM state
  constexpr bool OW_SLIP = DRAW && KIND == RMX_OFFICE_WORLD;
  uint32_t blocked[OW_SLIP ? A : 1] = {};
  if constexpr (OW_SLIP) {
    static_assert(MERGED, "OfficeWorld slip: 16-B or 4-B merged records");
    uint32_t wi[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {  // the intended action's record (word 0) of every agent, in flight together
      s[a].x = rs ? sx[a] : s[a].x;
      s[a].y = rs ? sy[a] : s[a].y;
      s[a].q = rs ? p.init_q[a] : s[a].q;
      s[a].f = rs ? RMX_F_ACTIVE : s[a].f;
      s[a].ret = rs ? 0.0f : s[a].ret;
      const uint32_t mi = move_index<KIND>(s[a], (uint32_t)p.final_q[a], 0u, p, bad, k[a]);
      const uint32_t idx = (uint32_t)p.mg_base[a] + __umul24(__umul24((uint32_t)s[a].q, (uint32_t)p.HW), 5u) + mi;
      wi[a] = M4 ? __builtin_amdgcn_raw_buffer_load_b32(mg4, idx * 4u, 0, 0)
                 : __builtin_amdgcn_raw_buffer_load_b32(mg, idx * 16u, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < A; ++a) {  // apply_wall_penalty, then get_stochastic_action in agent order
      const uint32_t ac = agent_action<KIND>(s[a], (uint32_t)p.final_q[a], bad, k[a]);
      blocked[a] = (ac < (uint32_t)RMX_WAIT && (wi[a] & kMvWall)) ? 1u : 0u;
      s[a].act = (int32_t)(blocked[a] ? (uint32_t)RMX_WAIT
                                      : (ac < (uint32_t)RMX_WAIT ? (uint32_t)slip_choice(p, (int32_t)ac, rng) : ac));
    }
  }
  uint4 r[A];
  AgentRes o[A];
#pragma unroll
  for (int a = 0; a < A; ++a) {  // stage 1: every agent's move-word lookup in flight together
    // (as selects the compiler turns into one exec-masked block for every agent's words; written as bit selects that
    // stay per agent, every config measured 15-23 % slower, profiles/r05_ab_log.md "bfi")
    s[a].x = rs ? sx[a] : s[a].x;
    s[a].y = rs ? sy[a] : s[a].y;
    s[a].q = rs ? p.init_q[a] : s[a].q;
    s[a].f = rs ? RMX_F_ACTIVE : s[a].f;
    // (the return's select stays in this block although its loads are issued last: moved after the lookups, the
    // lookups issued per agent and every config ran 0-3 % slower, profiles/r05_ab_log.md "retsel")
    s[a].ret = rs ? 0.0f : s[a].ret;
    // (every outcome's record fetched before the draw instead, 18-45 % slower: profiles/r06_ab_log.md "spec")
    if constexpr (DRAW && KIND == RMX_FROZEN_LAKE) {  // get_stochastic_action for an active agent whose RM is not final
      if ((s[a].f & RMX_F_ACTIVE) && (uint32_t)s[a].q != (uint32_t)p.final_q[a]) {
        if (s[a].act == RMX_WAIT)
          bad |= 1u;  // the reference's slip map has no "wait" entry (KeyError)
        else if ((uint32_t)s[a].act < (uint32_t)RMX_WAIT)
          s[a].act = slip_choice(p, s[a].act, rng);
      }
    }
#ifdef RMX_DIAG
    if (a == 0) STAMP(3);
    if (diag & 4096) {  // no table lookups: a move word computed from the state
      const uint32_t mi = move_index<KIND>(s[a], (uint32_t)p.final_q[a], (uint32_t)p.mv_base[a], p, bad, k[a]);
      m[a] = (mi & 0x00030303u);
      continue;
    }
#endif
    // (all five actions' records fetched before the action arrived instead, 7-13 % slower: profiles/r06_ab_log.md
    // "all5")
    if constexpr (MERGED) {  // one lookup gives the move and the RM step: stage 2 only decodes
      // the record's byte offset ((q * HW + y * W + x) * 5 + ac + mg_base) * RB with 24-bit multiplies (x, y, q < 256 on
      // the fast path; garbage state stays inside 32 bits and the descriptor's range): __umul24 compiled to the
      // quarter-rate v_mul_lo_u32 / v_mad_u64_u32 (round 5, profiles/r05_ab_log.md "idx")
      const uint32_t ac = agent_action<KIND>(s[a], (uint32_t)p.final_q[a], bad, k[a]);
      constexpr uint32_t RB = M4 ? 4u : 16u;
      const uint32_t hw5 = ((uint32_t)p.HW * (5u * RB)) & 0xFFFFFFu, w5 = ((uint32_t)p.W * (5u * RB)) & 0xFFFFFFu;
      const uint32_t ro = ((uint32_t)s[a].q & 0xFFu) * hw5 + ((uint32_t)s[a].y & 0xFFu) * w5 +
                          ((uint32_t)s[a].x & 0xFFu) * (5u * RB) + (ac + (uint32_t)p.mg_base[a]) * RB;
      if constexpr (M4) {
        r[a] = make_uint4(__builtin_amdgcn_raw_buffer_load_b32(mg4, ro, 0, 0), 0u, 0u, 0u);
      } else {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(mg, ro, 0, 0);
        r[a] = make_uint4(v[0], v[1], v[2], v[3]);
      }
    } else {
      if constexpr (QRM) prev_cell[a] = (uint32_t)(s[a].y * p.W + s[a].x);  // infos prev_s: before the move
      m[a] = tb.mv(move_index<KIND>(s[a], (uint32_t)p.final_q[a], (uint32_t)p.mv_base[a], p, bad, k[a]));
    }
  }
  if constexpr (RNG_LATE) {  // FIXED without slip: a resetting lane's generator, after the lookups, if it may differ
    if (rs && live && p.rs_dirty) rng = ld_pcg(p.rs_rng, N, e);  // (else the env's generator IS the cached one)
  }
  if (LATE_DISC && !p.gamma_is_one) {
    __builtin_amdgcn_sched_barrier(0);
    disc = p.disc[min((uint32_t)t, (uint32_t)p.max_t + 1u)];
  }
#pragma unroll
  for (int a = 0; a < A; ++a) {  // stage 2
#ifdef RMX_DIAG
    if (a == 0) STAMP(4);
    if (diag & 4096) {
      const uint32_t ti = rm_index(s[a], m[a], (uint32_t)p.rm_base[a], p, k[a]);
      r[a] = make_uint4(ti & 3u, 0u, 0u, 0u);
      continue;
    }
#endif
    if constexpr (M4) {  // the palette entry (bits 28-29) as a signed byte of a uniform word: extract + convert; the
                         // float palette picked with two select levels per agent cost ~7 more instructions (round 5,
                         // profiles/r05_ab_log.md "idx"); shaping (r.z) is 0: M4 needs no shaping
      const int32_t pb = __builtin_amdgcn_readfirstlane((int)p.mg_palb[a]);
      r[a].y = __float_as_uint((float)(int32_t)__builtin_amdgcn_sbfe(pb, (r[a].x >> 25) & 0x18u, 8u));
    }
    if constexpr (OW_SLIP) {  // the wall penalty / failure of the intended action, the plant of the final cell
      const uint32_t hz = __builtin_amdgcn_ubfe(r[a].x, 25, 1);
      const uint32_t fl = (blocked[a] & (uint32_t)p.wall_fail) | (hz & (uint32_t)p.hazard_fail);
      r[a].x = (r[a].x & ~(kMvWall | kMvFail)) | (blocked[a] << 24) | (fl << 26);
    }
    if constexpr (MERGED) {
      const uint32_t w0 = r[a].x;
      k[a].mm = k[a].moving ? w0 : 0u;  // wall / hazard / fail at bits 24-26, as in the move word
      s[a].x = (int32_t)(w0 & 0xFFu);
      s[a].y = (int32_t)__builtin_amdgcn_ubfe(w0, 8, 8);
      r[a].x = __builtin_amdgcn_ubfe(w0, 16, 8) | (__builtin_amdgcn_ubfe(w0, 27, 1) << 8);
      continue;
    }
    const uint32_t ti = rm_index(s[a], m[a], (uint32_t)p.rm_base[a], p, k[a]);
    if constexpr (QRM) {  // every hypothetical RM state's entry for the same event, in flight with r[a]
      const uint32_t ev = __builtin_amdgcn_ubfe(m[a], 16, 8);
#pragma unroll
      for (int j = 0; j < QXB; ++j) {
        qe[a][j] = make_uint2(0u, 0u);
        if (j < p.n_qrm[a]) {
          const uint4 v = tb.rm((uint32_t)p.rm_base[a] + (uint32_t)p.qrm_q[a][j] * (uint32_t)p.E + ev);
          qe[a][j] = make_uint2(v.x, v.w);
        }
      }
    }
    r[a] = tb.rm(ti);
  }
  STAMP(5);
#pragma unroll
  for (int a = 0; a < A; ++a) {
    o[a] = finish<KIND>(s[a], k[a], r[a], t1, disc, p);
    all_term &= o[a].term;
    all_trunc &= o[a].trunc;
  }
  const uint32_t done = (all_term | all_trunc) & (live ? 1u : 0u);
#ifdef RMX_DIAG
  if (p.stamps) {  // make the stamp wait for the step logic (not only for memory)
    asm volatile("" ::"v"(done), "v"(s[0].f), "v"(s[A - 1].f), "v"(o[0].reward), "v"(o[A - 1].reward));
  }
#endif
  // episode statistics (evaluation_metrics.py:248-267 bookkeeping) of the envs that finished this step
  auto flush_stats = [&]() {
    if (p.wave_stats) {  // per-wave slab slot: one plain 32-B store per wave with a finished episode
      LaneStats ls = {0.0, (int)done, 0, done ? t1 : 0};
      double rsum = 0.0;
#pragma unroll
      for (int a = 0; a < A; ++a) {
        rsum += (double)s[a].ret;
        ls.successes += done ? (int)o[a].succ : 0;
      }
      ls.ret = done ? rsum : 0.0;
      wave_flush_slot(p.slab, slot, ls, __any(done));
    } else if (done) {  // per-env slots: no-return atomics from the finishing lanes only
      // thread-per-env: the agents' returns and successes summed in the lane (agent order), one adder into
      // the agent-0 slots (3 atomic instructions per wave at any A, not 1 + 2A)
      double rs = 0.0;
      uint32_t sc = 0;
#pragma unroll
      for (int a = 0; a < A; ++a) {
        rs += (double)s[a].ret;
        sc += o[a].succ;
      }
      env_stats_env(p, e, t1);
      env_stats_ret(p, e, rs, sc);
    }
  };
  // FrozenLake with A <= 2: ~6 % of the envs finish each step, so nearly every wave has stats atomics; issued
  // before the column stores their latency overlaps the store burst (config 2: 2.89-2.92 vs 3.02-3.05 us per
  // step, profiles/r02_ab_log.md ab1/ab2).  OfficeWorld episodes rarely end and A >= 3 measured neutral or
  // slower, so those keep the atomics last.
  if constexpr (STATS_FIRST) flush_stats();
  STAMP(6);
  // What a packet with OUT_PK leaves behind is read by the next packet of its window without a release fence in
  // between (rmx_queue.cpp queue_run), so every byte of it must be written through: the record's words by st() with
  // sc1, the statistics slots and the error word by agent-scope atomics (flush_stats with per-env slots, atomicOr).
  // Audit of the default-policy stores of this body: byte_st, the optional columns (shaping, renv, enc_state) and the
  // rng columns sit in the `else` of `if constexpr (OUT_PK)` below; the QRM stores need QXB > 0 and the report RPT:
  // all compiled out of these packets (the assertions here and at the top).  The per-wave slab slot's plain store
  // (p.wave_stats, a run-time switch) is never reached: launch_tpe_t dispatches a window kernel only with
  // !p.wave_stats, and rmx_step_seq packs only handles with per-env slots (seq_packs).
  static_assert(!OUT_PK || (SAUX == kStoreAux && !QRM && !RNG && !RPT && IO != kIoCols),
                "a hand-off packet stores through st() with sc1 and through agent-scope atomics only");
  if constexpr (OUT_PK) {
    // the record only: x, y and rm_q are table bytes here (rmx_layout.h); the window's first step writes every word
    // (the buffer holds another window's records), later ones ep_ret only where it changed
    if (live) {
      st(r_pk, off, (uint32_t)pk_col_t(A) * col, t1);
#pragma unroll
      for (int a = 0; a < A; ++a) {
        const uint32_t f1 = s[a].f | (done ? RMX_F_ENV_DONE : 0u);
        st(r_pk, off, (uint32_t)pk_col_cell(A, a) * col, (int32_t)pk_cell((uint32_t)s[a].x, (uint32_t)s[a].y, (uint32_t)s[a].q));
        st(r_pk, off, (uint32_t)pk_col_flags(A, a) * col, (int32_t)f1);
        if (IO == kIoColsToPk || __float_as_int(s[a].ret) != __float_as_int(s0[a].ret))
          st(r_pk, off, (uint32_t)pk_col_ret(A, a) * col, __float_as_int(s[a].ret));
      }
    } else {
      bad = 0;
    }
  } else if (live) {
    // a window's last step (kIoPkToCols) stores every word: the columns hold the values from before the window
    constexpr bool ALL = SKIP == kSkipNone || IO == kIoPkToCols;
    st(r_t, off, 0, t1);
    if (p.env_done) byte_st<SAUX>(p, (uint32_t)e, done);
#pragma unroll
    for (int a = 0; a < A; ++a) {
      const uint32_t f1 = s[a].f | (done ? RMX_F_ENV_DONE : 0u);
      st(r_x, off, a * col, s[a].x);
      st(r_y, off, a * col, s[a].y);
      if (ALL || s[a].q != s0[a].q) st(r_q, off, a * col, s[a].q);
      st(r_f, off, a * col, (int32_t)f1);
      if (ALL || __float_as_int(s[a].ret) != __float_as_int(s0[a].ret))
        st(r_ret, off, a * col, __float_as_int(s[a].ret));
      st(r_rew, off, a * col, __float_as_int(o[a].reward));
    }
    // the optional outputs, one wave-uniform test per column (tested inside the agent loop, the compiler re-derived
    // each condition per agent: ~4 instructions per column and agent)
    if (p.shaping) {
      const auto r = col_rsrc(p.shaping, cols);
#pragma unroll
      for (int a = 0; a < A; ++a) st(r, off, a * col, __float_as_int(o[a].shaping));
    }
    if (p.renv) {
      const auto r = col_rsrc(p.renv, cols);
#pragma unroll
      for (int a = 0; a < A; ++a) st(r, off, a * col, __float_as_int(o[a].renv));
    }
    if (p.enc_state) {  // state_encoder_*.encode of the new observation
      const auto r = col_rsrc(p.enc_state, cols);
#pragma unroll
      for (int a = 0; a < A; ++a) st(r, off, a * col, (s[a].y * p.W + s[a].x) * p.enc_nq[a] + s[a].q);
    }
    if constexpr (RNG) {
      const auto r_rng = col_rsrc(p.rng, (uint32_t)N * 32u);
      const uint32_t o8 = (uint32_t)e * 8u, c8 = (uint32_t)N * 8u;
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      // the generator moves with slip draws and at a reset only (FIXED with a clean cache: not even then without slip)
      if (DRAW || (rs && (!FIXED || p.rs_dirty))) {
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{(uint32_t)rng.hi, (uint32_t)(rng.hi >> 32)}, r_rng, o8, 0, SAUX);
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{(uint32_t)rng.lo, (uint32_t)(rng.lo >> 32)}, r_rng, o8, c8, SAUX);
      }
      if (rs && FIXED && !p.rs_dirty) {  // same seed, same increment: only the episode counter moves
        st(col_rsrc(p.episode, (uint32_t)N * 4u), off, 0, episode);
      } else if (rs) {  // a reseed changes the increment words too
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{(uint32_t)rng.ihi, (uint32_t)(rng.ihi >> 32)}, r_rng, o8, 2u * c8,
                                              SAUX);
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{(uint32_t)rng.ilo, (uint32_t)(rng.ilo >> 32)}, r_rng, o8, 3u * c8,
                                              SAUX);
        st(col_rsrc(p.episode, (uint32_t)N * 4u), off, 0, episode);
      }
      if constexpr (RSTART && !FIXED) {  // the precompute moved on (draws every step; a new generator after a reset)
        const auto r_nx = col_rsrc(p.nx_rng, (uint32_t)N * 32u);
        if (nx.fresh || nx.i != nx.i0) {
          __builtin_amdgcn_raw_buffer_store_b64(u32x2{(uint32_t)nx.g.hi, (uint32_t)(nx.g.hi >> 32)}, r_nx, o8, 0, SAUX);
          __builtin_amdgcn_raw_buffer_store_b64(u32x2{(uint32_t)nx.g.lo, (uint32_t)(nx.g.lo >> 32)}, r_nx, o8, c8, SAUX);
          st(col_rsrc(p.nx_idx, (uint32_t)N * 4u), off, 0, nx.i);
        }
        if (nx.fresh) {
          __builtin_amdgcn_raw_buffer_store_b64(u32x2{(uint32_t)nx.g.ihi, (uint32_t)(nx.g.ihi >> 32)}, r_nx, o8, 2u * c8,
                                                SAUX);
          __builtin_amdgcn_raw_buffer_store_b64(u32x2{(uint32_t)nx.g.ilo, (uint32_t)(nx.g.ilo >> 32)}, r_nx, o8, 3u * c8,
                                                SAUX);
          st(col_rsrc(p.nx_ep, (uint32_t)N * 4u), off, 0, nx.k);
        }
      }
    }
  } else {
    bad = 0;
  }
#ifdef RMX_DIAG
  if (QRM && (p.diag & 131072)) {  // timing ablation: QRM lookups kept (registers), QRM stores dropped
    uint32_t keep = 0;
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
      for (int j = 0; j < (QXB > 0 ? QXB : 1); ++j) keep ^= qe[a][j].x ^ qe[a][j].y;
    if (keep == 0x7fffffffu) atomicOr(p.err, 2u);
  } else
#endif
  if constexpr (QRM) {  // QRM counterfactual experiences (rm_environment_wrapper.py:140-183)
    const int32_t Qx = p.n_qrm_max;
    const uint32_t nq_col = (uint32_t)Qx * (uint32_t)A * (uint32_t)N;
    const auto r_s = col_rsrc(p.qrm_s, nq_col * 4u), r_sn = col_rsrc(p.qrm_sn, nq_col * 4u);
    const auto r_rq = col_rsrc(p.qrm_rq, nq_col * 4u), r_dn = col_rsrc(p.qrm_done, nq_col);
#pragma unroll
    for (int a = 0; a < A; ++a) {
      const uint32_t nQ = (uint32_t)p.enc_nq[a];
      const uint32_t new_cell = (uint32_t)(s[a].y * p.W + s[a].x);
      const uint32_t env_term = (s[a].f >> 4) & 1u;  // RMX_F_ENV_TERM of this step
#pragma unroll
      for (int j = 0; j < QXB; ++j) {
        if (j >= Qx) continue;  // uniform
        const bool valid = j < p.n_qrm[a];  // missing states of a shorter RM: (-1, -1, 0, 0)
        const uint32_t so = (uint32_t)(a * Qx + j) * (uint32_t)N;
        const int32_t s_enc = valid ? (int32_t)(prev_cell[a] * nQ + p.qrm_q[a][j]) : -1;
        const int32_t sn_enc = valid ? (int32_t)(new_cell * nQ + (qe[a][j].x & 0xFFu)) : -1;
        const uint32_t dn = valid ? (env_term | ((qe[a][j].x >> 8) & 1u)) : 0u;
        if (live) {
          st(r_s, off, so * 4u, s_enc);
          st(r_sn, off, so * 4u, sn_enc);
          st(r_rq, off, so * 4u, valid ? (int32_t)qe[a][j].y : 0);
          __builtin_amdgcn_raw_buffer_store_b8((uint8_t)dn, r_dn, (uint32_t)e, so, kStoreAux);
        }
      }
    }
  }
  if (__any(bad)) {
    if ((tid & 63) == 0) atomicOr(p.err, 1u);
  }
#ifdef RMX_DIAG
  STAMP(7);
  if (!(diag & 1)) {
#endif
  if constexpr (!STATS_FIRST) flush_stats();
#ifdef RMX_DIAG
  }
  STAMP(8);
  if (p.stamps && (tid & 63) == 0) {
    unsigned long long* w = p.stamps + (((size_t)blockIdx.x * blockDim.x + tid) >> 6) * (2 * kStamps);
#pragma unroll
    for (int i = 0; i < kStamps; ++i) {
      w[i] = st_clk[i];
      w[kStamps + i] = st_rt[i];
    }
  }
#endif
  if constexpr (RPT) {  // the env's slot values after this step's adds (the same f64 add the atomic performs)
    double rs = 0.0;
    uint32_t sc = 0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
      rs += (double)s[a].ret;
      sc += o[a].succ;
    }
    report_tail(p, rin, done, rs, sc, t1);
  }
  // A hand-off packet has no release fence behind it: each storing wave waits here until its record stores and its
  // atomics have completed (gfx9: stores count in vmcnt), so they are in memory when the last wave has ended.
  if constexpr (OUT_PK) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
