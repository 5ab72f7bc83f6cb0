"""GPU parity at the field-width and table-mode limits of the step kernels.

The rest of the suite sits in one corner of the parameter space: RM states <= 9, events <= 8, x / y <= 13, at most 4
agents, and reward sets that either never reach the 4-B merged records or reach them with one small positive palette.
This module puts the other corners under test:

* LIMIT WORLDS (`CASES`): 5 / 7 / 8 agents, ~250 RM states, 160 / 250 events, 255-wide and 255-high grids on the fast
  path, 256-wide and 4,096-cell grids on the generic one, generated so that the high values are actually used (the
  liveness conditions of `liveness()` are asserted on the oracle's trajectory in every test that steps a world);
* the reference-recorded limit goldens (tests/golden/gen_golden.py: 200-state chains with 1 and 8 agents, negative
  and two-palette 4-B records, 5 rewards, 16 / 17 QRM states) in every kernel mode;
* palette edges and size edges of the table-mode selection, one world on each side of every threshold.

Every row asserts `VecRMEnv.step_info` (rmx_step_info) against `expected_info`, a restatement of rmx_create's selection
rules (the size formulas of build_fast_blob / build_merged / build_table_blob, the eligibility rule of build_compact)
computed from the tables alone, never read back from the engine.  Bar: integer columns, flags, env_done, rewards, renv
and enc_state bit-exact against the CPU oracle; ep_ret and statistics as in tests/test_random_maps_gpu.py; goldens
bit-exact / <= 1e-6 as in tests/test_engine_gpu.py.

The world generator, the oracle runs and `expected_info` need no GPU: tests/test_limits_cpu.py uses them for the
host path, the plain-Python stepper and the liveness measurements.
"""
import functools
import os

import numpy as np
import pytest

import oracle as O
from rmx import tables as T
from rmx._capi import F_ACTIVE, F_ENV_DONE, F_TERM, F_TRUNC

pytestmark = pytest.mark.gpu

N_ENVS, N_STEPS, CHECK_EVERY = 1500, 150, 25
REWARD_TOL = 1e-6
KNOBS = ("RMX_FAST", "RMX_FAST_TABLES", "RMX_FAST_STATS", "RMX_FAST_SKIP", "RMX_GENERIC_SKIP", "RMX_LAYOUT",
         "RMX_ROLLOUT_LDS", "RMX_BLOCK")
MODES = {
    "default": {},
    "global": {"RMX_FAST_TABLES": "global"},
    "merged": {"RMX_FAST_TABLES": "merged"},
    "merged4": {"RMX_FAST_TABLES": "merged4"},
    "nt": {"RMX_FAST_SKIP": "3"},
    "wave_stats": {"RMX_FAST_STATS": "wave"},
    "generic": {"RMX_FAST": "0"},
    "generic_skip": {"RMX_FAST": "0", "RMX_GENERIC_SKIP": "1"},
    "generic_lpe": {"RMX_FAST": "0", "RMX_LAYOUT": "lpe"},
}
FAST_MODES = ["default", "global", "merged", "merged4", "nt", "wave_stats", "generic", "generic_skip", "generic_lpe"]
GENERIC_MODES = ["default", "generic_skip", "generic_lpe"]


# --------------------------------------------------------------------------------------------------------------
# Limit worlds
# --------------------------------------------------------------------------------------------------------------
def _label(k):
    return f"s{k:03d}"  # zero-padded: the sorted() state order is the numeric one, index == k


def _limit_rm(rng, Q, ev_cells, rewards, q_high, final_p, none_p=0.1):
    """A random RM over s000..s{Q-1}; s{Q-1} is the final state (to_state of the last inserted transition).  With
    q_high four out of five transitions lead into states >= 128, so an agent spends its episode there."""
    tr = {}

    def dst():
        if q_high and rng.random() < 0.8:
            return int(rng.integers(128, Q - 1))
        return int(rng.integers(0, Q - 1))

    for q in range(Q - 1):
        if q == 0:
            evs = list(ev_cells)
        else:
            order = rng.permutation(len(ev_cells))
            evs = [ev_cells[i] for i in order[: int(rng.integers(1, 4))]]
        for ev in evs:  # (the initial state leaves on every event: the high region is entered early)
            to = Q - 1 if rng.random() < final_p else dst()
            tr[(_label(q), tuple(ev))] = (_label(to), float(rewards[rng.integers(len(rewards))]))
        if rng.random() < none_p:
            tr[(_label(q), None)] = (_label(dst()), float(rewards[rng.integers(len(rewards))]))
    src = int(rng.integers(128, Q - 1)) if q_high else int(rng.integers(0, Q - 1))
    tr.pop((_label(src), tuple(ev_cells[0])), None)
    tr[(_label(src), tuple(ev_cells[0]))] = (_label(Q - 1), float(rewards[0]))  # inserted last: s{Q-1} is final
    return T.RewardMachineSpec(tr, initial_state=_label(0))


def make_world(seed, kind, W, H, A, Q, n_ev, zone, rewards, modifier=1.0, shaping=False, max_t=60, q_high=False,
               n_low_ev=0, hazard_div=12, wall_p=0.12, hazard_fail=None, wall_fail=False, final_p=0.05,
               detect_all=False, none_p=0.1):
    """The unpacked description (tests/pyref.py's world dict) of a limit world.

    `zone` = (x0, y0, x1, y1) is where the agents start and where the events are, so that an episode of max_t steps
    stays in it: a zone at high x / y / cell index is how the high coordinates get used.  Event ids follow the sorted
    order of the event cells (x-major), so with `n_low_ev` the lowest-sorted cells OUTSIDE the zone (it must then span
    the highest columns) take the ids 1..n_low_ev and every event inside the zone has an id above them."""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = zone
    hot = [(x, y) for x in range(x0, x1 + 1) for y in range(y0, y1 + 1)]
    hot_set = set(hot)
    ev_low = [c for c in sorted((x, y) for x in range(W) for y in range(H)) if c not in hot_set][:n_low_ev]
    assert len(ev_low) == n_low_ev and (not ev_low or max(ev_low) < min(hot))
    perm = rng.permutation(len(hot))
    n_hot = n_ev - n_low_ev
    ev_hot = [hot[i] for i in perm[:n_hot]]
    rest = [hot[i] for i in perm[n_hot:]]
    assert len(rest) >= A, "the zone must hold the starts"
    starts = rest[:A]
    n_haz = min(len(rest) - A, len(hot) // hazard_div) if hazard_div else 0
    hazards = rest[A: A + n_haz]
    walls = []
    if kind == T.OFFICE_WORLD:
        for x in range(max(0, x0 - 1), min(W, x1 + 2)):
            for y in range(max(0, y0 - 1), min(H, y1 + 2)):
                for nx, ny in ((x + 1, y), (x, y + 1)):
                    if nx < W and ny < H and rng.random() < wall_p:
                        walls += [((x, y), (nx, ny)), ((nx, ny), (x, y))]
    detectors = []
    for _ in range(A):
        d = list(ev_low) + [c for c in ev_hot if detect_all or rng.random() < 0.85]
        detectors.append(d if len(d) > n_low_ev else list(ev_low) + ev_hot[:1])
    rms = [_limit_rm(rng, Q, [c for c in detectors[a] if c in hot_set], rewards, q_high, final_p, none_p)
           for a in range(A)]
    if shaping:
        for rm in rms:
            rm.add_reward_shaping(0.9, 0.9)
    return {"kind": "frozen_lake" if kind == T.FROZEN_LAKE else "office_world", "width": W, "height": H,
            "hazards": set(hazards), "walls": set(walls), "starts": starts, "rms": rms,
            "detectors": [set(d) for d in detectors], "hazard_penalty": -1.5, "wall_penalty": -0.25,
            "hazard_fail": True if kind == T.FROZEN_LAKE else bool(hazard_fail), "wall_fail": bool(wall_fail),
            "reward_modifier": modifier, "max_t": max_t, "shaping_gamma": 0.9 if shaping else None, "gamma": 0.95}


def compile_world(w, **extra):
    kind = T.FROZEN_LAKE if w["kind"] == "frozen_lake" else T.OFFICE_WORLD
    return T.compile_tables(kind, w["width"], w["height"], sorted(w["hazards"]), sorted(w["walls"]), w["starts"],
                            w["rms"], [sorted(d) for d in w["detectors"]], hazard_penalty=w["hazard_penalty"],
                            wall_penalty=w["wall_penalty"], hazard_fail=w["hazard_fail"], wall_fail=w["wall_fail"],
                            gamma=w["gamma"], shaping_gamma=w["shaping_gamma"], reward_modifier=w["reward_modifier"],
                            max_t=w["max_t"], **extra)


FRACT = (1.0, 2.5, -1.0, 0.75)  # rewards off the integer grid (with reward_modifier 1.5): never 4-B records
NEG = (-128.0, 127.0, -3.0)     # with the implicit 0 exactly four integers: 4-B records, both ends of the byte
FL, OW = T.FROZEN_LAKE, T.OFFICE_WORLD
# name: (target field, fast path?, make_world arguments).  The fractions in the comments are the liveness measured on
# the oracle's trajectory at 1,500 envs x 150 steps (share of the (step, env, agent) samples with the target >= 128;
# for the A > 4 worlds the share of samples in which only the last agent is still active).
CASES = {
    # generic and lane-per-agent kernels with 3 / 1 / 0 idle lanes per env; every agent index moves, is paid by its RM,
    # ends episodes both ways; only the last agent active in 0.039 (a5_fl), 0.019 (a7_ow), 0.022 (a8_ow_shaping) and
    # 0.0059 (a8_fl) of the samples
    "a5_fl": ("agents", False, dict(seed=11, kind=FL, W=8, H=7, A=5, Q=5, n_ev=8, zone=(0, 0, 7, 6), rewards=FRACT,
                                    modifier=1.5, max_t=40, final_p=0.3)),
    "a7_ow": ("agents", False, dict(seed=12, kind=OW, W=9, H=8, A=7, Q=5, n_ev=9, zone=(0, 0, 8, 7), rewards=FRACT,
                                    modifier=1.5, max_t=40, final_p=0.3, hazard_fail=True, wall_fail=True,
                                    hazard_div=6)),
    "a8_ow_shaping": ("agents", False, dict(seed=13, kind=OW, W=10, H=8, A=8, Q=6, n_ev=10, zone=(0, 0, 9, 7),
                                            rewards=FRACT, modifier=1.5, shaping=True, max_t=40, final_p=0.3,
                                            hazard_fail=True, wall_fail=True, hazard_div=6)),
    "a8_fl": ("agents", False, dict(seed=14, kind=FL, W=8, H=8, A=8, Q=5, n_ev=8, zone=(0, 0, 7, 7), rewards=FRACT,
                                    modifier=1.5, max_t=40, final_p=0.3)),
    # 250 RM states: one agent on the fast path (fast blob 13.4 KB; one merged section 160,000 B > 128 KiB: global by
    # default, 16-B and 4-B records when forced), two agents past the 16-KiB fast blob.  rm_q >= 128 in 0.79 / 0.80 of
    # the samples, state 249 reached
    "q250_a1_fast": ("q", True, dict(seed=21, kind=FL, W=4, H=2, A=1, Q=250, n_ev=2, zone=(0, 0, 3, 1), rewards=NEG,
                                     q_high=True, hazard_div=0, detect_all=True)),
    "q250_a2_generic": ("q", False, dict(seed=22, kind=OW, W=6, H=5, A=2, Q=250, n_ev=6, zone=(0, 0, 5, 4),
                                         rewards=FRACT, modifier=1.5, shaping=True, q_high=True, detect_all=True)),
    # 160 events on the fast path (fast blob 16,336 B of 16,384), 250 on the generic one (table blob ~46 KB).  Detected
    # event id >= 128 in 0.29 / 0.81 of the samples, the last id reached
    "e160_a1_fast": ("ev", True, dict(seed=31, kind=FL, W=16, H=15, A=1, Q=4, n_ev=159, zone=(12, 0, 15, 14),
                                      rewards=NEG, n_low_ev=127, detect_all=True, hazard_div=30)),
    "e250_a2_generic": ("ev", False, dict(seed=32, kind=OW, W=16, H=16, A=2, Q=10, n_ev=249, zone=(8, 0, 15, 15),
                                          rewards=FRACT, modifier=1.5, shaping=True, n_low_ev=127, detect_all=True,
                                          hazard_div=40)),
    # x and y at the last fast-path width / height, and one past it.  x (y) >= 128 in every sample, W - 1 (H - 1)
    # reached
    "w255_h2_fast": ("x", True, dict(seed=41, kind=FL, W=255, H=2, A=1, Q=4, n_ev=14, zone=(235, 0, 254, 1),
                                     rewards=(1.0, 3.0, -2.0), hazard_div=40)),
    "w2_h255_fast": ("y", True, dict(seed=42, kind=FL, W=2, H=255, A=1, Q=4, n_ev=14, zone=(0, 235, 1, 254),
                                     rewards=(1.0, 3.0, -2.0), hazard_div=40)),
    "w256_h2": ("x", False, dict(seed=43, kind=FL, W=256, H=2, A=2, Q=4, n_ev=14, zone=(236, 0, 255, 1),
                                 rewards=FRACT, modifier=1.5, hazard_div=40)),
    # 4,096 cells, square and as one row.  Cell index >= 2,048 in every sample, cell 4,095 reached
    "cells4096_sq": ("cell", False, dict(seed=51, kind=OW, W=64, H=64, A=2, Q=5, n_ev=12, zone=(52, 52, 63, 63),
                                         rewards=FRACT, modifier=1.5, shaping=True, hazard_div=40)),
    "cells4096_row": ("cell", False, dict(seed=52, kind=FL, W=4096, H=1, A=2, Q=5, n_ev=12, zone=(4056, 0, 4095, 0),
                                          rewards=FRACT, modifier=1.5, hazard_div=40)),
}
# slip and random starts at the limits: compile_tables options on top of a case, the RMX_* settings and the kernel that
# must run.  8 agents and 250 states x 2 agents: the generic kernel, rng columns, no reset cache.  On the fast path
# (merged records forced: these worlds' tables are past the default's 128 KiB) the 250-state machine under slip with
# the fixed-seed reset cache and with a reseed per episode, and random starts over a 255-wide and a 255-high lake, whose
# cached start cells are x | y << 8 bytes.
RNG_CASES = {
    "a8_fl_slip": ("a8_fl", dict(stochastic=True, seed_schedule=(1000, 1000, 1)), {}, "generic"),
    "a8_fl_slip_skip": ("a8_fl", dict(stochastic=True, seed_schedule=(1000, 1000, 1)), MODES["generic_skip"],
                        "generic"),
    "a8_fl_randstart": ("a8_fl", dict(random_starts=True, seed_schedule=(1000, 1000, 1)), {}, "generic"),
    "q250_a2_slip": ("q250_a2_generic", dict(stochastic=True, seed_schedule=(1000, 1000, 1)), {}, "generic"),
    "q250_a1_slip_cache": ("q250_a1_fast", dict(stochastic=True, seed_schedule=(1, 1, 0)), MODES["merged"], "fast"),
    "q250_a1_slip_reseed": ("q250_a1_fast", dict(stochastic=True, seed_schedule=(1, 1, 1)), MODES["merged"], "fast"),
    "w255_randstart_cache": ("w255_h2_fast", dict(random_starts=True, seed_schedule=(1, 1, 0)), MODES["merged4"],
                             "fast"),
    "h255_randstart_slip_cache": ("w2_h255_fast", dict(random_starts=True, stochastic=True, seed_schedule=(1, 1, 0)),
                                  MODES["merged"], "fast"),
}


@functools.lru_cache(maxsize=None)
def rng_reference(case, n=N_ENVS):
    base, extra, _, _ = RNG_CASES[case]
    tab = compile_world(limit_world(base)[0], **extra)
    hi = 4 if tab.stochastic and tab.kind == T.FROZEN_LAKE else 5  # FrozenLake's slip map has no wait
    acts = np.random.default_rng(7).integers(0, hi, size=(N_STEPS, tab.n_agents, n), dtype=np.int32)
    return tab, acts, oracle_run(tab, acts, seed=31)


def check_rng_liveness(case, tab, ref):
    """The limit is still reached under slip / random starts, and the envs' generators have diverged."""
    tr = ref["traj"]
    assert len(np.unique(ref["snaps"][N_STEPS - 1]["rng"][1])) > tr["rm_q"].shape[2] // 2
    if case.startswith("q250"):
        assert (tr["rm_q"] >= 128).mean() >= 0.10
    if case.startswith("w255"):
        assert (tr["pos_x"] >= 128).mean() >= 0.10 and tr["pos_x"].max() == 254
    if case.startswith("h255"):
        assert (tr["pos_y"] >= 128).mean() >= 0.10 and tr["pos_y"].max() == 254


@functools.lru_cache(maxsize=None)
def limit_world(case):
    """(world description, compiled tables) of a CASES entry; built once per process and never modified."""
    w = make_world(**CASES[case][2])
    return w, compile_world(w)


def case_actions(case, n=N_ENVS, steps=N_STEPS):
    A = limit_world(case)[1].n_agents
    rng = np.random.default_rng(CASES[case][2]["seed"] + 100)
    return rng.integers(0, 5, size=(steps, A, n), dtype=np.int32)  # 4 = wait


def oracle_run(tab, acts, seed=123, snap_every=CHECK_EVERY):
    """The oracle stepped over acts [T, A, N]: per-step pos_x / pos_y / rm_q / flags (the liveness input), the full
    column set every `snap_every` steps and after the last one, and the final statistics."""
    Tn, A, N = acts.shape
    orc = O.OracleEnv(tab, N)
    orc.reset(seed=seed)
    traj = {k: np.zeros((Tn, A, N), np.int32) for k in ("pos_x", "pos_y", "rm_q")}
    traj["flags"] = np.zeros((Tn, A, N), np.uint32)
    traj["reward"] = np.zeros((Tn, A, N), np.float32)
    traj["renv"] = np.zeros((Tn, A, N), np.float32)
    snaps = {}
    for s in range(Tn):
        orc.step(acts[s])
        for k in traj:
            traj[k][s] = getattr(orc, k)
        if s % snap_every == snap_every - 1 or s == Tn - 1:
            cols = ("pos_x", "pos_y", "rm_q", "t", "flags", "env_done", "reward", "renv", "enc_state", "ep_ret",
                    "shaping")
            snaps[s] = {k: getattr(orc, k).copy() for k in cols}
            if orc.rng is not None:
                snaps[s]["rng"] = orc.rng.copy()
    return {"traj": traj, "snaps": snaps, "stats": orc.stats.copy()}


@functools.lru_cache(maxsize=None)
def case_reference(case):
    tab = limit_world(case)[1]
    return oracle_run(tab, case_actions(case))


def liveness(case, tab, traj):
    """The figures that show a run reached the limit it is there for (asserted by check_liveness)."""
    target = CASES[case][0]
    x, y, q, f = traj["pos_x"], traj["pos_y"], traj["rm_q"], traj["flags"]
    A = tab.n_agents
    out = {}
    if target == "q":  # (and the last state index itself is reached)
        out["frac_q_ge_128"], out["top"] = float((q >= 128).mean()), [int(q.max()) == tab.n_rm_states - 1]
    elif target == "ev":
        ev = np.stack([tab.cell_event[a][(y[:, a] * tab.width + x[:, a])] for a in range(A)], axis=1)
        out["frac_ev_ge_128"], out["top"] = float((ev >= 128).mean()), [int(ev.max()) == tab.n_events - 1]
    elif target == "x":
        out["frac_x_ge_128"], out["top"] = float((x >= 128).mean()), [int(x.max()) == tab.width - 1]
    elif target == "y":
        out["frac_y_ge_128"], out["top"] = float((y >= 128).mean()), [int(y.max()) == tab.height - 1]
    elif target == "cell":
        cell = y * tab.width + x
        out["frac_cell_ge_2048"], out["top"] = float((cell >= 2048).mean()), [int(cell.max()) == 4095]
    else:
        active = (f & F_ACTIVE) != 0
        done = (f & F_ENV_DONE) != 0
        out["moves"] = [bool((np.diff(x[:, a], axis=0) != 0).any() or (np.diff(y[:, a], axis=0) != 0).any())
                        for a in range(A)]
        out["rm_reward"] = [bool(((traj["reward"][:, a] - traj["renv"][:, a]) != 0).any()) for a in range(A)]
        # an episode's end by termination (every agent terminated, none truncated) and by truncation
        out["ends_term"] = [bool((done[:, a] & ((f[:, a] & F_TERM) != 0) & ((f[:, a] & F_TRUNC) == 0)).any())
                            for a in range(A)]
        out["ends_trunc"] = [bool((done[:, a] & ((f[:, a] & F_TRUNC) != 0)).any()) for a in range(A)]
        out["frac_only_last_active"] = float((active[:, A - 1] & ~active[:, : A - 1].any(axis=1)).mean())
    return out


def check_liveness(case, tab, traj):
    lv = liveness(case, tab, traj)
    for k, v in lv.items():
        if k.startswith("frac_") and k != "frac_only_last_active":
            assert v >= 0.10, (case, lv)
        elif k == "frac_only_last_active":
            assert v > 0, (case, lv)
        else:
            assert all(v), (case, k, lv)
    return lv


# --------------------------------------------------------------------------------------------------------------
# rmx_create's selection rules, restated from the tables alone
# --------------------------------------------------------------------------------------------------------------
FAST_BLOB_MAX, MERGED_DEFAULT_MAX, MERGED_MAX, GENERIC_BLOB_MAX = 16 * 1024, 128 * 1024, 2 << 20, 64 * 1024


def _a16(n):
    return (n + 15) & ~15


def n_qrm_max(tab):
    return int(tab.qrm_states.shape[1]) if tab.n_qrm is not None and int(tab.n_qrm.max()) > 0 else 0


def generic_blob_bytes(tab):
    """build_table_blob: [cell u16][cell_event u8][next_q u8][rm_reward f32][shape f32][qrm_states u8], 16-B aligned."""
    A, Q, E, HW = tab.n_agents, tab.n_rm_states, tab.n_events, tab.width * tab.height
    n = _a16(2 * HW)
    n = _a16(n + A * HW)
    n = _a16(n + A * Q * E)
    n = _a16(n + 4 * A * Q * E)
    if tab.shape is not None:
        n = _a16(n + 4 * A * Q * E)
    if n_qrm_max(tab) > 0:
        n = _a16(n + A * n_qrm_max(tab))
    return n


def fast_blob_bytes(tab):
    """build_fast_blob: one u32 move word per (agent, cell, action), one 16-B RM entry per (agent, q, event), 16 B of
    info per agent."""
    A, Q, E, HW = tab.n_agents, tab.n_rm_states, tab.n_events, tab.width * tab.height
    return _a16(4 * A * HW * 5) + 16 * A * Q * E + 16 * A


def fast_eligible(tab, n_envs):
    if tab.n_agents > 4 or max(tab.width, tab.height, tab.n_events, tab.n_rm_states) > 255:
        return False
    if tab.n_agents * n_envs >= 1 << 30:
        return False
    return fast_blob_bytes(tab) + 4 * 128 + 4 * 3 * 64 <= FAST_BLOB_MAX


def _section_key(tab, a):
    """What build_merged stores for agent a: per (q, cell, action) the destination, its wall / hazard / fail bits, the
    RM successor with its final bit, the scaled reward and the shaping term of the event at the destination."""
    W, H, HW = tab.width, tab.height, tab.width * tab.height
    up = -1 if tab.kind == T.FROZEN_LAKE else 1
    dest = np.zeros((HW, 5), np.int64)
    bits = np.zeros((HW, 5), np.int64)
    for c in range(HW):
        x, y = c % W, c // W
        for ac, (dx, dy) in enumerate(((0, up), (0, -up), (-1, 0), (1, 0), (0, 0))):
            can = ac < 4 and bool((int(tab.cell[c]) >> ac) & 1)
            wall = tab.kind == T.OFFICE_WORLD and ac < 4 and not can
            nc = (y + dy) * W + (x + dx) if can else c
            haz = bool(int(tab.cell[nc]) & T.HAZARD)
            fail = haz if tab.kind == T.FROZEN_LAKE else bool((wall and tab.wall_fail) or (haz and tab.hazard_fail))
            dest[c, ac], bits[c, ac] = nc, wall | (haz << 1) | (fail << 2)
    ev = tab.cell_event[a].astype(np.int64)[dest]  # [HW, 5]
    nq = tab.next_q[a].astype(np.int64)[:, ev]  # [Q, HW, 5]
    rw = (np.float32(tab.reward_modifier) * tab.rm_reward[a])[:, ev].astype(np.float32)
    sh = tab.shape[a][:, ev].astype(np.float32) if tab.shape is not None else np.zeros_like(rw)
    word0 = dest[None] | (nq << 16) | (bits[None] << 24) | ((nq == int(tab.final_q[a])).astype(np.int64) << 27)
    return word0.tobytes() + rw.tobytes() + sh.tobytes(), rw


def merged_layout(tab):
    """build_merged: (fits, stored sections, bytes of the 16-B records, per stored section the reward words)."""
    sec_bytes = tab.n_rm_states * tab.width * tab.height * 5 * 16
    if sec_bytes > MERGED_MAX:
        return False, 0, 0, []
    keys, rws = [], []
    for a in range(tab.n_agents):
        k, rw = _section_key(tab, a)
        if k not in keys:
            if (len(keys) + 1) * sec_bytes > MERGED_MAX:
                return False, 0, 0, []
            keys.append(k)
            rws.append(rw)
    return True, len(keys), len(keys) * sec_bytes, rws


def compact_eligible(tab, rws):
    """build_compact: no shaping; per stored section at most 4 distinct reward bit patterns, each an integer in
    [-128, 127] and not -0.0."""
    if tab.shape is not None:
        return False
    for rw in rws:
        pal = np.unique(rw.view(np.uint32))
        if len(pal) > 4:
            return False
        for bitsv in pal:
            v = float(np.array([bitsv], np.uint32).view(np.float32)[0])
            if not (-128.0 <= v <= 127.0 and v == int(v)) or (v == 0.0 and bitsv >> 31):
                return False
    return True


def expected_info(tab, n_envs, env=None, with_qrm=False):
    """The step_info a device handle must report for these tables under the RMX_* settings in `env`."""
    env = env or {}
    rng_on = bool(tab.stochastic or tab.random_starts)
    lpe = env.get("RMX_LAYOUT") == "lpe" and not rng_on
    rollout_lpe = lpe or (not rng_on and env.get("RMX_LAYOUT") != "tpe")
    fast = env.get("RMX_FAST", "1") != "0" and not lpe and fast_eligible(tab, n_envs)
    ok, n_sec, bytes16, rws = merged_layout(tab) if fast else (False, 0, 0, [])
    tables = "global"
    if fast and ok and bytes16 <= MERGED_DEFAULT_MAX:
        tables = "merged" if tab.stochastic else "merged4"
    tables = env.get("RMX_FAST_TABLES", tables)
    want_m4 = tables == "merged4"
    if fast and tables in ("merged", "merged4") and not ok:
        tables = "global"
    m4_bytes = 0
    if fast and want_m4 and tables != "global":
        if compact_eligible(tab, rws):
            m4_bytes = bytes16 // 4
        else:
            tables = "merged"
    if tables == "global":
        n_sec = bytes16 = 0
    store = int(env.get("RMX_FAST_SKIP", 3 if n_envs * tab.n_agents >= 1 << 23 else 2))
    qx = n_qrm_max(tab)
    qrm = bool(with_qrm and qx > 0)
    seed_fixed = fast and rng_on and tab.seed_schedule[2] == 0
    if fast and rng_on:  # the SLIP instantiations: merged records, the small-N store mode, one-byte shuffle rows
        n_free = tab.width * tab.height - int(((tab.cell & T.HAZARD) != 0).sum())
        applies = not qrm and store == 2 and tables in ("merged", "merged4") and \
            (not tab.random_starts or seed_fixed or n_free + 8 <= 192)
    else:
        applies = fast and (not qrm or qx <= (16 if tab.n_agents <= 2 else 8))
    if applies:
        step_tables = "global" if qrm else tables
        info = {"variant": "fast", "tables": step_tables,
                "record_bytes": {"merged": 16, "merged4": 4}.get(step_tables, 0),
                "store_mode": store, "wave_stats": int(env.get("RMX_FAST_STATS") == "wave" or n_envs >= 1 << 20),
                "block": 256 if n_envs >= 1 << 20 else 64, "qrm_fast": int(qrm)}
    else:
        info = {"variant": "lane_per_agent" if lpe else "generic", "tables": "none", "record_bytes": 0,
                "store_mode": int(env.get("RMX_GENERIC_SKIP", n_envs >= 1 << 20)), "wave_stats": 1,
                "block": int(env.get("RMX_BLOCK", 256)), "qrm_fast": 0}
    info.update({"merged_sections": n_sec if fast else 0, "merged_bytes": bytes16 if fast else 0,
                 "merged4_bytes": m4_bytes, "fast_blob_bytes": fast_blob_bytes(tab) if fast else 0,
                 "generic_blob_bytes": generic_blob_bytes(tab),
                 "seed_fixed": int(seed_fixed),
                 "rollout_layout": "lane_per_agent" if rollout_lpe else "thread_per_env"})
    return info


# --------------------------------------------------------------------------------------------------------------
# GPU tests
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch():
    import torch as _t
    assert _t.cuda.is_available(), "gpu tests need a ROCm device"
    return _t


def _set_mode(monkeypatch, mode):
    env = MODES[mode] if isinstance(mode, str) else mode
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return env


def _same_columns(env, snap, what):
    for k in ("pos_x", "pos_y", "rm_q", "t", "env_done", "reward", "renv", "enc_state"):
        np.testing.assert_array_equal(getattr(env, k).cpu().numpy(), snap[k], err_msg=f"{what} {k}")
    np.testing.assert_array_equal(env.flags.cpu().numpy().view(np.uint32), snap["flags"], err_msg=f"{what} flags")
    np.testing.assert_allclose(env.ep_ret.cpu().numpy(), snap["ep_ret"], rtol=1e-5, atol=1e-5)
    if env.shaping is not None:
        np.testing.assert_allclose(env.shaping.cpu().numpy(), snap["shaping"], rtol=0, atol=1e-6)
    if env.rng is not None:
        np.testing.assert_array_equal(env.rng.cpu().numpy().view(np.uint64), snap["rng"], err_msg=f"{what} rng")


def _same_stats(env, stats):
    env.check_errors()
    st = env.stats()
    assert st[1] == stats[1] and st[2] == stats[2] and st[3] == stats[3], (st, stats)
    np.testing.assert_allclose(st[0], stats[0], rtol=1e-5, atol=1e-4)


def _run_vs_reference(torch, tab, acts, ref, mode_env, with_qrm=False, seed=123):
    """One device handle stepped over acts, step_info against the restated rules, columns against the oracle's."""
    from rmx.engine import VecRMEnv

    Tn, A, N = acts.shape
    env = VecRMEnv(tab, N, with_enc_state=True, with_qrm=with_qrm)
    info, want = env.step_info, expected_info(tab, N, mode_env, with_qrm)
    assert info == want, {k: (info[k], want[k]) for k in want if info[k] != want[k]}
    assert env.step_variant == want["variant"]
    env.reset(seed=seed)
    dev = torch.as_tensor(acts, device="cuda")
    for s in range(Tn):
        env.step(dev[s])
        if s in ref["snaps"]:
            _same_columns(env, ref["snaps"][s], f"step {s}")
    _same_stats(env, ref["stats"])
    return env, info


def _case_modes():
    return [(c, m) for c in CASES for m in (FAST_MODES if CASES[c][1] else GENERIC_MODES)]


@pytest.mark.parametrize("case,mode", _case_modes())
def test_limit_world_vs_oracle(case, mode, torch, monkeypatch):
    """Every limit world in every kernel mode that applies to it: 1,500 envs x 150 caller-action steps (wait
    included) against the oracle, whose own trajectory must meet the world's liveness conditions."""
    mode_env = _set_mode(monkeypatch, mode)
    tab = limit_world(case)[1]
    ref = case_reference(case)
    check_liveness(case, tab, ref["traj"])
    _, info = _run_vs_reference(torch, tab, case_actions(case), ref, mode_env)
    if not CASES[case][1]:
        assert info["variant"] == ("lane_per_agent" if mode == "generic_lpe" else "generic")
    elif not mode.startswith("generic"):
        assert info["variant"] == "fast"


ROLLOUT_MODES = {
    "fast_lds": {}, "fast_l2": {"RMX_ROLLOUT_LDS": "0"},
    "merged_lds": {"RMX_FAST_TABLES": "merged"}, "merged_l2": {"RMX_FAST_TABLES": "merged", "RMX_ROLLOUT_LDS": "0"},
    "generic_tpe": {"RMX_FAST": "0", "RMX_LAYOUT": "tpe"}, "generic_lpe": {"RMX_FAST": "0", "RMX_LAYOUT": "lpe"},
}


@functools.lru_cache(maxsize=None)
def rollout_reference(case):
    tab = limit_world(case)[1]
    orc = O.OracleEnv(tab, N_ENVS)
    orc.rollout(9, 0, N_STEPS)
    return {k: getattr(orc, k).copy() for k in ("pos_x", "pos_y", "rm_q", "t", "flags", "ep_ret")}, orc.stats.copy()


def _rollout_modes():
    return [(c, m) for c in CASES for m in ROLLOUT_MODES if CASES[c][1] or m.startswith("generic")]


@pytest.mark.parametrize("case,mode", _rollout_modes())
def test_limit_world_rollout_equals_stepwise(case, mode, torch, monkeypatch):
    """The fused rollout (hashed actions) equals the same handle kind stepped one rmx_step_hashed at a time, and the
    oracle's rollout: on both layouts of the generic kernels, and with LDS-staged and L2-read tables on the fast one."""
    from rmx.engine import VecRMEnv

    mode_env = _set_mode(monkeypatch, ROLLOUT_MODES[mode])
    tab = limit_world(case)[1]
    a, b = VecRMEnv(tab, N_ENVS), VecRMEnv(tab, N_ENVS)
    want = expected_info(tab, N_ENVS, mode_env)
    assert a.step_info == want
    assert want["rollout_layout"] == ("thread_per_env" if mode == "generic_tpe" else "lane_per_agent")
    a.rollout(9, 0, N_STEPS)
    for s in range(N_STEPS):
        b.step_hashed(9, s)
    cols, stats = rollout_reference(case)
    for k in ("pos_x", "pos_y", "rm_q", "t", "flags"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
        np.testing.assert_array_equal(getattr(a, k).cpu().numpy().view(cols[k].dtype), cols[k], err_msg=k)
    np.testing.assert_allclose(a.ep_ret.cpu().numpy(), cols["ep_ret"], rtol=1e-5, atol=1e-5)
    _same_stats(a, stats)
    _same_stats(b, stats)


@pytest.mark.parametrize("case", list(CASES))
def test_limit_world_checkpoint_and_host(case, torch, monkeypatch):
    """A checkpoint taken at step 75 by the world's default kernel resumes bit-exactly in a fresh handle of another
    kernel family (fast -> generic, generic -> lane-per-agent) and in a host handle; both end where the oracle does."""
    from rmx.engine import HostRMEnv, VecRMEnv

    _set_mode(monkeypatch, "default")
    tab = limit_world(case)[1]
    acts, ref = case_actions(case), case_reference(case)
    dev = torch.as_tensor(acts, device="cuda")
    a = VecRMEnv(tab, N_ENVS, with_enc_state=True)
    for s in range(75):
        a.step(dev[s])
    blob = a.save_state()
    _set_mode(monkeypatch, "generic" if CASES[case][1] else "generic_lpe")
    b = VecRMEnv(tab, N_ENVS, with_enc_state=True)
    assert b.step_variant == ("generic" if CASES[case][1] else "lane_per_agent") != a.step_variant
    b.load_state(blob)
    h = HostRMEnv(tab, N_ENVS, with_enc_state=True)
    assert h.step_info["variant"] == "host" and set(h.step_info.values()) - {"host", "none", "thread_per_env"} == {0}
    h.load_state(blob)
    for s in range(75, N_STEPS):
        b.step(dev[s])
        h.step(acts[s])
    last = ref["snaps"][N_STEPS - 1]
    _same_columns(b, last, "resumed")
    _same_stats(b, ref["stats"])
    for k in ("pos_x", "pos_y", "rm_q", "t", "env_done", "reward", "renv", "enc_state"):
        np.testing.assert_array_equal(getattr(h, k), getattr(b, k).cpu().numpy(), err_msg=f"host {k}")
    np.testing.assert_allclose(h.ep_ret, b.ep_ret.cpu().numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_array_equal(h.flags, b.flags.cpu().numpy().view(np.uint32))
    np.testing.assert_array_equal(h.stats()[1:], b.stats()[1:])


@pytest.mark.parametrize("case", list(RNG_CASES))
def test_limit_world_slip_and_random_starts(case, torch, monkeypatch):
    """Slip and random starts at the limits (RNG_CASES) against the oracle with the rng columns: the generic kernel at
    8 agents and past the 16-KiB fast blob, where no fixed-seed reset cache exists (seed_fixed is a fast-path thing);
    the fast kernel's slip instantiation at 250 RM states and over 255-wide / 255-high lakes, with and without it."""
    _, extra, env_vars, variant = RNG_CASES[case]
    mode_env = _set_mode(monkeypatch, env_vars)
    tab, acts, ref = rng_reference(case)
    check_rng_liveness(case, tab, ref)
    env, info = _run_vs_reference(torch, tab, acts, ref, mode_env, seed=31)
    assert info["variant"] == variant and info["rollout_layout"] == "thread_per_env" and env.rng is not None
    assert info["seed_fixed"] == int(variant == "fast" and extra["seed_schedule"][2] == 0)


# ---- the reference-recorded limit goldens x modes ----------------------------------------------------------------
GOLDEN_MODES = {
    "fl8_chain200": ["default", "generic_skip", "generic_lpe"],
    "fl1_chain200": FAST_MODES, "fl2_negpal": FAST_MODES, "fl2_pal5": FAST_MODES,
    "fl1_qrm16": FAST_MODES + ["qrm", "qrm_generic"], "fl1_qrm17": FAST_MODES + ["qrm", "qrm_generic"],
}
MODES["qrm"] = {}
MODES["qrm_generic"] = {"RMX_FAST": "0"}


@pytest.mark.parametrize("name,mode", [(n, m) for n, ms in GOLDEN_MODES.items() for m in ms])
def test_limit_golden_matches_reference(name, mode, configs, golden_dir, torch, monkeypatch):
    """The limit goldens against the reference's recorded trajectories, with the comparison of
    test_engine_gpu.test_engine_matches_reference_golden, in every mode; step_info in every row."""
    from rmx.engine import VecRMEnv
    from test_oracle_golden import check_qrm

    mode_env = _set_mode(monkeypatch, mode)
    qrm = mode.startswith("qrm")
    g = dict(np.load(os.path.join(golden_dir, f"traj_{name}.npz")))
    tab = T.compile_scenario(configs[name])
    acts = torch.as_tensor(g["actions"].astype(np.int32), device="cuda")
    Tn, A, N = acts.shape
    env = VecRMEnv(tab, N, with_qrm=qrm)
    info, want = env.step_info, expected_info(tab, N, mode_env, qrm)
    assert info == want, {k: (info[k], want[k]) for k in want if info[k] != want[k]}
    fast_mode = mode in ("default", "global", "merged", "merged4", "nt", "wave_stats", "qrm")
    if name == "fl8_chain200":
        assert info["variant"] == ("lane_per_agent" if mode == "generic_lpe" else "generic")
    else:
        assert (info["variant"] == "fast") == (fast_mode and not (name == "fl1_qrm17" and qrm))
    if name == "fl2_negpal" and mode == "default":  # two stored sections with a palette each, 4-B records
        assert (info["tables"], info["record_bytes"], info["merged_sections"]) == ("merged4", 4, 2)
    if name == "fl2_pal5" and mode in ("default", "merged4"):  # five distinct rewards in one section: 16-B records
        assert (info["tables"], info["record_bytes"], info["merged_sections"], info["merged4_bytes"]) == \
            ("merged", 16, 2, 0)
    if name == "fl1_chain200" and mode in ("default", "merged4"):
        assert (info["tables"], info["record_bytes"], info["merged_sections"]) == ("merged4", 4, 1)
    if qrm:  # 16 counterfactual states: the last size the fast kernel serves; 17: the generic kernel
        assert info["qrm_fast"] == int(name == "fl1_qrm16" and mode == "qrm")
        assert info["variant"] == ("fast" if name == "fl1_qrm16" and mode == "qrm" else "generic")
    env.reset(seed=int(g["seed"]))
    np.testing.assert_array_equal(env.pos_x.cpu().numpy(), g["reset_xy"][0, 0])
    np.testing.assert_array_equal(env.pos_y.cpu().numpy(), g["reset_xy"][0, 1])
    keys = ["pos_x", "pos_y", "rm_q", "reward", "renv", "flags", "env_done", "t"] + \
        (["qrm_s", "qrm_sn", "qrm_rq", "qrm_done"] if env.qrm_s is not None else [])
    rec = {k: [] for k in keys}
    for s in range(Tn):
        env.step(acts[s])
        for k in keys:
            rec[k].append(getattr(env, k).clone())
    env.check_errors()
    r = {k: torch.stack(v).cpu().numpy() for k, v in rec.items()}
    np.testing.assert_array_equal(r["pos_x"], g["pos_x"])
    np.testing.assert_array_equal(r["pos_y"], g["pos_y"])
    np.testing.assert_array_equal(r["rm_q"], g["q"])
    np.testing.assert_array_equal((r["flags"] & F_TERM) != 0, g["term"])
    np.testing.assert_array_equal((r["flags"] & F_TRUNC) != 0, g["trunc"])
    np.testing.assert_array_equal((r["flags"] & F_ACTIVE) != 0, g["active"])
    np.testing.assert_array_equal(r["env_done"].astype(bool), g["env_done"])
    np.testing.assert_array_equal(r["t"], g["t"])
    assert np.max(np.abs(r["reward"].astype(np.float64) - g["reward"])) <= REWARD_TOL
    assert np.max(np.abs(r["renv"].astype(np.float64) - g["renv"])) <= REWARD_TOL
    assert np.max(np.abs(g["shaping"])) == 0.0  # (no limit golden has shaping)
    if "qrm_s" in r and "qrm_s" in g:
        check_qrm(tab, {**r, "q": r["rm_q"]}, g, g["actions"].astype(np.int32), r["renv"])


# ---- palette edges -------------------------------------------------------------------------------------------------
def palette_world(rewards0, rewards1=None, modifier=1.0, shaping=False):
    """A 5 x 4 lake without holes, three event cells, two agents whose RMs differ only in their rewards: a ring
    s0 -> s1 -> ... -> s0 over the events in turn that pays rewards[k] on leaving s_k, and one way out to the final
    state."""
    evs = [(1, 1), (3, 2), (2, 0)]

    def ring(rw):
        n = len(rw)
        tr = {(f"s{k}", evs[k % 3]): (f"s{(k + 1) % n}", rw[k]) for k in range(n)}
        tr[("s0", evs[2])] = ("sfin", rw[0])
        rm = T.RewardMachineSpec(tr, initial_state="s0")
        return rm

    rms = [ring(rewards0), ring(rewards0 if rewards1 is None else rewards1)]
    return T.compile_tables(T.FROZEN_LAKE, 5, 4, [], (), [(0, 0), (4, 3)], rms, [evs, evs], hazard_penalty=0.0,
                            reward_modifier=modifier, shaping_gamma=0.9 if shaping else None, max_t=60)


PALETTES = {
    # name: (palette_world arguments, record bytes, stored sections)
    "neg_3_distinct": (dict(rewards0=(-128.0, 127.0)), 4, 1),
    "neg_exactly_4": (dict(rewards0=(-128.0, -1.0, 127.0)), 4, 1),
    "five_distinct": (dict(rewards0=(1.0, 2.0, 3.0, 4.0)), 16, 1),
    "plus_128": (dict(rewards0=(128.0, 1.0)), 16, 1),
    "minus_129": (dict(rewards0=(-129.0, 1.0)), 16, 1),
    "half": (dict(rewards0=(0.5, 1.0)), 16, 1),
    "modifier_integer_product": (dict(rewards0=(2.0, -2.0), modifier=1.5), 4, 1),
    "modifier_fraction": (dict(rewards0=(1.0, 2.0), modifier=1.5), 16, 1),
    "negative_zero": (dict(rewards0=(-0.0, 2.0)), 16, 1),
    "shaping": (dict(rewards0=(1.0, 2.0), shaping=True), 16, 1),
    "two_palettes": (dict(rewards0=(-128.0, 127.0), rewards1=(-3.0, 5.0, 7.0)), 4, 2),
    "one_palette_too_many": (dict(rewards0=(-128.0, 127.0), rewards1=(1.0, 2.0, 3.0, 4.0)), 16, 2),
}


@functools.lru_cache(maxsize=None)
def palette_reference(name):
    tab = palette_world(**PALETTES[name][0])
    acts = np.random.default_rng(5).integers(0, 5, size=(N_STEPS, 2, N_ENVS), dtype=np.int32)
    return tab, acts, oracle_run(tab, acts)


def check_palette_liveness(name, tab, ref):
    """Every reward of both machines is paid in the oracle's run (so a wrong palette entry cannot hide)."""
    paid = ref["traj"]["reward"]
    for a, key in ((0, "rewards0"), (1, "rewards1")):
        rw = PALETTES[name][0].get(key) or PALETTES[name][0]["rewards0"]
        for r in rw:
            v = np.float32(np.float32(tab.reward_modifier) * np.float32(r))
            assert (paid[:, a] == v).any(), (name, a, r)


@pytest.mark.parametrize("forced", ["default", "merged4"])
@pytest.mark.parametrize("name", list(PALETTES))
def test_palette_edges(name, forced, torch, monkeypatch):
    """The reward sets at the edge of the 4-B records' palette (four signed bytes per stored section): which record
    size the handle runs, by default and with merged4 forced, and the oracle's rewards either way."""
    mode_env = _set_mode(monkeypatch, forced)
    tab, acts, ref = palette_reference(name)
    check_palette_liveness(name, tab, ref)
    _, info = _run_vs_reference(torch, tab, acts, ref, mode_env)
    _, rec_bytes, sections = PALETTES[name]
    assert (info["variant"], info["record_bytes"], info["merged_sections"]) == ("fast", rec_bytes, sections)
    assert info["tables"] == ("merged4" if rec_bytes == 4 else "merged")
    assert (info["merged4_bytes"] > 0) == (rec_bytes == 4)


# ---- size edges ----------------------------------------------------------------------------------------------------
def size_world(W, H, A, Q, n_ev=2, same_rm=True, shaping=False, kind=T.FROZEN_LAKE):
    """A world of exactly these table sizes: Q states in a ring over the n_ev event cells (integer rewards 1 / 2 / 3,
    so 4-B records are possible), agents started next to the events at the grid's far end."""
    cells = [(x, y) for y in range(H) for x in range(W)]
    evs = cells[-n_ev:]

    def ring(shift):
        tr = {(_label(k), evs[(k + shift) % n_ev]): (_label((k + 1) % (Q - 1)), float(1 + k % 3)) for k in range(Q - 1)}
        tr[(_label(0), evs[(shift + 1) % n_ev])] = (_label(Q - 1), 1.0)
        return T.RewardMachineSpec(tr, initial_state=_label(0))

    rms = [ring(0 if same_rm else a) for a in range(A)]
    starts = [cells[-n_ev - 1 - a] for a in range(A)]
    return T.compile_tables(kind, W, H, [], (), starts, rms, [evs] * A, hazard_penalty=0.0, max_t=40,
                            shaping_gamma=0.9 if shaping else None, gamma=0.95)


SIZE_EDGES = {
    # name: (size_world arguments, forced mode, (variant, tables, sections, 16-B record bytes))
    # the default keeps the merged table while it is at most 128 KiB (rmx_handle.h kFastMergedDefaultBytes)
    "merged_default_under": (dict(W=21, H=13, A=1, Q=6), "default", ("fast", "merged4", 1, 131040)),
    "merged_default_over": (dict(W=137, H=2, A=1, Q=6), "default", ("fast", "global", 0, 0)),
    # (64 KiB is no threshold of the default: both sides of it run the 4-B records)
    "merged_64k_under": (dict(W=17, H=12, A=1, Q=4), "default", ("fast", "merged4", 1, 65280)),
    "merged_64k_over": (dict(W=41, H=5, A=1, Q=4), "default", ("fast", "merged4", 1, 65600)),
    # a forced merged table must fit 2 MiB, per section ...
    "merged_max_under": (dict(W=131, H=4, A=1, Q=50), "merged", ("fast", "merged", 1, 2096000)),
    "merged_max_over": (dict(W=25, H=21, A=1, Q=50), "merged", ("fast", "global", 0, 0)),
    # ... and over all stored sections: two different RMs cross it, two identical ones share one section
    "merged_sum_shared": (dict(W=16, H=15, A=2, Q=56), "merged4", ("fast", "merged4", 1, 1075200)),
    "merged_sum_over": (dict(W=16, H=15, A=2, Q=56, same_rm=False), "merged4", ("fast", "global", 0, 0)),
    # the fast path's blob must fit 16 KiB (with its 1,280 B of staging slack): 16,368 B in, 16,400 B out
    "fast_blob_under": (dict(W=248, H=3, A=1, Q=4), "default", ("fast", "global", 0, 0)),
    "fast_blob_over": (dict(W=149, H=5, A=1, Q=4), "default", ("generic", "none", 0, 0)),
    # the generic kernels' blob must fit 64 KiB of LDS: 65,344 B runs (the over side: test_generic_blob_over_64k)
    "generic_blob_under": (dict(W=64, H=16, A=2, Q=113, n_ev=29, shaping=True, kind=T.OFFICE_WORLD), "default",
                           ("generic", "none", 0, 0)),
}
GENERIC_BLOB_OVER = dict(W=64, H=16, A=2, Q=114, n_ev=29, shaping=True, kind=T.OFFICE_WORLD)


@functools.lru_cache(maxsize=None)
def size_reference(name):
    tab = size_world(**SIZE_EDGES[name][0])
    acts = np.random.default_rng(3).integers(0, 5, size=(N_STEPS, tab.n_agents, N_ENVS), dtype=np.int32)
    return tab, acts, oracle_run(tab, acts)


def check_size_liveness(tab, ref):
    """The ring is walked and episodes end: RM rewards are paid and the RM leaves its initial state."""
    assert (ref["traj"]["rm_q"] > 0).mean() > 0.05 and ref["stats"][1] > 0


@pytest.mark.parametrize("name", list(SIZE_EDGES))
def test_size_edges(name, torch, monkeypatch):
    """A pair of worlds on either side of every size threshold of the table-mode selection."""
    _, forced, (variant, tables, sections, bytes16) = SIZE_EDGES[name]
    mode_env = _set_mode(monkeypatch, forced)
    tab, acts, ref = size_reference(name)
    check_size_liveness(tab, ref)
    _, info = _run_vs_reference(torch, tab, acts, ref, mode_env)
    assert (info["variant"], info["tables"], info["merged_sections"], info["merged_bytes"]) == \
        (variant, tables, sections, bytes16)
    if name == "fast_blob_under":
        assert info["fast_blob_bytes"] + 1280 == 16368
    if name == "generic_blob_under":
        assert info["generic_blob_bytes"] == 65344


def test_generic_blob_over_64k(torch):
    """One RM state more and the generic blob is 65,904 B: rmx_create refuses it and hands out no handle."""
    from rmx.engine import VecRMEnv

    tab = size_world(**GENERIC_BLOB_OVER)
    assert generic_blob_bytes(tab) == 65904 > GENERIC_BLOB_MAX
    with pytest.raises(ValueError, match="tables exceed 64 KiB of LDS"):
        VecRMEnv(tab, 64)
