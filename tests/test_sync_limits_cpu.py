"""The synchronous calls (rmx_reset_sync / rmx_step_sync / rmx_step_sync_begin + rmx_sync_wait) and get_mdp at the
engine's limits: the host-handle half, and what tests/test_sync_limits_gpu.py shares with it (nothing here needs a GPU).

A host handle serves the same entry points as the resident workgroup (host_sync_out, HostEngine::copy_out in
csrc/rmx_hoststep.cpp), so the shapes, the limit worlds, the QRM columns, the two-halves contract and get_mdp are put
against the CPU oracle here first; the GPU module then runs the same drivers on device handles, where the 16-byte
request word, the 32-byte output records and the per-bucket instantiations of csrc/rmx_sync.hip are.

Comparison rules (the project's): a synchronous handle against an asynchronous one of the same path is bit-exact in
every column; anything against the oracle has integers and flags exact and floats within REWARD_TOL = 1e-6; every
comparison includes enc_state, and shaping where the world has it.  The worlds are those of tests/test_limits_gpu.py
(CASES, RNG_CASES, SIZE_EDGES) and the goldens; tests/LIMITS.md lists which shape runs which instantiation."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle as O
import test_limits_gpu as L
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv
from test_oracle_golden import LIMIT_TRAJ, check_mdp, check_qrm

REWARD_TOL = L.REWARD_TOL
INT_COLS = ("pos_x", "pos_y", "rm_q", "flags", "t", "env_done", "enc_state")
FLOAT_COLS = ("reward", "renv", "ep_ret", "shaping")
QRM_COLS = ("qrm_s", "qrm_sn", "qrm_rq", "qrm_done")
RESET_COLS = ("pos_x", "pos_y", "rm_q", "flags", "t", "ep_ret")  # what a reset defines (enc_state: see below)
N_SYNC, K_SYNC, K_REQ = 65, 150, 60  # a partial second wave; steps of the limit-world runs; of the request-word runs

# ---- A. the shapes of the request word ------------------------------------------------------------------------------
# (A, N): N * A <= 15 travels inline (slots k = a * N + e: k < 7 in the ctl word, 7..14 in the acts word), 16 through
# the action array.  Worlds by agent count: goldens up to 4 agents, limit worlds past them.
REQUEST_SHAPES = [(1, 7), (1, 8), (4, 2), (8, 1), (4, 3), (2, 7), (7, 2), (1, 15), (3, 5), (5, 3), (1, 16), (2, 8),
                  (4, 4), (8, 2)]
# fl2_open's agents encode with 9 and 3 RM states, fl4_randstart_open's with 9 / 3 / 9 / 3: an enc_state word built with
# another agent's stride shows (every limit world's agents share one stride)
SHAPE_WORLD = {1: "ow1", 2: "fl2_open", 3: "ow3", 4: "fl4", (4, 3): "fl4_randstart_open", 5: "a5_fl", 7: "a7_ow",
               8: "a8_fl"}
INVALID_ACTIONS = (5, 15, 16, 20, -1, 2**31 - 1)  # 16 and 20: the low nibble is a valid action (0, 4)
INVALID_SHAPES = [(5, 3), (8, 2)]  # 15 actions: the last inline shape; 16: the first on the action array


def shape_tables(A, configs, N=None):
    name = SHAPE_WORLD.get((A, N), SHAPE_WORLD[A])
    return L.limit_world(name)[1] if name in L.CASES else T.compile_scenario(configs[name])


def n_action_values(tab):
    return 4 if tab.stochastic and tab.kind == T.FROZEN_LAKE else 5  # FrozenLake's slip map has no wait


def request_actions(tab, N, steps=K_REQ):
    """Actions [steps, A, N] over every value the world takes (wait included), and the proof that every slot of the
    request took every one of them during the run: a swapped or dropped nibble cannot hide behind equal actions."""
    hi = n_action_values(tab)
    acts = np.random.default_rng(1000 * tab.n_agents + N).integers(0, hi, size=(steps, tab.n_agents, N), dtype=np.int32)
    flat = acts.reshape(steps, -1)
    for k in range(flat.shape[1]):
        assert set(flat[:, k].tolist()) == set(range(hi)), (k, sorted(set(flat[:, k].tolist())))
    return acts


# ---- the oracle's side ----------------------------------------------------------------------------------------------
def expected_enc(tab, snap):
    """state_encoder's index (y * W + x) * nQ + q, restated from the columns (a reset defines it on the synchronous
    path; the oracle writes the column only when it steps)."""
    nq = np.asarray(tab.enc_nq, np.int64)[:, None]
    return ((snap["pos_y"].astype(np.int64) * tab.width + snap["pos_x"]) * nq + snap["rm_q"]).astype(np.int32)


def oracle_snapshot(orc, qrm=False):
    snap = {k: getattr(orc, k).copy() for k in INT_COLS + FLOAT_COLS}
    if orc.rng is not None:
        snap["rng"], snap["episode"] = orc.rng.copy(), orc.episode.copy()
    if qrm:
        snap.update({k: getattr(orc, k).copy() for k in QRM_COLS})
    return snap


def oracle_record(tab, acts, seed=123, reseed=None, qrm=False):
    """The oracle over acts [K, A, N] with the whole column set after every step (L.oracle_run keeps it every 25th),
    after the first reset and after the resets `reseed` = {step: new base seed} made before those steps."""
    orc = O.OracleEnv(tab, acts.shape[2])
    orc.reset(seed=seed)
    ref = {"snaps": {}, "resets": {-1: oracle_snapshot(orc)}}
    for s in range(acts.shape[0]):
        if reseed and s in reseed:
            orc.reset(seed=reseed[s])
            ref["resets"][s] = oracle_snapshot(orc)
        assert orc.step(acts[s]) == 0
        ref["snaps"][s] = oracle_snapshot(orc, qrm)
    ref["stats"] = orc.stats.copy()
    return ref


# ---- comparisons ----------------------------------------------------------------------------------------------------
def columns(env):
    """Every bound column of a handle as host arrays (a device handle's are copied back; its resident workgroup must
    have ended)."""
    out = {}
    for k in INT_COLS + FLOAT_COLS + QRM_COLS + ("rng", "episode"):
        v = getattr(env, k, None)
        if v is not None:
            v = v.cpu().numpy() if hasattr(v, "cpu") else v.copy()
            out[k] = v.view(np.uint32) if k == "flags" else v.view(np.uint64) if k == "rng" else v
    return out


def assert_bit_equal(got, want, where, keys=None):
    """Sync against async on the same path: the same env_step, so the same bits (floats compared as words)."""
    for k in keys or [k for k in got if k in want]:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize, (where, k)
        u = {1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        np.testing.assert_array_equal(a.view(u), b.view(u), err_msg=f"{where}: {k}")


def assert_vs_oracle(tab, got, snap, where, keys=None, qrm=False):
    """Integers and flags exact, floats within REWARD_TOL; a world with shaping must hand its shaping column out, every
    world its enc_state."""
    if keys is None:
        keys = INT_COLS + tuple(k for k in FLOAT_COLS if k != "shaping" or tab.shape is not None)
    for k in keys:
        want = expected_enc(tab, snap) if k == "enc_state" else snap[k]
        if k in FLOAT_COLS:
            err = np.max(np.abs(got[k].astype(np.float64) - want.astype(np.float64)))
            assert err <= REWARD_TOL, (where, k, err)
        else:
            np.testing.assert_array_equal(got[k], want, err_msg=f"{where}: {k}")
    if qrm:
        for a in range(tab.n_agents):  # (rows past an agent's own count belong to nobody)
            nq = int(tab.n_qrm[a])
            for k in ("qrm_s", "qrm_sn", "qrm_done"):
                np.testing.assert_array_equal(got[k][a, :nq], snap[k][a, :nq], err_msg=f"{where}: {k} agent {a}")
            err = np.max(np.abs(got["qrm_rq"][a, :nq].astype(np.float64) - snap["qrm_rq"][a, :nq]), initial=0.0)
            assert err <= REWARD_TOL, (where, "qrm_rq", a, err)


def assert_same_stats(s_env, a_env, ref_stats):
    """test_sync_equals_async's bar between the two handles; counts exact and the return sum as in
    tests/test_raw_capi_gpu.py against the oracle."""
    s_env.check_errors()
    ss, sa = s_env.stats(), a_env.stats()
    np.testing.assert_array_equal(ss[1:], sa[1:])
    np.testing.assert_allclose(ss[0], sa[0], rtol=1e-12)
    np.testing.assert_array_equal(ss[1:], ref_stats[1:])
    np.testing.assert_allclose(ss[0], ref_stats[0], rtol=1e-6, atol=1e-6)


def host_engine(tab, n, **kw):
    return HostRMEnv(tab, n, with_enc_state=True, **kw)


def run_sync(make, tab, acts, ref, seed=123, reseed=None, qrm=False, to_async=lambda a: a, between=None):
    """The driver of both modules.  Two handles from `make` (host or device): one stepped through reset_sync /
    step_sync, one through reset / step.  After every reset and every step the synchronous call's columns against the
    oracle's (`ref`: oracle_record's or L.oracle_run's with snap_every = 1) and, bit for bit, against the asynchronous
    handle; after sync_end the synchronous handle's own columns, rng / episode and statistics likewise."""
    N = acts.shape[2]
    s_env, a_env = make(tab, N, with_qrm=qrm), make(tab, N, with_qrm=qrm)
    try:
        resets = dict(reseed or {})
        resets[-1] = seed
        for s in range(-1, acts.shape[0]):
            if s in resets:
                a_env.reset(seed=resets[s])
                out = s_env.reset_sync(seed=resets[s])
                if "resets" in ref:
                    assert_vs_oracle(tab, out, ref["resets"][s], f"reset before step {s + 1}",
                                     RESET_COLS + ("enc_state",))
                assert_bit_equal(out, columns(a_env), f"reset before step {s + 1}", RESET_COLS)
                for k in ("reward", "renv", "env_done"):  # a reset returns no step outputs
                    assert not out[k].any(), k
            if s < 0:
                continue
            a_env.step(to_async(acts[s]), autoreset=True)
            out = s_env.step_sync(acts[s], autoreset=True)
            assert_vs_oracle(tab, out, ref["snaps"][s], f"step {s}", qrm=qrm)
            assert_bit_equal(out, columns(a_env), f"step {s} (sync / async)")
            if between is not None:
                between(s)
        s_env.sync_end()
        last, mine, other = ref["snaps"][acts.shape[0] - 1], columns(s_env), columns(a_env)
        assert set(mine) == set(other) and set(INT_COLS + QRM_COLS[:4 * qrm]) <= set(mine)
        assert_bit_equal(mine, other, "after sync_end")
        assert_vs_oracle(tab, mine, last, "after sync_end", qrm=qrm)
        if tab.stochastic or tab.random_starts:
            np.testing.assert_array_equal(mine["rng"], last["rng"], err_msg="rng after sync_end")
            if "episode" in last:
                np.testing.assert_array_equal(mine["episode"], last["episode"], err_msg="episode after sync_end")
        assert_same_stats(s_env, a_env, ref["stats"])
    finally:
        s_env.close()
        a_env.close()


# ---- the worlds of section B ----------------------------------------------------------------------------------------
# (case, N): every limit world at a partial second wave, three at the dict API's single env, two at the whole block
# (a7_ow ends one episode in ~30,000 by truncation: none at 65 envs x 150 steps, nor at 256; 68 is the first N above 65
# whose action draw holds one for every agent, so that world runs there)
WORLD_N = {"a7_ow": 68}
WORLD_RUNS = [(c, WORLD_N.get(c, N_SYNC)) for c in L.CASES] + [("a8_ow_shaping", 1), ("q250_a2_generic", 1),
                                                                ("cells4096_row", 1), ("a8_fl", 256), ("w256_h2", 256)]
RNG_RUNS = ["a8_fl_slip", "a8_fl_randstart", "q250_a2_slip", "h255_randstart_slip_cache"]
RESEED = {70: 4242}  # a reset with a new base seed before step 70


@functools.lru_cache(maxsize=None)
def world_reference(case, n):
    """The oracle on a limit world at n envs: L.oracle_run with every step kept.  The world's liveness conditions hold
    on this trajectory (L.check_liveness: the target field >= 128, or the cell >= 2,048, in at least 10 % of the
    samples and its top value reached; with more than four agents every agent index moves, is paid by its RM and ends
    episodes both ways, and somewhere only the last agent is still active) before an engine is touched.  A single env
    (the dict API's shape) is no sample of the world: there the share alone is asserted, where the world has one."""
    tab = L.limit_world(case)[1]
    acts = L.case_actions(case, n=n, steps=K_SYNC)
    ref = L.oracle_run(tab, acts, snap_every=1)
    if n >= N_SYNC:
        ref["liveness"] = L.check_liveness(case, tab, ref["traj"])
    else:
        ref["liveness"] = lv = L.liveness(case, tab, ref["traj"])
        assert all(v >= 0.10 for k, v in lv.items() if k.startswith("frac_") and k != "frac_only_last_active"), lv
    return tab, acts, ref


@functools.lru_cache(maxsize=None)
def rng_world_reference(case, n=N_SYNC):
    """A slip / random-start limit world at n envs: liveness on L.rng_reference's trajectory (the limit is still
    reached, the envs' generators have diverged), then the oracle with a reseed in mid-run and the episode column."""
    tab, acts, plain = L.rng_reference(case, n=n)
    L.check_rng_liveness(case, tab, plain)
    ref = oracle_record(tab, acts, seed=31, reseed=RESEED)
    assert ref["snaps"][acts.shape[0] - 1]["episode"].max() >= 1  # autoresets after the reseed: the schedule's 2nd term
    return tab, acts, ref


@functools.lru_cache(maxsize=None)
def blob_limit_reference(n=N_SYNC):
    """SIZE_EDGES["generic_blob_under"]: 65,344 B of tables, the most LDS a handle can ask for."""
    tab = L.size_world(**L.SIZE_EDGES["generic_blob_under"][0])
    assert L.generic_blob_bytes(tab) == 65344
    acts = np.random.default_rng(3).integers(0, 5, size=(K_SYNC, tab.n_agents, n), dtype=np.int32)
    ref = oracle_record(tab, acts)
    ref["traj"] = {"rm_q": np.stack([ref["snaps"][s]["rm_q"] for s in range(K_SYNC)])}
    L.check_size_liveness(tab, ref)
    return tab, acts, ref


# ---- C. QRM worlds --------------------------------------------------------------------------------------------------
QRM_RUNS = [("q250_a1_fast", 3, 150), ("q250_a1_fast", 256, 40), ("q250_a2_generic", N_SYNC, 60)]


@functools.lru_cache(maxsize=None)
def qrm_reference(case, n, steps):
    tab = L.limit_world(case)[1]
    assert int(tab.n_qrm.max()) == 249 == L.n_qrm_max(tab)  # every non-final state but the current one
    acts = L.case_actions(case, n=n, steps=steps)
    ref = oracle_record(tab, acts, qrm=True)
    q = np.stack([ref["snaps"][s]["rm_q"] for s in range(steps)])
    sn = np.stack([ref["snaps"][s]["qrm_sn"] for s in range(steps)])
    assert (q >= 128).mean() >= 0.10, (q >= 128).mean()
    enc = np.asarray(tab.enc_nq).reshape(1, -1, 1, 1)
    assert ((sn % enc) >= 128).mean() >= 0.10  # counterfactual successors in the upper half of the machine
    return tab, acts, ref


def golden_qrm(name, configs, golden_dir, steps=K_SYNC):
    """The first `steps` steps of a QRM golden: its tables, actions, seed and the reference's recorded tuples."""
    g = dict(np.load(os.path.join(golden_dir, f"traj_{name}.npz")))
    full = g["actions"].shape[0]
    g = {k: (v[:steps] if v.ndim and v.shape[0] == full else v) for k, v in g.items()}
    assert name in LIMIT_TRAJ and "qrm_s" in g
    return T.compile_scenario(configs[name]), g["actions"].astype(np.int32), int(g["seed"]), g


def run_golden_qrm(make, tab, acts, seed, g):
    """step_sync's QRM columns over a golden's actions against the reference's infos["qrm_experience"] tuples."""
    env = make(tab, acts.shape[2], with_qrm=True)
    try:
        env.reset_sync(seed=seed)
        keys = ("rm_q", "renv") + QRM_COLS
        rec = {k: [] for k in keys}
        for s in range(acts.shape[0]):
            out = env.step_sync(acts[s], autoreset=True)
            for k in keys:
                rec[k].append(out[k].copy())
        r = {k: np.stack(v) for k, v in rec.items()}
        np.testing.assert_array_equal(r["rm_q"], g["q"])
        check_qrm(tab, {**r, "q": r["rm_q"]}, g, acts, r["renv"])
    finally:
        env.close()


def qrm_request(env):
    """rmx_buffers asking a handle for the four QRM columns (and nothing else), with the arrays behind it."""
    shape = (env.A, max(int(env.cfg.n_qrm_max), 1), env.N)
    arrs = [np.zeros(shape, dt) for dt in (np.int32, np.int32, np.float32, np.uint8)]
    b = _capi.RmxBuffers()
    for k, v in zip(QRM_COLS, arrs):
        setattr(b, k, v.ctypes.data)
    return b, arrs


def run_qrm_refused(make, tab, stream=lambda env: None):
    """A handle without QRM columns asked for them through the C ABI: RMX_E_STATE, after the step itself (the
    request is served before its outputs are unpacked), and the handle goes on."""
    N = 3
    acts = L.case_actions("q250_a1_fast", n=N, steps=3)
    ref = oracle_record(tab, acts)
    env = make(tab, N)
    try:
        env.reset_sync(seed=123)
        b, _ = qrm_request(env)
        a0 = np.ascontiguousarray(acts[0])
        rc = env.lib.rmx_step_sync(env._h, a0.ctypes.data, 1, C.byref(b), stream(env))
        assert rc == _capi.RMX_E_STATE and b"QRM" in env.lib.rmx_last_error()
        assert_vs_oracle(tab, env.step_sync(acts[1], autoreset=True), ref["snaps"][1], "the step after the refusal")
        env.check_errors()
    finally:
        env.close()


# ---- D. the two halves ----------------------------------------------------------------------------------------------
def run_two_halves(make, tab, acts, stream=lambda env: None, async_step=None):
    """rmx_step_sync_begin, host work, rmx_sync_wait = rmx_step_sync; the error contract of csrc/rmx_capi_sync.cpp:
    rmx_sync_wait with nothing outstanding and a second begin are RMX_E_STATE, the pending request stays served
    exactly once; rmx_sync_end serves a begun request and drops its outputs.  async_step(env, actions) (device
    handles): an asynchronous entry point while a request is pending ends the resident workgroup first, which serves
    the request (sync_end: "a begun request is served first"), so both steps count and rmx_sync_wait then finds
    nothing outstanding."""
    N = acts.shape[2]
    ref = oracle_record(tab, acts)
    env, twin = make(tab, N), make(tab, N)
    lib, E_STATE = env.lib, _capi.RMX_E_STATE
    try:
        out, b = env._sync_out()
        twin.reset_sync(seed=123)
        env.reset_sync(seed=123)
        assert lib.rmx_sync_wait(env._h, C.byref(b)) == E_STATE
        assert b"no synchronous request is outstanding" in lib.rmx_last_error()
        work = 0
        for s in range(acts.shape[0] - 4):
            a = np.ascontiguousarray(acts[s])
            assert lib.rmx_step_sync_begin(env._h, a.ctypes.data, 1, stream(env)) == 0, lib.rmx_last_error()
            if s % 10 == 3:  # a second begin is refused and disturbs nothing
                assert lib.rmx_step_sync_begin(env._h, a.ctypes.data, 1, stream(env)) == E_STATE
                assert b"a synchronous request is outstanding" in lib.rmx_last_error()
            work += int(np.sum(ref["snaps"][s]["pos_x"]))  # the caller's own work between the halves
            assert lib.rmx_sync_wait(env._h, C.byref(b)) == 0, lib.rmx_last_error()
            assert_bit_equal(out, twin.step_sync(acts[s], autoreset=True), f"two halves, step {s}")
            assert_vs_oracle(tab, out, ref["snaps"][s], f"two halves, step {s}")
            if s % 10 == 5:
                assert lib.rmx_sync_wait(env._h, C.byref(b)) == E_STATE
        s = acts.shape[0] - 4
        a = np.ascontiguousarray(acts[s])
        # rmx_sync_end with a request pending: the step counts, its outputs are dropped, nothing is outstanding
        assert lib.rmx_step_sync_begin(env._h, a.ctypes.data, 1, stream(env)) == 0
        assert lib.rmx_sync_end(env._h) == 0
        assert lib.rmx_sync_wait(env._h, C.byref(b)) == E_STATE
        assert_vs_oracle(tab, columns(env), ref["snaps"][s], "after rmx_sync_end on a pending request",
                         ("pos_x", "pos_y", "rm_q", "flags", "t", "ep_ret"))
        s += 1
        if async_step is not None:
            a = np.ascontiguousarray(acts[s])
            assert lib.rmx_step_sync_begin(env._h, a.ctypes.data, 1, stream(env)) == 0
            async_step(env, acts[s + 1])
            assert lib.rmx_sync_wait(env._h, C.byref(b)) == E_STATE
            assert b"no synchronous request is outstanding" in lib.rmx_last_error()
            s += 2
        else:
            env.step_sync(acts[s], autoreset=True)
            s += 1
        while s < acts.shape[0]:  # the handle keeps working
            assert_vs_oracle(tab, env.step_sync(acts[s], autoreset=True), ref["snaps"][s], f"afterwards, step {s}")
            s += 1
        env.sync_end()
        env.check_errors()
        assert work > 0
    finally:
        env.close()
        twin.close()


# ---- invalid actions ------------------------------------------------------------------------------------------------
def run_invalid_actions(make, tab, N, to_async=lambda a: a):
    """Every slot k of the request x every invalid value: step_sync raises ValueError and sets the error word once;
    the slot was stepped as wait (never as the value's low nibble), exactly as the asynchronous path and the oracle
    step the same array; the next valid step succeeds."""
    A = tab.n_agents
    hi = n_action_values(tab)
    rng = np.random.default_rng(17)
    s_env, a_env, orc = make(tab, N), make(tab, N), O.OracleEnv(tab, N)
    try:
        a_env.reset(seed=5)
        s_env.reset_sync(seed=5)
        orc.reset(seed=5)
        moved_on_nibble = 0
        for k in range(A * N):
            for v in INVALID_ACTIONS:
                acts = rng.integers(0, hi, size=(A, N), dtype=np.int32)
                probe = O.OracleEnv(tab, N)  # what the step would be had the low nibble been taken for the action
                for name in RESET_COLS:
                    getattr(probe, name)[...] = getattr(orc, name)
                low = acts.copy()
                low.reshape(-1)[k] = (v & 15) if (v & 15) < hi else 0
                acts.reshape(-1)[k] = v
                assert orc.step(acts) == _capi.RMX_E_ACTION
                probe.step(low)
                moved_on_nibble += int((probe.pos_x != orc.pos_x).any() or (probe.pos_y != orc.pos_y).any())
                with pytest.raises(ValueError, match="outside"):
                    s_env.step_sync(acts, autoreset=True)
                out = {name: val.copy() for name, val in s_env._sync_out()[0].items()}
                with pytest.raises(ValueError):
                    s_env.check_errors()
                s_env.check_errors()  # once
                a_env.step(to_async(acts), autoreset=True)
                with pytest.raises(ValueError):
                    a_env.check_errors()
                assert_bit_equal(out, columns(a_env), f"slot {k} action {v}")
                assert_vs_oracle(tab, out, oracle_snapshot(orc), f"slot {k} action {v}")
                good = rng.integers(0, hi, size=(A, N), dtype=np.int32)
                orc.step(good)
                a_env.step(to_async(good), autoreset=True)
                assert_vs_oracle(tab, s_env.step_sync(good, autoreset=True), oracle_snapshot(orc), f"after slot {k}")
                s_env.check_errors()
        # the comparison could tell: stepping the low nibble would have moved some agent elsewhere
        assert moved_on_nibble >= A * N
    finally:
        s_env.close()
        a_env.close()


# ---- E. get_mdp -----------------------------------------------------------------------------------------------------
MDP_CASES = [c for c in L.CASES]  # every limit world is deterministic (slip / random starts: RNG_CASES)


def mdp_liveness(case, tab, a, nxt, done):
    """The arrays hold what the world is there for: a successor whose RM index is >= 128 (250-state machines), whose
    cell is >= 2,048 (4,096-cell grids)."""
    nq = int(tab.enc_nq[a])
    has = nxt >= 0
    if case.startswith("q250"):
        assert ((nxt[has] % nq) >= 128).any() and int((nxt[has] % nq).max()) == 249
    if case.startswith("cells4096"):
        assert ((nxt[has] // nq) >= 2048).any() and int((nxt[has] // nq).max()) == 4095


def oracle_mdp_as_golden(tab, a, fix):
    """The oracle's get_mdp (O.mdp, the call test_oracle_mdp_matches_reference pins to the reference) in the layout
    check_mdp compares against."""
    nxt, rew, done = O.mdp(tab, a, fix_fl=fix)
    return {f"a{a}_next": nxt, f"a{a}_reward": rew.astype(np.float64), f"a{a}_done": done.astype(np.int8)}, nxt, done


def mdp_states(env, a):
    S = C.c_int64()
    _capi.check(env.lib.rmx_mdp_states(env._h, a, C.byref(S)), "rmx_mdp_states")
    return S.value


# ======================================================================================================================
# The host-handle tests
# ======================================================================================================================
@pytest.mark.parametrize("A,N", REQUEST_SHAPES)
def test_request_shapes_on_a_host_handle(A, N, configs):
    """The shapes of section A through a host handle's synchronous calls: 60 steps with autoreset, every action value
    in every slot, every column after every step against the oracle and an asynchronous host handle."""
    tab = shape_tables(A, configs, N)
    acts = request_actions(tab, N)
    run_sync(host_engine, tab, acts, oracle_record(tab, acts))


@pytest.mark.parametrize("A,N", INVALID_SHAPES)
def test_invalid_actions_on_a_host_handle(A, N, configs):
    run_invalid_actions(host_engine, shape_tables(A, configs), N)


@pytest.mark.parametrize("case,N", WORLD_RUNS)
def test_limit_worlds_through_host_step_sync(case, N):
    """Every limit world through HostRMEnv.step_sync against the oracle's run, whose liveness is asserted first."""
    tab, acts, ref = world_reference(case, N)
    run_sync(host_engine, tab, acts, ref)


@pytest.mark.parametrize("case", RNG_RUNS)
def test_rng_worlds_through_host_step_sync(case):
    """Slip and random starts at 8 agents, 250 RM states and 255 rows, with a reset_sync to a new seed in mid-run: the
    rng and episode columns after the run are the oracle's."""
    tab, acts, ref = rng_world_reference(case)
    run_sync(host_engine, tab, acts, ref, seed=31, reseed=RESEED)


def test_blob_limit_world_through_host_step_sync():
    tab, acts, ref = blob_limit_reference()
    run_sync(host_engine, tab, acts, ref)


@pytest.mark.parametrize("case,N,steps", QRM_RUNS)
def test_qrm_columns_through_host_step_sync(case, N, steps):
    """249 counterfactuals per agent and step through host_sync_out: all four arrays equal the asynchronous host
    handle's bit for bit and the oracle's."""
    tab, acts, ref = qrm_reference(case, N, steps)
    run_sync(host_engine, tab, acts, ref, qrm=True)


@pytest.mark.parametrize("name", ["fl1_qrm16", "fl1_qrm17"])
def test_qrm_goldens_through_host_step_sync(name, configs, golden_dir):
    run_golden_qrm(host_engine, *golden_qrm(name, configs, golden_dir))


def test_qrm_columns_refused_without_qrm_on_a_host_handle():
    run_qrm_refused(host_engine, L.limit_world("q250_a1_fast")[1])


@pytest.mark.parametrize("case,N", [("a8_fl", 1), ("q250_a2_generic", N_SYNC)])
def test_two_halves_on_a_host_handle(case, N):
    tab = L.limit_world(case)[1]
    run_two_halves(host_engine, tab, L.case_actions(case, n=N, steps=40))


@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("case", MDP_CASES)
def test_host_mdp_equals_oracle_on_limit_worlds(case, fix):
    """get_mdp of every agent of every limit world from a host handle against the oracle's: next / done identical,
    rewards within 1e-6, rmx_mdp_states = W * H * enc_nq[a]."""
    tab = L.limit_world(case)[1]
    assert not (tab.stochastic or tab.random_starts)
    env = HostRMEnv(tab, 1)
    try:
        for a in range(tab.n_agents):
            g, nxt, done = oracle_mdp_as_golden(tab, a, fix)
            assert mdp_states(env, a) == tab.width * tab.height * int(tab.enc_nq[a]) == nxt.shape[0]
            if fix or tab.kind == T.OFFICE_WORLD:  # (FrozenLake without the fix: the reference's decode has no entries)
                mdp_liveness(case, tab, a, nxt, done)
            check_mdp(tab, a, *env.mdp_arrays(a, fix), g)
    finally:
        env.close()
