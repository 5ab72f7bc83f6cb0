"""The reference's own action stream inside the learn step (include/rmx.h RMX_LEARN_NUMPY,
rmx.learn.VecQLearning(policy_seeds=...).act_step(reference_stream=True)) on host handles: whole training runs recorded
from the reference's QLearning choosing its own actions, the plain-Python restatement (tests/policyref.py) against the
installed numpy and against the engine, sharding, mixed use and every refusal."""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import learn_common as LC
import policy_common as PC
import policyref as PR
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv
from rmx.learn import VecQLearning
from test_learn_cpu import _lcfg, _raw
from test_random_maps_gpu import CASES, random_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_recorded_fixture_is_present():
    assert PC.FIXTURES == PC.EXPECTED


@pytest.mark.parametrize("case", PC.EXPECTED)
def test_whole_runs_of_the_reference_choosing_its_own_actions(case):
    PC.replay_fixture(case, HostRMEnv)


# ---- the restatement against numpy's own Generator ------------------------------------------------------------------
def _numpy_choose(g, eps, row):
    """qlearning.py:120-143 on a real Generator."""
    if g.uniform(0, 1) < eps:
        return int(g.choice(range(4)))
    m = max(row)
    return int(g.choice([i for i, v in enumerate(row) if v == m]))


ROWS = ([1.0, 1.0, 1.0, 1.0], [0.5, 2.0, 2.0, 2.0], [3.0, 0.0, 3.0, 3.0], [1.0, 1.0, 0.0, -1.0], [0.0, 0.0, 0.0, 0.5],
        [-1.0, -2.0, -1.0, -3.0], [2.0, 1.0, 2.0, 2.0])


def test_restatement_equals_numpy_on_mixed_sequences():
    pick = np.random.default_rng(3)
    n = 0
    for seed in list(range(40)) + [2020, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5, 2 ** 64 - 1]:
        g, r = np.random.default_rng(seed), PR.Pcg(seed)
        for _ in range(150):
            row, eps = ROWS[pick.integers(len(ROWS))], (0.0, 0.3, 1.0)[pick.integers(3)]
            assert PR.choose(r, eps, row) == _numpy_choose(g, eps, row), seed
            n += 1
        assert r.state() == g.bit_generator.state, seed
    assert n == 45 * 150
    # the redraw of Lemire's method, forced: a buffered half of 0 and three maxima (left = 0 < thr = 1)
    for seed in range(30):
        g = np.random.default_rng(seed)
        st = g.bit_generator.state
        st["has_uint32"], st["uinteger"] = 1, 0
        g.bit_generator.state = st
        r = PR.Pcg(st)
        for _ in range(3):
            assert PR.choose(r, 0.0, ROWS[1]) == _numpy_choose(g, 0.0, ROWS[1]), seed
        assert r.state() == g.bit_generator.state, seed


# ---- the engine against the restatement -----------------------------------------------------------------------------
def _fresh(N=5, seeds=None, **kw):
    tab = T.compile_scenario(T.baseline_scenario(2))
    env = HostRMEnv(tab, N)
    env.reset(seed=1)
    A = tab.n_agents
    if seeds is None:
        seeds = np.arange(A * N, dtype=np.uint64).reshape(A, N) * 977 + 3
    return tab, env, VecQLearning(env, 0.9, 0.2, use_qrm=True, policy_seeds=seeds, **kw)


def _set_rows(L, rows):
    """rows[a][e] -> the row of the state (a, e) is about to leave."""
    st = PC.states_to_leave(L.env, L.env.tables)
    for a in range(L.env.A):
        for e in range(L.env.N):
            L.q[a, e, st[a, e]] = rows[a][e]


def test_seeding_is_numpys_default_rng():
    seeds = np.array([[0, 1, 2020, 2 ** 32 - 1, 2 ** 32], [2 ** 32 + 7, 2 ** 63, 2 ** 64 - 1, 12345678901234, 7]], np.uint64)
    _, env, L = _fresh(seeds=seeds)
    for a in range(2):
        for e in range(5):
            assert L.rng_state(a, e) == np.random.default_rng(int(seeds[a, e])).bit_generator.state
    _, env1, L1 = _fresh(seeds=2020)  # an int: every learner, as the FrozenLake runner
    assert all(L1.rng_state(a, e) == np.random.default_rng(2020).bit_generator.state for a in range(2) for e in range(5))
    # a run handed to a real Generator and back
    g = np.random.default_rng(5)
    g.random(3), g.integers(0, 3)
    L.set_rng_state(1, 2, g.bit_generator.state)
    assert L.rng_state(1, 2) == g.bit_generator.state and g.bit_generator.state["has_uint32"] == 1
    with pytest.raises(ValueError):
        L.set_rng_state(0, 0, np.random.Generator(np.random.MT19937(1)).bit_generator.state)


def test_forced_redraw_and_the_buffer_word():
    tab, env, L = _fresh()
    out = np.zeros((2, 5), np.int32)
    for a in range(2):
        for e in range(5):
            st = L.rng_state(a, e)
            st["has_uint32"], st["uinteger"] = 1, 0
            L.set_rng_state(a, e, st)
    _set_rows(L, [[ROWS[1]] * 5, [ROWS[2]] * 5])  # three maxima everywhere
    # numpy itself on the same states
    want_np = np.zeros((2, 5), np.int32)
    for a in range(2):
        for e in range(5):
            g = np.random.default_rng(0)
            g.bit_generator.state = L.rng_state(a, e)
            want_np[a, e] = _numpy_choose(g, 0.0, ROWS[1 + a])
    want, after = PC.expect_step(L, 0.0)
    assert np.array_equal(want, want_np)
    L.act_step(0.0, reference_stream=True, learn=False, actions_out=out)
    assert np.array_equal(out, want) and np.array_equal(L.rng, after)
    assert (L.rng[4] >> np.uint64(32) == 1).all()  # the redraw drew 64 bits and buffered the high half again


def test_one_maximum_draws_no_choice_and_leaves_the_buffer_word():
    tab, env, L = _fresh()
    out = np.zeros((2, 5), np.int32)
    L.rng[4] = (np.uint64(1) << np.uint64(32)) | np.uint64(0xDEADBEEF)
    before = L.rng.copy()
    _set_rows(L, [[ROWS[4]] * 5, [ROWS[4]] * 5])  # one maximum: action 3
    want, after = PC.expect_step(L, 0.0)
    L.act_step(0.0, reference_stream=True, learn=False, actions_out=out)
    assert (out == 3).all() and np.array_equal(out, want) and np.array_equal(L.rng, after)
    assert np.array_equal(L.rng[4], before[4]) and np.array_equal(L.rng[2:4], before[2:4])
    assert (L.rng[:2] != before[:2]).any(axis=0).all()  # the explore draw was taken all the same
    # an explore step uses the buffered half and clears the flag
    want, after = PC.expect_step(L, 1.0)
    L.act_step(1.0, reference_stream=True, learn=False, actions_out=out)
    assert np.array_equal(out, want) and np.array_equal(L.rng, after)
    assert (out == (0xDEADBEEF * 4) >> 32).all() and (L.rng[4] == 0xDEADBEEF).all()


def test_best_leaves_the_column_and_an_evaluation_step_advances_it():
    tab, env, L = _fresh()
    out = np.zeros((2, 5), np.int32)
    _set_rows(L, [[ROWS[k % len(ROWS)] for k in range(5)], [ROWS[(k + 3) % len(ROWS)] for k in range(5)]])
    before, q0, v0 = L.rng.copy(), L.q.copy(), L.visits.copy()
    want, _ = PC.expect_step(L, 0.7, best=True)
    L.act_step(0.7, reference_stream=True, best=True, learn=False, actions_out=out)
    assert np.array_equal(out, want) and np.array_equal(L.rng, before)
    want, after = PC.expect_step(L, 0.7)
    L.act_step(0.7, reference_stream=True, learn=False, actions_out=out)
    assert np.array_equal(out, want) and np.array_equal(L.rng, after)
    assert (L.rng[:2] != before[:2]).any(axis=0).all()
    assert np.array_equal(LC.bits(L.q), LC.bits(q0)) and np.array_equal(L.visits, v0)  # learn=False: tables only read


def test_nan_rows():
    nan = float("nan")
    rows = [[nan, 1.0, 2.0, 0.0], [nan, nan, nan, nan], [1.0, nan, 1.0, 0.0], [0.0, nan, nan, 5.0], [2.0, 2.0, nan, 2.0]]
    tab, env, L = _fresh()
    out = np.zeros((2, 5), np.int32)
    _set_rows(L, [rows, rows[::-1]])
    before = L.rng.copy()
    want, after = PC.expect_step(L, 0.0)
    L.act_step(0.0, reference_stream=True, learn=False, actions_out=out)
    assert np.array_equal(out, want) and np.array_equal(L.rng, after)
    assert out[0].tolist()[:2] == [3, 3]  # a NaN maximum: action 3 ...
    assert np.array_equal(L.rng[4, 0, :2], before[4, 0, :2])  # ... and no choice draw
    assert out[0, 3] == 3 and out[0, 4] in (0, 1, 3)  # a NaN further on is skipped
    _set_rows(L, [rows, rows[::-1]])
    want, _ = PC.expect_step(L, 0.0, best=True)
    L.act_step(0.0, reference_stream=True, best=True, learn=False, actions_out=out)
    assert np.array_equal(out, want)


@pytest.mark.parametrize("name", ["fl_small_merged", "ow_regs_eligible"])
def test_training_runs_equal_the_restatement(name):
    tab = dataclasses.replace(random_tables(*CASES[name]), max_t=25)
    N, K, A = 4, 80, tab.n_agents
    env = HostRMEnv(tab, N)
    env.reset(seed=2)
    L = VecQLearning(env, 0.9, 0.3, qtable_init=0.5, use_qrm=True, policy_seeds=np.arange(A * N).reshape(A, N) + 100)
    out = np.zeros((A, N), np.int32)
    seen = set()
    for t in range(K):
        want, after = PC.expect_step(L, 0.25)
        L.act_step(0.25, reference_stream=True, actions_out=out)
        assert np.array_equal(out, want), t
        assert np.array_equal(L.rng, after), t
        seen |= set(out.ravel().tolist())
    assert seen == {0, 1, 2, 3} and (L.visits > 0).any() and (env.t < K).all()
    env.check_errors()


# ---- sharding, mixed use --------------------------------------------------------------------------------------------
def test_two_shards_equal_the_whole():
    tab = dataclasses.replace(random_tables(*CASES["ow_regs_eligible"]), max_t=25)
    A, N, K = tab.n_agents, 6, 70
    seeds = np.random.default_rng(8).integers(0, 2 ** 40, size=(A, N), dtype=np.uint64)
    kw = dict(qtable_init=0.5, use_qrm=True)
    whole = HostRMEnv(tab, N)
    halves = [HostRMEnv(tab, 3, env_offset=o, n_envs_global=N) for o in (0, 3)]
    Lw = VecQLearning(whole, 0.9, 0.3, policy_seeds=seeds, **kw)
    Lh = [VecQLearning(h, 0.9, 0.3, policy_seeds=seeds[:, o:o + 3], **kw) for h, o in zip(halves, (0, 3))]
    ow, oh = np.zeros((A, N), np.int32), [np.zeros((A, 3), np.int32) for _ in range(2)]
    for t in range(K):
        Lw.act_step(0.2, reference_stream=True, actions_out=ow)
        for L, o in zip(Lh, oh):
            L.act_step(0.2, reference_stream=True, actions_out=o)
        assert np.array_equal(ow, np.concatenate(oh, axis=1)), t
    assert np.array_equal(LC.bits(Lw.q), LC.bits(np.concatenate([L.q for L in Lh], axis=1)))
    assert np.array_equal(Lw.visits, np.concatenate([L.visits for L in Lh], axis=1))
    assert np.array_equal(Lw.rng, np.concatenate([L.rng for L in Lh], axis=2))
    assert (Lw.visits > 0).any()


def test_mixed_use_and_a_restored_column():
    tab = dataclasses.replace(random_tables(*CASES["fl_small_merged"]), max_t=25)
    A, N = tab.n_agents, 5
    env = HostRMEnv(tab, N)
    env.reset(seed=4)
    L = VecQLearning(env, 0.9, None, qtable_init=0.5, policy_seeds=77)
    out = np.zeros((A, N), np.int32)
    hashed = env.fill_actions(6, 0, 40)

    def segment(t0):
        """reference-stream steps alternating with engine-policy and caller-action steps; only the first move the column"""
        trace = []
        for t in range(t0, t0 + 12):
            col = L.rng.copy()
            if t % 3 == 0:
                want, after = PC.expect_step(L, 0.3)
                L.act_step(0.3, reference_stream=True, actions_out=out)
                assert np.array_equal(out, want) and np.array_equal(L.rng, after) and not np.array_equal(L.rng, col)
            elif t % 3 == 1:
                L.act_step(0.3, 9, t, actions_out=out)
                assert np.array_equal(L.rng, col)
            else:
                L.step(hashed[t])
                assert np.array_equal(L.rng, col)
            trace.append(out.copy())
        return trace

    segment(0)
    saved = env.save_state(), L.q.copy(), L.visits.copy(), L.rng.copy()
    first = segment(12)
    end = L.q.copy(), L.visits.copy(), L.rng.copy()
    env.load_state(saved[0])
    L.q[...], L.visits[...], L.rng[...] = saved[1], saved[2], saved[3]
    again = segment(12)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    assert np.array_equal(LC.bits(L.q), LC.bits(end[0])) and np.array_equal(L.visits, end[1])
    assert np.array_equal(L.rng, end[2]) and (L.visits > 0).any()


# ---- refusals -------------------------------------------------------------------------------------------------------
def test_refusals():
    tab = T.compile_scenario(T.baseline_scenario(2))
    lib, h, keep = _raw(tab)
    assert lib.rmx_abi_version() == 12
    INV, STATE = _capi.RMX_E_INVALID, _capi.RMX_E_STATE
    s_max = C.c_int64()
    assert lib.rmx_learn_states(h, C.byref(s_max)) == 0
    q = np.ones((2, 4, s_max.value, 4))
    col = np.zeros(5 * 2 * 4 + 2, np.uint64)
    base = col.ctypes.data + (-col.ctypes.data % 16)  # a 16-byte aligned address inside col
    seeds = np.arange(8, dtype=np.uint64)
    out = np.zeros((2, 4), np.int32)
    # before rmx_learn_bind
    assert lib.rmx_learn_rng_bind(h, base) == STATE and b"rmx_learn_bind" in lib.rmx_last_error()
    assert lib.rmx_learn_rng_seed(h, seeds.ctypes.data, None) == STATE and b"rmx_learn_bind" in lib.rmx_last_error()
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(use_qrm=1)), q.ctypes.data, None) == 0
    # no column bound
    assert lib.rmx_learn_step_policy(h, 0.1, 1 | 4, 0, 0, 1, None, None) == STATE
    assert b"rmx_learn_rng_bind" in lib.rmx_last_error()
    assert lib.rmx_learn_step_policy(h, 0.1, 1 | 2 | 4, 0, 0, 1, None, None) == STATE
    assert lib.rmx_learn_rng_seed(h, seeds.ctypes.data, None) == STATE and b"rmx_learn_rng_bind" in lib.rmx_last_error()
    assert np.array_equal(q, np.ones_like(q))  # (nothing was stepped)
    # a misaligned column, NULL seeds, NULL handles
    assert lib.rmx_learn_rng_bind(h, base + 8) == INV and b"aligned" in lib.rmx_last_error()
    assert lib.rmx_learn_rng_bind(h, base) == 0
    assert lib.rmx_learn_rng_seed(h, None, None) == INV and b"seeds" in lib.rmx_last_error()
    assert lib.rmx_learn_rng_bind(None, base) == INV and b"NULL" in lib.rmx_last_error()
    assert lib.rmx_learn_rng_seed(None, seeds.ctypes.data, None) == INV and b"NULL" in lib.rmx_last_error()
    # unknown flags are still refused, with and without the new one
    for flags in (8, 4 | 8, 1 | 8, 16):
        assert lib.rmx_learn_step_policy(h, 0.5, flags, 0, 0, 1, None, None) == INV and b"flags" in lib.rmx_last_error()
    assert lib.rmx_learn_step_policy(h, 1.5, 1 | 4, 0, 0, 1, None, None) == INV and b"epsilon" in lib.rmx_last_error()
    # a good seed and step (actions_out NULL, then given); the words before and after the column are the caller's
    assert lib.rmx_learn_rng_seed(h, seeds.ctypes.data, None) == 0
    k = (base - col.ctypes.data) // 8
    assert (col[:k] == 0).all() and (col[k + 40:] == 0).all() and (col[k:k + 32] != 0).all() and (col[k + 32:k + 40] == 0).all()
    assert lib.rmx_learn_step_policy(h, 0.1, 1 | 4, 0, 0, 1, None, None) == 0
    assert lib.rmx_learn_step_policy(h, 0.1, 1 | 4, 0, 0, 1, out.ctypes.data, None) == 0
    assert (col[:k] == 0).all() and (col[k + 40:] == 0).all()
    # NULL unbinds
    assert lib.rmx_learn_rng_bind(h, None) == 0
    assert lib.rmx_learn_step_policy(h, 0.1, 1 | 4, 0, 0, 1, None, None) == STATE
    assert lib.rmx_learn_step_policy(h, 0.1, 1, 0, 0, 1, None, None) == 0  # the engine's policy needs no column
    lib.rmx_destroy(h)


def test_python_class_argument_checks():
    tab = T.compile_scenario(T.baseline_scenario(2))
    env = HostRMEnv(tab, 3)
    with pytest.raises(ValueError, match="policy_seeds"):
        VecQLearning(env, 0.9, 0.1, policy_seeds=np.zeros((2, 4), np.uint64))
    with pytest.raises(ValueError, match="policy_seeds"):
        VecQLearning(env, 0.9, 0.1, policy_seeds=-1)
    L = VecQLearning(env, 0.9, 0.1)
    assert L.rng is None
    with pytest.raises(RuntimeError, match="policy_seeds"):
        L.act_step(0.1, reference_stream=True)
    with pytest.raises(ValueError, match="seed and t_global"):
        L.act_step(0.1)
    L.act_step(0.1, 3, 0)  # (positional seed / t_global as before)


# ---- the policy's arithmetic as a stand-alone program under AddressSanitizer + UBSan ------------------------------
def _digest():
    """policy_host_main.cpp's sequence on tests/policyref.py."""
    m = 2 ** 64 - 1
    rows = [[1, 1, 1, 1], [0.5, 2, 2, 2], [3, 0, 3, 3], [1, 1, 0, -1], [0, 0, 0, 0.5], [float("nan"), 1, 2, 0]]
    d = 0xcbf29ce484222325
    for s in range(200):
        g = PR.Pcg({"state": {"state": (((s * 0x9E3779B97F4A7C15) & m) << 64) | (~s & m), "inc": (s << 64) | (s << 1) | 1},
                    "has_uint32": s & 1, "uinteger": 0})
        for i in range(500):
            a = PR.choose(g, (i % 3) * 0.5, [float(v) for v in rows[(s + i) % 6]])
            d = ((d ^ a) * 0x100000001b3) & m
        w = g.words()
        d = ((d ^ w[0] ^ w[1] ^ w[4]) * 0x100000001b3) & m
    return d


def test_policy_arithmetic_clean_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler for the sanitizer build")
    exe = str(tmp_path / "policy_host_main")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "multiagent-rl-rm_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "data", "policy_host_main.cpp")], check=True)
    # the sanitizer runtimes are linked statically: the program does not depend on what the environment preloads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    got = next(ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("POLICY_HOST_DIGEST"))
    assert int(got, 16) == _digest()
