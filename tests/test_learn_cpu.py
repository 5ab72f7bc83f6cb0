"""The tabular Q-learning / QRM learner fused into the step (include/rmx.h "tabular Q-learning / QRM learners",
rmx.learn.VecQLearning) on host handles: against fixtures recorded from the reference's own QLearning, against a plain
Python restatement on randomised worlds (tests/learnref.py), the engine's policy, the step's own columns against a
twin stepped with rmx_step, every refusal, and the host path under AddressSanitizer / UBSan as a stand-alone program.
"""
import ctypes as C
import dataclasses
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import learn_common as LC
import learnref as LR
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv
from rmx.learn import VecQLearning
from test_random_maps_gpu import CASES, random_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_recorded_fixture_is_present():
    assert LC.FIXTURES == LC.EXPECTED


@pytest.mark.parametrize("case", LC.EXPECTED)
def test_fixtures_from_the_reference_qlearning(case):
    LC.replay_fixture(case, HostRMEnv, lambda a: a)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("use_qrm", [True, False])
@pytest.mark.parametrize("lr", [None, 0.3])
def test_host_equals_the_python_restatement_on_random_worlds(name, use_qrm, lr):
    tab = random_tables(*CASES[name])
    rsh = use_qrm and tab.phi is not None
    N, K = 3, 70  # max_t = 60: truncation and an auto-reset fall inside the run
    env = HostRMEnv(tab, N)
    twin = HostRMEnv(tab, N, with_qrm=True, with_enc_state=True)
    L = VecQLearning(env, 0.9, lr, qtable_init=0.5, use_qrm=use_qrm, use_rsh=rsh)
    R = LR.LearnRef(twin, 0.9, lr, qtable_init=0.5, use_qrm=use_qrm, use_rsh=rsh)
    acts = env.fill_actions(9, 0, K)
    for t in range(K):
        L.step(acts[t])
        R.step(acts[t])
    assert np.array_equal(LC.bits(L.q), LC.bits(R.q))
    assert np.array_equal(L.visits, R.visits)
    assert (R.visits > 0).any() and (env.t < K).any()  # something was learnt, an env was reset


def _policy_pair(tab, N, **kw):
    env = HostRMEnv(tab, N, env_offset=5, n_envs_global=100)
    twin = HostRMEnv(tab, N, env_offset=5, n_envs_global=100, with_qrm=True, with_enc_state=True)
    return env, twin, VecQLearning(env, 0.9, 0.2, **kw), LR.LearnRef(twin, 0.9, 0.2, **kw)


def test_policy_epsilon_one_is_fill_actions():
    tab = T.compile_scenario(T.baseline_scenario(2))
    env, _, L, _ = _policy_pair(tab, 7, use_qrm=True)
    out = np.full((tab.n_agents, 7), -1, np.int32)
    for t in range(5):
        L.act_step(1.0, 77, t, actions_out=out)
        assert np.array_equal(out, env.fill_actions(77, t, 1)[0])


def test_policy_ties_on_an_untouched_table_follow_the_hash():
    tab = T.compile_scenario(T.baseline_scenario(2))
    env, twin, L, R = _policy_pair(tab, 64, use_qrm=True)
    out = np.zeros((tab.n_agents, 64), np.int32)
    want = R.choose(0.0, 3, 0)
    L.act_step(0.0, 3, 0, learn=False, actions_out=out)
    assert np.array_equal(out, want)
    assert sorted(set(out.ravel().tolist())) == [0, 1, 2, 3]  # four-way ties: every action is drawn
    assert not np.array_equal(out, env.fill_actions(3, 0, 1)[0])  # (its own draw, not the explore action)


@pytest.mark.parametrize("best", [False, True])
def test_policy_steps_equal_the_restatement(best):
    tab = random_tables(*CASES["ow_regs_eligible"])
    env, twin, L, R = _policy_pair(tab, 6, use_qrm=True, use_rsh=True)
    out = np.zeros((tab.n_agents, 6), np.int32)
    for t in range(90):
        want = R.choose(0.3, 11, t, best=best)
        L.act_step(0.3, 11, t, best=best, actions_out=out)
        assert np.array_equal(out, want), t
        R.step(want)
    assert np.array_equal(LC.bits(L.q), LC.bits(R.q)) and np.array_equal(L.visits, R.visits)
    assert np.array_equal(L.greedy(), R.choose(0.0, 0, 0, best=True, autoreset=False))


def test_step_without_update_leaves_the_tables_untouched():
    tab = T.compile_scenario(T.baseline_scenario(2))
    env, _, L, _ = _policy_pair(tab, 9, use_qrm=True)
    for t in range(20):
        L.act_step(0.5, 1, t)
    q, v, t0 = L.q.copy(), L.visits.copy(), env.t.copy()
    for t in range(20, 30):
        L.act_step(0.5, 1, t, learn=False)
        L.act_step(0.0, 1, t, best=True, learn=False)
    assert np.array_equal(LC.bits(L.q), LC.bits(q)) and np.array_equal(L.visits, v)
    assert not np.array_equal(env.t, t0)  # (the envs did step)


@pytest.mark.parametrize("name", ["fl_small_merged", "ow_regs_eligible"])
def test_learn_steps_leave_the_columns_and_statistics_as_rmx_step(name):
    tab = random_tables(*CASES[name])
    N, K = 5, 150
    kw = dict(with_qrm=True, with_enc_state=True)
    env, twin = HostRMEnv(tab, N, **kw), HostRMEnv(tab, N, **kw)
    L = VecQLearning(env, 0.9, 0.1, use_qrm=True)
    acts = env.fill_actions(4, 0, K)
    acts[17, 0, 2] = 4  # wait: stepped, no table column
    acts[40, 0, 1] = 9  # invalid: stepped as wait and reported, as rmx_step does
    for t in range(K):
        L.step(acts[t])
        twin.step(acts[t])
        if t % 37 == 0 or t == K - 1:
            LC.assert_same_columns(LC.columns(env), LC.columns(twin), (name, t))
    assert np.array_equal(env.stats().view(np.uint64), twin.stats().view(np.uint64))
    assert env.stats()[_capi.STAT_EPISODES] > 0
    for e in (env, twin):
        with pytest.raises(ValueError, match="action"):
            e.check_errors()


# ---- refusals ------------------------------------------------------------------------------------------------------
def _raw(tab, n=4, bind=True):
    lib = _capi.load_library()
    cfg, keep = _capi.make_config(tab, n, device=_capi.DEVICE_HOST)
    h = C.c_void_p()
    assert lib.rmx_create(C.byref(cfg), C.byref(h)) == 0, lib.rmx_last_error()
    cols = None
    if bind:
        A = tab.n_agents
        cols = [np.zeros((A, n), np.int32) for _ in range(3)] + [np.zeros((A, n), np.uint32), np.zeros((A, n), np.float32),
                                                                  np.zeros(n, np.int32), np.zeros((A, n), np.float32)]
        b = _capi.RmxBuffers(*[c.ctypes.data for c in cols])
        assert lib.rmx_bind(h, C.byref(b)) == 0
        assert lib.rmx_reset(h, None, 0, None) == 0
    return lib, h, (cfg, keep, cols)


def _lcfg(**kw):
    c = _capi.RmxLearnConfig()
    c.gamma, c.learning_rate = 0.9, 0.1
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_refusals():
    lib = _capi.load_library()
    tab = T.compile_scenario(T.baseline_scenario(2))
    lib, h, keep = _raw(tab)
    s_max = C.c_int64()
    assert lib.rmx_learn_states(h, C.byref(s_max)) == 0 and s_max.value == 10 * 10 * 4
    q = np.ones((2, 4, s_max.value, 4))
    v = np.zeros_like(q)
    INV, STATE = _capi.RMX_E_INVALID, _capi.RMX_E_STATE

    def refused(cfg, qq, vv, word, handle=h):
        assert lib.rmx_learn_bind(handle, None if cfg is None else C.byref(cfg), qq, vv) == INV
        assert word.encode() in lib.rmx_last_error(), lib.rmx_last_error()

    acts = np.zeros((2, 4), np.int32)
    # a learn step before rmx_learn_bind
    assert lib.rmx_learn_step(h, acts.ctypes.data, 1, None) == STATE and b"rmx_learn_bind" in lib.rmx_last_error()
    assert lib.rmx_learn_step_policy(h, 0.1, 1, 0, 0, 1, None, None) == STATE
    refused(None, q.ctypes.data, None, "NULL")
    refused(_lcfg(), None, None, "q table")
    for bad in (float("nan"), float("inf"), -0.5):
        refused(_lcfg(gamma=bad), q.ctypes.data, None, "gamma")
        refused(_lcfg(learning_rate=bad), q.ctypes.data, None, "learning_rate")
    refused(_lcfg(learning_rate=0.0), q.ctypes.data, None, "visits")
    refused(_lcfg(use_rsh=1), q.ctypes.data, None, "use_rsh without use_qrm")
    refused(_lcfg(use_qrm=1, use_rsh=1), q.ctypes.data, None, "phi")
    # a good bind, then the step's own argument checks
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(use_qrm=1)), q.ctypes.data, v.ctypes.data) == 0
    assert lib.rmx_learn_step(h, None, 1, None) == INV and b"actions" in lib.rmx_last_error()
    assert lib.rmx_learn_step_policy(h, 1.5, 1, 0, 0, 1, None, None) == INV and b"epsilon" in lib.rmx_last_error()
    assert lib.rmx_learn_step_policy(h, float("nan"), 1, 0, 0, 1, None, None) == INV
    assert lib.rmx_learn_step_policy(h, 0.5, 8, 0, 0, 1, None, None) == INV and b"flags" in lib.rmx_last_error()
    assert lib.rmx_learn_step(h, acts.ctypes.data, 1, None) == 0 and v.sum() == 2 * 4 * 3
    lib.rmx_destroy(h)
    # no QRM state lists / no encoder strides
    lib, h2, keep2 = _raw(dataclasses.replace(tab, n_qrm=None, qrm_states=None))
    refused(_lcfg(use_qrm=1), q.ctypes.data, None, "n_qrm_max", h2)
    lib.rmx_destroy(h2)
    lib, h3, keep3 = _raw(dataclasses.replace(tab, n_qrm=None, qrm_states=None, enc_nq=None))
    refused(_lcfg(), q.ctypes.data, None, "enc_nq", h3)
    assert lib.rmx_learn_states(h3, C.byref(s_max)) == INV
    lib.rmx_destroy(h3)
    # slip / random starts
    for extra in ({"stochastic": True}, {"random_start_positions": True}):
        tab_s = T.compile_scenario(dict(T.baseline_scenario(2), **extra))
        lib, h4, keep4 = _raw(tab_s, bind=False)
        refused(_lcfg(), q.ctypes.data, None, "deterministic dynamics", h4)
        lib.rmx_destroy(h4)
    # a learn step before rmx_bind
    lib, h5, keep5 = _raw(tab, bind=False)
    assert lib.rmx_learn_bind(h5, C.byref(_lcfg()), q.ctypes.data, None) == 0
    assert lib.rmx_learn_step(h5, acts.ctypes.data, 1, None) == STATE and b"rmx_bind" in lib.rmx_last_error()
    lib.rmx_destroy(h5)


def test_null_handles_are_rejected_without_touching_a_gpu():
    lib = _capi.load_library()
    INV = _capi.RMX_E_INVALID
    assert lib.rmx_learn_states(None, None) == INV
    assert lib.rmx_learn_bind(None, C.byref(_lcfg()), None, None) == INV and b"NULL" in lib.rmx_last_error()
    assert lib.rmx_learn_step(None, None, 1, None) == INV and b"NULL" in lib.rmx_last_error()
    assert lib.rmx_learn_step_policy(None, 0.1, 1, 0, 0, 1, None, None) == INV and b"NULL" in lib.rmx_last_error()


def test_python_class_refuses_shaping_without_qrm():
    tab = T.compile_scenario(T.baseline_scenario(5))
    env = HostRMEnv(tab, 2)
    with pytest.raises(ValueError, match="use_rsh without use_qrm"):
        VecQLearning(env, 0.9, 0.1, use_rsh=True)
    with pytest.raises(ValueError, match="learning_rate"):
        VecQLearning(env, 0.9, 0.0)
    import rmx
    assert rmx.VecQLearning is VecQLearning


# ---- the host learn step as a stand-alone program under AddressSanitizer + UBSan ----------------------------------
def _digest(tab, n, steps):
    """learn_host_main.cpp's sequence through librmx.so's host handle."""
    d = 0xcbf29ce484222325
    for mode in range(2):
        env = HostRMEnv(tab, n)
        env.reset(seed=5)
        L = VecQLearning(env, 0.9, 0.1 if mode == 0 else None, use_qrm=mode == 0)
        for s in range(steps):
            if s % 4 == 3:
                L.act_step(0.3, 11, s)
            else:
                L.step(env.fill_actions(11, s, 1)[0])
        for col in (L.q, L.visits):
            for byte in col.tobytes():
                d = ((d ^ byte) * 0x100000001b3) & (2**64 - 1)
    return d


def test_host_learn_step_clean_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler for the sanitizer build")
    with open(os.path.join(ROOT, "tests", "golden", "configs.json")) as f:
        import json
        tab = T.compile_scenario(json.load(f)["fl2"])
    n, steps = 3, 200
    A, Qx = tab.n_agents, tab.qrm_states.shape[1]
    blob = struct.pack("<8i4f4i", tab.kind, tab.width, tab.height, A, tab.n_rm_states, tab.n_events, tab.max_t, Qx,
                       tab.hazard_penalty, tab.wall_penalty, tab.gamma, tab.reward_modifier, tab.hazard_fail,
                       tab.wall_fail, n, steps)
    for arr, dt in ((tab.cell, np.uint16), (tab.cell_event, np.uint8), (tab.next_q, np.uint8),
                    (tab.rm_reward, np.float32), (tab.init_q, np.int32), (tab.final_q, np.int32),
                    (tab.start_xy, np.int32), (tab.n_qrm, np.int32), (tab.qrm_states, np.uint8), (tab.enc_nq, np.int32)):
        blob += np.ascontiguousarray(arr, dt).tobytes()
    cfg_path = tmp_path / "fl2.bin"
    cfg_path.write_bytes(blob)
    csrc = os.path.join(ROOT, "multiagent-rl-rm_amd", "csrc")
    exe = str(tmp_path / "learn_host_main")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "data", "learn_host_main.cpp"),
                    os.path.join(csrc, "rmx_hoststep.cpp"), os.path.join(csrc, "rmx_tables.cpp")], check=True)
    # the sanitizer runtimes are linked statically, so the program does not depend on the load order of whatever the
    # inherited environment preloads; the environment is passed on as it is, plus the sanitizers' options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(cfg_path)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    got = next(ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("LEARN_HOST_DIGEST"))
    assert int(got, 16) == _digest(tab, n, steps)
