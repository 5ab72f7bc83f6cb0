"""The Watkins Q(lambda) learners fused into the step (include/rmx.h "Watkins Q(lambda) learners", rmx.learn.VecQLambda)
on host handles: against fixtures recorded from the reference's own QLearningLambda, against the tests' dense numpy
restatement on randomised worlds (tests/lambda_common.py over tests/learnref.py), the list capacity, every refusal,
when the lists are emptied and when they are left alone, and the shared update as a stand-alone program under
AddressSanitizer / UBSan.
"""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import lambda_common as MC
import learn_common as LC
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv
from rmx.learn import VecQLambda, VecQLearning
from test_learn_cpu import _lcfg, _raw
from test_random_maps_gpu import random_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FL, OW = T.FROZEN_LAKE, T.OFFICE_WORLD


def test_every_recorded_fixture_is_present():
    assert MC.FIXTURES == MC.EXPECTED


@pytest.mark.parametrize("case", MC.EXPECTED)
def test_fixtures_from_the_reference_qlearning_lambda(case):
    cov = MC.replay_fixture(case, HostRMEnv, lambda a: a)
    # what the recorder asserted of the reference's run is what this replay went through
    want = {"fl2_lr": ("term_wipes",), "fl2_open_visits": ("trunc_terminal",), "fl2_open_underflow": ("underflows", "revisits"),
            "ow2_plain": ("trunc_live", "reset_wipes"), "fl2_policy": ("term_wipes",), "fl2_slip_policy": ("resets",)}[case]
    assert all(cov[k] >= 1 for k in want), cov
    if case == "fl2_open_visits":
        assert cov["longest"] > 64


# A = 1, 2, 3, 5, 8 (every AMAX bucket of the device kernel but 4, which the GPU file runs), both kinds, ragged N
RANDOM = {
    "ow_a1": (4, OW, 9, 7, 1, 4, 5, True, 1),
    "fl_a2": (1, FL, 6, 6, 2, 3, 3, False, 3),
    "fl_a3": (3, FL, 7, 6, 3, 4, 5, False, 2),
    "fl_a5": (11, FL, 8, 7, 5, 5, 8, False, 3),
    "ow_a8": (13, OW, 10, 8, 8, 6, 10, True, 2),
}


@pytest.mark.parametrize("name", sorted(RANDOM))
@pytest.mark.parametrize("lr", [None, 0.3])
def test_host_equals_the_dense_restatement_on_random_worlds(name, lr):
    *args, N = RANDOM[name]
    tab = dataclasses.replace(random_tables(*args), max_t=20)
    K = 70  # max_t = 20: truncations and auto-resets fall inside the run
    env = HostRMEnv(tab, N)
    twin = HostRMEnv(tab, N, with_qrm=True, with_enc_state=True)
    tit = False if name == "fl_a3" else None  # a lake with the OfficeWorld runner's rule as well: truncations decay
    L = VecQLambda(env, 0.9, 0.7, lr, trunc_is_terminal=tit)
    R = MC.DenseLambda(twin, 0.9, 0.7, lr, trunc_is_terminal=tit)
    acts = env.fill_actions(9, 0, K)
    acts[17, 0, 0] = 4  # wait: stepped, no table column, no list touched
    for t in range(K):
        L.step(acts[t])
        R.step(acts[t])
        if t % 9 == 0 or t == K - 1:
            LC.assert_same_bits(L.q, R.q, (name, t, "q"))
            assert np.array_equal(L.visits, R.visits), (name, t)
            LC.assert_same_bits(L.traces(), R.e, (name, t, "traces"))
            assert np.array_equal(L.trace_counts(), np.count_nonzero(R.e.reshape(env.A, N, -1), axis=-1))
    MC.assert_list_invariant(L)
    assert (R.visits > 0).any() and (env.t < K).all() and (R.e != 0).any()
    assert L.trace_counts().max() <= tab.max_t + 1  # (the documented bound under auto-resetting learn steps)
    env.check_errors()


def test_lambda_zero_leaves_every_count_zero():
    tab = T.compile_scenario(T.baseline_scenario(2))
    env = HostRMEnv(tab, 5)
    L = VecQLambda(env, 0.9, 0.0, 0.2, trace_cap=1)
    Q = VecQLearning(HostRMEnv(tab, 5), 0.9, 0.2, qtable_init=0.0, use_qrm=False)
    for t in range(80):
        L.act_step(0.5, 3, t)
        Q.act_step(0.5, 3, t)
        assert not L.trace_counts().any()
    env.check_errors()
    assert (L.visits > 0).any() and np.array_equal(L.visits, Q.visits)  # (one-step Q-learning's visits, its own arithmetic)


def _canaried(shape, dtype, fill):
    """An array of `shape` inside a larger allocation, with 64 canary elements either side."""
    n = int(np.prod(shape))
    raw = np.full(n + 128, fill, dtype)
    return raw, raw[64:64 + n].reshape(shape)


def cap_overflow(env, to_actions=lambda a: a, steps=33):
    """trace_cap = 3 on `env` over canaried arrays: RMX_E_TRACE, counts never above 3, canaries intact.  Shared with the
    GPU file (there the arrays are views of larger tensors)."""
    host = getattr(env, "device", None) == "cpu"
    A, N = env.A, env.N
    L = VecQLambda(env, 0.9, 0.9, 0.3, trace_cap=3)
    if host:
        raws, views = zip(_canaried((A, 3, N), np.int32, -7), _canaried((A, 3, N), np.float64, -7.0),
                          _canaried((A, N), np.int32, -7))
        views[2][...] = 0
    else:
        t = env.torch
        raws = [t.full((n + 128,), -7, dtype=dt, device=env.device)
                for n, dt in ((A * 3 * N, t.int32), (A * 3 * N, t.float64), (A * N, t.int32))]
        views = [raws[0][64:64 + A * 3 * N].view(A, 3, N), raws[1][64:64 + A * 3 * N].view(A, 3, N),
                 raws[2][64:64 + A * N].view(A, N)]
        views[2].zero_()
    L.bind_traces(views[0], views[1], views[2], 3)
    acts = HostRMEnv(env.tables, N).fill_actions(5, 0, steps)
    for k in range(steps):
        L.step(to_actions(acts[k]))
        assert L.trace_counts().max() <= 3
    assert L.trace_counts().max() == 3
    with pytest.raises(RuntimeError, match="trace") as ei:
        env.check_errors()
    assert f"rc={_capi.RMX_E_TRACE}" in str(ei.value)
    env.check_errors()  # reported once, then cleared
    for raw in raws:
        r = LC.host(raw)
        assert (r[:64] == -7).all() and (r[-64:] == -7).all()
    MC.assert_list_invariant(L)
    # the cell's own update was applied all the same: every step visited a cell
    assert LC.host(L.visits).sum() == steps * A * N
    # an invalid action reported at the same time wins, and clears both
    bad = acts[0].copy()
    bad[0, 0] = 9
    for k in range(8):
        L.step(to_actions(bad if k == 0 else acts[k]))
    with pytest.raises(ValueError, match="action"):
        env.check_errors()
    env.check_errors()
    return L


def test_a_full_list_drops_the_trace_and_reports_it():
    tab = dataclasses.replace(random_tables(1, FL, 6, 6, 2, 3, 3, False), max_t=20)
    cap_overflow(HostRMEnv(tab, 5))


def test_refusals():
    lib = _capi.load_library()
    tab = T.compile_scenario(T.baseline_scenario(2))
    lib, h, keep = _raw(tab)
    INV, STATE = _capi.RMX_E_INVALID, _capi.RMX_E_STATE
    full = C.c_int32()
    assert lib.rmx_learn_lambda_slots(h, C.byref(full)) == 0 and full.value == 4 * 10 * 10 * 4
    assert lib.rmx_learn_lambda_slots(None, C.byref(full)) == INV and lib.rmx_learn_lambda_slots(h, None) == INV
    A, N, S4 = 2, 4, full.value
    q = np.zeros((A, N, S4 // 4, 4))
    v = np.zeros_like(q)
    idx, val, cnt = np.zeros((A, S4, N), np.int32), np.zeros((A, S4, N), np.float64), np.zeros((A, N), np.int32)
    p = lambda x: x.ctypes.data  # noqa: E731

    def refused(word, lambd=0.5, cap=S4, i=p(idx), w=p(val), c=p(cnt), code=INV, handle=h):
        assert lib.rmx_learn_lambda_bind(handle, lambd, cap, i, w, c) == code, lib.rmx_last_error()
        assert word.encode() in lib.rmx_last_error(), lib.rmx_last_error()

    # before rmx_learn_bind
    refused("rmx_learn_bind", code=STATE)
    assert lib.rmx_learn_traces_clear(h, None, None) == STATE and b"rmx_learn_lambda_bind" in lib.rmx_last_error()
    assert lib.rmx_learn_lambda_bind(None, 0.5, S4, p(idx), p(val), p(cnt)) == INV
    assert lib.rmx_learn_traces_clear(None, None, None) == INV
    # a learner bound with use_qrm
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(use_qrm=1)), p(q), p(v)) == 0
    refused("use_qrm")
    phi = np.zeros((A, tab.n_rm_states))
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(use_qrm=1, use_rsh=1, phi=p(phi))), p(q), p(v)) == 0
    refused("use_qrm")
    assert lib.rmx_learn_bind(h, C.byref(_lcfg()), p(q), p(v)) == 0
    for bad in (float("nan"), float("inf"), -0.1, 1.0 + 2.0 ** -52):
        refused("lambd", lambd=bad)
    for bad in (0, -1, S4 + 1):
        refused("cap", cap=bad)
    refused("NULL", w=None)
    refused("NULL", c=None)
    refused("aligned", i=p(idx) + 2)
    refused("aligned", w=p(val) + 4)
    refused("aligned", c=p(cnt) + 1)
    # nothing was bound by the refused calls: the steps are still Q-learning's, and there is nothing to clear
    assert lib.rmx_learn_traces_clear(h, None, None) == STATE
    acts = np.zeros((A, N), np.int32)
    assert lib.rmx_learn_step(h, p(acts), 1, None) == 0 and not cnt.any()
    # a good bind (lambd = 0 and 1 are in range), then a NULL idx unbinds, and a later rmx_learn_bind drops the binding
    for lam in (0.0, 1.0, 0.5):
        assert lib.rmx_learn_lambda_bind(h, lam, S4, p(idx), p(val), p(cnt)) == 0
    assert lib.rmx_learn_step(h, p(acts), 1, None) == 0 and (cnt == 1).all()
    assert lib.rmx_learn_traces_clear(h, None, None) == 0 and not cnt.any()
    assert lib.rmx_learn_lambda_bind(h, 0.5, S4, None, None, None) == 0
    assert lib.rmx_learn_traces_clear(h, None, None) == STATE
    assert lib.rmx_learn_lambda_bind(h, 0.5, 1, p(idx), p(val), p(cnt)) == 0
    assert lib.rmx_learn_bind(h, C.byref(_lcfg()), p(q), p(v)) == 0
    assert lib.rmx_learn_traces_clear(h, None, None) == STATE
    assert lib.rmx_learn_step(h, p(acts), 1, None) == 0 and not cnt.any()
    assert lib.rmx_check_errors(h) == 0
    lib.rmx_destroy(h)


def _walk(tab, N, steps=12):
    env = HostRMEnv(tab, N)
    env.reset(seed=3)
    L = VecQLambda(env, 0.9, 0.8, 0.2)
    for t in range(steps):
        L.act_step(0.5, 3, t)
    assert (L.trace_counts() > 0).any(axis=0).all()  # (an agent that fell into a hole has had its terminal wipe)
    return env, L


def test_a_masked_reset_clears_only_the_masked_envs():
    tab = T.compile_scenario(T.baseline_scenario(2))
    env, L = _walk(tab, 7)
    before = L.trace_counts()
    mask = np.array([1, 0, 0, 1, 0, 1, 0], np.uint8)
    env.reset(mask=mask, seed=3)
    after = L.trace_counts()
    assert not after[:, mask == 1].any() and np.array_equal(after[:, mask == 0], before[:, mask == 0])
    L.clear_traces(mask=np.array([0, 1, 0, 0, 0, 0, 0], np.uint8))
    assert not L.trace_counts()[:, 1].any() and np.array_equal(L.trace_counts()[:, 2], before[:, 2])
    env.reset(seed=3)
    assert not L.trace_counts().any() and not L.traces().any()
    # rmx_reset_sync and rmx_set_state empty them too
    for again in ("reset_sync", "load_state"):
        for t in range(6):
            L.act_step(0.5, 3, t)
        assert L.trace_counts().any()
        if again == "reset_sync":
            env.reset_sync(seed=3)
        else:
            env.load_state(env.save_state())
        assert not L.trace_counts().any(), again


def test_a_step_without_update_leaves_the_lists_alone_but_wipes_on_auto_reset():
    tab = dataclasses.replace(T.compile_scenario(T.baseline_scenario(2)), max_t=15)
    env, L = _walk(tab, 6, steps=10)
    cnt, idx, val = L.trace_counts(), L.trace_idx.copy(), L.trace_val.copy()
    wiped = np.zeros(6, bool)
    for t in range(10, 30):
        resets = (env.flags[0] & _capi.F_ENV_DONE) != 0  # this step auto-resets these envs
        L.act_step(0.5, 3, t, learn=False)
        wiped |= resets
        now = L.trace_counts()
        assert not now[:, wiped].any() and np.array_equal(now[:, ~wiped], cnt[:, ~wiped]), t
    assert wiped.all()  # max_t = 15: every env ran into its step limit
    # until its wipe nothing of a list was rewritten (the slots of a wiped list stay as they were: only the count goes)
    assert np.array_equal(L.trace_idx, idx) and np.array_equal(LC.bits(L.trace_val), LC.bits(val))


def test_a_plain_step_leaves_the_lists_alone():
    tab = dataclasses.replace(T.compile_scenario(T.baseline_scenario(2)), max_t=15)
    env, L = _walk(tab, 6, steps=10)
    cnt, e, q = L.trace_counts(), L.traces(), L.q.copy()
    acts = env.fill_actions(8, 0, 30)
    for t in range(20):  # past the step limit: the plain steps' own auto-resets do not know the learners
        env.step(acts[t])
    env.step_seq(acts[20:25])
    env.rollout(3, 100, 5)
    assert env.stats()[_capi.STAT_EPISODES] > 0
    assert np.array_equal(L.trace_counts(), cnt) and np.array_equal(LC.bits(L.traces()), LC.bits(e))
    assert np.array_equal(LC.bits(L.q), LC.bits(q))
    L.clear_traces()
    assert not L.trace_counts().any()


def test_python_class():
    tab = T.compile_scenario(T.baseline_scenario(2))
    env = HostRMEnv(tab, 2)
    for bad in (0, 4 * 400 + 1):
        with pytest.raises(ValueError, match="cap"):
            VecQLambda(env, 0.9, 0.5, 0.1, trace_cap=bad)
    with pytest.raises(ValueError, match="lambd"):
        VecQLambda(env, 0.9, 1.5, 0.1)
    L = VecQLambda(env, 0.9, 0.5)
    assert L.trace_cap == L.trace_full == 4 * L.S_max and not L.q.any() and L.traces().shape == L.q.shape
    assert isinstance(L, VecQLearning) and VecQLambda.step is VecQLearning.step \
        and VecQLambda.act_step is VecQLearning.act_step and VecQLambda.greedy is VecQLearning.greedy
    with pytest.raises(ValueError, match="mask"):
        L.clear_traces(mask=np.zeros(3, np.uint8))
    import rmx
    assert rmx.VecQLambda is VecQLambda


# ---- the shared update as a stand-alone program under AddressSanitizer + UBSan ----------------------------------------
def test_shared_update_clean_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler for the sanitizer build")
    exe = str(tmp_path / "lambda_update_main")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(ROOT, "tests", "data", "lambda_update_main.cpp")], check=True)
    # the sanitizer runtimes are linked statically, so the program does not depend on the load order of whatever the
    # inherited environment preloads; the environment is passed on as it is, plus the sanitizers' options
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    assert "LAMBDA_UPDATE_OK" in r.stdout
