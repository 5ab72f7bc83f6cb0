"""The QR-max learners in the learn step (include/rmx.h "QR-max learners", rmx.learn.VecQRMax) on host handles: against
fixtures recorded from the reference's own QRMax_v2 (every table bit for bit, the slip cases included), every refusal
of the bind and of rmx_learn_run, exclusivity with the Q(lambda) and R-max bindings, the successor-list capacity over
canaried arrays, run(T) against T single steps, known() / env_transitions(), unbind, and the shared rules as a
stand-alone program under AddressSanitizer and UBSan.
"""
import ctypes as C
import dataclasses
import os
import shutil
import subprocess

import numpy as np
import pytest

import learn_common as LC
import qrmax_common as QC
import slearn_common as SC
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv
from rmx.learn import VecQLearning, VecQRMax
from test_learn_cpu import _lcfg, _raw
from test_random_maps_gpu import random_tables

FL, OW = T.FROZEN_LAKE, T.OFFICE_WORLD


def test_the_abi_version_is_unchanged():
    assert _capi.load_library().rmx_abi_version() == 12


def test_every_recorded_fixture_is_present():
    assert QC.FIXTURES == QC.EXPECTED


@pytest.mark.parametrize("case", QC.EXPECTED)
def test_fixtures_from_the_reference_qrmax(case):
    cov = QC.replay_fixture(case, HostRMEnv, lambda a: a)
    # what the recorder asserted of the reference's run is what this replay went through
    want = {"ow2_t1": ("solves", "resets"), "ow3_qrm_t2": ("shortcuts", "many_known_one_solve"),
            "fl2_open_t3": ("trunc_final", "final_row_nonzero"), "fl2_numpy_t1": ("flat_draws", "argmax_picks"),
            "fl2_slip_t3": ("solves",), "fl2_rel_t2": ("solves",), "fl2_slip_tq2": ("dropped_mass",)}[case]
    assert all(cov[k] >= 1 for k in want), cov
    assert (cov["max_succ"] >= 3) == (case in ("fl2_slip_t3", "fl2_slip_tq2"))


def _model(A, N, S, P, cap=5):
    sq, sa, s = (A, N, S, 4), (A, N, P, 4), (A, N, S)
    return dict(known_tsqa=np.zeros(sq, np.uint8), n_tsa=np.zeros(sa, np.int32), n_rsa=np.zeros(sa, np.int32),
                sum_rsa=np.zeros(sa), succ_idx=np.zeros(sa + (cap,), np.int32), succ_cnt=np.zeros(sa + (cap,), np.int32),
                n_tqs=np.zeros(s, np.int32), tq_next=np.zeros(s, np.int32), n_rqs=np.zeros(s, np.int32),
                sum_rqs=np.zeros(s), final=np.zeros(s, np.uint8))


def test_refusals():
    tab = T.compile_scenario(T.baseline_scenario(2))
    lib, h, keep = _raw(tab)
    INV, STATE = _capi.RMX_E_INVALID, _capi.RMX_E_STATE
    full = C.c_int32()
    assert lib.rmx_learn_qrmax_slots(h, C.byref(full)) == 0 and full.value == 5
    assert lib.rmx_learn_qrmax_slots(None, C.byref(full)) == INV and lib.rmx_learn_qrmax_slots(h, None) == INV
    A, N, S, P = 2, 4, 10 * 10 * 4, 100
    q = np.full((A, N, S, 4), 2.0)
    v = np.zeros_like(q)
    m = _model(A, N, S, P)
    p = lambda x: x.ctypes.data  # noqa: E731
    ptrs = {k: p(m[k]) for k in VecQRMax.MODEL}

    def bind(handle=h, te=2, re_=2, tq=1, rq=1, delta=1e-3, rel=0, it=100, cap=5, **over):
        a = dict(ptrs, **over)
        return lib.rmx_learn_qrmax_bind(handle, te, re_, tq, rq, delta, rel, it, cap, *[a[k] for k in VecQRMax.MODEL])

    def refused(word, code=INV, **kw):
        assert bind(**kw) == code, lib.rmx_last_error()
        assert word.encode() in lib.rmx_last_error(), lib.rmx_last_error()

    # before rmx_learn_bind
    refused("rmx_learn_bind", code=STATE)
    assert bind(handle=None) == INV
    n, mx, tot = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.rmx_learn_qrmax_info(h, C.byref(n), C.byref(mx), C.byref(tot)) == STATE
    # a learner with shaping, without visits, with gamma >= 1
    phi = np.zeros((A, tab.n_rm_states))
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(gamma=0.5, use_qrm=1, use_rsh=1, phi=p(phi))), p(q), p(v)) == 0
    refused("use_rsh")
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(gamma=0.5)), p(q), None) == 0
    refused("visits")
    for g in (1.0, 1.5):
        assert lib.rmx_learn_bind(h, C.byref(_lcfg(gamma=g)), p(q), p(v)) == 0
        refused("gamma")
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(gamma=0.5, use_qrm=1)), p(q), p(v)) == 0
    for name in ("te", "re_", "tq", "rq"):
        for bad in (0, -3):
            refused("threshold", **{name: bad})
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        refused("vi_delta", delta=bad)
    for bad in (0, -1):
        refused("max_iter", it=bad)
    for bad in (0, -1, 6):
        refused("cap", cap=bad)
    for name in VecQRMax.MODEL[1:]:  # (a NULL first array unbinds)
        refused("NULL", **{name: None})
    for name in ("sum_rsa", "sum_rqs"):
        refused("aligned", **{name: ptrs[name] + 4})
    for name in ("n_tsa", "n_rsa", "succ_idx", "succ_cnt", "n_tqs", "tq_next", "n_rqs"):
        refused("aligned", **{name: ptrs[name] + 2})
    assert lib.rmx_learn_qrmax_info(h, None, C.byref(mx), C.byref(tot)) == INV
    # nothing was bound by the refused calls: the steps are still Q-learning's
    acts = np.zeros((A, N), np.int32)
    assert lib.rmx_learn_step(h, p(acts), 1, None) == 0 and not any(a.any() for a in m.values())
    assert lib.rmx_learn_qrmax_info(h, C.byref(n), C.byref(mx), C.byref(tot)) == STATE
    # a good bind; Q(lambda) lists and an R-max model are refused while it stands; rmx_learn_run is refused
    assert bind() == 0
    ti, tv, tc = np.zeros((A, 8, N), np.int32), np.zeros((A, 8, N)), np.zeros((A, N), np.int32)
    assert lib.rmx_learn_lambda_bind(h, 0.5, 8, p(ti), p(tv), p(tc)) == STATE and b"QR-max" in lib.rmx_last_error()
    rsum, ri, rc = np.zeros_like(q), np.zeros((A, N, S, 4, 5), np.int32), np.zeros((A, N, S, 4, 5), np.int32)
    assert lib.rmx_learn_rmax_bind(h, 2, 1e-3, 0, 100, 5, p(rsum), p(ri), p(rc)) == STATE
    assert b"QR-max" in lib.rmx_last_error()
    assert lib.rmx_learn_run(h, 3, 0.0, _capi.LEARN_UPDATE, 1, 0, None, None) == STATE
    assert b"rmx_learn_run" in lib.rmx_last_error() and b"QR-max" in lib.rmx_last_error()
    assert lib.rmx_learn_step(h, p(acts), 1, None) == 0 and m["succ_cnt"].any() and (v > 0).any()
    assert lib.rmx_learn_qrmax_info(h, C.byref(n), C.byref(mx), C.byref(tot)) == 0 and n.value >= 0
    # a NULL first array unbinds; then the lists bind, and refuse the model; likewise an R-max model; a later
    # rmx_learn_bind drops either binding
    assert bind(known_tsqa=None) == 0
    assert lib.rmx_learn_run(h, 1, 0.0, _capi.LEARN_UPDATE, 1, 0, None, None) == 0
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(gamma=0.5)), p(q), p(v)) == 0
    assert lib.rmx_learn_lambda_bind(h, 0.5, 8, p(ti), p(tv), p(tc)) == 0
    refused("lambda", code=STATE)
    assert lib.rmx_learn_lambda_bind(h, 0.5, 8, None, None, None) == 0
    assert lib.rmx_learn_rmax_bind(h, 2, 1e-3, 0, 100, 5, p(rsum), p(ri), p(rc)) == 0
    refused("R-max", code=STATE)
    assert lib.rmx_learn_rmax_bind(h, 0, 0.0, 0, 0, 0, None, None, None) == 0
    assert bind(rel=1, cap=1) == 0
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(gamma=0.5)), p(q), p(v)) == 0
    assert lib.rmx_learn_qrmax_info(h, C.byref(n), C.byref(mx), C.byref(tot)) == STATE
    before = m["succ_cnt"].copy()
    assert lib.rmx_learn_step(h, p(acts), 1, None) == 0 and np.array_equal(m["succ_cnt"], before)
    assert lib.rmx_check_errors(h) == 0
    lib.rmx_destroy(h)


def test_python_refusals_and_the_initial_value():
    tab = T.compile_scenario(T.baseline_scenario(2))
    env = HostRMEnv(tab, 3)
    with pytest.raises(ValueError, match="gamma"):
        VecQRMax(env, 1.0)
    for kw, word in ((dict(nsamples_te=0), "threshold"), (dict(nsamples_rq=0), "threshold"), (dict(vi_delta=0.0), "vi_delta"),
                     (dict(max_iter=0), "max_iter"), (dict(succ_cap=0), "cap"), (dict(succ_cap=6), "cap")):
        with pytest.raises(ValueError, match=word):
            VecQRMax(env, 0.9, **kw)
    L = VecQRMax(env, 0.9, nsamples_te=2, nsamples_re=2, max_reward=0.5)
    assert L.n_tsqa is L.visits and L.succ_cap == L.succ_full == 5
    for a in range(env.A):  # R_max = max_reward * nQ, per agent
        assert (L.q[a] == 0.5 * int(tab.enc_nq[a]) / (1.0 - 0.9)).all()
    with pytest.raises(ValueError, match="epsilon"):
        L.act_step(0.1, 3, 0)
    with pytest.raises(ValueError, match="epsilon"):
        L.run(2, 0.1, 3, 0)
    with pytest.raises(RuntimeError, match="rmx_learn_run"):
        VecQLearning.run(L, 2, None, 3, 0)
    with pytest.raises(ValueError, match="arrays"):
        L.bind_model(5, n_tsa=L.n_tsa)


def test_agents_with_different_rm_sizes_start_at_their_own_value():
    tab = dataclasses.replace(random_tables(2, OW, 12, 10, 4, 6, 7, True), max_t=20)
    env = HostRMEnv(tab, 2)
    L = VecQRMax(env, 0.5)
    for a in range(env.A):
        assert (L.q[a] == int(tab.enc_nq[a]) / 0.5).all()


def test_a_full_list_drops_the_entry_and_keeps_the_canaries():
    tab = SC.fl_slip_randstart_world()  # A = 5, slip and random starts, max_t = 20
    QC.cap_overflow(HostRMEnv(tab, 5))


def _walked(tab, N, K=40, **kw):
    env = HostRMEnv(tab, N)
    env.reset(seed=4)
    L = VecQRMax(env, 0.5, vi_delta=1e-3, **kw)
    for t in range(K):
        L.act_step(None, 7, t)
    return env, L


def _same(a, b):
    for k in a:
        x, y = (LC.bits(a[k]), LC.bits(b[k])) if a[k].dtype == np.float64 else (a[k], b[k])
        assert np.array_equal(x, y), k


def test_run_equals_single_steps():
    tab = dataclasses.replace(random_tables(1, FL, 6, 6, 2, 3, 3, False), max_t=20)
    seeds = np.arange(2 * 4, dtype=np.uint64).reshape(2, 4) + 11
    for stream in (False, True):
        envs = [HostRMEnv(tab, 4) for _ in range(2)]
        for e in envs:
            e.reset(seed=4)
        La, Lb = (VecQRMax(e, 0.5, nsamples_te=2, nsamples_re=2, vi_delta=1e-3, policy_seeds=seeds) for e in envs)
        oa, ob = np.full((30, 2, 4), -1, np.int32), np.full((30, 2, 4), -1, np.int32)
        La.run(30, None, 7, 0, reference_stream=stream, actions_out=oa)
        for t in range(30):
            Lb.act_step(None, 7, t, reference_stream=stream, actions_out=ob[t])
        assert np.array_equal(oa, ob) and (oa >= 0).all()
        _same(QC.model_of(La), QC.model_of(Lb))
        assert np.array_equal(La.rng, Lb.rng) and La.solve_info() == Lb.solve_info() and La.solve_info()[0] > 0
        LC.assert_same_columns(LC.columns(envs[0]), LC.columns(envs[1]), "columns")


def test_best_and_no_learn_steps_leave_the_model_alone():
    tab = dataclasses.replace(random_tables(1, FL, 6, 6, 2, 3, 3, False), max_t=20)
    env, L = _walked(tab, 5, nsamples_te=2, nsamples_re=2)
    assert L.solve_info()[0] > 0 and L.known().any()
    before, solves = QC.model_of(L), L.solve_info()
    out = np.full((2, 5), -1, np.int32)
    for t in range(40, 70):
        L.act_step(None, 7, t, best=(t % 2 == 0), learn=False, actions_out=out)
        assert ((out >= 0) & (out < 4)).all()
    _same(before, QC.model_of(L))
    assert L.solve_info() == solves and (env.t > 0).any()
    want = L.greedy()  # best=True is np.argmax of the row whatever the row, whatever the seed
    L.act_step(None, 123, 999, best=True, learn=False, autoreset=False, actions_out=out)
    assert np.array_equal(out, want)
    env.check_errors()


def test_the_shuffle_is_drawn_under_best_too():
    tab = dataclasses.replace(random_tables(1, FL, 6, 6, 2, 3, 3, False), max_t=20)
    env = HostRMEnv(tab, 3)
    env.reset(seed=4)
    L = VecQRMax(env, 0.5, policy_seeds=np.arange(6, dtype=np.uint64).reshape(2, 3))
    out = np.full((2, 3), -1, np.int32)
    for best in (True, False):
        before = L.rng.copy()
        want = L.greedy()
        L.act_step(best=best, learn=False, autoreset=False, reference_stream=True, actions_out=out)
        assert (L.rng[:2] != before[:2]).any(axis=0).all()  # every learner's generator moved
        if best:
            assert np.array_equal(out, want)
    # the shuffle is numpy's own: three random_interval draws on a 4-list, then choice on the shuffled list
    g = np.random.default_rng(0)  # learner (0, 0) has seed 0; its second call meets a flat row
    g.shuffle([0, 1, 2, 3])
    acts = [0, 1, 2, 3]
    g.shuffle(acts)
    assert out[0, 0] == g.choice(acts)
    assert L.rng_state(0, 0) == g.bit_generator.state


def test_known_and_env_transitions():
    tab = dataclasses.replace(random_tables(2, OW, 12, 10, 4, 6, 7, True), max_t=20)
    env, L = _walked(tab, 3, nsamples_te=2, nsamples_re=2, use_qrm=True)
    QC.assert_list_invariant(L)
    tr, known = L.env_transitions(), L.known()
    assert tr.shape == (4, 3, L.P, 4, L.P) and known.shape == (4, 3, L.S_max, 4) and known.dtype == bool
    assert np.array_equal(tr.sum(axis=-1), L.n_tsa)  # the full cap drops nothing
    assert known.any() and not known.all()
    assert (np.count_nonzero(tr, axis=-1) <= 1).all()  # a deterministic world: one successor
    # value iteration wrote known or final entries only: every other entry still holds the optimistic value
    for a in range(env.A):
        S, nq = L.n_states[a], int(tab.enc_nq[a])
        untouched = ~known[a, :, :S] & ~(L.final[a, :, :S, None] != 0)
        assert (L.q[a, :, :S][untouched] == nq / 0.5).all()
    # the shortcut: pairs known with fewer own samples than the threshold
    assert ((L.known_tsqa != 0) & (L.n_tsqa < 2)).any()
    assert L.solve_info()[0] > 0 and L.solve_info()[2] >= L.solve_info()[1] >= 1
    env.check_errors()


def test_unbind_returns_to_qlearning_steps_on_the_same_tables():
    tab = dataclasses.replace(random_tables(1, FL, 6, 6, 2, 3, 3, False), max_t=20)
    env, L = _walked(tab, 4, K=20, nsamples_te=2, nsamples_re=2)
    q0, v0 = L.q.copy(), L.visits.copy()
    model = QC.model_of(L)
    L.unbind()
    acts = env.fill_actions(11, 0, 20)
    Q = VecQLearning(HostRMEnv(tab, 4), 0.5, 1.0)  # a Q-learner on a twin brought to the same env state and tables
    for name in LC.STATE_COLS:
        getattr(Q.env, name)[...] = getattr(env, name)
    Q.q[...] = q0
    Q.visits[...] = v0
    for t in range(20):
        L.step(acts[t])
        Q.step(acts[t])
    LC.assert_same_bits(L.q, Q.q, "q")
    assert np.array_equal(L.visits, Q.visits) and (L.visits != v0).any()
    now = QC.model_of(L)
    for k in VecQRMax.MODEL:  # the unbound model is not touched
        assert np.array_equal(now[k], model[k]), k
    with pytest.raises(RuntimeError):
        L.solve_info()
    L.bind_model(L.succ_cap, **L.model())
    assert L.solve_info() == (0, 0, 0)
    env.check_errors()


# ---- the shared rules as a stand-alone program under AddressSanitizer + UBSan -----------------------------------------
def test_shared_rules_clean_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler for the sanitizer build")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "qrmax_update_main")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-o", exe, os.path.join(root, "tests", "data", "qrmax_update_main.cpp")], check=True)
    # the sanitizer runtimes are linked statically: nothing is preloaded, and the program is its own process
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    assert "QRMAX_UPDATE_OK" in r.stdout
