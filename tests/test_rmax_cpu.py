"""The R-max learners in the learn step (include/rmx.h "R-max learners", rmx.learn.VecRMax) on host handles: against
fixtures recorded from the reference's own RMax, every refusal of the bind and of rmx_learn_run, the successor-list
capacity over canaried arrays, steps that leave the model alone, transitions() / known(), and unbind.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import learn_common as LC
import rmax_common as RC
import slearn_common as SC
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv
from rmx.learn import VecQLearning, VecRMax
from test_learn_cpu import _lcfg, _raw
from test_random_maps_gpu import random_tables

FL, OW = T.FROZEN_LAKE, T.OFFICE_WORLD


def test_every_recorded_fixture_is_present():
    assert RC.FIXTURES == RC.EXPECTED


@pytest.mark.parametrize("case", RC.EXPECTED)
def test_fixtures_from_the_reference_rmax(case):
    cov = RC.replay_fixture(case, HostRMEnv, lambda a: a)
    # what the recorder asserted of the reference's run is what this replay went through
    want = {"ow2_t1": ("solves",), "ow3_qrm_t2": ("double_cross",), "fl2_open_t3": ("trunc_terminal", "term_over_counts"),
            "fl2_numpy_t1": ("flat_draws", "argmax_picks"), "fl2_slip_t3": ("solves",), "fl2_rel_t2": ("solves",)}[case]
    assert all(cov[k] >= 1 for k in want), cov
    assert (cov["max_succ"] >= 3) == (case == "fl2_slip_t3")


def test_refusals():
    tab = T.compile_scenario(T.baseline_scenario(2))
    lib, h, keep = _raw(tab)
    INV, STATE = _capi.RMX_E_INVALID, _capi.RMX_E_STATE
    full = C.c_int32()
    assert lib.rmx_learn_rmax_slots(h, C.byref(full)) == 0 and full.value == 5
    assert lib.rmx_learn_rmax_slots(None, C.byref(full)) == INV and lib.rmx_learn_rmax_slots(h, None) == INV
    A, N, S = 2, 4, 10 * 10 * 4
    q = np.full((A, N, S, 4), 2.0)
    v = np.zeros_like(q)
    rsum = np.zeros_like(q)
    idx, cnt = np.zeros((A, N, S, 4, 5), np.int32), np.zeros((A, N, S, 4, 5), np.int32)
    p = lambda x: x.ctypes.data  # noqa: E731

    def refused(word, thr=2, delta=1e-3, rel=0, it=100, cap=5, r=p(rsum), i=p(idx), c=p(cnt), code=INV, handle=h):
        assert lib.rmx_learn_rmax_bind(handle, thr, delta, rel, it, cap, r, i, c) == code, lib.rmx_last_error()
        assert word.encode() in lib.rmx_last_error(), lib.rmx_last_error()

    # before rmx_learn_bind
    refused("rmx_learn_bind", code=STATE)
    assert lib.rmx_learn_rmax_bind(None, 2, 1e-3, 0, 100, 5, p(rsum), p(idx), p(cnt)) == INV
    n, m = C.c_int64(), C.c_int64()
    assert lib.rmx_learn_rmax_info(h, C.byref(n), C.byref(m)) == STATE
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
    for bad in (0, -3):
        refused("threshold", thr=bad)
    for bad in (0.0, -1e-3, float("nan"), float("inf")):
        refused("vi_delta", delta=bad)
    for bad in (0, -1):
        refused("max_iter", it=bad)
    for bad in (0, -1, 6):
        refused("cap", cap=bad)
    refused("NULL", i=None)
    refused("NULL", c=None)
    refused("aligned", r=p(rsum) + 4)
    refused("aligned", i=p(idx) + 2)
    refused("aligned", c=p(cnt) + 1)
    # nothing was bound by the refused calls: the steps are still Q-learning's
    acts = np.zeros((A, N), np.int32)
    assert lib.rmx_learn_step(h, p(acts), 1, None) == 0 and not cnt.any() and not rsum.any()
    assert lib.rmx_learn_rmax_info(h, C.byref(n), C.byref(m)) == STATE
    # a good bind; Q(lambda) lists are refused while it stands, and the other way round; rmx_learn_run is refused
    assert lib.rmx_learn_rmax_bind(h, 2, 1e-3, 0, 100, 5, p(rsum), p(idx), p(cnt)) == 0
    ti, tv, tc = np.zeros((A, 8, N), np.int32), np.zeros((A, 8, N)), np.zeros((A, N), np.int32)
    assert lib.rmx_learn_lambda_bind(h, 0.5, 8, p(ti), p(tv), p(tc)) == STATE and b"R-max" in lib.rmx_last_error()
    assert lib.rmx_learn_run(h, 3, 0.0, _capi.LEARN_UPDATE, 1, 0, None, None) == STATE
    assert b"rmx_learn_run" in lib.rmx_last_error()
    assert lib.rmx_learn_step(h, p(acts), 1, None) == 0 and cnt.any() and (v > 0).any()
    assert lib.rmx_learn_rmax_info(h, C.byref(n), C.byref(m)) == 0 and n.value >= 0
    # a NULL rsum unbinds; then the lists bind, and refuse the model; a later rmx_learn_bind drops either binding
    assert lib.rmx_learn_rmax_bind(h, 0, 0.0, 0, 0, 0, None, None, None) == 0
    assert lib.rmx_learn_run(h, 1, 0.0, _capi.LEARN_UPDATE, 1, 0, None, None) == 0
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(gamma=0.5)), p(q), p(v)) == 0
    assert lib.rmx_learn_lambda_bind(h, 0.5, 8, p(ti), p(tv), p(tc)) == 0
    refused("lambda", code=STATE)
    assert lib.rmx_learn_lambda_bind(h, 0.5, 8, None, None, None) == 0
    assert lib.rmx_learn_rmax_bind(h, 2, 1e-3, 1, 100, 1, p(rsum), p(idx), p(cnt)) == 0
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(gamma=0.5)), p(q), p(v)) == 0
    assert lib.rmx_learn_rmax_info(h, C.byref(n), C.byref(m)) == STATE
    before = cnt.copy()
    assert lib.rmx_learn_step(h, p(acts), 1, None) == 0 and np.array_equal(cnt, before)
    assert lib.rmx_check_errors(h) == 0
    lib.rmx_destroy(h)


def test_python_refusals():
    tab = T.compile_scenario(T.baseline_scenario(2))
    env = HostRMEnv(tab, 3)
    with pytest.raises(ValueError, match="gamma"):
        VecRMax(env, 1.0)
    for kw, word in ((dict(s_a_threshold=0), "threshold"), (dict(vi_delta=0.0), "vi_delta"), (dict(max_iter=0), "max_iter"),
                     (dict(succ_cap=0), "cap"), (dict(succ_cap=6), "cap")):
        with pytest.raises(ValueError, match=word):
            VecRMax(env, 0.9, **kw)
    L = VecRMax(env, 0.9, s_a_threshold=2)
    assert L.counts is L.visits and float(L.q[0, 0, 0, 0]) == 1.0 / (1.0 - 0.9) and L.succ_cap == L.succ_full == 5
    with pytest.raises(ValueError, match="epsilon"):
        L.act_step(0.1, 3, 0)
    with pytest.raises(ValueError, match="epsilon"):
        L.run(2, 0.1, 3, 0)
    with pytest.raises(RuntimeError, match="rmx_learn_run"):
        VecQLearning.run(L, 2, None, 3, 0)


def test_a_full_list_drops_the_entry_and_keeps_the_canaries():
    tab = SC.fl_slip_randstart_world()  # A = 5, slip and random starts, max_t = 20
    RC.cap_overflow(HostRMEnv(tab, 5))


def _walked(tab, N, K=40, **kw):
    env = HostRMEnv(tab, N)
    env.reset(seed=4)
    L = VecRMax(env, 0.5, vi_delta=1e-3, **kw)
    for t in range(K):
        L.act_step(None, 7, t)
    return env, L


def test_best_and_no_learn_steps_leave_the_model_alone():
    tab = dataclasses.replace(random_tables(1, FL, 6, 6, 2, 3, 3, False), max_t=20)
    env, L = _walked(tab, 5, s_a_threshold=2)
    assert L.solve_info()[0] > 0 and L.known().any()
    before = RC.model_of(L)
    solves = L.solve_info()
    out = np.full((2, 5), -1, np.int32)
    for t in range(40, 70):
        L.act_step(None, 7, t, best=(t % 2 == 0), learn=False, actions_out=out)
        assert ((out >= 0) & (out < 4)).all()
    after = RC.model_of(L)
    for k in before:
        assert np.array_equal(LC.bits(before[k]) if before[k].dtype == np.float64 else before[k],
                              LC.bits(after[k]) if after[k].dtype == np.float64 else after[k]), k
    assert L.solve_info() == solves and (env.t > 0).any()
    # best=True is np.argmax of the row whatever the row (a flat one included), whatever the seed: never a draw
    want = L.greedy()
    L.act_step(None, 123, 999, best=True, learn=False, autoreset=False, actions_out=out)
    assert np.array_equal(out, want)
    env.check_errors()


def test_the_epsilon_column_is_left_alone():
    tab = dataclasses.replace(random_tables(1, FL, 6, 6, 2, 3, 3, False), max_t=5)
    env = HostRMEnv(tab, 4)
    env.reset(seed=4)
    L = VecRMax(env, 0.5, s_a_threshold=1, vi_delta=1e-3)
    col = np.full((2, 4), 0.75)
    assert L.lib.rmx_learn_eps_bind(env._h, col.ctypes.data, 0.1, 0.5) == 0
    acts = env.fill_actions(3, 0, 30)
    for t in range(30):  # max_t = 5: auto-resets inside, by both kinds of step
        if t % 2:
            L.step(acts[t])
        else:
            L.act_step(None, 3, t)
    assert (col == 0.75).all() and (env.t < 30).all()


def test_transitions_and_known():
    tab = dataclasses.replace(random_tables(2, OW, 12, 10, 4, 6, 7, True), max_t=20)
    env, L = _walked(tab, 3, s_a_threshold=2, use_qrm=True)
    RC.assert_list_invariant(L)
    tr, known = L.transitions(), L.known()
    assert tr.shape == (4, 3, L.S_max, 4, L.S_max) and known.shape == (4, 3, L.S_max, 4) and known.dtype == bool
    assert np.array_equal(tr.sum(axis=-1), L.counts)  # the full cap drops nothing
    assert np.array_equal(known, L.counts >= 2) and known.any() and not known.all()
    assert (np.count_nonzero(tr, axis=-1) <= 1).all()  # a deterministic world: one successor
    # value iteration wrote the known pairs only: every other entry still holds the optimistic value
    assert (L.q[~known] == 1.0 / (1.0 - 0.5)).all() and (L.q[known] != 2.0).any()
    # with use_qrm the RM state actually held is counted twice: its pair crosses threshold 2 in one step
    assert L.solve_info()[0] > 0
    env.check_errors()


def test_unbind_returns_to_qlearning_steps_on_the_same_tables():
    tab = dataclasses.replace(random_tables(1, FL, 6, 6, 2, 3, 3, False), max_t=20)
    env, L = _walked(tab, 4, K=20, s_a_threshold=2)
    q0, v0 = L.q.copy(), L.visits.copy()
    model = RC.model_of(L)
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
    now = RC.model_of(L)
    for k in ("rsum", "idx", "cnt"):  # the unbound model is not touched
        assert np.array_equal(now[k], model[k]), k
    with pytest.raises(RuntimeError):
        L.solve_info()
    L.bind_model(L.rsum, L.succ_idx, L.succ_cnt, L.succ_cap)
    assert L.solve_info() == (0, 0)
    env.check_errors()
