"""rmx_learn_model_run (include/rmx.h, "runs of R-max and QR-max learners") on host handles: the entry and its refusals,
run(T) through it against T single act_steps for both learners and every policy with T above the cap of one call,
runs that do not learn, and the recorded reference runs that chose their own actions replayed one run per snapshot
interval."""
import ctypes as C
import dataclasses
import json
import os
import re

import numpy as np
import pytest

import learn_common as LC
import model_run_common as MC
import policy_common as PC
import qrmax_common as QC
import rmax_common as RC
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv
from rmx.learn import VecQLearning, VecQRMax, VecRMax
from test_learn_cpu import _lcfg, _raw
from test_random_maps_gpu import random_tables

FL = T.FROZEN_LAKE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tiny_world():
    return dataclasses.replace(random_tables(1, FL, 6, 6, 2, 3, 3, False), max_t=20)


def test_the_entry_is_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "rmx.h")).read()
    assert re.search(r"#define RMX_LEARN_MODEL_RUN_MAX 256\b", src)
    assert re.search(r"\bint rmx_learn_model_run\(rmx_handle\* h, int32_t T, int flags, uint64_t seed, int64_t t_global,",
                     src)
    assert "rmx_learn_model_run" in _capi.EXPORTS and _capi.LEARN_MODEL_RUN_MAX == 256
    assert hasattr(_capi.load_library(), "rmx_learn_model_run")


def test_refusals():
    tab = T.compile_scenario(T.baseline_scenario(2))
    lib, h, keep = _raw(tab)
    INV, STATE = _capi.RMX_E_INVALID, _capi.RMX_E_STATE
    UPD, MAX = _capi.LEARN_UPDATE, _capi.LEARN_MODEL_RUN_MAX
    p = lambda x: x.ctypes.data  # noqa: E731

    def refused(code, word, *args):
        assert lib.rmx_learn_model_run(*args) == code, lib.rmx_last_error()
        assert word.encode() in lib.rmx_last_error(), lib.rmx_last_error()

    refused(INV, "NULL", None, 3, UPD, 1, 0, None, None)
    for bad in (0, -1, MAX + 1):
        refused(INV, "RMX_LEARN_MODEL_RUN_MAX", h, bad, UPD, 1, 0, None, None)
    refused(INV, "flags", h, 3, 8, 1, 0, None, None)
    # before rmx_bind, before rmx_learn_bind
    lib2, h2, keep2 = _raw(tab, bind=False)
    refused(STATE, "rmx_bind", h2, 3, UPD, 1, 0, None, None)
    refused(STATE, "rmx_learn_bind", h, 3, UPD, 1, 0, None, None)
    # a learner without a model: rmx_learn_run is its entry
    A, N, S = 2, 4, 10 * 10 * 4
    q, v = np.full((A, N, S, 4), 2.0), np.zeros((A, N, S, 4))
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(gamma=0.5)), p(q), p(v)) == 0
    refused(STATE, "rmx_learn_run", h, 3, UPD, 1, 0, None, None)
    assert lib.rmx_learn_run(h, 1, 0.0, UPD, 1, 0, None, None) == 0
    # an R-max model: served; RMX_LEARN_NUMPY needs the column; rmx_learn_run still refuses the handle
    rsum, ri, rc = np.zeros_like(q), np.zeros((A, N, S, 4, 5), np.int32), np.zeros((A, N, S, 4, 5), np.int32)
    assert lib.rmx_learn_rmax_bind(h, 2, 1e-3, 0, 100, 5, p(rsum), p(ri), p(rc)) == 0
    refused(STATE, "rmx_learn_rng_bind", h, 3, UPD | _capi.LEARN_NUMPY, 1, 0, None, None)
    assert lib.rmx_learn_run(h, 3, 0.0, UPD, 1, 0, None, None) == STATE
    assert b"rmx_learn_run" in lib.rmx_last_error() and b"R-max" in lib.rmx_last_error()
    out = np.full((3, A, N), -1, np.int32)
    assert lib.rmx_learn_model_run(h, 3, UPD, 1, 0, p(out), None) == 0, lib.rmx_last_error()
    assert ((out >= 0) & (out < 4)).all() and rc.any()
    # a QR-max model likewise
    assert lib.rmx_learn_rmax_bind(h, 0, 0.0, 0, 0, 0, None, None, None) == 0
    refused(STATE, "rmx_learn_run", h, 3, UPD, 1, 0, None, None)
    P = 100
    sq, sa, s = (A, N, S, 4), (A, N, P, 4), (A, N, S)
    m = dict(known_tsqa=np.zeros(sq, np.uint8), n_tsa=np.zeros(sa, np.int32), n_rsa=np.zeros(sa, np.int32),
             sum_rsa=np.zeros(sa), succ_idx=np.zeros(sa + (5,), np.int32), succ_cnt=np.zeros(sa + (5,), np.int32),
             n_tqs=np.zeros(s, np.int32), tq_next=np.zeros(s, np.int32), n_rqs=np.zeros(s, np.int32),
             sum_rqs=np.zeros(s), final=np.zeros(s, np.uint8))
    v[...] = 0
    assert lib.rmx_learn_qrmax_bind(h, 2, 2, 1, 1, 1e-3, 0, 100, 5, *[p(m[k]) for k in VecQRMax.MODEL]) == 0
    refused(STATE, "rmx_learn_rng_bind", h, 3, UPD | _capi.LEARN_NUMPY, 1, 0, None, None)
    assert lib.rmx_learn_run(h, 3, 0.0, UPD, 1, 0, None, None) == STATE
    assert b"rmx_learn_run" in lib.rmx_last_error() and b"QR-max" in lib.rmx_last_error()
    out[...] = -1
    assert lib.rmx_learn_model_run(h, 3, UPD, 1, 0, p(out), None) == 0, lib.rmx_last_error()
    assert ((out >= 0) & (out < 4)).all() and m["succ_cnt"].any()
    for handle in (h, h2):
        lib.rmx_destroy(handle)


class _Counting:
    """The library with the calls of one entry counted."""

    def __init__(self, lib, name):
        self._lib, self._name, self.calls = lib, name, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name != self._name:
            return f

        def counted(*args):
            self.calls.append(args)
            return f(*args)
        return counted


@pytest.mark.parametrize("policy", ["hash", "hash_best", "numpy"])
@pytest.mark.parametrize("kind", MC.KINDS)
def test_run_equals_single_steps_across_the_cap(kind, policy):
    tab, N = tiny_world(), 3
    T_ = _capi.LEARN_MODEL_RUN_MAX + 3
    kw = dict(best=True) if policy == "hash_best" else {}
    (ex, Lx), (ey, Ly) = (MC.make(HostRMEnv, kind, tab, N, 2, use_qrm=True, numpy_policy=policy == "numpy")
                          for _ in range(2))
    Lx.lib = _Counting(Lx.lib, "rmx_learn_model_run")
    ox, oy = MC.new_out(Lx, T_), MC.new_out(Ly, T_)
    MC.run(Lx, T_, 40, ox, **kw)
    assert [c[1] for c in Lx.lib.calls] == [_capi.LEARN_MODEL_RUN_MAX, 3]  # the split, through the new entry
    per_step = MC.steps(Ly, T_, 40, oy, **kw)
    MC.same(kind, Lx, Ly, (kind, policy), (ox, oy))
    assert sum(per_step) > 0 and Ly.known().any() and (ey.t < T_).all()  # solves happened, episodes wrapped
    # and the Python loop kept for comparison is the same thing
    ez, Lz = MC.make(HostRMEnv, kind, tab, N, 2, use_qrm=True, numpy_policy=policy == "numpy")
    oz = MC.new_out(Lz, T_)
    MC.run(Lz, T_, 40, oz, fused=False, **kw)
    MC.same(kind, Lx, Lz, (kind, policy, "looped"), (ox, oz))
    for e in (ex, ey, ez):
        e.check_errors()


@pytest.mark.parametrize("kind", MC.KINDS)
def test_a_run_that_does_not_learn_leaves_the_model_and_the_solve_count(kind):
    tab = tiny_world()
    env, L = MC.make(HostRMEnv, kind, tab, 4, 2, use_qrm=True)
    MC.run(L, 40)
    assert L.solve_info()[0] > 0 and L.known().any()
    before, solves, t0 = MC.COMMON[kind].model_of(L), L.solve_info(), env.t.copy()
    out = MC.new_out(L, 30)
    MC.run(L, 30, 40, out, learn=False)
    MC.run(L, 5, 70, learn=False, best=True)
    after = MC.COMMON[kind].model_of(L)
    for k in before:
        assert np.array_equal(LC.bits(before[k]) if before[k].dtype.kind == "f" else before[k],
                              LC.bits(after[k]) if after[k].dtype.kind == "f" else after[k]), k
    assert L.solve_info() == solves and ((out >= 0) & (out < 4)).all() and (env.t != t0).any()
    with pytest.raises(RuntimeError, match="rmx_learn_run"):  # the Q-learning entry still refuses the handle
        VecQLearning.run(L, 2, None, 3, 0)
    env.check_errors()


def _intervals(snaps, n_steps):
    edges = [0] + [s for s in snaps if 0 < s <= n_steps]
    if edges[-1] != n_steps:
        edges.append(n_steps)
    return list(zip(edges[:-1], edges[1:]))


def test_the_reference_rmax_run_with_its_own_actions_one_run_per_snapshot_interval():
    """rmax_fl2_numpy_t1 as RC.replay_fixture checks it, with L.run between the snapshots instead of act_steps."""
    case = "fl2_numpy_t1"
    d = np.load(os.path.join(RC.GOLDEN, f"rmax_{case}.npz"))
    cov = json.loads(str(d["coverage"]))
    tab = T.compile_scenario(json.loads(str(d["scenario"])))
    acts = d["actions"].astype(np.int32)
    n_steps, A, N = acts.shape
    env = HostRMEnv(tab, N)
    env.reset(seed=int(d["seed"]))
    gamma, delta = float(d["gamma"]), float(d["vi_delta"])
    L = VecRMax(env, gamma, s_a_threshold=int(d["threshold"]), max_reward=float(d["max_reward"]), vi_delta=delta,
                vi_delta_rel=bool(d["vi_delta_rel"]), use_qrm=bool(d["use_qrm"]),
                trunc_is_terminal=bool(d["trunc_is_terminal"]), policy_seeds=d["policy_seeds"])
    snaps = [int(v) for v in d["snap_steps"]]
    out = np.full((n_steps, A, N), -1, np.int32)
    for lo, hi in _intervals(snaps, n_steps):
        L.run(hi - lo, reference_stream=True, actions_out=out[lo:hi])
        if hi not in snaps:
            continue
        k = snaps.index(hi)
        bad = np.argwhere(out[:hi] != acts[:hi])
        assert bad.size == 0, (case, "actions: first difference at [t, a, e] =", bad[0].tolist())
        assert np.array_equal(L.counts, d["counts"][k].astype(np.float64)), (case, hi, "counts")
        LC.assert_same_bits(L.rsum, d["rsum"][k], (case, hi, "rsum"))
        assert np.array_equal(L.transitions(), RC.dense(d["t_idx"][k], d["t_cnt"][k], L.S_max)), (case, hi, "lists")
        RC.assert_list_invariant(L)
        if k == 2:
            assert L.solve_info()[0] == int(d["solves"][k].sum()), (case, "solves")
        if cov["max_succ"] <= 2:
            LC.assert_same_bits(L.q, d["q"][k], (case, hi, "q"))
        else:
            assert float(np.abs(L.q - d["q"][k]).max()) <= 2 * delta / (1 - gamma), (case, hi)
    assert np.array_equal(PC.words(L.rng), d["rng_final"]), case
    solves, sweeps = L.solve_info()
    assert solves == cov["solves"] and (cov["max_succ"] > 2 or sweeps == cov["max_sweeps"]), (solves, sweeps, cov)
    env.check_errors()
    env.close()


def test_the_reference_qrmax_run_with_its_own_actions_one_run_per_snapshot_interval():
    """qrmax_fl2_numpy_t1 as QC.replay_fixture checks it, with L.run between the snapshots instead of act_steps."""
    case = "fl2_numpy_t1"
    d = np.load(os.path.join(QC.GOLDEN, f"qrmax_{case}.npz"))
    cov = json.loads(str(d["coverage"]))
    tab = T.compile_scenario(json.loads(str(d["scenario"])))
    acts = d["actions"].astype(np.int32)
    n_steps, A, N = acts.shape
    env = HostRMEnv(tab, N)
    env.reset(seed=int(d["seed"]))
    te, re_, tq, rq = (int(v) for v in d["nsamples"])
    L = VecQRMax(env, float(d["gamma"]), nsamples_te=te, nsamples_re=re_, nsamples_tq=tq, nsamples_rq=rq,
                 max_reward=float(d["max_reward"]), vi_delta=float(d["vi_delta"]), vi_delta_rel=bool(d["vi_delta_rel"]),
                 use_qrm=bool(d["use_qrm"]), trunc_is_terminal=bool(d["trunc_is_terminal"]),
                 policy_seeds=d["policy_seeds"])
    snaps = [int(v) for v in d["snap_steps"]]
    out = np.full((n_steps, A, N), -1, np.int32)
    for lo, hi in _intervals(snaps, n_steps):
        L.run(hi - lo, reference_stream=True, actions_out=out[lo:hi])
        if hi not in snaps:
            continue
        k = snaps.index(hi)
        bad = np.argwhere(out[:hi] != acts[:hi])
        assert bad.size == 0, (case, "actions: first difference at [t, a, e] =", bad[0].tolist())
        assert np.array_equal(L.n_tsqa, d["n_tsqa"][k].astype(np.float64)), (case, hi, "n_tsqa")
        for name in QC.INT_TABLES:
            if name == "tq_next":  # (meaningful where (q, s') was observed)
                seen = d["n_tqs"][k] > 0
                assert np.array_equal(L.tq_next[seen], d["tq_next"][k][seen]), (case, hi, name)
                continue
            assert np.array_equal(getattr(L, name), d[name][k]), (case, hi, name)
        for name in QC.FLOAT_TABLES:
            LC.assert_same_bits(getattr(L, name), d[name][k], (case, hi, name))
        K = d["t_cnt"].shape[-1]
        cnt, idx = L.succ_cnt, L.succ_idx
        assert np.array_equal(cnt[..., :K], d["t_cnt"][k]) and not cnt[..., K:].any(), (case, hi, "succ_cnt")
        assert np.array_equal(idx[..., :K][cnt[..., :K] > 0], d["t_idx"][k][d["t_cnt"][k] > 0]), (case, hi, "succ_idx")
        QC.assert_list_invariant(L)
        LC.assert_same_bits(L.q, d["q"][k], (case, hi, "q"))
        if k == 2:
            info = L.solve_info()
            assert info[0] == int(d["solves"][k].sum()) and info[2] == int(d["sweeps"][k].sum()), (case, info)
    assert np.array_equal(PC.words(L.rng), d["rng_final"]), case
    assert L.solve_info() == (cov["solves"], cov["max_sweeps"], cov["total_sweeps"]), (case, L.solve_info(), cov)
    env.check_errors()
    env.close()
