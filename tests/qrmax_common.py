"""Shared pieces of tests/test_qrmax_cpu.py and tests/test_qrmax_gpu.py: the QR-max fixtures recorded from the
reference's own QRMax_v2 (tests/golden/gen_golden_qrmax.py) and their replay on an engine handle, the list invariants,
the device-against-host run, and the successor-list overflow over canaried arrays.  No comparison takes a tolerance:
floats are compared as uint64 bit patterns."""
import glob
import json
import os

import numpy as np
import pytest

import learn_common as LC
import policy_common as PC
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv
from rmx.learn import VecQRMax

GOLDEN = LC.GOLDEN
FIXTURES = sorted(os.path.basename(p)[len("qrmax_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "qrmax_*.npz")))
# the recorder's cases: a missing file must fail the suite, not shrink it
EXPECTED = ["fl2_numpy_t1", "fl2_open_t3", "fl2_rel_t2", "fl2_slip_t3", "fl2_slip_tq2", "ow2_t1", "ow3_qrm_t2"]

INT_TABLES = ("n_tsa", "n_rsa", "n_tqs", "tq_next", "n_rqs", "known_tsqa", "final")
FLOAT_TABLES = ("sum_rsa", "sum_rqs")


def assert_list_invariant(L):
    """Filled slots come first, hold distinct positions, and their counts sum to n_tsa (where no entry was dropped);
    nothing of an agent lies past its own rows."""
    idx, cnt, n_tsa = LC.host(L.succ_idx), LC.host(L.succ_cnt), LC.host(L.n_tsa)
    assert (cnt >= 0).all()
    filled = cnt > 0
    assert (filled[..., :-1] | ~filled[..., 1:]).all(), "an empty slot before a filled one"
    assert (idx[filled] >= 0).all() and (idx[filled] < L.P).all()
    srt = np.sort(np.where(filled, idx, -1 - np.arange(cnt.shape[-1])), axis=-1)
    assert (srt[..., 1:] != srt[..., :-1]).all(), "a successor listed twice"
    if L.succ_cap == L.succ_full:
        assert np.array_equal(cnt.sum(axis=-1), n_tsa)
    assert (n_tsa <= L.nsamples_te).all() and (LC.host(L.n_rsa) <= L.nsamples_re).all()
    assert (LC.host(L.n_tqs) <= L.nsamples_tq).all() and (LC.host(L.n_rqs) <= L.nsamples_rq).all()
    for a in range(cnt.shape[0]):
        S = L.n_states[a]
        for name in ("known_tsqa", "n_tqs", "n_rqs", "final", "n_tsqa"):
            assert not LC.host(getattr(L, name))[a, :, S:].any(), (name, a)


def replay_fixture(case, make_env, as_actions):
    """Replay a recorded run with QR-max learn steps.  Every saved table equals the reference's at every snapshot
    (floats as uint64 bit patterns, Q on the slip cases included), as do the solves, the longest solve's sweeps and
    the sweeps in all; where the reference chose the actions, the actions and the generators too.  Returns the
    coverage."""
    d = np.load(os.path.join(GOLDEN, f"qrmax_{case}.npz"))
    cov = json.loads(str(d["coverage"]))
    tab = T.compile_scenario(json.loads(str(d["scenario"])))
    acts = d["actions"].astype(np.int32)
    n_steps, A, N = acts.shape
    env = make_env(tab, N)
    env.reset(seed=int(d["seed"]))
    policy = "policy_seeds" in d.files
    te, re_, tq, rq = (int(v) for v in d["nsamples"])
    L = VecQRMax(env, float(d["gamma"]), nsamples_te=te, nsamples_re=re_, nsamples_tq=tq, nsamples_rq=rq,
                 max_reward=float(d["max_reward"]), vi_delta=float(d["vi_delta"]), vi_delta_rel=bool(d["vi_delta_rel"]),
                 use_qrm=bool(d["use_qrm"]), trunc_is_terminal=bool(d["trunc_is_terminal"]),
                 policy_seeds=d["policy_seeds"] if policy else None)
    assert tuple(L.q.shape) == d["q"].shape[1:], (tuple(L.q.shape), d["q"].shape)
    assert [int(v) for v in d["n_states"]] == L.n_states and L.succ_cap == L.succ_full == 5
    assert cov["max_succ"] <= L.succ_full and cov["max_sweeps"] < L.max_iter
    snaps = [int(v) for v in d["snap_steps"]]
    if policy:
        out = np.full((n_steps, A, N), -1, np.int32) if L.host else \
            env.torch.full((n_steps, A, N), -1, dtype=env.torch.int32, device=env.device)
    else:
        dev_acts = as_actions(acts)
    for t in range(n_steps):
        if policy:
            L.act_step(reference_stream=True, actions_out=out[t])
        else:
            L.step(dev_acts[t])
        if t + 1 in snaps:
            k = snaps.index(t + 1)
            if policy:
                bad = np.argwhere(LC.host(out[:t + 1]) != acts[:t + 1])
                assert bad.size == 0, (case, "actions: first difference at [t, a, e] =", bad[0].tolist())
            assert np.array_equal(LC.host(L.n_tsqa), d["n_tsqa"][k].astype(np.float64)), (case, t + 1, "n_tsqa")
            for name in INT_TABLES:
                if name == "tq_next":  # (meaningful where (q, s') was observed)
                    seen = d["n_tqs"][k] > 0
                    assert np.array_equal(LC.host(L.tq_next)[seen], d["tq_next"][k][seen]), (case, t + 1, name)
                    continue
                assert np.array_equal(LC.host(getattr(L, name)), d[name][k]), (case, t + 1, name)
            for name in FLOAT_TABLES:
                LC.assert_same_bits(getattr(L, name), d[name][k], (case, t + 1, name))
            # the lists in the reference's own order, slot for slot
            K = d["t_cnt"].shape[-1]
            cnt, idx = LC.host(L.succ_cnt), LC.host(L.succ_idx)
            assert np.array_equal(cnt[..., :K], d["t_cnt"][k]) and not cnt[..., K:].any(), (case, t + 1, "succ_cnt")
            assert np.array_equal(idx[..., :K][cnt[..., :K] > 0], d["t_idx"][k][d["t_cnt"][k] > 0]), (case, t + 1, "succ_idx")
            assert_list_invariant(L)
            LC.assert_same_bits(L.q, d["q"][k], (case, t + 1, "q"))
            if k == 2:
                info = L.solve_info()
                assert info[0] == int(d["solves"][k].sum()) and info[2] == int(d["sweeps"][k].sum()), (case, info)
    if policy:
        assert np.array_equal(PC.words(L.rng), d["rng_final"]), case
    assert L.solve_info() == (cov["solves"], cov["max_sweeps"], cov["total_sweeps"]), (case, L.solve_info(), cov)
    env.check_errors()
    env.close()
    return cov


def model_of(L):
    m = {k: LC.host(v).copy() for k, v in L.model().items()}
    m.update(q=LC.host(L.q).copy(), n_tsqa=LC.host(L.n_tsqa).copy())
    return m


def assert_same_model(a, b, what):
    """Two learners' q, counts and sums (floats as bit patterns), flags and successor lists, slot for slot."""
    ma, mb = model_of(a), model_of(b)
    for key in ("q", "n_tsqa") + FLOAT_TABLES:
        LC.assert_same_bits(ma[key], mb[key], (what, key))
    for key in ("n_tsa", "n_rsa", "n_tqs", "n_rqs", "known_tsqa", "final", "succ_cnt"):
        assert np.array_equal(ma[key], mb[key]), (what, key)
    assert np.array_equal(ma["succ_idx"][ma["succ_cnt"] > 0], mb["succ_idx"][mb["succ_cnt"] > 0]), (what, "succ_idx")
    assert np.array_equal(ma["tq_next"][ma["n_tqs"] > 0], mb["tq_next"][mb["n_tqs"] > 0]), (what, "tq_next")


def device_equals_host(tab, N, make_dev, make_host, as_actions, policy, threshold, K=20, use_qrm=False, seed=21,
                       caller=None, gamma=0.5, vi_delta=1e-3):
    """K QR-max learn steps on a device handle and a host handle: q, the whole model, the actions, the columns and the
    solve statistics equal bit for bit.  policy: "actions" (the caller's), "hash" (the engine's) or "numpy"."""
    dev, hst = make_dev(tab, N), make_host(tab, N)
    dev.reset(seed=seed)
    hst.reset(seed=seed)
    A = tab.n_agents
    seeds = np.arange(A * N, dtype=np.uint64).reshape(A, N) * 977 + 5 if policy == "numpy" else None
    Ld, Lh = (VecQRMax(e, gamma, nsamples_te=threshold, nsamples_re=threshold, vi_delta=vi_delta, use_qrm=use_qrm,
                       policy_seeds=seeds) for e in (dev, hst))
    rng = np.random.default_rng(seed)
    out_d = dev.torch.full((K, A, N), -1, dtype=dev.torch.int32, device=dev.device)
    out_h = np.full((K, A, N), -1, np.int32)
    per_step = []
    for t in range(K):
        before = Lh.solve_info()[0]
        if policy == "actions":
            a = caller(rng) if caller else rng.integers(0, 5, size=(A, N), dtype=np.int32)
            Ld.step(as_actions(a))
            Lh.step(a)
        elif policy == "hash":
            for L, o in ((Ld, out_d), (Lh, out_h)):
                L.act_step(None, 5, t, best=(t % 7 == 6), actions_out=o[t])
        else:
            for L, o in ((Ld, out_d), (Lh, out_h)):
                L.act_step(reference_stream=True, best=(t % 7 == 6), actions_out=o[t])
        per_step.append(Lh.solve_info()[0] - before)
    assert_same_model(Ld, Lh, "model")
    if policy != "actions":
        assert np.array_equal(LC.host(out_d), out_h)
    if policy == "numpy":
        assert np.array_equal(PC.words(Ld.rng), PC.words(Lh.rng))
    assert_list_invariant(Ld)
    LC.assert_same_columns(LC.columns(dev), LC.columns(hst), "columns")
    assert Ld.solve_info() == Lh.solve_info()
    info = Lh.solve_info()
    seen = dict(solves=info[0], sweeps=info[1], total=info[2], per_step=per_step, known=int(Lh.known().sum()),
                wrapped=bool((hst.t < K).all()), rows4=4 * max(Lh.n_states))
    for e in (dev, hst):
        e.check_errors()
        e.close()
    return seen


def _canaried(shape, dtype, fill):
    """An array of `shape` inside a larger allocation, with 64 canary elements either side."""
    n = int(np.prod(shape))
    raw = np.full(n + 128, fill, dtype)
    return raw, raw[64:64 + n].reshape(shape)


def cap_overflow(env, to_actions=lambda a: a, steps=40):
    """succ_cap = 1 on a slip world with every model array canaried: RMX_E_MODEL once, no slot past cap written, the
    canaries intact, n_tsa advanced all the same.  Shared with the GPU file (there the arrays are views of larger
    tensors)."""
    host = getattr(env, "device", None) == "cpu"
    env.reset(seed=9)
    L = VecQRMax(env, 0.5, nsamples_te=3, nsamples_re=3, vi_delta=1e-3, succ_cap=1)
    raws, views = {}, {}
    for name, arr in L.model().items():
        shape = tuple(arr.shape)
        n = int(np.prod(shape))
        if host:
            raws[name], views[name] = _canaried(shape, arr.dtype, 7)
            views[name][...] = 0
        else:
            t = env.torch
            raws[name] = t.full((n + 128,), 7, dtype=arr.dtype, device=env.device)
            views[name] = raws[name][64:64 + n].view(shape)
            views[name].zero_()
    L.bind_model(1, **views)
    acts = HostRMEnv(env.tables, env.N).fill_actions(5, 0, steps) % 4
    for k in range(steps):
        L.step(to_actions(acts[k]))
    with pytest.raises(RuntimeError, match="successor") as ei:
        env.check_errors()
    assert f"rc={_capi.RMX_E_MODEL}" in str(ei.value)
    env.check_errors()  # reported once, then cleared
    for name, raw in raws.items():
        r = LC.host(raw)
        assert (r[:64] == 7).all() and (r[-64:] == 7).all(), name
    n_tsa, cnt = LC.host(L.n_tsa), LC.host(L.succ_cnt)[..., 0]
    assert (cnt <= n_tsa).all() and (cnt < n_tsa).any()  # dropped entries were still counted
    assert n_tsa.max() == 3 and n_tsa.sum() > cnt.sum()
    return L
