"""Shared pieces of tests/test_rmax_cpu.py and tests/test_rmax_gpu.py: the R-max fixtures recorded from the reference's
own RMax (tests/golden/gen_golden_rmax.py) and their replay on an engine handle, the device-against-host run, and the
successor-list overflow over canaried arrays."""
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
from rmx.learn import VecRMax

GOLDEN = LC.GOLDEN
FIXTURES = sorted(os.path.basename(p)[len("rmax_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "rmax_*.npz")))
# the recorder's cases: a missing file must fail the suite, not shrink it
EXPECTED = ["fl2_numpy_t1", "fl2_open_t3", "fl2_rel_t2", "fl2_slip_t3", "ow2_t1", "ow3_qrm_t2"]


def dense(idx, cnt, S_max):
    """[A, N, S_max, 4, S_max] from successor lists [A, N, S_max, 4, K] in any slot order (empty slots: cnt == 0)."""
    A, N, S, _, K = cnt.shape
    out = np.zeros((A, N, S, 4, S_max), np.float64)
    a, e, s, k, j = np.nonzero(cnt)
    out[a, e, s, k, idx[a, e, s, k, j]] = cnt[a, e, s, k, j]
    return out


def assert_list_invariant(L):
    """Filled slots come first, hold distinct successors inside the agent's rows, and their counts sum to counts
    (where no entry was dropped)."""
    idx, cnt, counts = LC.host(L.succ_idx), LC.host(L.succ_cnt), LC.host(L.counts)
    assert (cnt >= 0).all()
    filled = cnt > 0
    assert (filled[..., :-1] | ~filled[..., 1:]).all(), "an empty slot before a filled one"
    for a in range(cnt.shape[0]):
        assert (idx[a][filled[a]] >= 0).all() and (idx[a][filled[a]] < L.n_states[a]).all()
        assert not filled[a, :, L.n_states[a]:].any() and not counts[a, :, L.n_states[a]:].any()
    srt = np.sort(np.where(filled, idx, -1 - np.arange(cnt.shape[-1])), axis=-1)
    assert (srt[..., 1:] != srt[..., :-1]).all(), "a successor listed twice"
    if L.succ_cap == L.succ_full:
        assert np.array_equal(cnt.sum(axis=-1), counts)


def replay_fixture(case, make_env, as_actions):
    """Replay a recorded run with R-max learn steps.  counts, rsum, the successor lists and the solve count equal the
    reference's at every snapshot (floats as uint64 bit patterns); q bit for bit where no (s, a) has more than two
    successors, else within 2 * vi_delta / (1 - gamma); where the reference chose the actions, the actions and the
    generators too.  Returns the coverage and the largest |q - reference|."""
    d = np.load(os.path.join(GOLDEN, f"rmax_{case}.npz"))
    cov = json.loads(str(d["coverage"]))
    tab = T.compile_scenario(json.loads(str(d["scenario"])))
    acts = d["actions"].astype(np.int32)
    n_steps, A, N = acts.shape
    env = make_env(tab, N)
    env.reset(seed=int(d["seed"]))
    policy = "policy_seeds" in d.files
    gamma, delta = float(d["gamma"]), float(d["vi_delta"])
    L = VecRMax(env, gamma, s_a_threshold=int(d["threshold"]), max_reward=float(d["max_reward"]), vi_delta=delta,
                vi_delta_rel=bool(d["vi_delta_rel"]), use_qrm=bool(d["use_qrm"]),
                trunc_is_terminal=bool(d["trunc_is_terminal"]), policy_seeds=d["policy_seeds"] if policy else None)
    assert tuple(L.q.shape) == d["q"].shape[1:], (tuple(L.q.shape), d["q"].shape)
    assert [int(v) for v in d["n_states"]] == L.n_states and L.succ_cap == L.succ_full == 5
    assert cov["max_succ"] <= L.succ_full and cov["max_sweeps"] < L.max_iter
    snaps = [int(v) for v in d["snap_steps"]]
    if policy:
        out = np.full((n_steps, A, N), -1, np.int32) if L.host else \
            env.torch.full((n_steps, A, N), -1, dtype=env.torch.int32, device=env.device)
    else:
        dev_acts = as_actions(acts)
    worst = 0.0
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
            assert np.array_equal(LC.host(L.counts), d["counts"][k].astype(np.float64)), (case, t + 1, "counts")
            LC.assert_same_bits(L.rsum, d["rsum"][k], (case, t + 1, "rsum"))
            assert np.array_equal(L.transitions(), dense(d["t_idx"][k], d["t_cnt"][k], L.S_max)), (case, t + 1, "lists")
            assert_list_invariant(L)
            if k == 2:
                assert L.solve_info()[0] == int(d["solves"][k].sum()), (case, "solves")
            if cov["max_succ"] <= 2:
                LC.assert_same_bits(L.q, d["q"][k], (case, t + 1, "q"))
            else:
                diff = float(np.abs(LC.host(L.q) - d["q"][k]).max())
                worst = max(worst, diff)
                print(f"{case} step {t + 1}: largest |q - reference| = {diff:.3e}")
                assert diff <= 2 * delta / (1 - gamma), (case, t + 1, diff)
    if policy:
        assert np.array_equal(PC.words(L.rng), d["rng_final"]), case
    solves, sweeps = L.solve_info()
    assert solves == cov["solves"], (case, solves, cov["solves"])
    if cov["max_succ"] <= 2:
        assert sweeps == cov["max_sweeps"], (case, sweeps, cov["max_sweeps"])
    env.check_errors()
    env.close()
    cov["worst_q_diff"] = worst
    return cov


def model_of(L):
    return dict(q=LC.host(L.q).copy(), counts=LC.host(L.counts).copy(), rsum=LC.host(L.rsum).copy(),
                idx=LC.host(L.succ_idx).copy(), cnt=LC.host(L.succ_cnt).copy())


def assert_same_model(a, b, what):
    """Two learners' q, counts, rsum (bit patterns) and successor lists, slot for slot."""
    ma, mb = model_of(a), model_of(b)
    for key in ("q", "counts", "rsum"):
        LC.assert_same_bits(ma[key], mb[key], (what, key))
    assert np.array_equal(ma["cnt"], mb["cnt"]), (what, "succ_cnt")
    assert np.array_equal(ma["idx"][ma["cnt"] > 0], mb["idx"][mb["cnt"] > 0]), (what, "succ_idx")


def device_equals_host(tab, N, make_dev, make_host, as_actions, policy, threshold, K=20, use_qrm=False, seed=21,
                       caller=None, gamma=0.5, vi_delta=1e-3):
    """K R-max learn steps on a device handle and a host handle: q, counts, rsum, the lists, the actions, the columns
    and the solve count equal bit for bit.  policy: "actions" (the caller's), "hash" (the engine's) or "numpy"."""
    dev, hst = make_dev(tab, N), make_host(tab, N)
    dev.reset(seed=seed)
    hst.reset(seed=seed)
    A = tab.n_agents
    seeds = np.arange(A * N, dtype=np.uint64).reshape(A, N) * 977 + 5 if policy == "numpy" else None
    Ld, Lh = (VecRMax(e, gamma, s_a_threshold=threshold, vi_delta=vi_delta, use_qrm=use_qrm, policy_seeds=seeds)
              for e in (dev, hst))
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
                L.act_step(reference_stream=True, actions_out=o[t])
        per_step.append(Lh.solve_info()[0] - before)
    assert_same_model(Ld, Lh, "model")
    if policy != "actions":
        assert np.array_equal(LC.host(out_d), out_h)
    if policy == "numpy":
        assert np.array_equal(PC.words(Ld.rng), PC.words(Lh.rng))
    assert_list_invariant(Ld)
    LC.assert_same_columns(LC.columns(dev), LC.columns(hst), "columns")
    assert Ld.solve_info() == Lh.solve_info()
    seen = dict(solves=Lh.solve_info()[0], sweeps=Lh.solve_info()[1], per_step=per_step,
                known=int(Lh.known().sum()), wrapped=bool((hst.t < K).all()), rows4=4 * max(Lh.n_states))
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
    """succ_cap = 1 on a slip world over canaried arrays: RMX_E_MODEL, no slot past cap written, the canaries intact,
    counts advanced all the same.  Shared with the GPU file (there the arrays are views of larger tensors)."""
    host = getattr(env, "device", None) == "cpu"
    A, N = env.A, env.N
    env.reset(seed=9)
    L = VecRMax(env, 0.5, s_a_threshold=3, vi_delta=1e-3, succ_cap=1)
    shape = (A, N, L.S_max, 4)
    n = int(np.prod(shape))
    if host:
        raws, views = zip(_canaried(shape, np.float64, -7.0), _canaried(shape + (1,), np.int32, -7),
                          _canaried(shape + (1,), np.int32, -7))
        for v in views:
            v[...] = 0
    else:
        t = env.torch
        raws = [t.full((n + 128,), -7, dtype=dt, device=env.device) for dt in (t.float64, t.int32, t.int32)]
        views = [raws[0][64:64 + n].view(shape), raws[1][64:64 + n].view(shape + (1,)), raws[2][64:64 + n].view(shape + (1,))]
        for v in views:
            v.zero_()
    L.bind_model(views[0], views[1], views[2], 1)
    acts = HostRMEnv(env.tables, N).fill_actions(5, 0, steps) % 4
    for k in range(steps):
        L.step(to_actions(acts[k]))
    with pytest.raises(RuntimeError, match="successor") as ei:
        env.check_errors()
    assert f"rc={_capi.RMX_E_MODEL}" in str(ei.value)
    env.check_errors()  # reported once, then cleared
    for raw in raws:
        r = LC.host(raw)
        assert (r[:64] == -7).all() and (r[-64:] == -7).all()
    counts, cnt = LC.host(L.counts), LC.host(L.succ_cnt)[..., 0]
    assert (cnt <= counts).all() and (cnt < counts).any()  # dropped entries were still counted
    assert counts.max() == 3 and counts.sum() > cnt.sum()
    return L
