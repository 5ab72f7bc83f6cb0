"""Shared pieces of tests/test_learn_run_cpu.py and tests/test_learn_run_gpu.py: T learn steps in one call
(VecQLearning.run / rmx_learn_run).  The reference's recorded runs replayed one run per snapshot interval, the twin
comparison (run(T) against T act_steps, device against host), and the worlds and modes both files use."""
import dataclasses
import json
import os

import numpy as np

import lambda_common as MC
import learn_common as LC
import policy_common as PC
import slearn_common as SC
from rmx import tables as T
from rmx.learn import VecQLambda, VecQLearning
from test_random_maps_gpu import random_tables

FL, OW = T.FROZEN_LAKE, T.OFFICE_WORLD

# the recorded runs of the reference in which its learners chose their own actions; written out: a missing file fails
GOLDEN_RUNS = [
    ("policy", "fl2_eps0"), ("policy", "fl2_eps1"), ("policy", "fl2_qrm"), ("policy", "fl2_visits"),
    ("policy", "ow2_final"),
    ("slearn", "fl2_delay_plain"), ("slearn", "fl2_randstart_qrm"), ("slearn", "fl2_randstart_slip_visits"),
    ("slearn", "fl2_slip_qrm"), ("slearn", "ow2_allslip_qrm"),
    ("lambda", "fl2_policy"), ("lambda", "fl2_slip_policy"),
]
GOLDEN_IDS = [f"{k}_{c}" for k, c in GOLDEN_RUNS]

ENV_KEYS = (("pos_x", "env_pos_x"), ("pos_y", "env_pos_y"), ("rm_q", "env_q"), ("t", "env_t"), ("episode", "env_episode"))


def new_out(L, n, fill=-1):
    """An actions_out [n, A, N] for L's env, filled with `fill`."""
    env = L.env
    if L.host:
        return np.full((n, env.A, env.N), fill, np.int32)
    return env.torch.full((n, env.A, env.N), fill, dtype=env.torch.int32, device=env.device)


def replay_run(kind, case, make_env):
    """The runner's whole loop as one run per snapshot interval.  At every snapshot the actions of every step so far,
    q, visits (Q(lambda): the counts and the dense traces) and, where recorded, the env equal the recording as bit
    patterns; at the end every learner's generator too."""
    d = np.load(os.path.join(LC.GOLDEN, f"{kind}_{case}.npz"))
    tab = T.compile_scenario(json.loads(str(d["scenario"])))
    acts = d["actions"].astype(np.int32)
    n_steps, A, N = acts.shape
    assert 2 <= N <= 4 and 200 <= n_steps <= 1100, (N, n_steps)
    env = make_env(tab, N)
    env.reset(seed=int(d["seed"]))
    lr, eps = float(d["learning_rate"]), float(d["epsilon"])
    lr = None if lr == 0.0 else lr
    if kind == "lambda":
        L = VecQLambda(env, float(d["gamma"]), float(d["lambd"]), lr, trunc_is_terminal=bool(d["trunc_is_terminal"]),
                       policy_seeds=d["policy_seeds"])
    else:
        L = VecQLearning(env, float(d["gamma"]), lr, qtable_init=float(d["qtable_init"]), use_qrm=bool(d["use_qrm"]),
                         use_rsh=bool(d["use_rsh"]), trunc_is_terminal=bool(d["trunc_is_terminal"]),
                         policy_seeds=d["policy_seeds"])
    assert tuple(L.q.shape) == d["q"].shape[1:] and tuple(L.rng.shape) == (5, A, N)
    out = new_out(L, n_steps)
    snaps = [int(v) for v in d["snap_steps"]]
    assert snaps == sorted(set(snaps)) and snaps[0] >= 1 and snaps[-1] <= n_steps
    prev = 0
    for k, snap in enumerate(snaps):
        L.run(snap - prev, eps, reference_stream=True, actions_out=out[prev:snap])
        prev = snap
        bad = np.argwhere(LC.host(out[:snap]) != acts[:snap])
        assert bad.size == 0, (case, "actions: first difference at [t, a, e] =", bad[0].tolist())
        LC.assert_same_bits(L.q, d["q"][k], (case, snap, "q"))
        assert np.array_equal(LC.host(L.visits), d["visits"][k].astype(np.float64)), (case, snap)
        if kind == "lambda":
            assert np.array_equal(L.trace_counts(), d["e_cnt"][k]), (case, snap, "trace counts")
            LC.assert_same_bits(L.traces(), MC.dense_from_lists(d["e_idx"][k], d["e_val"][k], d["e_cnt"][k], L.S_max),
                                (case, snap, "traces"))
            MC.assert_list_invariant(L)
        if "env_rng" in d.files:
            for col, key in ENV_KEYS:
                assert np.array_equal(LC.host(getattr(env, col)), d[key][k].astype(np.int32)), (case, snap, col)
            assert np.array_equal(PC.words(env.rng), d["env_rng"][k]), (case, snap, "env rng")
    if prev < n_steps:
        L.run(n_steps - prev, eps, reference_stream=True, actions_out=out[prev:])
        assert np.array_equal(LC.host(out), acts), case
    assert np.array_equal(PC.words(L.rng), d["rng_final"]), case
    env.check_errors()
    env.close()


# ---- run(T) against T act_steps, device against host ----------------------------------------------------------------
# test_policy_gpu.py's three worlds: N = 300 is a full 256-thread block and a partial one whose last wave has a tail,
# A = 5 the 8-agent bucket; max_t = 20 so that truncation and the auto-reset fall inside the run.  The fourth is a
# FrozenLake with slip and random starts (the env's own generator and the episode column).
WORLDS = {
    "a3_n300": (lambda: random_tables(3, FL, 14, 14, 3, 5, 6, False), 300),
    "a5_n70": (lambda: random_tables(11, FL, 8, 7, 5, 5, 8, False), 70),
    "ow_a4_n65": (lambda: random_tables(2, OW, 12, 10, 4, 6, 7, True), 65),
    "fl_slip_randstart": (SC.fl_slip_randstart_world, 65),
}
DET_WORLDS = ["a3_n300", "a5_n70", "ow_a4_n65"]
# mode: (learner keywords, run / act_step keywords, needs policy_seeds)
MODES = {
    "hash_qrm": (dict(learning_rate=0.3, qtable_init=0.25, use_qrm=True), dict(seed=5, t_global=1000), False),
    "numpy_qrm": (dict(learning_rate=0.3, qtable_init=0.25, use_qrm=True), dict(reference_stream=True), True),
    "qrm_visits": (dict(learning_rate=None, qtable_init=0.25, use_qrm=True), dict(seed=9, t_global=3), False),
    "plain_visits": (dict(learning_rate=None, qtable_init=0.5), dict(reference_stream=True), True),
    "best": (dict(learning_rate=0.3, qtable_init=0.25, use_qrm=True), dict(seed=5, t_global=7, best=True), False),
    "eval_numpy": (dict(learning_rate=0.3, qtable_init=0.25, use_qrm=True), dict(reference_stream=True, learn=False),
                   True),
    "lambda": (dict(lambd=0.8, learning_rate=0.2), dict(reference_stream=True), True),
}
CASES = [(w, m) for w in DET_WORLDS for m in sorted(MODES)] + [("fl_slip_randstart", "hash_qrm"),
                                                               ("fl_slip_randstart", "lambda")]
CASE_IDS = [f"{w}-{m}" for w, m in CASES]
EPS, T_RUN, SPLIT = 0.2, 70, (1, 40, 29)


def world(name):
    make, N = WORLDS[name]
    return dataclasses.replace(make(), max_t=20), N


def seeds_for(tab, N):
    return np.random.default_rng(tab.n_agents * N).integers(0, 2 ** 64, size=(tab.n_agents, N), dtype=np.uint64)


def make_learner(env_cls, tab, N, mode, seed=31, **lam_kw):
    """A fresh handle (every output column bound) with the mode's learner; special initial tables so that ties, the
    argmax and the visit counts all matter from the first step."""
    env = env_cls(tab, N, with_qrm=True, with_enc_state=True)
    env.reset(seed=seed)
    kw, _, needs_seeds = MODES[mode]
    kw = dict(kw)
    seeds = seeds_for(tab, N) if needs_seeds else None
    if "lambd" in kw:
        L = VecQLambda(env, 0.9, kw.pop("lambd"), kw.pop("learning_rate"), policy_seeds=seeds, **lam_kw)
    else:
        L = VecQLearning(env, 0.9, kw.pop("learning_rate"), policy_seeds=seeds, **kw)
    return L


def call_kw(mode):
    return dict(MODES[mode][1])


def advance_kw(kw, k):
    """The keywords of the step k global steps later."""
    kw = dict(kw)
    if "t_global" in kw:
        kw["t_global"] += k
    return kw


def run_split(L, mode, split=SPLIT, out=None):
    kw, done = call_kw(mode), 0
    for n in split:
        L.run(n, EPS, actions_out=None if out is None else out[done:done + n], **advance_kw(kw, done))
        done += n
    return done


def run_steps(L, mode, n, out=None, start=0):
    kw = call_kw(mode)
    for k in range(n):
        L.act_step(EPS, actions_out=None if out is None else out[k], **advance_kw(kw, start + k))


def same_stats(x, y, exact):
    """The integer statistics exactly; the return sum exactly, or (a device run against single steps: another order
    of summation) by the rule of rmx_rollout against stepwise, tests/test_limits_gpu.py::_same_stats."""
    sx, sy = LC.host(x.stats()), LC.host(y.stats())
    assert sx[1] == sy[1] and sx[2] == sy[2] and sx[3] == sy[3], (sx, sy)
    if exact:
        assert np.array_equal(sx.view(np.uint64), sy.view(np.uint64)), (sx, sy)
    else:
        np.testing.assert_allclose(sx[0], sy[0], rtol=1e-5, atol=1e-4)


def same_learners(Lx, Ly, what, exact_stats):
    """Everything a run leaves behind, bit for bit; check_errors clean on both."""
    x, y = Lx.env, Ly.env
    LC.assert_same_columns(LC.columns(x), LC.columns(y), what)
    LC.assert_same_bits(Lx.q, Ly.q, (what, "q"))
    LC.assert_same_bits(Lx.visits, Ly.visits, (what, "visits"))
    assert (Lx.rng is None) == (Ly.rng is None)
    if Lx.rng is not None:
        assert np.array_equal(PC.words(Lx.rng), PC.words(Ly.rng)), (what, "learner generators")
    assert (x.rng is None) == (y.rng is None)
    if x.rng is not None:
        assert np.array_equal(PC.words(x.rng), PC.words(y.rng)), (what, "env generator")
        assert np.array_equal(LC.host(x.episode), LC.host(y.episode)), (what, "episode")
    if isinstance(Lx, VecQLambda):
        assert np.array_equal(Lx.trace_counts(), Ly.trace_counts()), (what, "trace counts")
        assert np.array_equal(LC.host(Lx.trace_idx), LC.host(Ly.trace_idx)), (what, "trace_idx")
        LC.assert_same_bits(Lx.trace_val, Ly.trace_val, (what, "trace_val"))
        LC.assert_same_bits(Lx.traces(), Ly.traces(), (what, "traces"))
        MC.assert_list_invariant(Lx)
    same_stats(x, y, exact_stats)
    x.check_errors()
    y.check_errors()


def liveness(L, mode, q0):
    """The run did what its mode is about: resets fell inside it, the tables moved (or, without learn, did not)."""
    env = L.env
    assert (LC.host(env.t) < T_RUN).all() and float(LC.host(env.stats())[1]) > 0
    moved = (LC.bits(LC.host(L.q)) != LC.bits(q0)).any()
    if call_kw(mode).get("learn", True):
        assert moved and (LC.host(L.visits) > 0).any()
    else:
        assert not moved and not (LC.host(L.visits) > 0).any()


def twin_case(cls_x, cls_y, wname, mode, x_runs=True, y_runs=False, exact_stats=True):
    """Two fresh handles of the same world and mode, x stepped by run(1); run(40); run(29) (or by 70 act_steps) and y
    likewise: the same actions of every step and the same everything afterwards."""
    tab, N = world(wname)
    Lx, Ly = make_learner(cls_x, tab, N, mode), make_learner(cls_y, tab, N, mode)
    q0 = LC.host(Lx.q).copy()
    r0 = None if Lx.rng is None else PC.words(Lx.rng).copy()
    ox, oy = new_out(Lx, T_RUN), new_out(Ly, T_RUN)
    for L, o, runs in ((Lx, ox, x_runs), (Ly, oy, y_runs)):
        if runs:
            run_split(L, mode, out=o)
        else:
            run_steps(L, mode, T_RUN, out=o)
    got, want = LC.host(ox), LC.host(oy)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (wname, mode, "actions: first difference at [t, a, e] =", bad[0].tolist())
    assert want.min() >= 0 and want.max() <= 3
    same_learners(Lx, Ly, (wname, mode), exact_stats)
    liveness(Lx, mode, q0)
    if r0 is not None:  # the draws are taken whether or not the step learns
        assert (PC.words(Lx.rng)[:2] != r0[:2]).any()
        assert np.array_equal(PC.words(Lx.rng)[2:4], r0[2:4])  # the increment is never written
    Lx.env.close()
    Ly.env.close()


def mixed_use(cls, mode, exact_stats):
    """run(7), an act_step, a step_seq window (clear_traces after it on a Q(lambda) learner, as documented), a masked
    reset, a get_state / set_state round trip, run(5): equal to the twin that takes single steps."""
    tab, N = world("ow_a4_n65")
    Lx, Ly = make_learner(cls, tab, N, mode), make_learner(cls, tab, N, mode)
    kw = call_kw(mode)
    acts = np.random.default_rng(3).integers(0, 4, size=(25, tab.n_agents, N), dtype=np.int32)
    mask = np.zeros(N, np.uint8)
    mask[::3] = 1
    ox, oy = new_out(Lx, 13), new_out(Ly, 13)
    for L, o, runs in ((Lx, ox, True), (Ly, oy, False)):
        env = L.env
        a = acts if L.host else env.torch.as_tensor(acts, device=env.device)
        if runs:
            L.run(7, EPS, actions_out=o[:7], **kw)
        else:
            run_steps(L, mode, 7, out=o[:7])
        L.act_step(EPS, actions_out=o[7], **advance_kw(kw, 7))
        env.step_seq(a)
        if isinstance(L, VecQLambda):
            L.clear_traces()
        env.reset(mask=mask, seed=9)
        env.load_state(env.save_state())
        if runs:
            L.run(5, EPS, actions_out=o[8:], **advance_kw(kw, 8))
        else:
            run_steps(L, mode, 5, out=o[8:], start=8)
    assert np.array_equal(LC.host(ox), LC.host(oy))
    same_learners(Lx, Ly, ("mixed", mode), exact_stats)
    assert (LC.host(Lx.visits) > 0).any() and float(LC.host(Lx.env.stats())[1]) > 0
    Lx.env.close()
    Ly.env.close()


def overflow_case(cls, exact_stats, rebind=None):
    """A cap below the longest list the run reaches: the same RMX_E_TRACE, tables and lists as the stepwise twin.
    rebind(L, cap): binds the caller's own trace arrays on both twins and returns a check to run at the end."""
    import pytest
    tab, N = world("a3_n300")
    probe = make_learner(cls, tab, N, "lambda")
    longest = 0
    for k in range(30):
        probe.act_step(EPS, **call_kw("lambda"))
        longest = max(longest, int(probe.trace_counts().max()))
    probe.env.close()
    cap = longest - 2
    assert cap >= 2
    Lx, Ly = (make_learner(cls, tab, N, "lambda", trace_cap=cap) for _ in range(2))
    checks = [rebind(L, cap) for L in (Lx, Ly)] if rebind else []
    Lx.run(30, EPS, **call_kw("lambda"))
    run_steps(Ly, "lambda", 30)
    with pytest.raises(RuntimeError) as ex:
        Lx.env.check_errors()
    with pytest.raises(RuntimeError) as ey:
        Ly.env.check_errors()
    assert str(ex.value) == str(ey.value) and "trace" in str(ex.value).lower()
    assert int(Lx.trace_counts().max()) <= cap
    same_learners(Lx, Ly, "overflow", exact_stats)
    for check in checks:
        check()
    Lx.env.close()
    Ly.env.close()
