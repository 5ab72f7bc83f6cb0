"""Shared pieces of tests/test_learn_eps_cpu.py and tests/test_learn_eps_gpu.py: per-learner epsilon schedules
(include/rmx.h, rmx_learn_eps_bind / rmx_learn_eps_decay; VecQLearning(epsilon_start=...)).  The training runs recorded
from the reference's own QLearning decaying its own epsilon at its env's resets (tests/golden/gen_golden_eps.py) and
their replay step by step and through run, the twin comparisons (run(T) against T act_steps, device against host, a
constant column against the scalar epsilon) and the places where the column must and must not move."""
import dataclasses
import json
import os

import numpy as np

import learn_common as LC
import learn_run_common as RC
import policy_common as PC
from rmx import _capi
from rmx import tables as T
from rmx.learn import VecQLambda, VecQLearning
from test_random_maps_gpu import random_tables

FL, OW = T.FROZEN_LAKE, T.OFFICE_WORLD
# the recorder's cases, written out: a missing file must fail the suite, not shrink it
EXPECTED = ["fl2", "fl2_pow2", "fl2_rs_slip", "ow2_fail"]
FLOOR_CASES = ("fl2", "fl2_rs_slip", "ow2_fail")


def decayed(col, end, decay):
    """learn_done_episode on a whole array: one float64 multiply, then Python's max(end, x)."""
    x = np.asarray(col, np.float64) * np.float64(decay)
    return np.where(x > end, x, np.float64(end))


def column(L):
    return LC.host(L.epsilon).copy()


def set_column(L, values):
    values = np.ascontiguousarray(values, np.float64)
    assert values.shape == (L.env.A, L.env.N)
    if L.host:
        L.epsilon[...] = values
    else:
        L.epsilon.copy_(L.env.torch.from_numpy(values).to(L.env.device))


def done_before_step(env):
    """[N] bool: the envs the next auto-resetting step resets first."""
    return (LC.host(env.flags).view(np.uint32)[0] & _capi.F_ENV_DONE) != 0


# ---- the recorded runs ---------------------------------------------------------------------------------------------
def load(case):
    d = np.load(os.path.join(LC.GOLDEN, f"eps_{case}.npz"))
    return d, T.compile_scenario(json.loads(str(d["scenario"])))


def fixture_learner(d, tab, make_env):
    """The recorder's setup: one reset, the learners built with the recorded schedule, and the decay of that first
    reset through learn_done_episode (env.reset leaves the column alone)."""
    N = d["actions"].shape[2]
    env = make_env(tab, N)
    env.reset(seed=int(d["seed"]))
    lr = float(d["learning_rate"])
    e0, e1, dec = (float(d[k]) for k in ("epsilon_start", "epsilon_end", "epsilon_decay"))
    L = VecQLearning(env, float(d["gamma"]), None if lr == 0.0 else lr, qtable_init=float(d["qtable_init"]),
                     use_qrm=bool(d["use_qrm"]), use_rsh=bool(d["use_rsh"]), trunc_is_terminal=bool(d["trunc_is_terminal"]),
                     policy_seeds=d["policy_seeds"], epsilon_start=e0, epsilon_end=e1, epsilon_decay=dec)
    assert tuple(L.epsilon.shape) == (env.A, N) and (column(L) == e0).all()
    assert (L.epsilon_end, L.epsilon_decay) == (e1, dec)
    L.learn_done_episode()
    LC.assert_same_bits(L.epsilon, decayed(np.full((env.A, N), e0), e1, dec), "the first reset's decay")
    return env, L


def check_snapshot(case, d, env, L, out, k, snap):
    acts = d["actions"].astype(np.int32)
    bad = np.argwhere(LC.host(out[:snap]) != acts[:snap])
    assert bad.size == 0, (case, "actions: first difference at [t, a, e] =", bad[0].tolist())
    LC.assert_same_bits(L.q, d["q"][k], (case, snap, "q"))
    assert np.array_equal(LC.host(L.visits), d["visits"][k].astype(np.float64)), (case, snap)
    LC.assert_same_bits(L.epsilon, d["epsilon"][k], (case, snap, "epsilon"))
    if "env_rng" in d.files:
        for col, key in RC.ENV_KEYS:
            assert np.array_equal(LC.host(getattr(env, col)), d[key][k].astype(np.int32)), (case, snap, col)
        assert np.array_equal(PC.words(env.rng), d["env_rng"][k]), (case, snap, "env rng")


def replay(case, make_env, through_run):
    """The runner's whole loop on the engine, step by step or as one run per snapshot interval: the actions, q, visits
    and every learner's epsilon at the snapshots and every generator at the end equal the reference's as bit patterns;
    on the slip / random-start case the env, its generator and its episode count too."""
    d, tab = load(case)
    n_steps, A, N = d["actions"].shape
    assert (d["resets"] >= 3).all()
    if case in FLOOR_CASES:  # the floor is reached, and resets after it leave it there
        assert (d["floor_reset"] >= 1).all() and (d["resets"] > d["floor_reset"]).all()
        assert (d["epsilon"][2] == float(d["epsilon_end"])).all()
    else:
        assert (d["floor_reset"] == 0).all()
    assert (d["epsilon"][0] > d["epsilon"][2]).all()  # the first snapshot catches the schedule on its way down
    assert ("env_rng" in d.files) == (case == "fl2_rs_slip")
    env, L = fixture_learner(d, tab, make_env)
    out = RC.new_out(L, n_steps)
    snaps = [int(v) for v in d["snap_steps"]]
    assert snaps == sorted(set(snaps)) and snaps[-1] == n_steps
    prev = 0
    for k, snap in enumerate(snaps):
        if through_run:
            L.run(snap - prev, reference_stream=True, actions_out=out[prev:snap])
        else:
            for t in range(prev, snap):
                L.act_step(reference_stream=True, actions_out=out[t])
        prev = snap
        check_snapshot(case, d, env, L, out, k, snap)
    assert np.array_equal(PC.words(L.rng), d["rng_final"]), case
    if env.episode is not None:
        assert np.array_equal(LC.host(env.episode) + 1, d["resets"]), case
    env.check_errors()
    env.close()


# ---- twins ---------------------------------------------------------------------------------------------------------
# the smallest shapes that can still go wrong: one learner; A = 5 (the 8-agent bucket with its a < p.A guard) on one
# full wave and a partial one; a second 256-thread block with one live lane.  max_t = 12: an env resets every 12 steps
# at the latest, so 300 steps see the floor reached and left behind.
WORLDS = {
    "a1_n1": (lambda: random_tables(5, FL, 6, 5, 1, 4, 5, False), 1),
    "a5_n70": (lambda: random_tables(11, FL, 8, 7, 5, 5, 8, False), 70),
    "a2_n257": (lambda: random_tables(7, OW, 9, 8, 2, 5, 6, True), 257),
}
T_RUN, SPLIT = 300, (1, 170, 129)
SCHEDULE = (0.3, 0.85)  # epsilon_end, epsilon_decay; the column starts at per-learner values in [0.2, 1.0]
TWIN_MODES = ["hash_qrm", "numpy_qrm"]
TWIN_CASES = [(w, m) for w in WORLDS for m in TWIN_MODES]
TWIN_IDS = [f"{w}-{m}" for w, m in TWIN_CASES]


def world(name, max_t=12):
    make, N = WORLDS[name]
    return dataclasses.replace(make(), max_t=max_t), N


def make_learner(env_cls, tab, N, mode, schedule=SCHEDULE, start=None, seed=31, **env_kw):
    """RC.make_learner with an epsilon schedule: a fresh handle with the mode's learner and, unless `start` gives one
    value for all, a column of per-learner values, some of them below the floor already."""
    env = env_cls(tab, N, with_qrm=True, with_enc_state=True, **env_kw)
    env.reset(seed=seed)
    kw, _, needs_seeds = RC.MODES[mode]
    kw = dict(kw)
    seeds = RC.seeds_for(tab, N) if needs_seeds else None
    sched = dict(epsilon_start=1.0 if start is None else start, epsilon_end=schedule[0], epsilon_decay=schedule[1])
    if "lambd" in kw:
        L = VecQLambda(env, 0.9, kw.pop("lambd"), kw.pop("learning_rate"), policy_seeds=seeds, **sched)
    else:
        L = VecQLearning(env, 0.9, kw.pop("learning_rate"), policy_seeds=seeds, **kw, **sched)
    if start is None:
        set_column(L, np.random.default_rng(N).uniform(0.2, 1.0, size=(tab.n_agents, N)))
    return L


def advance(L, mode, n, out, runs, start=0, split=None, epsilon=None):
    """n steps from global step `start`, as runs (split as given, or one run) or as single act_steps."""
    kw = RC.call_kw(mode)
    if runs:
        done = 0
        for m in split or (n,):
            L.run(m, epsilon, actions_out=out[done:done + m], **RC.advance_kw(kw, start + done))
            done += m
        assert done == n
    else:
        for k in range(n):
            L.act_step(epsilon, actions_out=out[k], **RC.advance_kw(kw, start + k))


def same_learners(Lx, Ly, what, exact_stats):
    RC.same_learners(Lx, Ly, what, exact_stats)
    LC.assert_same_bits(Lx.epsilon, Ly.epsilon, (what, "epsilon"))


def twin(cls_x, cls_y, tab, N, mode, n=T_RUN, split=SPLIT, x_runs=True, y_runs=False, exact_stats=True):
    """Two fresh handles with the same schedule and column, x advanced by runs and y by single steps (or as asked):
    the same actions at every step and the same everything afterwards, the column included; the schedule did move."""
    Lx, Ly = make_learner(cls_x, tab, N, mode), make_learner(cls_y, tab, N, mode)
    c0 = column(Lx)
    LC.assert_same_bits(c0, column(Ly), "initial column")
    ox, oy = RC.new_out(Lx, n), RC.new_out(Ly, n)
    advance(Lx, mode, n, ox, x_runs, split=split)
    advance(Ly, mode, n, oy, y_runs, split=split)
    got, want = LC.host(ox), LC.host(oy)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (mode, "actions: first difference at [t, a, e] =", bad[0].tolist())
    assert want.min() >= 0 and want.max() <= 3
    same_learners(Lx, Ly, (N, mode), exact_stats)
    c1 = column(Lx)
    end = SCHEDULE[0]
    # a value above the floor comes down to it at the lowest; one that started below it is lifted to it by the max
    assert (c1 >= np.minimum(c0, end)).all() and (c1 <= np.maximum(c0, end)).all()
    assert (c1 != c0).any() and (c1 == end).any(), "no env reset inside the run, or no floor reached"
    if c0.size >= 10:
        assert (c1 < c0).any() and (c1 > c0).any()
    episodes = float(LC.host(Lx.env.stats())[1])
    assert episodes >= N and (LC.host(Lx.visits) > 0).any()
    Lx.env.close()
    Ly.env.close()


def constant_column_case(cls, mode, c=0.25, n=60):
    """A column filled with c under decay 1.0 is the scalar path with epsilon = c, bit for bit, steps and runs."""
    tab, N = world("a5_n70")
    Lx = make_learner(cls, tab, N, mode, schedule=(0.0, 1.0), start=c)
    Ly = RC.make_learner(cls, tab, N, mode)
    assert Ly.epsilon is None
    ox, oy = RC.new_out(Lx, n), RC.new_out(Ly, n)
    half = n // 2
    advance(Lx, mode, half, ox, False)
    advance(Ly, mode, half, oy, False, epsilon=c)
    advance(Lx, mode, n - half, ox[half:], True, start=half)
    advance(Ly, mode, n - half, oy[half:], True, start=half, epsilon=c)
    assert np.array_equal(LC.host(ox), LC.host(oy))
    RC.same_learners(Lx, Ly, ("constant column", mode), exact_stats=True)
    assert (column(Lx) == c).all() and float(LC.host(Lx.env.stats())[1]) > 0
    Lx.env.close()
    Ly.env.close()


def per_learner_case(cls, mode, n=40):
    """Env 0 at epsilon 0.0 and env 1 at 1.0 on one handle: env 0 is env 0 of a handle stepped with the scalar 0.0
    (never explores), env 1 is env 1 of one stepped with the scalar 1.0 (every action is the explore draw: under the
    engine's policy the hashed action of rmx_fill_actions)."""
    tab, _ = world("a5_n70")
    N, A = 2, tab.n_agents
    Lm = make_learner(cls, tab, N, mode, schedule=(0.0, 1.0), start=0.0)
    set_column(Lm, np.repeat(np.array([[0.0, 1.0]]), A, axis=0))
    twins = {0: RC.make_learner(cls, tab, N, mode), 1: RC.make_learner(cls, tab, N, mode)}
    om = RC.new_out(Lm, n)
    advance(Lm, mode, n // 2, om, False)
    advance(Lm, mode, n - n // 2, om[n // 2:], True, start=n // 2)
    got = LC.host(om)
    for e, Lt in twins.items():
        ot = RC.new_out(Lt, n)
        advance(Lt, mode, n, ot, False, epsilon=float(e))
        assert np.array_equal(got[:, :, e], LC.host(ot)[:, :, e]), (mode, "env", e)
        LC.assert_same_bits(LC.host(Lm.q)[:, e], LC.host(Lt.q)[:, e], (mode, "q of env", e))
        assert np.array_equal(LC.host(Lm.visits)[:, e], LC.host(Lt.visits)[:, e])
        if Lm.rng is not None:
            assert np.array_equal(PC.words(Lm.rng)[:, :, e], PC.words(Lt.rng)[:, :, e])
        Lt.env.close()
    kw = RC.call_kw(mode)
    if "seed" in kw:  # the engine's policy: the explore action is the hashed action of that step
        hashed = LC.host(Lm.env.fill_actions(kw["seed"], kw["t_global"], n))
        assert np.array_equal(got[:, :, 1], hashed[:, :, 1])
        assert (got[:, :, 0] != hashed[:, :, 0]).any()
    LC.assert_same_bits(column(Lm), np.repeat(np.array([[0.0, 1.0]]), A, axis=0), "decay 1.0 moves nothing")
    assert float(LC.host(Lm.env.stats())[1]) > 0
    Lm.env.close()


def lifecycle_case(cls):
    """Where the column moves and where it must not (include/rmx.h, "per-learner epsilon schedules")."""
    tab, N = world("a5_n70", max_t=6)
    A = tab.n_agents
    end, dec = SCHEDULE
    L = make_learner(cls, tab, N, "hash_qrm")
    env = L.env
    rng = np.random.default_rng(4)
    to = (lambda a: a) if L.host else (lambda a: env.torch.as_tensor(a, device=env.device))
    seen = {"learn": 0, "best": 0, "noreset": 0}

    def acts(k=None):
        return rng.integers(0, 4, size=(A, N) if k is None else (k, A, N), dtype=np.int32)

    # 1. rmx_learn_step (the caller's actions) decays exactly the envs it auto-resets, all their agents
    for _ in range(16):
        c, done = column(L), done_before_step(env)
        L.step(to(acts()))
        LC.assert_same_bits(L.epsilon, np.where(done[None, :], decayed(c, end, dec), c), "learn step")
        seen["learn"] += int(done.sum())
    # 2. autoreset = False: done envs stay done and nothing decays, with the caller's actions and with the policy
    while not done_before_step(env).any():
        L.step(to(acts()))
    c = column(L)
    L.step(to(acts()), autoreset=False)
    L.act_step(None, 3, 100, autoreset=False)
    seen["noreset"] = int(done_before_step(env).sum())
    LC.assert_same_bits(L.epsilon, c, "autoreset = False")
    # 3. best = True, learn = False: the greedy evaluation episodes go through reset() too
    q0 = LC.host(L.q).copy()
    for k in range(8):
        c, done = column(L), done_before_step(env)
        L.act_step(None, 3, 200 + k, best=True, learn=False)
        LC.assert_same_bits(L.epsilon, np.where(done[None, :], decayed(c, end, dec), c), "best, learn = False")
        seen["best"] += int(done.sum())
    LC.assert_same_bits(L.q, q0, "an evaluation step learns nothing")
    assert seen["learn"] >= N and seen["best"] >= 1 and seen["noreset"] >= 1, seen
    # 4. everything outside learn steps leaves the column alone, auto-resets included
    set_column(L, np.random.default_rng(5).uniform(0.4, 1.0, size=(A, N)))
    c = column(L)
    e0 = float(LC.host(env.stats())[1])
    for _ in range(8):
        env.step(to(acts()))
    env.step_seq(to(acts(8)))
    env.rollout(3, 0, 16)
    assert float(LC.host(env.stats())[1]) > e0  # (those steps did auto-reset)
    mask = np.zeros(N, np.uint8)
    mask[::3] = 1
    env.reset(mask=mask, seed=9)
    env.reset(seed=10)
    env.load_state(env.save_state())
    LC.assert_same_bits(L.epsilon, c, "steps and resets outside the learner")
    # 5. learn_done_episode(mask): the masked envs, all their agents; None: every env
    L.learn_done_episode(mask if L.host else env.torch.as_tensor(mask, device=env.device))
    want = np.where(mask[None, :] != 0, decayed(c, end, dec), c)
    LC.assert_same_bits(L.epsilon, want, "learn_done_episode(mask)")
    L.learn_done_episode(mask.astype(bool))
    want = np.where(mask[None, :] != 0, decayed(want, end, dec), want)
    LC.assert_same_bits(L.epsilon, want, "learn_done_episode(bool mask)")
    L.learn_done_episode()
    LC.assert_same_bits(L.epsilon, decayed(want, end, dec), "learn_done_episode()")
    with __import__("pytest").raises(ValueError, match="mask"):
        L.learn_done_episode(np.zeros(N + 1, np.uint8))
    env.check_errors()
    env.close()


def odd_values_case(cls):
    """Column values are not validated: > 1 always explores, <= 0 and NaN never do; the decay lifts an entry that is
    not above epsilon_end, NaN included, to epsilon_end."""
    tab, _ = world("a5_n70")
    N, A = 4, tab.n_agents
    L = make_learner(cls, tab, N, "hash_qrm", schedule=(0.0, 1.0), start=0.0)
    vals = np.repeat(np.array([[1.5, -0.25, float("nan"), -0.0]]), A, axis=0)
    set_column(L, vals)
    Lz = RC.make_learner(cls, tab, N, "hash_qrm")
    n = 30
    om, oz = RC.new_out(L, n), RC.new_out(Lz, n)
    advance(L, "hash_qrm", n, om, False)
    advance(Lz, "hash_qrm", n, oz, False, epsilon=0.0)
    kw = RC.call_kw("hash_qrm")
    hashed = LC.host(L.env.fill_actions(kw["seed"], kw["t_global"], n))
    got = LC.host(om)
    assert np.array_equal(got[:, :, 0], hashed[:, :, 0])
    assert np.array_equal(got[:, :, 1:], LC.host(oz)[:, :, 1:])
    # every env has reset by now (max_t = 12): the decay lifts what is not above epsilon_end (NaN too) to it
    assert float(LC.host(L.env.stats())[1]) >= N
    LC.assert_same_bits(L.epsilon, np.repeat(np.array([[1.5, 0.0, 0.0, 0.0]]), A, axis=0), "odd values after resets")
    set_column(L, vals)
    L.bind_epsilon(L.epsilon, 0.125, 0.5)
    L.learn_done_episode()
    LC.assert_same_bits(L.epsilon, np.repeat(np.array([[0.75, 0.125, 0.125, 0.125]]), A, axis=0), "decay of odd values")
    L.env.close()
    Lz.env.close()


def rebind_case(cls):
    """unbind_epsilon brings the scalar path back; bind_epsilon takes the caller's own column; rmx_learn_bind drops
    the binding (as it drops the trace lists)."""
    import pytest
    tab, N = world("a5_n70")
    L = make_learner(cls, tab, N, "hash_qrm")
    with pytest.raises(ValueError, match="epsilon must be None"):
        L.act_step(0.1, 3, 0)
    with pytest.raises(ValueError, match="epsilon must be None"):
        L.run(2, 0.1, 3, 0)
    col = L.epsilon
    L.unbind_epsilon()
    assert L.epsilon is None
    with pytest.raises(ValueError, match="epsilon is required"):
        L.act_step(None, 3, 0)
    with pytest.raises(ValueError, match="epsilon is required"):
        L.run(2, seed=3, t_global=0)
    with pytest.raises((RuntimeError, ValueError), match="rmx_learn_eps_bind"):
        L.learn_done_episode()
    c = LC.host(col).copy()
    Ly = RC.make_learner(cls, tab, N, "hash_qrm")
    ox, oy = RC.new_out(L, 30), RC.new_out(Ly, 30)
    advance(L, "hash_qrm", 30, ox, False, epsilon=0.4)
    advance(Ly, "hash_qrm", 30, oy, False, epsilon=0.4)
    assert np.array_equal(LC.host(ox), LC.host(oy))
    RC.same_learners(L, Ly, "unbound", exact_stats=True)
    LC.assert_same_bits(col, c, "an unbound column is not touched")
    assert float(LC.host(L.env.stats())[1]) > 0
    # the caller's own column, a view inside a larger allocation
    if L.host:
        store = np.full(16 + L.env.A * N + 16, 7.0)
    else:
        store = L.env.torch.full((16 + L.env.A * N + 16,), 7.0, dtype=L.env.torch.float64, device=L.env.device)
    own = store[16:16 + L.env.A * N].reshape(L.env.A, N)
    own[...] = 0.9
    L.bind_epsilon(own, 0.1, 0.5)
    assert L.epsilon is own and (L.epsilon_end, L.epsilon_decay) == (0.1, 0.5)
    L.run(40, seed=3, t_global=30)
    w = LC.host(store)
    assert (w[:16] == 7.0).all() and (w[-16:] == 7.0).all()
    assert set(np.unique(LC.host(own)).tolist()) <= {0.9, 0.45, 0.225, 0.1125, 0.1} and (LC.host(own) < 0.9).any()
    for bad in (np.zeros((L.env.A, N), np.float32), np.zeros((L.env.A, N + 1)), np.zeros((N, L.env.A)).T):
        with pytest.raises(ValueError, match="epsilon column"):
            L.bind_epsilon(bad if L.host else _dev_like(L, bad), 0.1, 0.5)
    assert L.epsilon is own  # a refused column leaves the binding as it was
    # rmx_learn_bind drops the binding: the scalar path again, and rmx_learn_eps_decay has nothing to decay
    LC.bind(L, L.q, L.visits, 0.9, 0.3, True, False)
    before = LC.host(own).copy()
    assert L.lib.rmx_learn_eps_decay(L.env._h, None, None) == _capi.RMX_E_STATE
    assert b"rmx_learn_eps_bind" in L.lib.rmx_last_error()
    assert L.lib.rmx_learn_step_policy(L.env._h, 0.5, 1, 3, 70, 1, None, L._stream()) == 0
    L.env.check_errors()
    LC.assert_same_bits(own, before, "a dropped binding")
    L.env.close()
    Ly.env.close()


def _dev_like(L, bad):
    """`bad` (a numpy array of the wrong dtype, size or layout) as a tensor on L's device with the same flaw."""
    t = L.env.torch
    if not bad.flags.c_contiguous:
        return t.zeros(tuple(reversed(bad.shape)), dtype=t.float64, device=L.env.device).T
    return t.as_tensor(bad, device=L.env.device)
