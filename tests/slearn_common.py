"""Shared pieces of tests/test_slearn_cpu.py and tests/test_slearn_gpu.py: the learn step on slip and random-start
worlds (include/rmx.h RMX_LEARN_DYN_ENV).  The training runs recorded from the reference's own QLearning on its own
stochastic environments (tests/golden/gen_golden_slearn.py) and their replay on an engine handle, the random worlds,
and the twin run: a learn step and a plain step with the same actions must leave the same env."""
import dataclasses
import glob
import json
import os

import numpy as np

import learn_common as LC
import policy_common as PC
from rmx import tables as T
from rmx.learn import VecQLearning
from test_random_maps_gpu import SLIP_CASES, random_slip_tables, random_tables

GOLDEN = LC.GOLDEN
FIXTURES = sorted(os.path.basename(p)[len("slearn_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "slearn_*.npz")))
# the recorder's cases: a missing file must fail the suite, not shrink it
EXPECTED = ["fl2_delay_plain", "fl2_randstart_qrm", "fl2_randstart_slip_visits", "fl2_slip_qrm", "ow2_allslip_qrm"]

FL, OW = T.FROZEN_LAKE, T.OFFICE_WORLD
ENV_COLS = ("rng", "episode")


def env_words(env):
    """The env generator column as uint64 [4, N] on the host (a device column is an int64 tensor of the same bits)."""
    return PC.words(env.rng)


def replay_fixture(case, make_env):
    """The runner's whole loop on the engine: the actions of every step, q / visits and the env itself (positions, RM
    indices, timestep, the env generator's four words, the episode count) at the snapshots and every learner generator
    at the end must equal the reference's, the floats as bit patterns."""
    d = np.load(os.path.join(GOLDEN, f"slearn_{case}.npz"))
    tab = T.compile_scenario(json.loads(str(d["scenario"])))
    assert tab.stochastic or tab.random_starts
    acts = d["actions"].astype(np.int32)
    n_steps, A, N = acts.shape
    env = make_env(tab, N)
    env.reset(seed=int(d["seed"]))
    lr, eps = float(d["learning_rate"]), float(d["epsilon"])
    L = VecQLearning(env, float(d["gamma"]), None if lr == 0.0 else lr, qtable_init=float(d["qtable_init"]),
                     use_qrm=bool(d["use_qrm"]), use_rsh=bool(d["use_rsh"]),
                     trunc_is_terminal=bool(d["trunc_is_terminal"]), policy_seeds=d["policy_seeds"])
    assert tuple(L.q.shape) == d["q"].shape[1:] and tuple(L.rng.shape) == (5, A, N)
    if L.host:
        out = np.full((n_steps, A, N), -1, np.int32)
    else:
        out = env.torch.full((n_steps, A, N), -1, dtype=env.torch.int32, device=env.device)
    snaps = [int(v) for v in d["snap_steps"]]
    for t in range(n_steps):
        L.act_step(eps, reference_stream=True, actions_out=out[t])
        if t + 1 in snaps:
            k = snaps.index(t + 1)
            bad = np.argwhere(LC.host(out[:t + 1]) != acts[:t + 1])
            assert bad.size == 0, (case, "actions: first difference at [t, a, e] =", bad[0].tolist())
            LC.assert_same_bits(L.q, d["q"][k], (case, t + 1, "q"))
            assert np.array_equal(LC.host(L.visits), d["visits"][k].astype(np.float64)), (case, t + 1)
            for col, key in (("pos_x", "env_pos_x"), ("pos_y", "env_pos_y"), ("rm_q", "env_q"), ("t", "env_t"),
                             ("episode", "env_episode")):
                assert np.array_equal(LC.host(getattr(env, col)), d[key][k].astype(np.int32)), (case, t + 1, col)
            assert np.array_equal(env_words(env), d["env_rng"][k]), (case, t + 1, "env rng")
    assert np.array_equal(PC.words(L.rng), d["rng_final"]), case
    env.check_errors()
    env.close()
    return d["coverage"]


# ---- random worlds ---------------------------------------------------------------------------------------------------
def slip_world(name, max_t=20):
    return dataclasses.replace(random_slip_tables(*SLIP_CASES[name]), max_t=max_t)


def fl_slip_randstart_world(seed=11, W=8, H=7, A=5, Q=5, n_ev=8, max_t=20):
    """A FrozenLake world with slip and random starts (A = 5: the 8-agent bucket)."""
    return dataclasses.replace(random_tables(seed, FL, W, H, A, Q, n_ev, False, stochastic=True, random_starts=True,
                                             seed_schedule=(1000, 1000, 1)), max_t=max_t)


def caller_actions(rng, tab, N):
    """FrozenLake slip has no wait action (it is reported as invalid); OfficeWorld's wait draws nothing."""
    return rng.integers(0, 5 if tab.kind == OW else 4, size=(tab.n_agents, N), dtype=np.int32)


def env_columns(env):
    """Every bound column of the env, the generator and episode columns included."""
    out = LC.columns(env)
    out["rng"] = env_words(env).copy()
    out["episode"] = LC.host(env.episode).copy()
    return out


def twin_run(make_env, tab, N, K, seed, as_actions=lambda a: a, exact_stats=True, **env_kw):
    """L.step / an evaluation step on one handle, env.step with the same actions on a twin: identical columns after
    every step (state, outputs, rng, episode) and identical statistics; the evaluation steps leave q / visits
    untouched.  Returns what the run reached (liveness)."""
    x, y = make_env(tab, N, **env_kw), make_env(tab, N, **env_kw)
    x.reset(seed=seed)
    y.reset(seed=seed)
    L = VecQLearning(x, 0.9, 0.2, qtable_init=0.5, use_qrm=True)
    A = tab.n_agents
    out = np.zeros((A, N), np.int32) if L.host else x.torch.zeros((A, N), dtype=x.torch.int32, device=x.device)
    rng = np.random.default_rng(seed + 1)
    seen = {"evaluated": 0, "moved_rng": 0}
    for t in range(K):
        before = env_words(x).copy()
        if t % 4 == 3:  # an evaluation step: the engine's policy picks, nothing is learned
            q0, v0 = LC.host(L.q).copy(), LC.host(L.visits).copy()
            L.act_step(0.5, 7, t, learn=False, actions_out=out)
            a = LC.host(out).copy()
            if tab.kind == FL:
                assert a.min() >= 0 and a.max() <= 3
            LC.assert_same_bits(L.q, q0, (t, "q after an evaluation step"))
            assert np.array_equal(LC.host(L.visits), v0), t
            seen["evaluated"] += 1
        else:
            a = caller_actions(rng, tab, N)
            L.step(as_actions(a))
        y.step(as_actions(a))
        LC.assert_same_columns(env_columns(x), env_columns(y), ("twin", t))
        seen["moved_rng"] += int((env_words(x) != before).any())
        sx, sy = LC.host(x.stats()), LC.host(y.stats())
        if exact_stats:
            assert np.array_equal(sx.view(np.uint64), sy.view(np.uint64)), (t, sx, sy)
        else:  # the return sum in each kernel's own association (include/rmx.h): the counts are exact
            assert np.array_equal(sx[1:], sy[1:]) and abs(sx[0] - sy[0]) <= 1e-9 * max(1.0, abs(sy[0])), (t, sx, sy)
    seen["episodes"] = float(LC.host(x.stats())[1])
    seen["max_episode"] = int(LC.host(x.episode).max())
    seen["visited"] = int((LC.host(L.visits) > 0).sum())
    x.check_errors()
    y.check_errors()
    x.close()
    y.close()
    return seen
