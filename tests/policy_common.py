"""Shared pieces of tests/test_policy_cpu.py and tests/test_policy_gpu.py: the training runs recorded from the
reference's own QLearning choosing its own actions (tests/golden/gen_golden_policy.py), their replay on an engine
handle, and what tests/policyref.py expects of one reference-stream step of a handle."""
import glob
import json
import os

import numpy as np

import learn_common as LC
import policyref as PR
from rmx import _capi
from rmx import tables as T
from rmx.learn import VecQLearning

GOLDEN = LC.GOLDEN
FIXTURES = sorted(os.path.basename(p)[len("policy_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "policy_*.npz")))
# the recorder's cases: a missing file must fail the suite, not shrink it
EXPECTED = ["fl2_eps0", "fl2_eps1", "fl2_qrm", "fl2_visits", "ow2_final"]


def words(x):
    """A generator column as uint64 on the host (a device column is an int64 tensor of the same bits)."""
    x = LC.host(x)
    return np.ascontiguousarray(x).view(np.uint64)


def replay_fixture(case, make_env):
    """The runner's whole loop on the engine: the actions of every step, q / visits at the snapshots and every
    generator at the end must equal the reference's, the floats as bit patterns."""
    d = np.load(os.path.join(GOLDEN, f"policy_{case}.npz"))
    tab = T.compile_scenario(json.loads(str(d["scenario"])))
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
            got = LC.host(out[:t + 1])
            bad = np.argwhere(got != acts[:t + 1])
            assert bad.size == 0, (case, "actions: first difference at [t, a, e] =", bad[0].tolist())
            LC.assert_same_bits(L.q, d["q"][k], (case, t + 1, "q"))
            assert np.array_equal(LC.host(L.visits), d["visits"][k].astype(np.float64)), (case, t + 1)
    assert np.array_equal(words(L.rng), d["rng_final"]), case
    env.check_errors()
    env.close()


def states_to_leave(env, tab, autoreset=True):
    """[A, N]: the table row of the state the next step is about to leave (the start state where it resets first)."""
    x, y, q = (LC.host(getattr(env, n)).astype(np.int64) for n in ("pos_x", "pos_y", "rm_q"))
    if autoreset:
        done = (LC.host(env.flags).view(np.uint32)[0] & _capi.F_ENV_DONE) != 0
        sx = np.asarray(tab.start_xy, np.int64)
        x = np.where(done[None, :], sx[:, 0:1], x)
        y = np.where(done[None, :], sx[:, 1:2], y)
        q = np.where(done[None, :], np.asarray(tab.init_q, np.int64)[:, None], q)
    return (y * tab.width + x) * np.asarray(tab.enc_nq, np.int64)[:, None] + q


def expect_step(L, epsilon, best=False):
    """tests/policyref.py over the handle as it stands: the actions of the next reference-stream step [A, N] and the
    generator column after it [5, A, N]."""
    env, tab = L.env, L.env.tables
    st = states_to_leave(env, tab)
    q, col = LC.host(L.q), words(L.rng)
    acts = np.zeros((env.A, env.N), np.int32)
    after = col.copy()
    for a in range(env.A):
        for e in range(env.N):
            g = PR.Pcg(L.rng_state(a, e))
            assert g.words() == [int(v) for v in col[:, a, e]]
            acts[a, e] = PR.choose(g, epsilon, [float(v) for v in q[a, e, st[a, e]]], best=best)
            after[:, a, e] = g.words()
    return acts, after


def bind_column(L, column):
    """rmx_learn_rng_bind once more on L's handle with the caller's own column (a view of a larger allocation, say)."""
    ptr = column.ctypes.data if L.host else column.data_ptr()
    _capi.check(L.lib.rmx_learn_rng_bind(L.env._h, ptr), "rmx_learn_rng_bind")
    L.rng = column


def seed_column(L, seeds):
    seeds = np.ascontiguousarray(seeds, np.uint64)
    assert seeds.shape == (L.env.A, L.env.N)
    _capi.check(L.lib.rmx_learn_rng_seed(L.env._h, seeds.ctypes.data, L._stream()), "rmx_learn_rng_seed")
