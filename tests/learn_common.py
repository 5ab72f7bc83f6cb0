"""Shared pieces of tests/test_learn_cpu.py and tests/test_learn_gpu.py: the learner fixtures recorded from the
reference's own QLearning (tests/golden/gen_golden_learn.py) and their replay on an engine handle."""
import glob
import json
import os

import numpy as np

from rmx import tables as T
from rmx.learn import VecQLearning

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[len("learn_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "learn_*.npz")))
# the recorder's cases: a missing file must fail the suite, not shrink it
EXPECTED = ["fl1_qrm16_visits", "fl2_back_qrm", "fl2_open_trunc", "fl2_qrm", "fl2_visits", "ow2_plain", "ow3_qrm_rsh"]

STATE_COLS = ("pos_x", "pos_y", "rm_q", "flags", "ep_ret", "t")
OUT_COLS = ("reward", "renv", "env_done", "shaping", "enc_state", "qrm_s", "qrm_sn", "qrm_rq", "qrm_done")


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def load_fixture(case):
    d = np.load(os.path.join(GOLDEN, f"learn_{case}.npz"))
    tab = T.compile_scenario(json.loads(str(d["scenario"])))
    return d, tab


def replay_fixture(case, make_env, as_actions):
    """Replay the recorded actions with learn steps; q and visits must equal the reference's at every snapshot,
    compared as uint64 bit patterns."""
    d, tab = load_fixture(case)
    acts = d["actions"].astype(np.int32)
    n_steps, A, N = acts.shape
    env = make_env(tab, N)
    env.reset(seed=int(d["seed"]))
    lr = float(d["learning_rate"])
    L = VecQLearning(env, float(d["gamma"]), None if lr == 0.0 else lr, qtable_init=float(d["qtable_init"]),
                     use_qrm=bool(d["use_qrm"]), use_rsh=bool(d["use_rsh"]),
                     trunc_is_terminal=bool(d["trunc_is_terminal"]))
    assert tuple(L.q.shape) == d["q"].shape[1:], (tuple(L.q.shape), d["q"].shape)
    assert [int(v) for v in d["n_states"]] == L.n_states
    dev_acts = as_actions(acts)
    snaps = [int(v) for v in d["snap_steps"]]
    for t in range(n_steps):
        L.step(dev_acts[t])
        if t + 1 in snaps:
            k = snaps.index(t + 1)
            q, v = host(L.q), host(L.visits)
            bad = np.argwhere(bits(q) != bits(d["q"][k]))
            assert bad.size == 0, (case, t + 1, bad[:4].tolist(), q[tuple(bad[0])], d["q"][k][tuple(bad[0])])
            assert np.array_equal(v, d["visits"][k].astype(np.float64)), (case, t + 1)
    env.check_errors()
    env.close()


def columns(env):
    out = {}
    for n in STATE_COLS + OUT_COLS:
        x = getattr(env, n, None)
        if x is not None:
            out[n] = host(x).copy()
    return out


def assert_same_columns(a, b, what):
    assert a.keys() == b.keys()
    for n in a:
        x, y = a[n], b[n]
        if x.dtype.kind == "f":
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), (what, n)
