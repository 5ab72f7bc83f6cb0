"""Shared pieces of tests/test_lambda_cpu.py and tests/test_lambda_gpu.py: the Q(lambda) fixtures recorded from the
reference's own QLearningLambda (tests/golden/gen_golden_lambda.py) and their replay on an engine handle, the tests'
own dense numpy restatement of the update, and the device-against-host run."""
import glob
import json
import os

import numpy as np

import learn_common as LC
import policy_common as PC
from learnref import LearnRef
from rmx import _capi
from rmx import tables as T
from rmx.learn import VecQLambda

GOLDEN = LC.GOLDEN
FIXTURES = sorted(os.path.basename(p)[len("lambda_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "lambda_*.npz")))
# the recorder's cases: a missing file must fail the suite, not shrink it
EXPECTED = ["fl2_lr", "fl2_open_underflow", "fl2_open_visits", "fl2_policy", "fl2_slip_policy", "ow2_plain"]


def dense_from_lists(idx, val, cnt, S_max):
    """[A, N, S_max, 4] from the recorder's lists [A, N, Lmax] / [A, N]."""
    A, N = cnt.shape
    e = np.zeros((A, N, S_max * 4), np.float64)
    for a, n in np.ndindex(A, N):
        c = int(cnt[a, n])
        e[a, n, idx[a, n, :c]] = val[a, n, :c]
    return e.reshape(A, N, S_max, 4)


def assert_list_invariant(L):
    """Slots 0 .. cnt-1 hold distinct cells, each with a trace that is not 0 (and no NaN)."""
    cnt = L.trace_counts()
    idx, val = LC.host(L.trace_idx), LC.host(L.trace_val)
    assert cnt.min() >= 0 and cnt.max() <= L.trace_cap
    for a, n in np.ndindex(*cnt.shape):
        c = int(cnt[a, n])
        i, v = idx[a, :c, n], val[a, :c, n]
        assert len(set(i.tolist())) == c and (v > 0).all(), (a, n)
        assert (i >= 0).all() and (i < L.n_states[a] * 4).all(), (a, n)


def replay_fixture(case, make_env, as_actions):
    """Replay a recorded run with Q(lambda) learn steps: q, visits and the dense traces equal the reference's as uint64
    bit patterns at every snapshot; where the reference chose the actions, the actions and the generators too."""
    d = np.load(os.path.join(GOLDEN, f"lambda_{case}.npz"))
    tab = T.compile_scenario(json.loads(str(d["scenario"])))
    acts = d["actions"].astype(np.int32)
    n_steps, A, N = acts.shape
    env = make_env(tab, N)
    env.reset(seed=int(d["seed"]))
    lr = float(d["learning_rate"])
    policy = "policy_seeds" in d.files
    L = VecQLambda(env, float(d["gamma"]), float(d["lambd"]), None if lr == 0.0 else lr,
                   trunc_is_terminal=bool(d["trunc_is_terminal"]), policy_seeds=d["policy_seeds"] if policy else None)
    assert tuple(L.q.shape) == d["q"].shape[1:], (tuple(L.q.shape), d["q"].shape)
    assert [int(v) for v in d["n_states"]] == L.n_states and L.trace_cap == 4 * L.S_max
    snaps = [int(v) for v in d["snap_steps"]]
    if policy:
        eps = float(d["epsilon"])
        out = np.full((n_steps, A, N), -1, np.int32) if L.host else \
            env.torch.full((n_steps, A, N), -1, dtype=env.torch.int32, device=env.device)
    else:
        dev_acts = as_actions(acts)
    for t in range(n_steps):
        if policy:
            L.act_step(eps, reference_stream=True, actions_out=out[t])
        else:
            L.step(dev_acts[t])
        if t + 1 in snaps:
            k = snaps.index(t + 1)
            if policy:
                bad = np.argwhere(LC.host(out[:t + 1]) != acts[:t + 1])
                assert bad.size == 0, (case, "actions: first difference at [t, a, e] =", bad[0].tolist())
            LC.assert_same_bits(L.q, d["q"][k], (case, t + 1, "q"))
            assert np.array_equal(LC.host(L.visits), d["visits"][k].astype(np.float64)), (case, t + 1)
            assert np.array_equal(L.trace_counts(), d["e_cnt"][k]), (case, t + 1, "trace counts")
            LC.assert_same_bits(L.traces(), dense_from_lists(d["e_idx"][k], d["e_val"][k], d["e_cnt"][k], L.S_max),
                                (case, t + 1, "traces"))
            assert_list_invariant(L)
            if "env_rng" in d.files:
                for col, key in (("pos_x", "env_pos_x"), ("pos_y", "env_pos_y"), ("rm_q", "env_q"), ("t", "env_t"),
                                 ("episode", "env_episode")):
                    assert np.array_equal(LC.host(getattr(env, col)), d[key][k].astype(np.int32)), (case, t + 1, col)
                assert np.array_equal(PC.words(env.rng), d["env_rng"][k]), (case, t + 1, "env rng")
    if policy:
        assert np.array_equal(PC.words(L.rng), d["rng_final"]), case
    env.check_errors()
    env.close()
    return json.loads(str(d["coverage"]))


# ---- the tests' own restatement: the reference's dense update in numpy, over the columns of a twin host handle --------
class DenseLambda(LearnRef):
    """QLearningLambda.update as the runner drives it (qlearning_lambda.py:33-84 without next_action), dense: one
    e_table per learner, every update sweeps the whole table in numpy, as the reference does.  tests/learnref.py
    supplies the twin host handle stepped with rmx_step and the non-QRM experience read off its columns."""

    def __init__(self, twin, gamma, lambd, learning_rate=None, trunc_is_terminal=None):
        super().__init__(twin, gamma, learning_rate, qtable_init=0.0, trunc_is_terminal=trunc_is_terminal)
        self.lambd = np.float64(lambd)
        self.e = np.zeros_like(self.q)

    def update_q(self, a, e, s, k, r, sn, done):
        if not (0 <= s < self.n_rows(a) and 0 <= sn < self.n_rows(a)):
            return
        q, v, et = self.q[a, e], self.visits[a, e], self.e[a, e]
        gamma = np.float64(self.gamma)
        v[s, k] += 1
        lr = np.float64(self.lr) if self.lr is not None else 1 / v[s, k]
        best = 0.0 if done else float(np.max(q[sn]))
        td = np.float64(r) + gamma * best - q[s, k]
        et[s, k] = 1.0
        with np.errstate(all="ignore"):
            q += lr * td * et
            if done:
                et.fill(0.0)
            else:
                et *= gamma * self.lambd

    def step(self, actions, autoreset=True, update=True):
        if autoreset:  # env.reset() clears the traces of every agent's learner, before the step
            self.e[:, (self.twin.flags[0] & _capi.F_ENV_DONE) != 0] = 0.0
        super().step(actions, autoreset, update)


def device_equals_host(tab, N, make_dev, make_host, as_actions, policy, K=60, lr=None, lambd=0.8, seed=21, cap=None,
                       caller=None):
    """K Q(lambda) learn steps on a device handle and a host handle: q, visits, the counts and traces() equal bit for
    bit.  policy: "actions" (the caller's), "hash" (the engine's) or "numpy" (the reference stream)."""
    dev, hst = make_dev(tab, N), make_host(tab, N)
    dev.reset(seed=seed)
    hst.reset(seed=seed)
    seeds = np.arange(tab.n_agents * N, dtype=np.uint64).reshape(tab.n_agents, N) * 977 + 5 if policy == "numpy" else None
    Ld, Lh = (VecQLambda(e, 0.9, lambd, lr, policy_seeds=seeds, trace_cap=cap) for e in (dev, hst))
    rng = np.random.default_rng(seed)
    longest = 0
    for t in range(K):
        longest = max(longest, int(Lh.trace_counts().max()))
        if policy == "actions":
            a = caller(rng) if caller else rng.integers(0, 5, size=(tab.n_agents, N), dtype=np.int32)
            Ld.step(as_actions(a))
            Lh.step(a)
        elif policy == "hash":
            for L in (Ld, Lh):
                L.act_step(0.3, 5, t, best=(t % 7 == 6))
        else:
            for L in (Ld, Lh):
                L.act_step(0.3, reference_stream=True)
    LC.assert_same_bits(Ld.q, Lh.q, "q")
    assert np.array_equal(LC.host(Ld.visits), Lh.visits)
    assert np.array_equal(Ld.trace_counts(), Lh.trace_counts())
    LC.assert_same_bits(Ld.traces(), Lh.traces(), "traces")
    assert_list_invariant(Ld)
    LC.assert_same_columns(LC.columns(dev), LC.columns(hst), "columns")
    seen = dict(visited=int((Lh.visits > 0).sum()), longest=longest,
                wrapped=bool((hst.t < K).all()))
    for e in (dev, hst):
        e.check_errors()
        e.close()
    return seen
