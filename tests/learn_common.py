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
EXPECTED = ["fl1_chain200_qrm", "fl1_qrm16_visits", "fl2_back_qrm", "fl2_open_trunc", "fl2_qrm", "fl2_visits", "ow2_plain",
            "ow3_qrm_rsh"]

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


# ---- pieces of the learner's limit tests (tests/test_learn_limits_cpu.py, tests/test_learn_limits_gpu.py) -------------
def assert_same_bits(a, b, what):
    """float64 tables equal as bit patterns."""
    bad = np.argwhere(bits(host(a)) != bits(host(b)))
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


def assert_same_but_nan(a, b, what):
    """NaN at the same positions, every other entry equal as bits (NaN payload and sign are the hardware's)."""
    a, b = host(a), host(b)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), (what, "NaN positions", np.argwhere(na != nb)[:4].tolist())
    bad = np.argwhere((bits(a) != bits(b)) & ~na)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


def bind(L, q, visits, gamma, learning_rate, use_qrm, use_rsh, phi=None):
    """rmx_learn_bind once more on L's handle, with the caller's own tables (numpy on a host handle, torch tensors or
    views of one on a device handle); L then drives them."""
    import ctypes as C

    from rmx import _capi
    cfg = _capi.RmxLearnConfig()
    cfg.gamma = float(gamma)
    cfg.learning_rate = 0.0 if learning_rate is None else float(learning_rate)
    cfg.use_qrm, cfg.use_rsh, cfg.trunc_is_terminal = int(use_qrm), int(use_rsh), int(L.trunc_is_terminal)
    L._phi = np.ascontiguousarray(phi, np.float64) if use_rsh else None
    cfg.phi = None if L._phi is None else L._phi.ctypes.data
    ptr = (lambda x: x.ctypes.data) if L.host else (lambda x: x.data_ptr())
    _capi.check(L.lib.rmx_learn_bind(L.env._h, C.byref(cfg), ptr(q), ptr(visits)), "rmx_learn_bind")
    L.q, L.visits = q, visits


SPECIAL = (0.0, -0.0, 5e-324, -2.2e-308, 1.7e308, float("inf"), 1.0, 1.0 + 2.0 ** -52, 0.1, -0.1)
SPECIAL_NEG = SPECIAL + (-1.7e308, float("-inf"), float("nan"))


def special_fill(shape, values):
    """A table drawn from `values` by np.random.default_rng(1)."""
    v = np.asarray(values, np.float64)
    return v[np.random.default_rng(1).integers(0, len(v), size=shape)]


def uneven_world():
    """A 12 x 10 OfficeWorld whose three agents have 6, 3 and 4 RM states (enc_nq), so that agents 1 and 2 own fewer
    rows than S_max = 720; max_t = 20."""
    from rmx import tables as T
    from test_random_maps_gpu import REWARDS, random_rm
    rng = np.random.default_rng(77)
    W, H = 12, 10
    cells = [(x, y) for y in range(H) for x in range(W)]
    perm = rng.permutation(len(cells))
    hazards = [cells[i] for i in perm[:8]]
    events = [cells[i] for i in perm[8:15]]
    starts = [cells[i] for i in perm[15:18]]
    rms = [random_rm(rng, Q, events, REWARDS) for Q in (6, 3, 4)]
    tab = T.compile_tables(T.OFFICE_WORLD, W, H, hazards, [], starts, rms, [events] * 3, hazard_penalty=-1.5,
                           wall_penalty=-0.25, hazard_fail=True, wall_fail=False, gamma=0.95, shaping_gamma=0.9,
                           reward_modifier=1.5, max_t=20)
    assert [int(v) for v in tab.enc_nq] == [6, 3, 4]
    return tab


# -- one handle, every entry point: a scripted sequence of segments run by two sides ----------------------------------
class EngineSide:
    """An engine handle (device or host) with its learner."""

    def __init__(self, env, L, as_actions=lambda a: a):
        self.env, self.L, self.to = env, L, as_actions
        self.out = None if L.host else env.torch.zeros(4, dtype=env.torch.float64, device=env.device)
        if L.host:
            self.out = np.zeros(4, np.float64)

    def learn(self, acts):
        self.L.step(self.to(acts))

    def plain(self, acts):
        self.env.step(self.to(acts))

    def seq(self, acts):
        self.env.step_seq(self.to(acts))

    def act(self, eps, seed, t, **kw):
        self.L.act_step(eps, seed, t, **kw)

    def report(self, acts):
        return host(self.env.step_report(self.to(acts), out=self.out)).copy()

    def tables(self):
        return host(self.L.q).copy(), host(self.L.visits).copy()

    def save(self):
        L = self.L
        return self.env.save_state(), (L.q.copy(), L.visits.copy()) if L.host else (L.q.clone(), L.visits.clone())

    def load(self, saved):
        blob, (q, v) = saved
        self.env.load_state(blob)
        if self.L.host:
            self.L.q[...], self.L.visits[...] = q, v
        else:
            self.L.q.copy_(q)
            self.L.visits.copy_(v)


class RefSide:
    """tests/learnref.py's restatement over a twin host handle that is only ever stepped with the plain entry points:
    its columns and statistics never pass through a learn step."""

    def __init__(self, twin, R):
        self.env, self.R = twin, R

    def learn(self, acts):
        self.R.step(acts)

    def plain(self, acts):
        self.env.step(acts)

    def seq(self, acts):
        self.env.step_seq(acts)

    def act(self, eps, seed, t, best=False, learn=True):
        self.R.step(self.R.choose(eps, seed, t, best=best), update=learn)

    def report(self, acts):
        return self.env.step_report(acts, out=np.zeros(4, np.float64)).copy()

    def tables(self):
        return self.R.q.copy(), self.R.visits.copy()

    def save(self):
        return self.env.save_state(), (self.R.q.copy(), self.R.visits.copy())

    def load(self, saved):
        blob, (q, v) = saved
        self.env.load_state(blob)
        self.R.q[...], self.R.visits[...] = q, v


MIXED_COLS = STATE_COLS + ("reward", "renv", "env_done", "shaping", "enc_state")


def mixed_use(x, y, A, N, between=lambda seg: None, after_seq=lambda: None):
    """The scripted training loop on both sides; after every segment the state and output columns, q, visits and the
    four statistics must be equal (bit patterns; the integer statistics as numbers).  `between(segment)` runs after
    each comparison, `after_seq()` right after the step_seq window.  Returns what the run reached (liveness)."""
    rng = np.random.default_rng(17)
    seen = {"episodes": 0.0, "segments": 0}

    def acts(k=None):
        return rng.integers(0, 5, size=(A, N) if k is None else (k, A, N), dtype=np.int32)  # 4 = wait

    def same(seg):
        cx = {n: c for n, c in columns(x.env).items() if n in MIXED_COLS}
        cy = {n: c for n, c in columns(y.env).items() if n in MIXED_COLS}
        assert set(STATE_COLS + ("reward", "renv", "env_done", "enc_state")) <= cx.keys()
        assert_same_columns(cx, cy, seg)
        (qx, vx), (qy, vy) = x.tables(), y.tables()
        assert_same_bits(qx, qy, (seg, "q"))
        assert_same_bits(vx, vy, (seg, "visits"))
        sx, sy = host(x.env.stats()), host(y.env.stats())
        assert np.array_equal(sx.view(np.uint64), sy.view(np.uint64)), (seg, sx, sy)
        seen["episodes"] = max(seen["episodes"], float(sx[1]))
        seen["segments"] += 1
        between(seg)

    def both(f):
        return f(x), f(y)

    t = 0
    for _ in range(3):  # 1
        a = acts()
        both(lambda s: s.learn(a))
    same(1)
    for _ in range(2):  # 2
        a = acts()
        both(lambda s: s.plain(a))
    same(2)
    a = acts(5)  # 3
    both(lambda s: s.seq(a))
    after_seq()
    same(3)
    for _ in range(2):  # 4
        both(lambda s: s.act(0.3, 5, t))
        t += 1
    same(4)
    a = acts()  # 5
    rx, ry = both(lambda s: s.report(a))
    assert np.array_equal(rx.view(np.uint64), ry.view(np.uint64)), (5, rx, ry)
    seen["episodes_at_report"] = float(rx[1])
    same(5)
    both(lambda s: s.act(0.0, 5, t, learn=False, best=True))  # 6
    t += 1
    same(6)
    mask = np.zeros(N, np.uint8)  # 7
    mask[::3] = 1
    both(lambda s: s.env.reset(mask=mask, seed=9))
    same(7)
    for _ in range(2):  # 8
        a = acts()
        both(lambda s: s.learn(a))
    same(8)
    saved = both(lambda s: s.save())  # 9
    a3 = acts(3)
    for k in range(3):
        both(lambda s: s.learn(a3[k]))
    same("9 first")
    first = (x.tables(), {n: c for n, c in columns(x.env).items() if n in MIXED_COLS}, host(x.env.stats()).copy())
    x.load(saved[0])
    y.load(saved[1])
    same("9 restored")
    for k in range(3):
        both(lambda s: s.learn(a3[k]))
    same("9 again")
    assert_same_bits(x.tables()[0], first[0][0], "9: q after the restored steps")
    assert_same_bits(x.tables()[1], first[0][1], "9: visits after the restored steps")
    assert_same_columns({n: c for n, c in columns(x.env).items() if n in MIXED_COLS}, first[1], "9: columns")
    assert np.array_equal(host(x.env.stats()).view(np.uint64), first[2].view(np.uint64))
    both(lambda s: s.env.rollout(3, 100, 10))  # 10
    same(10)
    a = acts()  # 11
    both(lambda s: s.learn(a))
    same(11)
    both(lambda s: s.env.clear_stats())  # 12
    same(12)
    assert float(host(x.env.stats())[1]) == 0.0
    for _ in range(2):  # 13
        a = acts()
        both(lambda s: s.learn(a))
    a = acts()
    rx, ry = both(lambda s: s.report(a))
    assert np.array_equal(rx.view(np.uint64), ry.view(np.uint64)), (13, rx, ry)
    same(13)
    seen["episodes_after_clear"] = float(rx[1])
    seen["visited"] = int((x.tables()[1] > 0).sum())
    return seen
