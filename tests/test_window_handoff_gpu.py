"""The hand-off between the packets of a packed rmx_step_seq window: packets 0 .. K - 2 end with no release fence
(their record stores are write-through, their statistics updates agent-scope atomics, each wave waits for them), and
the packets that read the record take its pointer from a kernarg-preloaded slot.

Every test runs a window on one engine and the same steps one rmx_step at a time on a twin, and compares every column
and the statistics with torch.equal, as tests/test_window_packed_gpu.py does.  Where it says "both forms", a third
engine created with RMX_SEQ_RELEASE=1 (a release fence on every packet) runs the same windows too."""
import numpy as np
import pytest

import test_window_packed_gpu as W
from rmx import tables as T

FL, OW = T.FROZEN_LAKE, T.OFFICE_WORLD
KNOBS = W.KNOBS + ("RMX_SEQ_RELEASE",)
# 257, 259 and 256 workgroups of 64 lanes: workgroups are dealt round-robin over the 8 XCDs, so a grid that is no
# multiple of 8 moves every block to another XCD from one packet to the next
ROTATING = (64 * 257, 64 * 259, 64 * 256)


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    assert _t.cuda.is_available(), "gpu tests need a ROCm device"
    return _t


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _release_engine(tab, n, monkeypatch):
    """An engine whose packed windows keep the release fence on every packet (read at rmx_create)."""
    monkeypatch.setenv("RMX_SEQ_RELEASE", "1")
    try:
        return W._engine(tab, n)
    finally:
        monkeypatch.delenv("RMX_SEQ_RELEASE")


def _world(which, kind, A):
    return T.compile_scenario(T.baseline_scenario(2)) if which == "cfg2" else W.small_world(kind, A)


def _window(e, acts, K, autoreset, torch, ref, what):
    """acts as one window on e: packed, exactly K packets, equal to the stepwise twin."""
    c0 = e.queue_counters()["packets"]
    e.step_seq(acts, autoreset=autoreset)
    assert W._packed(e), what
    assert e.queue_counters()["packets"] - c0 == K, what
    W._same(ref, e, torch, what)


ROTATE_CASES = [("small", kind, A, tables) for A in (1, 2, 3, 4) for kind in (FL, OW)
                for tables in ("merged", "merged4")] + [("cfg2", FL, 2, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("which,kind,A,tables", ROTATE_CASES,
                         ids=["%s-%s-A%d-%s" % (w, "fl" if k == FL else "ow", A, t) for w, k, A, t in ROTATE_CASES])
def test_grids_that_rotate_placement(which, kind, A, tables, torch, monkeypatch):
    """N = 64 * 257, 64 * 259 and 64 * 256, K in {2, 3, 8, 64}, autoreset 0 and 1, both forms: every window equals the
    stepwise twin, is packed and takes exactly K packets."""
    if tables:
        monkeypatch.setenv("RMX_FAST_TABLES", tables)
    tab = _world(which, kind, A)
    for n in ROTATING:
        a, b = W._engine(tab, n), W._engine(tab, n)
        c = _release_engine(tab, n, monkeypatch)
        if tables:
            assert b.step_info["tables"] == tables
        pre = W._acts(torch, 1, 5, A, n)  # into the middle of episodes
        for e in (a, b, c):
            W._steps(e, pre)
        for autoreset in (True, False):
            for K in (2, 3, 8, 64):
                acts = W._acts(torch, 100 * K + (n & 1023) + int(autoreset), K, A, n)
                W._steps(a, acts, autoreset=autoreset)
                _window(b, acts, K, autoreset, torch, a, (n, K, autoreset, "default"))
                _window(c, acts, K, autoreset, torch, a, (n, K, autoreset, "RMX_SEQ_RELEASE=1"))
        assert torch.equal(a.stats_tensor(), b.stats_tensor()) and torch.equal(a.stats_tensor(), c.stats_tensor())
        for e in (a, b, c):
            e.check_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [FL, OW], ids=["fl", "ow"])
@pytest.mark.parametrize("A", [2, 4])
def test_tails(A, kind, torch, monkeypatch):
    """N in {1, 63, 65, 1000}, K = 7: the preloaded N / block-size arguments with a partial last block, both forms."""
    tab = W.small_world(kind, A)
    for n in (1, 63, 65, 1000):
        a, b = W._engine(tab, n), W._engine(tab, n)
        c = _release_engine(tab, n, monkeypatch)
        pre = W._acts(torch, 2, 9, A, n)
        for e in (a, b, c):
            W._steps(e, pre)
        for autoreset in (True, False, True):
            acts = W._acts(torch, 7 * n + int(autoreset), 7, A, n)
            W._steps(a, acts, autoreset=autoreset)
            _window(b, acts, 7, autoreset, torch, a, (n, autoreset))
            _window(c, acts, 7, autoreset, torch, a, (n, autoreset, "release"))
        assert torch.equal(a.stats_tensor(), b.stats_tensor()) and torch.equal(a.stats_tensor(), c.stats_tensor())


@pytest.mark.gpu
def test_many_short_windows_back_to_back(torch):
    """200 windows of K = 2 per handle at N = 64 * 257, two handles (config 2 and a 4-agent small world) alternating on
    the device's queue: the record buffer is read again window after window, behind packet 0's fences only."""
    n, K = ROTATING[0], 2
    tab2, tab4 = T.compile_scenario(T.baseline_scenario(2)), W.small_world(FL, 4)
    a2, b2, a4, b4 = W._engine(tab2, n), W._engine(tab2, n), W._engine(tab4, n), W._engine(tab4, n)
    acts2, acts4 = W._acts(torch, 21, 40 * K, 2, n), W._acts(torch, 22, 40 * K, 4, n)
    for w in range(200):
        s = K * (w % 40)
        for a, b, acts in ((a2, b2, acts2), (a4, b4, acts4)):
            W._steps(a, acts[s:s + K])
            b.step_seq(acts[s:s + K])
            assert W._packed(b)
            W._same(a, b, torch, w)
    assert torch.equal(a2.stats_tensor(), b2.stats_tensor()) and torch.equal(a4.stats_tensor(), b4.stats_tensor())
    for e in (a2, b2, a4, b4):
        e.check_errors()


@pytest.mark.gpu
def test_long_window_with_fused_report(torch):
    """A 1,100-step window at N = 257 whose last packet carries the fused report: 1,099 hand-offs in a row, the state and
    the report vector equal to the stepwise path ending in rmx_step_report."""
    tab = T.compile_scenario(T.baseline_scenario(2))
    n, K = 257, 1100
    a, b = W._engine(tab, n), W._engine(tab, n)
    acts = np.random.default_rng(5).integers(0, 5, size=(K, tab.n_agents, n), dtype=np.int32)
    acts[:, :, ::3] = 4  # a third of the envs only wait: they run into the truncation
    acts = torch.as_tensor(acts, device="cuda").contiguous()
    ra = torch.zeros(4, dtype=torch.float64, device="cuda")
    rb = torch.zeros(4, dtype=torch.float64, device="cuda")
    W._steps(a, acts, out=ra)
    c0 = b.queue_counters()["packets"]
    b.step_seq(acts, out=rb)
    assert W._packed(b) and b.report_fused and b.queue_counters()["packets"] - c0 == K
    W._same(a, b, torch)
    assert torch.equal(ra, rb), (ra, rb)
    assert float(rb[1]) > 10 * n  # many autoresets inside the window


@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 3])
def test_timing_on(every, torch):
    """rmx_queue_timing(h, 1) and (h, 3) at K = 7: results unchanged, and the packets without a release fence carry
    their stamps like the others (a completion signal needs no release)."""
    K, n = 7, 1000
    tab = T.compile_scenario(T.baseline_scenario(2))
    a, b = W._engine(tab, n), W._engine(tab, n)
    acts = W._acts(torch, 4, K, 2, n)
    W._steps(a, acts)
    b.queue_timing(every)
    try:
        b.step_seq(acts)
        ts = b.queue_times().astype(np.int64)
    finally:
        b.queue_timing(0)
    assert W._packed(b)
    W._same(a, b, torch)
    assert ts[:, 0].tolist() == sorted(set(list(range(0, K - 1, every)) + [K - 1]))
    assert (ts[:, 1] > 0).all() and ((ts[:, 2] - ts[:, 1]) > 0).all() and (ts[1:, 1] >= ts[:-1, 2]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("config", [2, 4])
def test_recording_reuse(config, torch):
    """The same call three times: the second and third record and upload nothing.  Then the same call with another
    action pointer, which records again (the preloaded slots are part of what is recorded): still the stepwise result."""
    tab = T.compile_scenario(T.baseline_scenario(config))
    n, K = 1000, 5
    a, b = W._engine(tab, n), W._engine(tab, n)
    acts = W._acts(torch, 31, 2 * K, tab.n_agents, n)
    b.step_seq(acts[:K])
    c1 = b.queue_counters()
    b.step_seq(acts[:K])
    b.step_seq(acts[:K])
    d = {k: b.queue_counters()[k] - c1[k] for k in c1}
    assert d["recordings"] == 0 and d["uploads"] == 0 and d["windows"] == 2 and d["packets"] == 2 * K
    for _ in range(3):
        W._steps(a, acts[:K])
    W._same(a, b, torch, "reused")
    other = acts[K:].clone()
    c2 = b.queue_counters()
    b.step_seq(other)
    W._steps(a, other)
    assert W._packed(b) and b.queue_counters()["recordings"] - c2["recordings"] == 1
    W._same(a, b, torch, "other pointer")
    assert torch.equal(a.stats_tensor(), b.stats_tensor())


@pytest.mark.gpu
@pytest.mark.parametrize("A", [2, 4])
def test_out_of_range_column_words(A, torch):
    """256, 0x1FF and -1 in pos_x / pos_y / rm_q on both twins, then K = 3 windows: the columns come out as the three
    rmx_step calls leave them, all table bytes.  The record's pointer now travels in the slot that carries pos_x for
    the other kernels: nothing of the columns' contents reaches the record through it."""
    n = 1000
    tab = W.small_world(FL, A)
    words = [256, 0x1FF, -1]
    a, b = W._engine(tab, n), W._engine(tab, n)
    for r, autoreset in enumerate((False, True, True)):
        pre = W._acts(torch, 50 + r, 6, A, n)
        W._steps(a, pre, autoreset=False)
        W._steps(b, pre, autoreset=False)
        lanes_xy = torch.arange(r % 3, n, 3, device="cuda")
        lanes_q = torch.arange((r + 1) % 3, n, 3, device="cuda")
        for e in (a, b):
            W._garbage(torch, e.pos_x, lanes_xy, words)
            W._garbage(torch, e.pos_y, lanes_xy, words[1:] + words[:1])
            W._garbage(torch, e.rm_q, lanes_q, words[2:] + words[:2])
        acts = W._acts(torch, 80 + r, 3, A, n)
        W._steps(a, acts, autoreset=autoreset)
        _window(b, acts, 3, autoreset, torch, a, (r, autoreset))
        for col in (b.pos_x, b.pos_y, b.rm_q):
            assert int(col.min()) >= 0 and int(col.max()) < 256
        for e in (a, b):
            e.reset(seed=r)
    assert torch.equal(a.stats_tensor(), b.stats_tensor())
