"""Packed rmx_step_seq windows: the steps of one queue window hand the state to each other in the handle's packed
record (csrc/rmx_layout.h) instead of the caller's columns, and only the last step writes the per-step outputs.

The contract is rmx_step_seq's: after the call the caller's buffers hold exactly what the K rmx_step calls (the last
one rmx_step_report with `out`) would have left.  Every test here runs a window on one engine and the same steps one
by one on a twin from the same state, and compares every column bit for bit; `rmx_seq_packed` says whether the window
really took the packed form, so none of them passes on the unpacked window by accident.

The host check of the record's pack / unpack helpers needs no GPU (it compiles a plain C++ program against
rmx_layout.h)."""
import shutil
import subprocess

import numpy as np
import pytest

import test_limits_gpu as L
from rmx import _capi
from rmx import tables as T

COLS = ("pos_x", "pos_y", "rm_q", "flags", "t", "ep_ret", "reward", "env_done", "renv", "shaping", "enc_state", "rng",
        "episode")
KNOBS = ("RMX_FAST", "RMX_FAST_TABLES", "RMX_FAST_STATS", "RMX_FAST_SKIP", "RMX_GENERIC_SKIP", "RMX_LAYOUT",
         "RMX_QUEUE", "RMX_SEQ_PACKED", "RMX_BLOCK")
FL, OW = T.FROZEN_LAKE, T.OFFICE_WORLD


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    assert _t.cuda.is_available(), "gpu tests need a ROCm device"
    return _t


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _engine(tab, n, **kw):
    from rmx.engine import VecRMEnv
    return VecRMEnv(tab, n, with_enc_state=True, **kw)


def _same(a, b, torch, what=""):
    for k in COLS:
        x, y = getattr(a, k, None), getattr(b, k, None)
        if x is not None:
            assert torch.equal(x, y), (k, what)


def _packed(env):
    return bool(env.lib.rmx_seq_packed(env._h))


def _steps(env, acts, autoreset=True, out=None):
    """acts[0..K) one rmx_step at a time, the last one rmx_step_report with `out`."""
    K = acts.shape[0]
    for s in range(K):
        if out is not None and s == K - 1:
            env.step_report(acts[s], autoreset=autoreset, out=out)
        else:
            env.step(acts[s], autoreset=autoreset)


def _acts(torch, seed, K, A, n):
    a = np.random.default_rng(seed).integers(0, 5, size=(K, A, n), dtype=np.int32)
    return torch.as_tensor(a, device="cuda").contiguous()


# Small worlds of both kinds with 1..4 agents: short episodes (max_t 12, a third of the RM transitions final), so a
# 7-step window crosses terminations, truncations and autoresets; integer rewards, so both record sizes apply.
def small_world(kind, A):
    return L.compile_world(L.make_world(seed=60 + 4 * kind + A, kind=kind, W=6, H=5, A=A, Q=5, n_ev=6,
                                        zone=(0, 0, 5, 4), rewards=(1.0, 3.0, -2.0), max_t=12, final_p=0.3,
                                        hazard_fail=True, wall_fail=(A % 2 == 0)))


@pytest.mark.gpu
@pytest.mark.parametrize("tables", ["merged", "merged4"])
@pytest.mark.parametrize("kind", [FL, OW], ids=["fl", "ow"])
@pytest.mark.parametrize("A", [1, 2, 3, 4])
def test_window_equals_steps_bit_for_bit(A, kind, tables, torch, monkeypatch):
    """K in {1, 2, 3, 4, 7} from one state, N in {1, 255, 257, 1000} (tail lanes, a partial last block), autoreset 0
    and 1: every column equals the K rmx_step calls'.  K = 1 is today's kernel, K >= 2 a packed window."""
    monkeypatch.setenv("RMX_FAST_TABLES", tables)
    tab = small_world(kind, A)
    for n in (1, 255, 257, 1000):
        a, b = _engine(tab, n), _engine(tab, n)
        assert b.step_info["variant"] == "fast" and b.step_info["tables"] == tables
        pre = _acts(torch, 1, 9, A, n)  # into the middle of episodes, some envs done
        _steps(a, pre)
        _steps(b, pre)
        c0 = b.queue_counters()
        packets = 0
        for autoreset in (True, False, True):
            for K in (1, 2, 3, 4, 7):
                acts = _acts(torch, 100 * K + n, K, A, n)
                _steps(a, acts, autoreset=autoreset)
                b.step_seq(acts, autoreset=autoreset)
                assert _packed(b) == (K >= 2), (n, K)
                _same(a, b, torch, (n, K, autoreset))
                packets += K
        assert b.queue_counters()["packets"] - c0["packets"] == packets  # one packet per step
        assert torch.equal(a.stats_tensor(), b.stats_tensor())
        a.check_errors()
        b.check_errors()


@pytest.mark.gpu
def test_long_window_with_report(torch):
    """N = 257, K = 1,100 on FrozenLake (BASELINE config 2): a third of the envs only wait, so they run into the
    truncation at t = 1,001, the others finish and autoreset many times.  State bit-equal to the stepwise path ending
    in rmx_step_report, the report vectors equal."""
    tab = T.compile_scenario(T.baseline_scenario(2))
    n, K = 257, 1100
    assert tab.max_t == 1000
    a, b = _engine(tab, n), _engine(tab, n)
    acts = np.random.default_rng(3).integers(0, 5, size=(K, tab.n_agents, n), dtype=np.int32)
    acts[:, :, ::3] = 4  # wait
    acts = torch.as_tensor(acts, device="cuda").contiguous()
    ra = torch.zeros(4, dtype=torch.float64, device="cuda")
    rb = torch.zeros(4, dtype=torch.float64, device="cuda")
    trunc_seen = False
    for s in range(K):
        if s == K - 1:
            a.step_report(acts[s], out=ra)
        else:
            a.step(acts[s])
        if s == 1000:
            trunc_seen = bool(((a.flags & _capi.F_TRUNC) != 0).any()) and int(a.t.max()) == 1001
    assert trunc_seen
    b.step_seq(acts, out=rb)
    assert _packed(b)
    _same(a, b, torch)
    assert torch.equal(ra, rb), (ra, rb)
    assert float(rb[1]) > 10 * n  # many episodes (autoresets) inside the window


# Field extremes: the 255-wide and 255-high limit worlds of tests/test_limits_gpu.py (x, y up to 254) and a 255-state
# machine, the most the tables hold (next_q is a byte and 255 means "no final state"), so rm_q goes up to 254: the q250
# limit world's generator with Q = 255.  (world, table mode that runs it packed, column, value that must be reached)
def _q255_world():
    return L.compile_world(L.make_world(seed=21, kind=FL, W=4, H=2, A=1, Q=255, n_ev=2, zone=(0, 0, 3, 1),
                                        rewards=L.NEG, q_high=True, hazard_div=0, detect_all=True))


WIDTH_CASES = {
    "w255_h2_fast": (lambda: L.limit_world("w255_h2_fast")[1], "merged4", "pos_x", 254),
    "w2_h255_fast": (lambda: L.limit_world("w2_h255_fast")[1], "merged4", "pos_y", 254),
    "q255_a1": (_q255_world, "merged", "rm_q", 254),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(WIDTH_CASES))
def test_field_widths_through_windows(case, torch, monkeypatch):
    """x = 254, y = 254 and RM state 254 travel through the record's byte fields: 147 steps in windows of 7 equal the
    stepwise path, and the extreme value is really reached (the maximum over every step of the stepwise twin, which the
    window twin equals at every window's end)."""
    world, tables, col, top = WIDTH_CASES[case]
    monkeypatch.setenv("RMX_FAST_TABLES", tables)
    tab = world()
    n = 1500
    acts = np.random.default_rng(121).integers(0, 5, size=(147, tab.n_agents, n), dtype=np.int32)
    acts = torch.as_tensor(acts, device="cuda").contiguous()
    a, b = _engine(tab, n), _engine(tab, n)
    assert b.step_info["tables"] == tables
    hi = torch.zeros((), dtype=torch.int32, device="cuda")
    for w in range(147 // 7):
        for s in range(7 * w, 7 * w + 7):
            a.step(acts[s])
            hi = torch.maximum(hi, getattr(a, col).max())
        b.step_seq(acts[7 * w:7 * w + 7])
        assert _packed(b)
        _same(a, b, torch, w)
    assert int(hi) == top


def _garbage(torch, col, lanes, words):
    """words[i % len] written over col[:, lanes[i]] (int32 bit patterns)."""
    w = torch.as_tensor(np.array(words, dtype=np.int64).astype(np.uint32).view(np.int32), device="cuda")
    col[:, lanes] = w[torch.arange(lanes.numel(), device="cuda") % w.numel()].to(col.dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [FL, OW], ids=["fl", "ow"])
@pytest.mark.parametrize("tables", ["merged", "merged4"])
def test_out_of_range_column_words_never_reach_the_record(tables, kind, torch, monkeypatch):
    """The caller owns the columns and may write anything there.  Words outside 0..255 in pos_x, pos_y and rm_q (256,
    0x1FF, -1, 0x01000003, ...) written on both twins, on lanes that include inactive agents and agents at their final
    RM state: windows of K in {2, 3, 7} leave every column as the K rmx_step calls do, with and without autoreset.
    The record's byte fields rely on the merged step replacing x, y and rm_q of EVERY agent by table bytes; a step that
    let a frozen agent keep its column word would fail here, in windows only.  (Out-of-range words index the tables
    through masked fields and a bounded buffer descriptor: no access leaves the table.)"""
    monkeypatch.setenv("RMX_FAST_TABLES", tables)
    A, n = 2, 1000
    tab = small_world(kind, A)
    words = [256, 0x1FF, -1, 0x01000003, 0x7FFFFFFF, 0x100, 65536 + 2, -256]
    a, b = _engine(tab, n), _engine(tab, n)
    final_q = torch.as_tensor(np.asarray(tab.final_q, np.int32), device="cuda").view(A, 1)
    seen_inactive = seen_final = False
    seed = 0
    for autoreset in (False, True):
        for K in (2, 3, 7):
            seed += 1
            pre = _acts(torch, 40 + seed, 6, A, n)  # without autoreset: inactive agents and final RM states stay
            _steps(a, pre, autoreset=False)
            _steps(b, pre, autoreset=False)
            _same(a, b, torch, "pre")
            inactive = (a.flags & _capi.F_ACTIVE) == 0
            at_final = a.rm_q == final_q
            lanes_xy = torch.arange(seed % 3, n, 3, device="cuda")      # x and y garbage: a third of the envs
            lanes_q = torch.arange((seed + 1) % 3, n, 3, device="cuda")  # rm_q garbage: another third
            seen_inactive |= bool(inactive[:, lanes_xy].any()) and bool(inactive[:, lanes_q].any())
            seen_final |= bool(at_final[:, lanes_xy].any())  # (their rm_q is kept: still final when the window starts)
            for e in (a, b):
                _garbage(torch, e.pos_x, lanes_xy, words)
                _garbage(torch, e.pos_y, lanes_xy, words[3:] + words[:3])
                _garbage(torch, e.rm_q, lanes_q, words[5:] + words[:5])
            acts = _acts(torch, 70 + seed, K, A, n)
            _steps(a, acts, autoreset=autoreset)
            b.step_seq(acts, autoreset=autoreset)
            assert _packed(b)
            _same(a, b, torch, (K, autoreset))
            for col in (b.pos_x, b.pos_y, b.rm_q):  # what today's step leaves: table bytes
                assert int(col.min()) >= 0 and int(col.max()) < 256
            for e in (a, b):
                e.reset(seed=seed)
    assert seen_inactive and seen_final
    assert torch.equal(a.stats_tensor(), b.stats_tensor())


@pytest.mark.gpu
def test_t_and_agent_steps_keep_all_their_bits(torch):
    """`t` and agent_steps (the flags word's top half) beyond 255: an OfficeWorld without failures at the largest max_t
    (60,000), 300 steps from the reset in windows of 60.  Then `t` beyond 65,535, which only a caller's own write to
    the column can produce: t = 65,530 everywhere and three windows without autoreset across 2^16."""
    w = L.make_world(seed=71, kind=OW, W=6, H=5, A=2, Q=5, n_ev=6, zone=(0, 0, 5, 4), rewards=(1.0, 3.0, -2.0),
                     max_t=60000, final_p=0.0, hazard_fail=False, wall_fail=False, none_p=0.0)
    tab = L.compile_world(w)
    n = 257
    a, b = _engine(tab, n), _engine(tab, n)
    acts = _acts(torch, 5, 300, tab.n_agents, n)
    for k in range(5):
        _steps(a, acts[60 * k:60 * k + 60])
        b.step_seq(acts[60 * k:60 * k + 60])
        assert _packed(b)
        _same(a, b, torch, k)
    assert int(b.t.max()) > 255 and int((b.flags >> 16).max()) > 255
    for e in (a, b):
        e.t.fill_(65530)
    for k in range(3):
        _steps(a, acts[7 * k:7 * k + 7], autoreset=False)
        b.step_seq(acts[7 * k:7 * k + 7], autoreset=False)
        assert _packed(b)
        _same(a, b, torch, k)
    assert int(b.t.min()) == 65530 + 21


@pytest.mark.gpu
def test_no_stale_private_state(torch):
    """The record never outlives its window: a masked reset and a restored checkpoint between windows, two handles
    alternating on the device's queue, a third identical call (the recorded window reused: nothing recorded, nothing
    uploaded) and the same call with another action buffer all equal the stepwise path."""
    tab2, tab4 = T.compile_scenario(T.baseline_scenario(2)), T.compile_scenario(T.baseline_scenario(4))
    n, K = 1000, 5
    a2, b2, a4, b4 = _engine(tab2, n), _engine(tab2, n), _engine(tab4, n), _engine(tab4, n)
    acts2, acts4 = _acts(torch, 11, 4 * K, 2, n), _acts(torch, 12, 4 * K, 4, n)
    mask = torch.zeros(n, dtype=torch.uint8, device="cuda")
    mask[::3] = 1
    blob = None
    for w in range(4):  # two handles, window by window
        for a, b, acts in ((a2, b2, acts2), (a4, b4, acts4)):
            _steps(a, acts[K * w:K * w + K])
            b.step_seq(acts[K * w:K * w + K])
            assert _packed(b)
            _same(a, b, torch, w)
        if w == 0:
            blob = b2.save_state()
            for e in (a2, b2):
                e.reset(mask=mask, seed=9)
        if w == 2:
            for e in (a2, b2):
                e.load_state(blob)
    # the same call three times: the second and third reuse the recording
    b2.step_seq(acts2[:K])
    c1 = b2.queue_counters()
    b2.step_seq(acts2[:K])
    b2.step_seq(acts2[:K])
    d = {k: b2.queue_counters()[k] - c1[k] for k in c1}
    assert d["recordings"] == 0 and d["uploads"] == 0 and d["windows"] == 2 and d["packets"] == 2 * K
    for _ in range(3):
        _steps(a2, acts2[:K])
    _same(a2, b2, torch, "reused")
    other = acts2[K:2 * K].clone()  # the same call, another action pointer
    b2.step_seq(other)
    _steps(a2, other)
    assert _packed(b2)
    _same(a2, b2, torch, "other pointer")
    assert torch.equal(a2.stats_tensor(), b2.stats_tensor()) and torch.equal(a4.stats_tensor(), b4.stats_tensor())


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["fl2_slip", "fl2_randstart", "RMX_SEQ_PACKED=0", "wave_stats", "global"])
def test_ineligible_handles_keep_todays_window(which, configs, torch, monkeypatch):
    """Slip and random-start handles, per-wave statistics, the global-table step and RMX_SEQ_PACKED=0 run the window of K
    column-to-column steps: on the queue, one packet per step, not packed, equal to the stepwise path."""
    knob = {"RMX_SEQ_PACKED=0": ("RMX_SEQ_PACKED", "0"), "wave_stats": ("RMX_FAST_STATS", "wave"),
            "global": ("RMX_FAST_TABLES", "global")}.get(which)
    if knob:
        monkeypatch.setenv(*knob)
    tab = T.compile_scenario(configs[which] if which in configs else T.baseline_scenario(2))
    n, K = 1000, 6
    a, b = _engine(tab, n), _engine(tab, n)
    hi = 4 if tab.stochastic and tab.kind == FL else 5  # FrozenLake's slip map has no wait
    acts = torch.as_tensor(np.random.default_rng(2).integers(0, hi, size=(3 * K, tab.n_agents, n), dtype=np.int32),
                           device="cuda").contiguous()
    ra = torch.zeros(4, dtype=torch.float64, device="cuda")
    rb = torch.zeros(4, dtype=torch.float64, device="cuda")
    c0 = b.queue_counters()
    for w in range(3):
        _steps(a, acts[K * w:K * w + K], out=ra)
        b.step_seq(acts[K * w:K * w + K], out=rb)
        assert not _packed(b) and b.queue_info()["dispatch"] == "queue"
        _same(a, b, torch, w)
        assert torch.equal(ra, rb)
    d = b.queue_counters()
    assert d["packets"] - c0["packets"] == 3 * K and d["windows"] - c0["windows"] == 3


@pytest.mark.gpu
@pytest.mark.parametrize("K,every", [(2, 1), (7, 1), (7, 3)])
def test_timing_changes_nothing(K, every, torch):
    """rmx_queue_timing on: a packed window's results are unchanged and every strided packet (and the last) is stamped."""
    tab = T.compile_scenario(T.baseline_scenario(2))
    n = 1000
    a, b = _engine(tab, n), _engine(tab, n)
    acts = _acts(torch, 4, K, 2, n)
    _steps(a, acts)
    b.queue_timing(every)
    try:
        b.step_seq(acts)
        ts = b.queue_times().astype(np.int64)
    finally:
        b.queue_timing(0)
    assert _packed(b)
    _same(a, b, torch)
    assert ts[:, 0].tolist() == sorted(set(list(range(0, K - 1, every)) + [K - 1]))
    assert ((ts[:, 2] - ts[:, 1]) > 0).all() and (ts[1:, 1] >= ts[:-1, 2]).all()


# ---- host check of the record's helpers (no GPU) ----------------------------------------------------------------
PACK_CHECK = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include "rmx_layout.h"
using namespace rmx;
static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); bad = 1; } } while (0)
int main() {
  // every field at both ends and around them, every combination: the cell word gives back x, y, q and nothing else
  const uint32_t ends[] = {0u, 1u, 2u, 127u, 128u, 253u, 254u, 255u};
  for (uint32_t x : ends) for (uint32_t y : ends) for (uint32_t q : ends) {
    const uint32_t w = pk_cell(x, y, q);
    CHECK(pk_x(w) == x && pk_y(w) == y && pk_q(w) == q && (w >> 24) == 0u);
  }
  // a field never leaks into its neighbours
  CHECK(pk_cell(255u, 0u, 0u) == 0x000000FFu && pk_cell(0u, 255u, 0u) == 0x0000FF00u && pk_cell(0u, 0u, 255u) == 0x00FF0000u);
  // wider inputs are cut to their byte, never spilled into a neighbour (the kernel only packs table bytes)
  CHECK(pk_cell(0x1FFu, 0u, 0u) == 0xFFu && pk_cell(0u, 0x100u, 0u) == 0u && pk_cell(0u, 0u, 0xFFFFFFFFu) == 0x00FF0000u);
  // the columns of the record: 3A + 1 distinct ones in [0, 3A], for every agent count of the fast path
  for (int A = 1; A <= kFastMaxAgents; ++A) {
    bool seen[3 * kFastMaxAgents + 1] = {};
    for (int a = 0; a < A; ++a) {
      const int c[3] = {pk_col_cell(A, a), pk_col_flags(A, a), pk_col_ret(A, a)};
      for (int k = 0; k < 3; ++k) { CHECK(c[k] >= 0 && c[k] < 3 * A && !seen[c[k]]); seen[c[k]] = true; }
    }
    CHECK(pk_col_t(A) == 3 * A && !seen[pk_col_t(A)]);
    CHECK(pk_bytes(A, 1000) == (size_t)(3 * A + 1) * 4000);
    CHECK(pk_bytes(A, (size_t)1 << 20) < ((size_t)1 << 31));  // 32-bit buffer offsets below 1M envs
  }
  // the flags word, ep_ret and t are whole words of the record: nothing to pack, all 32 bits kept by construction
  static_assert(kIoCols == 0 && kIoColsToPk == 1 && kIoPkToPk == 2 && kIoPkToCols == 3, "symbol names carry these");
  std::printf(bad ? "pack check FAILED\n" : "pack check ok\n");
  return bad;
}
"""


def test_pack_helpers_on_the_host(tmp_path):
    """rmx_layout.h's pack / unpack helpers at every field's extremes, as a plain C++ program on the CPU."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "pack_check.cpp"
    src.write_text(PACK_CHECK)
    exe = tmp_path / "pack_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", _capi.CSRC, str(src), "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "pack check ok" in r.stdout, r.stdout + r.stderr
