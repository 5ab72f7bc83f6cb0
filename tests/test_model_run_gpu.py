"""Fused runs of the model learners on the device (csrc/rmx_learn_rmax_run.hip, csrc/rmx_learn_qrmax_run.hip behind
VecRMax.run / VecQRMax.run on a VecRMEnv): ONE launch of T steps, one wave per env, against the host's T single steps
and the device's looped run, bit for bit: every agent-count bucket and block edge, both kinds, both policies, thresholds
1 and 2, with and without QRM; a world below one wave of entries; a slip world with random starts; two crossings in
one agent-step; runs in pieces between single steps; the two-launch fallback for a world over the LDS limit; and the
successor-list capacity at a block edge."""
import dataclasses

import numpy as np
import pytest

import learn_common as LC
import model_run_common as MC
import slearn_common as SC
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv, VecRMEnv
from rmx.learn import VecQRMax, VecRMax
from test_learn_gpu import WORLDS
from test_random_maps_gpu import random_tables

pytestmark = pytest.mark.gpu

BLOCK = 64  # kRMaxBlock, csrc/rmx_rmax.h
LDS_MAX = 65536 - 512  # kModelRunLdsMax, csrc/rmx_internal.h: 64 KiB less the kernel's own words
STATES_MAX = 4064  # kRMaxStatesMax, csrc/rmx_rmax.h

# tests/test_learn_gpu.py's worlds: A = 1, 2, 4, 3, 5, 8 (every AMAX bucket; 5 and 8 share the last), N = 1, 63, 64,
# 257, 65, 257, both kinds; max_t = 20 and T = 20.  Each world runs two of the (threshold, policy, use_qrm) triples,
# chosen so that every world sees both thresholds, both policies and QRM on and off, and the six worlds together
# every pair of the three settings.
TRIPLES = [((1, "hash", True), (2, "numpy", False)), ((1, "numpy", False), (2, "hash", True)),
           ((1, "hash", False), (2, "numpy", True)), ((1, "numpy", True), (2, "hash", False))]
SHAPES = ["ow_a1_n1", "fl_a2_n63", "ow_a4_n64", "fl_a3_n257", "fl_a5_n65", "ow_a8_n257"]
CASES = [(name,) + triple for i, name in enumerate(SHAPES) for triple in TRIPLES[i % 4]]


@pytest.mark.parametrize("kind", MC.KINDS)
@pytest.mark.parametrize("name,threshold,policy,use_qrm", CASES)
def test_fused_run_equals_the_host_loop_and_the_device_loop(name, threshold, policy, use_qrm, kind):
    make, N = WORLDS[name]
    tab = dataclasses.replace(make(), max_t=20)
    seen = MC.run_equals_steps(kind, VecRMEnv, HostRMEnv, tab, N, threshold, 20, use_qrm=use_qrm,
                               numpy_policy=policy == "numpy", loop_cls=VecRMEnv)
    assert seen["solves"] > 0 and seen["known"] > 0 and seen["sweeps"] >= 2, seen  # (a sweep that wrote, at least)
    assert seen["rows4"] > BLOCK  # the lane stride of a solve wraps


@pytest.mark.parametrize("kind", MC.KINDS)
def test_a_world_below_one_wave_of_entries(kind):
    tab = dataclasses.replace(random_tables(9, T.FROZEN_LAKE, 7, 1, 1, 2, 1, False), max_t=20)
    assert 4 * tab.width * tab.height * int(max(tab.enc_nq)) < BLOCK
    seen = MC.run_equals_steps(kind, VecRMEnv, HostRMEnv, tab, 1, 2, 20)
    assert seen["solves"] > 0 and seen["rows4"] < BLOCK and 0 in seen["per_step"], seen
    seen = MC.run_equals_steps(kind, VecRMEnv, HostRMEnv, tab, 65, 1, 20, numpy_policy=True)
    assert seen["solves"] > 0, seen


@pytest.mark.parametrize("kind", MC.KINDS)
def test_a_slip_world_with_random_starts(kind):
    """The env generator columns and the episode counts (MC.same compares them on such a world) equal the host's."""
    tab = SC.fl_slip_randstart_world()  # A = 5, slip and random starts, max_t = 20
    assert tab.stochastic and tab.random_starts
    for threshold, numpy_policy in ((1, False), (2, True)):
        seen = MC.run_equals_steps(kind, VecRMEnv, HostRMEnv, tab, 65, threshold, 20, numpy_policy=numpy_policy)
        assert seen["solves"] > 0 and seen["resets"], seen


TWO_CROSSINGS_SEED = 6  # found on the host: the hashed policy's seed under which steps 14 and 17 solve twice


def test_rmax_with_qrm_crosses_twice_in_one_agent_step():
    """use_qrm, threshold 2, one agent: the RM state actually held is counted twice and crosses at once; when the
    policy takes the same action in the same cell again, the other RM states' pairs cross in that one agent-step, each
    solved before the next experience."""
    make, _ = WORLDS["ow_a1_n1"]
    tab = dataclasses.replace(make(), max_t=20)
    assert tab.n_agents == 1 and int(tab.n_qrm[0]) >= 3
    for N in (1, 65):
        seen = MC.run_equals_steps("rmax", VecRMEnv, HostRMEnv, tab, N, 2, 20, use_qrm=True, seed=TWO_CROSSINGS_SEED)
        if N == 1:
            assert max(seen["per_step"]) >= 2, seen


@pytest.mark.parametrize("kind", MC.KINDS)
def test_runs_in_pieces_between_single_steps_and_a_greedy_run(kind):
    """run(7), three act_steps, run(13) on the device against 23 single steps on the host; then a best=True run that
    does not learn changes no model, and one that learns equals the host's."""
    make, N = WORLDS["fl_a2_n63"]
    tab = dataclasses.replace(make(), max_t=20)
    (ed, Ld), (eh, Lh) = (MC.make(cls, kind, tab, N, 2, use_qrm=True) for cls in (VecRMEnv, HostRMEnv))
    od, oh = MC.new_out(Ld, 23), MC.new_out(Lh, 23)
    MC.run(Ld, 7, 0, od[:7])
    MC.steps(Ld, 3, 7, od[7:10])
    MC.run(Ld, 13, 10, od[10:])
    MC.steps(Lh, 23, 0, oh)
    MC.same(kind, Ld, Lh, "pieces", (od, oh))
    assert Lh.solve_info()[0] > 0
    before, solves = MC.COMMON[kind].model_of(Ld), Ld.solve_info()
    for L in (Ld, Lh):
        MC.run(L, 9, 23, best=True, learn=False)
    after = MC.COMMON[kind].model_of(Ld)
    for k in before:
        x, y = (LC.bits(v) if v.dtype.kind == "f" else v for v in (before[k], after[k]))
        assert np.array_equal(x, y), k
    assert Ld.solve_info() == solves
    MC.same(kind, Ld, Lh, "greedy, not learning")
    od, oh = MC.new_out(Ld, 9), MC.new_out(Lh, 9)
    MC.run(Ld, 9, 32, od, best=True)
    MC.steps(Lh, 9, 32, oh, best=True)
    MC.same(kind, Ld, Lh, "greedy, learning", (od, oh))
    for e in (ed, eh):
        e.check_errors()
        e.close()


def _blob_bytes(tab):
    """The table blob the kernels stage (csrc/rmx_tables.cpp, build_table_blob): sections aligned to 16 bytes."""
    al = lambda n: (n + 15) & ~15  # noqa: E731
    HW, A, QE = tab.width * tab.height, tab.n_agents, tab.n_rm_states * tab.n_events
    n = al(2 * HW)
    n = al(n + A * HW)
    n = al(n + A * QE)
    n = al(n + 4 * A * QE)
    if tab.shape is not None:
        n = al(n + 4 * A * QE)
    if tab.qrm_states is not None and tab.qrm_states.size:
        n = al(n + A * tab.qrm_states.shape[-1])
    return n


@pytest.mark.parametrize("kind", MC.KINDS)
def test_a_world_over_the_lds_limit_takes_the_two_launch_steps(kind):
    """31 x 59 cells, two agents of two RM states: 16 B per state plus the tables pass 64 KiB, while one row fewer
    fits beside the kernel's own words.  The run is then T two-launch steps behind the same call, and equals the host."""
    mk = lambda H: dataclasses.replace(random_tables(17, T.FROZEN_LAKE, 31, H, 2, 2, 2, False), max_t=20)  # noqa: E731
    tab, below = mk(59), mk(58)
    s_max = lambda t: t.width * t.height * int(max(t.enc_nq))  # noqa: E731
    assert s_max(tab) <= STATES_MAX
    assert _blob_bytes(tab) + 16 * s_max(tab) > 65536 > LDS_MAX >= _blob_bytes(below) + 16 * s_max(below)
    env, L = MC.make(VecRMEnv, kind, tab, 2, 1)
    assert MC.lds_bytes(L) == _blob_bytes(tab) + 16 * s_max(tab)  # the handle's own blob is the size computed here
    env.close()
    seen = MC.run_equals_steps(kind, VecRMEnv, HostRMEnv, tab, 2, 1, 3)
    assert seen["solves"] > 0, seen


@pytest.mark.parametrize("kind", MC.KINDS)
def test_a_full_list_at_a_block_edge_in_a_fused_run(kind):
    """cap_overflow's world (slip, random starts, N = 65, succ_cap = 1 inside canaried allocations) through fused
    runs: the canaries are intact, the model equals the host's, and check_errors raises as on the stepwise path."""
    tab = SC.fl_slip_randstart_world()
    learners, raws = [], []
    for cls in (VecRMEnv, HostRMEnv):
        env = cls(tab, 65)
        env.reset(seed=9)
        if kind == "rmax":
            L = VecRMax(env, 0.5, s_a_threshold=3, vi_delta=1e-3, succ_cap=1)
            arrays = dict(rsum=L.rsum, succ_idx=L.succ_idx, succ_cnt=L.succ_cnt)
        else:
            L = VecQRMax(env, 0.5, nsamples_te=3, nsamples_re=3, vi_delta=1e-3, succ_cap=1)
            arrays = L.model()
        raw, views = {}, {}
        for name, arr in arrays.items():
            shape = tuple(arr.shape)
            n = int(np.prod(shape))
            if L.host:
                raw[name] = np.full(n + 128, 7, arr.dtype)
                views[name] = raw[name][64:64 + n].reshape(shape)
                views[name][...] = 0
            else:
                raw[name] = env.torch.full((n + 128,), 7, dtype=arr.dtype, device=env.device)
                views[name] = raw[name][64:64 + n].view(shape)
                views[name].zero_()
        if kind == "rmax":
            L.bind_model(views["rsum"], views["succ_idx"], views["succ_cnt"], 1)
        else:
            L.bind_model(1, **views)
        MC.run(L, 25, 0)
        MC.run(L, 15, 25)
        with pytest.raises(RuntimeError, match="successor") as ei:
            env.check_errors()
        assert f"rc={_capi.RMX_E_MODEL}" in str(ei.value)
        env.check_errors()  # reported once, then cleared
        for name, r in raw.items():
            r = LC.host(r)
            assert (r[:64] == 7).all() and (r[-64:] == 7).all(), name
        learners.append(L)
        raws.append(raw)
    Ld, Lh = learners
    MC.same(kind, Ld, Lh, "overflow")
    total = LC.host(Lh.counts if kind == "rmax" else Lh.n_tsa)
    cnt = LC.host(Lh.succ_cnt)[..., 0]
    assert (cnt <= total).all() and (cnt < total).any()  # dropped entries were still counted
    for L in learners:
        L.env.close()
