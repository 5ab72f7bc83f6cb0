"""The R-max learn step on the device (csrc/rmx_learn_rmax.hip behind rmx.learn.VecRMax on a VecRMEnv): the reference
fixtures, device against host bit for bit over every agent-count bucket, block edge and policy with thresholds 1 and 2,
worlds below and above one workgroup of (s, k) pairs, a slip world with random starts, two crossings in one step, and
the successor-list capacity at a block edge.
"""
import dataclasses

import numpy as np
import pytest

import learn_common as LC
import rmax_common as RC
import slearn_common as SC
from rmx import tables as T
from rmx.engine import HostRMEnv, VecRMEnv
from rmx.learn import VecRMax
from test_learn_gpu import WORLDS, _dev_actions
from test_random_maps_gpu import random_tables

pytestmark = pytest.mark.gpu

BLOCK = 64  # kRMaxBlock, csrc/rmx_rmax.h


@pytest.mark.parametrize("case", RC.EXPECTED)
def test_fixtures_from_the_reference_rmax_on_the_device(case):
    RC.replay_fixture(case, VecRMEnv, _dev_actions)


# tests/test_learn_gpu.py's worlds: A = 1, 2, 4, 3, 5, 8 (every AMAX bucket; 5 and 8 share the last), N = 1, 63, 64,
# 257, 65, 257, both kinds; max_t = 20 and 20 steps, so that a solve is some ten sweeps and the host side stays quick.  Each of the
# three policies runs on three of them.
SHAPES = [("ow_a1_n1", "actions"), ("fl_a2_n63", "hash"), ("ow_a4_n64", "numpy"), ("fl_a3_n257", "actions"),
          ("fl_a5_n65", "numpy"), ("ow_a8_n257", "hash"), ("fl_a5_n65", "actions"), ("ow_a8_n257", "numpy"),
          ("ow_a4_n64", "hash")]


@pytest.mark.parametrize("threshold", [1, 2])
@pytest.mark.parametrize("name,policy", SHAPES)
def test_device_equals_host_bit_for_bit(name, policy, threshold, monkeypatch):
    make, N = WORLDS[name]
    tab = dataclasses.replace(make(), max_t=20)
    learners = tab.n_agents * N
    # fewer workgroups than the longest worklist, so that the grid stride wraps (the default grid is 2048)
    grid = 512 if name == "ow_a8_n257" else max(1, min(7, learners // 3))
    monkeypatch.setenv("RMX_RMAX_GRID", str(grid))
    seen = RC.device_equals_host(tab, N, VecRMEnv, HostRMEnv, _dev_actions, policy, threshold, K=20)
    assert seen["solves"] > 0 and seen["known"] > 0 and seen["sweeps"] >= 2, seen  # (a sweep that wrote, at least)
    assert seen["rows4"] > BLOCK  # the (s, k) stride of a solve wraps
    # without QRM an agent-step is one experience: a step's solves are its worklist entries
    if threshold == 1 and learners > 1:  # the first step has most learners on the worklist: more than workgroups
        assert seen["per_step"][0] > grid and seen["per_step"][0] >= learners // 3, seen
    if threshold == 2 and learners < 200:
        assert 0 in seen["per_step"], seen  # steps with an empty worklist


def test_a_world_below_one_workgroup_of_pairs_and_single_entries():
    tab = dataclasses.replace(random_tables(9, T.FROZEN_LAKE, 7, 1, 1, 2, 1, False), max_t=20)
    assert 4 * tab.width * tab.height * int(max(tab.enc_nq)) < BLOCK
    seen = RC.device_equals_host(tab, 1, VecRMEnv, HostRMEnv, _dev_actions, "hash", 2, K=20)
    assert seen["solves"] > 0 and seen["rows4"] < BLOCK and 1 in seen["per_step"] and 0 in seen["per_step"], seen
    seen = RC.device_equals_host(tab, 65, VecRMEnv, HostRMEnv, _dev_actions, "numpy", 1, K=20)
    assert seen["solves"] > 0, seen


def test_device_equals_host_on_a_slip_world_with_random_starts():
    tab = SC.fl_slip_randstart_world()  # A = 5, slip and random starts, max_t = 20
    N = 65
    for threshold in (1, 2):
        seen = RC.device_equals_host(tab, N, VecRMEnv, HostRMEnv, _dev_actions, "actions", threshold, K=20,
                                     caller=lambda rng: SC.caller_actions(rng, tab, N))
        assert seen["solves"] > 0, seen


def test_with_qrm_a_learner_crosses_twice_in_one_step(monkeypatch):
    """use_qrm, threshold 2, one agent walking right (3), left (2), right, left: the RM state actually held is counted twice
    and its pair crosses at once, the other RM states' pairs are counted once; when the walk takes the same action in
    the same cell again they all cross in that one agent-step, each solved before the next experience."""
    make, _ = WORLDS["ow_a1_n1"]
    tab = dataclasses.replace(make(), max_t=20)
    assert tab.n_agents == 1 and int(tab.n_qrm[0]) >= 3
    for N in (1, 65):
        monkeypatch.setenv("RMX_RMAX_GRID", "4")
        step = iter(range(100))
        walk = lambda rng: np.full((1, N), (3, 2)[next(step) % 2], np.int32)  # noqa: E731
        seen = RC.device_equals_host(tab, N, VecRMEnv, HostRMEnv, _dev_actions, "actions", 2, K=12, use_qrm=True,
                                     caller=walk)
        assert max(seen["per_step"]) >= 2 * N, seen  # every env walks the same walk


def test_a_full_list_at_a_block_edge_drops_the_entry_and_keeps_the_canaries():
    """N = 65: one full wave and one lane of the next; cap = 1 inside larger tensors whose margins must stay as they
    were, and the model must equal the host's."""
    tab = SC.fl_slip_randstart_world()
    dev, hst = VecRMEnv(tab, 65), HostRMEnv(tab, 65)
    Ld = RC.cap_overflow(dev, _dev_actions)
    Lh = RC.cap_overflow(hst)
    RC.assert_same_model(Ld, Lh, "overflow")
    dev.close()
