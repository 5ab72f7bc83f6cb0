"""The QR-max learn step on the device (csrc/rmx_learn_qrmax.hip behind rmx.learn.VecQRMax on a VecRMEnv): the
reference fixtures, device against host bit for bit over every agent-count bucket, block edge and policy with thresholds
1 and 2, worlds below and above one workgroup of (s, q, a) entries, a slip world with random starts, one solve per
learner in a step where several pairs become known, and the successor-list capacity at a block edge.
"""
import dataclasses

import numpy as np
import pytest

import qrmax_common as QC
import slearn_common as SC
from rmx import tables as T
from rmx.engine import HostRMEnv, VecRMEnv
from test_learn_gpu import WORLDS, _dev_actions
from test_random_maps_gpu import random_tables

pytestmark = pytest.mark.gpu

BLOCK = 64  # kRMaxBlock, csrc/rmx_rmax.h


@pytest.mark.parametrize("case", QC.EXPECTED)
def test_fixtures_from_the_reference_qrmax_on_the_device(case):
    QC.replay_fixture(case, VecRMEnv, _dev_actions)


# tests/test_learn_gpu.py's worlds: A = 1, 2, 4, 3, 5, 8 (every AMAX bucket; 5 and 8 share the last), N = 1, 63, 64,
# 257, 65, 257, both kinds; max_t = 20 and 20 steps.  Each of the three policies runs on three of them.
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
    monkeypatch.setenv("RMX_QRMAX_GRID", str(grid))
    seen = QC.device_equals_host(tab, N, VecRMEnv, HostRMEnv, _dev_actions, policy, threshold, K=20)
    assert seen["solves"] > 0 and seen["known"] > 0 and seen["sweeps"] >= 2 and seen["total"] >= seen["sweeps"], seen
    assert seen["rows4"] > BLOCK  # the (s, q, a) stride of a solve wraps
    # an agent-step is at most one solve: a step's solves are its worklist entries
    assert max(seen["per_step"]) <= learners, seen
    if threshold == 1 and learners > 1:  # the first step has most learners on the worklist: more than workgroups
        assert seen["per_step"][0] > grid and seen["per_step"][0] >= learners // 3, seen


def test_a_world_below_one_workgroup_of_entries():
    tab = dataclasses.replace(random_tables(9, T.FROZEN_LAKE, 7, 1, 1, 2, 1, False), max_t=20)
    assert 4 * tab.width * tab.height * int(max(tab.enc_nq)) < BLOCK
    seen = QC.device_equals_host(tab, 1, VecRMEnv, HostRMEnv, _dev_actions, "hash", 2, K=20)
    assert seen["solves"] > 0 and seen["rows4"] < BLOCK and 1 in seen["per_step"] and 0 in seen["per_step"], seen
    seen = QC.device_equals_host(tab, 65, VecRMEnv, HostRMEnv, _dev_actions, "numpy", 1, K=20)
    assert seen["solves"] > 0, seen


def test_device_equals_host_on_a_slip_world_with_random_starts():
    tab = SC.fl_slip_randstart_world()  # A = 5, slip and random starts, max_t = 20
    N = 65
    for threshold in (1, 2):
        seen = QC.device_equals_host(tab, N, VecRMEnv, HostRMEnv, _dev_actions, "actions", threshold, K=20,
                                     caller=lambda rng: SC.caller_actions(rng, tab, N))
        assert seen["solves"] > 0, seen


def test_with_qrm_several_pairs_become_known_in_a_step_and_each_learner_solves_once(monkeypatch):
    """use_qrm, thresholds 2, one agent walking right (3), left (2), right, left: when the walk takes the same action in
    the same cell again, the pairs of every RM state become known in that one agent-step (the state actually held is
    counted twice and was known a step earlier), yet each learner solves exactly once in it."""
    make, _ = WORLDS["ow_a1_n1"]
    tab = dataclasses.replace(make(), max_t=20)
    assert tab.n_agents == 1 and int(tab.n_qrm[0]) >= 3
    for N in (1, 65):
        monkeypatch.setenv("RMX_QRMAX_GRID", "4")
        step = iter(range(100))
        walk = lambda rng: np.full((1, N), (3, 2)[next(step) % 2], np.int32)  # noqa: E731
        seen = QC.device_equals_host(tab, N, VecRMEnv, HostRMEnv, _dev_actions, "actions", 2, K=12, use_qrm=True,
                                     caller=walk)
        # every env walks the same walk: a step solves for every learner or for none, never twice for one
        assert set(seen["per_step"]) == {0, N}, seen
        assert seen["known"] >= 2 * N * int(tab.n_qrm[0]), seen  # several RM states' pairs per learner


def test_a_full_list_at_a_block_edge_drops_the_entry_and_keeps_the_canaries():
    """N = 65: one full wave and one lane of the next; cap = 1 inside larger tensors whose margins must stay as they
    were, and the model must equal the host's."""
    tab = SC.fl_slip_randstart_world()
    dev, hst = VecRMEnv(tab, 65), HostRMEnv(tab, 65)
    Ld = QC.cap_overflow(dev, _dev_actions)
    Lh = QC.cap_overflow(hst)
    QC.assert_same_model(Ld, Lh, "overflow")
    dev.close()
