"""The Q(lambda) learn step on the device (csrc/rmx_learn.hip behind rmx.learn.VecQLambda on a VecRMEnv): the reference
fixtures, device against host bit for bit over every agent-count bucket, block edge and policy, a slip world, the list
capacity at a block edge, the masked reset, and plain steps mixed in.
"""
import dataclasses

import numpy as np
import pytest

import lambda_common as MC
import learn_common as LC
import slearn_common as SC
from rmx import tables as T
from rmx.engine import HostRMEnv, VecRMEnv
from rmx.learn import VecQLambda
from test_lambda_cpu import cap_overflow
from test_learn_gpu import WORLDS, _dev_actions

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", MC.EXPECTED)
def test_fixtures_from_the_reference_qlearning_lambda_on_the_device(case):
    MC.replay_fixture(case, VecRMEnv, _dev_actions)


# tests/test_learn_gpu.py's worlds: A = 1, 2, 4, 3, 5, 8 (every AMAX bucket; 5 and 8 share the last), N = 1, 63, 64,
# 257, 65, 257, both kinds; max_t = 20 so that truncation and the auto-reset's wipe fall inside the 60 steps.  Each of
# the three policies runs on three of them; the rate alternates between 1 / visits and a fixed one.
SHAPES = [("ow_a1_n1", "actions", None), ("fl_a2_n63", "hash", 0.3), ("ow_a4_n64", "numpy", None),
          ("fl_a3_n257", "actions", 0.3), ("fl_a5_n65", "numpy", 0.3), ("ow_a8_n257", "hash", None),
          ("fl_a5_n65", "actions", None), ("ow_a8_n257", "numpy", 0.3), ("ow_a4_n64", "hash", 0.3)]


@pytest.mark.parametrize("name,policy,lr", SHAPES)
def test_device_equals_host_bit_for_bit(name, policy, lr):
    make, N = WORLDS[name]
    tab = dataclasses.replace(make(), max_t=20)
    seen = MC.device_equals_host(tab, N, VecRMEnv, HostRMEnv, _dev_actions, policy, K=60, lr=lr)
    assert seen["visited"] > 0 and seen["longest"] > 4 and seen["wrapped"], seen  # (longer than one sweep batch)


def test_device_equals_host_on_a_slip_world_with_random_starts():
    tab = SC.fl_slip_randstart_world()  # A = 5, slip and random starts, max_t = 20
    N = 65
    seen = MC.device_equals_host(tab, N, VecRMEnv, HostRMEnv, _dev_actions, "actions", K=60, lr=0.3,
                                 caller=lambda rng: SC.caller_actions(rng, tab, N))
    assert seen["visited"] > 0 and seen["longest"] > 4 and seen["wrapped"], seen
    seen = MC.device_equals_host(tab, N, VecRMEnv, HostRMEnv, _dev_actions, "numpy", K=60, lr=None)
    assert seen["visited"] > 0 and seen["wrapped"], seen


def test_a_full_list_at_a_block_edge_drops_the_trace_and_keeps_the_canaries():
    """N = 65: one full wave and one lane of the next; cap = 3 inside larger tensors whose margins must stay as they
    were (no write past slot cap, past env N or by a tail lane), and the lists must equal the host's."""
    make, N = WORLDS["fl_a5_n65"]
    tab = dataclasses.replace(make(), max_t=20)
    dev, hst = VecRMEnv(tab, N), HostRMEnv(tab, N)
    Ld = cap_overflow(dev, _dev_actions)
    Lh = cap_overflow(hst)
    LC.assert_same_bits(Ld.q, Lh.q, "q")
    assert np.array_equal(Ld.trace_counts(), Lh.trace_counts())
    LC.assert_same_bits(Ld.traces(), Lh.traces(), "traces")
    dev.close()


def test_reset_with_a_mask_clears_only_the_masked_envs():
    make, N = WORLDS["fl_a2_n63"]
    tab = dataclasses.replace(make(), max_t=20)
    dev = VecRMEnv(tab, N)
    dev.reset(seed=3)
    L = VecQLambda(dev, 0.9, 0.8, 0.2)
    for t in range(12):
        L.act_step(0.5, 3, t)
    before = L.trace_counts()
    assert before.any(axis=0).all()
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    dev.reset(mask=mask, seed=3)
    after = L.trace_counts()
    assert not after[:, mask == 1].any() and np.array_equal(after[:, mask == 0], before[:, mask == 0])
    only = np.zeros(N, np.uint8)
    only[1] = 1
    L.clear_traces(mask=only)
    now = L.trace_counts()
    assert not now[:, 1].any() and np.array_equal(now[:, 2], before[:, 2])
    L.clear_traces()
    assert not L.trace_counts().any()
    # rmx_reset_sync and rmx_set_state empty them too
    for again in ("reset_sync", "load_state"):
        for t in range(6):
            L.act_step(0.5, 3, t)
        assert L.trace_counts().any()
        if again == "reset_sync":
            dev.reset_sync(seed=3)
        else:
            dev.load_state(dev.save_state())
        assert not L.trace_counts().any(), again
    dev.check_errors()
    dev.close()


def test_plain_steps_between_learn_steps_leave_the_lists_alone():
    """Learn steps, plain rmx_step calls, learn steps again, on the device and on the host: the plain steps change no
    list (their auto-resets do not know the learners), and the two sides stay equal bit for bit throughout."""
    make, N = WORLDS["ow_a4_n64"]
    tab = dataclasses.replace(make(), max_t=20)
    dev, hst = VecRMEnv(tab, N), HostRMEnv(tab, N)
    for e in (dev, hst):
        e.reset(seed=5)
    Ld, Lh = VecQLambda(dev, 0.9, 0.8, 0.25), VecQLambda(hst, 0.9, 0.8, 0.25)
    acts = hst.fill_actions(31, 0, 60)
    dacts = _dev_actions(acts)
    for t in range(60):
        if 15 <= t < 40:  # past the step limit: every env auto-resets inside the plain steps
            if t == 15:
                cnt, e = Ld.trace_counts(), Ld.traces()
                assert cnt.any()
            dev.step(dacts[t])
            hst.step(acts[t])
            if t in (27, 39):
                assert np.array_equal(Ld.trace_counts(), cnt) and np.array_equal(LC.bits(Ld.traces()), LC.bits(e))
        else:
            Ld.step(dacts[t])
            Lh.step(acts[t])
    LC.assert_same_bits(Ld.q, Lh.q, "q")
    assert np.array_equal(LC.host(Ld.visits), Lh.visits)
    assert np.array_equal(Ld.trace_counts(), Lh.trace_counts())
    LC.assert_same_bits(Ld.traces(), Lh.traces(), "traces")
    LC.assert_same_columns(LC.columns(dev), LC.columns(hst), "columns")
    dev.check_errors()
    dev.close()
