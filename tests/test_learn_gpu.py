"""The learn step on the device (csrc/rmx_learn.hip behind rmx.learn.VecQLearning on a VecRMEnv): the reference
fixtures, device against host bit for bit over every agent-count bucket, block edge and table shape, the engine's
policy under sharding, learner tables past 4 GiB, and the step's own columns against a twin stepped with rmx_step.
"""
import dataclasses
import json
import os

import numpy as np
import pytest

import learn_common as LC
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv, VecRMEnv
from rmx.learn import VecQLearning
from test_limits_gpu import FRACT, compile_world, make_world
from test_random_maps_gpu import random_tables

pytestmark = pytest.mark.gpu

FL, OW = T.FROZEN_LAKE, T.OFFICE_WORLD


def _dev_actions(a):
    import torch
    return torch.as_tensor(a, device="cuda")


@pytest.mark.parametrize("case", LC.EXPECTED)
def test_fixtures_from_the_reference_qlearning_on_the_device(case):
    LC.replay_fixture(case, VecRMEnv, _dev_actions)


def _golden(name):
    with open(os.path.join(LC.GOLDEN, "configs.json")) as f:
        return T.compile_scenario(json.load(f)[name])


# name: (tables, N).  max_t = 20 so that truncation and the auto-reset fall inside the 60 steps.  Every AMAX bucket
# (1, 2, 3, 4, 8 with A = 5 and 8), one env, a wave less / exactly / more than one, more than one block, both kinds,
# agents with different encoder strides (fl2_open: 9 and 3 RM states, so S_max pads agent 1), 17 counterfactuals.
WORLDS = {
    "ow_a1_n1": (lambda: random_tables(4, OW, 9, 7, 1, 4, 5, True), 1),
    "fl_a2_n63": (lambda: random_tables(1, FL, 6, 6, 2, 3, 3, False), 63),
    "ow_a4_n64": (lambda: random_tables(2, OW, 12, 10, 4, 6, 7, True), 64),
    "fl_a3_n257": (lambda: random_tables(3, FL, 14, 14, 3, 5, 6, False), 257),
    "fl_a5_n65": (lambda: random_tables(11, FL, 8, 7, 5, 5, 8, False), 65),
    "ow_a8_n257": (lambda: random_tables(13, OW, 10, 8, 8, 6, 10, True), 257),
    "fl_a2_n1000": (lambda: random_tables(7, FL, 7, 5, 2, 4, 4, False), 1000),
    "fl2_open_n65": (lambda: _golden("fl2_open"), 65),
    "fl1_qrm17_n64": (lambda: _golden("fl1_qrm17"), 64),
}


@pytest.mark.parametrize("name", sorted(WORLDS))
@pytest.mark.parametrize("use_qrm", [True, False])
def test_device_equals_host_bit_for_bit(name, use_qrm):
    make, N = WORLDS[name]
    tab = dataclasses.replace(make(), max_t=20)
    if name == "fl2_open_n65":
        assert len(set(int(v) for v in tab.enc_nq)) > 1
    if name == "fl1_qrm17_n64":
        assert int(tab.n_qrm[0]) == 17
    lr = 0.3 if use_qrm else None  # a fixed rate with the QRM experiences, 1 / visits with the single update
    rsh = use_qrm and tab.phi is not None
    K = 60
    kw = dict(with_qrm=True, with_enc_state=True)
    dev, hst = VecRMEnv(tab, N, **kw), HostRMEnv(tab, N, **kw)
    Ld = VecQLearning(dev, 0.9, lr, qtable_init=0.25, use_qrm=use_qrm, use_rsh=rsh)
    Lh = VecQLearning(hst, 0.9, lr, qtable_init=0.25, use_qrm=use_qrm, use_rsh=rsh)
    acts = hst.fill_actions(21, 0, K)
    dacts = _dev_actions(acts)
    for t in range(K):
        Ld.step(dacts[t])
        Lh.step(acts[t])
    assert np.array_equal(LC.bits(LC.host(Ld.q)), LC.bits(Lh.q))
    assert np.array_equal(LC.host(Ld.visits), Lh.visits)
    LC.assert_same_columns(LC.columns(dev), LC.columns(hst), name)
    assert (Lh.visits > 0).any() and (hst.t < K).all()
    dev.check_errors()
    dev.close()


def test_policy_steps_device_equals_host_and_a_shard_reproduces_its_rows():
    tab = dataclasses.replace(random_tables(2, OW, 12, 10, 4, 6, 7, True), max_t=20)
    NG, e0, n, K = 200, 70, 50, 60
    full_d, full_h = VecRMEnv(tab, NG), HostRMEnv(tab, NG)
    shard = VecRMEnv(tab, n, env_offset=e0, n_envs_global=NG)
    kw = dict(qtable_init=0.0, use_qrm=True, use_rsh=True)
    Ld, Lh, Ls = (VecQLearning(e, 0.9, 0.2, **kw) for e in (full_d, full_h, shard))
    import torch
    out_d = torch.zeros((tab.n_agents, NG), dtype=torch.int32, device="cuda")
    out_s = torch.zeros((tab.n_agents, n), dtype=torch.int32, device="cuda")
    out_h = np.zeros((tab.n_agents, NG), np.int32)
    seen = set()
    for t in range(K):
        best = t % 7 == 6
        for L, out in ((Ld, out_d), (Lh, out_h), (Ls, out_s)):
            L.act_step(0.3, 5, t, best=best, actions_out=out)
        assert np.array_equal(out_d.cpu().numpy(), out_h), t
        assert np.array_equal(out_s.cpu().numpy(), out_h[:, e0:e0 + n]), t
        seen |= set(out_h.ravel().tolist())
    assert seen == {0, 1, 2, 3}
    qd, qs = LC.host(Ld.q), LC.host(Ls.q)
    assert np.array_equal(LC.bits(qd), LC.bits(Lh.q)) and np.array_equal(LC.host(Ld.visits), Lh.visits)
    assert np.array_equal(LC.bits(qs), LC.bits(Lh.q[:, e0:e0 + n]))
    assert np.array_equal(LC.host(Ls.visits), Lh.visits[:, e0:e0 + n])
    # an evaluation step reads the tables only
    Ld.act_step(0.0, 5, K, best=True, learn=False)
    assert np.array_equal(LC.bits(LC.host(Ld.q)), LC.bits(qd))
    Lh.act_step(0.0, 5, K, best=True, learn=False)
    assert np.array_equal(LC.host(Ld.greedy()), Lh.greedy())
    for e in (full_d, shard):
        e.check_errors()
        e.close()


def test_tables_past_4_gib():
    """Learner tables whose byte offsets pass 2^31 and 2^32: the envs on either side of both offsets, the first and
    the last env equal host runs of those envs alone (the policy and the update are independent of the sharding)."""
    import torch
    tab = compile_world(make_world(seed=51, kind=OW, W=64, H=64, A=2, Q=2, n_ev=12, zone=(52, 52, 63, 63),
                                   rewards=FRACT, modifier=1.5, hazard_div=40))
    A = tab.n_agents
    per = 64 * 64 * int(max(tab.enc_nq)) * 4 * 8  # bytes of one learner
    assert per == 256 * 1024
    N = (2 ** 32 // per + 16 + A - 1) // A  # the smallest shard (plus a margin of 16 learners) that gets past 4 GiB
    assert A * N * per > 2 ** 32 and N == 8200
    free = torch.cuda.mem_get_info()[0]
    assert free > 2.2 * A * N * per, f"needs {2.2 * A * N * per / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} free"
    dev = VecRMEnv(tab, N)
    L = VecQLearning(dev, 0.9, 0.5, use_qrm=True)
    assert L.q.numel() * 8 > 2 ** 32
    K = 3
    for t in range(K):
        L.act_step(0.5, 9, t)
    picks = {(0, 0), (A - 1, N - 1)}
    for off in (2 ** 31, 2 ** 32):
        i = off // per  # the learner that starts at the offset, and the one before it
        picks |= {((i - 1) // N, (i - 1) % N), (i // N, i % N)}
    assert len(picks) == 6
    for a, e in sorted(picks):
        hst = HostRMEnv(tab, 1, env_offset=e, n_envs_global=N)
        Lh = VecQLearning(hst, 0.9, 0.5, use_qrm=True)
        for t in range(K):
            Lh.act_step(0.5, 9, t)
        assert (Lh.visits[a, 0] > 0).any()
        assert np.array_equal(LC.bits(L.q[a, e].cpu().numpy()), LC.bits(Lh.q[a, 0])), (a, e)
        assert np.array_equal(L.visits[a, e].cpu().numpy(), Lh.visits[a, 0]), (a, e)
    dev.check_errors()
    dev.close()


@pytest.mark.parametrize("name", ["fl_a2_n63", "ow_a4_n64", "fl_a5_n65"])
def test_learn_steps_leave_the_columns_and_statistics_as_rmx_step_on_the_device(name):
    """The statistics are sums of float32 episode returns of magnitude 2^-8 .. 2^8 over a few hundred episodes: every
    partial sum is exact in float64, so the return sum is equal whatever the kernel's association."""
    make, N = WORLDS[name]
    tab = dataclasses.replace(make(), max_t=20)
    K = 60
    kw = dict(with_qrm=True, with_enc_state=True)
    dev, twin = VecRMEnv(tab, N, **kw), VecRMEnv(tab, N, **kw)
    L = VecQLearning(dev, 0.9, 0.1, use_qrm=True)
    acts = HostRMEnv(tab, N).fill_actions(4, 0, K)
    acts[17, 0, 2] = 4  # wait
    acts[40, 0, 1] = 9  # invalid: reported by both
    dacts = _dev_actions(acts)
    for t in range(K):
        L.step(dacts[t])
        twin.step(dacts[t])
        if t % 25 == 0 or t == K - 1:
            LC.assert_same_columns(LC.columns(dev), LC.columns(twin), (name, t))
    assert np.array_equal(dev.stats().view(np.uint64), twin.stats().view(np.uint64))
    assert dev.stats()[_capi.STAT_EPISODES] > 0
    for e in (dev, twin):
        with pytest.raises(ValueError, match="action"):
            e.check_errors()
        e.close()
