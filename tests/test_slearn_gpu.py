"""The learn step on slip and random-start worlds on the device (the STOCH instantiations of csrc/rmx_learn.hip behind
VecQLearning on a VecRMEnv built from a stochastic or random-start scenario): the recorded runs of the reference,
device against host bit for bit over a partial last block and the 8-agent bucket with canaries around the generator
and episode columns, and the twin run against rmx_step."""
import ctypes as C

import numpy as np
import pytest

import learn_common as LC
import policy_common as PC
import slearn_common as SC
from rmx import _capi
from rmx.engine import HostRMEnv, VecRMEnv
from rmx.learn import VecQLearning
from test_random_maps_gpu import random_slip_tables

pytestmark = pytest.mark.gpu

FL, OW = SC.FL, SC.OW
CANARY = 0x5A5AC3C3A5A53C3C
CANARY32 = 0x5A5AC3C3


@pytest.mark.parametrize("case", SC.EXPECTED)
def test_whole_runs_of_the_reference_on_the_device(case):
    SC.replay_fixture(case, VecRMEnv)


# N = 300: a full 256-thread block and a partial one whose last wave has a tail; A = 5: the 8-agent bucket, whose agents
# 5..7 own no column words.  max_t = 20 so that truncation, the auto-reset and the reseed fall inside the run many times.
WORLDS = {
    "fl_a3_n300": (lambda: SC.dataclasses.replace(random_slip_tables(3, FL, 14, 14, 3, 5, 6, False, {}), max_t=20), 300),
    "fl_a5_n70_randstart": (lambda: SC.fl_slip_randstart_world(), 70),
    "ow_a4_n65_allslip": (lambda: SC.dataclasses.replace(
        random_slip_tables(2, OW, 12, 10, 4, 6, 7, True, {"all_slip": True}), max_t=20), 65),
}
K = 70


def _rebind_with_canaries(dev):
    """The env generator and episode columns again, each inside a larger allocation of canary words."""
    import torch
    N = dev.N
    rng_store = torch.full((16 + 4 * N + 64,), CANARY, dtype=torch.int64, device=dev.device)
    ep_store = torch.full((32 + N + 64,), CANARY32, dtype=torch.int32, device=dev.device)
    rng, ep = rng_store[16:16 + 4 * N].view(4, N), ep_store[32:32 + N]
    rng.copy_(dev.rng)
    ep.copy_(dev.episode)
    dev.rng, dev.episode = rng, ep
    dev._buf.rng, dev._buf.episode = rng.data_ptr(), ep.data_ptr()
    _capi.check(dev.lib.rmx_bind(dev._h, C.byref(dev._buf)), "rmx_bind")
    return rng_store, ep_store


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_device_equals_host_bit_for_bit_with_canaries_around_the_columns(name):
    import torch
    make, N = WORLDS[name]
    tab = make()
    A = tab.n_agents
    assert tab.stochastic and tab.max_t == 20 and bool(tab.random_starts) == ("randstart" in name)
    dev = VecRMEnv(tab, N, with_qrm=True, with_enc_state=True)
    hst = HostRMEnv(tab, N, with_qrm=True, with_enc_state=True)
    dev.reset(seed=17)
    hst.reset(seed=17)
    rng_store, ep_store = _rebind_with_canaries(dev)
    seeds = np.random.default_rng(A * N).integers(0, 2 ** 64, size=(A, N), dtype=np.uint64)
    kw = dict(qtable_init=0.25, use_qrm=True)
    Ld = VecQLearning(dev, 0.9, 0.3, policy_seeds=seeds, **kw)
    Lh = VecQLearning(hst, 0.9, 0.3, policy_seeds=seeds, **kw)
    n = 5 * A * N
    store = torch.full((16 + n + 64,), CANARY, dtype=torch.int64, device=dev.device)
    PC.bind_column(Ld, store[16:16 + n].view(5, A, N))
    PC.seed_column(Ld, seeds)
    assert np.array_equal(PC.words(Ld.rng), Lh.rng)
    out_d = torch.full((K, A, N), -1, dtype=torch.int32, device=dev.device)
    out_h = np.full((K, A, N), -1, np.int32)
    rng = np.random.default_rng(5)
    slips = resets = 0
    for t in range(K):
        best, learn = t % 11 == 10, t % 13 != 12
        # what the host is about to do: the envs that reset, and (below) the moves that were not the intended ones
        resetting = (hst.flags[0] & _capi.F_ENV_DONE) != 0
        resets += int(resetting.sum())
        x0 = hst.pos_x.copy()
        if t % 3 == 0:  # the caller's actions
            a = SC.caller_actions(rng, tab, N)
            out_h[t] = a
            out_d[t] = torch.as_tensor(a, device=dev.device)
            Ld.step(out_d[t])
            Lh.step(a)
        elif t % 3 == 1:  # the engine's policy
            Ld.act_step(0.2, 23, t, best=best, learn=learn, actions_out=out_d[t])
            Lh.act_step(0.2, 23, t, best=best, learn=learn, actions_out=out_h[t])
        else:  # the learners' numpy streams
            Ld.act_step(0.2, reference_stream=True, best=best, learn=learn, actions_out=out_d[t])
            Lh.act_step(0.2, reference_stream=True, best=best, learn=learn, actions_out=out_h[t])
        # an intended move up or down that changed x was a slip (moves are along one axis; a reset moves both)
        slips += int(((out_h[t] < 2) & (hst.pos_x != x0) & ~resetting[None, :]).sum())
    # liveness, from the host side first
    assert resets >= N and hst.episode.min() >= 1 and hst.episode.max() >= 3
    assert (Lh.visits > 0).any() and (hst.t <= 21).all()
    assert slips >= 20
    # the device against the host
    assert np.array_equal(out_d.cpu().numpy(), out_h)
    LC.assert_same_bits(Ld.q, Lh.q, (name, "q"))
    assert np.array_equal(LC.host(Ld.visits), Lh.visits)
    assert np.array_equal(PC.words(Ld.rng), Lh.rng)
    LC.assert_same_columns(SC.env_columns(dev), SC.env_columns(hst), name)
    sd, sh = dev.stats(), hst.stats()
    assert np.array_equal(sd[1:], sh[1:]) and sh[1] >= N
    # the words around the three columns are the caller's
    w = PC.words(store)
    assert (w[:16] == CANARY).all() and (w[16 + n:] == CANARY).all()
    w = PC.words(rng_store)
    assert (w[:16] == CANARY).all() and (w[16 + 4 * N:] == CANARY).all()
    w = ep_store.cpu().numpy()
    assert (w[:32] == CANARY32).all() and (w[32 + N:] == CANARY32).all()
    dev.check_errors()
    dev.close()


def test_learn_step_and_rmx_step_leave_the_same_env_on_the_device():
    import torch
    tab = SC.slip_world("fl_slip_delay")
    seen = SC.twin_run(VecRMEnv, tab, 257, 40, seed=31, as_actions=lambda a: torch.as_tensor(a, device="cuda"),
                       exact_stats=False)
    assert seen["evaluated"] == 10 and seen["moved_rng"] >= 35
    assert seen["episodes"] >= 257 and seen["max_episode"] >= 1 and seen["visited"] > 0
