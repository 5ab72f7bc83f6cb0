"""The reference's own action stream on the device (the numpy instantiation of csrc/rmx_learn.hip behind
VecQLearning(policy_seeds=...).act_step(reference_stream=True) on a VecRMEnv): the recorded runs of the reference,
device against host bit for bit over a partial last block and the 8-agent bucket, the forced redraw, and the words
around the caller's column."""
import dataclasses

import numpy as np
import pytest

import learn_common as LC
import policy_common as PC
from rmx import tables as T
from rmx.engine import HostRMEnv, VecRMEnv
from rmx.learn import VecQLearning
from test_random_maps_gpu import random_tables

pytestmark = pytest.mark.gpu

FL, OW = T.FROZEN_LAKE, T.OFFICE_WORLD
CANARY = 0x5A5AC3C3A5A53C3C


@pytest.mark.parametrize("case", PC.EXPECTED)
def test_whole_runs_of_the_reference_on_the_device(case):
    PC.replay_fixture(case, VecRMEnv)


# N = 300: a full 256-thread block and a partial one whose last wave has a tail; A = 5: the 8-agent bucket, whose agents
# 5..7 own no column words.  max_t = 20 so that truncation and the auto-reset fall inside the run.
WORLDS = {
    "a3_n300": (lambda: random_tables(3, FL, 14, 14, 3, 5, 6, False), 300, 70),
    "a5_n70": (lambda: random_tables(11, FL, 8, 7, 5, 5, 8, False), 70, 70),
    "ow_a4_n65": (lambda: random_tables(2, OW, 12, 10, 4, 6, 7, True), 65, 60),
}


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_device_equals_host_bit_for_bit_with_canaries_around_the_column(name):
    import torch
    make, N, K = WORLDS[name]
    tab = dataclasses.replace(make(), max_t=20)
    A = tab.n_agents
    dev, hst = VecRMEnv(tab, N), HostRMEnv(tab, N)
    seeds = np.random.default_rng(A * N).integers(0, 2 ** 64, size=(A, N), dtype=np.uint64)
    kw = dict(qtable_init=0.25, use_qrm=True)
    Ld = VecQLearning(dev, 0.9, 0.3, policy_seeds=seeds, **kw)
    Lh = VecQLearning(hst, 0.9, 0.3, policy_seeds=seeds, **kw)
    assert np.array_equal(PC.words(Ld.rng), Lh.rng)  # the seeding
    # the device column again, inside a larger allocation: 16 words before it and 64 after it must stay the caller's
    n = 5 * A * N
    store = torch.full((16 + n + 64,), CANARY, dtype=torch.int64, device=dev.device)
    PC.bind_column(Ld, store[16:16 + n].view(5, A, N))
    PC.seed_column(Ld, seeds)
    assert np.array_equal(PC.words(Ld.rng), Lh.rng)
    out_d = torch.full((K, A, N), -1, dtype=torch.int32, device=dev.device)
    out_h = np.full((K, A, N), -1, np.int32)
    for t in range(K):
        best, learn = t % 11 == 10, t % 13 != 12
        if t % 9 == 8:  # actions_out = None
            Ld.act_step(0.2, reference_stream=True, best=best, learn=learn)
            Lh.act_step(0.2, reference_stream=True, best=best, learn=learn)
        else:
            Ld.act_step(0.2, reference_stream=True, best=best, learn=learn, actions_out=out_d[t])
            Lh.act_step(0.2, reference_stream=True, best=best, learn=learn, actions_out=out_h[t])
    assert np.array_equal(out_d.cpu().numpy(), out_h)
    assert (out_h[8] == -1).all() and set(out_h[:8].ravel().tolist()) == {0, 1, 2, 3}
    LC.assert_same_bits(Ld.q, Lh.q, (name, "q"))
    assert np.array_equal(LC.host(Ld.visits), Lh.visits)
    assert np.array_equal(PC.words(Ld.rng), Lh.rng)
    LC.assert_same_columns(LC.columns(dev), LC.columns(hst), name)
    w = PC.words(store)
    assert (w[:16] == CANARY).all() and (w[16 + n:] == CANARY).all()
    flags = Lh.rng[4] >> np.uint64(32)
    assert (Lh.visits > 0).any() and (hst.t < K).all() and flags.min() == 0 and flags.max() == 1
    dev.check_errors()
    dev.close()


def test_forced_redraw_on_the_device():
    import torch
    tab = T.compile_scenario(T.baseline_scenario(2))
    A, N = tab.n_agents, 130
    dev = VecRMEnv(tab, N)
    dev.reset(seed=1)
    L = VecQLearning(dev, 0.9, 0.2, use_qrm=True, policy_seeds=np.arange(A * N, dtype=np.uint64).reshape(A, N))
    L.rng[4] = 1 << 32  # a buffered half of 0 in every learner
    st = PC.states_to_leave(dev, tab)
    rows = torch.tensor([[0.5, 2.0, 2.0, 2.0], [3.0, 0.0, 3.0, 3.0]], dtype=torch.float64, device=dev.device)
    for a in range(A):
        L.q[a, torch.arange(N, device=dev.device), torch.as_tensor(st[a], device=dev.device)] = rows[a]
    # one learner handed over from a real Generator (set_rng_state on a device column), numpy itself as its reference
    g = np.random.default_rng(99)
    st = g.bit_generator.state
    st["has_uint32"], st["uinteger"] = 1, 0
    g.bit_generator.state = st
    L.set_rng_state(0, 129, st)
    assert L.rng_state(0, 129) == st
    g.uniform(0, 1)
    numpy_pick = int(g.choice([1, 2, 3]))
    want, after = PC.expect_step(L, 0.0)
    assert want[0, 129] == numpy_pick and L.rng_state(0, 128) != st
    out = torch.zeros((A, N), dtype=torch.int32, device=dev.device)
    L.act_step(0.0, reference_stream=True, learn=False, actions_out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(PC.words(L.rng), after)
    assert L.rng_state(0, 129) == g.bit_generator.state
    assert set(want[0].tolist()) == {1, 2, 3} and set(want[1].tolist()) == {0, 2, 3}
    assert (after[4] >> np.uint64(32) == 1).all()  # every learner redrew: 64 fresh bits, the high half buffered
    dev.check_errors()
    dev.close()
