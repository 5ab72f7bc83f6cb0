"""T learn steps in ONE launch on the device (learn_run_kernel, csrc/rmx_learn_run.hip, behind VecQLearning.run /
VecQLambda.run on a VecRMEnv): the reference's recorded runs one run per snapshot interval, run(T) against T
act_steps on a twin handle, device against host, the words around the caller's arrays, the Q(lambda) overflow and
mixed use."""
import numpy as np
import pytest

import learn_common as LC
import learn_run_common as RC
import policy_common as PC
from rmx.engine import HostRMEnv, VecRMEnv

pytestmark = pytest.mark.gpu

CANARY = 0x5A5AC3C3A5A53C3C
CANARY32 = 0x5A5AC3C3


@pytest.mark.parametrize("kind,case", RC.GOLDEN_RUNS, ids=RC.GOLDEN_IDS)
def test_whole_runs_of_the_reference_through_run(kind, case):
    RC.replay_run(kind, case, VecRMEnv)


@pytest.mark.parametrize("wname,mode", RC.CASES, ids=RC.CASE_IDS)
def test_run_equals_single_steps_on_a_twin(wname, mode):
    # one launch sums the returns per lane over the run, then per wave: the return sum by the rollout's rule
    RC.twin_case(VecRMEnv, VecRMEnv, wname, mode, exact_stats=False)


@pytest.mark.parametrize("wname,mode", RC.CASES, ids=RC.CASE_IDS)
def test_device_run_equals_host_run(wname, mode):
    RC.twin_case(VecRMEnv, HostRMEnv, wname, mode, x_runs=True, y_runs=True, exact_stats=False)


@pytest.mark.parametrize("mode", ["hash_qrm", "lambda"])
def test_mixed_use(mode):
    RC.mixed_use(VecRMEnv, mode, exact_stats=False)


def _guarded(torch, dev, shape, dtype, canary, fill, before=16, after=64):
    """A tensor of `shape` (filled with `fill`) inside a larger allocation of canaries, and that allocation."""
    n = int(np.prod(shape))
    store = torch.full((before + n + after,), canary, dtype=dtype, device=dev)
    view = store[before:before + n].view(*shape)
    if fill is not None:
        view.fill_(fill)
    return view, store


def _intact(store, n, canary, before=16):
    w = store.cpu()
    return bool((w[:before] == canary).all() and (w[before + n:] == canary).all())


def _guard_traces(torch, L, cap):
    """L's three trace arrays again as views inside canaries (the lists empty); returns the check."""
    env = L.env
    A, N = env.A, env.N
    idx, s_idx = _guarded(torch, env.device, (A, cap, N), torch.int32, CANARY32, 0)
    val, s_val = _guarded(torch, env.device, (A, cap, N), torch.float64, 1.5, 0.0)
    cnt, s_cnt = _guarded(torch, env.device, (A, N), torch.int32, CANARY32, 0)
    L.bind_traces(idx, val, cnt, cap)

    def check():
        assert _intact(s_idx, A * cap * N, CANARY32) and _intact(s_val, A * cap * N, 1.5)
        assert _intact(s_cnt, A * N, CANARY32)
    return check


def test_nothing_outside_the_callers_arrays_is_touched():
    """N = 65 (one wave and one lane of the next), A = 5 (the 8-agent bucket: agents 5..7 own nothing)."""
    import torch
    tab, _ = RC.world("a5_n70")
    N, A, K = 65, tab.n_agents, 30
    L = RC.make_learner(VecRMEnv, tab, N, "lambda")
    dev = L.env.device
    col, s_col = _guarded(torch, dev, (5, A, N), torch.int64, CANARY, 0)
    PC.bind_column(L, col)
    PC.seed_column(L, RC.seeds_for(tab, N))
    check_traces = _guard_traces(torch, L, L.trace_cap)
    out, s_out = _guarded(torch, dev, (K, A, N), torch.int32, CANARY32, -1)
    L.run(K, RC.EPS, reference_stream=True, actions_out=out)
    got = out.cpu().numpy()
    assert got.min() >= 0 and got.max() <= 3
    assert _intact(s_out, K * A * N, CANARY32) and _intact(s_col, 5 * A * N, CANARY)
    check_traces()
    assert (LC.host(L.visits) > 0).any() and int(L.trace_counts().max()) > 1
    # actions_out = None: nothing is written
    L.run(K, RC.EPS, reference_stream=True)
    assert np.array_equal(out.cpu().numpy(), got) and _intact(s_out, K * A * N, CANARY32)
    # best under the numpy stream draws nothing: the generator column is untouched
    before = PC.words(s_col).copy()
    L.run(K, RC.EPS, reference_stream=True, best=True, actions_out=out)
    assert np.array_equal(PC.words(s_col), before)
    assert _intact(s_out, K * A * N, CANARY32)
    check_traces()
    L.env.check_errors()
    L.env.close()


def test_lambda_overflow_is_reported_as_by_single_steps():
    """The bound arrays end at slot cap of the last agent: canaries behind them."""
    import torch
    made = []

    def rebind(L, cap):
        made.append(_guard_traces(torch, L, cap))
        return made[-1]
    RC.overflow_case(VecRMEnv, exact_stats=False, rebind=rebind)
    assert len(made) == 2
