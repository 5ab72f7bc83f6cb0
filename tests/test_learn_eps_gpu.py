"""Per-learner epsilon schedules on the device (the EPS instantiations of learn_step_kernel and learn_run_kernel,
csrc/rmx_learn_eps.hip / rmx_learn_run_eps.hip, and eps_decay_kernel, behind VecQLearning(epsilon_start=...) on a
VecRMEnv): the reference's recorded runs with its per-episode decay step by step and through run, run(T) against T
act_steps, device against host, a constant column against the scalar epsilon, per-learner values, where the column
moves and where it must not, Q(lambda), the words around the caller's column and the refusals."""
import dataclasses

import numpy as np
import pytest

import eps_common as EC
import learn_common as LC
import learn_run_common as RC
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv, VecRMEnv
from test_random_maps_gpu import random_tables

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", EC.EXPECTED)
def test_whole_runs_of_the_reference_step_by_step(case):
    EC.replay(case, VecRMEnv, through_run=False)


@pytest.mark.parametrize("case", EC.EXPECTED)
def test_whole_runs_of_the_reference_through_run(case):
    EC.replay(case, VecRMEnv, through_run=True)


@pytest.mark.parametrize("wname,mode", EC.TWIN_CASES, ids=EC.TWIN_IDS)
def test_run_equals_single_steps_on_a_twin(wname, mode):
    # one launch sums the returns per lane over the run, then per wave: the return sum by the rollout's rule
    tab, N = EC.world(wname)
    EC.twin(VecRMEnv, VecRMEnv, tab, N, mode, exact_stats=False)


@pytest.mark.parametrize("mode", EC.TWIN_MODES)
def test_a_run_above_the_cap_carries_the_column_across_launches(mode):
    tab = dataclasses.replace(random_tables(3, T.FROZEN_LAKE, 14, 14, 3, 5, 6, False), max_t=12)
    n = _capi.LEARN_RUN_MAX + 5
    EC.twin(VecRMEnv, VecRMEnv, tab, 3, mode, n=n, split=(n,), exact_stats=False)


@pytest.mark.parametrize("wname,mode", EC.TWIN_CASES, ids=EC.TWIN_IDS)
def test_device_equals_host(wname, mode):
    tab, N = EC.world(wname)
    EC.twin(VecRMEnv, HostRMEnv, tab, N, mode, x_runs=True, y_runs=True, exact_stats=False)


@pytest.mark.parametrize("wname", list(EC.WORLDS))
def test_device_steps_equal_host_steps(wname):
    tab, N = EC.world(wname)
    EC.twin(VecRMEnv, HostRMEnv, tab, N, "numpy_qrm", n=120, x_runs=False, y_runs=False, exact_stats=True)


@pytest.mark.parametrize("mode", ["plain_visits", "hash_qrm", "numpy_qrm", "lambda"])
def test_a_constant_column_is_the_scalar_path(mode):
    EC.constant_column_case(VecRMEnv, mode)


@pytest.mark.parametrize("mode", EC.TWIN_MODES)
def test_each_learner_explores_under_its_own_epsilon(mode):
    EC.per_learner_case(VecRMEnv, mode)


def test_column_values_are_not_validated():
    EC.odd_values_case(VecRMEnv)


def test_where_the_column_moves_and_where_it_does_not():
    EC.lifecycle_case(VecRMEnv)


def test_slip_and_random_start_worlds_with_a_decaying_column():
    """The STOCH kernels (the env's own generator and the episode column) with a schedule: run against steps, and the
    device run against the host's."""
    import slearn_common as SC
    tab = dataclasses.replace(SC.fl_slip_randstart_world(), max_t=12)
    EC.twin(VecRMEnv, VecRMEnv, tab, 65, "hash_qrm", n=120, split=(1, 70, 49), exact_stats=False)
    EC.twin(VecRMEnv, HostRMEnv, tab, 65, "numpy_qrm", n=120, split=(1, 70, 49), x_runs=True, y_runs=True,
            exact_stats=False)


def test_lambda_learners_with_a_decaying_column():
    tab, N = EC.world("a5_n70")
    EC.twin(VecRMEnv, VecRMEnv, tab, N, "lambda", n=120, split=(1, 70, 49), exact_stats=False)
    EC.twin(VecRMEnv, HostRMEnv, tab, N, "lambda", n=120, split=(1, 70, 49), x_runs=True, y_runs=True,
            exact_stats=False)


def test_unbinding_rebinding_and_a_new_learner():
    """With the caller's own column as a view inside a larger allocation: nothing around it is written."""
    EC.rebind_case(VecRMEnv)


def test_refusals_on_a_device_handle():
    import torch
    tab, N = EC.world("a5_n70")
    env = VecRMEnv(tab, N)
    lib, h = env.lib, env._h
    INV, STATE = _capi.RMX_E_INVALID, _capi.RMX_E_STATE
    col = torch.full((tab.n_agents * N + 1,), 0.5, dtype=torch.float64, device=env.device)

    def refused(code, word, fn, *args):
        assert fn(*args) == code, (fn.__name__, args)
        msg = lib.rmx_last_error()
        assert msg and word.encode() in msg, msg

    bind, decay = lib.rmx_learn_eps_bind, lib.rmx_learn_eps_decay
    refused(STATE, "rmx_learn_bind", bind, h, col.data_ptr(), 0.1, 0.9)
    refused(STATE, "rmx_learn_bind", decay, h, None, None)
    L = RC.make_learner(VecRMEnv, tab, N, "hash_qrm")
    h = L.env._h
    refused(STATE, "rmx_learn_eps_bind", decay, h, None, None)
    refused(INV, "aligned", bind, h, col.data_ptr() + 4, 0.1, 0.9)
    refused(INV, "eps_end", bind, h, col.data_ptr(), 1.5, 0.9)
    refused(INV, "eps_decay", bind, h, col.data_ptr(), 0.1, float("nan"))
    refused(STATE, "rmx_learn_eps_bind", decay, h, None, None)
    assert bind(h, col.data_ptr(), 0.1, 0.5) == 0 and decay(h, None, None) == 0
    env.sync_end()
    torch.cuda.synchronize()
    w = col.cpu().numpy()
    assert (w[:-1] == 0.25).all() and w[-1] == 0.5  # the word behind the column is not the column's
    L.env.check_errors()
    L.env.close()
    env.close()
