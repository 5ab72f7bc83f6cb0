"""T learn steps in one call on the host path (rmx_learn_run on a RMX_DEVICE_HOST handle behind
VecQLearning.run / VecQLambda.run): the reference's recorded runs one run per snapshot interval, run(T) against T
act_steps on a twin handle, mixed use, the Q(lambda) overflow, the refusals, the chunking above RMX_LEARN_RUN_MAX and
the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import learn_common as LC
import learn_run_common as RC
import policy_common as PC
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv
from rmx.learn import VecQLambda, VecQLearning
from test_learn_cpu import _lcfg, _raw


@pytest.mark.parametrize("kind,case", RC.GOLDEN_RUNS, ids=RC.GOLDEN_IDS)
def test_whole_runs_of_the_reference_through_run(kind, case):
    RC.replay_run(kind, case, HostRMEnv)


@pytest.mark.parametrize("wname,mode", RC.CASES, ids=RC.CASE_IDS)
def test_run_equals_single_steps_on_a_twin(wname, mode):
    RC.twin_case(HostRMEnv, HostRMEnv, wname, mode)  # the host runs the same T steps: the return sum is equal too


@pytest.mark.parametrize("mode", ["hash_qrm", "lambda"])
def test_mixed_use(mode):
    RC.mixed_use(HostRMEnv, mode, exact_stats=True)


def test_lambda_overflow_is_reported_as_by_single_steps():
    RC.overflow_case(HostRMEnv, exact_stats=True)


def test_refusals_of_the_raw_call():
    tab = T.compile_scenario(T.baseline_scenario(2))
    lib, h, keep = _raw(tab)
    INV, STATE = _capi.RMX_E_INVALID, _capi.RMX_E_STATE
    MAX = _capi.LEARN_RUN_MAX
    s_max = C.c_int64()
    assert lib.rmx_learn_states(h, C.byref(s_max)) == 0
    q = np.ones((2, 4, s_max.value, 4))

    def refused(code, word, *args, handle=h):
        assert lib.rmx_learn_run(handle, *args) == code
        msg = lib.rmx_last_error()
        assert msg and word.encode() in msg, msg

    good = (3, 0.1, 1, 0, 0, None, None)
    refused(STATE, "rmx_learn_bind", *good)  # before rmx_learn_bind
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(use_qrm=1)), q.ctypes.data, None) == 0
    refused(INV, "T must", 0, 0.1, 1, 0, 0, None, None)
    refused(INV, "T must", -1, 0.1, 1, 0, 0, None, None)
    refused(INV, "T must", MAX + 1, 0.1, 1, 0, 0, None, None)
    refused(INV, "epsilon", 3, 1.5, 1, 0, 0, None, None)
    refused(INV, "epsilon", 3, float("nan"), 1, 0, 0, None, None)
    for flags in (8, 1 | 8, 4 | 8, 16):
        refused(INV, "flags", 3, 0.1, flags, 0, 0, None, None)
    refused(STATE, "rmx_learn_rng_bind", 3, 0.1, 1 | 4, 0, 0, None, None)  # RMX_LEARN_NUMPY with no column
    refused(INV, "NULL", *good, handle=None)
    assert np.array_equal(q, np.ones_like(q))  # nothing was stepped
    out = np.full((3, 2, 4), -1, np.int32)
    assert lib.rmx_learn_run(h, 3, 0.1, 1, 0, 0, out.ctypes.data, None) == 0
    assert out.min() >= 0 and out.max() <= 3 and (q != 1.0).any()
    assert lib.rmx_learn_run(h, MAX, 0.1, 1, 0, 3, None, None) == 0  # the cap itself is served
    lib.rmx_destroy(h)
    lib, h2, keep2 = _raw(tab, bind=False)  # before rmx_bind
    assert lib.rmx_learn_bind(h2, C.byref(_lcfg()), q.ctypes.data, None) == 0
    refused(STATE, "rmx_bind", *good, handle=h2)
    lib.rmx_destroy(h2)


def test_python_run_checks_its_arguments():
    tab = T.compile_scenario(T.baseline_scenario(2))
    env = HostRMEnv(tab, 2)
    L = VecQLearning(env, 0.9, 0.1, use_qrm=True)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="T must"):
            L.run(bad, 0.1, 1, 0)
    with pytest.raises(ValueError, match="seed and t_global"):
        L.run(2, 0.1)
    with pytest.raises(RuntimeError, match="policy_seeds"):
        L.run(2, 0.1, reference_stream=True)
    with pytest.raises(ValueError, match="actions_out"):
        L.run(3, 0.1, 1, 0, actions_out=np.zeros((2, 2, 2), np.int32))  # too short for T = 3
    with pytest.raises(ValueError, match="epsilon"):
        L.run(2, 1.5, 1, 0)
    assert (L.visits == 0).all()
    env.close()


@pytest.mark.parametrize("mode", ["hash_qrm", "numpy_qrm"])
def test_a_run_above_the_cap_is_split_seamlessly(mode):
    """RMX_LEARN_RUN_MAX + 5 steps through run (two calls underneath: t_global and the actions_out offset advance)
    against that many single steps."""
    tab = T.compile_scenario(T.baseline_scenario(2))
    n = _capi.LEARN_RUN_MAX + 5
    Lx, Ly = RC.make_learner(HostRMEnv, tab, 2, mode), RC.make_learner(HostRMEnv, tab, 2, mode)
    ox, oy = RC.new_out(Lx, n), RC.new_out(Ly, n)
    Lx.run(n, RC.EPS, actions_out=ox, **RC.call_kw(mode))
    RC.run_steps(Ly, mode, n, out=oy)
    assert np.array_equal(ox, oy) and ox.min() >= 0
    RC.same_learners(Lx, Ly, ("split", mode), exact_stats=True)


def test_lambda_learner_inherits_run():
    assert VecQLambda.run is VecQLearning.run


def test_abi_stays_put():
    lib = _capi.load_library()
    assert lib.rmx_abi_version() == 12 and _capi.ABI_VERSION == 12
    assert "rmx_learn_run" in _capi.EXPORTS and callable(lib.rmx_learn_run)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "rmx.h")) as f:
        text = f.read()
    assert re.search(r"^int rmx_learn_run\(rmx_handle\* h, int32_t T, double epsilon, int flags, uint64_t seed, "
                     r"int64_t t_global,\s*int32_t\* actions_out[^;]*void\* hip_stream\);", text, re.M)
    m = re.search(r"^#define RMX_LEARN_RUN_MAX (\d+)", text, re.M)
    assert m and int(m.group(1)) == _capi.LEARN_RUN_MAX == 4096
    assert re.search(r"^#define RMX_ABI_VERSION 12\b", text, re.M)
    assert "rmx_learn_run.hip" in _capi.HASHED_SOURCES
