"""Per-learner epsilon schedules on the host path (rmx_learn_eps_bind / rmx_learn_eps_decay on a RMX_DEVICE_HOST handle
behind VecQLearning(epsilon_start=...)): the reference's recorded runs with its per-episode decay step by step and
through run, run(T) against T act_steps, a constant column against the scalar epsilon, per-learner values, sharding,
where the column moves and where it must not, Q(lambda), the refusals and the ABI."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

import eps_common as EC
import learn_common as LC
import learn_run_common as RC
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv
from rmx.learn import VecQLambda, VecQLearning
from test_learn_cpu import _lcfg, _raw
from test_random_maps_gpu import random_tables


def test_every_recorded_case_is_there():
    for case in EC.EXPECTED:
        assert os.path.exists(os.path.join(LC.GOLDEN, f"eps_{case}.npz")), case


@pytest.mark.parametrize("case", EC.EXPECTED)
def test_whole_runs_of_the_reference_step_by_step(case):
    EC.replay(case, HostRMEnv, through_run=False)


@pytest.mark.parametrize("case", EC.EXPECTED)
def test_whole_runs_of_the_reference_through_run(case):
    EC.replay(case, HostRMEnv, through_run=True)


@pytest.mark.parametrize("wname,mode", EC.TWIN_CASES, ids=EC.TWIN_IDS)
def test_run_equals_single_steps_on_a_twin(wname, mode):
    tab, N = EC.world(wname)
    EC.twin(HostRMEnv, HostRMEnv, tab, N, mode)


@pytest.mark.parametrize("mode", EC.TWIN_MODES)
def test_a_run_above_the_cap_carries_the_column_across_launches(mode):
    tab = dataclasses.replace(random_tables(3, T.FROZEN_LAKE, 14, 14, 3, 5, 6, False), max_t=12)
    n = _capi.LEARN_RUN_MAX + 5
    EC.twin(HostRMEnv, HostRMEnv, tab, 3, mode, n=n, split=(n,))


@pytest.mark.parametrize("mode", ["plain_visits", "hash_qrm", "numpy_qrm", "lambda"])
def test_a_constant_column_is_the_scalar_path(mode):
    EC.constant_column_case(HostRMEnv, mode)


@pytest.mark.parametrize("mode", EC.TWIN_MODES)
def test_each_learner_explores_under_its_own_epsilon(mode):
    EC.per_learner_case(HostRMEnv, mode)


def test_column_values_are_not_validated():
    EC.odd_values_case(HostRMEnv)


def test_a_sharded_job_leaves_each_shard_its_slice_of_the_column():
    """The engine's policy hashes the global env index: two shards of three envs (env_offset) end with the columns,
    tables and actions of envs 0..2 and 3..5 of the unsharded handle."""
    tab, _ = EC.world("a5_n70")
    A, N, n = tab.n_agents, 6, 80
    start = np.random.default_rng(8).uniform(0.2, 1.0, size=(A, N))
    whole = EC.make_learner(HostRMEnv, tab, N, "hash_qrm")
    EC.set_column(whole, start)
    ow = RC.new_out(whole, n)
    EC.advance(whole, "hash_qrm", n, ow, True, split=(30, 50))
    assert (EC.column(whole) < start).any()
    for off in (0, 3):
        shard = EC.make_learner(HostRMEnv, tab, 3, "hash_qrm", env_offset=off, n_envs_global=N)
        EC.set_column(shard, start[:, off:off + 3])
        os_ = RC.new_out(shard, n)
        EC.advance(shard, "hash_qrm", n, os_, False)
        assert np.array_equal(os_, ow[:, :, off:off + 3]), off
        LC.assert_same_bits(shard.epsilon, EC.column(whole)[:, off:off + 3], ("shard column", off))
        LC.assert_same_bits(shard.q, whole.q[:, off:off + 3], ("shard q", off))
        shard.env.close()
    whole.env.close()


def test_where_the_column_moves_and_where_it_does_not():
    EC.lifecycle_case(HostRMEnv)


def test_lambda_learners_with_a_decaying_column():
    tab, N = EC.world("a5_n70")
    EC.twin(HostRMEnv, HostRMEnv, tab, N, "lambda", n=120, split=(1, 70, 49))
    assert VecQLambda.learn_done_episode is VecQLearning.learn_done_episode


def test_unbinding_rebinding_and_a_new_learner():
    EC.rebind_case(HostRMEnv)


def test_python_arguments():
    tab = T.compile_scenario(T.baseline_scenario(2))
    env = HostRMEnv(tab, 2)
    for kw in (dict(epsilon_end=0.1), dict(epsilon_decay=0.9)):
        with pytest.raises(ValueError, match="epsilon_start"):
            VecQLearning(env, 0.9, 0.1, **kw)
    L = VecQLearning(env, 0.9, 0.1, epsilon_start=0.7)
    assert (L.epsilon == 0.7).all() and L.epsilon.dtype == np.float64 and L.epsilon.shape == (2, 2)
    assert (L.epsilon_end, L.epsilon_decay) == (0.7, 1.0)  # the defaults: a schedule that stays where it starts
    L.learn_done_episode()
    assert (L.epsilon == 0.7).all()
    for bad in (dict(epsilon_end=1.5), dict(epsilon_end=-0.1), dict(epsilon_decay=1.01), dict(epsilon_decay=float("nan"))):
        with pytest.raises(ValueError, match="eps_end|eps_decay"):
            VecQLearning(env, 0.9, 0.1, epsilon_start=0.5, **bad)
    M = VecQLambda(env, 0.9, 0.8, 0.1, epsilon_start=1.0, epsilon_end=0.2, epsilon_decay=0.5)
    M.learn_done_episode()
    assert (M.epsilon == 0.5).all() and M.trace_cnt is not None
    env.close()


def test_refusals_of_the_raw_calls():
    tab = T.compile_scenario(T.baseline_scenario(2))
    lib, h, keep = _raw(tab)
    INV, STATE = _capi.RMX_E_INVALID, _capi.RMX_E_STATE
    s_max = C.c_int64()
    assert lib.rmx_learn_states(h, C.byref(s_max)) == 0
    q = np.ones((2, 4, s_max.value, 4))
    store = np.full(2 * 4 + 1, 0.5)
    col = store[:8]
    assert col.ctypes.data % 8 == 0

    def refused(code, word, fn, *args):
        assert fn(*args) == code, (fn.__name__, args)
        msg = lib.rmx_last_error()
        assert msg and word.encode() in msg, msg

    bind, decay = lib.rmx_learn_eps_bind, lib.rmx_learn_eps_decay
    refused(STATE, "rmx_learn_bind", bind, h, col.ctypes.data, 0.1, 0.9)  # before rmx_learn_bind
    refused(STATE, "rmx_learn_bind", decay, h, None, None)
    refused(INV, "NULL", bind, None, col.ctypes.data, 0.1, 0.9)
    refused(INV, "NULL", decay, None, None, None)
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(use_qrm=1)), q.ctypes.data, None) == 0
    refused(STATE, "rmx_learn_eps_bind", decay, h, None, None)  # no column bound
    refused(INV, "aligned", bind, h, col.ctypes.data + 4, 0.1, 0.9)
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        refused(INV, "eps_end", bind, h, col.ctypes.data, bad, 0.9)
    for bad in (-0.01, 1.01, float("nan"), float("inf"), float("-inf")):
        refused(INV, "eps_decay", bind, h, col.ctypes.data, 0.1, bad)
    refused(STATE, "rmx_learn_eps_bind", decay, h, None, None)  # a refused bind bound nothing
    for end, dec in ((0.0, 0.0), (1.0, 1.0), (0.1, 0.9)):  # the ends of both ranges are served
        assert bind(h, col.ctypes.data, end, dec) == 0
    assert decay(h, None, None) == 0
    assert (col == 0.45).all() and store[8] == 0.5
    # the scalar is validated as ever and otherwise ignored; flag 8 is still no flag
    assert lib.rmx_learn_step_policy(h, 1.5, 1, 0, 0, 1, None, None) == INV and b"epsilon" in lib.rmx_last_error()
    assert lib.rmx_learn_run(h, 2, float("nan"), 1, 0, 0, None, None) == INV and b"epsilon" in lib.rmx_last_error()
    assert lib.rmx_learn_step_policy(h, 0.1, 8, 0, 0, 1, None, None) == INV and b"flags" in lib.rmx_last_error()
    col[:] = 0.0
    out = np.full((2, 4), -1, np.int32)
    assert lib.rmx_learn_step_policy(h, 1.0, 1, 7, 0, 1, out.ctypes.data, None) == 0  # column 0.0: nobody explores
    greedy = out.copy()
    lib2, h2, keep2 = _raw(tab)
    q2 = np.ones_like(q)
    assert lib.rmx_learn_bind(h2, C.byref(_lcfg(use_qrm=1)), q2.ctypes.data, None) == 0
    assert lib.rmx_learn_step_policy(h2, 0.0, 1, 7, 0, 1, out.ctypes.data, None) == 0
    assert np.array_equal(out, greedy)
    # NULL unbinds (eps_end / eps_decay are not looked at); rmx_learn_bind drops a binding
    assert bind(h, None, 7.0, float("nan")) == 0
    refused(STATE, "rmx_learn_eps_bind", decay, h, None, None)
    assert bind(h, col.ctypes.data, 0.1, 0.9) == 0 and decay(h, None, None) == 0
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(use_qrm=1)), q.ctypes.data, None) == 0
    refused(STATE, "rmx_learn_eps_bind", decay, h, None, None)
    lib.rmx_destroy(h)
    lib.rmx_destroy(h2)


def test_abi_and_documents():
    lib = _capi.load_library()
    assert lib.rmx_abi_version() == _capi.ABI_VERSION
    for name in ("rmx_learn_eps_bind", "rmx_learn_eps_decay"):
        assert name in _capi.EXPORTS and callable(getattr(lib, name))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "rmx.h")) as f:
        text = f.read()
    assert re.search(r"^int rmx_learn_eps_bind\(rmx_handle\* h, double\* eps.*double eps_end, double eps_decay\);$", text,
                     re.M)
    assert re.search(r"^int rmx_learn_eps_decay\(rmx_handle\* h, const uint8_t\* env_mask.*void\* hip_stream\);$", text,
                     re.M)
    assert "never call learn_done_episode" not in text
    docs = {"include/rmx.h": text}
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md", os.path.join("multiagent-rl-rm_amd", "rmx", "learn.py")):
        with open(os.path.join(root, rel)) as f:
            docs[rel] = f.read()
    for rel, body in docs.items():  # no document still lists epsilon decay as not reproduced
        for m in re.finditer(r"[Nn]ot\s+reproduced:[^.]*\.", body):
            assert "epsilon" not in m.group(0), (rel, m.group(0))
        assert "rmx_learn_eps_bind" in body or "epsilon_start" in body, rel
    assert "4.10.5" in docs["DESIGN.md"]
    for name in ("rmx_learn_eps.hip", "rmx_learn_run_eps.hip"):
        assert name in _capi.HASHED_SOURCES
