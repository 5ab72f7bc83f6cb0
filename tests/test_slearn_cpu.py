"""The learn step on slip and random-start worlds (include/rmx.h RMX_LEARN_DYN_ENV; VecQLearning on an env built from a
stochastic or random-start scenario) on host handles: whole training runs recorded from the reference's QLearning on
the reference's own stochastic environments, the twin run against the plain step, the gate, a masked reset with a new
seed, sharding, and the host learn step as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import learn_common as LC
import slearn_common as SC
from rmx import _capi
from rmx import tables as T
from rmx.engine import HostRMEnv
from rmx.learn import VecQLearning
from test_learn_cpu import _lcfg, _raw
from test_random_maps_gpu import SLIP_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2 ** 64 - 1


def test_every_recorded_fixture_is_present():
    assert SC.FIXTURES == SC.EXPECTED


@pytest.mark.parametrize("case", SC.EXPECTED)
def test_whole_runs_of_the_reference_on_slip_and_random_start_worlds(case):
    draws, differing, resets, starts = (int(v) for v in SC.replay_fixture(case, HostRMEnv))
    # what the recorder asserted of the reference's run (the fixture really exercises what it is named for)
    N = {"ow2_allslip_qrm": 3}.get(case, 4)
    assert resets > N
    assert differing >= 100 if "slip" in case or "delay" in case else draws == 0
    assert starts >= {"fl2_randstart_slip_visits": 20, "fl2_randstart_qrm": 3}.get(case, 1)


# ---- the twin run: a learn step leaves the env as the plain step does ------------------------------------------------
@pytest.mark.parametrize("name", sorted(SLIP_CASES) + ["fl_slip_randstart"])
def test_learn_step_and_plain_step_leave_the_same_env(name):
    tab = SC.fl_slip_randstart_world() if name == "fl_slip_randstart" else SC.slip_world(name)
    seen = SC.twin_run(HostRMEnv, tab, 6, 60, seed=31, with_enc_state=True)
    assert seen["evaluated"] == 15 and seen["moved_rng"] >= 50  # the evaluation steps draw their slips too
    assert seen["episodes"] >= 6 and seen["max_episode"] >= 2 and seen["visited"] > 0


# ---- the gate --------------------------------------------------------------------------------------------------------
def test_the_gate():
    INV = _capi.RMX_E_INVALID
    assert (_capi.LEARN_DYN_FIXED, _capi.LEARN_DYN_ENV) == (0, 1)
    slip = T.compile_scenario(dict(T.baseline_scenario(2), stochastic=True))
    rand = T.compile_scenario(dict(T.baseline_scenario(2), random_start_positions=True))
    for tab in (slip, rand):
        lib, h, keep = _raw(tab, bind=False)
        assert lib.rmx_abi_version() == 12
        s_max = C.c_int64()
        assert lib.rmx_learn_states(h, C.byref(s_max)) == 0
        q = np.ones((2, 4, s_max.value, 4))
        # 0, and a zeroed word: the old refusal, word for word
        for cfg in (_lcfg(), _lcfg(dynamics=_capi.LEARN_DYN_FIXED)):
            assert lib.rmx_learn_bind(h, C.byref(cfg), q.ctypes.data, None) == INV
            assert lib.rmx_last_error() == (b"the learn step serves deterministic dynamics and fixed starts "
                                            b"(cfg.stochastic / cfg.random_starts are set)")
        for bad in (2, -1, 1 << 20):
            assert lib.rmx_learn_bind(h, C.byref(_lcfg(dynamics=bad)), q.ctypes.data, None) == INV
            assert b"dynamics" in lib.rmx_last_error()
        assert lib.rmx_learn_bind(h, C.byref(_lcfg(dynamics=_capi.LEARN_DYN_ENV)), q.ctypes.data, None) == 0
        lib.rmx_destroy(h)
    # a deterministic handle: 2 is refused all the same, 0 and 1 are both taken
    lib, h, keep = _raw(T.compile_scenario(T.baseline_scenario(2)), bind=False)
    s_max = C.c_int64()
    assert lib.rmx_learn_states(h, C.byref(s_max)) == 0
    q = np.ones((2, 4, s_max.value, 4))
    assert lib.rmx_learn_bind(h, C.byref(_lcfg(dynamics=2)), q.ctypes.data, None) == INV
    assert b"dynamics" in lib.rmx_last_error()
    for ok in (0, 1):
        assert lib.rmx_learn_bind(h, C.byref(_lcfg(dynamics=ok)), q.ctypes.data, None) == 0
    lib.rmx_destroy(h)
    assert C.sizeof(_capi.RmxLearnConfig) == 40 and _capi.RmxLearnConfig.dynamics.offset == 28  # the layout of ABI 12


def test_dynamics_env_on_a_deterministic_handle_replays_a_learn_fixture(monkeypatch):
    bound = []

    class Spy(_capi.RmxLearnConfig):
        def __setattr__(self, k, v):
            if k == "dynamics":
                bound.append(v)
            super().__setattr__(k, v)

    monkeypatch.setattr(_capi, "RmxLearnConfig", Spy)
    LC.replay_fixture("fl2_qrm", HostRMEnv, lambda a: a)
    assert bound == [_capi.LEARN_DYN_ENV]  # VecQLearning asked for the env's dynamics


# ---- a masked reset with a new seed, mid-run -------------------------------------------------------------------------
def _numpy_words(seed):
    st = np.random.default_rng(seed).bit_generator.state["state"]
    return [st["state"] >> 64, st["state"] & M64, st["inc"] >> 64, st["inc"] & M64]


def test_masked_reset_with_a_new_seed_mid_run():
    tab = SC.slip_world("fl_slip_delay")
    N, A = 9, tab.n_agents
    x, y = HostRMEnv(tab, N), HostRMEnv(tab, N)
    x.reset(seed=5)
    y.reset(seed=5)
    L = VecQLearning(x, 0.9, None, qtable_init=0.5, policy_seeds=3)
    out = np.zeros((A, N), np.int32)

    def run(k):
        for _ in range(k):
            L.act_step(0.3, reference_stream=True, actions_out=out)
            y.step(out)
            LC.assert_same_columns(SC.env_columns(x), SC.env_columns(y), "twin")

    run(45)
    assert x.episode.min() >= 1  # every env has been reseeded inside the run
    q0, v0, col0, ep0, rng0 = L.q.copy(), L.visits.copy(), L.rng.copy(), x.episode.copy(), x.rng.copy()
    mask = np.zeros(N, np.uint8)
    mask[::2] = 1
    x.reset(mask=mask, seed=77)
    y.reset(mask=mask, seed=77)
    m = mask.astype(bool)
    # the tables and the learners' generators are the caller's: a reset of the env does not touch them
    LC.assert_same_bits(L.q, q0, "q")
    LC.assert_same_bits(L.visits, v0, "visits")
    assert np.array_equal(L.rng, col0)
    # the reset envs restart the schedule at episode 0 of the new seed, the others keep generator and count
    assert (x.episode[m] == 0).all() and np.array_equal(x.episode[~m], ep0[~m]) and np.array_equal(x.rng[:, ~m], rng0[:, ~m])
    scale, es, ks = tab.seed_schedule
    for e in np.flatnonzero(m):
        assert [int(v) for v in x.rng[:, e]] == _numpy_words((77 * scale + int(e) * es) & M64), e
    assert (x.t[m] == 0).all()
    run(45)
    assert x.episode[m].min() >= 1 and (L.visits > v0).any()
    LC.assert_same_columns(SC.env_columns(x), SC.env_columns(y), "end")


# ---- shards ----------------------------------------------------------------------------------------------------------
def test_two_shards_equal_the_whole_on_a_slip_world():
    tab = SC.slip_world("ow_slip_walls_fail")
    A, N, K = tab.n_agents, 6, 70
    kw = dict(qtable_init=0.5, use_qrm=True)
    whole = HostRMEnv(tab, N)
    halves = [HostRMEnv(tab, 3, env_offset=o, n_envs_global=N) for o in (0, 3)]
    for env in [whole] + halves:
        env.reset(seed=12)
    Lw = VecQLearning(whole, 0.9, 0.3, **kw)
    Lh = [VecQLearning(h, 0.9, 0.3, **kw) for h in halves]
    ow, oh = np.zeros((A, N), np.int32), [np.zeros((A, 3), np.int32) for _ in range(2)]
    for t in range(K):
        Lw.act_step(0.2, 9, t, actions_out=ow)
        for L, o in zip(Lh, oh):
            L.act_step(0.2, 9, t, actions_out=o)
        assert np.array_equal(ow, np.concatenate(oh, axis=1)), t
    assert np.array_equal(LC.bits(Lw.q), LC.bits(np.concatenate([L.q for L in Lh], axis=1)))
    assert np.array_equal(Lw.visits, np.concatenate([L.visits for L in Lh], axis=1))
    cw, ch = SC.env_columns(whole), [SC.env_columns(h) for h in halves]
    for n in cw:
        got = np.concatenate([c[n] for c in ch], axis=cw[n].ndim - 1)
        assert np.array_equal(cw[n].view(np.uint32) if cw[n].dtype.kind == "f" else cw[n],
                              got.view(np.uint32) if got.dtype.kind == "f" else got), n
    assert (Lw.visits > 0).any() and whole.episode.max() >= 2


# ---- the host learn step on a slip + random-start world as a stand-alone program under ASan + UBSan -----------------
SAN_N, SAN_STEPS, SAN_SEED = 7, 120, 21


def _san_world():
    return SC.fl_slip_randstart_world(seed=4, W=5, H=4, A=3, Q=3, n_ev=3, max_t=12)


def _fnv(d, arr):
    for b in np.ascontiguousarray(arr).view(np.uint8).ravel().tolist():
        d = ((d ^ b) * 0x100000001b3) & M64
    return d


def _san_expected(tab):
    """slearn_host_main.cpp's sequence on a HostRMEnv."""
    env = HostRMEnv(tab, SAN_N, with_qrm=True, with_enc_state=True)
    env.reset(seed=SAN_SEED)
    A = tab.n_agents
    seeds = (np.arange(A * SAN_N, dtype=np.uint64) * np.uint64(7919) + np.uint64(1)).reshape(A, SAN_N)
    L = VecQLearning(env, 0.9, None, qtable_init=0.5, use_qrm=True, policy_seeds=seeds)
    out = np.zeros((A, SAN_N), np.int32)
    for s in range(SAN_STEPS):
        best, learn = s % 11 == 10, s % 13 != 12
        if s % 3 == 0:
            L.step(((np.arange(A * SAN_N, dtype=np.int64) + s) % 4).astype(np.int32).reshape(A, SAN_N))
        elif s % 3 == 1:
            L.act_step(0.25, SAN_SEED, s, best=best, learn=learn, actions_out=out)
        else:
            L.act_step(0.25, reference_stream=True, best=best, learn=learn, actions_out=out)
    d = 0xcbf29ce484222325
    for arr in (L.q, L.visits, L.rng, env.rng, env.episode, env.pos_x, env.pos_y, env.rm_q, env.t):
        d = _fnv(d, arr)
    assert env.episode.max() >= 3 and (L.visits > 0).any()
    return d


def test_host_learn_step_on_a_slip_world_clean_under_asan_ubsan(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler for the sanitizer build")
    tab = _san_world()
    assert tab.stochastic and tab.random_starts
    cfg, keep = _capi.make_config(tab, SAN_N, device=_capi.DEVICE_HOST)
    order = ("cell", "cell_event", "next_q", "rm_reward", "init_q", "final_q", "start_xy", "n_qrm", "qrm_states", "enc_nq")
    assert "shape" not in keep and all(k in keep for k in order)
    world = tmp_path / "world.bin"
    world.write_bytes(bytes(cfg) + b"".join(keep[k].tobytes() for k in order))
    csrc = os.path.join(ROOT, "multiagent-rl-rm_amd", "csrc")
    exe = str(tmp_path / "slearn_host_main")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    "-I", csrc, "-o", exe, os.path.join(ROOT, "tests", "data", "slearn_host_main.cpp"),
                    os.path.join(csrc, "rmx_hoststep.cpp"), os.path.join(csrc, "rmx_tables.cpp")], check=True)
    # the sanitizer runtimes are linked statically: the program does not depend on what the environment preloads
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(world), str(SAN_STEPS), str(SAN_SEED)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    got = next(ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("SLEARN_HOST_DIGEST"))
    assert int(got, 16) == _san_expected(tab)
