"""The resident workgroup behind rmx_reset_sync / rmx_step_sync / rmx_step_sync_begin + rmx_sync_wait
(csrc/rmx_sync.hip, driven by sync_setup / sync_begin / sync_copy_out in csrc/rmx_capi_sync.cpp) and mdp_kernel at the
engine's limits.

What only this path has, and where it is put under test here:
* the 16-byte request word: 15 actions in 4-bit fields, slots 0..6 in the ctl word and 7..14 in the acts word, the
  action array from 16 actions on (REQUEST_SHAPES: N * A in {7, 8, 12, 14, 15, 16} through different (A, N), every slot
  taking every action value, wait included; every slot x every invalid value, 16 and 20 among them);
* the 32-byte output records (x | y << 16, rm_q, flags, reward / renv, ep_ret, shaping, enc_state) at W = 4,096,
  H = 255, rm_q = 249 and with shaping, every column compared;
* its instantiations: the agent buckets 1 / 2 / 3 / 4 / 8 (the 8-bucket at A = 5, 7 and 8 with its runtime a < A guards
  in the load, step, store and write-back loops) x slip / random starts x QRM (249 counterfactuals through the
  mailbox, N up to 256);
* its static LDS on top of the 65,344-byte table blob;
* the write-back to the device columns: after sync_end, across the 30-us idle timeout, in one-launch-per-call mode;
* the two-halves form and its error contract; the dict API with 8 agents at N = 1.

The drivers, worlds and comparison rules are tests/test_sync_limits_cpu.py's (which runs them on host handles);
tests/LIMITS.md has the table of shapes and instantiations."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import test_limits_gpu as L
import test_sync_limits_cpu as S
from rmx import _capi
from rmx import tables as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    assert _t.cuda.is_available(), "gpu tests need a ROCm device"
    return _t


def device_engine(tab, n, **kw):
    from rmx.engine import VecRMEnv
    return VecRMEnv(tab, n, with_enc_state=True, **kw)


def to_device(torch):
    return lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def stream_of(env):
    return env._stream()


# ---- A. the request word --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,N", S.REQUEST_SHAPES)
def test_request_word_shapes(A, N, configs, torch):
    """60 steps with autoreset at each shape of the request: every slot takes every action value (asserted on the
    actions), every column after every step equals the oracle's and an asynchronous handle's."""
    tab = S.shape_tables(A, configs, N)
    acts = S.request_actions(tab, N)
    S.run_sync(device_engine, tab, acts, S.oracle_record(tab, acts), to_async=to_device(torch))


@pytest.mark.parametrize("A,N", S.INVALID_SHAPES)
def test_invalid_actions_in_every_slot(A, N, configs, torch):
    """15 actions inline (every nibble of both words) and 16 on the action array: each slot x {5, 15, 16, 20, -1,
    2^31 - 1} is a reported error, stepped as wait, never as its low nibble."""
    S.run_invalid_actions(device_engine, S.shape_tables(A, configs), N, to_async=to_device(torch))


# ---- B. limit worlds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,N", S.WORLD_RUNS)
def test_limit_worlds_through_the_resident_workgroup(case, N, torch):
    tab, acts, ref = S.world_reference(case, N)
    S.run_sync(device_engine, tab, acts, ref, to_async=to_device(torch))


@pytest.mark.parametrize("case", S.RNG_RUNS)
def test_rng_worlds_through_the_resident_workgroup(case, torch):
    """STOCH instantiations at the limits (the 8-bucket's slip and random_starts<8> among them) with a reset_sync to a
    new seed in mid-run; the rng and episode columns written back at sync_end are the oracle's."""
    tab, acts, ref = S.rng_world_reference(case)
    S.run_sync(device_engine, tab, acts, ref, seed=31, reseed=S.RESEED, to_async=to_device(torch))


def test_blob_limit_world_launches(torch):
    """65,344 B of dynamic LDS plus the resident kernel's static words: it launches and equals the oracle."""
    tab, acts, ref = S.blob_limit_reference()
    S.run_sync(device_engine, tab, acts, ref, to_async=to_device(torch))


@pytest.mark.parametrize("mode,case", [("idle", "a8_fl_slip"), ("launch", "a8_fl_randstart")])
def test_relaunch_paths_of_the_eight_agent_bucket(mode, case, torch, monkeypatch):
    """idle: a 30-us idle timeout and short pauses, so the workgroup writes its state back and a new one reloads it
    between requests; launch: one launch per call.  Both with the rng columns of an 8-agent world in the hand-over."""
    monkeypatch.setenv(*(("RMX_SYNC_IDLE_US", "30") if mode == "idle" else ("RMX_SYNC", "launch")))
    tab, acts, ref = S.rng_world_reference(case)
    pause = np.random.default_rng(6)

    def between(s):
        if mode == "idle" and s % 7 == 3:
            time.sleep(pause.uniform(0, 2e-4))

    S.run_sync(device_engine, tab, acts, ref, seed=31, reseed=S.RESEED, to_async=to_device(torch), between=between)


# ---- C. QRM columns through the mailbox -----------------------------------------------------------------------------
@pytest.mark.parametrize("case,N,steps", S.QRM_RUNS)
def test_qrm_columns_through_the_mailbox(case, N, steps, torch):
    tab, acts, ref = S.qrm_reference(case, N, steps)
    S.run_sync(device_engine, tab, acts, ref, qrm=True, to_async=to_device(torch))


@pytest.mark.parametrize("name", ["fl1_qrm16", "fl1_qrm17"])
def test_qrm_goldens_through_the_mailbox(name, configs, golden_dir, torch):
    S.run_golden_qrm(device_engine, *S.golden_qrm(name, configs, golden_dir))


def test_rebind_with_qrm_columns_between_sync_steps(torch):
    """A handle without QRM columns, synchronous steps, rmx_bind with QRM columns (the mailbox is freed and rebuilt with
    its QRM sections), synchronous steps: the results continue as one uninterrupted asynchronous run's."""
    from rmx.engine import _ptr

    case, N, K = "q250_a1_fast", 3, 80
    tab = L.limit_world(case)[1]
    acts = L.case_actions(case, n=N, steps=K)
    ref = S.oracle_record(tab, acts, qrm=True)
    env, a_env = device_engine(tab, N), device_engine(tab, N, with_qrm=True)
    put = to_device(torch)
    try:
        a_env.reset(seed=123)
        env.reset_sync(seed=123)
        for s in range(K):
            if s == K // 2:
                for k in S.QRM_COLS:
                    setattr(env, k, torch.zeros_like(getattr(a_env, k)))
                    setattr(env._buf, k, _ptr(getattr(env, k)))
                _capi.check(env.lib.rmx_bind(env._h, C.byref(env._buf)), "rmx_bind")
                env._sy = None  # host arrays for the new column set
            a_env.step(put(acts[s]), autoreset=True)
            out = env.step_sync(acts[s], autoreset=True)
            assert ("qrm_s" in out) == (s >= K // 2)
            S.assert_vs_oracle(tab, out, ref["snaps"][s], f"step {s}", qrm=s >= K // 2)
            S.assert_bit_equal(out, S.columns(a_env), f"step {s}")
        env.sync_end()
        S.assert_bit_equal(S.columns(env), S.columns(a_env), "after sync_end")
        S.assert_same_stats(env, a_env, ref["stats"])
    finally:
        env.close()
        a_env.close()


def test_qrm_columns_refused_without_qrm(torch):
    S.run_qrm_refused(device_engine, L.limit_world("q250_a1_fast")[1], stream=stream_of)


# ---- D. the two halves ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,N", [("a8_fl", 1), ("q250_a2_generic", S.N_SYNC)])
def test_two_halves(case, N, torch):
    tab = L.limit_world(case)[1]
    put = to_device(torch)
    S.run_two_halves(device_engine, tab, L.case_actions(case, n=N, steps=40), stream=stream_of,
                     async_step=lambda env, a: env.step(put(a), autoreset=True))


def test_dict_api_with_eight_agents(configs, golden_dir, monkeypatch):
    """The dict API (rmx.compat through csrc/rmx_dictstep.c) on the 8-agent golden, one env: 8 inline actions per
    request.  The resident workgroup against the host step, dict for dict, and against the reference's recording."""
    from rmx import compat as CP
    from test_compat_cpu import CountingStep, _golden_seed, _strip
    from test_host_vs_device_gpu import _close, _dict_wrapper

    counting = CountingStep()
    monkeypatch.setattr(CP, "_dictstep_module", lambda: counting)
    name, e, steps = "fl8_chain200", 1, 150
    g = dict(np.load(os.path.join(golden_dir, f"traj_{name}.npz")))
    desc = configs[name]
    (wh, envh, agh), (wg, envg, agg) = _dict_wrapper(desc, "cpu"), _dict_wrapper(desc, 0)
    assert len(agg) == 8
    try:
        base, episode = int(g["seed"]), 0
        assert wh.reset(seed=_golden_seed(desc, base, e, episode))[0] == \
            wg.reset(seed=_golden_seed(desc, base, e, episode))[0]
        names = ["up", "down", "left", "right"]
        for s in range(steps):
            outs = [w.step({ag.name: CP.ActionRL(names[int(g["actions"][s, i, e])]) for i, ag in enumerate(agents)})
                    for w, agents in ((wh, agh), (wg, agg))]
            (oh, rwh, th, uh, ih), (og, rwg, tg, ug, ig) = outs
            assert oh == og and th == tg and uh == ug, s
            assert _close(rwh, rwg), (s, rwh, rwg)
            sh, sg = _strip(ih), _strip(ig)
            for n in sh:
                assert [k for k, _ in sh[n]] == [k for k, _ in sg[n]], s
                for (k, vh), (_, vg) in zip(sh[n], sg[n]):
                    assert (abs(vh - vg) <= 1e-6) if isinstance(vh, float) else vh == vg, (s, n, k)
            for i, ag in enumerate(agg):
                assert og[ag.name] == {"pos_x": int(g["pos_x"][s, i, e]), "pos_y": int(g["pos_y"][s, i, e])}, (s, i)
                assert abs(rwg[ag.name] - g["reward"][s, i, e]) <= 1e-6
                assert ag.get_reward_machine().get_state_index(ig[ag.name]["q"]) == int(g["q"][s, i, e])
            assert envh.timestep == envg.timestep == int(g["t"][s, e])
            if g["env_done"][s, e]:
                episode += 1
                assert wh.reset(seed=_golden_seed(desc, base, e, episode))[0] == \
                    wg.reset(seed=_golden_seed(desc, base, e, episode))[0]
        assert counting.calls == 2 * steps  # the C step path served both wrappers (no Python fallback)
        assert g["q"][:steps, :, e].max() >= 8  # (every agent's chain advances on the two-cell lake)
    finally:
        wg._engine.close()
        wh._engine.close()


# ---- E. get_mdp -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fix", [False, True])
@pytest.mark.parametrize("case", S.MDP_CASES)
def test_mdp_kernel_on_limit_worlds(case, fix, torch):
    """mdp_kernel on every agent of every limit world (S up to W * H * enc_nq = 7,500 and 20,480 states, successors
    encoded from 250 RM states, 4,096 cells, 250 events): next / done identical to the host handle's and the oracle's,
    rewards within 1e-6."""
    from rmx.engine import HostRMEnv, VecRMEnv

    tab = L.limit_world(case)[1]
    h, d = HostRMEnv(tab, 1), VecRMEnv(tab, 1)
    try:
        for a in range(tab.n_agents):
            g, nxt, done = S.oracle_mdp_as_golden(tab, a, fix)
            assert S.mdp_states(d, a) == tab.width * tab.height * int(tab.enc_nq[a]) == S.mdp_states(h, a)
            if fix or tab.kind == T.OFFICE_WORLD:
                S.mdp_liveness(case, tab, a, nxt, done)
            hn, hr, hd = h.mdp_arrays(a, fix)
            dn, dr, dd = (x.cpu().numpy() for x in d.mdp_arrays(a, fix))
            np.testing.assert_array_equal(dn, hn)
            np.testing.assert_array_equal(dd, hd)
            np.testing.assert_allclose(dr, hr, rtol=0, atol=1e-6)
            S.check_mdp(tab, a, dn, dr, dd, g)
        d.check_errors()
    finally:
        h.close()
        d.close()
