"""The CPU half of the limit tests (tests/test_limits_gpu.py holds the worlds, the oracle runs and the restated
selection rules; nothing here needs a GPU).

* tests/pyref.py, the plain-Python stepper that reads no compiled table, is pinned to the reference's recorded
  trajectories, then compared with the oracle on every limit world: the oracle and the engine share the dense uint8
  tables of rmx.tables, pyref works from the position sets and the transitions dicts.
* The oracle's trajectory on every limit, palette and size world meets the liveness conditions the GPU tests rely on
  (the measured figures are in the case tables' comments and in test_limit_world_liveness below).
* The host path equals the oracle on every palette edge and size edge (the limit worlds themselves: tests/
  test_host_random_maps.py); at the 64-KiB table limit it refuses what a device handle refuses.
* The restated selection rules on the limit worlds.
"""
import os

import numpy as np
import pytest

import oracle as O
import pyref
import test_limits_gpu as L
from rmx.engine import HostRMEnv

REWARD_TOL = 1e-6


def _pyref_vs(world, acts, columns):
    """pyref stepped over acts [T, A, N]; columns(s) gives the other side's dict of arrays after step s."""
    env = pyref.PyRefEnv(world, acts.shape[2])
    for s in range(acts.shape[0]):
        out = env.step(acts[s])
        ref = columns(s)
        for k in ("pos_x", "pos_y", "q", "flags", "t", "env_done"):
            if k in ref:
                np.testing.assert_array_equal(np.asarray(out[k], np.int64), ref[k].astype(np.int64), err_msg=f"{s} {k}")
        for k in ("reward", "renv", "shaping"):
            if k in ref:
                assert np.max(np.abs(np.asarray(out[k], np.float64) - ref[k].astype(np.float64))) <= REWARD_TOL, (s, k)


@pytest.mark.parametrize("name", ["fl2_quirks", "ow2_fail", "ow3"])
def test_pyref_matches_reference_golden(name, configs, golden_dir):
    """The plain-Python stepper reproduces the reference's recorded trajectories: the integer columns exactly, the
    rewards within 1e-6 (FrozenLake quirks: None-event self loops, rewarding final-state loops, hole penalties;
    OfficeWorld with failing walls and plants; three agents with shaping)."""
    g = dict(np.load(os.path.join(golden_dir, f"traj_{name}.npz")))
    world = pyref.world_from_scenario(configs[name])
    acts = g["actions"].astype(np.int32)

    def columns(s):
        return {"pos_x": g["pos_x"][s], "pos_y": g["pos_y"][s], "q": g["q"][s], "t": g["t"][s],
                "env_done": g["env_done"][s], "reward": g["reward"][s], "renv": g["renv"][s],
                "shaping": g["shaping"][s]}

    env = pyref.PyRefEnv(world, acts.shape[2])
    for s in range(acts.shape[0]):
        out = env.step(acts[s])
        ref = columns(s)
        for k in ("pos_x", "pos_y", "q", "t", "env_done"):
            np.testing.assert_array_equal(np.asarray(out[k], np.int64), ref[k].astype(np.int64), err_msg=f"{s} {k}")
        fl = np.asarray(out["flags"], np.int64)
        np.testing.assert_array_equal((fl & pyref.F_TERM) != 0, g["term"][s])
        np.testing.assert_array_equal((fl & pyref.F_TRUNC) != 0, g["trunc"][s])
        np.testing.assert_array_equal((fl & pyref.F_ACTIVE) != 0, g["active"][s])
        for k in ("reward", "renv", "shaping"):
            assert np.max(np.abs(np.asarray(out[k], np.float64) - ref[k])) <= REWARD_TOL, (s, k)


@pytest.mark.parametrize("case", list(L.CASES))
def test_pyref_matches_oracle_on_limit_world(case):
    """64 envs x 150 steps of every limit world: the oracle (dense uint8 tables) against the stepper that reads the
    unpacked description.  A signed byte in the packing of next_q or cell_event fails here."""
    world, tab = L.limit_world(case)
    acts = L.case_actions(case, n=64)
    orc = O.OracleEnv(tab, 64)

    def columns(s):
        orc.step(acts[s])
        return {"pos_x": orc.pos_x, "pos_y": orc.pos_y, "q": orc.rm_q, "flags": orc.flags, "t": orc.t,
                "env_done": orc.env_done, "reward": orc.reward, "renv": orc.renv, "shaping": orc.shaping}

    _pyref_vs(world, acts, columns)


@pytest.mark.parametrize("case", list(L.CASES))
def test_limit_world_liveness(case):
    """The oracle's trajectory at the GPU tests' size reaches the limit the world is there for."""
    tab = L.limit_world(case)[1]
    L.check_liveness(case, tab, L.case_reference(case)["traj"])


@pytest.mark.parametrize("name", list(L.PALETTES))
def test_palette_world_liveness_and_host(name):
    tab, acts, ref = L.palette_reference(name)
    L.check_palette_liveness(name, tab, ref)
    _host_vs_reference(tab, acts, ref)
    _, rec_bytes, sections = L.PALETTES[name]
    for forced in ({}, {"RMX_FAST_TABLES": "merged4"}):
        info = L.expected_info(tab, L.N_ENVS, forced)
        assert (info["variant"], info["record_bytes"], info["merged_sections"]) == ("fast", rec_bytes, sections), info


@pytest.mark.parametrize("name", list(L.SIZE_EDGES))
def test_size_world_liveness_and_host(name):
    _, forced, (variant, tables, sections, bytes16) = L.SIZE_EDGES[name]
    tab, acts, ref = L.size_reference(name)
    L.check_size_liveness(tab, ref)
    _host_vs_reference(tab, acts, ref)
    info = L.expected_info(tab, L.N_ENVS, L.MODES[forced])
    assert (info["variant"], info["tables"], info["merged_sections"], info["merged_bytes"]) == \
        (variant, tables, sections, bytes16), info


def _host_vs_reference(tab, acts, ref, seed=123):
    env = HostRMEnv(tab, acts.shape[2], with_enc_state=True)
    env.reset(seed=seed)
    for s in range(acts.shape[0]):
        env.step(acts[s])
        if s in ref["snaps"]:
            snap = ref["snaps"][s]
            for k in ("pos_x", "pos_y", "rm_q", "t", "flags", "env_done", "reward", "renv", "enc_state"):
                np.testing.assert_array_equal(getattr(env, k), snap[k], err_msg=f"{s} {k}")
            np.testing.assert_allclose(env.ep_ret, snap["ep_ret"], rtol=1e-5, atol=1e-5)
            if env.shaping is not None:
                np.testing.assert_allclose(env.shaping, snap["shaping"], rtol=0, atol=1e-6)
            if env.rng is not None:
                np.testing.assert_array_equal(env.rng, snap["rng"])
    env.check_errors()
    st, so = env.stats(), ref["stats"]
    assert st[1] == so[1] and st[2] == so[2] and st[3] == so[3], (st, so)
    np.testing.assert_allclose(st[0], so[0], rtol=1e-5, atol=1e-4)
    return env


def test_generic_blob_limit_on_the_host_path():
    """At 65,344 B of tables a host handle steps; at 65,904 B it is refused like a device handle (include/rmx.h)."""
    tab = L.size_world(**L.GENERIC_BLOB_OVER)
    assert L.generic_blob_bytes(tab) == 65904
    with pytest.raises(ValueError, match="tables exceed 64 KiB"):
        HostRMEnv(tab, 4)
    assert L.generic_blob_bytes(L.size_world(**L.SIZE_EDGES["generic_blob_under"][0])) == 65344


def test_limit_world_table_modes():
    """What the restated rules say about the limit worlds (the engine's agreement is asserted row by row on the GPU):
    the kernel and table modes the case table promises are the ones the sizes give."""
    def tables(case, **env):
        return L.expected_info(L.limit_world(case)[1], L.N_ENVS, env)

    q = tables("q250_a1_fast")
    assert (q["variant"], q["tables"], q["fast_blob_bytes"]) == ("fast", "global", 12176)  # one section: 160,000 B
    assert tables("q250_a1_fast", RMX_FAST_TABLES="merged")["merged_bytes"] == 160000
    m4 = tables("q250_a1_fast", RMX_FAST_TABLES="merged4")
    assert (m4["tables"], m4["record_bytes"], m4["merged4_bytes"], m4["merged_sections"]) == ("merged4", 4, 40000, 1)
    assert tables("q250_a2_generic")["variant"] == "generic" and \
        L.fast_blob_bytes(L.limit_world("q250_a2_generic")[1]) > 3 * L.FAST_BLOB_MAX
    e = tables("e160_a1_fast")
    assert e["variant"] == "fast" and e["fast_blob_bytes"] + 1280 == 16336 <= L.FAST_BLOB_MAX
    g = tables("e250_a2_generic")
    assert g["variant"] == "generic" and 40000 < g["generic_blob_bytes"] <= L.GENERIC_BLOB_MAX
    for c in ("w255_h2_fast", "w2_h255_fast"):
        assert tables(c)["variant"] == "fast" and tables(c, RMX_FAST_TABLES="merged4")["record_bytes"] == 4
    for c in ("w256_h2", "cells4096_sq", "cells4096_row", "a5_fl", "a7_ow", "a8_ow_shaping", "a8_fl"):
        assert tables(c)["variant"] == "generic"
        assert tables(c, RMX_LAYOUT="lpe")["variant"] == "lane_per_agent"
    for c, (target, fast, kw) in L.CASES.items():
        tab = L.limit_world(c)[1]
        assert (tab.n_agents, tab.width, tab.height) == (kw["A"], kw["W"], kw["H"])
        assert tab.n_rm_states == kw["Q"] and tab.n_events <= kw["n_ev"] + 1, (c, tab.n_rm_states, tab.n_events)
        if kw.get("detect_all"):  # (elsewhere an event cell no agent's detector drew is no event)
            assert tab.n_events == kw["n_ev"] + 1
        assert (tables(c)["variant"] == "fast") == fast
