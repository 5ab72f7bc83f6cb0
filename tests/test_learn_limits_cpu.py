"""The learner at its limits and in mixed use, on host handles (the GPU half: tests/test_learn_limits_gpu.py).

* Every field-width and table-mode limit world of tests/test_limits_gpu.py through the learn step, against the plain
  Python restatement (tests/learnref.py): 249 dependent counterfactual updates per agent-step, RM indices, QRM list
  bytes and event ids above 127, table rows up to 20,479.  Liveness is asserted per world from the restatement's own
  visits and the twin's columns, never from the engine under test.
* One handle driven through every entry point of a training loop (learn steps, plain steps, a step window, the fused
  report, masked resets, a checkpoint round trip, a rollout, cleared statistics) against a twin that only ever runs the
  plain entry points, with the learner restated beside it.
* Rebinding other tables, another gamma and another phi on a live handle.
* What a caller may write: tables filled with signed zeros, denormals, huge values, infinities and NaN; pos_x / pos_y /
  rm_q columns overwritten out of range.
"""
import dataclasses
import json
import os

import numpy as np
import pytest

import learn_common as LC
import learnref as LR
import test_limits_gpu as LIM
from rmx import tables as T
from rmx.engine import HostRMEnv
from rmx.learn import VecQLearning
from test_random_maps_gpu import CASES, random_tables

FL, OW = T.FROZEN_LAKE, T.OFFICE_WORLD


def limit_liveness(case, tab, R, ev_seen):
    """What shows that a run of limit world `case` used the field it is there for; from the restatement's visits
    (R.visits [A, N, S_max, 4]) and the event ids detected on the twin (ev_seen)."""
    nQ = int(max(tab.enc_nq))
    rows = np.flatnonzero((R.visits > 0).any(axis=(0, 1, 3)))
    out = {"top_row": int(rows.max()), "rows": R.S_max}
    if case.startswith("q250"):
        assert int(tab.n_qrm.max()) == 249
        out["rows_q_ge_128"] = int((rows % nQ >= 128).sum())
        assert out["rows_q_ge_128"] > 0, (case, out)
    elif case in ("e160_a1_fast", "e250_a2_generic"):
        out["ev_max"] = max(ev_seen)
        assert out["ev_max"] >= 128, (case, out)
    elif case in ("w255_h2_fast", "w2_h255_fast", "w256_h2", "cells4096_sq", "cells4096_row"):
        assert out["top_row"] >= R.S_max // 2, (case, out)
    return out


@pytest.mark.parametrize("lr", [None, 0.3])
@pytest.mark.parametrize("use_qrm", [True, False])
@pytest.mark.parametrize("case", list(LIM.CASES))
def test_host_equals_the_restatement_on_the_limit_worlds(case, use_qrm, lr):
    tab = LIM.limit_world(case)[1]
    rsh = use_qrm and tab.phi is not None
    N, K = 2, 70
    env = HostRMEnv(tab, N)
    twin = HostRMEnv(tab, N, with_qrm=True, with_enc_state=True)
    L = VecQLearning(env, 0.9, lr, qtable_init=0.5, use_qrm=use_qrm, use_rsh=rsh)
    R = LR.LearnRef(twin, 0.9, lr, qtable_init=0.5, use_qrm=use_qrm, use_rsh=rsh)
    acts = env.fill_actions(9, 0, K)
    ev_seen = {0}
    for t in range(K):
        L.step(acts[t])
        R.step(acts[t])
        for a in range(tab.n_agents):  # the event detected on the cell the step ended on
            ev_seen |= set(tab.cell_event[a][twin.pos_y[a] * tab.width + twin.pos_x[a]].tolist())
    LC.assert_same_bits(L.q, R.q, (case, "q"))
    LC.assert_same_bits(L.visits, R.visits, (case, "visits"))
    assert (R.visits > 0).any()
    limit_liveness(case, tab, R, ev_seen)


# ---- one handle, every entry point ---------------------------------------------------------------------------------
MIXED_WORLDS = {"ow_a4": (2, OW, 12, 10, 4, 6, 7, True), "fl_a2": (1, FL, 6, 6, 2, 3, 3, False)}


@pytest.mark.parametrize("world", sorted(MIXED_WORLDS))
def test_one_host_handle_through_every_entry_point(world):
    """The handle with the learner against a twin that never runs a learn step: the twin's columns and statistics come
    from rmx_step / rmx_step_seq / rmx_step_report / rmx_rollout alone, the learner's tables from the restatement.  A
    learn step that left the episode statistics or a column to anything but the step's own accounting fails here."""
    tab = dataclasses.replace(random_tables(*MIXED_WORLDS[world]), max_t=20)
    N = 5
    env = HostRMEnv(tab, N, with_enc_state=True)
    twin = HostRMEnv(tab, N, with_qrm=True, with_enc_state=True)
    kw = dict(use_qrm=True, qtable_init=0.0)
    L = VecQLearning(env, 0.9, 0.2, **kw)
    R = LR.LearnRef(twin, 0.9, 0.2, **kw)
    seen = LC.mixed_use(LC.EngineSide(env, L), LC.RefSide(twin, R), tab.n_agents, N)
    assert seen["episodes"] > 0 and seen["visited"] > 0 and seen["segments"] == 15
    if world == "fl_a2":  # (the OfficeWorld's first episodes are the truncations inside the rollout)
        assert seen["episodes_at_report"] > 0 and seen["episodes_after_clear"] > 0


# ---- rebind --------------------------------------------------------------------------------------------------------
def rebind_phases(make_env, new_table, as_actions, tab, N):
    """Tables X with shaping for 5 learn steps, then fresh tables Y without shaping and another gamma for 5, then fresh
    tables Z with shaping again and ANOTHER phi for 5.  Returns X after phase 1, X after phase 3, Y after phase 2, Y
    after phase 3, Z (host arrays)."""
    env = make_env(tab, N)
    L = VecQLearning(env, 0.9, 0.3, qtable_init=0.5, use_qrm=True, use_rsh=True)
    acts = HostRMEnv(tab, N).fill_actions(4, 0, 15)
    phi2 = np.asarray(tab.phi, np.float64) * 0.5 + 0.25
    assert not np.array_equal(phi2, tab.phi)
    X = (L.q, L.visits)
    for t in range(5):
        L.step(as_actions(acts[t]))
    x1 = [LC.host(v).copy() for v in X]
    Y = (new_table(env, L, 0.5), new_table(env, L, 0.0))
    LC.bind(L, Y[0], Y[1], 0.7, 0.3, True, False)
    for t in range(5, 10):
        L.step(as_actions(acts[t]))
    y2 = [LC.host(v).copy() for v in Y]
    x2 = [LC.host(v).copy() for v in X]
    Z = (new_table(env, L, 0.5), new_table(env, L, 0.0))
    LC.bind(L, Z[0], Z[1], 0.7, 0.3, True, True, phi=phi2)
    for t in range(10, 15):
        L.step(as_actions(acts[t]))
    env.check_errors()
    out = dict(x1=x1, x2=x2, x3=[LC.host(v).copy() for v in X], y2=y2, y3=[LC.host(v).copy() for v in Y],
               z=[LC.host(v).copy() for v in Z])
    env.close()
    return out


def host_table(env, L, fill):
    return np.full(L.q.shape, fill, np.float64)


def rebind_reference(tab, N):
    """The three phases restated: one twin, a LearnRef per phase over it (phase 3 over a table copy with phi2)."""
    twin = HostRMEnv(tab, N, with_qrm=True, with_enc_state=True)
    acts = twin.fill_actions(4, 0, 15)
    tabs = [tab, tab, dataclasses.replace(tab, phi=np.asarray(tab.phi, np.float64) * 0.5 + 0.25)]
    out = []
    for ph, (gamma, rsh) in enumerate(((0.9, True), (0.7, False), (0.7, True))):
        R = LR.LearnRef(twin, gamma, 0.3, qtable_init=0.5, use_qrm=True, use_rsh=rsh)
        R.tab = tabs[ph]
        for t in range(5 * ph, 5 * ph + 5):
            R.step(acts[t])
        out.append((R.q, R.visits))
    return out


def check_rebind(got, ref):
    for k, (a, b) in enumerate(zip(got["x1"], ref[0])):
        LC.assert_same_bits(a, b, ("X", k))
    for name in ("x2", "x3"):  # X is not written once other tables are bound
        for a, b in zip(got[name], got["x1"]):
            LC.assert_same_bits(a, b, name)
    for k, (a, b) in enumerate(zip(got["y2"], ref[1])):
        LC.assert_same_bits(a, b, ("Y", k))
    for a, b in zip(got["y3"], got["y2"]):
        LC.assert_same_bits(a, b, "y3")
    for k, (a, b) in enumerate(zip(got["z"], ref[2])):  # the new phi was taken
        LC.assert_same_bits(a, b, ("Z", k))
    assert (ref[2][1] > 0).any() and not np.array_equal(ref[2][0], ref[1][0])


def rebind_world():
    return dataclasses.replace(random_tables(*CASES["ow_regs_eligible"]), max_t=20)


def test_rebinding_tables_gamma_and_phi_on_a_host_handle():
    tab = rebind_world()
    N = 4
    ref = rebind_reference(tab, N)
    check_rebind(rebind_phases(HostRMEnv, host_table, lambda a: a, tab, N), ref)
    # the phases are told apart by the reference itself: shaping, gamma and phi each change the tables
    twin = HostRMEnv(tab, N, with_qrm=True, with_enc_state=True)
    acts = twin.fill_actions(4, 0, 15)
    for t in range(10):
        twin.step(acts[t])
    R = LR.LearnRef(twin, 0.7, 0.3, qtable_init=0.5, use_qrm=True, use_rsh=True)  # phase 3 with the FIRST phi
    for t in range(10, 15):
        R.step(acts[t])
    assert not np.array_equal(LC.bits(R.q), LC.bits(ref[2][0]))


# ---- special values in the tables ----------------------------------------------------------------------------------
def special_run(make_env, as_table, tab, values, lr, reference=None):
    """70 policy steps (epsilon 0.3, best on every fifth) over a q table drawn from `values`.  Against `reference`
    (a function of the twin: the restatement) or, without one, returns (actions [70, A, N], q, visits, q0)."""
    N = 4
    env = make_env(tab, N)
    L = VecQLearning(env, 0.9, lr, use_qrm=True, use_rsh=True)
    q0 = LC.special_fill(tuple(L.q.shape), values)
    as_table(L.q, q0)
    out = np.zeros((tab.n_agents, N), np.int32) if L.host else env.torch.zeros((tab.n_agents, N), dtype=env.torch.int32,
                                                                               device=env.device)
    R = reference(q0) if reference else None
    acts = []
    for t in range(70):
        best = t % 5 == 4
        L.act_step(0.3, 11, t, best=best, actions_out=out)
        acts.append(LC.host(out).copy())
        if R is not None:
            want = R.choose(0.3, 11, t, best=best)
            assert np.array_equal(acts[-1], want), t
            R.step(want)
    res = (np.stack(acts), LC.host(L.q).copy(), LC.host(L.visits).copy(), q0)
    env.check_errors()
    env.close()
    if R is not None:
        LC.assert_same_but_nan(res[1], R.q, "q")
        LC.assert_same_bits(res[2], R.visits, "visits")
    return res


def check_special(values, acts, q, q0):
    """The run is live: every action drawn, more than 1,000 entries changed, NaNs appeared where the issue's
    measurement says they do (from 0 x inf with 1 / visits, and whenever the fill holds -inf / NaN)."""
    assert sorted(set(acts.ravel().tolist())) == [0, 1, 2, 3]
    changed = (LC.bits(q) != LC.bits(q0)) & ~(np.isnan(q) & np.isnan(q0))
    assert changed.sum() > 1000, changed.sum()
    new_nan = int((np.isnan(q) & ~np.isnan(q0)).sum())
    if len(values) > len(LC.SPECIAL):
        assert np.isnan(q0).any() and new_nan > 0
    return new_nan


def np_fill(dst, src):
    dst[...] = src


@pytest.mark.parametrize("lr", [0.3, None])
@pytest.mark.parametrize("values", [LC.SPECIAL, LC.SPECIAL_NEG], ids=["nonneg", "neg_inf_nan"])
def test_special_values_in_the_tables_on_the_host(values, lr):
    tab = random_tables(*CASES["ow_regs_eligible"])

    def reference(q0):
        twin = HostRMEnv(tab, 4, with_qrm=True, with_enc_state=True)
        R = LR.LearnRef(twin, 0.9, lr, use_qrm=True, use_rsh=True)
        R.q[...] = q0
        return R

    acts, q, _, q0 = special_run(HostRMEnv, np_fill, tab, values, lr, reference)
    new_nan = check_special(values, acts, q, q0)
    if lr is None and len(values) == len(LC.SPECIAL):
        assert new_nan == 359  # through 0 x inf: (1 - 1 / 1) * inf on an entry's first visit


def test_policy_on_a_nan_row_is_action_3():
    """A row whose maximum is NaN has no entry equal to it: greedy and best give action 3 (include/rmx.h).  The
    maximum is NaN only when row[0] is (np.max of the engine: m = row[0], then m = v where v > m)."""
    tab = T.compile_scenario(T.baseline_scenario(2))
    N = 64
    env = HostRMEnv(tab, N)
    L = VecQLearning(env, 0.9, 0.2, use_qrm=True)
    nan = float("nan")
    L.q[...] = 0.0
    L.q[0, :, :, :] = (nan, 5.0, 1.0, 2.0)  # agent 0: a NaN maximum
    L.q[1, :, :, :] = (1.0, nan, 7.0, nan)  # agent 1: NaN further on is skipped, the maximum is entry 2
    out = np.full((2, N), -1, np.int32)
    for best in (True, False):
        L.act_step(0.0, 3, 0, best=best, learn=False, autoreset=False, actions_out=out)
        assert (out[0] == 3).all() and (out[1] == 2).all(), (best, out)
    assert LR.policy_action((nan, 5.0, 1.0, 2.0), 3, 0, N, 0, 2, 0, 0.0, True) == 3
    assert LR.policy_action((nan, 5.0, 1.0, 2.0), 3, 0, N, 0, 2, 0, 0.0, False) == 3
    assert LR.policy_action((1.0, nan, 7.0, nan), 3, 0, N, 0, 2, 1, 0.0, False) == 2


# ---- out-of-range columns ------------------------------------------------------------------------------------------
WORDS = [256, 0x1FF, -1, 0x01000003, 0x7FFFFFFF, 0x100, 65536 + 2, -256]  # test_window_packed_gpu's value list


def _golden(name):
    with open(os.path.join(LC.GOLDEN, "configs.json")) as f:
        return T.compile_scenario(json.load(f)[name])


@pytest.mark.parametrize("use_qrm", [False, True])
def test_out_of_range_columns_drop_the_experience_on_the_host(use_qrm):
    """fl2_open: enc_nq 9 and 3, so agent 1 owns 75 of the 225 rows.  Every second env gets garbage, in two forms:
    (a) the words of test_out_of_range_column_words_never_reach_the_record in pos_x, pos_y and rm_q (the host clamps
        such x / y / q to 0 before the step, so these envs are only required to leave everyone else alone);
    (b) agent 1 parked on the last cells with rm_q = 3 .. 8: inside the RM tables' 9 padded states, so not clamped, but
        (cell * 3 + rm_q) is past agent 1's last row.  The experience must be dropped and the policy must read a
        zero row; on these envs the host must equal the restatement, which states both rules.
    Learners of clean envs equal a run without garbage bit for bit, rows past an agent's own count keep what the
    caller put there (a row whose maximum is action 3, so that a policy reading it is told from the zero row)."""
    tab = dataclasses.replace(_golden("fl2_open"), max_t=20)
    W, H = tab.width, tab.height
    assert [int(v) for v in tab.enc_nq] == [9, 3] and tab.n_rm_states == 9
    N, K = 16, 10
    own = [W * H * int(v) for v in tab.enc_nq]
    lr = 0.3 if use_qrm else None
    env, clean = HostRMEnv(tab, N), HostRMEnv(tab, N)
    twin = HostRMEnv(tab, N, with_qrm=True, with_enc_state=True)
    kw = dict(qtable_init=0.5, use_qrm=use_qrm)
    L, Lc = VecQLearning(env, 0.9, lr, **kw), VecQLearning(clean, 0.9, lr, **kw)
    R = LR.LearnRef(twin, 0.9, lr, **kw)
    past = np.array([0.5, 1.5, 2.5, 3.5])  # rows past an agent's own count: the caller's, with their maximum at action 3
    for a in range(tab.n_agents):
        for tbl in (L.q, Lc.q, R.q):
            tbl[a, :, own[a]:] = past
    words = np.array(WORDS, np.int64).astype(np.uint32).view(np.int32)
    form_a, form_b = np.arange(1, N, 4), np.arange(3, N, 4)
    acts = env.fill_actions(6, 0, K)
    dropped = zero_rows = 0
    for t in range(K):
        for e in (env, twin):
            for a in range(tab.n_agents):
                e.pos_x[a, form_a] = words[(form_a + t) % len(words)]
                e.pos_y[a, form_a] = words[(form_a + t + 3) % len(words)]
                e.rm_q[a, form_a] = words[(form_a + t + 5) % len(words)]
            e.pos_x[1, form_b] = W - 1 - (form_b // 4 + t) % 2
            e.pos_y[1, form_b] = H - 1
            e.rm_q[1, form_b] = 3 + (form_b // 4 + t) % 6
        if t % 3 == 2:  # a policy step: the row of a state outside the table is a zero row
            out = np.zeros((2, N), np.int32)
            want = R.choose(0.0, 8, t, best=True, autoreset=False)
            L.act_step(0.0, 8, t, best=True, autoreset=False, actions_out=out)
            assert np.array_equal(out[:, form_b], want[:, form_b]), t
            outside = R.encode(*R.pre_state(False))[1, form_b] >= own[1]
            zero_rows += int(outside.sum())
            assert (out[1, form_b[outside]] == 0).all()  # np.argmax of the zero row (the row at that index says 3)
            R.step(out, autoreset=False)
            Lc.step(out, autoreset=False)
            continue
        s_pre = R.encode(*R.pre_state(False))
        dropped += int((s_pre[1, form_b] >= own[1]).sum())
        L.step(acts[t], autoreset=False)
        Lc.step(acts[t], autoreset=False)
        R.step(acts[t], autoreset=False)
    assert dropped > 0 and zero_rows > 0
    ok = np.ones(N, bool)
    ok[form_a] = ok[form_b] = False
    for got, want in ((L.q, Lc.q), (L.visits, Lc.visits)):
        LC.assert_same_bits(got[:, ok], want[:, ok], "clean envs")
    live = np.ones(N, bool)
    live[form_a] = False
    LC.assert_same_bits(L.q[:, live], R.q[:, live], "restatement, q")
    LC.assert_same_bits(L.visits[:, live], R.visits[:, live], "restatement, visits")
    for a in range(tab.n_agents):  # rows past the agent's own count: never touched, in any env
        assert (L.q[a, :, own[a]:] == past).all() and (L.visits[a, :, own[a]:] == 0.0).all(), a
    assert (L.visits[1, form_b] > 0).any()  # (those envs did learn on their in-range steps)
