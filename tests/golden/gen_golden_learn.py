"""Record learner fixtures by running the REFERENCE's own QLearning behind AgentRL.update_policy (needs the reference
checkout that gen_golden.py imports; the fixtures, not the reference, travel with the tests).

Imports ``gen_golden`` (the reference with the offline stubs) for ``make_env``, ``hash_action`` and ``seed_for``,
attaches the reference's real ``QLearning`` (learning_algorithms/qlearning.py) to every agent, runs the runner's loop
(frozen_lake_main.py:336-376, office_main.py:1696-1749) on hashed actions and calls ``update_policy`` for every agent
after every step as the runners do.  The update is never restated here: the tables saved are the learners' own
``q_table`` / ``visits``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_learn.py [case ...]

Each case is saved as ``learn_<case>.npz``: the actions [T, A, N], the learner parameters, and ``q`` / ``visits`` of
every (agent, env) [3, A, N, S_max, 4] after the steps ``snap_steps`` (two earlier steps and the last; rows past an
agent's own state count stay at qtable_init / 0), and the scenario dict as JSON (``rmx.tables.compile_scenario``).
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402

from multiagent_rlrm.learning_algorithms.qlearning import QLearning  # noqa: E402

# case -> (config, n_envs, n_steps, seed, learner).  lr None: the 1 / visits rate; tit: the `terminated` the runner
# passes (FrozenLake: done or truncated, frozen_lake_main.py:359; OfficeWorld: done, office_main.py:1733)
CASES = {
    "fl2_qrm": ("fl2", 4, 600, 31, dict(gamma=0.9, lr=0.1, use_qrm=True, use_rsh=False)),
    "fl2_visits": ("fl2", 4, 600, 32, dict(gamma=0.9, lr=None, use_qrm=False, use_rsh=False)),
    "ow3_qrm_rsh": ("ow3", 2, 1100, 33, dict(gamma=0.9, lr=0.5, use_qrm=True, use_rsh=True)),
    "fl1_qrm16_visits": ("fl1_qrm16", 3, 600, 34, dict(gamma=0.95, lr=None, use_qrm=True, use_rsh=False)),
    # (short RMs: ow1's A-C-B-D is never completed by a hashed walk, and an OfficeWorld update is done only then)
    "ow2_plain": ("ow2_final", 3, 1100, 35, dict(gamma=0.9, lr=0.25, use_qrm=False, use_rsh=False)),
    # fl2 never reaches the step limit under hashed actions (its holes end every episode within ~250 steps): the
    # truncated FrozenLake update is recorded on the hole-free lake, whose episodes run into t = 1001
    "fl2_open_trunc": ("fl2_open", 2, 1600, 36, dict(gamma=0.9, lr=None, use_qrm=False, use_rsh=False)),
}
# The named scenarios' RMs only move forward in get_all_states() order, so a counterfactual's next-state row is never
# one that an earlier counterfactual of the same call wrote.  This RM has a backward transition (s1 --B--> s0): an
# agent that bumps into the lake's edge on B updates (B, s0) as experience 0 and reads that row as experience 1.
FL_BACK = [["s0", "A", "s1", 1], ["s1", "B", "s0", 0.5], ["s1", "A", "s2", 2]]
G.CONFIGS["fl2_back"] = {"kind": "frozen_lake", "layout": G.OPEN_LAKE, "penalty": 0.0,
                         "agents": [{"start": [4, 4], "rm": FL_BACK}, {"start": [3, 1], "rm": G.FL_AB}]}
CASES["fl2_back_qrm"] = ("fl2_back", 2, 1100, 37, dict(gamma=0.9, lr=0.3, use_qrm=True, use_rsh=False))
# 200 counterfactual updates per step (the 201-state chain of the limit goldens on the two-cell lake): QRM list entries
# and table rows with RM index >= 128, 402-row learners.  The hashed walk itself climbs the chain slowly: measured on
# the recording, the RM state after the step is >= 128 in 0.000 of the 300 x 2 (step, env) samples (0 of 600, highest
# state 77).  The rows with RM index >= 128 are visited all the same, in every snapshot, by the counterfactual updates
# (asserted in run()): they are what a narrow q_j or row index would corrupt.
CASES["fl1_chain200_qrm"] = ("fl1_chain200", 2, 300, 38, dict(gamma=0.95, lr=0.3, use_qrm=True, use_rsh=False))
HIGH_Q_SHARE = {"fl1_chain200_qrm": None}  # filled by run(): the measured share
QINIT = 1.0


def f32(x):
    return float(np.float32(x)) == float(x)


def run(case):
    cfg_name, N, T, seed, lp = CASES[case]
    cfg = G.CONFIGS[cfg_name]
    A = len(cfg["agents"])
    fl = cfg["kind"] == "frozen_lake"
    probe, pagents, _ = G.make_env(cfg)
    W, H = probe.env.grid_width, probe.env.grid_height
    S = [W * H * ag.get_reward_machine().numbers_state() for ag in pagents]
    S_max = max(S)
    snap_steps = [T // 3, (2 * T) // 3, T]
    q = np.full((3, A, N, S_max, 4), QINIT, np.float64)
    visits = np.zeros((3, A, N, S_max, 4), np.float64)
    acts = np.zeros((T, A, N), np.int8)
    n_done = n_alias = n_trunc = n_high = q_top = 0
    for v in (cfg.get("penalty", 0.0), cfg.get("plants_penalty", 0.0), cfg.get("wall_penalty", 0.0),
              cfg.get("reward_modifier", 1.0)):
        assert f32(v), f"{case}: {v} is not a float32 value"
    for e in range(N):
        rm_env, agents, _ = G.make_env(cfg)
        for i, ag in enumerate(agents):
            # the constructor formats learning_rate (qlearning.py:37), so 1 / visits is set on the built object
            alg = QLearning(gamma=lp["gamma"], action_selection="greedy", learning_rate=0.5 if lp["lr"] is None else lp["lr"],
                            qtable_init=QINIT, use_qrm=lp["use_qrm"], use_rsh=lp["use_rsh"], state_space_size=S[i],
                            action_space_size=4)
            alg.learning_rate = lp["lr"]
            ag.set_learning_algorithm(alg)
        need_reset, episode, states = True, 0, None
        for t in range(T):
            if need_reset:
                states, _ = rm_env.reset(G.seed_for(cfg, seed, e, episode))
                states = copy.deepcopy(states)
                need_reset = False
            actions = {}
            for i, ag in enumerate(agents):
                a = G.hash_action(seed, t, N, e, A, i)
                acts[t, i, e] = a
                actions[ag.name] = ag.actions_dix()[a]
            new_states, rewards, terms, truncs, infos = rm_env.step(actions)
            for ag in agents:
                terminated = (terms[ag.name] or truncs[ag.name]) if fl else terms[ag.name]
                assert f32(infos[ag.name].get("Renv", 0)) and f32(infos[ag.name]["RQ"]), case
                exps = infos[ag.name].get("qrm_experience", []) if lp["use_qrm"] else []
                written = set()
                for x in exps:  # (s, a, r, sn, done, ...): observed, not restated
                    assert f32(x[9]), case
                    n_done += bool(x[4])
                    n_alias += (not x[4]) and x[3] in written
                    written.add(x[0])
                if not lp["use_qrm"]:
                    n_done += bool(terminated)
                    n_trunc += bool(truncs[ag.name]) and bool(terminated)
                ag.update_policy(state=states[ag.name], action=actions[ag.name], reward=rewards[ag.name],
                                 next_state=new_states[ag.name], terminated=terminated, infos=infos[ag.name])
            states = copy.deepcopy(new_states)
            q_now = [ag.get_reward_machine().get_state_index(ag.get_reward_machine().get_current_state()) for ag in agents]
            n_high += sum(v >= 128 for v in q_now)
            q_top = max([q_top] + q_now)
            if all(terms.values()) or all(truncs.values()):
                need_reset = True
                episode += 1
            for k, st in enumerate(snap_steps):
                if t + 1 == st:
                    for i, ag in enumerate(agents):
                        alg = ag.get_learning_algorithm()
                        q[k, i, e, :S[i]] = alg.q_table
                        visits[k, i, e, :S[i]] = alg.visits
    share = float(np.mean([(visits[2, i, :, :S[i]] > 0).mean() for i in range(A)]))
    assert share >= 0.05, (case, share)
    assert n_done >= 1, case
    # a row written earlier in the same call is read only under a backward RM transition: the recorded case has one,
    # the runners' forward-only RMs none (checked, not just claimed)
    if case == "fl2_back_qrm":
        assert n_alias >= 1, case
    else:
        assert n_alias == 0, (case, n_alias)
    # the truncated FrozenLake update: on the hole-free lake; fl2's episodes end long before the step limit
    if case == "fl2_open_trunc":
        assert n_trunc >= 1, case
    if case == "fl2_visits":
        assert n_trunc == 0, (case, n_trunc)
    if case in HIGH_Q_SHARE:  # RM indices above 127 are lived in, and their rows are in every snapshot
        nQ = S[0] // (W * H)
        high = (np.arange(S_max) % nQ) >= 128
        assert all((visits[k, 0, :, high] > 0).any() for k in range(3)), case
        HIGH_Q_SHARE[case] = n_high / (T * N * A)
        print(f"{case}: RM state >= 128 in {HIGH_Q_SHARE[case]:.3f} of the {T} x {N} samples, highest {q_top}")
    print(f"{case}: visited share {share:.3f}, done {n_done}, same-call rows {n_alias}, truncated updates {n_trunc}")
    return dict(actions=acts, seed=np.int64(seed), config=np.array(cfg_name),
                scenario=np.array(json.dumps(cfg)), gamma=np.float64(lp["gamma"]),
                learning_rate=np.float64(0.0 if lp["lr"] is None else lp["lr"]), use_qrm=np.int32(lp["use_qrm"]),
                use_rsh=np.int32(lp["use_rsh"]), trunc_is_terminal=np.int32(fl), qtable_init=np.float64(QINIT),
                snap_steps=np.asarray(snap_steps, np.int32), n_states=np.asarray(S, np.int32), q=q,
                visits=visits.astype(np.uint32))


def main(only=None):
    for case in only or CASES:
        out = run(case)
        path = os.path.join(HERE, f"learn_{case}.npz")
        G._savez(path, **out)
        assert os.path.getsize(path) < 727 * 1024, (case, os.path.getsize(path))
        print("  ", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
