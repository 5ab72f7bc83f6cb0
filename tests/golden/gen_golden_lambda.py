"""Record Q(lambda) learner fixtures by running the REFERENCE's own QLearningLambda behind AgentRL.update_policy (needs
the reference checkout that gen_golden.py imports; the fixtures, not the reference, travel with the tests).

Imports ``gen_golden`` (the reference with the offline stubs) for ``make_env``, ``hash_action`` and ``seed_for``,
attaches the reference's real ``QLearningLambda`` (learning_algorithms/qlearning_lambda.py) to every agent and runs the
runner's loop (frozen_lake_main.py:336-376, office_main.py:1696-1749): hashed actions, or ``select_action`` for every
agent on the learner's own generator; ``rm_env.step``; ``update_policy`` for every agent; ``reset(seed of the
episode)`` before the step that follows an episode's end, which clears the traces (ma_frozen_lake.py:77-81,
ma_office.py:100-102).  The update is never restated here: the tables saved are the learners' own ``q_table`` /
``visits`` / ``e_table``, and the coverage each case asserts is read off those tables around the reference's calls.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_lambda.py [case ...]

Each case is saved as ``lambda_<case>.npz``: the actions [T, A, N], the learner parameters, ``q`` [3, A, N, S_max, 4]
after the steps ``snap_steps``, ``visits`` likewise, the traces at those steps as lists (``e_idx`` / ``e_val``
[3, A, N, Lmax], ``e_cnt`` [3, A, N]: the non-zero entries of ``e_table`` in flat index order), the scenario dict as
JSON, ``coverage`` (the counts asserted below) and, for the policy cases, the learner seeds, eps, every learner's final
generator as the engine's five column words, and for the slip case the env's generator [3, 4, N], episode [3, N],
positions, RM indices and timestep at the snapshots.
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
import gen_golden_policy as P  # noqa: E402

from multiagent_rlrm.learning_algorithms.qlearning_lambda import QLearningLambda  # noqa: E402

# case -> (config, n_envs, n_steps, reset seed, gamma, lambd, lr (None: 1 / visits), eps (None: hashed actions))
CASES = {
    "fl2_lr": ("fl2", 4, 600, 61, 0.9, 0.8, 0.1, None),
    "fl2_open_visits": ("fl2_open", 2, 1600, 62, 0.9, 0.8, None, None),
    "fl2_open_underflow": ("fl2_open", 2, 1600, 63, 0.9, 0.001, 0.3, None),
    # (the seed is one under which a hashed walk runs into the step limit with neither agent's RM finished)
    "ow2_plain": ("ow2_final", 3, 1100, 125, 0.9, 0.9, 0.25, None),
    "fl2_policy": ("fl2", 4, 600, 65, 0.9, 0.8, 0.1, 0.1),
    "fl2_slip_policy": ("fl2_randstart_slip", 4, 600, 66, 0.9, 0.8, 0.1, 0.1),
}
TINY = np.finfo(np.float64).tiny  # the smallest normal


def f32(x):
    return float(np.float32(x)) == float(x)


def run(case):
    cfg_name, N, T, seed, gamma, lambd, lr, eps = CASES[case]
    cfg = G.CONFIGS[cfg_name]
    A = len(cfg["agents"])
    fl = cfg["kind"] == "frozen_lake"
    rng_on = bool(cfg.get("stochastic", False)) or bool(cfg.get("random_start_positions", False))
    probe, pagents, _ = G.make_env(cfg)
    W, H = probe.env.grid_width, probe.env.grid_height
    S = [W * H * ag.get_reward_machine().numbers_state() for ag in pagents]
    S_max = max(S)
    snap_steps = [T // 3, (2 * T) // 3, T]
    for v in (cfg.get("penalty", 0.0), cfg.get("plants_penalty", 0.0), cfg.get("wall_penalty", 0.0),
              cfg.get("reward_modifier", 1.0)):
        assert f32(v), f"{case}: {v} is not a float32 value"
    seeds = P.learner_seeds(case, A, N)
    q = np.zeros((3, A, N, S_max, 4), np.float64)
    visits = np.zeros((3, A, N, S_max, 4), np.float64)
    e_dense = np.zeros((3, A, N, S_max * 4), np.float64)
    acts = np.zeros((T, A, N), np.int8)
    rng_final = np.zeros((5, A, N), np.uint64)
    env_rng = np.zeros((3, 4, N), np.uint64)
    env_episode = np.zeros((3, N), np.int32)
    env_pos_x, env_pos_y = np.zeros((3, A, N), np.int8), np.zeros((3, A, N), np.int8)
    env_q, env_t = np.zeros((3, A, N), np.int16), np.zeros((3, N), np.int32)
    n_term_wipe = n_trunc_term = n_underflow = n_revisit = n_trunc_live = n_reset_wipe = n_resets = 0
    longest = 0
    for e in range(N):
        rm_env, agents, _ = G.make_env(cfg)
        for i, ag in enumerate(agents):
            alg = QLearningLambda(gamma=gamma, lambd=lambd, action_selection="greedy", learning_rate=lr,
                                  epsilon_start=0.0 if eps is None else eps, state_space_size=S[i],
                                  action_space_size=4, seed=int(seeds[i, e]))
            assert alg.learning_rate == lr and not alg.q_table.any()
            ag.set_learning_algorithm(alg)
        algs = [ag.get_learning_algorithm() for ag in agents]
        zeroed = [set() for _ in agents]  # cells whose trace went through a subnormal to exactly 0
        need_reset, episode, states = True, 0, None
        for t in range(T):
            if need_reset:
                live = [int(np.count_nonzero(alg.e_table)) for alg in algs]
                states, _ = rm_env.reset(G.seed_for(cfg, seed, e, episode))
                states = copy.deepcopy(states)
                assert not any(alg.e_table.any() for alg in algs), case  # the reset clears every learner's traces
                n_reset_wipe += sum(v > 0 for v in live)
                n_resets += 1
                need_reset = False
            actions = {}
            for i, ag in enumerate(agents):
                if eps is None:
                    a = G.hash_action(seed, t, N, e, A, i)
                    actions[ag.name] = ag.actions_dix()[a]
                else:
                    actions[ag.name] = ag.select_action(rm_env.env.get_state(ag))
                    a = next(k for k, v in ag.actions_dix().items() if v is actions[ag.name])
                acts[t, i, e] = a
            new_states, rewards, terms, truncs, infos = rm_env.step(actions)
            for i, ag in enumerate(agents):
                alg = algs[i]
                terminated = (terms[ag.name] or truncs[ag.name]) if fl else terms[ag.name]
                assert f32(infos[ag.name].get("Renv", 0)) and f32(infos[ag.name]["RQ"]), case
                before = alg.e_table.copy()
                v_before = alg.visits.copy()
                ag.update_policy(state=states[ag.name], action=actions[ag.name], reward=rewards[ag.name],
                                 next_state=new_states[ag.name], terminated=terminated, infos=infos[ag.name])
                after = alg.e_table
                cell = np.flatnonzero((alg.visits - v_before).ravel())  # the cell this update visited
                assert cell.size == 1, case
                if int(cell[0]) in zeroed[i]:
                    n_revisit += 1
                    zeroed[i].discard(int(cell[0]))
                if terminated:
                    assert not after.any(), case
                    n_term_wipe += bool(before.any())
                    n_trunc_term += bool(truncs[ag.name])
                else:
                    gone = np.flatnonzero(((before > 0) & (before < TINY) & (after == 0)).ravel())
                    n_underflow += gone.size
                    zeroed[i].update(int(v) for v in gone)
                    longest = max(longest, int(np.count_nonzero(after)))
                    if all(truncs.values()) and not all(terms.values()):
                        n_trunc_live += bool(after.any())
                assert alg.epsilon == (0.0 if eps is None else eps)
            states = copy.deepcopy(new_states)
            if all(terms.values()) or all(truncs.values()):
                need_reset = True
                episode += 1
            if t + 1 in snap_steps:
                k = snap_steps.index(t + 1)
                for i, ag in enumerate(agents):
                    q[k, i, e, :S[i]] = algs[i].q_table
                    visits[k, i, e, :S[i]] = algs[i].visits
                    e_dense[k, i, e, :S[i] * 4] = algs[i].e_table.ravel()
                    rm = ag.get_reward_machine()
                    env_pos_x[k, i, e], env_pos_y[k, i, e] = new_states[ag.name]["pos_x"], new_states[ag.name]["pos_y"]
                    env_q[k, i, e] = rm.get_state_index(rm.get_current_state())
                env_t[k, e] = rm_env.env.timestep
                if rng_on:
                    env_rng[k, :, e] = P.words(rm_env.env.rng.bit_generator.state)[:4]
                env_episode[k, e] = n_resets_env(episode, need_reset)
        for i in range(A):
            rng_final[:, i, e] = P.words(algs[i].rng.bit_generator.state)
    coverage = dict(term_wipes=n_term_wipe, trunc_terminal=n_trunc_term, underflows=n_underflow, revisits=n_revisit,
                    trunc_live=n_trunc_live, reset_wipes=n_reset_wipe, longest=longest, resets=n_resets)
    print(f"{case}: {coverage}")
    if case == "fl2_lr":  # terminal updates that wipe live traces
        assert n_term_wipe >= 10, case
    if case == "fl2_open_visits":
        assert n_trunc_term >= 1 and longest > 64, case
    if case == "fl2_open_underflow":
        assert n_underflow >= 1 and n_revisit >= 1, case
    if case == "ow2_plain":  # an episode ends by truncation with live traces; the reset clears them, not the update
        assert n_trunc_live >= 1 and n_reset_wipe >= 1, case
    if case == "fl2_slip_policy":
        assert n_resets > N, case  # at least one reseed inside the run
    # the traces as lists: the non-zero entries in flat index order
    e_cnt = np.count_nonzero(e_dense, axis=-1).astype(np.int32)
    Lmax = max(int(e_cnt.max()), 1)
    e_idx = np.zeros((3, A, N, Lmax), np.int32)
    e_val = np.zeros((3, A, N, Lmax), np.float64)
    for k, i, e in np.ndindex(3, A, N):
        nz = np.flatnonzero(e_dense[k, i, e])
        e_idx[k, i, e, :nz.size] = nz
        e_val[k, i, e, :nz.size] = e_dense[k, i, e, nz]
    out = dict(actions=acts, seed=np.int64(seed), config=np.array(cfg_name), scenario=np.array(json.dumps(cfg)),
               gamma=np.float64(gamma), lambd=np.float64(lambd), learning_rate=np.float64(0.0 if lr is None else lr),
               trunc_is_terminal=np.int32(fl), snap_steps=np.asarray(snap_steps, np.int32),
               n_states=np.asarray(S, np.int32), q=q, visits=visits.astype(np.uint32), e_idx=e_idx, e_val=e_val,
               e_cnt=e_cnt, coverage=np.array(json.dumps(coverage)))
    if eps is not None:
        out.update(policy_seeds=seeds, epsilon=np.float64(eps), rng_final=rng_final)
    if rng_on:
        out.update(env_rng=env_rng, env_episode=env_episode, env_pos_x=env_pos_x, env_pos_y=env_pos_y, env_q=env_q,
                   env_t=env_t)
    return out


def n_resets_env(episode, need_reset):
    """The engine's episode column after this step: episodes started so far, minus one."""
    return episode - 1 if need_reset else episode


def main(only=None):
    for case in only or CASES:
        out = run(case)
        path = os.path.join(HERE, f"lambda_{case}.npz")
        G._savez(path, **out)
        assert os.path.getsize(path) < 727 * 1024, (case, os.path.getsize(path))
        print("  ", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
