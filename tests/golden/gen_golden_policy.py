"""Record whole training runs of the REFERENCE: its own QLearning chooses every action from its own numpy generator
(needs the reference checkout that gen_golden.py imports; the fixtures, not the reference, travel with the tests).

Imports ``gen_golden`` (the reference with the offline stubs) for ``make_env`` and ``seed_for``, attaches the
reference's real ``QLearning`` (learning_algorithms/qlearning.py) with ``seed=`` and ``epsilon_start = epsilon_end =
eps`` to every agent and runs the runner's loop (frozen_lake_main.py:345-376, office_main.py:1709-1749): ``select_action``
for every agent, ``rm_env.step``, ``update_policy`` for every agent.  Nothing of the policy is restated here: the
actions saved are what ``select_action`` returned, the generator states the learners' own ``bit_generator.state``.  The
coverage counts below are read off the arguments the learner itself hands to ``rng.choice``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_policy.py [case ...]

Each case is saved as ``policy_<case>.npz``: the learner seeds [A, N], eps and the learner parameters, the chosen
actions [T, A, N], ``q`` / ``visits`` [3, A, N, S_max, 4] after the steps ``snap_steps``, every learner's final
generator as the engine's five column words [5, A, N] (state high, state low, increment high, increment low,
(has_uint32 << 32) | uinteger), and the scenario dict as JSON.
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

M64 = (1 << 64) - 1
# case -> (config, n_envs, n_steps, reset seed, eps, qtable_init, learner).  lr None: the 1 / visits rate
CASES = {
    "fl2_qrm": ("fl2", 4, 600, 41, 0.1, 1.0, dict(gamma=0.9, lr=0.1, use_qrm=True)),
    "fl2_visits": ("fl2", 4, 600, 42, 0.3, 1.0, dict(gamma=0.9, lr=None, use_qrm=False)),
    "ow2_final": ("ow2_final", 3, 1100, 43, 0.1, 2.0, dict(gamma=0.9, lr=0.25, use_qrm=False)),
    "fl2_eps0": ("fl2", 2, 200, 44, 0.0, 1.0, dict(gamma=0.9, lr=0.1, use_qrm=True)),
    "fl2_eps1": ("fl2", 2, 200, 45, 1.0, 1.0, dict(gamma=0.9, lr=0.1, use_qrm=True)),
}
MIN_EACH = 20  # explore draws and greedy choices among k = 1, 2, 3, 4 maxima, per case with 0 < eps < 1


def learner_seeds(case, A, N):
    """Env 0 of fl2_qrm is the FrozenLake runner's own seeding: every learner 2020 (frozen_lake_main.py:269-295).  The
    others are arbitrary, among them 0, one-word and two-word SeedSequence entropy."""
    rng = np.random.default_rng(sum(case.encode()))
    seeds = rng.integers(0, 2 ** 32, size=(A, N), dtype=np.uint64)
    seeds[0, N - 1] = rng.integers(2 ** 32, 2 ** 63, dtype=np.uint64)
    seeds[A - 1, N - 1] = 2 ** 64 - 1
    seeds[A - 1, 1] = 0
    if case == "fl2_qrm":
        seeds[:, 0] = 2020
    return seeds


class Spy:
    """The learner's generator, with the sequences it is asked to choose from written down."""

    def __init__(self, g, log):
        self.g, self.log = g, log

    def uniform(self, *a):
        return self.g.uniform(*a)

    def choice(self, seq):
        self.log.append(seq)
        return self.g.choice(seq)


def words(state):
    s, i = state["state"]["state"], state["state"]["inc"]
    return [s >> 64, s & M64, i >> 64, i & M64, (state["has_uint32"] << 32) | state["uinteger"]]


def run(case):
    cfg_name, N, T, seed, eps, qinit, lp = CASES[case]
    cfg = G.CONFIGS[cfg_name]
    A = len(cfg["agents"])
    fl = cfg["kind"] == "frozen_lake"
    probe, pagents, _ = G.make_env(cfg)
    W, H = probe.env.grid_width, probe.env.grid_height
    S = [W * H * ag.get_reward_machine().numbers_state() for ag in pagents]
    S_max = max(S)
    snap_steps = [T // 3, (2 * T) // 3, T]
    seeds = learner_seeds(case, A, N)
    q = np.full((3, A, N, S_max, 4), qinit, np.float64)
    visits = np.zeros((3, A, N, S_max, 4), np.float64)
    acts = np.zeros((T, A, N), np.int8)
    rng_final = np.zeros((5, A, N), np.uint64)
    log = []
    for e in range(N):
        rm_env, agents, _ = G.make_env(cfg)
        for i, ag in enumerate(agents):
            # the constructor formats learning_rate (qlearning.py:37), so 1 / visits is set on the built object
            alg = QLearning(gamma=lp["gamma"], action_selection="greedy", learning_rate=0.5 if lp["lr"] is None else lp["lr"],
                            epsilon_start=eps, epsilon_end=eps, qtable_init=qinit, use_qrm=lp["use_qrm"], use_rsh=False,
                            state_space_size=S[i], action_space_size=4, seed=int(seeds[i, e]))
            alg.learning_rate = lp["lr"]
            assert alg.epsilon == eps
            alg.rng = Spy(alg.rng, log)
            ag.set_learning_algorithm(alg)
        need_reset, episode, states = True, 0, None
        for t in range(T):
            if need_reset:
                states, _ = rm_env.reset(G.seed_for(cfg, seed, e, episode))
                states = copy.deepcopy(states)
                need_reset = False
            actions = {}
            for i, ag in enumerate(agents):
                actions[ag.name] = ag.select_action(rm_env.env.get_state(ag))
                acts[t, i, e] = next(k for k, v in ag.actions_dix().items() if v is actions[ag.name])
            new_states, rewards, terms, truncs, infos = rm_env.step(actions)
            for ag in agents:
                terminated = (terms[ag.name] or truncs[ag.name]) if fl else terms[ag.name]
                assert G_f32(infos[ag.name].get("Renv", 0)) and G_f32(infos[ag.name]["RQ"]), case
                ag.update_policy(state=states[ag.name], action=actions[ag.name], reward=rewards[ag.name],
                                 next_state=new_states[ag.name], terminated=terminated, infos=infos[ag.name])
            states = copy.deepcopy(new_states)
            if all(terms.values()) or all(truncs.values()):
                need_reset = True
                episode += 1
            for k, st in enumerate(snap_steps):
                if t + 1 == st:
                    for i, ag in enumerate(agents):
                        alg = ag.get_learning_algorithm()
                        q[k, i, e, :S[i]] = alg.q_table
                        visits[k, i, e, :S[i]] = alg.visits
        for i, ag in enumerate(agents):
            alg = ag.get_learning_algorithm()
            assert alg.epsilon == eps  # (the runners never decay it)
            rng_final[:, i, e] = words(alg.rng.g.bit_generator.state)
    n_explore = sum(isinstance(s, range) for s in log)
    n_k = {k: sum((not isinstance(s, range)) and len(s) == k for s in log) for k in (1, 2, 3, 4)}
    assert len(log) == T * A * N
    print(f"{case}: explore {n_explore}, greedy ties {n_k}, buffered halves {int((rng_final[4] >> np.uint64(32)).sum())}")
    if 0.0 < eps < 1.0:
        assert n_explore >= MIN_EACH and all(v >= MIN_EACH for v in n_k.values()), case
    elif eps == 0.0:
        assert n_explore == 0
    else:
        assert n_explore == len(log)
    return dict(actions=acts, seed=np.int64(seed), policy_seeds=seeds, epsilon=np.float64(eps), config=np.array(cfg_name),
                scenario=np.array(json.dumps(cfg)), gamma=np.float64(lp["gamma"]),
                learning_rate=np.float64(0.0 if lp["lr"] is None else lp["lr"]), use_qrm=np.int32(lp["use_qrm"]),
                use_rsh=np.int32(0), trunc_is_terminal=np.int32(fl), qtable_init=np.float64(qinit),
                snap_steps=np.asarray(snap_steps, np.int32), n_states=np.asarray(S, np.int32), q=q,
                visits=visits.astype(np.uint32), rng_final=rng_final,
                counts=np.asarray([n_explore, n_k[1], n_k[2], n_k[3], n_k[4]], np.int64))


def G_f32(x):
    return float(np.float32(x)) == float(x)


def main(only=None):
    for case in only or CASES:
        out = run(case)
        path = os.path.join(HERE, f"policy_{case}.npz")
        G._savez(path, **out)
        assert os.path.getsize(path) < 727 * 1024, (case, os.path.getsize(path))
        print("  ", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
