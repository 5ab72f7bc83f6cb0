"""Record whole training runs of the REFERENCE with its per-episode epsilon decay: its own QLearning, built with
``epsilon_start != epsilon_end``, chooses every action from its own numpy generator while the environment's own
``reset()`` calls ``learn_done_episode`` on it (ma_frozen_lake.py:86-88, ma_office.py:107-108) (needs the reference
checkout that gen_golden.py imports; the fixtures, not the reference, travel with the tests).

Imports ``gen_golden`` (through gen_golden_policy.py, whose helpers it uses) and the reference's real ``QLearning``
and runs the runner's loop as gen_golden_policy.py does: ``reset(seed of the episode)`` before the first step and
before the step that follows an episode's end, ``select_action`` for every agent, ``rm_env.step``, ``update_policy``
for every agent.  Nothing of the schedule is restated here: the epsilons saved are the learners' own ``epsilon``
attributes.  The loop resets once before step 0, so every learner has decayed once before its first draw.  On the
slip / random-start case the env is watched as gen_golden_slearn.py watches it (its ``Watch``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_eps.py [case ...]

Each case is saved as ``eps_<case>.npz``: what ``policy_<case>.npz`` holds (but no scalar epsilon), and
  epsilon_start, epsilon_end, epsilon_decay   the schedule every learner was built with
  epsilon [3, A, N]     every learner's ``epsilon`` after each snapshot step
  resets [N]            ``reset()`` calls per env over the run, the one before step 0 included
  floor_reset [N]       the number of the reset (1-based) at which the env's learners first stood at epsilon_end; 0: never
and on the slip / random-start case gen_golden_slearn.py's env_* arrays.
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_policy as P  # noqa: E402
import gen_golden_slearn as SL  # noqa: E402

from multiagent_rlrm.learning_algorithms.qlearning import QLearning  # noqa: E402

G = P.G
# case -> (config, n_envs, n_steps, reset seed, (epsilon_start, epsilon_end, epsilon_decay), qtable_init, learner)
CASES = {
    "fl2": ("fl2", 4, 600, 61, (1.0, 0.2, 0.8), 1.0, dict(gamma=0.9, lr=0.1, use_qrm=True)),
    "ow2_fail": ("ow2_fail", 3, 1200, 62, (0.9, 0.05, 0.7), 2.0, dict(gamma=0.9, lr=None, use_qrm=False)),
    "fl2_rs_slip": ("fl2_randstart_slip", 4, 600, 63, (1.0, 0.2, 0.8), 1.0, dict(gamma=0.9, lr=0.1, use_qrm=True)),
    "fl2_pow2": ("fl2", 2, 600, 64, (0.5, 0.0, 0.5), 1.0, dict(gamma=0.9, lr=0.1, use_qrm=True)),
}
FLOOR_CASES = ("fl2", "ow2_fail", "fl2_rs_slip")  # epsilon_end is reached exactly, and the env resets again after it
MIN_RESETS = 3
# the first snapshot is early, while the schedule is still on its way down (ow2_fail's episodes are a few steps long)
FIRST_SNAP = {"ow2_fail": 30}


def run(case):
    cfg_name, N, T, seed, (e0, e1, dec), qinit, lp = CASES[case]
    cfg = G.CONFIGS[cfg_name]
    A = len(cfg["agents"])
    fl = cfg["kind"] == "frozen_lake"
    dyn = bool(cfg.get("stochastic", False)) or bool(cfg.get("random_start_positions", False))
    snap_steps = [FIRST_SNAP.get(case, T // 8), T // 2, T]
    watch = SL.Watch(A, N, snap_steps)
    probe, pagents, _ = G.make_env(cfg)
    watch.attach(probe, pagents)  # (the probe: not an env of the run)
    W, H = probe.env.grid_width, probe.env.grid_height
    S = [W * H * ag.get_reward_machine().numbers_state() for ag in pagents]
    S_max = max(S)
    seeds = P.learner_seeds(case, A, N)
    q = np.full((3, A, N, S_max, 4), qinit, np.float64)
    visits = np.zeros((3, A, N, S_max, 4), np.float64)
    eps = np.zeros((3, A, N), np.float64)
    acts = np.zeros((T, A, N), np.int8)
    rng_final = np.zeros((5, A, N), np.uint64)
    resets = np.zeros(N, np.int32)
    floor_reset = np.zeros(N, np.int32)
    log = []
    for e in range(N):
        rm_env, agents, _ = G.make_env(cfg)
        watch.attach(rm_env, agents)
        algs = []
        for i, ag in enumerate(agents):
            # the constructor formats learning_rate (qlearning.py:37), so 1 / visits is set on the built object
            alg = QLearning(gamma=lp["gamma"], action_selection="greedy", learning_rate=0.5 if lp["lr"] is None else lp["lr"],
                            epsilon_start=e0, epsilon_end=e1, epsilon_decay=dec, qtable_init=qinit, use_qrm=lp["use_qrm"],
                            use_rsh=False, state_space_size=S[i], action_space_size=4, seed=int(seeds[i, e]))
            alg.learning_rate = lp["lr"]
            assert alg.epsilon == e0
            alg.rng = P.Spy(alg.rng, log)
            ag.set_learning_algorithm(alg)
            algs.append(alg)
        need_reset, episode, states = True, 0, None
        for t in range(T):
            if need_reset:
                states, _ = rm_env.reset(G.seed_for(cfg, seed, e, episode))  # (decays every learner's epsilon)
                states = copy.deepcopy(states)
                need_reset = False
                resets[e] += 1
                assert len({alg.epsilon for alg in algs}) == 1
                if floor_reset[e] == 0 and algs[0].epsilon == e1:
                    floor_reset[e] = resets[e]
            actions = {}
            for i, ag in enumerate(agents):
                actions[ag.name] = ag.select_action(rm_env.env.get_state(ag))
                acts[t, i, e] = next(k for k, v in ag.actions_dix().items() if v is actions[ag.name])
            new_states, rewards, terms, truncs, infos = rm_env.step(actions)
            for ag in agents:
                terminated = (terms[ag.name] or truncs[ag.name]) if fl else terms[ag.name]
                assert P.G_f32(infos[ag.name].get("Renv", 0)) and P.G_f32(infos[ag.name]["RQ"]), case
                ag.update_policy(state=states[ag.name], action=actions[ag.name], reward=rewards[ag.name],
                                 next_state=new_states[ag.name], terminated=terminated, infos=infos[ag.name])
            states = copy.deepcopy(new_states)
            if all(terms.values()) or all(truncs.values()):
                need_reset = True
                episode += 1
            for k, st in enumerate(snap_steps):
                if t + 1 == st:
                    for i, alg in enumerate(algs):
                        q[k, i, e, :S[i]] = alg.q_table
                        visits[k, i, e, :S[i]] = alg.visits
                        eps[k, i, e] = alg.epsilon
        for i, alg in enumerate(algs):
            rng_final[:, i, e] = P.words(alg.rng.g.bit_generator.state)
    n_explore = sum(isinstance(s, range) for s in log)
    n_k = {k: sum((not isinstance(s, range)) and len(s) == k for s in log) for k in (1, 2, 3, 4)}
    assert len(log) == T * A * N
    print(f"{case}: explore {n_explore}, greedy ties {n_k}, resets {resets.tolist()}, floor at reset "
          f"{floor_reset.tolist()}, epsilon at the snapshots {[sorted(set(v.ravel().tolist())) for v in eps]}")
    assert n_explore >= P.MIN_EACH and all(v >= P.MIN_EACH for v in n_k.values()), case
    assert (resets >= MIN_RESETS).all(), case
    assert watch.built == N + 1 and watch.resets == int(resets.sum())
    if case in FLOOR_CASES:
        assert (floor_reset >= 1).all() and (resets > floor_reset).all() and (eps[2] == e1).all(), case
    else:
        assert (floor_reset == 0).all() and (eps[2] > e1).all(), case
    # the first snapshot catches the schedule on its way: decayed, and not yet where it ends
    assert (eps[0] < e0).all() and (eps[0] > eps[2]).all(), case
    out = dict(actions=acts, seed=np.int64(seed), policy_seeds=seeds, epsilon_start=np.float64(e0),
               epsilon_end=np.float64(e1), epsilon_decay=np.float64(dec), config=np.array(cfg_name),
               scenario=np.array(json.dumps(cfg)), gamma=np.float64(lp["gamma"]),
               learning_rate=np.float64(0.0 if lp["lr"] is None else lp["lr"]), use_qrm=np.int32(lp["use_qrm"]),
               use_rsh=np.int32(0), trunc_is_terminal=np.int32(fl), qtable_init=np.float64(qinit),
               snap_steps=np.asarray(snap_steps, np.int32), n_states=np.asarray(S, np.int32), q=q,
               visits=visits.astype(np.uint32), epsilon=eps, rng_final=rng_final, resets=resets, floor_reset=floor_reset,
               counts=np.asarray([n_explore, n_k[1], n_k[2], n_k[3], n_k[4]], np.int64))
    if dyn:  # the env's own generator and episode count, as slearn_<case>.npz holds them
        assert (watch.episode[2] == resets - 1).all(), case
        assert len(watch.starts) >= 3 and watch.differing >= SL.MIN_DIFFERING, case
        out.update(env_pos_x=watch.pos_x, env_pos_y=watch.pos_y, env_q=watch.q, env_t=watch.t, env_rng=watch.rng,
                   env_episode=watch.episode,
                   coverage=np.asarray([watch.draws, watch.differing, watch.resets, len(watch.starts)], np.int64))
    return out


def main(only=None):
    for case in only or CASES:
        out = run(case)
        path = os.path.join(HERE, f"eps_{case}.npz")
        G._savez(path, **out)
        assert os.path.getsize(path) < 727 * 1024, (case, os.path.getsize(path))
        print("  ", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
