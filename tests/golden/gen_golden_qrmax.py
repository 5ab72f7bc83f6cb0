"""Record QR-max learner fixtures by running the REFERENCE's own QRMax_v2 behind AgentRL.update_policy (needs the
reference checkout that gen_golden.py imports; the fixtures, not the reference, travel with the tests).

Imports ``gen_golden`` (the reference with the offline stubs) for ``make_env``, ``hash_action`` and ``seed_for``,
attaches the reference's real ``QRMax_v2`` (learning_algorithms/qrmax_v2.py) to every agent, as ``create_qrmax``
(office_main.py:720-746) builds it for ``--algorithm QRMAX`` / ``QRMAXRM``, calls ``learn_init`` as the runner does
(office_main.py:660) and runs the runner's loop (office_main.py:1696-1749, frozen_lake_main.py:336-376): hashed
actions, or ``select_action`` for every agent on the learner's own generator; ``rm_env.step``; ``update_policy`` for
every agent; ``reset(seed of the episode)`` before the step that follows an episode's end (which does nothing to a
QRMax_v2).  The update is never restated here: the tables saved are the learner's own; the sweeps of each solve are
obtained by wrapping ``solve_VI`` and differencing ``VI_iterations``, and the coverage each case asserts is read off
the learner's tables around the reference's calls.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_qrmax.py [case ...]

Each case is saved as ``qrmax_<case>.npz``: the actions [T, A, N], the learner parameters, and after the steps
``snap_steps`` (leading axis 3) ``q`` / ``n_tsqa`` / ``known_tsqa`` [A, N, S_max, 4] (``Q[s, q, a]`` at row s * nQ + q),
``n_tsa`` / ``n_rsa`` / ``sum_rsa`` [A, N, P, 4], the lists of ``nTSAS_dict`` in its own order with their ``nTSAS``
counts (``t_idx`` / ``t_cnt`` [A, N, P, 4, K], K the longest list), ``n_tqs`` / ``tq_next`` / ``n_rqs`` / ``sum_rqs`` /
``final`` [A, N, S_max] at the encoded (s', q) = s' * nQ + q (``final`` at s * nQ + q), ``solves`` (``VI_solved``) and
``sweeps`` (``VI_iterations``) [A, N]; the coverage counters as JSON, the longest solve's sweeps among them; for the
policy case the learner seeds and every learner's final generator as the engine's five column words.
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

from multiagent_rlrm.learning_algorithms.qrmax_v2 import QRMax_v2  # noqa: E402

MAX_ITER = 10000  # QRMax_v2.max_num_value_iter
# case -> (config, n_envs, n_steps, reset seed, QRMax_v2 arguments, policy: "hash" or "numpy")
CASES = {
    # a. the runner's own setting on a deterministic world: Kthreshold = 1
    "ow2_t1": ("ow2_final", 2, 600, 81, dict(gamma=0.9, nsamplesTE=1, nsamplesRE=1, VI_delta=1e-4), "hash"),
    # b. QRMAXRM: counterfactual experiences, the shortcut, several newly known pairs and one solve
    "ow3_qrm_t2": ("ow3", 2, 330, 72, dict(gamma=0.8, nsamplesTE=2, nsamplesRE=2, VI_delta=1e-3, use_qrm=True), "hash"),
    # c. FrozenLake: done or truncated is terminal; a final state's row keeps its values until the next solve
    "fl2_open_t3": ("fl2_open", 2, 1300, 73, dict(gamma=0.8, nsamplesTE=3, nsamplesRE=3, VI_delta=1e-3), "hash"),
    # d. select_action on the learner's own generator: the shuffle on every call
    "fl2_numpy_t1": ("fl2", 2, 400, 84, dict(gamma=0.9, nsamplesTE=1, nsamplesRE=1, VI_delta=1e-4), "numpy"),
    # e. a slip world: three and more successors, Q still bit for bit
    "fl2_slip_t3": ("fl2_slip", 2, 500, 85, dict(gamma=0.8, nsamplesTE=3, nsamplesRE=3, VI_delta=1e-3), "hash"),
    # f. the relative convergence test
    "fl2_rel_t2": ("fl2", 2, 400, 86, dict(gamma=0.9, nsamplesTE=2, nsamplesRE=2, VI_delta=1e-3, VI_delta_rel=True),
                   "hash"),
    # g. the RM model needs two samples: a listed successor whose (q, s') was never observed, its mass dropped
    "fl2_slip_tq2": ("fl2_slip", 2, 1500, 90, dict(gamma=0.8, nsamplesTE=3, nsamplesRE=3, nsamplesTQ=2, nsamplesRQ=2,
                                                  VI_delta=1e-3), "hash"),
}


def f32(x):
    return float(np.float32(x)) == float(x)


def dropped_mass(alg):
    """Does the solve about to run meet an (s, q, a) it backs up with a listed successor s1 whose nTQS[q, s1] == 0?"""
    for (s, a), lst in alg.nTSAS_dict.items():
        if not (alg.knownTSA[s, a] and alg.knownRSA[s, a]):
            continue
        for q in range(alg.nQ):
            if alg.knownTSQA[s, q, a] and (s, q) not in alg.final_states and any(alg.nTQS[q, s1] == 0 for s1 in lst):
                return True
    return False


def run(case):
    cfg_name, N, T, seed, kw, policy = CASES[case]
    cfg = G.CONFIGS[cfg_name]
    A = len(cfg["agents"])
    fl = cfg["kind"] == "frozen_lake"
    probe, pagents, _ = G.make_env(cfg)
    W, H = probe.env.grid_width, probe.env.grid_height
    PP = W * H
    nQ = [ag.get_reward_machine().numbers_state() for ag in pagents]
    S = [PP * n for n in nQ]
    S_max = max(S)
    te = kw["nsamplesTE"]
    snap_steps = [T // 3, (2 * T) // 3, T]
    for v in (cfg.get("penalty", 0.0), cfg.get("plants_penalty", 0.0), cfg.get("wall_penalty", 0.0),
              cfg.get("reward_modifier", 1.0)):
        assert f32(v), f"{case}: {v} is not a float32 value"
    seeds = P.learner_seeds(case, A, N)
    q = np.zeros((3, A, N, S_max, 4), np.float64)
    for i in range(A):  # (rows past an agent's own keep the fill)
        q[:, i] = 1.0 * nQ[i] / (1.0 - kw["gamma"])
    n_tsqa = np.zeros((3, A, N, S_max, 4), np.float64)
    known_tsqa = np.zeros((3, A, N, S_max, 4), np.uint8)
    n_tsa = np.zeros((3, A, N, PP, 4), np.float64)
    n_rsa = np.zeros((3, A, N, PP, 4), np.float64)
    sum_rsa = np.zeros((3, A, N, PP, 4), np.float64)
    lists = [[[None] * N for _ in range(A)] for _ in range(3)]
    n_tqs = np.zeros((3, A, N, S_max), np.float64)
    tq_next = np.zeros((3, A, N, S_max), np.int32)
    n_rqs = np.zeros((3, A, N, S_max), np.float64)
    sum_rqs = np.zeros((3, A, N, S_max), np.float64)
    final = np.zeros((3, A, N, S_max), np.uint8)
    solves = np.zeros((3, A, N), np.int64)
    sweeps = np.zeros((3, A, N), np.int64)
    acts = np.zeros((T, A, N), np.int8)
    rng_final = np.zeros((5, A, N), np.uint64)
    cov = dict(solves=0, max_sweeps=0, total_sweeps=0, max_succ=0, resets=0, shortcuts=0, many_known_one_solve=0,
               trunc_final=0, final_row_nonzero=0, flat_draws=0, argmax_picks=0, dropped_mass=0, known_skips=0)
    for e in range(N):
        rm_env, agents, _ = G.make_env(cfg)
        n_known = [0] * A
        for i, ag in enumerate(agents):
            alg = QRMax_v2(state_space_size=S[i], action_space_size=4, gamma=kw["gamma"], VI_delta=kw["VI_delta"],
                           VI_delta_rel=kw.get("VI_delta_rel", False), q_space_size=nQ[i], nsamplesTE=te,
                           nsamplesRE=kw["nsamplesRE"], nsamplesTQ=kw.get("nsamplesTQ", 1),
                           nsamplesRQ=kw.get("nsamplesRQ", 1), seed=int(seeds[i, e]), use_qrm=kw.get("use_qrm", False))
            assert alg.max_num_value_iter == MAX_ITER and alg.R_max == nQ[i]
            ag.set_learning_algorithm(alg)
            alg.learn_init()

            def solve(alg=alg, real=alg.solve_VI):
                before = alg.VI_iterations
                cov["dropped_mass"] += dropped_mass(alg)
                real()
                cov["max_sweeps"] = max(cov["max_sweeps"], alg.VI_iterations - before)
            alg.solve_VI = solve

            def check(*a, i=i, real=alg.check_known):
                r = real(*a)
                n_known[i] += bool(r)
                return r
            alg.check_known = check
        algs = [ag.get_learning_algorithm() for ag in agents]
        need_reset, episode, states = True, 0, None
        for t in range(T):
            if need_reset:
                states, _ = rm_env.reset(G.seed_for(cfg, seed, e, episode))
                states = copy.deepcopy(states)
                cov["resets"] += 1
                need_reset = False
            actions = {}
            for i, ag in enumerate(agents):
                if policy == "hash":
                    a = G.hash_action(seed, t, N, e, A, i)
                    actions[ag.name] = ag.actions_dix()[a]
                else:
                    state = rm_env.env.get_state(ag)
                    _, info = ag.encoder.encode(state)
                    row = algs[i].Q[info["s"], info["q"]]
                    flat = bool(np.all(row == row[0]))
                    st = algs[i].rng.bit_generator.state
                    actions[ag.name] = ag.select_action(state)
                    a = next(k for k, v in ag.actions_dix().items() if v is actions[ag.name])
                    assert algs[i].rng.bit_generator.state != st  # the shuffle advances it on every call
                    cov["flat_draws"] += flat
                    cov["argmax_picks"] += not flat
                acts[t, i, e] = a
            new_states, rewards, terms, truncs, infos = rm_env.step(actions)
            for i, ag in enumerate(agents):
                alg = algs[i]
                terminated = (terms[ag.name] or truncs[ag.name]) if fl else terms[ag.name]
                assert f32(infos[ag.name].get("Renv", 0)) and f32(infos[ag.name]["RQ"]), case
                for x in infos[ag.name].get("qrm_experience", []) if kw.get("use_qrm") else []:
                    assert f32(x[9]), case
                k_before = alg.knownTSQA.copy()
                c_before = (alg.nTSQA.copy(), alg.nTSA.copy(), alg.nTQS.copy())
                s_before, f_before, n_known[i] = alg.VI_solved, len(alg.final_states), 0
                ag.update_policy(state=states[ag.name], action=actions[ag.name], reward=rewards[ag.name],
                                 next_state=new_states[ag.name], terminated=terminated, infos=infos[ag.name])
                assert alg.VI_solved - s_before == (n_known[i] > 0)
                cov["many_known_one_solve"] += n_known[i] >= 2 and alg.VI_solved - s_before == 1
                cov["shortcuts"] += int(((alg.knownTSQA == 1) & (k_before == 0) & (alg.nTSQA < te)).sum())
                cov["trunc_final"] += bool(truncs[ag.name]) and len(alg.final_states) > f_before
                cov["final_row_nonzero"] += any(alg.Q[s_, q_].any() for s_, q_ in alg.final_states)
                cov["known_skips"] += all(np.array_equal(b, c) for b, c in zip(c_before, (alg.nTSQA, alg.nTSA, alg.nTQS)))
            states = copy.deepcopy(new_states)
            if all(terms.values()) or all(truncs.values()):
                need_reset = True
                episode += 1
            if t + 1 in snap_steps:
                k = snap_steps.index(t + 1)
                for i in range(A):
                    alg = algs[i]
                    q[k, i, e, :S[i]] = alg.Q.reshape(S[i], 4)
                    n_tsqa[k, i, e, :S[i]] = alg.nTSQA.reshape(S[i], 4)
                    known_tsqa[k, i, e, :S[i]] = alg.knownTSQA.reshape(S[i], 4)
                    n_tsa[k, i, e], n_rsa[k, i, e], sum_rsa[k, i, e] = alg.nTSA, alg.nRSA, alg.sumRSA
                    lists[k][i][e] = {sa: [(s1, alg.nTSAS[sa[0], sa[1], s1]) for s1 in lst]
                                      for sa, lst in alg.nTSAS_dict.items()}
                    n_tqs[k, i, e, :S[i]] = alg.nTQS.T.reshape(S[i])  # [q, s1] -> s1 * nQ + q
                    n_rqs[k, i, e, :S[i]] = alg.nRQS.T.reshape(S[i])
                    sum_rqs[k, i, e, :S[i]] = alg.sumRQS.T.reshape(S[i])
                    for (q_, s1), lst in alg.nTQSQ_dict.items():
                        assert len(lst) == 1 and alg.nTQSQ[q_, s1, lst[0]] == alg.nTQS[q_, s1]
                        tq_next[k, i, e, s1 * nQ[i] + q_] = lst[0]
                    for s_, q_ in alg.final_states:
                        final[k, i, e, s_ * nQ[i] + q_] = 1
                    solves[k, i, e], sweeps[k, i, e] = alg.VI_solved, alg.VI_iterations
        for i in range(A):
            rng_final[:, i, e] = P.words(algs[i].rng.bit_generator.state)
            cov["solves"] += algs[i].VI_solved
            cov["total_sweeps"] += algs[i].VI_iterations
            cov["max_succ"] = max([cov["max_succ"]] + [len(v) for v in algs[i].nTSAS_dict.values()])
    cov = {k: int(v) for k, v in cov.items()}
    print(f"{case}: {cov}")
    # every case: solves happened, each below the sweep limit; all but the short QRM run went through a reset
    assert cov["solves"] >= 10 and cov["max_sweeps"] < MAX_ITER, (case, cov)
    if case != "ow3_qrm_t2":
        assert cov["resets"] > N, (case, cov)
    if case == "ow3_qrm_t2":
        assert cov["shortcuts"] >= 1 and cov["many_known_one_solve"] >= 1, (case, cov)
    if case == "fl2_open_t3":
        assert cov["trunc_final"] >= 1 and cov["final_row_nonzero"] >= 1, (case, cov)
    if case == "fl2_numpy_t1":
        assert cov["flat_draws"] >= 10 and cov["argmax_picks"] >= 10, (case, cov)
    if case == "fl2_slip_t3":
        assert cov["max_succ"] >= 3, (case, cov)
    if case == "fl2_slip_tq2":
        assert cov["dropped_mass"] >= 1, (case, cov)
    K = max(cov["max_succ"], 1)
    t_idx = np.zeros((3, A, N, PP, 4, K), np.int32)
    t_cnt = np.zeros((3, A, N, PP, 4, K), np.int32)
    for k, i, e in np.ndindex(3, A, N):
        for (s, a), lst in lists[k][i][e].items():
            for j, (s1, c) in enumerate(lst):
                assert float(c) == int(c) and c > 0
                t_idx[k, i, e, s, a, j] = s1
                t_cnt[k, i, e, s, a, j] = int(c)
    ints = dict(n_tsa=n_tsa, n_rsa=n_rsa, n_tqs=n_tqs, n_rqs=n_rqs, n_tsqa=n_tsqa)
    out = dict(actions=acts, seed=np.int64(seed), config=np.array(cfg_name), scenario=np.array(json.dumps(cfg)),
               gamma=np.float64(kw["gamma"]), nsamples=np.asarray([te, kw["nsamplesRE"], kw.get("nsamplesTQ", 1),
                                                                    kw.get("nsamplesRQ", 1)], np.int32),
               vi_delta=np.float64(kw["VI_delta"]), vi_delta_rel=np.int32(bool(kw.get("VI_delta_rel", False))),
               use_qrm=np.int32(bool(kw.get("use_qrm", False))), max_reward=np.float64(1.0),
               trunc_is_terminal=np.int32(fl), snap_steps=np.asarray(snap_steps, np.int32),
               n_states=np.asarray(S, np.int32), q=q, known_tsqa=known_tsqa, sum_rsa=sum_rsa, t_idx=t_idx, t_cnt=t_cnt,
               tq_next=tq_next, sum_rqs=sum_rqs, final=final, solves=solves, sweeps=sweeps,
               coverage=np.array(json.dumps(cov)), **{k: v.astype(np.int32) for k, v in ints.items()})
    for k, v in ints.items():
        assert np.array_equal(out[k].astype(np.float64), v), k
    if policy == "numpy":
        out.update(policy_seeds=seeds, rng_final=rng_final)
    return out


def main(only=None):
    for case in only or CASES:
        out = run(case)
        path = os.path.join(HERE, f"qrmax_{case}.npz")
        G._savez(path, **out)
        assert os.path.getsize(path) < 727 * 1024, (case, os.path.getsize(path))
        print("  ", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
