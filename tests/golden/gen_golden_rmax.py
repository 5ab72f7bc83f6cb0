"""Record R-max learner fixtures by running the REFERENCE's own RMax behind AgentRL.update_policy (needs the reference
checkout that gen_golden.py imports; the fixtures, not the reference, travel with the tests).

Imports ``gen_golden`` (the reference with the offline stubs) for ``make_env``, ``hash_action`` and ``seed_for``,
attaches the reference's real ``RMax`` (learning_algorithms/rmax.py) to every agent, as office_main.py:663-684 builds
it for ``--algorithm RMAX`` / ``RMAXRM``, and runs the runner's loop (office_main.py:1696-1749,
frozen_lake_main.py:336-376): hashed actions, or ``select_action`` for every agent on the learner's own generator;
``rm_env.step``; ``update_policy`` for every agent; ``reset(seed of the episode)`` before the step that follows an
episode's end (which does nothing to an RMax).  The update is never restated here: the tables saved are the learners'
own ``q_table`` / ``s_a_counts`` / ``rewards`` / ``transitions``; solves are counted by wrapping the learner's
``value_iteration`` and sweeps by counting the ``np.einsum`` calls inside it, and the coverage each case asserts is
read off the learner's tables around the reference's calls.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_rmax.py [case ...]

Each case is saved as ``rmax_<case>.npz``: the actions [T, A, N], the learner parameters, and after the steps
``snap_steps`` ``q`` [3, A, N, S_max, 4], ``counts`` and ``rsum`` likewise, the non-zero entries of ``transitions`` as
lists in successor order (``t_idx`` / ``t_cnt`` [3, A, N, S_max, 4, K], K the largest number of successors), the number
of solves [3, A, N]; the largest sweep count of any solve, the largest number of successors of any (s, a) and the
other coverage counters as JSON; for the policy case the learner seeds and every learner's final generator as the
engine's five column words.
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

from multiagent_rlrm.learning_algorithms.rmax import RMax  # noqa: E402

MAX_ITER = 10000  # RMax.max_num_value_iter
# case -> (config, n_envs, n_steps, reset seed, RMax arguments, policy: "hash" or "numpy")
CASES = {
    # a. the runner's own setting on a deterministic world: Kthreshold = 1 (office_main.py:371)
    "ow2_t1": ("ow2_final", 2, 1100, 71, dict(gamma=0.9, s_a_threshold=1, VI_delta=1e-4), "hash"),
    # b. RMAXRM: counterfactual experiences; an agent-step crosses twice
    "ow3_qrm_t2": ("ow3", 2, 330, 72, dict(gamma=0.8, s_a_threshold=2, VI_delta=1e-3, use_qrm=True), "hash"),
    # c. FrozenLake: done or truncated is terminal; a truncation overrides a state that already has counts
    "fl2_open_t3": ("fl2_open", 2, 1300, 73, dict(gamma=0.8, s_a_threshold=3, VI_delta=1e-3), "hash"),
    # d. select_action on the learner's own generator
    "fl2_numpy_t1": ("fl2", 2, 600, 74, dict(gamma=0.9, s_a_threshold=1, VI_delta=1e-4), "numpy"),
    # e. a slip world: three and more successors, q within the derived bound only
    "fl2_slip_t3": ("fl2_slip", 2, 500, 75, dict(gamma=0.8, s_a_threshold=3, VI_delta=1e-3), "hash"),
    # f. the relative convergence test
    "fl2_rel_t2": ("fl2", 2, 600, 76, dict(gamma=0.9, s_a_threshold=2, VI_delta=1e-3, VI_delta_rel=True), "hash"),
}


def f32(x):
    return float(np.float32(x)) == float(x)


class Counting:
    """np.einsum, counted: value_iteration calls it once per sweep and nothing else here calls it."""

    def __init__(self):
        self.real, self.calls = np.einsum, 0

    def __call__(self, *a, **k):
        self.calls += 1
        return self.real(*a, **k)


def run(case):
    cfg_name, N, T, seed, kw, policy = CASES[case]
    cfg = G.CONFIGS[cfg_name]
    A = len(cfg["agents"])
    fl = cfg["kind"] == "frozen_lake"
    probe, pagents, _ = G.make_env(cfg)
    W, H = probe.env.grid_width, probe.env.grid_height
    S = [W * H * ag.get_reward_machine().numbers_state() for ag in pagents]
    S_max = max(S)
    thr = kw["s_a_threshold"]
    snap_steps = [T // 3, (2 * T) // 3, T]
    for v in (cfg.get("penalty", 0.0), cfg.get("plants_penalty", 0.0), cfg.get("wall_penalty", 0.0),
              cfg.get("reward_modifier", 1.0)):
        assert f32(v), f"{case}: {v} is not a float32 value"
    seeds = P.learner_seeds(case, A, N)
    q = np.full((3, A, N, S_max, 4), 1.0 / (1.0 - kw["gamma"]), np.float64)  # (rows past an agent's own keep the fill)
    counts = np.zeros((3, A, N, S_max, 4), np.float64)
    rsum = np.zeros((3, A, N, S_max, 4), np.float64)
    trans = [[[None] * N for _ in range(A)] for _ in range(3)]
    solves = np.zeros((3, A, N), np.int64)
    acts = np.zeros((T, A, N), np.int8)
    rng_final = np.zeros((5, A, N), np.uint64)
    cov = dict(solves=0, max_sweeps=0, max_succ=0, double_cross=0, term_over_counts=0, terminal_updates=0,
               trunc_terminal=0, known_skips=0, flat_draws=0, argmax_picks=0, resets=0)
    counter = Counting()
    np.einsum = counter
    try:
        for e in range(N):
            rm_env, agents, _ = G.make_env(cfg)
            n_solves = [0] * A
            for i, ag in enumerate(agents):
                alg = RMax(state_space_size=S[i], action_space_size=4, seed=int(seeds[i, e]), **kw)
                assert alg.max_num_value_iter == MAX_ITER
                ag.set_learning_algorithm(alg)

                def counted(alg=alg, i=i, real=alg.value_iteration):
                    before = counter.calls
                    real()
                    n_solves[i] += 1
                    cov["max_sweeps"] = max(cov["max_sweeps"], counter.calls - before)
                alg.value_iteration = counted
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
                        st = algs[i].rng.bit_generator.state
                        actions[ag.name] = ag.select_action(rm_env.env.get_state(ag))
                        a = next(k for k, v in ag.actions_dix().items() if v is actions[ag.name])
                        drew = algs[i].rng.bit_generator.state != st
                        cov["flat_draws"] += drew
                        cov["argmax_picks"] += not drew
                    acts[t, i, e] = a
                new_states, rewards, terms, truncs, infos = rm_env.step(actions)
                for i, ag in enumerate(agents):
                    alg = algs[i]
                    terminated = (terms[ag.name] or truncs[ag.name]) if fl else terms[ag.name]
                    assert f32(infos[ag.name].get("Renv", 0)) and f32(infos[ag.name]["RQ"]), case
                    for x in infos[ag.name].get("qrm_experience", []) if kw.get("use_qrm") else []:
                        assert f32(x[9]), case
                    c_before = alg.s_a_counts.copy()
                    n_before = n_solves[i]
                    ag.update_policy(state=states[ag.name], action=actions[ag.name], reward=rewards[ag.name],
                                     next_state=new_states[ag.name], terminated=terminated, infos=infos[ag.name])
                    cov["double_cross"] += n_solves[i] - n_before >= 2
                    if terminated:
                        cov["terminal_updates"] += 1
                        cov["trunc_terminal"] += bool(truncs[ag.name])
                        # rows that went to the threshold in all four columns at once had counts below it before
                        over = np.flatnonzero((alg.s_a_counts == thr).all(axis=1) & (c_before < thr).any(axis=1)
                                              & (c_before > 0).any(axis=1))
                        cov["term_over_counts"] += int(over.size > 0)
                    cov["known_skips"] += bool(np.array_equal(c_before, alg.s_a_counts))
                states = copy.deepcopy(new_states)
                if all(terms.values()) or all(truncs.values()):
                    need_reset = True
                    episode += 1
                if t + 1 in snap_steps:
                    k = snap_steps.index(t + 1)
                    for i in range(A):
                        q[k, i, e, :S[i]] = algs[i].q_table
                        counts[k, i, e, :S[i]] = algs[i].s_a_counts
                        rsum[k, i, e, :S[i]] = algs[i].rewards
                        trans[k][i][e] = [np.array(v) for v in np.nonzero(algs[i].transitions)] + \
                            [algs[i].transitions[np.nonzero(algs[i].transitions)]]
                        solves[k, i, e] = n_solves[i]
            for i in range(A):
                rng_final[:, i, e] = P.words(algs[i].rng.bit_generator.state)
                cov["solves"] += n_solves[i]
                cov["max_succ"] = max(cov["max_succ"], int(np.count_nonzero(algs[i].transitions, axis=-1).max()))
    finally:
        np.einsum = counter.real
    cov = {k: int(v) for k, v in cov.items()}
    print(f"{case}: {cov}")
    # every case: solves happened, each below the sweep limit, and the run went through a reset
    assert cov["solves"] >= 10 and cov["max_sweeps"] < MAX_ITER and cov["resets"] > N, (case, cov)
    if case in ("ow2_t1", "ow3_qrm_t2", "fl2_open_t3", "fl2_numpy_t1", "fl2_rel_t2"):
        assert cov["max_succ"] <= 2, (case, cov)  # q is compared bit for bit
    if case == "ow3_qrm_t2":
        assert cov["double_cross"] >= 1, (case, cov)
    if case == "fl2_open_t3":
        assert cov["trunc_terminal"] >= 1 and cov["term_over_counts"] >= 1, (case, cov)
    if case == "fl2_numpy_t1":
        assert cov["flat_draws"] >= 10 and cov["argmax_picks"] >= 10, (case, cov)
    if case == "fl2_slip_t3":
        assert cov["max_succ"] >= 3, (case, cov)
    # the transitions as lists: the non-zero entries of each (s, a) row in successor order
    K = max(cov["max_succ"], 1)
    t_idx = np.zeros((3, A, N, S_max, 4, K), np.int32)
    t_cnt = np.zeros((3, A, N, S_max, 4, K), np.int32)
    for k, i, e in np.ndindex(3, A, N):
        s_, a_, n_, c_ = trans[k][i][e]
        fill = np.zeros((S_max, 4), np.int64)
        for s, a, n, c in zip(s_, a_, n_, c_):
            assert float(c) == int(c) and c > 0
            t_idx[k, i, e, s, a, fill[s, a]] = n
            t_cnt[k, i, e, s, a, fill[s, a]] = int(c)
            fill[s, a] += 1
    out = dict(actions=acts, seed=np.int64(seed), config=np.array(cfg_name), scenario=np.array(json.dumps(cfg)),
               gamma=np.float64(kw["gamma"]), threshold=np.int32(thr), vi_delta=np.float64(kw["VI_delta"]),
               vi_delta_rel=np.int32(bool(kw.get("VI_delta_rel", False))), use_qrm=np.int32(bool(kw.get("use_qrm", False))),
               max_reward=np.float64(1.0), trunc_is_terminal=np.int32(fl), snap_steps=np.asarray(snap_steps, np.int32),
               n_states=np.asarray(S, np.int32), q=q, counts=counts.astype(np.uint32), rsum=rsum, t_idx=t_idx,
               t_cnt=t_cnt, solves=solves, coverage=np.array(json.dumps(cov)))
    assert np.array_equal(out["counts"].astype(np.float64), counts)
    if policy == "numpy":
        out.update(policy_seeds=seeds, rng_final=rng_final)
    return out


def main(only=None):
    for case in only or CASES:
        out = run(case)
        path = os.path.join(HERE, f"rmax_{case}.npz")
        G._savez(path, **out)
        assert os.path.getsize(path) < 727 * 1024, (case, os.path.getsize(path))
        print("  ", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
