"""Time the R-max learn step (csrc/rmx_learn_rmax.hip: the step kernel plus the solve kernel) beside the QRM
Q-learning learn step at the same shapes, and print the tables of profiles/learn_rmax.md.

    python scripts/learn_rmax_bench.py [--envs 64,4096,65536] [--steps 200] [--trials 5] [--first 12] [--out FILE]

BASELINE config 2 (FrozenLake map1, 2 agents) with use_qrm, gamma 0.9, vi_delta 1e-4, the engine's hashed policy.
Steady state, per size, windows of `steps` learn steps on one stream timed by device events after a warm-up window,
the variants alternating trial by trial, each on a handle of its own:
  * "R-max, learning": s_a_threshold far above anything the windows reach: every step updates counts, reward sums and
    successor lists, no pair crosses, the solve kernel finds an empty worklist;
  * "R-max, all known": counts filled with the threshold: every update_q returns at its first test (a converged run);
  * "QRM Q-learning": VecQLearning(use_qrm=True).act_step, the yardstick (its kernels are csrc/rmx_learn.hip's).
The first steps: a fresh model with s_a_threshold = 1, each of the first `first` steps timed on its own (device events
around the step's two launches), with the solves and the longest solve's sweeps read after each step (that read
synchronises and is outside the events).  Not bench.py: this measures the learner, bench.py the flagship step.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multiagent-rl-rm_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="64,4096,65536")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--first", type=int, default=12)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from rmx import tables as T
    from rmx.engine import VecRMEnv
    from rmx.learn import VecQLearning, VecRMax

    if not torch.cuda.is_available():
        raise SystemExit("learn_rmax_bench.py needs the GPU: nothing is measured without one")
    tab = T.compile_scenario(T.baseline_scenario(2))
    A, K = tab.n_agents, args.steps
    S_max = tab.width * tab.height * int(max(tab.enc_nq))
    cap = 5
    per_learner = S_max * 4 * (24 + 8 * cap)
    free = torch.cuda.mem_get_info()[0]
    lines = [f"{torch.cuda.get_device_name(0)}; BASELINE config 2 tables, {A} agents, S_max = {S_max}, use_qrm, gamma 0.9, "
             f"vi_delta 1e-4, the engine's hashed policy; windows of {K} learn steps on one stream, device events, "
             f"{args.trials} alternating trials after a warm-up window.", "",
             f"Memory per learner: S_max * 4 * (24 + 8 * cap) = {per_learner} B at cap {cap} (q, counts, rsum, the two "
             f"lists); {free / 1e9:.0f} GB free: {int(0.9 * free // (A * per_learner))} envs of {A} learners fit in 90 % "
             "of it.", "",
             "| envs | learn step | us / step: median (min - max) | ns / learner-step |", "|---|---|---|---|"]
    first_lines = ["| envs | step | us | solves in the step | longest solve so far (sweeps) |", "|---|---|---|---|---|"]
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for N in (int(v) for v in args.envs.split(",")):
        envs = [VecRMEnv(tab, N) for _ in range(3)]
        for e in envs:
            e.reset(seed=1)
        learn = VecRMax(envs[0], 0.9, s_a_threshold=1 << 30, use_qrm=True)
        known = VecRMax(envs[1], 0.9, s_a_threshold=3, use_qrm=True)
        known.counts.fill_(3.0)
        qrm = VecQLearning(envs[2], 0.9, 0.1, use_qrm=True)
        t_global = [0]
        variants = {"R-max, learning": lambda t: learn.act_step(None, 3, t),
                    "R-max, all known": lambda t: known.act_step(None, 3, t),
                    "QRM Q-learning": lambda t: qrm.act_step(0.1, 3, t)}
        times = {k: [] for k in variants}
        for trial in range(args.trials + 1):  # trial 0 warms every variant up
            for name, fn in variants.items():
                ev0.record()
                for k in range(K):
                    fn(t_global[0] + k)
                ev1.record()
                ev1.synchronize()
                if trial:
                    times[name].append(ev0.elapsed_time(ev1) * 1e3 / K)
            t_global[0] += K
        assert learn.solve_info()[0] == 0 and known.solve_info()[0] == 0  # no crossing in either steady state
        for name, ts in times.items():
            med = statistics.median(ts)
            lines.append(f"| {N} | {name} | {med:.2f} ({min(ts):.2f} - {max(ts):.2f}) | {med * 1e3 / (A * N):.3f} |")
        for e in envs:
            e.check_errors()
            e.close()
        del learn, known, qrm, envs
        torch.cuda.empty_cache()
        # the first steps of a fresh model at threshold 1
        env = VecRMEnv(tab, N)
        env.reset(seed=1)
        L = VecRMax(env, 0.9, s_a_threshold=1, use_qrm=True)
        L.act_step(None, 3, 0, learn=False, autoreset=False)  # (loads the step kernel; the model is untouched)
        env.reset(seed=1)
        done = 0
        for t in range(args.first):
            ev0.record()
            L.act_step(None, 3, t)
            ev1.record()
            ev1.synchronize()
            solves, sweeps = L.solve_info()
            first_lines.append(f"| {N} | {t} | {ev0.elapsed_time(ev1) * 1e3:.1f} | {solves - done} | {sweeps} |")
            done = solves
        env.check_errors()
        env.close()
        del L, env
        torch.cuda.empty_cache()
    text = "\n".join(lines + ["", "The first steps of a fresh model, s_a_threshold = 1:", ""] + first_lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
