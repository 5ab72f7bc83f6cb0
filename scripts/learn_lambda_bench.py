"""Time the Q(lambda) learn step (the step and every learner's sweep over its sparse trace list in one launch) beside
the same handle's plain Q-learning learn step, and write profiles/learn_lambda.md.

    python scripts/learn_lambda_bench.py [--envs N] [--steps 200] [--trials 7] [--cap L] [--out profiles/learn_lambda.md]

BASELINE config 2 (FrozenLake map1, 2 agents), lambda = 0.8, gamma = 0.9, lr 0.1, the engine's policy with epsilon 0.1.
--envs defaults to the largest power of two whose tables (q, visits, the trace lists at --cap slots, default the
4 * S_max that cannot overflow) fit in 60 % of the free device memory.  Each window of `steps` launches is timed by
device events after a warm-up window; the two variants alternate, trial by trial, on ONE handle and one pair of
tables: the lists are unbound for the Q-learning windows and bound again (and emptied) for the Q(lambda) ones.  The
list lengths are read after every Q(lambda) window.  Not bench.py: this measures the learner, bench.py the flagship
step.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multiagent-rl-rm_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--cap", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_lambda.md"))
    args = ap.parse_args()

    import torch

    from rmx import tables as T
    from rmx.engine import VecRMEnv
    from rmx.learn import VecQLambda

    if not torch.cuda.is_available():
        raise SystemExit("learn_lambda_bench.py needs the GPU: nothing is measured without one")
    tab = T.compile_scenario(T.baseline_scenario(2))
    A, K = tab.n_agents, args.steps
    S_max = tab.width * tab.height * int(max(tab.enc_nq))
    cap = args.cap or 4 * S_max
    per_env = A * (2 * S_max * 4 * 8 + cap * 12 + 4)  # q, visits, trace_idx + trace_val, trace_cnt
    free = torch.cuda.mem_get_info()[0]
    N = args.envs
    if not N:
        N = 1
        while 2 * N * per_env <= 0.6 * free:
            N *= 2
    env = VecRMEnv(tab, N)
    L = VecQLambda(env, 0.9, 0.8, 0.1, trace_cap=cap)
    lists = (L.trace_idx, L.trace_val, L.trace_cnt, cap)
    t_global = [0]

    def window():
        for _ in range(K):
            L.act_step(0.1, 3, t_global[0])
            t_global[0] += 1

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {"Q(lambda)": [], "Q-learning": []}
    means, maxima = [], []
    for trial in range(args.trials + 1):  # trial 0 warms both variants up
        for name in times:
            if name == "Q(lambda)":
                L.bind_traces(*lists)
                L.clear_traces()
            else:
                L.unbind_traces()
            ev0.record()
            window()
            ev1.record()
            ev1.synchronize()
            if trial:
                times[name].append(ev0.elapsed_time(ev1) * 1e3 / K)
                if name == "Q(lambda)":
                    means.append(float(L.trace_cnt.double().mean()))
                    maxima.append(int(L.trace_cnt.max()))
    env.check_errors()
    gb = N * per_env / 1e9
    lines = ["# The Q(lambda) learn step beside the Q-learning learn step", "",
             f"{torch.cuda.get_device_name(0)}; BASELINE config 2 tables, {N} envs x {A} agents (the largest power of two "
             f"whose tables fit: {gb:.1f} GB of q, visits and trace lists at {cap} slots per learner, "
             f"{free / 1e9:.0f} GB free), lambda 0.8, gamma 0.9, lr 0.1, the engine's policy with epsilon 0.1; windows of "
             f"{K} launches on one stream, device events, {args.trials} alternating trials after a warm-up window; one "
             "handle and one pair of tables for both variants (the lists unbound for the Q-learning windows).", "",
             f"    python scripts/learn_lambda_bench.py --envs {N} --steps {K} --trials {args.trials} --cap {cap}", "",
             "| learn step | us / step: median (min - max) | ns / learner-step |", "|---|---|---|"]
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"| {name} | {med:.2f} ({min(ts):.2f} - {max(ts):.2f}) | {med * 1e3 / (A * N):.3f} |")
    ratio = statistics.median(times["Q(lambda)"]) / statistics.median(times["Q-learning"])
    lines += ["", f"Ratio Q(lambda) / Q-learning: {ratio:.2f}.", "",
              f"List length after each Q(lambda) window of {K} steps (every learner, the lists emptied before the "
              f"window): mean {statistics.mean(means):.1f} (windows: {min(means):.1f} - {max(means):.1f}), maximum "
              f"{max(maxima)}.", "",
              "A sweep reads and writes 12 B of list and gathers / scatters one 8-B table cell per live trace; the "
              f"reference's dense update sweeps two whole tables, q and e: {2 * A * S_max * 4 * 8 * N / 1e9:.1f} GB read "
              "and written per step at this size."]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
