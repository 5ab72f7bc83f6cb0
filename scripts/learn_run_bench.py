"""Time 1,000 learn steps as 1,000 act_step calls (parent commit and this one) and as ONE run(1000) (this commit), at
64, 4,096 and 65,536 envs, and write profiles/learn_run.md.

    python scripts/learn_run_bench.py --parent DIR [--steps 1000] [--trials 7] [--out FILE]

DIR is a built checkout of the parent commit (its multiagent-rl-rm_amd/rmx/librmx.so in place).  BASELINE config 2
(FrozenLake map1, 2 agents), QRM learner, lr 0.1, epsilon 0.1, with the engine's policy and with the reference's numpy
stream (a seed per learner); one Q(lambda) row (lambda 0.8, the engine's policy) at 4,096 envs.  Each window of `steps`
steps is timed by device events and by the host's clock (the call that starts the window to the end of the
synchronisation after it), after a warm-up window.  Every tree is measured in processes of its own (one library per
process): parent, this commit, parent, this commit, each with half the trials (this commit's two variants alternate
trial by trial), so that a drift of the machine and the difference between two processes both show up as spread of
(a).  Not bench.py: this measures the learner, bench.py the flagship step.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (64, 4096, 65536)
LAMBDA_N = 4096


def measure(tree, steps, trials):
    """In a child process: us per step of every trial (device events, host clock), per configuration and variant,
    with the package of `tree`."""
    sys.path.insert(0, os.path.join(tree, "multiagent-rl-rm_amd"))
    import numpy as np
    import torch

    from rmx import tables as T
    from rmx.engine import VecRMEnv
    from rmx.learn import VecQLambda, VecQLearning

    if not torch.cuda.is_available():
        raise SystemExit("learn_run_bench.py needs the GPU: nothing is measured without one")
    tab = T.compile_scenario(T.baseline_scenario(2))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    result = {}

    def seeds(n):  # a seed per learner (one seed everywhere would make every env the same run)
        return np.arange(2 * n, dtype=np.uint64).reshape(2, n) + 2020

    configs = [(f"{p}/{n}", n, p) for n in SIZES for p in ("engine", "stream")] + [(f"lambda/{LAMBDA_N}", LAMBDA_N, "lambda")]
    for key, n, policy in configs:
        env = VecRMEnv(tab, n)
        if policy == "lambda":
            L = VecQLambda(env, 0.9, 0.8, 0.1)
        else:
            L = VecQLearning(env, 0.9, 0.1, use_qrm=True, policy_seeds=seeds(n) if policy == "stream" else None)

        def by_steps(t0, L=L, policy=policy):
            if policy == "stream":
                for _ in range(steps):
                    L.act_step(0.1, reference_stream=True)
            else:
                for k in range(steps):
                    L.act_step(0.1, 3, t0 + k)

        def by_run(t0, L=L, policy=policy):
            if policy == "stream":
                L.run(steps, 0.1, reference_stream=True)
            else:
                L.run(steps, 0.1, 3, t0)

        variants = {"step": by_steps}
        if hasattr(L, "run"):
            variants["run"] = by_run
        dev = {k: [] for k in variants}
        wall = {k: [] for k in variants}
        t = 0
        for trial in range(trials + 1):  # trial 0 warms every variant up
            for name, window in variants.items():
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                ev0.record()
                window(t)
                ev1.record()
                ev1.synchronize()
                w1 = time.perf_counter()
                t += steps
                if trial:
                    dev[name].append(ev0.elapsed_time(ev1) * 1e3 / steps)
                    wall[name].append((w1 - w0) * 1e6 / steps)
        env.check_errors()
        result[key] = {"dev": dev, "wall": wall}
        env.close()
        del L, env, by_steps, by_run, variants
        torch.cuda.empty_cache()
    print("TIMES " + json.dumps({"device": torch.cuda.get_device_name(0), "times": result}))


def child(tree, args, trials):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, "--steps", str(args.steps), "--trials", str(trials)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
    if r.returncode != 0:
        raise SystemExit(f"measuring {tree} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    print(f"measured {tree} ({trials} trials)", file=sys.stderr, flush=True)
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("TIMES "))[6:])


def fmt(ts):
    return f"{statistics.median(ts):.2f} ({min(ts):.2f} - {max(ts):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_run.md"))
    args = ap.parse_args()
    if args.child:
        return measure(args.child, args.steps, args.trials)
    if not args.parent or not os.path.exists(os.path.join(args.parent, "multiagent-rl-rm_amd", "rmx", "librmx.so")):
        raise SystemExit("--parent must be a built checkout of the parent commit")
    first = (args.trials + 1) // 2
    runs = [child(args.parent, args, first), child(ROOT, args, first)]
    if args.trials > first:
        runs += [child(args.parent, args, args.trials - first), child(ROOT, args, args.trials - first)]

    def series(key, kind, which):
        procs = runs[0::2] if which == "a" else runs[1::2]
        variant = "run" if which == "c" else "step"
        return sum((r["times"][key][kind][variant] for r in procs), [])

    lines = ["# T learn steps in one launch: run(1000) against 1,000 act_step calls", "",
             f"{runs[1]['device']}; BASELINE config 2 tables, 2 agents, QRM learner (lr 0.1, visits counted), epsilon "
             f"0.1; windows of {args.steps} steps on one stream, device events, {args.trials} trials per variant after a "
             "warm-up window; four processes in turn (parent, this commit, parent, this commit), each with half the "
             "trials and a warm-up window of its own; the numpy stream with one generator seed per learner.  (a) "
             f"{args.steps} act_step calls on the parent commit, (b) the same on this commit, (c) one run({args.steps}) "
             "on this commit.  The margin is (a)'s own min - max trial spread.", "",
             "| policy | envs | (a) us / step: median (min - max) | (b) | (c) | (c) / (a) | (b) within (a)'s spread | "
             "(c) faster than (a) by more than the spread |", "|---|---|---|---|---|---|---|---|"]
    raw = []
    keys = [(p, n) for n in SIZES for p in ("engine", "stream")] + [("lambda", LAMBDA_N)]
    for p, n in keys:
        key = f"{p}/{n}"
        a, b, c = (series(key, "dev", w) for w in "abc")
        ma, mb, mc = (statistics.median(x) for x in (a, b, c))
        spread = max(a) - min(a)
        inside = min(a) <= mb <= max(a)
        faster = ma - mc > spread
        name = {"engine": "engine's policy", "stream": "numpy stream", "lambda": "Q(lambda), engine's policy"}[p]
        lines.append(f"| {name} | {n} | {fmt(a)} | {fmt(b)} | {fmt(c)} | {mc / ma:.3f} | "
                     f"{'yes' if inside else 'NO'} (b / a = {mb / ma:.4f}) | {'yes' if faster else 'NO'} "
                     f"(a - c = {ma - mc:.2f}, spread {spread:.2f}) |")
        raw.append(f"{name}, {n} envs: (a) " + ", ".join(f"{x:.2f}" for x in a) + "; (b) " +
                   ", ".join(f"{x:.2f}" for x in b) + "; (c) " + ", ".join(f"{x:.2f}" for x in c) + ".")
    lines += ["", "Host wall-clock per window at 64 envs (us / step, the first call of the window to the end of the "
              "synchronisation after it; the device-event time of a window of single steps already contains the gaps "
              "between launches that the host leaves):", "",
              "| policy | (a) wall us / step | (c) wall us / step | (c) / (a) |", "|---|---|---|---|"]
    for p in ("engine", "stream"):
        a, c = series(f"{p}/64", "wall", "a"), series(f"{p}/64", "wall", "c")
        lines.append(f"| {p} | {fmt(a)} | {fmt(c)} | {statistics.median(c) / statistics.median(a):.3f} |")
        raw.append(f"wall, {p}, 64 envs: (a) " + ", ".join(f"{x:.2f}" for x in a) + "; (c) " +
                   ", ".join(f"{x:.2f}" for x in c) + ".")
    lines += ["", "Trials in order, us / step:", ""] + [f"- {r}" for r in raw]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
