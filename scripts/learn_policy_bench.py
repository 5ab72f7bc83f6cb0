"""Time the policy learn step with the engine's own policy on the parent commit and on this one, and with the
reference's numpy stream (act_step(reference_stream=True)) on this one, and write profiles/learn_policy_stream.md.

    python scripts/learn_policy_bench.py --parent DIR [--envs 65536] [--steps 200] [--trials 7] [--out FILE]

DIR is a built checkout of the parent commit (its multiagent-rl-rm_amd/rmx/librmx.so in place).  BASELINE config 2
(FrozenLake map1, 2 agents), QRM learner, lr 0.1, epsilon 0.1; each window of `steps` launches is timed by device
events after a warm-up window.  Every tree is measured in processes of its own (one library per process): parent, this
commit, parent, this commit, each with half the trials (this commit's two variants alternate trial by trial), so that
a drift of the machine and the difference between two processes both show up as spread of (a).  Not bench.py: this
measures the learner, bench.py the flagship step.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(tree, envs, steps, trials, stream):
    """In a child process: us per step of every trial, per variant, with the package of `tree`."""
    sys.path.insert(0, os.path.join(tree, "multiagent-rl-rm_amd"))
    import torch

    from rmx import tables as T
    from rmx.engine import VecRMEnv
    from rmx.learn import VecQLearning

    if not torch.cuda.is_available():
        raise SystemExit("learn_policy_bench.py needs the GPU: nothing is measured without one")
    tab = T.compile_scenario(T.baseline_scenario(2))
    variants = {}
    env = VecRMEnv(tab, envs)
    L = VecQLearning(env, 0.9, 0.1, use_qrm=True)
    variants["engine"] = (env, lambda t: L.act_step(0.1, 3, t))
    if stream:
        env2 = VecRMEnv(tab, envs)
        import numpy as np
        # a seed per learner (the same seed everywhere would make every env the same run: no divergence, one access
        # pattern)
        L2 = VecQLearning(env2, 0.9, 0.1, use_qrm=True,
                          policy_seeds=np.arange(2 * envs, dtype=np.uint64).reshape(2, envs) + 2020)
        variants["stream"] = (env2, lambda t: L2.act_step(0.1, reference_stream=True))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in variants}
    t = 0
    for trial in range(trials + 1):  # trial 0 warms every variant up
        for name, (_, step) in variants.items():
            ev0.record()
            for k in range(steps):
                step(t + k)
            ev1.record()
            ev1.synchronize()
            if trial:
                times[name].append(ev0.elapsed_time(ev1) * 1e3 / steps)
        t += steps
    for e, _ in variants.values():
        e.check_errors()
    print("TIMES " + json.dumps({"device": torch.cuda.get_device_name(0), "times": times}))


def child(tree, args, trials, stream):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, "--envs", str(args.envs), "--steps", str(args.steps),
           "--trials", str(trials)] + (["--stream"] if stream else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    if r.returncode != 0:
        raise SystemExit(f"measuring {tree} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("TIMES "))[6:])


def fmt(ts):
    return f"{statistics.median(ts):.2f} ({min(ts):.2f} - {max(ts):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--stream", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_policy_stream.md"))
    args = ap.parse_args()
    if args.child:
        return measure(args.child, args.envs, args.steps, args.trials, args.stream)
    if not args.parent or not os.path.exists(os.path.join(args.parent, "multiagent-rl-rm_amd", "rmx", "librmx.so")):
        raise SystemExit("--parent must be a built checkout of the parent commit")
    first = (args.trials + 1) // 2
    runs = [child(args.parent, args, first, False), child(ROOT, args, first, True)]
    if args.trials > first:
        runs += [child(args.parent, args, args.trials - first, False), child(ROOT, args, args.trials - first, True)]
    here = runs[1]
    a = sum((r["times"]["engine"] for r in runs[0::2]), [])
    b = sum((r["times"]["engine"] for r in runs[1::2]), [])
    c = sum((r["times"]["stream"] for r in runs[1::2]), [])
    med_a, med_b, med_c = (statistics.median(x) for x in (a, b, c))
    inside = min(a) <= med_b <= max(a)
    N = args.envs
    lines = ["# The policy learn step: the engine's policy before and after, and the reference's numpy stream", "",
             f"{here['device']}; BASELINE config 2 tables, {N} envs x 2 agents, QRM learner (lr 0.1, visits counted), "
             f"epsilon 0.1, windows of {args.steps} launches on one stream, device events, {args.trials} trials per variant "
             "after a warm-up window; four processes in turn (parent, this commit, parent, this commit), each with "
             "half the trials and a warm-up window of its own; one numpy generator seed per learner.", "",
             "| variant | us / step: median (min - max) |", "|---|---|",
             f"| (a) act_step, the engine's policy, parent commit | {fmt(a)} |",
             f"| (b) act_step, the engine's policy, this commit | {fmt(b)} |",
             f"| (c) act_step(reference_stream=True), this commit | {fmt(c)} |", "",
             "Trials in order, us / step: (a) " + ", ".join(f"{x:.2f}" for x in a) + "; (b) " +
             ", ".join(f"{x:.2f}" for x in b) + "; (c) " + ", ".join(f"{x:.2f}" for x in c) + ".", "",
             f"Trial-to-trial spread of (a): {max(a) - min(a):.2f} us ({min(a):.2f} - {max(a):.2f}).  The median of (b), "
             f"{med_b:.2f} us, lies {'inside' if inside else 'OUTSIDE'} it (b / a = {med_b / med_a:.4f}).  The two earlier "
             "instantiations of learn_step_kernel keep the parent's instruction stream and register counts (one "
             "hidden-argument load sits 8 bytes further on: LearnCall grew by the column pointer).",
             f"(c) / (b) = {med_c / med_b:.3f}: {(med_c - med_b) * 1e3 / (2 * N):.4f} ns per learner-step for the five "
             "8-B column loads, the two or three 8-B stores, one or two 128-bit multiplies and the data-dependent branch."]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
