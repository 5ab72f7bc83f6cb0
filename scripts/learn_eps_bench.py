"""Time 1,000 learn steps as 1,000 act_step calls and as ONE run(1000), on the parent commit and on this one without
and with an epsilon schedule bound, at 4,096 and 65,536 envs, and write profiles/learn_eps.md.

    python scripts/learn_eps_bench.py --parent DIR [--steps 1000] [--trials 7] [--out FILE]

DIR is a built checkout of the parent commit (its multiagent-rl-rm_amd/rmx/librmx.so in place).  The protocol is
scripts/learn_run_bench.py's: BASELINE config 2 (FrozenLake map1, 2 agents), QRM learner, lr 0.1, with the engine's
policy and with the reference's numpy stream (a seed per learner); each window of `steps` steps is timed by device
events after a warm-up window; every tree is measured in processes of its own (parent, this commit, parent, this
commit), each with half the trials.  Variants: (a) the parent with the scalar epsilon 0.1, (b) this commit with the
scalar epsilon 0.1 and no column bound, (c) this commit with a column that starts at 1.0 in every window and decays by
0.9 per episode down to 0.1.  (b) must lie inside (a)'s own min - max spread; (c) has no threshold.
A second table times the EPS kernels beside their twins without a schedule on the same work: BASELINE config 5's
OfficeWorld with its first two agents (the two-agent OfficeWorld bucket), 4,096 and 65,536 envs, with the scalar
epsilon 0.1 and with a column that holds 0.1 under decay 1.0, which is the scalar path bit for bit; Q-learning with
the engine's policy and with the numpy stream, Q(lambda) with the engine's policy, and Q(lambda) with slip.
Not bench.py: this measures the learner, bench.py the flagship step.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (4096, 65536)
SCHEDULE = (1.0, 0.1, 0.9)


def measure(tree, steps, trials, order=0):
    """In a child process: us per step of every trial (device events), per configuration and variant, with the package
    of `tree`."""
    sys.path.insert(0, os.path.join(tree, "multiagent-rl-rm_amd"))
    import numpy as np
    import torch

    from rmx import tables as T
    from rmx.engine import VecRMEnv
    from rmx.learn import VecQLambda, VecQLearning

    if not torch.cuda.is_available():
        raise SystemExit("learn_eps_bench.py needs the GPU: nothing is measured without one")
    tab = T.compile_scenario(T.baseline_scenario(2))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    has_eps = hasattr(VecQLearning, "bind_epsilon")
    result = {}

    def seeds(n):  # a seed per learner (one seed everywhere would make every env the same run)
        return np.arange(2 * n, dtype=np.uint64).reshape(2, n) + 2020

    for n in SIZES:
        for policy in ("engine", "stream"):
            kw = dict(reference_stream=True) if policy == "stream" else dict(seed=3)
            learners = {"scalar": {}}
            if has_eps:
                learners["column"] = dict(epsilon_start=SCHEDULE[0], epsilon_end=SCHEDULE[1], epsilon_decay=SCHEDULE[2])
            dev = {}
            for lname, sched in learners.items():
                env = VecRMEnv(tab, n)
                L = VecQLearning(env, 0.9, 0.1, use_qrm=True, policy_seeds=seeds(n) if policy == "stream" else None, **sched)
                eps = None if sched else 0.1

                def by_steps(t0, L=L, eps=eps):
                    if policy == "stream":
                        for _ in range(steps):
                            L.act_step(eps, **kw)
                    else:
                        for k in range(steps):
                            L.act_step(eps, t_global=t0 + k, **kw)

                def by_run(t0, L=L, eps=eps):
                    if policy == "stream":
                        L.run(steps, eps, **kw)
                    else:
                        L.run(steps, eps, t_global=t0, **kw)

                t = 0
                for trial in range(trials + 1):  # trial 0 warms every variant up
                    for vname, window in (("step", by_steps), ("run", by_run)):
                        if sched:  # every window anneals from the start of the schedule
                            L.epsilon.fill_(SCHEDULE[0])
                        torch.cuda.synchronize()
                        ev0.record()
                        window(t)
                        ev1.record()
                        ev1.synchronize()
                        t += steps
                        if trial:
                            dev.setdefault(f"{lname}/{vname}", []).append(ev0.elapsed_time(ev1) * 1e3 / steps)
                env.check_errors()
                if sched:
                    c = L.epsilon.cpu().numpy()
                    result.setdefault("column_end", {})[f"{policy}/{n}"] = [float(c.min()), float(c.mean()), float(c.max())]
                env.close()
                del L, env, by_steps, by_run
                torch.cuda.empty_cache()
            result[f"{policy}/{n}"] = dev
    if has_eps:  # the EPS kernels beside their twins on the same work (a constant column is the scalar path)
        ow = T.baseline_scenario(5)
        ow = dict(ow, agents=ow["agents"][:2])
        twins = {}
        for name, scen, lam, policy in (("hash", ow, False, "engine"), ("numpy", ow, False, "stream"),
                                        ("hash, Q(lambda)", ow, True, "engine"),
                                        ("hash, Q(lambda), slip", dict(ow, stochastic=True), True, "engine")):
            otab = T.compile_scenario(scen)
            for n in SIZES:
                kw = dict(reference_stream=True) if policy == "stream" else dict(seed=3)
                dev = {}
                pairs = []
                both = (("scalar", {}), ("column", dict(epsilon_start=0.1, epsilon_end=0.0, epsilon_decay=1.0)))
                for lname, sched in both[::-1] if order else both:  # which handle is built (and timed) first
                    env = VecRMEnv(otab, n)
                    env.reset(seed=5)
                    ps = seeds(n) if policy == "stream" else None
                    L = VecQLambda(env, 0.9, 0.8, 0.1, policy_seeds=ps, **sched) if lam else \
                        VecQLearning(env, 0.9, 0.1, policy_seeds=ps, **sched)
                    pairs.append((lname, env, L, None if sched else 0.1))
                t = 0
                for trial in range(trials + 1):
                    for lname, env, L, eps in pairs:  # the two learners alternate window by window
                        for vname in ("step", "run"):
                            torch.cuda.synchronize()
                            ev0.record()
                            if vname == "run":
                                L.run(steps, eps, **(kw if policy == "stream" else dict(kw, t_global=t)))
                            elif policy == "stream":
                                for _ in range(steps):
                                    L.act_step(eps, **kw)
                            else:
                                for k in range(steps):
                                    L.act_step(eps, t_global=t + k, **kw)
                            ev1.record()
                            ev1.synchronize()
                            if trial:
                                dev.setdefault(f"{lname}/{vname}", []).append(ev0.elapsed_time(ev1) * 1e3 / steps)
                    t += steps
                same = bool(torch.equal(pairs[0][2].q, pairs[1][2].q))
                for _, env, L, _ in pairs:
                    env.check_errors()
                    env.close()
                del pairs, L, env
                torch.cuda.empty_cache()
                dev["same_tables"] = same
                twins[f"{name}/{n}"] = dev
        result["twins"] = twins
    print("TIMES " + json.dumps({"device": torch.cuda.get_device_name(0), "times": result}))


def child(tree, args, trials, order=0):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, "--steps", str(args.steps), "--trials", str(trials),
           "--order", str(order)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
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
    ap.add_argument("--order", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_eps.md"))
    args = ap.parse_args()
    if args.child:
        return measure(args.child, args.steps, args.trials, args.order)
    if not args.parent or not os.path.exists(os.path.join(args.parent, "multiagent-rl-rm_amd", "rmx", "librmx.so")):
        raise SystemExit("--parent must be a built checkout of the parent commit")
    first = (args.trials + 1) // 2
    runs = [child(args.parent, args, first), child(ROOT, args, first)]
    if args.trials > first:
        runs += [child(args.parent, args, args.trials - first), child(ROOT, args, args.trials - first, 1)]

    def series(key, which, variant):
        procs, learner = {"a": (runs[0::2], "scalar"), "b": (runs[1::2], "scalar"), "c": (runs[1::2], "column")}[which]
        return sum((r["times"][key][f"{learner}/{variant}"] for r in procs), [])

    sched = f"{SCHEDULE[0]} -> {SCHEDULE[1]} at {SCHEDULE[2]} per episode"
    lines = ["# Per-learner epsilon schedules: the learn step and the run with and without a column", "",
             f"{runs[1]['device']}; BASELINE config 2 tables, 2 agents, QRM learner (lr 0.1, visits counted); windows of "
             f"{args.steps} steps on one stream, device events, {args.trials} trials per variant after a warm-up window; "
             "four processes in turn (parent, this commit, parent, this commit), each with half the trials and a warm-up "
             "window of its own; the numpy stream with one generator seed per learner.  (a) the parent commit with the "
             "scalar epsilon 0.1, (b) this commit with the scalar epsilon 0.1 and no column bound, (c) this commit with "
             f"a column decaying {sched} (refilled with {SCHEDULE[0]} before every window).  The margin is (a)'s own "
             "min - max trial spread.", "",
             "| call | policy | envs | (a) us / step: median (min - max) | (b) | (c) | (b) / (a) | (b) within (a)'s "
             "spread | (c) / (a) |", "|---|---|---|---|---|---|---|---|---|"]
    raw = []
    for variant, call in (("step", f"{args.steps} act_step calls"), ("run", f"one run({args.steps})")):
        for n in SIZES:
            for p in ("engine", "stream"):
                key = f"{p}/{n}"
                a, b, c = (series(key, w, variant) for w in "abc")
                ma, mb, mc = (statistics.median(x) for x in (a, b, c))
                inside = min(a) <= mb <= max(a)
                name = {"engine": "engine's policy", "stream": "numpy stream"}[p]
                lines.append(f"| {call} | {name} | {n} | {fmt(a)} | {fmt(b)} | {fmt(c)} | {mb / ma:.4f} | "
                             f"{'yes' if inside else 'NO'} | {mc / ma:.3f} |")
                row = (f"{call}, {name}, {n} envs: (a) " + ", ".join(f"{x:.2f}" for x in a) + "; (b) " +
                       ", ".join(f"{x:.2f}" for x in b) + "; (c) " + ", ".join(f"{x:.2f}" for x in c))
                raw.append(row + ".")
    ends = runs[1]["times"].get("column_end", {})
    lines += ["", "The column after the last window (min / mean / max over the learners): " +
              "; ".join(f"{k}: {v[0]:.3f} / {v[1]:.3f} / {v[2]:.3f}" for k, v in ends.items()) + ".",
              "", "Trials in order, us / step:", ""] + [f"- {r}" for r in raw]
    mine = runs[1::2]
    lines += ["", "## The EPS kernels beside their twins on the same work", "",
              "BASELINE config 5's OfficeWorld with its first two agents (the two-agent OfficeWorld bucket), learning rate "
              "0.1; the scalar epsilon 0.1 against a column that holds 0.1 under decay 1.0, which is the scalar path bit "
              "for bit (the q tables of the two handles are compared after the last window); the two handles alternate "
              "window by window inside this commit's two processes.  The first process builds the handle without a "
              "schedule first, the second the one with the column first, so that what belongs to the order of "
              "allocation and what to the kernel can be told apart: the last two columns give the ratio per process.  "
              "us / step, median (min - max).", "",
              "| learner | envs | call | no schedule | column | column / no schedule | same tables | ratio, no schedule "
              "built first | ratio, column built first |", "|---|---|---|---|---|---|---|---|---|"]
    traw = []
    for key in mine[0]["times"]["twins"]:
        name, n = key.rsplit("/", 1)
        for variant, call in (("step", f"{args.steps} act_step calls"), ("run", f"one run({args.steps})")):
            x = sum((r["times"]["twins"][key][f"scalar/{variant}"] for r in mine), [])
            y = sum((r["times"]["twins"][key][f"column/{variant}"] for r in mine), [])
            same = all(r["times"]["twins"][key]["same_tables"] for r in mine)
            per = [statistics.median(r["times"]["twins"][key][f"column/{variant}"]) /
                   statistics.median(r["times"]["twins"][key][f"scalar/{variant}"]) for r in mine]
            lines.append(f"| {name} | {n} | {call} | {fmt(x)} | {fmt(y)} | {statistics.median(y) / statistics.median(x):.4f} | "
                         f"{'yes' if same else 'NO'} | {per[0]:.4f} | {per[-1] if len(per) > 1 else float('nan'):.4f} |")
            traw.append(f"{name}, {n} envs, {call}: no schedule " + ", ".join(f"{v:.2f}" for v in x) + "; column " +
                        ", ".join(f"{v:.2f}" for v in y) + ".")
    lines += ["", "Trials in order, us / step:", ""] + [f"- {r}" for r in traw]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
