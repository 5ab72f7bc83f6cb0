"""Time the learn step on the parent commit and on this one, and on a slip world on this one, and write the timing
section of profiles/learn_slip.md.

    python scripts/learn_slip_bench.py --parent DIR [--envs 65536] [--steps 200] [--rounds 4] [--trials 2] [--out FILE]

DIR is a built checkout of the parent commit (its multiagent-rl-rm_amd/rmx/librmx.so in place).  BASELINE config 2
(FrozenLake map1, 2 agents), QRM learner, lr 0.1, the caller's actions (hashed, 0..3); the slip world is the same
scenario with stochastic=True.  Each window of `steps` launches is timed by device events after a warm-up window.
Every tree is measured in processes of its own (one library per process), parent and this commit in turn, `rounds`
times, each process with `trials` windows per variant (one variant after the other, the deterministic learn step
first on both sides), so that a drift of the machine and the difference between two processes both show up as the
parent's own spread.
  (a) the deterministic learn step: parent against this commit;
  (b) the learn step on the slip world (this commit only: the parent refuses the bind) beside the yardstick, all of it
      the parent's: its learn step + (its rmx_step on the slip world - its rmx_step on the deterministic world).
Not bench.py: this measures the learner, bench.py the flagship step.  The text of --out before the marker line is kept.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARKER = "<!-- timing: written by scripts/learn_slip_bench.py -->"


def measure(tree, envs, steps, trials, here):
    """In a child process: us per step of every trial, per variant, with the package of `tree`."""
    sys.path.insert(0, os.path.join(tree, "multiagent-rl-rm_amd"))
    import torch

    from rmx import tables as T
    from rmx.engine import VecRMEnv
    from rmx.learn import VecQLearning

    if not torch.cuda.is_available():
        raise SystemExit("learn_slip_bench.py needs the GPU: nothing is measured without one")
    plain = T.compile_scenario(T.baseline_scenario(2))
    slip = T.compile_scenario(dict(T.baseline_scenario(2), stochastic=True))

    def build(tab, learn):
        env = VecRMEnv(tab, envs)
        env.reset(seed=1)
        acts = env.fill_actions(5, 0, steps)  # [steps, A, N], 0..3 (FrozenLake slip has no wait action)
        if learn:
            L = VecQLearning(env, 0.9, 0.1, use_qrm=True)
            return env, lambda k: L.step(acts[k])
        return env, lambda k: env.step(acts[k])

    # one variant after the other, each built, warmed up, timed and freed before the next: the learn step of (a) is
    # the first thing either tree's process does, with the same memory behind it
    variants = [("learn", plain, True)]
    variants += [("learn_slip", slip, True)] if here else [("step", plain, False), ("step_slip", slip, False)]
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {}
    for name, tab, learn in variants:
        env, step = build(tab, learn)
        times[name] = []
        for trial in range(trials + 1):  # trial 0 warms up
            ev0.record()
            for k in range(steps):
                step(k)
            ev1.record()
            ev1.synchronize()
            if trial:
                times[name].append(ev0.elapsed_time(ev1) * 1e3 / steps)
        env.check_errors()
        env.close()
        del env, step
        torch.cuda.empty_cache()
    print("TIMES " + json.dumps({"device": torch.cuda.get_device_name(0), "times": times}))


def child(tree, args, here):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", tree, "--envs", str(args.envs), "--steps", str(args.steps),
           "--trials", str(args.trials)] + (["--here"] if here else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    if r.returncode != 0:
        raise SystemExit(f"measuring {tree} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("TIMES "))[6:])


def fmt(ts):
    return f"{statistics.median(ts):.2f} ({min(ts):.2f} - {max(ts):.2f})"


def seq(ts):
    return ", ".join(f"{x:.2f}" for x in ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--here", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--trials", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_slip.md"))
    args = ap.parse_args()
    if args.child:
        return measure(args.child, args.envs, args.steps, args.trials, args.here)
    if not args.parent or not os.path.exists(os.path.join(args.parent, "multiagent-rl-rm_amd", "rmx", "librmx.so")):
        raise SystemExit("--parent must be a built checkout of the parent commit")
    if args.rounds * args.trials < 7:
        raise SystemExit("at least seven windows per side (rounds * trials)")
    old, new = [], []
    for _ in range(args.rounds):  # alternated pairs of processes
        old.append(child(args.parent, args, False))
        new.append(child(ROOT, args, True))

    def col(runs, name):
        return sum((r["times"][name] for r in runs), [])

    a_old, a_new, b_new = col(old, "learn"), col(new, "learn"), col(new, "learn_slip")
    s_plain, s_slip = col(old, "step"), col(old, "step_slip")
    med = statistics.median
    inside = min(a_old) <= med(a_new) <= max(a_old)
    yard = med(a_old) + med(s_slip) - med(s_plain)
    # the yardstick's own run-to-run spread: the sum of the three parent spreads it is built from
    spread = (max(a_old) - min(a_old)) + (max(s_slip) - min(s_slip)) + (max(s_plain) - min(s_plain))
    N, n = args.envs, args.rounds * args.trials
    lines = [MARKER, "", "## Timing", "",
             f"{new[0]['device']}; BASELINE config 2 tables, {N} envs x 2 agents, QRM learner (lr 0.1, visits counted), the "
             f"caller's actions, windows of {args.steps} launches on one stream, device events; {args.rounds} alternated "
             f"pairs of processes (parent, this commit), each process with a warm-up window and {args.trials} timed windows "
             f"per variant, one variant after the other, the deterministic learn step first: {n} windows per side.  "
             "The slip world is the same scenario with stochastic=True.", "",
             "| variant | us / step: median (min - max) |", "|---|---|",
             f"| (a) learn step, deterministic world, parent commit | {fmt(a_old)} |",
             f"| (a) learn step, deterministic world, this commit | {fmt(a_new)} |",
             f"| rmx_step, deterministic world, parent commit | {fmt(s_plain)} |",
             f"| rmx_step, slip world, parent commit | {fmt(s_slip)} |",
             f"| (b) learn step, slip world, this commit | {fmt(b_new)} |", "",
             f"Windows in order, us / step: learn, parent: {seq(a_old)}; learn, this commit: {seq(a_new)}; rmx_step, "
             f"parent: {seq(s_plain)}; rmx_step on the slip world, parent: {seq(s_slip)}; learn on the slip world, this "
             f"commit: {seq(b_new)}.", "",
             f"(a) The parent's windows span {min(a_old):.2f} - {max(a_old):.2f} us.  This commit's median, "
             f"{med(a_new):.2f} us, lies {'inside' if inside else 'OUTSIDE'} that span (this / parent = "
             f"{med(a_new) / med(a_old):.4f}).", "",
             f"(b) The yardstick, all of it measured on the parent: learn step + (rmx_step on the slip world - rmx_step) = "
             f"{med(a_old):.2f} + ({med(s_slip):.2f} - {med(s_plain):.2f}) = {yard:.2f} us, with a run-to-run spread of "
             f"{spread:.2f} us (the three spans added).  The learn step on the slip world takes {med(b_new):.2f} us: "
             f"{med(b_new) - yard:+.2f} us against the yardstick, "
             f"{'within' if med(b_new) - yard <= spread else 'MORE THAN'} that spread; "
             f"{(med(b_new) - med(a_new)) * 1e3 / N:.4f} ns per env-step more than the deterministic learn step of this "
             "commit."]
    head = ""
    if os.path.exists(args.out):
        with open(args.out) as f:
            head = f.read().split(MARKER)[0]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + "\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
