"""Time the learn step (rmx_learn_step: the step and every learner's update in one launch) beside the parent's way of
feeding a learner (rmx_step with the QRM columns bound), and write profiles/learn_step.md.

    python scripts/learn_bench.py [--envs 65536] [--steps 200] [--trials 7] [--out profiles/learn_step.md]

BASELINE config 2 (FrozenLake map1, 2 agents, 3 QRM counterfactuals each), hashed actions filled beforehand, each
window of `steps` launches timed by device events after a warm-up window; the two variants alternate, trial by trial.
Not bench.py: this measures the learner, bench.py the flagship step.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multiagent-rl-rm_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--trials", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_step.md"))
    args = ap.parse_args()

    import torch

    from rmx import tables as T
    from rmx.engine import VecRMEnv
    from rmx.learn import VecQLearning

    if not torch.cuda.is_available():
        raise SystemExit("learn_bench.py needs the GPU: nothing is measured without one")
    tab = T.compile_scenario(T.baseline_scenario(2))
    N, K, A = args.envs, args.steps, tab.n_agents
    variants = {}
    # the parent's way: the step with the QRM columns bound, a learner would read them afterwards
    feed = VecRMEnv(tab, N, with_qrm=True)
    variants["rmx_step, QRM columns bound"] = (feed, feed.step)
    # the learn step, QRM learner (3 experiences per agent-step), with and without the visit counts' traffic
    qrm_env = VecRMEnv(tab, N)
    qrm = VecQLearning(qrm_env, 0.9, 0.1, use_qrm=True)
    variants["rmx_learn_step, QRM, lr 0.1, visits counted"] = (qrm_env, qrm.step)
    one_env = VecRMEnv(tab, N)
    one = VecQLearning(one_env, 0.9, None, use_qrm=False)
    variants["rmx_learn_step, no QRM, 1/visits"] = (one_env, one.step)
    pol_env = VecRMEnv(tab, N)
    pol = VecQLearning(pol_env, 0.9, 0.1, use_qrm=True)
    t_pol = [0]

    def pol_step(_):
        pol.act_step(0.1, 3, t_pol[0])
        t_pol[0] += 1
    variants["rmx_learn_step_policy, QRM, epsilon 0.1"] = (pol_env, pol_step)

    acts = feed.fill_actions(3, 0, K)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in variants}
    for trial in range(args.trials + 1):  # trial 0 warms every variant up
        for name, (env, step) in variants.items():
            ev0.record()
            for t in range(K):
                step(acts[t])
            ev1.record()
            ev1.synchronize()
            if trial:
                times[name].append(ev0.elapsed_time(ev1) * 1e3 / K)
    for env, _ in variants.values():
        env.check_errors()
    base = statistics.median(times["rmx_step, QRM columns bound"])
    exp = {"rmx_learn_step, QRM, lr 0.1, visits counted": int(tab.n_qrm.sum()),
           "rmx_learn_step, no QRM, 1/visits": A,
           "rmx_learn_step_policy, QRM, epsilon 0.1": int(tab.n_qrm.sum())}
    # algorithmic bytes of one experience: the 32-B next-state row, the entry read and written (8 + 8), the visit
    # count read and written (8 + 8); a done experience reads no row
    per_exp = 32 + 16 + 16
    table_gb = qrm.q.numel() * 8 / 1e9
    lines = ["# The learn step beside the step that feeds a learner", "",
             f"{torch.cuda.get_device_name(0)}; BASELINE config 2 tables, {N} envs x {A} agents, windows of {K} launches "
             f"on one stream with hashed actions, device events, {args.trials} alternating trials after a warm-up "
             f"window.  q and visits: {table_gb:.2f} GB each per learner set ([A][N][{qrm.S_max}][4] float64).", "",
             "| variant | us / step: median (min - max) | ratio to rmx_step | experiences / step | ns / experience "
             "beyond rmx_step | GB/s of learner traffic |", "|---|---|---|---|---|---|"]
    for name, ts in times.items():
        med = statistics.median(ts)
        row = f"| {name} | {med:.2f} ({min(ts):.2f} - {max(ts):.2f}) | {med / base:.2f} |"
        if name in exp:
            n_exp = exp[name] * N
            row += f" {n_exp} | {(med - base) * 1e3 / n_exp:.4f} | {n_exp * per_exp / (med * 1e-6) / 1e9:.0f} |"
        else:
            row += " - | - | - |"
        lines.append(row)
    lines += ["", f"Algorithmic bytes per experience: {per_exp} (32-B next-state row, 8 + 8 B entry, 8 + 8 B visit count; "
              "the policy reads one more 32-B row per agent-step).  The rows are gathered from tables far larger than "
              "the 256 MB Infinity Cache; where the time goes: profiles/learn_step_counters.md and DESIGN.md 4.10."]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
