"""Time the QR-max learn step (csrc/rmx_learn_qrmax.hip: the step kernel plus the solve kernel) beside the R-max learn
step at the same shapes in the same session, and print the tables of profiles/learn_qrmax.md.

    python scripts/learn_qrmax_bench.py [--envs 64,4096,65536] [--steps 200] [--trials 5] [--first 12] [--out FILE]

BASELINE config 2 (FrozenLake map1, 2 agents), with and without use_qrm, gamma 0.9, vi_delta 1e-4, the engine's hashed
policy.  Steady state, per size, windows of `steps` learn steps on one stream timed by device events after a warm-up
window, the variants alternating trial by trial, each on a handle of its own:
  * "learning": thresholds far above anything the windows reach: every step updates the counts, the reward sums and the
    successor lists, nothing becomes known, the solve kernel finds an empty worklist;
  * "all known": every count at its threshold and every known flag set: every update returns at its tests (a converged
    run).
The first steps: a fresh model with thresholds 1, each of the first `first` steps timed on its own (device events
around the step's two launches), with the solve statistics read after each step (that read synchronises and is outside
the events).  Not bench.py: this measures the learner, bench.py the flagship step.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multiagent-rl-rm_amd"))

BIG = 1 << 30


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
    from rmx.learn import VecQRMax, VecRMax

    if not torch.cuda.is_available():
        raise SystemExit("learn_qrmax_bench.py needs the GPU: nothing is measured without one")
    tab = T.compile_scenario(T.baseline_scenario(2))
    A, K = tab.n_agents, args.steps
    P = tab.width * tab.height
    S_max = P * int(max(tab.enc_nq))
    cap = 5
    qr_bytes = S_max * 4 * 17 + P * 4 * (16 + 8 * cap) + S_max * 21
    rm_bytes = S_max * 4 * (24 + 8 * cap)
    free = torch.cuda.mem_get_info()[0]
    lines = [f"{torch.cuda.get_device_name(0)}; BASELINE config 2 tables, {A} agents, P = {P}, S_max = {S_max}, gamma 0.9, "
             f"vi_delta 1e-4, the engine's hashed policy; windows of {K} learn steps on one stream, device events, "
             f"{args.trials} alternating trials after a warm-up window.", "",
             f"Bytes per learner at cap {cap}: QR-max S_max*4*17 (q, visits, known_tsqa) + P*4*(16 + 8*cap) (n_tsa, n_rsa, "
             f"sum_rsa, the two lists) + S_max*21 (n_tqs, tq_next, n_rqs, sum_rqs, final) = {qr_bytes} B; R-max "
             f"S_max*4*(24 + 8*cap) = {rm_bytes} B.  {free / 1e9:.0f} GB free: {int(0.9 * free // (A * qr_bytes))} envs of "
             f"{A} QR-max learners fit in 90 % of it, {int(0.9 * free // (A * rm_bytes))} of R-max learners.", "",
             "| envs | use_qrm | learn step | us / step: median (min - max) | ns / learner-step |", "|---|---|---|---|---|"]
    first_lines = ["| envs | use_qrm | learner | step | us | solves in the step | longest solve so far (sweeps) | sweeps so far |",
                   "|---|---|---|---|---|---|---|---|"]
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for N in (int(v) for v in args.envs.split(",")):
        for use_qrm in (False, True):
            envs = [VecRMEnv(tab, N) for _ in range(4)]
            for e in envs:
                e.reset(seed=1)
            q_learn = VecQRMax(envs[0], 0.9, BIG, BIG, BIG, BIG, use_qrm=use_qrm)
            q_known = VecQRMax(envs[1], 0.9, 3, 3, 1, 1, use_qrm=use_qrm)
            q_known.known_tsqa.fill_(1)
            q_known.n_tsa.fill_(3)
            q_known.n_rsa.fill_(3)
            q_known.n_tqs.fill_(1)
            q_known.n_rqs.fill_(1)
            r_learn = VecRMax(envs[2], 0.9, s_a_threshold=BIG, use_qrm=use_qrm)
            r_known = VecRMax(envs[3], 0.9, s_a_threshold=3, use_qrm=use_qrm)
            r_known.counts.fill_(3.0)
            variants = {"QR-max, learning": q_learn, "QR-max, all known": q_known, "R-max, learning": r_learn,
                        "R-max, all known": r_known}
            times = {k: [] for k in variants}
            t_global = 0
            for trial in range(args.trials + 1):  # trial 0 warms every variant up
                for name, L in variants.items():
                    ev0.record()
                    for k in range(K):
                        L.act_step(None, 3, t_global + k)
                    ev1.record()
                    ev1.synchronize()
                    if trial:
                        times[name].append(ev0.elapsed_time(ev1) * 1e3 / K)
                t_global += K
            assert all(L.solve_info()[0] == 0 for L in variants.values())  # no solve in any steady state
            for name, ts in times.items():
                med = statistics.median(ts)
                lines.append(f"| {N} | {int(use_qrm)} | {name} | {med:.2f} ({min(ts):.2f} - {max(ts):.2f}) | "
                             f"{med * 1e3 / (A * N):.3f} |")
            for e in envs:
                e.check_errors()
                e.close()
            del variants, q_learn, q_known, r_learn, r_known, envs
            torch.cuda.empty_cache()
            # the first steps of a fresh model at thresholds 1
            for name in ("QR-max", "R-max"):
                env = VecRMEnv(tab, N)
                env.reset(seed=1)
                L = VecQRMax(env, 0.9, 1, 1, 1, 1, use_qrm=use_qrm) if name == "QR-max" else \
                    VecRMax(env, 0.9, s_a_threshold=1, use_qrm=use_qrm)
                L.act_step(None, 3, 0, learn=False, autoreset=False)  # (loads the step kernel; the model is untouched)
                env.reset(seed=1)
                done = 0
                for t in range(args.first):
                    ev0.record()
                    L.act_step(None, 3, t)
                    ev1.record()
                    ev1.synchronize()
                    info = L.solve_info()
                    first_lines.append(f"| {N} | {int(use_qrm)} | {name} | {t} | {ev0.elapsed_time(ev1) * 1e3:.1f} | "
                                       f"{info[0] - done} | {info[1]} | {info[2] if len(info) > 2 else '-'} |")
                    done = info[0]
                env.check_errors()
                env.close()
                del L, env
                torch.cuda.empty_cache()
    text = "\n".join(lines + ["", "The first steps of a fresh model, thresholds 1:", ""] + first_lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
