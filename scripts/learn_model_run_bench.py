"""Time a step inside run(T) of the R-max and QR-max learners: the fused run (rmx_learn_model_run: one launch, one wave
per env; csrc/rmx_learn_rmax_run.hip, csrc/rmx_learn_qrmax_run.hip) against the looped run (fused=False: one Python
call and at most two launches per step, what run(T) was before), and print the table of profiles/learn_model_run.md.

    python scripts/learn_model_run_bench.py [--envs 64,4096,65536] [--steps 200] [--first 12] [--trials 5] [--out FILE]

BASELINE config 2 (FrozenLake map1, 2 agents) with use_qrm, gamma 0.9, vi_delta 1e-4, the engine's hashed policy.  Both
sides of a cell run in one process on one device, each on a handle of its own, alternating trial by trial after a
warm-up trial; a run is timed by device events on one stream.  Three phases per learner and size:
  * "fresh, thresholds 1": run(`first`) from a fresh model with every threshold 1 (the model and the env are put back
    before every trial): almost every learner solves in every step;
  * "learning, threshold 100": run(`steps`) windows that follow one another from a fresh model with the reference's
    default thresholds (R-max s_a_threshold 100; QR-max nsamples_te = nsamples_re = 100): both sides go through the
    same steps, so a trial's two windows do the same work; few steps cross;
  * "all known": run(`steps`) windows on a model whose every count stands at its threshold: no update, no solve.
Not bench.py: this measures the learners' runs, bench.py the flagship step.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multiagent-rl-rm_amd"))

GAMMA, SEED = 0.9, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="64,4096,65536")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--first", type=int, default=12)
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from rmx import tables as T
    from rmx.engine import VecRMEnv
    from rmx.learn import VecQRMax, VecRMax

    if not torch.cuda.is_available():
        raise SystemExit("learn_model_run_bench.py needs the GPU: nothing is measured without one")
    tab = T.compile_scenario(T.baseline_scenario(2))
    A = tab.n_agents
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def make(kind, N, threshold):
        env = VecRMEnv(tab, N)
        env.reset(seed=1)
        if kind == "R-max":
            return VecRMax(env, GAMMA, s_a_threshold=threshold, use_qrm=True)
        return VecQRMax(env, GAMMA, nsamples_te=threshold, nsamples_re=threshold, use_qrm=True)

    def fresh(L, q0):
        """The model as it was bound, the env at its first state."""
        L.q.copy_(q0)
        L.visits.zero_()
        arrays = (L.rsum, L.succ_idx, L.succ_cnt) if isinstance(L, VecRMax) else tuple(L.model().values())
        for x in arrays:
            x.zero_()
        L.env.reset(seed=1)

    def all_known(L):
        if isinstance(L, VecRMax):
            L.counts.fill_(float(L.s_a_threshold))
        else:
            L.known_tsqa.fill_(1)
            L.n_tsa.fill_(L.nsamples_te)
            L.n_rsa.fill_(L.nsamples_re)
            L.n_tqs.fill_(L.nsamples_tq)
            L.n_rqs.fill_(L.nsamples_rq)

    def timed(L, T_, t0, fused):
        ev0.record()
        L.run(T_, None, SEED, t0, fused=fused)
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e3 / T_

    lines = [f"{torch.cuda.get_device_name(0)}; BASELINE config 2 tables, {A} agents, use_qrm, gamma {GAMMA}, vi_delta "
             f"1e-4, the engine's hashed policy; us per step inside run(T), device events on one stream, median (min - "
             f"max) of {args.trials} alternating trials after a warm-up trial; T = {args.first} for the fresh phase, "
             f"{args.steps} for the other two.", "",
             "| learner | envs | phase | fused run, us / step | looped run, us / step | fused / looped | solves in the "
             "timed runs (either side) |", "|---|---|---|---|---|---|---|"]
    for kind in ("R-max", "QR-max"):
        for N in (int(v) for v in args.envs.split(",")):
            for phase, threshold, T_ in (("fresh, thresholds 1", 1, args.first),
                                         ("learning, threshold 100", 100, args.steps), ("all known", 3, args.steps)):
                pair = {True: make(kind, N, threshold), False: make(kind, N, threshold)}
                q0 = pair[True].q.clone()
                if phase == "all known":
                    for L in pair.values():
                        all_known(L)
                times, solved = {True: [], False: []}, {True: 0, False: 0}
                for trial in range(args.trials + 1):  # trial 0 warms both sides up
                    for fused in (True, False) if trial % 2 else (False, True):
                        L = pair[fused]
                        if threshold == 1:
                            fresh(L, q0)
                        before = L.solve_info()[0]  # (synchronises; outside the events)
                        us = timed(L, T_, 0 if threshold == 1 else trial * T_, fused)
                        if trial:
                            times[fused].append(us)
                            solved[fused] += L.solve_info()[0] - before
                assert solved[True] == solved[False], (kind, N, phase, solved)  # the two sides did the same work
                assert (solved[True] == 0) == (phase == "all known") or phase.startswith("learning"), (phase, solved)
                f, l = (statistics.median(times[k]) for k in (True, False))
                cell = lambda ts: f"{statistics.median(ts):.2f} ({min(ts):.2f} - {max(ts):.2f})"  # noqa: E731
                lines.append(f"| {kind} | {N} | {phase} | {cell(times[True])} | {cell(times[False])} | {f / l:.2f} | "
                             f"{solved[True]} |")
                print(lines[-1], file=sys.stderr, flush=True)  # (progress; the table is printed at the end)
                for L in pair.values():
                    L.env.check_errors()
                    L.env.close()
                del pair, q0, L
                torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
