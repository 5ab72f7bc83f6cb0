"""Shared pieces of tests/test_model_run_cpu.py and tests/test_model_run_gpu.py: R-max and QR-max learners driven by
run(T) (rmx_learn_model_run: on a GPU env one launch, one wave per env) against the same learners driven by T single
act_steps.  Every comparison is bit for bit, floats as bit patterns: both sides run the same functions in the same
order."""
import numpy as np

import learn_common as LC
import policy_common as PC
import qrmax_common as QC
import rmax_common as RC
import slearn_common as SC
from rmx.learn import VecQRMax, VecRMax

KINDS = ("rmax", "qrmax")
COMMON = {"rmax": RC, "qrmax": QC}
HASH_SEED = 5


def make(env_cls, kind, tab, N, threshold, use_qrm=False, numpy_policy=False, seed=21, gamma=0.5, vi_delta=1e-3):
    """A fresh handle, reset, with the kind's learner on it (device_equals_host's parameters)."""
    env = env_cls(tab, N)
    env.reset(seed=seed)
    A = tab.n_agents
    seeds = np.arange(A * N, dtype=np.uint64).reshape(A, N) * 977 + 5 if numpy_policy else None
    if kind == "rmax":
        L = VecRMax(env, gamma, s_a_threshold=threshold, vi_delta=vi_delta, use_qrm=use_qrm, policy_seeds=seeds)
    else:
        L = VecQRMax(env, gamma, nsamples_te=threshold, nsamples_re=threshold, vi_delta=vi_delta, use_qrm=use_qrm,
                     policy_seeds=seeds)
    return env, L


def new_out(L, n, fill=-1):
    """An actions_out [n, A, N] for L's env, filled with `fill`."""
    env = L.env
    if L.host:
        return np.full((n, env.A, env.N), fill, np.int32)
    return env.torch.full((n, env.A, env.N), fill, dtype=env.torch.int32, device=env.device)


def policy_kw(L, start, seed=HASH_SEED):
    """The keywords of a step or run that begins at global step `start`: the learners' own generators where the
    learner has them, else the engine's hashed policy."""
    return dict(reference_stream=True) if L.rng is not None else dict(seed=seed, t_global=start)


def run(L, T, start=0, out=None, seed=HASH_SEED, **kw):
    """One run(T) (the fused entry unless kw says fused=False)."""
    L.run(T, actions_out=out, **policy_kw(L, start, seed), **kw)


def steps(L, T, start=0, out=None, seed=HASH_SEED, **kw):
    """T single act_steps; returns the solves of each step."""
    per_step = []
    for k in range(T):
        before = L.solve_info()[0]
        L.act_step(actions_out=None if out is None else out[k], **policy_kw(L, start + k, seed), **kw)
        per_step.append(L.solve_info()[0] - before)
    return per_step


def same(kind, Lx, Ly, what, outs=None):
    """Everything a run leaves behind: the model and q, every column (the env generator and episode columns where
    the world has them), the learners' generators, the solve statistics, and the actions."""
    COMMON[kind].assert_same_model(Lx, Ly, (what, "model"))
    tab = Lx.env.tables
    cols = SC.env_columns if (tab.stochastic or tab.random_starts) else LC.columns
    LC.assert_same_columns(cols(Lx.env), cols(Ly.env), (what, "columns"))
    if Lx.rng is not None:
        assert np.array_equal(PC.words(Lx.rng), PC.words(Ly.rng)), (what, "generators")
    assert Lx.solve_info() == Ly.solve_info(), (what, Lx.solve_info(), Ly.solve_info())
    if outs is not None:
        x, y = LC.host(outs[0]), LC.host(outs[1])
        assert np.array_equal(x, y) and (x >= 0).all(), (what, "actions")


def run_equals_steps(kind, cls_x, cls_y, tab, N, threshold, T, use_qrm=False, numpy_policy=False, loop_cls=None,
                     seed=HASH_SEED, **kw):
    """A handle of cls_x driven by ONE run(T) against a handle of cls_y driven by T act_steps (and, with loop_cls, a
    third handle driven by run(T, fused=False)).  Returns what the stepwise side went through."""
    ex, Lx = make(cls_x, kind, tab, N, threshold, use_qrm, numpy_policy)
    ey, Ly = make(cls_y, kind, tab, N, threshold, use_qrm, numpy_policy)
    ox, oy = new_out(Lx, T), new_out(Ly, T)
    run(Lx, T, 0, ox, seed, **kw)
    per_step = steps(Ly, T, 0, oy, seed, **kw)
    same(kind, Lx, Ly, "run against steps", (ox, oy))
    COMMON[kind].assert_list_invariant(Lx)
    envs = [ex, ey]
    if loop_cls is not None:
        ez, Lz = make(loop_cls, kind, tab, N, threshold, use_qrm, numpy_policy)
        oz = new_out(Lz, T)
        run(Lz, T, 0, oz, seed, fused=False, **kw)
        same(kind, Lx, Lz, "run against the looped run", (ox, oz))
        envs.append(ez)
    info = Ly.solve_info()
    seen = dict(solves=info[0], sweeps=info[1], per_step=per_step, known=int(Ly.known().sum()),
                rows4=4 * max(Ly.n_states), resets=bool((LC.host(ey.t) < T).any()))
    for e in envs:
        e.check_errors()
        e.close()
    return seen


def lds_bytes(L):
    """What one fused launch needs: the staged table blob, then 16 bytes per state (csrc/rmx_internal.h,
    model_run_lds).  The blob's size is the handle's own (rmx_step_info, generic_blob_bytes)."""
    return int(L.env.step_info["generic_blob_bytes"]) + 16 * L.S_max
