"""``VecQLearning`` — one tabular Q-learning / QRM learner per (env, agent), updated inside the step launch.

The batched equivalent of attaching the reference's ``QLearning`` (learning_algorithms/qlearning.py:6-110) to every
agent and calling ``update_policy`` after every step as the runners do (frozen_lake_main.py:345-376,
office_main.py:1709-1749): N replicas of the runner's experiment in one process, each learner's table bit-comparable
with the reference's ``q_table`` (include/rmx.h, "tabular Q-learning / QRM learners").  On a ``VecRMEnv`` the tables
are torch tensors on the engine's GPU and a learn step is one kernel launch (csrc/rmx_learn.hip); on a ``HostRMEnv``
they are numpy arrays and the host path runs the same arithmetic (csrc/rmx_learn.h).

The learners follow the env's dynamics (``RMX_LEARN_DYN_ENV``): on an env built from a slip (``stochastic``) or
random-start scenario a learn step reseeds the env's generator at every auto-reset, draws the random starts, chooses
the actions from the fresh start's rows, draws the slips and updates with the intended action and the state actually
reached, in the runner's order; the env's generator and the learners' own never mix.  Whole reference training runs
on such worlds are reproduced bit for bit, the env's generator and episode count included (tests/golden/slearn_*.npz).

Epsilon is the reference learner's own: with ``epsilon_start`` every learner has its entry in the ``[A, N]`` column
``epsilon``, decayed as ``learn_done_episode`` decays it (``max(epsilon_end, epsilon * epsilon_decay)``) whenever a
learn step auto-resets the learner's env, which is what both worlds' ``reset()`` do to every ``QLearning`` learner
(include/rmx.h, "per-learner epsilon schedules"; tests/golden/eps_*.npz).  Without it a step takes one scalar epsilon.

``VecQLambda`` is the same for the reference's ``QLearningLambda`` (Watkins Q(lambda), replacing traces): the learn step
then sweeps each learner's list of live traces instead of the reference's dense ``e_table`` (tests/golden/lambda_*.npz).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from .tables import FROZEN_LAKE


class VecQLearning:
    """``q`` and ``visits``: ``[A, N, S_max, 4]`` float64, ``q[a, e]`` the ``q_table`` of agent a's learner in env e
    (rows past ``W*H*enc_nq[a]`` unused).  ``learning_rate=None`` is the reference's ``1 / visits`` rate.
    ``trunc_is_terminal=None`` follows the env kind: the FrozenLake runner passes ``done or truncated`` to the update,
    the OfficeWorld runner ``done``.  ``policy_seeds`` (an int, or an ``[A, N]`` array of learner seeds) gives every
    learner the reference's own ``np.random.default_rng(seed)`` for ``act_step(reference_stream=True)``: ``rng`` is
    then the generator column ``[5, A, N]`` (include/rmx.h; an int64 tensor holding the uint64 words on a GPU env, a
    uint64 array on a host env).  ``epsilon_start`` gives every learner the reference's epsilon schedule: ``epsilon``
    is then an ``[A, N]`` float64 tensor (array on a host env) filled with it and bound (rmx_learn_eps_bind),
    ``epsilon_end`` defaults to ``epsilon_start`` and ``epsilon_decay`` to 1.0; ``act_step`` and ``run`` then take no
    epsilon of their own.  The column may be overwritten per learner at any time (an epsilon sweep over the envs)."""

    def __init__(self, env, gamma, learning_rate=None, qtable_init=1.0, use_qrm=False, use_rsh=False,
                 trunc_is_terminal=None, policy_seeds=None, epsilon_start=None, epsilon_end=None, epsilon_decay=None):
        # argument checks before the tables are allocated (several GB on a GPU env)
        if learning_rate is not None and float(learning_rate) == 0.0:
            raise ValueError("learning_rate must be > 0, or None for 1 / visits")
        if use_rsh and not use_qrm:
            raise ValueError("use_rsh without use_qrm is not supported (rmx_learn_bind refuses it: the reference's "
                             "non-QRM shaping reads a label-keyed dict by index)")
        if epsilon_start is None and (epsilon_end is not None or epsilon_decay is not None):
            raise ValueError("epsilon_end / epsilon_decay need epsilon_start")
        self.env, self.lib = env, env.lib
        self.host = getattr(env, "device", None) == "cpu"
        tab = env.tables
        if trunc_is_terminal is None:
            trunc_is_terminal = tab.kind == FROZEN_LAKE
        s_max = C.c_int64()
        _capi.check(self.lib.rmx_learn_states(env._h, C.byref(s_max)), "rmx_learn_states")
        self.S_max = int(s_max.value)
        self.n_states = [tab.width * tab.height * int(n) for n in tab.enc_nq]
        shape = (env.A, env.N, self.S_max, 4)
        if self.host:
            self.q = np.full(shape, float(qtable_init), np.float64)
            self.visits = np.zeros(shape, np.float64)
            ptr = lambda x: x.ctypes.data  # noqa: E731
        else:
            t = env.torch
            self.q = t.full(shape, float(qtable_init), dtype=t.float64, device=env.device)
            self.visits = t.zeros(shape, dtype=t.float64, device=env.device)
            ptr = lambda x: x.data_ptr()  # noqa: E731
        self._phi = None
        if use_rsh and tab.phi is not None:
            self._phi = np.ascontiguousarray(tab.phi, np.float64)
        cfg = _capi.RmxLearnConfig()
        cfg.gamma = float(gamma)
        cfg.learning_rate = 0.0 if learning_rate is None else float(learning_rate)
        cfg.use_qrm, cfg.use_rsh, cfg.trunc_is_terminal = int(bool(use_qrm)), int(bool(use_rsh)), int(bool(trunc_is_terminal))
        cfg.phi = None if self._phi is None else self._phi.ctypes.data
        cfg.dynamics = _capi.LEARN_DYN_ENV  # slip and random starts as the env has them (deterministic: no difference)
        _capi.check(self.lib.rmx_learn_bind(env._h, C.byref(cfg), ptr(self.q), ptr(self.visits)), "rmx_learn_bind")
        self.gamma, self.learning_rate = float(gamma), learning_rate
        self.use_qrm, self.use_rsh, self.trunc_is_terminal = bool(use_qrm), bool(use_rsh), bool(trunc_is_terminal)
        self.rng = None
        if policy_seeds is not None:
            seeds = np.asarray(policy_seeds)
            if seeds.dtype.kind not in "iu" or (seeds.dtype.kind == "i" and (seeds < 0).any()):
                raise ValueError("policy_seeds must be non-negative integers")
            seeds = np.ascontiguousarray(np.broadcast_to(seeds.astype(np.uint64), (env.A, env.N))) \
                if seeds.ndim == 0 else np.ascontiguousarray(seeds, np.uint64)
            if seeds.shape != (env.A, env.N):
                raise ValueError(f"policy_seeds must be an int or [A={env.A}, N={env.N}]")
            if self.host:
                self.rng = np.zeros((5, env.A, env.N), np.uint64)
            else:
                self.rng = env.torch.zeros((5, env.A, env.N), dtype=env.torch.int64, device=env.device)
            _capi.check(self.lib.rmx_learn_rng_bind(env._h, ptr(self.rng)), "rmx_learn_rng_bind")
            _capi.check(self.lib.rmx_learn_rng_seed(env._h, seeds.ctypes.data, self._stream()), "rmx_learn_rng_seed")
        self.epsilon = self.epsilon_end = self.epsilon_decay = None
        if epsilon_start is not None:
            if self.host:
                col = np.full((env.A, env.N), float(epsilon_start), np.float64)
            else:
                col = env.torch.full((env.A, env.N), float(epsilon_start), dtype=env.torch.float64, device=env.device)
            self.bind_epsilon(col, float(epsilon_start) if epsilon_end is None else epsilon_end,
                              1.0 if epsilon_decay is None else epsilon_decay)

    def _stream(self):
        return None if self.host else self.env._stream()

    def bind_epsilon(self, col, end, decay):
        """rmx_learn_eps_bind with the caller's own column: a contiguous float64 ``[A, N]`` array (host env) or tensor
        on the engine's device, holding every learner's current epsilon.  ``end`` / ``decay``: the reference's
        ``epsilon_end`` / ``epsilon_decay``.  ``act_step`` / ``run`` then take ``epsilon=None``."""
        env = self.env
        if self.host:
            ok = isinstance(col, np.ndarray) and col.dtype == np.float64 and col.flags.c_contiguous and \
                col.size == env.A * env.N
            p = col.ctypes.data if ok else None
        else:
            t = env.torch
            ok = t.is_tensor(col) and col.dtype is t.float64 and col.get_device() == env.device.index and \
                col.is_contiguous() and col.numel() == env.A * env.N
            p = col.data_ptr() if ok else None
        if not ok:
            raise ValueError(f"the epsilon column must be a contiguous float64 [A={env.A}, N={env.N}] "
                             + ("array" if self.host else "tensor on the engine's device"))
        _capi.check(self.lib.rmx_learn_eps_bind(env._h, p, float(end), float(decay)), "rmx_learn_eps_bind")
        self.epsilon, self.epsilon_end, self.epsilon_decay = col, float(end), float(decay)

    def unbind_epsilon(self):
        """Back to one scalar ``epsilon`` per ``act_step`` / ``run`` call."""
        _capi.check(self.lib.rmx_learn_eps_bind(self.env._h, None, 0.0, 0.0), "rmx_learn_eps_bind")
        self.epsilon = self.epsilon_end = self.epsilon_decay = None

    def learn_done_episode(self, mask=None):
        """The reference's ``learn_done_episode`` for every learner of the masked envs ([N] bool / uint8; None: every
        env): ``epsilon = max(epsilon_end, epsilon * epsilon_decay)``, in stream order (rmx_learn_eps_decay).  The
        learn steps do this themselves at their auto-resets; this serves the resets a loop makes before its first step
        (``env.reset`` leaves the column alone)."""
        _capi.check(self.lib.rmx_learn_eps_decay(self.env._h, self._mask_ptr(mask), self._stream()),
                    "rmx_learn_eps_decay")

    def _mask_ptr(self, mask):
        """An [N] env mask as the pointer the ABI takes (None: NULL); the array stays alive in ``self._mask``."""
        env = self.env
        if mask is None:
            return None
        if self.host:
            m = np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
            p = m.ctypes.data
        else:
            m = env.torch.as_tensor(mask).to(device=env.device, dtype=env.torch.uint8).contiguous()
            p = m.data_ptr()
        if (m.size if self.host else m.numel()) != env.N:
            raise ValueError(f"mask must be [N={env.N}]")
        self._mask = m  # (a device mask is read in stream order, as env.reset's)
        return p

    def _epsilon_arg(self, epsilon):
        """The scalar the ABI validates: the caller's, or with a schedule bound (where it must be None) 0."""
        if self.epsilon is not None:
            if epsilon is not None:
                raise ValueError("an epsilon schedule is bound (epsilon_start / bind_epsilon): epsilon must be None")
            return 0.0
        if epsilon is None:
            raise ValueError("epsilon is required (no epsilon schedule is bound)")
        return float(epsilon)

    def step(self, actions, autoreset=True):
        """One wrapper step with the caller's actions ([A, N] int32, 0..3) and every learner's update."""
        env = self.env
        if self.host:
            a = env._acts(actions)
            p = a.ctypes.data
        else:
            t = env.torch
            a = actions
            if a.dtype is not t.int32 or a.get_device() != env.device.index or not a.is_contiguous():
                a = a.to(device=env.device, dtype=t.int32).contiguous()
            if a.numel() != env.A * env.N:
                raise ValueError(f"actions must be [A={env.A}, N={env.N}]")
            p = a.data_ptr()
        _capi.check(self.lib.rmx_learn_step(env._h, p, 1 if autoreset else 0, self._stream()), "rmx_learn_step")

    def act_step(self, epsilon=None, seed=None, t_global=None, best=False, learn=True, autoreset=True, actions_out=None,
                 reference_stream=False):
        """One step with the engine's policy (epsilon-greedy over each learner's own row with hash-chosen ties;
        ``best``: np.argmax), and with ``learn`` the update.  ``actions_out``: an [A, N] int32 array / tensor that
        receives the chosen actions.  ``reference_stream``: the reference's ``choose_action`` on each learner's own
        numpy generator instead (``policy_seeds``); ``seed`` and ``t_global`` are then unused and may be ``None``.
        ``epsilon``: the scalar every learner explores under; ``None`` (and only ``None``) with an epsilon schedule
        bound, where each learner has its own and the step decays it at its env's auto-reset."""
        env = self.env
        epsilon = self._epsilon_arg(epsilon)
        if reference_stream:
            if self.rng is None:
                raise RuntimeError("act_step(reference_stream=True) needs policy_seeds at construction")
            seed = t_global = 0
        elif seed is None or t_global is None:
            raise ValueError("the engine's policy needs seed and t_global")
        p = None
        if actions_out is not None:
            if self.host:
                p = env._out(actions_out, np.int32, env.A * env.N, "actions_out").ctypes.data
            else:
                t = env.torch
                if actions_out.dtype is not t.int32 or actions_out.get_device() != env.device.index or \
                        not actions_out.is_contiguous() or actions_out.numel() < env.A * env.N:
                    raise ValueError("actions_out must be a contiguous int32 [A, N] tensor on the engine's device")
                p = actions_out.data_ptr()
        flags = (_capi.LEARN_UPDATE if learn else 0) | (_capi.LEARN_BEST if best else 0) | \
            (_capi.LEARN_NUMPY if reference_stream else 0)
        _capi.check(self.lib.rmx_learn_step_policy(env._h, float(epsilon), flags, int(seed) & (2**64 - 1),
                                                   int(t_global), 1 if autoreset else 0, p, self._stream()),
                    "rmx_learn_step_policy")
        return actions_out

    def run(self, T, epsilon=None, seed=None, t_global=None, best=False, learn=True, reference_stream=False,
            actions_out=None):
        """``T`` consecutive auto-resetting ``act_step``s (global steps ``t_global .. t_global + T - 1``) in one
        launch on a GPU env (rmx_learn_run; csrc/rmx_learn_run.hip): the tables, every column, the generators and the
        trace lists end as the T single steps leave them, bit for bit, and the return sum of the episode statistics
        agrees to rounding (it is summed in another order).  ``actions_out``: a contiguous int32 ``[T, A, N]`` tensor
        (an array on a host env) that receives every step's actions.  A ``T`` above ``RMX_LEARN_RUN_MAX`` is split
        into consecutive calls.  A run pays one launch and one Python call for T steps and touches the state and
        output columns once: at config 2 with QRM a step inside run(1000) takes 0.63 of a step called on its own at
        64 envs, 0.70 at 4,096 and 0.73 at 65,536 (profiles/learn_run.md; worlds of five or more agents have not been
        timed).  ``epsilon`` as in ``act_step``: with a schedule bound every env anneals at its own resets inside the
        launch."""
        env = self.env
        epsilon = self._epsilon_arg(epsilon)
        T = int(T)
        if T < 1:
            raise ValueError("T must be >= 1")
        if reference_stream:
            if self.rng is None:
                raise RuntimeError("run(reference_stream=True) needs policy_seeds at construction")
            seed = t_global = 0
        elif seed is None or t_global is None:
            raise ValueError("the engine's policy needs seed and t_global")
        p, AN = None, env.A * env.N
        if actions_out is not None:
            if self.host:
                p = env._out(actions_out, np.int32, T * AN, "actions_out").ctypes.data
            else:
                t = env.torch
                if actions_out.dtype is not t.int32 or actions_out.get_device() != env.device.index or \
                        not actions_out.is_contiguous() or actions_out.numel() < T * AN:
                    raise ValueError("actions_out must be a contiguous int32 [T, A, N] tensor on the engine's device")
                p = actions_out.data_ptr()
        flags = (_capi.LEARN_UPDATE if learn else 0) | (_capi.LEARN_BEST if best else 0) | \
            (_capi.LEARN_NUMPY if reference_stream else 0)
        done = 0
        while done < T:  # the cap of one launch is invisible from here
            n = min(T - done, _capi.LEARN_RUN_MAX)
            _capi.check(self.lib.rmx_learn_run(env._h, n, float(epsilon), flags, int(seed) & (2**64 - 1),
                                               int(t_global) + done, None if p is None else p + 4 * done * AN,
                                               self._stream()), "rmx_learn_run")
            done += n
        return actions_out

    def rng_state(self, a, e):
        """Learner (a, e)'s generator as numpy's own ``bit_generator.state`` dict (hand it to a real ``Generator``)."""
        if self.rng is None:
            raise RuntimeError("no generator column (policy_seeds)")
        if self.host:
            w = [int(v) for v in self.rng[:, a, e]]
        else:
            self.env.sync_end()
            w = [int(v) & (2**64 - 1) for v in self.rng[:, a, e].cpu().numpy()]
        return {"bit_generator": "PCG64", "state": {"state": (w[0] << 64) | w[1], "inc": (w[2] << 64) | w[3]},
                "has_uint32": w[4] >> 32, "uinteger": w[4] & 0xFFFFFFFF}

    def set_rng_state(self, a, e, state):
        """Set learner (a, e)'s generator from a ``bit_generator.state`` dict of a PCG64."""
        if self.rng is None:
            raise RuntimeError("no generator column (policy_seeds)")
        if state.get("bit_generator") != "PCG64":
            raise ValueError("the learners' generators are PCG64")
        st, inc = int(state["state"]["state"]), int(state["state"]["inc"])
        has, u = int(state["has_uint32"]), int(state["uinteger"])
        if not (0 <= st < 2**128 and 0 <= inc < 2**128 and has in (0, 1) and 0 <= u < 2**32):
            raise ValueError("not a PCG64 state")
        m = 2**64 - 1
        w = np.array([st >> 64, st & m, inc >> 64, inc & m, (has << 32) | u], np.uint64)
        if self.host:
            self.rng[:, a, e] = w
        else:
            self.env.sync_end()
            self.rng[:, a, e] = self.env.torch.from_numpy(w.view(np.int64)).to(self.env.device)

    def greedy(self):
        """np.argmax of every learner's row at its env's current state: [A, N] (numpy int64 / torch int64)."""
        env, tab = self.env, self.env.tables
        env.sync_end()
        if self.host:
            nq = np.asarray(tab.enc_nq, np.int64)[:, None]
            s = (env.pos_y.astype(np.int64) * tab.width + env.pos_x) * nq + env.rm_q
            rows = np.take_along_axis(self.q, s[:, :, None, None].repeat(4, axis=3), axis=2)[:, :, 0, :]
            return np.argmax(rows, axis=-1)
        t = env.torch
        nq = t.as_tensor(np.asarray(tab.enc_nq, np.int64), device=env.device)[:, None]
        s = (env.pos_y.to(t.int64) * tab.width + env.pos_x) * nq + env.rm_q
        rows = t.gather(self.q, 2, s[:, :, None, None].expand(-1, -1, 1, 4))[:, :, 0, :]
        m = rows.max(dim=-1).values  # the first maximum, as np.argmax (torch.argmax leaves ties open)
        three = t.full_like(s, 3)
        return t.where(rows[..., 0] == m, three - 3,
                       t.where(rows[..., 1] == m, three - 2, t.where(rows[..., 2] == m, three - 1, three)))


class VecQLambda(VecQLearning):
    """One Watkins Q(lambda) learner with replacing traces per (env, agent): the reference's ``QLearningLambda``
    (learning_algorithms/qlearning_lambda.py) as ``AgentRL.update_policy`` drives it, i.e. without ``next_action``:
    the traces always decay and are wiped when an update is terminal or the env resets (include/rmx.h, "Watkins
    Q(lambda) learners").  ``step``, ``act_step``, ``greedy`` and the generator accessors are ``VecQLearning``'s; the
    learn step behind them is the Q(lambda) one, still one launch on a GPU env.

    The reference's dense ``e_table`` is kept as per-learner lists of the live traces: ``trace_idx`` /  ``trace_val``
    ``[A, L, N]`` (slot-major) and ``trace_cnt`` ``[A, N]``; ``traces()`` rebuilds the dense table.  ``trace_cap``
    (default: ``4 * S_max``, which cannot overflow) is L; a trace that finds its list full is dropped and
    ``env.check_errors()`` raises ``RuntimeError``.  Steps taken through the env's own ``step`` / ``step_seq`` /
    ``rollout`` leave the lists alone, their auto-resets included: call ``clear_traces`` when mixing them in.
    The reference's ``reset()`` does not call ``learn_done_episode`` on a ``QLearningLambda`` (it is no ``QLearning``),
    so its runners keep epsilon fixed: leave ``epsilon_start`` unset for them.  The class has a ``learn_done_episode``
    of its own; a loop that calls it at every reset is what ``epsilon_start`` / ``epsilon_end`` / ``epsilon_decay``
    reproduce here.  Not reproduced: an explicit ``next_action``, softmax action selection."""

    def __init__(self, env, gamma, lambd, learning_rate=None, qtable_init=0.0, trunc_is_terminal=None,
                 policy_seeds=None, trace_cap=None, epsilon_start=None, epsilon_end=None, epsilon_decay=None):
        super().__init__(env, gamma, learning_rate, qtable_init=qtable_init, use_qrm=False, use_rsh=False,
                         trunc_is_terminal=trunc_is_terminal, policy_seeds=policy_seeds, epsilon_start=epsilon_start,
                         epsilon_end=epsilon_end, epsilon_decay=epsilon_decay)
        full = C.c_int32()
        _capi.check(self.lib.rmx_learn_lambda_slots(env._h, C.byref(full)), "rmx_learn_lambda_slots")
        self.trace_full = int(full.value)
        self.trace_cap = self.trace_full if trace_cap is None else int(trace_cap)
        self.lambd = float(lambd)
        cap = max(self.trace_cap, 1)  # (a refused cap is refused by the bind below, not by the allocation)
        if self.host:
            self.trace_idx = np.zeros((env.A, cap, env.N), np.int32)
            self.trace_val = np.zeros((env.A, cap, env.N), np.float64)
            self.trace_cnt = np.zeros((env.A, env.N), np.int32)
        else:
            t = env.torch
            self.trace_idx = t.zeros((env.A, cap, env.N), dtype=t.int32, device=env.device)
            self.trace_val = t.zeros((env.A, cap, env.N), dtype=t.float64, device=env.device)
            self.trace_cnt = t.zeros((env.A, env.N), dtype=t.int32, device=env.device)
        self.bind_traces(self.trace_idx, self.trace_val, self.trace_cnt, self.trace_cap)

    def _ptr(self, x):
        return x.ctypes.data if self.host else x.data_ptr()

    def bind_traces(self, idx, val, cnt, cap, lambd=None):
        """rmx_learn_lambda_bind with the caller's own arrays (numpy on a host env, tensors or views on a GPU env)."""
        _capi.check(self.lib.rmx_learn_lambda_bind(self.env._h, self.lambd if lambd is None else float(lambd),
                                                   int(cap), self._ptr(idx), self._ptr(val), self._ptr(cnt)),
                    "rmx_learn_lambda_bind")
        self.trace_idx, self.trace_val, self.trace_cnt, self.trace_cap = idx, val, cnt, int(cap)

    def unbind_traces(self):
        """Back to plain Q-learning steps on the same tables (``bind_traces`` binds the lists again)."""
        _capi.check(self.lib.rmx_learn_lambda_bind(self.env._h, 0.0, 0, None, None, None), "rmx_learn_lambda_bind")

    def trace_counts(self):
        """The length of every learner's list: [A, N] int32 (numpy)."""
        if self.host:
            return self.trace_cnt.copy()
        self.env.sync_end()
        return self.trace_cnt.cpu().numpy()

    def traces(self):
        """The dense ``e_table`` of every learner rebuilt from its list: [A, N, S_max, 4] float64 (numpy)."""
        cnt = self.trace_counts()
        idx = self.trace_idx if self.host else self.trace_idx.cpu().numpy()
        val = self.trace_val if self.host else self.trace_val.cpu().numpy()
        A, N = cnt.shape
        e = np.zeros((A, N, self.S_max * 4), np.float64)
        for j in range(int(cnt.max(initial=0))):
            a, n = np.nonzero(cnt > j)
            e[a, n, idx[a, j, n]] = val[a, j, n]
        return e.reshape(A, N, self.S_max, 4)

    def clear_traces(self, mask=None):
        """Empty the lists of the masked envs ([N] bool / uint8; None: every env)."""
        _capi.check(self.lib.rmx_learn_traces_clear(self.env._h, self._mask_ptr(mask), self._stream()),
                    "rmx_learn_traces_clear")


class VecRMax(VecQLearning):
    """One R-max learner per (env, agent): the reference's ``RMax`` (learning_algorithms/rmax.py) as
    ``AgentRL.update_policy`` drives it, which is what the OfficeWorld runner's ``--algorithm RMAX`` / ``RMAXRM``
    (``use_qrm``) build (include/rmx.h, "R-max learners").  Every learner keeps its own model: ``counts`` (the bound
    ``visits`` table, the reference's ``s_a_counts``), ``rsum`` (``rewards``) ``[A, N, S_max, 4]`` float64, and the
    non-zero entries of the reference's dense ``transitions`` as lists ``succ_idx`` / ``succ_cnt``
    ``[A, N, S_max, 4, cap]`` int32 in first-seen order; ``q`` starts at ``max_reward / (1 - gamma)``.  The observation
    that brings a pair to ``s_a_threshold`` solves the learner's MDP by value iteration at once (``vi_delta``,
    ``vi_delta_rel``, at most ``max_iter`` sweeps).  On a GPU env a learn step is the step kernel plus a solve kernel
    that walks the learners with a solve pending (csrc/rmx_learn_rmax.hip), and ``run(T)`` is one launch in which a
    wave per env steps and solves in place (csrc/rmx_learn_rmax_run.hip); a host env runs the same functions in order.

    ``step``, ``act_step``, ``greedy`` and the generator accessors are ``VecQLearning``'s.  There is no
    epsilon: ``act_step`` / ``run`` take none (passing one raises); a flat row draws one of the four actions, any
    other row takes its first maximum.  ``succ_cap`` (default: ``rmx_learn_rmax_slots``, which cannot overflow) is
    cap; a successor that finds its list full is dropped from the list (still counted) and ``env.check_errors()``
    raises ``RuntimeError``.  No reset touches the model.  Not reproduced: ``noupdate_cnt`` and the early-stop return
    value of ``update``, ``QRMax_v2``, ``UCBVI``, ``OPSRL``."""

    def __init__(self, env, gamma, s_a_threshold=100, max_reward=1.0, vi_delta=1e-4, vi_delta_rel=False, use_qrm=False,
                 trunc_is_terminal=None, policy_seeds=None, succ_cap=None, max_iter=10000):
        if not float(gamma) < 1.0:
            raise ValueError("R-max needs gamma < 1")
        super().__init__(env, gamma, learning_rate=1.0, qtable_init=float(max_reward) / (1.0 - float(gamma)),
                         use_qrm=use_qrm, use_rsh=False, trunc_is_terminal=trunc_is_terminal, policy_seeds=policy_seeds)
        self.learning_rate = None  # (R-max has none; the Q-learning steps after unbind() run at rate 1)
        full = C.c_int32()
        _capi.check(self.lib.rmx_learn_rmax_slots(env._h, C.byref(full)), "rmx_learn_rmax_slots")
        self.succ_full = int(full.value)
        self.succ_cap = self.succ_full if succ_cap is None else int(succ_cap)
        self.s_a_threshold, self.max_reward = int(s_a_threshold), float(max_reward)
        self.vi_delta, self.vi_delta_rel, self.max_iter = float(vi_delta), bool(vi_delta_rel), int(max_iter)
        self.counts = self.visits
        cap = max(self.succ_cap, 1)  # (a refused cap is refused by the bind below, not by the allocation)
        shape = (env.A, env.N, self.S_max, 4)
        if self.host:
            self.rsum = np.zeros(shape, np.float64)
            self.succ_idx = np.zeros(shape + (cap,), np.int32)
            self.succ_cnt = np.zeros(shape + (cap,), np.int32)
        else:
            t = env.torch
            self.rsum = t.zeros(shape, dtype=t.float64, device=env.device)
            self.succ_idx = t.zeros(shape + (cap,), dtype=t.int32, device=env.device)
            self.succ_cnt = t.zeros(shape + (cap,), dtype=t.int32, device=env.device)
        self.bind_model(self.rsum, self.succ_idx, self.succ_cnt, self.succ_cap)

    def _ptr(self, x):
        return x.ctypes.data if self.host else x.data_ptr()

    def bind_model(self, rsum, succ_idx, succ_cnt, cap):
        """rmx_learn_rmax_bind with the caller's own arrays (numpy on a host env, tensors or views on a GPU env)."""
        _capi.check(self.lib.rmx_learn_rmax_bind(self.env._h, self.s_a_threshold, self.vi_delta,
                                                 int(self.vi_delta_rel), self.max_iter, int(cap), self._ptr(rsum),
                                                 self._ptr(succ_idx), self._ptr(succ_cnt)), "rmx_learn_rmax_bind")
        self.rsum, self.succ_idx, self.succ_cnt, self.succ_cap = rsum, succ_idx, succ_cnt, int(cap)

    def unbind(self):
        """Back to plain Q-learning steps on the same tables (``bind_model`` binds the model again)."""
        _capi.check(self.lib.rmx_learn_rmax_bind(self.env._h, 0, 0.0, 0, 0, 0, None, None, None), "rmx_learn_rmax_bind")

    def _epsilon_arg(self, epsilon):
        if epsilon is not None:
            raise ValueError("R-max has no epsilon: epsilon must be None")
        return 0.0

    def run(self, T, epsilon=None, seed=None, t_global=None, best=False, learn=True, reference_stream=False,
            actions_out=None, fused=True):
        """``T`` consecutive auto-resetting ``act_step``s (global steps ``t_global .. t_global + T - 1``), with the
        result contract of ``VecQLearning.run``: the tables, the model, every column, the generators and
        ``solve_info()`` end as the T single steps leave them, bit for bit, and the return sum of the episode
        statistics agrees to rounding.  On a GPU env the T steps are one launch (rmx_learn_model_run;
        csrc/rmx_learn_rmax_run.hip, csrc/rmx_learn_qrmax_run.hip): one wave owns one env, lane 0 steps it and
        applies the model updates, and every solve runs on the wave's 64 lanes at the place the reference has it.  A
        ``T`` above ``RMX_LEARN_MODEL_RUN_MAX`` is split into consecutive calls; a world whose tables and solve
        values do not fit in 64 KiB of LDS together is stepped by the same call as T two-launch steps.
        ``fused=False`` loops ``act_step`` in Python instead, one call and at most two launches per step: the same
        results.  Measured at config 2 with QRM (profiles/learn_model_run.md): the fused run takes 0.46-0.57 of the
        loop's time per step at 64 and 4,096 envs and about half on a fresh model at threshold 1 from 4,096 envs up,
        but at 65,536 envs a step without a solve is 3.0-4.4 times SLOWER fused (a whole wave per env with one lane
        busy): pass ``fused=False`` there once solves have become rare.  Nothing chooses automatically.
        ``actions_out``: a contiguous int32 ``[T, A, N]`` tensor (an array on a host env)."""
        env = self.env
        self._epsilon_arg(epsilon)
        T = int(T)
        if T < 1:
            raise ValueError("T must be >= 1")
        if reference_stream:
            if self.rng is None:
                raise RuntimeError("run(reference_stream=True) needs policy_seeds at construction")
            seed = t_global = 0
        elif seed is None or t_global is None:
            raise ValueError("the engine's policy needs seed and t_global")
        AN = env.A * env.N
        p = flat = None
        if actions_out is not None:
            if self.host:
                flat = env._out(actions_out, np.int32, T * AN, "actions_out").reshape(-1)
                p = flat.ctypes.data
            else:
                t = env.torch
                if actions_out.dtype is not t.int32 or actions_out.get_device() != env.device.index or \
                        not actions_out.is_contiguous() or actions_out.numel() < T * AN:
                    raise ValueError("actions_out must be a contiguous int32 [T, A, N] tensor on the engine's device")
                flat = actions_out.view(-1)
                p = actions_out.data_ptr()
        if not fused:
            for k in range(T):
                self.act_step(None, seed, int(t_global) + k, best=best, learn=learn,
                              actions_out=None if flat is None else flat[k * AN:(k + 1) * AN],
                              reference_stream=reference_stream)
            return actions_out
        flags = (_capi.LEARN_UPDATE if learn else 0) | (_capi.LEARN_BEST if best else 0) | \
            (_capi.LEARN_NUMPY if reference_stream else 0)
        done = 0
        while done < T:  # the cap of one launch is invisible from here
            n = min(T - done, _capi.LEARN_MODEL_RUN_MAX)
            _capi.check(self.lib.rmx_learn_model_run(env._h, n, flags, int(seed) & (2**64 - 1), int(t_global) + done,
                                                     None if p is None else p + 4 * done * AN, self._stream()),
                        "rmx_learn_model_run")
            done += n
        return actions_out

    def _np(self, x):
        if self.host:
            return x
        self.env.sync_end()
        return x.cpu().numpy()

    def known(self):
        """``counts >= s_a_threshold``: [A, N, S_max, 4] bool (numpy), the pairs value iteration writes."""
        return self._np(self.counts) >= self.s_a_threshold

    def transitions(self):
        """The reference's dense ``transitions`` rebuilt from the lists: [A, N, S_max, 4, S_max] float64 (numpy)."""
        idx, cnt = self._np(self.succ_idx), self._np(self.succ_cnt)
        A, N, S, _, cap = cnt.shape
        out = np.zeros((A, N, S, 4, S), np.float64)
        a, e, s, k, j = np.nonzero(cnt)
        out[a, e, s, k, idx[a, e, s, k, j]] = cnt[a, e, s, k, j]
        return out

    def solve_info(self):
        """``(solves, max_sweeps)``: the solves made since the model was bound, and the sweeps of the longest one
        (the converging sweep included).  Synchronises a GPU env."""
        n, m = C.c_int64(), C.c_int64()
        _capi.check(self.lib.rmx_learn_rmax_info(self.env._h, C.byref(n), C.byref(m)), "rmx_learn_rmax_info")
        return int(n.value), int(m.value)


class VecQRMax(VecQLearning):
    """One QR-max learner per (env, agent): the reference's ``QRMax_v2`` (learning_algorithms/qrmax_v2.py) as
    ``AgentRL.update_policy`` drives it, which is what the OfficeWorld runner's ``--algorithm QRMAX`` / ``QRMAXRM``
    (``use_qrm``) build through ``create_qrmax`` (include/rmx.h, "QR-max learners").  QR-max is the R-max variant that
    exploits the Reward Machine: it learns the environment model over grid positions only (``n_tsa``, ``n_rsa``,
    ``sum_rsa`` ``[A, N, P, 4]`` and the successors of each (position, action) as lists ``succ_idx`` / ``succ_cnt``
    ``[A, N, P, 4, cap]`` in first-seen order, ``P = W*H``), the RM model separately (``n_tqs``, ``tq_next``, ``n_rqs``,
    ``sum_rqs`` ``[A, N, S_max]`` at the encoded ``(s', q)``), and takes ``(s, q, a)`` as known (``known_tsqa``) as soon
    as both factors are, so one visit to a cell in any RM state teaches every RM state.  ``visits`` is the reference's
    ``nTSQA``; ``final`` ``[A, N, S_max]`` marks the observed final states; ``q`` starts at ``max_reward * nQ /
    (1 - gamma)`` with ``nQ = enc_nq[a]``, per agent.  An agent-step in which anything became known ends with one
    value iteration (``vi_delta``, ``vi_delta_rel``, at most ``max_iter`` sweeps).  On a GPU env a learn step is the
    step kernel plus a solve kernel that walks the learners with a solve pending (csrc/rmx_learn_qrmax.hip), and
    ``run(T)`` is one launch in which a wave per env steps and solves in place (csrc/rmx_learn_qrmax_run.hip); a host
    env runs the same functions in order.  Every table equals the reference's bit for bit, on slip worlds too.

    ``step``, ``act_step``, ``greedy`` and the generator accessors are ``VecQLearning``'s.  There is no
    epsilon: ``act_step`` / ``run`` take none (passing one raises).  With ``reference_stream`` every call shuffles the
    four actions on the learner's generator first, as the reference does; a flat row then picks from the shuffled list,
    any other row takes its first maximum.  ``succ_cap`` (default: ``rmx_learn_qrmax_slots``, which cannot overflow) is
    cap; a successor that finds its list full is dropped from the list (still counted) and ``env.check_errors()``
    raises ``RuntimeError``.  No reset touches the model.  Not reproduced: ``noupdate_cnt`` and the early-stop return
    value of ``update``; ``reset_VI``; ``tosolve_VI`` / ``learn_done_episode`` (never armed); ``save_environment`` /
    ``load_environment`` (the model arrays are yours: copy them); the bookkeeping no computation reads (``nTSQAS``,
    ``nTSQA_dict``, ``entrySQ_dict``, ``nRSQA``, ``nRSQASQ``, ``sumR``, ``pTSAS``); ``UCBVI``, ``OPSRL``."""

    MODEL = ("known_tsqa", "n_tsa", "n_rsa", "sum_rsa", "succ_idx", "succ_cnt", "n_tqs", "tq_next", "n_rqs", "sum_rqs",
             "final")

    def __init__(self, env, gamma, nsamples_te=100, nsamples_re=100, nsamples_tq=1, nsamples_rq=1, max_reward=1.0,
                 vi_delta=1e-4, vi_delta_rel=False, use_qrm=False, trunc_is_terminal=None, policy_seeds=None,
                 succ_cap=None, max_iter=10000):
        if not float(gamma) < 1.0:
            raise ValueError("QR-max needs gamma < 1")
        super().__init__(env, gamma, learning_rate=1.0, qtable_init=0.0, use_qrm=use_qrm, use_rsh=False,
                         trunc_is_terminal=trunc_is_terminal, policy_seeds=policy_seeds)
        self.learning_rate = None  # (QR-max has none; the Q-learning steps after unbind() run at rate 1)
        tab = env.tables
        for a in range(env.A):  # R_max = max_reward * nQ, per agent
            self.q[a] = float(max_reward) * int(tab.enc_nq[a]) / (1.0 - float(gamma))
        full = C.c_int32()
        _capi.check(self.lib.rmx_learn_qrmax_slots(env._h, C.byref(full)), "rmx_learn_qrmax_slots")
        self.succ_full = int(full.value)
        self.succ_cap = self.succ_full if succ_cap is None else int(succ_cap)
        self.nsamples_te, self.nsamples_re = int(nsamples_te), int(nsamples_re)
        self.nsamples_tq, self.nsamples_rq = int(nsamples_tq), int(nsamples_rq)
        self.max_reward = float(max_reward)
        self.vi_delta, self.vi_delta_rel, self.max_iter = float(vi_delta), bool(vi_delta_rel), int(max_iter)
        self.P = tab.width * tab.height
        self.n_tsqa = self.visits
        cap = max(self.succ_cap, 1)  # (a refused cap is refused by the bind below, not by the allocation)
        sq, sa, s = (env.A, env.N, self.S_max, 4), (env.A, env.N, self.P, 4), (env.A, env.N, self.S_max)
        spec = dict(known_tsqa=(sq, "uint8"), n_tsa=(sa, "int32"), n_rsa=(sa, "int32"), sum_rsa=(sa, "float64"),
                    succ_idx=(sa + (cap,), "int32"), succ_cnt=(sa + (cap,), "int32"), n_tqs=(s, "int32"),
                    tq_next=(s, "int32"), n_rqs=(s, "int32"), sum_rqs=(s, "float64"), final=(s, "uint8"))
        if self.host:
            arrays = {k: np.zeros(shape, dt) for k, (shape, dt) in spec.items()}
        else:
            t = env.torch
            arrays = {k: t.zeros(shape, dtype=getattr(t, dt), device=env.device) for k, (shape, dt) in spec.items()}
        self.bind_model(self.succ_cap, **arrays)

    def _ptr(self, x):
        return x.ctypes.data if self.host else x.data_ptr()

    def bind_model(self, cap, **arrays):
        """rmx_learn_qrmax_bind with the caller's own arrays, by the names of ``MODEL`` (numpy on a host env, tensors
        or views on a GPU env)."""
        if sorted(arrays) != sorted(self.MODEL):
            raise ValueError(f"bind_model takes exactly the arrays {self.MODEL}")
        _capi.check(self.lib.rmx_learn_qrmax_bind(self.env._h, self.nsamples_te, self.nsamples_re, self.nsamples_tq,
                                                  self.nsamples_rq, self.vi_delta, int(self.vi_delta_rel),
                                                  self.max_iter, int(cap), *[self._ptr(arrays[k]) for k in self.MODEL]),
                    "rmx_learn_qrmax_bind")
        for k in self.MODEL:
            setattr(self, k, arrays[k])
        self.succ_cap = int(cap)

    def model(self):
        """The bound model arrays by name (what ``bind_model`` takes)."""
        return {k: getattr(self, k) for k in self.MODEL}

    def unbind(self):
        """Back to plain Q-learning steps on the same tables (``bind_model`` binds the model again)."""
        _capi.check(self.lib.rmx_learn_qrmax_bind(self.env._h, 0, 0, 0, 0, 0.0, 0, 0, 0, *([None] * 11)),
                    "rmx_learn_qrmax_bind")

    def _epsilon_arg(self, epsilon):
        if epsilon is not None:
            raise ValueError("QR-max has no epsilon: epsilon must be None")
        return 0.0

    def run(self, T, epsilon=None, seed=None, t_global=None, best=False, learn=True, reference_stream=False,
            actions_out=None, fused=True):
        """``T`` consecutive auto-resetting ``act_step``s (global steps ``t_global .. t_global + T - 1``) in one
        launch on a GPU env, exactly as ``VecRMax.run``: the tables, the model, every column, the generators and
        ``solve_info()`` end as the T single steps leave them, bit for bit.  ``fused=False`` loops ``act_step`` in
        Python instead: at 65,536 envs with everything known a fused step was measured 2.7 times SLOWER than a looped
        one (level while learning; 0.32-0.64 of the loop's time at 64 and 4,096 envs; profiles/learn_model_run.md), so
        pass ``fused=False`` there once solves have become rare.  ``actions_out``: a contiguous int32 ``[T, A, N]`` tensor (an array on a host env)."""
        return VecRMax.run(self, T, epsilon, seed, t_global, best, learn, reference_stream, actions_out, fused)

    def _np(self, x):
        if self.host:
            return x
        self.env.sync_end()
        return x.cpu().numpy()

    def known(self):
        """The reference's ``known(s, q, a)``: ``knownTSA[s, a] and knownRSA[s, a] and knownTSQA[s, q, a]`` as
        ``[A, N, S_max, 4]`` bool (numpy); with final states excluded, the entries value iteration writes."""
        tab = self.env.tables
        env_known = (self._np(self.n_tsa) >= self.nsamples_te) & (self._np(self.n_rsa) >= self.nsamples_re)
        out = self._np(self.known_tsqa) != 0
        for a in range(self.env.A):
            nq = int(tab.enc_nq[a])
            out[a, :, :self.P * nq] &= np.repeat(env_known[a], nq, axis=1)
            out[a, :, self.P * nq:] = False
        return out

    def env_transitions(self):
        """The reference's dense ``nTSAS`` rebuilt from the lists: [A, N, P, 4, P] float64 (numpy)."""
        idx, cnt = self._np(self.succ_idx), self._np(self.succ_cnt)
        A, N, P, _, cap = cnt.shape
        out = np.zeros((A, N, P, 4, P), np.float64)
        a, e, s, k, j = np.nonzero(cnt)
        out[a, e, s, k, idx[a, e, s, k, j]] = cnt[a, e, s, k, j]
        return out

    def solve_info(self):
        """``(solves, max_sweeps, total_sweeps)``: the solves made since the model was bound, the sweeps of the
        longest one and the sweeps of all of them.  Synchronises a GPU env."""
        n, m, s = C.c_int64(), C.c_int64(), C.c_int64()
        _capi.check(self.lib.rmx_learn_qrmax_info(self.env._h, C.byref(n), C.byref(m), C.byref(s)),
                    "rmx_learn_qrmax_info")
        return int(n.value), int(m.value), int(s.value)
