"""Plain Python / numpy restatement of the learn step's update and policy (include/rmx.h, "tabular Q-learning / QRM
learners"), driven by the engine's own step outputs: a twin env (HostRMEnv with the QRM columns and enc_state bound)
is stepped with rmx_step, and the experiences are read from its columns.  Every operation is one Python float
(IEEE float64) operation in the reference's order (qlearning.py:70-79, 82-108).
"""
import numpy as np

from rmx import _capi

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def splitmix64(x):
    z = (x + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def row_max(row):
    """np.max of a row as the engine takes it: m = row[0], then m = v where v > m.  A NaN in row[0] stays (no
    comparison with it is true); a NaN further on is skipped."""
    m = float(row[0])
    for v in row[1:]:
        if float(v) > m:
            m = float(v)
    return m


def policy_action(row, seed, t, n_global, e, A, i, epsilon, best):
    """include/rmx.h, "the engine's policy".  A row with no entry equal to its maximum (a NaN maximum) gives action
    3, greedy and best alike; an explore draw comes before the row is looked at."""
    m = row_max(row)
    maxs = [k for k in range(4) if float(row[k]) == m]
    if best:
        return maxs[0] if maxs else 3
    h0 = splitmix64((seed ^ ((((t * n_global + e) * A + i) * GOLDEN) & M64)) & M64)
    h1 = splitmix64(h0)
    h2 = splitmix64(h1)
    if (h1 >> 11) * 2.0 ** -53 < epsilon:
        return h0 >> 62
    if not maxs:
        return 3
    return maxs[((h2 >> 32) * len(maxs)) >> 32]


class LearnRef:
    def __init__(self, twin, gamma, learning_rate=None, qtable_init=1.0, use_qrm=False, use_rsh=False,
                 trunc_is_terminal=None):
        self.twin, self.tab = twin, twin.tables
        tab = self.tab
        self.A, self.N = twin.A, twin.N
        self.S_max = tab.width * tab.height * int(max(tab.enc_nq))
        self.q = np.full((self.A, self.N, self.S_max, 4), float(qtable_init), np.float64)
        self.visits = np.zeros_like(self.q)
        self.gamma, self.lr = float(gamma), learning_rate
        self.use_qrm, self.use_rsh = use_qrm, use_rsh
        self.tit = (tab.kind == 0) if trunc_is_terminal is None else trunc_is_terminal

    def pre_state(self, autoreset=True):
        """(x, y, q) [A, N] of the state the next step leaves: the start state where the step auto-resets first."""
        tw, tab = self.twin, self.tab
        x, y, q = tw.pos_x.copy(), tw.pos_y.copy(), tw.rm_q.copy()
        if autoreset:
            done = (tw.flags[0] & _capi.F_ENV_DONE) != 0
            for a in range(self.A):
                x[a, done], y[a, done], q[a, done] = tab.start_xy[a, 0], tab.start_xy[a, 1], tab.init_q[a]
        return x, y, q

    def encode(self, x, y, q):
        nq = np.asarray(self.tab.enc_nq, np.int64)[:, None]
        return (y.astype(np.int64) * self.tab.width + x) * nq + q

    def n_rows(self, a):
        """Agent a's own rows, W * H * enc_nq[a]: a state outside them has no row (a column the caller overwrote)."""
        return self.tab.width * self.tab.height * int(self.tab.enc_nq[a])

    def choose(self, epsilon, seed, t_global, best=False, autoreset=True):
        tw = self.twin
        s = self.encode(*self.pre_state(autoreset))
        out = np.zeros((self.A, self.N), np.int32)
        for a in range(self.A):
            for e in range(self.N):
                row = self.q[a, e, s[a, e]] if 0 <= s[a, e] < self.n_rows(a) else (0.0, 0.0, 0.0, 0.0)  # a zero row
                out[a, e] = policy_action(row, seed, t_global, tw.n_envs_global, tw.env_offset + e, self.A, a,
                                          epsilon, best)
        return out

    def update_q(self, a, e, s, k, r, sn, done):
        if not (0 <= s < self.n_rows(a) and 0 <= sn < self.n_rows(a)):
            return  # dropped, never written: the experience's state is outside the agent's rows
        q, v = self.q[a, e], self.visits[a, e]
        cur = float(q[s, k])
        v[s, k] += 1.0
        lr = 1.0 / float(v[s, k]) if self.lr is None else float(self.lr)
        maxq = 0.0 if done else row_max(q[sn])
        x = (1.0 - lr) * cur
        b = self.gamma * maxq
        c = r + b
        d = lr * c
        q[s, k] = x + d

    def step(self, actions, autoreset=True, update=True):
        """Step the twin with rmx_step and apply every learner's update from its columns."""
        tw, tab = self.twin, self.tab
        px, py, pq = self.pre_state(autoreset)
        s_pre = self.encode(px, py, pq)
        tw.step(actions, autoreset)
        if not update:
            return
        acts = np.asarray(actions).reshape(self.A, self.N)
        for a in range(self.A):
            nQ = int(tab.enc_nq[a])
            for e in range(self.N):
                k = int(acts[a, e])
                if not 0 <= k < 4:
                    continue
                renv = float(tw.renv[a, e])
                if self.use_qrm:
                    for j in range(int(tab.n_qrm[a])):
                        s, sn = int(tw.qrm_s[a, j, e]), int(tw.qrm_sn[a, j, e])
                        r = renv + float(tw.qrm_rq[a, j, e])
                        if self.use_rsh:
                            g = self.gamma * float(tab.phi[a, sn % nQ])
                            sh = g - float(tab.phi[a, s % nQ])
                            r = r + sh
                        self.update_q(a, e, s, k, r, sn, bool(tw.qrm_done[a, j, e]))
                else:
                    if not (0 <= px[a, e] < tab.width and 0 <= py[a, e] < tab.height
                            and 0 <= pq[a, e] < tab.n_rm_states):
                        continue  # a pre-step column outside the grid / the RM tables: the engine's result is unspecified
                    cell = int(tw.pos_y[a, e]) * tab.width + int(tw.pos_x[a, e])
                    rq = float(tab.rm_reward[a, pq[a, e], tab.cell_event[a, cell]])
                    m = float(np.float32(tab.reward_modifier)) * rq
                    r = renv + m
                    f = int(tw.flags[a, e])
                    done = bool(f & _capi.F_TERM) or (self.tit and bool(f & _capi.F_TRUNC))
                    self.update_q(a, e, int(s_pre[a, e]), k, r, int(tw.enc_state[a, e]), done)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)
