"""The reference's action choice in plain Python, with no numpy Generator inside: QLearning.choose_action
(learning_algorithms/qlearning.py:112-143, "greedy" selection) on a PCG64 stream restated from numpy's pcg64.h,
_generator.pyx and distributions.c (include/rmx.h, RMX_LEARN_NUMPY).  tests/test_policy_cpu.py compares it with the
installed numpy's own Generator, and the engine with it."""
import numpy as np

M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
MULT = 0x2360ED051FC65DA44385DF649FCCF645


class Pcg:
    """numpy's PCG64 from a ``bit_generator.state`` dict (or a seed, through numpy's own SeedSequence seeding only)."""

    def __init__(self, state):
        if not isinstance(state, dict):
            state = np.random.default_rng(state).bit_generator.state
        self.s, self.i = int(state["state"]["state"]), int(state["state"]["inc"])
        self.has, self.u = int(state["has_uint32"]), int(state["uinteger"])

    def state(self):
        return {"bit_generator": "PCG64", "state": {"state": self.s, "inc": self.i}, "has_uint32": self.has,
                "uinteger": self.u}

    def words(self):
        """The engine's five column words."""
        return [self.s >> 64, self.s & M64, self.i >> 64, self.i & M64, (self.has << 32) | self.u]

    def next64(self):
        self.s = (self.s * MULT + self.i) & M128
        hi, lo = self.s >> 64, self.s & M64
        x, r = hi ^ lo, hi >> 58
        return ((x >> r) | (x << ((64 - r) & 63))) & M64

    def next32(self):
        if self.has:
            self.has = 0
            return self.u
        v = self.next64()
        self.has, self.u = 1, v >> 32
        return v & 0xFFFFFFFF

    def double(self):
        return (self.next64() >> 11) * (1.0 / 9007199254740992.0)

    def below(self, k):
        """Generator.choice of a k-sequence = integers(0, k): Lemire on buffered 32-bit draws."""
        if k == 1:
            return 0
        m = self.next32() * k
        left = m & 0xFFFFFFFF
        if left < k:
            thr = (0xFFFFFFFF - (k - 1)) % k
            while left < thr:
                m = self.next32() * k
                left = m & 0xFFFFFFFF
        return m >> 32


def row_max(row):
    """include/rmx.h: m = row[0], then m = v for every later v > m."""
    m = row[0]
    for v in row[1:]:
        if v > m:
            m = v
    return m


def choose(g, epsilon, row, best=False):
    """One choose_action of a learner whose generator is g over its q_table row (4 floats)."""
    m = row_max(row)
    maxs = [i for i, v in enumerate(row) if v == m]
    if best:
        return maxs[0] if maxs else 3
    if g.double() < epsilon:
        return g.below(4)
    if not maxs:  # a NaN maximum: the reference raises, the engine takes action 3 and draws nothing
        return 3
    return maxs[g.below(len(maxs))]
