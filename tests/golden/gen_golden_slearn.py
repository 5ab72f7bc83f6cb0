"""Record whole training runs of the REFERENCE on slip and random-start worlds: its own QLearning chooses every action
from its own numpy generator while its environment draws the slips and the random starts from the env's generator
(needs the reference checkout that gen_golden.py imports; the fixtures, not the reference, travel with the tests).

The loop is gen_golden_policy.py's ``run()`` itself, imported and run over the cases below (the runner's loop:
``select_action`` for every agent, ``rm_env.step``, ``update_policy`` for every agent, ``reset(seed of the episode)``
before the step that follows an episode's end).  Around it, the environments ``gen_golden.make_env`` builds are
watched, never changed: after the steps ``snap_steps`` the env's own state is written down (positions, RM indices, the
timestep, ``env.rng.bit_generator.state`` as the engine's four words, the number of episodes started), and the
coverage counts are read off the reference's own calls (``get_stochastic_action``'s argument and result, ``reset``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_slearn.py [case ...]

Each case is saved as ``slearn_<case>.npz``: everything ``policy_<case>.npz`` holds, and
  env_pos_x, env_pos_y, env_q [3, A, N], env_t [3, N]   the env after each snapshot step
  env_rng [3, 4, N]      the env generator: state high, state low, increment high, increment low
  env_episode [3, N]     episodes started so far, minus one (the engine's episode column: 0 after the first reset)
  coverage [4]           slip draws, draws whose outcome differs from the intended action, resets, distinct start tuples
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_policy as P  # noqa: E402

G = P.G
# case -> (config, n_envs, n_steps, reset seed, eps, qtable_init, learner), as gen_golden_policy.CASES
CASES = {
    "fl2_slip_qrm": ("fl2_slip", 4, 600, 51, 0.1, 1.0, dict(gamma=0.9, lr=0.1, use_qrm=True)),
    "fl2_randstart_slip_visits": ("fl2_randstart_slip", 4, 600, 52, 0.3, 1.0, dict(gamma=0.9, lr=None, use_qrm=False)),
    "fl2_randstart_qrm": ("fl2_randstart", 4, 600, 53, 0.1, 1.0, dict(gamma=0.9, lr=0.1, use_qrm=True)),
    "ow2_allslip_qrm": ("ow2_allslip", 3, 1100, 54, 0.1, 2.0, dict(gamma=0.9, lr=0.1, use_qrm=True)),
    "fl2_delay_plain": ("fl2_delay", 4, 600, 55, 0.1, 1.0, dict(gamma=0.9, lr=0.1, use_qrm=False)),
}
MIN_DIFFERING = 100  # per slip case: draws whose outcome is not the intended action
MIN_STARTS = {"fl2_randstart_slip_visits": 20, "fl2_randstart_qrm": 3}  # distinct start tuples


class Watch:
    """What the environments of one case did, read off their own calls."""

    def __init__(self, A, N, snap_steps):
        self.A, self.N, self.snaps = A, N, snap_steps
        self.pos_x = np.zeros((3, A, N), np.int8)
        self.pos_y = np.zeros((3, A, N), np.int8)
        self.q = np.zeros((3, A, N), np.int16)
        self.t = np.zeros((3, N), np.int32)
        self.rng = np.zeros((3, 4, N), np.uint64)
        self.episode = np.zeros((3, N), np.int32)
        self.draws = self.differing = self.resets = 0
        self.starts = set()
        self.built = 0

    def attach(self, rm_env, agents):
        """The (e + 1)-th environment built is env e's (run() builds one probe first)."""
        e = self.built - 1
        self.built += 1
        if e < 0:
            return
        env = rm_env.env
        seen = {"steps": 0, "resets": 0}
        step, reset, slip = rm_env.step, rm_env.reset, env.get_stochastic_action

        def watched_slip(agent, intended):
            got = slip(agent, intended)
            self.draws += 1
            self.differing += str(got) != str(intended)
            return got

        def watched_reset(*a, **kw):
            out = reset(*a, **kw)
            seen["resets"] += 1
            self.resets += 1
            self.starts.add(tuple((int(ag.state["pos_x"]), int(ag.state["pos_y"])) for ag in agents))
            return out

        def watched_step(actions):
            out = step(actions)
            seen["steps"] += 1
            if seen["steps"] in self.snaps:
                k = self.snaps.index(seen["steps"])
                for i, ag in enumerate(agents):
                    rm = ag.get_reward_machine()
                    self.pos_x[k, i, e], self.pos_y[k, i, e] = out[0][ag.name]["pos_x"], out[0][ag.name]["pos_y"]
                    self.q[k, i, e] = rm.get_state_index(rm.get_current_state())
                self.t[k, e] = env.timestep
                self.rng[k, :, e] = P.words(env.rng.bit_generator.state)[:4]
                self.episode[k, e] = seen["resets"] - 1
            return out

        env.get_stochastic_action, rm_env.reset, rm_env.step = watched_slip, watched_reset, watched_step


def run(case):
    cfg_name, N, T = CASES[case][:3]
    cfg = G.CONFIGS[cfg_name]
    watch = Watch(len(cfg["agents"]), N, [T // 3, (2 * T) // 3, T])
    make_env = G.make_env

    def watched_make_env(c):
        rm_env, agents, det = make_env(c)
        watch.attach(rm_env, agents)
        return rm_env, agents, det

    P.CASES[case] = CASES[case]
    G.make_env = watched_make_env
    try:
        out = P.run(case)  # (asserts MIN_EACH explore and tie counts itself)
    finally:
        G.make_env = make_env
        del P.CASES[case]
    assert watch.built == N + 1 and [int(v) for v in out["snap_steps"]] == watch.snaps
    slip = bool(cfg.get("stochastic", False))
    print(f"{case}: slip draws {watch.draws}, differing {watch.differing}, resets {watch.resets}, "
          f"distinct starts {len(watch.starts)}")
    assert (watch.differing >= MIN_DIFFERING) if slip else watch.draws == 0, case
    assert watch.resets > N, case  # at least one reseed inside the run
    assert len(watch.starts) >= MIN_STARTS.get(case, 1), case
    out.update(env_pos_x=watch.pos_x, env_pos_y=watch.pos_y, env_q=watch.q, env_t=watch.t, env_rng=watch.rng,
               env_episode=watch.episode,
               coverage=np.asarray([watch.draws, watch.differing, watch.resets, len(watch.starts)], np.int64))
    return out


def main(only=None):
    for case in only or CASES:
        out = run(case)
        path = os.path.join(HERE, f"slearn_{case}.npz")
        G._savez(path, **out)
        assert os.path.getsize(path) < 727 * 1024, (case, os.path.getsize(path))
        print("  ", os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
