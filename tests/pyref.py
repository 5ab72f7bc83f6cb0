"""A plain-Python restatement of one deterministic wrapper step, independent of the compiled tables.

TEST INFRASTRUCTURE ONLY.  The CPU oracle (oracle/rmx_oracle.c) and the engine both read the dense uint8 / float32
tables of rmx.tables.compile_tables; a fault in that packing (a signed byte, a truncated index) would be shared by
both.  This stepper works from the unpacked description instead: position sets, wall pairs, the Reward Machines'
``transitions`` dicts keyed by state labels and event positions, and the penalties; Python ints and float64 only.
It restates RMEnvironmentWrapper.step over MultiAgentFrozenLake / MultiAgentOfficeWorld.step and the runners' episode
loop (rm_environment_wrapper.py:43-107, ma_frozen_lake.py:96-154,200-242, ma_office.py:122-202,252-325,
frozen_lake_main.py:336-376, office_main.py:1696-1749) for deterministic dynamics with configured starts: no slip, no
random starts.  tests/test_limits_cpu.py pins it to the reference's recorded trajectories first, then uses it as a
second opinion on the limit worlds the reference cannot record.

A world is a dict:
  kind ("frozen_lake" | "office_world"), width, height, hazards {(x, y)}, walls {((x, y), (x', y'))} (directed),
  starts [(x, y)] per agent, rms [RewardMachineSpec-like: .transitions, .initial_state, .potentials] per agent,
  detectors [{(x, y)}] per agent, hazard_penalty, wall_penalty, hazard_fail, wall_fail, reward_modifier, max_t,
  shaping_gamma (None: no shaping).
"""
F_ACTIVE, F_FAIL, F_TERM, F_TRUNC, F_ENV_TERM, F_RM_TERM, F_ENV_DONE = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40
UP, DOWN, LEFT, RIGHT, WAIT = 0, 1, 2, 3, 4


def state_order(rm):
    """State labels in index order: the initial state first, the rest sorted (reward_machine.py:20-39)."""
    states = {rm.initial_state}
    for (u1, _e), (u2, _r) in rm.transitions.items():
        states.update((u1, u2))
    rest = sorted(states - {rm.initial_state})
    return [rm.initial_state] + rest


def final_state(rm):
    """to_state of the last inserted transition (reward_machine.py:152-163)."""
    last = None
    for v in rm.transitions.values():
        last = v[0]
    return last


class _Agent:
    __slots__ = ("x", "y", "q", "active", "fail", "steps")


class PyRefEnv:
    """n_envs independent envs; step(actions[A][n_envs]) returns the per-step outputs as nested lists [A][n_envs]
    (t and env_done: [n_envs])."""

    def __init__(self, world, n_envs):
        self.w = world
        self.fl = world["kind"] == "frozen_lake"
        self.A = len(world["rms"])
        self.N = int(n_envs)
        self.index = [{s: i for i, s in enumerate(state_order(rm))} for rm in world["rms"]]
        self.final = [final_state(rm) for rm in world["rms"]]
        self.walls = {(tuple(a), tuple(b)) for a, b in world["walls"]}
        self.hazards = {tuple(p) for p in world["hazards"]}
        self.det = [{tuple(p) for p in d} for d in world["detectors"]]
        self.envs = []
        self.t = [0] * self.N
        self.done = [False] * self.N
        for _ in range(self.N):
            self.envs.append([_Agent() for _ in range(self.A)])
        for e in range(self.N):
            self._reset(e)

    def _reset(self, e):
        self.t[e] = 0
        self.done[e] = False
        for a, ag in enumerate(self.envs[e]):
            ag.x, ag.y = (int(v) for v in self.w["starts"][a])
            ag.q = self.w["rms"][a].initial_state
            ag.active, ag.fail, ag.steps = True, False, 0

    def _target(self, x, y, action):
        """The cell `action` leads to, or None where the grid edge (or an OfficeWorld wall) blocks it."""
        up = -1 if self.fl else 1  # FrozenLake: up = y - 1; OfficeWorld: up = y + 1
        dx, dy = {UP: (0, up), DOWN: (0, -up), LEFT: (-1, 0), RIGHT: (1, 0)}[action]
        nx, ny = x + dx, y + dy
        if not (0 <= nx < self.w["width"] and 0 <= ny < self.w["height"]):
            return None
        if ((x, y), (nx, ny)) in self.walls:
            return None
        return nx, ny

    def step(self, actions):
        w, A, N = self.w, self.A, self.N
        out = {k: [[0] * N for _ in range(A)] for k in ("pos_x", "pos_y", "q", "flags", "reward", "renv", "shaping")}
        for e in range(N):
            if self.done[e]:  # the loop rule: a finished episode is reset before the next step
                self._reset(e)
            t1 = self.t[e] + 1
            all_term = all_trunc = True
            for a, ag in enumerate(self.envs[e]):
                ac = int(actions[a][e])
                rm, fin = w["rms"][a], self.final[a]
                renv = 0.0
                if self.fl:
                    if ag.active and ag.q != fin:  # an agent whose RM is final no longer moves
                        tgt = None if ac == WAIT else self._target(ag.x, ag.y, ac)
                        if tgt is not None:
                            ag.x, ag.y = tgt
                        if (ag.x, ag.y) in self.hazards:
                            ag.fail = True
                            renv = float(w["hazard_penalty"])
                        ag.steps += 1
                    trunc = ag.steps > w["max_t"] or t1 > w["max_t"]
                    env_term = trunc or ag.q == fin or ag.fail  # the RM state before this step's RM transition
                else:
                    if ag.active:
                        if ac != WAIT:
                            tgt = self._target(ag.x, ag.y, ac)
                            if tgt is None:  # a wall collision: the penalty, and the agent waits
                                renv = float(w["wall_penalty"])
                                if w["wall_fail"]:
                                    ag.fail = True
                            else:
                                ag.x, ag.y = tgt
                        if (ag.x, ag.y) in self.hazards:
                            if w["hazard_fail"]:
                                ag.fail = True
                            renv += float(w["hazard_penalty"])
                        ag.steps += 1
                    env_term = ag.fail
                    trunc = t1 > w["max_t"]
                if env_term or trunc:
                    ag.active = False
                # the wrapper steps every agent's RM on its (new) position
                pos = (ag.x, ag.y)
                event = pos if pos in self.det[a] else None
                prev = ag.q
                nxt, rq = rm.transitions.get((prev, event), (prev, 0.0))
                ag.q = nxt
                rm_term = nxt == fin
                term = env_term or rm_term
                out["pos_x"][a][e], out["pos_y"][a][e] = ag.x, ag.y
                out["q"][a][e] = self.index[a][nxt]
                out["renv"][a][e] = renv
                out["reward"][a][e] = renv + float(w["reward_modifier"]) * float(rq)
                if w.get("shaping_gamma") is not None:
                    phi = rm.potentials
                    out["shaping"][a][e] = float(w["shaping_gamma"]) * phi.get(nxt, 0) - phi.get(prev, 0)
                out["flags"][a][e] = (ag.steps << 16) | (F_ACTIVE if ag.active else 0) | (F_FAIL if ag.fail else 0) | \
                    (F_TERM if term else 0) | (F_TRUNC if trunc else 0) | (F_ENV_TERM if env_term else 0) | \
                    (F_RM_TERM if rm_term else 0)
                all_term &= term
                all_trunc &= trunc
            self.t[e] = t1
            self.done[e] = all_term or all_trunc
            if self.done[e]:
                for a in range(A):
                    out["flags"][a][e] |= F_ENV_DONE
        out["t"] = list(self.t)
        out["env_done"] = [int(d) for d in self.done]
        return out


def world_from_scenario(desc, max_t=1000):
    """A tests/golden/configs.json scenario with ``rm`` rows as a world dict, through the map parsers only (no
    compiled table): rmx.tables.scenario_symbols and the rows' own labels."""
    from rmx import maps as _maps
    from rmx import tables as T

    sym, parsed = T.scenario_symbols(desc)
    rms = [T._rm_from_rows(ag["rm"], sym) for ag in desc["agents"]]
    sg = desc.get("shaping_gamma")
    if sg is not None:
        for rm in rms:
            rm.add_reward_shaping(sg, sg)
    n = len(rms)
    common = {"starts": [tuple(ag["start"]) for ag in desc["agents"]], "rms": rms, "shaping_gamma": sg,
              "reward_modifier": desc.get("reward_modifier", 1.0), "max_t": max_t}
    if desc["kind"] == "frozen_lake":
        w, h = parsed["dims"]
        return dict(common, kind="frozen_lake", width=w, height=h, hazards=set(parsed["holes"]), walls=set(),
                    detectors=[set(parsed["goals"].values())] * n, hazard_penalty=desc.get("penalty", 0.0),
                    wall_penalty=0.0, hazard_fail=True, wall_fail=False)
    gh, gw = parsed["grid_size"]
    walls = {(tuple(a), tuple(b)) for a, b in parsed["walls"]} | {(tuple(b), tuple(a)) for a, b in parsed["walls"]}
    det = {tuple(sym[s]) for s in _maps.OFFICE_WORLD_EVENT_SYMBOLS if s in sym}
    return dict(common, kind="office_world", width=gw, height=gh, hazards=set(parsed["coords"]["plant"]), walls=walls,
                detectors=[det] * n, hazard_penalty=desc.get("plants_penalty", -100.0),
                wall_penalty=desc.get("wall_penalty", 0.0), hazard_fail=desc.get("terminate_on_plants", False),
                wall_fail=desc.get("terminate_hit_walls", False))
