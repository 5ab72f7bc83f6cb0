"""The learn kernel (csrc/rmx_learn.hip) at its limits and in mixed use; the host half, the restatement and the
liveness of the inputs: tests/test_learn_limits_cpu.py.

* Device against host, bit for bit, on every limit world of tests/test_limits_gpu.py and on the 65,344-byte table
  blob: every agent-count bucket with a partial wave and a partial 256-thread block, 249 counterfactuals per
  agent-step, QRM list bytes / RM indices / event ids above 127, rows up to 20,479.
* One device handle through every entry point of a training loop, beside a host handle: the learn kernel accounts
  episodes in the per-wave slab (256-thread geometry), the fast step in per-env slots (64-thread blocks), the fused
  report sums both; the packed window's record, the reset cache and the slab carry nothing across a segment.
* Rebinding tables, gamma and phi; special values in the tables; out-of-range columns, between guard tables.
"""
import dataclasses

import numpy as np
import pytest

import learn_common as LC
import test_learn_limits_cpu as CPU
import test_limits_gpu as LIM
from rmx import tables as T
from rmx.engine import HostRMEnv, VecRMEnv
from rmx.learn import VecQLearning
from test_random_maps_gpu import CASES, random_tables

pytestmark = pytest.mark.gpu

KNOBS = LIM.KNOBS + ("RMX_SEQ_PACKED", "RMX_QUEUE")


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _dev_actions(a):
    import torch
    return torch.as_tensor(a, device="cuda")


def _limit_tables(name):
    if name == "generic_blob_under":
        tab = LIM.size_world(**LIM.SIZE_EDGES[name][0])
        assert LIM.generic_blob_bytes(tab) == 65344 and tab.n_rm_states == 113
        return tab
    return LIM.limit_world(name)[1]


@pytest.mark.parametrize("use_qrm", [True, False])
@pytest.mark.parametrize("name", list(LIM.CASES) + ["generic_blob_under"])
def test_device_equals_host_on_the_limit_worlds(name, use_qrm):
    """N = 65 (A <= 2) / 257 (A = 5, 7, 8): a partial wave and a partial block.  The learn kernel stages the generic
    table blob in LDS with 256 threads whatever the handle's own step kernel is; at 65,344 B it must still launch."""
    tab = dataclasses.replace(_limit_tables(name), max_t=20)
    N = 257 if tab.n_agents > 2 else 65
    lr = 0.3 if use_qrm else None
    rsh = use_qrm and tab.phi is not None
    K = 60
    kw = dict(with_qrm=True, with_enc_state=True)
    dev, hst = VecRMEnv(tab, N, **kw), HostRMEnv(tab, N, **kw)
    Ld = VecQLearning(dev, 0.9, lr, qtable_init=0.25, use_qrm=use_qrm, use_rsh=rsh)
    Lh = VecQLearning(hst, 0.9, lr, qtable_init=0.25, use_qrm=use_qrm, use_rsh=rsh)
    acts = hst.fill_actions(21, 0, K)
    dacts = _dev_actions(acts)
    for t in range(K):
        Ld.step(dacts[t])
        Lh.step(acts[t])
    dev.check_errors()
    LC.assert_same_bits(Ld.q, Lh.q, (name, "q"))
    LC.assert_same_bits(Ld.visits, Lh.visits, (name, "visits"))
    LC.assert_same_columns(LC.columns(dev), LC.columns(hst), name)
    assert (Lh.visits > 0).any() and (hst.t < K).all()
    dev.close()


# ---- one handle, every entry point ---------------------------------------------------------------------------------
def _packed(env):
    return bool(env.lib.rmx_seq_packed(env._h))


@pytest.mark.parametrize("N", [65, 257])
@pytest.mark.parametrize("world", sorted(CPU.MIXED_WORLDS))
def test_one_device_handle_through_every_entry_point(world, N, monkeypatch):
    """The script of learn_common.mixed_use on a device handle and a host handle.  The handle runs the fast step with
    merged tables (forced: the 4-agent world's merged table is past the default's 128 KiB, and only merged tables
    pack a window), so plain steps use per-env statistics slots, the fused report and the packed record, and learn
    steps the per-wave slab.  Between the segments another pair of device handles runs a window on the same queue.
    The return sum is compared as bits: float32 episode returns of magnitude 2^-8 .. 2^8 over a few hundred
    episodes, every partial sum exact in float64 (as in test_learn_gpu).  Measured on the host: the lake ends
    episodes in every segment (23 / 95 by the first report at N = 65 / 257, 6 / 18 between the clear and the last
    report); the OfficeWorld's agents neither fail nor finish within the 19 steps before the rollout, so its first
    43 / 171 episodes are the truncations inside the rollout and its statistics are zero before."""
    import torch
    monkeypatch.setenv("RMX_FAST_TABLES", "merged")
    tab = dataclasses.replace(random_tables(*CPU.MIXED_WORLDS[world]), max_t=20)
    dev, hst = VecRMEnv(tab, N, with_enc_state=True), HostRMEnv(tab, N, with_enc_state=True)
    assert dev.step_info["variant"] == "fast" and dev.step_info["tables"] == "merged" and dev.report_fused
    kw = dict(use_qrm=True, qtable_init=0.0)
    Ld, Lh = VecQLearning(dev, 0.9, 0.2, **kw), VecQLearning(hst, 0.9, 0.2, **kw)
    # the other pair: BASELINE config 2, one handle stepped, one running windows
    tab2 = T.compile_scenario(T.baseline_scenario(2))
    a2, b2 = VecRMEnv(tab2, 257, with_enc_state=True), VecRMEnv(tab2, 257, with_enc_state=True)
    acts2 = torch.as_tensor(np.random.default_rng(12).integers(0, 5, size=(16 * 5, 2, 257), dtype=np.int32),
                            device="cuda").contiguous()
    windows = [0]

    def between(seg):
        w = windows[0]
        windows[0] += 1
        for s in range(5 * w, 5 * w + 5):
            a2.step(acts2[s])
        b2.step_seq(acts2[5 * w:5 * w + 5])
        assert _packed(b2)
        LC.assert_same_columns(LC.columns(a2), LC.columns(b2), ("other pair", seg))

    def after_seq():
        assert _packed(dev)

    seen = LC.mixed_use(LC.EngineSide(dev, Ld, _dev_actions), LC.EngineSide(hst, Lh), tab.n_agents, N, between,
                        after_seq)
    assert seen["episodes"] > 0 and seen["visited"] > 0
    if world == "fl_a2":  # episodes end in every part of the script, between the clear and the last report too
        assert seen["episodes_at_report"] > 0 and seen["episodes_after_clear"] > 0
    assert seen["segments"] == 15 == windows[0]
    assert torch.equal(a2.stats_tensor(), b2.stats_tensor())
    for e in (dev, a2, b2):
        e.check_errors()
        e.close()


# ---- rebind --------------------------------------------------------------------------------------------------------
def _dev_table(env, L, fill):
    t = env.torch
    return t.full(tuple(L.q.shape), fill, dtype=t.float64, device=env.device)


def test_rebinding_tables_gamma_and_phi_on_a_device_handle():
    tab = CPU.rebind_world()
    N = 65
    h = CPU.rebind_phases(HostRMEnv, CPU.host_table, lambda a: a, tab, N)
    d = CPU.rebind_phases(VecRMEnv, _dev_table, _dev_actions, tab, N)
    CPU.check_rebind(d, [h["x1"], h["y2"], h["z"]])


# ---- special values in the tables ----------------------------------------------------------------------------------
def _torch_fill(dst, src):
    import torch
    dst.copy_(torch.as_tensor(src))


@pytest.mark.parametrize("lr", [0.3, None])
@pytest.mark.parametrize("values", [LC.SPECIAL, LC.SPECIAL_NEG], ids=["nonneg", "neg_inf_nan"])
def test_special_values_in_the_tables_on_the_device(values, lr):
    tab = random_tables(*CASES["ow_regs_eligible"])
    ha, hq, hv, q0 = CPU.special_run(HostRMEnv, CPU.np_fill, tab, values, lr)
    da, dq, dv, _ = CPU.special_run(VecRMEnv, _torch_fill, tab, values, lr)
    for t in range(len(ha)):
        assert np.array_equal(da[t], ha[t]), t
    LC.assert_same_but_nan(dq, hq, "q")
    LC.assert_same_bits(dv, hv, "visits")
    CPU.check_special(values, ha, hq, q0)


# ---- out-of-range columns, between guard tables --------------------------------------------------------------------
@pytest.mark.parametrize("use_qrm", [True, False])
def test_out_of_range_columns_on_the_device_between_guards(use_qrm):
    """pos_x / pos_y / rm_q of every second env overwritten slightly out of range (x in [W, W+2], y in [H, H+1], rm_q in
    [enc_nq, enc_nq+3]; alone and together), on the 12 x 10 world whose agents own 720, 360 and 480 of the 720 rows.
    The tables are views into one allocation with a guard of one whole learner before the first and after the last
    learner.  Before anything is launched the largest row an update WITHOUT the range check could form from these
    values is computed and must stay inside the following learner or the guard: a missing check fails an assertion
    below, it does not leave the test's memory.  (rm_q after a step is a table byte, <= 255; x and y move by at most
    one per step, and the garbage is rewritten every three steps.)  The device leaves the garbage envs themselves
    unspecified (the host clamps such columns to 0 first), so only the guards, the rows past each agent's own count
    and the clean envs are pinned."""
    import torch
    tab = LC.uneven_world()
    W, H, A, N = tab.width, tab.height, tab.n_agents, 66
    enc = [int(v) for v in tab.enc_nq]
    own = [W * H * n for n in enc]
    dev, hst = VecRMEnv(tab, N), HostRMEnv(tab, N)
    lr = 0.3 if use_qrm else None
    kw = dict(qtable_init=0.5, use_qrm=use_qrm, use_rsh=use_qrm)
    Ld, Lh = VecQLearning(dev, 0.9, lr, **kw), VecQLearning(hst, 0.9, lr, **kw)
    S_max = Ld.S_max
    assert (W, H, S_max) == (12, 10, 720)
    steps = 3  # learn steps between two garbage writes
    cell_max = (H + 1 + steps) * W + (W + 2 + steps)
    row_max = cell_max * max(enc) + 255
    assert row_max < 2 * S_max, (row_max, S_max)  # inside the next learner, or the guard after the last one
    SENT = 12345.678
    per = S_max * 4
    big = [torch.full(((A * N + 2) * per,), SENT, dtype=torch.float64, device="cuda") for _ in range(2)]
    qv, vv = (b[per:(A * N + 1) * per].view(A, N, S_max, 4) for b in big)
    qv.fill_(0.5)
    vv.fill_(0.0)
    LC.bind(Ld, qv, vv, 0.9, lr, use_qrm, use_qrm, phi=tab.phi)
    lanes = np.arange(1, N, 2)
    form = (lanes // 2) % 4  # 0: x, y and rm_q; 1: x only; 2: y only; 3: rm_q only
    lanes_t = torch.as_tensor(lanes, device="cuda")
    out_d = torch.zeros((A, N), dtype=torch.int32, device="cuda")
    out_h = np.zeros((A, N), np.int32)
    acts = hst.fill_actions(6, 0, 9)
    dacts = _dev_actions(acts)
    n_garbage = 0
    for rnd in range(3):
        for a in range(A):
            k = lanes // 2 + rnd + a
            for col, sel, val in ((dev.pos_x, (form == 0) | (form == 1), W + k % 3),
                                  (dev.pos_y, (form == 0) | (form == 2), H + k % 2),
                                  (dev.rm_q, (form == 0) | (form == 3), enc[a] + k % 4)):
                new = torch.as_tensor(val[sel].astype(np.int32), device="cuda")
                assert int(new.min()) >= 0 and int(new.max()) <= max(W + 2, H + 1, enc[a] + 3)
                col[a, lanes_t[torch.as_tensor(sel, device="cuda")]] = new
                n_garbage += int(sel.sum())
        for s in range(steps):
            t = rnd * steps + s
            if s == 1:  # a policy step: a state outside the table reads a zero row, never the next learner's
                Ld.act_step(0.3, 5, t, actions_out=out_d)
                Lh.act_step(0.3, 5, t, actions_out=out_h)
                assert np.array_equal(out_d.cpu().numpy()[:, ::2], out_h[:, ::2]), t
            else:
                Ld.step(dacts[t])
                Lh.step(acts[t])
    dev.check_errors()
    assert n_garbage > 0
    for b in big:
        g = b.cpu().numpy()
        assert (g[:per] == SENT).all() and (g[(A * N + 1) * per:] == SENT).all(), "a guard table was written"
    q, v = qv.cpu().numpy(), vv.cpu().numpy()
    for a in range(A):  # rows past the agent's own count, in every env
        assert (q[a, :, own[a]:] == 0.5).all() and (v[a, :, own[a]:] == 0.0).all(), a
    LC.assert_same_bits(q[:, ::2], Lh.q[:, ::2], "clean envs, q")
    LC.assert_same_bits(v[:, ::2], Lh.visits[:, ::2], "clean envs, visits")
    assert (Lh.visits[:, ::2] > 0).any()
    dev.close()
