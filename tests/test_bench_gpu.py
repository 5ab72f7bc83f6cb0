"""bench.py --dump-outputs on the GPU: the arrays a plain run writes are what the CPU oracle computes for the last
reported window (its seed's actions, reset, W warmup steps, K steps), both when the window fits the action buffer and
when it reads a small buffer cyclically as several rmx_step_seq calls."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENVS = 4096


@pytest.mark.gpu
@pytest.mark.parametrize("K,W,buf_mb", [(20, 5, 4096), (100, 37, 1)], ids=["one-run", "cyclic"])
def test_dumped_outputs_equal_the_oracle(K, W, buf_mb, tmp_path):
    import bench
    import oracle as O
    from rmx import tables as T

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup",
                        str(W), "--n-envs", str(N_ENVS), "--spin-ms", "20", "--act-buf-mb", str(buf_mb),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == K and line["ms_per_step"] > 0 and line["config"]["dispatch"] == "queue"
    assert line["roofline"] is None and line["configs"] == {} and line["detail"] is None  # a plain run

    tab = T.compile_scenario(T.baseline_scenario(2))
    A = tab.n_agents
    rows = min(W + K, (buf_mb << 20) // (4 * A * N_ENVS))
    assert (rows < W + K) == (buf_mb == 1) and len(bench.act_segments(W, K, rows)) == (4 if buf_mb == 1 else 1)
    acts = O.hash_actions(bench.WINDOW_SEEDS[-1], 0, rows, N_ENVS, 0, N_ENVS, A)
    orc = O.OracleEnv(tab, N_ENVS)
    for g in range(W + K):
        orc.step(acts[g % rows])
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"pos_x", "pos_y", "rm_q", "flags", "t", "ep_ret", "reward", "env_done", "report"}
    for k, v in got.items():
        assert v.dtype in (np.float32, np.float64), k
    for k in ("pos_x", "pos_y", "rm_q", "t", "env_done", "reward", "ep_ret"):
        np.testing.assert_array_equal(got[k], getattr(orc, k), err_msg=k)
    np.testing.assert_array_equal(got["flags"], orc.flags.astype(np.float64))
    rep, so = got["report"], orc.stats
    assert rep[1] == so[1] and rep[2] == so[2] and rep[3] == so[3] and abs(rep[0] - so[0]) <= 1e-6 * max(1, abs(so[0]))
    assert so[1] > 0  # episodes ended inside the window: the report is not trivially zero
