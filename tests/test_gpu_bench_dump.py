"""bench.py --dump-outputs on the device: one plain run of the benchmark at
N=1,024 (every row is kept at this size) writes the stats of its timed
gh_step call and the tables after its last round; they must equal, value for
value, what the CPU oracle computes for the same configuration (full
membership start, the bench's seed and timeouts). A plain run carries none
of the --full legs. Run on a MI355X: pytest -m gpu."""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parents[1]


def test_bench_dump_matches_oracle(tmp_path, oracle_mod):
    n, warmup, steps = 1024, 2, 3
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--n", str(n), "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(tmp_path)], capture_output=True, text=True,
                       timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert d["cpu_baseline"] is None and d["secondary"] is None and d["placement"] is None

    orc = oracle_mod.Oracle(oracle_mod.default_config(n, fanout=4, seed=0x5EED0003, t_fail=16, t_cleanup=16))
    orc.init_full(2, 0, 0)
    orc.step(warmup)
    st = orc.step(steps)
    hb, ts, _ = orc.export_state()
    alive = np.ones(n)  # no member left: alive is the process flag, all running
    orc.close()

    got = {f.name: np.load(f) for f in tmp_path.iterdir()}
    assert sorted(got) == ["alive.npy", "hb_rows.npy", "round_stats.npy", "rows.npy", "ts_rows.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    rows = got["rows.npy"].astype(np.int64)
    assert np.array_equal(rows, np.arange(n))
    assert got["round_stats.npy"].tolist() == [float(v) for v in st.values()], (got["round_stats.npy"], st)
    assert st["rounds"] == steps and st["last_round"] == warmup + steps
    assert np.array_equal(got["hb_rows.npy"], hb[rows]) and np.array_equal(got["ts_rows.npy"], ts[rows])
    assert np.array_equal(got["alive.npy"], alive)
