"""bench.py's plain run (no --full): the headline line and nothing else, --steps timed steps, and --dump-outputs writing
what the last timed step computed -- the same files on a second run with the same arguments, and the oracle's frame."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from sc_gameengine_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECTORS, STEPS, WARMUP = 16, 5, 2


def run_plain(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--sectors", str(SECTORS), "--steps", str(STEPS),
           "--warmup", str(WARMUP), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1500:]
    return json.loads(lines[0])


@pytest.mark.timeout(600)
def test_plain_run_prints_the_headline_and_dumps_the_last_timed_step(oracle, tmp_path):
    d = run_plain(tmp_path / "a")
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["unit"] == "entities/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["metric"].startswith("entities/sec world-tick")
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(d["config"]["entities_total"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["config"]["full"] is False and "skipped" in d["parity_in_run"]
    for key in ("roofline", "cpu_baseline", "secondary", "end_to_end"):
        assert key not in d, key

    files = sorted(os.listdir(tmp_path / "a"))
    assert {"world_matrices.npy", "world_matrix_rows.npy", "visible.npy", "counts.npy"} <= set(files), files
    arrays = {f: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) and a.size > 0 for a in arrays.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20

    # the same arguments give the same files
    run_plain(tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "b")) == files
    for f in files:
        assert np.array_equal(np.load(tmp_path / "b" / f), arrays[f]), f

    # the last timed step's frame is the oracle's after W + K producer applications (one explicit, then one fused per step)
    w, _, _ = bench.make_world(argparse.Namespace(sectors=SECTORS, workload="config3"), 0, (1, 1))
    from sc_gameengine_amd.tick import camera_view_proj
    ow = oracle.OracleWorld.from_arrays(w.pos, w.rot, w.scale, w.parent, w.bmin, w.bmax, has_mesh=w.has_mesh, has_bounds=w.has_bounds)
    for _ in range(WARMUP + STEPS):
        ow.nudge_roots_x(0.01)
    ow.transform_system()
    ow.culling_system(view_proj=camera_view_proj(w.camera))
    rows = arrays["world_matrix_rows.npy"].astype(np.int64)
    assert np.array_equal(rows, np.arange(w.n))                       # a small world is dumped whole
    assert np.array_equal(arrays["world_matrices.npy"], ow.world_matrices()[:w.n][rows])
    assert np.array_equal(arrays["visible.npy"], ow.visible().astype(np.float64))
    assert "pairs.npy" not in arrays                                   # config 3: all bodies static, no pair: nothing to write
    counts = dict(zip([f for f, _ in capi.Counts._fields_], arrays["counts.npy"]))
    assert counts["pairs"] == 0 and counts["visible"] == len(arrays["visible.npy"]) and counts["entities"] == w.n
    ow.close()
