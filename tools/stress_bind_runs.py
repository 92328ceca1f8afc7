#!/usr/bin/env python3
"""Bind runs and material touches on random worlds, handle ranges, pipeline tables, budgets and table sizes against the witnesses of
tests/bind_runs_ref.py (tests/test_gpu_bind_runs.py::check_binds does the comparing).  python tools/stress_bind_runs.py [--seeds 30]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle_py                                   # noqa: E402
from tests import worlds                                       # noqa: E402
from tests.test_gpu_bind_runs import check_binds               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seeds", type=int, default=30)
args = ap.parse_args()
oracle_py.build()
bad = 0
for seed in range(args.seeds):
    rng = np.random.default_rng(13000 + seed)
    n = int(rng.choice([1, 65, 300, 5000, 30000, 90000]))
    w = worlds.random_world(n, seed=seed, spread=float(rng.choice([40.0, 150.0])), p_child=float(rng.choice([0.0, 0.3])), p_no_mesh=float(rng.choice([0.0, 0.2])))
    nmesh = int(rng.choice([1, 3, 40, 70000]))
    nmat = int(rng.choice([1, 6, 33, 300, 65537, 70000]))
    w.mesh = rng.integers(0, nmesh + 2, w.n).astype(np.uint32)
    w.material = rng.integers(0, nmat + 3, w.n).astype(np.uint32)          # a few handles past the table
    pipeline = rng.integers(0, int(rng.choice([1, 2, 128])), nmat).astype(np.uint8)
    pipeline[rng.random(nmat) < 0.1] = 0xFF
    budget = int(rng.choice([0, 1, 64, 4096, 1 << 20]))
    max_runs = int(rng.choice([1, 7, 64, n]))
    freeze = bool(rng.integers(0, 2))
    try:
        check_binds(oracle_py, w, pipeline, mesh_count=nmesh, max_draws=budget, max_runs=min(max_runs, n), graph=bool(rng.integers(0, 2)), freeze=freeze)
    except AssertionError as e:
        bad += 1
        print(f"seed {seed}: n {n} meshes {nmesh} materials {nmat} budget {budget} max_runs {max_runs} freeze {freeze}: {str(e)[:300]}", flush=True)
print(f"{args.seeds - bad} of {args.seeds} run tables, reports and bitmaps equal")
sys.exit(1 if bad else 0)
