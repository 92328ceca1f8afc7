#!/usr/bin/env python3
"""What SC_TICK_SWEEP_SHAPES_EXACT costs: one leg of the comparison per process, meant to run under
rocprofv3 --kernel-trace --stats, whose kernel table gives k_sweep_queries<false> / k_sweep_queries<true> in microseconds per launch.

    SC_TICK_LIB=<libsc_tick.so of the build under test> python tools/sweep_shapes_cost.py --mode aabb|exact [--ticks 200]

The config-5 world with a collider on every entity (BOX / SPHERE / CAPSULE by index modulo 3, sized from the bounds' half extents) and
4 096 sweeps of 10 m, each starting 2 m above a random entity in a random level direction, radius 0.4, half height 0.5.  A build of the
parent commit runs the aabb leg alone (it has no other).  Prints one JSON line: the wall time of a tick with and without SC_TICK_SWEEPS
(bursts ending in a synchronise), the hits, and in exact mode the report's words."""
import argparse
import json
import os
import sys
import time

import numpy as np

os.environ.setdefault("SC_TICK_LAX_BIND", "1")                  # the parent's build lacks the newer symbols
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sc_gameengine_amd import capi, synth_world as sw          # noqa: E402
from sc_gameengine_amd.tick import WorldTick, camera_view_proj  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="aabb", choices=["aabb", "exact"])
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--sweeps", type=int, default=4096)
ap.add_argument("--small", action="store_true", help="a small world: a rehearsal of the script, not a measurement")
args = ap.parse_args()

F = np.float32
w = sw.generate(8, 8, 15) if args.small else sw.generate_config5(128, 256)
he = ((w.bmax - w.bmin) * F(0.5)).astype(F)
typ = (capi.COLLIDER_BOX + np.arange(w.n) % 3).astype(np.uint8)
radius = np.maximum(he[:, 0], he[:, 2]).astype(F)
hh = np.maximum(he[:, 1] - radius, 0).astype(F)
rng = np.random.default_rng(2201)
k = args.sweeps
roots = np.flatnonzero(w.parent < 0)
at = w.pos[rng.choice(roots, k)]
yaw = rng.uniform(0, 2 * np.pi, k)
a = (at + F([0, 2.0, 0])).astype(F)
b = (a + np.stack([np.cos(yaw), np.zeros(k), np.sin(yaw)], axis=1) * 10.0).astype(F)

t = WorldTick.from_world(w, broadphase=True)
t.upload_colliders(0, typ, he, radius, hh)
t.set_view_proj(camera_view_proj(w.camera))
t.set_frame_producer(2, 1.0 / 60.0)
t.advance_movers(1.0 / 60.0)
t.set_sweep_queries(a, b, np.full(k, 0.4, F), np.full(k, 0.5, F), np.full(k, 0xFFFFFFFF, np.uint32))
if args.mode == "exact":
    t.set_sweep_shapes(capi.SWEEP_SHAPES_EXACT)
PLAIN = capi.FULL | capi.PRODUCE_NEXT
wall = {}
for name, flags in (("with_sweeps", PLAIN | capi.SWEEPS), ("without", PLAIN), ("with_sweeps_again", PLAIN | capi.SWEEPS)):
    for _ in range(30):
        t.run(flags)
    t.sync()
    t0 = time.perf_counter()
    for _ in range(args.ticks):
        t.run(flags)
    t.sync()
    wall[name] = round((time.perf_counter() - t0) / args.ticks * 1e6, 2)
hits = t.sweep_hits()
out = {"lib": os.path.basename(os.path.dirname(capi.LIB_PATH)) + "/" + os.path.basename(capi.LIB_PATH), "mode": args.mode, "entities": int(w.n),
       "sweeps": k, "tick_us": wall, "hits": int(hits["hit"].sum()), "mean_travel_m": round(float(hits["travel"][hits["hit"] == 1].mean()), 3)}
if args.mode == "exact":
    out["info"] = t.sweep_shape_info()
print(json.dumps(out), flush=True)
t.close()
