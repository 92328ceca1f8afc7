#!/usr/bin/env python3
"""What SC_TICK_ANCHORED_SWEEPS costs: one leg of the comparison per process.

    SC_TICK_LIB=<libsc_tick.so of the build under test> python tools/anchored_sweep_cost.py --mode none|sweeps|anchored [--exact] [--ticks 200]

The config-5 world with a collider on every entity (as tools/sweep_shapes_cost.py) and 4 096 capsule sweeps of 10 m (radius 0.4, half
height 0.5), each from 2 m above a vehicle in a random level direction.  --mode anchored: the sweeps ride on the vehicles (movers) --
local start (0, 2, 0) undone by the carrier's scale, the end a world offset (end_frame 1), skip_self --, SC_TICK_ANCHORED_SWEEPS.
--mode sweeps: the same segments in world space, where those vehicles are when the leg starts, as plain SC_TICK_SWEEPS with the
carrier's id skipped -- what the anchored tick is held against, and a leg a build of the parent commit can run; the difference is what
the resolve and the two segment stores add.  --mode none: no set, no flag.  Every tick is FULL | PRODUCE_NEXT with the movers as the
frame producer.  Prints one JSON line: the wall time of a tick with and without the flag (bursts ending in a synchronise), the
SC_TICK_K_PAIRS slot of ticks sampled afterwards (the pair search behind the queries: it must not move), the hits and in exact mode the
report.  Under rocprofv3 --kernel-trace --stats the kernel table gives k_anchored_sweeps<false> / <true> and k_sweep_queries<false> /
<true> in microseconds per launch."""
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
ap.add_argument("--mode", default="anchored", choices=["none", "sweeps", "anchored"])
ap.add_argument("--exact", action="store_true")
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
rng = np.random.default_rng(3801)
k = args.sweeps
kind = getattr(w, "mover_kind", None)
vehicles = np.flatnonzero((w.parent < 0) & (kind != 0)) if kind is not None and (kind != 0).any() else np.flatnonzero(w.parent < 0)
anchor = rng.choice(vehicles, k).astype(np.uint32)
yaw = rng.uniform(0, 2 * np.pi, k)
offset = (np.stack([np.cos(yaw), np.zeros(k), np.sin(yaw)], axis=1) * 10.0).astype(F)
# the carriers are yawed roots: their y axis is the world's, so a local (0, 2 / scale.y, 0) is 2 m above them
local_start = np.stack([np.zeros(k), 2.0 / w.scale[anchor, 1].astype(np.float64), np.zeros(k)], axis=1).astype(F)
cap_r, cap_hh, mask = np.full(k, 0.4, F), np.full(k, 0.5, F), np.full(k, 0xFFFFFFFF, np.uint32)

t = WorldTick.from_world(w, broadphase=True)
t.upload_colliders(0, typ, he, radius, hh)
t.set_view_proj(camera_view_proj(w.camera))
t.set_frame_producer(2, 1.0 / 60.0)
t.advance_movers(1.0 / 60.0)
if args.exact:
    t.set_sweep_shapes(capi.SWEEP_SHAPES_EXACT)
PLAIN = capi.FULL | capi.PRODUCE_NEXT
legs, flag, read, report = [("without", PLAIN)], 0, None, None
if args.mode == "sweeps":
    # the vehicles drive on while a leg runs: the world-space sweeps start where the vehicles ARE after as many ticks as the other
    # leg's first burst, so that both legs sweep through about the same surroundings
    for _ in range(30 + args.ticks):
        t.run(PLAIN)
    a = (t.positions()[anchor] + F([0, 2.0, 0])).astype(F)
    t.set_sweep_queries(a, (a + offset).astype(F), cap_r, cap_hh, mask, skip_id=anchor)
    flag, read, report = capi.SWEEPS, t.sweep_hits, t.sweep_shape_info
if args.mode == "anchored":
    t.anchored_sweeps(anchor, local_start, offset, cap_r, cap_hh, mask, end_frame=np.ones(k, np.uint8))
    flag, read, report = capi.ANCHORED_SWEEPS, t.anchored_sweep_hits, t.anchored_sweep_shape_info
if flag:
    legs = [("with_flag", PLAIN | flag), ("without", PLAIN), ("with_flag_again", PLAIN | flag)]
wall = {}
for name, flags in legs:
    for _ in range(30):
        t.run(flags)
    t.sync()
    t0 = time.perf_counter()
    for _ in range(args.ticks):
        t.run(flags)
    t.sync()
    wall[name] = round((time.perf_counter() - t0) / args.ticks * 1e6, 2)
out = {"lib": os.path.basename(os.path.dirname(capi.LIB_PATH)) + "/" + os.path.basename(capi.LIB_PATH), "mode": args.mode, "exact": bool(args.exact),
       "entities": int(w.n), "sweeps": k, "tick_us": wall}
# the pair search's own slot, sampled: with and without the flag
slot = {}
for name, flags in (("with_flag", PLAIN | flag), ("without", PLAIN)) if flag else (("without", PLAIN),):
    t.set_profiling(1)
    t.set_profiling_kernels([capi.K_PAIRS])
    for _ in range(60):
        t.run(flags)
    t.sync()
    ms = t.kernel_times_ms(capi.K_PAIRS)[10:]
    slot[name] = {"n": int(len(ms)), "median_us": round(float(np.median(ms)) * 1e3, 2), "min_us": round(float(ms.min()) * 1e3, 2)}
    t.set_profiling(0)
out["k_pairs_us"] = slot
if flag:
    t.run(PLAIN | flag)
    hits = read()
    out["hits"] = int(hits["hit"].sum())
    out["mean_travel_m"] = round(float(hits["travel"][hits["hit"] == 1].mean()), 3) if out["hits"] else 0.0
    if args.mode == "anchored":
        out["unanswered"] = int((hits["pad"] != 0).sum())
    if args.exact:
        out["info"] = report()
print(json.dumps(out), flush=True)
t.close()
