#!/usr/bin/env python3
"""What pair sleep (scTickSetPairSleep) adds to the pair half, in one process on one device.

    python tools/pair_sleep_cost.py [--legs box,mixed,empty,box-rest,box-moving] [--rounds 5] [--burst 200]

The flow, the legs and the slot of tools/pair_islands_cost.py: scTickRun(FULL | PRODUCE_NEXT | SPLIT_PAIRS | PAIR_SHAPES) then
scTickRunPairs on config 5, the pair half bracketed by the SC_TICK_K_PAIRS event slot; leg "box": every entity a BOX of its bounds' half
extents, leg "mixed": BOX / SPHERE / CAPSULE by index modulo 3, leg "empty": the boxes with every mask 0 -- config 5's movers advance in
all three.  "box-rest": the boxes with nothing produced for the next frame, a world fully at rest; "box-moving": every root nudged by
two tolerances a tick, a world fully moving.  Per leg two contexts on the same world with pair islands on, sleep off and on, timed in
interleaved rounds.  --trace N: no timing, N flagged steps per leg with sleep on -- the run to put under rocprofv3 --kernel-trace
--stats, whose kernel table gives k_pair_sleep_{motion,edges,resolve,finish} per launch."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sc_gameengine_amd import capi, synth_world as sw          # noqa: E402
from sc_gameengine_amd.tick import WorldTick, camera_view_proj  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--legs", default="box,mixed,empty,box-rest,box-moving")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=200)
ap.add_argument("--tol", type=float, default=0.005)
ap.add_argument("--rest-runs", type=int, default=120)
ap.add_argument("--trace", type=int, default=0)
ap.add_argument("--small", action="store_true", help="a small world: a rehearsal of the script, not a measurement")
args = ap.parse_args()

w = sw.generate(8, 8, 15) if args.small else sw.generate_config5(128, 256)
if args.small:
    w.group[:], w.mask[:] = sw.GROUP_DYNAMIC, sw.MASK_ALL
kind, param = (1, 0.01) if args.small else (2, 1.0 / 60.0)
vp = camera_view_proj(w.camera)
SPLIT = capi.FULL | capi.PRODUCE_NEXT | capi.SPLIT_PAIRS | capi.PAIR_SHAPES
REST = capi.FULL | capi.SPLIT_PAIRS | capi.PAIR_SHAPES
he = ((w.bmax - w.bmin) * np.float32(0.5)).astype(np.float32)


def colliders(leg):
    if not leg.startswith("mixed"):
        return np.full(w.n, capi.COLLIDER_BOX, np.uint8), he, np.full(w.n, 0.5, np.float32), np.full(w.n, 0.5, np.float32)
    typ = (capi.COLLIDER_BOX + np.arange(w.n) % 3).astype(np.uint8)
    radius = np.maximum(he[:, 0], he[:, 2]).astype(np.float32)
    return typ, he, radius, np.maximum(he[:, 1] - radius, 0).astype(np.float32)


def context(leg, sleep):
    t = WorldTick.from_world(w, broadphase=True)
    t.upload_colliders(0, *colliders(leg))
    if leg == "empty":
        t.upload_layers(0, w.group, np.zeros(w.n, np.uint32))
    t.set_view_proj(vp)
    if leg.endswith("-moving"):
        t.set_frame_producer(1, 2.0 * args.tol)
        t.nudge_roots_x(2.0 * args.tol)
    elif not leg.endswith("-rest"):
        t.set_frame_producer(kind, param)
        (t.advance_movers if kind == 2 else t.nudge_roots_x)(param)
    t.set_pair_shapes(max(int(t.max_pairs), 1))
    t.pair_islands(True, 2)
    if sleep:
        t.pair_sleep(True, args.tol, args.tol, args.rest_runs, 1 << 16)
    t.flags = REST if leg.endswith("-rest") else SPLIT
    return t


def step(t):
    t.run(t.flags)
    t.run_pairs()


for leg in args.legs.split(","):
    if args.trace:
        t = context(leg, True)
        for _ in range(args.trace):
            step(t)
        t.sync()
        print(json.dumps({"colliders": leg, "steps": args.trace, "info": t.read_pair_shapes()[1], "sleep": t.read_pair_sleep()[3]}), flush=True)
        t.close()
        continue
    ctxs = {"sleep off": context(leg, False), "sleep on": context(leg, True)}
    for t in ctxs.values():
        for _ in range(30):
            step(t)
        t.sync()
    res = {k: {"step_us": [], "pair_half_us": []} for k in ctxs}
    for rnd in range(args.rounds):
        for name, t in ctxs.items():
            for _ in range(20):
                step(t)
            t.sync()
            t0 = time.perf_counter()
            for _ in range(args.burst):
                step(t)
            t.sync()
            res[name]["step_us"].append((time.perf_counter() - t0) / args.burst * 1e6)
            t.set_profiling(1)
            t.set_profiling_kernels([capi.K_PAIRS])
            for _ in range(40):
                step(t)
            res[name]["pair_half_us"].append(float(np.median(t.kernel_times_ms(capi.K_PAIRS)[-40:])) * 1e3)
            t.set_profiling(0)
    for name, t in ctxs.items():
        r = res[name]
        out = {"workload": "small" if args.small else "config5", "colliders": leg, "leg": name, "entities": int(w.n), "pairs": int(t.counts().pairs),
               "step_us_median": round(float(np.median(r["step_us"])), 2), "step_us_min": round(float(np.min(r["step_us"])), 2),
               "step_us_max": round(float(np.max(r["step_us"])), 2),
               "pair_half_us_median": round(float(np.median(r["pair_half_us"])), 2), "pair_half_us_min": round(float(np.min(r["pair_half_us"])), 2),
               "pair_half_us_max": round(float(np.max(r["pair_half_us"])), 2), "info": t.read_pair_shapes()[1]}
        if name.endswith("on"):
            out["sleep"] = t.read_pair_sleep()[3]
        print(json.dumps(out), flush=True)
    for t in ctxs.values():
        t.close()
