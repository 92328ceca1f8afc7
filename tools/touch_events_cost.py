#!/usr/bin/env python3
"""What SC_TICK_TOUCH_EVENTS costs, in one process on one device.

    python tools/touch_events_cost.py [--workload config5|forest] [--parent build_ab/libsc_tick_parent.so]

The caller-owned split flow -- scTickRun(FULL | PRODUCE_NEXT | SPLIT_PAIRS | <flag set>) then scTickRunPairs -- whose SC_TICK_K_PAIRS
event slot brackets the pair half: border merge, pair search, the narrow-phase pass, the event tails.  Four flag sets on this build,
each on a context of its own over the same world, and the first of them on a build of the parent commit (--parent):

    PAIR_SHAPES | PAIR_EVENTS                   what a host ran before touch events, diffing the touching list itself
    TOUCH_EVENTS                                the events alone: no touching list is written
    PAIR_SHAPES | TOUCH_EVENTS                  list and events from one pass
    PAIR_SHAPES | TOUCH_EVENTS | PAIR_EVENTS    everything

config5: 1 048 576 entities, every one with a collider, BOX / SPHERE / CAPSULE by index modulo 3 sized from its bounds (the "mixed" leg of
tools/pair_shapes_cost.py).  forest: the 2 000 entities of tests/pair_shapes_cases.py.  Interleaved rounds: the wall time of a burst of
steps ending in a synchronise, then on a separate profiled burst the K_PAIRS slot alone; median and min - max over the rounds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SC_TICK_LAX_BIND", "1")                  # the parent's build lacks the newer symbols
from sc_gameengine_amd import capi, synth_world as sw          # noqa: E402
from sc_gameengine_amd.tick import WorldTick, camera_view_proj  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="config5")
ap.add_argument("--parent", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=200)
args = ap.parse_args()

if args.workload == "config5":
    w = sw.generate_config5(128, 256)
    kind, param = 2, 1.0 / 60.0
    he = ((w.bmax - w.bmin) * np.float32(0.5)).astype(np.float32)
    radius = np.maximum(he[:, 0], he[:, 2]).astype(np.float32)
    col = ((capi.COLLIDER_BOX + np.arange(w.n) % 3).astype(np.uint8), he, radius, np.maximum(he[:, 1] - radius, 0).astype(np.float32))
    vp = camera_view_proj(w.camera)
elif args.workload == "forest":
    from tests import pair_shapes_cases                        # noqa: E402
    w, c = pair_shapes_cases.forest()
    kind, param = 1, 0.01
    col = (c.type, c.he, c.radius, c.hh)
    vp = None
else:
    ap.error(f"unknown workload {args.workload}")
SPLIT = capi.FULL | capi.PRODUCE_NEXT | capi.SPLIT_PAIRS
S, P, T = capi.PAIR_SHAPES, capi.PAIR_EVENTS, capi.TOUCH_EVENTS
this_lib = capi.LIB_PATH


def step(t, flags):
    t.run(flags)
    t.run_pairs()


ROOM = None          # what every list, table and event list is sized for: twice the pair count of the first tick (a sweep costs by the slot)


def context(lib, flags):
    global ROOM
    capi._LIB = None
    capi.LIB_PATH = os.path.abspath(lib)
    t = WorldTick.from_world(w, broadphase=True)
    t.upload_colliders(0, *col)
    if vp is not None:
        t.set_view_proj(vp)
    t.set_frame_producer(kind, param)
    (t.advance_movers if kind == 2 else t.nudge_roots_x)(param)
    if ROOM is None:
        step(t, SPLIT)
        ROOM = max(2 * int(t.counts().pairs), 1024)
    room = ROOM
    if flags & S:
        t.set_pair_shapes(room)
    if flags & P:
        t.set_pair_events(room, room)
    if flags & T:
        t.set_touch_events(room, room)
    return t


legs = {}
if args.parent:
    legs["parent: PAIR_SHAPES | PAIR_EVENTS"] = (context(args.parent, S | P), SPLIT | S | P)
for name, f in (("PAIR_SHAPES | PAIR_EVENTS", S | P), ("TOUCH_EVENTS", T), ("PAIR_SHAPES | TOUCH_EVENTS", S | T),
                ("PAIR_SHAPES | TOUCH_EVENTS | PAIR_EVENTS", S | T | P)):
    legs[name] = (context(this_lib, f), SPLIT | f)
for t, flags in legs.values():
    for _ in range(30):
        step(t, flags)
    t.sync()
res = {k: {"step_us": [], "pair_half_us": []} for k in legs}
for rnd in range(args.rounds):
    for name, (t, flags) in legs.items():
        for _ in range(20):
            step(t, flags)
        t.sync()
        t0 = time.perf_counter()
        for _ in range(args.burst):
            step(t, flags)
        t.sync()
        res[name]["step_us"].append((time.perf_counter() - t0) / args.burst * 1e6)
        t.set_profiling(1)
        t.set_profiling_kernels([capi.K_PAIRS])
        for _ in range(40):
            step(t, flags)
        res[name]["pair_half_us"].append(float(np.median(t.kernel_times_ms(capi.K_PAIRS)[-40:])) * 1e3)
        t.set_profiling(0)
for name, (t, flags) in legs.items():
    r = res[name]
    out = {"workload": args.workload, "leg": name, "entities": int(w.n), "pairs": int(t.counts().pairs), "room": ROOM}
    for key in ("pair_half_us", "step_us"):
        out[key] = {"median": round(float(np.median(r[key])), 2), "min": round(float(np.min(r[key])), 2), "max": round(float(np.max(r[key])), 2)}
    if flags & S:
        out["touching_list"] = t.read_pair_shapes()[1]
    if flags & P:
        out["pair_events"] = t.pair_events()[2]
    if (flags & T) and not name.startswith("parent"):
        out["touch_events"] = t.touch_events()[2]
    print(json.dumps(out), flush=True)
for t, _ in legs.values():
    t.close()
