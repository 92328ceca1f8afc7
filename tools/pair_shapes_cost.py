#!/usr/bin/env python3
"""What SC_TICK_PAIR_SHAPES costs, and pair contacts and pair manifolds on top of it, in one process on one device.

    SC_TICK_LAX_BIND=1 python tools/pair_shapes_cost.py [--workload config5|config3dyn] [--parent libsc_tick_parent.so]

The caller-owned split flow -- scTickRun(FULL | PRODUCE_NEXT | SPLIT_PAIRS [| PAIR_SHAPES]) then scTickRunPairs -- whose
SC_TICK_K_PAIRS event slot brackets the pair half.  Every entity gets a collider first: leg "box" a BOX of its bounds' half extents
(SynthWorld's bounds are centred: the world AABBs and the pair set stay what they were), leg "mixed" BOX / SPHERE / CAPSULE by index
modulo 3 with sizes from the same half extents (another pair set: its size is printed).  Per leg up to six contexts on the same world --
a build of the parent commit (--parent) without and with the flag, this build without the flag, with it, with it and pair contacts
(scTickSetPairContacts), and with manifolds on top of those (scTickSetPairManifolds) -- are timed in interleaved rounds: the wall
time of a burst of steps ending in a synchronise, then on a separate profiled burst the K_PAIRS slot alone."""
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
ap.add_argument("--workload", default="config5")
ap.add_argument("--parent", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--burst", type=int, default=200)
ap.add_argument("--this-first", action="store_true", help="create and time this build's contexts before the parent's (position effects)")
args = ap.parse_args()

if args.workload == "config5":
    w = sw.generate_config5(128, 256)
    kind, param = 2, 1.0 / 60.0
elif args.workload == "config3dyn":
    w = sw.config("config3")
    dyn = (np.arange(w.n) % 16) == 4
    w.group[dyn], w.mask[dyn] = sw.GROUP_DYNAMIC, sw.MASK_ALL
    kind, param = 1, 0.01
else:
    ap.error(f"unknown workload {args.workload}")
vp = camera_view_proj(w.camera)
SPLIT = capi.FULL | capi.PRODUCE_NEXT | capi.SPLIT_PAIRS
he = ((w.bmax - w.bmin) * np.float32(0.5)).astype(np.float32)
this_lib = capi.LIB_PATH


def colliders(leg):
    if leg == "box":
        return np.full(w.n, capi.COLLIDER_BOX, np.uint8), he, np.full(w.n, 0.5, np.float32), np.full(w.n, 0.5, np.float32)
    typ = (capi.COLLIDER_BOX + np.arange(w.n) % 3).astype(np.uint8)
    radius = np.maximum(he[:, 0], he[:, 2]).astype(np.float32)
    return typ, he, radius, np.maximum(he[:, 1] - radius, 0).astype(np.float32)


def context(lib, leg, flagged, contacts=False, manifolds=False):
    capi._LIB = None
    capi.LIB_PATH = os.path.abspath(lib)
    t = WorldTick.from_world(w, broadphase=True)
    t.upload_colliders(0, *colliders(leg))
    t.set_view_proj(vp)
    t.set_frame_producer(kind, param)
    (t.advance_movers if kind == 2 else t.nudge_roots_x)(param)
    if flagged:
        t.set_pair_shapes(max(int(t.max_pairs), 1))
    if contacts:
        t.set_pair_contacts(True)
    if manifolds:
        t.set_pair_manifolds(True)
    return t


def step(t, flags):
    t.run(flags)
    t.run_pairs()


for leg in ("box", "mixed"):
    legs = []
    if args.parent:
        legs += [("parent, flag off", args.parent, False, False, False), ("parent, flag on", args.parent, True, False, False)]
    legs += [("this build, flag off", this_lib, False, False, False), ("this build, flag on", this_lib, True, False, False),
             ("this build, flag on, contacts on", this_lib, True, True, False), ("this build, flag on, contacts on, manifolds on", this_lib, True, True, True)]
    if args.this_first:
        legs.reverse()
    ctxs = {name: (context(lib, leg, flagged, contacts, manifolds), SPLIT | (capi.PAIR_SHAPES if flagged else 0)) for name, lib, flagged, contacts, manifolds in legs}
    for t, flags in ctxs.values():
        for _ in range(30):
            step(t, flags)
        t.sync()
    res = {k: {"step_us": [], "pair_half_us": []} for k in ctxs}
    for rnd in range(args.rounds):
        for name, (t, flags) in ctxs.items():
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
    for name, (t, flags) in ctxs.items():
        r = res[name]
        out = {"workload": args.workload, "colliders": leg, "leg": name, "entities": int(w.n), "pairs": int(t.counts().pairs),
               "step_us_median": round(float(np.median(r["step_us"])), 2), "step_us_min": round(float(np.min(r["step_us"])), 2),
               "step_us_max": round(float(np.max(r["step_us"])), 2),
               "pair_half_us_median": round(float(np.median(r["pair_half_us"])), 2), "pair_half_us_min": round(float(np.min(r["pair_half_us"])), 2),
               "pair_half_us_max": round(float(np.max(r["pair_half_us"])), 2)}
        if flags & capi.PAIR_SHAPES:
            out["info"] = t.read_pair_shapes()[1]
        if "contacts on" in name:
            out["contacts"] = t.read_pair_contacts()[1]
        if name.endswith("manifolds on"):
            out["manifolds"] = t.read_pair_manifolds()[1]
        print(json.dumps(out), flush=True)
    for t, _ in ctxs.values():
        t.close()
