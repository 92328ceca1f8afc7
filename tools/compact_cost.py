#!/usr/bin/env python3
"""What the end-of-tick slot of config 3 costs, by the form of its compaction and by how much is visible, in ONE process.

    python tools/compact_cost.py [--rounds 6] [--burst 400] [lib.so[#ENV=v,...] ...]

Without arguments: the built library as SC_TICK_VARIANT=16 (one workgroup per span, compactBody), as SC_TICK_COMPACT_G=5, 10 and 21 (the
wide form with that many spans per workgroup) and as it is (the wide form under compactWideGroup's rule).  Every variant gets a context of
its own on the same world; they are timed in interleaved rounds under two cameras: config 3's own (a few thousand visible) and one whose
frustum holds the whole world (every renderable visible: the list is 4 MB).  Per variant and camera: the slot's duration from the
dispatch's own timestamps, the fused kernel's, the step by wall time of a burst, the launch shape (compact_stats) and the visible count."""
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
ap.add_argument("libs", nargs="*")
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--burst", type=int, default=400)
args = ap.parse_args()
own = capi.LIB_PATH
libs = args.libs or [own + "#SC_TICK_VARIANT=16", own + "#SC_TICK_COMPACT_G=5", own + "#SC_TICK_COMPACT_G=10", own + "#SC_TICK_COMPACT_G=21", own]

w = sw.config("config3")
side = float(max(w.sectors) * sw.SECTOR_SIZE)
whole = {"pos": np.array([w.origin[0] * sw.SECTOR_SIZE + side / 2, 2.0 * side, w.origin[1] * sw.SECTOR_SIZE + side / 2], np.float32),
         "rot": np.array([-np.pi / 2, 0.0, 0.0], np.float32), "fovY": 60.0, "nearZ": 0.1, "farZ": 4.0 * side, "aspect": 16.0 / 9.0}
cameras = {"config3": camera_view_proj(w.camera), "all-visible": camera_view_proj(whole)}
flags = capi.FULL | capi.PRODUCE_NEXT

ctxs = {}
for spec in libs:
    path, _, envs = spec.partition("#")
    for kv in filter(None, envs.split(",")):
        k, _, v = kv.partition("=")
        os.environ[k] = v
    capi._LIB = None
    capi.LIB_PATH = os.path.abspath(path)
    t = WorldTick.from_world(w, broadphase=True)
    for kv in filter(None, envs.split(",")):
        os.environ.pop(kv.partition("=")[0], None)
    t.set_frame_producer(1, 0.01)
    t.nudge_roots_x(0.01)
    ctxs[os.path.basename(path) + ("#" + envs if envs else "")] = t

for cam, vp in cameras.items():
    res = {p: {"step_us": [], "k1_us": [], "eot_us": []} for p in ctxs}
    for t in ctxs.values():
        t.set_view_proj(vp)
        for _ in range(30):
            t.run(flags)
        t.sync()
    for rnd in range(args.rounds):
        for p, t in ctxs.items():
            for _ in range(20):
                t.run(flags)
            t.sync()
            t0 = time.perf_counter()
            for _ in range(args.burst):
                t.run(flags)
            t.sync()
            res[p]["step_us"].append((time.perf_counter() - t0) / args.burst * 1e6)
            t.set_profiling(1)
            for _ in range(40):
                t.run(flags)
            res[p]["k1_us"] += [x * 1e3 for x in t.kernel_times_ms(capi.K_XFORM_CULL)]
            res[p]["eot_us"] += [x * 1e3 for x in t.kernel_times_ms(capi.K_PAIRS)]
            t.set_profiling(0)
    for p, t in ctxs.items():
        r = res[p]
        shape = t.compact_stats() if hasattr(t, "compact_stats") and hasattr(t.lib, "scTickGetCompactStats") else None
        print(json.dumps({"lib": p, "camera": cam, "end_of_tick_us": round(float(np.median(r["eot_us"])), 2), "end_of_tick_us_min": round(float(np.min(r["eot_us"])), 2),
                          "k_xform_cull_us": round(float(np.median(r["k1_us"])), 2), "step_us_median": round(float(np.median(r["step_us"])), 2),
                          "step_us_min": round(float(np.min(r["step_us"])), 2), "compact": shape,
                          "visible": int(t.counts().visible)}), flush=True)
for t in ctxs.values():
    t.close()
