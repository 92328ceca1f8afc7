#!/usr/bin/env python3
"""Host time of N eager scTickRun calls with no sync between them, per library build, builds side by side in one process, order
alternated from round to round; and carry_stats() after the bursts.  --narrow: every run also carries PAIR_SHAPES with all six stages
of the narrow phase on (list, contacts, manifolds, islands, persistence, sleep).
usage: host_cost.py [--workload config3|tiny] [--narrow] libA.so libB.so ..."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sc_gameengine_amd import capi, synth_world as sw          # noqa: E402
from sc_gameengine_amd.tick import WorldTick, camera_view_proj  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="+")
ap.add_argument("--workload", default="config3")
ap.add_argument("--calls", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--narrow", action="store_true")
args = ap.parse_args()

w = sw.config("config3") if args.workload == "config3" else sw.generate(4, 4, 15)
vp = camera_view_proj(w.camera)
flags = capi.FULL | capi.PRODUCE_NEXT | (capi.PAIR_SHAPES if args.narrow else 0)
ctxs = {}
for path in args.libs:
    capi._LIB = None
    capi.LIB_PATH = os.path.abspath(path)
    t = WorldTick.from_world(w, broadphase=True)
    t.set_view_proj(vp)
    t.set_frame_producer(1, 0.01)
    t.nudge_roots_x(0.01)
    if args.narrow:
        t.set_pair_shapes(1 << 12); t.set_pair_contacts(True); t.set_pair_manifolds(True)
        t.pair_islands(True); t.pair_persistence(True); t.pair_sleep(True)
    for _ in range(30):
        t.run(flags)
    t.sync()
    ctxs[os.path.basename(path)] = t
res = {p: [] for p in ctxs}
names = list(ctxs)
for rnd in range(args.rounds):
    order = names[rnd % len(names):] + names[:rnd % len(names)]
    for name in order:
        t = ctxs[name]
        run, ctx = t.lib.scTickRun, t.ctx
        for _ in range(50):
            run(ctx, flags)
        t.sync()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            run(ctx, flags)
        t1 = time.perf_counter()
        t.sync()
        res[name].append((t1 - t0) / args.calls * 1e6)
for name, t in ctxs.items():
    print(json.dumps({"lib": name, "workload": args.workload, "narrow": args.narrow, "calls": args.calls, "host_us_per_call_median": round(float(np.median(res[name])), 3),
                      "host_us_per_call_min": round(float(np.min(res[name])), 3), "rounds": [round(x, 3) for x in res[name]],
                      "carry_stats": t.carry_stats(), "visible": int(t.counts().visible)}), flush=True)
for t in ctxs.values():
    t.close()
