#!/usr/bin/env python3
"""What SC_TICK_TRIGGERS costs: one leg of the comparison per process.

    SC_TICK_LIB=<libsc_tick.so of the build under test> python tools/trigger_cost.py --mode none|overlaps|triggers [--exact] [--ticks 200]

The config-5 world with a collider on every entity (as tools/overlap_cost.py) and 4 096 volumes of about one sector -- boxes, spheres and
capsules by index modulo 3, yawed.  --mode triggers: the volumes ride on vehicles (movers), SC_TICK_TRIGGERS.  --mode overlaps: equal
volumes in world space where those vehicles are when the leg starts, SC_TICK_OVERLAPS with as many id slots -- what the flagged steady tick is held against:
the difference is what resolve, diff and remember add to the existing kernel.  --mode none is the leg a build of the parent commit can
run: no set, no flag.  Every tick is FULL | PRODUCE_NEXT with the movers as the frame producer.
--resync: every tick runs behind scTickSetTile with another rank, so every flagged tick is a resync tick -- every volume enters its whole
row and reserves event slots -- and, with or without the flag, a learn tick: the two legs differ by the resync tick's own cost.
Prints one JSON line: the wall time of a tick with and without the flag (bursts ending in a synchronise) and the report of a last flagged
tick.  Under rocprofv3 --kernel-trace --stats the kernel table gives k_trigger_volumes<false> / <true> (and k_overlap_queries) in
microseconds per launch: steady launches without --resync, resync launches with it."""
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
ap.add_argument("--mode", default="triggers", choices=["none", "overlaps", "triggers"])
ap.add_argument("--exact", action="store_true")
ap.add_argument("--ticks", type=int, default=200)
ap.add_argument("--volumes", type=int, default=4096)
ap.add_argument("--max-members", type=int, default=256)
ap.add_argument("--resync", action="store_true", help="every tick behind scTickSetTile with another rank: every volume resyncs on every flagged tick")
ap.add_argument("--small", action="store_true", help="a small world: a rehearsal of the script, not a measurement")
args = ap.parse_args()

F = np.float32
w = sw.generate(8, 8, 15) if args.small else sw.generate_config5(128, 256)
he = ((w.bmax - w.bmin) * F(0.5)).astype(F)
typ = (capi.COLLIDER_BOX + np.arange(w.n) % 3).astype(np.uint8)
radius = np.maximum(he[:, 0], he[:, 2]).astype(F)
hh = np.maximum(he[:, 1] - radius, 0).astype(F)
rng = np.random.default_rng(3101)
k = args.volumes
kind = getattr(w, "mover_kind", None)
vehicles = np.flatnonzero((w.parent < 0) & (kind != 0)) if kind is not None and (kind != 0).any() else np.flatnonzero(w.parent < 0)
anchor = rng.choice(vehicles, k).astype(np.uint32)
yaw = rng.uniform(0, 2 * np.pi, k)
m = np.zeros((k, 4, 4))
m[:, 0, 0], m[:, 0, 2], m[:, 2, 0], m[:, 2, 2] = np.cos(yaw), np.sin(yaw), -np.sin(yaw), np.cos(yaw)
m[:, 1, 1] = m[:, 3, 3] = 1.0
# a volume's local matrix undoes its carrier's scale (M = T R S * S^-1 Y = T R Y), so that the resolved volume has the size of the world-space one
local = m.copy()
local[:, :3, :3] /= w.scale[anchor].astype(np.float64)[:, :, None]
local16 = np.ascontiguousarray(local.transpose(0, 2, 1).reshape(k, 16), F)
m[:, :3, 3] = w.pos[anchor].astype(np.float64)
world16 = np.ascontiguousarray(m.transpose(0, 2, 1).reshape(k, 16), F)
vtyp = (capi.COLLIDER_BOX + np.arange(k) % 3).astype(np.uint8)
vhe, vrad, vhh = np.tile(F([22.0, 6.0, 22.0]), (k, 1)), np.full(k, 24.0, F), np.full(k, 8.0, F)      # about a 64 m sector across once yawed
mask = np.full(k, 0xFFFFFFFF, np.uint32)
shapes = capi.OVERLAP_SHAPES_EXACT if args.exact else capi.OVERLAP_SHAPES_AABB

t = WorldTick.from_world(w, broadphase=True)
t.upload_colliders(0, typ, he, radius, hh)
t.set_view_proj(camera_view_proj(w.camera))
t.set_frame_producer(2, 1.0 / 60.0)
t.advance_movers(1.0 / 60.0)
PLAIN = capi.FULL | capi.PRODUCE_NEXT
legs = [("without", PLAIN)]
if args.mode == "overlaps":
    # the vehicles drive on while a leg runs: the world-space volumes stand where the vehicles ARE after as many ticks as the other leg's
    # first burst, so that both legs answer with member rows of about one size
    for _ in range(30 + args.ticks):
        t.run(PLAIN)
    world16[:, 12:15] = t.positions()[anchor]
    t.overlap_queries(vtyp, world16, vhe, vrad, vhh, mask, max_hits=args.max_members, shapes=shapes)
    legs = [("with_flag", PLAIN | capi.OVERLAPS), ("without", PLAIN), ("with_flag_again", PLAIN | capi.OVERLAPS)]
if args.mode == "triggers":
    t.trigger_volumes(anchor, vtyp, local16, vhe, vrad, vhh, mask, max_members=args.max_members, max_events=1 << 20, shapes=shapes)
    legs = [("with_flag", PLAIN | capi.TRIGGERS), ("without", PLAIN), ("with_flag_again", PLAIN | capi.TRIGGERS)]
wall = {}


def step(flags, i):
    if args.resync:                                             # another rank: ids are renamed, every volume forgets its row (and the bins learn)
        t.set_tile(1 + i % 2, 0)
    t.run(flags)


for name, flags in legs:
    for i in range(30):
        step(flags, i)
    t.sync()
    t0 = time.perf_counter()
    for i in range(args.ticks):
        step(flags, i)
    t.sync()
    wall[name] = round((time.perf_counter() - t0) / args.ticks * 1e6, 2)
out = {"lib": os.path.basename(os.path.dirname(capi.LIB_PATH)) + "/" + os.path.basename(capi.LIB_PATH), "mode": args.mode, "exact": bool(args.exact),
       "entities": int(w.n), "volumes": k, "max_members": args.max_members, "resync": bool(args.resync), "tick_us": wall}
if args.mode == "overlaps":
    step(PLAIN | capi.OVERLAPS, 0)
    out["info"] = t.overlap_info()
if args.mode == "triggers":
    step(PLAIN | capi.TRIGGERS, 0)
    out["info"] = t.trigger_info()
print(json.dumps(out), flush=True)
t.close()
