#!/usr/bin/env python3
"""Cost of the ray batch inside the tick: config-5 world, 1M entities, one front ray per vehicle
as the traffic AI casts it (sc_traffic_ai.cpp:303-319), tick time with and without SC_TICK_RAYS; then, on the same world in the
same process, 4096 capsule sweeps (radius 0.4 m, half height 0.5 m, 20 m along the same headings) with SC_TICK_SWEEPS; then 4096
entity-anchored rays of 20 m riding on the vehicles (the same probe given in each vehicle's local frame) with SC_TICK_ANCHORED_RAYS:
tick_us and tick_with_4096_rays_us of this same process are the yardsticks, anchored_minus_plain_us the difference; then the pair-events
leg: the same tick without queries, SC_TICK_PAIR_EVENTS off and on (room for 2^17 tracked pairs and 2^14 events), and what one frame
reads back through scTickReadPairEvents against scTickReadPairs -- bytes, and the host time of the one call."""
import os, sys, time, json
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sc_gameengine_amd import capi, synth_world as sw
from sc_gameengine_amd.tick import WorldTick

w = sw.generate_config5(128, 256)
t = WorldTick.from_world(w, broadphase=True)
t.set_camera(w.camera)
veh = np.flatnonzero(w.mover_kind == 1)
yaw = w.rot[veh, 1]
fwd = np.stack([np.sin(yaw), np.zeros_like(yaw), np.cos(yaw)], axis=1).astype(np.float32)
o = (w.pos[veh] + fwd * np.float32(1.7) + np.float32([0, 0.6, 0])).astype(np.float32)
out = {"entities": int(w.n), "rays": int(len(veh))}
t.set_frame_producer(2, 1.0 / 60.0)
for name, rays in (("tick_us", 0), ("tick_with_rays_us", len(veh)), ("tick_with_4096_rays_us", 4096)):
    t.set_ray_queries(o[:rays], fwd[:rays], np.full(rays, 20.0, np.float32), np.full(rays, 1, np.uint32))
    fl = capi.FULL | capi.PRODUCE_NEXT | (capi.RAYS if rays else 0)
    for _ in range(20): t.run(fl)
    t.sync()
    n = 200
    t0 = time.perf_counter()
    for _ in range(n): t.run(fl)
    t.sync()
    out[name] = round((time.perf_counter() - t0) / n * 1e6, 2)
    if rays:
        h = t.ray_hits(); out[name.replace("_us", "_hits")] = int(h["hit"].sum())
# the sweeps leg: a pedestrian-sized capsule from where the first 4096 front rays start, 20 m ahead
k = 4096
t.set_ray_queries(o[:0], fwd[:0], np.zeros(0, np.float32), np.zeros(0, np.uint32))
t.set_sweep_queries(o[:k], o[:k] + fwd[:k] * np.float32(20.0), np.full(k, 0.4, np.float32), np.full(k, 0.5, np.float32), np.full(k, 1, np.uint32))
fl = capi.FULL | capi.PRODUCE_NEXT | capi.SWEEPS
for _ in range(20): t.run(fl)
t.sync()
n = 200
t0 = time.perf_counter()
for _ in range(n): t.run(fl)
t.sync()
out["tick_with_4096_sweeps_us"] = round((time.perf_counter() - t0) / n * 1e6, 2)
out["tick_with_4096_sweeps_hits"] = int(t.sweep_hits()["hit"].sum())
# the anchored leg: the front ray of the first 4096 vehicles in their own frames -- 1.7 m ahead, 0.6 m up in world metres, along local +z
t.set_sweep_queries(o[:0], o[:0], np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.uint32))
local = (np.float32([0.0, 0.6, 1.7]) / w.scale[veh[:k]]).astype(np.float32)
t.set_anchored_rays(veh[:k].astype(np.uint32), local, np.tile(np.float32([0, 0, 1]), (k, 1)), np.full(k, 20.0, np.float32), np.full(k, 1, np.uint32))
fl = capi.FULL | capi.PRODUCE_NEXT | capi.ANCHORED_RAYS
for _ in range(20): t.run(fl)
t.sync()
learn = t.learn_ticks()
t0 = time.perf_counter()
for _ in range(n): t.run(fl)
t.sync()
out["tick_with_4096_anchored_rays_us"] = round((time.perf_counter() - t0) / n * 1e6, 2)
out["tick_with_4096_anchored_rays_hits"] = int(t.anchored_ray_hits()["hit"].sum())
out["anchored_learn_ticks_while_timed"] = t.learn_ticks() - learn
out["anchored_minus_plain_us"] = round(out["tick_with_4096_anchored_rays_us"] - out["tick_with_4096_rays_us"], 2)
# the pair-events leg: no queries, the flag off and on in the same process; then one frame's read-back either way
fl = capi.FULL | capi.PRODUCE_NEXT
t.set_pair_events(1 << 17, 1 << 14)
for name, f in (("tick_pair_events_off_us", fl), ("tick_pair_events_on_us", fl | capi.PAIR_EVENTS)):
    for _ in range(20): t.run(f)
    t.sync()
    t0 = time.perf_counter()
    for _ in range(n): t.run(f)
    t.sync()
    out[name] = round((time.perf_counter() - t0) / n * 1e6, 2)
out["pair_events_minus_off_us"] = round(out["tick_pair_events_on_us"] - out["tick_pair_events_off_us"], 2)
t0 = time.perf_counter(); b, e, info = t.pair_events(); out["read_pair_events_call_us"] = round((time.perf_counter() - t0) * 1e6, 1)
t0 = time.perf_counter(); got, total = t.pairs(); out["read_pairs_call_us"] = round((time.perf_counter() - t0) * 1e6, 1)
out["pair_events_info"] = info
out["read_pair_events_bytes"] = 24 + 8 * (len(b) + len(e))
out["read_pairs_bytes"] = 8 * len(got)
print(json.dumps(out))
