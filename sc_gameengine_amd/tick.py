"""WorldTick -- thin Python host over the C ABI (libsc_tick.so) for tests and bench.py.

It mirrors what the C++ adapter systems do (sc_gameengine_amd/host/sc_tick_systems.cpp): push entity
state, set the frame's viewProj, run the tick, read results.  No CPU fallback, no oracle import.
"""
import ctypes as C

import numpy as np

from . import capi


def _f(a):
    return a.ctypes.data_as(capi.F32P)


def _u(a):
    return a.ctypes.data_as(capi.U32P)


def _c32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# what WorldTick.sweep_hits() returns (== ScTickSweepHit)
SWEEP_HIT_DTYPE = np.dtype([("hit", np.uint32), ("id", np.uint32), ("distance", np.float32), ("position", np.float32, 3),
                            ("normal", np.float32, 3), ("layer", np.uint32), ("travel", np.float32), ("pad", np.uint32)])


# what WorldTick.ray_hits() and anchored_ray_hits() return (== ScTickRayHit)
RAY_HIT_DTYPE = np.dtype([("hit", np.uint32), ("id", np.uint32), ("distance", np.float32), ("position", np.float32, 3),
                          ("normal", np.float32, 3), ("layer", np.uint32), ("pad", np.uint32, 2)])


# ---- host-side camera math (CameraSystem stays on the host, sc_ecs.cpp:213-272) ----------------
def host_mat4_trs(pos, rot, scale):
    p, r, s, o = _c32(pos), _c32(rot), _c32(scale), np.zeros(16, np.float32)
    assert capi.load().scTickHostMat4Trs(_f(p), _f(r), _f(s), _f(o))
    return o


def host_mat4_mul(a, b):
    a, b, o = _c32(a), _c32(b), np.zeros(16, np.float32)
    assert capi.load().scTickHostMat4Mul(_f(a), _f(b), _f(o))
    return o


def host_mat4_inverse(a):
    a, o = _c32(a), np.zeros(16, np.float32)
    assert capi.load().scTickHostMat4Inverse(_f(a), _f(o))
    return o


def host_mat4_perspective(fov, aspect, zn, zf, flip):
    o = np.zeros(16, np.float32)
    assert capi.load().scTickHostMat4PerspectiveRhZo(float(fov), float(aspect), float(zn), float(zf), int(flip), _f(o))
    return o


def host_camera_view_proj(camera_world, fov_y_deg=60.0, aspect=16.0 / 9.0, near=0.1, far=1000.0):
    m, o = _c32(camera_world), np.zeros(16, np.float32)
    assert capi.load().scTickHostCameraViewProj(_f(m), float(fov_y_deg), float(aspect), float(near), float(far), _f(o))
    return o


def camera_view_proj(cam):
    """viewProj of a root camera entity described by a SynthWorld camera dict."""
    world = host_mat4_trs(cam["pos"], cam["rot"], (1.0, 1.0, 1.0))
    return host_camera_view_proj(world, cam["fovY"], cam["aspect"], cam["nearZ"], cam["farZ"])


class WorldTick:
    def __init__(self, capacity, device=0, tile_origin=(0, 0), tile_sectors=(0, 0), sector_size=64.0,
                 max_pairs=0, max_draws=0):
        self.lib = capi.load()
        d = capi.ContextDesc()
        d.device_ordinal = device
        d.capacity = capacity
        d.tile_origin_x, d.tile_origin_z = tile_origin
        d.tile_sectors_x, d.tile_sectors_z = tile_sectors
        d.sector_size = sector_size
        d.max_pairs = max_pairs
        d.max_draws_budget = max_draws
        self.ctx = self.lib.scTickCreateContext(C.byref(d))
        if not self.ctx:
            raise capi.ScTickError("scTickCreateContext failed: " + (self.lib.scTickGetLastError(None) or b"").decode())
        self.capacity = capacity
        self.max_pairs = max_pairs if max_pairs else capacity * 4
        self.n = 0

    # ---- plumbing ----
    def _ok(self, r, what):
        if not r:
            raise capi.ScTickError(f"{what}: " + (self.lib.scTickGetLastError(self.ctx) or b"").decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.scTickDestroyContext(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- state ----
    @classmethod
    def from_world(cls, w, device=0, broadphase=True, max_pairs=0, max_draws=0, capacity=None):
        t = cls(capacity or max(w.n, 1), device=device,
                tile_origin=w.origin if broadphase else (0, 0),
                tile_sectors=w.sectors if broadphase else (0, 0),
                max_pairs=max_pairs, max_draws=max_draws)
        t.upload_world(w)
        return t

    def upload_world(self, w):
        self.set_count(w.n)
        if w.n == 0:
            return
        self.upload_locals(0, w.pos, w.rot, w.scale)
        self.upload_bounds(0, w.bmin, w.bmax, w.has_bounds)
        self.upload_render_meshes(0, w.has_mesh, w.mesh, w.material)
        self.upload_layers(0, w.group, w.mask)
        self.set_topology(w.parent)
        if getattr(w, "mover_kind", None) is not None:
            self.upload_movers(0, w.mover_kind, w.mover_vel, w.mover_lo, w.mover_hi)
        if getattr(w, "is_agent", None) is not None:
            self.set_lane_graph(w.lane_graph)
            self.upload_traffic_agents(0, w.is_agent, w.agent_lane, w.agent_s, w.agent_speed, w.agent_mode)

    def set_count(self, n):
        self._ok(self.lib.scTickSetEntityCount(self.ctx, n), "scTickSetEntityCount")
        self.n = n

    def upload_locals(self, first, pos, rot, scale):
        p, r, s = _c32(pos), _c32(rot), _c32(scale)
        rep = np.zeros(len(p), np.uint8)
        self._ok(self.lib.scTickUploadLocals(self.ctx, first, len(p), _f(p), _f(r), _f(s), rep.ctypes.data_as(capi.U8P)),
                 "scTickUploadLocals")
        return rep

    def upload_positions(self, first, pos):
        p = _c32(pos)
        self._ok(self.lib.scTickUploadPositions(self.ctx, first, len(p), _f(p)), "scTickUploadPositions")

    def upload_bounds(self, first, bmin, bmax, has=None):
        a, b = _c32(bmin), _c32(bmax)
        h = None if has is None else np.ascontiguousarray(has, np.uint8)
        self._ok(self.lib.scTickUploadBounds(self.ctx, first, len(a), _f(a), _f(b),
                                             None if h is None else h.ctypes.data_as(capi.U8P)), "scTickUploadBounds")

    def upload_colliders(self, first, type, half_extents=None, radius=None, half_height=None):
        """Collider per entity from `first` on (capi.COLLIDER_*; type None = BOX for len(half_extents) entities): the broadphase
        proxy is formed from it instead of the Bounds box.  None for a value array = the reference's default 0.5."""
        t = None if type is None else np.ascontiguousarray(type, np.uint8).reshape(-1)
        he = None if half_extents is None else _c32(half_extents).reshape(-1, 3)
        r = None if radius is None else _c32(radius).reshape(-1)
        hh = None if half_height is None else _c32(half_height).reshape(-1)
        given = [len(a) for a in (t, he, r, hh) if a is not None]
        assert given and min(given) == max(given), "upload_colliders: arrays of one length, at least one of them"
        self._ok(self.lib.scTickUploadColliders(self.ctx, first, given[0], None if t is None else t.ctypes.data_as(capi.U8P),
                                                None if he is None else _f(he), None if r is None else _f(r),
                                                None if hh is None else _f(hh)), "scTickUploadColliders")

    def colliders(self):
        """(type, half_extents[n,3], radius, half_height) of every entity as stored (BOUNDS and 0.5s where none was uploaded)"""
        t, he = np.zeros(self.n, np.uint8), np.zeros((self.n, 3), np.float32)
        r, hh = np.zeros(self.n, np.float32), np.zeros(self.n, np.float32)
        self._ok(self.lib.scTickReadColliders(self.ctx, 0, self.n, t.ctypes.data_as(capi.U8P), _f(he), _f(r), _f(hh)), "scTickReadColliders")
        return t, he, r, hh

    def upload_render_meshes(self, first, has, mesh, material):
        h = np.ascontiguousarray(has, np.uint8)
        m, t = np.ascontiguousarray(mesh, np.uint32), np.ascontiguousarray(material, np.uint32)
        self._ok(self.lib.scTickUploadRenderMeshes(self.ctx, first, len(h), h.ctypes.data_as(capi.U8P), _u(m), _u(t)),
                 "scTickUploadRenderMeshes")

    def upload_layers(self, first, group, mask):
        g, m = np.ascontiguousarray(group, np.uint32), np.ascontiguousarray(mask, np.uint32)
        self._ok(self.lib.scTickUploadLayers(self.ctx, first, len(g), _u(g), _u(m)), "scTickUploadLayers")

    def set_topology(self, parent):
        p = np.ascontiguousarray(parent, np.int32)
        self._ok(self.lib.scTickSetTopology(self.ctx, p.ctypes.data_as(capi.I32P), len(p)), "scTickSetTopology")

    def mark_dirty(self, first, count):
        self._ok(self.lib.scTickMarkDirty(self.ctx, first, count), "scTickMarkDirty")

    def mark_dirty_indices(self, idx):
        i = np.ascontiguousarray(idx, np.uint32)
        self._ok(self.lib.scTickMarkDirtyIndices(self.ctx, _u(i), len(i)), "scTickMarkDirtyIndices")

    def upload_world_matrices(self, first, m16):
        m = _c32(m16)
        self._ok(self.lib.scTickUploadWorldMatrices(self.ctx, first, len(m), _f(m)), "scTickUploadWorldMatrices")

    # ---- frame inputs ----
    def set_view_proj(self, vp):
        v = _c32(vp)
        self._ok(self.lib.scTickSetViewProj(self.ctx, _f(v)), "scTickSetViewProj")

    def set_frustum_planes(self, planes, valid=True):
        p = _c32(planes).reshape(24)
        self._ok(self.lib.scTickSetFrustumPlanes(self.ctx, _f(p), 1 if valid else 0), "scTickSetFrustumPlanes")

    def frustum_planes(self):
        p, v = np.zeros(24, np.float32), C.c_int()
        self._ok(self.lib.scTickGetFrustumPlanes(self.ctx, _f(p), C.byref(v)), "scTickGetFrustumPlanes")
        return p.reshape(6, 4), v.value

    def set_camera(self, cam):
        vp = camera_view_proj(cam)
        self.set_view_proj(vp)
        return vp

    def set_draw_budget(self, max_draws):
        """WorldStreamingBudgets::maxDrawsBudget for the next SC_TICK_DRAWS (0 = unlimited)"""
        self._ok(self.lib.scTickSetDrawBudget(self.ctx, int(max_draws)), "scTickSetDrawBudget")

    def set_freeze_culling(self, on):
        self._ok(self.lib.scTickSetFreezeCulling(self.ctx, 1 if on else 0), "scTickSetFreezeCulling")

    # ---- tick ----
    def run(self, flags=capi.XFORM | capi.CULL):
        self._ok(self.lib.scTickRun(self.ctx, flags), "scTickRun")

    def sync(self):
        self._ok(self.lib.scTickSynchronize(self.ctx), "scTickSynchronize")

    def nudge_roots_x(self, dx):
        self._ok(self.lib.scTickNudgeRootsX(self.ctx, float(dx)), "scTickNudgeRootsX")

    # ---- ray queries over this tick's boxes ----
    def set_ray_queries(self, origin, direction, max_dist, mask):
        o, dd = _c32(origin).reshape(-1, 3), _c32(direction).reshape(-1, 3)
        md, mk = _c32(max_dist).reshape(-1), np.ascontiguousarray(mask, np.uint32).reshape(-1)
        self._ok(self.lib.scTickSetRayQueries(self.ctx, len(o), _f(o), _f(dd), _f(md), _u(mk)), "scTickSetRayQueries")

    def ray_hits(self):
        """Structured array (hit, id, distance, position[3], normal[3], layer) of the last run's ray batch."""
        n = C.c_uint32()
        self._ok(self.lib.scTickReadRayHits(self.ctx, None, 0, C.byref(n)), "scTickReadRayHits")
        buf = (capi.RayHit * max(n.value, 1))()
        if n.value:
            self._ok(self.lib.scTickReadRayHits(self.ctx, buf, n.value, C.byref(n)), "scTickReadRayHits")
        return np.frombuffer(buf, dtype=RAY_HIT_DTYPE, count=n.value).copy()

    # ---- exact collider shapes for the ray queries and the anchored rays (scTickSetRayShapes) ----
    def set_ray_shapes(self, mode):
        """capi.RAY_SHAPES_AABB (default) / capi.RAY_SHAPES_EXACT: in EXACT mode the runs with capi.RAYS and capi.ANCHORED_RAYS answer a
        candidate whose proxy comes from a typed collider (upload_colliders: box, sphere, capsule) by the shape itself, taken through the
        entity's world matrix of the tick; Bounds proxies and a neighbour tile's records keep their AABB answer.  Drops captured graphs,
        costs no learn tick (scTickSetRayShapes)."""
        self._ok(self.lib.scTickSetRayShapes(self.ctx, int(mode)), "scTickSetRayShapes")

    def ray_shapes(self):
        mode = C.c_uint32()
        self._ok(self.lib.scTickGetRayShapes(self.ctx, C.byref(mode)), "scTickGetRayShapes")
        return int(mode.value)

    # ---- exact collider shapes for the capsule sweeps (scTickSetSweepShapes) ----
    def set_sweep_shapes(self, mode):
        """capi.SWEEP_SHAPES_EXACT: the runs with capi.SWEEPS answer a candidate whose proxy comes from a typed collider (box, sphere,
        capsule) by advancing the capsule itself towards the shape itself, through the entity's world matrix of that tick; the grown-AABB
        test stays the pre-filter.  capi.SWEEP_SHAPES_AABB (the default): the capsule's box against the world AABBs.  A property of the
        context; costs no learn tick (scTickSetSweepShapes)."""
        self._ok(self.lib.scTickSetSweepShapes(self.ctx, int(mode)), "scTickSetSweepShapes")

    def sweep_shapes(self):
        mode = C.c_uint32()
        self._ok(self.lib.scTickGetSweepShapes(self.ctx, C.byref(mode)), "scTickGetSweepShapes")
        return int(mode.value)

    def sweep_shape_info(self):
        """What the last run's sweeps did with their candidates in capi.SWEEP_SHAPES_EXACT mode (scTickGetSweepShapeInfo): a dict with
        refined, kept_as_boxes, exhausted."""
        info = capi.SweepShapeInfo()
        self._ok(self.lib.scTickGetSweepShapeInfo(self.ctx, C.byref(info)), "scTickGetSweepShapeInfo")
        return {k: int(getattr(info, k)) for k, _ in capi.SweepShapeInfo._fields_ if k != "pad"}

    # ---- entity-anchored rays: given in an entity's local frame, resolved on the device every tick ----
    def set_anchored_rays(self, anchor, local_origin, local_dir, max_dist, mask, skip_self=None):
        """Rays in the local frame of the entities `anchor` (dense indices; capi.ANCHOR_NONE: a world-space ray), answered by every run
        with capi.ANCHORED_RAYS against that tick's matrices and boxes (scTickSetAnchoredRays).  skip_self: per ray, whether the anchor's
        own box never answers (None: all).  A call with as many rays as the current set costs no learn tick and no graph capture."""
        an = np.ascontiguousarray(anchor, np.uint32).reshape(-1)
        o, dd = _c32(local_origin).reshape(-1, 3), _c32(local_dir).reshape(-1, 3)
        md, mk = _c32(max_dist).reshape(-1), np.ascontiguousarray(mask, np.uint32).reshape(-1)
        sk = None if skip_self is None else np.ascontiguousarray(skip_self, np.uint8).reshape(-1)
        assert len(o) == len(an) and len(dd) == len(an) and len(md) == len(an) and len(mk) == len(an) and (sk is None or len(sk) == len(an))
        self._ok(self.lib.scTickSetAnchoredRays(self.ctx, len(an), _u(an), _f(o), _f(dd), _f(md), _u(mk),
                                                None if sk is None else sk.ctypes.data_as(capi.U8P)), "scTickSetAnchoredRays")
        self._anchored_rays = len(an)

    def anchored_ray_hits(self):
        """Structured array like ray_hits() of the last run's anchored rays."""
        n = C.c_uint32()
        self._ok(self.lib.scTickReadAnchoredRayHits(self.ctx, None, 0, C.byref(n)), "scTickReadAnchoredRayHits")
        buf = (capi.RayHit * max(n.value, 1))()
        if n.value:
            self._ok(self.lib.scTickReadAnchoredRayHits(self.ctx, buf, n.value, C.byref(n)), "scTickReadAnchoredRayHits")
        return np.frombuffer(buf, dtype=RAY_HIT_DTYPE, count=n.value).copy()

    def anchored_ray_anchors(self):
        """The anchors as they stand now: renamed by remove_entities where their entity moved, capi.ANCHOR_DEAD where it was removed."""
        k = getattr(self, "_anchored_rays", 0)
        out = np.zeros(max(k, 1), np.uint32)
        if k:
            self._ok(self.lib.scTickReadAnchoredRays(self.ctx, 0, k, _u(out)), "scTickReadAnchoredRays")
        return out[:k].copy()

    # ---- capsule sweeps over this tick's boxes ----
    def set_sweep_queries(self, start, end, radius, half_height, mask, skip_id=None):
        """Upright-capsule sweeps from start to end (scTickSetSweepQueries); skip_id: per sweep, a box id that never answers (None: none)."""
        a, b = _c32(start).reshape(-1, 3), _c32(end).reshape(-1, 3)
        r, hh = _c32(radius).reshape(-1), _c32(half_height).reshape(-1)
        mk = np.ascontiguousarray(mask, np.uint32).reshape(-1)
        sk = None if skip_id is None else np.ascontiguousarray(skip_id, np.uint32).reshape(-1)
        assert len(b) == len(a) and len(r) == len(a) and len(hh) == len(a) and len(mk) == len(a) and (sk is None or len(sk) == len(a))
        self._ok(self.lib.scTickSetSweepQueries(self.ctx, len(a), _f(a), _f(b), _f(r), _f(hh), _u(mk), None if sk is None else _u(sk)),
                 "scTickSetSweepQueries")

    def sweep_hits(self):
        """Structured array (hit, id, distance = hit fraction, position[3] = the capsule's centre, normal[3], layer, travel = metres, pad)
        of the last run's sweep batch."""
        n = C.c_uint32()
        self._ok(self.lib.scTickReadSweepHits(self.ctx, None, 0, C.byref(n)), "scTickReadSweepHits")
        buf = (capi.SweepHit * max(n.value, 1))()
        if n.value:
            self._ok(self.lib.scTickReadSweepHits(self.ctx, buf, n.value, C.byref(n)), "scTickReadSweepHits")
        return np.frombuffer(buf, dtype=SWEEP_HIT_DTYPE, count=n.value).copy()

    # ---- overlap queries: collider volumes answered from this tick's boxes ----
    def overlap_queries(self, type, matrices, half_extents, radius, half_height, mask, skip_id=None, max_hits=64,
                        shapes=capi.OVERLAP_SHAPES_AABB):
        """Volumes -- a collider type (capi.COLLIDER_BOX / _SPHERE / _CAPSULE), its values and a world matrix (column-major [k, 16]) each --
        answered by every run with capi.OVERLAPS: which boxes of that tick meet the volume's box (capi.OVERLAP_SHAPES_AABB), or which
        collider shapes meet the volume itself (capi.OVERLAP_SHAPES_EXACT).  skip_id: per volume, a box id that never answers (None:
        none); max_hits: id slots per volume.  A call with the same count, max_hits and mode as the current set costs no learn tick
        and no graph capture (scTickSetOverlapQueries)."""
        t = np.ascontiguousarray(type, np.uint8).reshape(-1)
        k = len(t)
        m, he = _c32(matrices).reshape(-1, 16), _c32(half_extents).reshape(-1, 3)
        r, hh = _c32(radius).reshape(-1), _c32(half_height).reshape(-1)
        mk = np.ascontiguousarray(mask, np.uint32).reshape(-1)
        sk = None if skip_id is None else np.ascontiguousarray(skip_id, np.uint32).reshape(-1)
        assert len(m) == k and len(he) == k and len(r) == k and len(hh) == k and len(mk) == k and (sk is None or len(sk) == k)
        self._ok(self.lib.scTickSetOverlapQueries(self.ctx, k, t.ctypes.data_as(capi.U8P), _f(m), _f(he), _f(r), _f(hh), _u(mk),
                                                  None if sk is None else _u(sk), int(max_hits), int(shapes)), "scTickSetOverlapQueries")

    def overlap_info(self):
        """What the last run's overlap queries found (scTickReadOverlapHits): a dict with queries, max_hits, hits, truncated_queries,
        refined, kept_as_boxes, shapes."""
        info = capi.OverlapInfo()
        self._ok(self.lib.scTickReadOverlapHits(self.ctx, None, None, 0, C.byref(info)), "scTickReadOverlapHits")
        return {k: int(getattr(info, k)) for k, _ in capi.OverlapInfo._fields_ if k != "pad"}

    def overlap_hits(self):
        """(counts [k], ids [k, max_hits]) of the last run's overlap queries: counts[q] is the true number of hits of volume q, the first
        min(counts[q], max_hits) slots of ids[q] hold distinct ids (rank << 24 | dense index) of them, in no particular order."""
        info = self.overlap_info()
        k, mh = info["queries"], info["max_hits"]
        counts, ids = np.zeros(max(k, 1), np.uint32), np.zeros((max(k, 1), max(mh, 1)), np.uint32)
        if k:
            self._ok(self.lib.scTickReadOverlapHits(self.ctx, _u(counts), _u(ids), k, None), "scTickReadOverlapHits")
        return counts[:k].copy(), ids[:k, :mh].copy()

    # ---- trigger volumes: anchored overlap volumes with enter / exit events ----
    def trigger_volumes(self, anchor, type, local_matrices, half_extents, radius, half_height, mask, skip_self=None, max_members=64,
                        max_events=1024, shapes=capi.OVERLAP_SHAPES_AABB):
        """Volumes like overlap_queries' in the local frame of the entities `anchor` (dense indices; capi.ANCHOR_NONE: world space),
        answered by every run with capi.TRIGGERS against that tick's matrices and boxes, and reported as who entered and who left since
        the last run with the flag (scTickSetTriggerVolumes).  skip_self: per volume, whether the anchor itself never answers (None: all).
        A call with the same count, max_members, max_events and mode as the current set keeps what is remembered and costs no learn
        tick and no graph capture."""
        an = np.ascontiguousarray(anchor, np.uint32).reshape(-1)
        k = len(an)
        t = np.ascontiguousarray(type, np.uint8).reshape(-1)
        m, he = _c32(local_matrices).reshape(-1, 16), _c32(half_extents).reshape(-1, 3)
        r, hh = _c32(radius).reshape(-1), _c32(half_height).reshape(-1)
        mk = np.ascontiguousarray(mask, np.uint32).reshape(-1)
        sk = None if skip_self is None else np.ascontiguousarray(skip_self, np.uint8).reshape(-1)
        assert len(t) == k and len(m) == k and len(he) == k and len(r) == k and len(hh) == k and len(mk) == k and (sk is None or len(sk) == k)
        self._ok(self.lib.scTickSetTriggerVolumes(self.ctx, k, _u(an), t.ctypes.data_as(capi.U8P), _f(m), _f(he), _f(r), _f(hh), _u(mk),
                                                  None if sk is None else sk.ctypes.data_as(capi.U8P), int(max_members), int(max_events),
                                                  int(shapes)), "scTickSetTriggerVolumes")
        self._trigger_volumes, self._trigger_events = k, int(max_events)

    def trigger_info(self):
        """What the last run's trigger volumes found (scTickReadTriggerMembers): a dict with volumes, max_members, members, entered,
        exited, resync_volumes, overflow_volumes, events_truncated."""
        info = capi.TriggerInfo()
        self._ok(self.lib.scTickReadTriggerMembers(self.ctx, None, None, 0, C.byref(info)), "scTickReadTriggerMembers")
        return {k: int(getattr(info, k)) for k, _ in capi.TriggerInfo._fields_}

    def trigger_members(self):
        """(counts [k], ids [k, max_members]) of the last run with capi.TRIGGERS: counts[v] is the true number of members of volume v, the
        first min(counts[v], max_members) slots of ids[v] hold distinct ids (rank << 24 | dense index) of them, in no particular order."""
        info = self.trigger_info()
        k, mm = info["volumes"], info["max_members"]
        counts, ids = np.zeros(max(k, 1), np.uint32), np.zeros((max(k, 1), max(mm, 1)), np.uint32)
        if k:
            self._ok(self.lib.scTickReadTriggerMembers(self.ctx, _u(counts), _u(ids), k, None), "scTickReadTriggerMembers")
        return counts[:k].copy(), ids[:k, :mm].copy()

    def trigger_events(self):
        """(entered [e, 2], exited [x, 2]) of the last run with capi.TRIGGERS as (volume, id) pairs in no particular order; when
        trigger_info()["events_truncated"] is set each list holds max_events of the true entries."""
        cap = max(getattr(self, "_trigger_events", 0), 1)
        ent, exi = np.zeros((cap, 2), np.uint32), np.zeros((cap, 2), np.uint32)
        info = capi.TriggerInfo()
        self._ok(self.lib.scTickReadTriggerEvents(self.ctx, _u(ent), cap, _u(exi), cap, C.byref(info)), "scTickReadTriggerEvents")
        room = getattr(self, "_trigger_events", 0)
        return ent[:min(info.entered, room)].copy(), exi[:min(info.exited, room)].copy()

    def trigger_matrices(self):
        """[k, 16] column-major: the volumes' world matrices as the last run with capi.TRIGGERS resolved them (NaN: no members by the
        resolve -- a dead anchor or a non-finite entry)."""
        k = getattr(self, "_trigger_volumes", 0)
        out = np.zeros((max(k, 1), 16), np.float32)
        self._ok(self.lib.scTickReadTriggerMatrices(self.ctx, 0, k, _f(out)), "scTickReadTriggerMatrices")
        return out[:k].copy()

    def trigger_anchors(self):
        """The anchors as they stand now: renamed by remove_entities where their entity moved, capi.ANCHOR_DEAD where it was removed."""
        k = getattr(self, "_trigger_volumes", 0)
        out = np.zeros(max(k, 1), np.uint32)
        if k:
            self._ok(self.lib.scTickReadTriggerVolumes(self.ctx, 0, k, _u(out)), "scTickReadTriggerVolumes")
        return out[:k].copy()

    # ---- entity-anchored capsule sweeps: given in an entity's local frame, resolved on the device every tick ----
    def anchored_sweeps(self, anchor, local_start, local_end, radius, half_height, mask, skip_self=None, end_frame=None):
        """Upright-capsule sweeps in the local frame of the entities `anchor` (dense indices; capi.ANCHOR_NONE: world space), answered by
        every run with capi.ANCHORED_SWEEPS against that tick's matrices and boxes, in the context's sweep mode (scTickSetAnchoredSweeps).
        end_frame: per sweep capi.SWEEP_END_LOCAL (local_end is a point of the anchor's frame; None: all) or capi.SWEEP_END_WORLD_OFFSET
        (a world-space displacement from the resolved start).  skip_self: per sweep, whether the anchor's own box never answers (None:
        all).  A call with as many sweeps as the current set costs no learn tick and no graph capture."""
        an = np.ascontiguousarray(anchor, np.uint32).reshape(-1)
        k = len(an)
        a, b = _c32(local_start).reshape(-1, 3), _c32(local_end).reshape(-1, 3)
        r, hh = _c32(radius).reshape(-1), _c32(half_height).reshape(-1)
        mk = np.ascontiguousarray(mask, np.uint32).reshape(-1)
        sk = None if skip_self is None else np.ascontiguousarray(skip_self, np.uint8).reshape(-1)
        ef = None if end_frame is None else np.ascontiguousarray(end_frame, np.uint8).reshape(-1)
        assert len(a) == k and len(b) == k and len(r) == k and len(hh) == k and len(mk) == k and (sk is None or len(sk) == k) and (ef is None or len(ef) == k)
        self._ok(self.lib.scTickSetAnchoredSweeps(self.ctx, k, _u(an), _f(a), _f(b), _f(r), _f(hh), _u(mk),
                                                  None if sk is None else sk.ctypes.data_as(capi.U8P),
                                                  None if ef is None else ef.ctypes.data_as(capi.U8P)), "scTickSetAnchoredSweeps")
        self._anchored_sweeps = k

    def anchored_sweep_hits(self):
        """Structured array like sweep_hits() of the last run's anchored sweeps; `pad` is the status (capi.ASWEEP_*)."""
        n = C.c_uint32()
        self._ok(self.lib.scTickReadAnchoredSweepHits(self.ctx, None, 0, C.byref(n)), "scTickReadAnchoredSweepHits")
        buf = (capi.SweepHit * max(n.value, 1))()
        if n.value:
            self._ok(self.lib.scTickReadAnchoredSweepHits(self.ctx, buf, n.value, C.byref(n)), "scTickReadAnchoredSweepHits")
        return np.frombuffer(buf, dtype=SWEEP_HIT_DTYPE, count=n.value).copy()

    def anchored_sweep_segments(self):
        """(start [k, 3], end [k, 3]): the world-space segments the last run with capi.ANCHORED_SWEEPS resolved (NaN: not answered)."""
        k = getattr(self, "_anchored_sweeps", 0)
        a, b = np.zeros((max(k, 1), 3), np.float32), np.zeros((max(k, 1), 3), np.float32)
        self._ok(self.lib.scTickReadAnchoredSweepSegments(self.ctx, 0, k, _f(a), _f(b)), "scTickReadAnchoredSweepSegments")
        return a[:k].copy(), b[:k].copy()

    def anchored_sweep_anchors(self):
        """The anchors as they stand now: renamed by remove_entities where their entity moved, capi.ANCHOR_DEAD where it was removed."""
        k = getattr(self, "_anchored_sweeps", 0)
        out = np.zeros(max(k, 1), np.uint32)
        if k:
            self._ok(self.lib.scTickReadAnchoredSweeps(self.ctx, 0, k, _u(out)), "scTickReadAnchoredSweeps")
        return out[:k].copy()

    def anchored_sweep_shape_info(self):
        """What the last run's anchored sweeps did with their candidates in capi.SWEEP_SHAPES_EXACT mode (scTickGetAnchoredSweepShapeInfo):
        a dict with refined, kept_as_boxes, exhausted.  Separate from sweep_shape_info()."""
        info = capi.SweepShapeInfo()
        self._ok(self.lib.scTickGetAnchoredSweepShapeInfo(self.ctx, C.byref(info)), "scTickGetAnchoredSweepShapeInfo")
        return {k: int(getattr(info, k)) for k, _ in capi.SweepShapeInfo._fields_ if k != "pad"}

    def occupied(self, pos, radius, mask):
        """isOccupiedWorld for a batch of points (sc_traffic_spawner.cpp:93-116); returns a uint8 array."""
        p, r = _c32(pos).reshape(-1, 3), _c32(radius).reshape(-1)
        m = np.ascontiguousarray(mask, np.uint32).reshape(-1)
        out = np.zeros(len(p), np.uint8)
        self._ok(self.lib.scTickQueryOccupied(self.ctx, len(p), _f(p), _f(r), _u(m), out.ctypes.data_as(capi.U8P)), "scTickQueryOccupied")
        return out

    def set_draw_sort_table(self, pipeline_of_material, mesh_count):
        """Material::pipelineId per material handle (0xFF = no such material) and the number of mesh handles:
        what the renderer's filter + sort of the draw list reads (sc_vk.cpp:1842-1864)."""
        p = np.ascontiguousarray(pipeline_of_material, np.uint8)
        self._ok(self.lib.scTickSetDrawSortTable(self.ctx, p.ctypes.data_as(capi.U8P), len(p), int(mesh_count)), "scTickSetDrawSortTable")
        self._material_count = len(p)

    # ---- sector residency (WorldPartition::pumpCompletedLoads / pumpUnloadQueue) ----
    def append_entities(self, pos, rot, scale, bmin=None, bmax=None, mesh=None, material=None, group=None, mask=None, parent=None):
        """Create len(pos) entities at the end of the dense order; returns the first one's dense index."""
        p, r, s = _c32(pos).reshape(-1, 3), _c32(rot).reshape(-1, 3), _c32(scale).reshape(-1, 3)
        k = len(p)
        opt_f = [None if a is None else _c32(a) for a in (bmin, bmax)]
        opt_u = [None if a is None else np.ascontiguousarray(a, np.uint32) for a in (mesh, material, group, mask)]
        par = None if parent is None else np.ascontiguousarray(parent, np.int32)
        first = C.c_uint32()
        self._ok(self.lib.scTickAppendEntities(
            self.ctx, k, _f(p), _f(r), _f(s), *[None if a is None else _f(a) for a in opt_f],
            *[None if a is None else _u(a) for a in opt_u],
            None if par is None else par.ctypes.data_as(capi.I32P), C.byref(first)), "scTickAppendEntities")
        self.n += k
        return first.value

    def remove_entities(self, idx):
        """Swap-remove the entities at these dense indices, in this order; returns (moved_from, moved_to)."""
        i = np.ascontiguousarray(idx, np.uint32)
        src, dst, m = np.zeros(len(i), np.uint32), np.zeros(len(i), np.uint32), C.c_uint32()
        self._ok(self.lib.scTickRemoveEntities(self.ctx, _u(i), len(i), _u(src), _u(dst), C.byref(m)), "scTickRemoveEntities")
        self.n -= len(i)
        return src[:m.value].copy(), dst[:m.value].copy()

    def activate_sector(self, sector, resolve_mesh=None, resolve_material=None):
        """Spawn a parsed .scsector (sectors.SectorData) as pumpCompletedLoads does (sc_world_partition.cpp:916-958):
        one root entity per instance with setLocal, RenderMesh handles from the resolvers (asset id -> handle; the
        reference resolves id 0 to handle 0, :746-749), unit-cube Bounds.  Returns the dense indices."""
        rm = resolve_mesh or (lambda a: 0)
        rt = resolve_material or (lambda a: 0)
        mesh = np.array([0 if int(a) == 0 else rm(int(a)) for a in sector.mesh_id], np.uint32)
        mat = np.array([0 if int(a) == 0 else rt(int(a)) for a in sector.material_id], np.uint32)
        first = self.append_entities(sector.pos, sector.rot, sector.scale, mesh=mesh, material=mat)
        return np.arange(first, first + len(mesh), dtype=np.uint32)

    # ---- upstream movers ----
    def upload_movers(self, first, kind, vel, lo, hi):
        k = np.ascontiguousarray(kind, np.uint8)
        v, a, b = _c32(vel), _c32(lo), _c32(hi)
        self._ok(self.lib.scTickUploadMovers(self.ctx, first, len(k), k.ctypes.data_as(capi.U8P), _f(v), _f(a), _f(b)), "scTickUploadMovers")

    def advance_movers(self, dt):
        self._ok(self.lib.scTickAdvanceMovers(self.ctx, float(dt)), "scTickAdvanceMovers")

    # ---- on-rails traffic ----
    def set_lane_graph(self, g):
        """g: lanes.LaneGraph (or anything with the same arrays)"""
        a = {k: np.ascontiguousarray(getattr(g, k), dt) for k, dt in (
            ("seg_start", np.float32), ("seg_dir", np.float32), ("seg_length", np.float32), ("seg_active", np.uint8),
            ("seg_end_node", np.uint32), ("seg_speed_limit", np.float32), ("node_pos", np.float32),
            ("node_conn_offset", np.uint32), ("node_conn", np.uint32))}
        lg = capi.LaneGraph()
        lg.segments, lg.nodes, lg.connections = len(a["seg_length"]), len(a["node_pos"]), len(a["node_conn"])
        lg.seg_start3, lg.seg_dir3, lg.seg_length = _f(a["seg_start"]), _f(a["seg_dir"]), _f(a["seg_length"])
        lg.seg_active = a["seg_active"].ctypes.data_as(capi.U8P)
        lg.seg_end_node, lg.seg_speed_limit = _u(a["seg_end_node"]), _f(a["seg_speed_limit"])
        lg.node_pos3, lg.node_conn_offset, lg.node_conn = _f(a["node_pos"]), _u(a["node_conn_offset"]), _u(a["node_conn"])
        self._ok(self.lib.scTickSetLaneGraph(self.ctx, C.byref(lg)), "scTickSetLaneGraph")

    def set_lane_active(self, segment_ids, active):
        ids = np.ascontiguousarray(segment_ids, np.uint32)
        self._ok(self.lib.scTickSetLaneActive(self.ctx, _u(ids), len(ids), 1 if active else 0), "scTickSetLaneActive")

    def upload_traffic_agents(self, first, is_agent, lane_id, lane_s, target_speed, mode, look_ahead=None):
        ia, md = np.ascontiguousarray(is_agent, np.uint8), np.ascontiguousarray(mode, np.uint8)
        ln, ls, sp = np.ascontiguousarray(lane_id, np.uint32), _c32(lane_s), _c32(target_speed)
        la = None if look_ahead is None else _c32(look_ahead)
        self._ok(self.lib.scTickUploadTrafficAgents(self.ctx, first, len(ia), ia.ctypes.data_as(capi.U8P), _u(ln), _f(ls), _f(sp),
                                                    md.ctypes.data_as(capi.U8P), None if la is None else _f(la)), "scTickUploadTrafficAgents")

    def traffic_agents(self):
        """(lane_id, lane_s, target_speed, mode) of every entity (meaningful where the entity is an agent)"""
        ln, ls, sp, md = np.zeros(self.n, np.uint32), np.zeros(self.n, np.float32), np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)
        self._ok(self.lib.scTickReadTrafficAgents(self.ctx, 0, self.n, _u(ln), _f(ls), _f(sp), md.ctypes.data_as(capi.U8P)), "scTickReadTrafficAgents")
        return ln, ls, sp, md

    def set_traffic_sensors(self, on=True, front_ray_length=20.0, safe_distance=10.0):
        """the traffic AI's obstacle ray per OnRails agent, cast in every run with BROADPHASE; its brake scales the next on-rails step"""
        self._ok(self.lib.scTickSetTrafficSensors(self.ctx, 1 if on else 0, float(front_ray_length), float(safe_distance)), "scTickSetTrafficSensors")

    def upload_traffic_sensors(self, first, front_ray_length, safe_distance):
        """per-agent TrafficSensors::frontRayLength / safeDistance for the entities first .. first + len - 1"""
        rl, sf = _c32(front_ray_length).reshape(-1), _c32(safe_distance).reshape(-1)
        assert len(rl) == len(sf)
        self._ok(self.lib.scTickUploadTrafficSensors(self.ctx, first, len(rl), _f(rl), _f(sf)), "scTickUploadTrafficSensors")

    def traffic_sensors(self):
        """(lastHitDistance, lastHitType) per entity as the last ray tick left them (0 none, 2 vehicle, 3 world)"""
        dist, typ = np.zeros(self.n, np.float32), np.zeros(self.n, np.uint8)
        self._ok(self.lib.scTickReadTrafficSensors(self.ctx, 0, self.n, _f(dist), typ.ctypes.data_as(capi.U8P)), "scTickReadTrafficSensors")
        return dist, typ

    def traffic_brakes(self):
        out = np.zeros(self.n, np.float32)
        self._ok(self.lib.scTickReadTrafficBrakes(self.ctx, 0, self.n, _f(out)), "scTickReadTrafficBrakes")
        return out

    def set_traffic_speed_multiplier(self, m):
        self._ok(self.lib.scTickSetTrafficSpeedMultiplier(self.ctx, float(m)), "scTickSetTrafficSpeedMultiplier")

    def select_traffic_tiers(self, player_pos, a_enter=50.0, a_exit=70.0, b_enter=110.0, b_exit=150.0, max_physics=24, max_kinematic=64):
        """TrafficLODSystem's tier selection; returns (physics, kinematic, on_rails) counts after the caps"""
        pp = _c32(player_pos)
        tp = capi.TierParams(a_enter, a_exit, b_enter, b_exit, max_physics, max_kinematic)
        out = capi.TierCounts()
        self._ok(self.lib.scTickSelectTrafficTiers(self.ctx, _f(pp), C.byref(tp), C.byref(out)), "scTickSelectTrafficTiers")
        return out.physics, out.kinematic, out.on_rails

    def select_traffic_despawns(self, player_pos, max_total):
        """TrafficLODSystem's total cap: dense indices of the vehicles to despawn, in the reference's order"""
        pp = _c32(player_pos)
        cnt = C.c_uint32()
        self._ok(self.lib.scTickSelectTrafficDespawns(self.ctx, _f(pp), int(max_total), None, 0, C.byref(cnt)), "scTickSelectTrafficDespawns")
        out = np.zeros(max(cnt.value, 1), np.uint32)
        if cnt.value:
            self._ok(self.lib.scTickSelectTrafficDespawns(self.ctx, _f(pp), int(max_total), _u(out), cnt.value, C.byref(cnt)), "scTickSelectTrafficDespawns")
        return out[:cnt.value].copy()

    def set_frame_producer(self, kind, param=0.0):
        """0 none, 1 nudge roots by `param`, 2 advance movers by dt=`param`: run() then is the whole frame"""
        self._ok(self.lib.scTickSetFrameProducer(self.ctx, int(kind), float(param)), "scTickSetFrameProducer")

    def mover_velocities(self):
        out = np.zeros((self.n, 2), np.float32)
        self._ok(self.lib.scTickReadMoverVelocities(self.ctx, 0, self.n, _f(out)), "scTickReadMoverVelocities")
        return out

    # ---- multi-GPU tiles ----
    def set_tile(self, rank, neighbour_mask):
        self._ok(self.lib.scTickSetTile(self.ctx, rank, neighbour_mask), "scTickSetTile")

    def set_tile_grid(self, tile_x, tile_z, tiles_x, tiles_z):
        self._ok(self.lib.scTickSetTileGrid(self.ctx, tile_x, tile_z, tiles_x, tiles_z), "scTickSetTileGrid")

    def set_border_capacity(self, records_per_ring_sector):
        """records per ring sector of a side (on average) a border message can carry; every tile of a world alike, before comm_init / binding"""
        self._ok(self.lib.scTickSetBorderCapacity(self.ctx, int(records_per_ring_sector)), "scTickSetBorderCapacity")

    def border_bytes(self, direction):
        return int(self.lib.scTickBorderBytes(self.ctx, direction))

    def bind_border(self, direction, send_ptr, recv_ptr):
        self._ok(self.lib.scTickBindBorderBuffers(self.ctx, direction, send_ptr, recv_ptr), "scTickBindBorderBuffers")

    def set_pairs_stream(self, hip_stream):
        """Pipelined tiles: merge + queries + pair search of a tick go to this stream (None / 0 switches it off)."""
        self._ok(self.lib.scTickSetPairsStream(self.ctx, C.c_void_p(hip_stream or None)), "scTickSetPairsStream")

    def bind_border_parity(self, parity, direction, send_ptr, recv_ptr):
        self._ok(self.lib.scTickBindBorderBuffersParity(self.ctx, parity, direction, C.c_void_p(send_ptr), C.c_void_p(recv_ptr)),
                 "scTickBindBorderBuffersParity")

    def border_buffer(self, parity, direction, recv=False):
        """device address of the message buffer bound for (tick parity, direction); 0 = none"""
        return int(self.lib.scTickGetBorderBuffer(self.ctx, parity, direction, 1 if recv else 0) or 0)

    def run_pairs(self):
        self._ok(self.lib.scTickRunPairs(self.ctx), "scTickRunPairs")

    # ---- library-owned exchange (RCCL communicator inside libsc_tick.so) ----
    def comm_init(self, unique_id, world_size, rank, peers=None):
        """unique_id: 128 bytes from capi.comm_unique_id() of rank 0, handed to every rank by the host's own channel.
        peers (optional): rank of the neighbour in each of the 8 directions, -1 = none (default: row-major tile order)."""
        if peers is not None:
            pr = np.ascontiguousarray(peers, np.int32)
            assert len(pr) == 8
            self._ok(self.lib.scTickCommSetPeers(self.ctx, pr.ctypes.data_as(capi.I32P)), "scTickCommSetPeers")
        uid = np.frombuffer(bytes(unique_id), np.uint8).copy()
        assert len(uid) == capi.COMM_ID_BYTES
        self._ok(self.lib.scTickCommInit(self.ctx, uid.ctypes.data_as(capi.U8P), int(world_size), int(rank)), "scTickCommInit")

    def comm_destroy(self):
        self._ok(self.lib.scTickCommDestroy(self.ctx), "scTickCommDestroy")

    def set_pipelined(self, on):
        """False / 0 = off, True / 1 = on (default depth 4), 2..4 = on with that many copies of the per-tick broadphase state"""
        self._ok(self.lib.scTickSetPipelined(self.ctx, int(on)), "scTickSetPipelined")

    def gather_visible_counts(self, max_ranks=128):
        """Every rank's visible count of the last tick (one all-gather over the library's communicator; every rank must call),
        this rank's offset in the global visible list and the list's length: (counts, offset, total).  SURVEY 8e, result assembly."""
        counts = np.zeros(max_ranks, np.uint32)
        off, tot = C.c_uint64(), C.c_uint64()
        self._ok(self.lib.scTickGatherVisibleCounts(self.ctx, counts.ctypes.data_as(capi.U32P), max_ranks, C.byref(off), C.byref(tot)), "scTickGatherVisibleCounts")
        ranks = max(self.comm_info()["world_size"], 1)
        return counts[:ranks].copy(), int(off.value), int(tot.value)

    def comm_info(self):
        """the exchange as the library sees it (communicator, peers, operations per group, host time per half of a step) as a dict"""
        ci = capi.CommInfo()
        self._ok(self.lib.scTickGetCommInfo(self.ctx, C.byref(ci)), "scTickGetCommInfo")
        return {k: (list(getattr(ci, k)) if k == "peer_rank" else getattr(ci, k)) for k, _ in capi.CommInfo._fields_}

    def set_world_layers(self, group, mask, known=True):
        """the tiled world's layer vocabulary: arrays (or ORs) of the group and mask words of every collider on ANY tile (scTickSetWorldLayers)"""
        g = int(np.bitwise_or.reduce(np.asarray(group, np.uint32).ravel())) if np.ndim(group) else int(group)
        m = int(np.bitwise_or.reduce(np.asarray(mask, np.uint32).ravel())) if np.ndim(mask) else int(mask)
        self._ok(self.lib.scTickSetWorldLayers(self.ctx, g, m, 1 if known else 0), "scTickSetWorldLayers")

    def bin_stats(self):
        """how the broadphase bins are filled: remembered slots, those written on every tick, whether the last tick could leave slots unwritten, learn ticks;
        quiet_last_tick: the last tick filled no bin at all (nothing reads them: scTickGetBinStats) -- the other flags then tell of the last tick that did"""
        st = np.zeros(4, np.uint32)
        self._ok(self.lib.scTickGetBinStats(self.ctx, _u(st)), "scTickGetBinStats")
        return {"remembered_slots": int(st[0]), "written_every_tick": int(st[1]), "lazy_last_tick": bool(st[2] & capi.BIN_LAZY),
                "unchanged_records_stay": bool(st[2] & capi.BIN_STAY), "pair_role_sweep_only": bool(st[2] & capi.BIN_SWEEP_ONLY),
                "quiet_last_tick": bool(st[2] & capi.BIN_QUIET),
                "learn_ticks": int(st[3])}

    def tail_stats(self):
        """where the last tick ended: whether its fused kernel owned the dirty words (dirty clear and root nudge per span), and whether the
        world is span-closed -- no parent link crosses a span boundary (host-side: no read-back)"""
        st = np.zeros(2, np.uint32)
        self._ok(self.lib.scTickGetTailStats(self.ctx, _u(st)), "scTickGetTailStats")
        return {"tail_owned_dirty": bool(st[0]), "span_closed": bool(st[1])}

    def compact_stats(self):
        """how the last tick's compaction was cut into workgroups: workgroups of the compaction role and spans per workgroup, 0 / 0 when
        the tick had none (host-side: no read-back).  More than one span per workgroup on a launch of its own: the wide form ran"""
        st = np.zeros(2, np.uint32)
        self._ok(self.lib.scTickGetCompactStats(self.ctx, _u(st)), "scTickGetCompactStats")
        return {"workgroups": int(st[0]), "spans_per_workgroup": int(st[1])}

    def carry_stats(self):
        """the carried compaction since creation: ticks that deferred their compaction, compactions carried at the head of the next tick's
        fused launch, compactions settled by a launch of their own (host-side: no read-back; scTickGetCarryStats)"""
        st = np.zeros(3, np.uint32)
        self._ok(self.lib.scTickGetCarryStats(self.ctx, _u(st)), "scTickGetCarryStats")
        return {"deferred": int(st[0]), "carried": int(st[1]), "settled": int(st[2])}

    def frame_stats(self):
        """which code wrote the last tick's frame: (who wrote the draw items, who staged the read-back block) as capi.FRAME_ITEMS_* /
        capi.FRAME_BLOCK_* (host-side: no read-back, no synchronisation; scTickGetFrameStats)"""
        st = np.zeros(2, np.uint32)
        self._ok(self.lib.scTickGetFrameStats(self.ctx, _u(st)), "scTickGetFrameStats")
        return int(st[0]), int(st[1])

    def learn_ticks(self):
        """learn ticks so far (host-side counter: no read-back)"""
        st = np.zeros(1, np.uint32)
        self._ok(self.lib.scTickGetLearnTicks(self.ctx, _u(st)), "scTickGetLearnTicks")
        return int(st[0])

    def bounds_class_stats(self):
        """bounds classes (host-side counters): distinct boxes in the palette, wave-tiles whose bounded entities share one, wave-tiles whose do not,
        bounded entities whose box the full palette could not take"""
        st = np.zeros(4, np.uint32)
        self._ok(self.lib.scTickGetBoundsClassStats(self.ctx, _u(st)), "scTickGetBoundsClassStats")
        return {"palette_entries": int(st[0]), "tiles_shared": int(st[1]), "tiles_mixed": int(st[2]), "entities_no_class": int(st[3])}

    def topology_class_stats(self):
        """topology classes (host-side): distinct patterns, wave-tiles that are closed and numbered, wave-tiles that are not (as of the last
        re-link), and whether the last run's fused kernel was the classed instance"""
        st = np.zeros(4, np.uint32)
        self._ok(self.lib.scTickGetTopologyClassStats(self.ctx, _u(st)), "scTickGetTopologyClassStats")
        return {"patterns": int(st[0]), "tiles_classed": int(st[1]), "tiles_unclassed": int(st[2]), "classed_last_tick": bool(st[3])}

    def reset_host_times(self):
        self._ok(self.lib.scTickResetHostTimes(self.ctx), "scTickResetHostTimes")

    def tile_step(self, flags):
        """One whole step of a tile: tick + pack, RCCL exchange, merge + pair search -- one call, nothing waits on the host."""
        self._ok(self.lib.scTickTileStep(self.ctx, flags), "scTickTileStep")

    def exchange_borders(self):
        self._ok(self.lib.scTickExchangeBorders(self.ctx), "scTickExchangeBorders")

    def set_stream(self, hip_stream, external=True):
        """external=True: run on the caller's hipStream_t (0 = the legacy default stream); False: own stream"""
        self._ok(self.lib.scTickSetStream(self.ctx, hip_stream, 1 if external else 0), "scTickSetStream")

    def set_profiling(self, period):
        """0 = off, n = record HIP events on every n-th tick"""
        self._ok(self.lib.scTickSetProfiling(self.ctx, int(period)), "scTickSetProfiling")

    def set_profiling_kernels(self, kernels=None):
        """time only these kernels (capi.K_* indices; None = all): a launch timed by events costs ~6 us of gap on its queue"""
        mask = 0 if kernels is None else sum(1 << int(k) for k in kernels)
        self._ok(self.lib.scTickSetProfilingKernels(self.ctx, mask), "scTickSetProfilingKernels")

    def set_graph_mode(self, on):
        self._ok(self.lib.scTickSetGraphMode(self.ctx, 1 if on else 0), "scTickSetGraphMode")

    def kernel_times_ms(self, kernel):
        cnt = C.c_uint32()
        self._ok(self.lib.scTickGetKernelTimes(self.ctx, kernel, None, 0, C.byref(cnt)), "scTickGetKernelTimes")
        out = np.zeros(cnt.value, np.float32)
        if cnt.value:
            self._ok(self.lib.scTickGetKernelTimes(self.ctx, kernel, _f(out), cnt.value, C.byref(cnt)), "scTickGetKernelTimes")
        return out

    # ---- per-frame read-back, overlapped with the next tick ----
    def set_frame_readback(self, max_visible, max_draws=0):
        self._ok(self.lib.scTickSetFrameReadback(self.ctx, int(max_visible), int(max_draws)), "scTickSetFrameReadback")

    def acquire_frame(self, frames_back=0, copy=True):
        """Frame `frames_back` (0 latest, 1 the one before): (frame struct, visible indices, draw items as a (n, 80) byte array).
        With copy=False the arrays are views of the pinned buffer (valid until the second run after this frame's)."""
        fr = capi.Frame()
        self._ok(self.lib.scTickAcquireFrame(self.ctx, int(frames_back), C.byref(fr)), "scTickAcquireFrame")
        nv, nd = fr.visible_in_buffer, fr.draws_in_buffer
        vis = np.ctypeslib.as_array(fr.visible_indices, shape=(nv,)) if nv else np.zeros(0, np.uint32)
        draws = (np.ctypeslib.as_array(C.cast(fr.draws, capi.U8P), shape=(nd * 80,)).reshape(nd, 80) if nd else np.zeros((0, 80), np.uint8))
        return fr, (vis.copy() if copy else vis), (draws.copy() if copy else draws)

    # ---- bind runs of the sorted draw list + material touch set (capi.BIND_RUNS with DRAWS | SORT_DRAWS) ----
    BIND_RUN_DTYPE = np.dtype([(n, np.uint32) for n, _ in capi.BindRun._fields_])

    def set_bind_runs(self, max_runs):
        """Room for max_runs rows in the run table (scTickSetBindRuns; after set_draw_sort_table; 0 switches it off)."""
        self._ok(self.lib.scTickSetBindRuns(self.ctx, int(max_runs)), "scTickSetBindRuns")
        self._max_runs = int(max_runs)

    def bind_runs(self):
        """(runs, info) of the last run with capi.BIND_RUNS: a structured array (first, count, pipeline, material, mesh, binds) of the
        first min(info["runs"], max_runs) runs in list order, and the report as a dict whose totals cover all runs."""
        cap = getattr(self, "_max_runs", 0)
        runs = np.zeros(max(cap, 1), self.BIND_RUN_DTYPE)
        info = capi.BindInfo()
        self._ok(self.lib.scTickReadBindRuns(self.ctx, runs.ctypes.data_as(C.POINTER(capi.BindRun)), cap, C.byref(info)), "scTickReadBindRuns")
        out = {k: int(getattr(info, k)) for k, _ in capi.BindInfo._fields_}
        return runs[:min(out["runs"], cap)].copy(), out

    def material_touches(self):
        """bool[material_count]: handle h was the materialId of some emitted draw of the last run with capi.BIND_RUNS."""
        cnt = C.c_uint32()
        self._ok(self.lib.scTickReadMaterialTouches(self.ctx, None, 0, C.byref(cnt)), "scTickReadMaterialTouches")
        words = np.zeros(max(cnt.value, 1), np.uint32)
        if cnt.value:
            self._ok(self.lib.scTickReadMaterialTouches(self.ctx, _u(words), cnt.value, C.byref(cnt)), "scTickReadMaterialTouches")
        bits = np.unpackbits(words[:cnt.value].view(np.uint8), bitorder="little").astype(bool)
        return bits[:getattr(self, "_material_count", len(bits))].copy()

    def acquire_frame_binds(self, frames_back=0):
        """The bind runs staged with frame `frames_back` (set_frame_readback + set_bind_runs): (tick, runs, info dict, touches bool array);
        a frame whose run had no capi.BIND_RUNS has no runs and an all-zero report."""
        fb = capi.FrameBinds()
        self._ok(self.lib.scTickAcquireFrameBinds(self.ctx, int(frames_back), C.byref(fb)), "scTickAcquireFrameBinds")
        nr, nw = fb.runs_in_buffer, fb.info.touch_words
        runs = (np.ctypeslib.as_array(C.cast(fb.runs, capi.U32P), shape=(nr * 6,)).copy().view(self.BIND_RUN_DTYPE) if nr
                else np.zeros(0, self.BIND_RUN_DTYPE))
        words = np.ctypeslib.as_array(fb.touch_words, shape=(nw,)).copy() if nw else np.zeros(0, np.uint32)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
        info = {k: int(getattr(fb.info, k)) for k, _ in capi.BindInfo._fields_}
        return int(fb.tick), runs, info, bits[:getattr(self, "_material_count", len(bits))].copy()

    # ---- results ----
    def counts(self):
        c = capi.Counts()
        self._ok(self.lib.scTickGetCounts(self.ctx, C.byref(c)), "scTickGetCounts")
        return c

    def _index_list(self, fn, name):
        cnt = C.c_uint32()
        out = np.zeros(max(self.n, 1), np.uint32)
        self._ok(fn(self.ctx, _u(out), len(out), C.byref(cnt)), name)
        return out[:cnt.value].copy()

    def visible(self):
        return self._index_list(self.lib.scTickReadVisible, "scTickReadVisible")

    def culled(self):
        return self._index_list(self.lib.scTickReadCulled, "scTickReadCulled")

    def visibility_bits(self):
        nw = (self.n + 63) // 64
        w = np.zeros(max(nw, 1), np.uint64)
        self._ok(self.lib.scTickReadVisibilityBits(self.ctx, w.ctypes.data_as(capi.U64P), len(w)), "scTickReadVisibilityBits")
        bits = np.unpackbits(w[:nw].view(np.uint8), bitorder="little")[:self.n]
        return bits.astype(np.uint8)

    def world_matrices(self, first=0, count=None):
        count = self.n - first if count is None else count
        out = np.zeros((count, 16), np.float32)
        self._ok(self.lib.scTickReadWorldMatrices(self.ctx, first, count, _f(out)), "scTickReadWorldMatrices")
        return out

    def world_matrices_indexed(self, idx):
        i = np.ascontiguousarray(idx, np.uint32)
        out = np.zeros((len(i), 16), np.float32)
        self._ok(self.lib.scTickReadWorldMatricesIndexed(self.ctx, _u(i), len(i), _f(out)), "scTickReadWorldMatricesIndexed")
        return out

    def dirty(self):
        out = np.zeros(self.n, np.uint8)
        self._ok(self.lib.scTickReadDirty(self.ctx, 0, self.n, out.ctypes.data_as(capi.U8P)), "scTickReadDirty")
        return out

    def positions(self):
        out = np.zeros((self.n, 3), np.float32)
        self._ok(self.lib.scTickReadPositions(self.ctx, 0, self.n, _f(out)), "scTickReadPositions")
        return out

    def world_aabbs(self):
        mn, mx = np.zeros((self.n, 3), np.float32), np.zeros((self.n, 3), np.float32)
        self._ok(self.lib.scTickReadWorldAabbs(self.ctx, 0, self.n, _f(mn), _f(mx)), "scTickReadWorldAabbs")
        return mn, mx

    def pairs(self, cap=None):
        cnt = C.c_uint32()
        self._ok(self.lib.scTickReadPairs(self.ctx, None, 0, C.byref(cnt)), "scTickReadPairs")
        n = min(cnt.value, self.max_pairs)              # the list holds at most max_pairs; cnt is the number found
        n = n if cap is None else min(cap, n)
        out = np.full((max(n, 1), 2), 0xFFFFFFFF, np.uint32)
        if n:
            self._ok(self.lib.scTickReadPairs(self.ctx, _u(out), n, C.byref(cnt)), "scTickReadPairs")
        out = out[:n]
        out = out[out[:, 1] != 0xFFFFFFFF]              # a full shard segment keeps fewer than were found
        return out.copy(), cnt.value

    # ---- pair events: which pairs begun / ended since the last run with capi.PAIR_EVENTS ----
    def set_pair_events(self, max_tracked, max_events):
        """Remember the pair set on the device and report its tick-to-tick difference on every run with capi.PAIR_EVENTS
        (scTickSetPairEvents): room for max_tracked pairs in the set and max_events pairs in each list; (0, 0) switches it off."""
        self._ok(self.lib.scTickSetPairEvents(self.ctx, int(max_tracked), int(max_events)), "scTickSetPairEvents")
        self._max_events = int(max_events)

    def pair_events(self):
        """(begun[k, 2], ended[m, 2], info) of the last run with capi.PAIR_EVENTS: uint32 ids a < b in unspecified order; info is a dict
        (begun, ended, tracked, resync, overflow, events_truncated) whose begun / ended are the true totals -- the lists hold at most max_events."""
        cap = getattr(self, "_max_events", 0)
        b, e = np.zeros((max(cap, 1), 2), np.uint32), np.zeros((max(cap, 1), 2), np.uint32)
        info = capi.PairEventInfo()
        self._ok(self.lib.scTickReadPairEvents(self.ctx, _u(b), cap, _u(e), cap, C.byref(info)), "scTickReadPairEvents")
        out = {k: int(getattr(info, k)) for k, _ in capi.PairEventInfo._fields_}
        return b[:min(out["begun"], cap)].copy(), e[:min(out["ended"], cap)].copy(), out

    # ---- touching pairs: the pairs of the tick's list whose collider shapes overlap ----
    def set_pair_shapes(self, max_touching):
        """List, on every run with capi.PAIR_SHAPES, the pairs of the tick's pair list whose collider shapes (upload_colliders: box, sphere,
        capsule, through the members' world matrices of the tick) overlap: room for max_touching pairs; 0 switches it off
        (scTickSetPairShapes).  Drops captured graphs, costs no learn tick."""
        self._ok(self.lib.scTickSetPairShapes(self.ctx, int(max_touching)), "scTickSetPairShapes")
        self._max_touching = int(max_touching)

    def _read_listed(self, name, info_type, count, dtype, shape=(), pointer=capi.U32P):
        """What the readers of the touching list and of the records per entry of it share: room for max_touching records of `dtype`, the
        call `name`, the report as a dict, and the first min(report[count], max_touching) records."""
        cap = getattr(self, "_max_touching", 0)
        rec = np.zeros((max(cap, 1),) + shape, dtype)
        info = info_type()
        self._ok(getattr(self.lib, name)(self.ctx, rec.ctypes.data_as(pointer), cap, C.byref(info)), name)
        out = {k: int(getattr(info, k)) for k, _ in info_type._fields_}
        return rec[:min(out[count], cap)].copy(), out

    def read_pair_shapes(self):
        """(touching[n, 2], info) of the last run with capi.PAIR_SHAPES: uint32 ids a < b in unspecified order; info is a dict (tested,
        touching, refined, kept_as_boxes, truncated, pairs_truncated) whose touching is the true total -- the list holds at most
        max_touching."""
        return self._read_listed("scTickReadPairShapes", capi.PairShapeInfo, "touching", np.uint32, (2,))

    # ---- pair contacts: point, depth, normal and kind of every entry of the touching list ----
    CONTACT_DTYPE = np.dtype([("point", np.float32, 3), ("depth", np.float32), ("normal", np.float32, 3), ("kind", np.uint32)])

    def set_pair_contacts(self, on):
        """Write, on every run with capi.PAIR_SHAPES, one contact record per entry of the touching list (scTickSetPairContacts); needs
        set_pair_shapes(max_touching > 0) first.  Drops captured graphs, costs no learn tick."""
        self._ok(self.lib.scTickSetPairContacts(self.ctx, 1 if on else 0), "scTickSetPairContacts")

    def pair_contacts_enabled(self):
        on = C.c_uint32()
        self._ok(self.lib.scTickGetPairContacts(self.ctx, C.byref(on)), "scTickGetPairContacts")
        return bool(on.value)

    def read_pair_contacts(self):
        """(records[n], info) of the last run with capi.PAIR_SHAPES while contacts were enabled: a structured array (point[3], depth,
        normal[3], kind), record i for entry i of read_pair_shapes()'s list; info is a dict (written, round_round, round_box, box_box,
        unrefined, deep, degenerate, reserved) over the records written."""
        return self._read_listed("scTickReadPairContacts", capi.PairContactInfo, "written", self.CONTACT_DTYPE, pointer=C.POINTER(capi.PairContact))

    # ---- pair manifolds: up to four points and depths of every entry of the touching list ----
    MANIFOLD_DTYPE = np.dtype([("point", np.float32, (4, 3)), ("depth", np.float32, 4), ("count", np.uint32), ("kind", np.uint32),
                               ("reserved", np.uint32, 2)])

    def set_pair_manifolds(self, on):
        """Write, on every run with capi.PAIR_SHAPES, one manifold record per entry of the touching list (scTickSetPairManifolds); needs
        set_pair_contacts(True) first.  Drops captured graphs, costs no learn tick."""
        self._ok(self.lib.scTickSetPairManifolds(self.ctx, 1 if on else 0), "scTickSetPairManifolds")

    def pair_manifolds_enabled(self):
        on = C.c_uint32()
        self._ok(self.lib.scTickGetPairManifolds(self.ctx, C.byref(on)), "scTickGetPairManifolds")
        return bool(on.value)

    def read_pair_manifolds(self):
        """(records[n], info) of the last run with capi.PAIR_SHAPES while manifolds were enabled: a structured array (point[4][3],
        depth[4], count, kind, reserved[2]), record i for entry i of read_pair_shapes()'s list and record i of read_pair_contacts(); info
        is a dict (written, points, with_one, with_two, with_three, with_four, face, reduced) over the records written."""
        return self._read_listed("scTickReadPairManifolds", capi.PairManifoldInfo, "written", self.MANIFOLD_DTYPE, pointer=C.POINTER(capi.PairManifold))

    # ---- pair islands: the connected components of the movable entities under the touching list ----
    def pair_islands(self, on, fixed_groups=2):
        """Compute, on every run with capi.PAIR_SHAPES, the islands of the touching list (scTickSetPairIslands): entities whose group has a
        bit of fixed_groups are fixed and join nothing (the reference's static bodies are on layer 2).  Needs set_pair_shapes(max_touching
        > 0) first.  Drops captured graphs, costs no learn tick."""
        self._ok(self.lib.scTickSetPairIslands(self.ctx, 1 if on else 0, int(fixed_groups)), "scTickSetPairIslands")

    def pair_islands_enabled(self):
        on, fixed = C.c_uint32(), C.c_uint32()
        self._ok(self.lib.scTickGetPairIslands(self.ctx, C.byref(on), C.byref(fixed)), "scTickGetPairIslands")
        return bool(on.value)

    def pair_islands_fixed_groups(self):
        """The fixed_groups the islands go by (0 while they are off)."""
        on, fixed = C.c_uint32(), C.c_uint32()
        self._ok(self.lib.scTickGetPairIslands(self.ctx, C.byref(on), C.byref(fixed)), "scTickGetPairIslands")
        return int(fixed.value)

    def read_pair_islands(self):
        """(labels[count], edge_islands[n], info) of the last run with capi.PAIR_SHAPES while islands were enabled: labels[e] is the id of
        the member with the smallest dense index in e's island (capi.ISLAND_NONE for a fixed entity), edge_islands[i] the island of entry
        i of read_pair_shapes()'s list; info is a dict (edges, linking, anchored, islands, bodies, movable, list_truncated, gave_up)."""
        cap = getattr(self, "_max_touching", 0)
        labels, edges = np.zeros(max(self.n, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
        info = capi.PairIslandInfo()
        self._ok(self.lib.scTickReadPairIslands(self.ctx, _u(labels), self.n, _u(edges), cap, C.byref(info)), "scTickReadPairIslands")
        out = {k: int(getattr(info, k)) for k, _ in capi.PairIslandInfo._fields_}
        return labels[:self.n].copy(), edges[:min(out["edges"], cap)].copy(), out

    # ---- pair persistence: this run's manifold points matched to the last flagged run's, with an age and a payload per point ----
    PERSIST_DTYPE = np.dtype([("prev_entry", np.uint32), ("prev_slot", np.uint8, 4), ("age", np.uint8, 4), ("reserved", np.uint32)])

    def pair_persistence(self, on, match_dist=0.02):
        """Match, on every run with capi.PAIR_SHAPES, every entry of the touching list and every point of its manifold to the last such
        run's (scTickSetPairPersistence): points match within match_dist metres in the first member's frame (the default is Bullet's
        contact breaking threshold).  Needs set_pair_manifolds(True) first.  Drops captured graphs, costs no learn tick; a second call
        while it is on keeps what is remembered."""
        self._ok(self.lib.scTickSetPairPersistence(self.ctx, 1 if on else 0, float(match_dist)), "scTickSetPairPersistence")

    def _pair_persistence(self):
        on, dist = C.c_uint32(), C.c_float()
        self._ok(self.lib.scTickGetPairPersistence(self.ctx, C.byref(on), C.byref(dist)), "scTickGetPairPersistence")
        return bool(on.value), float(dist.value)

    def pair_persistence_enabled(self):
        return self._pair_persistence()[0]

    def pair_persistence_match_dist(self):
        """The match_dist the matching goes by (0 while it is off)."""
        return self._pair_persistence()[1]

    def write_pair_payloads(self, rows, first=0):
        """Overwrite the payload rows [first, first + len(rows)) of the last flagged run -- float32 [n][4][4], four words for each of an
        entry's four slots -- which the next flagged run carries to the points it matches (scTickWritePairPayloads): where a solver
        leaves its accumulated impulses."""
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 4, 4)
        self._ok(self.lib.scTickWritePairPayloads(self.ctx, _f(rows), int(first), len(rows)), "scTickWritePairPayloads")

    def read_pair_payloads(self):
        """rows[n][4][4] of the last flagged run as they stand: what the run carried, then what write_pair_payloads wrote."""
        cap = getattr(self, "_max_touching", 0)
        info = capi.PairPersistInfo()
        self._ok(self.lib.scTickReadPairPersistence(self.ctx, None, 0, C.byref(info)), "scTickReadPairPersistence")
        rows = np.zeros((max(cap, 1), 4, 4), np.float32)
        self._ok(self.lib.scTickReadPairPayloads(self.ctx, _f(rows), cap), "scTickReadPairPayloads")
        return rows[:min(int(info.written), cap)].copy()

    def read_pair_persistence(self):
        """(records[n], info) of the last run with capi.PAIR_SHAPES while persistence was enabled: a structured array (prev_entry,
        prev_slot[4], age[4], reserved), record i for entry i of read_pair_shapes()'s list and record i of read_pair_manifolds(); info is a
        dict (written, kept_pairs, new_pairs, kept_points, new_points, resync, list_truncated, gave_up)."""
        return self._read_listed("scTickReadPairPersistence", capi.PairPersistInfo, "written", self.PERSIST_DTYPE, pointer=C.POINTER(capi.PairPersist))

    # ---- pair sleep: which islands are at rest, who fell asleep, who woke ----
    def pair_sleep(self, on, lin_tol=0.005, ang_tol=0.005, rest_runs=120, max_events=4096):
        """Keep, on every run with capi.PAIR_SHAPES, a rest state per entity (scTickSetPairSleep): an entity is still while its world rows
        stay within lin_tol (translation) / ang_tol (the nine other elements) of an anchor pose, an island falls asleep once every member
        has been still for rest_runs runs (1 .. 255; the default is Bullet's 2 s at 60 Hz), and each run reports at most max_events ids
        per event list.  Needs pair_islands(True) first.  A second call with the same max_events keeps what is remembered."""
        self._ok(self.lib.scTickSetPairSleep(self.ctx, 1 if on else 0, float(lin_tol), float(ang_tol), int(rest_runs), int(max_events)), "scTickSetPairSleep")

    def pair_sleep_params(self):
        """(enabled, lin_tol, ang_tol, rest_runs, max_events) as the context holds them (zeros while off)"""
        on, rr, me = C.c_uint32(), C.c_uint32(), C.c_uint32()
        lt, at = C.c_float(), C.c_float()
        self._ok(self.lib.scTickGetPairSleep(self.ctx, C.byref(on), C.byref(lt), C.byref(at), C.byref(rr), C.byref(me)), "scTickGetPairSleep")
        return bool(on.value), float(lt.value), float(at.value), int(rr.value), int(me.value)

    @property
    def pair_sleep_enabled(self):
        return self.pair_sleep_params()[0]

    def wake_entities(self, ids):
        """The host's activateBody (scTickWakeEntities): rest = 0 and no anchor for the ids (rank << 24 | index) of own entities, so the
        next flagged run reports their islands in `woke`.  Outside any captured graph: graph mode replays across it."""
        i = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        self._ok(self.lib.scTickWakeEntities(self.ctx, _u(i), len(i)), "scTickWakeEntities")

    def read_pair_sleep(self):
        """(states[n], fell_asleep, woke, info) of the last run with capi.PAIR_SHAPES while pair sleep was enabled: the state word per
        entity (rest | capi.SLEEP_ASLEEP | SLEEP_STILL | SLEEP_MOVABLE), the two event lists as ids -- each cut at max_events, the true
        counts in info -- and info as a dict (flags, asleep, islands_asleep, fell_asleep, woke, awake_entries, epoch, pad)."""
        cap = self.pair_sleep_params()[4]
        states = np.zeros(max(self.n, 1), np.uint32)
        fell, woke = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
        info = capi.PairSleepInfo()
        self._ok(self.lib.scTickReadPairSleep(self.ctx, _u(states), self.n, _u(fell), cap, _u(woke), cap, C.byref(info)), "scTickReadPairSleep")
        out = {k: int(getattr(info, k)) for k, _ in capi.PairSleepInfo._fields_}
        return states[:self.n].copy(), fell[:min(out["fell_asleep"], cap)].copy(), woke[:min(out["woke"], cap)].copy(), out

    # ---- touch events: which pairs begun / ended TOUCHING since the last run with capi.TOUCH_EVENTS ----
    def set_touch_events(self, max_tracked, max_events):
        """Remember the touching set -- the pairs of the tick's list that the collider shapes do not prove apart -- on the device and report
        its tick-to-tick difference on every run with capi.TOUCH_EVENTS (scTickSetTouchEvents): room for max_tracked pairs in the set and
        max_events pairs in each list; (0, 0) switches it off.  Needs neither capi.PAIR_SHAPES nor set_pair_shapes."""
        self._ok(self.lib.scTickSetTouchEvents(self.ctx, int(max_tracked), int(max_events)), "scTickSetTouchEvents")
        self._max_touch_events = int(max_events)

    def touch_events(self):
        """(begun[k, 2], ended[m, 2], info) of the last run with capi.TOUCH_EVENTS, shaped as pair_events() returns them."""
        cap = getattr(self, "_max_touch_events", 0)
        b, e = np.zeros((max(cap, 1), 2), np.uint32), np.zeros((max(cap, 1), 2), np.uint32)
        info = capi.TouchEventInfo()
        self._ok(self.lib.scTickReadTouchEvents(self.ctx, _u(b), cap, _u(e), cap, C.byref(info)), "scTickReadTouchEvents")
        out = {k: int(getattr(info, k)) for k, _ in capi.TouchEventInfo._fields_}
        return b[:min(out["begun"], cap)].copy(), e[:min(out["ended"], cap)].copy(), out

    def draws(self):
        cnt = C.c_uint32()
        self._ok(self.lib.scTickReadDraws(self.ctx, None, 0, C.byref(cnt)), "scTickReadDraws")
        buf = (capi.DrawItem * max(cnt.value, 1))()
        if cnt.value:
            self._ok(self.lib.scTickReadDraws(self.ctx, buf, cnt.value, C.byref(cnt)), "scTickReadDraws")
        n = cnt.value
        a = np.frombuffer(buf, dtype=np.uint8, count=80 * n).reshape(n, 80) if n else np.zeros((0, 80), np.uint8)
        idx = a[:, 0:4].copy().view(np.uint32).ravel()
        mesh = a[:, 4:8].copy().view(np.uint32).ravel()
        mat = a[:, 8:12].copy().view(np.uint32).ravel()
        model = a[:, 16:80].copy().view(np.float32).reshape(n, 16)
        return idx, mesh, mat, model
