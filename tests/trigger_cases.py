"""Cases of the trigger-volume tests, shared by the GPU suite (tests/test_gpu_triggers.py) and its CPU twin (tests/test_triggers_cpu.py,
which asserts without a GPU that every case is what it claims).  Tiny worlds on the 4 x 4 grid of 64 m sectors of tests/overlap_cases.py.
Inputs only: no GPU, no kernel logic; every expected answer comes from tests/trigger_ref.py.
The builders are cached: what they return is shared between tests and must be left unchanged."""
import functools

import numpy as np

from sc_gameengine_amd import synth_world as sw
from tests import collider_ref as cr, overlap_cases as oc, overlap_ref as ref, ray_walk_cases as rc, trigger_ref as tr, worlds

F = np.float32
U = np.uint32
ALL = 0xFFFFFFFF
NONE = tr.NONE
ORIGIN = oc.ORIGIN
VOLUME_COUNTS = rc.BATCH_SIZES  # 1, 3, 4, 5, 4 097: a workgroup holds four waves, one volume each


def world(pos, rot=None, scale=None, parent=None, half=1.0, group=None, mask=None):
    """entities with a Bounds box of +-half around their origin, group 1, mask all, on the tile [0, 256) x [0, 256)"""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    n = len(pos)
    half = np.broadcast_to(np.asarray(half, F).reshape(-1, 1), (n, 3)).astype(F)
    one = np.ones(n, np.uint8)
    return sw.SynthWorld(pos=pos.copy(), rot=np.zeros((n, 3), F) if rot is None else np.ascontiguousarray(rot, F).reshape(n, 3).copy(),
                         scale=np.ones((n, 3), F) if scale is None else np.ascontiguousarray(scale, F).reshape(n, 3).copy(),
                         parent=np.full(n, -1, np.int32) if parent is None else np.ascontiguousarray(parent, np.int32).copy(),
                         bmin=(-half).astype(F), bmax=half.copy(), has_mesh=one.copy(), has_bounds=one.copy(), mesh=np.zeros(n, U),
                         material=np.zeros(n, U), group=np.ones(n, U) if group is None else np.ascontiguousarray(group, U).copy(),
                         mask=np.full(n, ALL, U) if mask is None else np.ascontiguousarray(mask, U).copy(),
                         sector_of=np.zeros((n, 2), np.int32), origin=ORIGIN, sectors=rc.SECTORS)


def state(oracle, w, col=None):
    """(world matrices [n, 16], box min, box max) of a world as the oracle's transform system leaves it; col: typed colliders' boxes"""
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    m = ow.world_matrices()[:w.n].copy()
    if col is None:
        mn, mx = ow.world_aabbs()
        mn, mx = mn[:w.n].copy(), mx[:w.n].copy()
    else:
        mn, mx = col.witness(ow, w.n)
    ow.close()
    return m, mn, mx


def unanchored(vol):
    """an overlap set (tests/overlap_ref.py) as world-space trigger volumes"""
    k = len(vol["type"])
    return tr.volumes(np.full(k, NONE, U), vol["type"], vol["m16"], vol["he"], vol["radius"], vol["hh"], vol["mask"])


def concat(*vols):
    return {k: np.concatenate([v[k] for v in vols]) if vols[0][k] is not None else None for k in vols[0]}


# ---- 1. resolve: a moving hierarchy ---------------------------------------------------------------------------------------------
HIERARCHY_TICKS, HIERARCHY_NUDGE = 4, 1.75


@functools.lru_cache(maxsize=None)
def hierarchy_case():
    """(world, volumes): 60 unrotated boxes, then a root, its child and its grandchild (indices 60, 61, 62), the parents rotated and
    non-uniformly scaled.  Two volumes ride on each of the three -- one with a turned, scaled local matrix --, two are world space."""
    rng = np.random.default_rng(611)
    pos = np.concatenate([np.stack([rng.uniform(60, 180, 60), rng.uniform(-2, 2, 60), rng.uniform(60, 180, 60)], axis=1),
                          [[100, 0, 100], [6, 0.5, 3], [-4, 1, 5]]])
    rot = np.concatenate([np.zeros((60, 3)), [[0.3, 0.7, -0.2], [0.1, -0.4, 0.5], [0.2, 0.2, 0.2]]])
    scale = np.concatenate([np.ones((60, 3)), [[1.5, 0.8, 1.2], [0.7, 1.3, 1.1], [1, 1, 1]]])
    parent = np.concatenate([np.full(60, -1), [-1, 60, 61]])
    w = world(pos, rot, scale, parent)
    anchor = U([60, 60, 61, 61, 62, 62, NONE, NONE])
    local = np.concatenate([oc.trs([[0, 0, 0]]), oc.trs([[5, 0, -3]], [[0.4, -0.3, 0.9]], [[1.2, 0.7, 1.0]]),
                            oc.trs([[1, 0, 2]]), oc.trs([[-3, 1, 2]], [[-0.5, 0.2, 0.1]], [[0.8, 1.1, 1.4]]),
                            oc.trs([[0, 0, 0]]), oc.trs([[2, -1, 4]], [[0.1, 1.0, -0.7]], [[1.0, 1.3, 0.9]]),
                            oc.trs([[128, 0, 128]]), oc.trs([[110, 0, 120]], [[0.2, 0.5, 0.3]], [[1.1, 0.9, 1.3]])])
    typ = np.array([cr.BOX, cr.SPHERE, cr.CAPSULE, cr.BOX, cr.SPHERE, cr.BOX, cr.BOX, cr.CAPSULE], np.uint8)
    he = np.tile(F([18, 5, 18]), (8, 1))
    vol = tr.volumes(anchor, typ, local, he, np.full(8, 14.0, F), np.full(8, 10.0, F), np.full(8, ALL, U))
    return w, vol


# ---- 2. the sequence ------------------------------------------------------------------------------------------------------------
SEQ_N, SEQ_TICKS, SEQ_UNFLAGGED, SEQ_STILL = 200, 16, (5, 6), 9
SEQ_MAX_MEMBERS, SEQ_MAX_EVENTS = 64, 512
SEQ_MOVERS = 50


@functools.lru_cache(maxsize=None)
def sequence_world():
    """(world, colliders, steps): 200 roots, every collider type, yaw, pitch and roll random, scales non-uniform; the first 50 move by up to
    4 m a tick; steps[k] are the positions of tick k (tick SEQ_STILL repeats the tick before it: nothing moves)"""
    rng = np.random.default_rng(621)
    n = SEQ_N
    pos = np.stack([rng.uniform(40, 216, n), rng.uniform(-2, 2, n), rng.uniform(40, 216, n)], axis=1).astype(F)
    w = world(pos, rng.uniform(-np.pi, np.pi, (n, 3)), rng.uniform(1.0, 1.3, (n, 3)))
    col = cr.Colliders(n)
    col.type[:] = rng.choice(np.arange(5, dtype=np.uint8), n, p=(0.1, 0.04, 0.3, 0.28, 0.28))
    col.he[:] = rng.uniform(0.8, 3.0, (n, 3)).astype(F)
    col.radius[:] = rng.uniform(0.8, 2.5, n).astype(F)
    col.hh[:] = np.maximum(rng.uniform(-0.5, 2.5, n), 0.0).astype(F)
    vel = np.zeros((n, 3), F)
    vel[:SEQ_MOVERS, [0, 2]] = rng.uniform(-4, 4, (SEQ_MOVERS, 2))
    steps, p = [], pos.copy()
    for k in range(SEQ_TICKS):
        if k and k != SEQ_STILL:
            p = (p + vel).astype(F)
            out = (p[:, [0, 2]] < 20) | (p[:, [0, 2]] > 236)
            vel[:, [0, 2]] = np.where(out, -vel[:, [0, 2]], vel[:, [0, 2]])
        steps.append(p.copy())
    return w, col, steps


@functools.lru_cache(maxsize=None)
def sequence_volumes(turned):
    """14 volumes on movers (boxes, spheres, capsules; every third one sees its carrier) and 10 in world space, 24 .. 50 m across;
    turned: local matrices rotated and non-uniformly scaled (the EXACT run), else translations"""
    rng = np.random.default_rng(622 + int(turned))
    k_a, k_w = 14, 10
    k = k_a + k_w
    anchor = np.concatenate([rng.choice(SEQ_MOVERS, k_a, replace=False), np.full(k_w, NONE)]).astype(U)
    lpos = np.concatenate([rng.uniform(-4, 4, (k_a, 3)) * [1, 0.2, 1], np.stack([rng.uniform(60, 196, k_w), rng.uniform(-1, 1, k_w), rng.uniform(60, 196, k_w)], axis=1)])
    local = oc.trs(lpos, rng.uniform(-np.pi, np.pi, (k, 3)) if turned else None, rng.uniform(0.8, 1.3, (k, 3)) if turned else None)
    typ = np.array([cr.BOX, cr.SPHERE, cr.CAPSULE], np.uint8)[np.arange(k) % 3]
    he = rng.uniform(12, 25, (k, 3)) * [1.0, 0.3, 1.0]
    return tr.volumes(anchor, typ, local, he, rng.uniform(10, 18, k), rng.uniform(0, 10, k), np.full(k, ALL, U), (np.arange(k) % 3 != 2).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def sequence_sets(oracle, shapes):
    """per tick (member sets, resolved matrices) of the witness; computed once per mode and shared"""
    w, col, steps = sequence_world()
    vol = sequence_volumes(bool(shapes))
    ow = worlds.oracle_world(oracle, w, camera=False)
    ents = ow.dense_entities()
    out = []
    for k in range(SEQ_TICKS):
        ow.set_local_positions(ents, steps[k])
        ow.transform_system()
        m = ow.world_matrices()[:w.n].copy()
        mn, mx = col.witness(ow, w.n)
        sets, m16, _ = tr.members(oracle, mn, mx, w.group, w.mask, m, col, vol, w.n, shapes)
        out.append((sets, m16, m))
    ow.close()
    return out


# ---- 3. row edges ---------------------------------------------------------------------------------------------------------------
EDGE_MAX_MEMBERS = 66
EDGE_COUNTS = (0, 1, 63, 64, 65, EDGE_MAX_MEMBERS, EDGE_MAX_MEMBERS + 1)
EDGE_NEXT = (0, 3, 63, 64, 64, EDGE_MAX_MEMBERS, 10)         # the next tick: the overflowing volume fits, one grows, one shrinks


def line_volumes(counts):
    """world-space volumes over the first counts[v] boxes of oc.line_world()"""
    m = np.asarray(counts)
    k = len(m)
    lo = np.stack([np.full(k, 19.0), np.full(k, -1.0), np.full(k, 29.0)], axis=1).astype(F)
    hi = np.stack([np.where(m > 0, 20.0 + 2.0 * (m - 1) + 0.25, 19.5), np.full(k, 1.0), np.full(k, 31.0)], axis=1).astype(F)
    return unanchored(oc.box_volumes(lo, hi))


def span_volumes(first, last):
    """world-space volumes over the boxes first[v] .. last[v] of oc.line_world()"""
    first, last = np.asarray(first), np.asarray(last)
    k = len(first)
    lo = np.stack([20.0 + 2.0 * first - 0.5, np.full(k, -1.0), np.full(k, 29.0)], axis=1).astype(F)
    hi = np.stack([20.0 + 2.0 * last + 0.25, np.full(k, 1.0), np.full(k, 31.0)], axis=1).astype(F)
    return unanchored(oc.box_volumes(lo, hi))


# ---- 4. one entity, one member, whatever record reports it ----------------------------------------------------------------------
STRADDLER, PLATE, SPILLED = 93, 94, 89          # the box across the corner (128, 128); the big-list plate; box (ix 9, iz 8) of the crowd
CORNERS = ((60, 60), (90, 80), (93.5, 90.5), (126, 126), (130, 130), (60, 60))


@functools.lru_cache(maxsize=None)
def reporter_world():
    """rc.crowded_world()'s boxes (90 in one sector: 26 records in the overflow list), a box across the sector corner (128, 128) -- four
    sectors -- and a plate over three sectors (the big list)"""
    cw, _, _ = rc.crowded_world()
    mn = np.concatenate([cw.bmin, F([[124, 0, 124], [10, -1, 200]])])
    mx = np.concatenate([cw.bmax, F([[132, 4, 132], [200, 0, 230]])])
    return rc.box_world(mn, mx, ORIGIN)


def reporter_volume(corner):
    """one world-space box from (corner.x, -2, corner.z) to (250, 8, 250): moving its low corner moves the low corner of every intersection"""
    return unanchored(oc.box_volumes(F([[corner[0], -2, corner[1]]]), F([[250, 8, 250]])))


# ---- 5. the event cap -----------------------------------------------------------------------------------------------------------
CAP_EVENTS = 4


# ---- 6. residency ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def residency_case():
    """(world, volumes, removal): 12 boxes on a line (indices 0 .. 11), four carriers (12 .. 15) with a box of their own beside the line;
    volumes ride on 12, 13, 15, on 15 again seeing its carrier, and one is world space.  Removing [13, 2] (swap-remove, in this order)
    kills 13's volume and relocates 15 -> 13 and 14 -> 2."""
    i = np.arange(12)
    pos = np.concatenate([np.stack([20.0 + 2.0 * i, np.zeros(12), np.full(12, 30.0)], axis=1), [[22, 0, 33], [28, 0, 33], [34, 0, 33], [40, 0, 33]]])
    w = world(pos, half=0.25)
    k = 5
    vol = tr.volumes(U([12, 13, 15, 15, NONE]), np.full(k, cr.BOX, np.uint8), oc.trs(np.concatenate([np.zeros((4, 3)), [[30, 0, 31]]])),
                     np.concatenate([np.tile(F([3.5, 2, 4]), (4, 1)), F([[13, 2, 4]])]), np.zeros(k, F), np.zeros(k, F), np.full(k, ALL, U),
                     np.array([1, 1, 1, 0, 1], np.uint8))
    return w, vol, [13, 2]


def swap_remove(w, idx):
    """(world after removing the entities idx -- dense indices at the time of the call -- one after the other, old index -> new index or
    None) by the pool's swap-remove rule: the last entity moves into the hole"""
    order = list(range(w.n))
    for i in idx:
        at = order.index(i)
        order[at] = order[-1]
        order.pop()
    renamed = {old: (order.index(old) if old in order else None) for old in range(w.n)}
    keep = np.array(order)
    return world(w.pos[keep], half=w.bmax[keep, 0]), renamed


# ---- 9. a world that cannot pair ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quiet_case():
    """the sequence world at tick 0 in group 1 with mask 2 (no two entities pass the filter) and the sequence's translated volumes"""
    import copy
    w, col, _ = sequence_world()
    w = copy.deepcopy(w)
    w.group[:], w.mask[:] = 1, 2
    return w, col, sequence_volumes(False)


def tiled(vol, count):
    idx = np.arange(count) % len(vol["type"])
    return tr.take(vol, idx), idx
