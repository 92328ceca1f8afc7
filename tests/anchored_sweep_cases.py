"""Cases of the entity-anchored capsule sweeps, shared by the GPU suite (tests/test_gpu_anchored_sweeps.py) and its CPU twin
(tests/test_anchored_sweeps_cpu.py, which proves without a GPU that every case is what it claims).  Inputs only: no GPU, no kernel
logic; every expected answer comes from tests/anchored_sweeps_ref.py.
A sweep set is a dict of arrays (anchor, ls, le, radius, hh, mask, skip_self, end_frame).  The builders are cached: what they return is
shared between tests and must be left unchanged."""
import functools

import numpy as np

from tests import anchored_sweeps_ref as ar, collider_ref as cr, ray_walk_cases as rc, sweep_shapes_cases as sc, trigger_cases as tc

F = np.float32
U = np.uint32
ALL = 0xFFFFFFFF
NONE, DEAD = ar.ANCHOR_NONE, ar.ANCHOR_DEAD
COUNTS = rc.BATCH_SIZES         # 1, 3, 4, 5, 4 097: a workgroup holds four waves, one sweep each; one sweep past 4 096
KEYS = ("anchor", "ls", "le", "radius", "hh", "mask", "skip_self", "end_frame")
CELLS = ("hit", "miss", "starts in overlap", "zero length")
PER_CELL = 8
STATUS_ROWS = 8                 # rows 0 .. 7 of the table: four without an anchor, four that do not resolve to finite numbers
OWN_ROWS = slice(460, 480)      # rows that start at their anchor's origin and see the anchor (skip_self 0)
ZERO_ROWS = slice(480, 500)     # zero-length rows


def sweeps(anchor, ls, le, radius, hh, mask=None, skip_self=None, end_frame=None):
    an = np.ascontiguousarray(anchor, U).reshape(-1)
    k = len(an)
    full = lambda x, t: np.broadcast_to(np.asarray(x, t), (k,)).copy()          # noqa: E731
    return {"anchor": an, "ls": np.ascontiguousarray(ls, F).reshape(k, 3).copy(), "le": np.ascontiguousarray(le, F).reshape(k, 3).copy(),
            "radius": full(radius, F), "hh": full(hh, F), "mask": full(ALL if mask is None else mask, U),
            "skip_self": full(1 if skip_self is None else skip_self, np.uint8), "end_frame": full(0 if end_frame is None else end_frame, np.uint8)}


def args(q):
    """in the order of WorldTick.anchored_sweeps"""
    return tuple(q[k] for k in KEYS)


def take(q, idx):
    return {k: q[k][idx].copy() for k in KEYS}


def tiled(q, count):
    """the table repeated (and cut) to `count` sweeps, begun behind its status rows so that the smallest counts are sweeps that are answered"""
    idx = (np.arange(count) + STATUS_ROWS) % len(q["anchor"])
    return take(q, idx), idx


def unanchored(a, b, radius, hh, mask):
    """world-space sweeps (scTickSetSweepQueries' arrays) as anchored sweeps without an anchor, end_frame 0"""
    return sweeps(np.full(len(np.asarray(a).reshape(-1, 3)), NONE, U), a, b, radius, hh, mask)


def witness(oracle, m, mn, mx, group, mask, col, q, mode=ar.AABB):
    return ar.sweep(oracle, m, mn, mx, group, mask, col, q["anchor"], q["ls"], q["le"], q["radius"], q["hh"], q["mask"], q["skip_self"],
                    q["end_frame"], mode)


def cell_of(hits, segments):
    """which cell of CELLS every answered sweep falls into (-1: not answered), from the witness's answer alone"""
    s, e = segments
    with np.errstate(all="ignore"):
        d = e - s
        len_sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    zero = len_sq <= F(1e-6)
    hit = hits["hit"] == 1
    out = np.select([hits["pad"] != 0, zero, hit & (hits["travel"] == 0), hit], [-1, 3, 2, 0], 1)
    return out


def to_local(m16, points):
    """points [k, 3] (float64) in the frames m16 [k, 16]: the float64 inverse, rounded to fp32"""
    M = np.ascontiguousarray(m16, F).reshape(-1, 4, 4).transpose(0, 2, 1).astype(np.float64)
    return np.einsum("kij,kj->ki", np.linalg.inv(M[:, :3, :3]), np.asarray(points, np.float64) - M[:, :3, 3]).astype(F)


# ---- the table: 500 sweeps across the 1 200 entities of the exact sweeps' world ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(oracle):
    """(world, colliders, sweeps): tests/sweep_shapes_cases.py's world_case -- 1 200 entities, depth <= 2, sheared frames -- and its 500
    world-space sweeps taken into the frames of random entities (one in ten stays world space): even rows end at a local point, odd rows
    at a world offset.  Rows 0 .. 7 have each status but 0, OWN_ROWS start at their anchor's own origin and see it, ZERO_ROWS are zero
    length."""
    w, col, (a, b, radius, hh, mask, _) = sc.world_case(oracle)
    m, mn, mx = tc.state(oracle, w, col)
    k = len(a)
    rng = np.random.default_rng(3801)
    anchor = rng.integers(0, w.n, k).astype(U)
    # OWN_ROWS: entities with a shape of their own whose origin no box of a lower id holds -- selected by the witness, in both modes (at
    # t = 0 the lower id wins a tie) -- so that the anchor itself is the answer where it is not skipped
    typed = np.flatnonzero((col.type >= cr.BOX) & ((w.group & 0xFFFF) != 0) & ((w.mask & 0xFFFF) != 0))
    probe = sweeps(typed, np.zeros((len(typed), 3), F), F([[0, 0, 2]] * len(typed)), 0.3, 0.6, skip_self=0, end_frame=1)
    seen = [witness(oracle, m, mn, mx, w.group, w.mask, col, probe, mode)[0]["id"] == typed for mode in (ar.AABB, ar.EXACT)]
    anchor[OWN_ROWS] = rng.choice(typed[seen[0] & seen[1]], OWN_ROWS.stop - OWN_ROWS.start, replace=False)
    M = m.reshape(-1, 4, 4).transpose(0, 2, 1).astype(np.float64)
    free = (np.abs(np.linalg.det(M[anchor, :3, :3])) < 1e-3) | (rng.random(k) < 0.1)
    free[OWN_ROWS] = False
    frame = (np.arange(k) % 2).astype(np.uint8)
    skip = (rng.random(k) < 0.7).astype(np.uint8)
    mask = mask.copy()
    a, b = a.copy(), b.copy()
    a[OWN_ROWS] = m[anchor[OWN_ROWS], 12:15]
    b[OWN_ROWS] = a[OWN_ROWS] + rng.normal(size=(20, 3)).astype(F) * F(3.0)
    skip[OWN_ROWS], mask[OWN_ROWS] = 0, ALL
    radius, hh = radius.copy(), hh.copy()
    radius[OWN_ROWS], hh[OWN_ROWS] = 0.3, 0.6                                  # (the sweeper the selection above was made with)
    ls, le = a.copy(), b.copy()
    at = np.flatnonzero(~free)
    ls[at], le[at] = to_local(m[anchor[at]], a[at]), to_local(m[anchor[at]], b[at])
    ls[OWN_ROWS] = 0
    off = frame == ar.END_WORLD_OFFSET
    le[off] = b[off] - a[off]
    anchor[free] = NONE
    zero = np.arange(ZERO_ROWS.start, ZERO_ROWS.stop)
    le[zero] = np.where(off[zero][:, None], F(0.0), ls[zero])
    # the statuses: no anchor (the count, beyond it, dead, the largest index); not finite (the squared length of a local end far away, an
    # unanchored offset that overflows, an unanchored segment whose squared length overflows, a world offset whose squared length does)
    anchor[0:4] = [w.n, w.n + 7, DEAD, 0x00FFFFFF]
    anchor[4:8] = [anchor[8] if anchor[8] != NONE else 0, NONE, NONE, anchor[9] if anchor[9] != NONE else 1]
    frame[4:8] = [0, 1, 0, 1]
    ls[4:8] = [[0, 0, 0], [3e38, 0, 0], [-2e19, 0, 0], [0, 0, 0]]
    le[4:8] = [[1e30, 1e30, 1e30], [3e38, 0, 0], [2e19, 0, 0], [3e38, 0, 0]]
    return w, col, sweeps(anchor, ls, le, radius, hh, mask, skip, frame)


@functools.lru_cache(maxsize=None)
def table_state(oracle):
    """(matrices, box min, box max) of the table's world as the transform stage leaves it"""
    w, col, _ = table(oracle)
    return tc.state(oracle, w, col)


@functools.lru_cache(maxsize=None)
def table_answers(oracle, mode):
    w, col, q = table(oracle)
    m, mn, mx = table_state(oracle)
    return witness(oracle, m, mn, mx, w.group, w.mask, col, q, mode)


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
WALL_TRAVEL = 19.0


def yaw_wall_case(shift=0.0):
    """(matrices, colliders, sweeps, target): entity 0, a half-metre box at (100, 0, 100 - shift) yawed by 90 degrees, carries a capsule
    (radius 0.5, half height 0.5) that sweeps 32 m along its local +x: world -z.  Entity 1 is a wall, half extents (20, 3, 0.5), at
    (100, 0, 80): its face lies at z = 80.5, the capsule's centre stops at z = 81, so the travel is 19 - shift."""
    m = sc.matrices_of([[100, 0, 100 - shift], [100, 0, 80]], [[0, np.pi / 2, 0], [0, 0, 0]])
    col = sc.colliders(2, [cr.BOX, cr.BOX], he=[[0.5, 0.5, 0.5], [20, 3, 0.5]], radius=[0.5, 0.5], hh=[0.5, 0.5])
    return m, col, sweeps([0], [[0, 0, 0]], [[32, 0, 0]], 0.5, 0.5), 1


PROBE_HEIGHT, PROBE_RADIUS, PROBE_HH = 3.0, 0.25, 0.5


def tilt_probe_case():
    """(matrices, colliders, sweeps, target): entity 0, a chassis at (60, 3, 60) rolled by 30 degrees about z, probes 4 m straight DOWN
    (end_frame 1: a world offset) with a capsule of radius 0.25, half height 0.5; entity 1 is a slab, half extents (10, 0.5, 10), whose top
    face lies at y = 0.  The capsule lands at height - (hh + radius) = 2.25.  Sweep 1 is the same numbers in end_frame 0: it follows the
    tilt, 2 m sideways."""
    m = sc.matrices_of([[60, PROBE_HEIGHT, 60], [60, -0.5, 60]], [[0, 0, np.pi / 6], [0, 0, 0]])
    col = sc.colliders(2, [cr.BOX, cr.BOX], he=[[1, 0.25, 2], [10, 0.5, 10]], radius=[0.5, 0.5], hh=[0.5, 0.5])
    return m, col, sweeps([0, 0], [[0, 0, 0]] * 2, [[0, -4, 0]] * 2, PROBE_RADIUS, PROBE_HH, end_frame=[1, 0]), 1


# ---- the sector walk at its edges ----------------------------------------------------------------------------------------------------
def walk_rows(kind, where):
    """(world, [a, b, radius, hh, mask], role) of tests/ray_walk_cases.py: role 0 is a miss, 1 and 2 are hits.  edge: a grown box met at
    travel == far behind a sector boundary and its neighbour one ulp short; zero: overlap tests on a grown face; crowded: 90 boxes in
    one sector, 26 of them in the overflow list (every sweep hits)"""
    if kind == "crowded":
        q = rc.crowded_sweeps()
        return rc.crowded_world()[0], q, np.ones(len(q[0]), int)
    w, _, q, meta = (rc.sweep_batch if kind == "edge" else rc.zero_batch)(where)
    return w, q, meta["role"]


def walk_sets(w, q, seed=7):
    """The sweep rows of tests/ray_walk_cases.py (a, b, radius, hh, mask) as anchored sets: (world-space set, set in the frames of
    translated anchors, the world with those anchors, kept rows).  An anchor's matrix is the identity plus a translation T, so the
    header's formula gives back a point p when fl(fl(p - T) + T) == p; a row is kept when a T of the set does that for both its ends
    (asserted by tests/test_anchored_sweeps_cpu.py on the witness).  Anchor t is entity w.n + t of rc.box_world(..., anchors=T)."""
    a, b, r, hh, mask = q
    rng = np.random.default_rng(seed)
    T = (rng.integers(-64, 64, (7, 3)) * 0.25).astype(F)
    back = lambda l, t: ((F(1.0) * l + F(0.0) * l[[1, 2, 0]]) + F(0.0) * l[[2, 0, 1]]) + t           # noqa: E731
    keep, anchor, la, lb = [], [], [], []
    for i in range(len(a)):
        for t in range(len(T)):
            l1, l2 = (a[i] - T[t]).astype(F), (b[i] - T[t]).astype(F)
            if np.array_equal(back(l1, T[t]).view(U), a[i].view(U)) and np.array_equal(back(l2, T[t]).view(U), b[i].view(U)):
                keep.append(i); anchor.append(w.n + t); la.append(l1); lb.append(l2)
                break
    keep = np.array(keep, np.int64)
    moved = sweeps(anchor, np.stack(la), np.stack(lb), r[keep], hh[keep], mask[keep], skip_self=0)
    world = rc.box_world(w.bmin, w.bmax, w.origin, group=w.group, anchors=T)
    return unanchored(a, b, r, hh, mask), moved, world, keep


# ---- residency -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def residency_case():
    """(world, sweeps, removal): tests/trigger_cases.py's residency world -- 12 boxes on a line, four carriers beside it.  Sweeps ride on
    12, 13, 15, on 15 again seeing its carrier, on 14, and one is world space; each goes 6 m across the line.  Removing [13, 2] kills
    13's sweep and relocates 15 -> 13 and 14 -> 2."""
    w, _, removal = tc.residency_case()
    q = sweeps([12, 13, 15, 15, 14, NONE], [[0, 0, 0]] * 5 + [[30, 0, 36]], [[0, 0, -6]] * 5 + [[30, 0, 28]], 0.3, 0.4,
               skip_self=[1, 1, 1, 0, 1, 1], end_frame=[0, 1, 0, 0, 1, 0])
    return w, q, removal


def renamed(q, names):
    """the set after a removal: names maps an old index to the new one or None"""
    an = U([a if a == NONE else (DEAD if names[int(a)] is None else names[int(a)]) for a in q["anchor"]])
    return dict(q, anchor=an)
