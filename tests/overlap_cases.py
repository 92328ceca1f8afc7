"""Cases of the overlap-query tests, shared by the GPU suite (tests/test_gpu_overlaps.py) and its CPU twin (tests/test_overlaps_cpu.py,
which asserts without a GPU that every case is what it claims).  Tiny worlds on a 4 x 4 grid of 64 m sectors, like
tests/ray_walk_cases.py.  Inputs only: no GPU, no kernel logic; every expected answer comes from tests/overlap_ref.py.
The builders are cached: what they return is shared between tests and must be left unchanged."""
import functools

import numpy as np

from tests import collider_ref as cr, overlap_ref as ref, pair_shapes_cases as G, ray_walk_cases as rc

F = np.float32
U = np.uint32
ALL = 0xFFFFFFFF
ORIGIN = (0, 0)                 # the tile covers [0, 256) x [0, 256); the bin grid has a ring of one sector around it
TYPES = (cr.BOX, cr.SPHERE, cr.CAPSULE)
KINDS = ("axis", "turned")      # a volume's matrix: a translation, or a rotation times a non-uniform scale
PER_CELL = 24
TABLE_MAX_HITS = 128            # id slots per volume of the table: its fullest answer fits
QUERY_COUNTS = rc.BATCH_SIZES   # 1, 3, 4, 5, 4 097: a workgroup holds four waves, one volume each
# (chosen here on the CPU: tests/test_overlaps_cpu.py asserts what the GPU tests count on, and that the fp32 witness alone stays within
#  the cap of pairs near contact)
MIXED_SEED, VOLUME_SEED, MIXED_N = 501, 502, 500


def trs(pos, rot=None, scale=None):
    """[k, 16] column-major fp32 matrices T * Rz * Ry * Rx * S, formed in float64: the columns are orthogonal up to the last rounding"""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    k = len(pos)
    rot = np.zeros((k, 3)) if rot is None else np.asarray(rot, np.float64).reshape(k, 3)
    scale = np.ones((k, 3)) if scale is None else np.asarray(scale, np.float64).reshape(k, 3)
    out = np.zeros((k, 4, 4))
    for i in range(k):
        cx, cy, cz = np.cos(rot[i]); sx, sy, sz = np.sin(rot[i])
        rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        out[i, :3, :3] = (rz @ ry @ rx) * scale[i][None, :]
        out[i, :3, 3] = pos[i]
        out[i, 3, 3] = 1.0
    return np.ascontiguousarray(out.transpose(0, 2, 1).reshape(k, 16), F)       # m[c * 4 + r]


def box_volumes(lo, hi, mask=None, skip=None):
    """axis-aligned BOX volumes whose box is [lo, hi] to the bit (asserted): centre and half extents through an identity matrix"""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    k = len(lo)
    c, h = rc.as_box_colliders(lo, hi)
    vol = ref.volumes(np.full(k, cr.BOX, np.uint8), trs(c), h, np.zeros(k, F), np.zeros(k, F),
                      np.full(k, ALL, U) if mask is None else mask, skip)
    mn, mx = ref.volume_boxes(vol)
    assert np.array_equal(mn.view(U), lo.view(U)) and np.array_equal(mx.view(U), hi.view(U))
    return vol


# ---- (a) the mixed world and the table of volumes --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_world():
    """(world, colliders): 500 roots over the middle of the tile, yaw, pitch and roll random, scales non-uniform, every collider type --
    a few BOUNDS proxies and a few without a proxy among them --, sizes of 0.8 .. 3.5 m"""
    rng = np.random.default_rng(MIXED_SEED)
    n = MIXED_N
    pos = np.stack([rng.uniform(30, 226, n), rng.uniform(-3, 3, n), rng.uniform(30, 226, n)], axis=1).astype(F)
    w = G.flat_world(pos, rng.uniform(-np.pi, np.pi, (n, 3)).astype(F), rng.uniform(1.0, 1.3, (n, 3)).astype(F), origin=ORIGIN)
    w.bmin[:], w.bmax[:] = F(-1.0), F(1.0)
    col = cr.Colliders(n)
    col.type[:] = rng.choice(np.arange(5, dtype=np.uint8), n, p=(0.08, 0.04, 0.3, 0.3, 0.28))
    col.he[:] = rng.uniform(0.8, 3.5, (n, 3)).astype(F)
    col.radius[:] = rng.uniform(0.8, 2.5, n).astype(F)
    col.hh[:] = rng.uniform(-0.5, 2.5, n).astype(F)
    return w, col


@functools.lru_cache(maxsize=None)
def volume_table():
    """(volumes, cell per volume): PER_CELL volumes per cell (type, kind) of TYPES x KINDS, 16 .. 70 m across, over the mixed world -- the boxes are slabs a metre or two
    thick, so that their long edges, where a box answer and a shape answer part, run through the crowd; every
    fifth one asks for group bit 1 only (no entity has it: an empty answer), every seventh skips the entity nearest to its centre"""
    rng = np.random.default_rng(VOLUME_SEED)
    typ, m, he, rad, hh, cell = [], [], [], [], [], []
    for ti, t in enumerate(TYPES):
        for ki, kind in enumerate(KINDS):
            k = PER_CELL
            pos = np.stack([rng.uniform(40, 216, k), rng.uniform(-2, 2, k), rng.uniform(40, 216, k)], axis=1)
            turned = kind == "turned"
            m.append(trs(pos, rng.uniform(-np.pi, np.pi, (k, 3)) if turned else None, rng.uniform(0.7, 1.6, (k, 3)) if turned else None))
            typ.append(np.full(k, t, np.uint8)); he.append(rng.uniform(14.0, 34.0, (k, 3)) * [1.0, 0.04, 1.0]); rad.append(rng.uniform(8.0, 16.0, k))
            hh.append(rng.uniform(-2.0, 12.0, k)); cell.append(np.full(k, ti * len(KINDS) + ki))
    k = len(TYPES) * len(KINDS) * PER_CELL
    mask = np.where(np.arange(k) % 5 == 4, 2, ALL).astype(U)
    m = np.concatenate(m)
    # (the entity nearest to the volume's centre: an answer but for the skip)
    wpos = mixed_world()[0].pos
    nearest = np.argmin(((wpos[None, :, [0, 2]] - m[:, None, [12, 14]]) ** 2).sum(axis=2), axis=1)
    skip = np.where(np.arange(k) % 7 == 3, nearest, ref.NO_SKIP).astype(U)
    return ref.volumes(np.concatenate(typ), m, np.concatenate(he), np.concatenate(rad), np.concatenate(hh), mask, skip), np.concatenate(cell)


@functools.lru_cache(maxsize=None)
def odd_volumes():
    """(volumes, names): a BOX volume whose matrix has a zero column (degenerate: box answers in EXACT mode), a big one of the same kind, and
    a SPHERE of radius 0 under a scale of 1e20 -- every input finite, the squared column norms infinite, pad = 0 * inf: a NaN box"""
    m = np.concatenate([trs([[100, 0, 100]], None, [[1, 1, 0]]), trs([[128, 0, 128]], [[0.3, 0.4, 0.5]], [[1, 0, 1]]),
                        trs([[128, 0, 128]], None, [[1e20, 1e20, 1e20]])])
    vol = ref.volumes([cr.BOX, cr.BOX, cr.SPHERE], m, [[12, 6, 12], [90, 10, 90], [1, 1, 1]], [1, 1, 0], [0, 0, 0], np.full(3, ALL, U))
    return vol, ("zero column", "zero column, large", "nan box")


# ---- (b) boxes in two and four sectors -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def straddle_case():
    """(world, volumes, expected entity sets): box 0 lies across x = 64 (two sectors), box 1 across z = 128 (two), box 2 across the corner
    (128, 64) (four), box 3 in one sector.  Volumes cover one, some and all of the copies of each."""
    mn = F([[60, 0, 10], [20, 0, 124], [124, 0, 60], [200, 0, 200]])
    mx = F([[68, 4, 14], [24, 4, 132], [132, 4, 68], [204, 4, 204]])
    lo = F([[55, 0, 8], [65, 0, 8], [55, 0, 8], [18, 0, 120], [18, 0, 129], [18, 0, 100],
            [120, 0, 56], [129, 0, 56], [120, 0, 65], [129, 0, 65], [120, 0, 56], [126, 0, 56], [100, 0, 40], [-60, -5, -60]])
    hi = F([[62, 4, 16], [70, 4, 16], [70, 4, 16], [26, 4, 126], [26, 4, 134], [26, 4, 140],
            [126, 4, 62], [134, 4, 62], [126, 4, 70], [134, 4, 70], [134, 4, 62], [130, 4, 70], [160, 4, 90], [316, 9, 316]])
    want = [[0], [0], [0], [1], [1], [1], [2], [2], [2], [2], [2], [2], [2], [0, 1, 2, 3]]
    return rc.box_world(mn, mx, ORIGIN), box_volumes(lo, hi), want


# ---- (c) faces on a sector boundary ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_case():
    """(world, volumes, meta): per axis (x, z), side (+, -) and boundary (64, 128, 192) one 2 m box with a face ON the boundary and three
    volumes approaching it from the other side, their face one float short of the plane (a miss), on it (a closed touch: a hit) and one
    float past it (a hit).  meta: dict(box, role) per volume, role 0 / 1 / 2 in that order."""
    mn, mx, centre, half, box, role, faces, axes, signs = [], [], [], [], [], [], [], [], []
    for axis in (0, 2):
        for sign in (+1, -1):
            for bi, plane in enumerate((64.0, 128.0, 192.0)):
                minor = F(20.0 + 70.0 * bi + (8.0 if sign > 0 else 30.0) + (14.0 if axis else 0.0))
                b_lo, b_hi = np.zeros(3, F), np.zeros(3, F)
                b_lo[axis], b_hi[axis] = (F(plane), F(plane + 2.0)) if sign > 0 else (F(plane - 2.0), F(plane))
                b_lo[2 - axis], b_hi[2 - axis] = minor, F(minor + F(2.0))
                b_lo[1], b_hi[1] = F(0.0), F(2.0)
                e = len(mn)
                mn.append(b_lo); mx.append(b_hi)
                for r, face in enumerate((rc.down(F(plane)), F(plane), rc.up(F(plane))) if sign > 0 else (rc.up(F(plane)), F(plane), rc.down(F(plane)))):
                    # the volume's near face is fl(c -+ h): with c two metres behind the face, h = |c - face| is exact and so is the face
                    c, h = ((b_lo + b_hi) * F(0.5)).astype(F), F([1.0, 1.0, 1.0])
                    c[axis] = F(F(face) - F(sign * 2.0))
                    h[axis] = F(abs(c[axis] - F(face)))
                    centre.append(c); half.append(h); box.append(e); role.append(r); faces.append(F(face)); axes.append(axis); signs.append(sign)
    k = len(centre)
    vol = ref.volumes(np.full(k, cr.BOX, np.uint8), trs(np.stack(centre)), np.stack(half), np.zeros(k, F), np.zeros(k, F), np.full(k, ALL, U))
    meta = dict(box=np.array(box), role=np.array(role), face=np.array(faces, F), axis=np.array(axes), sign=np.array(signs))
    return rc.box_world(np.stack(mn), np.stack(mx), ORIGIN), vol, meta


# ---- (d) the crowded sector ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crowded_volumes():
    """over rc.crowded_world(): a volume inside the crowded sector, one over it and its neighbours, a sphere and a capsule in it"""
    box = box_volumes(F([[70, -1, 70], [-4, -10, -4]]), F([[86, 3, 86], [196, 10, 196]]))
    rnd = ref.volumes([cr.SPHERE, cr.CAPSULE], trs([[90, 0.5, 90], [100, 0.5, 80]], [[0, 0, 0], [0.2, 0.1, 1.2]]), np.ones((2, 3)), [9.0, 3.0], [0.0, 12.0],
                      np.full(2, ALL, U))
    return {k: np.concatenate([box[k], rnd[k]]) for k in box if k != "skip"} | {"skip": None}


# ---- (e) the big list ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_case():
    """(world, volumes): a plate over three sectors and a box outside the grid (both in the big list), three small boxes; a volume larger
    than the grid, one wholly outside it on the far box, one outside it on nothing, one on the plate alone"""
    mn = F([[10, -1, 10], [-500, 0, -500], [30, 0, 30], [130, 0, 130], [250, 0, 250]])
    mx = F([[200, 0, 40], [-498, 2, -498], [32, 2, 32], [132, 2, 132], [252, 2, 252]])
    lo = F([[-1000, -1000, -1000], [-504, -1, -504], [600, 0, 600], [150, -2, 20]])
    hi = F([[1000, 1000, 1000], [-499, 1, -499], [610, 4, 610], [160, 2, 30]])
    return rc.box_world(mn, mx, ORIGIN), box_volumes(lo, hi)


# ---- (f) mask, skip_id, truncation -----------------------------------------------------------------------------------------------
LINE = 70
MAX_HITS = (1, 3, 64)


@functools.lru_cache(maxsize=None)
def line_world():
    """70 half-metre boxes 2 m apart along x from 20 m (three sectors), box i in group 1 << (i % 3)"""
    i = np.arange(LINE)
    mn = np.stack([20.0 + 2.0 * i, np.zeros(LINE), np.full(LINE, 30.0)], axis=1).astype(F)
    return rc.box_world(mn, (mn + F(0.5)).astype(F), ORIGIN, group=(1 << (i % 3)).astype(U))


def line_volumes(max_hits):
    """volumes over the first 0, max_hits and max_hits + 1 boxes of the line"""
    m = np.array([0, max_hits, max_hits + 1])
    lo = np.stack([np.full(3, 19.0), np.full(3, -1.0), np.full(3, 29.0)], axis=1).astype(F)
    hi = np.stack([np.where(m > 0, 20.0 + 2.0 * (m - 1) + 0.25, 19.5), np.full(3, 1.0), np.full(3, 31.0)], axis=1).astype(F)
    return box_volumes(lo, hi), m


def filter_volumes():
    """the whole line asked for with one group bit each, with two of them, and with box 3 (and an id of another rank) skipped"""
    lo, hi = np.tile(F([19, -1, 29]), (5, 1)), np.tile(F([170, 1, 31]), (5, 1))
    return box_volumes(lo, hi, mask=np.array([1, 2, 4, 5, ALL], U), skip=np.array([ref.NO_SKIP, ref.NO_SKIP, 2, 3, 3 | (1 << 24)], U))


# ---- (h) a world that cannot pair ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quiet_world():
    """the mixed world's entities in group 1 with mask 2: no two of them pass the filter, a query for group 1 meets them all the same"""
    w, col = mixed_world()
    import copy
    w = copy.deepcopy(w)
    w.group[:], w.mask[:] = 1, 2
    return w, col


def tiled(vol, count):
    idx = np.arange(count) % len(vol["type"])
    return ref.take(vol, idx), idx
