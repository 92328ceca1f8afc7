"""Seeded and constructed cases of the exact shapes for capsule sweeps, shared by the GPU suite (tests/test_gpu_sweep_shapes.py) and its
CPU twin (tests/test_sweep_shapes_cpu.py).  Inputs and witness calls only: no GPU."""
import numpy as np

from tests import collider_ref as cr, sweep_ref, sweep_shapes_ref as ss, worlds
from tests.shape_rays_ref import shape_records

F = np.float32
ALL = 0xFFFFFFFF


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def matrices_of(pos, rot=None, scale=None):
    """column-major fp32 world matrices m[c*4 + r] of roots: R(rot) * diag(scale), translated (orthogonal columns)"""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    k = len(pos)
    rot = np.zeros((k, 3)) if rot is None else np.asarray(rot, np.float64).reshape(k, 3)
    scale = np.ones((k, 3)) if scale is None else np.asarray(scale, np.float64).reshape(k, 3)
    m = np.zeros((k, 16), F)
    for i in range(k):
        M = np.eye(4)
        M[:3, :3] = rotation(*rot[i]) * scale[i][None]
        M[:3, 3] = pos[i]
        m[i] = M.T.reshape(-1)
    return m


def colliders(n, types, he=None, radius=None, hh=None):
    col = cr.Colliders(n)
    col.type[:] = types
    if he is not None:
        col.he[:] = F(he)
    if radius is not None:
        col.radius[:] = F(radius)
    if hh is not None:
        col.hh[:] = np.maximum(F(hh), F(0.0))
    return col


def boxes_of(m, col):
    return cr.typed_boxes(m, col.type, col.he, col.radius, col.hh)


def sweeps_of(start, end, radius, hh, mask=None, skip=None):
    a, b = np.ascontiguousarray(start, F).reshape(-1, 3), np.ascontiguousarray(end, F).reshape(-1, 3)
    k = len(a)
    full = lambda x: np.broadcast_to(np.asarray(x, F), (k,)).copy()             # noqa: E731
    return (a, b, full(radius), full(hh), np.full(k, ALL, np.uint32) if mask is None else np.ascontiguousarray(mask, np.uint32).reshape(k),
            None if skip is None else np.ascontiguousarray(skip, np.uint32).reshape(k))


def witness(m, mn, mx, group, mask, col, q, mode=ss.EXACT, **kw):
    a, b, r, hh, qm, skip = q
    return ss.sweep32(m, mn, mx, group, mask, col, a, b, r, hh, qm, skip_id=skip, mode=mode, **kw)


def ndir_of(q):
    dv, far, moving = sweep_ref.segments(q[0], q[1])
    with np.errstate(all="ignore"):
        nd = np.where(moving[:, None], dv * (F(1.0) / far)[:, None], F(0.0)).astype(F)
    return nd, far


def pair_advance(m, col, e, q, t0=None, **kw):
    """the advancement of sweep k towards entity e[k] alone, from t0 (default 0): advance32's tuple"""
    typ, shp = shape_records(col, len(m))
    nd, far = ndir_of(q)
    k = len(e)
    return ss.advance32(m, typ, shp, np.asarray(e, np.int64), [q[0][:, i] for i in range(3)], [nd[:, i] for i in range(3)], far, q[2],
                        np.maximum(q[3], F(0.0)), np.zeros(k, F) if t0 is None else np.asarray(t0, F), **kw)


# ---- one target per sweep, all three types: the agreement of the two witnesses --------------------------------------
SEEDS = (1, 2, 3)           # (chosen on the CPU: the float64 witness alone leaves out 0, 1 and 0 of 300 as grazing)
SPREAD = 60.0               # targets within +-60 m per axis, sweeps start up to 15 m from them: coordinates below 75 m
PAIRS = 300


def pair_world(seed, k=PAIRS):
    """k targets of random type, rotation and per-axis scale, and one sweep each: from 4 .. 15 m away towards a point within about 1.5 m of
    the target's centre, 5 .. 25 m long"""
    rng = np.random.default_rng(seed)
    col = colliders(k, rng.choice([cr.BOX, cr.SPHERE, cr.CAPSULE], k), he=rng.uniform(0.2, 2.5, (k, 3)), radius=rng.uniform(0.2, 1.5, k),
                    hh=rng.uniform(0.0, 2.0, k))
    pos = rng.uniform(-SPREAD, SPREAD, (k, 3))
    m = matrices_of(pos, rng.uniform(-np.pi, np.pi, (k, 3)), rng.uniform(0.5, 2.0, (k, 3)))
    away = rng.normal(size=(k, 3))
    away[:, 1] *= 0.3
    away /= np.linalg.norm(away, axis=1, keepdims=True)
    start = pos + away * rng.uniform(4, 15, (k, 1))
    d = (pos + rng.normal(size=(k, 3)) * 1.5) - start
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    end = start + d * rng.uniform(5, 25, (k, 1))
    q = sweeps_of(start, end, rng.uniform(0.2, 0.6, k), rng.choice(np.array([0.0, 0.5, 0.9], F), k))
    return m, col, q


# ---- the constructed scene: answers in closed form -------------------------------------------------------------------
def constructed():
    """0: a sphere of radius 1.5 under scale 2 (R = 3) at (10, 0, 40); 1: an axis-aligned box, half extents (1, 2, 3), at the origin;
    2: a prop of half extents (1, 1, 1) yawed by 45 degrees at (30, 0, 0) -- a diamond in plan whose bounding square is 2.83 m wide;
    3: a wall, half extents (20, 3, 0.5), at (0, 0, -30); 4: a capsule, radius 1, half height 2, at (-30, 0, 30).
    Sweeps (radius 0.4, half height 0.5):
      0  head-on at the sphere along +x: contact at 10 - 3.4 = 6.6
      1  head-on at the box's +x face from x = 12: contact at 12 - 1.4 = 10.6, the grown AABB's own answer
      2  along the prop's edge direction (1, 0, -1) / sqrt 2, 1.8 m from its centre: through the corner of the bounding square (the grown
         square reaches 1.814 * sqrt 2 = 2.57 m along the diagonal), 0.4 m clear of the prop itself
      3  along the wall, 0.3 m off its face, for 10 m
      4  starting in overlap with the capsule
      5  an overlap test beside the sphere on its bounding cube's diagonal: inside the grown cube, 0.28 m clear of the sphere
      6  an overlap test inside the box"""
    pos, rot, scale, col, q = constructed_scene()
    return matrices_of(pos, rot, scale), col, q


def constructed_scene():
    """constructed() as (pos, rot, scale, colliders, sweeps): what a world is built from"""
    pos = [[10, 0, 40], [0, 0, 0], [30, 0, 0], [0, 0, -30], [-30, 0, 30]]
    rot = [[0, 0, 0], [0, 0, 0], [0, np.pi / 4, 0], [0, 0, 0], [0, 0, 0]]
    scale = [[2, 2, 2], [1, 1, 1], [1, 1, 1], [1, 1, 1], [1, 1, 1]]
    col = colliders(5, [cr.SPHERE, cr.BOX, cr.BOX, cr.BOX, cr.CAPSULE], he=[[1, 1, 1], [1, 2, 3], [1, 1, 1], [20, 3, 0.5], [1, 1, 1]],
                    radius=[1.5, 0.5, 0.5, 0.5, 1.0], hh=[0.5, 0.5, 0.5, 0.5, 2.0])
    h = np.sqrt(0.5)
    beside = np.array([30 + 1.8 * h, 0, 1.8 * h])
    along = np.array([h, 0, -h])
    zw = -30 + 0.5 + 0.4 + 0.3
    start = [[0, 0, 40], [12, 0, 0], beside - 6 * along, [-5, 0, zw], [-30, 2.5, 30.5], [12.6, 0, 42.6], [0.5, 0, 0]]
    end = [[10, 0, 40], [0, 0, 0], beside + 6 * along, [5, 0, zw], [-30, 2.5, 40], [12.6, 0, 42.6], [0.5, 0, 0]]
    return pos, rot, scale, col, sweeps_of(start, end, 0.4, 0.5)


def world_case(oracle, n=1200, seed=301, k=500, spread=60.0, max_depth=2, sheared=True):
    """(world, colliders, sweeps): a random world of every collider type -- with max_depth > 0 and non-uniform parent scales its children
    are sheared -- and k sweeps, most of them aimed at an entity from 3 .. 20 m away"""
    w = worlds.random_world(n, seed=seed, spread=spread, max_depth=max_depth if sheared else 0)
    rng = np.random.default_rng(seed + 1)
    col = cr.Colliders.random(w.n, rng)
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    centre = ow.world_matrices()[:w.n][:, 12:15]
    ow.close()
    rng = np.random.default_rng(seed + 2)
    target = rng.integers(0, w.n, k)
    away = rng.normal(size=(k, 3)).astype(F)
    away[:, 1] *= 0.3
    away /= np.linalg.norm(away, axis=1, keepdims=True).astype(F)
    a = (centre[target] + away * rng.uniform(3, 20, (k, 1)).astype(F)).astype(F)
    b = (centre[target] + rng.normal(size=(k, 3)).astype(F) * F(1.0) + (centre[target] - a) * rng.uniform(-0.3, 0.6, (k, 1)).astype(F)).astype(F)
    b[k - 20:] = a[k - 20:]                                                     # overlap tests
    a[k - 40:k - 20] = centre[target[k - 40:k - 20]]                            # starting at a collider's centre
    radius = rng.choice(np.array([0.0, 0.3, 0.5, 1.0], F), k)
    hh = rng.choice(np.array([-1.0, 0.0, 0.6, 0.9], F), k)
    mask = rng.choice(np.array([1, 3, ALL], np.uint32), k)
    return w, col, (a, b, radius, hh, mask, None)
