"""Seeded cases of the exact-shape ray tests, shared by the GPU suite (tests/test_gpu_shape_rays.py) and its CPU twin
(tests/test_shape_rays_cpu.py, which asserts without a GPU that the seeds give the GPU tests what they count on).  Inputs and the
witness call only: no GPU."""
import numpy as np

from tests import collider_ref as cr, shape_rays_ref as sr, worlds

F = np.float32
ALL = 0xFFFFFFFF


def witness(ow, w, col, q, mode=sr.EXACT, skip=None):
    mn, mx = col.witness(ow, w.n)
    return sr.cast(ow.world_matrices()[:w.n], mn, mx, w.group, w.mask, col, *q, mode=mode, skip=skip)


def rays_of(o, d, md=None, mask=None):
    o, d = np.ascontiguousarray(o, F).reshape(-1, 3), np.ascontiguousarray(d, F).reshape(-1, 3)
    k = len(o)
    return (o, d, np.full(k, 100.0, F) if md is None else np.ascontiguousarray(md, F).reshape(k),
            np.full(k, ALL, np.uint32) if mask is None else np.ascontiguousarray(mask, np.uint32).reshape(k))


# ---- an identity box is its own AABB
def identity_box_rays():
    rng = np.random.default_rng(201)
    he = F([1.0, 0.5, 2.0])
    o = rng.uniform(-6, 6, (900, 3)).astype(F)
    d = rng.normal(size=(900, 3)).astype(F)
    aim = rng.uniform(-1, 1, (600, 3)).astype(F) * he * F(1.3)
    d[:600] = aim - o[:600]                                                     # general: towards the box, some past its edges
    for a in range(3):                                                           # axis-parallel: one or two zero components
        d[600 + 40 * a:640 + 40 * a, a] = 0.0
    d[720:750, 0] = 0.0; d[720:750, 1] = 0.0
    o[720:750, :2] = rng.uniform(-1, 1, (30, 2)).astype(F) * he[:2]
    o[750:850] = rng.uniform(-1, 1, (100, 3)).astype(F) * he                    # origin inside
    d[850:] = o[850:] * F(2.0)                                                  # pointing away
    return he, rays_of(o, d, np.full(900, 30.0, F))


# ---- a random world
SEED_WORLD, SEED_COL, SEED_RAYS = 211, 212, 213       # (chosen on the CPU: tests/test_shape_rays_cpu.py asserts the counts below without a GPU)
NUDGE = 0.8


def random_case(oracle):
    """(world, colliders, rays): 2 000 entities, depth 3, every collider type, 20 plates that are only in the big list; 3 000 rays, most
    of them aimed at an entity from 3 .. 30 m away, some axis-parallel, some starting at collider centres, some outside the bin grid."""
    w = worlds.random_world(2000, seed=SEED_WORLD, spread=140.0, max_depth=3)
    rng = np.random.default_rng(SEED_COL)
    col = cr.Colliders.random(w.n, rng)
    roots = np.flatnonzero(w.parent < 0)[:20]
    col.type[roots] = cr.BOX
    col.he[roots] = F([80.0, 0.5, 80.0])                                        # wider than 2 x 2 sectors whatever their rotation
    w.scale[roots] = 1.0; w.rot[roots, 0] = 0.0; w.rot[roots, 2] = 0.0
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    m = ow.world_matrices()[:w.n]
    ow.close()
    centre = m[:, 12:15]
    rng = np.random.default_rng(SEED_RAYS)
    k = 3000
    target = rng.integers(0, w.n, k)
    away = rng.normal(size=(k, 3)).astype(F)
    away[:, 1] *= 0.3
    away /= np.linalg.norm(away, axis=1, keepdims=True).astype(F)
    o = (centre[target] + away * rng.uniform(3, 30, (k, 1)).astype(F)).astype(F)
    d = ((centre[target] + rng.normal(size=(k, 3)).astype(F) * F(0.8)) - o).astype(F)
    d[2000:2100, 0] = 0.0                                                       # the |dir| < 1e-6 branch of one or two axes
    d[2100:2200, 2] = 0.0
    d[2200:2260, [0, 2]] = 0.0
    o[2300:2500] = centre[target[2300:2500]]                                    # starting at a collider's centre
    o[2500:2560] += F([3000.0, 0, -2500.0])                                     # outside the bin grid: the big list only
    md = np.where(rng.random(k) < 0.2, rng.uniform(200, 900, k), rng.uniform(5, 60, k)).astype(F)
    mask = rng.choice(np.array([1, 2, 3, ALL], np.uint32), k)
    return w, col, (o, d, md, mask)


def winner_counts(want, plain, col):
    """winners per collider type, and how many rays answer differently in the two modes"""
    hit = want["hit"] == 1
    types = col.type[want["id"][hit]]
    differ = (want["hit"] != plain["hit"]) | (want["id"] != plain["id"]) | (want["distance"].view(np.uint32) != plain["distance"].view(np.uint32))
    return {k: int((types == k).sum()) for k in (cr.BOUNDS, cr.BOX, cr.SPHERE, cr.CAPSULE)}, int(differ.sum())
