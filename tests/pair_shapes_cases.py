"""Seeded and constructed cases of the touching-pairs tests, shared by the GPU suite (tests/test_gpu_pair_shapes.py) and its CPU twin
(tests/test_pair_shapes_cpu.py, which asserts without a GPU that the seeds give the GPU tests what they count on).  Inputs only: no GPU."""
import numpy as np

from sc_gameengine_amd import synth_world as sw
from tests import collider_ref as cr, worlds

F = np.float32
ALL = 0xFFFFFFFF


def flat_world(pos, rot, scale, origin=(-2, -2), sectors=(4, 4)):
    """Roots with unit Bounds, group 1, mask all, in a rectangle of 64 m sectors around the origin."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    n = len(pos)
    return sw.SynthWorld(pos=pos.copy(), rot=np.ascontiguousarray(rot, F).reshape(n, 3).copy(), scale=np.ascontiguousarray(scale, F).reshape(n, 3).copy(),
                         parent=np.full(n, -1, np.int32), bmin=np.full((n, 3), -0.5, F), bmax=np.full((n, 3), 0.5, F),
                         has_mesh=np.ones(n, np.uint8), has_bounds=np.ones(n, np.uint8), mesh=np.zeros(n, np.uint32),
                         material=np.zeros(n, np.uint32), group=np.ones(n, np.uint32), mask=np.full(n, ALL, np.uint32),
                         sector_of=np.zeros((n, 2), np.int32), origin=origin, sectors=sectors)


def oracle_matrices(oracle, w):
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    m = ow.world_matrices()[:w.n].copy()
    ow.close()
    return m


def oracle_pairs(oracle, m, col, w):
    """the AABB pair set of the witness boxes, as the pair search must report it: [k][2] dense indices a < b, sorted"""
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    mn, mx = col.witness(ow, w.n)
    ow.close()
    return np.ascontiguousarray(oracle.broadphase_bruteforce(mn, mx, w.group, w.mask), np.uint32).reshape(-1, 2)


# ---- the agreement world: roots only, so every frame is orthogonal ------------------------------------------------------------
AGREEMENT_SEEDS = (401, 402, 403)
AGREEMENT_N = 600


def agreement_world(seed, n=AGREEMENT_N):
    """600 roots in a 40 m x 6 m x 40 m volume, yaw, pitch and roll random, scales non-uniform, the three collider types mixed, sizes of
    0.3 .. 1.8 m"""
    rng = np.random.default_rng(seed)
    pos = (rng.uniform(-1, 1, (n, 3)) * [20.0, 3.0, 20.0]).astype(F)
    rot = rng.uniform(-np.pi, np.pi, (n, 3)).astype(F)
    scale = rng.uniform(1.0, 1.25, (n, 3)).astype(F)
    w = flat_world(pos, rot, scale)
    col = cr.Colliders(n)
    col.type[:] = rng.choice(np.array([cr.BOX, cr.SPHERE, cr.CAPSULE], np.uint8), n, p=(0.28, 0.38, 0.34))
    col.he[:] = rng.uniform(0.3, 1.44, (n, 3)).astype(F)
    col.radius[:] = rng.uniform(0.3, 1.3, n).astype(F)
    col.hh[:] = rng.uniform(0.0, 0.8, n).astype(F)
    return w, col


# ---- closed forms ------------------------------------------------------------------------------------------------------------
S2, S3 = np.sqrt(0.5), np.sqrt(1.0 / 3.0)
Q = np.pi / 4
GAP = 1e-2


def closed_form_cases():
    """[(name, touching, listed, (pos, rot, type, he, radius, hh) of member 0, the same of member 1)]: positions relative to the case's
    own origin.  touching: the answer in closed form; listed: the members' AABBs overlap, so the pair search reports the pair."""
    box = lambda p, r, he: (p, r, cr.BOX, he, 0.5, 0.5)                         # noqa: E731
    sph = lambda p, rad: (p, (0, 0, 0), cr.SPHERE, (1, 1, 1), rad, 0.5)         # noqa: E731
    cap = lambda p, r, rad, hh: (p, r, cr.CAPSULE, (1, 1, 1), rad, hh)          # noqa: E731
    out = []
    # two 4.4 m x 2 m vehicles yawed by 45 degrees, 3 m apart across their lanes (column 0 of the yaw is (cos, 0, -sin)): 1 m of air
    car = (1.0, 0.75, 2.2)
    out.append(("vehicles in neighbouring lanes", False, True, box((0, 0, 0), (0, Q, 0), car), box((3 * S2, 0, -3 * S2), (0, Q, 0), car)))
    for sgn, touch in ((1, False), (-1, True)):
        g = sgn * GAP
        d = 1.0 + (0.5 + g) * S3
        out.append((f"sphere at a box corner, gap {g:+}", touch, True, box((0, 0, 0), (0, 0, 0), (1, 1, 1)), sph((d, d, 0 + d), 0.5)))
        # the box edge x = 1, y = 1 runs along z; the capsule's axis (-1, 1, 0) / sqrt 2 crosses it at right angles, its middle nearest
        c = 1.0 + (0.3 + g) * S2
        out.append((f"capsule across a box edge, gap {g:+}", touch, True, box((0, 0, 0), (0, 0, 0), (1, 1, 1)), cap((c, c, 0), (0, 0, Q), 0.3, 1.5)))
        # parallel capsules, axes (-1, 1, 0) / sqrt 2, set off at right angles to them
        s = (0.4 + 0.5 + g) * S2
        out.append((f"parallel capsules, gap {g:+}", touch, True, cap((0, 0, 0), (0, 0, Q), 0.4, 1.0), cap((s, s, 0), (0, 0, Q), 0.5, 1.0)))
        # two boxes of one orientation: nine cross axes of parallel edges, null vectors up to rounding
        o = (1.0 + 1.0 + g) * S2
        out.append((f"boxes with parallel edges, gap {g:+}", touch, True, box((0, 0, 0), (0, Q, 0), (1, 0.5, 2)), box((o, 0, -o), (0, Q, 0), (1, 0.5, 2))))
        # a capsule without height and the sphere of its radius give one answer
        k = (1.0 + g) * S3
        out.append((f"capsule without height, gap {g:+}", touch, True, cap((0, 0, 0), (0.3, 0.2, 0.1), 0.5, 0.0), sph((k, k, k), 0.5)))
        out.append((f"the same as a sphere, gap {g:+}", touch, True, sph((0, 0, 0), 0.5), sph((k, k, k), 0.5)))
        # identity boxes are their own AABBs
        out.append((f"identity boxes, gap {g:+}", touch, touch, box((0, 0, 0), (0, 0, 0), (1, 0.5, 0.75)), box((2.0 + g, 0.3, -0.2), (0, 0, 0), (1, 0.5, 0.75))))
    return out


def closed_form_world():
    """(world, colliders, cases): case i is the pair (2i, 2i + 1), 20 m from its neighbours"""
    cases = closed_form_cases()
    n = 2 * len(cases)
    pos, rot = np.zeros((n, 3)), np.zeros((n, 3))
    col = cr.Colliders(n)
    for i, (_, _, _, *members) in enumerate(cases):
        origin = np.array([-100.0 + 20.0 * (i % 10), 0.0, -40.0 + 40.0 * (i // 10)])
        for j, (p, r, typ, he, rad, hh) in enumerate(members):
            e = 2 * i + j
            pos[e], rot[e] = origin + np.asarray(p, np.float64), r
            col.type[e], col.he[e], col.radius[e], col.hh[e] = typ, F(he), F(rad), F(hh)
    return flat_world(pos, rot, np.ones((n, 3))), col, cases


# ---- the GPU suite's forest --------------------------------------------------------------------------------------------------
FOREST_SEED_WORLD, FOREST_SEED_COL = 411, 412          # (chosen on the CPU: tests/test_pair_shapes_cpu.py asserts the counts without a GPU)
FOREST_N, FOREST_SPREAD, FOREST_NUDGE = 2000, 30.0, 0.4


def forest():
    """(world, colliders): 2 000 entities, depth 3, children under non-uniformly scaled parents (sheared frames), every collider type,
    20 plates that are only in the big list"""
    w = worlds.random_world(FOREST_N, seed=FOREST_SEED_WORLD, spread=FOREST_SPREAD, max_depth=3)
    w.pos[w.parent < 0, 1] *= F(0.15)
    w.scale[:] = np.random.default_rng(FOREST_SEED_WORLD + 1000).uniform(0.6, 1.5, (w.n, 3)).astype(F)
    w.group[:], w.mask[:] = 1, ALL
    rng = np.random.default_rng(FOREST_SEED_COL)
    col = cr.Colliders.random(w.n, rng, p=(0.1, 0.05, 0.2, 0.37, 0.28))
    col.he[:] = rng.uniform(0.2, 1.2, (w.n, 3)).astype(F)
    col.radius[:] = rng.uniform(0.2, 0.9, w.n).astype(F)
    col.hh[:] = rng.uniform(-0.3, 1.2, w.n).astype(F)
    roots = np.flatnonzero(w.parent < 0)[:20]
    col.type[roots] = cr.BOX
    col.he[roots] = F([80.0, 0.05, 80.0])                                       # wider than 2 x 2 sectors whatever their rotation
    w.scale[roots] = 1.0; w.rot[roots, 0] = 0.0; w.rot[roots, 2] = 0.0
    w.pos[roots, 1] = np.linspace(-60.0, -40.0, 20).astype(F)                  # below the crowd, a metre apart: plates meet nothing
    return w, col


# ---- pair lists of awkward lengths --------------------------------------------------------------------------------------------
# none, one, around a wave, several shard segments with empty ones among them, a total that is no multiple of the workgroup
WALK_LENGTHS, WALK_SEED = (0, 1, 63, 64, 65, 300, 1001), 420


def couples_world(k, seed):
    """k couples of overlapping AABBs scattered over a 16 x 16 sector rectangle, no two couples near each other: exactly k pairs, spread
    over the pair search's workgroups and so over its shard segments.  Every second couple's shapes are apart."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(33 * 33, max(k, 1), replace=False)
    base = np.stack([(cells % 33) * 30.0 - 480.0, rng.uniform(-2, 2, len(cells)), (cells // 33) * 30.0 - 480.0], axis=1)
    n = 2 * len(cells)
    pos = np.repeat(base, 2, axis=0)
    apart = np.arange(len(cells)) % 2 == 1
    off = np.where(apart[:, None], [0.62, 0.62, 0.62], [0.4, 0.3, 0.2])       # radii 0.5 + 0.5: |off| = 1.07 is apart, 0.54 touches
    pos[1::2] += off if k else [200.0, 0.0, 0.0]                               # (k == 0: two lone entities)
    w = flat_world(pos, rng.uniform(-np.pi, np.pi, (n, 3)), np.ones((n, 3)), origin=(-8, -8), sectors=(16, 16))
    col = cr.Colliders(n)
    col.type[:] = rng.choice(np.array([cr.SPHERE, cr.CAPSULE], np.uint8), n)
    col.type[::7] = cr.BOX
    col.he[:] = 0.35; col.radius[:] = 0.5; col.hh[:] = 0.0
    col.he[np.repeat(~apart, 2)] = 0.6
    return w, col, int(apart.sum()) if k else 0
