"""Worlds of the pair-manifold tests, shared by the GPU suite (tests/test_gpu_pair_manifolds.py) and its CPU twin
(tests/test_pair_manifolds_cpu.py).  Inputs only: no GPU.

    manifold_world()   constructed cases, one per pair, each with its count, kind and -- where a closed form exists -- its points and depths
    resting_world()    seeded: boxes stacked on boxes (random yaw about the shared normal, a tilt of 0 to 2 degrees), capsules lying on
                       boxes and beside each other -- the areas and lines the agreement worlds of tests/pair_shapes_cases.py hardly hold

Rotations are the engine's R = Rz * Ry * Rx (angles about x, y, z).  Member 0 of a case is `a` (the lower index), member 1 is `b`."""
import numpy as np

from tests import collider_ref as cr, pair_manifolds_ref as M
from tests.pair_contacts_cases import CM, Q, S2, S3, TILT
from tests.pair_shapes_cases import flat_world

F = np.float32
H90 = np.pi / 2
DEG = np.pi / 180.0
OCT = S2 - 0.5                                                # a unit square cut by its twin turned 45 degrees: vertices (+-0.5, +-OCT), (+-OCT, +-0.5)


def manifold_cases():
    """[(name, count or None, kind, points or None, depth or None, member a, member b)] with members (pos, rot, scale, type, he, radius,
    hh); positions and points relative to the case's own origin.  points: the SET of expected points (any order), or for a REDUCED case
    the set they are drawn from; depth: one value for every point."""
    box = lambda p, r, he: (p, r, (1, 1, 1), cr.BOX, he, 0.5, 0.5)                      # noqa: E731
    sph = lambda p, rad: (p, (0, 0, 0), (1, 1, 1), cr.SPHERE, (1, 1, 1), rad, 0.5)      # noqa: E731
    cap = lambda p, r, rad, hh: (p, r, (1, 1, 1), cr.CAPSULE, (1, 1, 1), rad, hh)       # noqa: E731
    slab = box((0, 0, 0), (0, 0, 0), (2, 0.5, 2))
    y = 0.5 - CM / 2                                           # halfway between the slab's top face and what lies CM deep in it
    out = []
    out.append(("cube flat on a larger slab", 4, M.FACE, [(0.3 + sx, y, -0.2 + sz) for sx in (-0.5, 0.5) for sz in (-0.5, 0.5)], CM,
                slab, box((0.3, 1.0 - CM, -0.2), (0, 0, 0), (0.5, 0.5, 0.5))))
    octagon = [(sx * 0.5, y, sz * OCT) for sx in (-1, 1) for sz in (-1, 1)] + [(sx * OCT, y, sz * 0.5) for sx in (-1, 1) for sz in (-1, 1)]
    out.append(("cube on an equal face, yawed 45 degrees", 4, M.FACE | M.REDUCED, octagon, CM,
                box((0, 0, 0), (0, 0, 0), (0.5, 0.5, 0.5)), box((0, 1.0 - CM, 0), (0, Q, 0), (0.5, 0.5, 0.5))))
    out.append(("cube overhanging a slab edge", 4, M.FACE, [(x, y, sz * 0.5) for x in (1.7, 2.0) for sz in (-1, 1)], CM,
                slab, box((2.2, 1.0 - CM, 0), (0, 0, 0), (0.5, 0.5, 0.5))))
    # turned 3 degrees about z: the edge x = -0.5, y = -0.5 of the cube is its lowest, 0.5 (sin + cos) below the centre
    s, c = np.sin(3 * DEG), np.cos(3 * DEG)
    out.append(("cube tilted 3 degrees about an edge", 2, M.FACE, [(-0.5 * c + 0.5 * s, y, sz * 0.5) for sz in (-1, 1)], CM,
                slab, box((0, 0.5 + 0.5 * (s + c) - CM, 0), (0, 0, 3 * DEG), (0.5, 0.5, 0.5))))
    h = 0.5 * np.sqrt(3.0)
    out.append(("corner-down cube", 1, M.FACE, [(0, 0, h - CM / 2)], CM,
                box((0, 0, 0), (Q, TILT, 0), (0.5, 0.5, 0.5)), box((0, 0, h + 0.25 - CM), (0, 0, 0), (2, 2, 0.25))))
    r = 0.5 * np.sqrt(2.0)
    out.append(("edge-edge boxes", 1, M.SINGLE, [(0, r - CM / 2, 0)], CM,
                box((0, 0, 0), (Q, 0, 0), (2, 0.5, 0.5)), box((0, 2 * r - CM, 0), (0, 0, Q), (0.5, 0.5, 2))))
    # a capsule turned 90 degrees about z lies along x
    out.append(("capsule lying on a box face", 2, M.SEGMENT, [(0.2 - 0.8, y, 0.1), (0.2 + 0.8, y, 0.1)], CM,
                slab, cap((0.2, 0.5 + 0.3 - CM, 0.1), (0, 0, H90), 0.3, 0.8)))
    out.append(("capsule sticking out over the edge", 2, M.SEGMENT, [(1.6 - 0.8, y, 0.1), (2.0, y, 0.1)], CM,
                slab, cap((1.6, 0.5 + 0.3 - CM, 0.1), (0, 0, H90), 0.3, 0.8)))
    out.append(("capsule standing on a face", 1, M.SEGMENT, [(0.4, y, -0.3)], CM,
                slab, cap((0.4, 0.5 + 0.8 + 0.3 - CM, -0.3), (0, 0, 0), 0.3, 0.8)))
    e = 1.0 + (0.3 - CM) * S2
    out.append(("capsule against a box edge", 1, M.SINGLE, [(1.0 - CM / 2 * S2, 1.0 - CM / 2 * S2, 0)], CM,
                box((0, 0, 0), (0, 0, 0), (1, 1, 1)), cap((e, e, 0), (0, 0, Q), 0.3, 1.5)))
    # the centre line 0.3 below the face y = 1: both ends 0.3 + 0.2 deep; along the face's normal the whole round lies in the box, so the
    # middle of what the two share is the centre line itself
    out.append(("DEEP capsule", None, M.SEGMENT, [(0.1 - 0.3, 0.7, 0), (0.1 + 0.3, 0.7, 0)], 0.5,
                box((0, 0, 0), (0, 0, 0), (1, 1, 1)), cap((0.1, 0.7, 0), (0, 0, H90), 0.2, 0.3)))
    d = 0.4 + 0.5 - CM
    out.append(("parallel capsules side by side", 2, M.SEGMENT, [(0.395, -1, 0), (0.395, 1, 0)], CM,
                cap((0, 0, 0), (0, 0, 0), 0.4, 1.0), cap((d, 0, 0), (0, 0, 0), 0.5, 1.0)))
    out.append(("parallel capsules with partial overlap", 2, M.SEGMENT, [(0.395, -0.3, 0), (0.395, 1, 0)], CM,
                cap((0, 0, 0), (0, 0, 0), 0.4, 1.0), cap((d, 0.7, 0), (0, 0, 0), 0.5, 1.0)))
    out.append(("crossed capsules", 1, M.SINGLE, [(0, 0, 0.395)], CM,
                cap((0, 0, 0), (0, 0, 0), 0.4, 1.0), cap((0, 0, d), (0, 0, H90), 0.5, 1.0)))
    out.append(("sphere pair", 1, M.SINGLE, [(0.495, 0, 0)], CM, sph((0, 0, 0), 0.5), sph((1.0 - CM, 0, 0), 0.5)))
    out.append(("sphere on a box face", 1, M.SINGLE, [(1.0 - CM / 2, 0.2, 0.3)], CM,
                box((0, 0, 0), (0, 0, 0), (1, 1, 1)), sph((1.5 - CM, 0.2, 0.3), 0.5)))
    proxy = ((0.3, 0, 0), (0, 0, 0), (1, 1, 1), cr.BOUNDS, (1, 1, 1), 0.5, 0.5)
    out.append(("a Bounds proxy", 0, M.NONE, None, None, sph((0, 0, 0), 0.5), proxy))
    flat = ((0.3, 0, 0), (0, 0, 0), (0, 1, 1), cr.BOX, (1, 1, 1), 0.5, 0.5)
    out.append(("a zero column", 0, M.NONE, None, None, sph((0, 0, 0), 0.5), flat))
    return out


def manifold_world():
    """(world, colliders, cases, origins): case i is the pair (2i, 2i + 1), 20 m from its neighbours"""
    cases = manifold_cases()
    n = 2 * len(cases)
    pos, rot, scale = np.zeros((n, 3)), np.zeros((n, 3)), np.ones((n, 3))
    origins = np.zeros((len(cases), 3))
    col = cr.Colliders(n)
    for i, case in enumerate(cases):
        origins[i] = [-100.0 + 20.0 * (i % 10), 0.0, -40.0 + 40.0 * (i // 10)]
        for j, (p, r, sc, typ, he, rad, hh) in enumerate(case[5:]):
            e = 2 * i + j
            pos[e], rot[e], scale[e] = origins[i] + np.asarray(p, np.float64), r, sc
            col.type[e], col.he[e], col.radius[e], col.hh[e] = typ, F(he), F(rad), F(hh)
    return flat_world(pos, rot, scale), col, cases, origins


# ---- the resting world ---------------------------------------------------------------------------------------------------------
RESTING_SEEDS = (2601, 2602, 2603, 2604, 2605, 2606, 2607, 2608)
RESTING_STACKS, RESTING_ON_BOX, RESTING_BESIDE = 150, 25, 25
STACK, ON_BOX, BESIDE = 0, 1, 2


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def resting_world(seed):
    """(world, colliders, unit kinds): unit i is the pair (2i, 2i + 1) on an 8 m grid.  Every unit rests 2 to 8 cm deep in its partner:
    a box on a box (half of them of equal footprint, so that yaw makes octagons; a fifth overhanging), a capsule lying on a box (a third
    sticking out over an edge), a capsule lying beside a capsule with a random shift along the axis."""
    rng = np.random.default_rng(seed)
    units = np.array([STACK] * RESTING_STACKS + [ON_BOX] * RESTING_ON_BOX + [BESIDE] * RESTING_BESIDE)
    k = len(units)
    side = int(np.ceil(np.sqrt(k)))
    n = 2 * k
    pos, rot = np.zeros((n, 3)), np.zeros((n, 3))
    col = cr.Colliders(n)
    col.he[:] = 0.5; col.radius[:] = 0.5; col.hh[:] = 0.5
    for i, unit in enumerate(units):
        origin = np.array([(i % side - side / 2) * 8.0, rng.uniform(-1, 1), (i // side - side / 2) * 8.0])
        a, b = 2 * i, 2 * i + 1
        deep = rng.uniform(0.02, 0.05)
        tilt = 2.0 * DEG * rng.uniform()
        lean = rng.uniform(0, 2 * np.pi)                       # which way the tilt leans
        if unit == STACK:
            equal = rng.uniform() < 0.5
            ha = np.array([rng.uniform(0.6, 1.2), rng.uniform(0.3, 0.6), rng.uniform(0.6, 1.2)])
            hb = np.array([ha[0], rng.uniform(0.3, 0.6), ha[2]]) if equal else np.array([rng.uniform(0.4, 0.9), rng.uniform(0.3, 0.6), rng.uniform(0.4, 0.9)])
            if equal:                                          # an octagon keeps more than four vertices only while they are below the face; a
                tilt = rng.uniform(0.3, 0.8) * DEG             # tilt under a tenth of a degree leaves the two boxes' normals within TOL
                deep += 0.03
            col.type[a] = col.type[b] = cr.BOX
            col.he[a], col.he[b] = F(ha), F(hb)
            rot[a] = [0, rng.uniform(-np.pi, np.pi), 0]
            rot[b] = [tilt * np.cos(lean), rot[a][1] + rng.uniform(-np.pi, np.pi), tilt * np.sin(lean)]
            Rb = rotation(*rot[b])
            reach = (np.abs(Rb[1]) * hb).sum()                 # how far b reaches below its centre
            shift = rng.uniform(-0.2, 0.2, 2) * (1.0 if rng.uniform() < 0.8 else 4.0) * ha[[0, 2]]
            Ra = rotation(*rot[a])
            pos[a] = origin
            pos[b] = origin + Ra @ np.array([shift[0], 0, shift[1]]) + [0, ha[1] + reach - deep, 0]
        elif unit == ON_BOX:
            ha = np.array([rng.uniform(0.8, 1.5), rng.uniform(0.3, 0.6), rng.uniform(0.8, 1.5)])
            radius, hh = rng.uniform(0.2, 0.4), rng.uniform(0.4, 0.9)
            col.type[a], col.type[b] = cr.BOX, cr.CAPSULE
            col.he[a], col.radius[b], col.hh[b] = F(ha), F(radius), F(hh)
            rot[a] = [0, rng.uniform(-np.pi, np.pi), 0]
            rot[b] = [H90 + tilt, rng.uniform(-np.pi, np.pi), 0]
            out = rng.uniform() < 0.33
            Ra = rotation(*rot[a])
            along = rng.uniform(-0.3, 0.3) * ha[0] + (ha[0] if out else 0.0)
            pos[a] = origin
            pos[b] = origin + Ra @ np.array([along, 0, rng.uniform(-0.3, 0.3) * ha[2]]) + [0, ha[1] + radius + hh * np.sin(tilt) - deep, 0]
        else:
            ra, rb = rng.uniform(0.25, 0.5, 2)
            hha, hhb = rng.uniform(0.6, 1.2, 2)
            col.type[a] = col.type[b] = cr.CAPSULE
            col.radius[a], col.radius[b], col.hh[a], col.hh[b] = F(ra), F(rb), F(hha), F(hhb)
            yaw = rng.uniform(-np.pi, np.pi)
            rot[a] = [H90, yaw, 0]
            rot[b] = [H90 + tilt * np.cos(lean), yaw + 0.25 * tilt * np.sin(lean), 0]
            Ra = rotation(*rot[a])
            axis, across = Ra @ np.array([0, 1.0, 0]), Ra @ np.array([1.0, 0, 0])
            pos[a] = origin
            pos[b] = origin + across * (ra + rb - deep) + axis * rng.uniform(-0.8, 0.8) * hha
    return flat_world(pos, rot, np.ones((n, 3))), col, units
