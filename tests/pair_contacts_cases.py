"""Constructed cases of the pair-contact tests, each with its answer in closed form, shared by the GPU suite
(tests/test_gpu_pair_contacts.py) and its CPU twin (tests/test_pair_contacts_cpu.py).  Inputs only: no GPU.

Rotations are the engine's R = Rz * Ry * Rx (angles about x, y, z).  Member 0 of a case is `a` (the lower index), member 1 is `b`; the
normal points from a to b."""
import numpy as np

from tests import collider_ref as cr, pair_contacts_ref as K
from tests.pair_shapes_cases import flat_world

F = np.float32
S2, S3 = np.sqrt(0.5), np.sqrt(1.0 / 3.0)
Q = np.pi / 4
CM = 1e-2
TILT = -np.arctan(S2)                                         # with Q about x: a cube's (1, 1, 1) corner points along +z


def contact_cases():
    """[(name, kind, normal or None, depth, point or None, member a, member b)] with members (pos, rot, scale, type, he, radius, hh);
    positions relative to the case's own origin.  None: the test states the property instead (see test_pair_contacts_cpu.py)."""
    box = lambda p, r, he: (p, r, (1, 1, 1), cr.BOX, he, 0.5, 0.5)                      # noqa: E731
    sph = lambda p, rad: (p, (0, 0, 0), (1, 1, 1), cr.SPHERE, (1, 1, 1), rad, 0.5)      # noqa: E731
    cap = lambda p, r, rad, hh: (p, r, (1, 1, 1), cr.CAPSULE, (1, 1, 1), rad, hh)       # noqa: E731
    out = []
    out.append(("two spheres along x", K.ROUND_ROUND, (1, 0, 0), CM, (0.495, 0, 0), sph((0, 0, 0), 0.5), sph((1.0 - CM, 0, 0), 0.5)))
    out.append(("sphere on a box face", K.ROUND_BOX, (1, 0, 0), CM, (1.0 - CM / 2, 0.2, 0.3),
                box((0, 0, 0), (0, 0, 0), (1, 1, 1)), sph((1.5 - CM, 0.2, 0.3), 0.5)))
    d = 1.0 + (0.5 - CM) * S3
    out.append(("sphere at a box corner", K.ROUND_BOX, (S3, S3, S3), CM, tuple(np.full(3, 1.0 - CM / 2 * S3)),
                box((0, 0, 0), (0, 0, 0), (1, 1, 1)), sph((d, d, d), 0.5)))
    # the box edge x = 1, y = 1 runs along z; the capsule's axis (-1, 1, 0) / sqrt 2 crosses it at right angles, its middle nearest
    c = 1.0 + (0.3 - CM) * S2
    out.append(("capsule across a box edge", K.ROUND_BOX, (S2, S2, 0), CM, (1.0 - CM / 2 * S2, 1.0 - CM / 2 * S2, 0),
                box((0, 0, 0), (0, 0, 0), (1, 1, 1)), cap((c, c, 0), (0, 0, Q), 0.3, 1.5)))
    # parallel capsules, axes (-1, 1, 0) / sqrt 2, set off at right angles to them: the point is anywhere along the shared stretch
    s = (0.4 + 0.5 - CM) * S2
    out.append(("parallel capsules", K.ROUND_ROUND, (S2, S2, 0), CM, None, cap((0, 0, 0), (0, 0, Q), 0.4, 1.0), cap((s, s, 0), (0, 0, Q), 0.5, 1.0)))
    # the sphere is b: the normal is the box's outward face normal; surfaces at x = 1 (box) and x = 0.8 - 0.5 (sphere)
    out.append(("sphere with its centre inside a box", K.ROUND_BOX | K.DEEP, (1, 0, 0), 0.5 + 0.2, (0.65, 0.1, -0.2),
                box((0, 0, 0), (0, 0, 0), (1, 1, 1)), sph((0.8, 0.1, -0.2), 0.5)))
    # the same with the sphere as a: the normal turns round
    out.append(("box around the centre of sphere a", K.ROUND_BOX | K.DEEP, (0, -1, 0), 0.5 + 0.25, (0.1, 0.625, -0.2),
                sph((0.1, 0.75, -0.2), 0.5), box((0, 0, 0), (0, 0, 0), (1, 1, 1))))
    # one orientation: a's axis x and b's axis x overlap equally, the earlier one -- a's -- is reported; b's vertex (0.99, -0.2, -0.95) is
    # clamped into a's face
    out.append(("boxes face to face", K.BOX_FACE_A, (1, 0, 0), CM, (1.0 - CM / 2, -0.2, -0.75),
                box((0, 0, 0), (0, 0, 0), (1, 0.5, 0.75)), box((2.0 - CM, 0.3, -0.2), (0, 0, 0), (1, 0.5, 0.75))))
    # a cube standing on its corner under a plate: the plate, b, owns the face
    h = 0.5 * np.sqrt(3.0)
    out.append(("box corner into a face", K.BOX_FACE_B, (0, 0, 1), CM, (0, 0, h - CM / 2),
                box((0, 0, 0), (Q, TILT, 0), (0.5, 0.5, 0.5)), box((0, 0, h + 0.25 - CM), (0, 0, 0), (2, 2, 0.25))))
    # a beam along x turned 45 degrees about x, a beam along z turned 45 degrees about z above it: the ridge of one meets the keel of the other
    r = 0.5 * np.sqrt(2.0)
    out.append(("boxes crossed edge to edge", K.BOX_EDGE, (0, 1, 0), CM, (0, r - CM / 2, 0),
                box((0, 0, 0), (Q, 0, 0), (2, 0.5, 0.5)), box((0, 2 * r - CM, 0), (0, 0, Q), (0.5, 0.5, 2))))
    out.append(("coincident spheres", K.ROUND_ROUND | K.DEGENERATE, (0, 1, 0), 0.5 + 0.25, (0, 0, 0), sph((0, 0, 0), 0.5), sph((0, 0, 0), 0.25)))
    proxy = ((0.3, 0, 0), (0, 0, 0), (1, 1, 1), cr.BOUNDS, (1, 1, 1), 0.5, 0.5)
    out.append(("a Bounds proxy", K.NONE, (0, 0, 0), 0.0, (0, 0, 0), sph((0, 0, 0), 0.5), proxy))
    flat = ((0.3, 0, 0), (0, 0, 0), (0, 1, 1), cr.BOX, (1, 1, 1), 0.5, 0.5)
    out.append(("a zero column", K.NONE, (0, 0, 0), 0.0, (0, 0, 0), sph((0, 0, 0), 0.5), flat))
    return out


def contact_world():
    """(world, colliders, cases, origins): case i is the pair (2i, 2i + 1), 20 m from its neighbours"""
    cases = contact_cases()
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
