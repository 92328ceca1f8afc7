"""Witness of the collider box rule, independent of the kernels: numpy fp32, one rounding per
operation, left to right.  It takes WORLD matrices (the oracle's, column-major m[c*4 + r]) and returns world AABBs that go
to the oracle's broadphase_bruteforce / broadphase_grid / raycast_boxes, which take explicit boxes.

    c_r = M[r,3]        n_k = (M[0,k]^2 + M[1,k]^2) + M[2,k]^2
    BOX      (ex, ey, ez) = halfExtents            pad = 0
    SPHERE   (ex, ey, ez) = (0, 0, 0)              pad = radius * sqrt(max(n_0, n_1, n_2))
    CAPSULE  (ex, ey, ez) = (0, max(0, hh), 0)     pad = radius * sqrt(max(n_0, n_2))
    h_r = ((|M[r,0]| ex + |M[r,1]| ey) + |M[r,2]| ez) + pad         min = c - h, max = c + h

BOUNDS entities take the box handed in (the oracle's world_aabbs(): today's rule); NONE, and BOUNDS entities without
Bounds, have the "no box" value (+inf, -inf)."""
import numpy as np

BOUNDS, NONE, BOX, SPHERE, CAPSULE = 0, 1, 2, 3, 4
F = np.float32


def typed_boxes(m16, ctype, half_extents, radius, half_height):
    """Boxes of every row as if its type were typed (rows of type BOUNDS / NONE come out as 'no box')."""
    m = np.ascontiguousarray(m16, F).reshape(-1, 16)
    n = len(m)
    ctype = np.asarray(ctype, np.uint8).reshape(n)
    he = np.ascontiguousarray(half_extents, F).reshape(n, 3)
    r = np.ascontiguousarray(radius, F).reshape(n)
    hh = np.ascontiguousarray(half_height, F).reshape(n)
    M = lambda row, col: m[:, col * 4 + row]                      # noqa: E731
    e = np.zeros((n, 3), F)
    e[ctype == BOX] = he[ctype == BOX]
    e[ctype == CAPSULE, 1] = np.maximum(F(0.0), hh[ctype == CAPSULE])
    nk = [(M(0, k) * M(0, k) + M(1, k) * M(1, k)) + M(2, k) * M(2, k) for k in range(3)]
    with np.errstate(invalid="ignore", over="ignore"):
        pad = np.zeros(n, F)
        sph, cap = ctype == SPHERE, ctype == CAPSULE
        pad[sph] = (r * np.sqrt(np.maximum(np.maximum(nk[0], nk[1]), nk[2])))[sph]
        pad[cap] = (r * np.sqrt(np.maximum(nk[0], nk[2])))[cap]
        mn, mx = np.full((n, 3), np.inf, F), np.full((n, 3), -np.inf, F)
        typed = ctype >= BOX
        for row in range(3):
            h = ((np.abs(M(row, 0)) * e[:, 0] + np.abs(M(row, 1)) * e[:, 1]) + np.abs(M(row, 2)) * e[:, 2]) + pad
            c = M(row, 3)
            mn[typed, row] = (c - h)[typed]
            mx[typed, row] = (c + h)[typed]
    assert mn.dtype == F and mx.dtype == F
    return mn, mx


def boxes(m16, ctype, half_extents, radius, half_height, bounds_min, bounds_max):
    """World AABBs of every entity's proxy; bounds_min / bounds_max: the Bounds boxes (inf where an entity has no Bounds)."""
    ctype = np.asarray(ctype, np.uint8).reshape(-1)
    mn, mx = typed_boxes(m16, ctype, half_extents, radius, half_height)
    b = ctype == BOUNDS
    mn[b], mx[b] = np.asarray(bounds_min, F)[b], np.asarray(bounds_max, F)[b]
    return mn, mx


class Colliders:
    """Host model of the per-entity collider state: what was uploaded, hence what the witness and colliders() must show."""

    def __init__(self, n):
        self.type = np.zeros(n, np.uint8)
        self.he = np.full((n, 3), 0.5, F)
        self.radius = np.full(n, 0.5, F)
        self.hh = np.full(n, 0.5, F)

    @classmethod
    def random(cls, n, rng, p=(0.2, 0.15, 0.25, 0.2, 0.2)):
        c = cls(n)
        c.type[:] = rng.choice(5, n, p=p).astype(np.uint8)
        c.he[:] = rng.uniform(0.05, 2.5, (n, 3)).astype(F)
        c.radius[:] = rng.uniform(0.05, 2.0, n).astype(F)
        c.hh[:] = rng.uniform(-0.5, 2.5, n).astype(F)          # some negative: stored as 0
        return c

    def upload(self, t, first=0, count=None):
        sl = slice(first, len(self.type) if count is None else first + count)
        t.upload_colliders(first, self.type[sl], self.he[sl], self.radius[sl], self.hh[sl])
        self.hh[sl] = np.maximum(self.hh[sl], F(0.0))

    def witness(self, ow, n):
        bmn, bmx = ow.world_aabbs()
        return boxes(ow.world_matrices()[:n], self.type[:n], self.he[:n], self.radius[:n], self.hh[:n], bmn[:n], bmx[:n])
