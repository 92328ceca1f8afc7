"""Witness of the overlap queries (include/sc_tick.h "overlap queries"), assembled from the witnesses the project already has -- no
arithmetic of its own.  A volume is a collider without an entity:

    its box        tests/collider_ref.py::typed_boxes over its matrix
    AABB mode      the oracle's broadphase_bruteforce over the entities' boxes plus the volumes' boxes, a volume carrying the layers
                   group 0xFFFF, mask = the query's mask (the rays' filter); only (entity, volume) pairs are kept, minus skip_id
    EXACT mode     tests/pair_shapes_ref.py::touching32 over those hits, the volumes appended as rows n .. n + k - 1 of the matrices and
                   of the collider arrays, the pairs given as (entity, n + q): the entity is member A, the volume member B

Volumes: a dict of arrays type, m16, he, radius, hh, mask and skip (None or ids)."""
import numpy as np

from tests import collider_ref as cr, pair_shapes_ref as R

F = np.float32
U = np.uint32
NO_SKIP = 0xFFFFFFFF
CHUNK = 64                      # volumes per brute-force call: volumes pass the filter against each other, and those pairs are dropped


def volumes(type, m16, he, radius, hh, mask, skip=None):
    k = len(np.asarray(type).reshape(-1))
    return dict(type=np.ascontiguousarray(type, np.uint8).reshape(k), m16=np.ascontiguousarray(m16, F).reshape(k, 16),
                he=np.ascontiguousarray(he, F).reshape(k, 3), radius=np.ascontiguousarray(radius, F).reshape(k),
                hh=np.ascontiguousarray(hh, F).reshape(k), mask=np.ascontiguousarray(mask, U).reshape(k),
                skip=None if skip is None else np.ascontiguousarray(skip, U).reshape(k))


def take(vol, idx):
    """the volumes idx of a set"""
    return {k: (None if v is None else v[idx]) for k, v in vol.items()}


def args(vol):
    """what WorldTick.overlap_queries takes, in its order"""
    return vol["type"], vol["m16"], vol["he"], vol["radius"], vol["hh"], vol["mask"], vol["skip"]


def volume_boxes(vol):
    return cr.typed_boxes(vol["m16"], vol["type"], vol["he"], vol["radius"], vol["hh"])


def aabb_hits(oracle, mn, mx, group, mask, vol, rank=0):
    """[(entity, volume)] of AABB mode as an [h, 2] array of dense indices, sorted by volume, then entity"""
    mn, mx = np.ascontiguousarray(mn, F).reshape(-1, 3), np.ascontiguousarray(mx, F).reshape(-1, 3)
    n, k = len(mn), len(vol["type"])
    vmn, vmx = volume_boxes(vol)
    group, mask = np.ascontiguousarray(group, U), np.ascontiguousarray(mask, U)
    out = []
    for lo in range(0, k, CHUNK):
        hi = min(k, lo + CHUNK)
        pairs = oracle.broadphase_bruteforce(np.concatenate([mn, vmn[lo:hi]]), np.concatenate([mx, vmx[lo:hi]]),
                                             np.concatenate([group, np.full(hi - lo, 0xFFFF, U)]), np.concatenate([mask, vol["mask"][lo:hi]]))
        pairs = np.ascontiguousarray(pairs, U).reshape(-1, 2).astype(np.int64)
        pairs = pairs[(pairs[:, 0] < n) & (pairs[:, 1] >= n)]
        pairs[:, 1] += lo - n
        out.append(pairs)
    hits = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    if vol["skip"] is not None and len(hits):
        hits = hits[(hits[:, 0] | (rank << 24)) != vol["skip"][hits[:, 1]].astype(np.int64)]
    return hits[np.lexsort((hits[:, 0], hits[:, 1]))]


def with_volumes(matrices, col, vol, n):
    """(matrices, colliders) of n entities with the volumes appended as rows n .. n + k - 1"""
    k = len(vol["type"])
    m = np.concatenate([np.ascontiguousarray(matrices, F).reshape(-1, 16)[:n], vol["m16"]])
    both = cr.Colliders(n + k)
    both.type[:n], both.he[:n], both.radius[:n], both.hh[:n] = col.type[:n], col.he[:n], col.radius[:n], col.hh[:n]
    both.type[n:], both.he[n:], both.radius[n:], both.hh[n:] = vol["type"], vol["he"], vol["radius"], vol["hh"]
    return m, both


def exact_hits(hits, matrices, col, vol, n):
    """(touching, refined) per row of the AABB-mode hits: touching32 over the pairs (entity, n + q).  col None: a context without
    colliders -- every hit stands on its box answer."""
    if col is None or not len(hits):
        return np.ones(len(hits), bool), np.zeros(len(hits), bool)
    m, both = with_volumes(matrices, col, vol, n)
    pairs = np.stack([hits[:, 0], hits[:, 1] + n], axis=1).astype(U)
    return R.touching32(m, both, pairs)


def answer(hits, k, max_hits, shapes=0, touching=None, refined=None):
    """(id sets per volume, counts, info) as scTickReadOverlapHits must report them (rank 0)"""
    keep = np.ones(len(hits), bool) if touching is None else touching
    sets = [np.sort(hits[keep & (hits[:, 1] == q), 0]).astype(U) for q in range(k)]
    counts = np.array([len(s) for s in sets], U)
    info = dict(queries=k, max_hits=max_hits, hits=int(counts.sum()), truncated_queries=int((counts > max_hits).sum()),
                refined=0 if refined is None else int(refined.sum()), kept_as_boxes=0 if refined is None else int((keep & ~refined).sum()),
                shapes=shapes)
    return sets, counts, info
