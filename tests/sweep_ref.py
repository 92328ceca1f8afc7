"""Witness of the capsule sweeps (include/sc_tick.h "capsule sweeps"), independent of the kernels: numpy
fp32, one rounding per operation, left to right, and the oracle's brute-force ray test over explicit boxes.

    sweeper   hh = max(0, half_height);  e = (radius, hh + radius, radius)
    segment   d = end - start;  lenSq = (d.x d.x + d.y d.y) + d.z d.z;  lenSq > 1e-6: far = sqrt(lenSq), else an overlap test at start
    test      oracle.raycast_boxes(lo - e, hi + e, group, mask, start, d, far, query_mask): the oracle normalises d as the spec does
              (1 / sqrt(lenSq)), so its distance is t; distance = t / far, travel = t
    skip_id   the box takes no part (its group is masked out for that query)
    overlap   closed containment of start in the grown boxes, lowest id (the oracle rejects a zero direction)

A box that does not exist (min > max on an axis, or NaN: no Bounds, collider NONE) stays non-existent however far it is grown."""
import numpy as np

F = np.float32
NO_ID = 0xFFFFFFFF
HIT_DTYPE = np.dtype([("hit", np.uint32), ("id", np.uint32), ("distance", np.float32), ("position", np.float32, 3),
                      ("normal", np.float32, 3), ("layer", np.uint32), ("travel", np.float32), ("pad", np.uint32)])


def half_extents(radius, half_height):
    r = np.ascontiguousarray(radius, F).reshape(-1)
    hh = np.maximum(F(0.0), np.ascontiguousarray(half_height, F).reshape(-1))
    e = np.stack([r, hh + r, r], axis=1)
    assert e.dtype == F
    return e


def segments(start, end):
    """(d, far, moving): far = 0 and moving False where the query is an overlap test."""
    a, b = np.ascontiguousarray(start, F).reshape(-1, 3), np.ascontiguousarray(end, F).reshape(-1, 3)
    d = b - a
    len_sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    moving = len_sq > F(1e-6)
    far = np.where(moving, np.sqrt(len_sq), F(0.0)).astype(F)
    assert d.dtype == F and len_sq.dtype == F
    return d, far, moving


def grown(mn, mx, e):
    mn, mx = np.ascontiguousarray(mn, F), np.ascontiguousarray(mx, F)
    with np.errstate(invalid="ignore"):
        exists = (mn <= mx).all(axis=1)
        lo, hi = mn - e, mx + e
    lo[~exists], hi[~exists] = np.inf, -np.inf
    return lo, hi


def sweep_boxes(oracle, mn, mx, group, mask, start, end, radius, half_height, query_mask, skip_id=None):
    """Structured array like WorldTick.sweep_hits() for every query, against the boxes (mn, mx) with their layers."""
    a = np.ascontiguousarray(start, F).reshape(-1, 3)
    k = len(a)
    group, mask = np.ascontiguousarray(group, np.uint32), np.ascontiguousarray(mask, np.uint32)
    qm = np.ascontiguousarray(query_mask, np.uint32).reshape(k)
    skip = np.full(k, NO_ID, np.uint32) if skip_id is None else np.ascontiguousarray(skip_id, np.uint32).reshape(k)
    e = half_extents(radius, half_height)
    d, far, moving = segments(a, end)
    out = np.zeros(k, HIT_DTYPE)
    out["id"] = NO_ID
    out["normal"][:, 1] = 1.0
    # one oracle call per distinct sweeper (the oracle takes one set of boxes) and per skipped box
    keys = np.concatenate([e.view(np.uint32), skip.reshape(-1, 1)], axis=1)
    _, inverse = np.unique(keys, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    for u in range(inverse.max() + 1 if k else 0):
        sel = np.flatnonzero(inverse == u)
        lo, hi = grown(mn, mx, e[sel[0]])
        g = group
        if skip[sel[0]] != NO_ID and skip[sel[0]] < len(g):
            g = group.copy(); g[skip[sel[0]]] = 0
        mv = sel[moving[sel]]
        if len(mv):
            r = oracle.raycast_boxes(lo, hi, g, mask, a[mv], d[mv], far[mv], qm[mv])
            for f in ("hit", "id", "position", "normal", "layer"):
                out[f][mv] = r[f]
            out["travel"][mv] = r["distance"]
            out["distance"][mv] = np.where(r["hit"] == 1, r["distance"] / far[mv], F(0.0)).astype(F)
        for q in sel[~moving[sel]]:
            ok = ((g & 0xFFFF & qm[q]) != 0) & ((mask & 0xFFFF) != 0)
            with np.errstate(invalid="ignore"):
                inside = ok & (lo[:, 0] <= hi[:, 0]) & ((a[q] >= lo) & (a[q] <= hi)).all(axis=1)
            ids = np.flatnonzero(inside)
            if len(ids):
                out["hit"][q], out["id"][q], out["layer"][q] = 1, ids[0], g[ids[0]] & 0xFFFF
                out["position"][q] = a[q] + F(0.0) * F(0.0)          # start + ndir * t with ndir = 0, t = 0
    return out
