"""Witness of the entity-anchored rays (include/sc_tick.h "entity-anchored rays"), independent of the kernels:
numpy fp32, one rounding per operation, left to right, around the oracle's brute-force ray test over explicit boxes.

    resolve   R_r = row r of the anchor's world matrix (the oracle's world_matrices(), column-major: R_r = m[r], m[4 + r], m[8 + r], m[12 + r])
              o_r = ((R_r.x l.x + R_r.y l.y) + R_r.z l.z) + R_r.w        d_r = (R_r.x v.x + R_r.y v.y) + R_r.z v.z
    cast      oracle.raycast_boxes(boxes, o, d, max_dist, mask): max_dist is world metres, the oracle normalises d as the rays' spec does
    skip_self the anchor's box takes no part: its group is masked out, one oracle call per distinct skipped box (as tests/sweep_ref.py)
    no anchor ANCHOR_NONE: (l, v) are world space and go to the oracle untouched
    a miss    an anchor >= the entity count (ANCHOR_DEAD is), a resolved origin that is not finite, a resolved direction whose squared
              length (d.x d.x + d.y d.y) + d.z d.z is not finite: RaycastHit{} without asking the oracle"""
import numpy as np

F = np.float32
ANCHOR_NONE, ANCHOR_DEAD = 0xFFFFFFFF, 0xFFFFFFFE
NO_ID = 0xFFFFFFFF
HIT_DTYPE = np.dtype([("hit", np.uint32), ("id", np.uint32), ("distance", np.float32), ("position", np.float32, 3),
                      ("normal", np.float32, 3), ("layer", np.uint32), ("pad", np.uint32, 2)])


def resolve(matrices, anchor, local_origin, local_dir):
    """(o, d, ok): world-space origin and direction of every ray, ok False where the ray misses by rule.  Rays without an anchor
    come back as given."""
    m = np.ascontiguousarray(matrices, F).reshape(-1, 16)
    an = np.ascontiguousarray(anchor, np.uint32).reshape(-1)
    l, v = np.ascontiguousarray(local_origin, F).reshape(-1, 3), np.ascontiguousarray(local_dir, F).reshape(-1, 3)
    o, d = l.copy(), v.copy()
    ok = np.ones(len(an), bool)
    free = an == ANCHOR_NONE
    gone = ~free & (an >= len(m))
    ok[gone] = False
    at = np.flatnonzero(~free & ~gone)
    if len(at):
        a = an[at]
        with np.errstate(all="ignore"):
            for r in range(3):
                rx, ry, rz, rw = m[a, r], m[a, 4 + r], m[a, 8 + r], m[a, 12 + r]
                o[at, r] = ((rx * l[at, 0] + ry * l[at, 1]) + rz * l[at, 2]) + rw
                d[at, r] = (rx * v[at, 0] + ry * v[at, 1]) + rz * v[at, 2]
            len_sq = (d[at, 0] * d[at, 0] + d[at, 1] * d[at, 1]) + d[at, 2] * d[at, 2]
        assert o.dtype == F and d.dtype == F and len_sq.dtype == F
        ok[at] = np.isfinite(o[at]).all(axis=1) & np.isfinite(len_sq)
    return o, d, ok


def cast(oracle, mn, mx, group, mask, matrices, anchor, local_origin, local_dir, max_dist, query_mask, skip_self=None, skip_ids=None):
    """Structured array like WorldTick.anchored_ray_hits() against the boxes (mn, mx) with their layers.  skip_ids: the index among
    the boxes that each anchor's own box has (default: the anchor itself -- one context, boxes in dense order)."""
    an = np.ascontiguousarray(anchor, np.uint32).reshape(-1)
    k = len(an)
    group, mask = np.ascontiguousarray(group, np.uint32), np.ascontiguousarray(mask, np.uint32)
    md, qm = np.ascontiguousarray(max_dist, F).reshape(k), np.ascontiguousarray(query_mask, np.uint32).reshape(k)
    sk = np.ones(k, bool) if skip_self is None else np.ascontiguousarray(skip_self, np.uint8).reshape(k) != 0
    own = an.astype(np.int64) if skip_ids is None else np.ascontiguousarray(skip_ids, np.int64).reshape(k)
    o, d, ok = resolve(matrices, an, local_origin, local_dir)
    out = np.zeros(k, HIT_DTYPE)
    out["id"] = NO_ID
    out["normal"][:, 1] = 1.0
    skipped = np.where(ok & sk & (an != ANCHOR_NONE), own, -1)
    for s in np.unique(skipped[ok]) if ok.any() else []:
        sel = np.flatnonzero(ok & (skipped == s))
        g = group
        if 0 <= s < len(g):
            g = group.copy(); g[s] = 0
        out[sel] = oracle.raycast_boxes(mn, mx, g, mask, o[sel], d[sel], md[sel], qm[sel])
    return out
