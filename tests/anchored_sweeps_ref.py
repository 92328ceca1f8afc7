"""Witness of the entity-anchored capsule sweeps (include/sc_tick.h "entity-anchored capsule sweeps"), independent of
the kernels.  It restates nothing:

    resolve   the point formula is tests/anchored_ref.py's resolve, called once for the local starts and once for the local ends, with a
              zero direction; the offset frame (end_frame 1) is one fp32 add, e_r = s_r + le_r
    status    1: an anchor >= the entity count (ANCHOR_DEAD is); 2: a component of s or e, or (d.x d.x + d.y d.y) + d.z d.z of d = e - s,
              that is not finite.  Both are a miss (SweepHit{}) and their segment reads as the quiet NaN
    sweep     tests/sweep_ref.py's sweep_boxes (AABB mode) or tests/sweep_shapes_ref.py's sweep32 (EXACT mode) over the resolved segments
    skip_id   the anchor's own id where skip_self is set and the sweep has an anchor, else none"""
import numpy as np

from tests import anchored_ref, sweep_ref, sweep_shapes_ref as ss

F = np.float32
U = np.uint32
ANCHOR_NONE, ANCHOR_DEAD = anchored_ref.ANCHOR_NONE, anchored_ref.ANCHOR_DEAD
NO_ID = sweep_ref.NO_ID
HIT_DTYPE = sweep_ref.HIT_DTYPE
AABB, EXACT = ss.AABB, ss.EXACT
END_LOCAL, END_WORLD_OFFSET = 0, 1
ANSWERED, NO_ANCHOR, NOT_FINITE = 0, 1, 2
QNAN = np.array([0x7FC00000], U).view(F)[0]


def resolve(matrices, anchor, local_start, local_end, end_frame=None):
    """(s [k, 3], e [k, 3], status [k]) over the world matrices of the entities that exist (their number is the entity count)"""
    m = np.ascontiguousarray(matrices, F).reshape(-1, 16)
    an = np.ascontiguousarray(anchor, U).reshape(-1)
    k = len(an)
    ls, le = np.ascontiguousarray(local_start, F).reshape(k, 3), np.ascontiguousarray(local_end, F).reshape(k, 3)
    frame = np.zeros(k, np.uint8) if end_frame is None else np.ascontiguousarray(end_frame, np.uint8).reshape(k)
    zero = np.zeros((k, 3), F)
    s, _, _ = anchored_ref.resolve(m, an, ls, zero)
    as_point, _, _ = anchored_ref.resolve(m, an, le, zero)
    with np.errstate(all="ignore"):
        e = np.where((frame == END_WORLD_OFFSET)[:, None], s + le, as_point)
        d = e - s
        len_sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert s.dtype == F and e.dtype == F and len_sq.dtype == F
    status = np.zeros(k, U)
    status[~(np.isfinite(s).all(axis=1) & np.isfinite(e).all(axis=1) & np.isfinite(len_sq))] = NOT_FINITE
    status[(an != ANCHOR_NONE) & (an >= len(m))] = NO_ANCHOR
    s, e = s.copy(), e.copy()
    s[status != ANSWERED], e[status != ANSWERED] = QNAN, QNAN
    return s, e, status


def skip_ids(anchor, skip_self=None):
    an = np.ascontiguousarray(anchor, U).reshape(-1)
    sk = np.ones(len(an), bool) if skip_self is None else np.ascontiguousarray(skip_self, np.uint8).reshape(len(an)) != 0
    return np.where(sk & (an != ANCHOR_NONE), an, U(NO_ID)).astype(U)


def sweep(oracle, matrices, mn, mx, group, mask, col, anchor, local_start, local_end, radius, half_height, query_mask, skip_self=None,
          end_frame=None, mode=AABB):
    """(hits like WorldTick.anchored_sweep_hits() with pad = status, (s, e) like anchored_sweep_segments(), the EXACT report or None).
    matrices, mn, mx, group, mask: of the entities that exist; col: the Colliders host model or None."""
    s, e, status = resolve(matrices, anchor, local_start, local_end, end_frame)
    k = len(status)
    out = np.zeros(k, HIT_DTYPE)
    out["id"] = NO_ID
    out["normal"][:, 1] = 1.0
    out["pad"] = status
    at = np.flatnonzero(status == ANSWERED)
    r, hh = np.ascontiguousarray(radius, F).reshape(k), np.ascontiguousarray(half_height, F).reshape(k)
    qm, skip = np.ascontiguousarray(query_mask, U).reshape(k), skip_ids(anchor, skip_self)
    info = dict.fromkeys(ss.INFO_FIELDS, 0) if mode == EXACT else None
    if len(at):
        if mode == EXACT:
            hits, info = ss.sweep32(matrices, mn, mx, group, mask, col, s[at], e[at], r[at], hh[at], qm[at], skip_id=skip[at], mode=EXACT)
        else:
            hits = sweep_ref.sweep_boxes(oracle, mn, mx, group, mask, s[at], e[at], r[at], hh[at], qm[at], skip_id=skip[at])
        out[at] = hits
        out["pad"][at] = ANSWERED
    return out, (s, e), info


def resolve64(matrices, anchor, local_point):
    """float64 p_r = R_r.x l.x + R_r.y l.y + R_r.z l.z + R_r.w of every anchored point, and the bound of the fp32 formula's error per component:
    three multiplies and three adds, each within eps32 / 2 relative of a partial sum no larger than T = |R_r.x l.x| + |R_r.y l.y| +
    |R_r.z l.z| + |R_r.w| -- 4 * eps32 * T covers them with room to spare"""
    m = np.ascontiguousarray(matrices, F).reshape(-1, 16).astype(np.float64)
    an = np.ascontiguousarray(anchor, U).reshape(-1)
    l = np.ascontiguousarray(local_point, F).reshape(-1, 3).astype(np.float64)
    p, bound = np.zeros((len(an), 3)), np.zeros((len(an), 3))
    for r in range(3):
        terms = [m[an, r] * l[:, 0], m[an, 4 + r] * l[:, 1], m[an, 8 + r] * l[:, 2], m[an, 12 + r]]
        p[:, r] = terms[0] + terms[1] + terms[2] + terms[3]
        bound[:, r] = 4 * np.finfo(F).eps * sum(np.abs(t) for t in terms)
    return p, bound
