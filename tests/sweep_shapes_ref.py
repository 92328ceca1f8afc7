"""Witnesses of the exact shapes for capsule sweeps (include/sc_tick.h "exact shapes for capsule sweeps"), independent
of the kernels.

    advance32    numpy fp32 written from the header text: one rounding per operation, left to right.  The advancement of one sweeper towards
                 one refinable target, vectorised over (sweep, target) pairs.  Where the header says "routine 1 / routine 2 of the touching
                 pairs" the arithmetic is tests/pair_shapes_ref.py's: its clamp01, its round and frame builders, its F and its sorting
                 network; the closed forms are restated here only because the sweeps also need the closest points.
    sweep32      the whole query: brute force over every entity for every sweep -- filter, skip, the grown-AABB slab test (the rays' slab
                 routine of tests/shape_rays_ref.py), refinement of the refinable candidates, the winner, and the report's words.  In AABB mode
                 it must equal tests/sweep_ref.py's sweep_boxes bit for bit (tests/test_sweep_shapes_cpu.py checks that).
    contact64    float64 and another route: gap64(t) from pair_shapes_ref's float64 distance (golden-section minimisation of the exact
                 point-segment / point-box distance), the first contact by a dense scan of [0, far] plus bisection.  No step rule, no secant.

    dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z      c_k = column k      T = translation      n_k = dot(c_k, c_k)"""
import numpy as np

from tests import collider_ref as cr, pair_shapes_ref as ps, sweep_ref
from tests.shape_rays_ref import dot, shape_records, slab

F = np.float32
ZERO, ONE, HALF = F(0.0), F(1.0), F(0.5)
TOL = F(1e-3)                                                  # SC_TICK_SWEEP_SHAPES_TOL
STEPS = 12                                                     # SC_TICK_SWEEP_SHAPES_STEPS
AABB, EXACT = 0, 1
NO_ID = sweep_ref.NO_ID
HIT_DTYPE = sweep_ref.HIT_DTYPE
MISS, HIT = 1, 2
INFO_FIELDS = ("refined", "kept_as_boxes", "exhausted")


def seg_seg(p1, d1, p2, d2):
    """routine 1's closed form over 3-lists of 1-D fp32 arrays: (dot(v, v), v) with v = (p1 + d1*s) - (p2 + d2*t)"""
    r = [p1[i] - p2[i] for i in range(3)]
    a, e, f = dot(d1, d1), dot(d2, d2), dot(d2, r)
    c, b = dot(d1, r), dot(d1, d2)
    den = a * e - b * b
    s_0 = np.zeros_like(a)
    t_0 = np.where(e > ZERO, ps.clamp01(f / e), ZERO)
    s_1 = ps.clamp01((-c) / a)
    t_1 = np.zeros_like(a)
    s_2 = np.where(den > ZERO, ps.clamp01((b * f - c * e) / den), ZERO).astype(F)
    t_2 = (b * s_2 + f) / e
    below, above = t_2 < ZERO, ~(t_2 < ZERO) & (t_2 > ONE)
    s_2 = np.where(below, ps.clamp01((-c) / a), np.where(above, ps.clamp01((b - c) / a), s_2))
    t_2 = np.where(below, ZERO, np.where(above, ONE, t_2))
    has_a, has_e = a > ZERO, e > ZERO
    s = np.where(~has_a, s_0, np.where(~has_e, s_1, s_2)).astype(F)
    t = np.where(~has_a, t_0, np.where(~has_e, t_1, t_2)).astype(F)
    v = [(p1[i] + d1[i] * s) - (p2[i] + d2[i] * t) for i in range(3)]
    d2_ = dot(v, v)
    assert d2_.dtype == F
    return d2_, v


def seg_box(y0, dy, H, segment):
    """routine 2's fifteen evaluations: (fmin, at) -- the first strictly smaller value in the routine's order keeps its parameter;
    segment False: a point, one evaluation"""
    f0 = ps._box_dist2(y0, dy, H, ZERO)
    fmin, at = f0, np.zeros_like(f0)

    def take(fmin, at, x, t):
        better = x < fmin
        return np.where(better, x, fmin), np.where(better, t, at).astype(F)

    fmin, at = take(fmin, at, ps._box_dist2(y0, dy, H, ONE), np.ones_like(f0))
    b = [np.zeros_like(f0)] + [None] * 6 + [np.ones_like(f0)]
    for k in range(3):
        b[1 + 2 * k] = ps.clamp01((H[k] - y0[k]) / dy[k])
        b[2 + 2 * k] = ps.clamp01(((-H[k]) - y0[k]) / dy[k])
    for i, j in ps.NETWORK:
        swap = b[j] < b[i]
        b[i], b[j] = np.where(swap, b[j], b[i]), np.where(swap, b[i], b[j])
    for i in range(7):
        lo, hi = b[i], b[i + 1]
        tm = (lo + hi) * HALF
        num, den = [], []
        for k in range(3):
            y = y0[k] + dy[k] * tm
            out = np.abs(y) - H[k] > ZERO
            face = np.where(y > ZERO, H[k], -H[k])
            num.append(np.where(out, (y0[k] - face) * dy[k], ZERO).astype(F))
            den.append(np.where(out, dy[k] * dy[k], ZERO).astype(F))
        ns, ds = (num[0] + num[1]) + num[2], (den[0] + den[1]) + den[2]
        ts = np.where(ds > ZERO, (-ns) / ds, lo)
        ts = np.where(ts < lo, lo, ts)
        ts = np.where(ts > hi, hi, ts).astype(F)
        fmin, at = take(fmin, at, ps._box_dist2(y0, dy, H, ts), ts)
        if i < 6:
            fmin, at = take(fmin, at, ps._box_dist2(y0, dy, H, hi), hi)
    fmin, at = np.where(segment, fmin, f0), np.where(segment, at, ZERO).astype(F)
    assert fmin.dtype == F and at.dtype == F
    return fmin, at


class Targets:
    """the refinable targets e (1-D dense indices) of matrices m as the advancement takes them: built once, outside the step loop"""

    def __init__(self, m, typ, shp, e):
        col, T, n, s = ps._members(m, shp, e)
        self.box = typ[e] == cr.BOX
        self.T = T
        self.At, self.Rt = ps._round(col, n, s, typ[e])
        self.u, self.H = ps._frame(col, n, s)


def dist2_32(tg, o, d, ay, t):
    """(dist2, v = ps - pt) of the sweeper at travel t (o, d: 3-lists; ay: the sweeper's half axis)"""
    zero = np.zeros_like(ay)
    A = [zero, ay, zero]
    d1 = [A[i] + A[i] for i in range(3)]
    c = [o[i] + d[i] * t for i in range(3)]
    # a round target
    p1 = [c[i] - A[i] for i in range(3)]
    p2 = [tg.T[i] - tg.At[i] for i in range(3)]
    d2v = [tg.At[i] + tg.At[i] for i in range(3)]
    rr, rv = seg_seg(p1, d1, p2, d2v)
    # a box
    w = [c[i] - tg.T[i] for i in range(3)]
    ya = [dot(tg.u[k], A) for k in range(3)]
    y0 = [dot(tg.u[k], w) - ya[k] for k in range(3)]
    dy = [ya[k] + ya[k] for k in range(3)]
    fmin, at = seg_box(y0, dy, tg.H, ay != ZERO)
    z = []
    for k in range(3):
        y = y0[k] + dy[k] * at
        lo = np.where(y < -tg.H[k], -tg.H[k], y)
        z.append(np.where(lo > tg.H[k], tg.H[k], lo).astype(F))
    bv = []
    for i in range(3):
        ps_ = (c[i] - A[i]) + d1[i] * at
        pt = ((tg.u[0][i] * z[0] + tg.u[1][i] * z[1]) + tg.u[2][i] * z[2]) + tg.T[i]
        bv.append(ps_ - pt)
    dist2 = np.where(tg.box, fmin, rr).astype(F)
    v = [np.where(tg.box, bv[i], rv[i]).astype(F) for i in range(3)]
    return dist2, v


def advance32(m, typ, shp, e, o, d, far, radius, hh, t0, steps=STEPS, tol=TOL):
    """The header's advancement for pairs (sweep, target e): (kind MISS / HIT, t, normal[3], exhausted, evaluations).  o, d: 3-lists of 1-D
    fp32 arrays (start, ndir); far, radius, hh (>= 0), t0: 1-D fp32."""
    k = len(e)
    with np.errstate(all="ignore"):
        tg = Targets(m, typ, shp, e)
        ay = np.where(hh * hh > ZERO, hh, ZERO).astype(F)
        Rs = np.where(tg.box, radius, radius + tg.Rt).astype(F)
        t = np.asarray(t0, F).copy()
        tp, gp = np.zeros(k, F), np.zeros(k, F)
        prev = np.zeros(k, bool)
        live = np.ones(k, bool)
        kind = np.full(k, MISS, np.int32)
        rt = np.zeros(k, F)
        nrm = [np.zeros(k, F), np.ones(k, F), np.zeros(k, F)]
        evals = np.zeros(k, np.int32)
        v = [np.zeros(k, F) for _ in range(3)]

        def hit_with_normal(sel):
            vv = dot(v, v)
            q = np.sqrt(vv)
            for i in range(3):
                nrm[i][sel] = np.where(vv > ZERO, v[i] / q, nrm[i])[sel]
            kind[sel] = HIT
            rt[sel] = t[sel]

        for _ in range(steps):
            if not live.any():
                break
            d2_, vn = dist2_32(tg, o, d, ay, t)
            for i in range(3):
                v[i] = np.where(live, vn[i], v[i])
            evals += live
            inside = live & (t == ZERO) & ~(d2_ > Rs * Rs)
            kind[inside] = HIT                                                   # t = +0, normal (0, 1, 0)
            live &= ~inside
            g = np.sqrt(d2_) - Rs
            met = live & (g <= tol)
            hit_with_normal(met)
            live &= ~met
            live &= ~(far == ZERO)                                               # an overlap test: one evaluation
            step = g
            slope = (g - gp) / (t - tp)
            live &= ~(prev & ~(slope < ZERO))
            sec = (-g) / slope
            step = np.where(prev & (sec > step), sec, step)
            tp, gp = np.where(live, t, tp), np.where(live, g, gp)
            prev |= live
            t = np.where(live, t + step, t).astype(F)
            live &= ~(t > far)
        exhausted = live.copy()
        hit_with_normal(live)
    assert rt.dtype == F and all(x.dtype == F for x in nrm)
    return kind, rt, nrm, exhausted, evals


def sweep32(matrices, mn, mx, group, mask, col, start, end, radius, half_height, query_mask, skip_id=None, mode=EXACT, own=None, n=None,
            chunk=128, detail=False):
    """(hits like WorldTick.sweep_hits(), report dict).  col: the Colliders host model (None: a context without colliders -- nothing is
    refined); skip_id: per sweep a box id that never answers; own: which entities are the answering context's own (default all);
    n: the entity count (default every box).  detail: also the per-candidate arrays (sweep, entity, kind, t, exhausted, evaluations)."""
    mn, mx = np.ascontiguousarray(mn, F).reshape(-1, 3), np.ascontiguousarray(mx, F).reshape(-1, 3)
    n = len(mn) if n is None else n
    mn, mx = mn[:n], mx[:n]
    m = np.ascontiguousarray(matrices, F).reshape(-1, 16)[:n]
    g16 = np.ascontiguousarray(group, np.uint32)[:n] & 0xFFFF
    m16 = np.ascontiguousarray(mask, np.uint32)[:n] & 0xFFFF
    a = np.ascontiguousarray(start, F).reshape(-1, 3)
    k = len(a)
    qm = np.ascontiguousarray(query_mask, np.uint32).reshape(k)
    skip = np.full(k, NO_ID, np.uint32) if skip_id is None else np.ascontiguousarray(skip_id, np.uint32).reshape(k)
    e3 = sweep_ref.half_extents(radius, half_height)
    rad = e3[:, 0]
    hh = np.maximum(ZERO, np.ascontiguousarray(half_height, F).reshape(k))
    dv, far, moving = sweep_ref.segments(a, end)
    with np.errstate(all="ignore"):
        inv = ONE / far
        nd = np.where(moving[:, None], dv * inv[:, None], ZERO).astype(F)
    typ, shp = shape_records(col, n) if col is not None else (np.zeros(n, np.uint8), np.zeros((n, 4), F))
    ids = np.arange(n)
    e_ok = np.ones(n, bool) if own is None else np.asarray(own, bool)[:n]
    refinable = ps.refinable(m, typ, e_ok, ids) if col is not None and n else np.zeros(n, bool)
    with np.errstate(invalid="ignore"):
        has_box = (mn <= mx).all(axis=1)
    out = np.zeros(k, HIT_DTYPE)
    out["id"] = NO_ID
    out["normal"][:, 1] = 1.0
    info = dict.fromkeys(INFO_FIELDS, 0)
    rows = []
    for c0 in range(0, k if n else 0, chunk):
        rs = np.arange(c0, min(c0 + chunk, k))
        O = [a[rs, i][:, None] for i in range(3)]
        D = [nd[rs, i][:, None] for i in range(3)]
        with np.errstate(invalid="ignore"):
            lo = [mn[:, i][None] - e3[rs, i][:, None] for i in range(3)]
            hi = [mx[:, i][None] + e3[rs, i][:, None] for i in range(3)]
        hit, t, axis = slab(O, D, far[rs][:, None], lo, hi)
        cand = hit & has_box[None] & ((g16[None] & qm[rs][:, None]) != 0) & (m16[None] != 0) & (ids[None] != skip[rs][:, None].astype(np.int64))
        da = np.select([axis == 0, axis == 1, axis == 2], [np.broadcast_to(D[0], axis.shape), np.broadcast_to(D[1], axis.shape),
                                                           np.broadcast_to(D[2], axis.shape)], ZERO)
        sgn = np.where(da > ZERO, F(-1.0), ONE)
        nrm = [np.where(axis == i, sgn, ZERO).astype(F) for i in range(3)]
        nrm[1] = np.where(axis == 3, ONE, nrm[1])
        t = t.copy()
        if mode == EXACT:
            ri, ei = np.nonzero(cand & refinable[None])
            info["kept_as_boxes"] += int((cand & ~refinable[None]).sum())
            info["refined"] += len(ri)
            if len(ri):
                q = rs[ri]
                kind, rt, rn, ex, ev = advance32(m, typ, shp, ei, [a[q, i] for i in range(3)], [nd[q, i] for i in range(3)], far[q], rad[q], hh[q],
                                                 t[ri, ei])
                info["exhausted"] += int(ex.sum())
                cand[ri[kind == MISS], ei[kind == MISS]] = False
                h = kind == HIT
                t[ri[h], ei[h]] = rt[h]
                for i in range(3):
                    nrm[i][ri[h], ei[h]] = rn[i][h]
                if detail:
                    rows.append(np.stack([q, ei, kind, rt.view(np.uint32), ex, ev], axis=1))
        tt = np.where(cand, t, np.inf)
        win = np.argmin(tt, axis=1)                       # the first of equal travels: the lower id
        rr = np.arange(len(rs))
        found = cand[rr, win]
        w, r = win[found], rs[found]
        bt = t[rr[found], w]
        out["hit"][r] = 1
        out["id"][r] = w
        out["travel"][r] = bt
        with np.errstate(all="ignore"):
            out["distance"][r] = np.where(far[r] > ZERO, bt / far[r], ZERO)
        out["layer"][r] = g16[w]
        out["position"][r] = a[r] + nd[r] * bt[:, None]
        for i in range(3):
            out["normal"][r, i] = nrm[i][rr[found], w]
    if detail:
        return out, info, (np.concatenate(rows) if rows else np.zeros((0, 6), np.int64))
    return out, info


# ---- float64, by another route --------------------------------------------------------------------------------------
def gap64(m, typ, shp, e, centre, radius, hh, iters=64):
    """signed gap in metres between the upright capsule (centre [k][3] float64, radius, hh) and the colliders of entities e: the float64
    distance of tests/pair_shapes_ref.py -- golden-section minimisation over the sweeper's segment of the exact point-segment / point-box
    distance -- for matrices with orthogonal columns"""
    e = np.asarray(e, np.int64)
    k = len(e)
    col, T, nk, s = ps._members64(m, shp, e)
    box = typ[e] == cr.BOX
    At, Rt = ps._round64(col, nk, s, typ[e])
    At[box] = 0.0
    centre = np.asarray(centre, np.float64).reshape(k, 3)
    A = np.zeros((k, 3)); A[:, 1] = np.asarray(hh, np.float64)
    R = np.asarray(radius, np.float64)
    with np.errstate(all="ignore"):
        u = [col[j] / np.sqrt(nk[j])[:, None] for j in range(3)]
        H = np.stack([s[:, j] * np.sqrt(nk[j]) for j in range(3)], axis=1)
    rr = ps._golden(lambda t: ps._point_segment(centre - A + 2.0 * A * t[:, None], T - At, 2.0 * At), k, iters) - (R + Rt)

    def to_box(t):
        q = centre - A + 2.0 * A * t[:, None] - T
        y = np.stack([np.einsum("ij,ij->i", q, u[j]) for j in range(3)], axis=1)
        return np.linalg.norm(np.maximum(np.abs(y) - H, 0.0), axis=1)

    rb = ps._golden(to_box, k, iters) - R
    return np.where(box, rb, rr)


def contact64(m, typ, shp, e, start, ndir, far, radius, hh, samples=257, bisect=44):
    """First contact of sweeps (start, ndir, far) with the colliders of e, in float64: (hit, t, slope at t, minimum gap over [0, far]).
    A dense scan of [0, far] finds the first sample with gap <= 0, bisection between it and the sample before finds the crossing; the
    minimum gap is refined by golden section around the lowest sample.  hit with t = 0 when the sweep starts in contact."""
    e = np.asarray(e, np.int64)
    k = len(e)
    start, ndir = np.asarray(start, np.float64).reshape(k, 3), np.asarray(ndir, np.float64).reshape(k, 3)
    far, radius, hh = (np.asarray(x, np.float64).reshape(k) for x in (far, radius, hh))

    def g(t, sel=slice(None)):
        return gap64(m, typ, shp, e[sel], start[sel] + ndir[sel] * t[:, None], radius[sel], hh[sel])

    ts = np.linspace(0.0, 1.0, samples)[None] * far[:, None]                    # [k][samples]
    rep = np.repeat(np.arange(k), samples)
    gs = gap64(m, typ, shp, e[rep], start[rep] + ndir[rep] * ts.reshape(-1)[:, None], radius[rep], hh[rep]).reshape(k, samples)
    below = gs <= 0.0
    hit = below.any(axis=1)
    first = np.argmax(below, axis=1)
    t = np.zeros(k)
    slope = np.zeros(k)
    # the minimum gap: golden section over the two intervals next to the lowest sample (gap is convex in t)
    low = np.argmin(gs, axis=1)
    a_, b_ = ts[np.arange(k), np.maximum(low - 1, 0)], ts[np.arange(k), np.minimum(low + 1, samples - 1)]
    gold = (np.sqrt(5.0) - 1.0) / 2.0
    x1, x2 = b_ - gold * (b_ - a_), a_ + gold * (b_ - a_)
    g1, g2 = g(x1), g(x2)
    for _ in range(40):
        left = g1 < g2
        b_ = np.where(left, x2, b_); a_ = np.where(left, a_, x1)
        x1, x2 = b_ - gold * (b_ - a_), a_ + gold * (b_ - a_)
        g1, g2 = g(x1), g(x2)
    gmin = np.minimum(np.minimum(g1, g2), gs.min(axis=1))
    cross = np.flatnonzero(hit & (first > 0))
    if len(cross):
        lo, hi = ts[cross, first[cross] - 1], ts[cross, first[cross]]
        for _ in range(bisect):
            mid = 0.5 * (lo + hi)
            neg = g(mid, cross) <= 0.0
            hi = np.where(neg, mid, hi); lo = np.where(neg, lo, mid)
        t[cross] = hi
        h = 1e-4
        slope[cross] = (g(hi + h, cross) - g(hi - h, cross)) / (2.0 * h)
    return hit, t, slope, gmin
