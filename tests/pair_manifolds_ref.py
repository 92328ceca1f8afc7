"""Witnesses of the pair manifolds (include/sc_tick.h "pair manifolds"), independent of the kernel.

    manifolds32  numpy fp32 written from the header text, operation by operation, over the listed pairs of a touching list (ids as
                 scTickReadPairShapes gives them), built on tests/pair_contacts_ref.py and tests/pair_shapes_ref.py: a structured array
                 (point[4][3], depth[4], count, kind, reserved[2]) the device must reproduce bit for bit; report() turns it into
                 ScTickPairManifoldInfo.
    float64, by another route: Witness64 -- the incident polygon cut by the reference prism as an intersection of half planes (every pair
                 of boundary lines intersected, the points inside all of them kept, ordered by angle), the capsule's stretch on a face and
                 two capsules' shared stretch by exact interval arithmetic on linear functions of the segment parameter.  For matrices
                 with orthogonal columns."""
import numpy as np

from tests import collider_ref as cr
from tests import pair_contacts_ref as K
from tests import pair_shapes_ref as R
from tests.pair_contacts_ref import clamp, image, pick, sign
from tests.pair_shapes_ref import F, ZERO, ONE, HALF, SAT_EPS, clamp01, dot
from tests.shape_rays_ref import shape_records

NONE, SINGLE, SEGMENT, FACE = 0, 1, 2, 3
REDUCED = 1 << 8
DTYPE = np.dtype([("point", F, (4, 3)), ("depth", F, 4), ("count", np.uint32), ("kind", np.uint32), ("reserved", np.uint32, 2)])
INFO_FIELDS = ("written", "points", "with_one", "with_two", "with_three", "with_four", "face", "reduced")
NEG = F(-1.0)
SLOTS = 8
SKIN32 = F(2.5e-4)                                             # SC_TICK_MANIFOLD_SKIN
FLAT32 = F(1e-3)                                               # SC_TICK_MANIFOLD_FLAT


def _two(keep, pts, pens):
    """the kept ones of two candidates in their order: (count, point[2][3] as lists of arrays, depth[2]), unused slots +0"""
    k0, k1 = keep
    count = k0.astype(np.int64) + k1.astype(np.int64)
    first = [np.where(k0, pts[0][c], pts[1][c]) for c in range(3)]
    first_d = np.where(k0, pens[0], pens[1])
    second = [np.where(k0 & k1, pts[1][c], ZERO).astype(F) for c in range(3)]
    second_d = np.where(k0 & k1, pens[1], ZERO).astype(F)
    return count, [[np.where(count > 0, first[c], ZERO).astype(F) for c in range(3)], second], [np.where(count > 0, first_d, ZERO).astype(F), second_d]


def _round_box_segment(mr, mx):
    """SEGMENT, a capsule on a box face: (count, points, depths); count 0 where the rule does not apply or keeps nothing"""
    (cr_, Tr, nr, sr_, tr), (cx, Tx, nx, sx, _) = mr, mx
    A, Rr = R._round(cr_, nr, sr_, tr)
    u, H = R._frame(cx, nx, sx)
    w = [Tr[i] - Tx[i] for i in range(3)]
    y0, dy = [], []
    for k in range(3):
        yc, ya = dot(u[k], w), dot(u[k], A)
        y0.append(yc - ya); dy.append(ya + ya)
    is_point = (A[0] == ZERO) & (A[1] == ZERO) & (A[2] == ZERO)
    fmin, at = K.seg_box(y0, dy, H, is_point)
    y = [y0[k] + dy[k] * at for k in range(3)]
    q = [clamp(y[k], H[k]) for k in range(3)]
    m = [H[k] - np.abs(y[k]) for k in range(3)]
    deep = ~(fmin > ZERO)
    kd, least = np.zeros(len(fmin), np.int64), m[0]
    for k in (1, 2):
        better = m[k] < least
        least, kd = np.where(better, m[k], least).astype(F), np.where(better, k, kd)
    out = [y[k] != q[k] for k in range(3)]
    n_out = out[0].astype(np.int64) + out[1] + out[2]
    kf = np.where(deep, kd, np.where(out[0], 0, np.where(out[1], 1, 2)))
    applies = ~is_point & (deep | (n_out == 1))
    sg = sign(pick(kf, y))
    lo, hi = np.zeros_like(fmin), np.ones_like(fmin)
    empty = np.zeros(len(fmin), bool)
    for k in range(3):
        use, moving = kf != k, dy[k] != ZERO
        b0, b1 = (H[k] - y0[k]) / dy[k], ((-H[k]) - y0[k]) / dy[k]
        tl, th = np.where(b1 < b0, b1, b0), np.where(b1 < b0, b0, b1)
        lo = np.where(use & moving & (tl > lo), tl, lo).astype(F)
        hi = np.where(use & moving & (th < hi), th, hi).astype(F)
        empty |= use & ~moving & (np.abs(y0[k]) > H[k])
    applies &= ~empty & (lo <= hi)
    yk0, dyk, hk = pick(kf, y0), pick(kf, dy), pick(kf, H)
    keep, pts, pens = [], [], []
    for end in range(2):
        t = hi if end else lo
        yk = yk0 + dyk * t
        up = sg * yk
        pen = Rr - (up - hk)
        # the end is R deep along the face's normal only where the line through it leaves the round at R: a centre line that lies flat on
        # the face, or a true end of it that the normal leaves on the far side of the segment
        dd = (dy[0] * dy[0] + dy[1] * dy[1]) + dy[2] * dy[2]
        flat = Rr * (dyk * dyk) <= FLAT32 * dd
        lean = sg * dyk
        outward = ((t == ONE) & (lean <= ZERO)) if end else ((t == ZERO) & (lean >= ZERO))
        least_ = hk - up
        back = least_ - (hk + hk)
        l = np.where(back < -Rr, -Rr, back).astype(F)
        h = np.where(least_ < Rr, least_, Rr).astype(F)
        ok = applies & (pen >= ZERO) & (flat | outward) & (l <= h)      # (l > h: the end lies beyond the opposite face, out of reach)
        if end:
            ok &= hi != lo
        mid = (l + h) * HALF
        x = [np.where(kf == k, yk + sg * mid, y0[k] + dy[k] * t).astype(F) for k in range(3)]
        keep.append(ok); pts.append(image(u, Tx, x)); pens.append(pen)
    return _two(keep, pts, pens)


def _round_round_segment(ma, mb, normal):
    """SEGMENT, capsule on capsule"""
    (ca, Ta, na, sa, ta), (cb, Tb, nb, sb, tb) = ma, mb
    Aa, Ra = R._round(ca, na, sa, ta)
    Ab, Rb = R._round(cb, nb, sb, tb)
    seg = ((Aa[0] != ZERO) | (Aa[1] != ZERO) | (Aa[2] != ZERO)) & ((Ab[0] != ZERO) | (Ab[1] != ZERO) | (Ab[2] != ZERO))
    p1 = [Ta[i] - Aa[i] for i in range(3)]; d1 = [Aa[i] + Aa[i] for i in range(3)]
    p2 = [Tb[i] - Ab[i] for i in range(3)]; d2 = [Ab[i] + Ab[i] for i in range(3)]
    a, e = dot(d1, d1), dot(d2, d2)
    total = Ra + Rb
    keep, pts, pens = [], [], []
    s0 = None
    for c in range(2):
        g = [p2[i] + d2[i] if c else p2[i] for i in range(3)]
        r = [g[i] - p1[i] for i in range(3)]
        s_raw = dot(r, d1) / a
        s = clamp01(s_raw)
        within = s == s_raw
        pa = [p1[i] + d1[i] * s for i in range(3)]
        w = [pa[i] - p2[i] for i in range(3)]
        t = clamp01(dot(w, d2) / e)
        v = [pa[i] - np.where(within, g[i], p2[i] + d2[i] * t) for i in range(3)]
        d2v = dot(v, v)
        dist = np.sqrt(d2v)
        pen = total - dist
        # ... and only where this candidate's own direction is the contact's normal, to within what FLAT allows the two radii
        wn = [((-v[i]) / dist) - normal[i] for i in range(3)]
        # ... and where the line through the pair leaves either round at its radius: at right angles to its centre line, to within
        # FLAT, or through a true end on the far side of the segment
        wv = [(-v[i]) / dist for i in range(3)]
        c1, c2 = dot(wv, d1), dot(wv, d2)
        tp = np.where(within, ONE if c else ZERO, t).astype(F)
        free_a = ((s == ZERO) & (c1 <= ZERO)) | ((s == ONE) & (c1 >= ZERO)) | (Ra * (c1 * c1) <= FLAT32 * a)
        free_b = ((tp == ZERO) & (c2 >= ZERO)) | ((tp == ONE) & (c2 <= ZERO)) | (Rb * (c2 * c2) <= FLAT32 * e)
        ok = seg & (pen >= ZERO) & (d2v > ZERO) & (total * dot(wn, wn) <= FLAT32) & free_a & free_b
        if c:
            ok &= s != s0
        else:
            s0 = s
        far, near = dist + Rb, dist - Rb
        hi, lo = np.where(far < Ra, far, Ra).astype(F), np.where(near < -Ra, -Ra, near).astype(F)
        mid = (lo + hi) * HALF
        keep.append(ok); pts.append([(pa[i] + ((-v[i]) / dist) * mid).astype(F) for i in range(3)]); pens.append(pen)
    return _two(keep, pts, pens)


def _box_box_axis(ma, mb):
    """contact rule 3's search once more, for what the record does not carry: (kind, i, j, sg, normal)"""
    (ca, Ta, na, sa, _), (cb, Tb, nb, sb, _) = ma, mb
    ua, Ha = R._frame(ca, na, sa)
    ub, Hb = R._frame(cb, nb, sb)
    w = [Tb[i] - Ta[i] for i in range(3)]
    t = [dot(w, ua[i]) for i in range(3)]
    Rm = [[dot(ua[i], ub[j]) for j in range(3)] for i in range(3)]
    Q = [[np.abs(Rm[i][j]) + SAT_EPS for j in range(3)] for i in range(3)]
    k = len(t[0])
    bo, bt = None, None
    bkind, bi, bj = np.full(k, K.BOX_FACE_A, np.uint32), np.zeros(k, np.int64), np.zeros(k, np.int64)
    for i in range(3):
        o = (Ha[i] + ((Hb[0] * Q[i][0] + Hb[1] * Q[i][1]) + Hb[2] * Q[i][2])) - np.abs(t[i])
        if i == 0:
            bo, bt = o, t[0]
        else:
            better = o < bo
            bo, bt, bi = np.where(better, o, bo).astype(F), np.where(better, t[i], bt).astype(F), np.where(better, i, bi)
    for j in range(3):
        ra = (Ha[0] * Q[0][j] + Ha[1] * Q[1][j]) + Ha[2] * Q[2][j]
        tl = (t[0] * Rm[0][j] + t[1] * Rm[1][j]) + t[2] * Rm[2][j]
        o = (ra + Hb[j]) - np.abs(tl)
        better = o < bo
        bo, bt = np.where(better, o, bo).astype(F), np.where(better, tl, bt).astype(F)
        bkind, bj = np.where(better, K.BOX_FACE_B, bkind).astype(np.uint32), np.where(better, j, bj)
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            ra = Ha[i1] * Q[i2][j] + Ha[i2] * Q[i1][j]
            rb = Hb[j1] * Q[i][j2] + Hb[j2] * Q[i][j1]
            tl = t[i2] * Rm[i1][j] - t[i1] * Rm[i2][j]
            l2 = ONE - Rm[i][j] * Rm[i][j]
            o = ((ra + rb) - np.abs(tl)) / np.sqrt(l2)
            better = ~(l2 < K.EDGE_EPS) & (o < bo)
            bo, bt = np.where(better, o, bo).astype(F), np.where(better, tl, bt).astype(F)
            bkind = np.where(better, K.BOX_EDGE, bkind).astype(np.uint32)
            bi, bj = np.where(better, i, bi), np.where(better, j, bj)
    return bkind, bi, bj, sign(bt), (ua, Ha, Ta), (ub, Hb, Tb)


def _face(ma, mb, normal):
    """FACE: (count, kind, points [4][3] as arrays [k], depths [4]); count 0 where the contact is an edge or nothing is kept"""
    bkind, bi, bj, sg, (ua, Ha, Ta), (ub, Hb, Tb) = _box_box_axis(ma, mb)
    k = len(sg)
    of_b = bkind == K.BOX_FACE_B
    is_face = bkind != K.BOX_EDGE
    uo = [[np.where(of_b, ub[a][c], ua[a][c]) for c in range(3)] for a in range(3)]
    ut = [[np.where(of_b, ua[a][c], ub[a][c]) for c in range(3)] for a in range(3)]
    Ho = [np.where(of_b, Hb[a], Ha[a]) for a in range(3)]
    Ht = [np.where(of_b, Ha[a], Hb[a]) for a in range(3)]
    To = [np.where(of_b, Tb[c], Ta[c]) for c in range(3)]
    Tt = [np.where(of_b, Ta[c], Tb[c]) for c in range(3)]
    ax = np.where(of_b, bj, bi)
    a1 = (ax + 1) % 3
    a2 = (a1 + 1) % 3
    sr = np.where(of_b, -sg, sg).astype(F)
    cm = dot(normal, ut[0])
    big, mi = np.abs(cm), np.zeros(k, np.int64)
    for a in (1, 2):
        ck = dot(normal, ut[a])
        better = np.abs(ck) > big
        big, cm, mi = np.where(better, np.abs(ck), big).astype(F), np.where(better, ck, cm).astype(F), np.where(better, a, mi)
    sm = np.where((cm < ZERO) != of_b, ONE, NEG).astype(F)
    m1 = (mi + 1) % 3
    Hp, Hq, Hr = pick(a1, Ho), pick(a2, Ho), pick(ax, Ho)
    poly = np.zeros((2, k, SLOTS, 3), F)
    for j in range(4):
        s1, s2 = (ONE if j in (0, 3) else NEG), (ONE if j < 2 else NEG)
        g = [np.where(mi == a, sm, np.where(m1 == a, s1, s2)).astype(F) * Ht[a] for a in range(3)]
        v = image(ut, Tt, g)
        r = [v[c] - To[c] for c in range(3)]
        x = [dot(r, uo[a]) for a in range(3)]
        poly[0, :, j, 0], poly[0, :, j, 1], poly[0, :, j, 2] = pick(a1, x), pick(a2, x), sr * pick(ax, x)
    n = np.full(k, 4, np.int64)
    rows = np.arange(k)
    for pl in range(4):
        comp, src, dst, upper = pl >> 1, pl & 1, (pl & 1) ^ 1, (pl & 1) == 0
        hside = Hq if comp else Hp
        hv = (hside if upper else -hside).astype(F)
        last = np.where(n > 0, n - 1, 0)
        pv = poly[src, rows, last].copy()
        cnt = np.zeros(k, np.int64)
        for i in range(SLOTS):
            live = i < n
            cur = poly[src, :, i].copy()
            xc, xp = cur[:, comp], pv[:, comp]
            in_c, in_p = ((xc <= hv), (xp <= hv)) if upper else ((xc >= hv), (xp >= hv))
            t = (hv - xp) / (xc - xp)
            cut = np.stack([pv[:, c] + (cur[:, c] - pv[:, c]) * t for c in range(3)], axis=1).astype(F)
            put = np.flatnonzero(live & (in_c != in_p) & (cnt < SLOTS))
            poly[dst, put, cnt[put]] = cut[put]
            cnt[put] += 1
            put = np.flatnonzero(live & in_c & (cnt < SLOTS))
            poly[dst, put, cnt[put]] = cur[put]
            cnt[put] += 1
            pv = np.where(live[:, None], cur, pv)
        n = cnt
    P = poly[0]
    pen_all = (Hr[:, None] - P[:, :, 2]).astype(F)
    # kept: at or below the reference face, not below the reference box, and the point within SKIN of the other box
    kept = (np.arange(SLOTS)[None, :] < n[:, None]) & (pen_all >= ZERO)
    for i in range(SLOTS):
        z = P[:, i, 2]
        zz = sr * (z + pen_all[:, i] * HALF)
        x = [np.where(a1 == a, P[:, i, 0], np.where(a2 == a, P[:, i, 1], zz)).astype(F) for a in range(3)]
        pt = image(uo, To, x)
        r = [pt[c] - Tt[c] for c in range(3)]
        inside = z >= -Hr
        for a in range(3):
            inside &= np.abs(dot(r, ut[a])) - Ht[a] <= SKIN32
        kept[:, i] &= inside
    count = kept.sum(axis=1)
    # up to four: polygon order
    sel = np.zeros((k, 4), np.int64)
    seen = np.zeros(k, np.int64)
    for i in range(SLOTS):
        put = np.flatnonzero(kept[:, i] & (seen < 4))
        sel[put, seen[put]] = i
        seen[kept[:, i]] += 1
    # more: the deepest, the farthest from it, the largest area on either side
    many = count > 4
    c0, first, best = sel[:, 0].copy(), np.ones(k, bool), np.zeros(k, F)
    for i in range(SLOTS):
        better = kept[:, i] & (first | (pen_all[:, i] > best))
        best, c0, first = np.where(better, pen_all[:, i], best).astype(F), np.where(better, i, c0), first & ~better
    pa, qa = P[rows, c0, 0], P[rows, c0, 1]
    c1, first = sel[:, 1].copy(), np.ones(k, bool)
    for i in range(SLOTS):
        dp, dq = P[:, i, 0] - pa, P[:, i, 1] - qa
        d2 = dp * dp + dq * dq
        better = kept[:, i] & (first | (d2 > best))
        best, c1, first = np.where(better, d2, best).astype(F), np.where(better, i, c1), first & ~better
    ex, ey = P[rows, c1, 0] - pa, P[rows, c1, 1] - qa
    most, least = np.zeros(k, F), np.zeros(k, F)
    left, right, cl, cr_ = np.zeros(k, bool), np.zeros(k, bool), np.zeros(k, np.int64), np.zeros(k, np.int64)
    for i in range(SLOTS):
        area = ex * (P[:, i, 1] - qa) - ey * (P[:, i, 0] - pa)
        assert area.dtype == F
        up, down = kept[:, i] & (area > most), kept[:, i] & (area < least)
        most, cl, left = np.where(up, area, most).astype(F), np.where(up, i, cl), left | up
        least, cr_, right = np.where(down, area, least).astype(F), np.where(down, i, cr_), right | down
    reduced = np.stack([c0, c1, np.where(left, cl, cr_), cr_], axis=1)
    sel = np.where(many[:, None], reduced, sel)
    count = np.where(many, 2 + left.astype(np.int64) + right, count)
    count = np.where(is_face, count, 0)
    kind = np.where(many, FACE | REDUCED, FACE).astype(np.uint32)
    points, depths = [], []
    for s in range(4):
        i = sel[:, s]
        p, q, z = P[rows, i, 0], P[rows, i, 1], P[rows, i, 2]
        pen = Hr - z
        zz = sr * (z + pen * HALF)
        x = [np.where(a1 == a, p, np.where(a2 == a, q, zz)).astype(F) for a in range(3)]
        pt = image(uo, To, x)
        live = s < count
        points.append([np.where(live, pt[c], ZERO).astype(F) for c in range(3)])
        depths.append(np.where(live, pen, ZERO).astype(F))
    return count, kind, points, depths


def manifolds32(matrices, col, pairs, n=None, rank=0):
    """one record per pair of `pairs` [k][2] (ids, a < b as listed): the structured array the device must write"""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    m = np.ascontiguousarray(matrices, F).reshape(-1, 16)
    n = len(m) if n is None else n
    m = m[:n]
    out = np.zeros(len(pairs), DTYPE)
    if not len(pairs) or col is None:
        return out
    contact = K.contacts32(m, col, pairs, n=n, rank=rank)
    idx = np.flatnonzero((contact["kind"] & 0xFF) != K.NONE)
    if not len(idx):
        return out
    typ, shp = shape_records(col, n)
    e = (pairs[idx] & 0xFFFFFF).astype(np.int64)
    ea, eb = e[:, 0], e[:, 1]
    ck = contact["kind"][idx]
    with np.errstate(all="ignore"):
        ma = R._members(m, shp, ea) + (typ[ea],)
        mb = R._members(m, shp, eb) + (typ[eb],)
        boxa, boxb = typ[ea] == cr.BOX, typ[eb] == cr.BOX
        normal = [contact["normal"][idx, c] for c in range(3)]
        f_count, f_kind, f_pts, f_dep = _face(ma, mb, normal)
        a_count, a_pts, a_dep = _round_box_segment(mb, ma)                     # a is the box
        b_count, b_pts, b_dep = _round_box_segment(ma, mb)                     # b is the box
        r_count, r_pts, r_dep = _round_round_segment(ma, mb, normal)
    r_count = np.where((ck & K.DEGENERATE) != 0, 0, r_count)
    bb, ra, rb = boxa & boxb, boxa & ~boxb, boxb & ~boxa
    rr = ~boxa & ~boxb
    count = np.where(bb, f_count, np.where(ra, a_count, np.where(rb, b_count, r_count)))
    kind = np.where(bb, f_kind, SEGMENT).astype(np.uint32)
    single = count == 0
    rec = np.zeros(len(idx), DTYPE)
    for s in range(4):
        for c in range(3):
            seg = np.where(ra, a_pts[s][c], np.where(rb, b_pts[s][c], r_pts[s][c])) if s < 2 else np.zeros(len(idx), F)
            value = np.where(bb, f_pts[s][c], seg)
            rec["point"][:, s, c] = np.where(single, contact["point"][idx, c] if s == 0 else ZERO, value)
        seg = np.where(ra, a_dep[s], np.where(rb, b_dep[s], r_dep[s])) if s < 2 else np.zeros(len(idx), F)
        value = np.where(bb, f_dep[s], seg)
        rec["depth"][:, s] = np.where(single, contact["depth"][idx] if s == 0 else ZERO, value)
    rec["count"] = np.where(single, 1, count)
    rec["kind"] = np.where(single, SINGLE, kind)
    assert rr.dtype == bool
    out[idx] = rec
    return out


def report(rec):
    """ScTickPairManifoldInfo of the written records, as a dict"""
    count, kind = rec["count"], rec["kind"]
    return dict(written=len(rec), points=int(count.sum()), with_one=int((count == 1).sum()), with_two=int((count == 2).sum()),
                with_three=int((count == 3).sum()), with_four=int((count == 4).sum()), face=int(((kind & 0xFF) == FACE).sum()),
                reduced=int(((kind & REDUCED) != 0).sum()))


def bits(rec):
    """the records as raw words [k][20], for bit-for-bit comparison"""
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 20)


# ---- float64, by another route -------------------------------------------------------------------------------------------------------
TOL = 1e-3                                                     # metres: what "clearly" means to the float64 witness


SKIN = 0.5 * TOL                                              # a point of a manifold may lie ON a surface, or a hair outside it


def reach64(shape, p, d, far=16.0, iters=60):
    """how far one can go from the points p [k][3] along the unit d [k][3] and stay within SKIN of the (convex) shape: bisection on the
    exact distance; 0 where p itself is further out"""
    lo, hi = np.zeros(len(p)), np.full(len(p), far)
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        inside = shape.distance(p + d * mid[:, None]) <= SKIN
        lo, hi = np.where(inside, mid, lo), np.where(inside, hi, mid)
    return lo


def overlap_at64(sa, sb, p, n):
    """the overlap of the two shapes on the line through p along n (from a to b): from p forward to a's surface plus back to b's.  A
    clipped vertex lies on a side plane of the reference box and a midpoint above a leaning edge a hair outside the other box, so both
    shapes are taken SKIN thicker and the two skins the line leaves through are taken off again (exact where it leaves at right angles)"""
    return reach64(sa, p, n) + reach64(sb, p, -n) - 2.0 * SKIN


def _polygon_area(pq):
    """area of the convex hull of a few points of the plane (ordered by angle about their mean)"""
    pq = np.asarray(pq, np.float64)
    if len(pq) < 3:
        return 0.0
    c = pq.mean(axis=0)
    o = pq[np.argsort(np.arctan2(pq[:, 1] - c[1], pq[:, 0] - c[0]))]
    return 0.5 * abs(float(np.sum(o[:, 0] * np.roll(o[:, 1], -1) - np.roll(o[:, 0], -1) * o[:, 1])))


class Expect64:
    """what the float64 witness expects of one pair: kind (SINGLE / SEGMENT / FACE), the points and depths of every kept vertex or end,
    whether the pair is robust (nothing within TOL of a decision), and for FACE the kept polygon's area and the reference frame"""
    def __init__(self, kind, points, depths, robust, area=0.0, frame=None):
        self.kind, self.points, self.depths, self.robust, self.area, self.frame = kind, np.asarray(points, np.float64).reshape(-1, 3), np.asarray(depths, np.float64), robust, area, frame


def _box_axes64(sa, sb, i):
    """least-overlap search of pair i over the fifteen axes in float64: [(overlap, unit axis from a to b, owner 0 / 1 / 2 = edge, index)]"""
    ua, ub, Ha, Hb, w = sa.u[i], sb.u[i], sa.H[i], sb.H[i], sb.T[i] - sa.T[i]
    cands = [(ua[k], 0, k) for k in range(3)] + [(ub[k], 1, k) for k in range(3)]
    for a in range(3):
        for b in range(3):
            L = np.cross(ua[a], ub[b])
            ln = np.linalg.norm(L)
            if ln > 0.02:
                cands.append((L / ln, 2, 3 * a + b))
    out = []
    for L, owner, k in cands:
        tl = float(w @ L)
        o = float(Ha @ np.abs(ua @ L) + Hb @ np.abs(ub @ L)) - abs(tl)
        out.append((o, L if tl >= 0 else -L, owner, k))
    return out


def face64(sa, sb, i):
    """the box-box pair i: the incident face cut by the reference prism as an intersection of half planes"""
    axes = _box_axes64(sa, sb, i)
    o, n, owner, ax = min(axes[:6], key=lambda a: a[0])       # the best face axis (an axis within 1e-6 rad of it is the same axis)
    others = [a for a in axes if np.linalg.norm(np.cross(a[1], n)) > 1e-6]
    robust = all(abs(a[0] - o) > TOL for a in others)
    if any(a[0] < o for a in others if a[2] == 2):            # an edge axis overlaps less
        return Expect64(SINGLE, [], [], robust)
    if any(a[0] < o for a in others):
        return Expect64(FACE, [], [], False)
    so, st = (sa, sb) if owner == 0 else (sb, sa)
    To, uo, Ho, Tt, ut, Ht = so.T[i], so.u[i], so.H[i], st.T[i], st.u[i], st.H[i]
    d = n if owner == 0 else -n                               # the reference face's outward normal
    sr = 1.0 if float(d @ uo[ax]) >= 0 else -1.0
    c = ut @ d
    m = int(np.argmax(np.abs(c)))
    robust &= all(abs(c[m]) - abs(c[k]) > TOL for k in range(3) if k != m)
    centre = Tt - np.sign(c[m]) * Ht[m] * ut[m]
    e1, e2 = Ht[(m + 1) % 3] * ut[(m + 1) % 3], Ht[(m + 2) % 3] * ut[(m + 2) % 3]
    a1, a2 = (ax + 1) % 3, (ax + 2) % 3
    quad = np.array([centre + s1 * e1 + s2 * e2 for s1, s2 in ((1, 1), (-1, 1), (-1, -1), (1, -1))]) - To
    P = np.stack([quad @ uo[a1], quad @ uo[a2], sr * (quad @ uo[ax])], axis=1)
    # z over the face's plane as an affine function of (p, q)
    A = np.column_stack([P[:, 0], P[:, 1], np.ones(4)])
    if abs(np.linalg.det(A[:3])) < 1e-6:
        return Expect64(FACE, [], [], False)
    coef = np.linalg.solve(A[:3], P[:3, 2])
    lines = [(1.0, 0.0, Ho[a1]), (-1.0, 0.0, Ho[a1]), (0.0, 1.0, Ho[a2]), (0.0, -1.0, Ho[a2])]      # a p + b q <= c
    mid = P[:, :2].mean(axis=0)
    for j in range(4):
        p0, p1 = P[j, :2], P[(j + 1) % 4, :2]
        nrm = np.array([p1[1] - p0[1], p0[0] - p1[0]])
        nrm /= np.linalg.norm(nrm)
        if nrm @ (mid - p0) > 0:
            nrm = -nrm
        lines.append((nrm[0], nrm[1], float(nrm @ p0)))
    verts = []
    for j in range(8):
        for k in range(j + 1, 8):
            (aj, bj, cj), (ak, bk, ck) = lines[j], lines[k]
            det = aj * bk - ak * bj
            if abs(det) < 1e-9:
                continue
            x = np.array([(cj * bk - ck * bj) / det, (aj * ck - ak * cj) / det])
            margin = min(c_ - a_ * x[0] - b_ * x[1] for l_, (a_, b_, c_) in enumerate(lines) if l_ not in (j, k))
            if abs(margin) <= TOL:
                robust = False
            if margin >= -1e-9 and not any(np.abs(x - v).max() < 1e-9 for v in verts):
                verts.append(x)
    points, depths, kept = [], [], []
    for x in verts:
        z = float(coef @ [x[0], x[1], 1.0])
        pen = Ho[ax] - z
        if abs(pen) <= TOL:
            robust = False
        point = To + x[0] * uo[a1] + x[1] * uo[a2] + sr * (z + 0.5 * pen) * uo[ax]
        out = np.abs(ut @ (point - Tt)) - Ht                   # how far the point lies outside the other box, per axis
        if (np.abs(out - float(SKIN32)) <= 0.2 * float(SKIN32)).any() or abs(z + Ho[ax]) <= TOL:
            robust = False
        if pen >= 0 and z >= -Ho[ax] and (out <= float(SKIN32)).all():
            kept.append(x)
            points.append(point)
            depths.append(pen)
    return Expect64(FACE if kept else SINGLE, points, depths, robust, _polygon_area(kept), (To, uo[a1], uo[a2]))


def capsule_face64(sc, sx, i):
    """the pair i of a capsule (sc) and a box (sx): the stretch of the centre line over the face, by exact slab geometry"""
    u, H, R_ = sx.u[i], sx.H[i], sc.R[i]
    y0, dy = u @ (sc.T[i] - sc.A[i] - sx.T[i]), u @ (2.0 * sc.A[i])
    f = lambda t: float(np.linalg.norm(np.maximum(np.abs(y0 + dy * t) - H, 0.0)))      # noqa: E731
    lo, hi = 0.0, 1.0
    for _ in range(80):                                        # the convex distance's minimum by ternary search
        m1, m2 = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        lo, hi = (lo, m2) if f(m1) <= f(m2) else (m1, hi)
    y = y0 + dy * (0.5 * (lo + hi))
    out = np.abs(y) - H
    robust = bool((np.abs(out) > TOL).all())
    if (out > 0).sum() > 1:
        return Expect64(SINGLE, [], [], robust)
    if (out > 0).sum() == 1:
        kf = int(np.argmax(out))
    else:
        order = np.argsort(-out)                               # inside: the nearest face
        kf = int(order[0])
        robust &= bool(out[order[0]] - out[order[1]] > TOL)
    sg = 1.0 if y[kf] >= 0 else -1.0
    lo, hi = 0.0, 1.0
    for k in range(3):
        if k == kf:
            continue
        robust &= all(abs(abs(e) - H[k]) > TOL for e in (y0[k], y0[k] + dy[k]))
        if abs(dy[k]) < 1e-12:
            if abs(y0[k]) > H[k]:
                return Expect64(SINGLE, [], [], robust)
            continue
        b = sorted(((H[k] - y0[k]) / dy[k], (-H[k] - y0[k]) / dy[k]))
        lo, hi = max(lo, b[0]), min(hi, b[1])
    if not lo < hi:
        return Expect64(SINGLE, [], [], False)
    points, depths = [], []
    lean = R_ * dy[kf] ** 2 / float(dy @ dy)                  # R cos^2 of the angle between the centre line and the face's normal
    flat = lean <= float(FLAT32)
    for t, end in ((lo, 0.0), (hi, 1.0)):
        yt = y0 + dy * t
        up = sg * yt[kf]
        pen = R_ - (up - H[kf])
        if abs(pen) <= TOL:
            robust = False
        outward = t == end and (sg * dy[kf] >= 0 if end == 0.0 else sg * dy[kf] <= 0)      # a true end, the normal leaves it on the far side
        if not outward and abs(lean - float(FLAT32)) <= 0.1 * float(FLAT32):
            robust = False
        share = min(up + R_, H[kf]) - max(up - R_, -H[kf])    # what the round and the box share on the line along the axis
        if abs(share) <= TOL:
            robust = False
        if pen >= 0 and (flat or outward) and share >= 0:
            mid = 0.5 * (max(up - R_, -H[kf]) + min(up + R_, H[kf]))      # the middle of what the round and the box share along the axis
            x = yt.copy()
            x[kf] = sg * mid
            points.append(sx.T[i] + x @ u)
            depths.append(pen)
    return Expect64(SEGMENT if points else SINGLE, points, depths, robust)


def capsule_capsule64(sa, sb, i, normal):
    """the pair i of two capsules: each end of b's segment against a's segment, or a's nearer end against b's segment"""
    p1, d1, p2, d2, Ra, Rb = sa.T[i] - sa.A[i], 2.0 * sa.A[i], sb.T[i] - sb.A[i], 2.0 * sb.A[i], sa.R[i], sb.R[i]
    robust, points, depths, params = True, [], [], []
    for g in (p2, p2 + d2):
        s = float((g - p1) @ d1 / (d1 @ d1))
        margin = TOL / np.linalg.norm(d1)
        if abs(s) <= margin or abs(s - 1.0) <= margin:
            robust = False
        if 0.0 <= s <= 1.0:
            pa, pb = p1 + d1 * s, g
        else:
            s = min(max(s, 0.0), 1.0)
            pa = p1 + d1 * s
            t = min(max(float((pa - p2) @ d2 / (d2 @ d2)), 0.0), 1.0)
            pb = p2 + d2 * t
        if any(abs(s - s_) <= margin for s_ in params):
            robust &= any(s == s_ for s_ in params)            # (both clamped to the same end: one candidate, robustly)
            if any(s == s_ for s_ in params):
                continue
        params.append(s)
        dist = float(np.linalg.norm(pb - pa))
        pen = Ra + Rb - dist
        if abs(pen) <= TOL or dist <= TOL:
            robust = False
        turn = (Ra + Rb) * float(np.sum(((pb - pa) / dist - normal) ** 2)) if dist > 0 else np.inf      # the candidate's direction against the contact's
        if abs(turn - float(FLAT32)) <= 0.1 * float(FLAT32):
            robust = False
        free = True
        if dist > 0:                                           # either round must end at its radius on the line through the pair
            for (q0, dq, rad, at, sign_) in ((p1, d1, Ra, pa, 1.0), (p2, d2, Rb, pb, -1.0)):
                u_ = float(((at - q0) @ dq) / (dq @ dq))       # where on its centre line the point sits
                cos_ = sign_ * float((pb - pa) @ dq) / (dist * np.linalg.norm(dq))
                lean_ = rad * cos_ ** 2
                beyond = (u_ <= 1e-9 and cos_ <= 0) or (u_ >= 1 - 1e-9 and cos_ >= 0)
                if not beyond and abs(lean_ - float(FLAT32)) <= 0.1 * float(FLAT32):
                    robust = False
                free &= beyond or lean_ <= float(FLAT32)
        if pen >= 0 and dist > 0 and turn <= float(FLAT32) and free:
            mid = 0.5 * (max(-Ra, dist - Rb) + min(Ra, dist + Rb))
            points.append(pa + (pb - pa) / dist * mid)
            depths.append(pen)
    return Expect64(SEGMENT if points else SINGLE, points, depths, robust)


def expect64(sa, sb, i, normal):
    """the float64 witness's answer for pair i of two Shapes64 (None: a pair with a sphere in it -- SINGLE by definition); normal: the
    contact's, from a to b, unit"""
    seg_a, seg_b = bool(np.any(sa.A[i] != 0)), bool(np.any(sb.A[i] != 0))
    if sa.box[i] and sb.box[i]:
        return face64(sa, sb, i)
    if sa.box[i] or sb.box[i]:
        sc, sx = (sb, sa) if sa.box[i] else (sa, sb)
        return capsule_face64(sc, sx, i) if (seg_b if sa.box[i] else seg_a) else None
    return capsule_capsule64(sa, sb, i, normal) if seg_a and seg_b else None
