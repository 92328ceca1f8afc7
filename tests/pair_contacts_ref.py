"""Witnesses of the pair contacts (include/sc_tick.h "pair contacts"), independent of the kernel.

    contacts32   numpy fp32 written from the header text, operation by operation, over the listed pairs of a touching list (ids as
                 scTickReadPairShapes gives them): a structured array (point, depth, normal, kind) the device must reproduce bit for bit;
                 report() turns the kinds into ScTickPairContactInfo.
    float64, by another route: support functions.  A box is its eight vertices, a round its segment's two ends plus the radius;
                 overlap64(d) = max_{x in a} x.d - min_{y in b} y.d for a unit d -- how far b must move along d to clear a.  Point-shape
                 distances are exact (point-segment, point-box).  For matrices with orthogonal columns."""
import numpy as np

from tests import collider_ref as cr
from tests import pair_shapes_ref as R
from tests.pair_shapes_ref import F, ZERO, ONE, HALF, SAT_EPS, NETWORK, clamp01, dot
from tests.shape_rays_ref import shape_records

EDGE_EPS = F(1e-4)                                             # SC_TICK_PAIR_CONTACTS_EDGE_EPS
NONE, ROUND_ROUND, ROUND_BOX, BOX_FACE_A, BOX_FACE_B, BOX_EDGE = 0, 1, 2, 3, 4, 5
DEEP, DEGENERATE = 1 << 8, 1 << 9
DTYPE = np.dtype([("point", F, 3), ("depth", F), ("normal", F, 3), ("kind", np.uint32)])
INFO_FIELDS = ("written", "round_round", "round_box", "box_box", "unrefined", "deep", "degenerate", "reserved")
NEG = F(-1.0)


def sign(x):
    return np.where(x < ZERO, NEG, ONE).astype(F)


def clamp(x, h):
    c = np.where(x < -h, -h, x)
    return np.where(c > h, h, c).astype(F)


def image(u, T, x):
    """T + (x_0 u_0 + x_1 u_1) + x_2 u_2 per component"""
    return [T[c] + ((x[0] * u[0][c] + x[1] * u[1][c]) + x[2] * u[2][c]) for c in range(3)]


def pick(i, a):
    """a[i] for index arrays i over a list of three arrays"""
    return np.where(i == 0, a[0], np.where(i == 1, a[1], a[2])).astype(F)


def seg_seg(p1, d1, p2, d2):
    """routine 1's closed form: s, t, v"""
    r = [p1[i] - p2[i] for i in range(3)]
    a, e, f = dot(d1, d1), dot(d2, d2), dot(d2, r)
    c, b = dot(d1, r), dot(d1, d2)
    den = a * e - b * b
    s_0 = np.zeros_like(a)
    t_0 = np.where(e > ZERO, clamp01(f / e), ZERO)
    s_1 = clamp01((-c) / a)
    t_1 = np.zeros_like(a)
    s_2 = np.where(den > ZERO, clamp01((b * f - c * e) / den), ZERO).astype(F)
    t_2 = (b * s_2 + f) / e
    below, above = t_2 < ZERO, ~(t_2 < ZERO) & (t_2 > ONE)
    s_2 = np.where(below, clamp01((-c) / a), np.where(above, clamp01((b - c) / a), s_2))
    t_2 = np.where(below, ZERO, np.where(above, ONE, t_2))
    hasA, hasE = a > ZERO, e > ZERO
    s = np.where(~hasA, s_0, np.where(~hasE, s_1, s_2)).astype(F)
    t = np.where(~hasA, t_0, np.where(~hasE, t_1, t_2)).astype(F)
    v = [(p1[i] + d1[i] * s) - (p2[i] + d2[i] * t) for i in range(3)]
    return s, t, v


def seg_box(y0, dy, H, point):
    """routine 2's fmin and the parameter it was found at"""
    f0 = R._box_dist2(y0, dy, H, ZERO)
    fmin, at = f0, np.zeros_like(f0)

    def least(fmin, at, x, t):
        better = x < fmin
        return np.where(better, x, fmin).astype(F), np.where(better, t, at).astype(F)

    one = np.ones_like(f0)
    fmin, at = least(fmin, at, R._box_dist2(y0, dy, H, ONE), one)
    b = [np.zeros_like(f0)] + [None] * 6 + [one]
    for k in range(3):
        b[1 + 2 * k] = clamp01((H[k] - y0[k]) / dy[k])
        b[2 + 2 * k] = clamp01(((-H[k]) - y0[k]) / dy[k])
    for i, j in NETWORK:
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
        fmin, at = least(fmin, at, R._box_dist2(y0, dy, H, ts), ts)
        if i < 6:
            fmin, at = least(fmin, at, R._box_dist2(y0, dy, H, hi), hi)
    return np.where(point, f0, fmin).astype(F), np.where(point, ZERO, at).astype(F)


def _round_round(ma, mb):
    (ca, Ta, na, sa, ta), (cb, Tb, nb, sb, tb) = ma, mb
    Aa, Ra = R._round(ca, na, sa, ta)
    Ab, Rb = R._round(cb, nb, sb, tb)
    p1 = [Ta[i] - Aa[i] for i in range(3)]; d1 = [Aa[i] + Aa[i] for i in range(3)]
    p2 = [Tb[i] - Ab[i] for i in range(3)]; d2 = [Ab[i] + Ab[i] for i in range(3)]
    s, t, v = seg_seg(p1, d1, p2, d2)
    d2v = dot(v, v)
    total = Ra + Rb
    ok = d2v > ZERO
    dist = np.sqrt(d2v)
    depth = np.where(ok, total - dist, total).astype(F)
    far, near = dist + Rb, dist - Rb
    hi, lo = np.where(far < Ra, far, Ra).astype(F), np.where(near < -Ra, -Ra, near).astype(F)
    mid = (lo + hi) * HALF
    point, normal = [], []
    for i in range(3):
        pa = p1[i] + d1[i] * s
        n = (-v[i]) / dist
        normal.append(np.where(ok, n, ONE if i == 1 else ZERO).astype(F))
        point.append(np.where(ok, pa + n * mid, pa).astype(F))
    kind = np.where(ok, ROUND_ROUND, ROUND_ROUND | DEGENERATE).astype(np.uint32)
    return point, depth, normal, kind


def _round_box(mr, mx, round_is_a):
    (cr_, Tr, nr, sr_, tr), (cx, Tx, nx, sx, _) = mr, mx
    A, Rr = R._round(cr_, nr, sr_, tr)
    u, H = R._frame(cx, nx, sx)
    w = [Tr[i] - Tx[i] for i in range(3)]
    y0, dy = [], []
    for k in range(3):
        yc, ya = dot(u[k], w), dot(u[k], A)
        y0.append(yc - ya); dy.append(ya + ya)
    is_point = (A[0] == ZERO) & (A[1] == ZERO) & (A[2] == ZERO)
    fmin, at = seg_box(y0, dy, H, is_point)
    y = [y0[k] + dy[k] * at for k in range(3)]
    q = [clamp(y[k], H[k]) for k in range(3)]
    m = [H[k] - np.abs(y[k]) for k in range(3)]
    shallow = fmin > ZERO
    dist = np.sqrt(fmin)
    kd, least = np.zeros(len(fmin), np.int64), m[0]
    for k in (1, 2):
        better = m[k] < least
        least, kd = np.where(better, m[k], least).astype(F), np.where(better, k, kd)
    sg = sign(pick(kd, y))
    yk0, dyk, hk = pick(kd, y0), pick(kd, dy), pick(kd, H)
    e0, e1 = sg * yk0, sg * (yk0 + dyk)
    low = np.where(e1 < e0, e1, e0).astype(F)
    e = [(y[k] - q[k]) / dist for k in range(3)]
    nb = [np.where(shallow, e[k], np.where(kd == k, sg, ZERO)).astype(F) for k in range(3)]
    ell = [(H[k] + H[k]) / np.abs(e[k]) for k in range(3)]
    depth = np.where(shallow, Rr - dist, Rr + (hk - low)).astype(F)
    l = ell[0]
    for k in (1, 2):
        l = np.where(ell[k] < l, ell[k], l).astype(F)
    far, back = dist + l, least - (hk + hk)
    hi_s = np.where(far < Rr, far, Rr).astype(F)
    lo_d, hi_d = np.where(back < -Rr, -Rr, back).astype(F), np.where(least < Rr, least, Rr).astype(F)
    mid = np.where(shallow, -((dist + hi_s) * HALF), (lo_d + hi_d) * HALF).astype(F)
    on_line = image(u, Tx, y)
    point, normal = [], []
    for i in range(3):
        n_box = (nb[0] * u[0][i] + nb[1] * u[1][i]) + nb[2] * u[2][i]
        point.append((on_line[i] + n_box * mid).astype(F))
        normal.append(np.where(round_is_a, -n_box, n_box).astype(F))
    kind = np.where(shallow, ROUND_BOX, ROUND_BOX | DEEP).astype(np.uint32)
    return point, depth, normal, kind


def _box_box(ma, mb):
    (ca, Ta, na, sa, _), (cb, Tb, nb, sb, _) = ma, mb
    ua, Ha = R._frame(ca, na, sa)
    ub, Hb = R._frame(cb, nb, sb)
    w = [Tb[i] - Ta[i] for i in range(3)]
    t = [dot(w, ua[i]) for i in range(3)]
    Rm = [[dot(ua[i], ub[j]) for j in range(3)] for i in range(3)]
    Q = [[np.abs(Rm[i][j]) + SAT_EPS for j in range(3)] for i in range(3)]
    k = len(t[0])
    bo = bt = None
    bL = None
    bkind = np.full(k, BOX_FACE_A, np.uint32)
    bi, bj = np.zeros(k, np.int64), np.zeros(k, np.int64)

    def take(better, o, tl, L, kind, i, j):
        nonlocal bo, bt, bL, bkind, bi, bj
        bo, bt = np.where(better, o, bo).astype(F), np.where(better, tl, bt).astype(F)
        bL = [np.where(better, L[c], bL[c]).astype(F) for c in range(3)]
        bkind = np.where(better, kind, bkind).astype(np.uint32)
        if i is not None:
            bi = np.where(better, i, bi)
        if j is not None:
            bj = np.where(better, j, bj)

    for i in range(3):
        rb = (Hb[0] * Q[i][0] + Hb[1] * Q[i][1]) + Hb[2] * Q[i][2]
        o = (Ha[i] + rb) - np.abs(t[i])
        if i == 0:
            bo, bt, bL = o, t[0], [ua[0][c] for c in range(3)]
        else:
            take(o < bo, o, t[i], ua[i], BOX_FACE_A, i, None)
    for j in range(3):
        ra = (Ha[0] * Q[0][j] + Ha[1] * Q[1][j]) + Ha[2] * Q[2][j]
        tl = (t[0] * Rm[0][j] + t[1] * Rm[1][j]) + t[2] * Rm[2][j]
        o = (ra + Hb[j]) - np.abs(tl)
        take(o < bo, o, tl, ub[j], BOX_FACE_B, None, j)
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            ra = Ha[i1] * Q[i2][j] + Ha[i2] * Q[i1][j]
            rb = Hb[j1] * Q[i][j2] + Hb[j2] * Q[i][j1]
            tl = t[i2] * Rm[i1][j] - t[i1] * Rm[i2][j]
            l2 = ONE - Rm[i][j] * Rm[i][j]
            o = ((ra + rb) - np.abs(tl)) / np.sqrt(l2)
            L = [Rm[i1][j] * ua[i2][c] - Rm[i2][j] * ua[i1][c] for c in range(3)]
            assert o.dtype == F and L[0].dtype == F
            take(~(l2 < EDGE_EPS) & (o < bo), o, tl, L, BOX_EDGE, i, j)
    depth = np.where(bo < ZERO, ZERO, bo).astype(F)
    sg = sign(bt)
    ln = np.sqrt(dot(bL, bL))
    edge = bkind == BOX_EDGE
    n = [np.where(edge, sg * (bL[c] / ln), sg * bL[c]).astype(F) for c in range(3)]
    half = depth * HALF
    # a face
    of_b = bkind == BOX_FACE_B
    uo = [[np.where(of_b, ub[k_][c], ua[k_][c]) for c in range(3)] for k_ in range(3)]
    ut = [[np.where(of_b, ua[k_][c], ub[k_][c]) for c in range(3)] for k_ in range(3)]
    Ho = [np.where(of_b, Hb[k_], Ha[k_]) for k_ in range(3)]
    Ht = [np.where(of_b, Ha[k_], Hb[k_]) for k_ in range(3)]
    To = [np.where(of_b, Tb[c], Ta[c]) for c in range(3)]
    Tt = [np.where(of_b, Ta[c], Tb[c]) for c in range(3)]
    ax = np.where(of_b, bj, bi)
    g = []
    for k_ in range(3):
        neg = dot(n, ut[k_]) < ZERO
        g.append(np.where(neg != of_b, NEG, ONE).astype(F) * Ht[k_])
    p = [Tt[c] - ((g[0] * ut[0][c] + g[1] * ut[1][c]) + g[2] * ut[2][c]) for c in range(3)]
    r = [p[c] - To[c] for c in range(3)]
    x = []
    for k_ in range(3):
        xk = dot(r, uo[k_])
        x.append(np.where(ax == k_, xk, clamp(xk, Ho[k_])).astype(F))
    pc = image(uo, To, x)
    face_point = [np.where(of_b, pc[c] - n[c] * half, pc[c] + n[c] * half).astype(F) for c in range(3)]
    # an edge of each
    ga = [np.where(bi == k_, ZERO, sign(dot(n, ua[k_])) * Ha[k_]).astype(F) for k_ in range(3)]
    gb = [np.where(bj == k_, ZERO, (-sign(dot(n, ub[k_]))) * Hb[k_]).astype(F) for k_ in range(3)]
    ea, eb = image(ua, Ta, ga), image(ub, Tb, gb)
    ha, hb = pick(bi, Ha), pick(bj, Hb)
    p1, d1, p2, d2 = [], [], [], []
    for c in range(3):
        va, vb = pick(bi, [ua[0][c], ua[1][c], ua[2][c]]) * ha, pick(bj, [ub[0][c], ub[1][c], ub[2][c]]) * hb
        p1.append(ea[c] - va); d1.append(va + va)
        p2.append(eb[c] - vb); d2.append(vb + vb)
    s, t_, _ = seg_seg(p1, d1, p2, d2)
    edge_point = [((p1[c] + d1[c] * s) + (p2[c] + d2[c] * t_)) * HALF for c in range(3)]
    point = [np.where(edge, edge_point[c], face_point[c]).astype(F) for c in range(3)]
    return point, depth, n, bkind


def contacts32(matrices, col, pairs, n=None, rank=0):
    """one record per pair of `pairs` [k][2] (ids, a < b as listed): the structured array the device must write"""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    m = np.ascontiguousarray(matrices, F).reshape(-1, 16)
    n = len(m) if n is None else n
    m = m[:n]
    out = np.zeros(len(pairs), DTYPE)
    if not len(pairs) or col is None:
        return out
    typ, shp = shape_records(col, n)
    e = (pairs & 0xFFFFFF).astype(np.int64)
    e_ok = ((pairs >> 24) == rank) & (e < n)
    ok = np.stack([R.refinable(m, typ, e_ok[:, s], e[:, s]) for s in range(2)], axis=1)
    idx = np.flatnonzero(ok[:, 0] & ok[:, 1])
    if not len(idx):
        return out
    ea, eb = e[idx, 0], e[idx, 1]
    with np.errstate(all="ignore"):
        ma = R._members(m, shp, ea) + (typ[ea],)
        mb = R._members(m, shp, eb) + (typ[eb],)
        boxa, boxb = typ[ea] == cr.BOX, typ[eb] == cr.BOX
        bb, rr = _box_box(ma, mb), _round_round(ma, mb)
        ra, rb = _round_box(mb, ma, False), _round_box(ma, mb, True)       # (a is the box; b is the box)

        def choose(f):
            return np.where(boxa & boxb, f(bb), np.where(boxa, f(ra), np.where(boxb, f(rb), f(rr))))

        for c in range(3):
            out["point"][idx, c] = choose(lambda r_: r_[0][c])
            out["normal"][idx, c] = choose(lambda r_: r_[2][c])
        out["depth"][idx] = choose(lambda r_: r_[1])
        out["kind"][idx] = choose(lambda r_: r_[3])
    return out


def report(rec):
    """ScTickPairContactInfo of the written records, as a dict"""
    shape, kind = rec["kind"] & 0xFF, rec["kind"]
    return dict(written=len(rec), round_round=int((shape == ROUND_ROUND).sum()), round_box=int((shape == ROUND_BOX).sum()),
                box_box=int((shape >= BOX_FACE_A).sum()), unrefined=int((shape == NONE).sum()), deep=int(((kind & DEEP) != 0).sum()),
                degenerate=int(((kind & DEGENERATE) != 0).sum()), reserved=0)


def bits(rec):
    """the records as raw words [k][8], for bit-for-bit comparison"""
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 8)


# ---- float64, by another route: support functions and exact point-shape distances --------------------------------------------------
class Shapes64:
    """the shapes of entities e in float64: a box's centre, unit axes and half lengths; a round's two ends and radius"""

    def __init__(self, matrices, col, e):
        m = np.ascontiguousarray(matrices, F).reshape(-1, 16)
        typ, shp = shape_records(col, len(m))
        e = np.asarray(e, np.int64)
        c, self.T, nk, s = R._members64(m, shp, e)
        self.box = typ[e] == cr.BOX
        self.u = np.stack([c[k] / np.sqrt(nk[k])[:, None] for k in range(3)], axis=1)          # [e][axis][xyz]
        self.H = np.stack([s[:, k] * np.sqrt(nk[k]) for k in range(3)], axis=1)
        A, self.R = R._round64(c, nk, s, typ[e])
        self.A = np.where((typ[e] == cr.CAPSULE)[:, None], A, 0.0)

    def extent(self, d):
        """(max, min) of x.d over the shape, d [e][3] unit"""
        centre = np.einsum("ij,ij->i", self.T, d)
        rb = np.einsum("ek,ek->e", self.H, np.abs(np.einsum("ekc,ec->ek", self.u, d)))
        rr = np.abs(np.einsum("ij,ij->i", self.A, d)) + self.R
        r = np.where(self.box, rb, rr)
        return centre + r, centre - r

    def distance(self, p):
        """exact distance of points p [e][3] from the shape's surface-bounded solid (0 inside)"""
        y = np.einsum("ekc,ec->ek", self.u, p - self.T)
        db = np.linalg.norm(np.maximum(np.abs(y) - self.H, 0.0), axis=1)
        dr = np.maximum(R._point_segment(p, self.T - self.A, 2.0 * self.A) - self.R, 0.0)
        return np.where(self.box, db, dr)


def overlap64(sa, sb, d):
    """how far b must move along the unit d to clear a: max_a x.d - min_b y.d"""
    return sa.extent(d)[0] - sb.extent(d)[1]


def axes15(sa, sb):
    """the fifteen box-box axes in float64, unit, [15][e][3]; null cross products are replaced by a's first axis"""
    out = [sa.u[:, i] for i in range(3)] + [sb.u[:, j] for j in range(3)]
    for i in range(3):
        for j in range(3):
            L = np.cross(sa.u[:, i], sb.u[:, j])
            ln = np.linalg.norm(L, axis=1)
            out.append(np.where((ln > 1e-6)[:, None], L / np.where(ln > 1e-6, ln, 1.0)[:, None], sa.u[:, 0]))
    return np.stack(out)
