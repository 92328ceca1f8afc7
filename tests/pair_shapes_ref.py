"""Witnesses of the touching pairs (include/sc_tick.h "touching pairs"), independent of the kernels, both brute force
over a given pair list.

    touching32   numpy fp32 written from the header text: one rounding per operation, left to right.  Inputs: the oracle's world matrices
                 (column-major m[c*4 + r]), the Colliders host model of tests/collider_ref.py (None: a context without colliders), the
                 pair list as scTickReadPairs gives it (ids rank << 24 | dense index).  Its decisions are what the device must reproduce
                 exactly; report() turns them into ScTickPairShapeInfo.
    gap64        float64 and a different route: round-round and round-box by golden-section minimisation over the segment parameter of
                 the exact point-segment / point-box distance (convex in t) -- not by the closed forms --, box-box by the separating-axis
                 test in float64.  Returns a signed gap in metres: > 0 apart, < 0 overlapping.  For matrices with orthogonal columns.

    dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z      c_k = column k      T = translation      n_k = dot(c_k, c_k)"""
import numpy as np

from tests import collider_ref as cr
from tests.shape_rays_ref import dot, shape_records

F = np.float32
ZERO, ONE, HALF = F(0.0), F(1.0), F(0.5)
SAT_EPS = F(1e-6)                                              # SC_TICK_PAIR_SHAPES_SAT_EPS
NETWORK = ((1, 6), (2, 4), (3, 5), (2, 3), (4, 5), (1, 4), (3, 6), (1, 2), (3, 4), (5, 6), (2, 3), (4, 5))
INFO_FIELDS = ("tested", "touching", "refined", "kept_as_boxes", "truncated", "pairs_truncated")


def clamp01(x):
    c = np.where(x > ZERO, x, ZERO)
    return np.where(c < ONE, c, ONE).astype(F)


def _members(m, shp, e):
    """columns, translation, column norms and records of entities e (1-D)"""
    R_ = [[m[e, c * 4 + r] for c in range(4)] for r in range(3)]                # R_[r][c]
    col = [[R_[0][c], R_[1][c], R_[2][c]] for c in range(3)]
    T = [R_[r][3] for r in range(3)]
    n = [dot(col[c], col[c]) for c in range(3)]
    return col, T, n, [shp[e, j] for j in range(4)]


def refinable(m, typ, e_ok, e):
    """per id: may the member be refined (e_ok: own rank, below the count; e: the dense index, valid where e_ok)"""
    ee = np.where(e_ok, e, 0)
    t = typ[ee] if len(typ) else np.zeros(len(ee), np.uint8)
    ok = e_ok & ((t == cr.BOX) | (t == cr.SPHERE) | (t == cr.CAPSULE))
    if len(m):
        with np.errstate(all="ignore"):
            _, _, n, _ = _members(m, np.zeros((len(m), 4), F), ee)
            for k in range(3):
                ok &= (n[k] > ZERO) & np.isfinite(n[k])
    return ok


def _round(col, n, s, typ):
    """(A[3], R) of spheres and capsules"""
    sph = typ == cr.SPHERE
    nyz = np.where(n[2] < n[1], n[1], n[2])
    Rs = s[3] * np.sqrt(np.where(n[0] < nyz, nyz, n[0]))
    Rc = s[3] * np.sqrt(np.where(n[0] < n[2], n[2], n[0]))
    A = [col[1][i] * s[1] for i in range(3)]
    axis = ~sph & (dot(A, A) > ZERO)
    A = [np.where(axis, A[i], ZERO).astype(F) for i in range(3)]
    return A, np.where(sph, Rs, Rc).astype(F)


def _round_round_apart(ma, mb):
    (ca, Ta, na, sa, ta), (cb, Tb, nb, sb, tb) = ma, mb
    Aa, Ra = _round(ca, na, sa, ta)
    Ab, Rb = _round(cb, nb, sb, tb)
    p1 = [Ta[i] - Aa[i] for i in range(3)]; d1 = [Aa[i] + Aa[i] for i in range(3)]
    p2 = [Tb[i] - Ab[i] for i in range(3)]; d2 = [Ab[i] + Ab[i] for i in range(3)]
    r = [p1[i] - p2[i] for i in range(3)]
    a, e, f = dot(d1, d1), dot(d2, d2), dot(d2, r)
    c, b = dot(d1, r), dot(d1, d2)
    den = a * e - b * b
    # not a > 0
    s_0 = np.zeros_like(a)
    t_0 = np.where(e > ZERO, clamp01(f / e), ZERO)
    # a > 0, not e > 0
    s_1 = clamp01((-c) / a)
    t_1 = np.zeros_like(a)
    # both
    s_2 = np.where(den > ZERO, clamp01((b * f - c * e) / den), ZERO).astype(F)
    t_2 = (b * s_2 + f) / e
    below, above = t_2 < ZERO, ~(t_2 < ZERO) & (t_2 > ONE)
    s_2 = np.where(below, clamp01((-c) / a), np.where(above, clamp01((b - c) / a), s_2))
    t_2 = np.where(below, ZERO, np.where(above, ONE, t_2))
    hasA, hasE = a > ZERO, e > ZERO
    s = np.where(~hasA, s_0, np.where(~hasE, s_1, s_2)).astype(F)
    t = np.where(~hasA, t_0, np.where(~hasE, t_1, t_2)).astype(F)
    v = [(p1[i] + d1[i] * s) - (p2[i] + d2[i] * t) for i in range(3)]
    total = Ra + Rb
    d2_ = dot(v, v)
    assert d2_.dtype == F and total.dtype == F
    return d2_ > total * total


def _frame(col, n, s):
    q = [np.sqrt(n[k]) for k in range(3)]
    u = [[col[k][i] / q[k] for i in range(3)] for k in range(3)]
    H = [s[k] * q[k] for k in range(3)]
    return u, H


def _box_dist2(y0, dy, H, t):
    g = []
    for k in range(3):
        x = np.abs(y0[k] + dy[k] * t) - H[k]
        g.append(np.where(x > ZERO, x, ZERO).astype(F))
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]


def _round_box_apart(mr, mx):
    (cr_, Tr, nr, sr_, tr), (cx, Tx, nx, sx, _) = mr, mx
    A, R = _round(cr_, nr, sr_, tr)
    u, H = _frame(cx, nx, sx)
    w = [Tr[i] - Tx[i] for i in range(3)]
    y0, dy = [], []
    for k in range(3):
        yc, ya = dot(u[k], w), dot(u[k], A)
        y0.append(yc - ya); dy.append(ya + ya)
    f0 = _box_dist2(y0, dy, H, ZERO)
    fmin = f0
    least = lambda m_, x: np.where(x < m_, x, m_)                               # noqa: E731
    fmin = least(fmin, _box_dist2(y0, dy, H, ONE))
    b = [np.zeros_like(f0)] + [None] * 6 + [np.ones_like(f0)]
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
        fmin = least(fmin, _box_dist2(y0, dy, H, ts))
        if i < 6:
            fmin = least(fmin, _box_dist2(y0, dy, H, hi))
    point = (A[0] == ZERO) & (A[1] == ZERO) & (A[2] == ZERO)
    fmin = np.where(point, f0, fmin)
    assert fmin.dtype == F and R.dtype == F
    return fmin > R * R


def _box_box_apart(ma, mb):
    (ca, Ta, na, sa, _), (cb, Tb, nb, sb, _) = ma, mb
    ua, Ha = _frame(ca, na, sa)
    ub, Hb = _frame(cb, nb, sb)
    w = [Tb[i] - Ta[i] for i in range(3)]
    t = [dot(w, ua[i]) for i in range(3)]
    Rm = [[dot(ua[i], ub[j]) for j in range(3)] for i in range(3)]
    Q = [[np.abs(Rm[i][j]) + SAT_EPS for j in range(3)] for i in range(3)]
    apart = np.zeros(len(t[0]), bool)
    for i in range(3):
        rb = (Hb[0] * Q[i][0] + Hb[1] * Q[i][1]) + Hb[2] * Q[i][2]
        apart |= np.abs(t[i]) > Ha[i] + rb
    for j in range(3):
        ra = (Ha[0] * Q[0][j] + Ha[1] * Q[1][j]) + Ha[2] * Q[2][j]
        tl = (t[0] * Rm[0][j] + t[1] * Rm[1][j]) + t[2] * Rm[2][j]
        apart |= np.abs(tl) > ra + Hb[j]
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            ra = Ha[i1] * Q[i2][j] + Ha[i2] * Q[i1][j]
            rb = Hb[j1] * Q[i][j2] + Hb[j2] * Q[i][j1]
            tl = t[i2] * Rm[i1][j] - t[i1] * Rm[i2][j]
            assert tl.dtype == F and ra.dtype == F
            apart |= np.abs(tl) > ra + rb
    return apart


def touching32(matrices, col, pairs, n=None, rank=0):
    """(touching, refined) per pair of `pairs` [k][2] (ids): bool arrays.  col None = no colliders were uploaded; n = the entity count
    (default: every matrix); rank = the answering context's."""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    m = np.ascontiguousarray(matrices, F).reshape(-1, 16)
    n = len(m) if n is None else n
    m = m[:n]
    typ, shp = shape_records(col, n) if col is not None else (np.zeros(n, np.uint8), np.zeros((n, 4), F))
    k = len(pairs)
    touching, refined = np.ones(k, bool), np.zeros(k, bool)
    if not k or col is None:
        return touching, refined
    e = (pairs & 0xFFFFFF).astype(np.int64)
    e_ok = ((pairs >> 24) == rank) & (e < n)
    ok = np.stack([refinable(m, typ, e_ok[:, s], e[:, s]) for s in range(2)], axis=1)
    refined = ok[:, 0] & ok[:, 1]
    idx = np.flatnonzero(refined)
    if not len(idx):
        return touching, refined
    ea, eb = e[idx, 0], e[idx, 1]
    with np.errstate(all="ignore"):
        ma = _members(m, shp, ea) + (typ[ea],)
        mb = _members(m, shp, eb) + (typ[eb],)
        boxa, boxb = typ[ea] == cr.BOX, typ[eb] == cr.BOX
        apart = np.where(boxa & boxb, _box_box_apart(ma, mb),
                         np.where(boxa, _round_box_apart(mb, ma), np.where(boxb, _round_box_apart(ma, mb), _round_round_apart(ma, mb))))
    touching[idx] = ~apart
    return touching, refined


def report(touching, refined, max_touching, pairs_truncated=False):
    """ScTickPairShapeInfo as a dict"""
    k = int(touching.sum())
    return dict(tested=len(touching), touching=k, refined=int(refined.sum()), kept_as_boxes=int((~refined).sum()),
                truncated=int(k > max_touching), pairs_truncated=int(bool(pairs_truncated)))


def keys(pairs):
    p = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2).astype(np.uint64)
    return (p[:, 0] << np.uint64(32)) | p[:, 1]


def type_pair(col, pairs):
    """0..5 per pair: the unordered pair of collider types among BOX, SPHERE, CAPSULE (box-box 0, box-sphere 1, box-capsule 2,
    sphere-sphere 3, sphere-capsule 4, capsule-capsule 5); -1 when a member has another type"""
    p = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2) & 0xFFFFFF
    ta, tb = col.type[p[:, 0]].astype(np.int64) - cr.BOX, col.type[p[:, 1]].astype(np.int64) - cr.BOX
    lo, hi = np.minimum(ta, tb), np.maximum(ta, tb)
    table = np.array([[0, 1, 2], [-1, 3, 4], [-1, -1, 5]])
    ok = (lo >= 0) & (hi <= 2)
    return np.where(ok, table[np.clip(lo, 0, 2), np.clip(hi, 0, 2)], -1)


# ---- float64, by another route --------------------------------------------------------------------------------------
GOLD = (np.sqrt(5.0) - 1.0) / 2.0


def _golden(g, k, iters=90):
    """minimum over t in [0, 1] of the convex g (vectorised over k problems)"""
    lo, hi = np.zeros(k), np.ones(k)
    x1, x2 = hi - GOLD * (hi - lo), lo + GOLD * (hi - lo)
    g1, g2 = g(x1), g(x2)
    for _ in range(iters):
        left = g1 < g2
        hi = np.where(left, x2, hi); lo = np.where(left, lo, x1)
        nx1, nx2 = hi - GOLD * (hi - lo), lo + GOLD * (hi - lo)
        x1, x2 = nx1, nx2
        g1, g2 = g(x1), g(x2)
    return np.minimum(np.minimum(g1, g2), np.minimum(g(np.zeros(k)), g(np.ones(k))))


def _members64(m, shp, e):
    M = np.asarray(m[e], np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)      # M[:, r, c]
    col = [M[:, :3, k] for k in range(3)]
    T = M[:, :3, 3]
    nk = [np.einsum("ij,ij->i", c, c) for c in col]
    return col, T, nk, np.asarray(shp[e], np.float64)


def _round64(col, nk, s, typ):
    sph = typ == cr.SPHERE
    R = s[:, 3] * np.sqrt(np.where(sph, np.maximum(np.maximum(nk[0], nk[1]), nk[2]), np.maximum(nk[0], nk[2])))
    A = col[1] * s[:, 1:2]
    A[sph] = 0.0
    return A, R


def _point_segment(p, a, d):
    """distance of points p from the segments a + d*[0, 1]"""
    dd = np.einsum("ij,ij->i", d, d)
    with np.errstate(all="ignore"):
        t = np.where(dd > 0, np.einsum("ij,ij->i", p - a, d) / np.where(dd > 0, dd, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    return np.linalg.norm(p - (a + d * t[:, None]), axis=1)


def gap64(matrices, col, pairs):
    """signed gap in metres of every pair (dense indices; every member typed BOX, SPHERE or CAPSULE, columns orthogonal): > 0 apart"""
    p = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2) & 0xFFFFFF
    m = np.ascontiguousarray(matrices, F).reshape(-1, 16)
    typ, shp = shape_records(col, len(m))
    ea, eb = p[:, 0].astype(np.int64), p[:, 1].astype(np.int64)
    # a box, when there is one, goes second
    swap = (typ[ea] == cr.BOX) & (typ[eb] != cr.BOX)
    ea, eb = np.where(swap, eb, ea), np.where(swap, ea, eb)
    ca, Ta, na, sa = _members64(m, shp, ea)
    cb, Tb, nb, sb = _members64(m, shp, eb)
    k = len(ea)
    out = np.zeros(k)
    boxa, boxb = typ[ea] == cr.BOX, typ[eb] == cr.BOX
    Aa, Ra = _round64(ca, na, sa, typ[ea])
    Ab, Rb = _round64(cb, nb, sb, typ[eb])
    ub = [cb[j] / np.sqrt(nb[j])[:, None] for j in range(3)]
    Hb = np.stack([sb[:, j] * np.sqrt(nb[j]) for j in range(3)], axis=1)
    # round - round: the point of segment a at t against segment b
    rr = _golden(lambda t: _point_segment(Ta - Aa + 2.0 * Aa * t[:, None], Tb - Ab, 2.0 * Ab), k) - (Ra + Rb)

    def to_box(t):                                                             # round - box: the point of segment a at t against box b
        q = Ta - Aa + 2.0 * Aa * t[:, None] - Tb
        y = np.stack([np.einsum("ij,ij->i", q, ub[j]) for j in range(3)], axis=1)
        return np.linalg.norm(np.maximum(np.abs(y) - Hb, 0.0), axis=1)

    rb = _golden(to_box, k) - Ra
    # box - box: the largest separation over the fifteen axes, normalised
    ua = [ca[i] / np.sqrt(na[i])[:, None] for i in range(3)]
    Ha = np.stack([sa[:, i] * np.sqrt(na[i]) for i in range(3)], axis=1)
    w = Tb - Ta
    axes = ua + ub + [np.cross(ua[i], ub[j]) for i in range(3) for j in range(3)]
    bb = np.full(k, -np.inf)
    for L in axes:
        ln = np.linalg.norm(L, axis=1)
        good = ln > 1e-9
        Ln = L / np.where(good, ln, 1.0)[:, None]
        ra = sum(Ha[:, i] * np.abs(np.einsum("ij,ij->i", ua[i], Ln)) for i in range(3))
        rbb = sum(Hb[:, j] * np.abs(np.einsum("ij,ij->i", ub[j], Ln)) for j in range(3))
        sep = np.abs(np.einsum("ij,ij->i", w, Ln)) - ra - rbb
        bb = np.where(good, np.maximum(bb, sep), bb)
    out = np.where(boxa & boxb, bb, np.where(boxb, rb, rr))
    return out
