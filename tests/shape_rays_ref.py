"""Witness of the exact collider shapes for rays (include/sc_tick.h "exact shapes for rays"), independent of the
kernels and written from the header text: numpy fp32, one rounding per operation, left to right, brute force over every entity for
every ray.

    inputs    the oracle's world matrices (column-major m[c*4 + r]), the witness boxes of tests/collider_ref.py (every entity's proxy
              AABB; +inf / -inf = no proxy), the layers as uploaded, the Colliders host model, the rays
    AABB      the slab test (intersectRayAABB with the far limit at max_dist) restated here in numpy; in AABB mode cast() must equal the
              oracle's raycast_boxes bit for bit (tests/test_shape_rays_cpu.py checks that once)
    EXACT     an AABB hit of a typed collider (BOX, SPHERE, CAPSULE) is refined by the shape taken through the entity's matrix; a BOUNDS
              proxy keeps its AABB answer

    dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z      c_k = column k      T = translation      n_k = dot(c_k, c_k)      q = o - T

cast() returns the ScTickRayHit fields; shape_t64() evaluates the same shapes in float64 for the geometry check."""
import numpy as np

from tests import collider_ref as cr

F = np.float32
NO_ID = 0xFFFFFFFF
HIT_DTYPE = np.dtype([("hit", np.uint32), ("id", np.uint32), ("distance", np.float32), ("position", np.float32, 3),
                      ("normal", np.float32, 3), ("layer", np.uint32), ("pad", np.uint32, 2)])
AABB, EXACT = 0, 1
ZERO, ONE, EPS = F(0.0), F(1.0), F(1e-6)


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def not_negative(t):
    return np.where(t > ZERO, t, ZERO)


def slab(o, d, far, mn, mx):
    """intersectRayAABB with tmax = far over arrays: o, d, mn, mx are 3-lists of broadcastable fp32 arrays; (hit, t, axis)."""
    shape = np.broadcast(o[0], d[0], far, mn[0], mx[0]).shape
    hit = np.ones(shape, bool)
    tmin, tmax = np.zeros(shape, F), np.broadcast_to(far, shape).astype(F)
    axis = np.full(shape, 3, np.int32)
    with np.errstate(all="ignore"):
        for i in range(3):
            par = np.broadcast_to(np.abs(d[i]) < EPS, shape)
            outside = (o[i] < mn[i]) | (o[i] > mx[i])
            ood = ONE / d[i]
            t1, t2 = (mn[i] - o[i]) * ood, (mx[i] - o[i]) * ood
            swap = t1 > t2
            t1, t2 = np.where(swap, t2, t1), np.where(swap, t1, t2)
            grow = ~par & (t1 > tmin)
            tmin = np.where(grow, t1, tmin)
            axis = np.where(grow, i, axis)
            tmax = np.where(par, tmax, np.where(tmax < t2, tmax, t2))
            hit &= np.where(par, ~outside, ~(tmin > tmax))
    assert tmin.dtype == F
    return hit, tmin, axis


MISS, HIT, INSIDE = 1, 2, 3


def round_hit(qc, R, d, L):
    """roundHit(qc, R) over 1-D arrays: (kind, t, normal[3])"""
    with np.errstate(all="ignore"):
        b = dot(qc, d)
        c = dot(qc, qc) - R * R
        disc = b * b - c
        t = not_negative((-b) - np.sqrt(disc))
        inside = c <= ZERO
        ok = ~inside & (b < ZERO) & (disc >= ZERO) & (t <= L)
        nrm = [(qc[r] + d[r] * t) / R for r in range(3)]
    kind = np.where(inside, INSIDE, np.where(ok, HIT, MISS))
    assert t.dtype == F and nrm[0].dtype == F
    return kind, t, nrm


def refine(m, ctype, shape4, e, o, d, L):
    """The shapes of entities e (1-D) against rays (o, d, L) (3-lists of 1-D arrays, one ray per e): (kind, t, normal[3]) with
    kind 0 = the AABB answer stands, MISS, HIT (inside is a hit at t = +0 with normal (0, 1, 0))."""
    k = len(e)
    R_ = [[m[e, c * 4 + r] for c in range(4)] for r in range(3)]                # R_[r][c]
    col = [[R_[0][c], R_[1][c], R_[2][c]] for c in range(3)]
    q = [o[r] - R_[r][3] for r in range(3)]
    n = [dot(col[c], col[c]) for c in range(3)]
    ex, ey, ez, rad = (shape4[e, j] for j in range(4))
    typ = ctype[e]
    kind = np.zeros(k, np.int32)
    t = np.zeros(k, F)
    nrm = [np.zeros(k, F), np.ones(k, F), np.zeros(k, F)]
    with np.errstate(all="ignore"):
        # BOX
        good = (n[0] > ZERO) & (n[1] > ZERO) & (n[2] > ZERO) & np.isfinite(n[0]) & np.isfinite(n[1]) & np.isfinite(n[2])
        lo = [dot(col[c], q) / n[c] for c in range(3)]
        ld = [dot(col[c], d) / n[c] for c in range(3)]
        bh, bt, bax = slab(lo, ld, L, [-ex, -ey, -ez], [ex, ey, ez])
        box = (typ == cr.BOX) & good
        kind[box] = np.where(bh, HIT, MISS)[box]
        t[box] = bt[box]
        for a in range(3):
            face = box & bh & (bax == a)
            sgn = np.where(ld[a] > ZERO, F(-1.0), ONE)
            inv = ONE / np.sqrt(n[a])
            for r in range(3):
                nrm[r][face] = (sgn * (col[a][r] * inv) + ZERO)[face]
        # SPHERE and CAPSULE: the radius of the round part, the maximum selected as the collider's AABB selects it
        sph, cap = typ == cr.SPHERE, typ == cr.CAPSULE
        nyz = np.where(sph & (n[2] < n[1]), n[1], n[2])
        R = rad * np.sqrt(np.where(n[0] < nyz, nyz, n[0]))
        sk, st, sn = round_hit(q, R, d, L)
        A = [col[1][r] * ey for r in range(3)]
        aa = dot(A, A)
        as_sphere = sph | (cap & ~(aa > ZERO))
        kind[as_sphere] = sk[as_sphere]
        t[as_sphere] = st[as_sphere]
        for r in range(3):
            nrm[r][as_sphere] = sn[r][as_sphere]
        # CAPSULE with an axis
        ad, aq, dq, qq = dot(A, d), dot(A, q), dot(d, q), dot(q, q)
        ka = aa - ad * ad
        kb = aa * dq - aq * ad
        kc = (aa * qq - aq * aq) - (R * R) * aa
        in_body = (kc <= ZERO) & (-aa <= aq) & (aq <= aa)
        disc = kb * kb - ka * kc
        tb = not_negative(((-kb) - np.sqrt(disc)) / ka)
        yb = aq + tb * ad
        side = (kc > ZERO) & (ka > ZERO) & (kb < ZERO) & (disc >= ZERO) & (-aa <= yb) & (yb <= aa) & (tb <= L)
        f = yb / aa
        side_n = [((q[r] + d[r] * tb) - A[r] * f) / R for r in range(3)]
        pk, pt, pn = round_hit([q[r] + A[r] for r in range(3)], R, d, L)
        mk, mt, mn_ = round_hit([q[r] - A[r] for r in range(3)], R, d, L)
        inside = in_body | (pk == INSIDE) | (mk == INSIDE)
        ck = np.where(side, HIT, MISS)
        ct = np.where(side, tb, ZERO)
        cn = [np.where(side, side_n[r], nrm[r]) for r in range(3)]
        for k2, t2, n2 in ((pk, pt, pn), (mk, mt, mn_)):
            take = (k2 == HIT) & ((ck != HIT) | (t2 < ct))
            ck = np.where(take, HIT, ck)
            ct = np.where(take, t2, ct)
            cn = [np.where(take, n2[r], cn[r]) for r in range(3)]
        ck = np.where(inside, INSIDE, ck)
        axial = cap & (aa > ZERO)
        kind[axial] = ck[axial]
        t[axial] = ct[axial]
        for r in range(3):
            nrm[r][axial] = cn[r][axial]
    ins = kind == INSIDE
    kind[ins] = HIT
    t[ins] = ZERO
    nrm[0][ins], nrm[1][ins], nrm[2][ins] = ZERO, ONE, ZERO
    assert t.dtype == F and all(x.dtype == F for x in nrm)
    return kind, t, nrm


def shape_records(col, n=None):
    """(type, [n][4] (ex, ey, ez, radius)) as the device holds them: the record of tests/collider_ref.py's box rule."""
    n = len(col.type) if n is None else n
    typ = np.asarray(col.type[:n], np.uint8)
    s = np.zeros((n, 4), F)
    box, sph, cap = typ == cr.BOX, typ == cr.SPHERE, typ == cr.CAPSULE
    s[box, :3] = col.he[:n][box]
    s[sph, 3] = col.radius[:n][sph]
    s[cap, 1] = np.maximum(F(0.0), col.hh[:n][cap])
    s[cap, 3] = col.radius[:n][cap]
    return typ, s


def normalise(direction, max_dist):
    """(valid, dir): the rays' normalisation -- no segment when |d|^2 <= 1e-6 or the length is negative (or either is a NaN)"""
    dv = np.ascontiguousarray(direction, F).reshape(-1, 3)
    md = np.ascontiguousarray(max_dist, F).reshape(-1)
    with np.errstate(all="ignore"):
        len_sq = dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1] + dv[:, 2] * dv[:, 2]
        valid = (len_sq > EPS) & (md >= ZERO)
        inv = ONE / np.sqrt(len_sq)
        d = dv * inv[:, None]
    assert d.dtype == F
    return valid, d


def cast(matrices, mn, mx, group, mask, col, origin, direction, max_dist, ray_mask, mode=EXACT, skip=None, own=None, chunk=256):
    """Structured array like WorldTick.ray_hits().  col: the Colliders host model (None: a context without colliders -- nothing is
    refined); skip: per ray, the dense index of a box that never answers (negative: none); own: which entities are the answering
    context's own (default all) -- a neighbour tile's records keep their AABB answer."""
    m = np.ascontiguousarray(matrices, F).reshape(-1, 16)
    mn, mx = np.ascontiguousarray(mn, F).reshape(-1, 3), np.ascontiguousarray(mx, F).reshape(-1, 3)
    n = len(mn)
    m = m[:n]
    g16 = np.ascontiguousarray(group, np.uint32)[:n] & 0xFFFF
    m16 = np.ascontiguousarray(mask, np.uint32)[:n] & 0xFFFF
    o = np.ascontiguousarray(origin, F).reshape(-1, 3)
    md = np.ascontiguousarray(max_dist, F).reshape(-1)
    rm = np.ascontiguousarray(ray_mask, np.uint32).reshape(-1)
    k = len(o)
    sk = np.full(k, -1, np.int64) if skip is None else np.ascontiguousarray(skip, np.int64).reshape(k)
    valid, d = normalise(direction, md)
    typ, shp = shape_records(col, n) if col is not None else (np.zeros(n, np.uint8), np.zeros((n, 4), F))
    typed = (typ == cr.BOX) | (typ == cr.SPHERE) | (typ == cr.CAPSULE)
    if own is not None:
        typed &= np.asarray(own, bool)[:n]
    has_box = mn[:, 0] <= mx[:, 0]
    out = np.zeros(k, HIT_DTYPE)
    out["id"] = NO_ID
    out["normal"][:, 1] = 1.0
    ids = np.arange(n)
    for a in range(0, k, chunk):
        rs = np.flatnonzero(valid[a:a + chunk]) + a
        if not len(rs) or not n:
            continue
        O = [o[rs, i][:, None] for i in range(3)]
        D = [d[rs, i][:, None] for i in range(3)]
        hit, t, axis = slab(O, D, md[rs][:, None], [mn[:, i][None] for i in range(3)], [mx[:, i][None] for i in range(3)])
        cand = hit & has_box[None] & ((g16[None] & rm[rs][:, None]) != 0) & (m16[None] != 0) & (ids[None] != sk[rs][:, None])
        # the AABB answer of every candidate
        da = np.select([axis == 0, axis == 1, axis == 2], [np.broadcast_to(D[0], axis.shape), np.broadcast_to(D[1], axis.shape),
                                                           np.broadcast_to(D[2], axis.shape)], ZERO)
        sgn = np.where(da > ZERO, F(-1.0), ONE)
        nrm = [np.where(axis == i, sgn, ZERO).astype(F) for i in range(3)]
        nrm[1] = np.where(axis == 3, ONE, nrm[1])
        t = t.copy()
        if mode == EXACT and col is not None:
            ri, ei = np.nonzero(cand & typed[None])
            if len(ri):
                kind, rt, rn = refine(m, typ, shp, ei, [o[rs[ri], i] for i in range(3)], [d[rs[ri], i] for i in range(3)], md[rs[ri]])
                cand[ri[kind == MISS], ei[kind == MISS]] = False
                h = kind == HIT
                t[ri[h], ei[h]] = rt[h]
                for i in range(3):
                    nrm[i][ri[h], ei[h]] = rn[i][h]
        tt = np.where(cand, t, np.inf)
        win = np.argmin(tt, axis=1)                       # the first of equal distances: the lower id
        rows = np.arange(len(rs))
        found = cand[rows, win]
        w, r = win[found], rs[found]
        bt = t[rows[found], w]
        out["hit"][r] = 1
        out["id"][r] = w
        out["distance"][r] = bt
        out["layer"][r] = g16[w]
        out["position"][r] = o[r] + d[r] * bt[:, None]
        for i in range(3):
            out["normal"][r, i] = nrm[i][rows[found], w]
    return out


# ---- the same shapes in float64: what the geometry check of tests/test_shape_rays_cpu.py compares against ----------------------------
def shape_t64(m, typ, shp, e, o, d, L):
    """Entry distance of ray (o, d unit, L) into the collider of entity e, in float64, for a matrix with orthogonal columns:
    (t or None, margin) -- margin: how far the case is from a decision the fp32 arithmetic could take the other way (relative
    distance from tangency, metres from a box edge or a capsule seam); None = no such decision nearby."""
    M = np.asarray(m[e], np.float64).reshape(4, 4).T                           # M[r, c]
    c = [M[:3, k] for k in range(3)]
    T = M[:3, 3]
    q = np.asarray(o, np.float64) - T
    d = np.asarray(d, np.float64)
    nk = [float(x @ x) for x in c]
    ex, ey, ez, rad = (float(x) for x in shp[e])

    def sphere(qc, R):
        b, cc = float(qc @ d), float(qc @ qc) - R * R
        if cc <= 0:
            return 0.0, abs(cc) / (R * R + 1e-300)
        disc = b * b - cc
        margin = abs(disc) / (R * R + 1e-300)
        if b >= 0 or disc < 0:
            return None, margin
        t = -b - np.sqrt(disc)
        return (t if t <= L else None), min(margin, abs(t - L))

    if typ[e] == cr.BOX:
        s = [np.sqrt(x) for x in nk]
        lo = np.array([c[k] @ q / s[k] for k in range(3)])                     # metres along the box's unit axes
        ld = np.array([c[k] @ d / s[k] for k in range(3)])
        he = np.array([ex * s[0], ey * s[1], ez * s[2]])
        t0, t1 = 0.0, L
        margin = np.inf
        for k in range(3):
            if abs(ld[k]) < 1e-12:
                margin = min(margin, abs(abs(lo[k]) - he[k]))
                if abs(lo[k]) > he[k]:
                    return None, margin
                continue
            a, b = (-he[k] - lo[k]) / ld[k], (he[k] - lo[k]) / ld[k]
            a, b = min(a, b), max(a, b)
            t0, t1 = max(t0, a), min(t1, b)
        # distance of the entry (or of the closest approach of the slabs) from an edge: the gap between the deciding parameters, in metres
        margin = min(margin, abs(t1 - t0))
        if t0 > t1:
            return None, margin
        p = lo + ld * t0
        near = np.sort(he - np.abs(p))
        if t0 > 0:
            margin = min(margin, near[1])                                       # the second smallest: the hit's distance from an edge
        return t0, margin
    if typ[e] == cr.SPHERE:
        return sphere(q, rad * np.sqrt(max(nk)))
    R = rad * np.sqrt(max(nk[0], nk[2]))
    A = c[1] * ey
    aa = float(A @ A)
    if aa <= 0:
        return sphere(q, R)
    u = A / np.sqrt(aa)
    half = np.sqrt(aa)
    best, margin, inside = None, np.inf, False
    for sgnA in (1.0, -1.0):
        t, mg = sphere(q - sgnA * A, R)
        margin = min(margin, mg)
        if t is not None:
            inside |= t == 0.0
            best = t if best is None or t < best else best
    y0, yd = float(q @ u), float(d @ u)
    qp, dp = q - y0 * u, d - yd * u
    a2, b2, c2 = float(dp @ dp), float(qp @ dp), float(qp @ qp) - R * R
    if c2 <= 0 and abs(y0) <= half:
        inside = True
    if c2 <= 0:
        margin = min(margin, abs(abs(y0) - half))
    elif a2 > 1e-18:
        disc = b2 * b2 - a2 * c2
        margin = min(margin, abs(disc) / (a2 * R * R + 1e-300))
        if b2 < 0 and disc >= 0:
            t = (-b2 - np.sqrt(disc)) / a2
            y = y0 + t * yd
            margin = min(margin, abs(abs(y) - half))                            # metres from a seam
            if abs(y) <= half and t <= L:
                best = t if best is None or t < best else best
    if inside:
        return 0.0, margin
    return best, margin
