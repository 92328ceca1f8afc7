"""Exact collider shapes for rays without a GPU: the ABI surface, and the witness (tests/shape_rays_ref.py) the GPU tests compare
against -- in AABB mode it is the oracle's raycast_boxes bit for bit, in EXACT mode it agrees with the same shapes evaluated in float64,
and the seeds of the GPU suite's random case give it enough winners of every kind."""
import ctypes as C
import os
import re

import numpy as np

from sc_gameengine_amd import capi
from tests import collider_ref as cr, shape_rays_cases as G, shape_rays_ref as sr, worlds

F = np.float32
ALL = 0xFFFFFFFF
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sc_tick.h")


def oracle_state(oracle, w, col):
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    out = (ow.world_matrices()[:w.n], *col.witness(ow, w.n))
    ow.close()
    return out


def random_rays(rng, k, centre, n):
    target = rng.integers(0, n, k)
    away = rng.normal(size=(k, 3)).astype(F)
    away /= np.linalg.norm(away, axis=1, keepdims=True).astype(F)
    o = (centre[target] + away * rng.uniform(2, 25, (k, 1)).astype(F)).astype(F)
    d = ((centre[target] + rng.normal(size=(k, 3)).astype(F) * F(0.8)) - o).astype(F)
    return o, d, rng.uniform(5, 60, k).astype(F), np.full(k, ALL, np.uint32)


def test_ray_shape_symbols_are_exported_and_bound():
    lib = capi.load()
    for name in ("scTickSetRayShapes", "scTickGetRayShapes"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert lib.scTickGetApiVersion() == 7
    assert capi.SYMBOLS["scTickSetRayShapes"] == (C.c_int, [C.c_void_p, C.c_uint32])
    assert capi.SYMBOLS["scTickGetRayShapes"] == (C.c_int, [C.c_void_p, capi.U32P])
    assert (capi.RAY_SHAPES_AABB, capi.RAY_SHAPES_EXACT) == (0, 1) == (sr.AABB, sr.EXACT)
    text = open(HEADER).read()
    assert re.search(r"enum\s*\{\s*SC_TICK_RAY_SHAPES_AABB\s*=\s*0\s*,\s*SC_TICK_RAY_SHAPES_EXACT\s*=\s*1\s*\}", text)
    # a NULL context: every call returns 0
    mode = C.c_uint32(5)
    assert lib.scTickSetRayShapes(None, 0) == 0 and lib.scTickSetRayShapes(None, 1) == 0
    assert lib.scTickGetRayShapes(None, C.byref(mode)) == 0 and lib.scTickGetRayShapes(None, None) == 0
    assert mode.value == 5


def test_the_witness_in_aabb_mode_is_the_oracles_raycast_boxes(oracle):
    w = worlds.random_world(1500, seed=301, spread=80.0, max_depth=3)
    rng = np.random.default_rng(302)
    col = cr.Colliders.random(w.n, rng)
    m, mn, mx = oracle_state(oracle, w, col)
    k = 2000
    o, d, md, mask = random_rays(rng, k, m[:, 12:15], w.n)
    d[:200, 0] = 0.0; d[200:300, [1, 2]] = 0.0                                  # the parallel-axis rule
    o[300:500] = m[rng.integers(0, w.n, 200), 12:15]                            # from inside
    d[500:520] *= F(1e-5)                                                       # no segment
    md[520:540] = -1.0
    mask[:] = rng.choice(np.array([1, 2, 3, ALL], np.uint32), k)
    want = oracle.raycast_boxes(mn, mx, w.group, w.mask, o, d, md, mask)
    got = sr.cast(m, mn, mx, w.group, w.mask, col, o, d, md, mask, mode=sr.AABB)
    assert got.tobytes() == want.tobytes()
    assert want["hit"].sum() > 800 and (want["hit"] == 0).sum() > 100 and (want["distance"][want["hit"] == 1] == 0).sum() > 100
    # a context without colliders refines nothing, whatever the mode
    assert sr.cast(m, mn, mx, w.group, w.mask, None, o, d, md, mask, mode=sr.EXACT).tobytes() == want.tobytes()


# ---- the witness against geometry -----------------------------------------------------------------------------------
GEOMETRY_SEEDS = (311, 312, 313)
# The largest |fp32 - float64| distance over the committed seeds is 1.991e-4 m (measured here, on the CPU: seed 311; coordinates up to
# 100 m, where an ulp is 7.6e-6 m).  The bound is four times that: the error grows with the coordinates' ulp, another seed may sit a
# little higher.
GEOMETRY_MEASURED = 1.991e-4
GEOMETRY_BOUND = 4 * GEOMETRY_MEASURED
ILL = 1e-3


def geometry_case(oracle, seed):
    """(hit/id agreement, largest distance error, excluded share) of one seed: roots only, so every matrix has orthogonal columns"""
    w = worlds.random_world(600, seed=seed, spread=70.0, p_child=0.0, p_no_bounds=0.0)
    rng = np.random.default_rng([seed, 7])
    col = cr.Colliders.random(w.n, rng, p=(0.1, 0.1, 0.3, 0.25, 0.25))
    col.hh[:] = np.maximum(col.hh, F(0.0))
    m, mn, mx = oracle_state(oracle, w, col)
    k = 500
    o, d, md, mask = random_rays(rng, k, m[:, 12:15], w.n)
    got = sr.cast(m, mn, mx, w.group, w.mask, col, o, d, md, mask)
    typ, shp = sr.shape_records(col)
    valid, dirs = sr.normalise(d, md)
    assert valid.all()
    mn64, mx64 = mn.astype(np.float64), mx.astype(np.float64)
    excluded, worst, disagree = 0, 0.0, []
    for r in range(k):
        o64, d64 = o[r].astype(np.float64), dirs[r].astype(np.float64)
        d64 /= np.linalg.norm(d64)
        L = float(md[r])
        with np.errstate(all="ignore"):                                          # candidates: the float64 slab test against the boxes, a millimetre wider
            t1, t2 = (mn64 - ILL - o64) / d64, (mx64 + ILL - o64) / d64
            lo, hi = np.minimum(t1, t2).max(axis=1), np.maximum(t1, t2).min(axis=1)
        cands = np.flatnonzero((np.maximum(lo, 0.0) <= np.minimum(hi, L)) & (mn[:, 0] <= mx[:, 0]))
        best, best_e, margin = None, -1, np.inf
        for e in cands:
            if typ[e] >= cr.BOX:
                t, mg = sr.shape_t64(m, typ, shp, e, o64, d64, L)
            else:                                                                # a Bounds proxy: the box itself
                with np.errstate(all="ignore"):
                    s1, s2 = (mn64[e] - o64) / d64, (mx64[e] - o64) / d64
                a, b = max(np.minimum(s1, s2).max(), 0.0), min(np.maximum(s1, s2).min(), L)
                t, mg = (a if a <= b else None), abs(b - a)
            margin = min(margin, mg)
            if t is not None and (best is None or t < best):
                best, best_e = t, int(e)
        if margin < ILL:
            excluded += 1
            continue
        if (best is not None) != bool(got["hit"][r]) or (best is not None and best_e != int(got["id"][r])):
            disagree.append(r)
        elif best is not None:
            worst = max(worst, abs(float(got["distance"][r]) - best))
    return disagree, worst, excluded / k, int(got["hit"].sum())


def test_the_witness_agrees_with_the_shapes_in_float64(oracle):
    worst = 0.0
    for seed in GEOMETRY_SEEDS:
        disagree, err, share, hits = geometry_case(oracle, seed)
        print(f"seed {seed}: largest |fp32 - float64| distance {err:.3e} m, excluded {share:.3f}, hits {hits}, disagreements {disagree}")
        assert share <= 0.05 and hits > 200
        assert not disagree
        worst = max(worst, err)
    print(f"largest distance error over the seeds: {worst:.3e} m (bound {GEOMETRY_BOUND:.3e})")
    assert worst <= GEOMETRY_BOUND
    assert worst >= GEOMETRY_MEASURED / 2                                        # (the comment above is the measurement)


# ---- properties -----------------------------------------------------------------------------------------------------
def test_properties_of_the_witness(oracle):
    w = worlds.random_world(1200, seed=321, spread=60.0, max_depth=3)
    rng = np.random.default_rng(322)
    col = cr.Colliders.random(w.n, rng)
    col.hh[:] = np.maximum(col.hh, F(0.0))
    m, mn, mx = oracle_state(oracle, w, col)
    k = 1500
    q = random_rays(rng, k, m[:, 12:15], w.n)
    exact = sr.cast(m, mn, mx, w.group, w.mask, col, *q)
    plain = sr.cast(m, mn, mx, w.group, w.mask, col, *q, mode=sr.AABB)
    hit = exact["hit"] == 1
    # every exact hit is also an AABB hit
    assert (plain["hit"][hit] == 1).all()
    assert hit.sum() > 400 and ((plain["hit"] == 1) & ~hit).sum() > 50
    # never -0
    assert not np.signbit(exact["distance"]).any() and (exact["distance"][~hit] == 0).all()
    typ, shp = sr.shape_records(col)
    # (entity, ray) pairs: every ray against the entity it met in AABB mode, and against a random one
    ray = np.concatenate([np.flatnonzero(plain["hit"] == 1), np.arange(k)])
    e = np.concatenate([plain["id"][plain["hit"] == 1].astype(np.int64), rng.integers(0, w.n, k)])
    o = [q[0][ray, i] for i in range(3)]
    _, d = sr.normalise(q[1], q[2])
    kind, t, _ = sr.refine(m, typ, shp, e, o, [d[ray, i] for i in range(3)], q[2][ray])
    assert not np.signbit(t).any() and set(np.unique(kind)) <= {0, sr.MISS, sr.HIT}

    # a capsule without height answers with the bits of roundHit at its own R
    flat = cr.Colliders(w.n)
    flat.type[:] = cr.CAPSULE; flat.radius[:] = col.radius; flat.hh[:] = 0.0
    typ, shp = sr.shape_records(flat)
    col0, col2 = [m[e, r] for r in range(3)], [m[e, 8 + r] for r in range(3)]
    n0, n2 = sr.dot(col0, col0), sr.dot(col2, col2)
    R = shp[e, 3] * np.sqrt(np.where(n0 < n2, n2, n0))
    qc = [o[r] - m[e, 12 + r] for r in range(3)]
    dd = [d[ray, i] for i in range(3)]
    rk, rt, rn = sr.round_hit(qc, R, dd, q[2][ray])
    kind, t, nrm = sr.refine(m, typ, shp, e, o, dd, q[2][ray])
    h = rk == sr.HIT
    assert np.array_equal(kind == sr.HIT, (rk == sr.HIT) | (rk == sr.INSIDE)) and h.sum() > 100
    assert np.array_equal(t[h].view(np.uint32), rt[h].view(np.uint32))
    assert all(np.array_equal(nrm[i][h].view(np.uint32), rn[i][h].view(np.uint32)) for i in range(3))

    # an identity box at the origin answers with the AABB mode's bits
    he, rays = G.identity_box_rays()
    one = cr.Colliders(1)
    one.type[:] = cr.BOX; one.he[:] = he
    eye = np.eye(4, dtype=F).reshape(1, 16)
    a = sr.cast(eye, -he[None], he[None], [1], [ALL], one, *rays, mode=sr.AABB)
    b = sr.cast(eye, -he[None], he[None], [1], [ALL], one, *rays, mode=sr.EXACT)
    assert a.tobytes() == b.tobytes() and 300 < a["hit"].sum() < 800
    assert a.tobytes() == oracle.raycast_boxes(-he[None], he[None], [1], [ALL], *rays).tobytes()


def test_the_gpu_suites_random_case_has_enough_winners_of_every_kind(oracle):
    w, col, q = G.random_case(oracle)
    ow = worlds.oracle_world(oracle, w, camera=False)
    for tick in range(2):
        if tick:
            ow.nudge_roots_x(G.NUDGE)
        ow.transform_system()
        want = G.witness(ow, w, col, q)
        counts, differ = G.winner_counts(want, G.witness(ow, w, col, q, mode=sr.AABB), col)
        print(counts, differ)
        assert all(counts[k] >= 100 for k in counts) and differ >= 200, (counts, differ)
    mn, mx = col.witness(ow, w.n)
    assert ((mx[:, 0] - mn[:, 0]) > 128.0).sum() >= 20      # the plates: wider than two sectors
    ow.close()
