"""Entity-anchored rays without a GPU: the ABI surface, and the witness (tests/anchored_ref.py) the GPU tests compare against --
an identity anchor is no anchor, a quarter turn about y turns +z into +x as the uploaded sin / cos say, a parent chain composes,
the miss rules hold, and the seeds of the GPU suite's random case give it enough hits and misses on every tick."""
import ctypes as C

import numpy as np

from sc_gameengine_amd import capi
from sc_gameengine_amd import tick as T
from tests import anchored_ref as ar, worlds

F = np.float32
ALL = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def small_world(oracle, pos, rot, scale, parent):
    n = len(pos)
    w = worlds.random_world(n, seed=121, p_child=0.0, p_no_bounds=0.0)
    w.pos[:], w.rot[:], w.scale[:], w.parent[:] = F(pos), F(rot), F(scale), parent
    w.group[:] = 1; w.mask[:] = ALL
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    out = (w, ow.world_matrices(), *ow.world_aabbs())
    ow.close()
    return out


def test_anchored_ray_symbols_are_exported_and_bound():
    lib = capi.load()
    for name in ("scTickSetAnchoredRays", "scTickReadAnchoredRayHits", "scTickReadAnchoredRays"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert capi.ANCHORED_RAYS == 1 << 11 and not (capi.FULL & capi.ANCHORED_RAYS)
    assert not capi.ANCHORED_RAYS & (capi.RAYS | capi.SWEEPS | capi.PRODUCE_NEXT | capi.DENSE_AABBS | 1 << 16 | 1 << 17 | 1 << 18)
    assert (capi.ANCHOR_NONE, capi.ANCHOR_DEAD) == (ar.ANCHOR_NONE, ar.ANCHOR_DEAD) and capi.ANCHOR_DEAD != capi.ANCHOR_NONE
    assert capi.ANCHOR_DEAD > 0xFFFFFF                       # beyond every entity count: a dead anchor misses by the count rule alone
    assert lib.scTickGetApiVersion() == 7
    assert C.sizeof(capi.RayHit) == 48 == ar.HIT_DTYPE.itemsize == T.RAY_HIT_DTYPE.itemsize
    # a NULL context: every call returns 0
    n, one = C.c_uint32(), np.zeros(3, F)
    u = np.zeros(1, np.uint32)
    assert lib.scTickSetAnchoredRays(None, 0, None, None, None, None, None, None) == 0
    assert lib.scTickSetAnchoredRays(None, 1, u.ctypes.data_as(capi.U32P), one.ctypes.data_as(capi.F32P), one.ctypes.data_as(capi.F32P),
                                     one.ctypes.data_as(capi.F32P), u.ctypes.data_as(capi.U32P), None) == 0
    assert lib.scTickReadAnchoredRayHits(None, None, 0, C.byref(n)) == 0
    assert lib.scTickReadAnchoredRays(None, 0, 0, None) == 0
    assert lib.scTickReadAnchoredRays(None, 0, 1, u.ctypes.data_as(capi.U32P)) == 0


def test_an_identity_anchor_is_no_anchor(oracle):
    rng = np.random.default_rng(122)
    n = 40
    pos = rng.uniform(-20, 20, (n, 3)); pos[0] = 0.0
    rot = rng.uniform(-3, 3, (n, 3)); rot[0] = 0.0
    scale = rng.uniform(0.5, 3, (n, 3)); scale[0] = 1.0
    w, m, mn, mx = small_world(oracle, pos, rot, scale, np.full(n, -1, np.int32))
    assert np.array_equal(m[0], np.eye(4, dtype=F).ravel())
    k = 200
    o = rng.uniform(-25, 25, (k, 3)).astype(F)
    d = (rng.normal(size=(k, 3)) * rng.uniform(0.01, 30, (k, 1))).astype(F)
    md, mask = np.full(k, 50.0, F), np.full(k, ALL, np.uint32)
    no_skip = np.zeros(k, np.uint8)
    free = ar.cast(oracle, mn, mx, w.group, w.mask, m, np.full(k, ar.ANCHOR_NONE, np.uint32), o, d, md, mask)
    tied = ar.cast(oracle, mn, mx, w.group, w.mask, m, np.zeros(k, np.uint32), o, d, md, mask, skip_self=no_skip)
    plain = oracle.raycast_boxes(mn, mx, w.group, w.mask, o, d, md, mask)
    assert free.tobytes() == tied.tobytes() == plain.tobytes()
    assert 20 < plain["hit"].sum() < k - 20
    # with the skip on, box 0 never answers -- and nothing else changes for the rays that did not meet it
    skipped = ar.cast(oracle, mn, mx, w.group, w.mask, m, np.zeros(k, np.uint32), o, d, md, mask)
    assert (skipped["id"] != 0).all()
    other = plain["id"] != 0
    assert skipped[other].tobytes() == plain[other].tobytes()


def test_a_quarter_turn_about_y_turns_z_into_x(oracle):
    quarter = F(np.pi / 2)
    w, m, mn, mx = small_world(oracle, [[3, 4, 5], [0, 0, 0]], [[0, quarter, 0], [0, 0, 0]], [[1, 1, 1]] * 2, np.full(2, -1, np.int32))
    o, d, ok = ar.resolve(m, [0], [[0, 0, 0]], [[0, 0, 1]])
    assert ok.all() and np.array_equal(o[0], F([3, 4, 5]))
    s, c = np.sin(quarter, dtype=F), np.cos(quarter, dtype=F)          # what the upload takes with the host's libm, to an ulp
    assert abs(d[0, 0] - s) <= np.spacing(s) and d[0, 1] == 0 and abs(d[0, 2] - c) <= np.spacing(F(1.0))
    assert d[0, 0] > F(0.9999999) and abs(d[0, 2]) < F(1e-7)
    # and +x into -z
    _, d, _ = ar.resolve(m, [0], [[0, 0, 0]], [[1, 0, 0]])
    assert abs(d[0, 2] + s) <= np.spacing(s) and abs(d[0, 0] - c) <= np.spacing(F(1.0))


def test_a_parent_chain_composes(oracle):
    rng = np.random.default_rng(123)
    pos, rot, scale = rng.uniform(-5, 5, (3, 3)), rng.uniform(-3, 3, (3, 3)), rng.uniform(0.5, 2, (3, 3))
    w, m, mn, mx = small_world(oracle, pos, rot, scale, np.array([-1, 0, 1], np.int32))
    local = [T.host_mat4_trs(pos[i], rot[i], scale[i]).astype(np.float64).reshape(4, 4).T for i in range(3)]
    chain = local[0] @ local[1] @ local[2]
    l, v = F([0.3, -1.2, 2.0]), F([0.5, 0.1, -2.0])
    o, d, ok = ar.resolve(m, [2], [l], [v])
    assert ok.all()
    assert np.allclose(o[0], (chain @ np.append(l.astype(np.float64), 1.0))[:3], rtol=1e-5, atol=1e-5)
    assert np.allclose(d[0], chain[:3, :3] @ v.astype(np.float64), rtol=1e-5, atol=1e-5)
    # the grandchild's frame is not its parent's
    o1, _, _ = ar.resolve(m, [1], [l], [v])
    assert not np.allclose(o[0], o1[0], atol=1e-3)


def test_the_miss_rules(oracle):
    w, m, mn, mx = small_world(oracle, [[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.zeros((3, 3)), [[1, 1, 1], [1e-4] * 3, [1, 1, 1]], np.full(3, -1, np.int32))
    bad = m.copy()
    bad[2, 12] = np.inf
    huge = m.copy()
    huge[2, 0] = F(1e19)                                      # v.x = 1e19 gives d.x = 1e38: finite, its square is not
    anchor = np.array([3, ar.ANCHOR_DEAD, 1, 1, 2, 2, 0], np.uint32)
    v = F([[1, 0, 0]] * 3 + [[9000, 0, 0]] + [[1, 0, 0]] + [[1e19, 0, 0]] + [[1, 0, 0]])
    q = (anchor, np.zeros((7, 3), F), v, np.full(7, 10.0, F), np.full(7, ALL, np.uint32))
    none = np.zeros(7, np.uint8)
    for mats, want in ((m, [0, 0, 0, 1, 1, 1, 1]), (bad, [0, 0, 0, 1, 0, 0, 1]), (huge, [0, 0, 0, 1, 1, 0, 1])):
        got = ar.cast(oracle, mn, mx, w.group, w.mask, mats, *q, skip_self=none)
        assert list(got["hit"]) == want
        miss = got[got["hit"] == 0]
        assert (miss["id"] == ar.NO_ID).all() and (miss["normal"] == F([0, 1, 0])).all() and (miss["distance"] == 0).all()


def test_the_gpu_suites_random_case_has_hits_and_misses_on_every_tick(oracle):
    from tests import test_gpu_anchored_rays as G
    w, q, skip = G.random_case()
    ow = worlds.oracle_world(oracle, w, camera=False)
    for tick in range(3):
        if tick:
            ow.nudge_roots_x(G.NUDGE)
        ow.transform_system()
        want = G.witness(oracle, w, ow, q, skip)
        assert want["hit"].sum() > 300 and (want["hit"] == 0).sum() > 100
    mn, mx = ow.world_aabbs()
    assert ((mx[:, 0] - mn[:, 0]) > 128.0).sum() >= 30      # the plates: wider than two sectors
    ow.close()
