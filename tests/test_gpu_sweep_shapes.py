"""Exact collider shapes for capsule sweeps (scTickSetSweepShapes, SC_TICK_SWEEP_SHAPES_EXACT) through the C ABI against the fp32 witness
(tests/sweep_shapes_ref.py: the header's spec in numpy over the oracle's world matrices and the witness boxes of tests/collider_ref.py).
The GPU's matrices and boxes equal the oracle's / the witness's as IEEE values, so hit, id and layer must be equal, distance, travel,
position and normal equal as bit patterns, misses included, and the report's words equal."""
import numpy as np
import pytest

from sc_gameengine_amd import capi
from sc_gameengine_amd.tick import WorldTick
from tests import collider_ref as cr, sweep_ref, sweep_shapes_ref as ss, worlds
from tests.sweep_shapes_cases import ALL, colliders, constructed_scene, sweeps_of, witness, world_case
from tests.test_gpu_shape_rays import same_world, small_world
from tests.test_gpu_sweeps import compare

pytestmark = pytest.mark.gpu
FLAGS = capi.XFORM | capi.BROADPHASE | capi.DENSE_AABBS
SWEEPS = FLAGS | capi.SWEEPS
F = np.float32
EXACT, AABB = capi.SWEEP_SHAPES_EXACT, capi.SWEEP_SHAPES_AABB


def start(oracle, w, col, mode=EXACT, **kw):
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    t = WorldTick.from_world(w, broadphase=True, **kw)
    if col is not None:
        col.upload(t)
    t.set_sweep_shapes(mode)
    return t, ow


def set_queries(t, q):
    t.set_sweep_queries(*q[:5], skip_id=q[5])


def expect(t, ow, w, col, q, mode=ss.EXACT):
    """the witness over the oracle's matrices and the witness boxes, which the GPU's must equal"""
    if col is not None:
        m, mn, mx = same_world(t, ow, w, col)
    else:
        m = ow.world_matrices()[:w.n]
        mn, mx = ow.world_aabbs()
        assert np.array_equal(t.world_matrices(), m)
    return witness(m, mn, mx, w.group, w.mask, col, q, mode=mode)


def check(t, ow, w, col, q):
    want, info = expect(t, ow, w, col, q)
    compare(t.sweep_hits(), want)
    assert t.sweep_shape_info() == info, (t.sweep_shape_info(), info)
    return want, info


# ---- 1. sweep counts on either side of a workgroup's four waves ------------------------------------------------------
def test_sweep_counts_either_side_of_a_workgroup(oracle):
    w, col, q = world_case(oracle, n=800, seed=401, k=130)
    t, ow = start(oracle, w, col)
    for k in (1, 3, 4, 5, 130):
        qk = tuple(None if x is None else x[:k] for x in q)
        set_queries(t, qk)
        t.run(SWEEPS)
        want, info = check(t, ow, w, col, qk)
        assert len(want) == k
    assert 30 < want["hit"].sum() < 125 and info["refined"] > 40 and info["kept_as_boxes"] > 10 and info["exhausted"] == 0
    t.close(); ow.close()


# ---- 2. a sector holding 1, 63, 64 and 65 records: the last lane and the overflow list; a candidate in the big list ----
@pytest.mark.parametrize("crowd", [1, 63, 64, 65])
def test_a_sector_up_to_and_beyond_its_bin(oracle, crowd):
    rng = np.random.default_rng(410 + crowd)
    n = crowd + 1
    pos = np.zeros((n, 3))
    pos[:crowd, 0], pos[:crowd, 2] = rng.uniform(6, 58, crowd), rng.uniform(6, 58, crowd)          # one sector, clear of its edges
    pos[crowd] = [-40, -6, -40]                                                  # a plate 160 m wide: only in the big list
    rot = np.zeros((n, 3)); rot[:, 1] = rng.uniform(-3, 3, n); rot[crowd] = [0.05, 0.5, 0.0]
    w = small_world(pos, rot)
    types = rng.choice([cr.BOX, cr.SPHERE, cr.CAPSULE], n); types[crowd] = cr.BOX
    he = rng.uniform(0.3, 1.5, (n, 3)); he[crowd] = [80, 0.5, 80]
    col = colliders(n, types, he=he, radius=rng.uniform(0.3, 1.2, n), hh=rng.uniform(0, 1.5, n))
    k = 60
    a = np.stack([rng.uniform(0, 64, k), rng.uniform(-1, 1, k), rng.uniform(0, 64, k)], axis=1)
    b = np.stack([rng.uniform(0, 64, k), rng.uniform(-1, 1, k), rng.uniform(0, 64, k)], axis=1)
    b[40:, 1] = -14.0                                                            # down onto the tilted plate
    a[50:] -= [60, 0, 60]; b[50:] -= [60, 0, 60]
    q = sweeps_of(a, b, rng.choice(F([0.3, 0.5]), k), rng.choice(F([0.0, 0.6]), k))
    t, ow = start(oracle, w, col)
    set_queries(t, q)
    for _ in range(2):                                                           # the learn tick, then remembered slots
        t.run(SWEEPS)
        want, info = check(t, ow, w, col, q)
    assert t.counts().big_boxes == 1 and (t.counts().bin_overflow > 0) == (crowd > 64)
    hit = want["hit"] == 1
    assert (want["id"][hit] == crowd).sum() >= 5 and info["exhausted"] == 0       # the plate answers, by its shape
    plain, _ = expect(t, ow, w, col, q, mode=ss.AABB)
    assert (plain["travel"][hit & (want["id"] == crowd)] < want["travel"][hit & (want["id"] == crowd)]).all()
    if crowd > 1:
        assert (want["id"][hit] < crowd).sum() >= 10
    t.close(); ow.close()


# ---- 3. each target type alone, then mixed, under sheared parents; two ticks with the roots moved in between ---------
def test_every_target_type_alone_and_mixed_on_two_ticks(oracle):
    w, mixed, q = world_case(oracle, n=900, seed=421, k=300)
    t, ow = start(oracle, w, mixed)
    set_queries(t, q)
    rng = np.random.default_rng(423)
    for types in (cr.BOX, cr.SPHERE, cr.CAPSULE, None):
        col = mixed
        if types is not None:                                                    # (a collider re-upload: the next tick answers by the new shapes)
            col = cr.Colliders(w.n)
            col.type[:], col.he[:], col.radius[:], col.hh[:] = types, mixed.he, mixed.radius, mixed.hh
        col.upload(t)
        for tick in range(2 if types is None else 1):
            if tick:
                ow.nudge_roots_x(0.7); t.nudge_roots_x(0.7)
                ow.transform_system()
            t.run(SWEEPS)
            want, info = check(t, ow, w, col, q)
            plain, _ = expect(t, ow, w, col, q, mode=ss.AABB)
            differ = (want["travel"].view(np.uint32) != plain["travel"].view(np.uint32)) | (want["id"] != plain["id"])
            assert info["refined"] > 100 and info["exhausted"] == 0 and differ.sum() > 60 and 60 < want["hit"].sum() < 290, (info, differ.sum())
    m = ow.world_matrices()[:w.n]
    c0, c1 = m[:, 0:3], m[:, 4:7]
    cosine = np.abs((c0 * c1).sum(axis=1)) / (np.linalg.norm(c0, axis=1) * np.linalg.norm(c1, axis=1) + 1e-30)
    assert (cosine[np.unique(want["id"][want["hit"] == 1])] > 0.05).sum() >= 5   # sheared frames among the winners
    assert info["kept_as_boxes"] > 20
    t.close(); ow.close()


# ---- 4. the constructed cases, a tie and skip_id ---------------------------------------------------------------------
def test_constructed_cases_a_tie_and_skip_id(oracle):
    pos, rot, scale, col5, q7 = constructed_scene()
    # 5 and 6: two equal spheres in one place -- a tie, which goes to the lower id
    pos = pos + [[60, 0, -60], [60, 0, -60]]
    rot = rot + [[0, 0, 0]] * 2
    scale = scale + [[1, 1, 1]] * 2
    col = colliders(7, list(col5.type) + [cr.SPHERE] * 2, he=list(col5.he) + [[1, 1, 1]] * 2, radius=list(col5.radius) + [0.8, 0.8],
                    hh=list(col5.hh) + [0.5, 0.5])
    a = np.concatenate([q7[0], F([[50, 0.2, -60], [50, 0.2, -60], [50, 0.2, -60]])])
    b = np.concatenate([q7[1], F([[60, 0, -60], [60, 0, -60], [60, 0, -60]])])
    skip = np.full(10, ALL, np.uint32); skip[8] = 5; skip[9] = 6
    q = sweeps_of(a, b, 0.4, 0.5, skip=skip)
    w = small_world(pos, rot, scale)
    t, ow = start(oracle, w, col)
    set_queries(t, q)
    t.run(SWEEPS)
    got = t.sweep_hits()
    want, info = check(t, ow, w, col, q)
    plain, _ = expect(t, ow, w, col, q, mode=ss.AABB)
    tol = float(ss.TOL)
    assert list(got["hit"]) == [1, 1, 0, 0, 1, 0, 1, 1, 1, 1] and list(got["id"][[0, 1, 4, 6, 7, 8, 9]]) == [0, 1, 4, 1, 5, 6, 5]
    assert 6.6 - tol - 1e-5 <= got["travel"][0] <= 6.6 + 1e-5 and np.allclose(got["normal"][0], [-1, 0, 0], atol=1e-5)
    assert abs(float(got["travel"][1]) - 10.6) <= tol and abs(float(got["travel"][1]) - float(plain["travel"][1])) <= tol
    assert plain["hit"][2] == 1 and plain["id"][2] == 2 and plain["hit"][5] == 1           # the bounding square stops what the prop lets pass
    for s in (4, 6):
        assert got["travel"][s] == 0 and np.array_equal(got["normal"][s], F([0, 1, 0]))
    assert got["travel"][7].view(np.uint32) == got["travel"][8].view(np.uint32) == got["travel"][9].view(np.uint32)
    assert info["refined"] == 6 + 2 * 3 - 2 and info["kept_as_boxes"] == 0 and info["exhausted"] == 0
    t.close(); ow.close()


# ---- 5. mode changes, with and without graph replay ------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_mode_changes_return_to_the_first_bits_and_cost_no_learn_tick(oracle, graph):
    w, col, q = world_case(oracle, n=700, seed=431, k=200)
    t, ow = start(oracle, w, col, mode=AABB)
    never = WorldTick.from_world(w, broadphase=True)                             # a context that never sets the mode
    col.upload(never)
    assert t.sweep_shapes() == AABB == never.sweep_shapes()
    for x in (t, never):
        set_queries(x, q)
    if graph:
        t.set_graph_mode(True)
    for _ in range(3):                                                           # the learn tick, the capture, a replay
        t.run(SWEEPS)
    never.run(SWEEPS)
    first = t.sweep_hits()
    m, mn, mx = same_world(t, ow, w, col)
    assert first.tobytes() == never.sweep_hits().tobytes()
    compare(first, sweep_ref.sweep_boxes(oracle, mn, mx, w.group, w.mask, *q[:5]))
    with pytest.raises(capi.ScTickError, match="SC_TICK_SWEEP_SHAPES_AABB mode"):
        t.sweep_shape_info()
    want = {AABB: expect(t, ow, w, col, q, mode=ss.AABB), EXACT: expect(t, ow, w, col, q)}
    assert want[AABB][0].tobytes() == first.tobytes()
    assert (want[AABB][0]["travel"].view(np.uint32) != want[EXACT][0]["travel"].view(np.uint32)).sum() > 40
    learn = t.learn_ticks()
    for mode in (EXACT, AABB, EXACT, EXACT, AABB):
        t.set_sweep_shapes(mode)
        assert t.sweep_shapes() == mode
        for _ in range(3):                                                       # (graph mode: a capture and two replays -- the report replays too)
            t.run(SWEEPS)
            compare(t.sweep_hits(), want[mode][0])
            if mode == EXACT:
                assert t.sweep_shape_info() == want[EXACT][1]
    assert t.sweep_hits().tobytes() == first.tobytes() and t.learn_ticks() == learn
    t.close(); never.close(); ow.close()


# ---- 6. residency ----------------------------------------------------------------------------------------------------
def test_colliders_travel_with_relocated_entities(oracle):
    w = worlds.random_world(900, seed=441, spread=50.0, p_child=0.0)
    rng = np.random.default_rng(442)
    col = cr.Colliders.random(w.n, rng)
    k = 300
    a = rng.uniform(-50, 50, (k, 3)); a[:, 1] = rng.uniform(-2, 2, k)
    d = rng.normal(size=(k, 3)); d[:, 1] *= 0.2
    q = sweeps_of(a, a + d * rng.uniform(3, 12, (k, 1)), rng.choice(F([0.3, 0.6]), k), rng.choice(F([0.0, 0.7]), k))
    gone = rng.choice(np.arange(100, 700), 60, replace=False).astype(np.uint32)
    t, ow = start(oracle, w, col)
    set_queries(t, q)
    t.run(SWEEPS)
    check(t, ow, w, col, q)
    before = ow.dense_entities()
    for e in before[gone]:
        assert ow.destroy(int(e))
    src, dst = t.remove_entities(gone)
    n1 = w.n - len(gone)
    now = cr.Colliders(n1)
    group, mask = w.group[:n1].copy(), w.mask[:n1].copy()
    for x, y in ((now.type, col.type), (now.he, col.he), (now.radius, col.radius), (now.hh, col.hh), (group, w.group), (mask, w.mask)):
        x[:] = y[:n1]
        x[dst] = y[src]
    ow.transform_system()
    t.run(SWEEPS)
    m = ow.world_matrices()[:n1]
    mn, mx = now.witness(ow, n1)
    assert np.array_equal(t.world_matrices(), m)
    want, info = witness(m, mn, mx, group, mask, now, q)
    compare(t.sweep_hits(), want)
    assert t.sweep_shape_info() == info
    hit = want["hit"] == 1
    assert hit.sum() > 40 and np.isin(want["id"][hit], dst).sum() >= 2 and len(src) > 20
    t.close(); ow.close()


# ---- 7. tiles ----------------------------------------------------------------------------------------------------------
def test_a_neighbours_sphere_keeps_its_box_answer_and_a_pipelined_tile_refuses(oracle):
    """2 x 1 tiles on one GPU, the caller-owned split flow (the arrangement of the exact rays' tile test).  Four spheres of tile 1 lie on
    the shared edge and reach 0.2 m into tile 0, which knows them from the border merge alone: its sweeps answer at their grown AABBs.
    Four spheres of tile 0 stand 4 m before the edge; a sweep that meets one of them first answers at the sphere itself."""
    import torch
    from sc_gameengine_amd import synth_world as sw, tiles
    from tests.test_gpu_tiles import split_world
    from tests.test_gpu_tiles_edge import network
    grid, S = (2, 1), (6, 6)
    w = sw.generate(S[0] * grid[0], S[1], 15, tiles=grid)
    w.group[:], w.mask[:] = sw.GROUP_DYNAMIC, sw.MASK_ALL
    n = w.n // 2
    edge = 64.0 * S[0]
    props = (w.parent < 0) & (np.arange(w.n) % 16 != 0)
    lone = props & ~np.isin(np.arange(w.n), w.parent[w.parent >= 0])
    zs = F([40.0, 110.0, 200.0, 300.0])
    near = np.flatnonzero(lone & (np.arange(w.n) >= n))[:4]
    w.pos[near] = np.stack([np.full(4, edge + 0.3, F), np.full(4, 200.0, F), zs], axis=1)
    own = np.flatnonzero(lone & (np.arange(w.n) < n))[:4]
    w.pos[own] = np.stack([np.full(4, edge - 4.0, F), np.full(4, 200.0, F), zs], axis=1)
    for e in (near, own):
        w.scale[e] = 1.0; w.rot[e] = 0.0
    col = cr.Colliders(w.n)
    col.type[near] = cr.SPHERE; col.type[own] = cr.SPHERE
    col.radius[near] = 0.5; col.radius[own] = 0.5
    # sweeps along +x, 0.3 m beside the centres: 0..3 start behind tile 0's spheres, 4..7 between them and the edge
    a = np.concatenate([np.stack([np.full(4, edge - 8.0, F), np.full(4, 200.0, F), zs + F(0.3)], axis=1),
                        np.stack([np.full(4, edge - 2.0, F), np.full(4, 200.0, F), zs + F(0.3)], axis=1)]).astype(F)
    b = a + F([1.9, 0, 0]); b[:4] = a[:4] + F([5.0, 0, 0])
    q = sweeps_of(a, b, 0.2, 0.0)
    parts, n = split_world(w, grid, S)
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    m = ow.world_matrices()[:w.n]
    mn, mx = col.witness(ow, w.n)
    flags = capi.XFORM | capi.BROADPHASE | capi.SPLIT_PAIRS | capi.DENSE_AABBS | capi.SWEEPS
    ticks = [WorldTick.from_world(p, broadphase=True, max_pairs=1 << 16) for p in parts]
    for r, t in enumerate(ticks):
        t.upload_colliders(0, col.type[r * n:(r + 1) * n], col.he[r * n:(r + 1) * n], col.radius[r * n:(r + 1) * n], col.hh[r * n:(r + 1) * n])
        t.set_sweep_shapes(EXACT)
    bufs = [tiles.BorderBuffers(t, r, grid, "cuda") for r, t in enumerate(ticks)]
    set_queries(ticks[0], q)
    for t in ticks:
        t.run(flags)
    with pytest.raises(capi.ScTickError, match="scTickRunPairs is pending"):
        ticks[0].set_sweep_shapes(AABB)
    with pytest.raises(capi.ScTickError, match="after scTickRunPairs"):
        ticks[0].sweep_shape_info()
    network(bufs, grid, parity=0)
    for t in ticks:
        t.run_pairs()
    got = ticks[0].sweep_hits()
    assert np.array_equal(np.concatenate([t.world_matrices() for t in ticks]), m)
    want, info = witness(m, mn, mx, w.group, w.mask, col, q, own=np.arange(w.n) < n)
    assert list(want["hit"]) == [1] * 8
    assert np.array_equal(want["id"][:4], own.astype(np.uint32)) and np.array_equal(want["id"][4:], near.astype(np.uint32))
    assert np.array_equal(tiles.global_pair_ids(got["id"].reshape(-1, 1), n).ravel(), want["id"].astype(np.uint64))
    assert ((got["id"][4:] >> 24) == 1).all() and (got["pad"] == 0).all()
    for f in ("hit", "layer"):
        assert np.array_equal(got[f], want[f])
    for f in ("distance", "travel", "position", "normal"):
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f
    assert ticks[0].sweep_shape_info() == info and info["refined"] == 4 and info["kept_as_boxes"] == 4
    # the own spheres answer where the capsule touches them (4 - sqrt(0.49 - 0.09) = 3.3675, less at most TOL over the slope), the
    # neighbour's at their grown AABB's face (2.3 - 0.5 - 0.2 = 1.6)
    assert ((got["travel"][:4] > 3.36) & (got["travel"][:4] <= 3.3676)).all() and np.allclose(got["travel"][4:], 1.6, atol=1e-4)
    assert (got["normal"][4:] == F([-1, 0, 0])).all() and (got["normal"][:4, 2] > 0.3).all()
    # a pipelined context refuses the run
    stream = torch.cuda.Stream()
    ticks[1].set_pairs_stream(stream.cuda_stream)
    set_queries(ticks[1], q)
    assert ticks[1].lib.scTickRun(ticks[1].ctx, flags) == 0
    assert b"SC_TICK_SWEEP_SHAPES_EXACT cannot run on a pipelined context" in ticks[1].lib.scTickGetLastError(ticks[1].ctx)
    for t in ticks:
        t.close()
    ow.close()


# ---- 8. the caller-owned gap of a split tick -------------------------------------------------------------------------
def test_the_gap_of_an_exact_split_tick_refuses_what_would_change_its_shapes(oracle):
    w, col, q = world_case(oracle, n=700, seed=451, k=200)
    t, ow = start(oracle, w, col)
    set_queries(t, q)
    split = SWEEPS | capi.SPLIT_PAIRS
    t.run(split)
    m = ow.world_matrices()[:w.n]
    rng = np.random.default_rng(452)
    scrambled = m[rng.permutation(w.n)].copy()
    other = cr.Colliders.random(w.n, rng)
    refused = "is refused between scTickRun"
    with pytest.raises(capi.ScTickError, match="scTickUploadWorldMatrices " + refused):
        t.upload_world_matrices(0, scrambled)
    with pytest.raises(capi.ScTickError, match="scTickUploadColliders " + refused):
        other.upload(t)
    with pytest.raises(capi.ScTickError, match="scTickRemoveEntities " + refused):
        t.remove_entities(np.arange(10, 40, dtype=np.uint32))
    assert t.lib.scTickSetEntityCount(t.ctx, w.n - 100) == 0 and b"scTickSetEntityCount is refused" in t.lib.scTickGetLastError(t.ctx)
    assert b"sweeps capsules in SC_TICK_SWEEP_SHAPES_EXACT mode" in t.lib.scTickGetLastError(t.ctx)
    with pytest.raises(capi.ScTickError, match="scTickRun with SC_TICK_XFORM " + refused):
        t.run(capi.XFORM)
    t.nudge_roots_x(5.0)                                                        # locals are the next tick's: welcome
    t.run_pairs()
    want, info = check(t, ow, w, col, q)                                        # tick t's shapes, untouched
    assert info["refined"] > 50
    # AABB mode: the host owns the gap
    t.upload_world_matrices(0, m)
    t.set_sweep_shapes(AABB)
    ow.nudge_roots_x(5.0); ow.transform_system()
    t.run(split)
    same_world(t, ow, w, col)
    t.upload_world_matrices(0, scrambled)
    t.run_pairs()
    compare(t.sweep_hits(), witness(ow.world_matrices()[:w.n], *col.witness(ow, w.n), w.group, w.mask, col, q, mode=ss.AABB)[0])
    t.close(); ow.close()


# ---- 9. errors -------------------------------------------------------------------------------------------------------
def test_sweep_shape_api_errors(oracle):
    w, col, q = world_case(oracle, n=300, seed=461, k=100)
    t = WorldTick.from_world(w, broadphase=True)
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    assert t.sweep_shapes() == AABB
    for bad in (2, 7, ALL):
        with pytest.raises(capi.ScTickError, match="unknown sweep shape mode"):
            t.set_sweep_shapes(bad)
    assert t.sweep_shapes() == AABB
    assert t.lib.scTickGetSweepShapes(t.ctx, None) == 0 and b"null argument" in t.lib.scTickGetLastError(t.ctx)
    assert t.lib.scTickGetSweepShapeInfo(t.ctx, None) == 0 and b"null argument" in t.lib.scTickGetLastError(t.ctx)
    t.set_sweep_shapes(EXACT)
    t.run(FLAGS)
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_SWEEPS"):
        t.sweep_shape_info()
    t.run(SWEEPS)                                                                # an empty batch reports zeros
    assert t.sweep_shape_info() == dict(refined=0, kept_as_boxes=0, exhausted=0) and len(t.sweep_hits()) == 0
    t.run(FLAGS | capi.SPLIT_PAIRS)
    with pytest.raises(capi.ScTickError, match="scTickRunPairs is pending"):
        t.set_sweep_shapes(AABB)
    assert t.sweep_shapes() == EXACT
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_SWEEPS"):      # the missing flag is named before the pending half
        t.sweep_shape_info()
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_SWEEPS"):
        t.sweep_hits()
    t.run_pairs()
    t.run(SWEEPS | capi.SPLIT_PAIRS)
    with pytest.raises(capi.ScTickError, match="the sweep shape report is ready after scTickRunPairs"):
        t.sweep_shape_info()
    with pytest.raises(capi.ScTickError, match="sweep hits are ready after scTickRunPairs"):
        t.sweep_hits()
    t.run_pairs()
    t.set_sweep_shapes(AABB)
    t.run(SWEEPS | capi.SPLIT_PAIRS)
    with pytest.raises(capi.ScTickError, match="SC_TICK_SWEEP_SHAPES_AABB mode: nothing was refined"):      # ... and so is the mode of that run
        t.sweep_shape_info()
    t.run_pairs()
    t.set_sweep_shapes(EXACT)
    # EXACT mode on a context without colliders: nothing is refined, the answers are the AABB mode's
    set_queries(t, q)
    t.run(SWEEPS)
    want, info = check(t, ow, w, None, q)
    assert info["refined"] == 0 and info["kept_as_boxes"] > 30 and 10 < want["hit"].sum() < 100
    t.set_sweep_shapes(AABB)
    t.run(SWEEPS)
    assert t.sweep_hits().tobytes() == want.tobytes()
    t.close(); ow.close()
