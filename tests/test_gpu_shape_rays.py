"""Exact collider shapes for rays (scTickSetRayShapes, SC_TICK_RAY_SHAPES_EXACT) through the C ABI against the witness
(tests/shape_rays_ref.py: the header's spec in numpy fp32 over the oracle's world matrices and the witness boxes of
tests/collider_ref.py).  The GPU's matrices and boxes equal the oracle's / the witness's as IEEE values, so hit, id and layer must be
equal and distance, position and normal equal as bit patterns, misses included; the pad words are 0."""
import numpy as np
import pytest

from sc_gameengine_amd import capi, synth_world as sw
from sc_gameengine_amd.tick import WorldTick
from tests import anchored_ref as ar, collider_ref as cr, shape_rays_ref as sr, worlds
from tests.shape_rays_cases import NUDGE, identity_box_rays, random_case, rays_of, winner_counts, witness

pytestmark = pytest.mark.gpu
FLAGS = capi.XFORM | capi.BROADPHASE | capi.DENSE_AABBS
RAYS = FLAGS | capi.RAYS
F = np.float32
ALL = 0xFFFFFFFF
EXACT, AABB = capi.RAY_SHAPES_EXACT, capi.RAY_SHAPES_AABB


def compare(got, want):
    assert len(got) == len(want)
    for f in ("hit", "id", "layer"):
        assert np.array_equal(got[f], want[f]), f"{f}: {np.flatnonzero(got[f] != want[f])[:8]}"
    for f in ("distance", "position", "normal"):
        bad = np.flatnonzero((got[f].view(np.uint32) != want[f].view(np.uint32)).reshape(len(got), -1).any(axis=1))
        assert not len(bad), f"{f}: rays {bad[:8]} got {got[f][bad[:3]]} want {want[f][bad[:3]]}"
    assert (got["pad"] == 0).all()


def same_world(t, ow, w, col):
    """The GPU's matrices equal the oracle's and its boxes the collider witness's; returns (matrices, mn, mx)."""
    m = ow.world_matrices()[:w.n]
    mn, mx = col.witness(ow, w.n)
    assert np.array_equal(t.world_matrices(), m), "world matrices differ from the oracle"
    gmn, gmx = t.world_aabbs()
    assert np.array_equal(gmn, mn) and np.array_equal(gmx, mx), "world AABBs differ from the witness"
    return m, mn, mx


def small_world(pos, rot=None, scale=None):
    """Roots with unit Bounds, group 1, mask all, in a 4 x 4 sector rectangle around the origin."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3)
    n = len(pos)
    return sw.SynthWorld(pos=pos.copy(), rot=np.zeros((n, 3), F) if rot is None else np.ascontiguousarray(rot, F).reshape(n, 3),
                         scale=np.ones((n, 3), F) if scale is None else np.ascontiguousarray(scale, F).reshape(n, 3),
                         parent=np.full(n, -1, np.int32), bmin=np.full((n, 3), -0.5, F), bmax=np.full((n, 3), 0.5, F),
                         has_mesh=np.ones(n, np.uint8), has_bounds=np.ones(n, np.uint8), mesh=np.zeros(n, np.uint32),
                         material=np.zeros(n, np.uint32), group=np.ones(n, np.uint32), mask=np.full(n, ALL, np.uint32),
                         sector_of=np.zeros((n, 2), np.int32), origin=(-2, -2), sectors=(4, 4))


def colliders(n, types, he=None, radius=None, hh=None):
    col = cr.Colliders(n)
    col.type[:] = types
    if he is not None:
        col.he[:] = F(he)
    if radius is not None:
        col.radius[:] = F(radius)
    if hh is not None:
        col.hh[:] = F(hh)
    return col


def start(oracle, w, col, mode=EXACT, **kw):
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    t = WorldTick.from_world(w, broadphase=True, **kw)
    col.upload(t)
    t.set_ray_shapes(mode)
    return t, ow


# ---- 1. an identity box is its own AABB -----------------------------------------------------------------------------
def test_an_identity_box_at_the_origin_answers_with_the_aabb_modes_bits(oracle):
    he, q = identity_box_rays()
    w = small_world([[0, 0, 0]])
    col = colliders(1, cr.BOX, he=[he])
    t, ow = start(oracle, w, col, mode=AABB)
    t.set_ray_queries(*q)
    t.run(RAYS)
    _, mn, mx = same_world(t, ow, w, col)
    assert np.array_equal(mn[0], -he) and np.array_equal(mx[0], he)
    plain = t.ray_hits()
    compare(plain, oracle.raycast_boxes(mn, mx, w.group, w.mask, *q))
    t.set_ray_shapes(EXACT)
    assert t.ray_shapes() == EXACT
    t.run(RAYS)
    exact = t.ray_hits()
    assert exact.tobytes() == plain.tobytes()
    compare(exact, witness(ow, w, col, q))
    hit = plain["hit"] == 1
    assert hit[:600].sum() > 200 and (~hit[:600]).sum() > 50 and hit[750:850].all() and not hit[850:].any()
    assert (plain["distance"][750:850] == 0).all() and hit[600:750].sum() > 5
    t.close(); ow.close()


# ---- 2. a random world (tests/shape_rays_cases.py) ------------------------------------------------------------------
def test_random_world_against_the_witness_on_two_ticks(oracle):
    w, col, q = random_case(oracle)
    t, ow = start(oracle, w, col)
    t.set_ray_queries(*q)
    for tick in range(2):
        if tick:
            ow.nudge_roots_x(NUDGE); t.nudge_roots_x(NUDGE)
            ow.transform_system()
        t.run(RAYS)
        same_world(t, ow, w, col)
        want = witness(ow, w, col, q)
        compare(t.ray_hits(), want)
        counts, differ = winner_counts(want, witness(ow, w, col, q, mode=sr.AABB), col)
        assert all(counts[k] >= 100 for k in counts) and differ >= 200, (counts, differ)
    assert t.counts().big_boxes >= 20
    t.close(); ow.close()


# ---- 3. constructed cases, answers in closed form -------------------------------------------------------------------
def test_constructed_cases_with_answers_in_closed_form(oracle):
    # 0: a 4.4 m x 2 m vehicle box yawed by 45 degrees at the origin; 1: a small box in the lane beside it, inside the first one's AABB;
    # 2: a sphere of radius 1.5 under scale 2; 3: an upright capsule, radius 1, half height 2
    pos = [[0, 0, 0], [2, 0, -1], [10, 0, 40], [0, 0, 80]]
    rot = [[0, np.pi / 4, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    scale = [[1, 1, 1], [1, 1, 1], [2, 2, 2], [1, 1, 1]]
    w = small_world(pos, rot, scale)
    col = colliders(4, [cr.BOX, cr.BOX, cr.SPHERE, cr.CAPSULE], he=[[1.0, 0.75, 2.2], [0.25, 0.25, 0.25], [1, 1, 1], [1, 1, 1]],
                    radius=[0.5, 0.5, 1.5, 1.0], hh=[0.5, 0.5, 0.5, 2.0])
    o = [[2, 0, -4],                  # down the neighbouring lane, through the corner of box 0's AABB, ending before box 0 itself
         [0, 0, 40],                  # along +x through the sphere's centre: distance 10, R = 3
         [0, 0.5, 60],                # the capsule's side, along +z
         [0, 10, 80],                 # down the capsule's axis: the parallel branch (ka = 0), the upper cap
         [0, -10, 80],                # up its axis: the lower cap
         [0, 2.5, 60]]                # a cap from the side: 0.5 above the seam, 20 m away
    d = [[0, 0, 1], [1, 0, 0], [0, 0, 1], [0, -1, 0], [0, 3, 0], [0, 0, 1]]
    q = rays_of(o, d, [4.0, 100, 100, 100, 100, 100])
    t, ow = start(oracle, w, col, mode=AABB)
    t.set_ray_queries(*q)
    t.run(RAYS)
    _, mn, mx = same_world(t, ow, w, col)
    plain = t.ray_hits()
    compare(plain, witness(ow, w, col, q, mode=sr.AABB))
    assert plain["id"][0] == 0 and 1.7 < plain["distance"][0] < 1.8             # the yawed box's AABB is about 4.5 m wide
    assert mx[0, 0] > 2.26 and plain["distance"][1] == 7.0                      # (the bounding cube's face happens to be the pole)
    t.set_ray_shapes(EXACT)
    t.run(RAYS)
    got = t.ray_hits()
    compare(got, witness(ow, w, col, q))
    assert list(got["hit"]) == [1] * 6 and list(got["id"]) == [1, 2, 3, 3, 3, 3]
    assert np.array_equal(got["distance"][:5], F([2.75, 7.0, 19.0, 7.0, 7.0]))
    assert np.array_equal(got["position"][:5], F([[2, 0, -1.25], [7, 0, 40], [0, 0.5, 79], [0, 3, 80], [0, -3, 80]]))
    assert np.array_equal(got["normal"][:5], F([[0, 0, -1], [-1, 0, 0], [0, 0, -1], [0, 1, 0], [0, -1, 0]]))
    # the cap from the side: sqrt(1 - 0.25) short of the axis, fp32 to an ulp or two
    assert abs(float(got["distance"][5]) - (20.0 - np.sqrt(0.75))) < 4e-6 and plain["distance"][5] == 19.0
    t.close(); ow.close()


# ---- 4. degenerate inputs -------------------------------------------------------------------------------------------
def test_degenerate_matrices_and_a_zero_radius(oracle):
    # 0: a box with a zero-scale column; 1: a capsule with a zero-scale y column; 2: a sphere and 3: a capsule of radius 0
    pos = [[0, 0, 0], [20, 0, 0], [40, 0, 0], [60, 0, 0]]
    scale = [[0, 1, 1], [1.5, 0, 1], [1, 1, 1], [1, 1, 1]]
    rot = [[0.3, 0.5, 0.1], [0, 0, 0.4], [0, 0, 0], [0.2, 0, 0.3]]
    w = small_world(pos, rot, scale)
    col = colliders(4, [cr.BOX, cr.CAPSULE, cr.SPHERE, cr.CAPSULE], he=[[1, 1, 1]] * 4, radius=[0.5, 1.0, 0.0, 0.0], hh=[0.5, 2.0, 0.5, 1.5])
    rng = np.random.default_rng(241)
    k = 400
    target = rng.integers(0, 4, k)
    o = (F(pos)[target] + rng.normal(size=(k, 3)) * 4).astype(F)
    d = ((F(pos)[target] + rng.normal(size=(k, 3)) * 0.7) - o).astype(F)
    o[300:340] = F(pos)[target[300:340]]; d[300:340] = rng.normal(size=(40, 3))          # from the centre outwards
    d[340:] = F(pos)[target[340:]] - o[340:]                                    # straight at the centre: the zero radius is met exactly there or not at all
    q = rays_of(o, d, np.full(k, 30.0, F))
    t, ow = start(oracle, w, col)
    t.set_ray_queries(*q)
    t.run(RAYS)
    same_world(t, ow, w, col)
    got, want, plain = t.ray_hits(), witness(ow, w, col, q), witness(ow, w, col, q, mode=sr.AABB)
    assert not np.isnan(want["normal"]).any()                                   # (a NaN's sign and payload are nobody's spec)
    compare(got, want)
    on_box = (plain["hit"] == 1) & (plain["id"] == 0)
    assert on_box.sum() > 30 and got[on_box].tobytes() == plain[on_box].tobytes()         # the AABB answer stands
    # the flattened capsule is the sphere of its own R: the same entity as a SPHERE gives the same bits
    col2 = colliders(4, [cr.BOX, cr.SPHERE, cr.SPHERE, cr.CAPSULE], he=[[1, 1, 1]] * 4, radius=[0.5, 1.0, 0.0, 0.0], hh=[0.5, 2.0, 0.5, 1.5])
    m = ow.world_matrices()[:4]
    assert m[1, 4] == 0 and m[1, 5] == 0 and m[1, 6] == 0
    as_sphere = sr.cast(m, *col.witness(ow, 4), w.group, w.mask, col2, *q)
    assert as_sphere.tobytes() == want.tobytes() and ((want["hit"] == 1) & (want["id"] == 1)).sum() > 30
    assert ((want["id"] == 2) | (want["id"] == 3)).sum() > 5
    t.close(); ow.close()


# ---- 5. anchored rays -----------------------------------------------------------------------------------------------
def test_anchored_rays_in_exact_mode(oracle):
    w = worlds.random_world(1500, seed=251, spread=60.0, max_depth=2)
    rng = np.random.default_rng(252)
    col = cr.Colliders.random(w.n, rng)
    k = 600
    anchor = rng.integers(0, w.n, k).astype(np.uint32)
    anchor[:100] = capi.ANCHOR_NONE
    anchor[100:110] = capi.ANCHOR_DEAD
    l = rng.uniform(-4, 4, (k, 3)).astype(F)
    l[110:250] = rng.uniform(-0.05, 0.05, (140, 3))                             # inside the anchor's own collider
    v = (rng.normal(size=(k, 3)) * rng.uniform(0.01, 30, (k, 1))).astype(F)
    l[:100] = rng.uniform(-60, 60, (100, 3)); v[:100] = rng.normal(size=(100, 3))
    md = rng.uniform(2, 80, k).astype(F)
    mask = rng.choice(np.array([1, 3, ALL], np.uint32), k)
    skip = (rng.random(k) < 0.5).astype(np.uint8)
    t, ow = start(oracle, w, col)
    t.set_anchored_rays(anchor, l, v, md, mask, skip_self=skip)
    t.set_ray_queries(l[:100], v[:100], md[:100], mask[:100])
    for tick in range(2):
        if tick:
            ow.nudge_roots_x(0.6); t.nudge_roots_x(0.6)
            ow.transform_system()
        t.run(RAYS | capi.ANCHORED_RAYS)
        m, mn, mx = same_world(t, ow, w, col)
        o, d, ok = ar.resolve(m, anchor, l, v)
        own = np.where((skip != 0) & (anchor < w.n), anchor.astype(np.int64), -1)
        want = sr.cast(m, mn, mx, w.group, w.mask, col, o, np.where(ok[:, None], d, 0).astype(F), md, mask, skip=own)
        got = t.anchored_ray_hits()
        compare(got, want)
        assert got[:100].tobytes() == t.ray_hits().tobytes()                    # no anchor: the plain EXACT ray, bit for bit
        assert not got["hit"][100:110].any()
        hit = got["hit"] == 1
        assert hit.sum() > 150 and (~hit).sum() > 100
        sk = hit & (skip != 0) & (anchor < w.n)
        assert (got["id"][sk] != anchor[sk]).all() and sk.sum() > 30
        plain = sr.cast(m, mn, mx, w.group, w.mask, col, o, np.where(ok[:, None], d, 0).astype(F), md, mask, skip=own, mode=sr.AABB)
        assert (plain["distance"].view(np.uint32) != want["distance"].view(np.uint32)).sum() > 50
    t.close(); ow.close()


# ---- 6. mode changes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_mode_changes_return_to_the_first_bits_and_cost_no_learn_tick(oracle, graph):
    w = worlds.random_world(1200, seed=261, spread=60.0, max_depth=2)
    rng = np.random.default_rng(262)
    col = cr.Colliders.random(w.n, rng)
    k = 500
    o = rng.uniform(-60, 60, (k, 3)).astype(F)
    q = rays_of(o, rng.normal(size=(k, 3)), rng.uniform(5, 80, k))
    t, ow = start(oracle, w, col, mode=AABB)
    assert t.ray_shapes() == AABB
    t.set_ray_queries(*q)
    if graph:
        t.set_graph_mode(True)
    want = {AABB: witness(ow, w, col, q, mode=sr.AABB), EXACT: witness(ow, w, col, q)}
    assert (want[AABB]["distance"].view(np.uint32) != want[EXACT]["distance"].view(np.uint32)).sum() > 50
    for _ in range(3):                                                          # the learn tick, the capture, a replay
        t.run(RAYS)
    first = t.ray_hits()
    compare(first, want[AABB])
    learn = t.learn_ticks()
    for mode in (EXACT, AABB, EXACT, EXACT, AABB):
        t.set_ray_shapes(mode)
        assert t.ray_shapes() == mode
        for _ in range(3):                                                      # (graph mode: a capture and two replays)
            t.run(RAYS)
            compare(t.ray_hits(), want[mode])
    assert t.ray_hits().tobytes() == first.tobytes()
    assert t.learn_ticks() == learn
    t.close(); ow.close()


# ---- 7. residency ---------------------------------------------------------------------------------------------------
def test_colliders_travel_with_relocated_entities(oracle):
    w = worlds.random_world(900, seed=271, spread=50.0, p_child=0.0)
    rng = np.random.default_rng(272)
    col = cr.Colliders.random(w.n, rng)
    k = 500
    q = rays_of(rng.uniform(-50, 50, (k, 3)), rng.normal(size=(k, 3)), rng.uniform(5, 80, k))
    gone = rng.choice(np.arange(100, 700), 60, replace=False).astype(np.uint32)
    t, ow = start(oracle, w, col)
    t.set_ray_queries(*q)
    t.run(RAYS)
    same_world(t, ow, w, col)
    compare(t.ray_hits(), witness(ow, w, col, q))
    before = ow.dense_entities()
    for e in before[gone]:
        assert ow.destroy(int(e))
    src, dst = t.remove_entities(gone)
    assert len(src) > 20
    n1 = w.n - len(gone)
    now = cr.Colliders(n1)
    group, mask = w.group[:n1].copy(), w.mask[:n1].copy()
    for a, b in ((now.type, col.type), (now.he, col.he), (now.radius, col.radius), (now.hh, col.hh), (group, w.group), (mask, w.mask)):
        a[:] = b[:n1]
        a[dst] = b[src]
    ow.transform_system()
    t.run(RAYS)
    m = ow.world_matrices()[:n1]
    mn, mx = now.witness(ow, n1)
    assert np.array_equal(t.world_matrices(), m)
    gmn, gmx = t.world_aabbs()
    assert np.array_equal(gmn, mn) and np.array_equal(gmx, mx)
    want = sr.cast(m, mn, mx, group, mask, now, *q)
    compare(t.ray_hits(), want)
    hit = want["hit"] == 1
    assert hit.sum() > 50 and np.isin(want["id"][hit], dst).sum() > 3            # relocated entities answer, with their own shapes
    assert (now.type[dst] != col.type[dst]).sum() > 5
    t.close(); ow.close()


# ---- 8. tiles -------------------------------------------------------------------------------------------------------
def test_a_neighbours_record_keeps_its_aabb_answer_and_a_pipelined_tile_refuses(oracle):
    """2 x 1 tiles on one GPU, the caller-owned split flow.  Four spheres of tile 1 lie on the shared edge and reach 0.2 m into tile 0,
    which knows them from the border merge alone: its rays answer at their AABB faces.  Four spheres of tile 0 stand 4 m before the
    edge; a ray that meets one of them first answers at the sphere itself."""
    import torch
    from sc_gameengine_amd import tiles
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
    # rays along +x, 0.3 m beside the centres: rays 0..3 start behind tile 0's spheres, rays 4..7 between them and the edge
    o = np.concatenate([np.stack([np.full(4, edge - 8.0, F), np.full(4, 200.0, F), zs + F(0.3)], axis=1),
                        np.stack([np.full(4, edge - 2.0, F), np.full(4, 200.0, F), zs + F(0.3)], axis=1)]).astype(F)
    q = rays_of(o, np.tile(F([1, 0, 0]), (8, 1)), np.full(8, 20.0, F))
    parts, n = split_world(w, grid, S)
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    m = ow.world_matrices()[:w.n]
    mn, mx = col.witness(ow, w.n)
    flags = capi.XFORM | capi.BROADPHASE | capi.SPLIT_PAIRS | capi.DENSE_AABBS | capi.RAYS
    ticks = [WorldTick.from_world(p, broadphase=True, max_pairs=1 << 16) for p in parts]
    for r, t in enumerate(ticks):
        t.upload_colliders(0, col.type[r * n:(r + 1) * n], col.he[r * n:(r + 1) * n], col.radius[r * n:(r + 1) * n], col.hh[r * n:(r + 1) * n])
        t.set_ray_shapes(EXACT)
    bufs = [tiles.BorderBuffers(t, r, grid, "cuda") for r, t in enumerate(ticks)]
    ticks[0].set_ray_queries(*q)
    for t in ticks:
        t.run(flags)
    with pytest.raises(capi.ScTickError, match="scTickRunPairs is pending"):
        ticks[0].set_ray_shapes(AABB)
    network(bufs, grid, parity=0)
    for t in ticks:
        t.run_pairs()
    got = ticks[0].ray_hits()
    assert np.array_equal(np.concatenate([t.world_matrices() for t in ticks]), m)
    assert all(t.counts().border_lost == 0 for t in ticks)
    want = sr.cast(m, mn, mx, w.group, w.mask, col, *q, own=np.arange(w.n) < n)
    assert list(want["hit"]) == [1] * 8
    assert np.array_equal(want["id"][:4], own.astype(np.uint32)) and np.array_equal(want["id"][4:], near.astype(np.uint32))
    assert np.array_equal(tiles.global_pair_ids(got["id"].reshape(-1, 1), n).ravel(), want["id"].astype(np.uint64))
    assert ((got["id"][4:] >> 24) == 1).all() and (got["pad"] == 0).all()
    for f in ("hit", "layer"):
        assert np.array_equal(got[f], want[f])
    for f in ("distance", "position", "normal"):
        assert np.array_equal(got[f].view(np.uint32), want[f].view(np.uint32)), f
    # the own spheres answer at their surface (4 - sqrt(0.25 - 0.09) = 3.6), the neighbour's at their AABB's face (2.3 - 0.5 = 1.8)
    assert np.allclose(got["distance"][:4], 3.6, atol=1e-4) and np.allclose(got["distance"][4:], 1.8, atol=1e-4)
    assert (got["normal"][4:] == F([-1, 0, 0])).all() and (got["normal"][:4, 2] > 0.5).all()
    whole = sr.cast(m, mn, mx, w.group, w.mask, col, *q)                        # what one context over the whole world would answer
    assert np.allclose(whole["distance"][4:], 1.9, atol=1e-4)
    # a pipelined context refuses the run
    stream = torch.cuda.Stream()
    ticks[1].set_pairs_stream(stream.cuda_stream)
    ticks[1].set_ray_queries(*q)
    assert ticks[1].lib.scTickRun(ticks[1].ctx, flags) == 0
    assert b"SC_TICK_RAY_SHAPES_EXACT cannot run on a pipelined context" in ticks[1].lib.scTickGetLastError(ticks[1].ctx)
    for t in ticks:
        t.close()
    ow.close()


# ---- 8b. the caller-owned gap of a split tick ------------------------------------------------------------------------
def test_the_gap_of_an_exact_split_tick_refuses_what_would_change_its_shapes(oracle):
    """The pair half of a split tick refines against the matrices, colliders and dense indices as they stand when it runs, so in EXACT
    mode the calls that rewrite one of them are refused between the halves -- tick t's answers stay tick t's.  AABB mode keeps the free
    gap: the records hold tick t's boxes, a host may scramble the matrices."""
    w = worlds.random_world(900, seed=281, spread=50.0, max_depth=2)
    rng = np.random.default_rng(282)
    col = cr.Colliders.random(w.n, rng)
    k = 400
    q = rays_of(rng.uniform(-50, 50, (k, 3)), rng.normal(size=(k, 3)), rng.uniform(5, 80, k))
    t, ow = start(oracle, w, col)
    t.set_ray_queries(*q)
    split = RAYS | capi.SPLIT_PAIRS
    t.run(split)
    m = ow.world_matrices()[:w.n]
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
    with pytest.raises(capi.ScTickError, match="scTickRun with SC_TICK_XFORM " + refused):
        t.run(capi.XFORM)
    t.nudge_roots_x(5.0)                                                        # locals are the next tick's: welcome
    t.run_pairs()
    assert np.array_equal(t.world_matrices(), m)
    want = witness(ow, w, col, q)
    compare(t.ray_hits(), want)                                                 # tick t's shapes, untouched
    assert want["hit"].sum() > 50 and (want["distance"].view(np.uint32) != witness(ow, w, col, q, mode=sr.AABB)["distance"].view(np.uint32)).sum() > 20
    # behind the pair half the same calls work; without rays in the pending tick nothing is refused either
    t.upload_world_matrices(0, m)
    ow.nudge_roots_x(5.0); ow.transform_system()
    t.run(FLAGS | capi.SPLIT_PAIRS)
    t.upload_world_matrices(0, ow.world_matrices()[:w.n])
    t.run_pairs()
    # AABB mode: the host owns the gap
    t.set_ray_shapes(AABB)
    t.run(split)
    same_world(t, ow, w, col)
    t.upload_world_matrices(0, scrambled)
    t.run_pairs()
    compare(t.ray_hits(), witness(ow, w, col, q, mode=sr.AABB))
    t.close(); ow.close()


# ---- 9. errors ------------------------------------------------------------------------------------------------------
def test_ray_shape_api_errors(oracle):
    w = worlds.random_world(300, seed=291, spread=40.0)
    t = WorldTick.from_world(w, broadphase=True)
    assert t.ray_shapes() == AABB
    for bad in (2, 7, ALL):
        with pytest.raises(capi.ScTickError, match="unknown ray shape mode"):
            t.set_ray_shapes(bad)
    assert t.ray_shapes() == AABB
    assert t.lib.scTickGetRayShapes(t.ctx, None) == 0
    assert b"null argument" in t.lib.scTickGetLastError(t.ctx)
    t.set_ray_shapes(EXACT)
    t.run(FLAGS | capi.SPLIT_PAIRS)
    with pytest.raises(capi.ScTickError, match="scTickRunPairs is pending"):
        t.set_ray_shapes(AABB)
    assert t.ray_shapes() == EXACT
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_RAYS"):      # the missing flag is named before the pending half
        t.ray_hits()
    t.run_pairs()
    t.run(RAYS | capi.SPLIT_PAIRS)
    with pytest.raises(capi.ScTickError, match="ray hits are ready after scTickRunPairs"):
        t.ray_hits()
    t.run_pairs()
    assert len(t.ray_hits()) == 0
    t.set_ray_shapes(AABB)
    assert t.ray_shapes() == AABB
    # EXACT mode on a context without colliders: nothing is refined, the answers are the AABB mode's
    rng = np.random.default_rng(292)
    q = rays_of(rng.uniform(-40, 40, (200, 3)), rng.normal(size=(200, 3)), np.full(200, 60.0, F))
    t.set_ray_queries(*q)
    t.run(RAYS)
    plain = t.ray_hits()
    t.set_ray_shapes(EXACT)
    t.run(RAYS)
    assert t.ray_hits().tobytes() == plain.tobytes() and 10 < plain["hit"].sum() < 200
    t.close()
