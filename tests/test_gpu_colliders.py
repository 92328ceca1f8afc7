"""Broadphase proxies from Collider shapes (scTickUploadColliders) against a witness that is
independent of the kernels: tests/collider_ref.py restates the box rule in numpy fp32 on the ORACLE's world matrices, and
its boxes go to the oracle's brute-force / grid pair search and ray cast.  Boxes read back from the device must equal the
witness under IEEE ==, pair sets must be identical; nothing is excluded."""
import numpy as np
import pytest

from sc_gameengine_amd import capi, synth_world as sw, tiles
from sc_gameengine_amd.tick import WorldTick, camera_view_proj
from tests import collider_ref as cr, worlds

pytestmark = pytest.mark.gpu
FLAGS = capi.XFORM | capi.BROADPHASE | capi.DENSE_AABBS
F = np.float32


def sorted_pairs(p):
    p = np.asarray(p, np.uint32).reshape(-1, 2)
    if len(p) == 0:
        return p
    k = p[:, 0].astype(np.uint64) << np.uint64(32) | p[:, 1].astype(np.uint64)
    return p[np.argsort(k)]


Colliders = cr.Colliders          # the host model of the per-entity collider state (shared with tests/test_gpu_tail_matrix.py)


def check_tick(oracle, t, ow, w, col, brute=True, cell=64.0):
    """One tick's boxes and pair set against the witness; returns (witness boxes, wanted pairs)."""
    mn, mx = col.witness(ow, w.n)
    gmn, gmx = t.world_aabbs()
    assert np.array_equal(gmn, mn) and np.array_equal(gmx, mx), f"{(gmn != mn).any(axis=1).sum() + (gmx != mx).any(axis=1).sum()} boxes differ from the witness"
    want = oracle.broadphase_bruteforce(mn, mx, w.group, w.mask) if brute else oracle.broadphase_grid(mn, mx, w.group, w.mask, cell)
    got, total = t.pairs()
    assert total == len(want), f"pair count {total} != {len(want)}"
    assert np.array_equal(sorted_pairs(got), want)
    c = t.counts()
    assert c.pairs_truncated == 0 and c.border_lost == 0
    return (mn, mx), want


def run_ticks(oracle, w, col, ticks=3, nudge=0.7, brute=True, flags=FLAGS, max_pairs=1 << 18):
    ow = worlds.oracle_world(oracle, w, camera=False)
    t = WorldTick.from_world(w, broadphase=True, max_pairs=max_pairs)
    if col is not None:
        col.upload(t)
    model = col if col is not None else Colliders(w.n)
    wants = []
    for k in range(ticks):
        if k:
            ow.nudge_roots_x(nudge); t.nudge_roots_x(nudge)
        ow.transform_system()
        t.run(flags)
        wants.append(check_tick(oracle, t, ow, w, model, brute=brute)[1])
    return t, ow, wants


# ---- 1. the default is unchanged -----------------------------------------------------------------------------------
def test_default_unchanged_without_the_call_and_with_all_bounds(oracle):
    w = worlds.random_world(3000, seed=31, spread=150.0, max_depth=3)          # the world of test_random_world_mixed_layers
    ow = worlds.oracle_world(oracle, w, camera=False)
    a = WorldTick.from_world(w, broadphase=True, max_pairs=1 << 18)                               # no collider call at all
    b = WorldTick.from_world(w, broadphase=True, max_pairs=1 << 18)
    b.upload_colliders(0, np.full(w.n, capi.COLLIDER_BOUNDS, np.uint8))         # every entity explicitly BOUNDS: the collider instances run
    for k in range(3):
        if k:
            ow.nudge_roots_x(0.7); a.nudge_roots_x(0.7); b.nudge_roots_x(0.7)
        ow.transform_system()
        a.run(FLAGS); b.run(FLAGS)
        mn, mx = ow.world_aabbs()
        for t in (a, b):
            gmn, gmx = t.world_aabbs()
            assert gmn.tobytes() == mn[:w.n].tobytes() and gmx.tobytes() == mx[:w.n].tobytes()        # byte-equal: to the oracle, hence to each other
        want = oracle.broadphase_bruteforce(mn, mx, w.group, w.mask)
        pa, pb = sorted_pairs(a.pairs()[0]), sorted_pairs(b.pairs()[0])
        assert np.array_equal(pa, want) and np.array_equal(pb, want) and len(want) > 50
    a.close(); b.close(); ow.close()


def test_box_of_centred_bounds_gives_the_bounds_pair_set(oracle):
    w = worlds.random_world(3000, seed=36, spread=150.0, max_depth=3, p_no_bounds=0.0)
    w.bmin[:] = -w.bmax
    col = Colliders(w.n)
    col.type[:] = cr.BOX; col.he[:] = w.bmax
    tb, owb, wb = run_ticks(oracle, w, None)
    tc, owc, wc = run_ticks(oracle, w, col)
    for x, y in zip(wb, wc):
        assert np.array_equal(x, y) and len(x) > 50
    assert np.array_equal(tb.world_aabbs()[0], tc.world_aabbs()[0]) and np.array_equal(tb.world_aabbs()[1], tc.world_aabbs()[1])
    for x in (tb, tc, owb, owc):
        x.close()


# ---- 2. mixed types ------------------------------------------------------------------------------------------------
def test_mixed_types_against_brute_force_and_culling_untouched(oracle):
    rng = np.random.default_rng(5)
    w = worlds.random_world(3000, seed=37, spread=150.0, max_depth=3, p_no_bounds=0.25)
    w.scale[:] = (rng.uniform(0.2, 3.0, (w.n, 3)) * rng.choice([-1.0, 1.0], (w.n, 3), p=[0.3, 0.7])).astype(F)       # non-uniform, some negative
    col = Colliders.random(w.n, rng)
    typed, none = col.type >= cr.BOX, col.type == cr.NONE
    assert (typed & (w.has_bounds == 0)).sum() > 100 and (none & (w.has_bounds == 1)).sum() > 100
    assert all((col.type == k).sum() > 200 for k in range(5))
    ow = worlds.oracle_world(oracle, w)
    t = WorldTick.from_world(w, broadphase=True, max_pairs=1 << 18)
    col.upload(t)
    vp = camera_view_proj(w.camera)
    t.set_view_proj(vp)
    for k in range(3):
        if k:
            ow.nudge_roots_x(0.7); t.nudge_roots_x(0.7)
        ow.transform_system(); ow.culling_system(view_proj=vp)
        t.run(capi.FULL | capi.DENSE_AABBS)
        _, want = check_tick(oracle, t, ow, w, col)
        assert len(want) > 50 and not none[want.ravel()].any()                      # NONE entities appear in no pair
        assert np.array_equal(t.visible(), ow.visible())                            # the cull sphere still comes from Bounds
        assert (typed & (w.has_bounds == 0))[want.ravel()].any()                    # typed colliders without Bounds do collide
    t.close(); ow.close()


# ---- 3. off-centre bounds: the box about the ORIGIN is another box --------------------------------------------------
def test_off_centre_bounds_box_differs_from_bounds(oracle):
    w = worlds.random_world(2500, seed=38, spread=60.0, p_child=0.3, p_no_bounds=0.0)
    w.bmin[:, 1] = 0.0                                                             # a mesh whose bounds start at y = 0
    col = Colliders(w.n)
    col.type[:] = cr.BOX
    col.he[:] = (w.bmax - w.bmin) * F(0.5)                                         # the bounds' half extents, about the origin
    tb, owb, wb = run_ticks(oracle, w, None, ticks=2)
    tc, owc, wc = run_ticks(oracle, w, col, ticks=2)
    for x, y in zip(wb, wc):
        assert len(x) > 50 and len(y) > 50 and not np.array_equal(x, y)
    for x in (tb, tc, owb, owc):
        x.close()


# ---- 4. extremes ---------------------------------------------------------------------------------------------------
def test_big_spheres_and_spheres_outside_the_rectangle(oracle):
    rng = np.random.default_rng(9)
    w = worlds.random_world(2500, seed=39, spread=700.0, max_depth=2)              # the rectangle is +-512 m
    col = Colliders.random(w.n, rng)
    col.type[:60] = cr.SPHERE; col.radius[:60] = rng.uniform(60.0, 150.0, 60).astype(F)      # wider than 2x2 sectors
    t, ow, wants = run_ticks(oracle, w, col, ticks=2)
    assert t.counts().big_boxes > 100 and len(wants[-1]) > 0
    t.close(); ow.close()


def test_three_hundred_colliders_in_one_sector(oracle):
    rng = np.random.default_rng(10)
    w = worlds.random_world(1500, seed=40, spread=300.0, p_child=0.0)
    w.pos[:300] = F([10.0, 0.0, 10.0]) + rng.uniform(-8, 8, (300, 3)).astype(F)
    col = Colliders.random(w.n, rng, p=(0.1, 0.1, 0.3, 0.25, 0.25))
    col.type[:300] = rng.choice([cr.BOX, cr.SPHERE, cr.CAPSULE], 300).astype(np.uint8)
    t, ow, wants = run_ticks(oracle, w, col, ticks=2)
    assert t.counts().bin_overflow > 200 and len(wants[-1]) > 1000
    t.close(); ow.close()


def test_chains_deeper_than_the_fused_kernel_walks(oracle):
    rng = np.random.default_rng(11)
    w = worlds.chain_world(12, branches=20, seed=41)
    w.pos[:20] = rng.uniform(-100, 100, (20, 3)).astype(F)
    col = Colliders.random(w.n, rng)
    t, ow, wants = run_ticks(oracle, w, col, ticks=3, nudge=1.5)
    assert t.counts().max_depth > 3 and (col.type[w.n // 2:] >= cr.BOX).sum() > 20
    t.close(); ow.close()


# ---- 5. lazy records, home slots, cleanStay, graph replay -----------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_capsule_driven_through_static_sphere_props(oracle, graph):
    """Static props (they cannot meet each other: their bins stay unwritten between learn ticks) with sphere colliders, one dynamic
    capsule driven through them for 75 ticks -- past a learn period -- so the pair search has to REBUILD the props' records from
    their colliders when the capsule enters their sector.  The pair set is checked on every tick."""
    w = sw.generate(8, 8, 15)
    n = w.n
    col = Colliders(n)
    roots = np.flatnonzero(w.parent < 0)
    props = roots[roots % 16 != 0]
    col.type[props] = cr.SPHERE; col.radius[props] = 2.5
    cap = int(props[0])
    w.group[cap], w.mask[cap] = sw.GROUP_DYNAMIC, sw.MASK_ALL
    w.rot[cap] = 0.0; w.scale[cap] = 1.0
    col.type[cap] = cr.CAPSULE; col.radius[cap] = 1.5; col.hh[cap] = 2.0
    ow = worlds.oracle_world(oracle, w, camera=False)
    t = WorldTick.from_world(w, broadphase=True, max_pairs=1 << 18)
    col.upload(t)
    t.set_graph_mode(graph)
    path = np.zeros((75, 3), F)
    path[:, 0] = np.linspace(5.0, 500.0, 75); path[:, 1] = 1.0; path[:, 2] = np.linspace(7.0, 470.0, 75)
    hits, rebuilt = 0, False
    for k in range(75):
        ow.set_local_positions(ow.dense_entities()[[cap]], path[k:k + 1]); t.upload_positions(cap, path[k:k + 1])
        ow.transform_system()
        t.run(FLAGS)
        _, want = check_tick(oracle, t, ow, w, col)
        hits += len(want)
        rebuilt = rebuilt or t.bin_stats()["lazy_last_tick"]
        if k == 40:
            # a collider upload between ticks changes the next tick's pairs although no matrix changes: the prop nearest to the
            # capsule's next position grows to reach it (its record may not stay as it is)
            d = np.linalg.norm(w.pos[props[1:]][:, [0, 2]] - path[41, [0, 2]], axis=1)
            grow = int(props[1:][np.argmin(d)])
            col.radius[grow] = F(d.min() + 3.0)
            col.upload(t, grow, 1)
            ow.set_local_positions(ow.dense_entities()[[cap]], path[41:42]); t.upload_positions(cap, path[41:42])
            ow.transform_system(); t.run(FLAGS)
            _, w41 = check_tick(oracle, t, ow, w, col)
            assert any(set(p) == {cap, grow} for p in w41.tolist())
    assert hits > 20 and rebuilt and t.bin_stats()["learn_ticks"] >= 2
    t.close(); ow.close()


# ---- 6. residency --------------------------------------------------------------------------------------------------
def test_colliders_follow_their_entities_and_new_indices_start_as_bounds(oracle):
    rng = np.random.default_rng(13)
    w = worlds.random_world(1200, seed=42, spread=120.0, p_child=0.0)
    col = Colliders.random(w.n, rng)
    t = WorldTick.from_world(w, broadphase=True, capacity=w.n, max_pairs=1 << 18)
    col.upload(t)
    gone = rng.choice(w.n, 200, replace=False).astype(np.uint32)
    src, dst = t.remove_entities(gone)
    keep = {k: getattr(w, k).copy() for k in ("pos", "rot", "scale", "bmin", "bmax", "has_bounds", "has_mesh", "group", "mask", "mesh", "material")}
    for a in list(keep.values()) + [col.type, col.he, col.radius, col.hh]:
        a[dst] = a[src]
    n1 = w.n - 200
    ty, he, r, hh = t.colliders()
    assert np.array_equal(ty, col.type[:n1]) and np.array_equal(he, col.he[:n1]) and np.array_equal(r, col.radius[:n1]) and np.array_equal(hh, col.hh[:n1])
    # append into the freed indices: BOUNDS with the default values, whatever collider lived there before
    k = 150
    apos = rng.uniform(-100, 100, (k, 3)).astype(F); arot = rng.uniform(-3, 3, (k, 3)).astype(F); ascl = rng.uniform(0.5, 2.0, (k, 3)).astype(F)
    abmin, abmax = -rng.uniform(0.5, 2.0, (k, 3)).astype(F), rng.uniform(0.5, 2.0, (k, 3)).astype(F)
    first = t.append_entities(apos, arot, ascl, bmin=abmin, bmax=abmax, group=np.full(k, 1, np.uint32), mask=np.full(k, 0xFFFFFFFF, np.uint32))
    assert first == n1
    n2 = n1 + k
    col.type[n1:n2] = cr.BOUNDS; col.he[n1:n2] = 0.5; col.radius[n1:n2] = 0.5; col.hh[n1:n2] = 0.5
    ty, he, r, hh = t.colliders()
    assert np.array_equal(ty, col.type[:n2]) and np.array_equal(he, col.he[:n2]) and np.array_equal(r, col.radius[:n2]) and np.array_equal(hh, col.hh[:n2])
    # the device agrees: boxes and pairs of the world as it now is
    w2 = sw.SynthWorld(pos=np.concatenate([keep["pos"][:n1], apos]), rot=np.concatenate([keep["rot"][:n1], arot]), scale=np.concatenate([keep["scale"][:n1], ascl]),
                       parent=np.full(n2, -1, np.int32), bmin=np.concatenate([keep["bmin"][:n1], abmin]), bmax=np.concatenate([keep["bmax"][:n1], abmax]),
                       has_mesh=np.concatenate([keep["has_mesh"][:n1], np.ones(k, np.uint8)]), has_bounds=np.concatenate([keep["has_bounds"][:n1], np.ones(k, np.uint8)]),
                       mesh=np.zeros(n2, np.uint32), material=np.zeros(n2, np.uint32),
                       group=np.concatenate([keep["group"][:n1], np.full(k, 1, np.uint32)]), mask=np.concatenate([keep["mask"][:n1], np.full(k, 0xFFFFFFFF, np.uint32)]),
                       sector_of=np.zeros((n2, 2), np.int32), origin=w.origin, sectors=w.sectors)
    ow = worlds.oracle_world(oracle, w2, camera=False)
    ow.transform_system()
    for _ in range(2):
        t.run(FLAGS)
        _, want = check_tick(oracle, t, ow, w2, col)
    assert len(want) > 20
    # a grown count starts its new indices as BOUNDS too
    t.set_count(n2 - 50); t.set_count(n2)
    assert (t.colliders()[0][n2 - 50:] == cr.BOUNDS).all()
    t.close(); ow.close()


# ---- 7. rays -------------------------------------------------------------------------------------------------------
def test_ray_queries_hit_the_collider_boxes_and_never_a_none_entity(oracle):
    rng = np.random.default_rng(14)
    w = worlds.random_world(2500, seed=43, spread=120.0, max_depth=2)
    w.group[:] = rng.choice([1, 2, 4], w.n).astype(np.uint32); w.mask[:] = 0xFFFFFFFF
    col = Colliders.random(w.n, rng)
    ow = worlds.oracle_world(oracle, w, camera=False)
    t = WorldTick.from_world(w, broadphase=True, max_pairs=1 << 18)
    col.upload(t)
    q = 512
    org = rng.uniform(-130, 130, (q, 3)).astype(F); dr = rng.normal(size=(q, 3)).astype(F)
    md = rng.uniform(10, 200, q).astype(F); rmask = rng.choice([1, 2, 4, 7, 0xFFFFFFFF], q).astype(np.uint32)
    # and rays aimed straight at NONE entities that have Bounds
    none = np.flatnonzero((col.type == cr.NONE) & (w.has_bounds == 1) & (w.parent < 0))[:64]
    org[:len(none)] = w.pos[none] + F([0.0, 30.0, 0.0]); dr[:len(none)] = F([0.0, -1.0, 0.0]); md[:len(none)] = 60.0; rmask[:len(none)] = 0xFFFFFFFF
    t.set_ray_queries(org, dr, md, rmask)
    ow.transform_system()
    t.run(FLAGS | capi.RAYS)
    (mn, mx), _ = check_tick(oracle, t, ow, w, col)
    want = oracle.raycast_boxes(mn, mx, w.group, w.mask, org, dr, md, rmask)
    got = t.ray_hits()
    assert len(got) == len(want)
    for f in ("hit", "id", "layer"):
        assert np.array_equal(got[f], want[f]), f
    for f in ("distance", "position", "normal"):
        assert np.array_equal(got[f][got["hit"] == 1].view(np.uint32), want[f][want["hit"] == 1].view(np.uint32)), f        # bit patterns
    assert got["hit"].sum() > 50 and len(none) > 20
    assert not np.isin(got["id"][got["hit"] == 1] & 0xFFFFFF, np.flatnonzero(col.type == cr.NONE)).any()
    t.close(); ow.close()


# ---- 8. tiles ------------------------------------------------------------------------------------------------------
def _tile_world():
    grid, S = (2, 1), (6, 6)
    w = sw.generate(S[0] * grid[0], S[1] * grid[1], 15, tiles=grid)
    rng = np.random.default_rng(15)
    dyn = rng.random(w.n) < 0.3
    w.group[dyn], w.mask[dyn] = sw.GROUP_DYNAMIC, sw.MASK_ALL
    roots = np.flatnonzero((w.parent < 0) & (np.arange(w.n) % 16 != 0))
    edge = rng.choice(roots, len(roots) // 6, replace=False)
    w.pos[edge, 0] = (64.0 * S[0] + rng.uniform(-1.5, 1.5, len(edge))).astype(F)       # right onto the border between the two tiles
    col = Colliders(w.n)
    col.type[roots] = rng.choice([cr.BOUNDS, cr.BOX, cr.SPHERE, cr.CAPSULE], len(roots)).astype(np.uint8)
    col.type[edge] = rng.choice([cr.SPHERE, cr.CAPSULE], len(edge)).astype(np.uint8)   # spheres and capsules straddle it
    col.radius[:] = rng.uniform(0.5, 2.5, w.n).astype(F); col.hh[:] = rng.uniform(0.0, 2.0, w.n).astype(F)
    col.he[:] = rng.uniform(0.3, 2.0, (w.n, 3)).astype(F)
    col.type[rng.choice(roots, 200, replace=False)] = cr.NONE
    return w, col, grid, S


def _check_tiles(oracle, ticks, ow, w, col, n):
    mn, mx = col.witness(ow, w.n)
    want = oracle.broadphase_grid(mn, mx, w.group, w.mask, 16.0)
    got = []
    for t in ticks:
        p, total = t.pairs()
        c = t.counts()
        assert total == len(p) and c.border_lost == 0 and c.pairs_truncated == 0
        got.append(tiles.global_pair_ids(p, n))
    got = np.concatenate(got).astype(np.uint64)
    key = np.sort(np.minimum(got[:, 0], got[:, 1]) << np.uint64(32) | np.maximum(got[:, 0], got[:, 1]))
    wkey = want[:, 0].astype(np.uint64) << np.uint64(32) | want[:, 1].astype(np.uint64)
    assert len(key) == len(np.unique(key)), "a pair was reported twice"
    assert np.array_equal(key, wkey), f"{len(np.setdiff1d(wkey, key))} missing, {len(np.setdiff1d(key, wkey))} unexpected of {len(wkey)}"
    assert len(wkey) > 50 and ((want[:, 0] // n) != (want[:, 1] // n)).sum() > 5       # pairs across the border occur


def test_two_tiles_in_order(oracle):
    import torch
    from tests.test_gpu_tiles import split_world
    w, col, grid, S = _tile_world()
    parts, n = split_world(w, grid, S)
    ow = worlds.oracle_world(oracle, w, camera=False)
    ticks = [WorldTick.from_world(p, broadphase=True, max_pairs=1 << 16) for p in parts]
    for r, t in enumerate(ticks):
        t.upload_colliders(0, col.type[r * n:(r + 1) * n], col.he[r * n:(r + 1) * n], col.radius[r * n:(r + 1) * n], col.hh[r * n:(r + 1) * n])
    bufs = [tiles.BorderBuffers(t, r, grid, "cuda") for r, t in enumerate(ticks)]
    for step in range(3):
        if step:
            ow.nudge_roots_x(0.9)
            for t in ticks:
                t.nudge_roots_x(0.9)
        ow.transform_system()
        for t in ticks:
            t.run(capi.XFORM | capi.BROADPHASE | capi.SPLIT_PAIRS)
        for t in ticks:
            t.sync()
        for r, b in enumerate(bufs):
            for d, nb in tiles.neighbours(r, grid).items():
                bufs[nb].recv[7 - d].copy_(b.send[d])
        torch.cuda.synchronize()
        for t in ticks:
            t.run_pairs()
        _check_tiles(oracle, ticks, ow, w, col, n)
    for t in ticks:
        t.close()
    ow.close()


def test_two_tiles_pipelined(oracle):
    import torch
    from tests.test_gpu_tiles import split_world
    w, col, grid, S = _tile_world()
    parts, n = split_world(w, grid, S)
    ow = worlds.oracle_world(oracle, w, camera=False)
    ticks, bufs, s1, s2 = [], [], [], []
    for r, p in enumerate(parts):
        t = WorldTick.from_world(p, broadphase=True, max_pairs=1 << 16)
        t.upload_colliders(0, col.type[r * n:(r + 1) * n], col.he[r * n:(r + 1) * n], col.radius[r * n:(r + 1) * n], col.hh[r * n:(r + 1) * n])
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        t.set_stream(a.cuda_stream, external=True)
        t.set_pairs_stream(b.cuda_stream)
        t.set_frame_producer(1, 0.7)
        ticks.append(t); s1.append(a); s2.append(b)
        bufs.append(tiles.BorderBuffers(t, r, grid, "cuda", pipelined=True))
    for t in ticks:
        t.nudge_roots_x(0.7)
    steps = 6
    for step in range(steps):
        q = step % len(bufs[0].sets)
        for t in ticks:
            t.run(capi.XFORM | capi.BROADPHASE | capi.SPLIT_PAIRS | capi.PRODUCE_NEXT)
        for r, b in enumerate(bufs):
            for d, nb in tiles.neighbours(r, grid).items():
                s2[nb].wait_stream(s1[r])
                with torch.cuda.stream(s2[nb]):
                    bufs[nb].sets[q][3][7 - d].copy_(b.sets[q][2][d], non_blocking=True)
        for t in ticks:
            t.run_pairs()
    for _ in range(steps):
        ow.nudge_roots_x(0.7)
    ow.transform_system()
    _check_tiles(oracle, ticks, ow, w, col, n)
    torch.cuda.synchronize()
    for t in ticks:
        t.close()
    ow.close()


# ---- 9. errors -----------------------------------------------------------------------------------------------------
def test_bad_uploads_fail_with_a_message_and_change_nothing():
    t = WorldTick(64)
    t.set_count(10)
    t.upload_colliders(0, np.full(10, cr.SPHERE, np.uint8), radius=np.full(10, 2.0, F))
    before = [a.copy() for a in t.colliders()]
    ok = np.full(4, cr.BOX, np.uint8)
    for kw, text in ((dict(type=np.array([2, 5, 2, 2], np.uint8)), "unknown collider type"),
                     (dict(type=ok, radius=F([1, -1, 1, 1])), "radius"),
                     (dict(type=ok, half_extents=F([[1, 1, 1], [1, np.nan, 1], [1, 1, 1], [1, 1, 1]])), "half extents"),
                     (dict(type=ok, half_extents=F([[1, 1, 1], [1, -0.5, 1], [1, 1, 1], [1, 1, 1]])), "half extents"),
                     (dict(type=ok, radius=F([1, np.inf, 1, 1])), "radius"),
                     (dict(type=ok, half_height=F([1, np.nan, 1, 1])), "half height")):
        with pytest.raises(capi.ScTickError, match=text):
            t.upload_colliders(2, **kw)
    with pytest.raises(capi.ScTickError, match="range exceeds entity count"):
        t.upload_colliders(8, ok)
    after = t.colliders()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    # defaults: type None = BOX, missing arrays = 0.5; a negative half height is stored as 0
    t.upload_colliders(0, None, half_height=F([-2.0, 1.0]))
    ty, he, r, hh = t.colliders()
    assert (ty[:2] == cr.BOX).all() and (he[:2] == 0.5).all() and (r[:2] == 0.5).all() and np.array_equal(hh[:2], F([0.0, 1.0]))
    t.close()
