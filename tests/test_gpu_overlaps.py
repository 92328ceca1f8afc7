"""Overlap queries (scTickSetOverlapQueries, SC_TICK_OVERLAPS) through the C ABI against the witness of tests/overlap_ref.py: the
collider box rule for the volumes' boxes, the oracle's brute force over every box for AABB mode, touching32 over its hits for EXACT mode.
Every answer is compared as a sorted id set per volume, plus the counts, plus the report.  tests/test_overlaps_cpu.py proves without a
GPU that the cases (tests/overlap_cases.py) are what they claim.  Every batch runs for the learn tick and a tick on the home slots."""
import numpy as np
import pytest

from sc_gameengine_amd import capi
from sc_gameengine_amd.tick import WorldTick
from tests import overlap_cases as oc, overlap_ref as ref, ray_walk_cases as rc, worlds

pytestmark = pytest.mark.gpu
BASE = capi.XFORM | capi.BROADPHASE
FLAGS = BASE | capi.OVERLAPS
AABB, EXACT = capi.OVERLAP_SHAPES_AABB, capi.OVERLAP_SHAPES_EXACT
F = np.float32
U = np.uint32
TICKS = 2                 # the learn tick and one on the home slots


def compare(t, want):
    """the last run's answer against (sets, counts, info) of the witness"""
    sets, counts, info = want
    got_counts, ids = t.overlap_hits()
    got_info = t.overlap_info()
    assert got_info == info, f"{got_info} != {info}"
    assert np.array_equal(got_counts, counts)
    mh = info["max_hits"]
    assert ids.shape == (len(counts), mh)
    for q in range(len(counts)):
        got = ids[q, :min(int(counts[q]), mh)]
        assert len(np.unique(got)) == len(got), q                              # every entity at most once
        if counts[q] <= mh:
            assert np.array_equal(np.sort(got), sets[q]), q
        else:
            assert np.isin(got, sets[q]).all(), q                              # max_hits distinct members of the true set


def witness(oracle, mn, mx, w, vol, max_hits, shapes=AABB, m=None, col=None):
    hits = ref.aabb_hits(oracle, mn, mx, w.group, w.mask, vol)
    if shapes == AABB:
        return ref.answer(hits, len(vol["type"]), max_hits)
    touching, refined = ref.exact_hits(hits, m, col, vol, w.n)
    return ref.answer(hits, len(vol["type"]), max_hits, EXACT, touching, refined)


def run_boxes(oracle, w, vol, max_hits=64, shapes=AABB, graph=False, max_pairs=0):
    """a world of Bounds boxes on unrotated roots (rc.box_world): the boxes are the world's own bmin / bmax"""
    want = witness(oracle, w.bmin, w.bmax, w, vol, max_hits, shapes)
    t = WorldTick.from_world(w, broadphase=True, max_pairs=max_pairs)
    t.overlap_queries(*ref.args(vol), max_hits=max_hits, shapes=shapes)
    if graph:
        t.set_graph_mode(True)
    for _ in range(5 if graph else TICKS):
        t.run(FLAGS)
        compare(t, want)
    c = t.counts()
    t.close()
    return want, c


def mixed(oracle, world=None):
    """(world, colliders, oracle matrices, witness boxes with colliders, Bounds boxes without)"""
    w, col = oc.mixed_world() if world is None else world
    ow = worlds.oracle_world(oracle, w, camera=False); ow.transform_system()
    m = ow.world_matrices()[:w.n].copy()
    mn, mx = col.witness(ow, w.n)
    bmn, bmx = ow.world_aabbs()
    ow.close()
    return w, col, m, (mn, mx), (bmn[:w.n], bmx[:w.n])


# ---- (a) volume types -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [AABB, EXACT])
def test_every_volume_type_against_bounds_proxies(oracle, shapes):
    """no colliders uploaded: the entities' boxes are their Bounds boxes, and EXACT mode has nothing to refine -- the same answer"""
    w, _, m, _, bounds = mixed(oracle)
    vol, _ = oc.volume_table()
    want = witness(oracle, *bounds, w, vol, oc.TABLE_MAX_HITS, shapes, m, None)
    assert want[2]["hits"] >= 1000 and want[2]["refined"] == 0 and want[2]["kept_as_boxes"] == (want[2]["hits"] if shapes == EXACT else 0)
    t = WorldTick.from_world(w, broadphase=True)
    t.overlap_queries(*ref.args(vol), max_hits=oc.TABLE_MAX_HITS, shapes=shapes)
    for _ in range(TICKS):
        t.run(FLAGS)
        assert np.array_equal(t.world_matrices(), m)
        compare(t, want)
    t.close()


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("shapes", [AABB, EXACT])
def test_every_volume_type_against_mixed_colliders(oracle, shapes, graph):
    """boxes, spheres and capsules -- axis-aligned, and rotated with a non-uniform scale -- against oriented boxes, spheres, capsules,
    Bounds proxies and entities without a proxy; masks that meet nobody and skipped ids among them"""
    w, col, m, boxes, _ = mixed(oracle)
    vol, _ = oc.volume_table()
    want = witness(oracle, *boxes, w, vol, oc.TABLE_MAX_HITS, shapes, m, col)
    t = WorldTick.from_world(w, broadphase=True)
    col.upload(t)
    t.overlap_queries(*ref.args(vol), max_hits=oc.TABLE_MAX_HITS, shapes=shapes)
    if graph:
        t.set_graph_mode(True)
    for _ in range(5 if graph else TICKS):
        t.run(FLAGS | capi.DENSE_AABBS)
        assert np.array_equal(t.world_matrices(), m)
        gmn, gmx = t.world_aabbs()
        has = np.isfinite(boxes[0][:, 0])
        assert np.array_equal(gmn[:w.n][has].view(U), boxes[0][has].view(U)) and np.array_equal(gmx[:w.n][has].view(U), boxes[1][has].view(U))
        compare(t, want)
    if shapes == EXACT:
        assert want[2]["refined"] >= 2000 and want[2]["kept_as_boxes"] >= 100 and want[2]["hits"] < want[2]["refined"] + want[2]["kept_as_boxes"]
    t.close()


@pytest.mark.parametrize("shapes", [AABB, EXACT])
def test_a_degenerate_volume_keeps_its_box_answers_and_a_nan_volume_meets_nothing(oracle, shapes):
    w, col, m, boxes, _ = mixed(oracle)
    vol, names = oc.odd_volumes()
    want = witness(oracle, *boxes, w, vol, 512, shapes, m, col)
    assert want[1][0] >= 1 and want[1][1] >= 100 and want[1][2] == 0 and want[2]["refined"] == 0
    t = WorldTick.from_world(w, broadphase=True)
    col.upload(t)
    t.overlap_queries(*ref.args(vol), max_hits=512, shapes=shapes)
    for _ in range(TICKS):
        t.run(FLAGS)
        compare(t, want)
    t.close()


# ---- (b) duplicates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_a_box_in_two_or_four_sectors_answers_once(oracle, graph):
    w, vol, sets = oc.straddle_case()
    want, _ = run_boxes(oracle, w, vol, graph=graph)
    assert [list(s) for s in want[0]] == sets


# ---- (c) sector edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_a_closed_touch_on_a_sector_boundary_is_a_hit_and_one_float_short_is_not(oracle, graph):
    w, vol, meta = oc.edge_case()
    want, _ = run_boxes(oracle, w, vol, graph=graph)
    assert np.array_equal(want[1], (meta["role"] >= 1).astype(U))


# ---- (d) the crowded sector -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_a_crowded_sector_answers_from_its_bin_and_the_overflow_list(oracle, graph):
    w, _, _ = rc.crowded_world()
    want, c = run_boxes(oracle, w, oc.crowded_volumes(), max_hits=128, graph=graph, max_pairs=1 << 12)
    assert c.bin_overflow == 26 and want[1][1] == 92


# ---- (e) the big list -------------------------------------------------------------------------------------------------------------
def test_big_boxes_a_volume_over_the_whole_grid_and_one_outside_it(oracle):
    w, vol = oc.big_case()
    want, c = run_boxes(oracle, w, vol)
    assert c.big_boxes == 2 and [list(s) for s in want[0]] == [[0, 1, 2, 3, 4], [1], [], [0]]


# ---- (f) mask, skip_id, truncation ------------------------------------------------------------------------------------------------
def test_mask_and_skip_id_are_honoured(oracle):
    want, _ = run_boxes(oracle, oc.line_world(), oc.filter_volumes(), max_hits=128)
    assert list(want[1]) == [24, 23, 22, 46, 70]


@pytest.mark.parametrize("max_hits", oc.MAX_HITS)
def test_a_row_that_is_too_short_holds_members_and_the_count_stays_true(oracle, max_hits):
    vol, m = oc.line_volumes(max_hits)
    want, _ = run_boxes(oracle, oc.line_world(), vol, max_hits=max_hits)
    assert list(want[1]) == [0, max_hits, max_hits + 1] and want[2]["truncated_queries"] == 1


# ---- (g) query counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", oc.QUERY_COUNTS)
def test_query_counts_that_leave_waves_without_a_volume(oracle, count):
    w, col, m, boxes, _ = mixed(oracle)
    base, _ = oc.volume_table()
    vol, idx = oc.tiled(base, count)
    sets, counts, _ = witness(oracle, *boxes, w, base, 32, EXACT, m, col)
    hits = ref.aabb_hits(oracle, *boxes, w.group, w.mask, base)
    touching, refined = ref.exact_hits(hits, m, col, base, w.n)
    per_refined, per_kept = np.bincount(hits[refined, 1], minlength=len(counts)), np.bincount(hits[touching & ~refined, 1], minlength=len(counts))
    info = dict(queries=count, max_hits=32, hits=int(counts[idx].sum()), truncated_queries=int((counts[idx] > 32).sum()),
                refined=int(per_refined[idx].sum()), kept_as_boxes=int(per_kept[idx].sum()), shapes=EXACT)
    t = WorldTick.from_world(w, broadphase=True)
    col.upload(t)
    t.overlap_queries(*ref.args(vol), max_hits=32, shapes=EXACT)
    if count == 5:
        t.set_graph_mode(True)
    for _ in range(TICKS):
        t.run(FLAGS)
        compare(t, ([sets[i] for i in idx], counts[idx], info))
    t.close()


# ---- (h) quiet ticks --------------------------------------------------------------------------------------------------------------
def test_the_first_flagged_tick_after_quiet_ones_sees_every_record(oracle):
    """a world that cannot pair runs quiet ticks (no bin is filled); a flagged tick fills them all and answers as the witness says"""
    w, col, m, boxes, _ = mixed(oracle, oc.quiet_world())
    vol, _ = oc.volume_table()
    want = witness(oracle, *boxes, w, vol, oc.TABLE_MAX_HITS, EXACT, m, col)
    assert want[2]["hits"] >= 1000
    t = WorldTick.from_world(w, broadphase=True)
    col.upload(t)
    t.overlap_queries(*ref.args(vol), max_hits=oc.TABLE_MAX_HITS, shapes=EXACT)
    t.run(BASE)                                             # the learn tick
    for _ in range(3):
        t.run(BASE)
        assert t.bin_stats()["quiet_last_tick"]
    for _ in range(2):
        t.run(FLAGS)
        assert not t.bin_stats()["quiet_last_tick"] and not t.bin_stats()["lazy_last_tick"]
        compare(t, want)
        t.run(BASE)
        assert t.bin_stats()["quiet_last_tick"]
    assert t.learn_ticks() == 1
    t.close()


# ---- (i) the setter under graph replay: an eager and a graph-mode context side by side -----------------------------------------
def test_replacing_the_set_under_graph_replay(oracle):
    """the set is replaced after capture -- other sizes, an empty set, the first size again --, then the mode, then max_hits: after
    every tick, of both parities, the replaying context answers what the eager one does and what the witness says"""
    w, col, m, boxes, _ = mixed(oracle)
    base, _ = oc.volume_table()
    twins = [WorldTick.from_world(w, broadphase=True) for _ in range(2)]
    for t in twins:
        col.upload(t)
    twins[1].set_graph_mode(True)
    steps = [(16, 64, EXACT), (9, 64, EXACT), (1500, 64, EXACT), (0, 64, EXACT), (16, 64, EXACT), (16, 64, AABB), (16, 5, AABB), (16, 5, AABB)]
    rng = np.random.default_rng(77)
    for step, (size, max_hits, shapes) in enumerate(steps):
        vol, _ = oc.tiled(ref.take(base, rng.permutation(len(base["type"]))), size)
        learn = [t.learn_ticks() for t in twins]
        for t in twins:
            t.overlap_queries(*ref.args(vol), max_hits=max_hits, shapes=shapes)
        if not size:
            for t in twins:
                with pytest.raises(capi.ScTickError, match="needs scTickSetOverlapQueries first"):
                    t.run(FLAGS)
                t.run(BASE)
            continue
        want = witness(oracle, *boxes, w, vol, max_hits, shapes, m, col)
        for tick in range(3):                               # a fresh capture where one is due, then both parities replayed
            for t in twins:
                t.run(FLAGS)
                compare(t, want)
            # ... and the twins agree with each other: the counts, the reports, and every row that holds its whole answer (the slots behind
            # a row's count are unspecified, and so is which members a truncated row holds)
            a, b = twins[0].overlap_hits(), twins[1].overlap_hits()
            assert np.array_equal(a[0], b[0]) and twins[0].overlap_info() == twins[1].overlap_info()
            for q in np.flatnonzero(a[0] <= max_hits):
                assert np.array_equal(np.sort(a[1][q, :a[0][q]]), np.sort(b[1][q, :b[0][q]])), (step, tick, q)
        # the same count, max_hits and mode as the set before (the last step): no learn tick; anything else: one
        same = step > 0 and steps[step - 1] == steps[step]
        assert [t.learn_ticks() - l for t, l in zip(twins, learn)] == [0 if same else 1] * 2, step
    for t in twins:
        t.close()


# ---- (j) moving entities ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_answers_follow_the_entities(oracle, graph):
    w, col = oc.mixed_world()
    vol, _ = oc.volume_table()
    ow = worlds.oracle_world(oracle, w, camera=False)
    t = WorldTick.from_world(w, broadphase=True)
    col.upload(t)
    t.overlap_queries(*ref.args(vol), max_hits=oc.TABLE_MAX_HITS, shapes=EXACT)
    if graph:
        t.set_graph_mode(True)
    seen = []
    for tick in range(4):
        ow.nudge_roots_x(1.75); t.nudge_roots_x(1.75)
        ow.transform_system()
        m = ow.world_matrices()[:w.n].copy()
        want = witness(oracle, *col.witness(ow, w.n), w, vol, oc.TABLE_MAX_HITS, EXACT, m, col)
        t.run(FLAGS)
        assert np.array_equal(t.world_matrices(), m)
        compare(t, want)
        seen.append(np.concatenate(want[0]))
    assert all(not np.array_equal(seen[k], seen[k + 1]) for k in range(3))      # the answers did change
    t.close(); ow.close()


# ---- (k) refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_has_its_text(oracle):
    w = oc.line_world()
    vol = oc.filter_volumes()
    a = list(ref.args(vol))
    t = WorldTick.from_world(w, broadphase=True)
    with pytest.raises(capi.ScTickError, match="needs scTickSetOverlapQueries first"):
        t.run(FLAGS)
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_OVERLAPS"):
        t.overlap_hits()
    t.overlap_queries(*a, max_hits=8)
    bad = [(1, "m16", np.nan), (3, "radius", np.inf), (2, "he", np.nan), (4, "hh", -np.inf)]
    for at, name, value in bad:
        b = [x.copy() if x is not None else None for x in a]
        b[at].reshape(-1)[1] = value
        with pytest.raises(capi.ScTickError, match="must be finite"):
            t.overlap_queries(*b, max_hits=8)
    for kind in (capi.COLLIDER_BOUNDS, capi.COLLIDER_NONE, 5):
        b = [x.copy() if x is not None else None for x in a]
        b[0][2] = kind
        with pytest.raises(capi.ScTickError, match="a volume's type is SC_TICK_COLLIDER_BOX, _SPHERE or _CAPSULE"):
            t.overlap_queries(*b, max_hits=8)
    with pytest.raises(capi.ScTickError, match="max_hits must be at least 1"):
        t.overlap_queries(*a, max_hits=0)
    with pytest.raises(capi.ScTickError, match="count \\* max_hits does not fit"):
        t.overlap_queries(*a, max_hits=1 << 30)
    with pytest.raises(capi.ScTickError, match="unknown overlap shape mode"):
        t.overlap_queries(*a, max_hits=8, shapes=2)
    # every refused call left the set of eight slots in place
    with pytest.raises(capi.ScTickError, match="needs SC_TICK_BROADPHASE in the same run"):
        t.run(capi.XFORM | capi.OVERLAPS)
    with pytest.raises(capi.ScTickError, match="cannot run with SC_TICK_SPLIT_PAIRS"):
        t.run(FLAGS | capi.SPLIT_PAIRS)
    t.run(FLAGS)
    want = witness(oracle, w.bmin, w.bmax, w, vol, 8)
    compare(t, want)
    assert want[2]["truncated_queries"] == 5
    # NULL buffers give the sizes; a short capacity fills its rows and no more
    info = capi.OverlapInfo()
    assert t.lib.scTickReadOverlapHits(t.ctx, None, None, 0, info) == 1 and (info.queries, info.max_hits, info.hits) == (5, 8, 185)
    counts, ids = np.full(3, 999, U), np.full((3, 8), 999, U)
    assert t.lib.scTickReadOverlapHits(t.ctx, counts.ctypes.data_as(capi.U32P), ids.ctypes.data_as(capi.U32P), 2, None) == 1
    assert list(counts) == [24, 23, 999] and (ids[:2] < oc.LINE).all() and (ids[2] == 999).all()
    t.run(BASE)
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_OVERLAPS"):
        t.overlap_hits()
    t.run(FLAGS)
    t.overlap_queries(*a, max_hits=16)
    with pytest.raises(capi.ScTickError, match="re-sized since the last run"):
        t.overlap_hits()
    t.set_pipelined(True)
    with pytest.raises(capi.ScTickError, match="SC_TICK_OVERLAPS cannot run on a pipelined context"):
        t.run(FLAGS | capi.SPLIT_PAIRS)
    t.set_pipelined(False)
    t.set_tile(0, 1 << 4)
    with pytest.raises(capi.ScTickError, match="SC_TICK_OVERLAPS cannot run on a context with neighbours"):
        t.run(FLAGS | capi.SPLIT_PAIRS)
    t.set_tile(0, 0)
    t.overlap_queries(*[x[:0] if x is not None else None for x in a], max_hits=16)      # count 0 clears the set
    with pytest.raises(capi.ScTickError, match="needs scTickSetOverlapQueries first"):
        t.run(FLAGS)
    t.close()
