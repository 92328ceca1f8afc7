"""Trigger volumes (scTickSetTriggerVolumes, SC_TICK_TRIGGERS) through the C ABI against the witness of tests/trigger_ref.py: the resolve in
numpy fp32, the members from the overlap witness over the resolved volumes, the events as set differences.  Every expected set is exact.
tests/test_triggers_cpu.py proves without a GPU that the cases (tests/trigger_cases.py) are what they claim."""
import numpy as np
import pytest

from sc_gameengine_amd import capi
from sc_gameengine_amd.tick import WorldTick
from tests import overlap_cases as oc, overlap_ref as ref, trigger_cases as tc, trigger_ref as tr, worlds

pytestmark = pytest.mark.gpu
BASE = capi.XFORM | capi.BROADPHASE
FLAGS = BASE | capi.TRIGGERS
AABB, EXACT = capi.OVERLAP_SHAPES_AABB, capi.OVERLAP_SHAPES_EXACT
F = np.float32
U = np.uint32
TWELVE = [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]


def check(t, wt, sets):
    """the last flagged run against the witness for the true member sets of that tick; returns the witness's (entered, exited, info)"""
    ent, exi, info = wt.tick(sets)
    got_info = t.trigger_info()
    assert got_info == info, f"{got_info} != {info}"
    counts, ids = t.trigger_members()
    assert list(counts) == [len(s) for s in sets] and ids.shape == (wt.k, wt.max_members)
    for v, s in enumerate(sets):
        got = ids[v, :min(len(s), wt.max_members)]
        assert len(np.unique(got)) == len(got), v                               # every entity at most once
        if len(s) <= wt.max_members:
            assert np.array_equal(np.sort(got), s), v
        else:
            assert np.isin(got, s).all(), v                                     # max_members distinct members of the true set
    e, x = t.trigger_events()
    for got, full, name in ((e, ent, "entered"), (x, exi, "exited")):
        got = [tuple(p) for p in got.tolist()]
        if len(full) > wt.max_events:                                           # a truncated list: max_events distinct, valid entries
            assert len(got) == wt.max_events == len(set(got)) and set(got) <= set(full), name
        else:
            assert sorted(got) == full, name
    return ent, exi, info


def identity(n):
    return np.tile(np.eye(4, dtype=F).reshape(16), (n, 1))


def box_sets(oracle, w, vol):
    """members over a world of Bounds boxes on unrotated roots at the origin (rc.box_world): the boxes are the world's own bmin / bmax"""
    return tr.members(oracle, w.bmin, w.bmax, w.group, w.mask, identity(w.n), None, vol, w.n)[0]


# ---- 1. resolve -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [AABB, EXACT])
def test_resolved_matrices_match_the_witness_bit_for_bit_and_unanchored_volumes_answer_as_overlap_queries(oracle, shapes):
    w, vol = tc.hierarchy_case()
    k = len(vol["type"])
    ow = worlds.oracle_world(oracle, w, camera=False)
    t = WorldTick.from_world(w, broadphase=True)
    t.trigger_volumes(*tr.args(vol), max_members=64, max_events=256, shapes=shapes)
    none = np.flatnonzero(vol["anchor"] == tc.NONE)
    t.overlap_queries(vol["type"][none], vol["m16"][none], vol["he"][none], vol["radius"][none], vol["hh"][none], vol["mask"][none], max_hits=64, shapes=shapes)
    wt = tr.Witness(k, 64, 256)
    seen = []
    for tick in range(tc.HIERARCHY_TICKS):
        ow.nudge_roots_x(tc.HIERARCHY_NUDGE); t.nudge_roots_x(tc.HIERARCHY_NUDGE)
        ow.transform_system()
        m = ow.world_matrices()[:w.n].copy()
        mn, mx = ow.world_aabbs()
        sets, m16, alive = tr.members(oracle, mn[:w.n], mx[:w.n], w.group, w.mask, m, None, vol, w.n, shapes)
        t.run(FLAGS | capi.OVERLAPS)
        assert np.array_equal(t.world_matrices(), m)
        got = t.trigger_matrices()
        assert alive.all() and np.array_equal(got.view(U), m16.view(U)), tick
        check(t, wt, sets)
        counts, ids = t.overlap_hits()
        for j, v in enumerate(none):
            assert np.array_equal(np.sort(ids[j, :counts[j]]), sets[v]), (tick, v)
        seen.append(m16[:6].copy())
    assert all(not np.array_equal(seen[i], seen[i + 1]) for i in range(3))      # the anchors did move
    t.close(); ow.close()


# ---- 2. the sequence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("shapes", [AABB, EXACT])
def test_a_sequence_of_sixteen_ticks_reports_the_differences_between_consecutive_flagged_ticks(oracle, shapes, graph):
    w, col, steps = tc.sequence_world()
    vol = tc.sequence_volumes(shapes == EXACT)
    per_tick = tc.sequence_sets(oracle, shapes)
    t = WorldTick.from_world(w, broadphase=True)
    col.upload(t)
    t.trigger_volumes(*tr.args(vol), max_members=tc.SEQ_MAX_MEMBERS, max_events=tc.SEQ_MAX_EVENTS, shapes=shapes)
    if graph:
        t.set_graph_mode(True)
    wt = tr.Witness(len(vol["type"]), tc.SEQ_MAX_MEMBERS, tc.SEQ_MAX_EVENTS)
    for tick in range(tc.SEQ_TICKS):
        t.upload_positions(0, steps[tick])
        sets, m16, m = per_tick[tick]
        if tick in tc.SEQ_UNFLAGGED:
            t.run(BASE)
            with pytest.raises(capi.ScTickError, match="did not request SC_TICK_TRIGGERS"):
                t.trigger_info()
            continue
        t.run(FLAGS)
        assert np.array_equal(t.world_matrices(), m)
        assert np.array_equal(t.trigger_matrices().view(U), m16.view(U)), tick
        check(t, wt, sets)
    assert t.learn_ticks() == 1
    t.close()


# ---- 3. row edges -------------------------------------------------------------------------------------------------------------------
def test_rows_of_0_1_63_64_65_max_and_max_plus_one_members(oracle):
    w = oc.line_world()
    mm = tc.EDGE_MAX_MEMBERS
    t = WorldTick.from_world(w, broadphase=True)
    wt = tr.Witness(len(tc.EDGE_COUNTS), mm, 1024)
    first = tc.line_volumes(tc.EDGE_COUNTS)
    t.trigger_volumes(*tr.args(first), max_members=mm, max_events=1024)
    t.run(FLAGS)
    ent, exi, info = check(t, wt, box_sets(oracle, w, first))
    assert info["overflow_volumes"] == 1 and info["resync_volumes"] == 6 and not [p for p in ent if p[0] == 6] and not exi
    counts, ids = t.trigger_members()
    assert counts[6] == mm + 1 and len(np.unique(ids[6])) == mm and (ids[6] <= mm).all()
    nxt = tc.line_volumes(tc.EDGE_NEXT)                                         # the same shape: the memory stays, but for the volume that overflowed
    t.trigger_volumes(*tr.args(nxt), max_members=mm, max_events=1024)
    t.run(FLAGS)
    ent, exi, info = check(t, wt, box_sets(oracle, w, nxt))
    assert info["resync_volumes"] == 1 and info["overflow_volumes"] == 0
    assert ent == [(1, 1), (1, 2)] + [(6, i) for i in range(10)] and exi == [(4, 64)]
    t.run(FLAGS)
    _, _, info = check(t, wt, box_sets(oracle, w, nxt))
    assert (info["entered"], info["exited"], info["resync_volumes"]) == (0, 0, 0)
    assert t.learn_ticks() == 1
    t.close()


def test_rows_of_hundreds_of_members_at_the_row_cap(oracle):
    """max_members at SC_TICK_TRIGGER_MAX_MEMBERS (the largest LDS rows): a volume over the whole mixed world, then over a part of it"""
    w, _ = oc.mixed_world()
    m, mn, mx = tc.state(oracle, w)
    cap = capi.TRIGGER_MAX_MEMBERS
    t = WorldTick.from_world(w, broadphase=True)
    wt = tr.Witness(2, cap, 4096)
    sizes = []
    for lo, hi in (([0, 120], [256, 256]), ([100, 0], [256, 256]), ([0, 0], [256, 180])):
        vol = tc.unanchored(oc.box_volumes(F([[lo[0], -50, lo[1]], [90, -50, 90]]), F([[hi[0], 50, hi[1]], [150, 50, 150]])))
        sets = tr.members(oracle, mn, mx, w.group, w.mask, m, None, vol, w.n)[0]
        t.trigger_volumes(*tr.args(vol), max_members=cap, max_events=4096)
        t.run(FLAGS)
        ent, exi, _ = check(t, wt, sets)
        sizes.append((len(sets[0]), len(ent), len(exi)))
    assert all(n > 256 for n, _, _ in sizes) and all(e > 64 and x > 64 for _, e, x in sizes[1:])      # several chunks a side, both ways
    t.close()


# ---- 4. one entity, one member, whatever record reports it ---------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_an_entity_reported_from_another_sector_neither_leaves_nor_enters(oracle, graph):
    w = tc.reporter_world()
    t = WorldTick.from_world(w, broadphase=True, max_pairs=1 << 12)
    t.trigger_volumes(*tr.args(tc.reporter_volume(tc.CORNERS[0])), max_members=128, max_events=256)
    if graph:
        t.set_graph_mode(True)
    wt = tr.Witness(1, 128, 256)
    for tick, corner in enumerate(tc.CORNERS):
        vol = tc.reporter_volume(corner)
        t.trigger_volumes(*tr.args(vol), max_members=128, max_events=256)
        t.run(FLAGS)
        ent, exi, info = check(t, wt, box_sets(oracle, w, vol))
        c = t.counts()
        assert c.bin_overflow >= 26 and c.big_boxes == 1                        # the crowd spills into the overflow list, the plate is in the big list
        if tick:
            moved = {i for _, i in ent + exi}
            assert not moved & {tc.STRADDLER, tc.PLATE} and (tc.SPILLED in moved) == (tick in (3, 5))
    t.close()


# ---- 5. the event cap ---------------------------------------------------------------------------------------------------------------
def test_ten_entries_for_four_slots_report_the_true_totals_and_four_of_them(oracle):
    w = oc.line_world()
    t = WorldTick.from_world(w, broadphase=True)
    wt = tr.Witness(2, 64, tc.CAP_EVENTS)
    steps = (([0, 30], [9, 33], (14, 0, 1)),                # ten entries in one volume, four in the other: four slots
             ([2, 30], [11, 33], (2, 2, 0)),                # the next tick's events are right
             ([2, 30], [11, 37], (4, 0, 0)),                # exactly max_events: complete
             ([20, 30], [24, 30], (5, 17, 1)))              # ... and the exits are capped alike
    for first, last, want in steps:
        vol = tc.span_volumes(first, last)
        t.trigger_volumes(*tr.args(vol), max_members=64, max_events=tc.CAP_EVENTS)
        t.run(FLAGS)
        _, _, info = check(t, wt, box_sets(oracle, w, vol))
        assert (info["entered"], info["exited"], info["events_truncated"]) == want
    t.close()


# ---- 6. residency -------------------------------------------------------------------------------------------------------------------
def test_anchors_follow_a_removal_and_every_volume_resyncs_behind_it(oracle):
    w, vol, removal = tc.residency_case()
    k = len(vol["type"])
    t = WorldTick.from_world(w, broadphase=True, capacity=w.n + 4)
    t.trigger_volumes(*tr.args(vol), max_members=32, max_events=256)
    wt = tr.Witness(k, 32, 256)

    def sets_of(world, volumes):
        m, mn, mx = tc.state(oracle, world)
        return tr.members(oracle, mn, mx, world.group, world.mask, m, None, volumes, world.n)[0]

    for _ in range(2):
        t.run(FLAGS)
        check(t, wt, sets_of(w, vol))
    assert list(t.trigger_anchors()) == list(vol["anchor"])
    src, dst = t.remove_entities(removal)
    after, renamed = tc.swap_remove(w, removal)
    assert dict(zip(src.tolist(), dst.tolist())) == {15: 13, 14: 2}
    moved = dict(vol, anchor=U([12, tr.DEAD, 13, 13, tc.NONE]))
    assert list(t.trigger_anchors()) == list(moved["anchor"])
    wt.forget()
    t.run(FLAGS)
    sets = sets_of(after, moved)
    _, _, info = check(t, wt, sets)
    assert info["resync_volumes"] == k and len(sets[1]) == 0 and 13 not in sets[2] and 13 in sets[3]      # dead: no members; skip_self follows the rename
    dead = t.trigger_matrices()[1]
    assert (dead[TWELVE].view(U) == 0x7FC00000).all()
    # an append forces no resync: the new box enters the world-space volume, nothing else happens
    first = t.append_entities([[30, 0, 30.5]], [[0, 0, 0]], [[1, 1, 1]], bmin=[[-0.25] * 3], bmax=[[0.25] * 3], group=[1], mask=[0xFFFFFFFF])
    assert first == after.n
    grown = tc.world(np.concatenate([after.pos, [[30, 0, 30.5]]]), half=0.25)
    t.run(FLAGS)
    ent, exi, info = check(t, wt, sets_of(grown, moved))
    assert info["resync_volumes"] == 0 and (4, first) in ent and not exi
    # a shrinking count forgets every row
    t.set_count(after.n)
    wt.forget()
    t.run(FLAGS)
    _, _, info = check(t, wt, sets_of(after, moved))
    assert info["resync_volumes"] == k
    # so does another rank: ids are renamed
    t.set_tile(3, 0)
    wt.forget()
    t.run(FLAGS)
    m, mn, mx = tc.state(oracle, after)
    ranked = tr.members(oracle, mn, mx, after.group, after.mask, m, None, moved, after.n, 0, rank=3)[0]
    _, _, info = check(t, wt, ranked)
    assert info["resync_volumes"] == k and all((s >> 24 == 3).all() for s in ranked)
    t.close()


# ---- 7. a same-shape rewrite keeps the memory: an eager and a graph-mode context side by side ----------------------------------------
def test_a_zone_moved_by_a_rewrite_yields_ordinary_events_under_graph_replay(oracle):
    w = oc.line_world()
    twins = [WorldTick.from_world(w, broadphase=True) for _ in range(2)]
    twins[1].set_graph_mode(True)
    wts = [tr.Witness(2, 16, 64) for _ in twins]
    spans = [([0, 40], [5, 45]), ([2, 40], [7, 45]), ([4, 41], [9, 45]), ([4, 41], [9, 45]), ([10, 30], [14, 40]), ([12, 30], [15, 40])]
    for step, (first, last) in enumerate(spans):
        vol = tc.span_volumes(first, last)
        sets = box_sets(oracle, w, vol)
        learn = [t.learn_ticks() for t in twins]
        reports = []
        for t, wt in zip(twins, wts):
            t.trigger_volumes(*tr.args(vol), max_members=16, max_events=64)
            t.run(FLAGS)
            ent, exi, info = check(t, wt, sets)
            reports.append((ent, exi, info))
            assert info["resync_volumes"] == (2 if step == 0 else 0)
            assert step == 0 or step == 3 or (len(ent) >= 1 and len(exi) >= 1)  # a moved zone: ordinary entries and exits
        assert reports[0] == reports[1]
        assert [t.learn_ticks() - l for t, l in zip(twins, learn)] == [1 if step == 0 else 0] * 2
    # a re-sizing call forgets: other max_events, then another mode, then another count
    for kwargs, count in ((dict(max_members=16, max_events=32), 2), (dict(max_members=16, max_events=32, shapes=EXACT), 2), (dict(max_members=16, max_events=32, shapes=EXACT), 1)):
        vol = tr.take(tc.span_volumes(*spans[-1]), np.arange(count))
        sets = box_sets(oracle, w, vol)
        for i, t in enumerate(twins):
            t.trigger_volumes(*tr.args(vol), **kwargs)
            wts[i] = tr.Witness(count, 16, 32)
            for _ in range(3):                                                  # a fresh capture, then both parities replayed
                t.run(FLAGS)
                _, _, info = check(t, wts[i], sets)
            assert info["resync_volumes"] == 0 and info["entered"] == 0
    for t in twins:
        t.close()


# ---- 8. volume counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", tc.VOLUME_COUNTS)
def test_volume_counts_that_leave_waves_without_a_volume(oracle, count):
    w, col, steps = tc.sequence_world()
    base = tc.sequence_volumes(False)
    vol, idx = tc.tiled(base, count)
    per_tick = tc.sequence_sets(oracle, AABB)
    t = WorldTick.from_world(w, broadphase=True)
    col.upload(t)
    t.trigger_volumes(*tr.args(vol), max_members=tc.SEQ_MAX_MEMBERS, max_events=1 << 16)
    if count == 5:
        t.set_graph_mode(True)
    wt = tr.Witness(count, tc.SEQ_MAX_MEMBERS, 1 << 16)
    for tick in (0, 1, 2):
        t.upload_positions(0, steps[tick])
        t.run(FLAGS)
        check(t, wt, [per_tick[tick][0][i] for i in idx])
    t.close()


# ---- 9. a world that cannot pair ----------------------------------------------------------------------------------------------------
def test_quiet_ticks_stay_quiet_around_a_flagged_tick(oracle):
    w, col, vol = tc.quiet_case()
    m, mn, mx = tc.state(oracle, w, col)
    sets = tr.members(oracle, mn, mx, w.group, w.mask, m, col, vol, w.n, EXACT)[0]
    t = WorldTick.from_world(w, broadphase=True)
    col.upload(t)
    t.trigger_volumes(*tr.args(vol), max_members=tc.SEQ_MAX_MEMBERS, max_events=tc.SEQ_MAX_EVENTS, shapes=EXACT)
    wt = tr.Witness(len(vol["type"]), tc.SEQ_MAX_MEMBERS, tc.SEQ_MAX_EVENTS)
    t.run(BASE)                                             # the learn tick
    for _ in range(3):
        t.run(BASE)
        assert t.bin_stats()["quiet_last_tick"]
    carry = t.carry_stats()
    for _ in range(2):
        t.run(FLAGS)
        assert not t.bin_stats()["quiet_last_tick"] and not t.bin_stats()["lazy_last_tick"]
        check(t, wt, sets)
        t.run(BASE)
        assert t.bin_stats()["quiet_last_tick"]
    assert t.learn_ticks() == 1 and t.carry_stats() == carry
    t.close()


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------
def test_every_refusal_has_its_text(oracle):
    w = oc.line_world()
    vol = tc.span_volumes([0, 5], [9, 20])
    a = list(tr.args(vol))
    t = WorldTick.from_world(w, broadphase=True)
    with pytest.raises(capi.ScTickError, match="needs scTickSetTriggerVolumes first"):
        t.run(FLAGS)
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_TRIGGERS"):
        t.trigger_members()
    t.trigger_volumes(*a, max_members=8, max_events=8)
    for at, value in ((2, np.nan), (4, np.inf), (3, np.nan), (5, -np.inf)):
        b = [x.copy() for x in a]
        b[at].reshape(-1)[1] = value
        with pytest.raises(capi.ScTickError, match="must be finite"):
            t.trigger_volumes(*b, max_members=8, max_events=8)
    for kind in (capi.COLLIDER_BOUNDS, capi.COLLIDER_NONE, 5):
        b = [x.copy() for x in a]
        b[1][1] = kind
        with pytest.raises(capi.ScTickError, match="a volume's type is SC_TICK_COLLIDER_BOX, _SPHERE or _CAPSULE"):
            t.trigger_volumes(*b, max_members=8, max_events=8)
    with pytest.raises(capi.ScTickError, match="max_members must be at least 1"):
        t.trigger_volumes(*a, max_members=0, max_events=8)
    with pytest.raises(capi.ScTickError, match="exceeds SC_TICK_TRIGGER_MAX_MEMBERS"):
        t.trigger_volumes(*a, max_members=capi.TRIGGER_MAX_MEMBERS + 1, max_events=8)
    with pytest.raises(capi.ScTickError, match="unknown shape mode"):
        t.trigger_volumes(*a, max_members=8, max_events=8, shapes=2)
    null = [None if i == 2 else x.ctypes.data_as(p) for i, (x, p) in enumerate(zip(a, (capi.U32P, capi.U8P, capi.F32P, capi.F32P, capi.F32P, capi.F32P, capi.U32P, capi.U8P)))]
    assert t.lib.scTickSetTriggerVolumes(t.ctx, 2, *null, 8, 8, 0) == 0 and "null argument" in t.lib.scTickGetLastError(t.ctx).decode()
    full = [x.ctypes.data_as(p) for x, p in zip(a, (capi.U32P, capi.U8P, capi.F32P, capi.F32P, capi.F32P, capi.F32P, capi.U32P, capi.U8P))]
    # (refused on the sizes alone, before an array is read)
    assert t.lib.scTickSetTriggerVolumes(t.ctx, (1 << 20) + 1, *full, 1024, 8, 0) == 0 and "count * max_members does not fit" in t.lib.scTickGetLastError(t.ctx).decode()
    # every refused call left the set of eight slots in place
    with pytest.raises(capi.ScTickError, match="SC_TICK_TRIGGERS needs SC_TICK_BROADPHASE in the same run"):
        t.run(capi.XFORM | capi.TRIGGERS)
    with pytest.raises(capi.ScTickError, match="SC_TICK_TRIGGERS cannot run with SC_TICK_SPLIT_PAIRS"):
        t.run(FLAGS | capi.SPLIT_PAIRS)
    t.run(FLAGS)
    wt = tr.Witness(2, 8, 8)
    _, _, info = check(t, wt, box_sets(oracle, w, vol))
    assert info["overflow_volumes"] == 2 and info["entered"] == 0
    # NULL buffers give the sizes; a short capacity fills its rows and no more
    raw = capi.TriggerInfo()
    assert t.lib.scTickReadTriggerEvents(t.ctx, None, 0, None, 0, raw) == 1 and (raw.volumes, raw.max_members, raw.members) == (2, 8, 26)
    counts, ids = np.full(2, 999, U), np.full((2, 8), 999, U)
    assert t.lib.scTickReadTriggerMembers(t.ctx, counts.ctypes.data_as(capi.U32P), ids.ctypes.data_as(capi.U32P), 1, None) == 1
    assert list(counts) == [10, 999] and (ids[0] < 10).all() and (ids[1] == 999).all()
    m = np.zeros((3, 16), F)
    assert t.lib.scTickReadTriggerMatrices(t.ctx, 1, 2, m.ctypes.data_as(capi.F32P)) == 0 and "range exceeds" in t.lib.scTickGetLastError(t.ctx).decode()
    # a split flow in flight refuses the setter
    t.run(BASE | capi.SPLIT_PAIRS)
    with pytest.raises(capi.ScTickError, match="scTickRunPairs is pending"):
        t.trigger_volumes(*a, max_members=8, max_events=8)
    t.run_pairs()
    for read in (t.trigger_members, t.trigger_events, t.trigger_matrices, t.trigger_info):
        with pytest.raises(capi.ScTickError, match="did not request SC_TICK_TRIGGERS"):
            read()
    assert list(t.trigger_anchors()) == [tc.NONE, tc.NONE]                       # host-side: needs no run
    t.run(FLAGS)
    t.trigger_volumes(*a, max_members=16, max_events=8)
    with pytest.raises(capi.ScTickError, match="re-sized since the last run"):
        t.trigger_members()
    t.set_pipelined(True)
    with pytest.raises(capi.ScTickError, match="SC_TICK_TRIGGERS cannot run on a pipelined context"):
        t.run(FLAGS | capi.SPLIT_PAIRS)
    t.set_pipelined(False)
    t.set_tile(0, 1 << 4)
    with pytest.raises(capi.ScTickError, match="SC_TICK_TRIGGERS cannot run on a context with neighbours"):
        t.run(FLAGS | capi.SPLIT_PAIRS)
    t.set_tile(0, 0)
    t.trigger_volumes(*[x[:0] for x in a], max_members=16, max_events=8)         # count 0 clears the set
    with pytest.raises(capi.ScTickError, match="needs scTickSetTriggerVolumes first"):
        t.run(FLAGS)
    t.close()
