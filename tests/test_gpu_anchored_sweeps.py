"""Entity-anchored capsule sweeps (scTickSetAnchoredSweeps, SC_TICK_ANCHORED_SWEEPS) through the C ABI against the witness of
tests/anchored_sweeps_ref.py: the resolve of tests/anchored_ref.py, then the plain sweeps' witnesses over the resolved segments.  The GPU's
matrices and boxes equal the oracle's / the collider witness's as IEEE values, so hits, statuses and resolved segments must be equal as
bit patterns, misses included, and the EXACT report's words equal.  tests/test_anchored_sweeps_cpu.py proves without a GPU that the
cases of tests/anchored_sweep_cases.py are what they claim."""
import numpy as np
import pytest

from sc_gameengine_amd import capi
from sc_gameengine_amd.tick import WorldTick
from tests import anchored_sweep_cases as ac, ray_walk_cases as rc, sweep_ref, sweep_shapes_cases as sc, trigger_cases as tc, worlds
from tests.test_gpu_shape_rays import same_world
from tests.test_gpu_sweeps import compare as compare_plain

pytestmark = pytest.mark.gpu
BASE = capi.XFORM | capi.BROADPHASE | capi.DENSE_AABBS
FLAGS = BASE | capi.ANCHORED_SWEEPS
F = np.float32
U = np.uint32
AABB, EXACT = capi.SWEEP_SHAPES_AABB, capi.SWEEP_SHAPES_EXACT
MODES = (AABB, EXACT)


def start(oracle, w, col, mode, **kw):
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    t = WorldTick.from_world(w, broadphase=True, **kw)
    if col is not None:
        col.upload(t)
    t.set_sweep_shapes(mode)
    return t, ow


def same_hits(got, want):
    assert len(got) == len(want)
    for f in ("hit", "id", "layer", "pad"):
        assert np.array_equal(got[f], want[f]), f"{f}: {np.flatnonzero(got[f] != want[f])[:8]}"
    for f in ("distance", "travel", "position", "normal"):
        assert np.array_equal(got[f].view(U), want[f].view(U)), f                # bit patterns, misses included


def check(t, want, mode):
    """the last flagged run against a witness answer (hits, segments, report)"""
    hits, (s, e), info = want
    same_hits(t.anchored_sweep_hits(), hits)
    gs, ge = t.anchored_sweep_segments()
    assert np.array_equal(gs.view(U), s.view(U)) and np.array_equal(ge.view(U), e.view(U))
    if mode == EXACT:
        assert t.anchored_sweep_shape_info() == info, (t.anchored_sweep_shape_info(), info)
    else:
        with pytest.raises(capi.ScTickError, match="SC_TICK_SWEEP_SHAPES_AABB mode"):
            t.anchored_sweep_shape_info()


def expect(oracle, t, ow, w, col, q, mode):
    """the witness over the oracle's matrices and the witness boxes, which the GPU's must equal"""
    if col is not None:
        m, mn, mx = same_world(t, ow, w, col)
    else:
        m = ow.world_matrices()[:w.n]
        mn, mx = ow.world_aabbs()
        mn, mx = mn[:w.n], mx[:w.n]
        assert np.array_equal(t.world_matrices(), m)
    return ac.witness(oracle, m, mn, mx, w.group[:w.n], w.mask[:w.n], col, q, mode)


# ---- 1. both frames, both modes, with the transform stage in the run and without it ------------------------------------------------
@pytest.mark.parametrize("xform", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_the_table_in_both_frames_and_modes_with_and_without_the_transform_stage(oracle, mode, xform):
    """500 sweeps across 1 200 entities: hits, misses, starts in overlap, zero-length sweeps and every status, on the learn tick and on the
    home slots.  Without SC_TICK_XFORM the sweeps resolve against the matrices scTickUploadWorldMatrices left."""
    w, col, q = ac.table(oracle)
    t, ow = start(oracle, w, col, mode)
    t.anchored_sweeps(*ac.args(q))
    for _ in range(2):
        t.run(FLAGS)
        same_world(t, ow, w, col)
        check(t, ac.table_answers(oracle, mode), mode)
    ow.nudge_roots_x(0.7)
    ow.transform_system()
    if xform:
        t.nudge_roots_x(0.7)
        t.run(FLAGS)
        want = expect(oracle, t, ow, w, col, q, mode)
    else:
        m = ow.world_matrices()[:w.n].copy()
        t.upload_world_matrices(0, m)
        t.run(FLAGS & ~capi.XFORM)
        assert np.array_equal(t.world_matrices().view(U), m.view(U))
        mn, mx = t.world_aabbs()                                                # (the boxes of a run without the transform stage: as the library keeps them)
        old, new = ac.table_state(oracle)[1:], col.witness(ow, w.n)
        assert any(np.array_equal(mn, b[0]) and np.array_equal(mx, b[1]) for b in (old, new))
        want = ac.witness(oracle, m, mn, mx, w.group, w.mask, col, q, mode)
    check(t, want, mode)
    before = ac.table_answers(oracle, mode)
    both = (before[0]["hit"] == 1) & (want[0]["hit"] == 1) & (q["anchor"] != ac.NONE)
    assert (before[1][0][both] != want[1][0][both]).any(axis=1).sum() > 100      # the segments moved with their anchors
    assert not xform or t.learn_ticks() == 1
    t.close(); ow.close()


# ---- 2. sweep counts on either side of a workgroup's four waves, and one past 4 096 --------------------------------------------------
@pytest.mark.parametrize("count", ac.COUNTS)
@pytest.mark.parametrize("mode", MODES)
def test_sweep_counts_that_leave_waves_without_a_sweep(oracle, mode, count):
    w, col, q = ac.table(oracle)
    tiled, idx = ac.tiled(q, count)
    hits, (s, e), info = ac.table_answers(oracle, mode)
    if mode == EXACT:                                                           # the report: whole copies of the table plus the rows of the last, partial one
        m, mn, mx = ac.table_state(oracle)
        rest = ac.witness(oracle, m, mn, mx, w.group, w.mask, col, ac.take(q, idx[:count % 500]), mode)[2] if count % 500 else dict.fromkeys(info, 0)
        info = {k: (count // 500) * info[k] + rest[k] for k in info}
    t, ow = start(oracle, w, col, mode)
    t.anchored_sweeps(*ac.args(tiled))
    if count == 5:
        t.set_graph_mode(True)
    for _ in range(3):
        t.run(FLAGS)
        check(t, (hits[idx], (s[idx], e[idx]), info), mode)
    assert len(t.anchored_sweep_hits()) == count == len(t.anchored_sweep_anchors())
    t.close(); ow.close()


# ---- 3. an unanchored set and the same arrays as a plain set, in one run -------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_an_unanchored_set_answers_as_the_plain_sweeps_of_the_same_run(oracle, mode):
    w, col, _ = ac.table(oracle)
    _, _, (a, b, radius, hh, mask, _) = sc.world_case(oracle)
    m, mn, mx = ac.table_state(oracle)
    t, ow = start(oracle, w, col, mode)
    t.set_sweep_queries(a, b, radius, hh, mask)
    t.anchored_sweeps(*ac.args(ac.unanchored(a, b, radius, hh, mask)))
    t.run(FLAGS | capi.SWEEPS)
    same_world(t, ow, w, col)
    plain = t.sweep_hits()
    assert t.anchored_sweep_hits().tobytes() == plain.tobytes()
    want = ac.witness(oracle, m, mn, mx, w.group, w.mask, col, ac.unanchored(a, b, radius, hh, mask), mode)
    check(t, want, mode)
    compare_plain(plain, want[0])
    # the two reports are separate: the anchored set cut to its first 200 rows, the plain one whole
    half = ac.unanchored(a[:200], b[:200], radius[:200], hh[:200], mask[:200])
    t.anchored_sweeps(*ac.args(half))
    t.run(FLAGS | capi.SWEEPS)
    assert t.anchored_sweep_hits().tobytes() == t.sweep_hits()[:200].tobytes() and t.sweep_hits().tobytes() == plain.tobytes()
    cut = ac.witness(oracle, m, mn, mx, w.group, w.mask, col, half, mode)
    check(t, cut, mode)
    if mode == EXACT:
        assert t.sweep_shape_info() == want[2] and want[2]["refined"] > cut[2]["refined"] > 20
    else:
        with pytest.raises(capi.ScTickError, match="SC_TICK_SWEEP_SHAPES_AABB mode"):
            t.sweep_shape_info()
    t.close(); ow.close()


# ---- 4. skip_self --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_the_anchors_own_box_answers_at_once_unless_it_is_skipped(oracle, mode):
    w, col, q = ac.table(oracle)
    own = ac.take(q, np.arange(500)[ac.OWN_ROWS])
    t, ow = start(oracle, w, col, mode)
    t.anchored_sweeps(*ac.args(own))
    t.run(FLAGS)
    got = t.anchored_sweep_hits()
    check(t, expect(oracle, t, ow, w, col, own, mode), mode)
    assert (got["hit"] == 1).all() and (got["travel"] == 0).all() and np.array_equal(got["id"], own["anchor"])
    learn = t.learn_ticks()
    blind = dict(own, skip_self=np.ones(20, np.uint8))
    t.anchored_sweeps(*ac.args(blind))
    t.run(FLAGS)
    check(t, expect(oracle, t, ow, w, col, blind, mode), mode)
    assert (t.anchored_sweep_hits()["id"] != own["anchor"]).all() and t.learn_ticks() == learn
    t.close(); ow.close()


# ---- 5. every status -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_every_status_a_shrunk_count_and_a_matrix_that_holds_a_nan(oracle, mode):
    w, q, _ = ac.residency_case()
    t, ow = start(oracle, w, None, mode)
    t.anchored_sweeps(*ac.args(q))
    t.run(FLAGS)
    want = expect(oracle, t, ow, w, None, q, mode)
    check(t, want, mode)
    assert (want[0]["pad"] == 0).all() and (want[0]["hit"] == 1).all()
    # the count shrinks under live anchors: 14 and 15 are beyond it; regrown, they answer again
    t.set_count(14)
    t.run(FLAGS)
    m, (mn, mx) = ow.world_matrices()[:14], ow.world_aabbs()
    cut = ac.witness(oracle, m, mn[:14], mx[:14], w.group[:14], w.mask[:14], None, q, mode)
    check(t, cut, mode)
    assert list(cut[0]["pad"]) == [0, 0, 1, 1, 1, 0] and list(t.anchored_sweep_anchors()) == list(q["anchor"])      # the anchors are left alone
    t.set_count(w.n)
    t.run(FLAGS)
    check(t, want, mode)
    # an anchor at the count, beyond it, dead; an overflowing squared length
    odd = ac.sweeps([w.n, w.n + 1000, ac.DEAD, 12, ac.NONE], [[0, 0, 0]] * 4 + [[3e38, 0, 0]], [[0, 0, -6]] * 3 + [[3e30, 0, 0], [3e38, 0, 0]], 0.3, 0.4,
                    end_frame=[0, 1, 0, 0, 1])
    t.anchored_sweeps(*ac.args(odd))
    t.run(FLAGS)
    res = expect(oracle, t, ow, w, None, odd, mode)
    check(t, res, mode)
    assert list(res[0]["pad"]) == [1, 1, 1, 2, 2]
    # an uploaded matrix with a NaN, in a run without the transform stage: its sweeps are not finite, the others answer as before
    t.anchored_sweeps(*ac.args(q))
    bad = ow.world_matrices()[:w.n].copy()
    bad[12, 5] = np.nan
    t.upload_world_matrices(12, bad[12:13])
    t.run(FLAGS & ~capi.XFORM)
    assert np.array_equal(t.world_matrices(), bad, equal_nan=True) and np.isnan(t.world_matrices()[12, 5])
    mn, mx = t.world_aabbs()
    nan = ac.witness(oracle, bad, mn, mx, w.group, w.mask, None, q, mode)
    check(t, nan, mode)
    assert list(nan[0]["pad"]) == [2, 0, 0, 0, 0, 0] and nan[0][1:].tobytes() == want[0][1:].tobytes()
    t.close(); ow.close()


# ---- 6. four ticks of moving anchors with nothing between them but the run -----------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_four_ticks_of_moving_anchors_follow_the_oracle_without_a_learn_tick(oracle, mode):
    w, col, q = ac.table(oracle)
    t, ow = start(oracle, w, col, mode)
    t.anchored_sweeps(*ac.args(q))
    t.set_frame_producer(1, 0.5)                                                # the root nudge, applied at the end of every run on the device
    t.run(FLAGS | capi.PRODUCE_NEXT)
    learn, seen = t.learn_ticks(), []
    for tick in range(4):
        ow.nudge_roots_x(0.5)                                                   # what the producer did at the end of the last run
        ow.transform_system()
        t.run(FLAGS | capi.PRODUCE_NEXT)
        want = expect(oracle, t, ow, w, col, q, mode)
        check(t, want, mode)
        seen.append(want)
    assert t.learn_ticks() == learn == 1
    on = (q["anchor"] != ac.NONE) & (seen[0][0]["pad"] == 0)
    assert (seen[0][1][0][on] != seen[3][1][0][on]).any(axis=1).all()            # every anchored start moved
    assert (seen[0][0]["id"] != seen[3][0]["id"]).sum() > 5
    t.close(); ow.close()


# ---- 7. residency --------------------------------------------------------------------------------------------------------------------
def test_anchors_follow_a_removal(oracle):
    w, q, removal = ac.residency_case()
    t, ow = start(oracle, w, None, AABB, capacity=w.n + 4)
    t.anchored_sweeps(*ac.args(q))
    t.run(FLAGS)
    check(t, expect(oracle, t, ow, w, None, q, AABB), AABB)
    assert list(t.anchored_sweep_anchors()) == list(q["anchor"])
    src, dst = t.remove_entities(removal)
    after, names = tc.swap_remove(w, removal)
    assert dict(zip(src.tolist(), dst.tolist())) == {15: 13, 14: 2}
    moved = ac.renamed(q, names)
    assert list(t.anchored_sweep_anchors()) == list(moved["anchor"]) == [12, ac.DEAD, 13, 13, 2, ac.NONE]
    t.run(FLAGS)
    m, mn, mx = tc.state(oracle, after)
    assert np.array_equal(t.world_matrices(), m)
    want = ac.witness(oracle, m, mn, mx, after.group, after.mask, None, moved)
    check(t, want, AABB)
    assert list(want[0]["pad"]) == [0, 1, 0, 0, 0, 0] and want[0]["id"][3] == 13 and want[0]["id"][2] != 13
    # an append leaves the anchors alone
    first = t.append_entities([[30, 0, 30.5]], [[0, 0, 0]], [[1, 1, 1]], bmin=[[-0.25] * 3], bmax=[[0.25] * 3], group=[1], mask=[0xFFFFFFFF])
    assert first == after.n and list(t.anchored_sweep_anchors()) == list(moved["anchor"])
    t.close(); ow.close()


# ---- 8. the graph twin ---------------------------------------------------------------------------------------------------------------
def test_an_eager_and_a_graph_context_agree_after_every_tick_and_every_setter(oracle):
    """Both parities captured and replayed; a same-count rewrite between replays shows in the next replay and costs no learn tick; a
    re-size re-captures; scTickSetSweepShapes toggled between captures."""
    w, col, q = ac.table(oracle)
    sets = [ac.take(q, np.arange(0, 120)), ac.take(q, np.arange(300, 420)), ac.take(q, np.arange(100, 170))]
    twins = [WorldTick.from_world(w, broadphase=True) for _ in range(2)]
    ow = worlds.oracle_world(oracle, w, camera=False)
    for t in twins:
        col.upload(t)
        t.set_frame_producer(1, 0.25)
        t.anchored_sweeps(*ac.args(sets[0]))
    twins[1].set_graph_mode(True)
    steps = [("run", 5), ("set", 1), ("run", 3), ("mode", EXACT), ("run", 5), ("set", 0), ("run", 3), ("set", 2), ("run", 5), ("mode", AABB), ("run", 3)]
    cur, mode, ticks = sets[0], AABB, 0
    learn = [t.learn_ticks() for t in twins]
    for what, arg in steps:
        if what == "set":
            cur = sets[arg]
            resize = len(cur["anchor"]) != len(twins[0].anchored_sweep_anchors())
            before = [t.learn_ticks() for t in twins]
            for t in twins:
                t.anchored_sweeps(*ac.args(cur))
        elif what == "mode":
            mode = arg
            for t in twins:
                t.set_sweep_shapes(mode)
        else:
            for k in range(arg):
                ow.transform_system()
                for t in twins:
                    t.run(FLAGS | capi.PRODUCE_NEXT)
                a, b = twins
                assert a.anchored_sweep_hits().tobytes() == b.anchored_sweep_hits().tobytes()
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a.anchored_sweep_segments(), b.anchored_sweep_segments()))
                assert np.array_equal(a.world_matrices(), b.world_matrices()) and a.pairs()[1] == b.pairs()[1]
                if mode == EXACT:
                    assert a.anchored_sweep_shape_info() == b.anchored_sweep_shape_info()
                if k == arg - 1:                                                # the last tick of a phase: against the witness
                    check(b, expect(oracle, b, ow, w, col, cur, mode), mode)
                ow.nudge_roots_x(0.25)
                ticks += 1
            if ticks > 5:                                                       # a same-count rewrite and a mode change cost no learn tick, a re-size costs one
                assert [t.learn_ticks() - l for t, l in zip(twins, before)] == [1 if resize else 0] * 2
    assert [t.learn_ticks() for t in twins] == [learn[0] + 2] * 2               # the first tick's and the re-size's
    for t in twins:
        t.close()
    ow.close()


# ---- 9. the sector walk at its edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["world", "translated"])
@pytest.mark.parametrize("kind,where", [("edge", "near"), ("edge", "far"), ("zero", "near"), ("zero", "far"), ("crowded", "near")])
def test_the_walk_rows_through_the_anchored_path(oracle, kind, where, family):
    """the sweep rows of tests/ray_walk_cases.py -- the grown box met at travel == far on a sector boundary and the neighbour one ulp
    short; overlap tests on the closed face of a grown box in the next sector; a sector whose records spill into the overflow list --
    once in world space and once in a translated anchor's frame"""
    w, rows, role = ac.walk_rows(kind, where)
    none, moved, w2, keep = ac.walk_sets(w, rows)
    want = sweep_ref.sweep_boxes(oracle, w.bmin, w.bmax, w.group, w.mask, *rows)
    q, src = none, rows
    if family == "translated":
        w, q, want, role, src = w2, moved, want[keep], role[keep], tuple(x[keep] for x in rows)
    t = WorldTick.from_world(w, broadphase=True, max_pairs=1 << 12 if kind == "crowded" else 0)
    t.anchored_sweeps(*ac.args(q))
    for _ in range(2):                                                          # the learn tick and one on the home slots
        t.run(FLAGS)
        got = t.anchored_sweep_hits()
        same_hits(got, want)
        s, e = t.anchored_sweep_segments()
        assert np.array_equal(s.view(U), src[0].view(U)) and np.array_equal(e.view(U), src[1].view(U))
    assert (got["hit"][role >= 1] == 1).all() and (got["hit"][role == 0] == 0).all() and (role >= 1).sum() >= 20
    assert kind != "crowded" or t.counts().bin_overflow == 26
    t.close()


# ---- 10. refusals, and a context that never sets ------------------------------------------------------------------------------------
def test_every_refusal_has_its_text_and_leaves_the_previous_set_answering(oracle):
    w, q, _ = ac.residency_case()
    t, ow = start(oracle, w, None, AABB)
    with pytest.raises(capi.ScTickError, match="needs scTickSetAnchoredSweeps first"):
        t.run(FLAGS)
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_ANCHORED_SWEEPS"):
        t.anchored_sweep_hits()
    a = list(ac.args(q))
    t.anchored_sweeps(*a)
    t.run(FLAGS)
    want = expect(oracle, t, ow, w, None, q, AABB)
    check(t, want, AABB)
    learn = t.learn_ticks()
    for at, value in ((1, np.nan), (2, np.inf), (3, np.nan), (4, -np.inf)):
        b = [x.copy() for x in a]
        b[at].reshape(-1)[1] = value
        with pytest.raises(capi.ScTickError, match="must be finite"):
            t.anchored_sweeps(*b)
    b = [x.copy() for x in a]; b[3][2] = -0.5
    with pytest.raises(capi.ScTickError, match="radius must be >= 0"):
        t.anchored_sweeps(*b)
    b = [x.copy() for x in a]; b[7][0] = 2
    with pytest.raises(capi.ScTickError, match="end_frame is SC_TICK_SWEEP_END_LOCAL or SC_TICK_SWEEP_END_WORLD_OFFSET"):
        t.anchored_sweeps(*b)
    kinds = (capi.U32P, capi.F32P, capi.F32P, capi.F32P, capi.F32P, capi.U32P, capi.U8P, capi.U8P)
    for missing in range(6):
        null = [None if i == missing else x.ctypes.data_as(p) for i, (x, p) in enumerate(zip(a, kinds))]
        assert t.lib.scTickSetAnchoredSweeps(t.ctx, len(a[0]), *null) == 0 and "null argument" in t.lib.scTickGetLastError(t.ctx).decode()
    with pytest.raises(capi.ScTickError, match="SC_TICK_ANCHORED_SWEEPS needs SC_TICK_BROADPHASE in the same run"):
        t.run(capi.XFORM | capi.ANCHORED_SWEEPS)
    with pytest.raises(capi.ScTickError, match="SC_TICK_ANCHORED_SWEEPS cannot run with SC_TICK_SPLIT_PAIRS"):
        t.run(FLAGS | capi.SPLIT_PAIRS)
    check(t, want, AABB)                                                        # refused runs and set calls changed nothing ...
    t.run(FLAGS)
    check(t, want, AABB)                                                        # ... and the previous set still answers
    assert t.learn_ticks() == learn
    # NULL optional arrays: every sweep skips its anchor and ends at a local point
    full = [x.ctypes.data_as(p) for x, p in zip(a, kinds)]
    assert t.lib.scTickSetAnchoredSweeps(t.ctx, len(a[0]), *full[:6], None, None) == 1
    t.run(FLAGS)
    check(t, expect(oracle, t, ow, w, None, ac.sweeps(q["anchor"], q["ls"], q["le"], q["radius"], q["hh"]), AABB), AABB)
    t.anchored_sweeps(*a)
    # a short capacity fills its records and no more; a range beyond the set is refused
    n, buf = capi.C.c_uint32(), (capi.SweepHit * 6)()
    assert t.lib.scTickReadAnchoredSweepHits(t.ctx, buf, 2, capi.C.byref(n)) == 1 and n.value == 6 and buf[1].hit == 1 and buf[2].hit == 0 and buf[2].id == 0
    seg = np.zeros((8, 3), F)
    assert t.lib.scTickReadAnchoredSweepSegments(t.ctx, 4, 3, seg.ctypes.data_as(capi.F32P), None) == 0 and "range exceeds" in t.lib.scTickGetLastError(t.ctx).decode()
    # a split flow in flight refuses the setter; an unflagged run closes the reads; the anchors need no run
    t.run(BASE | capi.SPLIT_PAIRS)
    with pytest.raises(capi.ScTickError, match="scTickRunPairs is pending"):
        t.anchored_sweeps(*a)
    t.run_pairs()
    for read in (t.anchored_sweep_hits, t.anchored_sweep_segments, t.anchored_sweep_shape_info):
        with pytest.raises(capi.ScTickError, match="did not request SC_TICK_ANCHORED_SWEEPS"):
            read()
    assert list(t.anchored_sweep_anchors()) == list(q["anchor"])
    t.run(FLAGS)
    t.anchored_sweeps(*[x[:4] for x in a])
    with pytest.raises(capi.ScTickError, match="re-sized since the last run"):
        t.anchored_sweep_hits()
    t.set_pipelined(True)
    with pytest.raises(capi.ScTickError, match="SC_TICK_ANCHORED_SWEEPS cannot run on a pipelined context"):
        t.run(FLAGS | capi.SPLIT_PAIRS)
    t.set_pipelined(False)
    t.set_tile(0, 1 << 4)
    with pytest.raises(capi.ScTickError, match="SC_TICK_ANCHORED_SWEEPS cannot run on a context with neighbours"):
        t.run(FLAGS | capi.SPLIT_PAIRS)
    t.set_tile(0, 0)
    t.run(FLAGS)
    check(t, expect(oracle, t, ow, w, None, ac.take(q, np.arange(4)), AABB), AABB)
    t.anchored_sweeps(*[x[:0] for x in a])                                      # count 0 clears the set
    with pytest.raises(capi.ScTickError, match="needs scTickSetAnchoredSweeps first"):
        t.run(FLAGS)
    t.close(); ow.close()


def test_a_context_that_never_sets_gives_the_tick_outputs_of_its_twin(oracle):
    w, col, q = ac.table(oracle)
    twins = [WorldTick.from_world(w, broadphase=True) for _ in range(2)]
    for t in twins:
        col.upload(t)
    twins[0].anchored_sweeps(*ac.args(q))
    for tick in range(3):
        for t in twins:
            t.nudge_roots_x(0.4)
        twins[0].run(FLAGS)
        twins[1].run(BASE)
        a, b = twins
        assert np.array_equal(a.world_matrices().view(U), b.world_matrices().view(U)) and a.counts().big_boxes == b.counts().big_boxes
        assert all(np.array_equal(x, y) for x, y in zip(a.world_aabbs(), b.world_aabbs()))
        pa, pb = a.pairs(), b.pairs()
        assert pa[1] == pb[1] and (len(pa[0]) < pa[1] or np.array_equal(np.sort(pa[0].view(np.uint64).reshape(-1)), np.sort(pb[0].view(np.uint64).reshape(-1))))
    for t in twins:
        t.close()
