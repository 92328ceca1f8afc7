"""Pair contacts (scTickSetPairContacts) through the C ABI against the fp32 witness (tests/pair_contacts_ref.py: the header's spec in numpy
fp32).  The witness takes the touching list the library itself reports for the tick -- which tests/test_gpu_pair_shapes.py's check()
holds against the touching witness -- and the tick's world matrices; record i must equal the witness's record for entry i of that list
bit for bit, and the report its counts exactly.  The worlds and closed forms are checked without a GPU in
tests/test_pair_contacts_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from sc_gameengine_amd import capi, synth_world as sw
from sc_gameengine_amd.tick import WorldTick
from tests import collider_ref as cr, pair_contacts_cases as KC, pair_contacts_ref as K, pair_shapes_cases as G, pair_shapes_ref as R
from tests.test_gpu_pair_shapes import check, start

pytestmark = pytest.mark.gpu
FLAGS = capi.XFORM | capi.BROADPHASE
SHAPES = FLAGS | capi.PAIR_SHAPES
F = np.float32
SENTINEL = 0x5A5A5A5A


def start_contacts(w, col, max_touching=1 << 16, **kw):
    t = start(w, col, max_touching=max_touching, **kw)
    t.set_pair_contacts(True)
    assert t.pair_contacts_enabled()
    return t


def check_contacts(t, col, max_touching, rank=0):
    """the records of the last flagged tick against the witness over the library's own touching list, entry by entry; returns
    (list, records)"""
    listed, sinfo = t.read_pair_shapes()
    rec, info = t.read_pair_contacts()
    assert len(rec) == len(listed) == min(sinfo["touching"], max_touching) == info["written"]
    want = K.contacts32(t.world_matrices(), col, listed, n=t.n, rank=rank)
    differ = np.flatnonzero((K.bits(rec) != K.bits(want)).any(axis=1))
    assert not len(differ), f"{len(differ)} of {len(rec)} records differ; first: pair {listed[differ[0]].tolist()} got {rec[differ[0]]} want {want[differ[0]]}"
    assert info == K.report(want), f"{info} != {K.report(want)}"
    return listed, rec


# ---- 1. the constructed cases in one world -----------------------------------------------------------------------------------------
def test_constructed_cases_bit_for_bit(oracle):
    w, col, cases, origins = KC.contact_world()
    t = start_contacts(w, col)
    t.run(SHAPES)
    assert np.array_equal(t.world_matrices(), G.oracle_matrices(oracle, w))
    check(t, col, 1 << 16)
    listed, rec = check_contacts(t, col, 1 << 16)
    order = np.argsort(R.keys(listed))
    assert listed[order].tolist() == [[2 * i, 2 * i + 1] for i in range(len(cases))]
    assert rec["kind"][order].tolist() == [c[1] for c in cases]
    for i, (name, kind, normal, depth, point, *_) in zip(order, cases):
        assert abs(float(rec["depth"][i]) - depth) < 1e-4, name
        if normal is not None:
            assert np.abs(rec["normal"][i] - np.asarray(normal)).max() < 1e-4, name
    t.close()


# ---- 2. an agreement world and the forest ------------------------------------------------------------------------------------------
def test_agreement_world_bit_for_bit(oracle):
    w, col = G.agreement_world(G.AGREEMENT_SEEDS[0])
    t = start_contacts(w, col)
    for _ in range(2):
        t.run(SHAPES)
        check(t, col, 1 << 16)
        listed, rec = check_contacts(t, col, 1 << 16)
        shape = rec["kind"] & 0xFF
        assert len(rec) > 600 and all((shape == k).sum() >= 10 for k in range(1, 6)) and ((rec["kind"] & K.DEEP) != 0).sum() >= 30
    t.close()


def test_forest_with_sheared_frames_and_twice_named_pairs(oracle):
    w, col = G.forest()
    t = start_contacts(w, col)
    for _ in range(2):
        t.nudge_roots_x(G.FOREST_NUDGE)
        t.run(SHAPES)
        check(t, col, 1 << 16)
        listed, rec = check_contacts(t, col, 1 << 16)
        assert (rec["kind"] == K.NONE).sum() >= 100 and ((rec["kind"] & 0xFF) >= K.BOX_FACE_A).sum() >= 50
        # a pair the list names twice is listed twice, each time with the same record
        keys, first, counts = np.unique(R.keys(listed), return_index=True, return_counts=True)
        for key in keys[counts > 1]:
            rows = K.bits(rec[R.keys(listed) == key])
            assert (rows == rows[0]).all()
    t.close()


# ---- 3. touching lists at which the walk can go wrong ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", G.WALK_LENGTHS)
def test_touching_lists_of_awkward_lengths(oracle, k):
    w, col, _ = G.couples_world(k, G.WALK_SEED + k)
    if k:
        w.pos[1::2] = w.pos[0::2] + F([0.4, 0.3, 0.2])      # every couple touches: the touching list has exactly k entries
        col.he[:] = 0.6
    t = start_contacts(w, col, max_touching=2048)
    for _ in range(2):                                      # the learn tick and a tick on the home slots
        t.run(SHAPES)
        check(t, col, 2048)
        listed, rec = check_contacts(t, col, 2048)
        assert len(listed) == k and (rec["kind"] != K.NONE).all()
    t.close()


# ---- 4. capacities -----------------------------------------------------------------------------------------------------------------
def test_short_lists_short_reads_and_a_truncated_pair_list(oracle):
    w, col = G.forest()
    t = start_contacts(w, col, max_touching=100)
    t.run(SHAPES)
    check(t, col, 100)
    listed, rec = check_contacts(t, col, 100)               # the list and the records still correspond, entry by entry
    _, info = t.read_pair_contacts()
    assert info["written"] == 100 == len(rec) and t.read_pair_shapes()[1]["touching"] > 1000
    # a read with less room than max_touching: capacity records, the buffer beyond them keeps its sentinel
    buf = np.full((64, 8), SENTINEL, np.uint32)
    cinfo = capi.PairContactInfo()
    assert t.lib.scTickReadPairContacts(t.ctx, buf.ctypes.data_as(C.POINTER(capi.PairContact)), 40, C.byref(cinfo)) == 1
    assert cinfo.written == 100 and np.array_equal(buf[:40], K.bits(rec[:40])) and (buf[40:] == SENTINEL).all()
    assert t.lib.scTickReadPairContacts(t.ctx, None, 0, C.byref(cinfo)) == 1 and cinfo.written == 100      # the report alone
    t.close()
    t = start_contacts(w, col, max_pairs=1024)              # a truncated pair list: records of what was listed
    t.run(SHAPES)
    check(t, col, 1 << 16)
    check_contacts(t, col, 1 << 16)
    assert t.counts().pairs_truncated == 1
    t.close()


# ---- 5. the pass leaves the rest alone ---------------------------------------------------------------------------------------------
def test_every_other_output_is_that_of_a_twin_without_contacts(oracle):
    w, col = G.forest()
    on, off, never = start_contacts(w, col), start_contacts(w, col), start(w, col)
    off.set_pair_contacts(False)
    assert not off.pair_contacts_enabled() and not never.pair_contacts_enabled()
    for t in (on, off, never):
        t.set_pair_events(1 << 14, 1 << 14)
        t.set_touch_events(1 << 14, 1 << 14)
    rng = np.random.default_rng(2461)
    flags = SHAPES | capi.PAIR_EVENTS | capi.TOUCH_EVENTS
    for tick in range(3):
        pos = w.pos.copy()
        pos[w.parent < 0] += rng.uniform(-0.5, 0.5, (int((w.parent < 0).sum()), 3)).astype(F)
        outs = []
        for t in (on, off, never):
            t.upload_positions(0, pos)
            t.run(flags)
            check(t, col, 1 << 16)
            lst, sinfo = t.read_pair_shapes()
            tb, te, ti = t.touch_events()
            pb, pe, pi = t.pair_events()
            outs.append((np.sort(R.keys(lst)), sinfo, np.sort(R.keys(tb)), np.sort(R.keys(te)), ti, np.sort(R.keys(pb)), np.sort(R.keys(pe)), pi))
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
        assert tick == 0 or (outs[0][4]["begun"] >= 1 and outs[0][4]["ended"] >= 1)
        check_contacts(on, col, 1 << 16)                    # all three features in one run
        for t in (off, never):
            with pytest.raises(capi.ScTickError, match="pair contacts were not enabled"):
                t.read_pair_contacts()
    for t in (on, off, never):
        t.close()


# ---- 6. graph replay ---------------------------------------------------------------------------------------------------------------
def test_replayed_graphs_with_contacts_toggled_between_captures(oracle):
    w, col = G.forest()
    t = start(w, col)
    t.set_graph_mode(True)
    learn = None
    for phase, enabled in enumerate((False, True, False, True)):
        t.set_pair_contacts(enabled)                        # drops the graphs: the next ticks capture and replay with / without the launch
        for _ in range(4):
            t.nudge_roots_x(0.25)
            t.run(SHAPES)
            check(t, col, 1 << 16)
            if enabled:
                check_contacts(t, col, 1 << 16)
            else:
                with pytest.raises(capi.ScTickError, match="pair contacts were not enabled"):
                    t.read_pair_contacts()
        learn = t.learn_ticks() if learn is None else learn
    assert t.learn_ticks() == learn                         # the setter asked for no learn tick
    t.close()


# ---- 7. residency ------------------------------------------------------------------------------------------------------------------
def test_records_follow_removals_and_a_new_collider_upload(oracle):
    w, col = G.agreement_world(2431, n=900)
    rng = np.random.default_rng(2432)
    t = start_contacts(w, col, capacity=w.n)
    t.run(SHAPES)
    check_contacts(t, col, 1 << 16)
    gone = rng.choice(np.arange(100, 700), 80, replace=False).astype(np.uint32)
    src, dst = t.remove_entities(gone)
    n1 = w.n - len(gone)
    now = cr.Colliders(n1)
    for a, b in ((now.type, col.type), (now.he, col.he), (now.radius, col.radius), (now.hh, col.hh)):
        a[:] = b[:n1]
        a[dst] = b[src]
    t.run(SHAPES)
    check(t, now, 1 << 16)
    check_contacts(t, now, 1 << 16)
    # a new upload over a range: other types, other sizes, some Bounds proxies -- the records follow
    other = cr.Colliders.random(n1, rng, p=(0.2, 0.0, 0.3, 0.25, 0.25))
    other.he[:] = rng.uniform(0.3, 1.4, (n1, 3)).astype(F); other.radius[:] = rng.uniform(0.3, 1.2, n1).astype(F)
    for a, b in ((now.type, other.type), (now.he, other.he), (now.radius, other.radius), (now.hh, other.hh)):
        a[200:600] = b[200:600]
    before = t.read_pair_contacts()[0]
    now.upload(t, 200, 400)
    t.run(SHAPES)
    check(t, now, 1 << 16)
    _, rec = check_contacts(t, now, 1 << 16)
    assert (rec["kind"] == K.NONE).sum() > 20 and not np.array_equal(np.sort(before["kind"]), np.sort(rec["kind"]))
    t.close()


# ---- 8. the split flow -------------------------------------------------------------------------------------------------------------
def test_the_split_flow_writes_the_records_behind_run_pairs(oracle):
    w, col = G.agreement_world(2441, n=700)
    t = start_contacts(w, col)
    t.run(SHAPES | capi.SPLIT_PAIRS)
    with pytest.raises(capi.ScTickError, match="pair contacts are ready after scTickRunPairs"):
        t.read_pair_contacts()
    with pytest.raises(capi.ScTickError, match="scTickRunPairs is pending"):
        t.set_pair_contacts(False)
    with pytest.raises(capi.ScTickError, match="scTickRunPairs is pending"):
        t.set_pair_contacts(True)
    assert t.pair_contacts_enabled()
    t.run_pairs()
    check(t, col, 1 << 16)
    _, rec = check_contacts(t, col, 1 << 16)
    assert len(rec) > 300
    t.close()


# ---- 9. tiles ----------------------------------------------------------------------------------------------------------------------
def test_a_neighbour_tiles_sphere_gives_none(oracle):
    """2 x 1 tiles on one GPU, the caller-owned split flow, as tests/test_gpu_pair_shapes.py sets it up: sphere B of tile 1 reaches 0.2 m
    into tile 0, which knows it from the border merge alone; sphere A of tile 0 overlaps it.  The pair is listed on its AABB answer and
    its record is SC_TICK_CONTACT_NONE; the pair A - C of two own spheres gets a ROUND_ROUND record."""
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
    b = int(np.flatnonzero(lone & (np.arange(w.n) >= n))[0])
    a, c = (int(x) for x in np.flatnonzero(lone & (np.arange(w.n) < n))[:2])
    w.pos[b] = [edge + 0.3, 200.0, 100.3]
    w.pos[a] = [edge - 0.3, 200.0, 100.0]
    w.pos[c] = [edge - 0.9, 200.0, 100.3]
    col = cr.Colliders(w.n)
    for e in (a, b, c):
        w.scale[e] = 1.0; w.rot[e] = 0.0
        col.type[e] = cr.SPHERE; col.radius[e] = 0.5
    parts, n = split_world(w, grid, S)
    flags = SHAPES | capi.SPLIT_PAIRS
    ticks = [WorldTick.from_world(p, broadphase=True, max_pairs=1 << 16) for p in parts]
    cols = []
    for r, t in enumerate(ticks):
        part = cr.Colliders(n)
        for x, y in ((part.type, col.type), (part.he, col.he), (part.radius, col.radius), (part.hh, col.hh)):
            x[:] = y[r * n:(r + 1) * n]
        part.upload(t)
        t.set_pair_shapes(1 << 16)
        t.set_pair_contacts(True)
        cols.append(part)
    bufs = [tiles.BorderBuffers(t, r, grid, "cuda") for r, t in enumerate(ticks)]
    for t in ticks:
        t.run(flags)
    network(bufs, grid, parity=0)
    for t in ticks:
        t.run_pairs()
    ida, idb, idc = a, (1 << 24) | (b - n), c
    ab, ac = R.keys([[ida, idb]])[0], R.keys([[min(ida, idc), max(ida, idc)]])[0]
    held = 0
    for r, t in enumerate(ticks):
        check(t, cols[r], 1 << 16, rank=r)
        listed, rec = check_contacts(t, cols[r], 1 << 16, rank=r)
        keys = R.keys(listed)
        held += int((keys == ab).sum())
        assert (rec["kind"][keys == ab] == K.NONE).all() and not K.bits(rec[keys == ab]).any()
        if r == 0:
            assert (keys == ac).sum() == 1 and (rec["kind"][keys == ac] == K.ROUND_ROUND).all()
    assert held >= 1
    for t in ticks:
        t.close()


# ---- 10. every refusal, switching off and re-sizing --------------------------------------------------------------------------------
def test_pair_contact_api_errors_and_sizes(oracle):
    w, col = G.agreement_world(2451, n=300)
    t = start(w, col, max_touching=0)
    with pytest.raises(capi.ScTickError, match="needs scTickSetPairShapes\\(max_touching > 0\\) first"):
        t.set_pair_contacts(True)
    t.set_pair_contacts(False)                              # nothing to free: welcome
    assert not t.pair_contacts_enabled()
    t.run(FLAGS)                                            # the refusal changed nothing: the context still runs
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_PAIR_SHAPES"):
        t.read_pair_contacts()
    t.set_pair_shapes(64)
    t.run(SHAPES)
    with pytest.raises(capi.ScTickError, match="pair contacts were not enabled"):
        t.read_pair_contacts()
    t.run(SHAPES | capi.SPLIT_PAIRS)
    with pytest.raises(capi.ScTickError, match="pair contacts were not enabled"):      # ... which is said before the pending half is
        t.read_pair_contacts()
    t.run_pairs()
    t.set_pair_contacts(True)
    with pytest.raises(capi.ScTickError, match="pair contacts were not enabled"):      # enabled since: the last run still wrote none
        t.read_pair_contacts()
    t.run(SHAPES)
    check(t, col, 64)
    _, rec = check_contacts(t, col, 64)
    assert len(rec) == 64
    info = capi.PairContactInfo()
    assert t.lib.scTickReadPairContacts(t.ctx, None, 0, None) == 0 and b"null argument" in t.lib.scTickGetLastError(t.ctx)
    assert t.lib.scTickGetPairContacts(t.ctx, None) == 0 and b"null argument" in t.lib.scTickGetLastError(t.ctx)
    t.run(FLAGS)
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_PAIR_SHAPES"):
        t.read_pair_contacts()
    # another size: the contact buffer follows the list
    t.set_pair_shapes(1 << 12)
    assert t.pair_contacts_enabled()
    t.run(SHAPES)
    check(t, col, 1 << 12)
    _, rec = check_contacts(t, col, 1 << 12)
    assert len(rec) > 64
    t.set_pair_contacts(False)
    t.run(SHAPES)
    check(t, col, 1 << 12)
    with pytest.raises(capi.ScTickError, match="pair contacts were not enabled"):
        t.read_pair_contacts()
    t.set_pair_contacts(True)
    t.run(SHAPES)
    t.set_pair_contacts(False)
    with pytest.raises(capi.ScTickError, match="switched off since the last scTickRun"):
        t.read_pair_contacts()
    # scTickSetPairShapes(0) switches contacts off too
    t.set_pair_contacts(True)
    t.set_pair_shapes(0)
    assert not t.pair_contacts_enabled()
    with pytest.raises(capi.ScTickError, match="needs scTickSetPairShapes\\(max_touching > 0\\) first"):
        t.set_pair_contacts(True)
    t.run(FLAGS)
    t.close()
    # a context without colliders: every pair is listed on its AABB answer, every record is NONE
    t = start_contacts(w, None)
    t.run(SHAPES)
    check(t, None, 1 << 16)
    _, rec = check_contacts(t, None, 1 << 16)
    assert len(rec) > 50 and not K.bits(rec).any()
    t.close()
