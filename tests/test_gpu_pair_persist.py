"""Pair persistence (scTickSetPairPersistence) through the C ABI against the fp32 witness (tests/pair_persist_ref.py: the header's spec in
numpy fp32).  The device's list order is not fixed, so the witness works from the lists as read back: the previous flagged run's list,
manifolds, records, payload rows and matrices, and this run's list, manifolds and matrices.  Records and payload rows must equal its
answer bit for bit, the report exactly.  The worlds and their floors are checked without a GPU in tests/test_pair_persist_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from sc_gameengine_amd import capi
from tests import (pair_contacts_ref as K, pair_manifolds_ref as M, pair_persist_cases as PC, pair_persist_ref as P, pair_shapes_cases as G,
                   pair_shapes_ref as R)
from tests.test_gpu_pair_manifolds import box_couples, check_manifolds, start_manifolds
from tests.test_gpu_pair_shapes import start
from tests.test_pair_persist_cpu import tallies

pytestmark = pytest.mark.gpu
FLAGS = capi.XFORM | capi.BROADPHASE
SHAPES = FLAGS | capi.PAIR_SHAPES
F = np.float32
SENTINEL = 0x5A5A5A5A
BIG = 1 << 16


class Tracked:
    """a context with persistence on, and what the witness remembers of its last flagged run"""
    def __init__(self, w, col, max_touching=BIG, match_dist=PC.MATCH_DIST, **kw):
        self.t = start_manifolds(w, col, max_touching=max_touching, **kw)
        self.max_touching, self.match_dist, self.prev = max_touching, match_dist, None
        self.t.pair_persistence(True, match_dist)
        assert self.t.pair_persistence_enabled() and self.t.pair_persistence_match_dist() == float(F(match_dist))

    def run(self, flags=SHAPES):
        self.t.run(flags)
        return self.check()

    def check(self):
        """the last flagged run against the witness; returns (what it leaves behind, report)"""
        t = self.t
        listed, sinfo = t.read_pair_shapes()
        man, minfo = t.read_pair_manifolds()
        rec, info = t.read_pair_persistence()
        rows = t.read_pair_payloads()
        m = t.world_matrices()
        assert len(rec) == len(rows) == len(man) == len(listed) == min(sinfo["touching"], self.max_touching) == info["written"]
        want, want_rows, want_info = P.persist32(self.prev, listed, man, m, self.match_dist, truncated=bool(sinfo["truncated"] | sinfo["pairs_truncated"]))
        assert info == want_info, f"{info} != {want_info}"
        differ = np.flatnonzero((P.bits(rec) != P.bits(want)).any(axis=1))
        assert not len(differ), f"{len(differ)} of {len(rec)} records differ; first: entry {differ[0]} pair {listed[differ[0]].tolist()} got {rec[differ[0]]} want {want[differ[0]]}"
        assert np.array_equal(P.row_bits(rows), P.row_bits(want_rows)), "carried payload rows differ"
        assert not rec["reserved"].any()
        self.prev = P.Run(listed, man, rec, rows, m)
        return self.prev, info

    def write(self, rows, first=0):
        self.t.write_pair_payloads(rows, first)
        self.prev.payloads[first:first + len(rows)] = rows

    def forget(self):
        self.prev = None

    def close(self):
        self.t.close()


def live_slots(run):
    return np.arange(4)[None, :] < run.manifolds["count"][:, None]


def payload_rows(listed):
    """rows that are a function of (pair, slot), NaN bit patterns among them: words (a, b, slot, a quiet NaN carrying the entry's b)"""
    rows = np.zeros((len(listed), 4, 4), np.uint32)
    rows[:, :, 0] = listed[:, 0, None] + 1
    rows[:, :, 1] = listed[:, 1, None] + 1
    rows[:, :, 2] = np.arange(4)[None, :] + 1
    rows[:, :, 3] = 0x7FC00000 | (listed[:, 1, None] & 0xFFFF)
    return rows.view(F)


# ---- 1. the constructed sequence ---------------------------------------------------------------------------------------------------
def test_constructed_sequence_new_kept_and_moved(oracle):
    w, col, cases, pos3, rot3 = PC.constructed()
    x = Tracked(w, col)
    one, info = x.run()
    check_manifolds(x.t, col, BIG)
    assert info["resync"] == 1 and info["kept_pairs"] == 0 and info["kept_points"] == 0 and info["new_pairs"] == len(cases)
    assert (one.records["prev_entry"] == P.NONE).all() and (one.records["prev_slot"] == 0xFF).all() and not one.records["age"].any()
    two, info = x.run()
    live = live_slots(two)
    assert info["resync"] == 0 and info["new_points"] == 0 and info["kept_pairs"] == len(cases) and info["kept_points"] == int(live.sum())
    assert (two.records["age"][live] == 1).all() and np.array_equal(R.keys(one.listed[two.records["prev_entry"]]), R.keys(two.listed))
    x.t.upload_locals(0, pos3, rot3, w.scale)
    three, info = x.run()
    entry = {int(a) // 2: i for i, a in enumerate(three.listed[:, 0])}
    for i, case in enumerate(cases):
        how = PC.MOTIONS.get(case[0])
        if how == PC.LIFTED:
            assert i not in entry
            continue
        r, n = three.records[entry[i]], int(three.manifolds["count"][entry[i]])
        assert two.listed[r["prev_entry"]].tolist() == [2 * i, 2 * i + 1], case[0]
        if how == PC.SLID_FIVE:
            assert r["prev_slot"].tolist() == [0xFF] * 4 and not r["age"].any()
        else:
            assert r["prev_slot"].tolist() == list(range(n)) + [0xFF] * (4 - n) and r["age"].tolist() == [2] * n + [0] * (4 - n), case[0]
        if how == PC.TURNED:                                # kept in a's frame, decimetres away in world space
            old = two.manifolds["point"][int(r["prev_entry"])]
            assert n == 4 and np.abs(three.manifolds["point"][entry[i]] - old).max() > 0.1
    x.close()


# ---- 2. the slide worlds and the carry worlds --------------------------------------------------------------------------------------
def test_slide_worlds_hold_their_floors_on_the_device(oracle):
    total = np.zeros(4, np.int64)
    for seed in PC.SEEDS:
        w, col, pos2 = PC.slide_world(seed)
        x = Tracked(w, col)
        one, _ = x.run()
        x.t.upload_positions(0, pos2)
        two, info = x.run()
        got = tallies(two, one)
        assert got[0] == info["kept_points"] and got[1] == info["new_points"] and info["gave_up"] == 0
        total += got
        x.close()
    print("slide worlds on the device: kept, new, mixed entries, moved-slot entries =", total.tolist())
    assert total[0] >= PC.FLOORS["kept_points"] and total[1] >= PC.FLOORS["new_points"]
    assert total[2] >= PC.FLOORS["mixed_entries"] and total[3] >= PC.FLOORS["moved_slot_entries"]


def test_carry_worlds_keep_every_point_with_its_slot(oracle):
    for seed in PC.SEEDS:
        w, col, pos2 = PC.carry_world(seed)
        x = Tracked(w, col)
        one, _ = x.run()
        x.t.upload_positions(0, pos2)
        two, info = x.run()
        live = live_slots(two)
        assert info["new_points"] == 0 and info["kept_pairs"] == len(one.listed) == len(two.listed) and info["kept_points"] == int(live.sum())
        assert np.array_equal(two.records["prev_slot"][live], np.broadcast_to(np.arange(4, dtype=np.uint8), live.shape)[live])
        assert (two.records["age"][live] == 1).all()
        x.close()


# ---- 3. payloads -------------------------------------------------------------------------------------------------------------------
def test_payload_rows_ride_on_kept_points_bit_for_bit(oracle):
    w, col, pos2 = PC.slide_world(PC.SEEDS[0])
    x = Tracked(w, col)
    one, _ = x.run()
    assert not P.row_bits(one.payloads).any()               # nothing remembered: four +0 everywhere
    x.write(payload_rows(one.listed))                       # every slot, those at or above count too
    assert np.array_equal(P.row_bits(x.t.read_pair_payloads()), P.row_bits(payload_rows(one.listed)))
    x.t.upload_positions(0, pos2)
    two, info = x.run()
    live, kept = live_slots(two), two.records["prev_slot"] != 0xFF
    assert info["kept_points"] >= 150 and info["new_points"] >= 50
    source = payload_rows(one.listed)[np.minimum(two.records["prev_entry"], len(one.listed) - 1)[:, None], np.minimum(two.records["prev_slot"], 3)]
    assert np.array_equal(P.row_bits(two.payloads)[kept], P.row_bits(source)[kept]) and not P.row_bits(two.payloads)[~kept].any()
    assert not kept[~live].any()                            # a slot at or above count is never carried, whatever row lay there
    three, info3 = x.run()                                  # no write in between: what was carried is carried on
    kept3 = three.records["prev_slot"] != 0xFF
    assert info3["new_points"] == 0 and np.array_equal(kept3, live_slots(three))
    order2, order3 = np.argsort(R.keys(two.listed)), np.argsort(R.keys(three.listed))
    assert np.array_equal(P.row_bits(three.payloads)[order3], P.row_bits(two.payloads)[order2])
    part = (payload_rows(three.listed[5:9]).view(np.uint32) ^ 0x00010000).view(F)      # a write to first > 0
    x.write(part, first=5)
    now = x.t.read_pair_payloads()
    assert np.array_equal(P.row_bits(now[5:9]), P.row_bits(part)) and np.array_equal(P.row_bits(now[:5]), P.row_bits(three.payloads[:5]))
    assert np.array_equal(P.row_bits(now[9:]), P.row_bits(three.payloads[9:]))
    four, _ = x.run()
    at = {int(k): i for i, k in enumerate(R.keys(four.listed))}
    for j in range(5, 9):                                   # the written rows arrive with the points of their pairs
        i = at[int(R.keys(three.listed[j:j + 1])[0])]
        n = int(four.manifolds["count"][i])
        assert np.array_equal(P.row_bits(four.payloads[i, :n]), P.row_bits(part[j - 5, :n]))
    x.close()


# ---- 4. touching lists on the wave's and the workgroup's edges -----------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 63, 64, 65, 129))
def test_touching_lists_of_awkward_lengths_all_boxes(oracle, k):
    w, col = box_couples(k)
    x = Tracked(w, col, max_touching=2048)
    one, info = x.run()
    assert len(one.listed) == k and info["resync"] == 1 and info["new_pairs"] == k
    x.write(payload_rows(one.listed))
    two, info = x.run()
    live = live_slots(two)
    assert len(two.listed) == k and info["kept_pairs"] == k and info["new_points"] == 0 and info["kept_points"] == int(live.sum()) >= k
    assert (two.records["age"][live] == 1).all() and P.row_bits(two.payloads)[live].all()
    x.close()


# ---- 5. a pair the list names twice ------------------------------------------------------------------------------------------------
def test_forest_entries_of_one_pair_point_at_the_smallest_remembered_entry(oracle):
    """the manifold suite's forest: whatever its list names twice matches one remembered entry, the smallest (the witness holds every
    entry to that rule; tests/test_pair_persist_cpu.py feeds it a list with duplicates)"""
    w, col = G.forest()
    x = Tracked(w, col)
    for tick in range(3):
        if tick < 2:
            x.t.nudge_roots_x(G.FOREST_NUDGE)
        before = x.prev
        run, info = x.run()
        assert info["gave_up"] == 0 and len(run.listed) > 1000 and (info["kept_pairs"] > 700 if tick else info["resync"] == 1)
        if tick == 2:                                       # nothing moved: every remembered pair is found again, every point kept in place
            live = live_slots(run)
            assert info["kept_pairs"] == len(run.listed) and info["new_points"] == 0 and (run.records["age"][live] >= 1).all()
        keys1, keys2 = (R.keys(before.listed) if before else np.zeros(0, np.uint64)), R.keys(run.listed)
        uniq, counts = np.unique(keys2, return_counts=True)
        for key in uniq[counts > 1]:
            first = np.flatnonzero(keys1 == key)
            assert (run.records["prev_entry"][keys2 == key] == (first[0] if len(first) else P.NONE)).all()
    x.close()


# ---- 6. a truncated touching list --------------------------------------------------------------------------------------------------
def test_a_truncated_list_answers_and_remembers_what_was_listed(oracle):
    w, col = G.forest()
    x = Tracked(w, col, max_touching=100)
    for tick in range(3):
        run, info = x.run()
        assert info["written"] == 100 == len(run.listed) and info["list_truncated"] == 1 and info["resync"] == (1 if tick == 0 else 0)
        assert x.t.read_pair_shapes()[1]["touching"] > 1000
    buf = np.full((64, 4), SENTINEL, np.uint32)             # less room than max_touching: the buffer beyond keeps its sentinel
    pinfo = capi.PairPersistInfo()
    assert x.t.lib.scTickReadPairPersistence(x.t.ctx, buf.ctypes.data_as(C.POINTER(capi.PairPersist)), 40, C.byref(pinfo)) == 1
    assert pinfo.written == 100 and np.array_equal(buf[:40], P.bits(run.records[:40])) and (buf[40:] == SENTINEL).all()
    rows = np.full((64, 16), SENTINEL, np.uint32)
    assert x.t.lib.scTickReadPairPayloads(x.t.ctx, rows.view(F).ctypes.data_as(capi.F32P), 40) == 1
    assert np.array_equal(rows[:40], P.row_bits(run.payloads[:40]).reshape(-1, 16)) and (rows[40:] == SENTINEL).all()
    x.close()
    x = Tracked(w, col, max_pairs=1024)                     # a truncated pair list
    for _ in range(2):
        _, info = x.run()
        assert info["list_truncated"] == 1 and x.t.counts().pairs_truncated == 1
    x.close()


# ---- 7. resync ---------------------------------------------------------------------------------------------------------------------
def test_resync_after_renames_and_resizes_and_unflagged_runs_in_between(oracle):
    w, col = G.agreement_world(2631, n=900)
    x = Tracked(w, col, capacity=w.n)
    t = x.t

    def expect(resync):
        run, info = x.run()
        assert info["resync"] == resync and len(run.listed) > 200
        if resync:
            assert (run.records["prev_entry"] == P.NONE).all() and info["kept_pairs"] == 0
        else:                                               # (this world's pair list gains a pair or two from tick to tick: the witness holds each entry)
            assert info["kept_pairs"] >= len(run.listed) - 60 and info["kept_points"] > 10 * info["new_points"]
        return run

    def settle():
        expect(0)

    expect(1)
    settle()
    expect(0)
    for _ in range(2):                                      # runs without the flag leave the memory alone
        t.run(FLAGS)
        with pytest.raises(capi.ScTickError, match="did not request SC_TICK_PAIR_SHAPES"):
            t.read_pair_persistence()
    expect(0)
    t.remove_entities(np.arange(100, 700, 8, dtype=np.uint32))
    x.forget()
    expect(1)
    settle()
    expect(0)
    t.set_count(t.n - 20)                                   # a shrinking count
    x.forget()
    expect(1)
    settle()
    t.set_count(t.n + 20)                                   # ... a growing one renames nothing: what was remembered is kept, and
    run, info = x.run()                                     # the pairs of the twenty entities back in the count are new
    assert info["resync"] == 0 and info["kept_pairs"] > 1000 and 0 < info["new_pairs"] < 200
    settle()
    expect(0)
    t.set_tile(3, 0)                                        # ids carry the rank
    x.forget()
    run = expect(1)
    assert (run.listed >> 24 == 3).all()
    settle()
    expect(0)
    t.set_pair_shapes(BIG)                                  # the same size: the memory stays
    settle()
    expect(0)
    t.set_pair_shapes(1 << 12)                              # another size
    x.max_touching = 1 << 12
    x.forget()
    assert t.pair_persistence_enabled() and t.pair_persistence_match_dist() == float(F(PC.MATCH_DIST))
    expect(1)
    settle()
    expect(0)
    x.close()


# ---- 8. age saturation -------------------------------------------------------------------------------------------------------------
def test_the_age_of_a_resting_point_saturates_at_255(oracle):
    w, col, cases, _ = PC.MC.manifold_world()
    x = Tracked(w, col)
    for tick in range(260):
        x.t.run(SHAPES)
        if tick in (0, 1, 254, 255, 256, 259):
            listed, _ = x.t.read_pair_shapes()
            rec, info = x.t.read_pair_persistence()
            i = int(np.flatnonzero(listed[:, 0] == 0)[0])   # the cube flat on the slab: four points
            assert rec["age"][i].tolist() == [min(tick, 255)] * 4 and rec["prev_slot"][i].tolist() == ([0, 1, 2, 3] if tick else [0xFF] * 4)
            assert info["resync"] == (1 if tick == 0 else 0)
    x.close()


# ---- 9. graph replay ---------------------------------------------------------------------------------------------------------------
def test_replayed_graphs_of_both_parities_equal_an_eager_twin(oracle):
    w, col, pos2 = PC.slide_world(PC.SEEDS[1])
    mid = ((w.pos.astype(np.float64) + pos2) / 2).astype(F)
    eager, graph = Tracked(w, col), Tracked(w, col)
    graph.t.set_graph_mode(True)

    def both(pos):
        outs = []
        for x in (eager, graph):
            x.t.upload_positions(0, pos)
            run, info = x.run()
            order = np.argsort(R.keys(run.listed))
            prev_pair = np.where(run.records["prev_entry"] != P.NONE, R.keys(x.before.listed)[np.minimum(run.records["prev_entry"], len(x.before.listed) - 1)]
                                 if x.before is not None else 0, 0)
            outs.append((R.keys(run.listed)[order], prev_pair[order], run.records["prev_slot"][order], run.records["age"][order],
                         P.row_bits(run.payloads)[order], info))
            x.before = run
        for a, b in zip(*outs):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
        return outs[0][-1]

    eager.before = graph.before = None
    for pos in (w.pos, w.pos, w.pos):                       # the learn tick and a capture per tick parity: what follows are replays
        both(pos)
    learn = graph.t.learn_ticks()
    for x in (eager, graph):
        x.write(payload_rows(x.prev.listed))
    infos = [both(pos) for pos in (mid, pos2, pos2, w.pos, mid, w.pos)]      # six ticks, both parities replayed
    assert all(i["resync"] == 0 for i in infos) and infos[1]["kept_points"] > 100 and infos[3]["new_points"] > 30
    for x in (eager, graph):                                # toggled between captures: off drops the memory, on starts from nothing
        x.t.pair_persistence(False)
        assert not x.t.pair_persistence_enabled() and x.t.pair_persistence_match_dist() == 0.0
        x.t.run(SHAPES)
        with pytest.raises(capi.ScTickError, match="pair persistence was not enabled"):
            x.t.read_pair_persistence()
        x.t.pair_persistence(True, PC.MATCH_DIST)
        x.forget()
        x.before = None
    assert both(w.pos)["resync"] == 1
    tight = both(pos2)
    both(w.pos)
    for x in (eager, graph):                                # another match_dist after a capture: the memory stays, the next run goes by it
        x.t.pair_persistence(True, 0.05)
        x.match_dist = 0.05
        x.write(payload_rows(x.prev.listed))                # ... and a payload write between replays
    wide = both(pos2)
    assert wide["resync"] == 0 and wide["kept_points"] > tight["kept_points"] + 30
    both(pos2)
    assert graph.t.learn_ticks() == learn                   # the setters asked for no learn tick: the checked ticks were replays
    eager.close()
    graph.close()


# ---- 10. the split flow ------------------------------------------------------------------------------------------------------------
def test_the_split_flow_matches_behind_run_pairs(oracle):
    w, col, pos2 = PC.slide_world(PC.SEEDS[2])
    x = Tracked(w, col)
    t = x.t
    one, _ = x.run()
    x.write(payload_rows(one.listed))
    t.upload_positions(0, pos2)
    t.run(SHAPES | capi.SPLIT_PAIRS)
    with pytest.raises(capi.ScTickError, match="pair persistence is ready after scTickRunPairs"):
        t.read_pair_persistence()
    with pytest.raises(capi.ScTickError, match="pair persistence is ready after scTickRunPairs"):
        t.read_pair_payloads()
    with pytest.raises(capi.ScTickError, match="scTickRunPairs is pending"):
        t.write_pair_payloads(payload_rows(one.listed[:1]))
    with pytest.raises(capi.ScTickError, match="scTickRunPairs is pending"):
        t.pair_persistence(True, 0.05)
    assert t.pair_persistence_match_dist() == float(F(PC.MATCH_DIST))
    t.run_pairs()
    two, info = x.check()                                   # records and carried rows appear behind run_pairs
    assert info["resync"] == 0 and info["kept_points"] > 100 and P.row_bits(two.payloads).any()
    t.run(SHAPES | capi.SPLIT_PAIRS)                        # a rename between the halves: forgotten again behind the pair half
    t.set_tile(3, 0)
    x.forget()
    t.run_pairs()
    _, info = x.check()
    assert info["resync"] == 1
    x.forget()
    _, info = x.run()
    assert info["resync"] == 1
    _, info = x.run()
    assert info["resync"] == 0 and info["new_points"] == 0
    x.close()


# ---- 11. the pass leaves the rest alone --------------------------------------------------------------------------------------------
def test_every_other_output_is_that_of_a_twin_without_persistence(oracle):
    w, col = G.forest()
    on, off = Tracked(w, col), Tracked(w, col)
    off.t.pair_persistence(False)
    never = start_manifolds(w, col)
    ticks = (on.t, off.t, never)
    for t in ticks:
        t.pair_islands(True, 0)
        t.set_pair_events(1 << 14, 1 << 14)
        t.set_touch_events(1 << 14, 1 << 14)
    rng = np.random.default_rng(2671)
    flags = SHAPES | capi.PAIR_EVENTS | capi.TOUCH_EVENTS
    for tick in range(3):
        pos = w.pos.copy()
        pos[w.parent < 0] += rng.uniform(-0.5, 0.5, (int((w.parent < 0).sum()), 3)).astype(F)
        outs = []
        for t in ticks:
            t.upload_positions(0, pos)
            t.run(flags)
            lst, sinfo = t.read_pair_shapes()
            crec, cinfo = t.read_pair_contacts()
            mrec, minfo = t.read_pair_manifolds()
            labels, edge, iinfo = t.read_pair_islands()
            tb, te, ti = t.touch_events()
            pb, pe, pi = t.pair_events()
            order = np.argsort(R.keys(lst), kind="stable")
            outs.append((R.keys(lst)[order], sinfo, K.bits(crec)[order], cinfo, M.bits(mrec)[order], minfo, labels, edge[order], iinfo,
                         np.sort(R.keys(tb)), np.sort(R.keys(te)), ti, np.sort(R.keys(pb)), np.sort(R.keys(pe)), pi))
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
        on.check()                                          # all six features in one run
        for t in ticks[1:]:
            with pytest.raises(capi.ScTickError, match="pair persistence was not enabled"):
                t.read_pair_persistence()
    for t in ticks:
        t.close()


# ---- 12. every refusal -------------------------------------------------------------------------------------------------------------
def test_pair_persistence_api_errors(oracle):
    w, col = G.agreement_world(2651, n=300)
    t = start(w, col, max_touching=64)
    t.set_pair_contacts(True)
    with pytest.raises(capi.ScTickError, match="needs scTickSetPairManifolds\\(1\\) first"):
        t.pair_persistence(True)
    t.pair_persistence(False)                               # nothing to free: welcome
    t.set_pair_manifolds(True)
    for bad in (0.0, -0.02, np.inf, -np.inf, np.nan):
        with pytest.raises(capi.ScTickError, match="match_dist must be finite and > 0"):
            t.pair_persistence(True, bad)
    assert not t.pair_persistence_enabled()
    t.run(SHAPES)                                           # the refusals changed nothing: the context still runs
    with pytest.raises(capi.ScTickError, match="pair persistence was not enabled"):
        t.read_pair_persistence()
    t.pair_persistence(True)
    assert t.pair_persistence_enabled() and t.pair_persistence_match_dist() == float(F(0.02))
    for call in (t.read_pair_persistence, t.read_pair_payloads, lambda: t.write_pair_payloads(np.zeros((1, 4, 4), F))):
        with pytest.raises(capi.ScTickError, match="pair persistence was not enabled"):      # enabled since: the last run still matched nothing
            call()
    t.run(FLAGS)
    for call in (t.read_pair_persistence, t.read_pair_payloads, lambda: t.write_pair_payloads(np.zeros((1, 4, 4), F))):
        with pytest.raises(capi.ScTickError, match="did not request SC_TICK_PAIR_SHAPES"):
            call()
    t.run(SHAPES)
    rec, info = t.read_pair_persistence()
    assert info["written"] == 64 == len(rec) and info["list_truncated"] == 1
    t.write_pair_payloads(np.ones((4, 4, 4), F), first=60)
    t.write_pair_payloads(np.zeros((0, 4, 4), F), first=64)
    with pytest.raises(capi.ScTickError, match="exceeds the records the last run wrote"):
        t.write_pair_payloads(np.ones((5, 4, 4), F), first=60)
    with pytest.raises(capi.ScTickError, match="exceeds the records the last run wrote"):
        t.write_pair_payloads(np.ones((1, 4, 4), F), first=0xFFFFFFFF)
    assert t.lib.scTickWritePairPayloads(t.ctx, None, 0, 1) == 0 and b"null argument" in t.lib.scTickGetLastError(t.ctx)
    assert t.lib.scTickReadPairPersistence(t.ctx, None, 0, None) == 0 and b"null argument" in t.lib.scTickGetLastError(t.ctx)
    assert t.lib.scTickGetPairPersistence(t.ctx, None, None) == 0 and b"null argument" in t.lib.scTickGetLastError(t.ctx)
    pinfo = capi.PairPersistInfo()
    assert t.lib.scTickReadPairPersistence(t.ctx, None, 0, C.byref(pinfo)) == 1 and pinfo.written == 64      # the report alone
    assert t.lib.scTickReadPairPayloads(t.ctx, None, 0) == 1
    t.pair_persistence(False)
    for call in (t.read_pair_persistence, t.read_pair_payloads, lambda: t.write_pair_payloads(np.zeros((1, 4, 4), F))):
        with pytest.raises(capi.ScTickError, match="pair persistence was switched off since the last scTickRun"):
            call()
    for off in (lambda: t.set_pair_manifolds(False), lambda: t.set_pair_contacts(False), lambda: t.set_pair_shapes(0)):
        t.set_pair_shapes(64); t.set_pair_contacts(True); t.set_pair_manifolds(True); t.pair_persistence(True)
        assert t.pair_persistence_enabled()
        off()                                               # each of the three switches persistence off too
        assert not t.pair_persistence_enabled()
    t.run(FLAGS)
    t.close()
