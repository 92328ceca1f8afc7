"""Pair events without a GPU: the ABI surface, the witness (tests/pair_events_ref.py) on hand-written sets, and every scripted world of
tests/test_gpu_pair_events.py checked for what its GPU test relies on -- if a seed drifts, this file fails, not the GPU test's premise."""
import ctypes as C

import numpy as np

from sc_gameengine_amd import capi
from tests import pair_events_ref as R

U = np.uint32


def P(*pairs):
    return np.array(pairs, U).reshape(-1, 2)


def test_pair_event_symbols_are_exported_and_bound():
    lib = capi.load()
    for name in ("scTickSetPairEvents", "scTickReadPairEvents"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert capi.PAIR_EVENTS == 1 << 12 and not (capi.FULL & capi.PAIR_EVENTS)
    assert lib.scTickGetApiVersion() == 7
    assert C.sizeof(capi.PairEventInfo) == 24
    assert [n for n, _ in capi.PairEventInfo._fields_] == ["begun", "ended", "tracked", "resync", "overflow", "events_truncated"]
    info = capi.PairEventInfo()
    assert lib.scTickSetPairEvents(None, 16, 16) == 0
    assert lib.scTickReadPairEvents(None, None, 0, None, 0, C.byref(info)) == 0


def test_witness_on_hand_written_sets():
    wt = R.Witness(max_tracked=4, max_events=2)
    a = P((0, 1), (2, 3))
    b, e, i = wt.tick(a)                                   # first tick: resync, everything begins
    assert np.array_equal(b, a) and len(e) == 0 and i == dict(begun=2, ended=0, tracked=2, resync=1, overflow=0, events_truncated=0)
    b, e, i = wt.tick(a)                                   # a still tick
    assert len(b) == 0 and len(e) == 0 and i == dict(begun=0, ended=0, tracked=2, resync=0, overflow=0, events_truncated=0)
    b, e, i = wt.tick(P((0, 1), (2, 5), (4, 5)))           # (2,3) ends, two begin
    assert np.array_equal(b, P((2, 5), (4, 5))) and np.array_equal(e, P((2, 3))) and i["tracked"] == 3 and not i["events_truncated"]
    b, e, i = wt.tick(P((0, 1), (0, 2), (0, 3), (0, 4), (0, 5)))      # five pairs do not fit four: overflow, nothing listed, nothing kept
    assert len(b) == 0 and len(e) == 0 and i == dict(begun=0, ended=0, tracked=0, resync=0, overflow=1, events_truncated=0)
    b, e, i = wt.tick(P((0, 1)))                           # the next tick that fits is a resync tick
    assert np.array_equal(b, P((0, 1))) and len(e) == 0 and i["resync"] == 1
    b, e, i = wt.tick(P((1, 2), (1, 3), (1, 4)))           # three begin with room for two: true totals, the flag
    assert i == dict(begun=3, ended=1, tracked=3, resync=0, overflow=0, events_truncated=1) and len(b) == 3
    b, e, i = wt.tick(P((1, 2)))                           # ... and the set was remembered in full
    assert len(b) == 0 and np.array_equal(e, P((1, 3), (1, 4))) and not i["events_truncated"]
    b, e, i = wt.tick(P((1, 2)), pairs_truncated=True)     # a truncated pair list is an overflow whatever its length
    assert i["overflow"] == 1 and i["tracked"] == 0
    wt.tick(P((1, 2)))
    wt.invalidate()                                        # a rename
    b, e, i = wt.tick(P((1, 2), (0, 7)))
    assert i["resync"] == 1 and np.array_equal(b, P((0, 7), (1, 2))) and len(e) == 0      # lists come out sorted by key
    # key order: the high word is a
    assert np.array_equal(R.sorted_pairs(P((1, 0xFFFFFFFF), (0, 5), (1, 2))), P((0, 5), (1, 2), (1, 0xFFFFFFFF)))


def events_of(sets, max_tracked=1 << 30, max_events=1 << 30):
    wt = R.Witness(max_tracked, max_events)
    return [wt.tick(s) for s in sets]


def test_line_script_is_what_its_test_says(oracle):
    w, steps, sets = R.script_sets(oracle, "line")
    assert w.n == 6 and len(steps) == len(R.LINE_EVENTS) == 4
    assert [0, 1] in sets[0].tolist()                      # the pair whose key has a zero high word
    for (b, e, i), (wb, we) in zip(events_of(sets), R.LINE_EVENTS):
        assert b.tolist() == [list(p) for p in wb] and e.tolist() == [list(p) for p in we]


def test_random_run_has_a_begun_and_an_ended_pair_on_every_tick(oracle):
    w, steps, sets = R.script_sets(oracle, "random")
    assert w.n == 3000 and len(sets) == 12
    ev = events_of(sets)
    assert ev[0][2]["resync"] == 1 and ev[0][2]["begun"] == len(sets[0]) > 1000
    for b, e, i in ev[1:]:
        assert i["begun"] >= 1 and i["ended"] >= 1
    # the small run (graph mode: 8 ticks; split tick, unflagged ticks in between: the first 4): events of both kinds inside the first four
    # ticks, and the sets of ticks 0 and 3 differ (the diff over two unflagged ticks is not empty)
    ws, _, small = R.script_sets(oracle, "small")
    ev = events_of(small)
    assert ws.n == 600 and len(small) == 8
    assert sum(i["begun"] for _, _, i in ev[1:4]) >= 1 and sum(i["ended"] for _, _, i in ev[1:4]) >= 1
    assert sum(i["begun"] + i["ended"] for _, _, i in ev[4:]) >= 1
    b, e, _ = events_of([small[0], small[3]])[1]
    assert len(b) + len(e) >= 1


def test_crowded_world_fills_its_table(oracle):
    w, steps, sets = R.script_sets(oracle, "crowded")
    assert len(sets) == 6
    for s in sets:
        assert 0.9 * R.CROWDED_MAX_TRACKED <= len(s) <= R.CROWDED_MAX_TRACKED
    for b, e, i in events_of(sets, R.CROWDED_MAX_TRACKED)[1:]:
        assert i["overflow"] == 0 and i["begun"] >= 10 and i["ended"] >= 10
    # the tables as the kernels fill them (TableModel: same hash, same probing): 2 x max_tracked slots, a load factor just under one half,
    # long probe runs, and on EVERY tick a run that crosses the table's end -- keys whose home is in the last slots land at slot 0 or
    # later (how many keys a run pushes past the end does not depend on the insertion order) -- which later ticks look up past the wrap too
    m = R.TableModel(R.CROWDED_MAX_TRACKED, 1024)
    stats = [m.tick(s)[3] for s in sets]
    assert all(st["slots"] == 2 * R.CROWDED_MAX_TRACKED and 0.45 <= st["load"] <= 0.5 for st in stats)
    assert all(st["longest_insert_probe"] >= 10 for st in stats)
    assert all(st["insert_wraps"] >= 1 for st in stats) and sum(st["lookup_wraps"] for st in stats[1:]) >= 1


def test_table_model_reproduces_the_witness_on_every_script(oracle):
    """The kernels' algorithm restated on the host (tests/pair_events_ref.py TableModel) gives the witness's lists and reports on every
    script the GPU tests run, at the capacities they run them with: the scheme itself is right, whatever the device then does with it."""
    for name, mt, me in (("line", 64, 64), ("random", 4096, 4096), ("small", 1024, 1024), ("crowded", R.CROWDED_MAX_TRACKED, 1024),
                         ("cluster", R.CLUSTER_MAX_TRACKED, 64), ("cluster", 1024, R.TRUNCATION_MAX_EVENTS)):
        sets = R.script_sets(oracle, name)[2]
        m, wt = R.TableModel(mt, me), R.Witness(mt, me)
        for s in sets:
            b, e, info, _ = m.tick(s)
            wb, we, wi = wt.tick(s)
            assert info == wi and b == R.keys(wb).tolist() and e == R.keys(we).tolist(), name
    m, wt = R.TableModel(4096, 4096), R.Witness(4096, 4096)               # a truncated pair list
    s = R.script_sets(oracle, "small")[2][0]
    assert m.tick(s, pairs_truncated=True)[2] == wt.tick(s, pairs_truncated=True)[2]
    assert m.tick(s)[2] == wt.tick(s)[2] and m.tick(s)[2]["resync"] == 0


def test_cluster_script_crosses_the_capacity_on_one_tick_only(oracle):
    w, steps, sets = R.script_sets(oracle, "cluster")
    sizes = [len(s) for s in sets]
    assert len(sizes) == 4
    assert sizes[0] <= R.CLUSTER_MAX_TRACKED < sizes[1] and sizes[2] <= R.CLUSTER_MAX_TRACKED and sizes[3] <= R.CLUSTER_MAX_TRACKED
    ev = [i for _, _, i in events_of(sets, R.CLUSTER_MAX_TRACKED)]
    assert [i["overflow"] for i in ev] == [0, 1, 0, 0] and [i["resync"] for i in ev] == [1, 0, 1, 0]
    assert ev[2]["begun"] == sizes[2] and ev[3]["begun"] + ev[3]["ended"] >= 1      # the last tick is an ordinary diff that reports something
    # the truncation test runs the same script with room for every pair and for TRUNCATION_MAX_EVENTS events
    ev = [i for _, _, i in events_of(sets, 1024, R.TRUNCATION_MAX_EVENTS)]
    assert ev[1]["begun"] >= 20 and ev[1]["events_truncated"] == 1 and ev[2]["ended"] >= 20 and ev[2]["events_truncated"] == 1
    assert ev[3]["events_truncated"] == 0 and ev[3]["begun"] + ev[3]["ended"] >= 1
    # and the small run's set does not fit a pair list of 64: pairs_truncated, hence overflow
    assert len(R.script_sets(oracle, "small")[2][0]) > 64
