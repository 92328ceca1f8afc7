"""Pair events on the GPU against the witness (tests/pair_events_ref.py): every comparison exact, on sorted lists.  After every tick each
test also holds scTickReadPairs against the oracle's set, so that a wrong event cannot be a wrong pair set in disguise.  The scripts and
their premises are checked without a GPU in tests/test_pair_events_cpu.py."""
import numpy as np
import pytest

from sc_gameengine_amd import capi, synth_world as sw
from sc_gameengine_amd.tick import WorldTick
from tests import pair_events_ref as R, worlds

pytestmark = pytest.mark.gpu
FLAGS = capi.XFORM | capi.BROADPHASE
EV = FLAGS | capi.PAIR_EVENTS
F = np.float32


def check_pairs(t, want):
    got, total = t.pairs()
    assert total == len(want), f"pair count {total} != {len(want)}"
    assert np.array_equal(R.sorted_pairs(got), want)


def check_events(t, wt, want, pairs_truncated=False):
    """the library's report of the last flagged tick against the witness's for the oracle's set `want`; returns the witness's answer"""
    wb, we, wi = wt.tick(want, pairs_truncated)
    b, e, info = t.pair_events()
    assert info == wi, f"{info} != {wi}"
    for got, full, name in ((b, wb, "begun"), (e, we, "ended")):
        if len(full) > wt.max_events:                      # a truncated list: max_events distinct members of the true set
            assert len(got) == wt.max_events and len(np.unique(R.keys(got))) == wt.max_events, name
            assert np.isin(R.keys(got), R.keys(full)).all(), name
        else:
            assert np.array_equal(R.sorted_pairs(got), full), name
        assert (got[:, 0] < got[:, 1]).all()
    return wb, we, wi


def start(oracle, name, max_tracked, max_events, max_pairs=1 << 16):
    w, steps, sets = R.script_sets(oracle, name)
    t = WorldTick.from_world(w, broadphase=True, max_pairs=max_pairs)
    t.set_pair_events(max_tracked, max_events)
    return t, steps, sets, R.Witness(max_tracked, max_events)


def run_script(t, wt, steps, sets, ticks=None, run=None):
    infos = []
    for k in range(ticks or len(steps)):
        if steps[k] is not None:
            t.upload_positions(0, steps[k])
        (run or (lambda: t.run(EV)))()
        check_pairs(t, sets[k])
        infos.append(check_events(t, wt, sets[k])[2])
    return infos


# ---- 1. a hand-built line of boxes -----------------------------------------------------------------------------------------------
def test_line_of_boxes_exact_lists_on_every_tick(oracle):
    t, steps, sets, wt = start(oracle, "line", 64, 64)
    for k, (wb, we) in enumerate(R.LINE_EVENTS):
        if steps[k] is not None:
            t.upload_positions(0, steps[k])
        t.run(EV)
        check_pairs(t, sets[k])
        b, e, info = t.pair_events()
        assert R.sorted_pairs(b).tolist() == [list(p) for p in wb] and R.sorted_pairs(e).tolist() == [list(p) for p in we]
        assert info == dict(begun=len(wb), ended=len(we), tracked=len(sets[k]), resync=int(k == 0), overflow=0, events_truncated=0)
        check_events(t, wt, sets[k])
    t.close()


# ---- 2. random motion ------------------------------------------------------------------------------------------------------------
def test_random_motion_events_replay_into_the_oracles_set(oracle):
    t, steps, sets, wt = start(oracle, "random", 4096, 4096)
    live = set()
    for k in range(len(steps)):
        if steps[k] is not None:
            t.upload_positions(0, steps[k])
        t.run(EV)
        check_pairs(t, sets[k])
        check_events(t, wt, sets[k])
        b, e, info = t.pair_events()                      # the host's pair cache: ended out, begun in (cleared first on a resync)
        if info["resync"]:
            live.clear()
        live -= set(map(tuple, e.tolist()))
        live |= set(map(tuple, b.tolist()))
        assert k == 0 or (info["begun"] >= 1 and info["ended"] >= 1)
    assert live == set(map(tuple, sets[-1].tolist()))
    t.close()


# ---- 3. the table at its limit ---------------------------------------------------------------------------------------------------
def test_table_at_its_limit(oracle):
    t, steps, sets, wt = start(oracle, "crowded", R.CROWDED_MAX_TRACKED, 1024)
    infos = run_script(t, wt, steps, sets)
    assert all(0.9 * R.CROWDED_MAX_TRACKED <= i["tracked"] <= R.CROWDED_MAX_TRACKED for i in infos)
    assert t.counts().bin_overflow > 200                  # (and the pair search went through its slow path)
    t.close()


# ---- 4. overflow and recovery ----------------------------------------------------------------------------------------------------
def test_overflow_drops_the_set_and_the_next_tick_resyncs(oracle):
    t, steps, sets, wt = start(oracle, "cluster", R.CLUSTER_MAX_TRACKED, 64)
    infos = run_script(t, wt, steps, sets)
    assert [i["overflow"] for i in infos] == [0, 1, 0, 0] and [i["resync"] for i in infos] == [1, 0, 1, 0]
    assert infos[1] == dict(begun=0, ended=0, tracked=0, resync=0, overflow=1, events_truncated=0)
    assert infos[2]["begun"] == len(sets[2]) and infos[2]["ended"] == 0
    t.close()


def test_a_truncated_pair_list_is_an_overflow(oracle):
    w, steps, sets = R.script_sets(oracle, "small")
    t = WorldTick.from_world(w, broadphase=True, max_pairs=64)
    t.set_pair_events(4096, 4096)                         # the tables would take the set: the pair list does not
    wt = R.Witness(4096, 4096)
    for k in range(2):
        if steps[k] is not None:
            t.upload_positions(0, steps[k])
        t.run(EV)
        c = t.counts()
        assert c.pairs == len(sets[k]) and c.pairs_truncated == 1
        _, _, wi = check_events(t, wt, sets[k], pairs_truncated=True)
        assert wi["overflow"] == 1
    t.close()


# ---- 5. event-list truncation ----------------------------------------------------------------------------------------------------
def test_event_lists_truncate_with_true_totals_and_the_set_stays_whole(oracle):
    t, steps, sets, wt = start(oracle, "cluster", 1024, R.TRUNCATION_MAX_EVENTS)
    infos = run_script(t, wt, steps, sets)                # (check_events: max_events distinct members of the true sets on the truncated ticks)
    assert infos[1]["begun"] >= 20 and infos[1]["events_truncated"] == 1
    assert infos[2]["ended"] >= 20 and infos[2]["events_truncated"] == 1
    assert infos[3]["events_truncated"] == 0 and infos[3]["begun"] + infos[3]["ended"] >= 1      # the next tick's events are the witness's, exactly
    t.close()


# ---- 6. renames ------------------------------------------------------------------------------------------------------------------
def test_removals_resync_and_appends_arrive_as_events(oracle):
    rng = np.random.default_rng(17)
    w = worlds.random_world(1200, seed=42, spread=40.0, p_child=0.0)
    t = WorldTick.from_world(w, broadphase=True, capacity=w.n, max_pairs=1 << 16)
    t.set_pair_events(8192, 8192)
    wt = R.Witness(8192, 8192)

    def tick(world):
        ow = worlds.oracle_world(oracle, world, camera=False)
        ow.transform_system()
        want = R.oracle_pairs(oracle, ow, world)
        ow.close()
        t.run(EV)
        check_pairs(t, want)
        return check_events(t, wt, want)

    assert tick(w)[2]["resync"] == 1
    assert tick(w)[2] == dict(begun=0, ended=0, tracked=wt.prev.size, resync=0, overflow=0, events_truncated=0)
    # a removal that relocates entities: dense indices are renamed, the next flagged tick starts over against the renamed world
    gone = rng.choice(w.n, 200, replace=False).astype(np.uint32)
    src, dst = t.remove_entities(gone)
    assert len(src) > 50
    names = ("pos", "rot", "scale", "bmin", "bmax", "has_bounds", "has_mesh", "group", "mask", "mesh", "material")
    a = {k: getattr(w, k).copy() for k in names}
    for v in a.values():
        v[dst] = v[src]
    n1 = w.n - 200

    def world_of(n):
        return sw.SynthWorld(parent=np.full(n, -1, np.int32), sector_of=np.zeros((n, 2), np.int32), origin=w.origin, sectors=w.sectors,
                             **{k: v[:n] for k, v in a.items()})

    wt.invalidate()
    wb, _, wi = tick(world_of(n1))
    assert wi["resync"] == 1 and wi["begun"] == len(wb) > 100 and wi["ended"] == 0
    # appended entities rename nothing: their pairs simply begin
    k = 150
    add = dict(pos=rng.uniform(-35, 35, (k, 3)).astype(F), rot=rng.uniform(-3, 3, (k, 3)).astype(F), scale=rng.uniform(0.5, 2.0, (k, 3)).astype(F),
               bmin=-rng.uniform(0.5, 2.0, (k, 3)).astype(F), bmax=rng.uniform(0.5, 2.0, (k, 3)).astype(F), has_bounds=np.ones(k, np.uint8),
               has_mesh=np.ones(k, np.uint8), group=np.full(k, 1, np.uint32), mask=np.full(k, 0xFFFFFFFF, np.uint32), mesh=np.zeros(k, np.uint32),
               material=np.zeros(k, np.uint32))
    first = t.append_entities(add["pos"], add["rot"], add["scale"], bmin=add["bmin"], bmax=add["bmax"], mesh=add["mesh"], material=add["material"],
                              group=add["group"], mask=add["mask"])
    assert first == n1
    a = {key: np.concatenate([v[:n1], add[key]]) for key, v in a.items()}
    wb, we, wi = tick(world_of(n1 + k))
    assert wi["resync"] == 0 and len(we) == 0 and len(wb) >= 1 and (wb[:, 1] >= n1).all()
    # a shrinking count invalidates indices too
    t.set_count(n1 + k - 50)
    wt.invalidate()
    assert tick(world_of(n1 + k - 50))[2]["resync"] == 1
    t.close()


# ---- 7. unflagged ticks in between -----------------------------------------------------------------------------------------------
def test_unflagged_ticks_leave_the_remembered_set_alone(oracle):
    t, steps, sets, wt = start(oracle, "small", 1024, 1024)
    for k in range(4):
        if steps[k] is not None:
            t.upload_positions(0, steps[k])
        flagged = k in (0, 3)
        t.run(EV if flagged else FLAGS)
        check_pairs(t, sets[k])
        if flagged:
            wb, we, wi = check_events(t, wt, sets[k])      # (the witness never saw ticks 1 and 2: tick 3 is held against tick 0)
        else:
            with pytest.raises(capi.ScTickError, match="did not request SC_TICK_PAIR_EVENTS"):
                t.pair_events()
    assert wi["resync"] == 0 and len(wb) + len(we) >= 1
    t.close()


# ---- 8. graph mode ---------------------------------------------------------------------------------------------------------------
def test_replayed_graphs_read_their_counts_on_the_device(oracle):
    t, steps, sets, wt = start(oracle, "small", 1024, 1024)
    t.set_graph_mode(True)
    infos = run_script(t, wt, steps, sets, ticks=8)
    assert infos[0]["resync"] == 1 and sum(i["begun"] + i["ended"] for i in infos[1:]) >= 2
    t.close()


# ---- 9. split tick on a lone context ---------------------------------------------------------------------------------------------
def test_split_tick_reports_after_run_pairs(oracle):
    t, steps, sets, wt = start(oracle, "small", 1024, 1024)

    def split():
        t.run(EV | capi.SPLIT_PAIRS)
        with pytest.raises(capi.ScTickError, match="after scTickRunPairs"):
            t.pair_events()
        t.run_pairs()

    infos = run_script(t, wt, steps, sets, ticks=4, run=split)
    # the same answers as the plain tick's
    p, _, _, pw = start(oracle, "small", 1024, 1024)
    assert run_script(p, pw, steps, sets, ticks=4) == infos
    t.close(); p.close()


def test_a_rename_between_the_halves_of_a_split_tick_still_resyncs(oracle):
    """caller-owned split flow: entities removed between scTickRun(.. | SPLIT_PAIRS) and scTickRunPairs -- the remembered set is dropped at
    once, so the pending pair half is a resync tick in the ids of its own tick, and what it remembers is forgotten again behind it: the
    next flagged tick is a resync tick too; a changed rank renames every id as well"""
    t, steps, sets, wt = start(oracle, "line", 64, 64)
    t.run(EV)
    assert t.pair_events()[2]["resync"] == 1
    t.run(EV | capi.SPLIT_PAIRS)
    t.remove_entities(np.uint32([5]))                     # the last box: in no pair, nothing relocates -- the set stays {(0, 1)}
    t.run_pairs()
    b, e, info = t.pair_events()                          # (the rename already dropped the remembered set: the pending half starts over, in its tick's ids)
    assert info == dict(begun=1, ended=0, tracked=1, resync=1, overflow=0, events_truncated=0) and b.tolist() == [[0, 1]]
    t.run(EV)
    check_pairs(t, sets[0])
    b, e, info = t.pair_events()
    assert info == dict(begun=1, ended=0, tracked=1, resync=1, overflow=0, events_truncated=0) and b.tolist() == [[0, 1]]
    t.set_tile(3, 0)
    t.run(EV)
    b, e, info = t.pair_events()
    assert info["resync"] == 1 and info["ended"] == 0 and b.tolist() == [[3 << 24, 3 << 24 | 1]]
    t.close()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_carry_the_librarys_message(oracle):
    w, steps, sets = R.script_sets(oracle, "line")
    t = WorldTick.from_world(w, broadphase=True)
    with pytest.raises(capi.ScTickError, match="needs scTickSetPairEvents first"):
        t.run(EV)
    t.set_pair_events(64, 64)
    with pytest.raises(capi.ScTickError, match="needs SC_TICK_BROADPHASE"):
        t.run(capi.XFORM | capi.PAIR_EVENTS)
    t.run(EV)
    assert t.pair_events()[2]["resync"] == 1
    t.run(FLAGS)
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_PAIR_EVENTS"):
        t.pair_events()
    with pytest.raises(capi.ScTickError, match="both positive, or both 0"):
        t.set_pair_events(64, 0)
    t.set_pipelined(True)
    with pytest.raises(capi.ScTickError, match="pipelined context"):
        t.run(EV | capi.SPLIT_PAIRS)
    t.set_pipelined(False)
    t.run(EV)                                             # (switching the pipeline off again leaves the events usable)
    check_pairs(t, sets[0])
    t.set_pair_events(0, 0)
    with pytest.raises(capi.ScTickError, match="pair events were switched off since the last scTickRun"):
        t.pair_events()
    with pytest.raises(capi.ScTickError, match="needs scTickSetPairEvents first"):
        t.run(EV)
    t.set_pair_events(64, 64)
    t.run(FLAGS | capi.SPLIT_PAIRS)
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_PAIR_EVENTS"):      # the missing flag is named before the pending half
        t.pair_events()
    t.run_pairs()
    t.run(EV | capi.SPLIT_PAIRS)
    with pytest.raises(capi.ScTickError, match="pair events are ready after scTickRunPairs"):
        t.pair_events()
    t.run_pairs()
    t.pair_events()                                       # ... and readable behind it
    t.close()
