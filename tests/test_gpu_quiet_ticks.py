"""Quiet ticks (include/sc_tick.h, scTickGetBinStats): a broadphase tick of a world that cannot pair, whose bins
nothing else reads, does the device work of the same call without SC_TICK_BROADPHASE.  Against the oracle, and against a twin
context created under SC_TICK_VARIANT=8, which fills and sweeps the bins on every tick as before.

Worlds and the oracle side: tests/quiet_ticks_cases.py (12 x 12 sectors, 2 304 entities, spans of three tiles)."""
import numpy as np
import pytest

from sc_gameengine_amd import capi
from sc_gameengine_amd.tick import WorldTick
from tests import quiet_ticks_cases as qc

pytestmark = pytest.mark.gpu

FULLP = capi.FULL | capi.PRODUCE_NEXT
COUNT_FIELDS = [n for n, _ in capi.Counts._fields_]


def make(monkeypatch, w, quiet=True, dx=qc.DX, capacity=None, **kw):
    monkeypatch.setenv("SC_TICK_SPANS", qc.SPANS)
    monkeypatch.setenv("SC_TICK_VARIANT", "0" if quiet else "8")
    t = WorldTick.from_world(w, broadphase=True, capacity=capacity, **kw)
    monkeypatch.delenv("SC_TICK_SPANS"); monkeypatch.delenv("SC_TICK_VARIANT")
    t.set_view_proj(qc.camera_view_proj(w.camera))
    t.set_frame_producer(1, float(dx))
    return t


def pair_keys(p):
    p = np.asarray(p, np.uint32).reshape(-1, 2)
    return np.sort(p[:, 0].astype(np.uint64) << np.uint64(32) | p[:, 1].astype(np.uint64))


def is_quiet(t):
    return t.bin_stats()["quiet_last_tick"]


def counts_of(t):
    c = t.counts()
    return {f: int(getattr(c, f)) for f in COUNT_FIELDS}


def assert_oracle(t, side, pairs=True):
    assert np.array_equal(t.world_matrices(), side.matrices())                 # IEEE equality, as test_gpu_parity
    assert np.array_equal(t.visible(), side.visible())
    if pairs:
        want = side.pairs()
        got, total = t.pairs()
        assert total == len(want) and np.array_equal(pair_keys(got), pair_keys(want))
        c = t.counts()
        assert c.pairs == len(want) and c.pairs_truncated == 0


def assert_twins(a, b, rays=False):
    """everything a caller reads back, identical in both forms"""
    assert np.array_equal(a.world_matrices().view(np.uint32), b.world_matrices().view(np.uint32))
    assert np.array_equal(a.visible(), b.visible())
    assert np.array_equal(a.positions().view(np.uint32), b.positions().view(np.uint32))
    assert np.array_equal(a.dirty(), b.dirty())
    assert counts_of(a) == counts_of(b)
    pa, ta = a.pairs(); pb, tb = b.pairs()
    assert ta == tb and np.array_equal(pair_keys(pa), pair_keys(pb))
    if rays:
        assert a.ray_hits().tobytes() == b.ray_hits().tobytes()


def assert_ray_hits(got, want):
    """every field as a bit pattern (tests/test_gpu_rays.py)"""
    assert len(got) == len(want)
    for f in ("hit", "id", "layer"):
        assert np.array_equal(got[f], want[f]), f
    for f in ("distance", "position", "normal"):
        a, b = got[f][got["hit"] == 1], want[f][want["hit"] == 1]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f


def test_quiet_stretch_of_forty_ticks(monkeypatch, oracle):
    """The headline's tick on a small world: after the learn tick every tick is quiet, no learn tick falls into the stretch, and what
    a caller reads is the oracle's on every 8th tick and the last -- with an empty pair set."""
    w = qc.world()
    side = qc.OracleSide(oracle, w)
    t = make(monkeypatch, w)
    for k in range(40):
        side.tick()
        t.run(FULLP)
        assert is_quiet(t) == (k >= 1), f"tick {k}"
        if k % 8 == 0 or k == 39:
            assert_oracle(t, side)
            got, total = t.pairs()
            assert total == 0 and len(got) == 0 and len(side.pairs()) == 0
        side.produce(qc.DX)
    assert t.learn_ticks() == 1
    bs = t.bin_stats()
    assert bs["pair_role_sweep_only"] and bs["remembered_slots"] > 0             # (the other fields tell of the tick that binned)
    t.close(); side.close()


def test_boxes_that_moved_while_nobody_looked(monkeypatch, oracle):
    """Roots move 2.3 m per tick through ten quiet ticks: boxes cross sectors and no record follows.  The ray tick behind them must find
    every box where it is now; so must a second one that comes behind a quiet tick whose transforms moved the boxes a last time and left
    nothing dirty (no entity is rebuilt on it: every always-written slot must be rewritten all the same)."""
    w, rays, want, boxes = qc.moved_boxes_expectation(oracle)
    assert all(h["hit"].sum() > qc.RAYS // 2 for h in want) and want[0].tobytes() != want[1].tobytes()
    t, twin = make(monkeypatch, w, True, qc.DX_FAR), make(monkeypatch, w, False, qc.DX_FAR)
    for c in (t, twin):
        c.set_ray_queries(*rays)                                # before the first tick: the batch's buffers exist when the slots are learnt
    seen, producing = 0, True
    for k, (kind, produce) in enumerate(qc.MOVED_SEQUENCE):
        if producing and not produce:
            for c in (t, twin):
                c.set_frame_producer(0)                          # (a run without PRODUCE_NEXT would launch a set producer ahead of the tick)
            producing = False
        if kind == "rays" and not produce:
            assert not t.dirty().any() and not twin.dirty().any()         # the second ray tick rebuilds nothing
        flags = capi.FULL | (capi.PRODUCE_NEXT if produce else 0) | (capi.RAYS if kind == "rays" else 0)
        t.run(flags); twin.run(flags)
        assert is_quiet(t) == (kind == "quiet" and k >= 1) and not is_quiet(twin), f"tick {k}"
        if kind == "rays":
            assert t.bin_stats()["unchanged_records_stay"] is False and t.learn_ticks() == 1
            assert_ray_hits(t.ray_hits(), want[seen])
            assert_twins(t, twin, rays=True)
            seen += 1
    assert seen == 2
    t.close(); twin.close()


@pytest.mark.parametrize("how", ["layers", "append"])
def test_becoming_pairable_and_back(monkeypatch, oracle, how):
    """Five quiet ticks, then the world can pair -- one prop per sector becomes a dynamic body, or one dynamic entity is appended -- and
    the next ticks bin and find the oracle's pairs; the change is taken back and quiet ticks resume with an empty pair set."""
    w = qc.world()
    side = qc.OracleSide(oracle, w)
    t = make(monkeypatch, w, capacity=w.n + 8, max_pairs=1 << 16)

    def ticks(count, quiet_from, expect_pairs):
        for k in range(count):
            side.tick()
            t.run(FULLP)
            assert is_quiet(t) == (k >= quiet_from), f"tick {k}"
            assert_oracle(t, side)
            assert (t.counts().pairs > 0) == expect_pairs
            side.produce(qc.DX)

    ticks(6, 1, False)                                           # the learn tick and five quiet ticks
    if how == "layers":
        w2 = qc.world()
        qc.make_dynamic(w2, qc.dynamic_parents(w2.n))             # (the prop of every sector whose child sits in its box: pairs everywhere)
        t.upload_layers(0, w2.group, w2.mask)
    else:
        r = int(np.flatnonzero((w.parent < 0) & (w.has_bounds == 1))[37])
        w2 = qc.with_dynamic_entity(qc.world(), side.pos[r])      # on top of a prop, in the last span alone
        assert t.append_entities(w2.pos[-1:], w2.rot[-1:], w2.scale[-1:], w2.bmin[-1:], w2.bmax[-1:], w2.mesh[-1:], w2.material[-1:],
                                 w2.group[-1:], w2.mask[-1:]) == w.n
    side.replace_world(w2)
    ticks(3, 99, True)                                           # never quiet: a learn tick, then ticks that search
    if how == "layers":
        t.upload_layers(0, w.group, w.mask)
    else:
        src, dst = t.remove_entities([w.n])
        assert len(src) == 0                                     # the last entity: nothing moves
    side.replace_world(qc.world())
    ticks(4, 1, False)                                           # a learn tick, then quiet again
    assert t.learn_ticks() == 3
    t.close(); side.close()


def _sensors(t, w):
    zeros = np.zeros(w.n, np.float32)
    t.upload_traffic_agents(0, np.zeros(w.n, np.uint8), np.zeros(w.n, np.uint32), zeros, zeros, np.zeros(w.n, np.uint8))
    t.set_traffic_sensors(True)


@pytest.mark.parametrize("case", ["can_pair", "sensors", "split_pairs", "dense_aabbs", "pair_events"])
def test_not_eligible(monkeypatch, case):
    """Each of these alone keeps every tick a binning one, with the outputs of the form that never takes a quiet tick."""
    w = qc.world()
    if case == "can_pair":
        qc.make_dynamic(w, qc.dynamic_rule(w.n))
    t, twin = make(monkeypatch, w, True, max_pairs=1 << 16), make(monkeypatch, w, False, max_pairs=1 << 16)
    flags = FULLP | {"split_pairs": capi.SPLIT_PAIRS, "dense_aabbs": capi.DENSE_AABBS, "pair_events": capi.PAIR_EVENTS}.get(case, 0)
    for c in (t, twin):
        if case == "sensors":
            _sensors(c, w)
        if case == "pair_events":
            c.set_pair_events(1 << 12, 1 << 12)
    for k in range(5):
        for c in (t, twin):
            c.run(flags)
            if case == "split_pairs":
                c.run_pairs()
        assert not is_quiet(t) and not is_quiet(twin), f"tick {k}"
        assert_twins(t, twin)
        if case == "dense_aabbs":
            (amn, amx), (bmn, bmx) = t.world_aabbs(), twin.world_aabbs()
            assert amn.tobytes() == bmn.tobytes() and amx.tobytes() == bmx.tobytes()
        if case == "pair_events":
            ea, eb = t.pair_events(), twin.pair_events()
            assert ea[2] == eb[2] and np.array_equal(pair_keys(ea[0]), pair_keys(eb[0])) and np.array_equal(pair_keys(ea[1]), pair_keys(eb[1]))
    assert t.counts().pairs == 0                                 # (config3dyn's bodies meet nothing at this size: eligibility goes by the layer words)
    assert t.learn_ticks() == twin.learn_ticks() == 1
    t.close(); twin.close()


def test_graph_mode_keeps_quiet_and_binning_ticks_apart(monkeypatch, oracle):
    """Graph replay: six quiet ticks, a ray tick, six quiet ticks.  The quiet tick's graph is its own -- the ray tick neither replays it
    nor is replayed for it -- and everything read back equals the eager run's, and the oracle's."""
    w = qc.world()
    side = qc.OracleSide(oracle, w)
    side.tick()                                                  # (the loop's first tick finds nothing left to do: the same frame)
    rays = qc.rays_through(*side.boxes(), w.has_bounds, w.parent)
    t, eager = make(monkeypatch, w), make(monkeypatch, w)
    t.set_graph_mode(True)
    for c in (t, eager):
        c.set_ray_queries(*rays)
    for k in range(13):
        flags = FULLP | (capi.RAYS if k == 6 else 0)
        side.tick()
        t.run(flags); eager.run(flags)
        assert is_quiet(t) == is_quiet(eager) == (k >= 1 and k != 6), f"tick {k}"
        assert_twins(t, eager, rays=(k == 6))
        if k in (0, 5, 6, 7, 12):
            assert_oracle(t, side)
        if k == 6:
            want = side.ray_hits(rays)
            assert want["hit"].sum() > qc.RAYS // 2
            assert_ray_hits(t.ray_hits(), want)
        side.produce(qc.DX)
    assert t.learn_ticks() == eager.learn_ticks() == 1
    t.close(); eager.close(); side.close()


def test_both_forms_agree(monkeypatch):
    """Twenty ticks of the headline's step with quiet ticks and without: every field of the counts, the matrices, the visible list."""
    w = qc.world()
    t, twin = make(monkeypatch, w, True), make(monkeypatch, w, False)
    for k in range(20):
        t.run(FULLP); twin.run(FULLP)
        assert is_quiet(t) == (k >= 1) and not is_quiet(twin)
        assert_twins(t, twin)
    assert t.counts().visible > 0
    t.close(); twin.close()
