"""The oracle side of every case of tests/test_gpu_wave_chains.py, without a device.  The eligibility rule of the cooperative form is
restated on the parent arrays (wave_chain_cases.tops / cooperative), and for every case it is asserted which wave-tiles take which
form on which tick, so that each case has what it is there for: chains with the parent in a lower and in a higher lane, the one link
that leaves its wave-tile and where it leads, a wave-tile in which all lanes but one qualify, neighbours that alternate, a partial
last wave-tile, spans of one tile, a cycle, a stale seed in the child's own wave-tile.  Across the set both forms occur, and lanes
with top 0, 1, 2 and 3 occur under the cooperative form.  A GPU test that passes on a world without its property would prove nothing."""
import numpy as np
import pytest

from oracle import oracle_np as onp
from sc_gameengine_amd import capi
from tests import test_tile_pipeline_cpu as tpc, wave_chain_cases as wc, worlds

WAVE = wc.WAVE
IDENT = np.eye(4, dtype=np.float32).ravel()
SEEN = {"coop_tops": set(), "forms": set()}        # filled by the cases, read by the last test of the file


def test_the_table_covers_what_the_issue_lists():
    by = {c.name: c for c in wc.CASES}
    inst = {(c.depth, c.flags, c.tail) for c in wc.CASES if c.name.startswith("in-wave-depth")}
    assert inst == {(d, f, t) for d in (1, 2, 3) for f in ("xform", "xform-cull") for t in (True, False)}
    assert by["in-wave-quiet"].flags == "quiet" and by["in-wave-quiet-graph"].graph and by["depth0"].depth == 0
    link = {n: by[n].links[0] for n in ("lane63-under-lane0", "other-wave", "tile-before", "tile-behind", "other-span", "all-but-one")}
    child, parent = link["lane63-under-lane0"]
    assert parent % WAVE == 63 and child == parent + 1
    child, parent = link["other-wave"]
    assert child // wc.TILE == parent // wc.TILE and abs(child // WAVE - parent // WAVE) > 1
    span = 2 * wc.TILE
    child, parent = link["tile-before"]
    assert parent // wc.TILE == child // wc.TILE - 1 and parent // span == child // span
    child, parent = link["tile-behind"]
    assert parent // wc.TILE == child // wc.TILE + 1 and parent // span == child // span
    child, parent = link["other-span"]
    assert parent // span != child // span and not by["other-span"].closed
    assert len(by["alternate"].links) == 10 and by["n100"].n == 100 and by["n257"].n % WAVE == 1 and by["n193-xform"].n % WAVE == 1
    assert by["one-tile-spans"].tiles == 1 and by["one-tile-spans"].spans == 3 and by["cycle"].cycle
    assert all(200 <= c.n <= 2048 or c.n == 100 or c.n == 193 for c in wc.CASES)


@pytest.mark.parametrize("c", wc.CASES, ids=wc.IDS)
def test_case_on_the_oracle(oracle, c):
    w = wc.world(c)
    span = c.tiles * wc.TILE
    level = worlds.depths(w.parent)
    chain = wc.chain_of(level)
    waves = -(-w.n // WAVE)
    assert level.max() == c.depth and chain == min(c.depth, wc.MAX_CHAIN)
    assert tpc.closed(w.parent, span) == c.closed
    i = np.arange(w.n)
    kid = np.flatnonzero(w.parent >= 0)
    leaves = kid[w.parent[kid] // WAVE != kid // WAVE]                       # the links that leave their wave-tile
    assert sorted(leaves) == sorted(ch for ch, _ in c.links)
    rebuild_waves = sorted({ch // WAVE for ch, _ in c.links})
    if c.depth:
        inside = kid[w.parent[kid] // WAVE == kid // WAVE]
        lower, higher = (w.parent[inside] < inside).sum(), (w.parent[inside] > inside).sum()
        assert lower > 20 and higher > 20                                    # parents in lower AND in higher lanes
        deep = inside[level[inside] == c.depth]
        assert len(deep) > 10                                                # chains of the full depth, wholly inside a wave-tile
    for v in c.flat:
        assert (w.parent[v * WAVE:(v + 1) * WAVE] < 0).all()
    if c.name == "all-but-one":
        v = rebuild_waves[0]
        lanes = i[v * WAVE:(v + 1) * WAVE]
        assert (w.parent[lanes] >= 0).sum() > 20 and (w.parent[lanes][w.parent[lanes] >= 0] // WAVE != v).sum() == 1
    if c.name.startswith("alternate"):
        assert rebuild_waves == list(range(1, 20, 2))
    if w.n % WAVE:
        assert (w.parent[(waves - 1) * WAVE:] >= 0).any() or w.n % WAVE == 1 or c.depth == 0    # chains in the partial wave-tile, or its one lane
    if c.cycle:
        assert (level < 0).sum() == 3 and (np.flatnonzero(level < 0) // WAVE == wc.CYCLE_AT // WAVE).all()

    side = wc.OracleSide(oracle, c, w)
    s = side.script
    assert len(s.mids) > 0 and (c.depth == 0 or (len(s.seeds) > 0 and len(s.seed_kids) > 0))
    reach = level >= 0
    before_m = None
    for k in range(wc.TICKS):
        side.prepare(k)
        dirty_in = side.ow.dirty()[:w.n].astype(bool)
        side.tick()
        m = side.ow.world_matrices()[:w.n]
        stored = np.tile(IDENT, (w.n, 1)) if k == 0 else before_m.copy()
        if k == 4:
            stored[s.seeds] = s.fake
        want, _, _ = onp.transform_system(side.ow.local_positions()[:w.n], w.rot, w.scale, np.where(reach, w.parent, -1), dirty_in & reach, stored)
        assert np.array_equal(m[reach].view(np.uint32), want[reach].view(np.uint32)), f"tick {k}"

        # which wave-tiles take which form on this tick
        top = wc.tops(w.parent, level, dirty_in, chain)
        coop = wc.cooperative(w.parent, top) if chain >= 1 else np.zeros(waves, bool)
        assert len(coop) == waves
        if k <= 1 or side.produce:                                           # every root dirty: every chain recomputes from its root
            assert np.array_equal(top[reach], level[reach]), f"tick {k}"
            assert sorted(np.flatnonzero(~coop)) == (rebuild_waves if chain >= 1 else list(range(waves))), f"tick {k}"
        if k == 3 and not side.produce:
            assert (top < 0).all() and (coop.all() or chain == 0)            # nothing recomputes: no exchange, nothing stored
        if k == 2 and not side.produce and c.depth >= 2:
            assert (top[s.mids] == 0).all() and (top[np.isin(w.parent, s.mids)] == 1).all()      # the seed is the clean root's rows
        if k == 4 and c.depth and not side.produce:
            assert not dirty_in[s.seeds].any() and (top[s.seed_kids] == 0).all() and np.array_equal(m[s.seeds], s.fake)
            if not c.links:
                # a clean parent with a stale stored matrix in its child's own wave-tile, under the cooperative form: the child reads the
                # rows from memory (top 0), and the grandchildren read the child's lane (top 1)
                assert (s.seeds // WAVE == w.parent[s.seed_kids][0] // WAVE).any() and coop[s.seed_kids // WAVE].all()
                assert c.depth < 2 or (top[np.isin(w.parent, s.seed_kids)] == 1).all()
        if chain >= 1:
            for v in np.flatnonzero(coop):
                SEEN["coop_tops"] |= set(int(x) for x in top[v * WAVE:(v + 1) * WAVE] if x >= 0)
            SEEN["forms"] |= set(bool(x) for x in coop)
            # under the cooperative form a lane's parent recomputes in the same trip with top one less: what the exchange relies on
            for v in np.flatnonzero(coop):
                lanes = i[v * WAVE:(v + 1) * WAVE]
                up = lanes[top[lanes] >= 1]
                assert (top[w.parent[up]] == top[up] - 1).all() and (w.parent[up] // WAVE == v).all(), f"tick {k}"
        if k and not side.produce and k != 3 and (k != 4 or c.depth):
            assert (m.view(np.uint32) != before_m.view(np.uint32)).any()
        side.after()
        d = side.ow.dirty()[:w.n].astype(bool)
        assert d[~reach].all()                                                   # a cycle keeps its bits
        assert np.array_equal(d[reach], (level[reach] == 0) if side.produce else np.zeros(reach.sum(), bool))
        before_m = m
    side.close()


def test_both_forms_and_every_top_occur():
    """(runs behind the cases of this file)"""
    assert SEEN["forms"] == {True, False} and SEEN["coop_tops"] == {0, 1, 2, 3}
