"""The oracle side of every case of tests/test_gpu_row_stores.py, without a device: each world has the shape its case is there for
(the seeds' children in the tile behind their parents, in one span; a span of one tile; a span wider than the tail's one round trip;
closed or open under the host's rule), and each tick does on the oracle what its kind promises -- clean lanes beside dirty ones in
a wave, clean rows that stay bit for bit, the stale seed inherited by the children, a draw budget below the visible count.  A GPU
test that passes on a world without its property would prove nothing."""
import numpy as np
import pytest

from oracle import oracle_np as onp
from sc_gameengine_amd import capi
from tests import row_store_cases as rc, worlds

TILE = rc.TILE


def closed(parent, span):
    p = np.ascontiguousarray(parent, np.int32)
    return bool(capi.load().scTickHostSpanClosed(p.ctypes.data_as(capi.I32P), len(p), span))


def test_the_table_covers_what_the_issue_lists():
    by = {c.name: c for c in rc.CASES}
    for name in ("seed-before", "clean-rows-stay"):
        c = by[name]
        assert (c.n, c.tiles, c.depth, c.spans) == (2 * TILE - 37, 2, 1, 1) and not FLAGS(c) & capi.PRODUCE_NEXT
    assert "seed" in by["seed-before"].ticks and {"half", "none"} <= set(by["clean-rows-stay"].ticks)
    one = [c for c in rc.CASES if c.tiles == 1]
    assert sorted(c.n for c in one) == [100, 256, 257] and all(FLAGS(c) & capi.PRODUCE_NEXT and c.closed and c.tail for c in one)
    assert [c.spans for c in one if c.n == 257] == [2]
    assert (by["five-tiles"].n, by["five-tiles"].tiles) == (14 * TILE - 37, 5) and by["five-tiles"].tiles > 3      # (spanTail asks for three tiles at once)
    nocull = [c for c in rc.CASES if FLAGS(c) == capi.XFORM | capi.PRODUCE_NEXT]
    assert sorted(c.depth for c in nocull) == [0, 2] and all(c.closed and c.tail for c in nocull)
    assert not by["tail-off"].tail and by["tail-off"].closed and not by["open-world"].closed and by["open-world"].n == 2011
    assert (by["depth5"].n, by["depth5"].depth) == (1243, 5)
    assert FLAGS(by["draws"]) & capi.DRAWS and by["draws"].max_draws > 0
    assert by["quiet-graph"].graph and FLAGS(by["quiet-graph"]) == capi.FULL | capi.PRODUCE_NEXT


def FLAGS(c):
    return rc.FLAG_SETS[c.flags]


def waves_with_clean_beside_dirty(dirty):
    d = np.zeros(-(-len(dirty) // 64) * 64, bool)
    d[:len(dirty)] = dirty
    d = d.reshape(-1, 64)
    return int((d.any(axis=1) & ~d.all(axis=1)).sum())


@pytest.mark.parametrize("c", rc.CASES, ids=rc.IDS)
def test_case_on_the_oracle(oracle, c):
    w = rc.world(c)
    span = c.tiles * TILE
    level = worlds.depths(w.parent)
    assert w.n == c.n and level.max() == c.depth and level.min() == 0
    assert worlds.compute_span(c.n, c.spans) == min(span, -(-c.n // TILE) * TILE)
    assert closed(w.parent, span) == c.closed
    kid = np.flatnonzero(w.parent >= 0)
    if c.world == "seed-before":
        # every seed's child sits in the tile behind its parent's, in the same span; the parents' wave has other roots in it
        assert np.array_equal(w.parent[rc.SEED_KIDS], rc.SEED_PARENTS)
        assert (rc.SEED_PARENTS // TILE == 0).all() and (rc.SEED_KIDS // TILE == 1).all() and span == 2 * TILE
        assert (level[rc.SEED_PARENTS] == 0).all() and rc.SEED_PARENTS.min() % 64 != 0
        assert ((kid // TILE) == (w.parent[kid] // TILE)).any()                  # (and a family inside one tile)
    if not c.closed:
        assert (kid // span != w.parent[kid] // span).sum() > 10
    if c.depth > 3:
        assert (level > 3).sum() > 10                                            # rows the level kernels rebuild from the fused kernel's

    side = rc.OracleSide(oracle, c, w)
    s = side.script
    roots = level == 0
    before_m = None
    for k in range(rc.TICKS):
        kind = c.ticks[k]
        side.prepare(k)
        dirty_in = side.ow.dirty()[:w.n].astype(bool)
        side.tick()
        m = side.ow.world_matrices()[:w.n]
        if k == 0:
            assert kind == "all" and dirty_in.all()
        else:
            changed = (m.view(np.uint32) != before_m.view(np.uint32)).any(axis=1)
            if side.produce or kind == "roots":
                assert dirty_in[roots].all() and changed[roots].all()
            elif kind == "half":
                assert np.array_equal(np.flatnonzero(dirty_in), s.half) and changed[s.half].all()
                assert waves_with_clean_beside_dirty(dirty_in) == -(-w.n // 64)   # in every wave
                stay = np.ones(w.n, bool)
                stay[s.half] = False
                stay[np.isin(w.parent, s.half)] = False
                assert stay.sum() > 100 and not changed[stay].any()              # clean rows stay, bit for bit
            elif kind == "none":
                assert not dirty_in.any() and not changed.any()
            elif kind == "mids":
                assert np.array_equal(np.flatnonzero(dirty_in), s.mids) and changed[s.mids].all()
            elif kind == "seed":
                assert len(s.seeds) > 0 and len(s.seed_kids) > 0 and not dirty_in[s.seeds].any() and dirty_in[s.seed_kids].all()
                assert np.array_equal(m[s.seeds], s.fake) and changed[s.seed_kids].all()
                # the children carry the stale row: column 0 of the fake matrix is (1.5, 0, 0), no product of the real locals gives that
                if c.world == "seed-before":
                    stored = before_m.copy()
                    stored[s.seeds] = s.fake
                    want, _, _ = onp.transform_system(side.ow.local_positions()[:w.n], w.rot, w.scale, w.parent, dirty_in, stored)
                    assert np.array_equal(m.view(np.uint32), want.view(np.uint32))
                    assert np.array_equal(np.flatnonzero(dirty_in), np.sort(np.concatenate([s.seed_kids, s.others])))
                    assert len(s.others) == 150                   # every root of tile 0 in front of lane 200 (lanes 100..149 are children)
                    assert waves_with_clean_beside_dirty(dirty_in[:TILE]) >= 1   # lanes 192..199 dirty beside the clean seeds
        if FLAGS(c) & capi.CULL:
            vis, cul = side.ow.visible(), side.ow.culled()
            assert len(vis) > 0 and len(cul) > 0
            if FLAGS(c) & capi.DRAWS:
                ent, _, _, _, dropped = side.ow.draw_items(max_draws=c.max_draws)
                assert len(vis) > c.max_draws and len(ent) == c.max_draws and dropped > 0
        side.after()
        d = side.ow.dirty()[:w.n].astype(bool)
        assert np.array_equal(d, roots if side.produce else np.zeros(w.n, bool))
        before_m = m
    side.close()
