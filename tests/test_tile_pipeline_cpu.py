"""The oracle side of every case of tests/test_gpu_tile_pipeline.py, without a device: the worlds have the shape their names promise
(span width, ragged ends, parents in the tile before and behind, closed or open under the host's rule), and each of the five ticks
does what the case is there for -- every level rebuilt, only the middle level, nothing, the stale seed -- on the oracle's side,
checked against the numpy model where that is cheap.  A GPU test that passes on an empty visible list or on matrices that never
change would prove nothing."""
import numpy as np
import pytest

from oracle import oracle_np as onp
from sc_gameengine_amd import capi
from tests import tile_pipeline_cases as tc, worlds

IDENT = np.eye(4, dtype=np.float32).ravel()


def closed(parent, span):
    p = np.ascontiguousarray(parent, np.int32)
    return bool(capi.load().scTickHostSpanClosed(p.ctypes.data_as(capi.I32P), len(p), span))


def test_the_table_covers_what_the_loop_can_get_wrong():
    by = {c.name: c for c in tc.CASES}
    assert [by[f"{t}-tiles"].tiles for t in (1, 2, 3, 4, 5)] == [1, 2, 3, 4, 5]
    for t in (1, 2, 3, 4, 5):
        c = by[f"{t}-tiles"]
        total = -(-c.n // tc.TILE)
        assert c.n == tc.TILE * total - 37 and worlds.compute_span(c.n, c.spans) == t * tc.TILE
        assert t == 1 or total % t == t - 1                                      # the last workgroup is one tile short of the others
    assert by["full-tiles"].n % (by["full-tiles"].tiles * tc.TILE) == 0 and by["n100"].n == 100 and by["n257-one-span"].n == 257
    assert {(c.depth, c.flags) for c in tc.CASES if c.name.startswith("depth") and c.closed} == {(d, f) for d in range(4) for f in ("xform", "xform-cull")}
    assert {c.flags for c in tc.CASES} == set(tc.FLAG_SETS)
    assert any(c.flags == "quiet" and not c.tail for c in tc.CASES) and any(c.flags == "quiet" and c.graph for c in tc.CASES)


@pytest.mark.parametrize("c", tc.CASES, ids=tc.IDS)
def test_case_on_the_oracle(oracle, c):
    w = tc.world(c)
    span = c.tiles * tc.TILE
    level = worlds.depths(w.parent)
    assert level.max() == c.depth
    assert closed(w.parent, span) == c.closed
    own, before, behind, other = tc.parent_tiles(w, span)
    if c.closed:
        assert other == 0 and (c.depth == 0 or own > 0)
        if c.tiles >= 2 and c.depth and c.n > 2 * tc.TILE:
            assert before > 0 and behind > 0                                     # the walk ahead reads tiles the span has written or will write
    else:
        assert other > 10
    if c.cycle:
        assert (level < 0).sum() == 3 and np.flatnonzero(level < 0)[0] // tc.TILE == c.tiles + 1

    side = tc.OracleSide(oracle, c, w)
    s = side.script
    assert len(s.mids) > 0 and (c.depth == 0 or (len(s.seeds) > 0 and len(s.seed_kids) > 0))
    reach = level >= 0
    before_m = None
    for k in range(tc.TICKS):
        side.prepare(k)
        dirty_in = side.ow.dirty()[:w.n].astype(bool)
        side.tick()
        m = side.ow.world_matrices()[:w.n]
        # the numpy model from the same inputs: the positions, the dirty flags and the stored matrices in front of the tick
        stored = np.tile(IDENT, (w.n, 1)) if k == 0 else before_m.copy()
        if k == 4:
            stored[s.seeds] = s.fake
        want, _, _ = onp.transform_system(side.ow.local_positions()[:w.n], w.rot, w.scale, np.where(reach, w.parent, -1), dirty_in & reach, stored)
        assert np.array_equal(m[reach].view(np.uint32), want[reach].view(np.uint32)), f"tick {k}"
        if k == 0:
            if side.flags & capi.CULL:
                assert len(side.ow.visible()) > 0 and len(side.ow.culled()) > 0
        else:
            changed = (m.view(np.uint32) != before_m.view(np.uint32)).any(axis=1)
            assert not changed[~reach].any()
            if k == 1 or side.produce:
                assert all(changed[level == lv].any() for lv in range(c.depth + 1))
            if not side.produce:
                if k == 2:
                    assert changed[s.mids].all() and changed.sum() < reach.sum() and np.array_equal(np.flatnonzero(dirty_in & reach), s.mids)
                    assert c.depth < 2 or not changed[level == 0].any()
                if k == 3:
                    assert not dirty_in[reach].any() and not changed.any()
                if k == 4 and c.depth:
                    assert np.array_equal(m[s.seeds], s.fake) and changed[s.seed_kids].all() and not dirty_in[s.seeds].any()
        side.after()
        d = side.ow.dirty()[:w.n].astype(bool)
        assert d[~reach].all()                                                   # a cycle keeps its bits
        assert np.array_equal(d[reach], (level[reach] == 0) if side.produce else np.zeros(reach.sum(), bool))
        before_m = m
    side.close()
