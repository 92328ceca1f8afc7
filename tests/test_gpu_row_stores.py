"""The matrix-row stores of the fused kernel's instances without binning (xformCullPipelined: write-through stores under
SC_ROW_STORE_POLICY, in flight beside the next tile's loads and across the end of the span) against the oracle, tick by tick, at the
smallest shapes at which that can go wrong.  The cases, their five ticks and the oracle's side are in
tests/row_store_cases.py; tests/test_row_stores_cpu.py shows without a device that every case has what it is there for.

After every tick, against the oracle brought to the same frame: all world matrices IEEE-equal; the visible list equal, in order;
visible, culled and renderables_total; the dirty flags; the local positions, bit for bit; with SC_TICK_DRAWS the draw items under a
budget below the visible count.  The span is pinned with SC_TICK_SPANS at creation; which instance ran -- with the tail or without --
is asserted from scTickGetTailStats."""
import numpy as np
import pytest

from sc_gameengine_amd import capi
from sc_gameengine_amd.tick import WorldTick, camera_view_proj
from tests import row_store_cases as rc

pytestmark = pytest.mark.gpu


def make(monkeypatch, c, w):
    flags = rc.FLAG_SETS[c.flags]
    monkeypatch.setenv("SC_TICK_SPANS", str(c.spans))
    monkeypatch.setenv("SC_TICK_TAIL", "1" if c.tail else "0")
    t = WorldTick.from_world(w, broadphase=bool(flags & capi.BROADPHASE), max_draws=c.max_draws)
    monkeypatch.delenv("SC_TICK_SPANS"); monkeypatch.delenv("SC_TICK_TAIL")
    t.set_view_proj(camera_view_proj(w.camera))
    if flags & capi.PRODUCE_NEXT:
        t.set_frame_producer(1, float(rc.DX))
    if c.max_draws:
        t.set_draw_budget(c.max_draws)
    if c.graph:
        t.set_graph_mode(True)
    return t


def apply(t, side, k):
    """OracleSide.prepare on the device: the same arrays"""
    s, kind = side.script, side.c.ticks[k]
    if kind == "roots" and not side.produce:
        t.nudge_roots_x(float(rc.DX))
    if kind == "seed":
        for e, m in zip(s.seeds, s.fake):
            t.upload_world_matrices(int(e), m[None])
    for idx, pos in s.moves(kind, side.nth(k)):
        for e, p in zip(idx, pos):
            t.upload_positions(int(e), p[None])


@pytest.mark.parametrize("c", rc.CASES, ids=rc.IDS)
def test_five_ticks_against_the_oracle(monkeypatch, oracle, c):
    w = rc.world(c)
    flags = rc.FLAG_SETS[c.flags]
    side = rc.OracleSide(oracle, c, w)
    t = make(monkeypatch, c, w)
    assert t.tail_stats()["span_closed"] == c.closed
    ow = side.ow
    for k in range(rc.TICKS):
        side.prepare(k); apply(t, side, k)
        side.tick()
        t.run(flags)
        assert t.tail_stats()["tail_owned_dirty"] == (c.closed and c.tail), f"tick {k}"
        assert np.array_equal(t.world_matrices(), ow.world_matrices()[:w.n]), f"tick {k}"      # IEEE equality, as test_gpu_parity
        if flags & capi.CULL:
            vis, cul, cand = ow.visible(), ow.culled(), ow.candidates()
            assert np.array_equal(t.visible(), vis), f"tick {k}"
            cnt = t.counts()
            assert (cnt.visible, cnt.culled, cnt.renderables_total) == (len(vis), len(cul), len(cand)), f"tick {k}"
        if flags & capi.DRAWS:
            ent, mesh, mat, model, dropped = ow.draw_items(max_draws=c.max_draws)
            idx, gmesh, gmat, gmodel = t.draws()
            assert np.array_equal(idx, ent) and np.array_equal(gmesh, mesh) and np.array_equal(gmat, mat), f"tick {k}"
            assert np.array_equal(gmodel, model), f"tick {k}"
            cnt = t.counts()
            assert cnt.draws_emitted == len(ent) and cnt.draws_dropped == dropped and dropped > 0, f"tick {k}"
        if flags & capi.BROADPHASE:
            got, total = t.pairs()
            assert total == 0 and len(got) == 0
        side.after()
        assert np.array_equal(t.dirty(), ow.dirty()[:w.n]), f"tick {k}"
        assert np.array_equal(t.positions().view(np.uint32), ow.local_positions()[:w.n].view(np.uint32)), f"tick {k}"
    t.close(); side.close()
