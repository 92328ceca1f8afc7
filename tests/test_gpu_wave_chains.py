"""Parent chains resolved inside a wave-tile (SC_WAVE_CHAINS: the cooperative form of the fused kernel's instances without binning,
a lane's parent matrix from the parent's lane) and the rebuild the other wave-tiles fall back to, against the oracle, tick by tick,
at the smallest shapes at which either can go wrong.  The cases and their worlds are in tests/wave_chain_cases.py, the five ticks
and the oracle's side in tests/tile_pipeline_cases.py; tests/test_wave_chains_cpu.py shows without a device which wave-tiles take
which form on which tick.

After every tick, against the oracle brought to the same frame: all world matrices IEEE-equal; the visible list equal, in order;
visible, culled and renderables_total; the dirty flags; the local positions, bit for bit.  The span is pinned with SC_TICK_SPANS at
creation; which instance ran -- with the tail or without -- is asserted from scTickGetTailStats.  The device keeps no count of the
forms: that would cost the kernel instructions."""
import numpy as np
import pytest

from sc_gameengine_amd import capi
from tests import test_gpu_tile_pipeline as tp, wave_chain_cases as wc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", wc.CASES, ids=wc.IDS)
def test_five_ticks_against_the_oracle(monkeypatch, oracle, c):
    w = wc.world(c)
    flags = wc.FLAG_SETS[c.flags]
    side = wc.OracleSide(oracle, c, w)
    t = tp.make(monkeypatch, c, w)
    assert t.tail_stats()["span_closed"] == c.closed
    ow = side.ow
    for k in range(wc.TICKS):
        side.prepare(k); tp.apply(t, side, k)
        side.tick()
        t.run(flags)
        assert t.tail_stats()["tail_owned_dirty"] == (c.closed and c.tail), f"tick {k}"
        if c.flags == "quiet":
            assert t.bin_stats()["quiet_last_tick"] == (k >= 1), f"tick {k}"    # (tick 0 learns the bins' slots)
        assert np.array_equal(t.world_matrices(), ow.world_matrices()[:w.n]), f"tick {k}"      # IEEE equality, as test_gpu_parity
        if flags & capi.CULL:
            vis, cul, cand = ow.visible(), ow.culled(), ow.candidates()
            assert np.array_equal(t.visible(), vis), f"tick {k}"
            cnt = t.counts()
            assert (cnt.visible, cnt.culled, cnt.renderables_total) == (len(vis), len(cul), len(cand)), f"tick {k}"
        if flags & capi.BROADPHASE:
            got, total = t.pairs()
            assert total == 0 and len(got) == 0
        side.after()
        assert np.array_equal(t.dirty(), ow.dirty()[:w.n]), f"tick {k}"
        assert np.array_equal(t.positions().view(np.uint32), ow.local_positions()[:w.n].view(np.uint32)), f"tick {k}"
    t.close(); side.close()
