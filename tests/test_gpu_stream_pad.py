"""SC_TICK_STREAM_PAD at creation puts the per-entity streams further apart than the capacity (a measurement knob).  Nothing may depend
on the pitch: contexts with pads 0, 64 and 4160 on one world, through ticks, an in-place remove (the relocation kernel walks the streams
by their pitch) and an append, have to agree byte for byte."""
import numpy as np
import pytest

from sc_gameengine_amd import capi
from sc_gameengine_amd.tick import WorldTick, camera_view_proj
from tests import tile_pipeline_cases as tc, worlds

pytestmark = pytest.mark.gpu


def state(t, flags):
    out = [t.world_matrices().tobytes(), t.dirty().tobytes(), t.positions().tobytes(), t.visible().tobytes()]
    if flags & capi.BROADPHASE:
        got, total = t.pairs()
        out.append((int(total), np.sort(got[:, 0].astype(np.uint64) << np.uint64(32) | got[:, 1].astype(np.uint64)).tobytes()))
    return out


@pytest.mark.parametrize("flags", [capi.XFORM | capi.CULL, capi.FULL | capi.PRODUCE_NEXT], ids=["xform-cull", "full"])
def test_pads_agree_byte_for_byte(monkeypatch, flags):
    w = worlds.span_closed_world(1243, 512, 2, 77)
    ctx = []
    for pad in ("0", "64", "4160"):
        monkeypatch.setenv("SC_TICK_STREAM_PAD", pad)
        t = WorldTick.from_world(w, broadphase=bool(flags & capi.BROADPHASE), capacity=1536)
        monkeypatch.delenv("SC_TICK_STREAM_PAD")
        t.set_view_proj(camera_view_proj(w.camera))
        t.set_frame_producer(1, float(tc.DX))
        ctx.append(t)
    rng = np.random.default_rng(78)
    extra = (rng.uniform(-20, 20, (5, 3)), rng.uniform(-3, 3, (5, 3)), rng.uniform(0.5, 2, (5, 3)))
    for k in range(6):
        got = []
        for t in ctx:
            if k == 2:
                t.remove_entities([3, 700, 41])
            if k == 4:
                t.append_entities(*extra, parent=[-1, 5, t.n, -1, 900])
            t.run(flags)
            got.append(state(t, flags))
        assert got[0] == got[1] == got[2], f"tick {k}"
    for t in ctx:
        t.close()
