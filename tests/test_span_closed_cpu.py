"""The host's span-closed rule (scTickHostSpanClosed: no parent link crosses a boundary between runs of `span` dense indices), which
decides whether the fused kernel may end the tick for its own spans.  No device needed."""
import numpy as np

from sc_gameengine_amd import capi, synth_world as sw


def closed(parent, span):
    p = np.ascontiguousarray(parent, np.int32)
    return bool(capi.load().scTickHostSpanClosed(p.ctypes.data_as(capi.I32P), len(p), span))


def test_rule_on_small_cases():
    assert closed([], 256) and closed([-1, -1, -1], 256)
    assert closed([-1, 0, 1, -1], 256)
    p = np.full(600, -1, np.int32)
    p[255] = 254; p[256] = 257                       # both stay inside their spans of 256
    assert closed(p, 256)
    p[256] = 255                                     # child at the first index of a span, parent at the last of the one before
    assert not closed(p, 256) and closed(p, 512)
    p[256] = -1; p[511] = 512                        # a forward parent across the boundary counts too
    assert not closed(p, 256) and not closed(p, 512) and closed(p, 1024)
    q = np.int32([-1, 7, 9, -5])                     # entries that name no entity of the world are no links
    assert closed(q, 2)
    assert not closed([-1, 0], 0)                    # no span, no claim


def test_synth_world_is_span_closed_at_every_span():
    w = sw.generate(16, 16, 15)
    i = np.arange(w.n)
    kids = w.parent >= 0
    assert (np.abs(w.parent[kids] - i[kids]) == 1).all() and (w.parent[kids] // 16 == i[kids] // 16).all()
    for span in (256, 512, 768, 1024):
        assert closed(w.parent, span)
