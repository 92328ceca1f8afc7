"""worlds.span_closed_world at every (n, span, depth) tests/test_gpu_tail_matrix.py runs: closed under the host's rule
(scTickHostSpanClosed) at its span and open once one link is moved across a boundary, every level present in every span, far links of
both kinds.  No device needed."""
import numpy as np
import pytest

from sc_gameengine_amd import capi
from tests import worlds

CASES = worlds.tail_cases()


def closed(parent, span):
    p = np.ascontiguousarray(parent, np.int32)
    return bool(capi.load().scTickHostSpanClosed(p.ctypes.data_as(capi.I32P), len(p), span))


def test_the_table_gives_the_spans_it_names():
    for tiles, n, spans, depth, seed in worlds.TAIL_LADDER:
        assert worlds.compute_span(n, spans) == tiles * worlds.TILE and n % 32 != 0 and 2 * tiles * worlds.TILE < n
    assert worlds.compute_span(worlds.TAIL_MATRIX_N, worlds.TAIL_MATRIX_SPANS) == worlds.TAIL_MATRIX_TILES * worlds.TILE
    assert [t for t, *_ in worlds.TAIL_LADDER] == [1, 3, 4, 17, 33, 65]
    # the library's rule on shapes whose answer is known: 1 M entities under the default 1536 spans walk three tiles per span
    assert worlds.compute_span(1 << 20, 1536) == 768 and worlds.compute_span(1100, 4096) == 256 and worlds.compute_span(0, 7) == 256


@pytest.mark.parametrize("n,span,depth,seed", CASES)
def test_span_closed_world(n, span, depth, seed):
    w = worlds.span_closed_world(n, span, depth, seed)
    i = np.arange(n)
    kids = w.parent >= 0
    assert w.n == n and n % 32 != 0 and n % span != 0
    assert closed(w.parent, span)
    assert (w.parent[kids] // span == i[kids] // span).all()                     # the rule restated
    if span > worlds.TILE:
        assert not closed(w.parent, span - worlds.TILE) or depth == 0            # (far links reach over the narrower span's boundaries)
    # one link moved across a boundary opens it, from either side
    for child, parent in ((span, span - 1), (span - 1, span), (2 * span, span + 5)):
        p = w.parent.copy()
        p[child] = parent
        assert not closed(p, span)
    # a link between two tiles of one span does not (the boundary probe of the GPU test), and deepens nothing past level 1
    if span > worlds.TILE:
        p = w.parent.copy()
        p[span - worlds.TILE] = span - worlds.TILE - 1
        assert closed(p, span) and worlds.depths(p).max() == max(depth, 1)
    p = w.parent.copy()
    p[span] = span - 1
    assert worlds.depths(p).max() == max(depth, 1)
    # every level in every span (the last one is long enough in every case of the table)
    lv = worlds.depths(w.parent)
    assert lv.min() == 0 and lv.max() == depth
    for b in range(0, n, span):
        hist = np.bincount(lv[b:b + span], minlength=depth + 1)
        assert (hist > 0).all() and len(hist) == depth + 1, (b, hist)
    if depth:
        near = kids & (w.parent == i - 1)
        assert 0.3 < near[kids].mean() < 0.7                                     # about half keep the index before
        assert (w.parent[kids] > i[kids]).sum() > 10                             # forward parents
        if span > worlds.TILE:
            other = w.parent[kids] // worlds.TILE != i[kids] // worlds.TILE
            assert other.sum() > 10 and (other & (w.parent[kids] > i[kids])).any()          # parents in another tile of the span
        assert (w.pos[kids] == np.float32([0.3, 0.1, -0.2])).all()
    assert 0 < (w.has_bounds == 0).sum() < n // 4 and 0 < (w.has_mesh == 0).sum() < n // 4
    # without far links every parent is the index before
    v = worlds.span_closed_world(n, span, depth, seed, far_links=False)
    assert closed(v.parent, span) and (v.parent[v.parent >= 0] == i[v.parent >= 0] - 1).all()
    assert np.array_equal(worlds.depths(v.parent), lv)


def test_add_cycle_keeps_the_world_closed():
    for tiles, n, spans, depth, seed in worlds.TAIL_LADDER[-2:]:
        span = tiles * worlds.TILE
        w = worlds.span_closed_world(n, span, depth, seed)
        trio = worlds.add_cycle(w, 2 * span - 200)
        assert trio[0] - span >= 8192
        assert closed(w.parent, span)
        lv = worlds.depths(w.parent)
        assert np.array_equal(np.flatnonzero(lv < 0), trio) and lv.max() == depth
