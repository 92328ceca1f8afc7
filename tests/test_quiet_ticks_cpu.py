"""Quiet ticks without a GPU: the ABI surface, and the oracle side of tests/test_gpu_quiet_ticks.py -- what the GPU tests expect must
not be trivially true: the ray ticks have hits (different ones each), the pairable worlds have pairs, the quiet world has none."""
import numpy as np

from sc_gameengine_amd import capi, synth_world as sw
from tests import quiet_ticks_cases as qc


def test_the_world_and_its_spans():
    w = qc.world()
    assert w.n == 2304 and set(np.unique(np.asarray(sw.roots(w)) % 16)) <= set(range(16))
    from tests import worlds
    assert worlds.compute_span(w.n, int(qc.SPANS)) == 768 and worlds.compute_span(w.n + 1, int(qc.SPANS)) == 768      # three tiles; the appended entity opens a fourth span
    assert sorted(set(worlds.depths(w.parent).tolist())) == [0, 1, 2]
    # no two layer words of it admit a pair; under the config3dyn rule they do
    words = {(int(g) & 0xFFFF, int(m) & 0xFFFF) for g, m in zip(w.group, w.mask)}
    assert not any((ga & mb) and (gb & ma) for ga, ma in words for gb, mb in words)
    assert qc.dynamic_rule(w.n).sum() == qc.dynamic_parents(w.n).sum() == qc.S * qc.S and sw.SECTOR_SIZE == qc.SECTOR
    w.group[4], w.mask[4] = sw.GROUP_DYNAMIC, sw.MASK_ALL
    words = {(int(g) & 0xFFFF, int(m) & 0xFFFF) for g, m in zip(w.group, w.mask)}
    assert any((ga & mb) and (gb & ma) for ga, ma in words for gb, mb in words)


def test_bin_stats_symbol_and_free_variant_bit():
    lib = capi.load()
    assert hasattr(lib, "scTickGetBinStats") and "scTickGetBinStats" in capi.SYMBOLS
    assert lib.scTickGetApiVersion() == 7


def test_quiet_world_has_no_pairs_and_the_pairable_ones_do(oracle):
    w = qc.world()
    side = qc.OracleSide(oracle, w)
    side.tick()
    assert len(side.pairs()) == 0 and len(side.visible()) > 0
    w2 = qc.world()
    qc.make_dynamic(w2, qc.dynamic_parents(w2.n))
    side.replace_world(w2)
    side.tick()
    assert len(side.pairs()) >= qc.S * qc.S
    r = int(np.flatnonzero((w.parent < 0) & (w.has_bounds == 1))[37])
    side.replace_world(qc.with_dynamic_entity(qc.world(), side.pos[r]))
    side.tick()
    p = side.pairs()
    assert len(p) >= 1 and (p == w.n).any(axis=1).all()                       # every pair is the appended body's
    side.close()


def test_moved_boxes_expectation_is_not_trivial(oracle):
    w, rays, hits, boxes = qc.moved_boxes_expectation(oracle)
    assert len(rays[0]) == qc.RAYS and len(hits) == 2
    for h in hits:
        assert h["hit"].sum() > qc.RAYS // 2
    assert hits[0].tobytes() != hits[1].tobytes()                            # the boxes moved between the two ray ticks
    # ... and since the learn tick (tick 0) a good share of the boxes has changed sector: 10 nudges of 2.3 m against sectors of 64 m
    first = qc.OracleSide(oracle, qc.world()); first.tick()
    mn0, mx0 = first.boxes(); first.close()
    moved = np.floor(boxes[0][0][:, 0] / qc.SECTOR) != np.floor(mn0[:, 0] / qc.SECTOR)
    assert moved.mean() > 0.25
    # rays cast at the boxes of the learn tick, or the second batch at the boxes of the first, answer differently: stale bins cannot pass
    assert oracle.raycast_boxes(mn0, mx0, w.group, w.mask, *rays).tobytes() != hits[0].tobytes()
    assert oracle.raycast_boxes(*boxes[0], w.group, w.mask, *rays).tobytes() != hits[1].tobytes()
