"""The classed tail instances of the fused kernel end the tick for a wave-tile inside the tile that walks it: the root nudge's px store
from the lane's own register (or, for a clean root, from a px load that rides with the tile's requests) and the wave-tile's new dirty
words from one ballot -- no spanTail, no second barrier, no root-mask or unreachable words.  What that can get wrong, at the smallest
shapes: where a wave-tile, a tile and a span end (1, 63, 64, 65, 191, 256, 257, 768, 769, 1000 and 2 * 768 + 65 entities: a last
wave-tile with at most 32 and with more than 32 live lanes, whole waves past n, a last tile with no look-ahead), spans of 1, 2, 3 and 4
tiles, closed wave-tiles of chain depth 1, 2 and 3, and roots that are CLEAN on a producing tick beside roots that are dirty.

Ten ticks, so that a px stored in a tile is read by the next tick:

  0, 1   producing; everything dirty, then the nudged roots           (px from the register)
  2      producer off                                                 (every dirty word reads zero afterwards)
  3      producing, nothing dirty                                     (every root's px from the load)
  4      producer off
  5      producing, only some children edited                         (clean roots beside recomputing lanes)
  6      producer off
  7      producing, some roots edited with upload_positions, some children too   (both px paths in one wave)
  8      producing                                                    (what tick 7 stored, read back by the kernel)
  9      producer off

After every tick: which instance ran (topology_class_stats, tail_stats) first; then against the oracle brought to the same frame --
world matrices by IEEE equality, positions and dirty flags by bit pattern, the visible list in order, the counts; then byte for byte
against a context of the same library created under SC_TICK_TOPO_CLASSES=0 and against a graph twin, all three given the same calls.
A world of one entity is flat: no instance is classed there, and the case runs the general tail."""
import dataclasses

import numpy as np
import pytest

from sc_gameengine_amd import capi, synth_world as sw
from sc_gameengine_amd.tick import WorldTick, camera_view_proj
from tests import worlds

pytestmark = pytest.mark.gpu
WAVE, TILE = 64, worlds.TILE
PLAN = ("all", "produce", "off", "produce", "off", "kids", "off", "roots", "produce", "off")
FLAG_SETS = {"xform-cull": capi.XFORM | capi.CULL, "xform": capi.XFORM, "quiet": capi.FULL}


@dataclasses.dataclass(frozen=True)
class Case:
    n: int
    spans: int                     # SC_TICK_SPANS at creation
    depth: int
    flags: str = "xform-cull"
    tail: bool = True              # SC_TICK_TAIL at creation
    dx: float = 0.37               # the producer's parameter
    seed: int = 1

    @property
    def tiles(self):               # tiles per span
        return worlds.compute_span(self.n, self.spans) // TILE

    @property
    def name(self):
        return f"n{self.n}-{self.tiles}tiles-depth{self.depth}-{self.flags}" + ("" if self.tail else "-no-tail") + ("-negative" if self.dx < 0 else "")


def _cases():
    out, k = [], 0
    for n in (1, 63, 64, 65, 191, 256, 257, 768, 769, 1000, 2 * 768 + 65):          # every count in spans of one tile
        out.append(Case(n, -(-n // TILE), 1 + k % 3, seed=300 + k)); k += 1
    for n, spans in ((257, 1), (768, 2), (768, 1), (769, 2), (769, 1), (1000, 2), (1000, 1), (1601, 4), (1601, 3), (1601, 2)):      # wider spans
        out.append(Case(n, spans, 1 + k % 3, seed=300 + k)); k += 1
    # producer and flags: a negative parameter; without culling (the kCull = false instances) at every depth; the tail switched off; the headline's tick
    out += [Case(1000, 2, 2, dx=-0.61, seed=330), Case(1601, 3, 1, flags="xform", seed=331), Case(1000, 2, 2, flags="xform", seed=332),
            Case(769, 1, 3, flags="xform", seed=333), Case(1000, 2, 2, tail=False, seed=334), Case(1601, 3, 3, flags="xform", tail=False, seed=335),
            Case(1000, 2, 2, flags="quiet", seed=336)]
    return out


CASES = _cases()
IDS = [c.name for c in CASES]
assert len(set(IDS)) == len(IDS)
assert {c.tiles for c in CASES} == {1, 2, 3, 4} and {c.depth for c in CASES} == {1, 2, 3}


def closed_world(c):
    """every wave-tile closed: its lanes shuffled into chains of up to depth + 1 entities, every second chain of full depth"""
    n = c.n
    w = worlds.random_world(n, seed=c.seed, p_child=0.0, spread=max(40.0, 1.8 * n ** 0.5))
    rng = np.random.default_rng([c.seed, 0xC1A5])
    for base in range(0, n, WAVE):
        lanes = base + rng.permutation(min(WAVE, n - base))
        k = g = 0
        while k < len(lanes):
            size = c.depth + 1 if g % 2 == 0 else int(rng.integers(1, c.depth + 2))
            grp = lanes[k:k + size]
            w.parent[grp[1:]] = grp[:-1]
            k += size; g += 1
    kids = w.parent >= 0
    w.pos[kids] = rng.uniform(-2, 2, (int(kids.sum()), 3)).astype(np.float32)
    if c.flags == "quiet":
        w.group[:], w.mask[:] = sw.GROUP_STATIC, sw.MASK_STATIC          # static bodies meet nothing: the world cannot pair
    assert worlds.depths(w.parent).max() == (c.depth if n > c.depth else n - 1)
    return w


class Edits:
    """what the host changes in front of ticks 5 and 7: index and position arrays, applied to the oracle and to every context"""

    def __init__(self, w):
        rng = np.random.default_rng([w.n, 0xED17])
        roots, kids = np.flatnonzero(w.parent < 0), np.flatnonzero(w.parent >= 0)
        pick = lambda a, m: np.unique(np.concatenate([a[:1], a[-1:], a[::max(1, len(a) // m)]])).astype(np.uint32) if len(a) else np.zeros(0, np.uint32)   # noqa: E731
        self.kids5, self.roots7, self.kids7 = pick(kids, 12), pick(roots, 10), pick(kids[1:], 6)
        self.pos = {k: rng.uniform(-3, 3, (len(a), 3)).astype(np.float32) for k, a in (("kids5", self.kids5), ("roots7", self.roots7), ("kids7", self.kids7))}
        self.roots = roots

    def at(self, k):
        if PLAN[k] == "kids":
            return [(self.kids5, self.pos["kids5"])]
        if PLAN[k] == "roots":
            return [(self.roots7, self.pos["roots7"]), (self.kids7, self.pos["kids7"])]
        return []


def make(monkeypatch, c, w, classes=True, graph=False):
    monkeypatch.setenv("SC_TICK_SPANS", str(c.spans))
    monkeypatch.setenv("SC_TICK_TAIL", "1" if c.tail else "0")
    monkeypatch.setenv("SC_TICK_TOPO_CLASSES", "1" if classes else "0")
    t = WorldTick.from_world(w, broadphase=bool(FLAG_SETS[c.flags] & capi.BROADPHASE))
    for k in ("SC_TICK_SPANS", "SC_TICK_TAIL", "SC_TICK_TOPO_CLASSES"):
        monkeypatch.delenv(k)
    t.set_view_proj(camera_view_proj(w.camera))
    if graph:
        t.set_graph_mode(True)
    return t


def snapshot(t, flags):
    out = [t.world_matrices().tobytes(), t.dirty().tobytes(), t.positions().tobytes()]
    if flags & capi.CULL:
        cnt = t.counts()
        out += [t.visible().tobytes(), (cnt.visible, cnt.culled, cnt.renderables_total)]
    return out


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_ten_ticks(monkeypatch, oracle, c):
    w = closed_world(c)
    n, base = w.n, FLAG_SETS[c.flags]
    assert worlds.compute_span(n, c.spans) == c.tiles * TILE
    edits = Edits(w)
    ow = worlds.oracle_world(oracle, w, camera=False)
    ents = ow.dense_entities()
    vp = camera_view_proj(w.camera)
    t, twin, plain = make(monkeypatch, c, w), make(monkeypatch, c, w, graph=True), make(monkeypatch, c, w, classes=False)
    ctxs = (t, twin, plain)
    assert t.tail_stats()["span_closed"]
    hier = n > 1                                                          # (one entity: a flat world, never classed)
    producing = None
    for k, what in enumerate(PLAN):
        produce = what != "off"
        if produce != producing:
            for x in ctxs:
                x.set_frame_producer(1 if produce else 0, c.dx)           # (a producer that is set runs at the head of every run without PRODUCE_NEXT)
            producing = produce
        for idx, pos in edits.at(k):
            if len(idx):
                ow.set_local_positions(ents[idx], pos)
            for x in ctxs:
                for e, p in zip(idx, pos):
                    x.upload_positions(int(e), p[None])
        flags = base | (capi.PRODUCE_NEXT if produce else 0)
        ow.transform_system()
        if flags & capi.CULL:
            ow.culling_system(view_proj=vp)
        for x in ctxs:
            x.run(flags)
        # which instance ran
        binned = bool(flags & capi.BROADPHASE) and not t.bin_stats()["quiet_last_tick"]      # (tick 0 of a quiet world learns the bins' slots)
        assert [x.topology_class_stats()["classed_last_tick"] for x in ctxs] == [hier and not binned, hier and not binned, False], f"tick {k}"
        assert [x.tail_stats()["tail_owned_dirty"] for x in ctxs] == [c.tail] * 3, f"tick {k}"
        # against the oracle
        assert np.array_equal(t.world_matrices(), ow.world_matrices()[:n]), f"tick {k}"       # IEEE equality, as test_gpu_parity
        if flags & capi.CULL:
            vis, cul, cand = ow.visible(), ow.culled(), ow.candidates()
            assert np.array_equal(t.visible(), vis), f"tick {k}"
            cnt = t.counts()
            assert (cnt.visible, cnt.culled, cnt.renderables_total) == (len(vis), len(cul), len(cand)), f"tick {k}"
        if produce:
            ow.nudge_roots_x(float(np.float32(c.dx)))
        assert np.array_equal(t.positions().view(np.uint32), ow.local_positions()[:n].view(np.uint32)), f"tick {k}"
        assert np.array_equal(t.dirty(), ow.dirty()[:n]), f"tick {k}"
        assert np.array_equal(t.dirty(), (w.parent < 0).astype(np.uint8) if produce else np.zeros(n, np.uint8)), f"tick {k}"
        # against the unclassed context and the graph twin: byte for byte
        got = snapshot(t, flags)
        assert snapshot(twin, flags) == got, f"tick {k}: graph twin"
        assert snapshot(plain, flags) == got, f"tick {k}: SC_TICK_TOPO_CLASSES=0"
    for x in ctxs:
        x.close()
    ow.close()
