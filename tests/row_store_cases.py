"""Cases of tests/test_gpu_row_stores.py and their oracle side, shared with tests/test_row_stores_cpu.py (no GPU here).

The fused kernel's instances without binning store their matrix rows with a cache policy of their own (SC_ROW_STORE_POLICY: write-through
stores that do not stay in L2), through an address the kernel forms itself, in flight beside the loads of the next tile and across the
end of the span.  What that could get wrong: a tile that asks for rows of the tile before while that tile's stores are in flight (the
seed); rows of clean lanes beside stored ones; a span of one tile (the stores straight into the tail); a span wider than the tail's one
round trip; the tail without culling; no tail; and whoever reads the rows in the next launch of the same tick, from another cache
(level kernels, the draw-item writer).  A case is a world, a span width, a flag set and five ticks, each tick one of

  all     everything dirty (the upload; only as tick 0)
  roots   every root moved and dirty (the nudge)
  half    every second root moved and dirty: clean lanes beside dirty ones in every wave
  mids    only the middle level of some chains moved and dirty
  none    nothing dirty
  seed    some clean roots' stored matrices replaced by stale ones on both sides, their children moved and dirty, and (the world of
          `seed-before` only) every other root of the seeds' tile moved and dirty

With SC_TICK_PRODUCE_NEXT the device nudges the roots itself behind every tick, so there every tick has the nudge as well."""
import dataclasses

import numpy as np

from sc_gameengine_amd import capi
from sc_gameengine_amd.tick import camera_view_proj
from tests import tile_pipeline_cases as tc, worlds

TILE = worlds.TILE
DX = tc.DX
TICKS = 5
FLAG_SETS = {"xform-cull": capi.XFORM | capi.CULL, "quiet": tc.QUIET, "xform-produce": capi.XFORM | capi.PRODUCE_NEXT,
             "draws": capi.XFORM | capi.CULL | capi.DRAWS}
LADDER = ("all", "roots", "mids", "none", "seed")          # the five ticks of tests/tile_pipeline_cases.py
SEED_N = 2 * TILE - 37
SEED_PARENTS = np.arange(200, TILE)                        # lanes 200..255 of tile 0 ...
SEED_KIDS = SEED_PARENTS + 56                              # ... and their children, the first 56 lanes of tile 1
DRAW_BUDGET = 40


@dataclasses.dataclass(frozen=True)
class Case(tc.Case):
    ticks: tuple = LADDER
    world: str = "ladder"          # "ladder": tile_pipeline_cases.world; "seed-before": seed_before_world
    max_draws: int = 0


CASES = (
    # the seed in the tile before, and clean rows beside stored ones: one span of two tiles, depth 1
    [Case("seed-before", SEED_N, 2, 1, ticks=("all", "roots", "none", "seed", "none"), world="seed-before", seed=70),
     Case("clean-rows-stay", SEED_N, 2, 1, ticks=("all", "half", "none", "half", "none"), world="seed-before", seed=70)]
    # one-tile spans: no loop trip, the stores straight into the tail
    + [Case("one-tile-n100", 100, 1, 2, flags="quiet", seed=71), Case("one-tile-n256", 256, 1, 2, flags="quiet", seed=72),
       Case("one-tile-n257-two-spans", 257, 1, 1, flags="quiet", seed=73)]
    # five tiles per span: the tail's second loop
    + [Case("five-tiles", 14 * TILE - 37, 5, 2, flags="quiet", seed=74)]
    # the tail without culling
    + [Case(f"tail-no-cull-depth{d}", tc._ladder_n(3), 3, d, flags="xform-produce", seed=75 + d) for d in (0, 2)]
    # no tail: switched off, and a world that is not span-closed
    + [Case("tail-off", tc._ladder_n(3), 3, 2, flags="quiet", tail=False, seed=78), Case("open-world", 2011, 3, 2, closed=False, seed=79)]
    # readers in the next launch of the same tick: the level kernels, the draw-item writer
    + [Case("depth5", 1243, 2, 5, closed=False, seed=80), Case("draws", tc._ladder_n(3), 3, 2, flags="draws", max_draws=DRAW_BUDGET, seed=81)]
    # graph replay of the quiet tick
    + [Case("quiet-graph", tc._ladder_n(3), 3, 2, flags="quiet", graph=True, seed=82)]
)
IDS = [c.name for c in CASES]
assert len(set(IDS)) == len(IDS)


def seed_before_world(seed):
    """One span of two tiles, depth 1: the roots in lanes 200..255 of tile 0 have one child each in tile 1, the roots in lanes 0..49
    one each in their own tile (lanes 100..149); everything else is a root without children."""
    w = worlds.random_world(SEED_N, seed=seed, p_child=0.0, spread=60.0)
    own = np.arange(100, 150)
    w.parent[SEED_KIDS] = SEED_PARENTS
    w.parent[own] = own - 100
    w.pos[SEED_KIDS] = w.pos[own] = np.float32([0.3, 0.1, -0.2])
    return w


def world(c):
    if c.world == "seed-before":
        w = seed_before_world(c.seed)
        assert w.n == c.n and worlds.compute_span(c.n, c.spans) == c.tiles * TILE
        return w
    return tc.world(c)


class Script:
    """The five ticks' changes, as index / value arrays both sides apply: the oracle here, the device in the GPU test."""

    def __init__(self, c, w):
        base = tc.Script(w)
        rng = np.random.default_rng([w.n, 0x5702])
        self.level = base.level
        self.mids, self.mid_pos = base.mids, base.mid_pos
        roots = np.flatnonzero(self.level == 0)
        self.half = roots[::2].astype(np.uint32)
        self.half_pos = rng.uniform(-40, 40, (2, len(self.half), 3)).astype(np.float32)     # (a "half" tick may come twice)
        if c.world == "seed-before":
            self.seeds = SEED_PARENTS.astype(np.uint32)
            self.fake = np.tile(np.eye(4, dtype=np.float32).ravel(), (len(self.seeds), 1))
            self.fake[:, 12:15] = rng.uniform(-5, 5, (len(self.seeds), 3)).astype(np.float32)
            self.fake[:, 0] = np.float32(1.5)
            self.seed_kids = SEED_KIDS.astype(np.uint32)
            self.kid_pos = rng.uniform(-1, 1, (len(self.seed_kids), 3)).astype(np.float32)
            self.others = np.setdiff1d(roots[roots < TILE], SEED_PARENTS).astype(np.uint32)    # every other root of tile 0
            self.other_pos = rng.uniform(-40, 40, (len(self.others), 3)).astype(np.float32)
        else:
            self.seeds, self.fake, self.seed_kids, self.kid_pos = base.seeds, base.fake, base.seed_kids, base.kid_pos
            self.others, self.other_pos = np.zeros(0, np.uint32), np.zeros((0, 3), np.float32)

    def moves(self, kind, nth):
        """(entities, positions) uploaded in front of a tick of this kind (the nth of its kind)"""
        if kind == "half":
            return [(self.half, self.half_pos[nth % 2])]
        if kind == "mids":
            return [(self.mids, self.mid_pos)]
        if kind == "seed":
            return [(self.seed_kids, self.kid_pos), (self.others, self.other_pos)]
        return []


class OracleSide:
    """the oracle brought to the frame of tick k before the device runs it"""

    def __init__(self, oracle, c, w):
        self.c, self.w, self.script = c, w, Script(c, w)
        self.ow = worlds.oracle_world(oracle, w, camera=False)
        self.ents = self.ow.dense_entities()
        self.vp = camera_view_proj(w.camera)
        self.flags = FLAG_SETS[c.flags]
        self.produce = bool(self.flags & capi.PRODUCE_NEXT)

    def nth(self, k):
        return self.c.ticks[:k].count(self.c.ticks[k])

    def prepare(self, k):
        """the host's changes in front of tick k (the device side applies the same arrays: test_gpu_row_stores.apply)"""
        s, ow, kind = self.script, self.ow, self.c.ticks[k]
        if kind == "roots" and not self.produce:
            ow.nudge_roots_x(float(DX))
        if kind == "seed":
            for e, m in zip(s.seeds, s.fake):
                tr = ow.get_transform(int(self.ents[e]))
                for q in range(16):
                    tr.worldMatrix[q] = float(m[q])
        for idx, pos in s.moves(kind, self.nth(k)):
            if len(idx):
                ow.set_local_positions(self.ents[idx], pos)

    def tick(self):
        self.ow.transform_system()
        if self.flags & capi.CULL:
            self.ow.culling_system(view_proj=self.vp)

    def after(self):
        """what the device's producer does behind the tick"""
        if self.produce:
            self.ow.nudge_roots_x(float(DX))

    def close(self):
        self.ow.close()
