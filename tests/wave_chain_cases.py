"""Cases of tests/test_gpu_wave_chains.py and their oracle side, shared with tests/test_wave_chains_cpu.py (no GPU here).

The fused kernel's instances without binning resolve parent chains inside a wave-tile of 64 entities when every chain link of the
wave-tile stays inside it (SC_WAVE_CHAINS, the cooperative form: a lane multiplies once and takes its parent's world matrix from the
parent's lane); a wave-tile with one link that leaves it rebuilds every ancestor in every lane as before.  What that could get
wrong depends on where a child's parent sits -- a lower lane, a HIGHER lane, lane 63 under lane 0 of the next wave-tile, another wave
of the tile, the tile before or behind, another span -- on which lanes of a wave-tile take part (a partial last wave-tile, clean lanes,
members of a cycle, a clean parent whose stored matrix is the seed), and on which instance runs (chain 1, 2, 3; culling; the tail;
the last tile of a span).  A case is a world, a span width and a flag set; every case runs the five ticks of
tests/tile_pipeline_cases.py (all dirty; roots nudged; middle levels only; nothing; stale seeds under dirty children).

Worlds: every wave-tile keeps its lanes 0, 1, 62 and 63 as roots without children, and its other lanes are shuffled into parent
chains inside the wave-tile (a parent is as often in a higher lane as in a lower one).  A case's `links` then hang a reserved lane
under a reserved lane somewhere else: the one link that leaves its wave-tile."""
import dataclasses

import numpy as np

from sc_gameengine_amd import synth_world as sw
from tests import tile_pipeline_cases as tc, worlds

TILE = worlds.TILE
WAVE = 64
TICKS = tc.TICKS
FLAG_SETS = tc.FLAG_SETS
RESERVED = (0, 1, 62, 63)
MAX_CHAIN = 3                      # kMaxChain: the deepest chain the fused kernel resolves itself


def at(wave, lane):
    return WAVE * wave + lane


@dataclasses.dataclass(frozen=True)
class Case(tc.Case):
    links: tuple = ()              # (child, parent) pairs between reserved lanes
    flat: tuple = ()               # wave-tiles left without chains: roots only


N2 = tc._ladder_n(2)               # 1243: spans of 2, 2 and 1 tiles, 20 wave-tiles, the last with 27 lanes

CASES = (
    # chains wholly inside a wave-tile, parents in lower and in higher lanes: one instance per chain depth, culling and tail
    [Case(f"in-wave-depth{d}-{f}-{'tail' if t else 'no-tail'}", N2, 2, d, flags=f, tail=t, seed=100 + 4 * d + 2 * t + (f == "xform"))
     for d in (1, 2, 3) for f in ("xform", "xform-cull") for t in (True, False)]
    + [Case("in-wave-quiet", N2, 2, 2, flags="quiet", seed=120), Case("in-wave-quiet-graph", N2, 2, 2, flags="quiet", graph=True, seed=121)]
    # no exchange: a flat world (the chain-0 instance), and flat wave-tiles in a world with chains (every pass skipped)
    + [Case("depth0", N2, 2, 0, seed=122), Case("flat-waves", N2, 2, 2, flat=(0, 5, 6, 18), seed=123)]
    # the one link that leaves its wave-tile
    + [Case("lane63-under-lane0", N2, 2, 2, links=((at(3, 0), at(2, 63)),), seed=124),
       Case("other-wave", N2, 2, 2, links=((at(3, 1), at(0, 62)),), seed=125),
       Case("tile-before", N2, 2, 2, links=((at(5, 1), at(2, 62)),), seed=126),
       Case("tile-behind", N2, 2, 2, links=((at(1, 1), at(6, 62)),), seed=127),
       Case("other-span", N2, 2, 2, links=((at(9, 1), at(3, 62)),), closed=False, seed=128),
       Case("other-span-xform", N2, 2, 3, flags="xform", links=((at(9, 1), at(3, 62)),), closed=False, seed=129),
       Case("all-but-one", N2, 2, 3, links=((at(2, 1), at(6, 62)),), seed=130)]
    # neighbouring wave-tiles alternate between the two forms
    + [Case("alternate", N2, 2, 2, links=tuple((at(v, 1), at(v - 1, 62)) for v in range(1, 20, 2)), seed=131),
       Case("alternate-quiet", N2, 2, 3, flags="quiet", links=tuple((at(v, 1), at(v - 1, 62)) for v in range(1, 20, 2)), seed=132)]
    # a partial last wave-tile; spans of one tile (only the copy of the stage without a tile to walk ahead of)
    + [Case("n100", 100, 1, 2, seed=133), Case("n257", 257, 2, 2, seed=134), Case("n193-xform", 193, 1, 3, flags="xform", seed=135),
       Case("one-tile-spans", tc._ladder_n(1), 1, 2, seed=136)]
    # a cycle keeps its bits; the stale seed of a clean parent in the child's own wave-tile, without culling (the parent's lane holds nothing)
    + [Case("cycle", N2, 2, 2, cycle=True, seed=137), Case("stale-seed-xform", N2, 2, 2, flags="xform", seed=138)]
)
IDS = [c.name for c in CASES]
assert len(set(IDS)) == len(IDS)
CYCLE_AT = at(9, 20)               # lanes 20..22 of wave-tile 9 (tile 2, the second span)


def world(c):
    w = worlds.random_world(c.n, seed=c.seed, p_child=0.0, spread=max(40.0, 1.8 * c.n ** 0.5))
    rng = np.random.default_rng([c.seed, 0x3A7E])
    for v, base in enumerate(range(0, c.n, WAVE)):
        if v in c.flat or c.depth == 0:
            continue
        lanes = rng.permutation([l for l in range(WAVE) if l not in RESERVED and base + l < c.n])
        k = g = 0
        while k < len(lanes):                              # every second chain is of full depth, the others of any
            size = c.depth + 1 if g % 2 == 0 else int(rng.integers(1, c.depth + 2))
            grp = base + lanes[k:k + size]
            w.parent[grp[1:]] = grp[:-1]
            k += size
            g += 1
    for child, parent in c.links:
        assert child % WAVE in RESERVED and parent % WAVE in RESERVED and w.parent[child] < 0 and w.parent[parent] < 0
        w.parent[child] = parent
    if c.cycle:
        worlds.add_cycle(w, CYCLE_AT)
    w.pos[w.parent >= 0] = np.float32([0.3, 0.1, -0.2])
    if c.flags == "quiet":
        w.group[:], w.mask[:] = sw.GROUP_STATIC, sw.MASK_STATIC          # static bodies meet nothing: the world cannot pair
    assert w.n == c.n and worlds.compute_span(c.n, c.spans) == min(c.tiles * TILE, -(-c.n // TILE) * TILE)
    return w


def tops(parent, level, dirty, chain):
    """The fused kernel's walk restated: per entity, how many levels above it its dirty ancestor nearest the root sits (0: the entity
    itself is the top); -1: no dirty ancestor, deeper than the chain, or unreachable (a cycle) -- the entity does not recompute."""
    parent, level = np.asarray(parent), np.asarray(level)
    top = np.full(len(parent), -1, np.int32)
    j = np.arange(len(parent))
    for lev in range(chain + 1):
        on = (level >= lev) & (level <= chain)
        top = np.where(on & dirty[j], lev, top)
        j = np.where(on & (parent[j] >= 0), parent[j], j)
    return top


def cooperative(parent, top):
    """The eligibility rule restated, per wave-tile: every lane with top >= 1 has its parent in its own wave-tile."""
    i = np.arange(len(parent))
    out = (top >= 1) & (parent // WAVE != i // WAVE)
    pad = np.zeros(-(-len(parent) // WAVE) * WAVE, bool)
    pad[:len(parent)] = out
    return ~pad.reshape(-1, WAVE).any(axis=1)


def chain_of(level):
    return int(min(max(level.max(), 0), MAX_CHAIN))


OracleSide = tc.OracleSide
