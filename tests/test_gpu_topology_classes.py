"""The classed instance of the fused kernel (topology classes: a wave-tile's parents, depths and flags from a pattern table and the
tile's 64 dirty bits instead of a link word per entity and per ancestor) against the oracle, tick by tick, at the smallest shapes at
which it can go wrong: one wave-tile, one entity in the second, one tile, spans of two tiles; chains of depth 0..3 inside the wave-
tiles with parents in lower and in higher lanes; one pattern and one per wave-tile.

Seven ticks: the five of tests/tile_pipeline_cases.py (everything dirty; the roots; middle levels only; nothing; children dirty under
clean parents whose stored matrices were replaced: the seed rows), then leaves only, then some roots with children only.  After
every tick, against the oracle brought to the same frame: all world matrices IEEE-equal, the visible list equal in order, the
counts, the dirty flags, the local positions.  Which instance ran is asserted from scTickGetTopologyClassStats on every tick.

Then the switch (SC_TICK_TOPO_CLASSES=0 against 1 on one world, byte-equal), and the transitions on one context: what drops the
classes (appended roots, an in-place remove), what re-derives them open (a parent across wave-tiles) or changed (a rotation that
becomes trivial), closure restored, and a replayed graph across a change of eligibility."""
import dataclasses

import numpy as np
import pytest

from sc_gameengine_amd import capi, synth_world as sw
from sc_gameengine_amd.tick import WorldTick, camera_view_proj
from tests import test_gpu_tile_pipeline as tp, tile_pipeline_cases as tc, worlds

pytestmark = pytest.mark.gpu
WAVE = 64


@dataclasses.dataclass(frozen=True)
class Case(tc.Case):
    one_pattern: bool = False


CASES = (
    # entity counts: one wave-tile; one entity in the second; one tile, its last wave-tile past the end; two spans of two tiles
    [Case(f"n{n}", n, 2 if n > 256 else 1, 2, seed=200 + n % 7) for n in (64, 65, 192, 1024)]
    # one chain instance per depth (depth 0: a flat world has no walk to save -- never the classed instance)
    + [Case(f"depth{d}", 1024, 2, d, seed=210 + d) for d in (0, 1, 3)]
    # one pattern for the whole world, with a clipped last wave-tile (a second pattern) and without
    + [Case("one-pattern", 1024, 2, 2, one_pattern=True, seed=220), Case("one-pattern-n200-xform", 200, 1, 3, flags="xform", one_pattern=True, seed=221)]
    # without culling; without the tail; the headline's tick (quiet, the producer in the tail) eagerly and replayed
    + [Case("xform", 1024, 2, 2, flags="xform", seed=222), Case("no-tail", 1024, 2, 2, tail=False, seed=223),
       Case("quiet", 1024, 2, 2, flags="quiet", seed=224), Case("quiet-graph", 1024, 2, 2, flags="quiet", graph=True, seed=225),
       Case("quiet-no-tail", 1000, 2, 3, flags="quiet", tail=False, seed=226)]
)
IDS = [c.name for c in CASES]


def lane_parents(rng, depth, live=WAVE):
    """parent lane per lane of one wave-tile (-1: root): lanes shuffled into chains of up to depth + 1, every second one of full depth"""
    rel = np.full(WAVE, -1, np.int32)
    lanes = rng.permutation(live)
    k = g = 0
    while depth and k < len(lanes):
        size = depth + 1 if g % 2 == 0 else int(rng.integers(1, depth + 2))
        grp = lanes[k:k + size]
        rel[grp[1:]] = grp[:-1]
        k += size; g += 1
    return rel


def world(c):
    w = worlds.random_world(c.n, seed=c.seed, p_child=0.0, spread=max(40.0, 1.8 * c.n ** 0.5))
    rng = np.random.default_rng([c.seed, 0x70B0])
    shared = lane_parents(rng, c.depth)
    for base in range(0, c.n, WAVE):
        live = min(WAVE, c.n - base)
        rel = shared.copy() if c.one_pattern else lane_parents(rng, c.depth, live)
        rel[live:] = -1
        rel[:live][rel[:live] >= live] = -1                  # (a shared pattern clipped by the end of the world: the parent is gone)
        w.parent[base:base + live] = np.where(rel[:live] < 0, -1, base + rel[:live])
    if c.one_pattern:
        w.has_mesh[:] = 1; w.has_bounds[:] = 1
    w.pos[w.parent >= 0] = np.float32([0.3, 0.1, -0.2])
    if c.flags == "quiet":
        w.group[:], w.mask[:] = sw.GROUP_STATIC, sw.MASK_STATIC
    assert worlds.depths(w.parent).max() == c.depth
    return w


class Extra:
    """ticks 5 and 6: leaves only, then roots with children only"""

    def __init__(self, w):
        level = worlds.depths(w.parent)
        has_kids = np.zeros(w.n, bool)
        has_kids[w.parent[w.parent >= 0]] = True
        rng = np.random.default_rng([w.n, 0x1EAF])
        self.leaves = np.flatnonzero((level >= 1) & ~has_kids)[::4].astype(np.uint32)
        self.roots = np.flatnonzero((level == 0) & has_kids)[::3].astype(np.uint32)
        self.leaf_pos = rng.uniform(-2, 2, (len(self.leaves), 3)).astype(np.float32)
        self.root_pos = rng.uniform(-30, 30, (len(self.roots), 3)).astype(np.float32)

    def at(self, k):
        return (self.leaves, self.leaf_pos) if k == 5 else (self.roots, self.root_pos) if k == 6 else (np.zeros(0, np.uint32), np.zeros((0, 3), np.float32))


def check(t, ow, w, flags, where):
    assert np.array_equal(t.world_matrices(), ow.world_matrices()[:w.n]), where              # IEEE equality, as test_gpu_parity
    if flags & capi.CULL:
        vis, cul, cand = ow.visible(), ow.culled(), ow.candidates()
        assert np.array_equal(t.visible(), vis), where
        cnt = t.counts()
        assert (cnt.visible, cnt.culled, cnt.renderables_total) == (len(vis), len(cul), len(cand)), where


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_seven_ticks_against_the_oracle(monkeypatch, oracle, c):
    w = world(c)
    flags = tc.FLAG_SETS[c.flags]
    side = tc.OracleSide(oracle, c, w)
    extra = Extra(w)
    t = tp.make(monkeypatch, c, w)
    st = t.topology_class_stats()
    tiles = -(-c.n // WAVE)
    assert (st["tiles_classed"], st["tiles_unclassed"]) == (tiles, 0)
    if c.one_pattern:
        assert st["patterns"] == (1 if c.n % WAVE == 0 else 2)
    elif c.depth:
        assert st["patterns"] > 1 or tiles == 1
    ow = side.ow
    for k in range(tc.TICKS + 2):
        side.prepare(k); tp.apply(t, side, k)
        idx, pos = extra.at(k)
        if len(idx):
            ow.set_local_positions(side.ents[idx], pos)
            for e, p in zip(idx, pos):
                t.upload_positions(int(e), p[None])
        side.tick()
        t.run(flags)
        binned = bool(flags & capi.BROADPHASE) and not t.bin_stats()["quiet_last_tick"]      # (tick 0 of a quiet world learns the bins' slots)
        assert t.topology_class_stats()["classed_last_tick"] == (c.depth >= 1 and not binned), f"tick {k}"
        assert t.tail_stats()["tail_owned_dirty"] == c.tail, f"tick {k}"
        check(t, ow, w, flags, f"tick {k}")
        side.after()
        assert np.array_equal(t.dirty(), ow.dirty()[:w.n]), f"tick {k}"
        assert np.array_equal(t.positions().view(np.uint32), ow.local_positions()[:w.n].view(np.uint32)), f"tick {k}"
    t.close(); side.close()


@pytest.mark.parametrize("flags", ["xform-cull", "quiet"])
def test_switch_is_byte_equal(monkeypatch, flags):
    c = Case("switch", 1024, 2, 3, flags=flags, seed=230)
    w = world(c)
    f = tc.FLAG_SETS[flags]
    script, extra = tc.Script(w), Extra(w)
    ctx = []
    for on in ("1", "0"):
        monkeypatch.setenv("SC_TICK_TOPO_CLASSES", on)
        ctx.append(tp.make(monkeypatch, c, w))
        monkeypatch.delenv("SC_TICK_TOPO_CLASSES")
    for k in (0, 1, 2, 3, 5, 6):
        got = []
        for t in ctx:
            if k == 1 and not f & capi.PRODUCE_NEXT:
                t.nudge_roots_x(float(tc.DX))
            idx, pos = (script.mids, script.mid_pos) if k == 2 else extra.at(k)
            for e, p in zip(idx, pos):
                t.upload_positions(int(e), p[None])
            t.run(f)
            got.append((t.world_matrices().tobytes(), t.visible().tobytes(), t.dirty().tobytes(), t.positions().tobytes(), (t.counts().visible, t.counts().culled, t.counts().renderables_total)))
        quiet = all(t.bin_stats()["quiet_last_tick"] for t in ctx) if f & capi.BROADPHASE else True
        assert [t.topology_class_stats()["classed_last_tick"] for t in ctx] == [quiet, False], f"tick {k}"
        assert got[0] == got[1], f"tick {k}"
    for t in ctx:
        t.close()


class Mirror:
    """The arrays of a context that is edited, and a fresh oracle world of them: everything is marked dirty on the device, so one tick
    of both has to give the same matrices and the same visible list whatever the context went through."""

    def __init__(self, w):
        self.w = dataclasses.replace(w, **{f.name: getattr(w, f.name).copy() for f in dataclasses.fields(w)
                                           if isinstance(getattr(w, f.name), np.ndarray) and len(getattr(w, f.name)) == w.n})
        self.w.camera = w.camera
        self.vp = camera_view_proj(w.camera)

    def arrays(self):
        return [f.name for f in dataclasses.fields(self.w) if isinstance(getattr(self.w, f.name), np.ndarray) and len(getattr(self.w, f.name)) == self.n]

    @property
    def n(self):
        return len(self.w.parent)

    def append(self, k, parent, rng):
        n, w = self.n, self.w
        new = {"pos": rng.uniform(-20, 20, (k, 3)), "rot": rng.uniform(-3, 3, (k, 3)), "scale": rng.uniform(0.5, 2, (k, 3)),
               "bmin": np.full((k, 3), -0.5), "bmax": np.full((k, 3), 0.5), "parent": np.asarray(parent), "has_mesh": np.ones(k), "has_bounds": np.ones(k),
               "mesh": np.zeros(k), "material": np.zeros(k), "group": np.full(k, 0xFFFFFFFF), "mask": np.full(k, 0xFFFFFFFF), "sector_of": np.zeros((k, 2))}
        for name in self.arrays():
            a = getattr(w, name)
            setattr(w, name, np.concatenate([a, new[name].astype(a.dtype)]))
        return {name: getattr(w, name)[n:] for name in new}

    def remove(self, src, dst, count):
        """a swap-remove as the library reports it: entity src[i] now sits at dst[i], the last `count` indices are gone"""
        w, n1 = self.w, self.n - count
        rename = {int(s): int(d) for s, d in zip(src, dst)}
        for name in self.arrays():
            a = getattr(w, name)
            a[dst] = a[src]
            setattr(w, name, a[:n1].copy())
        w.parent[:] = [rename.get(int(q), int(q)) for q in w.parent]
        assert (w.parent < n1).all()

    def check(self, oracle, t, flags, where):
        w = self.w
        ow = oracle.OracleWorld.from_arrays(w.pos, w.rot, w.scale, w.parent, w.bmin, w.bmax, has_mesh=w.has_mesh, has_bounds=w.has_bounds,
                                            mesh_id=w.mesh, material_id=w.material)
        ow.transform_system()
        ow.culling_system(view_proj=self.vp)
        t.mark_dirty(0, self.n)
        t.run(flags)
        check(t, ow, w, flags, where)
        ow.close()


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_transitions_on_one_context(monkeypatch, oracle, graph):
    c = Case("transitions", 448, 1, 2, seed=240, one_pattern=True)           # seven wave-tiles, two tiles, one pattern
    w = world(c)
    w.rot[:] = np.float32([0.3, -0.2, 0.1])                                  # (no axis trivial anywhere)
    flags = capi.XFORM | capi.CULL
    rng = np.random.default_rng(241)
    monkeypatch.setenv("SC_TICK_SPANS", "1")
    t = WorldTick.from_world(w, broadphase=False, capacity=1024)
    monkeypatch.delenv("SC_TICK_SPANS")
    t.set_view_proj(camera_view_proj(w.camera))
    if graph:
        t.set_graph_mode(True)
    m = Mirror(w)
    classed = lambda: t.topology_class_stats()["classed_last_tick"]
    stats = lambda: tuple(t.topology_class_stats()[k] for k in ("patterns", "tiles_classed", "tiles_unclassed"))

    for k in range(3):                                                       # (replayed twice in graph mode)
        m.check(oracle, t, flags, f"start {k}")
        assert classed() and stats() == (1, 7, 0)
    # appended roots: link words written without a re-link -- the classes are behind, the general instance runs
    a = m.append(3, [-1, -1, -1], rng)
    t.append_entities(a["pos"], a["rot"], a["scale"], a["bmin"], a["bmax"], a["mesh"], a["material"], a["group"], a["mask"])
    for k in range(2):
        m.check(oracle, t, flags, f"roots appended {k}")
        assert not classed()
    # an append with parents re-links: the new entities hang under wave-tile 0 from wave-tile 7 -- derived, and not closed
    a = m.append(2, [5, m.n - 1], rng)
    t.append_entities(a["pos"], a["rot"], a["scale"], a["bmin"], a["bmax"], a["mesh"], a["material"], a["group"], a["mask"], parent=a["parent"])
    m.check(oracle, t, flags, "child appended across wave-tiles")
    assert not classed() and stats()[1:] == (7, 1)
    # closure restored by a topology upload: classed again, the clipped last wave-tile a pattern of its own
    m.w.parent[-2] = m.n - 5; m.w.parent[-1] = -1
    t.set_topology(m.w.parent)
    for k in range(2):
        m.check(oracle, t, flags, f"closure restored {k}")
        assert classed() and stats() == (2, 8, 0)
    # a rotation that becomes trivial about one axis flips a bit of a link word: re-derived, a third pattern, still classed
    m.w.rot[70, 1] = 0.0
    t.upload_locals(70, m.w.pos[70:71], m.w.rot[70:71], m.w.scale[70:71])
    m.check(oracle, t, flags, "trivial rotation")
    assert classed() and stats() == (3, 8, 0)
    # an in-place remove (a childless root; the last entity, another childless root, takes its place): relocated on the device
    # without a re-link -- the general instance until the next one
    victim = int(np.flatnonzero((m.w.parent < 0) & ~np.isin(np.arange(m.n), m.w.parent))[3])
    src, dst = t.remove_entities([victim])
    m.remove(src, dst, 1)
    for k in range(2):
        m.check(oracle, t, flags, f"removed {k}")
        assert not classed()
    # set a parent across wave-tiles, then take it back: open, then closed and classed
    keep = int(m.w.parent[130])
    m.w.parent[130] = 3
    t.set_topology(m.w.parent)
    m.check(oracle, t, flags, "parent set across wave-tiles")
    assert not classed() and stats()[2] == 1
    m.w.parent[130] = keep
    t.set_topology(m.w.parent)
    for k in range(2):
        m.check(oracle, t, flags, f"closed again {k}")
        assert classed() and stats()[2] == 0
    t.close()
