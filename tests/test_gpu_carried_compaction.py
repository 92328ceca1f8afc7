"""The carried compaction: a tick whose end-of-tick launch would be the wide compaction alone defers it, and the next tick's fused launch
(k_xform_cull_classed_tail_carry) runs it at the head of its grid on the words the tick before left -- or, where the next call cannot carry
it, settle() launches it first.  Whatever happens in between, every read returns what the tick computed.

Worlds: closed wave-tiles of chain depth 1, 2 and 3 (test_gpu_classed_tail's closed_world) with entity counts at the edges of a wave-tile, a
tile and a span, SC_TICK_SPANS pinned, SC_TICK_COMPACT_G of 1, 3 and more than the launch has spans (one carry workgroup), and SynthWorld
v1 at 4x4 and 16x16 sectors.  No frame producer runs: the host moves a few roots and turns the camera in front of every tick, so a
fresh oracle world built from the host's copy of the arrays is the reference of every tick.

Every read compares the visible list, the culled list, the counts and the visibility bits three ways: against the oracle, byte for byte
against a context created under SC_TICK_CARRY=0, and against a graph-mode twin, which must not defer.  carry_stats() says what ran."""
import numpy as np
import pytest

from sc_gameengine_amd import capi, synth_world as sw
from sc_gameengine_amd.tick import WorldTick, camera_view_proj
from tests import worlds
from tests.test_gpu_classed_tail import Case, closed_world
from tests.test_gpu_end_of_tick import FIELDS, mirror_of, remove_in_mirror

pytestmark = pytest.mark.gpu
TILE = worlds.TILE
FLAGS = capi.XFORM | capi.CULL | capi.CULLED_LIST


def make(monkeypatch, w, spans, carry=True, graph=False, force_g=0, broadphase=False, max_draws=0, capacity=None):
    env = {"SC_TICK_SPANS": str(spans), "SC_TICK_CARRY": "1" if carry else "0"}
    if force_g:
        env["SC_TICK_COMPACT_G"] = str(force_g)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = WorldTick.from_world(w, broadphase=broadphase, max_draws=max_draws, capacity=capacity)
    for k in env:
        monkeypatch.delenv(k)
    if graph:
        t.set_graph_mode(True)
    return t


def trio(monkeypatch, w, spans, **kw):
    """the context under test, its SC_TICK_CARRY=0 twin and its graph twin"""
    return make(monkeypatch, w, spans, **kw), make(monkeypatch, w, spans, carry=False, **kw), make(monkeypatch, w, spans, graph=True, **kw)


def camera(w, k):
    """tick k's camera: the world's, turned; "nothing": looks at the sky from above the world; "everything": straight down from high up"""
    cam = dict(w.camera)
    if k == "nothing":
        cam["pos"], cam["rot"] = np.float32([0, 500, 0]), np.float32([1.2, 0, 0])
    elif k == "everything":
        cam["pos"], cam["rot"], cam["farZ"] = np.float32(np.mean(w.pos[w.parent < 0], axis=0) * [1, 0, 1] + [0, 900, 0]), np.float32([-np.pi / 2, 0, 0]), 5000.0
    else:
        cam["rot"] = np.float32(cam["rot"]) + np.float32([0.0, 0.9 * k, 0.0])
    return camera_view_proj(cam)


def move_roots(ctxs, m, k):
    """the host's edit in front of tick k: a few roots get new positions (in the mirror and in every context)"""
    roots = np.flatnonzero(m.parent < 0)
    idx = roots[k % 3::max(1, len(roots) // 5)]
    pos = np.random.default_rng([len(m.parent), k]).uniform(-30, 30, (len(idx), 3)).astype(np.float32)
    m.pos[idx] = pos
    for t in ctxs:
        for e, p in zip(idx, pos):
            t.upload_positions(int(e), p[None])


def expected(oracle, m, vp, culled=True):
    n = len(m.parent)
    ow = worlds.oracle_world(oracle, m, camera=False)
    ow.transform_system(); ow.culling_system(view_proj=vp)
    vis, cul, cand = np.asarray(ow.visible(), np.uint32), np.asarray(ow.culled(), np.uint32), len(ow.candidates())
    ow.close()
    bits = np.zeros(n, np.uint8); bits[vis] = 1
    return {"visible": vis, "culled": cul if culled else None, "counts": (len(vis), len(cul), cand), "bits": bits}


def read(t, culled=True):
    """(reads settle: the order is the one a renderer would use -- list, then counts)"""
    vis = t.visible()
    cul = t.culled() if culled else None
    c = t.counts()
    return {"visible": vis, "culled": cul, "counts": (c.visible, c.culled, c.renderables_total), "bits": t.visibility_bits()}


def same(a, b, where):
    for k in ("visible", "culled", "bits"):
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), f"{where}: {k}"
    assert tuple(a["counts"]) == tuple(b["counts"]), f"{where}: counts"


def check_all(ctxs, want, where, culled=True):
    got = [read(t, culled) for t in ctxs]
    same(got[0], want, f"{where}: oracle")
    same(got[1], got[0], f"{where}: SC_TICK_CARRY=0 twin")
    same(got[2], got[0], f"{where}: graph twin")
    for name, t in zip(("SC_TICK_CARRY=0 twin", "graph twin"), ctxs[1:]):
        assert t.carry_stats() == {"deferred": 0, "carried": 0, "settled": 0}, f"{where}: {name} deferred"
    st = ctxs[0].carry_stats()
    assert st["carried"] + st["settled"] == st["deferred"], f"{where}: a deferred compaction was dropped or is still pending after a read ({st})"


def tick(ctxs, m, k, flags=FLAGS, cam=None):
    vp = camera(m, k if cam is None else cam)
    move_roots(ctxs, m, k)
    for t in ctxs:
        t.set_view_proj(vp)
        t.run(flags)
    return vp


def close(ctxs):
    for t in ctxs:
        t.close()


# (n, SC_TICK_SPANS, depth, SC_TICK_COMPACT_G, ticks): counts at the edges of a wave-tile (65, 191), a tile (256, 257) and a span (768, 769,
# 2 * 768 + 65); spans of 1 to 4 tiles; G of 1, 3, the library's rule (0) and more than the launch has spans (64: one carry workgroup);
# 2, 3 and 7 producing ticks before the read
SHAPES = [(65, 1, 1, 0, 2), (191, 1, 2, 1, 3), (256, 1, 3, 0, 7), (257, 2, 1, 3, 2), (768, 3, 2, 1, 3), (769, 2, 3, 3, 7), (769, 1, 1, 0, 2),
          (1000, 2, 2, 64, 3), (1601, 7, 3, 3, 7), (1601, 3, 1, 1, 2), (1601, 2, 2, 64, 3)]


def shape_world(n, spans, depth, seed):
    return closed_world(Case(n, spans, depth, seed=seed))


@pytest.mark.parametrize("n,spans,depth,g,ticks", SHAPES, ids=[f"n{n}-spans{s}-depth{d}-G{g}-{k}ticks" for n, s, d, g, k in SHAPES])
def test_ticks_without_a_read_between(monkeypatch, oracle, n, spans, depth, g, ticks):
    w = shape_world(n, spans, depth, 500 + n + spans)
    m = mirror_of(w)
    ctxs = trio(monkeypatch, w, spans, force_g=g)
    t = ctxs[0]
    for k in range(ticks):
        vp = tick(ctxs, m, k)
        assert t.topology_class_stats()["classed_last_tick"] and t.tail_stats()["tail_owned_dirty"], f"tick {k}"
        groups = t.compact_stats()
        assert groups["workgroups"] * groups["spans_per_workgroup"] >= -(-n // worlds.compute_span(n, spans)), f"tick {k}"      # the deferred launch's shape
        if g == 64:
            assert groups["workgroups"] == 1
    assert t.carry_stats() == {"deferred": ticks, "carried": ticks - 1, "settled": 0}
    check_all(ctxs, expected(oracle, m, vp), f"{ticks} ticks")
    assert t.carry_stats() == {"deferred": ticks, "carried": ticks - 1, "settled": 1}
    close(ctxs)


@pytest.mark.parametrize("sx,props", [(4, 15), (16, 15)], ids=["synth-4x4", "synth-16x16"])
def test_synth_worlds(monkeypatch, oracle, sx, props):
    w = sw.generate(sx, sx, props, hierarchy=True)
    m = mirror_of(w)
    ctxs = trio(monkeypatch, w, 4)
    t = ctxs[0]
    deferred = 0
    for k in range(3):
        vp = tick(ctxs, m, k)
        deferred += t.topology_class_stats()["classed_last_tick"] and t.tail_stats()["tail_owned_dirty"]
    assert t.carry_stats() == {"deferred": deferred, "carried": max(deferred - 1, 0), "settled": 0}
    assert deferred == 3, "SynthWorld v1 with 16 entities per sector is span-closed and classed: every tick defers"
    check_all(ctxs, expected(oracle, m, vp), "three ticks")
    close(ctxs)


def test_a_read_after_every_tick(monkeypatch, oracle):
    w = shape_world(1000, 2, 2, 610)
    m = mirror_of(w)
    ctxs = trio(monkeypatch, w, 2)
    for k in range(4):
        vp = tick(ctxs, m, k)
        check_all(ctxs, expected(oracle, m, vp), f"tick {k}")
    assert ctxs[0].carry_stats() == {"deferred": 4, "carried": 0, "settled": 4}
    close(ctxs)


@pytest.mark.parametrize("cam", ["nothing", "everything"])
def test_cameras_that_see_nothing_and_everything(monkeypatch, oracle, cam):
    w = shape_world(1601, 3, 2, 620)
    w.has_bounds[:] = 1
    m = mirror_of(w)
    ctxs = trio(monkeypatch, w, 3)
    tick(ctxs, m, 0)
    vp = tick(ctxs, m, 1, cam=cam)
    want = expected(oracle, m, vp)
    assert want["counts"][0] == (0 if cam == "nothing" else want["counts"][2]), "the camera does not see what the case is about"
    tick(ctxs, m, 2, cam=cam)                                      # (the carried role scatters nothing / a full word per lane)
    check_all(ctxs, expected(oracle, m, vp), cam)
    close(ctxs)


def test_the_list_is_the_ticks_own_cameras(monkeypatch, oracle):
    w = shape_world(769, 2, 3, 630)
    m = mirror_of(w)
    ctxs = trio(monkeypatch, w, 2)
    tick(ctxs, m, 0)
    vp = tick(ctxs, m, 1)
    for t in ctxs:
        t.set_view_proj(camera(m, 5))                              # between the deferred tick and the read
    check_all(ctxs, expected(oracle, m, vp), "camera set behind the tick")
    close(ctxs)


def test_culled_list_on_then_off(monkeypatch, oracle):
    w = shape_world(1000, 2, 1, 640)
    m = mirror_of(w)
    ctxs = trio(monkeypatch, w, 2)
    tick(ctxs, m, 0)                                               # SC_TICK_CULLED_LIST on: deferred ...
    tick(ctxs, m, 1, flags=capi.XFORM | capi.CULL)                 # ... carried by a tick without it
    assert ctxs[0].carry_stats() == {"deferred": 2, "carried": 1, "settled": 0}
    vp = tick(ctxs, m, 2)                                          # and the other way round
    check_all(ctxs, expected(oracle, m, vp), "culled list off, then on")
    vp = tick(ctxs, m, 3, flags=capi.XFORM | capi.CULL)
    check_all(ctxs, expected(oracle, m, vp, culled=False), "culled list on, then off", culled=False)
    close(ctxs)


@pytest.mark.parametrize("kind", ["xform-only", "draws", "broadphase", "split"])
def test_a_tick_that_cannot_carry(monkeypatch, oracle, kind):
    """a deferred tick, then a tick of another kind, then the reads: the lists are the last CULLING tick's, the counts too"""
    w = shape_world(1000, 2, 2, 650)
    binned = kind in ("broadphase", "split")
    if binned:
        w.group[:], w.mask[:] = sw.GROUP_STATIC, sw.MASK_STATIC
        w.group[5], w.mask[5] = sw.GROUP_DYNAMIC, sw.MASK_ALL           # one dynamic body: the world can pair, no tick is quiet
    m = mirror_of(w)
    ctxs = trio(monkeypatch, w, 2, broadphase=binned, max_draws=64 if kind == "draws" else 0)
    tick(ctxs, m, 0)
    vp = tick(ctxs, m, 1)
    t = ctxs[0]
    assert t.carry_stats() == {"deferred": 2, "carried": 1, "settled": 0}
    if kind == "xform-only":
        tick(ctxs, m, 2, flags=capi.XFORM)
        want = expected(oracle, m, vp, culled=False)                   # (no culling on that tick: tick 1's list and counts stand; the culled list is refused
                                                                       #  behind a run without SC_TICK_CULLED_LIST, its count is in the counts)
    elif kind == "draws":
        vp = tick(ctxs, m, 2, flags=FLAGS | capi.DRAWS)
        want = expected(oracle, m, vp)
    elif kind == "broadphase":
        vp = tick(ctxs, m, 2, flags=FLAGS | capi.BROADPHASE)
        want = expected(oracle, m, vp)
    else:
        vp = tick(ctxs, m, 2, flags=FLAGS | capi.BROADPHASE | capi.SPLIT_PAIRS)
        for x in ctxs:
            x.run_pairs()
        want = expected(oracle, m, vp)
    st = t.carry_stats()
    assert st["deferred"] == 2 and st["carried"] + st["settled"] == 2, f"the pending compaction was neither carried nor settled: {st}"
    check_all(ctxs, want, kind, culled=kind != "xform-only")
    close(ctxs)


@pytest.mark.parametrize("edit", ["append-roots", "remove", "upload-matrices"])
def test_world_edits_between_deferred_ticks(monkeypatch, oracle, edit):
    w = shape_world(1000, 2, 2, 660)
    m = mirror_of(w)
    ctxs = trio(monkeypatch, w, 2, capacity=1280)
    tick(ctxs, m, 0)
    vp = tick(ctxs, m, 1)
    if edit == "append-roots":
        k = 40
        rng = np.random.default_rng(3)
        extra = dict(pos=rng.uniform(-50, 50, (k, 3)).astype(np.float32), rot=np.zeros((k, 3), np.float32), scale=np.ones((k, 3), np.float32),
                     parent=np.full(k, -1, np.int32), bmin=np.full((k, 3), -0.5, np.float32), bmax=np.full((k, 3), 0.5, np.float32),
                     has_mesh=np.ones(k, np.uint8), has_bounds=np.ones(k, np.uint8), mesh=np.zeros(k, np.uint32), material=np.zeros(k, np.uint32))
        for t in ctxs:
            assert t.append_entities(extra["pos"], extra["rot"], extra["scale"]) == len(m.parent)
    elif edit == "remove":
        leaves = np.setdiff1d(np.arange(len(m.parent)), m.parent[m.parent >= 0])
        gone = leaves[leaves < 800][::9][:30]
        moves = [t.remove_entities(gone) for t in ctxs]
    else:
        rows = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (8, 1))
        for t in ctxs:
            t.upload_world_matrices(100, rows)
    # the edit changes no list that a tick has produced: tick 1's results, read now (the pending compaction keeps its own n and its own words)
    if edit != "remove":
        got = [read(t) for t in ctxs]
        n1 = len(m.parent)
        want = expected(oracle, m, vp)
        assert np.array_equal(got[0]["visible"], want["visible"]) and np.array_equal(got[0]["culled"], want["culled"]) and got[0]["counts"] == want["counts"]
        assert np.array_equal(got[0]["bits"][:n1], want["bits"])
        for g in got[1:]:
            same(g, got[0], f"{edit}: twins, before the next tick")
    if edit == "append-roots":
        for f in FIELDS:
            setattr(m, f, np.concatenate([getattr(m, f), extra[f].astype(getattr(m, f).dtype)]))
    elif edit == "remove":
        src, dst = moves[0]
        assert all(np.array_equal(s, src) and np.array_equal(d, dst) for s, d in moves)
        remove_in_mirror(m, gone, src, dst)
    if edit != "upload-matrices":                                  # (an uploaded matrix of a clean entity stays: a fresh oracle world would recompute it)
        for k in (2, 3, 4):
            vp = tick(ctxs, m, k)
        check_all(ctxs, expected(oracle, m, vp), f"{edit}: three ticks on")
    close(ctxs)


def test_sync_then_visibility_bits(monkeypatch, oracle):
    w = shape_world(1601, 3, 3, 670)
    m = mirror_of(w)
    ctxs = trio(monkeypatch, w, 3)
    for k in range(3):
        vp = tick(ctxs, m, k)
    want = expected(oracle, m, vp)
    for t in ctxs:
        assert np.array_equal(t.visibility_bits(), want["bits"]), "the bits are the last tick's copy, pending compaction or not"
        t.sync()
        assert np.array_equal(t.visibility_bits(), want["bits"])
    assert ctxs[0].carry_stats() == {"deferred": 3, "carried": 2, "settled": 1}
    check_all(ctxs, want, "after sync")
    close(ctxs)


def test_profiling_every_kernel_keeps_its_samples(monkeypatch, oracle):
    """a static world with bins: quiet ticks, whose end-of-tick launch is sampled in the K_PAIRS slot -- one sample per sampled tick, and a
    sampled tick does not defer; with only the fused kernel timed, every tick defers and its samples include the carried role"""
    w = shape_world(1000, 2, 2, 680)
    w.group[:], w.mask[:] = sw.GROUP_STATIC, sw.MASK_STATIC
    m = mirror_of(w)
    ctxs = trio(monkeypatch, w, 2, broadphase=True)
    full = FLAGS | capi.BROADPHASE
    vp = tick(ctxs, m, 0, flags=full)                              # the learn tick: binned, cannot defer
    check_all(ctxs, expected(oracle, m, vp), "learn tick")
    t = ctxs[0]
    assert t.carry_stats()["deferred"] == 0
    for x in ctxs[:2]:
        x.set_profiling(1)
    for k in (1, 2, 3):
        vp = tick(ctxs, m, k, flags=full)
        assert t.bin_stats()["quiet_last_tick"]
    assert [len(x.kernel_times_ms(capi.K_PAIRS)) for x in ctxs[:2]] == [3, 3]
    assert t.carry_stats()["deferred"] == 0
    for x in ctxs[:2]:
        x.set_profiling_kernels([capi.K_XFORM_CULL])
        x.set_profiling(1)                                         # (drops the samples so far)
    for k in (4, 5, 6):
        vp = tick(ctxs, m, k, flags=full)
    assert [len(x.kernel_times_ms(capi.K_XFORM_CULL)) for x in ctxs[:2]] == [3, 3] and len(t.kernel_times_ms(capi.K_PAIRS)) == 0
    assert t.carry_stats() == {"deferred": 3, "carried": 2, "settled": 0}
    for x in ctxs[:2]:
        x.set_profiling(0)
    check_all(ctxs, expected(oracle, m, vp), "profiled ticks")
    close(ctxs)
