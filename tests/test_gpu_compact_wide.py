"""The end-of-tick kernel's wide form (k_compact_wide: one workgroup takes G consecutive spans, one visibility word per thread, scatter by
word) at the smallest shapes at which it can go wrong, against the oracle and against the SC_TICK_VARIANT=16 twin, which keeps one
workgroup per span.  Which form ran is asserted from compact_stats() after every tick, so that no assertion can pass on the old path.

Cases are in tests/compact_wide_cases.py; tests/test_compact_wide_cpu.py shows with the oracle alone that each has the property its name
claims.  Every case runs TICKS ticks with SC_TICK_PRODUCE_NEXT (the roots move between ticks), with and without SC_TICK_CULLED_LIST; the
span is pinned with SC_TICK_SPANS and G with SC_TICK_COMPACT_G at creation.  The oracle's lists of a case are computed once and shared."""
import functools

import numpy as np
import pytest

from sc_gameengine_amd import capi
from sc_gameengine_amd.tick import WorldTick, camera_view_proj
from tests import compact_wide_cases as cw, worlds

pytestmark = pytest.mark.gpu

BASE = capi.XFORM | capi.CULL | capi.PRODUCE_NEXT
CULLED = [False, True]
CULLED_IDS = ["visible-only", "culled-list"]


def make(monkeypatch, w, spans, force_g=0, narrow=False):
    env = {"SC_TICK_SPANS": str(spans)}
    if force_g:
        env["SC_TICK_COMPACT_G"] = str(force_g)
    if narrow:
        env["SC_TICK_VARIANT"] = "16"
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = WorldTick.from_world(w, broadphase=False)
    for k in env:
        monkeypatch.delenv(k)
    t.set_view_proj(camera_view_proj(w.camera))
    t.set_frame_producer(1, float(cw.DX))
    return t


def stats(t):
    s = t.compact_stats()
    return s["workgroups"], s["spans_per_workgroup"]


@functools.lru_cache(maxsize=None)
def shape_reference(name):
    from oracle import oracle_py
    oracle_py.build()
    c = next(c for c in cw.SHAPES if c.name == name)
    return reference(oracle_py, cw.shape_world(c))


@functools.lru_cache(maxsize=None)
def posed():
    from oracle import oracle_py
    oracle_py.build()
    return cw.poses(oracle_py)


@functools.lru_cache(maxsize=None)
def pattern_reference(name):
    from oracle import oracle_py
    return reference(oracle_py, cw.pattern_world(name, *posed())[0])


def reference(oracle, w):
    ow = worlds.oracle_world(oracle, w, camera=False)
    vp = camera_view_proj(w.camera)
    out = []
    for _ in range(cw.TICKS):
        ow.transform_system(); ow.culling_system(view_proj=vp)
        out.append((ow.visible().copy(), ow.culled().copy(), len(ow.candidates())))
        ow.nudge_roots_x(float(cw.DX))
    ow.close()
    for a in out:
        a[0].setflags(write=False); a[1].setflags(write=False)
    return tuple(out)


def check_lists(t, twin, vis, cul, ncand, culled_list):
    """one tick's lists and counters of both contexts: the oracle's, in order; cul None: the candidates' count is not known either"""
    for c in (t, twin):
        assert np.array_equal(c.visible(), vis)
        k = c.counts()
        assert k.visible == len(vis)
        if ncand is not None:
            assert (k.culled, k.renderables_total) == (ncand - len(vis), ncand)
        if culled_list and cul is not None:
            assert np.array_equal(c.culled(), cul)
    if culled_list:
        assert np.array_equal(t.culled(), twin.culled())
    a, b = t.counts(), twin.counts()
    assert (a.visible, a.culled, a.renderables_total) == (b.visible, b.culled, b.renderables_total)


def run_case(monkeypatch, w, spans, force_g, grid, want, ref, culled_list):
    """want: (workgroups, spans per workgroup) of the context under test; the twin must show (grid, 1)"""
    flags = BASE | (capi.CULLED_LIST if culled_list else 0)
    t, twin = make(monkeypatch, w, spans, force_g), make(monkeypatch, w, spans, force_g, narrow=True)
    assert stats(t) == (0, 0)                                                    # nothing ran yet
    for k in range(cw.TICKS):
        t.run(flags); twin.run(flags)
        assert t.tail_stats()["tail_owned_dirty"] and twin.tail_stats()["tail_owned_dirty"], f"tick {k}"
        assert stats(t) == want and stats(twin) == (grid, 1), f"tick {k}"
        if ref is not None:
            vis, cul, ncand = ref[k]
            check_lists(t, twin, vis, cul, ncand, culled_list)
        else:
            bits = np.asarray(t.visibility_bits()).astype(bool)[:w.n]
            vis = np.flatnonzero(bits)
            assert len(vis) > 0
            check_lists(t, twin, vis, None, None, culled_list)
            if culled_list:
                cul = t.culled().astype(np.int64)
                c = t.counts()
                assert c.culled == len(cul) and c.renderables_total == len(vis) + len(cul)
                assert len(np.intersect1d(vis, cul)) == 0 and np.all(np.diff(cul) > 0)
    t.close(); twin.close()


@pytest.mark.parametrize("culled_list", CULLED, ids=CULLED_IDS)
@pytest.mark.parametrize("c", cw.SHAPES, ids=lambda c: c.name)
def test_shapes(monkeypatch, c, culled_list):
    w = cw.shape_world(c)
    want = (c.workgroups, c.g) if c.g else (c.grid, 1)
    assert c.g == 0 or c.g > 1
    run_case(monkeypatch, w, c.spans, c.force_g, c.grid, want, shape_reference(c.name) if c.oracle else None, culled_list)


@pytest.mark.parametrize("culled_list", CULLED, ids=CULLED_IDS)
@pytest.mark.parametrize("name", cw.PATTERNS)
def test_visibility_patterns(monkeypatch, name, culled_list):
    w, _ = cw.pattern_world(name, *posed())
    run_case(monkeypatch, w, 4096, 64, 3 * 64, (3, 64), pattern_reference(name), culled_list)


@pytest.mark.parametrize("culled_list", CULLED, ids=CULLED_IDS)
@pytest.mark.parametrize("kind", ["open", "deep"])
def test_worlds_that_keep_the_old_form_with_xform(monkeypatch, oracle, kind, culled_list):
    """A parent in another span / a hierarchy deeper than the fused kernel's chain: a tick with SC_TICK_XFORM leaves the dirty clear and the
    producer to the end-of-tick kernel, which keeps one workgroup per span; a tick with SC_TICK_CULL alone takes the wide form."""
    w = cw.open_world() if kind == "open" else cw.deep_world()
    grid = -(-w.n // cw.OPEN_SPAN)
    cl = capi.CULLED_LIST if culled_list else 0
    t, twin = make(monkeypatch, w, cw.OPEN_SPANS, cw.OPEN_G), make(monkeypatch, w, cw.OPEN_SPANS, cw.OPEN_G, narrow=True)
    assert not t.tail_stats()["span_closed"] or kind == "deep"
    ow = worlds.oracle_world(oracle, w, camera=False)
    vp = camera_view_proj(w.camera)
    for k in range(cw.TICKS):
        ow.transform_system(); ow.culling_system(view_proj=vp)
        t.run(BASE | cl); twin.run(BASE | cl)
        assert not t.tail_stats()["tail_owned_dirty"] and stats(t) == (grid, 1) and stats(twin) == (grid, 1), f"tick {k}"
        assert len(ow.visible()) > 0 and len(ow.culled()) > 0
        check_lists(t, twin, ow.visible(), ow.culled(), len(ow.candidates()), culled_list)
        assert np.array_equal(t.world_matrices(), ow.world_matrices()[:w.n])
        ow.nudge_roots_x(float(cw.DX))
    before = ow.visible().copy()
    # culling alone, from another camera (the matrices stay: the lists change for the camera's sake)
    vp2 = camera_view_proj(cw.second_camera(w))
    ow.culling_system(view_proj=vp2)
    assert not np.array_equal(ow.visible(), before) and len(ow.visible()) > 0
    for c in (t, twin):
        c.set_frame_producer(0)                                                  # (a producer that is set runs at the head of every run without PRODUCE_NEXT)
        c.set_view_proj(vp2)
        c.run(capi.CULL | cl)
    assert stats(t) == (-(-grid // cw.OPEN_G), cw.OPEN_G) and cw.OPEN_G > 1 and stats(twin) == (grid, 1)
    check_lists(t, twin, ow.visible(), ow.culled(), len(ow.candidates()), culled_list)
    t.close(); twin.close(); ow.close()


def test_graph_replay_keeps_the_form_it_was_captured_with(monkeypatch):
    """captured ticks: the wide form replays, and the lists stay the twin's"""
    c = next(c for c in cw.SHAPES if c.name == "span256-g5")
    w = cw.shape_world(c)
    ref = shape_reference(c.name)
    t, twin = make(monkeypatch, w, c.spans, c.force_g), make(monkeypatch, w, c.spans, c.force_g, narrow=True)
    t.set_graph_mode(True); twin.set_graph_mode(True)
    for k in range(cw.TICKS):
        t.run(BASE | capi.CULLED_LIST); twin.run(BASE | capi.CULLED_LIST)
        assert stats(t) == (c.workgroups, c.g) and stats(twin) == (c.grid, 1)
        check_lists(t, twin, *ref[k], True)
    t.close(); twin.close()
