"""Bind runs of the sorted draw list and the material touch set on the device (SC_TICK_BIND_RUNS; include/sc_tick.h "bind runs") against
the witnesses of tests/bind_runs_ref.py, fed with the oracle's emitted list (ow.draw_items) and its renderer order
(ow.renderer_draw_order): the run table, every ScTickBindInfo field and the bitmap must be equal exactly, and the draw list itself must
not change with the flag.  The worlds are the smallest that reach every path of sc_tick_bindruns.hip: one workgroup (up to 8192
draws) and several, wave and round boundaries inside a workgroup, the LDS bitmap and the per-wave fallback beyond 65536 materials."""
import ctypes as C

import numpy as np
import pytest

from sc_gameengine_amd import capi
from sc_gameengine_amd.tick import WorldTick, camera_view_proj
from tests import bind_runs_ref as R
from tests import worlds

pytestmark = pytest.mark.gpu
SORTED = capi.XFORM | capi.CULL | capi.DRAWS | capi.SORT_DRAWS
FLAGS = SORTED | capi.BIND_RUNS


def oracle_lists(ow, vp, pipeline, mesh_count, max_draws=0, freeze=False):
    """(emitted material handles, sorted materials, sorted meshes) of the oracle's tick"""
    ow.transform_system(); ow.culling_system(view_proj=vp, freeze=freeze)
    ent, mesh, mat, model, dropped = ow.draw_items(max_draws=max_draws)
    order = ow.renderer_draw_order(pipeline, mesh_count)
    return mat, mat[order], mesh[order]


def assert_binds(t, want, draws_without_flag=None):
    wruns, winfo, wtouched = want
    runs, info = t.bind_runs()
    assert info == winfo
    assert runs.dtype == R.RUN_DTYPE and np.array_equal(runs, wruns)
    touched = t.material_touches()
    assert touched.dtype == bool and np.array_equal(touched, wtouched)
    c = t.counts()
    assert info["draws"] == c.draws_sorted
    if draws_without_flag is not None:                         # the flag changes nothing about the list itself
        for a, b in zip(t.draws(), draws_without_flag):
            assert np.array_equal(a, b)
    return runs, info, touched


def check_binds(oracle, w, pipeline, mesh_count, max_draws=0, max_runs=None, graph=False, freeze=False):
    ow = worlds.oracle_world(oracle, w, camera=False)
    t = WorldTick.from_world(w, broadphase=False, max_draws=max_draws)
    vp = camera_view_proj(w.camera)
    t.set_view_proj(vp)
    t.set_freeze_culling(freeze)
    t.set_draw_sort_table(pipeline, mesh_count)
    t.set_bind_runs(w.n if max_runs is None else max_runs)
    t.run(SORTED)
    plain = t.draws()
    emitted, smat, smesh = oracle_lists(ow, vp, pipeline, mesh_count, max_draws, freeze)
    want = R.expected(pipeline, smat, smesh, emitted, w.n if max_runs is None else max_runs)
    if graph:
        t.set_graph_mode(True)
    out = None
    for _ in range(2 if graph else 1):                          # graph mode: the capture, then a replay; the results are equal
        t.run(FLAGS)
        out = assert_binds(t, want, plain)
    t.close(); ow.close()
    return want, out


# ---- the worlds (tests/test_bind_runs_cpu.py checks, without a GPU, that they are what the tests below rely on) ----
SMALL_PIPELINE = np.array([1, 0, 1, 0xFF, 0, 1], np.uint8)     # test_sorted_draws_small_budget's tables: material 3 does not exist ...
SMALL_MESHES, SMALL_BUDGET = 3, 4096                           # ... and mesh 3 is out of range


def small_budget_world(oracle):
    """6000 entities seen by a camera that leaves more than the budget of 4096 visible.  Material 4's draws all carry the invalid mesh 3; a few entities carry handles past the table (6, 9);
    material 5 is taken away from everything and given to the LAST 40 visible entities only, which the budget drops."""
    w = worlds.random_world(6000, seed=51, spread=120.0, p_no_mesh=0.05)
    w.camera["pos"], w.camera["rot"] = np.float32([0.0, 0.0, 200.0]), np.float32([0.0, 0.0, 0.0])      # from outside: about 5000 visible
    ow = worlds.oracle_world(oracle, w, camera=False)
    ow.transform_system()
    vis = ow.culling_system(view_proj=camera_view_proj(w.camera)).copy()
    ow.close()
    w.material[w.material == 5] = 2
    w.mesh[w.material == 4] = 3
    w.material[vis[100:4000:400]] = np.where(np.arange(10) % 2 == 0, 6, 9)
    w.material[vis[-40:]] = 5
    return w, vis


def test_small_budget_touches_and_runs(oracle):
    w, vis = small_budget_world(oracle)
    assert len(vis) > SMALL_BUDGET + 40                          # the last 40 visible entities lie past the budget
    (wruns, winfo, wtouched), _ = check_binds(oracle, w, SMALL_PIPELINE, SMALL_MESHES, max_draws=SMALL_BUDGET)
    assert winfo["draws"] < SMALL_BUDGET and winfo["runs"] >= 8 and not winfo["runs_truncated"]
    assert wtouched.tolist() == [True, True, True, True, True, False]
    # material 4: touched, though none of its draws survives the renderer's mesh check; 3: touched, though it has no Material;
    # 5: only dropped draws carry it; 6 and 9 lie past the table: no bit (and no word) for them
    assert 4 not in wruns["material"] and 3 not in wruns["material"] and winfo["touch_words"] == 1


def test_truncated_table_keeps_the_full_totals(oracle):
    w, _ = small_budget_world(oracle)
    full, _ = check_binds(oracle, w, SMALL_PIPELINE, SMALL_MESHES, max_draws=SMALL_BUDGET)
    (wruns, winfo, _), (runs, info, _) = check_binds(oracle, w, SMALL_PIPELINE, SMALL_MESHES, max_draws=SMALL_BUDGET, max_runs=5)
    assert len(runs) == 5 and np.array_equal(runs, full[0][:5]) and info["runs_truncated"] == 1
    assert info["runs"] == full[1]["runs"] > 5
    for k in ("draws", "pipeline_binds", "material_binds", "mesh_binds", "materials_touched"):
        assert info[k] == full[1][k]
    assert int(runs["first"][-1] + runs["count"][-1]) < info["draws"]     # the last reported row's count comes from the row behind the table


BOUNDARY_STARTS = [0, 63, 128, 192, 500, 530, 1000, 1100, 1299]          # run k = items [start k, start k+1)
BOUNDARY_N = 1300


def boundary_world():
    """Every entity visible (frozen culling, every entity a renderable), keys ascending with the dense index: the sorted list is the
    dense order and its runs are BOUNDARY_STARTS -- 65 items from item 63 (across a wave's round), exactly 64 from 128, 30 across
    item 512 (a wave's 512 items end there), 100 across item 1024, a tail run of one item."""
    w = worlds.random_world(BOUNDARY_N, seed=61, spread=60.0, p_no_mesh=0.0, p_child=0.2)
    run_of = np.searchsorted(BOUNDARY_STARTS, np.arange(BOUNDARY_N), side="right") - 1
    w.material = (run_of // 2).astype(np.uint32)               # keys (pipeline, material, mesh) ascend with the run
    w.mesh = (run_of % 2).astype(np.uint32)
    return w, np.array([0, 0, 0, 1, 1], np.uint8)


def test_runs_across_wave_and_round_boundaries(oracle):
    w, pipeline = boundary_world()
    (wruns, winfo, _), _ = check_binds(oracle, w, pipeline, 2, freeze=True)
    assert winfo["draws"] == BOUNDARY_N
    assert wruns["first"].tolist() == BOUNDARY_STARTS
    assert wruns["count"].tolist() == [63, 65, 64, 308, 30, 470, 100, 199, 1]
    assert wruns["binds"].tolist() == [7, 4, 6, 4, 6, 4, 7, 4, 6]
    assert (winfo["pipeline_binds"], winfo["material_binds"], winfo["mesh_binds"]) == (2, 5, 9)


def test_one_key_all_distinct_keys_and_nothing_survives(oracle):
    w = worlds.random_world(2000, seed=53, spread=80.0)
    one = np.array([0, 1], np.uint8)
    w.mesh[:] = 2; w.material[:] = 1
    (_, winfo, wtouched), _ = check_binds(oracle, w, one, 3)
    assert winfo["runs"] == 1 and winfo["draws"] > 100 and wtouched.tolist() == [False, True]
    w.material = np.arange(w.n, dtype=np.uint32)                # every draw its own material: every draw its own run
    (_, winfo, wtouched), _ = check_binds(oracle, w, (np.arange(w.n) % 3 == 0).astype(np.uint8), 3)
    assert winfo["runs"] == winfo["draws"] > 100 and winfo["materials_touched"] == winfo["draws"] and winfo["touch_words"] == 63
    (wruns, winfo, wtouched), _ = check_binds(oracle, w, np.full(w.n, 0xFF, np.uint8), 3)      # no material exists: nothing is drawn ...
    assert winfo["runs"] == 0 and winfo["draws"] == 0 and len(wruns) == 0
    assert winfo["materials_touched"] > 100                     # ... and every emitted draw's material is touched all the same


def multi_workgroup_world():
    """The 60 000-entity world of test_sorted_draws_multi_workgroup_and_graph (more than 8192 sorted draws, no budget) with fewer
    distinct keys, so that runs are long enough for one to lie across item 8192 (asserted from the witness by the test)."""
    w = worlds.random_world(60000, seed=55, spread=150.0, p_child=0.2)
    rng = np.random.default_rng(4)
    w.mesh = rng.integers(0, 12, w.n).astype(np.uint32)
    w.material = rng.integers(0, 40, w.n).astype(np.uint32)
    pipeline = (np.arange(40) % 2).astype(np.uint8)
    pipeline[::17] = 0xFF
    return w, pipeline, 11


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_multi_workgroup_lists(oracle, graph):
    w, pipeline, meshes = multi_workgroup_world()
    (wruns, winfo, _), _ = check_binds(oracle, w, pipeline, meshes, graph=graph)
    assert winfo["draws"] > 8192 and winfo["runs"] > 300
    first, end = wruns["first"].astype(np.int64), wruns["first"].astype(np.int64) + wruns["count"]
    assert np.any((first < 8192) & (end > 8192))                # a run that starts in one workgroup's items and ends in the next one's


def test_touches_beyond_the_lds_bitmap(oracle):
    """test_sorted_draws_handles_span_several_key_bytes' tables: 65538 material handles are 2049 words, one more than the workgroup's
    LDS bitmap holds -- the per-wave path."""
    w = worlds.random_world(5000, seed=52, spread=100.0)
    rng = np.random.default_rng(3)
    w.mesh = rng.choice([0, 1, 255, 256, 70000, 2**24 - 1], w.n).astype(np.uint32)
    w.material = rng.choice([0, 7, 300, 65536, 65537, 65538, 2**24], w.n).astype(np.uint32)
    pipeline = np.full(65538, 0xFF, np.uint8)
    pipeline[[0, 7, 300, 65536, 65537]] = [1, 0, 127, 0, 1]
    (_, winfo, wtouched), _ = check_binds(oracle, w, pipeline, 2**24)
    assert winfo["touch_words"] == 2049 and np.flatnonzero(wtouched).tolist() == [0, 7, 300, 65536, 65537]


def test_overlapped_readback_next_to_the_frame(oracle):
    w = worlds.random_world(3000, seed=57, spread=100.0)
    w.material = (np.arange(w.n) % 97).astype(np.uint32)
    pipeline = (np.arange(97) % 2).astype(np.uint8)
    ow = worlds.oracle_world(oracle, w, camera=False)
    t = WorldTick.from_world(w, broadphase=False)
    t.set_draw_sort_table(pipeline, 4)
    t.set_bind_runs(512)
    t.set_frame_readback(w.n, w.n)                           # (bind runs first, then the frame read-back; the other order below)
    cams = []
    for k in range(3):
        cam = dict(w.camera); cam["rot"] = w.camera["rot"] + np.float32([0.0, 0.9 * k, 0.0])
        cams.append(camera_view_proj(cam))
    sync = []
    for k, vp in enumerate(cams):
        t.set_view_proj(vp)
        t.run(FLAGS)
        emitted, smat, smesh = oracle_lists(ow, vp, pipeline, 4)
        sync.append(assert_binds(t, R.expected(pipeline, smat, smesh, emitted, 512)))
        if k:                                                   # tick k is queued: take frame k - 1
            tick, runs, info, touched = t.acquire_frame_binds(1)
            assert tick == k - 1 == t.acquire_frame(1)[0].tick
            assert info == sync[k - 1][1] and np.array_equal(runs, sync[k - 1][0]) and np.array_equal(touched, sync[k - 1][2])
    assert len({s[1]["draws"] for s in sync}) == 3 and all(s[1]["runs"] > 50 for s in sync)      # the camera moved: three different lists
    tick, runs, info, touched = t.acquire_frame_binds(0)
    assert tick == 2 == t.acquire_frame(0)[0].tick and info == sync[2][1] and np.array_equal(runs, sync[2][0])
    t.run(SORTED)                                               # a run without the flag stages no binds
    tick, runs, info, touched = t.acquire_frame_binds(0)
    assert tick == 3 and len(runs) == 0 and not any(info.values())
    assert t.acquire_frame_binds(1)[2] == sync[2][1]
    # off and on again, the frame read-back first this time, and a smaller table
    t.set_bind_runs(0)
    with pytest.raises(capi.ScTickError, match="scTickSetBindRuns"):
        t.acquire_frame_binds(0)
    t.set_frame_readback(0, 0)
    t.set_frame_readback(w.n, w.n)
    t.set_bind_runs(16)
    t.run(FLAGS)
    tick, runs, info, touched = t.acquire_frame_binds(0)
    assert tick == 0 and info == dict(sync[2][1], runs_truncated=1) and np.array_equal(runs, sync[2][0][:16]) and np.array_equal(touched, sync[2][2])
    # another material_count resizes the bitmap (and the staging blocks with it)
    wider = np.concatenate((pipeline, np.zeros(1000, np.uint8)))
    t.set_draw_sort_table(wider, 4)
    t.run(FLAGS)
    tick, runs, info, touched = t.acquire_frame_binds(0)
    assert info["touch_words"] == (97 + 1000 + 31) // 32 and len(touched) == 1097 and np.array_equal(touched[:97], sync[2][2]) and not touched[97:].any()
    assert np.array_equal(t.material_touches(), touched)
    t.close(); ow.close()


def test_errors_name_the_missing_call_and_the_next_run_works(oracle):
    w = worlds.random_world(500, seed=58, spread=60.0)
    pipeline = np.array([0, 1, 0, 1, 0, 1], np.uint8)
    t = WorldTick.from_world(w, broadphase=False)
    t.set_camera(w.camera)
    lib, err = t.lib, lambda: t.lib.scTickGetLastError(t.ctx)
    info, fb, cnt = capi.BindInfo(), capi.FrameBinds(), C.c_uint32()
    assert lib.scTickSetBindRuns(t.ctx, 64) == 0 and b"scTickSetDrawSortTable" in err()          # before a sort table
    t.set_draw_sort_table(pipeline, 4)
    assert lib.scTickRun(t.ctx, FLAGS) == 0 and b"scTickSetBindRuns" in err()                    # the flag without scTickSetBindRuns
    t.set_bind_runs(64)
    assert lib.scTickRun(t.ctx, capi.XFORM | capi.CULL | capi.DRAWS | capi.BIND_RUNS) == 0 and b"SC_TICK_SORT_DRAWS" in err()
    assert lib.scTickRun(t.ctx, capi.XFORM | capi.CULL | capi.BIND_RUNS) == 0 and b"SC_TICK_DRAWS" in err()
    t.run(SORTED)
    assert lib.scTickReadBindRuns(t.ctx, None, 0, C.byref(info)) == 0 and b"did not request SC_TICK_BIND_RUNS" in err()
    assert lib.scTickReadMaterialTouches(t.ctx, None, 0, C.byref(cnt)) == 0 and b"did not request SC_TICK_BIND_RUNS" in err()
    t.run(FLAGS)
    assert lib.scTickReadBindRuns(t.ctx, None, 0, None) == 0 and b"null argument" in err()       # NULLs
    assert lib.scTickReadMaterialTouches(t.ctx, None, 0, None) == 0 and b"null argument" in err()
    assert lib.scTickAcquireFrameBinds(t.ctx, 0, None) == 0 and b"null argument" in err()
    assert lib.scTickSetBindRuns(None, 64) == 0 and lib.scTickReadBindRuns(None, None, 0, C.byref(info)) == 0
    assert lib.scTickReadMaterialTouches(None, None, 0, C.byref(cnt)) == 0 and lib.scTickAcquireFrameBinds(None, 0, C.byref(fb)) == 0
    assert lib.scTickAcquireFrameBinds(t.ctx, 0, C.byref(fb)) == 0 and b"scTickSetFrameReadback" in err()      # without the frame read-back
    assert lib.scTickReadBindRuns(t.ctx, None, 0, C.byref(info)) == 1 and info.runs > 0          # runs may be NULL with capacity 0: the report alone
    # ... and the next valid run works: against the witness
    ow = worlds.oracle_world(oracle, w, camera=False)
    vp = camera_view_proj(w.camera)
    emitted, smat, smesh = oracle_lists(ow, vp, pipeline, 4)
    t.run(FLAGS)
    assert_binds(t, R.expected(pipeline, smat, smesh, emitted, 64))
    # an empty context has nothing to launch: an all-zero report, an empty bitmap of the table's size
    t.set_count(0)
    t.run(FLAGS)
    runs, info = t.bind_runs()
    assert len(runs) == 0 and info == dict(runs=0, runs_truncated=0, draws=0, pipeline_binds=0, material_binds=0, mesh_binds=0, materials_touched=0, touch_words=1)
    assert t.material_touches().tolist() == [False] * 6
    t.close(); ow.close()
