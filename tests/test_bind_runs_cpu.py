"""Bind runs without a GPU: the ABI surface, the worlds of tests/test_gpu_bind_runs.py checked for what its tests rely on, and the two witnesses of tests/bind_runs_ref.py against each other -- the literal walk of
VkRenderer's bind loop (sc_vk.cpp:1866-1907) and the vectorised table -- on random and hand-built sorted key lists."""
import ctypes as C
import os
import re

import numpy as np

from sc_gameengine_amd import capi
from tests import bind_runs_ref as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sc_tick.h")
NEW_SYMBOLS = ("scTickSetBindRuns", "scTickReadBindRuns", "scTickReadMaterialTouches", "scTickAcquireFrameBinds")


def both(keys):
    k = np.array(keys, np.uint32).reshape(-1, 3)
    a, at = R.walk_runs(k[:, 0], k[:, 1], k[:, 2])
    b, bt = R.vector_runs(k[:, 0], k[:, 1], k[:, 2])
    assert np.array_equal(a, b) and at == bt
    assert int(a["count"].sum()) == len(k) and (len(a) == 0 or (a["first"][0] == 0 and np.all(np.diff(a["first"]) == a["count"][:-1])))
    return a, at


def test_bind_run_symbols_are_declared_exported_and_bound():
    text = open(HEADER).read()
    lib = capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, text) and name in capi.SYMBOLS and hasattr(lib, name)
    assert re.search(r"SC_TICK_BIND_RUNS\s*=\s*1u << 13", text)
    assert capi.BIND_RUNS == 1 << 13 and not (capi.FULL & capi.BIND_RUNS)
    assert re.search(r"#define SC_TICK_API_VERSION 7u", text) and lib.scTickGetApiVersion() == 7
    assert C.sizeof(capi.BindRun) == 24 and [n for n, _ in capi.BindRun._fields_] == list(R.RUN_FIELDS)
    assert C.sizeof(capi.BindInfo) == 32
    assert [n for n, _ in capi.BindInfo._fields_] == ["runs", "runs_truncated", "draws", "pipeline_binds", "material_binds", "mesh_binds",
                                                      "materials_touched", "touch_words"]
    assert capi.FrameBinds.info.offset == 8 and capi.FrameBinds.runs_in_buffer.offset == 40 and capi.FrameBinds.runs.offset == 48
    assert R.RUN_DTYPE.itemsize == 24
    # the layouts the older structs keep
    assert C.sizeof(capi.Frame) == 56 and C.sizeof(capi.DrawItem) == 80 and C.sizeof(capi.Counts) == 64
    # NULL context: 0, nothing touched
    info, fb, cnt = capi.BindInfo(), capi.FrameBinds(), C.c_uint32()
    assert lib.scTickSetBindRuns(None, 16) == 0
    assert lib.scTickReadBindRuns(None, None, 0, C.byref(info)) == 0
    assert lib.scTickReadMaterialTouches(None, None, 0, C.byref(cnt)) == 0
    assert lib.scTickAcquireFrameBinds(None, 0, C.byref(fb)) == 0


def test_hand_built_case():
    runs, totals = both([(0, 1, 5), (0, 2, 5), (1, 3, 5), (1, 3, 6)])
    assert runs["binds"].tolist() == [7, 2, 7, 4]             # a new material on the same mesh binds no mesh; a new pipeline binds all three
    assert runs["first"].tolist() == [0, 1, 2, 3] and runs["count"].tolist() == [1, 1, 1, 1] and totals == (2, 3, 3)
    runs, totals = both([(0, 1, 5)] * 3 + [(0, 1, 6)] * 2 + [(0, 2, 6)])
    assert runs["binds"].tolist() == [7, 4, 2] and runs["count"].tolist() == [3, 2, 1] and totals == (1, 2, 2)


def test_empty_single_equal_and_distinct_lists():
    runs, totals = both([])
    assert len(runs) == 0 and totals == (0, 0, 0)
    runs, totals = both([(1, 4, 2)])
    assert runs.tolist() == [(0, 1, 1, 4, 2, 7)] and totals == (1, 1, 1)
    runs, totals = both([(1, 4, 2)] * 1000)
    assert runs.tolist() == [(0, 1000, 1, 4, 2, 7)]
    keys = sorted((p, m, g) for p in range(2) for m in range(2 * p, 2 * p + 7) for g in range(9))       # every key once
    runs, totals = both(keys)
    assert len(runs) == len(keys) and np.all(runs["count"] == 1) and totals == (2, 14, len(keys))


def test_witnesses_agree_on_random_sorted_lists():
    rng = np.random.default_rng(77)
    for trial in range(60):
        n = int(rng.choice([2, 63, 64, 65, 500, 3000]))
        nmat, nmesh = int(rng.choice([1, 3, 40])), int(rng.choice([1, 2, 30]))
        table = rng.integers(0, int(rng.choice([1, 2, 5])), nmat)
        mat = rng.integers(0, nmat, n)
        mesh = rng.integers(0, nmesh, n)
        order = np.lexsort((mesh, mat, table[mat]))
        runs, totals = both(np.stack([table[mat][order], mat[order], mesh[order]], 1))
        keys = np.unique(np.stack([table[mat], mat, mesh], 1), axis=0)
        assert len(runs) == len(keys) and totals[2] <= len(keys)                # a sorted list: one run per distinct key
        assert totals[0] == len(np.unique(table[mat])) and totals[1] == len(np.unique(mat))
    # an UNSORTED list is walked all the same (the loop does not care): the witnesses still agree
    both(rng.integers(0, 3, (2000, 3)))


def test_touches_and_expected():
    t = R.touches(np.array([5, 2, 2, 9, 6, 0xFFFFFFFF], np.uint32), 6)
    assert t.tolist() == [False, False, True, False, False, True]               # 6, 9 and the invalid handle lie past the table
    assert R.touches(np.zeros(0, np.uint32), 0).shape == (0,)
    table = np.array([1, 0, 1, 0xFF], np.uint8)
    runs, info, touched = R.expected(table, sorted_material=[1, 1, 0, 2], sorted_mesh=[0, 1, 1, 1], emitted_material=[3, 0, 1, 1, 2, 7], max_runs=3)
    assert runs.tolist() == [(0, 1, 0, 1, 0, 7), (1, 1, 0, 1, 1, 4), (2, 1, 1, 0, 1, 7)]
    assert info == dict(runs=4, runs_truncated=1, draws=4, pipeline_binds=2, material_binds=3, mesh_binds=3, materials_touched=4, touch_words=1)
    assert touched.tolist() == [True, True, True, True]                         # material 3 has no Material (0xFF) and is touched all the same


def test_gpu_worlds_are_what_their_tests_say(oracle):
    """If a seed drifts, this fails, not the premise of a GPU test."""
    from sc_gameengine_amd.tick import camera_view_proj
    from tests import test_gpu_bind_runs as G
    from tests import worlds

    def witness(w, pipeline, meshes, max_draws=0, freeze=False):
        ow = worlds.oracle_world(oracle, w, camera=False)
        emitted, smat, smesh = G.oracle_lists(ow, camera_view_proj(w.camera), pipeline, meshes, max_draws, freeze)
        ow.close()
        return R.expected(pipeline, smat, smesh, emitted, w.n), emitted

    w, vis = G.small_budget_world(oracle)
    assert len(vis) > G.SMALL_BUDGET + 40
    (runs, info, touched), emitted = witness(w, G.SMALL_PIPELINE, G.SMALL_MESHES, G.SMALL_BUDGET)
    assert len(emitted) == G.SMALL_BUDGET and 5 not in emitted and {3, 4, 6, 9} <= set(emitted.tolist())
    assert np.all(w.mesh[w.material == 4] == 3) and touched[4] and not touched[5] and info["runs"] > 5
    w, pipeline = G.boundary_world()
    (runs, info, _), _ = witness(w, pipeline, 2, freeze=True)
    assert runs["first"].tolist() == G.BOUNDARY_STARTS and info["draws"] == G.BOUNDARY_N
    w, pipeline, meshes = G.multi_workgroup_world()
    (runs, info, _), _ = witness(w, pipeline, meshes)
    first, end = runs["first"].astype(np.int64), runs["first"].astype(np.int64) + runs["count"]
    assert info["draws"] > 8192 and np.any((first < 8192) & (end > 8192))
