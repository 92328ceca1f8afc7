"""Witnesses for the bind runs of the sorted draw list and the material touch set (include/sc_tick.h "bind runs"), over plain arrays:
(pipe, material, mesh) of the sorted list and the material handles of the emitted list.  Two independent ones for the runs --
  walk_runs     VkRenderer::recordCommandBuffer's loop (src/engine/src/sc_vk.cpp:1866-1907) taken literally, with its boundPipeline /
                boundMaterial / boundMesh variables, emitting a run whenever the key changes
  vector_runs   the same table from np.flatnonzero of the key changes and np.diff
and touchMaterial (sc_assets.cpp:441-445) for the touches.  No GPU, no oracle."""
import numpy as np

RUN_FIELDS = ("first", "count", "pipeline", "material", "mesh", "binds")
RUN_DTYPE = np.dtype([(n, np.uint32) for n in RUN_FIELDS])
BIND_PIPELINE, BIND_MATERIAL, BIND_MESH = 1, 2, 4


def walk_runs(pipe, material, mesh):
    """The reference loop, one draw after the other.  Pipeline ids stand for the VkPipelines they map to one to one; a mesh handle
    stands for &m_meshes[handle].  Returns the run table and the bind totals (pipeline, material, mesh)."""
    bound_pipeline, bound_material, bound_mesh = None, None, None      # VK_NULL_HANDLE, kInvalidMaterialHandle, nullptr
    runs, totals, last_key = [], [0, 0, 0], None
    for t, (p, m, g) in enumerate(zip(np.asarray(pipe).tolist(), np.asarray(material).tolist(), np.asarray(mesh).tolist())):
        binds = 0
        if bound_pipeline != p:                     # :1880-1888
            binds |= BIND_PIPELINE
            bound_pipeline, bound_mesh, bound_material = p, None, None
        if bound_material != m:                     # :1890-1895
            binds |= BIND_MATERIAL
            bound_material = m
        if bound_mesh != g:                         # :1901-1907
            binds |= BIND_MESH
            bound_mesh = g
        if (p, m, g) != last_key:
            runs.append([t, 0, p, m, g, binds])
            last_key = (p, m, g)
            for k in range(3):
                totals[k] += (binds >> k) & 1
        else:
            assert binds == 0                       # inside a run the loop binds nothing
        runs[-1][1] += 1
    out = np.zeros(len(runs), RUN_DTYPE)
    for k, name in enumerate(RUN_FIELDS):
        out[name] = [r[k] for r in runs]
    return out, tuple(totals)


def vector_runs(pipe, material, mesh):
    pipe, material, mesh = (np.asarray(a, np.uint32) for a in (pipe, material, mesh))
    n = len(pipe)
    out = np.zeros(0, RUN_DTYPE)
    if n == 0:
        return out, (0, 0, 0)
    dp, dm, dg = (np.concatenate(([True], a[1:] != a[:-1])) for a in (pipe, material, mesh))
    first = np.flatnonzero(dp | dm | dg)
    out = np.zeros(len(first), RUN_DTYPE)
    out["first"] = first
    out["count"] = np.diff(np.concatenate((first, [n])))
    out["pipeline"], out["material"], out["mesh"] = pipe[first], material[first], mesh[first]
    out["binds"] = dp[first] * BIND_PIPELINE + (dp | dm)[first] * BIND_MATERIAL + (dp | dg)[first] * BIND_MESH
    b = out["binds"]
    return out, (int((b & 1).sum()), int(((b >> 1) & 1).sum()), int(((b >> 2) & 1).sum()))


def touches(emitted_material, material_count):
    """bool[material_count]: the handles touchMaterial marks when called with every emitted draw's materialId."""
    m = np.asarray(emitted_material, np.uint32)
    out = np.zeros(material_count, bool)
    out[m[m < material_count]] = True
    return out


def expected(pipeline_of_material, sorted_material, sorted_mesh, emitted_material, max_runs):
    """What scTickReadBindRuns / scTickReadMaterialTouches must return: (the first max_runs runs, the ScTickBindInfo dict, the touches)."""
    table = np.asarray(pipeline_of_material, np.uint8)
    sorted_material = np.asarray(sorted_material, np.uint32)
    pipe = table[sorted_material].astype(np.uint32) if len(sorted_material) else np.zeros(0, np.uint32)
    runs, (pb, mb, gb) = walk_runs(pipe, sorted_material, sorted_mesh)
    vruns, vtot = vector_runs(pipe, sorted_material, sorted_mesh)
    assert np.array_equal(runs, vruns) and vtot == (pb, mb, gb)
    touched = touches(emitted_material, len(table))
    info = dict(runs=len(runs), runs_truncated=int(len(runs) > max_runs), draws=len(sorted_material), pipeline_binds=pb, material_binds=mb,
                mesh_binds=gb, materials_touched=int(touched.sum()), touch_words=(len(table) + 31) // 32)
    return runs[:max_runs], info, touched
