"""The entity-anchored capsule sweeps without a GPU: the ABI surface, the witness's identities (tests/anchored_sweeps_ref.py against the
plain sweeps' witnesses), closed-form cases worked out by hand, the fp32 resolve against float64, and that every row of
tests/anchored_sweep_cases.py is what it claims -- so that the GPU suite (tests/test_gpu_anchored_sweeps.py) tests what it says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sc_gameengine_amd import capi
from sc_gameengine_amd.tick import SWEEP_HIT_DTYPE, WorldTick
from tests import anchored_sweep_cases as ac, anchored_sweeps_ref as ar, ray_walk_cases as rc, sweep_ref, sweep_shapes_cases as sc, sweep_shapes_ref as ss
from tests.shape_rays_ref import shape_records

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sc_tick.h")
F = np.float32
U = np.uint32
NAMES = ("scTickSetAnchoredSweeps", "scTickReadAnchoredSweepHits", "scTickReadAnchoredSweepSegments", "scTickReadAnchoredSweeps",
         "scTickGetAnchoredSweepShapeInfo")
MODES = (ar.AABB, ar.EXACT)


# ---- the ABI surface ----------------------------------------------------------------------------------------------------------------
def test_anchored_sweep_symbols_are_declared_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"#define\s+SC_TICK_API_VERSION\s+7u", text)
    flags = {n: eval(v.replace("u", "")) for n, v in re.findall(r"^\s*(SC_TICK_[A-Z_]+)\s*=\s*((?:0x[0-9a-fA-F]+|1)u(?: << \d+)?),", text, re.M)}
    assert flags["SC_TICK_ANCHORED_SWEEPS"] == 1 << 18 == 0x00040000 == capi.ANCHORED_SWEEPS and len(flags) >= 19
    assert [n for n, v in flags.items() if v & capi.ANCHORED_SWEEPS] == ["SC_TICK_ANCHORED_SWEEPS"] and not capi.ANCHORED_SWEEPS & capi.FULL
    assert len(set(flags.values())) == len(flags) and all(v & (v - 1) == 0 for v in flags.values())      # one bit each, no bit twice
    assert re.search(r"enum \{ SC_TICK_SWEEP_END_LOCAL = 0, SC_TICK_SWEEP_END_WORLD_OFFSET = 1 \};", text)
    assert re.search(r"enum \{ SC_TICK_ASWEEP_ANSWERED = 0, SC_TICK_ASWEEP_NO_ANCHOR = 1, SC_TICK_ASWEEP_NOT_FINITE = 2 \};", text)
    assert (capi.SWEEP_END_LOCAL, capi.SWEEP_END_WORLD_OFFSET) == (0, 1) == (ar.END_LOCAL, ar.END_WORLD_OFFSET)
    assert (capi.ASWEEP_ANSWERED, capi.ASWEEP_NO_ANCHOR, capi.ASWEEP_NOT_FINITE) == (0, 1, 2) == (ar.ANSWERED, ar.NO_ANCHOR, ar.NOT_FINITE)
    assert (capi.ANCHOR_NONE, capi.ANCHOR_DEAD) == (ar.ANCHOR_NONE, ar.ANCHOR_DEAD)
    assert C.sizeof(capi.SweepHit) == 48 == SWEEP_HIT_DTYPE.itemsize == ar.HIT_DTYPE.itemsize and "sizeof(ScTickSweepHit) == 48" in text
    assert SWEEP_HIT_DTYPE.fields["pad"][1] == 44 == ar.HIT_DTYPE.fields["pad"][1]
    assert re.search(r"int scTickSetAnchoredSweeps\(ScTickContext\* ctx, uint32_t count, const uint32_t\* anchor, const float\* local_start3, "
                     r"const float\* local_end3,\s*const float\* radius, const float\* half_height, const uint32_t\* mask, const uint8_t\* skip_self,\s*"
                     r"const uint8_t\* end_frame\);", text)
    assert re.search(r"int scTickReadAnchoredSweepHits\(ScTickContext\* ctx, ScTickSweepHit\* hits, uint32_t capacity, uint32_t\* count\);", text)
    assert re.search(r"int scTickReadAnchoredSweepSegments\(ScTickContext\* ctx, uint32_t first, uint32_t count, float\* start3, float\* end3\);", text)
    assert re.search(r"int scTickReadAnchoredSweeps\(ScTickContext\* ctx, uint32_t first, uint32_t count, uint32_t\* anchor\);", text)
    assert re.search(r"int scTickGetAnchoredSweepShapeInfo\(ScTickContext\* ctx, ScTickSweepShapeInfo\* info\);", text)
    lib = capi.load()
    assert lib.scTickGetApiVersion() == 7
    for name in NAMES:
        assert hasattr(lib, name) and name in capi.SYMBOLS
    ctx, u32 = C.c_void_p, C.c_uint32
    assert capi.SYMBOLS["scTickSetAnchoredSweeps"] == (C.c_int, [ctx, u32, capi.U32P, capi.F32P, capi.F32P, capi.F32P, capi.F32P, capi.U32P, capi.U8P, capi.U8P])
    assert capi.SYMBOLS["scTickReadAnchoredSweepHits"] == (C.c_int, [ctx, C.POINTER(capi.SweepHit), u32, capi.U32P])
    assert capi.SYMBOLS["scTickReadAnchoredSweepSegments"] == (C.c_int, [ctx, u32, u32, capi.F32P, capi.F32P])
    assert capi.SYMBOLS["scTickReadAnchoredSweeps"] == (C.c_int, [ctx, u32, u32, capi.U32P])
    assert capi.SYMBOLS["scTickGetAnchoredSweepShapeInfo"] == (C.c_int, [ctx, C.POINTER(capi.SweepShapeInfo)])


def test_a_null_context_is_refused_and_nothing_is_written():
    lib = capi.load()
    info = capi.SweepShapeInfo(9, 9, 9, 9)
    a = (C.c_uint32 * 4)(*([7] * 4))
    s, e = (C.c_float * 3)(*([7.0] * 3)), (C.c_float * 3)(*([7.0] * 3))
    hits = (capi.SweepHit * 1)()
    n = C.c_uint32(7)
    assert lib.scTickSetAnchoredSweeps(None, 0, None, None, None, None, None, None, None, None) == 0
    assert lib.scTickSetAnchoredSweeps(None, 1, a, s, e, s, s, a, None, None) == 0
    assert lib.scTickReadAnchoredSweepHits(None, hits, 1, C.byref(n)) == 0 and lib.scTickReadAnchoredSweepSegments(None, 0, 1, s, e) == 0
    assert lib.scTickReadAnchoredSweeps(None, 0, 1, a) == 0 and lib.scTickGetAnchoredSweepShapeInfo(None, C.byref(info)) == 0
    assert (info.refined, info.kept_as_boxes, info.exhausted, info.pad) == (9, 9, 9, 9) and list(a) == [7] * 4 and n.value == 7
    assert list(s) == [7.0] * 3 and list(e) == [7.0] * 3


def test_no_new_method_of_the_host_class_reads_as_a_setter():
    new = [n for n in dir(WorldTick) if "anchored_sweep" in n]
    assert sorted(new) == ["anchored_sweep_anchors", "anchored_sweep_hits", "anchored_sweep_segments", "anchored_sweep_shape_info", "anchored_sweeps"]
    assert not [n for n in new if n.startswith(("set_", "upload_", "bind_"))]


# ---- the witness's identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_without_an_anchor_and_on_an_identity_anchor_the_witness_is_the_plain_witness(oracle, mode):
    w, col, _ = ac.table(oracle)
    m, mn, mx = ac.table_state(oracle)
    _, _, (a, b, radius, hh, mask, _) = sc.world_case(oracle)
    if mode == ar.EXACT:
        plain, info = ss.sweep32(m, mn, mx, w.group, w.mask, col, a, b, radius, hh, mask, mode=ss.EXACT)
    else:
        plain, info = sweep_ref.sweep_boxes(oracle, mn, mx, w.group, w.mask, a, b, radius, hh, mask), None
    q = ac.unanchored(a, b, radius, hh, mask)
    got, (s, e), got_info = ac.witness(oracle, m, mn, mx, w.group, w.mask, col, q, mode)
    assert got.tobytes() == plain.tobytes() and got_info == info and (got["pad"] == 0).all()
    assert np.array_equal(s.view(U), a.view(U)) and np.array_equal(e.view(U), b.view(U))
    # one more entity whose matrix is the identity, in no group and without a shape: a frame that changes no bit of a point
    eye = np.eye(4, dtype=F).reshape(1, 16)
    m1, mn1, mx1 = np.concatenate([m, eye]), np.concatenate([mn, F([[np.inf] * 3])]), np.concatenate([mx, F([[-np.inf] * 3])])
    group1, mask1 = np.concatenate([w.group, U([0])]), np.concatenate([w.mask, U([0])])
    col1 = None
    if mode == ar.EXACT:
        col1 = sc.colliders(w.n + 1, np.concatenate([col.type, [1]]), he=np.concatenate([col.he, F([[1, 1, 1]])]),
                            radius=np.concatenate([col.radius, F([1])]), hh=np.concatenate([col.hh, F([0])]))
    on_eye = dict(q, anchor=np.full(len(a), w.n, U))
    got1, (s1, e1), info1 = ac.witness(oracle, m1, mn1, mx1, group1, mask1, col1, on_eye, mode)
    assert got1.tobytes() == plain.tobytes() and info1 == info
    # (+0 of the products added to -0 gives +0: compared as values, which the hits just were as bytes)
    assert np.array_equal(s1, a) and np.array_equal(e1, b)
    assert 100 < plain["hit"].sum() < 480


# ---- closed forms -------------------------------------------------------------------------------------------------------------------
def answers(oracle, m, col, q, mode):
    mn, mx = sc.boxes_of(m, col)
    n = len(m)
    return ac.witness(oracle, m, mn, mx, np.ones(n, U), np.full(n, ac.ALL, U), col, q, mode)


def contact64(m, col, target, segments, q):
    typ, shp = shape_records(col, len(m))
    a, b, r, hh = segments[0], segments[1], q["radius"], q["hh"]
    nd, far = sc.ndir_of((a, b))
    return ss.contact64(m, typ, shp, np.full(len(a), target), a, nd, far, r, np.maximum(hh, F(0.0)))


@pytest.mark.parametrize("mode", MODES)
def test_local_plus_x_of_an_entity_yawed_by_ninety_degrees_meets_the_wall_along_world_minus_z(oracle, mode):
    m, col, q, wall = ac.yaw_wall_case()
    hits, (s, e), _ = answers(oracle, m, col, q, mode)
    assert np.array_equal(s[0], F([100, 0, 100])) and np.array_equal(e[0], F([100, 0, 68]))      # (the cosine, 6e-17, drowns in 100)
    assert hits["hit"][0] == 1 and hits["id"][0] == wall and hits["pad"][0] == 0
    tol = float(ss.TOL) if mode == ar.EXACT else 0.0
    assert ac.WALL_TRAVEL - tol <= hits["travel"][0] <= ac.WALL_TRAVEL
    assert np.allclose(hits["position"][0], [100, 0, 100 - hits["travel"][0]], atol=1e-6) and np.allclose(hits["normal"][0], [0, 0, 1], atol=1e-6)
    assert hits["distance"][0] == hits["travel"][0] / F(32.0)
    if mode == ar.EXACT:
        hit64, t64, _, _ = contact64(m, col, wall, (s, e), q)
        assert hit64[0] and abs(t64[0] - ac.WALL_TRAVEL) < 1e-9 and t64[0] - tol - 1e-5 <= hits["travel"][0] <= t64[0] + 1e-5
    # the same numbers read as world space go along +x and find nothing
    world, _, _ = answers(oracle, m, col, dict(q, anchor=U([ac.NONE])), mode)
    assert world["hit"][0] == 0


@pytest.mark.parametrize("mode", MODES)
def test_an_offset_probe_goes_straight_down_from_a_tilted_anchor_and_lands_on_the_slab(oracle, mode):
    m, col, q, slab = ac.tilt_probe_case()
    hits, (s, e), _ = answers(oracle, m, col, q, mode)
    want = ac.PROBE_HEIGHT - (ac.PROBE_HH + ac.PROBE_RADIUS)
    assert np.array_equal(s, F([[60, 3, 60]] * 2)) and np.array_equal(e[0], F([60, -1, 60]))
    # end_frame 0 follows the tilt: (0, -4, 0) through a roll of 30 degrees ends 4 sin 30 = 2 m sideways and only 4 cos 30 = 3.46 m lower
    assert abs(e[1][0] - 62.0) < 1e-5 and abs(e[1][1] - (3.0 - 4.0 * np.cos(np.pi / 6))) < 1e-5 and e[1][2] == 60
    tol = float(ss.TOL) if mode == ar.EXACT else 0.0
    assert hits["hit"][0] == 1 and hits["id"][0] == slab and want - tol <= hits["travel"][0] <= want
    assert np.allclose(hits["normal"][0], [0, 1, 0]) and np.allclose(hits["position"][0], [60, 3 - hits["travel"][0], 60], atol=1e-6)
    assert hits["hit"][1] == 1 and hits["travel"][1] > hits["travel"][0] + 0.3                   # the tilted one travels further to the slab
    if mode == ar.EXACT:
        hit64, t64, _, _ = contact64(m, col, slab, (s, e), q)
        assert hit64.all() and abs(t64[0] - want) < 1e-9
        assert (t64 - tol - 1e-5 <= hits["travel"]).all() and (hits["travel"] <= t64 + 1e-5).all()
    # the chassis' own box lies around the start: without skip_self it answers at once
    seen, _, _ = answers(oracle, m, col, dict(q, skip_self=np.zeros(2, np.uint8)), mode)
    assert (seen["hit"] == 1).all() and (seen["id"] == 0).all() and (seen["travel"] == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_two_ticks_of_a_translated_anchor_shorten_the_travel_by_the_translation(oracle, mode):
    travel = []
    for shift in (0.0, 2.0):
        m, col, q, wall = ac.yaw_wall_case(shift)
        hits, _, _ = answers(oracle, m, col, q, mode)
        assert hits["hit"][0] == 1 and hits["id"][0] == wall
        travel.append(hits["travel"][0])
    # 100 - 81 and 98 - 81 along a direction that is (0, 0, -1) to the bit (far = 32, a power of two): exact in fp32
    assert travel[0] == F(19.0) and travel[1] == F(17.0) and travel[0] - travel[1] == F(2.0)


# ---- the resolve against float64 ----------------------------------------------------------------------------------------------------
def test_the_fp32_resolve_agrees_with_float64_within_four_roundings(oracle):
    w, _, q = ac.table(oracle)
    m, _, _ = ac.table_state(oracle)
    s, e, status = ar.resolve(m, q["anchor"], q["ls"], q["le"], q["end_frame"])
    on = np.flatnonzero((q["anchor"] != ac.NONE) & (status == 0))
    assert len(on) > 400 and s.dtype == F and e.dtype == F
    want, bound = ar.resolve64(m, q["anchor"][on], q["ls"][on])
    assert (np.abs(s[on].astype(np.float64) - want) <= bound).all()
    local = on[q["end_frame"][on] == 0]
    want, bound = ar.resolve64(m, q["anchor"][local], q["le"][local])
    assert len(local) > 150 and (np.abs(e[local].astype(np.float64) - want) <= bound).all()
    off = on[q["end_frame"][on] == 1]
    assert len(off) > 150 and np.array_equal(e[off].view(U), (s[off] + q["le"][off]).view(U))     # the offset frame: one fp32 add
    # the frames are not trivial: sheared, scaled, some of them children of children
    c = m[q["anchor"][on]].reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
    cosine = np.abs((c[:, 0] * c[:, 1]).sum(axis=1)) / (np.linalg.norm(c[:, 0], axis=1) * np.linalg.norm(c[:, 1], axis=1))
    assert (cosine > 0.05).sum() >= 20 and w.parent[q["anchor"][on]].max() >= 0


# ---- the table ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_every_cell_of_the_table_holds_eight_sweeps_and_every_status_occurs(oracle, mode):
    w, col, q = ac.table(oracle)
    hits, segments, info = ac.table_answers(oracle, mode)
    assert len(hits) == 500 == len(q["anchor"]) and w.n == 1200
    cell = ac.cell_of(hits, segments)
    for frame in (0, 1):
        for c, name in enumerate(ac.CELLS):
            assert ((cell == c) & (q["end_frame"] == frame)).sum() >= ac.PER_CELL, (frame, name)
    assert list(hits["pad"][:ac.STATUS_ROWS]) == [1] * 4 + [2] * 4 and (hits["pad"][ac.STATUS_ROWS:] == 0).all()
    gone = hits[:ac.STATUS_ROWS]
    assert (gone["hit"] == 0).all() and (gone["id"] == ar.NO_ID).all() and (gone["travel"] == 0).all() and np.array_equal(gone["normal"], F([[0, 1, 0]] * 8))
    assert (segments[0][:8].view(U) == 0x7FC00000).all() and (segments[1][:8].view(U) == 0x7FC00000).all()
    assert np.isfinite(segments[0][8:]).all() and np.isfinite(segments[1][8:]).all()
    # anchored and world-space rows, seeing and not seeing their anchor, on roots and on children
    on = q["anchor"][8:] != ac.NONE
    assert on.sum() > 400 and (~on).sum() > 20 and 100 < q["skip_self"].sum() < 400
    # the rows that start at their anchor's origin see the anchor at once; told to skip it, they answer otherwise
    own = hits[ac.OWN_ROWS]
    assert (own["hit"] == 1).all() and (own["travel"] == 0).all()
    assert (own["id"] == q["anchor"][ac.OWN_ROWS]).all()
    blind, _, _ = ac.witness(oracle, *ac.table_state(oracle), w.group, w.mask, col, dict(ac.take(q, np.arange(500)[ac.OWN_ROWS]), skip_self=np.ones(20, np.uint8)), mode)
    assert (blind["id"] != q["anchor"][ac.OWN_ROWS]).all() and (blind.tobytes() != own.tobytes())
    for frame in (0, 1):
        assert (q["end_frame"][ac.OWN_ROWS] == frame).sum() >= 8
    if mode == ar.EXACT:
        plain, _, _ = ac.table_answers(oracle, ar.AABB)
        assert info["refined"] > 100 and info["kept_as_boxes"] > 10
        assert ((plain["travel"].view(U) != hits["travel"].view(U)) | (plain["id"] != hits["id"])).sum() > 40


@pytest.mark.parametrize("count", ac.COUNTS)
def test_sweep_counts_leave_waves_without_a_sweep(oracle, count):
    _, _, q = ac.table(oracle)
    tiled, idx = ac.tiled(q, count)
    assert len(tiled["anchor"]) == count == len(idx) and (count % 4 != 0 or count == 4) and ac.COUNTS == (1, 3, 4, 5, 4097)


@pytest.mark.parametrize("kind,where", [("edge", "near"), ("edge", "far"), ("zero", "near"), ("zero", "far"), ("crowded", "near")])
def test_the_walk_rows_keep_their_bits_in_a_translated_frame(oracle, kind, where):
    """the sweep rows of tests/ray_walk_cases.py as the GPU suite sends them: world space, and in the frame of a translated anchor"""
    w, q, role = ac.walk_rows(kind, where)
    none, moved, w2, keep = ac.walk_sets(w, q)
    assert len(keep) >= len(q[0]) // 2 and (role[keep] >= 1).sum() >= 20 and (kind == "crowded" or (role[keep] == 0).sum() >= 10)
    m = np.tile(np.eye(4, dtype=F).reshape(16), (w2.n, 1))
    m[:, 12:15] = w2.pos
    s, e, status = ar.resolve(m, moved["anchor"], moved["ls"], moved["le"], moved["end_frame"])
    assert (status == 0).all() and np.array_equal(s.view(U), q[0][keep].view(U)) and np.array_equal(e.view(U), q[1][keep].view(U))
    assert (moved["anchor"] >= w.n).all() and (none["anchor"] == ac.NONE).all() and not moved["skip_self"].any()
    # the anchored witness over the translated frames is the plain witness of the kept rows
    plain = sweep_ref.sweep_boxes(oracle, w.bmin, w.bmax, w.group, w.mask, *q)
    got, _, _ = ac.witness(oracle, m, w2.bmin, w2.bmax, w2.group, w2.mask, None, moved)
    assert got.tobytes() == plain[keep].tobytes() and (plain["hit"][role >= 1] == 1).all() and (plain["hit"][role == 0] == 0).all()


def test_the_residency_case_relocates_two_anchors_and_kills_one(oracle):
    from tests import trigger_cases as tc
    w, q, removal = ac.residency_case()
    after, names = tc.swap_remove(w, removal)
    moved = ac.renamed(q, names)
    assert list(moved["anchor"]) == [12, ac.DEAD, 13, 13, 2, ac.NONE]
    for world, sweeps, dead in ((w, q, []), (after, moved, [1])):
        m, mn, mx = tc.state(oracle, world)
        hits, _, _ = ac.witness(oracle, m, mn, mx, world.group, world.mask, None, sweeps)
        assert list(np.flatnonzero(hits["pad"])) == dead and (hits["hit"][hits["pad"] == 0] == 1).all()
        assert hits["id"][3] == sweeps["anchor"][3] and hits["travel"][3] == 0 and hits["id"][2] != sweeps["anchor"][2] and hits["travel"][2] > 0
