"""Pair manifolds without a GPU: the ABI surface, and the witnesses (tests/pair_manifolds_ref.py) the GPU tests compare against -- the fp32
witness written from the header answers the constructed cases as their closed forms say, and agrees with float64 geometry computed by
another route (half-plane intersection, exact segment and slab geometry) on the resting worlds and the agreement worlds."""
import ctypes as C
import os
import re

import numpy as np

from sc_gameengine_amd import capi
from tests import collider_ref as cr, pair_contacts_ref as K, pair_manifolds_cases as MC, pair_manifolds_ref as M, pair_shapes_cases as G, pair_shapes_ref as R

F = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sc_tick.h")
TOL = 1e-3                # metres: the contact margin of the contact test
LEFT_OUT_CAP = 0.005      # at most 0.5 % of a seed's touching pairs may lie within TOL of contact
KINDS = dict(NONE=0, SINGLE=1, SEGMENT=2, FACE=3)
FLOORS = dict(face=100, reduced=20, capsule_face_two=50, capsule_capsule_two=50)      # the robust subset, over the resting seeds together


# ---- 1. the ABI surface -------------------------------------------------------------------------------------------------------------
def test_pair_manifold_symbols_are_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"#define\s+SC_TICK_API_VERSION\s+7u", text)
    for name, value in KINDS.items():
        assert re.search(rf"#define\s+SC_TICK_MANIFOLD_{name}\s+{value}u", text), name
        assert getattr(capi, "MANIFOLD_" + name) == value == getattr(M, name)
    assert re.search(r"#define\s+SC_TICK_MANIFOLD_REDUCED\s+\(1u << 8\)", text) and capi.MANIFOLD_REDUCED == 1 << 8 == M.REDUCED
    assert re.search(r"#define\s+SC_TICK_MANIFOLD_SKIN\s+2\.5e-4f", text) and float(M.SKIN32) == float(F(2.5e-4))
    assert re.search(r"#define\s+SC_TICK_MANIFOLD_FLAT\s+1e-3f", text) and float(M.FLAT32) == float(F(1e-3))
    struct = re.search(r"typedef struct ScTickPairManifold\s[^{]*\{(.*?)\}\s*ScTickPairManifold;", text, re.S)
    assert struct and re.findall(r"(float|uint32_t)\s+(\w+)(\[[^;]*\])?;", struct.group(1)) == [
        ("float", "point", "[4][3]"), ("float", "depth", "[4]"), ("uint32_t", "count", ""), ("uint32_t", "kind", ""), ("uint32_t", "reserved", "[2]")]
    info = re.search(r"typedef struct ScTickPairManifoldInfo[^{]*\{(.*?)\}\s*ScTickPairManifoldInfo;", text, re.S)
    assert info and re.findall(r"uint32_t\s+(\w+);", info.group(1)) == list(M.INFO_FIELDS)
    assert re.search(r"int scTickSetPairManifolds\(ScTickContext\* ctx, uint32_t enable\);", text)
    assert re.search(r"int scTickGetPairManifolds\(ScTickContext\* ctx, uint32_t\* enabled\);", text)
    assert re.search(r"int scTickReadPairManifolds\(ScTickContext\* ctx, ScTickPairManifold\* out, uint32_t capacity, ScTickPairManifoldInfo\* info\);", text)
    # no new run flag: bits 16 and up stay free of public flags
    assert not re.search(r"SC_TICK_\w+\s*=\s*1u\s*<<\s*(1[6-9]|2\d|3[01])\s*,", text)
    lib = capi.load()
    for name in ("scTickSetPairManifolds", "scTickGetPairManifolds", "scTickReadPairManifolds"):
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert lib.scTickGetApiVersion() == 7
    assert capi.SYMBOLS["scTickSetPairManifolds"] == (C.c_int, [C.c_void_p, C.c_uint32])
    assert capi.SYMBOLS["scTickGetPairManifolds"] == (C.c_int, [C.c_void_p, capi.U32P])
    assert capi.SYMBOLS["scTickReadPairManifolds"] == (C.c_int, [C.c_void_p, C.POINTER(capi.PairManifold), C.c_uint32, C.POINTER(capi.PairManifoldInfo)])
    assert C.sizeof(capi.PairManifold) == 80 == M.DTYPE.itemsize and C.sizeof(capi.PairManifoldInfo) == 32
    offsets = dict(point=0, depth=48, count=64, kind=68)
    for name, at in offsets.items():
        assert getattr(capi.PairManifold, name).offset == at == M.DTYPE.fields[name][1], name
    assert tuple(n for n, _ in capi.PairManifoldInfo._fields_) == M.INFO_FIELDS
    # a NULL context: every call returns 0 and writes nothing
    info = capi.PairManifoldInfo(*([9] * 8))
    rec = (capi.PairManifold * 2)()
    C.memset(rec, 0x5A, C.sizeof(rec))
    on = C.c_uint32(7)
    assert lib.scTickSetPairManifolds(None, 1) == 0 and lib.scTickSetPairManifolds(None, 0) == 0
    assert lib.scTickGetPairManifolds(None, C.byref(on)) == 0 and lib.scTickGetPairManifolds(None, None) == 0 and on.value == 7
    assert lib.scTickReadPairManifolds(None, rec, 2, C.byref(info)) == 0 and lib.scTickReadPairManifolds(None, None, 0, None) == 0
    assert info.written == 9 and info.reduced == 9 and bytes(rec) == b"\x5A" * 160


# ---- 2. closed forms ----------------------------------------------------------------------------------------------------------------
def test_constructed_cases_answer_as_their_closed_forms_say(oracle):
    w, col, cases, origins = MC.manifold_world()
    m = G.oracle_matrices(oracle, w)
    k = len(cases)
    pairs = np.stack([2 * np.arange(k), 2 * np.arange(k) + 1], axis=1).astype(np.uint32)
    touching, refined = R.touching32(m, col, pairs)
    assert touching.all()
    rec = M.manifolds32(m, col, pairs)
    contact = K.contacts32(m, col, pairs)
    for i, (name, count, kind, points, depth, *_) in enumerate(cases):
        r = rec[i]
        n = int(r["count"])
        assert int(r["kind"]) == kind, (name, int(r["kind"]), n)
        assert (n == count) if count is not None else (1 <= n <= 2), (name, n)
        assert not M.bits(rec[i:i + 1])[0, 18:].any() and not r["point"][n:].view(np.uint32).any() and not r["depth"][n:].view(np.uint32).any(), name
        if kind == M.NONE:
            assert not M.bits(rec[i:i + 1]).any(), name
            continue
        got = r["point"][:n].astype(np.float64) - origins[i]
        want = np.asarray(points, np.float64)
        far = np.abs(got[:, None, :] - want[None, :, :]).max(axis=2)          # [got][want]
        assert (far.min(axis=1) < 1e-4).all(), (name, got)
        assert len(set(far.argmin(axis=1).tolist())) == n, (name, got)         # n different ones of the expected points
        assert kind & M.REDUCED or len(want) == n, name
        assert np.abs(r["depth"][:n] - depth).max() < 1e-4, (name, r["depth"])
        if kind == M.SINGLE:
            assert np.array_equal(r["point"][0].view(np.uint32), contact["point"][i].view(np.uint32)), name
            assert r["depth"][0].view(np.uint32) == contact["depth"][i].view(np.uint32), name
    assert M.report(rec) == dict(written=k, points=int(rec["count"].sum()), with_one=7, with_two=6, with_three=0, with_four=3, face=5, reduced=1)
    # the constructed world's own AABB pair list names every case, so the GPU suite meets each of them
    listed = G.oracle_pairs(oracle, m, col, w)
    assert listed.tolist() == pairs.tolist()


# ---- 3. the two witnesses agree -----------------------------------------------------------------------------------------------------
def match(got, want):
    """largest distance from a point of either set to its nearest of the other (inf when exactly one is empty)"""
    if not len(got) or not len(want):
        return 0.0 if len(got) == len(want) else np.inf
    far = np.linalg.norm(got[:, None, :] - want[None, :, :], axis=2)
    return max(float(far.min(axis=1).max()), float(far.min(axis=0).max()))


def agreement(oracle, w, col, seed, worst, tally):
    """one world: the properties over every pair clear of contact, the exact match over the float64 witness's robust subset"""
    m = G.oracle_matrices(oracle, w)
    pairs = G.oracle_pairs(oracle, m, col, w)
    touching, refined = R.touching32(m, col, pairs)
    assert refined.all()
    pairs = pairs[touching]
    rec, contact = M.manifolds32(m, col, pairs), K.contacts32(m, col, pairs)
    gap = R.gap64(m, col, pairs)
    clear = np.abs(gap) > TOL                                  # what is left out is decided by the float64 witness alone
    left_out = int((~clear).sum())
    kind, count = rec["kind"] & 0xFF, rec["count"].astype(np.int64)
    print(f"seed {seed}: {len(pairs)} touching, {left_out} within {TOL} m of contact, kinds {np.bincount(kind, minlength=4).tolist()}, "
          f"counts {np.bincount(count, minlength=5).tolist()}, reduced {int(((rec['kind'] & M.REDUCED) != 0).sum())}")
    assert left_out <= LEFT_OUT_CAP * len(pairs)
    sa, sb = K.Shapes64(m, col, pairs[:, 0]), K.Shapes64(m, col, pairs[:, 1])
    # slots beyond count are +0, depths are not negative, a SINGLE record's slot 0 is the contact record's
    live = np.arange(4)[None, :] < count[:, None]
    assert not rec["point"].view(np.uint32)[~live].any() and not rec["depth"].view(np.uint32)[~live].any() and not rec["reserved"].any()
    assert (rec["depth"][live] >= 0).all() and (count[kind != M.NONE] >= 1).all() and (count <= 4).all()
    single = kind == M.SINGLE
    assert np.array_equal(rec["point"][single, 0].view(np.uint32), contact["point"][single].view(np.uint32))
    assert np.array_equal(rec["depth"][single, 0].view(np.uint32), contact["depth"][single].view(np.uint32))
    # per point: between the two surfaces along the contact normal, within TOL of both shapes, the depth the overlap there
    rows, slots = np.nonzero(live & clear[:, None] & ~single[:, None])      # (a SINGLE point is the contact test's business)
    p, depth = rec["point"][rows, slots].astype(np.float64), rec["depth"][rows, slots].astype(np.float64)
    n = contact["normal"][rows].astype(np.float64)
    n /= np.linalg.norm(n, axis=1)[:, None]
    pa, pb = K.Shapes64(m, col, pairs[rows, 0]), K.Shapes64(m, col, pairs[rows, 1])
    pn = np.einsum("ij,ij->i", p, n)
    values = dict(slab=np.maximum(pb.extent(n)[1] - pn, pn - pa.extent(n)[0]), near_both=np.maximum(pa.distance(p), pb.distance(p)),
                  depth_vs_overlap=np.abs(M.overlap_at64(pa, pb, p, n) - depth))
    # a FACE point lies inside the reference face's side slabs
    face = kind[rows] == M.FACE
    of_b = (contact["kind"][rows] & 0xFF) == K.BOX_FACE_B
    ref_u, ref_T, ref_H = np.where(of_b[:, None, None], pb.u, pa.u), np.where(of_b[:, None], pb.T, pa.T), np.where(of_b[:, None], pb.H, pa.H)
    y = np.einsum("ekc,ec->ek", ref_u, p - ref_T)
    along = np.abs(np.einsum("ekc,ec->ek", ref_u, n))
    side = np.where(along >= along.max(axis=1, keepdims=True), -np.inf, np.abs(y) - ref_H).max(axis=1)
    values["face_side_slabs"] = np.where(face, side, -np.inf)
    bad = {}
    for name, value in values.items():
        if len(value):
            worst[name] = max(worst.get(name, -np.inf), float(value.max()))
            over = ~(value <= TOL)
            if over.any():
                print(f"  {name}: {int(over.sum())} of {len(value)} points beyond {TOL} m, by manifold kind {np.bincount(kind[rows][over], minlength=4).tolist()}, "
                      f"largest by kind {[float(f'{value[over & (kind[rows] == k)].max():.3g}') if (over & (kind[rows] == k)).any() else 0.0 for k in range(4)]}")
            bad[name] = [(pairs[rows[j]].tolist(), int(rec["kind"][rows[j]]), int(contact["kind"][rows[j]]), float(value[j])) for j in np.flatnonzero(~(value <= TOL))[:4]]
    # the float64 witness pair by pair: the exact match on its robust subset, the area a REDUCED record spans
    for i in np.flatnonzero(clear):
        normal = contact["normal"][i].astype(np.float64)
        want = M.expect64(sa, sb, i, normal / max(np.linalg.norm(normal), 1e-30))
        if want is None:
            assert kind[i] == M.SINGLE, pairs[i]
            continue
        got = rec["point"][i, :count[i]].astype(np.float64)
        reduced = bool(rec["kind"][i] & M.REDUCED)
        if reduced and want.kind == M.FACE and len(want.points) > 4:
            To, e1, e2 = want.frame
            area = M._polygon_area(np.stack([(got - To) @ e1, (got - To) @ e2], axis=1))
            worst["reduced_area_share"] = min(worst.get("reduced_area_share", np.inf), area / want.area)
            tally["reduced_checked"] += 1
            assert area >= 0.5 * want.area - 1e-9, (seed, pairs[i].tolist(), area, want.area)
        if not want.robust:
            continue
        caps = int(col.type[pairs[i, 0]] == cr.CAPSULE) + int(col.type[pairs[i, 1]] == cr.CAPSULE)
        assert kind[i] == want.kind, (seed, pairs[i].tolist(), int(kind[i]), want.kind)
        if want.kind == M.SINGLE:
            continue
        if len(want.points) > 4:
            assert reduced and 3 <= count[i] <= 4, (seed, pairs[i].tolist(), int(count[i]))
            far = np.linalg.norm(got[:, None, :] - want.points[None, :, :], axis=2)
            assert far.min(axis=1).max() <= TOL and len(set(far.argmin(axis=1).tolist())) == count[i], (seed, pairs[i].tolist(), got, want.points)
            tally["face"] += 1; tally["reduced"] += 1
            continue
        assert not reduced and count[i] == len(want.points), (seed, pairs[i].tolist(), int(count[i]), len(want.points))
        d = match(got, want.points)
        worst["robust_point"] = max(worst.get("robust_point", 0.0), d)
        assert d <= TOL, (seed, pairs[i].tolist(), got, want.points)
        dd = float(np.abs(np.sort(rec["depth"][i, :count[i]].astype(np.float64)) - np.sort(want.depths)).max())
        worst["robust_depth"] = max(worst.get("robust_depth", 0.0), dd)
        assert dd <= TOL, (seed, pairs[i].tolist(), rec["depth"][i], want.depths)
        tally["face"] += int(want.kind == M.FACE)
        tally["capsule_face_two"] += int(want.kind == M.SEGMENT and caps == 1 and count[i] == 2)
        tally["capsule_capsule_two"] += int(want.kind == M.SEGMENT and caps == 2 and count[i] == 2)
    return bad


def test_fp32_manifolds_agree_with_float64_geometry_on_the_resting_worlds(oracle):
    worst, tally = {}, dict(face=0, reduced=0, capsule_face_two=0, capsule_capsule_two=0, reduced_checked=0)
    bad = {}
    for seed in MC.RESTING_SEEDS:
        w, col, _ = MC.resting_world(seed)
        for name, rows in agreement(oracle, w, col, seed, worst, tally).items():
            bad.setdefault(name, []).extend(rows)
    print("robust subset:", tally)
    print("largest deviations:", {k: float(f"{v:.3g}") for k, v in worst.items()})
    assert all(tally[k] >= v for k, v in FLOORS.items()), tally
    assert not any(bad.values()), bad


_AGREEMENT = {}


def agreement_worlds(oracle):
    """the three agreement worlds once, for the two tests below"""
    if not _AGREEMENT:
        worst, tally = {}, dict(face=0, reduced=0, capsule_face_two=0, capsule_capsule_two=0, reduced_checked=0)
        bad = {}
        for seed in G.AGREEMENT_SEEDS:
            w, col = G.agreement_world(seed)
            for name, rows in agreement(oracle, w, col, seed, worst, tally).items():
                bad.setdefault(name, []).extend(rows)
        print("robust subset:", tally)
        print("largest deviations:", {k: float(f"{v:.3g}") for k, v in worst.items()})
        _AGREEMENT.update(bad=bad, tally=tally)
    return _AGREEMENT["bad"], _AGREEMENT["tally"]


def test_fp32_manifolds_agree_with_float64_geometry_on_the_agreement_worlds(oracle):
    """random orientations, overlaps of up to a metre: the exact match on the robust subset, the bit rules, the slab between the two
    surfaces, the reference face's side slabs and the area a REDUCED record spans (all asserted inside agreement())"""
    bad, tally = agreement_worlds(oracle)
    assert tally["face"] >= 50, tally                          # (these worlds hardly hold a lying capsule: the floors are the resting worlds')
    assert not bad["slab"] and not bad["face_side_slabs"], bad


def test_points_and_depths_of_deep_random_overlaps_on_the_agreement_worlds(oracle):
    """shapes up to a metre inside each other at random angles: every point of every manifold still lies within TOL of both shapes, and
    its depth is the two shapes' float64 overlap on the line through it along the contact's normal.  Without the keep conditions of the
    spec (the point within SC_TICK_MANIFOLD_SKIN of the other box, a round's centre line within SC_TICK_MANIFOLD_FLAT of lying across the
    line, a capsule end that reaches the box) 17 to 34 of about 400 points per seed lay up to 0.33 m outside a shape and 109 to 157
    depths missed the line's overlap by up to 1.74 m: an inclined capsule's end, the vertex of a steeply leaning face."""
    bad, _ = agreement_worlds(oracle)
    assert not bad["near_both"] and not bad["depth_vs_overlap"], {k: bad[k][:3] for k in ("near_both", "depth_vs_overlap")}
