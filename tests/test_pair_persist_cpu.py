"""Pair persistence without a GPU: the ABI surface, and the witness (tests/pair_persist_ref.py) the GPU tests compare against -- the cases
of tests/pair_persist_cases.py are what they claim by the witness alone, and the witness agrees with float64 distances in `a`'s frame
computed by another route."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sc_gameengine_amd import capi
from tests import pair_manifolds_ref as M, pair_persist_cases as PC, pair_persist_ref as P, pair_shapes_cases as G, pair_shapes_ref as R

F = np.float32
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sc_tick.h")
NAMES = ("scTickSetPairPersistence", "scTickGetPairPersistence", "scTickReadPairPersistence", "scTickWritePairPayloads", "scTickReadPairPayloads")


# ---- 1. the ABI surface -------------------------------------------------------------------------------------------------------------
def test_pair_persistence_symbols_are_exported_and_bound():
    text = open(HEADER).read()
    assert re.search(r"#define\s+SC_TICK_API_VERSION\s+7u", text)
    assert re.search(r"#define\s+SC_TICK_PERSIST_NONE\s+0xFFFFFFFFu", text) and capi.PERSIST_NONE == 0xFFFFFFFF == P.NONE
    struct = re.search(r"typedef struct ScTickPairPersist\s[^{]*\{(.*?)\}\s*ScTickPairPersist;", text, re.S)
    assert struct and re.findall(r"(uint8_t|uint32_t)\s+(\w+)(\[[^;]*\])?;", struct.group(1)) == [
        ("uint32_t", "prev_entry", ""), ("uint8_t", "prev_slot", "[4]"), ("uint8_t", "age", "[4]"), ("uint32_t", "reserved", "")]
    info = re.search(r"typedef struct ScTickPairPersistInfo[^{]*\{(.*?)\}\s*ScTickPairPersistInfo;", text, re.S)
    assert info and re.findall(r"uint32_t\s+(\w+);", info.group(1)) == list(P.INFO_FIELDS)
    assert re.search(r"int scTickSetPairPersistence\(ScTickContext\* ctx, uint32_t enable, float match_dist\);", text)
    assert re.search(r"int scTickGetPairPersistence\(ScTickContext\* ctx, uint32_t\* enabled, float\* match_dist\);", text)
    assert re.search(r"int scTickReadPairPersistence\(ScTickContext\* ctx, ScTickPairPersist\* out, uint32_t capacity, ScTickPairPersistInfo\* info\);", text)
    assert re.search(r"int scTickWritePairPayloads\(ScTickContext\* ctx, const float\* rows, uint32_t first, uint32_t count\);", text)
    assert re.search(r"int scTickReadPairPayloads\(ScTickContext\* ctx, float\* rows, uint32_t capacity\);", text)
    # no new run flag: bits 16 and up stay free of public flags
    assert not re.search(r"SC_TICK_\w+\s*=\s*1u\s*<<\s*(1[6-9]|2\d|3[01])\s*,", text)
    lib = capi.load()
    for name in NAMES:
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert lib.scTickGetApiVersion() == 7
    assert capi.SYMBOLS["scTickSetPairPersistence"] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_float])
    assert capi.SYMBOLS["scTickGetPairPersistence"] == (C.c_int, [C.c_void_p, capi.U32P, capi.F32P])
    assert capi.SYMBOLS["scTickReadPairPersistence"] == (C.c_int, [C.c_void_p, C.POINTER(capi.PairPersist), C.c_uint32, C.POINTER(capi.PairPersistInfo)])
    assert capi.SYMBOLS["scTickWritePairPayloads"] == (C.c_int, [C.c_void_p, capi.F32P, C.c_uint32, C.c_uint32])
    assert capi.SYMBOLS["scTickReadPairPayloads"] == (C.c_int, [C.c_void_p, capi.F32P, C.c_uint32])
    assert C.sizeof(capi.PairPersist) == 16 == P.DTYPE.itemsize and C.sizeof(capi.PairPersistInfo) == 32
    for name, at in dict(prev_entry=0, prev_slot=4, age=8, reserved=12).items():
        assert getattr(capi.PairPersist, name).offset == at == P.DTYPE.fields[name][1], name
    assert tuple(n for n, _ in capi.PairPersistInfo._fields_) == P.INFO_FIELDS
    # a NULL context: every call returns 0 and writes nothing
    info = capi.PairPersistInfo(*([9] * 8))
    rec = (capi.PairPersist * 2)()
    C.memset(rec, 0x5A, C.sizeof(rec))
    rows = (C.c_float * 32)(*([1.5] * 32))
    on, dist = C.c_uint32(7), C.c_float(7.0)
    assert lib.scTickSetPairPersistence(None, 1, 0.02) == 0 and lib.scTickSetPairPersistence(None, 0, 0.0) == 0
    assert lib.scTickGetPairPersistence(None, C.byref(on), C.byref(dist)) == 0 and lib.scTickGetPairPersistence(None, None, None) == 0
    assert on.value == 7 and dist.value == 7.0
    assert lib.scTickReadPairPersistence(None, rec, 2, C.byref(info)) == 0 and lib.scTickReadPairPersistence(None, None, 0, None) == 0
    assert lib.scTickWritePairPayloads(None, rows, 0, 2) == 0 and lib.scTickWritePairPayloads(None, None, 0, 0) == 0
    assert lib.scTickReadPairPayloads(None, rows, 2) == 0 and lib.scTickReadPairPayloads(None, None, 0) == 0
    assert info.written == 9 and info.gave_up == 9 and bytes(rec) == b"\x5A" * 32 and list(rows) == [1.5] * 32


# ---- 2. the cases, by the witness alone ---------------------------------------------------------------------------------------------
def witness_run(oracle, w, col, prev, match_dist=PC.MATCH_DIST):
    """a flagged run of the witnesses over world w: the touching unit pairs in ascending order, their manifolds, the persistence answer"""
    m = G.oracle_matrices(oracle, w)
    pairs = PC.unit_pairs(w.n)
    touching, _ = R.touching32(m, col, pairs)
    listed = pairs[touching]
    man = M.manifolds32(m, col, listed)
    rec, rows, info = P.persist32(prev, listed, man, m, match_dist)
    return P.Run(listed, man, rec, rows, m), info


def moved(w, pos, rot=None):
    w2 = G.flat_world(pos, w.rot if rot is None else rot, w.scale)
    return w2


def tallies(run, prev):
    """(kept points, new points, entries with both, entries in which a kept point changed its slot) of a run"""
    count, slot = run.manifolds["count"], run.records["prev_slot"]
    live = np.arange(4)[None, :] < count[:, None]
    kept = live & (slot != 0xFF)
    new = live & (slot == 0xFF)
    changed = (kept & (slot != np.arange(4)[None, :])).any(axis=1)
    return int(kept.sum()), int(new.sum()), int((kept.any(axis=1) & new.any(axis=1)).sum()), int(changed.sum())


@pytest.fixture(scope="module")
def slide_runs(oracle):
    out = []
    for seed in PC.SEEDS:
        w, col, pos2 = PC.slide_world(seed)
        first, info1 = witness_run(oracle, w, col, None)
        second, info2 = witness_run(oracle, moved(w, pos2), col, first)
        out.append((first, info1, second, info2))
    return out


def test_the_slide_worlds_hold_their_floors(slide_runs):
    total = np.zeros(4, np.int64)
    for first, info1, second, info2 in slide_runs:
        assert info1["resync"] == 1 and info1["kept_pairs"] == 0 and info1["kept_points"] == 0 and info1["new_points"] == int(first.manifolds["count"].sum())
        assert (first.records["prev_entry"] == P.NONE).all() and not first.records["age"].any() and not first.payloads.any()
        got = tallies(second, first)
        assert got[0] == info2["kept_points"] and got[1] == info2["new_points"] and info2["resync"] == 0
        total += got
    print("slide worlds: kept, new, mixed entries, moved-slot entries =", total.tolist())
    assert total[0] >= PC.FLOORS["kept_points"] and total[1] >= PC.FLOORS["new_points"]
    assert total[2] >= PC.FLOORS["mixed_entries"] and total[3] >= PC.FLOORS["moved_slot_entries"]


def test_the_witness_agrees_with_float64_distances_in_the_first_members_frame(slide_runs):
    for first, _, second, _ in slide_runs:
        x, y = P.local_points64(second.matrices, second.listed, second.manifolds), P.local_points64(first.matrices, first.listed, first.manifolds)
        at = {int(k): i for i, k in reversed(list(enumerate(P.keys(first.listed))))}
        singles = 0
        for i, key in enumerate(P.keys(second.listed)):
            pe = at.get(int(key), P.NONE)
            assert pe == int(second.records["prev_entry"][i])
            if pe == P.NONE:
                continue
            for s in range(int(second.manifolds["count"][i])):
                t = int(second.records["prev_slot"][i, s])
                if t != 0xFF:                              # every kept slot is within the match distance
                    assert np.linalg.norm(x[i, s] - y[pe, t]) <= PC.MATCH_DIST + 1e-4
            if second.manifolds["count"][i] == 1 and first.manifolds["count"][pe] == 1 and np.linalg.norm(x[i, 0] - y[pe, 0]) < PC.MATCH_DIST - 1e-4:
                singles += 1                               # one point in both runs, clearly within it: kept
                assert second.records["prev_slot"][i, 0] == 0 and second.records["age"][i, 0] == 1
        assert singles >= 5


def test_the_carry_worlds_keep_every_point_with_its_slot(oracle):
    for seed in PC.SEEDS:
        w, col, pos2 = PC.carry_world(seed)
        first, _ = witness_run(oracle, w, col, None)
        first.payloads[:] = np.arange(first.payloads.size, dtype=F).reshape(first.payloads.shape) + F(1.0)      # (slots at or above count too)
        second, info = witness_run(oracle, moved(w, pos2), col, first)
        assert np.array_equal(second.listed, first.listed) and np.array_equal(second.manifolds["count"], first.manifolds["count"])
        live = np.arange(4)[None, :] < second.manifolds["count"][:, None]
        assert np.array_equal(second.records["prev_slot"][live], np.broadcast_to(np.arange(4, dtype=np.uint8), live.shape)[live])
        assert (second.records["prev_slot"][~live] == 0xFF).all() and (second.records["age"][live] == 1).all() and not second.records["age"][~live].any()
        assert info["new_points"] == 0 and info["kept_pairs"] == len(first.listed) and info["kept_points"] == int(live.sum())
        assert np.array_equal(second.payloads[live], first.payloads[live]) and not P.row_bits(second.payloads[~live]).any()


def test_the_constructed_sequence_is_what_its_motions_say(oracle):
    w, col, cases, pos3, rot3 = PC.constructed()
    one, _ = witness_run(oracle, w, col, None)
    two, info2 = witness_run(oracle, w, col, one)
    live = np.arange(4)[None, :] < two.manifolds["count"][:, None]
    assert info2["new_points"] == 0 and (two.records["age"][live] == 1).all() and np.array_equal(two.records["prev_entry"], np.arange(len(two.listed)))
    three, info3 = witness_run(oracle, moved(w, pos3, rot3), col, two)
    entry = {int(a) // 2: i for i, a in enumerate(three.listed[:, 0])}
    seen = set()
    for i, case in enumerate(cases):
        how = PC.MOTIONS.get(case[0])
        seen.add(how)
        if how == PC.LIFTED:
            assert i not in entry
            continue
        r, n = three.records[entry[i]], int(three.manifolds["count"][entry[i]])
        assert n == int(two.manifolds["count"][i]) and int(r["prev_entry"]) == i, case[0]
        if how == PC.SLID_FIVE:
            assert n == 2 and r["prev_slot"].tolist() == [0xFF] * 4 and r["age"].tolist() == [0] * 4
        else:                                               # unchanged, carried, slid within the distance, turned with the slab: kept in place
            assert r["prev_slot"].tolist() == list(range(n)) + [0xFF] * (4 - n) and r["age"].tolist() == [2] * n + [0] * (4 - n), case[0]
        if how == PC.TURNED:                                # ... although the points moved by decimetres in world space
            assert n == 4 and np.abs(three.manifolds["point"][entry[i]] - two.manifolds["point"][i]).max() > 0.1
    assert seen >= {PC.TURNED, PC.SLID_A_CENTIMETRE, PC.SLID_FIVE, PC.CARRIED, PC.LIFTED, None}


def test_a_pair_named_twice_matches_the_smallest_remembered_entry_from_both_entries(oracle):
    w, col, _ = PC.slide_world(PC.SEEDS[0])
    first, _ = witness_run(oracle, w, col, None)
    pick = np.array([3, 7, 3, 9, 7, 3])                        # a remembered list that names two pairs more than once
    m = first.matrices
    rows = (np.arange(len(pick) * 16, dtype=F) + F(1.0)).reshape(-1, 4, 4)
    rec1, _, _ = P.persist32(None, first.listed[pick], first.manifolds[pick], m, PC.MATCH_DIST)
    prev = P.Run(first.listed[pick], first.manifolds[pick], rec1, rows, m)
    now = np.array([7, 3, 3, 11])
    rec, carried, info = P.persist32(prev, first.listed[now], first.manifolds[now], m, PC.MATCH_DIST)
    assert rec["prev_entry"].tolist() == [1, 0, 0, P.NONE] and info["kept_pairs"] == 3 and info["new_pairs"] == 1
    n = int(first.manifolds["count"][3])
    assert n >= 1 and rec["prev_slot"][1].tolist() == rec["prev_slot"][2].tolist() == list(range(n)) + [0xFF] * (4 - n)
    assert np.array_equal(carried[1], carried[2]) and np.array_equal(carried[1, :n], rows[0, :n]) and not carried[3].any()
