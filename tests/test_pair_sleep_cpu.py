"""Pair sleep without a GPU: the binding exposes the entry points, and every case of tests/pair_sleep_cases.py is what it claims -- the
run in which each island falls asleep and wakes, the event counts, the rest counts, the overflow rows exceeding their capacity -- derived
from the oracle's pair set through the fp32 touching witness, the islands' witness and the sleep witness of tests/pair_sleep_ref.py, never
from the library.  A second formulation of STILL in float64 agrees on all cases.  The GPU suite (tests/test_gpu_pair_sleep.py) counts on it."""
import ctypes as C

import numpy as np
import pytest

from sc_gameengine_amd import capi
from tests import pair_sleep_cases as SC, pair_sleep_ref as Z


def test_the_binding_exposes_the_entry_points_and_a_32_byte_report():
    assert C.sizeof(capi.PairSleepInfo) == 32
    assert [n for n, _ in capi.PairSleepInfo._fields_] == list(Z.INFO_FIELDS)
    assert (capi.SLEEP_ASLEEP, capi.SLEEP_STILL, capi.SLEEP_MOVABLE) == (Z.ASLEEP, Z.STILL, Z.MOVABLE) == (1 << 8, 1 << 9, 1 << 10)
    assert (capi.SLEEP_INFO_RESYNC, capi.SLEEP_INFO_FELL_OVERFLOW, capi.SLEEP_INFO_WOKE_OVERFLOW, capi.SLEEP_INFO_LIST_TRUNCATED) == \
        (Z.RESYNC, Z.FELL_OVERFLOW, Z.WOKE_OVERFLOW, Z.LIST_TRUNCATED) == (1, 2, 4, 8)
    lib = capi.load()
    u32p, f32p = capi.U32P, capi.F32P
    ctx = capi.SYMBOLS["scTickSetPairSleep"][1][0]
    want = {"scTickSetPairSleep": [ctx, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_uint32],
            "scTickGetPairSleep": [ctx, u32p, f32p, f32p, u32p, u32p],
            "scTickWakeEntities": [ctx, u32p, C.c_uint32],
            "scTickReadPairSleep": [ctx, u32p, C.c_uint32, u32p, C.c_uint32, u32p, C.c_uint32, C.POINTER(capi.PairSleepInfo)]}
    for name, args in want.items():
        assert capi.SYMBOLS[name] == (C.c_int, args)
        assert getattr(lib, name).restype is C.c_int and list(getattr(lib, name).argtypes) == args
    assert lib.scTickGetApiVersion() == 7
    from sc_gameengine_amd.tick import WorldTick
    assert all(callable(getattr(WorldTick, m)) for m in ("pair_sleep", "wake_entities", "read_pair_sleep"))
    assert isinstance(WorldTick.pair_sleep_enabled, property)


@pytest.mark.parametrize("case", SC.CASES, ids=SC.NAMES)
def test_the_case_is_what_it_claims_and_both_formulations_of_still_agree(oracle, case):
    runs = SC.simulate(oracle, case)
    assert len(runs) == len(case.steps) >= 2
    ever = np.zeros(case.w.n, bool)
    for k, (states, fell, woke, info) in enumerate(runs):
        assert info["fell_asleep"] == len(fell) == case.fell.get(k, info["fell_asleep"] if case.name.startswith("random") else 0), f"run {k}: {info}"
        assert info["woke"] == len(woke) == case.woke.get(k, info["woke"] if case.name.startswith("random") else 0), f"run {k}: {info}"
        assert info["epoch"] == k + 1 and bool(info["flags"] & Z.RESYNC) == (k == 0)
        assert bool(info["flags"] & Z.FELL_OVERFLOW) == (len(fell) > case.max_events) and bool(info["flags"] & Z.WOKE_OVERFLOW) == (len(woke) > case.max_events)
        asleep = (states & Z.ASLEEP) != 0
        assert info["asleep"] == int(asleep.sum()) and not (asleep & ((states & Z.MOVABLE) == 0)).any()
        if k in case.rest:
            assert (states & 0xFF).tolist() == case.rest[k], f"run {k}"
        ever |= asleep
    assert not ever[list(case.never_asleep)].any()
    if case.fell or case.woke:
        assert ever.any()
    # the second formulation
    for k, (a, b) in enumerate(zip(runs, SC.simulate(oracle, case, still=Z.still64))):
        assert np.array_equal(a[0], b[0]) and a[3] == b[3], f"run {k}"


def test_the_overflow_rows_exceed_their_lists_and_the_table_covers_the_wave_edges(oracle):
    by_name = dict(zip(SC.NAMES, SC.CASES))
    for cap in (1, 64):
        case = by_name[f"65 events into a list of {cap}"]
        runs = SC.simulate(oracle, case)
        assert runs[3][3]["fell_asleep"] == 65 > cap and runs[3][3]["flags"] & Z.FELL_OVERFLOW
        assert runs[4][3]["woke"] == 33 and bool(runs[4][3]["flags"] & Z.WOKE_OVERFLOW) == (33 > cap)
    assert [by_name[f"{n} islands of one"].w.n for n in SC.COUNTS] == [1, 63, 64, 65, 129]
    for s in SC.RANDOM_SEEDS:
        case = by_name[f"random world of 600, seed {s}"]
        runs = SC.simulate(oracle, case)
        assert case.w.n == 600 and 0.25 < ((case.w.group & SC.STATIC) != 0).mean() < 0.42 and len(runs) == 12
        assert sum(r[3]["fell_asleep"] for r in runs) >= 30 and sum(r[3]["woke"] for r in runs) >= 1      # frozen islands sleep, a pushed fixed body wakes some
        assert runs[-1][3]["asleep"] >= 30 and runs[-1][3]["awake_entries"] >= 100
        assert all(r[3]["fell_asleep"] == 0 for r in runs[:6])      # frozen from run 4 on: at rest in runs 4, 5 and 6
