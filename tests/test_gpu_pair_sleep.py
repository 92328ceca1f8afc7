"""Pair sleep (scTickSetPairSleep) through the C ABI against the witness of tests/pair_sleep_ref.py.  Every case of
tests/pair_sleep_cases.py runs eager and with graph mode on: state words and report must equal the witness over what the same run read
back -- matrices, labels, edge islands, the listed pairs -- bit for bit, the event lists as sets (a short list: a subset, with the true
counts), and all of it the oracle-derived simulation of the case.  The cases themselves are checked without a GPU in
tests/test_pair_sleep_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from sc_gameengine_amd import capi, synth_world as sw
from sc_gameengine_amd.tick import WorldTick
from tests import collider_ref as cr, pair_contacts_ref as K, pair_islands_cases as PC, pair_manifolds_ref as M, pair_shapes_cases as G, \
    pair_shapes_ref as R, pair_sleep_cases as SC, pair_sleep_ref as Z
from tests.test_gpu_pair_shapes import start

pytestmark = pytest.mark.gpu
FLAGS = capi.XFORM | capi.BROADPHASE
SHAPES = FLAGS | capi.PAIR_SHAPES
F = np.float32
SENTINEL = 0x5A5A5A5A
BIG = 1 << 16
U32P = C.POINTER(C.c_uint32)


def words_of(w):
    return (w.group & 0xFFFF) | ((w.mask & 0xFFFF) << 16)


def check_sleep(t, z, words, fixed_groups):
    """the rest state of the last flagged run against the witness `z` over what that run read back; returns (states, fell, woke, info)"""
    m = t.world_matrices()
    listed, _ = t.read_pair_shapes()
    labels, edge, iinfo = t.read_pair_islands()
    assert iinfo["gave_up"] == 0
    states, fell, woke, info = t.read_pair_sleep()
    ws, wf, ww, wi = z.run(m, words, fixed_groups, labels, listed, edge, iinfo["list_truncated"])
    assert info == wi, f"{info} != {wi}"
    assert len(states) == t.n and np.array_equal(states, ws), f"{int((states != ws).sum())} of {t.n} state words differ"
    for got, want in ((fell, wf), (woke, ww)):
        if len(want) > z.max_events:                        # a short list: max_events distinct members of the true set
            assert len(got) == z.max_events and len(np.unique(got)) == len(got) and np.isin(got, want).all()
        else:
            assert np.array_equal(np.sort(got), np.sort(want))
    return states, fell, woke, info


def drive(t, case, k):
    """run k of a case: its wake call, its locals (or its patched matrices, or nothing), one flagged run"""
    step = case.steps[k]
    if step.wake is not None:
        t.wake_entities(step.wake)
    if step.hold:
        t.run(SHAPES & ~capi.XFORM)
        return
    t.upload_locals(0, step.pos, case.w.rot, step.scale)
    if not step.patch:
        t.run(SHAPES)
        return
    t.run(capi.XFORM)                                       # (not a flagged run: the rest state stays as it is)
    m = t.world_matrices().copy()
    for e, idx, value in step.patch:
        m[e, idx] = value
    t.upload_world_matrices(0, m)
    t.run(SHAPES & ~capi.XFORM)


# ---- 1. the case table, eager and from captured graphs over both tick parities -----------------------------------------------------
@pytest.mark.parametrize("graph", (False, True), ids=("eager", "graph"))
@pytest.mark.parametrize("case", SC.CASES, ids=SC.NAMES)
def test_case_against_the_witness_and_the_oracle_derived_simulation(oracle, case, graph):
    t = start(case.w, case.col, max_pairs=1 << 18)
    t.pair_islands(True, case.fixed_groups)
    t.pair_sleep(True, **case.params())
    on, lin, ang, runs, cap = t.pair_sleep_params()
    assert t.pair_sleep_enabled and on and (F(lin), F(ang), runs, cap) == (F(case.lin_tol), F(case.ang_tol), case.rest_runs, case.max_events)
    if graph:
        t.set_graph_mode(True)                              # run 0 learns, runs 1 and 2 capture a parity each, the others replay
    z = Z.Witness(rank=0, **case.params())
    want = SC.simulate(oracle, case)
    plain = not any(s.patch or s.hold for s in case.steps)
    learn = None
    for k in range(len(case.steps)):
        if case.steps[k].wake is not None:
            z.wake(case.steps[k].wake)
        drive(t, case, k)
        states, fell, woke, info = check_sleep(t, z, case.words(), case.fixed_groups)
        assert np.array_equal(t.world_matrices(), SC.reference(oracle, case, k)[0], equal_nan=True), f"run {k}: matrices differ from the oracle"
        assert info == want[k][3], f"run {k}: {info} != {want[k][3]}"
        assert np.array_equal(states, want[k][0]), f"run {k}"
        if k == 3:
            learn = t.learn_ticks()
    if graph and plain and learn is not None and len(case.steps) <= 16:      # (the home slots age: a long case learns them afresh now and then)
        assert t.learn_ticks() == learn                     # replay = graph mode and no learn tick: the runs behind run 3 were replays
    t.close()


# ---- 2. an eager and a graph twin side by side through every setter -----------------------------------------------------------------
def test_an_eager_and_a_graph_twin_agree_after_every_setter(oracle):
    case = SC.random_world(4143)
    w, col = case.w, case.col
    eager, graph = start(w, col), start(w, col)
    graph.set_graph_mode(True)
    twins = (eager, graph)
    words = case.words()
    z = Z.Witness(lin_tol=SC.TOL, ang_tol=SC.TOL, rest_runs=2, max_events=4096)
    tick = [0]

    def phase(ticks, on=True):
        """every read equal after every tick, the graph twin held to the witness; returns the last report"""
        info = None
        for _ in range(ticks):
            step = case.steps[min(tick[0], len(case.steps) - 1)]
            tick[0] += 1
            for t in twins:
                t.upload_locals(0, step.pos, w.rot, step.scale)
                t.run(SHAPES)
            if not on:
                for t in twins:
                    with pytest.raises(capi.ScTickError, match="pair sleep was not enabled"):
                        t.read_pair_sleep()
                continue
            a, b = eager.read_pair_sleep(), graph.read_pair_sleep()
            assert a[3] == b[3] and np.array_equal(a[0], b[0]) and np.array_equal(np.sort(a[1]), np.sort(b[1])) and np.array_equal(np.sort(a[2]), np.sort(b[2]))
            info = check_sleep(graph, z, words, PC.STATIC)[3]
        return info

    for t in twins:
        t.pair_islands(True, PC.STATIC)
        t.pair_sleep(True, SC.TOL, SC.TOL, 2, 4096)
    first = phase(8)
    assert first["asleep"] >= 20 and first["epoch"] == 8
    for t in twins:
        t.pair_sleep(True, 0.5, SC.TOL, 2, 4096)             # behind a capture: another lin_tol reaches the next run, the memory stays
        assert t.pair_sleep_params()[1] == 0.5
    z.lin_tol = 0.5
    second = phase(3)
    assert second["epoch"] == 11 and not second["flags"] & Z.RESYNC and second["asleep"] > first["asleep"]
    for t in twins:
        t.pair_sleep(True, 0.5, SC.TOL, 200, 4096)           # another rest_runs: everybody has rested for fewer runs than that
    z.rest_runs = 200
    third = phase(2)
    assert third["asleep"] == 0 and third["epoch"] == 13
    for t in twins:
        t.pair_sleep(True, 0.5, SC.TOL, 2, 4096)
    z.rest_runs = 2
    fourth = phase(2)
    states = graph.read_pair_sleep()[0]
    sleepers = np.flatnonzero(states & Z.ASLEEP)[:5].astype(np.uint32)
    assert fourth["asleep"] == second["asleep"] and len(sleepers) == 5
    for t in twins:
        t.wake_entities(sleepers)                            # outside the captured graph, which replays across it
    z.wake(sleepers)
    fifth = phase(1)
    assert fifth["woke"] >= 5 and np.isin(sleepers, graph.read_pair_sleep()[2]).all()
    phase(2)
    for t in twins:
        t.pair_sleep(False)
        assert not t.pair_sleep_enabled
    phase(2, on=False)
    for t in twins:
        t.pair_sleep(True, SC.TOL, SC.TOL, 2, 4096)
    z = Z.Witness(lin_tol=SC.TOL, ang_tol=SC.TOL, rest_runs=2, max_events=4096)
    last = None
    for k in range(3):
        last = phase(1)
        assert bool(last["flags"] & Z.RESYNC) == (k == 0) and last["epoch"] == k + 1
    assert last["asleep"] >= 20
    for t in twins:
        t.close()


# ---- 3. the pass leaves the rest alone ---------------------------------------------------------------------------------------------
def test_every_other_output_is_that_of_a_twin_that_never_enables_sleep(oracle):
    w, col = G.forest()
    on, never = start(w, col), start(w, col)
    for t in (on, never):
        t.set_pair_contacts(True)
        t.set_pair_manifolds(True)
        t.pair_islands(True, 0)
        t.pair_persistence(True)
        t.set_pair_events(1 << 14, 1 << 14)
        t.set_touch_events(1 << 14, 1 << 14)
    on.pair_sleep(True, SC.TOL, SC.TOL, 2, 4096)
    assert on.pair_sleep_enabled and not never.pair_sleep_enabled
    z = Z.Witness(lin_tol=SC.TOL, ang_tol=SC.TOL, rest_runs=2, max_events=4096)
    rng = np.random.default_rng(4191)
    flags = SHAPES | capi.PAIR_EVENTS | capi.TOUCH_EVENTS
    roots = np.flatnonzero(w.parent < 0)
    moving = roots[::2]
    pos = w.pos.copy()
    for tick in range(4):
        if tick < 3:
            pos[moving] += rng.uniform(-0.5, 0.5, (len(moving), 3)).astype(F)
        outs = []
        for t in (on, never):
            t.upload_positions(0, pos)
            t.run(flags)
            lst, sinfo = t.read_pair_shapes()
            crec, cinfo = t.read_pair_contacts()
            mrec, minfo = t.read_pair_manifolds()
            labels, edge, iinfo = t.read_pair_islands()
            prec, pinfo = t.read_pair_persistence()
            tb, te, ti = t.touch_events()
            pb, pe, pi = t.pair_events()
            order = np.argsort(R.keys(lst), kind="stable")
            outs.append((R.keys(lst)[order], sinfo, K.bits(crec)[order], cinfo, M.bits(mrec)[order], minfo, labels, edge[order], iinfo,
                         prec["age"][order], prec["prev_slot"][order], pinfo, np.sort(R.keys(tb)), np.sort(R.keys(te)), ti,
                         np.sort(R.keys(pb)), np.sort(R.keys(pe)), pi))
        for x, y in zip(*outs):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y
        info = check_sleep(on, z, words_of(w), 0)[3]
        with pytest.raises(capi.ScTickError, match="pair sleep was not enabled"):
            never.read_pair_sleep()
    assert info["asleep"] >= 1 and info["awake_entries"] >= 1
    for t in (on, never):
        t.close()


# ---- 4. two in-order tiles on one GPU ----------------------------------------------------------------------------------------------
def test_a_neighbours_member_counts_as_still_and_the_ids_carry_the_rank(oracle):
    """the world of tests/test_gpu_pair_islands.py: spheres A and C of tile 0 touch; sphere B of tile 1 lies on the shared edge, its AABB
    meets A's, and it touches D of tile 1.  B moves in every run: B and D never sleep on tile 1; on tile 0 the entry A - B is anchored on
    a neighbour's member, which counts as still -- A and C fall asleep all the same."""
    from sc_gameengine_amd import tiles
    from tests.test_gpu_tiles import split_world
    from tests.test_gpu_tiles_edge import network
    grid, S = (2, 1), (6, 6)
    w = sw.generate(S[0] * grid[0], S[1], 15, tiles=grid)
    w.group[:], w.mask[:] = sw.GROUP_DYNAMIC, sw.MASK_ALL
    n = w.n // 2
    edge = 64.0 * S[0]
    props = (w.parent < 0) & (np.arange(w.n) % 16 != 0)
    lone = props & ~np.isin(np.arange(w.n), w.parent[w.parent >= 0])
    b, d = (int(x) for x in np.flatnonzero(lone & (np.arange(w.n) >= n))[:2])
    a, c = (int(x) for x in np.flatnonzero(lone & (np.arange(w.n) < n))[:2])
    w.pos[a] = [edge - 0.6, 200.0, 100.0]
    w.pos[c] = [edge - 1.4, 200.0, 100.0]
    w.pos[b] = [edge + 0.3, 200.0, 100.6]
    w.pos[d] = [edge + 1.1, 200.0, 100.6]
    col = cr.Colliders(w.n)
    for e in (a, b, c, d):
        w.scale[e] = 1.0; w.rot[e] = 0.0
        col.type[e] = cr.SPHERE; col.radius[e] = 0.5
    parts, n = split_world(w, grid, S)
    ticks = [WorldTick.from_world(p, broadphase=True, max_pairs=1 << 16) for p in parts]
    for r, t in enumerate(ticks):
        part = cr.Colliders(n)
        for x, y in ((part.type, col.type), (part.he, col.he), (part.radius, col.radius), (part.hh, col.hh)):
            x[:] = y[r * n:(r + 1) * n]
        part.upload(t)
        t.set_pair_shapes(BIG)
        t.pair_islands(True, 0)
        t.pair_sleep(True, SC.TOL, SC.TOL, 2, 4096)
    bufs = [tiles.BorderBuffers(t, r, grid, "cuda") for r, t in enumerate(ticks)]
    zs = [Z.Witness(lin_tol=SC.TOL, ang_tol=SC.TOL, rest_runs=2, max_events=4096, rank=r) for r in range(2)]
    out = None
    for step in range(4):
        ticks[1].upload_positions(b - n, (w.pos[b] + F([0.0, 0.0, 0.02 * (step % 2)])).reshape(1, 3))
        for t in ticks:
            t.run(SHAPES | capi.SPLIT_PAIRS)
        network(bufs, grid, parity=step % len(bufs[0].sets))
        for t in ticks:
            t.run_pairs()
        assert all(t.counts().border_lost == 0 for t in ticks)
        out = [check_sleep(t, zs[r], words_of(parts[r]), 0) for r, t in enumerate(ticks)]
        if step == 2:
            fell0, fell1 = out[0][1], out[1][1]
            assert a in fell0.tolist() and c in fell0.tolist() and (fell0 >> 24 == 0).all()
            assert len(fell1) > 0 and (fell1 >> 24 == 1).all() and not np.isin([(1 << 24) | (b - n), (1 << 24) | (d - n)], fell1).any()
    listed0 = ticks[0].read_pair_shapes()[0]
    assert (R.keys(listed0) == R.keys([[a, (1 << 24) | (b - n)]])[0]).any()      # the anchored entry on the neighbour's moving member is listed
    s0, s1 = out[0][0], out[1][0]
    assert s0[a] & Z.ASLEEP and s0[c] & Z.ASLEEP and not s1[b - n] & Z.ASLEEP and not s1[d - n] & Z.ASLEEP
    with pytest.raises(capi.ScTickError, match="an id of another rank"):
        ticks[0].wake_entities([(1 << 24) | (b - n)])
    ticks[1].wake_entities([(1 << 24) | 0])
    for t in ticks:
        t.close()


# ---- 5. resyncs --------------------------------------------------------------------------------------------------------------------
def test_removals_a_shrunk_count_a_resized_list_and_a_rename_between_the_halves_resync(oracle):
    """(a removal between the halves of a tick that lists the touching pairs is refused by the library, so the rename between the halves
    is the one such a tick admits: scTickSetTile to another rank)"""
    case = SC.random_world(4144)
    w, col = case.w, case.col
    rest = case.steps[-1]                                   # everything where it was left: all at rest
    t = start(w, col, capacity=w.n)
    t.pair_islands(True, PC.STATIC)
    t.pair_sleep(True, SC.TOL, SC.TOL, 2, 4096)
    z = Z.Witness(lin_tol=SC.TOL, ang_tol=SC.TOL, rest_runs=2, max_events=4096)
    words, n_now = case.words(), [w.n]

    def runs(k, split=False, between=None):
        info = None
        for _ in range(k):
            t.upload_locals(0, rest.pos[:n_now[0]], w.rot[:n_now[0]], rest.scale[:n_now[0]])
            if split:
                t.run(SHAPES | capi.SPLIT_PAIRS)
                if between:
                    between()
                t.run_pairs()
            else:
                t.run(SHAPES)
            info = check_sleep(t, z, words, PC.STATIC)[3]
        return info

    first = runs(1)
    assert first["flags"] & Z.RESYNC and first["asleep"] == 0 and first["fell_asleep"] == 0 and first["epoch"] == 1
    settled = runs(2)
    assert settled["asleep"] == settled["fell_asleep"] > 300 and not settled["flags"] & Z.RESYNC
    # removals rename dense indices: nothing is remembered
    gone = np.random.default_rng(4145).choice(np.arange(100, 500), 60, replace=False).astype(np.uint32)
    src, dst = t.remove_entities(gone)
    n1 = w.n - len(gone)
    words = words[:n1].copy(); words[dst] = case.words()[src]
    moved = SC.Step(rest.pos[:n1].copy(), rest.scale[:n1].copy())
    moved.pos[dst], moved.scale[dst] = rest.pos[src], rest.scale[src]
    rot = w.rot[:n1].copy(); rot[dst] = w.rot[src]
    rest, w.rot, n_now[0] = moved, rot, n1
    z.resync()
    info = runs(1)
    assert info["flags"] & Z.RESYNC and info["asleep"] == 0 and info["woke"] == 0 and info["epoch"] == 1
    assert runs(2)["asleep"] > 250
    # a shrunk count
    n_now[0] = n1 - 100
    t.set_count(n_now[0])
    words = words[:n_now[0]]
    z.resync()
    info = runs(1)
    assert info["flags"] & Z.RESYNC and info["asleep"] == 0 and info["woke"] == 0
    assert runs(2)["asleep"] > 200
    # a same-size scTickSetPairShapes keeps the memory, another size forgets it
    t.set_pair_shapes(BIG)
    assert t.pair_sleep_enabled and not runs(1)["flags"] & Z.RESYNC
    t.set_pair_shapes(BIG // 2)
    assert t.pair_sleep_enabled and t.pair_sleep_params() == (True, float(SC.TOL), float(SC.TOL), 2, 4096)
    z.resync()
    assert runs(1)["flags"] & Z.RESYNC
    assert runs(2)["asleep"] > 200
    # the caller-owned split flow, without and with a rename between its halves
    assert not runs(1, split=True)["flags"] & Z.RESYNC

    def remove_some():
        with pytest.raises(capi.ScTickError, match="scTickRunPairs is pending"):
            t.pair_sleep(True, SC.TOL, SC.TOL, 3, 4096)
        with pytest.raises(capi.ScTickError, match="scTickRunPairs is pending"):
            t.wake_entities([0])
        with pytest.raises(capi.ScTickError, match="pair sleep is ready after scTickRunPairs"):
            t.read_pair_sleep()
        with pytest.raises(capi.ScTickError, match="scTickRemoveEntities is refused between"):
            t.remove_entities(np.arange(10, 20, dtype=np.uint32))
        t.set_tile(3, 0)

    # (the pair half of that tick still runs in the ids from before the rename: only its resync is checked, behind the next whole tick)
    assert runs(1)["asleep"] > 200
    t.upload_locals(0, rest.pos[:n_now[0]], w.rot[:n_now[0]], rest.scale[:n_now[0]])
    t.run(SHAPES | capi.SPLIT_PAIRS)
    remove_some()
    t.run_pairs()
    z = Z.Witness(lin_tol=SC.TOL, ang_tol=SC.TOL, rest_runs=2, max_events=4096, rank=3)
    info = runs(1)                                          # forgotten again behind the pair half: this run starts from nothing
    assert info["flags"] & Z.RESYNC and info["epoch"] == 1 and info["asleep"] == 0 and info["woke"] == 0
    runs(2)
    states, fell, woke, info = t.read_pair_sleep()
    assert info["asleep"] > 200 and len(fell) > 200 and (fell >> 24 == 3).all()
    t.close()


# ---- 6. every refusal, short reads, NULL with capacity 0 ----------------------------------------------------------------------------
def test_pair_sleep_api_errors_and_short_reads(oracle):
    case = SC.singles(129)
    w, col = case.w, case.col
    t = start(w, col)
    with pytest.raises(capi.ScTickError, match="needs scTickSetPairIslands\\(1\\) first"):
        t.pair_sleep(True)
    with pytest.raises(capi.ScTickError, match="needs scTickSetPairSleep\\(1\\) first"):
        t.wake_entities([0])
    t.pair_sleep(False)                                     # nothing to free: welcome
    assert not t.pair_sleep_enabled and t.pair_sleep_params() == (False, 0.0, 0.0, 0, 0)
    t.pair_islands(True, PC.STATIC)
    for args, msg in (((np.nan, 0.1, 3, 16), "finite and >= 0"), ((0.1, np.inf, 3, 16), "finite and >= 0"), ((-0.1, 0.1, 3, 16), "finite and >= 0"),
                      ((0.1, -1e-9, 3, 16), "finite and >= 0"), ((0.1, 0.1, 0, 16), "rest_runs must be in 1 .. 255"), ((0.1, 0.1, 256, 16), "rest_runs must be in 1 .. 255"),
                      ((0.1, 0.1, 3, 0), "max_events must be > 0")):
        with pytest.raises(capi.ScTickError, match=msg):
            t.pair_sleep(True, *args)
        assert not t.pair_sleep_enabled
    t.run(SHAPES)                                           # the refusals changed nothing: the context still runs
    t.pair_sleep(True)                                      # Python's defaults: Bullet's 2 s at 60 Hz
    assert t.pair_sleep_params() == (True, float(F(0.005)), float(F(0.005)), 120, 4096)
    with pytest.raises(capi.ScTickError, match="pair sleep was not enabled"):      # enabled since: the last run kept no rest state
        t.read_pair_sleep()
    with pytest.raises(capi.ScTickError, match="rest_runs must be in 1 .. 255"):   # a refusal leaves the enabled state as it was
        t.pair_sleep(True, 0.1, 0.1, 1000, 16)
    assert t.pair_sleep_params() == (True, float(F(0.005)), float(F(0.005)), 120, 4096)
    t.pair_sleep(True, SC.TOL, SC.TOL, 1, 4096)
    t.run(FLAGS)
    with pytest.raises(capi.ScTickError, match="did not request SC_TICK_PAIR_SHAPES"):
        t.read_pair_sleep()
    z = Z.Witness(lin_tol=SC.TOL, ang_tol=SC.TOL, rest_runs=1, max_events=4096)
    for _ in range(2):
        t.run(SHAPES)
        states, fell, woke, info = check_sleep(t, z, case.words(), PC.STATIC)
    assert info["fell_asleep"] == len(fell) == 129 and info["asleep"] == 129
    for bad, msg in (([129], "at or above the entity count"), ([5, 1 << 24], "an id of another rank"), ([0, 1, 0xFFFFFF], "at or above the entity count")):
        with pytest.raises(capi.ScTickError, match=msg):
            t.wake_entities(bad)
    assert t.lib.scTickWakeEntities(t.ctx, None, 3) == 0 and b"null argument" in t.lib.scTickGetLastError(t.ctx)
    assert t.lib.scTickWakeEntities(t.ctx, None, 0) == 1
    info_c = capi.PairSleepInfo()
    assert t.lib.scTickReadPairSleep(t.ctx, None, 0, None, 0, None, 0, None) == 0 and b"null argument" in t.lib.scTickGetLastError(t.ctx)
    assert t.lib.scTickGetPairSleep(t.ctx, None, None, None, None, None) == 0 and b"null argument" in t.lib.scTickGetLastError(t.ctx)
    assert t.lib.scTickReadPairSleep(t.ctx, None, 0, None, 0, None, 0, C.byref(info_c)) == 1 and info_c.fell_asleep == 129      # the report alone
    st, fl, wk = (np.full(160, SENTINEL, np.uint32) for _ in range(3))      # less room: the buffers beyond keep their sentinel
    assert t.lib.scTickReadPairSleep(t.ctx, st.ctypes.data_as(U32P), 100, fl.ctypes.data_as(U32P), 50, wk.ctypes.data_as(U32P), 7, C.byref(info_c)) == 1
    assert np.array_equal(st[:100], states[:100]) and (st[100:] == SENTINEL).all()
    assert np.array_equal(fl[:50], fell[:50]) and (fl[50:] == SENTINEL).all() and (wk == SENTINEL).all()
    # the refused wakes changed nothing: the next run has no events
    t.run(SHAPES)
    assert check_sleep(t, z, case.words(), PC.STATIC)[3]["woke"] == 0
    t.pair_sleep(False)
    with pytest.raises(capi.ScTickError, match="pair sleep was switched off since the last scTickRun"):
        t.read_pair_sleep()
    t.pair_sleep(True, SC.TOL, SC.TOL, 1, 4096)
    t.pair_islands(False)                                   # switching the islands off switches sleep off too
    assert not t.pair_sleep_enabled
    t.pair_islands(True, PC.STATIC)
    t.pair_sleep(True, SC.TOL, SC.TOL, 1, 4096)
    t.set_pair_shapes(0)                                    # ... and so does switching the touching pairs off
    assert not t.pair_sleep_enabled and not t.pair_islands_enabled()
    with pytest.raises(capi.ScTickError, match="needs scTickSetPairIslands"):
        t.pair_sleep(True)
    t.run(FLAGS)
    t.close()
