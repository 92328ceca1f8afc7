"""The witness of the touch events (include/sc_tick.h "touch events") and the scripted worlds its tests run.

The touching set of a tick is `pair_shapes_ref.touching32` over the ORACLE's pair set of the tick (`pair_shapes_cases.oracle_pairs`: the
witness boxes of the colliders through the oracle's matrices), duplicates dropped; the events are `pair_events_ref.Witness` over those
sets.  Nothing here is restated: the three are imported.  No GPU, no library call in this file.

A script is (world, colliders, one entry per tick): the positions to set before that tick (None = a still tick), as in
tests/pair_events_ref.py.  tests/test_touch_events_cpu.py checks that every script gives its GPU test what it counts on."""
import numpy as np

from tests import collider_ref as cr, pair_events_ref as E, pair_shapes_cases as G, pair_shapes_ref as R, worlds

F = np.float32
Witness = E.Witness
keys, sorted_pairs, EMPTY = E.keys, E.sorted_pairs, E.EMPTY


def touching_of(pairs, m, col, n=None, rank=0):
    """the touching set of a pair list: the pairs touching32 does not prove apart, each once, sorted by key"""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    touching, _ = R.touching32(m, col, pairs, n=n, rank=rank)
    return E.unkeys(np.unique(E.keys(pairs[touching])))


def tick_sets(oracle, w, col, steps):
    """per tick of a script: (AABB pair set, touching set, world matrices), from the oracle and the witnesses alone"""
    ow = worlds.oracle_world(oracle, w, camera=False)
    out = []
    for pos in steps:
        if pos is not None:
            E.set_positions(ow, None, pos)
        ow.transform_system()
        m = ow.world_matrices()[:w.n].copy()
        if col is None:
            pairs = np.ascontiguousarray(E.oracle_pairs(oracle, ow, w), np.uint32).reshape(-1, 2)
        else:
            mn, mx = col.witness(ow, w.n)
            pairs = np.ascontiguousarray(oracle.broadphase_bruteforce(mn, mx, w.group, w.mask), np.uint32).reshape(-1, 2)
        out.append((E.sorted_pairs(pairs), touching_of(pairs, m, col), m))
    ow.close()
    return out


_SETS = {}


def script_sets(oracle, name):
    """(world, colliders, steps, [(pairs, touching, matrices) per tick]) of a named script; computed once per session -- read-only"""
    if name not in _SETS:
        w, col, steps = SCRIPTS[name]()
        _SETS[name] = (w, col, steps, tick_sets(oracle, w, col, steps))
    return _SETS[name]


def events_of(sets, max_tracked=1 << 30, max_events=1 << 30):
    wt = Witness(max_tracked, max_events)
    return [wt.tick(s) for s in sets]


# ---- the scripted world: four couples, every type pair, eight ticks ---------------------------------------------------------------
# Couple k is the entities (2k, 2k + 1), its first member at COUPLE_ORIGIN[k]; only the second member moves.  Every couple is an AABB
# pair on all eight ticks.
#   A (0, 1)  a sphere (r 0.5) slides along x past the corner edge y = z = 1 of a 2 m cube, at y = z = 1.3: its centre is
#             sqrt(0.18 + max(0, |x| - 1)^2) from the cube -- below 0.5 for |x| < 1.2646
#   B (2, 3)  a capsule (r 0.3) crosses the cube's edge x = y = 1 at right angles, its middle nearest: the gap is SCRIPT_GAP_B[tick]
#   C (4, 5)  two 2 m x 4.4 m vehicles yawed by 45 degrees pass in lanes 3 m apart: a metre of air on every tick
#   D (6, 7)  parallel capsules (r 0.4 and 0.5) set off at right angles to their axes: the gap is SCRIPT_GAP_D[tick]
COUPLE_ORIGIN = np.array([[-30.0, 0.0, 0.0], [-10.0, 0.0, 0.0], [10.0, 0.0, 0.0], [30.0, 0.0, 0.0]])
SCRIPT_X_A = (1.45, 1.30, 1.20, 0.5, -0.5, -1.20, -1.30, -1.45)
SCRIPT_GAP_B = (0.5, 0.2, 0.05, -0.05, -0.3, -0.05, 0.05, 0.5)
SCRIPT_S_C = (-2.1, -1.5, -0.9, -0.3, 0.3, 0.9, 1.5, 2.1)
SCRIPT_GAP_D = (-0.3, -0.1, 0.1, 0.3, 0.1, -0.1, -0.3, -0.3)
A, B, C, D = (0, 1), (2, 3), (4, 5), (6, 7)
# derived by hand from the four lines above.  touching: A on ticks 2-5, B on 3-5, C never, D on 0-1 and 5-7
SCRIPT_TOUCHING = [[D], [D], [A], [A, B], [A, B], [A, B, D], [D], [D]]
SCRIPT_EVENTS = [([D], []), ([], []), ([A], [D]), ([B], []), ([], []), ([D], []), ([], [A, B]), ([], [])]      # (begun, ended); tick 0 is the resync
SCRIPT_PAIRS = [A, B, C, D]


def scripted_world():
    S2, Q = G.S2, G.Q
    n = 8
    rot = np.zeros((n, 3))
    col = cr.Colliders(n)
    col.type[:] = [cr.BOX, cr.SPHERE, cr.BOX, cr.CAPSULE, cr.BOX, cr.BOX, cr.CAPSULE, cr.CAPSULE]
    col.he[0] = col.he[2] = 1.0
    col.radius[1] = 0.5
    rot[3] = (0, 0, Q); col.radius[3], col.hh[3] = 0.3, 1.5
    rot[4] = rot[5] = (0, Q, 0); col.he[4] = col.he[5] = (1.0, 0.75, 2.2)
    rot[6] = rot[7] = (0, 0, Q); col.radius[6], col.radius[7], col.hh[6], col.hh[7] = 0.4, 0.5, 1.0, 1.0
    steps = []
    for k in range(8):
        pos = np.zeros((n, 3))
        pos[0::2] = COUPLE_ORIGIN
        pos[1] = COUPLE_ORIGIN[0] + [SCRIPT_X_A[k], 1.3, 1.3]
        c = 1.0 + (0.3 + SCRIPT_GAP_B[k]) * S2
        pos[3] = COUPLE_ORIGIN[1] + [c, c, 0.0]
        lateral, heading = np.array([S2, 0.0, -S2]), np.array([S2, 0.0, S2])      # columns 0 and 2 of the yaw
        pos[5] = COUPLE_ORIGIN[2] + 3.0 * lateral + SCRIPT_S_C[k] * heading
        s = (0.4 + 0.5 + SCRIPT_GAP_D[k]) * S2
        pos[7] = COUPLE_ORIGIN[3] + [s, s, 0.0]
        steps.append(pos.astype(F))
    w = G.flat_world(steps[0], rot, np.ones((n, 3)))
    return w, col, [None] + steps[1:]


# ---- random motion: an agreement world whose roots each go their own way ----------------------------------------------------------
NUDGE = 0.5               # metres per axis and tick, at most


def nudged_run(seed, n, ticks, move_seed):
    """pair_shapes_cases.agreement_world(seed, n); before every tick but the first every entity is displaced by up to +-NUDGE per axis"""
    w, col = G.agreement_world(seed, n)
    rng = np.random.default_rng(move_seed)
    pos, steps = w.pos.copy(), [None]
    for _ in range(ticks - 1):
        pos = (pos + rng.uniform(-NUDGE, NUDGE, pos.shape).astype(F)).astype(F)
        steps.append(pos)
    return w, col, steps


# tests/test_touch_events_cpu.py: the worlds of pair_shapes_cases.AGREEMENT_SEEDS, each moved with the seed AGREEMENT_MOVE + its own.  An
# event needs a gap that changes sign between two ticks, with steps of up to NUDGE: about one in two hundred has a gap within a millimetre
# of zero on one of the two ticks, which is that test's cap -- the move seeds were chosen with the two witnesses alone to stay under it
# (3, 4 and 4 of some 940 events each; + 1000 gives 5, 1 and 8, + 2000 gives 6, 6 and 6).
AGREEMENT_TICKS, AGREEMENT_MOVE = 4, 3000
RANDOM_N, RANDOM_SEED, RANDOM_MOVE_SEED, RANDOM_TICKS = 600, 471, 472, 10      # (the graph test runs all ten ticks, the others the first few)


# ---- pair lists of awkward lengths: a resync tick, then half the couples moved apart ------------------------------------------------
def couples_run(k):
    """pair_shapes_cases.couples_world(k): k AABB pairs, every second couple's shapes apart.  The second tick moves half of the touching
    couples -- those with an index divisible by four -- apart: the second member goes from (0.4, 0.3, 0.2) to (0.7, 0.7, 0.7) off the first,
    1.21 m between centres with radii 0.5 + 0.5, the AABBs still overlapping (a couple with a box in it may go on touching: the witness
    decides)"""
    w, col, apart = G.couples_world(k, G.WALK_SEED + k)
    pos = w.pos.copy()
    if k:
        moved = np.repeat(np.arange(k) % 4 == 0, 2) & (np.arange(2 * k) % 2 == 1)
        pos[moved] += F([0.3, 0.4, 0.5])
    return w, col, [None, pos]


# ---- colliders that change between ticks --------------------------------------------------------------------------------------------
def collider_change_world():
    """(world, colliders, colliders after the upload).  Couples 0-2: spheres of radius 0.5 with centres 0.8 m apart -- touching.  Couple 3: a
    sphere of radius 0.5 and a 0.6 m cube at (0.68, 0.68, 0) from it: the AABBs overlap, the cube's nearest edge is 0.537 m from the
    centre -- apart.  The upload shrinks the radius of entity 1 to 0.2 (couple 0 ends: 0.7 < 0.8) and makes the cube a sphere of radius 0.5
    (couple 3 begins: centres 0.962 m apart); couples 1 and 2 stay as they are."""
    n = 8
    pos = np.zeros((n, 3))
    pos[:, 0] = np.repeat(np.arange(4) * 20.0 - 30.0, 2)
    pos[1:6:2, 0] += 0.8
    pos[7] += [0.68, 0.68, 0.0]
    w = G.flat_world(pos, np.zeros((n, 3)), np.ones((n, 3)))
    col = cr.Colliders(n)
    col.type[:] = cr.SPHERE
    col.type[7] = cr.BOX; col.he[7] = 0.3
    after = cr.Colliders(n)
    after.type[:], after.he[:], after.radius[:], after.hh[:] = col.type, col.he, col.radius, col.hh
    after.radius[1] = 0.2
    after.type[7] = cr.SPHERE
    return w, col, after


COLLIDER_CHANGE_EVENTS = ([(6, 7)], [(0, 1)])           # (begun, ended) of the tick after the upload


SCRIPTS = {
    "scripted": scripted_world,
    "random": lambda: nudged_run(RANDOM_SEED, RANDOM_N, RANDOM_TICKS, RANDOM_MOVE_SEED),
    "forest": lambda: G.forest() + ([None, None],),
    **{f"couples{k}": (lambda k=k: couples_run(k)) for k in G.WALK_LENGTHS},
}
