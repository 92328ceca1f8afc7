"""Worlds of the pair-persistence tests, shared by the GPU suite (tests/test_gpu_pair_persist.py) and its CPU twin
(tests/test_pair_persist_cpu.py), built on tests/pair_manifolds_cases.py.  Inputs only: no GPU.

    slide_world(seed)    resting_world(seed) and its second tick: every `b` moved in x and z by up to 4 cm in a random direction -- points
                         that stay within the match distance, points that leave it, entries with both, points that change their slot
    carry_world(seed)    the same world and a second tick that moves every entity by one vector: every point keeps its slot
    constructed()        manifold_world() and the per-case motions of its third tick, the turned slab among them

Rotations are the engine's R = Rz * Ry * Rx (angles about x, y, z)."""
import numpy as np

from tests import pair_manifolds_cases as MC

F = np.float32
MATCH_DIST = 0.02                                             # Bullet's contact breaking threshold: WorldTick.pair_persistence's default
SEEDS = (2601, 2602, 2603)
UNITS = 200
FLOORS = dict(kept_points=600, new_points=300, mixed_entries=40, moved_slot_entries=4)      # sums over the three seeds
CARRY = (3.0, 0.25, -1.5)


def slide_world(seed):
    """(world, colliders, pos2): pos2 is the second tick's positions"""
    w, col, _ = MC.resting_world(seed)
    assert w.n == 2 * UNITS
    rng = np.random.default_rng(seed + 7000)
    ang = rng.uniform(0, 2 * np.pi, UNITS)
    ln = rng.uniform(0, 0.04, UNITS)
    pos2 = w.pos.copy()
    pos2[1::2, 0] += (ln * np.cos(ang)).astype(F)
    pos2[1::2, 2] += (ln * np.sin(ang)).astype(F)
    return w, col, pos2


def carry_world(seed):
    w, col, _ = MC.resting_world(seed)
    return w, col, (w.pos + F(CARRY)).astype(F)


def unit_pairs(n):
    k = np.arange(n // 2)
    return np.stack([2 * k, 2 * k + 1], axis=1).astype(np.uint32)


# ---- the constructed sequence ----------------------------------------------------------------------------------------------------
TURNED, SLID_A_CENTIMETRE, SLID_FIVE, CARRIED, LIFTED = "turned", "slid 1 cm", "slid 5 cm", "carried", "lifted"
MOTIONS = {
    "cube flat on a larger slab": TURNED,                      # the slab yaws 90 degrees and takes the cube round: all four kept, in a's frame alone
    "cube overhanging a slab edge": SLID_A_CENTIMETRE,         # b moves 1 cm along x: within the match distance, kept
    "capsule lying on a box face": SLID_FIVE,                  # b moves 5 cm along x: both ends are new points of a kept pair
    "sphere pair": CARRIED,                                    # both move by one vector: kept
    "cube on an equal face, yawed 45 degrees": LIFTED,         # b leaves: the pair is not listed
}


def constructed():
    """(world, colliders, cases, pos3, rot3): tick 3 of the constructed sequence (ticks 1 and 2 are the world as it is)"""
    w, col, cases, _ = MC.manifold_world()
    pos3, rot3 = w.pos.astype(np.float64), w.rot.astype(np.float64)
    for i, case in enumerate(cases):
        a, b = 2 * i, 2 * i + 1
        how = MOTIONS.get(case[0])
        if how == TURNED:
            rel = pos3[b] - pos3[a]
            pos3[b] = pos3[a] + [rel[2], rel[1], -rel[0]]      # Ry(90 degrees): x' = z, z' = -x
            rot3[a, 1] += np.pi / 2
            rot3[b, 1] += np.pi / 2
        elif how == SLID_A_CENTIMETRE:
            pos3[b, 0] += 0.01
        elif how == SLID_FIVE:
            pos3[b, 0] += 0.05
        elif how == CARRIED:
            pos3[a] += CARRY
            pos3[b] += CARRY
        elif how == LIFTED:
            pos3[b, 1] += 1.0
    return w, col, cases, pos3.astype(F), rot3.astype(F)
