"""The case table of the pair-sleep tests, shared by the GPU suite (tests/test_gpu_pair_sleep.py) and its CPU twin
(tests/test_pair_sleep_cpu.py, which asserts without a GPU that every case is what it claims).  Tiny worlds of spheres and boxes as
tests/pair_islands_cases.py builds them, driven run by run through their locals: a case is a list of steps, a step the positions and
scales of one flagged run (rotations are zero, so element 0 of an entity's matrix is its x scale and the translation is its position,
exactly), optionally a patch of matrix elements (uploaded as world matrices, the run then goes without the transform stage), a `hold`
(no upload at all, no transform stage: the patched matrices stay) or ids to wake ahead of the run.  Inputs and the oracle-derived
reference only: no GPU."""
import numpy as np

from tests import pair_islands_cases as PC, pair_islands_ref as I, pair_shapes_cases as G, pair_shapes_ref as R, pair_sleep_ref as Z

F = np.float32
TOL = F(2.0 ** -7)                # lin_tol and ang_tol of the table: a power of two, so that steps of TOL are exact in fp32
REST_RUNS = 3
STATIC = PC.STATIC


class Step:
    def __init__(self, pos, scale=None, patch=None, hold=False, wake=None):
        self.pos = np.ascontiguousarray(pos, F)
        self.scale = np.ones_like(self.pos) if scale is None else np.ascontiguousarray(scale, F)
        self.patch, self.hold, self.wake = patch, hold, wake


class Case:
    """fell / woke: {run: true event count}, every other run has none; rest: {run: the rest counts of every entity};
    never_asleep: entities that are asleep in no run"""

    def __init__(self, name, w, col, steps, fixed_groups=STATIC, lin_tol=TOL, ang_tol=TOL, rest_runs=REST_RUNS, max_events=4096, fell=None, woke=None,
                 rest=None, never_asleep=()):
        self.name, self.w, self.col, self.steps, self.fixed_groups = name, w, col, steps, fixed_groups
        self.lin_tol, self.ang_tol, self.rest_runs, self.max_events = float(lin_tol), float(ang_tol), rest_runs, max_events
        self.fell, self.woke, self.rest, self.never_asleep = fell or {}, woke or {}, rest or {}, never_asleep

    def params(self):
        return dict(lin_tol=self.lin_tol, ang_tol=self.ang_tol, rest_runs=self.rest_runs, max_events=self.max_events)

    def words(self):
        return (self.w.group & 0xFFFF) | ((self.w.mask & 0xFFFF) << 16)

    def __repr__(self):
        return self.name


def _steps(base, runs, moves=None, **kw):
    """`runs` steps of the positions `base`; moves: {run: {entity: offset}} added to that run's positions alone"""
    out = []
    for k in range(runs):
        pos = np.array(base, np.float64)
        for e, off in (moves or {}).get(k, {}).items():
            pos[e] += off
        out.append(Step(pos.astype(F), **kw))
    return out


def _jiggle(e, runs):
    """entity e two tolerances off in x in every second of the runs, back in place in the last of them: from the second of the runs on it
    is away from its anchor in each, and the last of the runs is the last in which it moved"""
    runs = list(runs)
    return {k: ({e: [2.0 * float(TOL), 0.0, 0.0]} if (len(runs) - 1 - j) % 2 == 1 else {}) for j, k in enumerate(runs)}


def _grid(n, pitch=16.0):
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    return np.stack([(k % side - side // 2) * pitch, np.zeros(n), (k // side - side // 2) * pitch], axis=1)


COUNTS = (1, 63, 64, 65, 129)


def singles(n, max_events=4096):
    """n spheres far from each other: islands of one.  All fall asleep in run 3, every second one moves a metre in run 4 and wakes"""
    base = _grid(n)
    steps = _steps(base, 5, {4: {e: [1.0, 0.0, 0.0] for e in range(0, n, 2)}})
    name = f"{n} islands of one" if max_events == 4096 else f"65 events into a list of {max_events}"
    return Case(name, PC._world(base), PC._spheres(n, 1.0), steps, max_events=max_events, fell={3: n}, woke={4: (n + 1) // 2})


def chain():
    """a serpentine chain of 65 spheres, ids shuffled, and a mover that waits 100 m away.  The chain's end member jiggles in runs 1 .. 4
    (nobody of the chain sleeps, the mover does in run 3), then stops: all 65 fall asleep in run 7.  In run 9 the mover arrives on top of
    the end member: all 66 wake; they fall asleep again in run 12."""
    n = 65
    order = np.random.default_rng(4165).permutation(n)
    pos = PC._permuted(PC.serpentine(n), order)
    end = int(order[n - 1])
    away, on_top = [0.0, 0.0, 100.0], pos[end] + [0.0, PC.STEP, 0.0]
    base = np.concatenate([pos, [away]])
    moves = _jiggle(end, range(1, 5))
    for k in range(9, 13):
        moves[k] = {n: on_top - np.array(away)}
    return Case("chain of 65 and a mover", PC._world(base), PC._spheres(n + 1), _steps(base, 13, moves), fell={3: 1, 7: n, 12: n + 1}, woke={9: n + 1})


def creep():
    """entity 0 creeps 0.4 tolerances a run in x, entity 1 the same on its x scale (element 0 of its matrix): still, still, tripped"""
    base = _grid(2)
    steps = []
    for k in range(7):
        pos, scale = base.copy(), np.ones((2, 3))
        pos[0, 0] += 0.4 * float(TOL) * k
        scale[1, 0] += 0.4 * float(TOL) * k
        steps.append(Step(pos, scale))
    rest = {k: [r, r] for k, r in enumerate([0, 1, 2, 0, 1, 2, 0])}
    return Case("creep of 0.4 tolerances a run", PC._world(base), PC._spheres(2, 1.0), steps, rest=rest, never_asleep=(0, 1))


def edges():
    """run 1 against the anchors of run 0, every difference exact in fp32: a step of exactly the tolerance is still, the next float above
    it is not -- in x from 0, and on the x scale from 1"""
    base = np.array([[0.0, 0.0, -30.0], [0.0, 0.0, -10.0], [0.0, 0.0, 10.0], [0.0, 0.0, 30.0]])
    above = np.nextafter(TOL, F(1.0))
    pos, scale = base.astype(F), np.ones((4, 3), F)
    pos[0, 0], pos[1, 0] = TOL, above
    scale[2, 0], scale[3, 0] = F(1.0) + TOL, np.nextafter(F(1.0) + TOL, F(2.0))
    assert F(scale[3, 0] - F(1.0)) > TOL and F(scale[2, 0] - F(1.0)) == TOL and above > TOL
    return Case("tolerance edges", PC._world(base), PC._spheres(4, 1.0), [Step(base), Step(pos, scale)], rest={0: [0, 0, 0, 0], 1: [1, 0, 1, 0]})


def zero_tolerance():
    """tolerances of 0: only a bit-identical pose is still, -0 against +0 included; the smallest step is not"""
    base = np.array([[16.0, 0.0, -20.0], [0.0, 0.0, 0.0], [16.0, 0.0, 20.0]])
    moved = base.astype(F)
    moved[1, 0] = F(-0.0)
    moved[2, 0] = np.nextafter(F(16.0), F(17.0))
    steps = [Step(base)] + [Step(moved) for _ in range(4)]
    return Case("tolerance 0", PC._world(base), PC._spheres(3, 1.0), steps, lin_tol=0.0, ang_tol=0.0, fell={3: 2, 4: 1},
                rest={1: [1, 1, 0], 4: [4, 4, 3]})


def nan_row():
    """three spheres in a row, touching; from run 2 on element 0 of the middle one's matrix is a NaN.  It is never still and never asleep.
    (A NaN box is no collider: the pair search stops listing its pairs, so the outer two become islands of one and sleep by themselves.)"""
    base = np.array([[-PC.STEP, 0.0, 0.0], [0.0, 0.0, 0.0], [PC.STEP, 0.0, 0.0]])
    steps = [Step(base), Step(base), Step(base, patch=[(1, 0, np.nan)])] + [Step(base, patch=[(1, 0, np.nan)], hold=True) for _ in range(4)]
    return Case("a NaN row", PC._world(base), PC._spheres(3), steps, fell={3: 2}, never_asleep=(1,), rest={6: [6, 0, 6]})


def slab(fixed_groups):
    """tests/pair_islands_cases.slab: a ground slab of group 2 under 8 stacks of 3 boxes.  The top box of the last stack jiggles up to
    run 3, the slab slides 10 cm in run 8 and stays there.  Slab fixed: 7 stacks fall asleep in run 3 and the jiggled one in run 6, each
    by itself; in run 8 the slab has rest 0 and wakes all 24 bodies through their anchored entries; in run 9 it has rest 1 and they are
    asleep again.  Nothing fixed: one island of 25, asleep in run 6, awake in run 8, asleep again in run 11."""
    c = PC.slab(fixed_groups)
    order = np.random.default_rng(3925).permutation(c.w.n)      # (as PC.slab permutes: entity order[k] sits at its k-th position)
    ground, top = int(order[0]), int(order[1 + 3 * 7 + 2])
    assert c.w.group[ground] == STATIC and (np.delete(c.w.group, ground) == 1).all() and c.w.pos[top, 1] > 2.0
    moves = _jiggle(top, range(1, 4))
    for k in range(8, 12):
        moves[k] = {ground: [0.1, 0.0, 0.0]}
    steps = _steps(c.w.pos, 12, moves)
    if fixed_groups:
        return Case("slab under 8 stacks, slab fixed", c.w, c.col, steps, fixed_groups=STATIC, fell={3: 21, 6: 3, 9: 24}, woke={8: 24}, never_asleep=(ground,))
    return Case("slab under 8 stacks, nothing fixed", c.w, c.col, steps, fixed_groups=0, fell={6: 25, 11: 25}, woke={8: 25})


def merge():
    """two chains of 5 and a bridging body 40 m away.  Chain A and the bridge fall asleep in run 3; a member of chain B jiggles in every
    run.  In run 5 the bridge fills the gap: one island of 11, awake -- chain A and the bridge wake."""
    a = np.stack([PC.STEP * np.arange(5), np.zeros(5), np.zeros(5)], axis=1)
    b = a + [6 * PC.STEP, 0.0, 0.0]
    base = np.concatenate([a, b, [[5 * PC.STEP, 0.0, 40.0]]])
    moves = _jiggle(9, range(1, 8))
    for k in range(5, 8):
        moves[k] = dict(moves[k]); moves[k][10] = [0.0, 0.0, -40.0]
    return Case("a sleeping and a waking island merge", PC._world(base), PC._spheres(11), _steps(base, 8, moves), fell={3: 6}, woke={5: 6},
                never_asleep=(5, 6, 7, 8, 9))


def saturation():
    """260 runs of a world of 4 at rest -- a touching couple and two singles: rest stays at 255 and asleep stays"""
    base = np.array([[0.0, 0.0, 0.0], [PC.STEP, 0.0, 0.0], [40.0, 0.0, 0.0], [-40.0, 0.0, 0.0]])
    return Case("saturation over 260 runs", PC._world(base), PC._spheres(4), _steps(base, 260), fell={3: 4}, rest={254: [254] * 4, 255: [255] * 4, 259: [255] * 4})


def wake():
    """a chain of 65 at rest falls asleep in run 3; one member is woken ahead of run 5: all 65 wake in run 5 and fall asleep again in
    run 8"""
    n = 65
    pos = PC._permuted(PC.serpentine(n), np.random.default_rng(4166).permutation(n))
    steps = _steps(pos, 9)
    steps[5].wake = np.array([17], np.uint32)
    return Case("wake one member of a sleeping chain", PC._world(pos), PC._spheres(n), steps, fell={3: n, 8: n}, woke={5: n})


RANDOM_SEEDS = (4141, 4142)


def random_world(seed):
    """tests/pair_islands_cases.random_world(600): a third in group 2.  12 runs; every movable entity moves by up to 5 cm in x and z in
    every run, a random third of them is frozen from run 4 on; a tenth of the fixed ones move in run 8"""
    c = PC.random_world(seed, 600)
    rng = np.random.default_rng(seed + 70)
    movable = np.flatnonzero((c.w.group & STATIC) == 0)
    fixed = np.flatnonzero((c.w.group & STATIC) != 0)
    frozen = rng.choice(movable, len(movable) // 3, replace=False)
    pushed = rng.choice(fixed, len(fixed) // 10, replace=False)
    steps, pos = [], c.w.pos.astype(np.float64)
    for k in range(12):
        step = np.zeros_like(pos)
        step[movable] = np.stack([rng.uniform(-0.05, 0.05, len(movable)), np.zeros(len(movable)), rng.uniform(-0.05, 0.05, len(movable))], axis=1)
        if k >= 4:
            step[frozen] = 0.0
        if k == 8:
            step[pushed, 0] = 0.05
        pos = pos + (step if k else 0.0)
        steps.append(Step(pos.astype(F), c.w.scale))
    return Case(f"random world of 600, seed {seed}", c.w, c.col, steps)


def cases():
    out = [singles(n) for n in COUNTS]
    out += [chain(), creep(), edges(), zero_tolerance(), nan_row(), slab(STATIC), slab(0), merge(), singles(65, max_events=1), singles(65, max_events=64),
            saturation(), wake()]
    out += [random_world(s) for s in RANDOM_SEEDS]
    return out


CASES = cases()
NAMES = [c.name for c in CASES]
_REFERENCE, _SIMULATED = {}, {}


def reference(oracle, case, k):
    """(matrices [n][16], touching set [j][2], labels, edge islands, the islands' report) of run k of a case, from the oracle's matrices
    and pair set and the fp32 witnesses of the touching pairs and the islands -- never from the library.  Computed once per distinct step
    and shared; do not write to it."""
    step = case.steps[k]
    key = (case.name, step.pos.tobytes(), step.scale.tobytes(), repr(step.patch))
    if key not in _REFERENCE:
        w = case.w
        saved = w.pos, w.scale
        w.pos, w.scale = step.pos, step.scale
        try:
            m = G.oracle_matrices(oracle, w)
            pairs = G.oracle_pairs(oracle, m, case.col, w)
        finally:
            w.pos, w.scale = saved
        for e, idx, value in step.patch or ():
            m[e, idx] = value
            pairs = pairs[~(pairs == e).any(axis=1)]       # a NaN box is no collider: the pair search lists none of its pairs
        touching, _ = R.touching32(m, case.col, pairs)
        tset = pairs[touching]
        labels, edge, info = I.islands_union_find(tset, case.words(), w.n, case.fixed_groups)
        for a in (m, tset, labels, edge):
            a.setflags(write=False)
        _REFERENCE[key] = (m, tset, labels, edge, info)
    return _REFERENCE[key]


def simulate(oracle, case, still=Z.still32):
    """[(states, fell, woke, info)] of every run of a case: the witness over reference().  Shared (for the fp32 witness); do not write to it."""
    key = (case.name, still.__name__)
    if key not in _SIMULATED:
        z = Z.Witness(rank=0, still=still, **case.params())
        out = []
        for k, step in enumerate(case.steps):
            if step.wake is not None:
                z.wake(step.wake)
            m, tset, labels, edge, info = reference(oracle, case, k)
            out.append(z.run(m, case.words(), case.fixed_groups, labels, tset, edge, info["list_truncated"]))
        _SIMULATED[key] = out
    return _SIMULATED[key]
