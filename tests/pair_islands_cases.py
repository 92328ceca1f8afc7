"""The case table of the pair-island tests, shared by the GPU suite (tests/test_gpu_pair_islands.py) and its CPU twin
(tests/test_pair_islands_cpu.py, which asserts without a GPU that every case is what it claims).  Worlds as tests/pair_shapes_cases.py
builds them: spheres and boxes on a flat grid of 64 m sectors, dense indices permuted against the spatial order wherever order could
matter.  Inputs and the oracle-derived reference only: no GPU."""
import numpy as np

from tests import collider_ref as cr, pair_islands_ref as I, pair_shapes_cases as G, pair_shapes_ref as R

F = np.float32
STATIC = 2                        # the group the reference puts static bodies on (sc_physics.cpp:372-379)
R_SPHERE, STEP = 4.0, 7.0         # chain links: radius < step < 2 * radius, so a sphere touches the next and not the one after
ROW = 3                           # a serpentine's rows lie three steps apart: at most ~40 boxes in a 64 m sector


class Case:
    def __init__(self, name, w, col, fixed_groups=STATIC, islands=None, sizes=None, anchored=None, max_touching=1 << 16, ticks=None, min_edges=0):
        self.name, self.w, self.col, self.fixed_groups, self.max_touching = name, w, col, fixed_groups, max_touching
        self.islands, self.sizes, self.anchored, self.min_edges = islands, sizes, anchored, min_edges
        self.ticks = ticks if ticks is not None else [w.pos.copy()]      # the positions of every tick of the case
        self.per_tick = None                                             # [(islands, sizes)] per tick where they differ from tick to tick

    def words(self):
        return (self.w.group & 0xFFFF) | ((self.w.mask & 0xFFFF) << 16)

    def __repr__(self):
        return self.name


def _world(pos, n_sectors=4):
    pos = np.asarray(pos, np.float64)
    return G.flat_world(pos, np.zeros_like(pos), np.ones_like(pos), origin=(-n_sectors // 2, -n_sectors // 2), sectors=(n_sectors, n_sectors))


def _spheres(n, radius=R_SPHERE):
    col = cr.Colliders(n)
    col.type[:] = cr.SPHERE
    col.radius[:] = radius
    return col


def _permuted(pos, order):
    """entity order[k] sits at pos[k]"""
    out = np.empty_like(pos)
    out[np.asarray(order)] = pos
    return out


def serpentine(n):
    """n grid points, each one step from the one before and at least sqrt(2) steps from every other: rows of `width` points three steps
    apart, joined at alternating ends by two points"""
    width = max(8, int(np.ceil(np.sqrt(n * ROW))))
    pts, z, forward = [], 0, True
    while len(pts) < n:
        pts += [(x, z) for x in (range(width) if forward else range(width - 1, -1, -1))]
        end = width - 1 if forward else 0
        pts += [(end, z + k) for k in range(1, ROW)]
        z, forward = z + ROW, not forward
    p = np.array(pts[:n], np.float64)
    p -= p.mean(axis=0).round()
    return np.stack([p[:, 0] * STEP, np.zeros(n), p[:, 1] * STEP], axis=1)


CHAIN_LENGTHS = (1, 2, 63, 64, 65, 257, 4097)
CHAIN_ORDERS = ("ascending", "reversed", "shuffled")


def chain(n, order):
    pos = serpentine(n)
    ids = {"ascending": np.arange(n), "reversed": np.arange(n)[::-1], "shuffled": np.random.default_rng(3900 + n).permutation(n)}[order]
    side = 4 if n <= 257 else 16
    return Case(f"chain of {n}, ids {order}", _world(_permuted(pos, ids), side), _spheres(n), islands=int(n >= 2), sizes=[n] if n >= 2 else [],
                anchored=0, min_edges=n - 1)


def ring():
    n = 65
    rad = STEP / (2.0 * np.sin(np.pi / n))
    ang = 2.0 * np.pi * np.arange(n) / n
    pos = np.stack([rad * np.cos(ang), np.zeros(n), rad * np.sin(ang)], axis=1)
    return Case("ring of 65", _world(_permuted(pos, np.random.default_rng(3965).permutation(n)), 4), _spheres(n), islands=1, sizes=[n], anchored=0, min_edges=n)


def cluster():
    n = 16
    return Case("cluster of 16 on one point", _world(np.tile([10.0, 0.0, 10.0], (n, 1))), _spheres(n, 0.5), islands=1, sizes=[n], anchored=0, min_edges=120)


def star(hub_fixed):
    """a hub of radius 20 and 200 spheres of radius 0.25 with their centres on its equator, 0.63 m apart: each touches the hub alone.
    The hub has the largest index, so every leaf's edge ends up hooking under, or racing for, one root."""
    k = 200
    ang = 2.0 * np.pi * np.arange(k) / k
    pos = np.concatenate([np.stack([20.0 * np.cos(ang), np.zeros(k), 20.0 * np.sin(ang)], axis=1), [[0.0, 0.0, 0.0]]])
    order = np.concatenate([np.random.default_rng(3920).permutation(k), [k]])
    w = _world(_permuted(pos, order))
    col = _spheres(k + 1, 0.25)
    col.radius[k] = 20.0
    if hub_fixed:
        w.group[k] = STATIC
        return Case("star, hub fixed", w, col, islands=0, sizes=[], anchored=k, min_edges=k)
    return Case("star, hub movable", w, col, islands=1, sizes=[k + 1], anchored=0, min_edges=k)


def slab(fixed_groups):
    """a ground slab of group 2 under 8 separate stacks of 3 boxes: what the feature exists for"""
    pos, he, group = [[0.0, -0.5, 0.0]], [[20.0, 0.5, 3.0]], [STATIC]
    for s in range(8):
        for level in range(3):
            pos.append([-17.5 + 5.0 * s, 0.45 + 0.9 * level, 0.0]); he.append([0.5, 0.5, 0.5]); group.append(1)
    n = len(pos)
    order = np.random.default_rng(3925).permutation(n)
    w = _world(_permuted(np.array(pos), order))
    col = cr.Colliders(n)
    col.type[:] = cr.BOX
    col.he[order] = F(he)
    w.group[order] = np.uint32(group)
    if fixed_groups:
        return Case("slab under 8 stacks, slab fixed", w, col, fixed_groups=STATIC, islands=8, sizes=[3] * 8, anchored=8, min_edges=24)
    return Case("slab under 8 stacks, nothing fixed", w, col, fixed_groups=0, islands=1, sizes=[25], anchored=0, min_edges=24)


def movers():
    """two chains of 5 and a mover that fills the gap between them on ticks 2 and 3 and is away on ticks 1 and 4"""
    a = np.stack([STEP * np.arange(5), np.zeros(5), np.zeros(5)], axis=1)
    b = a + [6 * STEP, 0.0, 0.0]
    away, between = [5 * STEP, 0.0, 40.0], [5 * STEP, 0.0, 0.0]
    order = np.random.default_rng(3930).permutation(11)
    ticks = [_permuted(np.concatenate([a, b, [m]]), order).astype(F) for m in (away, between, between, away)]
    c = Case("movers", _world(ticks[0]), _spheres(11), ticks=ticks)
    c.per_tick = [(2, [5, 5]), (1, [11]), (1, [11]), (2, [5, 5])]
    return c


def empty():
    k = 7
    gx, gz = np.meshgrid(np.arange(k), np.arange(k))
    pos = np.stack([gx.ravel() * 20.0 - 60.0, np.zeros(k * k), gz.ravel() * 20.0 - 60.0], axis=1)
    w = _world(pos)
    w.group[::5] = STATIC
    return Case("empty touching list", w, _spheres(k * k, 1.0), islands=0, sizes=[], anchored=0)


RANDOM_SEEDS, RANDOM_SIZES = (3941, 3942, 3943), (600, 2000)


def random_world(seed, n, bounds=False):
    """tests/pair_shapes_cases.agreement_world with n colliders at its density, about a third of them in group 2; bounds: a tenth are
    Bounds proxies, whose pairs stay on their AABB answer"""
    w, col = G.agreement_world(seed, n=n)
    grow = np.sqrt(n / G.AGREEMENT_N)
    w.pos[:, 0] *= F(grow); w.pos[:, 2] *= F(grow)
    rng = np.random.default_rng(seed + 50)
    w.group[rng.random(n) < 1.0 / 3.0] = STATIC
    if bounds:
        col.type[rng.random(n) < 0.1] = cr.BOUNDS
    return Case(f"random world of {n}, seed {seed}" + (", Bounds proxies" if bounds else ""), w, col, min_edges=n // 2)


def truncated():
    c = random_world(3951, 600)
    c.name, c.max_touching, c.min_edges = "truncated touching list", 100, 100
    return c


def cases():
    out = [chain(n, o) for n in CHAIN_LENGTHS for o in CHAIN_ORDERS]
    out += [ring(), cluster(), star(False), star(True), slab(STATIC), slab(0), movers(), empty(), truncated()]
    out += [random_world(s, n) for n in RANDOM_SIZES for s in RANDOM_SEEDS]
    out += [random_world(3961, 600, bounds=True)]
    return out


CASES = cases()
NAMES = [c.name for c in CASES]
_REFERENCE = {}


def reference(oracle, case, tick=0):
    """(touching set [k][2], kept_as_boxes, labels, info) of one tick of a case, from the oracle's matrices and pair set and the fp32
    witness of the touching pairs -- never from the library.  Computed once per (case, tick) and shared; do not write to it."""
    key = (case.name, tick)
    if key not in _REFERENCE:
        w = case.w
        saved = w.pos
        w.pos = np.ascontiguousarray(case.ticks[tick], F)
        try:
            m = G.oracle_matrices(oracle, w)
            pairs = G.oracle_pairs(oracle, m, case.col, w)
        finally:
            w.pos = saved
        touching, refined = R.touching32(m, case.col, pairs)
        tset = pairs[touching]
        labels, _, info = I.islands_union_find(tset, case.words(), w.n, case.fixed_groups, list_truncated=len(tset) > case.max_touching)
        for a in (tset, labels):
            a.setflags(write=False)
        _REFERENCE[key] = (tset, int((touching & ~refined).sum()), labels, info)
    return _REFERENCE[key]
