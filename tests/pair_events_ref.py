"""The witness of the pair events (include/sc_tick.h "pair events") and the scripted worlds its tests run.

Given the pair sets of consecutive flagged ticks as sorted uint32[k, 2], `Witness.tick` returns what the library must report: the begun and
ended sets (numpy set difference on the 64-bit keys a << 32 | b) under the resync, overflow and truncation rules.  The sets come from
`oracle.broadphase_bruteforce` / `broadphase_grid` on the ORACLE's own world AABBs (`oracle_pairs`), as in tests/test_gpu_broadphase.py --
never from the library's pair list.

A script is a start world and one entry per tick: the positions to set before that tick (None = a still tick).  The GPU tests feed them
through upload_positions, the oracle through set_local_positions; tests/test_pair_events_cpu.py checks that every script really produces
the situation its GPU test relies on.  No GPU, no library call in this file.
"""
import numpy as np

from tests import worlds

F = np.float32


# ---- the witness ---------------------------------------------------------------------------------------------------------------
def keys(p):
    p = np.asarray(p, np.uint32).reshape(-1, 2)
    return p[:, 0].astype(np.uint64) << np.uint64(32) | p[:, 1].astype(np.uint64)


def unkeys(k):
    k = np.asarray(k, np.uint64)
    return np.stack([(k >> np.uint64(32)).astype(np.uint32), (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)], axis=1).reshape(-1, 2)


def sorted_pairs(p):
    """rows (a, b) ordered by the key a << 32 | b"""
    return unkeys(np.sort(keys(p)))


EMPTY = np.zeros((0, 2), np.uint32)


class Witness:
    """The remembered set and the rules.  tick(pairs) -> (begun, ended, info): sorted uint32[k, 2] lists in full -- a truncated tick
    (info["events_truncated"]) lists any max_events members of them -- and the six words of ScTickPairEventInfo."""

    def __init__(self, max_tracked, max_events):
        self.max_tracked, self.max_events = int(max_tracked), int(max_events)
        self.prev = None                                  # keys of the remembered set; None = nothing remembered

    def invalidate(self):
        """dense indices were renamed (remove_entities, a shrinking count): the next flagged tick is a resync tick"""
        self.prev = None

    def tick(self, pairs, pairs_truncated=False):
        cur = np.unique(keys(pairs))
        assert len(cur) == len(np.asarray(pairs).reshape(-1, 2)), "a pair set lists every pair once"
        if pairs_truncated or len(cur) > self.max_tracked:
            self.prev = None
            return EMPTY, EMPTY, dict(begun=0, ended=0, tracked=0, resync=0, overflow=1, events_truncated=0)
        resync = self.prev is None
        begun = cur if resync else np.setdiff1d(cur, self.prev, assume_unique=True)
        ended = np.zeros(0, np.uint64) if resync else np.setdiff1d(self.prev, cur, assume_unique=True)
        self.prev = cur
        trunc = len(begun) > self.max_events or len(ended) > self.max_events
        return unkeys(begun), unkeys(ended), dict(begun=len(begun), ended=len(ended), tracked=len(cur), resync=int(resync), overflow=0,
                                                  events_truncated=int(trunc))


# ---- the tables, restated --------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def pair_hash(k):
    """pairHash of sc_tick_pair_events.hip: MurmurHash3's 64-bit finaliser, low 32 bits"""
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & _M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & _M64
    k ^= k >> 33
    return k & 0xFFFFFFFF


class TableModel:
    """The three kernels' algorithm on the host, slot for slot: two open-addressing tables used in turn, linear probing from
    pair_hash(key) & (slots - 1), a mark per slot, the sweep, the swap.  (Which slots a set occupies under linear probing does not depend
    on the insertion order, so the occupancy figures hold for the device whatever order its threads run in; the probe lengths are those of
    this order.)  tick(pairs) -> (begun keys, ended keys, info, stats) with stats = slots, load, longest_insert_probe, insert_wraps,
    lookup_wraps: how many keys were placed / found in the previous table at a slot below their home, i.e. past the table's end."""

    def __init__(self, max_tracked, max_events):
        self.slots = 64
        while self.slots < 2 * max_tracked:
            self.slots <<= 1
        self.max_tracked, self.max_events = int(max_tracked), int(max_events)
        self.table = [[0] * self.slots, [0] * self.slots]
        self.marks = [set(), set()]
        self.cur, self.valid = 0, 0

    def tick(self, pairs, pairs_truncated=False):
        ks = [int(k) for k in keys(pairs)]
        mask = self.slots - 1
        overflow = pairs_truncated or len(ks) > self.max_tracked
        cur, prev, pmarks = self.table[self.cur], self.table[self.cur ^ 1], self.marks[self.cur ^ 1]
        begun, ended, tracked = [], [], 0
        stats = dict(slots=self.slots, load=0.0, longest_insert_probe=0, insert_wraps=0, lookup_wraps=0)
        if not overflow:
            for k in ks:                                                   # k_pair_events_diff
                home = pair_hash(k) & mask
                pos, inserted = home, False
                for n in range(self.slots):
                    if cur[pos] == 0:
                        cur[pos], inserted = k, True
                        break
                    if cur[pos] == k:
                        break
                    pos = (pos + 1) & mask
                if not inserted:
                    continue
                tracked += 1
                stats["longest_insert_probe"] = max(stats["longest_insert_probe"], n)
                stats["insert_wraps"] += pos < home
                pos, found = home, False
                for n in range(self.slots):
                    if prev[pos] == k:
                        pmarks.add(pos)
                        found = True
                        stats["lookup_wraps"] += pos < home
                        break
                    if prev[pos] == 0:
                        break
                    pos = (pos + 1) & mask
                if not found:
                    begun.append(k)
        for i in range(self.slots):                                        # k_pair_events_sweep
            if not overflow and prev[i] and i not in pmarks:
                ended.append(prev[i])
            prev[i] = 0
            if overflow:
                cur[i] = 0
        pmarks.clear()
        stats["load"] = tracked / self.slots
        if overflow:                                                       # k_pair_events_finish
            self.valid = 0
            return [], [], dict(begun=0, ended=0, tracked=0, resync=0, overflow=1, events_truncated=0), stats
        info = dict(begun=len(begun), ended=len(ended), tracked=tracked, resync=int(not self.valid), overflow=0,
                    events_truncated=int(len(begun) > self.max_events or len(ended) > self.max_events))
        self.valid, self.cur = 1, self.cur ^ 1
        return sorted(begun), sorted(ended), info, stats


def oracle_pairs(oracle, ow, w, brute=True, cell=64.0):
    """this tick's pair set from the oracle's own boxes (call after ow.transform_system())"""
    mn, mx = ow.world_aabbs()
    n = len(w.group)
    if brute:
        return oracle.broadphase_bruteforce(mn[:n], mx[:n], w.group, w.mask)
    return oracle.broadphase_grid(mn[:n], mx[:n], w.group, w.mask, cell)


def set_positions(ow, t, pos):
    """one tick's positions on both sides (either may be None); setLocalPosition marks every entity dirty on both"""
    if ow is not None:
        ow.set_local_positions(ow.dense_entities()[:len(pos)], pos)
    if t is not None:
        t.upload_positions(0, pos)


def oracle_sets(oracle, w, steps, brute=True):
    """the pair set of every tick of a script, from the oracle alone"""
    ow = worlds.oracle_world(oracle, w, camera=False)
    out = []
    for pos in steps:
        if pos is not None:
            set_positions(ow, None, pos)
        ow.transform_system()
        out.append(oracle_pairs(oracle, ow, w, brute))
    ow.close()
    return out


_SETS = {}


def script_sets(oracle, name):
    """(world, steps, pair set per tick) of a named script; computed once per session and shared by the tests -- treat as read-only"""
    if name not in _SETS:
        w, steps = SCRIPTS[name]()
        _SETS[name] = (w, steps, oracle_sets(oracle, w, steps))
    return _SETS[name]


# ---- the scripted worlds -------------------------------------------------------------------------------------------------------
def line_world():
    """Six unit boxes on the x axis, everything collides with everything.  Boxes 0 and 1 overlap -- pair (0, 1), whose key has a zero
    high word, exists from the first tick -- the others stand 3 m apart.  Box 4 steps next to box 3 (pair (3, 4) begins), stays, steps back."""
    w = worlds.random_world(6, seed=1, p_child=0.0, p_no_bounds=0.0, p_no_mesh=0.0)
    w.pos[:] = 0.0
    w.pos[:, 0] = F([0.0, 0.8, 3.0, 6.0, 9.0, 12.0])
    w.rot[:] = 0.0
    w.scale[:] = 1.0
    w.bmin[:], w.bmax[:] = -0.5, 0.5
    w.group[:], w.mask[:] = 1, 0xFFFFFFFF
    near, held = w.pos.copy(), None
    near[4, 0] = 6.7
    return w, [None, near, held, w.pos.copy()]


LINE_EVENTS = [([(0, 1)], []), ([(3, 4)], []), ([], []), ([], [(3, 4)])]      # (begun, ended) per tick; the first tick is the resync


def random_run(n, seed, ticks, move_seed):
    """worlds.random_world(n, spread=150, max_depth=3); before every tick but the first a random tenth of the ROOTS is displaced by up to
    +-3 m per axis (their families follow).  Nudging all roots together would change no pair."""
    w = worlds.random_world(n, seed=seed, spread=150.0, max_depth=3)
    rng = np.random.default_rng(move_seed)
    roots = np.flatnonzero(w.parent < 0)
    pos, steps = w.pos.copy(), [None]
    for _ in range(ticks - 1):
        mv = rng.choice(roots, max(len(roots) // 10, 1), replace=False)
        pos = pos.copy()
        pos[mv] += rng.uniform(-3.0, 3.0, (len(mv), 3)).astype(F)
        steps.append(pos)
    return w, steps


RANDOM_N, RANDOM_TICKS, RANDOM_SEED, RANDOM_MOVE_SEED = 3000, 12, 31, 5
SMALL_N, SMALL_SEED, SMALL_MOVE_SEED = 600, 32, 5          # graph mode (8 ticks), split tick (4 ticks), unflagged ticks in between (4 ticks)


def crowded_run():
    """One sector holds 300 of 1500 boxes (the world of test_bin_overflow_takes_the_slow_path, the crowd drawn a little closer: +-7.2 m);
    six ticks, before each but the first the crowd jitters by up to +-0.25 m.  The set fills 90-100 % of CROWDED_MAX_TRACKED = 4096, whose
    tables have 8192 slots: a load factor just under one half, with long probe runs.  The crowd is the dense indices CROWD_FIRST ..
    CROWD_FIRST + 299, chosen -- the hash is fixed, so this is settled on the host (TableModel) -- so that on every tick the occupied run
    over the table's last slot carries on at slot 0: at least one key is placed, and on later ticks looked up, past the wrap.
    tests/test_pair_events_cpu.py pins all of it."""
    w = worlds.random_world(1500, seed=33, spread=300.0, p_child=0.0)
    crowd = slice(CROWD_FIRST, CROWD_FIRST + 300)
    w.pos[crowd] = F([10.0, 0.0, 10.0]) + np.random.default_rng(1).uniform(-7.2, 7.2, (300, 3)).astype(F)
    rng = np.random.default_rng(7)
    pos, steps = w.pos.copy(), [None]
    for _ in range(5):
        pos = pos.copy()
        pos[crowd] += rng.uniform(-0.25, 0.25, (300, 3)).astype(F)
        steps.append(pos)
    return w, steps


CROWD_FIRST = 119
CROWDED_MAX_TRACKED = 4096       # the table tests/test_pair_events_cpu.py checks and the GPU test reads


def cluster_run():
    """A sparse world of 400 flat boxes whose first CLUSTER entities are teleported together before tick 1 -- every two of them then
    overlap: CLUSTER * (CLUSTER - 1) / 2 more pairs -- and back apart before tick 2; before tick 3 one of them steps onto its neighbour."""
    w = worlds.random_world(400, seed=52, spread=150.0, p_child=0.0, p_no_bounds=0.0)
    w.group[:], w.mask[:] = 1, 0xFFFFFFFF
    w.rot[:CLUSTER] = 0.0
    w.scale[:CLUSTER] = 1.0
    w.bmin[:CLUSTER], w.bmax[:CLUSTER] = -1.0, 1.0
    w.pos[:CLUSTER] = F([200.0, 0.0, 200.0]) + F([5.0, 0.0, 0.0]) * np.arange(CLUSTER, dtype=F)[:, None]      # a row of their own, 5 m apart
    apart = w.pos.copy()
    together = apart.copy()
    together[:CLUSTER] = F([-200.0, 0.0, 200.0]) + F([0.1, 0.0, 0.0]) * np.arange(CLUSTER, dtype=F)[:, None]
    step = apart.copy()
    step[1] = apart[0] + F([0.5, 0.0, 0.0])
    return w, [None, together, apart, step]


CLUSTER = 8                      # 28 pairs begin at once
CLUSTER_MAX_TRACKED = 16         # between the quiet ticks' set (5, 6 pairs) and the teleport tick's (33)
TRUNCATION_MAX_EVENTS = 4

SCRIPTS = {
    "line": line_world,
    "random": lambda: random_run(RANDOM_N, RANDOM_SEED, RANDOM_TICKS, RANDOM_MOVE_SEED),
    "small": lambda: random_run(SMALL_N, SMALL_SEED, 8, SMALL_MOVE_SEED),
    "crowded": crowded_run,
    "cluster": cluster_run,
}
