"""Witness of the trigger volumes (include/sc_tick.h "trigger volumes"), assembled from the witnesses the project already has.

    resolve     numpy fp32 in the header's operation order: M = W * L, left to right, unfused; ANCHOR_NONE: M = L untouched; an anchor
                >= n or a non-finite entry among the twelve: no members, the matrix reported as the quiet NaN 0x7FC00000
    members     tests/overlap_ref.py (aabb_hits, exact_hits) over the resolved volumes -- no shape arithmetic in here; skip_self becomes
                the skip id rank << 24 | anchor
    events      Python set differences against the sets of the last flagged tick (class Witness)

Volumes: the dict of tests/overlap_ref.py (its m16 is the LOCAL matrix, its skip None) plus `anchor` and `skip_self`."""
import numpy as np

from tests import overlap_ref as ref

F = np.float32
U = np.uint32
NONE, DEAD = 0xFFFFFFFF, 0xFFFFFFFE
QNAN = np.array([0x7FC00000], U).view(F)[0]


def volumes(anchor, type, local16, he, radius, hh, mask, skip_self=None):
    vol = ref.volumes(type, local16, he, radius, hh, mask)
    k = len(vol["type"])
    vol["anchor"] = np.ascontiguousarray(anchor, U).reshape(k)
    vol["skip_self"] = np.ones(k, np.uint8) if skip_self is None else np.ascontiguousarray(skip_self, np.uint8).reshape(k)
    return vol


def take(vol, idx):
    return {k: (None if v is None else v[idx]) for k, v in vol.items()}


def args(vol):
    """what WorldTick.trigger_volumes takes, in its order"""
    return vol["anchor"], vol["type"], vol["m16"], vol["he"], vol["radius"], vol["hh"], vol["mask"], vol["skip_self"]


def resolve(world16, vol, n):
    """(m16 [k, 16] fp32 column-major with last row (0, 0, 0, 1), alive [k]) as scTickReadTriggerMatrices reports them"""
    W = np.ascontiguousarray(world16, F).reshape(-1, 16)
    L = vol["m16"]
    k = len(L)
    out = np.zeros((k, 16), F)
    out[:, 15] = F(1.0)
    alive = np.ones(k, bool)
    with np.errstate(all="ignore"):
        for v in range(k):
            a = int(vol["anchor"][v])
            l = lambda r, c: L[v, c * 4 + r]
            if a == NONE:
                for r in range(3):
                    for c in range(4):
                        out[v, c * 4 + r] = l(r, c)
            elif a >= n:
                alive[v] = False
            else:
                w = lambda r, c: W[a, c * 4 + r]
                for r in range(3):
                    for c in range(3):
                        out[v, c * 4 + r] = F(F(F(w(r, 0) * l(0, c)) + F(w(r, 1) * l(1, c))) + F(w(r, 2) * l(2, c)))
                    out[v, 12 + r] = F(F(F(F(w(r, 0) * l(0, 3)) + F(w(r, 1) * l(1, 3))) + F(w(r, 2) * l(2, 3))) + w(r, 3))
            twelve = out[v].reshape(4, 4)[:, :3]
            if alive[v] and not np.isfinite(twelve).all():
                alive[v] = False
            if not alive[v]:
                out[v].reshape(4, 4)[:, :3] = QNAN
    assert out.dtype == F
    return out, alive


def resolve64(world16, vol, n):
    """the same product in float64 (alive volumes only are meaningful)"""
    W = np.asarray(world16, np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
    L = np.asarray(vol["m16"], np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
    out = np.zeros((len(L), 16))
    for v in range(len(L)):
        a = int(vol["anchor"][v])
        m = L[v].copy() if a == NONE else (W[a] @ L[v] if a < n else np.full((4, 4), np.nan))
        m[3] = [0, 0, 0, 1]
        out[v] = m.T.reshape(16)
    return out


def members(oracle, mn, mx, group, mask, world16, col, vol, n, shapes=0, rank=0):
    """(sets: a sorted uint32 id array per volume, resolved matrices, alive): the overlap witness over the resolved volumes"""
    m16, alive = resolve(world16, vol, n)
    k = len(alive)
    sets = [np.zeros(0, U) for _ in range(k)]
    idx = np.flatnonzero(alive)
    if len(idx):
        anchored = (vol["anchor"][idx] < n) & (vol["skip_self"][idx] != 0)
        skip = np.where(anchored, vol["anchor"][idx] | U(rank << 24), U(ref.NO_SKIP)).astype(U)
        res = ref.volumes(vol["type"][idx], m16[idx], vol["he"][idx], vol["radius"][idx], vol["hh"][idx], vol["mask"][idx], skip)
        hits = ref.aabb_hits(oracle, mn, mx, group, mask, res, rank)
        keep = np.ones(len(hits), bool)
        if shapes:
            keep, _ = ref.exact_hits(hits, world16, col, res, n)
        for j, v in enumerate(idx):
            sets[v] = np.sort(hits[keep & (hits[:, 1] == j), 0]).astype(U) | U(rank << 24)
    return sets, m16, alive


class Witness:
    """what the context remembers, and what a flagged tick must report for the true member sets of that tick"""

    def __init__(self, k, max_members, max_events):
        self.k, self.max_members, self.max_events = k, max_members, max_events
        self.memory = [None] * k

    def forget(self):
        self.memory = [None] * self.k

    def tick(self, sets):
        """(entered, exited) as sorted lists of (volume, id) and the info dict"""
        entered, exited, resync, overflow = [], [], 0, 0
        for v, s in enumerate(sets):
            now = set(int(x) for x in s)
            if len(now) > self.max_members:
                overflow += 1
                self.memory[v] = None
                continue
            if self.memory[v] is None:
                resync += 1
                entered += [(v, i) for i in now]
            else:
                entered += [(v, i) for i in now - self.memory[v]]
                exited += [(v, i) for i in self.memory[v] - now]
            self.memory[v] = now
        info = dict(volumes=self.k, max_members=self.max_members, members=int(sum(len(s) for s in sets)), entered=len(entered), exited=len(exited),
                    resync_volumes=resync, overflow_volumes=overflow,
                    events_truncated=int(len(entered) > self.max_events or len(exited) > self.max_events))
        return sorted(entered), sorted(exited), info
