"""A witness of the pair sleep, written from the text of include/sc_tick.h "pair sleep": numpy fp32, a plain loop per island, no code
shared with the kernels.  It works from what a run reads back -- the world matrices [n][16] (column-major: element c * 4 + r is row r,
column c), the islands' labels and edge islands, the listed touching pairs -- and keeps anchor, rest and the asleep bit from run to run.
No GPU, no library."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
ASLEEP, STILL, MOVABLE = 1 << 8, 1 << 9, 1 << 10
RESYNC, FELL_OVERFLOW, WOKE_OVERFLOW, LIST_TRUNCATED = 1, 2, 4, 8
INFO_FIELDS = ("flags", "asleep", "islands_asleep", "fell_asleep", "woke", "awake_entries", "epoch", "pad")
LIN = [12, 13, 14]                         # the translation: .w of rows 0..2
ANG = [0, 1, 2, 4, 5, 6, 8, 9, 10]         # the nine other elements of the three rows


def still32(m, anchor, lin_tol, ang_tol):
    """still(e) in fp32: subtract, absolute value, compare; a NaN anywhere compares false"""
    m, anchor = np.ascontiguousarray(m, F), np.ascontiguousarray(anchor, F)
    with np.errstate(invalid="ignore"):
        d = np.abs(m - anchor)
        assert d.dtype == F
        return (d[:, LIN] <= F(lin_tol)).all(axis=1) & (d[:, ANG] <= F(ang_tol)).all(axis=1)


def still64(m, anchor, lin_tol, ang_tol):
    """the same in float64, element by element in Python: agrees with still32 wherever the fp32 difference is exact"""
    out = np.zeros(len(m), bool)
    for e in range(len(m)):
        ok = True
        for idx, tol in [(i, lin_tol) for i in LIN] + [(i, ang_tol) for i in ANG]:
            w, a = float(m[e][idx]), float(anchor[e][idx])
            if w != w or a != a or not abs(w - a) <= float(F(tol)):
                ok = False
        out[e] = ok
    return out


class Witness:
    def __init__(self, lin_tol=0.005, ang_tol=0.005, rest_runs=120, max_events=4096, rank=0, still=still32):
        self.lin_tol, self.ang_tol, self.rest_runs, self.max_events, self.rank, self.still = lin_tol, ang_tol, rest_runs, max_events, rank, still
        self.resync()

    def resync(self):
        self.valid, self.epoch = False, 0
        self.anchor = np.zeros((0, 16), F)
        self.rest = np.zeros(0, np.uint32)
        self.asleep = np.zeros(0, bool)

    def _cover(self, n):
        """an entity the count newly covers starts from the zeroed state"""
        have = len(self.rest)
        if n > have:
            self.anchor = np.concatenate([self.anchor, np.zeros((n - have, 16), F)])
            self.rest = np.concatenate([self.rest, np.zeros(n - have, np.uint32)])
            self.asleep = np.concatenate([self.asleep, np.zeros(n - have, bool)])

    def wake(self, ids):
        for i in np.asarray(ids, np.uint32).reshape(-1):
            e = int(i) & 0xFFFFFF
            assert int(i) >> 24 == self.rank and e < len(self.rest)
            self.rest[e] = 0
            self.anchor[e, LIN + ANG] = np.nan

    def run(self, m, words, fixed_groups, labels, listed, edge, list_truncated=0):
        """one flagged run over n = len(m) entities; returns (states[n], fell ids, woke ids, info) with the event sets complete
        (a short list of the library's is a subset of them)"""
        m = np.ascontiguousarray(m, F).reshape(-1, 16)
        n = len(m)
        labels, edge = np.asarray(labels, np.uint32), np.asarray(edge, np.uint32)
        listed = np.asarray(listed, np.uint32).reshape(-1, 2)
        assert len(labels) == n and len(edge) == len(listed)
        self._cover(n)
        first = not self.valid
        self.epoch += 1
        still = np.zeros(n, bool) if first else self.still(m, self.anchor[:n], self.lin_tol, self.ang_tol)
        self.anchor[:n][~still] = m[~still]
        self.rest[:n] = np.where(still, np.minimum(self.rest[:n] + 1, 255), 0)
        group = np.asarray(words, np.uint32)[:n] & 0xFFFF
        fixed = (group & fixed_groups) != 0
        movable = ~fixed
        assert np.array_equal(labels != NONE, movable)
        awake = set()
        for root in np.unique(labels[movable]):            # a plain loop per island
            members = np.flatnonzero(labels == root)
            if (self.rest[members] < self.rest_runs).any():
                awake.add(int(root))

        def own(idv):
            e = int(idv) & 0xFFFFFF
            return e if (int(idv) >> 24) == self.rank and e < n else -1

        for a, b in listed:                                 # the anchored-entry rule
            ea, eb = own(a), own(b)
            ma, mb = ea >= 0 and movable[ea], eb >= 0 and movable[eb]
            if ma == mb:
                continue
            mover, other = (ea, eb) if ma else (eb, ea)
            if other >= 0 and fixed[other] and self.rest[other] == 0:
                awake.add(int(labels[mover]))
        asleep = np.array([bool(movable[e]) and int(labels[e]) not in awake for e in range(n)], bool)
        was = self.asleep[:n].copy()
        fell = np.flatnonzero(asleep & ~was).astype(np.uint32) | np.uint32(self.rank << 24)
        woke = np.flatnonzero(~asleep & was).astype(np.uint32) | np.uint32(self.rank << 24)
        self.asleep[:n] = asleep
        self.valid = True
        states = self.rest[:n] | np.where(asleep, ASLEEP, 0).astype(np.uint32) | np.where(still, STILL, 0).astype(np.uint32) | \
            np.where(movable, MOVABLE, 0).astype(np.uint32)
        roots_asleep = int((asleep & ((labels & 0xFFFFFF) == np.arange(n))).sum())
        flags = (RESYNC if first else 0) | (FELL_OVERFLOW if len(fell) > self.max_events else 0) | (WOKE_OVERFLOW if len(woke) > self.max_events else 0) | \
            (LIST_TRUNCATED if list_truncated else 0)
        info = dict(flags=flags, asleep=int(asleep.sum()), islands_asleep=roots_asleep, fell_asleep=len(fell), woke=len(woke),
                    awake_entries=int(sum(1 for x in edge if x != NONE and int(x) in awake)), epoch=self.epoch, pad=0)
        return states.astype(np.uint32), fell, woke, info
