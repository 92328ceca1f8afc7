"""Witness of pair persistence (include/sc_tick.h "pair persistence"), independent of the kernels: numpy fp32 written from the header text,
one rounding per operation, left to right.  The device's list order is not fixed, so the witness always works from the lists as read
back: it takes the previous flagged run's touching list, manifold records, persistence records and payload rows (as they stood when this
run began) with that run's world matrices, and this run's list, manifolds and matrices, and returns the records, the payload rows and the
report the device must reproduce bit for bit.

    dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z      c_k = column k      T = translation      n_k = dot(c_k, c_k)"""
import numpy as np

from tests.shape_rays_ref import dot

F = np.float32
NONE = 0xFFFFFFFF                                              # SC_TICK_PERSIST_NONE
DTYPE = np.dtype([("prev_entry", np.uint32), ("prev_slot", np.uint8, 4), ("age", np.uint8, 4), ("reserved", np.uint32)])
INFO_FIELDS = ("written", "kept_pairs", "new_pairs", "kept_points", "new_points", "resync", "list_truncated", "gave_up")


class Run:
    """what a flagged run leaves behind: its list [n][2], manifold records, persistence records, payload rows [n][4][4] and matrices"""
    def __init__(self, listed, manifolds, records, payloads, matrices):
        self.listed = np.ascontiguousarray(listed, np.uint32).reshape(-1, 2)
        self.manifolds, self.records = manifolds, records
        self.payloads = np.ascontiguousarray(payloads, F).reshape(-1, 4, 4)
        self.matrices = np.ascontiguousarray(matrices, F).reshape(-1, 16)


def keys(pairs):
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    return (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64)


def local_points32(matrices, listed, manifolds):
    """[n][4][3] fp32: the manifold points of every entry in the frame of its first member; slots at or above count are +0"""
    m = np.ascontiguousarray(matrices, F).reshape(-1, 16)
    listed = np.ascontiguousarray(listed, np.uint32).reshape(-1, 2)
    out = np.zeros((len(listed), 4, 3), F)
    count = manifolds["count"]
    idx = np.flatnonzero(count > 0)
    if not len(idx):
        return out
    e = (listed[idx, 0] & 0xFFFFFF).astype(np.int64)
    rows = [[m[e, c * 4 + r] for c in range(4)] for r in range(3)]              # rows[r][c]
    col = [[rows[0][c], rows[1][c], rows[2][c]] for c in range(3)]
    T = [rows[r][3] for r in range(3)]
    with np.errstate(all="ignore"):
        u = []
        for k in range(3):
            q = np.sqrt(dot(col[k], col[k])).astype(F)
            u.append([(col[k][i] / q).astype(F) for i in range(3)])
        for s in range(4):
            p = manifolds["point"][idx, s]
            r = [(p[:, i] - T[i]).astype(F) for i in range(3)]
            live = s < count[idx]
            for k in range(3):
                out[idx, s, k] = np.where(live, dot(r, u[k]), F(0.0))
    return out


def persist32(prev, listed, manifolds, matrices, match_dist, truncated=False):
    """(records, payload rows [n][4][4], info) of a flagged run over `listed` / `manifolds` / `matrices`; prev: the remembered Run, or
    None on a resync.  truncated: ScTickPairShapeInfo::truncated | pairs_truncated of the run."""
    listed = np.ascontiguousarray(listed, np.uint32).reshape(-1, 2)
    n = len(listed)
    rec = np.zeros(n, DTYPE)
    rec["prev_entry"] = NONE
    rec["prev_slot"] = 0xFF
    rows = np.zeros((n, 4, 4), F)
    x = local_points32(matrices, listed, manifolds)
    m2 = F(match_dist) * F(match_dist)
    kept_points = 0
    if prev is not None and len(prev.listed):
        y = local_points32(prev.matrices, prev.listed, prev.manifolds)
        pk = keys(prev.listed)
        order = np.argsort(pk, kind="stable")                   # the first of equal keys is the smallest entry index
        sk = pk[order]
        k = keys(listed)
        at = np.searchsorted(sk, k, side="left")
        found = (at < len(sk)) & (sk[np.minimum(at, len(sk) - 1)] == k)
        for i in np.flatnonzero(found):
            pe = int(order[at[i]])
            rec["prev_entry"][i] = pe
            taken = [False] * 4
            for s in range(int(manifolds["count"][i])):
                best, bd = -1, None
                for t in range(int(prev.manifolds["count"][pe])):
                    if taken[t]:
                        continue
                    with np.errstate(all="ignore"):
                        e = [F(x[i, s, c] - y[pe, t, c]) for c in range(3)]
                        d = F(F(F(e[0] * e[0]) + F(e[1] * e[1])) + F(e[2] * e[2]))
                    if d <= m2 and (best < 0 or d < bd):
                        best, bd = t, d
                if best >= 0:
                    taken[best] = True
                    rec["prev_slot"][i, s] = best
                    rec["age"][i, s] = min(int(prev.records["age"][pe, best]) + 1, 255)
                    rows[i, s] = prev.payloads[pe, best]
                    kept_points += 1
    kept_pairs = int((rec["prev_entry"] != NONE).sum())
    info = dict(written=n, kept_pairs=kept_pairs, new_pairs=n - kept_pairs, kept_points=kept_points,
                new_points=int(manifolds["count"].sum()) - kept_points, resync=1 if prev is None else 0, list_truncated=1 if truncated else 0, gave_up=0)
    return rec, rows, info


def bits(rec):
    """the records as raw words [k][4], for bit-for-bit comparison"""
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 4)


def row_bits(rows):
    """payload rows as raw words, in their own shape"""
    return np.ascontiguousarray(rows, F).view(np.uint32)


# ---- float64, by another route -------------------------------------------------------------------------------------------------------
def local_points64(matrices, listed, manifolds):
    """[n][4][3] float64: the same points through the inverse of the normalised rotation (orthogonal frames)"""
    m = np.ascontiguousarray(matrices, F).reshape(-1, 16).astype(np.float64)
    listed = np.ascontiguousarray(listed, np.uint32).reshape(-1, 2)
    e = (listed[:, 0] & 0xFFFFFF).astype(np.int64)
    M4 = m[e].reshape(-1, 4, 4).transpose(0, 2, 1)             # [n][r][c]
    Rm = M4[:, :3, :3]
    U = Rm / np.linalg.norm(Rm, axis=1, keepdims=True)         # unit columns
    r = manifolds["point"].astype(np.float64) - M4[:, None, :3, 3]
    return np.einsum("nsr,nrk->nsk", r, U)
