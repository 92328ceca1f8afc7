"""Two independent witnesses of the pair islands, written from the text of include/sc_tick.h "pair islands": a union-find and a
breadth-first search.  Both take (pairs, group words, count, fixed_groups, rank) -- the touching list as [k][2] ids, the layer words of
the context's entities (the group is their low 16 bits) -- and return (labels[count], edge_islands[k], info).  No GPU, no library."""
from collections import deque

import numpy as np

NONE = 0xFFFFFFFF
INFO_FIELDS = ("edges", "linking", "anchored", "islands", "bodies", "movable", "list_truncated", "gave_up")


def _movable_entities(words, count, fixed_groups):
    g = np.ascontiguousarray(words, np.uint32)[:count] & np.uint32(0xFFFF)
    return (g & np.uint32(fixed_groups)) == 0


def _member(idv, ok, count, rank):
    """dense index of a member id, or -1 when it is fixed"""
    e = int(idv) & 0xFFFFFF
    return e if (int(idv) >> 24) == rank and e < count and ok[e] else -1


def _finish(labels_idx, ok, pairs, members, count, rank, list_truncated):
    labels = np.full(count, NONE, np.uint32)
    for e in range(count):
        if ok[e]:
            labels[e] = (rank << 24) | labels_idx[e]
    edge = np.full(len(pairs), NONE, np.uint32)
    linking = 0
    for i, (a, b) in enumerate(members):
        if a >= 0:
            edge[i] = labels[a]
        elif b >= 0:
            edge[i] = labels[b]
        linking += a >= 0 and b >= 0
    roots, sizes = np.unique(labels[ok], return_counts=True)
    big = sizes >= 2
    info = dict(edges=len(pairs), linking=int(linking), anchored=int(len(pairs) - linking), islands=int(big.sum()), bodies=int(sizes[big].sum()),
                movable=int(ok.sum()), list_truncated=int(bool(list_truncated)), gave_up=0)
    return labels, edge, info


def islands_union_find(pairs, words, count, fixed_groups=2, rank=0, list_truncated=0):
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    ok = _movable_entities(words, count, fixed_groups)
    members = [(_member(a, ok, count, rank), _member(b, ok, count, rank)) for a, b in pairs]
    parent = list(range(count))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:                            # full compression: this witness need not resemble the device's halving
            parent[x], x = root, parent[x]
        return root

    for a, b in members:
        if a >= 0 and b >= 0:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)           # the smaller index stays the root: the root is the label
    return _finish([find(e) for e in range(count)], ok, pairs, members, count, rank, list_truncated)


def islands_bfs(pairs, words, count, fixed_groups=2, rank=0, list_truncated=0):
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    ok = _movable_entities(words, count, fixed_groups)
    members = [(_member(a, ok, count, rank), _member(b, ok, count, rank)) for a, b in pairs]
    near = [[] for _ in range(count)]
    for a, b in members:
        if a >= 0 and b >= 0:
            near[a].append(b); near[b].append(a)
    label = [-1] * count
    for start in range(count):                              # ascending: whoever starts a search is the smallest index of its island
        if not ok[start] or label[start] >= 0:
            continue
        label[start] = start
        todo = deque([start])
        while todo:
            for y in near[todo.popleft()]:
                if label[y] < 0:
                    label[y] = start
                    todo.append(y)
    return _finish(label, ok, pairs, members, count, rank, list_truncated)


def island_sizes(labels):
    """sorted sizes of the islands of two or more members"""
    lab = np.asarray(labels, np.uint32)
    _, sizes = np.unique(lab[lab != NONE], return_counts=True)
    return sorted(int(s) for s in sizes if s >= 2)
