"""The cases of tests/ray_walk_cases.py are what they claim (no GPU): every adversarial query is answered by the oracle's brute force
with a hit at the very end of the segment, on a box that the model of the unpadded sector walk does not reach, and its lower neighbour
misses.  The expected answers of tests/test_gpu_ray_walk.py are these brute-force answers."""
import numpy as np
import pytest

from tests import ray_walk_cases as rc, sweep_ref

F = np.float32
U = np.uint32
MIN_PER_CELL = 8
WHERE = ("near", "far")


def bits(x):
    return np.ascontiguousarray(x, F).view(U)


def boxes_of(w, n=None):
    n = w.n if n is None else n
    return w.bmin[:n], w.bmax[:n], w.group[:n], w.mask[:n]


@pytest.mark.parametrize("where", WHERE)
def test_ray_cells_hit_at_the_end_of_the_segment_beyond_the_modelled_walk(oracle, where):
    w, grid, rays, meta = rc.ray_batch(where)
    o, d, md, mask = rays
    want = oracle.raycast_boxes(*boxes_of(w), *rays)
    found, lower, upper = meta["role"] == 1, meta["role"] == 0, meta["role"] == 2
    assert (want["hit"][found] == 1).all() and np.array_equal(want["id"][found], meta["box"][found])
    assert np.array_equal(bits(want["distance"][found]), bits(md[found]))                      # t == max_dist
    assert (want["hit"][upper] == 1).all() and np.array_equal(want["id"][upper], meta["box"][upper])
    assert np.array_equal(bits(rc.up(want["distance"][upper])), bits(md[upper]))               # max_dist is t's upper neighbour
    assert (want["hit"][lower] == 0).all()
    # the model: not big, and registered in no sector of the unpadded walk's rectangle
    mn, mx = w.bmin[meta["box"]], w.bmax[meta["box"]]
    assert not grid.plan_bins(mn, mx)[4].any()
    rect = grid.walk_rect(o, rc.normalise(d), md)
    assert grid.unregistered(rect, mn, mx)[found].all()
    cells = list(rc.ray_cells(where))
    assert len(cells) == len(rc.DIRECTIONS) * len(rc.SPANS)
    for ci, (direction, span) in enumerate(cells):
        sel = found & (meta["cell"] == ci)
        assert sel.sum() >= MIN_PER_CELL, (where, direction, span, int(sel.sum()))
        assert rc._span_ok(tuple(r[sel] for r in rect), span).all()
        nd = rc.normalise(d[sel])
        if direction == "diag":
            assert (np.abs(nd[:, 0]) > 0.05).all() and (np.abs(nd[:, 2]) > 0.05).all()
        else:
            axis, sign = (0 if direction[1] == "x" else 2), (1 if direction[0] == "+" else -1)
            assert (np.sign(nd[:, axis]) == sign).all() and (nd[:, 2 - axis] == 0).all()
    # both kinds of boundary face occur: min == 64 k exactly, max == the last float below 64 k
    hit_boxes = np.unique(meta["box"][found])
    assert (np.mod(w.bmin[hit_boxes][:, [0, 2]], 64) == 0).any() and (np.mod(rc.up(w.bmax[hit_boxes][:, [0, 2]]), 64) == 0).any()


@pytest.mark.parametrize("where", WHERE)
def test_sweep_cells_meet_the_grown_box_at_the_end_beyond_the_modelled_walk(oracle, where):
    w, grid, q, meta = rc.sweep_batch(where)
    a, b, radius, hh, mask = q
    want = sweep_ref.sweep_boxes(oracle, *boxes_of(w), *q)
    found, lower = meta["role"] == 1, meta["role"] == 0
    mn, mx = w.bmin[meta["box"]], w.bmax[meta["box"]]
    hit, t, far, nd = rc.sweep_witness(a, b, radius, hh, mn, mx)                               # the numpy witness and the C oracle agree
    assert np.array_equal(hit, want["hit"] == 1) and np.array_equal(bits(t[hit]), bits(want["travel"][hit]))
    assert (want["hit"][found] == 1).all() and np.array_equal(want["id"][found], meta["box"][found])
    tr = want["travel"][found]
    assert ((bits(tr) == bits(far[found])) | (bits(rc.up(tr)) == bits(far[found]))).all()
    assert (want["hit"][lower] == 0).all()
    assert not grid.plan_bins(mn, mx)[4].any()
    rect = grid.walk_rect(a, nd, far, radius)
    assert grid.unregistered(rect, mn, mx)[found].all()
    for ci, (direction, span) in enumerate(rc.sweep_cells(where)):
        sel = found & (meta["cell"] == ci)
        assert sel.sum() >= MIN_PER_CELL, (where, direction, span, int(sel.sum()))
        assert rc._span_ok(tuple(r[sel] for r in rect), span).all()
    assert all((radius[found] == r).sum() >= 20 for r in rc.RADII)


@pytest.mark.parametrize("where", WHERE)
def test_zero_length_sweeps_start_on_the_grown_face(oracle, where):
    w, grid, q, meta = rc.zero_batch(where)
    a, b, radius, hh, mask = q
    d, far, moving = sweep_ref.segments(a, b)
    assert not moving.any() and (b != a).any()
    want = sweep_ref.sweep_boxes(oracle, *boxes_of(w), *q)
    on_face, lower, adversarial = meta["role"] >= 1, meta["role"] == 0, meta["role"] == 1
    assert (want["hit"][on_face] == 1).all() and np.array_equal(want["id"][on_face], meta["box"][on_face]) and (want["travel"] == 0).all()
    assert (want["hit"][lower] == 0).all()
    mn, mx = w.bmin[meta["box"]], w.bmax[meta["box"]]
    assert np.array_equal(rc.sweep_witness(a, b, radius, hh, mn, mx)[0], want["hit"] == 1)
    rect = grid.walk_rect(a, np.zeros_like(a), np.zeros(len(a), F), radius)
    assert np.array_equal(grid.unregistered(rect, mn, mx)[on_face], adversarial[on_face])
    for ci, direction in enumerate(rc.DIRECTIONS):
        count = int((adversarial & (meta["cell"] == ci)).sum())
        if (direction, where) in rc.ZERO_CELLS:
            assert count >= MIN_PER_CELL, (where, direction, count)
        else:
            assert count == 0, (where, direction, count)           # (why: the comment above ZERO_CELLS)


def test_the_first_example(oracle):
    w, grid, rays = rc.first_example()
    o, d, md, mask = rays
    want = oracle.raycast_boxes(*boxes_of(w), *rays)
    assert list(want["hit"]) == [0, 1, 1] and bits(want["distance"])[1] == bits(md)[1] == bits(want["distance"])[2]
    rect = grid.walk_rect(o, rc.normalise(d), md)
    assert grid.unregistered(rect, w.bmin[[0, 0, 0]], w.bmax[[0, 0, 0]])[:2].all()
    assert (o[:, 0] + rc.normalise(d)[:, 0] * md)[1] == rc.down(F(64.0))


def test_anchored_wrappers_reproduce_the_origins():
    for where in WHERE:
        w, _, rays, meta = rc.ray_batch(where)
        an, o, d, md, mask, skip = rc.as_anchor_none(rays)
        assert (an == rc.ALL).all() and o is rays[0] and not skip.any()
        T, keep, q = rc.as_anchor_translated(rays, w.n)
        anchor, l = q[0], q[1]
        assert len(keep) > len(rays[0]) // 2 and (anchor >= w.n).all() and (anchor < w.n + len(T)).all()
        t = T[anchor - w.n]
        assert np.array_equal(bits(l + t), bits(rays[0][keep]))
        assert (np.bincount(meta["cell"][keep][meta["role"][keep] == 1]) >= 4).all()       # every cell keeps cases
        wa = rc.box_world(w.bmin, w.bmax, w.origin, group=w.group, anchors=T)
        assert wa.n == w.n + len(T) and not wa.has_bounds[w.n:].any() and not wa.group[w.n:].any()


def test_the_face_and_tie_boxes_are_box_colliders_to_the_bit():
    for where in WHERE:
        w = rc.face_world(where)[0]
        c, h = rc.as_box_colliders(w.bmin, w.bmax)
        assert (h > 0).all()
    for name, mn, mx, rays, sweeps in rc.tie_worlds():
        rc.as_box_colliders(mn, mx)
    w = rc.crowded_world()[0]
    rc.as_box_colliders(w.bmin, w.bmax)


def test_the_crowded_world_passes_64_records_in_exactly_one_sector(oracle):
    w, grid, sector = rc.crowded_world()
    x0, x1, z0, z1, big = grid.plan_bins(w.bmin, w.bmax)
    assert not big.any()
    records = np.zeros((grid.sx, grid.sz), int)
    for i in range(w.n):
        for gx in range(int(x0[i]), int(x1[i]) + 1):
            for gz in range(int(z0[i]), int(z1[i]) + 1):
                records[gx, gz] += 1
    assert records[sector] == 90 and (records > 64).sum() == 1
    rays = rc.crowded_rays()
    want = oracle.raycast_boxes(*boxes_of(w), *rays)
    own = np.tile(np.arange(90, dtype=U), 2)
    assert (want["hit"][:180] == 1).all() and np.array_equal(want["id"][:180], own)          # every box is asked for by its own rays
    inside = want["position"][90:180]
    assert ((inside > w.bmin[:90] - F(1e-3)) & (inside < w.bmax[:90] + F(1e-3))).all()
    o, d, md, _ = rays
    end = o[90:180] + rc.normalise(d[90:180]) * md[90:180, None]
    assert ((end > w.bmin[:90]) & (end < w.bmax[:90])).all()                                 # the diagonal rays end inside their box
    assert list(want["id"][180:]) == [90] * 4 + [91] * 4                                     # across the crowd to the box behind it
    rect = grid.walk_rect(o[180:], rc.normalise(d[180:]), md[180:])
    assert ((rect[0] <= sector[0]) & (rect[1] >= sector[0]) & (rect[2] <= sector[1]) & (rect[3] >= sector[1])).all()
    sweeps = rc.crowded_sweeps()
    ws = sweep_ref.sweep_boxes(oracle, *boxes_of(w), *sweeps)
    assert (ws["hit"] == 1).all() and len(np.unique(ws["id"])) > 60


def test_the_tie_worlds_tie(oracle):
    worlds = rc.tie_worlds()
    assert [t[0] for t in worlds] == ["bin_big_0", "bin_big_1", "bin_crowd_0", "bin_crowd_1"]
    grid = rc.Grid((0, 0))
    for name, mn, mx, rays, sweeps in worlds:
        n = len(mn)
        group, mask = np.ones(n, U), np.full(n, rc.ALL, U)
        x0, x1, z0, z1, big = grid.plan_bins(mn, mx)
        if name.startswith("bin_big"):
            assert big[0] != big[1] and big.sum() == 1                      # one in a bin, one in the big list
        else:
            assert not big.any()
            crowd = (x0[2] , z0[2])
            in_crowd = lambda i: x0[i] <= crowd[0] <= x1[i] and z0[i] <= crowd[1] <= z1[i]
            assert sum(in_crowd(i) for i in range(n)) == 91 and in_crowd(0) != in_crowd(1)     # one is a record of the crowded sector
            rect = grid.walk_rect(rays[0], rc.normalise(rays[1]), rays[2])
            assert rect[0][0] <= crowd[0] <= rect[1][0] and rect[2][0] <= crowd[1] <= rect[3][0]   # the walk reads that sector
        for q, cast, field in ((rays, oracle.raycast_boxes, "distance"),
                               (sweeps, lambda *a: sweep_ref.sweep_boxes(oracle, *a), "travel")):
            alone = []
            for i in (0, 1):
                g = np.zeros(n, U); g[i] = 1
                r = cast(mn, mx, g, mask, *q)
                assert r["hit"][0] == 1 and r["id"][0] == i
                alone.append(bits(r[field])[0])
            assert alone[0] == alone[1], name                               # the same t to the bit
            both = cast(mn, mx, group, mask, *q)
            assert both["hit"][0] == 1 and both["id"][0] == 0 and bits(both[field])[0] == alone[0]


def test_batch_sizes_leave_waves_without_a_ray():
    rays = rc.ray_batch("near")[2]
    for count in rc.BATCH_SIZES:
        t = rc.tiled(rays, count)
        assert all(len(x) == count for x in t)
    assert [c % 4 for c in rc.BATCH_SIZES] == [1, 3, 0, 1, 1] and max(rc.BATCH_SIZES) > 4096
