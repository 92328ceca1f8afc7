"""CPU twin of tests/test_gpu_graph_setters.py: the case table is well-formed, its mutations change what the oracle answers on the chosen
worlds (the driver's non-vacuity condition, checked without a GPU), and every setter of WorldTick is either called by a case or listed
with its reason in NOT_A_TICK_INPUT -- a new setter that is in neither fails here, which is what keeps "a setter called after a
capture reaches the next run" a tested rule and not a convention."""
import inspect

import numpy as np
import pytest

from sc_gameengine_amd import capi, synth_world as sw
from sc_gameengine_amd.tick import WorldTick, camera_view_proj
from tests import graph_setter_cases as G
from tests import worlds


class Recorder:
    """stands in for a WorldTick: records the setters a step calls and checks their arguments against the entity count"""

    def __init__(self, n):
        self.n, self.capacity, self.calls = n, n, []

    def _range(self, first, count):
        assert 0 <= first and count > 0 and first + count <= self.n, f"range {first} + {count} leaves the {self.n} entities"

    def __getattr__(self, name):
        if name.startswith("_") or not hasattr(WorldTick, name):
            raise AttributeError(name)

        def call(*a, **kw):
            self.calls.append((name, a, kw))
            check = getattr(self, "_check_" + name, None)
            if check:
                check(*a, **kw)
            elif name.startswith("upload_"):
                self._range(a[0], len(a[1]))
                assert all(len(x) == len(a[1]) for x in a[2:] if x is not None), f"{name}: arrays of different lengths"
        return call

    def _check_set_count(self, n):
        assert 0 < n <= self.capacity
        self.n = n

    def _check_set_topology(self, parent):
        p = np.asarray(parent)
        assert len(p) == self.n and (p < self.n).all() and (p >= -1).all() and (p != np.arange(self.n)).all()
        assert (worlds.depths(p) >= 0).all(), "a parent cycle"

    def _check_mark_dirty_indices(self, idx):
        assert len(idx) and (np.asarray(idx) < self.n).all()

    def _check_upload_world_matrices(self, first, m):
        self._range(first, len(m))
        m = np.asarray(m)
        assert (m[:, [3, 7, 11]] == 0).all() and (m[:, 15] == 1).all(), "not affine"

    def _check_set_anchored_rays(self, anchor, *arrays, **kw):
        assert (np.asarray(anchor) < self.n).all() and all(len(x) == len(anchor) for x in arrays)

    def _check_set_ray_queries(self, o, d, md, mk):
        assert len(o) == len(d) == len(md) == len(mk)

    def _check_set_sweep_queries(self, a, b, r, hh, mk, skip_id=None):
        assert len(a) == len(b) == len(r) == len(hh) == len(mk)

    def _check_set_draw_sort_table(self, pipeline, mesh_count):
        p = np.asarray(pipeline)
        assert ((p < 128) | (p == 0xFF)).all() and mesh_count >= 0

    def _check_set_lane_active(self, ids, active):
        assert len(ids)

    def names(self):
        return [c[0] for c in self.calls]


def record(case):
    """(names per step, names of the set-up, the states behind every step) of a case run against the recorder"""
    st = G.new_state(case.world)
    r = Recorder(st.w.n)
    if case.setup:
        case.setup(r, st)
    setup, per_step = r.names(), []
    for s in case.steps:
        before = len(r.calls)
        s.apply(r, st)
        per_step.append(r.calls[before:])
    return setup, per_step, st


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_case_is_well_formed(case):
    assert case.flow in "ABQPS" and case.world in G.WORLDS and case.steps and case.reads
    assert bool(case.flags & capi.BROADPHASE) == (case.flow != "A")
    setup, per_step, st = record(case)                       # (the recorder checks every call's arguments)
    for s, calls in zip(case.steps, per_step):
        assert calls or s.name.startswith("set_graph_mode"), f"{s.name} calls nothing"
        assert s.count is None or "counts" in case.reads
        assert s.effect == G.NO_EFFECT or set(s.effect) <= set(case.reads)
    w = G.world(case.world)
    words = np.unique(np.stack([w.group, w.mask], axis=1), axis=0).astype(np.uint64)      # Bullet's filter over the distinct layer words
    can_pair = any((g1 & m2) and (g2 & m1) for g1, m1 in words for g2, m2 in words)
    if case.flow == "Q":
        assert not can_pair, "flow Q needs a world that cannot pair: its broadphase ticks are the quiet ones"
    if case.flow in "BP" and case.world in ("crowd", "colliding"):
        assert can_pair
    if case.oracle:
        assert st.n == st.w.n and not st.freeze and st.frustum_valid, "the last tick must be one the oracle can restate"
        assert not ({"pairs", "rays"} & set(case.oracle)) or "colliders" not in st.extra, "the oracle's boxes are the Bounds boxes"
    if "sorted" in case.oracle:
        assert st.pipeline is not None
    if "rays" in case.oracle:
        assert st.rays is not None


def test_batches_pass_the_first_capacity_and_come_back():
    for name in ("ray_queries", "sweep_queries", "anchored_rays"):
        case = G.CASE_BY_ID[name + "-B"]
        _, per_step, _ = record(case)
        sizes = [len(calls[0][1][0]) for calls in per_step]
        assert sizes == [16, 9, 1500, 0, 16] and max(sizes) > G.BATCH_CAP > 16
    assert G.world("crowd").n == 3000                         # (the anchors' range)


def test_the_deepened_topology_exceeds_the_captured_chain():
    case = G.CASE_BY_ID["topology-A"]
    st = G.new_state(case.world)
    r = Recorder(st.w.n)
    depth = [int(worlds.depths(st.w.parent).max())]
    for s in case.steps:
        s.apply(r, st)
        depth.append(int(worlds.depths(st.w.parent).max()))
    KMAXCHAIN = 3                                              # sc_tick_internal.h: ancestors the fused kernel walks itself
    assert depth == [0, 2, 40, 0] and depth[1] <= KMAXCHAIN < depth[2]


def _oracle_tick(oracle, w, vp, nudges=0, freeze=False, dx=float(G.DX)):
    ow = worlds.oracle_world(oracle, w, camera=False)
    for _ in range(nudges):
        ow.nudge_roots_x(dx)
    ow.transform_system()
    ow.culling_system(view_proj=vp, freeze=freeze)
    return ow


def test_draw_budgets_change_the_oracles_draw_list(oracle):
    """budget rows: 0 -> 100 -> 5000 -> 0 on the plain list needs more than 5 000 visible draws on every tick of the run; the sorted rows
    need more than 8 192 sorted draws without a budget (several workgroups per pass) and fewer with it"""
    for flow in "AB":
        w = G.world(G.CASE_BY_ID["draw_budget_plain-" + flow].world)
        vp = camera_view_proj(w.camera)
        for nudges in (0, 3, 9, 23):
            ow = _oracle_tick(oracle, w, vp, nudges)
            emitted = [len(ow.draw_items(max_draws=b)[0]) for b in (0, 100, 5000, 0)]
            ow.close()
            assert emitted[1] == 100 and emitted[2] == 5000 and emitted[0] > 5000, emitted
        big = G.world(G.CASE_BY_ID["draw_budget_sorted_multi_workgroup-" + flow].world)
        ow = _oracle_tick(oracle, big, camera_view_proj(big.camera), 3)
        ow.draw_items(max_draws=0)
        unlimited = len(ow.renderer_draw_order(G.SORTED_BIG_PIPELINE, G.SORTED_BIG_MESHES))
        ow.draw_items(max_draws=4096)
        limited = len(ow.renderer_draw_order(G.SORTED_BIG_PIPELINE, G.SORTED_BIG_MESHES))
        ow.close()
        assert unlimited > G.SORT_GROUP_KEYS and limited <= 4096 < unlimited


def test_no_sector_of_a_broadphase_world_overflows_its_bin(oracle):
    """a full bin's overflow count is not a function of the inputs (two eager contexts differ in it), so the worlds of the broadphase
    flows stay below 64 boxes per sector over the whole run"""
    for name in sorted({c.world for c in G.CASES if c.flow in "BP" and not c.world.startswith("laned")}):
        w = G.world(name)
        for nudges in (0, 36):
            ow = _oracle_tick(oracle, w, camera_view_proj(w.camera), nudges)
            mn, mx = ow.world_aabbs()
            ow.close()
            box = np.isfinite(mn[:w.n, 0])
            lo = np.floor(np.stack([mn[:w.n][box][:, 0], mn[:w.n][box][:, 2]], axis=1) / 64.0).astype(np.int64)
            hi = np.floor(np.stack([mx[:w.n][box][:, 0], mx[:w.n][box][:, 2]], axis=1) / 64.0).astype(np.int64)
            small = ((hi - lo) <= 1).all(axis=1)                        # (boxes wider than 2 x 2 sectors go to the big list, not into bins)
            lo, hi = lo[small], hi[small]
            who = np.arange(len(lo))
            cells = np.unique(np.concatenate([np.stack([who, x, z], axis=1) for x in (lo[:, 0], hi[:, 0]) for z in (lo[:, 1], hi[:, 1])]), axis=0)
            _, per = np.unique(cells[:, 1:], axis=0, return_counts=True)
            assert per.max() < 64, f"{name}: a sector touched by {per.max()} boxes"


def test_sort_tables_and_meshes_change_the_oracles_order(oracle):
    case = G.CASE_BY_ID["draw_sort_table-A"]
    st = G.new_state(case.world)
    r = Recorder(st.w.n)
    case.setup(r, st)
    ow = _oracle_tick(oracle, st.w, st.vp, 3)
    ow.draw_items(max_draws=0)
    orders = [ow.renderer_draw_order(st.pipeline, st.mesh_count)]
    passes = []
    for s in case.steps:
        s.apply(r, st)
        orders.append(ow.renderer_draw_order(st.pipeline, st.mesh_count))
        passes.append((len(st.pipeline), st.mesh_count))
    ow.close()
    assert not np.array_equal(orders[0], orders[1]) and not np.array_equal(orders[1], orders[2])
    assert passes[0] == (6, G.SMALL_MESHES) and passes[1][0] > 256 and passes[1][1] > 256        # the second table adds a key byte to both handles


def test_freeze_and_cameras_change_the_oracles_visible_list(oracle):
    case = G.CASE_BY_ID["freeze_culling-Q"]
    w = G.world(case.world)
    vp = camera_view_proj(w.camera)
    # (the frozen list is the one of the last tick before the step; the first tick behind it -- and behind the un-freeze, the first fresh one --
    #  must show another: ticks 4 | 5 and 10 | 11 of flow Q, 2 | 3 and 5 | 6 of flow A)
    lists = [_oracle_tick(oracle, w, vp, k, dx=case.dx) for k in range(12)]
    for k in (2, 4, 5, 10):
        assert not np.array_equal(lists[k].visible(), lists[k + 1].visible()), "a frozen list would equal the next tick's"
    for ow in lists:
        ow.close()
    a, b = _oracle_tick(oracle, w, vp, 3), _oracle_tick(oracle, w, vp, 4)
    c = _oracle_tick(oracle, w, camera_view_proj(G.OTHER_CAMERA), 3)
    assert not np.array_equal(a.visible(), c.visible()) and len(c.visible()) > 10
    for ow in (a, b, c):
        ow.close()


def test_ray_batches_hit_and_layers_flip_the_pair_set(oracle):
    w = G.world("crowd")
    ow = _oracle_tick(oracle, w, camera_view_proj(w.camera), 5)
    mn, mx = ow.world_aabbs()
    ow.close()
    hits = [oracle.raycast_boxes(mn, mx, w.group, w.mask, *G._rays(seed, k)) for seed, k in ((1, 16), (2, 16), (3, 9), (4, 1500))]
    assert all((h["hit"] == 1).any() for h in hits)
    assert not np.array_equal(hits[0]["id"], hits[1]["id"])
    w = G.world("colliding")
    ow = _oracle_tick(oracle, w, camera_view_proj(w.camera), 5)
    mn, mx = ow.world_aabbs()
    ow.close()
    own = len(oracle.broadphase_grid(mn, mx, w.group, w.mask, G.CELL))
    static = len(oracle.broadphase_grid(mn, mx, np.full(w.n, sw.GROUP_STATIC, np.uint32), np.full(w.n, sw.MASK_STATIC, np.uint32), G.CELL))
    dynamic = len(oracle.broadphase_grid(mn, mx, np.full(w.n, sw.GROUP_DYNAMIC, np.uint32), np.full(w.n, sw.MASK_ALL, np.uint32), G.CELL))
    assert static == 0 < own < dynamic and own > 100          # worldCanPair flips both ways: sweepOnly on, off, off with more pairs


def test_the_other_lane_graph_is_another_graph():
    w = G.world("laned")
    assert (np.asarray(w.lane_graph.seg_speed_limit) != np.float32(3.0)).any() and len(w.lane_graph.seg_length) > 2
    bare = G.world("laned_bare")
    assert bare.is_agent is None and bare.lane_graph is None and bare.later["is_agent"].any() and bare.mover_kind is not None


def test_every_setter_is_named_by_a_case_or_listed_with_a_reason():
    setters = {n for n, f in inspect.getmembers(WorldTick, inspect.isfunction) if n.split("_")[0] in ("set", "upload", "bind")}
    named = set()
    for case in G.CASES:
        setup, per_step, _ = record(case)
        named |= {c[0] for calls in per_step for c in calls}
        if any(s.name.startswith("set_graph_mode") for s in case.steps):
            named.add("set_graph_mode")
    for names in G.BORDER_CASES.values():
        named |= set(names)
    named &= setters
    listed = set(G.NOT_A_TICK_INPUT)
    assert listed <= setters, f"not setters of WorldTick: {sorted(listed - setters)}"
    assert not (named & listed), f"both named by a case and listed: {sorted(named & listed)}"
    missing = setters - named - listed
    assert not missing, (f"{sorted(missing)}: called by no step of tests/graph_setter_cases.py and not in NOT_A_TICK_INPUT -- a setter that a tick "
                         "reads needs a case (does a captured graph see the change?), any other a one-line reason")
    assert all(len(reason) > 20 for reason in G.NOT_A_TICK_INPUT.values())


def test_the_safe_subset_names_cases_that_exist():
    ids = set(G.CASE_BY_ID) | set(G.BORDER_CASES)
    assert set(G.SAFE_AT_PARENT) <= ids
    assert all(G.CASE_BY_ID[i].graph_safe_at_parent for i in G.SAFE_AT_PARENT if i in G.CASE_BY_ID)
