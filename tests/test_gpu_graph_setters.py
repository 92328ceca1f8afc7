"""Graph replay after every setter (tests/graph_setter_cases.py): two contexts on the same world, an eager twin and a graph twin
(set_graph_mode(True) after the common set-up), ticked side by side.  Between two phases of ticks -- each long enough for both tick
parities to be captured AND replayed -- both get the same setter calls; after EVERY tick every output the case reads must be equal
between the twins, bit for bit.  A third, eager control context gets each step one phase late: on the first tick behind a step the
eager twin must differ from it in the outputs the step names, so a stale replay cannot coincide with a fresh tick.  The graph twin's
learn ticks must not move over the last four ticks of a phase (scTickRun: replay = graphMode && !sampled && !learn -- those ticks were
captures and replays).  Where the oracle states the result, the graph twin's last tick is compared with it as well.

Between all ticks every context gets the same root nudge (or, where a case says so, new positions for a handful of entities)."""
import numpy as np
import pytest

from sc_gameengine_amd import capi, synth_world as sw, tiles
from sc_gameengine_amd.tick import WorldTick, camera_view_proj
from tests import graph_setter_cases as G
from tests import worlds

pytestmark = pytest.mark.gpu


# ---- canonical forms of the outputs ----------------------------------------------------------------------------------------------------
def _keys(p):
    p = np.asarray(p, np.uint32).reshape(-1, 2)
    return p[:, 0].astype(np.uint64) << np.uint64(32) | p[:, 1].astype(np.uint64)


def _fields(a, skip=("pad", "reserved")):
    return {f: a[f].copy() for f in a.dtype.names if f not in skip}


def _counts(t, flags):
    c = t.counts()
    names = ["entities", "max_depth", "unreachable", "relinks"]
    if flags & capi.CULL:
        names += ["renderables_total", "visible", "culled"]
    if flags & capi.BROADPHASE:
        names += ["pairs", "pairs_truncated", "bin_overflow", "big_boxes", "border_lost", "vocabulary_violations"]
    if flags & capi.DRAWS:
        names += ["draws_emitted", "draws_dropped", "draws_sorted"]
    return {k: int(getattr(c, k)) for k in names}


def _pairs(t, flags):
    p, total = t.pairs()
    return np.sort(_keys(p)), total


def _events(triple):
    """begun / ended sorted by pair id; a list cut at max_events holds an unspecified choice of the events: the report alone then"""
    b, e, info = triple
    if info["events_truncated"]:
        return info
    return np.sort(_keys(b)), np.sort(_keys(e)), info


def _pair_shapes(t, flags):
    """the touching list sorted by pair id, and the contact and manifold records -- record i belongs to entry i -- in that order; a list
    cut at max_touching holds an unspecified choice of the touching pairs: the reports alone then"""
    p, info = t.read_pair_shapes()
    out = {"info": info}
    cut = info["touching"] > len(p)
    order = np.argsort(_keys(p), kind="stable")
    if not cut:
        out["touching"] = _keys(p)[order]
    # (the reports of the contacts and manifolds count kinds over the records WRITTEN: of a cut list, only how many were)
    if t.pair_contacts_enabled():
        rec, ci = t.read_pair_contacts()
        out["contact_info"] = ci["written"] if cut else ci
        if not cut:
            out["contacts"] = _fields(rec[order])
    if t.pair_manifolds_enabled():
        rec, mi = t.read_pair_manifolds()
        out["manifold_info"] = mi["written"] if cut else mi
        if not cut:
            out["manifolds"] = _fields(rec[order])
    return out


def _flagged(flag, read):
    """an output of a flagged feature: read only behind a run that carried the flag"""
    return lambda t, flags: read(t) if flags & flag else None


READERS = {
    "world_matrices": lambda t, f: t.world_matrices(),
    "visible": lambda t, f: t.visible(),
    "culled": lambda t, f: t.culled(),
    "counts": _counts,
    "pairs": lambda t, f: _pairs(t, f) if f & capi.BROADPHASE else None,
    "draws": lambda t, f: t.draws(),
    "bind_runs": lambda t, f: (t.bind_runs(), t.material_touches()),
    "ray_hits": _flagged(capi.RAYS, lambda t: _fields(t.ray_hits())),
    "sweep_hits": _flagged(capi.SWEEPS, lambda t: _fields(t.sweep_hits(), skip=())),
    "sweep_shape_info": _flagged(capi.SWEEPS, lambda t: t.sweep_shape_info()),
    "anchored_ray_hits": _flagged(capi.ANCHORED_RAYS, lambda t: _fields(t.anchored_ray_hits())),
    "pair_events": _flagged(capi.PAIR_EVENTS, lambda t: _events(t.pair_events())),
    "touch_events": _flagged(capi.TOUCH_EVENTS, lambda t: _events(t.touch_events())),
    "pair_shapes": lambda t, f: _pair_shapes(t, f),
    "traffic_agents": lambda t, f: t.traffic_agents(),
    "traffic_sensors": lambda t, f: t.traffic_sensors(),
    "traffic_brakes": lambda t, f: t.traffic_brakes(),
    "mover_velocities": lambda t, f: t.mover_velocities(),
}
assert set(n for c in G.CASES for n in c.reads) <= set(READERS)


def read(t, name, flags):
    """an output in its canonical form; a reader the context refuses (a feature that is off: no movers yet, sensors off) reads as its
    error text, which the twins must share like any value -- but a device fault is no refusal: it goes up, and ends the session"""
    try:
        return READERS[name](t, flags)
    except capi.ScTickError as e:
        if _device_fault(e):
            raise
        return ("refused", str(e))


def _device_fault(e):
    return any(text in str(e) for text in ("illegal memory access", "unspecified launch failure", "hipErrorLaunchFailure", "hipErrorIllegalAddress"))


def same(a, b):
    """bit for bit, through tuples, lists and dicts"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    return type(a) is type(b) and a == b


def test_the_comparison_is_bit_for_bit():
    """(needs no device, but belongs with the driver it guards)"""
    z = np.zeros(3, np.float32)
    assert same((z, {"a": 1}), (z.copy(), {"a": 1})) and not same(z, -z) and not same(z, z.astype(np.float64))
    assert not same({"a": 1}, {"a": 2}) and not same((z,), (z, z)) and same(None, None) and not same(None, z)


# ---- one context of a case ---------------------------------------------------------------------------------------------------------------
class Twin:
    def __init__(self, case, graph, label):
        self.case, self.label = case, label
        self.st = st = G.new_state(case.world, graph=graph)
        self.t = t = WorldTick.from_world(st.w, broadphase=case.flow != "A", max_pairs=case.max_pairs)
        t.set_view_proj(st.vp)
        if case.setup:
            case.setup(t, st)
        if case.flow == "P":
            t.set_pipelined(True)
        t.set_profiling(0)
        if graph:
            t.set_graph_mode(True)
        self.ticks = 0
        self.flags = 0
        self.override = None                                # a step's run flags, from that step on

    def apply(self, step):
        step.apply(self.t, self.st)
        if step.flags is not None:
            self.override = G._flow_flags(self.case.flow, step.flags)

    def tick(self):
        case, t, st = self.case, self.t, self.st
        if self.ticks:
            if case.move == "positions":
                st.w.pos[:32, 0] = st.w.pos[:32, 0] + np.float32(case.dx)
                t.upload_positions(0, st.w.pos[:32])
            else:
                G.nudge(t, st, case.dx)
        self.flags = f = case.run_flags(self.ticks) if self.override is None else self.override
        if case.flow == "P":
            t.tile_step(f)
        elif case.flow == "S":
            t.run(f | capi.SPLIT_PAIRS); t.run_pairs()
        else:
            t.run(f)
        self.ticks += 1

    def outputs(self, names):
        return {n: read(self.t, n, self.flags) for n in names}

    def close(self):
        self.t.close()


def _oracle_check(oracle, case, twin):
    """the graph twin's last tick against the oracle, asked afresh about the world as the host mirror has it"""
    t, st = twin.t, twin.st
    assert st.n == st.w.n and not st.freeze and st.frustum_valid, "an oracle check needs a last tick the oracle can restate"
    w = st.w
    ow = worlds.oracle_world(oracle, w, camera=False)
    try:
        ow.transform_system()
        ow.culling_system(view_proj=st.vp)
        what = f"{case.id}: last tick (tick {twin.ticks - 1}), graph twin against the oracle: "
        if "xform" in case.oracle:
            assert np.array_equal(t.world_matrices(), ow.world_matrices()[:w.n]), what + "world_matrices"
        if "visible" in case.oracle:
            assert np.array_equal(t.visible(), ow.visible()), what + "visible"
        if "draws" in case.oracle or "sorted" in case.oracle:
            ent, mesh, mat, model, dropped = ow.draw_items(max_draws=st.budget)
            idx, gmesh, gmat, gmodel = t.draws()
            c = t.counts()
            assert (c.draws_emitted, c.draws_dropped) == (len(ent), dropped), what + "counts (draws_emitted, draws_dropped)"
            if "sorted" in case.oracle:
                order = ow.renderer_draw_order(st.pipeline, st.mesh_count)
                assert c.draws_sorted == len(order), what + "counts (draws_sorted)"
                ent, mesh, mat, model = ent[order], mesh[order], mat[order], model[order]
            assert np.array_equal(idx, ent) and np.array_equal(gmesh, mesh) and np.array_equal(gmat, mat), what + "draws"
            assert np.array_equal(gmodel, model), what + "draws (model matrices)"
        if "rays" in case.oracle or "pairs" in case.oracle:
            mn, mx = ow.world_aabbs()
            mn, mx = mn[:w.n], mx[:w.n]
            if "rays" in case.oracle and (twin.flags & capi.RAYS) and len(st.rays[0]):
                from tests.test_gpu_rays import compare
                compare(t.ray_hits(), oracle.raycast_boxes(mn, mx, w.group, w.mask, *st.rays))
            if "pairs" in case.oracle and (twin.flags & capi.BROADPHASE):
                want = oracle.broadphase_grid(mn, mx, w.group, w.mask, G.CELL)
                got, total = t.pairs()
                assert total == len(want), what + f"pairs ({total} against {len(want)})"
                assert np.array_equal(np.sort(_keys(got)), np.sort(_keys(want))), what + "pairs"
    finally:
        ow.close()


class RunningOracle:
    """An oracle world ticked beside the twins, for results that depend on the run: the frozen visible list, the frame producers, the
    on-rails agents (tests/test_gpu_traffic.py's oracle side) with their speed multiplier, lane activity and front-ray sensors.  It
    follows the graph twin's host mirror (State.freeze, State.extra: producer, mult, lane_events, agents, sensors) and does, per tick,
    what the library's tick does in the library's order: the move, the producer (ahead of the transforms, or behind the tick with
    SC_TICK_PRODUCE_NEXT), transforms, culling, the agents' rays."""

    def __init__(self, oracle, case):
        self.oracle = oracle
        w = self.w = G.world(case.world)
        self.ow = worlds.oracle_world(oracle, w, camera=False)
        self.ol, self.lane_events = None, 0
        agents = getattr(w, "later", None) or {k: getattr(w, k) for k in ("is_agent", "agent_lane", "agent_s", "agent_speed", "agent_mode")}
        if agents["is_agent"] is not None:
            self.ol = oracle.OracleLanes()
            self.ol.build_sectors(w.sector_of[::32, 0], w.sector_of[::32, 1])
            self.is_agent = agents["is_agent"]
            self.a = dict(lane=agents["agent_lane"].copy(), s=agents["agent_s"].copy(), speed=agents["agent_speed"].copy(), mode=agents["agent_mode"].copy(),
                          look=np.full(w.n, 12.0, np.float32))
            self.is_vehicle = (self.is_agent.astype(bool) | (w.mover_kind == 1)).astype(np.uint8)
        self.vel = None if w.mover_vel is None else w.mover_vel.copy()
        self.brake = self.sensed = None

    def _produce(self, st):
        kind, param = st.extra.get("producer", (0, 0.0))
        if kind == 1:
            self.ow.nudge_roots_x(param)
        elif kind == 2:
            if self.ol and st.extra.get("agents", getattr(self.w, "is_agent", None) is not None):
                self.ow.traffic_ai_onrails_braked(self.ol, self.is_agent, self.a["lane"], self.a["s"], self.a["speed"], self.a["mode"], self.a["look"],
                                                  self.brake, param, st.extra.get("mult", 1.0))
            self.ow.advance_movers(self.w.mover_kind, self.vel, self.w.mover_lo, self.w.mover_hi, param)

    def tick(self, twin):
        st, case = twin.st, twin.case
        if twin.ticks > 1:
            self.ow.nudge_roots_x(float(case.dx))
        for ids, active in st.extra.get("lane_events", [])[self.lane_events:]:
            for seg in ids:
                self.ol.set_active(int(seg), active)
        self.lane_events = len(st.extra.get("lane_events", []))
        sensors = st.extra.get("sensors")
        if sensors is None or not sensors["on"]:
            self.brake = self.sensed = None                 # (switched off: every brake is 0 from here on)
        folded = bool(twin.flags & capi.PRODUCE_NEXT)
        if not folded:
            self._produce(st)
        self.ow.transform_system()
        self.ow.culling_system(view_proj=st.vp, freeze=st.freeze)
        if sensors is not None and sensors["on"] and (twin.flags & capi.BROADPHASE):
            mn, mx = self.ow.world_aabbs()
            n = self.w.n
            self.brake, dist, typ = self.ow.traffic_front_ray_sensors(mn[:n], mx[:n], self.w.group, self.w.mask, self.is_agent, self.a["mode"], self.is_vehicle,
                                                                      sensors["ray"], sensors["safe"])
            self.sensed = (dist, typ)
        if folded:
            self._produce(st)

    def check(self, twin, what):
        t, n = twin.t, self.w.n
        bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
        assert np.array_equal(t.world_matrices(), self.ow.world_matrices()[:n]), what + "world_matrices"
        assert np.array_equal(t.visible(), self.ow.visible()), what + ("visible (frozen)" if twin.st.freeze else "visible")
        assert np.array_equal(bits(t.positions()), bits(self.ow.local_positions()[:n])), what + "positions"
        if self.ol and twin.st.extra.get("agents", getattr(self.w, "is_agent", None) is not None):
            ln, ls, sp, md = t.traffic_agents()
            a = self.is_agent.astype(bool)
            assert np.array_equal(ln[a], self.a["lane"][a]) and np.array_equal(md[a], self.a["mode"][a]), what + "traffic_agents (lane, mode)"
            assert np.array_equal(bits(ls[a]), bits(self.a["s"][a])) and np.array_equal(bits(sp[a]), bits(self.a["speed"][a])), what + "traffic_agents (s, speed)"
            if self.sensed is not None:
                onr = a & (self.a["mode"] == 2)
                gd, gt = t.traffic_sensors()
                assert np.array_equal(bits(t.traffic_brakes()[onr]), bits(self.brake[onr])), what + "traffic_brakes"
                assert np.array_equal(bits(gd[onr]), bits(self.sensed[0][onr])) and np.array_equal(gt[onr], self.sensed[1][onr]), what + "traffic_sensors"

    def close(self):
        self.ow.close()
        if self.ol:
            self.ol.close()


def run_case(case, oracle=None):
    eager, graph, control = Twin(case, False, "eager"), Twin(case, True, "graph"), Twin(case, False, "control")
    twins = (eager, graph, control)
    running = RunningOracle(oracle, case) if "running" in case.oracle else None
    try:
        phases = [(None, G.TICKS_BEFORE[case.flow])] + [(s, G.TICKS_AFTER[case.flow]) for s in case.steps]
        for k, (step, ticks) in enumerate(phases):
            if step is not None:
                eager.apply(step)
                graph.apply(step)
                if k >= 2:
                    control.apply(case.steps[k - 2])                          # the control is one step behind
            learnt = []
            for j in range(ticks):
                for tw in twins:
                    tw.tick()
                if running:
                    running.tick(graph)
                what = f"{case.id}: phase {k} ({step.name if step else 'before any step'}), tick {j} of the phase (tick {eager.ticks - 1})"
                a, b = eager.outputs(case.reads), graph.outputs(case.reads)
                for name in case.reads:
                    if not same(a[name], b[name]):
                        # (before any step the control is a second eager twin: if it differs too, the output is not a function of the inputs)
                        also = "" if step is not None or same(a[name], control.outputs((name,))[name]) else " -- and so does a second EAGER context's"
                        diff = ""
                        if name == "counts":
                            diff = ": " + ", ".join(f"{f} {b[name][f]} against {a[name][f]}" for f in a[name] if a[name][f] != b[name][f])
                        pytest.fail(f"{what}: {name} of the graph twin differs from the eager twin's{also}{diff}")
                if step is not None and j == step.effect_tick and step.effect != G.NO_EFFECT:
                    if step.count:
                        x, y = a["counts"][step.count], control.outputs(("counts",))["counts"][step.count]
                        assert x != y, f"{what}: the step has no effect: counts.{step.count} is {x} with it and without it"
                    else:
                        names = step.effect or case.reads
                        c = control.outputs(names)
                        assert any(not same(a[n], c[n]) for n in names), f"{what}: the step has no effect on any of {names}"
                learnt.append(graph.t.learn_ticks())
                if case.flow == "Q" and step is None and j == ticks - 1:
                    assert graph.t.bin_stats()["quiet_last_tick"], f"{what}: a quiet tick was expected of this world"
            if running:
                running.check(graph, f"{case.id}: phase {k} ({step.name if step else 'before any step'}), its last tick (tick {graph.ticks - 1}), graph twin against the oracle: ")
            last = learnt[-min(5, len(learnt)):]
            assert last[0] == last[-1], f"{case.id}: phase {k}: learn ticks moved over the last ticks of the phase ({learnt}): they were not all captures and replays"
        if case.oracle and not running:
            _oracle_check(oracle, case, graph)
    finally:
        for tw in twins:
            tw.close()
        if running:
            running.close()


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_setter_between_replays(oracle, case):
    try:
        run_case(case, oracle)
    except capi.ScTickError as e:
        if _device_fault(e):
            pytest.exit(f"{case.id}: the device faulted ({e}): nothing more is started on it", returncode=3)
        raise


# ---- caller-owned border buffers re-bound between replays --------------------------------------------------------------------------------
def _two_tile_world():
    """a 2 x 1 world as tests/test_gpu_tiles.py builds it: dynamic props on both sides of the shared edge"""
    S, grid = (6, 6), (2, 1)
    w = sw.generate(S[0] * grid[0], S[1] * grid[1], 15, tiles=grid)
    rng = np.random.default_rng(7)
    dyn = rng.random(w.n) < 0.3
    w.group[dyn], w.mask[dyn] = sw.GROUP_DYNAMIC, sw.MASK_ALL
    roots = np.flatnonzero((w.parent < 0) & (np.arange(w.n) % 16 != 0))
    edge = rng.choice(roots, len(roots) // 6, replace=False)
    w.pos[edge, 0] = (64.0 * S[0] + rng.uniform(-3.0, 3.0, len(edge))).astype(np.float32)
    w.group[edge], w.mask[edge] = sw.GROUP_DYNAMIC, sw.MASK_ALL
    return w, grid, S


class _Tiles:
    """the tiles of a split world as contexts of one flow (all eager or all in graph mode), with caller-owned message tensors"""

    def __init__(self, parts, grid, graph, per_parity):
        import torch
        self.torch, self.grid, self.per_parity = torch, grid, per_parity
        self.ticks = [WorldTick.from_world(p, broadphase=True, max_pairs=1 << 16) for p in parts]
        self.kept = []                                      # every tensor ever bound stays referenced until close()
        for r, t in enumerate(self.ticks):
            t.set_tile(r, tiles.neighbour_mask(r, grid))
            t.set_tile_grid(*tiles.tile_of(r, grid), grid[0], grid[1])
        self.bind()
        if graph:
            for t in self.ticks:
                t.set_graph_mode(True)

    def bind(self):
        """NEW tensors for every direction of every tile: one set for all parities (bind_border), or one per parity (bind_border_parity:
        parity 0's carries the messages of an in-order tile, parity 1's is bound and never used)"""
        torch = self.torch
        self.sets = []
        for r, t in enumerate(self.ticks):
            per_tile = []
            for q in range(2 if self.per_parity else 1):
                send = {d: torch.zeros(t.border_bytes(d) // 4, dtype=torch.int32, device="cuda") for d in tiles.neighbours(r, self.grid)}
                recv = {d: torch.zeros(t.border_bytes(d) // 4, dtype=torch.int32, device="cuda") for d in tiles.neighbours(r, self.grid)}
                for d in send:
                    if self.per_parity:
                        t.bind_border_parity(q, d, send[d].data_ptr(), recv[d].data_ptr())
                    else:
                        t.bind_border(d, send[d].data_ptr(), recv[d].data_ptr())
                per_tile.append((send, recv))
            self.sets.append(per_tile)
        self.kept.append(self.sets)

    def step(self, k, nudge):
        """one split step of every tile; returns the send tensors the step's messages must be in"""
        torch = self.torch
        q = 0                                               # (an in-order tile works on set 0 whatever its tick parity: stateFor)
        for t in self.ticks:
            if k:
                t.nudge_roots_x(nudge)
            t.run(capi.XFORM | capi.BROADPHASE | capi.SPLIT_PAIRS)
        for t in self.ticks:
            t.sync()
        for r in range(len(self.ticks)):
            for d, nb in tiles.neighbours(r, self.grid).items():
                self.sets[nb][q][1][7 - d].copy_(self.sets[r][q][0][d])
        torch.cuda.synchronize()
        for t in self.ticks:
            t.run_pairs()
        return [self.sets[r][q][0] for r in range(len(self.ticks))]

    def pair_keys(self, n):
        got = []
        for t in self.ticks:
            p, total = t.pairs()
            assert total == len(p)
            got.append(tiles.global_pair_ids(p, n))
        got = np.concatenate(got).astype(np.uint64)
        return np.sort(np.minimum(got[:, 0], got[:, 1]) << np.uint64(32) | np.maximum(got[:, 0], got[:, 1]))

    def close(self):
        for t in self.ticks:
            t.close()


def _message(tensor):
    """a message as a multiset of words (the order of the records in a cell's slots is not specified)"""
    return np.sort(tensor.cpu().numpy())


@pytest.mark.parametrize("per_parity", [False, True], ids=["border_rebind-S", "border_rebind_parity-S"])
def test_border_rebind(oracle, per_parity):
    """Flow S in graph mode on a 2 x 1 world: after the first phase every direction of both tiles is bound to NEW tensors (the old ones
    stay alive: a stale graph then shows as a wrong pair set and never touches freed memory).  The tiles' pair sets stay equal to the
    eager twins' and to the whole-world oracle's, and the new send tensors carry the tick's message."""
    from tests.test_gpu_tiles import split_world
    w, grid, S = _two_tile_world()
    parts, n = split_world(w, grid, S)
    ow = worlds.oracle_world(oracle, w, camera=False)
    eager, graph = _Tiles(parts, grid, False, per_parity), _Tiles(parts, grid, True, per_parity)
    nudge, k = 0.9, 0
    try:
        for phase in range(3):
            if phase:
                eager.bind(); graph.bind()
            learnt = []
            for j in range(G.TICKS_BEFORE["S"] if phase == 0 else G.TICKS_AFTER["S"]):
                if k:
                    ow.nudge_roots_x(nudge)
                ow.transform_system()
                mn, mx = ow.world_aabbs()
                want = oracle.broadphase_grid(mn, mx, w.group, w.mask, G.CELL)
                wkey = np.sort(want[:, 0].astype(np.uint64) << np.uint64(32) | want[:, 1].astype(np.uint64))
                se, sg = eager.step(k, nudge), graph.step(k, nudge)
                what = f"border_rebind{'_parity' if per_parity else ''}-S: phase {phase} ({'new tensors bound' if phase else 'before any step'}), tick {j} of the phase (tick {k})"
                ke, kg = eager.pair_keys(n), graph.pair_keys(n)
                assert np.array_equal(ke, wkey), f"{what}: pairs of the eager tiles differ from the oracle's ({len(ke)} against {len(wkey)})"
                assert np.array_equal(kg, ke), f"{what}: pairs of the graph tiles differ from the eager tiles' ({len(kg)} against {len(ke)})"
                crossing = (want[:, 0] // n) != (want[:, 1] // n)
                assert crossing.sum() > 5, f"{what}: no pairs across the edge: the messages would not matter"
                for r in range(len(parts)):
                    for d in se[r]:
                        me, mg = _message(se[r][d]), _message(sg[r][d])
                        assert me.any(), f"{what}: the eager tile {r} sent an empty message in direction {d}"
                        assert np.array_equal(mg, me), f"{what}: send buffer of graph tile {r}, direction {d}, does not carry the tick's message"
                learnt.append([t.learn_ticks() for t in graph.ticks])
                k += 1
            assert learnt[-5] == learnt[-1], f"phase {phase}: learn ticks moved over the last four ticks ({learnt})"
    finally:
        eager.close(); graph.close(); ow.close()


@pytest.mark.timeout(300)
def test_border_rebind_parity_pipelined_loopback():
    """Flow P with neighbours: the centre tile of tests/test_gpu_comm.py over the one-rank loop-back communicator, pipelined, each half of
    a step a graph of its own.  After the first phase every (parity, direction) is bound to NEW tensors in place of the library's own
    buffers (which stay allocated).  The pair sets stay equal to the eager twin's, and the new send tensors carry the messages."""
    import torch
    from tests.test_gpu_comm import centre_tile_world, keys, RANK
    w = centre_tile_world()
    vp = camera_view_proj(w.camera)
    depth, flags = 4, capi.FULL
    twins, kept = [], []
    for graph in (False, True):
        t = WorldTick.from_world(w, broadphase=True, max_pairs=1 << 17)
        t.set_view_proj(vp)
        t.set_tile(RANK, 0xFF); t.set_tile_grid(1, 1, 3, 3)
        t.comm_init(capi.comm_unique_id(), 1, 0, peers=[0] * 8)
        t.set_pipelined(depth)
        t.set_graph_mode(graph)
        twins.append(t)
    eager, graph = twins
    k = 0
    try:
        sets = None
        for phase in range(2):
            if phase:
                sets = []
                for t in twins:
                    mine = {}
                    for q in range(depth):
                        for d in range(8):
                            words = t.border_bytes(d) // 4
                            mine[q, d] = (torch.zeros(words, dtype=torch.int32, device="cuda"), torch.zeros(words, dtype=torch.int32, device="cuda"))
                            t.bind_border_parity(q, d, mine[q, d][0].data_ptr(), mine[q, d][1].data_ptr())
                    sets.append(mine)
                kept.append(sets)
            learnt = []
            for j in range(G.TICKS_BEFORE["P"] if phase == 0 else G.TICKS_AFTER["P"] + depth):
                for t in twins:
                    if k:
                        t.nudge_roots_x(0.6)
                    t.tile_step(flags)
                what = f"border_rebind_parity-P: phase {phase} ({'new tensors bound' if phase else 'before any step'}), tick {j} of the phase (tick {k})"
                ke, kg = keys(eager), keys(graph)
                assert len(ke) > 100
                assert np.array_equal(kg, ke), f"{what}: pairs of the graph twin differ from the eager twin's ({len(kg)} against {len(ke)})"
                learnt.append(graph.learn_ticks())
                k += 1
            assert learnt[-5] == learnt[-1], f"phase {phase}: learn ticks moved over the last four ticks ({learnt})"
        for t in twins:
            t.sync()
        for q in range(depth):
            for d in range(8):
                me, mg = _message(sets[0][q, d][0]), _message(sets[1][q, d][0])
                assert me.any(), f"the eager twin's new send buffer (parity {q}, direction {d}) is empty"
                assert np.array_equal(mg, me), f"border_rebind_parity-P: new send buffer (parity {q}, direction {d}) of the graph twin does not carry the message"
    finally:
        for t in twins:
            t.close()
