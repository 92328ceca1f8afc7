"""The renderer's frame on every end-of-tick path: the case table of tests/test_gpu_frame_paths.py, shared with its CPU twin
tests/test_frame_cases_cpu.py (inputs and claims only: nothing here touches a GPU or the oracle).

A frame is the ordered visible list, the draw items and the read-back block.  Which code writes the items and the block depends on how
the tick ends (scTickGetFrameStats); a row names a world, how its context is created, the read-back sizes, the draw
budget, and a list of ticks -- each with its flags, the actions taken before it, and the PATH IT CLAIMS: (who writes the items, who
stages the block) as capi.FRAME_ITEMS_* / capi.FRAME_BLOCK_*, plus, where the row is about them, whether the tick is a quiet one,
whether the fused kernel's tail owns the dirty words, and the form of the compaction launch.  The GPU test asserts every claim from the
library's host-side reports before it compares a byte, so no row can pass on another path than the one it names.

Sizes may be given relative to the oracle's counts of the very tick they are applied before (tests/frame_ref.py resolves them):
V visible, E emitted under the budget in force, D draws_sorted, S visible entities of the first span (a span boundary's place in the list).

Rows without a read-back run TWIN_TICKS ticks, so that their graph twin captures and replays both tick parities."""
import copy
import dataclasses
import functools

import numpy as np

from sc_gameengine_amd import capi as X
from tests import compact_wide_cases as cw, quiet_ticks_cases as qc, worlds

FULL, XC, D = X.FULL, X.XFORM | X.CULL, X.DRAWS
SORTED = D | X.SORT_DRAWS
BINDS = SORTED | X.BIND_RUNS
NEXT = X.PRODUCE_NEXT
SPLIT = X.SPLIT_PAIRS
# the paths a tick can claim: (who writes the draw items, who stages the block)
EOT_BUFFER = (X.FRAME_ITEMS_EOT_BUFFER, X.FRAME_BLOCK_NONE)
EOT_BLOCK = (X.FRAME_ITEMS_EOT_BLOCK, X.FRAME_BLOCK_EOT)
EMIT_STAGED = (X.FRAME_ITEMS_EMIT_STAGED, X.FRAME_BLOCK_EMIT_STAGED)
EMIT_STAGE = (X.FRAME_ITEMS_EMIT, X.FRAME_BLOCK_STAGE)
EMIT_BUFFER = (X.FRAME_ITEMS_EMIT, X.FRAME_BLOCK_NONE)
SORT_STAGE = (X.FRAME_ITEMS_SORT, X.FRAME_BLOCK_STAGE)
SORT_BUFFER = (X.FRAME_ITEMS_SORT, X.FRAME_BLOCK_NONE)
NONE_STAGE = (X.FRAME_ITEMS_NONE, X.FRAME_BLOCK_STAGE)
NONE_HOST = (X.FRAME_ITEMS_NONE, X.FRAME_BLOCK_HOST)
# the six rows of the issue's table ("who writes the items / the block"), by the name a row's cells use
PATH_CELLS = {"path:eot-buffer": EOT_BUFFER, "path:eot-block": EOT_BLOCK, "path:emit-staged": EMIT_STAGED, "path:emit+stage": EMIT_STAGE,
              "path:sort+stage": SORT_STAGE, "path:none+stage": NONE_STAGE}
# how a tick ends
END_CELLS = ["end:combined", "end:combined-colliders", "end:compact-narrow", "end:compact-wide", "end:split-pairs", "end:tail-owned",
             "end:open-world", "end:produce-next", "end:deep-chain", "end:quiet-after-binning", "end:learn-after-quiet"]
# the cross the table must hold: the writers that can run under each ending.  The end-of-tick role writes only where the run has its pair
# search (never on a compaction launch of its own, a split run or a quiet tick); the staged emission kernel only where it has not; a learn
# tick bins, so it is a combined launch.  A world's ending (tail-owned, open, deep, PRODUCE_NEXT) goes with and without a broadphase: all six.
_PAIRS_NOW = ("path:eot-buffer", "path:eot-block", "path:emit+stage", "path:sort+stage", "path:none+stage")
_ALONE = ("path:emit-staged", "path:emit+stage", "path:sort+stage", "path:none+stage")
_EITHER = tuple(PATH_CELLS)
FEASIBLE = {"end:combined": _PAIRS_NOW, "end:combined-colliders": _PAIRS_NOW, "end:compact-narrow": _ALONE, "end:compact-wide": _ALONE,
            "end:split-pairs": _ALONE, "end:tail-owned": _EITHER, "end:open-world": _EITHER, "end:produce-next": _EITHER, "end:deep-chain": _EITHER,
            "end:quiet-after-binning": _ALONE, "end:learn-after-quiet": _PAIRS_NOW}
BUDGET_CELLS = ["budget:0", "budget:1", "budget:V-1", "budget:V", "budget:V+1", "budget:across-max-draws", "budget:span-boundary"]
CAPACITY_CELLS = ["visible:0", "visible:1", "visible:5", "visible:V-1", "visible:V", "visible:V+1", "draws:0", "draws:1", "draws:E-1", "draws:E",
                  "draws:E+1", "draws:sorted-fewer-than-emitted", "draws:sorted-counts-sorted", "draws:sorted-past-8192"]
EMPTY_CELLS = ["empty:camera-away", "empty:no-mesh", "empty:context"]
SWITCH_CELLS = ["switch:sequence", "switch:readback-resized", "switch:readback-then-binds", "switch:binds-then-readback"]
CELLS = list(PATH_CELLS) + END_CELLS + BUDGET_CELLS + CAPACITY_CELLS + EMPTY_CELLS + SWITCH_CELLS + ["graph-twin"]

DX = np.float32(0.25)
TWIN_TICKS = 5                      # a learn tick, a capture and a replay on either tick parity
MAX_CHAIN = cw.MAX_CHAIN
BIG_N = 20000


@dataclasses.dataclass(frozen=True)
class Tick:
    flags: int
    path: tuple                     # claimed frame_stats()
    pre: tuple = ()                 # actions before the run (frame_ref.OracleSide.before)
    quiet: object = None            # claimed bin_stats()["quiet_last_tick"]; None: the row does not name it
    tail: object = None             # claimed tail_stats()["tail_owned_dirty"]
    compact: object = None          # "wide" / "narrow": claimed form of compact_stats()
    run_pairs: bool = False         # SC_TICK_SPLIT_PAIRS: scTickRunPairs behind the run, a frame taken before and after


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    world: str
    ticks: tuple
    cells: tuple
    spans: int = 4                  # SC_TICK_SPANS at creation
    env: tuple = ()                 # further (name, value) pairs at creation
    broadphase: bool = True
    colliders: bool = False
    max_draws: int = 300            # the draw budget at creation
    readback: object = None         # (max_visible, max_draws) switched on before the first tick; None: off
    producer: object = None         # the frame producer's root nudge (ticks with SC_TICK_PRODUCE_NEXT)
    pipeline: object = None         # scTickSetDrawSortTable
    mesh_count: int = 0
    bind_runs: int = 0
    nothing_visible: bool = False   # the row is about an empty list: exempt from the 70 <= V < n - 70 rule, V == 0 instead

    @property
    def n(self):
        return world(self.world).n

    @property
    def span(self):
        return worlds.compute_span(self.n, self.spans)

    @property
    def bit_exact(self):
        """the items equal the oracle's in every bit (frame_ref.items_mismatch): every world but the synthetic city, whose exact zeros
        carry the sign the device's 3 x 4 products give them"""
        return self.world not in ("static", "dynamic")

    @property
    def has_readback(self):
        return self.readback is not None or any(a[0] == "readback" for t in self.ticks for a in t.pre)

    @staticmethod
    def away_camera(w):
        """turned up at the sky from five far planes above the world: nothing of it is in view"""
        cam = dict(w.camera)
        cam["pos"] = np.array([w.camera["pos"][0], 5000.0, w.camera["pos"][2]], np.float32)
        cam["rot"] = np.array([1.4, 0.4, 0.0], np.float32)
        return cam


# ---- worlds: the ones the earlier tables built, at 2 000 - 4 000 entities ----
PIPELINE = np.array([1, 0, 1, 0xFF, 0, 1], np.uint8)       # material 3 does not exist: its draws are dropped by the sort ...
MESHES = 3                                                  # ... and so are those of mesh 3


def _spread(w, factor):
    """the roots moved apart: no broadphase bin of 64 x 64 m holds more than its 64 records (which record of an overflowing bin keeps a
    remembered slot is settled by the order of arrival on the learn tick: its counters are not reproducible, and not this table's subject)"""
    w.pos[w.parent < 0] *= np.float32(factor)
    return w


@functools.lru_cache(maxsize=None)
def _world(name):
    if name == "static":                                    # config 3's kind: cannot pair, quiet ticks once the slots are learnt
        return qc.world()
    if name == "dynamic":                                   # one dynamic parent per sector: pairs everywhere, never quiet
        w = qc.world()
        qc.make_dynamic(w, qc.dynamic_parents(w.n))
        return w
    if name in ("flat", "flat-no-mesh"):                    # roots only: span-closed at every span
        w = worlds.random_world(3000, seed=57, spread=100.0, p_child=0.0)
        if name == "flat-no-mesh":
            w.has_mesh[:] = 0
        return _spread(w, 4.0)
    if name in ("closed", "open"):                          # ten spans of 256 and a ragged one; "open": one parent link across a boundary
        w = _spread(worlds.span_closed_world(2597, 256, 2, 31), 5.0)
        if name == "open":
            w.parent[256] = 255
        return w
    if name == "deep":                                      # chains of eight: level kernels run behind the fused kernel
        return _spread(worlds.chain_world(8, branches=300), 2.4)
    if name == "big":
        w = worlds.random_world(BIG_N, seed=55, spread=110.0, p_child=0.2)
        w.camera["pos"], w.camera["rot"] = np.float32([0.0, 0.0, 200.0]), np.float32([0.0, 0.0, 0.0])      # from outside
        return w
    raise KeyError(name)


def world(name):
    """a fresh copy (rows change layers)"""
    w = _world(name)
    c = copy.copy(w)
    for f in ("pos", "rot", "scale", "parent", "bmin", "bmax", "has_mesh", "has_bounds", "mesh", "material", "group", "mask"):
        setattr(c, f, np.array(getattr(w, f)))
    c.camera = dict(w.camera)
    return c


def layers(which):
    """(group, mask) of the "static" world's entities under ("layers", which)"""
    w = world("static" if which == "static" else "dynamic")
    return w.group, w.mask


def nudged(flags, path, k, **kw):
    """k ticks, the roots nudged by DX between them"""
    return tuple(Tick(flags, path, pre=(("nudge", DX),) if i else (), **kw) for i in range(k))


RB = (2304, 512)                    # the static / dynamic world: every visible index, more items than the budget of 300
RB_FLAT = (3000, 512)
WIDE = dict(world="flat", broadphase=False, spans=4096)
NARROW = dict(world="flat", broadphase=False, spans=4096, env=(("SC_TICK_VARIANT", "16"),))
SORT = dict(pipeline=PIPELINE, mesh_count=MESHES, bind_runs=64)
SORT_SYNTH = dict(pipeline=np.array([1, 0xFF, 0], np.uint8), mesh_count=1 << 20, bind_runs=64)      # the synthetic city's materials are 0..2: 1 does not exist


def _budget_walk(path, path0):
    """one tick per budget edge, relative to that tick's own V and span boundary; budget 0 takes path0"""
    edges = [("1", "budget:1"), ("V-1", "budget:V-1"), ("V", "budget:V"), ("V+1", "budget:V+1"), ("S-1", "budget:span-boundary"),
             ("S", "budget:span-boundary"), ("S+1", "budget:span-boundary"), (0, "budget:0")]
    ticks = tuple(Tick(None, path0 if b == 0 else path, pre=(("budget", b),)) for b, _ in edges)
    return ticks, tuple(dict.fromkeys(c for _, c in edges))


def _with_flags(ticks, flags):
    return tuple(dataclasses.replace(t, flags=flags) for t in ticks)


def _visible_walk(path, md=512):
    sizes = [(0, "visible:0"), (1, "visible:1"), (5, "visible:5"), ("V-1", "visible:V-1"), ("V", "visible:V"), ("V+1", "visible:V+1")]
    return tuple(Tick(None, path, pre=(("readback", mv, md),)) for mv, _ in sizes), tuple(c for _, c in sizes)


def _cases():
    out = []

    def add(id, ticks, cells, **kw):
        out.append(Case(id=id, ticks=tuple(ticks), cells=tuple(cells), **kw))

    # ---- every writer, crossed with how the tick ends ----
    # the combined end-of-tick launch (compaction and pair search), plain and collider instance
    for tag, col, end in (("", False, "end:combined"), ("-colliders", True, "end:combined-colliders")):
        kw = dict(world="dynamic", colliders=col)
        add("combined%s-buffer" % tag, nudged(FULL | D, EOT_BUFFER, TWIN_TICKS, quiet=False), ["path:eot-buffer", end, "graph-twin"], **kw)
        add("combined%s-block" % tag, nudged(FULL | D, EOT_BLOCK, 3, quiet=False), ["path:eot-block", end], readback=RB, **kw)
        add("combined%s-budget0" % tag, nudged(FULL | D, EMIT_STAGE, 3), ["path:emit+stage", end, "budget:0"], readback=(2304, 2304), max_draws=0, **kw)
        add("combined%s-sorted" % tag, nudged(FULL | BINDS, SORT_STAGE, 3), ["path:sort+stage", end, "draws:sorted-fewer-than-emitted", "draws:sorted-counts-sorted"],
            readback=(2304, 2304), max_draws=0, **SORT_SYNTH, **kw)
        add("combined%s-no-draws" % tag, nudged(FULL, NONE_STAGE, 3), ["path:none+stage", end], readback=RB, **kw)
    add("combined-budget-over", nudged(FULL | D, EMIT_STAGE, 3), ["path:emit+stage", "end:combined"], readback=(2304, 200), world="dynamic")
    # the compaction's own launch: one span per workgroup (k_compact), several (k_compact_wide)
    for tag, how, form, end in (("narrow", NARROW, "narrow", "end:compact-narrow"), ("wide", WIDE, "wide", "end:compact-wide")):
        add(tag + "-staged", nudged(XC | D, EMIT_STAGED, 3, compact=form), ["path:emit-staged", end], readback=RB_FLAT, **how)
        add(tag + "-budget0", nudged(XC | D, EMIT_STAGE, 3, compact=form), ["path:emit+stage", end, "budget:0"], readback=(3000, 3000), max_draws=0, **how)
        add(tag + "-sorted", nudged(XC | BINDS, SORT_STAGE, 3, compact=form), ["path:sort+stage", end, "draws:sorted-fewer-than-emitted"],
            readback=(3000, 3000), max_draws=0, **SORT, **how)
        add(tag + "-no-draws", nudged(XC, NONE_STAGE, 3, compact=form), ["path:none+stage", end], readback=RB_FLAT, **how)
        add(tag + "-buffer", nudged(XC | D, EMIT_BUFFER, TWIN_TICKS, compact=form), [end, "graph-twin"], **how)
    add("wide-sorted-buffer", nudged(XC | BINDS, SORT_BUFFER, TWIN_TICKS, compact="wide"), ["end:compact-wide", "graph-twin"], **SORT, **WIDE)
    # SC_TICK_SPLIT_PAIRS: the compact+pack launch, scTickRunPairs behind it
    add("split-staged", nudged(FULL | SPLIT | D, EMIT_STAGED, 3, run_pairs=True, quiet=False), ["path:emit-staged", "end:split-pairs"], readback=RB, world="dynamic")
    add("split-budget0", nudged(FULL | SPLIT | D, EMIT_STAGE, 3, run_pairs=True), ["path:emit+stage", "end:split-pairs"], readback=(2304, 2304), max_draws=0, world="dynamic")
    add("split-sorted", nudged(FULL | SPLIT | BINDS, SORT_STAGE, 3, run_pairs=True), ["path:sort+stage", "end:split-pairs"], readback=(2304, 2304), max_draws=0,
        world="dynamic", **SORT_SYNTH)
    add("split-no-draws", nudged(FULL | SPLIT, NONE_STAGE, 3, run_pairs=True), ["path:none+stage", "end:split-pairs"], readback=RB, world="dynamic")
    add("split-buffer", nudged(FULL | SPLIT | D, EMIT_BUFFER, TWIN_TICKS, run_pairs=True), ["end:split-pairs", "graph-twin"], world="dynamic")
    # the fused kernel's tail owns the dirty words / a parent link across a span boundary keeps them in compactBody
    for name, owns, end in (("closed", True, "end:tail-owned"), ("open", False, "end:open-world")):
        kw = dict(world=name, spans=4096)
        add(name + "-combined-block", nudged(FULL | D, EOT_BLOCK, 3, tail=owns), ["path:eot-block", end], readback=(2597, 512), **kw)
        add(name + "-combined-buffer", nudged(FULL | D, EOT_BUFFER, TWIN_TICKS, tail=owns), ["path:eot-buffer", end, "graph-twin"], **kw)
        add(name + "-staged", nudged(XC | D, EMIT_STAGED, 3, tail=owns, compact="wide" if owns else "narrow"), ["path:emit-staged", end],
            readback=(2597, 512), broadphase=False, **kw)
        add(name + "-stage", nudged(XC | D, EMIT_STAGE, 3, tail=owns), ["path:emit+stage", end], readback=(2597, 2597), max_draws=0, broadphase=False, **kw)
        add(name + "-sorted", nudged(FULL | BINDS, SORT_STAGE, 3, tail=owns), ["path:sort+stage", end], readback=(2597, 2597), max_draws=0, **SORT, **kw)
        add(name + "-no-draws", nudged(XC, NONE_STAGE, 3, tail=owns), ["path:none+stage", end], readback=(2597, 512), broadphase=False, **kw)
    # SC_TICK_PRODUCE_NEXT: the roots are nudged at the end of the tick whose items are being written
    kw = dict(producer=DX)
    add("produce-combined-block", [Tick(FULL | D | NEXT, EOT_BLOCK)] * 3, ["path:eot-block", "end:produce-next"], readback=RB, world="dynamic", **kw)
    add("produce-combined-buffer", [Tick(FULL | D | NEXT, EOT_BUFFER)] * TWIN_TICKS, ["path:eot-buffer", "end:produce-next", "graph-twin"], world="dynamic", **kw)
    add("produce-wide-staged", [Tick(XC | D | NEXT, EMIT_STAGED, compact="wide", tail=True)] * 3, ["path:emit-staged", "end:produce-next"], readback=RB_FLAT, **WIDE, **kw)
    add("produce-open-staged", [Tick(XC | D | NEXT, EMIT_STAGED, compact="narrow", tail=False)] * 3, ["path:emit-staged", "end:produce-next", "end:open-world"],
        readback=(2597, 512), world="open", spans=4096, broadphase=False, **kw)
    add("produce-wide-stage", [Tick(XC | D | NEXT, EMIT_STAGE, compact="wide")] * 3, ["path:emit+stage", "end:produce-next"], readback=(3000, 3000), max_draws=0, **WIDE, **kw)
    add("produce-wide-sorted", [Tick(XC | BINDS | NEXT, SORT_STAGE, compact="wide")] * 3, ["path:sort+stage", "end:produce-next"], readback=(3000, 3000), max_draws=0,
        **SORT, **WIDE, **kw)
    add("produce-combined-no-draws", [Tick(FULL | NEXT, NONE_STAGE)] * 3, ["path:none+stage", "end:produce-next"], readback=RB, world="dynamic", **kw)
    # deeper than kMaxChain: the level kernels finish matrices and visibility behind the fused kernel
    kw = dict(world="deep")
    add("deep-combined-block", nudged(FULL | D, EOT_BLOCK, 3, tail=False), ["path:eot-block", "end:deep-chain"], readback=(2400, 512), **kw)
    add("deep-staged", nudged(XC | D, EMIT_STAGED, 3, tail=False, compact="narrow"), ["path:emit-staged", "end:deep-chain"], readback=(2400, 512), broadphase=False, **kw)
    add("deep-stage", nudged(XC | D, EMIT_STAGE, 3, tail=False), ["path:emit+stage", "end:deep-chain"], readback=(2400, 2400), max_draws=0, broadphase=False, **kw)
    add("deep-combined-buffer", nudged(FULL | D, EOT_BUFFER, TWIN_TICKS, tail=False), ["path:eot-buffer", "end:deep-chain", "graph-twin"], **kw)
    add("deep-sorted", nudged(XC | BINDS, SORT_STAGE, 3, tail=False), ["path:sort+stage", "end:deep-chain"], readback=(2400, 2400), max_draws=0, broadphase=False, **SORT, **kw)
    add("deep-no-draws", nudged(FULL, NONE_STAGE, 3, tail=False), ["path:none+stage", "end:deep-chain"], readback=(2400, 512), **kw)
    # quiet ticks (config 3's own tick): the learn tick bins, the ticks behind it do not; upload_layers ends the stretch with a learn tick
    P = FULL | D | NEXT
    dyn, sta = (("layers", "dynamic"),), (("layers", "static"),)
    for tag, env, form in (("", (), "wide"), ("-narrow", (("SC_TICK_VARIANT", "16"),), "narrow")):
        add("quiet%s-staged" % tag,
            [Tick(P, EOT_BLOCK, quiet=False), Tick(P, EMIT_STAGED, quiet=True, compact=form), Tick(P, EMIT_STAGED, quiet=True, compact=form),
             Tick(P, EOT_BLOCK, quiet=False, pre=dyn), Tick(P, EOT_BLOCK, quiet=False), Tick(P, EOT_BLOCK, quiet=False, pre=sta),
             Tick(P, EMIT_STAGED, quiet=True, compact=form)],
            ["path:emit-staged", "path:eot-block", "end:quiet-after-binning", "end:learn-after-quiet", "end:produce-next"],
            world="static", readback=RB, producer=qc.DX, env=env)
    add("quiet-stage", [Tick(P, EMIT_STAGE, quiet=False)] + [Tick(P, EMIT_STAGE, quiet=True)] * 2 + [Tick(P, EMIT_STAGE, quiet=False, pre=dyn)],
        ["path:emit+stage", "end:quiet-after-binning", "end:learn-after-quiet"], world="static", readback=(2304, 2304), max_draws=0, producer=qc.DX)
    add("quiet-sorted", [Tick(FULL | BINDS | NEXT, SORT_STAGE, quiet=False)] + [Tick(FULL | BINDS | NEXT, SORT_STAGE, quiet=True)] * 2
        + [Tick(FULL | BINDS | NEXT, SORT_STAGE, quiet=False, pre=dyn)],
        ["path:sort+stage", "end:quiet-after-binning", "end:learn-after-quiet"], world="static", readback=(2304, 2304), max_draws=0, producer=qc.DX, **SORT_SYNTH)
    add("quiet-no-draws", [Tick(FULL | NEXT, NONE_STAGE, quiet=False)] + [Tick(FULL | NEXT, NONE_STAGE, quiet=True)] * 2
        + [Tick(FULL | NEXT, NONE_STAGE, quiet=False, pre=dyn)],
        ["path:none+stage", "end:quiet-after-binning", "end:learn-after-quiet"], world="static", readback=RB, producer=qc.DX)
    add("quiet-buffer", [Tick(P, EOT_BUFFER, quiet=False)] + [Tick(P, EMIT_BUFFER, quiet=True)] * (TWIN_TICKS - 1) + [Tick(P, EOT_BUFFER, quiet=False, pre=dyn)],
        ["path:eot-buffer", "end:quiet-after-binning", "end:learn-after-quiet", "graph-twin"], world="static", producer=qc.DX)

    # ---- budget edges, relative to the very tick's visible count and to a span boundary's place in the list ----
    for tag, path, path0, flags, how, rb in (("combined", EOT_BLOCK, EMIT_STAGE, FULL | D, dict(world="dynamic"), (2304, 2304)),
                                            ("wide", EMIT_STAGED, EMIT_STAGE, XC | D, WIDE, (3000, 3000))):
        ticks, cells = _budget_walk(path, path0)
        add("budget-walk-" + tag, _with_flags(ticks, flags), cells, readback=rb, **how)
        add("budget-across-max-draws-" + tag,
            [Tick(flags, path, pre=(("budget", 200),)), Tick(flags, EMIT_STAGE, pre=(("budget", 400),)), Tick(flags, path, pre=(("budget", 300),)),
             Tick(flags, EMIT_STAGE, pre=(("budget", 301),)), Tick(flags, path, pre=(("budget", 1),))],
            ["budget:across-max-draws"], readback=(rb[0], 300), **how)
    ticks, cells = _budget_walk(EOT_BUFFER, EOT_BUFFER)
    add("budget-walk-buffer", _with_flags(ticks, FULL | D), cells + ("graph-twin",), world="dynamic")

    # ---- block capacities ----
    for tag, path, flags, how, budget in (("combined", EOT_BLOCK, FULL | D, dict(world="dynamic"), 300), ("wide-staged", EMIT_STAGED, XC | D, WIDE, 300),
                                          ("wide-stage", EMIT_STAGE, XC | D, WIDE, 0)):
        ticks, cells = _visible_walk(path)
        add("capacity-visible-" + tag, _with_flags(ticks, flags), cells, max_draws=budget, **how)
    sizes = [(0, "draws:0"), (1, "draws:1"), ("E-1", "draws:E-1"), ("E", "draws:E"), ("E+1", "draws:E+1")]
    add("capacity-draws-stage", [Tick(XC | D, EMIT_STAGE, pre=(("readback", 3000, md),)) for md, _ in sizes], [c for _, c in sizes], max_draws=0, **WIDE)
    # (under a budget the items fit or the path changes: E - 1 items of room send the tick to the emission kernel and the staging kernel)
    for tag, path, flags, how in (("combined", EOT_BLOCK, FULL | D, dict(world="dynamic")), ("wide", EMIT_STAGED, XC | D, WIDE)):
        add("capacity-draws-budget-" + tag,
            [Tick(flags, EMIT_STAGE, pre=(("readback", 64, "E-1"),)), Tick(flags, path, pre=(("readback", 64, "E"),)), Tick(flags, path, pre=(("readback", 64, "E+1"),)),
             Tick(flags, EMIT_STAGE, pre=(("readback", 64, 1),))],
            ["draws:E-1", "draws:E", "draws:E+1", "draws:1"], **how)
    sizes = [(0, "draws:0"), (1, "draws:1"), ("D-1", "draws:sorted-counts-sorted"), ("D", "draws:sorted-counts-sorted"), ("D+1", "draws:sorted-counts-sorted"),
             ("E", "draws:sorted-fewer-than-emitted")]
    add("capacity-draws-sorted", [Tick(XC | BINDS, SORT_STAGE, pre=(("readback", 5, md),)) for md, _ in sizes], dict.fromkeys(c for _, c in sizes), max_draws=0, **SORT, **WIDE)
    add("sorted-past-8192", nudged(XC | BINDS, SORT_STAGE, 2), ["draws:sorted-past-8192", "path:sort+stage"], world="big", broadphase=False, readback=(BIG_N, BIG_N),
        max_draws=0, **SORT)

    # ---- nothing visible, nothing emitted, nothing there ----
    away, main = (("camera", "away"),), (("camera", "main"),)
    city = dict(world="dynamic", broadphase=False)            # (every entity of the city has Bounds: one without is visible from anywhere)
    for tag, path, flags, how, budget, rb in (("combined", EOT_BLOCK, FULL | D, dict(world="dynamic"), 300, RB), ("staged", EMIT_STAGED, XC | D, city, 300, RB),
                                              ("stage", EMIT_STAGE, XC | D, city, 0, RB), ("sorted", SORT_STAGE, XC | BINDS, dict(SORT_SYNTH, **city), 0, RB)):
        add("camera-away-" + tag, [Tick(flags, path, pre=away), Tick(flags, path), Tick(flags, path, pre=main)], ["empty:camera-away"], readback=rb, max_draws=budget,
            nothing_visible=True, **how)
    for tag, path, flags, budget in (("staged", EMIT_STAGED, XC | D, 300), ("stage", EMIT_STAGE, XC | D, 0), ("combined", EOT_BLOCK, FULL | D, 300)):
        add("no-mesh-" + tag, nudged(flags, path, 2), ["empty:no-mesh"], world="flat-no-mesh", spans=4096, broadphase=bool(flags & X.BROADPHASE), readback=RB_FLAT,
            max_draws=budget, nothing_visible=True)
    # the emptied context: every scTickRun ends with a frame -- zeros under the next tick index
    add("emptied-context", [Tick(XC | D, EMIT_STAGED), Tick(XC | D, EMIT_STAGED), Tick(XC | D, NONE_HOST, pre=(("empty",),)), Tick(XC, NONE_HOST), Tick(XC | D, NONE_HOST)],
        ["empty:context"], readback=RB_FLAT, nothing_visible=True, **WIDE)

    # ---- path switches on one context, the host one frame behind ----
    q = dict(quiet=True)
    add("switch-sequence",
        [Tick(P, EOT_BLOCK, quiet=False),                                        # the learn tick: the end-of-tick role writes the block
         Tick(P, EMIT_STAGED, **q), Tick(P, EMIT_STAGED, **q),                   # quiet ticks: the staged emission kernel
         Tick(FULL | BINDS | NEXT, SORT_STAGE, **q), Tick(FULL | BINDS | NEXT, SORT_STAGE, **q),      # sorted with bind runs
         Tick(FULL | NEXT, NONE_STAGE, **q),                                     # a run without SC_TICK_DRAWS
         Tick(P, EMIT_STAGE, pre=(("budget", 600),), **q),                       # budget above max_draws
         Tick(P, EMIT_STAGED, pre=(("budget", 300),), **q),                      # ... and back
         Tick(P, EOT_BLOCK, quiet=False, pre=dyn), Tick(P, EOT_BLOCK, quiet=False),
         Tick(P, EOT_BLOCK, quiet=False, pre=(("readback", 1000, 400),)),       # other sizes in the middle: the tick index restarts
         Tick(P, EOT_BLOCK, quiet=False),
         Tick(FULL | BINDS | NEXT, SORT_STAGE, quiet=False, pre=(("readback", 0, 0), ("bind_runs", 32), ("readback", 2304, 512))),
         Tick(FULL | BINDS | NEXT, SORT_STAGE, quiet=False),
         Tick(FULL | BINDS | NEXT, SORT_STAGE, quiet=False, pre=(("bind_runs", 0), ("readback", 0, 0), ("readback", 2000, 500), ("bind_runs", 48))),
         Tick(P, EOT_BLOCK, quiet=False)],
        SWITCH_CELLS + ["path:eot-block", "path:emit-staged", "path:sort+stage", "path:none+stage", "path:emit+stage"],
        world="static", readback=RB, producer=qc.DX, **SORT_SYNTH)
    return out


CASES = _cases()
CASE_BY_ID = {c.id: c for c in CASES}
assert len(CASE_BY_ID) == len(CASES)


def create_env(case):
    return dict((("SC_TICK_SPANS", str(case.spans)),) + tuple(case.env))


def collider_state(case):
    """the colliders of a row with the collider instance: every type, at random (they shape the broadphase proxies, never the frame)"""
    from tests import collider_ref
    return collider_ref.Colliders.random(case.n, np.random.default_rng(31))
