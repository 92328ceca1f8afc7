"""ctypes binding of libsc_tick.so -- exactly the symbols include/sc_tick.h declares.

There is no CPU fallback: if the HIP library is missing or no AMD GPU is present, loading or
context creation raises.  Nothing in this package imports oracle/.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SC_TICK_LIB") or os.path.join(HERE, "libsc_tick.so")      # SC_TICK_LIB: A/B builds (tools/)

# scTickRun flags (include/sc_tick.h)
XFORM, CULL, BROADPHASE, CULLED_LIST, DRAWS, DENSE_AABBS, SPLIT_PAIRS, SORT_DRAWS, RAYS, PRODUCE_NEXT = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
SWEEPS = 1 << 10
ANCHORED_RAYS = 1 << 11
PAIR_EVENTS = 1 << 12         # SC_TICK_PAIR_EVENTS: which pairs begun / ended since the last run with this flag (scTickSetPairEvents)
BIND_RUNS = 1 << 13           # SC_TICK_BIND_RUNS: with DRAWS | SORT_DRAWS, the bind runs of the sorted list and the material touch set (scTickSetBindRuns)
PAIR_SHAPES = 1 << 14         # SC_TICK_PAIR_SHAPES: also list the pairs of this tick whose collider shapes overlap (scTickSetPairShapes)
TOUCH_EVENTS = 1 << 15        # SC_TICK_TOUCH_EVENTS: which pairs begun / ended TOUCHING since the last run with this flag (scTickSetTouchEvents)
OVERLAPS = 1 << 16            # SC_TICK_OVERLAPS: answer the overlap queries set by scTickSetOverlapQueries against this tick's boxes
TRIGGERS = 1 << 17            # SC_TICK_TRIGGERS: answer the trigger volumes (scTickSetTriggerVolumes) and report who entered / left since the last run with it
ANCHORED_SWEEPS = 1 << 18     # SC_TICK_ANCHORED_SWEEPS: answer the entity-anchored capsule sweeps (scTickSetAnchoredSweeps) against this tick's matrices and boxes
ANCHOR_NONE, ANCHOR_DEAD = 0xFFFFFFFF, 0xFFFFFFFE      # SC_TICK_ANCHOR_*: a world-space ray; a ray whose anchor was removed
RAY_SHAPES_AABB, RAY_SHAPES_EXACT = 0, 1               # SC_TICK_RAY_SHAPES_*: what a ray's candidates are (scTickSetRayShapes)
SWEEP_SHAPES_AABB, SWEEP_SHAPES_EXACT = 0, 1           # SC_TICK_SWEEP_SHAPES_*: what a capsule sweep's candidates are (scTickSetSweepShapes)
OVERLAP_SHAPES_AABB, OVERLAP_SHAPES_EXACT = 0, 1       # SC_TICK_OVERLAP_SHAPES_*: what an overlap query's hits are (scTickSetOverlapQueries)
# SC_TICK_CONTACT_*: ScTickPairContact::kind (scTickSetPairContacts)
CONTACT_NONE, CONTACT_ROUND_ROUND, CONTACT_ROUND_BOX, CONTACT_BOX_FACE_A, CONTACT_BOX_FACE_B, CONTACT_BOX_EDGE = 0, 1, 2, 3, 4, 5
CONTACT_DEEP, CONTACT_DEGENERATE = 1 << 8, 1 << 9
# SC_TICK_MANIFOLD_*: ScTickPairManifold::kind (scTickSetPairManifolds)
MANIFOLD_NONE, MANIFOLD_SINGLE, MANIFOLD_SEGMENT, MANIFOLD_FACE = 0, 1, 2, 3
MANIFOLD_REDUCED = 1 << 8
PERSIST_NONE = 0xFFFFFFFF     # SC_TICK_PERSIST_NONE: ScTickPairPersist::prev_entry of a pair that is not remembered (scTickSetPairPersistence)
SLEEP_ASLEEP, SLEEP_STILL, SLEEP_MOVABLE = 1 << 8, 1 << 9, 1 << 10      # SC_TICK_SLEEP_*: bits of a state word above its rest count (scTickSetPairSleep)
SLEEP_INFO_RESYNC, SLEEP_INFO_FELL_OVERFLOW, SLEEP_INFO_WOKE_OVERFLOW, SLEEP_INFO_LIST_TRUNCATED = 1, 2, 4, 8      # SC_TICK_SLEEP_INFO_*: ScTickPairSleepInfo::flags
ISLAND_NONE = 0xFFFFFFFF      # SC_TICK_ISLAND_NONE: the label of a fixed entity, the island of an entry with no movable member (scTickSetPairIslands)
SWEEP_END_LOCAL, SWEEP_END_WORLD_OFFSET = 0, 1         # SC_TICK_SWEEP_END_*: what an anchored sweep's local_end is (scTickSetAnchoredSweeps)
ASWEEP_ANSWERED, ASWEEP_NO_ANCHOR, ASWEEP_NOT_FINITE = 0, 1, 2      # SC_TICK_ASWEEP_*: ScTickSweepHit::pad of an anchored sweep
TRIGGER_MAX_MEMBERS = 1024    # SC_TICK_TRIGGER_MAX_MEMBERS: id slots per trigger volume at most
SWEEP_SHAPES_TOL, SWEEP_SHAPES_STEPS, SWEEP_SHAPES_SEEN = 1e-3, 12, 256
FULL = XFORM | CULL | BROADPHASE
K_XFORM_CULL, K_COMPACT, K_PAIRS, K_NUDGE, K_COUNT = 0, 1, 2, 3, 4
BIN_LAZY, BIN_STAY, BIN_SWEEP_ONLY, BIN_QUIET = 1, 2, 4, 8     # scTickGetBinStats stats[2]: what the last tick did with the bins (BIN_QUIET: nothing at all)
# scTickGetFrameStats: who wrote the last tick's draw items (SC_TICK_FRAME_ITEMS_*) / staged its read-back block (SC_TICK_FRAME_BLOCK_*)
FRAME_ITEMS_NONE, FRAME_ITEMS_EOT_BUFFER, FRAME_ITEMS_EOT_BLOCK, FRAME_ITEMS_EMIT, FRAME_ITEMS_EMIT_STAGED, FRAME_ITEMS_SORT = 0, 1, 2, 3, 4, 5
FRAME_BLOCK_NONE, FRAME_BLOCK_EOT, FRAME_BLOCK_EMIT_STAGED, FRAME_BLOCK_STAGE, FRAME_BLOCK_HOST = 0, 1, 2, 3, 4
NO_PARENT = -1
# collider types (SC_TICK_COLLIDER_*): what an entity's broadphase proxy is formed from
COLLIDER_BOUNDS, COLLIDER_NONE, COLLIDER_BOX, COLLIDER_SPHERE, COLLIDER_CAPSULE = 0, 1, 2, 3, 4
COMM_ID_BYTES = 128
HAVE_PAIR_SEARCH = True       # flipped when the broadphase pair kernels are in the library

F32P = C.POINTER(C.c_float)
U32P = C.POINTER(C.c_uint32)
I32P = C.POINTER(C.c_int32)
U8P = C.POINTER(C.c_uint8)
U64P = C.POINTER(C.c_uint64)


class ContextDesc(C.Structure):
    _fields_ = [("device_ordinal", C.c_int32), ("capacity", C.c_uint32),
                ("tile_origin_x", C.c_int32), ("tile_origin_z", C.c_int32),
                ("tile_sectors_x", C.c_uint32), ("tile_sectors_z", C.c_uint32),
                ("sector_size", C.c_float), ("max_pairs", C.c_uint32),
                ("max_draws_budget", C.c_uint32), ("reserved", C.c_uint32)]


class Counts(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "entities", "renderables_total", "visible", "culled", "pairs", "pairs_truncated",
        "draws_emitted", "draws_dropped", "max_depth", "unreachable", "bin_overflow", "big_boxes", "draws_sorted", "border_lost", "relinks",
        "vocabulary_violations")]


class DrawItem(C.Structure):
    _fields_ = [("dense_index", C.c_uint32), ("mesh_id", C.c_uint32), ("material_id", C.c_uint32),
                ("pad", C.c_uint32), ("model", C.c_float * 16)]


class RayHit(C.Structure):
    _fields_ = [("hit", C.c_uint32), ("id", C.c_uint32), ("distance", C.c_float), ("position", C.c_float * 3),
                ("normal", C.c_float * 3), ("layer", C.c_uint32), ("pad", C.c_uint32 * 2)]


class SweepHit(C.Structure):
    _fields_ = [("hit", C.c_uint32), ("id", C.c_uint32), ("distance", C.c_float), ("position", C.c_float * 3),
                ("normal", C.c_float * 3), ("layer", C.c_uint32), ("travel", C.c_float), ("pad", C.c_uint32)]


class PairEventInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("begun", "ended", "tracked", "resync", "overflow", "events_truncated")]


class TouchEventInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("begun", "ended", "tracked", "resync", "overflow", "events_truncated")]


class SweepShapeInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("refined", "kept_as_boxes", "exhausted", "pad")]


class OverlapInfo(C.Structure):                          # ScTickOverlapInfo: 32 bytes
    _fields_ = [(n, C.c_uint32) for n in ("queries", "max_hits", "hits", "truncated_queries", "refined", "kept_as_boxes", "shapes", "pad")]


class TriggerInfo(C.Structure):                          # ScTickTriggerInfo: 32 bytes
    _fields_ = [(n, C.c_uint32) for n in ("volumes", "max_members", "members", "entered", "exited", "resync_volumes", "overflow_volumes",
                                          "events_truncated")]


class PairShapeInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("tested", "touching", "refined", "kept_as_boxes", "truncated", "pairs_truncated")]


class PairContact(C.Structure):                          # ScTickPairContact: 32 bytes
    _fields_ = [("point", C.c_float * 3), ("depth", C.c_float), ("normal", C.c_float * 3), ("kind", C.c_uint32)]


class PairContactInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("written", "round_round", "round_box", "box_box", "unrefined", "deep", "degenerate", "reserved")]


class PairManifold(C.Structure):                         # ScTickPairManifold: 80 bytes
    _fields_ = [("point", (C.c_float * 3) * 4), ("depth", C.c_float * 4), ("count", C.c_uint32), ("kind", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class PairManifoldInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("written", "points", "with_one", "with_two", "with_three", "with_four", "face", "reduced")]


class PairIslandInfo(C.Structure):                       # ScTickPairIslandInfo: 32 bytes
    _fields_ = [(n, C.c_uint32) for n in ("edges", "linking", "anchored", "islands", "bodies", "movable", "list_truncated", "gave_up")]


class PairPersist(C.Structure):                          # ScTickPairPersist: 16 bytes
    _fields_ = [("prev_entry", C.c_uint32), ("prev_slot", C.c_uint8 * 4), ("age", C.c_uint8 * 4), ("reserved", C.c_uint32)]


class PairPersistInfo(C.Structure):                      # ScTickPairPersistInfo: 32 bytes
    _fields_ = [(n, C.c_uint32) for n in ("written", "kept_pairs", "new_pairs", "kept_points", "new_points", "resync", "list_truncated", "gave_up")]


class PairSleepInfo(C.Structure):                        # ScTickPairSleepInfo: 32 bytes
    _fields_ = [(n, C.c_uint32) for n in ("flags", "asleep", "islands_asleep", "fell_asleep", "woke", "awake_entries", "epoch", "pad")]


class Frame(C.Structure):
    _fields_ = [("tick", C.c_uint64), ("renderables_total", C.c_uint32), ("visible", C.c_uint32), ("culled", C.c_uint32),
                ("draws_emitted", C.c_uint32), ("draws_dropped", C.c_uint32), ("draws_sorted", C.c_uint32),
                ("visible_in_buffer", C.c_uint32), ("draws_in_buffer", C.c_uint32),
                ("visible_indices", U32P), ("draws", C.POINTER(DrawItem))]


class BindRun(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("first", "count", "pipeline", "material", "mesh", "binds")]


class BindInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("runs", "runs_truncated", "draws", "pipeline_binds", "material_binds", "mesh_binds",
                                          "materials_touched", "touch_words")]


class FrameBinds(C.Structure):
    _fields_ = [("tick", C.c_uint64), ("info", BindInfo), ("runs_in_buffer", C.c_uint32),
                ("runs", C.POINTER(BindRun)), ("touch_words", U32P)]


class LaneGraph(C.Structure):
    _fields_ = [("segments", C.c_uint32), ("nodes", C.c_uint32), ("connections", C.c_uint32),
                ("seg_start3", F32P), ("seg_dir3", F32P), ("seg_length", F32P), ("seg_active", U8P), ("seg_end_node", U32P),
                ("seg_speed_limit", F32P), ("node_pos3", F32P), ("node_conn_offset", U32P), ("node_conn", U32P)]


class TierParams(C.Structure):
    _fields_ = [("tier_a_enter", C.c_float), ("tier_a_exit", C.c_float), ("tier_b_enter", C.c_float), ("tier_b_exit", C.c_float),
                ("max_physics", C.c_uint32), ("max_kinematic", C.c_uint32)]


class TierCounts(C.Structure):
    _fields_ = [("physics", C.c_uint32), ("kinematic", C.c_uint32), ("on_rails", C.c_uint32), ("total", C.c_uint32)]


class CommInfo(C.Structure):
    _fields_ = [("has_communicator", C.c_uint32), ("world_size", C.c_uint32), ("rank", C.c_uint32), ("rccl_version", C.c_uint32),
                ("neighbour_mask", C.c_uint32), ("peer_rank", C.c_int32 * 8), ("operations_per_group", C.c_uint32),
                ("pipeline_depth", C.c_uint32), ("border_records_per_sector", C.c_uint32), ("bytes_sent_per_step", C.c_uint64),
                ("host_steps", C.c_uint64), ("host_tick_half_us", C.c_double), ("host_pair_half_us", C.c_double)]


class SectorInfo(C.Structure):
    _fields_ = [("version", C.c_uint32), ("sector_x", C.c_int32), ("sector_z", C.c_int32), ("instances", C.c_uint32),
                ("lanes", C.c_uint32), ("lane_points", C.c_uint32), ("spawners", C.c_uint32), ("colliders", C.c_uint32),
                ("truncated", C.c_uint32)]


class SectorInstances(C.Structure):
    _fields_ = [("capacity", C.c_uint32),
                ("id", U64P), ("model_id", U64P), ("mesh_id", U64P), ("material_id", U64P), ("albedo_texture_id", U64P),
                ("material_flags", U32P), ("tags", U32P),
                ("pos3", F32P), ("rot3", F32P), ("scale3", F32P), ("name64", C.c_void_p)]


# every symbol of include/sc_tick.h: name -> (restype, argtypes)
_CTX = C.c_void_p
SYMBOLS = {
    "scTickGetApiVersion": (C.c_uint32, []),
    "scTickCreateContext": (_CTX, [C.POINTER(ContextDesc)]),
    "scTickDestroyContext": (None, [_CTX]),
    "scTickGetLastError": (C.c_char_p, [_CTX]),
    "scTickSetEntityCount": (C.c_int, [_CTX, C.c_uint32]),
    "scTickUploadLocals": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P, F32P, F32P, U8P]),
    "scTickUploadPositions": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P]),
    "scTickUploadBounds": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P, F32P, U8P]),
    "scTickUploadColliders": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, U8P, F32P, F32P, F32P]),
    "scTickReadColliders": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, U8P, F32P, F32P, F32P]),
    "scTickUploadRenderMeshes": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, U8P, U32P, U32P]),
    "scTickUploadLayers": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, U32P, U32P]),
    "scTickSetTopology": (C.c_int, [_CTX, I32P, C.c_uint32]),
    "scTickMarkDirty": (C.c_int, [_CTX, C.c_uint32, C.c_uint32]),
    "scTickMarkDirtyIndices": (C.c_int, [_CTX, U32P, C.c_uint32]),
    "scTickUploadWorldMatrices": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P]),
    "scTickSetDirtyFlags": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, U8P]),
    "scTickSetDrawBudget": (C.c_int, [_CTX, C.c_uint32]),
    "scTickSetDrawSortTable": (C.c_int, [_CTX, U8P, C.c_uint32, C.c_uint32]),
    "scTickSetTile": (C.c_int, [_CTX, C.c_uint32, C.c_uint32]),
    "scTickSetTileGrid": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "scTickSetBorderCapacity": (C.c_int, [_CTX, C.c_uint32]),
    "scTickBorderBytes": (C.c_uint32, [_CTX, C.c_uint32]),
    "scTickBindBorderBuffers": (C.c_int, [_CTX, C.c_uint32, C.c_void_p, C.c_void_p]),
    "scTickRunPairs": (C.c_int, [_CTX]),
    "scTickSetPairsStream": (C.c_int, [_CTX, C.c_void_p]),
    "scTickBindBorderBuffersParity": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "scTickGetBorderBuffer": (C.c_void_p, [_CTX, C.c_uint32, C.c_uint32, C.c_int]),
    "scTickSetStream": (C.c_int, [_CTX, C.c_void_p, C.c_int]),
    "scTickCommGetUniqueId": (C.c_int, [U8P]),
    "scTickCommInit": (C.c_int, [_CTX, U8P, C.c_uint32, C.c_uint32]),
    "scTickCommSetPeers": (C.c_int, [_CTX, I32P]),
    "scTickCommDestroy": (C.c_int, [_CTX]),
    "scTickSetPipelined": (C.c_int, [_CTX, C.c_int]),
    "scTickGetCommInfo": (C.c_int, [_CTX, C.POINTER(CommInfo)]),
    "scTickGatherVisibleCounts": (C.c_int, [_CTX, U32P, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "scTickGetBinStats": (C.c_int, [_CTX, U32P]),
    "scTickGetLearnTicks": (C.c_int, [_CTX, U32P]),
    "scTickGetTailStats": (C.c_int, [_CTX, U32P]),
    "scTickGetCompactStats": (C.c_int, [_CTX, U32P]),
    "scTickGetCarryStats": (C.c_int, [_CTX, U32P]),
    "scTickGetFrameStats": (C.c_int, [_CTX, U32P]),
    "scTickGetBoundsClassStats": (C.c_int, [_CTX, U32P]),
    "scTickGetTopologyClassStats": (C.c_int, [_CTX, U32P]),
    "scTickSetWorldLayers": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, C.c_int]),
    "scTickResetHostTimes": (C.c_int, [_CTX]),
    "scTickTileStep": (C.c_int, [_CTX, C.c_uint32]),
    "scTickExchangeBorders": (C.c_int, [_CTX]),
    "scTickUploadMovers": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, U8P, F32P, F32P, F32P]),
    "scTickAdvanceMovers": (C.c_int, [_CTX, C.c_float]),
    "scTickReadMoverVelocities": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P]),
    "scTickSetFrameProducer": (C.c_int, [_CTX, C.c_uint32, C.c_float]),
    "scTickSetFrameReadback": (C.c_int, [_CTX, C.c_uint32, C.c_uint32]),
    "scTickAcquireFrame": (C.c_int, [_CTX, C.c_uint32, C.POINTER(Frame)]),
    "scTickSetBindRuns": (C.c_int, [_CTX, C.c_uint32]),
    "scTickReadBindRuns": (C.c_int, [_CTX, C.POINTER(BindRun), C.c_uint32, C.POINTER(BindInfo)]),
    "scTickReadMaterialTouches": (C.c_int, [_CTX, U32P, C.c_uint32, U32P]),
    "scTickAcquireFrameBinds": (C.c_int, [_CTX, C.c_uint32, C.POINTER(FrameBinds)]),
    "scTickSetLaneGraph": (C.c_int, [_CTX, C.POINTER(LaneGraph)]),
    "scTickSetLaneActive": (C.c_int, [_CTX, U32P, C.c_uint32, C.c_int]),
    "scTickUploadTrafficAgents": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, U8P, U32P, F32P, F32P, U8P, F32P]),
    "scTickReadTrafficAgents": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, U32P, F32P, F32P, U8P]),
    "scTickSetTrafficSpeedMultiplier": (C.c_int, [_CTX, C.c_float]),
    "scTickSetTrafficSensors": (C.c_int, [_CTX, C.c_int, C.c_float, C.c_float]),
    "scTickReadTrafficBrakes": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P]),
    "scTickUploadTrafficSensors": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P, F32P]),
    "scTickReadTrafficSensors": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P, U8P]),
    "scTickSelectTrafficTiers": (C.c_int, [_CTX, F32P, C.POINTER(TierParams), C.POINTER(TierCounts)]),
    "scTickSelectTrafficDespawns": (C.c_int, [_CTX, F32P, C.c_uint32, U32P, C.c_uint32, U32P]),
    "scTickSetViewProj": (C.c_int, [_CTX, F32P]),
    "scTickSetFrustumPlanes": (C.c_int, [_CTX, F32P, C.c_int]),
    "scTickGetFrustumPlanes": (C.c_int, [_CTX, F32P, C.POINTER(C.c_int)]),
    "scTickSetFreezeCulling": (C.c_int, [_CTX, C.c_int]),
    "scTickRun": (C.c_int, [_CTX, C.c_uint32]),
    "scTickSynchronize": (C.c_int, [_CTX]),
    "scTickNudgeRootsX": (C.c_int, [_CTX, C.c_float]),
    "scTickGetCounts": (C.c_int, [_CTX, C.POINTER(Counts)]),
    "scTickReadVisible": (C.c_int, [_CTX, U32P, C.c_uint32, U32P]),
    "scTickReadCulled": (C.c_int, [_CTX, U32P, C.c_uint32, U32P]),
    "scTickReadVisibilityBits": (C.c_int, [_CTX, U64P, C.c_uint32]),
    "scTickReadWorldMatrices": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P]),
    "scTickReadWorldMatricesIndexed": (C.c_int, [_CTX, U32P, C.c_uint32, F32P]),
    "scTickReadDirty": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, U8P]),
    "scTickReadPositions": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P]),
    "scTickReadWorldAabbs": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P, F32P]),
    "scTickReadPairs": (C.c_int, [_CTX, U32P, C.c_uint32, U32P]),
    "scTickReadDraws": (C.c_int, [_CTX, C.POINTER(DrawItem), C.c_uint32, U32P]),
    "scTickSetRayQueries": (C.c_int, [_CTX, C.c_uint32, F32P, F32P, F32P, U32P]),
    "scTickReadRayHits": (C.c_int, [_CTX, C.POINTER(RayHit), C.c_uint32, U32P]),
    "scTickSetSweepQueries": (C.c_int, [_CTX, C.c_uint32, F32P, F32P, F32P, F32P, U32P, U32P]),
    "scTickReadSweepHits": (C.c_int, [_CTX, C.POINTER(SweepHit), C.c_uint32, U32P]),
    "scTickSetAnchoredRays": (C.c_int, [_CTX, C.c_uint32, U32P, F32P, F32P, F32P, U32P, U8P]),
    "scTickReadAnchoredRayHits": (C.c_int, [_CTX, C.POINTER(RayHit), C.c_uint32, U32P]),
    "scTickReadAnchoredRays": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, U32P]),
    "scTickSetRayShapes": (C.c_int, [_CTX, C.c_uint32]),
    "scTickGetRayShapes": (C.c_int, [_CTX, U32P]),
    "scTickSetSweepShapes": (C.c_int, [_CTX, C.c_uint32]),
    "scTickGetSweepShapes": (C.c_int, [_CTX, U32P]),
    "scTickGetSweepShapeInfo": (C.c_int, [_CTX, C.POINTER(SweepShapeInfo)]),
    "scTickSetPairEvents": (C.c_int, [_CTX, C.c_uint32, C.c_uint32]),
    "scTickReadPairEvents": (C.c_int, [_CTX, U32P, C.c_uint32, U32P, C.c_uint32, C.POINTER(PairEventInfo)]),
    "scTickSetTouchEvents": (C.c_int, [_CTX, C.c_uint32, C.c_uint32]),
    "scTickReadTouchEvents": (C.c_int, [_CTX, U32P, C.c_uint32, U32P, C.c_uint32, C.POINTER(TouchEventInfo)]),
    "scTickSetPairShapes": (C.c_int, [_CTX, C.c_uint32]),
    "scTickReadPairShapes": (C.c_int, [_CTX, U32P, C.c_uint32, C.POINTER(PairShapeInfo)]),
    "scTickSetPairContacts": (C.c_int, [_CTX, C.c_uint32]),
    "scTickGetPairContacts": (C.c_int, [_CTX, U32P]),
    "scTickReadPairContacts": (C.c_int, [_CTX, C.POINTER(PairContact), C.c_uint32, C.POINTER(PairContactInfo)]),
    "scTickSetPairManifolds": (C.c_int, [_CTX, C.c_uint32]),
    "scTickGetPairManifolds": (C.c_int, [_CTX, U32P]),
    "scTickReadPairManifolds": (C.c_int, [_CTX, C.POINTER(PairManifold), C.c_uint32, C.POINTER(PairManifoldInfo)]),
    "scTickSetPairIslands": (C.c_int, [_CTX, C.c_uint32, C.c_uint32]),
    "scTickGetPairIslands": (C.c_int, [_CTX, U32P, U32P]),
    "scTickReadPairIslands": (C.c_int, [_CTX, U32P, C.c_uint32, U32P, C.c_uint32, C.POINTER(PairIslandInfo)]),
    "scTickSetPairPersistence": (C.c_int, [_CTX, C.c_uint32, C.c_float]),
    "scTickGetPairPersistence": (C.c_int, [_CTX, U32P, F32P]),
    "scTickReadPairPersistence": (C.c_int, [_CTX, C.POINTER(PairPersist), C.c_uint32, C.POINTER(PairPersistInfo)]),
    "scTickWritePairPayloads": (C.c_int, [_CTX, F32P, C.c_uint32, C.c_uint32]),
    "scTickReadPairPayloads": (C.c_int, [_CTX, F32P, C.c_uint32]),
    "scTickSetPairSleep": (C.c_int, [_CTX, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_uint32]),
    "scTickGetPairSleep": (C.c_int, [_CTX, U32P, F32P, F32P, U32P, U32P]),
    "scTickWakeEntities": (C.c_int, [_CTX, U32P, C.c_uint32]),
    "scTickReadPairSleep": (C.c_int, [_CTX, U32P, C.c_uint32, U32P, C.c_uint32, U32P, C.c_uint32, C.POINTER(PairSleepInfo)]),
    "scTickSetOverlapQueries": (C.c_int, [_CTX, C.c_uint32, U8P, F32P, F32P, F32P, F32P, U32P, U32P, C.c_uint32, C.c_uint32]),
    "scTickReadOverlapHits": (C.c_int, [_CTX, U32P, U32P, C.c_uint32, C.POINTER(OverlapInfo)]),
    "scTickSetTriggerVolumes": (C.c_int, [_CTX, C.c_uint32, U32P, U8P, F32P, F32P, F32P, F32P, U32P, U8P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "scTickReadTriggerEvents": (C.c_int, [_CTX, U32P, C.c_uint32, U32P, C.c_uint32, C.POINTER(TriggerInfo)]),
    "scTickReadTriggerMembers": (C.c_int, [_CTX, U32P, U32P, C.c_uint32, C.POINTER(TriggerInfo)]),
    "scTickReadTriggerMatrices": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P]),
    "scTickReadTriggerVolumes": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, U32P]),
    "scTickSetAnchoredSweeps": (C.c_int, [_CTX, C.c_uint32, U32P, F32P, F32P, F32P, F32P, U32P, U8P, U8P]),
    "scTickReadAnchoredSweepHits": (C.c_int, [_CTX, C.POINTER(SweepHit), C.c_uint32, U32P]),
    "scTickReadAnchoredSweepSegments": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, F32P, F32P]),
    "scTickGetAnchoredSweepShapeInfo": (C.c_int, [_CTX, C.POINTER(SweepShapeInfo)]),
    "scTickReadAnchoredSweeps": (C.c_int, [_CTX, C.c_uint32, C.c_uint32, U32P]),
    "scTickQueryOccupied": (C.c_int, [_CTX, C.c_uint32, F32P, F32P, U32P, U8P]),
    "scTickSetProfiling": (C.c_int, [_CTX, C.c_int]),
    "scTickSetProfilingKernels": (C.c_int, [_CTX, C.c_uint32]),
    "scTickGetKernelTimes": (C.c_int, [_CTX, C.c_uint32, F32P, C.c_uint32, U32P]),
    "scTickSetGraphMode": (C.c_int, [_CTX, C.c_int]),
    "scTickGetStream": (C.c_void_p, [_CTX]),
    "scTickSectorParse": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(SectorInfo), C.POINTER(SectorInstances)]),
    "scTickSectorReadFile": (C.c_int, [C.c_char_p, C.POINTER(SectorInfo), C.POINTER(SectorInstances)]),
    "scTickHashAssetPath": (C.c_uint64, [C.c_char_p]),
    "scTickSectorPath": (C.c_uint32, [C.c_char_p, C.c_int32, C.c_int32, C.c_char_p, C.c_uint32]),
    "scTickAppendEntities": (C.c_int, [_CTX, C.c_uint32, F32P, F32P, F32P, F32P, F32P, U32P, U32P, U32P, U32P, I32P, U32P]),
    "scTickRemoveEntities": (C.c_int, [_CTX, U32P, C.c_uint32, U32P, U32P, U32P]),
    "scTickHostMat4Mul": (C.c_int, [F32P, F32P, F32P]),
    "scTickHostMat4Trs": (C.c_int, [F32P, F32P, F32P, F32P]),
    "scTickHostMat4Inverse": (C.c_int, [F32P, F32P]),
    "scTickHostMat4PerspectiveRhZo": (C.c_int, [C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, F32P]),
    "scTickHostCameraViewProj": (C.c_int, [F32P, C.c_float, C.c_float, C.c_float, C.c_float, F32P]),
    "scTickHostSpanClosed": (C.c_int, [I32P, C.c_uint32, C.c_uint32]),
    "scTickHostTopologyClasses": (C.c_int, [I32P, U8P, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint16), U32P, U32P]),
}

_LIB = None


class ScTickError(RuntimeError):
    pass


def load():
    """Load libsc_tick.so and bind every declared symbol.  Raises if the library is absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ScTickError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C sc_gameengine_amd/csrc).  There is no CPU fallback for the tick path.")
    lib = C.CDLL(LIB_PATH)
    lax = bool(os.environ.get("SC_TICK_LAX_BIND"))     # tools/ab_step.py only: A/B against a build of an older commit
    for name, (res, args) in SYMBOLS.items():
        if lax and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def comm_unique_id():
    """128-byte RCCL unique id (rank 0 calls this; the host hands the bytes to every rank)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    if not load().scTickCommGetUniqueId(buf):
        raise ScTickError("scTickCommGetUniqueId failed: " + (load().scTickGetLastError(None) or b"").decode())
    return bytes(buf)
