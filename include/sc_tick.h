/*
 * sc_tick.h -- C ABI of the MI355X world-tick library (libsc_tick.so).
 *
 * One context owns the device-resident SoA state of one world tile on one GPU and runs the
 * RenderPrep hot path of SandboxCityEngine on it:
 *
 *   TransformSystem            src/core/src/sc_ecs.cpp:118-211
 *   (CameraSystem stays on the host: sc_ecs.cpp:213-272; its product, viewProj, is an input here)
 *   CullingSystem              src/engine/world/sc_world_partition.cpp:1199-1284
 *   RenderPrepStreamingSystem  src/engine/world/sc_world_partition.cpp:1286-1359 (draw emission)
 *   AABB broadphase            Bullet btDbvtBroadphase behind src/engine/physics/sc_physics.cpp:218-225, :289, :296-299
 *
 * The reference has no FFI on this path: systems are C++ functions `void(World&, float, void*)`
 * (src/core/include/sc_scheduler.h:38).  This ABI is what the C++ adapter systems in
 * sc_gameengine_amd/host/sc_tick_systems.cpp (same signature, same state structs) call; a cgo /
 * JNI / ctypes binding would bind exactly these symbols.  Conventions follow the reference's own
 * C ABI, src/engine/include/sc_engine_render.h:130-163 and src/engine/src/sc_engine_render.cpp:88-177:
 * extern "C", opaque context from paired create/destroy, `int` 1 = ok / 0 = failed, every entry
 * point tolerates NULL, POD structs with fixed-size arrays, the caller owns every buffer it passes
 * and the callee copies, and a GetApiVersion().
 *
 * Entities are addressed by their DENSE index in the Transform pool (ComponentPool<Transform>::
 * denseEntities order, src/core/include/sc_ecs.h:199-277): that order defines the order of the
 * candidate / visible / culled lists (sc_world_partition.cpp:1206-1210, :1273-1280).
 *
 * Threading: a context may be used from any thread, one call at a time (systems may run on any job
 * worker: src/core/src/sc_scheduler.cpp:117-126); every call binds the device itself.
 * All device work is queued on the context's own stream; calls that return data synchronise it.
 */
#ifndef SC_TICK_H
#define SC_TICK_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SC_TICK_API_VERSION 7u
#define SC_TICK_MAX_ENTITIES ((1u << 24) - 1u)   /* Entity::INDEX_BITS = 24 (sc_ecs.h:18-20); index 0xFFFFFF is the "no parent" value */
#define SC_TICK_NO_PARENT (-1)

typedef struct ScTickContext ScTickContext;

/* scTickRun flags: which stages of the tick to execute */
enum {
  SC_TICK_XFORM       = 1u << 0,   /* TransformSystem */
  SC_TICK_CULL        = 1u << 1,   /* CullingSystem: visibility bits + ordered visible list */
  SC_TICK_BROADPHASE  = 1u << 2,   /* world AABBs + grid pair search */
  SC_TICK_CULLED_LIST = 1u << 3,   /* also build CullingState::culled */
  SC_TICK_DRAWS       = 1u << 4,   /* RenderPrepStreamingSystem draw list from the visible list */
  SC_TICK_DENSE_AABBS = 1u << 5,   /* with BROADPHASE: also keep per-entity world AABBs for scTickReadWorldAabbs */
  SC_TICK_SPLIT_PAIRS = 1u << 6,   /* with BROADPHASE on a multi-GPU tile: stop after filling the bins and packing the
                                      border messages; the caller exchanges them and calls scTickRunPairs */
  SC_TICK_SORT_DRAWS  = 1u << 7,   /* with DRAWS: the list comes out in the renderer's bind order (scTickSetDrawSortTable) */
  SC_TICK_RAYS        = 1u << 8,   /* with BROADPHASE: answer the ray queries set by scTickSetRayQueries against this tick's boxes */
  SC_TICK_PRODUCE_NEXT = 1u << 9,  /* with XFORM: the frame producer (scTickSetFrameProducer) is applied at the END of this run, inside
                                      the end-of-tick kernel, as the producer of the NEXT frame -- instead of at the start of the next
                                      scTickRun.  Results of this run are unaffected; positions read back are already the next frame's. */
  SC_TICK_SWEEPS      = 1u << 10,  /* with BROADPHASE: answer the capsule sweeps set by scTickSetSweepQueries against this tick's boxes */
  SC_TICK_ANCHORED_RAYS = 1u << 11, /* with BROADPHASE: answer the entity-anchored rays set by scTickSetAnchoredRays against this tick's boxes */
  SC_TICK_PAIR_EVENTS = 1u << 12,  /* with BROADPHASE: report which pairs begun and which ended since the last run with this flag (scTickSetPairEvents) */
  SC_TICK_BIND_RUNS   = 1u << 13,  /* with DRAWS | SORT_DRAWS: also the bind runs of the sorted list and the material touch set (scTickSetBindRuns) */
  SC_TICK_PAIR_SHAPES = 1u << 14,  /* with BROADPHASE: also list the pairs of this tick whose collider shapes overlap (scTickSetPairShapes) */
  SC_TICK_TOUCH_EVENTS = 1u << 15, /* with BROADPHASE: report which pairs begun and which ended TOUCHING since the last run with this flag (scTickSetTouchEvents) */
  SC_TICK_OVERLAPS    = 0x00010000u, /* bit 16.  With BROADPHASE: answer the overlap queries set by scTickSetOverlapQueries against this tick's boxes */
  SC_TICK_TRIGGERS    = 0x00020000u, /* bit 17.  With BROADPHASE: answer the trigger volumes set by scTickSetTriggerVolumes and report who entered / left since the last run with this flag */
  SC_TICK_ANCHORED_SWEEPS = 0x00040000u, /* bit 18.  With BROADPHASE: answer the entity-anchored capsule sweeps set by scTickSetAnchoredSweeps against this tick's matrices and boxes */
  SC_TICK_FULL        = SC_TICK_XFORM | SC_TICK_CULL | SC_TICK_BROADPHASE
};

typedef struct ScTickContextDesc
{
  int32_t  device_ordinal;     /* HIP device */
  uint32_t capacity;           /* max entities in this context, <= SC_TICK_MAX_ENTITIES */
  /* broadphase grid: the rectangle of sectors this context's tile covers, in worldToSector
   * coordinates (sc_world_partition.cpp:268-275).  sectors_x == 0 disables the broadphase. */
  int32_t  tile_origin_x;
  int32_t  tile_origin_z;
  uint32_t tile_sectors_x;
  uint32_t tile_sectors_z;
  float    sector_size;        /* WorldPartitionConfig::sectorSizeMeters, 64 m (sc_world_partition.h:151) */
  uint32_t max_pairs;          /* capacity of the pair list (0 = capacity entities * 4) */
  uint32_t max_draws_budget;   /* WorldStreamingBudgets::maxDrawsBudget (sc_world_partition.h:309); 0 = unlimited */
  uint32_t reserved;
} ScTickContextDesc;

typedef struct ScTickCounts    /* CullingStats (sc_world_partition.h:334-339) + pair / draw counts */
{
  uint32_t entities;
  uint32_t renderables_total;
  uint32_t visible;
  uint32_t culled;
  uint32_t pairs;              /* pairs found (may exceed the pair capacity; the list is then truncated) */
  uint32_t pairs_truncated;    /* 1 if pairs > capacity */
  uint32_t draws_emitted;      /* RenderPrepStats (sc_world_partition.h:353-357) */
  uint32_t draws_dropped;
  uint32_t max_depth;          /* deepest hierarchy level after scTickSetTopology */
  uint32_t unreachable;        /* entities in or below a parent cycle (never updated, sc_ecs.cpp:173-210) */
  /* bin_overflow, big_boxes and border_lost are counted where the bins are filled.  After a QUIET tick (scTickGetBinStats: a broadphase
     tick of a world that cannot pair and whose bins nothing else reads fills none) they keep the values of the most recent tick that did. */
  uint32_t bin_overflow;       /* bin records that found their sector's bin (64 records) full: they sit in the sector overflow list */
  uint32_t big_boxes;          /* boxes in the big list: larger than 2x2 sectors or outside the tile rectangle */
  uint32_t draws_sorted;       /* with SC_TICK_SORT_DRAWS: draws left after the renderer's mesh / material handle checks */
  uint32_t border_lost;        /* records the fixed capacities could not carry: border messages that ran out of room
                                  (scTickSetBorderCapacity), big boxes reaching beyond the eight neighbouring tiles, a sector with more
                                  than 64 + 1024 boxes; non-zero means pairs may be missing */
  uint32_t relinks;            /* whole-world hierarchy re-links (O(entities) on the host) this context has done so far */
  uint32_t vocabulary_violations;  /* with scTickSetWorldLayers(known): border records and big boxes that ARRIVED from a neighbour with group or
                                      mask bits outside the declared vocabulary this tick -- the neighbour broke the contract, pairs in bins
                                      this tile leaves unwritten may be missing; 0 otherwise.  (This tile's own layers cannot leave the
                                      vocabulary: scTickUploadLayers / scTickAppendEntities refuse them.) */
} ScTickCounts;

typedef struct ScTickDrawItem  /* DrawItem, sc_ecs.h:159-165: 80 bytes, model at offset 16, column-major */
{
  uint32_t dense_index;        /* the host adapter maps it to the Entity handle */
  uint32_t mesh_id;
  uint32_t material_id;
  uint32_t pad;
  float    model[16];
} ScTickDrawItem;

/* kernels whose per-launch durations scTickGetKernelTimes reports (SC_TICK_K_PAIRS: the end-of-tick kernel of a tick with
 * SC_TICK_BROADPHASE -- compaction + pair search in one launch, or the compaction alone on a quiet tick, scTickGetBinStats) */
enum { SC_TICK_K_XFORM_CULL = 0, SC_TICK_K_COMPACT = 1, SC_TICK_K_PAIRS = 2, SC_TICK_K_NUDGE = 3 /* producer: nudge or movers */, SC_TICK_K_COUNT = 4 };

uint32_t       scTickGetApiVersion(void);
ScTickContext* scTickCreateContext(const ScTickContextDesc* desc);
void           scTickDestroyContext(ScTickContext* ctx);
/* text of the last failure on this context (or of the last failed create when ctx is NULL) */
const char*    scTickGetLastError(const ScTickContext* ctx);

/* ---- entity state upload (host -> device SoA).  [first, first+count) are dense indices. ---- */
/* (scTickSetEntityCount: when the count changes, the per-run words of the bounds classes below are brought up to date for the runs
 *  of 64 that gained or lost entities -- a small copy on the context's stream, which the call waits for) */
int scTickSetEntityCount(ScTickContext* ctx, uint32_t count);
/* setLocal (sc_ecs.h:78-84): position, XYZ Euler radians, scale; marks the range dirty.  sin/cos of
 * the angles are taken here with the host libm, as mat4_rotation_xyz does (sc_math.cpp:102-107), so
 * device matrices equal the host's bit for bit.  An all-zero scale is stored as (1,1,1), the repair
 * TransformSystem applies (sc_ecs.cpp:143-149); repaired[i] (nullable) reports it. */
int scTickUploadLocals(ScTickContext* ctx, uint32_t first, uint32_t count,
                       const float* pos3, const float* rot3, const float* scale3, uint8_t* repaired);
/* setLocalPosition (sc_ecs.h:92-96) */
int scTickUploadPositions(ScTickContext* ctx, uint32_t first, uint32_t count, const float* pos3);
/* Bounds::localAabb (sc_world_partition.h:298-301); has_bounds NULL = every entity has one */
int scTickUploadBounds(ScTickContext* ctx, uint32_t first, uint32_t count,
                       const float* min3, const float* max3, const uint8_t* has_bounds);
/* RenderMesh (sc_ecs.h:107-111); has_mesh NULL = every entity is a culling candidate */
int scTickUploadRenderMeshes(ScTickContext* ctx, uint32_t first, uint32_t count,
                             const uint8_t* has_mesh, const uint32_t* mesh_id, const uint32_t* material_id);
/* collision filter group / mask (sc_physics.cpp:372-379); low 16 bits are kept, 0xFFFFFFFF = all */
int scTickUploadLayers(ScTickContext* ctx, uint32_t first, uint32_t count,
                       const uint32_t* group, const uint32_t* mask);
/* Collider (sc_physics.h:12-28; createShape, sc_physics.cpp:136-166): what an entity's broadphase proxy is formed from.
 * BOUNDS, the default of every entity, is the box of its Bounds (an entity without Bounds then has no proxy); NONE is an
 * entity without a Collider component: it enters no bin and no big list, forms no pair and answers no ray; BOX / SPHERE /
 * CAPSULE are the reference's three shapes, centred on the entity's ORIGIN, and need no Bounds.  With M the entity's world
 * matrix, c = M[:,3], n_k the squared norm of column k of M (own spec; fp32, unfused, left to right):
 *   BOX      h_r = (|M[r,0]| hx + |M[r,1]| hy) + |M[r,2]| hz
 *   SPHERE   h_r = radius * sqrt(max(n_0, n_1, n_2))
 *   CAPSULE  h_r = |M[r,1]| * max(0, half_height) + radius * sqrt(max(n_0, n_2))
 * and the box is [c - h, c + h].  Culling is not affected: the cull sphere always comes from Bounds.
 * type NULL = BOX for every entity; half_extents3 / radius / half_height NULL = the reference's defaults 0.5 / 0.5 / 0.5.
 * Fails for an unknown type, a negative or non-finite half extent or radius, a non-finite half_height (a negative one is
 * stored as 0).  All five values are kept per entity whatever its type, travel with it through scTickRemoveEntities, and
 * come back through scTickReadColliders; scTickAppendEntities and a growing scTickSetEntityCount start new entities as
 * BOUNDS.  A context that never calls scTickUploadColliders runs exactly the kernels it ran without this call. */
enum { SC_TICK_COLLIDER_BOUNDS = 0, SC_TICK_COLLIDER_NONE = 1, SC_TICK_COLLIDER_BOX = 2, SC_TICK_COLLIDER_SPHERE = 3, SC_TICK_COLLIDER_CAPSULE = 4 };
int scTickUploadColliders(ScTickContext* ctx, uint32_t first, uint32_t count, const uint8_t* type,
                          const float* half_extents3, const float* radius, const float* half_height);
int scTickReadColliders(ScTickContext* ctx, uint32_t first, uint32_t count, uint8_t* type,
                        float* half_extents3, float* radius, float* half_height);
/* Transform::parent for every entity as a dense index (SC_TICK_NO_PARENT = root).  A parent that is
 * out of range or the entity itself is detached and the entity marked dirty (sc_ecs.cpp:151-160).
 * Computes hierarchy depth; entities in or below a parent cycle are flagged unreachable. */
int scTickSetTopology(ScTickContext* ctx, const int32_t* parent_dense_index, uint32_t count);
/* markDirty (sc_ecs.h:73-76) */
int scTickMarkDirty(ScTickContext* ctx, uint32_t first, uint32_t count);
int scTickMarkDirtyIndices(ScTickContext* ctx, const uint32_t* dense_indices, uint32_t count);
/* set Transform::dirty of a range to exactly these values (1 = dirty); used when a host ECS re-syncs
 * its whole state after the pool's dense order changed (sc_ecs.h:240-262 swap-remove) */
int scTickSetDirtyFlags(ScTickContext* ctx, uint32_t first, uint32_t count, const uint8_t* dirty);
/* seed Transform::worldMatrix (column-major Mat4, must be affine: row 3 == 0,0,0,1) */
int scTickUploadWorldMatrices(ScTickContext* ctx, uint32_t first, uint32_t count, const float* mat16);

/* ---- per-frame inputs ---- */
/* RenderFrameData::viewProj (sc_ecs.h:167-173); the six planes are derived as frustumFromViewProj
 * does (sc_world_partition.cpp:1071-1103) */
int scTickSetViewProj(ScTickContext* ctx, const float view_proj[16]);
/* or the planes directly: 6 x (nx, ny, nz, d), and Frustum::valid */
int scTickSetFrustumPlanes(ScTickContext* ctx, const float planes24[24], int valid);
int scTickGetFrustumPlanes(ScTickContext* ctx, float planes24[24], int* valid);
/* CullingState::freezeCulling (sc_world_partition.cpp:1227-1233) */
int scTickSetFreezeCulling(ScTickContext* ctx, int freeze);
/* WorldStreamingBudgets::maxDrawsBudget for the next SC_TICK_DRAWS (overrides the create-time value; 0 = unlimited).  May be
 * called between any two runs, with graph replay on too: a changed budget re-captures the next run (a captured tick holds the
 * budget by value); an unchanged one costs nothing. */
int scTickSetDrawBudget(ScTickContext* ctx, uint32_t max_draws);

/* ---- the tick ---- */
int scTickRun(ScTickContext* ctx, uint32_t flags);       /* queues the stages; returns at once */
int scTickSynchronize(ScTickContext* ctx);
/* upstream producer of SynthWorld's dirty regime (ii): localPos.x += dx on every root, marked dirty
 * (the device-side analogue of PhysicsSyncSystem's transform writes, sc_physics.cpp:1167-1186) */
int scTickNudgeRootsX(ScTickContext* ctx, float dx);

/* ---- multi-GPU tiles (one context per GPU, one process per GPU) ----
 * The world is cut into equal rectangular tiles of sectors; each context owns one (ScTickContextDesc
 * tile_*).  Transform and culling need no exchange.  The broadphase needs the boxes that reach over a
 * tile edge: after scTickRun(... | SC_TICK_BROADPHASE | SC_TICK_SPLIT_PAIRS) the message for each
 * existing neighbour sits in the bound send buffer; the caller moves send[d] of this rank into
 * recv[7-d] of the neighbour in direction d (RCCL send/recv, or a peer copy) on the context's stream
 * and then calls scTickRunPairs.  Directions: d = 0..7 for (dx,dz) = (-1,-1) (0,-1) (1,-1) (-1,0)
 * (1,0) (-1,1) (0,1) (1,1).  Pair ids are rank << 24 | dense index. */
int scTickSetTile(ScTickContext* ctx, uint32_t rank, uint32_t neighbour_mask);
/* This tile's place (tile_x, tile_z) in the grid of tiles_x x tiles_z equal tiles; sets the neighbour mask from it.
 * With the grid known the border messages also carry the big boxes (wider than 2x2 sectors or outside the tile's
 * rectangle) that reach a neighbour's region, so pairs with them are found across tile
 * borders too: a tile reports a box-vs-big pair when it owns the sector of the box's primary copy, and a big-vs-big
 * pair when it owns the sector holding the low corner of the intersection (sectors outside the world belong to the
 * nearest tile).  A big box may reach its own tile and the eight around it; one that reaches further, or a message
 * that runs out of room, is counted in ScTickCounts::border_lost. */
int scTickSetTileGrid(ScTickContext* ctx, uint32_t tile_x, uint32_t tile_z, uint32_t tiles_x, uint32_t tiles_z);
/* Capacity of the border messages: `records_per_ring_sector` records per sector of a ring side ON AVERAGE (the side's
 * sectors share the message: a crowded ring sector may take more than its share), never less than one full sector (its
 * 64-record bin + 1024 overflow records).  Default 16 -- SynthWorld's ring sectors hold 0-2.  A world authored at the engine's
 * streaming budget (200 entities per sector, src/sandbox/src/main.cpp:92-99) with districts on tile edges wants more; what a
 * message cannot hold is counted in ScTickCounts::border_lost, never dropped silently.  Every tile of a world must use the
 * same value (the two sides of an edge agree on the message size).  Call before scTickCommInit / before binding buffers:
 * bound buffers are unbound, scTickBorderBytes changes. */
int scTickSetBorderCapacity(ScTickContext* ctx, uint32_t records_per_ring_sector);
/* size in bytes of the fixed-capacity border message of direction d (same on both sides of an edge) */
uint32_t scTickBorderBytes(ScTickContext* ctx, uint32_t direction);
/* caller-owned device buffers (e.g. torch tensors) of at least scTickBorderBytes(d) bytes each.  scTickBindBorderBuffers and
 * scTickBindBorderBuffersParity may be called again between two steps with other buffers, with graph replay on too: while
 * captured graphs exist, a changed address waits for the work in flight and re-captures
 * the next tick half and pair half (a captured pack or merge holds the addresses by value); the same addresses cost nothing.
 * The buffers bound before must stay allocated until that call returns. */
int scTickBindBorderBuffers(ScTickContext* ctx, uint32_t direction, void* send_device_ptr, void* recv_device_ptr);
int scTickRunPairs(ScTickContext* ctx);
/* Pipelined tiles.  With a pairs stream set (hipStream_t; NULL switches it off), scTickRunPairs queues the merge, the ray
 * queries and the pair search of tick t on THAT stream, and the next scTickRun may start its fused kernel while they run:
 * everything the two halves share -- bins, big list, spill list, border messages -- exists `depth` times (3 unless
 * scTickSetPipelined chose otherwise, at most 4), selected by tick parity t mod depth (counters, big-box bits and the pair
 * output already are).  The library orders the halves with events: scTickRun makes the pairs stream wait for the pack of its
 * tick, and tick t+depth-1, whose end-of-tick kernel clears the counters tick t+depth fills again, first waits for the pair half
 * of tick t.  With depth d the pair half (exchange latency included) may take up to d-2 ticks before it holds anything up;
 * until that clearing, the parity keeps tick t's results (counts, pair shard counters) for the host to read.  The caller issues the exchange
 * of tick t on the pairs stream after scTickRun (border buffers of parity t mod depth, counted from the moment the pairs stream
 * was set: scTickBindBorderBuffersParity), then calls scTickRunPairs -- e.g. the pairs
 * stream is torch's current stream, where its RCCL operations go, and the tick runs on the context's own stream.
 * Read the results of tick t (pairs, ray hits, counts) after its scTickRunPairs and before the next scTickRun, as always.
 * With graph replay on (scTickSetGraphMode) each half of a pipelined step is a graph of its own, on its own stream.  Switching the pairs stream on or off synchronises and clears the per-parity broadphase
 * state (the two flows clear it differently): the previous tick's pairs / counts are no longer readable afterwards. */
int scTickSetPairsStream(ScTickContext* ctx, void* hip_stream);
int scTickBindBorderBuffersParity(ScTickContext* ctx, uint32_t parity, uint32_t direction, void* send_device_ptr, void* recv_device_ptr);
/* the device buffer bound for (tick parity, direction): recv == 0 the outgoing message, != 0 the incoming one; NULL = none.
 * Parity 0 is also the in-order flows' only set. */
void* scTickGetBorderBuffer(ScTickContext* ctx, uint32_t parity, uint32_t direction, int recv);
/* ---- the exchange itself, owned by the library (north_star: "Host code stays C++ ... RCCL over xGMI exchanging only
 * tile-border AABBs").  The reference has no counterpart: it is a single process ("Distributed
 * communication backend: none"); the tile sharding is this build's, its unit is the sector grid of
 * src/engine/world/sc_world_partition.cpp:268-287.
 * One RCCL communicator per context = per GPU = per process.  Rank 0 asks for a unique id, the host hands its 128 bytes
 * to every rank over whatever channel it has (a file, a socket, MPI, torch.distributed: bench.py), and every rank calls
 * scTickCommInit after scTickSetTileGrid.  The neighbour in direction d is the rank of tile (tile_x+dx, tile_z+dz) in
 * row-major tile order unless scTickCommSetPeers says otherwise (-1 = none).  The library then owns the border message
 * buffers of both tick parities (RCCL is opened with dlopen on first use; a single-GPU host never needs it).
 * scTickTileStep(flags) is one whole step of a tile in one call: scTickRun(flags | SC_TICK_SPLIT_PAIRS), the exchange as
 * ONE group of ncclSend / ncclRecv on the stream the pair half runs on (the pairs stream when pipelined), scTickRunPairs.
 * Nothing in it waits on the host.  A tile without neighbours (1x1 grid) runs scTickRun(flags).  A tile WITH neighbours
 * and no communicator fails: the exchange is never skipped silently.
 * scTickSetPipelined(n) = scTickSetPairsStream with a second stream of the library's own: n = 0 off, 1 = on with the default
 * depth (4 copies of the per-tick broadphase state), 2..4 = on with that depth (2 leaves the pair half no tick to hide under). */
#define SC_TICK_COMM_ID_BYTES 128
int scTickCommGetUniqueId(uint8_t id[SC_TICK_COMM_ID_BYTES]);
int scTickCommInit(ScTickContext* ctx, const uint8_t id[SC_TICK_COMM_ID_BYTES], uint32_t world_size, uint32_t rank);
int scTickCommSetPeers(ScTickContext* ctx, const int32_t peer_rank[8]);
int scTickCommDestroy(ScTickContext* ctx);
int scTickSetPipelined(ScTickContext* ctx, int enable);
/* What a multi-GPU run needs in order to be read afterwards: the communicator as ncclCommInitRank saw it, the exchange's
 * shape, and the host time scTickTileStep spends issuing each half of a step (averages since the last reset; an in-order
 * captured step counts as one tick half).  Valid without a communicator too (a 1x1 grid: zeros). */
typedef struct ScTickCommInfo
{
  uint32_t has_communicator, world_size, rank;
  uint32_t rccl_version;               /* ncclGetVersion of the library the context bound at run time */
  uint32_t neighbour_mask;
  int32_t  peer_rank[8];               /* -1 = no neighbour in that direction */
  uint32_t operations_per_group;       /* ncclSend + ncclRecv calls inside the one group of a step */
  uint32_t pipeline_depth;             /* 0 = in order */
  uint32_t border_records_per_sector;  /* scTickSetBorderCapacity */
  uint64_t bytes_sent_per_step;        /* fixed-size messages: what the group moves out of this rank per step */
  uint64_t host_steps;
  double   host_tick_half_us, host_pair_half_us;
} ScTickCommInfo;
int scTickGetCommInfo(ScTickContext* ctx, ScTickCommInfo* out);
/* Result assembly at N > 1: the global visible list is the concatenation of the tiles' lists in rank order --
 * entities are created tile-major, so that IS the order of the reference's serial compaction over the whole world
 * (src/engine/world/sc_world_partition.cpp:1273-1280) -- and each rank copies its slice to the host at its own offset.  This call
 * is the one tiny collective that needs: an all-gather of the ranks' visible counts of the last tick over the context's
 * communicator (ncclAllGather of one uint32 per rank; every rank must call it, after the same tick).  counts_out (may be NULL)
 * receives min(world_size, capacity) counts; *offset_out = the sum of the counts of the ranks before this one = where this rank's
 * scTickReadVisible slice starts in the global list (its ids are dense indices of the tile: add rank * entities-per-tile for
 * global dense indices); *total_out = the length of the global list.  Without a communicator (a 1x1 grid) the tile is the world:
 * offset 0, total = its own count.  Synchronises the context (a read-back call, like scTickReadVisible). */
int scTickGatherVisibleCounts(ScTickContext* ctx, uint32_t* counts_out, uint32_t capacity, uint64_t* offset_out, uint64_t* total_out);

/* Broadphase bins, how they are filled (diagnostics; the pair set never depends on any of it).  Records keep the bin slot they
 * reserved at the last "learn" tick while their box stays in its sector (no reservation, i.e. no atomic, on the ticks in
 * between; SC_TICK_HOME_PERIOD ticks apart, default 64; SC_TICK_VARIANT bit 1 switches the slots off), and the slots of a bin
 * whose own records cannot pass the group/mask filter against each other -- static props only -- are not even written until a
 * record from elsewhere needs them (the pair search then rebuilds them; SC_TICK_VARIANT bit 5 switches that off; ticks with
 * ray queries or traffic sensors, and pipelined tiles, write every record).
 * QUIET ticks: a run with SC_TICK_BROADPHASE does the device work of the same call without the flag -- no bin, counter, layer summary
 * or home word is read or written; the pair set is empty by construction -- while ALL of this holds: no two layer words of the world
 * admit a pair (bit 2 below); the remembered slots are on, learnt and current (no append, remove, re-link or layer upload since the learn
 * tick); the flags hold none of SC_TICK_RAYS, _SWEEPS, _ANCHORED_RAYS, _PAIR_EVENTS, _PAIR_SHAPES, _DENSE_AABBS, _SPLIT_PAIRS; traffic
 * sensors are off, the tile has no neighbours and no pairs stream.  Any other tick bins as ever, and the first one behind a quiet stretch
 * rewrites every record it would otherwise have left alone (boxes may have moved unseen) and applies the learn rule (the slots age on
 * through the stretch, but no learn tick falls inside it).  ScTickCounts::bin_overflow, big_boxes and border_lost keep the values of the
 * most recent tick that binned.  SC_TICK_VARIANT bit 3 (8) switches quiet ticks off.
 * stats[0] remembered slots, [1] of those written on every tick, [2] bit 0: the last tick was allowed to leave the other slots
 * unwritten, bit 1: it left records of entities whose matrix was not rebuilt as they were, bit 2: no two of the uploaded layer words
 * (nor, on a tile, of the declared world vocabulary) admit a pair, so the pair role was launched as a sweep over the bins' counters
 * (a quarter of the workgroups; a launch shape, never a shortcut of the search), bit 3: the last tick was a quiet tick (the other bits then
 * still tell of the most recent tick that binned), [3] learn ticks so far.  Reads the slots back (a few MB): not for the frame loop. */
int scTickGetBinStats(ScTickContext* ctx, uint32_t stats[4]);
/* Where the tick ends (diagnostics; no result depends on it).  The fused kernel works in spans of consecutive dense indices, one
 * workgroup each.  In a world where no parent link crosses a span boundary ("span-closed") the workgroup also ends the tick for its
 * span -- clears Transform::dirty and, with SC_TICK_PRODUCE_NEXT and producer kind 1, nudges the roots -- instead of the end-of-tick
 * kernel; a tick with SC_TICK_XFORM but neither SC_TICK_CULL nor a pair half then has no second launch at all.  Worlds with hierarchy
 * levels beyond the fused kernel's chain, producer kind 2, traffic sensors, and contexts created under SC_TICK_TAIL=0 keep the
 * end-of-tick kernel's form.  stats[0] 1 = the last scTickRun's fused kernel owned the dirty words, [1] 1 = the world is span-closed for
 * the current span.  Host-side, no read-back (flushes a pending re-link; the span-closed state is rescanned, O(n), only after the
 * entity count moved to another span). */
int scTickGetTailStats(ScTickContext* ctx, uint32_t stats[2]);
/* How the last scTickRun's compaction was cut into workgroups (diagnostics; no result depends on it).  The compaction (the ordered visible
 * and culled lists, CullingStats' counters) is a role of the tick's end-of-tick launch.  Where that launch has nothing else to do -- a tick
 * with SC_TICK_CULL and without a pair half, whose fused kernel owned the dirty words (above) or which has no SC_TICK_XFORM -- and a
 * span holds at most 16384 entities, the launch takes its WIDE form: one workgroup takes several consecutive spans, one visibility word
 * (64 entities) per thread, and scatters word by word.  Every other launch keeps one workgroup per span (two where the pair search shares
 * the launch).  stats[0] workgroups of the compaction role, [1] spans per workgroup; 0 / 0 when the tick had no compaction (no
 * SC_TICK_CULL and the dirty words owned by the fused kernel, or an empty context).  Host-side, no read-back, no synchronisation.
 * A/B switches, read at creation: SC_TICK_VARIANT bit 4 (16) keeps one workgroup per span everywhere; SC_TICK_COMPACT_G=<n> fixes the
 * spans per workgroup of the wide form (clamped to what one word per thread allows) instead of the library's rule.
 * SC_TICK_VARIANT bits that remain: 1 (2) home slots off, 3 (8) quiet ticks off, 4 (16) wide compaction off, 5 (32) lazy records off. */
int scTickGetCompactStats(ScTickContext* ctx, uint32_t stats[2]);
/* The carried compaction (diagnostics; no result depends on it).  Where a tick's end-of-tick launch would be the wide compaction alone, behind
 * the classed tail instance of the fused kernel, launched eagerly (no graph replay), on a context without pairs stream, neighbours or frame
 * read-back, on a run without SC_TICK_DRAWS / SC_TICK_SORT_DRAWS / SC_TICK_BIND_RUNS and with the launch's profiling slot not timed on that
 * tick, the launch is DEFERRED: the next scTickRun whose fused launch is that instance carries it as a few workgroups at the head of its own
 * grid -- one launch per tick instead of two -- and any other next call that depends on it settles it first with the launch the tick would
 * have made: scTickSynchronize, every read of a list, the counts or a frame, scTickGatherVisibleCounts, the graph / pipelined / stream /
 * read-back / draw-budget setters, and a tick that cannot carry.  Every tick's lists and counts are what they were, one launch later or at
 * once when asked; scTickGetCompactStats reports the deferred launch's shape.  stats[0] ticks that deferred, [1] compactions carried,
 * [2] compactions settled, since creation.  Host-side, no read-back, no synchronisation.  A/B switch, read at creation: SC_TICK_CARRY=0
 * never defers. */
int scTickGetCarryStats(ScTickContext* ctx, uint32_t stats[3]);
/* stats[3] of the above alone: learn ticks so far.  Host-side, no read-back, no synchronisation (what a timed loop may ask). */
int scTickGetLearnTicks(ScTickContext* ctx, uint32_t* learn_ticks);
/* Bounds classes (diagnostics; no result depends on them).  The library keeps a table of the distinct local boxes it was given
 * (scTickUploadBounds, compared by bit pattern, up to 4096) and, per run of 64 consecutive dense indices, whether the entities with
 * Bounds there all have the same box; where they do, the fused kernel fetches that box once per run instead of once per entity.
 * stats[0] boxes in the table, [1] runs whose bounded entities share a box, [2] runs whose bounded entities do not (different boxes, or
 * a box the full table could not take; runs without a bounded entity count in neither), [3] bounded entities whose box is not in
 * the table.  Host-side, no read-back, no synchronisation -- but a walk over every entity's host record (O(n), about a millisecond
 * at a million entities): for tests and logs, not for the frame loop. */
int scTickGetBoundsClassStats(ScTickContext* ctx, uint32_t stats[4]);
/* Topology classes (diagnostics; no result depends on them).  A run of 64 consecutive dense indices is CLOSED when every entity in it has
 * at most three ancestors and all of them in the same run; its pattern is what the run's entities are to each other and carry as flags
 * (parent by position in the run, RenderMesh / Bounds, depth, which rotation axes are trivial).  The library numbers the distinct patterns
 * of the world (by bit pattern, up to 256) wherever it re-links the hierarchy.  In a world with a hierarchy whose every run is closed and
 * numbered -- worlds built from prefabs look like this -- a tick with SC_TICK_XFORM and without a binning half runs an instance of the fused
 * kernel that reads a run's pattern from a small table instead of a link word per entity and per ancestor.  Appending roots and removing
 * entities without a re-link leave the numbering behind; the general instance runs until the next re-link.  stats[0] patterns, [1] runs that
 * are closed and numbered, [2] runs that are not, as of the last re-link (a pending one is flushed), [3] 1 = the last scTickRun's fused
 * kernel was that instance.  Host-side, no read-back.  SC_TICK_TOPO_CLASSES=0 at creation: never that instance (A/B switch). */
int scTickGetTopologyClassStats(ScTickContext* ctx, uint32_t stats[4]);
/* The layer VOCABULARY of the tiled world: the OR of the group words and the OR of the mask words of every collider that exists on
 * ANY tile, now or later (until the next call; bits 0..15, or 0xFFFFFFFF = all, as scTickUploadLayers).  With it a pipelined tile
 * (scTickSetPipelined / scTickSetPairsStream) leaves the bins unwritten whose own records can meet nothing the world contains --
 * static props in a world without dynamic bodies, say -- because nothing will ever read them; without it (known = 0, the default)
 * a pipelined tile writes every record on every tick.  A contract, and a checked one: while a vocabulary is declared,
 * scTickUploadLayers / scTickAppendEntities FAIL for a group or mask word outside it (declare the wider vocabulary first), a call
 * that narrows the vocabulary below the layers already uploaded fails too, and a record or big box that arrives from a neighbour
 * with bits outside it is counted in ScTickCounts::vocabulary_violations (bench.py's N > 1 gate requires 0).  In-order flows do not
 * need the declaration (they rebuild unwritten bins on demand). */
int scTickSetWorldLayers(ScTickContext* ctx, uint32_t group_or, uint32_t mask_or, int known);
int scTickResetHostTimes(ScTickContext* ctx);
int scTickTileStep(ScTickContext* ctx, uint32_t flags);
/* the middle third of scTickTileStep on its own, for hosts that interleave other work: after scTickRun(... | SC_TICK_SPLIT_PAIRS) */
int scTickExchangeBorders(ScTickContext* ctx);
/* external != 0: run all device work of this context on the caller's stream `hip_stream` (hipStream_t;
 * NULL is the legacy default stream), e.g. the stream its RCCL calls are ordered on.
 * external == 0: return to the context's own stream. */
int scTickSetStream(ScTickContext* ctx, void* hip_stream, int external);

/* ---- upstream movers (the step before the path) ----
 * The engine's on-rails traffic tier writes Transform::localPos every fixed step and marks it dirty
 * (src/engine/traffic/sc_traffic_ai.cpp:434-460, speed 12 m/s src/engine/traffic/sc_traffic_lanes.h:17).
 * SynthWorld's movers are that model reduced to straight segments inside the agent's sector:
 *   kind 1 (vehicle): pos += vel*dt, wrapping inside [lo, hi) on x and z
 *   kind 2 (ped):     pos += vel*dt, reflecting at lo / hi (the velocity component flips)
 * Only localPos.x / .z change; the moved entities are marked dirty, exactly as setLocalPosition does.
 * These two kinds are SynthWorld's stand-ins (peds have no reference counterpart); the engine's own mover, the on-rails
 * traffic agent, is below ("on-rails traffic") and advances in the same call. */
int scTickUploadMovers(ScTickContext* ctx, uint32_t first, uint32_t count, const uint8_t* kind,
                       const float* vel_xz2, const float* lo_xz2, const float* hi_xz2);
int scTickAdvanceMovers(ScTickContext* ctx, float dt);
int scTickReadMoverVelocities(ScTickContext* ctx, uint32_t first, uint32_t count, float* vel_xz2);
/* Make a producer part of the frame: every scTickRun then starts with it, so the whole frame (producer +
 * tick) is one stream sequence and, in graph mode, one captured hipGraph.  kind 0 = none,
 * 1 = scTickNudgeRootsX(param), 2 = scTickAdvanceMovers(param). */
int scTickSetFrameProducer(ScTickContext* ctx, uint32_t kind, float param);

/* ---- on-rails traffic: the engine's own upstream mover ----
 * TrafficAISystem moves every agent of the OnRails tier along the lane graph each fixed step and writes its Transform
 * (src/engine/traffic/sc_traffic_ai.cpp:264-299 preamble, :434-460 on-rails branch): targetSpeed is smoothed towards the
 * lane's speed limit (smoothExp, :58-62, response 2.5), the agent advances targetSpeed * dt along its lane
 * (TrafficLaneGraph::advanceAlongLane, src/engine/traffic/sc_traffic_lanes.cpp:291-352, crossing into the best-aligned
 * connected segment, :137-156, parking on a dead end), localPos.x/z follow the lane, localRot = (0, atan2(dir.x, dir.z), 0),
 * dirty = true.  An agent without a lane (lane id 0xFFFFFFFF) first takes the nearest active one (:264-272,
 * TrafficLaneGraph::queryNearestLane, sc_traffic_lanes.cpp:240-279).  The obstacle ray and its brake (:300-345) are
 * scTickSetTrafficSensors below; without it obstacleBrake = 0, as in the reference when TrafficAIState::physics is null.
 * The Physics / Kinematic tiers are Bullet's (absent): agents in those modes are left
 * alone, their transforms arrive through the upload calls like any physics-synced body's.
 * The lane graph is handed over flat: per segment the start node's position, the direction, length, end node, active flag
 * and the speed limit of its start node (laneSpeedLimit, sc_traffic_lanes.cpp:392-400); per node its position and the
 * segments that start there (LaneNode::connections, CSR).  sin / cos of each segment's yaw are taken here with the host
 * libm, so an agent's world matrix equals the host's bit for bit: the device never evaluates a trigonometric function.
 * scTickUploadTrafficAgents gives entities a TrafficAgent + TrafficVehicle (sc_traffic_common.h:26-44): lane id
 * (0xFFFFFFFF = none: the next step looks for the nearest lane), laneS, targetSpeed, mode 0 Physics /
 * 1 Kinematic / 2 OnRails, lookAheadDist (NULL = 12).  Agents then move with scTickAdvanceMovers(dt) or as the frame
 * producer kind 2, next to SynthWorld's straight-line movers. */
typedef struct ScTickLaneGraph
{
  uint32_t segments, nodes, connections;
  const float* seg_start3;          /* [segments][3] m_nodes[startNode].pos */
  const float* seg_dir3;            /* [segments][3] LaneSegment::dir (unit) */
  const float* seg_length;          /* [segments] */
  const uint8_t* seg_active;        /* [segments], NULL = all active */
  const uint32_t* seg_end_node;     /* [segments] */
  const float* seg_speed_limit;     /* [segments] m_nodes[startNode].speedLimit */
  const float* node_pos3;           /* [nodes][3] */
  const uint32_t* node_conn_offset; /* [nodes + 1] */
  const uint32_t* node_conn;        /* [connections] segment ids, in LaneNode::connections order */
} ScTickLaneGraph;
int scTickSetLaneGraph(ScTickContext* ctx, const ScTickLaneGraph* graph);
/* TrafficLaneGraph::removeSector / re-activation (sc_traffic_lanes.cpp:164-171, :227-237) */
int scTickSetLaneActive(ScTickContext* ctx, const uint32_t* segment_ids, uint32_t count, int active);
int scTickUploadTrafficAgents(ScTickContext* ctx, uint32_t first, uint32_t count, const uint8_t* is_agent, const uint32_t* lane_id,
                              const float* lane_s, const float* target_speed, const uint8_t* mode, const float* look_ahead_dist);
int scTickReadTrafficAgents(ScTickContext* ctx, uint32_t first, uint32_t count, uint32_t* lane_id, float* lane_s,
                            float* target_speed, uint8_t* mode);
/* The traffic AI's obstacle ray (sc_traffic_ai.cpp:300-345, the branch the reference takes when TrafficAIState::physics is
 * set).  With sensors enabled every scTickRun that includes SC_TICK_BROADPHASE casts, right after the boxes of the tick are
 * binned, one ray per OnRails agent: from 1.7 m ahead of the agent's origin and 0.6 m above it, along
 * normalize(sin(yaw), 0, cos(yaw)) with the yaw's sin / cos as the entity holds them, front_ray_length long (TrafficSensors::
 * frontRayLength, 20 m), mask 1; a hit other than the agent's own box closer than safe_distance (TrafficSensors::safeDistance,
 * 10 m) leaves obstacleBrake = clamp01((safe - d) / safe) for the agent, and the next on-rails step -- scTickAdvanceMovers or
 * the frame producer, SC_TICK_PRODUCE_NEXT included -- scales its desired speed by 1 - obstacleBrake (:436).  As for the ray
 * queries below the candidates are the WORLD AABBS of the broadphase with the collision layers as uploaded (own spec: Bullet
 * is absent; an agent's own box never answers).  Order in a frame: rays from the poses of frame t against the boxes of frame
 * t, then the step to frame t+1 -- what the reference does (the ray sees Bullet's world as the last physics step left it).
 * On a TILED world the reference's ray would see the whole world, so with sensors on (switch them on before the border buffers exist:
 * scTickBindBorderBuffers* / scTickCommInit, on every tile) the border messages carry a halo section -- the sender's core-edge
 * records, a full bin per cell in fixed slots -- that lands in the receiver's ring bins, and an in-order step (scTickTileStep without
 * scTickSetPipelined, or the caller-owned split flow) casts the rays in the PAIR half, behind the merge: an agent within a ray's
 * length (at most one sector) of the tile edge brakes for a vehicle on the neighbour tile, exactly as the whole world's agents would.
 * With the step fused into the end-of-tick kernel (SC_TICK_PRODUCE_NEXT) the next frame is produced in the tick half, BEFORE these
 * rays: the brake then acts one tick later -- the reference's own ordering against Bullet's last step.  A PIPELINED tile keeps
 * the rays in the tick half and sees its own boxes only (its pair half runs under the next tick).  The brake of a run
 * without SC_TICK_BROADPHASE is the last one computed.  front_ray_length / safe_distance here are every agent's values until
 * scTickUploadTrafficSensors gives some agents their own (the reference's per-entity TrafficSensors component falls back to exactly
 * these defaults).  Needs agents (scTickUploadTrafficAgents) and a tile rectangle. */
int scTickSetTrafficSensors(ScTickContext* ctx, int enable, float front_ray_length, float safe_distance);
int scTickReadTrafficBrakes(ScTickContext* ctx, uint32_t first, uint32_t count, float* obstacle_brake);
/* Per-agent TrafficSensors (src/engine/traffic/sc_traffic_common.h:46-53; the AI reads frontRayLength / safeDistance of the agent's own
 * component, sc_traffic_ai.cpp:306-308): scTickSetTrafficSensors gives every entity the two defaults, scTickUploadTrafficSensors
 * overrides them for a range.  The whole component travels with its entity through scTickRemoveEntities, as the reference's pool
 * swap-removes it (sc_ecs.h:240-262): the two values, lastHitDistance / lastHitType, and the brake -- so a scTickAdvanceMovers between a
 * removal and the next ray tick scales a relocated agent's speed by its own last brake.  An entity appended later starts with the
 * defaults and empty last-hit values (scTickAppendEntities).  What the AI leaves in the component
 * (:339-345, read by the debug state :420-421, :479-480) comes back through scTickReadTrafficSensors: lastHitDistance -- the hit's
 * distance, or the agent's ray length without a hit -- and lastHitType -- 0 None, 2 Vehicle, 3 World; own spec like the rays:
 * Vehicle = the hit entity is a vehicle by its mover kind (a traffic agent, or a kind-1 mover: what carries a VehicleComponent,
 * :327); a box that arrived from a neighbour tile has no mover kind on this tile and counts as a vehicle when its group has the
 * dynamic bit; Self (1) does not occur because an agent's own box never answers.  Values of agents that are not OnRails, or
 * before the first ray tick, are 0. */
int scTickUploadTrafficSensors(ScTickContext* ctx, uint32_t first, uint32_t count, const float* front_ray_length, const float* safe_distance);
int scTickReadTrafficSensors(ScTickContext* ctx, uint32_t first, uint32_t count, float* last_hit_distance, uint8_t* last_hit_type);
/* TrafficDebugState::speedMultiplier (sc_traffic_ai.cpp:297-298); 1 by default */
int scTickSetTrafficSpeedMultiplier(ScTickContext* ctx, float multiplier);
/* TrafficLODSystem's tier selection (src/engine/traffic/sc_traffic_lod.cpp:269-274 threshold repair, :303-307 xz distance to
 * the player, :323-353 hysteresis, :355-417 the physics / kinematic caps -- candidates sorted by distance, descending, equal
 * distances in pool order, everything past the cap demoted): every agent's TrafficVehicle::mode becomes its desired tier.
 * The total cap (:419-465) is scTickSelectTrafficDespawns below; the despawn itself stays with the caller. */
typedef struct ScTickTierParams     /* TrafficDebugState, sc_traffic_common.h:67-75 */
{
  float tier_a_enter, tier_a_exit, tier_b_enter, tier_b_exit;   /* 50 / 70 / 110 / 150 m */
  uint32_t max_physics, max_kinematic;                          /* 24 / 64; 0 = no cap */
} ScTickTierParams;
typedef struct ScTickTierCounts { uint32_t physics, kinematic, on_rails, total; } ScTickTierCounts;   /* tierPhysics / tierKinematic / tierOnRails / totalVehicles */
int scTickSelectTrafficTiers(ScTickContext* ctx, const float player_pos[3], const ScTickTierParams* params, ScTickTierCounts* out);
/* The total cap behind the tier selection (sc_traffic_lod.cpp:419-465): with more vehicles than max_total
 * (TrafficDebugState::maxTrafficVehiclesTotal; 0 = no cap) the surplus is picked for despawning -- vehicles of the OnRails tier
 * first, then Kinematic, then Physics (the tiers as scTickSelectTrafficTiers left them), the farthest from the player first inside
 * a tier, equal distances in pool order.  *count = how many must go; their dense indices come back in that order (as many as
 * capacity holds).  The despawn itself is the caller's: scTickRemoveEntities. */
int scTickSelectTrafficDespawns(ScTickContext* ctx, const float player_pos[3], uint32_t max_total,
                                uint32_t* dense_indices, uint32_t capacity, uint32_t* count);

/* The renderer's draw order (VkRenderer::recordCommandBuffer, src/engine/src/sc_vk.cpp:1842-1864): draws whose
 * mesh handle is >= mesh_count or whose material handle has no Material are skipped, the rest sorted by
 * (Material::pipelineId, material handle, mesh handle).  pipeline_of_material[h] = pipelineId (< 128; PipelineId has
 * two values, sc_assets.h:22-26) of material handle h, 0xFF = no such material; both counts <= 2^24.  With
 * SC_TICK_DRAWS | SC_TICK_SORT_DRAWS the list scTickReadDraws returns is that sorted list.  Equal keys keep their
 * visible-list order (std::sort leaves it unspecified).  Call again when materials or meshes are created. */
int scTickSetDrawSortTable(ScTickContext* ctx, const uint8_t* pipeline_of_material, uint32_t material_count, uint32_t mesh_count);

/* ---- results (each synchronises the stream) ---- */
int scTickGetCounts(ScTickContext* ctx, ScTickCounts* out);
int scTickReadVisible(ScTickContext* ctx, uint32_t* dense_indices, uint32_t capacity, uint32_t* count);
int scTickReadCulled(ScTickContext* ctx, uint32_t* dense_indices, uint32_t capacity, uint32_t* count);
/* one bit per dense index, bit i of word i/64; set = visible candidate */
int scTickReadVisibilityBits(ScTickContext* ctx, uint64_t* words, uint32_t word_capacity);
int scTickReadWorldMatrices(ScTickContext* ctx, uint32_t first, uint32_t count, float* mat16);
int scTickReadWorldMatricesIndexed(ScTickContext* ctx, const uint32_t* dense_indices, uint32_t count, float* mat16);
int scTickReadDirty(ScTickContext* ctx, uint32_t first, uint32_t count, uint8_t* dirty);
int scTickReadPositions(ScTickContext* ctx, uint32_t first, uint32_t count, float* pos3);
int scTickReadWorldAabbs(ScTickContext* ctx, uint32_t first, uint32_t count, float* min3, float* max3);
/* pairs (a, b), a < b, unordered list; *count = pairs found.  The device keeps the list in 64 equal
 * segments (max_pairs / 64 each); at most that many pairs per segment are kept, pairs_truncated tells. */
int scTickReadPairs(ScTickContext* ctx, uint32_t* pairs2, uint32_t capacity, uint32_t* count);
int scTickReadDraws(ScTickContext* ctx, ScTickDrawItem* items, uint32_t capacity, uint32_t* count);

/* ---- per-frame read-back, overlapped with the next tick ----
 * In resident mode the engine still needs, every frame, what the renderer consumes: the visible list
 * (CullingState::visible, sc_world_partition.h:341-351), the draw items (RenderFrameData::draws, sc_ecs.h:167-173) and
 * the stats.  scTickSetFrameReadback(max_visible, max_draws) makes every scTickRun end with a small staging kernel (the
 * frame's counts, the first max_visible visible indices, the first max_draws draw items when SC_TICK_DRAWS ran, in ONE
 * device block) and ONE device-to-host copy of that block into pinned host memory, on a copy stream of the library's own:
 * the copy of frame t runs under the kernels of tick t+1.  Blocks and host buffers are double-buffered.
 * scTickAcquireFrame(frames_back) waits for the copy of ONE frame -- 0: the most recently queued, 1: the one before, which
 * is how a host overlaps: queue tick t+1, then take frame t -- and for nothing queued after it, and hands out pointers into
 * the pinned buffer; they stay valid until the second scTickRun after the one that produced the frame.
 * (0, 0) switches it off; any other call restarts the tick index at 0 and drops both frames.  Not combinable with graph replay.
 * max_visible is taken as given: visible_in_buffer never exceeds it (the block pads its index area to a multiple of four entries, so
 * that the items stay 16-byte aligned; the padding is never reported).  EVERY scTickRun ends with a frame: a run on an empty context
 * without SC_TICK_BROADPHASE, which launches nothing, leaves a frame of zeros under the next tick index. */
typedef struct ScTickFrame
{
  uint64_t tick;                   /* index of the scTickRun that produced it (counted from the first one after switching on) */
  uint32_t renderables_total, visible, culled;      /* CullingStats */
  uint32_t draws_emitted, draws_dropped, draws_sorted;
  uint32_t visible_in_buffer;      /* min(visible, max_visible) */
  uint32_t draws_in_buffer;        /* min(draws, max_draws); 0 when the run had no SC_TICK_DRAWS */
  const uint32_t* visible_indices;         /* pinned host memory */
  const ScTickDrawItem* draws;             /* pinned host memory */
} ScTickFrame;
int scTickSetFrameReadback(ScTickContext* ctx, uint32_t max_visible, uint32_t max_draws);
int scTickAcquireFrame(ScTickContext* ctx, uint32_t frames_back, ScTickFrame* out);
/* Which code wrote the last scTickRun's frame (diagnostics; no result depends on it -- every writer produces the same items and the same
 * block).  stats[0]: who wrote the draw items, stats[1]: who staged the read-back block.  Host-side: no read-back, no synchronisation.
 * The rule: a plain draw list rides in the compaction role of the combined end-of-tick launch when the tick has one
 * (SC_TICK_BROADPHASE with its pair search in the same run, SC_TICK_CULL) -- into the draw buffer, or, with the read-back on and
 * 0 < draw budget <= max_draws, straight into the block, header included; with the read-back on and such a budget but no combined launch
 * (no broadphase, a quiet tick, SC_TICK_SPLIT_PAIRS) one emission kernel writes items and block; otherwise the emission kernel or the
 * sort writes the draw buffer and a staging kernel copies its head into the block.  An empty context without SC_TICK_BROADPHASE launches
 * nothing: the library writes that frame -- zeros under the next tick index -- itself. */
#define SC_TICK_FRAME_ITEMS_NONE 0u          /* the run had no SC_TICK_DRAWS, or launched nothing (an empty context, below) */
#define SC_TICK_FRAME_ITEMS_EOT_BUFFER 1u    /* compaction role of the end-of-tick launch, into the draw buffer */
#define SC_TICK_FRAME_ITEMS_EOT_BLOCK 2u     /* ... into the read-back block */
#define SC_TICK_FRAME_ITEMS_EMIT 3u          /* the emission kernel, into the draw buffer */
#define SC_TICK_FRAME_ITEMS_EMIT_STAGED 4u   /* the staged emission kernel, into the read-back block */
#define SC_TICK_FRAME_ITEMS_SORT 5u          /* SC_TICK_SORT_DRAWS: the sort, into the draw buffer */
#define SC_TICK_FRAME_BLOCK_NONE 0u          /* the read-back is off */
#define SC_TICK_FRAME_BLOCK_EOT 1u           /* compaction role of the end-of-tick launch */
#define SC_TICK_FRAME_BLOCK_EMIT_STAGED 2u   /* the staged emission kernel */
#define SC_TICK_FRAME_BLOCK_STAGE 3u         /* the staging kernel */
#define SC_TICK_FRAME_BLOCK_HOST 4u          /* an empty context: no launch, the library wrote the zero frame */
int scTickGetFrameStats(ScTickContext* ctx, uint32_t stats[2]);

/* ---- bind runs of the sorted draw list, and the material touch set ----
 * What a renderer does with the sorted list, found on the device behind the sort.  The specification is the reference's own loop and
 * its own touchMaterial, not one of this build's.
 *
 * RUNS.  VkRenderer::recordCommandBuffer walks the sorted list, binds the pipeline when it changes, the material's descriptor set when
 * it changes, the mesh buffers when they change, and issues one vkCmdDrawIndexed per item (src/engine/src/sc_vk.cpp:1866-1911).  A run
 * is a maximal stretch of equal key (pipeline, material, mesh) in the first draws_sorted items of the list scTickReadDraws returns.  The
 * runs come in list order: `first` ascends, the counts sum to draws_sorted.  A host that instances issues one instanced or indirect draw
 * per run instead of `count` draws.  `binds` is the state machine of that loop (:1866-1907): run 0 has all three bits; for every later
 * run, against the run before it,
 *     bit 0  bind pipeline   `pipeline` differs (boundPipeline != targetPipeline, which also resets boundMesh and boundMaterial)
 *     bit 1  bind material   bit 0 is set, or `material` differs
 *     bit 2  bind mesh       bit 0 is set, or `mesh` differs
 * so two adjacent runs with different materials and the same mesh do NOT bind the mesh again -- the sort order produces that case.
 * PipelineId has two values, each mapped to its own VkPipeline (sc_assets.h:22-26): comparing ids is comparing pipelines.
 * A mesh whose indexCount is 0 is skipped by the reference before its mesh bind (:1898-1899).  The library does not know index counts:
 * a consumer that skips such runs reproduces the reference's binds (the only adjacent run with the same mesh is empty as well).
 * Equal keys keep the order of the stable sort (scTickSetDrawSortTable); the reference's std::sort leaves it unspecified.
 *
 * TOUCHES.  RenderPrepStreamingSystem calls assets->touchMaterial(rm->materialId) for every draw it emits (sc_world_partition.cpp:
 * 1322-1326), which keeps the texture streamer's LRU alive (sc_assets.cpp:441-455).  Bit h of the bitmap is set if and only if some
 * EMITTED draw -- the first draws_emitted entries of the visible list: behind the budget, before the renderer's filter -- has
 * materialId == h and h < material_count.  Like touchMaterial (sc_assets.cpp:441-445) it does not care whether the draw's mesh handle is
 * valid and ignores handles past the table; a handle below material_count whose table entry is 0xFF is touched all the same.  Draws
 * dropped by the budget touch nothing.  touchMesh is an empty function in the reference (sc_assets.h:151): there is no mesh bitmap.
 * The bitmap is rebuilt from zero on every flagged run; material_count is the one of the last scTickSetDrawSortTable.
 *
 * scTickSetBindRuns(max_runs) sizes the run table (0 = off, frees it); it needs scTickSetDrawSortTable first and drops captured graphs.
 * A later scTickSetDrawSortTable with another material_count resizes the bitmap.  scTickRun with SC_TICK_BIND_RUNS fails without
 * scTickSetBindRuns and without SC_TICK_DRAWS | SC_TICK_SORT_DRAWS in the same run.  The launches sit behind the sort on the tick's
 * stream and replay from a captured graph; a run without the flag launches what it launched before this call existed. */
typedef struct ScTickBindRun            /* 24 bytes */
{
  uint32_t first, count;                /* items [first, first+count) of the sorted list scTickReadDraws returns */
  uint32_t pipeline, material, mesh;    /* the run's key */
  uint32_t binds;                       /* bit 0: bind pipeline, bit 1: bind material, bit 2: bind mesh -- before this run's first draw */
} ScTickBindRun;
typedef struct ScTickBindInfo
{
  uint32_t runs;               /* runs found (may exceed max_runs; the table then holds the first max_runs) */
  uint32_t runs_truncated;     /* 1 if runs > max_runs */
  uint32_t draws;              /* == ScTickCounts::draws_sorted: sum of count over ALL runs */
  uint32_t pipeline_binds, material_binds, mesh_binds;   /* over ALL runs, truncated or not */
  uint32_t materials_touched;  /* set bits of the touch bitmap */
  uint32_t touch_words;        /* (material_count + 31) / 32 at the time of the run */
} ScTickBindInfo;
int scTickSetBindRuns(ScTickContext* ctx, uint32_t max_runs);
/* results of the last scTickRun(... | SC_TICK_BIND_RUNS); each synchronises.  runs may be NULL with capacity 0: min(info->runs,
 * max_runs, capacity) rows are written.  words: bit h % 32 of word h / 32; *word_count = touch_words, min(that, word_capacity) are written. */
int scTickReadBindRuns(ScTickContext* ctx, ScTickBindRun* runs, uint32_t capacity, ScTickBindInfo* info);
int scTickReadMaterialTouches(ScTickContext* ctx, uint32_t* words, uint32_t word_capacity, uint32_t* word_count);
/* Overlapped read-back, next to scTickSetFrameReadback: with both switched on (in either order; switching either on or off
 * reallocates) every run with SC_TICK_BIND_RUNS stages report, table and bitmap into a double-buffered block of their own, copied on
 * the frame's copy stream behind the frame's block: scTickAcquireFrame and scTickAcquireFrameBinds of one frame wait on the same event.
 * A run without the flag stages nothing: its runs_in_buffer is 0 and its info all zeros.  Fails without both features. */
typedef struct ScTickFrameBinds
{
  uint64_t tick;                        /* == ScTickFrame::tick of the same frames_back */
  ScTickBindInfo info;
  uint32_t runs_in_buffer;              /* min(info.runs, max_runs); 0 when the run had no SC_TICK_BIND_RUNS */
  const ScTickBindRun* runs;            /* pinned host memory, valid as long as the frame's own pointers */
  const uint32_t* touch_words;          /* info.touch_words words */
} ScTickFrameBinds;
int scTickAcquireFrameBinds(ScTickContext* ctx, uint32_t frames_back, ScTickFrameBinds* out);

/* ---- host-side helpers (no GPU work) ----
 * CameraSystem stays on the host (O(#cameras), sc_ecs.cpp:213-272).  These restate the four sc_math
 * functions it and the editor use (sc_math.h:31-58) with the reference's libm calls and operation
 * order, for callers that do not link the engine's own sc_math.  Column-major Mat4, m[c*4+r]. */
int scTickHostMat4Mul(const float a[16], const float b[16], float out[16]);                        /* sc_math.cpp:11-85 */
int scTickHostMat4Trs(const float pos[3], const float rot[3], const float scale[3], float out[16]); /* :130-142 */
int scTickHostMat4Inverse(const float a[16], float out[16]);                                        /* :144-207 */
int scTickHostMat4PerspectiveRhZo(float fov_y_radians, float aspect, float z_near, float z_far,
                                  int flip_y, float out[16]);                                       /* :209-232 */
/* viewProj = perspective(fovY*pi/180, aspect, near, far, flipY) * inverse(cameraWorld), sc_ecs.cpp:261-270 */
int scTickHostCameraViewProj(const float camera_world[16], float fov_y_degrees, float aspect,
                             float z_near, float z_far, float out_view_proj[16]);
/* 1 when no parent link crosses a boundary between runs of `span` consecutive dense indices (parent[i] / span == i / span for every
 * entity with a parent; negative or out-of-range entries are no links), else 0 -- the rule scTickGetTailStats reports on. */
int scTickHostSpanClosed(const int32_t* parent, uint32_t count, uint32_t span);
/* The rule behind scTickGetTopologyClassStats, on its own: for a parent array (SC_TICK_NO_PARENT = none) and one flag byte per entity (bit 0
 * has RenderMesh, bit 1 has Bounds, bits 2 / 3 / 4 rotation about X / Y / Z trivial; other bits ignored), tile_class[t] of every run t of 64
 * consecutive indices (ceil(count / 64) entries; the last run is clipped to count) = the number of its pattern from 1, in order of first
 * appearance, or 0 when the run is not closed -- a parent outside the run, more than three ancestors, a cycle, an entry that names no other
 * entity of the world -- or when its pattern would be number max_patterns + 1 (max_patterns <= 256).  *pattern_count = the patterns numbered.
 * pattern_words (may be null; [max_patterns][64]): every pattern's words -- bits 0..23 the parent's position in the run or 0xFFFFFF for
 * none, bit 24 / 25 RenderMesh / Bounds, bits 26..28 depth, bits 29..31 trivial axes; positions past count carry 7 << 26 | 0xFFFFFF. */
int scTickHostTopologyClasses(const int32_t* parent, const uint8_t* flags, uint32_t count, uint32_t max_patterns,
                              uint16_t* tile_class, uint32_t* pattern_count, uint32_t* pattern_words);

/* ---- sector data (.scsector) and residency: the callers either side of the tick ----
 * Host-side reader of the editor/streamer sector format, tools/shared/world_format.cpp:185-338 (ReadSectorFile;
 * record layout as written by WriteSectorFile :76-181), straight into SoA arrays the upload calls take.
 * All versions the reference reads are read the same way: the INST record size is derived from the chunk size,
 * names / texture overrides are present when the record is long enough (:219-230), extra record bytes are
 * skipped, unknown chunks are skipped by their size, zero-sized chunk headers are ignored, and known chunks are
 * parsed by their own counts.  A file that ends early leaves the remaining fields at the reference's defaults
 * (id 0, scale 1, empty name), as its ifstream reads do; info->truncated tells. */
typedef struct ScTickSectorInfo
{
  uint32_t version;                /* SectorFile::version (kSectorVersion = 4, world_format.h:13) */
  int32_t  sector_x, sector_z;     /* SectorFile::sector */
  uint32_t instances;              /* records in the file (may exceed what was stored: see capacity) */
  uint32_t lanes, lane_points, spawners, colliders;
  uint32_t truncated;              /* 1 = the data ended inside a header, count or record */
} ScTickSectorInfo;

typedef struct ScTickSectorInstances
{
  uint32_t capacity;               /* records each non-NULL array below can hold; the first `capacity` are stored */
  uint64_t* id;                    /* Instance::id */
  uint64_t* model_id;              /* 0 for version < 4 */
  uint64_t* mesh_id;               /* asset ids (HashAssetPath), resolved to handles by the caller (:746-792 of sc_world_partition.cpp) */
  uint64_t* material_id;
  uint64_t* albedo_texture_id;     /* 0 unless the record carries overrides */
  uint32_t* material_flags;
  uint32_t* tags;
  float* pos3; float* rot3; float* scale3;     /* Instance::transform, [capacity][3] each: what setLocal takes */
  char* name64;                    /* [capacity][64], NUL-terminated (kInstanceNameMax) */
} ScTickSectorInstances;

/* 0 = not a sector file (bad magic / shorter than the magic) or NULL arguments; `out` may be NULL to only fill info */
int scTickSectorParse(const void* data, uint64_t size, ScTickSectorInfo* info, const ScTickSectorInstances* out);
int scTickSectorReadFile(const char* path, ScTickSectorInfo* info, const ScTickSectorInstances* out);
/* AssetId of a path: FNV-1a 64 (with the reference's non-standard starting value) over the lexically normalised, '/'-separated, lower-cased path (world_format.cpp:52-74); 0 for NULL */
uint64_t scTickHashAssetPath(const char* path);
/* "<root>/sectors/sector_<x>_<z>.scsector" (world_format.cpp:382-389); returns the length needed (excluding NUL) */
uint32_t scTickSectorPath(const char* world_root, int32_t x, int32_t z, char* out, uint32_t capacity);

/* Sector activation (WorldPartition::pumpCompletedLoads, sc_world_partition.cpp:916-958): `count` entities are
 * created at the END of the Transform pool's dense order (ComponentPool::add, sc_ecs.h:203-221) with setLocal
 * (dirty), a RenderMesh, Bounds (NULL min/max = the unit cube kUnitCubeBounds, :27) and collision layers (NULL =
 * group/mask all).  parent = NULL: all roots, nothing else is touched (O(count) work); otherwise dense indices
 * (earlier entities or this batch) and the hierarchy is re-linked.  *first_index = dense index of the first one.
 * An appended entity is no mover and no traffic agent, whoever held its slot before; once scTickSetTrafficSensors has been called
 * its TrafficSensors are a new component's (sc_traffic_common.h:46-53): the context's defaults for front_ray_length / safe_distance,
 * lastHitDistance 0, lastHitType None, brake 0 -- also while the sensors are switched off. */
int scTickAppendEntities(ScTickContext* ctx, uint32_t count, const float* pos3, const float* rot3, const float* scale3,
                         const float* bounds_min3, const float* bounds_max3,
                         const uint32_t* mesh_id, const uint32_t* material_id,
                         const uint32_t* group, const uint32_t* mask, const int32_t* parent, uint32_t* first_index);
/* Despawn (WorldPartition::pumpUnloadQueue -> World::destroy, sc_world_partition.cpp:963-990, sc_ecs.cpp:28-42):
 * `count` distinct entities, named by their dense indices AT THE TIME OF THE CALL, are removed one after the other
 * with the pool's swap-remove (the last entity moves into the hole, sc_ecs.h:240-262), so the dense order afterwards
 * is the reference's.  Children of a removed entity become dirty roots (sc_ecs.cpp:151-160).  The net relocations
 * are returned: entity that was at moved_from[k] is now at moved_to[k] (arrays of `count`; may be NULL).
 * Device cost is O(count) unless a removed or relocated entity has children (then the hierarchy is re-linked). */
int scTickRemoveEntities(ScTickContext* ctx, const uint32_t* dense_indices, uint32_t count,
                         uint32_t* moved_from, uint32_t* moved_to, uint32_t* moved_count);

/* ---- ray queries over the broadphase bins ----
 * A batch of rays answered inside the tick, after the bins are filled and before the pair search consumes them --
 * what the traffic AI asks once per agent and frame (sc_traffic_ai.cpp:319, :644) and the vehicle camera once
 * (sc_vehicle.cpp:600).  Shaped like PhysicsWorld::raycast (src/engine/physics/sc_physics.cpp:740-777): the
 * direction is normalised the same way (no hit when |dir|^2 <= 1e-6), the segment runs from origin to
 * origin + ndir * max_dist, a box takes part when (group & mask) != 0 and its own mask is not empty (Bullet's default
 * filter with the callback's group 0xFFFF), the closest hit wins.  The reference tests Bullet's exact shapes; here the
 * candidates are the world AABBs of the broadphase, tested with the reference's own slab arithmetic
 * (intersectRayAABB, tools/world_editor/editor_core/editor_core.cpp:438-470); equal distances go to the lower id.
 * On a tiled world a context answers for the boxes registered in its own sectors, which includes the neighbours' boxes
 * that reach into them (the queries run after the border merge); the part of a ray beyond the tile is the neighbour's.
 * The answer equals brute force over every registered box with that slab test, hits at t == max_dist included: the sector walk
 * is padded by the roundings of the segment's end, so a box whose face lies an ulp past it, across a sector boundary, is found. */
typedef struct ScTickRayHit     /* RaycastHit, sc_physics.h:106-114 */
{
  uint32_t hit;                /* 0 / 1 */
  uint32_t id;                 /* rank << 24 | dense index of the box that was hit (0xFFFFFFFF: none) */
  float    distance;           /* along the normalised direction */
  float    position[3];        /* origin + ndir * distance */
  float    normal[3];          /* axis normal of the face the ray entered through; (0,1,0) when it starts inside the box */
  uint32_t layer;              /* the box's collision group */
  uint32_t pad[2];
} ScTickRayHit;
/* origin3 / dir3: [count][3]; max_dist, mask: [count].  The set stays until it is replaced (count 0 clears it).  Fails -- and leaves
 * the previous set in place -- when an origin, a direction or a max_dist is not finite, or a direction's squared length
 * (x*x + y*y) + z*z overflows fp32.  A negative max_dist and a direction of |dir|^2 <= 1e-6 are accepted and answered with a miss. */
int scTickSetRayQueries(ScTickContext* ctx, uint32_t count, const float* origin3, const float* dir3,
                        const float* max_dist, const uint32_t* mask);
/* results of the last scTickRun(... | SC_TICK_BROADPHASE | SC_TICK_RAYS) (after scTickRunPairs on a tiled world) */
int scTickReadRayHits(ScTickContext* ctx, ScTickRayHit* hits, uint32_t capacity, uint32_t* count);

/* ---- capsule sweeps over the broadphase bins ----
 * A batch of upright-capsule sweeps answered where the rays are: after the bins are filled (on a tiled world: after the border
 * merge) and before the pair search consumes them.  Shaped like PhysicsWorld::sweepCapsule (src/engine/physics/sc_physics.h:179,
 * sc_physics.cpp:779-810), which sweeps btCapsuleShape(radius, 2 * halfHeight) through Bullet's exact shapes.  Bullet is not in
 * the tree, so -- as for the rays -- this is this build's OWN SPEC: the candidates are the broadphase's world AABBs, the sweeper is
 * the capsule's own AABB, and a box swept against a box is a ray against the box grown by the sweeper's half extents: the slab
 * arithmetic is intersectRayAABB again (editor_core.cpp:438-470).
 * All arithmetic is fp32, unfused, left to right, with correctly rounded / and sqrt.  For (start, end, radius, half_height, mask, skip_id):
 *   sweeper     hh = (half_height > 0) ? half_height : 0;   e = (radius, hh + radius, radius)
 *   segment     d = end - start;  lenSq = (d.x*d.x + d.y*d.y) + d.z*d.z;
 *               lenSq > 1e-6:  far = sqrt(lenSq), inv = 1 / far, ndir = d * inv
 *               otherwise an OVERLAP test at start: ndir = (0,0,0), far = 0 (every axis of the slab test is then containment, closed)
 *   candidates  every record the ray queries see, under their filter -- (group & mask) != 0 and the proxy's own mask not empty --
 *               applied before the box is touched; a box whose id == skip_id never answers (0xFFFFFFFF: none)
 *   test        lo' = lo - e, hi' = hi + e per component, then the rays' slab test of (start, ndir, far) against (lo', hi');
 *               the smallest t wins, equal t goes to the lower id
 * On a tiled world the rays' rule holds: a context answers for the boxes registered in its own sectors (the neighbours' boxes that
 * reach into them included); the part of a sweep beyond the tile is the neighbour's.  A pipelined tile sees what its rays see.
 * The answer equals brute force over every registered box with that test, hits at t == far and the closed containment of an overlap
 * test included: the sector walk reaches the sweeper's radius and the roundings of the segment's end beyond the segment. */
typedef struct ScTickSweepHit   /* SweepHit, sc_physics.h:116; laid out like ScTickRayHit */
{
  uint32_t hit;                /* 0 / 1 */
  uint32_t id;                 /* rank << 24 | dense index of the box that was hit (0xFFFFFFFF: none) */
  float    distance;           /* the hit FRACTION of the sweep, t / far (SweepHit::distance = m_closestHitFraction, sc_physics.cpp:801); 0 when far == 0 */
  float    position[3];        /* start + ndir * t: the capsule's CENTRE at the hit -- not Bullet's contact point */
  float    normal[3];          /* axis normal of the grown box's face the centre entered through; (0,1,0) when the sweep starts in overlap (t = 0) */
  uint32_t layer;              /* the box's collision group */
  float    travel;             /* t in metres */
  uint32_t pad;
} ScTickSweepHit;              /* a miss is SweepHit{}: id 0xFFFFFFFF, normal (0,1,0), zeros */
#ifdef __cplusplus
static_assert(sizeof(ScTickSweepHit) == 48, "ScTickSweepHit is 48 bytes, like ScTickRayHit");
#else
_Static_assert(sizeof(ScTickSweepHit) == 48, "ScTickSweepHit is 48 bytes, like ScTickRayHit");
#endif
/* start3 / end3: [count][3]; radius, half_height, mask: [count]; skip_id: [count] or NULL (none).  The set stays until it is replaced
 * (count 0 clears it).  Fails -- and leaves the previous set in place -- when a start, end, radius or half_height is not finite, a
 * radius is negative, or a segment's squared length overflows fp32. */
int scTickSetSweepQueries(ScTickContext* ctx, uint32_t count, const float* start3, const float* end3, const float* radius,
                          const float* half_height, const uint32_t* mask, const uint32_t* skip_id);
/* results of the last scTickRun(... | SC_TICK_BROADPHASE | SC_TICK_SWEEPS) (after scTickRunPairs on a tiled world) */
int scTickReadSweepHits(ScTickContext* ctx, ScTickSweepHit* hits, uint32_t capacity, uint32_t* count);

/* ---- entity-anchored rays over the broadphase bins ----
 * Rays that follow an entity on the device.  scTickSetRayQueries takes world-space rays and replacing them costs a learn tick and a
 * fresh graph capture; the callers the ray section cites do not have world-space rays: the vehicle camera's occlusion ray starts behind
 * the vehicle along a direction fixed in its frame (sc_vehicle.cpp:570-611), the raycast vehicle's wheel probes are chassis-local by
 * definition (VehicleWheelConfig::connectionPoint / direction, sc_physics.h:63-72; their answers are what getVehicleTelemetry reports,
 * sc_physics.cpp:1034-1055), the traffic debug sensor ray rides on a moving agent (sc_traffic_ai.cpp:622-652) -- and in resident mode
 * the entity's pose of this frame exists only on the device.  An anchored ray is given once, in its anchor's LOCAL frame; every tick the
 * kernel that casts it resolves it against that tick's world matrix of the anchor and answers it against that tick's boxes.  The frame
 * loop makes no host round trip, runs no learn tick and re-captures no graph.
 * This build's OWN SPEC, like the rays and the sweeps.  All arithmetic is fp32, unfused, left to right.  For ray k with anchor a, local
 * origin l, local direction v, and R_r = (w_r.x, w_r.y, w_r.z, w_r.w) row r (0..2) of a's world matrix as this run's transform stage
 * leaves it (without SC_TICK_XFORM: as it stands on the device):
 *   o_r = ((R_r.x*l.x + R_r.y*l.y) + R_r.z*l.z) + R_r.w
 *   d_r =  (R_r.x*v.x + R_r.y*v.y) + R_r.z*v.z
 * The ray (o, d, max_dist, mask) is then answered exactly as a ray of scTickSetRayQueries: same normalisation (|d|^2 <= 1e-6 is a miss),
 * same filter, same slab arithmetic, same tie rule, same ScTickRayHit with the pad words 0.
 *   max_dist    world metres along the NORMALISED direction; the anchor's scale does not scale it
 *   skip_self   != 0 (NULL: every ray): the box with id (rank << 24 | a), the anchor's own, never answers
 *   anchor      SC_TICK_ANCHOR_NONE: no anchor, l and v are world space and go through untouched -- the answer equals the plain ray
 *               query's bit for bit
 *   a miss      (RaycastHit{}: id 0xFFFFFFFF, normal (0,1,0), zeros) when the anchor is >= the entity count at run time (a dead anchor
 *               always is), when a resolved origin is not finite, or when the resolved direction's squared length
 *               (d.x*d.x + d.y*d.y) + d.z*d.z is not finite
 * On a tiled world the rays' rule holds: the cast runs behind the border merge and a context answers for the boxes registered in its own
 * sectors (the neighbours' boxes that reach into them included).  In a split flow the tick half resolves the rays into a snapshot of
 * its tick parity and the pair half casts from it -- a pipelined tile's matrices may be the next tick's by then; the arithmetic is the
 * same, so are the bits.  A pipelined tile sees what its rays see.
 * Residency: scTickRemoveEntities renames the anchors of relocated entities (moved_from -> moved_to) and turns the anchors of removed
 * entities into SC_TICK_ANCHOR_DEAD, which always misses; O(rays) per call, no learn tick of its own.  scTickAppendEntities and
 * scTickSetEntityCount leave the anchors alone: an anchor beyond a shrunken count simply misses. */
#define SC_TICK_ANCHOR_NONE 0xFFFFFFFFu   /* anchor[k]: the ray is world space */
#define SC_TICK_ANCHOR_DEAD 0xFFFFFFFEu   /* what scTickReadAnchoredRays reports for a ray whose anchor was removed */
/* anchor, max_dist, mask: [count]; local_origin3 / local_dir3: [count][3]; skip_self: [count] or NULL (all 1).  The set stays until it is
 * replaced (count 0 clears it).  A call with THE SAME COUNT as the current set only rewrites the device arrays, behind whatever is queued:
 * no learn tick, and a captured graph stays valid; another count behaves like scTickSetRayQueries.  Fails -- and leaves the previous set
 * in place -- when a local origin, local direction or max_dist is not finite, a max_dist is negative, a required array is NULL, or
 * scTickRunPairs is pending. */
int scTickSetAnchoredRays(ScTickContext* ctx, uint32_t count, const uint32_t* anchor, const float* local_origin3,
                          const float* local_dir3, const float* max_dist, const uint32_t* mask, const uint8_t* skip_self);
/* results of the last scTickRun(... | SC_TICK_BROADPHASE | SC_TICK_ANCHORED_RAYS) (after scTickRunPairs on a tiled world) */
int scTickReadAnchoredRayHits(ScTickContext* ctx, ScTickRayHit* hits, uint32_t capacity, uint32_t* count);
/* the anchors of rays first .. first + count - 1 as they stand now (after removals); host-side, no read-back */
int scTickReadAnchoredRays(ScTickContext* ctx, uint32_t first, uint32_t count, uint32_t* anchor);

/* ---- exact shapes for rays: oriented box, sphere, capsule ----
 * The ray queries and the entity-anchored rays answer from the broadphase's WORLD AABBs; a box yawed by 45 degrees is then as wide as its
 * diagonal and a sphere answers at the face of its bounding cube.  scTickSetRayShapes(SC_TICK_RAY_SHAPES_EXACT) makes the runs with
 * SC_TICK_RAYS and SC_TICK_ANCHORED_RAYS answer a candidate whose proxy comes from a typed collider (scTickUploadColliders: BOX, SPHERE,
 * CAPSULE) by the shape itself, taken through the entity's world matrix of this tick.  The AABB test stays as the pre-filter; the sector
 * walk, the filter, the skip rule, the tie rule and ScTickRayHit are what they were.  Capsule sweeps (which have a mode of their own: "exact shapes for capsule sweeps"),
 * the traffic AI's front rays, scTickQueryOccupied and the pair search do not change: they see AABBs in either mode.
 * This build's OWN SPEC, like the rays.  All arithmetic is fp32, unfused, left to right, with correctly rounded / and sqrt;
 * dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 * A candidate record passes the filter and the skip test, then the slab test against its AABB (dir: the normalised direction, L: max_dist).
 *   An AABB miss: the candidate does not answer, in both modes.
 *   An AABB hit in EXACT mode is REFINED when colliders were uploaded, the id's rank is this context's, e = id & 0xFFFFFF is below the
 *   entity count and the collider type of e is BOX, SPHERE or CAPSULE.  Otherwise the AABB answer stands, bit for bit as in AABB mode:
 *   BOUNDS proxies, a neighbour tile's border records, a context without colliders, and the degenerate box matrices named below.
 * With R_r = row r (0..2) of e's world matrix as this run's transform stage leaves it:
 *   c_k = (R_0[k], R_1[k], R_2[k]) column k (0..2);  T = (R_0.w, R_1.w, R_2.w);  n_k = dot(c_k, c_k);  q = o - T;
 *   (ex, ey, ez, radius) = the collider's record: a box's half extents, (0, 0, 0, radius) for a sphere, (0, max(0, half_height), 0, radius)
 *   for a capsule.
 * "Inside" always means hit, t = +0, normal (0,1,0): the rule for a ray that starts inside a box.  Every reported t is (t > 0) ? t : +0,
 * never -0.  Every acceptance below is a positive comparison (t <= L, disc >= 0, ...): a NaN is a miss.
 *   BOX       some n_k not > 0 or not finite: the AABB answer stands.  Otherwise lo_k = dot(c_k, q) / n_k, ld_k = dot(c_k, dir) / n_k and
 *             s = the slab test of (lo, ld, L) against (-(ex,ey,ez), +(ex,ey,ez)) -- the same routine, parallel-axis rule included.
 *             A miss: the candidate does not answer.  t = s.t.  Face axis a < 3: sgn = ld_a > 0 ? -1 : 1, inv = 1 / sqrt(n_a),
 *             normal_r = sgn * (c_a[r] * inv) + 0   (the addition of +0 makes a zero component +0 whatever the sign: an axis-aligned
 *             box reports the AABB answer's bits).  No face (the origin is inside): inside.
 *   roundHit(qc, R)   b = dot(qc, dir);  c = dot(qc, qc) - R*R;  c <= 0: inside.  Require b < 0, else miss.  disc = b*b - c; require
 *             disc >= 0, else miss.  t = (-b) - sqrt(disc), clamped as above; require t <= L, else miss.  normal_r = (qc_r + dir_r*t) / R.
 *   SPHERE    R = radius * sqrt(max(n_0, n_1, n_2)), the maximum selected as the collider's AABB selects it: m = (n_2 < n_1) ? n_1 : n_2,
 *             then (n_0 < m) ? m : n_0.  The answer is roundHit(q, R).
 *   CAPSULE   hh = ey;  R = radius * sqrt((n_0 < n_2) ? n_2 : n_0);  A = c_1 * hh per component;  aa = dot(A, A).
 *             Not aa > 0: the answer is roundHit(q, R).  Otherwise
 *               ad = dot(A, dir); aq = dot(A, q); dq = dot(dir, q); qq = dot(q, q);
 *               ka = aa - ad*ad;  kb = aa*dq - aq*ad;  kc = (aa*qq - aq*aq) - (R*R)*aa;
 *             inside the body: kc <= 0 and -aa <= aq and aq <= aa.
 *             side: needs kc > 0, ka > 0, kb < 0 (the ray approaches the axis: with kb >= 0 both roots lie behind the origin) and
 *               disc = kb*kb - ka*kc >= 0;  tb = ((-kb) - sqrt(disc)) / ka, clamped;  yb = aq + tb*ad;  valid when -aa <= yb, yb <= aa
 *               and tb <= L;  normal_r = ((q_r + dir_r*tb) - A_r*(yb/aa)) / R.
 *             caps: roundHit(q + A, R) and roundHit(q - A, R).
 *             Any inside among body and caps: inside.  Otherwise the smallest t among the valid of side, cap q + A, cap q - A, in that
 *             order, a later one replacing an earlier one only when strictly smaller.  None valid: the candidate does not answer.
 * Among candidates the smallest t wins -- refined or standing alike -- and equal t goes to the lower id; position = o + dir*t, layer and
 * id as in AABB mode, the pad words 0.
 * For a matrix whose columns are mutually orthogonal (every root, every chain under uniformly scaled parents) this is the shape itself:
 * the box with half extents e_k * |c_k|, the sphere and the capsule's round part scaled by the largest column they span.  For a sheared
 * matrix it is the shape in the frame these formulas define.
 * The mode is a property of the context and stays until it is changed (default AABB).  Setting it drops captured graphs and asks for no
 * learn tick: the bins are not concerned.  It fails on an unknown mode and while scTickRunPairs is pending.  A run with SC_TICK_RAYS or
 * SC_TICK_ANCHORED_RAYS in EXACT mode fails on a pipelined context (scTickSetPipelined / scTickSetPairsStream): by the time its rays are
 * cast the matrices may be the next tick's.  In-order tiles (scTickTileStep) and the caller-owned split flow work, with ONE RESTRICTION on
 * the latter: the pair half refines against the matrix rows, the collider records and the dense indices as they stand when scTickRunPairs
 * runs (the bins hold tick t's boxes; nothing holds tick t's shapes, and the snapshot of the anchored rays holds the resolved ray, not the
 * candidates).  So between scTickRun(.. | SC_TICK_SPLIT_PAIRS) with SC_TICK_RAYS or SC_TICK_ANCHORED_RAYS in EXACT mode and its
 * scTickRunPairs, the calls that rewrite one of them fail with a last-error text and change nothing: scTickUploadWorldMatrices,
 * scTickUploadColliders, scTickRemoveEntities, scTickSetEntityCount and scTickRun with SC_TICK_XFORM.  Everything else a host does in the
 * gap -- locals, positions, layers, bounds, appends, read-backs -- is the next tick's and is welcome; in AABB mode, and for a pending tick
 * without ray flags, the gap is as free as before.  A context that never calls scTickSetRayShapes launches exactly the kernels it launched
 * before. */
enum { SC_TICK_RAY_SHAPES_AABB = 0, SC_TICK_RAY_SHAPES_EXACT = 1 };
int scTickSetRayShapes(ScTickContext* ctx, uint32_t mode);   /* default SC_TICK_RAY_SHAPES_AABB */
int scTickGetRayShapes(ScTickContext* ctx, uint32_t* mode);

/* ---- pair events: the tick-to-tick difference of the pair set ----
 * What a broadphase hands its narrow phase besides "the pairs of this tick": Bullet's btDbvtBroadphase (behind sc_physics.cpp:218-225) keeps
 * an overlapping-pair cache and reports pairs as they are ADDED and REMOVED (btOverlappingPairCache::addOverlappingPair /
 * removeOverlappingPair).  scTickReadPairs returns the whole set on every tick; a host that keeps contact caches or trigger enter / exit
 * would diff two such lists on the CPU.  With pair events the device remembers the set and reports the difference.  This build's OWN SPEC:
 *   scTickSetPairEvents(max_tracked_pairs, max_events) enables them (and sizes every buffer; (0, 0) switches them off and frees the buffers).
 *   The context then remembers the pair set of the last run that carried SC_TICK_PAIR_EVENTS.  A run with the flag reports
 *     begun   the pairs of this tick's set that are not in the remembered set
 *     ended   the pairs of the remembered set that are not in this tick's set
 *   and then remembers its own set.  Pairs look as in scTickReadPairs: ids a < b, id = rank << 24 | dense index.  The order inside a list
 *   is unspecified.  Runs without the flag leave the remembered set alone: the next flagged run diffs against the last flagged one.
 *   RESYNC     begun = every pair of this tick, ended = nothing, resync = 1: on the first flagged run after enabling, after anything that
 *              renames or invalidates dense indices (scTickRemoveEntities, a shrinking scTickSetEntityCount), and after an overflow tick.
 *              Appending entities forces no resync, nor do topology, layer or collider uploads: their effect arrives as ordinary events.
 *   OVERFLOW   this tick's set does not fit max_tracked_pairs, or the pair list itself was truncated (ScTickCounts::pairs_truncated):
 *              overflow = 1, both lists empty with counts 0 (tracked and resync 0 too), the remembered set is dropped; the next flagged
 *              run that fits is a resync tick.
 *   TRUNCATED  more than max_events pairs begin, or end: begun / ended carry the true totals, each list holds max_events valid members,
 *              events_truncated = 1.  The remembered set is complete all the same -- the next tick's events are right -- and the host
 *              recovers this tick with scTickReadPairs.
 *   Nothing is lost silently: every loss sets one of the three flags.
 * The events are formed on the device behind the pair search, on its stream (after scTickRunPairs in a split flow): no host round trip,
 * and the launches replay from a captured graph.  Device memory: two tables of slots x 8 bytes, slots = the power of two >=
 * 2 x max_tracked_pairs, plus slots / 4 bytes of marks, plus 2 x max_events x 8 bytes.  A context that never enables them allocates and
 * launches exactly what it did without this call.
 * scTickRun / scTickTileStep fail for SC_TICK_PAIR_EVENTS without SC_TICK_BROADPHASE, without a prior scTickSetPairEvents, or on a
 * pipelined context (scTickSetPipelined / scTickSetPairsStream: its tick parities overlap in time).  scTickReadPairEvents fails when the
 * last run did not carry the flag and while scTickRunPairs is pending. */
typedef struct ScTickPairEventInfo
{
  uint32_t begun, ended;       /* pairs that begun / ended this tick (true totals: may exceed max_events, and the caller's capacities) */
  uint32_t tracked;            /* size of the remembered set after this tick */
  uint32_t resync;             /* 1 = nothing was remembered: begun is this tick's whole set */
  uint32_t overflow;           /* 1 = the set did not fit: nothing is listed, nothing is remembered */
  uint32_t events_truncated;   /* 1 = begun or ended exceeds max_events */
} ScTickPairEventInfo;
int scTickSetPairEvents(ScTickContext* ctx, uint32_t max_tracked_pairs, uint32_t max_events);
/* begun2 / ended2: [cap][2] (a, b), either may be NULL with capacity 0; min(count, max_events, capacity) pairs are written to each.
 * Synchronises; copies the 24 bytes of `info` and the listed pairs, nothing else. */
int scTickReadPairEvents(ScTickContext* ctx, uint32_t* begun2, uint32_t begun_cap, uint32_t* ended2, uint32_t ended_cap, ScTickPairEventInfo* info);

/* ---- touching pairs: exact collider-shape overlap over the pair list ----
 * The pair search reports pairs of WORLD AABBs: a 4.4 m x 2 m vehicle box yawed by 45 degrees is a 4.5 m square to it, and two cars
 * passing in neighbouring lanes are a pair.  What Bullet's narrow phase answers in the reference (behind sc_physics.cpp:218-225) is whether
 * the shapes themselves touch.  A run with SC_TICK_PAIR_SHAPES also lists the pairs of this tick's pair list whose collider shapes
 * (scTickUploadColliders: BOX, SPHERE, CAPSULE) overlap, taken through the members' world matrices of this tick.  The list is boolean:
 * contact point, normal and depth are the "pair contacts" below, opt-in.  This build's OWN SPEC, like the exact shapes for rays, whose frame conventions it shares.  All
 * arithmetic is fp32, unfused, left to right, with correctly rounded / and sqrt; dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z;
 * clamp01(x) = (c < 1) ? c : 1 with c = (x > 0) ? x : 0 (a NaN is 0).
 *   scTickSetPairShapes(max_touching) enables the pass and sizes its list (0 switches it off and frees the buffers).
 *   The filter only ever REMOVES pairs: a pair (a, b) of the list is dropped only when one of the positive comparisons below proves the
 *   shapes apart.  A NaN makes such a comparison false, so the pair is kept: a NaN in a matrix column makes its member not refinable, a
 *   NaN translation reaches every comparison of the pair's routine (in F it makes g_k = 0: no distance, no separation), and collider
 *   records are finite (scTickUploadColliders refuses others).  Touching is a subset of the pairs.
 *   A member id is REFINABLE under the conditions under which the exact rays refine a candidate: colliders were uploaded, the id's rank is
 *   this context's, e = id & 0xFFFFFF is below the entity count, the collider type of e is BOX, SPHERE or CAPSULE, and every n_k below is
 *   finite and > 0.  A pair with a member that is not refinable is listed on its AABB answer -- it is in the pair list, so it is listed --
 *   and counted in kept_as_boxes: BOUNDS proxies, a neighbour tile's border records, degenerate matrices, a context without colliders.
 * Per refinable member, with R_r = row r of e's world matrix as this run's transform stage leaves it:
 *   c_k = (R_0[k], R_1[k], R_2[k]);  T = (R_0.w, R_1.w, R_2.w);  n_k = dot(c_k, c_k);  (ex, ey, ez, radius) = the collider's record
 *   (a box's half extents; (0, 0, 0, radius) for a sphere; (0, max(0, half_height), 0, radius) for a capsule).
 *   SPHERE   the point T (A = 0), R = radius * sqrt(m), m = (n_0 < m') ? m' : n_0 with m' = (n_2 < n_1) ? n_1 : n_2.
 *   CAPSULE  the segment T - A .. T + A, A = c_1 * ey per component, R = radius * sqrt((n_0 < n_2) ? n_2 : n_0).  Not dot(A, A) > 0:
 *            A = 0, the sphere of radius R.
 *   BOX      centre T, q_k = sqrt(n_k), unit axes u_k = c_k / q_k per component, half lengths H_k = e_k * q_k.  The columns are taken as
 *            orthogonal: for a sheared matrix this is the shape in the frame these formulas define, as for the rays.
 * Three routines cover the six type pairs (a is the member with the lower id).
 *   1. ROUND - ROUND (sphere / capsule in any combination): the squared distance of two segments by the clamped closed form.
 *        p1 = Ta - Aa; d1 = Aa + Aa; p2 = Tb - Ab; d2 = Ab + Ab; r = p1 - p2 (per component);
 *        a = dot(d1, d1); e = dot(d2, d2); f = dot(d2, r); s = 0; t = 0;
 *        not a > 0:  when e > 0, t = clamp01(f / e).
 *        otherwise   c = dot(d1, r);  not e > 0: s = clamp01((-c) / a).  Otherwise b = dot(d1, d2); den = a*e - b*b;
 *                    when den > 0, s = clamp01((b*f - c*e) / den);  t = (b*s + f) / e;
 *                    t < 0: t = 0, s = clamp01((-c) / a);  else t > 1: t = 1, s = clamp01((b - c) / a).
 *        v = (p1 + d1*s) - (p2 + d2*t) per component.  APART when dot(v, v) > (Ra + Rb) * (Ra + Rb).
 *   2. ROUND - BOX: the segment in the box's frame.  w = Tround - Tbox; per axis k: yc = dot(u_k, w); ya = dot(u_k, A); y0_k = yc - ya;
 *        dy_k = ya + ya.  F(t) = (g_0*g_0 + g_1*g_1) + g_2*g_2 with g_k = (x > 0) ? x : 0, x = |y0_k + dy_k*t| - H_k: the squared distance
 *        of the segment's point t from the box, convex and piecewise quadratic in t.  fmin = F(0).  When A is not (0, 0, 0):
 *        fmin = min(fmin, F(1));  b_0 = 0, b_7 = 1, b_(1+2k) = clamp01((H_k - y0_k) / dy_k), b_(2+2k) = clamp01(((-H_k) - y0_k) / dy_k);
 *        b_1..b_6 are put in ascending order by the compare-exchanges (1,6) (2,4) (3,5) (2,3) (4,5) (1,4) (3,6) (1,2) (3,4) (5,6) (2,3)
 *        (4,5), in this order, (i,j) leaving the smaller in b_i.  For i = 0..6: lo = b_i, hi = b_(i+1), tm = (lo + hi) * 0.5; per axis k
 *        with y = y0_k + dy_k*tm: when |y| - H_k > 0, num_k = (y0_k - ((y > 0) ? H_k : -H_k)) * dy_k and den_k = dy_k*dy_k, else both 0;
 *        ns = (num_0 + num_1) + num_2, ds likewise; ts = (ds > 0) ? (-ns) / ds : lo; ts = (ts < lo) ? lo : ts; ts = (ts > hi) ? hi : ts;
 *        fmin = min(fmin, F(ts)), and for i < 6 fmin = min(fmin, F(hi)).  min(m, x) = (x < m) ? x : m.
 *        APART when fmin > R * R.  (The minimum of F lies at a breakpoint, an end, or the stationary point of one interval: all are
 *        visited, so no search for the sign change of F' is needed.)
 *   3. BOX - BOX: the 15-axis separating-axis test in a's frame (Gottschalk; Ericson's TestOBBOBB).  w = Tb - Ta; t_i = dot(w, ua_i);
 *        R_ij = dot(ua_i, ub_j); Q_ij = |R_ij| + SC_TICK_PAIR_SHAPES_SAT_EPS.
 *        a's axis i:   APART when |t_i| > Ha_i + ((Hb_0*Q_i0 + Hb_1*Q_i1) + Hb_2*Q_i2).
 *        b's axis j:   APART when |(t_0*R_0j + t_1*R_1j) + t_2*R_2j| > ((Ha_0*Q_0j + Ha_1*Q_1j) + Ha_2*Q_2j) + Hb_j.
 *        ua_i x ub_j, with i1 = (i+1) % 3, i2 = (i+2) % 3, j1, j2 likewise:
 *                      APART when |t_i2*R_i1j - t_i1*R_i2j| > (Ha_i1*Q_i2j + Ha_i2*Q_i1j) + (Hb_j1*Q_ij2 + Hb_j2*Q_ij1).
 *        The epsilon keeps a cross axis of two (nearly) parallel edges -- a null vector up to rounding -- from separating anything.
 * Pairs look as in scTickReadPairs: a < b, id = rank << 24 | dense index.  The order inside the list is unspecified.  A pair that the
 * pair list names twice is tested, counted and listed once per naming.
 * The pass runs on the device behind the pair search, on its stream (after scTickRunPairs in a split flow; with SC_TICK_PAIR_EVENTS in
 * the same run, before the events, which still diff the AABB pair set): two launches, no host round trip, replayed from a captured
 * graph.  It reads the resident collider records and matrix rows and owns no per-entity state.  Device memory: max_touching x 8 bytes.
 * scTickSetPairShapes drops captured graphs, asks for no learn tick, and fails while scTickRunPairs is pending.  A context that never
 * calls it allocates and launches exactly what it did before.
 * scTickRun / scTickTileStep fail, with a last-error text and nothing changed, for SC_TICK_PAIR_SHAPES without SC_TICK_BROADPHASE, without
 * a prior scTickSetPairShapes, or on a pipelined context (scTickSetPipelined / scTickSetPairsStream: by the time its pair half runs the
 * matrices may be the next tick's -- the reason EXACT rays refuse it).  In the caller-owned split flow the pair half reads the matrix
 * rows, the collider records and the dense indices as they stand when scTickRunPairs runs, so between
 * scTickRun(.. | SC_TICK_SPLIT_PAIRS | SC_TICK_PAIR_SHAPES) and its scTickRunPairs the calls that rewrite one of them fail as they do for
 * EXACT rays: scTickUploadWorldMatrices, scTickUploadColliders, scTickRemoveEntities, scTickSetEntityCount, scTickRun with SC_TICK_XFORM.
 * scTickReadPairShapes fails when the last run did not carry the flag and while scTickRunPairs is pending. */
#define SC_TICK_PAIR_SHAPES_SAT_EPS 1e-6f
typedef struct ScTickPairShapeInfo
{
  uint32_t tested;          /* pairs of this tick's list that were looked at (the clamped total, as pair events count it) */
  uint32_t touching;        /* true total of pairs listed as touching: may exceed max_touching and the caller's capacity */
  uint32_t refined;         /* pairs decided by the shapes of both members */
  uint32_t kept_as_boxes;   /* pairs with a member that cannot be refined: listed on their AABB answer */
  uint32_t truncated;       /* 1 = touching > max_touching: the list holds max_touching valid members */
  uint32_t pairs_truncated; /* 1 = the pair list itself was truncated this tick (ScTickCounts::pairs_truncated): the touching list is of what was listed */
} ScTickPairShapeInfo;
int scTickSetPairShapes(ScTickContext* ctx, uint32_t max_touching);   /* 0 switches it off and frees the buffers */
/* pairs2: [capacity][2] (a, b), may be NULL with capacity 0.  Synchronises; copies the 24 bytes of `info` and
 * min(touching, max_touching, capacity) pairs, nothing else. */
int scTickReadPairShapes(ScTickContext* ctx, uint32_t* pairs2, uint32_t capacity, ScTickPairShapeInfo* info);

/* ---- pair contacts: point, normal and depth of every touching pair ----
 * The touching list is boolean.  A host that pushes a character out of a wall, places a decal or feeds a solver needs what Bullet's narrow
 * phase hands the reference with the pair (sc_physics.cpp:218-225): where the shapes meet, in which direction, how deep.  While pair
 * contacts are enabled, every run with SC_TICK_PAIR_SHAPES also writes one ScTickPairContact per entry of the touching list: record i
 * belongs to entry i of the list scTickReadPairShapes returns for the same tick.  There is no run flag of its own.  This build's OWN SPEC,
 * over the "touching pairs" text above: the same fp32 arithmetic (unfused, left to right, correctly rounded / and sqrt), the same dot and
 * clamp01, the same REFINABLE rule, the same SPHERE / CAPSULE (A, R) and BOX (u_k, H_k, T) construction, the same routines 1 - 3 with
 * their intermediate values.  sign(x) = (x < 0) ? -1 : +1 (so sign(0) = sign(NaN) = +1); clamp(x, h) = (c > h) ? h : c with
 * c = (x < -h) ? -h : x; a sum over three axes of a frame is (x_0*u_0 + x_1*u_1) + x_2*u_2 per component, and "the world image" of frame
 * coordinates x is T + that sum.
 *   normal  a unit vector from member a to member b of the listed pair (a < b as listed);
 *   depth   >= 0: how far b must move along normal for the two features to just touch;
 *   point   on the contact line (through the closest feature points, along normal): the middle of the stretch of that line that lies
 *           in both shapes -- the midpoint between the two surfaces unless one shape reaches right through the other;
 *   kind    which routine answered, SC_TICK_CONTACT_*, with the DEEP and DEGENERATE bits.
 * NOT REFINED: a pair with a member that is not refinable (kept_as_boxes) gets SC_TICK_CONTACT_NONE and all floats 0.
 * 1. ROUND - ROUND (kind ROUND_ROUND): p1, d1, p2, d2, s, t, v as in routine 1; d2v = dot(v, v); Pa = p1 + d1*s.
 *      d2v > 0:  dist = sqrt(d2v); depth = (Ra + Rb) - dist; normal = (-v) / dist per component.  On the line Pa + normal*x, a is
 *                [-Ra, Ra] and b is [dist - Rb, dist + Rb]:  far = dist + Rb; hi = (far < Ra) ? far : Ra;  near = dist - Rb;
 *                lo = (near < -Ra) ? -Ra : near;  mid = (lo + hi) * 0.5;  point = Pa + normal*mid per component.
 *      otherwise (coincident centre lines, or a NaN): DEGENERATE; normal = (0, 1, 0); depth = Ra + Rb; point = Pa.
 * 2. ROUND - BOX (kind ROUND_BOX): y0, dy, F and fmin as in routine 2, and `at`, the parameter at which fmin was found: 0 for F(0), and
 *      each later candidate (F(1), then per interval F(ts) and F(hi), in that order) replaces it only when strictly smaller.
 *      y_k = y0_k + dy_k*at; q_k = clamp(y_k, H_k); m_k = H_k - |y_k|; k' = the first k with the smallest m_k (strict <);
 *      sg = sign(y_k'); dist = sqrt(fmin); e_k = (y_k - q_k) / dist; ell_k = (H_k + H_k) / |e_k|; l = the least ell_k (ell_0, then each
 *      later one when strictly smaller).  On the line y + nBox*x the round is [-R, R].
 *      fmin > 0 (shallow): nb_k = e_k; depth = R - dist.  The box is [-(dist + l), -dist]:  far = dist + l;
 *                hi = (far < R) ? far : R;  mid = -((dist + hi) * 0.5).
 *      otherwise (DEEP: the centre-line point is inside the box): nb_k = (k == k') ? sg : 0;
 *                e0 = sg*y0_k'; e1 = sg*(y0_k' + dy_k'); low = (e1 < e0) ? e1 : e0; depth = R + (H_k' - low): the overlap of the whole
 *                round along that face's normal (a sphere: low = |y_k'|, so depth = R + m_k').  The box is [m_k' - 2H_k', m_k']:
 *                back = m_k' - (H_k' + H_k'); lo = (back < -R) ? -R : back; hi = (m_k' < R) ? m_k' : R; mid = (lo + hi) * 0.5.
 *      nBox = the sum of nb_k u_k; point = (the world image of y) + nBox*mid per component; normal = -nBox when the round is a, else
 *      nBox.
 * 3. BOX - BOX: R_ij, Q_ij, t_i as in routine 3, and the fifteen axes in its order.  Overlap o and signed projection tl per axis:
 *        a's axis i:    o = (Ha_i + ((Hb_0*Q_i0 + Hb_1*Q_i1) + Hb_2*Q_i2)) - |t_i|;  tl = t_i;  L = ua_i.
 *        b's axis j:    tl = (t_0*R_0j + t_1*R_1j) + t_2*R_2j;  o = (((Ha_0*Q_0j + Ha_1*Q_1j) + Ha_2*Q_2j) + Hb_j) - |tl|;  L = ub_j.
 *        ua_i x ub_j:   l2 = 1 - R_ij*R_ij; skipped when l2 < SC_TICK_PAIR_CONTACTS_EDGE_EPS (parallel edges add nothing to the face axes);
 *                       tl = t_i2*R_i1j - t_i1*R_i2j;  o = (((Ha_i1*Q_i2j + Ha_i2*Q_i1j) + (Hb_j1*Q_ij2 + Hb_j2*Q_ij1)) - |tl|) / sqrt(l2);
 *                       L = R_i1j*ua_i2 - R_i2j*ua_i1 per component.
 *      The first axis starts as the best; a later one replaces it only when its o is strictly smaller: ties stay with the earlier axis,
 *      faces come before edges.  depth = (o < 0) ? 0 : o (a pair inside the separating-axis epsilon); sg = sign(tl);
 *      normal = sg * L for a face axis, sg * (L / sqrt(dot(L, L))) for an edge axis.  h = depth * 0.5.
 *      BOX_FACE_A (a's axis i):  g_j = sign(dot(normal, ub_j)) * Hb_j;  p = Tb - the sum of g_j ub_j  (b's vertex furthest against the
 *                       normal);  r = p - Ta;  x_k = dot(r, ua_k), and for the two k other than i x_k = clamp(x_k, Ha_k);
 *                       point = (the world image of x in a's frame) + normal*h.
 *      BOX_FACE_B (b's axis j):  g_k = -sign(dot(normal, ua_k)) * Ha_k;  p = Ta - the sum of g_k ua_k  (a's vertex furthest along the
 *                       normal);  r = p - Tb;  x_k = dot(r, ub_k), clamped for the two k other than j;
 *                       point = (the world image of x in b's frame) - normal*h.
 *      BOX_EDGE (i, j): ga_k = (k == i) ? 0 : sign(dot(normal, ua_k)) * Ha_k;  gb_k = (k == j) ? 0 : (-sign(dot(normal, ub_k))) * Hb_k;
 *                       ea, eb = the world images of ga in a's frame and gb in b's;  va = ua_i * Ha_i;  vb = ub_j * Hb_j;
 *                       p1 = ea - va; d1 = va + va; p2 = eb - vb; d2 = vb + vb;  s, t by routine 1's closed form;
 *                       point = ((p1 + d1*s) + (p2 + d2*t)) * 0.5.
 * LIMITS: one point per pair (more of them: the "pair manifolds" below).  A DEEP capsule reports the face nearest to the centre-line point routine 2 stopped at, with
 * the capsule's overlap along that face's normal, which need not be the capsule's minimum translation; point stays on the line through
 * that centre-line point.  A sheared matrix gives the shape in the frame these formulas define.  A neighbour
 * tile's shapes are unknown (NONE).  A pipelined context already refuses the flag.
 *   scTickSetPairContacts(enable) needs a prior scTickSetPairShapes(max_touching > 0) -- otherwise it fails with a last-error text and
 *   nothing changes -- and allocates max_touching records of 32 bytes, 8 control words and 8 report words; 0 frees them.  Like
 *   scTickSetPairShapes it drops captured graphs, asks for no learn tick and fails while scTickRunPairs is pending.
 *   scTickSetPairShapes(0) switches contacts off too; scTickSetPairShapes(another size) re-sizes their buffer.
 * The pass is two more launches behind the narrow-phase pass, on its stream -- a thread per entry of the list, then one thread for the
 * report --, the entry count read on the device, so they replay from a captured graph.  A context that never enables it launches exactly what it did before.
 * scTickReadPairContacts synchronises like scTickReadPairShapes and copies the 32 bytes of `info` and min(touching, max_touching,
 * capacity) records, nothing else.  It fails when the last run did not carry SC_TICK_PAIR_SHAPES, when contacts were not enabled at that
 * run, and while scTickRunPairs is pending. */
#define SC_TICK_PAIR_CONTACTS_EDGE_EPS 1e-4f
#define SC_TICK_CONTACT_NONE        0u      /* the pair was kept on its AABB answer: all floats are 0 */
#define SC_TICK_CONTACT_ROUND_ROUND 1u
#define SC_TICK_CONTACT_ROUND_BOX   2u
#define SC_TICK_CONTACT_BOX_FACE_A  3u
#define SC_TICK_CONTACT_BOX_FACE_B  4u
#define SC_TICK_CONTACT_BOX_EDGE    5u
#define SC_TICK_CONTACT_DEEP        (1u << 8)   /* ROUND_BOX: the round's centre line is inside the box */
#define SC_TICK_CONTACT_DEGENERATE  (1u << 9)   /* no direction could be formed: the fallback normal (0, 1, 0) */
typedef struct ScTickPairContact
{
  float point[3];
  float depth;
  float normal[3];
  uint32_t kind;            /* SC_TICK_CONTACT_* in the low byte, DEEP / DEGENERATE above it */
} ScTickPairContact;
typedef struct ScTickPairContactInfo          /* counts over the records written, not over the true touching total */
{
  uint32_t written;         /* min(touching, max_touching) */
  uint32_t round_round;
  uint32_t round_box;
  uint32_t box_box;         /* BOX_FACE_A, BOX_FACE_B and BOX_EDGE */
  uint32_t unrefined;       /* SC_TICK_CONTACT_NONE */
  uint32_t deep;
  uint32_t degenerate;
  uint32_t reserved;        /* 0 */
} ScTickPairContactInfo;
int scTickSetPairContacts(ScTickContext* ctx, uint32_t enable);
int scTickGetPairContacts(ScTickContext* ctx, uint32_t* enabled);
/* out: [capacity] records, may be NULL with capacity 0 */
int scTickReadPairContacts(ScTickContext* ctx, ScTickPairContact* out, uint32_t capacity, ScTickPairContactInfo* info);

/* ---- pair manifolds: up to four contact points per touching pair ----
 * One point cannot describe a resting contact: a box on a slab touches over an area, a capsule lying on a floor along a line.  While pair
 * manifolds are enabled, every run with SC_TICK_PAIR_SHAPES also writes one ScTickPairManifold per entry of the touching list: record i
 * belongs to entry i of the list and to contact record i of the same tick, whose normal it shares (it is not repeated here).  No run flag
 * of its own.  This build's OWN SPEC, over the "pair contacts" text above: the same fp32 arithmetic, dot, sign, clamp, clamp01, frame sums
 * and world image, and the intermediate values routines 1 - 3 and the contact rules name.  Ties go to the earlier index.  Every point is
 * halfway between the two surfaces along the face's or the pair's own direction; depth[i] >= 0 belongs to point[i].
 * NONE: the contact is SC_TICK_CONTACT_NONE: count 0, all words 0.
 * SINGLE: count 1, point[0] and depth[0] are the contact's, bit for bit.  Every contact that no rule below replaces: one with a sphere
 *      (A = 0) in it, BOX_EDGE, any DEGENERATE contact, a shallow ROUND_BOX whose closest box feature is an edge or a vertex (more than
 *      one k with y_k != q_k, that is, a non-zero e_k), and a SEGMENT or FACE rule that keeps no point.
 * SEGMENT, a capsule on a box face: a ROUND_BOX contact whose round has A != 0 and that is DEEP (k' and sg as the contact rule has them)
 *      or shallow with exactly one k with y_k != q_k (that k is k'; sg = sign(y_k')).
 *      lo = 0, hi = 1; for the two k other than k', ascending:  dy_k != 0:  b0 = (H_k - y0_k) / dy_k; b1 = ((-H_k) - y0_k) / dy_k (routine
 *      2's breakpoints before clamp01); tl = (b1 < b0) ? b1 : b0; th = (b1 < b0) ? b0 : b1; lo = (tl > lo) ? tl : lo; hi = (th < hi) ? th : hi.
 *      dy_k == 0: the clip is empty when |y0_k| > H_k.  Empty, or not lo <= hi (rounding alone can do it): SINGLE.
 *      The ends t_0 = lo, t_1 = hi; t_1 is left out when hi == lo.  Per end: yk = y0_k' + dy_k'*t; up = sg*yk; pen = R - (up - H_k'); kept
 *      when pen >= 0, l <= h (below: the round reaches the box at that end) and the line through the end along the face's normal leaves
 *      the round at R: dd = (dy_0*dy_0 + dy_1*dy_1) + dy_2*dy_2 and R*(dy_k'*dy_k') <= SC_TICK_MANIFOLD_FLAT*dd (the centre line lies flat
 *      on the face), or the end is a true end of the centre line that the normal leaves on the far side (t_0 == 0 and sg*dy_k' >= 0;
 *      t_1 == 1 and sg*dy_k' <= 0).  On the line through the centre-line point along the face's normal the round is [-R, R] and the box
 *      [least - 2H_k', least]: least = H_k' - up; back = least - (H_k' + H_k'); l = (back < -R) ? -R : back; h = (least < R) ? least : R;
 *      mid = (l + h) * 0.5;  x_k' = yk + sg*mid and x_k = y0_k + dy_k*t for the other two;  point = the world image of x in the box's
 *      frame;  depth = pen.  The kept ends fill the slots in their order.
 * SEGMENT, capsule on capsule: a ROUND_ROUND contact, not DEGENERATE, both rounds with A != 0.  p1, d1, p2, d2 as in routine 1;
 *      a = dot(d1, d1); e = dot(d2, d2).  Two candidates, c = 0, 1:  g = p2 (c = 0) or p2 + d2 (c = 1);  s_c = clamp01(dot(g - p1, d1) / a);
 *      Pa = p1 + d1*s_c;  the partner Pb is g itself when clamp01 left the quotient as it was (the end projects into segment 1), else
 *      p2 + d2*t with t = clamp01(dot(Pa - p2, d2) / e): every candidate pairs an end of one segment with its closest point on the
 *      other.  v = Pa - Pb;  d2v = dot(v, v);  dist = sqrt(d2v);
 *      pen = (Ra + Rb) - dist;  w = (-v) / dist per component;  kept when pen >= 0, d2v > 0, the candidate's own direction is the contact's
 *      -- (Ra + Rb) * dot(w - normal, w - normal) <= SC_TICK_MANIFOLD_FLAT -- and the line through the pair leaves either round at its
 *      radius: c1 = dot(w, d1): s_c == 0 and c1 <= 0, or s_c == 1 and c1 >= 0, or Ra*(c1*c1) <= SC_TICK_MANIFOLD_FLAT*a;  c2 = dot(w, d2),
 *      tp = the partner's parameter (0 or 1 for g itself, else t): tp == 0 and c2 >= 0, or tp == 1 and c2 <= 0, or
 *      Rb*(c2*c2) <= SC_TICK_MANIFOLD_FLAT*e.  Candidate 1 is left out when s_1 == s_0.  far, near, hi, lo, mid as in
 *      contact rule 1 with this dist;  point = Pa + w*mid per component;  depth = pen.  None kept: SINGLE.
 *      Neither SEGMENT rule has a parallelism threshold: a crossing pair keeps no end, a lying pair keeps both.
 * FACE: BOX_FACE_A or BOX_FACE_B.  The reference box o is the axis's owner (a, axis i; or b, axis j), the other box is t.  ax = that
 *      axis, a1 = (ax + 1) % 3, a2 = (ax + 2) % 3;  sg = sign(tl) of the contact rule;  sr = sg for FACE_A, -sg for FACE_B: the reference
 *      face lies at sr * Ho_ax along uo_ax.  The incident face: c_k = dot(normal, ut_k); m = the first k with the largest |c_k| (strict >);
 *      sm = +1 when (c_m < 0) differs from "FACE_B", else -1; m1 = (m + 1) % 3, m2 = (m + 2) % 3.  Its vertices j = 0..3 have the signs
 *      (s1, s2) = (+, +), (-, +), (-, -), (+, -):  g_m = sm*Ht_m, g_m1 = s1*Ht_m1, g_m2 = s2*Ht_m2;  V = the world image of g in t's frame;
 *      r = V - To;  x_k = dot(r, uo_k);  the vertex is (p, q, z) = (x_a1, x_a2, sr*x_ax).
 *      Clip (Sutherland-Hodgman) against p <= Ho_a1, p >= -Ho_a1, q <= Ho_a2, q >= -Ho_a2, in that order; per plane with bound h on
 *      coordinate x: walk the vertices in order, each with its predecessor (the first with the last): when exactly one of the two is
 *      inside, emit prev + (cur - prev) * ((h - x_prev) / (x_cur - x_prev)) per component (all three); then emit cur when it is inside.
 *      A vertex beyond the eighth is not emitted.
 *      The point of a vertex is the world image in o's frame of x_a1 = p, x_a2 = q, x_ax = sr * (z + pen*0.5) with pen = Ho_ax - z, its
 *      depth pen.  A vertex is kept when pen >= 0, z >= -Ho_ax (it is not below the reference box) and the point lies within
 *      SC_TICK_MANIFOLD_SKIN of the other box: r = point - Tt and |dot(r, ut_k)| - Ht_k <= SC_TICK_MANIFOLD_SKIN for k = 0, 1, 2.  Nothing kept: SINGLE.  Up to four: the slots in polygon order.  More: REDUCED, and the
 *      slots are: the deepest (largest pen); the one farthest from it by dp*dp + dq*dq; with (ex, ey) the in-face vector from the first to
 *      the second, area = ex*(q - q_first) - ey*(p - p_first): the largest area above 0, left out when none is; the smallest area below
 *      0, left out when none is.  Each of the four searches takes the first vertex and then each later one that is strictly better.
 * WHAT THE EXTRA CONDITIONS BUY: every point lies in both shapes, to within a millimetre, and its depth is the two shapes' overlap on the
 * line through it along the contact's normal -- on a box resting a few centimetres deep as on shapes a metre inside each other at random
 * angles, where an inclined capsule's end or the vertex of a steeply leaning face would otherwise report a feature's depth under a point
 * outside one shape.  What they drop falls back towards SINGLE.
 * LIMITS: BOX_EDGE and edge or vertex features give one point.  A DEEP capsule uses the face its contact reports.  A sheared matrix gives
 * the shape in the frame these formulas define.  A neighbour tile's shapes give NONE.  A pipelined context already refuses the flag.
 * Bullet's btBoxBoxDetector culls to the deepest point plus an angular spread around the centroid; this rule goes by extent instead.
 *   scTickSetPairManifolds(enable) needs pair contacts enabled -- otherwise it fails with a last-error text and nothing changes -- and
 *   allocates max_touching records of 80 bytes, 8 control words and 8 report words; 0 frees them.  It drops captured graphs, asks for no
 *   learn tick and fails while scTickRunPairs is pending.  scTickSetPairContacts(0) and scTickSetPairShapes(0) switch manifolds off too;
 *   scTickSetPairShapes(another size) re-sizes their buffer.
 * The pass is two more launches behind the contacts' -- a thread per entry of the list, then one thread for the report --, the entry
 * count read on the device, so they replay from a captured graph.  A context that never enables it launches exactly what it did before.
 * scTickReadPairManifolds synchronises like scTickReadPairContacts and copies the 32 bytes of `info` and min(touching, max_touching,
 * capacity) records, nothing else.  It fails when the last run did not carry SC_TICK_PAIR_SHAPES, when manifolds were not enabled at that
 * run, when they were switched off since, and while scTickRunPairs is pending. */
#define SC_TICK_MANIFOLD_SKIN     2.5e-4f   /* metres: how far outside the other box a FACE point may lie (a leaning edge) */
#define SC_TICK_MANIFOLD_FLAT     1e-3f     /* metres: R * cos^2 of the angle a round's centre line may make with the line its depth is measured on */
#define SC_TICK_MANIFOLD_NONE     0u   /* the pair's contact is SC_TICK_CONTACT_NONE: count 0, all words 0 */
#define SC_TICK_MANIFOLD_SINGLE   1u   /* the contact's own point and depth, count 1 */
#define SC_TICK_MANIFOLD_SEGMENT  2u   /* ends of a capsule's contact stretch, count 1..2 */
#define SC_TICK_MANIFOLD_FACE     3u   /* incident face clipped to the reference face, count 1..4 */
#define SC_TICK_MANIFOLD_REDUCED  (1u << 8)  /* FACE: more than four vertices were kept, four were chosen */
typedef struct ScTickPairManifold       /* 80 bytes: five 16-byte stores */
{
  float    point[4][3];
  float    depth[4];
  uint32_t count;                       /* 0..4; slots >= count are +0 */
  uint32_t kind;                        /* SC_TICK_MANIFOLD_* in the low byte, REDUCED above it */
  uint32_t reserved[2];                 /* 0 */
} ScTickPairManifold;
typedef struct ScTickPairManifoldInfo   /* 32 bytes, over the records written */
{
  uint32_t written;         /* min(touching, max_touching) */
  uint32_t points;          /* the sum of count */
  uint32_t with_one;
  uint32_t with_two;
  uint32_t with_three;
  uint32_t with_four;
  uint32_t face;            /* SC_TICK_MANIFOLD_FACE, REDUCED or not */
  uint32_t reduced;
} ScTickPairManifoldInfo;
int scTickSetPairManifolds(ScTickContext* ctx, uint32_t enable);
int scTickGetPairManifolds(ScTickContext* ctx, uint32_t* enabled);
/* out: [capacity] records, may be NULL with capacity 0 */
int scTickReadPairManifolds(ScTickContext* ctx, ScTickPairManifold* out, uint32_t capacity, ScTickPairManifoldInfo* info);

/* ---- pair islands: the connected components of the touching pairs ----
 * What a rigid-body host does next with a tick's touching list is group it: Bullet builds simulation islands, the connected components of
 * the contact graph in which a static body belongs to no island and joins none (btSimulationIslandManager; PhysicsWorld::isBodyActive,
 * sc_physics.cpp:593, reports its island state).  Islands are what a solver parallelises over and what sleeping goes by.  While pair
 * islands are enabled, every run with SC_TICK_PAIR_SHAPES also labels every entity and every entry of the touching list with its island.
 * No run flag of its own.  This build's OWN SPEC, definition by definition:
 *   IDS        as scTickReadPairs gives them: rank << 24 | dense index.
 *   MOVABLE    An entity e of this context is movable when e < count and (group(e) & fixed_groups) == 0, group being the low 16 bits of
 *              its layer word (scTickUploadLayers).  Every other member id is FIXED: a set group bit, a neighbour tile's rank, an index
 *              at or above the count.  fixed_groups is the caller's: the reference puts static bodies on layer 2 (sc_physics.cpp:372-379);
 *              0 makes every own entity movable.
 *   EDGES      the entries of this tick's touching list as the narrow-phase pass wrote them: the first min(touching, max_touching)
 *              entries, pairs kept on their AABB answer and pairs named twice included.  An entry is LINKING when both members are
 *              movable; otherwise it is ANCHORED and joins nothing.
 *   ISLANDS    An island is a connected component of the movable entities under the linking edges; a movable entity with no linking
 *              edge is an island of one.  label(e) = the id of the member with the smallest dense index in e's island;
 *              label(a fixed e below the count) = SC_TICK_ISLAND_NONE.  The labels are a function of the inputs alone: they depend
 *              neither on scheduling nor on the order inside the list.
 *   EDGE ISLANDS   edge_island(i), for entry i of the touching list: the label of its first member if that member is movable, else the
 *              label of its second member if that one is, else SC_TICK_ISLAND_NONE.  It sits beside contact record i and manifold
 *              record i of the same tick, so a host groups contacts by island without a lookup.
 *   NO MEMORY  Every flagged run recomputes from its own list.  scTickRemoveEntities, a changed count, a layer upload and a tile change
 *              need no resync rule.
 *   TRUNCATED LISTS   With a truncated touching list or pair list the islands are those of what was listed and may be split;
 *              ScTickPairIslandInfo::list_truncated says so.
 * LIMITS: a neighbour tile's bodies are fixed, so an island never crosses a tile border.  A pipelined context already refuses the flag.
 * The islands keep no sleeping state: they only group (the rest state is pair sleep's, below, opt-in).
 *   scTickSetPairIslands(enable, fixed_groups) needs scTickSetPairShapes(max_touching > 0) first and refuses fixed_groups bits above 15
 *   -- either fails with a last-error text and nothing changes.  DEVICE MEMORY: 8 bytes per entity of the context's capacity (the
 *   union-find's word and the label), 4 bytes per entry of max_touching, 32 KB of per-workgroup tallies, 8 control words and 8 report
 *   words; 0 frees them.  It drops
 *   captured graphs, asks for no learn tick and fails while scTickRunPairs is pending.  scTickSetPairShapes(0) switches islands off too;
 *   scTickSetPairShapes(another size) re-sizes their buffer and keeps fixed_groups.  A second call with another fixed_groups reaches the
 *   next run, in graph mode too.
 * The pass is four more launches between the narrow-phase pass and the list's report, on the pair half's stream, with no host round
 * trip -- a thread per entity (its own root, or none), a thread per entry (a lock-free union-find: the larger root is hooked under the
 * smaller with a compare-and-swap), a thread per entity and entry (labels, edge islands, the counts), one workgroup for the report --, the
 * counts read on the device, so they replay from a captured graph.  In the split flow they run behind scTickRunPairs; between the halves
 * of such a tick scTickUploadLayers is refused while islands are enabled.  A context that never enables it allocates and launches
 * exactly what it did before.
 * scTickReadPairIslands synchronises like scTickReadPairContacts and copies the 32 bytes of `info`, min(count, label_capacity) labels and
 * min(edges, edge_capacity) edge islands, nothing else.  It fails when the last run did not carry SC_TICK_PAIR_SHAPES, when islands were
 * not enabled at that run, when they were switched off since, and while scTickRunPairs is pending. */
#define SC_TICK_ISLAND_NONE 0xFFFFFFFFu    /* the label of a fixed entity, the island of an entry with no movable member */
typedef struct ScTickPairIslandInfo     /* 32 bytes */
{
  uint32_t edges;           /* entries of the touching list looked at: min(touching, max_touching) */
  uint32_t linking;         /* entries with two movable members */
  uint32_t anchored;        /* the others; edges == linking + anchored */
  uint32_t islands;         /* islands of two or more members */
  uint32_t bodies;          /* members of those islands */
  uint32_t movable;         /* movable entities below the count */
  uint32_t list_truncated;  /* ScTickPairShapeInfo::truncated | pairs_truncated of the same run */
  uint32_t gave_up;         /* 0; non-zero: a lane left a loop at its bound, the labels are not to be trusted */
} ScTickPairIslandInfo;
int scTickSetPairIslands(ScTickContext* ctx, uint32_t enable, uint32_t fixed_groups);
int scTickGetPairIslands(ScTickContext* ctx, uint32_t* enabled, uint32_t* fixed_groups);
/* labels: [label_capacity], edge_islands: [edge_capacity]; either may be NULL with capacity 0 */
int scTickReadPairIslands(ScTickContext* ctx, uint32_t* labels, uint32_t label_capacity, uint32_t* edge_islands, uint32_t edge_capacity,
                          ScTickPairIslandInfo* info);

/* ---- pair persistence: this run's contact points matched to the last run's ----
 * Every flagged run writes its manifolds from nothing; a rigid-body host needs to know which of this tick's contact points is the same
 * point as last tick's -- for warm starting, accumulated impulses and contact age (Bullet's btPersistentManifold behind
 * sc_physics.cpp:218-225).  While pair persistence is enabled, every run with SC_TICK_PAIR_SHAPES also matches each entry of its touching
 * list to the entry of the same pair in the last such run, each manifold point of the entry to a point of that earlier manifold, carries
 * a per-point age and a 16-byte caller payload across the match, and remembers this run for the next one.  No run flag of its own.  This
 * build's OWN SPEC, operation by operation; all arithmetic fp32, unfused, left to right; dot as the touching pairs define it.
 *   LOCAL POINT   Entry i with listed pair (a, b) and manifold record i of this run.  For each slot s < count: c_k and n_k are the columns
 *              of a's world matrix this tick and their squared norms as the touching pairs form them; u_k = c_k / sqrt(n_k) per component
 *              (the box frame's u, whatever a's collider type); r = point[s] - T_a; x_s,k = dot(r, u_k).  A record with count == 0
 *              (SC_TICK_MANIFOLD_NONE) has no local points.  The record's stored fp32 point is the input.
 *   REMEMBERED RUN   the last run with SC_TICK_PAIR_SHAPES while persistence was enabled, unless a resync (below) came since.  Its
 *              entries are the first min(touching, max_touching) of its list; the remembered entry of a pair is the smallest entry index
 *              of that run that names the pair.
 *   PAIR MATCH   prev_entry is that index, or SC_TICK_PERSIST_NONE when the pair is not remembered or nothing is.  A pair that this
 *              run's list names twice matches the same remembered entry from both entries.
 *   POINT MATCH   greedy, in slot order, one to one.  m2 = match_dist * match_dist, one fp32 product formed once per run.  For
 *              s = 0 .. count-1, over the remembered entry's slots t = 0 .. count_old-1 that no earlier s took, y_t its local points:
 *              e_k = x_s,k - y_t,k; d = (e_0*e_0 + e_1*e_1) + e_2*e_2; t is a candidate when d <= m2.  The first candidate is the best; a
 *              later one replaces it only when its d is strictly smaller.  With a best t: prev_slot[s] = t, age[s] = min(age_old[t] + 1,
 *              255), payload[s] = payload_old[t] bit for bit, and t is taken.  Otherwise prev_slot[s] = 0xFF, age[s] = 0 and payload[s] is
 *              four +0.  A NaN d matches nothing.  Slots at or above count are 0xFF, 0 and +0.
 *   RESYNC     on the first flagged run after enabling, after scTickRemoveEntities, after a shrinking scTickSetEntityCount, after
 *              scTickSetTile to another rank, and after scTickSetPairShapes with another size: nothing is remembered, every prev_entry is
 *              NONE and info.resync = 1.  A rename between the halves of a split tick is forgotten again behind the pair half, as for
 *              pair events.  Runs without SC_TICK_PAIR_SHAPES leave the memory alone.  A same-value second call of the setter keeps the
 *              memory; a call with another match_dist keeps it too and reaches the next run, in graph mode as well.
 *   TRUNCATED LISTS   Entries beyond max_touching are neither answered nor remembered.  info.list_truncated is
 *              ScTickPairShapeInfo::truncated | pairs_truncated of the run.  The tables are sized by max_touching: they cannot overflow.
 * LIMITS: matching is in a's frame only, with no drift test of a remembered point against b and no feature ids; a neighbour tile's shapes
 * give NONE and so no points; a pipelined context already refuses the flag.
 *   scTickSetPairPersistence(enable, match_dist) needs pair manifolds enabled, and match_dist finite and > 0 -- otherwise it fails with a
 *   last-error text and nothing changes.  DEVICE MEMORY, per entry of max_touching: the 16-byte record, and on each of two sides 48
 *   bytes of local points, 16 bytes of ages and count and 64 bytes of payload rows (272 bytes); per side a table of slots = the power
 *   of two >= max(2 * max_touching, 64), 12 bytes a slot; 16 KB of per-workgroup tallies, 16 control words and 16 report words; 0 frees
 *   them.  It drops captured graphs, asks for no learn tick and fails while scTickRunPairs is pending.  scTickSetPairManifolds(0),
 *   scTickSetPairContacts(0) and scTickSetPairShapes(0) switch persistence off too.
 * The pass is three more launches behind the manifolds', ahead of the list's report, on the pair half's stream, with no host round trip
 * -- a thread per entry (enter, look up, match, write), a thread per slot (the remembered side's table cleared: the next run's empty
 * "current"), one workgroup for the report, which turns the sides over --, the counts, the side and the validity read on the device, so
 * both parities of the tick replay from captured graphs.  A context that never enables it allocates and launches exactly what it did before.
 *   scTickWritePairPayloads overwrites rows [first, first + count) of the last flagged run's payload rows -- the rows the next flagged
 *   run carries from --, ordered behind that run on its stream.  It fails when the last run did not carry SC_TICK_PAIR_SHAPES with
 *   persistence on, when first + count exceeds that run's `written`, and while scTickRunPairs is pending.  scTickReadPairPayloads
 *   returns min(written, capacity) of those rows as they stand: what the run carried, then what was written.
 * The reads synchronise and fail like scTickReadPairManifolds. */
#define SC_TICK_PERSIST_NONE 0xFFFFFFFFu   /* prev_entry of a pair that is not remembered */
typedef struct ScTickPairPersist        /* 16 bytes, record i beside manifold record i */
{
  uint32_t prev_entry;                  /* entry of the remembered run's list, or SC_TICK_PERSIST_NONE */
  uint8_t  prev_slot[4];                /* slot of that entry's manifold, or 0xFF */
  uint8_t  age[4];                      /* flagged runs this point has been matched for, saturating at 255 */
  uint32_t reserved;                    /* 0 */
} ScTickPairPersist;
typedef struct ScTickPairPersistInfo    /* 32 bytes */
{
  uint32_t written;         /* min(touching, max_touching) */
  uint32_t kept_pairs;      /* entries with a prev_entry */
  uint32_t new_pairs;       /* the others; written == kept_pairs + new_pairs */
  uint32_t kept_points;     /* slots below count with a prev_slot */
  uint32_t new_points;      /* slots below count without */
  uint32_t resync;          /* 1: nothing was remembered */
  uint32_t list_truncated;  /* ScTickPairShapeInfo::truncated | pairs_truncated of the same run */
  uint32_t gave_up;         /* 0; non-zero: a probe loop reached its bound (it cannot at load one half), the records are not to be trusted */
} ScTickPairPersistInfo;
int scTickSetPairPersistence(ScTickContext* ctx, uint32_t enable, float match_dist);
int scTickGetPairPersistence(ScTickContext* ctx, uint32_t* enabled, float* match_dist);
/* out: [capacity] records, may be NULL with capacity 0 */
int scTickReadPairPersistence(ScTickContext* ctx, ScTickPairPersist* out, uint32_t capacity, ScTickPairPersistInfo* info);
/* rows: [count][4][4] floats -- four payload rows of four words per entry */
int scTickWritePairPayloads(ScTickContext* ctx, const float* rows, uint32_t first, uint32_t count);
/* rows: [capacity][4][4] floats, may be NULL with capacity 0 */
int scTickReadPairPayloads(ScTickContext* ctx, float* rows, uint32_t capacity);

/* ---- pair sleep: islands at rest fall asleep and wake ----
 * The islands are what sleeping goes by; the one step of Bullet's island pipeline a rigid-body host still ran on the CPU every tick is which
 * islands are at rest, which bodies just fell asleep and which were just woken (PhysicsWorld::isBodyActive / activateBody,
 * sc_physics.h:167-168; the traffic AI asks every frame, sc_traffic_ai.cpp:382-383).  The library has no velocities; it has what Bullet's
 * thresholds stand in for: every tick's world matrices, resident, next to the island labels.  While pair sleep is enabled, every run with
 * SC_TICK_PAIR_SHAPES (pair islands being on) also does the following, on the world rows w_0, w_1, w_2 of the run (three float4 per
 * entity, .w the translation) as its narrow phase reads them.  No run flag of its own.  This build's OWN SPEC:
 *   STILL      Every own entity below the count keeps an ANCHOR POSE of three rows a_0..a_2 (48 bytes).  still(e) holds when
 *              |w_r.w - a_r.w| <= lin_tol for the three rows and |w_r.{x,y,z} - a_r.{x,y,z}| <= ang_tol for the nine other elements: plain
 *              fp32 -- subtract, absolute value, compare.  A NaN anywhere (a row or the anchor) makes the entity not still.  When not
 *              still, the anchor becomes the current pose: a creep of 0.4 * tol per run trips on the third run and starts over.
 *   REST       rest(e) = still ? min(rest_old + 1, 255) : 0 -- 8 bits, saturating like persistence's age; rest_runs is in 1 .. 255.
 *              Tracked for movable and fixed entities alike (movable and fixed as the pair islands define them).
 *   AWAKE ISLANDS   An island of this run (by this run's labels) is awake when a member has rest < rest_runs, or when an anchored entry
 *              of the listed touching list -- one member movable, the other not -- names one of its members together with an own
 *              fixed entity below the count that has rest == 0 in this run (a kinematic platform under a stack).
 *   ASLEEP     asleep(e) = e is movable and its island is not awake.  An island of one sleeps by itself.
 *   STATE      per entity: rest | SC_TICK_SLEEP_ASLEEP | SC_TICK_SLEEP_STILL | SC_TICK_SLEEP_MOVABLE (bits 8, 9, 10).
 *   EVENTS     fell_asleep: the ids (rank << 24 | index) asleep now and not at the last flagged run; woke: the reverse.  The order
 *              inside a list is unspecified.  Each list holds at most max_events ids; the true counts are in info, with an overflow bit
 *              per list in info.flags; which ids a short list holds is unspecified.
 *   WAKE       scTickWakeEntities sets rest = 0 and marks the anchor unset (NaN rows) for the named own entities: the next flagged run
 *              sees them not still, and `woke` reports their islands.  An id of another rank or at or above the count fails the call and
 *              nothing changes.  It is a write to device state outside any captured graph: a captured graph replays across it.
 *   RESYNC     on the first flagged run after enabling, after scTickRemoveEntities, after a shrinking scTickSetEntityCount, after
 *              scTickSetTile to another rank, after scTickSetPairShapes with another size and after a set call with another max_events:
 *              nothing is remembered, every anchor becomes the current pose, every rest is 0, there are no events and info.flags has
 *              SC_TICK_SLEEP_INFO_RESYNC.  A rename between the halves of a split tick is forgotten again behind the pair half, as for pair
 *              events.  A same-parameter set call keeps the memory; a changed tolerance or rest_runs keeps it too, reaches the next run
 *              and drops captured graphs (a capture holds them as kernel arguments).  Runs without SC_TICK_PAIR_SHAPES leave the memory
 *              alone.  An entity that a growing count newly covers starts from the zeroed state: rest 0, an anchor of all zeros.
 * LIMITS: no velocities and no forces -- a host that pushes a sleeping body calls scTickWakeEntities; the tolerances are absolute on
 * matrix elements (a scaled body's rotation elements scale with it); a member of another rank, or one at or above the count, counts as
 * still -- it is the other tile's to report, and an island never crosses a tile border; the awake entries are counted, not compacted into
 * a work list; the epoch is a 32-bit word (2^32 flagged runs); a pipelined context already refuses the flag.
 *   scTickSetPairSleep(enable, lin_tol, ang_tol, rest_runs, max_events) needs pair islands enabled, the tolerances finite and >= 0,
 *   rest_runs in 1 .. 255 and max_events > 0 -- otherwise it fails with a last-error text and nothing changes.  DEVICE MEMORY: per entity
 *   of the context's capacity 48 bytes of anchor, 4 of state and 4 of an `awake` word (indexed by island root), 4 * max_events bytes per
 *   event list, 32 KB of per-workgroup tallies, 16 control words and 8 report words; 0 frees them.  It asks for no learn tick and fails
 *   while scTickRunPairs is pending, as does scTickWakeEntities.  scTickSetPairIslands(0) and scTickSetPairShapes(0) switch sleep off too.
 * The pass is four more launches behind the islands', ahead of the list's report, on the pair half's stream, with no host round trip: a
 * thread per entity (rows against anchor; a movable entity with rest < rest_runs stores the run's epoch into the awake word of its
 * island), a thread per entry (the anchored-entry rule), a thread per entity and entry (asleep, state word, events by ballot with one
 * slot reservation per list and wave that has events), one workgroup for the report, which moves the epoch on.  Every writer of an awake
 * word writes the same value: no read-modify-write, no clearing pass.  Counts, epoch and validity are read on the device, so both
 * parities of the tick replay from captured graphs.  A context that never enables it allocates and launches exactly what it did before.
 *   scTickReadPairSleep returns the report, min(entity count, state_capacity) state words, and of each list min(true count, max_events,
 *   its capacity) ids; each array may be NULL with capacity 0.  It synchronises and fails like scTickReadPairIslands. */
#define SC_TICK_SLEEP_ASLEEP  (1u << 8)
#define SC_TICK_SLEEP_STILL   (1u << 9)
#define SC_TICK_SLEEP_MOVABLE (1u << 10)
#define SC_TICK_SLEEP_INFO_RESYNC         1u
#define SC_TICK_SLEEP_INFO_FELL_OVERFLOW  2u
#define SC_TICK_SLEEP_INFO_WOKE_OVERFLOW  4u
#define SC_TICK_SLEEP_INFO_LIST_TRUNCATED 8u    /* ScTickPairIslandInfo::list_truncated of the same run */
typedef struct ScTickPairSleepInfo      /* 32 bytes */
{
  uint32_t flags;           /* SC_TICK_SLEEP_INFO_* */
  uint32_t asleep;          /* entities asleep */
  uint32_t islands_asleep;  /* island roots asleep, singles included */
  uint32_t fell_asleep;     /* true count of the run's fell_asleep events */
  uint32_t woke;            /* true count of the run's woke events */
  uint32_t awake_entries;   /* entries of the listed touching list whose edge island is awake */
  uint32_t epoch;           /* flagged runs since the last resync, that run being 1 */
  uint32_t pad;             /* 0 */
} ScTickPairSleepInfo;
int scTickSetPairSleep(ScTickContext* ctx, uint32_t enable, float lin_tol, float ang_tol, uint32_t rest_runs, uint32_t max_events);
int scTickGetPairSleep(ScTickContext* ctx, uint32_t* enabled, float* lin_tol, float* ang_tol, uint32_t* rest_runs, uint32_t* max_events);
/* ids: [n] rank << 24 | index of own entities below the count */
int scTickWakeEntities(ScTickContext* ctx, const uint32_t* ids, uint32_t n);
int scTickReadPairSleep(ScTickContext* ctx, uint32_t* states, uint32_t state_capacity, uint32_t* fell_asleep, uint32_t fell_capacity,
                        uint32_t* woke, uint32_t woke_capacity, ScTickPairSleepInfo* info);

/* ---- touch events: the tick-to-tick difference of the touching set ----
 * Pair events report begin / end for the AABB pair set; the touching pairs decide which pairs really overlap but return the whole list on
 * every tick, with no memory.  A host that keeps a contact cache or fires trigger enter / exit wants begin / end of TOUCHING: two yawed
 * vehicles in neighbouring lanes are an AABB pair that never touches, and a pedestrian capsule meets the bounding cube of a rotated prop
 * metres before it meets the prop.  This build's OWN SPEC: the "pair events" text with "this tick's pair set" replaced by "this tick's
 * touching set".
 *   THE SET    The touching set of a tick is the set of distinct pairs (a, b), a < b, of this tick's pair list that the "touching pairs"
 *              section does not prove apart: the same three routines, the same refinability rule, the same fp32 operation order.  A pair
 *              with a member that is not refinable -- a BOUNDS proxy, a neighbour tile's border record, a degenerate matrix, any member
 *              of a context without colliders -- is in the set on its AABB answer; so in a world without uploaded colliders touch events
 *              equal pair events as sets.  A pair that the pair list names twice is in the set once.
 *   The flag needs neither SC_TICK_PAIR_SHAPES nor scTickSetPairShapes, and max_touching does not limit it: a truncated touching LIST
 *   (ScTickPairShapeInfo::truncated) loses no event.  With both flags in a run each pair is decided once, in one pass.
 *   scTickSetTouchEvents(max_tracked_pairs, max_events) enables them (and sizes every buffer; (0, 0) switches them off and frees the
 *   buffers).  The context then remembers the touching set of the last run that carried SC_TICK_TOUCH_EVENTS.  A run with the flag reports
 *     begun   the pairs of this tick's touching set that are not in the remembered set
 *     ended   the pairs of the remembered set that are not in this tick's touching set
 *   and then remembers its own set.  Ids are rank << 24 | dense index, a < b.  The order inside a list is unspecified.  Runs without the
 *   flag leave the remembered set alone.
 *   RESYNC     begun = the whole touching set, ended = nothing, resync = 1: on the first flagged run, after scTickRemoveEntities, a
 *              shrinking scTickSetEntityCount, scTickSetTile to another rank, and after an overflow tick -- exactly where pair events
 *              resync; a rename between the halves of a split tick is forgotten again behind the pair half, as for pair events.
 *              Appends force no resync, nor do topology, layer or COLLIDER uploads: their effect arrives as ordinary events -- a collider
 *              that shrinks ends its touches, a type change is decided by the new shape.
 *   OVERFLOW   the pair list was truncated (ScTickCounts::pairs_truncated), or this tick's touching set holds more than
 *              max_tracked_pairs distinct pairs: overflow = 1, every count 0, both lists empty, the remembered set is dropped; the next
 *              flagged run that fits is a resync tick.  It is the TOUCHING count that decides: a tick with 1 000 AABB pairs of which 40
 *              touch fits max_tracked_pairs = 40.
 *   TRUNCATED  more than max_events pairs begin, or end: begun / ended carry the true totals, each list holds max_events valid members,
 *              events_truncated = 1.  The remembered set is whole all the same.
 * Order behind the pair search, on its stream (after scTickRunPairs in a split flow): the narrow phase -- ONE pass for the touching list
 * and / or the touch events -- then the pair events, which keep diffing the AABB set: their output is the same with touch events on or
 * off.  No host round trip; the launches replay from a captured graph.  Device memory, as for pair events: two tables of slots x 8 bytes,
 * slots = the power of two >= 2 x max_tracked_pairs (at least 64), plus slots / 4 bytes of marks, plus 2 x max_events x 8 bytes.
 * scTickSetTouchEvents drops captured graphs, asks for no learn tick, and fails while scTickRunPairs is pending.  A context that never
 * calls it allocates and launches exactly what it did before.
 * scTickRun / scTickTileStep fail, with a last-error text and nothing changed, for SC_TICK_TOUCH_EVENTS without SC_TICK_BROADPHASE, without
 * a prior scTickSetTouchEvents, or on a pipelined context (scTickSetPipelined / scTickSetPairsStream: its tick parities overlap in time,
 * and by the time its pair half runs the matrices may be the next tick's).  In the caller-owned split flow the pending pair half reads
 * matrices, colliders and dense indices as they stand, so between scTickRun(.. | SC_TICK_SPLIT_PAIRS | SC_TICK_TOUCH_EVENTS) and its
 * scTickRunPairs the calls refused for a pending SC_TICK_PAIR_SHAPES tick are refused too: scTickUploadWorldMatrices,
 * scTickUploadColliders, scTickRemoveEntities, scTickSetEntityCount, scTickRun with SC_TICK_XFORM.  scTickReadTouchEvents fails when the
 * last run did not carry the flag and while scTickRunPairs is pending.
 * Not covered: contacts (point, normal, depth), a neighbour tile's shapes (its records stay on their box answer), pipelined tiles. */
typedef struct ScTickTouchEventInfo
{
  uint32_t begun, ended;       /* pairs that begun / ended touching this tick (true totals: may exceed max_events, and the caller's capacities) */
  uint32_t tracked;            /* size of the remembered touching set after this tick */
  uint32_t resync;             /* 1 = nothing was remembered: begun is this tick's whole touching set */
  uint32_t overflow;           /* 1 = the set did not fit: nothing is listed, nothing is remembered */
  uint32_t events_truncated;   /* 1 = begun or ended exceeds max_events */
} ScTickTouchEventInfo;
int scTickSetTouchEvents(ScTickContext* ctx, uint32_t max_tracked_pairs, uint32_t max_events);
/* begun2 / ended2: [cap][2] (a, b), either may be NULL with capacity 0; min(count, max_events, capacity) pairs are written to each.
 * Synchronises; copies the 24 bytes of `info` and the listed pairs, nothing else. */
int scTickReadTouchEvents(ScTickContext* ctx, uint32_t* begun2, uint32_t begun_cap, uint32_t* ended2, uint32_t ended_cap, ScTickTouchEventInfo* info);

/* ---- exact shapes for capsule sweeps: sphere, capsule, oriented box ----
 * The capsule sweeps answer from the broadphase's WORLD AABBs with the sweeper's own AABB: a pedestrian capsule walking past a prop yawed
 * by 45 degrees is stopped by the corner of the prop's bounding square, and the sweeper itself has square corners.  The reference sweeps
 * Bullet's rounded capsule through Bullet's exact shapes (convexSweepTest behind PhysicsWorld::sweepCapsule, sc_physics.cpp:779-810), an
 * iterative convex cast.  scTickSetSweepShapes(SC_TICK_SWEEP_SHAPES_EXACT) makes the runs with SC_TICK_SWEEPS answer a candidate whose
 * proxy comes from a typed collider (scTickUploadColliders: BOX, SPHERE, CAPSULE) by a conservative advancement of the capsule itself
 * towards the shape itself, over the distance routines of the touching pairs.  The grown-AABB test stays as the pre-filter; the sector
 * walk, the filter, the skip rule, the tie rule, ScTickSweepHit, scTickSetSweepQueries and scTickReadSweepHits are what they were.
 * This build's OWN SPEC.  All arithmetic is fp32, unfused, left to right, with correctly rounded / and sqrt; dot as the rays define it.
 * A candidate record passes the filter and the skip test, then the capsule sweeps' slab test against its grown AABB (sweeper e, segment
 * (start, ndir, far) as defined there) -- a capsule lies inside its AABB and a collider's shape inside its world AABB, so the pre-filter
 * loses nothing.
 *   A grown-AABB miss: the candidate does not answer, in both modes.
 *   A grown-AABB hit with entry time t0 (the slab test's t) in EXACT mode is REFINED when the box's id is refinable the way a member of
 *   a touching pair is: colliders were uploaded, the id's rank is this context's, e = id & 0xFFFFFF is below the entity count, the collider
 *   type of e is BOX, SPHERE or CAPSULE, and every n_k is finite and > 0.  Otherwise the grown-AABB answer stands, bit for bit as in AABB
 *   mode: BOUNDS proxies, a neighbour tile's border records, degenerate matrices, a context without colliders.
 * The sweeper at travel t is a ROUND in the sense of the touching pairs: centre c(t) = start + ndir*t per component, A = (0, hh, 0) with
 * hh as the capsule sweeps define it -- not hh*hh > 0: A = (0, 0, 0), a sphere --, R = radius.  The target's round (A_t, R_t) or box frame
 * (u_k, H_k, T) is what the touching pairs build from its matrix and record.
 *   dist2(t)  SPHERE, CAPSULE: routine 1 of the touching pairs with p1 = c(t) - A, d1 = A + A, p2 = T - A_t, d2 = A_t + A_t: its
 *             dot(v, v).  ps - pt below is that v.
 *             BOX: routine 2 with w = c(t) - T: its fmin, together with the parameter it was found at -- at = 0 for F(0), and every later
 *             evaluation of the fifteen, in the routine's order (F(1); then per interval i: F(ts), and for i < 6 F(hi)), takes over only
 *             when strictly smaller.  ps = (c(t) - A) + (A + A)*at per component; z_k = the coordinate y0_k + dy_k*at clamped into the box,
 *             lo = (y < -H_k) ? -H_k : y, z_k = (lo > H_k) ? H_k : lo;  pt_i = ((u_0[i]*z_0 + u_1[i]*z_1) + u_2[i]*z_2) + T_i.
 *   Rs        R + R_t for a SPHERE or CAPSULE target, R for a BOX.     gap(t) = sqrt(dist2(t)) - Rs.
 * gap is convex in t (the distance of two convex sets in linear relative motion) and ndir is a unit vector, so neither a step of gap(t)
 * metres nor a step to the zero of the secant through two iterates left of the first contact passes that contact:
 *   t = t0;  no previous iterate;  repeat SC_TICK_SWEEP_SHAPES_STEPS times:
 *     d2 = dist2(t)
 *     t == 0 and not d2 > Rs*Rs:   INSIDE: hit, t = +0, normal (0,1,0) -- the touching pairs' comparison: a NaN is inside
 *     g = sqrt(d2) - Rs
 *     g <= SC_TICK_SWEEP_SHAPES_TOL:   HIT at t
 *     far == 0:   MISS (an overlap test makes one evaluation)
 *     step = g;   with a previous iterate (tp, gp):  slope = (g - gp) / (t - tp);  not slope < 0: MISS (convex and not approaching: it
 *                 never arrives);  sec = (-g) / slope;  sec > step: step = sec
 *     (tp, gp) = (t, g);  t = t + step;  t > far: MISS
 *   after the last repetition: HIT at the t reached, counted in `exhausted` -- a sweep never passes through what it ran out of steps for.
 * A HIT's normal: v = ps - pt of the last evaluation made, vv = dot(v, v); vv > 0: v / sqrt(vv) per component, else (0,1,0).
 * The rest of the hit: position = start + ndir*t (the capsule's centre), travel = t, distance = t / far (0 when far == 0), layer and id as in
 * AABB mode.  Among candidates the smallest t wins -- refined or standing alike -- and equal t goes to the lower id.
 * scTickGetSweepShapeInfo reports what the last run's sweeps did with their candidates.  A candidate is a box that passed the filter, the
 * skip test and the grown-AABB test of one sweep; it is counted once for that sweep however many sectors hold a record of it, for the
 * first SC_TICK_SWEEP_SHAPES_SEEN candidates of a sweep (beyond that a box met again in another sector counts again).  The words are
 * zeroed and written on the device: a captured graph replays them.
 * The mode is a property of the context and stays until it is changed (default AABB).  Setting it drops captured graphs and asks for no
 * learn tick.  It fails on an unknown mode and while scTickRunPairs is pending.  A run with SC_TICK_SWEEPS in EXACT mode fails on a
 * pipelined context (scTickSetPipelined / scTickSetPairsStream): by the time its sweeps are cast the matrices may be the next tick's.
 * In-order tiles and the caller-owned split flow work, with the exact rays' restriction on the latter: between
 * scTickRun(.. | SC_TICK_SPLIT_PAIRS | SC_TICK_SWEEPS) in EXACT mode and its scTickRunPairs, scTickUploadWorldMatrices,
 * scTickUploadColliders, scTickRemoveEntities, scTickSetEntityCount and scTickRun with SC_TICK_XFORM fail and change nothing.  A context
 * that never calls scTickSetSweepShapes allocates and launches exactly what it did before; AABB mode launches the kernel it always did.
 * Not covered: rotated sweepers (the reference's is upright), contact points, a neighbour tile's shapes, pipelined tiles. */
enum { SC_TICK_SWEEP_SHAPES_AABB = 0, SC_TICK_SWEEP_SHAPES_EXACT = 1 };
#define SC_TICK_SWEEP_SHAPES_TOL   1e-3f   /* metres */
#define SC_TICK_SWEEP_SHAPES_STEPS 12
#define SC_TICK_SWEEP_SHAPES_SEEN  256u
typedef struct ScTickSweepShapeInfo
{
  uint32_t refined;         /* candidates answered by their shape */
  uint32_t kept_as_boxes;   /* candidates left on their grown-AABB answer */
  uint32_t exhausted;       /* refined candidates that ran out of steps: reported as a hit at the travel reached */
  uint32_t pad;             /* 0 */
} ScTickSweepShapeInfo;
int scTickSetSweepShapes(ScTickContext* ctx, uint32_t mode);   /* default SC_TICK_SWEEP_SHAPES_AABB */
int scTickGetSweepShapes(ScTickContext* ctx, uint32_t* mode);
/* of the last scTickRun(... | SC_TICK_SWEEPS) (after scTickRunPairs in a split flow); fails when that run did not carry the flag or swept
 * in AABB mode.  Synchronises; copies the 16 bytes of `info`. */
int scTickGetSweepShapeInfo(ScTickContext* ctx, ScTickSweepShapeInfo* info);

/* ---- overlap queries: collider volumes answered from this tick's boxes ----
 * "Which entities are inside this volume": a trigger zone, a blast radius, a spawn-clearance box, an editor's box select, what a
 * kinematic body stands in.  The rays and the sweeps answer "what does this segment meet first", the pair search "which boxes meet each
 * other"; an overlap query is a COLLIDER WITHOUT AN ENTITY, tested against the world exactly as the touching pairs test a pair.  Answered
 * where the rays are: after the bins are filled and before the pair search consumes them.
 * This build's OWN SPEC, like the rays, the sweeps and the touching pairs.  All arithmetic is fp32, unfused, left to right, with correctly
 * rounded / and sqrt; dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 *   volume q    a collider type (SC_TICK_COLLIDER_BOX, _SPHERE or _CAPSULE), its values stored as scTickUploadColliders stores them -- the
 *               record (ex, ey, ez, radius) is a box's half extents and 0, (0, 0, 0, radius) for a sphere, (0, max(0, half_height), 0,
 *               radius) for a capsule --, an affine world matrix (mat16, column-major like scTickUploadWorldMatrices; its last row is
 *               not read), a mask and a skip_id (NULL: 0xFFFFFFFF, none)
 *   volume box  the collider box rule (scTickUploadColliders) applied to the volume's matrix M: n_k = (M[0,k]^2 + M[1,k]^2) + M[2,k]^2;
 *               pad = 0 for a box, radius * sqrt(max(n_0, n_1, n_2)) for a sphere -- m = (n_2 < n_1) ? n_1 : n_2, then (n_0 < m) ? m : n_0 --
 *               and radius * sqrt((n_0 < n_2) ? n_2 : n_0) for a capsule; h_r = ((|M[r,0]|*ex + |M[r,1]|*ey) + |M[r,2]|*ez) + pad;
 *               min_r = M[r,3] - h_r, max_r = M[r,3] + h_r
 *   candidates  every record the ray queries see -- this tick's bins, big list and sector overflow list.  A record passes when
 *               (group & mask) != 0 and the proxy's own mask is not empty (the rays' filter), its id is not skip_id, and its box meets the
 *               volume's box under the pair search's rule: closed intervals on all three axes, box.min <= volume.max and volume.min <=
 *               box.max, positive comparisons only.  A NaN in the volume's box therefore meets nothing: zero hits, reported, not an error.
 *   SC_TICK_OVERLAP_SHAPES_AABB   every candidate is a hit.
 *   SC_TICK_OVERLAP_SHAPES_EXACT  a candidate whose entity is refinable as a member of a touching pair is -- colliders were uploaded, the
 *               id's rank is this context's, e = id & 0xFFFFFF is below the entity count, the collider type of e is BOX, SPHERE or
 *               CAPSULE, and the three n_k of e's world matrix of this tick are finite and positive -- is a hit unless the touching pairs'
 *               routine for the two types says "apart" ("touching pairs": round-round, round-box, box-box), with the ENTITY AS MEMBER A
 *               AND THE VOLUME AS MEMBER B -- the order a pair (i, j), i < j, has when the volume is given the id n + q.  A candidate that
 *               cannot be refined (a BOUNDS proxy, a degenerate matrix, a context without colliders) stays a hit on its box answer, and so
 *               does every candidate of a volume whose own n_k are not all finite and positive.
 *   output      per volume the TRUE number of hits and up to max_hits ids (rank << 24 | dense index, as a ray hit carries them) in
 *               unspecified order.  An entity appears at most once however many sectors hold a record of its box.  When the count exceeds
 *               max_hits the slots hold max_hits distinct members of the true set, which ones is unspecified, and the volume counts as
 *               truncated.
 * The walk: the sectors floorf(min * invSector) .. floorf(max * invSector) of the volume's box in x and z, clamped to the grid.  Two closed
 * intervals that meet share a point and a box is registered in every sector of that same range of its own, so the answer equals brute
 * force over every registered box; a box in several sectors is reported from the one that holds the low corner of the two boxes'
 * intersection, as a pair is.  The cost is linear in the sectors the volume's box covers: a volume over the whole grid reads every bin.
 * scTickSetOverlapQueries: type [count]; mat16 [count][16]; half_extents3 [count][3]; radius, half_height, mask [count]; skip_id [count]
 * or NULL.  Every array but skip_id is required whatever the types.  The set stays until it is replaced; count 0 clears it.  It fails --
 * and leaves the previous set in place -- on a non-finite matrix entry (the twelve that are read), half extent, radius or half_height, a
 * type other than BOX, SPHERE, CAPSULE, max_hits == 0 with count > 0, a count * max_hits beyond 2^30 - 1 id slots, and an unknown
 * mode.  A call with THE SAME count, max_hits and mode as the current set only rewrites the volumes, behind
 * whatever is queued: no learn tick, and a captured graph stays valid.  Anything else re-sizes the set (the query batches' grow rule),
 * costs a learn tick and a fresh capture.
 * skip_id is an id like any other the caller holds: scTickRemoveEntities does NOT rename it when the entity it names is relocated.
 * A run with SC_TICK_OVERLAPS fails, with a last-error text, without SC_TICK_BROADPHASE, without a set (count 0 or never set), together
 * with SC_TICK_SPLIT_PAIRS, on a context with neighbours (scTickSetTile with a non-zero mask) and on a pipelined context: tiles are not
 * covered.  The flag makes the tick fill every bin (no quiet tick, no lazy records), like the rays. */
enum { SC_TICK_OVERLAP_SHAPES_AABB = 0, SC_TICK_OVERLAP_SHAPES_EXACT = 1 };
typedef struct ScTickOverlapInfo
{
  uint32_t queries;            /* volumes of the set the run answered */
  uint32_t max_hits;           /* id slots per volume */
  uint32_t hits;               /* sum of the true counts */
  uint32_t truncated_queries;  /* volumes whose count exceeds max_hits */
  uint32_t refined;            /* EXACT: candidates decided by a shape routine (hits or not); 0 in AABB mode */
  uint32_t kept_as_boxes;      /* EXACT: hits left on their box answer; 0 in AABB mode */
  uint32_t shapes;             /* the mode the run answered in */
  uint32_t pad;                /* 0 */
} ScTickOverlapInfo;
#ifdef __cplusplus
static_assert(sizeof(ScTickOverlapInfo) == 32, "ScTickOverlapInfo is 32 bytes");
#else
_Static_assert(sizeof(ScTickOverlapInfo) == 32, "ScTickOverlapInfo is 32 bytes");
#endif
int scTickSetOverlapQueries(ScTickContext* ctx, uint32_t count, const uint8_t* type, const float* mat16, const float* half_extents3,
                            const float* radius, const float* half_height, const uint32_t* mask, const uint32_t* skip_id,
                            uint32_t max_hits, uint32_t shapes);
/* results of the last scTickRun(... | SC_TICK_BROADPHASE | SC_TICK_OVERLAPS): counts [query_capacity], ids [query_capacity][max_hits] (row
 * q: the first min(counts[q], max_hits) slots), for the first min(queries, query_capacity) volumes; `info` alone (counts and ids NULL)
 * gives the sizes.  Each of counts, ids and info may be NULL.  Synchronises; the report's sums are formed by this call from the per-volume
 * words the device wrote (saturating at 2^32 - 1). */
int scTickReadOverlapHits(ScTickContext* ctx, uint32_t* counts, uint32_t* ids, uint32_t query_capacity, ScTickOverlapInfo* info);

/* ---- trigger volumes: anchored overlap volumes with enter / exit events ----
 * A trigger zone rides on an entity -- a vehicle's proximity zone, a pedestrian's personal space, a pickup, the reference's
 * Collider::isTrigger bodies (CF_NO_CONTACT_RESPONSE: sc_physics.h:27, sc_physics.cpp:346-347, :438-439) -- and its consumer wants "who
 * came in, who left", not the member list.  A trigger volume is to an overlap query what an entity-anchored ray is to a ray: given in
 * its anchor's LOCAL frame, resolved on the device against this tick's world matrix, answered as the overlap query of the resolved volume
 * would be, and reported as the DIFFERENCE against the last run that carried SC_TICK_TRIGGERS.  A set of its own with a flag of its own;
 * a context that never calls scTickSetTriggerVolumes allocates and launches nothing for it.
 * This build's OWN SPEC.  All arithmetic is fp32, unfused, left to right.
 *   resolve     W = the anchor's world matrix rows as this run's transform stage leaves them (without SC_TICK_XFORM: as they stand), L =
 *               the volume's local affine matrix (local_mat16, column-major; its last row is not read).  For r, k in 0..2:
 *                 M[r,k] = (W[r,0]*L[0,k] + W[r,1]*L[1,k]) + W[r,2]*L[2,k]
 *                 M[r,3] = ((W[r,0]*L[0,3] + W[r,1]*L[1,3]) + W[r,2]*L[2,3]) + W[r,3]
 *               anchor == SC_TICK_ANCHOR_NONE: M = L untouched (a world-space zone).  A volume has NO MEMBERS this tick when its anchor
 *               is >= the entity count at run time (SC_TICK_ANCHOR_DEAD always is) or one of the twelve entries of M is not finite;
 *               scTickReadTriggerMatrices then reports all twelve as the quiet NaN 0x7FC00000.
 *   members     exactly what scTickSetOverlapQueries answers for a volume with matrix M, the same type, values and mask: the volume box,
 *               the candidates, the filter, the closed-interval pair rule, the low-corner rule ("every entity once"), and in
 *               SC_TICK_OVERLAP_SHAPES_EXACT mode the touching pairs' routines with the entity as member A ("overlap queries" above).  An
 *               unanchored trigger volume's member set equals the overlap query's answer for the same volume, in both modes.
 *               skip_self[v] != 0 (NULL: all 1): the id (rank << 24 | anchor) never answers; without an anchor it has no effect.
 *   events      an event is a pair (volume index, id), id = rank << 24 | dense index.  The context remembers, per volume, the member row of
 *               the last run that carried SC_TICK_TRIGGERS.  A flagged run reports entered = members now that were not remembered and
 *               exited = remembered members that are not members now, then remembers its own rows.  Unflagged runs leave the memory
 *               alone.  The order inside both lists and inside a row is unspecified.
 *   RESYNC      per volume (info.resync_volumes): nothing was remembered for it -- entered is its whole row, exited nothing.  Every volume
 *               on the first flagged run after a set call that re-sizes, scTickRemoveEntities, a shrinking scTickSetEntityCount and
 *               scTickSetTile with another rank (ids are renamed); one volume after its own overflow tick.  Appends, and topology, layer and
 *               collider uploads, force no resync.
 *   OVERFLOW    per volume (info.overflow_volumes): its true count exceeds max_members.  Its row holds max_members distinct members of the
 *               true set, as a truncated overlap row does; it contributes NO events, its memory is dropped (it resyncs on the next flagged
 *               tick on which it fits), and it is counted here and not under resync_volumes.  The other volumes are untouched.
 *   TRUNCATED   more than max_events entries enter, or leave, over all volumes: info.entered / info.exited carry the true totals, each
 *               list holds max_events valid, distinct entries, events_truncated = 1.  The memory is complete all the same: the host
 *               recovers the tick from scTickReadTriggerMembers.  Nothing is lost silently.
 * The row cap.  While a wave forms the two differences it holds the volume's new row and its remembered row in LDS: 2 rows x
 * SC_TICK_TRIGGER_MAX_MEMBERS x 4 bytes = 8 KB per wave, 32 KB for the four waves of a workgroup, five workgroups in a CU's 160 KB.
 * scTickSetTriggerVolumes: anchor, type, radius, half_height, mask [count]; local_mat16 [count][16]; half_extents3 [count][3]; skip_self
 * [count] or NULL.  Every array but skip_self is required whatever the types.  The set stays until it is replaced; count 0 clears it and
 * frees it.  The call fails -- and leaves the previous set in place -- on a non-finite entry among the twelve read from local_mat16, a
 * non-finite half extent, radius or half_height, a type other than BOX, SPHERE, CAPSULE, max_members == 0 with count > 0, max_members
 * above SC_TICK_TRIGGER_MAX_MEMBERS, a count * max_members beyond 2^30 - 1 id slots, an unknown mode (SC_TICK_OVERLAP_SHAPES_*), a required
 * array NULL, and while scTickRunPairs is pending.  A call with THE SAME count, max_members, max_events and mode as the current set only
 * rewrites anchors, locals and values, behind whatever is queued: it KEEPS THE REMEMBERED ROWS, costs no learn tick and leaves a captured
 * graph valid -- a world-space zone moved by hand this way yields ordinary events.  Anything else re-sizes the set (the query batches'
 * grow rule, as scTickSetOverlapQueries), forgets every row, costs a learn tick and a fresh capture.
 * Residency: scTickRemoveEntities renames the anchors of relocated entities (moved_from -> moved_to) and turns the anchors of removed ones
 * into SC_TICK_ANCHOR_DEAD, as for the anchored rays; skip_self follows because it is derived from the anchor.
 * A run with SC_TICK_TRIGGERS fails, with a last-error text, where one with SC_TICK_OVERLAPS does: without SC_TICK_BROADPHASE, without a
 * set, together with SC_TICK_SPLIT_PAIRS, on a context with neighbours and on a pipelined context -- tiles are not covered.  The flag
 * makes the tick fill every bin (no quiet tick, no lazy records), like the other bin readers. */
#define SC_TICK_TRIGGER_MAX_MEMBERS 1024u   /* max_members at most: 2 rows x 1 024 ids x 4 bytes = 8 KB of LDS per wave */
typedef struct ScTickTriggerInfo
{
  uint32_t volumes;            /* volumes of the set the run answered */
  uint32_t max_members;        /* id slots per volume */
  uint32_t members;            /* sum of the true counts */
  uint32_t entered;            /* true total of entries */
  uint32_t exited;             /* true total of exits */
  uint32_t resync_volumes;     /* volumes nothing was remembered for (and that did not overflow) */
  uint32_t overflow_volumes;   /* volumes whose count exceeds max_members */
  uint32_t events_truncated;   /* 1: entered or exited exceeds max_events */
} ScTickTriggerInfo;
#ifdef __cplusplus
static_assert(sizeof(ScTickTriggerInfo) == 32, "ScTickTriggerInfo is 32 bytes");
#else
_Static_assert(sizeof(ScTickTriggerInfo) == 32, "ScTickTriggerInfo is 32 bytes");
#endif
int scTickSetTriggerVolumes(ScTickContext* ctx, uint32_t count, const uint32_t* anchor, const uint8_t* type, const float* local_mat16,
                            const float* half_extents3, const float* radius, const float* half_height, const uint32_t* mask,
                            const uint8_t* skip_self, uint32_t max_members, uint32_t max_events, uint32_t shapes);
/* The reads below answer for the last scTickRun(... | SC_TICK_BROADPHASE | SC_TICK_TRIGGERS); they fail when the last run lacked the flag
 * or the set was re-sized since.  They synchronise; the report's sums are formed by the call from the per-volume words the device wrote
 * (saturating at 2^32 - 1).  Every output pointer may be NULL.
 * events: entered2 [entered_cap][2], exited2 [exited_cap][2] as (volume, id); min(info.entered, max_events, entered_cap) pairs are written
 * (likewise exited). */
int scTickReadTriggerEvents(ScTickContext* ctx, uint32_t* entered2, uint32_t entered_cap, uint32_t* exited2, uint32_t exited_cap, ScTickTriggerInfo* info);
/* members: counts [volume_capacity] (true counts), ids [volume_capacity][max_members] (row v: the first min(counts[v], max_members) slots),
 * for the first min(volumes, volume_capacity) volumes */
int scTickReadTriggerMembers(ScTickContext* ctx, uint32_t* counts, uint32_t* ids, uint32_t volume_capacity, ScTickTriggerInfo* info);
/* the resolved world matrices of the last flagged run: mat16 [count][16], column-major with the last row (0, 0, 0, 1) */
int scTickReadTriggerMatrices(ScTickContext* ctx, uint32_t first, uint32_t count, float* mat16);
/* the anchors as they stand now (renamed or SC_TICK_ANCHOR_DEAD after scTickRemoveEntities); host-side, needs no run */
int scTickReadTriggerVolumes(ScTickContext* ctx, uint32_t first, uint32_t count, uint32_t* anchor);

/* ---- entity-anchored capsule sweeps over the broadphase bins ----
 * Capsule sweeps that follow an entity on the device: what the anchored rays are to the ray queries and the trigger volumes to the overlap
 * queries.  The consumer of a capsule sweep is almost always a moving entity -- a pedestrian's or a kinematic body's move test, a ground
 * probe under a vehicle, the clearance test ahead of an agent (PhysicsWorld::sweepCapsule, sc_physics.h:179, sc_physics.cpp:779-810, takes
 * start and end in world space) -- and in resident mode that entity's pose of this frame exists only on the device.  An anchored sweep is
 * given once, in its anchor's LOCAL frame; every run with SC_TICK_ANCHORED_SWEEPS resolves it against that tick's world matrix of the
 * anchor and answers it against that tick's boxes: no host round trip, no learn tick, no graph re-capture in the frame loop.
 * This build's OWN SPEC.  All arithmetic is fp32, unfused, left to right.  For sweep k with anchor a, local start ls, local end le, and
 * R_r = (w_r.x, w_r.y, w_r.z, w_r.w) row r (0..2) of a's world matrix as this run's transform stage leaves it (without SC_TICK_XFORM: as
 * it stands on the device):
 *   s_r = ((R_r.x*ls.x + R_r.y*ls.y) + R_r.z*ls.z) + R_r.w                       (the anchored rays' origin formula)
 *   end_frame SC_TICK_SWEEP_END_LOCAL (0)         le is a point in the anchor's frame:   e_r by the same formula as s_r
 *   end_frame SC_TICK_SWEEP_END_WORLD_OFFSET (1)  le is a world-space displacement:      e_r = s_r + le_r
 * (the offset form: a probe "0.4 m straight down whatever the chassis' tilt", a world velocity times dt).
 *   anchor      SC_TICK_ANCHOR_NONE: s = ls untouched; e = le untouched (frame 0), e_r = ls_r + le_r (frame 1)
 * The resolved sweep (s, e, radius, half_height, mask, skip_id) is then answered exactly as a sweep of scTickSetSweepQueries, under the
 * context's sweep mode (scTickSetSweepShapes: AABB or EXACT): same sweeper, same zero-length rule (|e - s|^2 <= 1e-6: an overlap test at
 * s), same filter, same tests, same tie rule, same ScTickSweepHit.  An unanchored frame-0 sweep equals the plain sweep query's answer bit
 * for bit, in both modes.
 *   skip_self   != 0 (NULL: every sweep) on a sweep that has an anchor: skip_id = rank << 24 | a, the anchor's own box never answers;
 *               otherwise no box is skipped
 *   radius, half_height   world metres: the anchor's scale does not scale them, and the sweeper stays UPRIGHT in world space whatever the
 *               anchor's rotation (the reference's sweeper is upright) -- a limit of this spec
 * ScTickSweepHit::pad carries the sweep's status:
 *   SC_TICK_ASWEEP_ANSWERED (0)    the record is the answer
 *   SC_TICK_ASWEEP_NO_ANCHOR (1)   the anchor is >= the entity count at run time (SC_TICK_ANCHOR_DEAD always is)
 *   SC_TICK_ASWEEP_NOT_FINITE (2)  a component of s or e is not finite, or (d.x*d.x + d.y*d.y) + d.z*d.z of d = e - s is not finite
 * Statuses 1 and 2 are a miss (SweepHit{}) and scTickReadAnchoredSweepSegments reports the quiet NaN 0x7FC00000 in all six words for
 * them: a mover that lost its anchor must not read "path clear", which is why the status exists and is not 0.
 * scTickGetAnchoredSweepShapeInfo reports the three words of ScTickSweepShapeInfo for the last run with this flag in EXACT mode, under
 * the rules of scTickGetSweepShapeInfo; the report is separate from the plain sweeps': a run with both flags fills both.
 * Residency: scTickRemoveEntities renames the anchors of relocated entities and turns the anchors of removed ones into
 * SC_TICK_ANCHOR_DEAD, as for the anchored rays and the trigger volumes.  scTickAppendEntities and scTickSetEntityCount leave them alone.
 * A run with SC_TICK_ANCHORED_SWEEPS fails, with a last-error text, without SC_TICK_BROADPHASE, without a set, together with
 * SC_TICK_SPLIT_PAIRS, on a context with neighbours and on a pipelined context -- tiles are not covered.  The flag makes the tick fill
 * every bin (no quiet tick, no lazy records), like the other bin readers.  A context that never calls scTickSetAnchoredSweeps allocates
 * and launches nothing for them.
 * Not covered: rotated sweepers, a capsule scaled by its anchor, tiles, split flows, pipelined contexts, contact points. */
enum { SC_TICK_SWEEP_END_LOCAL = 0, SC_TICK_SWEEP_END_WORLD_OFFSET = 1 };
enum { SC_TICK_ASWEEP_ANSWERED = 0, SC_TICK_ASWEEP_NO_ANCHOR = 1, SC_TICK_ASWEEP_NOT_FINITE = 2 };
/* anchor, radius, half_height, mask: [count]; local_start3 / local_end3: [count][3]; skip_self: uint8 [count] or NULL (all 1); end_frame:
 * uint8 [count] or NULL (all 0).  The set stays until it is replaced; count 0 clears and frees it.  A call with THE SAME COUNT as the
 * current set only rewrites the device arrays, behind whatever is queued: no learn tick, and a captured graph stays valid; another count
 * behaves like scTickSetSweepQueries.  Fails -- and leaves the previous set in place -- when a local start, local end, radius or
 * half_height is not finite, a radius is negative, an end_frame is neither 0 nor 1, a required array is NULL, or scTickRunPairs is
 * pending. */
int scTickSetAnchoredSweeps(ScTickContext* ctx, uint32_t count, const uint32_t* anchor, const float* local_start3, const float* local_end3,
                            const float* radius, const float* half_height, const uint32_t* mask, const uint8_t* skip_self,
                            const uint8_t* end_frame);
/* The reads below answer for the last scTickRun(... | SC_TICK_BROADPHASE | SC_TICK_ANCHORED_SWEEPS); they fail when the last run lacked
 * the flag or the set was re-sized since.  They synchronise. */
int scTickReadAnchoredSweepHits(ScTickContext* ctx, ScTickSweepHit* hits, uint32_t capacity, uint32_t* count);
/* the resolved world-space segments of sweeps first .. first + count - 1: start3 / end3 [count][3] (either may be NULL) */
int scTickReadAnchoredSweepSegments(ScTickContext* ctx, uint32_t first, uint32_t count, float* start3, float* end3);
/* of the last run with the flag; fails when that run swept in AABB mode.  Copies the 16 bytes of `info`. */
int scTickGetAnchoredSweepShapeInfo(ScTickContext* ctx, ScTickSweepShapeInfo* info);
/* the anchors as they stand now (renamed or SC_TICK_ANCHOR_DEAD after scTickRemoveEntities); host-side, needs no run */
int scTickReadAnchoredSweeps(ScTickContext* ctx, uint32_t first, uint32_t count, uint32_t* anchor);

/* isOccupiedWorld (src/engine/traffic/sc_traffic_spawner.cpp:93-116), for a batch of at most 256 points: blocked[k] = 1
 * when some entity whose collision group meets mask[k] has dx*dx + dz*dz < radius[k]*radius[k] to point k, measured on
 * Transform::localPos in the xz plane like the reference (which walks its TrafficAgent and VehicleComponent pools; the
 * group mask selects the same entities here).  Answers from the positions as they are on the device now; synchronises. */
int scTickQueryOccupied(ScTickContext* ctx, uint32_t count, const float* pos3, const float* radius, const uint32_t* mask,
                        uint8_t* blocked);

/* ---- measurement ---- */
/* record HIP events around the kernel launches (on the context's stream) of every `enable`-th tick
 * from now on (1 = every tick; event records cost host time, so long runs sample); 0 = stop */
int scTickSetProfiling(ScTickContext* ctx, int enable);
/* ... and only around the kernels of `mask` (bit SC_TICK_K_*; 0 = all, the default).  Timing a launch by events costs ~6 us of gap on the
 * queue: a run that is itself being timed samples the dominant kernel alone. */
int scTickSetProfilingKernels(ScTickContext* ctx, uint32_t mask);
/* durations (ms) of the launches of `kernel` recorded since profiling was enabled; synchronises */
int scTickGetKernelTimes(ScTickContext* ctx, uint32_t kernel, float* ms, uint32_t capacity, uint32_t* count);
/* capture the current stage sequence into a hipGraph and replay it on scTickRun (0 = eager launches).  scTickTileStep on
 * an in-order tile replays the whole step (RCCL group included) as one graph; on a pipelined tile each half of the step is
 * a graph of its own, on its own stream.  Not combinable with the frame read-back.
 * Every setter of this header may be called between two runs while graph replay is on.  The next run re-captures where a
 * captured graph would hold a stale value -- a count, a budget, a mode, a buffer address -- and replays where nothing it holds
 * changed (tests/test_gpu_graph_setters.py; DESIGN.md section 6, "what invalidates a capture"). */
int scTickSetGraphMode(ScTickContext* ctx, int enable);
/* native stream handle (hipStream_t) for callers that order their own work against the tick */
void* scTickGetStream(ScTickContext* ctx);

#ifdef __cplusplus
}
#endif
#endif /* SC_TICK_H */
