// sc_tick_internal.h -- device-side data layout shared by the kernels and the C-ABI implementation.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

namespace sctick {

#ifdef __HIPCC__
// the wave's predicate mask straight from the compare (HIP's __ballot goes through an integer: v_cndmask + v_cmp_ne per call)
__device__ __forceinline__ unsigned long long ballot64(bool pred) { return __builtin_amdgcn_ballot_w64(pred); }
#endif


// ---- link word: one dword per entity carries topology + component flags --------------------
//   bits  0..23  dense index of the parent (kNoParent = root)          Transform::parent
//   bit   24     has RenderMesh  (culling candidate)                   sc_world_partition.cpp:1206-1210
//   bit   25     has Bounds                                            sc_world_partition.cpp:1252-1263
//   bits 26..28  hierarchy depth: 0..kMaxChain exact, kDeep = deeper (handled by level kernels),
//                kUnreachable = in/below a parent cycle (never visited, sc_ecs.cpp:173-210)
//   bits 29..31  rotation about X / Y / Z is trivial: the uploaded sin is exactly 0 and cos exactly 1
//                (angle 0), so the kernel substitutes the constants instead of streaming them
constexpr uint32_t kParentMask  = 0x00FFFFFFu;
constexpr uint32_t kNoParent    = 0x00FFFFFFu;
constexpr uint32_t kHasMesh     = 1u << 24;
constexpr uint32_t kHasBounds   = 1u << 25;
constexpr uint32_t kDepthShift  = 26;
constexpr uint32_t kDepthMask   = 7u;
constexpr uint32_t kMaxChain    = 3;      // ancestors the fused kernel walks itself
constexpr uint32_t kDeep        = 5;      // depth > kMaxChain: level kernels
constexpr uint32_t kUnreachable = 7;
constexpr uint32_t kRotTrivialX = 1u << 29, kRotTrivialY = 1u << 30, kRotTrivialZ = 1u << 31;
__host__ __device__ inline uint32_t linkDepth(uint32_t lk) { return (lk >> kDepthShift) & kDepthMask; }

// collider types (== SC_TICK_COLLIDER_*)
constexpr uint32_t kColliderBounds = 0, kColliderNone = 1, kColliderBox = 2, kColliderSphere = 3, kColliderCapsule = 4;
constexpr uint32_t kPaletteCap = 4096;    // distinct local boxes a context tells apart; entities beyond that are of class "none"
constexpr uint32_t kClassMask = 0xFFFFu, kClassMixed = 0xFFFFu, kClassNone = 0xFFFFu;
constexpr uint32_t kTileNoBounds = 1u << 30;         // host bookkeeping: no entity of the tile has Bounds (the kernel never looks)
constexpr uint32_t kTileLayersShared = 1u << 31;
constexpr uint32_t kTile = 256;           // entities per workgroup pass (4 waves of 64)
// Topology classes (topoTable()): a wave-tile whose parent links all stay inside it and whose chains are at most kMaxChain long
// is "closed"; its pattern is its 64 link words with the parent field replaced by the parent's lane.  The distinct patterns of a world
// (by bit pattern, up to kTopoCap: 128 KiB of table, what the caches keep beside the streams) are numbered, and pattern index + 1 sits in
// bits 16..29 of the tile's word 0 (0: the tile is not classed).  Derived by the host wherever link words are (scTickHostTopologyClasses).
constexpr uint32_t kTopoCap = 256;
constexpr uint32_t kTopoShift = 16, kTopoMask = 0x3FFFu;
constexpr uint32_t kTopoInactive = (7u << 26) | 0x00FFFFFFu;      // the link word of a lane past the entity count: (kUnreachable << kDepthShift) | kNoParent
// One table entry per lane of a pattern, 8 bytes, everything the fused kernel's walk ends up holding:
//   x: bits 24..31 as the link word has them (mesh, bounds, depth, rotation-trivial bits), bits 0..5 / 6..11 / 12..17 the lanes of ancestors
//      1 / 2 / 3 (the lane itself above its depth);  y: the rotation-trivial bits of the lane and of ancestors 1..3, three bits each from bit 0
// the pattern table, [kTopoCap][64] entries of 8 bytes: the kTopoCap * 128 words in front of the bounds palette
__host__ __device__ inline const uint2* topoTable(const float* boundsPalette) { return reinterpret_cast<const uint2*>(boundsPalette) - (size_t)kTopoCap * 64u; }
inline void topoEntry(const uint32_t pattern[64], uint32_t lane, uint32_t out[2])
{
  const uint32_t own = pattern[lane];
  uint32_t x = own & 0xFF000000u, y = own >> 29, cur = own, at = lane;
  for (uint32_t k = 1; k <= 3u; ++k) {
    const bool up = (cur & 0x00FFFFFFu) != 0x00FFFFFFu;
    if (up) { at = cur & 63u; cur = pattern[at]; y |= (cur >> 29) << (3u * k); } else { at = lane; cur = 0x00FFFFFFu; }
    x |= at << (6u * (k - 1u));
  }
  out[0] = x; out[1] = y;
}
constexpr uint32_t kMaxSpanWords = 128;   // spans up to 4096 entities keep the fused producer's ballots in LDS

struct Frustum6 { float p[6][4]; };       // (nx, ny, nz, d) x 6, Frustum (sc_world_partition.h:39-43)

// All 4-byte per-entity streams live in ONE slab, stream k at byte offset k * capBytes, so a kernel
// addresses every stream from a single base (one SGPR pair, 32-bit lane offsets) instead of keeping
// thirty pointers live in scalar registers.  The world-matrix rows form a second slab of float4.
enum Stream : uint32_t {
  kPX, kPY, kPZ, kRSX, kRCX, kRSY, kRCY, kRSZ, kRCZ, kSX, kSY, kSZ,
  kBMINX, kBMINY, kBMINZ, kBMAXX, kBMAXY, kBMAXZ, kLINK, kLAYERS, kMESH, kMATERIAL, kStreamCount
};

// Lane graph of the traffic system (TrafficLaneGraph, src/engine/traffic/sc_traffic_lanes.h:13-30) as the on-rails advance
// reads it: per segment its start node's position and length, its direction and speed limit (laneSpeedLimit = the start
// node's, sc_traffic_lanes.cpp:392-400), its end node, the active flag, and sin / cos of yaw = atan2(dir.x, dir.z) taken with
// the HOST libm when the graph is set -- an on-rails agent's rotation only ever takes these per-segment values
// (sc_traffic_ai.cpp:455), so the device never evaluates a trigonometric function and stays bit-equal to the host.
struct LaneGraphDev {
  const float4* segA;           // start.xyz, length
  const float4* segB;           // dir.xyz, speed limit
  const uint4*  segC;           // end node, active, bits of sin(yaw), bits of cos(yaw)
  const float4* nodePos;        // xyz
  const uint32_t* nodeConnOff;  // [nodes + 1] offsets into nodeConn (LaneNode::connections)
  const uint32_t* nodeConn;     // segment ids
  uint32_t segments, nodes;
};
constexpr uint32_t kInvalidLane = 0xFFFFFFFFu;               // kInvalidLaneId, sc_traffic_common.h:9
constexpr uint32_t kTierPhysics = 0, kTierKinematic = 1, kTierOnRails = 2;   // TrafficSimMode, sc_traffic_common.h:11-16
constexpr uint32_t kMoverTraffic = 3;                        // moverKind of a traffic agent (1 / 2: SynthWorld's straight-line movers)
constexpr uint32_t kTierNearCap = 1u << 16;                  // agents whose desired tier is not OnRails, per selection

// Device SoA state of one context.  All arrays are sized to `cap` (padded to kTile).
struct DeviceState {
  const char* fslab;        // kStreamCount streams x cap x 4 B
  char* rslab;              // 3 row streams x cap x 16 B (w0, w1, w2)
  uint32_t capBytes;        // cap * 4
  uint32_t capBytes16;      // cap * 16
  // inputs: Transform locals (sc_ecs.h:63-71); rotation kept as host-libm sin/cos of the Euler angles
  float *px, *py, *pz;
  float *rsx, *rcx, *rsy, *rcy, *rsz, *rcz;
  float *sx, *sy, *sz;
  uint32_t* link;
  uint32_t* dirty;          // 1 bit per entity (Transform::dirty), word i/32
  uint32_t* unreach;        // 1 bit per entity: depth == kUnreachable (dirty survives the tick there)
  uint32_t* rootMask;       // 1 bit per entity: no parent and reachable (the root nudge's lanes); rebuilt from `link` wherever link words change
  // Bounds::localAabb (sc_world_partition.h:298-301)
  float *bminx, *bminy, *bminz, *bmaxx, *bmaxy, *bmaxz;
  // RenderMesh + collision layers
  uint32_t *meshId, *materialId;
  uint32_t* layers;         // group | mask << 16
  // Bounds classes: a table of the distinct local boxes (found by bit pattern) and, per wave-tile of 64 consecutive entities,
  // what its entities share -- derived from the streams above by the host for the fused kernel alone, which then fetches a
  // shared box / layer word once per tile through the scalar path instead of once per lane.  The streams stay authoritative.
  const float* boundsPalette;  // [kPaletteCap][8]: bmin.xyz, bmax.xyz as uploaded, two words of padding.  The same allocation holds the topology classes'
                               // pattern table IN FRONT of it (topoTable(): no new member, the kernels' argument block keeps its layout)
  const uint32_t* tileClass;   // [cap / 64][2], == boundsPalette + kPaletteCap * 8 words (one allocation: the kernel addresses both from boundsPalette).
                               // word 0 = palette index shared by the tile's entities with Bounds (kClassMixed: none shared) | kTileLayersShared when
                               // the layer words of its entities WITH A PROXY -- with Bounds, while no collider was ever uploaded -- are all equal
                               // (only colliders use the word: never take it for a lane without a proxy); word 1 = that layer word
  // outputs
  float4 *w0, *w1, *w2;     // world matrix rows 0..2 (affine 3x4; row 3 is 0,0,0,1)
  uint64_t* vis;            // visibility bits, word i/64
  uint64_t* cand;           // candidate bits (only written when the culled list is requested)
  uint64_t* recomp;         // "recomputed this tick" bits (only when deep levels exist)
  uint32_t* blockVis;       // visible count per span
  uint32_t* blockCand;      // candidate count per span
  uint32_t* visibleIdx;     // ordered visible dense indices
  uint32_t* culledIdx;
  const float* frustum;     // the six planes (nx, ny, nz, d), device copy refreshed when the host sets them
  uint32_t* counters;       // [0] visible total, [1] culled total, [2] pairs, [3] bin overflow, [4] draws, [5] dropped
  // broadphase
  float4 *aabbMin, *aabbMax;   // dense-order world AABBs (debug / read-back only: SC_TICK_DENSE_AABBS)
  uint32_t* binCount;          // records per sector bin (self-cleaning: the pair kernel zeroes what it read)
  uint32_t* binLayers;         // OR of the records' (group | mask << 16) per bin: lets the pair kernel skip a bin unread
  float4* bins;                // [sector][kBinCap][2]: (min.xyz, layers) (max.xyz, id | primary<<31)
  // Home slots (round 3): where an entity's records went the last time the bins were filled with reservations ("learn" tick).
  // While the entity's box keeps its primary sector, its records go straight to those slots -- no reservation, i.e. no atomic,
  // which on this chip executes at the memory side (11 of the fused kernel's 39 us were its atomics).  Shared by every parity copy.
  uint32_t* homeA;             // [cap] primary sector of the entity's records at the learn tick (0xFFFFFFFF: none)
  uint32_t* homeB;             // [cap] four 8-bit slots: the copies in sectors homeA + {0, 1, binSX, binSX + 1}; 0xFF = no reservation
  uint32_t* homeCount;         // [sectors] slots of each bin that are reserved: what binCount starts a tick from
  uint32_t* homeLayers;        // [sectors] OR of the reserved records' layer words: what binLayers starts a tick from
  // Ordered home slots (round 4): at the learn tick the reserved records of every bin are re-numbered -- and moved -- so that the
  // records that pass the group/mask filter against their own kind ("cast" records: dynamic bodies) come first.  A bin that holds
  // nothing but its reserved records on a later tick is then searched without classifying anything: the cast records are slots
  // [0, D), everything else behind them (k_order_home, "fast sectors" in the pair role).
  uint32_t* homeCast;          // [sectors] bits 0..7: D, cast records among the reserved slots; kCastFast: the rest cannot meet each other
  const uint32_t* pairConst;   // what every pair-role workgroup copies into LDS: words [0, 1008) the triangular pair table (2016 x uint16), [kPairConstCast, +65) the cast table
  const float4* nullRec;       // one null record (nullRecord(): inverted box, layers 0) for lanes that have no bin slot to load
  uint8_t* homePerm;           // [sectors][kBinCap] learn tick only: slot a reserved record moved to (k_home_flags re-numbers homeB through it)
  // Lazy records (round 3): a bin whose reserved records cannot pass the group/mask filter against each other is read by the
  // pair search only when a record from elsewhere arrives that can -- so its owners do not write it (homeB bit 6 of a slot
  // byte = "write every tick"), and the wave that does need such a bin rebuilds its records from the owners' matrices.
  uint32_t* lazyCtl;           // [0] big boxes of the last pair search (!= 0: the next fused kernel writes every record),
                               // [1 + parity] 1 = that tick's fused kernel wrote every reserved record (what its pair search goes by),
                               // [1 + kMaxParity + parity] records / big boxes that arrived from a neighbour outside the declared layer vocabulary
  float4* bigList;             // [cap][2] boxes that cannot be binned (too large, outside the rect, bin full)
  float4* spill;               // [ovfCap][2] sector OVERFLOW list: records that found their sector bin full -- this tile's own
                               // (fused kernel) and the neighbours' border records (merge) alike ...
  uint32_t* spillSector;       // ... and the sector each belongs to: the wave that searches that sector gathers them back
  uint32_t* ovfLo;             // per sector: lowest overflow-list index tagged with it (0xFFFFFFFF: none) ...
  uint32_t* ovfHi;             // ... and one past the highest: the slice a sector's wave has to sweep (entities of a sector sit
                               // together in pool order, so its overflow records sit together in the list)
  uint32_t* crowdQueue;        // [kMaxParity][sectors] crowded sectors of the tick -- queued by whoever was handed slot 64 of a bin -- for the pair search
  uint32_t* ovfIdx;            // [pair-role waves][kOvfPerSector] scratch: overflow-list indices of the sector a wave is working on
  uint2* pairs;                // (a, b) ids, a < b; id = rank << 24 | dense index; kPairShards segments of shardCap
  uint32_t* pairShardCount;    // [kMaxParity parities + snapshot][kPairShards] counters, one per 128-byte line (kShardStride words apart)
  // upstream movers (allocated on first scTickUploadMovers)
  uint32_t* moverKind; float *mvx, *mvz, *mlox, *mloz, *mhix, *mhiz;
  // traffic agents (TrafficAgent + TrafficVehicle, sc_traffic_common.h:26-44; allocated on first scTickUploadTrafficAgents)
  LaneGraphDev lanes;
  uint32_t* aLane; float* aS; float* aSpeed; uint32_t* aMode; float* aLook; uint32_t* aDesired;
  float* aBrake;               // obstacleBrake per agent from its front ray (sc_traffic_ai.cpp:300-345); nullptr = no sensors: brake 0
  // per-agent TrafficSensors (sc_traffic_common.h:46-53): frontRayLength / safeDistance per entity, and what the AI leaves in them (lastHitDistance,
  // lastHitType: 0 none, 2 vehicle, 3 world); allocated with aBrake
  float* aRayLen; float* aSafe; float* aHitDist; uint32_t* aHitType;
  float4* agentRays;           // [cap][2] with the rays cast in the PAIR half (tiled, in order): (origin xyz, ray length) (forward x, forward z, safe distance, -)
                               // of every listed agent as the tick half found them -- the frame producer may have moved the agents on by then
  uint32_t* agentList;         // dense indices of the OnRails agents, rebuilt every tick that casts their rays
  uint32_t* agentCount;
  uint32_t* tierCounts;        // [0..2] desired tiers, [3] entries in tierNear
  uint2* tierNear;             // (dense index, bits of the distance) of agents whose desired tier is Physics or Kinematic
  // multi-GPU border exchange: one message per neighbour direction (caller-owned device buffers)
  uint32_t* borderSend[8];
  uint32_t* borderRecv[8];
  // Colliders (scTickUploadColliders; allocated on its first call, nullptr before: every entity is then kColliderBounds and the
  // kernels' collider instances are never launched).  One 16-byte record per entity, outside the stream slab, in the form the box
  // rule consumes it: (ex, ey, ez, radius) -- a box's half extents, (0, 0, 0) for a sphere, (0, max(0,
  // halfHeight), 0) for a capsule -- and the type in a byte of its own.
  float4* colShape;
  uint8_t* colType;
  // (last on purpose: the offsets of everything above in the kernels' argument block stay what they were)
};

// Border message layout (uint32 words): [0] records in the spill-over area, [1] overflow flag, [2..2+L) per-cell counts,
// then the record capacity (8 words a record): borderFixedSlots() fixed slots for every cell, cell after cell, and behind
// them the spill-over area (what cells hold beyond their fixed slots, packed cell after cell); then the big-box section:
// [0] boxes, [1] overflow flag, boxes (8 words each); then, with traffic sensors on a tiled world, the halo section.
// L = sectors on that ring side.
constexpr uint32_t kPairConstCast = 1008;      // DeviceState::pairConst: first word of the cast table
constexpr uint32_t kPairConstWords = 1076;     // (padded to 16 bytes)
constexpr uint32_t kBorderHeader = 2;
constexpr uint32_t kBorderRecsPerBin = 16;    // default: a message holds L * 16 records (shared by the side's sectors: a crowded ring sector
                                              // may take more than its share), at least one full sector; scTickSetBorderCapacity raises it
constexpr uint32_t kOvfPerSector = 1024;      // overflow records one sector can hold besides its bin (what lies beyond is counted, never silent)
constexpr uint32_t kOvfWaves = 2048u * 4u;    // pair-role waves that can own an ovfIdx scratch row (the launcher's workgroup cap x 4)
constexpr uint32_t kBorderBigCap = 128;       // big boxes (wider than 2x2 sectors, outside the rectangle, bin full) per message
constexpr uint32_t kBorderBigWords = 2u + kBorderBigCap * 8u;
constexpr float kBigReach = 2.0f;             // sectors around a tile's owned region within which it must know a big box

constexpr uint32_t kBinCap = 64;          // one wave lane per record of a bin
// Pair output is sharded: a wave buffers its hits in LDS and appends them to the segment of its workgroup's
// shard with one atomic per flush; 64 counters on separate cache lines instead of one hot word.
constexpr uint32_t kPairShards = 64, kShardStride = 32, kWavePairBuf = 192;
constexpr uint32_t kPrimary = 0x80000000u;
// counters[]: 0 visible, 1 culled, 4 draws, 5 dropped, 6 renderables; per tick parity q: 8+8q+{0 pairs, 1 big, 2 bin-full}
constexpr uint32_t kCtrPar = 8, kCtrPairs = 0, kCtrBig = 1, kCtrBinFull = 2, kCtrBorderLost = 3, kCtrBigLocal = 4, kCtrSpill = 5;
constexpr uint32_t kCtrCrowdTail = 6, kCtrCrowdHead = 7;     // crowded sectors queued by the binning / taken by the pair search (reset with the parity's counters)
constexpr uint32_t kHomeOff = 0, kHomeLearn = 1, kHomeUse = 2;
constexpr uint32_t kNoHome = 0xFFFFFFFFu, kNoSlot = 0xFFu;
constexpr uint32_t kHomeHot = 0x80000000u;                         // homeCount: the bin was rebuilt since the learn tick, its owners write it again
constexpr uint32_t kCastFast = 0x100u;                            // homeCast: no two of the bin's reserved non-cast records pass the filter against each other
constexpr uint32_t kSlotMask = 0x3Fu, kSlotAlways = 0x40u;     // a homeB slot byte: slot in the bin, "written on every tick" (lazy records)
// Tick "parity": which copy of the per-tick broadphase state a tick works on.  The in-order flows alternate between two
// copies; pipelined tiles rotate through `depth` (2..kMaxParity) copies, so that the pair half of tick t may still run while
// the fused kernels of ticks t+1 .. t+depth-1 refill the others.
constexpr uint32_t kMaxParity = 4, kCounterWords = kCtrPar + 8u * (kMaxParity + 1u);
// (kCtrBig counts the big list: this tile's boxes, then -- after the border merge -- its neighbours' that reach it;
//  kCtrBigLocal keeps this tile's own count; kCtrBorderLost: records or boxes a border message had no room for, or
//  big boxes that reach beyond the eight neighbouring tiles -- pairs may be missing)

struct TickParams {
  uint32_t n;               // entities
  uint32_t span;            // entities per workgroup (multiple of kTile)
  uint32_t flags;           // SC_TICK_* | internal bits below
  uint32_t freeze;          // CullingState::freezeCulling
  uint32_t frustumValid;
  // broadphase grid: sectors [binOx, binOx+binSX) x [binOz, binOz+binSZ), keyed like worldToSector
  float binOx, binOz, invSector;
  uint32_t binSX, binSZ;
  uint32_t parity;          // tick parity: selects the counter set (and, through the context, the bins / lists)
  uint32_t maxPairs;
  uint32_t rankBits;        // rank << 24, OR-ed into every box id
  uint32_t neighbourMask;   // bit d set: a neighbour tile exists in direction d (its ring side is foreign)
  uint32_t chain;           // min(deepest hierarchy level, kMaxChain): selects the fused kernel's specialisation
  uint32_t resetParity;     // kFlagDeferredReset: the parity whose counters this tick's end-of-tick kernel clears (the next tick's)
  uint32_t tileX, tileZ, tilesX, tilesZ;   // this tile's place in the grid of equal tiles (tilesX == 0: unknown, no big-box exchange)
  uint32_t producerKind; float producerParam;   // with SC_TICK_PRODUCE_NEXT: the frame producer fused into the end-of-tick kernel
  float trafficSmooth, trafficMult;             // movers: 1 - exp(-2.5 dt) (smoothExp, sc_traffic_ai.cpp:58-62; host libm) and dbg->speedMultiplier
  uint32_t bigCap;          // entries the big list can hold (capacity + room for the neighbours' boxes): every index into it is held below this
  uint32_t ovfCap;          // entries the sector overflow list can hold
  uint32_t pairRun;         // pair role: a wave takes its sectors in runs of pairRun consecutive ones (pairRunFor())
  uint32_t cus;             // compute units of the device (launch geometry)
  uint32_t homeMode;        // bins: 0 every record reserves its slot (atomics), 1 the same and the slots are remembered (learn tick),
                            // 2 records with a remembered slot are stored there directly (kHome*)
  uint32_t homeReset;       // the pair search leaves binCount / binLayers at homeCount / homeLayers instead of zero
  uint32_t borderRecs;      // border messages: records per ring sector of a side, on average (scTickSetBorderCapacity; kBorderRecsPerBin)
  // draw emission folded into the end-of-tick kernel's compaction role (RenderPrepStreamingSystem, sc_world_partition.cpp:1306-1329): the
  // workgroup that places a visible entity in the ordered list knows its position there, i.e. the index of its draw item
  uint32_t emitMode;        // 0 off, 1 items to emitTarget (draw items), 2 the frame read-back block at emitTarget (header, visible head, items)
  uint32_t emitBudget;      // RenderPrepStreaming's draw budget (0 = none)
  uint32_t emitMaxVisible;  // mode 2: entries of the visible list the block holds
  uint32_t emitTickLo, emitTickHi;
  uint32_t* emitTarget;
  uint32_t cleanStay;       // kHomeUse ticks: an entity whose matrix was not rebuilt leaves its (always written) slots as they are -- they hold
                            // this very record; 0 after anything else changed boxes (bounds / matrix uploads) and when the pair half runs pipelined
  uint32_t lazy;            // kHomeUse ticks: reserved records of bins that cannot produce a pair may be left unwritten (DeviceState::lazyCtl):
                            // 1 = bins whose own records cannot meet each other, rebuilt on demand (in-order flows); 2 = bins whose records
                            // can meet nothing in the world's declared vocabulary, never needed (pipelined tiles, scTickSetWorldLayers);
                            // 0 when something else reads the bins (ray queries, traffic sensors) or neither applies
  uint32_t vocab;           // lazy 2: group bits | mask bits << 16 of every collider that can exist in the tiled world
  uint32_t halo;            // border messages carry the halo section (traffic sensors on a tiled world): the neighbours' core-edge records land in the ring bins
  uint32_t vocabKnown;      // scTickSetWorldLayers declared the world's layer vocabulary (`vocab`): the border merge counts arrivals outside it
  uint32_t sweepOnly;       // host hint (worldCanPair): no two layer words of this world admit a pair -- the pair role only sweeps the counters; sizes its grid, nothing else
  uint32_t fastPairs;       // the pair role takes bins that hold nothing but their ordered reserved records through the fast path (homeCast)
  uint32_t colliders;       // scTickUploadColliders was called (DeviceState::colType exists): the fused and level kernels run their collider instances
};
// What the wide compaction touches, and nothing else: the slim argument of the body where it runs on another tick's words than the
// launch's own (a copy of DeviceState and TickParams for the role cost the fused kernel SGPR spills).  flags: only SC_TICK_CULLED_LIST is read.
struct CompactView {
  const uint64_t *vis, *cand;
  const uint32_t *blockVis, *blockCand;
  uint32_t *visibleIdx, *culledIdx, *counters;
  uint32_t n, span, flags;
};
// The carried compaction: the pending tick's view, its workgroups (at the head of the fused launch's grid) and the spans each takes
struct CarryParams { CompactView view; uint32_t groups, group; };
// neighbour directions: d = (dz+1)*3 + (dx+1), skipping the centre -> 0..7; opposite(d) = 7 - d
__host__ __device__ inline void borderDir(uint32_t d, int& dx, int& dz) { const uint32_t k = d < 4 ? d : d + 1; dx = (int)(k % 3) - 1; dz = (int)(k / 3) - 1; }
// side messages span the whole ring side including its two end cells (used when no tile exists past them)
__host__ __device__ inline uint32_t borderLen(uint32_t d, uint32_t coreSX, uint32_t coreSZ) { int dx, dz; borderDir(d, dx, dz); return (dx != 0 && dz != 0) ? 1u : (dx == 0 ? coreSX + 2u : coreSZ + 2u); }
__host__ __device__ inline uint32_t borderDirOf(int dx, int dz) { const uint32_t k9 = (uint32_t)((dz + 1) * 3 + (dx + 1)); return k9 < 4 ? k9 : k9 - 1u; }
// hasNb(p, dx, dz): a tile exists one step in that direction
__host__ __device__ inline bool hasNb(const TickParams& p, int dx, int dz) { return (p.neighbourMask >> borderDirOf(dx, dz)) & 1u; }
// records one border message can carry: `recs` per ring sector of the side on average, at least one sector's bin and overflow list
constexpr uint32_t kSectorRecMax = 64u + kOvfPerSector;      // what one sector can hold at all: its bin + its share of the overflow list
__host__ __device__ inline uint32_t borderRecCap(uint32_t L, uint32_t recs) { return L * recs > kSectorRecMax ? L * recs : kSectorRecMax; }
// of a message's record capacity, every cell owns this many FIXED slots (the first records of a cell travel without a scan);
// the rest of the capacity is one spill-over area shared by the cells that hold more
constexpr uint32_t kBorderFixed = 4;
__host__ __device__ inline uint32_t borderFixedSlots(uint32_t L, uint32_t recs) { const uint32_t per = borderRecCap(L, recs) / L; return per < kBorderFixed ? per : kBorderFixed; }
__host__ __device__ inline uint32_t borderBinWords(uint32_t d, uint32_t coreSX, uint32_t coreSZ, uint32_t recs) { const uint32_t L = borderLen(d, coreSX, coreSZ); return kBorderHeader + L + borderRecCap(L, recs) * 8u; }
// The HALO section (round 4, traffic sensors on a tiled world): behind the big boxes, the records of the sender's CORE-EDGE sectors along that
// side -- what an obstacle ray cast from the receiver's edge needs to see in the neighbour's territory (sc_traffic_ai.cpp:300-345: the
// reference's ray sees the whole physics world).  Fixed slots: cell l owns kBinCap records at a fixed offset, so neither pack nor
// merge needs a prefix scan.  Layout: [L counts][L x kBinCap records of 8 words].  Present only when both tiles run with sensors.
__host__ __device__ inline uint32_t borderHaloWords(uint32_t d, uint32_t coreSX, uint32_t coreSZ) { const uint32_t L = borderLen(d, coreSX, coreSZ); return L + L * kBinCap * 8u; }
__host__ __device__ inline uint32_t borderWords(uint32_t d, uint32_t coreSX, uint32_t coreSZ, uint32_t recs, uint32_t halo = 0u)
{ return borderBinWords(d, coreSX, coreSZ, recs) + kBorderBigWords + (halo ? borderHaloWords(d, coreSX, coreSZ) : 0u); }
constexpr uint32_t kFlagHasDeep = 1u << 16;   // write recomp bits for the level kernels
constexpr uint32_t kFlagDeferredReset = 1u << 17;   // pipelined tiles: a pair kernel never clears the other parity's counters / big bits; a small kernel
                                                    // behind it on the pairs stream snapshots the results and clears its OWN parity
constexpr uint32_t kFlagDenseAabbs = 1u << 5; // == SC_TICK_DENSE_AABBS
constexpr uint32_t kFlagOverlaps = 1u << 19;    // SC_TICK_OVERLAPS as TickParams::flags carries it: the public flag is bit 16, kFlagHasDeep's position, and only
                                                // the low 16 public bits are copied into the word (fillParams) -- no kernel looks at this bit, the launch list does
constexpr uint32_t kFlagTriggers = 1u << 21;    // SC_TICK_TRIGGERS (public bit 17, kFlagDeferredReset's position) likewise: the launch list looks at it, no kernel does
constexpr uint32_t kFlagAnchoredSweeps = 1u << 22;      // SC_TICK_ANCHORED_SWEEPS (public bit 18, kFlagTailOwnsDirty's position) likewise
constexpr uint32_t kFlagTopoClasses = 1u << 20;    // every wave-tile of the world is classed and the classes are current: the fused kernel without binning takes
                                                    // its classed instance (no link word is read: xformCullClassed)
constexpr uint32_t kFlagTailOwnsDirty = 1u << 18;   // span-closed world: every workgroup of the fused kernel ends the tick for its own span (dirty clear, and the
                                                    // root nudge with SC_TICK_PRODUCE_NEXT: spanTail); the end-of-tick kernel then touches neither

// ---- renderer draw order (sc_tick_drawsort.hip) ----
constexpr uint32_t kSortThreads = 1024, kSortGroup = 8192;     // keys one workgroup orders per pass
constexpr uint64_t kDrawInvalid = 1ull << 55;                  // above every pipeline id (< 128): dropped draws sort last
constexpr uint32_t kNoMaterial = 0xFFu;                        // pipeline table entry of a material handle that does not exist
constexpr uint32_t kCtrDrawsSorted = 7;                        // counters[7]: draws that survived the renderer's handle checks
struct DrawSortState {
  uint64_t* key[2]; uint32_t* idx[2];     // ping-pong (key, rank in the visible list)
  uint32_t* hist;                         // [256][groups] digit totals for multi-workgroup passes
  const uint8_t* pipeline;                // Material::pipelineId per material handle, kNoMaterial = none
  uint32_t materialCount, meshCount;
  uint32_t passes; uint32_t shift[7];     // key bytes that can differ, least significant first
};
void launchSortedDraws(const DeviceState& d, const DrawSortState& st, uint32_t budget, uint32_t bound, void* items, hipStream_t s);

// ---- ray queries over the bins (sc_tick_queries.hip) ----
struct RayHit48 { uint32_t hit, id; float distance; float position[3]; float normal[3]; uint32_t layer; uint32_t pad; uint32_t pad2; };   // == ScTickRayHit
struct RayQueryState {
  const float4* origin;     // xyz + maxDist
  const float4* dir;        // xyz + mask (bit pattern)
  RayHit48* hits;
  uint32_t count;
};
// exact (scTickSetRayShapes, SC_TICK_RAY_SHAPES_EXACT): the instance that refines an AABB hit of an own typed collider by the shape itself --
// chosen here, on the host; the kernels' arguments are the same either way
void launchRayQueries(const DeviceState& d, const TickParams& p, const RayQueryState& q, bool exact, hipStream_t s);
// ---- capsule sweeps over the bins: a kernel argument of their own (DeviceState and TickParams keep their layout) ----
struct SweepHit48 { uint32_t hit, id; float distance; float position[3]; float normal[3]; uint32_t layer; float travel; uint32_t pad; };   // == ScTickSweepHit, laid out like RayHit48
static_assert(sizeof(SweepHit48) == sizeof(RayHit48), "sweep hits are read back like ray hits");
struct SweepQueryState {
  const float4* start;      // xyz + radius
  const float4* end;        // xyz + half height
  const uint2* filter;      // (mask, skip id)
  SweepHit48* hits;
  uint32_t count;
};
// exactInfo (scTickSetSweepShapes, SC_TICK_SWEEP_SHAPES_EXACT; nullptr: AABB mode): the instance that refines a grown-AABB hit of a refinable
// collider by the shape itself -- chosen here, on the host -- and the words of its report (== ScTickSweepShapeInfo), zeroed before the launch
constexpr float kSweepShapesTol = 1e-3f;        // == SC_TICK_SWEEP_SHAPES_TOL
constexpr int kSweepShapesSteps = 12;           // == SC_TICK_SWEEP_SHAPES_STEPS
constexpr uint32_t kSweepSeenCap = 256;         // == SC_TICK_SWEEP_SHAPES_SEEN: boxes one sweep counts once
constexpr uint32_t kSweepInfoWords = 4;
void launchSweepQueries(const DeviceState& d, const TickParams& p, const SweepQueryState& q, uint32_t* exactInfo, hipStream_t s);
// ---- overlap queries (include/sc_tick.h "overlap queries"): collider volumes without an entity, answered from this tick's records.  A kernel
// argument of their own, like the sweeps'.  Volume q is five 16-byte words: rows 0..2 of its world matrix (x, y, z, translation), its
// collider record (ex, ey, ez, radius) as DeviceState::colShape would hold it, and the bit patterns (type, mask, skip id, 0).
constexpr uint32_t kOverlapVolumeWords = 5;
struct OverlapQueryState {
  const float4* volume;     // [count][kOverlapVolumeWords]
  uint32_t* counts;         // [count] the true number of hits per volume
  uint32_t* ids;            // [count][maxHits]: the first min(counts[q], maxHits) slots of row q hold distinct ids of its hits
  uint2* tally;             // [count] EXACT mode: (candidates decided by a shape routine, hits left on their box answer) per volume.  The report's
                            // sums are the READER's (scTickReadOverlapHits): one word all 4 096 waves add to takes ~88 additions per microsecond
  uint32_t count, maxHits;
};
// exact (SC_TICK_OVERLAP_SHAPES_EXACT): the instance that asks the touching pairs' routines about a refinable candidate -- chosen on the host
void launchOverlapQueries(const DeviceState& d, const TickParams& p, const OverlapQueryState& q, bool exact, hipStream_t s);
// ---- trigger volumes (include/sc_tick.h "trigger volumes"): overlap volumes given in an entity's local frame, resolved against this tick's
// world matrix of that entity by the kernel that answers them, which also forms the difference against the row it remembers.  A kernel
// argument of their own.  Volume v is kOverlapVolumeWords 16-byte words like an overlap query's -- rows 0..2 of its LOCAL matrix, its
// collider record, (type, mask, 0, 0) -- plus its (anchor, skip_self) word.  ONE id row per volume in device memory: it is the member row
// the readers see and the remembered row the next flagged tick diffs against; remembered[v] says how many of its slots are remembered.
constexpr uint32_t kTriggerRowCap = 1024;        // == SC_TICK_TRIGGER_MAX_MEMBERS: two rows of 4 KB per wave in LDS while diffing
constexpr uint32_t kTriggerNone = 0xFFFFFFFFu;   // remembered[v]: nothing is remembered for the volume (the next flagged tick resyncs it)
constexpr uint32_t kTriggerResync = 1u, kTriggerOverflow = 2u;      // stat[v].z bits
struct TriggerState {
  const float4* local;      // [count][kOverlapVolumeWords]
  const uint2* anchor;      // [count] (dense index | kAnchorNone | kAnchorDead, skip_self)
  float4* world;            // [count][3] the resolved rows of the last flagged run (NaN rows: a volume without members by the resolve)
  uint32_t* counts;         // [count] the true number of members per volume
  uint32_t* ids;            // [count][maxMembers] the member row = the remembered row
  uint32_t* remembered;     // [count] slots of the row that are remembered, or kTriggerNone.  Reset by the HOST, outside any captured graph
  uint4* stat;              // [count] (entered, exited, kTrigger* bits, 0) per volume: the report's sums are the reader's
  uint32_t* ctl;            // [2] event slots reserved this tick (entered, exited): one atomic per list per wave that has events
  uint2* entered; uint2* exited;     // [maxEvents] each: (volume, id)
  uint32_t count, maxMembers, maxEvents;
};
void launchTriggerVolumes(const DeviceState& d, const TickParams& p, const TriggerState& t, bool exact, hipStream_t s);
// ---- entity-anchored rays (include/sc_tick.h "entity-anchored rays"): given in an entity's local frame, resolved against this tick's
// world matrix of that entity by the kernel that casts them.  A kernel argument of their own, like the sweeps'. ----
constexpr uint32_t kAnchorNone = 0xFFFFFFFFu;    // == SC_TICK_ANCHOR_NONE: origin and direction are world space
constexpr uint32_t kAnchorDead = 0xFFFFFFFEu;    // == SC_TICK_ANCHOR_DEAD: the anchor was removed (beyond every entity count: a miss)
struct AnchoredRayState {
  const float4* origin;     // local xyz + maxDist (world metres)
  const float4* dir;        // local xyz + mask (bit pattern)
  const uint2* anchor;      // (dense index of the anchor | kAnchorNone | kAnchorDead, skip_self)
  RayHit48* hits;
  // split flows: the tick half resolves into a snapshot -- world-space (origin, maxDist), (direction, mask), skip id -- of the tick's
  // parity, the pair half casts from it (the next tick's fused kernel may have rewritten the matrices by then)
  float4* snapOrigin; float4* snapDir; uint32_t* snapSkip;
  uint32_t count;
};
void launchAnchoredRays(const DeviceState& d, const TickParams& p, const AnchoredRayState& q, bool fromSnapshot, bool exact, hipStream_t s);   // resolve + cast; fromSnapshot (pair half): cast
void launchAnchoredRaySnapshot(const DeviceState& d, const TickParams& p, const AnchoredRayState& q, hipStream_t s);      // tick half: resolve
// ---- entity-anchored capsule sweeps (include/sc_tick.h "entity-anchored capsule sweeps"): given in an entity's local frame, resolved
// against this tick's world matrix of that entity by the kernel that sweeps them.  A kernel argument of their own. ----
constexpr uint32_t kASweepAnswered = 0, kASweepNoAnchor = 1, kASweepNotFinite = 2;      // == SC_TICK_ASWEEP_*: SweepHit48::pad
struct AnchoredSweepState {
  const float4* start;      // local xyz + radius (world metres)
  const float4* end;        // local xyz -- a point of the anchor's frame, or a world-space displacement (end_frame) -- + half height
  const uint4* anchor;      // (dense index of the anchor | kAnchorNone | kAnchorDead, skip_self, end_frame, mask)
  SweepHit48* hits;
  float4* segment;          // [count][2] the resolved (start, end) of the last flagged run; quiet NaNs where the status is not 0
  uint32_t count;
};
// exactInfo: as for launchSweepQueries, words of their own (== ScTickSweepShapeInfo, scTickGetAnchoredSweepShapeInfo)
void launchAnchoredSweeps(const DeviceState& d, const TickParams& p, const AnchoredSweepState& q, uint32_t* exactInfo, hipStream_t s);
// ---- pair begin / end events (sc_tick_pair_events.hip; include/sc_tick.h "pair events"): the difference between this tick's pair set and
// the set of the last tick that ran with SC_TICK_PAIR_EVENTS, formed on the device behind the pair search.  A kernel argument of its own.
// Two open-addressing tables of 64-bit keys a << 32 | b (0 = empty: a < b rules it out) are used in turn: the one holding the remembered
// set ("previous") is probed, marked and -- by the sweep -- emptied, the other ("current") is filled and becomes the remembered set.
struct PairEventState {
  unsigned long long* table[2];   // [slots] each
  uint32_t* marks[2];             // [slots / 32] each: bit = "this slot's pair is in this tick's set too"
  uint32_t* ctl;                  // kPe* words below; tables, marks and ctl are ONE allocation: zero bytes all over = nothing remembered
  uint32_t* info;                 // what the last flagged tick reports (== ScTickPairEventInfo)
  uint2* begun; uint2* ended;     // [maxEvents] each
  uint32_t slots;                 // power of two >= 2 * maxTracked (and >= 64)
  uint32_t maxTracked, maxEvents;
};
// ctl words: which table is filled this tick; 1 = the other one holds a remembered set (0: the next flagged tick is a resync tick);
// the tick's running counts; != 0: this tick's set does not fit (or a probe ran out of slots)
constexpr uint32_t kPeCur = 0, kPeValid = 1, kPeBegun = 2, kPeEnded = 3, kPeTracked = 4, kPeOverflow = 5, kPeCtlWords = 16;
constexpr uint32_t kPeInfoWords = 8;
void launchPairEvents(const DeviceState& d, const TickParams& p, const PairEventState& e, hipStream_t s);
// the sweep and the finish alone, for a state whose current table another kernel filled (touch events: the narrow-phase pass)
void launchPairEventsTail(const PairEventState& e, hipStream_t s);
#ifdef __HIPCC__
__device__ __forceinline__ uint32_t pairHash(unsigned long long k)
{
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;   // (MurmurHash3's 64-bit finaliser)
  return (uint32_t)k;
}
// One pair (key = a << 32 | b, never 0) of this tick's set: it enters the CURRENT table -- `inserted`: by this lane; a pair met twice enters
// once -- and a pair that entered is looked up in the PREVIOUS table: `found` and its slot marked, or not found: the pair has begun.
// Both probe loops are bounded by the slot count; one that runs out raises the overflow word, it never spins.
__device__ __forceinline__ void pairSetEnter(const PairEventState& e, unsigned long long* curT, const unsigned long long* prevT, uint32_t* prevM,
                                             uint32_t mask, unsigned long long key, bool& inserted, bool& found)
{
  const uint32_t home = pairHash(key) & mask;
  uint32_t pos = home;
  bool placed = false;
  for (uint32_t n = 0; n < e.slots; ++n) {
    // (a slot only ever goes from empty to a key inside the entering kernel; the load is served past the L1, and a slot read as empty is
    //  taken with a compare-and-swap, which answers with what is really there)
    unsigned long long v = __hip_atomic_load(&curT[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == 0ull) {
      v = atomicCAS(&curT[pos], 0ull, key);
      if (v == 0ull) { inserted = true; placed = true; break; }
    }
    if (v == key) { placed = true; break; }             // the pair list named it twice: it is in the set once
    pos = (pos + 1u) & mask;
  }
  if (!placed) atomicOr(&e.ctl[kPeOverflow], 1u);       // every slot taken by other keys: cannot happen while the set fits
  if (inserted) {
    pos = home;
    for (uint32_t n = 0; n < e.slots; ++n) {
      const unsigned long long v = prevT[pos];
      if (v == key) { atomicOr(&prevM[pos >> 5], 1u << (pos & 31u)); found = true; break; }
      if (v == 0ull) break;
      pos = (pos + 1u) & mask;
    }
  }
}
#endif
// ---- touching pairs (sc_tick_pair_shapes.hip; include/sc_tick.h "touching pairs"): the pairs of this tick's list whose collider shapes
// overlap, decided on the device behind the pair search from the resident collider records and this tick's matrix rows.  A kernel
// argument of its own; the pass owns no per-entity state.
struct PairShapeState {
  uint2* list;                    // [maxTouching] (a, b) as the pair list holds them
  uint32_t* ctl;                  // kPs* words below: the tick's running counts
  uint32_t* info;                 // what the last flagged tick reports (== ScTickPairShapeInfo)
  uint32_t maxTouching;
};
constexpr uint32_t kPsTouching = 0, kPsRefined = 1, kPsKept = 2, kPsTested = 3, kPsPairsTruncated = 4, kPsCtlWords = 8;
constexpr uint32_t kPsInfoWords = 8;
constexpr float kPairShapesSatEps = 1e-6f;      // == SC_TICK_PAIR_SHAPES_SAT_EPS
// ---- pair contacts (k_pair_contacts, sc_tick_pair_shapes.hip; include/sc_tick.h "pair contacts"): one record per entry of the touching
// list -- point, depth, normal, kind -- written behind the narrow-phase pass while the list's running count is still up.  All null
// until scTickSetPairContacts: nothing is launched.
struct PairContactState {
  float4* rec;                    // [2 * maxTouching]: record i = (point, depth), (normal, kind) of list entry i (== ScTickPairContact)
  uint32_t* ctl;                  // kPc* words below: the tick's running kind counts
  uint32_t* info;                 // what the last tick with contacts reports (== ScTickPairContactInfo)
  uint32_t maxTouching;           // the touching list's
};
constexpr uint32_t kPcRoundRound = 0, kPcRoundBox = 1, kPcBoxBox = 2, kPcUnrefined = 3, kPcDeep = 4, kPcDegenerate = 5, kPcCtlWords = 8;
constexpr uint32_t kPcInfoWords = 8;
constexpr uint32_t kContactNone = 0, kContactRoundRound = 1, kContactRoundBox = 2, kContactBoxFaceA = 3, kContactBoxFaceB = 4, kContactBoxEdge = 5,
                   kContactDeep = 1u << 8, kContactDegenerate = 1u << 9;      // == SC_TICK_CONTACT_*
constexpr float kPairContactsEdgeEps = 1e-4f;   // == SC_TICK_PAIR_CONTACTS_EDGE_EPS
// ---- pair manifolds (k_pair_manifolds, sc_tick_pair_manifolds.hip; include/sc_tick.h "pair manifolds"): up to four points per entry of the
// touching list, written behind the contact records while the list's running count is still up.  All null until scTickSetPairManifolds:
// nothing is launched.
struct PairManifoldState {
  float4* rec;                    // [5 * maxTouching]: record i = five float4 of list entry i (== ScTickPairManifold)
  uint32_t* ctl;                  // kPm* words below: the tick's running counts
  uint32_t* info;                 // what the last tick with manifolds reports (== ScTickPairManifoldInfo)
  uint32_t maxTouching;           // the touching list's
};
constexpr uint32_t kPmOne = 0, kPmTwo = 1, kPmThree = 2, kPmFour = 3, kPmFace = 4, kPmReduced = 5, kPmCtlWords = 8;
constexpr uint32_t kPmInfoWords = 8;
constexpr uint32_t kManifoldNone = 0, kManifoldSingle = 1, kManifoldSegment = 2, kManifoldFace = 3, kManifoldReduced = 1u << 8;      // == SC_TICK_MANIFOLD_*
constexpr float kManifoldSkin = 2.5e-4f, kManifoldFlat = 1e-3f;      // == SC_TICK_MANIFOLD_SKIN, SC_TICK_MANIFOLD_FLAT
constexpr uint32_t kManifoldWave = 64;          // threads per workgroup of k_pair_manifolds: one wave, its clip polygons in LDS
// ---- pair islands (sc_tick_pair_islands.hip; include/sc_tick.h "pair islands"): the connected components of the movable entities under
// the linking entries of the touching list, by a lock-free union-find between the narrow-phase pass and the list's report.  All null
// until scTickSetPairIslands: nothing is launched.
struct PairIslandState {
  uint32_t* edge;                 // [maxTouching]: the island of list entry i
  uint32_t* ctl;                  // word kPiGaveUp alone
  uint32_t* info;                 // what the last tick with islands reports (== ScTickPairIslandInfo)
  uint32_t maxTouching;           // the touching list's
  uint32_t* partial;              // [kPiMaxBlocks][4]: the tallies kPiLinking .. kPiMovable of every workgroup, rewritten by every launch, summed by the report
  uint32_t* parent;               // [cap] the union-find: a dense index <= the entity's own, or kIslandNone for a fixed entity
  uint32_t* labels;               // [cap] what scTickReadPairIslands returns; between init and flatten: != 0 = a hook landed on this root
  uint32_t cap;                   // the context's padded capacity
  uint32_t fixedGroups;           // the caller's: a group bit in it makes an entity fixed
};
constexpr uint32_t kPiLinking = 0, kPiIslands = 1, kPiBodies = 2, kPiMovable = 3, kPiGaveUp = 4, kPiCtlWords = 8;
constexpr uint32_t kPiMaxBlocks = 2048;         // workgroups per launch of the pass at most (grid-stride beyond)
constexpr uint32_t kPiInfoWords = 8;
constexpr uint32_t kIslandNone = 0xFFFFFFFFu;   // == SC_TICK_ISLAND_NONE
// ---- pair persistence (sc_tick_pair_persist.hip; include/sc_tick.h "pair persistence"): every entry of the touching list matched to the
// entry of the same pair in the last flagged run, its manifold points matched to that entry's points in `a`'s frame, an age and a
// 16-byte payload per point carried across the match.  Two sides, used in turn like the pair events' tables: the one the last flagged run
// filled ("remembered") is probed and -- by the sweep -- emptied, the other ("current") is filled.  All null until
// scTickSetPairPersistence: nothing is launched.
struct PairPersistState {
  uint4* rec;                     // [maxTouching]: record i of list entry i (== ScTickPairPersist)
  uint32_t* ctl;                  // kPp* words below, and behind them in the same allocation (`slabBytes` in all) the tables of both sides:
                                  // zero bytes all over = nothing remembered
  uint32_t* info;                 // [kPpInfoWords]: what the last flagged run reports (== ScTickPairPersistInfo), then the side it filled
  uint32_t maxTouching;           // the touching list's
  unsigned long long* key[2];     // [slots] each: a << 32 | b of a listed pair, 0 = empty
  uint32_t* val[2];               // [slots] each: ~(the smallest entry index that names the slot's pair), kept by an atomic maximum; 0 = none
  float4* local[2];               // [4 * maxTouching] each: entry i's four local points (twelve floats), then (ages, count, 0, 0)
  float4* payload[2];             // [4 * maxTouching] each: entry i's four payload rows
  uint32_t* partial;              // [kPpMaxBlocks][4]: every workgroup's tallies, rewritten by every launch, summed by the finish
  uint32_t slots;                 // power of two >= 2 * maxTouching (and >= 64)
  float matchDist;                // the caller's
  size_t slabBytes;
};
constexpr uint32_t kPpCur = 0, kPpValid = 1, kPpGaveUp = 2, kPpCtlWords = 16;
constexpr uint32_t kPpKeptPairs = 0, kPpKeptPoints = 1, kPpNewPoints = 2;      // a workgroup's tallies (the fourth word is not used)
constexpr uint32_t kPpMaxBlocks = 1024;         // workgroups of k_pair_persist_match at most (grid-stride beyond)
constexpr uint32_t kPpInfoWords = 16, kPpInfoSide = 8;
constexpr uint32_t kPersistNone = 0xFFFFFFFFu;  // == SC_TICK_PERSIST_NONE
// ---- pair sleep (sc_tick_pair_sleep.hip; include/sc_tick.h "pair sleep"): which islands are at rest, which bodies fell asleep, which were
// woken.  Per entity of capacity an anchor pose (three float4), a state word and an `awake` word (indexed by the island's root); two event
// lists.  One slab: zero bytes all over = nothing remembered, the next flagged run is a resync.  All null until scTickSetPairSleep:
// nothing is launched.
struct PairSleepState {
  uint32_t* ctl;                  // kPz* words below, and behind them in the same allocation (`slabBytes` in all) state, awake and anchor
  uint32_t* info;                 // [kPzInfoWords]: what the last flagged run reports (== ScTickPairSleepInfo)
  uint32_t maxTouching;           // the touching list's (a re-sized list is a resync)
  uint32_t* state;                // [cap]: rest | ASLEEP << 8 | STILL << 9 | MOVABLE << 10 as of the last flagged run
  uint32_t* awake;                // [cap]: word r == the run's epoch = the island with root r is awake in this run
  float4* anchor;                 // [3 * cap]: rows 0..2 of entity e at 3 * e; a NaN row = unset
  uint32_t* fell;                 // [maxEvents] ids that fell asleep in the last flagged run
  uint32_t* woke;                 // [maxEvents] ids that woke
  uint32_t* partial;              // [kPzMaxBlocks][4]: every workgroup's tallies of the resolve, rewritten by every launch, summed by the finish
  uint32_t cap;                   // the context's padded capacity
  uint32_t maxEvents;
  uint32_t restRuns;              // 1 .. 255
  float linTol, angTol;
  size_t slabBytes;
};
constexpr uint32_t kPzEpoch = 0, kPzValid = 1, kPzFell = 2, kPzWoke = 3, kPzCtlWords = 16;
constexpr uint32_t kPzAsleep = 0, kPzIslandsAsleep = 1, kPzAwakeEntries = 2;      // a workgroup's tallies (the fourth word is not used)
constexpr uint32_t kPzMaxBlocks = 2048;         // workgroups per launch of the pass at most (grid-stride beyond)
constexpr uint32_t kPzInfoWords = 8;
constexpr uint32_t kSleepAsleep = 1u << 8, kSleepStill = 1u << 9, kSleepMovable = 1u << 10;      // == SC_TICK_SLEEP_ASLEEP / _STILL / _MOVABLE
constexpr uint32_t kSleepResync = 1u, kSleepFellOverflow = 2u, kSleepWokeOverflow = 4u, kSleepListTruncated = 8u;      // == SC_TICK_SLEEP_INFO_*
// The shapes as the touching pairs take them (include/sc_tick.h "touching pairs"), shared with the exact shapes for capsule sweeps
// (sc_tick_queries.hip): a member through its matrix, the round and the box frame built from it, and the two distance cores.  All of it
// fp32, unfused, left to right, as the header states it operation by operation.
#ifdef __HIPCC__
__device__ __forceinline__ float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ float clamp01(float x) { const float c = (x > 0.0f) ? x : 0.0f; return (c < 1.0f) ? c : 1.0f; }   // (a NaN is 0)

// a member of a pair as the routines take it: columns c[k], translation T, n[k] = dot(c[k], c[k]), the record (ex, ey, ez, radius)
struct Member { float c[3][3]; float T[3]; float n[3]; float4 s; uint32_t type; bool ok; };

// ok = the member can be refined: an own entity below the count with a typed collider and three finite, positive column norms
__device__ __forceinline__ Member fetchMember(const DeviceState& d, uint32_t id, uint32_t count, uint32_t rankBits)
{
  Member m;
  m.ok = false; m.type = kColliderBounds; m.s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int k = 0; k < 3; ++k) { m.c[k][0] = m.c[k][1] = m.c[k][2] = 0.0f; m.T[k] = 0.0f; m.n[k] = 0.0f; }
  const uint32_t e = id & 0x00FFFFFFu;
  if (!d.colType || (id & 0xFF000000u) != rankBits || e >= count) return m;
  m.type = d.colType[e];
  if (m.type != kColliderBox && m.type != kColliderSphere && m.type != kColliderCapsule) return m;
  m.s = d.colShape[e];
  const float4 r0 = d.w0[e], r1 = d.w1[e], r2 = d.w2[e];
  m.c[0][0] = r0.x; m.c[0][1] = r1.x; m.c[0][2] = r2.x;
  m.c[1][0] = r0.y; m.c[1][1] = r1.y; m.c[1][2] = r2.y;
  m.c[2][0] = r0.z; m.c[2][1] = r1.z; m.c[2][2] = r2.z;
  m.T[0] = r0.w; m.T[1] = r1.w; m.T[2] = r2.w;
#pragma unroll
  for (int k = 0; k < 3; ++k) m.n[k] = dot3(m.c[k], m.c[k]);
  m.ok = m.n[0] > 0.0f && m.n[1] > 0.0f && m.n[2] > 0.0f && isfinite(m.n[0]) && isfinite(m.n[1]) && isfinite(m.n[2]);
  return m;
}

// a sphere or a capsule: the segment T - A .. T + A (A = 0: a point) and the radius around it
struct Round { float A[3]; float R; };
__device__ __forceinline__ Round roundOf(const Member& m)
{
  Round r;
  if (m.type == kColliderSphere) {
    const float nyz = (m.n[2] < m.n[1]) ? m.n[1] : m.n[2];
    r.R = m.s.w * sqrtf((m.n[0] < nyz) ? nyz : m.n[0]);
    r.A[0] = r.A[1] = r.A[2] = 0.0f;
  } else {
    r.R = m.s.w * sqrtf((m.n[0] < m.n[2]) ? m.n[2] : m.n[0]);
#pragma unroll
    for (int i = 0; i < 3; ++i) r.A[i] = m.c[1][i] * m.s.y;
    if (!(dot3(r.A, r.A) > 0.0f)) r.A[0] = r.A[1] = r.A[2] = 0.0f;      // no axis: the sphere of radius R
  }
  return r;
}

// a box in its own orthonormal frame: unit axes u[k], half lengths H[k]
struct Frame { float u[3][3]; float H[3]; };
__device__ __forceinline__ Frame frameOf(const Member& m)
{
  Frame f;
  const float e[3] = { m.s.x, m.s.y, m.s.z };
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float q = sqrtf(m.n[k]);
#pragma unroll
    for (int i = 0; i < 3; ++i) f.u[k][i] = m.c[k][i] / q;
    f.H[k] = e[k] * q;
  }
  return f;
}

__device__ __forceinline__ float boxDist2(const float y0[3], const float dy[3], const float H[3], float t)
{
  float g[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { const float x = fabsf(y0[k] + dy[k] * t) - H[k]; g[k] = (x > 0.0f) ? x : 0.0f; }
  return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

// The segment-segment core: the closest points of p1 + d1*[0, 1] and p2 + d2*[0, 1] by the clamped closed form -- their parameters s
// and t, their difference v (first minus second) and its squared length
struct SegSeg { float s, t, dist2; float v[3]; };
__device__ __forceinline__ SegSeg segSegCore(const float p1[3], const float d1[3], const float p2[3], const float d2[3])
{
  float r[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) r[i] = p1[i] - p2[i];
  const float a = dot3(d1, d1), e = dot3(d2, d2), f = dot3(d2, r);
  float s = 0.0f, t = 0.0f;
  if (!(a > 0.0f)) { if (e > 0.0f) t = clamp01(f / e); }
  else {
    const float c = dot3(d1, r);
    if (!(e > 0.0f)) s = clamp01((-c) / a);
    else {
      const float b = dot3(d1, d2);
      const float den = a * e - b * b;
      if (den > 0.0f) s = clamp01((b * f - c * e) / den);
      t = (b * s + f) / e;
      if (t < 0.0f) { t = 0.0f; s = clamp01((-c) / a); }
      else if (t > 1.0f) { t = 1.0f; s = clamp01((b - c) / a); }
    }
  }
  SegSeg o; o.s = s; o.t = t;
#pragma unroll
  for (int i = 0; i < 3; ++i) o.v[i] = (p1[i] + d1[i] * s) - (p2[i] + d2[i] * t);
  o.dist2 = dot3(o.v, o.v);
  return o;
}

// The segment-box core: the segment y0 + dy*[0, 1] in the box's frame.  F(t), the squared distance of its point t from the box, is convex
// and piecewise quadratic with breakpoints where a coordinate crosses a face plane -- its minimum is F at a breakpoint, at an end, or at the
// stationary point of one of the seven intervals between them: fifteen evaluations, the first strictly smaller one in their order keeps
// its parameter.  segment false: a point (every dy is 0 and every F would be F(0) again) -- one evaluation.
struct SegBox { float fmin, at; };
__device__ __forceinline__ SegBox segBoxCore(const float y0[3], const float dy[3], const float H[3], bool segment)
{
  SegBox o;
  o.fmin = boxDist2(y0, dy, H, 0.0f); o.at = 0.0f;
  if (segment) {
    float x = boxDist2(y0, dy, H, 1.0f);
    if (x < o.fmin) { o.fmin = x; o.at = 1.0f; }
    float b[8];
    b[0] = 0.0f; b[7] = 1.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      b[1 + 2 * k] = clamp01((H[k] - y0[k]) / dy[k]);
      b[2 + 2 * k] = clamp01(((-H[k]) - y0[k]) / dy[k]);
    }
    // b[1..6] in ascending order: a fixed network of twelve compare-exchanges
#define SC_CX(i, j) { const float lo = (b[j] < b[i]) ? b[j] : b[i], hi = (b[j] < b[i]) ? b[i] : b[j]; b[i] = lo; b[j] = hi; }
    SC_CX(1, 6) SC_CX(2, 4) SC_CX(3, 5) SC_CX(2, 3) SC_CX(4, 5) SC_CX(1, 4) SC_CX(3, 6) SC_CX(1, 2) SC_CX(3, 4) SC_CX(5, 6) SC_CX(2, 3) SC_CX(4, 5)
#undef SC_CX
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const float lo = b[i], hi = b[i + 1];
      const float tm = (lo + hi) * 0.5f;
      float num[3], den[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float y = y0[k] + dy[k] * tm;
        const bool out = fabsf(y) - H[k] > 0.0f;
        const float face = (y > 0.0f) ? H[k] : -H[k];
        num[k] = out ? (y0[k] - face) * dy[k] : 0.0f;
        den[k] = out ? dy[k] * dy[k] : 0.0f;
      }
      const float ns = (num[0] + num[1]) + num[2], ds = (den[0] + den[1]) + den[2];
      float ts = (ds > 0.0f) ? (-ns) / ds : lo;
      ts = (ts < lo) ? lo : ts;
      ts = (ts > hi) ? hi : ts;
      x = boxDist2(y0, dy, H, ts);
      if (x < o.fmin) { o.fmin = x; o.at = ts; }
      if (i < 6) { x = boxDist2(y0, dy, H, hi); if (x < o.fmin) { o.fmin = x; o.at = hi; } }
    }
  }
  return o;
}

// The three routines of the touching pairs (include/sc_tick.h "touching pairs"), shared with the overlap queries (sc_tick_queries.hip):
// true = the two shapes are provably apart.  A positive comparison alone says so: a NaN keeps the pair.
// 1. round - round: the squared distance between two segments by the clamped closed form; apart when it exceeds (Ra + Rb)^2
__device__ __forceinline__ bool roundRoundApart(const Member& ma, const Member& mb)
{
  const Round ra = roundOf(ma), rb = roundOf(mb);
  float p1[3], d1[3], p2[3], d2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    p1[i] = ma.T[i] - ra.A[i]; d1[i] = ra.A[i] + ra.A[i];
    p2[i] = mb.T[i] - rb.A[i]; d2[i] = rb.A[i] + rb.A[i];
  }
  const SegSeg c = segSegCore(p1, d1, p2, d2);
  const float sum = ra.R + rb.R;
  return c.dist2 > sum * sum;
}

// 2. round - box: the segment in the box's frame; apart when the minimum of F (segBoxCore) exceeds R^2
__device__ __forceinline__ bool roundBoxApart(const Member& mr, const Member& mx)
{
  const Round rd = roundOf(mr);
  const Frame fr = frameOf(mx);
  float w[3], y0[3], dy[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = mr.T[i] - mx.T[i];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float yc = dot3(fr.u[k], w), ya = dot3(fr.u[k], rd.A);
    y0[k] = yc - ya; dy[k] = ya + ya;
  }
  const SegBox c = segBoxCore(y0, dy, fr.H, rd.A[0] != 0.0f || rd.A[1] != 0.0f || rd.A[2] != 0.0f);
  return c.fmin > rd.R * rd.R;
}

// 3. box - box: the 15-axis separating-axis test in A's frame; apart when some axis has |t . L| > ra + rb
__device__ __forceinline__ bool boxBoxApart(const Member& ma, const Member& mb)
{
  const Frame fa = frameOf(ma), fb = frameOf(mb);
  float Rm[3][3], Ab[3][3], w[3], t[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = mb.T[i] - ma.T[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t[i] = dot3(w, fa.u[i]);
#pragma unroll
    for (int j = 0; j < 3; ++j) { Rm[i][j] = dot3(fa.u[i], fb.u[j]); Ab[i][j] = fabsf(Rm[i][j]) + kPairShapesSatEps; }
  }
  bool apart = false;
#pragma unroll
  for (int i = 0; i < 3; ++i) {                            // L = A's axis i
    const float rb = (fb.H[0] * Ab[i][0] + fb.H[1] * Ab[i][1]) + fb.H[2] * Ab[i][2];
    apart = apart || (fabsf(t[i]) > fa.H[i] + rb);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {                            // L = B's axis j
    const float ra = (fa.H[0] * Ab[0][j] + fa.H[1] * Ab[1][j]) + fa.H[2] * Ab[2][j];
    const float tl = (t[0] * Rm[0][j] + t[1] * Rm[1][j]) + t[2] * Rm[2][j];
    apart = apart || (fabsf(tl) > ra + fb.H[j]);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {                            // L = A's axis i x B's axis j
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      const float ra = fa.H[i1] * Ab[i2][j] + fa.H[i2] * Ab[i1][j];
      const float rb = fb.H[j1] * Ab[i][j2] + fb.H[j2] * Ab[i][j1];
      const float tl = t[i2] * Rm[i1][j] - t[i1] * Rm[i2][j];
      apart = apart || (fabsf(tl) > ra + rb);
    }
  }
  return apart;
}
#endif
// ---- touch events (include/sc_tick.h "touch events"): the pair events' difference taken over the TOUCHING set.  A second PairEventState;
// the narrow-phase kernel enters what it decides "not apart" into that state's current table (its <.., Events> instances), the pair
// events' sweep and finish do the rest.
// The narrow phase's states in one host-side struct (ScTickContext owns it; the device-argument structs inside keep their layout), and
// the stages one run of it executes as a bit set.  planTick is the set's only writer and applies the dependency rules there: contacts
// and islands need the list, manifolds the contacts, persistence the manifolds, sleep the islands.
struct NarrowPhase {
  PairEventState touch;           // scTickSetTouchEvents
  PairShapeState list; PairContactState contacts; PairManifoldState manifolds; PairIslandState islands; PairPersistState persist; PairSleepState sleep;
};
enum NarrowStage : uint32_t { kStageList = 1, kStageTouch = 2, kStageContacts = 4, kStageManifolds = 8, kStageIslands = 16, kStagePersist = 32, kStageSleep = 64 };
// One narrow-phase launch per tick for the list (SC_TICK_PAIR_SHAPES) and / or the touch state (SC_TICK_TOUCH_EVENTS), then the stages of
// `stages` in this order, all ahead of the list's report: contacts and their report, manifolds, persistence, islands, sleep.  It goes by
// `stages` alone: a stage named there is enabled and has what it needs (planTick).
void launchPairShapes(const DeviceState& d, const TickParams& p, const NarrowPhase& np, uint32_t stages, hipStream_t s);
// the sleep pass and its report (sc_tick_pair_sleep.hip), launched by launchPairShapes behind launchPairIslands; launchPairSleepWake is
// scTickWakeEntities' one launch over `n` dense indices on the device
void launchPairSleep(const DeviceState& d, const TickParams& p, const PairShapeState& list, const PairIslandState& islands, const PairSleepState& sleep,
                     hipStream_t s);
void launchPairSleepWake(const PairSleepState& sleep, const uint32_t* ids, uint32_t n, hipStream_t s);
// the persistence pass, its sweep and its report (sc_tick_pair_persist.hip), launched by launchPairShapes behind launchPairManifolds
void launchPairPersist(const DeviceState& d, const TickParams& p, const PairShapeState& list, const PairManifoldState& manifolds, const PairPersistState& persist,
                       hipStream_t s);
// the island pass and its report (sc_tick_pair_islands.hip), launched by launchPairShapes between the narrow-phase pass and the list's report
void launchPairIslands(const DeviceState& d, const TickParams& p, const PairShapeState& list, const PairIslandState& islands, hipStream_t s);
// k_pair_manifolds and its report (sc_tick_pair_manifolds.hip), launched by launchPairShapes between the contacts' report and the list's
void launchPairManifolds(const DeviceState& d, const TickParams& p, const PairShapeState& list, const PairManifoldState& manifolds, hipStream_t s);
// ---- bind runs of the sorted draw list and the material touch set (sc_tick_bindruns.hip; include/sc_tick.h "bind runs") ----
struct BindRun24 { uint32_t first, count, pipeline, material, mesh, binds; };      // == ScTickBindRun
// the report's words (== ScTickBindInfo)
constexpr uint32_t kBiRuns = 0, kBiTruncated = 1, kBiDraws = 2, kBiPipelineBinds = 3, kBiMaterialBinds = 4, kBiMeshBinds = 5, kBiMaterialsTouched = 6,
                   kBiTouchWords = 7, kBiWords = 8;
struct BindRunState {
  BindRun24* runs;          // [maxRuns + 1]: the row behind the last reported one is kept for that one's count
  uint32_t* info;           // [kBiWords], and behind it in the same allocation ...
  uint32_t* touch;          // ... [touchWords]: bit h % 32 of word h / 32 = material handle h was touched
  uint32_t maxRuns, touchWords, materialCount;
};
void launchBindRuns(const DeviceState& d, const DrawSortState& st, const BindRunState& b, uint32_t bound, hipStream_t s);
// frame read-back: [kBiWords report][maxRuns rows of 6 words][touchWords] into `block`
void launchStageBinds(const BindRunState& b, uint32_t* block, hipStream_t s);
void launchAgentFrontRays(const DeviceState& d, const TickParams& p, hipStream_t s);
void launchAgentRaySnapshot(const DeviceState& d, const TickParams& p, hipStream_t s);         // tick half: list the agents, note their rays
void launchAgentFrontRaysFromSnapshot(const DeviceState& d, const TickParams& p, hipStream_t s); // pair half, behind the merge: cast them
void launchFillSensors(const DeviceState& d, uint32_t first, uint32_t count, float rayLen, float safe, hipStream_t s);
constexpr uint32_t kMaxOccupancyQueries = 256;
void launchOccupancy(const DeviceState& d, uint32_t n, const float4* q, uint32_t count, uint32_t* blocked, hipStream_t s);

// launchers (sc_tick_kernels.hip)
void launchXformCull(const DeviceState& d, const TickParams& p, uint32_t grid, hipStream_t s, hipEvent_t evA = nullptr, hipEvent_t evB = nullptr);
// the classed tail culling instance with the compaction of the tick before at the head of its grid (carryInstance(p): such an instance exists for this launch)
bool carryInstance(const TickParams& p);
void launchXformCullCarry(const DeviceState& d, const TickParams& p, uint32_t grid, const DeviceState& pd, const TickParams& pp, uint32_t pgrid, uint32_t wideG,
                          hipStream_t s, hipEvent_t evA = nullptr, hipEvent_t evB = nullptr);
void launchSnapshotHome(const DeviceState& d, uint32_t sectors, uint32_t n, uint32_t binSX, uint32_t binSZ, uint32_t vocabMode, uint32_t vocab, uint32_t ordered, hipStream_t s);
void launchDeepLevel(const DeviceState& d, const TickParams& p, const uint32_t* levelList, uint32_t count, hipStream_t s);
// the end-of-tick kernel alone.  wideG: spans per workgroup of the wide form (compactWideGroup; 0: one workgroup per span, compactBody)
uint32_t compactWideGroup(const TickParams& p, uint32_t grid, uint32_t forced);
void compactLaunchShape(uint32_t grid, bool merged, uint32_t wideG, uint32_t shape[2]);
void launchCompact(const DeviceState& d, const TickParams& p, uint32_t grid, uint32_t wideG, hipStream_t s, hipEvent_t evA = nullptr, hipEvent_t evB = nullptr);
bool launchPairs(const DeviceState& d, const TickParams& p, hipStream_t s, hipEvent_t done = nullptr);
uint32_t pairRunFor(uint32_t sectors, uint32_t cus, bool sweepOnly);
void launchCompactPairs(const DeviceState& d, const TickParams& p, uint32_t compactGrid, hipStream_t s, hipEvent_t evA = nullptr, hipEvent_t evB = nullptr);
void launchGatherPairs(const DeviceState& d, const TickParams& p, uint32_t parity, uint2* dst, uint32_t* total, hipStream_t s);
void launchCompactPack(const DeviceState& d, const TickParams& p, uint32_t grid, hipStream_t s, hipEvent_t done = nullptr);
void launchBorderPack(const DeviceState& d, const TickParams& p, hipStream_t s);
void launchBorderMerge(const DeviceState& d, const TickParams& p, hipStream_t s);
void launchNudgeRootsX(const DeviceState& d, uint32_t n, float dx, hipStream_t s);
void launchRootMask(const DeviceState& d, uint32_t n, hipStream_t s);
void launchAdvanceMovers(const DeviceState& d, uint32_t n, float dt, float trafficSmooth, float trafficMult, hipStream_t s);
struct TierParams { float px, pz, aEnter, aExit, bEnter, bExit; };
void launchTrafficTiers(const DeviceState& d, uint32_t n, const TierParams& tp, hipStream_t s);
void launchApplyTiers(const DeviceState& d, uint32_t n, const uint2* patches, uint32_t patchCount, hipStream_t s);
void launchTrafficDespawnKeys(const DeviceState& d, uint32_t n, float px, float pz, uint32_t* count, uint32_t* outIdx, unsigned long long* outKey, hipStream_t s);
void launchDenseAabbs(const DeviceState& d, uint32_t n, hipStream_t s);
void launchSetDirtyRange(const DeviceState& d, uint32_t first, uint32_t count, hipStream_t s);
void launchSetDirtyIndices(const DeviceState& d, const uint32_t* idx, uint32_t count, hipStream_t s);
void launchMoveEntities(const DeviceState& d, const uint32_t* src, const uint32_t* dst, uint32_t moves, hipStream_t s);
void launchSetFrustum(const DeviceState& d, const Frustum6& fr, hipStream_t s);
void launchResetParity(const DeviceState& d, uint32_t q, hipStream_t s);
void launchPatchParents(const DeviceState& d, const uint32_t* pairs, uint32_t count, hipStream_t s);
void launchGatherRows(const DeviceState& d, const uint32_t* idx, uint32_t count, float* out12, hipStream_t s);
void launchEmitDraws(const DeviceState& d, uint32_t budget, void* items, hipStream_t s);
// ---- the frame read-back block: the one definition of its layout and of the 80-byte draw item ("Which code writes the frame")
// [header: kFrameHeaderWords][visible indices: frameVisibleWords(max_visible)][draw items: max_draws of kDrawItemBytes]
constexpr uint32_t kFrameHeaderWords = 16, kDrawItemBytes = 80;      // (kDrawItemBytes == sizeof(ScTickDrawItem): asserted in sc_tick_api.hip)
enum : uint32_t { kFhVisible = 0, kFhCulled = 1, kFhRenderablesTotal = 2, kFhDrawsEmitted = 3, kFhDrawsDropped = 4, kFhDrawsSorted = 5,
                  kFhTickLo = 6, kFhTickHi = 7, kFhVisibleInBuffer = 8, kFhDrawsInBuffer = 9 };      // (words 10 .. 15 are zero)
// the header's words, by value: a struct a writer indexes, not an array handed out through a pointer ("What the compiler decides on")
struct FrameHeader { uint32_t w[kFrameHeaderWords]; };
__host__ __device__ inline FrameHeader frameHeader(uint32_t visible, uint32_t culled, uint32_t total, uint32_t emitted, uint32_t dropped, uint32_t sorted,
                                                   uint32_t tickLo, uint32_t tickHi, uint32_t visibleInBuffer, uint32_t drawsInBuffer)
{
  return FrameHeader{ { visible, culled, total, emitted, dropped, sorted, tickLo, tickHi, visibleInBuffer, drawsInBuffer, 0, 0, 0, 0, 0, 0 } };
}
// word k for a thread that writes one of them: selects over registers (a run-time index into the struct would put it into LDS, 16 KB a workgroup)
__host__ __device__ inline uint32_t frameHeaderWord(const FrameHeader& h, uint32_t k)
{
  uint32_t v = 0u;
#pragma unroll
  for (uint32_t i = 0; i <= kFhDrawsInBuffer; ++i) v = (k == i) ? h.w[i] : v;
  return v;
}
// words the block keeps for the visible indices: max_visible rounded up to four, so that the draw items behind them stay 16-byte
// aligned.  The writers take max_visible as the caller gave it -- the clamp of visible_in_buffer -- and find the items through frameItems.
__host__ __device__ inline uint32_t frameVisibleWords(uint32_t maxVisible) { return (maxVisible + 3u) & ~3u; }
template <typename Word> __host__ __device__ inline Word* frameItems(Word* block, uint32_t maxVisible) { return block + kFrameHeaderWords + frameVisibleWords(maxVisible); }
inline size_t frameBlockBytes(uint32_t maxVisible, uint32_t maxDraws) { return ((size_t)kFrameHeaderWords + frameVisibleWords(maxVisible)) * 4u + (size_t)maxDraws * kDrawItemBytes; }
#ifdef __HIPCC__
// The draw item, written once: DrawItem{entity, mesh, material, worldMatrix} (sc_world_partition.cpp:1314-1321), the model column-major.
// `o`: the item's five float4; a, b, c: rows 0 .. 2 of entity j's world matrix, loaded by the caller (each source addresses the slab its own way).
__device__ __forceinline__ void writeDrawItem(const DeviceState& d, float4* o, uint32_t j, float4 a, float4 b, float4 c)
{
  o[0] = make_float4(__uint_as_float(j), __uint_as_float(d.meshId[j]), __uint_as_float(d.materialId[j]), 0.0f);
  o[1] = make_float4(a.x, b.x, c.x, 0.0f);     // column 0
  o[2] = make_float4(a.y, b.y, c.y, 0.0f);
  o[3] = make_float4(a.z, b.z, c.z, 0.0f);
  o[4] = make_float4(a.w, b.w, c.w, 1.0f);     // translation column
}
#endif
void launchEmitDrawsStaged(const DeviceState& d, uint32_t budget, uint32_t* block, uint32_t maxVisible, uint64_t tick, hipStream_t s, hipEvent_t done = nullptr);
void launchStageFrame(const DeviceState& d, uint32_t* block, uint32_t maxVisible, uint32_t maxDraws, const void* items, uint32_t drawMode /*0 none, 1 plain, 2 sorted*/,
                      uint64_t tick, hipStream_t s, hipEvent_t done = nullptr);

} // namespace sctick
