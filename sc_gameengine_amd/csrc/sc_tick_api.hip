// sc_tick_api.hip -- implementation of the C ABI in include/sc_tick.h (host side of libsc_tick.so).
//
// Host code here is compiled with -ffp-contract=off as well: the frustum planes and the sin/cos of
// the Euler angles are produced on the host with the same libm calls and the same operation order
// as the reference (sc_world_partition.cpp:1071-1103, sc_math.cpp:102-107).
#include "../../include/sc_tick.h"
#include "sc_tick_internal.h"
#include "sc_tick_rccl.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

using namespace sctick;

namespace {

thread_local std::string gCreateError;

struct EventPair { hipEvent_t a = nullptr, b = nullptr; };

// Which code writes the frame -- the draw items and the read-back block -- on a tick with these TickParams::flags: the one rule behind
// enqueueStages' launches and scTickGetFrameStats' report; planTick asks once per tick (framePathFor).
//   stagedEmit   the read-back is on and a plain draw list's budget fits the block: the items go straight into the block
//   foldEmit     the combined end-of-tick launch runs (compaction and pair search): its compaction role writes the items
//   stagedByEot  both: that role writes the whole block, header included
struct FramePath {
  bool needCompact, pairsNow, stagedEmit, foldEmit, stagedByEot;
  uint32_t items, block;               // SC_TICK_FRAME_ITEMS_* / SC_TICK_FRAME_BLOCK_*
};

// The record the readers see, in three groups, each with its own rule (ScTickContext::last, lastBinned, lastWith; recordRun).
// (1) The last ACCEPTED scTickRun: assigned whole from its plan, never in parts and never by a run that was refused.
struct RunRecord {
  uint32_t flags = 0;                                  // as requested (a quiet tick's SC_TICK_BROADPHASE included: scTickReadPairs answers)
  bool quiet = false, tail = false, topo = false;      // scTickGetBinStats bit 3 / scTickGetTailStats / scTickGetTopologyClassStats
  uint32_t compact[2] = { 0u, 0u };                    // the end-of-tick launch's shape (scTickGetCompactStats)
  uint32_t frame[2] = { 0u, 0u };                      // FramePath::items, block (scTickGetFrameStats)
  void* draws = nullptr;                               // where SC_TICK_DRAWS left its items: the frame read-back block, or null = the draw buffer (scTickReadDraws)
};
// (2) The most recent tick that BINNED with home slots -- a quiet or transform-only tick leaves it (scTickGetBinStats)
struct BinOutcome { bool lazy = false, stay = false, sweepOnly = false; };
// (3) The last accepted run THAT CARRIED THE FEATURE'S FLAG: what it was sized for or ran as (each reader checks RunRecord::flags first)
struct LastWith {
  bool sweepsExact = false;                            // SC_TICK_SWEEPS ran in EXACT mode (scTickGetSweepShapeInfo)
  uint32_t narrow = 0;                                 // the NarrowStage set SC_TICK_PAIR_SHAPES ran with: TickPlan::narrow of that run (narrowResult)
  uint32_t overlapCount = 0, overlapMaxHits = 0, overlapShapes = 0;      // what SC_TICK_OVERLAPS answered (scTickReadOverlapHits)
  uint32_t triggerCount = 0, triggerMaxMembers = 0, triggerMaxEvents = 0;     // what SC_TICK_TRIGGERS answered (scTickReadTrigger*)
  uint32_t asweepCount = 0; bool asweepsExact = false;  // what SC_TICK_ANCHORED_SWEEPS answered, and in which mode (scTickReadAnchoredSweep*, scTickGetAnchoredSweepShapeInfo)
  uint32_t bindTouchWords = 0; bool bindEmpty = false; // SC_TICK_BIND_RUNS: the bitmap's size; the run of an empty context (the report reads as zeros)
};

// Everything decided about one scTickRun.  planTick is its only writer; commitPlan, enqueueStages, graphKey and the record go by it and by
// nothing else of the tick.  A NEW PER-TICK DECISION IS A FIELD HERE, decided in planTick -- never a context field.
struct TickPlan {
  RunRecord rec;                       // what the readers are told once the run is accepted
  uint32_t run = 0;                    // the flags as run: a quiet tick runs without SC_TICK_BROADPHASE
  TickParams p{}; uint32_t grid = 0;
  FramePath path{};
  uint32_t compactG = 0;               // spans per workgroup of the end-of-tick kernel's wide form, 0 = compactBody's form
  uint32_t visSel = 0;                 // the copy of the visibility words this tick writes = ScTickContext::visSel once commitPlan has run (a carrying tick: not the copy its rider reads)
  bool sampled = false, carry = false, defer = false, replay = false, wholeStep = false;
  bool triggers = false;               // the trigger volumes are answered by this tick (k_trigger_volumes, at the overlap queries' launch site)
  bool anchoredSweeps = false;         // the entity-anchored sweeps are answered by this tick (k_anchored_sweeps, next to the trigger volumes' launch)
  uint32_t narrow = 0;                 // the NarrowStage set this tick's pair half executes (launchPairShapes goes by it, the record copies it)
  bool binned = false, learn = false;  // the home slots' side of a binning tick: it ran at all / as a learn tick ...
  uint32_t homeXform = 0;              // ... learnt with or without SC_TICK_XFORM (ScTickContext::homeXform)
  BinOutcome bins;
};

// What a capture was captured for: stale when any of it differs (graphKey; DESIGN, "What invalidates a capture")
struct GraphKey {
  TickParams p{};
  uint64_t epoch = ~0ull;              // ScTickContext::topoEpoch
  uint32_t compactG = 0, visSel = 0;   // TickPlan's: which form of the end-of-tick kernel is inside, which copy of the visibility words it writes
  bool rccl = false;                   // the library's RCCL group is inside (captured in relaxed mode)
  bool operator==(const GraphKey& o) const
  { return epoch == o.epoch && compactG == o.compactG && visSel == o.visSel && rccl == o.rccl && std::memcmp(&p, &o.p, sizeof p) == 0; }
};
// a captured graph of one tick parity
struct CapturedGraph { hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; GraphKey key; };

// a local box as uploaded, by bit pattern (-0 is not +0, a NaN is its bits): the key of the bounds palette
struct BoxKey {
  uint32_t w[6];
  bool operator==(const BoxKey& o) const { return std::memcmp(w, o.w, sizeof w) == 0; }
};
struct BoxKeyHash {
  size_t operator()(const BoxKey& k) const { uint64_t h = 0xcbf29ce484222325ull; for (uint32_t x : k.w) { h ^= x; h *= 0x100000001b3ull; } return (size_t)h; }
};

// host clock, microseconds (scTickTileStep: host time per half of a step, scTickGetCommInfo)
double nowUs() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

} // namespace

struct ScTickContext
{
  ScTickContextDesc desc{};
  int device = 0;
  uint32_t cap = 0;          // padded capacity
  uint32_t n = 0;
  hipStream_t stream = nullptr;
  DeviceState d{};
  std::vector<void*> allocs;
  std::string err;

  // host mirrors needed to (re)build link words
  std::vector<int32_t> hParent;
  std::vector<uint32_t> hLayers;     // group | mask << 16 as uploaded (scTickUploadLayers), for the world-vocabulary contract
  bool layerSetStale = true, ownLayersCanPair = true; uint32_t layerSetN = 0;      // worldCanPair(): do any two of this context's layer words admit a pair?
  std::vector<uint8_t> hFlags;       // bit0 has mesh, bit1 has bounds, bits 2..4 rotation about X/Y/Z trivial (sin 0, cos 1)
  // bounds classes (DeviceState::boundsPalette / tileClass): grow-only palette of the distinct boxes scTickUploadBounds has seen,
  // the class of every entity's box, and the host copy of the wave-tiles' words (refreshTiles keeps the device copy equal)
  std::unordered_map<BoxKey, uint32_t, BoxKeyHash> paletteIndex;
  std::vector<uint32_t> hPalette;    // 8 words per entry, as on the device
  std::vector<uint16_t> hClass;      // palette index per entity; kClassNone: the palette was full when its box arrived
  std::vector<uint32_t> hTile;
  // colliders (scTickUploadColliders): the five values per entity as uploaded -- what scTickReadColliders returns; the device keeps
  // the derived record (DeviceState::colShape / colType).  Empty until the first upload: every entity is SC_TICK_COLLIDER_BOUNDS.
  std::vector<uint8_t> hColType;
  std::vector<float> hColValues;     // [capacity][5]: half extents xyz, radius, half height
  std::vector<uint32_t> hChildren;   // direct children per entity (valid while !linksStale)
  // child lists in dense-index space (-1 = none), valid while !linksStale: a despawn patches exactly the links that
  // name a relocated entity instead of re-linking the world
  std::vector<int32_t> hFirstChild, hNextSib, hPrevSib;
  bool linksStale = true;
  uint32_t maxDepth = 0, unreachable = 0, relinks = 0;
  std::vector<uint32_t> levelOffsets;   // offsets into dLevelList for depth kMaxChain+1, +2, ...
  uint32_t* dLevelList = nullptr;
  uint32_t levelListCap = 0;

  Frustum6 frustum{};
  int frustumValid = 0;
  bool frustumStale = true;          // the device copy (DeviceState::frustum) is behind the host's
  int freeze = 0;

  uint32_t spansWanted = 1536;
  // Span-closed: no parent link crosses a span boundary (for every entity with a parent, parent / span == index / span; all ancestors
  // by induction).  Then the fused kernel's workgroups end the tick for their own spans (kFlagTailOwnsDirty).  Kept for the span it was
  // derived for (closureSpan; 0 = never derived): by rebuildLinks, by fillParams when another entity count gives another span, and by the
  // in-place remove path for the entities it relocates or re-parents.  A tick on which nothing changed scans nothing.
  bool tailEnabled = true;             // SC_TICK_TAIL=0 at creation: the end-of-tick kernel keeps the dirty clear and the producer (A/B switch)
  bool spanClosed = false; uint32_t closureSpan = 0;
  // Topology classes (topoTable(), bits 16..29 of the tile words): derived with the link words (flushLinks) from hParent and
  // hFlags.  topoCurrent: the device's link words are the ones the classes were derived from -- dropped by every path that edits link
  // words on the device without a re-link (appended roots, the in-place remove), until the next re-link.  hTopo: pattern index + 1 per
  // wave-tile as the tile words carry it.  A tick is eligible for the classed instance (kFlagTopoClasses, fillParams) when the classes are
  // current and no tile of the world is unclassed.
  bool topoEnabled = true;             // SC_TICK_TOPO_CLASSES=0 at creation: never eligible (A/B switch)
  bool topoCurrent = false;
  uint32_t topoPatterns = 0, topoClassed = 0, topoUnclassed = 0;
  std::vector<uint16_t> hTopo;
  // The end-of-tick kernel's wide form (k_compact_wide): SC_TICK_VARIANT bit 4 (16) at creation keeps one workgroup per span (A/B switch);
  // SC_TICK_COMPACT_G at creation fixes the spans per workgroup instead of compactWideGroup's rule (measurements, tests).  The tick's
  // own choice is TickPlan::compactG.
  bool wideCompact = true; uint32_t compactForceG = 0;
  // The carried compaction.  A tick whose end-of-tick launch would be k_compact_wide on its own may DEFER it
  // (deferCompact's rule): `pending` then holds that launch's arguments, and the next tick's fused launch carries it at the head of
  // its grid (k_xform_cull_classed_tail_carry) or -- where that tick cannot -- settle() launches it first.  Whoever reads a list or
  // the counts, or changes how ticks are launched, settles first.  vis / cand / blockVis / blockCand exist twice (visAlt: the second
  // copy): a carrying tick writes the copy its rider does not read, visSel names the copy the last tick wrote and stateFor hands it
  // to everyone.  carryEnabled: SC_TICK_CARRY=0 at creation never defers (A/B switch).  carryStats: scTickGetCarryStats.
  struct PendingCompact { bool on = false; DeviceState d{}; TickParams p{}; uint32_t grid = 0, wideG = 0; };
  PendingCompact pending;
  bool carryEnabled = true;
  uint32_t visSel = 0;
  uint64_t* visAlt[2] = { nullptr, nullptr };          // vis, cand
  uint32_t* blockAlt[2] = { nullptr, nullptr };        // blockVis, blockCand
  uint32_t carryStats[3] = { 0u, 0u, 0u };             // ticks deferred, compactions carried, compactions settled
  uint32_t cus = 0;           // compute units (hipDeviceProp_t::multiProcessorCount)
  RunRecord last; BinOutcome lastBinned; LastWith lastWith;      // the record the readers see: recordRun writes it, once a run is accepted

  // scratch device buffers for indexed read-back
  uint32_t* dIdx = nullptr; float* dRows = nullptr; uint32_t scratchCap = 0;
  void* dDraws = nullptr;
  RayQueryState rays{};                // scTickSetRayQueries: device copies of the batch + the hit buffer
  uint32_t rayCap = 0;
  SweepQueryState sweeps{};            // scTickSetSweepQueries: the same for the capsule sweeps
  uint32_t sweepCap = 0;
  // scTickSetAnchoredRays: the same for the entity-anchored rays, plus one snapshot of the resolved rays per tick parity (split flows:
  // parity q's lies q * anchoredCap entries into each snapshot array) and the host mirror of (anchor, skip_self) that
  // scTickRemoveEntities keeps current
  AnchoredRayState anchored{};
  uint32_t anchoredCap = 0;
  // scTickSetRayShapes: SC_TICK_RAY_SHAPES_EXACT selects the exact-shape instances of the ray and anchored-ray kernels (launch time:
  // a captured graph holds the instance it was captured with, so a change drops the graphs)
  uint32_t rayShapes = SC_TICK_RAY_SHAPES_AABB;
  // scTickSetSweepShapes: SC_TICK_SWEEP_SHAPES_EXACT selects the exact-shape instance of the sweep kernel, likewise; sweepInfo: the words of
  // its report (== ScTickSweepShapeInfo), allocated by the first call that sets EXACT, zeroed on the stream before every launch
  uint32_t sweepShapes = SC_TICK_SWEEP_SHAPES_AABB;
  uint32_t* sweepInfo = nullptr;
  // scTickSetOverlapQueries: the volumes, the count and id rows and the report's running words; overlapCap: volumes the per-volume arrays
  // hold, overlapIdCap: id slots.  overlapShapes selects the kernel instance at launch time, like the modes above.
  OverlapQueryState overlaps{};
  uint32_t overlapCap = 0; size_t overlapIdCap = 0;
  uint32_t overlapShapes = SC_TICK_OVERLAP_SHAPES_AABB;
  std::vector<uint2> hAnchor;
  // scTickSetTriggerVolumes: the volumes, one id row per volume (the member row IS the remembered row), the per-volume words, the two
  // event lists and the two slot counters; triggerCap: volumes the per-volume arrays hold, triggerIdCap: id slots, triggerEventCap:
  // events per list.  hTriggerAnchor mirrors (anchor, skip_self) for scTickRemoveEntities and scTickReadTriggerVolumes.
  TriggerState triggers{};
  uint32_t triggerCap = 0, triggerEventCap = 0; size_t triggerIdCap = 0;
  uint32_t triggerShapes = SC_TICK_OVERLAP_SHAPES_AABB;
  std::vector<uint2> hTriggerAnchor;
  // scTickSetAnchoredSweeps: the entity-anchored capsule sweeps, their hits and resolved segments; asweepInfo: the words of their EXACT
  // report (their own, not sweepInfo), allocated with the first set.  hSweepAnchor mirrors the anchor words for scTickRemoveEntities and
  // scTickReadAnchoredSweeps.  All null until the call: nothing is launched.
  AnchoredSweepState asweeps{};
  uint32_t asweepCap = 0;
  uint32_t* asweepInfo = nullptr;
  std::vector<uint4> hSweepAnchor;
  // scTickSetPairEvents: the tables, marks and control words of the pair events (one allocation, pairEventSlab: zero bytes all over =
  // nothing remembered, which is how a rename resyncs), the report and the two lists.  All null until the call: nothing is launched.
  PairEventState pairEvents{};
  void* pairEventSlab = nullptr; size_t pairEventSlabBytes = 0;
  bool pairEventsResyncAgain = false;      // ids were renamed between the halves of a split tick: forget again what its pair half remembers
  // The narrow phase: the touch events' state (scTickSetTouchEvents: the pair events' state a second time, filled by the narrow-phase
  // kernel; touchEventSlab is its one allocation) and the six stages of the touching pairs, which sizeNarrowPhase alone sizes.  All null
  // until the setters' calls: nothing is launched.
  NarrowPhase narrow{};
  void* touchEventSlab = nullptr; size_t touchEventSlabBytes = 0;
  DrawSortState sort{};                // renderer draw order (scTickSetDrawSortTable); key/idx buffers allocated on first use
  uint8_t* dPipeline = nullptr; uint32_t pipelineCap = 0;
  // scTickSetBindRuns: run table, report and touch bitmap of the sorted list (all null until the call: nothing is launched)
  BindRunState bind{};

  // profiling
  bool profiling = false;
  uint32_t profPeriod = 1;     // record events on every profPeriod-th tick only (event records are not free)
  uint32_t profMask = 0xFFFFFFFFu;   // ... and only around these kernels (bit SC_TICK_K_*; scTickSetProfilingKernels)
  uint64_t tickIndex = 0;
  std::vector<EventPair> times[SC_TICK_K_COUNT];
  std::vector<EventPair> eventPool;

  // graph
  bool graphMode = false;
  CapturedGraph graph[kMaxParity + 1];                 // the tick, one per broadphase tick parity; with its RCCL group: the whole tile step (exchange + pair half);
                                                       // [kMaxParity]: the quiet tick's (it binds to no parity, and alternating with binning ticks must not re-capture either)
  bool captureWholeStep = false;                       // set by scTickTileStep around its scTickRun
  bool ownStep = false;                                // scTickTileStep is running: the pair half follows the tick half at once, nothing of the host's in between
  uint64_t topoEpoch = 0;
  // pipelined tile + graph replay: the pair half (exchange, merge, queries, pair search, snapshot) is a graph of its own,
  // replayed on the pairs stream; the two graphs of a step are ordered by events recorded between them, outside any capture
  CapturedGraph pairGraph[kMaxParity];
  // home slots of the bins (binEntityWave): remembered at a learn tick, used until the world's shape changes or they age
  bool homeEnabled = true, homeValid = false, homeCountsLive = false;
  bool lazyEnabled = true;                             // lazy records (DeviceState::lazyCtl)
  bool fastPairs = true;                               // ordered home slots: bins without visitors take the pair role's fast path (DeviceState::homeCast)
  uint32_t learnTicks = 0;                             // scTickGetBinStats, scTickGetLearnTicks
  // Quiet ticks (quietTick()): a broadphase tick of a world that cannot pair, whose bins nothing else reads either, runs the device work
  // of the same call without SC_TICK_BROADPHASE; its pair set is empty by construction and reported so by the host
  bool quietEnabled = true;                            // SC_TICK_VARIANT bit 3 switches them off (A/B)
  bool worldLayersKnown = false; uint32_t worldLayers = 0;   // scTickSetWorldLayers: group bits | mask bits << 16 of every collider of the tiled world
  bool boxesTouched = false;                           // bounds or world matrices were uploaded since the last broadphase tick (TickParams::cleanStay)
  uint64_t homeEpoch = ~0ull; uint32_t homeAge = 0, homePeriod = 64;
  uint32_t homeXform = 0;                              // SC_TICK_XFORM of the learn tick: entities deeper than the fused kernel's chain are binned by the level
                                                       // kernels on transforming ticks and by the fused kernel otherwise -- slots learned one way are not valid the other

  // broadphase
  uint32_t sectors = 0, maxPairs = 0;
  uint2* dPairsOut = nullptr;          // gathered (contiguous) pair list for read-back
  uint32_t* dPairTotal = nullptr;      // [0] pairs found, [1] truncated flag
  uint32_t parity = 0, lastParity = 0;
  uint32_t rank = 0, neighbourMask = 0;
  uint32_t tileX = 0, tileZ = 0, tilesX = 0, tilesZ = 0;
  uint32_t producerKind = 0; float producerParam = 0.0f;      // part of the frame when set (scTickSetFrameProducer)
  float trafficMult = 1.0f;                                   // TrafficDebugState::speedMultiplier (sc_traffic_common.h:63)
  bool sensors = false; float sensorRay = 20.0f, sensorSafe = 10.0f;   // TrafficSensors defaults (sc_traffic_ai.cpp:307-309)
  bool halo = false;                                                    // border messages carry the halo section (sensors were on when the tile got its neighbours)
  void* laneAllocs[6] = {};                                   // device copies of the lane graph (scTickSetLaneGraph)
  uint2* dTierPatch = nullptr;                                // tier selection: the few modes the caps changed
  bool pairsPending = false;
  TickPlan pendingTick;                                // ... of this tick: its pair half goes by ITS plan (TickParams, sampling, learn), whatever ran in between
  hipStream_t ownStream = nullptr;
  // pipelined tiles (scTickSetPairsStream): merge + queries + pair search of tick t run on a second stream under the fused
  // kernel of tick t+1; everything the two halves share is double-buffered by tick parity (set 0 lives in `d`)
  hipStream_t pairsStream = nullptr;
  struct AltSet { uint32_t* binCount = nullptr; uint32_t* binLayers = nullptr; float4* bins = nullptr; float4* bigList = nullptr;
                  float4* spill = nullptr; uint32_t* spillSector = nullptr; uint32_t* ovfLo = nullptr; uint32_t* ovfHi = nullptr;
                  uint32_t* borderSend[8] = {}; uint32_t* borderRecv[8] = {}; };
  AltSet alt[kMaxParity - 1];          // parity q > 0 works on alt[q - 1]
  uint32_t pipeDepth = 3;              // copies a pipelined tile rotates through (scTickSetPipelined)
  uint32_t borderRecs = kBorderRecsPerBin;   // border messages: records per ring sector of a side on average (scTickSetBorderCapacity)
  hipEvent_t packed[kMaxParity] = {}, pairsDone[kMaxParity] = {};
  bool pairsInFlight[kMaxParity] = {};
  // library-owned exchange (scTickCommInit): one RCCL communicator per context, the border messages of both tick
  // parities in buffers of the library's own, the neighbour in direction d at rank peer[d]
  // per-frame read-back (scTickSetFrameReadback): staged on the tick stream, copied on a stream of its own, double-buffered
  struct FrameReadback {
    uint32_t maxVisible = 0, maxDraws = 0; size_t bytes = 0;
    uint32_t* dBlock[2] = {}; uint32_t* hBlock[2] = {};
    hipStream_t copyStream = nullptr; hipEvent_t staged[2] = {}, copied[2] = {};
    bool inFlight[2] = { false, false }; uint64_t frames = 0;
    // bind runs next to the frame (scTickAcquireFrameBinds): [kBiWords report][max_runs rows][touch words], copied behind the frame's block
    uint32_t* dBinds[2] = {}; uint32_t* hBinds[2] = {}; size_t bindBytes = 0;
    bool bindsStaged[2] = { false, false };      // that frame's run carried SC_TICK_BIND_RUNS
  } rb;
  ncclComm_t comm = nullptr;
  uint32_t commSize = 0, commRank = 0;
  int32_t peer[8] = { -1, -1, -1, -1, -1, -1, -1, -1 };
  bool peersSet = false;
  uint32_t* ownBorder[kMaxParity][8][2] = {};   // [parity][direction][send, recv]
  double hostAcc[2] = { 0.0, 0.0 }; uint64_t hostSteps = 0;     // scTickTileStep: host time issuing the tick half / the exchange + pair half
  hipStream_t ownPairsStream = nullptr;
  uint32_t* dGather = nullptr; uint32_t gatherCap = 0;          // scTickGatherVisibleCounts: one count per rank
};

namespace {

bool fail(ScTickContext* c, const char* what, hipError_t e = hipSuccess)
{
  char buf[512];
  if (e != hipSuccess) std::snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  else std::snprintf(buf, sizeof buf, "%s", what);
  if (c) c->err = buf; else gCreateError = buf;
  return false;
}

#define HIP_OK(c, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fail((c), #call, e_); return 0; } } while (0)

bool bind(ScTickContext* c)
{
  const hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail(c, "hipSetDevice", e);
  return true;
}

template <typename T>
bool dalloc(ScTickContext* c, T*& p, size_t count, bool zero = true)
{
  void* v = nullptr;
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  hipError_t e = hipMalloc(&v, bytes);
  if (e != hipSuccess) return fail(c, "hipMalloc", e);
  // (the tick stream is non-blocking, i.e. not ordered against the null stream this memset runs on, and a memset of device memory may
  //  return before it is done: wait for it, so that whatever is enqueued next sees the zeros -- allocations are rare)
  if (zero) { e = hipMemset(v, 0, bytes); if (e == hipSuccess) e = hipStreamSynchronize(nullptr); if (e != hipSuccess) return fail(c, "hipMemset", e); }
  c->allocs.push_back(v);
  p = static_cast<T*>(v);
  return true;
}

bool sync(ScTickContext* c);

void dfree(ScTickContext* c, void* p)
{
  if (!p) return;
  auto it = std::find(c->allocs.begin(), c->allocs.end(), p);
  if (it != c->allocs.end()) c->allocs.erase(it);
  hipFree(p);
}

// scratch index / row buffers for indexed calls: grown geometrically, the old pair is released
bool needScratch(ScTickContext* c, size_t count)
{
  if (c->scratchCap >= count) return true;
  if (!sync(c)) return false;                         // nothing queued may still read the old buffers
  const size_t want = std::max(count, (size_t)c->scratchCap * 2u);
  dfree(c, c->dIdx); dfree(c, c->dRows);
  c->dIdx = nullptr; c->dRows = nullptr; c->scratchCap = 0;
  if (!dalloc(c, c->dIdx, want, false) || !dalloc(c, c->dRows, want * 12, false)) return false;
  c->scratchCap = (uint32_t)want;
  return true;
}

bool rangeOk(ScTickContext* c, uint32_t first, uint32_t count)
{
  if ((uint64_t)first + count > c->n) return fail(c, "range exceeds entity count");
  return true;
}

bool h2d(ScTickContext* c, void* dst, const void* src, size_t bytes)
{
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream);
  if (e != hipSuccess) return fail(c, "hipMemcpyAsync H2D", e);
  return true;
}
bool d2h(ScTickContext* c, void* dst, const void* src, size_t bytes)
{
  const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream);
  if (e != hipSuccess) return fail(c, "hipMemcpyAsync D2H", e);
  return true;
}
bool sync(ScTickContext* c)
{
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, "hipStreamSynchronize", e);
  if (c->pairsStream) {                       // pipelined tiles: the pair search half runs on its own stream
    e = hipStreamSynchronize(c->pairsStream);
    if (e != hipSuccess) return fail(c, "hipStreamSynchronize (pairs stream)", e);
  }
  return true;
}

// the device state a tick of parity q works on: set 0 is `d` itself, set 1 swaps in the second copy of everything the
// pair search of one tick and the fused kernel of the next would otherwise share
DeviceState stateFor(const ScTickContext* c, uint32_t q)
{
  DeviceState s = c->d;
  // the visibility words and span counts the last tick wrote (the next one writes): the other copy may still feed a carried compaction
  if (c->visSel) { s.vis = c->visAlt[0]; s.cand = c->visAlt[1]; s.blockVis = c->blockAlt[0]; s.blockCand = c->blockAlt[1]; }
  if (c->pairsStream && q >= 1u && q < kMaxParity) {
    const ScTickContext::AltSet& a = c->alt[q - 1u];
    s.binCount = a.binCount; s.binLayers = a.binLayers; s.bins = a.bins; s.bigList = a.bigList;
    s.spill = a.spill; s.spillSector = a.spillSector; s.ovfLo = a.ovfLo; s.ovfHi = a.ovfHi;
    for (int k = 0; k < 8; ++k) { s.borderSend[k] = a.borderSend[k]; s.borderRecv[k] = a.borderRecv[k]; }
  }
  return s;
}

// A deferred compaction that nothing will carry: its own launch, now, on the tick stream -- plain k_compact_wide with the arguments the
// deferring tick would have given it, which is the launch order of a tick that never deferred.  Never dropped: carried or settled.
void settle(ScTickContext* c)
{
  if (!c->pending.on) return;
  launchCompact(c->pending.d, c->pending.p, c->pending.grid, c->pending.wideG, c->stream);
  c->pending.on = false;
  c->carryStats[2]++;
}

// results of the pair half (pairs, ray hits, broadphase counters) are read on the tick stream: let it finish first
bool joinPairs(ScTickContext* c)
{
  if (!c->pairsStream) return true;
  const hipError_t e = hipStreamSynchronize(c->pairsStream);
  if (e != hipSuccess) return fail(c, "hipStreamSynchronize (pairs stream)", e);
  return true;
}

// de-interleave [count][3] into three SoA streams and upload
bool upload3(ScTickContext* c, const float* src3, uint32_t first, uint32_t count, float* dx, float* dy, float* dz)
{
  std::vector<float> sx(count), sy(count), sz(count);
  for (uint32_t i = 0; i < count; ++i) { sx[i] = src3[3 * i]; sy[i] = src3[3 * i + 1]; sz[i] = src3[3 * i + 2]; }
  const bool ok = h2d(c, dx + first, sx.data(), count * 4u) && h2d(c, dy + first, sy.data(), count * 4u) &&
                  h2d(c, dz + first, sz.data(), count * 4u);
  return ok && sync(c);      // staging vectors die here
}

// ---- bounds classes ------------------------------------------------------------------------------------------------
// the palette entry of a box, added if it is new and there is room (kClassNone otherwise: always correct, only not faster)
uint32_t classOfBox(ScTickContext* c, const BoxKey& k)
{
  const auto it = c->paletteIndex.find(k);
  if (it != c->paletteIndex.end()) return it->second;
  const uint32_t at = (uint32_t)c->paletteIndex.size();
  if (at >= kPaletteCap) return kClassNone;
  c->paletteIndex.emplace(k, at);
  std::copy(k.w, k.w + 6, c->hPalette.begin() + 8u * (size_t)at);
  return at;
}
// entries [from, size) of the palette to the device (entries are never changed once written: a running tick reads older ones only)
bool uploadPalette(ScTickContext* c, uint32_t from)
{
  const uint32_t to = (uint32_t)c->paletteIndex.size();
  if (to <= from) return true;
  return h2d(c, const_cast<float*>(c->d.boundsPalette) + 8u * (size_t)from, c->hPalette.data() + 8u * (size_t)from, (size_t)(to - from) * 32u);
}
// does entity i have a broadphase proxy?  Its Bounds, until a collider says otherwise.
bool hasProxyHost(const ScTickContext* c, uint32_t i)
{
  const uint32_t type = c->hColType.empty() ? (uint32_t)SC_TICK_COLLIDER_BOUNDS : c->hColType[i];
  return type == SC_TICK_COLLIDER_BOUNDS ? (c->hFlags[i] & 2u) != 0u : type != SC_TICK_COLLIDER_NONE;
}
// the two words of wave-tile t from the host mirrors; entities at or past n are not part of it.  The shared box is over the
// entities with Bounds (culling and BOUNDS colliders read it), the shared layer word over the entities with a proxy.
void tileWords(const ScTickContext* c, uint32_t t, uint32_t out[2])
{
  const uint32_t lo = t * 64u, hi = std::min(c->n, lo + 64u);
  uint32_t cls = kClassMixed, layers = 0u; bool any = false, anyProxy = false, sameLayers = true;
  for (uint32_t i = lo; i < hi; ++i) {
    if (c->hFlags[i] & 2u) {
      if (!any) { any = true; cls = c->hClass[i]; }
      else if (c->hClass[i] != cls) cls = kClassMixed;    // (kClassNone == kClassMixed: a box outside the palette mixes its tile)
    }
    if (hasProxyHost(c, i)) {
      if (!anyProxy) { anyProxy = true; layers = c->hLayers[i]; }
      else if (c->hLayers[i] != layers) sameLayers = false;
    }
  }
  out[0] = (cls & kClassMask) | (any ? 0u : kTileNoBounds) | (sameLayers ? kTileLayersShared : 0u) | ((uint32_t)c->hTopo[t] << kTopoShift);
  out[1] = sameLayers ? layers : 0u;
}
// recompute the listed wave-tiles and bring the device copy up to date with one contiguous copy (the caller synchronises)
bool refreshTileList(ScTickContext* c, const std::vector<uint32_t>& tiles)
{
  if (tiles.empty()) return true;
  const uint32_t count = c->cap / 64u;
  uint32_t lo = count, hi = 0u;
  for (uint32_t t : tiles) {
    if (t >= count) continue;
    tileWords(c, t, &c->hTile[2u * (size_t)t]);
    lo = std::min(lo, t); hi = std::max(hi, t + 1u);
  }
  if (lo >= hi) return true;
  return h2d(c, const_cast<uint32_t*>(c->d.tileClass) + 2u * (size_t)lo, c->hTile.data() + 2u * (size_t)lo, (size_t)(hi - lo) * 8u);
}
// ... the wave-tiles that entities [first, end) lie in
bool refreshTiles(ScTickContext* c, uint32_t first, uint32_t end)
{
  if (end <= first) return true;
  std::vector<uint32_t> tiles;
  for (uint32_t t = first >> 6; t <= (end - 1u) >> 6; ++t) tiles.push_back(t);
  return refreshTileList(c, tiles);
}

// entities [first, first + count) back to SC_TICK_COLLIDER_BOUNDS with the default values (new indices: an appended entity must not
// inherit the collider of whoever held its index before)
bool resetColliders(ScTickContext* c, uint32_t first, uint32_t count)
{
  if (!c->d.colType || !count) return true;
  std::fill(c->hColType.begin() + first, c->hColType.begin() + first + count, (uint8_t)SC_TICK_COLLIDER_BOUNDS);
  std::fill(c->hColValues.begin() + 5u * (size_t)first, c->hColValues.begin() + 5u * ((size_t)first + count), 0.5f);
  const hipError_t e = hipMemsetAsync(c->d.colType + first, (int)kColliderBounds, count, c->stream);
  if (e != hipSuccess) return fail(c, "hipMemsetAsync", e);
  c->boxesTouched = true;
  return true;
}

void computeSpan(const ScTickContext* c, uint32_t& span, uint32_t& grid)
{
  const uint32_t n = std::max(c->n, 1u);
  const uint32_t tiles = (n + kTile - 1) / kTile;
  const uint32_t g = std::min(std::max(c->spansWanted, 1u), tiles);
  const uint32_t tilesPer = (tiles + g - 1) / g;
  span = tilesPer * kTile;
  grid = (n + span - 1) / span;
}

// the span-closed state from the parent mirror, for the span the current entity count gives (O(n): only where links or the span changed)
void deriveSpanClosed(ScTickContext* c)
{
  uint32_t span, grid;
  computeSpan(c, span, grid);
  c->closureSpan = span;
  c->spanClosed = scTickHostSpanClosed(c->hParent.data(), c->n, span) != 0;
}

// Transform::parent validation (sc_ecs.cpp:151-160) + depth / cycle classification.
// Returns the dense indices that were detached (they are marked dirty by the caller).
void rebuildLinks(ScTickContext* c, std::vector<uint32_t>& link, std::vector<uint32_t>& unreachBits,
                  std::vector<uint32_t>& detached, std::vector<std::vector<uint32_t>>& deepLevels)
{
  const uint32_t n = c->n;
  link.assign(n, 0);
  unreachBits.assign((c->cap + 31) / 32, 0);
  detached.clear();
  deepLevels.clear();

  std::vector<int32_t>& par = c->hParent;
  for (uint32_t i = 0; i < n; ++i) {
    const int32_t p = par[i];
    if (p == SC_TICK_NO_PARENT) continue;
    if (p < 0 || (uint32_t)p >= n || (uint32_t)p == i) { par[i] = SC_TICK_NO_PARENT; detached.push_back(i); }
  }

  std::fill(c->hChildren.begin(), c->hChildren.begin() + n, 0u);
  std::fill(c->hFirstChild.begin(), c->hFirstChild.begin() + n, -1);
  for (uint32_t i = n; i-- > 0;) {               // backwards, pushing at the front: lists come out in ascending order
    c->hNextSib[i] = -1; c->hPrevSib[i] = -1;
    if (par[i] == SC_TICK_NO_PARENT) continue;
    const uint32_t q = (uint32_t)par[i];
    c->hChildren[q]++;
    const int32_t head = c->hFirstChild[q];
    c->hNextSib[i] = head;
    if (head >= 0) c->hPrevSib[(uint32_t)head] = (int32_t)i;
    c->hFirstChild[q] = (int32_t)i;
  }

  // depth by walking up with memoisation; a walk that meets its own trail has found a cycle
  constexpr int32_t kUnknown = -1, kCycle = -2;
  std::vector<int32_t> depth(n, kUnknown);
  std::vector<uint32_t> trailMark(n, 0);
  std::vector<uint32_t> trail;
  for (uint32_t i = 0; i < n; ++i) {
    if (depth[i] != kUnknown) continue;
    trail.clear();
    uint32_t cur = i;
    int32_t above = -1;          // depth of the resolved node just above the trail (-1: the trail ends in a root)
    bool cyc = false;
    const uint32_t stamp = i + 1u;
    for (;;) {
      if (depth[cur] != kUnknown) { cyc = depth[cur] == kCycle; above = depth[cur]; break; }
      if (trailMark[cur] == stamp) { cyc = true; break; }       // met our own trail: a parent cycle
      trailMark[cur] = stamp;
      trail.push_back(cur);
      if (par[cur] == SC_TICK_NO_PARENT) break;
      cur = (uint32_t)par[cur];
    }
    // trail holds the unresolved nodes from i upward; number them from the top down.  Everything
    // that leads into a cycle has no root above it either, so it is unreachable as well.
    for (size_t k = trail.size(); k-- > 0;) depth[trail[k]] = cyc ? kCycle : ++above;
  }

  c->maxDepth = 0; c->unreachable = 0;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t dfield;
    if (depth[i] == kCycle) { dfield = kUnreachable; c->unreachable++; unreachBits[i >> 5] |= 1u << (i & 31u); }
    else {
      const uint32_t dv = (uint32_t)depth[i];
      c->maxDepth = std::max(c->maxDepth, dv);
      if (dv <= kMaxChain) dfield = dv;
      else {
        dfield = kDeep;
        const uint32_t lv = dv - kMaxChain - 1;
        if (deepLevels.size() <= lv) deepLevels.resize(lv + 1);
        deepLevels[lv].push_back(i);
      }
    }
    const uint32_t p = (par[i] == SC_TICK_NO_PARENT) ? kNoParent : (uint32_t)par[i];
    link[i] = p | ((c->hFlags[i] & 1u) ? kHasMesh : 0u) | ((c->hFlags[i] & 2u) ? kHasBounds : 0u) | (dfield << kDepthShift) |
              ((c->hFlags[i] & 4u) ? kRotTrivialX : 0u) | ((c->hFlags[i] & 8u) ? kRotTrivialY : 0u) | ((c->hFlags[i] & 16u) ? kRotTrivialZ : 0u);
  }
  deriveSpanClosed(c);
}

// The topology classes of the world as hParent and hFlags stand (behind rebuildLinks: invalid parents are detached), the pattern table
// and the tile words' class bits to the device (the caller synchronises).  Tile words are copied only where a class changed.
bool refreshTopoClasses(ScTickContext* c)
{
  const uint32_t tiles = (c->n + 63u) / 64u, all = c->cap / 64u;
  std::vector<uint16_t> cls(tiles, (uint16_t)0);
  std::vector<uint32_t> words((size_t)kTopoCap * 64u);
  uint32_t patterns = 0;
  c->topoCurrent = false;
  if (!scTickHostTopologyClasses(c->hParent.data(), c->hFlags.data(), c->n, kTopoCap, cls.data(), &patterns, words.data())) return fail(c, "topology classes");
  c->topoPatterns = patterns; c->topoClassed = 0;
  for (uint32_t t = 0; t < tiles; ++t) if (cls[t]) c->topoClassed++;
  c->topoUnclassed = tiles - c->topoClassed;
  if (patterns) {
    std::vector<uint32_t> table((size_t)patterns * 128u);
    for (uint32_t q = 0; q < patterns; ++q)
      for (uint32_t lane = 0; lane < 64u; ++lane) topoEntry(&words[64u * (size_t)q], lane, &table[((size_t)q * 64u + lane) * 2u]);
    if (!h2d(c, const_cast<uint2*>(topoTable(c->d.boundsPalette)), table.data(), table.size() * sizeof(uint32_t))) return false;
  }
  uint32_t lo = all, hi = 0u;
  for (uint32_t t = 0; t < all; ++t) {
    const uint16_t want = t < tiles ? cls[t] : (uint16_t)0;
    if (c->hTopo[t] == want) continue;
    c->hTopo[t] = want;
    c->hTile[2u * (size_t)t] = (c->hTile[2u * (size_t)t] & ~(kTopoMask << kTopoShift)) | ((uint32_t)want << kTopoShift);
    lo = std::min(lo, t); hi = std::max(hi, t + 1u);
  }
  if (lo < hi && !h2d(c, const_cast<uint32_t*>(c->d.tileClass) + 2u * (size_t)lo, c->hTile.data() + 2u * (size_t)lo, (size_t)(hi - lo) * 8u)) return false;
  c->topoCurrent = true;
  return true;
}

int flushLinks(ScTickContext* c)
{
  if (!c->linksStale) return 1;
  std::vector<uint32_t> link, unreachBits, detached;
  std::vector<std::vector<uint32_t>> deep;
  rebuildLinks(c, link, unreachBits, detached, deep);
  if (!refreshTopoClasses(c)) return 0;
  if (c->n) { if (!h2d(c, c->d.link, link.data(), (size_t)c->n * 4u)) return 0; }
  launchRootMask(c->d, c->n, c->stream);
  if (!h2d(c, c->d.unreach, unreachBits.data(), unreachBits.size() * 4u)) return 0;

  c->levelOffsets.assign(1, 0);
  std::vector<uint32_t> flat;
  for (auto& lv : deep) { flat.insert(flat.end(), lv.begin(), lv.end()); c->levelOffsets.push_back((uint32_t)flat.size()); }
  if (!flat.empty()) {
    if (flat.size() > c->levelListCap) {
      if (!sync(c)) return 0;
      dfree(c, c->dLevelList); c->dLevelList = nullptr; c->levelListCap = 0;
      uint32_t* p = nullptr;
      if (!dalloc(c, p, flat.size(), false)) return 0;
      c->dLevelList = p; c->levelListCap = (uint32_t)flat.size();
    }
    if (!h2d(c, c->dLevelList, flat.data(), flat.size() * 4u)) return 0;
  }
  uint32_t* dDet = nullptr;
  if (!detached.empty()) {
    // detached entities become dirty roots (sc_ecs.cpp:154-160)
    if (!needScratch(c, detached.size())) return 0;
    dDet = c->dIdx;
    if (!h2d(c, dDet, detached.data(), detached.size() * 4u)) return 0;
    launchSetDirtyIndices(c->d, dDet, (uint32_t)detached.size(), c->stream);
  }
  if (!sync(c)) return 0;
  c->linksStale = false;
  c->topoEpoch++;
  c->relinks++;
  return 1;
}

EventPair takeEvents(ScTickContext* c)
{
  EventPair p;
  if (!c->eventPool.empty()) { p = c->eventPool.back(); c->eventPool.pop_back(); return p; }
  hipEventCreate(&p.a); hipEventCreate(&p.b);
  return p;
}

// The profiling sampling rule.  A tick is sampled when profiling is on and its index is a multiple of the period; its pair half
// goes by the tick's decision (TickPlan::sampled, kept with the pending tick).  Kernel k is timed on a launch when timing is allowed there -- the tick or its
// pair half is sampled and runs eagerly: never inside a stream capture -- and k is in the mask.
bool tickSampled(const ScTickContext* c) { return c->profiling && (c->tickIndex % c->profPeriod) == 0; }
bool timed(const ScTickContext* c, uint32_t k, bool allowed) { return allowed && c->profiling && ((c->profMask >> k) & 1u); }

// kernel k timed by marker events around the launches in scope (~6 us of gap on the queue per marker)
struct Scoped
{
  ScTickContext* c; uint32_t k; EventPair p; bool on;
  Scoped(ScTickContext* c_, uint32_t k_, bool allowed) : c(c_), k(k_), on(timed(c_, k_, allowed))
  {
    if (on) { p = takeEvents(c); hipEventRecord(p.a, c->stream); }
  }
  ~Scoped() { if (on) { hipEventRecord(p.b, c->stream); c->times[k].push_back(p); } }
};

// Capacity of the sector overflow list, in records.  A box has at most four records (the sectors its xz range touches), a
// bin keeps 64 of a sector's, so 4 x capacity can never run out for a tile's own boxes however crowded its sectors are; the
// neighbours' border records that find their landing bin full come on top (what a border message can carry, eight messages).
uint32_t ovfRecords(const ScTickContext* c)
{
  const uint64_t own = 4ull * c->cap;
  uint64_t border = 0;
  for (uint32_t d = 0; d < 8; ++d) border += borderRecCap(borderLen(d, c->desc.tile_sectors_x, c->desc.tile_sectors_z), c->borderRecs);
  return (uint32_t)std::min<uint64_t>(own + border, 0xFFFFFF00ull);
}

void fillParams(ScTickContext* c, uint32_t flags, TickParams& p, uint32_t& grid)
{
  std::memset(&p, 0, sizeof p);
  p.n = c->n;
  computeSpan(c, p.span, grid);
  p.flags = flags & 0xFFFFu;        // SC_TICK_DENSE_AABBS == kFlagDenseAabbs
  if (c->levelOffsets.size() > 1 && (flags & SC_TICK_XFORM)) p.flags |= kFlagHasDeep;
  if (flags & SC_TICK_ANCHORED_SWEEPS) p.flags |= kFlagAnchoredSweeps;      // (likewise: bit 18 is kFlagTailOwnsDirty's position)
  if (flags & SC_TICK_TRIGGERS) p.flags |= kFlagTriggers;      // (likewise: bit 17 is kFlagDeferredReset's position)
  if (flags & SC_TICK_OVERLAPS) p.flags |= kFlagOverlaps;      // (the public bit is one of the internal ones' positions: it travels as a bit of its own)
  // The fused kernel's workgroups end the tick for their own spans (spanTail) when the world is span-closed, no level kernel reads `dirty`
  // behind the fused kernel, and the tick's producer is none or the root nudge.  The movers' producer stays in the end-of-tick kernel
  // (the agents' front rays are cast between the two kernels against this frame's positions), and so does the nudge while traffic
  // sensors are on, for the same reason.  Part of a captured graph's key, like every flag.
  if (p.span != c->closureSpan) deriveSpanClosed(c);       // (appends / removes moved the entity count to another span; hParent is current: flushLinks ran)
  const bool producerOk = !(flags & SC_TICK_PRODUCE_NEXT) || (c->producerKind == 1u && !c->sensors);
  if (c->tailEnabled && (flags & SC_TICK_XFORM) && !(p.flags & kFlagHasDeep) && c->spanClosed && producerOk) p.flags |= kFlagTailOwnsDirty;
  // The classed instance of the fused kernel (kFlagTopoClasses): a tick with the transform half and without binning, in a world with a
  // hierarchy (a flat world has no walk to save), no deep level and no unreachable entity, whose every wave-tile is classed by classes
  // that are current.  Part of a captured graph's key, like every flag.
  if (c->topoEnabled && c->topoCurrent && (flags & SC_TICK_XFORM) && !(flags & SC_TICK_BROADPHASE) && c->levelOffsets.size() <= 1 && c->unreachable == 0
      && c->maxDepth >= 1 && c->maxDepth <= kMaxChain && c->n && c->topoUnclassed == 0) p.flags |= kFlagTopoClasses;
  p.freeze = c->freeze ? 1u : 0u;
  p.frustumValid = c->frustumValid ? 1u : 0u;
  // the bin grid is the tile plus a ring of one sector: boxes that poke over the tile edge stay
  // binnable, and on a multi-GPU world the ring is where a neighbour's border boxes land
  p.binOx = (float)c->desc.tile_origin_x - 1.0f;
  p.binOz = (float)c->desc.tile_origin_z - 1.0f;
  p.invSector = 1.0f / c->desc.sector_size;                 // worldToSector, sc_world_partition.cpp:270
  p.binSX = c->desc.tile_sectors_x ? c->desc.tile_sectors_x + 2u : 0u;
  p.binSZ = c->desc.tile_sectors_x ? c->desc.tile_sectors_z + 2u : 0u;
  p.parity = c->parity;
  p.maxPairs = c->maxPairs;
  p.rankBits = c->rank << 24;
  p.neighbourMask = c->neighbourMask;
  p.chain = std::min(c->maxDepth, kMaxChain);
  p.ovfCap = ovfRecords(c);
  if (c->pairsStream && (flags & SC_TICK_BROADPHASE)) { p.flags |= kFlagDeferredReset; p.resetParity = (c->parity + 1u) % c->pipeDepth; }
  if (flags & SC_TICK_PRODUCE_NEXT) { p.producerKind = c->producerKind; p.producerParam = c->producerParam; }
  p.trafficSmooth = 1.0f - std::exp(-2.5f * c->producerParam);       // smoothExp(current, target, 2.5f, dt), sc_traffic_ai.cpp:58-62, :437
  p.trafficMult = c->trafficMult;
  p.bigCap = c->cap + 8u * kBorderBigCap;
  p.cus = c->cus;
  p.pairRun = pairRunFor(p.binSX * p.binSZ, c->cus, false);
  p.borderRecs = c->borderRecs;
  p.halo = c->halo ? 1u : 0u;
  p.tileX = c->tileX; p.tileZ = c->tileZ; p.tilesX = c->tilesX; p.tilesZ = c->tilesZ;
  p.colliders = c->d.colType ? 1u : 0u;         // (part of a captured graph's key: the instance choice follows it)
}

// the sweeps' instance: the report words of the exact-shape kernel, nullptr in AABB mode (launchSweepQueries chooses by it)
uint32_t* exactSweepInfo(const ScTickContext* c) { return c->sweepShapes == SC_TICK_SWEEP_SHAPES_EXACT ? c->sweepInfo : nullptr; }

// the anchored rays as a tick of parity q sees them: its own copy of the snapshot
AnchoredRayState anchoredFor(const ScTickContext* c, uint32_t q)
{
  AnchoredRayState a = c->anchored;
  if (a.snapOrigin) { const size_t off = (size_t)q * c->anchoredCap; a.snapOrigin += off; a.snapDir += off; a.snapSkip += off; }
  return a;
}

// pair events: forget the remembered set (dense indices were renamed, or are no longer valid) -- the next flagged tick is a resync tick.
// Queued on the tick stream, behind the ticks already issued.
// Collider shapes in the caller-owned split flow: a pair half that refines by shape -- rays in EXACT mode, the touching pairs -- reads the
// matrix rows, the collider records and the dense indices AS THEY STAND when it runs (the bins hold tick t's boxes, nothing holds tick
// t's shapes).  So whatever rewrites one of those is refused between the halves of such a tick -- tick t's answers stay tick t's.
// What the pending pair half does with the shapes (nullptr: nothing, the gap is the host's):
const char* pendingShapeReader(const ScTickContext* c)
{
  if (!c->pairsPending) return nullptr;
  if (c->rayShapes == SC_TICK_RAY_SHAPES_EXACT && (c->pendingTick.p.flags & (SC_TICK_RAYS | SC_TICK_ANCHORED_RAYS)))
    return "casts rays in SC_TICK_RAY_SHAPES_EXACT mode";
  if (c->sweepShapes == SC_TICK_SWEEP_SHAPES_EXACT && (c->pendingTick.p.flags & SC_TICK_SWEEPS))
    return "sweeps capsules in SC_TICK_SWEEP_SHAPES_EXACT mode";
  if (c->pendingTick.p.flags & SC_TICK_PAIR_SHAPES) return "lists the touching pairs (SC_TICK_PAIR_SHAPES)";
  if (c->pendingTick.p.flags & SC_TICK_TOUCH_EVENTS) return "reports touch events (SC_TICK_TOUCH_EVENTS)";
  return nullptr;
}
#define REFUSE_WHILE_SHAPES_PENDING(c, what) \
  do { if (const char* reads = pendingShapeReader(c)) \
         return fail(c, (std::string(what " is refused between scTickRun(.. | SC_TICK_SPLIT_PAIRS) and scTickRunPairs of a tick that ") + reads + \
                         ": its pair half reads the matrices and colliders as they stand").c_str()); } while (0)

// Trigger volumes: "nothing remembered" is a per-volume word, reset here by the host -- outside any captured graph -- behind whatever is
// queued: the next flagged tick is a resync tick for every volume.
bool resyncTriggers(ScTickContext* c)
{
  if (!c->triggers.count) return true;
  const hipError_t e = hipMemsetAsync(c->triggers.remembered, 0xFF, (size_t)c->triggers.count * sizeof(uint32_t), c->stream);
  return e == hipSuccess ? true : fail(c, "hipMemsetAsync (trigger volumes)", e);
}

// (touch events remember pairs by the same ids: they are forgotten in the same places, by the same call)
bool resyncPairEvents(ScTickContext* c)
{
  if (!resyncTriggers(c)) return false;               // (trigger volumes remember members by the same ids: forgotten in the same places)
  if (c->pairEventSlab) {
    const hipError_t e = hipMemsetAsync(c->pairEventSlab, 0, c->pairEventSlabBytes, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemsetAsync (pair events)", e);
  }
  if (c->touchEventSlab) {
    const hipError_t e = hipMemsetAsync(c->touchEventSlab, 0, c->touchEventSlabBytes, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemsetAsync (touch events)", e);
  }
  if (c->narrow.persist.ctl) {                           // (pair persistence remembers entries by the same ids: both tables empty, nothing valid)
    const hipError_t e = hipMemsetAsync(c->narrow.persist.ctl, 0, c->narrow.persist.slabBytes, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemsetAsync (pair persistence)", e);
  }
  if (c->narrow.sleep.ctl) {                             // (pair sleep keeps anchors and rest counts by dense index: nothing remembered, the epoch from 1)
    const hipError_t e = hipMemsetAsync(c->narrow.sleep.ctl, 0, c->narrow.sleep.slabBytes, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemsetAsync (pair sleep)", e);
  }
  // caller-owned split flow: the pair half of the tick already issued is still to come and will remember ITS set, in the ids from before
  // the rename -- runPendingPairs forgets it again behind that half
  if (c->pairsPending && ((c->pendingTick.p.flags & (SC_TICK_PAIR_EVENTS | SC_TICK_TOUCH_EVENTS)) || (c->pendingTick.narrow & (kStagePersist | kStageSleep))))
    c->pairEventsResyncAgain = true;
  return true;
}

// What closes every pair half, behind the pair search on its stream, now that the pair set is complete.  The narrow phase -- which of its
// pairs touch: ONE launch of the pair-shape kernel whatever mix of SC_TICK_PAIR_SHAPES and SC_TICK_TOUCH_EVENTS the tick carries (each
// pair is decided once), then the list's report and / or the touch state's sweep and finish -- then the pair events: what begun, what ended.
void closePairHalf(ScTickContext* c, const DeviceState& ds, const TickPlan& plan, hipStream_t s)
{
  const TickParams& p = plan.p;
  if (plan.narrow) launchPairShapes(ds, p, c->narrow, plan.narrow, s);
  if (p.flags & SC_TICK_PAIR_EVENTS) launchPairEvents(ds, p, c->pairEvents, s);
}

// pipelined tiles: a tick refills the bins and counters of its parity, which the pair half of pipeDepth ticks ago read, and
// the tick before it clears those counters.  That half finished long ago unless the exchange is very slow; wait for it.
// (Cross-stream: never captured.)
void waitParityFree(ScTickContext* c, const TickParams& p)
{
  // this tick's end-of-tick kernel clears the NEXT tick's parity (TickParams::resetParity), whose last pair half -- pipeDepth - 1
  // ticks ago -- must be over by then; this tick's own parity was made free one tick ago the same way
  const uint32_t q = p.resetParity;
  if (!(p.flags & kFlagDeferredReset) || !c->pairsInFlight[q]) return;
  // (a queue-to-queue wait costs a bubble of ~10 us on the device even when it is already satisfied: ask first)
  if (hipEventQuery(c->pairsDone[q]) != hipSuccess) {
    // The host is usually ahead of the device here (the flow is device-bound), so the pair half of pipeDepth - 1 ticks ago has often not ended
    // when this tick is issued -- and the queue-to-queue wait then sits in front of this tick's fused kernel on every step: 4-5 us of
    // bubble on the tick stream (tools/trace_timeline.py).  The HOST waits instead (round 4): no tick is issued more than pipeDepth - 1
    // ticks ahead of a finished pair half, the tick stream never sees a barrier, and with the tick before this one already queued the
    // device does not run dry.
    (void)hipEventSynchronize(c->pairsDone[q]);
  }
  (void)hipGetLastError();                        // hipErrorNotReady from the query is not an error
  c->pairsInFlight[q] = false;
}

// pipelined tiles: whatever is queued on the pairs stream from here on (the exchange) is ordered behind this tick's pack
// (rode: the event was attached to the compaction + pack dispatch already -- enqueueStages' answer)
void publishPacked(ScTickContext* c, const TickParams& p, bool rode)
{
  if (!c->pairsStream || !(p.flags & SC_TICK_BROADPHASE) || !(p.flags & SC_TICK_SPLIT_PAIRS)) return;
  if (!rode) hipEventRecord(c->packed[p.parity], c->stream);
  hipStreamWaitEvent(c->pairsStream, c->packed[p.parity], 0);
}

// Obstacle rays on a tiled world (sc_traffic_ai.cpp:300-345: the reference's ray sees the whole physics world): with neighbours, the halo
// section in the messages and an in-order step, the rays are cast in the PAIR half behind the merge.  A pipelined tile keeps them in
// the tick half (its own boxes only): the pair half of tick t runs under tick t + 1, whose frame producer reads the brakes.
bool raysInPairHalf(const ScTickContext* c, uint32_t flags)
{
  return c->sensors && c->halo && c->neighbourMask && !c->pairsStream && (flags & SC_TICK_SPLIT_PAIRS) && (flags & SC_TICK_BROADPHASE);
}

// Bind runs next to the frame read-back: the two staging blocks and their pinned copies exist while both features are on.  Called
// by whichever of scTickSetBindRuns, scTickSetDrawSortTable and scTickSetFrameReadback changed a size (the tick stream is idle by then).
bool reallocBindBlocks(ScTickContext* c)
{
  ScTickContext::FrameReadback& rb = c->rb;
  if (rb.copyStream && hipStreamSynchronize(rb.copyStream) != hipSuccess) return fail(c, "hipStreamSynchronize (copy stream)");
  for (int k = 0; k < 2; ++k) {
    dfree(c, rb.dBinds[k]); rb.dBinds[k] = nullptr; rb.bindsStaged[k] = false;
    if (rb.hBinds[k]) { hipHostFree(rb.hBinds[k]); rb.hBinds[k] = nullptr; }
  }
  rb.bindBytes = 0;
  if (!rb.bytes || !c->bind.info) return true;
  const size_t words = (size_t)kBiWords + (size_t)c->bind.maxRuns * 6u + c->bind.touchWords;
  for (int k = 0; k < 2; ++k) {
    if (!dalloc(c, rb.dBinds[k], words)) return false;
    void* h = nullptr;
    if (hipHostMalloc(&h, words * 4u, hipHostMallocDefault) != hipSuccess) return fail(c, "hipHostMalloc (bind runs)");
    std::memset(h, 0, words * 4u);
    rb.hBinds[k] = static_cast<uint32_t*>(h);
  }
  rb.bindBytes = words * 4u;
  return true;
}

// the run table (one row more than reported: sc_tick_bindruns.hip), the report and -- sized by the sort table's material_count -- the bitmap.
// The callers see to it that no captured graph keeps the old buffers.
bool reallocBindRuns(ScTickContext* c, uint32_t maxRuns)
{
  BindRunState& b = c->bind;
  dfree(c, b.runs); dfree(c, b.info);
  b = BindRunState{};
  if (maxRuns) {
    const uint32_t touchWords = (c->sort.materialCount + 31u) / 32u;
    if (!dalloc(c, b.runs, (size_t)maxRuns + 1u) || !dalloc(c, b.info, (size_t)kBiWords + touchWords)) return false;
    b.touch = b.info + kBiWords;
    b.maxRuns = maxRuns; b.touchWords = touchWords; b.materialCount = c->sort.materialCount;
  }
  return reallocBindBlocks(c);
}

// frame read-back: this tick's slot of the two blocks, which the copy of two frames ago may still read; the tick stream waits for it
uint32_t frameSlot(const ScTickContext::FrameReadback& rb) { return (uint32_t)(rb.frames & 1u); }
// (asked first: a satisfied wait costs a bubble too)
void waitFrameBlock(ScTickContext* c)
{
  ScTickContext::FrameReadback& rb = c->rb;
  const uint32_t f = frameSlot(rb);
  if (!rb.inFlight[f]) return;
  if (hipEventQuery(rb.copied[f]) != hipSuccess) hipStreamWaitEvent(c->stream, rb.copied[f], 0);
  (void)hipGetLastError();
}

// this tick's frame is on its way to the host (or, on an emptied context, already there): `copied` is what scTickAcquireFrame waits on
hipError_t publishFrame(ScTickContext* c, bool bindsStaged)
{
  ScTickContext::FrameReadback& rb = c->rb;
  const uint32_t f = frameSlot(rb);
  rb.bindsStaged[f] = bindsStaged; rb.inFlight[f] = true;
  rb.frames++;
  return hipEventRecord(rb.copied[f], rb.copyStream);
}

// the frame path (FramePath) of a tick with these TickParams::flags
FramePath framePathFor(const ScTickContext* c, uint32_t flags)
{
  FramePath f;
  // (kFlagTailOwnsDirty: the transform half left nothing for the end-of-tick kernel -- without culling there is no compaction role to launch)
  f.needCompact = (flags & SC_TICK_CULL) != 0 || ((flags & SC_TICK_XFORM) && !(flags & kFlagTailOwnsDirty));
  f.pairsNow = (flags & SC_TICK_BROADPHASE) && !(flags & SC_TICK_SPLIT_PAIRS);
  const uint32_t drawBudget = c->desc.max_draws_budget;
  f.stagedEmit = c->rb.bytes && (flags & SC_TICK_DRAWS) && !(flags & SC_TICK_SORT_DRAWS) && drawBudget && drawBudget <= c->rb.maxDraws;
  f.foldEmit = f.needCompact && f.pairsNow && (flags & SC_TICK_CULL) && (flags & SC_TICK_DRAWS) &&
               !(flags & SC_TICK_SORT_DRAWS) && (f.stagedEmit || !c->rb.bytes);
  f.stagedByEot = f.foldEmit && f.stagedEmit;
  f.items = !(flags & SC_TICK_DRAWS) ? SC_TICK_FRAME_ITEMS_NONE : (flags & SC_TICK_SORT_DRAWS) ? SC_TICK_FRAME_ITEMS_SORT
          : f.stagedByEot ? SC_TICK_FRAME_ITEMS_EOT_BLOCK : f.foldEmit ? SC_TICK_FRAME_ITEMS_EOT_BUFFER
          : f.stagedEmit ? SC_TICK_FRAME_ITEMS_EMIT_STAGED : SC_TICK_FRAME_ITEMS_EMIT;
  f.block = !c->rb.bytes ? SC_TICK_FRAME_BLOCK_NONE : f.stagedByEot ? SC_TICK_FRAME_BLOCK_EOT
          : f.stagedEmit ? SC_TICK_FRAME_BLOCK_EMIT_STAGED : SC_TICK_FRAME_BLOCK_STAGE;
  return f;
}

// path.foldEmit.  Draw emission rides in the end-of-tick kernel when the order is the plain one: the compaction role knows every visible
// entity's place in the list, i.e. its draw item (emitVisible).  With the frame read-back on (and a budget that fits the block)
// the items, the head of the visible list and the header go straight into the block -- no emission kernel, no staging kernel.
// Fills the launch's `pe`; returns the event it records (the block's `staged`), or null.
hipEvent_t fillFoldEmit(ScTickContext* c, const FramePath& path, TickParams& pe)
{
  pe.emitBudget = c->desc.max_draws_budget;
  if (!path.stagedByEot) { pe.emitMode = 1u; pe.emitTarget = reinterpret_cast<uint32_t*>(c->dDraws); return nullptr; }
  ScTickContext::FrameReadback& rb = c->rb;
  const uint32_t f = frameSlot(rb);
  waitFrameBlock(c);
  pe.emitMode = 2u; pe.emitTarget = rb.dBlock[f]; pe.emitMaxVisible = rb.maxVisible;
  pe.emitTickLo = (uint32_t)rb.frames; pe.emitTickHi = (uint32_t)(rb.frames >> 32);
  return rb.staged[f];
}

// The frame behind the end-of-tick launches: what they did not fold -- sorted draws, split flows, a budget beyond the block -- is emitted here (read-back on,
// plain order and a budget that fits the block: emission and staging are one launch; else emission or sort, bind runs, staging); the block is copied and published.
void enqueueFrame(ScTickContext* c, const DeviceState& ds, uint32_t flags, const FramePath& path)
{
  const uint32_t budget = c->desc.max_draws_budget;
  if ((flags & SC_TICK_DRAWS) && !path.stagedEmit && !path.foldEmit) {
    const uint32_t bound = (budget && budget < c->n) ? budget : c->n;
    if (flags & SC_TICK_SORT_DRAWS) {
      launchSortedDraws(ds, c->sort, budget, bound, c->dDraws, c->stream);
      if (flags & SC_TICK_BIND_RUNS) launchBindRuns(ds, c->sort, c->bind, bound, c->stream);      // the sorted keys are still in place
    } else launchEmitDraws(ds, budget, c->dDraws, c->stream);
  }
  if (!c->rb.bytes) return;
  ScTickContext::FrameReadback& rb = c->rb;
  const uint32_t f = frameSlot(rb);
  if (!path.stagedByEot) waitFrameBlock(c);             // (the end-of-tick kernel's launch waited already)
  bool binds = false;
  if (path.stagedEmit) {                                // (stagedByEot: the end-of-tick kernel wrote the block)
    if (!path.stagedByEot) launchEmitDrawsStaged(ds, budget, rb.dBlock[f], rb.maxVisible, rb.frames, c->stream, rb.staged[f]);      // (RunRecord::draws: the items lie in the block)
  } else {
    // (a flagged run is a sorted one, so it comes through here: its bind block is staged ahead of the frame's, whose `staged` covers both)
    binds = rb.bindBytes && (flags & SC_TICK_BIND_RUNS);
    if (binds) launchStageBinds(c->bind, rb.dBinds[f], c->stream);
    const uint32_t drawMode = (flags & SC_TICK_DRAWS) ? ((flags & SC_TICK_SORT_DRAWS) ? 2u : 1u) : 0u;
    launchStageFrame(ds, rb.dBlock[f], rb.maxVisible, rb.maxDraws, c->dDraws, drawMode, rb.frames, c->stream, rb.staged[f]);
  }
  // (`staged` rides on the staging dispatch: its completion signal, no marker packet on the tick queue)
  hipStreamWaitEvent(rb.copyStream, rb.staged[f], 0);
  hipMemcpyAsync(rb.hBlock[f], rb.dBlock[f], rb.bytes, hipMemcpyDeviceToHost, rb.copyStream);
  if (binds) hipMemcpyAsync(rb.hBinds[f], rb.dBinds[f], rb.bindBytes, hipMemcpyDeviceToHost, rb.copyStream);      // before `copied`
  publishFrame(c, binds);
}

// the tick's launches on c->stream, nothing else: safe inside a stream capture (the callers put waitParityFree before
// and publishPacked behind it).  Every per-tick decision comes from the plan; launches are timed only on an eager, sampled tick.
// Returns whether the `packed` event rode on the compaction + pack dispatch (publishPacked).
bool enqueueStages(ScTickContext* c, const TickPlan& plan, bool inCapture)
{
  const TickParams& p = plan.p;
  const FramePath& path = plan.path;
  const uint32_t flags = p.flags, grid = plan.grid;
  const DeviceState ds = stateFor(c, p.parity);
  const bool timing = !inCapture && plan.sampled;
  bool rode = false;
  if (c->producerKind && !(flags & SC_TICK_PRODUCE_NEXT)) {
    Scoped s(c, SC_TICK_K_NUDGE, timing);
    if (c->producerKind == 1) launchNudgeRootsX(ds, c->n, c->producerParam, c->stream);
    else launchAdvanceMovers(ds, c->n, c->producerParam, p.trafficSmooth, p.trafficMult, c->stream);
  }
  if (flags & (SC_TICK_XFORM | SC_TICK_CULL | SC_TICK_BROADPHASE)) {
    // the dominant kernel is timed by its own begin / end timestamps (the figure the roofline uses)
    // (a carrying tick's launch has the pending compaction at the head of its grid: the timestamps then include that role;
    //  planTick: a carrying or deferring tick is never a captured one)
    auto fused = [&](hipEvent_t evA, hipEvent_t evB) {
      if (!plan.carry) { launchXformCull(ds, p, grid, c->stream, evA, evB); return; }
      const ScTickContext::PendingCompact& pc = c->pending;
      launchXformCullCarry(ds, p, grid, pc.d, pc.p, pc.grid, pc.wideG, c->stream, evA, evB);
      c->pending.on = false;
      c->carryStats[1]++;
    };
    if (timed(c, SC_TICK_K_XFORM_CULL, timing)) {
      const EventPair ev = takeEvents(c);
      fused(ev.a, ev.b);
      c->times[SC_TICK_K_XFORM_CULL].push_back(ev);
    } else fused(nullptr, nullptr);
    if (p.homeMode == kHomeLearn) {
      // the slots handed out by the fused kernel are the remembered ones (the level kernels' and the neighbours' records reserve
      // behind them on every tick); the other copies of the bins start their next tick from the same counts
      launchSnapshotHome(ds, c->sectors, c->n, p.binSX, p.binSZ, (c->pairsStream && c->worldLayersKnown) ? 1u : 0u, c->worldLayers, p.fastPairs, c->stream);
      if (c->pairsStream)
        for (uint32_t q = 0; q < c->pipeDepth; ++q) {
          if (q == p.parity) continue;
          const DeviceState o = stateFor(c, q);
          hipMemcpyAsync(o.binCount, ds.homeCount, (size_t)c->sectors * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream);
          hipMemcpyAsync(o.binLayers, ds.homeLayers, (size_t)c->sectors * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream);
        }
    }
  }
  if (flags & kFlagHasDeep) {
    for (size_t lv = 0; lv + 1 < c->levelOffsets.size(); ++lv) {
      const uint32_t b = c->levelOffsets[lv], e = c->levelOffsets[lv + 1];
      launchDeepLevel(ds, p, c->dLevelList + b, e - b, c->stream);
    }
  }
  // the traffic AI's obstacle rays (scTickSetTrafficSensors): against this tick's boxes, before the frame producer moves the agents
  // (a tile with neighbours, stepped in order: the rays are cast in the pair half, behind the merge, where the neighbours' boxes are in
  //  the bins too -- raysInPairHalf(); here the agents are only listed with their rays as this frame has them)
  if ((flags & SC_TICK_BROADPHASE) && c->sensors && ds.aLane) {
    if (raysInPairHalf(c, flags)) launchAgentRaySnapshot(ds, p, c->stream);
    else launchAgentFrontRays(ds, p, c->stream);
  }
  if ((flags & SC_TICK_BROADPHASE) && (flags & SC_TICK_DENSE_AABBS)) launchDenseAabbs(ds, c->n, c->stream);   // read-back aid, off the hot path
  const bool exactRays = c->rayShapes == SC_TICK_RAY_SHAPES_EXACT;
  if (path.pairsNow && (flags & SC_TICK_RAYS)) launchRayQueries(ds, p, c->rays, exactRays, c->stream);      // the bins are full, not yet consumed
  if (path.pairsNow && (flags & SC_TICK_SWEEPS)) launchSweepQueries(ds, p, c->sweeps, exactSweepInfo(c), c->stream);
  // (overlap queries: scTickRun refuses them in a split flow, so this is their one launch site -- the pair half never sees the flag)
  if (path.pairsNow && (flags & kFlagOverlaps)) launchOverlapQueries(ds, p, c->overlaps, c->overlapShapes == SC_TICK_OVERLAP_SHAPES_EXACT, c->stream);
  // (trigger volumes: refused in a split flow like the overlap queries -- their one launch site; whether they run is the plan's word)
  if (plan.triggers) launchTriggerVolumes(ds, p, c->triggers, c->triggerShapes == SC_TICK_OVERLAP_SHAPES_EXACT, c->stream);
  // (entity-anchored sweeps: refused in a split flow too -- their one launch site, by the plan's word; their EXACT report has its own words)
  if (plan.anchoredSweeps)
    launchAnchoredSweeps(ds, p, c->asweeps, c->sweepShapes == SC_TICK_SWEEP_SHAPES_EXACT ? c->asweepInfo : nullptr, c->stream);
  // entity-anchored rays: resolved against the matrices the transform stage just left and cast in one launch; in a split flow they are
  // only resolved here, into this parity's snapshot -- the pair half casts them behind the merge, when a pipelined tile's matrices may
  // already be the next tick's
  if (flags & SC_TICK_ANCHORED_RAYS) {
    if (path.pairsNow) launchAnchoredRays(ds, p, anchoredFor(c, p.parity), false, exactRays, c->stream);
    else if (flags & SC_TICK_BROADPHASE) launchAnchoredRaySnapshot(ds, p, anchoredFor(c, p.parity), c->stream);
  }
  if (path.needCompact && path.pairsNow) {
    TickParams pe = p;
    const hipEvent_t done = path.foldEmit ? fillFoldEmit(c, path, pe) : nullptr;
    // both depend only on the fused kernel: one launch, workgroups split by role (timed as K_PAIRS, by the dispatch's own
    // begin / end timestamps like the fused kernel: no marker packets on the queue)
    if (timed(c, SC_TICK_K_PAIRS, timing)) {
      const EventPair ev = takeEvents(c);
      launchCompactPairs(ds, pe, grid, c->stream, ev.a, ev.b);
      c->times[SC_TICK_K_PAIRS].push_back(ev);
      if (done) hipEventRecord(done, c->stream);
    } else launchCompactPairs(ds, pe, grid, c->stream, nullptr, done);      // (`staged` rides on the dispatch: its completion signal)
    closePairHalf(c, ds, plan, c->stream);
  } else {
    const bool packToo = path.needCompact && (flags & SC_TICK_BROADPHASE) && (flags & SC_TICK_SPLIT_PAIRS);
    if (packToo) {
      Scoped s(c, SC_TICK_K_COMPACT, timing);
      // pipelined tile, eager: the `packed` event rides on the dispatch (publishPacked then only makes the pairs stream wait)
      rode = c->pairsStream && !inCapture && !s.on;
      launchCompactPack(ds, p, grid, c->stream, rode ? c->packed[p.parity] : nullptr);      // compaction and pack share a launch
    } else if (path.needCompact && plan.defer) {
      // deferred: the launch's arguments are kept, the next tick's fused launch carries it or settle() launches it
      ScTickContext::PendingCompact& pc = c->pending;
      pc.on = true; pc.d = ds; pc.p = p; pc.grid = grid; pc.wideG = plan.compactG;
      c->carryStats[0]++;
    } else if (path.needCompact) {
      // a quiet tick's end-of-tick kernel: timed in the slot of a broadphase tick's end-of-tick kernel, SC_TICK_K_PAIRS, and like it by the
      // dispatch's own begin / end timestamps (whoever reads that slot sees what the tick's second launch cost, whichever it was)
      if (plan.rec.quiet && timed(c, SC_TICK_K_PAIRS, timing)) {
        const EventPair ev = takeEvents(c);
        launchCompact(ds, p, grid, plan.compactG, c->stream, ev.a, ev.b);
        c->times[SC_TICK_K_PAIRS].push_back(ev);
      } else {
        Scoped s(c, SC_TICK_K_COMPACT, timing && !plan.rec.quiet);
        launchCompact(ds, p, grid, plan.compactG, c->stream);
      }
    }
    if (flags & SC_TICK_BROADPHASE) {
      if (flags & SC_TICK_SPLIT_PAIRS) {                                            // the caller exchanges, then scTickRunPairs
        if (!packToo) {
          launchBorderPack(ds, p, c->stream);
          if (flags & kFlagDeferredReset) launchResetParity(ds, p.resetParity, c->stream);      // (the fused launch does it itself)
        }
      }
      else {
        { Scoped s(c, SC_TICK_K_PAIRS, timing); launchPairs(ds, p, c->stream); }
        closePairHalf(c, ds, plan, c->stream);
      }
    }
  }
  enqueueFrame(c, ds, flags, path);
  return rode;
}

// drop captured graphs: every one of the array (the tick's: the quiet tick's too)
void dropGraphs(CapturedGraph* g, uint32_t count)
{
  for (uint32_t k = 0; k < count; ++k) {
    if (g[k].exec) { hipGraphExecDestroy(g[k].exec); g[k].exec = nullptr; }
    if (g[k].graph) { hipGraphDestroy(g[k].graph); g[k].graph = nullptr; }
  }
}
template <uint32_t N> void dropGraphs(CapturedGraph (&g)[N]) { dropGraphs(g, N); }
// ... every capture of the context: the tick's graphs and the pair half's (a pipelined tile's)
void dropCaptures(ScTickContext* c) { dropGraphs(c->graph); dropGraphs(c->pairGraph); }

// The key of a capture of this plan's tick, or of its pair half, as the context stands (rccl: the library's RCCL group goes inside)
GraphKey graphKey(const ScTickContext* c, const TickPlan& plan, bool rccl)
{
  GraphKey k;
  k.p = plan.p; k.epoch = c->topoEpoch; k.compactG = plan.compactG; k.visSel = plan.visSel; k.rccl = rccl;
  return k;
}

// Graph replay: launch g's graph on s, capturing it first when there is none or it was captured for another key (the RCCL group
// touches the communicator's own resources during capture, so a capture with it inside is relaxed).  body() enqueues the work on s; it
// returns 0 on an error whose text it has set.  what: the graph's name in the error texts.
template <typename Body>
int replayGraph(ScTickContext* c, hipStream_t s, CapturedGraph& g, const GraphKey& key, const char* what, Body body)
{
  if (!g.exec || !(g.key == key)) {
    dropGraphs(&g, 1);
    HIP_OK(c, hipStreamBeginCapture(s, key.rccl ? hipStreamCaptureModeRelaxed : hipStreamCaptureModeThreadLocal));
    const int ok = body();
    const hipError_t ce = hipStreamEndCapture(s, &g.graph);
    if (!ok) { if (g.graph) { hipGraphDestroy(g.graph); g.graph = nullptr; } return 0; }
    if (ce != hipSuccess) return fail(c, what, ce);
    if (!g.graph) return fail(c, (std::string(what) + " returned no graph (the capture was invalidated)").c_str());
    HIP_OK(c, hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
    g.key = key;
  }
  HIP_OK(c, hipGraphLaunch(g.exec, s));
  return 1;
}

void rowsToMat4(const float* r12, float* m16)
{
  // rows -> column-major Mat4 (m[c*4+r]); last row (0,0,0,1)
  for (int r = 0; r < 3; ++r) for (int col = 0; col < 4; ++col) m16[col * 4 + r] = r12[r * 4 + col];
  m16[3] = 0.0f; m16[7] = 0.0f; m16[11] = 0.0f; m16[15] = 1.0f;
}

// ---- shared steps of the C ABI's pair-half calls: one gate and one copy for the readers, one grow rule, one owner of the narrow-phase buffers ----
// The gate of every call that reads a result of the last scTickRun's pair half, in one order: that run carried `flag`; the feature was
// enabled at that run (enabledThen; features without such a state pass true); its pair half is not pending; the feature's buffers are
// still there (onNow; likewise); then the pairs stream is joined.  The call site passes the texts (nullptr where the check cannot fail).
bool lastRunResult(ScTickContext* c, uint32_t flag, const char* notRequested, bool enabledThen, const char* notEnabled, const char* pending,
                   bool onNow, const char* switchedOff)
{
  if (!(c->last.flags & flag)) return fail(c, notRequested);
  if (!enabledThen) return fail(c, notEnabled);
  if (c->pairsPending) return fail(c, pending);
  if (!onNow) return fail(c, switchedOff);
  return joinPairs(c);
}

// The stages of the touching pairs that are enabled now, as a NarrowStage set: a stage is on while its control words exist
uint32_t narrowOn(const ScTickContext* c)
{
  const NarrowPhase& np = c->narrow;
  return (np.list.ctl ? kStageList : 0u) | (np.contacts.ctl ? kStageContacts : 0u) | (np.manifolds.ctl ? kStageManifolds : 0u) |
         (np.islands.ctl ? kStageIslands : 0u) | (np.persist.ctl ? kStagePersist : 0u) | (np.sleep.ctl ? kStageSleep : 0u);
}

// The gate of the touching pairs' readers, one row per stage: its bit -- in LastWith::narrow "it ran then", in narrowOn "it is on now" --
// and its texts (the list always ran with its flag: no such text)
struct NarrowReader { uint32_t stage; const char *notEnabled, *pending, *switchedOff; };
const NarrowReader kNarrowReaders[] = {
  { kStageList, nullptr, "touching pairs are ready after scTickRunPairs", "touching pairs were switched off since the last scTickRun" },
  { kStageContacts, "pair contacts were not enabled at the last scTickRun (scTickSetPairContacts)", "pair contacts are ready after scTickRunPairs", "pair contacts were switched off since the last scTickRun" },
  { kStageManifolds, "pair manifolds were not enabled at the last scTickRun (scTickSetPairManifolds)", "pair manifolds are ready after scTickRunPairs", "pair manifolds were switched off since the last scTickRun" },
  { kStageIslands, "pair islands were not enabled at the last scTickRun (scTickSetPairIslands)", "pair islands are ready after scTickRunPairs", "pair islands were switched off since the last scTickRun" },
  { kStagePersist, "pair persistence was not enabled at the last scTickRun (scTickSetPairPersistence)", "pair persistence is ready after scTickRunPairs", "pair persistence was switched off since the last scTickRun" },
  { kStageSleep, "pair sleep was not enabled at the last scTickRun (scTickSetPairSleep)", "pair sleep is ready after scTickRunPairs", "pair sleep was switched off since the last scTickRun" },
};
bool narrowResult(ScTickContext* c, uint32_t stage)
{
  for (const NarrowReader& r : kNarrowReaders)
    if (r.stage == stage)
      return bind(c) && lastRunResult(c, SC_TICK_PAIR_SHAPES, "the last scTickRun did not request SC_TICK_PAIR_SHAPES",
                                      !r.notEnabled || (c->lastWith.narrow & stage) != 0u, r.notEnabled, r.pending, (narrowOn(c) & stage) != 0u, r.switchedOff);
  return false;
}

// ... and what most of them do next: the report, then the first min(the report's count, what the device keeps, the caller's room) records
template <typename Info>
bool readReportAndRecords(ScTickContext* c, Info* info, const uint32_t* devInfo, uint32_t Info::*count, uint32_t kept, const void* devRec,
                          size_t recBytes, void* out, uint32_t capacity)
{
  if (!d2h(c, info, devInfo, sizeof *info) || !sync(c)) return false;
  const uint32_t m = std::min(std::min(info->*count, kept), out ? capacity : 0u);
  return !m || (d2h(c, out, devRec, (size_t)m * recBytes) && sync(c));
}

// One array of a query batch: the state's pointer to it, its elements per query, whether it starts out as zeros.
template <typename T> struct BatchArray { T*& p; size_t per; bool zero; };
template <typename T> BatchArray<T> batchArray(T*& p, bool zero = false, size_t per = 1) { return { p, per, zero }; }

// The grow rule of the query batches (rays, sweeps, anchored rays), for a batch of `count` queries behind a sync.  A count within the
// capacity keeps the arrays; a larger one frees every array and allocates them anew for max(count, 1 024) queries.  One failure path: the
// batch is left empty (held 0) with capacity 0, the epoch where it was.  A call that succeeds moves the epoch whether it grew the arrays
// or not: a captured frame holds the old batch size -- and the next broadphase tick is a learn tick.
template <typename... T>
bool growBatch(ScTickContext* c, uint32_t& cap, uint32_t& held, uint32_t count, BatchArray<T>... arrays)
{
  if (count > cap) {
    auto drop = [&](auto& a) { dfree(c, const_cast<void*>(static_cast<const void*>(a.p))); a.p = nullptr; };      // (inputs are pointers to const)
    (drop(arrays), ...);
    cap = 0; held = 0;
    const uint32_t want = std::max(count, 1024u);
    if (!(dalloc(c, arrays.p, want * arrays.per, arrays.zero) && ...)) { (drop(arrays), ...); return false; }
    cap = want;
  }
  held = count;
  c->topoEpoch++;
  return true;
}

// ---- the narrow phase's buffers.  What the caller wants of them is ONE record: every setter's arguments as the context holds them.
// narrowWanted reads the current record off the context; a setter changes its own fields and hands the record to sizeNarrowPhase, the
// one place that sizes the six stages and the one that writes the caller's parameters into their states.
struct NarrowWant {
  uint32_t maxTouching = 0;            // the list's entries; 0: everything off
  bool contacts = false, manifolds = false, islands = false, persist = false;
  uint32_t fixedGroups = 0;            // islands
  float matchDist = 0.0f;              // persistence
  uint32_t sleepEvents = 0;            // sleep: its max_events; 0: off
  float linTol = 0.0f, angTol = 0.0f; uint32_t restRuns = 0;
};
NarrowWant narrowWanted(const ScTickContext* c)
{
  const NarrowPhase& np = c->narrow;
  const uint32_t on = narrowOn(c);
  NarrowWant w;                        // (a stage that is off holds zeros)
  w.maxTouching = np.list.maxTouching;
  w.contacts = (on & kStageContacts) != 0u; w.manifolds = (on & kStageManifolds) != 0u; w.islands = (on & kStageIslands) != 0u; w.persist = (on & kStagePersist) != 0u;
  w.fixedGroups = np.islands.fixedGroups; w.matchDist = np.persist.matchDist;
  w.sleepEvents = np.sleep.maxEvents; w.linTol = np.sleep.linTol; w.angTol = np.sleep.angTol; w.restRuns = np.sleep.restRuns;
  return w;
}

// One level freed, all null: what a level that goes off, one that is allocated afresh and a failed allocation all go through
template <typename State, typename... P> void freeLevel(ScTickContext* c, State& s, P*... allocations) { (dfree(c, allocations), ...); s = State{}; }
template <typename State, typename Rec> void freeNarrowLevel(ScTickContext* c, State& s, Rec* State::*rec) { freeLevel(c, s, s.*rec, s.ctl, s.info); }
void freeIslandLevel(ScTickContext* c) { PairIslandState& s = c->narrow.islands; freeLevel(c, s, s.edge, s.ctl, s.info, s.parent, s.labels, s.partial); }
void freePersistLevel(ScTickContext* c)
{
  PairPersistState& s = c->narrow.persist;
  freeLevel(c, s, s.rec, s.ctl, s.info, s.partial, s.local[0], s.local[1], s.payload[0], s.payload[1]);
}
void freeSleepLevel(ScTickContext* c) { PairSleepState& s = c->narrow.sleep; freeLevel(c, s, s.ctl, s.info, s.fell, s.woke, s.partial); }

// One level allocated afresh for `entries` entries of the list (0: freed, nothing allocated); a failure leaves what it allocated in the
// state, and sizeNarrowPhase frees every level.  The list, the contacts and the manifolds: control words, a report, recsPer records per entry.
template <typename State, typename Rec>
bool sizeNarrowLevel(ScTickContext* c, State& s, Rec* State::*rec, uint32_t ctlWords, uint32_t infoWords, uint32_t recsPer, uint32_t entries)
{
  freeNarrowLevel(c, s, rec);
  if (!entries) return true;
  if (!dalloc(c, s.ctl, ctlWords) || !dalloc(c, s.info, infoWords) || !dalloc(c, s.*rec, (size_t)recsPer * entries, false)) return false;
  s.maxTouching = entries;
  return true;
}

// The islands: an island word per entry, and the union-find's two words per entity of the context's capacity
bool sizeIslandLevel(ScTickContext* c, uint32_t entries)
{
  PairIslandState& s = c->narrow.islands;
  freeIslandLevel(c);
  if (!entries) return true;
  if (!dalloc(c, s.ctl, kPiCtlWords) || !dalloc(c, s.info, kPiInfoWords) || !dalloc(c, s.edge, entries, false) || !dalloc(c, s.parent, c->cap) ||
      !dalloc(c, s.labels, c->cap) || !dalloc(c, s.partial, 4u * kPiMaxBlocks)) return false;
  s.maxTouching = entries; s.cap = c->cap;
  return true;
}

// Persistence: a record per entry, two sides of local points (with ages and counts) and payload rows per entry, and one slab of control
// words and both sides' tables, which a resync zeroes as a whole
bool sizePersistLevel(ScTickContext* c, uint32_t entries)
{
  PairPersistState& s = c->narrow.persist;
  freePersistLevel(c);
  if (!entries) return true;
  uint64_t slots = 64u;
  while (slots < 2ull * entries) slots <<= 1;
  if (slots > (1ull << 31)) return fail(c, "pair persistence: max_touching is too large for its tables");
  // [control words][key 0][key 1][value 0][value 1]: the keys 8-byte aligned behind 64 bytes of control words
  const size_t words = (size_t)kPpCtlWords + 2u * 2u * (size_t)slots + 2u * (size_t)slots;
  bool ok = dalloc(c, s.ctl, words) && dalloc(c, s.info, kPpInfoWords) && dalloc(c, s.rec, entries) && dalloc(c, s.partial, 4u * kPpMaxBlocks);
  for (int k = 0; k < 2 && ok; ++k) ok = dalloc(c, s.local[k], 4u * (size_t)entries) && dalloc(c, s.payload[k], 4u * (size_t)entries);
  if (!ok) return false;
  s.key[0] = reinterpret_cast<unsigned long long*>(s.ctl + kPpCtlWords); s.key[1] = s.key[0] + slots;
  s.val[0] = reinterpret_cast<uint32_t*>(s.key[1] + slots); s.val[1] = s.val[0] + slots;
  s.slots = (uint32_t)slots; s.slabBytes = words * sizeof(uint32_t);
  s.maxTouching = entries;
  return true;
}

// Sleep: one slab -- control words, a state word and an awake word per entity of the context's capacity, three anchor rows per entity --,
// which a resync zeroes as a whole; the two event lists, the report and the resolve's tallies
bool sizeSleepLevel(ScTickContext* c, uint32_t entries, uint32_t maxEvents)
{
  PairSleepState& s = c->narrow.sleep;
  freeSleepLevel(c);
  if (!entries) return true;
  // [control words][state][awake][anchor]: the anchor rows 16-byte aligned behind 64 bytes of control words and 2 * cap words (cap is a multiple of the tile)
  const size_t words = (size_t)kPzCtlWords + 2u * (size_t)c->cap + 12u * (size_t)c->cap;
  if (!dalloc(c, s.ctl, words) || !dalloc(c, s.info, kPzInfoWords) || !dalloc(c, s.fell, maxEvents) || !dalloc(c, s.woke, maxEvents) ||
      !dalloc(c, s.partial, 4u * kPzMaxBlocks)) return false;
  s.state = s.ctl + kPzCtlWords; s.awake = s.state + c->cap; s.anchor = reinterpret_cast<float4*>(s.awake + c->cap);
  s.slabBytes = words * sizeof(uint32_t);
  s.cap = c->cap; s.maxTouching = entries; s.maxEvents = maxEvents;
  return true;
}

// Make the context match `want`; `level` is the stage the calling setter sets.  Dependencies are settled here, once: nothing without the
// list, no manifolds without contacts, no persistence without manifolds, no sleep without islands.  The list, contacts, manifolds and
// islands are allocated afresh when the setter sets them or the list is allocated afresh, freed when they have to be off, and otherwise
// left alone.  Persistence and sleep hold a memory: allocated afresh -- a resync -- only when the list's size (sleep: or max_events)
// differs from theirs.  Then the caller's parameters are written from the record, zero where a stage is off.  A failed allocation leaves
// all six off (the allocator's text stands): nothing is ever on without what it needs, or sized for another list.
enum NarrowLevel { kNarrowList, kNarrowContacts, kNarrowManifolds, kNarrowIslands, kNarrowPersist, kNarrowSleep };
bool sizeNarrowPhase(ScTickContext* c, NarrowLevel level, const NarrowWant& want)
{
  NarrowPhase& np = c->narrow;
  NarrowWant w = want;
  w.contacts = w.contacts && w.maxTouching; w.islands = w.islands && w.maxTouching;
  w.manifolds = w.manifolds && w.contacts; w.persist = w.persist && w.manifolds;
  if (!w.islands) w.sleepEvents = 0u;
  const uint32_t m = w.maxTouching, persistEntries = w.persist ? m : 0u, sleepEntries = w.sleepEvents ? m : 0u;
  const bool list = level == kNarrowList;
  bool ok = true;
  if (list) ok = sizeNarrowLevel(c, np.list, &PairShapeState::list, kPsCtlWords, kPsInfoWords, 1u, m);
  if (ok && (list || level == kNarrowContacts || !w.contacts)) ok = sizeNarrowLevel(c, np.contacts, &PairContactState::rec, kPcCtlWords, kPcInfoWords, 2u, w.contacts ? m : 0u);
  if (ok && (list || level == kNarrowManifolds || !w.manifolds)) ok = sizeNarrowLevel(c, np.manifolds, &PairManifoldState::rec, kPmCtlWords, kPmInfoWords, 5u, w.manifolds ? m : 0u);
  if (ok && (list || level == kNarrowIslands || !w.islands)) ok = sizeIslandLevel(c, w.islands ? m : 0u);
  if (ok && persistEntries != np.persist.maxTouching) ok = sizePersistLevel(c, persistEntries);
  if (ok && (sleepEntries != np.sleep.maxTouching || w.sleepEvents != np.sleep.maxEvents)) ok = sizeSleepLevel(c, sleepEntries, w.sleepEvents);
  if (!ok) {
    freeNarrowLevel(c, np.list, &PairShapeState::list); freeNarrowLevel(c, np.contacts, &PairContactState::rec); freeNarrowLevel(c, np.manifolds, &PairManifoldState::rec);
    freeIslandLevel(c); freePersistLevel(c); freeSleepLevel(c);
    return false;
  }
  np.islands.fixedGroups = w.islands ? w.fixedGroups : 0u;
  np.persist.matchDist = w.persist ? w.matchDist : 0.0f;
  const bool sleep = w.sleepEvents != 0u;
  np.sleep.linTol = sleep ? w.linTol : 0.0f; np.sleep.angTol = sleep ? w.angTol : 0.0f; np.sleep.restRuns = sleep ? w.restRuns : 0u;
  return true;
}

} // namespace

extern "C" {

uint32_t scTickGetApiVersion(void) { return SC_TICK_API_VERSION; }

const char* scTickGetLastError(const ScTickContext* ctx) { return ctx ? ctx->err.c_str() : gCreateError.c_str(); }

ScTickContext* scTickCreateContext(const ScTickContextDesc* desc)
{
  if (!desc) { fail(nullptr, "null desc"); return nullptr; }
  if (desc->capacity == 0 || desc->capacity > SC_TICK_MAX_ENTITIES) { fail(nullptr, "capacity must be 1..2^24-1"); return nullptr; }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) { fail(nullptr, "no HIP device available (libsc_tick needs an AMD GPU; there is no CPU fallback)", e); return nullptr; }
  if (desc->device_ordinal < 0 || desc->device_ordinal >= count) { fail(nullptr, "device ordinal out of range"); return nullptr; }

  // SC_TICK_VARIANT: the four A/B switches that remain (include/sc_tick.h); any other bit names a retired experiment
  const char* vs = std::getenv("SC_TICK_VARIANT");
  const uint32_t variant = vs ? (uint32_t)std::atoi(vs) : 0u;
  if (variant & ~(2u | 8u | 16u | 32u)) { fail(nullptr, "SC_TICK_VARIANT: only bits 1 (2, home slots off) and 5 (32, lazy records off) and 3 (8, quiet ticks off) and 4 (16, one compaction workgroup per span) remain"); return nullptr; }

  ScTickContext* c = new ScTickContext();
  c->desc = *desc;
  c->device = desc->device_ordinal;
  if (c->desc.sector_size <= 0.001f) c->desc.sector_size = 64.0f;     // WorldPartition::configure, sc_world_partition.cpp:222-223
  c->cap = ((desc->capacity + kTile - 1) / kTile) * kTile;
  if (const char* s = std::getenv("SC_TICK_SPANS")) { const int v = std::atoi(s); if (v > 0) c->spansWanted = (uint32_t)v; }
  if (const char* s = std::getenv("SC_TICK_COMPACT_G")) { const int v = std::atoi(s); if (v > 0) c->compactForceG = (uint32_t)v; }
  if (const char* s = std::getenv("SC_TICK_TAIL")) c->tailEnabled = std::atoi(s) != 0;      // A/B switch: 0 keeps the dirty clear and the root nudge in the end-of-tick kernel
  if (const char* s = std::getenv("SC_TICK_TOPO_CLASSES")) c->topoEnabled = std::atoi(s) != 0;      // A/B switch: 0 never takes the classed instance of the fused kernel
  if (const char* s = std::getenv("SC_TICK_CARRY")) c->carryEnabled = std::atoi(s) != 0;            // A/B switch: 0 never defers a compaction (every tick launches its own)

  bool ok = bind(c);
  if (ok) {
    int cu = 0;
    if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && cu > 0) c->cus = (uint32_t)cu;
    else c->cus = 256u;                                   // MI355X
  }
  if (ok) {
    // (keeping compute units out of the tick stream's reach with a CU mask, so that the RCCL kernel of the pair half finds
    //  free ones at once, was measured: 124-232 us per step against 89 -- masked queues schedule badly here)
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) ok = fail(c, "hipStreamCreate", e);
    c->ownStream = c->stream;
  }
  DeviceState& d = c->d;
  const size_t N = c->cap;
  // one slab for every 4-byte stream, one for the matrix rows (see Stream in sc_tick_internal.h)
  // The streams' PITCH, in entries: cap + SC_TICK_STREAM_PAD (at creation; rounded up to a multiple of 64, at most 65536; default 0).  With
  // the default, neighbouring streams lie a power of two apart wherever the capacity is one; the pad is there to measure whether that
  // costs anything (part B).  Every kernel addresses stream k at k * capBytes, every copy goes through the
  // per-stream pointers below, and every stream is used up to cap entries only.
  size_t P = N;
  if (const char* s = std::getenv("SC_TICK_STREAM_PAD")) { const int v = std::atoi(s); if (v > 0) P = N + (size_t)std::min((v + 63) / 64 * 64, 65536); }
  float* fslab = nullptr; float4* rslab = nullptr;
  ok = ok && dalloc(c, fslab, (size_t)kStreamCount * P) && dalloc(c, rslab, 3 * P);
  if (ok) {
    auto F = [&](uint32_t k) { return fslab + (size_t)k * P; };
    d.fslab = reinterpret_cast<const char*>(fslab); d.rslab = reinterpret_cast<char*>(rslab);
    d.capBytes = (uint32_t)(P * 4u); d.capBytes16 = (uint32_t)(P * 16u);
    d.px = F(kPX); d.py = F(kPY); d.pz = F(kPZ);
    d.rsx = F(kRSX); d.rcx = F(kRCX); d.rsy = F(kRSY); d.rcy = F(kRCY); d.rsz = F(kRSZ); d.rcz = F(kRCZ);
    d.sx = F(kSX); d.sy = F(kSY); d.sz = F(kSZ);
    d.bminx = F(kBMINX); d.bminy = F(kBMINY); d.bminz = F(kBMINZ); d.bmaxx = F(kBMAXX); d.bmaxy = F(kBMAXY); d.bmaxz = F(kBMAXZ);
    d.link = reinterpret_cast<uint32_t*>(F(kLINK)); d.layers = reinterpret_cast<uint32_t*>(F(kLAYERS));
    d.meshId = reinterpret_cast<uint32_t*>(F(kMESH)); d.materialId = reinterpret_cast<uint32_t*>(F(kMATERIAL));
    d.w0 = rslab; d.w1 = rslab + P; d.w2 = rslab + 2 * P;
  }
  ok = ok && dalloc(c, d.dirty, N / 32) && dalloc(c, d.unreach, N / 32) && dalloc(c, d.rootMask, N / 32)
          && dalloc(c, d.vis, N / 64) && dalloc(c, d.cand, N / 64) && dalloc(c, d.recomp, N / 64)
          && dalloc(c, d.blockVis, N / kTile) && dalloc(c, d.blockCand, N / kTile)
          && dalloc(c, d.visibleIdx, N) && dalloc(c, d.culledIdx, N) && dalloc(c, d.counters, kCounterWords)
          && dalloc(c, d.aabbMin, N) && dalloc(c, d.aabbMax, N);
  // the second copy of what a carried compaction reads while the carrying tick writes (131 KB + 16 KB at 1M entities)
  ok = ok && dalloc(c, c->visAlt[0], N / 64) && dalloc(c, c->visAlt[1], N / 64) && dalloc(c, c->blockAlt[0], N / kTile) && dalloc(c, c->blockAlt[1], N / kTile);
  { float* f = nullptr; ok = ok && dalloc(c, f, 32); d.frustum = f; }
  {
    // bounds classes: both tables at their full size from the start, so that their pointers never change under a captured graph,
    // in ONE allocation, the tile words behind the palette: the fused kernel addresses both from one pointer (a second one held
    // in SGPRs across the tile cost its cull-only instances a wave per SIMD).  Every wave-tile starts out as "nobody has Bounds"
    // (and the topology classes' pattern table in front of the palette: topoTable())
    float* pal = nullptr;
    ok = ok && dalloc(c, pal, (size_t)kTopoCap * 128u + (size_t)kPaletteCap * 8u + N / 64 * 2);
    if (pal) pal += (size_t)kTopoCap * 128u;
    uint32_t* tc = pal ? reinterpret_cast<uint32_t*>(pal) + (size_t)kPaletteCap * 8u : nullptr;
    d.boundsPalette = pal; d.tileClass = tc;
    c->hPalette.assign((size_t)kPaletteCap * 8u, 0u);
    c->hTile.assign(N / 64 * 2, 0u);
    c->hTopo.assign(N / 64, (uint16_t)0);
    for (size_t t = 0; t < N / 64; ++t) c->hTile[2 * t] = kClassMixed | kTileNoBounds | kTileLayersShared;
    ok = ok && h2d(c, tc, c->hTile.data(), c->hTile.size() * sizeof(uint32_t)) && sync(c);
  }
  c->sectors = desc->tile_sectors_x ? (desc->tile_sectors_x + 2u) * (desc->tile_sectors_z + 2u) : 0u;
  c->maxPairs = desc->max_pairs ? desc->max_pairs : desc->capacity * 4u;
  c->maxPairs = ((c->maxPairs + kPairShards - 1u) / kPairShards) * kPairShards;   // equal shard segments
  if (ok && c->sectors) {
    if ((uint64_t)desc->tile_sectors_x * desc->tile_sectors_z > (1u << 24) || desc->tile_sectors_x > 65533u || desc->tile_sectors_z > 65533u)
      ok = fail(c, "tile rectangle too large");           // (the pair search carries a sector's grid coordinates as 16 + 16 bits)
    ok = ok && dalloc(c, d.binCount, c->sectors) && dalloc(c, d.binLayers, c->sectors) && dalloc(c, d.bins, (size_t)c->sectors * kBinCap * 2u, false)
            && dalloc(c, d.bigList, (N + 8u * kBorderBigCap) * 2u, false) && dalloc(c, d.spill, 2u * (size_t)ovfRecords(c), false) && dalloc(c, d.spillSector, ovfRecords(c))
            && dalloc(c, d.crowdQueue, (size_t)kMaxParity * c->sectors)
            && dalloc(c, d.ovfIdx, (size_t)kOvfWaves * kOvfPerSector, false) && dalloc(c, d.ovfLo, c->sectors, false) && dalloc(c, d.ovfHi, c->sectors)
            && dalloc(c, d.pairs, c->maxPairs, false) && dalloc(c, d.pairShardCount, (kMaxParity + 1u) * kPairShards * kShardStride)
            && dalloc(c, c->dPairsOut, c->maxPairs, false) && dalloc(c, c->dPairTotal, 4)
            && dalloc(c, d.homeA, N, false) && dalloc(c, d.homeB, N, false) && dalloc(c, d.homeCount, c->sectors) && dalloc(c, d.homeLayers, c->sectors) && dalloc(c, d.lazyCtl, 1u + 2u * kMaxParity)
            && dalloc(c, d.homeCast, c->sectors) && dalloc(c, d.homePerm, (size_t)c->sectors * kBinCap);
    if (ok) { e = hipMemset(d.homeA, 0xFF, N * sizeof(uint32_t)); if (e == hipSuccess) e = hipMemset(d.homeB, 0xFF, N * sizeof(uint32_t)); if (e != hipSuccess) ok = fail(c, "hipMemset", e); }
  }
  if (ok && c->sectors) {
    float4* nr = nullptr;
    ok = dalloc(c, nr, 2);
    if (ok) {
      const uint32_t inf = 0x7F800000u, ninf = 0xFF800000u;
      const uint32_t words[8] = { inf, inf, inf, 0u, ninf, ninf, ninf, 0x00FFFFFFu };      // nullRecord() in sc_tick_kernels.hip
      ok = h2d(c, nr, words, sizeof words) && sync(c);
      d.nullRec = nr;
    }
    // the pair role's constant tables (sc_tick_kernels.hip: pairsBody's prologue copies them into LDS)
    uint32_t* pc = nullptr;
    ok = ok && dalloc(c, pc, kPairConstWords);
    if (ok) {
      std::vector<uint32_t> words(kPairConstWords, 0u);
      uint16_t* tab = reinterpret_cast<uint16_t*>(words.data());
      for (uint32_t i = 1; i < kBinCap; ++i)
        for (uint32_t j = 0; j < i; ++j) tab[i * (i - 1u) / 2u + j] = (uint16_t)(i << 8 | j);
      for (uint32_t t = 1; t <= kBinCap; ++t) { const uint32_t G = 64u / t; words[kPairConstCast + t] = G | ((65536u / G + 1u) << 8); }
      ok = h2d(c, pc, words.data(), words.size() * sizeof(uint32_t)) && sync(c);
      d.pairConst = pc;
    }
  }
  if (variant & 32u) c->lazyEnabled = false;            // SC_TICK_VARIANT bit 5: every remembered slot is written on every tick (A/B)
  if (variant & 2u) c->homeEnabled = false;             // SC_TICK_VARIANT bit 1: every record reserves its slot on every tick (A/B)
  if (variant & 16u) c->wideCompact = false;            // SC_TICK_VARIANT bit 4: the end-of-tick kernel alone keeps one workgroup per span, compactBody's form (A/B)
  if (variant & 8u) c->quietEnabled = false;            // SC_TICK_VARIANT bit 3: a tick whose bins nobody reads fills and sweeps them all the same (A/B)
  if (const char* fp = std::getenv("SC_TICK_FAST_PAIRS")) c->fastPairs = std::atoi(fp) != 0;      // 0: every bin goes through the general pair search (A/B)
  if (const char* hp = std::getenv("SC_TICK_HOME_PERIOD")) { const int v = std::atoi(hp); if (v > 0) c->homePeriod = (uint32_t)v; }
  if (ok && c->sectors) { e = hipMemset(d.ovfLo, 0xFF, (size_t)c->sectors * sizeof(uint32_t)); if (e != hipSuccess) ok = fail(c, "hipMemset", e); }
  if (ok) { void* p = nullptr; e = hipMalloc(&p, N * sizeof(ScTickDrawItem)); if (e != hipSuccess) ok = fail(c, "hipMalloc draws", e); else { c->allocs.push_back(p); c->dDraws = p; } }
  if (ok) {
    // Transform{}: worldMatrix = identity, scale = 1, cos = 1 (sc_ecs.h:63-71)
    std::vector<float> ones(N, 1.0f);
    std::vector<float4> e0(N, make_float4(1, 0, 0, 0)), e1(N, make_float4(0, 1, 0, 0)), e2(N, make_float4(0, 0, 1, 0));
    ok = h2d(c, d.sx, ones.data(), N * 4) && h2d(c, d.sy, ones.data(), N * 4) && h2d(c, d.sz, ones.data(), N * 4)
      && h2d(c, d.rcx, ones.data(), N * 4) && h2d(c, d.rcy, ones.data(), N * 4) && h2d(c, d.rcz, ones.data(), N * 4)
      && h2d(c, d.w0, e0.data(), N * 16) && h2d(c, d.w1, e1.data(), N * 16) && h2d(c, d.w2, e2.data(), N * 16) && sync(c);
  }
  if (!ok) { gCreateError = c->err; scTickDestroyContext(c); return nullptr; }
  c->hParent.assign(desc->capacity, SC_TICK_NO_PARENT);
  c->hFlags.assign(desc->capacity, 0);
  c->hClass.assign(desc->capacity, (uint16_t)kClassNone);
  c->hLayers.assign(desc->capacity, 0u);               // (as the device stream starts out)
  c->hChildren.assign(desc->capacity, 0);
  c->hFirstChild.assign(desc->capacity, -1); c->hNextSib.assign(desc->capacity, -1); c->hPrevSib.assign(desc->capacity, -1);
  return c;
}

void scTickDestroyContext(ScTickContext* c)
{
  if (!c) return;
  hipSetDevice(c->device);
  c->pending.on = false;                               // (a pending compaction has no reader left: dropped)
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->pairsStream) hipStreamSynchronize(c->pairsStream);
  c->stream = c->ownStream;
  dropGraphs(c->graph); dropGraphs(c->pairGraph);      // (teardown keeps its text word for word, this line included: DESIGN.md section 6)
  for (auto& v : c->times) for (auto& p : v) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
  for (auto& p : c->eventPool) { hipEventDestroy(p.a); hipEventDestroy(p.b); }
  for (uint32_t k = 0; k < kMaxParity; ++k) { if (c->packed[k]) hipEventDestroy(c->packed[k]); if (c->pairsDone[k]) hipEventDestroy(c->pairsDone[k]); }
  if (c->rb.copyStream) {
    hipStreamSynchronize(c->rb.copyStream);
    for (int k = 0; k < 2; ++k) { if (c->rb.hBinds[k]) hipHostFree(c->rb.hBinds[k]); if (c->rb.hBlock[k]) hipHostFree(c->rb.hBlock[k]); if (c->rb.staged[k]) hipEventDestroy(c->rb.staged[k]); if (c->rb.copied[k]) hipEventDestroy(c->rb.copied[k]); }
    hipStreamDestroy(c->rb.copyStream);
  }
  if (c->pairsStream) hipStreamSynchronize(c->pairsStream);
  if (c->comm) { std::string why; if (const RcclApi* r = rccl(&why)) r->CommDestroy(c->comm); c->comm = nullptr; }
  for (void* p : c->allocs) hipFree(p);
  if (c->ownPairsStream) hipStreamDestroy(c->ownPairsStream);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
}

int scTickSetEntityCount(ScTickContext* c, uint32_t count)
{
  if (!c) return 0;
  if (count > c->desc.capacity) return fail(c, "count exceeds capacity");
  REFUSE_WHILE_SHAPES_PENDING(c, "scTickSetEntityCount");
  const uint32_t before = c->n;
  c->n = count;
  c->linksStale = true;
  if (before == count) return 1;
  if (!bind(c)) return 0;
  if (count > before && !resetColliders(c, before, count - before)) return 0;      // new indices start without a collider of their own
  if (count < before && !resyncPairEvents(c)) return 0;                            // remembered pairs may name indices that are gone
  // the wave-tiles that gained or lost entities (bounds classes: lanes at or past n are not part of a tile)
  if (!refreshTiles(c, std::min(before, count), std::max(before, count))) return 0;
  return sync(c) ? 1 : 0;
}

int scTickUploadLocals(ScTickContext* c, uint32_t first, uint32_t count, const float* pos3, const float* rot3,
                       const float* scale3, uint8_t* repaired)
{
  if (!c || !pos3 || !rot3 || !scale3) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!count) return 1;
  std::vector<float> s[6], k(3 * (size_t)count);
  for (auto& v : s) v.resize(count);
  for (uint32_t i = 0; i < count; ++i) {
    // host libm, float overloads -- what std::sin/std::cos resolve to in mat4_rotation_xyz
    s[0][i] = std::sin(rot3[3 * i]);     s[1][i] = std::cos(rot3[3 * i]);
    s[2][i] = std::sin(rot3[3 * i + 1]); s[3][i] = std::cos(rot3[3 * i + 1]);
    s[4][i] = std::sin(rot3[3 * i + 2]); s[5][i] = std::cos(rot3[3 * i + 2]);
    float a = scale3[3 * i], b = scale3[3 * i + 1], z = scale3[3 * i + 2];
    const bool rep = (a == 0.0f && b == 0.0f && z == 0.0f);          // sc_ecs.cpp:143-149
    if (rep) { a = b = z = 1.0f; }
    if (repaired) repaired[i] = rep ? 1 : 0;
    k[3 * (size_t)i] = a; k[3 * (size_t)i + 1] = b; k[3 * (size_t)i + 2] = z;
    // an axis whose sin/cos came out as exactly (0, 1) need not be streamed by the kernels (link-word flag)
    const uint8_t triv = (uint8_t)(((s[0][i] == 0.0f && s[1][i] == 1.0f) ? 4u : 0u) | ((s[2][i] == 0.0f && s[3][i] == 1.0f) ? 8u : 0u) |
                                   ((s[4][i] == 0.0f && s[5][i] == 1.0f) ? 16u : 0u));
    uint8_t& f = c->hFlags[first + i];
    const uint8_t want = (f & 32u) ? (uint8_t)(triv & ~8u) : triv;       // traffic agents: the device rewrites their yaw -- Y is always streamed
    if ((f & 28u) != want) { f = (uint8_t)((f & ~28u) | want); c->linksStale = true; }
  }
  DeviceState& d = c->d;
  float* dst[6] = { d.rsx, d.rcx, d.rsy, d.rcy, d.rsz, d.rcz };
  for (int q = 0; q < 6; ++q) if (!h2d(c, dst[q] + first, s[q].data(), (size_t)count * 4u)) return 0;
  if (!upload3(c, pos3, first, count, d.px, d.py, d.pz)) return 0;
  if (!upload3(c, k.data(), first, count, d.sx, d.sy, d.sz)) return 0;
  launchSetDirtyRange(d, first, count, c->stream);
  return sync(c) ? 1 : 0;
}

int scTickUploadPositions(ScTickContext* c, uint32_t first, uint32_t count, const float* pos3)
{
  if (!c || !pos3) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!count) return 1;
  if (!upload3(c, pos3, first, count, c->d.px, c->d.py, c->d.pz)) return 0;
  launchSetDirtyRange(c->d, first, count, c->stream);
  return sync(c) ? 1 : 0;
}

int scTickUploadBounds(ScTickContext* c, uint32_t first, uint32_t count, const float* min3, const float* max3, const uint8_t* has)
{
  if (!c || !min3 || !max3) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!count) return 1;
  c->boxesTouched = true;
  if (!upload3(c, min3, first, count, c->d.bminx, c->d.bminy, c->d.bminz)) return 0;
  if (!upload3(c, max3, first, count, c->d.bmaxx, c->d.bmaxy, c->d.bmaxz)) return 0;
  for (uint32_t i = 0; i < count; ++i) {
    uint8_t& f = c->hFlags[first + i];
    const uint8_t nf = (uint8_t)((f & ~2u) | ((!has || has[i]) ? 2u : 0u));
    if (nf != f) { f = nf; c->linksStale = true; }          // link words only change when membership does
  }
  // bounds classes, behind the streams they are derived from: the class of every uploaded box (a run of equal boxes is looked
  // up once), then the wave-tiles of the range
  {
    const uint32_t paletteWas = (uint32_t)c->paletteIndex.size();
    BoxKey prev{}; uint32_t prevClass = kClassNone; bool havePrev = false;
    for (uint32_t i = 0; i < count; ++i) {
      BoxKey k;
      std::memcpy(k.w, min3 + 3 * (size_t)i, 12); std::memcpy(k.w + 3, max3 + 3 * (size_t)i, 12);
      if (!havePrev || !(k == prev)) { prevClass = classOfBox(c, k); prev = k; havePrev = true; }
      c->hClass[first + i] = (uint16_t)prevClass;
    }
    if (!uploadPalette(c, paletteWas) || !refreshTiles(c, first, first + count)) return 0;
  }
  return sync(c) ? 1 : 0;
}

int scTickUploadColliders(ScTickContext* c, uint32_t first, uint32_t count, const uint8_t* type, const float* he3, const float* radius, const float* halfHeight)
{
  if (!c) return 0;
  REFUSE_WHILE_SHAPES_PENDING(c, "scTickUploadColliders");
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  // validate before anything is stored: a failed call leaves the context as it was
  for (uint32_t i = 0; i < count; ++i) {
    if (type && type[i] > SC_TICK_COLLIDER_CAPSULE) return fail(c, "unknown collider type (SC_TICK_COLLIDER_*)");
    if (he3) for (int k = 0; k < 3; ++k) { const float v = he3[3 * (size_t)i + k]; if (!std::isfinite(v) || v < 0.0f) return fail(c, "collider half extents must be finite and not negative"); }
    if (radius && (!std::isfinite(radius[i]) || radius[i] < 0.0f)) return fail(c, "collider radius must be finite and not negative");
    if (halfHeight && !std::isfinite(halfHeight[i])) return fail(c, "collider half height must be finite");
    // (the declared layer vocabulary covers every collider there is, scTickSetWorldLayers: an entity cannot become one outside it)
    if (c->worldLayersKnown && (!type || type[i] >= SC_TICK_COLLIDER_BOX) && first + i < c->hLayers.size() && (c->hLayers[first + i] & ~c->worldLayers))
      return fail(c, "collider on an entity whose layers lie outside the declared world vocabulary (scTickSetWorldLayers)");
  }
  DeviceState& d = c->d;
  if (!d.colType) {
    // first call: the storage (every entity SC_TICK_COLLIDER_BOUNDS = 0, as the zeroed allocation has it), and from now on the
    // collider instances of the fused and level kernels -- captured graphs are stale (TickParams::colliders is part of their key)
    if (!sync(c)) return 0;
    const size_t N = c->cap;
    if (!dalloc(c, d.colShape, N) || !dalloc(c, d.colType, N)) { d.colShape = nullptr; d.colType = nullptr; return 0; }
    c->hColType.assign(c->desc.capacity, (uint8_t)SC_TICK_COLLIDER_BOUNDS);
    c->hColValues.assign((size_t)c->desc.capacity * 5u, 0.5f);
  }
  if (!count) return 1;
  std::vector<float4> shape(count);
  std::vector<uint8_t> types(count);
  bool membership = false;
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t g = first + i;
    const uint8_t t = type ? type[i] : (uint8_t)SC_TICK_COLLIDER_BOX;
    float* v = &c->hColValues[5u * (size_t)g];
    const bool had = hasProxyHost(c, g);
    c->hColType[g] = t;
    if (he3) { v[0] = he3[3 * (size_t)i]; v[1] = he3[3 * (size_t)i + 1]; v[2] = he3[3 * (size_t)i + 2]; } else v[0] = v[1] = v[2] = 0.5f;
    v[3] = radius ? radius[i] : 0.5f;
    v[4] = halfHeight ? (halfHeight[i] < 0.0f ? 0.0f : halfHeight[i]) : 0.5f;      // max(0, ...), sc_physics.cpp:154
    membership = membership || had != hasProxyHost(c, g);
    types[i] = t;
    // the record as the box rule consumes it (colliderAabb): extents of the flat part, radius of the round part
    shape[i] = t == SC_TICK_COLLIDER_BOX ? make_float4(v[0], v[1], v[2], 0.0f)
             : t == SC_TICK_COLLIDER_SPHERE ? make_float4(0.0f, 0.0f, 0.0f, v[3])
             : t == SC_TICK_COLLIDER_CAPSULE ? make_float4(0.0f, v[4], 0.0f, v[3]) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }
  // what a bounds upload invalidates: unmoved entities' records are no longer this tick's (cleanStay), and where an entity gained or
  // lost its proxy, the remembered slots and the captured graphs (as a Bounds membership change does through the link words)
  c->boxesTouched = true;
  if (membership) { c->homeValid = false; c->topoEpoch++; }
  if (!h2d(c, d.colShape + first, shape.data(), (size_t)count * sizeof(float4)) || !h2d(c, d.colType + first, types.data(), count)) return 0;
  if (!refreshTiles(c, first, first + count)) return 0;      // (the tiles' shared layer words are over the entities with a proxy)
  return sync(c) ? 1 : 0;
}

int scTickReadColliders(ScTickContext* c, uint32_t first, uint32_t count, uint8_t* type, float* he3, float* radius, float* halfHeight)
{
  if (!c) return 0;
  if (!rangeOk(c, first, count)) return 0;
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t g = first + i;
    const bool have = !c->hColType.empty();
    const float* v = have ? &c->hColValues[5u * (size_t)g] : nullptr;
    if (type) type[i] = have ? c->hColType[g] : (uint8_t)SC_TICK_COLLIDER_BOUNDS;
    if (he3) for (int k = 0; k < 3; ++k) he3[3 * (size_t)i + k] = have ? v[k] : 0.5f;
    if (radius) radius[i] = have ? v[3] : 0.5f;
    if (halfHeight) halfHeight[i] = have ? v[4] : 0.5f;
  }
  return 1;
}

int scTickUploadRenderMeshes(ScTickContext* c, uint32_t first, uint32_t count, const uint8_t* has, const uint32_t* mesh, const uint32_t* material)
{
  if (!c) return 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!count) return 1;
  if (mesh && !h2d(c, c->d.meshId + first, mesh, (size_t)count * 4u)) return 0;
  if (material && !h2d(c, c->d.materialId + first, material, (size_t)count * 4u)) return 0;
  if (!sync(c)) return 0;
  for (uint32_t i = 0; i < count; ++i) {
    uint8_t& f = c->hFlags[first + i];
    const uint8_t nf = (uint8_t)((f & ~1u) | ((!has || has[i]) ? 1u : 0u));
    if (nf != f) { f = nf; c->linksStale = true; }
  }
  return 1;
}

int scTickUploadLayers(ScTickContext* c, uint32_t first, uint32_t count, const uint32_t* group, const uint32_t* mask)
{
  if (!c || !group || !mask) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  // (the island pass of a pending pair half decides "movable" from the layer words as they stand when it runs)
  if (c->pairsPending && (c->pendingTick.narrow & kStageIslands))
    return fail(c, "scTickUploadLayers is refused between scTickRun(.. | SC_TICK_SPLIT_PAIRS) and scTickRunPairs of a tick that computes pair islands: its pair half reads the layer words as they stand");
  if (!count) return 1;
  std::vector<uint32_t> packed(count);
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t g = group[i], m = mask[i];
    if ((g != 0xFFFFFFFFu && (g >> 16)) || (m != 0xFFFFFFFFu && (m >> 16))) return fail(c, "group/mask bits above 15 are not supported");
    packed[i] = (g & 0xFFFFu) | ((m & 0xFFFFu) << 16);
    // the declared layer vocabulary of the tiled world is a contract (scTickSetWorldLayers): a collider outside it could meet bins that
    // this or another tile leaves unwritten for good -- refused here instead of missing pairs silently there
    if (c->worldLayersKnown && (packed[i] & ~c->worldLayers))
      return fail(c, "layers outside the declared world vocabulary (scTickSetWorldLayers): declare the wider vocabulary on every tile first");
  }
  if (!h2d(c, c->d.layers + first, packed.data(), (size_t)count * 4u)) return 0;
  if (c->hLayers.size() < (size_t)first + count) c->hLayers.resize((size_t)first + count, 0u);
  std::copy(packed.begin(), packed.end(), c->hLayers.begin() + first);      // (host mirror: what a later, narrower vocabulary is checked against)
  c->layerSetStale = true;
  c->homeValid = false;                 // the bins' remembered layer summaries are behind
  if (!refreshTiles(c, first, first + count)) return 0;      // (bounds classes: the tiles' shared layer words)
  return sync(c) ? 1 : 0;
}

int scTickSetTopology(ScTickContext* c, const int32_t* parent, uint32_t count)
{
  if (!c || (!parent && count)) return c ? fail(c, "null argument") : 0;
  if (count != c->n) return fail(c, "topology must cover every entity (count != entity count)");
  if (!bind(c)) return 0;
  std::copy(parent, parent + count, c->hParent.begin());
  c->linksStale = true;
  return flushLinks(c);
}

// ---- sector residency -------------------------------------------------------------------------------
static uint32_t linkWordOfRoot(uint8_t f)
{
  return kNoParent | ((f & 1u) ? kHasMesh : 0u) | ((f & 2u) ? kHasBounds : 0u) |
         ((f & 4u) ? kRotTrivialX : 0u) | ((f & 8u) ? kRotTrivialY : 0u) | ((f & 16u) ? kRotTrivialZ : 0u);
}

int scTickAppendEntities(ScTickContext* c, uint32_t count, const float* pos3, const float* rot3, const float* scale3,
                         const float* bmin3, const float* bmax3, const uint32_t* mesh, const uint32_t* material,
                         const uint32_t* group, const uint32_t* mask, const int32_t* parent, uint32_t* firstOut)
{
  if (!c) return 0;
  if (count && (!pos3 || !rot3 || !scale3)) return fail(c, "null argument");
  if ((bmin3 == nullptr) != (bmax3 == nullptr) || (group == nullptr) != (mask == nullptr)) return fail(c, "bounds / layers come in pairs");
  if (!bind(c)) return 0;
  const uint32_t first = c->n;
  if ((uint64_t)first + count > c->desc.capacity) return fail(c, "append exceeds capacity");
  if (firstOut) *firstOut = first;
  if (!count) return 1;
  if (parent) for (uint32_t i = 0; i < count; ++i)
    if (parent[i] != SC_TICK_NO_PARENT && (parent[i] < 0 || (uint32_t)parent[i] >= first + count)) return fail(c, "parent index out of range");

  const bool wasStale = c->linksStale;
  c->n = first + count;
  for (uint32_t i = first; i < first + count; ++i) {
    c->hFlags[i] = 0; c->hParent[i] = SC_TICK_NO_PARENT; c->hChildren[i] = 0;
    c->hFirstChild[i] = -1; c->hNextSib[i] = -1; c->hPrevSib[i] = -1;
  }

  if (!resetColliders(c, first, count)) { c->n = first; c->linksStale = true; return 0; }
  std::vector<float> cube;
  if (!bmin3) { cube.assign((size_t)count * 6, 0.5f); for (size_t i = 0; i < (size_t)count * 3; ++i) cube[i] = -0.5f; }   // kUnitCubeBounds
  std::vector<uint32_t> all;
  if (!group) all.assign(count, 0xFFFFFFFFu);
  std::vector<uint32_t> zeros;
  if (!mesh || !material) zeros.assign(count, 0u);
  const bool ok =
      scTickUploadLocals(c, first, count, pos3, rot3, scale3, nullptr) &&
      scTickUploadBounds(c, first, count, bmin3 ? bmin3 : cube.data(), bmax3 ? bmax3 : cube.data() + (size_t)count * 3, nullptr) &&
      scTickUploadRenderMeshes(c, first, count, nullptr, mesh ? mesh : zeros.data(), material ? material : zeros.data()) &&
      scTickUploadLayers(c, first, count, group ? group : all.data(), mask ? mask : all.data());
  if (!ok) { c->n = first; c->linksStale = true; return 0; }
  for (uint32_t i = first; i < first + count; ++i) c->hFlags[i] &= (uint8_t)~32u;
  if (c->d.moverKind) {       // an appended entity is no mover until scTickUploadMovers says so
    const hipError_t e = hipMemsetAsync(c->d.moverKind + first, 0, (size_t)count * 4u, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemsetAsync", e);
  }
  if (c->d.aHitType) {        // ... and a new entity's TrafficSensors are the context's defaults with nothing hit yet (sc_traffic_common.h:46-53), not the slot's last occupant's
    launchFillSensors(c->d, first, count, c->sensorRay, c->sensorSafe, c->stream);
    hipError_t e = hipMemsetAsync(c->d.aHitDist + first, 0, (size_t)count * 4u, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d.aHitType + first, 0, (size_t)count * 4u, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d.aBrake + first, 0, (size_t)count * 4u, c->stream);
    if (e != hipSuccess) return fail(c, "hipMemsetAsync", e);
  }

  if (parent || wasStale) {
    if (parent) std::copy(parent, parent + count, c->hParent.begin() + first);
    c->linksStale = true;
    return flushLinks(c);
  }
  // roots only and the rest of the hierarchy untouched: write just the new link words (no re-link: the topology classes are behind)
  c->topoCurrent = false;
  std::vector<uint32_t> link(count);
  for (uint32_t i = 0; i < count; ++i) link[i] = linkWordOfRoot(c->hFlags[first + i]);
  if (!h2d(c, c->d.link + first, link.data(), (size_t)count * 4u)) { c->linksStale = true; return 0; }
  launchRootMask(c->d, c->n, c->stream);
  if (!sync(c)) { c->linksStale = true; return 0; }
  c->linksStale = false;
  c->topoEpoch++;
  return 1;
}

int scTickRemoveEntities(ScTickContext* c, const uint32_t* idx, uint32_t count, uint32_t* movedFrom, uint32_t* movedTo, uint32_t* movedCount)
{
  if (!c) return 0;
  if (movedCount) *movedCount = 0;
  if (!idx && count) return fail(c, "null argument");
  REFUSE_WHILE_SHAPES_PENDING(c, "scTickRemoveEntities");
  if (!bind(c)) return 0;
  if (!count) return 1;
  const uint32_t n0 = c->n;
  if (count > n0) return fail(c, "more removals than entities");

  // Replay the swap-removes on an index map that only holds the slots they touch.
  std::unordered_map<uint32_t, uint32_t> occupant;   // slot -> original index of the entity now in it
  std::unordered_map<uint32_t, uint32_t> where;      // original index -> slot it was moved to
  std::unordered_set<uint32_t> removed;
  occupant.reserve(count * 2u); where.reserve(count * 2u); removed.reserve(count * 2u);
  uint32_t size = n0;
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t r = idx[k];
    if (r >= n0) return fail(c, "dense index out of range");
    if (!removed.insert(r).second) return fail(c, "dense index listed twice");
    const auto w = where.find(r);
    const uint32_t slot = w == where.end() ? r : w->second;
    const uint32_t last = size - 1u;
    const auto o = occupant.find(last);
    const uint32_t lastOrig = o == occupant.end() ? last : o->second;
    if (slot != last) { occupant[slot] = lastOrig; where[lastOrig] = slot; }
    size = last;
  }
  const uint32_t n1 = size;
  std::vector<uint32_t> src, dst;
  for (const auto& kv : occupant) if (kv.first < n1 && kv.second != kv.first) { dst.push_back(kv.first); src.push_back(kv.second); }
  // deterministic order for the caller
  {
    std::vector<uint32_t> order(dst.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return dst[a] < dst[b]; });
    std::vector<uint32_t> s2(src.size()), d2(dst.size());
    for (uint32_t i = 0; i < order.size(); ++i) { s2[i] = src[order[i]]; d2[i] = dst[order[i]]; }
    src.swap(s2); dst.swap(d2);
  }
  const uint32_t moves = (uint32_t)src.size();

  std::unordered_map<uint32_t, uint32_t> newIndexOf;
  newIndexOf.reserve(moves * 2u);
  for (uint32_t k = 0; k < moves; ++k) newIndexOf[src[k]] = dst[k];
  auto remap = [&](int32_t i) -> int32_t {          // index before the call -> index after it (sources are >= n1, targets < n1)
    if (i < 0) return i;
    const auto m = newIndexOf.find((uint32_t)i);
    return m == newIndexOf.end() ? i : (int32_t)m->second;
  };

  // The hierarchy is patched in place unless an index sits in a level list or a cycle, or a removed entity
  // leaves a child behind (orphans change the depth of whole subtrees: full re-link, sc_ecs.cpp:151-160).
  bool relink = c->linksStale || c->unreachable > 0 || c->maxDepth > kMaxChain;
  for (uint32_t k = 0; k < count && !relink; ++k)
    for (int32_t ch = c->hFirstChild[idx[k]]; ch >= 0 && !relink; ch = c->hNextSib[(uint32_t)ch]) relink = !removed.count((uint32_t)ch);

  // device: relocate every per-entity array
  if (moves) {
    if (!needScratch(c, 2u * (size_t)moves)) return 0;
    if (!h2d(c, c->dIdx, src.data(), (size_t)moves * 4u) || !h2d(c, c->dIdx + moves, dst.data(), (size_t)moves * 4u)) return 0;
    launchMoveEntities(c->d, c->dIdx, c->dIdx + moves, moves, c->stream);
    if (!sync(c)) return 0;                          // the scratch buffer is reused for the parent patches below
    for (uint32_t k = 0; k < moves; ++k)             // (the layer words' host mirror moves along: sources lie beyond every target)
      if (src[k] < c->hLayers.size()) { if (c->hLayers.size() <= dst[k]) c->hLayers.resize((size_t)dst[k] + 1u, 0u); c->hLayers[dst[k]] = c->hLayers[src[k]]; }
    for (uint32_t k = 0; k < moves; ++k) c->hClass[dst[k]] = c->hClass[src[k]];      // (and the class of its box)
    if (!c->hColType.empty())                                                        // (and its collider)
      for (uint32_t k = 0; k < moves; ++k) {
        c->hColType[dst[k]] = c->hColType[src[k]];
        std::copy(c->hColValues.begin() + 5u * (size_t)src[k], c->hColValues.begin() + 5u * (size_t)src[k] + 5u, c->hColValues.begin() + 5u * (size_t)dst[k]);
      }
    c->layerSetStale = true;
  }

  std::vector<uint32_t> patch;                       // (entity, new parent) pairs for the device link words
  if (!relink) {
    c->topoCurrent = false;                          // link words are relocated and patched on the device: the topology classes are behind until the next re-link
    std::vector<int32_t>&par = c->hParent, &fc = c->hFirstChild, &ns = c->hNextSib, &ps = c->hPrevSib;
    // 1. unlink the removed entities from surviving parents (indices as before the call)
    for (uint32_t k = 0; k < count; ++k) {
      const uint32_t r = idx[k];
      const int32_t q = par[r];
      if (q < 0 || removed.count((uint32_t)q)) continue;
      if (ps[r] >= 0) ns[(uint32_t)ps[r]] = ns[r]; else fc[(uint32_t)q] = ns[r];
      if (ns[r] >= 0) ps[(uint32_t)ns[r]] = ps[r];
      c->hChildren[(uint32_t)q]--;
    }
    // 2. gather every write a relocation needs, reading only the records as they stand (sources are never written)
    struct Set { std::vector<int32_t>* arr; uint32_t at; int32_t value; };
    std::vector<Set> sets;
    for (uint32_t k = 0; k < moves; ++k) {
      const uint32_t s0 = src[k], d0 = dst[k];
      sets.push_back({ &par, d0, remap(par[s0]) });
      sets.push_back({ &fc, d0, remap(fc[s0]) });
      sets.push_back({ &ns, d0, remap(ns[s0]) });
      sets.push_back({ &ps, d0, remap(ps[s0]) });
      if (ps[s0] >= 0) sets.push_back({ &ns, (uint32_t)remap(ps[s0]), (int32_t)d0 });
      else if (par[s0] >= 0) sets.push_back({ &fc, (uint32_t)remap(par[s0]), (int32_t)d0 });
      if (ns[s0] >= 0) sets.push_back({ &ps, (uint32_t)remap(ns[s0]), (int32_t)d0 });
      for (int32_t ch = fc[s0]; ch >= 0; ch = ns[(uint32_t)ch]) {
        const uint32_t at = (uint32_t)remap(ch);
        sets.push_back({ &par, at, (int32_t)d0 });
        patch.push_back(at); patch.push_back(d0);
      }
      c->hFlags[d0] = c->hFlags[s0];
      c->hChildren[d0] = c->hChildren[s0];
    }
    // 3. apply (writes that meet on one field carry the same value)
    for (const Set& w : sets) (*w.arr)[w.at] = w.value;
    // span-closed state: only the relocated entities and the children re-parented to them have new links (a removed link can only
    // have been a crossing one in a world that was not closed: that stays "not closed" until the next re-link)
    if (c->spanClosed) {
      const uint32_t sp = c->closureSpan;
      auto crosses = [&](uint32_t i) { return par[i] >= 0 && (uint32_t)par[i] / sp != i / sp; };
      for (uint32_t k = 0; k < moves && c->spanClosed; ++k) if (crosses(dst[k])) c->spanClosed = false;
      for (size_t k = 0; k < patch.size() && c->spanClosed; k += 2) if (crosses(patch[k])) c->spanClosed = false;
    }
    if (!patch.empty()) {
      const uint32_t pairs = (uint32_t)(patch.size() / 2);
      if (!needScratch(c, patch.size())) return 0;
      if (!h2d(c, c->dIdx, patch.data(), patch.size() * 4u)) return 0;
      launchPatchParents(c->d, c->dIdx, pairs, c->stream);
    }
  } else {
    // parents are rewritten through the relocation map; a child of a removed entity gets an invalid parent,
    // which the re-link detaches and marks dirty (sc_ecs.cpp:151-160)
    for (uint32_t k = 0; k < moves; ++k) { c->hParent[dst[k]] = c->hParent[src[k]]; c->hFlags[dst[k]] = c->hFlags[src[k]]; }
    constexpr int32_t kGone = -2;
    for (uint32_t i = 0; i < n1; ++i) {
      const int32_t q = c->hParent[i];
      if (q == SC_TICK_NO_PARENT) continue;
      if (removed.count((uint32_t)q)) c->hParent[i] = kGone;
      else c->hParent[i] = remap(q);
    }
    c->linksStale = true;
  }
  c->n = n1;
  c->topoEpoch++;
  if (!resyncPairEvents(c)) return 0;                 // dense indices were renamed: the remembered pair set names entities that moved or are gone
  // anchored rays follow their entity: a relocated anchor is renamed, a removed one becomes dead (it misses from now on); the words
  // go to the device behind whatever is queued, and the set keeps its size -- no epoch bump of its own
  if (c->anchored.count) {
    bool changed = false;
    for (uint32_t k = 0; k < c->anchored.count; ++k) {
      uint32_t& a = c->hAnchor[k].x;
      if (a >= n0) continue;                            // no anchor, dead, or beyond the count: nothing to follow
      if (removed.count(a)) { a = kAnchorDead; changed = true; continue; }
      const auto m = newIndexOf.find(a);
      if (m != newIndexOf.end()) { a = m->second; changed = true; }
    }
    if (changed && !h2d(c, const_cast<uint2*>(c->anchored.anchor), c->hAnchor.data(), (size_t)c->anchored.count * sizeof(uint2))) return 0;
  }
  if (c->triggers.count) {                              // ... and so do the trigger volumes' anchors (their remembered rows went with resyncPairEvents above)
    bool changed = false;
    for (uint32_t k = 0; k < c->triggers.count; ++k) {
      uint32_t& a = c->hTriggerAnchor[k].x;
      if (a >= n0) continue;
      if (removed.count(a)) { a = kAnchorDead; changed = true; continue; }
      const auto m = newIndexOf.find(a);
      if (m != newIndexOf.end()) { a = m->second; changed = true; }
    }
    if (changed && !h2d(c, const_cast<uint2*>(c->triggers.anchor), c->hTriggerAnchor.data(), (size_t)c->triggers.count * sizeof(uint2))) return 0;
  }
  if (c->asweeps.count) {                               // ... and the anchored sweeps' anchors
    bool changed = false;
    for (uint32_t k = 0; k < c->asweeps.count; ++k) {
      uint32_t& a = c->hSweepAnchor[k].x;
      if (a >= n0) continue;
      if (removed.count(a)) { a = kAnchorDead; changed = true; continue; }
      const auto m = newIndexOf.find(a);
      if (m != newIndexOf.end()) { a = m->second; changed = true; }
    }
    if (changed && !h2d(c, const_cast<uint4*>(c->asweeps.anchor), c->hSweepAnchor.data(), (size_t)c->asweeps.count * sizeof(uint4))) return 0;
  }
  {
    // bounds classes: the wave-tiles that took a relocated entity, and those of the shrunk tail
    std::vector<uint32_t> tiles;
    for (uint32_t k = 0; k < moves; ++k) if (tiles.empty() || tiles.back() != dst[k] >> 6) tiles.push_back(dst[k] >> 6);      // (dst ascends)
    for (uint32_t t = n1 >> 6; t <= (n0 - 1u) >> 6; ++t) tiles.push_back(t);
    if (!refreshTileList(c, tiles)) return 0;
  }
  if (movedFrom && movedTo) { std::copy(src.begin(), src.end(), movedFrom); std::copy(dst.begin(), dst.end(), movedTo); }
  if (movedCount) *movedCount = moves;
  if (relink) return flushLinks(c);
  launchRootMask(c->d, c->n, c->stream);             // relocated link words, patched parents
  return sync(c) ? 1 : 0;
}

int scTickMarkDirty(ScTickContext* c, uint32_t first, uint32_t count)
{
  if (!c) return 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  launchSetDirtyRange(c->d, first, count, c->stream);
  return 1;
}

int scTickMarkDirtyIndices(ScTickContext* c, const uint32_t* idx, uint32_t count)
{
  if (!c || (!idx && count)) return c ? fail(c, "null argument") : 0;
  if (!bind(c)) return 0;
  if (!count) return 1;
  for (uint32_t i = 0; i < count; ++i) if (idx[i] >= c->n) return fail(c, "dense index out of range");
  if (!needScratch(c, count)) return 0;
  if (!h2d(c, c->dIdx, idx, (size_t)count * 4u)) return 0;
  launchSetDirtyIndices(c->d, c->dIdx, count, c->stream);
  return sync(c) ? 1 : 0;
}

int scTickSetDirtyFlags(ScTickContext* c, uint32_t first, uint32_t count, const uint8_t* flags)
{
  if (!c || !flags) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!count) return 1;
  // read-modify-write of the covered words on the host: exact flags for [first, first+count)
  const uint32_t w0 = first >> 5, w1 = (first + count + 31u) >> 5;
  std::vector<uint32_t> words(w1 - w0);
  if (!d2h(c, words.data(), c->d.dirty + w0, words.size() * 4u) || !sync(c)) return 0;
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t g = first + i, bit = 1u << (g & 31u);
    uint32_t& w = words[(g >> 5) - w0];
    w = flags[i] ? (w | bit) : (w & ~bit);
  }
  if (!h2d(c, c->d.dirty + w0, words.data(), words.size() * 4u)) return 0;
  return sync(c) ? 1 : 0;
}

int scTickSetDrawSortTable(ScTickContext* c, const uint8_t* pipelineOfMaterial, uint32_t materialCount, uint32_t meshCount)
{
  if (!c) return 0;
  if (!pipelineOfMaterial && materialCount) return fail(c, "null argument");
  if (materialCount > (1u << 24) || meshCount > (1u << 24)) return fail(c, "more than 2^24 material or mesh handles");
  for (uint32_t i = 0; i < materialCount; ++i)
    if (pipelineOfMaterial[i] >= 128u && pipelineOfMaterial[i] != kNoMaterial) return fail(c, "pipeline ids must be < 128 (0xFF = no such material)");
  if (!bind(c) || !sync(c)) return 0;
  DrawSortState& st = c->sort;
  if (!st.key[0]) {
    const size_t N = c->cap;
    const size_t groups = (N + kSortGroup - 1) / kSortGroup;
    if (!dalloc(c, st.key[0], N, false) || !dalloc(c, st.key[1], N, false) || !dalloc(c, st.idx[0], N, false) ||
        !dalloc(c, st.idx[1], N, false) || !dalloc(c, st.hist, 256u * groups, false)) return 0;
  }
  if (c->pipelineCap < std::max(materialCount, 1u)) {
    dfree(c, c->dPipeline); c->dPipeline = nullptr; c->pipelineCap = 0;
    const uint32_t want = std::max(materialCount, 64u);
    if (!dalloc(c, c->dPipeline, want, false)) return 0;
    c->pipelineCap = want;
  }
  if (materialCount && (!h2d(c, c->dPipeline, pipelineOfMaterial, materialCount) || !sync(c))) return 0;
  st.pipeline = c->dPipeline;
  st.materialCount = materialCount; st.meshCount = meshCount;
  // key = pipeline << 48 | material << 24 | mesh: sort only over the bytes the handle ranges can reach,
  // and always over the top byte (pipeline + the "dropped" mark)
  auto bytesOf = [](uint32_t count) { uint32_t top = count > 1u ? count - 1u : 0u, b = 0; while (top) { ++b; top >>= 8; } return b; };
  st.passes = 0;
  for (uint32_t b = 0; b < bytesOf(meshCount); ++b) st.shift[st.passes++] = 8u * b;
  for (uint32_t b = 0; b < bytesOf(materialCount); ++b) st.shift[st.passes++] = 24u + 8u * b;
  st.shift[st.passes++] = 48u;
  c->topoEpoch++;                      // captured graphs hold the old pass list
  if (c->bind.info && c->bind.materialCount != materialCount && !reallocBindRuns(c, c->bind.maxRuns)) return 0;      // the touch bitmap follows the table
  return 1;
}

int scTickSetDrawBudget(ScTickContext* c, uint32_t maxDraws)
{
  if (!c) return 0;
  if (maxDraws == c->desc.max_draws_budget) return 1;
  if (c->pending.on) { if (!bind(c)) return 0; settle(c); }
  // a captured tick holds the budget by value (the folded emission, the emission and sort launches, the run table's bound): not in the key
  if (c->graphMode) { if (!bind(c) || !sync(c)) return 0; dropGraphs(c->graph); }
  c->desc.max_draws_budget = maxDraws;
  return 1;
}

int scTickUploadWorldMatrices(ScTickContext* c, uint32_t first, uint32_t count, const float* m16)
{
  if (!c || !m16) return c ? fail(c, "null argument") : 0;
  REFUSE_WHILE_SHAPES_PENDING(c, "scTickUploadWorldMatrices");
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!count) return 1;
  c->boxesTouched = true;
  std::vector<float4> r0(count), r1(count), r2(count);
  for (uint32_t i = 0; i < count; ++i) {
    const float* m = m16 + 16 * (size_t)i;
    if (m[3] != 0.0f || m[7] != 0.0f || m[11] != 0.0f || m[15] != 1.0f) return fail(c, "world matrix is not affine (row 3 must be 0,0,0,1)");
    r0[i] = make_float4(m[0], m[4], m[8], m[12]);
    r1[i] = make_float4(m[1], m[5], m[9], m[13]);
    r2[i] = make_float4(m[2], m[6], m[10], m[14]);
  }
  if (!h2d(c, c->d.w0 + first, r0.data(), (size_t)count * 16u) || !h2d(c, c->d.w1 + first, r1.data(), (size_t)count * 16u) ||
      !h2d(c, c->d.w2 + first, r2.data(), (size_t)count * 16u)) return 0;
  return sync(c) ? 1 : 0;
}

int scTickSetFrustumPlanes(ScTickContext* c, const float planes[24], int valid)
{
  if (!c || !planes) return c ? fail(c, "null argument") : 0;
  std::memcpy(c->frustum.p, planes, sizeof c->frustum.p);
  c->frustumValid = valid ? 1 : 0;
  c->frustumStale = true;
  return 1;
}

int scTickGetFrustumPlanes(ScTickContext* c, float planes[24], int* valid)
{
  if (!c || !planes) return c ? fail(c, "null argument") : 0;
  std::memcpy(planes, c->frustum.p, sizeof c->frustum.p);
  if (valid) *valid = c->frustumValid;
  return 1;
}

// frustumFromViewProj, sc_world_partition.cpp:1071-1103: planes r3 +- r0, r3 +- r1, r3 +- r2 of the
// column-major matrix' rows, normalised by 1/sqrt(a^2+b^2+c^2) when that exceeds 1e-8 (else zero plane).
int scTickSetViewProj(ScTickContext* c, const float m[16])
{
  if (!c || !m) return c ? fail(c, "null argument") : 0;
  const float row[4][4] = { { m[0], m[4], m[8], m[12] }, { m[1], m[5], m[9], m[13] },
                            { m[2], m[6], m[10], m[14] }, { m[3], m[7], m[11], m[15] } };
  for (int pl = 0; pl < 6; ++pl) {
    const int axis = pl >> 1;
    float v[4];
    for (int k = 0; k < 4; ++k) v[k] = (pl & 1) ? row[3][k] - row[axis][k] : row[3][k] + row[axis][k];
    const float lenSq = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
    float* out = c->frustum.p[pl];
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    if (lenSq > 1e-8f) {
      const float invLen = 1.0f / std::sqrt(lenSq);
      out[0] = v[0] * invLen; out[1] = v[1] * invLen; out[2] = v[2] * invLen; out[3] = v[3] * invLen;
    }
  }
  c->frustumValid = 1;
  c->frustumStale = true;
  return 1;
}

int scTickSetFreezeCulling(ScTickContext* c, int freeze)
{
  if (!c) return 0;
  c->freeze = freeze ? 1 : 0;
  return 1;
}

static int exchangeBorders(ScTickContext* c, uint32_t parity, hipStream_t s, bool inCapture);

// merge what the neighbours sent, answer the ray queries, search the pairs: the half of a tile's step behind the exchange
// `done` (may be null) rides on the half's last dispatch; false = it could not (nothing launched): record it on the stream
static bool enqueuePairHalf(ScTickContext* c, const TickPlan& tick, hipStream_t ps, hipEvent_t done = nullptr)
{
  const TickParams& pp = tick.p;
  const DeviceState ds = stateFor(c, pp.parity);
  launchBorderMerge(ds, pp, ps);
  // (exact shapes: an in-order tile's matrices are still this tick's here; a pipelined context was refused by scTickRun)
  const bool exactRays = c->rayShapes == SC_TICK_RAY_SHAPES_EXACT;
  if (pp.flags & SC_TICK_RAYS) launchRayQueries(ds, pp, c->rays, exactRays, ps);   // sees the neighbours' border boxes too
  if (pp.flags & SC_TICK_SWEEPS) launchSweepQueries(ds, pp, c->sweeps, exactSweepInfo(c), ps);   // ... as do the capsule sweeps (exact shapes: as for the rays)
  if (pp.flags & SC_TICK_ANCHORED_RAYS) launchAnchoredRays(ds, pp, anchoredFor(c, pp.parity), true, exactRays, ps);   // ... and the anchored rays, as the tick half resolved them
  if (raysInPairHalf(c, pp.flags) && ds.aLane) launchAgentFrontRaysFromSnapshot(ds, pp, ps);      // ... and so do the agents' obstacle rays
  // (pair events are refused on a pipelined tile, the only flow that hands a `done` event in: nothing is queued behind a dispatch it rides on)
  const bool rode = launchPairs(ds, pp, ps, done);
  closePairHalf(c, ds, tick, ps);      // (the touching pairs: an in-order tile's matrices are still this tick's here; a pipelined context was refused by scTickRun)
  return rode;
}

// Can any two colliders this context may ever hold in its bins meet (Bullet's filter, sc_physics.cpp:700-712 via SURVEY 8a)?  From the
// host's mirror of the uploaded layer words -- and, on a tile, the declared vocabulary of the world (records arrive from neighbours).
// An all-static city cannot: its pair role is a sweep over the bins' counters and nothing else, and the launcher sizes the grid for
// that (pairGridFor).  A HINT for launch shapes only: the search itself never goes by it.
static bool worldCanPair(ScTickContext* c)
{
  if (c->layerSetStale || c->layerSetN != c->n) {
    std::vector<uint32_t> words;
    uint32_t last = 0; bool any = false, many = false;
    const size_t upto = std::min<size_t>(c->hLayers.size(), c->n);
    for (size_t i = 0; i < upto && !many; ++i) {
      const uint32_t w = c->hLayers[i];
      if (any && w == last) continue;
      last = w; any = true;
      if (std::find(words.begin(), words.end(), w) == words.end()) { if (words.size() >= 64u) many = true; else words.push_back(w); }
    }
    bool can = many;
    for (size_t a = 0; a < words.size() && !can; ++a)
      for (size_t b = a; b < words.size() && !can; ++b)
        can = ((words[a] & 0xFFFFu) & (words[b] >> 16)) && ((words[b] & 0xFFFFu) & (words[a] >> 16));
    c->ownLayersCanPair = can; c->layerSetStale = false; c->layerSetN = c->n;
  }
  if (c->ownLayersCanPair) return true;
  if (!c->neighbourMask) return false;
  return !c->worldLayersKnown || ((c->worldLayers & 0xFFFFu) & (c->worldLayers >> 16)) != 0u;
}

// A QUIET tick: a broadphase tick none of whose bins, counters, layer summaries or home words anybody reads -- the world cannot pair
// (worldCanPair), no query, sensor, event, shape pass, dense-box read-back, neighbour or caller-owned pair half looks at the bins, and the
// remembered slots are current, so nothing is to be learnt either.  Its device work is that of the same call without SC_TICK_BROADPHASE.
// The slots' age does not end a quiet stretch (nothing ages that anyone reads): the first binning tick behind it applies the usual rule.
static bool quietTick(ScTickContext* c, uint32_t flags)
{
  constexpr uint32_t kBinReaders = SC_TICK_RAYS | SC_TICK_SWEEPS | SC_TICK_ANCHORED_RAYS | SC_TICK_PAIR_EVENTS | SC_TICK_PAIR_SHAPES |
                                   SC_TICK_TOUCH_EVENTS | SC_TICK_DENSE_AABBS | SC_TICK_SPLIT_PAIRS | SC_TICK_OVERLAPS | SC_TICK_TRIGGERS |
                                   SC_TICK_ANCHORED_SWEEPS;
  if (!(flags & SC_TICK_BROADPHASE) || (flags & kBinReaders) || !c->quietEnabled || !c->homeEnabled || !c->lazyEnabled) return false;
  if (!c->n || c->sensors || c->neighbourMask || c->pairsStream || c->pairsPending) return false;
  if (!c->homeValid || c->homeEpoch != c->topoEpoch) return false;      // (a learn tick is due: an append, a remove, a re-link, a layer upload)
  return !worldCanPair(c);
}

// An empty context without a broadphase has nothing to launch (emptyTick)
static bool nothingToRun(const ScTickContext* c, uint32_t flags) { return c->n == 0 && !(flags & SC_TICK_BROADPHASE); }

// Every reason scTickRun refuses a call for, in one order; writes nothing but the error text.  (A run with nothing to launch is asked
// no more than the checks ahead of that line.)
static bool tickAccepted(ScTickContext* c, uint32_t flags)
{
  if ((flags & SC_TICK_BROADPHASE) && c->desc.tile_sectors_x == 0) return fail(c, "broadphase requested but the context has no tile rectangle");
  if (flags & SC_TICK_PAIR_EVENTS) {
    if (!(flags & SC_TICK_BROADPHASE)) return fail(c, "SC_TICK_PAIR_EVENTS needs SC_TICK_BROADPHASE in the same run (the events are the difference of this tick's pair set)");
    if (!c->pairEvents.ctl) return fail(c, "SC_TICK_PAIR_EVENTS needs scTickSetPairEvents first");
    if (c->pairsStream) return fail(c, "SC_TICK_PAIR_EVENTS cannot run on a pipelined context (scTickSetPipelined / scTickSetPairsStream): its tick parities overlap in time");
  }
  if (flags & SC_TICK_PAIR_SHAPES) {
    if (!(flags & SC_TICK_BROADPHASE)) return fail(c, "SC_TICK_PAIR_SHAPES needs SC_TICK_BROADPHASE in the same run (the touching pairs are those of this tick's pair list)");
    if (!c->narrow.list.ctl) return fail(c, "SC_TICK_PAIR_SHAPES needs scTickSetPairShapes first");
    if (c->pairsStream) return fail(c, "SC_TICK_PAIR_SHAPES cannot run on a pipelined context (scTickSetPipelined / scTickSetPairsStream): its pair half runs when the matrices may be the next tick's");
  }
  if (flags & SC_TICK_TOUCH_EVENTS) {
    if (!(flags & SC_TICK_BROADPHASE)) return fail(c, "SC_TICK_TOUCH_EVENTS needs SC_TICK_BROADPHASE in the same run (the events are the difference of this tick's touching set)");
    if (!c->narrow.touch.ctl) return fail(c, "SC_TICK_TOUCH_EVENTS needs scTickSetTouchEvents first");
    if (c->pairsStream) return fail(c, "SC_TICK_TOUCH_EVENTS cannot run on a pipelined context (scTickSetPipelined / scTickSetPairsStream): its tick parities overlap in time, and its pair half runs when the matrices may be the next tick's");
  }
  if (flags & SC_TICK_BIND_RUNS) {
    if ((flags & (SC_TICK_DRAWS | SC_TICK_SORT_DRAWS)) != (SC_TICK_DRAWS | SC_TICK_SORT_DRAWS))
      return fail(c, "SC_TICK_BIND_RUNS needs SC_TICK_DRAWS | SC_TICK_SORT_DRAWS in the same run (the runs are those of the sorted list; scTickSetDrawSortTable)");
    if (!c->sort.pipeline) return fail(c, "SC_TICK_SORT_DRAWS needs scTickSetDrawSortTable first");
    if (!c->bind.info) return fail(c, "SC_TICK_BIND_RUNS needs scTickSetBindRuns first");
  }
  if (flags & SC_TICK_OVERLAPS) {
    if (!(flags & SC_TICK_BROADPHASE)) return fail(c, "SC_TICK_OVERLAPS needs SC_TICK_BROADPHASE in the same run (the queries read this tick's bins)");
    if (!c->overlaps.count) return fail(c, "SC_TICK_OVERLAPS needs scTickSetOverlapQueries first (the set is empty)");
    if (c->neighbourMask) return fail(c, "SC_TICK_OVERLAPS cannot run on a context with neighbours (scTickSetTile): overlap queries do not cover tiles");
    if (c->pairsStream) return fail(c, "SC_TICK_OVERLAPS cannot run on a pipelined context (scTickSetPipelined / scTickSetPairsStream): overlap queries do not cover tiles");
    if (flags & SC_TICK_SPLIT_PAIRS) return fail(c, "SC_TICK_OVERLAPS cannot run with SC_TICK_SPLIT_PAIRS: overlap queries do not cover tiles");
  }
  if (flags & SC_TICK_TRIGGERS) {
    if (!(flags & SC_TICK_BROADPHASE)) return fail(c, "SC_TICK_TRIGGERS needs SC_TICK_BROADPHASE in the same run (the volumes read this tick's bins)");
    if (!c->triggers.count) return fail(c, "SC_TICK_TRIGGERS needs scTickSetTriggerVolumes first (the set is empty)");
    if (c->neighbourMask) return fail(c, "SC_TICK_TRIGGERS cannot run on a context with neighbours (scTickSetTile): trigger volumes do not cover tiles");
    if (c->pairsStream) return fail(c, "SC_TICK_TRIGGERS cannot run on a pipelined context (scTickSetPipelined / scTickSetPairsStream): trigger volumes do not cover tiles");
    if (flags & SC_TICK_SPLIT_PAIRS) return fail(c, "SC_TICK_TRIGGERS cannot run with SC_TICK_SPLIT_PAIRS: trigger volumes do not cover tiles");
  }
  if (flags & SC_TICK_ANCHORED_SWEEPS) {
    if (!(flags & SC_TICK_BROADPHASE)) return fail(c, "SC_TICK_ANCHORED_SWEEPS needs SC_TICK_BROADPHASE in the same run (the sweeps read this tick's bins)");
    if (!c->asweeps.count) return fail(c, "SC_TICK_ANCHORED_SWEEPS needs scTickSetAnchoredSweeps first (the set is empty)");
    if (c->neighbourMask) return fail(c, "SC_TICK_ANCHORED_SWEEPS cannot run on a context with neighbours (scTickSetTile): anchored sweeps do not cover tiles");
    if (c->pairsStream) return fail(c, "SC_TICK_ANCHORED_SWEEPS cannot run on a pipelined context (scTickSetPipelined / scTickSetPairsStream): anchored sweeps do not cover tiles");
    if (flags & SC_TICK_SPLIT_PAIRS) return fail(c, "SC_TICK_ANCHORED_SWEEPS cannot run with SC_TICK_SPLIT_PAIRS: anchored sweeps do not cover tiles");
  }
  if (c->rb.bytes && c->graphMode) return fail(c, "graph replay and the frame read-back cannot be combined");      // (an empty context's run stages a frame too)
  if (nothingToRun(c, flags)) return true;
  if (flags & SC_TICK_PRODUCE_NEXT) {
    if (!(flags & SC_TICK_XFORM)) return fail(c, "SC_TICK_PRODUCE_NEXT needs SC_TICK_XFORM (the producer rides on the end-of-tick kernel)");
    if (!c->producerKind) return fail(c, "SC_TICK_PRODUCE_NEXT needs scTickSetFrameProducer first");
  }
  if (c->pairsStream && (flags & SC_TICK_BROADPHASE) && !(flags & SC_TICK_SPLIT_PAIRS)) return fail(c, "a pairs stream is set: run the broadphase with SC_TICK_SPLIT_PAIRS + scTickRunPairs");
  if ((flags & SC_TICK_RAYS) && !(flags & SC_TICK_BROADPHASE)) return fail(c, "SC_TICK_RAYS needs SC_TICK_BROADPHASE in the same run (the queries read this tick's bins)");
  if ((flags & SC_TICK_SWEEPS) && !(flags & SC_TICK_BROADPHASE)) return fail(c, "SC_TICK_SWEEPS needs SC_TICK_BROADPHASE in the same run (the queries read this tick's bins)");
  if ((flags & SC_TICK_ANCHORED_RAYS) && !(flags & SC_TICK_BROADPHASE)) return fail(c, "SC_TICK_ANCHORED_RAYS needs SC_TICK_BROADPHASE in the same run (the queries read this tick's bins)");
  if ((flags & SC_TICK_SORT_DRAWS) && !c->sort.pipeline) return fail(c, "SC_TICK_SORT_DRAWS needs scTickSetDrawSortTable first");
  if ((flags & (SC_TICK_RAYS | SC_TICK_ANCHORED_RAYS)) && c->rayShapes == SC_TICK_RAY_SHAPES_EXACT && c->pairsStream)
    return fail(c, "SC_TICK_RAY_SHAPES_EXACT cannot run on a pipelined context (scTickSetPipelined / scTickSetPairsStream): its rays are cast when the matrices may be the next tick's");
  if ((flags & SC_TICK_SWEEPS) && c->sweepShapes == SC_TICK_SWEEP_SHAPES_EXACT && c->pairsStream)
    return fail(c, "SC_TICK_SWEEP_SHAPES_EXACT cannot run on a pipelined context (scTickSetPipelined / scTickSetPairsStream): its sweeps are cast when the matrices may be the next tick's");
  if ((flags & SC_TICK_BROADPHASE) && (flags & SC_TICK_SPLIT_PAIRS) && c->neighbourMask) {
    // every message of THIS tick parity needs its buffers: a missing one would make the pack skip that neighbour silently
    const DeviceState ds = stateFor(c, c->parity);
    for (uint32_t d = 0; d < 8; ++d)
      if (((c->neighbourMask >> d) & 1u) && (!ds.borderSend[d] || !ds.borderRecv[d]))
        return fail(c, "border buffers of this tick parity are not bound (scTickBindBorderBuffers / scTickBindBorderBuffersParity / scTickCommInit)");
  }
  return true;
}

// Decide everything about an accepted run of `flags`, leaving the context's persistent state as it is (commitPlan applies it).  What it
// does touch are memos, not decisions: worldCanPair's answer and the span-closed state (fillParams).
static TickPlan planTick(ScTickContext* c, uint32_t flags)
{
  TickPlan plan;
  plan.rec.flags = flags;
  // (a quiet tick keeps the flag in `flags` -- scTickReadPairs answers, with the empty set -- and everything below goes by `run`)
  plan.rec.quiet = quietTick(c, flags);
  const uint32_t run = plan.run = plan.rec.quiet ? (flags & ~(uint32_t)SC_TICK_BROADPHASE) : flags;
  TickParams& p = plan.p;
  fillParams(c, run, p, plan.grid);
  if (plan.rec.quiet) p.parity = 0u;                   // (no kernel of it reads the word; its graph is one whatever parity the binning ticks have reached)
  plan.rec.tail = (p.flags & kFlagTailOwnsDirty) != 0; plan.rec.topo = (p.flags & kFlagTopoClasses) != 0;
  if ((run & SC_TICK_BROADPHASE) && c->homeEnabled) {
    // home slots: a learn tick when nothing is remembered, the world's shape changed (entities, hierarchy, layers) or the
    // slots have aged
    plan.binned = true;
    plan.homeXform = (c->levelOffsets.size() > 1) ? (run & SC_TICK_XFORM) : 0u;       // (only worlds with deep levels care)
    plan.learn = !c->homeValid || c->homeEpoch != c->topoEpoch || c->homeAge >= c->homePeriod || c->homeXform != plan.homeXform;
    p.homeMode = plan.learn ? kHomeLearn : kHomeUse;
    p.homeReset = 1u;
    p.sweepOnly = worldCanPair(c) ? 0u : 1u;
    if (p.sweepOnly) p.pairRun = pairRunFor(p.binSX * p.binSZ, c->cus, true);
    p.fastPairs = (c->fastPairs && !p.sweepOnly) ? 1u : 0u;
    // lazy records: only while nothing but this tick's own pair search reads the bins, and that search runs before the next
    // tick rewrites the world matrices (it rebuilds unwritten records from them)
    // (a pipelined pair half cannot rebuild -- the matrices are the next tick's by then -- so there only the bins that nothing in the
    //  world's declared layer vocabulary can meet stay unwritten: they are never needed)
    // (and only while the pair half is this library's to issue: with a caller-owned exchange -- scTickRun(.. | SPLIT_PAIRS), the host's
    //  transport, scTickRunPairs -- the host may upload matrices, bounds or layers, append or remove entities, or run a transform-only
    //  tick between the halves, and a rebuild would then read the world of a later moment than tick t's: every record is written)
    const bool hostBetweenHalves = (run & SC_TICK_SPLIT_PAIRS) && !c->pairsStream && !c->ownStep;
    p.lazy = (!plan.learn && c->lazyEnabled && !(run & (SC_TICK_RAYS | SC_TICK_SWEEPS | SC_TICK_ANCHORED_RAYS | SC_TICK_OVERLAPS | SC_TICK_TRIGGERS | SC_TICK_ANCHORED_SWEEPS)) && !c->sensors && !hostBetweenHalves) ? (!c->pairsStream ? 1u : (c->worldLayersKnown ? 2u : 0u)) : 0u;
    p.vocab = c->worldLayers;
    p.vocabKnown = c->worldLayersKnown ? 1u : 0u;
    // records of entities that did not move stay as they are, unless something else changed boxes since the last tick
    p.cleanStay = (!plan.learn && c->lazyEnabled && !c->pairsStream && !c->boxesTouched) ? 1u : 0u;
    plan.bins.lazy = p.lazy != 0u; plan.bins.stay = p.cleanStay != 0u; plan.bins.sweepOnly = p.sweepOnly != 0u;
  }
  // the end-of-tick launch's shape (enqueueStages' rule for who carries the compaction role): the wide form only where the launch is
  // the compaction's own
  const FramePath& path = plan.path = framePathFor(c, p.flags);
  const bool alone = path.needCompact && !(p.flags & SC_TICK_BROADPHASE);
  plan.compactG = (alone && c->wideCompact) ? compactWideGroup(p, plan.grid, c->compactForceG) : 0u;
  if (path.needCompact) compactLaunchShape(plan.grid, path.pairsNow, plan.compactG, plan.rec.compact);
  plan.rec.frame[0] = path.items; plan.rec.frame[1] = path.block;
  plan.triggers = path.pairsNow && (p.flags & kFlagTriggers) != 0u;
  plan.anchoredSweeps = path.pairsNow && (p.flags & kFlagAnchoredSweeps) != 0u;
  // the narrow phase's stages (whichever half closes the pair search): the two flags' states are there (tickAccepted); a stage behind the
  // list runs when it is enabled and what it needs runs
  if (p.flags & SC_TICK_TOUCH_EVENTS) plan.narrow |= kStageTouch;
  if (p.flags & SC_TICK_PAIR_SHAPES) {
    const uint32_t on = narrowOn(c);
    uint32_t st = kStageList | (on & (kStageContacts | kStageIslands));
    if (st & kStageContacts) st |= on & kStageManifolds;
    if (st & kStageManifolds) st |= on & kStagePersist;
    if (st & kStageIslands) st |= on & kStageSleep;
    plan.narrow |= st;
  }
  if (path.stagedEmit) plan.rec.draws = frameItems(c->rb.dBlock[frameSlot(c->rb)], c->rb.maxVisible);
  plan.sampled = tickSampled(c);                       // (events need eager launches)
  plan.replay = c->graphMode && !plan.sampled && !plan.learn;
  plan.wholeStep = plan.replay && c->captureWholeStep;
  // The carried compaction.  A pending one rides at the head of this tick's fused launch where that launch is the carry-capable instance,
  // launched eagerly; otherwise commitPlan settles it first -- its own launch ahead of everything of this tick, which is the order of two
  // ticks that never deferred.  A carrying tick writes the other copy of the words (visSel, stateFor).  Then this tick's own compaction:
  // deferred when its launch would be k_compact_wide alone behind that instance, nothing else of the tick or the context needs the
  // lists on the device or on the host behind it, and the slot that would time the launch is not being timed on this tick.
  const bool instance = !c->graphMode && carryInstance(p);
  plan.carry = c->pending.on && instance;
  plan.visSel = c->visSel ^ (plan.carry ? 1u : 0u);
  const bool slotTimed = timed(c, plan.rec.quiet ? SC_TICK_K_PAIRS : SC_TICK_K_COMPACT, plan.sampled);
  plan.defer = c->carryEnabled && instance && alone && plan.compactG != 0u && !c->pairsStream && !c->neighbourMask && !c->rb.bytes &&
               !(p.flags & (SC_TICK_DRAWS | SC_TICK_SORT_DRAWS | SC_TICK_BIND_RUNS)) && !slotTimed;
  return plan;
}

// Apply the plan to the context's persistent state, just ahead of the tick's launches: what the bins remember, the frustum's device
// copy, and the pending compaction's fate (carried: the tick writes the other copy of the visibility words; else settled now).
static int commitPlan(ScTickContext* c, const TickPlan& plan)
{
  // matrices change and the bins do not follow; a quiet tick's records go stale the same way: the next binning tick rewrites every
  // always-written slot (cleanStay 0).  The bins' counters and layer summaries stay at homeCount / homeLayers, where the last pair
  // role left them; the slots age on.
  if (plan.rec.quiet || ((plan.run & SC_TICK_XFORM) && !(plan.run & SC_TICK_BROADPHASE))) c->boxesTouched = true;
  if (plan.rec.quiet) c->homeAge++;
  if (plan.binned) {
    if (plan.learn) {
      // every bin copy must be idle and empty for a learn tick (a rare event: the streams are joined here)
      c->homeXform = plan.homeXform;
      if (c->pairsStream && !sync(c)) return 0;
      if (c->homeCountsLive) {
        for (uint32_t q = 0; q < (c->pairsStream ? c->pipeDepth : 1u); ++q) {
          const DeviceState o = stateFor(c, q);
          HIP_OK(c, hipMemsetAsync(o.binCount, 0, (size_t)c->sectors * sizeof(uint32_t), c->stream));
          HIP_OK(c, hipMemsetAsync(o.binLayers, 0, (size_t)c->sectors * sizeof(uint32_t), c->stream));
        }
      }
      c->homeValid = true; c->homeEpoch = c->topoEpoch; c->homeAge = 0; c->learnTicks++;
    } else c->homeAge++;
    c->boxesTouched = false;
    c->homeCountsLive = true;
  }
  if (c->frustumStale && (plan.run & SC_TICK_CULL)) { launchSetFrustum(c->d, c->frustum, c->stream); c->frustumStale = false; }   // outside any graph
  if (plan.carry) c->visSel = plan.visSel; else settle(c);
  return 1;
}

// The record of an accepted run (ScTickContext::last, lastBinned, lastWith), written in this one place, behind the run's launches (a run
// that a HIP error ends in commitPlan, a capture or a replay leaves the record of the run before it).  `last` whole; `lastBinned` by a
// tick that binned; of `lastWith` what belongs to a flag in `with` -- the run's flags (an empty context's run launches nothing: of the
// features only the bind runs answer for it, with zeros).
static void recordRun(ScTickContext* c, const RunRecord& rec, const BinOutcome* binned, uint32_t with, uint32_t narrow)
{
  c->last = rec;
  if (binned) c->lastBinned = *binned;
  LastWith& w = c->lastWith;
  if (with & SC_TICK_BIND_RUNS) { w.bindTouchWords = c->bind.touchWords; w.bindEmpty = nothingToRun(c, rec.flags); }
  if (with & SC_TICK_OVERLAPS) { w.overlapCount = c->overlaps.count; w.overlapMaxHits = c->overlaps.maxHits; w.overlapShapes = c->overlapShapes; }
  if (with & SC_TICK_TRIGGERS) { w.triggerCount = c->triggers.count; w.triggerMaxMembers = c->triggers.maxMembers; w.triggerMaxEvents = c->triggers.maxEvents; }
  if (with & SC_TICK_ANCHORED_SWEEPS) { w.asweepCount = c->asweeps.count; w.asweepsExact = c->sweepShapes == SC_TICK_SWEEP_SHAPES_EXACT; }
  if (with & SC_TICK_SWEEPS) w.sweepsExact = c->sweepShapes == SC_TICK_SWEEP_SHAPES_EXACT;
  if (with & SC_TICK_PAIR_SHAPES) w.narrow = narrow;
}

// The run of an empty context without a broadphase: nothing to launch, the per-tick counts read as zero.  (With the broadphase the
// stages still run -- every kernel copes with n == 0: an emptied tile of a multi-GPU world must rewrite its border messages, header-only,
// and take part in the exchange, the merge and the pair search of the boxes its neighbours send.)
static int emptyTick(ScTickContext* c, uint32_t flags)
{
  RunRecord rec;                                     // (value-initialised but for its flags and, below, the frame's block)
  rec.flags = flags;
  settle(c);                                         // (a pending compaction writes the counters: ahead of the zeros)
  HIP_OK(c, hipMemsetAsync(c->d.counters, 0, 8 * sizeof(uint32_t), c->stream));
  if (c->rb.bytes) {
    // every scTickRun ends with a frame: this one is all zeros under the next tick index, written by the host into the pinned block
    // (nothing is launched and nothing copied; the block's copy of two frames ago is waited for on the host -- a rare tick)
    ScTickContext::FrameReadback& rb = c->rb;
    const uint32_t f = frameSlot(rb);
    if (rb.inFlight[f]) HIP_OK(c, hipEventSynchronize(rb.copied[f]));
    const FrameHeader h = frameHeader(0u, 0u, 0u, 0u, 0u, 0u, (uint32_t)rb.frames, (uint32_t)(rb.frames >> 32), 0u, 0u);
    std::memcpy(rb.hBlock[f], h.w, sizeof h.w);
    HIP_OK(c, publishFrame(c, false));
    rec.frame[1] = SC_TICK_FRAME_BLOCK_HOST;
  }
  recordRun(c, rec, nullptr, flags & SC_TICK_BIND_RUNS, 0u);
  return 1;
}

// One tick, in five steps: refuse, plan, commit, launch or replay, record.
int scTickRun(ScTickContext* c, uint32_t flags)
{
  if (!c) return 0;
  if (!bind(c)) return 0;
  if (!flushLinks(c)) return 0;
  if (flags & SC_TICK_XFORM) REFUSE_WHILE_SHAPES_PENDING(c, "scTickRun with SC_TICK_XFORM");
  if (!tickAccepted(c, flags)) return 0;
  if (nothingToRun(c, flags)) return emptyTick(c, flags);
  const TickPlan plan = planTick(c, flags);
  if (!commitPlan(c, plan)) return 0;
  const TickParams& p = plan.p;
  waitParityFree(c, p);
  bool rode = false;
  if (plan.replay) {
    // whole-step capture (scTickTileStep on a tile with neighbours): the RCCL group and the pair half join the graph, so a
    // step of an in-order tile is ONE hipGraphLaunch
    const uint32_t q = plan.rec.quiet ? kMaxParity : (plan.run & SC_TICK_BROADPHASE) ? p.parity : 0u;
    if (!replayGraph(c, c->stream, c->graph[q], graphKey(c, plan, plan.wholeStep), "hipStreamEndCapture", [&] {
          enqueueStages(c, plan, true);
          if (!plan.wholeStep) return 1;
          if (!exchangeBorders(c, p.parity, c->stream, true)) return 0;
          enqueuePairHalf(c, plan, c->stream);
          return 1;
        })) return 0;
  } else rode = enqueueStages(c, plan, false);
  publishPacked(c, p, rode);
  recordRun(c, plan.rec, plan.binned ? &plan.bins : nullptr, flags, plan.narrow);
  if (plan.run & SC_TICK_BROADPHASE) {
    if ((plan.run & SC_TICK_SPLIT_PAIRS) && !plan.wholeStep) { c->pairsPending = true; c->pendingTick = plan; }
    else { c->lastParity = c->parity; c->parity ^= 1u; }           // (in-order flows alternate between two copies)
  }
  c->tickIndex++;
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, "kernel launch", e);
  return 1;
}

// the pair half of a pending tick; withExchange: the library's own RCCL group goes first (scTickTileStep).  On a pipelined
// tile with graph replay on, the half is a graph of its own on the pairs stream (captured once per tick parity, relaxed mode
// when the RCCL group is inside: it touches the communicator's resources during capture).
static int runPendingPairs(ScTickContext* c, bool withExchange)
{
  const TickPlan& tick = c->pendingTick;               // (the tick's own decisions: tickIndex and the record have moved on)
  const TickParams& pp = tick.p;
  const uint32_t q = pp.parity;
  hipStream_t ps = c->pairsStream ? c->pairsStream : c->stream;
  if (c->pairsStream) {
    if (c->graphMode && !tick.sampled && !tick.learn) {
      if (!replayGraph(c, ps, c->pairGraph[q], graphKey(c, tick, withExchange), "hipStreamEndCapture (pair half)", [&] {
            if (withExchange && !exchangeBorders(c, q, ps, true)) return 0;
            enqueuePairHalf(c, tick, ps);
            return 1;
          })) return 0;
      HIP_OK(c, hipEventRecord(c->pairsDone[q], ps));
    } else {
      // a sampled tick times its pair chain too (exchange + merge + queries + pair search, on the pairs stream): SC_TICK_K_PAIRS
      EventPair ev; const bool on = timed(c, SC_TICK_K_PAIRS, tick.sampled);
      if (on) { ev = takeEvents(c); hipEventRecord(ev.a, ps); }
      if (withExchange && !exchangeBorders(c, q, ps, false)) return 0;
      if (!enqueuePairHalf(c, tick, ps, c->pairsDone[q])) HIP_OK(c, hipEventRecord(c->pairsDone[q], ps));
      if (on) { hipEventRecord(ev.b, ps); c->times[SC_TICK_K_PAIRS].push_back(ev); }
    }
    c->pairsInFlight[q] = true;
  } else {
    if (withExchange && !exchangeBorders(c, q, ps, false)) return 0;
    Scoped s(c, SC_TICK_K_PAIRS, tick.sampled);
    enqueuePairHalf(c, tick, ps);
  }
  if (c->pairEventsResyncAgain) {                     // (in-order flows only: the pair half ran on the tick stream)
    c->pairEventsResyncAgain = false;
    c->pairsPending = false;
    if (!resyncPairEvents(c)) return 0;
  }
  c->pairsPending = false;
  c->lastParity = c->parity;
  c->parity = c->pairsStream ? (c->parity + 1u) % c->pipeDepth : (c->parity ^ 1u);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, "kernel launch", e);
  return 1;
}

int scTickRunPairs(ScTickContext* c)
{
  if (!c) return 0;
  if (!bind(c)) return 0;
  if (!c->pairsPending) return fail(c, "scTickRunPairs without a preceding scTickRun(... | SC_TICK_BROADPHASE | SC_TICK_SPLIT_PAIRS)");
  return runPendingPairs(c, false);
}

int scTickSetTile(ScTickContext* c, uint32_t rank, uint32_t neighbourMask)
{
  if (!c) return 0;
  if (rank > 127u) return fail(c, "rank must be < 128 (7 id bits)");
  // records in remembered slots carry the rank in their ids, and which slots are written on every tick depends on the ring's ownership
  if (c->rank != rank || c->neighbourMask != (neighbourMask & 0xFFu)) { c->homeValid = false; c->topoEpoch++; }
  if (c->rank != rank && (!bind(c) || !resyncPairEvents(c))) return 0;      // pair ids carry the rank: remembered pairs would name the old one
  c->rank = rank;
  c->neighbourMask = neighbourMask & 0xFFu;
  return 1;
}

int scTickSetTileGrid(ScTickContext* c, uint32_t tileX, uint32_t tileZ, uint32_t tilesX, uint32_t tilesZ)
{
  if (!c) return 0;
  if (tilesX == 0 || tilesZ == 0 || tileX >= tilesX || tileZ >= tilesZ || (uint64_t)tilesX * tilesZ > 128u) return fail(c, "tile grid: need tile < tiles and at most 128 tiles");
  c->tileX = tileX; c->tileZ = tileZ; c->tilesX = tilesX; c->tilesZ = tilesZ;
  uint32_t mask = 0;
  for (uint32_t d = 0; d < 8; ++d) {
    int dx, dz; borderDir(d, dx, dz);
    const int x = (int)tileX + dx, z = (int)tileZ + dz;
    if (x >= 0 && z >= 0 && x < (int)tilesX && z < (int)tilesZ) mask |= 1u << d;
  }
  if (c->neighbourMask != mask) { c->homeValid = false; c->topoEpoch++; }
  c->neighbourMask = mask;
  return 1;
}

uint32_t scTickBorderBytes(ScTickContext* c, uint32_t dir)
{
  if (!c || dir > 7u || !c->desc.tile_sectors_x) return 0;
  return borderWords(dir, c->desc.tile_sectors_x, c->desc.tile_sectors_z, c->borderRecs, c->halo ? 1u : 0u) * 4u;
}

int scTickSetBorderCapacity(ScTickContext* c, uint32_t recordsPerRingSector)
{
  if (!c) return 0;
  if (!c->sectors) return fail(c, "the context has no broadphase");
  if (recordsPerRingSector < 1u || recordsPerRingSector > kSectorRecMax) return fail(c, "border capacity: 1..1088 records per ring sector (a sector holds at most 64 + 1024)");
  if (c->comm) return fail(c, "scTickSetBorderCapacity must precede scTickCommInit (the library's message buffers are sized there)");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  if (recordsPerRingSector == c->borderRecs) return 1;
  if (!bind(c) || !sync(c)) return 0;
  const uint32_t before = ovfRecords(c);
  c->borderRecs = recordsPerRingSector;
  // the sector overflow list has room for every border record that finds its landing bin full: grow it with the messages
  if (ovfRecords(c) > before) {
    auto regrow = [&](float4*& spill, uint32_t*& tags) -> bool {
      if (!spill) return true;
      dfree(c, spill); dfree(c, tags); spill = nullptr; tags = nullptr;
      return dalloc(c, spill, 2u * (size_t)ovfRecords(c), false) && dalloc(c, tags, ovfRecords(c));
    };
    if (!regrow(c->d.spill, c->d.spillSector)) return 0;
    for (auto& a : c->alt) if (!regrow(a.spill, a.spillSector)) return 0;
  }
  // library-owned message buffers are allocated by scTickCommInit; caller-owned ones must be re-bound at the new scTickBorderBytes
  for (uint32_t d = 0; d < 8; ++d) {
    c->d.borderSend[d] = c->d.borderRecv[d] = nullptr;
    for (auto& a : c->alt) a.borderSend[d] = a.borderRecv[d] = nullptr;
    for (uint32_t q = 0; q < kMaxParity; ++q) for (int k = 0; k < 2; ++k) if (c->ownBorder[q][d][k]) { dfree(c, c->ownBorder[q][d][k]); c->ownBorder[q][d][k] = nullptr; }
  }
  dropCaptures(c); c->topoEpoch++;
  return 1;
}

// a captured tick half (the pack), pair half (the merge) or whole step holds the message buffers' addresses by value: a changed binding
// drops every capture, behind a sync where one exists (a graph in flight still reads the old buffers)
static bool forgetBorderCaptures(ScTickContext* c)
{
  bool any = false;
  for (const CapturedGraph& g : c->graph) any = any || g.exec;
  for (const CapturedGraph& g : c->pairGraph) any = any || g.exec;
  if (!any) return true;
  if (!bind(c) || !sync(c)) return false;
  dropCaptures(c);
  return true;
}

int scTickBindBorderBuffers(ScTickContext* c, uint32_t dir, void* send, void* recv)
{
  if (!c || dir > 7u) return c ? fail(c, "bad direction") : 0;
  bool same = c->d.borderSend[dir] == send && c->d.borderRecv[dir] == recv;
  for (auto& a : c->alt) same = same && a.borderSend[dir] == send && a.borderRecv[dir] == recv;
  if (!same && !forgetBorderCaptures(c)) return 0;
  c->d.borderSend[dir] = static_cast<uint32_t*>(send);
  c->d.borderRecv[dir] = static_cast<uint32_t*>(recv);
  for (auto& a : c->alt) { a.borderSend[dir] = static_cast<uint32_t*>(send); a.borderRecv[dir] = static_cast<uint32_t*>(recv); }
  return 1;
}

int scTickBindBorderBuffersParity(ScTickContext* c, uint32_t parity, uint32_t dir, void* send, void* recv)
{
  if (!c) return 0;
  if (dir > 7 || parity >= kMaxParity) return fail(c, "direction must be 0..7 and parity 0..3");
  uint32_t* const oldSend = parity == 0 ? c->d.borderSend[dir] : c->alt[parity - 1u].borderSend[dir];
  uint32_t* const oldRecv = parity == 0 ? c->d.borderRecv[dir] : c->alt[parity - 1u].borderRecv[dir];
  if ((oldSend != send || oldRecv != recv) && !forgetBorderCaptures(c)) return 0;
  if (parity == 0) { c->d.borderSend[dir] = static_cast<uint32_t*>(send); c->d.borderRecv[dir] = static_cast<uint32_t*>(recv); }
  else { c->alt[parity - 1u].borderSend[dir] = static_cast<uint32_t*>(send); c->alt[parity - 1u].borderRecv[dir] = static_cast<uint32_t*>(recv); }
  return 1;
}

void* scTickGetBorderBuffer(ScTickContext* c, uint32_t parity, uint32_t dir, int recv)
{
  if (!c || dir > 7u || parity >= kMaxParity) return nullptr;
  uint32_t* const* set = parity == 0 ? (recv ? c->d.borderRecv : c->d.borderSend) : (recv ? c->alt[parity - 1u].borderRecv : c->alt[parity - 1u].borderSend);
  return set[dir];
}

int scTickSetPairsStream(ScTickContext* c, void* stream)
{
  if (!c) return 0;
  if (!bind(c)) return 0;
  settle(c);
  if (!sync(c)) return 0;
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  // The two flows clear the per-parity broadphase state differently (in order: a pair kernel clears the OTHER parity for the
  // next tick; pipelined: a small kernel behind the pair kernel clears its OWN parity), so a switch in either direction
  // would leave one parity's counters, shard counters and big-box bits holding the last tick's values.  Everything is idle
  // here (synchronised above): start both parities from a clean slate.
  auto resetBroadphaseState = [&]() -> bool {
    if (!c->sectors) return true;
    hipError_t e = hipMemsetAsync(c->d.counters + kCtrPar, 0, (kCounterWords - kCtrPar) * sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d.pairShardCount, 0, (kMaxParity + 1u) * kPairShards * kShardStride * sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d.binCount, 0, (size_t)c->sectors * sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d.binLayers, 0, (size_t)c->sectors * sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d.ovfLo, 0xFF, (size_t)c->sectors * sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->d.ovfHi, 0, (size_t)c->sectors * sizeof(uint32_t), c->stream);
    for (auto& a : c->alt) {
      if (e == hipSuccess && a.binCount) e = hipMemsetAsync(a.binCount, 0, (size_t)c->sectors * sizeof(uint32_t), c->stream);
      if (e == hipSuccess && a.binLayers) e = hipMemsetAsync(a.binLayers, 0, (size_t)c->sectors * sizeof(uint32_t), c->stream);
      if (e == hipSuccess && a.ovfLo) e = hipMemsetAsync(a.ovfLo, 0xFF, (size_t)c->sectors * sizeof(uint32_t), c->stream);
      if (e == hipSuccess && a.ovfHi) e = hipMemsetAsync(a.ovfHi, 0, (size_t)c->sectors * sizeof(uint32_t), c->stream);
    }
    if (e != hipSuccess) return fail(c, "hipMemsetAsync (broadphase state)", e);
    c->parity = 0; c->lastParity = 0;
    c->homeValid = false; c->homeCountsLive = false;      // every bin copy is empty again: the next tick learns its slots afresh
    return sync(c);
  };
  if (!stream) {
    if (c->pairsStream && !resetBroadphaseState()) return 0;
    c->pairsStream = nullptr; for (bool& f : c->pairsInFlight) f = false; c->topoEpoch++;
    return 1;
  }
  if (!c->sectors) return fail(c, "the context has no broadphase");
  for (uint32_t q = 1; q < c->pipeDepth; ++q) {
    ScTickContext::AltSet& a = c->alt[q - 1u];
    const size_t N = c->cap;
    if (!a.bins && (!dalloc(c, a.binCount, c->sectors) || !dalloc(c, a.binLayers, c->sectors) ||
        !dalloc(c, a.bins, (size_t)c->sectors * kBinCap * 2u, false) || !dalloc(c, a.bigList, (N + 8u * kBorderBigCap) * 2u, false) ||
        !dalloc(c, a.spill, 2u * (size_t)ovfRecords(c), false) || !dalloc(c, a.spillSector, ovfRecords(c)) || !dalloc(c, a.ovfLo, c->sectors, false) || !dalloc(c, a.ovfHi, c->sectors))) return 0;
    // (border buffers: scTickBindBorderBuffers writes every copy's slots itself, scTickBindBorderBuffersParity and
    //  scTickCommInit bind per parity -- nothing is inherited here.  Round 2 copied parity 1's pointers over a parity whose
    //  direction 0 was unbound, which is every tile without a (-1,-1) neighbour: parities 1..3 then shared one message set.)
  }
  for (uint32_t k = 0; k < kMaxParity; ++k) {
    if (!c->packed[k]) HIP_OK(c, hipEventCreateWithFlags(&c->packed[k], hipEventDisableTiming | hipEventReleaseToDevice));
    if (!c->pairsDone[k]) HIP_OK(c, hipEventCreateWithFlags(&c->pairsDone[k], hipEventDisableTiming | hipEventReleaseToDevice));
  }
  if (!c->pairsStream && !resetBroadphaseState()) return 0;
  c->pairsStream = static_cast<hipStream_t>(stream);
  for (bool& f : c->pairsInFlight) f = false;
  c->topoEpoch++;
  return 1;
}

int scTickSetStream(ScTickContext* c, void* stream, int external)
{
  if (!c) return 0;
  if (!bind(c)) return 0;
  settle(c);                                           // (on the stream the deferring tick ran on)
  if (!sync(c)) return 0;
  dropGraphs(c->graph);
  c->stream = external ? static_cast<hipStream_t>(stream) : c->ownStream;
  return 1;
}

int scTickSynchronize(ScTickContext* c)
{
  if (!c) return 0;
  if (!bind(c)) return 0;
  settle(c);
  return sync(c) ? 1 : 0;
}

int scTickNudgeRootsX(ScTickContext* c, float dx)
{
  if (!c) return 0;
  if (!bind(c) || !flushLinks(c)) return 0;
  Scoped s(c, SC_TICK_K_NUDGE, tickSampled(c));
  launchNudgeRootsX(c->d, c->n, dx, c->stream);
  return 1;
}

int scTickUploadMovers(ScTickContext* c, uint32_t first, uint32_t count, const uint8_t* kind, const float* vel, const float* lo, const float* hi)
{
  if (!c || !kind || !vel || !lo || !hi) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  DeviceState& d = c->d;
  if (!d.moverKind) {
    const size_t N = c->cap;
    if (!dalloc(c, d.moverKind, N) || !dalloc(c, d.mvx, N) || !dalloc(c, d.mvz, N) || !dalloc(c, d.mlox, N) ||
        !dalloc(c, d.mloz, N) || !dalloc(c, d.mhix, N) || !dalloc(c, d.mhiz, N)) return 0;
  }
  if (!count) return 1;
  std::vector<uint32_t> k32(count);
  std::vector<float> a[6];
  for (auto& v : a) v.resize(count);
  for (uint32_t i = 0; i < count; ++i) {
    if (kind[i] > 2) return fail(c, "mover kind must be 0 (none), 1 (vehicle: wrap) or 2 (ped: reflect)");
    k32[i] = kind[i];
    a[0][i] = vel[2 * i]; a[1][i] = vel[2 * i + 1]; a[2][i] = lo[2 * i]; a[3][i] = lo[2 * i + 1]; a[4][i] = hi[2 * i]; a[5][i] = hi[2 * i + 1];
  }
  float* dst[6] = { d.mvx, d.mvz, d.mlox, d.mloz, d.mhix, d.mhiz };
  if (!h2d(c, d.moverKind + first, k32.data(), (size_t)count * 4u)) return 0;
  for (int q = 0; q < 6; ++q) if (!h2d(c, dst[q] + first, a[q].data(), (size_t)count * 4u)) return 0;
  return sync(c) ? 1 : 0;
}

int scTickAdvanceMovers(ScTickContext* c, float dt)
{
  if (!c) return 0;
  if (!bind(c) || !flushLinks(c)) return 0;
  if (!c->d.moverKind) return fail(c, "no movers uploaded");
  Scoped s(c, SC_TICK_K_NUDGE, tickSampled(c));
  launchAdvanceMovers(c->d, c->n, dt, 1.0f - std::exp(-2.5f * dt), c->trafficMult, c->stream);
  return 1;
}

int scTickSetFrameProducer(ScTickContext* c, uint32_t kind, float param)
{
  if (!c) return 0;
  if (kind > 2u) return fail(c, "producer kind must be 0 (none), 1 (nudge roots) or 2 (advance movers)");
  if (kind == 2u && !c->d.moverKind) return fail(c, "no movers uploaded");
  if (!bind(c) || !sync(c)) return 0;
  dropGraphs(c->graph);                                   // the captured frame changes
  c->producerKind = kind;
  c->producerParam = param;
  return 1;
}

int scTickReadMoverVelocities(ScTickContext* c, uint32_t first, uint32_t count, float* vel)
{
  if (!c || !vel) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!c->d.moverKind) return fail(c, "no movers uploaded");
  if (!count) return 1;
  std::vector<float> x(count), z(count);
  if (!d2h(c, x.data(), c->d.mvx + first, (size_t)count * 4u) || !d2h(c, z.data(), c->d.mvz + first, (size_t)count * 4u) || !sync(c)) return 0;
  for (uint32_t i = 0; i < count; ++i) { vel[2 * i] = x[i]; vel[2 * i + 1] = z[i]; }
  return 1;
}

int scTickGetCounts(ScTickContext* c, ScTickCounts* out)
{
  if (!c || !out) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !joinPairs(c)) return 0;
  settle(c);
  uint32_t k[kCounterWords] = {};
  if (!d2h(c, k, c->d.counters, sizeof k) || !sync(c)) return 0;
  std::memset(out, 0, sizeof *out);
  const uint32_t resultSlot = c->lastParity;      // (a pipelined tile's parity keeps its results until the tick before its next use clears it)
  const uint32_t* bp = k + kCtrPar + 8u * resultSlot;
  out->entities = c->n;
  out->renderables_total = k[6];
  out->visible = k[0];
  out->culled = k[1];
  if (c->sectors && (c->last.flags & SC_TICK_BROADPHASE) && !c->pairsPending && !c->last.quiet) {      // (a quiet tick: 0 pairs by construction)
    TickParams pp{}; pp.maxPairs = c->maxPairs;
    launchGatherPairs(c->d, pp, resultSlot, c->dPairsOut, c->dPairTotal, c->stream);
    uint32_t tot[2] = {};
    if (!d2h(c, tot, c->dPairTotal, sizeof tot) || !sync(c)) return 0;
    out->pairs = tot[0];
    out->pairs_truncated = tot[1];
  }
  out->bin_overflow = bp[kCtrSpill];                 // length of the sector overflow list (own boxes + border records that landed in a full bin)
  out->big_boxes = (c->last.flags & SC_TICK_SPLIT_PAIRS) ? bp[kCtrBigLocal] : bp[kCtrBig];
  out->border_lost = bp[kCtrBorderLost];
  if (c->sectors) {
    uint32_t lc[1u + 2u * kMaxParity] = {};
    if (!d2h(c, lc, c->d.lazyCtl, sizeof lc) || !sync(c)) return 0;
    out->vocabulary_violations = lc[1u + kMaxParity + resultSlot];
  }
  out->draws_emitted = k[4];
  out->draws_dropped = k[5];
  out->draws_sorted = (c->last.flags & SC_TICK_SORT_DRAWS) ? k[kCtrDrawsSorted] : 0u;
  out->max_depth = c->maxDepth;
  out->unreachable = c->unreachable;
  out->relinks = c->relinks;
  return 1;
}

static int readIndexList(ScTickContext* c, const uint32_t* dev, uint32_t counterSlot, uint32_t* out, uint32_t cap, uint32_t* count)
{
  if (!c || !count) return c ? fail(c, "null argument") : 0;
  if (!bind(c)) return 0;
  settle(c);
  uint32_t k[16] = {};
  if (!d2h(c, k, c->d.counters, sizeof k) || !sync(c)) return 0;
  const uint32_t total = k[counterSlot];
  *count = total;
  const uint32_t take = std::min(total, cap);
  if (take && out) { if (!d2h(c, out, dev, (size_t)take * 4u) || !sync(c)) return 0; }
  return 1;
}

int scTickReadVisible(ScTickContext* c, uint32_t* out, uint32_t cap, uint32_t* count)
{
  return c ? readIndexList(c, c->d.visibleIdx, 0, out, cap, count) : 0;
}

int scTickReadCulled(ScTickContext* c, uint32_t* out, uint32_t cap, uint32_t* count)
{
  if (!c) return 0;
  if (!(c->last.flags & SC_TICK_CULLED_LIST)) return fail(c, "the last scTickRun did not request SC_TICK_CULLED_LIST");
  return readIndexList(c, c->d.culledIdx, 1, out, cap, count);
}

int scTickReadVisibilityBits(ScTickContext* c, uint64_t* words, uint32_t wordCap)
{
  if (!c || !words) return c ? fail(c, "null argument") : 0;
  if (!bind(c)) return 0;
  const uint32_t nWords = (c->n + 63u) / 64u;
  if (wordCap < nWords) return fail(c, "word capacity too small");
  // (the copy the last tick wrote: stateFor.  A pending compaction only reads it -- nothing to settle)
  if (nWords && (!d2h(c, words, stateFor(c, 0u).vis, (size_t)nWords * 8u) || !sync(c))) return 0;
  if (c->n & 63u) words[nWords - 1] &= (1ull << (c->n & 63u)) - 1ull;
  return 1;
}

int scTickReadWorldMatrices(ScTickContext* c, uint32_t first, uint32_t count, float* m16)
{
  if (!c || !m16) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!count) return 1;
  std::vector<float4> r0(count), r1(count), r2(count);
  if (!d2h(c, r0.data(), c->d.w0 + first, (size_t)count * 16u) || !d2h(c, r1.data(), c->d.w1 + first, (size_t)count * 16u) ||
      !d2h(c, r2.data(), c->d.w2 + first, (size_t)count * 16u) || !sync(c)) return 0;
  for (uint32_t i = 0; i < count; ++i) {
    const float rows[12] = { r0[i].x, r0[i].y, r0[i].z, r0[i].w, r1[i].x, r1[i].y, r1[i].z, r1[i].w, r2[i].x, r2[i].y, r2[i].z, r2[i].w };
    rowsToMat4(rows, m16 + 16 * (size_t)i);
  }
  return 1;
}

int scTickReadWorldMatricesIndexed(ScTickContext* c, const uint32_t* idx, uint32_t count, float* m16)
{
  if (!c || !m16 || (!idx && count)) return c ? fail(c, "null argument") : 0;
  if (!bind(c)) return 0;
  if (!count) return 1;
  for (uint32_t i = 0; i < count; ++i) if (idx[i] >= c->n) return fail(c, "dense index out of range");
  if (!needScratch(c, count)) return 0;
  if (!h2d(c, c->dIdx, idx, (size_t)count * 4u)) return 0;
  launchGatherRows(c->d, c->dIdx, count, c->dRows, c->stream);
  std::vector<float> rows((size_t)count * 12);
  if (!d2h(c, rows.data(), c->dRows, rows.size() * 4u) || !sync(c)) return 0;
  for (uint32_t i = 0; i < count; ++i) rowsToMat4(rows.data() + 12 * (size_t)i, m16 + 16 * (size_t)i);
  return 1;
}

int scTickReadDirty(ScTickContext* c, uint32_t first, uint32_t count, uint8_t* out)
{
  if (!c || !out) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!count) return 1;
  const uint32_t w0 = first >> 5, w1 = (first + count + 31u) >> 5;
  std::vector<uint32_t> words(w1 - w0);
  if (!d2h(c, words.data(), c->d.dirty + w0, words.size() * 4u) || !sync(c)) return 0;
  for (uint32_t i = 0; i < count; ++i) { const uint32_t g = first + i; out[i] = (words[(g >> 5) - w0] >> (g & 31u)) & 1u; }
  return 1;
}

int scTickReadPositions(ScTickContext* c, uint32_t first, uint32_t count, float* pos3)
{
  if (!c || !pos3) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!count) return 1;
  std::vector<float> x(count), y(count), z(count);
  if (!d2h(c, x.data(), c->d.px + first, (size_t)count * 4u) || !d2h(c, y.data(), c->d.py + first, (size_t)count * 4u) ||
      !d2h(c, z.data(), c->d.pz + first, (size_t)count * 4u) || !sync(c)) return 0;
  for (uint32_t i = 0; i < count; ++i) { pos3[3 * i] = x[i]; pos3[3 * i + 1] = y[i]; pos3[3 * i + 2] = z[i]; }
  return 1;
}

int scTickReadWorldAabbs(ScTickContext* c, uint32_t first, uint32_t count, float* min3, float* max3)
{
  if (!c || !min3 || !max3) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if ((c->last.flags & (SC_TICK_BROADPHASE | SC_TICK_DENSE_AABBS)) != (SC_TICK_BROADPHASE | SC_TICK_DENSE_AABBS))
    return fail(c, "the last scTickRun did not request SC_TICK_BROADPHASE | SC_TICK_DENSE_AABBS");
  if (!count) return 1;
  std::vector<float4> a(count), b(count);
  if (!d2h(c, a.data(), c->d.aabbMin + first, (size_t)count * 16u) || !d2h(c, b.data(), c->d.aabbMax + first, (size_t)count * 16u) || !sync(c)) return 0;
  for (uint32_t i = 0; i < count; ++i) {
    min3[3 * i] = a[i].x; min3[3 * i + 1] = a[i].y; min3[3 * i + 2] = a[i].z;
    max3[3 * i] = b[i].x; max3[3 * i + 1] = b[i].y; max3[3 * i + 2] = b[i].z;
  }
  return 1;
}

int scTickReadPairs(ScTickContext* c, uint32_t* pairs2, uint32_t cap, uint32_t* count)
{
  if (!c || !count) return c ? fail(c, "null argument") : 0;
  if (!bind(c)) return 0;
  if (!lastRunResult(c, SC_TICK_BROADPHASE, "the last scTickRun did not request SC_TICK_BROADPHASE", true, nullptr,
                     "scTickRunPairs has not been called for the last tick", true, nullptr)) return 0;
  if (c->last.quiet) { *count = 0; return 1; }      // no two colliders of that tick's world could meet: the empty set, whatever the bins' copies hold
  // the pair list is kept in per-shard segments on the device; gather them into one list first
  TickParams pp{}; pp.maxPairs = c->maxPairs;
  const uint32_t slot = c->lastParity;
  launchGatherPairs(c->d, pp, slot, c->dPairsOut, c->dPairTotal, c->stream);
  uint32_t tot[2] = {};
  if (!d2h(c, tot, c->dPairTotal, sizeof tot) || !sync(c)) return 0;
  *count = tot[0];
  // each shard keeps at most maxPairs / 64 pairs; recount what the gather could place
  std::vector<uint32_t> sc((kMaxParity + 1u) * kPairShards * kShardStride);
  if (!d2h(c, sc.data(), c->d.pairShardCount, sc.size() * sizeof(uint32_t)) || !sync(c)) return 0;
  uint32_t placed = 0;
  const uint32_t shardCap = c->maxPairs / kPairShards;
  for (uint32_t s = 0; s < kPairShards; ++s) placed += std::min(sc[(slot * kPairShards + s) * kShardStride], shardCap);
  const uint32_t take = std::min(placed, cap);
  if (take && pairs2) { if (!d2h(c, pairs2, c->dPairsOut, (size_t)take * 8u) || !sync(c)) return 0; }
  return 1;
}

int scTickReadDraws(ScTickContext* c, ScTickDrawItem* items, uint32_t cap, uint32_t* count)
{
  if (!c || !count) return c ? fail(c, "null argument") : 0;
  if (!bind(c)) return 0;
  if (!(c->last.flags & SC_TICK_DRAWS)) return fail(c, "the last scTickRun did not request SC_TICK_DRAWS");
  settle(c);
  uint32_t k[16] = {};
  if (!d2h(c, k, c->d.counters, sizeof k) || !sync(c)) return 0;
  const uint32_t have = (c->last.flags & SC_TICK_SORT_DRAWS) ? k[kCtrDrawsSorted] : k[4];
  *count = have;
  const uint32_t take = std::min(have, cap);
  if (take && items) { if (!d2h(c, items, c->last.draws ? c->last.draws : c->dDraws, (size_t)take * sizeof(ScTickDrawItem)) || !sync(c)) return 0; }
  return 1;
}

// (one read-back path for both hit types: they share the 48-byte layout)
static int readQueryHits(ScTickContext* c, uint32_t flag, const char* notRequested, const char* pending, const void* src, uint32_t have,
                         void* hits, uint32_t cap, uint32_t* count)
{
  if (!c || !count) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !lastRunResult(c, flag, notRequested, true, nullptr, pending, true, nullptr)) return 0;
  *count = have;
  const uint32_t take = std::min(have, cap);
  if (take && hits) { if (!d2h(c, hits, src, (size_t)take * sizeof(RayHit48)) || !sync(c)) return 0; }
  return 1;
}

int scTickSetRayQueries(ScTickContext* c, uint32_t count, const float* origin3, const float* dir3, const float* maxDist, const uint32_t* mask)
{
  if (!c) return 0;
  if (count && (!origin3 || !dir3 || !maxDist || !mask)) return fail(c, "null argument");
  // the kernel never sees a value it has no answer for: checked before anything changes, so a refused call leaves the previous set in place
  // (a negative max_dist and a direction of |dir|^2 <= 1e-6 have an answer: a miss)
  std::vector<float4> o(count), dd(count);
  for (uint32_t i = 0; i < count; ++i) {
    o[i] = make_float4(origin3[3 * i], origin3[3 * i + 1], origin3[3 * i + 2], maxDist[i]);
    float w; std::memcpy(&w, &mask[i], 4);
    dd[i] = make_float4(dir3[3 * i], dir3[3 * i + 1], dir3[3 * i + 2], w);
    const float v[7] = { o[i].x, o[i].y, o[i].z, o[i].w, dd[i].x, dd[i].y, dd[i].z };
    for (float x : v) if (!std::isfinite(x)) return fail(c, "ray queries: origin, dir and max_dist must be finite");
    if (!std::isfinite((dd[i].x * dd[i].x + dd[i].y * dd[i].y) + dd[i].z * dd[i].z)) return fail(c, "ray queries: the direction's squared length overflows fp32");
  }
  if (!bind(c) || !sync(c)) return 0;
  if (!growBatch(c, c->rayCap, c->rays.count, count, batchArray(c->rays.origin), batchArray(c->rays.dir), batchArray(c->rays.hits, true))) return 0;
  if (!count) return 1;
  if (!h2d(c, const_cast<float4*>(c->rays.origin), o.data(), (size_t)count * 16u) ||
      !h2d(c, const_cast<float4*>(c->rays.dir), dd.data(), (size_t)count * 16u)) return 0;
  return sync(c) ? 1 : 0;
}

int scTickReadRayHits(ScTickContext* c, ScTickRayHit* hits, uint32_t cap, uint32_t* count)
{
  static_assert(sizeof(ScTickRayHit) == sizeof(RayHit48), "ray hit layouts differ");
  return readQueryHits(c, SC_TICK_RAYS, "the last scTickRun did not request SC_TICK_RAYS", "ray hits are ready after scTickRunPairs",
                       c ? c->rays.hits : nullptr, c ? c->rays.count : 0u, hits, cap, count);
}

int scTickSetSweepQueries(ScTickContext* c, uint32_t count, const float* start3, const float* end3, const float* radius, const float* halfHeight,
                          const uint32_t* mask, const uint32_t* skipId)
{
  if (!c) return 0;
  if (count && (!start3 || !end3 || !radius || !halfHeight || !mask)) return fail(c, "null argument");
  // the kernel never sees a value it has no answer for: checked before anything changes, so a refused call leaves the previous set in place
  std::vector<float4> a(count), b(count); std::vector<uint2> f(count);
  for (uint32_t i = 0; i < count; ++i) {
    a[i] = make_float4(start3[3 * i], start3[3 * i + 1], start3[3 * i + 2], radius[i]);
    b[i] = make_float4(end3[3 * i], end3[3 * i + 1], end3[3 * i + 2], halfHeight[i]);
    f[i] = make_uint2(mask[i], skipId ? skipId[i] : 0xFFFFFFFFu);
    const float v[8] = { a[i].x, a[i].y, a[i].z, a[i].w, b[i].x, b[i].y, b[i].z, b[i].w };
    for (float x : v) if (!std::isfinite(x)) return fail(c, "sweep queries: start, end, radius and half_height must be finite");
    if (radius[i] < 0.0f) return fail(c, "sweep queries: radius must be >= 0");
    const float dx = b[i].x - a[i].x, dy = b[i].y - a[i].y, dz = b[i].z - a[i].z;
    if (!std::isfinite((dx * dx + dy * dy) + dz * dz)) return fail(c, "sweep queries: the segment's squared length overflows fp32");
  }
  if (!bind(c) || !sync(c)) return 0;
  if (!growBatch(c, c->sweepCap, c->sweeps.count, count, batchArray(c->sweeps.start), batchArray(c->sweeps.end), batchArray(c->sweeps.filter),
                 batchArray(c->sweeps.hits, true))) return 0;
  if (!count) return 1;
  if (!h2d(c, const_cast<float4*>(c->sweeps.start), a.data(), (size_t)count * 16u) ||
      !h2d(c, const_cast<float4*>(c->sweeps.end), b.data(), (size_t)count * 16u) ||
      !h2d(c, const_cast<uint2*>(c->sweeps.filter), f.data(), (size_t)count * 8u)) return 0;
  return sync(c) ? 1 : 0;
}

int scTickReadSweepHits(ScTickContext* c, ScTickSweepHit* hits, uint32_t cap, uint32_t* count)
{
  static_assert(sizeof(ScTickSweepHit) == sizeof(SweepHit48) && offsetof(ScTickSweepHit, travel) == offsetof(SweepHit48, travel), "sweep hit layouts differ");
  return readQueryHits(c, SC_TICK_SWEEPS, "the last scTickRun did not request SC_TICK_SWEEPS", "sweep hits are ready after scTickRunPairs",
                       c ? c->sweeps.hits : nullptr, c ? c->sweeps.count : 0u, hits, cap, count);
}

int scTickSetOverlapQueries(ScTickContext* c, uint32_t count, const uint8_t* type, const float* mat16, const float* halfExtents3, const float* radius,
                            const float* halfHeight, const uint32_t* mask, const uint32_t* skipId, uint32_t maxHits, uint32_t shapes)
{
  static_assert(sizeof(ScTickOverlapInfo) == 8u * sizeof(uint32_t), "ScTickOverlapInfo is eight words");
  if (!c) return 0;
  if (count && (!type || !mat16 || !halfExtents3 || !radius || !halfHeight || !mask)) return fail(c, "null argument");
  if (shapes != SC_TICK_OVERLAP_SHAPES_AABB && shapes != SC_TICK_OVERLAP_SHAPES_EXACT) return fail(c, "unknown overlap shape mode (SC_TICK_OVERLAP_SHAPES_*)");
  if (count && !maxHits) return fail(c, "overlap queries: max_hits must be at least 1");
  if ((uint64_t)count * maxHits > 0x3FFFFFFFull) return fail(c, "overlap queries: count * max_hits does not fit (at most 2^30 - 1 id slots)");
  // the kernel never sees a value it has no answer for: checked before anything changes, so a refused call leaves the previous set in place
  std::vector<float4> v((size_t)count * kOverlapVolumeWords);
  for (uint32_t i = 0; i < count; ++i) {
    const float* m = mat16 + 16u * (size_t)i;                 // column-major: m[col * 4 + row]
    const uint8_t t = type[i];
    if (t != SC_TICK_COLLIDER_BOX && t != SC_TICK_COLLIDER_SPHERE && t != SC_TICK_COLLIDER_CAPSULE)
      return fail(c, "overlap queries: a volume's type is SC_TICK_COLLIDER_BOX, _SPHERE or _CAPSULE");
    const float he[3] = { halfExtents3[3 * (size_t)i], halfExtents3[3 * (size_t)i + 1], halfExtents3[3 * (size_t)i + 2] };
    const float values[5] = { he[0], he[1], he[2], radius[i], halfHeight[i] };
    bool finite = true;
    for (float x : values) finite = finite && std::isfinite(x);
    for (int col = 0; col < 4; ++col) for (int row = 0; row < 3; ++row) finite = finite && std::isfinite(m[col * 4 + row]);
    if (!finite) return fail(c, "overlap queries: mat16, half_extents, radius and half_height must be finite");
    float4* q = &v[(size_t)i * kOverlapVolumeWords];
    for (int row = 0; row < 3; ++row) q[row] = make_float4(m[row], m[4 + row], m[8 + row], m[12 + row]);
    // the record as scTickUploadColliders stores it
    const float hh = halfHeight[i] < 0.0f ? 0.0f : halfHeight[i];
    q[3] = t == SC_TICK_COLLIDER_BOX ? make_float4(he[0], he[1], he[2], 0.0f)
         : t == SC_TICK_COLLIDER_SPHERE ? make_float4(0.0f, 0.0f, 0.0f, radius[i]) : make_float4(0.0f, hh, 0.0f, radius[i]);
    const uint32_t words[4] = { t, mask[i], skipId ? skipId[i] : 0xFFFFFFFFu, 0u };
    std::memcpy(&q[4], words, sizeof words);
  }
  if (!bind(c)) return 0;
  OverlapQueryState& o = c->overlaps;
  // The same count, max_hits and mode as the current set: only the volumes are rewritten, behind whatever is queued -- no epoch bump, so no
  // learn tick, and a captured graph (which holds the buffers, the two sizes and the kernel instance) stays valid.
  const uint32_t perVolume = count ? maxHits : 0u;             // (a cleared set holds no slots whatever max_hits says)
  if (count != o.count || perVolume != o.maxHits || shapes != c->overlapShapes) {
    if (!sync(c)) return 0;
    const size_t slots = (size_t)count * perVolume;
    auto empty = [&] { dfree(c, o.ids); o.ids = nullptr; c->overlapIdCap = 0; o.count = 0; o.maxHits = 0; };
    if (slots > c->overlapIdCap) {                             // the id rows: kept within their capacity, allocated anew beyond it
      empty();
      if (!dalloc(c, o.ids, std::max<size_t>(slots, 1024u))) return 0;
      c->overlapIdCap = std::max<size_t>(slots, 1024u);
    }
    if (!growBatch(c, c->overlapCap, o.count, count, batchArray(o.volume, false, kOverlapVolumeWords), batchArray(o.counts, true), batchArray(o.tally, true))) { empty(); return 0; }
    o.maxHits = perVolume;
    c->overlapShapes = shapes;
  }
  if (!count) return 1;
  if (!h2d(c, const_cast<float4*>(o.volume), v.data(), v.size() * sizeof(float4))) return 0;
  return sync(c) ? 1 : 0;
}

int scTickReadOverlapHits(ScTickContext* c, uint32_t* counts, uint32_t* ids, uint32_t queryCapacity, ScTickOverlapInfo* info)
{
  if (!c) return 0;
  // the set is as the run left it while count and max_hits are what that run answered (a same-size call only rewrites volumes)
  const bool stands = c->overlaps.count == c->lastWith.overlapCount && c->overlaps.maxHits == c->lastWith.overlapMaxHits;
  if (!bind(c) || !lastRunResult(c, SC_TICK_OVERLAPS, "the last scTickRun did not request SC_TICK_OVERLAPS", true, nullptr,
                                 "overlap hits are ready after scTickRunPairs", stands, "the overlap set was re-sized since the last run with SC_TICK_OVERLAPS: its results are gone")) return 0;
  const OverlapQueryState& o = c->overlaps;
  // the report's sums are formed here, from the per-volume words the waves wrote: no wave adds to a shared word
  const bool exact = c->lastWith.overlapShapes == SC_TICK_OVERLAP_SHAPES_EXACT;
  std::vector<uint32_t> perVolume(o.count);
  std::vector<uint2> tally(exact ? o.count : 0u);
  if (!d2h(c, perVolume.data(), o.counts, (size_t)o.count * sizeof(uint32_t))) return 0;
  if (exact && !d2h(c, tally.data(), o.tally, (size_t)o.count * sizeof(uint2))) return 0;
  const uint32_t take = std::min(o.count, queryCapacity);
  if (take && ids && !d2h(c, ids, o.ids, (size_t)take * o.maxHits * sizeof(uint32_t))) return 0;
  if (!sync(c)) return 0;
  if (take && counts) std::memcpy(counts, perVolume.data(), (size_t)take * sizeof(uint32_t));
  if (info) {
    uint64_t hits = 0, refined = 0, kept = 0; uint32_t truncated = 0;
    for (uint32_t n : perVolume) { hits += n; truncated += n > o.maxHits ? 1u : 0u; }
    for (const uint2& t : tally) { refined += t.x; kept += t.y; }
    info->queries = o.count; info->max_hits = o.maxHits; info->hits = (uint32_t)std::min<uint64_t>(hits, 0xFFFFFFFFull);
    info->truncated_queries = truncated; info->refined = (uint32_t)std::min<uint64_t>(refined, 0xFFFFFFFFull);
    info->kept_as_boxes = (uint32_t)std::min<uint64_t>(kept, 0xFFFFFFFFull); info->shapes = c->lastWith.overlapShapes; info->pad = 0u;
  }
  return 1;
}

int scTickSetTriggerVolumes(ScTickContext* c, uint32_t count, const uint32_t* anchor, const uint8_t* type, const float* localMat16, const float* halfExtents3,
                            const float* radius, const float* halfHeight, const uint32_t* mask, const uint8_t* skipSelf, uint32_t maxMembers,
                            uint32_t maxEvents, uint32_t shapes)
{
  static_assert(sizeof(ScTickTriggerInfo) == 8u * sizeof(uint32_t), "ScTickTriggerInfo is eight words");
  static_assert(kTriggerRowCap == SC_TICK_TRIGGER_MAX_MEMBERS, "the trigger row caps differ");
  if (!c) return 0;
  if (count && (!anchor || !type || !localMat16 || !halfExtents3 || !radius || !halfHeight || !mask)) return fail(c, "null argument");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  if (shapes != SC_TICK_OVERLAP_SHAPES_AABB && shapes != SC_TICK_OVERLAP_SHAPES_EXACT) return fail(c, "trigger volumes: unknown shape mode (SC_TICK_OVERLAP_SHAPES_*)");
  if (count && !maxMembers) return fail(c, "trigger volumes: max_members must be at least 1");
  if (maxMembers > kTriggerRowCap) return fail(c, "trigger volumes: max_members exceeds SC_TICK_TRIGGER_MAX_MEMBERS (a wave's two rows fit its LDS)");
  if ((uint64_t)count * maxMembers > 0x3FFFFFFFull) return fail(c, "trigger volumes: count * max_members does not fit (at most 2^30 - 1 id slots)");
  if (maxEvents > (1u << 27)) return fail(c, "trigger volumes: at most 2^27 events per list");
  // the kernel never sees a value it has no answer for: checked before anything changes, so a refused call leaves the previous set in place
  std::vector<float4> v((size_t)count * kOverlapVolumeWords);
  std::vector<uint2> an(count);
  for (uint32_t i = 0; i < count; ++i) {
    const float* m = localMat16 + 16u * (size_t)i;            // column-major: m[col * 4 + row]
    const uint8_t t = type[i];
    if (t != SC_TICK_COLLIDER_BOX && t != SC_TICK_COLLIDER_SPHERE && t != SC_TICK_COLLIDER_CAPSULE)
      return fail(c, "trigger volumes: a volume's type is SC_TICK_COLLIDER_BOX, _SPHERE or _CAPSULE");
    const float he[3] = { halfExtents3[3 * (size_t)i], halfExtents3[3 * (size_t)i + 1], halfExtents3[3 * (size_t)i + 2] };
    const float values[5] = { he[0], he[1], he[2], radius[i], halfHeight[i] };
    bool finite = true;
    for (float x : values) finite = finite && std::isfinite(x);
    for (int col = 0; col < 4; ++col) for (int row = 0; row < 3; ++row) finite = finite && std::isfinite(m[col * 4 + row]);
    if (!finite) return fail(c, "trigger volumes: local_mat16, half_extents, radius and half_height must be finite");
    float4* q = &v[(size_t)i * kOverlapVolumeWords];
    for (int row = 0; row < 3; ++row) q[row] = make_float4(m[row], m[4 + row], m[8 + row], m[12 + row]);
    const float hh = halfHeight[i] < 0.0f ? 0.0f : halfHeight[i];      // the record as scTickUploadColliders stores it
    q[3] = t == SC_TICK_COLLIDER_BOX ? make_float4(he[0], he[1], he[2], 0.0f)
         : t == SC_TICK_COLLIDER_SPHERE ? make_float4(0.0f, 0.0f, 0.0f, radius[i]) : make_float4(0.0f, hh, 0.0f, radius[i]);
    const uint32_t words[4] = { t, mask[i], 0u, 0u };
    std::memcpy(&q[4], words, sizeof words);
    an[i] = make_uint2(anchor[i], skipSelf ? (skipSelf[i] ? 1u : 0u) : 1u);
  }
  if (!bind(c)) return 0;
  TriggerState& t = c->triggers;
  // The same count, max_members, max_events and mode as the current set: only anchors, locals and values are rewritten, behind whatever is
  // queued -- the remembered rows stay, no epoch bump, so no learn tick, and a captured graph (which holds the buffers, the sizes and
  // the kernel instance) stays valid.
  const uint32_t perVolume = count ? maxMembers : 0u, events = count ? maxEvents : 0u;
  if (count != t.count || perVolume != t.maxMembers || events != t.maxEvents || shapes != c->triggerShapes) {
    if (!sync(c)) return 0;
    const size_t slots = (size_t)count * perVolume;
    auto empty = [&] {
      dfree(c, t.ids); dfree(c, t.entered); dfree(c, t.exited); dfree(c, t.ctl);
      t.ids = nullptr; t.entered = t.exited = nullptr; t.ctl = nullptr;
      c->triggerIdCap = 0; c->triggerEventCap = 0; t.count = 0; t.maxMembers = 0; t.maxEvents = 0;
    };
    if (!count) empty();                                       // count 0 clears the set AND frees it (growBatch below keeps the per-volume arrays' capacity)
    else {
      if (slots > c->triggerIdCap) {                           // the id rows: kept within their capacity, allocated anew beyond it
        dfree(c, t.ids); t.ids = nullptr; c->triggerIdCap = 0;
        if (!dalloc(c, t.ids, std::max<size_t>(slots, 1024u))) { empty(); return 0; }
        c->triggerIdCap = std::max<size_t>(slots, 1024u);
      }
      if (events > c->triggerEventCap || !t.entered) {
        dfree(c, t.entered); dfree(c, t.exited); t.entered = t.exited = nullptr; c->triggerEventCap = 0;
        const size_t room = std::max<size_t>(events, 64u);
        if (!dalloc(c, t.entered, room) || !dalloc(c, t.exited, room)) { empty(); return 0; }
        c->triggerEventCap = (uint32_t)room;
      }
      if (!t.ctl && !dalloc(c, t.ctl, 2u)) { empty(); return 0; }
    }
    if (!growBatch(c, c->triggerCap, t.count, count, batchArray(t.local, false, kOverlapVolumeWords), batchArray(t.anchor), batchArray(t.world, true, 3),
                   batchArray(t.counts, true), batchArray(t.remembered, true), batchArray(t.stat, true))) { empty(); return 0; }
    if (!count) {                                              // freed, not kept: a context that clears its set holds nothing for it
      dfree(c, const_cast<float4*>(t.local)); dfree(c, const_cast<uint2*>(t.anchor)); dfree(c, t.world); dfree(c, t.counts); dfree(c, t.remembered); dfree(c, t.stat);
      t = TriggerState{}; c->triggerCap = 0;
    }
    t.maxMembers = perVolume; t.maxEvents = events;
    c->triggerShapes = shapes;
    c->hTriggerAnchor = an;
    if (!resyncTriggers(c)) return 0;                          // a re-sized set remembers nothing
  } else c->hTriggerAnchor = an;
  if (!count) return 1;
  if (!h2d(c, const_cast<float4*>(t.local), v.data(), v.size() * sizeof(float4)) ||
      !h2d(c, const_cast<uint2*>(t.anchor), an.data(), an.size() * sizeof(uint2))) return 0;
  return sync(c) ? 1 : 0;
}

// the gate of the trigger readers: the last run carried the flag and the set is the size that run answered
static bool triggerResult(ScTickContext* c)
{
  const TriggerState& t = c->triggers;
  const bool stands = t.count == c->lastWith.triggerCount && t.maxMembers == c->lastWith.triggerMaxMembers && t.maxEvents == c->lastWith.triggerMaxEvents;
  return bind(c) && lastRunResult(c, SC_TICK_TRIGGERS, "the last scTickRun did not request SC_TICK_TRIGGERS", true, nullptr,
                                  "trigger results are ready after scTickRunPairs", stands,
                                  "the trigger set was re-sized since the last run with SC_TICK_TRIGGERS: its results are gone");
}

// the report: sums of the per-volume words the waves wrote (no wave adds to a shared word per hit)
static bool triggerInfo(ScTickContext* c, ScTickTriggerInfo* info, std::vector<uint32_t>* countsOut)
{
  const TriggerState& t = c->triggers;
  std::vector<uint32_t> counts(t.count);
  std::vector<uint4> stat(t.count);
  if (!d2h(c, counts.data(), t.counts, (size_t)t.count * sizeof(uint32_t)) || !d2h(c, stat.data(), t.stat, (size_t)t.count * sizeof(uint4)) || !sync(c)) return false;
  if (info) {
    uint64_t members = 0, entered = 0, exited = 0; uint32_t resync = 0, overflow = 0;
    for (uint32_t n : counts) members += n;
    for (const uint4& s : stat) { entered += s.x; exited += s.y; resync += (s.z & kTriggerResync) ? 1u : 0u; overflow += (s.z & kTriggerOverflow) ? 1u : 0u; }
    info->volumes = t.count; info->max_members = t.maxMembers; info->members = (uint32_t)std::min<uint64_t>(members, 0xFFFFFFFFull);
    info->entered = (uint32_t)std::min<uint64_t>(entered, 0xFFFFFFFFull); info->exited = (uint32_t)std::min<uint64_t>(exited, 0xFFFFFFFFull);
    info->resync_volumes = resync; info->overflow_volumes = overflow;
    info->events_truncated = (entered > t.maxEvents || exited > t.maxEvents) ? 1u : 0u;
  }
  if (countsOut) countsOut->swap(counts);
  return true;
}

int scTickReadTriggerEvents(ScTickContext* c, uint32_t* entered2, uint32_t enteredCap, uint32_t* exited2, uint32_t exitedCap, ScTickTriggerInfo* info)
{
  if (!c) return 0;
  if (!triggerResult(c)) return 0;
  const TriggerState& t = c->triggers;
  ScTickTriggerInfo sums;
  if (!triggerInfo(c, &sums, nullptr)) return 0;
  const uint32_t in = entered2 ? std::min(std::min(sums.entered, t.maxEvents), enteredCap) : 0u;
  const uint32_t out = exited2 ? std::min(std::min(sums.exited, t.maxEvents), exitedCap) : 0u;
  if (in && !d2h(c, entered2, t.entered, (size_t)in * sizeof(uint2))) return 0;
  if (out && !d2h(c, exited2, t.exited, (size_t)out * sizeof(uint2))) return 0;
  if ((in || out) && !sync(c)) return 0;
  if (info) *info = sums;
  return 1;
}

int scTickReadTriggerMembers(ScTickContext* c, uint32_t* counts, uint32_t* ids, uint32_t volumeCapacity, ScTickTriggerInfo* info)
{
  if (!c) return 0;
  if (!triggerResult(c)) return 0;
  const TriggerState& t = c->triggers;
  ScTickTriggerInfo sums;
  std::vector<uint32_t> perVolume;
  if (!triggerInfo(c, &sums, &perVolume)) return 0;
  const uint32_t take = std::min(t.count, volumeCapacity);
  if (take && ids && (!d2h(c, ids, t.ids, (size_t)take * t.maxMembers * sizeof(uint32_t)) || !sync(c))) return 0;
  if (take && counts) std::memcpy(counts, perVolume.data(), (size_t)take * sizeof(uint32_t));
  if (info) *info = sums;
  return 1;
}

int scTickReadTriggerMatrices(ScTickContext* c, uint32_t first, uint32_t count, float* mat16)
{
  if (!c) return 0;
  if (count && !mat16) return fail(c, "null argument");
  if (!triggerResult(c)) return 0;
  if ((uint64_t)first + count > c->triggers.count) return fail(c, "range exceeds the trigger volume count");
  if (!count) return 1;
  std::vector<float> rows((size_t)count * 12u);
  if (!d2h(c, rows.data(), c->triggers.world + 3u * (size_t)first, rows.size() * sizeof(float)) || !sync(c)) return 0;
  for (uint32_t k = 0; k < count; ++k) rowsToMat4(&rows[12u * (size_t)k], mat16 + 16u * (size_t)k);
  return 1;
}

int scTickReadTriggerVolumes(ScTickContext* c, uint32_t first, uint32_t count, uint32_t* anchor)
{
  if (!c) return 0;
  if (count && !anchor) return fail(c, "null argument");
  if ((uint64_t)first + count > c->triggers.count) return fail(c, "range exceeds the trigger volume count");
  for (uint32_t k = 0; k < count; ++k) anchor[k] = c->hTriggerAnchor[first + k].x;      // (host mirror: no read-back)
  return 1;
}

// pair events and touch events: one state each, allocated, read and freed alike (`what` names the feature in the error texts)
static int setEventState(ScTickContext* c, PairEventState& e, void*& slabOut, size_t& slabBytes, const std::string& what, uint32_t maxTracked, uint32_t maxEvents)
{
  if ((maxTracked == 0u) != (maxEvents == 0u)) return fail(c, (what + ": max_tracked_pairs and max_events are both positive, or both 0 (off)").c_str());
  if (maxTracked && !c->sectors) return fail(c, "the context has no broadphase");
  if (maxTracked > (1u << 27) || maxEvents > (1u << 27)) return fail(c, (what + ": at most 2^27 tracked pairs and 2^27 events").c_str());
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  if (!bind(c) || !sync(c)) return 0;
  dfree(c, slabOut); dfree(c, e.info); dfree(c, e.begun); dfree(c, e.ended);
  e = PairEventState{}; slabOut = nullptr; slabBytes = 0;
  dropCaptures(c);       // a captured tick holds the old buffers (or none); the pair search itself is not concerned
  if (!maxTracked) return 1;
  uint32_t slots = 64u;
  while (slots < 2u * maxTracked) slots <<= 1;
  // one allocation: table 0, table 1, marks 0, marks 1, control words
  const size_t tableBytes = (size_t)slots * sizeof(unsigned long long), markBytes = (size_t)(slots / 32u) * sizeof(uint32_t);
  const size_t bytes = 2u * tableBytes + 2u * markBytes + kPeCtlWords * sizeof(uint32_t);
  char* slab = nullptr;
  if (!dalloc(c, slab, bytes)) return 0;
  slabOut = slab; slabBytes = bytes;
  if (!dalloc(c, e.info, kPeInfoWords) || !dalloc(c, e.begun, maxEvents, false) || !dalloc(c, e.ended, maxEvents, false)) return 0;
  e.table[0] = reinterpret_cast<unsigned long long*>(slab); e.table[1] = reinterpret_cast<unsigned long long*>(slab + tableBytes);
  e.marks[0] = reinterpret_cast<uint32_t*>(slab + 2u * tableBytes); e.marks[1] = reinterpret_cast<uint32_t*>(slab + 2u * tableBytes + markBytes);
  e.ctl = reinterpret_cast<uint32_t*>(slab + 2u * tableBytes + 2u * markBytes);
  e.slots = slots; e.maxTracked = maxTracked; e.maxEvents = maxEvents;
  return 1;
}

static int readEventState(ScTickContext* c, const PairEventState& e, uint32_t flag, const char* notRequested, const char* pending, const char* off,
                          uint32_t* begun2, uint32_t begunCap, uint32_t* ended2, uint32_t endedCap, ScTickPairEventInfo* info)
{
  static_assert(sizeof(ScTickPairEventInfo) == 6u * sizeof(uint32_t) && kPeInfoWords >= 6u, "the device writes the report word by word");
  if (!info) return fail(c, "null argument");      // (the callers have checked c)
  if (!bind(c) || !lastRunResult(c, flag, notRequested, true, nullptr, pending, e.ctl != nullptr, off)) return 0;
  if (!d2h(c, info, e.info, sizeof *info) || !sync(c)) return 0;
  const uint32_t nb = std::min(std::min(info->begun, e.maxEvents), begun2 ? begunCap : 0u);
  const uint32_t ne = std::min(std::min(info->ended, e.maxEvents), ended2 ? endedCap : 0u);
  if (nb && !d2h(c, begun2, e.begun, (size_t)nb * sizeof(uint2))) return 0;
  if (ne && !d2h(c, ended2, e.ended, (size_t)ne * sizeof(uint2))) return 0;
  if ((nb || ne) && !sync(c)) return 0;
  return 1;
}

int scTickSetPairEvents(ScTickContext* c, uint32_t maxTracked, uint32_t maxEvents)
{
  if (!c) return 0;
  return setEventState(c, c->pairEvents, c->pairEventSlab, c->pairEventSlabBytes, "pair events", maxTracked, maxEvents);
}

int scTickReadPairEvents(ScTickContext* c, uint32_t* begun2, uint32_t begunCap, uint32_t* ended2, uint32_t endedCap, ScTickPairEventInfo* info)
{
  if (!c) return 0;
  return readEventState(c, c->pairEvents, SC_TICK_PAIR_EVENTS, "the last scTickRun did not request SC_TICK_PAIR_EVENTS", "pair events are ready after scTickRunPairs",
                        "pair events were switched off since the last scTickRun", begun2, begunCap, ended2, endedCap, info);
}

int scTickSetTouchEvents(ScTickContext* c, uint32_t maxTracked, uint32_t maxEvents)
{
  if (!c) return 0;
  return setEventState(c, c->narrow.touch, c->touchEventSlab, c->touchEventSlabBytes, "touch events", maxTracked, maxEvents);
}

int scTickReadTouchEvents(ScTickContext* c, uint32_t* begun2, uint32_t begunCap, uint32_t* ended2, uint32_t endedCap, ScTickTouchEventInfo* info)
{
  static_assert(sizeof(ScTickTouchEventInfo) == sizeof(ScTickPairEventInfo) && offsetof(ScTickTouchEventInfo, events_truncated) == offsetof(ScTickPairEventInfo, events_truncated),
                "the two reports are the same six words");
  if (!c) return 0;
  return readEventState(c, c->narrow.touch, SC_TICK_TOUCH_EVENTS, "the last scTickRun did not request SC_TICK_TOUCH_EVENTS", "touch events are ready after scTickRunPairs",
                        "touch events were switched off since the last scTickRun", begun2, begunCap, ended2, endedCap, reinterpret_cast<ScTickPairEventInfo*>(info));
}

int scTickSetPairShapes(ScTickContext* c, uint32_t maxTouching)
{
  if (!c) return 0;
  if (maxTouching && !c->sectors) return fail(c, "the context has no broadphase");
  if (maxTouching > (1u << 27)) return fail(c, "touching pairs: at most 2^27 listed pairs");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  if (!bind(c) || !sync(c)) return 0;
  dropCaptures(c);       // a captured tick holds the old buffers (or none); no epoch bump: the bins are not concerned
  // (every other stage follows the list: off with it, re-sized with it)
  NarrowWant w = narrowWanted(c);
  w.maxTouching = maxTouching;
  return sizeNarrowPhase(c, kNarrowList, w) ? 1 : 0;
}

int scTickSetPairContacts(ScTickContext* c, uint32_t enable)
{
  static_assert(sizeof(ScTickPairContact) == 2u * sizeof(float4) && offsetof(ScTickPairContact, normal) == sizeof(float4), "the device writes a record as two float4");
  static_assert(kPairContactsEdgeEps == SC_TICK_PAIR_CONTACTS_EDGE_EPS, "the edge-axis epsilon differs from the header's");
  static_assert(kContactNone == SC_TICK_CONTACT_NONE && kContactRoundRound == SC_TICK_CONTACT_ROUND_ROUND && kContactRoundBox == SC_TICK_CONTACT_ROUND_BOX &&
                kContactBoxFaceA == SC_TICK_CONTACT_BOX_FACE_A && kContactBoxFaceB == SC_TICK_CONTACT_BOX_FACE_B && kContactBoxEdge == SC_TICK_CONTACT_BOX_EDGE &&
                kContactDeep == SC_TICK_CONTACT_DEEP && kContactDegenerate == SC_TICK_CONTACT_DEGENERATE, "the contact kinds differ from the header's");
  if (!c) return 0;
  NarrowWant w = narrowWanted(c);
  if (enable && !w.maxTouching) return fail(c, "scTickSetPairContacts needs scTickSetPairShapes(max_touching > 0) first");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  if (!bind(c) || !sync(c)) return 0;
  dropCaptures(c);       // a captured tick holds the old buffers (or none); no epoch bump: the bins are not concerned
  w.contacts = enable != 0u;      // (pair manifolds need the contacts: off with them)
  return sizeNarrowPhase(c, kNarrowContacts, w) ? 1 : 0;
}

int scTickGetPairContacts(ScTickContext* c, uint32_t* enabled)
{
  if (!c || !enabled) return c ? fail(c, "null argument") : 0;
  *enabled = c->narrow.contacts.ctl ? 1u : 0u;
  return 1;
}

int scTickReadPairContacts(ScTickContext* c, ScTickPairContact* out, uint32_t capacity, ScTickPairContactInfo* info)
{
  static_assert(sizeof(ScTickPairContactInfo) == kPcInfoWords * sizeof(uint32_t), "the device writes the report word by word");
  if (!c || !info) return c ? fail(c, "null argument") : 0;
  const PairContactState& k = c->narrow.contacts;
  if (!narrowResult(c, kStageContacts)) return 0;
  return readReportAndRecords(c, info, k.info, &ScTickPairContactInfo::written, k.maxTouching, k.rec, sizeof(ScTickPairContact), out, capacity) ? 1 : 0;
}

int scTickSetPairManifolds(ScTickContext* c, uint32_t enable)
{
  static_assert(sizeof(ScTickPairManifold) == 5u * sizeof(float4) && offsetof(ScTickPairManifold, depth) == 3u * sizeof(float4) &&
                offsetof(ScTickPairManifold, count) == 4u * sizeof(float4), "the device writes a record as five float4");
  static_assert(kManifoldNone == SC_TICK_MANIFOLD_NONE && kManifoldSingle == SC_TICK_MANIFOLD_SINGLE && kManifoldSegment == SC_TICK_MANIFOLD_SEGMENT &&
                kManifoldFace == SC_TICK_MANIFOLD_FACE && kManifoldReduced == SC_TICK_MANIFOLD_REDUCED, "the manifold kinds differ from the header's");
  static_assert(kManifoldSkin == SC_TICK_MANIFOLD_SKIN && kManifoldFlat == SC_TICK_MANIFOLD_FLAT, "the manifold tolerances differ from the header's");
  if (!c) return 0;
  NarrowWant w = narrowWanted(c);
  if (enable && !w.contacts) return fail(c, "scTickSetPairManifolds needs scTickSetPairContacts(1) first");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  if (!bind(c) || !sync(c)) return 0;
  dropCaptures(c);       // a captured tick holds the old buffers (or none); no epoch bump: the bins are not concerned
  w.manifolds = enable != 0u;
  return sizeNarrowPhase(c, kNarrowManifolds, w) ? 1 : 0;
}

int scTickGetPairManifolds(ScTickContext* c, uint32_t* enabled)
{
  if (!c || !enabled) return c ? fail(c, "null argument") : 0;
  *enabled = c->narrow.manifolds.ctl ? 1u : 0u;
  return 1;
}

int scTickReadPairManifolds(ScTickContext* c, ScTickPairManifold* out, uint32_t capacity, ScTickPairManifoldInfo* info)
{
  static_assert(sizeof(ScTickPairManifoldInfo) == kPmInfoWords * sizeof(uint32_t), "the device writes the report word by word");
  if (!c || !info) return c ? fail(c, "null argument") : 0;
  const PairManifoldState& f = c->narrow.manifolds;
  if (!narrowResult(c, kStageManifolds)) return 0;
  return readReportAndRecords(c, info, f.info, &ScTickPairManifoldInfo::written, f.maxTouching, f.rec, sizeof(ScTickPairManifold), out, capacity) ? 1 : 0;
}

int scTickSetPairIslands(ScTickContext* c, uint32_t enable, uint32_t fixedGroups)
{
  static_assert(sizeof(ScTickPairIslandInfo) == 32u && sizeof(ScTickPairIslandInfo) == kPiInfoWords * sizeof(uint32_t), "the device writes the report word by word");
  static_assert(kIslandNone == SC_TICK_ISLAND_NONE, "the island of a fixed member differs from the header's");
  if (!c) return 0;
  NarrowWant w = narrowWanted(c);
  if (enable && !w.maxTouching) return fail(c, "scTickSetPairIslands needs scTickSetPairShapes(max_touching > 0) first");
  if (fixedGroups >> 16) return fail(c, "scTickSetPairIslands: fixed_groups bits above 15 are not supported");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  if (!bind(c) || !sync(c)) return 0;
  dropCaptures(c);       // a captured tick holds the old buffers (or none) and the old fixed groups; no epoch bump: the bins are not concerned
  w.islands = enable != 0u; w.fixedGroups = fixedGroups;
  return sizeNarrowPhase(c, kNarrowIslands, w) ? 1 : 0;
}

int scTickGetPairIslands(ScTickContext* c, uint32_t* enabled, uint32_t* fixedGroups)
{
  if (!c || !enabled || !fixedGroups) return c ? fail(c, "null argument") : 0;
  *enabled = c->narrow.islands.ctl ? 1u : 0u;
  *fixedGroups = c->narrow.islands.fixedGroups;
  return 1;
}

int scTickReadPairIslands(ScTickContext* c, uint32_t* labels, uint32_t labelCapacity, uint32_t* edgeIslands, uint32_t edgeCapacity, ScTickPairIslandInfo* info)
{
  if (!c || !info) return c ? fail(c, "null argument") : 0;
  const PairIslandState& s = c->narrow.islands;
  if (!narrowResult(c, kStageIslands)) return 0;
  // the report and the edge islands like every record reader; then the labels of the entities there are now
  if (!readReportAndRecords(c, info, s.info, &ScTickPairIslandInfo::edges, s.maxTouching, s.edge, sizeof(uint32_t), edgeIslands, edgeCapacity)) return 0;
  const uint32_t m = std::min(std::min(c->n, s.cap), labels ? labelCapacity : 0u);
  return (!m || (d2h(c, labels, s.labels, (size_t)m * sizeof(uint32_t)) && sync(c))) ? 1 : 0;
}

int scTickSetPairSleep(ScTickContext* c, uint32_t enable, float linTol, float angTol, uint32_t restRuns, uint32_t maxEvents)
{
  static_assert(sizeof(ScTickPairSleepInfo) == 32u && sizeof(ScTickPairSleepInfo) == kPzInfoWords * sizeof(uint32_t), "the device writes the report word by word");
  static_assert(kSleepAsleep == SC_TICK_SLEEP_ASLEEP && kSleepStill == SC_TICK_SLEEP_STILL && kSleepMovable == SC_TICK_SLEEP_MOVABLE, "the state bits differ from the header's");
  static_assert(kSleepResync == SC_TICK_SLEEP_INFO_RESYNC && kSleepFellOverflow == SC_TICK_SLEEP_INFO_FELL_OVERFLOW && kSleepWokeOverflow == SC_TICK_SLEEP_INFO_WOKE_OVERFLOW &&
                kSleepListTruncated == SC_TICK_SLEEP_INFO_LIST_TRUNCATED, "the report's flags differ from the header's");
  if (!c) return 0;
  NarrowWant w = narrowWanted(c);
  if (enable && !w.islands) return fail(c, "scTickSetPairSleep needs scTickSetPairIslands(1) first");
  if (enable && !(std::isfinite(linTol) && linTol >= 0.0f && std::isfinite(angTol) && angTol >= 0.0f))
    return fail(c, "scTickSetPairSleep: lin_tol and ang_tol must be finite and >= 0");
  if (enable && (restRuns < 1u || restRuns > 255u)) return fail(c, "scTickSetPairSleep: rest_runs must be in 1 .. 255");
  if (enable && !maxEvents) return fail(c, "scTickSetPairSleep: max_events must be > 0");
  if (enable && maxEvents > (1u << 24)) return fail(c, "scTickSetPairSleep: at most 2^24 events a list");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  if (!bind(c) || !sync(c)) return 0;
  // a captured tick holds the buffers (or none), and the tolerances and rest_runs as kernel arguments; no epoch bump: the bins are not
  // concerned.  (Already on with this max_events: what is remembered stays, and so do the captures where nothing changes)
  if (!(enable && w.sleepEvents == maxEvents && w.linTol == linTol && w.angTol == angTol && w.restRuns == restRuns)) dropCaptures(c);
  w.sleepEvents = enable ? maxEvents : 0u; w.linTol = linTol; w.angTol = angTol; w.restRuns = restRuns;
  return sizeNarrowPhase(c, kNarrowSleep, w) ? 1 : 0;
}

int scTickGetPairSleep(ScTickContext* c, uint32_t* enabled, float* linTol, float* angTol, uint32_t* restRuns, uint32_t* maxEvents)
{
  if (!c || !enabled || !linTol || !angTol || !restRuns || !maxEvents) return c ? fail(c, "null argument") : 0;
  const PairSleepState& z = c->narrow.sleep;      // (all zero while off)
  *enabled = z.ctl ? 1u : 0u; *linTol = z.linTol; *angTol = z.angTol; *restRuns = z.restRuns; *maxEvents = z.maxEvents;
  return 1;
}

int scTickWakeEntities(ScTickContext* c, const uint32_t* ids, uint32_t n)
{
  if (!c || (!ids && n)) return c ? fail(c, "null argument") : 0;
  if (!c->narrow.sleep.ctl) return fail(c, "scTickWakeEntities needs scTickSetPairSleep(1) first");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  const uint32_t count = std::min(c->n, c->narrow.sleep.cap);
  std::vector<uint32_t> dense(n);
  for (uint32_t i = 0; i < n; ++i) {                        // (every id is checked before anything is written)
    if ((ids[i] >> 24) != c->rank) return fail(c, "scTickWakeEntities: an id of another rank");
    dense[i] = ids[i] & 0x00FFFFFFu;
    if (dense[i] >= count) return fail(c, "scTickWakeEntities: an id at or above the entity count");
  }
  if (!n) return 1;
  if (!bind(c) || !sync(c)) return 0;                       // behind every run issued so far, outside any captured graph
  uint32_t* dIds = nullptr;
  if (!dalloc(c, dIds, n, false)) return 0;
  const bool ok = h2d(c, dIds, dense.data(), (size_t)n * sizeof(uint32_t));
  if (ok) launchPairSleepWake(c->narrow.sleep, dIds, n, c->stream);
  const bool done = ok && sync(c);
  dfree(c, dIds);
  return done ? 1 : 0;
}

int scTickReadPairSleep(ScTickContext* c, uint32_t* states, uint32_t stateCapacity, uint32_t* fellAsleep, uint32_t fellCapacity, uint32_t* woke, uint32_t wokeCapacity,
                        ScTickPairSleepInfo* info)
{
  if (!c || !info) return c ? fail(c, "null argument") : 0;
  const PairSleepState& z = c->narrow.sleep;
  if (!narrowResult(c, kStageSleep)) return 0;
  if (!d2h(c, info, z.info, sizeof *info) || !sync(c)) return 0;
  const uint32_t ns = std::min(std::min(c->n, z.cap), states ? stateCapacity : 0u);
  const uint32_t nf = std::min(std::min(info->fell_asleep, z.maxEvents), fellAsleep ? fellCapacity : 0u);
  const uint32_t nw = std::min(std::min(info->woke, z.maxEvents), woke ? wokeCapacity : 0u);
  if (ns && !d2h(c, states, z.state, (size_t)ns * sizeof(uint32_t))) return 0;
  if (nf && !d2h(c, fellAsleep, z.fell, (size_t)nf * sizeof(uint32_t))) return 0;
  if (nw && !d2h(c, woke, z.woke, (size_t)nw * sizeof(uint32_t))) return 0;
  return ((ns | nf | nw) == 0u || sync(c)) ? 1 : 0;
}

int scTickSetPairPersistence(ScTickContext* c, uint32_t enable, float matchDist)
{
  static_assert(sizeof(ScTickPairPersist) == 16u && sizeof(ScTickPairPersist) == sizeof(uint4), "the device writes the record with one 16-byte store");
  static_assert(sizeof(ScTickPairPersistInfo) == 32u && sizeof(ScTickPairPersistInfo) <= kPpInfoSide * sizeof(uint32_t), "the device writes the report word by word");
  static_assert(kPersistNone == SC_TICK_PERSIST_NONE, "the entry of an unmatched pair differs from the header's");
  if (!c) return 0;
  NarrowWant w = narrowWanted(c);
  if (enable && !w.manifolds) return fail(c, "scTickSetPairPersistence needs scTickSetPairManifolds(1) first");
  if (enable && !(std::isfinite(matchDist) && matchDist > 0.0f)) return fail(c, "scTickSetPairPersistence: match_dist must be finite and > 0");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  if (!bind(c) || !sync(c)) return 0;
  dropCaptures(c);       // a captured tick holds the old buffers (or none) and the old match distance; no epoch bump: the bins are not concerned
  w.persist = enable != 0u; w.matchDist = matchDist;      // (already on: its size stays, and with it what is remembered)
  return sizeNarrowPhase(c, kNarrowPersist, w) ? 1 : 0;
}

int scTickGetPairPersistence(ScTickContext* c, uint32_t* enabled, float* matchDist)
{
  if (!c || !enabled || !matchDist) return c ? fail(c, "null argument") : 0;
  *enabled = c->narrow.persist.ctl ? 1u : 0u;
  *matchDist = c->narrow.persist.ctl ? c->narrow.persist.matchDist : 0.0f;
  return 1;
}

namespace {
// the gate of the persistence readers and of the payload write: the last run matched, its pair half is through, the buffers are still there
bool pairPersistResult(ScTickContext* c) { return narrowResult(c, kStagePersist); }
// that run's `written` and the side it filled, as the finish kernel left them
bool pairPersistFilled(ScTickContext* c, uint32_t& written, uint32_t& side)
{
  uint32_t w[kPpInfoWords];
  if (!d2h(c, w, c->narrow.persist.info, sizeof w) || !sync(c)) return false;
  written = std::min(w[0], c->narrow.persist.maxTouching); side = w[kPpInfoSide] & 1u;
  return true;
}
} // namespace

int scTickReadPairPersistence(ScTickContext* c, ScTickPairPersist* out, uint32_t capacity, ScTickPairPersistInfo* info)
{
  if (!c || !info) return c ? fail(c, "null argument") : 0;
  const PairPersistState& s = c->narrow.persist;
  if (!pairPersistResult(c)) return 0;
  return readReportAndRecords(c, info, s.info, &ScTickPairPersistInfo::written, s.maxTouching, s.rec, sizeof(ScTickPairPersist), out, capacity) ? 1 : 0;
}

int scTickWritePairPayloads(ScTickContext* c, const float* rows, uint32_t first, uint32_t count)
{
  if (!c || (!rows && count)) return c ? fail(c, "null argument") : 0;
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  if (!pairPersistResult(c)) return 0;
  uint32_t written = 0, side = 0;
  if (!pairPersistFilled(c, written, side)) return 0;
  if ((uint64_t)first + count > written) return fail(c, "scTickWritePairPayloads: the range exceeds the records the last run wrote");
  if (!count) return 1;
  // (the rows the next flagged run carries from: behind the run on its stream)
  return (h2d(c, c->narrow.persist.payload[side] + 4u * (size_t)first, rows, (size_t)count * 4u * sizeof(float4)) && sync(c)) ? 1 : 0;
}

int scTickReadPairPayloads(ScTickContext* c, float* rows, uint32_t capacity)
{
  if (!c) return 0;
  if (!pairPersistResult(c)) return 0;
  uint32_t written = 0, side = 0;
  if (!pairPersistFilled(c, written, side)) return 0;
  const uint32_t m = std::min(written, rows ? capacity : 0u);
  return (!m || (d2h(c, rows, c->narrow.persist.payload[side], (size_t)m * 4u * sizeof(float4)) && sync(c))) ? 1 : 0;
}

int scTickReadPairShapes(ScTickContext* c, uint32_t* pairs2, uint32_t capacity, ScTickPairShapeInfo* info)
{
  static_assert(sizeof(ScTickPairShapeInfo) == 6u * sizeof(uint32_t) && kPsInfoWords >= 6u, "the device writes the report word by word");
  static_assert(kPairShapesSatEps == SC_TICK_PAIR_SHAPES_SAT_EPS, "the separating-axis epsilon differs from the header's");
  if (!c || !info) return c ? fail(c, "null argument") : 0;
  const PairShapeState& e = c->narrow.list;
  if (!narrowResult(c, kStageList)) return 0;
  return readReportAndRecords(c, info, e.info, &ScTickPairShapeInfo::touching, e.maxTouching, e.list, sizeof(uint2), pairs2, capacity) ? 1 : 0;
}

int scTickSetRayShapes(ScTickContext* c, uint32_t mode)
{
  if (!c) return 0;
  if (mode != SC_TICK_RAY_SHAPES_AABB && mode != SC_TICK_RAY_SHAPES_EXACT) return fail(c, "unknown ray shape mode (SC_TICK_RAY_SHAPES_*)");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending (its rays are cast in the mode its tick half ran in)");
  if (mode == c->rayShapes) return 1;
  if (!bind(c) || !sync(c)) return 0;
  c->rayShapes = mode;
  dropCaptures(c);       // a captured tick holds the other instance; no epoch bump: the bins are not concerned
  return 1;
}

int scTickGetRayShapes(ScTickContext* c, uint32_t* mode)
{
  if (!c || !mode) return c ? fail(c, "null argument") : 0;
  *mode = c->rayShapes;
  return 1;
}

int scTickSetSweepShapes(ScTickContext* c, uint32_t mode)
{
  static_assert(kSweepShapesTol == SC_TICK_SWEEP_SHAPES_TOL && kSweepShapesSteps == SC_TICK_SWEEP_SHAPES_STEPS && kSweepSeenCap == SC_TICK_SWEEP_SHAPES_SEEN,
                "the sweep refinement's constants differ from the header's");
  if (!c) return 0;
  if (mode != SC_TICK_SWEEP_SHAPES_AABB && mode != SC_TICK_SWEEP_SHAPES_EXACT) return fail(c, "unknown sweep shape mode (SC_TICK_SWEEP_SHAPES_*)");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending (its sweeps are cast in the mode its tick half ran in)");
  if (mode == c->sweepShapes) return 1;
  if (!bind(c) || !sync(c)) return 0;
  if (mode == SC_TICK_SWEEP_SHAPES_EXACT && !c->sweepInfo && !dalloc(c, c->sweepInfo, kSweepInfoWords)) return 0;
  c->sweepShapes = mode;
  dropCaptures(c);       // a captured tick holds the other instance; no epoch bump: the bins are not concerned
  return 1;
}

int scTickGetSweepShapes(ScTickContext* c, uint32_t* mode)
{
  if (!c || !mode) return c ? fail(c, "null argument") : 0;
  *mode = c->sweepShapes;
  return 1;
}

int scTickGetSweepShapeInfo(ScTickContext* c, ScTickSweepShapeInfo* info)
{
  static_assert(sizeof(ScTickSweepShapeInfo) == kSweepInfoWords * sizeof(uint32_t), "the device writes the report word by word");
  if (!c || !info) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !lastRunResult(c, SC_TICK_SWEEPS, "the last scTickRun did not request SC_TICK_SWEEPS",
                                 c->lastWith.sweepsExact && c->sweepInfo, "the last scTickRun swept in SC_TICK_SWEEP_SHAPES_AABB mode: nothing was refined",
                                 "the sweep shape report is ready after scTickRunPairs", true, nullptr)) return 0;
  if (!d2h(c, info, c->sweepInfo, sizeof *info) || !sync(c)) return 0;
  return 1;
}

int scTickSetAnchoredRays(ScTickContext* c, uint32_t count, const uint32_t* anchor, const float* localOrigin3, const float* localDir3,
                          const float* maxDist, const uint32_t* mask, const uint8_t* skipSelf)
{
  static_assert(kAnchorNone == SC_TICK_ANCHOR_NONE && kAnchorDead == SC_TICK_ANCHOR_DEAD, "anchor sentinels differ");
  if (!c) return 0;
  if (count && (!anchor || !localOrigin3 || !localDir3 || !maxDist || !mask)) return fail(c, "null argument");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending (its rays are resolved already)");
  // checked before anything changes, so a refused call leaves the previous set in place
  std::vector<float4> o(count), dd(count); std::vector<uint2> an(count);
  for (uint32_t i = 0; i < count; ++i) {
    o[i] = make_float4(localOrigin3[3 * i], localOrigin3[3 * i + 1], localOrigin3[3 * i + 2], maxDist[i]);
    float w; std::memcpy(&w, &mask[i], 4);
    dd[i] = make_float4(localDir3[3 * i], localDir3[3 * i + 1], localDir3[3 * i + 2], w);
    an[i] = make_uint2(anchor[i], skipSelf ? (skipSelf[i] ? 1u : 0u) : 1u);
    const float v[7] = { o[i].x, o[i].y, o[i].z, o[i].w, dd[i].x, dd[i].y, dd[i].z };
    for (float x : v) if (!std::isfinite(x)) return fail(c, "anchored rays: local_origin, local_dir and max_dist must be finite");
    if (maxDist[i] < 0.0f) return fail(c, "anchored rays: max_dist must be >= 0");
  }
  if (!bind(c)) return 0;
  // The same count as the current set: only the device arrays are rewritten, behind whatever is queued on the tick stream (the pair
  // half of a split flow reads the snapshot, never these arrays) -- no epoch bump, so no learn tick, and a captured graph stays valid.
  if (count != c->anchored.count) {
    AnchoredRayState& a = c->anchored;
    if (!sync(c) || !growBatch(c, c->anchoredCap, a.count, count, batchArray(a.origin), batchArray(a.dir), batchArray(a.anchor), batchArray(a.hits, true),
                               batchArray(a.snapOrigin, true, kMaxParity), batchArray(a.snapDir, true, kMaxParity), batchArray(a.snapSkip, true, kMaxParity))) return 0;
  }
  c->hAnchor = an;
  if (!count) return 1;
  if (!h2d(c, const_cast<float4*>(c->anchored.origin), o.data(), (size_t)count * 16u) ||
      !h2d(c, const_cast<float4*>(c->anchored.dir), dd.data(), (size_t)count * 16u) ||
      !h2d(c, const_cast<uint2*>(c->anchored.anchor), an.data(), (size_t)count * 8u)) return 0;
  return sync(c) ? 1 : 0;
}

int scTickReadAnchoredRayHits(ScTickContext* c, ScTickRayHit* hits, uint32_t cap, uint32_t* count)
{
  return readQueryHits(c, SC_TICK_ANCHORED_RAYS, "the last scTickRun did not request SC_TICK_ANCHORED_RAYS", "anchored ray hits are ready after scTickRunPairs",
                       c ? c->anchored.hits : nullptr, c ? c->anchored.count : 0u, hits, cap, count);
}

int scTickReadAnchoredRays(ScTickContext* c, uint32_t first, uint32_t count, uint32_t* anchor)
{
  if (!c) return 0;
  if (count && !anchor) return fail(c, "null argument");
  if ((uint64_t)first + count > c->anchored.count) return fail(c, "range exceeds the anchored ray count");
  for (uint32_t k = 0; k < count; ++k) anchor[k] = c->hAnchor[first + k].x;      // (host mirror: no read-back)
  return 1;
}

int scTickSetAnchoredSweeps(ScTickContext* c, uint32_t count, const uint32_t* anchor, const float* localStart3, const float* localEnd3, const float* radius,
                            const float* halfHeight, const uint32_t* mask, const uint8_t* skipSelf, const uint8_t* endFrame)
{
  static_assert(kASweepAnswered == SC_TICK_ASWEEP_ANSWERED && kASweepNoAnchor == SC_TICK_ASWEEP_NO_ANCHOR && kASweepNotFinite == SC_TICK_ASWEEP_NOT_FINITE,
                "anchored sweep statuses differ");
  if (!c) return 0;
  if (count && (!anchor || !localStart3 || !localEnd3 || !radius || !halfHeight || !mask)) return fail(c, "null argument");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  // checked before anything changes, so a refused call leaves the previous set in place
  std::vector<float4> a(count), b(count); std::vector<uint4> an(count);
  for (uint32_t i = 0; i < count; ++i) {
    a[i] = make_float4(localStart3[3 * (size_t)i], localStart3[3 * (size_t)i + 1], localStart3[3 * (size_t)i + 2], radius[i]);
    b[i] = make_float4(localEnd3[3 * (size_t)i], localEnd3[3 * (size_t)i + 1], localEnd3[3 * (size_t)i + 2], halfHeight[i]);
    const uint32_t frame = endFrame ? endFrame[i] : (uint32_t)SC_TICK_SWEEP_END_LOCAL;
    an[i] = make_uint4(anchor[i], skipSelf ? (skipSelf[i] ? 1u : 0u) : 1u, frame, mask[i]);
    const float v[8] = { a[i].x, a[i].y, a[i].z, a[i].w, b[i].x, b[i].y, b[i].z, b[i].w };
    for (float x : v) if (!std::isfinite(x)) return fail(c, "anchored sweeps: local_start, local_end, radius and half_height must be finite");
    if (radius[i] < 0.0f) return fail(c, "anchored sweeps: radius must be >= 0");
    if (frame != SC_TICK_SWEEP_END_LOCAL && frame != SC_TICK_SWEEP_END_WORLD_OFFSET)
      return fail(c, "anchored sweeps: end_frame is SC_TICK_SWEEP_END_LOCAL or SC_TICK_SWEEP_END_WORLD_OFFSET");
  }
  if (!bind(c)) return 0;
  AnchoredSweepState& q = c->asweeps;
  // The same count as the current set: only the device arrays are rewritten, behind whatever is queued on the tick stream -- no epoch
  // bump, so no learn tick, and a captured graph (which holds the buffers and the count) stays valid.
  if (count != q.count) {
    if (!sync(c)) return 0;
    if (count && !c->asweepInfo && !dalloc(c, c->asweepInfo, kSweepInfoWords)) return 0;
    if (!growBatch(c, c->asweepCap, q.count, count, batchArray(q.start), batchArray(q.end), batchArray(q.anchor), batchArray(q.hits, true),
                   batchArray(q.segment, true, 2))) return 0;
    if (!count) {                                        // freed, not kept: a context that clears its set holds nothing for it
      dfree(c, const_cast<float4*>(q.start)); dfree(c, const_cast<float4*>(q.end)); dfree(c, const_cast<uint4*>(q.anchor)); dfree(c, q.hits);
      dfree(c, q.segment); dfree(c, c->asweepInfo);
      q = AnchoredSweepState{}; c->asweepCap = 0; c->asweepInfo = nullptr;
    }
  }
  c->hSweepAnchor = an;
  if (!count) return 1;
  if (!h2d(c, const_cast<float4*>(q.start), a.data(), (size_t)count * sizeof(float4)) ||
      !h2d(c, const_cast<float4*>(q.end), b.data(), (size_t)count * sizeof(float4)) ||
      !h2d(c, const_cast<uint4*>(q.anchor), an.data(), (size_t)count * sizeof(uint4))) return 0;
  return sync(c) ? 1 : 0;
}

// the gate of the anchored sweeps' readers: the last run carried the flag and the set is the size that run answered
static bool anchoredSweepResult(ScTickContext* c, bool enabledThen = true, const char* notEnabled = nullptr)
{
  return bind(c) && lastRunResult(c, SC_TICK_ANCHORED_SWEEPS, "the last scTickRun did not request SC_TICK_ANCHORED_SWEEPS", enabledThen, notEnabled,
                                  "anchored sweep results are ready after scTickRunPairs", c->asweeps.count == c->lastWith.asweepCount,
                                  "the anchored sweep set was re-sized since the last run with SC_TICK_ANCHORED_SWEEPS: its results are gone");
}

int scTickReadAnchoredSweepHits(ScTickContext* c, ScTickSweepHit* hits, uint32_t cap, uint32_t* count)
{
  if (!c || !count) return c ? fail(c, "null argument") : 0;
  if (!anchoredSweepResult(c)) return 0;
  *count = c->asweeps.count;
  const uint32_t take = std::min(c->asweeps.count, cap);
  if (take && hits) { if (!d2h(c, hits, c->asweeps.hits, (size_t)take * sizeof(SweepHit48)) || !sync(c)) return 0; }
  return 1;
}

int scTickReadAnchoredSweepSegments(ScTickContext* c, uint32_t first, uint32_t count, float* start3, float* end3)
{
  if (!c) return 0;
  if (!anchoredSweepResult(c)) return 0;
  if ((uint64_t)first + count > c->asweeps.count) return fail(c, "range exceeds the anchored sweep count");
  if (!count || (!start3 && !end3)) return 1;
  std::vector<float4> seg((size_t)count * 2u);
  if (!d2h(c, seg.data(), c->asweeps.segment + 2u * (size_t)first, seg.size() * sizeof(float4)) || !sync(c)) return 0;
  for (uint32_t k = 0; k < count; ++k) {
    const float4 s = seg[2u * (size_t)k], e = seg[2u * (size_t)k + 1u];
    if (start3) { start3[3 * (size_t)k] = s.x; start3[3 * (size_t)k + 1] = s.y; start3[3 * (size_t)k + 2] = s.z; }
    if (end3) { end3[3 * (size_t)k] = e.x; end3[3 * (size_t)k + 1] = e.y; end3[3 * (size_t)k + 2] = e.z; }
  }
  return 1;
}

int scTickGetAnchoredSweepShapeInfo(ScTickContext* c, ScTickSweepShapeInfo* info)
{
  if (!c || !info) return c ? fail(c, "null argument") : 0;
  if (!anchoredSweepResult(c, c->lastWith.asweepsExact && c->asweepInfo, "the last scTickRun swept in SC_TICK_SWEEP_SHAPES_AABB mode: nothing was refined")) return 0;
  if (!d2h(c, info, c->asweepInfo, sizeof *info) || !sync(c)) return 0;
  return 1;
}

int scTickReadAnchoredSweeps(ScTickContext* c, uint32_t first, uint32_t count, uint32_t* anchor)
{
  if (!c) return 0;
  if (count && !anchor) return fail(c, "null argument");
  if ((uint64_t)first + count > c->asweeps.count) return fail(c, "range exceeds the anchored sweep count");
  for (uint32_t k = 0; k < count; ++k) anchor[k] = c->hSweepAnchor[first + k].x;      // (host mirror: no read-back)
  return 1;
}

int scTickQueryOccupied(ScTickContext* c, uint32_t count, const float* pos3, const float* radius, const uint32_t* mask, uint8_t* blocked)
{
  if (!c) return 0;
  if (count && (!pos3 || !radius || !mask || !blocked)) return fail(c, "null argument");
  if (count > kMaxOccupancyQueries) return fail(c, "at most 256 occupancy queries per call");
  if (!bind(c)) return 0;
  if (!count) return 1;
  std::memset(blocked, 0, count);
  if (!c->n) return 1;
  // queries (16 B each) and the answer bits share the scratch row buffer
  if (!needScratch(c, kMaxOccupancyQueries)) return 0;
  std::vector<float4> q(count);
  for (uint32_t k = 0; k < count; ++k) { float w; std::memcpy(&w, &mask[k], 4); q[k] = make_float4(pos3[3 * k], pos3[3 * k + 2], radius[k], w); }
  float4* dq = reinterpret_cast<float4*>(c->dRows);
  uint32_t* bits = c->dIdx;
  uint32_t out[kMaxOccupancyQueries / 32] = {};
  HIP_OK(c, hipMemsetAsync(bits, 0, sizeof out, c->stream));
  if (!h2d(c, dq, q.data(), (size_t)count * 16u)) return 0;
  launchOccupancy(c->d, c->n, dq, count, bits, c->stream);
  if (!d2h(c, out, bits, sizeof out) || !sync(c)) return 0;
  for (uint32_t k = 0; k < count; ++k) blocked[k] = (uint8_t)((out[k >> 5] >> (k & 31u)) & 1u);
  return 1;
}

int scTickSetProfilingKernels(ScTickContext* c, uint32_t mask)
{
  if (!c) return 0;
  c->profMask = mask ? mask : 0xFFFFFFFFu;
  return 1;
}

int scTickSetProfiling(ScTickContext* c, int enable)
{
  if (!c) return 0;
  if (!bind(c)) return 0;
  if (enable) {
    sync(c);
    for (auto& v : c->times) { for (auto& p : v) c->eventPool.push_back(p); v.clear(); }
  }
  c->profiling = enable != 0;
  c->profPeriod = enable > 1 ? (uint32_t)enable : 1u;
  c->tickIndex = 0;
  return 1;
}

int scTickGetKernelTimes(ScTickContext* c, uint32_t kernel, float* ms, uint32_t cap, uint32_t* count)
{
  if (!c || !count || kernel >= SC_TICK_K_COUNT) return c ? fail(c, "bad argument") : 0;
  if (!bind(c) || !sync(c)) return 0;
  auto& v = c->times[kernel];
  *count = (uint32_t)v.size();
  for (uint32_t i = 0; i < v.size() && i < cap && ms; ++i) {
    float t = 0.0f;
    HIP_OK(c, hipEventElapsedTime(&t, v[i].a, v[i].b));
    ms[i] = t;
  }
  return 1;
}

int scTickSetGraphMode(ScTickContext* c, int enable)
{
  if (!c) return 0;
  if (!bind(c)) return 0;
  settle(c);                                           // (a replayed tick carries nothing)
  c->graphMode = enable != 0;
  if (!enable) { sync(c); dropCaptures(c); }
  return 1;
}

void* scTickGetStream(ScTickContext* c) { return c ? (void*)c->stream : nullptr; }

// ---- per-frame read-back ---------------------------------------------------------------------------------------------
int scTickSetFrameReadback(ScTickContext* c, uint32_t maxVisible, uint32_t maxDraws)
{
  if (!c) return 0;
  if (!bind(c)) return 0;
  settle(c);                                           // (a context with a read-back never defers: its frames read the lists on the device)
  if (!sync(c)) return 0;
  ScTickContext::FrameReadback& rb = c->rb;
  if (rb.copyStream) HIP_OK(c, hipStreamSynchronize(rb.copyStream));
  for (int k = 0; k < 2; ++k) { dfree(c, rb.dBlock[k]); rb.dBlock[k] = nullptr; if (rb.hBlock[k]) { hipHostFree(rb.hBlock[k]); rb.hBlock[k] = nullptr; } rb.inFlight[k] = false; }
  rb.bytes = 0; rb.frames = 0; rb.maxVisible = rb.maxDraws = 0;
  if (!maxVisible && !maxDraws) return reallocBindBlocks(c) ? 1 : 0;      // (the bind runs lose their staging blocks)
  if (maxVisible > c->cap || maxDraws > c->cap) return fail(c, "read-back sizes exceed the context's capacity");
  static_assert(sizeof(ScTickDrawItem) == kDrawItemBytes && offsetof(ScTickDrawItem, model) == 16, "the device writes the item as five float4");
  const size_t bytes = frameBlockBytes(maxVisible, maxDraws);
  if (!rb.copyStream) {
    HIP_OK(c, hipStreamCreateWithFlags(&rb.copyStream, hipStreamNonBlocking));
    for (int k = 0; k < 2; ++k) {
      HIP_OK(c, hipEventCreateWithFlags(&rb.staged[k], hipEventDisableTiming));
      HIP_OK(c, hipEventCreateWithFlags(&rb.copied[k], hipEventDisableTiming));
    }
  }
  for (int k = 0; k < 2; ++k) {
    if (!dalloc(c, rb.dBlock[k], bytes / 4u)) return 0;
    void* h = nullptr;
    HIP_OK(c, hipHostMalloc(&h, bytes, hipHostMallocDefault));
    std::memset(h, 0, bytes);
    rb.hBlock[k] = static_cast<uint32_t*>(h);
  }
  rb.maxVisible = maxVisible; rb.maxDraws = maxDraws; rb.bytes = bytes;
  dropGraphs(c->graph);
  return reallocBindBlocks(c) ? 1 : 0;      // (... or get them)
}

int scTickAcquireFrame(ScTickContext* c, uint32_t framesBack, ScTickFrame* out)
{
  if (!c || !out) return c ? fail(c, "null argument") : 0;
  ScTickContext::FrameReadback& rb = c->rb;
  if (!rb.bytes) return fail(c, "scTickSetFrameReadback first");
  if (framesBack > 1u) return fail(c, "frames_back must be 0 (the latest frame) or 1 (the one before): two frames are kept");
  if (rb.frames <= framesBack) return fail(c, "that frame has not been produced yet");
  if (!bind(c)) return 0;
  const uint32_t f = (uint32_t)((rb.frames - 1u - framesBack) & 1u);
  HIP_OK(c, hipEventSynchronize(rb.copied[f]));               // this frame's copy only: later work keeps running
  const uint32_t* h = rb.hBlock[f];
  std::memset(out, 0, sizeof *out);
  out->tick = (uint64_t)h[kFhTickLo] | ((uint64_t)h[kFhTickHi] << 32);
  out->visible = h[kFhVisible]; out->culled = h[kFhCulled]; out->renderables_total = h[kFhRenderablesTotal];
  out->draws_emitted = h[kFhDrawsEmitted]; out->draws_dropped = h[kFhDrawsDropped]; out->draws_sorted = h[kFhDrawsSorted];
  out->visible_in_buffer = h[kFhVisibleInBuffer]; out->draws_in_buffer = h[kFhDrawsInBuffer];
  out->visible_indices = h + kFrameHeaderWords;
  out->draws = reinterpret_cast<const ScTickDrawItem*>(frameItems(h, rb.maxVisible));
  return 1;
}

// ---- bind runs of the sorted draw list + material touch set (sc_tick_bindruns.hip; the spec is restated in include/sc_tick.h) --------
// runs: maximal stretches of equal (pipeline, material, mesh) among the first draws_sorted items, with the binds VkRenderer's loop issues
// ahead of each (sc_vk.cpp:1866-1907); touches: the handles RenderPrepStreamingSystem hands touchMaterial (sc_world_partition.cpp:1322-1326,
// sc_assets.cpp:441-445) -- every emitted draw's, inside the table, whatever its mesh.
int scTickSetBindRuns(ScTickContext* c, uint32_t maxRuns)
{
  static_assert(sizeof(ScTickBindRun) == sizeof(BindRun24) && sizeof(ScTickBindRun) == 24, "bind run layouts differ");
  static_assert(sizeof(ScTickBindInfo) == kBiWords * sizeof(uint32_t) && offsetof(ScTickBindInfo, materials_touched) == kBiMaterialsTouched * 4u &&
                offsetof(ScTickBindInfo, mesh_binds) == kBiMeshBinds * 4u, "the device writes the report word by word");
  if (!c) return 0;
  if (maxRuns && !c->sort.pipeline) return fail(c, "scTickSetBindRuns needs scTickSetDrawSortTable first (the touch bitmap is sized by its material_count)");
  if (maxRuns > c->cap) return fail(c, "max_runs exceeds the context's capacity (a list has at most one run per draw)");
  if (!bind(c) || !sync(c)) return 0;
  dropCaptures(c);       // a captured tick holds the old buffers (or none)
  return reallocBindRuns(c, maxRuns) ? 1 : 0;
}

static bool bindRunsReadable(ScTickContext* c)
{
  if (!(c->last.flags & SC_TICK_BIND_RUNS)) return fail(c, "the last scTickRun did not request SC_TICK_BIND_RUNS");
  if (!c->bind.info) return fail(c, "bind runs were switched off since the last scTickRun");
  if (c->bind.touchWords != c->lastWith.bindTouchWords) return fail(c, "the draw sort table was resized since the last scTickRun");
  return true;
}

int scTickReadBindRuns(ScTickContext* c, ScTickBindRun* runs, uint32_t cap, ScTickBindInfo* info)
{
  if (!c || !info) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !bindRunsReadable(c)) return 0;
  if (c->lastWith.bindEmpty) { std::memset(info, 0, sizeof *info); info->touch_words = c->lastWith.bindTouchWords; return 1; }
  if (!d2h(c, info, c->bind.info, sizeof *info) || !sync(c)) return 0;
  const uint32_t take = std::min(std::min(info->runs, c->bind.maxRuns), runs ? cap : 0u);
  if (take && (!d2h(c, runs, c->bind.runs, (size_t)take * sizeof(ScTickBindRun)) || !sync(c))) return 0;
  return 1;
}

int scTickReadMaterialTouches(ScTickContext* c, uint32_t* words, uint32_t wordCap, uint32_t* wordCount)
{
  if (!c || !wordCount) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !bindRunsReadable(c)) return 0;
  *wordCount = c->lastWith.bindTouchWords;
  const uint32_t take = std::min(c->lastWith.bindTouchWords, words ? wordCap : 0u);
  if (!take) return 1;
  if (c->lastWith.bindEmpty) { std::memset(words, 0, (size_t)take * 4u); return 1; }
  if (!d2h(c, words, c->bind.touch, (size_t)take * 4u) || !sync(c)) return 0;
  return 1;
}

int scTickAcquireFrameBinds(ScTickContext* c, uint32_t framesBack, ScTickFrameBinds* out)
{
  if (!c || !out) return c ? fail(c, "null argument") : 0;
  ScTickContext::FrameReadback& rb = c->rb;
  if (!rb.bytes) return fail(c, "scTickAcquireFrameBinds needs scTickSetFrameReadback first");
  if (!rb.bindBytes) return fail(c, "scTickAcquireFrameBinds needs scTickSetBindRuns first");
  if (framesBack > 1u) return fail(c, "frames_back must be 0 (the latest frame) or 1 (the one before): two frames are kept");
  if (rb.frames <= framesBack) return fail(c, "that frame has not been produced yet");
  if (!bind(c)) return 0;
  const uint64_t tick = rb.frames - 1u - framesBack;
  const uint32_t f = (uint32_t)(tick & 1u);
  HIP_OK(c, hipEventSynchronize(rb.copied[f]));               // the event scTickAcquireFrame waits on: the bind block is copied ahead of it
  std::memset(out, 0, sizeof *out);
  out->tick = tick;                                           // (what the frame's own header carries: its index at staging time)
  const uint32_t* h = rb.hBinds[f];
  out->runs = reinterpret_cast<const ScTickBindRun*>(h + kBiWords);
  out->touch_words = h + kBiWords + (size_t)c->bind.maxRuns * 6u;
  if (!rb.bindsStaged[f]) return 1;                           // a run without SC_TICK_BIND_RUNS: zeros, nothing in the buffer
  std::memcpy(&out->info, h, sizeof out->info);
  out->runs_in_buffer = std::min(out->info.runs, c->bind.maxRuns);
  return 1;
}

// ---- on-rails traffic: lane graph, agents, tier selection ----------------------------------------------
int scTickSetLaneGraph(ScTickContext* c, const ScTickLaneGraph* g)
{
  if (!c || !g) return c ? fail(c, "null argument") : 0;
  if (g->segments && (!g->seg_start3 || !g->seg_dir3 || !g->seg_length || !g->seg_end_node || !g->seg_speed_limit)) return fail(c, "null segment array");
  if (g->nodes && (!g->node_pos3 || !g->node_conn_offset)) return fail(c, "null node array");
  if (g->connections && !g->node_conn) return fail(c, "null connection array");
  for (uint32_t i = 0; i < g->segments; ++i) if (g->seg_end_node[i] >= g->nodes) return fail(c, "segment end node out of range");
  for (uint32_t i = 0; i < g->nodes; ++i) if (g->node_conn_offset[i] > g->node_conn_offset[i + 1]) return fail(c, "node connection offsets must ascend");
  if (g->nodes && g->node_conn_offset[g->nodes] != g->connections) return fail(c, "node_conn_offset[nodes] != connections");
  if (!bind(c) || !sync(c)) return 0;
  for (void*& p : c->laneAllocs) { dfree(c, p); p = nullptr; }
  std::vector<float4> A(g->segments), B(g->segments), P(g->nodes);
  std::vector<uint4> C(g->segments);
  for (uint32_t i = 0; i < g->segments; ++i) {
    const float* st = g->seg_start3 + 3 * (size_t)i; const float* dr = g->seg_dir3 + 3 * (size_t)i;
    A[i] = make_float4(st[0], st[1], st[2], g->seg_length[i]);
    B[i] = make_float4(dr[0], dr[1], dr[2], g->seg_speed_limit[i]);
    // yawFromDir (sc_traffic_ai.cpp:72-75) and then the sin / cos mat4_rotation_xyz takes of it (sc_math.cpp:102-107), host libm
    const float yaw = std::atan2(dr[0], dr[2]);
    const float sy = std::sin(yaw), cy = std::cos(yaw);
    uint32_t sb, cb; std::memcpy(&sb, &sy, 4); std::memcpy(&cb, &cy, 4);
    C[i] = make_uint4(g->seg_end_node[i], (!g->seg_active || g->seg_active[i]) ? 1u : 0u, sb, cb);
  }
  for (uint32_t i = 0; i < g->nodes; ++i) P[i] = make_float4(g->node_pos3[3 * (size_t)i], g->node_pos3[3 * (size_t)i + 1], g->node_pos3[3 * (size_t)i + 2], 0.0f);
  float4 *dA = nullptr, *dB = nullptr, *dP = nullptr; uint4* dC = nullptr; uint32_t *dOff = nullptr, *dConn = nullptr;
  if (!dalloc(c, dA, g->segments, false) || !dalloc(c, dB, g->segments, false) || !dalloc(c, dC, g->segments, false) ||
      !dalloc(c, dP, g->nodes, false) || !dalloc(c, dOff, (size_t)g->nodes + 1u) || !dalloc(c, dConn, g->connections, false)) return 0;
  c->laneAllocs[0] = dA; c->laneAllocs[1] = dB; c->laneAllocs[2] = dC; c->laneAllocs[3] = dP; c->laneAllocs[4] = dOff; c->laneAllocs[5] = dConn;
  bool ok = true;
  if (g->segments) ok = h2d(c, dA, A.data(), A.size() * 16u) && h2d(c, dB, B.data(), B.size() * 16u) && h2d(c, dC, C.data(), C.size() * 16u);
  if (ok && g->nodes) ok = h2d(c, dP, P.data(), P.size() * 16u) && h2d(c, dOff, g->node_conn_offset, ((size_t)g->nodes + 1u) * 4u);
  if (ok && g->connections) ok = h2d(c, dConn, g->node_conn, (size_t)g->connections * 4u);
  if (!ok || !sync(c)) return 0;
  LaneGraphDev& L = c->d.lanes;
  L.segA = dA; L.segB = dB; L.segC = dC; L.nodePos = dP; L.nodeConnOff = dOff; L.nodeConn = dConn; L.segments = g->segments; L.nodes = g->nodes;
  c->topoEpoch++;                       // captured graphs hold the old table pointers
  return 1;
}

int scTickSetLaneActive(ScTickContext* c, const uint32_t* segIds, uint32_t count, int active)
{
  if (!c || (!segIds && count)) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !sync(c)) return 0;
  for (uint32_t k = 0; k < count; ++k) {
    if (segIds[k] >= c->d.lanes.segments) return fail(c, "segment id out of range");
    const uint32_t v = active ? 1u : 0u;
    if (!h2d(c, reinterpret_cast<uint32_t*>(const_cast<uint4*>(c->d.lanes.segC) + segIds[k]) + 1, &v, 4u)) return 0;
    if (!sync(c)) return 0;           // `v` dies with the iteration
  }
  return 1;
}

int scTickSetTrafficSpeedMultiplier(ScTickContext* c, float multiplier)
{
  if (!c) return 0;
  if (!bind(c) || !sync(c)) return 0;
  dropGraphs(c->graph);
  c->trafficMult = multiplier;
  return 1;
}

int scTickUploadTrafficAgents(ScTickContext* c, uint32_t first, uint32_t count, const uint8_t* isAgent, const uint32_t* laneId,
                              const float* laneS, const float* targetSpeed, const uint8_t* mode, const float* lookAhead)
{
  if (!c || !isAgent || !laneId || !laneS || !targetSpeed || !mode) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  DeviceState& d = c->d;
  const size_t N = c->cap;
  if (!d.moverKind && (!dalloc(c, d.moverKind, N) || !dalloc(c, d.mvx, N) || !dalloc(c, d.mvz, N) || !dalloc(c, d.mlox, N) ||
                       !dalloc(c, d.mloz, N) || !dalloc(c, d.mhix, N) || !dalloc(c, d.mhiz, N))) return 0;
  if (!d.aLane && (!dalloc(c, d.aLane, N) || !dalloc(c, d.aS, N) || !dalloc(c, d.aSpeed, N) || !dalloc(c, d.aMode, N) || !dalloc(c, d.aLook, N) ||
                   !dalloc(c, d.aDesired, N) || !dalloc(c, d.tierCounts, 4) || !dalloc(c, d.tierNear, kTierNearCap, false) || !dalloc(c, c->dTierPatch, kTierNearCap, false))) return 0;
  if (!count) return 1;
  if (!sync(c)) return 0;
  std::vector<uint32_t> kind(count), md(count);
  std::vector<float> look(count);
  if (!d2h(c, kind.data(), d.moverKind + first, (size_t)count * 4u) || !sync(c)) return 0;
  for (uint32_t i = 0; i < count; ++i) {
    if (mode[i] > 2u) return fail(c, "mode must be 0 (Physics), 1 (Kinematic) or 2 (OnRails)");
    if (isAgent[i]) kind[i] = kMoverTraffic; else if (kind[i] == kMoverTraffic) kind[i] = 0u;
    md[i] = mode[i];
    look[i] = lookAhead ? lookAhead[i] : 12.0f;              // TrafficAgent::lookAheadDist, sc_traffic_common.h:32
    uint8_t& f = c->hFlags[first + i];
    const uint8_t nf = isAgent[i] ? (uint8_t)((f | 32u) & ~8u) : (uint8_t)(f & ~32u);
    if (nf != f) { f = nf; c->linksStale = true; }            // an agent's yaw is always streamed (the device rewrites it; X and Z it sets to (0, 1))
  }
  const bool ok = h2d(c, d.moverKind + first, kind.data(), (size_t)count * 4u) && h2d(c, d.aLane + first, laneId, (size_t)count * 4u) &&
                  h2d(c, d.aS + first, laneS, (size_t)count * 4u) && h2d(c, d.aSpeed + first, targetSpeed, (size_t)count * 4u) &&
                  h2d(c, d.aMode + first, md.data(), (size_t)count * 4u) && h2d(c, d.aLook + first, look.data(), (size_t)count * 4u);
  return ok && sync(c) ? 1 : 0;
}

int scTickSetTrafficSensors(ScTickContext* c, int enable, float frontRayLength, float safeDistance)
{
  if (!c) return 0;
  if (!bind(c) || !sync(c)) return 0;
  if (enable) {
    if (!c->d.aLane) return fail(c, "no traffic agents uploaded");
    if (!c->sectors) return fail(c, "the obstacle rays read the broadphase bins: the context has no tile rectangle");
    if (!(frontRayLength >= 0.0f) || !(safeDistance >= 0.0f)) return fail(c, "ray length and safe distance must be >= 0");
    if (!c->d.aBrake && (!dalloc(c, c->d.aBrake, c->cap) || !dalloc(c, c->d.agentList, c->cap, false) || !dalloc(c, c->d.agentCount, 4) ||
                         !dalloc(c, c->d.aRayLen, c->cap) || !dalloc(c, c->d.aSafe, c->cap) || !dalloc(c, c->d.aHitDist, c->cap) || !dalloc(c, c->d.aHitType, c->cap))) return 0;
    if (!c->d.agentRays && !dalloc(c, c->d.agentRays, 2u * (size_t)c->cap, false)) return 0;
    c->sensorRay = frontRayLength; c->sensorSafe = safeDistance;
    launchFillSensors(c->d, 0, c->cap, frontRayLength, safeDistance, c->stream);        // every agent's TrafficSensors = these defaults until scTickUploadTrafficSensors says otherwise
    if (!sync(c)) return 0;
  } else if (c->d.aBrake) {
    HIP_OK(c, hipMemsetAsync(c->d.aBrake, 0, (size_t)c->cap * sizeof(float), c->stream));      // no sensors: brake 0 from here on
    if (!sync(c)) return 0;
  }
  // On a tiled world an agent near a tile edge has to see the neighbour's boxes: the border messages then carry the halo section (the
  // sender's core-edge records), which changes their size -- so the sensors must be switched before the message buffers exist
  // (scTickBindBorderBuffers* / scTickCommInit), on every tile alike.
  const bool wantHalo = enable != 0;
  if (wantHalo != c->halo) {
    bool bound = c->comm != nullptr;
    for (uint32_t d = 0; d < 8 && !bound; ++d) bound = c->d.borderSend[d] || c->d.borderRecv[d];
    if (bound) return fail(c, "on a tile with border buffers or a communicator the traffic sensors cannot be switched any more: the messages' halo section changes their size (call scTickSetTrafficSensors before scTickBindBorderBuffers / scTickCommInit, on every tile)");
    c->halo = wantHalo;
  }
  c->sensors = enable != 0;
  dropCaptures(c); c->topoEpoch++;
  return 1;
}

int scTickUploadTrafficSensors(ScTickContext* c, uint32_t first, uint32_t count, const float* frontRayLength, const float* safeDistance)
{
  if (!c || !frontRayLength || !safeDistance) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!c->d.aRayLen) return fail(c, "scTickSetTrafficSensors first");
  for (uint32_t i = 0; i < count; ++i)
    if (!(frontRayLength[i] >= 0.0f) || !(safeDistance[i] >= 0.0f)) return fail(c, "ray length and safe distance must be >= 0");
  if (!count) return 1;
  return h2d(c, c->d.aRayLen + first, frontRayLength, (size_t)count * 4u) && h2d(c, c->d.aSafe + first, safeDistance, (size_t)count * 4u) && sync(c) ? 1 : 0;
}

int scTickReadTrafficSensors(ScTickContext* c, uint32_t first, uint32_t count, float* lastHitDistance, uint8_t* lastHitType)
{
  if (!c || !lastHitDistance || !lastHitType) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!c->d.aHitDist) return fail(c, "scTickSetTrafficSensors first");
  if (!count) return 1;
  if (!joinPairs(c)) return 0;                            // (on a tiled world the rays are cast in the pair half)
  std::vector<uint32_t> typ(count);
  if (!d2h(c, lastHitDistance, c->d.aHitDist + first, (size_t)count * 4u) || !d2h(c, typ.data(), c->d.aHitType + first, (size_t)count * 4u) || !sync(c)) return 0;
  for (uint32_t i = 0; i < count; ++i) lastHitType[i] = (uint8_t)typ[i];
  return 1;
}

int scTickReadTrafficBrakes(ScTickContext* c, uint32_t first, uint32_t count, float* brake)
{
  if (!c || !brake) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!c->d.aBrake) return fail(c, "scTickSetTrafficSensors first");
  if (!count) return 1;
  return d2h(c, brake, c->d.aBrake + first, (size_t)count * 4u) && sync(c) ? 1 : 0;
}

int scTickReadTrafficAgents(ScTickContext* c, uint32_t first, uint32_t count, uint32_t* laneId, float* laneS, float* targetSpeed, uint8_t* mode)
{
  if (!c) return 0;
  if (!bind(c) || !rangeOk(c, first, count)) return 0;
  if (!c->d.aLane) return fail(c, "no traffic agents uploaded");
  if (!count) return 1;
  std::vector<uint32_t> md(count);
  bool ok = true;
  if (laneId) ok = ok && d2h(c, laneId, c->d.aLane + first, (size_t)count * 4u);
  if (laneS) ok = ok && d2h(c, laneS, c->d.aS + first, (size_t)count * 4u);
  if (targetSpeed) ok = ok && d2h(c, targetSpeed, c->d.aSpeed + first, (size_t)count * 4u);
  if (mode) ok = ok && d2h(c, md.data(), c->d.aMode + first, (size_t)count * 4u);
  if (!ok || !sync(c)) return 0;
  if (mode) for (uint32_t i = 0; i < count; ++i) mode[i] = (uint8_t)md[i];
  return 1;
}

int scTickSelectTrafficTiers(ScTickContext* c, const float playerPos[3], const ScTickTierParams* tp, ScTickTierCounts* out)
{
  if (!c || !playerPos || !tp) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !flushLinks(c)) return 0;
  if (!c->d.aLane) return fail(c, "no traffic agents uploaded");
  TierParams k;
  k.px = playerPos[0]; k.pz = playerPos[2];
  k.aEnter = tp->tier_a_enter; k.aExit = tp->tier_a_exit; k.bEnter = tp->tier_b_enter; k.bExit = tp->tier_b_exit;
  if (k.aExit < k.aEnter + 1.0f) k.aExit = k.aEnter + 1.0f;           // sc_traffic_lod.cpp:269-274
  if (k.bEnter < k.aExit + 1.0f) k.bEnter = k.aExit + 1.0f;
  if (k.bExit < k.bEnter + 1.0f) k.bExit = k.bEnter + 1.0f;
  HIP_OK(c, hipMemsetAsync(c->d.tierCounts, 0, 4 * sizeof(uint32_t), c->stream));
  launchTrafficTiers(c->d, c->n, k, c->stream);
  uint32_t cnt[4] = {};
  if (!d2h(c, cnt, c->d.tierCounts, sizeof cnt) || !sync(c)) return 0;
  if (cnt[3] > kTierNearCap) return fail(c, "more than 65536 agents want the Physics or Kinematic tier");
  std::vector<uint2> nearList(cnt[3]);
  if (cnt[3] && (!d2h(c, nearList.data(), c->d.tierNear, (size_t)cnt[3] * 8u) || !sync(c))) return 0;
  // the order ForEach would visit them in (Transform-pool dense order): the list arrives in atomic order
  std::sort(nearList.begin(), nearList.end(), [](const uint2& a, const uint2& b) { return a.x < b.x; });
  uint32_t physicsCount = cnt[0], kinematicCount = cnt[1], onRailsCount = cnt[2];
  std::vector<uint8_t> des(nearList.size());
  std::vector<float> dist(nearList.size());
  for (size_t q = 0; q < nearList.size(); ++q) {
    const uint32_t bits = nearList[q].y & 0x7FFFFFFFu;
    std::memcpy(&dist[q], &bits, 4);
    des[q] = (uint8_t)((nearList[q].y >> 31) ? kTierKinematic : kTierPhysics);
  }
  // the caps, sc_traffic_lod.cpp:355-417: candidates sorted by distance, descending (std::sort there; stable here, so equal
  // distances keep their pool order), everything past the cap is demoted
  std::vector<uint2> patches;
  auto byDistDesc = [&](uint32_t a, uint32_t b) { return dist[a] > dist[b]; };
  if (tp->max_physics > 0 && physicsCount > tp->max_physics) {
    std::vector<uint32_t> phys;
    for (uint32_t q = 0; q < des.size(); ++q) if (des[q] == kTierPhysics) phys.push_back(q);
    std::stable_sort(phys.begin(), phys.end(), byDistDesc);
    for (size_t a = tp->max_physics; a < phys.size(); ++a) {
      if (tp->max_kinematic == 0 || kinematicCount < tp->max_kinematic) { des[phys[a]] = (uint8_t)kTierKinematic; kinematicCount++; }
      else { des[phys[a]] = (uint8_t)kTierOnRails; onRailsCount++; }
      physicsCount--;
    }
  }
  if (tp->max_kinematic > 0 && kinematicCount > tp->max_kinematic) {
    std::vector<uint32_t> kin;
    for (uint32_t q = 0; q < des.size(); ++q) if (des[q] == kTierKinematic) kin.push_back(q);
    std::stable_sort(kin.begin(), kin.end(), byDistDesc);
    for (size_t a = tp->max_kinematic; a < kin.size(); ++a) { des[kin[a]] = (uint8_t)kTierOnRails; kinematicCount--; onRailsCount++; }
  }
  for (uint32_t q = 0; q < des.size(); ++q) patches.push_back(make_uint2(nearList[q].x, des[q]));
  if (!patches.empty() && !h2d(c, c->dTierPatch, patches.data(), patches.size() * 8u)) return 0;
  launchApplyTiers(c->d, c->n, c->dTierPatch, (uint32_t)patches.size(), c->stream);
  if (!sync(c)) return 0;
  if (out) { out->physics = physicsCount; out->kinematic = kinematicCount; out->on_rails = onRailsCount; out->total = physicsCount + kinematicCount + onRailsCount; }
  return 1;
}

int scTickSelectTrafficDespawns(ScTickContext* c, const float playerPos[3], uint32_t maxTotal, uint32_t* denseIndices, uint32_t capacity, uint32_t* count)
{
  if (!c || !playerPos || !count) return c ? fail(c, "null argument") : 0;
  *count = 0;
  if (!bind(c) || !flushLinks(c)) return 0;
  if (!c->d.aLane) return fail(c, "no traffic agents uploaded");
  if (maxTotal == 0 || !c->n) return 1;                                  // dbg.maxTrafficVehiclesTotal == 0: no cap (:421)
  // every agent with its ordering key, then the top of the order on the host (the list is short-lived scratch)
  uint32_t* dCount = nullptr; uint32_t* dIdx = nullptr; unsigned long long* dKey = nullptr;
  if (!dalloc(c, dCount, 4, false) || !dalloc(c, dIdx, c->n, false) || !dalloc(c, dKey, c->n, false)) return 0;
  // (zeroed on the tick stream itself: a hipMemset on the null stream is not ordered against a non-blocking stream)
  if (hipMemsetAsync(dCount, 0, 4 * sizeof(uint32_t), c->stream) != hipSuccess) { dfree(c, dCount); dfree(c, dIdx); dfree(c, dKey); return fail(c, "hipMemsetAsync"); }
  launchTrafficDespawnKeys(c->d, c->n, playerPos[0], playerPos[2], dCount, dIdx, dKey, c->stream);
  uint32_t agents = 0;
  int ok = d2h(c, &agents, dCount, sizeof agents) && sync(c);
  std::vector<uint32_t> idx; std::vector<unsigned long long> key;
  if (ok && agents > maxTotal) {
    idx.resize(agents); key.resize(agents);
    ok = d2h(c, idx.data(), dIdx, (size_t)agents * 4u) && d2h(c, key.data(), dKey, (size_t)agents * 8u) && sync(c);
  }
  dfree(c, dCount); dfree(c, dIdx); dfree(c, dKey);
  if (!ok) return 0;
  if (agents <= maxTotal) return 1;
  const uint32_t toRemove = agents - maxTotal;
  std::vector<uint32_t> order(agents);
  for (uint32_t k = 0; k < agents; ++k) order[k] = k;
  // OnRails before Kinematic before Physics, the farthest first; equal keys in pool order (std::sort there leaves it unspecified)
  auto before = [&](uint32_t a, uint32_t b) { return key[a] != key[b] ? key[a] > key[b] : idx[a] < idx[b]; };
  std::partial_sort(order.begin(), order.begin() + toRemove, order.end(), before);
  *count = toRemove;
  for (uint32_t k = 0; k < toRemove && k < capacity && denseIndices; ++k) denseIndices[k] = idx[order[k]];
  return 1;
}

int scTickSetWorldLayers(ScTickContext* c, uint32_t groupOr, uint32_t maskOr, int known)
{
  if (!c) return 0;
  if (!bind(c)) return 0;
  if (known && (((groupOr != 0xFFFFFFFFu) && (groupOr >> 16)) || ((maskOr != 0xFFFFFFFFu) && (maskOr >> 16)))) return fail(c, "group/mask bits above 15 are not supported");
  const uint32_t v = known ? ((groupOr & 0xFFFFu) | ((maskOr & 0xFFFFu) << 16)) : 0u;
  if (known) {                                        // the contract holds for what is already here, too
    const size_t upto = std::min<size_t>(c->hLayers.size(), c->n);
    for (size_t i = 0; i < upto; ++i)
      if (hasProxyHost(c, (uint32_t)i) && (c->hLayers[i] & ~v)) return fail(c, "the vocabulary does not cover the layers already uploaded to this tile");
  }
  if ((known != 0) != c->worldLayersKnown || v != c->worldLayers) {
    if (!sync(c)) return 0;
    c->worldLayersKnown = known != 0; c->worldLayers = v;
    c->homeValid = false;               // the slots' "written on every tick" bits follow the vocabulary
  }
  return 1;
}

int scTickGetLearnTicks(ScTickContext* c, uint32_t* learn_ticks)
{
  if (!c || !learn_ticks) return c ? fail(c, "null argument") : 0;
  *learn_ticks = c->learnTicks;            // (host-side: no read-back, no synchronisation)
  return 1;
}

int scTickGetBoundsClassStats(ScTickContext* c, uint32_t stats[4])
{
  if (!c || !stats) return c ? fail(c, "null argument") : 0;
  stats[0] = (uint32_t)c->paletteIndex.size(); stats[1] = stats[2] = stats[3] = 0u;
  for (uint32_t t = 0; t < (c->n + 63u) / 64u; ++t) {
    const uint32_t w = c->hTile[2u * (size_t)t];
    if (w & kTileNoBounds) continue;
    if ((w & kClassMask) < kPaletteCap) stats[1]++; else stats[2]++;
  }
  for (uint32_t i = 0; i < c->n; ++i) if ((c->hFlags[i] & 2u) && c->hClass[i] == kClassNone) stats[3]++;
  return 1;
}

int scTickGetTopologyClassStats(ScTickContext* c, uint32_t stats[4])
{
  if (!c || !stats) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !flushLinks(c)) return 0;
  stats[0] = c->topoPatterns; stats[1] = c->topoClassed; stats[2] = c->topoUnclassed;
  stats[3] = c->last.topo ? 1u : 0u;
  return 1;
}

int scTickGetTailStats(ScTickContext* c, uint32_t stats[2])
{
  if (!c || !stats) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !flushLinks(c)) return 0;
  uint32_t span, grid;
  computeSpan(c, span, grid);
  if (span != c->closureSpan) deriveSpanClosed(c);
  stats[0] = c->last.tail ? 1u : 0u;
  stats[1] = c->spanClosed ? 1u : 0u;
  return 1;
}

int scTickGetCompactStats(ScTickContext* c, uint32_t stats[2])
{
  if (!c || !stats) return c ? fail(c, "null argument") : 0;
  stats[0] = c->last.compact[0]; stats[1] = c->last.compact[1];
  return 1;
}

int scTickGetCarryStats(ScTickContext* c, uint32_t stats[3])
{
  if (!c || !stats) return c ? fail(c, "null argument") : 0;
  for (int k = 0; k < 3; ++k) stats[k] = c->carryStats[k];
  return 1;
}

int scTickGetFrameStats(ScTickContext* c, uint32_t stats[2])
{
  if (!c || !stats) return c ? fail(c, "null argument") : 0;
  stats[0] = c->last.frame[0]; stats[1] = c->last.frame[1];
  return 1;
}

int scTickGetBinStats(ScTickContext* c, uint32_t stats[4])
{
  if (!c || !stats) return c ? fail(c, "null argument") : 0;
  stats[0] = stats[1] = stats[2] = stats[3] = 0u;
  if (!bind(c)) return 0;
  if (!c->d.homeA || !c->n) return 1;
  stats[2] = (c->lastBinned.lazy ? 1u : 0u) | (c->lastBinned.stay ? 2u : 0u) | (c->lastBinned.sweepOnly ? 4u : 0u) | (c->last.quiet ? 8u : 0u); stats[3] = c->learnTicks;
  if (!c->homeValid) return 1;
  if (!sync(c)) return 0;
  std::vector<uint32_t> a(c->n), b(c->n);
  if (!d2h(c, a.data(), c->d.homeA, (size_t)c->n * 4u) || !d2h(c, b.data(), c->d.homeB, (size_t)c->n * 4u) || !sync(c)) return 0;
  for (uint32_t i = 0; i < c->n; ++i) {
    if (a[i] == kNoHome) continue;
    for (uint32_t k = 0; k < 4u; ++k) {
      const uint32_t byte = (b[i] >> (8u * k)) & 0xFFu;
      if (byte == kNoSlot) continue;
      stats[0]++; if (byte & kSlotAlways) stats[1]++;
    }
  }
  return 1;
}

// ---- the border exchange, owned by the library -------------------------------------------------------------------
static const RcclApi* needRccl(ScTickContext* c)
{
  std::string why;
  const RcclApi* r = rccl(&why);
  if (!r) { if (c) fail(c, why.c_str()); else gCreateError = why; }
  return r;
}

static bool ncclOk(ScTickContext* c, const RcclApi* r, ncclResult_t res, const char* what)
{
  if (res == ncclSuccess) return true;
  char buf[256];
  std::snprintf(buf, sizeof buf, "%s: %s", what, r->GetErrorString(res));
  if (c) fail(c, buf); else gCreateError = buf;
  return false;
}

int scTickCommGetUniqueId(uint8_t id[SC_TICK_COMM_ID_BYTES])
{
  if (!id) return 0;
  const RcclApi* r = needRccl(nullptr);
  if (!r) return 0;
  static_assert(sizeof(ncclUniqueId) == SC_TICK_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
  ncclUniqueId u;
  if (!ncclOk(nullptr, r, r->GetUniqueId(&u), "ncclGetUniqueId")) return 0;
  std::memcpy(id, &u, sizeof u);
  return 1;
}

int scTickCommDestroy(ScTickContext* c)
{
  if (!c) return 0;
  if (!c->comm) return 1;
  if (!bind(c)) return 0;
  sync(c);
  const RcclApi* r = needRccl(c);
  // captured steps hold ncclSend / ncclRecv nodes bound to this communicator and to the peers' ranks
  dropCaptures(c); c->topoEpoch++;
  if (r) r->CommDestroy(c->comm);
  c->comm = nullptr; c->commSize = 0; c->commRank = 0;
  return 1;
}

int scTickCommSetPeers(ScTickContext* c, const int32_t peerRank[8])
{
  if (!c || !peerRank) return c ? fail(c, "null argument") : 0;
  if (!bind(c) || !sync(c)) return 0;
  dropCaptures(c); c->topoEpoch++;       // a captured exchange names the old ranks
  for (int d = 0; d < 8; ++d) c->peer[d] = peerRank[d];
  c->peersSet = true;
  return 1;
}

int scTickCommInit(ScTickContext* c, const uint8_t id[SC_TICK_COMM_ID_BYTES], uint32_t worldSize, uint32_t rank)
{
  if (!c || !id) return c ? fail(c, "null argument") : 0;
  if (!worldSize || rank >= worldSize) return fail(c, "need rank < world_size");
  if (!c->sectors) return fail(c, "the context has no broadphase: nothing to exchange");
  if (!c->tilesX) return fail(c, "scTickSetTileGrid first (the neighbours' ranks follow from the tile's place in the grid)");
  if (c->pairsPending) return fail(c, "scTickRunPairs is pending");
  if (!bind(c) || !sync(c)) return 0;
  const RcclApi* r = needRccl(c);
  if (!r) return 0;
  if (c->comm && !scTickCommDestroy(c)) return 0;
  if (!c->peersSet) {
    // tiles in row-major rank order, as the entities are created tile-major
    if ((uint64_t)c->tilesX * c->tilesZ != worldSize) return fail(c, "world_size differs from the tile grid (use scTickCommSetPeers for another rank layout)");
    for (uint32_t d = 0; d < 8; ++d) {
      int dx, dz; borderDir(d, dx, dz);
      c->peer[d] = ((c->neighbourMask >> d) & 1u) ? (int32_t)(((int)c->tileZ + dz) * (int)c->tilesX + (int)c->tileX + dx) : -1;
    }
  }
  for (uint32_t d = 0; d < 8; ++d)
    if (((c->neighbourMask >> d) & 1u) && (c->peer[d] < 0 || (uint32_t)c->peer[d] >= worldSize)) return fail(c, "a neighbour's rank lies outside the communicator");
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  if (!ncclOk(c, r, r->CommInitRank(&c->comm, (int)worldSize, u, (int)rank), "ncclCommInitRank")) { c->comm = nullptr; return 0; }
  c->commSize = worldSize; c->commRank = rank;
  dropCaptures(c); c->topoEpoch++;       // (a graph captured against an earlier communicator must not be replayed)
  // the messages of both tick parities live in buffers of the library's own (a caller that runs its own transport binds
  // its buffers with scTickBindBorderBuffers instead and never comes here)
  for (uint32_t q = 0; q < kMaxParity; ++q)
    for (uint32_t d = 0; d < 8; ++d) {
      if (!((c->neighbourMask >> d) & 1u)) continue;
      const size_t words = borderWords(d, c->desc.tile_sectors_x, c->desc.tile_sectors_z, c->borderRecs, c->halo ? 1u : 0u);
      for (int k = 0; k < 2; ++k) if (!c->ownBorder[q][d][k] && !dalloc(c, c->ownBorder[q][d][k], words)) return 0;
      if (q == 0) { c->d.borderSend[d] = c->ownBorder[0][d][0]; c->d.borderRecv[d] = c->ownBorder[0][d][1]; }
      else { c->alt[q - 1u].borderSend[d] = c->ownBorder[q][d][0]; c->alt[q - 1u].borderRecv[d] = c->ownBorder[q][d][1]; }
    }
  return sync(c) ? 1 : 0;
}

int scTickGetCommInfo(ScTickContext* c, ScTickCommInfo* out)
{
  if (!c || !out) return c ? fail(c, "null argument") : 0;
  std::memset(out, 0, sizeof *out);
  out->world_size = c->commSize; out->rank = c->commRank; out->has_communicator = c->comm ? 1u : 0u;
  out->neighbour_mask = c->neighbourMask;
  out->pipeline_depth = c->pairsStream ? c->pipeDepth : 0u;
  out->border_records_per_sector = c->borderRecs;
  for (uint32_t d = 0; d < 8; ++d) {
    out->peer_rank[d] = ((c->neighbourMask >> d) & 1u) ? c->peer[d] : -1;
    if (!((c->neighbourMask >> d) & 1u) || !c->sectors) continue;
    out->operations_per_group += 2u;                                   // one ncclSend + one ncclRecv per neighbour
    out->bytes_sent_per_step += (uint64_t)borderWords(d, c->desc.tile_sectors_x, c->desc.tile_sectors_z, c->borderRecs, c->halo ? 1u : 0u) * 4u;
  }
  if (c->comm) { std::string why; if (const RcclApi* r = rccl(&why)) { int v = 0; if (r->GetVersion(&v) == ncclSuccess) out->rccl_version = (uint32_t)v; } }
  out->host_steps = c->hostSteps;
  out->host_tick_half_us = c->hostSteps ? c->hostAcc[0] / (double)c->hostSteps : 0.0;
  out->host_pair_half_us = c->hostSteps ? c->hostAcc[1] / (double)c->hostSteps : 0.0;
  return 1;
}

int scTickGatherVisibleCounts(ScTickContext* c, uint32_t* countsOut, uint32_t capacity, uint64_t* offsetOut, uint64_t* totalOut)
{
  if (!c || !offsetOut || !totalOut) return c ? fail(c, "null argument") : 0;
  if (!bind(c)) return 0;
  settle(c);
  if (!sync(c)) return 0;                                  // both streams idle: the collective below is the communicator's only operation in flight
  const uint32_t ranks = c->comm ? c->commSize : 1u;
  std::vector<uint32_t> counts(ranks, 0u);
  if (!c->comm) {
    if (!d2h(c, counts.data(), c->d.counters, sizeof(uint32_t)) || !sync(c)) return 0;
  } else {
    const RcclApi* r = needRccl(c);
    if (!r) return 0;
    if (c->gatherCap < ranks) {
      dfree(c, c->dGather); c->dGather = nullptr; c->gatherCap = 0;
      if (!dalloc(c, c->dGather, ranks)) return 0;
      c->gatherCap = ranks;
    }
    if (!ncclOk(c, r, r->AllGather(c->d.counters, c->dGather, 1, ncclUint32, c->comm, c->stream), "ncclAllGather (visible counts)")) return 0;
    if (!d2h(c, counts.data(), c->dGather, (size_t)ranks * sizeof(uint32_t)) || !sync(c)) return 0;
  }
  uint64_t before = 0, total = 0;
  const uint32_t me = c->comm ? c->commRank : 0u;
  for (uint32_t k = 0; k < ranks; ++k) { if (k < me) before += counts[k]; total += counts[k]; }
  if (countsOut) for (uint32_t k = 0; k < ranks && k < capacity; ++k) countsOut[k] = counts[k];
  *offsetOut = before; *totalOut = total;
  return 1;
}

int scTickResetHostTimes(ScTickContext* c)
{
  if (!c) return 0;
  c->hostAcc[0] = c->hostAcc[1] = 0.0; c->hostSteps = 0;
  return 1;
}

int scTickSetPipelined(ScTickContext* c, int enable)
{
  if (!c) return 0;
  if (!bind(c)) return 0;
  settle(c);
  if (!enable) return scTickSetPairsStream(c, nullptr);
  if (enable < 0 || enable > (int)kMaxParity) return fail(c, "pipeline depth must be 2..4 (1 = the default, 4; 0 = off)");
  // depth d: the pair half of a tick may take up to d - 2 ticks before it holds anything up (a tick's counters are cleared by
  // the tick before it, which therefore waits for the pair half d - 1 ticks back).  4 on the loop-back: 56 us per step
  // against 63 with 3; 2 leaves no overlap of the pair half with the next tick at all.
  const uint32_t depth = enable == 1 ? 4u : (uint32_t)enable;
  if (depth != c->pipeDepth) {
    if (c->pairsStream && !scTickSetPairsStream(c, nullptr)) return 0;     // re-enter with the new depth
    c->pipeDepth = depth;
  }
  // (a high-priority pairs stream was measured: no gain, 94 against 90 us per step with the loop-back exchange)
  if (!c->ownPairsStream) HIP_OK(c, hipStreamCreateWithFlags(&c->ownPairsStream, hipStreamNonBlocking));
  return scTickSetPairsStream(c, c->ownPairsStream);
}

// send[d] of this tile -> recv[7-d] of the neighbour in direction d, every existing neighbour, one RCCL group on `s`.
// A pair of ranks normally shares one edge or corner, i.e. one message each way; should a rank layout put several
// neighbours on one rank (scTickCommSetPeers: a periodic world, the loop-back test), point-to-point operations between
// two ranks match in posting order: sends go out by ascending direction, so the receives are posted by DESCENDING
// direction -- what a peer sent as its direction d arrives here as direction 7-d.
// inCapture: what the caller believes about `s`.  The group is only opened when the stream's capture state is that one: an
// RCCL group posted to a stream that is (or is not) being captured against the caller's expectation -- a capture that was
// invalidated half way, a stream forked into somebody else's capture -- is refused here instead of being handed to RCCL.
static int exchangeBorders(ScTickContext* c, uint32_t parity, hipStream_t s, bool inCapture)
{
  const RcclApi* r = needRccl(c);
  if (!r) return 0;
  if (!c->comm) return fail(c, "no communicator: scTickCommInit first");
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  const hipError_t qe = hipStreamIsCapturing(s, &st);
  if (qe != hipSuccess) return fail(c, "hipStreamIsCapturing", qe);
  if ((st == hipStreamCaptureStatusActive) != inCapture)
    return fail(c, inCapture ? "border exchange: the stream is not being captured although a capture was begun (capture invalidated?)"
                             : "border exchange: the stream is being captured by somebody else");
  const DeviceState ds = stateFor(c, parity);
  if (!ncclOk(c, r, r->GroupStart(), "ncclGroupStart")) return 0;
  ncclResult_t res = ncclSuccess;
  for (int d = 0; d < 8 && res == ncclSuccess; ++d) {
    if (!((c->neighbourMask >> d) & 1u)) continue;
    if (!ds.borderSend[d] || !ds.borderRecv[d]) { r->GroupEnd(); return fail(c, "border buffers are not bound"); }
    res = r->Send(ds.borderSend[d], (size_t)borderWords((uint32_t)d, c->desc.tile_sectors_x, c->desc.tile_sectors_z, c->borderRecs, c->halo ? 1u : 0u), ncclUint32, c->peer[d], c->comm, s);
  }
  for (int d = 7; d >= 0 && res == ncclSuccess; --d) {
    if (!((c->neighbourMask >> d) & 1u)) continue;
    res = r->Recv(ds.borderRecv[d], (size_t)borderWords((uint32_t)d, c->desc.tile_sectors_x, c->desc.tile_sectors_z, c->borderRecs, c->halo ? 1u : 0u), ncclUint32, c->peer[d], c->comm, s);
  }
  const ncclResult_t end = r->GroupEnd();
  if (!ncclOk(c, r, res, "ncclSend/ncclRecv")) return 0;
  return ncclOk(c, r, end, "ncclGroupEnd") ? 1 : 0;
}

int scTickExchangeBorders(ScTickContext* c)
{
  if (!c) return 0;
  if (!bind(c)) return 0;
  if (!c->pairsPending) return fail(c, "scTickExchangeBorders without a preceding scTickRun(... | SC_TICK_BROADPHASE | SC_TICK_SPLIT_PAIRS)");
  if (!c->neighbourMask) return 1;
  if (!c->comm) return fail(c, "no communicator: scTickCommInit first");
  return exchangeBorders(c, c->pendingTick.p.parity, c->pairsStream ? c->pairsStream : c->stream, false);
}

int scTickTileStep(ScTickContext* c, uint32_t flags)
{
  if (!c) return 0;
  struct Own { ScTickContext* c; explicit Own(ScTickContext* c_) : c(c_) { c->ownStep = true; } ~Own() { c->ownStep = false; } } own(c);
  if (!(flags & SC_TICK_BROADPHASE) || !c->neighbourMask) {                                                                // nothing to exchange
    if (!(flags & SC_TICK_BROADPHASE) || !c->pairsStream) return scTickRun(c, flags & ~(uint32_t)SC_TICK_SPLIT_PAIRS);
    if (!scTickRun(c, flags | SC_TICK_SPLIT_PAIRS)) return 0;                 // a lone pipelined tile: the pair half still runs on its own stream
    return runPendingPairs(c, false);
  }
  if (!c->comm) return fail(c, "no communicator: scTickCommInit first (a tile with neighbours cannot skip the exchange)");
  if (c->graphMode && !c->pairsStream) {
    // in-order tile, graph replay: the whole step -- producer, fused kernel, compaction + pack, the RCCL group, merge, pair
    // search -- is captured once per tick parity and replayed with one hipGraphLaunch
    const double g0 = nowUs();
    c->captureWholeStep = true;
    const int okr = scTickRun(c, flags | SC_TICK_SPLIT_PAIRS);
    c->captureWholeStep = false;
    if (!okr) return 0;
    const int okp = c->pairsPending ? runPendingPairs(c, true) : 1;     // a sampled (profiled) tick ran eagerly: finish it the eager way
    c->hostAcc[0] += nowUs() - g0; c->hostSteps++;
    return okp;
  }
  // eager, or a pipelined tile: the tick on its stream, then exchange + pair half on theirs (with graph replay on, each
  // half of a pipelined step is one hipGraphLaunch; the events that order them are recorded between the two)
  const double t0 = nowUs();
  if (!scTickRun(c, flags | SC_TICK_SPLIT_PAIRS)) return 0;
  const double t1 = nowUs();
  const int ok = runPendingPairs(c, true);
  c->hostAcc[0] += t1 - t0; c->hostAcc[1] += nowUs() - t1; c->hostSteps++;
  return ok;
}

} // extern "C"
