// Pair sleep (include/sc_tick.h "pair sleep"): which islands are at rest, which bodies just fell asleep and which were just woken.  What
// Bullet's island pipeline does with its deactivation timers behind PhysicsWorld::isBodyActive / activateBody (sc_physics.h:167-168), formed
// on the device behind the island pass -- labels and edge islands are final -- while the touching list's running count is still up.  The
// library has no velocities: a body is STILL while its world rows stay within a tolerance of an anchor pose, and the anchor follows it when
// they do not.  A translation unit of its own, so that every other kernel keeps its instruction stream.
//
//   k_pair_sleep_motion    a thread per entity: rows against anchor, the new rest count; a movable entity that has not rested long enough
//                          marks its island awake
//   k_pair_sleep_edges     a thread per entry: an anchored entry whose fixed member is an own entity that moved marks the island awake
//   k_pair_sleep_resolve   a thread per entity and per entry: asleep or not, the state word, the two event lists, the tallies
//   k_pair_sleep_finish    one workgroup: the tallies added up, the report, the event counts back to zero, the epoch moved on
//
// "Awake" is a word per island root that holds the run's epoch: every writer of a word writes the same value, so there is no atomic
// read-modify-write and no clearing pass; a word that holds anything else means "not awake in this run".  The epoch and the validity word
// live on the device, every grid is fixed by capacities and every count is read here, so both parities of the tick replay unchanged from
// captured graphs.  Plain HIP atomics and vector stores only.
#include "sc_tick_internal.h"
#include <algorithm>

namespace sctick {
namespace {

// movable (the islands' definition): an own id below the count whose group has no fixed bit.  The dense index is only used behind the test.
__device__ __forceinline__ bool sleepMovable(const DeviceState& d, uint32_t id, uint32_t count, uint32_t rankBits, uint32_t fixedGroups)
{
  const uint32_t e = id & 0x00FFFFFFu;
  if ((id & 0xFF000000u) != rankBits || e >= count) return false;
  return (d.layers[e] & 0xFFFFu & fixedGroups) == 0u;
}

// |w - a| <= tol on the three rotation elements of a row and on its translation: plain fp32, a NaN anywhere fails
__device__ __forceinline__ bool rowStill(const float4 w, const float4 a, float linTol, float angTol)
{
  return fabsf(w.x - a.x) <= angTol && fabsf(w.y - a.y) <= angTol && fabsf(w.z - a.z) <= angTol && fabsf(w.w - a.w) <= linTol;
}

__device__ __forceinline__ void markAwake(const PairSleepState& s, uint32_t island, uint32_t epoch)
{
  const uint32_t r = island & 0x00FFFFFFu;
  if (r < s.cap) __hip_atomic_store(&s.awake[r], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the entries this run answers: the first min(touching, every buffer's room) of the list
__device__ __forceinline__ uint32_t sleepListed(const PairShapeState& e, const PairIslandState& isl, const PairSleepState& s)
{
  const uint32_t listed = e.ctl[kPsTouching];
  uint32_t room = e.maxTouching < isl.maxTouching ? e.maxTouching : isl.maxTouching;
  room = room < s.maxTouching ? room : s.maxTouching;
  return listed < room ? listed : room;
}

// 1. a thread per entity below the count.  Three 16-byte loads of the rows and three of the anchor; the anchor is stored only where the
// entity moved, the state word only where it changed: a world at rest with saturated counts writes nothing.  While nothing is remembered
// (the validity word is 0: a resync) every entity counts as moved.
__global__ __launch_bounds__(kTile) void k_pair_sleep_motion(const DeviceState d, const PairIslandState isl, const PairSleepState s, uint32_t count)
{
  uint32_t n = count < s.cap ? count : s.cap;
  n = n < isl.cap ? n : isl.cap;
  const uint32_t epoch = s.ctl[kPzEpoch] + 1u;
  const bool valid = s.ctl[kPzValid] != 0u;
  const uint32_t stride = gridDim.x * kTile;
  for (uint32_t e = blockIdx.x * kTile + threadIdx.x; e < n; e += stride) {
    const float4 r0 = d.w0[e], r1 = d.w1[e], r2 = d.w2[e];
    float4* anchor = s.anchor + 3u * (size_t)e;
    const float4 a0 = anchor[0], a1 = anchor[1], a2 = anchor[2];
    const bool still = valid && rowStill(r0, a0, s.linTol, s.angTol) && rowStill(r1, a1, s.linTol, s.angTol) && rowStill(r2, a2, s.linTol, s.angTol);
    const uint32_t old = s.state[e];
    const uint32_t was = old & 0xFFu;
    const uint32_t rest = still ? (was < 255u ? was + 1u : 255u) : 0u;
    if (!still) { anchor[0] = r0; anchor[1] = r1; anchor[2] = r2; }
    const uint32_t label = isl.labels[e];
    const bool movable = label != kIslandNone;
    // (the ASLEEP bit stays the last run's until the resolve has compared it)
    const uint32_t word = (old & kSleepAsleep) | rest | (still ? kSleepStill : 0u) | (movable ? kSleepMovable : 0u);
    if (word != old) s.state[e] = word;
    if (movable && rest < s.restRuns) markAwake(s, label, epoch);
  }
}

// 2. a thread per entry of the touching list: an anchored entry -- one member movable, the other not -- whose other member is an own
// entity below the count (then it is a fixed one) with rest == 0 in this run wakes the movable member's island: a kinematic platform
// under a stack.  A launch of its own behind the motion pass, whose rest counts it reads.
__global__ __launch_bounds__(kTile) void k_pair_sleep_edges(const DeviceState d, const PairShapeState e, const PairIslandState isl, const PairSleepState s,
                                                           uint32_t count, uint32_t rankBits)
{
  const uint32_t n = sleepListed(e, isl, s);
  uint32_t bound = count < s.cap ? count : s.cap;
  bound = bound < isl.cap ? bound : isl.cap;
  const uint32_t epoch = s.ctl[kPzEpoch] + 1u;
  const uint32_t stride = gridDim.x * kTile;
  for (uint32_t i = blockIdx.x * kTile + threadIdx.x; i < n; i += stride) {
    const uint32_t island = isl.edge[i];
    if (island == kIslandNone) continue;
    const uint2 pr = e.list[i];
    const bool xm = sleepMovable(d, pr.x, bound, rankBits, isl.fixedGroups), ym = sleepMovable(d, pr.y, bound, rankBits, isl.fixedGroups);
    if (xm == ym) continue;                                 // (a linking entry: both members are in the island already)
    const uint32_t f = xm ? pr.y : pr.x;
    const uint32_t fe = f & 0x00FFFFFFu;
    if ((f & 0xFF000000u) != rankBits || fe >= bound) continue;      // (a neighbour's member counts as still)
    if ((s.state[fe] & 0xFFu) == 0u) markAwake(s, island, epoch);
  }
}

// one slot reservation per list and wave that has events; which ids a short list holds is whichever waves came first
__device__ __forceinline__ void appendEvents(bool mine, uint32_t id, uint32_t* counter, uint32_t* list, uint32_t room)
{
  const unsigned long long m = ballot64(mine);
  if (m == 0ull) return;                                    // (wave-uniform)
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0u;
  if (lane == (uint32_t)__ffsll((long long)m) - 1u) base = atomicAdd(counter, (uint32_t)__popcll(m));
  base = (uint32_t)__shfl((int)base, __ffsll((long long)m) - 1, 64);
  const uint32_t slot = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (mine && slot < room) list[slot] = id;
}

// 3. the awake words are settled: a thread per entity forms asleep, compares it with the bit the last flagged run left and writes the state
// word where it changed; a thread per entry counts the entries of awake islands.  Tallies go to a slot per workgroup.
__global__ __launch_bounds__(kTile) void k_pair_sleep_resolve(const PairShapeState e, const PairIslandState isl, const PairSleepState s, uint32_t count,
                                                             uint32_t rankBits)
{
  __shared__ uint32_t acc[kTile / 64u][4];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t n = sleepListed(e, isl, s);
  uint32_t bound = count < s.cap ? count : s.cap;
  bound = bound < isl.cap ? bound : isl.cap;
  const uint32_t both = n > bound ? n : bound;
  const uint32_t epoch = s.ctl[kPzEpoch] + 1u;
  uint32_t asleepCount = 0u, rootsAsleep = 0u, awakeEntries = 0u;      // (wave-uniform)
  const uint32_t stride = gridDim.x * kTile;
  for (uint32_t base = blockIdx.x * kTile + (threadIdx.x & ~63u); base < both; base += stride) {      // (wave-uniform trip count)
    const uint32_t i = base + lane;
    bool asleep = false, root = false, fell = false, woke = false, entryAwake = false;
    if (i < bound) {
      const uint32_t word = s.state[i];
      const uint32_t label = isl.labels[i];
      const uint32_t r = label & 0x00FFFFFFu;
      asleep = label != kIslandNone && r < s.cap && s.awake[r] != epoch;
      root = asleep && r == i;
      const bool was = (word & kSleepAsleep) != 0u;
      fell = asleep && !was; woke = !asleep && was;
      if (asleep != was) s.state[i] = (word & ~kSleepAsleep) | (asleep ? kSleepAsleep : 0u);
    }
    if (i < n) {
      const uint32_t island = isl.edge[i];
      const uint32_t r = island & 0x00FFFFFFu;
      entryAwake = island != kIslandNone && r < s.cap && s.awake[r] == epoch;
    }
    asleepCount += (uint32_t)__popcll(ballot64(asleep));
    rootsAsleep += (uint32_t)__popcll(ballot64(root));
    awakeEntries += (uint32_t)__popcll(ballot64(entryAwake));
    appendEvents(fell, rankBits | i, &s.ctl[kPzFell], s.fell, s.maxEvents);
    appendEvents(woke, rankBits | i, &s.ctl[kPzWoke], s.woke, s.maxEvents);
  }
  if (lane == 0) { acc[threadIdx.x >> 6][kPzAsleep] = asleepCount; acc[threadIdx.x >> 6][kPzIslandsAsleep] = rootsAsleep; acc[threadIdx.x >> 6][kPzAwakeEntries] = awakeEntries; }
  __syncthreads();
  if (threadIdx.x <= kPzAwakeEntries)
    s.partial[4u * blockIdx.x + threadIdx.x] = (acc[0][threadIdx.x] + acc[1][threadIdx.x]) + (acc[2][threadIdx.x] + acc[3][threadIdx.x]);
}

// 4. one workgroup: the tallies of the resolve's `blocks` workgroups added up; its first lane writes the report, zeroes the event counts
// and moves the epoch on.  The list's running count is still up (k_pair_shapes_finish runs behind this); the islands' report is written.
__global__ __launch_bounds__(kTile) void k_pair_sleep_finish(const PairIslandState isl, const PairSleepState s, uint32_t blocks)
{
  __shared__ uint32_t acc[kTile / 64u][4];
  if (blockIdx.x != 0) return;
  const uint4* partial = reinterpret_cast<const uint4*>(s.partial);
  uint32_t sum0 = 0u, sum1 = 0u, sum2 = 0u;
#pragma unroll
  for (uint32_t r = 0; r < kPzMaxBlocks / kTile; ++r) {
    const uint32_t b = r * kTile + threadIdx.x;
    const uint4 v = b < blocks ? partial[b] : make_uint4(0u, 0u, 0u, 0u);
    sum0 += v.x; sum1 += v.y; sum2 += v.z;
  }
#pragma unroll
  for (uint32_t off = 32u; off; off >>= 1) {
    sum0 += __shfl_down(sum0, off, 64); sum1 += __shfl_down(sum1, off, 64); sum2 += __shfl_down(sum2, off, 64);
  }
  if ((threadIdx.x & 63u) == 0u) { acc[threadIdx.x >> 6][0] = sum0; acc[threadIdx.x >> 6][1] = sum1; acc[threadIdx.x >> 6][2] = sum2; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint32_t epoch = s.ctl[kPzEpoch] + 1u;
  const uint32_t fell = s.ctl[kPzFell], woke = s.ctl[kPzWoke];
  s.info[0] = (s.ctl[kPzValid] ? 0u : kSleepResync) | (fell > s.maxEvents ? kSleepFellOverflow : 0u) | (woke > s.maxEvents ? kSleepWokeOverflow : 0u) |
              (isl.info[6] ? kSleepListTruncated : 0u);
  s.info[1] = (acc[0][0] + acc[1][0]) + (acc[2][0] + acc[3][0]);
  s.info[2] = (acc[0][1] + acc[1][1]) + (acc[2][1] + acc[3][1]);
  s.info[3] = fell; s.info[4] = woke;
  s.info[5] = (acc[0][2] + acc[1][2]) + (acc[2][2] + acc[3][2]);
  s.info[6] = epoch; s.info[7] = 0u;
  s.ctl[kPzFell] = 0u; s.ctl[kPzWoke] = 0u;
  s.ctl[kPzValid] = 1u;
  s.ctl[kPzEpoch] = epoch;
}

// scTickWakeEntities: rest = 0 and the anchor unset (NaN rows: the next flagged run sees the entity moved) for n dense indices the host
// has checked against the count
__global__ __launch_bounds__(kTile) void k_pair_sleep_wake(const PairSleepState s, const uint32_t* ids, uint32_t n)
{
  const uint32_t i = blockIdx.x * kTile + threadIdx.x;
  if (i >= n) return;
  const uint32_t e = ids[i];
  if (e >= s.cap) return;
  const uint32_t word = s.state[e];
  if (word & 0xFFu) s.state[e] = word & ~0xFFu;             // (ids named twice store the same value)
  const float q = __uint_as_float(0x7FC00000u);
  float4* anchor = s.anchor + 3u * (size_t)e;
  anchor[0] = make_float4(q, q, q, q); anchor[1] = make_float4(q, q, q, q); anchor[2] = make_float4(q, q, q, q);
}

} // namespace

void launchPairSleep(const DeviceState& d, const TickParams& p, const PairShapeState& list, const PairIslandState& islands, const PairSleepState& sleep,
                     hipStream_t s)
{
  // the grids by capacities alone -- a thread per entity the context can hold, per entry the list can hold (grid-stride beyond the cap);
  // the counts are read on the device
  const uint32_t eblocks = std::min(std::max((sleep.cap + kTile - 1u) / kTile, 1u), kPzMaxBlocks);
  const uint32_t lblocks = std::min(std::max((list.maxTouching + kTile - 1u) / kTile, 1u), kPzMaxBlocks);
  const uint32_t rblocks = std::max(eblocks, lblocks);      // (<= kPzMaxBlocks: the workgroups' tallies have a slot each)
  hipLaunchKernelGGL(k_pair_sleep_motion, dim3(eblocks), dim3(kTile), 0, s, d, islands, sleep, p.n);
  hipLaunchKernelGGL(k_pair_sleep_edges, dim3(lblocks), dim3(kTile), 0, s, d, list, islands, sleep, p.n, p.rankBits);
  hipLaunchKernelGGL(k_pair_sleep_resolve, dim3(rblocks), dim3(kTile), 0, s, list, islands, sleep, p.n, p.rankBits);
  hipLaunchKernelGGL(k_pair_sleep_finish, dim3(1), dim3(kTile), 0, s, islands, sleep, rblocks);
}

void launchPairSleepWake(const PairSleepState& sleep, const uint32_t* ids, uint32_t n, hipStream_t s)
{
  if (!n) return;
  hipLaunchKernelGGL(k_pair_sleep_wake, dim3((n + kTile - 1u) / kTile), dim3(kTile), 0, s, sleep, ids, n);
}

} // namespace sctick
