// Pair islands (include/sc_tick.h "pair islands"): the connected components of the movable entities under the linking entries of this
// tick's touching list, by a lock-free union-find in the manner of ECL-CC (Jaiganesh & Burtscher, HPDC 2018): init, link, flatten, and a
// one-workgroup report.  A translation unit of its own, so that every other kernel keeps its instruction stream.
//
// The one invariant everything rests on: parent[x] <= x, always, and a word only ever decreases.  A hook writes the SMALLER root into the
// LARGER root's word, path halving replaces a parent by a grandparent.  So a walk from x towards its root descends strictly -- it ends
// after at most x steps whatever other lanes do meanwhile --, the root of a finished component is its smallest index, and the labels are a
// function of the edge set alone.  No lane ever waits for another: a compare-and-swap that loses has been overtaken by one that won.
#include "sc_tick_internal.h"
#include <algorithm>

namespace sctick {
namespace {

__device__ __forceinline__ uint32_t parentLoad(const uint32_t* parent, uint32_t x)
{ return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// movable (the header's definition): an own id below the count whose group has no fixed bit.  The dense index is only used behind the test.
__device__ __forceinline__ bool islandMovable(const DeviceState& d, uint32_t id, uint32_t count, uint32_t rankBits, uint32_t fixedGroups)
{
  const uint32_t e = id & 0x00FFFFFFu;
  if ((id & 0xFF000000u) != rankBits || e >= count) return false;
  return (d.layers[e] & 0xFFFFu & fixedGroups) == 0u;
}

// A workgroup's tallies go to words of its own (PairIslandState::partial, four per workgroup), written unconditionally on every launch;
// the report's one workgroup adds them up.  Nothing is added to a shared word: one word takes about 88 device-scope additions per microsecond
// on this chip, and a wave-per-counter atomic on the 8 192 waves of a million entities was measured at 105 us for an
// empty list and 310 us with three counters in one line -- the whole pass, for sums the report can take later.
__device__ __forceinline__ void islandBlockTally(uint32_t (*acc)[4], uint32_t k, uint32_t mine)
{
  if ((threadIdx.x & 63u) == 0u) acc[threadIdx.x >> 6][k] = mine;
}

// 1. a thread per entity below the count: its own root, or NONE when fixed; its label word starts as 0 = "no hook has landed on me"
__global__ __launch_bounds__(kTile) void k_pair_islands_init(const DeviceState d, const PairIslandState s, uint32_t count)
{
  const uint32_t n = count < s.cap ? count : s.cap;
  const uint32_t stride = gridDim.x * kTile;
  for (uint32_t e = blockIdx.x * kTile + threadIdx.x; e < n; e += stride) {
    s.parent[e] = (d.layers[e] & 0xFFFFu & s.fixedGroups) ? kIslandNone : e;
    s.labels[e] = 0u;
  }
}

// The root of x while other lanes hook and halve, with path halving.  Every access to the parent array inside the link kernel is an
// agent-scope atomic: a plain load may be answered by this XCD's L2 with what the word held before another XCD's lane changed it.
// Every step moves to a strictly smaller index (parent[x] < x unless x is a root), so `bound` = the entity count cannot be reached;
// a lane that does reach it -- a corrupted word -- raises `gaveUp` and returns where it stands.
__device__ __forceinline__ uint32_t islandFindHalving(uint32_t* parent, uint32_t x, uint32_t bound, bool& gaveUp)
{
  uint32_t p = parentLoad(parent, x);
  for (uint32_t step = 0; step < bound; ++step) {
    if (p >= x) return x;                                   // a root (p == x); p > x cannot be: stop rather than climb
    const uint32_t g = parentLoad(parent, p);
    if (g >= p) return p;
    // halve: x skips its parent.  x is not a root (p < x), so no hook touches its word; a minimum keeps the word decreasing when two
    // lanes halve the same x from different moments.  (Fire and forget: the result is not used.)
    __hip_atomic_fetch_min(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p; p = g;
  }
  gaveUp = true;
  return x;
}

// ... and once nobody writes the array any more (the flatten kernel): plain loads, no halving
__device__ __forceinline__ uint32_t islandFindSettled(const uint32_t* parent, uint32_t x, uint32_t bound, bool& gaveUp)
{
  for (uint32_t step = 0; step <= bound; ++step) {
    const uint32_t p = parent[x];
    if (p >= x) return x;
    x = p;
  }
  gaveUp = true;
  return x;
}

// 2. a thread per entry of the touching list (the grid by the list's capacity, the entry count read here: the launch replays from a
// captured graph).  A linking entry finds both roots and hooks the larger under the smaller with a compare-and-swap that expects the
// larger to be a root still.  A lost race answers with the word's new value, a smaller index of the same tree: the lane goes on from
// there.  The hook that succeeds leaves 1 in the label word of the root it hooked under: the first member that ever joins a tree can only
// have hooked under its root, so the root of every island of two or more ends up marked, and no single does.
__global__ __launch_bounds__(kTile) void k_pair_islands_link(const DeviceState d, const PairShapeState e, const PairIslandState s, uint32_t count,
                                                            uint32_t rankBits)
{
  __shared__ uint32_t acc[kTile / 64u][4];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t listed = e.ctl[kPsTouching];
  const uint32_t room = e.maxTouching < s.maxTouching ? e.maxTouching : s.maxTouching;
  const uint32_t n = listed < room ? listed : room;
  const uint32_t bound = count < s.cap ? count : s.cap;
  uint32_t linking = 0u;                                    // (wave-uniform)
  bool gaveUp = false;
  const uint32_t stride = gridDim.x * kTile;
  for (uint32_t base = blockIdx.x * kTile + (threadIdx.x & ~63u); base < n; base += stride) {      // (wave-uniform trip count)
    const uint32_t i = base + lane;
    bool links = false;
    if (i < n) {
      const uint2 pr = e.list[i];
      links = islandMovable(d, pr.x, bound, rankBits, s.fixedGroups) && islandMovable(d, pr.y, bound, rankBits, s.fixedGroups);
      if (links) {
        uint32_t ra = islandFindHalving(s.parent, pr.x & 0x00FFFFFFu, bound, gaveUp);
        uint32_t rb = islandFindHalving(s.parent, pr.y & 0x00FFFFFFu, bound, gaveUp);
        // The retries: a lost compare-and-swap means `hi` was hooked by another lane meanwhile, and both new starting points -- the value
        // it answered with (< hi) and lo (< hi) -- lie below hi, as do their roots.  So max(ra, rb) falls strictly from try to try and
        // `bound` = the entity count (at most SC_TICK_MAX_ENTITIES = 2^24 - 1) tries cannot all be lost; in practice it is one or two.
        bool done = false;
        for (uint32_t attempt = 0; attempt < bound; ++attempt) {
          if (ra == rb) { done = true; break; }
          const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
          uint32_t seen = hi;
          if (__hip_atomic_compare_exchange_strong(&s.parent[hi], &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
            __hip_atomic_store(&s.labels[lo], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            done = true;
            break;
          }
          if (seen >= hi) break;                            // cannot be (a word only decreases): give up rather than climb
          ra = islandFindHalving(s.parent, seen, bound, gaveUp);
          rb = islandFindHalving(s.parent, lo, bound, gaveUp);
        }
        if (!done) gaveUp = true;
      }
    }
    linking += (uint32_t)__popcll(ballot64(links));
  }
  const bool anyGaveUp = ballot64(gaveUp) != 0ull;
  if (lane == 0 && anyGaveUp) atomicOr(&s.ctl[kPiGaveUp], 1u);      // (never, unless a word is corrupted)
  islandBlockTally(acc, kPiLinking, linking);
  __syncthreads();
  if (threadIdx.x == 0) s.partial[4u * blockIdx.x + kPiLinking] = (acc[0][kPiLinking] + acc[1][kPiLinking]) + (acc[2][kPiLinking] + acc[3][kPiLinking]);
}

// 3. the array is settled: a thread per entity writes its label, a thread per entry its edge island, and the report's counts are taken
// by ballot, per wave, then per workgroup (islandBlockTally).  An island is counted at its root, a body wherever it is not a single: nothing
// is ever added to a word that belongs to an island.
__global__ __launch_bounds__(kTile) void k_pair_islands_flatten(const DeviceState d, const PairShapeState e, const PairIslandState s, uint32_t count,
                                                               uint32_t rankBits)
{
  __shared__ uint32_t acc[kTile / 64u][4];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t listed = e.ctl[kPsTouching];
  const uint32_t room = e.maxTouching < s.maxTouching ? e.maxTouching : s.maxTouching;
  const uint32_t n = listed < room ? listed : room;
  const uint32_t bound = count < s.cap ? count : s.cap;
  const uint32_t both = n > bound ? n : bound;
  uint32_t movable = 0u, islands = 0u, bodies = 0u;        // (wave-uniform)
  bool gaveUp = false;
  const uint32_t stride = gridDim.x * kTile;
  for (uint32_t base = blockIdx.x * kTile + (threadIdx.x & ~63u); base < both; base += stride) {      // (wave-uniform trip count)
    const uint32_t i = base + lane;
    bool isMovable = false, isRoot = false, isBody = false;
    if (i < bound) {
      const uint32_t p = s.parent[i];
      uint32_t label = kIslandNone;
      if (p != kIslandNone) {
        isMovable = true;
        const uint32_t root = islandFindSettled(s.parent, i, bound, gaveUp);
        const bool marked = s.labels[i] != 0u;              // (this lane's own word: the one lane that reads it then writes it)
        isRoot = root == i && marked;
        isBody = root != i || marked;
        label = rankBits | root;
      }
      s.labels[i] = label;
    }
    if (i < n) {
      const uint2 pr = e.list[i];
      uint32_t island = kIslandNone;
      if (islandMovable(d, pr.x, bound, rankBits, s.fixedGroups)) island = rankBits | islandFindSettled(s.parent, pr.x & 0x00FFFFFFu, bound, gaveUp);
      else if (islandMovable(d, pr.y, bound, rankBits, s.fixedGroups)) island = rankBits | islandFindSettled(s.parent, pr.y & 0x00FFFFFFu, bound, gaveUp);
      s.edge[i] = island;
    }
    movable += (uint32_t)__popcll(ballot64(isMovable));
    islands += (uint32_t)__popcll(ballot64(isRoot));
    bodies += (uint32_t)__popcll(ballot64(isBody));
  }
  const bool anyGaveUp = ballot64(gaveUp) != 0ull;
  if (lane == 0 && anyGaveUp) atomicOr(&s.ctl[kPiGaveUp], 1u);
  islandBlockTally(acc, kPiMovable, movable); islandBlockTally(acc, kPiIslands, islands); islandBlockTally(acc, kPiBodies, bodies);
  __syncthreads();
  if (threadIdx.x >= kPiIslands && threadIdx.x <= kPiMovable)      // (the three words behind kPiLinking, which the link kernel's workgroups write)
    s.partial[4u * blockIdx.x + threadIdx.x] = (acc[0][threadIdx.x] + acc[1][threadIdx.x]) + (acc[2][threadIdx.x] + acc[3][threadIdx.x]);
}

// 4. one workgroup: the workgroups' tallies added up (the link kernel's `linkBlocks` first words, the flatten kernel's `flatBlocks` other
// three), then the tick's report (ScTickPairIslandInfo) by its first lane.  The list's running count and its truncation word are still
// up: k_pair_shapes_finish runs behind this.
__global__ __launch_bounds__(kTile) void k_pair_islands_finish(const PairShapeState e, const PairIslandState s, uint32_t linkBlocks, uint32_t flatBlocks)
{
  __shared__ uint32_t acc[kTile / 64u][4];
  if (blockIdx.x != 0) return;
  // (a workgroup, not a wave: a lane's loads are issued together, eight at most -- one wave walking 2 048 slots took 10.6 us, its 32
  //  loads one behind the other)
  const uint4* partial = reinterpret_cast<const uint4*>(s.partial);
  uint32_t sum[4] = { 0u, 0u, 0u, 0u };
#pragma unroll
  for (uint32_t r = 0; r < kPiMaxBlocks / kTile; ++r) {
    const uint32_t b = r * kTile + threadIdx.x;
    const uint4 v = b < flatBlocks ? partial[b] : make_uint4(0u, 0u, 0u, 0u);
    sum[kPiLinking] += b < linkBlocks ? v.x : 0u;
    sum[kPiIslands] += v.y; sum[kPiBodies] += v.z; sum[kPiMovable] += v.w;
  }
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
#pragma unroll
    for (uint32_t off = 32u; off; off >>= 1) sum[k] += __shfl_down(sum[k], off, 64);
    islandBlockTally(acc, k, sum[k]);
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) sum[k] = (acc[0][k] + acc[1][k]) + (acc[2][k] + acc[3][k]);
  const uint32_t listed = e.ctl[kPsTouching];
  const uint32_t room = e.maxTouching < s.maxTouching ? e.maxTouching : s.maxTouching;
  const uint32_t n = listed < room ? listed : room;
  s.info[0] = n; s.info[1] = sum[kPiLinking]; s.info[2] = n - sum[kPiLinking];
  s.info[3] = sum[kPiIslands]; s.info[4] = sum[kPiBodies]; s.info[5] = sum[kPiMovable];
  s.info[6] = (listed > e.maxTouching || e.ctl[kPsPairsTruncated] != 0u) ? 1u : 0u;
  s.info[7] = s.ctl[kPiGaveUp];
  s.ctl[kPiGaveUp] = 0u;
}

} // namespace

void launchPairIslands(const DeviceState& d, const TickParams& p, const PairShapeState& list, const PairIslandState& islands, hipStream_t s)
{
  // the grids by capacities alone -- a thread per entity the context can hold, per entry the list can hold (grid-stride beyond the cap);
  // the counts are read on the device
  const uint32_t eblocks = std::min(std::max((islands.cap + kTile - 1u) / kTile, 1u), kPiMaxBlocks);
  const uint32_t lblocks = std::min(std::max((list.maxTouching + kTile - 1u) / kTile, 1u), kPiMaxBlocks);
  hipLaunchKernelGGL(k_pair_islands_init, dim3(eblocks), dim3(kTile), 0, s, d, islands, p.n);
  hipLaunchKernelGGL(k_pair_islands_link, dim3(lblocks), dim3(kTile), 0, s, d, list, islands, p.n, p.rankBits);
  const uint32_t fblocks = std::max(eblocks, lblocks);      // (<= kPiMaxBlocks: the workgroups' tallies have a slot each)
  hipLaunchKernelGGL(k_pair_islands_flatten, dim3(fblocks), dim3(kTile), 0, s, d, list, islands, p.n, p.rankBits);
  hipLaunchKernelGGL(k_pair_islands_finish, dim3(1), dim3(kTile), 0, s, list, islands, lblocks, fblocks);
}

} // namespace sctick
