// sc_tick_pair_events.hip -- pair begin / end events: the tick-to-tick difference of the broadphase pair set (own spec).
//
// What Bullet's overlapping-pair cache hands its narrow phase (btOverlappingPairCache::addOverlappingPair / removeOverlappingPair behind
// src/engine/physics/sc_physics.cpp:218-225): which pairs are new this tick and which are gone.  Three launches behind the pair search, on
// its stream, no host round trip; every grid is fixed by capacities, every count is read on the device, so the launches replay unchanged
// from a captured graph.
//
//   k_pair_events_diff    a thread per pair of this tick, read in place from the shard segments: the pair enters the CURRENT table
//                         (64-bit compare-and-swap; a pair met twice enters once); a pair that entered is looked up in the PREVIOUS table --
//                         found: its slot is marked, not found: the pair has begun
//   k_pair_events_sweep   a thread per slot of the previous table: an occupied slot without a mark is a pair that has ended; every slot and
//                         mark is cleared, so the table is the next tick's empty "current"
//   k_pair_events_finish  one thread: the tick's report (ScTickPairEventInfo), the running counts back to zero, the tables swap roles
//
// A tick whose set does not fit (more pairs than max_tracked_pairs, or a truncated pair list) is an OVERFLOW tick: every workgroup of the
// first kernel finds that out from the counters before anything is inserted, nothing is listed, the sweep empties BOTH tables, and the
// next tick that fits finds nothing remembered -- a resync tick: every pair begins.  Every probe loop is bounded by the slot count; one
// that runs out (it cannot while the set fits: the load factor is at most one half) raises the same overflow word, it never spins.
// Plain HIP atomics and vector stores only.
#include "sc_tick_internal.h"

namespace sctick {

namespace {

// One wave appends the pairs of its lanes with `yes` to a list of `cap` entries whose running count is *counter: one atomic per wave,
// the count is the true total, entries beyond the capacity are not written.  Every lane of the wave must call.
__device__ __forceinline__ void appendWave(bool yes, uint2 pr, uint32_t* counter, uint2* list, uint32_t cap)
{
  const unsigned long long m = ballot64(yes);
  if (!m) return;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(counter, (uint32_t)__popcll(m));
  base = __shfl(base, 0, 64);
  const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
  if (yes && at < cap) list[at] = pr;
}

__global__ __launch_bounds__(kTile) void k_pair_events_diff(const DeviceState d, const PairEventState e, uint32_t parity, uint32_t maxPairs)
{
  static_assert(kPairShards == 64, "one lane per shard counter");
  __shared__ uint32_t prefix[kPairShards + 1];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t shardCap = maxPairs / kPairShards;
  if (threadIdx.x < 64u) {
    // pairs per shard segment, clamped to the segment as k_gather_pairs does, and their running sum
    const uint32_t c = d.pairShardCount[(parity * kPairShards + lane) * kShardStride];
    uint32_t s = c < shardCap ? c : shardCap;
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
      const uint32_t o = __shfl_up(s, off, 64);
      if (lane >= off) s += o;
    }
    prefix[lane + 1u] = s;
    if (lane == 0) prefix[0] = 0u;
  }
  __syncthreads();
  const uint32_t total = prefix[kPairShards];
  const uint32_t dropped = d.counters[kCtrPar + 8u * parity + kCtrPairs];      // pairs found after every segment was full: the list is truncated
  if (dropped != 0u || total > e.maxTracked) {                                 // the same answer in every workgroup: nothing is inserted anywhere
    if (blockIdx.x == 0 && threadIdx.x == 0) e.ctl[kPeOverflow] = 1u;
    return;
  }
  const uint32_t cur = e.ctl[kPeCur] & 1u;
  unsigned long long* curT = e.table[cur];
  const unsigned long long* prevT = e.table[cur ^ 1u];
  uint32_t* prevM = e.marks[cur ^ 1u];
  const uint32_t mask = e.slots - 1u;
  const uint32_t stride = gridDim.x * kTile;
  for (uint32_t base = blockIdx.x * kTile + (threadIdx.x & ~63u); base < total; base += stride) {      // (wave-uniform trip count)
    const uint32_t i = base + lane;
    bool inserted = false, found = false;
    uint2 pr = make_uint2(0u, 0u);
    if (i < total) {
      uint32_t s = 0;                                         // the segment pair i lies in: the last one that starts at or before i
#pragma unroll
      for (uint32_t step = 32u; step; step >>= 1) if (prefix[s + step] <= i) s += step;
      pr = d.pairs[(size_t)s * shardCap + (i - prefix[s])];
      const unsigned long long key = ((unsigned long long)pr.x << 32) | pr.y;
      // (no pair has a == b == 0; the key is the tables' "empty")
      if (key != 0ull) pairSetEnter(e, curT, prevT, prevM, mask, key, inserted, found);
    }
    const unsigned long long mt = ballot64(inserted);
    if (mt && lane == 0) atomicAdd(&e.ctl[kPeTracked], (uint32_t)__popcll(mt));
    appendWave(inserted && !found, pr, &e.ctl[kPeBegun], e.begun, e.maxEvents);
  }
}

__global__ __launch_bounds__(kTile) void k_pair_events_sweep(const PairEventState e)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t cur = e.ctl[kPeCur] & 1u;
  const bool overflow = e.ctl[kPeOverflow] != 0u;
  unsigned long long* prevT = e.table[cur ^ 1u];
  uint32_t* prevM = e.marks[cur ^ 1u];
  const uint32_t stride = gridDim.x * kTile;
  // (slots is a multiple of 64: a wave covers two whole mark words; the lane that owns a word -- lane 0, lane 32 -- is the only one that
  //  touches it: it reads it once, hands it to its 32 lanes by a shuffle, and clears it)
  for (uint32_t base = blockIdx.x * kTile + (threadIdx.x & ~63u); base < e.slots; base += stride) {
    const uint32_t i = base + lane;
    const unsigned long long v = prevT[i];
    uint32_t w = 0u;
    if ((i & 31u) == 0u) w = prevM[i >> 5];
    w = __shfl(w, (int)(lane & 32u), 64);
    const bool gone = !overflow && v != 0ull && !((w >> (i & 31u)) & 1u);
    if (v != 0ull) prevT[i] = 0ull;
    if ((i & 31u) == 0u && w != 0u) prevM[i >> 5] = 0u;
    if (overflow) {                                           // drop everything: what the first kernel may have entered goes too
      if (e.table[cur][i] != 0ull) e.table[cur][i] = 0ull;
      if ((i & 31u) == 0u) e.marks[cur][i >> 5] = 0u;
    }
    appendWave(gone, make_uint2((uint32_t)(v >> 32), (uint32_t)v), &e.ctl[kPeEnded], e.ended, e.maxEvents);
  }
}

__global__ __launch_bounds__(64) void k_pair_events_finish(const PairEventState e)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t begun = e.ctl[kPeBegun], ended = e.ctl[kPeEnded], tracked = e.ctl[kPeTracked];
  const uint32_t valid = e.ctl[kPeValid], overflow = e.ctl[kPeOverflow];
  if (overflow) {
    e.info[0] = 0u; e.info[1] = 0u; e.info[2] = 0u; e.info[3] = 0u; e.info[4] = 1u; e.info[5] = 0u;
    e.ctl[kPeValid] = 0u;                                     // both tables are empty: nothing is remembered
  } else {
    e.info[0] = begun; e.info[1] = ended; e.info[2] = tracked; e.info[3] = valid ? 0u : 1u; e.info[4] = 0u;
    e.info[5] = (begun > e.maxEvents || ended > e.maxEvents) ? 1u : 0u;
    e.ctl[kPeValid] = 1u;
    e.ctl[kPeCur] = (e.ctl[kPeCur] & 1u) ^ 1u;                // the table just filled is the remembered set, the swept one the next "current"
  }
  e.ctl[kPeBegun] = 0u; e.ctl[kPeEnded] = 0u; e.ctl[kPeTracked] = 0u; e.ctl[kPeOverflow] = 0u;
}

} // namespace

void launchPairEventsTail(const PairEventState& e, hipStream_t s)
{
  if (!e.ctl) return;
  const uint32_t sweepBlocks = std::min(std::max(e.slots / kTile, 1u), 2048u);      // a thread per slot
  hipLaunchKernelGGL(k_pair_events_sweep, dim3(sweepBlocks), dim3(kTile), 0, s, e);
  hipLaunchKernelGGL(k_pair_events_finish, dim3(1), dim3(64), 0, s, e);
}

void launchPairEvents(const DeviceState& d, const TickParams& p, const PairEventState& e, hipStream_t s)
{
  if (!e.ctl) return;
  // grids by capacities alone: a thread per pair the tables can take (grid-stride beyond that), a thread per slot
  const uint32_t most = std::min(p.maxPairs, e.maxTracked);
  const uint32_t diffBlocks = std::min(std::max((most + kTile - 1u) / kTile, 1u), 2048u);
  hipLaunchKernelGGL(k_pair_events_diff, dim3(diffBlocks), dim3(kTile), 0, s, d, e, p.parity, p.maxPairs);
  launchPairEventsTail(e, s);
}

} // namespace sctick
