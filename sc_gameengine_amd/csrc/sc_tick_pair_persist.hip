// Pair persistence (include/sc_tick.h "pair persistence"): which of this run's contact points is the same point as the last flagged run's.
// What Bullet's btPersistentManifold keeps behind src/engine/physics/sc_physics.cpp:218-225 -- a point's identity across ticks, so that a
// solver's accumulated impulses and a contact's age can ride on it -- formed on the device behind the manifold records, while the touching
// list's running count is still up.  A translation unit of its own, so that every other kernel keeps its instruction stream.
//
//   k_pair_persist_match    a thread per entry of the touching list: its manifold points in `a`'s frame; the pair enters the CURRENT side's
//                           table (64-bit compare-and-swap on the key, the smallest entry index kept by an atomic maximum of its complement);
//                           the pair is looked up in the REMEMBERED side; the points are matched greedily, in slot order, one to one; the
//                           record, this side's local points, ages and carried payload rows are written
//   k_pair_persist_sweep    a thread per slot of the remembered side's table: cleared, so that side is the next run's empty "current"
//   k_pair_persist_finish   one workgroup: the workgroups' tallies added up, the report (ScTickPairPersistInfo) and the side that was filled by
//                           its first lane, the validity word set, the side word flipped
//
// The side word and the validity word live on the device: every grid is fixed by capacities, every count is read here, so both parities of
// the tick replay unchanged from captured graphs.  Every probe loop is bounded by the slot count (the load factor is at most one half: a
// loop that runs out raises gave_up, it never spins).  Plain HIP atomics and vector stores only; no register array is indexed at run time.
#include "sc_tick_internal.h"
#include <algorithm>

namespace sctick {
namespace {

// the sum over a wave of a lane value in 0 .. 7, by one ballot per bit
__device__ __forceinline__ uint32_t waveSum3(uint32_t v)
{
  return (uint32_t)__popcll(ballot64((v & 1u) != 0u)) + 2u * (uint32_t)__popcll(ballot64((v & 2u) != 0u)) + 4u * (uint32_t)__popcll(ballot64((v & 4u) != 0u));
}

__global__ __launch_bounds__(kTile) void k_pair_persist_match(const DeviceState d, const PairShapeState e, const PairManifoldState f, const PairPersistState s,
                                                             uint32_t count, uint32_t rankBits)
{
  __shared__ uint32_t acc[kTile / 64u][4];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t listed = e.ctl[kPsTouching];
  uint32_t room = e.maxTouching < f.maxTouching ? e.maxTouching : f.maxTouching;      // (one number: every buffer follows the list)
  room = room < s.maxTouching ? room : s.maxTouching;
  const uint32_t n = listed < room ? listed : room;
  const uint32_t cur = s.ctl[kPpCur] & 1u;
  unsigned long long* curK = s.key[cur];
  uint32_t* curV = s.val[cur];
  const unsigned long long* prevK = s.key[cur ^ 1u];
  const uint32_t* prevV = s.val[cur ^ 1u];
  const float4* prevLocal = s.local[cur ^ 1u];
  const float4* prevPayload = s.payload[cur ^ 1u];
  float4* curLocal = s.local[cur];
  float4* curPayload = s.payload[cur];
  const uint32_t mask = s.slots - 1u;
  const float m2 = s.matchDist * s.matchDist;
  uint32_t keptPairs = 0u, keptPoints = 0u, newPoints = 0u;      // (wave-uniform)
  bool gaveUp = false;
  const uint32_t stride = gridDim.x * kTile;
  for (uint32_t base = blockIdx.x * kTile + (threadIdx.x & ~63u); base < n; base += stride) {      // (wave-uniform trip count)
    const uint32_t i = base + lane;
    bool kept = false;
    uint32_t nKept = 0u, nNew = 0u;
    if (i < n) {
      const uint2 pr = e.list[i];
      const float4* mrec = f.rec + 5u * (size_t)i;
      const float4 m0 = mrec[0], m1 = mrec[1], m2r = mrec[2], m4 = mrec[4];
      uint32_t cnt = __float_as_uint(m4.x);
      cnt = cnt < 4u ? cnt : 4u;
      // 1. the local points: `a`'s columns normalised as frameOf does, whatever its collider type.  (A record with points has an `a`
      //    that fetchMember accepted -- own rank, below the count; the test only keeps the loads in bounds whatever the record says.)
      const uint32_t ea = pr.x & 0x00FFFFFFu;
      if ((pr.x & 0xFF000000u) != rankBits || ea >= count) cnt = 0u;
      float x[4][3];
#pragma unroll
      for (int q = 0; q < 4; ++q) x[q][0] = x[q][1] = x[q][2] = 0.0f;
      if (cnt) {
        const float4 r0 = d.w0[ea], r1 = d.w1[ea], r2 = d.w2[ea];
        const float c[3][3] = { { r0.x, r1.x, r2.x }, { r0.y, r1.y, r2.y }, { r0.z, r1.z, r2.z } };
        const float T[3] = { r0.w, r1.w, r2.w };
        float u[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float q = sqrtf(dot3(c[k], c[k]));
#pragma unroll
          for (int j = 0; j < 3; ++j) u[k][j] = c[k][j] / q;
        }
        const float p[4][3] = { { m0.x, m0.y, m0.z }, { m0.w, m1.x, m1.y }, { m1.z, m1.w, m2r.x }, { m2r.y, m2r.z, m2r.w } };
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float r[3] = { p[q][0] - T[0], p[q][1] - T[1], p[q][2] - T[2] };
#pragma unroll
          for (int k = 0; k < 3; ++k) x[q][k] = ((uint32_t)q < cnt) ? dot3(r, u[k]) : 0.0f;
        }
      }
      // 2. the pair enters the current side: a pair named twice enters once, and the slot keeps the smallest entry index
      // 3. ... and is looked up in the remembered side (all zeros while nothing is remembered)
      const unsigned long long key = ((unsigned long long)pr.x << 32) | pr.y;
      uint32_t pe = kPersistNone;
      if (key != 0ull) {                                      // (no pair has a == b == 0; the key is the tables' "empty")
        const uint32_t home = pairHash(key) & mask;
        uint32_t pos = home;
        bool placed = false;
        for (uint32_t t = 0; t < s.slots; ++t) {
          unsigned long long v = __hip_atomic_load(&curK[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (v == 0ull) v = atomicCAS(&curK[pos], 0ull, key);
          if (v == 0ull || v == key) { atomicMax(&curV[pos], ~i); placed = true; break; }
          pos = (pos + 1u) & mask;
        }
        if (!placed) gaveUp = true;
        pos = home;
        bool ended = false;
        for (uint32_t t = 0; t < s.slots; ++t) {
          const unsigned long long v = prevK[pos];
          if (v == key) { pe = ~prevV[pos]; ended = true; break; }
          if (v == 0ull) { ended = true; break; }
          pos = (pos + 1u) & mask;
        }
        if (!ended) gaveUp = true;
        if (pe >= s.maxTouching) pe = kPersistNone;           // (a slot without a value cannot be: nothing is read out of bounds if it is)
      }
      kept = pe != kPersistNone;
      // 4. the points: greedy, in slot order, one to one; the first candidate is the best, a later one only when strictly nearer
      float y[4][3];
      uint32_t ageOld = 0u, cntOld = 0u;
#pragma unroll
      for (int q = 0; q < 4; ++q) y[q][0] = y[q][1] = y[q][2] = 0.0f;
      if (kept) {
        const float4* lrow = prevLocal + 4u * (size_t)pe;
        const float4 l0 = lrow[0], l1 = lrow[1], l2 = lrow[2], l3 = lrow[3];
        y[0][0] = l0.x; y[0][1] = l0.y; y[0][2] = l0.z; y[1][0] = l0.w; y[1][1] = l1.x; y[1][2] = l1.y;
        y[2][0] = l1.z; y[2][1] = l1.w; y[2][2] = l2.x; y[3][0] = l2.y; y[3][1] = l2.z; y[3][2] = l2.w;
        ageOld = __float_as_uint(l3.x);
        cntOld = __float_as_uint(l3.y);
        cntOld = cntOld < 4u ? cntOld : 4u;
      }
      uint32_t taken = 0u, slots = 0u, ages = 0u;
      float4* prow = curPayload + 4u * (size_t)i;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t best = 0xFFu;
        float bd = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float e0 = x[q][0] - y[t][0], e1 = x[q][1] - y[t][1], e2 = x[q][2] - y[t][2];
          const float dd = (e0 * e0 + e1 * e1) + e2 * e2;
          const bool open = (uint32_t)q < cnt && (uint32_t)t < cntOld && !((taken >> t) & 1u);
          const bool better = open && dd <= m2 && (best == 0xFFu || dd < bd);      // (a NaN distance is no candidate)
          best = better ? (uint32_t)t : best;
          bd = better ? dd : bd;
        }
        float4 row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        uint32_t age = 0u;
        if (best != 0xFFu) {
          taken |= 1u << best;
          const uint32_t was = (ageOld >> (8u * best)) & 0xFFu;
          age = was < 255u ? was + 1u : 255u;
          row = prevPayload[4u * (size_t)pe + best];
          ++nKept;
        } else if ((uint32_t)q < cnt) ++nNew;
        slots |= best << (8 * q);
        ages |= age << (8 * q);
        prow[q] = row;                                        // 6. the carried payload row, or four +0
      }
      // 5. the record, and 6. this side's local points and ages
      s.rec[i] = make_uint4(pe, slots, ages, 0u);
      float4* lrow = curLocal + 4u * (size_t)i;
      lrow[0] = make_float4(x[0][0], x[0][1], x[0][2], x[1][0]);
      lrow[1] = make_float4(x[1][1], x[1][2], x[2][0], x[2][1]);
      lrow[2] = make_float4(x[2][2], x[3][0], x[3][1], x[3][2]);
      lrow[3] = make_float4(__uint_as_float(ages), __uint_as_float(cnt), 0.0f, 0.0f);
    }
    keptPairs += (uint32_t)__popcll(ballot64(kept));
    keptPoints += waveSum3(nKept);
    newPoints += waveSum3(nNew);
  }
  const bool anyGaveUp = ballot64(gaveUp) != 0ull;
  if (lane == 0 && anyGaveUp) atomicOr(&s.ctl[kPpGaveUp], 1u);      // (never at load one half)
  // a workgroup's tallies go to words of its own, written on every launch; the finish adds them up: nothing is added to a shared word
  if (lane == 0) { acc[threadIdx.x >> 6][kPpKeptPairs] = keptPairs; acc[threadIdx.x >> 6][kPpKeptPoints] = keptPoints; acc[threadIdx.x >> 6][kPpNewPoints] = newPoints; }
  __syncthreads();
  if (threadIdx.x <= kPpNewPoints)
    s.partial[4u * blockIdx.x + threadIdx.x] = (acc[0][threadIdx.x] + acc[1][threadIdx.x]) + (acc[2][threadIdx.x] + acc[3][threadIdx.x]);
}

// a thread per slot of the remembered side's table: what the match kernel has just read is cleared, the side is the next run's "current"
__global__ __launch_bounds__(kTile) void k_pair_persist_sweep(const PairPersistState s)
{
  const uint32_t cur = s.ctl[kPpCur] & 1u;
  unsigned long long* prevK = s.key[cur ^ 1u];
  uint32_t* prevV = s.val[cur ^ 1u];
  const uint32_t stride = gridDim.x * kTile;
  for (uint32_t i = blockIdx.x * kTile + threadIdx.x; i < s.slots; i += stride) {
    if (prevK[i] != 0ull) prevK[i] = 0ull;
    if (prevV[i] != 0u) prevV[i] = 0u;
  }
}

// one workgroup: the tallies of the match kernel's `blocks` workgroups added up; its first lane writes the report, the side that was
// filled (what the payload calls copy to and from), and turns the sides over.  The list's running count and its truncation word are
// still up: k_pair_shapes_finish runs behind this.
__global__ __launch_bounds__(kTile) void k_pair_persist_finish(const PairShapeState e, const PairManifoldState f, const PairPersistState s, uint32_t blocks)
{
  __shared__ uint32_t acc[kTile / 64u][4];
  if (blockIdx.x != 0) return;
  const uint4* partial = reinterpret_cast<const uint4*>(s.partial);
  uint32_t sum0 = 0u, sum1 = 0u, sum2 = 0u;
#pragma unroll
  for (uint32_t r = 0; r < kPpMaxBlocks / kTile; ++r) {
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
  const uint32_t keptPairs = (acc[0][0] + acc[1][0]) + (acc[2][0] + acc[3][0]);
  const uint32_t keptPoints = (acc[0][1] + acc[1][1]) + (acc[2][1] + acc[3][1]);
  const uint32_t newPoints = (acc[0][2] + acc[1][2]) + (acc[2][2] + acc[3][2]);
  const uint32_t listed = e.ctl[kPsTouching];
  uint32_t room = e.maxTouching < f.maxTouching ? e.maxTouching : f.maxTouching;
  room = room < s.maxTouching ? room : s.maxTouching;
  const uint32_t n = listed < room ? listed : room;
  const uint32_t cur = s.ctl[kPpCur] & 1u;
  s.info[0] = n; s.info[1] = keptPairs; s.info[2] = n - keptPairs; s.info[3] = keptPoints; s.info[4] = newPoints;
  s.info[5] = s.ctl[kPpValid] ? 0u : 1u;
  s.info[6] = (listed > e.maxTouching || e.ctl[kPsPairsTruncated] != 0u) ? 1u : 0u;
  s.info[7] = s.ctl[kPpGaveUp];
  s.info[kPpInfoSide] = cur;
  s.ctl[kPpGaveUp] = 0u;
  s.ctl[kPpValid] = 1u;
  s.ctl[kPpCur] = cur ^ 1u;                                   // the side just filled is the remembered run, the swept one the next "current"
}

} // namespace

void launchPairPersist(const DeviceState& d, const TickParams& p, const PairShapeState& list, const PairManifoldState& manifolds, const PairPersistState& persist,
                       hipStream_t s)
{
  // the grids by capacities alone -- a thread per entry the list can hold, per slot of a table (grid-stride beyond the caps)
  const uint32_t blocks = std::min(std::max((persist.maxTouching + kTile - 1u) / kTile, 1u), kPpMaxBlocks);
  const uint32_t sweepBlocks = std::min(std::max(persist.slots / kTile, 1u), 2048u);
  hipLaunchKernelGGL(k_pair_persist_match, dim3(blocks), dim3(kTile), 0, s, d, list, manifolds, persist, p.n, p.rankBits);
  hipLaunchKernelGGL(k_pair_persist_sweep, dim3(sweepBlocks), dim3(kTile), 0, s, persist);
  hipLaunchKernelGGL(k_pair_persist_finish, dim3(1), dim3(kTile), 0, s, list, manifolds, persist, blocks);
}

} // namespace sctick
