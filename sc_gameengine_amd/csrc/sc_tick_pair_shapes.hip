// sc_tick_pair_shapes.hip -- touching pairs: the pairs of this tick's list whose collider shapes overlap (own spec, include/sc_tick.h
// "touching pairs").
//
// What Bullet's narrow phase answers behind src/engine/physics/sc_physics.cpp:218-225, as a boolean: the pair search reports pairs of
// world AABBs, this pass drops those whose shapes -- oriented box, sphere, capsule, through the members' world matrices of this tick --
// are provably apart.  Two launches behind the pair search, on its stream, no host round trip; the grids are fixed by capacities and every
// count is read on the device, so the launches replay unchanged from a captured graph.
//
//   k_pair_shapes<List, Events>
//                          a thread per pair of this tick, read in place from the shard segments as k_pair_events_diff reads them: both
//                          members' collider records and matrix rows, one of three routines (segment-segment distance, segment-box
//                          distance, 15-axis separating-axis test), one append per wave to the touching list
//   k_pair_shapes_finish   one thread: the tick's report (ScTickPairShapeInfo), the running counts back to zero
//   k_pair_contacts        opt-in (scTickSetPairContacts), between the two: a thread per entry of the touching list, one record each --
//                          point, depth, normal, kind (include/sc_tick.h "pair contacts"); k_pair_contacts_finish: its report
//   k_pair_manifolds       opt-in (scTickSetPairManifolds), behind the contacts: a thread per entry again, up to four points and depths
//                          each (include/sc_tick.h "pair manifolds"); k_pair_manifolds_finish: its report.  Both live in
//                          sc_tick_pair_manifolds.hip, a translation unit of their own, so that the kernels of this one keep their
//                          instruction streams whatever the manifolds grow into
//
// Touch events (include/sc_tick.h "touch events") are the pair events' difference over the touching SET: the <.., Events> instances enter
// every pair decided "not apart" into a second PairEventState's current table, probe its previous table and append to its `begun`, in
// the lane that decided the pair; k_pair_events_sweep / _finish then run on that state unchanged (launchPairEventsTail).  <true, false>
// is the kernel as it was; <false, true> writes no list; <true, true> decides each pair once for both.
//
// The filter only ever removes: a pair is dropped on a positive comparison alone, so a NaN keeps it, and a pair with a member that cannot
// be refined (a Bounds proxy, a neighbour tile's record, a degenerate matrix) is listed on its AABB answer.  Every loop has a fixed trip
// count; every index into the entity arrays is below the entity count, every index into the list below its capacity.  Plain HIP atomics
// and vector stores only.  All arithmetic is fp32, unfused, left to right, as the header states it operation by operation.
#include "sc_tick_internal.h"
#include "sc_tick_pair_contacts.h"

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

// (Member / fetchMember, Round / roundOf, Frame / frameOf, boxDist2, the two distance cores and the three routines roundRoundApart, roundBoxApart
//  and boxBoxApart: sc_tick_internal.h, shared with the sweeps and the overlap queries)

// List: the touching list and its report (SC_TICK_PAIR_SHAPES).  Events: every pair decided "not apart" enters the touch state's current
// table in the same lane and the same pass, as k_pair_events_diff enters a pair of the pair list (SC_TICK_TOUCH_EVENTS); `e` is then
// not looked at unless List is set too, and `t` is looked at only with Events.
template <bool List, bool Events>
__global__ __launch_bounds__(kTile) void k_pair_shapes(const DeviceState d, const PairShapeState e, const PairEventState t, uint32_t parity,
                                                       uint32_t maxPairs, uint32_t count, uint32_t rankBits)
{
  static_assert(kPairShards == 64, "one lane per shard counter");
  static_assert(List || Events, "a pass with nothing to write");
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
  if constexpr (List) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {             // what the report needs besides the running counts
      e.ctl[kPsTested] = total;
      e.ctl[kPsPairsTruncated] = d.counters[kCtrPar + 8u * parity + kCtrPairs] != 0u ? 1u : 0u;      // pairs found after every segment was full
    }
  }
  // touch events: a truncated pair list is an overflow tick -- the same answer in every workgroup, nothing is entered anywhere.  Whether
  // the touching set fits is not known before the pairs are decided: the wave that counts itself past maxTracked raises the word.
  bool enter = false;
  unsigned long long* curT = nullptr;
  const unsigned long long* prevT = nullptr;
  uint32_t* prevM = nullptr;
  uint32_t mask = 0u;
  if constexpr (Events) {
    enter = d.counters[kCtrPar + 8u * parity + kCtrPairs] == 0u;
    if (!enter && blockIdx.x == 0 && threadIdx.x == 0) t.ctl[kPeOverflow] = 1u;
    const uint32_t cur = t.ctl[kPeCur] & 1u;
    curT = t.table[cur]; prevT = t.table[cur ^ 1u]; prevM = t.marks[cur ^ 1u];
    mask = t.slots - 1u;
  }
  const uint32_t stride = gridDim.x * kTile;
  for (uint32_t base = blockIdx.x * kTile + (threadIdx.x & ~63u); base < total; base += stride) {      // (wave-uniform trip count)
    if constexpr (Events) {
      // an overflow tick lists and remembers nothing: stop entering once the word is up (one value for the wave: its first lane's)
      if (enter) {
        const uint32_t up = __hip_atomic_load(&t.ctl[kPeOverflow], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        enter = __builtin_amdgcn_readfirstlane(up) == 0u;
      }
      if (!List && !enter) break;                             // (wave-uniform: nothing is left for this wave to write)
    }
    const uint32_t i = base + lane;
    bool touching = false, refined = false, kept = false;
    uint2 pr = make_uint2(0u, 0u);
    if (i < total) {
      uint32_t s = 0;                                         // the segment pair i lies in: the last one that starts at or before i
#pragma unroll
      for (uint32_t step = 32u; step; step >>= 1) if (prefix[s + step] <= i) s += step;
      pr = d.pairs[(size_t)s * shardCap + (i - prefix[s])];
      const Member ma = fetchMember(d, pr.x, count, rankBits), mb = fetchMember(d, pr.y, count, rankBits);
      if (!(ma.ok && mb.ok)) { kept = true; touching = true; }
      else {
        refined = true;
        const bool boxA = ma.type == kColliderBox, boxB = mb.type == kColliderBox;
        bool apart;
        if (boxA && boxB) apart = boxBoxApart(ma, mb);
        else if (boxA) apart = roundBoxApart(mb, ma);
        else if (boxB) apart = roundBoxApart(ma, mb);
        else apart = roundRoundApart(ma, mb);
        touching = !apart;
      }
    }
    if constexpr (List) {
      const unsigned long long mr = ballot64(refined), mk = ballot64(kept);
      if (lane == 0) {
        if (mr) atomicAdd(&e.ctl[kPsRefined], (uint32_t)__popcll(mr));
        if (mk) atomicAdd(&e.ctl[kPsKept], (uint32_t)__popcll(mk));
      }
      appendWave(touching, pr, &e.ctl[kPsTouching], e.list, e.maxTouching);
    }
    if constexpr (Events) {
      bool inserted = false, found = false;
      const unsigned long long key = ((unsigned long long)pr.x << 32) | pr.y;
      // (no pair has a == b == 0; the key is the tables' "empty")
      if (enter && touching && key != 0ull) pairSetEnter(t, curT, prevT, prevM, mask, key, inserted, found);
      const unsigned long long mt = ballot64(inserted);
      if (mt && lane == 0) {
        const uint32_t added = (uint32_t)__popcll(mt);
        const uint32_t before = atomicAdd(&t.ctl[kPeTracked], added);
        if (before + added > t.maxTracked) atomicOr(&t.ctl[kPeOverflow], 1u);      // the touching set does not fit
      }
      appendWave(inserted && !found, pr, &t.ctl[kPeBegun], t.begun, t.maxEvents);
    }
  }
}

__global__ __launch_bounds__(64) void k_pair_shapes_finish(const PairShapeState e)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t touching = e.ctl[kPsTouching];
  e.info[0] = e.ctl[kPsTested]; e.info[1] = touching; e.info[2] = e.ctl[kPsRefined]; e.info[3] = e.ctl[kPsKept];
  e.info[4] = touching > e.maxTouching ? 1u : 0u; e.info[5] = e.ctl[kPsPairsTruncated];
  e.ctl[kPsTouching] = 0u; e.ctl[kPsRefined] = 0u; e.ctl[kPsKept] = 0u; e.ctl[kPsTested] = 0u; e.ctl[kPsPairsTruncated] = 0u;
}

// ---- pair contacts (include/sc_tick.h "pair contacts"): point, depth, normal and kind of every entry of the touching list ----
// (Contact and the three contact routines: sc_tick_pair_contacts.h, shared with the pair manifolds of sc_tick_pair_manifolds.hip)
//
// A thread per entry of the touching list the pass before just wrote (its running count is still up: k_pair_shapes_finish runs behind
// this kernel).  The grid goes by the list's capacity; the entry count is read here, so the launch replays from a captured graph.  The
// members' rows and records are the ones the pass before fetched.  Kind counts: one ballot per counter and trip, one atomic per counter
// and wave; k_pair_contacts_finish, one thread behind it, turns them into the report and zeroes them for the next tick (a ticket
// drawn behind a fence by every workgroup or wave was measured first: the fences cost more than the launch).
__global__ __launch_bounds__(kTile) void k_pair_contacts(const DeviceState d, const PairShapeState e, const PairContactState k, uint32_t count,
                                                         uint32_t rankBits)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t listed = e.ctl[kPsTouching];
  const uint32_t room = e.maxTouching < k.maxTouching ? e.maxTouching : k.maxTouching;      // (one number: the contact buffer follows the list)
  const uint32_t n = listed < room ? listed : room;
  uint32_t tally[6] = { 0u, 0u, 0u, 0u, 0u, 0u };          // (wave-uniform) kPcRoundRound .. kPcDegenerate
  const uint32_t stride = gridDim.x * kTile;
  for (uint32_t base = blockIdx.x * kTile + (threadIdx.x & ~63u); base < n; base += stride) {      // (wave-uniform trip count)
    const uint32_t i = base + lane;
    const bool live = i < n;
    uint32_t kind = kContactNone;
    if (live) {
      const uint2 pr = e.list[i];
      const Member ma = fetchMember(d, pr.x, count, rankBits), mb = fetchMember(d, pr.y, count, rankBits);
      Contact c;
      c.p[0] = c.p[1] = c.p[2] = 0.0f; c.depth = 0.0f; c.n[0] = c.n[1] = c.n[2] = 0.0f; c.kind = kContactNone;
      if (ma.ok && mb.ok) {
        const bool boxA = ma.type == kColliderBox, boxB = mb.type == kColliderBox;
        if (boxA && boxB) c = contactBoxBox(ma, mb);
        else if (boxA) c = contactRoundBox(mb, ma, false);
        else if (boxB) c = contactRoundBox(ma, mb, true);
        else c = contactRoundRound(ma, mb);
      }
      kind = c.kind;
      k.rec[2u * (size_t)i] = make_float4(c.p[0], c.p[1], c.p[2], c.depth);
      k.rec[2u * (size_t)i + 1u] = make_float4(c.n[0], c.n[1], c.n[2], __uint_as_float(kind));
    }
    const uint32_t shape = kind & 0xFFu;
    tally[kPcRoundRound] += (uint32_t)__popcll(ballot64(live && shape == kContactRoundRound));
    tally[kPcRoundBox] += (uint32_t)__popcll(ballot64(live && shape == kContactRoundBox));
    tally[kPcBoxBox] += (uint32_t)__popcll(ballot64(live && shape >= kContactBoxFaceA));
    tally[kPcUnrefined] += (uint32_t)__popcll(ballot64(live && shape == kContactNone));
    tally[kPcDeep] += (uint32_t)__popcll(ballot64(live && (kind & kContactDeep) != 0u));
    tally[kPcDegenerate] += (uint32_t)__popcll(ballot64(live && (kind & kContactDegenerate) != 0u));
  }
  if (lane == 0) {
#pragma unroll
    for (uint32_t j = 0; j < 6u; ++j) if (tally[j]) atomicAdd(&k.ctl[j], tally[j]);
  }
}

// one thread behind k_pair_contacts: the tick's report (ScTickPairContactInfo), the kind counts back to zero
__global__ __launch_bounds__(64) void k_pair_contacts_finish(const PairShapeState e, const PairContactState k)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t listed = e.ctl[kPsTouching];
  const uint32_t room = e.maxTouching < k.maxTouching ? e.maxTouching : k.maxTouching;
  k.info[0] = listed < room ? listed : room;
#pragma unroll
  for (uint32_t j = 0; j < 6u; ++j) { k.info[1u + j] = k.ctl[j]; k.ctl[j] = 0u; }
  k.info[7] = 0u;
}

} // namespace

// One narrow-phase launch per tick, whatever mix of SC_TICK_PAIR_SHAPES (list) and SC_TICK_TOUCH_EVENTS (touch) the run carries: each
// pair is decided once.  Behind it the list's report and / or the touch state's sweep and finish (k_pair_events_sweep / _finish, unchanged).
void launchPairShapes(const DeviceState& d, const TickParams& p, const NarrowPhase& np, uint32_t stages, hipStream_t s)
{
  const bool list = (stages & kStageList) != 0u, touch = (stages & kStageTouch) != 0u;
  if (!list && !touch) return;
  // the grid by the pair list's capacity alone: a thread per pair it can hold (grid-stride beyond that)
  const uint32_t blocks = std::min(std::max((p.maxPairs + kTile - 1u) / kTile, 1u), 2048u);
  const PairShapeState e = list ? np.list : PairShapeState{};
  const PairEventState t = touch ? np.touch : PairEventState{};
  if (list && touch) hipLaunchKernelGGL((k_pair_shapes<true, true>), dim3(blocks), dim3(kTile), 0, s, d, e, t, p.parity, p.maxPairs, p.n, p.rankBits);
  else if (list) hipLaunchKernelGGL((k_pair_shapes<true, false>), dim3(blocks), dim3(kTile), 0, s, d, e, t, p.parity, p.maxPairs, p.n, p.rankBits);
  else hipLaunchKernelGGL((k_pair_shapes<false, true>), dim3(blocks), dim3(kTile), 0, s, d, e, t, p.parity, p.maxPairs, p.n, p.rankBits);
  if (stages & kStageContacts) {
    // a thread per entry the list can hold (grid-stride beyond the cap), between the pass and its report, which zeroes the count
    const uint32_t cblocks = std::min(std::max((e.maxTouching + kTile - 1u) / kTile, 1u), 2048u);
    hipLaunchKernelGGL(k_pair_contacts, dim3(cblocks), dim3(kTile), 0, s, d, e, np.contacts, p.n, p.rankBits);
    hipLaunchKernelGGL(k_pair_contacts_finish, dim3(1), dim3(64), 0, s, e, np.contacts);
  }
  if (stages & kStageManifolds) launchPairManifolds(d, p, e, np.manifolds, s);      // behind the contacts' report, before the list's
  if (stages & kStagePersist) launchPairPersist(d, p, e, np.manifolds, np.persist, s);      // behind the manifolds' records
  if (stages & kStageIslands) launchPairIslands(d, p, e, np.islands, s);      // needs the list, not the contacts; before the list's report
  if (stages & kStageSleep) launchPairSleep(d, p, e, np.islands, np.sleep, s);      // labels and edge islands are final
  if (list) hipLaunchKernelGGL(k_pair_shapes_finish, dim3(1), dim3(64), 0, s, e);
  if (touch) launchPairEventsTail(t, s);
}

} // namespace sctick
