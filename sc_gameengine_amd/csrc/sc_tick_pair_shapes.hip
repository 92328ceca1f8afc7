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

// (Member / fetchMember, Round / roundOf, Frame / frameOf, boxDist2 and the two distance cores: sc_tick_internal.h, shared with the sweeps)
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
// The routines below restate the header's text operation by operation, over the same Member / Round / Frame and the same two cores the
// decisions above went through.  A register array is never indexed by a run-time value: sel3 picks by comparisons.
struct Contact { float p[3]; float depth; float n[3]; uint32_t kind; };

__device__ __forceinline__ float sel3(int i, float a0, float a1, float a2) { return (i == 0) ? a0 : ((i == 1) ? a1 : a2); }
__device__ __forceinline__ float signOf(float x) { return (x < 0.0f) ? -1.0f : 1.0f; }      // (sign(0) = sign(NaN) = +1)
__device__ __forceinline__ float clampTo(float x, float h) { const float c = (x < -h) ? -h : x; return (c > h) ? h : c; }
// T + (x_0 u_0 + x_1 u_1) + x_2 u_2, per component: a point of the frame's coordinates in the world
__device__ __forceinline__ void fromFrame(const Frame& f, const float T[3], const float x[3], float out[3])
{
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = T[c] + ((x[0] * f.u[0][c] + x[1] * f.u[1][c]) + x[2] * f.u[2][c]);
}

__device__ __forceinline__ Contact contactRoundRound(const Member& ma, const Member& mb)
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
  const bool apartPoints = c.dist2 > 0.0f;
  const float dist = sqrtf(c.dist2);
  Contact o;
  o.kind = apartPoints ? kContactRoundRound : (kContactRoundRound | kContactDegenerate);
  o.depth = apartPoints ? sum - dist : sum;
  // the stretch of the line Pa + normal*x that lies in both rounds: [-Ra, Ra] and [dist - Rb, dist + Rb]; the point is its middle
  const float far = dist + rb.R, near = dist - rb.R;
  const float hi = (far < ra.R) ? far : ra.R, lo = (near < -ra.R) ? -ra.R : near;
  const float mid = (lo + hi) * 0.5f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float pa = p1[i] + d1[i] * c.s;
    const float n = (-c.v[i]) / dist;
    o.n[i] = apartPoints ? n : ((i == 1) ? 1.0f : 0.0f);
    o.p[i] = apartPoints ? pa + n * mid : pa;
  }
  return o;
}

__device__ __forceinline__ Contact contactRoundBox(const Member& mr, const Member& mx, bool roundIsA)
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
  float y[3], q[3], m[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { y[k] = y0[k] + dy[k] * c.at; q[k] = clampTo(y[k], fr.H[k]); m[k] = fr.H[k] - fabsf(y[k]); }
  const bool shallow = c.fmin > 0.0f;
  const float dist = sqrtf(c.fmin);
  // deep: the face nearest to y -- the first of the smallest H_k - |y_k|
  int kd = 0; float least = m[0];
  if (m[1] < least) { least = m[1]; kd = 1; }
  if (m[2] < least) { least = m[2]; kd = 2; }
  const float sg = signOf(sel3(kd, y[0], y[1], y[2]));
  // ... and how far the whole centre line reaches in below that face: its end that lies lower along the face's normal (a point: y itself)
  const float yk0 = sel3(kd, y0[0], y0[1], y0[2]), dyk = sel3(kd, dy[0], dy[1], dy[2]);
  const float e0 = sg * yk0, e1 = sg * (yk0 + dyk);
  const float low = (e1 < e0) ? e1 : e0;
  const float hk = sel3(kd, fr.H[0], fr.H[1], fr.H[2]);
  float nb[3], ell[3];                                       // the box's outward direction in its frame; the box's depth behind q along it, per axis
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float e = (y[k] - q[k]) / dist;
    nb[k] = shallow ? e : ((k == kd) ? sg : 0.0f);
    ell[k] = (fr.H[k] + fr.H[k]) / fabsf(e);
  }
  // the stretch of the line y + nBox*x that lies in both shapes; the point is its middle
  //   shallow: the round [-R, R], the box [-(dist + l), -dist] with l the least ell_k;  deep: the box [m - 2H, m] of the face's axis
  float l = ell[0];
  if (ell[1] < l) l = ell[1];
  if (ell[2] < l) l = ell[2];
  const float far = dist + l, back = least - (hk + hk);
  const float hiS = (far < rd.R) ? far : rd.R;
  const float loD = (back < -rd.R) ? -rd.R : back, hiD = (least < rd.R) ? least : rd.R;
  const float mid = shallow ? -((dist + hiS) * 0.5f) : (loD + hiD) * 0.5f;
  Contact o;
  o.kind = shallow ? kContactRoundBox : (kContactRoundBox | kContactDeep);
  o.depth = shallow ? rd.R - dist : rd.R + (hk - low);
  float onLine[3];
  fromFrame(fr, mx.T, y, onLine);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float nBox = (nb[0] * fr.u[0][i] + nb[1] * fr.u[1][i]) + nb[2] * fr.u[2][i];
    o.p[i] = onLine[i] + nBox * mid;
    o.n[i] = roundIsA ? -nBox : nBox;
  }
  return o;
}

__device__ __forceinline__ Contact contactBoxBox(const Member& ma, const Member& mb)
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
  // the axis of least overlap: strict <, in boxBoxApart's order, so a tie stays with the earlier axis
  float bo = 0.0f, bt = 0.0f, bL[3] = { 0.0f, 0.0f, 0.0f };
  uint32_t bkind = kContactBoxFaceA; int bi = 0, bj = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {                            // L = A's axis i
    const float rb = (fb.H[0] * Ab[i][0] + fb.H[1] * Ab[i][1]) + fb.H[2] * Ab[i][2];
    const float o = (fa.H[i] + rb) - fabsf(t[i]);
    if (i == 0 || o < bo) { bo = o; bt = t[i]; bi = i; bL[0] = fa.u[i][0]; bL[1] = fa.u[i][1]; bL[2] = fa.u[i][2]; }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {                            // L = B's axis j
    const float ra = (fa.H[0] * Ab[0][j] + fa.H[1] * Ab[1][j]) + fa.H[2] * Ab[2][j];
    const float tl = (t[0] * Rm[0][j] + t[1] * Rm[1][j]) + t[2] * Rm[2][j];
    const float o = (ra + fb.H[j]) - fabsf(tl);
    if (o < bo) { bo = o; bt = tl; bkind = kContactBoxFaceB; bj = j; bL[0] = fb.u[j][0]; bL[1] = fb.u[j][1]; bL[2] = fb.u[j][2]; }
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
      const float l2 = 1.0f - Rm[i][j] * Rm[i][j];
      const float o = ((ra + rb) - fabsf(tl)) / sqrtf(l2);
      if (!(l2 < kPairContactsEdgeEps) && o < bo) {
        bo = o; bt = tl; bkind = kContactBoxEdge; bi = i; bj = j;
#pragma unroll
        for (int c = 0; c < 3; ++c) bL[c] = Rm[i1][j] * fa.u[i2][c] - Rm[i2][j] * fa.u[i1][c];
      }
    }
  }
  Contact o;
  o.kind = bkind;
  o.depth = (bo < 0.0f) ? 0.0f : bo;
  const float sg = signOf(bt);
  const float len = sqrtf(dot3(bL, bL));
#pragma unroll
  for (int c = 0; c < 3; ++c) o.n[c] = (bkind == kContactBoxEdge) ? sg * (bL[c] / len) : sg * bL[c];
  const float half = o.depth * 0.5f;
  if (bkind != kContactBoxEdge) {
    // a face: the other box's vertex furthest towards it, clamped into the face, half the depth back along the normal
    const bool ofB = bkind == kContactBoxFaceB;
    Frame fo, ft; float To[3], Tt[3];                        // the face's owner and the other box
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      fo.H[k] = ofB ? fb.H[k] : fa.H[k]; ft.H[k] = ofB ? fa.H[k] : fb.H[k];
      To[k] = ofB ? mb.T[k] : ma.T[k]; Tt[k] = ofB ? ma.T[k] : mb.T[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) { fo.u[k][c] = ofB ? fb.u[k][c] : fa.u[k][c]; ft.u[k][c] = ofB ? fa.u[k][c] : fb.u[k][c]; }
    }
    const int ax = ofB ? bj : bi;
    float g[3], p[3], r[3], x[3], pc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const bool neg = dot3(o.n, ft.u[k]) < 0.0f;
      g[k] = ((neg != ofB) ? -1.0f : 1.0f) * ft.H[k];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      p[c] = Tt[c] - ((g[0] * ft.u[0][c] + g[1] * ft.u[1][c]) + g[2] * ft.u[2][c]);
      r[c] = p[c] - To[c];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float xk = dot3(r, fo.u[k]); x[k] = (k == ax) ? xk : clampTo(xk, fo.H[k]); }
    fromFrame(fo, To, x, pc);
#pragma unroll
    for (int c = 0; c < 3; ++c) o.p[c] = ofB ? pc[c] - o.n[c] * half : pc[c] + o.n[c] * half;
  } else {
    // an edge of each: A's furthest along the normal, B's furthest against it; the midpoint of their closest points
    float ga[3], gb[3], ea[3], eb[3], p1[3], d1[3], p2[3], d2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ga[k] = (k == bi) ? 0.0f : signOf(dot3(o.n, fa.u[k])) * fa.H[k];
      gb[k] = (k == bj) ? 0.0f : (-signOf(dot3(o.n, fb.u[k]))) * fb.H[k];
    }
    fromFrame(fa, ma.T, ga, ea);
    fromFrame(fb, mb.T, gb, eb);
    const float ha = sel3(bi, fa.H[0], fa.H[1], fa.H[2]), hb = sel3(bj, fb.H[0], fb.H[1], fb.H[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float va = sel3(bi, fa.u[0][c], fa.u[1][c], fa.u[2][c]) * ha, vb = sel3(bj, fb.u[0][c], fb.u[1][c], fb.u[2][c]) * hb;
      p1[c] = ea[c] - va; d1[c] = va + va;
      p2[c] = eb[c] - vb; d2[c] = vb + vb;
    }
    const SegSeg s = segSegCore(p1, d1, p2, d2);
#pragma unroll
    for (int c = 0; c < 3; ++c) o.p[c] = ((p1[c] + d1[c] * s.s) + (p2[c] + d2[c] * s.t)) * 0.5f;
  }
  return o;
}

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
void launchPairShapes(const DeviceState& d, const TickParams& p, const PairShapeState* list, const PairEventState* touch, const PairContactState* contacts,
                      hipStream_t s)
{
  if (list && !list->ctl) list = nullptr;
  if (touch && !touch->ctl) touch = nullptr;
  if (!list && !touch) return;
  // the grid by the pair list's capacity alone: a thread per pair it can hold (grid-stride beyond that)
  const uint32_t blocks = std::min(std::max((p.maxPairs + kTile - 1u) / kTile, 1u), 2048u);
  const PairShapeState e = list ? *list : PairShapeState{};
  const PairEventState t = touch ? *touch : PairEventState{};
  if (list && touch) hipLaunchKernelGGL((k_pair_shapes<true, true>), dim3(blocks), dim3(kTile), 0, s, d, e, t, p.parity, p.maxPairs, p.n, p.rankBits);
  else if (list) hipLaunchKernelGGL((k_pair_shapes<true, false>), dim3(blocks), dim3(kTile), 0, s, d, e, t, p.parity, p.maxPairs, p.n, p.rankBits);
  else hipLaunchKernelGGL((k_pair_shapes<false, true>), dim3(blocks), dim3(kTile), 0, s, d, e, t, p.parity, p.maxPairs, p.n, p.rankBits);
  if (list && contacts && contacts->ctl) {
    // a thread per entry the list can hold (grid-stride beyond the cap), between the pass and its report, which zeroes the count
    const uint32_t cblocks = std::min(std::max((list->maxTouching + kTile - 1u) / kTile, 1u), 2048u);
    hipLaunchKernelGGL(k_pair_contacts, dim3(cblocks), dim3(kTile), 0, s, d, e, *contacts, p.n, p.rankBits);
    hipLaunchKernelGGL(k_pair_contacts_finish, dim3(1), dim3(64), 0, s, e, *contacts);
  }
  if (list) hipLaunchKernelGGL(k_pair_shapes_finish, dim3(1), dim3(64), 0, s, e);
  if (touch) launchPairEventsTail(t, s);
}

} // namespace sctick
