// sc_tick_queries.hip -- ray queries over the broadphase bins of the current tick.
//
// Shaped like PhysicsWorld::raycast (src/engine/physics/sc_physics.cpp:740-777): direction normalised the same
// way (rejected when |dir|^2 <= 1e-6), segment from origin to origin + ndir * maxDist, Bullet's default filter
// with the callback's group 0xFFFF and mask = the caller's mask, closest hit wins.  The reference tests Bullet's
// exact shapes; Bullet is not in the tree, so -- as for the pair search -- the spec here is this build's own:
// candidates are the WORLD AABBs the broadphase already holds, and the ray-box arithmetic is the reference's
// own slab test, intersectRayAABB (tools/world_editor/editor_core/editor_core.cpp:438-470), with the far limit
// set to maxDist.  Equal distances go to the lower id (PickEntity keeps the first, :487-491).
//
// One wave per ray.  The wave walks the sectors under the ray's xz extent, skipping those the segment misses;
// lanes take one bin record each; then the big list.  Every lane keeps its own best hit; one 64-bit min over
// (distance bits, id) picks the winner, whose lane writes the result.
// The capsule sweeps, the entity-anchored rays and the traffic AI's obstacle rays below share that wave routine.
#include "sc_tick_internal.h"

namespace sctick {

namespace {

struct Slab { bool hit; float t; uint32_t axis; };

// intersectRayAABB, editor_core.cpp:438-470 (tmax starts at the ray's length instead of 1e30)
__device__ __forceinline__ Slab rayBox(const float o[3], const float dir[3], float maxDist, const float4& lo, const float4& hi)
{
  const float mn[3] = { lo.x, lo.y, lo.z }, mx[3] = { hi.x, hi.y, hi.z };
  Slab s; s.hit = true; s.t = 0.0f; s.axis = 3u;
  float tmin = 0.0f, tmax = maxDist;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (fabsf(dir[i]) < 1e-6f) {
      if (o[i] < mn[i] || o[i] > mx[i]) s.hit = false;
    } else {
      const float ood = 1.0f / dir[i];
      float t1 = (mn[i] - o[i]) * ood, t2 = (mx[i] - o[i]) * ood;
      if (t1 > t2) { const float k = t1; t1 = t2; t2 = k; }
      if (t1 > tmin) { tmin = t1; s.axis = (uint32_t)i; }          // std::max(tmin, t1)
      tmax = tmax < t2 ? tmax : t2;                                 // std::min(tmax, t2)
      if (tmin > tmax) s.hit = false;
    }
  }
  s.t = tmin;
  return s;
}

// One ray, cast by a whole wave (every lane must call): `valid` false = no segment (|dir|^2 <= 1e-6 or a negative length).
// The result is wave-uniform.  skipId: a box that never answers (0xFFFFFFFF = none) -- an agent's own box for its front ray.
struct WaveRay { bool valid, hit; float t; uint32_t id, axis, layer; float dir[3]; };

// the outward normal of the axis-aligned face that a segment along `dir` entered through axis a (< 3); selects, not indexed
// arrays: an index the compiler cannot resolve puts the array in LDS
__device__ __forceinline__ float3 faceNormal(uint32_t a, const float dir[3])
{
  const float da = a == 0u ? dir[0] : (a == 1u ? dir[1] : dir[2]);
  const float sgn = da > 0.0f ? -1.0f : 1.0f;
  return make_float3(a == 0u ? sgn : 0.0f, a == 1u ? sgn : 0.0f, a == 2u ? sgn : 0.0f);
}

// ---- exact collider shapes (own spec, include/sc_tick.h "exact shapes for rays") ---------------------------------------------
// SC_TICK_RAY_SHAPES_EXACT: a candidate that passed the slab test against its AABB and whose proxy comes from a typed collider of this
// context is answered by the shape itself, taken through the entity's world matrix of this tick.  All of it fp32, unfused, left to right;
// every acceptance is a positive comparison, so a NaN is a miss.  c_k: column k of the matrix, T: its translation, q = o - T.
// (dot3: sc_tick_internal.h)
// what a shape reports: never -0 (the wave's 64-bit min orders distances by their bit patterns)
__device__ __forceinline__ float notNegative(float t) { return t > 0.0f ? t : 0.0f; }

// kShapeStands: the AABB answer stands (a degenerate box matrix); kShapeInside: the ray starts inside -- t = +0, normal (0, 1, 0)
enum : uint32_t { kShapeStands = 0u, kShapeMiss = 1u, kShapeHit = 2u, kShapeInside = 3u };
struct ShapeHit { uint32_t kind; float t; float n[3]; };

// a sphere of radius R about the point the ray's origin is qc away from
__device__ __forceinline__ ShapeHit roundHit(const float qc[3], float R, const float dir[3], float L)
{
  ShapeHit h; h.kind = kShapeMiss; h.t = 0.0f; h.n[0] = 0.0f; h.n[1] = 1.0f; h.n[2] = 0.0f;
  const float b = dot3(qc, dir);
  const float c = dot3(qc, qc) - R * R;
  if (c <= 0.0f) { h.kind = kShapeInside; return h; }
  if (!(b < 0.0f)) return h;
  const float disc = b * b - c;
  if (!(disc >= 0.0f)) return h;
  const float t = notNegative((-b) - sqrtf(disc));
  if (!(t <= L)) return h;
  h.kind = kShapeHit; h.t = t;
#pragma unroll
  for (int r = 0; r < 3; ++r) h.n[r] = (qc[r] + dir[r] * t) / R;
  return h;
}

// entity e's collider (type: box, sphere or capsule) against the ray (o, dir, L) that met its AABB
__device__ __forceinline__ ShapeHit shapeHit(const DeviceState& d, uint32_t e, uint32_t type, const float o[3], const float dir[3], float L)
{
  const float4 s = d.colShape[e];                       // (ex, ey, ez, radius)
  const float4 r0 = d.w0[e], r1 = d.w1[e], r2 = d.w2[e];
  const float c0[3] = { r0.x, r1.x, r2.x }, c1[3] = { r0.y, r1.y, r2.y }, c2[3] = { r0.z, r1.z, r2.z };
  const float q[3] = { o[0] - r0.w, o[1] - r1.w, o[2] - r2.w };
  const float n0 = dot3(c0, c0), n1 = dot3(c1, c1), n2 = dot3(c2, c2);
  ShapeHit h; h.kind = kShapeStands; h.t = 0.0f; h.n[0] = 0.0f; h.n[1] = 1.0f; h.n[2] = 0.0f;
  if (type == kColliderBox) {
    // the ray in the box's own frame: the slab test again, parallel-axis rule included
    if (!(n0 > 0.0f && n1 > 0.0f && n2 > 0.0f && isfinite(n0) && isfinite(n1) && isfinite(n2))) return h;
    const float lo[3] = { dot3(c0, q) / n0, dot3(c1, q) / n1, dot3(c2, q) / n2 };
    const float ld[3] = { dot3(c0, dir) / n0, dot3(c1, dir) / n1, dot3(c2, dir) / n2 };
    const Slab sl = rayBox(lo, ld, L, make_float4(-s.x, -s.y, -s.z, 0.0f), make_float4(s.x, s.y, s.z, 0.0f));
    if (!sl.hit) { h.kind = kShapeMiss; return h; }
    h.kind = kShapeHit; h.t = sl.t;                     // (tmin starts at +0 and only grows: never -0)
    if (sl.axis < 3u) {                                 // the face's outward normal: the unit column, against the ray
      const float lda = sl.axis == 0u ? ld[0] : (sl.axis == 1u ? ld[1] : ld[2]);
      const float na = sl.axis == 0u ? n0 : (sl.axis == 1u ? n1 : n2);
      const float sgn = lda > 0.0f ? -1.0f : 1.0f, inv = 1.0f / sqrtf(na);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const float ca = sl.axis == 0u ? c0[r] : (sl.axis == 1u ? c1[r] : c2[r]);
        h.n[r] = sgn * (ca * inv) + 0.0f;               // (+ 0: a zero component is +0 whatever the sign, as the AABB answer has it)
      }
    }
    return h;
  }
  // the round part's radius, the columns selected as colliderAabb selects them for its pad
  const float nyz = (type == kColliderSphere && n2 < n1) ? n1 : n2;
  const float R = s.w * sqrtf((n0 < nyz) ? nyz : n0);
  if (type == kColliderSphere) h = roundHit(q, R, dir, L);
  else {
    const float A[3] = { c1[0] * s.y, c1[1] * s.y, c1[2] * s.y };      // half the capsule's axis
    const float aa = dot3(A, A);
    if (!(aa > 0.0f)) h = roundHit(q, R, dir, L);
    else {
      const float ad = dot3(A, dir), aq = dot3(A, q), dq = dot3(dir, q), qq = dot3(q, q);
      const float ka = aa - ad * ad, kb = aa * dq - aq * ad, kc = (aa * qq - aq * aq) - (R * R) * aa;
      const float qp[3] = { q[0] + A[0], q[1] + A[1], q[2] + A[2] }, qm[3] = { q[0] - A[0], q[1] - A[1], q[2] - A[2] };
      const ShapeHit capP = roundHit(qp, R, dir, L), capM = roundHit(qm, R, dir, L);
      const bool inBody = kc <= 0.0f && -aa <= aq && aq <= aa;
      h.kind = kShapeMiss;
      if (inBody || capP.kind == kShapeInside || capM.kind == kShapeInside) h.kind = kShapeInside;
      else {
        if (kc > 0.0f && ka > 0.0f && kb < 0.0f) {      // the side: the infinite cylinder, between the two seams
          const float disc = kb * kb - ka * kc;
          if (disc >= 0.0f) {
            const float tb = notNegative(((-kb) - sqrtf(disc)) / ka);
            const float yb = aq + tb * ad;
            if (-aa <= yb && yb <= aa && tb <= L) {
              const float f = yb / aa;
              h.kind = kShapeHit; h.t = tb;
#pragma unroll
              for (int r = 0; r < 3; ++r) h.n[r] = ((q[r] + dir[r] * tb) - A[r] * f) / R;
            }
          }
        }
        if (capP.kind == kShapeHit && (h.kind != kShapeHit || capP.t < h.t)) h = capP;
        if (capM.kind == kShapeHit && (h.kind != kShapeHit || capM.t < h.t)) h = capM;
      }
    }
  }
  if (h.kind == kShapeInside) { h.kind = kShapeHit; h.t = 0.0f; h.n[0] = 0.0f; h.n[1] = 1.0f; h.n[2] = 0.0f; }
  return h;
}

// ---- exact collider shapes for capsule sweeps (own spec, include/sc_tick.h "exact shapes for capsule sweeps") ----------------------
// SC_TICK_SWEEP_SHAPES_EXACT: a candidate whose grown AABB the segment met at t0 and that is refinable the way a member of a touching pair
// is (fetchMember) is answered by a conservative advancement of the sweeper -- the round (o + dir*t, A = (0, ay, 0), radius) -- towards the
// collider's shape: gap(t) = sqrt(dist2(t)) - Rs with dist2 from the touching pairs' distance cores, a step of `gap` metres or to the zero
// of the secant through the last two iterates, whichever is further (gap is convex in t: neither passes the first contact).  The frame or
// round of the target is built once, outside the step loop; the loop has a fixed trip count.  exhausted: the steps ran out (a hit at the
// travel reached).
__device__ __forceinline__ ShapeHit sweepShapeHit(const Member& m, const float o[3], const float dir[3], float far, float ay, float radius, float t0,
                                                  bool& exhausted)
{
  ShapeHit h; h.kind = kShapeMiss; h.t = 0.0f; h.n[0] = 0.0f; h.n[1] = 1.0f; h.n[2] = 0.0f;
  exhausted = false;
  const bool box = m.type == kColliderBox;
  const float A[3] = { 0.0f, ay, 0.0f };
  const float d1[3] = { A[0] + A[0], A[1] + A[1], A[2] + A[2] };
  float p2[3] = { 0.0f, 0.0f, 0.0f }, d2[3] = { 0.0f, 0.0f, 0.0f }, ya[3] = { 0.0f, 0.0f, 0.0f }, dy[3] = { 0.0f, 0.0f, 0.0f }, Rs = radius;
  Frame fr;
#pragma unroll
  for (int k = 0; k < 3; ++k) { fr.u[k][0] = fr.u[k][1] = fr.u[k][2] = 0.0f; fr.H[k] = 0.0f; }
  if (box) {
    fr = frameOf(m);
#pragma unroll
    for (int k = 0; k < 3; ++k) { ya[k] = dot3(fr.u[k], A); dy[k] = ya[k] + ya[k]; }
  } else {
    const Round rt = roundOf(m);
#pragma unroll
    for (int i = 0; i < 3; ++i) { p2[i] = m.T[i] - rt.A[i]; d2[i] = rt.A[i] + rt.A[i]; }
    Rs = radius + rt.R;
  }
  float t = t0, tp = 0.0f, gp = 0.0f, v[3] = { 0.0f, 0.0f, 0.0f };
  bool prev = false, met = false;
#pragma unroll 1
  for (int it = 0; it < kSweepShapesSteps; ++it) {
    float c[3], dist2;
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = o[i] + dir[i] * t;
    if (box) {
      float w[3], y0[3], z[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) w[i] = c[i] - m.T[i];
#pragma unroll
      for (int k = 0; k < 3; ++k) y0[k] = dot3(fr.u[k], w) - ya[k];
      const SegBox sb = segBoxCore(y0, dy, fr.H, ay != 0.0f);
      dist2 = sb.fmin;
      // the two closest points: the segment's at the minimising parameter, and that point clamped into the box, back in world space
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float y = y0[k] + dy[k] * sb.at;
        const float lo = (y < -fr.H[k]) ? -fr.H[k] : y;
        z[k] = (lo > fr.H[k]) ? fr.H[k] : lo;
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float ps = (c[i] - A[i]) + d1[i] * sb.at;
        const float pt = ((fr.u[0][i] * z[0] + fr.u[1][i] * z[1]) + fr.u[2][i] * z[2]) + m.T[i];
        v[i] = ps - pt;
      }
    } else {
      float p1[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) p1[i] = c[i] - A[i];
      const SegSeg ss = segSegCore(p1, d1, p2, d2);
      dist2 = ss.dist2;
      v[0] = ss.v[0]; v[1] = ss.v[1]; v[2] = ss.v[2];
    }
    if (t == 0.0f && !(dist2 > Rs * Rs)) { h.kind = kShapeHit; return h; }      // inside (the touching pairs' comparison: a NaN is inside)
    const float g = sqrtf(dist2) - Rs;
    if (g <= kSweepShapesTol) { met = true; break; }
    if (far == 0.0f) return h;                                                   // an overlap test: one evaluation
    float step = g;
    if (prev) {
      const float slope = (g - gp) / (t - tp);
      if (!(slope < 0.0f)) return h;                                             // convex and not approaching: it never arrives
      const float sec = (-g) / slope;
      if (sec > step) step = sec;
    }
    prev = true; tp = t; gp = g;
    t = t + step;
    if (t > far) return h;
  }
  exhausted = !met;
  h.kind = kShapeHit; h.t = t;
  const float vv = dot3(v, v);
  if (vv > 0.0f) { const float q = sqrtf(vv); h.n[0] = v[0] / q; h.n[1] = v[1] / q; h.n[2] = v[2] / q; }
  return h;
}

// What one sweep's wave counts for scTickGetSweepShapeInfo (wave-uniform).  A box lies in up to four sectors, and in the overflow list
// besides: the wave remembers the ids it has counted (seen[], its own row of LDS) and counts a box once per sweep.  Beyond kSweepSeenCap
// counted boxes per sweep nothing more is remembered and a box met again counts again.
struct SweepTally { uint32_t* seen; uint32_t nSeen, refined, kept, exhausted; };
enum : uint32_t { kTallyRefined = 1u, kTallyKept = 2u, kTallyExhausted = 4u };
// every lane of the wave must call; kind 0: this lane has nothing to count
__device__ __forceinline__ void sweepTally(SweepTally& tl, uint32_t kind, uint32_t id)
{
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long m = ballot64(kind != 0u);
  while (m) {                                                                      // (wave-uniform)
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1ull;
    const uint32_t bid = __shfl(id, src, 64), bk = __shfl(kind, src, 64);
    bool dup = false;
    for (uint32_t k = lane; k < tl.nSeen; k += 64u) dup = dup || tl.seen[k] == bid;
    if (ballot64(dup)) continue;
    if (tl.nSeen < kSweepSeenCap) { if (lane == 0) tl.seen[tl.nSeen] = bid; tl.nSeen++; }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    tl.refined += (bk & kTallyRefined) ? 1u : 0u; tl.kept += (bk & kTallyKept) ? 1u : 0u; tl.exhausted += (bk & kTallyExhausted) ? 1u : 0u;
  }
}

// The segment o + dir * [0, maxDist] against this tick's records, by a whole wave; fills hit / t / id / axis / layer of `w`.
// kSweep (capsule sweeps, k_sweep_queries): every candidate box is grown by `grow` per axis before the slab test, and the sector
// walk reaches `reach` (the sweeper's xz half extent) further on every side.  The ray instance (kSweep false) takes neither and
// is the routine the ray kernels always had.
// kExact (the exact-shape instances of the ray kernels): an AABB hit of an own typed collider is refined by shapeHit, lanes keep the
// normal instead of the face's axis, and the winner's normal travels with the other shuffles into wn[3] (w.axis is not filled).
// kSweep && kExact (k_sweep_queries<true>): a grown-AABB hit of a refinable member is refined by sweepShapeHit -- ay: the sweeper's half
// axis, grow[0] its radius -- and every candidate is counted once in `tally`.
template <bool kSweep, bool kExact = false>
__device__ __forceinline__ void castSegmentWave(WaveRay& w, const DeviceState& d, const TickParams& p, const float o[3], const float dir[3], float maxDist,
                                                uint32_t rayMask, uint32_t skipId, const float grow[3], float reach, float* wn = nullptr,
                                                float ay = 0.0f, SweepTally* tally = nullptr)
{
  const uint32_t lane = threadIdx.x & 63u;
  const float ex = o[0] + dir[0] * maxDist, ez = o[2] + dir[2] * maxDist;

  // this lane's best so far
  float bt = INFINITY; uint32_t bid = 0xFFFFFFFFu, baxis = 3u, blayer = 0u;
  float bn0 = 0.0f, bn1 = 1.0f, bn2 = 0.0f;
  uint32_t cKind = 0u, cId = 0u;                        // exact sweeps: what the last consider() leaves for sweepTally
  auto consider = [&](const float4& lo, const float4& hi) {
    const uint32_t lay = __float_as_uint(lo.w);
    // Bullet's needsCollision with the callback's group 0xFFFF: (proxy.group & mask) && (0xFFFF & proxy.mask)
    if (!((lay & 0xFFFFu) & rayMask) || !(lay >> 16)) return;
    const uint32_t id = __float_as_uint(hi.w) & ~kPrimary;
    if (id == skipId) return;
    // (the filter came first on purpose: a null record -- layers 0, inverted box -- grown by the sweeper could become a real box)
    const Slab s = kSweep ? rayBox(o, dir, maxDist, make_float4(lo.x - grow[0], lo.y - grow[1], lo.z - grow[2], 0.0f),
                                   make_float4(hi.x + grow[0], hi.y + grow[1], hi.z + grow[2], 0.0f))
                          : rayBox(o, dir, maxDist, lo, hi);
    if (!s.hit) return;
    if (kExact) {
      // the AABB answer, as rayHitOf would report it ...
      float t = s.t, n[3] = { 0.0f, 1.0f, 0.0f };
      if (s.axis < 3u) { const float3 f = faceNormal(s.axis, dir); n[0] = f.x; n[1] = f.y; n[2] = f.z; }
      // ... stands for Bounds proxies, a neighbour tile's records and a context without colliders
      if constexpr (kSweep) {
        // (... and for a degenerate matrix: the refinability rule of the touching pairs)
        const Member m = fetchMember(d, id, p.n, p.rankBits);
        cId = id;
        if (!m.ok) cKind = kTallyKept;
        else {
          bool ranOut;
          const ShapeHit h = sweepShapeHit(m, o, dir, maxDist, ay, grow[0], s.t, ranOut);
          cKind = kTallyRefined | (ranOut ? kTallyExhausted : 0u);
          if (h.kind == kShapeMiss) return;
          t = h.t; n[0] = h.n[0]; n[1] = h.n[1]; n[2] = h.n[2];
        }
        if (t < bt || (t == bt && id < bid)) { bt = t; bid = id; blayer = lay & 0xFFFFu; bn0 = n[0]; bn1 = n[1]; bn2 = n[2]; }
        return;
      }
      const uint32_t e = id & 0x00FFFFFFu;
      if (d.colType && (id & 0x7F000000u) == p.rankBits && e < p.n) {
        const uint32_t type = d.colType[e];
        if (type == kColliderBox || type == kColliderSphere || type == kColliderCapsule) {
          const ShapeHit h = shapeHit(d, e, type, o, dir, maxDist);
          if (h.kind == kShapeMiss) return;
          if (h.kind == kShapeHit) { t = h.t; n[0] = h.n[0]; n[1] = h.n[1]; n[2] = h.n[2]; }
        }
      }
      if (t < bt || (t == bt && id < bid)) { bt = t; bid = id; blayer = lay & 0xFFFFu; bn0 = n[0]; bn1 = n[1]; bn2 = n[2]; }
      return;
    }
    if (s.t < bt || (s.t == bt && id < bid)) { bt = s.t; bid = id; baxis = s.axis; blayer = lay & 0xFFFFu; }
  };

  // sectors under the segment's xz extent, clamped to the bin grid (boxes outside it are in the big list)
  // Sweeps: the extent grown by `reach` on every side.  That suffices: a box whose grown form the segment meets has a point within
  // `reach` (per axis, in x and z) of a point of the segment; that point of the box lies in a sector of the grown extent, and a box is
  // registered in every sector it overlaps -- or is in the big list.  The long-segment skip test below grows by the same amount.
  //
  // The extent must hold every box the CLOSED slab test can accept, and the two are rounded independently.  With u = 2^-24 and dir.x > 0
  // (the other signs and z alike), rayBox accepts a box only if t1 = fl(fl(mn.x - o.x) * fl(1 / dir.x)) <= maxDist -- three roundings:
  // mn.x - o.x <= dir.x * maxDist * (1 + 3.1u) -- while the end is ex = fl(o.x + fl(dir.x * maxDist)) >= o.x + dir.x * maxDist - u * (maxDist
  // + |ex|).  So mn.x <= ex + 4.1u * maxDist + u * |ex|: a face a few ulps of max(|o|, |ex|, maxDist) PAST the rounded end is still hit at
  // t == maxDist, and when a sector boundary lies in between, the box is registered only beyond it.  A sweep adds the roundings of the grown
  // face fl(mn.x - grow) and of fl(ex + reach), each below u * (|ex| + reach); a zero-length sweep is the same with maxDist = 0.  (On the
  // origin's side nothing is lost: fl(mx.x - o.x) >= 0 exactly when mx.x >= o.x, and floorf(x * invSector) is monotone.)  All of it stays
  // below 7u * (|o| + |ex| + maxDist + reach) per axis; the extent is padded by 16u of that sum, taken over both axes, on every side and
  // before the clamp to the grid.  The pad is 1 m where the sum is 2^20 m (1 049 km): below that the long-segment skip test's metre covers
  // the same roundings, so the skip test stays as it was.  An infinite sum pads to the whole grid; a NaN visits no bin, as before.
  const float ax = fabsf(o[0]) > fabsf(ex) ? fabsf(o[0]) : fabsf(ex), az = fabsf(o[2]) > fabsf(ez) ? fabsf(o[2]) : fabsf(ez);
  const float padded = reach + 0x1p-20f * ((ax > az ? ax : az) + maxDist + reach);
  const float fx0 = floorf(((o[0] < ex ? o[0] : ex) - padded) * p.invSector) - p.binOx, fx1 = floorf(((o[0] < ex ? ex : o[0]) + padded) * p.invSector) - p.binOx;
  const float fz0 = floorf(((o[2] < ez ? o[2] : ez) - padded) * p.invSector) - p.binOz, fz1 = floorf(((o[2] < ez ? ez : o[2]) + padded) * p.invSector) - p.binOz;
  const float gridX = (float)p.binSX - 1.0f, gridZ = (float)p.binSZ - 1.0f;
  bool anyOverflow = false;
  if (p.binSX && fx1 >= 0.0f && fz1 >= 0.0f && fx0 <= gridX && fz0 <= gridZ) {
    const uint32_t gx0 = (uint32_t)(fx0 < 0.0f ? 0.0f : fx0), gx1 = (uint32_t)(fx1 > gridX ? gridX : fx1);
    const uint32_t gz0 = (uint32_t)(fz0 < 0.0f ? 0.0f : fz0), gz1 = (uint32_t)(fz1 > gridZ ? gridZ : fz1);
    const float size = 1.0f / p.invSector;
    for (uint32_t gz = gz0; gz <= gz1; ++gz)
      for (uint32_t gx = gx0; gx <= gx1; ++gx) {
        if (gx1 - gx0 > 1u || gz1 - gz0 > 1u) {
          // long ray: skip sectors the segment cannot touch (the sector's square, grown by a metre -- a sweep: and by its reach -- as a flat box)
          const float margin = kSweep ? 1.0f + reach : 1.0f;
          const float4 lo = make_float4(((float)gx + p.binOx) * size - margin, -INFINITY, ((float)gz + p.binOz) * size - margin, 0.0f);
          const float4 hi = make_float4(((float)gx + p.binOx + 1.0f) * size + margin, INFINITY, ((float)gz + p.binOz + 1.0f) * size + margin, 0.0f);
          if (!rayBox(o, dir, maxDist, lo, hi).hit) continue;
        }
        const uint32_t s = gz * p.binSX + gx;
        uint32_t n = d.binCount[s];
        if (n > kBinCap) { n = kBinCap; anyOverflow = true; }
        if (kSweep && kExact) cKind = 0u;
        if (lane < n) {
          const float4* rec = d.bins + 2u * ((size_t)s * kBinCap + lane);
          consider(rec[0], rec[1]);
        }
        if constexpr (kSweep && kExact) sweepTally(*tally, cKind, cId);
      }
  }
  const uint32_t nbig = min(d.counters[kCtrPar + 8u * p.parity + kCtrBig], p.bigCap);
  if constexpr (kSweep && kExact) {
    // (the same records in the same lanes; the trip count is the wave's, so that every lane reaches the tally)
    for (uint32_t b0 = 0; b0 < nbig; b0 += 64u) {
      const uint32_t b = b0 + lane;
      cKind = 0u;
      if (b < nbig) consider(d.bigList[2u * (size_t)b], d.bigList[2u * (size_t)b + 1u]);
      sweepTally(*tally, cKind, cId);
    }
  } else {
    for (uint32_t b = lane; b < nbig; b += 64u) consider(d.bigList[2u * (size_t)b], d.bigList[2u * (size_t)b + 1u]);
  }
  // records that found their sector's bin full -- this tile's own boxes and a neighbour's border records (k_border_merge)
  // -- live only in the sector overflow list; they are this tile's to answer for like the records in the bins.  Duplicates
  // of a box that is also binned elsewhere are harmless: the same box gives the same distance and the id breaks the tie.
  // (Only a ray that crossed a sector holding more than its bin can meet one of them: a record of the list belongs to a
  //  sector whose counter passed 64.)
  if (anyOverflow) {
    const uint32_t nspill = min(d.counters[kCtrPar + 8u * p.parity + kCtrSpill], p.ovfCap);
    if constexpr (kSweep && kExact) {
      for (uint32_t e0 = 0; e0 < nspill; e0 += 64u) {
        const uint32_t e = e0 + lane;
        cKind = 0u;
        if (e < nspill) consider(d.spill[2u * (size_t)e], d.spill[2u * (size_t)e + 1u]);
        sweepTally(*tally, cKind, cId);
      }
    } else {
      for (uint32_t e = lane; e < nspill; e += 64u) consider(d.spill[2u * (size_t)e], d.spill[2u * (size_t)e + 1u]);
    }
  }

  // closest hit of the wave: distances are >= 0, so their bit patterns order like the values
  unsigned long long key = ((unsigned long long)__float_as_uint(bt) << 32) | bid;
  unsigned long long best = key;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_xor(best, off, 64);
    best = other < best ? other : best;
  }
  const bool found = bid != 0xFFFFFFFFu && key == best;
  const unsigned long long winners = ballot64(found);
  if (!winners) return;
  const int win = __ffsll((long long)winners) - 1;
  w.hit = true;
  w.t = __shfl(bt, win, 64); w.id = __shfl(bid, win, 64); w.layer = __shfl(blayer, win, 64);
  if (kExact) { wn[0] = __shfl(bn0, win, 64); wn[1] = __shfl(bn1, win, 64); wn[2] = __shfl(bn2, win, 64); }
  else w.axis = __shfl(baxis, win, 64);
}

template <bool kExact = false>
__device__ __forceinline__ WaveRay castRayWave(const DeviceState& d, const TickParams& p, const float o[3], const float dm[3], float maxDist,
                                               uint32_t rayMask, uint32_t skipId, float* wn = nullptr)
{
  WaveRay w; w.valid = false; w.hit = false; w.t = 0.0f; w.id = 0xFFFFFFFFu; w.axis = 3u; w.layer = 0u; w.dir[0] = w.dir[1] = w.dir[2] = 0.0f;
  const float lenSq = dm[0] * dm[0] + dm[1] * dm[1] + dm[2] * dm[2];
  // (a NaN or non-positive length is no segment either)
  if (!(lenSq > 1e-6f) || !(maxDist >= 0.0f)) return w;
  w.valid = true;
  const float invLen = 1.0f / sqrtf(lenSq);
  const float dir[3] = { dm[0] * invLen, dm[1] * invLen, dm[2] * invLen };
  w.dir[0] = dir[0]; w.dir[1] = dir[1]; w.dir[2] = dir[2];
  const float none[3] = { 0.0f, 0.0f, 0.0f };
  castSegmentWave<false, kExact>(w, d, p, o, dir, maxDist, rayMask, skipId, none, 0.0f, wn);
  return w;
}

// what a ray leaves for the host: RaycastHit{} (sc_physics.h:106-114) unless the wave found a box
// kExact: the winner brought its own normal (wn); otherwise the normal is the entered face's
template <bool kExact>
__device__ __forceinline__ RayHit48 rayHitOf(const WaveRay& w, const float o[3], const float wn[3])
{
  RayHit48 out;
  out.hit = 0u; out.id = 0xFFFFFFFFu; out.distance = 0.0f;
  out.position[0] = out.position[1] = out.position[2] = 0.0f;
  out.normal[0] = 0.0f; out.normal[1] = 1.0f; out.normal[2] = 0.0f;
  out.layer = 0u; out.pad = 0u; out.pad2 = 0u;
  if (w.hit) {
    out.hit = 1u; out.id = w.id; out.distance = w.t; out.layer = w.layer;
    out.position[0] = o[0] + w.dir[0] * w.t; out.position[1] = o[1] + w.dir[1] * w.t; out.position[2] = o[2] + w.dir[2] * w.t;
    if constexpr (kExact) { out.normal[0] = wn[0]; out.normal[1] = wn[1]; out.normal[2] = wn[2]; }
    else if (w.axis < 3u) {                             // the face the ray entered through; a ray starting inside keeps (0,1,0)
      const float3 f = faceNormal(w.axis, w.dir);
      out.normal[0] = f.x; out.normal[1] = f.y; out.normal[2] = f.z;
    }
  }
  return out;
}

// kExact (SC_TICK_RAY_SHAPES_EXACT): the instance launched instead of the AABB one, never next to it
template <bool kExact>
__global__ __launch_bounds__(kTile) void k_ray_queries(const DeviceState d, const TickParams p, const RayQueryState q)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * (kTile / 64u) + (threadIdx.x >> 6);
  if (r >= q.count) return;
  const float4 od = q.origin[r], dm = q.dir[r];
  const float o[3] = { od.x, od.y, od.z };
  const float dv[3] = { dm.x, dm.y, dm.z };
  float wn[3] = { 0.0f, 1.0f, 0.0f };
  const WaveRay w = castRayWave<kExact>(d, p, o, dv, od.w, __float_as_uint(dm.w), 0xFFFFFFFFu, wn);
  const RayHit48 out = rayHitOf<kExact>(w, o, wn);
  if (lane == 0) q.hits[r] = out;
}

// ---- entity-anchored rays (own spec, include/sc_tick.h "entity-anchored rays") -----------------------------------------------
// A ray given in an entity's local frame -- a wheel probe (VehicleWheelConfig::connectionPoint / direction, sc_physics.h:63-72), the
// vehicle camera's occlusion ray (sc_vehicle.cpp:570-611), the traffic debug sensor ray (sc_traffic_ai.cpp:622-652) -- is taken through
// this tick's world matrix of its anchor, fp32, unfused, left to right:
//   o_r = ((R_r.x*l.x + R_r.y*l.y) + R_r.z*l.z) + R_r.w        d_r = (R_r.x*v.x + R_r.y*v.y) + R_r.z*v.z
// and then answered as a ray of k_ray_queries is; max_dist is world metres.  An anchor beyond the entity count (a dead anchor is), a
// resolved origin that is not finite or a resolved direction whose squared length is not finite: a miss, noted as direction (0, 0, 0),
// which castRayWave rejects.  kAnchorNone: the ray is world space already and goes through untouched -- bit for bit a plain ray.
struct ResolvedRay { float o[3], dv[3]; float maxDist; uint32_t mask, skipId; };

__device__ __forceinline__ ResolvedRay resolveAnchoredRay(const DeviceState& d, const TickParams& p, const float4& lo, const float4& lv, const uint2 an)
{
  ResolvedRay r;
  r.o[0] = lo.x; r.o[1] = lo.y; r.o[2] = lo.z; r.dv[0] = lv.x; r.dv[1] = lv.y; r.dv[2] = lv.z;
  r.maxDist = lo.w; r.mask = __float_as_uint(lv.w); r.skipId = 0xFFFFFFFFu;
  if (an.x == kAnchorNone) return r;
  r.o[0] = r.o[1] = r.o[2] = 0.0f; r.dv[0] = r.dv[1] = r.dv[2] = 0.0f;
  if (an.x >= p.n) return r;
  const float4 row[3] = { d.w0[an.x], d.w1[an.x], d.w2[an.x] };
  float o[3], dv[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[k] = ((row[k].x * lo.x + row[k].y * lo.y) + row[k].z * lo.z) + row[k].w;
    dv[k] = (row[k].x * lv.x + row[k].y * lv.y) + row[k].z * lv.z;
  }
  const float lenSq = dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2];          // (as castRayWave forms it)
  if (!(isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(lenSq))) return r;
  r.o[0] = o[0]; r.o[1] = o[1]; r.o[2] = o[2]; r.dv[0] = dv[0]; r.dv[1] = dv[1]; r.dv[2] = dv[2];
  if (an.y) r.skipId = p.rankBits | an.x;                                     // the anchor's own box never answers
  return r;
}

// ray r as k_anchored_ray_snapshot noted it
__device__ __forceinline__ ResolvedRay snapshotRay(const AnchoredRayState& q, uint32_t r)
{
  const float4 a = q.snapOrigin[r], b = q.snapDir[r];
  ResolvedRay ray;
  ray.o[0] = a.x; ray.o[1] = a.y; ray.o[2] = a.z; ray.dv[0] = b.x; ray.dv[1] = b.y; ray.dv[2] = b.z;
  ray.maxDist = a.w; ray.mask = __float_as_uint(b.w); ray.skipId = q.snapSkip[r];
  return ray;
}

// One wave per ray, like k_ray_queries.  The ray index is made scalar, so the ray, its anchor word and the twelve words of the anchor's
// matrix rows come through the scalar path: one fetch per wave, not one per lane.  kFromSnapshot (the pair half of a split flow): the
// ray was resolved by k_anchored_ray_snapshot in the tick half and is cast as it stands there.  kExact (SC_TICK_RAY_SHAPES_EXACT): as for
// k_ray_queries; the snapshot holds the resolved ray, and the candidates are refined against the matrices as they stand.
template <bool kFromSnapshot, bool kExact>
__global__ __launch_bounds__(kTile) void k_anchored_rays(const DeviceState d, const TickParams p, const AnchoredRayState q)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * (kTile / 64u) + (threadIdx.x >> 6));
  if (r >= q.count) return;
  const ResolvedRay ray = kFromSnapshot ? snapshotRay(q, r) : resolveAnchoredRay(d, p, q.origin[r], q.dir[r], q.anchor[r]);
  float wn[3] = { 0.0f, 1.0f, 0.0f };
  const WaveRay w = castRayWave<kExact>(d, p, ray.o, ray.dv, ray.maxDist, ray.mask, ray.skipId, wn);
  const RayHit48 out = rayHitOf<kExact>(w, ray.o, wn);
  if (lane == 0) q.hits[r] = out;
}

// The resolve-only form (the tick half of a split flow): a thread per ray, the same arithmetic, the result noted in the parity's snapshot.
__global__ __launch_bounds__(kTile) void k_anchored_ray_snapshot(const DeviceState d, const TickParams p, const AnchoredRayState q)
{
  const uint32_t r = blockIdx.x * kTile + threadIdx.x;
  if (r >= q.count) return;
  const ResolvedRay ray = resolveAnchoredRay(d, p, q.origin[r], q.dir[r], q.anchor[r]);
  q.snapOrigin[r] = make_float4(ray.o[0], ray.o[1], ray.o[2], ray.maxDist);
  q.snapDir[r] = make_float4(ray.dv[0], ray.dv[1], ray.dv[2], __uint_as_float(ray.mask));
  q.snapSkip[r] = ray.skipId;
}

// ---- capsule sweeps (own spec, include/sc_tick.h "capsule sweeps"; shaped like PhysicsWorld::sweepCapsule, sc_physics.cpp:779-810) --
// The sweeper is the upright capsule's own AABB, e = (radius, max(0, halfHeight) + radius, radius); a box swept against a box is the
// segment against the box grown by e, so the test is rayBox again.  A segment of |d|^2 <= 1e-6 is an overlap test at `start`: direction
// (0, 0, 0) and length 0 send every axis of the slab test through its containment branch.  One wave per sweep.
// kExact (SC_TICK_SWEEP_SHAPES_EXACT; the instance launched instead of the AABB one, never next to it): the sweeper is the round (centre,
// A = (0, ay, 0), radius) in the sense of the touching pairs' roundOf -- not dot(A, A) > 0: a sphere --; the grown-AABB test stays the
// pre-filter and the winner brings its own normal.
// info (kExact): the three running words of ScTickSweepShapeInfo, zeroed on the stream before the launch
// (Set-up and hit writer are written out in the one body, the face normal by its own selects and the cast as two calls: handing this
//  kernel's local arrays to one more helper changes the order they become registers in -- DESIGN 11.20.)
template <bool kExact>
__global__ __launch_bounds__(kTile) void k_sweep_queries(const DeviceState d, const TickParams p, const SweepQueryState q, uint32_t* __restrict__ info)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = blockIdx.x * (kTile / 64u) + (threadIdx.x >> 6);
  if (r >= q.count) return;
  const float4 a = q.start[r], b = q.end[r];
  const uint2 f = q.filter[r];
  const float o[3] = { a.x, a.y, a.z };
  const float radius = a.w, hh = (b.w > 0.0f) ? b.w : 0.0f;
  const float grow[3] = { radius, hh + radius, radius };
  const float ay = (hh * hh > 0.0f) ? hh : 0.0f;       // (dot(A, A) of A = (0, hh, 0) is hh*hh to the bit)
  const float dv[3] = { b.x - a.x, b.y - a.y, b.z - a.z };
  const float lenSq = (dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2];
  float far = 0.0f, dir[3] = { 0.0f, 0.0f, 0.0f };
  if (lenSq > 1e-6f) {
    far = sqrtf(lenSq);
    const float inv = 1.0f / far;
    dir[0] = dv[0] * inv; dir[1] = dv[1] * inv; dir[2] = dv[2] * inv;
  }
  WaveRay w; w.valid = true; w.hit = false; w.t = 0.0f; w.id = 0xFFFFFFFFu; w.axis = 3u; w.layer = 0u;
  float wn[3] = { 0.0f, 1.0f, 0.0f };
  uint32_t* seenRow = nullptr;
  if constexpr (kExact) {
    __shared__ uint32_t seen[kTile / 64u][kSweepSeenCap];
    seenRow = seen[threadIdx.x >> 6];
  }
  SweepTally tally; tally.seen = seenRow; tally.nSeen = 0u; tally.refined = 0u; tally.kept = 0u; tally.exhausted = 0u;
  if constexpr (kExact) castSegmentWave<true, true>(w, d, p, o, dir, far, f.x, f.y, grow, radius, wn, ay, &tally);
  else castSegmentWave<true>(w, d, p, o, dir, far, f.x, f.y, grow, radius);
  SweepHit48 out;
  out.hit = 0u; out.id = 0xFFFFFFFFu; out.distance = 0.0f;
  out.position[0] = out.position[1] = out.position[2] = 0.0f;
  out.normal[0] = 0.0f; out.normal[1] = 1.0f; out.normal[2] = 0.0f;           // SweepHit{} (sc_physics.h:116)
  out.layer = 0u; out.travel = 0.0f; out.pad = 0u;
  if (w.hit) {
    out.hit = 1u; out.id = w.id; out.layer = w.layer; out.travel = w.t;
    out.distance = far > 0.0f ? w.t / far : 0.0f;                              // the hit FRACTION (m_closestHitFraction, :801)
    out.position[0] = o[0] + dir[0] * w.t; out.position[1] = o[1] + dir[1] * w.t; out.position[2] = o[2] + dir[2] * w.t;   // the capsule's centre
    if constexpr (kExact) { out.normal[0] = wn[0]; out.normal[1] = wn[1]; out.normal[2] = wn[2]; }
    else if (w.axis < 3u) {                             // the face entered; a sweep that starts in overlap keeps (0,1,0)
      const float dn = w.axis == 0u ? dir[0] : (w.axis == 1u ? dir[1] : dir[2]);
      const float sgn = dn > 0.0f ? -1.0f : 1.0f;
      out.normal[0] = w.axis == 0u ? sgn : 0.0f; out.normal[1] = w.axis == 1u ? sgn : 0.0f; out.normal[2] = w.axis == 2u ? sgn : 0.0f;
    }
  }
  if (lane == 0) {
    q.hits[r] = out;
    if constexpr (kExact) {
      if (tally.refined) atomicAdd(&info[0], tally.refined);
      if (tally.kept) atomicAdd(&info[1], tally.kept);
      if (tally.exhausted) atomicAdd(&info[2], tally.exhausted);
    }
  }
}

// ---- entity-anchored capsule sweeps (own spec, include/sc_tick.h "entity-anchored capsule sweeps") ----------------------------
// A sweep whose consumer is a moving entity -- a pedestrian's move test, a ground probe under a vehicle (PhysicsWorld::sweepCapsule,
// sc_physics.cpp:779-810, takes world-space points) -- is given in its anchor's local frame and taken through this tick's world matrix
// of the anchor, fp32, unfused, left to right: the start by resolveAnchoredRay's origin formula,
//   s_r = ((R_r.x*ls.x + R_r.y*ls.y) + R_r.z*ls.z) + R_r.w
// the end by the same formula (end_frame 0: a point of the anchor's frame) or e_r = s_r + le_r (end_frame 1: a world-space
// displacement).  kAnchorNone: s = ls, e = le or ls + le, untouched.  The status: an anchor beyond the entity count (a dead anchor is);
// a component of s or e, or the squared length of e - s as the sweep kernels form it, that is not finite.
struct ResolvedSweep { float s[3], e[3]; uint32_t skipId, status; };

__device__ __forceinline__ ResolvedSweep resolveAnchoredSweep(const DeviceState& d, const TickParams& p, const float4& ls, const float4& le, const uint4 an)
{
  ResolvedSweep r;
  const float l[3] = { ls.x, ls.y, ls.z }, m[3] = { le.x, le.y, le.z };
  r.skipId = 0xFFFFFFFFu; r.status = kASweepAnswered;
  if (an.x == kAnchorNone) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { r.s[k] = l[k]; r.e[k] = an.z ? l[k] + m[k] : m[k]; }
  } else {
    r.s[0] = r.s[1] = r.s[2] = 0.0f; r.e[0] = r.e[1] = r.e[2] = 0.0f;
    if (an.x >= p.n) { r.status = kASweepNoAnchor; return r; }
    const float4 row[3] = { d.w0[an.x], d.w1[an.x], d.w2[an.x] };
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      r.s[k] = ((row[k].x * l[0] + row[k].y * l[1]) + row[k].z * l[2]) + row[k].w;
      r.e[k] = an.z ? r.s[k] + m[k] : ((row[k].x * m[0] + row[k].y * m[1]) + row[k].z * m[2]) + row[k].w;
    }
    if (an.y) r.skipId = p.rankBits | an.x;                                    // the anchor's own box never answers
  }
  const float dv[3] = { r.e[0] - r.s[0], r.e[1] - r.s[1], r.e[2] - r.s[2] };
  const float lenSq = (dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2];         // (as k_sweep_queries forms it)
  if (!(isfinite(r.s[0]) && isfinite(r.s[1]) && isfinite(r.s[2]) && isfinite(r.e[0]) && isfinite(r.e[1]) && isfinite(r.e[2]) && isfinite(lenSq)))
    r.status = kASweepNotFinite;
  return r;
}

// One wave per sweep.  The sweep index is made scalar as in k_anchored_rays, so the sweep's words, its anchor word and the twelve words
// of the anchor's matrix rows come through the scalar path: one fetch per wave.  Behind the resolve the body IS k_sweep_queries' -- its
// set-up, its two casts, its hit writer -- written out a second time: that kernel's comment and DESIGN 11.20 say why it is not shared.
// Lane 0 also notes the status in the record's pad word and the resolved segment (quiet NaNs for a sweep that was not answered).
// info (kExact): three words of their own, zeroed on the stream before the launch, added to only when non-zero.
template <bool kExact>
__global__ __launch_bounds__(kTile) void k_anchored_sweeps(const DeviceState d, const TickParams p, const AnchoredSweepState q, uint32_t* __restrict__ info)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * (kTile / 64u) + (threadIdx.x >> 6));
  if (r >= q.count) return;
  const float4 a = q.start[r], b = q.end[r];
  const uint4 an = q.anchor[r];
  const ResolvedSweep rs = resolveAnchoredSweep(d, p, a, b, an);
  SweepHit48 out;
  out.hit = 0u; out.id = 0xFFFFFFFFu; out.distance = 0.0f;
  out.position[0] = out.position[1] = out.position[2] = 0.0f;
  out.normal[0] = 0.0f; out.normal[1] = 1.0f; out.normal[2] = 0.0f;           // SweepHit{} (sc_physics.h:116)
  out.layer = 0u; out.travel = 0.0f; out.pad = rs.status;
  if (rs.status != kASweepAnswered) {                   // (wave-uniform: every operand came through the scalar path)
    if (lane == 0) {
      const float nan = __uint_as_float(0x7FC00000u);
      q.hits[r] = out;
      q.segment[2u * (size_t)r] = make_float4(nan, nan, nan, 0.0f);
      q.segment[2u * (size_t)r + 1u] = make_float4(nan, nan, nan, 0.0f);
    }
    return;
  }
  const float o[3] = { rs.s[0], rs.s[1], rs.s[2] };
  const float radius = a.w, hh = (b.w > 0.0f) ? b.w : 0.0f;
  const float grow[3] = { radius, hh + radius, radius };
  const float ay = (hh * hh > 0.0f) ? hh : 0.0f;       // (dot(A, A) of A = (0, hh, 0) is hh*hh to the bit)
  const float dv[3] = { rs.e[0] - rs.s[0], rs.e[1] - rs.s[1], rs.e[2] - rs.s[2] };
  const float lenSq = (dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2];
  float far = 0.0f, dir[3] = { 0.0f, 0.0f, 0.0f };
  if (lenSq > 1e-6f) {
    far = sqrtf(lenSq);
    const float inv = 1.0f / far;
    dir[0] = dv[0] * inv; dir[1] = dv[1] * inv; dir[2] = dv[2] * inv;
  }
  WaveRay w; w.valid = true; w.hit = false; w.t = 0.0f; w.id = 0xFFFFFFFFu; w.axis = 3u; w.layer = 0u;
  float wn[3] = { 0.0f, 1.0f, 0.0f };
  uint32_t* seenRow = nullptr;
  if constexpr (kExact) {
    __shared__ uint32_t seen[kTile / 64u][kSweepSeenCap];
    seenRow = seen[threadIdx.x >> 6];
  }
  SweepTally tally; tally.seen = seenRow; tally.nSeen = 0u; tally.refined = 0u; tally.kept = 0u; tally.exhausted = 0u;
  if constexpr (kExact) castSegmentWave<true, true>(w, d, p, o, dir, far, an.w, rs.skipId, grow, radius, wn, ay, &tally);
  else castSegmentWave<true>(w, d, p, o, dir, far, an.w, rs.skipId, grow, radius);
  if (w.hit) {
    out.hit = 1u; out.id = w.id; out.layer = w.layer; out.travel = w.t;
    out.distance = far > 0.0f ? w.t / far : 0.0f;                              // the hit FRACTION (m_closestHitFraction, :801)
    out.position[0] = o[0] + dir[0] * w.t; out.position[1] = o[1] + dir[1] * w.t; out.position[2] = o[2] + dir[2] * w.t;   // the capsule's centre
    if constexpr (kExact) { out.normal[0] = wn[0]; out.normal[1] = wn[1]; out.normal[2] = wn[2]; }
    else if (w.axis < 3u) {                             // the face entered; a sweep that starts in overlap keeps (0,1,0)
      const float dn = w.axis == 0u ? dir[0] : (w.axis == 1u ? dir[1] : dir[2]);
      const float sgn = dn > 0.0f ? -1.0f : 1.0f;
      out.normal[0] = w.axis == 0u ? sgn : 0.0f; out.normal[1] = w.axis == 1u ? sgn : 0.0f; out.normal[2] = w.axis == 2u ? sgn : 0.0f;
    }
  }
  if (lane == 0) {
    q.hits[r] = out;
    q.segment[2u * (size_t)r] = make_float4(rs.s[0], rs.s[1], rs.s[2], 0.0f);
    q.segment[2u * (size_t)r + 1u] = make_float4(rs.e[0], rs.e[1], rs.e[2], 0.0f);
    if constexpr (kExact) {
      if (tally.refined) atomicAdd(&info[0], tally.refined);
      if (tally.kept) atomicAdd(&info[1], tally.kept);
      if (tally.exhausted) atomicAdd(&info[2], tally.exhausted);
    }
  }
}

// ---- overlap queries (own spec, include/sc_tick.h "overlap queries") ---------------------------------------------------------
// "Which entities are inside this volume": a collider without an entity -- type, record and world matrix as an entity's would be --
// tested against the world exactly as the touching pairs test a pair.  The volume's box is the collider box rule (colliderAabb,
// sc_tick_kernels.hip) over its matrix, stated here over a Member: n_k are the squared column norms as that rule forms them, and the half
// extent is ((|M[r,0]|*ex + |M[r,1]|*ey) + |M[r,2]|*ez) + pad, the same operations in the same order.
__device__ __forceinline__ void memberAabb(const Member& m, float mn[3], float mx[3])
{
  float pad = 0.0f;
  if (m.type != kColliderBox) {
    const float nyz = (m.type == kColliderSphere && m.n[2] < m.n[1]) ? m.n[1] : m.n[2];      // sphere: max(n1, n2); capsule: n2
    pad = m.s.w * sqrtf((m.n[0] < nyz) ? nyz : m.n[0]);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float h = fabsf(m.c[0][r]) * m.s.x + fabsf(m.c[1][r]) * m.s.y + fabsf(m.c[2][r]) * m.s.z + pad;
    mn[r] = m.T[r] - h; mx[r] = m.T[r] + h;
  }
}

// One wave per volume, one lane per record.  The wave takes the records it has to look at in CHUNKS of up to 64, in one loop: the bins
// of the rectangle floorf(min * invSector) .. floorf(max * invSector) of the volume's box, clamped to the grid, sector after sector; then
// the big list; then -- only when a sector of the rectangle held more than its bin -- the sector overflow list.  No pad: two closed
// intervals that meet share a point, floorf(x * invSector) is monotone, and planBins registers a box in every sector of that same
// range of its own.  The cost is linear in the sectors the rectangle covers; a volume over the whole grid reads every bin.
//   A box lies in up to four sectors.  As in the pair search, a (volume, record) hit counts only in the sector that holds the low corner
// of the two boxes' intersection, floorf(max(box.min, volume.min) * invSector) in x and z: that sector is in the box's own range and in
// the rectangle, so exactly one of the box's records reports it.  A record of the overflow list belongs to the sector it is tagged
// with; a box of the big list has one record.
//   The wave owns row r of the id buffer and word r of the counts: ballot, prefix popcount and a running count -- no atomics at all (the
// report's sums are formed by the reader), vector stores, every index below count * maxHits.  The loop's trip count is the wave's (the volume is wave-uniform: it comes through the scalar path).
// kExact (SC_TICK_OVERLAP_SHAPES_EXACT; the instance launched instead of the AABB one): a hit whose entity is refinable (fetchMember) is
// dropped when the touching pairs' routine for the two types says "apart", the entity as member A and the volume as member B; a
// candidate that cannot be refined, and every candidate of a volume with a degenerate matrix, stays a hit on its box answer.
template <bool kExact>
__global__ __launch_bounds__(kTile) void k_overlap_queries(const DeviceState d, const TickParams p, const OverlapQueryState q)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * (kTile / 64u) + (threadIdx.x >> 6));
  if (r >= q.count) return;
  const float4* vol = q.volume + (size_t)kOverlapVolumeWords * r;
  const float4 r0 = vol[0], r1 = vol[1], r2 = vol[2], word = vol[4];
  Member mv;
  mv.s = vol[3]; mv.type = __float_as_uint(word.x);
  mv.c[0][0] = r0.x; mv.c[0][1] = r1.x; mv.c[0][2] = r2.x;
  mv.c[1][0] = r0.y; mv.c[1][1] = r1.y; mv.c[1][2] = r2.y;
  mv.c[2][0] = r0.z; mv.c[2][1] = r1.z; mv.c[2][2] = r2.z;
  mv.T[0] = r0.w; mv.T[1] = r1.w; mv.T[2] = r2.w;
#pragma unroll
  for (int k = 0; k < 3; ++k) mv.n[k] = dot3(mv.c[k], mv.c[k]);
  mv.ok = mv.n[0] > 0.0f && mv.n[1] > 0.0f && mv.n[2] > 0.0f && isfinite(mv.n[0]) && isfinite(mv.n[1]) && isfinite(mv.n[2]);
  const uint32_t mask = __float_as_uint(word.y), skipId = __float_as_uint(word.z);
  float vmn[3], vmx[3];
  memberAabb(mv, vmn, vmx);

  // the rectangle (a NaN box compares false everywhere: no sector, and no record meets it)
  const float fx0 = floorf(vmn[0] * p.invSector) - p.binOx, fx1 = floorf(vmx[0] * p.invSector) - p.binOx;
  const float fz0 = floorf(vmn[2] * p.invSector) - p.binOz, fz1 = floorf(vmx[2] * p.invSector) - p.binOz;
  const float gridX = (float)p.binSX - 1.0f, gridZ = (float)p.binSZ - 1.0f;
  uint32_t gx0 = 0u, gz0 = 0u, width = 0u, nSec = 0u;
  if (p.binSX && fx1 >= 0.0f && fz1 >= 0.0f && fx0 <= gridX && fz0 <= gridZ) {
    gx0 = (uint32_t)(fx0 < 0.0f ? 0.0f : fx0); gz0 = (uint32_t)(fz0 < 0.0f ? 0.0f : fz0);
    const uint32_t gx1 = (uint32_t)(fx1 > gridX ? gridX : fx1), gz1 = (uint32_t)(fz1 > gridZ ? gridZ : fz1);
    width = gx1 - gx0 + 1u;
    nSec = width * (gz1 - gz0 + 1u);
  }
  const uint32_t ctr = kCtrPar + 8u * p.parity;
  const uint32_t nbig = min(d.counters[ctr + kCtrBig], p.bigCap), nspill = min(d.counters[ctr + kCtrSpill], p.ovfCap);
  const uint32_t bigEnd = nSec + (nbig + 63u) / 64u, spillChunks = (nspill + 63u) / 64u;
  bool anyOverflow = false;
  uint32_t total = 0u, refined = 0u, kept = 0u;      // (wave-uniform)
  uint32_t gx = gx0, gz = gz0;                          // the sector of chunk k while k < nSec
  uint32_t* row = q.ids + (size_t)r * q.maxHits;
  // (anyOverflow is final once the sectors are through, before it can matter)
  for (uint32_t k = 0; k < bigEnd + (anyOverflow ? spillChunks : 0u); ++k) {
    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
    bool have = false, bySector = false;
    uint32_t sx = 0u, sz = 0u;                          // bySector: the sector this record is registered in
    if (k < nSec) {
      const uint32_t s = gz * p.binSX + gx;
      uint32_t n = d.binCount[s];
      if (n > kBinCap) { n = kBinCap; anyOverflow = true; }
      have = lane < n; bySector = true; sx = gx; sz = gz;
      if (have) { const float4* rec = d.bins + 2u * ((size_t)s * kBinCap + lane); lo = rec[0]; hi = rec[1]; }
      if (++gx == gx0 + width) { gx = gx0; ++gz; }
    } else if (k < bigEnd) {
      const uint32_t b = (k - nSec) * 64u + lane;
      have = b < nbig;
      if (have) { lo = d.bigList[2u * (size_t)b]; hi = d.bigList[2u * (size_t)b + 1u]; }
    } else {
      const uint32_t e = (k - bigEnd) * 64u + lane;
      have = e < nspill; bySector = true;
      if (have) {
        lo = d.spill[2u * (size_t)e]; hi = d.spill[2u * (size_t)e + 1u];
        const uint32_t s = d.spillSector[e];
        sx = s % p.binSX; sz = s / p.binSX;
      }
    }
    // the rays' filter, the skip id, the pair rule's closed intervals (positive comparisons: a NaN meets nothing), the low corner
    const uint32_t lay = __float_as_uint(lo.w);
    const uint32_t id = __float_as_uint(hi.w) & ~kPrimary;
    bool hit = have && ((lay & 0xFFFFu) & mask) != 0u && (lay >> 16) != 0u && id != skipId &&
               lo.x <= vmx[0] && vmn[0] <= hi.x && lo.y <= vmx[1] && vmn[1] <= hi.y && lo.z <= vmx[2] && vmn[2] <= hi.z;
    if (bySector) {
      const float lx = lo.x > vmn[0] ? lo.x : vmn[0], lz = lo.z > vmn[2] ? lo.z : vmn[2];
      hit = hit && (floorf(lx * p.invSector) - p.binOx) == (float)sx && (floorf(lz * p.invSector) - p.binOz) == (float)sz;
    }
    if constexpr (kExact) {
      bool refine = false;
      if (hit) {
        const Member m = fetchMember(d, id, p.n, p.rankBits);
        refine = m.ok && mv.ok;
        if (refine) {
          const bool boxA = m.type == kColliderBox, boxB = mv.type == kColliderBox;
          bool apart;
          if (boxA && boxB) apart = boxBoxApart(m, mv);
          else if (boxA) apart = roundBoxApart(mv, m);
          else if (boxB) apart = roundBoxApart(m, mv);
          else apart = roundRoundApart(m, mv);
          hit = !apart;
        }
      }
      // refined: decided by a routine; kept: a hit that stands on its box answer
      const unsigned long long mr = ballot64(refine);
      refined += (uint32_t)__popcll(mr);
      kept += (uint32_t)__popcll(ballot64(hit) & ~mr);
    }
    const unsigned long long m = ballot64(hit);
    if (hit) {
      const uint32_t at = total + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (at < q.maxHits) row[at] = id;
    }
    total += (uint32_t)__popcll(m);
  }
  if (lane == 0) {
    q.counts[r] = total;
    if constexpr (kExact) q.tally[r] = make_uint2(refined, kept);
  }
}

// ---- trigger volumes (own spec, include/sc_tick.h "trigger volumes") -----------------------------------------------------------
// An overlap volume in an entity's local frame, and the tick-to-tick difference of its answer: what the anchored rays are to the rays.
// One wave per volume.  The volume index is made scalar, so the local matrix, the anchor word and the twelve words of the anchor's matrix
// rows come through the scalar path, as in k_anchored_rays.  The wave
//   1. resolves M = W * L (fp32, unfused, left to right; kAnchorNone: M = L untouched) and notes the rows for the reader; an anchor beyond
//      the entity count or a non-finite entry among the twelve: no members this tick, the rows noted as quiet NaNs;
//   2. walks sectors, big list and overflow list by k_overlap_queries' rules -- A SECOND COPY OF THAT LOOP, kept apart so that the
//      overlap kernels' instruction streams stay what they were -- collecting its row in LDS;
//   3. fetches the row it remembers (the volume's row in device memory, TriggerState::remembered slots of it) into LDS beside it;
//   4. forms entered = new \ old and exited = old \ new by chunked compares: a lane holds one id of one row and reads the other row
//      four ids per 16-byte LDS read, every lane the same address (a broadcast, no bank conflict); an id that is an event gets bit 31
//      (no id has it: ranks are below 128) so that nothing is compared twice;
//   5. reserves its slots of the two event lists with ONE atomic per list, and only when it has events (no per-hit
//      additions to a shared word; a steady world adds nothing at all), and writes (volume, id) pairs into the slots below maxEvents;
//   6. overwrites its row in device memory -- the member row the readers see IS the remembered row -- and its per-volume words: the true
//      count, the slots remembered (kTriggerNone after an overflow), (entered, exited, resync / overflow bits).
// No pointer is swapped and no state lives outside the volume's own words, so one captured graph replays every tick.
template <bool kExact>
__global__ __launch_bounds__(kTile) void k_trigger_volumes(const DeviceState d, const TickParams p, const TriggerState t)
{
  extern __shared__ __attribute__((aligned(16))) uint32_t triggerRows[];      // [kTile / 64][2][stride]
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * (kTile / 64u) + (threadIdx.x >> 6));
  if (r >= t.count) return;
  const uint32_t stride = (t.maxMembers + 3u) & ~3u;                          // rows start on 16 bytes and are read four ids at a time
  uint32_t* rowNew = triggerRows + (size_t)(threadIdx.x >> 6) * 2u * stride;
  uint32_t* rowOld = rowNew + stride;

  // 1. resolve
  const float4* vol = t.local + (size_t)kOverlapVolumeWords * r;
  const float4 l0 = vol[0], l1 = vol[1], l2 = vol[2], word = vol[4];
  const uint2 an = t.anchor[r];
  float4 r0 = l0, r1 = l1, r2 = l2;
  bool alive = true;
  uint32_t skipId = 0xFFFFFFFFu;
  if (an.x != kAnchorNone) {
    alive = an.x < p.n;
    if (alive) {
      const float4 w[3] = { d.w0[an.x], d.w1[an.x], d.w2[an.x] };
      float4 m[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        m[k].x = (w[k].x * l0.x + w[k].y * l1.x) + w[k].z * l2.x;
        m[k].y = (w[k].x * l0.y + w[k].y * l1.y) + w[k].z * l2.y;
        m[k].z = (w[k].x * l0.z + w[k].y * l1.z) + w[k].z * l2.z;
        m[k].w = ((w[k].x * l0.w + w[k].y * l1.w) + w[k].z * l2.w) + w[k].w;
      }
      r0 = m[0]; r1 = m[1]; r2 = m[2];
      if (an.y) skipId = p.rankBits | an.x;                                   // the carrier never answers
    }
  }
  alive = alive && isfinite(r0.x) && isfinite(r0.y) && isfinite(r0.z) && isfinite(r0.w) && isfinite(r1.x) && isfinite(r1.y) && isfinite(r1.z) &&
          isfinite(r1.w) && isfinite(r2.x) && isfinite(r2.y) && isfinite(r2.z) && isfinite(r2.w);
  if (!alive) { const float q = __uint_as_float(0x7FC00000u); r0 = r1 = r2 = make_float4(q, q, q, q); }
  if (lane == 0) { float4* out = t.world + 3u * (size_t)r; out[0] = r0; out[1] = r1; out[2] = r2; }

  Member mv;
  mv.s = vol[3]; mv.type = __float_as_uint(word.x);
  mv.c[0][0] = r0.x; mv.c[0][1] = r1.x; mv.c[0][2] = r2.x;
  mv.c[1][0] = r0.y; mv.c[1][1] = r1.y; mv.c[1][2] = r2.y;
  mv.c[2][0] = r0.z; mv.c[2][1] = r1.z; mv.c[2][2] = r2.z;
  mv.T[0] = r0.w; mv.T[1] = r1.w; mv.T[2] = r2.w;
#pragma unroll
  for (int k = 0; k < 3; ++k) mv.n[k] = dot3(mv.c[k], mv.c[k]);
  mv.ok = mv.n[0] > 0.0f && mv.n[1] > 0.0f && mv.n[2] > 0.0f && isfinite(mv.n[0]) && isfinite(mv.n[1]) && isfinite(mv.n[2]);
  const uint32_t mask = __float_as_uint(word.y);
  float vmn[3], vmx[3];
  memberAabb(mv, vmn, vmx);

  // 2. the walk (k_overlap_queries' loop; a volume without members has a NaN box: no sector, and the lists are not looked at either)
  const float fx0 = floorf(vmn[0] * p.invSector) - p.binOx, fx1 = floorf(vmx[0] * p.invSector) - p.binOx;
  const float fz0 = floorf(vmn[2] * p.invSector) - p.binOz, fz1 = floorf(vmx[2] * p.invSector) - p.binOz;
  const float gridX = (float)p.binSX - 1.0f, gridZ = (float)p.binSZ - 1.0f;
  uint32_t gx0 = 0u, gz0 = 0u, width = 0u, nSec = 0u;
  if (p.binSX && fx1 >= 0.0f && fz1 >= 0.0f && fx0 <= gridX && fz0 <= gridZ) {
    gx0 = (uint32_t)(fx0 < 0.0f ? 0.0f : fx0); gz0 = (uint32_t)(fz0 < 0.0f ? 0.0f : fz0);
    const uint32_t gx1 = (uint32_t)(fx1 > gridX ? gridX : fx1), gz1 = (uint32_t)(fz1 > gridZ ? gridZ : fz1);
    width = gx1 - gx0 + 1u;
    nSec = width * (gz1 - gz0 + 1u);
  }
  const uint32_t ctr = kCtrPar + 8u * p.parity;
  const uint32_t nbig = alive ? min(d.counters[ctr + kCtrBig], p.bigCap) : 0u, nspill = alive ? min(d.counters[ctr + kCtrSpill], p.ovfCap) : 0u;
  const uint32_t bigEnd = nSec + (nbig + 63u) / 64u, spillChunks = (nspill + 63u) / 64u;
  bool anyOverflow = false;
  uint32_t total = 0u;                                  // (wave-uniform)
  uint32_t gx = gx0, gz = gz0;
  for (uint32_t k = 0; k < bigEnd + (anyOverflow ? spillChunks : 0u); ++k) {
    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hi = lo;
    bool have = false, bySector = false;
    uint32_t sx = 0u, sz = 0u;
    if (k < nSec) {
      const uint32_t s = gz * p.binSX + gx;
      uint32_t n = d.binCount[s];
      if (n > kBinCap) { n = kBinCap; anyOverflow = true; }
      have = lane < n; bySector = true; sx = gx; sz = gz;
      if (have) { const float4* rec = d.bins + 2u * ((size_t)s * kBinCap + lane); lo = rec[0]; hi = rec[1]; }
      if (++gx == gx0 + width) { gx = gx0; ++gz; }
    } else if (k < bigEnd) {
      const uint32_t b = (k - nSec) * 64u + lane;
      have = b < nbig;
      if (have) { lo = d.bigList[2u * (size_t)b]; hi = d.bigList[2u * (size_t)b + 1u]; }
    } else {
      const uint32_t e = (k - bigEnd) * 64u + lane;
      have = e < nspill; bySector = true;
      if (have) {
        lo = d.spill[2u * (size_t)e]; hi = d.spill[2u * (size_t)e + 1u];
        const uint32_t s = d.spillSector[e];
        sx = s % p.binSX; sz = s / p.binSX;
      }
    }
    const uint32_t lay = __float_as_uint(lo.w);
    const uint32_t id = __float_as_uint(hi.w) & ~kPrimary;
    bool hit = have && ((lay & 0xFFFFu) & mask) != 0u && (lay >> 16) != 0u && id != skipId &&
               lo.x <= vmx[0] && vmn[0] <= hi.x && lo.y <= vmx[1] && vmn[1] <= hi.y && lo.z <= vmx[2] && vmn[2] <= hi.z;
    if (bySector) {
      const float lx = lo.x > vmn[0] ? lo.x : vmn[0], lz = lo.z > vmn[2] ? lo.z : vmn[2];
      hit = hit && (floorf(lx * p.invSector) - p.binOx) == (float)sx && (floorf(lz * p.invSector) - p.binOz) == (float)sz;
    }
    if constexpr (kExact) {
      if (hit) {
        const Member m = fetchMember(d, id, p.n, p.rankBits);
        if (m.ok && mv.ok) {
          const bool boxA = m.type == kColliderBox, boxB = mv.type == kColliderBox;
          bool apart;
          if (boxA && boxB) apart = boxBoxApart(m, mv);
          else if (boxA) apart = roundBoxApart(mv, m);
          else if (boxB) apart = roundBoxApart(m, mv);
          else apart = roundRoundApart(m, mv);
          hit = !apart;
        }
      }
    }
    const unsigned long long hm = ballot64(hit);
    if (hit) {
      const uint32_t at = total + (uint32_t)__popcll(hm & ((1ull << lane) - 1ull));
      if (at < t.maxMembers) rowNew[at] = id;
    }
    total += (uint32_t)__popcll(hm);
  }

  // 3. the remembered row beside the new one, both padded to whole 16-byte reads with a word no id equals
  const uint32_t rem = t.remembered[r];
  const bool overflow = total > t.maxMembers, resync = rem == kTriggerNone;
  const uint32_t nNew = overflow ? t.maxMembers : total;
  const uint32_t nOld = (resync || overflow) ? 0u : (rem < t.maxMembers ? rem : t.maxMembers);
  uint32_t* row = t.ids + (size_t)r * t.maxMembers;
  for (uint32_t i = lane; i < ((nOld + 3u) & ~3u); i += 64u) rowOld[i] = i < nOld ? row[i] : 0xFFFFFFFFu;
  if (lane < 3u && nNew + lane < ((nNew + 3u) & ~3u)) rowNew[nNew + lane] = 0xFFFFFFFFu;
  __builtin_amdgcn_wave_barrier();

  // 4. the two differences (an overflowing volume has no events; a resync tick enters its whole row)
  uint32_t entered = 0u, exited = 0u;
  if (!overflow) {
    for (uint32_t base = 0; base < nNew; base += 64u) {
      const uint32_t i = base + lane;
      const bool in = i < nNew;
      const uint32_t x = in ? rowNew[i] : 0u;
      bool found = false;
      for (uint32_t j = 0; j < nOld; j += 4u) {
        const uint4 o = *reinterpret_cast<const uint4*>(rowOld + j);
        found = found || o.x == x || o.y == x || o.z == x || o.w == x;
      }
      const bool ev = in && !found;
      if (ev) rowNew[i] = x | kPrimary;
      entered += (uint32_t)__popcll(ballot64(ev));
    }
    __builtin_amdgcn_wave_barrier();
    for (uint32_t base = 0; base < nOld; base += 64u) {
      const uint32_t i = base + lane;
      const bool in = i < nOld;
      const uint32_t x = in ? rowOld[i] : 0u;
      bool found = false;
      for (uint32_t j = 0; j < nNew; j += 4u) {
        const uint4 o = *reinterpret_cast<const uint4*>(rowNew + j);
        found = found || (o.x & ~kPrimary) == x || (o.y & ~kPrimary) == x || (o.z & ~kPrimary) == x || (o.w & ~kPrimary) == x;
      }
      const bool ev = in && !found;
      if (ev) rowOld[i] = x | kPrimary;
      exited += (uint32_t)__popcll(ballot64(ev));
    }
    __builtin_amdgcn_wave_barrier();

    // 5. the event slots: one reservation per list, the marked ids behind it
    uint32_t baseIn = 0u, baseOut = 0u;
    if (lane == 0) {
      if (entered) baseIn = atomicAdd(&t.ctl[0], entered);
      if (exited) baseOut = atomicAdd(&t.ctl[1], exited);
    }
    baseIn = __shfl(baseIn, 0, 64); baseOut = __shfl(baseOut, 0, 64);
    if (entered) {
      uint32_t done = 0u;
      for (uint32_t base = 0; base < nNew; base += 64u) {
        const uint32_t i = base + lane;
        const uint32_t x = i < nNew ? rowNew[i] : 0u;
        const bool ev = (x & kPrimary) != 0u;
        const unsigned long long em = ballot64(ev);
        const uint32_t at = baseIn + done + (uint32_t)__popcll(em & ((1ull << lane) - 1ull));
        if (ev && at < t.maxEvents) t.entered[at] = make_uint2(r, x & ~kPrimary);
        done += (uint32_t)__popcll(em);
      }
    }
    if (exited) {
      uint32_t done = 0u;
      for (uint32_t base = 0; base < nOld; base += 64u) {
        const uint32_t i = base + lane;
        const uint32_t x = i < nOld ? rowOld[i] : 0u;
        const bool ev = (x & kPrimary) != 0u;
        const unsigned long long em = ballot64(ev);
        const uint32_t at = baseOut + done + (uint32_t)__popcll(em & ((1ull << lane) - 1ull));
        if (ev && at < t.maxEvents) t.exited[at] = make_uint2(r, x & ~kPrimary);
        done += (uint32_t)__popcll(em);
      }
    }
  }

  // 6. the row in place, and the volume's words
  for (uint32_t i = lane; i < nNew; i += 64u) row[i] = rowNew[i] & ~kPrimary;
  if (lane == 0) {
    t.counts[r] = total;
    t.remembered[r] = overflow ? kTriggerNone : nNew;
    t.stat[r] = make_uint4(entered, exited, overflow ? kTriggerOverflow : (resync ? kTriggerResync : 0u), 0u);
  }
}

// ---- the traffic AI's obstacle ray (src/engine/traffic/sc_traffic_ai.cpp:300-345) --------------------------------------------
// Every agent of the OnRails tier casts one ray per step from 1.7 m ahead of its origin (0.6 m up) along its heading --
// forward = normalize(sin(yaw), 0, cos(yaw)) with the yaw's sin / cos as the entity's rotation streams hold them (host libm) --
// of TrafficSensors::frontRayLength (20 m) with mask 1, and brakes by clamp01((safe - d) / safe) when something other than
// itself is closer than TrafficSensors::safeDistance (10 m).  As for the ray queries above the candidates are the world AABBs
// of this tick's bins (own spec: Bullet is absent); the agent's own box never answers (Bullet does not report a convex shape a
// ray starts inside, and the reference discards a self hit: :322-325, :336).  The brake waits in aBrake[] for the on-rails
// step that produces the next frame.
//
// The OnRails agents of this tick, listed.  kWithRays (tiled world, in-order step): the rays are cast in the PAIR half, behind the border
// merge, so that an agent near a tile edge sees the neighbour tile's boxes too (the halo section of the border messages puts them in
// the ring bins).  The tick half only lists the agents and notes each one's ray as it stands -- the frame producer fused into the
// end-of-tick kernel moves the agents on before the pair half runs.
template <bool kWithRays>
__global__ __launch_bounds__(kTile) void k_list_onrails_agents(const DeviceState d, uint32_t n)
{
  const uint32_t i = blockIdx.x * kTile + threadIdx.x;
  const bool agent = i < n && d.moverKind[i] == kMoverTraffic && d.aMode[i] == kTierOnRails;
  const unsigned long long m = ballot64(agent);
  if (!m) return;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(d.agentCount, (uint32_t)__popcll(m));
  base = __shfl(base, 0, 64);
  if (agent) {
    const uint32_t k = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    d.agentList[k] = i;
    if constexpr (kWithRays) {
      float forward[3] = { d.rsy[i], 0.0f, d.rcy[i] };               // (the arithmetic of k_agent_front_rays<false>, where the citations are)
      const float len = sqrtf(forward[0] * forward[0] + forward[1] * forward[1] + forward[2] * forward[2]);
      if (len > 1e-6f) { const float inv = 1.0f / len; forward[0] *= inv; forward[1] *= inv; forward[2] *= inv; }
      d.agentRays[2u * k] = make_float4(d.px[i] + forward[0] * 1.7f, d.py[i] + 0.6f, d.pz[i] + forward[2] * 1.7f, d.aRayLen[i]);
      d.agentRays[2u * k + 1u] = make_float4(forward[0], forward[2], d.aSafe[i], 0.0f);
    }
  }
}

__global__ __launch_bounds__(kTile) void k_fill_sensors(const DeviceState d, uint32_t first, uint32_t count, float rayLen, float safe)
{
  const uint32_t t = blockIdx.x * kTile + threadIdx.x;
  if (t < count) { d.aRayLen[first + t] = rayLen; d.aSafe[first + t] = safe; }
}

// (per-agent TrafficSensors: every agent casts with its own frontRayLength and brakes by its own safeDistance, :306-308; the
//  hit's distance and kind are left for the host as lastHitDistance / lastHitType, :339-345 -- Vehicle when the hit entity is a
//  vehicle by its mover kind (a traffic agent or a SynthWorld vehicle: what carries a VehicleComponent, :327), World otherwise;
//  a box that arrived from a neighbour tile has no mover kind here: Vehicle when its group has the dynamic bit; without a hit the
//  ray's length and None)
// What agent i's ray leaves: the brake for the on-rails step, the hit's distance and kind for the host.  Every lane calls; lane 0 writes.
__device__ __forceinline__ void writeAgentSensor(const DeviceState& d, const TickParams& p, uint32_t i, const WaveRay& w, float rayLen, float safe, uint32_t lane)
{
  float brake = 0.0f;
  if (w.hit && safe > 1e-3f && w.t < safe) {
    const float v = (safe - w.t) / safe;                            // clamp01 = std::max(0, std::min(v, 1)), :16-24
    const float m = (1.0f < v) ? 1.0f : v;
    brake = (0.0f < m) ? m : 0.0f;
  }
  if (lane == 0) {
    d.aBrake[i] = brake;
    d.aHitDist[i] = w.hit ? w.t : rayLen;                           // :319-322, :341-345
    uint32_t kind = 0u;
    if (w.hit) {
      const bool own = (w.id & 0x7F000000u) == p.rankBits;
      const uint32_t mk = own ? d.moverKind[w.id & 0x00FFFFFFu] : 0u;
      kind = own ? ((mk == 1u || mk == kMoverTraffic) ? 2u : 3u) : ((w.layer & 1u) ? 2u : 3u);
    }
    d.aHitType[i] = kind;
  }
}

// A wave per agent of the list.  kFromSnapshot: the pair half casts the rays that k_list_onrails_agents<true> noted in the tick half.
template <bool kFromSnapshot>
__global__ __launch_bounds__(kTile) void k_agent_front_rays(const DeviceState d, const TickParams p)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t count = *d.agentCount;
  const uint32_t waves = gridDim.x * (kTile / 64u);
  for (uint32_t k = blockIdx.x * (kTile / 64u) + (threadIdx.x >> 6); k < count; k += waves) {
    const uint32_t i = d.agentList[k];
    float origin[3], forward[3], rayLen, safe;
    if constexpr (kFromSnapshot) {
      const float4 a = d.agentRays[2u * k], b = d.agentRays[2u * k + 1u];
      origin[0] = a.x; origin[1] = a.y; origin[2] = a.z; forward[0] = b.x; forward[1] = 0.0f; forward[2] = b.y;
      rayLen = a.w; safe = b.z;
    } else {
      forward[0] = d.rsy[i]; forward[1] = 0.0f; forward[2] = d.rcy[i];                                         // { sin(currentYaw), 0, cos(currentYaw) }, :304
      const float len = sqrtf(forward[0] * forward[0] + forward[1] * forward[1] + forward[2] * forward[2]);      // normalize3, :38-48
      if (len > 1e-6f) { const float inv = 1.0f / len; forward[0] *= inv; forward[1] *= inv; forward[2] *= inv; }
      origin[0] = d.px[i] + forward[0] * 1.7f; origin[1] = d.py[i] + 0.6f; origin[2] = d.pz[i] + forward[2] * 1.7f;   // :311-315
      rayLen = d.aRayLen[i]; safe = d.aSafe[i];                       // :306-308
    }
    const WaveRay w = castRayWave(d, p, origin, forward, rayLen, 1u, i | p.rankBits);
    writeAgentSensor(d, p, i, w, rayLen, safe, lane);
  }
}

// isOccupiedWorld (src/engine/traffic/sc_traffic_spawner.cpp:93-116): is any agent closer than `radius` to the point, in the
// xz plane, by Transform::localPos -- dx*dx + dz*dz < radius*radius, strictly.  The reference walks the TrafficAgent and
// VehicleComponent pools; here an entity counts when its collision group meets the query's mask.  A handful of
// queries per frame (spawn attempts) against every entity: one thread per entity, all queries from LDS.
__global__ __launch_bounds__(kTile) void k_occupancy(const DeviceState d, uint32_t n, const float4* __restrict__ q, uint32_t count,
                                                     uint32_t* __restrict__ blocked)
{
  __shared__ float4 sq[kMaxOccupancyQueries];
  for (uint32_t k = threadIdx.x; k < count; k += kTile) sq[k] = q[k];
  __syncthreads();
  const uint32_t i = blockIdx.x * kTile + threadIdx.x;
  if (i >= n) return;
  const uint32_t group = d.layers[i] & 0xFFFFu;
  if (!group) return;
  const float x = d.px[i], z = d.pz[i];
  for (uint32_t k = 0; k < count; ++k) {
    const float4 c = sq[k];                              // (x, z, radius, mask)
    if (!(group & __float_as_uint(c.w))) continue;
    const float dx = x - c.x, dz = z - c.y;
    if (dx * dx + dz * dz < c.z * c.z) atomicOr(&blocked[k >> 5], 1u << (k & 31u));
  }
}

} // namespace

void launchOccupancy(const DeviceState& d, uint32_t n, const float4* q, uint32_t count, uint32_t* blocked, hipStream_t s)
{
  if (!n || !count) return;
  hipLaunchKernelGGL(k_occupancy, dim3((n + kTile - 1) / kTile), dim3(kTile), 0, s, d, n, q, count, blocked);
}

void launchFillSensors(const DeviceState& d, uint32_t first, uint32_t count, float rayLen, float safe, hipStream_t s)
{
  if (!count || !d.aRayLen) return;
  hipLaunchKernelGGL(k_fill_sensors, dim3((count + kTile - 1) / kTile), dim3(kTile), 0, s, d, first, count, rayLen, safe);
}

void launchAgentFrontRays(const DeviceState& d, const TickParams& p, hipStream_t s)
{
  if (!p.n || !d.aLane || !d.aBrake) return;
  hipMemsetAsync(d.agentCount, 0, sizeof(uint32_t), s);
  hipLaunchKernelGGL(k_list_onrails_agents<false>, dim3((p.n + kTile - 1) / kTile), dim3(kTile), 0, s, d, p.n);
  const uint32_t blocks = std::min((p.n + 3u) / 4u, 8192u);          // (a wave per agent, wave-strided over the list the kernel above wrote)
  hipLaunchKernelGGL(k_agent_front_rays<false>, dim3(std::max(blocks, 1u)), dim3(kTile), 0, s, d, p);
}

void launchAgentRaySnapshot(const DeviceState& d, const TickParams& p, hipStream_t s)
{
  if (!p.n || !d.aLane || !d.aBrake || !d.agentRays) return;
  hipMemsetAsync(d.agentCount, 0, sizeof(uint32_t), s);
  hipLaunchKernelGGL(k_list_onrails_agents<true>, dim3((p.n + kTile - 1) / kTile), dim3(kTile), 0, s, d, p.n);
}
void launchAgentFrontRaysFromSnapshot(const DeviceState& d, const TickParams& p, hipStream_t s)
{
  if (!p.n || !d.aLane || !d.aBrake || !d.agentRays) return;
  const uint32_t blocks = std::min((p.n + 3u) / 4u, 8192u);
  hipLaunchKernelGGL(k_agent_front_rays<true>, dim3(std::max(blocks, 1u)), dim3(kTile), 0, s, d, p);
}

// a wave per query, kTile / 64 queries a workgroup; an empty batch launches nothing
template <typename... Params, typename... Args>
static void launchWavePerQuery(void (*kernel)(Params...), uint32_t count, hipStream_t s, const Args&... args)
{
  const uint32_t perBlock = kTile / 64u;
  if (count) hipLaunchKernelGGL(kernel, dim3((count + perBlock - 1) / perBlock), dim3(kTile), 0, s, args...);
}

void launchRayQueries(const DeviceState& d, const TickParams& p, const RayQueryState& q, bool exact, hipStream_t s)
{
  launchWavePerQuery(exact ? k_ray_queries<true> : k_ray_queries<false>, q.count, s, d, p, q);
}

void launchSweepQueries(const DeviceState& d, const TickParams& p, const SweepQueryState& q, uint32_t* exactInfo, hipStream_t s)
{
  if (exactInfo) hipMemsetAsync(exactInfo, 0, kSweepInfoWords * sizeof(uint32_t), s);      // (an empty batch reports zeros)
  launchWavePerQuery(exactInfo ? k_sweep_queries<true> : k_sweep_queries<false>, q.count, s, d, p, q, exactInfo);
}

void launchAnchoredSweeps(const DeviceState& d, const TickParams& p, const AnchoredSweepState& q, uint32_t* exactInfo, hipStream_t s)
{
  if (exactInfo) hipMemsetAsync(exactInfo, 0, kSweepInfoWords * sizeof(uint32_t), s);      // (words of their own: a run with both flags fills both reports)
  launchWavePerQuery(exactInfo ? k_anchored_sweeps<true> : k_anchored_sweeps<false>, q.count, s, d, p, q, exactInfo);
}

void launchOverlapQueries(const DeviceState& d, const TickParams& p, const OverlapQueryState& q, bool exact, hipStream_t s)
{
  launchWavePerQuery(exact ? k_overlap_queries<true> : k_overlap_queries<false>, q.count, s, d, p, q);
}

// a wave per volume like the queries above, plus the wave's two rows in LDS: 2 * 4 * roundup4(maxMembers) bytes per wave, 32 KB per
// workgroup at the row cap; the two slot counters start every tick at zero (inside a captured graph too)
void launchTriggerVolumes(const DeviceState& d, const TickParams& p, const TriggerState& t, bool exact, hipStream_t s)
{
  if (!t.count) return;
  const uint32_t perBlock = kTile / 64u;
  const uint32_t stride = (std::min(t.maxMembers, kTriggerRowCap) + 3u) & ~3u;
  hipMemsetAsync(t.ctl, 0, 2u * sizeof(uint32_t), s);
  hipLaunchKernelGGL(exact ? k_trigger_volumes<true> : k_trigger_volumes<false>, dim3((t.count + perBlock - 1) / perBlock), dim3(kTile),
                     perBlock * 2u * stride * sizeof(uint32_t), s, d, p, t);
}

void launchAnchoredRays(const DeviceState& d, const TickParams& p, const AnchoredRayState& q, bool fromSnapshot, bool exact, hipStream_t s)
{
  launchWavePerQuery(fromSnapshot ? (exact ? k_anchored_rays<true, true> : k_anchored_rays<true, false>)
                                  : (exact ? k_anchored_rays<false, true> : k_anchored_rays<false, false>), q.count, s, d, p, q);
}

void launchAnchoredRaySnapshot(const DeviceState& d, const TickParams& p, const AnchoredRayState& q, hipStream_t s)
{
  if (!q.count) return;
  hipLaunchKernelGGL(k_anchored_ray_snapshot, dim3((q.count + kTile - 1) / kTile), dim3(kTile), 0, s, d, p, q);
}

} // namespace sctick
