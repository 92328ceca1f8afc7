// sc_tick_pair_manifolds.hip -- pair manifolds: up to four contact points per entry of the touching list (own spec, include/sc_tick.h
// "pair manifolds").
//
// Opt-in (scTickSetPairManifolds), two launches behind the contact records of sc_tick_pair_shapes.hip and before that file's
// k_pair_shapes_finish, which zeroes the list's running count: the grids are fixed by the list's capacity and the entry count is read on
// the device, so the launches replay unchanged from a captured graph.
//
//   k_pair_manifolds          a thread per entry of the touching list: the entry's contact by the shared routines
//                             (sc_tick_pair_contacts.h), then one of three rules -- a capsule's stretch on a box face, two capsules'
//                             shared stretch, a box's incident face clipped to the other's reference face -- and five float4 stores
//   k_pair_manifolds_finish   one thread: the tick's report (ScTickPairManifoldInfo), the running counts back to zero
//
// A translation unit of its own: the kernels of sc_tick_pair_shapes.hip keep their instruction streams whatever is added here.  Every
// loop has a fixed trip count; every index into the entity arrays is below the entity count, every index into the list below its
// capacity, every slot of the clip polygon below eight.  Plain HIP atomics and vector stores only.  All arithmetic is fp32, unfused, left
// to right, as the header states it operation by operation.
#include "sc_tick_internal.h"
#include "sc_tick_pair_contacts.h"

namespace sctick {

namespace {

// ---- pair manifolds (include/sc_tick.h "pair manifolds"): up to four points and depths of every entry of the touching list ----
// The rules restate the header's text operation by operation over the contact routines above, which hand out the intermediate values the
// text names.  A record starts as SINGLE -- the contact's own point and depth -- and a SEGMENT or FACE rule replaces it when it keeps a
// point.  No register array is indexed by a run-time value: the clip polygon lives in LDS, everything else goes through select chains.
struct Manifold { float p[4][3]; float depth[4]; uint32_t count, kind; };

// a or b, field by field (a select between the two structs themselves would take their addresses and put both into scratch)
__device__ __forceinline__ Member pickMember(bool first, const Member& a, const Member& b)
{
  Member m;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int i = 0; i < 3; ++i) m.c[k][i] = first ? a.c[k][i] : b.c[k][i];
    m.T[k] = first ? a.T[k] : b.T[k]; m.n[k] = first ? a.n[k] : b.n[k];
  }
  m.s = make_float4(first ? a.s.x : b.s.x, first ? a.s.y : b.s.y, first ? a.s.z : b.s.z, first ? a.s.w : b.s.w);
  m.type = first ? a.type : b.type; m.ok = first ? a.ok : b.ok;
  return m;
}

__device__ __forceinline__ int next3(int k) { return (k == 2) ? 0 : k + 1; }

// SEGMENT, a capsule on a box face: the centre line's parameter interval clipped to the face's two side slabs, its ends kept while they
// are within R of the face
__device__ __forceinline__ void manifoldRoundBox(const Member& mx, const RoundBoxParts& rp, const Contact& c, Manifold& m)
{
  if (!rp.segment) return;
  int kf = rp.kd;
  if (!(c.kind & kContactDeep)) {
    const bool o0 = rp.y[0] != rp.q[0], o1 = rp.y[1] != rp.q[1], o2 = rp.y[2] != rp.q[2];
    if ((int)o0 + (int)o1 + (int)o2 != 1) return;           // the closest box feature is an edge or a vertex
    kf = o0 ? 0 : (o1 ? 1 : 2);
  }
  const Frame fr = frameOf(mx);
  const float sg = signOf(sel3(kf, rp.y[0], rp.y[1], rp.y[2]));
  float lo = 0.0f, hi = 1.0f;
  bool empty = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k == kf) continue;
    if (rp.dy[k] != 0.0f) {
      const float b0 = (fr.H[k] - rp.y0[k]) / rp.dy[k], b1 = ((-fr.H[k]) - rp.y0[k]) / rp.dy[k];
      const float tl = (b1 < b0) ? b1 : b0, th = (b1 < b0) ? b0 : b1;
      lo = (tl > lo) ? tl : lo;
      hi = (th < hi) ? th : hi;
    } else if (fabsf(rp.y0[k]) > fr.H[k]) empty = true;
  }
  if (empty || !(lo <= hi)) return;
  const float yk0 = sel3(kf, rp.y0[0], rp.y0[1], rp.y0[2]), dyk = sel3(kf, rp.dy[0], rp.dy[1], rp.dy[2]);
  const float hk = sel3(kf, fr.H[0], fr.H[1], fr.H[2]);
  // an end is R deep along the face's normal only where the line through it leaves the round at R: a centre line that lies flat on the
  // face (to within kManifoldFlat), or a true end of it that the normal leaves on the far side of the segment
  const float dd = (rp.dy[0] * rp.dy[0] + rp.dy[1] * rp.dy[1]) + rp.dy[2] * rp.dy[2];
  const bool flat = rp.R * (dyk * dyk) <= kManifoldFlat * dd;
  const float lean = sg * dyk;
  Manifold o;
  o.count = 0u;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const float t = e ? hi : lo;
    const float yk = yk0 + dyk * t;
    const float up = sg * yk;
    const float pen = rp.R - (up - hk);
    const bool outward = e ? (t == 1.0f && lean <= 0.0f) : (t == 0.0f && lean >= 0.0f);
    // on the line through the centre-line point along the face's normal the round is [-R, R], the box [least - 2H, least]
    const float least = hk - up, back = least - (hk + hk);
    const float l = (back < -rp.R) ? -rp.R : back, h = (least < rp.R) ? least : rp.R;
    const float mid = (l + h) * 0.5f;
    const bool keep = pen >= 0.0f && (flat || outward) && l <= h && (e == 0 || hi != lo);      // (l > h: the end lies beyond the opposite face)
    float x[3], pt[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = (k == kf) ? yk + sg * mid : rp.y0[k] + rp.dy[k] * t;
    fromFrame(fr, mx.T, x, pt);
    if (keep) {
      const bool first = o.count == 0u;
#pragma unroll
      for (int i = 0; i < 3; ++i) { if (first) o.p[0][i] = pt[i]; else o.p[1][i] = pt[i]; }
      if (first) o.depth[0] = pen; else o.depth[1] = pen;
      ++o.count;
    }
  }
  if (!o.count) return;
  m.count = o.count; m.kind = kManifoldSegment;
#pragma unroll
  for (int i = 0; i < 3; ++i) { m.p[0][i] = o.p[0][i]; m.p[1][i] = (o.count > 1u) ? o.p[1][i] : 0.0f; }
  m.depth[0] = o.depth[0]; m.depth[1] = (o.count > 1u) ? o.depth[1] : 0.0f;
}

// SEGMENT, capsule on capsule: the two ends of segment 2 projected onto segment 1 -- each candidate pairs an end of one segment with its
// closest point on the other -- and kept while the rounds overlap there
__device__ __forceinline__ void manifoldRoundRound(const Member& ma, const Member& mb, const Contact& ct, Manifold& m)
{
  const Round ra = roundOf(ma), rb = roundOf(mb);
  const bool segA = ra.A[0] != 0.0f || ra.A[1] != 0.0f || ra.A[2] != 0.0f, segB = rb.A[0] != 0.0f || rb.A[1] != 0.0f || rb.A[2] != 0.0f;
  if (!(segA && segB)) return;
  float p1[3], d1[3], p2[3], d2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    p1[i] = ma.T[i] - ra.A[i]; d1[i] = ra.A[i] + ra.A[i];
    p2[i] = mb.T[i] - rb.A[i]; d2[i] = rb.A[i] + rb.A[i];
  }
  const float a = dot3(d1, d1), e = dot3(d2, d2);
  const float sum = ra.R + rb.R;
  Manifold o;
  o.count = 0u;
  float s0 = 0.0f;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    float g[3], r[3], pa[3], w[3], v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { g[i] = c ? p2[i] + d2[i] : p2[i]; r[i] = g[i] - p1[i]; }
    const float sraw = dot3(r, d1) / a;
    const float s = clamp01(sraw);
    const bool within = s == sraw;                           // the end of segment 2 projects into segment 1: it is the partner itself
#pragma unroll
    for (int i = 0; i < 3; ++i) { pa[i] = p1[i] + d1[i] * s; w[i] = pa[i] - p2[i]; }
    const float t = clamp01(dot3(w, d2) / e);
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = pa[i] - (within ? g[i] : p2[i] + d2[i] * t);
    const float dist2 = dot3(v, v);
    const float dist = sqrtf(dist2);
    const float pen = sum - dist;
    // kept where the candidate's own direction is the contact's normal and the line through the pair leaves either round at its radius:
    // at right angles to its centre line, each to within kManifoldFlat, or through a true end on the far side of the segment
    float wv[3], wn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { wv[i] = (-v[i]) / dist; wn[i] = wv[i] - ct.n[i]; }
    const float c1 = dot3(wv, d1), c2 = dot3(wv, d2);
    const float tp = within ? (c ? 1.0f : 0.0f) : t;
    const bool freeA = (s == 0.0f && c1 <= 0.0f) || (s == 1.0f && c1 >= 0.0f) || (ra.R * (c1 * c1) <= kManifoldFlat * a);
    const bool freeB = (tp == 0.0f && c2 >= 0.0f) || (tp == 1.0f && c2 <= 0.0f) || (rb.R * (c2 * c2) <= kManifoldFlat * e);
    const bool keep = pen >= 0.0f && dist2 > 0.0f && sum * dot3(wn, wn) <= kManifoldFlat && freeA && freeB && (c == 0 || s != s0);
    if (c == 0) s0 = s;
    const float far = dist + rb.R, near = dist - rb.R;
    const float hi = (far < ra.R) ? far : ra.R, lo = (near < -ra.R) ? -ra.R : near;
    const float mid = (lo + hi) * 0.5f;
    if (keep) {
      const bool first = o.count == 0u;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float pt = pa[i] + wv[i] * mid;
        if (first) o.p[0][i] = pt; else o.p[1][i] = pt;
      }
      if (first) o.depth[0] = pen; else o.depth[1] = pen;
      ++o.count;
    }
  }
  if (!o.count) return;
  m.count = o.count; m.kind = kManifoldSegment;
#pragma unroll
  for (int i = 0; i < 3; ++i) { m.p[0][i] = o.p[0][i]; m.p[1][i] = (o.count > 1u) ? o.p[1][i] : 0.0f; }
  m.depth[0] = o.depth[0]; m.depth[1] = (o.count > 1u) ? o.depth[1] : 0.0f;
}

// The clip polygon of one lane: two buffers of eight vertices (p, q, z) in the reference frame, laid out [buffer][slot][component][lane]
// so that the 64 lanes of the wave read and write 64 consecutive words -- one per bank -- whatever slot each lane's cursor is at.
constexpr uint32_t kPolySlots = 8, kPolyWords = 2u * kPolySlots * 3u * kManifoldWave;
__device__ __forceinline__ float& polyAt(float* poly, uint32_t buf, uint32_t slot, uint32_t comp)
{
  return poly[((buf * kPolySlots + (slot & (kPolySlots - 1u))) * 3u + comp) * kManifoldWave];      // (poly already points at the lane's column)
}

// FACE: the other box's incident face clipped to the side planes of the reference face (Sutherland-Hodgman, the planes and the vertices
// in a fixed order), the vertices at or below the reference face kept, four of them chosen when more are
__device__ __forceinline__ void manifoldFace(const Member& ma, const Member& mb, const Contact& c, const BoxBoxParts& bp, float* poly, Manifold& m)
{
  const Frame fa = frameOf(ma), fb = frameOf(mb);
  const bool ofB = (c.kind & 0xFFu) == kContactBoxFaceB;
  Frame fo, ft; float To[3], Tt[3];                          // the reference box and the other one
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    fo.H[k] = ofB ? fb.H[k] : fa.H[k]; ft.H[k] = ofB ? fa.H[k] : fb.H[k];
    To[k] = ofB ? mb.T[k] : ma.T[k]; Tt[k] = ofB ? ma.T[k] : mb.T[k];
#pragma unroll
    for (int i = 0; i < 3; ++i) { fo.u[k][i] = ofB ? fb.u[k][i] : fa.u[k][i]; ft.u[k][i] = ofB ? fa.u[k][i] : fb.u[k][i]; }
  }
  const int ax = ofB ? bp.bj : bp.bi, a1 = next3(ax), a2 = next3(a1);
  const float sr = ofB ? -bp.sg : bp.sg;                    // the reference face is the one at sr * H along the axis
  // the incident face: the other box's axis most along the normal (the first of the largest), on the side that faces the reference box
  float cm = dot3(c.n, ft.u[0]), big = fabsf(cm);
  int mi = 0;
#pragma unroll
  for (int k = 1; k < 3; ++k) {
    const float ck = dot3(c.n, ft.u[k]);
    if (fabsf(ck) > big) { big = fabsf(ck); cm = ck; mi = k; }
  }
  const float sm = ((cm < 0.0f) != ofB) ? 1.0f : -1.0f;
  const int m1 = next3(mi);
  const float Hp = sel3(a1, fo.H[0], fo.H[1], fo.H[2]), Hq = sel3(a2, fo.H[0], fo.H[1], fo.H[2]), Hr = sel3(ax, fo.H[0], fo.H[1], fo.H[2]);
#pragma unroll
  for (int j = 0; j < 4; ++j) {                              // its vertices (+, +), (-, +), (-, -), (+, -) over the axes after mi
    const float s1 = (j == 0 || j == 3) ? 1.0f : -1.0f, s2 = (j < 2) ? 1.0f : -1.0f;
    float g[3], v[3], r[3], x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = ((k == mi) ? sm : ((k == m1) ? s1 : s2)) * ft.H[k];
    fromFrame(ft, Tt, g, v);
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = v[i] - To[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = dot3(r, fo.u[k]);
    polyAt(poly, 0u, j, 0u) = sel3(a1, x[0], x[1], x[2]);
    polyAt(poly, 0u, j, 1u) = sel3(a2, x[0], x[1], x[2]);
    polyAt(poly, 0u, j, 2u) = sr * sel3(ax, x[0], x[1], x[2]);
  }
  uint32_t n = 4u;
#pragma unroll
  for (uint32_t pl = 0; pl < 4u; ++pl) {                     // p <= Hp, p >= -Hp, q <= Hq, q >= -Hq
    const uint32_t comp = pl >> 1, src = pl & 1u, dst = src ^ 1u;
    const bool upper = (pl & 1u) == 0u;
    const float hside = comp ? Hq : Hp;
    const float hv = upper ? hside : -hside;
    const uint32_t last = n ? n - 1u : 0u;
    float pv[3] = { polyAt(poly, src, last, 0u), polyAt(poly, src, last, 1u), polyAt(poly, src, last, 2u) };
    uint32_t cnt = 0u;
#pragma unroll
    for (uint32_t i = 0; i < kPolySlots; ++i) {
      if (i < n) {
        const float cur[3] = { polyAt(poly, src, i, 0u), polyAt(poly, src, i, 1u), polyAt(poly, src, i, 2u) };
        const float xc = comp ? cur[1] : cur[0], xp = comp ? pv[1] : pv[0];
        const bool inC = upper ? (xc <= hv) : (xc >= hv), inP = upper ? (xp <= hv) : (xp >= hv);
        if (inC != inP) {
          const float t = (hv - xp) / (xc - xp);
          if (cnt < kPolySlots) {
#pragma unroll
            for (uint32_t k = 0; k < 3u; ++k) polyAt(poly, dst, cnt, k) = pv[k] + (cur[k] - pv[k]) * t;
            ++cnt;
          }
        }
        if (inC && cnt < kPolySlots) {
#pragma unroll
          for (uint32_t k = 0; k < 3u; ++k) polyAt(poly, dst, cnt, k) = cur[k];
          ++cnt;
        }
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) pv[k] = cur[k];
      }
    }
    n = cnt;
  }
  // (four passes: the polygon is back in buffer 0)  kept: at or below the reference face, not below the reference box, and the point --
  // halfway up to the reference face -- within kManifoldSkin of the other box
  uint32_t mask = 0u;
#pragma unroll
  for (uint32_t i = 0; i < kPolySlots; ++i) {
    const float p = polyAt(poly, 0u, i, 0u), q = polyAt(poly, 0u, i, 1u), z = polyAt(poly, 0u, i, 2u);
    const float pen = Hr - z;
    const float zz = sr * (z + pen * 0.5f);
    float x[3], pt[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = (k == a1) ? p : ((k == a2) ? q : zz);
    fromFrame(fo, To, x, pt);
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = pt[k] - Tt[k];
    bool inside = z >= -Hr;
#pragma unroll
    for (int k = 0; k < 3; ++k) inside = inside && (fabsf(dot3(r, ft.u[k])) - ft.H[k] <= kManifoldSkin);
    if (i < n && pen >= 0.0f && inside) mask |= 1u << i;
  }
  uint32_t kept = 0u, c0 = 0u, c1 = 0u, c2 = 0u, c3 = 0u;
#pragma unroll
  for (uint32_t i = 0; i < kPolySlots; ++i) {
    if ((mask >> i) & 1u) {
      if (kept == 0u) c0 = i; else if (kept == 1u) c1 = i; else if (kept == 2u) c2 = i; else if (kept == 3u) c3 = i;
      ++kept;
    }
  }
  if (!kept) return;
  uint32_t count = kept, kind = kManifoldFace;
  if (kept > 4u) {
    kind |= kManifoldReduced;
    // the deepest; the one farthest from it in the face; the largest area on either side of the line through the two
    bool first = true;
    float best = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < kPolySlots; ++i) {
      const float pen = Hr - polyAt(poly, 0u, i, 2u);
      if (((mask >> i) & 1u) && (first || pen > best)) { best = pen; c0 = i; first = false; }
    }
    const float pa = polyAt(poly, 0u, c0, 0u), qa = polyAt(poly, 0u, c0, 1u);
    first = true;
#pragma unroll
    for (uint32_t i = 0; i < kPolySlots; ++i) {
      const float dp = polyAt(poly, 0u, i, 0u) - pa, dq = polyAt(poly, 0u, i, 1u) - qa;
      const float d2 = dp * dp + dq * dq;
      if (((mask >> i) & 1u) && (first || d2 > best)) { best = d2; c1 = i; first = false; }
    }
    const float ex = polyAt(poly, 0u, c1, 0u) - pa, ey = polyAt(poly, 0u, c1, 1u) - qa;
    float most = 0.0f, least = 0.0f;
    bool left = false, right = false;
    uint32_t cl = 0u, cr = 0u;
#pragma unroll
    for (uint32_t i = 0; i < kPolySlots; ++i) {
      const float area = ex * (polyAt(poly, 0u, i, 1u) - qa) - ey * (polyAt(poly, 0u, i, 0u) - pa);
      if ((mask >> i) & 1u) {
        if (area > most) { most = area; cl = i; left = true; }
        if (area < least) { least = area; cr = i; right = true; }
      }
    }
    c2 = left ? cl : cr; c3 = cr;
    count = 2u + (left ? 1u : 0u) + (right ? 1u : 0u);
  }
  m.count = count; m.kind = kind;
#pragma unroll
  for (uint32_t s = 0; s < 4u; ++s) {
    const uint32_t i = (s == 0u) ? c0 : ((s == 1u) ? c1 : ((s == 2u) ? c2 : c3));
    const float p = polyAt(poly, 0u, i, 0u), q = polyAt(poly, 0u, i, 1u), z = polyAt(poly, 0u, i, 2u);
    const float pen = Hr - z;
    const float zz = sr * (z + pen * 0.5f);
    float x[3], pt[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = (k == a1) ? p : ((k == a2) ? q : zz);
    fromFrame(fo, To, x, pt);
    const bool live = s < count;
#pragma unroll
    for (int k = 0; k < 3; ++k) m.p[s][k] = live ? pt[k] : 0.0f;
    m.depth[s] = live ? pen : 0.0f;
  }
}

// A thread per entry of the touching list, as k_pair_contacts: the grid by the list's capacity, the entry count read here.  One wave per
// workgroup, so the LDS a workgroup takes is its 64 polygons (12 KB).  Tallies by ballot, one atomic per counter and wave.
__global__ __launch_bounds__(kManifoldWave) void k_pair_manifolds(const DeviceState d, const PairShapeState e, const PairManifoldState f, uint32_t count,
                                                                  uint32_t rankBits)
{
  __shared__ float polygons[kPolyWords];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t listed = e.ctl[kPsTouching];
  const uint32_t room = e.maxTouching < f.maxTouching ? e.maxTouching : f.maxTouching;
  const uint32_t n = listed < room ? listed : room;
  uint32_t tally[6] = { 0u, 0u, 0u, 0u, 0u, 0u };          // (wave-uniform) kPmOne .. kPmReduced
  const uint32_t stride = gridDim.x * kManifoldWave;
  for (uint32_t base = blockIdx.x * kManifoldWave; base < n; base += stride) {      // (wave-uniform trip count)
    const uint32_t i = base + lane;
    const bool live = i < n;
    Manifold m;
#pragma unroll
    for (int s = 0; s < 4; ++s) { m.p[s][0] = m.p[s][1] = m.p[s][2] = 0.0f; m.depth[s] = 0.0f; }
    m.count = 0u; m.kind = kManifoldNone;
    if (live) {
      const uint2 pr = e.list[i];
      const Member ma = fetchMember(d, pr.x, count, rankBits), mb = fetchMember(d, pr.y, count, rankBits);
      if (ma.ok && mb.ok) {
        const bool boxA = ma.type == kColliderBox, boxB = mb.type == kColliderBox;
        Contact c;
        if (boxA && boxB) {
          BoxBoxParts bp;
          c = contactBoxBox(ma, mb, &bp);
          m.count = 1u; m.kind = kManifoldSingle; m.p[0][0] = c.p[0]; m.p[0][1] = c.p[1]; m.p[0][2] = c.p[2]; m.depth[0] = c.depth;
          if (c.kind != kContactBoxEdge) manifoldFace(ma, mb, c, bp, polygons + lane, m);
        } else if (boxA || boxB) {
          RoundBoxParts rp;
          const Member mr = pickMember(boxA, mb, ma), mx = pickMember(boxA, ma, mb);      // the round and the box: one routine, once
          c = contactRoundBox(mr, mx, !boxA, &rp);
          m.count = 1u; m.kind = kManifoldSingle; m.p[0][0] = c.p[0]; m.p[0][1] = c.p[1]; m.p[0][2] = c.p[2]; m.depth[0] = c.depth;
          manifoldRoundBox(mx, rp, c, m);
        } else {
          c = contactRoundRound(ma, mb);
          m.count = 1u; m.kind = kManifoldSingle; m.p[0][0] = c.p[0]; m.p[0][1] = c.p[1]; m.p[0][2] = c.p[2]; m.depth[0] = c.depth;
          if (!(c.kind & kContactDegenerate)) manifoldRoundRound(ma, mb, c, m);
        }
      }
      float4* out = f.rec + 5u * (size_t)i;
      out[0] = make_float4(m.p[0][0], m.p[0][1], m.p[0][2], m.p[1][0]);
      out[1] = make_float4(m.p[1][1], m.p[1][2], m.p[2][0], m.p[2][1]);
      out[2] = make_float4(m.p[2][2], m.p[3][0], m.p[3][1], m.p[3][2]);
      out[3] = make_float4(m.depth[0], m.depth[1], m.depth[2], m.depth[3]);
      out[4] = make_float4(__uint_as_float(m.count), __uint_as_float(m.kind), 0.0f, 0.0f);
    }
    tally[kPmOne] += (uint32_t)__popcll(ballot64(live && m.count == 1u));
    tally[kPmTwo] += (uint32_t)__popcll(ballot64(live && m.count == 2u));
    tally[kPmThree] += (uint32_t)__popcll(ballot64(live && m.count == 3u));
    tally[kPmFour] += (uint32_t)__popcll(ballot64(live && m.count == 4u));
    tally[kPmFace] += (uint32_t)__popcll(ballot64(live && (m.kind & 0xFFu) == kManifoldFace));
    tally[kPmReduced] += (uint32_t)__popcll(ballot64(live && (m.kind & kManifoldReduced) != 0u));
  }
  if (lane == 0) {
#pragma unroll
    for (uint32_t j = 0; j < 6u; ++j) if (tally[j]) atomicAdd(&f.ctl[j], tally[j]);
  }
}

// one thread behind k_pair_manifolds: the tick's report (ScTickPairManifoldInfo), the counts back to zero
__global__ __launch_bounds__(64) void k_pair_manifolds_finish(const PairShapeState e, const PairManifoldState f)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const uint32_t listed = e.ctl[kPsTouching];
  const uint32_t room = e.maxTouching < f.maxTouching ? e.maxTouching : f.maxTouching;
  const uint32_t one = f.ctl[kPmOne], two = f.ctl[kPmTwo], three = f.ctl[kPmThree], four = f.ctl[kPmFour];
  f.info[0] = listed < room ? listed : room;
  f.info[1] = ((one + 2u * two) + 3u * three) + 4u * four;
  f.info[2] = one; f.info[3] = two; f.info[4] = three; f.info[5] = four;
  f.info[6] = f.ctl[kPmFace]; f.info[7] = f.ctl[kPmReduced];
#pragma unroll
  for (uint32_t j = 0; j < 6u; ++j) f.ctl[j] = 0u;
}

} // namespace

void launchPairManifolds(const DeviceState& d, const TickParams& p, const PairShapeState& list, const PairManifoldState& manifolds, hipStream_t s)
{
  // a thread per entry the list can hold (grid-stride beyond the cap), a wave per workgroup
  const uint32_t blocks = std::min(std::max((list.maxTouching + kManifoldWave - 1u) / kManifoldWave, 1u), 8192u);
  hipLaunchKernelGGL(k_pair_manifolds, dim3(blocks), dim3(kManifoldWave), 0, s, d, list, manifolds, p.n, p.rankBits);
  hipLaunchKernelGGL(k_pair_manifolds_finish, dim3(1), dim3(64), 0, s, list, manifolds);
}

} // namespace sctick
