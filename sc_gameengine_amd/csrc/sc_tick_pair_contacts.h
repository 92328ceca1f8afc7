// sc_tick_pair_contacts.h -- the contact routines of the touching pairs (include/sc_tick.h "pair contacts"), shared by k_pair_contacts
// (sc_tick_pair_shapes.hip) and k_pair_manifolds (sc_tick_pair_manifolds.hip).  Device code only; include after sc_tick_internal.h.
// The routines restate the header's text operation by operation, over the same Member / Round / Frame and the same two cores the
// touching decisions go through.  A register array is never indexed by a run-time value: sel3 picks by comparisons.
#pragma once
#include "sc_tick_internal.h"

namespace sctick {

namespace {

struct Contact { float p[3]; float depth; float n[3]; uint32_t kind; };
// what the manifold rules take over from a contact routine besides its record (k_pair_manifolds; null: nothing is handed out)
struct RoundBoxParts { float y0[3], dy[3], y[3], q[3]; float R; int kd; bool segment; };
struct BoxBoxParts { int bi, bj; float sg; };

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

__device__ __forceinline__ Contact contactRoundBox(const Member& mr, const Member& mx, bool roundIsA, RoundBoxParts* parts = nullptr)
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
  if (parts) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { parts->y0[k] = y0[k]; parts->dy[k] = dy[k]; parts->y[k] = y[k]; parts->q[k] = q[k]; }
    parts->R = rd.R; parts->kd = kd; parts->segment = rd.A[0] != 0.0f || rd.A[1] != 0.0f || rd.A[2] != 0.0f;
  }
  return o;
}

__device__ __forceinline__ Contact contactBoxBox(const Member& ma, const Member& mb, BoxBoxParts* parts = nullptr)
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
  if (parts) { parts->bi = bi; parts->bj = bj; parts->sg = sg; }
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

} // namespace

} // namespace sctick
