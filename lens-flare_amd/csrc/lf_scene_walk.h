// lf_scene_walk.h -- the scene's ray / primitive tests and the walk over its tree, shared by the scene-radiance term
// (lf_scene.hip: closest hits and shadow rays of the integrator) and by the ghost march's occlusion test (lf_march_common.h:
// the any-hit walk of a lit ghost ray, lf_set_ghost_occlusion): ONE definition of the double-precision tests
// (scene/sphere.cpp:11-111, scene/triangle.cpp:25-112, scene/bvh.cpp:201-222), so that a ghost's shadow ray and the scene image
// decide "blocked" by the same bits.  Device code only; nothing here is part of the ABI.
#pragma once

#include "lf_internal.h"

namespace lfw {

struct V3 { double x, y, z; };
__host__ __device__ inline V3 v3(double x, double y, double z) { V3 r{x, y, z}; return r; }
__host__ __device__ inline V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__host__ __device__ inline V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__host__ __device__ inline V3 operator*(V3 a, double c) { return v3(a.x * c, a.y * c, a.z * c); }
__host__ __device__ inline V3 operator*(double c, V3 a) { return v3(c * a.x, c * a.y, c * a.z); }
__host__ __device__ inline V3 mulv(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
// dot(): (x*x' + y*y') + z*z' (the AVX build's _mm_dp_pd pairs x,y first; vector3D.h:256-262)
__host__ __device__ inline double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__host__ __device__ inline V3 cross(V3 u, V3 v) {
  return v3(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
}
__device__ inline double norm(V3 a) { return sqrt(dot(a, a)); }
// Vector3D::unit(): multiply by 1/norm (vector3D.h:214-217); operator/(double) does the same
__device__ inline V3 unit(V3 a) { double rn = 1. / norm(a); return a * rn; }
__device__ inline V3 divs(V3 a, double c) { const double rc = 1.0 / c; return v3(rc * a.x, rc * a.y, rc * a.z); }

// A ray as the traversal keeps it: the reference's Ray (o, d, min_t, max_t in double: every primitive
// test uses exactly these) plus what the box tests use -- floats that BRACKET the doubles.
struct DRay {
  V3 o, d; double min_t, max_t;
  float olx, oly, olz, ohx, ohy, ohz;  // floats strictly below / above o
  float ix, iy, iz;                    // 1 / d; NaN when |1 / d| is no finite float: the axis then never culls
  float tmin_c, tmax_c;                // min_t / max_t, widened by the box test's slack
};
// the closest hit so far: primitive + what its test produced; the normal is formed ONCE, at the end
struct Hit { double t, b1, b2; int prim; };

__device__ inline float f32_down(double x) { const float f = (float)x; return (double)f > x ? nextafterf(f, -INFINITY) : f; }
__device__ inline float f32_up(double x) { const float f = (float)x; return (double)f < x ? nextafterf(f, INFINITY) : f; }
// STRICTLY below / above: the origin's bracket.  With a direction component of exactly 0 the slab
// products are (lo - oh) * inf and (hi - ol) * inf; a difference of exactly 0 gives NaN, which the
// min / max of box_miss resolve towards "outside".  That is only right if a zero difference MEANS
// outside: lo == oh > o does, lo == oh == o (an origin exactly on the slab's plane, e.g. a shadow ray
// leaving an axis-aligned face along an axis) would not.
__device__ inline float f32_below(double x) { const float f = (float)x; return (double)f >= x ? nextafterf(f, -INFINITY) : f; }
__device__ inline float f32_above(double x) { const float f = (float)x; return (double)f <= x ? nextafterf(f, INFINITY) : f; }
__device__ inline float inv_dir(double d) {
  const double q = 1.0 / d;           // d = 0: +-inf, which culls correctly (a ray parallel to a slab)
  return (d != 0.0 && fabs(q) > 3.0e38) ? __int_as_float(0x7fc00000) : (float)q;
}
// max_t shrinks with every accepted hit: the float bound follows (2^-20 relative + 1e-30 absolute:
// four times what the box test's own rounding can be off, see box_miss)
__device__ inline void widen_max_t(DRay& r) {
  const float m = f32_up(r.max_t);
  r.tmax_c = fmaf(9.6e-7f, fabsf(m), m) + 1e-30f;
}
__device__ inline DRay make_ray(V3 o, V3 d, double min_t, double max_t) {
  DRay r;
  r.o = o; r.d = d; r.min_t = min_t; r.max_t = max_t;
  r.olx = f32_below(o.x); r.oly = f32_below(o.y); r.olz = f32_below(o.z);
  r.ohx = f32_above(o.x); r.ohy = f32_above(o.y); r.ohz = f32_above(o.z);
  r.ix = inv_dir(d.x); r.iy = inv_dir(d.y); r.iz = inv_dir(d.z);
  const float m = f32_down(min_t);
  r.tmin_c = fmaf(-9.6e-7f, fabsf(m), m) - 1e-30f;
  widen_max_t(r);
  return r;
}

// ---- primitives ------------------------------------------------------------------------------
// Sphere::test + intersect (scene/sphere.cpp:11-111)
__device__ inline bool hit_sphere(const LfPrim& s, int idx, DRay& r, Hit* h) {
  const V3 c = v3(s.d[0], s.d[1], s.d[2]);
  const V3 oc = r.o - c;
  const double a = dot(r.d, r.d);
  const double b = 2 * dot(oc, r.d);
  const double cc = dot(oc, oc) - s.d[4];
  double t1;
  if (b * b < 4.0 * a * cc) return false;
  if (b * b == 4.0 * a * cc) {
    const double root = (-b) / (2.0 * a);
    if (root < r.min_t || root > r.max_t) return false;
    t1 = root;
  } else {
    const double q = sqrt(b * b - 4.0 * a * cc);
    const double r1 = (-b - q) / (2.0 * a), r2 = (-b + q) / (2.0 * a);
    const double p1 = r2 < r1 ? r2 : r1, p2 = r1 < r2 ? r2 : r1;  // std::min / std::max
    if (p1 > r.max_t || p2 < r.min_t) return false;
    if (p1 < r.min_t) {
      if (p2 > r.max_t) return false;
      t1 = p2;
    } else {
      t1 = p1;
    }
  }
  r.max_t = t1;
  if (h) { h->t = t1; h->prim = idx; }
  return true;
}

// moller_trumbore + is_valid_intersection + Triangle::intersect (scene/triangle.cpp:25-112)
__device__ inline bool hit_triangle(const LfPrim& t, int idx, DRay& r, Hit* h) {
  // (e1 = p1 - p0 and e2 = p2 - p0 come with the primitive: the host's IEEE subtraction gives the bits
  // the device's would, and the test holds 6 doubles less)
  const V3 p0 = v3(t.d[0], t.d[1], t.d[2]), e1 = v3(t.d[3], t.d[4], t.d[5]), e2 = v3(t.d[6], t.d[7], t.d[8]);
  const V3 s = r.o - p0;
  const V3 s1 = cross(r.d, e2), s2 = cross(s, e1);
  const double rc = 1. / dot(s1, e1);  // operator/= multiplies by the reciprocal
  const double tt = dot(s2, e2) * rc, b1 = dot(s1, s) * rc, b2 = dot(s2, r.d) * rc;
  if (tt < r.min_t || tt > r.max_t) return false;
  if (b1 < 0 || b1 > 1) return false;
  if (b2 < 0 || b2 > 1) return false;
  if (b1 + b2 > 1) return false;
  r.max_t = tt;
  if (h) { h->t = tt; h->b1 = b1; h->b2 = b2; h->prim = idx; }
  return true;
}

// BBox::intersect (scene/bbox.cpp:12-49) as a conservative float test: true only when the DOUBLE ray
// provably misses the DOUBLE box or leaves it outside [min_t, max_t].
//   (lo - oh) <= lo - o and (hi - ol) >= hi - o exactly (box rounded outward, origin bracketed), so
//   after the multiplication by 1 / d the smaller product bounds the entry from below and the larger
//   one the exit from above, each off by at most 3 roundings (2^-24 each, relative) + underflow.
// tn > tf is decided with 2^-21 (|tn| + |tf|) + 1e-30 of slack, the two ends against bounds that were
// widened once per ray (make_ray / widen_max_t).  fminf / fmaxf drop NaNs: an axis without a usable
// reciprocal (both products NaN) simply does not cull; 0 * inf only arises for an origin strictly
// outside the slab of an axis the ray is parallel to (f32_below / f32_above), where the surviving
// infinite product culls, correctly.  The sum of the
// magnitudes is clamped so that an infinite entry (a ray parallel to a slab and outside it) still
// compares as "misses" instead of inf > inf.
__device__ inline bool box_miss(const DRay& r, float lx, float ly, float lz, float hx, float hy, float hz,
                                float* entry) {
  const float ax = (lx - r.ohx) * r.ix, bx = (hx - r.olx) * r.ix;
  const float ay = (ly - r.ohy) * r.iy, by = (hy - r.oly) * r.iy;
  const float az = (lz - r.ohz) * r.iz, bz = (hz - r.olz) * r.iz;
  const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
  const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
  const float mag = fminf(fabsf(tn) + fabsf(tf), 3.0e38f);
  *entry = tn;
  return (tn - tf > fmaf(4.8e-7f, mag, 1e-30f)) || tf < r.tmin_c || tn > r.tmax_c;
}

// closest hit (BVHAccel::intersect, scene/bvh.cpp:201-222: the recursion shrinks r.max_t as it goes,
// so whatever the visiting order the last accepted primitive is the closest one).  h == nullptr is
// the shadow-ray query (has_intersection): the first accepted primitive settles it.
// A node visit tests the boxes of both children (LfBvhNode) and descends into the nearer one first:
// the nearer subtree usually holds the closest hit, which then culls the farther one when it is
// popped.  The stack of deferred children holds one entry per level at most (the host refuses deeper
// trees); entry i of a lane lies at stack[STRIDE * i]: in the scene kernels in LDS ([depth][thread],
// STRIDE = their 256 threads: conflict-free), not in scratch memory; in the ghost march's occlusion test
// (STRIDE = 1) a lane's own array.
constexpr int kStackDepth = 24;
// what the reference's BVHAccel counts for its end-of-frame log (bvh.h:85,105; bvh.cpp:211;
// raytraced_renderer.cpp:706-709): rays handed to intersect() / has_intersection(), and primitive tests of
// the closest-hit queries (has_intersection does not count its tests) -- here per lane, summed at the
// kernel's end (lf_get_scene_counters)
struct SceneTally { unsigned rays, isects; };
template <int STRIDE = 256>
__device__ bool closest_hit(const LfSceneDev& sc, DRay& r, Hit* h, int* __restrict__ stack /* [kStackDepth][STRIDE] + tid */,
                            SceneTally& tally) {
  int sp = 0, cur = 0;
  bool any = false;
  tally.rays++;
  for (;;) {
    if (cur >= 0) {
      const float4* __restrict__ q = reinterpret_cast<const float4*>(sc.nodes + cur);
      const float4 q0 = q[0], q1 = q[1], q2 = q[2];
      const int2 ch = *reinterpret_cast<const int2*>(q + 3);
      float t0, t1;
      const bool m0 = box_miss(r, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, &t0) || ch.x == kLfNoChild;
      const bool m1 = box_miss(r, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, &t1) || ch.y == kLfNoChild;
      if (!m0 && !m1) {
        const bool second_first = t1 < t0;
        stack[STRIDE * sp++] = second_first ? ch.x : ch.y;
        cur = second_first ? ch.y : ch.x;
        continue;
      }
      if (!m0) { cur = ch.x; continue; }
      if (!m1) { cur = ch.y; continue; }
    } else {
      const int code = ~cur, first = code >> 2, count = (code & 3) + 1;
      bool hit_here = false;
      if (h) tally.isects += (unsigned)count;
      for (int i = 0; i < count; i++) {
        const LfPrim& p = sc.prims[first + i];
        const bool hit = p.type == 0 ? hit_sphere(p, first + i, r, h) : hit_triangle(p, first + i, r, h);
        hit_here = hit_here || hit;
      }
      if (hit_here) {
        if (!h) return true;
        any = true;
        widen_max_t(r);
      }
    }
    if (sp == 0) break;
    cur = stack[STRIDE * --sp];
  }
  return any;
}

}  // namespace lfw
