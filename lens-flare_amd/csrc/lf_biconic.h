// lf_biconic.h -- a biconic interface of the geometric lens (lf_set_lens_biconics; DESIGN.md section 4, "biconic interfaces"):
//   z(x, y) = (cx x^2 + cy y^2) / (1 + sqrt(1 - (1 + kx) cx^2 x^2 - (1 + ky) cy^2 y^2))
// cy the vertex curvature lf_set_lens holds, cx = 1 / Rx of the record (0: flat in x), axes the sensor's x and y: circular
// cylinders (one curvature zero, kx = ky = 0), toroids, the anamorphic flare.  ONE definition of the sag and of the surface
// event for the host (lf_biconic_sag, lf_biconic_event) and the kernels (lf_march_asph.hip), in lf_asphere.h's conventions:
// every multiply-add an explicit fmaf, every root and division the IEEE one, so that both sides agree bit for bit.
// Nothing here is part of the ABI.
#pragma once

#include <cmath>

#include "lf_internal.h"
#include "lf_march_events.h"
#include "lf_asphere.h"

namespace lfm {

// The record of a biconic (interface, direction of travel): the 32-byte slot of the table that an aspheric record would
// occupy (an interface carries one kind or the other), one aligned load, a wave-uniform row constant.
struct alignas(32) LfBicRec {
  float cx, kx, ky;
  float spare[5];
};
static_assert(sizeof(LfBicRec) == sizeof(LfAsphRec), "the aspheric record's slot");

// Newton steps on g(s) = P_z(s) - z(x(s), y(s)) from the start quadric's root.  Fixed: every lane of a wave runs them all.
// Three, measured ("biconic interfaces") over the rays of tests/test_biconics_cpu.py -- 23278 rays that
// float64 accepts clear of the rim and critical-angle bands, on the two cylinder faces of dgauss11_anamorphic.lens and a general
// biconic (cx = 1/45, cy = 1/30, kx = 0.4, ky = -0.6): a count of 0, 1, 2 loses 7667, 595, 1 of them to the criterion, 3 none.
// A cylinder's rays sit on the root at step 0 but for roundings; the worst accepted ray (the general biconic, refraction into
// the glass at incidence cosine 0.14) is 0.50, 2.5e-2, 5.6e-5, 1.1e-6 mm from the root after steps 0 .. 3 and at float32's
// floor, 8e-7, from step 4 on.
constexpr int kBicNewtonSteps = 3;
// The convergence criterion, |g| <= kBicTol * scale with scale = |o_z| + |z_s| + |s| |g'|: lf_asphere.h's derivation for a sag
// of two variables.  The best float s lies within half a spacing of the root and moves g by |g'| eps |s| (eps = 2^-24);
// P_z = fma(s, K_z, o_z) rounds below eps (|o_z| + |s K_z|); z_s carries its root, its quotient, the numerator's fma and
// product and the second fma of the root's argument (where the asphere has its polynomial's), and the roundings of x and
// y, which move it by eps |s| |z_x K_x + z_y K_y| = eps |s| |g' - K_z|: below 4 eps |z_s| + eps |s| |g' - K_z|.  The sum is
// below 4 eps scale; the last Newton step's own quotient and subtraction may leave s one spacing off the best: 8 eps.
constexpr float kBicTol = 4.76837158203125e-7f;   // 2^-21

// z, dz/dx and dz/dy at (x, y); false beyond the conic's domain (the root's argument negative, or a NaN).  With
// root = sqrt(u): z = A / (1 + root), dz/dx = cx x (2 + (z / root) (1 + kx) cx) / (1 + root) -- cx x / root on a sphere.
// A meridian of zero curvature has the slope cx * x = 0 times a finite factor: an exact zero.
__host__ __device__ inline bool lf_bic_sag(float cx, float cy, float kx, float ky, float x, float y, float& z, float& zx,
                                           float& zy) {
  const float x2 = x * x, y2 = y * y;
  const float px = (1.0f + kx) * cx, py = (1.0f + ky) * cy;
  const float u = fmaf(-(px * cx), x2, fmaf(-(py * cy), y2, 1.0f));
  const bool in = u >= 0.0f;
  const float root = sqrtf(in ? u : 0.0f);
  const float den = 1.0f + root;
  z = fmaf(cx, x2, cy * y2) / den;
  const float zr = z / root;
  zx = (cx * x) * (fmaf(zr, px, 2.0f) / den);
  zy = (cy * y) * (fmaf(zr, py, 2.0f) / den);
  return in;
}

// One event of one ray on a biconic interface: lf_asph_event's conventions, arguments and fates (AsphHit).
//   start   the near root of the quadric cx x^2 + cy y^2 + cm z^2 - 2 z = 0, cm the curvature of the larger magnitude:
//           the surface itself for a circular cylinder (kx = ky = 0, one curvature zero), a sphere (cx = cy, kx = ky = 0)
//           and a plane, where the Newton steps then move nothing but roundings;  a s^2 - 2 G s + F = 0 along the ray,
//           s = F / (G + sgn sqrt(G^2 - a F));  the vertex plane, s = -o_z / K_z, where the ray misses the quadric
//   refine  kBicNewtonSteps steps s -= g / g', g' = K_z - z_x K_x - z_y K_y
//   death   beyond the conic's domain at the last point, or |g| above the criterion there: kAsphMissed
//   normal  N = (-z_x, -z_y, 1) / |N|; KN, sq, k2, ct, refraction, reflection and aperture as lf_asph_event's
// A meridian of zero curvature leaves its component of K as it entered, bit for bit (its slope is an exact zero; the
// select keeps a -0.0f's sign too).  A dead lane's ray state is garbage nobody reads again.
__host__ __device__ inline AsphHit lf_bic_event(float& px, float& py, float& hz, float& r2o, float& dx, float& dy, float& dz,
                                                float dzv, float cy, const LfBicRec& k, float delta, float h2, bool reflect,
                                                float sgn) {
  const float cx = k.cx;
  const float oz = hz + dzv;
  float s;
  {
    const float cm = fabsf(cx) >= fabsf(cy) ? cx : cy;
    const float a = fmaf(cx, dx * dx, fmaf(cy, dy * dy, cm * (dz * dz)));
    const float od = fmaf(cx, px * dx, fmaf(cy, py * dy, cm * (oz * dz)));
    const float F = fmaf(cx, px * px, fmaf(cy, py * py, fmaf(cm, oz * oz, -2.0f * oz)));
    const float G = dz - od;
    const float disc = fmaf(G, G, -(a * F));
    s = disc >= 0.0f ? F / fmaf(sgn, sqrtf(disc), G) : -oz / dz;
  }
  float x, y, z, zs, zx, zy, gp;
  bool in;
#pragma unroll
  for (int it = 0; it <= kBicNewtonSteps; it++) {
    x = fmaf(s, dx, px); y = fmaf(s, dy, py); z = fmaf(s, dz, oz);
    in = lf_bic_sag(cx, cy, k.kx, k.ky, x, y, zs, zx, zy);
    gp = fmaf(-zx, dx, fmaf(-zy, dy, dz));
    if (it < kBicNewtonSteps) s = s - (z - zs) / gp;
  }
  const float g = z - zs;
  const float scale = fmaf(fabsf(s), fabsf(gp), fabsf(oz) + fabsf(zs));
  const bool conv = in && fabsf(g) <= kBicTol * scale;   // (false for any NaN)
  const float inv = 1.0f / sqrtf(fmaf(zx, zx, fmaf(zy, zy, 1.0f)));
  const float Nx = -zx * inv, Ny = -zy * inv, Nz = inv;
  const float KN = fmaf(dx, Nx, fmaf(dy, Ny, dz * Nz));
  AsphHit h;
  h.sq = fabsf(KN);
  const float k2 = fmaf(KN, KN, delta);
  h.ct = sqrtf(fmaxf(k2, 0.0f));
  h.tir = k2 < 0.0f;
  const float m = reflect ? -2.0f * KN : copysignf(h.ct, KN) - KN;
  dx = cx == 0.0f ? dx : fmaf(m, Nx, dx);
  dy = cy == 0.0f ? dy : fmaf(m, Ny, dy);
  dz = fmaf(m, Nz, dz);
  const float r2 = fmaf(x, x, y * y);
  px = x; py = y; hz = z; r2o = r2;
  h.fate = !conv ? kAsphMissed : !(r2 <= h2) ? kAsphAperture : (!reflect && h.tir) ? kAsphTir : kAsphAlive;
  return h;
}

// The event of a marching wave: asphere_event's interface, liveness masks and weight (the bare fraction of surface_event,
// coated_fraction or stack_fraction from sq and ct) on a biconic record.
template <bool W, class CT = NoCoat>
__device__ __forceinline__ lanemask biconic_event(Ray& r, float dzv, float cy, const LfBicRec& k, float delta, float h2,
                                                  bool reflect, float sgn, lanemask& geom_ok, float fs = 1.0f,
                                                  float fo = 1.0f, float fi = 1.0f, const CT& coat = CT()) {
  const AsphHit h = lf_bic_event(r.px, r.py, r.hz, r.r2, r.dx, r.dy, r.dz, dzv, cy, k, delta, h2, reflect, sgn);
  geom_ok = __ballot(h.fate == kAsphAlive || h.fate == kAsphTir);
  const bool no_tir = !h.tir;
  if (W) {
    float Rn, D;
    if (coat.on()) {   // wave-uniform
      if (coat.stacked()) stack_fraction(h.sq, h.ct, coat.stack(), Rn, D);
      else coated_fraction(h.sq, h.ct, coat.get(), Rn, D);
      if (!reflect) Rn = fminf(Rn, D);
    } else {           // (surface_event's bare fraction)
      const float a = (h.sq - h.ct) * fs, b = (h.sq + h.ct) * fs;
      const float pc = fi * h.ct;
      const float A = fmaf(fo, h.sq, -pc), B = fmaf(fo, h.sq, pc);
      const float u = a * B, v = A * b;
      Rn = 0.5f * fmaf(u, u, v * v);
      const float bB = b * B;
      D = bB * bB;
    }
    if (reflect) {
      r.wn *= no_tir ? Rn : 1.0f;
      r.wd *= no_tir ? D : 1.0f;
    } else {
      r.wn *= D - Rn;
      r.wd *= D;
    }
  }
  return reflect ? geom_ok : geom_ok & __ballot(no_tir);
}

}  // namespace lfm
