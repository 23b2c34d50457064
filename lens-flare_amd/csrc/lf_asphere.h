// lf_asphere.h -- an aspheric interface of the geometric lens (lf_set_lens_aspheres; DESIGN.md section 4, "aspheres"):
//   z(r^2) = c r^2 / (1 + sqrt(1 - (1 + kappa) c^2 r^2)) + r^4 (A4 + r^2 (A6 + r^2 (... A14)))
// ONE definition of the sag and of the surface event for the host (lf_asphere_sag, lf_asphere_event) and the kernels
// (lf_march_asph.hip): every multiply-add is an explicit fmaf, every root and division the IEEE one (the library is built
// with -fhip-fp32-correctly-rounded-divide-sqrt and -ffp-contract=off), so that both sides agree bit for bit -- as
// lf_point_lobe_q does for the point lights.  Nothing here is part of the ABI.
#pragma once

#include <cmath>

#include "lf_internal.h"
#include "lf_march_events.h"

namespace lfm {

// The record of an aspheric (interface, direction of travel): eight floats, one aligned 32-byte load -- a wave-uniform
// row constant.  a[m] multiplies r^(4 + 2 m).  All zero: no asphere (the interface is its base sphere).
struct alignas(32) LfAsphRec {
  float kappa;
  float a[6];
  float spare;
};
static_assert(sizeof(LfAsphRec) == 32, "one 32-byte load");

enum : int { kAsphAlive = 0, kAsphMissed = 1, kAsphAperture = 2, kAsphTir = 3 };

// Newton steps on g(s) = P_z(s) - z(r^2(s)) from the base sphere's root.  Fixed: every lane of a wave runs them all.
// Six: over the rays of tests/test_aspheres_cpu.py -- incidence cosines down to 0.05, hits out to the
// rim -- the worst ray (grazing on the convex side of interface 2 of dgauss11_asph.lens: it misses the base sphere and starts
// from the vertex plane, 6 mm off) is 6.0, 2.3, 0.67, 0.11, 3.7e-3, 4.4e-6 and then below 1e-10 from the root after steps
// 0 .. 6; a ray that meets the base sphere is there after three.  Four steps lose 7 of 1193 accepted rays of that case.
constexpr int kAsphNewtonSteps = 6;
// The convergence criterion, |g| <= kAsphTol * scale with scale = |o_z| + |z_s| + |s| |g'|: g subtracts P_z(s) =
// fma(s, K_z, o_z) and z_s = z(r^2(s)).  The ray parameter is a float: the best s lies within half a spacing of the
// root, which moves g by |g'| eps |s| (eps = 2^-24); P_z's own rounding is below eps (|o_z| + |s K_z|); z_s carries the
// root, the quotient, the polynomial's last fma and the roundings of x and y: below 4 eps |z_s| + eps |s| |g' - K_z|.
// The sum is below 4 eps scale; the last Newton step's own quotient and subtraction may leave s one spacing off the
// best one: twice that, 8 eps = 2^-21.
constexpr float kAsphTol = 4.76837158203125e-7f;   // 2^-21

// z and dz/d(r^2) at r2; false where r2 lies beyond the conic's domain (1 - (1 + kappa) c^2 r^2 < 0, or a NaN)
__host__ __device__ inline bool lf_asph_sag(float c, const LfAsphRec& k, float r2, float& z, float& zp) {
  const float kc2 = (1.0f + k.kappa) * (c * c);
  const float u = fmaf(-kc2, r2, 1.0f);
  const bool in = u >= 0.0f;
  const float root = sqrtf(in ? u : 0.0f);
  const float zc = (c * r2) / (1.0f + root);
  const float p = fmaf(r2, fmaf(r2, fmaf(r2, fmaf(r2, fmaf(r2, k.a[5], k.a[4]), k.a[3]), k.a[2]), k.a[1]), k.a[0]);
  z = fmaf(r2 * r2, p, zc);
  // d/dt [t^2 P(t)] = t (2 A4 + t (3 A6 + t (4 A8 + t (5 A10 + t (6 A12 + 7 t A14)))));  d/dt of the conic: c / (2 root)
  const float dp = r2 * fmaf(r2, fmaf(r2, fmaf(r2, fmaf(r2, fmaf(r2, 7.0f * k.a[5], 6.0f * k.a[4]), 5.0f * k.a[3]),
                                             4.0f * k.a[2]), 3.0f * k.a[1]), 2.0f * k.a[0]);
  zp = (0.5f * c) / root + dp;
  return in;
}

// What an event leaves beside the ray: the optical cosines of the Fresnel code (sq = n |cos(incidence)|, ct = n' cos t')
// and the lane's fate.
struct AsphHit {
  float sq, ct;
  int fate;
  bool tir;   // k2 < 0 (a mirror event survives it with R = 1, as in surface_event)
};

// One event of one ray on an aspheric interface; the Ray conventions of surface_event (lf_march_events.h): the position
// relative to the vertex of the interface the ray sits on, dzv to this one's, K = n d, sgn the direction of travel.
// delta = n'^2 - n^2, h2 the squared semi-aperture.  Geometry only: the weight is the caller's (asphere_event below).
//   start   the near root of the base sphere's vertex-form quadratic, s = F / (G + sgn sqrt(G^2 - c |K|^2 F)) (the
//           plane's for c = 0); the vertex plane, s = -o_z / K_z, where the ray misses the base sphere
//   refine  kAsphNewtonSteps steps s -= g / g', g' = K_z - 2 z'(r^2) (x K_x + y K_y)
//   death   beyond the conic's domain at the last point, or |g| above the criterion there: kAsphMissed
//   normal  N = (-2 z' x, -2 z' y, 1) / |N|;  KN = K.N, sq = |KN|, k2 = KN^2 + delta, ct = sqrt(k2)
//   refraction K' = K + (+-ct - KN) N (the sign of KN: the ray goes on through the surface); k2 < 0: kAsphTir
//   reflection K' = K - 2 KN N
//   aperture   r^2 <= h2 at the converged point, else kAsphAperture
// A dead lane's ray state is garbage nobody reads again.
__host__ __device__ inline AsphHit lf_asph_event(float& px, float& py, float& hz, float& r2o, float& dx, float& dy, float& dz,
                                                 float dzv, float c, const LfAsphRec& k, float delta, float h2, bool reflect,
                                                 float sgn) {
  const float oz = hz + dzv;
  float s;
  {
    const float od = fmaf(px, dx, fmaf(py, dy, oz * dz));
    const float oo = fmaf(oz, oz, fmaf(px, px, py * py));
    const float kk = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
    const float F = fmaf(c, oo, -2.0f * oz);
    const float G = fmaf(-c, od, dz);
    const float disc = fmaf(G, G, -((c * kk) * F));
    s = disc >= 0.0f ? F / fmaf(sgn, sqrtf(disc), G) : -oz / dz;
  }
  float x, y, z, r2, zs, zp, gp;
  bool in;
#pragma unroll
  for (int it = 0; it <= kAsphNewtonSteps; it++) {
    x = fmaf(s, dx, px); y = fmaf(s, dy, py); z = fmaf(s, dz, oz);
    r2 = fmaf(x, x, y * y);
    in = lf_asph_sag(c, k, r2, zs, zp);
    gp = fmaf(-2.0f * zp, fmaf(x, dx, y * dy), dz);
    if (it < kAsphNewtonSteps) s = s - (z - zs) / gp;
  }
  const float g = z - zs;
  const float scale = fmaf(fabsf(s), fabsf(gp), fabsf(oz) + fabsf(zs));
  const bool conv = in && fabsf(g) <= kAsphTol * scale;   // (false for any NaN)
  const float nx = -2.0f * zp * x, ny = -2.0f * zp * y;
  const float inv = 1.0f / sqrtf(fmaf(nx, nx, fmaf(ny, ny, 1.0f)));
  const float Nx = nx * inv, Ny = ny * inv, Nz = inv;
  const float KN = fmaf(dx, Nx, fmaf(dy, Ny, dz * Nz));
  AsphHit h;
  h.sq = fabsf(KN);
  const float k2 = fmaf(KN, KN, delta);
  h.ct = sqrtf(fmaxf(k2, 0.0f));
  h.tir = k2 < 0.0f;
  const float m = reflect ? -2.0f * KN : copysignf(h.ct, KN) - KN;
  dx = fmaf(m, Nx, dx); dy = fmaf(m, Ny, dy); dz = fmaf(m, Nz, dz);
  px = x; py = y; hz = z; r2o = r2;
  h.fate = !conv ? kAsphMissed : !(r2 <= h2) ? kAsphAperture : (!reflect && h.tir) ? kAsphTir : kAsphAlive;
  return h;
}

// The event of a marching wave: surface_event's interface and liveness masks, on an aspheric record.  A lane that
// misses, does not converge or leaves the aperture counts as vignetted (geom_ok false), a totally reflected one only
// loses `ok`.  W = true carries the weight from sq and ct through the code that exists: the bare Fresnel fraction of
// surface_event, coated_fraction or stack_fraction -- an aspheric interface may hold a film or a stack.
template <bool W, class CT = NoCoat>
__device__ __forceinline__ lanemask asphere_event(Ray& r, float dzv, float c, const LfAsphRec& k, float delta, float h2,
                                                  bool reflect, float sgn, lanemask& geom_ok, float fs = 1.0f,
                                                  float fo = 1.0f, float fi = 1.0f, const CT& coat = CT()) {
  const AsphHit h = lf_asph_event(r.px, r.py, r.hz, r.r2, r.dx, r.dy, r.dz, dzv, c, k, delta, h2, reflect, sgn);
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
