// lf_pose.h -- the pose of an interface of the geometric lens (lf_set_lens_poses; DESIGN.md section 4, "posed interfaces"):
//   P = V_k + t + R q,   R = Rx(ax) Ry(ay) Rz(az)
// q on the interface as lf_set_lens, lf_set_lens_aspheres and lf_set_lens_biconics define it (vertex at the origin), V_k the
// nominal vertex on the axis, t = (dx, dy, dz) in mm, the angles right-handed and in degrees, the turn about the surface's
// own z first (it rotates a cylinder's axis).  Each interface on its own: a record is no cumulative coordinate break.
// R and t are formed on the host in double and narrowed to float (lf_pose_make).  ONE definition of the event for the host
// (lf_pose_event) and the kernels (lf_march_asph.hip; lf_primary_general.h for lf_scene.hip), in lf_asphere.h's conventions: every multiply-add an explicit fmaf,
// every root and division the IEEE one, so that both sides agree bit for bit.  Nothing here is part of the ABI.
#pragma once

#include <cmath>

#include "lf_internal.h"
#include "lf_march_events.h"
#include "lf_asphere.h"
#include "lf_biconic.h"

namespace lfm {

// The record of a posed (interface, direction of travel): R row-major and t, in a side table of its own -- 64 bytes at the
// program record's own offset (one per primary row in the lens camera's LfPrimarySurfDev), two aligned wave-uniform loads
// (load_pose, below).
struct alignas(64) LfPoseRec {
  float r[9];
  float t[3];
  float spare[4];
};
static_assert(sizeof(LfPoseRec) == 64, "a program record's stride");

// the pose table's byte offset from the aspheric table it lies behind (one 32-byte aspheric record per program record)
__host__ __device__ inline size_t lf_pose_table_offset(int n_recs) { return ((size_t)n_recs * sizeof(LfAsphRec) + 63) & ~(size_t)63; }

// host: the record of decentre (mm) and tilt (degrees)
inline LfPoseRec lf_pose_make(double dx, double dy, double dz, double ax_deg, double ay_deg, double az_deg) {
  const double d2r = 3.14159265358979323846 / 180.0;
  const double ca = std::cos(ax_deg * d2r), sa = std::sin(ax_deg * d2r);
  const double cb = std::cos(ay_deg * d2r), sb = std::sin(ay_deg * d2r);
  const double cg = std::cos(az_deg * d2r), sg = std::sin(az_deg * d2r);
  // Rx(a) Ry(b) Rz(g)
  const double R[9] = {cb * cg,                 -cb * sg,                sb,
                       ca * sg + sa * sb * cg,  ca * cg - sa * sb * sg,  -sa * cb,
                       sa * sg - ca * sb * cg,  sa * cg + ca * sb * sg,  ca * cb};
  LfPoseRec p{};
  for (int i = 0; i < 9; i++) p.r[i] = (float)R[i];
  p.t[0] = (float)dx; p.t[1] = (float)dy; p.t[2] = (float)dz;
  return p;
}

// One event of one ray on a posed interface: lf_bic_event's conventions, arguments and fates, plus the pose.
//   1  o_z = hz + dzv (the row's shift, as in every event)
//   2  into the surface's frame: o' = R^T (o - t), K' = R^T K -- full 3 x 3 fmaf products (a record of zeros: the identity)
//   3  the existing general event with dzv = 0 and the row's own sgn: lf_asph_event where ASPH (an aspheric record),
//      lf_bic_event otherwise (a biconic record; or a sphere as 1/Rx = cy, kx = ky = 0; or a plane)
//   4  point and direction back: P = R q + t, K = R K'
//   5  r2 = fmaf(px, px, py py) of the point in lens coordinates
// The clear aperture is tested in the surface's frame (step 3: the rim moves with the glass).  A lane whose local K'_z has
// not the sign of the row's direction of travel is lost as kAsphMissed.  sq and ct are the local ones: a rigid motion does
// not change them.
template <bool ASPH>
__host__ __device__ inline AsphHit lf_pose_event_t(float& px, float& py, float& hz, float& r2o, float& dx, float& dy, float& dz,
                                                   float dzv, float cy, const LfAsphRec& ka, const LfBicRec& kb,
                                                   const LfPoseRec& p, float delta, float h2, bool reflect, float sgn) {
  const float* R = p.r;
  const float ux = px - p.t[0], uy = py - p.t[1], uz = (hz + dzv) - p.t[2];
  float qx = fmaf(R[0], ux, fmaf(R[3], uy, R[6] * uz));
  float qy = fmaf(R[1], ux, fmaf(R[4], uy, R[7] * uz));
  float qz = fmaf(R[2], ux, fmaf(R[5], uy, R[8] * uz));
  float kx = fmaf(R[0], dx, fmaf(R[3], dy, R[6] * dz));
  float ky = fmaf(R[1], dx, fmaf(R[4], dy, R[7] * dz));
  float kz = fmaf(R[2], dx, fmaf(R[5], dy, R[8] * dz));
  const bool towards = kz * sgn > 0.0f;   // (false for a NaN)
  float r2l;
  AsphHit h = ASPH ? lf_asph_event(qx, qy, qz, r2l, kx, ky, kz, 0.0f, cy, ka, delta, h2, reflect, sgn)
                   : lf_bic_event(qx, qy, qz, r2l, kx, ky, kz, 0.0f, cy, kb, delta, h2, reflect, sgn);
  if (!towards) h.fate = kAsphMissed;
  px = fmaf(R[0], qx, fmaf(R[1], qy, R[2] * qz)) + p.t[0];
  py = fmaf(R[3], qx, fmaf(R[4], qy, R[5] * qz)) + p.t[1];
  hz = fmaf(R[6], qx, fmaf(R[7], qy, R[8] * qz)) + p.t[2];
  dx = fmaf(R[0], kx, fmaf(R[1], ky, R[2] * kz));
  dy = fmaf(R[3], kx, fmaf(R[4], ky, R[5] * kz));
  dz = fmaf(R[6], kx, fmaf(R[7], ky, R[8] * kz));
  r2o = fmaf(px, px, py * py);
  return h;
}

// (asph != 0: `ka` is the interface's aspheric record; else `kb` its biconic one -- {cy, 0, 0} for a sphere, {0, 0, 0} on a plane)
__host__ __device__ inline AsphHit lf_pose_event(float& px, float& py, float& hz, float& r2o, float& dx, float& dy, float& dz,
                                                 float dzv, float cy, bool asph, const LfAsphRec& ka, const LfBicRec& kb,
                                                 const LfPoseRec& p, float delta, float h2, bool reflect, float sgn) {
  return asph ? lf_pose_event_t<true>(px, py, hz, r2o, dx, dy, dz, dzv, cy, ka, kb, p, delta, h2, reflect, sgn)
              : lf_pose_event_t<false>(px, py, hz, r2o, dx, dy, dz, dzv, cy, ka, kb, p, delta, h2, reflect, sgn);
}

#if defined(__HIPCC__)
// a record of a pose table: TWO 32-byte scalar loads (the offset is wave-uniform).  One helper for the march's tables
// (lf_march_asph.hip) and the lens camera's primary rows (lf_primary_general.h).
__device__ __forceinline__ LfPoseRec load_pose(const LfPoseRec* __restrict__ base, unsigned off) {
  typedef const char __attribute__((address_space(4))) * cptr;
  const lf_i8 v = *(const lf_i8 __attribute__((address_space(4)))*)((cptr)(base) + off);
  const lf_i8 w = *(const lf_i8 __attribute__((address_space(4)))*)((cptr)(base) + off + 32u);
  LfPoseRec r;
#pragma unroll
  for (int m = 0; m < 8; m++) r.r[m] = __int_as_float(v[m]);
  r.r[8] = __int_as_float(w[0]);
#pragma unroll
  for (int m = 0; m < 3; m++) r.t[m] = __int_as_float(w[1 + m]);
#pragma unroll
  for (int m = 0; m < 4; m++) r.spare[m] = 0.0f;
  return r;
}

// The event of a marching wave: biconic_event's interface, liveness masks and weight on a posed interface; `asph` is
// wave-uniform (a kind bit of the row).
template <bool W, class CT = NoCoat>
__device__ __forceinline__ lanemask pose_event(Ray& r, float dzv, float cy, bool asph, const LfAsphRec& ka, const LfPoseRec& p,
                                               float delta, float h2, bool reflect, float sgn, lanemask& geom_ok,
                                               float fs = 1.0f, float fo = 1.0f, float fi = 1.0f, const CT& coat = CT()) {
  const LfBicRec kb{ka.kappa, ka.a[0], ka.a[1], {}};   // (a biconic record sits in the aspheric record's slot)
  const AsphHit h = lf_pose_event(r.px, r.py, r.hz, r.r2, r.dx, r.dy, r.dz, dzv, cy, asph, ka, kb, p, delta, h2, reflect, sgn);
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
#endif

}  // namespace lfm
