// lf_primary_general.h -- the primary path N-1 .. 0 of a lens with aspheric and / or biconic records (lf_set_lens_aspheres,
// lf_set_lens_biconics), for the lens camera of the scene term under LF_LENSCAM_SURFACES_ALL (lf_set_lens_camera_surfaces;
// DESIGN.md section 4, "the scene through recorded interfaces").  primary_path (lf_march_events.h) and LfPrimaryDev know
// spheres only and stay as they are; the records travel in a side table of their own (LfPrimarySurfDev, lf_internal.h: one
// kind word and one 32-byte record slot per primary row).  Under LF_LENSCAM_SURFACES_POSED a row may be posed too
// (lf_set_lens_poses): its kind word carries LF_EV_POSE and its LfPoseRec lies behind the records (SURF = 3).  Device code only;
// nothing here is part of the ABI.
#pragma once

#include "lf_internal.h"
#include "lf_march_events.h"
#include "lf_asphere.h"
#include "lf_biconic.h"
#include "lf_pose.h"

namespace lfm {

// row e's kind word and record: wave-uniform scalar loads, the record ONE aligned 32-byte load (lf_march_asph.hip load_asph)
__device__ __forceinline__ int load_primary_surf_kind(const LfPrimarySurfDev* __restrict__ S, int e) {
  return *(const int __attribute__((address_space(4)))*)(&S->kind[e]);
}
__device__ __forceinline__ LfAsphRec load_primary_surf_rec(const LfPrimarySurfDev* __restrict__ S, int e) {
  const lf_i8 v = *(const lf_i8 __attribute__((address_space(4)))*)(&S->rec[e][0]);
  LfAsphRec r;
  r.kappa = __int_as_float(v[0]);
#pragma unroll
  for (int m = 0; m < 6; m++) r.a[m] = __int_as_float(v[1 + m]);
  r.spare = 0.0f;
  return r;
}

// one glass row of the path, CT the row's film constants (CoatPrimary / StackPrimary): a backward refraction with the
// arguments k_march_path_rays passes for one (lf_march_asph.hip) -- reflect = false, sgn = -1 -- so that
// lf_generate_lens_rays gives the ray and weight of the scene kernel's sample bit for bit
template <int SURF, class CT>
__device__ __forceinline__ lanemask primary_row_general(const LfPrimaryRow& w, const LfPrimarySurfDev* __restrict__ S, int e,
                                                        int lambda, Ray& r, lanemask& geom_ok, const CT& coat) {
  const int kind = load_primary_surf_kind(S, e);
  if (SURF >= 3 && (kind & LF_EV_POSE)) {      // wave-uniform: a posed row -- its record in the slot, R and t behind the records (SGPRs)
    const LfAsphRec rec = load_primary_surf_rec(S, e);
    const LfPoseRec pose = load_pose((const LfPoseRec*)&S->pose[0][0], (unsigned)e * (unsigned)sizeof(LfPoseRec));
    return pose_event<true>(r, w.dzv, w.curv, (kind & LF_EV_ASPH) != 0, rec, pose, w.delta[lambda], w.h2, false, -1.0f, geom_ok,
                            w.fs[lambda], w.fo[lambda], w.fi[lambda], coat);
  }
  if (SURF >= 2 && (kind & LF_EV_BICONIC)) {   // wave-uniform: a biconic record {1/Rx, kx, ky} in the row's slot
    const LfAsphRec rec = load_primary_surf_rec(S, e);
    return biconic_event<true>(r, w.dzv, w.curv, LfBicRec{rec.kappa, rec.a[0], rec.a[1], {}}, w.delta[lambda], w.h2, false,
                               -1.0f, geom_ok, w.fs[lambda], w.fo[lambda], w.fi[lambda], coat);
  }
  if (kind & LF_EV_ASPH) {                     // wave-uniform: an aspheric record
    const LfAsphRec rec = load_primary_surf_rec(S, e);
    return asphere_event<true>(r, w.dzv, w.curv, rec, w.delta[lambda], w.h2, false, -1.0f, geom_ok, w.fs[lambda],
                               w.fo[lambda], w.fi[lambda], coat);
  }
  return surface_event<true>(r, w.dzv, w.curv, w.ch, w.c2, w.sc, w.cn22[lambda], w.rn2[lambda], w.delta[lambda], w.h2, false,
                             (w.kind & LF_EV_FLAT) != 0, -1.0f, geom_ok, w.fs[lambda], w.fo[lambda], w.fi[lambda], coat);
}

// primary_path with the rows' records.  SURF = 0: spheres, primary_path itself; 1: aspheric records; 2: aspheric and
// biconic records (a lens may carry both kinds on different interfaces, as k_march_asph<VAR, true> allows); 3: pose records
// too (pose_event<true> in the frame of the row's aspheric or biconic event, as k_march_path_rays<.., true, true>).  VAR holds
// kVarCoat (the lens camera's kernels always do).  The Newton step counts are the events' fixed, wave-uniform six and three.
template <int VAR, int SURF>
__device__ __forceinline__ bool primary_path_general(const LfPrimaryDev* __restrict__ P, const LfPrimarySurfDev* __restrict__ S,
                                                     int lambda, Ray& r, const float* __restrict__ mask, int mw, int mh,
                                                     int lane) {
  if (SURF == 0) return primary_path<VAR>(P, lambda, r, mask, mw, mh, lane);
  static_assert((VAR & kVarCoat) != 0, "the lens camera's variants");
  { const float ns = P->n_start[lambda]; r.dx *= ns; r.dy *= ns; r.dz *= ns; }   // K = n d
  bool alive = true;
  const int n = P->n;
  for (int e = 0; e < n; e++) {   // wave-uniform
    const LfPrimaryRow& w = P->row[e];
    lanemask ok, geom_ok;
    if (w.kind & LF_EV_STOP) {
      ok = stop_event<true, (VAR & kVarFilt) != 0>(r, w.dzv, w.h2, P->inv_stop_h, mask, mw, mh);
    } else {
      if (VAR & kVarStack) ok = primary_row_general<SURF>(w, S, e, lambda, r, geom_ok, StackPrimary{&w, lambda});
      else ok = primary_row_general<SURF>(w, S, e, lambda, r, geom_ok, CoatPrimary{&w, lambda});
    }
    alive = alive && ((ok >> lane) & 1ull) != 0ull;
    if (__ballot(alive) == 0ull) break;   // every lane of the wave is blocked: nothing left to march
  }
  return alive;
}

}  // namespace lfm
