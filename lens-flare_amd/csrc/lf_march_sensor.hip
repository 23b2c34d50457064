// lf_march_sensor.hip -- sensor-reflection ghosts of the geometric lens (lf_set_sensor_ghosts; DESIGN.md section 4, "sensor
// ghosts"): the sensor is a mirror behind the lens.  The sensor path of interface i is marched from the sensor like every
// other path: back to i, reflected there, forward to the sensor plane, mirrored (lf_sensor_event.h), back through the whole
// lens and out -- 3 n - 2 i events.
//   k_march_sensor<VAR, SURF>      the frame: k_march_asph's frame (workgroups of 8 waves, the wave tile, march_tile_of, sgroups,
//                                  the samples dealt through s_next, the fixed-point LDS sums, the final write) over the sensor
//                                  paths' OWN table -- one self-contained row list per (path, wavelength) (lf_path_table.h), read
//                                  through the scalar cache -- geometry first, the weighted march again only for the lanes the
//                                  lights' pre-test admits, lit rays through lights_epilogue.  SURF: 0 spheres only, 1 + aspheric
//                                  rows, 2 + biconic rows, 3 + posed rows (lf_set_sensor_ghost_surfaces(LF_SENSOR_SURFACES_POSED)
//                                  on a lens with pose records: one more wave-uniform branch, on LF_EV_POSE, to pose_event --
//                                  lf_pose.h; SURF <= 2 is the code it was).  Adds to the ghost buffer on the ordinary launch's
//                                  fixed-point grid.
//   k_march_sensor_path_rays       lf_march_sensor_path_rays: k_march_path_rays with the sensor row
// Both always aim at the DEFAULT disc, the rear element's clear aperture: the first mirror of a sensor path lies behind the
// stop or has the stop's image clipped by what follows (the comment on lf_set_pupil_target).  For a posed lens the disc is the
// CENTRED rear element's clear aperture at its nominal vertex plane, also when that element is decentred -- the convention of
// the ordinary posed march and of the lens camera: it says where the samples aim and approximates nothing of the event.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "lf_internal.h"
#include "lf_march_events.h"
#include "lf_march_common.h"
#include "lf_asphere.h"
#include "lf_biconic.h"
#include "lf_pose.h"
#include "lf_path_table.h"
#include "lf_sensor_event.h"

using namespace lfm;

namespace {

constexpr int kSensorWgWaves = 8;

// The table: a header, one entry per (path, wavelength), the rows (128-byte aligned), the stack records behind them and --
// only where SURF = 3 reads it -- ONE LfPoseRec per posed interface behind those, from a 64-byte boundary on (a pose depends
// neither on the wavelength nor on the direction of travel).  A posed row carries LF_EV_POSE with LF_EV_ASPH or LF_EV_BICONIC
// (a sphere or a plane as the biconic {1/R, 0, 0}), and in its spare dword the record's byte offset from the table's start.
struct alignas(32) LfSensorTabHdr {
  int n_paths, n_lambda;
  int pad[6];
};
struct alignas(16) LfSensorPathHdr {
  int off;      // bytes from the table's start to the path's first row
  int n_ev;     // 3 n - 2 i
  int iface;    // i
  int skip;     // the sensor's reflectance is 0 at this wavelength: not marched
};

typedef const char __attribute__((address_space(4))) * sc_ptr;

// what the geometry and the weight need of a row: its first 64 bytes, ONE scalar load (the offset is wave-uniform)
struct SRow {
  float dzv, curv, ch, c2, sc, h2, sgn;
  int kind;
  float cn22, rn2, delta, fs, fo, fi;
  int coated;
  unsigned pose;   // (a posed row's: the byte offset of its pose record)
};
__device__ __forceinline__ SRow load_srow(sc_ptr tab, unsigned off) {
  const lf_i16 v = *(lf_const_prow_ptr)(tab + off);
  SRow r;
  r.dzv = __int_as_float(v[0]); r.curv = __int_as_float(v[1]); r.ch = __int_as_float(v[2]); r.c2 = __int_as_float(v[3]);
  r.sc = __int_as_float(v[4]); r.h2 = __int_as_float(v[5]); r.sgn = __int_as_float(v[6]); r.kind = v[7];
  r.cn22 = __int_as_float(v[8]); r.rn2 = __int_as_float(v[9]); r.delta = __int_as_float(v[10]);
  r.fs = __int_as_float(v[11]); r.fo = __int_as_float(v[12]); r.fi = __int_as_float(v[13]); r.coated = v[14];
  r.pose = (unsigned)v[15];
  return r;
}
// a row's aspheric / biconic record: its last 32 bytes, one scalar load
__device__ __forceinline__ LfAsphRec load_srow_rec(sc_ptr tab, unsigned off) {
  const lf_i8 v = *(const lf_i8 __attribute__((address_space(4)))*)(tab + off + (unsigned)offsetof(LfPathRow, asph));
  LfAsphRec r;
  r.kappa = __int_as_float(v[0]);
#pragma unroll
  for (int m = 0; m < 6; m++) r.a[m] = __int_as_float(v[1 + m]);
  r.spare = 0.0f;
  return r;
}
// a row's film or stack (PathCoat's encoding), every dword a scalar load
struct SensorCoat {
  sc_ptr row;
  int coated;
  __device__ __forceinline__ bool on() const { return coated != 0; }
  __device__ __forceinline__ bool stacked() const { return (coated & 2) != 0; }
  __device__ __forceinline__ LfCoatK get() const {
    const lf_i8 v = *(const lf_i8 __attribute__((address_space(4)))*)(row + (unsigned)offsetof(LfPathRow, coat));
    return LfCoatK{__int_as_float(v[0]), __int_as_float(v[1]), __int_as_float(v[2]), __int_as_float(v[3]),
                   __int_as_float(v[4]), __int_as_float(v[5]), __int_as_float(v[6]), __int_as_float(v[7])};
  }
  __device__ __forceinline__ StackLoad stack() const { return StackLoad{row + (coated & ~3)}; }
};

struct SensorArgs {
  float xmax, ymax;      // the WHOLE frame's rectangle on the sensor: half_w pitch, half_h pitch (mm)
  double inv_scale;      // 2^-bits of the launch's fixed-point grid (2^-36 unless the lights are HDR)
};

struct SensorTally {
  unsigned long long started = 0, reached = 0, lost = 0;
  unsigned n_light = 0;   // per lane
};

enum : int { kRowGlass = 0, kRowStop = 1, kRowSensor = 2 };

// One row of a sensor path, W as surface_event's: the stop, the sensor's mirror, an aspheric / biconic row, or the spherical
// event -- asph_row's dispatch (lf_march_asph.hip) plus the mirror.  *what: which of the three kinds of plane the row was.
template <bool W, int VAR, int SURF>
__device__ __forceinline__ lanemask sensor_row(Ray& r, sc_ptr tab, unsigned off, const float* __restrict__ mask, const MarchArgs& a,
                                               const SensorArgs& sa, int& what) {
  const SRow w = load_srow(tab, off);
  if (w.kind & LF_EV_STOP) {
    what = kRowStop;
    return stop_event_var<W, VAR>(r, w.dzv, w.h2, a.inv_stop_h, mask, a.mw, a.mh);
  }
  if (w.kind & LF_EV_SENSOR) {
    what = kRowSensor;
    return sensor_event<W>(r, w.dzv, sa.xmax, sa.ymax, w.fs);
  }
  what = kRowGlass;
  lanemask geom_ok;
  const bool reflect = (w.kind & LF_EV_REFLECT) != 0;
  if (VAR & kVarCoat) {
    const SensorCoat coat{tab + off, w.coated};
    if (SURF >= 3 && (w.kind & LF_EV_POSE)) {   // wave-uniform: the row's pose record, through the scalar cache
      const LfAsphRec rec = load_srow_rec(tab, off);
      const LfPoseRec pose = load_pose((const LfPoseRec*)(const char*)tab, w.pose);
      return pose_event<W>(r, w.dzv, w.curv, (w.kind & LF_EV_ASPH) != 0, rec, pose, w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo,
                           w.fi, coat);
    }
    if (SURF >= 2 && (w.kind & LF_EV_BICONIC)) {
      const LfAsphRec rec = load_srow_rec(tab, off);
      return biconic_event<W>(r, w.dzv, w.curv, LfBicRec{rec.kappa, rec.a[0], rec.a[1], {}}, w.delta, w.h2, reflect, w.sgn, geom_ok,
                              w.fs, w.fo, w.fi, coat);
    }
    if (SURF >= 1 && (w.kind & LF_EV_ASPH))
      return asphere_event<W>(r, w.dzv, w.curv, load_srow_rec(tab, off), w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi, coat);
    return surface_event<W>(r, w.dzv, w.curv, w.ch, w.c2, w.sc, w.cn22, w.rn2, w.delta, w.h2, reflect, (w.kind & LF_EV_FLAT) != 0,
                            w.sgn, geom_ok, w.fs, w.fo, w.fi, coat);
  }
  if (SURF >= 3 && (w.kind & LF_EV_POSE)) {
    const LfAsphRec rec = load_srow_rec(tab, off);
    const LfPoseRec pose = load_pose((const LfPoseRec*)(const char*)tab, w.pose);
    return pose_event<W>(r, w.dzv, w.curv, (w.kind & LF_EV_ASPH) != 0, rec, pose, w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi);
  }
  if (SURF >= 2 && (w.kind & LF_EV_BICONIC)) {
    const LfAsphRec rec = load_srow_rec(tab, off);
    return biconic_event<W>(r, w.dzv, w.curv, LfBicRec{rec.kappa, rec.a[0], rec.a[1], {}}, w.delta, w.h2, reflect, w.sgn, geom_ok,
                            w.fs, w.fo, w.fi);
  }
  if (SURF >= 1 && (w.kind & LF_EV_ASPH))
    return asphere_event<W>(r, w.dzv, w.curv, load_srow_rec(tab, off), w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi);
  return surface_event<W>(r, w.dzv, w.curv, w.ch, w.c2, w.sc, w.cn22, w.rn2, w.delta, w.h2, reflect, (w.kind & LF_EV_FLAT) != 0,
                          w.sgn, geom_ok, w.fs, w.fo, w.fi);
}

// sensor path q of one sensor sample per lane, every wavelength on its own: geometry, tallies, the lights' pre-test, the
// weighted march of the lit lanes, the lit epilogue into the tile's LDS sums (march_asph_path's steps)
template <int VAR, int SURF>
__device__ __forceinline__ void march_sensor_path(const LfLensDev* __restrict__ lens, sc_ptr tab, int n_lambda, int q,
                                                  const float* __restrict__ mask, const MarchArgs& a, const SensorArgs& sa,
                                                  lanemask start_mask, const StartRay& s0, int lane,
                                                  unsigned long long* __restrict__ s_acc, const float* __restrict__ s_chan,
                                                  SensorTally& T) {
  for (int l = 0; l < n_lambda; l++) {
    const lf_i4 ph = *(lf_const_phdr_ptr)(tab + (unsigned)(sizeof(LfSensorTabHdr) + sizeof(LfSensorPathHdr) * (size_t)(q * n_lambda + l)));
    if (ph[3] != 0) continue;     // (the sensor reflects nothing at this wavelength)
    const unsigned off0 = (unsigned)ph[0];
    const int n_ev = ph[1];
    const float ns = lens->n_start[l];
    Ray r[1];
    r[0] = Ray{s0.X, s0.Y, 0.0f, fmaf(s0.X, s0.X, s0.Y * s0.Y), s0.dx * ns, s0.dy * ns, s0.dz * ns, s0.w0, 1.0f};
    lanemask alive[1] = {start_mask};
    unsigned nlive = (unsigned)__popcll(start_mask);
    T.started += nlive;
    for (int e = 0; e < n_ev && nlive != 0u; e++) {
      int what;
      const lanemask ok = sensor_row<false, VAR, SURF>(r[0], tab, off0 + (unsigned)e * (unsigned)sizeof(LfPathRow), mask, a, sa, what);
      if (what == kRowSensor) {
        T.reached += nlive;
        T.lost += (unsigned)__popcll(alive[0] & ~ok);
      }
      alive[0] &= ok;
      nlive = (unsigned)__popcll(alive[0]);
    }
    if (nlive == 0u) continue;
    lanemask lit[1];
    if (lights_pretest<1, true, VAR>(lens, r, alive, lit) == 0ull) continue;
    // the path again with its weight: the same arithmetic on the ray, so the same ray bit for bit
    Ray rw{s0.X, s0.Y, 0.0f, fmaf(s0.X, s0.X, s0.Y * s0.Y), s0.dx * ns, s0.dy * ns, s0.dz * ns, s0.w0, 1.0f};
    for (int e = 0; e < n_ev; e++) {
      int what;
      (void)sensor_row<true, VAR, SURF>(rw, tab, off0 + (unsigned)e * (unsigned)sizeof(LfPathRow), mask, a, sa, what);
    }
    lights_epilogue<VAR>(lens, s_chan, rw, ((lit[0] >> lane) & 1ull) != 0ull, l, &s_acc[lane * 3], T.n_light);
  }
}

template <int VAR, int SURF>
__global__ __launch_bounds__(64 * kSensorWgWaves) void k_march_sensor(
    const LfLensDev* __restrict__ lens, const unsigned char* __restrict__ table, const float* __restrict__ mask, MarchArgs a,
    SensorArgs sa, double* __restrict__ ghost, unsigned long long* __restrict__ accum, unsigned long long* __restrict__ stats) {
  __shared__ unsigned long long s_acc[64 * 3];
  __shared__ unsigned long long s_cnt[kSensorStats];
  __shared__ int s_next;
  __shared__ float s_chan[kLightChan];
  const int tid = threadIdx.x;
  if (tid < 64 * 3) s_acc[tid] = 0ull;
  lights_channel_factors(lens, s_chan, tid, 64 * kSensorWgWaves);
  if (tid < kSensorStats) s_cnt[tid] = 0ull;
  if (tid == 0) s_next = 0;
  __syncthreads();

  // the workgroup's wave tile and its share of the samples: as k_march_asph
  const int tiles_x = ((a.W + (8 << a.xs) - 1) >> (3 + a.xs)) << a.xs;
  const int sgroups = a.sgroups;
  const int sg = (int)(blockIdx.x % (unsigned)sgroups);
  const unsigned slot = blockIdx.x / (unsigned)sgroups;
  const int tile_lin = (int)((slot & ~63u) | ((slot & 7u) << 3) | ((slot >> 3) & 7u));
  if (tile_lin >= a.n_tiles) return;
  int tx, trow;
  march_tile_of(a, tile_lin, tiles_x, tx, trow);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int x = ((tx >> a.xs) << (3 + a.xs)) + ((lane & 7) << a.xs) + (tx & ((1 << a.xs) - 1)), y = trow * 8 + (lane >> 3);
  const bool active = x < a.W && y >= a.y0 && y < a.y1;
  const lanemask active_mask = __ballot(active);
  const unsigned p = (unsigned)y * (unsigned)a.W + (unsigned)x;

  SampleSpec spec;
  spec.W = a.W; spec.G = a.G; spec.inv_G = a.inv_G; spec.xs = a.xs; spec.sub_bits = a.sub_bits; spec.inv_sub = a.inv_sub;
  spec.key = a.key; spec.pitch = lens->pitch; spec.half_w = a.half_w; spec.half_h = a.half_h;
  spec.pupil_h = lens->pupil_h; spec.vz = a.vz; spec.geom_norm = lens->geom_norm;

  const sc_ptr tab = (sc_ptr)table;
  const int n_paths = *(const int __attribute__((address_space(4)))*)(tab);
  const int n_lambda = *(const int __attribute__((address_space(4)))*)(tab + 4);

  SensorTally T;
  const int n_mine = (a.spp - sg + sgroups - 1) / sgroups;     // samples sg, sg + sgroups, ...
  if (active_mask != 0ull)
    for (;;) {
      int k = 0;
      if (lane == 0) k = atomicAdd(&s_next, 1);
      k = __builtin_amdgcn_readfirstlane(k);
      if (k >= n_mine) break;
      const int s = sg + k * sgroups;       // wave-uniform
      const StartRay s0 = sample_start(spec, x, y, s);
      for (int q = 0; q < n_paths; q++)
        march_sensor_path<VAR, SURF>(lens, tab, n_lambda, q, mask, a, sa, active_mask, s0, lane, s_acc, s_chan, T);
    }

  // ---- counters, a block of their own: one LDS add per wave, one global add per workgroup ----
  {
    unsigned long long v3 = T.n_light;
    for (int off = 32; off > 0; off >>= 1) v3 += __shfl_down(v3, off);
    const unsigned long long vals[kSensorStats] = {T.started, T.reached, T.lost, v3};
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kSensorStats; i++)
        if (vals[i]) atomicAdd(&s_cnt[i], vals[i]);
    }
  }
  __syncthreads();
  if (wave == 0 && lane < kSensorStats && s_cnt[lane]) atomicAdd(&stats[lane], s_cnt[lane]);
  if (wave == 0 && active) {
    if (a.sgroups == 1) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double v = ((double)s_acc[lane * 3 + c] * sa.inv_scale) / (double)a.spp;
        ghost[3 * (size_t)p + c] = a.accumulate ? ghost[3 * (size_t)p + c] + v : v;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++)
        if (s_acc[lane * 3 + c]) atomicAdd(&accum[3 * (size_t)p + c], s_acc[lane * 3 + c]);
    }
  }
}

// the integer sums of a launch split over sample groups -> the ghost buffer (k_march_finish's conversion, on the launch's grid)
__global__ void k_sensor_finish(const unsigned long long* __restrict__ accum, MarchArgs a, SensorArgs sa, double* __restrict__ ghost) {
  const size_t p = (size_t)a.y0 * a.W + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (size_t)a.y1 * a.W) return;
  if (!march_owns(a, (int)(p % a.W), (int)(p / a.W))) return;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double v = ((double)accum[3 * p + c] * sa.inv_scale) / (double)a.spp;
    ghost[3 * p + c] = a.accumulate ? ghost[3 * p + c] + v : v;
  }
}

// a replacing launch in which no column of the sensor reflects: zeros, in the pixels this context owns and no others
__global__ void k_sensor_zero(MarchArgs a, double* __restrict__ ghost) {
  const size_t p = (size_t)a.y0 * a.W + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (size_t)a.y1 * a.W) return;
  if (!march_owns(a, (int)(p % a.W), (int)(p / a.W))) return;
#pragma unroll
  for (int c = 0; c < 3; c++) ghost[3 * p + c] = 0.0;
}

// ---- lf_march_sensor_path_rays: k_march_path_rays (lf_march_asph.hip) with the sensor row ---------------------------------
template <bool FILT, bool COAT, int SURF>
__global__ __launch_bounds__(256) void k_march_sensor_path_rays(const LfLensDev* __restrict__ lens, const LfPathDev* __restrict__ P,
                                                                const float* __restrict__ mask, int mw, int mh, SensorArgs sa, int n,
                                                                const float* __restrict__ sensor_xy,
                                                                const float* __restrict__ pupil_uv, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool active = i < n;
  const float X = active ? sensor_xy[2 * i] : 0.0f, Y = active ? sensor_xy[2 * i + 1] : 0.0f;
  const float pa = active ? pupil_uv[2 * i] : 0.0f, pb = active ? pupil_uv[2 * i + 1] : 0.0f;
  const StartRay s0 = aim_at_pupil(X, Y, pa, pb, lens->pupil_h, lens->pupil_z - lens->z_sensor, lens->geom_norm);
  Ray r{X, Y, 0.0f, fmaf(X, X, Y * Y), s0.dx, s0.dy, s0.dz, s0.w0, 1.0f};
  { const float ns = P->n_start; r.dx *= ns; r.dy *= ns; r.dz *= ns; }   // K = n d
  bool alive = true;
  const int n_ev = P->n;
  for (int e = 0; e < n_ev; e++) {   // wave-uniform
    const LfPathRow& w = P->row[e];
    lanemask ok, geom_ok;
    const bool reflect = (w.kind & LF_EV_REFLECT) != 0;
    if (w.kind & LF_EV_STOP) {
      ok = stop_event<true, FILT>(r, w.dzv, w.h2, P->inv_stop_h, mask, mw, mh);
    } else if (w.kind & LF_EV_SENSOR) {
      ok = sensor_event<true>(r, w.dzv, sa.xmax, sa.ymax, w.fs);
    } else if (SURF >= 3 && (w.kind & LF_EV_POSE)) {   // wave-uniform
      const LfPoseRec pose = load_pose((const LfPoseRec*)P, (unsigned)w.pad);
      const bool asph = (w.kind & LF_EV_ASPH) != 0;
      if (COAT) ok = pose_event<true>(r, w.dzv, w.curv, asph, w.asph, pose, w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi, PathCoat{&w});
      else ok = pose_event<true>(r, w.dzv, w.curv, asph, w.asph, pose, w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi);
    } else if (SURF >= 2 && (w.kind & LF_EV_BICONIC)) {
      const LfBicRec rec{w.asph.kappa, w.asph.a[0], w.asph.a[1], {}};
      if (COAT) ok = biconic_event<true>(r, w.dzv, w.curv, rec, w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi, PathCoat{&w});
      else ok = biconic_event<true>(r, w.dzv, w.curv, rec, w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi);
    } else if (SURF >= 1 && (w.kind & LF_EV_ASPH)) {
      if (COAT) ok = asphere_event<true>(r, w.dzv, w.curv, w.asph, w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi, PathCoat{&w});
      else ok = asphere_event<true>(r, w.dzv, w.curv, w.asph, w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi);
    } else {
      if (COAT)
        ok = surface_event<true>(r, w.dzv, w.curv, w.ch, w.c2, w.sc, w.cn22, w.rn2, w.delta, w.h2, reflect, (w.kind & LF_EV_FLAT) != 0,
                                 w.sgn, geom_ok, w.fs, w.fo, w.fi, PathCoat{&w});
      else
        ok = surface_event<true>(r, w.dzv, w.curv, w.ch, w.c2, w.sc, w.cn22, w.rn2, w.delta, w.h2, reflect, (w.kind & LF_EV_FLAT) != 0,
                                 w.sgn, geom_ok, w.fs, w.fo, w.fi);
    }
    alive = alive && ((ok >> lane) & 1ull) != 0ull;
    if (__ballot(alive) == 0ull) break;
  }
  if (active) {
    float* o = out + 8 * (size_t)i;
    o[0] = r.px; o[1] = r.py; o[2] = P->front_zv + r.hz; o[3] = r.dx; o[4] = r.dy; o[5] = r.dz;
    o[6] = alive ? __fdiv_rn(r.wn, r.wd) : 0.0f;
    o[7] = alive ? 1.0f : 0.0f;
  }
}

// host: the pose block of a table -- ONE record per posed interface, in the interfaces' order; interface k's is the
// pose_slot(k)-th.  The block starts at a 64-byte boundary (load_pose's two aligned 32-byte loads).
int pose_slot(const lf_ctx* ctx, int k) {
  int m = 0;
  for (int j = 0; j < k; j++) m += ctx->pose.on[j] != 0 ? 1 : 0;
  return m;
}
void pose_block_fill(const lf_ctx* ctx, unsigned char* block) {
  const LfPoses& Po = ctx->pose;
  for (int k = 0; k < ctx->lens.n_surf; k++) {
    if (!Po.on[k]) continue;
    const LfPoseRec rec = lf_pose_make(Po.t[3 * k], Po.t[3 * k + 1], Po.t[3 * k + 2], Po.a[3 * k], Po.a[3 * k + 1], Po.a[3 * k + 2]);
    std::memcpy(block + (size_t)pose_slot(ctx, k) * sizeof(rec), &rec, sizeof(rec));
  }
}

// host: the rows of the sensor path of interface i at wavelength l, from base + first_row on (lf_sensor_path_sequence's order).
// pose_off != 0 (SURF = 3): the byte offset of the table's pose block; every crossing of a posed interface then becomes a
// posed row (build_path_table's fields, written HERE and not in lf_path_row_fill: lf_march_path_rays' rows stay what they
// are) that points at the interface's one record.  The stop's rows and the sensor's never carry the bit.
lf_status sensor_path_rows(const lf_ctx* ctx, int l, int i, unsigned char* base, size_t first_row, size_t* next_stack, size_t cap,
                           size_t pose_off, int* n_rows) {
  const LfLensDev& L = ctx->lens;
  const LfPoses& Po = ctx->pose;
  const int n = L.n_surf;
  int cnt = 0;
  lf_status st = LF_OK;
  auto put = [&](int k, int from, bool reflect, bool fwd) {
    const size_t row_off = first_row + (size_t)cnt * sizeof(LfPathRow);
    if (st == LF_OK) st = lf_path_row_fill(ctx, l, k, from, reflect, fwd, base, row_off, next_stack, cap);
    if (st == LF_OK && pose_off != 0 && Po.on[k] && L.surf[k].is_stop == 0.0f) {
      LfPathRow& w = *reinterpret_cast<LfPathRow*>(base + row_off);
      w.kind |= LF_EV_POSE;
      if (!(w.kind & LF_EV_BICONIC) && !(w.kind & LF_EV_ASPH && ctx->asph.n > 0)) {   // a sphere or a plane: as a biconic
        w.kind = (w.kind & ~LF_EV_ASPH) | LF_EV_BICONIC;
        w.asph = LfAsphRec{};
        w.asph.kappa = L.surf[k].curv;
      }
      w.pad = (int)(pose_off + (size_t)pose_slot(ctx, k) * sizeof(LfPoseRec));
    }
    cnt++;
  };
  for (int k = n - 1; k > i; k--) put(k, k + 1, false, false);
  put(i, i + 1, true, false);
  for (int k = i + 1; k < n; k++) put(k, k == i + 1 ? i : k - 1, false, true);
  {   // the sensor's mirror, coming from the rear element
    LfPathRow& w = *reinterpret_cast<LfPathRow*>(base + first_row + (size_t)cnt * sizeof(LfPathRow));
    w.dzv = L.surf[n - 1].zv - L.z_sensor;
    w.sgn = 1.0f;
    w.kind = LF_EV_SENSOR;
    w.fs = ctx->sensor.refl[l];
    cnt++;
  }
  for (int k = n - 1; k >= 0; k--) put(k, k + 1, false, false);
  *n_rows = cnt;
  return st;
}

// the default disc, whatever lf_set_pupil_target holds for the ordinary paths (lf_apply_pupil_target's arithmetic)
void default_disc(const lf_ctx* ctx, LfLensDev& L) {
  const int n = L.n_surf;
  L.pupil_h = ctx->raw_semi_ap[n - 1];
  L.pupil_z = L.surf[n - 1].zv;
  const double D = (double)L.z_sensor - (double)L.pupil_z;
  L.geom_norm = (float)((3.14159265358979323846 * (double)L.pupil_h * (double)L.pupil_h) / (D * D));
}

// SURF of the kernels: what kinds of row the table can hold (lf_surface_record_kind)
// (3: posed rows -- only for a lens with a pose record under LF_SENSOR_SURFACES_POSED; the entry points refuse such a lens
// under LF_SENSOR_SURFACES_CENTRED, and a lens without records launches what it launched whatever the setting)
int surf_kind(const lf_ctx* ctx) {
  if (lf_march_posed(ctx) && ctx->sensor.surfaces == LF_SENSOR_SURFACES_POSED) return 3;
  return lf_march_biconic(ctx) ? 2 : lf_march_aspheric(ctx) ? 1 : 0;
}

// host: the stack records' bytes of the whole selection, exactly: the pose block's offset goes into the rows while they are
// written, before the last stack record is.  The sensor path of interface i crosses interface k three times where k > i, twice
// where k == i and once in front of it (lf_sensor_path_sequence); lf_path_row_fill appends one record per crossing of a
// stacked interface.
size_t sensor_stack_bytes(const lf_ctx* ctx, const int* sel, int n_sel) {
  const LfCoatings& C = ctx->coat;
  if (C.n_stacked <= 0) return 0;
  size_t bytes = 0;
  for (int q = 0; q < n_sel; q++)
    for (int k = 0; k < ctx->lens.n_surf; k++) {
      if (C.n_layers[k] < 2 || ctx->lens.surf[k].is_stop != 0.0f) continue;
      bytes += (size_t)(k > sel[q] ? 3 : k == sel[q] ? 2 : 1) * sizeof(float) * kStackDwords(C.n_layers[k]);
    }
  return bytes * (size_t)ctx->lens.n_lambda;
}

// host: the whole table of the selection; uploads it where the device's copy differs
lf_status sensor_table_upload(lf_ctx* ctx, const int* sel, int n_sel) {
  const LfLensDev& L = ctx->lens;
  const int n = L.n_surf, nl = L.n_lambda;
  size_t total_rows = 0;
  for (int q = 0; q < n_sel; q++) total_rows += (size_t)(3 * n - 2 * sel[q]) * (size_t)nl;
  const size_t hdr = (sizeof(LfSensorTabHdr) + sizeof(LfSensorPathHdr) * (size_t)n_sel * (size_t)nl + 127) & ~(size_t)127;
  const size_t rows_end = hdr + total_rows * sizeof(LfPathRow);
  std::vector<unsigned char> buf(rows_end + total_rows * kPathStackRowBytes, 0);
  LfSensorTabHdr& H = *reinterpret_cast<LfSensorTabHdr*>(buf.data());
  H.n_paths = n_sel; H.n_lambda = nl;
  size_t next_row = hdr, next_stack = rows_end;
  // (SURF = 3 alone reads a pose block: it lies behind the last stack record, from the next 64-byte boundary on)
  const bool posed = surf_kind(ctx) == 3;
  const size_t stack_end = rows_end + sensor_stack_bytes(ctx, sel, n_sel);
  const size_t pose_off = posed ? (stack_end + 63) & ~(size_t)63 : 0;
  for (int q = 0; q < n_sel; q++)
    for (int l = 0; l < nl; l++) {
      LfSensorPathHdr& ph = reinterpret_cast<LfSensorPathHdr*>(buf.data() + sizeof(LfSensorTabHdr))[q * nl + l];
      int cnt = 0;
      if (3 * n - 2 * sel[q] > kPathRowsMax ||
          sensor_path_rows(ctx, l, sel[q], buf.data(), next_row, &next_stack, buf.size(), pose_off, &cnt) != LF_OK)
        return lf_fail(ctx, LF_ERR_STATE, "sensor ghosts: a path's rows exceed their table");
      ph.off = (int)next_row; ph.n_ev = cnt; ph.iface = sel[q];
      ph.skip = ctx->sensor.refl[l] == 0.0f ? 1 : 0;
      next_row += (size_t)cnt * sizeof(LfPathRow);
    }
  buf.resize(next_stack);
  if (posed) {   // (after the resize, which cuts the table at its last stack record: the block is part of the allocation)
    if (next_stack != stack_end) return lf_fail(ctx, LF_ERR_STATE, "sensor ghosts: the stack records are not where the pose block expects them");
    buf.resize(pose_off + (size_t)ctx->pose.n * sizeof(LfPoseRec), 0);
    pose_block_fill(ctx, buf.data() + pose_off);
  }
  LfSensorGhosts& S = ctx->sensor;
  if (S.table_dev && buf == S.table_host) return LF_OK;
  // (the stream is non-blocking: a kernel still walking the previous table must be done before it changes -- build_event_table)
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (buf.size() > S.table_cap) {
    if (S.table_dev) (void)hipFree(S.table_dev);
    S.table_dev = nullptr; S.table_cap = 0; S.table_host.clear();
    LF_HIP(ctx, hipMalloc((void**)&S.table_dev, buf.size()));
    S.table_cap = buf.size();
  }
  S.table_host.clear();
  hipEvent_t ev = lf_timing_begin(ctx, LFK_SENSOR_TABLE);   // ("sensor_table": one per upload)
  LF_HIP(ctx, hipMemcpy(S.table_dev, buf.data(), buf.size(), hipMemcpyHostToDevice));
  lf_timing_end(ctx, LFK_SENSOR_TABLE, ev);
  S.table_host.swap(buf);
  return LF_OK;
}

}  // namespace

int lf_sensor_selection(const lf_ctx* ctx, int out[LF_MAX_SURFACES]) {
  const LfSensorGhosts& S = ctx->sensor;
  const int n = ctx->lens.n_surf, stop = ctx->lens.stop;
  int m = 0;
  if (S.n_sel < 0) {
    for (int k = 0; k < n; k++) if (k != stop) out[m++] = k;
    return m;
  }
  for (int q = 0; q < S.n_sel; q++) {
    if (S.sel[q] < 0 || S.sel[q] >= n || S.sel[q] == stop) return -1;
    out[m++] = S.sel[q];
  }
  return m;
}

void lf_sensor_free(lf_ctx* ctx) {
  LfSensorGhosts& S = ctx->sensor;
  if (S.table_dev) (void)hipFree(S.table_dev);
  if (S.stats_dev) (void)hipFree(S.stats_dev);
  S.table_dev = nullptr; S.stats_dev = nullptr; S.table_cap = 0; S.table_host.clear();
}

// The frame's sensor ghosts: every selected sensor path of every sample, added to what the ghost buffer holds (add: behind
// the ordinary march of the same lf_trace_ghosts) or, under LF_SENSOR_GHOSTS_ONLY, as lf_set_ghost_accumulate says.  The
// launch's geometry (band, deal, tile stride, sample groups) is the ordinary unculled launch's (lf_march_launch_args).
lf_status lfk_march_sensor(lf_ctx* ctx, int spp, uint64_t key, bool add) {
  LfSensorGhosts& S = ctx->sensor;
  int sel[LF_MAX_SURFACES];
  const int n_sel = lf_sensor_selection(ctx, sel);
  if (n_sel < 0) return lf_fail(ctx, LF_ERR_STATE, "lf_trace_ghosts: the sensor ghosts' selection does not fit the installed lens (lf_set_sensor_ghosts)");
  bool any = false;
  for (int l = 0; l < ctx->lens.n_lambda; l++) any = any || S.refl[l] != 0.0f;
  const LfApertureDev& m = ctx->ap[LF_APERTURE_STARBURST];
  ctx->lens.pitch = ctx->sensor_w_mm / (float)ctx->W;
  {
    const lf_status st = lf_march_lights_ready(ctx);
    if (st != LF_OK) return st;
  }
  if (!S.stats_dev) {
    LF_HIP(ctx, hipMalloc((void**)&S.stats_dev, kSensorStats * sizeof(unsigned long long)));
    LF_HIP(ctx, hipMemsetAsync(S.stats_dev, 0, kSensorStats * sizeof(unsigned long long), ctx->stream));
  }
  if (ctx->y1 <= ctx->y0) return LF_OK;

  // the ordinary unculled launch's arguments: the same band, deal, wave tiles and sample groups by construction
  MarchArgs a;
  size_t tiles;
  if (!lf_march_launch_args(ctx, spp, key, false, &a, &tiles)) return LF_OK;
  a.accumulate = (add || ctx->ghost_accumulate) ? 1 : 0;
  a.n_tiles = (int)tiles;
  const size_t blocks = ((tiles + 63) / 64 * 64) * a.sgroups;
  if (blocks > 0x7fffffffull) return lf_fail(ctx, LF_ERR_INVALID, "band too large for one launch");

  // the lens as this launch sees it: the default disc, and the lights on the fixed-point grid.  Under ADD that is the grid of
  // the ordinary launch that has just run (ctx->march_fix_bits, which stays what that launch set); ONLY sizes its own.  Both
  // are 36 bits for every light that is not HDR.  The HDR exception: should the sensor paths' own sums not fit the ordinary
  // launch's grid (fewer ordinary paths than sensor paths, or a reduced pupil target against the default disc's larger
  // geom_norm), the coarser grid is taken -- the sums must not overflow -- and ADD then equals ordinary + ONLY to that
  // grid's quantum per contribution instead of bit for bit.
  LfLensDev up = ctx->lens;
  default_disc(ctx, up);
  a.vz = up.pupil_z - up.z_sensor;
  const int own_bits = lf_march_fix_bits(up, n_sel, spp);
  const int bits = add ? std::min(ctx->march_fix_bits, own_bits) : own_bits;
  if (!add) ctx->march_fix_bits = bits;
  SensorArgs sa;
  sa.xmax = a.half_w * up.pitch; sa.ymax = a.half_h * up.pitch;
  sa.inv_scale = std::ldexp(1.0, -bits);

  if (!any) {   // the sensor reflects nothing at any wavelength: nothing is launched; a replacing launch leaves zeros
    if (!a.accumulate) {
      const size_t px = (size_t)(ctx->y1 - ctx->y0) * ctx->W;
      hipLaunchKernelGGL(k_sensor_zero, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, ctx->stream, a, ctx->ghost);
      LF_HIP(ctx, hipGetLastError());
    }
    return LF_OK;
  }
  {
    const lf_status st = sensor_table_upload(ctx, sel, n_sel);
    if (st != LF_OK) return st;
  }
  {
    const lf_status st = lf_march_upload_lens(ctx, up, bits);
    if (st != LF_OK) return st;
  }
  if (a.sgroups > 1) {
    const size_t n_acc = (size_t)ctx->W * ctx->H_alloc * 3;
    if (!ctx->accum) LF_HIP(ctx, hipMalloc((void**)&ctx->accum, n_acc * sizeof(unsigned long long)));
    LF_HIP(ctx, hipMemsetAsync(ctx->accum + (size_t)ctx->y0 * ctx->W * 3, 0,
                               (size_t)(ctx->y1 - ctx->y0) * ctx->W * 3 * sizeof(unsigned long long), ctx->stream));
  }

  // the general light variant alone, crossed with occlusion, the bilinear stop and films: lfk_march_asph's eight
  constexpr int kGen = kVarLights | kVarNear | kVarArea;
  const int var = kGen | (ctx->ghost_occlusion ? kVarOccl : 0) | (ctx->mask_filter == LF_MASK_BILINEAR ? kVarFilt : 0) |
                  (ctx->coat.n > 0 ? (kVarCoat | kVarStack) : 0);
  const int surf = surf_kind(ctx);
  hipEvent_t ev = lf_timing_begin(ctx, LFK_MARCH_SENSOR);
#define LF_LAUNCH_SENSOR(VV)                                                                                             \
  do {                                                                                                                   \
    if (surf == 3) LF_LAUNCH_SENSOR2(VV, 3); else if (surf == 2) LF_LAUNCH_SENSOR2(VV, 2);                               \
    else if (surf == 1) LF_LAUNCH_SENSOR2(VV, 1); else LF_LAUNCH_SENSOR2(VV, 0);                                         \
  } while (0)
#define LF_LAUNCH_SENSOR2(VV, SS)                                                                                        \
  hipLaunchKernelGGL((k_march_sensor<VV, SS>), dim3((unsigned)blocks), dim3(64 * kSensorWgWaves), 0, ctx->stream, ctx->lens_dev, \
                     (const unsigned char*)S.table_dev, m.texels, a, sa, ctx->ghost, ctx->accum, S.stats_dev)
  switch (var) {
    case kGen: LF_LAUNCH_SENSOR(kGen); break;
    case kGen | kVarFilt: LF_LAUNCH_SENSOR(kGen | kVarFilt); break;
    case kGen | kVarCoat | kVarStack: LF_LAUNCH_SENSOR(kGen | kVarCoat | kVarStack); break;
    case kGen | kVarCoat | kVarStack | kVarFilt: LF_LAUNCH_SENSOR(kGen | kVarCoat | kVarStack | kVarFilt); break;
    case kGen | kVarOccl: LF_LAUNCH_SENSOR(kGen | kVarOccl); break;
    case kGen | kVarOccl | kVarFilt: LF_LAUNCH_SENSOR(kGen | kVarOccl | kVarFilt); break;
    case kGen | kVarOccl | kVarCoat | kVarStack: LF_LAUNCH_SENSOR(kGen | kVarOccl | kVarCoat | kVarStack); break;
    default: LF_LAUNCH_SENSOR(kGen | kVarOccl | kVarCoat | kVarStack | kVarFilt); break;
  }
#undef LF_LAUNCH_SENSOR
#undef LF_LAUNCH_SENSOR2
  lf_timing_end(ctx, LFK_MARCH_SENSOR, ev);
  LF_HIP(ctx, hipGetLastError());
  if (a.sgroups > 1) {
    const size_t px = (size_t)(ctx->y1 - ctx->y0) * ctx->W;
    hipLaunchKernelGGL(k_sensor_finish, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, ctx->stream, ctx->accum, a, sa, ctx->ghost);
    LF_HIP(ctx, hipGetLastError());
  }
  return LF_OK;
}

lf_status lfk_march_sensor_path_rays(lf_ctx* ctx, int lambda, int i, int n, const float* d_xy, const float* d_uv, float* d_out) {
  const LfApertureDev& m = ctx->ap[LF_APERTURE_STARBURST];
  ctx->lens.pitch = ctx->sensor_w_mm / (float)std::max(1, ctx->W);
  const LfLensDev& L = ctx->lens;
  if (3 * L.n_surf - 2 * i > kPathRowsMax) return lf_fail(ctx, LF_ERR_STATE, "lf_march_sensor_path_rays: the path's rows exceed their table");
  // (SURF = 3: the pose block behind the table and its stack records, from a 64-byte boundary on -- one record per posed interface)
  const bool posed = surf_kind(ctx) == 3;
  const size_t pose_off = posed ? (sizeof(LfPathDev) + kPathStackBytes + 63) & ~(size_t)63 : 0;
  std::vector<unsigned char> buf(posed ? pose_off + (size_t)ctx->pose.n * sizeof(LfPoseRec) : sizeof(LfPathDev) + kPathStackBytes, 0);
  LfPathDev& P = *reinterpret_cast<LfPathDev*>(buf.data());
  P.inv_stop_h = 1.0f / L.stop_h;
  P.front_zv = L.surf[0].zv;
  P.n_start = L.n_start[lambda];
  size_t next_stack = sizeof(LfPathDev);
  if (sensor_path_rows(ctx, lambda, i, buf.data(), offsetof(LfPathDev, row), &next_stack, sizeof(LfPathDev) + kPathStackBytes, pose_off, &P.n) != LF_OK)
    return lf_fail(ctx, LF_ERR_STATE, "lf_march_sensor_path_rays: the path's rows exceed their table");
  if (posed) pose_block_fill(ctx, buf.data() + pose_off);
  LfLensDev up = ctx->lens;
  default_disc(ctx, up);
  SensorArgs sa;
  sa.xmax = (0.5f * (float)ctx->W) * up.pitch; sa.ymax = (0.5f * (float)ctx->H) * up.pitch;
  sa.inv_scale = 0.0;
  unsigned char* d_tab = nullptr;
  LF_HIP(ctx, hipMalloc((void**)&d_tab, buf.size()));
  hipError_t e = hipMemcpy(d_tab, buf.data(), buf.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpyAsync(ctx->lens_dev, &up, sizeof(LfLensDev), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    const bool filt = ctx->mask_filter == LF_MASK_BILINEAR, coat = ctx->coat.n > 0;
    const int surf = surf_kind(ctx);
#define LF_LAUNCH_SPATH(FF, CC, SS)                                                                                           \
  hipLaunchKernelGGL((k_march_sensor_path_rays<FF, CC, SS>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,    \
                     ctx->lens_dev, (const LfPathDev*)d_tab, m.texels, m.w, m.h, sa, n, d_xy, d_uv, d_out)
#define LF_LAUNCH_SPATH2(FF, CC)                                                                                              \
  do {                                                                                                                        \
    if (surf == 3) LF_LAUNCH_SPATH(FF, CC, 3); else if (surf == 2) LF_LAUNCH_SPATH(FF, CC, 2);                                \
    else if (surf == 1) LF_LAUNCH_SPATH(FF, CC, 1); else LF_LAUNCH_SPATH(FF, CC, 0);                                          \
  } while (0)
    if (filt && coat) LF_LAUNCH_SPATH2(true, true);
    else if (filt) LF_LAUNCH_SPATH2(true, false);
    else if (coat) LF_LAUNCH_SPATH2(false, true);
    else LF_LAUNCH_SPATH2(false, false);
#undef LF_LAUNCH_SPATH
#undef LF_LAUNCH_SPATH2
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (the table is this call's own)
  (void)hipFree(d_tab);
  LF_HIP(ctx, e);
  return LF_OK;
}
