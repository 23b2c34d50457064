// lf_march_asph.hip -- the geometric lens with aspheric interfaces (lf_set_lens_aspheres; DESIGN.md section 4, "aspheres").
//   k_march_asph<VAR>      the frame of a lens with an aspheric record: every path of every sample marched alone from the
//                          sensor along its own flat sequence (the form of k_march_items / "cull_no_prefix", never the path
//                          tree), geometry first, the weighted march again only for the lanes the lights' pre-test admits,
//                          lit rays through lights_epilogue -- so every kind of light, several lights, ghost occlusion and
//                          both reaches are the code that exists.  A row whose sequence dword carries LF_EV_ASPH takes
//                          asphere_event (lf_asphere.h) behind a wave-uniform branch, every other row surface_event, bit for
//                          bit as in the other kernels.  Launched iff the lens has a record (or under "asph_force").
//   k_march_asph<VAR, true> the same kernel for a lens with a BICONIC record (lf_set_lens_biconics; lf_biconic.h): one more
//                          wave-uniform branch, on LF_EV_BICONIC, to biconic_event.  BIC = false is the code it was.
//   k_asphere_events       lf_asphere_events: one event for n rays, the device twin of lf_asphere_event
//   k_march_asph<VAR, true, true> the same kernel for a lens with a POSE record (lf_set_lens_poses; lf_pose.h): one more
//                          wave-uniform branch, on LF_EV_POSE, to pose_event.  POSE = false is the code it was.
//   k_biconic_events       lf_biconic_events: the device twin of lf_biconic_event
//   k_pose_events          lf_pose_events: the device twin of lf_pose_event
//   k_march_path_rays      lf_march_path_rays: one explicit ray per lane along the sequence of pair (i, j), with its weight
// The sample starts are sample_start's (lf_march_events.h): the path tree's rays for the same inputs, bit for bit.
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

using namespace lfm;

namespace {

constexpr int kAsphWgWaves = 8;

// a record of the aspheric table: ONE 32-byte scalar load (the offset is wave-uniform)
__device__ __forceinline__ LfAsphRec load_asph(const LfAsphRec* __restrict__ base, unsigned off) {
  typedef const char __attribute__((address_space(4))) * cptr;
  const lf_i8 v = *(const lf_i8 __attribute__((address_space(4)))*)((cptr)(base) + off);
  LfAsphRec r;
  r.kappa = __int_as_float(v[0]);
#pragma unroll
  for (int m = 0; m < 6; m++) r.a[m] = __int_as_float(v[1 + m]);
  r.spare = 0.0f;
  return r;
}

// (a record of the pose table: load_pose, lf_pose.h)

struct AsphTally {
  unsigned long long n_rays = 0, events = 0, n_clip = 0, n_vign = 0, n_tir = 0, n_scene = 0, n_rm_lane = 0, n_rm_rows = 0;
  unsigned n_light = 0;   // per lane
};

// One row of a path for wavelength slot j of its group, W as surface_event's: the stop, an aspheric row, or the spherical
// event.  *stop: the row was the stop (its dead lanes count as clipped).
template <bool W, int VAR, bool BIC = false, bool POSE = false>
__device__ __forceinline__ lanemask asph_row(Ray& r, unsigned cur, int j, const LfProgRow* __restrict__ recs,
                                             const LfWeightRow* __restrict__ wrecs, const LfWeightRow* __restrict__ wrec_table,
                                             const LfAsphRec* __restrict__ asph_table, const float* __restrict__ mask,
                                             float inv_stop_h, int mw, int mh, lanemask& geom_ok, bool& stop,
                                             const LfPoseRec* __restrict__ pose_table = nullptr) {
  const unsigned off = cur & 0xffffu, kind = cur >> 16;
  const LfProgRow wr = load_prec(recs, off);
  stop = (kind & LF_EV_STOP) != 0u;
  if (stop) {
    const lanemask ok = stop_event_var<W, VAR>(r, wr.dzv, wr.h2, inv_stop_h, mask, mw, mh);
    geom_ok = ok;
    return ok;
  }
  float fs = 1.0f, fo = 1.0f, fi = 1.0f;
  int coat = 0;
  if (W) {
    const char* const wj = (const char*)wrecs + 4 * j;
    fs = __int_as_float(load_wrec_dword(wj, off + (unsigned)offsetof(LfWeightRow, fs)));
    fo = __int_as_float(load_wrec_dword(wj, off + (unsigned)offsetof(LfWeightRow, fo)));
    fi = __int_as_float(load_wrec_dword(wj, off + (unsigned)offsetof(LfWeightRow, fi)));
    if (VAR & kVarCoat) coat = load_wrec_dword(wrecs, off + (unsigned)offsetof(LfWeightRow, coat));
  }
  const float delta = j == 0 ? wr.delta[0] : j == 1 ? wr.delta[1] : wr.delta[2];
  if (POSE && (kind & LF_EV_POSE)) {   // wave-uniform: a pose record at the program record's offset of the table behind the aspheric one
    const LfAsphRec rec = load_asph(asph_table, off >> 1);
    const LfPoseRec pose = load_pose(pose_table, off);
    return pose_event<W>(r, wr.dzv, wr.curv, (kind & LF_EV_ASPH) != 0u, rec, pose, delta, wr.h2, (kind & LF_EV_REFLECT) != 0, wr.sgn,
                         geom_ok, fs, fo, fi, CoatSel<VAR>{wrec_table, coat, j});
  }
  if (BIC && (kind & LF_EV_BICONIC)) {   // wave-uniform: a biconic record in the aspheric record's slot
    const LfAsphRec rec = load_asph(asph_table, off >> 1);
    return biconic_event<W>(r, wr.dzv, wr.curv, LfBicRec{rec.kappa, rec.a[0], rec.a[1], {}}, delta, wr.h2,
                            (kind & LF_EV_REFLECT) != 0, wr.sgn, geom_ok, fs, fo, fi, CoatSel<VAR>{wrec_table, coat, j});
  }
  if (kind & LF_EV_ASPH) {   // wave-uniform: the interface has a record (one per program record: 32 of its 64 bytes' offset)
    const LfAsphRec rec = load_asph(asph_table, off >> 1);
    return asphere_event<W>(r, wr.dzv, wr.curv, rec, delta, wr.h2, (kind & LF_EV_REFLECT) != 0, wr.sgn, geom_ok, fs, fo, fi,
                            CoatSel<VAR>{wrec_table, coat, j});
  }
  const float cn22 = j == 0 ? wr.cn22[0] : j == 1 ? wr.cn22[1] : wr.cn22[2];
  const float rn2 = j == 0 ? wr.rn2[0] : j == 1 ? wr.rn2[1] : wr.rn2[2];
  return surface_event<W>(r, wr.dzv, wr.curv, wr.ch, wr.c2, wr.sc, cn22, rn2, delta, wr.h2, (kind & LF_EV_REFLECT) != 0,
                          (kind & LF_EV_FLAT) != 0, wr.sgn, geom_ok, fs, fo, fi, CoatSel<VAR>{wrec_table, coat, j});
}

// path q of one sensor sample per lane, every wavelength on its own: geometry, tallies, the lights' pre-test, the weighted
// march of the lit lanes, the lit epilogue into the tile's LDS sums
template <int VAR, bool BIC = false, bool POSE = false>
__device__ __forceinline__ void march_asph_path(const LfLensDev* __restrict__ lens, const LfPairsDev* __restrict__ pairs,
                                                const int* __restrict__ seq_table, const LfProgRow* __restrict__ rec_table,
                                                const LfWeightRow* __restrict__ wrec_table,
                                                const LfAsphRec* __restrict__ asph_table, const float* __restrict__ mask,
                                                const MarchArgs& a, int K, int q, lanemask start_mask, const StartRay& s0, int lane,
                                                unsigned long long* __restrict__ s_acc, const float* __restrict__ s_chan,
                                                AsphTally& T) {
  const int n_lambda = lens->n_lambda, prog_recs = pairs->prog_recs;
  // (the pose table lies behind the aspheric one: lf_pose_table_offset)
  const LfPoseRec* const pose_table = POSE ? (const LfPoseRec*)((const char*)asph_table + lf_pose_table_offset(prog_recs)) : nullptr;
  const int n_ev = pairs->ev_cnt[q];
  typedef const int __attribute__((address_space(4))) * sptr;
  const sptr seq = (sptr)(seq_table + pairs->ev_off[q]);
  for (int l = 0; l < n_lambda; l++) {
    const int g = l / K, j = l - g * K;
    const LfProgRow* const recs = rec_table + (size_t)g * (size_t)prog_recs;
    const LfWeightRow* const wrecs = wrec_table + (size_t)g * (size_t)prog_recs;
    const float ns = lens->n_start[l];
    Ray r[1];
    r[0] = Ray{s0.X, s0.Y, 0.0f, fmaf(s0.X, s0.X, s0.Y * s0.Y), s0.dx * ns, s0.dy * ns, s0.dz * ns, s0.w0, 1.0f};
    lanemask alive[1] = {start_mask};
    unsigned nlive = (unsigned)__popcll(start_mask);
    T.n_rays += nlive;
    unsigned ev32 = 0u;
    for (int e = 0; e < n_ev && nlive != 0u; e++) {
      lanemask gv;
      bool stop;
      const lanemask ok = asph_row<false, VAR, BIC, POSE>(r[0], (unsigned)seq[e], j, recs, wrecs, wrec_table, asph_table, mask,
                                                          a.inv_stop_h, a.mw, a.mh, gv, stop, pose_table);
      const lanemask died = alive[0] & ~ok;
      if (died != 0ull) {
        if (stop) T.n_clip += (unsigned)__popcll(died);
        else {
          T.n_vign += (unsigned)__popcll(alive[0] & ~gv);
          T.n_tir += (unsigned)__popcll(alive[0] & gv & ~ok);
        }
        nlive -= (unsigned)__popcll(died);
        alive[0] &= ok;
      }
      ev32 += nlive;
    }
    T.events += ev32;
    if (nlive == 0u) continue;
    T.n_scene += nlive;
    lanemask lit[1];
    if (lights_pretest<1, true, VAR>(lens, r, alive, lit) == 0ull) continue;
    // the path again with its weight: the same arithmetic on the ray, so the same ray bit for bit
    Ray rw{s0.X, s0.Y, 0.0f, fmaf(s0.X, s0.X, s0.Y * s0.Y), s0.dx * ns, s0.dy * ns, s0.dz * ns, s0.w0, 1.0f};
    T.n_rm_lane += (unsigned long long)((unsigned)n_ev * (unsigned)__popcll(lit[0]));
    T.n_rm_rows += (unsigned)n_ev;
    for (int e = 0; e < n_ev; e++) {
      lanemask gv;
      bool stop;
      (void)asph_row<true, VAR, BIC, POSE>(rw, (unsigned)seq[e], j, recs, wrecs, wrec_table, asph_table, mask, a.inv_stop_h, a.mw, a.mh,
                                           gv, stop, pose_table);
    }
    lights_epilogue<VAR>(lens, s_chan, rw, ((lit[0] >> lane) & 1ull) != 0ull, l, &s_acc[lane * 3], T.n_light);
  }
}

template <int VAR, bool BIC = false, bool POSE = false>
__global__ __launch_bounds__(64 * kAsphWgWaves) void k_march_asph(
    const LfLensDev* __restrict__ lens, const LfPairsDev* __restrict__ pairs, const int* __restrict__ seq_table,
    const LfProgRow* __restrict__ rec_table, const LfWeightRow* __restrict__ wrec_table,
    const LfAsphRec* __restrict__ asph_table, const float* __restrict__ mask, MarchArgs a, int K, double* __restrict__ ghost,
    unsigned long long* __restrict__ accum, unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long s_acc[64 * 3];
  __shared__ unsigned long long s_cnt[kMarchCounters];
  __shared__ int s_next;
  __shared__ float s_chan[kLightChan];
  const int tid = threadIdx.x;
  if (tid < 64 * 3) s_acc[tid] = 0ull;
  lights_channel_factors(lens, s_chan, tid, 64 * kAsphWgWaves);
  if (tid < kMarchCounters) s_cnt[tid] = 0ull;
  if (tid == 0) s_next = 0;
  __syncthreads();

  // the workgroup's wave tile and its share of the samples: as k_march_cull (8 rows x 8 columns 2^xs apart)
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

  AsphTally T;
  const int n_mine = (a.spp - sg + sgroups - 1) / sgroups;     // samples sg, sg + sgroups, ...
  const int n_paths = pairs->n;
  if (active_mask != 0ull)
    for (;;) {
      int k = 0;
      if (lane == 0) k = atomicAdd(&s_next, 1);
      k = __builtin_amdgcn_readfirstlane(k);
      if (k >= n_mine) break;
      const int s = sg + k * sgroups;       // wave-uniform
      const StartRay s0 = sample_start(spec, x, y, s);
      for (int q = 0; q < n_paths; q++)
        march_asph_path<VAR, BIC, POSE>(lens, pairs, seq_table, rec_table, wrec_table, asph_table, mask, a, K, q, active_mask, s0, lane, s_acc,
                             s_chan, T);
    }

  // ---- counters: one LDS add per wave, one global add per workgroup (the slots of k_march_cull; executed = events) ----
  {
    unsigned long long v6 = T.n_light;
    for (int off = 32; off > 0; off >>= 1) v6 += __shfl_down(v6, off);
    const unsigned long long vals[kMarchCounters] = {T.n_rays, T.events, T.n_clip, T.n_vign, T.n_tir, T.n_scene, v6, T.events, T.n_rm_lane, T.n_rm_rows};
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kMarchCounters; i++)
        if (vals[i]) atomicAdd(&s_cnt[i], vals[i]);
    }
  }
  __syncthreads();
  if (wave == 0 && lane < kMarchCounters && s_cnt[lane]) atomicAdd(&counters[lane], s_cnt[lane]);
  if (wave == 0 && active) {
    if (a.sgroups == 1) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double v = ((double)s_acc[lane * 3 + c] * (1.0 / 68719476736.0)) / (double)a.spp;
        ghost[3 * (size_t)p + c] = a.accumulate ? ghost[3 * (size_t)p + c] + v : v;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++)
        if (s_acc[lane * 3 + c]) atomicAdd(&accum[3 * (size_t)p + c], s_acc[lane * 3 + c]);
    }
  }
}

// ---- lf_asphere_events: the host's lf_asphere_event, n times ------------------------------------------------------------
struct AsphEventArgs { float k[16]; };   // {c, delta, h2, sgn, dzv, 0, 0, 0, record}
__global__ __launch_bounds__(256) void k_asphere_events(AsphEventArgs c, int reflect, int n, const float* __restrict__ rays,
                                                        float* __restrict__ out, int* __restrict__ fates) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  LfAsphRec rec;
  rec.kappa = c.k[8];
#pragma unroll
  for (int m = 0; m < 6; m++) rec.a[m] = c.k[9 + m];
  rec.spare = 0.0f;
  const float* ri = rays + 6 * (size_t)i;
  float px = ri[0], py = ri[1], hz = ri[2], dx = ri[3], dy = ri[4], dz = ri[5], r2;
  const AsphHit h = lf_asph_event(px, py, hz, r2, dx, dy, dz, c.k[4], c.k[0], rec, c.k[1], c.k[2], reflect != 0, c.k[3]);
  float* o = out + 8 * (size_t)i;
  o[0] = px; o[1] = py; o[2] = hz; o[3] = dx; o[4] = dy; o[5] = dz; o[6] = h.sq; o[7] = h.ct;
  fates[i] = h.fate;
}

// ---- lf_biconic_events: the host's lf_biconic_event, n times; {cy, delta, h2, sgn, dzv, 0, 0, 0, cx, kx, ky, 0 ...} -----------
__global__ __launch_bounds__(256) void k_biconic_events(AsphEventArgs c, int reflect, int n, const float* __restrict__ rays,
                                                        float* __restrict__ out, int* __restrict__ fates) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const LfBicRec rec{c.k[8], c.k[9], c.k[10], {}};
  const float* ri = rays + 6 * (size_t)i;
  float px = ri[0], py = ri[1], hz = ri[2], dx = ri[3], dy = ri[4], dz = ri[5], r2;
  const AsphHit h = lf_bic_event(px, py, hz, r2, dx, dy, dz, c.k[4], c.k[0], rec, c.k[1], c.k[2], reflect != 0, c.k[3]);
  float* o = out + 8 * (size_t)i;
  o[0] = px; o[1] = py; o[2] = hz; o[3] = dx; o[4] = dy; o[5] = dz; o[6] = h.sq; o[7] = h.ct;
  fates[i] = h.fate;
}

// ---- lf_pose_events: the host's lf_pose_event, n times; the sixteen constants of lf_asphere_events (asph) or of
// lf_biconic_events, and the pose {R row-major, t, 0 ...} ------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pose_events(AsphEventArgs c, AsphEventArgs pose, int reflect, int asph, int n,
                                                     const float* __restrict__ rays, float* __restrict__ out,
                                                     int* __restrict__ fates) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  LfAsphRec ka;
  ka.kappa = c.k[8];
#pragma unroll
  for (int m = 0; m < 6; m++) ka.a[m] = c.k[9 + m];
  ka.spare = 0.0f;
  const LfBicRec kb{c.k[8], c.k[9], c.k[10], {}};
  LfPoseRec p;
#pragma unroll
  for (int m = 0; m < 9; m++) p.r[m] = pose.k[m];
#pragma unroll
  for (int m = 0; m < 3; m++) p.t[m] = pose.k[9 + m];
#pragma unroll
  for (int m = 0; m < 4; m++) p.spare[m] = 0.0f;
  const float* ri = rays + 6 * (size_t)i;
  float px = ri[0], py = ri[1], hz = ri[2], dx = ri[3], dy = ri[4], dz = ri[5], r2;
  const AsphHit h = lf_pose_event(px, py, hz, r2, dx, dy, dz, c.k[4], c.k[0], asph != 0, ka, kb, p, c.k[1], c.k[2], reflect != 0, c.k[3]);
  float* o = out + 8 * (size_t)i;
  o[0] = px; o[1] = py; o[2] = hz; o[3] = dx; o[4] = dy; o[5] = dz; o[6] = h.sq; o[7] = h.ct;
  fates[i] = h.fate;
}

// ---- lf_march_path_rays: the sequence of pair (i, j) for ONE wavelength, one row per event (lf_path_table.h; host: build_path_table) ----
// (POSE: the rows' pose records lie behind the table and its stack records, at kPathPoseOffset, one per row)
constexpr size_t kPathPoseOffset = (sizeof(LfPathDev) + kPathStackBytes + 63) & ~(size_t)63;
template <bool FILT, bool COAT, bool BIC = false, bool POSE = false>
__global__ __launch_bounds__(256) void k_march_path_rays(const LfLensDev* __restrict__ lens, const LfPathDev* __restrict__ P,
                                                         const float* __restrict__ mask, int mw, int mh, int n,
                                                         const float* __restrict__ sensor_xy, const float* __restrict__ pupil_uv,
                                                         float* __restrict__ out) {
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
    } else if (POSE && (w.kind & LF_EV_POSE)) {   // wave-uniform
      const LfPoseRec pose = load_pose((const LfPoseRec*)((const char*)P + kPathPoseOffset), (unsigned)e * (unsigned)sizeof(LfPoseRec));
      const bool asph = (w.kind & LF_EV_ASPH) != 0;
      if (COAT) ok = pose_event<true>(r, w.dzv, w.curv, asph, w.asph, pose, w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi, PathCoat{&w});
      else ok = pose_event<true>(r, w.dzv, w.curv, asph, w.asph, pose, w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi);
    } else if (BIC && (w.kind & LF_EV_BICONIC)) {
      const LfBicRec rec{w.asph.kappa, w.asph.a[0], w.asph.a[1], {}};
      if (COAT) ok = biconic_event<true>(r, w.dzv, w.curv, rec, w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi, PathCoat{&w});
      else ok = biconic_event<true>(r, w.dzv, w.curv, rec, w.delta, w.h2, reflect, w.sgn, geom_ok, w.fs, w.fo, w.fi);
    } else if (w.kind & LF_EV_ASPH) {
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

// host: the rows of pair (i, j) at wavelength l -- the order of lf_build_march_tables, the constants of pack_program
lf_status build_path_table(lf_ctx* ctx, int l, int i, int j, std::vector<unsigned char>& buf) {
  const LfLensDev& L = ctx->lens;
  const LfPoses& Po = ctx->pose;
  buf.assign(Po.n > 0 ? kPathPoseOffset + (size_t)kPathRowsMax * sizeof(LfPoseRec) : sizeof(LfPathDev) + kPathStackBytes, 0);
  LfPathDev& P = *reinterpret_cast<LfPathDev*>(buf.data());
  size_t next_stack = sizeof(LfPathDev);
  P.n = 0;
  P.inv_stop_h = 1.0f / L.stop_h;
  P.front_zv = L.surf[0].zv;
  P.n_start = L.n_start[l];
  lf_status st = LF_OK;
  auto put = [&](int k, int from, bool reflect, bool fwd) {
    if (P.n >= kPathRowsMax) { st = LF_ERR_STATE; return; }
    const size_t row_off = (size_t)((const unsigned char*)&P.row[P.n++] - buf.data());
    if (lf_path_row_fill(ctx, l, k, from, reflect, fwd, buf.data(), row_off, &next_stack, sizeof(LfPathDev) + kPathStackBytes) != LF_OK)
      st = LF_ERR_STATE;
    if (Po.n > 0 && Po.on[k] && L.surf[k].is_stop == 0.0f) {   // a posed row: its record, and which event runs in its frame
      LfPathRow& w = P.row[P.n - 1];
      w.kind |= LF_EV_POSE;
      if (!(w.kind & LF_EV_BICONIC) && !(w.kind & LF_EV_ASPH && ctx->asph.n > 0)) {   // a sphere or a plane: as a biconic
        w.kind = (w.kind & ~LF_EV_ASPH) | LF_EV_BICONIC;
        w.asph = LfAsphRec{};
        w.asph.kappa = L.surf[k].curv;
      }
      const LfPoseRec rec = lf_pose_make(Po.t[3 * k], Po.t[3 * k + 1], Po.t[3 * k + 2], Po.a[3 * k], Po.a[3 * k + 1], Po.a[3 * k + 2]);
      std::memcpy(buf.data() + kPathPoseOffset + (size_t)(P.n - 1) * sizeof(rec), &rec, sizeof(rec));
    }
  };
  if (i < 0) {
    for (int k = L.n_surf - 1; k >= 0; k--) put(k, k + 1, false, false);
  } else {
    for (int k = L.n_surf - 1; k > i; k--) put(k, k + 1, false, false);
    put(i, i + 1, true, false);
    for (int k = i + 1; k < j; k++) put(k, k == i + 1 ? i : k - 1, false, true);
    put(j, j == i + 1 ? i : j - 1, true, true);
    for (int k = j - 1; k >= 0; k--) put(k, k + 1, false, false);
  }
  if (st != LF_OK) return lf_fail(ctx, st, "lf_march_path_rays: the path's rows exceed their table");
  return LF_OK;
}

}  // namespace

lf_status lfk_asphere_events(lf_ctx* ctx, const float* consts16, int reflect, int forward, size_t n, const float* d_rays,
                             float* d_out, int* d_fates) {
  (void)forward;   // (in consts16[3])
  AsphEventArgs c;
  std::memcpy(c.k, consts16, sizeof(c.k));
  hipLaunchKernelGGL(k_asphere_events, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, c, reflect, (int)n, d_rays,
                     d_out, d_fates);
  LF_HIP(ctx, hipGetLastError());
  return LF_OK;
}

lf_status lfk_biconic_events(lf_ctx* ctx, const float* consts16, int reflect, size_t n, const float* d_rays, float* d_out,
                             int* d_fates) {
  AsphEventArgs c;
  std::memcpy(c.k, consts16, sizeof(c.k));
  hipLaunchKernelGGL(k_biconic_events, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, c, reflect, (int)n, d_rays,
                     d_out, d_fates);
  LF_HIP(ctx, hipGetLastError());
  return LF_OK;
}

lf_status lfk_pose_events(lf_ctx* ctx, const float* consts16, const float* pose16, int reflect, int asph, size_t n,
                          const float* d_rays, float* d_out, int* d_fates) {
  AsphEventArgs c, p;
  std::memcpy(c.k, consts16, sizeof(c.k));
  std::memcpy(p.k, pose16, sizeof(p.k));
  hipLaunchKernelGGL(k_pose_events, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, c, p, reflect, asph, (int)n,
                     d_rays, d_out, d_fates);
  LF_HIP(ctx, hipGetLastError());
  return LF_OK;
}

lf_status lfk_march_path_rays(lf_ctx* ctx, int lambda, int i, int j, int n, const float* d_xy, const float* d_uv, float* d_out) {
  const LfApertureDev& m = ctx->ap[LF_APERTURE_STARBURST];
  ctx->lens.pitch = ctx->sensor_w_mm / (float)std::max(1, ctx->W);
  std::vector<unsigned char> buf;
  lf_status st = build_path_table(ctx, lambda, i, j, buf);
  if (st != LF_OK) return st;
  unsigned char* d_tab = nullptr;
  LF_HIP(ctx, hipMalloc((void**)&d_tab, buf.size()));
  hipError_t e = hipMemcpy(d_tab, buf.data(), buf.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpyAsync(ctx->lens_dev, &ctx->lens, sizeof(LfLensDev), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    const bool filt = ctx->mask_filter == LF_MASK_BILINEAR, coat = ctx->coat.n > 0;
#define LF_LAUNCH_PATH(FF, CC, BB) LF_LAUNCH_PATH2(FF, CC, BB, false)
#define LF_LAUNCH_PATH2(FF, CC, BB, PP)                                                                                 \
  hipLaunchKernelGGL((k_march_path_rays<FF, CC, BB, PP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,    \
                     ctx->lens_dev, (const LfPathDev*)d_tab, m.texels, m.w, m.h, n, d_xy, d_uv, d_out)
    if (lf_march_posed(ctx)) {   // (a lens with a pose record: the instantiations that know both branches)
      if (filt && coat) LF_LAUNCH_PATH2(true, true, true, true);
      else if (filt) LF_LAUNCH_PATH2(true, false, true, true);
      else if (coat) LF_LAUNCH_PATH2(false, true, true, true);
      else LF_LAUNCH_PATH2(false, false, true, true);
    } else if (lf_march_biconic(ctx)) {   // (a lens with a biconic record: the instantiations that know the branch)
      if (filt && coat) LF_LAUNCH_PATH(true, true, true);
      else if (filt) LF_LAUNCH_PATH(true, false, true);
      else if (coat) LF_LAUNCH_PATH(false, true, true);
      else LF_LAUNCH_PATH(false, false, true);
    } else if (filt && coat) LF_LAUNCH_PATH(true, true, false);
    else if (filt) LF_LAUNCH_PATH(true, false, false);
    else if (coat) LF_LAUNCH_PATH(false, true, false);
    else LF_LAUNCH_PATH(false, false, false);
#undef LF_LAUNCH_PATH
#undef LF_LAUNCH_PATH2
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);   // (the table is this call's own)
  (void)hipFree(d_tab);
  LF_HIP(ctx, e);
  return LF_OK;
}

// The frame: instantiated for the GENERAL light variant alone (kVarLights | kVarNear | kVarArea decides a light's kind at run
// time), crossed with occlusion, the bilinear stop and films (general: kVarCoat | kVarStack) -- eight kernels.
lf_status lfk_march_asph(lf_ctx* ctx, const MarchArgs& a, size_t blocks) {
  if (ctx->prog_asph_off == 0) return lf_fail(ctx, LF_ERR_STATE, "aspheric march: the program holds no aspheric records");
  const LfApertureDev& m = ctx->ap[LF_APERTURE_STARBURST];
  constexpr int kGen = kVarLights | kVarNear | kVarArea;
  const int var = kGen | (ctx->ghost_occlusion ? kVarOccl : 0) | (ctx->mask_filter == LF_MASK_BILINEAR ? kVarFilt : 0) |
                  (ctx->coat.n > 0 ? (kVarCoat | kVarStack) : 0);
  const bool bic = lf_march_biconic(ctx);   // (a biconic record: the same kernel with the branch that knows it)
  const bool posed = lf_march_posed(ctx);   // (a pose record: ... with both branches)
  hipEvent_t ev = lf_timing_begin(ctx, LFK_MARCH);
#define LF_LAUNCH_ASPH(VV)                                                                                               \
  if (posed) LF_LAUNCH_ASPH2(VV, true, true); else if (bic) LF_LAUNCH_ASPH2(VV, true, false); else LF_LAUNCH_ASPH2(VV, false, false)
#define LF_LAUNCH_ASPH2(VV, BB, PP)                                                                                      \
  hipLaunchKernelGGL((k_march_asph<VV, BB, PP>), dim3((unsigned)blocks), dim3(64 * kAsphWgWaves), 0, ctx->stream, ctx->lens_dev,  \
                     ctx->pairs_dev, (const int*)(ctx->prog_dev + ctx->prog_seq_off),                                    \
                     (const LfProgRow*)(ctx->prog_dev + ctx->prog_rec_off),                                              \
                     (const LfWeightRow*)(ctx->prog_dev + ctx->prog_wrec_off),                                           \
                     (const LfAsphRec*)(ctx->prog_dev + ctx->prog_asph_off), m.texels, a, ctx->march_k, ctx->ghost,      \
                     ctx->accum, ctx->counters_dev)
  switch (var) {
    case kGen: LF_LAUNCH_ASPH(kGen); break;
    case kGen | kVarFilt: LF_LAUNCH_ASPH(kGen | kVarFilt); break;
    case kGen | kVarCoat | kVarStack: LF_LAUNCH_ASPH(kGen | kVarCoat | kVarStack); break;
    case kGen | kVarCoat | kVarStack | kVarFilt: LF_LAUNCH_ASPH(kGen | kVarCoat | kVarStack | kVarFilt); break;
    case kGen | kVarOccl: LF_LAUNCH_ASPH(kGen | kVarOccl); break;
    case kGen | kVarOccl | kVarFilt: LF_LAUNCH_ASPH(kGen | kVarOccl | kVarFilt); break;
    case kGen | kVarOccl | kVarCoat | kVarStack: LF_LAUNCH_ASPH(kGen | kVarOccl | kVarCoat | kVarStack); break;
    default: LF_LAUNCH_ASPH(kGen | kVarOccl | kVarCoat | kVarStack | kVarFilt); break;
  }
#undef LF_LAUNCH_ASPH
#undef LF_LAUNCH_ASPH2
  lf_timing_end(ctx, LFK_MARCH, ev);
  LF_HIP(ctx, hipGetLastError());
  return LF_OK;
}
