// lf_march_common.h -- what the two march kernels share (lf_march.hip: k_march, the path-tree walk of every
// sample; lf_cull.hip: k_march_cull, the march of the paths a pre-pass found able to reach the light): the
// launch arguments, the scalar-cache row loads and the sun's lobe.  Device code; nothing here is part of the ABI.
#pragma once

#include <cstddef>

#include "lf_internal.h"
#include "lf_march_events.h"
#include "lf_scene_walk.h"

namespace lfm {

// The sun's lobe: q = (1 - cos theta) / (1 - cos alpha), theta between the ray and the sun.
// 1 - d.s would cancel (d.s ~ 0.999: an absolute error of 1e-7 is 1e-4 of a 0.05 rad lobe, and the
// float unit vectors are only unit to 1e-7 as well), so
//   1 - cos theta = sin^2 theta / (1 + cos theta) = |d x s|^2 / (|d|^2 |s|^2 + sqrt(|d|^2 |s|^2) d.s)
// which has no cancellation and does not assume |d| = |s| = 1 (ss = |s|^2 from the host).  Valid for
// d.s > 0, which the pre-test guarantees.  (tests/test_gpu_march_f64.py checks the march against an
// independent float64 tracer; with the plain 1 - d.s the pixels were off by up to 1e-2.)
__device__ __forceinline__ float lobe_q(float dx, float dy, float dz, float sx, float sy, float sz,
                                        float ss, float inv_1mc) {
  const float cg = fmaf(dx, sx, fmaf(dy, sy, dz * sz));
  const float cx = fmaf(dy, sz, -(dz * sy)), cy = fmaf(dz, sx, -(dx * sz)), cz = fmaf(dx, sy, -(dy * sx));
  const float c2 = fmaf(cx, cx, fmaf(cy, cy, cz * cz));
  const float dd = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
  const float ds = dd * ss;
  const float den = fmaf(lf_sqrt(ds), cg, ds);
  return __fdiv_rn(c2, den) * inv_1mc;
}

// The lanes the weighted re-march is FOR.  The pre-test d.s > lobe_thr only selects (a 1/16 margin around the lobe); what the
// re-march's epilogue keeps is lobe_q < 1 on the re-marched ray's direction -- which is the first march's, bit for bit (the
// same events on the same ray).  So once the pre-test admits a lane of a completed path, the epilogue's own test is made on
// the first march's rays: lit[j] keeps the lanes that will contribute, and a wavelength none of whose lanes will is not
// marched again.  Behind the pre-test (a root and a division per wavelength), never on every completed path.  Returns the
// union of the narrowed masks.
// q[j]: the lobe_q the gate computed for wavelength j -- the value the epilogue would compute again on the re-marched ray's
// direction, so an epilogue that takes it from here needs neither the root nor the division a second time; defined where
// lit[j] came in non-empty (elsewhere 2: outside every lobe), and lit[j] goes out empty everywhere else.
template <int K>
__device__ __forceinline__ lanemask lobe_gate(const Ray (&r)[K], lanemask (&lit)[K], float sx, float sy, float sz, float ss,
                                              float inv_1mc, float (&q)[K]) {
  lanemask lit_any = 0ull;
#pragma unroll
  for (int j = 0; j < K; j++) {
    q[j] = 2.0f;
    if (lit[j] != 0ull) {
      q[j] = lobe_q(r[j].dx, r[j].dy, r[j].dz, sx, sy, sz, ss, inv_1mc);
      lit[j] &= __ballot(q[j] < 1.0f);
    }
    lit_any |= lit[j];
  }
  return lit_any;
}
template <int K>
__device__ __forceinline__ lanemask lobe_gate(const Ray (&r)[K], lanemask (&lit)[K], float sx, float sy, float sz, float ss,
                                              float inv_1mc) {
  float q[K];
  return lobe_gate<K>(r, lit, sx, sy, sz, ss, inv_1mc, q);
}

// ---- ghost occlusion (lf_set_ghost_occlusion; the kernels instantiated with kVarOccl, k_ghost_ray_visibility) ------------
// A ray that has left the front element at (px, py, z) lens millimetres (z absolute in the prescription's coordinates)
// along (dx, dy, dz) goes to the world exactly as the lens camera's primary ray does (lf_scene.hip scene_pixel, the same
// expressions in the same order, in double): oc = (px wpm, py wpm, (z - z_ref) wpm), origin = pos + c2w oc, direction =
// c2w unit(d) -- in a lens-camera frame the ghost's shadow ray and the scene image agree.  The shadow ray runs from
// min_t = 0 to max_t = +inf: the camera's clip planes belong to the image, not to what stands between the lens and a light.
// (max_t: where the ray ends -- a point light's reach under LF_OCCLUSION_REACH_LIGHT, lf_point_shadow_reach; +inf everywhere else)
__device__ __forceinline__ lfw::DRay ghost_shadow_ray(const LfOcclDev& o, float px, float py, float z, float dx, float dy, float dz,
                                                      double max_t = (double)INFINITY) {
  using namespace lfw;
  const double wpm = o.wpm;
  const V3 oc = v3((double)px * wpm, (double)py * wpm, ((double)z - o.z_ref) * wpm);
  const V3 dc = unit(v3((double)dx, (double)dy, (double)dz));
  const V3 ow = v3(o.pos[0] + ((oc.x * o.c2w[0] + oc.y * o.c2w[1]) + oc.z * o.c2w[2]),
                   o.pos[1] + ((oc.x * o.c2w[3] + oc.y * o.c2w[4]) + oc.z * o.c2w[5]),
                   o.pos[2] + ((oc.x * o.c2w[6] + oc.y * o.c2w[7]) + oc.z * o.c2w[8]));
  return make_ray(ow,
                  v3((dc.x * o.c2w[0] + dc.y * o.c2w[1]) + dc.z * o.c2w[2],
                     (dc.x * o.c2w[3] + dc.y * o.c2w[4]) + dc.z * o.c2w[5],
                     (dc.x * o.c2w[6] + dc.y * o.c2w[7]) + dc.z * o.c2w[8]),
                  0.0, max_t);
}
// ... and whether it sees the sky: the scene kernels' any-hit walk (lf_scene_walk.h closest_hit, h == nullptr) over the
// resident tree, the stack of deferred children in the lane's own array
__device__ inline bool ghost_ray_visible(const LfOcclDev& o, float px, float py, float z, float dx, float dy, float dz,
                                         double max_t = (double)INFINITY) {
  lfw::DRay ray = ghost_shadow_ray(o, px, py, z, dx, dy, dz, max_t);
  LfSceneDev sc{};
  sc.nodes = o.nodes; sc.prims = o.prims;
  int stack[lfw::kStackDepth];
  lfw::SceneTally tally{0u, 0u};
  return !lfw::closest_hit<1>(sc, ray, nullptr, stack, tally);
}

// ---- several lights (lf_set_lights; the kernels instantiated with kVarLights) ------------------------------------------
// Light k's lobe is the sun's with LfLensDev::light_*[k] in place of sun_*: the same pre-test against light_thr[k], the same
// lobe_q.  n_lights and every per-light scalar are wave-uniform and come through the scalar cache (k is a loop counter).
// ONE definition of each step, for every march kernel and the cull table's audit.

// is the direction d inside light k's lobe, exactly as the single-light march decides it: the pre-test d.s_k > thr_k AND
// lobe_q_k < 1 (q: lobe_q_k, valid where the pre-test holds)
__device__ __forceinline__ bool light_admits(const LfLensDev* __restrict__ lens, int k, float dx, float dy, float dz, float& q) {
  const float sx = lens->light_dir[k][0], sy = lens->light_dir[k][1], sz = lens->light_dir[k][2];
  const float cg = fmaf(dx, sx, fmaf(dy, sy, dz * sz));
  q = lobe_q(dx, dy, dz, sx, sy, sz, lens->light_ss[k], lens->light_inv_one_minus_cos[k]);
  return cg > lens->light_thr[k] && q < 1.0f;
}
// ... of the ray that left the front element at (px, py, front vertex + hz) along d: under VAR & kVarNear a POINT light k
// (lens->light_kind[k], wave-uniform: a scalar branch) takes the direction to it from that point -- s = L_k - P per lane,
// inside iff d.s > 0 and q < 1 (lf_point_lobe_q, lf_march_events.h); a directional light, and every light of a kernel
// without kVarNear, is decided by the direction alone, as above.  Under VAR & kVarArea an AREA light k (the same scalar
// branch on the kind; its twelve geometry floats scalar operands) is decided by lf_area_inside at that point, with q = 0:
// (1 - q)^2 is exactly 1, the factor of a light without a lobe.
template <int VAR>
__device__ __forceinline__ bool light_admits_at(const LfLensDev* __restrict__ lens, int k, float px, float py, float hz, float dx, float dy,
                                                float dz, float& q) {
  if ((VAR & kVarArea) && lens->light_kind[k] == LF_LIGHT_AREA) {
    q = 0.0f;
    return lf_area_inside(dx, dy, dz, px, py, lens->surf[0].zv + hz, lens->light_pos[k], lens->light_area[k]);
  }
  if ((VAR & kVarNear) && lens->light_kind[k] != LF_LIGHT_DIRECTIONAL) {
    float cg;
    q = lf_point_lobe_q(dx, dy, dz, px, py, lens->surf[0].zv + hz, lens->light_pos[k][0], lens->light_pos[k][1], lens->light_pos[k][2],
                        lens->light_inv_one_minus_cos[k], cg);
    return cg > 0.0f && q < 1.0f;
  }
  return light_admits(lens, k, dx, dy, dz, q);
}
// The pre-test of a completed path's K rays: lit[j] = the lanes of alive[j] that ANY light's pre-test admits (d.s_k > thr_k)
// and then -- GATE, the geometry-first kernels: what lobe_gate is to one light -- that lie inside ANY light's lobe, so that
// a wavelength none of whose lanes will contribute to any light is not marched again.  Returns the union of the masks.
// (VAR & kVarNear: a point light's pre-test is lf_point_pretest on the ray's exit point, a superset of its lobe;
//  VAR & kVarArea: an area light's is lf_area_pretest, its bounding sphere seen from that point)
template <int K, bool GATE, int VAR = kVarLights>
__device__ __forceinline__ lanemask lights_pretest(const LfLensDev* __restrict__ lens, const Ray (&r)[K], const lanemask (&alive)[K],
                                                   lanemask (&lit)[K]) {
  const int n = lens->n_lights;
  lanemask lit_any = 0ull;
#pragma unroll
  for (int j = 0; j < K; j++) {
    bool near = false;
    for (int k = 0; k < n; k++) {
      if ((VAR & kVarArea) && lens->light_kind[k] == LF_LIGHT_AREA) {   // (its bounding sphere, light_thr[k] the radius squared)
        near = lf_area_pretest(r[j].dx, r[j].dy, r[j].dz, r[j].px, r[j].py, lens->surf[0].zv + r[j].hz, lens->light_pos[k],
                               lens->light_thr[k]) || near;
        continue;
      }
      if ((VAR & kVarNear) && lens->light_kind[k] != LF_LIGHT_DIRECTIONAL) {
        near = lf_point_pretest(r[j].dx, r[j].dy, r[j].dz, r[j].px, r[j].py, lens->surf[0].zv + r[j].hz, lens->light_pos[k][0],
                                lens->light_pos[k][1], lens->light_pos[k][2], lens->light_thr[k]) || near;
        continue;
      }
      const float cg = fmaf(r[j].dx, lens->light_dir[k][0], fmaf(r[j].dy, lens->light_dir[k][1], r[j].dz * lens->light_dir[k][2]));
      near = near || cg > lens->light_thr[k];
    }
    lit[j] = alive[j] & __ballot(near);
    lit_any |= lit[j];
  }
  if (!GATE || lit_any == 0ull) return lit_any;
  lit_any = 0ull;
#pragma unroll
  for (int j = 0; j < K; j++) {
    if (lit[j] != 0ull) {
      bool in = false;
      for (int k = 0; k < n; k++) { float q; in = light_admits_at<VAR>(lens, k, r[j].px, r[j].py, r[j].hz, r[j].dx, r[j].dy, r[j].dz, q) || in; }
      lit[j] &= __ballot(in);
    }
    lit_any |= lit[j];
  }
  return lit_any;
}
// What a lit ray's contribution to light k is multiplied by per channel c, for wavelength l: light_radiance[k][c] *
// lambda_rgb[l][c] (one float multiply, as the single light's) at s_chan[(k * LF_MAX_LAMBDA + l) * 3 + c]: formed once per
// workgroup, before the kernel's first barrier.
constexpr int kLightChan = LF_MAX_LIGHTS * LF_MAX_LAMBDA * 3;
__device__ __forceinline__ void lights_channel_factors(const LfLensDev* __restrict__ lens, float* __restrict__ s_chan, int tid, int n_threads) {
  for (int i = tid; i < kLightChan; i += n_threads) {
    const int k = i / (LF_MAX_LAMBDA * 3), lc = i - k * (LF_MAX_LAMBDA * 3), l = lc / 3, c = lc - 3 * l;
    s_chan[i] = (k < lens->n_lights && l < lens->n_lambda) ? lens->light_radiance[k][c] * lens->lambda_rgb[l][c] : 0.0f;
  }
}
// The lit epilogue, after the ONE weighted re-march of wavelength l (rw: the re-marched ray; mine: this lane is one the
// pre-test admitted): per light k the single light's arithmetic -- q_k, (1 - q_k)^2 times the weight, kept where the lane
// lies inside lobe k -- one fixed-point value per (ray, light, channel), converted separately and added to the pixel's
// three sums at acc; n_light counts (ray, light) contributions.
//
// VAR & kVarOccl (lf_set_ghost_occlusion): contrib_k, computed as ever, is added only if the scene does not block the ray --
// its own exit point on the front element along its own exit direction (ghost_ray_visible above).  The ray is the same for
// every light, so a lane walks ONCE, at the first light it would contribute to; the tallies count (ray, light) pairs: those
// with contrib_k > 0 are the shadow tests made, those dropped the blocked ones -- wave-wide ballots, one pair of global
// adds per epilogue that tested anything.  Only the lanes with something to add walk (a few per wave), each with its own
// stack of deferred children (a lane's own array, kStackDepth ints of scratch): no LDS beside the kernel's own, so the
// workgroups per CU stay what the kVarLights twin's LDS allows.
//
// VAR & kVarOccl & kVarNear (lf_set_ghost_occlusion_reach, LF_OCCLUSION_REACH_LIGHT with a point light installed): the shadow
// ray of light k ends at reach_k -- +inf for a directional light, lf_point_shadow_reach for a point light -- so one walk no
// longer answers for every light.  The same any-hit walk over [0, reach_k], and its answers reused by monotonicity: a
// primitive's test forms its root without looking at max_t and accepts it iff it lies in [0, max_t] (lf_scene_walk.h
// hit_sphere, hit_triangle), and the box test only ever drops what the double ray provably misses, so "something within
// [0, T]" is exactly "some primitive's root <= T": nothing within [0, T] settles every shorter segment, something within
// [0, T] every longer one.  A lane keeps the longest segment it found free and the shortest it found blocked, and walks
// only for a reach between the two: the directional lights (all +inf) still share one walk, two lamps on the same side of
// every occluder share one, and each answer is the per-light definition's, whatever the other lights are.
//
// VAR & kVarArea: an area light's q is 0 (light_admits_at), so its contrib is wn / wd itself; under kVarOccl its reach is
// lf_area_shadow_reach -- just before the rectangle -- and joins the same reuse of walks.
template <int VAR = kVarLights>
__device__ __forceinline__ void lights_epilogue(const LfLensDev* __restrict__ lens, const float* __restrict__ s_chan, const Ray& rw,
                                                bool mine, int l, unsigned long long* __restrict__ acc, unsigned& n_light) {
  const int n = lens->n_lights;
  const float wq = __fdiv_rn(rw.wn, rw.wd);
  // kVarOccl: the launch's occlusion record behind the lens (wave-uniform: scalar loads), this lane's walk once made
  const LfOcclDev& occl = *(const LfOcclDev*)((const char*)lens + kLensOcclOffset);
  int vis = -1;                      // (1 = the ray sees the sky)
  // ... | kVarNear: what this lane's walks have settled -- nothing stands within [0, seen_to], something within [0, dark_from]
  double seen_to = -1.0, dark_from = 0.0;
  bool dark_any = false;
  unsigned w_tested = 0u, w_blocked = 0u;   // ... the wave's tallies (wave-uniform)
  for (int k = 0; k < n; k++) {
    float qq;
    const bool in = light_admits_at<VAR>(lens, k, rw.px, rw.py, rw.hz, rw.dx, rw.dy, rw.dz, qq);
    const float om = 1.0f - qq;
    float contrib = wq * (om * om);
    contrib = (mine && in && contrib > 0.0f) ? contrib : 0.0f;
    if ((VAR & kVarOccl) && (VAR & kVarNear)) {
      const bool test = contrib > 0.0f;
      // (the light's kind through the scalar cache, as in light_admits_at: a scalar branch around the lanes' reach)
      const bool point = lens->light_kind[k] != LF_LIGHT_DIRECTIONAL;
      const bool area = (VAR & kVarArea) && lens->light_kind[k] == LF_LIGHT_AREA;
      if (test) {
        const float z = occl.front_zv + rw.hz;
        double reach = (double)INFINITY;
        if (area)        // (... just before the rectangle's plane)
          reach = lf_area_shadow_reach(rw.dx, rw.dy, rw.dz, rw.px, rw.py, z, lens->light_pos[k], lens->light_area[k], occl.wpm);
        else if (point)
          reach = lf_point_shadow_reach(rw.dx, rw.dy, rw.dz, rw.px, rw.py, z, lens->light_pos[k][0], lens->light_pos[k][1],
                                        lens->light_pos[k][2], occl.wpm);
        bool v;
        if (reach <= seen_to) v = true;
        else if (dark_any && reach >= dark_from) v = false;
        else {
          v = ghost_ray_visible(occl, rw.px, rw.py, z, rw.dx, rw.dy, rw.dz, reach);
          if (v) seen_to = reach; else { dark_from = reach; dark_any = true; }
        }
        if (!v) contrib = 0.0f;
      }
      w_tested += (unsigned)__popcll(__ballot(test));
      w_blocked += (unsigned)__popcll(__ballot(test && contrib == 0.0f));
    } else if (VAR & kVarOccl) {
      const bool test = contrib > 0.0f;
      if (test) {
        if (vis < 0)
          vis = ghost_ray_visible(occl, rw.px, rw.py, occl.front_zv + rw.hz, rw.dx, rw.dy, rw.dz) ? 1 : 0;
        if (vis == 0) contrib = 0.0f;
      }
      w_tested += (unsigned)__popcll(__ballot(test));
      w_blocked += (unsigned)__popcll(__ballot(test && contrib == 0.0f));
    }
    n_light += contrib > 0.0f ? 1u : 0u;
    const float* const ch = s_chan + (k * LF_MAX_LAMBDA + l) * 3;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float v = contrib * ch[c];
      const unsigned long long fx = (unsigned long long)(v * 68719476736.0f);
      if (fx) atomicAdd(&acc[c], fx);
    }
  }
  if ((VAR & kVarOccl) && w_tested != 0u) {   // wave-uniform; the first active lane adds for the wave
    const lanemask act = __ballot(true);
    if (__lane_id() == (unsigned)(__ffsll((long long)act) - 1)) {
      atomicAdd(&occl.stats[0], (unsigned long long)w_tested);
      if (w_blocked) atomicAdd(&occl.stats[1], (unsigned long long)w_blocked);
    }
  }
}

struct MarchArgs {
  int mw, mh, W, H, y0, y1;
  int spp, G;          // G x G pupil strata, G = floor(sqrt(spp))
  float inv_G;
  int sub_bits;        // each stratum is split into 2^sub_bits x 2^sub_bits sub-cells
  float inv_sub;
  int trow0, tperiod;  // tile rows handled: trow0 + j * tperiod, j = 0 ..   (the frame dealt by tile rows)
  LfDeal deal;         // ... or by 64 x 64-pixel blocks (deal.bx > 0, lf_set_block_deal): own block k = rank + k n, 64 wave tiles each
  int sgroups;         // the samples of a tile are split over this many workgroups (power of two)
  int tail_from, tail_groups;   // k_march_cull: the launch's LAST tiles (slots >= tail_from, a multiple of 64) split over tail_groups
                       // workgroups each, so that the launch ends on short workgroups (0 / 1: no tail); the rest as `sgroups` says
  uint2 key;
  float inv_stop_h;    // 1 / stop_h (correctly rounded)
  float half_w, half_h;  // 0.5 * W, 0.5 * H
  float vz;            // pupil_z - z_sensor
  float lobe_thr;      // d.s above this may lie inside the sun's lobe (conservative, see lfk_march)
  int accumulate;      // add the launch's pixels to the ghost buffer instead of replacing them
  int n_tiles;         // wave tiles of the launch (the grid holds them padded to a multiple of 64)
  int xs;              // log2 of the lanes' pixel stride in x (lf_set_tile_stride): 0 = an 8 x 8 block of
                       // adjacent pixels per wave, 3 = columns 8 apart (a 64 x 8 block shared by 8 waves)
};

// wave tile `tile_lin` of the launch -> its position along x (tx: see k_march) and its tile row.  Dealt by rows: the launch's
// tile rows one after the other; by blocks: the 8 x 8 wave tiles of own block tile_lin / 64 (8 tile rows x 8 tiles across its
// 64 columns, whatever the tile stride).  All wave-uniform.
__device__ __forceinline__ void march_tile_of(const MarchArgs& a, int tile_lin, int tiles_x, int& tx, int& trow) {
  if (a.deal.bx > 0) {
    const int b = a.deal.rank + (tile_lin >> 6) * a.deal.n, w = tile_lin & 63;
    const int by = b / a.deal.bx;
    trow = by * 8 + (w >> 3);
    tx = (b - by * a.deal.bx) * 8 + (w & 7);
  } else {
    const int tj = tile_lin / tiles_x;
    tx = tile_lin - tj * tiles_x;
    trow = a.trow0 + tj * a.tperiod;
  }
}
// does this launch render pixel row y / pixel (x, y)?  (k_march_finish, k_scale_rows)
__device__ __forceinline__ bool march_owns(const MarchArgs& a, int x, int y) {
  if (a.deal.bx > 0) return lf_deal_mine(a.deal, x, y);
  const int t = y >> 3;
  return t >= a.trow0 && (t - a.trow0) % a.tperiod == 0;
}

// The program of a GROUP of up to 3 wavelengths, in two levels (LfProgHdr / LfProgRow in
// lf_internal.h): per row a 16-byte header (ONE s_load_dwordx4), per distinct (interface, direction)
// a 64-byte record (ONE s_load_dwordx16: the geometry once, the index ratios of each wavelength of
// the group).  A header names its own record and the NEXT row's, so stepping to the next row issues
// both loads at once; only a jump (a wave that died as a whole) loads header, then record.
typedef int lf_i16 __attribute__((ext_vector_type(16)));
typedef int lf_i4 __attribute__((ext_vector_type(4)));
typedef const lf_i16 __attribute__((address_space(4))) * lf_const_prow_ptr;
typedef const lf_i4 __attribute__((address_space(4))) * lf_const_phdr_ptr;
__device__ __forceinline__ LfProgRow load_prec(const LfProgRow* __restrict__ base, unsigned off) {
  // (base + 32-bit byte offset: the load takes it as its SGPR offset)
  typedef const char __attribute__((address_space(4))) * cptr;
  const lf_i16 v = *(lf_const_prow_ptr)((cptr)(base) + off);
  LfProgRow r;
  r.dzv = __int_as_float(v[0]); r.curv = __int_as_float(v[1]); r.h2 = __int_as_float(v[2]);
  r.sc = __int_as_float(v[3]); r.sgn = __int_as_float(v[4]);
#pragma unroll
  for (int j = 0; j < 3; j++) {
    r.delta[j] = __int_as_float(v[5 + j]); r.cn22[j] = __int_as_float(v[8 + j]); r.rn2[j] = __int_as_float(v[12 + j]);
  }
  r.ch = __int_as_float(v[11]); r.c2 = __int_as_float(v[15]);
  return r;
}
__device__ __forceinline__ LfWeightRow load_wrec(const LfWeightRow* __restrict__ base, unsigned off) {
  typedef const char __attribute__((address_space(4))) * cptr;
  const lf_i16 v = *(lf_const_prow_ptr)((cptr)(base) + off);
  LfWeightRow r;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    r.fs[j] = __int_as_float(v[j]); r.fo[j] = __int_as_float(v[4 + j]); r.fi[j] = __int_as_float(v[8 + j]);
  }
  r.pad0 = r.pad1 = r.pad2 = 0.0f;
  r.coat = v[12];
  r.pad3[0] = r.pad3[1] = r.pad3[2] = 0.0f;
  return r;
}
__device__ __forceinline__ LfProgHdr load_phdr(const LfProgHdr* __restrict__ base, unsigned off) {
  typedef const char __attribute__((address_space(4))) * cptr;
  const lf_i4 v = *(lf_const_phdr_ptr)((cptr)(base) + off);
  LfProgHdr h;
  h.flags = v[0]; h.skip = v[1]; h.rec = v[2]; h.rec_next = v[3];
  return h;
}

// ONE dword of a weight record through the scalar cache: what a single wavelength's re-march reads of it -- fs[j], fo[j],
// fi[j] (base = the group's weight records + 4 j bytes) and the record's film offset -- where load_wrec's sixteen
// dwords would land on the registers the callers hold across the row loop
__device__ __forceinline__ int load_wrec_dword(const void* __restrict__ base, unsigned off) {
  typedef const char __attribute__((address_space(4))) * cptr;
  return *(const int __attribute__((address_space(4)))*)((cptr)(base) + off);
}

// The weighted march of ONE path for wavelength j of group g (recs / wrecs: the group's records; wrec_table: group
// 0's, where the film offsets count from) along its own sequence (n_ev dwords at w): the same arithmetic on the ray as
// the geometry-only march, plus the Fresnel / aperture weight -- and, by the kernel's variant VAR (kVarCoat: launched
// for a lens with a film; kVarFilt: for a context under LF_MASK_BILINEAR), a coated row's film and the bilinear mask.
// The culled kernels' re-march of a lit path (k_march's path tree keeps the same loop
// inline: folded into this function, its K = 2 instantiation spilled 13 SGPRs more).
template <int VAR>
__device__ __forceinline__ void weighted_remarch(Ray& rw, const int* __restrict__ w, int n_ev, int j, const LfProgRow* __restrict__ recs,
                                                 const LfWeightRow* __restrict__ wrecs,
                                                 const LfWeightRow* __restrict__ wrec_table, const float* __restrict__ mask,
                                                 float inv_stop_h, int mw, int mh) {
  const char* const wj = (const char*)wrecs + 4 * j;
  // (the sequence dword one row ahead, unconditionally: the table ends on a spare dword -- pack_program)
  unsigned se = (unsigned)*(const int __attribute__((address_space(4)))*)(w);
  for (int left = n_ev; left > 0; --left) {
    const unsigned cur = se;
    se = (unsigned)*(const int __attribute__((address_space(4)))*)(++w);
    // the record and the row's weight scalars together, at the top of the row
    const unsigned off = cur & 0xffffu;
    const LfProgRow wr = load_prec(recs, off);
    const float w_fs = __int_as_float(load_wrec_dword(wj, off + (unsigned)offsetof(LfWeightRow, fs)));
    const float w_fo = __int_as_float(load_wrec_dword(wj, off + (unsigned)offsetof(LfWeightRow, fo)));
    const float w_fi = __int_as_float(load_wrec_dword(wj, off + (unsigned)offsetof(LfWeightRow, fi)));
    int w_coat = 0;
    if (VAR & kVarCoat) w_coat = load_wrec_dword(wrecs, off + (unsigned)offsetof(LfWeightRow, coat));   // (only a film kernel reads it)
    const unsigned wfl = cur >> 16;
    const float w_cn22 = j == 0 ? wr.cn22[0] : j == 1 ? wr.cn22[1] : wr.cn22[2];
    const float w_rn2 = j == 0 ? wr.rn2[0] : j == 1 ? wr.rn2[1] : wr.rn2[2];
    const float w_delta = j == 0 ? wr.delta[0] : j == 1 ? wr.delta[1] : wr.delta[2];
    if (wfl & LF_EV_STOP) {
      (void)stop_event_var<true, VAR>(rw, wr.dzv, wr.h2, inv_stop_h, mask, mw, mh);
    } else {
      lanemask geom_ok;
      (void)surface_event<true>(rw, wr.dzv, wr.curv, wr.ch, wr.c2, wr.sc, w_cn22, w_rn2, w_delta, wr.h2,
                                (wfl & LF_EV_REFLECT) != 0, (wfl & LF_EV_FLAT) != 0, wr.sgn, geom_ok, w_fs, w_fo, w_fi,
                                CoatSel<VAR>{wrec_table, w_coat, j});
    }
  }
}

}  // namespace lfm

// host, lf_march.hip: what every launch of a march over this context's share of the frame has in common -- the refusals of
// the installed lights, the launch arguments (false: the context owns no tile) and the upload of the lens on the launch's
// fixed-point grid with the occlusion record behind it.  The ordinary launch and the sensor paths' (lf_march_sensor.hip)
// both go through them.
lf_status lf_march_lights_ready(const lf_ctx* ctx);
bool lf_march_launch_args(const lf_ctx* ctx, int spp, uint64_t key, bool culled, lfm::MarchArgs* out, size_t* out_tiles);
lf_status lf_march_upload_lens(lf_ctx* ctx, const LfLensDev& L, int bits);
