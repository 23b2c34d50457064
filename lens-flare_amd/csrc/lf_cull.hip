// lf_cull.hip -- spend the rays where the light is (rounds 5 and 6): the march of the paths the cull table starts.
// Which (sensor block, pupil cell, path) combinations can reach the light is the cull TABLE's knowledge, and the table is
// lf_cull_prepass.hip's (built, cached, resolved, counted, audited).  Here is what it is FOR, the default launch (lfk_march_culled):
//   k_march_cull<K>  the march of exactly the started paths: per wave tile and sample one scalar load tells which; the
//                    paths of a sample share their common leg from the sensor (march_started_set, round 6: the bench
//                    frame's 5.9e10 events of started paths take 3.3e10 executed ones), geometry first and the Fresnel /
//                    aperture weight by a second march of the lanes that reach the lobe, the event arithmetic being
//                    lf_march_events.h's -- so a started ray is bit for bit the ray k_march and the oracle march, and
//                    since an unstarted one contributes 0 the PIXELS are those of the full enumeration.  Counters count
//                    what was started, every path as if marched alone (the oracle follows the same table:
//                    oracle/lf_geo_oracle.c geo_set_cull).  The row loop is built around the CU's ONE scalar unit, which
//                    it waits for (the row's kind decided once for its K wavelengths, the sequence dword prefetched
//                    unconditionally, one test at the row's end: 36.5 -> 33.1 ms), and a launch ends on short workgroups
//                    (its last tiles split over 4 workgroups whose integer sums meet in a small buffer: MarchArgs::tail_from).
//   k_march_items<K> the same for sampling specifications without pupil sub-cells: (pixel, sample) items compacted
//                    per path by ballot + an LDS prefix sum.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "lf_internal.h"
#include "lf_march_events.h"
#include "lf_march_common.h"

namespace {

using namespace lfm;

constexpr int kWgWaves = 8;
constexpr int kListBits = 12;
constexpr int kListMax = 1 << kListBits;   // samples of one tile's workgroup (spp / sgroups) listed at a time

// what a wave tallies while it marches (slots of lf_counters / lf_get_march_stats)
struct PathTally {
  unsigned long long n_rays = 0, events = 0, n_clip = 0, n_vign = 0, n_tir = 0, n_scene = 0, n_rm_lane = 0, n_rm_rows = 0;
  unsigned long long executed = 0;   // rows really executed (a row of the common leg once): march_started_set; march_started_path: = events
  unsigned n_light = 0;   // per lane
};

// What a lit ray's contribution is multiplied by per channel c, for wavelength l: sun_radiance[c] * lambda_rgb[l][c], wave-uniform
// and constant for a launch -- formed ONCE per workgroup (the same single float multiply) into LDS at [3 l + c], where the
// re-march's epilogue reads it instead of through six waited scalar loads per lit (path, wavelength).  Before the kernel's
// first barrier.
// (a kernel of several lights, VAR & kVarLights: per light, lights_channel_factors)
template <int VAR>
__device__ __forceinline__ void march_channel_factors(const LfLensDev* __restrict__ lens, float* __restrict__ s_chan, int tid) {
  if (VAR & kVarLights) { lights_channel_factors(lens, s_chan, tid, 64 * kWgWaves); return; }
  if (tid < LF_MAX_LAMBDA * 3) {
    const int l = tid / 3, c = tid - 3 * l;
    s_chan[tid] = l < lens->n_lambda ? lens->sun_radiance[c] * lens->lambda_rgb[l][c] : 0.0f;
  }
}

// One STARTED path q of one sensor sample per lane (start ray X, Y, s0; lanes in start_mask), every wavelength group:
// the events of the path's own sequence, K wavelengths together, tallies, the lobe test, the weighted second march
// (W1 = false) and the fixed-point add into the tile's LDS sums at pixel slot acc_slot.  Shared by the two culled
// kernels below: lane = pixel (k_march_cull) and lane = one compacted (pixel, sample) item (k_march_items).
template <int K, bool W1, int VAR>
__device__ __forceinline__ void march_started_path(const LfLensDev* __restrict__ lens, const LfPairsDev* __restrict__ pairs,
                                                   const int* __restrict__ seq_table, const LfProgRow* __restrict__ rec_table,
                                                   const LfWeightRow* __restrict__ wrec_table, const float* __restrict__ mask,
                                                   const MarchArgs& a, int q, lanemask start_mask, float X, float Y,
                                                   const StartRay& s0, int lane, int acc_slot,
                                                   unsigned long long* __restrict__ s_acc, const float* __restrict__ s_chan,
                                                   PathTally& T) {
  const int n_lambda = lens->n_lambda, prog_recs = pairs->prog_recs;
  const int n_groups = (n_lambda + K - 1) / K;
  const float inv_stop_h = a.inv_stop_h, lobe_thr = a.lobe_thr;
  const float sx = lens->sun_dir[0], sy = lens->sun_dir[1], sz = lens->sun_dir[2];
  const float inv_1mc = lens->sun_inv_one_minus_cos, sun_ss = lens->sun_ss;
  const int n_ev = pairs->ev_cnt[q];
  const int* const seq = seq_table + pairs->ev_off[q];
  for (int g = 0; g < n_groups; g++) {
    const LfProgRow* const recs = rec_table + (size_t)g * (size_t)prog_recs;
    const LfWeightRow* const wrecs = wrec_table + (size_t)g * (size_t)prog_recs;
    Ray r[K];
    lanemask alive[K];
    unsigned nlive = 0u;
#pragma unroll
    for (int j = 0; j < K; j++) {
      r[j] = Ray{X, Y, 0.0f, fmaf(X, X, Y * Y), s0.dx, s0.dy, s0.dz, s0.w0, 1.0f};
      const float ns = lens->n_start[min(g * K + j, n_lambda - 1)];
      r[j].dx *= ns; r[j].dy *= ns; r[j].dz *= ns;
      alive[j] = (g * K + j < n_lambda) ? start_mask : 0ull;
      nlive += (unsigned)__popcll(alive[j]);
    }
    T.n_rays += nlive;
    unsigned ev32 = 0u;
    unsigned se = (unsigned)*(const int __attribute__((address_space(4)))*)(seq);
    int e = 0;
    if (n_ev > 0 && nlive != 0u) for (;;) {     // (the row's end tests ONE thing: a wave without rays leaves through the row counter)
      const unsigned cur = se;
      se = (unsigned)*(const int __attribute__((address_space(4)))*)(seq + e + 1);     // (the table ends on a spare dword: pack_program)
      const LfProgRow wr = load_prec(recs, cur & 0xffffu);
      LfWeightRow ww;
      if (W1) ww = load_wrec(wrecs, cur & 0xffffu);
      else { for (int j = 0; j < 3; j++) { ww.fs[j] = 1.0f; ww.fo[j] = 1.0f; ww.fi[j] = 1.0f; } ww.coat = 0; }
      const unsigned kind = cur >> 16;
      lanemask okv[K], gv[K], died = 0ull;
      if (kind & LF_EV_STOP) {
#pragma unroll
        for (int j = 0; j < K; j++) {
          if (K > 1 && __builtin_expect(alive[j] == 0ull, 0)) { okv[j] = 0ull; gv[j] = 0ull; continue; }
          okv[j] = stop_event_var<W1, VAR>(r[j], wr.dzv, wr.h2, inv_stop_h, mask, a.mw, a.mh);
          gv[j] = okv[j];
          died |= alive[j] & ~okv[j];
        }
        if (__builtin_expect(died != 0ull, 0)) {
#pragma unroll
          for (int j = 0; j < K; j++) {
            const unsigned nd = (unsigned)__popcll(alive[j] & ~okv[j]);
            T.n_clip += nd; nlive -= nd; alive[j] &= okv[j];
          }
          if (nlive == 0u) e = n_ev;
        }
      } else {
        if (kind == 0u) {          // refraction at a curved interface: the common row, straight-line
#pragma unroll
          for (int j = 0; j < K; j++) {
            if (K > 1 && __builtin_expect(alive[j] == 0ull, 0)) { okv[j] = 0ull; gv[j] = 0ull; continue; }
            okv[j] = surface_event<W1>(r[j], wr.dzv, wr.curv, wr.ch, wr.c2, wr.sc, wr.cn22[j], wr.rn2[j],
                                       wr.delta[j], wr.h2, false, false, wr.sgn, gv[j], ww.fs[j], ww.fo[j], ww.fi[j],
                                       CoatSel<VAR>{wrec_table, ww.coat, j});
            died |= alive[j] & ~okv[j];
          }
        } else if (kind == (unsigned)LF_EV_REFLECT) {      // a curved mirror: two rows of every pair
#pragma unroll
          for (int j = 0; j < K; j++) {
            if (K > 1 && __builtin_expect(alive[j] == 0ull, 0)) { okv[j] = 0ull; gv[j] = 0ull; continue; }
            okv[j] = surface_event<W1>(r[j], wr.dzv, wr.curv, wr.ch, wr.c2, wr.sc, wr.cn22[j], wr.rn2[j],
                                       wr.delta[j], wr.h2, true, false, wr.sgn, gv[j], ww.fs[j], ww.fo[j], ww.fi[j],
                                       CoatSel<VAR>{wrec_table, ww.coat, j});
            died |= alive[j] & ~okv[j];
          }
        } else {
#pragma unroll
          for (int j = 0; j < K; j++) {
            if (K > 1 && __builtin_expect(alive[j] == 0ull, 0)) { okv[j] = 0ull; gv[j] = 0ull; continue; }
            okv[j] = surface_event<W1>(r[j], wr.dzv, wr.curv, wr.ch, wr.c2, wr.sc, wr.cn22[j], wr.rn2[j],
                                       wr.delta[j], wr.h2, (kind & LF_EV_REFLECT) != 0, (kind & LF_EV_FLAT) != 0,
                                       wr.sgn, gv[j], ww.fs[j], ww.fo[j], ww.fi[j],
                                       CoatSel<VAR>{wrec_table, ww.coat, j});
            died |= alive[j] & ~okv[j];
          }
        }
        if (__builtin_expect(died != 0ull, 0)) {
#pragma unroll
          for (int j = 0; j < K; j++) {
            T.n_vign += (unsigned)__popcll(alive[j] & ~gv[j]);
            T.n_tir += (unsigned)__popcll(alive[j] & gv[j] & ~okv[j]);
            nlive -= (unsigned)__popcll(alive[j] & ~okv[j]);
            alive[j] &= okv[j];
          }
          if (nlive == 0u) e = n_ev;
        }
      }
      ev32 += nlive;       // events completed: one per ray still alive after the row
      if (++e >= n_ev) break;
    }
    T.events += ev32;
    T.executed += ev32;
    if (nlive == 0u) continue;
    // ---- the path is complete for nlive rays --------------------------------------------------
    T.n_scene += nlive;
    lanemask lit[K], lit_any = 0ull;
    if (VAR & kVarLights) {
      lit_any = lights_pretest<K, !W1, VAR>(lens, r, alive, lit);
      if (lit_any == 0ull) continue;
    } else {
#pragma unroll
    for (int j = 0; j < K; j++) {
      const float cg = fmaf(r[j].dx, sx, fmaf(r[j].dy, sy, r[j].dz * sz));
      lit[j] = alive[j] & __ballot(cg > lobe_thr);
      lit_any |= lit[j];
    }
    if (lit_any == 0ull) continue;
    if (!W1) {
      lit_any = lobe_gate<K>(r, lit, sx, sy, sz, sun_ss, inv_1mc);
      if (lit_any == 0ull) continue;
    }
    }
    for (int j = 0; j < K; j++) {        // not unrolled (W1 = false): one copy of the weighted march
      lanemask lj = lit[0];
#pragma unroll
      for (int jj = 1; jj < K; jj++) lj = (j == jj) ? lit[jj] : lj;
      if (lj == 0ull) continue;
      const int l = g * K + j;
      Ray rw = j == 0 ? r[0] : j == 1 ? r[K > 1 ? 1 : 0] : r[K > 2 ? 2 : 0];
      if (!W1) {
        // the path again, alone and with its weight: the same arithmetic on the ray, so the same ray bit for bit
        rw = Ray{X, Y, 0.0f, fmaf(X, X, Y * Y), s0.dx, s0.dy, s0.dz, s0.w0, 1.0f};
        { const float ns = lens->n_start[l]; rw.dx *= ns; rw.dy *= ns; rw.dz *= ns; }
        T.n_rm_lane += (unsigned long long)((unsigned)n_ev * (unsigned)__popcll(lj));
        T.n_rm_rows += (unsigned)n_ev;
        weighted_remarch<VAR>(rw, seq, n_ev, j, recs, wrecs, wrec_table, mask, inv_stop_h, a.mw, a.mh);
      }
      if (VAR & kVarLights) {
        lights_epilogue<VAR>(lens, s_chan, rw, ((lj >> lane) & 1ull) != 0ull, l, &s_acc[acc_slot * 3], T.n_light);
        continue;
      }
      const float qq = lobe_q(rw.dx, rw.dy, rw.dz, sx, sy, sz, sun_ss, inv_1mc);
      const float om = 1.0f - qq;
      float contrib = __fdiv_rn(rw.wn, rw.wd) * (om * om);
      contrib = (((lj >> lane) & 1ull) != 0ull && qq < 1.0f && contrib > 0.0f) ? contrib : 0.0f;
      T.n_light += contrib > 0.0f ? 1u : 0u;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float v = contrib * s_chan[l * 3 + c];
        const unsigned long long fx = (unsigned long long)(v * 68719476736.0f);
        if (fx) atomicAdd(&s_acc[acc_slot * 3 + c], fx);
      }
    }
  }
}

// ---- the started paths of ONE sample, their common leg marched once (round 6) ----------------------------------------
// Every path starts with the same leg from the sensor towards the scene -- the primary path's events -- and leaves it at
// its first mirror i after N - 1 - i of them (the primary path never does).  march_started_path marches that leg again for
// every started path; the paths a sample starts, though, are few and MOST of what they execute is this leg (a pair (i, j)
// of the 11-interface lens: 10 - i of its 11 + 2 (j - i) events, and the rays that end early end in it).  Here the wave
// keeps ONE running state of the common leg: the started paths are taken in the order of their first mirrors, rear ones
// first (= descending path index: the selection lists pairs by (i, j) ascending with the primary path in front; the host
// checks it, LfCullArgs::prefix_ok), the leg is extended to where the next path leaves it, the path's own events run on a
// copy.  The arithmetic on a ray is the same events in the same order: pixels and counters are those of every path
// marched alone -- a row of the common leg counts once for every started path that shares it (the paths not yet done) --
// while the rows EXECUTED fall by the shared part (the device's executed-events counter, slot 7).
// Geometry first (W1 = false): a lane that ends inside the lobe marches its path again, alone, with the weight, as before.
// one surface row for the K wavelengths of a group, its kind a compile-time constant -> the lanes that ended on it
template <int K, bool REFLECT, bool FLAT>
__device__ __forceinline__ lanemask surface_rows(Ray (&r)[K], const lanemask (&alive)[K], const LfProgRow& wr, lanemask (&okv)[K],
                                                 lanemask (&gv)[K]) {
  lanemask died = 0ull;
#pragma unroll
  for (int j = 0; j < K; j++) {
    if (K > 1 && __builtin_expect(alive[j] == 0ull, 0)) { okv[j] = 0ull; gv[j] = 0ull; continue; }
    okv[j] = surface_event<false>(r[j], wr.dzv, wr.curv, wr.ch, wr.c2, wr.sc, wr.cn22[j], wr.rn2[j], wr.delta[j], wr.h2,
                                  REFLECT, FLAT, wr.sgn, gv[j]);
    died |= alive[j] & ~okv[j];
  }
  return died;
}

// One row (sequence dword `cur`) of the geometry-first march on a state of K rays (s, alive, nlive): the common leg's, whose
// rows count for the `mult` started paths that still share it, or a path's own copy of it (mult = 1).  A ray the row ends
// counts `mult` times in its fate; a state that lost its last ray leaves its loop through the row counter (e = end).
// (the scalar unit is what the row loops wait for: the row's kind is decided ONCE for its K wavelengths -- curved glass
// crossed, by far the most frequent, first -- and the event inlined with its flags constant, so that the row's end tests
// one thing)
template <int K, int VAR>
__device__ __forceinline__ void started_row(Ray (&s)[K], lanemask (&alive)[K], unsigned& nlive, unsigned cur, unsigned mult,
                                            const LfProgRow* __restrict__ recs, const float* __restrict__ mask, const MarchArgs& a,
                                            float inv_stop_h, PathTally& T, int& e, int end) {
  const LfProgRow wr = load_prec(recs, cur & 0xffffu);
  const unsigned kind = cur >> 16;
  lanemask okv[K], gv[K], died = 0ull;
  if (__builtin_expect(kind == 0u, 1)) {
    died = surface_rows<K, false, false>(s, alive, wr, okv, gv);
  } else if (kind & LF_EV_STOP) {
#pragma unroll
    for (int j = 0; j < K; j++) {
      if (K > 1 && __builtin_expect(alive[j] == 0ull, 0)) { okv[j] = 0ull; gv[j] = 0ull; continue; }
      okv[j] = stop_event_var<false, VAR>(s[j], wr.dzv, wr.h2, inv_stop_h, mask, a.mw, a.mh);
      gv[j] = okv[j];
      died |= alive[j] & ~okv[j];
    }
  } else if (kind & LF_EV_REFLECT) {
    if (kind & LF_EV_FLAT) died = surface_rows<K, true, true>(s, alive, wr, okv, gv);
    else died = surface_rows<K, true, false>(s, alive, wr, okv, gv);
  } else {
    died = surface_rows<K, false, true>(s, alive, wr, okv, gv);
  }
  if (__builtin_expect(died != 0ull, 0)) {
    // (a stop row: gv = okv, every ray it ends is clipped; a surface row: missed / outside the aperture, or totally reflected)
    const bool stop_row = (kind & LF_EV_STOP) != 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
      const unsigned nd = (unsigned)__popcll(alive[j] & ~okv[j]);
      const unsigned nv = (unsigned)__popcll(alive[j] & ~gv[j]);
      T.n_clip += stop_row ? (unsigned long long)nd * mult : 0ull;
      T.n_vign += stop_row ? 0ull : (unsigned long long)nv * mult;
      T.n_tir += stop_row ? 0ull : (unsigned long long)(nd - nv) * mult;
      nlive -= nd;
      alive[j] &= okv[j];
    }
    if (nlive == 0u) e = end;
  }
}

template <int K, int VAR>
__device__ __forceinline__ void march_started_set(const LfLensDev* __restrict__ lens, const LfPairsDev* __restrict__ pairs,
                                                  const int* __restrict__ seq_table, const LfProgRow* __restrict__ rec_table,
                                                  const LfWeightRow* __restrict__ wrec_table, const float* __restrict__ mask,
                                                  const MarchArgs& a, unsigned long long todo, lanemask active_mask, float X, float Y,
                                                  const StartRay& s0, int lane, unsigned long long* __restrict__ s_acc,
                                                  const int2* __restrict__ s_meta, const float* __restrict__ s_chan,
                                                  PathTally& T) {
  const int n_lambda = lens->n_lambda, prog_recs = pairs->prog_recs;
  const int n_groups = (n_lambda + K - 1) / K;
  const float inv_stop_h = a.inv_stop_h, lobe_thr = a.lobe_thr;
  const float sx = lens->sun_dir[0], sy = lens->sun_dir[1], sz = lens->sun_dir[2];
  const float inv_1mc = lens->sun_inv_one_minus_cos, sun_ss = lens->sun_ss;
  const unsigned n_started = (unsigned)__popcll(todo);
  // the sample's re-march tallies, added to the 64-bit ones once: at most kCullMaxPaths paths x LF_MAX_LAMBDA wavelengths of
  // at most 0xffff events (the s_meta packing), 64 lanes each
  static_assert((unsigned long long)kCullMaxPaths * LF_MAX_LAMBDA * 0xffffull * 64ull < (1ull << 32), "a sample's re-march rows overflow 32 bits");
  unsigned rm_lane = 0u, rm_rows = 0u;
  for (int g = 0; g < n_groups; g++) {
    const LfProgRow* const recs = rec_table + (size_t)g * (size_t)prog_recs;
    const LfWeightRow* const wrecs = wrec_table + (size_t)g * (size_t)prog_recs;
    // TWO states: r, the common leg, which only ever runs the leg's rows and stays where it is; c, the copy of it a started
    // path takes at its fork (or at the leg's end: the primary path) and runs its own rows on -- nothing is taken back
    Ray r[K], c[K];
    lanemask alive[K], calive[K];
    unsigned nlive = 0u;
#pragma unroll
    for (int j = 0; j < K; j++) {
      r[j] = Ray{X, Y, 0.0f, fmaf(X, X, Y * Y), s0.dx, s0.dy, s0.dz, s0.w0, 1.0f};
      const float ns = lens->n_start[min(g * K + j, n_lambda - 1)];
      r[j].dx *= ns; r[j].dy *= ns; r[j].dz *= ns;
      alive[j] = (g * K + j < n_lambda) ? active_mask : 0ull;
      nlive += (unsigned)__popcll(alive[j]);
    }
    T.n_rays += (unsigned long long)nlive * n_started;
    int depth = 0;            // events of the common leg done
    unsigned long long left = todo;
    while (left != 0ull && nlive != 0u) {
      const int q = 63 - __builtin_clzll(left);
      left &= ~(1ull << q);
      // (the path's events and where it leaves the common leg: from the workgroup's LDS copy, not three dependent scalar loads)
      const int2 meta = s_meta[q];
      const int mx = __builtin_amdgcn_readfirstlane(meta.x);       // (q is wave-uniform: so are the path's lengths and rows)
      const int n_ev = mx >> 16, L = mx & 0xffff;
      const int* const seq = seq_table + __builtin_amdgcn_readfirstlane(meta.y);
      const unsigned mult = (unsigned)__popcll(left) + 1u;         // this path and those still to come share the leg so far
      // (the sequence dword one row ahead, unconditionally: the leg's loop stops at L < n_ev or on the table's spare dword, the
      // path's own on the spare dword -- pack_program)
      unsigned se = (unsigned)*(const int __attribute__((address_space(4)))*)(seq + depth);
      // ---- the common leg, extended to where path q leaves it: rows depth .. L on r ----------------------
      unsigned seg = 0u;                 // sum of the rays alive after each row of the segment
      int e = depth;
      if (e < L) for (;;) {
        const unsigned cur = se;
        se = (unsigned)*(const int __attribute__((address_space(4)))*)(seq + e + 1);
        started_row<K, VAR>(r, alive, nlive, cur, mult, recs, mask, a, inv_stop_h, T, e, L);
        seg += nlive;       // events completed: one per ray still alive after the row
        if (++e >= L) break;
      }
      // ... counted once for every logical path that shares the row (`mult` paths), and once as executed
      T.events += (unsigned long long)seg * mult;
      T.executed += seg;
      depth = L;
      if (nlive == 0u) break;       // the common leg ended for every lane before path q left it: so did every path still to come
      // ---- the fork: the path's own rows L .. n_ev on a copy ---------------------------------------------
      unsigned cn = nlive;
#pragma unroll
      for (int j = 0; j < K; j++) { c[j] = r[j]; calive[j] = alive[j]; }
      if (L < n_ev) {
        unsigned own = 0u;
        for (;;) {
          const unsigned cur = se;
          se = (unsigned)*(const int __attribute__((address_space(4)))*)(seq + e + 1);
          started_row<K, VAR>(c, calive, cn, cur, 1u, recs, mask, a, inv_stop_h, T, e, n_ev);
          own += cn;
          if (++e >= n_ev) break;
        }
        T.events += own;
        T.executed += own;
      }
      if (cn != 0u) {
        // ---- the path is complete for cn rays (as march_started_path) ------------------------------------
        T.n_scene += cn;
        lanemask lit[K], lit_any = 0ull;
        float gq[K];       // the gate's lobe_q per wavelength: what the lit epilogue needs of the copy, which is dead from here on
        if (VAR & kVarLights) {
          lit_any = lights_pretest<K, true, VAR>(lens, c, calive, lit);
        } else {
#pragma unroll
        for (int j = 0; j < K; j++) {
          const float cg = fmaf(c[j].dx, sx, fmaf(c[j].dy, sy, c[j].dz * sz));
          lit[j] = calive[j] & __ballot(cg > lobe_thr);
          lit_any |= lit[j];
        }
        if (lit_any != 0ull) lit_any = lobe_gate<K>(c, lit, sx, sy, sz, sun_ss, inv_1mc, gq);
        }
        if (lit_any != 0ull) {
          for (int j = 0; j < K; j++) {        // not unrolled: one copy of the weighted march
            lanemask lj = lit[0];
#pragma unroll
            for (int jj = 1; jj < K; jj++) lj = (j == jj) ? lit[jj] : lj;
            if (lj == 0ull) continue;
            const int l = g * K + j;
            // the path again, alone and with its weight: the same arithmetic on the ray, so the same ray bit for bit
            Ray rw = Ray{X, Y, 0.0f, fmaf(X, X, Y * Y), s0.dx, s0.dy, s0.dz, s0.w0, 1.0f};
            { const float ns = lens->n_start[l]; rw.dx *= ns; rw.dy *= ns; rw.dz *= ns; }
            rm_lane += (unsigned)n_ev * (unsigned)__popcll(lj);
            rm_rows += (unsigned)n_ev;
            weighted_remarch<VAR>(rw, seq, n_ev, j, recs, wrecs, wrec_table, mask, inv_stop_h, a.mw, a.mh);
            if (VAR & kVarLights) {
              lights_epilogue<VAR>(lens, s_chan, rw, ((lj >> lane) & 1ull) != 0ull, l, &s_acc[lane * 3], T.n_light);
              continue;
            }
            // the three channel factors off ONE address, on their way while the weight is divided
            const float* const ch = s_chan + l * 3;
            const float ch0 = ch[0], ch1 = ch[1], ch2 = ch[2];
            // lobe_q of the re-marched ray's direction IS the gate's, bit for bit (lobe_gate): not computed again
            float qq = gq[0];
#pragma unroll
            for (int jj = 1; jj < K; jj++) qq = (j == jj) ? gq[jj] : qq;
            const float om = 1.0f - qq;
            float contrib = __fdiv_rn(rw.wn, rw.wd) * (om * om);
            contrib = (((lj >> lane) & 1ull) != 0ull && qq < 1.0f && contrib > 0.0f) ? contrib : 0.0f;
            T.n_light += contrib > 0.0f ? 1u : 0u;
            const float chv[3] = {ch0, ch1, ch2};
#pragma unroll
            for (int c3 = 0; c3 < 3; c3++) {
              const float v = contrib * chv[c3];
              const unsigned long long fx = (unsigned long long)(v * 68719476736.0f);
              if (fx) atomicAdd(&s_acc[lane * 3 + c3], fx);
            }
          }
        }
      }
      if (L >= n_ev) break;     // (the primary path: the common leg to its end, nothing after it)
    }
  }
  T.n_rm_lane += rm_lane;
  T.n_rm_rows += rm_rows;
}

// W1: the first (and then only) march of a started path carries its Fresnel / aperture weight.  false = geometry first,
// and the path is marched again with the weight, one wavelength at a time, only where a lane ended inside the lobe
// pre-test (k_march's scheme: 6 % of the STARTED rays are lit on the bench frame, so the weight's 17 of 44 vector
// instructions per event are mostly wasted in the first march: measured in profiles/r05_march_variants.txt).
// SHARED: the wave looks ONE table entry up per sample (its lanes share the sample's pupil sub-cell, a block holds the whole
// tile) and the started paths' common leg is marched once (march_started_set); otherwise (independent pixels, blocks smaller
// than a wave tile, the weight on every event, a selection out of order) every started path is marched alone.
#ifndef LF_SHARED_WAVES
#define LF_SHARED_WAVES 6     // waves per SIMD of the shared-leg kernel with K > 1 (two ray states per lane: 76 .. 80 VGPR;
                              // a workgroup holds 2 waves per SIMD, so 5 runs as 4: 47 ms against 38 on the bench frame)
#endif
// MODE 0: every started path alone; 1 = SHARED (one table entry per wave and sample, the leg once: march_started_set)
// VAR (lf_march_events.h): what the weighted march can evaluate -- kVarCoat: the lens has a film somewhere
// (lf_set_lens_coatings); kVarFilt: the stop mask is read bilinearly (lf_set_mask_filter)
template <int K, bool W1, int MODE, int VAR>
__global__ __launch_bounds__(64 * kWgWaves, ((VAR & kVarOccl) ? 4 : K == 1 ? 8 : MODE == 1 ? LF_SHARED_WAVES : 6))   // (kVarOccl: as k_march)
void k_march_cull(const LfLensDev* __restrict__ lens, const LfPairsDev* __restrict__ pairs,
                  const int* __restrict__ seq_table, const LfProgRow* __restrict__ rec_table,
                  const LfWeightRow* __restrict__ wrec_table, const float* __restrict__ mask, MarchArgs a,
                  LfCullArgs cull, double* __restrict__ ghost, unsigned long long* __restrict__ accum,
                  unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long s_acc[64 * 3];
  __shared__ unsigned long long s_cnt[kMarchCounters];
  __shared__ int s_next, s_nlist;
  // the chunk's listed samples: the sample's place in the chunk (kListBits bits) and, above it, the pupil sub-cell the
  // listing pass drew for it (a stratified sample's: sxi | syi << kMaxSubcellBits, what lf_set_pupil_subcells allows)
  static_assert(2 * kMaxSubcellBits <= 32 - kListBits, "a listed sample's sub-cell does not fit beside its place in the chunk");
  __shared__ unsigned s_list[kListMax];
  __shared__ int2 s_meta[MODE == 1 ? kCullMaxPaths : 1];      // per path: events << 16 | events of the common leg; first row of its sequence
  __shared__ float s_chan[(VAR & kVarLights) ? kLightChan : LF_MAX_LAMBDA * 3];
  const int tid = threadIdx.x;
  if (tid < 64 * 3) s_acc[tid] = 0ull;
  march_channel_factors<VAR>(lens, s_chan, tid);
  if (tid < kMarchCounters) s_cnt[tid] = 0ull;
  if (tid == 0) { s_next = 0; s_nlist = 0; }
  if (MODE == 1 && tid < pairs->n && tid < kCullMaxPaths) {
    const int n_ev = pairs->ev_cnt[tid], i1 = pairs->ij[tid][0];
    s_meta[tid] = make_int2((n_ev << 16) | (i1 < 0 ? n_ev : lens->n_surf - 1 - i1), pairs->ev_off[tid]);
  }
  __syncthreads();

  // tile of the workgroup: as k_march (XCD-aware slot swizzle, wave tile = 8 rows x 8 columns 2^xs apart)
  const int tiles_x = ((a.W + (8 << a.xs) - 1) >> (3 + a.xs)) << a.xs;
#ifdef LF_EXPERIMENTS
  if (cull.wg_clock && tid == 0) cull.wg_clock[2 * (size_t)blockIdx.x] = wall_clock64();
  struct ClockAtExit { unsigned long long* p; __device__ ~ClockAtExit() { if (p && threadIdx.x == 0) *p = wall_clock64(); } }
      clock_at_exit{cull.wg_clock ? cull.wg_clock + 2 * (size_t)blockIdx.x + 1 : nullptr};
#endif
  // the launch's last tiles are split finer than the rest (a.tail_from): the grid ends on short workgroups
  const unsigned n_head = (unsigned)a.tail_from * (unsigned)a.sgroups;
  const bool tail = a.tail_groups > 1 && blockIdx.x >= n_head;
  const int sgroups = tail ? a.tail_groups : a.sgroups;
  const int sg = tail ? (int)((blockIdx.x - n_head) % (unsigned)sgroups) : (int)(blockIdx.x % (unsigned)sgroups);
  const unsigned slot = tail ? (unsigned)a.tail_from + (blockIdx.x - n_head) / (unsigned)sgroups : blockIdx.x / (unsigned)sgroups;
  const int tile_lin = (int)((slot & ~63u) | ((slot & 7u) << 3) | ((slot >> 3) & 7u));
  if (tile_lin >= a.n_tiles) return;
  int tx, trow;
  march_tile_of(a, tile_lin, tiles_x, tx, trow);
  const unsigned tile_id = (unsigned)(trow * tiles_x + tx);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int x = ((tx >> a.xs) << (3 + a.xs)) + ((lane & 7) << a.xs) + (tx & ((1 << a.xs) - 1)), y = trow * 8 + (lane >> 3);
  const bool active = x < a.W && y >= a.y0 && y < a.y1;
  const lanemask active_mask = __ballot(active);
  const unsigned p = (unsigned)y * (unsigned)a.W + (unsigned)x;
  // the tile's cull row: its columns and 8 rows lie inside one block -- unless the blocks are smaller than the tile
  // (cull.multi: 16 / 32-pixel blocks of a small frame), where every lane has the row of its own pixel's block
  const int blk = ((trow * 8) >> cull.blk_log2) * cull.blocks_x + ((((tx >> a.xs) << (3 + a.xs))) >> cull.blk_log2);
  const unsigned long long* const crow = cull.table + lf_cull_row_of_block(blk, cull.share_n, cull.share_nb) * (size_t)(cull.cells + 1);
  const int blk_lane = (min(y, a.H - 1) >> cull.blk_log2) * cull.blocks_x + (min(x, a.W - 1) >> cull.blk_log2);
  const unsigned long long* const crow_lane = cull.multi ? cull.table + lf_cull_row_of_block(blk_lane, cull.share_n, cull.share_nb) * (size_t)(cull.cells + 1) : crow;

  const float pitch = lens->pitch, pupil_h = lens->pupil_h, geom_norm = lens->geom_norm;
  const float half_w = a.half_w, half_h = a.half_h, vz_u = a.vz;
  const int GG = a.G * a.G;
  // do the lanes of a wave aim a stratified sample at ONE cell of the table?  (they share a sub-cell of the stratum;
  // the table has m cells per stratum axis)
  const bool per_lane = (1 << a.sub_bits) < cull.m;

  PathTally T;

  const int n_mine = (a.spp - sg + sgroups - 1) / sgroups;     // samples sg, sg + sgroups, ...
  for (int chunk0 = 0; chunk0 < n_mine; chunk0 += kListMax) {
    // ---- which of the tile's samples start any path at all (most do not) -----------------------------
    const int chunk_n = min(kListMax, n_mine - chunk0);
    for (int k = tid; k < chunk_n; k += 64 * kWgWaves) {
      const int s = sg + (chunk0 + k) * sgroups;
      bool work = true;     // (a sample whose lanes look their cells up one by one is listed: the sample loop finds out)
      unsigned drawn = 0u;
      if (s >= GG && !cull.multi) work = crow[cull.cells] != 0ull;
      if (s < GG) {
        // the sub-cell the wave's lanes all aim sample s at: drawn HERE, once for the tile's eight waves, and kept beside the
        // listed sample -- and its table cell, where the lanes share one
        const uint4 r2 = philox4x32_10(make_uint4(tile_id, (unsigned)s, kDomainSubcell, 0u), a.key);
        const unsigned sxi = a.sub_bits ? (r2.x >> (32 - a.sub_bits)) : 0u, syi = a.sub_bits ? (r2.y >> (32 - a.sub_bits)) : 0u;
        drawn = sxi | (syi << kMaxSubcellBits);
        if (!per_lane && !cull.multi) {
          const int cy = s / a.G, cx = s - cy * a.G;
          work = crow[(cy * cull.m + (int)((syi << cull.m_shift) >> a.sub_bits)) * cull.P + cx * cull.m + (int)((sxi << cull.m_shift) >> a.sub_bits)] != 0ull;
        }
      }
      if (work) s_list[atomicAdd(&s_nlist, 1)] = (unsigned)k | (drawn << kListBits);
    }
    __syncthreads();
    const int n_list = s_nlist;
    for (;;) {
      int k = 0;
      if (lane == 0) k = atomicAdd(&s_next, 1);
      k = __builtin_amdgcn_readfirstlane(k);
      if (k >= n_list) break;
      const unsigned listed = (unsigned)__builtin_amdgcn_readfirstlane((int)s_list[k]);
      const int s = sg + (chunk0 + (int)(listed & (unsigned)(kListMax - 1))) * sgroups;       // wave-uniform
      // ---- sensor sample -> initial ray (the expressions of k_march / sample_start) -----------------
      const uint4 rnd = philox4x32_10(make_uint4(p, (unsigned)s, kDomainMarch, 0u), a.key);
      const float jx = u01(rnd.x), jy = u01(rnd.y);
      float ua = u01(rnd.z), ub = u01(rnd.w);
      int entry = -1;
      if (s < GG) {
        const int cy = s / a.G, cx = s - cy * a.G;
        // the sub-cell the wave's lanes all aim sample s at, as the listing pass drew it
        const unsigned sxi = (listed >> kListBits) & ((1u << kMaxSubcellBits) - 1u);
        const unsigned syi = listed >> (kListBits + kMaxSubcellBits);
        ua = ((float)cx + ((float)sxi + ua) * a.inv_sub) * a.inv_G;
        ub = ((float)cy + ((float)syi + ub) * a.inv_sub) * a.inv_G;
        if (!per_lane) entry = (cy * cull.m + (int)((syi << cull.m_shift) >> a.sub_bits)) * cull.P + cx * cull.m + (int)((sxi << cull.m_shift) >> a.sub_bits);
      }
      // the paths to start: one scalar load for the wave -- or, where the lanes aim at different cells of the table
      // (independent pixels), each lane's own mask and their union.  An unstratified sample (s >= G * G: a sample count
      // that is no square) takes the block's union entry.
      if (s >= GG) entry = cull.cells;
      const float pa0 = fmaf(2.0f, ua, -1.0f), pb0 = fmaf(2.0f, ub, -1.0f);
      const float X = -(((float)x + jx) - half_w) * pitch;
      const float Y = -(((float)y + jy) - half_h) * pitch;
      if (MODE == 1) {
        const unsigned long long todo = crow[entry];
        if (todo == 0ull) continue;
        const StartRay s0 = aim_at_pupil(X, Y, pa0, pb0, pupil_h, vz_u, geom_norm);
        march_started_set<K, VAR>(lens, pairs, seq_table, rec_table, wrec_table, mask, a, todo, active_mask, X, Y, s0, lane, s_acc, s_meta, s_chan, T);
        continue;
      }
      unsigned long long mine, todo;
      if (entry >= 0 && !cull.multi) { todo = crow[entry]; mine = todo; }
      else {
        const int fx = min(cull.P - 1, (int)(ua * (float)cull.P)), fy = min(cull.P - 1, (int)(ub * (float)cull.P));
        mine = active ? crow_lane[entry >= 0 ? entry : fy * cull.P + fx] : 0ull;
        unsigned lo = (unsigned)mine, hi = (unsigned)(mine >> 32);
        for (int off = 32; off > 0; off >>= 1) { lo |= __shfl_xor(lo, off); hi |= __shfl_xor(hi, off); }
        todo = ((unsigned long long)__builtin_amdgcn_readfirstlane(hi) << 32) | (unsigned long long)__builtin_amdgcn_readfirstlane(lo);
      }
      if (todo == 0ull) continue;
      const StartRay s0 = aim_at_pupil(X, Y, pa0, pb0, pupil_h, vz_u, geom_norm);
      unsigned long long left_q = todo;
      while (left_q != 0ull) {
        const int q = __builtin_ctzll(left_q);
        left_q &= left_q - 1ull;
        const lanemask start_mask = active_mask & __ballot(((mine >> q) & 1ull) != 0ull);   // (all active lanes when the wave shares a cell)
        march_started_path<K, W1, VAR>(lens, pairs, seq_table, rec_table, wrec_table, mask, a, q, start_mask, X, Y, s0, lane, lane, s_acc, s_chan, T);
      }
    }
    __syncthreads();
    if (tid == 0) { s_next = 0; s_nlist = 0; }
    __syncthreads();
  }

  // ---- counters: one LDS add per wave, one global add per workgroup (slots as k_march: executed events =
  // events, every path marched on its own; no second march) ---------------------------------------------
  {
    unsigned long long v6 = T.n_light;
    for (int off = 32; off > 0; off >>= 1) v6 += __shfl_down(v6, off);
    const unsigned long long vals[kMarchCounters] = {T.n_rays, T.events, T.n_clip, T.n_vign, T.n_tir, T.n_scene, v6, T.executed, T.n_rm_lane, T.n_rm_rows};
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kMarchCounters; i++)
        if (vals[i]) atomicAdd(&s_cnt[i], vals[i]);
    }
  }
  __syncthreads();
  if (wave == 0 && lane < kMarchCounters && s_cnt[lane]) atomicAdd(&counters[lane], s_cnt[lane]);

  if (tail) {
    // a tile of the split tail: the integer sums of its workgroups meet in tail_acc; the LAST to arrive converts them (the same
    // conversion as a whole tile's: the sums do not depend on who added what) and leaves sums and arrivals zero for the next launch
    if (wave != 0) return;
    const unsigned tt = slot - (unsigned)a.tail_from;
    unsigned long long* const acc = cull.tail_acc + (size_t)tt * 192u;
#pragma unroll
    for (int c = 0; c < 3; c++)
      if (s_acc[lane * 3 + c]) atomicAdd(&acc[lane * 3 + c], s_acc[lane * 3 + c]);
    __threadfence();
    int arrived = 0;
    if (lane == 0) arrived = atomicAdd(&cull.tail_done[tt], 1);
    arrived = __shfl(arrived, 0);
    if (arrived != sgroups - 1) return;
    __threadfence();
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const unsigned long long sum = atomicExch(&acc[lane * 3 + c], 0ull);
      if (active) {
        const double v = ((double)sum * (1.0 / 68719476736.0)) / (double)a.spp;
        ghost[3 * (size_t)p + c] = a.accumulate ? ghost[3 * (size_t)p + c] + v : v;
      }
    }
    if (lane == 0) atomicExch(&cull.tail_done[tt], 0);
    return;
  }
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

// ---- the same march, COMPACTED: one lane = one (pixel, sample) that starts the path --------------------------
// Where every pixel draws its own pupil point (lf_set_pupil_subcells(0): the independent-pixel estimator) the lanes of
// a wave tile aim at different cells of the table, want different paths, and a wave that marches path q for its tile
// and sample does so with the few lanes that want it: the same events as the coherent specification in 2.4 x the
// time (profiles/r05_march_variants.txt).  Here the tile's workgroup first LISTS what is to be started -- for a chunk
// of samples every (pixel, sample) looks its mask up, the paths are counted by ballot, and the (pixel, sample) items
// are written into one LDS array sorted by path -- and then marches the list: a wave takes 64 items of ONE path,
// rebuilds each lane's start ray from its (pixel, sample) and marches with every lane started.  Sums are integers
// in LDS, so pixels and counters do not depend on the order: bit for bit the frame of k_march_cull and of the oracle.
constexpr int kItemCap = 16384;      // items of a chunk (2 bytes each)
constexpr int kItemChunk = 256;      // samples per chunk at most (8 bits of an item; the pixel takes 6)
constexpr int kItemCellCache = 64;   // chunks of up to this many samples keep each (sample, pixel)'s table cell between the two listing passes

template <int K, int VAR>
__global__ __launch_bounds__(64 * kWgWaves, (VAR & kVarOccl) ? 4 : 6)      // (kVarOccl: as k_march; 42 KB of LDS lists: three workgroups per CU)
void k_march_items(const LfLensDev* __restrict__ lens, const LfPairsDev* __restrict__ pairs,
                   const int* __restrict__ seq_table, const LfProgRow* __restrict__ rec_table,
                   const LfWeightRow* __restrict__ wrec_table, const float* __restrict__ mask, MarchArgs a,
                   LfCullArgs cull, double* __restrict__ ghost, unsigned long long* __restrict__ accum,
                   unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long s_acc[64 * 3];
  __shared__ unsigned long long s_cnt[kMarchCounters];
  __shared__ int s_pcount[kCullMaxPaths], s_poff[kCullMaxPaths + 1], s_goff[kCullMaxPaths + 1], s_pfill[kCullMaxPaths];
  __shared__ int s_next;
  __shared__ unsigned short s_items[kItemCap];
  __shared__ unsigned short s_cell[kItemCellCache * 64];      // the table cell of every (sample of the chunk, pixel): count -> fill
  __shared__ float s_chan[(VAR & kVarLights) ? kLightChan : LF_MAX_LAMBDA * 3];
  const int tid = threadIdx.x;
  if (tid < 64 * 3) s_acc[tid] = 0ull;
  march_channel_factors<VAR>(lens, s_chan, tid);
  if (tid < kMarchCounters) s_cnt[tid] = 0ull;
  __syncthreads();

  const int tiles_x = ((a.W + (8 << a.xs) - 1) >> (3 + a.xs)) << a.xs;
  const int sg = blockIdx.x % a.sgroups;
  const unsigned slot = blockIdx.x / a.sgroups;
  const int tile_lin = (int)((slot & ~63u) | ((slot & 7u) << 3) | ((slot >> 3) & 7u));
  if (tile_lin >= a.n_tiles) return;
  int tx, trow;
  march_tile_of(a, tile_lin, tiles_x, tx, trow);
  const unsigned tile_id = (unsigned)(trow * tiles_x + tx);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int n_paths = pairs->n;
  const float pitch = lens->pitch, pupil_h = lens->pupil_h, geom_norm = lens->geom_norm;
  const float half_w = a.half_w, half_h = a.half_h, vz_u = a.vz;
  const int GG = a.G * a.G;
  // the cull row of THIS lane's pixel (one block holds the whole tile unless the blocks are smaller than it: cull.multi)
  const unsigned long long* crow;
  {
    const int lx = ((tx >> a.xs) << (3 + a.xs)) + ((lane & 7) << a.xs) + (tx & ((1 << a.xs) - 1)), ly = trow * 8 + (lane >> 3);
    const int blk = cull.multi ? (min(ly, a.H - 1) >> cull.blk_log2) * cull.blocks_x + (min(lx, a.W - 1) >> cull.blk_log2)
                               : ((trow * 8) >> cull.blk_log2) * cull.blocks_x + ((((tx >> a.xs) << (3 + a.xs))) >> cull.blk_log2);
    crow = cull.table + lf_cull_row_of_block(blk, cull.share_n, cull.share_nb) * (size_t)(cull.cells + 1);
  }
  // pixel `px` of the tile (the lane order of k_march / k_march_cull)
  auto pixel_of = [&](int px, int& x, int& y) {
    x = ((tx >> a.xs) << (3 + a.xs)) + ((px & 7) << a.xs) + (tx & ((1 << a.xs) - 1));
    y = trow * 8 + (px >> 3);
    return x < a.W && y >= a.y0 && y < a.y1;
  };
  // sample s of pixel (x, y): the point of the pupil square it aims at (the expressions of sample_start), with the
  // pixel jitter beside it
  auto pupil_point = [&](int x, int y, int s, float& ua, float& ub, float& jx, float& jy) {
    const uint4 rnd = philox4x32_10(make_uint4((unsigned)y * (unsigned)a.W + (unsigned)x, (unsigned)s, kDomainMarch, 0u), a.key);
    jx = u01(rnd.x); jy = u01(rnd.y);
    ua = u01(rnd.z); ub = u01(rnd.w);
    if (s < GG) {
      const int cy = s / a.G, cx = s - cy * a.G;
      unsigned sxi = 0u, syi = 0u;
      if (a.sub_bits) {     // (no sub-cells, no draw: s differs from lane to lane here, the draw would be a vector one)
        const uint4 r2 = philox4x32_10(make_uint4(tile_id, (unsigned)s, kDomainSubcell, 0u), a.key);
        sxi = r2.x >> (32 - a.sub_bits); syi = r2.y >> (32 - a.sub_bits);
      }
      ua = ((float)cx + ((float)sxi + ua) * a.inv_sub) * a.inv_G;
      ub = ((float)cy + ((float)syi + ub) * a.inv_sub) * a.inv_G;
    }
  };
  // the paths pixel (lane) starts for the chunk's k-th sample: the mask of the table cell that holds its pupil point
  // ... as the index of its table entry (cells = the block's union entry: an unstratified sample; 0xffff: no pixel there)
  auto cell_of = [&](int k_global) -> unsigned {
    int x, y;
    if (!pixel_of(lane, x, y)) return 0xffffu;
    const int s = sg + k_global * a.sgroups;
    if (s >= GG) return (unsigned)cull.cells;
    float ua, ub, jx, jy;
    pupil_point(x, y, s, ua, ub, jx, jy);
    const int fx = min(cull.P - 1, (int)(ua * (float)cull.P)), fy = min(cull.P - 1, (int)(ub * (float)cull.P));
    return (unsigned)(fy * cull.P + fx);
  };
  auto mask_at = [&](unsigned cell) -> unsigned long long { return cell == 0xffffu ? 0ull : crow[cell]; };
  auto wave_or = [](unsigned long long v) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    for (int off = 32; off > 0; off >>= 1) { lo |= __shfl_xor(lo, off); hi |= __shfl_xor(hi, off); }
    return ((unsigned long long)__builtin_amdgcn_readfirstlane(hi) << 32) | (unsigned long long)__builtin_amdgcn_readfirstlane(lo);
  };

  PathTally T;
  const int n_mine = (a.spp - sg + a.sgroups - 1) / a.sgroups;     // samples sg, sg + sgroups, ...
  // (the chunk to begin with: what the table's started fraction says fits the item list -- a chunk that does not fit is
  // counted for nothing and halved)
  int c0 = 0, ch = min(max(1, min(kItemChunk, cull.items_chunk0)), n_mine);
  while (c0 < n_mine) {
    const int chn = min(ch, n_mine - c0);
    // ---- count: how many (pixel, sample) items of this chunk start each path (a wave = one sample's 64 pixels) ---
    if (tid < kCullMaxPaths) { s_pcount[tid] = 0; s_pfill[tid] = 0; }
    if (tid == 0) s_next = 0;
    __syncthreads();
    const bool cached = chn <= kItemCellCache;
    for (int k = wave; k < chn; k += kWgWaves) {
      const unsigned cell = cell_of(c0 + k);
      if (cached) s_cell[k * 64 + lane] = (unsigned short)cell;
      const unsigned long long mine = mask_at(cell);
      unsigned long long u = wave_or(mine);
      while (u != 0ull) {
        const int q = __builtin_ctzll(u);
        u &= u - 1ull;
        const int c = __popcll(__ballot(((mine >> q) & 1ull) != 0ull));
        if (lane == 0) atomicAdd(&s_pcount[q], c);
      }
    }
    __syncthreads();
    if (tid == 0) {
      int off = 0, goff = 0;
      for (int q = 0; q < n_paths; q++) { s_poff[q] = off; s_goff[q] = goff; off += s_pcount[q]; goff += (s_pcount[q] + 63) >> 6; }
      s_poff[n_paths] = off; s_goff[n_paths] = goff;
    }
    __syncthreads();
    const int total = s_poff[n_paths];
    if (total > kItemCap && chn > 1) {      // too many for the list: a shorter chunk (one sample's 64 x 46 always fit)
      ch = max(1, chn >> 1);
      __syncthreads();
      continue;
    }
    // ---- fill: the items, sorted by path ------------------------------------------------------------------------
    for (int k = wave; k < chn; k += kWgWaves) {
      const unsigned long long mine = mask_at(cached ? (unsigned)s_cell[k * 64 + lane] : cell_of(c0 + k));
      unsigned long long u = wave_or(mine);
      while (u != 0ull) {
        const int q = __builtin_ctzll(u);
        u &= u - 1ull;
        const lanemask b = __ballot(((mine >> q) & 1ull) != 0ull);
        int base = 0;
        if (lane == 0) base = atomicAdd(&s_pfill[q], (int)__popcll(b));
        base = __builtin_amdgcn_readfirstlane(base);
        if ((b >> lane) & 1ull)
          s_items[s_poff[q] + base + (int)__popcll(b & ((1ull << lane) - 1ull))] = (unsigned short)((k << 6) | lane);
      }
    }
    __syncthreads();
    // ---- march the list: 64 items of one path per wave ------------------------------------------------------------
    const int n_groups_total = s_goff[n_paths];
    for (;;) {
      int gi = 0;
      if (lane == 0) gi = atomicAdd(&s_next, 1);
      gi = __builtin_amdgcn_readfirstlane(gi);
      if (gi >= n_groups_total) break;
      int q = 0;
      while (s_goff[q + 1] <= gi) q++;      // (wave-uniform: the path whose groups hold gi)
      const int first = s_poff[q] + ((gi - s_goff[q]) << 6), end = s_poff[q] + s_pcount[q];
      const bool have = first + lane < end;
      const unsigned item = have ? (unsigned)s_items[first + lane] : 0u;
      const int px = (int)(item & 63u), s = sg + (c0 + (int)(item >> 6)) * a.sgroups;
      int x, y;
      (void)pixel_of(px, x, y);
      float ua, ub, jx, jy;
      pupil_point(x, y, s, ua, ub, jx, jy);
      const float X = -(((float)x + jx) - half_w) * pitch;
      const float Y = -(((float)y + jy) - half_h) * pitch;
      const StartRay s0 = aim_at_pupil(X, Y, fmaf(2.0f, ua, -1.0f), fmaf(2.0f, ub, -1.0f), pupil_h, vz_u, geom_norm);
      march_started_path<K, false, VAR>(lens, pairs, seq_table, rec_table, wrec_table, mask, a, q, __ballot(have), X, Y, s0, lane, px, s_acc, s_chan, T);
    }
    __syncthreads();
    c0 += chn;
  }

  {
    unsigned long long v6 = T.n_light;
    for (int off = 32; off > 0; off >>= 1) v6 += __shfl_down(v6, off);
    const unsigned long long vals[kMarchCounters] = {T.n_rays, T.events, T.n_clip, T.n_vign, T.n_tir, T.n_scene, v6, T.executed, T.n_rm_lane, T.n_rm_rows};
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kMarchCounters; i++)
        if (vals[i]) atomicAdd(&s_cnt[i], vals[i]);
    }
  }
  __syncthreads();
  if (wave == 0 && lane < kMarchCounters && s_cnt[lane]) atomicAdd(&counters[lane], s_cnt[lane]);
  int x, y;
  const bool active = pixel_of(lane, x, y);
  if (wave == 0 && active) {
    const size_t p = (size_t)y * (size_t)a.W + (size_t)x;
    if (a.sgroups == 1) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double v = ((double)s_acc[lane * 3 + c] * (1.0 / 68719476736.0)) / (double)a.spp;
        ghost[3 * p + c] = a.accumulate ? ghost[3 * p + c] + v : v;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++)
        if (s_acc[lane * 3 + c]) atomicAdd(&accum[3 * p + c], s_acc[lane * 3 + c]);
    }
  }
}

}  // namespace

constexpr int kMarchTailTilesMax = 4096;
lf_status lfk_march_culled(lf_ctx* ctx, const MarchArgs& a_in, size_t blocks, size_t dyn_lds) {
  const LfApertureDev& m = ctx->ap[LF_APERTURE_STARBURST];
  MarchArgs a = a_in;
  LfCullArgs c;
  c.table = ctx->cull_dev; c.blocks_x = ctx->cull_bx; c.blocks_y = ctx->cull_by; c.cells = ctx->cull_cells;
  c.share_n = ctx->cull_resident.n; c.share_nb = ctx->cull_resident.nb;
  c.blk_log2 = ctx->cull_blk_log2;
  c.multi = ctx->cull_blk_log2 < 3 + a.xs ? 1 : 0;
  // the started paths' common leg is marched once (march_started_set) if a higher path index never leaves it later:
  // the primary path in front, the pairs by ascending first mirror -- the order lf_set_ghost_pairs(NULL) and any sorted list give
  c.prefix_ok = 1;
  for (int q = 1; q < ctx->pairs.n; q++) {
    const int ia = ctx->pairs.ij[q - 1][0], ib = ctx->pairs.ij[q][0];
    if (ib < 0 || (ia >= 0 && ib < ia)) c.prefix_ok = 0;
  }
  if (ctx->cull_no_prefix) c.prefix_ok = 0;
  c.P = ctx->cull_P; c.m = ctx->cull_m; c.m_shift = ctx->cull_m == 4 ? 2 : ctx->cull_m == 2 ? 1 : 0;
  hipEvent_t ev = lf_timing_begin(ctx, LFK_MARCH);
#define LF_LAUNCH_CULL1(KK, WW, SS)  do { switch (var) { case kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarCoatFilt); break; case kVarFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarFilt); break; \
                                                      case kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarCoat); break; case kVarBare: LF_LAUNCH_CULL2(KK, WW, SS, kVarBare); break; \
                                                      case kVarLights | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarLights | kVarCoatFilt); break; \
                                                      case kVarLights | kVarFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarLights | kVarFilt); break; \
                                                      case kVarLights | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarLights | kVarCoat); break; \
                                                      case kVarStack | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarStack | kVarCoat); break; \
                                                      case kVarStack | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarStack | kVarCoatFilt); break; \
                                                      case kVarStack | kVarLights | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarStack | kVarLights | kVarCoat); break; \
                                                      case kVarStack | kVarLights | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarStack | kVarLights | kVarCoatFilt); break; \
                                                      case kVarOccl | kVarLights | kVarBare: LF_LAUNCH_CULL2(KK, WW, SS, kVarOccl | kVarLights | kVarBare); break; \
                                                  case kVarOccl | kVarLights | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarOccl | kVarLights | kVarCoat); break; \
                                                  case kVarOccl | kVarLights | kVarFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarOccl | kVarLights | kVarFilt); break; \
                                                  case kVarOccl | kVarLights | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarOccl | kVarLights | kVarCoatFilt); break; \
                                                  case kVarOccl | kVarStack | kVarLights | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarOccl | kVarStack | kVarLights | kVarCoat); break; \
                                                  case kVarOccl | kVarStack | kVarLights | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarOccl | kVarStack | kVarLights | kVarCoatFilt); break; \
                                                      case kVarNear | kVarLights | kVarBare: LF_LAUNCH_CULL2(KK, WW, SS, kVarNear | kVarLights | kVarBare); break; \
                                                      case kVarNear | kVarLights | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarNear | kVarLights | kVarCoat); break; \
                                                      case kVarNear | kVarLights | kVarFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarNear | kVarLights | kVarFilt); break; \
                                                      case kVarNear | kVarLights | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarNear | kVarLights | kVarCoatFilt); break; \
                                                      case kVarNear | kVarStack | kVarLights | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarNear | kVarStack | kVarLights | kVarCoat); break; \
                                                      case kVarNear | kVarStack | kVarLights | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarNear | kVarStack | kVarLights | kVarCoatFilt); break; \
                                                      case kVarNear | kVarOccl | kVarLights | kVarBare: LF_LAUNCH_CULL2(KK, WW, SS, kVarNear | kVarOccl | kVarLights | kVarBare); break; \
                                                      case kVarNear | kVarOccl | kVarLights | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarNear | kVarOccl | kVarLights | kVarCoat); break; \
                                                      case kVarNear | kVarOccl | kVarLights | kVarFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarNear | kVarOccl | kVarLights | kVarFilt); break; \
                                                      case kVarNear | kVarOccl | kVarLights | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarNear | kVarOccl | kVarLights | kVarCoatFilt); break; \
                                                      case kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoat); break; \
                                                      case kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoatFilt); break; \
                                                      case kVarArea | kVarNear | kVarLights | kVarBare: LF_LAUNCH_CULL2(KK, WW, SS, kVarArea | kVarNear | kVarLights | kVarBare); break; \
                                                      case kVarArea | kVarNear | kVarLights | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarArea | kVarNear | kVarLights | kVarCoat); break; \
                                                      case kVarArea | kVarNear | kVarLights | kVarFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarArea | kVarNear | kVarLights | kVarFilt); break; \
                                                      case kVarArea | kVarNear | kVarLights | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarArea | kVarNear | kVarLights | kVarCoatFilt); break; \
                                                      case kVarArea | kVarNear | kVarStack | kVarLights | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarArea | kVarNear | kVarStack | kVarLights | kVarCoat); break; \
                                                      case kVarArea | kVarNear | kVarStack | kVarLights | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarArea | kVarNear | kVarStack | kVarLights | kVarCoatFilt); break; \
                                                      case kVarArea | kVarNear | kVarOccl | kVarLights | kVarBare: LF_LAUNCH_CULL2(KK, WW, SS, kVarArea | kVarNear | kVarOccl | kVarLights | kVarBare); break; \
                                                      case kVarArea | kVarNear | kVarOccl | kVarLights | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarArea | kVarNear | kVarOccl | kVarLights | kVarCoat); break; \
                                                      case kVarArea | kVarNear | kVarOccl | kVarLights | kVarFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarArea | kVarNear | kVarOccl | kVarLights | kVarFilt); break; \
                                                      case kVarArea | kVarNear | kVarOccl | kVarLights | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarArea | kVarNear | kVarOccl | kVarLights | kVarCoatFilt); break; \
                                                      case kVarArea | kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoat: LF_LAUNCH_CULL2(KK, WW, SS, kVarArea | kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoat); break; \
                                                      case kVarArea | kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoatFilt: LF_LAUNCH_CULL2(KK, WW, SS, kVarArea | kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoatFilt); break; \
                                                  default: LF_LAUNCH_CULL2(KK, WW, SS, kVarLights | kVarBare); break; } } while (0)
#define LF_LAUNCH_CULL2(KK, WW, SS, CC)                                                                       \
  hipLaunchKernelGGL((k_march_cull<KK, WW, SS, CC>), dim3((unsigned)blocks), dim3(64 * kWgWaves), dyn_lds, ctx->stream, ctx->lens_dev, \
                     ctx->pairs_dev, (const int*)(ctx->prog_dev + ctx->prog_seq_off),                         \
                     (const LfProgRow*)(ctx->prog_dev + ctx->prog_rec_off),                                  \
                     (const LfWeightRow*)(ctx->prog_dev + ctx->prog_wrec_off), m.texels, a, c, ctx->ghost,   \
                     ctx->accum, ctx->counters_dev)
#define LF_LAUNCH_ITEMS(KK)  do { switch (var) { case kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarCoatFilt); break; case kVarFilt: LF_LAUNCH_ITEMS2(KK, kVarFilt); break; \
                                              case kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarCoat); break; case kVarBare: LF_LAUNCH_ITEMS2(KK, kVarBare); break; \
                                              case kVarLights | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarLights | kVarCoatFilt); break; \
                                              case kVarLights | kVarFilt: LF_LAUNCH_ITEMS2(KK, kVarLights | kVarFilt); break; \
                                              case kVarLights | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarLights | kVarCoat); break; \
                                              case kVarStack | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarStack | kVarCoat); break; \
                                              case kVarStack | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarStack | kVarCoatFilt); break; \
                                              case kVarStack | kVarLights | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarStack | kVarLights | kVarCoat); break; \
                                              case kVarStack | kVarLights | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarStack | kVarLights | kVarCoatFilt); break; \
                                              case kVarOccl | kVarLights | kVarBare: LF_LAUNCH_ITEMS2(KK, kVarOccl | kVarLights | kVarBare); break; \
                                                  case kVarOccl | kVarLights | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarOccl | kVarLights | kVarCoat); break; \
                                                  case kVarOccl | kVarLights | kVarFilt: LF_LAUNCH_ITEMS2(KK, kVarOccl | kVarLights | kVarFilt); break; \
                                                  case kVarOccl | kVarLights | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarOccl | kVarLights | kVarCoatFilt); break; \
                                                  case kVarOccl | kVarStack | kVarLights | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarOccl | kVarStack | kVarLights | kVarCoat); break; \
                                                  case kVarOccl | kVarStack | kVarLights | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarOccl | kVarStack | kVarLights | kVarCoatFilt); break; \
                                              case kVarNear | kVarLights | kVarBare: LF_LAUNCH_ITEMS2(KK, kVarNear | kVarLights | kVarBare); break; \
                                              case kVarNear | kVarLights | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarNear | kVarLights | kVarCoat); break; \
                                              case kVarNear | kVarLights | kVarFilt: LF_LAUNCH_ITEMS2(KK, kVarNear | kVarLights | kVarFilt); break; \
                                              case kVarNear | kVarLights | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarNear | kVarLights | kVarCoatFilt); break; \
                                              case kVarNear | kVarStack | kVarLights | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarNear | kVarStack | kVarLights | kVarCoat); break; \
                                              case kVarNear | kVarStack | kVarLights | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarNear | kVarStack | kVarLights | kVarCoatFilt); break; \
                                              case kVarNear | kVarOccl | kVarLights | kVarBare: LF_LAUNCH_ITEMS2(KK, kVarNear | kVarOccl | kVarLights | kVarBare); break; \
                                              case kVarNear | kVarOccl | kVarLights | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarNear | kVarOccl | kVarLights | kVarCoat); break; \
                                              case kVarNear | kVarOccl | kVarLights | kVarFilt: LF_LAUNCH_ITEMS2(KK, kVarNear | kVarOccl | kVarLights | kVarFilt); break; \
                                              case kVarNear | kVarOccl | kVarLights | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarNear | kVarOccl | kVarLights | kVarCoatFilt); break; \
                                              case kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoat); break; \
                                              case kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoatFilt); break; \
                                              case kVarArea | kVarNear | kVarLights | kVarBare: LF_LAUNCH_ITEMS2(KK, kVarArea | kVarNear | kVarLights | kVarBare); break; \
                                              case kVarArea | kVarNear | kVarLights | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarArea | kVarNear | kVarLights | kVarCoat); break; \
                                              case kVarArea | kVarNear | kVarLights | kVarFilt: LF_LAUNCH_ITEMS2(KK, kVarArea | kVarNear | kVarLights | kVarFilt); break; \
                                              case kVarArea | kVarNear | kVarLights | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarArea | kVarNear | kVarLights | kVarCoatFilt); break; \
                                              case kVarArea | kVarNear | kVarStack | kVarLights | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarArea | kVarNear | kVarStack | kVarLights | kVarCoat); break; \
                                              case kVarArea | kVarNear | kVarStack | kVarLights | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarArea | kVarNear | kVarStack | kVarLights | kVarCoatFilt); break; \
                                              case kVarArea | kVarNear | kVarOccl | kVarLights | kVarBare: LF_LAUNCH_ITEMS2(KK, kVarArea | kVarNear | kVarOccl | kVarLights | kVarBare); break; \
                                              case kVarArea | kVarNear | kVarOccl | kVarLights | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarArea | kVarNear | kVarOccl | kVarLights | kVarCoat); break; \
                                              case kVarArea | kVarNear | kVarOccl | kVarLights | kVarFilt: LF_LAUNCH_ITEMS2(KK, kVarArea | kVarNear | kVarOccl | kVarLights | kVarFilt); break; \
                                              case kVarArea | kVarNear | kVarOccl | kVarLights | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarArea | kVarNear | kVarOccl | kVarLights | kVarCoatFilt); break; \
                                              case kVarArea | kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoat: LF_LAUNCH_ITEMS2(KK, kVarArea | kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoat); break; \
                                              case kVarArea | kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoatFilt: LF_LAUNCH_ITEMS2(KK, kVarArea | kVarNear | kVarOccl | kVarStack | kVarLights | kVarCoatFilt); break; \
                                                  default: LF_LAUNCH_ITEMS2(KK, kVarLights | kVarBare); break; } } while (0)
#define LF_LAUNCH_ITEMS2(KK, CC)                                                                             \
  hipLaunchKernelGGL((k_march_items<KK, CC>), dim3((unsigned)blocks), dim3(64 * kWgWaves), dyn_lds, ctx->stream, ctx->lens_dev, \
                     ctx->pairs_dev, (const int*)(ctx->prog_dev + ctx->prog_seq_off),                         \
                     (const LfProgRow*)(ctx->prog_dev + ctx->prog_rec_off),                                  \
                     (const LfWeightRow*)(ctx->prog_dev + ctx->prog_wrec_off), m.texels, a, c, ctx->ghost,   \
                     ctx->accum, ctx->counters_dev)
#define LF_LAUNCH_CULL(KK) do { if (items) LF_LAUNCH_ITEMS(KK); else if (weights_first) LF_LAUNCH_CULL1(KK, true, 0); \
                                else if (shared_leg) LF_LAUNCH_CULL1(KK, false, 1); else LF_LAUNCH_CULL1(KK, false, 0); } while (0)
  const bool weights_first = ctx->cull_weights_first;   // (lf_test_knob: the weight on every executed event)
  const int var = lf_march_variant(ctx);                // the variant that evaluates films / the bilinear mask
  // every pixel its own pupil point (no sub-cells at all): the compacted march.  (2 x 2 sub-cells, where the lanes of a
  // wave still look their cells up one by one, stay with k_march_cull: 48 against 59 ms on the bench frame)
  bool items = ctx->march_sub_bits == 0;
#ifdef LF_EXPERIMENTS
  if (const char* e = std::getenv("LF_CULL_ITEMS")) items = std::atoi(e) != 0;
#endif
  // one table entry per (wave tile, sample) and a selection in order: the started paths' common leg once (march_started_set)
  const bool shared_leg = c.prefix_ok && !c.multi && (1 << a.sub_bits) >= c.m;
  // ---- the tail: a launch drains for as long as its last workgroups run -- 0.65 to 1.7 ms for a tile of the bench frame,
  // during which the resident slots empty one by one (measured per workgroup, wall clock at start and end: half of the 768
  // slots idle over the last 0.7 ms of a 5 ms launch, 1/8 of the frame).  The LAST tiles (half a round of resident
  // workgroups) are therefore split over `tail_groups` workgroups each (samples sg, sg + groups, ...): the launch ends on
  // workgroups a quarter as long.  Whole tiles write their pixels themselves, split ones meet in tail_acc (k_march_cull).
  // 1/8, 1/4, 1/2 of the bench frame: 5.00 -> 4.83, 9.46 -> 9.32, 18.40 -> 18.34 ms; all of it: 36.5 -> 36.4; more groups or a
  // longer tail cost more than they save (a split tile repeats the workgroup's set-up and ends on 8 waves waiting for one)
  // (profiles/r06_cull_bounds.txt, 7.)
  a.tail_from = 0; a.tail_groups = 1; c.tail_acc = nullptr; c.tail_done = nullptr;
  {
    // k_march_items: a (sample, 64 pixels) wave lists about 64 x paths x the table's started fraction items; the chunk to begin
    // with is the power of two of samples that fits the list with a third to spare (blocks differ)
    const double per_sample = 64.0 * (double)std::max(1, ctx->pairs.n) * std::max(1e-4, ctx->cull_started_fraction) * 1.35;
    int ch0 = 256;
    while (ch0 > 1 && (double)ch0 * per_sample > (double)kItemCap) ch0 >>= 1;
    c.items_chunk0 = ch0;
  }
  if (!items && a.sgroups == 1 && !weights_first) {
    hipDeviceProp_t prop;
    LF_HIP(ctx, hipGetDeviceProperties(&prop, ctx->device));
    const int resident = prop.multiProcessorCount * (ctx->march_k == 1 ? 4 : 3);     // workgroups of 8 waves at 8 / 6 waves per SIMD
    int tail_tiles = ctx->march_tail_tiles >= 0 ? ctx->march_tail_tiles : resident / 2;
    int groups = ctx->march_tail_groups >= 0 ? ctx->march_tail_groups : 4;
    while (groups > 1 && groups * 32 > a.spp) groups /= 2;
    const int tiles_pad = (a.n_tiles + 63) / 64 * 64;
    tail_tiles = std::min(std::min(tail_tiles, kMarchTailTilesMax), tiles_pad) / 64 * 64;
    if (groups > 1 && tail_tiles > 0) {
      if (!ctx->tail_acc) {
        LF_HIP(ctx, hipMalloc((void**)&ctx->tail_acc, (size_t)kMarchTailTilesMax * 192 * sizeof(unsigned long long)));
        LF_HIP(ctx, hipMalloc((void**)&ctx->tail_done, (size_t)kMarchTailTilesMax * sizeof(int)));
        LF_HIP(ctx, hipMemsetAsync(ctx->tail_acc, 0, (size_t)kMarchTailTilesMax * 192 * sizeof(unsigned long long), ctx->stream));
        LF_HIP(ctx, hipMemsetAsync(ctx->tail_done, 0, (size_t)kMarchTailTilesMax * sizeof(int), ctx->stream));
      }
      a.tail_from = tiles_pad - tail_tiles; a.tail_groups = groups;
      c.tail_acc = ctx->tail_acc; c.tail_done = ctx->tail_done;
      blocks = (size_t)a.tail_from + (size_t)tail_tiles * groups;
    }
  }
#ifdef LF_EXPERIMENTS
  c.wg_clock = nullptr;
  const char* clock_file = std::getenv("LF_MARCH_WG_CLOCK");
  if (clock_file) {
    LF_HIP(ctx, hipMalloc((void**)&c.wg_clock, blocks * 16));
    LF_HIP(ctx, hipMemset(c.wg_clock, 0, blocks * 16));
    LF_HIP(ctx, hipDeviceSynchronize());
  }
#endif
  switch (ctx->march_k) {
    case 1: LF_LAUNCH_CULL(1); break;
    case 2: LF_LAUNCH_CULL(2); break;
    default: LF_LAUNCH_CULL(3); break;
  }
#undef LF_LAUNCH_CULL
#undef LF_LAUNCH_CULL1
#undef LF_LAUNCH_CULL2
#undef LF_LAUNCH_ITEMS
#undef LF_LAUNCH_ITEMS2
  lf_timing_end(ctx, LFK_MARCH, ev);
  LF_HIP(ctx, hipGetLastError());
#ifdef LF_EXPERIMENTS
  if (clock_file) {
    LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<unsigned long long> h(blocks * 2);
    LF_HIP(ctx, hipMemcpy(h.data(), c.wg_clock, blocks * 16, hipMemcpyDeviceToHost));
    if (FILE* f = std::fopen(clock_file, "wb")) { std::fwrite(h.data(), 8, h.size(), f); std::fclose(f); }
    (void)hipFree(c.wg_clock);
  }
#endif
  return LF_OK;
}
