// lf_cull_prepass.hip -- which marches are worth starting (rounds 5 and 6): the cull table, from the pre-pass to its audit.
// The north star's loop -- for each sensor sample, enumerate the ghost pairs, march each path, accumulate --
// leaves open which of those marches are worth starting.  On the bench frame 99.4 % of the (wave tile, sample,
// path, wavelength) combinations end with no lane inside the sun's lobe: their paths run into a diaphragm or
// leave the front element pointing elsewhere, and add exactly 0 to the sensor (profiles/r05_pair_table.json).
// Which ones can be known in advance: for a path q the map (sensor point x, pupil point u) -> exit direction
// is smooth, so over a small 4-D box (a block of 64 x 64 sensor pixels times one cell of the pupil square)
// a handful of marched rays bound where the whole box can go -- on every diaphragm of the path and in
// direction space when it leaves the lens.
//
// Here that knowledge is built (lfk_cull_prepass: level by level, or resolved from the cached sun-independent tree), counted and
// audited (lfk_cull_finish); the march that starts only what it enables is lf_cull.hip.
//   k_cull_level     the pre-pass, coarse to fine over the pupil square (levels P = 8 -> 16 -> 32 -> P_final, four
//                    children per kept box, work lists per path): one LANE = one box (sensor block, pupil cell,
//                    path) with its 15 rays in registers -- 13 at the middle wavelength (a 3 x 3 grid over the cell
//                    whose corners sit on the block's corners, + the cell's centre at the block's +-x, +-y edges) and
//                    the centre at both ends of the spectrum -- marched WITHOUT dying on a diaphragm.  The footprint of
//                    a box on an interface is a zonotope (centre + central-difference generators along the two pupil and
//                    two sensor axes, inflated, + a second-order slack); the box is dropped when a separating axis puts
//                    it wholly outside the clear aperture (the stop: outside its housing or on closed cells of the mask's
//                    occupancy grid), at the end the same in direction space against the sun's lobe.  What the samples
//                    CANNOT bound is kept: a box that lost a sample (to total reflection or a missed sphere: the map is not
//                    Lipschitz at that edge), a box whose samples all end unless the bound of the pass scalar stays below
//                    zero.  Result: per (block, cell) a 64-bit mask of the paths that may contribute.
//                    Round 6: the rules are round 5's, the kernel is not -- it builds a footprint only where a test can
//                    fire (the centre sample outside the clear aperture, the stop, the exit) instead of after every event
//                    of every box, needs no scratch, and builds the SAME table bit for bit in half the time (14.1 -> 6.9 ms
//                    on the bench frame); k_cull_level_general keeps round 5's kernel with the rules as arguments, for the
//                    regression test and for the rules that were replaced (lf_test_knob).
//   k_cull_audit     every table is CHECKED where it is used: a ray of every (block, cell, path) box it does not start,
//                    marched with the march's own events; one that reaches the light refutes the table and the launch
//                    marches everything (lf_set_cull_audit).  1.7 ms on the bench frame.
// WHAT THE BOUNDS ARE.  A second-order Taylor estimate of the bundle's map over the box from finite differences of 15
// rays -- the 4 first derivatives and the 4 pure second derivatives measured, of the 6 mixed ones two sums -- with
// factors for what is not measured (x 1.25 on the generators, x 1.2 on the lobe test) that were FOUND: lowered, each
// loses its first lit ray between x 0.9 and x 1.0.  They are not proofs.  Round 6 tried to replace them by proofs
// and by a complete model (profiles/r06_cull_bounds.txt): affine arithmetic on the box itself (every operation of the
// march as a form with a rigorous remainder, private terms folded back into the bundle's frame after every event) is
// sound by construction but its remainders compound over the 11 - 27 events of a path -- at the table's resolution it
// starts 50 % of everything against 7.7 %; a 17-ray stencil that measures all ten second derivatives with a geometric
// estimate of the third order starts 7.6 % and lost light on one of 160 random frames.  So the rules stand as round 5
// left them, on the evidence of the search (tests/cull_fuzz.py: 39 000 + this round's frames, none differing) -- and
// since a search covers what it drew, the AUDIT ships with them.
//
// No reference counterpart: the reference enumerates 13 fixed pairs per channel and draws each as one textured
// quad (src/pathtracer/pathtracer.cpp:735-762, :452-508) -- its "cull" is that a quad covers few pixels.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lf_internal.h"
#include "lf_march_events.h"
#include "lf_march_common.h"

namespace {

using namespace lfm;

constexpr int kCullSamples = 15;   // per box, at the middle wavelength: a 3 x 3 grid over the pupil cell (0 .. 8, 4 = the
                                   // centre; the mid-edge ones at the block's centre, the corners on the block's
                                   // corners) + the cell's centre at the block's +x, -x, +y, -y edges (9 .. 12);
                                   // and the centre sample at the first and the last wavelength (13, 14)
struct CullLevelArgs {
  int W, H;
  float pitch, half_w, half_h;
  int blocks_x, blocks_y, blk_log2;
  int share_rank, share_n, share_nb;   // a shared table (lf_cull_row_of_block): the first level runs this rank's blocks only
  int P;                   // pupil cells per axis at THIS level
  int P_final;             // ... of the table (the last level)
  int last;                // the last level writes the table, the others the next level's work list
  int n_paths;
  int lam[3];              // the wavelengths marched: the middle one (13 samples), the first and the last (the centre sample)
  int march_k, prog_recs;  // how the record table is grouped (lf_march.hip pack_program)
  float pupil_h, vz, geom_norm;
  float stop_h, inv_stop_h;
  float sx, sy, rho;       // the sun's direction (x, y) and the lobe's radius in direction space
  float margin;            // footprint inflation at this level
  float geo_margin;        // ... of the zonotope's generators alone (experiments: LF_CULL_GEO_MARGIN)
  int strict;              // footprint tests: 0 every box, 1 (shipped) only boxes with EVERY sample alive, 2 not for boxes that lost samples to
                           // total reflection (a missed sphere has the same square-root edge: two frames of a harsher random draw, wide
                           // suns on a perturbed 8-wavelength prescription, lost 19 and 213 lit rays under 2)
  int strict_lost;         // "all samples end here" by a scalar zonotope bound instead of the range rule
  float lobe_k;            // the footprint in direction space once more inflated for the lobe test (third order: a small lobe sees it)
  int slack_mode;          // experiments: LF_CULL_SLACK (1: second order summed over the four axes + twice the corners' cross terms)
  int keep_partial;        // a box that lost samples (total reflection, a missed sphere) is never dropped by the lobe test
  float lost_rel, lost_abs;  // "every sample ends here" drops a box only beyond this margin (see firmly_lost)
  int disable;             // experiments: bit 0 no aperture test, 1 no mask test, 2 no lobe test, 3 no all-samples-lost test
  unsigned list_stride;    // entries per path in the work lists
  unsigned occ[kCullOcc];  // occupancy rows of the stop mask
  // several lights (lf_set_lights): sx, sy, rho of every light the table is built for (entry 0 = the three above); a box
  // is dropped by the lobe test only if EVERY light's lobe rules it out
  int n_lights;
  float lsx[LF_MAX_LIGHTS], lsy[LF_MAX_LIGHTS], lrho[LF_MAX_LIGHTS];
};

// A glass event of the pre-pass: the arithmetic of surface_event<false> (lf_march_events.h) WITHOUT a clear aperture
// -- the sample goes on wherever the sphere is -- that also hands out HOW FAR the sample is from being lost:
// disc (< 0: no intersection) and, for a refraction, tir = (n' cos t')^2 / (|disc| + |n'^2 - n^2|) (< 0: total
// reflection), relative and of order 1 away from the boundary.  Not bit-critical: nothing here reaches a pixel.
// (The raw (n' cos t')^2 with one scale per box saves the reciprocal and 1.5 ms of the bench frame's pre-pass but
// loses its first lit ray on 3.6 mm blocks instead of 4.8 mm: profiles/r05_march_variants.txt.)
__device__ __forceinline__ void virtual_event(Ray& r, const LfProgRow& w, float cn22, float rn2, float delta, bool reflect,
                                              bool flat, float& disc_out, float& tir) {
  const float oz = r.hz + w.dzv;
  const float od = fmaf(r.px, r.dx, fmaf(r.py, r.dy, oz * r.dz));
  const float oo = fmaf(oz, oz, fmaf(r.px, r.px, r.py * r.py));
  const float Fh = fmaf(w.ch, oo, -oz);
  const float G = fmaf(-w.curv, od, r.dz);
  const float disc = fmaf(G, G, -(cn22 * Fh));
  disc_out = disc;
  const float sq = lf_sqrt(disc);
  const float t = flat ? (Fh + Fh) * lf_rcp(fmaf(w.sgn, sq, G)) : fmaf(-w.sgn, sq, G) * rn2;
  const float hx = fmaf(t, r.dx, r.px), hy = fmaf(t, r.dy, r.py), hz = fmaf(t, r.dz, oz);
  if (reflect) {
    tir = 1.0f;
    const float m = sq * (w.c2 * w.sgn);
    r.dx = fmaf(m, hx, r.dx); r.dy = fmaf(m, hy, r.dy); r.dz = fmaf(m, hz, fmaf(-2.0f * w.sgn, sq, r.dz));
  } else {
    const float k2 = disc + delta;
    tir = k2 * lf_rcp(fabsf(disc) + fabsf(delta) + 1e-30f);
    const float gs = lf_sqrt(k2) - sq, gcs = gs * w.sc;
    r.dx = fmaf(-gcs, hx, r.dx); r.dy = fmaf(-gcs, hy, r.dy); r.dz = fmaf(-gcs, hz, fmaf(w.sgn, gs, r.dz));
  }
  r.px = hx; r.py = hy; r.hz = hz;
}

// One LANE = one box (sensor block x pupil cell) of path blockIdx.y; its 13 rays live in registers, so a wave
// marches 64 boxes of ONE path in lockstep -- wave-uniform event sequence, rows through the scalar cache, no
// cross-lane traffic.  (The first version gave a box to a 16-lane row and reduced with ds_bpermute: 19 ms
// for the bench frame's 6e6 boxes at P = 16; profiles/r05_march_variants.txt.)
// Work: `items` = this level's list for the path (cell index = block * P * P + cell; null = every box of the
// level); a box that cannot be ruled out appends its four children to `next` (cells of 2P) or, on the last
// level, sets the path's bit in the table.
#ifndef LF_CULL_WAVES
#define LF_CULL_WAVES 3      // waves per SIMD: 2 / 3 / 4 -> 8.6 / 7.15 / 18.8 ms on the bench frame (193 / 168 / 128 VGPR)
#endif
#ifndef LF_CULL_WG
#define LF_CULL_WG 64        // lanes per workgroup: 256 / 128 / 64 -> 7.18 / 7.11 / 6.95 ms (a wave of decided boxes frees its slot at once)
#endif
__global__ __launch_bounds__(LF_CULL_WG, LF_CULL_WAVES) void k_cull_level_general(const LfLensDev* __restrict__ lens,
                                                    const LfPairsDev* __restrict__ pairs,
                                                    const int* __restrict__ seq_table,
                                                    const LfProgRow* __restrict__ rec_table, CullLevelArgs a,
                                                    const unsigned* __restrict__ items,
                                                    const unsigned* __restrict__ counts, unsigned items_stride,
                                                    unsigned* __restrict__ next, unsigned* __restrict__ next_counts,
                                                    unsigned long long* __restrict__ table,
                                                    unsigned long long* __restrict__ stats) {
  const int q = blockIdx.y;
  const unsigned PP = (unsigned)(a.P * a.P);
  // (first level: every box of the blocks this rank builds -- all of them unless the table is shared)
  const unsigned n_blk = (unsigned)(a.blocks_x * a.blocks_y);
  const unsigned n_mine = (n_blk + (unsigned)a.share_n - 1u - (unsigned)a.share_rank) / (unsigned)a.share_n;
  const unsigned n_items = items ? min(counts[q], items_stride) : n_mine * PP;
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  // (whole waves past the end leave; a partial last wave keeps its idle lanes: the loop below is wave-uniform)
  if ((i & ~63u) >= n_items) return;
  const bool valid = i < n_items;
  const unsigned item = valid ? (items ? items[(size_t)q * items_stride + i]
                                       : ((unsigned)a.share_rank + (unsigned)a.share_n * (i / PP)) * PP + i % PP) : 0u;
  const int blk = (int)(item / PP), cell = (int)(item % PP);
  const int ci = cell % a.P, cj = cell / a.P;
  const int bx = blk % a.blocks_x, by = blk / a.blocks_x;

  const float px0 = (float)(bx << a.blk_log2), px1 = fminf((float)a.W, (float)((bx + 1) << a.blk_log2));
  const float py0 = (float)(by << a.blk_log2), py1 = fminf((float)a.H, (float)((by + 1) << a.blk_log2));
  const float Xc = -((0.5f * (px0 + px1)) - a.half_w) * a.pitch, Yc = -((0.5f * (py0 + py1)) - a.half_h) * a.pitch;
  const float hX = 0.5f * (px1 - px0) * a.pitch, hY = 0.5f * (py1 - py0) * a.pitch;
  const float invP = 1.0f / (float)a.P;

  const int n_ev = pairs->ev_cnt[q];
  const int* const seq = seq_table + pairs->ev_off[q];
  const int lane = (int)(threadIdx.x & 63u);
  // ---- the box's 15 rays: 13 at the middle of the spectrum + the centre sample at its two ends ----------------
  // Dispersion moves the whole footprint, monotonically in the wavelength, between where the two ends of the spectrum
  // put it: the box must be ruled out for everything in between, so the centre sample is marched at both ends
  // as well and its largest deviation from the middle one widens every footprint.  (Testing the ends one after the
  // other and dropping the box when EACH misses is wrong -- the lobe may lie between them: 7042 of 1.3e10 lit rays
  // of the 8-wavelength 4K frame were lost that way, found by the full-enumeration comparison.)
  constexpr unsigned kAll = (1u << kCullSamples) - 1u;
  const LfProgRow* recs_of[3];
  int j_of[3];
  float ns_of[3];
#pragma unroll
  for (int w = 0; w < 3; w++) {
    const int l = a.lam[w], g = l / a.march_k;
    j_of[w] = l - g * a.march_k;
    recs_of[w] = rec_table + (size_t)g * (size_t)a.prog_recs;
    ns_of[w] = lens->n_start[l];
  }
  Ray r[kCullSamples];
#pragma unroll
  for (int t = 0; t < kCullSamples; t++) {
    float X = Xc, Y = Yc, fu = 0.5f, fv = 0.5f;
    if (t < 9) {
      fu = 0.5f * (float)(t % 3); fv = 0.5f * (float)(t / 3);
      // the four corners of the pupil cell sit on the four corners of the BLOCK as well (diagonals of the 4-D
      // box): what they deviate from the linear model by holds the cross terms between sensor and pupil
      if ((t % 3) != 1 && (t / 3) != 1) { X = Xc + (float)(t % 3 - 1) * hX; Y = Yc + (float)(t / 3 - 1) * hY; }
    }
    else if (t == 9) X = Xc + hX;
    else if (t == 10) X = Xc - hX;
    else if (t == 11) Y = Yc + hY;
    else if (t == 12) Y = Yc - hY;
    const float ns = t == 13 ? ns_of[1] : t == 14 ? ns_of[2] : ns_of[0];
    const float ua = ((float)ci + fu) * invP, ub = ((float)cj + fv) * invP;
    const StartRay s0 = aim_at_pupil(X, Y, fmaf(2.0f, ua, -1.0f), fmaf(2.0f, ub, -1.0f), a.pupil_h, a.vz, a.geom_norm);
    r[t] = Ray{X, Y, 0.0f, 0.0f, s0.dx * ns, s0.dy * ns, s0.dz * ns, 0.0f, 0.0f};
  }
  // `live`: bit t = sample t is still on the path (not lost to a missed sphere or to total reflection).  A box
  // that has lost samples is PARTIAL: what is left of it lies next to a region where the path ends -- total reflection or
  // the rim of a sphere, either way a square-root edge where the map is not Lipschitz -- and is not bounded by the samples
  // left: no footprint test drops it (strict = 1; the ball footprints below serve strict = 0 / 2, experiments).
  unsigned live = kAll;
  bool culled = !valid, keep = false, partial = false;
  bool tir_partial = false;     // some sample of the box ended by TOTAL REFLECTION: next to that boundary the refracted ray is grazing and
                                // the map unbounded -- what is left of the box cannot be bounded by the samples left (strict = 2)
  int why = 0;
  // Footprint of the box in a plane (an interface's, or direction space).  With every sample in use the
  // image of the box is modelled as a ZONOTOPE: centre c + the four generators g1, g2 (half the cell along the
  // two pupil axes: central differences of the mid-edge samples), gx, gy (half the block along x and y) + an
  // isotropic slack: what the linear model misses (largest deviation of the nine pupil samples and of the
  // edge mid-points from it) and how far the ends of the spectrum move the centre.  Its extent along a unit vector
  // n is sum |g . n|: a separating-axis test against a disc needs only that -- far tighter than a ball around c for
  // the elongated footprints of defocused ghosts.  A box that has lost samples falls back to a ball around a
  // sample still in use, inflated twice as much.
  struct Foot { float cx, cy, g1x, g1y, g2x, g2y, gxx, gxy, gyx, gyy, slack, ball; bool zono; };
  auto footprint = [&](bool dirs, unsigned use, float eps) {
    float vx[kCullSamples], vy[kCullSamples];
#pragma unroll
    for (int t = 0; t < kCullSamples; t++) { vx[t] = dirs ? r[t].dx : r[t].px; vy[t] = dirs ? r[t].dy : r[t].py; }
    Foot f;
    f.zono = use == kAll;
    const int ref = (use & 0x10u) ? 4 : (use ? __ffs((int)use) - 1 : 4);
    f.cx = vx[4]; f.cy = vy[4];
#pragma unroll
    for (int t = 0; t < kCullSamples; t++) if (t != 4 && ref == t) { f.cx = vx[t]; f.cy = vy[t]; }
    f.g1x = 0.5f * (vx[5] - vx[3]); f.g1y = 0.5f * (vy[5] - vy[3]);
    f.g2x = 0.5f * (vx[7] - vx[1]); f.g2y = 0.5f * (vy[7] - vy[1]);
    f.gxx = 0.5f * (vx[9] - vx[10]); f.gxy = 0.5f * (vy[9] - vy[10]);
    f.gyx = 0.5f * (vx[11] - vx[12]); f.gyy = 0.5f * (vy[11] - vy[12]);
    float dev2 = 0.0f, ru2 = 0.0f, rx2 = 0.0f, ry2 = 0.0f, rl2 = 0.0f;
#pragma unroll
    for (int t = 0; t < kCullSamples; t++) {
      const float ex = vx[t] - f.cx, ey = vy[t] - f.cy;
      const float d2 = ((use >> t) & 1u) ? fmaf(ex, ex, ey * ey) : 0.0f;
      if (t < 9) {
        ru2 = fmaxf(ru2, d2);
        const float at = (float)(t % 3 - 1), bt = (float)(t / 3 - 1);
        const bool corner = (t % 3) != 1 && (t / 3) != 1;     // (also displaced to the block's corner)
        const float mx = ex - fmaf(at, f.g1x, bt * f.g2x) - (corner ? fmaf(at, f.gxx, bt * f.gyx) : 0.0f);
        const float my = ey - fmaf(at, f.g1y, bt * f.g2y) - (corner ? fmaf(at, f.gxy, bt * f.gyy) : 0.0f);
        dev2 = fmaxf(dev2, fmaf(mx, mx, my * my));
      } else if (t < 11) rx2 = fmaxf(rx2, d2);
      else if (t < 13) ry2 = fmaxf(ry2, d2);
      else rl2 = fmaxf(rl2, d2);                               // the ends of the spectrum
    }
    {   // the edge mid-points against the centre: second order along x and y
      const float mx = 0.5f * (vx[9] + vx[10]) - vx[4], my = 0.5f * (vy[9] + vy[10]) - vy[4];
      const float nx = 0.5f * (vx[11] + vx[12]) - vx[4], ny = 0.5f * (vy[11] + vy[12]) - vy[4];
      dev2 = fmaxf(dev2, fmaxf(fmaf(mx, mx, my * my), fmaf(nx, nx, ny * ny)));
    }
    const float ru = lf_sqrt(ru2), rl = lf_sqrt(rl2);
    const float rx = (use & 0x600u) ? lf_sqrt(rx2) : ru, ry = (use & 0x1800u) ? lf_sqrt(ry2) : ru;
    f.ball = fmaf(partial ? 2.0f * a.margin : a.margin, ((ru + rx) + ry) + rl, eps);
    f.slack = fmaf(2.0f, lf_sqrt(dev2), fmaf(a.margin, rl, eps));
    if (a.slack_mode == 1) {
      // second order per axis (mid-points of opposite samples against the centre), SUMMED: at the extreme vertex of the
      // box all four add; and what the corners deviate by beyond that sum (cross terms), twice
      const float dax = 0.5f * (vx[5] + vx[3]) - vx[4], day = 0.5f * (vy[5] + vy[3]) - vy[4];
      const float dbx = 0.5f * (vx[7] + vx[1]) - vx[4], dby = 0.5f * (vy[7] + vy[1]) - vy[4];
      const float dxx = 0.5f * (vx[9] + vx[10]) - vx[4], dxy = 0.5f * (vy[9] + vy[10]) - vy[4];
      const float dyx = 0.5f * (vx[11] + vx[12]) - vx[4], dyy = 0.5f * (vy[11] + vy[12]) - vy[4];
      const float sx = (dax + dbx) + (dxx + dyx), sy = (day + dby) + (dxy + dyy);
      float c2 = 0.0f;
#pragma unroll
      for (int t = 0; t < 9; t += 2) {
        if (t == 4) continue;
        const float at = (float)(t % 3 - 1), bt = (float)(t / 3 - 1);
        const float mx = (vx[t] - vx[4]) - fmaf(at, f.g1x + f.gxx, bt * (f.g2x + f.gyx)) - sx;
        const float my = (vy[t] - vy[4]) - fmaf(at, f.g1y + f.gxy, bt * (f.g2y + f.gyy)) - sy;
        c2 = fmaxf(c2, fmaf(mx, mx, my * my));
      }
      const float sum2 = lf_sqrt(fmaf(dax, dax, day * day)) + lf_sqrt(fmaf(dbx, dbx, dby * dby)) +
                         lf_sqrt(fmaf(dxx, dxx, dxy * dxy)) + lf_sqrt(fmaf(dyx, dyx, dyy * dyy));
      f.slack = sum2 + fmaf(2.0f, lf_sqrt(c2), fmaf(a.margin, rl, eps));
    }
    return f;
  };
  // extent of the footprint along the unit vector (nx, ny), and along the axes (for the mask's grid)
  auto extent = [&](const Foot& f, float nx, float ny) {
    if (!f.zono) return f.ball;
    const float e = fabsf(fmaf(f.g1x, nx, f.g1y * ny)) + fabsf(fmaf(f.g2x, nx, f.g2y * ny)) +
                    fabsf(fmaf(f.gxx, nx, f.gxy * ny)) + fabsf(fmaf(f.gyx, nx, f.gyy * ny));
    return fminf(f.ball, fmaf(a.geo_margin, e, f.slack));
  };
  for (int e = 0; e < n_ev; e++) {
    if (__ballot(!culled && !keep) == 0ull) break;      // every box of the wave is decided
    const unsigned se = (unsigned)*(const int __attribute__((address_space(4)))*)(seq + e);
    const unsigned kind = se >> 16;
    // the interface once (its geometry is the same in every wavelength group), the index terms of the three wavelengths
    const LfProgRow wr = load_prec(recs_of[0], se & 0xffffu);
    float cn22_of[3], rn2_of[3], delta_of[3];
#pragma unroll
    for (int w = 0; w < 3; w++) {
      const LfProgRow x = w == 0 ? wr : load_prec(recs_of[w], se & 0xffffu);
      const int j = j_of[w];
      cn22_of[w] = j == 0 ? x.cn22[0] : j == 1 ? x.cn22[1] : x.cn22[2];
      rn2_of[w] = j == 0 ? x.rn2[0] : j == 1 ? x.rn2[1] : x.rn2[2];
      delta_of[w] = j == 0 ? x.delta[0] : j == 1 ? x.delta[1] : x.delta[2];
    }
    unsigned hit = 0u, okm = 0u;
    const unsigned live_before = live;
    // A ray goes on iff it meets the sphere (disc >= 0) and is not totally reflected ((n' cos t')^2 = disc + delta >= 0):
    // iff p = disc + min(0, delta) >= 0 -- ONE smooth scalar for both ways of ending (a mirror: p = disc)
    float pv[kCullSamples];
    // the total-reflection margins (virtual_event) of the samples that reach the interface: their range over the
    // box, and the one nearest to going on among those that end here by total reflection
    float t_max = -2.0f, t_min = 2.0f, t_lost = -2.0f;
#pragma unroll
    for (int t = 0; t < kCullSamples; t++) {
      const int w = t == 13 ? 1 : t == 14 ? 2 : 0;
      bool ok;
      if (kind & LF_EV_STOP) {
        const float tt = -(r[t].hz + wr.dzv) * lf_rcp(r[t].dz);
        const float hx = fmaf(tt, r[t].dx, r[t].px), hy = fmaf(tt, r[t].dy, r[t].py);
        r[t].px = hx; r[t].py = hy; r[t].hz = 0.0f;
        ok = hx == hx && hy == hy;
        if (ok) hit |= 1u << t;
        pv[t] = 1.0f;
      } else {
        float disc, tir;
        virtual_event(r[t], wr, cn22_of[w], rn2_of[w], delta_of[w], (kind & LF_EV_REFLECT) != 0, (kind & LF_EV_FLAT) != 0, disc, tir);
        pv[t] = (kind & LF_EV_REFLECT) ? disc : disc + fminf(0.0f, delta_of[w]);
        const bool reaches = disc >= 0.0f;
        if (reaches) hit |= 1u << t;                // (a totally reflected ray did reach the interface)
        ok = reaches && tir >= 0.0f;
        if (reaches && ((live >> t) & 1u)) {
          t_max = fmaxf(t_max, tir); t_min = fminf(t_min, tir);
          if (tir < 0.0f) { t_lost = fmaxf(t_lost, tir); tir_partial = true; }
        }
      }
      if (ok) okm |= 1u << t;
    }
    hit &= live;
    // "Every ray of the box ends here".  Round 5 first dropped such a box when even the sample nearest to going on was
    // further from it than half the range of the margins over the box (a rule fitted to the double Gauss: pair (3, 7),
    // profiles/r05_march_variants.txt) -- a draw of 6000 random frames with a second design family (a Cooke triplet,
    // steeper surfaces) found 14 frames where a sliver between the samples went on.  Now (strict_lost, the default):
    // the LARGEST value p can take over the box, bounded from its 15 samples like a footprint -- centre + the four
    // central-difference generators (x the footprints' inflation) + the second order of the four axes summed + twice
    // what the corners deviate by beyond that + how far the ends of the spectrum move the centre -- must stay below
    // zero; and only a box that had lost no sample before is bounded by its samples at all.
    bool firmly_lost = t_lost < -1.5f || t_lost < -(fmaf(a.lost_rel, t_max - t_min, a.lost_abs));
    if (a.strict_lost) {
      auto upper = [&](const float* v) {
        const float ga = 0.5f * (v[5] - v[3]), gb = 0.5f * (v[7] - v[1]), gx = 0.5f * (v[9] - v[10]), gy = 0.5f * (v[11] - v[12]);
        const float da = fabsf(0.5f * (v[5] + v[3]) - v[4]), db = fabsf(0.5f * (v[7] + v[1]) - v[4]);
        const float dx = fabsf(0.5f * (v[9] + v[10]) - v[4]), dy = fabsf(0.5f * (v[11] + v[12]) - v[4]);
        const float second = (da + db) + (dx + dy);
        float cross = 0.0f;
#pragma unroll
        for (int t = 0; t < 9; t += 2) {
          if (t == 4) continue;
          const float at = (float)(t % 3 - 1), bt = (float)(t / 3 - 1);
          cross = fmaxf(cross, fabsf((v[t] - v[4]) - fmaf(at, ga + gx, bt * (gb + gy))) - second);
        }
        const float disp = fmaxf(fabsf(v[13] - v[4]), fabsf(v[14] - v[4]));
        return v[4] + fmaf(a.geo_margin, (fabsf(ga) + fabsf(gb)) + (fabsf(gx) + fabsf(gy)), second + fmaf(2.0f, fmaxf(cross, 0.0f), a.margin * disp));
      };
      // (only a box whose samples all end at THIS event asks)
      firmly_lost = live_before == kAll && (okm & kAll) == 0u && !(kind & LF_EV_STOP) && upper(pv) < -1.0e-4f;
    }
    const Foot f = footprint(false, hit, 1e-3f);
    live &= okm;
    if (!culled && !keep) {
      if (hit == 0u) {                                       // no sample reaches the interface
        if (firmly_lost && !(a.disable & 8)) { culled = true; why = 7; } else { keep = true; why = 2; }
      }
      else {
        const float cx = f.cx, cy = f.cy;
        const float cr = lf_sqrt(fmaf(cx, cx, cy * cy));
        const float icr = cr > 0.0f ? lf_rcp(cr) : 0.0f;
        const bool bounded = a.strict == 0 || f.zono || (a.strict == 2 && !tir_partial);   // (STRICT: a box that lost samples is not bounded by the ones left)
        if (bounded && cr - extent(f, cx * icr, cy * icr) > lf_sqrt(wr.h2) && !(a.disable & 1)) { culled = true; why = 4; }   // wholly outside the clear aperture
        else if (bounded && (kind & LF_EV_STOP)) {
          // ... or on closed cells of the mask: texel coordinate = (h / stop_h + 1) / 2 of the mask's width
          const float s = 0.5f * (float)kCullOcc;
          const float radx = extent(f, 1.0f, 0.0f), rady = extent(f, 0.0f, 1.0f);
          const int ix0 = max(0, (int)floorf(fmaf(cx - radx, a.inv_stop_h, 1.0f) * s));
          const int ix1 = min(kCullOcc - 1, (int)floorf(fmaf(cx + radx, a.inv_stop_h, 1.0f) * s));
          const int iy0 = max(0, (int)floorf(fmaf(cy - rady, a.inv_stop_h, 1.0f) * s));
          const int iy1 = min(kCullOcc - 1, (int)floorf(fmaf(cy + rady, a.inv_stop_h, 1.0f) * s));
          bool open = false;
          if (ix0 <= ix1) {
            const unsigned span = (ix1 - ix0 >= 31 ? 0xffffffffu : ((2u << (ix1 - ix0)) - 1u)) << ix0;
            for (int iy = iy0; iy <= iy1; iy++) open = open || (a.occ[iy] & span) != 0u;
          }
          if (!open && !(a.disable & 2)) { culled = true; why = 5; }
        }
        if (!culled) {
          if (live == 0u && firmly_lost && !(a.disable & 8)) { culled = true; why = 7; }   // every sample ends here, by a margin
          else if (__popc(live & 0x1ffu) < 3) { keep = true; why = 2; }     // too little left to bound anything
          else if (live != kAll) partial = true;
        }
      }
    }
  }
  if (!culled && !keep) {
    // the path is complete: where can the box point?  (K is the unit direction in air again)
    const Foot f = footprint(true, live, 2e-5f);
    bool outside = true;     // ... of every light's lobe
    for (int k = 0; k < a.n_lights; k++) {
      const float ex = a.lsx[k] - f.cx, ey = a.lsy[k] - f.cy;
      const float dist = lf_sqrt(fmaf(ex, ex, ey * ey));
      const float id = dist > 0.0f ? lf_rcp(dist) : 0.0f;
      outside = outside && dist - a.lobe_k * extent(f, ex * id, ey * id) > a.lrho[k];
    }
    if (partial && (a.keep_partial || a.strict == 1 || (a.strict == 2 && tir_partial))) { keep = true; why = 1; }
    else if (outside && !(a.disable & 4)) { culled = true; why = 6; }
    else { keep = true; why = partial ? 1 : 3; }
  }
  if (stats && valid && why) atomicAdd(&stats[why], 1ull);
  // (measurements only, UNSAFE -- what the boxes nothing bounds cost the march: disable bit 4 drops the boxes kept with too few
  // samples left on the last level, bit 5 those kept because they had lost samples)
  if (a.last && (((a.disable & 16) && why == 2) || ((a.disable & 32) && why == 1))) keep = false;
  const bool enabled = valid && keep;
  if (a.last) {
    if (valid && enabled) {
      unsigned long long* row = table + lf_cull_row_of_block(blk, a.share_n, a.share_nb) * (size_t)(a.P * a.P + 1);
      const unsigned long long bit = 1ull << q;
      atomicOr(&row[cell], bit);
      atomicOr(&row[a.P * a.P], bit);
    }
    // how many (block, cell, path) combinations the march will start: one add per wave
    const lanemask em = __ballot(valid && enabled);
    if (em != 0ull && lane == (int)__builtin_ctzll(em)) atomicAdd(&next_counts[q], (unsigned)__popcll(em));
  } else {
    // the four children (cells of 2P) of every box kept, appended to the path's next list: one atomic per wave
    const lanemask em = __ballot(valid && enabled);
    if (em != 0ull) {
      unsigned base = 0u;
      if (lane == (int)__builtin_ctzll(em)) base = atomicAdd(&next_counts[q], 4u * (unsigned)__popcll(em));
      base = __shfl(base, (int)__builtin_ctzll(em));
      if (valid && enabled) {
        const unsigned at = base + 4u * (unsigned)__popcll(em & ((1ull << lane) - 1ull));
        const unsigned P2 = 2u * (unsigned)a.P;
        unsigned* out = next + (size_t)q * a.list_stride;
        if (at + 3u < a.list_stride) {
#pragma unroll
          for (int c = 0; c < 4; c++)
            out[at + c] = (unsigned)blk * (P2 * P2) + (unsigned)(2 * cj + (c >> 1)) * P2 + (unsigned)(2 * ci + (c & 1));
        }
      }
    }
  }
}

// ---- the pre-pass as it ships ---------------------------------------------------------------------------
// k_cull_level_general above evaluates whatever rules its arguments carry (a test's: lf_test_knob); the rules that SHIP
// are one set, and most of what the general kernel computes they never look at.  Under them
//   * a footprint is only ever taken over ALL 15 samples: a box that lost a sample is bounded by nothing (it is kept, or
//     dropped by the pass-scalar bound of the event at which all its samples end), so there is no ball around the samples
//     left, no reference sample other than the centre, no use-masks;
//   * on a glass interface the footprint can drop a box only if the centre sample already lies outside the clear
//     aperture (the test is  |c| - extent > h,  extent >= 0) -- a footprint is built only for the waves in which some
//     lane's centre does (round 5 built one after every event of every box: 233 lane-instructions per marched
//     ray-event against the march's 40); at the stop the mask's grid needs it for every box that got there whole;
//   * the total-reflection margin is only a sign: no reciprocal.
// Same expressions in the same order (the build is -ffp-contract=off): the table is the general kernel's BIT FOR BIT
// (tests/test_gpu_cull.py test_the_shipped_kernel_is_the_general_one).
__device__ __forceinline__ void cull_event(Ray& r, const LfProgRow& w, float cn22, float rn2, float delta, bool reflect, bool flat,
                                           float& disc_out, bool& goes_on) {
  const float oz = r.hz + w.dzv;
  const float od = fmaf(r.px, r.dx, fmaf(r.py, r.dy, oz * r.dz));
  const float oo = fmaf(oz, oz, fmaf(r.px, r.px, r.py * r.py));
  const float Fh = fmaf(w.ch, oo, -oz);
  const float G = fmaf(-w.curv, od, r.dz);
  const float disc = fmaf(G, G, -(cn22 * Fh));
  disc_out = disc;
  const float sq = lf_sqrt(disc);
  const float t = flat ? (Fh + Fh) * lf_rcp(fmaf(w.sgn, sq, G)) : fmaf(-w.sgn, sq, G) * rn2;
  const float hx = fmaf(t, r.dx, r.px), hy = fmaf(t, r.dy, r.py), hz = fmaf(t, r.dz, oz);
  if (reflect) {
    goes_on = true;
    const float m = sq * (w.c2 * w.sgn);
    r.dx = fmaf(m, hx, r.dx); r.dy = fmaf(m, hy, r.dy); r.dz = fmaf(m, hz, fmaf(-2.0f * w.sgn, sq, r.dz));
  } else {
    const float k2 = disc + delta;
    goes_on = k2 >= 0.0f;
    const float gs = lf_sqrt(k2) - sq, gcs = gs * w.sc;
    r.dx = fmaf(-gcs, hx, r.dx); r.dy = fmaf(-gcs, hy, r.dy); r.dz = fmaf(-gcs, hz, fmaf(w.sgn, gs, r.dz));
  }
  r.px = hx; r.py = hy; r.hz = hz;
}

// the shipped rules' constants (lf_ctx::CullRules' defaults: what k_cull_level_general is given when no test interferes)
constexpr float kShipLobeK = 1.2f;

// the footprint of a box whose 15 samples are all in use, in a plane (positions on an interface / directions at the exit):
// centre, generators, the slack that sums the second order of the four axes + twice the corners' cross terms, and the ball
struct ShipFoot { float cx, cy, g1x, g1y, g2x, g2y, gxx, gxy, gyx, gyy, slack, ball; };
template <bool DIRS>
__device__ __forceinline__ ShipFoot ship_footprint(const Ray (&r)[kCullSamples], float margin, float eps) {
  auto vx = [&](int t) { return DIRS ? r[t].dx : r[t].px; };
  auto vy = [&](int t) { return DIRS ? r[t].dy : r[t].py; };
  ShipFoot f;
  f.cx = vx(4); f.cy = vy(4);
  f.g1x = 0.5f * (vx(5) - vx(3)); f.g1y = 0.5f * (vy(5) - vy(3));
  f.g2x = 0.5f * (vx(7) - vx(1)); f.g2y = 0.5f * (vy(7) - vy(1));
  f.gxx = 0.5f * (vx(9) - vx(10)); f.gxy = 0.5f * (vy(9) - vy(10));
  f.gyx = 0.5f * (vx(11) - vx(12)); f.gyy = 0.5f * (vy(11) - vy(12));
  float ru2 = 0.0f, rx2 = 0.0f, ry2 = 0.0f, rl2 = 0.0f;
#pragma unroll
  for (int t = 0; t < kCullSamples; t++) {
    const float ex = vx(t) - f.cx, ey = vy(t) - f.cy;
    const float d2 = fmaf(ex, ex, ey * ey);
    if (t < 9) ru2 = fmaxf(ru2, d2);
    else if (t < 11) rx2 = fmaxf(rx2, d2);
    else if (t < 13) ry2 = fmaxf(ry2, d2);
    else rl2 = fmaxf(rl2, d2);
  }
  const float ru = lf_sqrt(ru2), rl = lf_sqrt(rl2);
  const float rx = lf_sqrt(rx2), ry = lf_sqrt(ry2);
  f.ball = fmaf(margin, ((ru + rx) + ry) + rl, eps);
  const float dax = 0.5f * (vx(5) + vx(3)) - vx(4), day = 0.5f * (vy(5) + vy(3)) - vy(4);
  const float dbx = 0.5f * (vx(7) + vx(1)) - vx(4), dby = 0.5f * (vy(7) + vy(1)) - vy(4);
  const float dxx = 0.5f * (vx(9) + vx(10)) - vx(4), dxy = 0.5f * (vy(9) + vy(10)) - vy(4);
  const float dyx = 0.5f * (vx(11) + vx(12)) - vx(4), dyy = 0.5f * (vy(11) + vy(12)) - vy(4);
  const float sx = (dax + dbx) + (dxx + dyx), sy = (day + dby) + (dxy + dyy);
  float c2 = 0.0f;
#pragma unroll
  for (int t = 0; t < 9; t += 2) {
    if (t == 4) continue;
    const float at = (float)(t % 3 - 1), bt = (float)(t / 3 - 1);
    const float mx = (vx(t) - vx(4)) - fmaf(at, f.g1x + f.gxx, bt * (f.g2x + f.gyx)) - sx;
    const float my = (vy(t) - vy(4)) - fmaf(at, f.g1y + f.gxy, bt * (f.g2y + f.gyy)) - sy;
    c2 = fmaxf(c2, fmaf(mx, mx, my * my));
  }
  const float sum2 = lf_sqrt(fmaf(dax, dax, day * day)) + lf_sqrt(fmaf(dbx, dbx, dby * dby)) +
                     lf_sqrt(fmaf(dxx, dxx, dxy * dxy)) + lf_sqrt(fmaf(dyx, dyx, dyy * dyy));
  f.slack = sum2 + fmaf(2.0f, lf_sqrt(c2), fmaf(margin, rl, eps));
  return f;
}
__device__ __forceinline__ float ship_extent(const ShipFoot& f, float geo_margin, float nx, float ny) {
  const float e = fabsf(fmaf(f.g1x, nx, f.g1y * ny)) + fabsf(fmaf(f.g2x, nx, f.g2y * ny)) +
                  fabsf(fmaf(f.gxx, nx, f.gxy * ny)) + fabsf(fmaf(f.gyx, nx, f.gyy * ny));
  return fminf(f.ball, fmaf(geo_margin, e, f.slack));
}
// the last test of a box that got through whole, the ONLY place the sun enters the pre-pass: its exit footprint (in direction
// space) lies wholly outside the lobe.  One function for the pre-pass (footprint in registers) and the per-frame resolve of the
// cached footprints (k_cull_resolve: the same twelve floats from memory), so that both decide every box alike, bit for bit.
__device__ __forceinline__ bool ship_lobe_culls(const ShipFoot& f, float geo_margin, float sx, float sy, float rho) {
  const float ex = sx - f.cx, ey = sy - f.cy;
  const float dist = lf_sqrt(fmaf(ex, ex, ey * ey));
  const float id = dist > 0.0f ? lf_rcp(dist) : 0.0f;
  return dist - kShipLobeK * ship_extent(f, geo_margin, ex * id, ey * id) > rho;
}

// several lights: the lights (bits of `live`) whose lobe the footprint can still reach
// (A: the kernel's arguments, CullLevelArgs / CullResolveArgs -- n_lights, lsx, lsy, lrho; k is uniform, the reads scalar)
template <class A>
__device__ __forceinline__ unsigned ship_lobes_reached(const ShipFoot& f, float geo_margin, unsigned live, const A& a) {
  for (int k = 0; k < a.n_lights; k++)
    if (((live >> k) & 1u) != 0u && ship_lobe_culls(f, geo_margin, a.lsx[k], a.lsy[k], a.lrho[k])) live &= ~(1u << k);
  return live;
}

// ---- the sun-independent part of the pre-pass, cached (lfk_cull_prepass) ------------------------------------------
// Everything a box's fate depends on before the lobe test -- the lens, the frame, the blocks, the mask's grid, the pairs, the
// rank's share -- stays the same while the sun moves.  The cache holds, per level and (path, own block, cell), one slot:
// kSlotCulled / kSlotKept where the kernel decides the box before the lobe test, kSlotFoot + i where it reaches it (i: the
// box's exit footprint, 12 floats, in the level's compacted array).  Children exist for every box that is not culled.
constexpr unsigned kSlotCulled = 0u, kSlotKept = 1u, kSlotFoot = 2u;
constexpr int kCullMaxLevels = 8;
struct CullCacheOut {
  unsigned* slots;         // this level's [path][own block][cell]
  float4* foots;           // this level's footprints, 3 x float4 each
  unsigned* foot_count;    // ... how many were appended
  unsigned foot_cap;
  unsigned n_mine;         // blocks this rank builds
};

// BUILD = false: the pre-pass as it ships (k_cull_level).  BUILD = true (k_cull_level_build): the same rules up to the lobe
// test, which is replaced by "emit the box's slot and footprint"; children of kept AND undecided boxes are listed.
// LIGHTS: the lobe test runs over the lights of CullLevelArgs (several: k_cull_level_lights) instead of the one sun
template <bool BUILD, bool LIGHTS = false>
__device__ __forceinline__ void cull_level_body(const LfLensDev* __restrict__ lens,
                                                    const LfPairsDev* __restrict__ pairs,
                                                    const int* __restrict__ seq_table,
                                                    const LfProgRow* __restrict__ rec_table, const CullLevelArgs& a,
                                                    const unsigned* __restrict__ items,
                                                    const unsigned* __restrict__ counts, unsigned items_stride,
                                                    unsigned* __restrict__ next, unsigned* __restrict__ next_counts,
                                                    unsigned long long* __restrict__ table,
                                                    unsigned long long* __restrict__ stats, const CullCacheOut& co) {
  const int q = blockIdx.y;
  const unsigned PP = (unsigned)(a.P * a.P);
  const unsigned n_blk = (unsigned)(a.blocks_x * a.blocks_y);
  const unsigned n_mine = (n_blk + (unsigned)a.share_n - 1u - (unsigned)a.share_rank) / (unsigned)a.share_n;
  const unsigned n_items = items ? min(counts[q], items_stride) : n_mine * PP;
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if ((i & ~63u) >= n_items) return;
  const bool valid = i < n_items;
  const unsigned item = valid ? (items ? items[(size_t)q * items_stride + i]
                                       : ((unsigned)a.share_rank + (unsigned)a.share_n * (i / PP)) * PP + i % PP) : 0u;
  const int blk = (int)(item / PP), cell = (int)(item % PP);
  const int ci = cell % a.P, cj = cell / a.P;
  const int bx = blk % a.blocks_x, by = blk / a.blocks_x;

  const float px0 = (float)(bx << a.blk_log2), px1 = fminf((float)a.W, (float)((bx + 1) << a.blk_log2));
  const float py0 = (float)(by << a.blk_log2), py1 = fminf((float)a.H, (float)((by + 1) << a.blk_log2));
  const float Xc = -((0.5f * (px0 + px1)) - a.half_w) * a.pitch, Yc = -((0.5f * (py0 + py1)) - a.half_h) * a.pitch;
  const float hX = 0.5f * (px1 - px0) * a.pitch, hY = 0.5f * (py1 - py0) * a.pitch;
  const float invP = 1.0f / (float)a.P;

  const int n_ev = pairs->ev_cnt[q];
  const int* const seq = seq_table + pairs->ev_off[q];
  const int lane = (int)(threadIdx.x & 63u);
  constexpr unsigned kAll = (1u << kCullSamples) - 1u;
  const LfProgRow* recs_of[3];
  int j_of[3];
  float ns_of[3];
#pragma unroll
  for (int w = 0; w < 3; w++) {
    const int l = a.lam[w], g = l / a.march_k;
    j_of[w] = l - g * a.march_k;
    recs_of[w] = rec_table + (size_t)g * (size_t)a.prog_recs;
    ns_of[w] = lens->n_start[l];
  }
  // the box's 15 rays (the sample layout of k_cull_level_general)
  Ray r[kCullSamples];
#pragma unroll
  for (int t = 0; t < kCullSamples; t++) {
    float X = Xc, Y = Yc, fu = 0.5f, fv = 0.5f;
    if (t < 9) {
      fu = 0.5f * (float)(t % 3); fv = 0.5f * (float)(t / 3);
      if ((t % 3) != 1 && (t / 3) != 1) { X = Xc + (float)(t % 3 - 1) * hX; Y = Yc + (float)(t / 3 - 1) * hY; }
    }
    else if (t == 9) X = Xc + hX;
    else if (t == 10) X = Xc - hX;
    else if (t == 11) Y = Yc + hY;
    else if (t == 12) Y = Yc - hY;
    const float ns = t == 13 ? ns_of[1] : t == 14 ? ns_of[2] : ns_of[0];
    const float ua = ((float)ci + fu) * invP, ub = ((float)cj + fv) * invP;
    const StartRay s0 = aim_at_pupil(X, Y, fmaf(2.0f, ua, -1.0f), fmaf(2.0f, ub, -1.0f), a.pupil_h, a.vz, a.geom_norm);
    r[t] = Ray{X, Y, 0.0f, 0.0f, s0.dx * ns, s0.dy * ns, s0.dz * ns, 0.0f, 0.0f};
  }
  unsigned live = kAll;
  bool culled = !valid, keep = false;
  int why = 0;
  for (int e = 0; e < n_ev; e++) {
    if (__ballot(!culled && !keep) == 0ull) break;      // every box of the wave is decided
    const unsigned se = (unsigned)*(const int __attribute__((address_space(4)))*)(seq + e);
    const unsigned kind = se >> 16;
    const LfProgRow wr = load_prec(recs_of[0], se & 0xffffu);
    float cn22_of[3], rn2_of[3], delta_of[3];
#pragma unroll
    for (int w = 0; w < 3; w++) {
      const LfProgRow x = w == 0 ? wr : load_prec(recs_of[w], se & 0xffffu);
      const int j = j_of[w];
      cn22_of[w] = j == 0 ? x.cn22[0] : j == 1 ? x.cn22[1] : x.cn22[2];
      rn2_of[w] = j == 0 ? x.rn2[0] : j == 1 ? x.rn2[1] : x.rn2[2];
      delta_of[w] = j == 0 ? x.delta[0] : j == 1 ? x.delta[1] : x.delta[2];
    }
    const bool stop = (kind & LF_EV_STOP) != 0u;
    unsigned hit = 0u, okm = 0u;
    const unsigned live_before = live;
    float pv[kCullSamples];      // the pass scalar of every sample: p = disc + min(0, n'^2 - n^2) (see k_cull_level_general)
#pragma unroll
    for (int t = 0; t < kCullSamples; t++) {
      const int w = t == 13 ? 1 : t == 14 ? 2 : 0;
      bool ok;
      if (stop) {
        const float tt = -(r[t].hz + wr.dzv) * lf_rcp(r[t].dz);
        const float hx = fmaf(tt, r[t].dx, r[t].px), hy = fmaf(tt, r[t].dy, r[t].py);
        r[t].px = hx; r[t].py = hy; r[t].hz = 0.0f;
        ok = hx == hx && hy == hy;
        if (ok) hit |= 1u << t;
        pv[t] = 1.0f;
      } else {
        float disc;
        bool goes_on;
        cull_event(r[t], wr, cn22_of[w], rn2_of[w], delta_of[w], (kind & LF_EV_REFLECT) != 0, (kind & LF_EV_FLAT) != 0, disc, goes_on);
        pv[t] = (kind & LF_EV_REFLECT) ? disc : disc + fminf(0.0f, delta_of[w]);
        const bool reaches = disc >= 0.0f;
        if (reaches) hit |= 1u << t;
        ok = reaches && goes_on;
      }
      if (ok) okm |= 1u << t;
    }
    hit &= live;
    const bool undecided = !culled && !keep;
    // "every ray of the box ends here": the zonotope bound of the pass scalar must stay below zero, on a box whole until now
    const bool all_end = undecided && live_before == kAll && (okm & kAll) == 0u && !stop;
    bool firmly_lost = false;
    if (__ballot(all_end) != 0ull) {
      const float* v = pv;
      const float ga = 0.5f * (v[5] - v[3]), gb = 0.5f * (v[7] - v[1]), gx = 0.5f * (v[9] - v[10]), gy = 0.5f * (v[11] - v[12]);
      const float da = fabsf(0.5f * (v[5] + v[3]) - v[4]), db = fabsf(0.5f * (v[7] + v[1]) - v[4]);
      const float dx = fabsf(0.5f * (v[9] + v[10]) - v[4]), dy = fabsf(0.5f * (v[11] + v[12]) - v[4]);
      const float second = (da + db) + (dx + dy);
      float cross = 0.0f;
#pragma unroll
      for (int t = 0; t < 9; t += 2) {
        if (t == 4) continue;
        const float at = (float)(t % 3 - 1), bt = (float)(t / 3 - 1);
        cross = fmaxf(cross, fabsf((v[t] - v[4]) - fmaf(at, ga + gx, bt * (gb + gy))) - second);
      }
      const float disp = fmaxf(fabsf(v[13] - v[4]), fabsf(v[14] - v[4]));
      const float upper = v[4] + fmaf(a.geo_margin, (fabsf(ga) + fabsf(gb)) + (fabsf(gx) + fabsf(gy)), second + fmaf(2.0f, fmaxf(cross, 0.0f), a.margin * disp));
      firmly_lost = all_end && upper < -1.0e-4f;
    }
    live &= okm;
    // a footprint can drop a box only where every sample reached the interface AND (the stop's mask, or the centre sample
    // outside the clear aperture)
    const float cx = r[4].px, cy = r[4].py;
    const float cr = lf_sqrt(fmaf(cx, cx, cy * cy));
    const float h = lf_sqrt(wr.h2);
    const bool whole = undecided && hit == kAll;
    if (__ballot(whole && (stop || cr > h)) != 0ull) {
      const ShipFoot f = ship_footprint<false>(r, a.margin, 1e-3f);
      const float icr = cr > 0.0f ? lf_rcp(cr) : 0.0f;
      if (whole && cr - ship_extent(f, a.geo_margin, cx * icr, cy * icr) > h) { culled = true; why = 4; }
      else if (whole && stop) {
        const float s = 0.5f * (float)kCullOcc;
        const float radx = ship_extent(f, a.geo_margin, 1.0f, 0.0f), rady = ship_extent(f, a.geo_margin, 0.0f, 1.0f);
        const int ix0 = max(0, (int)floorf(fmaf(cx - radx, a.inv_stop_h, 1.0f) * s));
        const int ix1 = min(kCullOcc - 1, (int)floorf(fmaf(cx + radx, a.inv_stop_h, 1.0f) * s));
        const int iy0 = max(0, (int)floorf(fmaf(cy - rady, a.inv_stop_h, 1.0f) * s));
        const int iy1 = min(kCullOcc - 1, (int)floorf(fmaf(cy + rady, a.inv_stop_h, 1.0f) * s));
        bool open = false;
        if (ix0 <= ix1) {
          const unsigned span = (ix1 - ix0 >= 31 ? 0xffffffffu : ((2u << (ix1 - ix0)) - 1u)) << ix0;
          for (int iy = iy0; iy <= iy1; iy++) open = open || (a.occ[iy] & span) != 0u;
        }
        if (!open) { culled = true; why = 5; }
      }
    }
    if (undecided && !culled) {
      if (hit == 0u) {                                       // no sample reaches the interface
        if (firmly_lost) { culled = true; why = 7; } else { keep = true; why = 2; }
      }
      else if (live == 0u && firmly_lost) { culled = true; why = 7; }   // every sample ends here, by a margin
      else if (__popc(live & 0x1ffu) < 3) { keep = true; why = 2; }     // too little left to bound anything
    }
  }
  if (!culled && !keep) {
    // the path is complete.  A box that lost samples is bounded by nothing: kept.  A whole one: where can it point?
    if (live != kAll) { keep = true; why = 1; }
  }
  if constexpr (BUILD) {
    // (lanes that are not valid are `culled`)
    const bool foot = !culled && !keep;
    const lanemask fm = __ballot(foot);
    unsigned slot = kSlotKept;
    if (fm != 0ull) {
      const ShipFoot f = ship_footprint<true>(r, a.margin, 2e-5f);
      unsigned base = 0u;
      if (lane == (int)__builtin_ctzll(fm)) base = atomicAdd(co.foot_count, (unsigned)__popcll(fm));
      base = __shfl(base, (int)__builtin_ctzll(fm));
      const unsigned at = base + (unsigned)__popcll(fm & ((1ull << lane) - 1ull));
      if (foot && at < co.foot_cap) {
        float4* const o = co.foots + (size_t)at * 3;
        o[0] = make_float4(f.cx, f.cy, f.g1x, f.g1y);
        o[1] = make_float4(f.g2x, f.g2y, f.gxx, f.gxy);
        o[2] = make_float4(f.gyx, f.gyy, f.slack, f.ball);
        slot = kSlotFoot + at;
      }
    }
    // (the slots start as kSlotCulled; a rank's blocks are rank, rank + n, ...: own index blk / n)
    if (!culled) co.slots[((size_t)q * co.n_mine + (size_t)(blk / a.share_n)) * PP + (unsigned)cell] = slot;
    keep = !culled;
  } else {
    if (__ballot(!culled && !keep) != 0ull) {
      const ShipFoot f = ship_footprint<true>(r, a.margin, 2e-5f);
      if (!culled && !keep) {
        const bool out = LIGHTS ? ship_lobes_reached(f, a.geo_margin, (1u << a.n_lights) - 1u, a) == 0u
                                : ship_lobe_culls(f, a.geo_margin, a.sx, a.sy, a.rho);
        if (out) { culled = true; why = 6; }
        else { keep = true; why = 3; }
      }
    }
    if (stats && valid && why) atomicAdd(&stats[why], 1ull);
  }
  const bool enabled = valid && keep;
  if (BUILD && a.last) return;
  if (a.last) {
    if (valid && enabled) {
      unsigned long long* row = table + lf_cull_row_of_block(blk, a.share_n, a.share_nb) * (size_t)(a.P * a.P + 1);
      const unsigned long long bit = 1ull << q;
      atomicOr(&row[cell], bit);
    }
    const lanemask em = __ballot(valid && enabled);
    // the row's summary word (its last): one atomic per wave and block, not per box (the lanes of a wave are boxes of ONE path)
    for (lanemask todo = em; todo != 0ull;) {
      const int first = (int)__builtin_ctzll(todo);
      const int b0 = __shfl(blk, first);
      if (lane == first) atomicOr(&table[lf_cull_row_of_block(b0, a.share_n, a.share_nb) * (size_t)(a.P * a.P + 1) + (size_t)(a.P * a.P)], 1ull << q);
      todo &= ~__ballot(blk == b0);
    }
    if (em != 0ull && lane == (int)__builtin_ctzll(em)) atomicAdd(&next_counts[q], (unsigned)__popcll(em));
  } else {
    const lanemask em = __ballot(valid && enabled);
    if (em != 0ull) {
      unsigned base = 0u;
      if (lane == (int)__builtin_ctzll(em)) base = atomicAdd(&next_counts[q], 4u * (unsigned)__popcll(em));
      base = __shfl(base, (int)__builtin_ctzll(em));
      if (valid && enabled) {
        const unsigned at = base + 4u * (unsigned)__popcll(em & ((1ull << lane) - 1ull));
        const unsigned P2 = 2u * (unsigned)a.P;
        unsigned* out = next + (size_t)q * a.list_stride;
        if (at + 3u < a.list_stride) {
#pragma unroll
          for (int c = 0; c < 4; c++)
            out[at + c] = (unsigned)blk * (P2 * P2) + (unsigned)(2 * cj + (c >> 1)) * P2 + (unsigned)(2 * ci + (c & 1));
        }
      }
    }
  }
}

__global__ __launch_bounds__(LF_CULL_WG, LF_CULL_WAVES) void k_cull_level(const LfLensDev* __restrict__ lens,
                                                    const LfPairsDev* __restrict__ pairs,
                                                    const int* __restrict__ seq_table,
                                                    const LfProgRow* __restrict__ rec_table, CullLevelArgs a,
                                                    const unsigned* __restrict__ items,
                                                    const unsigned* __restrict__ counts, unsigned items_stride,
                                                    unsigned* __restrict__ next, unsigned* __restrict__ next_counts,
                                                    unsigned long long* __restrict__ table,
                                                    unsigned long long* __restrict__ stats) {
  cull_level_body<false>(lens, pairs, seq_table, rec_table, a, items, counts, items_stride, next, next_counts, table, stats, CullCacheOut{});
}
__global__ __launch_bounds__(LF_CULL_WG, LF_CULL_WAVES) void k_cull_level_lights(const LfLensDev* __restrict__ lens,
                                                    const LfPairsDev* __restrict__ pairs,
                                                    const int* __restrict__ seq_table,
                                                    const LfProgRow* __restrict__ rec_table, CullLevelArgs a,
                                                    const unsigned* __restrict__ items,
                                                    const unsigned* __restrict__ counts, unsigned items_stride,
                                                    unsigned* __restrict__ next, unsigned* __restrict__ next_counts,
                                                    unsigned long long* __restrict__ table,
                                                    unsigned long long* __restrict__ stats) {
  cull_level_body<false, true>(lens, pairs, seq_table, rec_table, a, items, counts, items_stride, next, next_counts, table, stats, CullCacheOut{});
}
__global__ __launch_bounds__(LF_CULL_WG, LF_CULL_WAVES) void k_cull_level_build(const LfLensDev* __restrict__ lens,
                                                    const LfPairsDev* __restrict__ pairs,
                                                    const int* __restrict__ seq_table,
                                                    const LfProgRow* __restrict__ rec_table, CullLevelArgs a,
                                                    const unsigned* __restrict__ items,
                                                    const unsigned* __restrict__ counts, unsigned items_stride,
                                                    unsigned* __restrict__ next, unsigned* __restrict__ next_counts,
                                                    CullCacheOut co) {
  cull_level_body<true>(lens, pairs, seq_table, rec_table, a, items, counts, items_stride, next, next_counts, nullptr, nullptr, co);
}

// The per-frame resolve of a cached tree: one thread = one finest cell of one own block, a wave = an 8 x 8 patch of them (its
// lanes share their ancestors: the coarse levels' reads are broadcasts).  Per path, from the coarsest level down: a culled
// ancestor ends the walk, a kept one goes down, an undecided one takes the pre-pass's lobe test on its stored footprint.
// What survives to the finest level sets the path's bit: one plain store per cell, the row's summary word by one atomic
// per wave.  No lists, no per-box atomics, nothing for the host to read.
struct CullResolveArgs {
  int P_final, n_levels, n_paths, patches;     // patches of 8 x 8 cells per axis of a block
  int share_rank, share_n, share_nb;
  unsigned n_mine, n_waves;
  float sx, sy, rho, geo_margin;
  const unsigned* slots[kCullMaxLevels];
  const float4* foots[kCullMaxLevels];
  int n_lights;                                // several lights (LIGHTS): as CullLevelArgs'
  float lsx[LF_MAX_LIGHTS], lsy[LF_MAX_LIGHTS], lrho[LF_MAX_LIGHTS];
};
// LIGHTS: per lane a mask of the lights still alive instead of `alive`: an undecided ancestor clears the lights whose lobe
// its footprint cannot reach, the path's bit is set if any light survives to the finest level -- light k's bit survives exactly
// where the single-light walk for light k survives, so the table is the bitwise OR of the lights' single-light tables
template <bool LIGHTS>
__global__ __launch_bounds__(256) void k_cull_resolve(CullResolveArgs a, unsigned long long* __restrict__ table) {
  const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (wave >= a.n_waves) return;
  const int lane = (int)(threadIdx.x & 63u);
  const unsigned pp = (unsigned)(a.patches * a.patches);
  const unsigned own = wave / pp, patch = wave % pp;
  const int ci = (int)(patch % (unsigned)a.patches) * 8 + (lane & 7), cj = (int)(patch / (unsigned)a.patches) * 8 + (lane >> 3);
  const bool valid = ci < a.P_final && cj < a.P_final;
  const int blk = a.share_rank + a.share_n * (int)own;
  unsigned long long bits = 0ull;
  for (int q = 0; LIGHTS && q < a.n_paths; q++) {
    unsigned live = valid ? (1u << a.n_lights) - 1u : 0u;
    for (int lv = 0; lv < a.n_levels; lv++) {
      if (__ballot(live != 0u) == 0ull) break;
      const int sh = a.n_levels - 1 - lv;
      const int Pl = a.P_final >> sh;
      if (live != 0u) {
        const unsigned s = a.slots[lv][((size_t)q * a.n_mine + own) * (size_t)(Pl * Pl) + (size_t)((cj >> sh) * Pl + (ci >> sh))];
        if (s == kSlotCulled) live = 0u;
        else if (s >= kSlotFoot) {
          const float4* const p = a.foots[lv] + (size_t)(s - kSlotFoot) * 3;
          const float4 v0 = p[0], v1 = p[1], v2 = p[2];
          const ShipFoot f{v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
          live = ship_lobes_reached(f, a.geo_margin, live, a);
        }
      }
    }
    if (live != 0u) bits |= 1ull << q;
  }
  for (int q = 0; !LIGHTS && q < a.n_paths; q++) {
    bool alive = valid;
    for (int lv = 0; lv < a.n_levels; lv++) {
      if (__ballot(alive) == 0ull) break;
      const int sh = a.n_levels - 1 - lv;
      const int Pl = a.P_final >> sh;
      if (alive) {
        const unsigned s = a.slots[lv][((size_t)q * a.n_mine + own) * (size_t)(Pl * Pl) + (size_t)((cj >> sh) * Pl + (ci >> sh))];
        if (s == kSlotCulled) alive = false;
        else if (s >= kSlotFoot) {
          const float4* const p = a.foots[lv] + (size_t)(s - kSlotFoot) * 3;
          const float4 v0 = p[0], v1 = p[1], v2 = p[2];
          const ShipFoot f{v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
          if (ship_lobe_culls(f, a.geo_margin, a.sx, a.sy, a.rho)) alive = false;
        }
      }
    }
    if (alive) bits |= 1ull << q;
  }
  unsigned long long* const row = table + lf_cull_row_of_block(blk, a.share_n, a.share_nb) * (size_t)(a.P_final * a.P_final + 1);
  if (valid) row[cj * a.P_final + ci] = bits;
  unsigned long long any = bits;
  for (int o = 32; o > 0; o >>= 1) any |= __shfl_xor(any, o);
  if (lane == 0 && any != 0ull) atomicOr(&row[a.P_final * a.P_final], any);
}

uint64_t fnv(uint64_t h, const void* data, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(data);
  for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
  return h;
}

}  // namespace

// table cells per axis inside one stratum: 4, in a table of at most 128 cells per axis.  Where a wave's lanes share
// one sub-cell of the stratum (2^sub_bits >= m sub-cells per axis) the wave looks its cell up ONCE; otherwise
// (independent pixels, unstratified samples) every lane looks up the cell of its own pupil point.
static int cull_m(const lf_ctx* ctx, int G) {
  (void)ctx;
  int m = 4;
#ifdef LF_EXPERIMENTS
  if (const char* e = std::getenv("LF_CULL_M")) m = std::max(1, std::atoi(e));
#endif
  while (m > 1 && G * m > 128) m >>= 1;
  return m;
}

// Does the cull apply to this launch, and if not, why (lf_get_cull_reason)
int lf_cull_reason_of(const lf_ctx* ctx, int G) {
  // (the pre-pass's bounds are empirical rules found on spherical designs: DESIGN.md section 5)
  if (lf_march_posed(ctx)) return LF_CULL_POSED;   // (nor on a centred lens alone)
  if (lf_march_biconic(ctx)) return LF_CULL_ANAMORPHIC;   // (nor on surfaces of revolution alone)
  if (lf_march_aspheric(ctx)) return LF_CULL_ASPHERIC;
  if (ctx->march_cull == 0) return LF_CULL_OFF;
#ifdef LF_EXPERIMENTS
  if (const char* e = std::getenv("LF_MARCH_CULL")) if (std::atoi(e) == 0) return LF_CULL_OFF;
#endif
  if (ctx->lens.stop < 0) return LF_CULL_NO_STOP;
  if (!ctx->lens_lambda_monotonic) return LF_CULL_DISPERSION;
  // (a mask has 64 bits; up to 128 paths go in two launches over the halves of the selection: lfk_march -- with a table
  // of this context's own)
  if (ctx->pairs.n > 2 * kCullMaxPaths || (ctx->pairs.n > kCullMaxPaths && lf_cull_table_split(ctx))) return LF_CULL_TOO_MANY_PATHS;
  if (G < 1 || G > 64) return LF_CULL_TOO_MANY_SAMPLES;
  // a block must be SMALL on the sensor for 15 rays to bound it: <= 1.8 mm (the full-enumeration comparison finds no
  // skipped lit ray up to 7.2 mm blocks, profiles/r05_cull_block_size.json) -- frames narrower than 1280 pixels on a
  // 36 mm sensor take blocks of 32 or 16 pixels (lf_cull_block_log2)
  if (lf_cull_block_log2(ctx, 1, 1) < 0) return LF_CULL_BLOCK_TOO_LARGE;
  return LF_CULL_APPLIED;
}
bool lf_cull_applies(const lf_ctx* ctx, int G) { return lf_cull_reason_of(ctx, G) == LF_CULL_APPLIED; }

// log2 of the side of a cull block in pixels for this frame: 6 (64 pixels) where that is <= kCullMaxBlockMm on the sensor;
// 7 where 128 are still <= kCullBigBlockMm AND the launch has few samples (measured at 4K: 256 spp x 3 wavelengths tie, 1024 x 8
// lose: profiles/r05_march_variants.txt); 5 or 4 (32 / 16 pixels) where 64 are too large (a frame narrower than 1280
// pixels on 36 mm): a wave tile, (8 << xs) pixels wide, then spans several blocks and its lanes look their rows up one by
// one (LfCullArgs::multi); -1: even 16 pixels are too large.
int lf_cull_block_log2(const lf_ctx* ctx, int spp, int n_lambda) {
  const double mm_per_px = (double)ctx->sensor_w_mm / (double)std::max(1, ctx->W);
  int lg = kCullBlockLog2;
  while (lg > 4 && (double)(1 << lg) * mm_per_px > kCullMaxBlockMm) lg--;
  if ((double)(1 << lg) * mm_per_px > kCullMaxBlockMm) return -1;
  if (lg == kCullBlockLog2 && ctx->split.deal != LfSplit::kBlocks && (double)(2 << lg) * mm_per_px <= kCullBigBlockMm && (long long)spp * n_lambda < 768) {
#ifdef LF_EXPERIMENTS
    if (std::getenv("LF_CULL_SMALL_BLOCKS")) return lg;
#endif
    return lg + 1;
  }
  return lg;
}

// set bits of the table's cells (not of the union entries): the (block, cell, path) combinations the march will start
__global__ void k_cull_popcount(const unsigned long long* __restrict__ table, size_t rows, int cells,
                                unsigned long long* __restrict__ out) {
  const size_t n = rows * (size_t)(cells + 1);
  unsigned long long sum = 0ull;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    if ((int)(i % (size_t)(cells + 1)) != cells) sum += (unsigned long long)__popcll(table[i]);
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(out, sum);
}

// ---- the audit: what the table drops, sampled -----------------------------------------------------------------------
// The pre-pass's bounds are estimates (see the head of this file): what stands behind them is a search for counter-examples,
// and a search covers the prescriptions it drew.  So every table is also CHECKED where it is used: for every (block, cell,
// path) combination it does not start, `density` rays of that box -- a random pixel position in the block, a random point of
// the pupil cell, one of the launch's wavelengths; Philox keyed by the launch -- are marched as the march would (geometry
// only, real apertures), and a ray that ends inside the sun's lobe REFUTES the table: the launch marches everything
// (k_march, the path tree) and says so (lf_get_cull_audit, lf_get_cull_reason).  One wave = 64 cells of one block, the
// paths one after the other (wave-uniform event sequence, rows through the scalar cache, lanes whose cell starts the
// path idle): ~10 events per ray, 8.8e7 rays on the bench frame.
constexpr unsigned kDomainAudit = 0x0a0d17c5u;
struct CullAuditArgs {
  int W, H;
  float pitch, half_w, half_h;
  int blocks_x, blocks_y, blk_log2, share_n, share_nb;
  int P, n_paths, n_lambda, march_k, prog_recs;
  float pupil_h, vz, geom_norm, inv_stop_h, lobe_thr;
  int mw, mh;
  uint2 key;
  int density;
  int blk_first, blk_step;     // the blocks audited: blk_first + k blk_step (all of them; the frame dealt by blocks: this rank's)
};
// LIGHTS (several lights): a marched ray of a dropped box refutes the table if it ends inside ANY light's lobe (light_admits:
// the march's own per-light test)
// VAR: 0 = the sun alone; kVarLights = several lights; kVarLights | kVarNear = a point light among them (k_cull_audit_near): the
// EXACT per-ray test on the audit ray's own exit point (light_admits_at), never the widened direction the table was built with
template <int VAR>
__device__ __forceinline__ void cull_audit_body(const LfLensDev* __restrict__ lens, const LfPairsDev* __restrict__ pairs,
                                                const int* __restrict__ seq_table, const LfProgRow* __restrict__ rec_table,
                                                const float* __restrict__ mask, const CullAuditArgs& a,
                                                const unsigned long long* __restrict__ table,
                                                unsigned long long* __restrict__ out) {
  constexpr bool LIGHTS = (VAR & kVarLights) != 0;
  const int blk = a.blk_first + (int)blockIdx.y * a.blk_step;
  const int cells = a.P * a.P;
  const int cell = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if ((cell & ~63) >= cells) return;
  const bool valid = cell < cells;
  const int lane = (int)(threadIdx.x & 63u);
  const unsigned long long* const row = table + lf_cull_row_of_block(blk, a.share_n, a.share_nb) * (size_t)(cells + 1);
  const unsigned long long bits = valid ? row[cell] : ~0ull;
  const int ci = cell % a.P, cj = cell / a.P;
  const int bx = blk % a.blocks_x, by = blk / a.blocks_x;
  const float px0 = (float)(bx << a.blk_log2), px1 = fminf((float)a.W, (float)((bx + 1) << a.blk_log2));
  const float py0 = (float)(by << a.blk_log2), py1 = fminf((float)a.H, (float)((by + 1) << a.blk_log2));
  const float invP = 1.0f / (float)a.P;
  const float sx = lens->sun_dir[0], sy = lens->sun_dir[1], sz = lens->sun_dir[2];
  const float inv_1mc = lens->sun_inv_one_minus_cos, sun_ss = lens->sun_ss;
  unsigned n_rays = 0u, n_lit = 0u;
  for (int q = 0; q < a.n_paths; q++) {
    const bool dropped = valid && ((bits >> q) & 1ull) == 0ull;
    const lanemask todo = __ballot(dropped);
    if (todo == 0ull) continue;
    const int n_ev = pairs->ev_cnt[q];
    const int* const seq = seq_table + pairs->ev_off[q];
    for (int d = 0; d < a.density; d++) {
      // the wavelength of this wave's rays: one per (block, 64 cells, path, repetition), so the rows stay scalar
      const uint4 ru = philox4x32_10(make_uint4((unsigned)blk, blockIdx.x * 4u + (threadIdx.x >> 6), kDomainAudit, (unsigned)(q | (d << 8))), a.key);
      const int l = (int)(__builtin_amdgcn_readfirstlane(ru.x) % (unsigned)a.n_lambda);
      const int g = l / a.march_k, j = l - g * a.march_k;
      const LfProgRow* const recs = rec_table + (size_t)g * (size_t)a.prog_recs;
      const uint4 rnd = philox4x32_10(make_uint4((unsigned)(blk * cells + cell), (unsigned)(q | (d << 8)), kDomainAudit, 1u), a.key);
      const float X = -((px0 + u01(rnd.x) * (px1 - px0)) - a.half_w) * a.pitch;
      const float Y = -((py0 + u01(rnd.y) * (py1 - py0)) - a.half_h) * a.pitch;
      const float ua = ((float)ci + u01(rnd.z)) * invP, ub = ((float)cj + u01(rnd.w)) * invP;
      const StartRay s0 = aim_at_pupil(X, Y, fmaf(2.0f, ua, -1.0f), fmaf(2.0f, ub, -1.0f), a.pupil_h, a.vz, a.geom_norm);
      const float ns = lens->n_start[l];
      Ray r{X, Y, 0.0f, fmaf(X, X, Y * Y), s0.dx * ns, s0.dy * ns, s0.dz * ns, 1.0f, 1.0f};
      lanemask alive = todo;
      n_rays += dropped ? 1u : 0u;
      for (int e = 0; e < n_ev && alive != 0ull; e++) {
        const unsigned se = (unsigned)*(const int __attribute__((address_space(4)))*)(seq + e);
        const LfProgRow wr = load_prec(recs, se & 0xffffu);
        const unsigned kind = se >> 16;
        if (kind & LF_EV_STOP) alive &= stop_event<false>(r, wr.dzv, wr.h2, a.inv_stop_h, mask, a.mw, a.mh);
        else {
          lanemask geom_ok;
          const float cn22 = j == 0 ? wr.cn22[0] : j == 1 ? wr.cn22[1] : wr.cn22[2];
          const float rn2 = j == 0 ? wr.rn2[0] : j == 1 ? wr.rn2[1] : wr.rn2[2];
          const float delta = j == 0 ? wr.delta[0] : j == 1 ? wr.delta[1] : wr.delta[2];
          alive &= surface_event<false>(r, wr.dzv, wr.curv, wr.ch, wr.c2, wr.sc, cn22, rn2, delta, wr.h2, (kind & LF_EV_REFLECT) != 0,
                                        (kind & LF_EV_FLAT) != 0, wr.sgn, geom_ok);
        }
      }
      if (alive == 0ull) continue;
      bool lit;
      if (LIGHTS) {
        lit = false;
        for (int k = 0; k < lens->n_lights; k++) { float qk; lit = light_admits_at<VAR>(lens, k, r.px, r.py, r.hz, r.dx, r.dy, r.dz, qk) || lit; }
        lit = lit && ((alive >> lane) & 1ull) != 0ull;
      } else {
        const float cg = fmaf(r.dx, sx, fmaf(r.dy, sy, r.dz * sz));
        lit = ((alive >> lane) & 1ull) != 0ull && cg > a.lobe_thr && lobe_q(r.dx, r.dy, r.dz, sx, sy, sz, sun_ss, inv_1mc) < 1.0f;
      }
      n_lit += lit ? 1u : 0u;
    }
  }
  unsigned long long v0 = n_rays, v1 = n_lit;
  for (int o = 32; o > 0; o >>= 1) { v0 += __shfl_xor(v0, o); v1 += __shfl_xor(v1, o); }
  if (lane == 0) {
    if (v0) atomicAdd(&out[0], v0);
    if (v1) atomicAdd(&out[1], v1);
  }
}
template <bool LIGHTS>
__global__ __launch_bounds__(256) void k_cull_audit(const LfLensDev* __restrict__ lens, const LfPairsDev* __restrict__ pairs,
                                                    const int* __restrict__ seq_table, const LfProgRow* __restrict__ rec_table,
                                                    const float* __restrict__ mask, CullAuditArgs a,
                                                    const unsigned long long* __restrict__ table,
                                                    unsigned long long* __restrict__ out) {
  cull_audit_body<LIGHTS ? kVarLights : 0>(lens, pairs, seq_table, rec_table, mask, a, table, out);
}
__global__ __launch_bounds__(256) void k_cull_audit_near(const LfLensDev* __restrict__ lens, const LfPairsDev* __restrict__ pairs,
                                                         const int* __restrict__ seq_table, const LfProgRow* __restrict__ rec_table,
                                                         const float* __restrict__ mask, CullAuditArgs a,
                                                         const unsigned long long* __restrict__ table,
                                                         unsigned long long* __restrict__ out) {
  cull_audit_body<kVarLights | kVarNear>(lens, pairs, seq_table, rec_table, mask, a, table, out);
}
// ... an area light among them: lf_area_inside at the audit ray's exit point, never the cone the table took it as
__global__ __launch_bounds__(256) void k_cull_audit_area(const LfLensDev* __restrict__ lens, const LfPairsDev* __restrict__ pairs,
                                                         const int* __restrict__ seq_table, const LfProgRow* __restrict__ rec_table,
                                                         const float* __restrict__ mask, CullAuditArgs a,
                                                         const unsigned long long* __restrict__ table,
                                                         unsigned long long* __restrict__ out) {
  cull_audit_body<kVarLights | kVarNear | kVarArea>(lens, pairs, seq_table, rec_table, mask, a, table, out);
}

// The table is complete (built here, or completed by an all-gather): what fraction of all (block, cell, path)
// combinations it starts -- counted from the table itself, so that every rank of a shared table finds the same number
// and takes the same kernel -- and what its audit says.  `hash`: of the inputs it was built from; published only here.
lf_status lfk_cull_finish(lf_ctx* ctx, uint64_t hash) {
  if (!ctx->cull_popc_dev) LF_HIP(ctx, hipMalloc((void**)&ctx->cull_popc_dev, 4 * sizeof(unsigned long long)));
  LF_HIP(ctx, hipMemsetAsync(ctx->cull_popc_dev, 0, 4 * sizeof(unsigned long long), ctx->stream));
  const LfCullSlab& slab = ctx->cull_resident;
  const size_t rows = slab.nb > 0 ? (size_t)slab.nb * (size_t)slab.n : (size_t)ctx->cull_bx * ctx->cull_by;
  // the blocks this context marches: all of them -- or, the frame dealt by blocks, its own (whose rows lie together: its slab)
  const int n_blk = ctx->cull_bx * ctx->cull_by;
  const bool own = slab.own_rows_only;
  const int own_n = own ? slab.n : 1, own_rank = own ? slab.rank : 0;
  const int n_own_blk = (n_blk - own_rank + own_n - 1) / own_n;
  const size_t row_entries = (size_t)ctx->cull_cells + 1;
  if (own) hipLaunchKernelGGL(k_cull_popcount, dim3(1024), dim3(256), 0, ctx->stream, ctx->cull_dev + (size_t)own_rank * slab.nb * row_entries,
                              (size_t)n_own_blk, ctx->cull_cells, ctx->cull_popc_dev);
  else hipLaunchKernelGGL(k_cull_popcount, dim3(1024), dim3(256), 0, ctx->stream, ctx->cull_dev, rows, ctx->cull_cells, ctx->cull_popc_dev);
  LF_HIP(ctx, hipGetLastError());
  if (ctx->cull_audit_density > 0) {
    const LfLensDev& L = ctx->lens;
    const LfApertureDev& m = ctx->ap[LF_APERTURE_STARBURST];
    CullAuditArgs a;
    std::memset(&a, 0, sizeof(a));
    a.W = ctx->W; a.H = ctx->H; a.pitch = L.pitch; a.half_w = 0.5f * (float)ctx->W; a.half_h = 0.5f * (float)ctx->H;
    a.blocks_x = ctx->cull_bx; a.blocks_y = ctx->cull_by; a.blk_log2 = ctx->cull_blk_log2;
    a.share_n = slab.n; a.share_nb = slab.nb;
    a.P = ctx->cull_P; a.n_paths = ctx->pairs.n; a.n_lambda = L.n_lambda; a.march_k = ctx->march_k; a.prog_recs = ctx->pairs.prog_recs;
    a.pupil_h = L.pupil_h; a.vz = L.pupil_z - L.z_sensor; a.geom_norm = L.geom_norm; a.inv_stop_h = 1.0f / L.stop_h;
    a.lobe_thr = lf_march_lobe_thr(L);
    a.mw = m.w; a.mh = m.h;
    // under LF_MASK_BILINEAR the audit's (unchanged) nearest lookup reads the support texture behind the texels
    const float* audit_mask = m.texels;
    if (ctx->mask_filter == LF_MASK_BILINEAR) { audit_mask = m.texels + (size_t)m.w * m.h; a.mw = 2 * m.w; a.mh = 2 * m.h; }
    const uint64_t k = (ctx->cull_audit_seq++) * 0x9e3779b97f4a7c15ull ^ hash;
    a.key = make_uint2((unsigned)k, (unsigned)(k >> 32));
    a.density = ctx->cull_audit_density;
    a.blk_first = own_rank; a.blk_step = own_n;
    const dim3 grid((unsigned)((ctx->cull_cells + 255) / 256), (unsigned)n_own_blk);
    hipEvent_t ev = lf_timing_begin(ctx, LFK_CULL_AUDIT);
    // (the audit sees every light of the context, whatever the table was built for: lf_test_knob("cull_ignore_light"))
    if (lf_has_area_light(L))
      hipLaunchKernelGGL(k_cull_audit_area, grid, dim3(256), 0, ctx->stream, ctx->lens_dev, ctx->pairs_dev,
                         (const int*)(ctx->prog_dev + ctx->prog_seq_off), (const LfProgRow*)(ctx->prog_dev + ctx->prog_rec_off),
                         audit_mask, a, ctx->cull_dev, ctx->cull_popc_dev + 1);
    else if (lf_has_point_light(L))      // (a point light, also as the only light: the exact test at the audit ray's exit point)
      hipLaunchKernelGGL(k_cull_audit_near, grid, dim3(256), 0, ctx->stream, ctx->lens_dev, ctx->pairs_dev,
                         (const int*)(ctx->prog_dev + ctx->prog_seq_off), (const LfProgRow*)(ctx->prog_dev + ctx->prog_rec_off),
                         audit_mask, a, ctx->cull_dev, ctx->cull_popc_dev + 1);
    else if (L.n_lights > 1)
      hipLaunchKernelGGL(k_cull_audit<true>, grid, dim3(256), 0, ctx->stream, ctx->lens_dev, ctx->pairs_dev,
                         (const int*)(ctx->prog_dev + ctx->prog_seq_off), (const LfProgRow*)(ctx->prog_dev + ctx->prog_rec_off),
                         audit_mask, a, ctx->cull_dev, ctx->cull_popc_dev + 1);
    else
    hipLaunchKernelGGL(k_cull_audit<false>, grid, dim3(256), 0, ctx->stream, ctx->lens_dev, ctx->pairs_dev,
                       (const int*)(ctx->prog_dev + ctx->prog_seq_off), (const LfProgRow*)(ctx->prog_dev + ctx->prog_rec_off),
                       audit_mask, a, ctx->cull_dev, ctx->cull_popc_dev + 1);
    lf_timing_end(ctx, LFK_CULL_AUDIT, ev);
    LF_HIP(ctx, hipGetLastError());
  }
  unsigned long long got[4] = {0ull, 0ull, 0ull, 0ull};
  LF_HIP(ctx, hipMemcpyAsync(got, ctx->cull_popc_dev, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // a bring-up call the host gave up on (lf_comm_poison) publishes nothing: the table it waited for may never have arrived
  if (ctx->comm_poisoned.load()) return lf_fail(ctx, LF_ERR_STATE, "cull table: the communicator was abandoned while the table was being completed");
  ctx->cull_started_fraction = (double)got[0] / ((double)n_own_blk * (double)ctx->cull_cells * (double)std::max(1, ctx->pairs.n));
  ctx->cull_audit_rays += got[1];
  ctx->cull_audit_lit += got[2];
  ctx->cull_hash = hash;
  ctx->cull_bad_hash = 0;
  if (got[2] != 0ull) {          // an audit ray of a dropped box reached the light: this table is not used
    ctx->cull_bad_hash = hash;
    ctx->cull_audit_tripped++;
  }
  return LF_OK;
}

// The slab of table rows this context builds for a table of blocks of 2^blk_log2 pixels (lf_cull_row_of_block).  Dealt by
// blocks (lf_set_block_deal): the rows of this rank's blocks and nobody else's -- the deal's block is 64 pixels, a frame whose
// cull blocks are smaller builds the whole table on every rank (small frames: cheap).  A table shared between ranks: the
// rank's slab, the others come from the all-gather.
static LfCullSlab lf_cull_slab_of(const lf_ctx* ctx, int blk_log2) {
  const LfSplit& s = ctx->split;
  LfCullSlab slab;
  if (s.deal == LfSplit::kBlocks) {
    if (blk_log2 == kDealBlockLog2) { slab.rank = s.rank; slab.n = s.n; slab.own_rows_only = true; }
  } else if (s.table == LfSplit::kComm && ctx->comm_nranks > 1) {
    slab.rank = ctx->comm_rank; slab.n = ctx->comm_nranks;
  } else if (s.table == LfSplit::kHost) {
    slab.rank = s.table_rank; slab.n = s.table_n;
  }
  return slab;
}

// The ball and the dispersion slack grow with the level (a coarse box is more curved than 15 rays show); the zonotope's
// generators are inflated by the same factor at every level: lowered one level at a time, each loses its first lit ray
// between x 0.9 and x 1.0 (a zonotope is EXACT for the linear part of the map, the measured slack covers the rest:
// profiles/r05_march_variants.txt)
static float cull_level_margin(float margin, int P) {
  return margin * (P >= 64 ? 1.0f : P >= 32 ? 1.15f : P >= 16 ? 1.4f : 2.0f);
}

void lf_cull_cache_free(lf_ctx* ctx) {
  LfCullCache& C = ctx->cull_cache;
  if (C.slots) (void)hipFree(C.slots);
  for (float*& f : C.foots) { if (f) (void)hipFree(f); f = nullptr; }
  C.slots = nullptr; C.key = 0; C.reused = false; C.n_levels = 0; C.bytes = 0;
}

// blocks whose rows this rank builds: share_rank, share_rank + share_n, ... (cull_level_body counts them the same way)
static size_t cull_blocks_mine(const CullLevelArgs& a) { return ((size_t)a.blocks_x * a.blocks_y + (size_t)a.share_n - 1 - (size_t)a.share_rank) / (size_t)a.share_n; }

// ---- the levels, coarse to fine: ONE loop for the frame's table (lfk_cull_prepass) and the cached tree (cull_cache_build) ----
struct CullLevelRun {                   // a level as cull_run_levels hands it to its caller's two hooks
  int lv; dim3 grid;
  CullLevelArgs k;                      // the kernel's arguments; list_stride: of the list it writes (the last level: reads)
  size_t n_items, total_items;          // boxes of the longest list (level 0: every box of the own blocks) / of all lists
  const unsigned *items, *items_count; unsigned in_stride;   // the list the level reads, its lengths, its stride (level 0: null, every box)
  unsigned *next, *next_count;          // the list it writes (the last level: null), where it counts what it appends
  bool stop = false, synced = false;    // a hook's word: end here, nothing is wrong / after()'s: it has synchronised the stream
};
enum class CullLevelsEnd { kDone, kStopped, kTooLarge };   // nothing left to run / a hook stopped / a list beyond 2^31 entries

// the launch of a level kernel: the arguments the three of them share, then the kernel's own
template <class Kernel, class... Tail>
static void cull_launch_level(lf_ctx* ctx, Kernel kernel, const CullLevelRun& run, Tail... tail) {
  hipLaunchKernelGGL(kernel, run.grid, dim3(LF_CULL_WG), 0, ctx->stream, ctx->lens_dev, ctx->pairs_dev,
                     (const int*)(ctx->prog_dev + ctx->prog_seq_off), (const LfProgRow*)(ctx->prog_dev + ctx->prog_rec_off),
                     run.k, run.items, run.items_count, run.in_stride, run.next, run.next_count, tail...);
}

// Per level: the arguments, the work lists per path (ping-pong in `lists`, grown on demand), the grid by the longest list,
// launch(run), and the lists' lengths read back for the next level -- after(run) is called with that copy in flight, before the
// stream is synchronised.  Either hook may set run.stop.
template <class Launch, class After>
static lf_status cull_run_levels(lf_ctx* ctx, CullLevelArgs a, const int* levels, int n_levels, LfCullLists& lists,
                                 Launch&& launch, After&& after, CullLevelsEnd* end) {
  const float margin = ctx->cull_rules.margin;
  const size_t n_mine = cull_blocks_mine(a);
  unsigned max_items = 0; size_t total_items = 0;     // of the level about to run (longest list / all lists); level 0 runs every box
  *end = CullLevelsEnd::kDone;
  for (int lv = 0; lv < n_levels; lv++) {
    a.P = levels[lv]; a.last = lv + 1 == n_levels ? 1 : 0;
    a.margin = cull_level_margin(margin, a.P); a.geo_margin = margin;
    CullLevelRun run; run.lv = lv;
    run.n_items = lv == 0 ? n_mine * (size_t)a.P * a.P : (size_t)max_items;
    run.total_items = lv == 0 ? run.n_items * (size_t)a.n_paths : total_items;
    if (run.n_items == 0) break;
    run.items = lv == 0 ? nullptr : lists.list[(lv - 1) & 1];
    run.items_count = lv == 0 ? nullptr : ctx->cull_counts + (size_t)(lv - 1) * kCullMaxPaths;
    run.in_stride = a.list_stride;    // (of the list being read: set when it was written)
    run.next = nullptr; run.next_count = ctx->cull_counts + (size_t)lv * kCullMaxPaths;
    unsigned out_stride = 0;
    if (!a.last) {
      const size_t need = run.n_items * 4;        // every box may keep its four children
      if (need > 0x7fffffffull) { *end = CullLevelsEnd::kTooLarge; return LF_OK; }
      out_stride = (unsigned)need;
      const size_t total = need * (size_t)a.n_paths; const int slot = lv & 1;
      if (total > lists.cap[slot]) {
        LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (lists.list[slot]) (void)hipFree(lists.list[slot]);
        lists.list[slot] = nullptr; lists.cap[slot] = 0;
        LF_HIP(ctx, hipMalloc((void**)&lists.list[slot], total * sizeof(unsigned)));
        lists.cap[slot] = total;
      }
      run.next = lists.list[slot];
    }
    // the kernel reads its input with the stride it was written with (in_stride) and writes with the new one
    run.k = a; run.k.list_stride = a.last ? run.in_stride : out_stride;
    run.grid = dim3((unsigned)((run.n_items + LF_CULL_WG - 1) / LF_CULL_WG), (unsigned)a.n_paths);
    lf_status st = launch(run);
    if (st != LF_OK || run.stop) { *end = CullLevelsEnd::kStopped; return st; }
    LF_HIP(ctx, hipGetLastError());
    a.list_stride = out_stride;
    unsigned cnt[kCullMaxPaths] = {};      // how long the next level's lists are: the grid needs the longest
    if (!a.last) LF_HIP(ctx, hipMemcpyAsync(cnt, run.next_count, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
    st = after(run);
    if (st != LF_OK || run.stop) { *end = CullLevelsEnd::kStopped; return st; }
    if (!a.last && !run.synced) LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    max_items = 0; total_items = 0;
    for (int q = 0; q < a.n_paths; q++) { const unsigned c = std::min(cnt[q], out_stride); max_items = std::max(max_items, c); total_items += c; }
  }
  return LF_OK;
}

// Build the cached tree for `key`: the levels as lfk_cull_prepass runs them (cull_run_levels; it runs once), by the pre-pass's own
// kernel body with the lobe test replaced by "emit".  *fits = false (nothing resident): the tree exceeds the budget.
static lf_status cull_cache_build(lf_ctx* ctx, const CullLevelArgs& a, const int* levels, int n_levels, uint64_t key, bool* fits) {
  LfCullCache& C = ctx->cull_cache;
  *fits = false;
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  lf_cull_cache_free(ctx);
  const double budget = ctx->cull_cache_max_mb * 1048576.0;
  const size_t n_mine = cull_blocks_mine(a);
  size_t slot_entries = 0;
  for (int lv = 0; lv < n_levels; lv++) { C.slot_off[lv] = slot_entries; slot_entries += (size_t)a.n_paths * n_mine * (size_t)levels[lv] * levels[lv]; }
  if (n_mine == 0 || (double)slot_entries * sizeof(unsigned) > budget) return LF_OK;
  LfCullLists lists;               // the build's own (it lists the children of undecided boxes too): they go when it ends
  unsigned* foot_count = nullptr;  // per level, and of the level that runs: its capacity, its footprints as allocated while they are compacted
  size_t foot_cap = 0; float* loose = nullptr;
  // every box of the level may reach the lobe test -- room for all of them, or for what the budget leaves (a level that
  // appends more does not fit); compacted to what was appended, in `after`
  auto launch = [&](CullLevelRun& run) -> lf_status {
    foot_cap = (size_t)std::min((double)run.total_items, std::floor((budget - (double)C.bytes) / 48.0));
    if (run.total_items > 0xfffffff0ull || foot_cap == 0) { run.stop = true; return LF_OK; }
    LF_HIP(ctx, hipMalloc((void**)&C.foots[run.lv], foot_cap * 48));
    CullCacheOut co;
    co.slots = C.slots + C.slot_off[run.lv]; co.foots = (float4*)C.foots[run.lv]; co.foot_count = foot_count + run.lv;
    co.foot_cap = (unsigned)foot_cap; co.n_mine = (unsigned)n_mine;
    cull_launch_level(ctx, k_cull_level_build, run, co);
    return LF_OK;
  };
  auto after = [&](CullLevelRun& run) -> lf_status {
    const int lv = run.lv; unsigned n_foot = 0;
    LF_HIP(ctx, hipMemcpyAsync(&n_foot, foot_count + lv, sizeof(n_foot), hipMemcpyDeviceToHost, ctx->stream));
    LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    run.synced = true;
    if ((size_t)n_foot > foot_cap) { run.stop = true; return LF_OK; }        // beyond the budget
    C.n_foot[lv] = n_foot;
    if ((size_t)n_foot < foot_cap) {                                         // keep what was appended
      loose = C.foots[lv]; C.foots[lv] = nullptr;
      if (n_foot > 0) {
        LF_HIP(ctx, hipMalloc((void**)&C.foots[lv], (size_t)n_foot * 48));
        LF_HIP(ctx, hipMemcpy(C.foots[lv], loose, (size_t)n_foot * 48, hipMemcpyDeviceToDevice));
      }
      (void)hipFree(loose); loose = nullptr;
    }
    C.bytes += (size_t)n_foot * 48;
    return LF_OK;
  };
  CullLevelsEnd end = CullLevelsEnd::kDone;
  hipEvent_t ev = lf_timing_begin(ctx, LFK_CULL_CACHE_BUILD);
  const lf_status st = [&]() -> lf_status {
    LF_HIP(ctx, hipMalloc((void**)&C.slots, slot_entries * sizeof(unsigned)));
    LF_HIP(ctx, hipMalloc((void**)&foot_count, kCullMaxLevels * sizeof(unsigned)));
    LF_HIP(ctx, hipMemsetAsync(C.slots, 0, slot_entries * sizeof(unsigned), ctx->stream));
    LF_HIP(ctx, hipMemsetAsync(foot_count, 0, kCullMaxLevels * sizeof(unsigned), ctx->stream));
    LF_HIP(ctx, hipMemsetAsync(ctx->cull_counts, 0, 8 * kCullMaxPaths * sizeof(unsigned), ctx->stream));
    C.bytes = slot_entries * sizeof(unsigned); C.n_mine = (unsigned)n_mine;
    return cull_run_levels(ctx, a, levels, n_levels, lists, launch, after, &end);
  }();
  // the one way out: an error, a tree beyond the budget and a tree that fits all pass here
  lf_timing_end(ctx, LFK_CULL_CACHE_BUILD, ev);
  void* gone[] = {lists.list[0], lists.list[1], foot_count, loose};
  for (void* g : gone) if (g) (void)hipFree(g);
  if (st != LF_OK || end != CullLevelsEnd::kDone) { lf_cull_cache_free(ctx); return st; }
  for (int i = 0; i < n_levels; i++) C.levels[i] = levels[i];
  C.n_levels = n_levels; C.key = key; C.reused = false; *fits = true;
  return LF_OK;
}

// What decides a table, as its hash takes it in: the level arguments, the levels, the lens, the pairs, the mask -- for the
// cached tree's key (`sun` = false) with every field the sun sets zeroed, by name.  Each caller adds what is its own.
static uint64_t cull_inputs_hash(const lf_ctx* ctx, CullLevelArgs a, const int* levels, int n_levels, bool sun) {
  LfLensDev L = ctx->lens;
  if (!sun) {
    a.sx = a.sy = a.rho = 0.0f;
    L.sun_dir[0] = L.sun_dir[1] = L.sun_dir[2] = 0.0f;
    L.sun_radiance[0] = L.sun_radiance[1] = L.sun_radiance[2] = 0.0f;
    L.sun_inv_one_minus_cos = L.sun_ss = 0.0f;
    // ... and every light's (lf_set_lights): the tree does not depend on how many lights there are, or where
    a.n_lights = 0;
    std::memset(a.lsx, 0, sizeof(a.lsx)); std::memset(a.lsy, 0, sizeof(a.lsy)); std::memset(a.lrho, 0, sizeof(a.lrho));
    L.n_lights = 0;
    std::memset(L.light_dir, 0, sizeof(L.light_dir)); std::memset(L.light_radiance, 0, sizeof(L.light_radiance));
    std::memset(L.light_inv_one_minus_cos, 0, sizeof(L.light_inv_one_minus_cos));
    std::memset(L.light_ss, 0, sizeof(L.light_ss)); std::memset(L.light_thr, 0, sizeof(L.light_thr));
    std::memset(L.light_kind, 0, sizeof(L.light_kind)); std::memset(L.light_pos, 0, sizeof(L.light_pos));
    std::memset(L.light_area, 0, sizeof(L.light_area));
  }
  uint64_t h = 0xcbf29ce484222325ull;
  h = fnv(h, &a, sizeof(a));
  h = fnv(h, levels, sizeof(int) * (size_t)n_levels);
  h = fnv(h, &L, sizeof(L));
  h = fnv(h, ctx->pairs.ij, sizeof(int) * 2 * (size_t)ctx->pairs.n);
  return fnv(h, &ctx->mask_generation, sizeof(ctx->mask_generation));
}

lf_status lfk_cull_prepass(lf_ctx* ctx, int G, int spp) {
  const LfLensDev& L = ctx->lens;
  const lf_ctx::CullRules& R = ctx->cull_rules;
  CullLevelArgs a;
  std::memset(&a, 0, sizeof(a));
  a.W = ctx->W; a.H = ctx->H;
  a.pitch = L.pitch; a.half_w = 0.5f * (float)ctx->W; a.half_h = 0.5f * (float)ctx->H;
  a.blk_log2 = lf_cull_block_log2(ctx, spp, L.n_lambda);
  if (a.blk_log2 < 0) return lf_fail(ctx, LF_ERR_STATE, "cull pre-pass: no block size applies (lf_cull_applies comes first)");
  a.blocks_x = (ctx->W + (1 << a.blk_log2) - 1) >> a.blk_log2;
  a.blocks_y = (ctx->H + (1 << a.blk_log2) - 1) >> a.blk_log2;
  LfCullSlab slab = lf_cull_slab_of(ctx, a.blk_log2);
  const bool shared = slab.n > 1;
  a.share_n = slab.n;
  a.share_rank = slab.rank;
  a.share_nb = (a.blocks_x * a.blocks_y + a.share_n - 1) / a.share_n;
  const int m = cull_m(ctx, G);
  a.P_final = G * m;
  a.n_paths = ctx->pairs.n;
  // dispersion is monotonic in the wavelength's column (lf_derive_lens checks it; otherwise the launch does not cull:
  // LF_CULL_DISPERSION): the two ends of the spectrum bracket what lies between
  a.lam[0] = (L.n_lambda - 1) / 2; a.lam[1] = 0; a.lam[2] = L.n_lambda - 1;
  a.march_k = ctx->march_k; a.prog_recs = ctx->pairs.prog_recs;
  a.pupil_h = L.pupil_h; a.vz = L.pupil_z - L.z_sensor; a.geom_norm = L.geom_norm;
  a.stop_h = L.stop_h; a.inv_stop_h = 1.0f / L.stop_h;
  // the lights the table is built for: all of the context's (light 0 = the sun of lf_set_sun) -- a test leaves one out
  // (lf_test_knob("cull_ignore_light"): a table wrong by construction, which the audit must refute)
  for (int k = 0; k < std::max(1, L.n_lights); k++) {
    if (L.n_lights > 1 && k == ctx->cull_ignore_light) continue;
    const bool sun = L.n_lights <= 1;
    a.lsx[a.n_lights] = sun ? L.sun_dir[0] : L.light_dir[k][0];
    a.lsy[a.n_lights] = sun ? L.sun_dir[1] : L.light_dir[k][1];
    a.lrho[a.n_lights] = lf_cull_lobe_rho(sun ? L.sun_inv_one_minus_cos : L.light_inv_one_minus_cos[k]);
    // a point light enters as the direction unit(L) from the front vertex (light_dir[k]; light 0's is sun_dir too), its
    // radius widened by what that direction can differ from the one an exit point of the front element sees it in
    // an area light enters as the cone lf_area_light_cull_cone gives it: unit(C) (light_dir[k]) and the angular reach of its
    // corners, widened like a point light's (cull_no_widening: the corners' reach alone -- a wrong table, for the audit to refute)
    if (L.n_lights > 0 && L.light_kind[k] == LF_LIGHT_AREA) {
      float dir[3];
      lf_area_cull_cone(L.light_pos[k], L.light_area[k], lf_front_reach(L.surf[0].radius, ctx->raw_semi_ap[0]), !ctx->cull_no_widening, dir,
                        &a.lrho[a.n_lights]);
    } else
    if (L.n_lights > 0 && L.light_kind[k] != LF_LIGHT_DIRECTIONAL && !ctx->cull_no_widening) {
      const double lx = L.light_pos[k][0], ly = L.light_pos[k][1], lz = (double)L.light_pos[k][2] - (double)L.surf[0].zv;
      a.lrho[a.n_lights] += lf_cull_near_widening(lf_front_reach(L.surf[0].radius, ctx->raw_semi_ap[0]), std::sqrt(lx * lx + ly * ly + lz * lz));
    }
    a.n_lights++;
  }
  a.sx = a.lsx[0]; a.sy = a.lsy[0]; a.rho = a.lrho[0];
  const bool lights = a.n_lights > 1;
  std::memcpy(a.occ, ctx->cull_occ, sizeof(a.occ));
  a.keep_partial = R.keep_partial; a.lost_rel = R.lost_rel; a.lost_abs = R.lost_abs; a.strict = R.strict; a.lobe_k = R.lobe_k;
  a.strict_lost = R.strict_lost; a.slack_mode = R.slack_mode; a.disable = R.disable;
  // the levels: P_final, halved while it stays even and >= 8 (a coarser box is too curved for 15 rays to bound)
  int levels[8], n_levels = 0;
  {
    int P = a.P_final;
    levels[n_levels++] = P;
    int coarsest = 8;
#ifdef LF_EXPERIMENTS
    if (const char* e = std::getenv("LF_CULL_P0")) coarsest = std::max(2, std::atoi(e));
#endif
    while (n_levels < 8 && P % 2 == 0 && P / 2 >= coarsest) { P /= 2; levels[n_levels++] = P; }
    std::reverse(levels, levels + n_levels);
  }

  // is the resident table the one these inputs give?
  a.margin = R.margin;
  uint64_t h = cull_inputs_hash(ctx, a, levels, n_levels, true);
  h = fnv(h, &ctx->cull_rules_custom, sizeof(ctx->cull_rules_custom));
  if (shared) {   // (same slab, different tables: only this rank's rows, or all of them completed by an all-gather)
    const int how[2] = {(int)ctx->split.table, slab.own_rows_only ? 1 : 0};
    h = fnv(h, how, sizeof(how));
  }
  if (h == 0) h = 1;
  // ... and the cached tree's key: the same with the sun taken out
  const int how_k[4] = {slab.rank, slab.n, (int)ctx->split.table, slab.own_rows_only ? 1 : 0};
  uint64_t hk = fnv(cull_inputs_hash(ctx, a, levels, n_levels, false), how_k, sizeof(how_k));
  if (hk == 0) hk = 1;
  const size_t rows = (size_t)a.share_nb * (size_t)a.share_n;         // (= nblk unless shared: equal slabs, the last ones padded)
  const size_t row_entries = (size_t)a.P_final * a.P_final + 1;
  const size_t entries = rows * row_entries;
  // (mode 2 rebuilds at every launch -- except the table lf_cull_commit has just completed for this very launch)
  bool reuse = (ctx->march_cull == 1 || ctx->cull_fresh) && ctx->cull_dev && ctx->cull_hash == h;
#ifdef LF_EXPERIMENTS
  if (std::getenv("LF_CULL_NO_REUSE")) reuse = false;
#endif
  ctx->cull_fresh = false;
  ctx->cull_bx = a.blocks_x; ctx->cull_by = a.blocks_y; ctx->cull_cells = a.P_final * a.P_final; ctx->cull_G = G;
  ctx->cull_P = a.P_final; ctx->cull_m = m; ctx->cull_blk_log2 = a.blk_log2;
  if (reuse) return LF_OK;
  if (ctx->split.table == LfSplit::kHost && !ctx->cull_prepare_only)
    return lf_fail(ctx, LF_ERR_STATE, "the cull table is shared through the host (lf_set_cull_share): lf_cull_prepare, the host's "
                                      "all-gather and lf_cull_commit come before lf_trace_ghosts, with the same inputs");
  slab.nb = shared ? a.share_nb : 0;
  ctx->cull_resident = slab;
  if (entries > ctx->cull_cap) {
    LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->cull_dev) (void)hipFree(ctx->cull_dev);
    ctx->cull_dev = nullptr; ctx->cull_cap = 0; ctx->cull_hash = 0;
    LF_HIP(ctx, hipMalloc((void**)&ctx->cull_dev, entries * sizeof(unsigned long long)));
    ctx->cull_cap = entries;
  }
  if (!ctx->cull_counts) LF_HIP(ctx, hipMalloc((void**)&ctx->cull_counts, 8 * kCullMaxPaths * sizeof(unsigned)));
  ctx->cull_hash = 0;
  unsigned long long* stats_dev = nullptr;
#ifdef LF_EXPERIMENTS
  if (std::getenv("LF_CULL_STATS")) LF_HIP(ctx, hipMalloc((void**)&stats_dev, 32 * sizeof(unsigned long long)));
#endif
  // The cached tree (see k_cull_resolve).  Not for a test's rules or the general kernel, nor for a selection split over two
  // tables (their keys would alternate).  Policy: built by the first launch that sees a key -- but once a tree was dropped
  // before any launch reused it (a host that animates focus or zoom), only for a key seen on two launches running.
  bool cached = false;
  if (ctx->cull_cache_on && !ctx->cull_rules_custom && R.disable == 0 && ctx->cull_chunks <= 1 && n_levels <= kCullMaxLevels) {
    LfCullCache& C = ctx->cull_cache;
    if (C.key == hk) { cached = true; C.reused = true; }
    else {
      if (C.key != 0) { C.thrash = !C.reused; LF_HIP(ctx, hipStreamSynchronize(ctx->stream)); lf_cull_cache_free(ctx); }
      if ((hk != C.nofit_key || ctx->cull_cache_max_mb != C.nofit_mb) && (!C.thrash || C.last_key == hk)) {
        const lf_status st = cull_cache_build(ctx, a, levels, n_levels, hk, &cached);
        if (st != LF_OK) return st;
        if (!cached) { C.nofit_key = hk; C.nofit_mb = ctx->cull_cache_max_mb; }
      }
    }
    C.last_key = hk;
  }
  hipEvent_t ev = lf_timing_begin(ctx, LFK_CULL);
  LF_HIP(ctx, hipMemsetAsync(ctx->cull_dev, 0, entries * sizeof(unsigned long long), ctx->stream));
  LF_HIP(ctx, hipMemsetAsync(ctx->cull_counts, 0, 8 * kCullMaxPaths * sizeof(unsigned), ctx->stream));
  if (cached) {
    const LfCullCache& C = ctx->cull_cache;
    CullResolveArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    ra.P_final = a.P_final; ra.n_levels = C.n_levels; ra.n_paths = a.n_paths; ra.patches = (a.P_final + 7) / 8;
    ra.share_rank = a.share_rank; ra.share_n = a.share_n; ra.share_nb = a.share_nb;
    ra.n_mine = C.n_mine; ra.n_waves = C.n_mine * (unsigned)(ra.patches * ra.patches);
    ra.sx = a.sx; ra.sy = a.sy; ra.rho = a.rho; ra.geo_margin = R.margin;
    ra.n_lights = a.n_lights;
    std::memcpy(ra.lsx, a.lsx, sizeof(ra.lsx)); std::memcpy(ra.lsy, a.lsy, sizeof(ra.lsy)); std::memcpy(ra.lrho, a.lrho, sizeof(ra.lrho));
    for (int lv = 0; lv < C.n_levels; lv++) { ra.slots[lv] = C.slots + C.slot_off[lv]; ra.foots[lv] = (const float4*)C.foots[lv]; }
    if (lights) hipLaunchKernelGGL(k_cull_resolve<true>, dim3((ra.n_waves + 3u) / 4u), dim3(256), 0, ctx->stream, ra, ctx->cull_dev);
    else hipLaunchKernelGGL(k_cull_resolve<false>, dim3((ra.n_waves + 3u) / 4u), dim3(256), 0, ctx->stream, ra, ctx->cull_dev);
    LF_HIP(ctx, hipGetLastError());
  } else {
    std::chrono::steady_clock::time_point t_lv;      // (stats_dev: experiments only -- why the boxes of a level ended as they did)
    auto launch = [&](CullLevelRun& run) -> lf_status {
      if (stats_dev) LF_HIP(ctx, hipMemsetAsync(stats_dev, 0, 32 * sizeof(unsigned long long), ctx->stream));
      if (stats_dev) { LF_HIP(ctx, hipStreamSynchronize(ctx->stream)); t_lv = std::chrono::steady_clock::now(); }
      cull_launch_level(ctx, ctx->cull_rules_custom ? k_cull_level_general : lights ? k_cull_level_lights : k_cull_level, run, ctx->cull_dev, stats_dev);
      return LF_OK;
    };
    auto after = [&](CullLevelRun& run) -> lf_status {
      if (!stats_dev) return LF_OK;
      unsigned long long hs[32];
      LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
      std::fprintf(stderr, "CULL_LEVEL P %d items_per_path_max %zu ms %.3f\n", run.k.P, run.n_items,
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_lv).count());
      LF_HIP(ctx, hipMemcpy(hs, stats_dev, sizeof(hs), hipMemcpyDeviceToHost));
      static const char* names[8] = {"", "kept_inside_lobe_partial_box", "kept_too_few_samples_left", "kept_inside_lobe",
                                     "culled_aperture", "culled_mask", "culled_lobe", "culled_all_samples_lost"};
      for (int w = 1; w < 8; w++) std::fprintf(stderr, "CULL_STATS P %d %s %llu\n", run.k.P, names[w], hs[w]);
      return LF_OK;
    };
    CullLevelsEnd end;
    const lf_status st = cull_run_levels(ctx, a, levels, n_levels, ctx->cull_lists, launch, after, &end);
    if (st != LF_OK) return st;
    if (end == CullLevelsEnd::kTooLarge) return lf_fail(ctx, LF_ERR_INVALID, "cull pre-pass: frame too large");
  }
  // (comm_force_exchange: tests only -- the collective also with a single rank, as lf_comm_gather does)
  if (ctx->split.table == LfSplit::kComm && (shared || ctx->comm_force_exchange)) {
    // every rank has built its slab: one in-place all-gather completes the table everywhere
    const lf_status st = lf_comm_allgather_u64_inplace(ctx, ctx->cull_dev, (size_t)a.share_nb * row_entries);
    if (st != LF_OK) return st;
  }
  lf_timing_end(ctx, LFK_CULL, ev);
  if (stats_dev) (void)hipFree(stats_dev);
  if (ctx->cull_prepare_only) {       // the host's exchange is outstanding: lf_cull_commit finishes
    ctx->cull_hash_pending = h;
    return LF_OK;
  }
  return lfk_cull_finish(ctx, h);
}
