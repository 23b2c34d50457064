// lf_internal.h -- shared declarations of liblensflare_hip.so (host + gfx950 device code).
// Nothing here is part of the ABI; the ABI is include/lensflare.h.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "lensflare.h"

// ---- limits -------------------------------------------------------------------------------
// k_march's counters: the seven of lf_counters, executed events, re-march lane events, re-march rows
constexpr int kMarchCounters = 10;
constexpr int kMarchOcclSlot = 10;       // lf_get_ghost_occlusion_stats: shadow tests made, of those blocked (two slots)
constexpr int kMarchCounterSlots = 256;  // allocated (instrumented experiment builds append their tallies)
constexpr int kMarchHistSlot = 16;       // -DLF_MARCH_LIVE_HIST: 3 row kinds x 9 live-lane buckets
constexpr int kMarchPairSlot = 64;       // -DLF_MARCH_PAIR_STATS: 3 x 64 per-path tallies
constexpr int kMaxParaxialGhosts = 3 * 105;          // 3 colours x C(15,2) pairs
constexpr int kMaxGhostTris = 2 * kMaxParaxialGhosts; // two triangles per quad

// ---- device-resident frame state ----------------------------------------------------------
// Mirrors the public per-frame fields of PathTracer (pathtracer.h:93-94,128-135).  Written either
// by the frame-setup kernel (find_sun_pos on the device) or by lf_set_flares.
struct LfFlares {
  int n_flares;
  float angle_to_sun;
  double origin[LF_MAX_FLARES][2];
  double radiance[LF_MAX_FLARES][3];
  double axis_ray[2];
  int n_in_frame;   // in-frame lights find_sun_pos met, those beyond LF_MAX_FLARES (kept by nobody) included
  int pad;
};

// One rasterisable ghost triangle, vertices already y-sorted and shifted by -0.5
// (rasterize_textured_triangle, pathtracer.cpp:346-394).
struct LfGhostTri {
  float x0, y0, u0, v0, x1, y1, u1, v1, x2, y2, u2, v2;
  int bx0, bx1, by0, by1;  // loops run x in [bx0,bx1), y in [by0,by1)  (:402-403)
  double colour[3];        // ghost_color: unit R, G or B times 10 / scale_amt^2 widened (:482-494)
};

struct LfGhostList {
  int n_tris;
  int pad;
  LfGhostTri tri[kMaxGhostTris];
};

// flare occlusion (lf_flare_occlusion.hip): per flare of the flare state the shadow rays that met nothing, and that count
// over the rays per light
struct LfFlareVisDev {
  unsigned long long count[LF_MAX_FLARES];
  double visibility[LF_MAX_FLARES];
};

// Paraxial prescription (globals of pathtracer.cpp:541-556 + constants of :619-633, :737)
struct LfParaxialLens {
  int n, stop;
  float thickness[LF_MAX_SURFACES];
  float curvature[LF_MAX_SURFACES];
  float ior[3][LF_MAX_SURFACES];
  double clip;
  float recast_pos, recast_neg, marginal;
};

struct LfCamera {
  double c2w[9];  // row-major
  double pos[3];
  double hfov_deg, vfov_deg;
  double n_clip = 0.01, f_clip = 100.0;  // Camera::nClip / fClip (camera.h:188)
};

// ---- scene term (row f2): LfSceneDev, LfEnvDev and what they point at ---------------------
#include "lf_scene_types.h"

// per-wavelength starburst (row f4): n = 0 is the reference's monochrome starburst
struct LfStarSpectrum {
  int n, pad;
  double scale[LF_MAX_LAMBDA];     // lambda_ref / lambda_l
  double rgb[LF_MAX_LAMBDA][3];    // weight of wavelength l in R, G, B
};

// the DirectionalLights of find_sun_pos as kernel arguments (6 doubles each: posLight, radiance)
constexpr int kMaxSunLightArgs = 32;
struct LfSunLightArgs { double v[6 * kMaxSunLightArgs]; };

struct LfApertureDev {
  float* texels = nullptr;  // w*h (the STARBURST slot: 5 w h, the support texture of lf_set_mask_filter behind them)
  int w = 0, h = 0;
  lf_aperture_stats* stats = nullptr;  // device copy
  lf_aperture_stats host_stats{};
  double open_radius = 1.0;   // radius of the circle around the texels > 0, in units of the half width (host, lf_set_aperture)
  bool valid = false;
};

// ---- geometric lens (north-star march) -------------------------------------------------------
// One entry per interface and wavelength, everything the march needs, pre-derived on the host in
// float from the raw prescription (see lf_march.hip for the formulas).
struct LfSurfaceDev {
  float zv;        // vertex z (scene side first, light travels +z)
  float curv;      // 1/R, 0 for flats and the stop
  float radius;    // R as given (0 for flats)
  float h2;        // semi-aperture squared
  float is_stop;   // 1.0f for the stop
  float eta_fwd[LF_MAX_LAMBDA];  // n_before / n_after   (ray travelling +z refracts with this)
  float eta_bwd[LF_MAX_LAMBDA];  // n_after / n_before   (ray travelling -z)
  float n_before[LF_MAX_LAMBDA]; // index of the medium on the scene side of the interface
  float n_after[LF_MAX_LAMBDA];  // ... on the sensor side (the stop leaves the medium unchanged)
};

// the ghost march's occlusion test (lf_march_common.h ghost_ray_visible; DESIGN.md section 4, "ghost occlusion")
struct LfOcclDev {
  LfBvhNode* nodes;              // the scene's tree and primitives (LfSceneDev's)
  LfPrim* prims;
  unsigned long long* stats;     // {shadow tests made, of those blocked}: the march counters' slots kMarchOcclSlot, + 1
  double c2w[9], pos[3];         // the camera (lf_set_camera), row-major
  double wpm;                    // world units per lens millimetre
  double z_ref;                  // lens-space z that sits at the camera position: the paraxial entrance pupil (lf_get_lens_camera)
  float front_zv;                // vertex z of interface 0: a completed ghost ray's hz is relative to it
  int pad;
};

struct LfLensDev {
  int n_surf, stop, n_lambda, pad;
  float z_sensor;      // sensor plane z
  float pitch;         // mm per pixel
  float pupil_h;       // semi-aperture of the rear-most surface (pupil sampling disc)
  float pupil_z;       // z of the rear-most vertex
  float geom_norm;     // pupil area / (pupil_z - z_sensor)^2
  float stop_h;        // semi-aperture of the stop
  float sun_dir[3];    // unit, towards the sun (z < 0)
  float sun_radiance[3];
  float sun_inv_one_minus_cos;  // 1 / (1 - cos(angular radius))
  float sun_ss;                 // |sun_dir|^2 of the float vector as stored (exact in double, narrowed)
  float lambda_rgb[LF_MAX_LAMBDA][3];
  float n_start[LF_MAX_LAMBDA];  // index of the medium between the last interface and the sensor
  LfSurfaceDev surf[LF_MAX_SURFACES];
  // Every light of the march (lf_set_lights), light 0 among them: the sun_* fields above ARE light 0, which is all a
  // single-light kernel reads.  Behind everything else, so that no field a single-light kernel reads has moved.
  int n_lights;
  float light_dir[LF_MAX_LIGHTS][3];
  float light_radiance[LF_MAX_LIGHTS][3];
  float light_inv_one_minus_cos[LF_MAX_LIGHTS];
  float light_ss[LF_MAX_LIGHTS];
  float light_thr[LF_MAX_LIGHTS];   // lf_march_lobe_thr of light k (light 0's also travels as MarchArgs::lobe_thr)
  // Point lights (lf_set_lights_ex): light k's kind (lf_light_kind) and, for LF_LIGHT_POINT, its position in lens millimetres;
  // light_dir[k] is then unit(position - front vertex), what the cull pre-pass and lf_get_lights take.  Read by the
  // kVarNear kernels alone, and behind everything else: no field another kernel reads has moved.
  int light_kind[LF_MAX_LIGHTS];
  float light_pos[LF_MAX_LIGHTS][3];
  // Area lights (lf_set_lights_geom, LF_LIGHT_AREA): light_pos[k] is the rectangle's centre, light_area[k] its direction (unit
  // as stored), dim_x and dim_y in lens millimetres; light_thr[k] the squared radius of its bounding sphere (area_bound2,
  // lf_api.hip), light_dir[k] unit(centre - front vertex); there is no lobe (light_inv_one_minus_cos[k] = 1, read by no
  // kernel).  Read by the kVarArea kernels alone, behind everything else.
  float light_area[LF_MAX_LIGHTS][9];
};
// (a light at a finite distance, point or area: the kVarNear kernels, the exact audit, the launch's fit check)
inline bool lf_has_point_light(const LfLensDev& L) {
  for (int k = 0; k < L.n_lights; k++) if (L.light_kind[k] != LF_LIGHT_DIRECTIONAL) return true;
  return false;
}
inline bool lf_has_area_light(const LfLensDev& L) {
  for (int k = 0; k < L.n_lights; k++) if (L.light_kind[k] == LF_LIGHT_AREA) return true;
  return false;
}
// Ghost occlusion (lf_set_ghost_occlusion): the LfOcclDev record of a launch lies BEHIND the device's LfLensDev, in the same
// allocation, at kLensOcclOffset -- not inside it: LfLensDev keeps its size and its 4-byte alignment, so the kernels a context
// without occlusion launches compile to what they were, and nothing keyed on the lens (the cull table's hash) sees it.
// Written by the launch's upload (lf_fill_occlusion), read by the kVarOccl kernels' lit epilogue alone.
constexpr size_t kLensOcclOffset = (sizeof(LfLensDev) + 15) & ~(size_t)15;
constexpr size_t kLensDevBytes = kLensOcclOffset + sizeof(LfOcclDev);

struct LfPairsDev {
  int n;
  int total_events;              // rows of the event table per wavelength
  int ij[LF_MAX_PAIRS + 1][2];   // (-1,-1) = primary path
  int ev_off[LF_MAX_PAIRS + 1];  // first row of pair q in the event table
  int ev_cnt[LF_MAX_PAIRS + 1];  // N + 2(j - i) rows
  int prog_off;                  // first row of the shared-prefix program (wavelength 0)
  int prog_rows;                 // rows of the program per wavelength
  int prog_recs;                 // distinct interface records of a wavelength group's program
};

// One pre-expanded surface event: everything the march needs for it in ONE 32-byte scalar load.
// Two tables use it: the flat per-(wavelength, pair) sequences (n_lambda x total_events rows, read
// only by the rare weight re-march) and the per-wavelength path-tree program (see LF_EV_SAVE0).
struct alignas(32) LfEventRow {
  float dzv;       // vertex z of the interface the ray comes from (or the sensor) minus this one's
  float curv, h2, eta;
  float sgn;       // +1: the ray travels +z (towards the sensor), -1: -z
  int flags;       // bit 0: mirror reflection, bit 1: the stop, bit 2: flat (curv == 0)
  float radius;    // 1 / curv as given in the prescription (0 for flats)
  float eta2;      // eta * eta (float product)
  // (host only; lf_march_tables exports the eight fields above)
  float n_in, n_out;   // index of the medium the ray arrives in / leaves in (equal for a mirror and the stop)
  int surf_dir;        // interface index | direction of travel << 8: what a record is keyed by
  int pad[5];
};
enum { LF_EV_REFLECT = 1, LF_EV_STOP = 2, LF_EV_FLAT = 4 };
// ... and, only in the kind bits of a pair-sequence dword (pack_program) of a lens with aspheres (lf_set_lens_aspheres): the row's
// interface has an aspheric record -- k_march_asph takes asphere_event there (lf_asphere.h).  Never set for any other lens: the
// kernels that compare the kind against the three bits above never see it.
enum { LF_EV_ASPH = 8 };
// ... and, likewise only for a lens with a biconic record (lf_set_lens_biconics): the row's interface is a biconic -- the BIC
// instantiations of k_march_asph take biconic_event there (lf_biconic.h); the row's slot of the aspheric table holds {1/Rx, kx, ky}.
enum { LF_EV_BICONIC = 16 };
// ... and, only for a lens with a pose record (lf_set_lens_poses): the row's interface is posed -- the POSE instantiations of
// k_march_asph take pose_event there (lf_pose.h), on the row's record of the pose table.  The bit comes with LF_EV_ASPH (the
// interface has an aspheric record) or with LF_EV_BICONIC (a biconic record, or a sphere or plane written as one).  (32 is
// lf_path_table.h's LF_EV_SENSOR.)
enum { LF_EV_POSE = 64 };
// the conic constants and even coefficients of the prescription's interfaces (host; lf_set_lens_aspheres): coef[m * n_surfaces + k]
// multiplies r^(4 + 2 m) on interface k.  n = interfaces whose record is not all zero (0: a lens of spheres).
struct LfAspheres {
  int n = 0;
  float kappa[LF_MAX_SURFACES] = {};
  float coef[LF_MAX_ASPH_COEF * LF_MAX_SURFACES] = {};
};
// the biconic records of the prescription's interfaces (host; lf_set_lens_biconics): on[k] != 0: interface k is a biconic of
// x-meridian radius rx[k] (0: flat in x) and conic constants kx[k], ky[k] on the row's own (y-meridian) curvature.  A record
// of zeros is a record (a cylinder with power in y): `on` says whether there is one.  n = the records (0: none).
struct LfBiconics {
  int n = 0;
  int on[LF_MAX_SURFACES] = {};
  float rx[LF_MAX_SURFACES] = {};
  float kx[LF_MAX_SURFACES] = {};
  float ky[LF_MAX_SURFACES] = {};
};
// the pose records of the prescription's interfaces (host; lf_set_lens_poses): on[k] != 0: interface k is decentred by
// t[3 k ..] mm and tilted by a[3 k ..] degrees (lf_pose.h).  A record of zeros is a record.  n = the records (0: none).
struct LfPoses {
  int n = 0;
  int on[LF_MAX_SURFACES] = {};
  float t[3 * LF_MAX_SURFACES] = {};
  float a[3 * LF_MAX_SURFACES] = {};
};
// A program row as the device walks it: the interface once, the index ratios of the up to three
// wavelengths that march it together (lf_march.hip, k_march<K>); one 64-byte scalar load.
// (The program is stored in two levels: a 16-byte header per row -- what is particular to the row --
// and one 64-byte record per distinct (interface, direction of travel) -- the constants of the
// event, shared by all the rows that cross that interface that way.  As one table of 64-byte rows
// the double-Gauss program is 27 KB per wavelength group and misses the CU's 16 KB scalar cache on
// 35 % of its loads (SQC_DCACHE_MISSES, profiles/r02_frontend_counters.json); as 6.8 KB of headers
// + 1.4 KB of records it stays resident.)
struct alignas(16) LfProgHdr {
  int flags;        // as LfEventRow::flags of the per-wavelength program rows
  int skip;         // jump-table entry of this row: (rows to jump << 2) | state to restore
  int rec;          // byte offset of this row's record in the group's record table
  int rec_next;     // ... of the NEXT row's: both loads of the next row can then be issued together
};
// The march carries the ray's direction as OPTICAL direction cosines K = n d (|K| = the index of the
// medium the ray is in, a property of the row): Snell's law is then K' = K + (n' cos t' - n cos t) N with
// no scaling of K by the index ratio, and cos^2 of the refraction angle is one add (round 3; rounds 1-2
// carried the unit direction d and multiplied it by eta = n / n' at every refraction: 4 vector
// instructions per event more).  Per wavelength the record therefore holds
//   cn22 = 2 c n^2      (c F of the vertex-form intersection, with the ray parameter in units of 1 / n)
//   rn2  = R / n^2      (the root (G - sgn sqrt(disc)) R / n^2 of that quadratic)
//   delta = n'^2 - n^2  ((n' cos t')^2 = (n cos t)^2 + delta; negative: total reflection)
// n = index the ray arrives in, n' = leaves in; all float products / quotients of the prescription's
// indices (lf_march.hip pack_program, mirrored by the oracle).
struct alignas(64) LfProgRow {
  float dzv, curv, h2, sc;   // sc = sgn * c
  float sgn;
  float delta[3];   // wavelength g*K + j of group g (repeated past the group's / the lens' last one)
  float cn22[3];
  float ch;         // curv / 2
  float rn2[3];
  float c2;         // 2 curv (both exact: lf_march.hip, surface_event)
};
// what only the weight re-march needs of an (interface, direction): the scale factors of the Fresnel
// fraction (surface_event<true>): fs = 1 / (n + n'), fo = n'^2 / q, fi = n^2 / q, q = n'^2 n + n^2 n'
// coat: 0 = bare glass; else the byte offset, from the start of the weight records (group 0), of the
// interface's film constants (3 x LfCoatK: wavelength j of the group at + 32 j; lf_set_lens_coatings)
struct alignas(64) LfWeightRow {
  float fs[3], pad0;
  float fo[3], pad1;
  float fi[3], pad2;
  int coat;
  float pad3[3];
};
// One wavelength of a coated (interface, direction of travel): the constants of coated_fraction
// (lf_march_events.h), float arithmetic of the prescription and the film (lf_coat_constants):
// dm = m^2 - n^2, ph = 2 d / lambda, the s amplitudes' scales 1 / (n + m), 1 / (m + n') and the p
// amplitudes' m^2 / q1, n^2 / q1 (q1 = m^2 n + n^2 m), n'^2 / q2, m^2 / q2 (q2 = n'^2 m + m^2 n').
struct alignas(32) LfCoatK {
  float dm, ph, s01, s12, p01a, p01b, p12a, p12b;
};
// the film or the stack on interface k of the prescription (host): one state, written by lf_set_lens_coatings and by
// lf_set_lens_coating_stacks.  n_layers[k] = 0: bare; 1: a single film -- thickness_nm[k] / index[] hold it, and the
// LfCoatK records and coated_fraction evaluate it; >= 2: a stack -- thickness_nm[k] is 0, layer_nm / layer_index hold
// the layers, scene side first, zero-thickness layers already dropped (a single film is in them too, as layer 0)
struct LfCoatings {
  int n = 0;                                   // interfaces with a film or a stack (0: none)
  int n_stacked = 0;                           // ... with two or more layers: the kVarStack kernels
  float lambda_nm[LF_MAX_LAMBDA] = {};
  float thickness_nm[LF_MAX_SURFACES] = {};
  float index[LF_MAX_LAMBDA * LF_MAX_SURFACES] = {};   // [l * n_surfaces + k]
  int n_layers[LF_MAX_SURFACES] = {};
  float layer_nm[LF_MAX_COAT_LAYERS * LF_MAX_SURFACES] = {};                     // [j * n_surfaces + k]
  float layer_index[LF_MAX_COAT_LAYERS * LF_MAX_LAMBDA * LF_MAX_SURFACES] = {};   // [(j * n_lambda + l) * n_surfaces + k]
};
constexpr float kCoatMaxThicknessNm = 10000.0f;
void lf_coat_constants(float n_in, float m, float n_out, float thickness_nm, float lambda_nm, LfCoatK* c);
// One wavelength of a STACKED (interface, direction of travel): the record stack_fraction (lf_march_events.h) reads, float
// arithmetic where lf_coat_constants derives the single film's.  m[i], thickness_nm[i]: the N layers in the order the ray
// MEETS them.  out: kStackDwords(N) dwords -- [0] N (an int); [1 + 5 i ..] dm_i = m_i^2 - n^2, ph_i = 2 d_i / lambda and the
// scales of the interface in front of layer i, 1 / (m' + m_i), m_i^2 / q, m'^2 / q (m' the medium in front, q = m_i^2 m' +
// m'^2 m_i); [1 + 5 N ..] the last interface's, between layer N - 1 and n'.
constexpr int kStackDwords(int n_layers) { return 4 + 5 * n_layers; }
void lf_stack_constants(float n_in, float n_out, int n_layers, const float* m, const float* thickness_nm, float lambda_nm,
                        float* out);
// ... of interface `surf` of the installed stacks at wavelength l, for a ray travelling +z (the layers as listed: scene
// side first) or -z (reversed)
void lf_stack_constants_of(const LfCoatings& C, int n_surfaces, int n_lambda, int surf, int l, bool plus_z, float n_in,
                           float n_out, float* out);
// The march does not walk the per-pair sequences one by one: every path of a (sample, wavelength)
// starts with the same backward leg from the sensor, and all pairs (i, .) share the forward leg that
// follows the reflection at i.  The per-wavelength *program* is that tree in depth-first order:
// event rows as above plus, in the flags,
//   SAVE0 / SAVE1  before the event, park the ray state in slot 0 (a prefix fork: the row is the
//                  reflection at i) / slot 1 (a forward-leg fork: the row is the reflection at j)
//   END            after the event the path is complete (lobe test, tallies); bits 24.. = its index
//                  in LfPairsDev; then REST1 / REST0 take the parked state back (neither: the end)
//   bits 8..15     length of the run of plain rows starting here (0 for any flagged row)
//   bits 16..23    multiplicity: how many logical paths share this row (events and fates are
//                  tallied per logical path, exactly as if each had been marched on its own)
enum { LF_EV_REST1 = 8, LF_EV_SAVE0 = 0x10, LF_EV_SAVE1 = 0x20, LF_EV_END = 0x40, LF_EV_REST0 = 0x80 };

// ---- path culling (round 5; lf_cull_prepass.hip builds the table, lf_cull.hip marches what it starts) ----------
// Which paths can carry light from the sun to which part of the sensor through which part of the pupil: for
// every block of 64 x 64 sensor pixels and every cell of a P x P grid over the pupil square (P = G * m: m x m
// cells inside each of the march's G x G strata -- a wave aims all its lanes at ONE sub-cell of its stratum, so
// it knows which table cell it is in) a 64-bit mask of the selected paths, built by a coarse-to-fine pre-pass
// (k_cull_level) that marches 13 rays per (block, cell, path) and bounds where the whole 4-D box can go.  The
// march then starts ONLY the paths whose bit is set: the others end outside the sun's lobe or on a diaphragm,
// i.e. add exactly 0 -- the pixels are those of the full enumeration, bit for bit.  Entry `cells` of a block
// is the union over its cells (the unstratified samples s >= G * G of a non-square sample count).
// sensor blocks of 2^6 = 64 or 2^7 = 128 pixels a side (lf_cull_block_log2): a wave tile of any stride lies inside one;
// 128 where that is still <= 1.25 mm on the sensor (4K on 36 mm: the blocks of 1080p in millimetres, a quarter of the
// pre-pass's boxes) and the launch has few samples (lfk_cull_prepass)
constexpr int kCullBlockLog2 = 6;          // ... 5 or 4 (32 / 16 pixels) on frames whose 64 pixels are too large on the sensor
constexpr double kCullBigBlockMm = 1.25;
constexpr int kCullMaxPaths = 64;        // bits of a mask
constexpr double kCullMaxBlockMm = 1.8;  // a block may be this large on the sensor at most (lf_cull_applies)
constexpr int kCullOcc = 32;             // the stop mask's occupancy grid: kCullOcc x kCullOcc cells, any texel > 0
// A table SHARED between n ranks (lf_set_cull_share): rank b mod n builds block b's row, the rows a rank builds lie
// together (its slab, share_nb rows), the slabs follow each other in rank order -- one in-place all-gather of equal
// slabs completes the table everywhere.  Dealing the blocks round-robin balances the pre-pass: what a block costs
// depends on how many ghosts cross it.  n = 1: row b is block b.
__host__ __device__ inline size_t lf_cull_row_of_block(int b, int share_n, int share_nb) {
  return share_n > 1 ? (size_t)(b % share_n) * (size_t)share_nb + (size_t)(b / share_n) : (size_t)b;
}
constexpr int kMaxSubcellBits = 8;    // lf_set_pupil_subcells: at most 2^8 x 2^8 sub-cells per stratum (k_march_cull's sample list holds both indices)
struct LfCullArgs {
  const unsigned long long* table;   // [rows][cells + 1], row = lf_cull_row_of_block(block); null = every path everywhere
  int blocks_x, blocks_y;
  int prefix_ok;                      // the selection's order lets the started paths share their common leg (march_started_set)
  int multi;                          // a wave tile spans several blocks (blocks of 16 / 32 pixels under a 64-pixel tile): rows per lane
  int share_n, share_nb;              // see lf_cull_row_of_block
  int blk_log2;                       // log2 of a block's side in pixels
  int cells;                          // P * P, P = G * m cells per axis of the pupil square
  int P, m, m_shift;                  // m (1, 2 or 4) table cells per axis inside one stratum; m = 2^m_shift <= the
                                      // sub-cells per axis of the sampling specification (lf_set_pupil_subcells)
  unsigned long long* tail_acc;       // [tail tile][64 lanes][3]: where the workgroups of a split tail tile meet (MarchArgs::tail_from);
  int* tail_done;                     // [tail tile] arrivals: the last one converts and clears both (all zero between launches)
  int items_chunk0;                   // k_march_items: samples per chunk to begin with (the host's estimate from the table's started fraction)
#ifdef LF_EXPERIMENTS
  unsigned long long* wg_clock;       // [workgroup][2]: wall clock at its start / end (LF_MARCH_WG_CLOCK=<file>)
#endif
};

// ---- how a frame is dealt to the ranks of a multi-GPU job ------------------------------------------------------
// by tile rows (8 sensor rows, t % n == rank: lf_set_row_interleave, rounds 1-5) or by BLOCKS of 64 x 64 pixels (row-major
// index b % n == rank: lf_set_block_deal, round 6) -- the block is the cull table's: a rank that owns whole blocks reads only
// the table rows its own pre-pass wrote, so no table ever crosses a link.  bx = blocks per frame row, 0 = dealt by rows.
constexpr int kDealBlockLog2 = 6;
struct LfDeal { int n, rank, bx; };
__host__ __device__ inline bool lf_deal_mine(const LfDeal& d, int x, int y) {
  if (d.n <= 1) return true;
  return d.bx > 0 ? ((y >> kDealBlockLog2) * d.bx + (x >> kDealBlockLog2)) % d.n == d.rank : (y >> 3) % d.n == d.rank;
}
// What a context was asked to do with other ranks: the deal of its pixels, and who completes its cull table.
// Invariant: deal == kBlocks => table == kOwn (a rank that owns whole cull blocks builds the rows it reads and nothing else).
struct LfSplit {
  // the deal: tile rows t (8 sensor rows) with t % n == rank (lf_set_row_interleave), or 64 x 64-pixel blocks b (row-major)
  // with b % n == rank (lf_set_block_deal; kBlocks only with n > 1)
  enum Deal { kRows, kBlocks } deal = kRows;
  int rank = 0, n = 1;
  // who completes the cull table: nobody, this context builds all it reads / the library's RCCL communicator, inside
  // lf_trace_ghosts (lf_comm_share_cull; the slab is comm_rank's of comm_nranks) / the host (lf_set_cull_share: lf_cull_prepare
  // -> its own all-gather -> lf_cull_commit; the slab is table_rank's of table_n > 1, kHost only)
  enum Table { kOwn, kComm, kHost } table = kOwn;
  int table_rank = 0, table_n = 1;
  LfSplit with_deal(Deal d, int r, int k) const { LfSplit s = *this; s.deal = d; s.rank = r; s.n = k; return s; }
  LfSplit with_table(Table t, int r = 0, int k = 1) const { LfSplit s = *this; s.table = t; s.table_rank = r; s.table_n = k; return s; }
};
// The work lists of the pre-pass's levels (lf_cull_prepass.hip cull_run_levels): level lv writes list[lv & 1], per path
// list_stride entries, and the next level reads it.  Grown on demand; cap in entries.
struct LfCullLists { unsigned* list[2] = {nullptr, nullptr}; size_t cap[2] = {0, 0}; };
// A slab of cull table rows: this context builds the rows of the blocks b with b % n == rank (nb rows, lf_cull_row_of_block)
// -- and, own_rows_only (the frame dealt by blocks), nobody completes the others.  {0, 1, 0, false}: the whole table.
struct LfCullSlab { int rank = 0, n = 1, nb = 0; bool own_rows_only = false; };
// The pre-pass's sun-independent part, kept across launches (lf_cull_prepass.hip: k_cull_level_build fills it, k_cull_resolve turns it
// into a launch's table).  Per level one slot per (path, own block, cell) and the exit footprints of the boxes whose fate the
// sun decides.  `key`: the pre-pass's hash with the sun taken out.
struct LfCullCache {
  uint64_t key = 0;                  // of the resident tree (0 = none)
  bool reused = false;               // a launch after the one that built it found it valid
  int n_levels = 0;
  int levels[8] = {};
  unsigned n_mine = 0;               // own blocks
  unsigned* slots = nullptr;         // every level's slots, one allocation
  size_t slot_off[8] = {};           // ... where a level's begin (entries)
  float* foots[8] = {};              // per level: n_foot x 12 floats
  size_t n_foot[8] = {};
  size_t bytes = 0;                  // resident: slots + footprints
  // the policy (lfk_cull_prepass): a host that changes the key at every launch must not pay a build per frame
  bool thrash = false;               // a tree was dropped before it was ever reused: build only a key seen twice running
  uint64_t last_key = 0;             // the previous cacheable launch's key
  uint64_t nofit_key = 0;            // this key's tree exceeded the budget `nofit_mb`: today's path, no second attempt
  double nofit_mb = 0.0;
};

// ---- lens camera (round 4): the scene imaged through the prescription --------------------------
// The primary path N-1 .. 0 of a sensor sample (the ray travels -z, against the light), one row per
// interface in the order the ray meets them, the constants of surface_event for EVERY wavelength
// (lf_march.hip pack_program's float arithmetic; lf_lens_camera.hip build_primary_table).  Read by
// k_lens_rays and by k_scene_term's lens mode through the scalar cache.
struct LfPrimaryRow {
  float dzv, curv, ch, c2, sc, h2;
  int kind;        // 0 = curved glass, LF_EV_STOP, LF_EV_FLAT
  int coated;      // 0 bare; 1: the interface carries a film, coat[] holds its constants; else 2 | the byte offset, from this
                   // row, of its stack records behind the table (a multiple of 4; lf_upload_primary_table, StackPrimary)
  float cn22[LF_MAX_LAMBDA], rn2[LF_MAX_LAMBDA], delta[LF_MAX_LAMBDA];
  float fs[LF_MAX_LAMBDA], fo[LF_MAX_LAMBDA], fi[LF_MAX_LAMBDA];
  LfCoatK coat[LF_MAX_LAMBDA];
};
struct LfPrimaryDev {
  int n, n_lambda;
  float inv_stop_h;      // 1 / stop_h (correctly rounded)
  float front_zv;        // vertex z of interface 0 (0 by construction; kept for clarity)
  float n_start[LF_MAX_LAMBDA];
  LfPrimaryRow row[LF_MAX_SURFACES];
};
// the device allocation behind the table: every interface's stack records at their largest
constexpr size_t kPrimaryStackBytes = (size_t)LF_MAX_SURFACES * LF_MAX_LAMBDA * 4 * (4 + 5 * LF_MAX_COAT_LAYERS);
// The records of a lens with aspheric / biconic interfaces, beside the table in an allocation of their own (LfPrimaryRow keeps
// its layout: the kernels read it with compile-time offsets): per primary row e a kind word -- 0, LF_EV_ASPH or LF_EV_BICONIC --
// and a 32-byte slot in LfAsphRec's layout (lf_asphere.h; a biconic record {1/Rx, kx, ky} sits in the same slot, as it does in
// the march's table).  Built and uploaded by lf_upload_primary_table only for a lens that has records; read by
// primary_path_general (lf_primary_general.h) under LF_LENSCAM_SURFACES_ALL.
// Under LF_LENSCAM_SURFACES_POSED a posed row's kind word also carries LF_EV_POSE (with LF_EV_ASPH or LF_EV_BICONIC: which
// event runs in the surface's frame, as in lf_march_path_rays' rows) and `pose` holds the row's LfPoseRec (lf_pose.h: R
// row-major, t, four spare words), 64 bytes per row BEHIND the records, whose offsets do not move.  Row e is interface
// n - 1 - e: the pose of interface k lies in row n - 1 - k.  Uploaded only for a lens with pose records.
struct alignas(64) LfPrimarySurfDev {
  int kind[LF_MAX_SURFACES];
  alignas(32) float rec[LF_MAX_SURFACES][8];
  alignas(64) float pose[LF_MAX_SURFACES][16];
};
static_assert(offsetof(LfPrimarySurfDev, rec) == 64 && offsetof(LfPrimarySurfDev, pose) == 64 + 32 * LF_MAX_SURFACES,
              "the SURF = 1, 2 kernels read kind and rec at these offsets");
// what k_scene_term's lens mode needs beside the table (kernel argument, by value)
struct LfLensCamArgs {
  int mode;              // 1 = one reference wavelength carries R, G and B; 2 = one ray per wavelength
  int lambda_ref, n_lambda;
  int order_step;        // iteration i of the sample loop takes the march's sample (i * order_step) mod ns_aa
  int xs;                // log2 of the wave tile's pixel stride in x (lf_set_tile_stride)
  int W, G;              // sample_start's SampleSpec (the march's sampling specification)
  float inv_G;
  int sub_bits;
  float inv_sub;
  float pitch, half_w, half_h, pupil_h, vz, geom_norm;
  int mw, mh;
  double exposure;       // scale of the transmitted weight (lf_set_lens_camera)
  double world_per_mm;   // lens millimetres -> scene units
  double z_ref_mm;       // lens-space z that sits at the camera position (the entrance pupil's centre)
  float lambda_rgb[LF_MAX_LAMBDA][3];
};
// k_scene_term's device counters: rays handed to the closest-hit search (camera + shadow + hemisphere
// rays: BVHAccel::total_rays, bvh.h:85,105), primitive tests of closest-hit queries
// (BVHAccel::total_isects, bvh.cpp:211), lens samples started / that left the front element
constexpr int kSceneCounters = 4;

// ---- sensor ghosts (lf_set_sensor_reflectance, lf_set_sensor_ghosts; lf_march_sensor.hip) ------------------------------
// The sensor's reflectance per index column (n_refl = 0: none installed; cleared by lf_set_lens, kept by lf_focus_lens), the
// mode and the selected interfaces (n_sel < 0: every interface but the stop, resolved against the lens of the launch), and
// the paths' own table: one row list per (sensor path, wavelength), resident on the device.  Its dirty test is by content:
// a launch forms the rows on the host (a few hundred, microseconds) and uploads them only where they differ from
// table_host, what the device holds -- so a change of the lens, its focus, films, stacks, aspheric or biconic records, the
// reflectance, the pose records or the selection is caught without every setter having to know the table.  An upload counts
// as one "sensor_table" of lf_timing_get.
constexpr int kSensorStats = 4;   // rays started, that reached the mirror, lost off the rectangle there, lit (ray, light) pairs
struct LfSensorGhosts {
  int n_refl = 0;
  float refl[LF_MAX_LAMBDA] = {};
  int mode = LF_SENSOR_GHOSTS_OFF;
  int surfaces = LF_SENSOR_SURFACES_CENTRED;   // lf_set_sensor_ghost_surfaces (a setting of the context: nothing clears it)
  int n_sel = -1;
  int sel[LF_MAX_SURFACES] = {};
  unsigned char* table_dev = nullptr;
  size_t table_cap = 0;
  std::vector<unsigned char> table_host;
  unsigned long long* stats_dev = nullptr;   // kSensorStats x u64, allocated by the first launch
};

// ---- timing ---------------------------------------------------------------------------------
enum LfKernelId { LFK_MARCH = 0, LFK_FLARE_LAYER, LFK_GHOST_RASTER, LFK_DFT, LFK_FRAME_SETUP,
                  LFK_TONEMAP, LFK_EXCHANGE, LFK_SCENE, LFK_CULL, LFK_CULL_AUDIT, LFK_CULL_CACHE_BUILD, LFK_FLARE_VIS, LFK_MARCH_SENSOR,
                  LFK_SENSOR_TABLE, LFK_COUNT };

struct LfTimedLaunch { int kernel; hipEvent_t start, stop; };

// ---- the context ----------------------------------------------------------------------------
// makes ctx->stream wait for an exchange still running on ctx->comm_stream (lf_group.hip)
lf_status lf_comm_join(struct lf_ctx* ctx);

struct lf_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  mutable std::string err;

  int W = 0, H = 0, y0 = 0, y1 = 0;
  int H_alloc = 0;                     // rows allocated (H rounded up to 64) for in-place gathers
  LfSplit split;                       // how the frame is shared with other ranks: written by lf_install_split alone
  int ns_aa = 1;
  double flare_radius = 25.0, flare_intensity = 1.0;
  int flare_arithmetic = 0;   // lf_set_flare_arithmetic: 0 auto (exact pow in MT19937 parity mode), 1 exact, 2 fast

  LfApertureDev ap[2];
  // starburst spectrum |DFT2(aperture)| / total_value, aw*aw doubles; twiddles; row pass scratch
  double* spectrum = nullptr;
  double2* twiddle = nullptr;
  double2* dft_rows = nullptr;
  bool spectrum_valid = false;

  LfStarSpectrum star_spec{};
  LfParaxialLens pl{};
  LfCamera cam{};
  bool cam_valid = false;
  LfFlares* flares = nullptr;      // device
  LfGhostList* ghosts = nullptr;   // device
  LfParaxialLens* pl_dev = nullptr;
  bool flares_valid = false;
  int flares_n_host = 0;           // n_flares of the device record as the host knows it; -1: counted on the device (lf_find_sun_pos)
  // flare occlusion (lf_set_flare_occlusion, a setting of the context: nothing clears it; lf_flare_occlusion.hip)
  bool flare_occl = false;
  int flare_occl_rays = 0, flare_occl_origin = LF_FLARE_ORIGIN_CAMERA;
  float flare_occl_alpha = 0.0f;
  double flare_occl_wpm = 0.001;
  float* flare_samples_dev = nullptr;      // 4 floats per ray (lf_flare_shadow_samples), resident per setting
  int flare_samples_n = 0;                 // ... rays it holds
  LfFlareVisDev* flare_vis_dev = nullptr;
  LfFlares* flares_eff = nullptr;          // the EFFECTIVE flare record: radiance times visibility
  LfGhostList* ghosts_eff = nullptr;       // ... and quad list: colours times the axis flare's visibility
  double* sun_lights_dev = nullptr;  // staging for more than kMaxSunLightArgs directional lights
  size_t sun_lights_cap = 0;

  double* sample = nullptr;  // W*H*3
  double* ghost = nullptr;   // W*H*3
  double* scene = nullptr;   // W*H*3 or null
  double* star = nullptr;    // W*H*3: raytrace_starburst(x,y) alone (starburst + falloff)
  uint32_t* rgba = nullptr;  // W*H
  uint32_t* rgba_flip = nullptr;  // W*H, allocated by the first lf_save_image_rgba (rows top-down)
  bool ghost_valid = false, sample_valid = false;
  int rgba_y0 = 0, rgba_y1 = 0;  // rows [rgba_y0, rgba_y1) of rgba hold the tonemapped sample buffer

  // jitter
  int jitter_mode = 1;          // 0 = MT19937 table, 1 = counter
  uint64_t jitter_key = 0x1e45f1a4eULL;
  uint32_t* jitter_raw = nullptr;  // W*H*32 raw draws, pixel-major (MT mode)
  bool jitter_table_valid = false;
  uint32_t* jitter_aa_raw = nullptr;  // W*H*2*ns_aa pixel-jitter draws (MT mode), pixel-major
  int jitter_aa_ns = 0;

  // scene term
  LfSceneDev scene_dev{};
  bool scene_valid = false;
  double scene_bmin[3] = {}, scene_bmax[3] = {};   // the BVH root's box (lf_scene_bounds)
  int ns_area_light = 1;          // PathTracer::ns_area_light (pathtracer.h:108; the -l flag)
  LfEnvDev env_dev{};             // PathTracer::envLight (pathtracer.h:119)
  double* env_block = nullptr;    // one allocation behind env_dev's four tables
  double* probe_dev = nullptr;    // 8 doubles: where the single-ray scene probes leave their answer
  bool hemisphere_sample = false; // PathTracer::direct_hemisphere_sample (pathtracer.h:114; the -H flag)
  int samples_per_batch = 32;     // PathTracer::samplesPerBatch default (raytraced_renderer.h:67-81)
  double max_tolerance = 0.05;    // PathTracer::maxTolerance
  int scene_tree_depth = 24;                          // levels of the resident BVH (lf_set_scene): sizes k_scene_lens's stack
  unsigned long long* scene_counters_dev = nullptr;   // kSceneCounters x u64 (lf_get_scene_counters)

  // lens camera (lf_lens_camera.hip): the scene term's sample loop marches each sensor sample's primary
  // path through the prescription instead of calling the pinhole Camera::generate_ray
  int lenscam_mode = 0;               // 0 = off (pinhole), 1 = reference wavelength, 2 = per wavelength
  double lenscam_world_per_mm = 0.001;
  double lenscam_exposure_req = 0.0;  // what lf_set_lens_camera asked for; <= 0: calibrate on the axis
  double lenscam_exposure = 1.0;      // what the kernel uses
  double lenscam_z_ref = 0.0;         // entrance pupil z (mm, lens space)
  float lenscam_aim_margin = 0.0f;    // lf_set_lens_camera_aim: > 0: the lens camera's samples aim at the exit pupil's image
  float lenscam_pupil_h = 0.0f, lenscam_pupil_z = 0.0f, lenscam_geom_norm = 0.0f;   // its own disc (margin > 0)
  bool lenscam_dirty = true;          // table / calibration older than the lens, the mask or the pupil target
  LfPrimaryDev* primary_dev = nullptr;
  int lenscam_surfaces = LF_LENSCAM_SURFACES_SPHERICAL;   // lf_set_lens_camera_surfaces (a setting of the context: nothing clears it)
  LfPrimarySurfDev* primary_surf_dev = nullptr;           // the records of the primary rows (allocated for the first lens that has any)

  // geometric
  LfLensDev lens{};
  bool lens_valid = false, sun_valid = false;
  float light_radius[LF_MAX_LIGHTS] = {};   // the angular radii as lf_set_lights was given them (lf_get_lights)
  // the sampling specification's two coherence parameters (round 4 defaults, measured on the bench frame:
  // profiles/r04_tile_stride.json): 64 x 64 pupil sub-cells per stratum, shared by the 64 pixels of a wave
  // whose columns are 8 apart -- 108 ms and a tile correlation of 7.4 where rounds 1-3 (4 x 4 sub-cells,
  // adjacent pixels) had 110 ms and 37.7
  int march_sub_bits = 6;      // lf_set_pupil_subcells
  int march_xstride_log2 = 3;  // lf_set_tile_stride: the lanes of a wave take pixels 2^this apart in x
  float sensor_w_mm = 36.0f;
  int raw_n = 0, raw_stop = -1;   // the prescription as handed to lf_set_lens (for lf_paraxial_efl)
  float raw_radius[LF_MAX_SURFACES] = {}, raw_thickness[LF_MAX_SURFACES] = {};
  float raw_ior[LF_MAX_LAMBDA * LF_MAX_SURFACES] = {};
  float raw_semi_ap[LF_MAX_SURFACES] = {};
  float pupil_target_h = 0.0f, pupil_target_z = 0.0f;   // lf_set_pupil_target; h <= 0: the rear element
  LfCoatings coat;                                        // lf_set_lens_coatings / lf_set_lens_coating_stacks (cleared by lf_set_lens)
  LfAspheres asph;                                        // lf_set_lens_aspheres (cleared by lf_set_lens, kept by lf_focus_lens)
  LfBiconics bic;                                         // lf_set_lens_biconics (cleared by lf_set_lens, kept by lf_focus_lens)
  LfPoses pose;                                           // lf_set_lens_poses (likewise)
  bool asph_force = false;                                // lf_test_knob("asph_force"): k_march_asph on a lens of spheres, zero records
  int mask_filter = LF_MASK_NEAREST;                      // lf_set_mask_filter (a setting of the context: nothing clears it)
  std::vector<float> mask_host;                           // the STARBURST slot's texels (occupancy / open radius follow the filter)
  bool ghost_accumulate = false;                          // lf_set_ghost_accumulate
  bool ghost_occlusion = false;                           // lf_set_ghost_occlusion (a setting of the context: nothing clears it)
  double ghost_occl_wpm = 0.001;                          // ... its world units per lens millimetre
  int ghost_occl_reach = LF_OCCLUSION_REACH_SKY;          // lf_set_ghost_occlusion_reach (a setting of the context too): where a point
                                                          // light's shadow ray ends; SKY: occlusion with a point light is refused
  LfLensDev* lens_dev = nullptr;
  LfPairsDev pairs{};
  LfPairsDev* pairs_dev = nullptr;
  unsigned long long* counters_dev = nullptr;  // kMarchCounterSlots x u64
  unsigned long long* accum = nullptr;         // W*H_alloc*3 fixed-point partial sums (split launches)
  unsigned long long* tail_acc = nullptr;      // kMarchTailTilesMax x 192 sums + arrivals of the culled march's split tail (lf_cull.hip)
  int* tail_done = nullptr;
  int march_tail_tiles = -1, march_tail_groups = -1;   // lf_test_knob: the tail's size (-1: one round of resident workgroups) / split
  unsigned char* prog_dev = nullptr;           // the packed program: headers, then records (lf_march.hip pack_program)
  size_t prog_cap = 0, prog_rec_off = 0, prog_wrec_off = 0, prog_seq_off = 0;   // bytes; offsets of the records / weight records / pair sequences
  size_t prog_asph_off = 0;                    // ... of the aspheric records, one per program record (0: the lens has none; lf_march_asph.hip)
  // path culling (lf_cull_prepass.hip, lf_cull.hip): 0 = off (k_march walks every path of every sample), 1 = on, the table is reused
  // while its inputs (lens, pairs, sun, frame, pupil disc, mask, strata) are unchanged, 2 = on, rebuilt at every launch
  int march_cull = 1;
  unsigned long long* cull_dev = nullptr;
  size_t cull_cap = 0;                         // entries allocated
  LfCullLists cull_lists;                      // work lists of the pre-pass levels, kept between launches
  unsigned* cull_counts = nullptr;             // [levels][kCullMaxPaths] list lengths
  int cull_m = 1;                              // table cells per axis inside one stratum
  LfCullSlab cull_resident;                    // the layout of the RESIDENT table (written by lfk_cull_prepass alone)
  LfCullCache cull_cache;
  bool cull_cache_on = true;                   // lf_test_knob("cull_cache")
  double cull_cache_max_mb = 8192.0;           // lf_test_knob("cull_cache_max_mb"): the cache's byte budget (8 GiB)
  uint64_t cull_hash_pending = 0;              // of the slab lf_cull_prepare built (the host's exchange is outstanding)
  bool cull_prepare_only = false;              // (lf_cull_prepare is inside lfk_march)
  bool cull_fresh = false;                     // lf_cull_commit just completed the table: the next launch takes it even in mode 2
  unsigned long long* cull_popc_dev = nullptr; // four u64: set bits of the table (k_cull_popcount), then {rays, lit} of its audit
  double cull_started_fraction = 0.0;          // of all (block, cell, path) combinations, what the resident table starts
  // Above this the culled march loses to the path tree: it marches every started path on its own and with its
  // weight, the tree shares legs and lets rays die early (measured crossover on the 1080p frame: a sun of 0.2 rad
  // starts 17 % and ties, profiles/r05_march_variants.txt).  lf_set_march_culling's mode stays what it is; the
  // launch just takes the other kernel.
  double cull_max_fraction = 0.10;             // + 1.6 / paths: see lfk_march
  uint64_t cull_hash = 0;                      // of the inputs the resident table was built from (0 = none)
  int cull_bx = 0, cull_by = 0, cull_cells = 0, cull_G = 0, cull_P = 0, cull_blk_log2 = 6;
  // The pre-pass's rules.  What ships is ONE set (lf_cull_prepass.hip k_cull_level, constants in the kernel); a test may install
  // another through lf_test_knob ("cull_strict", ...: the rules round 5 replaced, kept to show what the audit is for) --
  // the table is then built by k_cull_level_general, which reads them from here.
  struct CullRules {
    float margin = 1.25f;        // footprint inflation
    int strict = 1, strict_lost = 1, slack_mode = 1, keep_partial = 0, disable = 0;
    float lobe_k = 1.2f, lost_rel = 0.5f, lost_abs = 0.002f;
  } cull_rules;
  bool cull_rules_custom = false;              // a test installed rules / asked for the general kernel (lf_test_knob)
  bool cull_force = false;                     // lf_test_knob("cull_force"): the culled kernel whatever the table starts
  bool cull_weights_first = false;             // lf_test_knob("cull_weights_first"): k_march_cull<K, true>
  int cull_ignore_light = -1;                  // lf_test_knob("cull_ignore_light"): the pre-pass / resolve leave this light out (a table wrong by construction)
  bool cull_no_widening = false;               // lf_test_knob("cull_no_widening"): a point light's radius in the cull table NOT widened (a table wrong by construction)
  bool cull_no_prefix = false;                // lf_test_knob("cull_no_prefix"): every started path marched alone from the sensor (round 5)
  int scene_compact = -1;                      // lf_test_knob("scene_compact"): -1 = by the tree's size, 0 / 1 forced
  bool comm_force_exchange = false;            // lf_test_knob("comm_force_exchange"): the collectives also with one rank
  int scene_lens_strided = -1;                 // lf_test_knob("scene_lens_strided"): k_scene_lens's wave tile: -1 by the tree's size, 0 / 1
  bool bvh_median = false;                     // lf_test_knob("bvh_median"): the round-2 median-split tree (A/B of the SAH tree)
  int bvh_leaf_max = 2;                        // lf_test_knob("bvh_leaf"): primitives per leaf at most (1 .. 4)
  // the audit of what the table drops (lf_cull_prepass.hip k_cull_audit): rays per dropped (block, cell, path), 0 = off
  int cull_audit_density = 1;
  unsigned long long cull_audit_rays = 0, cull_audit_lit = 0;   // since lf_reset_counters
  int cull_audit_tripped = 0;                  // launches since lf_reset_counters whose table an audit ray refuted
  uint64_t cull_bad_hash = 0;                  // the resident table was refuted: its launches march everything
  int cull_reason = 0;                         // why the last launch did (not) cull: lf_cull_reason
  int cull_chunks = 1;                         // launches the last lf_trace_ghosts split its selection into (> 64 paths: 2)
  uint64_t cull_audit_seq = 0;                 // tables audited by this context: keys the audit's rays
  bool lens_lambda_monotonic = true;           // every glass disperses the same way along the wavelength columns (lf_derive_lens)
  unsigned cull_occ[kCullOcc] = {};            // occupancy of the stop mask (host, lf_set_aperture)
  uint64_t mask_generation = 0;                // bumped by lf_set_aperture(STARBURST) and by a switch of lf_set_mask_filter
  bool last_march_culled = false;              // what the last lf_trace_ghosts ran
  int march_k = 1;                             // wavelengths (rays per lane) that walk together
  int march_fix_bits = 36;                     // the last launch's fixed-point exponent (lf_get_march_fix_bits)
  bool events_dirty = true;
  LfSensorGhosts sensor;                       // the sensor's mirror: reflectance, mode, selection and the paths' table

  // multi-GPU (lf_group.hip): the communicator this context belongs to, staging for the exchange
  void* comm = nullptr;          // ncclComm_t, or null (single GPU / rehearsal group)
  int comm_nranks = 1, comm_rank = 0;
  double* comm_stage = nullptr;  // send [groups][e] followed by recv [world][groups][e]
  size_t comm_stage_cap = 0;     // doubles
  // lf_comm_gather_async: the exchange of frame k runs on its own stream while frame k + 1 is marched
  hipStream_t comm_stream = nullptr;
  hipEvent_t comm_ev_main = nullptr, comm_ev_pack = nullptr, comm_ev_done = nullptr;
  hipEvent_t comm_ev_table = nullptr, comm_ev_table_done = nullptr;   // the shared cull table's all-gather (lf_comm_allgather_u64_inplace)
  bool comm_pending = false;     // an exchange on comm_stream the main stream has not yet waited for
  bool comm_f32 = false;         // lf_comm_set_exchange_precision(32): the tile rows travel as floats
  // A communicator call can block the calling HOST thread for good (ncclCommInitRank, the first collective's
  // enqueue: a peer that never joins).  A host that gives up on such a call from another thread says so with
  // lf_comm_poison: from then on the blocked call -- should it ever return -- publishes NOTHING into the context
  // (a communicator that arrives late is aborted where it stands), every lf_comm_* call is refused, and lf_destroy
  // leaks the context instead of freeing what the blocked thread still stands on.
  std::atomic<int> comm_busy{0};         // threads inside a call that may block
  std::atomic<bool> comm_poisoned{false};
  std::mutex comm_mu;                    // publication of comm / comm_nranks / comm_rank / comm_pending

  bool timing = false;
  std::vector<LfTimedLaunch> timed;       // launches not folded yet (bounded, see lf_api.hip)
  std::vector<hipEvent_t> event_pool;     // recycled events
  double timed_ms[LFK_COUNT] = {};        // folded totals since lf_timing_reset
  int timed_n[LFK_COUNT] = {};
};

// implemented in lf_api.hip
lf_status lf_fail(const lf_ctx* ctx, lf_status st, const std::string& msg);
// (stream: where the timed work runs; null = the context's main stream)
hipEvent_t lf_timing_begin(lf_ctx* ctx, int kernel, hipStream_t stream = nullptr);
void lf_timing_end(lf_ctx* ctx, int kernel, hipEvent_t start, hipStream_t stream = nullptr);

#define LF_HIP(ctx, expr)                                                                     \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return lf_fail(ctx, LF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
  } while (0)

// candidate selection of the march (the contract, the same expression in oracle/lf_geo_oracle.c): d.s above
// 1 - 1.0625 (1 - cos alpha) - 4e-7 MAY lie inside the lobe.  The 1/16 margin is relative, the 4e-7 absolute: the float
// dot product of two unit vectors is only good to ~2e-7, so a relative margin alone loses part of a sub-milliradian
// sun's lobe (1 - cos(0.8 mrad) = 3.2e-7).  Rounded down: float(thr) never exceeds thr.
inline float lf_march_lobe_thr_of(float inv_one_minus_cos) {
  const double thr = 1.0 - (1.0625 / (double)inv_one_minus_cos) * (1.0 + 1e-6) - 4e-7;
  float t = (float)thr;
  if ((double)t > thr) t = std::nextafterf(t, -2.0f);
  return t;
}
inline float lf_march_lobe_thr(const LfLensDev& L) { return lf_march_lobe_thr_of(L.sun_inv_one_minus_cos); }
// the radius, in (x, y) direction space, of what the pre-test admits around a light: the cull pre-pass's lobe test
// (a ray contributes only if d.s > lobe_thr: |d - s|^2 = 2 - 2 d.s < 2 (1 - thr) for unit vectors, and the (x, y)
// projection is no longer than the vector; the float march's directions are unit to ~1e-6)
inline float lf_cull_lobe_rho(float inv_one_minus_cos) {
  const double thr = 1.0 - (1.0625 / (double)inv_one_minus_cos) * (1.0 + 1e-6) - 4e-7;
  return (float)(std::sqrt(2.0 * (1.0 - thr)) * 1.001 + 1e-5);
}

inline LfDeal lf_deal_of(const lf_ctx* ctx) {
  const LfSplit& s = ctx->split;
  return LfDeal{s.n, s.rank, s.deal == LfSplit::kBlocks ? (ctx->W + (1 << kDealBlockLog2) - 1) >> kDealBlockLog2 : 0};
}
// The only writer of ctx->split: every setter validates its arguments, then installs the whole record.  A slab prepared for
// the host's exchange, or a table it completed, belongs to the table share it was built for: a different share drops it.
// (Whether the resident table is the one a launch needs is the pre-pass's hash to decide: lfk_cull_prepass.)
inline void lf_install_split(lf_ctx* ctx, const LfSplit& s) {
  const LfSplit& o = ctx->split;
  if (s.table != o.table || s.table_rank != o.table_rank || s.table_n != o.table_n) {
    ctx->cull_hash_pending = 0;
    ctx->cull_fresh = false;
  }
  ctx->split = s;
}
// the kernel variant of the weighted march (lf_march_events.h: kVarBare .. kVarCoatFilt, | kVarLights: several lights, | kVarStack,
// | kVarOccl: ghost occlusion -- always with kVarLights, whose epilogue it extends: one light is a list of one)
// | kVarNear: some installed light is a point light (lf_set_lights_ex) -- with kVarLights too, also when it is the only light
// | kVarNear | kVarOccl together: launched only under LF_OCCLUSION_REACH_LIGHT (lf_set_ghost_occlusion_reach); under
//   LF_OCCLUSION_REACH_SKY the launch's upload refuses the combination before any switch on the variant is reached
// | kVarArea: some installed light is an area light (lf_set_lights_geom) -- with kVarLights | kVarNear, also as the only light
inline int lf_march_variant(const lf_ctx* ctx) {
  const bool near = lf_has_point_light(ctx->lens);
  return (ctx->coat.n > 0 ? 1 : 0) | (ctx->mask_filter == LF_MASK_BILINEAR ? 2 : 0) |
         ((ctx->lens.n_lights > 1 || ctx->ghost_occlusion || near) ? 4 : 0) |
         (ctx->coat.n_stacked > 0 ? 8 : 0) |   // (kVarStack: only ever with kVarCoat -- a stacked interface counts in coat.n)
         (ctx->ghost_occlusion ? 16 : 0) |
         (near ? 32 : 0) |
         (lf_has_area_light(ctx->lens) ? 64 : 0);   // (kVarArea: an area light is a light at a finite distance too -- always with 4 | 32)
}
// The front element as a point light sees it (lf_set_lights_ex): r_f = sqrt(h0^2 + sag(h0)^2), the largest distance from the
// front vertex to a point of its clear aperture (radius 0: flat; a semi-aperture beyond the sphere: the hemisphere's)
inline double lf_front_reach(float radius, float semi_aperture) {
  const double h = semi_aperture, R = std::fabs((double)radius);
  const double sag = radius == 0.0f ? 0.0 : (h < R ? R - std::sqrt(R * R - h * h) : R);
  return std::sqrt(h * h + sag * sag);
}
// ... and how much wider than its lobe the cull pre-pass takes a point light at distance dist from the front vertex, in
// direction space around unit(L): for P on the front cap |unit(L - P) - unit(L)| <= |P| / min(|L - P|, |L|) <= r_f / (dist - r_f)
// (DESIGN.md section 5), with the relative and absolute float slack lf_cull_lobe_rho carries
inline float lf_cull_near_widening(double r_f, double dist) { return (float)(r_f / (dist - r_f) * 1.001 + 1e-5); }
// An area light (lf_set_lights_geom) as the cull pre-pass takes it (lf_area_light_cull_cone is this, exported; lf_api.hip):
// dir = unit(C) from the front vertex, *rho = max over the four corners of |unit(corner) - unit(C)| -- reached at a corner: the
// points within an angle below 90 degrees of unit(C) form a cone whose section by the light's plane is convex; a corner at
// 90 degrees or more: 2, every direction -- plus, with `widen`, r_f / (dmin - r_f), dmin the distance from the front vertex
// to the nearest point of the rectangle; with lf_cull_near_widening's relative and absolute slack.  C: the centre, g:
// direction, dim_x, dim_y as stored (LfLensDev::light_area).  All in double.
void lf_area_cull_cone(const float* C, const float* g, double r_f, bool widen, float dir[3], float* rho);
// the cull table is not this context's alone: shared between ranks, or built only in part (the frame dealt by blocks)
inline bool lf_cull_table_split(const lf_ctx* ctx) {
  return ctx->split.table != LfSplit::kOwn || ctx->split.deal == LfSplit::kBlocks;
}
// the flare layer calls the reference's own pow() (exact) or its cheaper equivalents (fast): DESIGN.md section 3
inline bool lf_flare_exact(const lf_ctx* ctx) {
  return ctx->flare_arithmetic == 1 || (ctx->flare_arithmetic == 0 && ctx->jitter_mode == 0);
}
// kernels launchers (lf_flare_kernels.hip)
lf_status lfk_aperture_stats(lf_ctx* ctx, int slot);
lf_status lfk_build_spectrum(lf_ctx* ctx);
lf_status lfk_frame_setup(lf_ctx* ctx, const LfSunLightArgs* lights_arg, const double* lights_dev,
                          int n_lights, bool project);
lf_status lfk_ghost_raster(lf_ctx* ctx, const LfGhostList* gl = nullptr);   // (gl, fl: null = the installed records)
// single-shot forms of the reference's public helper members (lf_draw_ghost ... lf_irradiance_falloff)
lf_status lfk_draw_ghost(lf_ctx* ctx, int channel, float r1, float r2, int bbox[4]);
lf_status lfk_raster_triangle(lf_ctx* ctx, const float v[12], const double colour[3], int bbox[4]);
lf_status lfk_fill_pixel(lf_ctx* ctx, const float v[12], int x, int y, const double colour[3]);
lf_status lfk_shift_vertex(lf_ctx* ctx, float x, float y, float scale, float shift_amount, double out[2]);
lf_status lfk_compute_phase(lf_ctx* ctx, int flare, double u, double v, double out[4]);
lf_status lfk_irradiance_falloff(lf_ctx* ctx, int x, int y, double radius, double out[3], const LfFlares* fl = nullptr);
lf_status lfk_flare_layer(lf_ctx* ctx, const LfFlares* fl = nullptr);
// lf_flare_occlusion.hip: the records a consuming call renders from -- the installed ones while lf_set_flare_occlusion is off
// (nothing is launched), else the effective ones, behind the two visibility kernels on the context's stream (`who` names
// the caller in the refusal, LF_ERR_STATE, of a state that lacks a camera, a scene or, for the front element's rays, a lens)
lf_status lf_flare_occlusion_update(lf_ctx* ctx, const char* who, const LfFlares** fl, const LfGhostList** gl);
void lf_flare_occlusion_free(lf_ctx* ctx);   // lf_destroy
lf_status lfk_tonemap(lf_ctx* ctx, int ya, int yb);
lf_status lfk_flip_rows(lf_ctx* ctx, uint32_t* out_dev);
// lf_march.hip
lf_status lfk_march(lf_ctx* ctx, int spp, uint64_t key);
lf_status lfk_lens_rays(lf_ctx* ctx, int lambda, int n, const float* d_xy, const float* d_uv,
                        float* d_out);
// ghost occlusion: what a launch / a query needs installed (`who` names the caller in the refusal), the device record of the
// state installed, and the batched per-ray query (d_rays: n x 6 floats, d_vis: n bytes)
lf_status lf_occlusion_ready(const lf_ctx* ctx, const char* who);
lf_status lf_fill_occlusion(const lf_ctx* ctx, double world_per_mm, LfOcclDev* o);
lf_status lfk_ghost_ray_visibility(lf_ctx* ctx, const LfOcclDev& o, size_t n, const float* d_rays, unsigned char* d_vis);
// ... per installed light, over [0, reach_k] (d_vis: n x n_lights bytes; the lens as uploaded holds the lights), and the
// refusal of occlusion with a point light installed unless the shadow rays end at the light (lf_set_ghost_occlusion_reach)
lf_status lfk_ghost_ray_light_visibility(lf_ctx* ctx, const LfOcclDev& o, size_t n, const float* d_rays, unsigned char* d_vis);
lf_status lf_occlusion_reach_ready(const lf_ctx* ctx, const char* who);
// point lights (lf_set_lights_ex): the installed ones against the front element of the lens as it is now (`who` names the
// caller in the refusal, LF_ERR_STATE); the batched per-ray lobe factors (d_rays: n x 6 floats, d_out: n x n_lights floats)
lf_status lf_point_lights_fit(const lf_ctx* ctx, const char* who);
lf_status lfk_ghost_ray_light_factors(lf_ctx* ctx, size_t n, const float* d_rays, float* d_out);
// lf_lens_camera.hip
lf_status lf_lenscam_prepare(lf_ctx* ctx);            // table + calibration up to date (no-op when clean)
lf_status lf_upload_primary_table(lf_ctx* ctx);       // LfPrimaryDev from ctx->lens (k_lens_rays needs it too)
void lf_fill_lenscam_args(const lf_ctx* ctx, LfLensCamArgs* a);
lf_status lf_build_march_tables(lf_ctx* ctx, std::vector<LfEventRow>& rows, std::vector<int>& skip);
lf_status lfk_mask_support(lf_ctx* ctx);              // the support texture of the bilinear stop mask, behind the texels
lf_status lfk_native_sqrt(lf_ctx* ctx, const float* d_x, float* d_y, size_t n);
lf_status lfk_native_rcp(lf_ctx* ctx, const float* d_x, float* d_y, size_t n);
void lf_apply_pupil_target(lf_ctx* ctx);
int lf_march_fix_bits(const LfLensDev& L, int n_paths, int spp);
// lf_cull_prepass.hip: the cull table
bool lf_cull_applies(const lf_ctx* ctx, int G);
int lf_cull_reason_of(const lf_ctx* ctx, int G);                       // lf_cull_reason: LF_CULL_APPLIED or why not
int lf_cull_block_log2(const lf_ctx* ctx, int spp, int n_lambda);      // log2 of a cull block's side in pixels (-1: none applies)
lf_status lfk_cull_prepass(lf_ctx* ctx, int G, int spp);
lf_status lfk_cull_finish(lf_ctx* ctx, uint64_t hash);                 // the table is complete: count what it starts, audit it
void lf_cull_cache_free(lf_ctx* ctx);               // lf_destroy
// lf_cull.hip: the march of what the table starts (a = the launch's arguments as lfk_march set them up: lf_march_common.h)
namespace lfm { struct MarchArgs; }
lf_status lfk_march_culled(lf_ctx* ctx, const lfm::MarchArgs& a, size_t blocks, size_t dyn_lds);
// lf_march.hip
lf_status lfk_cull_prepare(lf_ctx* ctx, int spp);
// lf_march_asph.hip: the march of a lens with aspheres (or of any lens under lf_test_knob("asph_force")), every path alone;
// the batched single event; one explicit ray per lane along the sequence of pair (i, j)
// (a lens with a biconic record, lf_set_lens_biconics, takes the same route through the kernel's BIC instantiations)
inline bool lf_march_biconic(const lf_ctx* ctx) { return ctx->bic.n > 0; }
// (and so does a lens with a pose record, lf_set_lens_poses, through the POSE instantiations)
inline bool lf_march_posed(const lf_ctx* ctx) { return ctx->pose.n > 0; }
inline bool lf_march_aspheric(const lf_ctx* ctx) {
  return ctx->asph.n > 0 || ctx->asph_force || lf_march_biconic(ctx) || lf_march_posed(ctx);
}
// is there a record on glass interface k, and of which kind: 0, LF_EV_BICONIC or LF_EV_ASPH.  ONE predicate for the rows of
// lf_march_path_rays (build_path_table) and of the lens camera's primary table (lf_upload_primary_table), so that
// lf_generate_lens_rays and the scene kernel agree on which rows are recorded.
inline int lf_surface_record_kind(const lf_ctx* ctx, int k) {
  const LfAspheres& A = ctx->asph;
  const int n_surf = ctx->lens.n_surf;
  bool any = A.kappa[k] != 0.0f;
  for (int m = 0; m < LF_MAX_ASPH_COEF; m++) any = any || A.coef[(size_t)m * n_surf + k] != 0.0f;
  if (ctx->bic.n > 0 && ctx->bic.on[k]) return LF_EV_BICONIC;
  if (A.n > 0 ? any : (ctx->asph_force && ctx->lens.surf[k].curv != 0.0f)) return LF_EV_ASPH;
  return 0;
}
lf_status lfk_march_asph(lf_ctx* ctx, const lfm::MarchArgs& a, size_t blocks);
lf_status lfk_asphere_events(lf_ctx* ctx, const float* consts16, int reflect, int forward, size_t n, const float* d_rays,
                             float* d_out, int* d_fates);
lf_status lfk_biconic_events(lf_ctx* ctx, const float* consts16, int reflect, size_t n, const float* d_rays, float* d_out,
                             int* d_fates);
lf_status lfk_pose_events(lf_ctx* ctx, const float* consts16, const float* pose16, int reflect, int asph, size_t n,
                          const float* d_rays, float* d_out, int* d_fates);
lf_status lfk_march_path_rays(lf_ctx* ctx, int lambda, int i, int j, int n, const float* d_xy, const float* d_uv, float* d_out);
// lf_march_sensor.hip: the sensor ghosts -- the frame's launch behind (add) or instead of the ordinary march, one explicit ray
// per lane along the sensor path of interface i, and what lf_destroy frees
lf_status lfk_march_sensor(lf_ctx* ctx, int spp, uint64_t key, bool add);
lf_status lfk_march_sensor_path_rays(lf_ctx* ctx, int lambda, int i, int n, const float* d_xy, const float* d_uv, float* d_out);
int lf_sensor_selection(const lf_ctx* ctx, int out[LF_MAX_SURFACES]);   // the interfaces a launch marches, in order; -1: one no longer fits the lens
void lf_sensor_free(lf_ctx* ctx);
// lf_group.hip: in-place all-gather of equal slabs of u64 on the communicator's stream, ordered after what the main
// stream has queued and before what it queues next
lf_status lf_comm_allgather_u64_inplace(lf_ctx* ctx, unsigned long long* base, size_t count_per_rank);
void lf_derive_lens(lf_ctx* ctx, int n, int stop, int n_lambda, const float* radius,
                    const float* thickness, const float* ior, const float* semi_ap,
                    float sensor_w_mm);
