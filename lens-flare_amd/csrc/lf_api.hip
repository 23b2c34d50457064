// lf_api.hip -- the extern "C" entry points of liblensflare_hip.so (include/lensflare.h).
// Host-side orchestration only: validation, device buffers, stream/event handling.  Every
// number that reaches a sensor pixel is computed by the gfx950 kernels in lf_flare_kernels.hip /
// lf_march.hip; there is no CPU fallback -- without a device lf_create fails.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lf_internal.h"
#include "lf_march_events.h"
#include "lf_asphere.h"
#include "lf_biconic.h"
#include "lf_pose.h"
#include "lf_sensor_event.h"
#include "../host/lf_collada.h"

lf_status lf_fail(const lf_ctx* ctx, lf_status st, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return st;
}

// HIP-event timing.  Events come from a pool and the list of pending launches is bounded: once it
// holds kTimedCap entries the finished ones are folded into per-kernel totals and their events go
// back to the pool, so a long timed run neither grows without bound nor creates events per launch.
static constexpr size_t kTimedCap = 512;

static hipEvent_t timing_event(lf_ctx* ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

// fold every launch whose stop event has completed (all of them if `wait`)
static void timing_fold(lf_ctx* ctx, bool wait) {
  size_t keep = 0;
  for (size_t i = 0; i < ctx->timed.size(); i++) {
    LfTimedLaunch& t = ctx->timed[i];
    const bool done = wait ? hipEventSynchronize(t.stop) == hipSuccess : hipEventQuery(t.stop) == hipSuccess;
    float ms = 0.f;
    if (done && hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) {
      ctx->timed_ms[t.kernel] += ms;
      ctx->timed_n[t.kernel]++;
      ctx->event_pool.push_back(t.start);
      ctx->event_pool.push_back(t.stop);
    } else {
      ctx->timed[keep++] = t;
    }
  }
  ctx->timed.resize(keep);
}

hipEvent_t lf_timing_begin(lf_ctx* ctx, int kernel, hipStream_t stream) {
  if (!ctx->timing) return nullptr;
  (void)kernel;
  if (ctx->timed.size() >= kTimedCap) timing_fold(ctx, false);
  if (ctx->timed.size() >= kTimedCap) timing_fold(ctx, true);
  hipEvent_t e = timing_event(ctx);
  if (e) (void)hipEventRecord(e, stream ? stream : ctx->stream);
  return e;
}

void lf_timing_end(lf_ctx* ctx, int kernel, hipEvent_t start, hipStream_t stream) {
  if (!ctx->timing || !start) return;
  hipEvent_t e = timing_event(ctx);
  if (!e) { ctx->event_pool.push_back(start); return; }
  (void)hipEventRecord(e, stream ? stream : ctx->stream);
  ctx->timed.push_back(LfTimedLaunch{kernel, start, e});
}

namespace {

const char* kKernelNames[LFK_COUNT] = {"march", "flare_layer", "ghost_raster", "dft",
                                       "frame_setup", "tonemap", "exchange", "scene_term", "cull_prepass", "cull_audit",
                                       "cull_cache_build", "flare_visibility", "march_sensor", "sensor_table"};

// the reference's hard-coded prescription (pathtracer.cpp:541-556); literals narrowed to float
// where the reference narrows them
void default_paraxial_lens(LfParaxialLens& L) {
  static const double th[9] = {7.700, 1.850, 3.520, 1.850, 4.180, 3.000, 1.850, 7.270, 83.91};
  static const double rgb[3][9] = {{1.652, 1.5991, 1, 1.6396, 1, 1, 1.5776, 1.68990, 1},
                                   {1.652, 1.6113, 1, 1.65, 1, 1, 1.5885, 1.6999, 1},
                                   {1.652, 1.6164, 1, 1.6542, 1, 1, 1.5930, 1.7040, 1}};
  static const double radii[9] = {30.810, -89.350, 580.380, -80.630, 28.340, 0, 0, 32.190, -52.990};
  std::memset(&L, 0, sizeof(L));
  L.n = 9;
  L.stop = 5;
  for (int k = 0; k < 9; k++) {
    L.thickness[k] = (float)th[k];
    for (int c = 0; c < 3; c++) L.ior[c][k] = (float)rgb[c][k];
    L.curvature[k] = radii[k] == 0 ? 0.0f : (float)(1 / radii[k]);
  }
  L.clip = 11.6;
  L.recast_pos = 11.6f;
  L.recast_neg = -11.5f;
  L.marginal = 14.5f;
}

template <typename T>
lf_status dev_alloc(lf_ctx* ctx, T** p, size_t count) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
  if (count == 0) return LF_OK;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
  if (e != hipSuccess) return lf_fail(ctx, LF_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e));
  return LF_OK;
}

// std::mt19937 (util/random_util.h:10-14), written from the algorithm's definition
struct Mt19937 {
  uint32_t s[624];
  int idx;
  explicit Mt19937(uint32_t seed) {
    s[0] = seed;
    for (int i = 1; i < 624; i++) s[i] = 1812433253u * (s[i - 1] ^ (s[i - 1] >> 30)) + (uint32_t)i;
    idx = 624;
  }
  uint32_t next() {
    if (idx >= 624) {
      for (int k = 0; k < 624; k++) {
        uint32_t y = (s[k] & 0x80000000u) | (s[(k + 1) % 624] & 0x7fffffffu);
        s[k] = s[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      idx = 0;
    }
    uint32_t y = s[idx++];
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
  }
};

void free_frame_buffers(lf_ctx* ctx) {
  if (ctx->sample) (void)hipFree(ctx->sample);
  if (ctx->ghost) (void)hipFree(ctx->ghost);
  if (ctx->star) (void)hipFree(ctx->star);
  if (ctx->scene) (void)hipFree(ctx->scene);
  if (ctx->rgba) (void)hipFree(ctx->rgba);
  if (ctx->rgba_flip) (void)hipFree(ctx->rgba_flip);
  ctx->rgba_flip = nullptr;
  if (ctx->jitter_raw) (void)hipFree(ctx->jitter_raw);
  if (ctx->jitter_aa_raw) (void)hipFree(ctx->jitter_aa_raw);
  ctx->jitter_aa_raw = nullptr;
  if (ctx->accum) (void)hipFree(ctx->accum);  // sized by the frame
  ctx->accum = nullptr;
  ctx->sample = ctx->ghost = ctx->scene = ctx->star = nullptr;
  ctx->rgba = nullptr;
  ctx->jitter_raw = nullptr;
  ctx->jitter_table_valid = ctx->ghost_valid = ctx->sample_valid = false;
  ctx->rgba_y0 = ctx->rgba_y1 = 0;
}

lf_status upload_paraxial(lf_ctx* ctx) {
  LF_HIP(ctx, hipMemcpyAsync(ctx->pl_dev, &ctx->pl, sizeof(LfParaxialLens), hipMemcpyHostToDevice,
                             ctx->stream));
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LF_OK;
}

// how far from the centre the mask is open (a sampling parameter for lf_aim_at_exit_pupil, not pixel
// arithmetic): the far corner of the outermost texel > 0, as the march maps texels onto [-h, h]^2.  grow2 = 1
// (LF_MASK_BILINEAR): every open texel's footprint grown by half a texel on every side, [x - 0.5, x + 1.5]
double mask_open_radius(const float* texels, int width, int height, int grow2) {
  double r2max = 0.0;
  const double hw = 0.5 * width, hh = 0.5 * height, g = 0.5 * grow2;
  for (int y = 0; y < height; y++)
    for (int x = 0; x < width; x++)
      if (texels[(size_t)y * width + x] > 0.0f) {
        const double ex = std::max(std::fabs(x - g - hw), std::fabs(x + 1 + g - hw)) / hw;
        const double ey = std::max(std::fabs(y - g - hh), std::fabs(y + 1 + g - hh)) / hh;
        r2max = std::max(r2max, ex * ex + ey * ey);
      }
  return std::sqrt(r2max);
}

// What follows the stop mask AND how it is read (lf_set_aperture(STARBURST), lf_set_mask_filter): the open radius,
// the occupancy grid of the cull pre-pass, the support texture of the bilinear lookup; a resident cull table and
// the lens camera's calibration are stale.
lf_status derive_stop_mask(lf_ctx* ctx) {
  LfApertureDev& a = ctx->ap[LF_APERTURE_STARBURST];
  const int width = a.w, height = a.h;
  const float* texels = ctx->mask_host.data();
  const int grow2 = ctx->mask_filter == LF_MASK_BILINEAR ? 1 : 0;   // half texels the open footprint grows by
  a.open_radius = mask_open_radius(texels, width, height, grow2);
  // occupancy of the stop mask for the march's cull pre-pass (lf_cull_prepass.hip): which of kCullOcc x kCullOcc cells
  // of the mask holds a texel > 0 (a texel belongs to every cell it touches; in half-texel units under the filter)
  for (int r = 0; r < kCullOcc; r++) ctx->cull_occ[r] = 0u;
  const long long w2 = 2ll * width, h2 = 2ll * height;
  for (int y = 0; y < height; y++)
    for (int x = 0; x < width; x++)
      if (texels[(size_t)y * width + x] > 0.0f) {
        const long long xa = std::max(0ll, 2ll * x - grow2), xb = std::min(w2, 2ll * (x + 1) + grow2);
        const long long ya = std::max(0ll, 2ll * y - grow2), yb = std::min(h2, 2ll * (y + 1) + grow2);
        const int cx0 = (int)(xa * kCullOcc / w2), cx1 = (int)((xb * kCullOcc - 1) / w2);
        const int cy0 = (int)(ya * kCullOcc / h2), cy1 = (int)((yb * kCullOcc - 1) / h2);
        for (int cy = cy0; cy <= cy1 && cy < kCullOcc; cy++)
          for (int cx = cx0; cx <= cx1 && cx < kCullOcc; cx++) ctx->cull_occ[cy] |= 1u << cx;
      }
  ctx->mask_generation++;
  ctx->lenscam_dirty = true;   // the stop mask is part of the lens camera's exposure calibration
  if (grow2) return lfk_mask_support(ctx);
  return LF_OK;
}

}  // namespace

// host: the float constants of coated_fraction (lf_march_events.h) for one (interface, direction, wavelength)
void lf_coat_constants(float n, float m, float np, float thickness_nm, float lambda_nm, LfCoatK* c) {
  const float m2 = m * m, n2 = n * n, np2 = np * np;
  c->dm = m2 - n2;
  c->ph = (2.0f * thickness_nm) / lambda_nm;
  c->s01 = 1.0f / (n + m);
  c->s12 = 1.0f / (m + np);
  const float q1 = std::fmaf(m2, n, n2 * m), q2 = std::fmaf(np2, m, m2 * np);
  c->p01a = m2 / q1; c->p01b = n2 / q1;
  c->p12a = np2 / q2; c->p12b = m2 / q2;
}

// host: the record of stack_fraction (lf_march_events.h) for one (interface, direction, wavelength): lf_internal.h
void lf_stack_constants(float n, float np, int N, const float* m, const float* thickness_nm, float lambda_nm, float* out) {
  const float n2 = n * n;
  const int count = N;
  std::memcpy(&out[0], &count, sizeof(int));
  float mp = n;   // the medium in front of the layer
  for (int i = 0; i < N; i++) {
    const float mi = m[i], mi2 = mi * mi, mp2 = mp * mp;
    float* o = out + 1 + 5 * i;
    o[0] = mi2 - n2;
    o[1] = (2.0f * thickness_nm[i]) / lambda_nm;
    o[2] = 1.0f / (mp + mi);
    const float q = std::fmaf(mi2, mp, mp2 * mi);
    o[3] = mi2 / q; o[4] = mp2 / q;
    mp = mi;
  }
  const float mp2 = mp * mp, np2 = np * np;
  float* o = out + 1 + 5 * N;
  o[0] = 1.0f / (mp + np);
  const float q = std::fmaf(np2, mp, mp2 * np);
  o[1] = np2 / q; o[2] = mp2 / q;
}

void lf_stack_constants_of(const LfCoatings& C, int n_surfaces, int n_lambda, int surf, int l, bool plus_z, float n_in,
                           float n_out, float* out) {
  const int N = C.n_layers[surf];
  float m[LF_MAX_COAT_LAYERS], d[LF_MAX_COAT_LAYERS];
  for (int i = 0; i < N; i++) {
    const int j = plus_z ? i : N - 1 - i;   // layer 0 lies on the scene side: a ray travelling -z meets it last
    m[i] = C.layer_index[((size_t)j * n_lambda + l) * n_surfaces + surf];
    d[i] = C.layer_nm[(size_t)j * n_surfaces + surf];
  }
  lf_stack_constants(n_in, n_out, N, m, d, C.lambda_nm[l], out);
}

// ---- ghost occlusion: the state a shadow ray needs, and its device record (lf_set_ghost_occlusion below) -------------
// what a shadow ray needs installed: the prescription (the mapping's z_ref is its entrance pupil), the camera, a scene
lf_status lf_occlusion_ready(const lf_ctx* ctx, const char* who) {
  std::string missing;
  if (!ctx->lens_valid) missing += " a lens (lf_set_lens)";
  if (!ctx->cam_valid) missing += std::string(missing.empty() ? "" : ",") + " a camera (lf_set_camera)";
  if (!ctx->scene_valid || ctx->scene_dev.n_prims < 1)
    missing += std::string(missing.empty() ? "" : ",") + " a scene of at least one primitive (lf_set_scene / lf_load_collada)";
  if (missing.empty()) return LF_OK;
  return lf_fail(ctx, LF_ERR_STATE, std::string(who) + ": ghost occlusion needs" + missing);
}

// occlusion is on: a point light among the installed ones needs shadow rays that end at it (lf_set_ghost_occlusion_reach)
lf_status lf_occlusion_reach_ready(const lf_ctx* ctx, const char* who) {
  if (!lf_has_point_light(ctx->lens) || ctx->ghost_occl_reach == LF_OCCLUSION_REACH_LIGHT) return LF_OK;
  return lf_fail(ctx, LF_ERR_STATE, std::string(who) + ": ghost occlusion with a point light installed is not supported while the shadow rays "
                                    "run to the sky (a point light's shadow ray ends at the light) -- "
                                    "lf_set_ghost_occlusion_reach(LF_OCCLUSION_REACH_LIGHT) ends them there; or switch "
                                    "lf_set_ghost_occlusion off, or install directional lights only");
}

lf_status lf_fill_occlusion(const lf_ctx* ctx, double world_per_mm, LfOcclDev* o) {
  std::memset(o, 0, sizeof(*o));
  // the camera position is the centre of the paraxial entrance pupil at the reference wavelength, as the lens camera
  // has it (lf_lenscam_prepare: the same call on the same prescription)
  double z = 0.0, m = 1.0;
  if (ctx->raw_stop >= 0 &&
      lf_paraxial_entrance_pupil(ctx->raw_n, ctx->raw_stop, ctx->raw_radius, ctx->raw_thickness,
                                 ctx->raw_ior + (size_t)(ctx->lens.n_lambda / 2) * ctx->raw_n, &z, &m) != LF_OK)
    return lf_fail(ctx, LF_ERR_INVALID, "ghost occlusion: the stop has no finite paraxial image through the front group");
  o->nodes = ctx->scene_dev.nodes; o->prims = ctx->scene_dev.prims;
  o->stats = ctx->counters_dev + kMarchOcclSlot;
  std::memcpy(o->c2w, ctx->cam.c2w, sizeof(o->c2w));
  std::memcpy(o->pos, ctx->cam.pos, sizeof(o->pos));
  o->wpm = world_per_mm;
  o->z_ref = z;
  o->front_zv = ctx->lens.surf[0].zv;
  return LF_OK;
}

// ---- the lights of the march ("several lights", "point lights") ----------------------------------
// One light as lf_set_lights_ex validates it, host arithmetic only (lf_validate_light is this, exported): why = the
// refusal's message.  front_radius / front_semi_aperture: interface 0 of the prescription (a point light's limits are
// its r_f; have_front = false: no lens yet, a point light cannot be judged)
static lf_status validate_light(int kind, const float* v, const float* rad, float ar, bool have_front, float front_radius,
                                float front_semi_aperture, std::string* why) {
  if (kind != LF_LIGHT_DIRECTIONAL && kind != LF_LIGHT_POINT) {
    *why = "light: kind must be LF_LIGHT_DIRECTIONAL (0) or LF_LIGHT_POINT (1)";
    return LF_ERR_INVALID;
  }
  if (kind == LF_LIGHT_DIRECTIONAL) {
    const double n = std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
    if (!(n > 0) || !(v[2] < 0) || !(ar > 0) || ar > 1.5f) { *why = "sun: direction must have z < 0, 0 < angular radius <= 1.5"; return LF_ERR_INVALID; }
    for (int c = 0; c < 3; c++)   // unsigned fixed-point sums: see lf_set_lambda_rgb; any finite magnitude is fine (lf_march_fix_bits)
      if (!std::isfinite(rad[c]) || rad[c] < 0.0f || !std::isfinite(v[c])) { *why = "sun: radiance must be finite and >= 0, the direction finite"; return LF_ERR_INVALID; }
    return LF_OK;
  }
  if (!(ar > 0) || ar > 1.5f) { *why = "point light: 0 < angular radius <= 1.5"; return LF_ERR_INVALID; }
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(rad[c]) || rad[c] < 0.0f || !std::isfinite(v[c])) { *why = "point light: radiance must be finite and >= 0, the position finite"; return LF_ERR_INVALID; }
  if (!have_front) { *why = "point light: its distance limits are the front element's -- lf_set_lens comes first"; return LF_ERR_STATE; }
  const double r_f = lf_front_reach(front_radius, front_semi_aperture);
  const double dist = std::sqrt((double)v[0] * v[0] + (double)v[1] * v[1] + (double)v[2] * v[2]);
  if (!((double)v[2] <= -2.0 * r_f) || !(dist >= 4.0 * r_f)) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), "point light too close to the front element: position (%g, %g, %g) mm needs z <= -2 r_f = %g and "
                  "|L| >= 4 r_f = %g (r_f = %g mm, the front element's reach from its vertex)", v[0], v[1], v[2], -2.0 * r_f, 4.0 * r_f, r_f);
    *why = buf;
    return LF_ERR_INVALID;
  }
  return LF_OK;
}

// One light as lf_set_lights_geom validates it (lf_validate_light_geom is this, exported): g = LF_LIGHT_GEOM_FLOATS floats.
// Kinds 0 and 1 are lf_set_lights_ex's, on the first three floats; an area light: everything finite, a direction, a
// rectangle that is not degenerate, each of its four corners within the point light's limits.
static lf_status validate_light_geom(int kind, const float* g, const float* rad, float ar, bool have_front, float front_radius,
                                     float front_semi_aperture, std::string* why) {
  if (kind == LF_LIGHT_DIRECTIONAL || kind == LF_LIGHT_POINT)
    return validate_light(kind, g, rad, ar, have_front, front_radius, front_semi_aperture, why);
  if (kind != LF_LIGHT_AREA) {
    *why = "light: kind must be LF_LIGHT_DIRECTIONAL (0), LF_LIGHT_POINT (1) or LF_LIGHT_AREA (2)";
    return LF_ERR_INVALID;
  }
  for (int c = 0; c < LF_LIGHT_GEOM_FLOATS; c++)
    if (!std::isfinite(g[c])) { *why = "area light: radiance must be finite and >= 0, the geometry (centre, direction, dim_x, dim_y) finite"; return LF_ERR_INVALID; }
  for (int c = 0; c < 3; c++)
    if (!std::isfinite(rad[c]) || rad[c] < 0.0f) { *why = "area light: radiance must be finite and >= 0, the geometry (centre, direction, dim_x, dim_y) finite"; return LF_ERR_INVALID; }
  const double C[3] = {g[0], g[1], g[2]}, d[3] = {g[3], g[4], g[5]}, e1[3] = {g[6], g[7], g[8]}, e2[3] = {g[9], g[10], g[11]};
  if (!(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] > 0.0)) { *why = "area light: the direction must not be zero"; return LF_ERR_INVALID; }
  const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
  const double n1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), n2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
  if (!(n1 > 0.0) || !(n2 > 0.0) || !(std::sqrt(cx * cx + cy * cy + cz * cz) >= 1e-6 * n1 * n2)) {
    *why = "area light: degenerate rectangle -- |dim_x x dim_y| must be >= 1e-6 |dim_x| |dim_y|";
    return LF_ERR_INVALID;
  }
  if (!have_front) { *why = "area light: its distance limits are the front element's -- lf_set_lens comes first"; return LF_ERR_STATE; }
  const double r_f = lf_front_reach(front_radius, front_semi_aperture);
  for (int i = 0; i < 4; i++) {
    const double su = (i & 1) ? 0.5 : -0.5, sv = (i & 2) ? 0.5 : -0.5;
    const double p[3] = {C[0] + su * e1[0] + sv * e2[0], C[1] + su * e1[1] + sv * e2[1], C[2] + su * e1[2] + sv * e2[2]};
    const double dist = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    if (!(p[2] <= -2.0 * r_f) || !(dist >= 4.0 * r_f)) {
      char buf[320];
      std::snprintf(buf, sizeof(buf), "area light too close to the front element: corner (%g, %g, %g) mm needs z <= -2 r_f = %g and "
                    "|corner| >= 4 r_f = %g (r_f = %g mm, the front element's reach from its vertex)", p[0], p[1], p[2], -2.0 * r_f, 4.0 * r_f, r_f);
      *why = buf;
      return LF_ERR_INVALID;
    }
  }
  return LF_OK;
}

// the squared radius of an area light's bounding sphere, as its pre-test takes it (lf_area_pretest): the longer half
// diagonal's square, in double, 1e-6 larger and never rounded down
static float area_bound2(const float* e1, const float* e2) {
  double p = 0.0, m = 0.0;
  for (int c = 0; c < 3; c++) {
    const double a = (double)e1[c] + (double)e2[c], b = (double)e1[c] - (double)e2[c];
    p += a * a; m += b * b;
  }
  const double rb2 = 0.25 * std::max(p, m) * (1.0 + 1e-6);
  float f = (float)rb2;
  if ((double)f < rb2) f = std::nextafterf(f, INFINITY);
  return f;
}

void lf_area_cull_cone(const float* C, const float* g, double r_f, bool widen, float dir[3], float* rho) {
  const double c[3] = {C[0], C[1], C[2]}, e1[3] = {g[3], g[4], g[5]}, e2[3] = {g[6], g[7], g[8]};
  const double nc = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  const double u[3] = {c[0] / nc, c[1] / nc, c[2] / nc};
  for (int k = 0; k < 3; k++) dir[k] = (float)u[k];
  double chord = 0.0;
  for (int i = 0; i < 4; i++) {
    const double su = (i & 1) ? 0.5 : -0.5, sv = (i & 2) ? 0.5 : -0.5;
    const double p[3] = {c[0] + su * e1[0] + sv * e2[0], c[1] + su * e1[1] + sv * e2[1], c[2] + su * e1[2] + sv * e2[2]};
    const double np_ = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    const double dot = (p[0] * u[0] + p[1] * u[1] + p[2] * u[2]) / np_;
    // (a corner at 90 degrees or more from unit(C): the section is no longer convex -- every direction)
    if (!(dot > 0.0)) { chord = 2.0; break; }
    const double dx = p[0] / np_ - u[0], dy = p[1] / np_ - u[1], dz = p[2] / np_ - u[2];
    chord = std::max(chord, std::sqrt(dx * dx + dy * dy + dz * dz));
  }
  if (!widen) { *rho = (float)chord; return; }
  // dmin: the nearest point of C + s e1 + t e2, s, t in [-1/2, 1/2], to the origin -- the interior minimum if it lies
  // inside, else the least of the four edges' (each a clamped projection)
  const double a11 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], a22 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
  const double a12 = e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2];
  const double b1 = -(c[0] * e1[0] + c[1] * e1[1] + c[2] * e1[2]), b2 = -(c[0] * e2[0] + c[1] * e2[1] + c[2] * e2[2]);
  auto dist_at = [&](double s, double t) {
    const double p[3] = {c[0] + s * e1[0] + t * e2[0], c[1] + s * e1[1] + t * e2[1], c[2] + s * e1[2] + t * e2[2]};
    return std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
  };
  auto clamp = [](double x) { return x < -0.5 ? -0.5 : x > 0.5 ? 0.5 : x; };
  double dmin = INFINITY;
  const double den = a11 * a22 - a12 * a12;
  if (den > 0.0) {
    const double s = (b1 * a22 - b2 * a12) / den, t = (b2 * a11 - b1 * a12) / den;
    if (std::fabs(s) <= 0.5 && std::fabs(t) <= 0.5) dmin = dist_at(s, t);
  }
  if (!std::isfinite(dmin)) {
    for (int i = 0; i < 2; i++) {
      const double f = i ? 0.5 : -0.5;
      dmin = std::min(dmin, dist_at(clamp((b1 - f * a12) / a11), f));   // t = f: minimise over s
      dmin = std::min(dmin, dist_at(f, clamp((b2 - f * a12) / a22)));   // s = f: minimise over t
    }
  }
  *rho = (float)chord + lf_cull_near_widening(r_f, dmin);
}

// the installed point and area lights against the front element of the lens as it is now (a launch's precondition: lf_march.hip)
lf_status lf_point_lights_fit(const lf_ctx* ctx, const char* who) {
  const LfLensDev& L = ctx->lens;
  for (int k = 0; k < L.n_lights; k++) {
    if (L.light_kind[k] == LF_LIGHT_DIRECTIONAL) continue;
    std::string why;
    if (L.light_kind[k] == LF_LIGHT_AREA) {
      float g[LF_LIGHT_GEOM_FLOATS];
      for (int c = 0; c < 3; c++) g[c] = L.light_pos[k][c];
      for (int c = 0; c < 9; c++) g[3 + c] = L.light_area[k][c];
      if (validate_light_geom(LF_LIGHT_AREA, g, L.light_radiance[k], 0.0f, ctx->lens_valid, ctx->raw_radius[0], ctx->raw_semi_ap[0], &why) != LF_OK)
        return lf_fail(ctx, LF_ERR_STATE, std::string(who) + ": light " + std::to_string(k) + " no longer fits the lens installed since -- " + why);
      continue;
    }
    if (validate_light(LF_LIGHT_POINT, L.light_pos[k], L.light_radiance[k], ctx->light_radius[k], ctx->lens_valid, ctx->raw_radius[0],
                       ctx->raw_semi_ap[0], &why) != LF_OK)
      return lf_fail(ctx, LF_ERR_STATE, std::string(who) + ": light " + std::to_string(k) + " no longer fits the lens installed since -- " + why);
  }
  return LF_OK;
}

extern "C" {

int lf_abi_version(void) { return LF_ABI_VERSION; }

const char* lf_last_error(const lf_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

// lf_test_knob's process-wide defaults (see there)
static std::mutex g_knob_mu;
static std::vector<std::pair<std::string, double>> g_knob_defaults;

lf_status lf_create(lf_ctx** out, int device) {
  if (!out) return LF_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return LF_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return LF_ERR_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return LF_ERR_NO_DEVICE;
  {
    // the library carries gfx950 code objects only: any other architecture would fail at the first
    // launch with an opaque HIP error (LF_ALLOW_ANY_ARCH=1: for experiments with a fat binary)
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return LF_ERR_NO_DEVICE;
    bool any_arch = false;
#ifdef LF_EXPERIMENTS
    any_arch = std::getenv("LF_ALLOW_ANY_ARCH") != nullptr;
#endif
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0 && !any_arch) return LF_ERR_NO_DEVICE;
  }
  lf_ctx* ctx = new lf_ctx();
  ctx->device = device;
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return LF_ERR_HIP;
  }
  ctx->own_stream = true;
#ifdef LF_EXPERIMENTS
  // (changes the sampling pattern; the oracles / tests use the default, 6)
  if (const char* sb = std::getenv("LF_MARCH_SUB_BITS")) {
    int v = std::atoi(sb);
    if (v >= 0 && v <= kMaxSubcellBits) ctx->march_sub_bits = v;
  }
#endif
  default_paraxial_lens(ctx->pl);
  bool ok = hipMalloc((void**)&ctx->flares, sizeof(LfFlares)) == hipSuccess &&
            hipMalloc((void**)&ctx->ghosts, sizeof(LfGhostList)) == hipSuccess &&
            hipMalloc((void**)&ctx->pl_dev, sizeof(LfParaxialLens)) == hipSuccess &&
            hipMalloc((void**)&ctx->lens_dev, kLensDevBytes) == hipSuccess &&
            hipMalloc((void**)&ctx->pairs_dev, sizeof(LfPairsDev)) == hipSuccess &&
            hipMalloc((void**)&ctx->counters_dev, kMarchCounterSlots * sizeof(unsigned long long)) == hipSuccess &&
            hipMalloc((void**)&ctx->scene_counters_dev, kSceneCounters * sizeof(unsigned long long)) == hipSuccess &&
            hipMalloc((void**)&ctx->primary_dev, sizeof(LfPrimaryDev) + kPrimaryStackBytes) == hipSuccess;
  for (int s = 0; s < 2 && ok; s++)
    ok = hipMalloc((void**)&ctx->ap[s].stats, sizeof(lf_aperture_stats)) == hipSuccess;
  if (!ok) { lf_destroy(ctx); return LF_ERR_OOM; }
  (void)hipMemset(ctx->flares, 0, sizeof(LfFlares));
  (void)hipMemset(ctx->ghosts, 0, sizeof(LfGhostList));
  (void)hipMemset(ctx->counters_dev, 0, kMarchCounterSlots * sizeof(unsigned long long));
  (void)hipMemset(ctx->scene_counters_dev, 0, kSceneCounters * sizeof(unsigned long long));
  if (upload_paraxial(ctx) != LF_OK) { lf_destroy(ctx); return LF_ERR_HIP; }
  {
    std::vector<std::pair<std::string, double>> defaults;
    { std::lock_guard<std::mutex> lock(g_knob_mu); defaults = g_knob_defaults; }
    for (const auto& kv : defaults) (void)lf_test_knob(ctx, kv.first.c_str(), kv.second);
  }
  *out = ctx;
  return LF_OK;
}

lf_status lf_destroy(lf_ctx* ctx) {
  if (!ctx) return LF_ERR_INVALID;
  // a communicator call the host gave up on (lf_comm_poison) may still be blocked in another thread, standing on
  // this context: nothing is freed then -- the context is LEAKED on purpose (the process is on its way out anyway)
  if (ctx->comm_poisoned.load() && ctx->comm_busy.load() > 0) return LF_ERR_STATE;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  (void)lf_comm_destroy(ctx);
  if (ctx->comm_stage) (void)hipFree(ctx->comm_stage);
  free_frame_buffers(ctx);
  lf_cull_cache_free(ctx);
  lf_flare_occlusion_free(ctx);
  lf_sensor_free(ctx);
  for (auto& t : ctx->timed) { (void)hipEventDestroy(t.start); (void)hipEventDestroy(t.stop); }
  for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
  for (int s = 0; s < 2; s++) {
    if (ctx->ap[s].texels) (void)hipFree(ctx->ap[s].texels);
    if (ctx->ap[s].stats) (void)hipFree(ctx->ap[s].stats);
  }
  void* ptrs[] = {ctx->spectrum, ctx->twiddle, ctx->dft_rows, ctx->flares, ctx->ghosts, ctx->pl_dev,
                  ctx->lens_dev, ctx->pairs_dev, ctx->counters_dev, ctx->accum,
                  ctx->prog_dev, ctx->sun_lights_dev,
                  ctx->scene_dev.nodes, ctx->scene_dev.prims, ctx->scene_dev.normals, ctx->scene_dev.materials,
                  ctx->scene_dev.lights, ctx->env_block, ctx->probe_dev, ctx->scene_counters_dev,
                  ctx->primary_dev, ctx->primary_surf_dev, ctx->cull_dev, ctx->cull_lists.list[0], ctx->cull_lists.list[1], ctx->cull_counts, ctx->cull_popc_dev,
                  ctx->tail_acc, ctx->tail_done};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return LF_OK;
}

lf_status lf_set_stream(lf_ctx* ctx, void* hip_stream) {
  if (!ctx) return LF_ERR_INVALID;
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
  ctx->stream = reinterpret_cast<hipStream_t>(hip_stream);
  ctx->own_stream = false;
  return LF_OK;
}

lf_status lf_synchronize(lf_ctx* ctx) {
  if (!ctx) return LF_ERR_INVALID;
  lf_status js = lf_comm_join(ctx);   // an exchange still running on the second stream
  if (js != LF_OK) return js;
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LF_OK;
}

// (re)allocate the frame-sized buffers for `rows` rows; content is lost
static lf_status alloc_frame_buffers(lf_ctx* ctx, int rows) {
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->comm_stream) { LF_HIP(ctx, hipStreamSynchronize(ctx->comm_stream)); ctx->comm_pending = false; }
  free_frame_buffers(ctx);
  ctx->H_alloc = rows;
  size_t n = (size_t)ctx->W * ctx->H_alloc;
  lf_status st;
  if ((st = dev_alloc(ctx, &ctx->sample, 3 * n)) != LF_OK) return st;
  if ((st = dev_alloc(ctx, &ctx->ghost, 3 * n)) != LF_OK) return st;
  if ((st = dev_alloc(ctx, &ctx->star, 3 * n)) != LF_OK) return st;
  if ((st = dev_alloc(ctx, &ctx->rgba, n)) != LF_OK) return st;
  LF_HIP(ctx, hipMemsetAsync(ctx->sample, 0, 3 * n * sizeof(double), ctx->stream));
  LF_HIP(ctx, hipMemsetAsync(ctx->ghost, 0, 3 * n * sizeof(double), ctx->stream));
  LF_HIP(ctx, hipMemsetAsync(ctx->star, 0, 3 * n * sizeof(double), ctx->stream));
  LF_HIP(ctx, hipMemsetAsync(ctx->rgba, 0, n * sizeof(uint32_t), ctx->stream));
  return LF_OK;
}

// rows the frame buffers need so that every group of `period` 8-row tile rows is addressable
// (the tile-row exchange of lf_gather / sharding.py views the frame as [groups][period][tile row])
static int padded_rows(int H, int period) {
  const int ntrows = (H + 7) / 8;
  return (ntrows + period - 1) / period * period * 8;
}

lf_status lf_set_frame(lf_ctx* ctx, int width, int height) {
  if (!ctx) return LF_ERR_INVALID;
  if (width <= 0 || height <= 0 || width > (1 << 15) || height > (1 << 15))
    return lf_fail(ctx, LF_ERR_INVALID, "frame size out of range");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  ctx->W = width; ctx->H = height; ctx->y0 = 0; ctx->y1 = height;
  lf_install_split(ctx, ctx->split.with_deal(LfSplit::kRows, 0, 1));    // the whole frame (a table share set before stays)
  // padded for every interleave period up to 8 (ceil(n/p) p <= n + p - 1); larger periods
  // re-allocate in lf_set_row_interleave
  return alloc_frame_buffers(ctx, ((height + 7) / 8 + 7) * 8);
}

lf_status lf_set_band(lf_ctx* ctx, int y0, int y1) {
  if (!ctx) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_set_band before lf_set_frame");
  if (y0 < 0 || y1 > ctx->H || y0 > y1) return lf_fail(ctx, LF_ERR_INVALID, "band out of range");
  ctx->y0 = y0; ctx->y1 = y1;
  return LF_OK;
}

lf_status lf_set_row_interleave(lf_ctx* ctx, int phase, int period) {
  if (!ctx) return LF_ERR_INVALID;
  if (period < 1 || phase < 0 || phase >= period)
    return lf_fail(ctx, LF_ERR_INVALID, "row interleave: need 0 <= phase < period");
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_set_row_interleave before lf_set_frame");
  if (padded_rows(ctx->H, period) > ctx->H_alloc) {
    // the tile-row exchange needs ceil(tile rows / period) * period tile rows: grow the buffers
    // (their content is lost -- set the interleave before rendering)
    LF_HIP(ctx, hipSetDevice(ctx->device));
    lf_status st = alloc_frame_buffers(ctx, padded_rows(ctx->H, period));
    if (st != LF_OK) return st;
  }
  lf_install_split(ctx, ctx->split.with_deal(LfSplit::kRows, phase, period));
  return LF_OK;
}

// The frame dealt by BLOCKS of 64 x 64 pixels (round 6): block b (row-major) belongs to rank b % nranks.  The block is the
// cull table's, so a rank's march reads only the table rows its own pre-pass wrote: the pre-pass, its audit and the march
// all shrink with the number of ranks and no table crosses a link.
lf_status lf_set_block_deal(lf_ctx* ctx, int rank, int nranks) {
  if (!ctx) return LF_ERR_INVALID;
  if (nranks < 1 || nranks > 64 || rank < 0 || rank >= nranks) return lf_fail(ctx, LF_ERR_INVALID, "block deal: need 0 <= rank < nranks <= 64");
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_set_block_deal before lf_set_frame");
  if (ctx->split.table != LfSplit::kOwn)
    return lf_fail(ctx, LF_ERR_STATE, "lf_set_block_deal: the cull table is shared between ranks (lf_comm_share_cull / lf_set_cull_share): "
                                      "a frame dealt by blocks shares nothing");
  lf_install_split(ctx, ctx->split.with_deal(nranks > 1 ? LfSplit::kBlocks : LfSplit::kRows, rank, nranks));   // (1: the whole frame)
  return LF_OK;
}

lf_status lf_set_params(lf_ctx* ctx, int ns_aa, double flare_radius, double flare_intensity) {
  if (!ctx || ns_aa < 0) return LF_ERR_INVALID;
  ctx->ns_aa = ns_aa;
  ctx->flare_radius = flare_radius;
  ctx->flare_intensity = flare_intensity;
  return LF_OK;
}

lf_status lf_set_flare_arithmetic(lf_ctx* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 2) return LF_ERR_INVALID;
  ctx->flare_arithmetic = mode;
  return LF_OK;
}

lf_status lf_set_aperture(lf_ctx* ctx, lf_aperture_slot slot, const float* texels, int width,
                          int height) {
  if (!ctx || !texels || (slot != LF_APERTURE_STARBURST && slot != LF_APERTURE_GHOST))
    return LF_ERR_INVALID;
  if (width <= 0 || height <= 0 || width > 4096 || height > 4096)
    return lf_fail(ctx, LF_ERR_INVALID, "aperture size out of range (1..4096)");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  LfApertureDev& a = ctx->ap[slot];
  a.valid = false;
  lf_status st;
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));  // kernels in flight may read the old texels / spectrum
  // (the stop mask's slot keeps room for its support texture, 2 w x 2 h, behind the texels: lf_set_mask_filter)
  if ((st = dev_alloc(ctx, &a.texels, (size_t)width * height * (slot == LF_APERTURE_STARBURST ? 5 : 1))) != LF_OK) return st;
  a.w = width; a.h = height;
  LF_HIP(ctx, hipMemcpyAsync(a.texels, texels, sizeof(float) * (size_t)width * height,
                             hipMemcpyHostToDevice, ctx->stream));
  if ((st = lfk_aperture_stats(ctx, slot)) != LF_OK) return st;
  a.valid = true;
  if (slot != LF_APERTURE_STARBURST) {
    a.open_radius = mask_open_radius(texels, width, height, 0);
  } else {
    ctx->mask_host.assign(texels, texels + (size_t)width * height);
    if ((st = derive_stop_mask(ctx)) != LF_OK) { a.valid = false; return st; }
    ctx->spectrum_valid = false;
    size_t rows = a.host_stats.max_y >= a.host_stats.min_y
                      ? (size_t)(a.host_stats.max_y - a.host_stats.min_y + 1) : 1;
    if ((st = dev_alloc(ctx, &ctx->spectrum, (size_t)width * width)) != LF_OK) return st;
    if ((st = dev_alloc(ctx, &ctx->twiddle, (size_t)width)) != LF_OK) return st;
    if ((st = dev_alloc(ctx, &ctx->dft_rows, rows * width)) != LF_OK) return st;
    if ((st = lfk_build_spectrum(ctx)) != LF_OK) return st;
  }
  return LF_OK;
}

lf_status lf_get_aperture_stats(lf_ctx* ctx, lf_aperture_slot slot, lf_aperture_stats* out) {
  if (!ctx || !out || (slot != 0 && slot != 1)) return LF_ERR_INVALID;
  if (!ctx->ap[slot].valid) return lf_fail(ctx, LF_ERR_STATE, "aperture not set");
  *out = ctx->ap[slot].host_stats;
  return LF_OK;
}

lf_status lf_set_paraxial_lens(lf_ctx* ctx, int n, int stop_index, const float* thickness,
                               const float* curvature, const float* ior_rgb) {
  if (!ctx) return LF_ERR_INVALID;
  if (!thickness || !curvature || !ior_rgb) {
    default_paraxial_lens(ctx->pl);
  } else {
    if (n < 2 || n > LF_MAX_SURFACES || stop_index < 0 || stop_index >= n)
      return lf_fail(ctx, LF_ERR_INVALID, "paraxial lens: bad n / stop index");
    LfParaxialLens L;
    default_paraxial_lens(L);
    L.n = n; L.stop = stop_index;
    for (int k = 0; k < n; k++) {
      L.thickness[k] = thickness[k];
      L.curvature[k] = curvature[k];
      for (int c = 0; c < 3; c++) L.ior[c][k] = ior_rgb[c * n + k];
    }
    ctx->pl = L;
  }
  ctx->ghost_valid = false;
  return upload_paraxial(ctx);
}

lf_status lf_set_camera(lf_ctx* ctx, const double c2w[9], const double pos[3], double hfov_deg,
                        double vfov_deg) {
  if (!ctx || !c2w || !pos) return LF_ERR_INVALID;
  std::memcpy(ctx->cam.c2w, c2w, 9 * sizeof(double));
  std::memcpy(ctx->cam.pos, pos, 3 * sizeof(double));
  ctx->cam.hfov_deg = hfov_deg;
  ctx->cam.vfov_deg = vfov_deg;
  ctx->cam_valid = true;
  return LF_OK;
}

lf_status lf_find_sun_pos(lf_ctx* ctx, const double* lights, int n_lights) {
  if (!ctx || n_lights < 0 || (n_lights > 0 && !lights)) return LF_ERR_INVALID;
  if (!ctx->cam_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_find_sun_pos before lf_set_camera");
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_find_sun_pos before lf_set_frame");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  // flare_origins.clear(); flare_radiance.clear() (raytraced_renderer.cpp:306-307); axis_ray and
  // angle_to_sun keep their previous values, exactly like the reference's members.
  // The lights travel as kernel arguments (no allocation, no copy, no synchronisation per frame);
  // only a scene with more than kMaxSunLightArgs directional lights takes the staged path.
  if (n_lights <= kMaxSunLightArgs) {
    LfSunLightArgs args;
    std::memset(&args, 0, sizeof(args));
    if (n_lights > 0) std::memcpy(args.v, lights, sizeof(double) * 6 * (size_t)n_lights);
    lf_status st = lfk_frame_setup(ctx, &args, nullptr, n_lights, true);
    if (st != LF_OK) return st;
  } else {
    if ((size_t)n_lights > ctx->sun_lights_cap) {
      LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (ctx->sun_lights_dev) (void)hipFree(ctx->sun_lights_dev);
      ctx->sun_lights_dev = nullptr; ctx->sun_lights_cap = 0;
      LF_HIP(ctx, hipMalloc((void**)&ctx->sun_lights_dev, sizeof(double) * 6 * (size_t)n_lights));
      ctx->sun_lights_cap = (size_t)n_lights;
    }
    LF_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the previous frame may still read the buffer
    LF_HIP(ctx, hipMemcpy(ctx->sun_lights_dev, lights, sizeof(double) * 6 * (size_t)n_lights,
                          hipMemcpyHostToDevice));
    lf_status st = lfk_frame_setup(ctx, nullptr, ctx->sun_lights_dev, n_lights, true);
    if (st != LF_OK) return st;
  }
  ctx->flares_n_host = -1;   // (counted by the kernel)
  ctx->flares_valid = true;
  ctx->ghost_valid = false;
  return LF_OK;
}

lf_status lf_set_flares(lf_ctx* ctx, int n, const double* origins, const double* radiance,
                        const double axis_ray[2], float angle_to_sun) {
  if (!ctx || n < 0 || n > LF_MAX_FLARES || (n > 0 && (!origins || !radiance)) || !axis_ray)
    return LF_ERR_INVALID;
  LfFlares f;
  std::memset(&f, 0, sizeof(f));
  f.n_flares = n;
  f.n_in_frame = n;
  f.angle_to_sun = angle_to_sun;
  for (int k = 0; k < n; k++) {
    f.origin[k][0] = origins[2 * k]; f.origin[k][1] = origins[2 * k + 1];
    for (int c = 0; c < 3; c++) f.radiance[k][c] = radiance[3 * k + c];
  }
  f.axis_ray[0] = axis_ray[0]; f.axis_ray[1] = axis_ray[1];
  LF_HIP(ctx, hipMemcpyAsync(ctx->flares, &f, sizeof(f), hipMemcpyHostToDevice, ctx->stream));
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->flares_n_host = n;
  ctx->flares_valid = true;
  ctx->ghost_valid = false;
  return LF_OK;
}

lf_status lf_get_flares(lf_ctx* ctx, int* n, double* origins, double* radiance, double axis_ray[2],
                        float* angle_to_sun) {
  if (!ctx || !n) return LF_ERR_INVALID;
  LfFlares f;
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LF_HIP(ctx, hipMemcpy(&f, ctx->flares, sizeof(f), hipMemcpyDeviceToHost));
  *n = f.n_flares;
  for (int k = 0; k < f.n_flares; k++) {
    if (origins) { origins[2 * k] = f.origin[k][0]; origins[2 * k + 1] = f.origin[k][1]; }
    if (radiance) for (int c = 0; c < 3; c++) radiance[3 * k + c] = f.radiance[k][c];
  }
  if (axis_ray) { axis_ray[0] = f.axis_ray[0]; axis_ray[1] = f.axis_ray[1]; }
  if (angle_to_sun) *angle_to_sun = f.angle_to_sun;
  return LF_OK;
}

lf_status lf_set_jitter_mt19937(lf_ctx* ctx, uint32_t seed, const uint32_t* order, size_t n_order) {
  if (!ctx) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_set_jitter_mt19937 before lf_set_frame");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)ctx->W * ctx->H;
  std::vector<uint32_t> own;
  if (!order) {  // the reference's tile queue: 32x32 tiles, y-major; pixels y-major inside a tile
    own.reserve(n);
    const int T = 32;
    for (int ty = 0; ty < ctx->H; ty += T)
      for (int tx = 0; tx < ctx->W; tx += T)
        for (int y = ty; y < std::min(ty + T, ctx->H); y++)
          for (int x = tx; x < std::min(tx + T, ctx->W); x++)
            own.push_back((uint32_t)(x + y * ctx->W));
    order = own.data();
    n_order = own.size();
  }
  // Each visited pixel consumes 2*ns_aa draws (pixel jitter, pathtracer.cpp:844) and then the 32
  // draws of calculate_irradiance_falloff (:1050).  Only the latter reach the device, stored
  // pixel-major; a pixel visited twice keeps its last visit, like the reference's buffer.
  std::vector<uint32_t> table(n * 32, 0u);
  const size_t naa = 2 * (size_t)ctx->ns_aa;
  std::vector<uint32_t> aa(n * naa, 0u);
  Mt19937 mt(seed);
  for (size_t v = 0; v < n_order; v++) {
    if (order[v] >= n) return lf_fail(ctx, LF_ERR_INVALID, "visit order: pixel index out of range");
    uint32_t* da = aa.data() + (size_t)order[v] * naa;
    for (size_t k = 0; k < naa; k++) da[k] = mt.next();   // consumed by the scene-term kernel
    uint32_t* dst = table.data() + (size_t)order[v] * 32;
    for (int k = 0; k < 32; k++) dst[k] = mt.next();
  }
  lf_status st;
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a running flare layer may read the old tables
  if ((st = dev_alloc(ctx, &ctx->jitter_raw, n * 32)) != LF_OK) return st;
  LF_HIP(ctx, hipMemcpy(ctx->jitter_raw, table.data(), table.size() * sizeof(uint32_t),
                        hipMemcpyHostToDevice));
  if ((st = dev_alloc(ctx, &ctx->jitter_aa_raw, n * naa)) != LF_OK) return st;
  if (naa)
    LF_HIP(ctx, hipMemcpy(ctx->jitter_aa_raw, aa.data(), aa.size() * sizeof(uint32_t),
                          hipMemcpyHostToDevice));
  ctx->jitter_aa_ns = ctx->ns_aa;
  ctx->jitter_mode = 0;
  ctx->jitter_table_valid = true;
  return LF_OK;
}

lf_status lf_set_jitter_counter(lf_ctx* ctx, uint64_t key) {
  if (!ctx) return LF_ERR_INVALID;
  ctx->jitter_mode = 1;
  ctx->jitter_key = key;
  return LF_OK;
}

lf_status lf_set_scene_term(lf_ctx* ctx, const double* rgb) {
  if (!ctx) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_set_scene_term before lf_set_frame");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  size_t n = (size_t)ctx->W * ctx->H * 3;
  if (!rgb) {
    if (ctx->scene) { LF_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->scene); }
    ctx->scene = nullptr;
    return LF_OK;
  }
  lf_status st;
  if (!ctx->scene && (st = dev_alloc(ctx, &ctx->scene, n)) != LF_OK) return st;
  // the context's stream is non-blocking: a null-stream copy is NOT ordered behind a flare layer
  // that still reads the previous scene term
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LF_HIP(ctx, hipMemcpy(ctx->scene, rgb, n * sizeof(double), hipMemcpyHostToDevice));
  return LF_OK;
}

lf_status lf_generate_ghost_buffer(lf_ctx* ctx) {
  if (!ctx) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_generate_ghost_buffer before lf_set_frame");
  if (!ctx->flares_valid) return lf_fail(ctx, LF_ERR_STATE, "no flare state: call lf_find_sun_pos or lf_set_flares");
  if (!ctx->ap[LF_APERTURE_GHOST].valid) return lf_fail(ctx, LF_ERR_STATE, "ghost aperture not set");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  lf_status st;
  if ((st = lfk_frame_setup(ctx, nullptr, nullptr, 0, false)) != LF_OK) return st;
  // (lf_set_flare_occlusion: the quads' colours times the visibility of the flare that supplied axis_ray; off: the list itself)
  const LfGhostList* gl = nullptr;
  if ((st = lf_flare_occlusion_update(ctx, "lf_generate_ghost_buffer", nullptr, &gl)) != LF_OK) return st;
  if ((st = lfk_ghost_raster(ctx, gl)) != LF_OK) return st;
  ctx->ghost_valid = true;
  return LF_OK;
}

lf_status lf_render_flare_layer(lf_ctx* ctx) {
  if (!ctx) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_render_flare_layer before lf_set_frame");
  if (!ctx->flares_valid) return lf_fail(ctx, LF_ERR_STATE, "no flare state: call lf_find_sun_pos or lf_set_flares");
  if (!ctx->ap[LF_APERTURE_STARBURST].valid || !ctx->spectrum_valid)
    return lf_fail(ctx, LF_ERR_STATE, "starburst aperture not set");
  if (ctx->jitter_mode == 0 && !ctx->jitter_table_valid)
    return lf_fail(ctx, LF_ERR_STATE, "MT19937 jitter selected but no table (frame was resized?)");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  lf_status st;
  // (lf_set_flare_occlusion: the effective flare record, radiance times visibility; off: the installed one)
  const LfFlares* fl = nullptr;
  if ((st = lf_flare_occlusion_update(ctx, "lf_render_flare_layer", &fl, nullptr)) != LF_OK) return st;
  if ((st = lfk_flare_layer(ctx, fl)) != LF_OK) return st;
  ctx->sample_valid = true;
  ctx->rgba_y0 = ctx->rgba_y1 = 0;  // the tonemapped copy is stale
  return LF_OK;
}

lf_status lf_read_tile(lf_ctx* ctx, int which, int x0, int y0, int x1, int y1, double* dst,
                       size_t pixel_stride) {
  if (!ctx || !dst || which < 0 || which > 3 || pixel_stride < 3) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_read_tile before lf_set_frame");
  if (which == 3 && !ctx->scene)
    return lf_fail(ctx, LF_ERR_STATE, "lf_read_tile(LF_SCENE_BUFFER) before lf_render_scene_term / lf_set_scene_term");
  if (x0 < 0 || y0 < 0 || x1 > ctx->W || y1 > ctx->H || x0 > x1 || y0 > y1)
    return lf_fail(ctx, LF_ERR_INVALID, "tile out of range");
  if (x0 == x1 || y0 == y1) return LF_OK;
  const double* src = which == 0 ? ctx->sample : which == 1 ? ctx->ghost : which == 2 ? ctx->star : ctx->scene;
  { const lf_status js = lf_comm_join(ctx); if (js != LF_OK) return js; }
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const size_t tw = (size_t)(x1 - x0);
  if (pixel_stride == 3) {
    LF_HIP(ctx, hipMemcpy2D(dst, tw * 3 * sizeof(double), src + 3 * ((size_t)y0 * ctx->W + x0),
                            (size_t)ctx->W * 3 * sizeof(double), tw * 3 * sizeof(double),
                            (size_t)(y1 - y0), hipMemcpyDeviceToHost));
  } else {
    std::vector<double> tmp(tw * 3 * (size_t)(y1 - y0));
    LF_HIP(ctx, hipMemcpy2D(tmp.data(), tw * 3 * sizeof(double),
                            src + 3 * ((size_t)y0 * ctx->W + x0), (size_t)ctx->W * 3 * sizeof(double),
                            tw * 3 * sizeof(double), (size_t)(y1 - y0), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tw * (size_t)(y1 - y0); i++)
      for (int c = 0; c < 3; c++) dst[i * pixel_stride + c] = tmp[3 * i + c];
  }
  return LF_OK;
}

lf_status lf_read_pixel(lf_ctx* ctx, int which, int x, int y, double rgb[3]) {
  return lf_read_tile(ctx, which, x, y, x + 1, y + 1, rgb, 3);
}

lf_status lf_write_to_framebuffer(lf_ctx* ctx, int x0, int y0, int x1, int y1, uint32_t* dst,
                                  size_t row_stride) {
  if (!ctx || !dst) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_write_to_framebuffer before lf_set_frame");
  if (x0 < 0 || y0 < 0 || x1 > ctx->W || y1 > ctx->H || x0 > x1 || y0 > y1)
    return lf_fail(ctx, LF_ERR_INVALID, "tile out of range");
  if (row_stride < (size_t)(x1 - x0)) return lf_fail(ctx, LF_ERR_INVALID, "row_stride < tile width");
  if (x0 == x1 || y0 == y1) return LF_OK;
  LF_HIP(ctx, hipSetDevice(ctx->device));
  { const lf_status js = lf_comm_join(ctx); if (js != LF_OK) return js; }
  if (y0 < ctx->rgba_y0 || y1 > ctx->rgba_y1) {
    // tonemap the current band and whatever else the tile needs (the reference tonemaps exactly
    // the tile, image.h:208-223; whole rows keep the launch simple), remember the rows done
    const int ya = std::min(y0, ctx->y0 < ctx->y1 ? ctx->y0 : y0);
    const int yb = std::max(y1, ctx->y0 < ctx->y1 ? ctx->y1 : y1);
    lf_status st = lfk_tonemap(ctx, ya, yb);
    if (st != LF_OK) return st;
    ctx->rgba_y0 = ya; ctx->rgba_y1 = yb;
  }
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LF_HIP(ctx, hipMemcpy2D(dst, row_stride * sizeof(uint32_t), ctx->rgba + (size_t)y0 * ctx->W + x0,
                          (size_t)ctx->W * sizeof(uint32_t), (size_t)(x1 - x0) * sizeof(uint32_t),
                          (size_t)(y1 - y0), hipMemcpyDeviceToHost));
  return LF_OK;
}

lf_status lf_save_image_rgba(lf_ctx* ctx, uint32_t* dst) {
  if (!ctx || !dst) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_save_image_rgba before lf_set_frame");
  if (!ctx->sample_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_save_image_rgba before lf_render_flare_layer");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  { const lf_status js = lf_comm_join(ctx); if (js != LF_OK) return js; }
  lf_status st = lfk_tonemap(ctx, 0, ctx->H);   // the saved image is always the whole frame
  if (st != LF_OK) return st;
  ctx->rgba_y0 = 0; ctx->rgba_y1 = ctx->H;
  const size_t n = (size_t)ctx->W * ctx->H;
  if (!ctx->rgba_flip) LF_HIP(ctx, hipMalloc((void**)&ctx->rgba_flip, n * sizeof(uint32_t)));
  st = lfk_flip_rows(ctx, ctx->rgba_flip);
  if (st != LF_OK) return st;
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LF_HIP(ctx, hipMemcpy(dst, ctx->rgba_flip, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return LF_OK;
}

lf_status lf_device_buffer(lf_ctx* ctx, int which, void** dptr, size_t* bytes) {
  if (!ctx || !dptr || which < 0 || which > 2) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_device_buffer before lf_set_frame");
  *dptr = which == 0 ? ctx->sample : which == 1 ? ctx->ghost : ctx->star;
  if (bytes) *bytes = (size_t)ctx->W * ctx->H_alloc * 3 * sizeof(double);
  return LF_OK;
}

// ---------------------------------------------------------------- geometric lens -------------
lf_status lf_set_lens(lf_ctx* ctx, int n_surfaces, int stop_index, int n_lambda,
                      const float* radius, const float* thickness, const float* ior,
                      const float* semi_aperture, float sensor_width_mm) {
  if (!ctx || !radius || !thickness || !ior || !semi_aperture) return LF_ERR_INVALID;
  if (n_surfaces < 1 || n_surfaces > LF_MAX_SURFACES || n_lambda < 1 || n_lambda > LF_MAX_LAMBDA ||
      stop_index < -1 || stop_index >= n_surfaces || !(sensor_width_mm > 0))
    return lf_fail(ctx, LF_ERR_INVALID, "lens: bad sizes");
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_set_lens before lf_set_frame");
  for (int k = 0; k < n_surfaces; k++) {
    if (!(semi_aperture[k] > 0) || !std::isfinite(semi_aperture[k]))
      return lf_fail(ctx, LF_ERR_INVALID, "lens: semi-aperture <= 0 or not finite");
    if (!std::isfinite(radius[k]) || !std::isfinite(thickness[k]))
      return lf_fail(ctx, LF_ERR_INVALID, "lens: radius / thickness not finite (a flat surface is radius 0)");
    if (k == stop_index && radius[k] != 0) return lf_fail(ctx, LF_ERR_INVALID, "lens: the stop must be flat");
    for (int l = 0; l < n_lambda; l++)
      if ((!(ior[l * n_surfaces + k] >= 1.0f) || !std::isfinite(ior[l * n_surfaces + k])) && k != stop_index)
        return lf_fail(ctx, LF_ERR_INVALID, "lens: index of refraction < 1 or not finite");
  }
  // a pupil target belongs to the prescription it was computed for (lf_aim_at_exit_pupil): a new lens
  // starts from the default disc, the rear element's clear aperture; so do its coatings: a new lens is bare
  ctx->pupil_target_h = 0.0f; ctx->pupil_target_z = 0.0f;
  ctx->coat = LfCoatings{};
  ctx->asph = LfAspheres{};      // (and its aspheres: a new lens is one of spheres)
  ctx->bic = LfBiconics{};       // (and its biconic records)
  ctx->pose = LfPoses{};         // (and its pose records)
  ctx->sensor.n_refl = 0;        // (and its sensor's reflectance; the sensor ghosts' mode is a setting of the context and stays)
  ctx->lenscam_dirty = true;
  lf_derive_lens(ctx, n_surfaces, stop_index, n_lambda, radius, thickness, ior, semi_aperture,
                 sensor_width_mm);
  ctx->raw_n = n_surfaces; ctx->raw_stop = stop_index;
  std::memcpy(ctx->raw_radius, radius, sizeof(float) * (size_t)n_surfaces);
  std::memcpy(ctx->raw_thickness, thickness, sizeof(float) * (size_t)n_surfaces);
  std::memcpy(ctx->raw_ior, ior, sizeof(float) * (size_t)n_surfaces * (size_t)n_lambda);
  ctx->lens_valid = true;
  ctx->events_dirty = true;
  // default pair set: every pair of glass surfaces + the primary path
  return lf_set_ghost_pairs(ctx, nullptr, 0, 1);
}

lf_status lf_set_lambda_rgb(lf_ctx* ctx, const float* weights) {
  if (!ctx || !weights) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_set_lambda_rgb before lf_set_lens");
  // the march's sums are UNSIGNED fixed point: a weight must be finite and >= 0 (a host whose colour matrix has
  // negative lobes renders the positive and the negative part as two frames and subtracts)
  for (int k = 0; k < 3 * ctx->lens.n_lambda; k++)
    if (!std::isfinite(weights[k]) || weights[k] < 0.0f)
      return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lambda_rgb: weights must be finite and >= 0");
  for (int l = 0; l < ctx->lens.n_lambda; l++)
    for (int c = 0; c < 3; c++) ctx->lens.lambda_rgb[l][c] = weights[3 * l + c];
  return LF_OK;
}

lf_status lf_validate_light(int kind, const float vec[3], const float radiance[3], float angular_radius, float front_radius,
                            float front_semi_aperture, char* message, size_t message_size) {
  if (message && message_size) message[0] = 0;
  if (!vec || !radiance) return LF_ERR_INVALID;
  if (!(front_semi_aperture > 0.0f) || !std::isfinite(front_semi_aperture) || !std::isfinite(front_radius)) return LF_ERR_INVALID;
  std::string why;
  const lf_status st = validate_light(kind, vec, radiance, angular_radius, true, front_radius, front_semi_aperture, &why);
  if (message && message_size) std::snprintf(message, message_size, "%s", why.c_str());
  return st;
}

// (stride: floats per light in vec -- 3: the three-float calls, which know kinds 0 and 1 alone; LF_LIGHT_GEOM_FLOATS: lf_set_lights_geom)
static lf_status set_lights(lf_ctx* ctx, const char* who, int n_lights, const int* kind, const float* vec, const float* radiance,
                            const float* angular_radius, int stride = 3) {
  if (n_lights < 1 || n_lights > LF_MAX_LIGHTS)
    return lf_fail(ctx, LF_ERR_INVALID, std::string(who) + ": 1 .. LF_MAX_LIGHTS (" + std::to_string(LF_MAX_LIGHTS) + ") lights per launch");
  // every light is validated before any is installed: a refusal leaves the previous lights in place
  LfLensDev L = ctx->lens;
  float radius[LF_MAX_LIGHTS];
  for (int k = 0; k < n_lights; k++) {
    const float* d = vec + stride * k;
    const float* rad = radiance + 3 * k;
    const float ar = angular_radius[k];
    const int kd = kind ? kind[k] : LF_LIGHT_DIRECTIONAL;
    std::string why;
    const lf_status st = stride == 3 ? validate_light(kd, d, rad, ar, ctx->lens_valid, ctx->raw_radius[0], ctx->raw_semi_ap[0], &why)
                                     : validate_light_geom(kd, d, rad, ar, ctx->lens_valid, ctx->raw_radius[0], ctx->raw_semi_ap[0], &why);
    if (st != LF_OK) return lf_fail(ctx, st, why);
    // a point light's direction: from the front vertex (z = 0 in the prescription's coordinates) to its position
    // (an area light's: to its centre)
    const double n = std::sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
    for (int c = 0; c < 3; c++) {
      L.light_dir[k][c] = (float)(d[c] / n);
      L.light_radiance[k][c] = rad[c];
      L.light_pos[k][c] = kd != LF_LIGHT_DIRECTIONAL ? d[c] : 0.0f;
    }
    L.light_kind[k] = kd;
    radius[k] = ar;
    L.light_inv_one_minus_cos[k] = (float)(1.0 / (1.0 - std::cos((double)ar)));
    L.light_ss[k] = (float)((double)L.light_dir[k][0] * L.light_dir[k][0] +
                            (double)L.light_dir[k][1] * L.light_dir[k][1] +
                            (double)L.light_dir[k][2] * L.light_dir[k][2]);
    L.light_thr[k] = lf_march_lobe_thr_of(L.light_inv_one_minus_cos[k]);
    for (int c = 0; c < 9; c++) L.light_area[k][c] = 0.0f;
    if (kd == LF_LIGHT_AREA) {
      // the direction normalised in double, then narrowed; the edges as given; no lobe: the angular radius is ignored (0), the
      // lobe's scalars hold a quarter sphere's (finite, read by no kernel), light_thr the bounding sphere's squared radius
      const double nd = std::sqrt((double)d[3] * d[3] + (double)d[4] * d[4] + (double)d[5] * d[5]);
      for (int c = 0; c < 3; c++) L.light_area[k][c] = (float)((double)d[3 + c] / nd);
      for (int c = 3; c < 9; c++) L.light_area[k][c] = d[3 + c];
      radius[k] = 0.0f;
      L.light_inv_one_minus_cos[k] = 1.0f;
      L.light_thr[k] = area_bound2(d + 6, d + 9);
    }
  }
  for (int k = n_lights; k < LF_MAX_LIGHTS; k++) {
    for (int c = 0; c < 3; c++) L.light_dir[k][c] = L.light_radiance[k][c] = L.light_pos[k][c] = 0.0f;
    for (int c = 0; c < 9; c++) L.light_area[k][c] = 0.0f;
    L.light_inv_one_minus_cos[k] = L.light_ss[k] = L.light_thr[k] = 0.0f;
    L.light_kind[k] = LF_LIGHT_DIRECTIONAL;
  }
  L.n_lights = n_lights;
  // light 0 is the sun of the single-light kernels
  for (int c = 0; c < 3; c++) { L.sun_dir[c] = L.light_dir[0][c]; L.sun_radiance[c] = L.light_radiance[0][c]; }
  L.sun_inv_one_minus_cos = L.light_inv_one_minus_cos[0];
  L.sun_ss = L.light_ss[0];
  ctx->lens = L;
  for (int k = 0; k < LF_MAX_LIGHTS; k++) ctx->light_radius[k] = k < n_lights ? radius[k] : 0.0f;
  ctx->sun_valid = true;
  return LF_OK;
}

lf_status lf_set_lights_ex(lf_ctx* ctx, int n_lights, const int* kind, const float* vec, const float* radiance,
                           const float* angular_radius) {
  if (!ctx || !kind || !vec || !radiance || !angular_radius) return LF_ERR_INVALID;
  return set_lights(ctx, "lf_set_lights_ex", n_lights, kind, vec, radiance, angular_radius);
}

lf_status lf_set_lights(lf_ctx* ctx, int n_lights, const float* dir, const float* radiance, const float* angular_radius) {
  if (!ctx || !dir || !radiance || !angular_radius) return LF_ERR_INVALID;
  return set_lights(ctx, "lf_set_lights", n_lights, nullptr, dir, radiance, angular_radius);
}

lf_status lf_set_sun(lf_ctx* ctx, const float dir[3], const float radiance[3],
                     float angular_radius) {
  if (!ctx || !dir || !radiance) return LF_ERR_INVALID;
  return lf_set_lights(ctx, 1, dir, radiance, &angular_radius);
}

lf_status lf_get_lights_ex(lf_ctx* ctx, int* n_lights, int* kind, float* vec, float* radiance, float* angular_radius) {
  if (!ctx) return LF_ERR_INVALID;
  const int n = ctx->sun_valid ? ctx->lens.n_lights : 0;
  if (n_lights) *n_lights = n;
  for (int k = 0; k < n; k++) {
    const bool point = ctx->lens.light_kind[k] != LF_LIGHT_DIRECTIONAL;
    if (kind) kind[k] = ctx->lens.light_kind[k];
    for (int c = 0; c < 3; c++) {
      if (vec) vec[3 * k + c] = point ? ctx->lens.light_pos[k][c] : ctx->lens.light_dir[k][c];
      if (radiance) radiance[3 * k + c] = ctx->lens.light_radiance[k][c];
    }
    if (angular_radius) angular_radius[k] = ctx->light_radius[k];
  }
  return LF_OK;
}

// (a point light: the unit vector from the front vertex to its position, which is what light_dir[k] holds)
lf_status lf_get_lights(lf_ctx* ctx, int* n_lights, float* dir, float* radiance, float* angular_radius) {
  if (!ctx) return LF_ERR_INVALID;
  const int n = ctx->sun_valid ? ctx->lens.n_lights : 0;
  if (n_lights) *n_lights = n;
  for (int k = 0; k < n; k++) {
    for (int c = 0; c < 3; c++) {
      if (dir) dir[3 * k + c] = ctx->lens.light_dir[k][c];
      if (radiance) radiance[3 * k + c] = ctx->lens.light_radiance[k][c];
    }
    if (angular_radius) angular_radius[k] = ctx->light_radius[k];
  }
  return LF_OK;
}

// ---- the twelve-float family (lf_set_lights_geom: area lights; DESIGN.md section 4, "area lights") ---------------------
lf_status lf_set_lights_geom(lf_ctx* ctx, int n_lights, const int* kind, const float* geom, const float* radiance,
                             const float* angular_radius) {
  if (!ctx || !kind || !geom || !radiance || !angular_radius) return LF_ERR_INVALID;
  return set_lights(ctx, "lf_set_lights_geom", n_lights, kind, geom, radiance, angular_radius, LF_LIGHT_GEOM_FLOATS);
}

lf_status lf_get_lights_geom(lf_ctx* ctx, int* n_lights, int* kind, float* geom, float* radiance, float* angular_radius) {
  if (!ctx) return LF_ERR_INVALID;
  const LfLensDev& L = ctx->lens;
  const int n = ctx->sun_valid ? L.n_lights : 0;
  if (n_lights) *n_lights = n;
  for (int k = 0; k < n; k++) {
    if (kind) kind[k] = L.light_kind[k];
    if (geom) {
      float* g = geom + LF_LIGHT_GEOM_FLOATS * k;
      for (int c = 0; c < 3; c++) g[c] = L.light_kind[k] != LF_LIGHT_DIRECTIONAL ? L.light_pos[k][c] : L.light_dir[k][c];
      for (int c = 0; c < 9; c++) g[3 + c] = L.light_area[k][c];
    }
    for (int c = 0; c < 3; c++) if (radiance) radiance[3 * k + c] = L.light_radiance[k][c];
    if (angular_radius) angular_radius[k] = ctx->light_radius[k];
  }
  return LF_OK;
}

lf_status lf_validate_light_geom(int kind, const float* geom, const float radiance[3], float angular_radius, float front_radius,
                                 float front_semi_aperture, char* message, size_t message_size) {
  if (message && message_size) message[0] = 0;
  if (!geom || !radiance) return LF_ERR_INVALID;
  if (!(front_semi_aperture > 0.0f) || !std::isfinite(front_semi_aperture) || !std::isfinite(front_radius)) return LF_ERR_INVALID;
  std::string why;
  const lf_status st = validate_light_geom(kind, geom, radiance, angular_radius, true, front_radius, front_semi_aperture, &why);
  if (message && message_size) std::snprintf(message, message_size, "%s", why.c_str());
  return st;
}

// an area light's geometry as lf_set_lights_geom stores it: the centre, then direction (normalised in double, narrowed),
// dim_x, dim_y -- what the kernels' definitions take; false: not finite, or no direction
static bool stored_area(const float* geom, float C[3], float g[9]) {
  for (int c = 0; c < LF_LIGHT_GEOM_FLOATS; c++) if (!std::isfinite(geom[c])) return false;
  const double nd = std::sqrt((double)geom[3] * geom[3] + (double)geom[4] * geom[4] + (double)geom[5] * geom[5]);
  if (!(nd > 0.0)) return false;
  for (int c = 0; c < 3; c++) { C[c] = geom[c]; g[c] = (float)((double)geom[3 + c] / nd); }
  for (int c = 3; c < 9; c++) g[c] = geom[3 + c];
  return true;
}

lf_status lf_light_geom_factor(int kind, const float* geom, float angular_radius, const float ray[6], float* factor, int* inside,
                               double* t) {
  if (!geom || !ray) return LF_ERR_INVALID;
  if (kind == LF_LIGHT_DIRECTIONAL || kind == LF_LIGHT_POINT) {
    float q = 0.0f;
    int in = 0;
    const lf_status st = lf_light_lobe_factor(kind, geom, angular_radius, ray, &q, &in);
    if (st != LF_OK) return st;
    const float om = 1.0f - q;
    if (factor) *factor = in ? om * om : 0.0f;
    if (inside) *inside = in;
    if (t) *t = (double)INFINITY;
    return LF_OK;
  }
  if (kind != LF_LIGHT_AREA) return LF_ERR_INVALID;
  float C[3], g[9];
  if (!stored_area(geom, C, g)) return LF_ERR_INVALID;
  for (int c = 0; c < 6; c++) if (!std::isfinite(ray[c])) return LF_ERR_INVALID;
  const bool in = lfm::lf_area_inside(ray[3], ray[4], ray[5], ray[0], ray[1], ray[2], C, g);
  if (factor) *factor = in ? 1.0f : 0.0f;
  if (inside) *inside = in ? 1 : 0;
  if (t) (void)lfm::lf_area_shadow_reach(ray[3], ray[4], ray[5], ray[0], ray[1], ray[2], C, g, 1.0, t);
  return LF_OK;
}

lf_status lf_area_light_pretest(const float* geom, const float ray[6], int* admitted) {
  if (!geom || !ray || !admitted) return LF_ERR_INVALID;
  float C[3], g[9];
  if (!stored_area(geom, C, g)) return LF_ERR_INVALID;
  for (int c = 0; c < 6; c++) if (!std::isfinite(ray[c])) return LF_ERR_INVALID;
  *admitted = lfm::lf_area_pretest(ray[3], ray[4], ray[5], ray[0], ray[1], ray[2], C, area_bound2(g + 3, g + 6)) ? 1 : 0;
  return LF_OK;
}

lf_status lf_ghost_shadow_reach_geom(int kind, const float* geom, const float ray[6], double world_per_mm, double* reach) {
  if (!geom || !ray || !reach) return LF_ERR_INVALID;
  if (kind == LF_LIGHT_DIRECTIONAL || kind == LF_LIGHT_POINT) return lf_ghost_shadow_reach(kind, geom, ray, world_per_mm, reach);
  if (kind != LF_LIGHT_AREA) return LF_ERR_INVALID;
  if (!(world_per_mm > 0.0) || !std::isfinite(world_per_mm)) return LF_ERR_INVALID;
  float C[3], g[9];
  if (!stored_area(geom, C, g)) return LF_ERR_INVALID;
  for (int c = 0; c < 6; c++) if (!std::isfinite(ray[c])) return LF_ERR_INVALID;
  *reach = lfm::lf_area_shadow_reach(ray[3], ray[4], ray[5], ray[0], ray[1], ray[2], C, g, world_per_mm);
  return LF_OK;
}

lf_status lf_area_light_cull_cone(const float* geom, float front_radius, float front_semi_aperture, float dir[3], float* rho) {
  if (!geom || !dir || !rho) return LF_ERR_INVALID;
  if (!(front_semi_aperture > 0.0f) || !std::isfinite(front_semi_aperture) || !std::isfinite(front_radius)) return LF_ERR_INVALID;
  const float rad[3] = {0.0f, 0.0f, 0.0f};
  std::string why;
  if (validate_light_geom(LF_LIGHT_AREA, geom, rad, 0.0f, true, front_radius, front_semi_aperture, &why) != LF_OK) return LF_ERR_INVALID;
  float C[3], g[9];
  if (!stored_area(geom, C, g)) return LF_ERR_INVALID;
  lf_area_cull_cone(C, g, lf_front_reach(front_radius, front_semi_aperture), true, dir, rho);
  return LF_OK;
}

// The lobe factor of ONE exit ray for ONE light, host arithmetic: the definitions the kernels call (lf_march_events.h
// lf_point_lobe_q for a point light; for a directional light the sun's expression, whose root the device takes with
// v_sqrt_f32 -- 1 ulp -- where the host's is correctly rounded: q agrees to 2 ulp there, bit for bit for a point light).
// The light is normalised / stored exactly as lf_set_lights_ex stores it.
lf_status lf_light_lobe_factor(int kind, const float vec[3], float angular_radius, const float ray[6], float* q, int* inside) {
  if (!vec || !ray || (kind != LF_LIGHT_DIRECTIONAL && kind != LF_LIGHT_POINT)) return LF_ERR_INVALID;
  if (!(angular_radius > 0) || angular_radius > 1.5f) return LF_ERR_INVALID;
  for (int c = 0; c < 3; c++) if (!std::isfinite(vec[c])) return LF_ERR_INVALID;
  for (int c = 0; c < 6; c++) if (!std::isfinite(ray[c])) return LF_ERR_INVALID;
  const float inv_1mc = (float)(1.0 / (1.0 - std::cos((double)angular_radius)));
  float qq, cg;
  bool in;
  if (kind == LF_LIGHT_POINT) {
    qq = lfm::lf_point_lobe_q(ray[3], ray[4], ray[5], ray[0], ray[1], ray[2], vec[0], vec[1], vec[2], inv_1mc, cg);
    in = cg > 0.0f && qq < 1.0f;
  } else {
    const double n = std::sqrt((double)vec[0] * vec[0] + (double)vec[1] * vec[1] + (double)vec[2] * vec[2]);
    if (!(n > 0)) return LF_ERR_INVALID;
    const float s[3] = {(float)(vec[0] / n), (float)(vec[1] / n), (float)(vec[2] / n)};
    const float ss = (float)((double)s[0] * s[0] + (double)s[1] * s[1] + (double)s[2] * s[2]);
    // (a light at s - 0 with |s|^2 handed in: lf_point_lobe_q's arithmetic IS lobe_q's once s and ss are given)
    const float dx = ray[3], dy = ray[4], dz = ray[5];
    cg = fmaf(dx, s[0], fmaf(dy, s[1], dz * s[2]));
    const float cx = fmaf(dy, s[2], -(dz * s[1])), cy = fmaf(dz, s[0], -(dx * s[2])), cz = fmaf(dx, s[1], -(dy * s[0]));
    const float c2 = fmaf(cx, cx, fmaf(cy, cy, cz * cz));
    const float dd = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
    const float ds = dd * ss;
    qq = (c2 / fmaf(sqrtf(ds), cg, ds)) * inv_1mc;
    in = cg > lf_march_lobe_thr_of(inv_1mc) && qq < 1.0f;
  }
  if (q) *q = qq;
  if (inside) *inside = in ? 1 : 0;
  return LF_OK;
}

// (1 - q_k)^2 of n exit rays {origin xyz in lens millimetres, z absolute; direction xyz} for every installed light k where
// the ray lies inside it, 0 elsewhere: k_ghost_ray_light_factors calls what the lit epilogue calls (light_admits_at)
lf_status lf_ghost_ray_light_factors(lf_ctx* ctx, size_t n, const float* rays, float* out) {
  if (!ctx || (n > 0 && (!rays || !out))) return LF_ERR_INVALID;
  if (n > 0x7fffffffull / LF_MAX_LIGHTS) return lf_fail(ctx, LF_ERR_INVALID, "lf_ghost_ray_light_factors: too many rays for one call");
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_ghost_ray_light_factors before lf_set_lens");
  if (!ctx->sun_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_ghost_ray_light_factors: no light installed (lf_set_sun / lf_set_lights / lf_set_lights_ex)");
  lf_status st = lf_point_lights_fit(ctx, "lf_ghost_ray_light_factors");
  if (st != LF_OK) return st;
  if (n == 0) return LF_OK;
  LF_HIP(ctx, hipSetDevice(ctx->device));
  const int nl = ctx->lens.n_lights;
  float *d_rays = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc((void**)&d_rays, n * 6 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, n * (size_t)nl * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(d_rays, rays, n * 6 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpyAsync(ctx->lens_dev, &ctx->lens, sizeof(LfLensDev), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) st = lfk_ghost_ray_light_factors(ctx, n, d_rays, d_out);
  if (e == hipSuccess && st == LF_OK) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(out, d_out, n * (size_t)nl * sizeof(float), hipMemcpyDeviceToHost);
  if (d_rays) (void)hipFree(d_rays);
  if (d_out) (void)hipFree(d_out);
  if (st != LF_OK) return st;
  LF_HIP(ctx, e);
  return LF_OK;
}

lf_status lf_paraxial_efl(int n, int stop, const float* radius, const float* thickness,
                          const float* ior_row, double* efl_mm) {
  if (n < 1 || n > LF_MAX_SURFACES || !radius || !thickness || !ior_row || !efl_mm) return LF_ERR_INVALID;
  // ray (height, angle); T(d) = [[1, d], [0, 1]], R(c, n1, n2) = [[1, 0], [c (n1 - n2) / n2, n1 / n2]]
  double m00 = 1, m01 = 0, m10 = 0, m11 = 1, n1 = 1.0;
  for (int k = 0; k < n; k++) {
    if (k != stop) {
      const double c = radius[k] == 0.0f ? 0.0 : 1.0 / (double)radius[k], n2 = ior_row[k];
      if (!(n2 >= 1.0)) return LF_ERR_INVALID;
      const double r10 = c * (n1 - n2) / n2, r11 = n1 / n2;
      const double a10 = r10 * m00 + r11 * m10, a11 = r10 * m01 + r11 * m11;
      m10 = a10; m11 = a11;
      n1 = n2;
    }
    if (k + 1 < n) {  // the last thickness (to the sensor) does not change the power
      const double d = thickness[k];
      m00 += d * m10; m01 += d * m11;
    }
  }
  if (m10 == 0.0) return LF_ERR_INVALID;  // afocal
  *efl_mm = -1.0 / (m10 * n1);            // image-space medium n1 (air for a camera lens)
  return LF_OK;
}

// Where a collimated beam from field angle theta (small) lands on the sensor plane, per unit of theta: the
// height of its CHIEF ray (the one through the stop's centre) -- the centre of the beam's image whether the
// sensor sits in the focal plane (then this is the focal length) or not (a lens refocused by lf_focus_lens:
// focal length + sensor shift x the chief ray's exit slope).  Paraxial, the reference's T / R operators.
static bool paraxial_image_scale(int n, int stop, const float* radius, const float* thickness, const float* ior_row,
                                 double* scale) {
  // two rays from the first vertex, (height 1, slope 0) and (height 0, slope 1): everything is linear in them
  double y[2] = {1.0, 0.0}, u[2] = {0.0, 1.0}, ys[2] = {1.0, 0.0};
  double n1 = 1.0;
  for (int k = 0; k < n; k++) {
    if (k == stop) { ys[0] = y[0]; ys[1] = y[1]; }
    else {
      const double c = radius[k] == 0.0f ? 0.0 : 1.0 / (double)radius[k], n2 = ior_row[k];
      if (!(n2 >= 1.0)) return false;
      for (int r = 0; r < 2; r++) u[r] = c * (n1 - n2) / n2 * y[r] + n1 / n2 * u[r];
      n1 = n2;
    }
    for (int r = 0; r < 2; r++) y[r] += (double)thickness[k] * u[r];   // (the last thickness: to the sensor)
  }
  // chief ray of slope 1: height y0 at the first vertex such that it crosses the stop's centre
  const double y0 = (stop >= 0 && ys[0] != 0.0) ? -ys[1] / ys[0] : 0.0;
  *scale = y0 * y[0] + y[1];
  return std::isfinite(*scale) && *scale != 0.0;
}

lf_status lf_paraxial_image_scale(int n, int stop, const float* radius, const float* thickness, const float* ior_row,
                                  double* scale_mm) {
  if (n <= 0 || !radius || !thickness || !ior_row || !scale_mm) return LF_ERR_INVALID;
  return paraxial_image_scale(n, stop, radius, thickness, ior_row, scale_mm) ? LF_OK : LF_ERR_INVALID;
}

// the light flare `flare` of the flare state stands for: its direction through the image scale, its radiance
// the x-meridian prescription of a lens with biconic records (lf_set_lens_biconics): Rx where a record is on, the row's
// radius elsewhere
static void meridian_x_radii(const lf_ctx* ctx, float rx[LF_MAX_SURFACES]) {
  for (int k = 0; k < ctx->raw_n; k++) rx[k] = ctx->bic.on[k] ? ctx->bic.rx[k] : ctx->raw_radius[k];
}

// (efl_x_mm: the image scale of the x meridian -- *efl_mm's value unless the lens has biconic records and the caller left
// the scale to the prescription, efl_mm <= 0: then the paraxial scale of the x-radii prescription)
static lf_status light_of_flare(lf_ctx* ctx, const char* who, const LfFlares& f, int flare, double* efl_mm, double* efl_x_mm,
                                float dir[3], float rad[3]) {
  if (!(*efl_mm > 0.0) && ctx->bic.n > 0) {
    float rx[LF_MAX_SURFACES];
    meridian_x_radii(ctx, rx);
    if (!paraxial_image_scale(ctx->raw_n, ctx->raw_stop, rx, ctx->raw_thickness,
                              ctx->raw_ior + (size_t)(ctx->lens.n_lambda / 2) * ctx->raw_n, efl_x_mm) || !(*efl_x_mm > 0.0))
      return lf_fail(ctx, LF_ERR_INVALID, std::string(who) + ": the prescription's x meridian images no distant point on its sensor");
  }
  if (!(*efl_mm > 0.0)) {
    // the image scale of THIS sensor position: the focal length when the sensor sits in the focal plane (the
    // shipped prescriptions), the chief ray's landing height per unit field angle when lf_focus_lens has moved it
    if (!paraxial_image_scale(ctx->raw_n, ctx->raw_stop, ctx->raw_radius, ctx->raw_thickness,
                              ctx->raw_ior + (size_t)(ctx->lens.n_lambda / 2) * ctx->raw_n, efl_mm) || !(*efl_mm > 0.0))
      return lf_fail(ctx, LF_ERR_INVALID, std::string(who) + ": the prescription images no distant point on its sensor");
  }
  if (!(*efl_x_mm > 0.0)) *efl_x_mm = *efl_mm;
  const double sw = ctx->sensor_w_mm, sh = sw * (double)ctx->H / (double)ctx->W;
  dir[0] = (float)((f.origin[flare][0] - 0.5) * sw / *efl_x_mm);
  dir[1] = (float)((f.origin[flare][1] - 0.5) * sh / *efl_mm);
  dir[2] = -1.0f;
  for (int c = 0; c < 3; c++) rad[c] = (float)f.radiance[flare][c];
  return LF_OK;
}

lf_status lf_set_sun_from_flares(lf_ctx* ctx, int flare, double efl_mm, float angular_radius) {
  if (!ctx || flare < 0 || flare >= LF_MAX_FLARES) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_set_sun_from_flares before lf_set_frame");
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_set_sun_from_flares before lf_set_lens");
  if (!ctx->flares_valid) return lf_fail(ctx, LF_ERR_STATE, "no flare state: call lf_find_sun_pos or lf_set_flares");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  LfFlares f;
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LF_HIP(ctx, hipMemcpy(&f, ctx->flares, sizeof(f), hipMemcpyDeviceToHost));
  if (flare >= f.n_flares) return lf_fail(ctx, LF_ERR_INVALID, "lf_set_sun_from_flares: no such flare in the frame");
  float dir[3], rad[3];
  double efl_x_mm = efl_mm > 0.0 ? efl_mm : 0.0;
  const lf_status st = light_of_flare(ctx, "lf_set_sun_from_flares", f, flare, &efl_mm, &efl_x_mm, dir, rad);
  if (st != LF_OK) return st;
  return lf_set_sun(ctx, dir, rad, angular_radius);
}

lf_status lf_set_lights_from_flares(lf_ctx* ctx, double efl_mm, float angular_radius, int* n_taken) {
  if (!ctx) return LF_ERR_INVALID;
  if (n_taken) *n_taken = 0;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_set_lights_from_flares before lf_set_frame");
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_set_lights_from_flares before lf_set_lens");
  if (!ctx->flares_valid) return lf_fail(ctx, LF_ERR_STATE, "no flare state: call lf_find_sun_pos or lf_set_flares");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  LfFlares f;
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LF_HIP(ctx, hipMemcpy(&f, ctx->flares, sizeof(f), hipMemcpyDeviceToHost));
  if (f.n_flares < 1) return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lights_from_flares: no flare in the frame");
  // (the flare state keeps LF_MAX_FLARES flares; what find_sun_pos met beyond them it only counted)
  if (f.n_flares > LF_MAX_LIGHTS || f.n_in_frame > LF_MAX_LIGHTS)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lights_from_flares: " + std::to_string(std::max(f.n_flares, f.n_in_frame)) + " flares in the frame, one launch marches at most LF_MAX_LIGHTS = " +
                                            std::to_string(LF_MAX_LIGHTS) + " lights (compose launches with lf_set_ghost_accumulate)");
  float dir[3 * LF_MAX_LIGHTS], rad[3 * LF_MAX_LIGHTS], ar[LF_MAX_LIGHTS];
  double efl_x_mm = efl_mm > 0.0 ? efl_mm : 0.0;
  for (int k = 0; k < f.n_flares; k++) {
    const lf_status st = light_of_flare(ctx, "lf_set_lights_from_flares", f, k, &efl_mm, &efl_x_mm, dir + 3 * k, rad + 3 * k);
    if (st != LF_OK) return st;
    ar[k] = angular_radius;
  }
  const lf_status st = lf_set_lights(ctx, f.n_flares, dir, rad, ar);
  if (st == LF_OK && n_taken) *n_taken = f.n_flares;
  return st;
}

// The scene's lights as the lights of the march: the in-frame flares (DirectionalLights) as lf_set_lights_from_flares takes
// them, then every PointLight of the installed scene lights (type 1 of lf_set_scene_lights, LfLight::v its position) through
// the INVERSE of the lens camera's mapping, in double: p_lens = c2w^T (p_world - pos) / wpm + (0, 0, z_ref), z_ref the
// paraxial entrance pupil's z (lf_fill_occlusion's, lf_get_lens_camera's).  A point light the front element's limits
// refuse (behind the camera, or closer than lf_set_lights_ex allows) is skipped and not counted.
// (areas: lf_set_lights_from_scene_ex -- every AreaLight too, type 3: position as a point, direction as c2w^T v, dim_x and dim_y
// as c2w^T v / wpm, in double, then narrowed; a rectangle lf_set_lights_geom's validation refuses is skipped and not counted)
static lf_status set_lights_from_scene(lf_ctx* ctx, const std::string& who, bool areas, double efl_mm, float angular_radius,
                                       double world_per_mm, int* n_directional, int* n_point, int* n_area) {
  if (!ctx) return LF_ERR_INVALID;
  if (n_directional) *n_directional = 0;
  if (n_point) *n_point = 0;
  if (n_area) *n_area = 0;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, who + " before lf_set_frame");
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, who + " before lf_set_lens");
  if (!ctx->cam_valid) return lf_fail(ctx, LF_ERR_STATE, who + " before lf_set_camera");
  if (!(world_per_mm > 0.0) || !std::isfinite(world_per_mm))
    return lf_fail(ctx, LF_ERR_INVALID, who + ": world_per_mm must be > 0 and finite");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int kind[LF_MAX_LIGHTS];
  float vec[LF_LIGHT_GEOM_FLOATS * LF_MAX_LIGHTS] = {}, rad[3 * LF_MAX_LIGHTS], ar[LF_MAX_LIGHTS];
  constexpr int GF = LF_LIGHT_GEOM_FLOATS;
  int n = 0, n_dir = 0, n_pt = 0, n_ar = 0;
  const std::string too_many = who + ": more lights than one launch marches (LF_MAX_LIGHTS = " + std::to_string(LF_MAX_LIGHTS) +
                               "; compose launches with lf_set_ghost_accumulate)";
  if (ctx->flares_valid) {
    LfFlares f;
    LF_HIP(ctx, hipMemcpy(&f, ctx->flares, sizeof(f), hipMemcpyDeviceToHost));
    if (f.n_flares > LF_MAX_LIGHTS || f.n_in_frame > LF_MAX_LIGHTS) return lf_fail(ctx, LF_ERR_INVALID, too_many);
    double efl_x_mm = efl_mm > 0.0 ? efl_mm : 0.0;
    for (int k = 0; k < f.n_flares; k++) {
      const lf_status st = light_of_flare(ctx, who.c_str(), f, k, &efl_mm, &efl_x_mm, vec + GF * n, rad + 3 * n);
      if (st != LF_OK) return st;
      kind[n] = LF_LIGHT_DIRECTIONAL; ar[n] = angular_radius;
      n++; n_dir++;
    }
  }
  if (ctx->scene_valid && ctx->scene_dev.n_lights > 0) {
    std::vector<LfLight> lts((size_t)ctx->scene_dev.n_lights);
    LF_HIP(ctx, hipMemcpy(lts.data(), ctx->scene_dev.lights, lts.size() * sizeof(LfLight), hipMemcpyDeviceToHost));
    double z_ref = 0.0, mag = 1.0;
    if (ctx->raw_stop >= 0 &&
        lf_paraxial_entrance_pupil(ctx->raw_n, ctx->raw_stop, ctx->raw_radius, ctx->raw_thickness,
                                   ctx->raw_ior + (size_t)(ctx->lens.n_lambda / 2) * ctx->raw_n, &z_ref, &mag) != LF_OK)
      return lf_fail(ctx, LF_ERR_INVALID, who + ": the stop has no finite paraxial image through the front group");
    const double r_f = lf_front_reach(ctx->raw_radius[0], ctx->raw_semi_ap[0]);
    const double* M = ctx->cam.c2w;
    for (const LfLight& l : lts) {
      if (l.type == 3 && areas) {
        // the rectangle in lens millimetres: a point, a direction and two edges through the inverse mapping
        const double w[3] = {l.v[0] - ctx->cam.pos[0], l.v[1] - ctx->cam.pos[1], l.v[2] - ctx->cam.pos[2]};
        float g[GF];
        g[0] = (float)(((M[0] * w[0] + M[3] * w[1]) + M[6] * w[2]) / world_per_mm);
        g[1] = (float)(((M[1] * w[0] + M[4] * w[1]) + M[7] * w[2]) / world_per_mm);
        g[2] = (float)(((M[2] * w[0] + M[5] * w[1]) + M[8] * w[2]) / world_per_mm + z_ref);
        const double* const vs[3] = {l.dir, l.dim_x, l.dim_y};
        for (int i = 0; i < 3; i++) {
          const double sc = i == 0 ? 1.0 : world_per_mm;
          for (int c = 0; c < 3; c++) g[3 + 3 * i + c] = (float)(((M[c] * vs[i][0] + M[3 + c] * vs[i][1]) + M[6 + c] * vs[i][2]) / sc);
        }
        const float rgb[3] = {(float)l.rgb[0], (float)l.rgb[1], (float)l.rgb[2]};
        std::string why;
        if (validate_light_geom(LF_LIGHT_AREA, g, rgb, 0.0f, true, ctx->raw_radius[0], ctx->raw_semi_ap[0], &why) != LF_OK) continue;
        if (n >= LF_MAX_LIGHTS) return lf_fail(ctx, LF_ERR_INVALID, too_many);
        for (int c = 0; c < GF; c++) vec[GF * n + c] = g[c];
        for (int c = 0; c < 3; c++) rad[3 * n + c] = rgb[c];
        kind[n] = LF_LIGHT_AREA; ar[n] = 0.0f;
        n++; n_ar++;
        continue;
      }
      if (l.type != 1) continue;
      const double w[3] = {l.v[0] - ctx->cam.pos[0], l.v[1] - ctx->cam.pos[1], l.v[2] - ctx->cam.pos[2]};
      const float p[3] = {(float)(((M[0] * w[0] + M[3] * w[1]) + M[6] * w[2]) / world_per_mm),
                          (float)(((M[1] * w[0] + M[4] * w[1]) + M[7] * w[2]) / world_per_mm),
                          (float)(((M[2] * w[0] + M[5] * w[1]) + M[8] * w[2]) / world_per_mm + z_ref)};
      const double dist = std::sqrt((double)p[0] * p[0] + (double)p[1] * p[1] + (double)p[2] * p[2]);
      if (!std::isfinite(dist) || !((double)p[2] <= -2.0 * r_f) || !(dist >= 4.0 * r_f)) continue;   // (behind the limit: skipped)
      if (n >= LF_MAX_LIGHTS) return lf_fail(ctx, LF_ERR_INVALID, too_many);
      for (int c = 0; c < 3; c++) { vec[GF * n + c] = p[c]; rad[3 * n + c] = (float)l.rgb[c]; }
      kind[n] = LF_LIGHT_POINT; ar[n] = angular_radius;
      n++; n_pt++;
    }
  }
  if (n < 1) return lf_fail(ctx, LF_ERR_INVALID, who + (areas ? ": no flare in the frame and no point or area light in front of the lens"
                                                                : ": no flare in the frame and no point light in front of the lens"));
  const lf_status st = set_lights(ctx, who.c_str(), n, kind, vec, rad, ar, GF);
  if (st != LF_OK) return st;
  if (n_directional) *n_directional = n_dir;
  if (n_point) *n_point = n_pt;
  if (n_area) *n_area = n_ar;
  return LF_OK;
}

lf_status lf_set_lights_from_scene(lf_ctx* ctx, double efl_mm, float angular_radius, double world_per_mm, int* n_directional,
                                   int* n_point) {
  return set_lights_from_scene(ctx, "lf_set_lights_from_scene", false, efl_mm, angular_radius, world_per_mm, n_directional, n_point, nullptr);
}

lf_status lf_set_lights_from_scene_ex(lf_ctx* ctx, double efl_mm, float angular_radius, double world_per_mm, int* n_directional,
                                      int* n_point, int* n_area) {
  return set_lights_from_scene(ctx, "lf_set_lights_from_scene_ex", true, efl_mm, angular_radius, world_per_mm, n_directional, n_point, n_area);
}

lf_status lf_set_ghost_pairs(lf_ctx* ctx, const int* pairs, int n_pairs, int include_primary) {
  if (!ctx || n_pairs < 0) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_set_ghost_pairs before lf_set_lens");
  LfPairsDev P;
  std::memset(&P, 0, sizeof(P));
  const int ns = ctx->lens.n_surf, stop = ctx->lens.stop;
  if (include_primary) { P.ij[P.n][0] = -1; P.ij[P.n][1] = -1; P.n++; }
  if (!pairs || n_pairs == 0) {
    for (int i = 0; i < ns; i++)
      for (int j = i + 1; j < ns; j++) {
        if (i == stop || j == stop) continue;
        if (P.n >= LF_MAX_PAIRS + 1) return lf_fail(ctx, LF_ERR_INVALID, "too many ghost pairs");
        P.ij[P.n][0] = i; P.ij[P.n][1] = j; P.n++;
      }
  } else {
    if (n_pairs > LF_MAX_PAIRS) return lf_fail(ctx, LF_ERR_INVALID, "too many ghost pairs");
    for (int q = 0; q < n_pairs; q++) {
      int i = pairs[2 * q], j = pairs[2 * q + 1];
      if (i == -1 && j == -1) {  // the primary path, listed explicitly
        if (P.n > 0 && P.ij[0][0] < 0) return lf_fail(ctx, LF_ERR_INVALID, "primary path listed twice");
        if (P.n > 0) {  // keep it first, like include_primary does
          for (int k = P.n; k > 0; k--) { P.ij[k][0] = P.ij[k - 1][0]; P.ij[k][1] = P.ij[k - 1][1]; }
        }
        P.ij[0][0] = -1; P.ij[0][1] = -1; P.n++;
        continue;
      }
      if (i < 0 || j <= i || j >= ns || i == stop || j == stop)
        return lf_fail(ctx, LF_ERR_INVALID, "ghost pair must satisfy 0 <= i < j < n, neither the stop");
      P.ij[P.n][0] = i; P.ij[P.n][1] = j; P.n++;
    }
  }
  if (P.n == 0) return lf_fail(ctx, LF_ERR_INVALID, "empty pair set");
  ctx->pairs = P;
  ctx->events_dirty = true;
  return LF_OK;
}

lf_status lf_set_pupil_subcells(lf_ctx* ctx, int bits) {
  if (!ctx) return LF_ERR_INVALID;
  if (bits < 0 || bits > kMaxSubcellBits) return lf_fail(ctx, LF_ERR_INVALID, "pupil sub-cell bits must be 0..8");
  ctx->march_sub_bits = bits;
  return LF_OK;
}

lf_status lf_set_tile_stride(lf_ctx* ctx, int stride) {
  if (!ctx) return LF_ERR_INVALID;
  if (stride != 1 && stride != 2 && stride != 4 && stride != 8)
    return lf_fail(ctx, LF_ERR_INVALID, "tile stride must be 1, 2, 4 or 8");
  ctx->march_xstride_log2 = stride == 1 ? 0 : stride == 2 ? 1 : stride == 4 ? 2 : 3;
  return LF_OK;
}

lf_status lf_trace_ghosts(lf_ctx* ctx, int spp, uint64_t key) {
  if (!ctx || spp <= 0) return LF_ERR_INVALID;
  if (!ctx->lens_valid || !ctx->sun_valid)
    return lf_fail(ctx, LF_ERR_STATE, "lf_trace_ghosts needs lf_set_lens and lf_set_sun");
  if (!ctx->ap[LF_APERTURE_STARBURST].valid)
    return lf_fail(ctx, LF_ERR_STATE, "aperture mask (LF_APERTURE_STARBURST slot) not set");
  if (ctx->pupil_target_h > 0.0f && ctx->lens.stop >= 0 && ctx->sensor.mode != LF_SENSOR_GHOSTS_ONLY) {
    // a reduced disc (the stop's image) is an unbiased estimator only for paths that cross the stop before
    // their first reflection; a pair with both mirrors behind the stop reaches the sensor through parts of
    // the rear element the disc does not cover
    for (int q = 0; q < ctx->pairs.n; q++)
      if (ctx->pairs.ij[q][0] > ctx->lens.stop)
        return lf_fail(ctx, LF_ERR_STATE,
                       "a pupil target is set and the pair selection holds a pair with both mirrors behind the stop: "
                       "such pairs need the default disc (march them in a second launch, lf_set_ghost_accumulate)");
  }
  if (ctx->ghost_occlusion) {
    const lf_status ready = lf_occlusion_ready(ctx, "lf_trace_ghosts");
    if (ready != LF_OK) return ready;
  }
  const int sensor_mode = ctx->sensor.mode;
  if (sensor_mode != LF_SENSOR_GHOSTS_OFF && ctx->sensor.n_refl == 0)
    return lf_fail(ctx, LF_ERR_STATE, "lf_trace_ghosts: sensor ghosts are on and the sensor has no reflectance (lf_set_sensor_reflectance)");
  if (sensor_mode != LF_SENSOR_GHOSTS_OFF && ctx->pose.n > 0 && ctx->sensor.surfaces != LF_SENSOR_SURFACES_POSED)
    return lf_fail(ctx, LF_ERR_UNSUPPORTED, "lf_trace_ghosts: sensor ghosts (lf_set_sensor_ghosts: LF_SENSOR_GHOSTS_ADD / LF_SENSOR_GHOSTS_ONLY) "
                                            "are not marched through a lens with posed interfaces (lf_set_lens_poses) under "
                                            "LF_SENSOR_SURFACES_CENTRED; lf_set_sensor_ghost_surfaces(LF_SENSOR_SURFACES_POSED) marches them");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  lf_status st = LF_OK;
  if (sensor_mode != LF_SENSOR_GHOSTS_ONLY) st = lfk_march(ctx, spp, key);
  // the sensor's mirror: its paths behind the ordinary selection's (ADD) or alone (ONLY), a launch of their own
  if (st == LF_OK && sensor_mode != LF_SENSOR_GHOSTS_OFF) st = lfk_march_sensor(ctx, spp, key, sensor_mode == LF_SENSOR_GHOSTS_ADD);
  if (st != LF_OK) return st;
  ctx->ghost_valid = true;
  return LF_OK;
}

lf_status lf_set_march_culling(lf_ctx* ctx, int mode) {
  if (!ctx) return LF_ERR_INVALID;
  if (mode < 0 || mode > 2) return lf_fail(ctx, LF_ERR_INVALID, "march culling: 0 off, 1 on, 2 on and rebuilt at every launch");
  ctx->march_cull = mode;
  return LF_OK;
}

// ---- the pre-pass of a multi-GPU frame, shared ----------------------------------------------
lf_status lf_set_cull_share(lf_ctx* ctx, int rank, int nranks) {
  if (!ctx) return LF_ERR_INVALID;
  if (nranks < 1 || nranks > 64 || rank < 0 || rank >= nranks) return lf_fail(ctx, LF_ERR_INVALID, "lf_set_cull_share: 0 <= rank < nranks <= 64");
  if (ctx->split.table == LfSplit::kComm) return lf_fail(ctx, LF_ERR_STATE, "lf_set_cull_share: the table is shared through the communicator (lf_comm_share_cull)");
  if (nranks > 1 && ctx->split.deal == LfSplit::kBlocks)
    return lf_fail(ctx, LF_ERR_STATE, "lf_set_cull_share: the frame is dealt by blocks (lf_set_block_deal): every rank builds the rows it reads, nothing is shared");
  lf_install_split(ctx, nranks > 1 ? ctx->split.with_table(LfSplit::kHost, rank, nranks) : ctx->split.with_table(LfSplit::kOwn));
  return LF_OK;
}

lf_status lf_cull_prepare(lf_ctx* ctx, int spp) {
  if (!ctx) return LF_ERR_INVALID;
  if (ctx->split.table != LfSplit::kHost) return lf_fail(ctx, LF_ERR_STATE, "lf_cull_prepare without lf_set_cull_share(rank, nranks > 1)");
  if (!ctx->lens_valid || !ctx->ap[LF_APERTURE_STARBURST].valid || ctx->W == 0)
    return lf_fail(ctx, LF_ERR_STATE, "lf_cull_prepare: frame, prescription and aperture mask come first");
  if (spp < 1) return LF_ERR_INVALID;
  LF_HIP(ctx, hipSetDevice(ctx->device));
  return lfk_cull_prepare(ctx, spp);
}

lf_status lf_cull_table_view(lf_ctx* ctx, void** device_ptr, uint64_t* entries, uint64_t* entries_per_rank) {
  if (!ctx || !device_ptr || !entries || !entries_per_rank) return LF_ERR_INVALID;
  *device_ptr = nullptr; *entries = 0; *entries_per_rank = 0;
  if (ctx->cull_hash_pending == 0) return LF_OK;           // (this launch does not cull: nothing to exchange)
  LF_HIP(ctx, hipSetDevice(ctx->device));
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));          // the slab is written when the host's exchange reads it
  *entries_per_rank = (uint64_t)ctx->cull_resident.nb * (uint64_t)(ctx->cull_cells + 1);
  *entries = *entries_per_rank * (uint64_t)ctx->cull_resident.n;
  *device_ptr = ctx->cull_dev;
  return LF_OK;
}

lf_status lf_cull_commit(lf_ctx* ctx) {
  if (!ctx) return LF_ERR_INVALID;
  if (ctx->split.table != LfSplit::kHost) return lf_fail(ctx, LF_ERR_STATE, "lf_cull_commit without lf_set_cull_share(rank, nranks > 1)");
  if (ctx->cull_hash_pending == 0) return LF_OK;
  LF_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t h = ctx->cull_hash_pending;
  ctx->cull_hash_pending = 0;
  const lf_status st = lfk_cull_finish(ctx, h);
  if (st != LF_OK) return st;
  ctx->cull_fresh = true;
  return LF_OK;
}

lf_status lf_get_cull_info(lf_ctx* ctx, int info[8]) {
  if (!ctx || !info) return LF_ERR_INVALID;
  info[0] = ctx->march_cull;
  info[1] = ctx->last_march_culled ? 1 : 0;
  info[2] = ctx->cull_bx; info[3] = ctx->cull_by; info[4] = ctx->cull_cells; info[5] = ctx->cull_G; info[6] = ctx->cull_P;
  info[7] = 1 << ctx->cull_blk_log2;
  return LF_OK;
}

lf_status lf_get_cull_reason(lf_ctx* ctx, int* reason) {
  if (!ctx || !reason) return LF_ERR_INVALID;
  *reason = ctx->cull_reason;
  return LF_OK;
}

lf_status lf_set_cull_audit(lf_ctx* ctx, int rays_per_dropped_box) {
  if (!ctx) return LF_ERR_INVALID;
  if (rays_per_dropped_box < 0 || rays_per_dropped_box > 255) return lf_fail(ctx, LF_ERR_INVALID, "cull audit: 0 (off) .. 255 rays per dropped box");
  if (rays_per_dropped_box != ctx->cull_audit_density) ctx->cull_hash = 0;     // (a resident table was audited at the other density)
  ctx->cull_audit_density = rays_per_dropped_box;
  return LF_OK;
}

lf_status lf_get_cull_audit(lf_ctx* ctx, uint64_t* rays, uint64_t* lit, int* launches_refuted) {
  if (!ctx) return LF_ERR_INVALID;
  if (rays) *rays = ctx->cull_audit_rays;
  if (lit) *lit = ctx->cull_audit_lit;
  if (launches_refuted) *launches_refuted = ctx->cull_audit_tripped;
  return LF_OK;
}

// TEST HOOK (lensflare.h): the switches of the test suite and of bench.py's A/B legs, by name
// (ctx == null: the value becomes the default of every context created afterwards -- a test that cannot reach the
// contexts a helper creates; value 0 of a 0/1 knob takes the default away again)
lf_status lf_test_knob(lf_ctx* ctx, const char* name, double value) {
  if (!name) return LF_ERR_INVALID;
  if (!ctx) {
    std::lock_guard<std::mutex> lock(g_knob_mu);
    for (size_t i = 0; i < g_knob_defaults.size(); i++)
      if (g_knob_defaults[i].first == name) { g_knob_defaults.erase(g_knob_defaults.begin() + (long)i); break; }
    if (value != 0.0) g_knob_defaults.emplace_back(name, value);
    return LF_OK;
  }
  const std::string n(name);
  const int iv = (int)value;
  lf_ctx::CullRules& R = ctx->cull_rules;
  bool rules = true;
  if (n == "cull_force") { ctx->cull_force = iv != 0; return LF_OK; }
  if (n == "cull_weights_first") { ctx->cull_weights_first = iv != 0; return LF_OK; }
  if (n == "cull_no_prefix") { ctx->cull_no_prefix = iv != 0; return LF_OK; }
  if (n == "asph_force") { ctx->asph_force = iv != 0; ctx->events_dirty = true; return LF_OK; }
  if (n == "cull_ignore_light") { ctx->cull_ignore_light = iv; return LF_OK; }      // (-1: off; k: the cull table is built WITHOUT light k -- the audit's test)
  if (n == "cull_no_widening") { ctx->cull_no_widening = iv != 0; return LF_OK; }    // (1: a point light enters the cull table with a directional light's radius -- wrong by construction)
  if (n == "cull_cache") { ctx->cull_cache_on = iv != 0; return LF_OK; }            // (0: the pre-pass marches its boxes at every build)
  if (n == "cull_cache_max_mb") { ctx->cull_cache_max_mb = value; return LF_OK; }   // (the cached tree's byte budget, MiB)
  if (n == "scene_compact") { ctx->scene_compact = iv < 0 ? -1 : iv != 0; return LF_OK; }
  if (n == "comm_force_exchange") { ctx->comm_force_exchange = iv != 0; return LF_OK; }
  if (n == "scene_lens_strided") { ctx->scene_lens_strided = iv < 0 ? -1 : iv != 0; return LF_OK; }
  if (n == "bvh_median") { ctx->bvh_median = iv != 0; return LF_OK; }
  if (n == "bvh_leaf") { ctx->bvh_leaf_max = iv; return LF_OK; }
  if (n == "march_tail_tiles") { ctx->march_tail_tiles = iv; return LF_OK; }       // (-1: the default, one round of resident workgroups)
  if (n == "march_tail_groups") { ctx->march_tail_groups = iv; return LF_OK; }     // (1: no split tail)
  if (n == "cull_general_kernel") { if (!iv) R = lf_ctx::CullRules(); ctx->cull_rules_custom = iv != 0; }
  else if (n == "cull_strict") R.strict = iv;
  else if (n == "cull_strict_lost") R.strict_lost = iv;
  else if (n == "cull_slack") R.slack_mode = iv;
  else if (n == "cull_keep_partial") R.keep_partial = iv;
  else if (n == "cull_disable") R.disable = iv;
  else if (n == "cull_margin") R.margin = (float)value;
  else if (n == "cull_lobe_k") R.lobe_k = (float)value;
  else if (n == "cull_lost_rel") R.lost_rel = (float)value;
  else if (n == "cull_lost_abs") R.lost_abs = (float)value;
  else rules = false;
  if (!rules) return lf_fail(ctx, LF_ERR_INVALID, "lf_test_knob: unknown knob '" + n + "'");
  if (n != "cull_general_kernel") ctx->cull_rules_custom = true;
  ctx->cull_hash = 0;
  return LF_OK;
}

lf_status lf_get_cull_started_fraction(lf_ctx* ctx, double* fraction) {
  if (!ctx || !fraction) return LF_ERR_INVALID;
  *fraction = ctx->cull_started_fraction;
  return LF_OK;
}

lf_status lf_get_cull_table(lf_ctx* ctx, uint64_t* out, size_t n_entries) {
  if (!ctx || !out) return LF_ERR_INVALID;
  if (!ctx->last_march_culled || !ctx->cull_dev || ctx->cull_hash == 0)
    return lf_fail(ctx, LF_ERR_STATE, "lf_get_cull_table: the last lf_trace_ghosts did not cull (or none has run)");
  if (ctx->cull_chunks > 1)
    return lf_fail(ctx, LF_ERR_STATE, "lf_get_cull_table: the last lf_trace_ghosts marched more than 64 paths in two launches, each with its own table");
  const size_t n = (size_t)ctx->cull_bx * ctx->cull_by * (size_t)(ctx->cull_cells + 1);
  if (n_entries != n) return lf_fail(ctx, LF_ERR_INVALID, "lf_get_cull_table: size must be blocks_x * blocks_y * (cells + 1)");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const LfCullSlab& r = ctx->cull_resident;
  if (r.n > 1) {
    // a shared table lies slab by slab (lf_cull_row_of_block): handed out in block order all the same
    const size_t re = (size_t)(ctx->cull_cells + 1), rows = (size_t)r.nb * r.n;
    std::vector<uint64_t> raw(rows * re);
    LF_HIP(ctx, hipMemcpy(raw.data(), ctx->cull_dev, raw.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (int b = 0; b < ctx->cull_bx * ctx->cull_by; b++)
      std::memcpy(out + (size_t)b * re, raw.data() + lf_cull_row_of_block(b, r.n, r.nb) * re, re * sizeof(uint64_t));
    return LF_OK;
  }
  LF_HIP(ctx, hipMemcpy(out, ctx->cull_dev, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return LF_OK;
}

lf_status lf_get_march_fix_bits(lf_ctx* ctx, int* bits) {
  if (!ctx || !bits) return LF_ERR_INVALID;
  *bits = ctx->march_fix_bits;
  return LF_OK;
}

// ---- ghost occlusion ("ghost occlusion") ---------------------------------------------------------
lf_status lf_set_ghost_occlusion(lf_ctx* ctx, int on, double world_per_mm) {
  if (!ctx) return LF_ERR_INVALID;
  if (on != 0 && (!(world_per_mm > 0.0) || !std::isfinite(world_per_mm)))
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_ghost_occlusion: world_per_mm must be > 0 and finite");
  ctx->ghost_occlusion = on != 0;
  if (on != 0) ctx->ghost_occl_wpm = world_per_mm;
  return LF_OK;
}

lf_status lf_get_ghost_occlusion(lf_ctx* ctx, int* on, double* world_per_mm, int* march_variant) {
  if (!ctx) return LF_ERR_INVALID;
  if (on) *on = ctx->ghost_occlusion ? 1 : 0;
  if (world_per_mm) *world_per_mm = ctx->ghost_occl_wpm;
  if (march_variant) *march_variant = lf_march_variant(ctx);
  return LF_OK;
}

lf_status lf_get_ghost_occlusion_stats(lf_ctx* ctx, uint64_t out[2]) {
  if (!ctx || !out) return LF_ERR_INVALID;
  unsigned long long c[2];
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LF_HIP(ctx, hipMemcpy(c, ctx->counters_dev + kMarchOcclSlot, sizeof(c), hipMemcpyDeviceToHost));
  out[0] = c[0]; out[1] = c[1];
  return LF_OK;
}

lf_status lf_ghost_ray_visibility(lf_ctx* ctx, size_t n, const float* rays, unsigned char* visible) {
  if (!ctx || (n > 0 && (!rays || !visible))) return LF_ERR_INVALID;
  if (n > 0x7fffffffull) return lf_fail(ctx, LF_ERR_INVALID, "lf_ghost_ray_visibility: too many rays for one call");
  if (!ctx->ghost_occlusion)
    return lf_fail(ctx, LF_ERR_STATE, "lf_ghost_ray_visibility: ghost occlusion is off (lf_set_ghost_occlusion gives the mapping its scale)");
  lf_status st = lf_occlusion_ready(ctx, "lf_ghost_ray_visibility");
  if (st != LF_OK) return st;
  if (n == 0) return LF_OK;
  LfOcclDev o;
  st = lf_fill_occlusion(ctx, ctx->ghost_occl_wpm, &o);
  if (st != LF_OK) return st;
  LF_HIP(ctx, hipSetDevice(ctx->device));
  float* d_rays = nullptr;
  unsigned char* d_vis = nullptr;
  hipError_t e = hipMalloc((void**)&d_rays, n * 6 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_vis, n);
  if (e == hipSuccess) e = hipMemcpy(d_rays, rays, n * 6 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) st = lfk_ghost_ray_visibility(ctx, o, n, d_rays, d_vis);
  if (e == hipSuccess && st == LF_OK) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(visible, d_vis, n, hipMemcpyDeviceToHost);
  if (d_rays) (void)hipFree(d_rays);
  if (d_vis) (void)hipFree(d_vis);
  if (st != LF_OK) return st;
  LF_HIP(ctx, e);
  return LF_OK;
}

// ---- where a point light's shadow ray ends ("the reach of a shadow ray") --------------------------
lf_status lf_set_ghost_occlusion_reach(lf_ctx* ctx, int reach) {
  if (!ctx) return LF_ERR_INVALID;
  if (reach != LF_OCCLUSION_REACH_SKY && reach != LF_OCCLUSION_REACH_LIGHT)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_ghost_occlusion_reach: LF_OCCLUSION_REACH_SKY (0) or LF_OCCLUSION_REACH_LIGHT (1)");
  ctx->ghost_occl_reach = reach;
  return LF_OK;
}

lf_status lf_get_ghost_occlusion_reach(lf_ctx* ctx, int* reach) {
  if (!ctx || !reach) return LF_ERR_INVALID;
  *reach = ctx->ghost_occl_reach;
  return LF_OK;
}

// The reach of ONE exit ray's shadow ray for ONE light, host arithmetic: the definition the kernels call
// (lf_march_events.h lf_point_shadow_reach), bit for bit
lf_status lf_ghost_shadow_reach(int kind, const float vec[3], const float ray[6], double world_per_mm, double* reach) {
  if (!vec || !ray || !reach || (kind != LF_LIGHT_DIRECTIONAL && kind != LF_LIGHT_POINT)) return LF_ERR_INVALID;
  if (!(world_per_mm > 0.0) || !std::isfinite(world_per_mm)) return LF_ERR_INVALID;
  for (int c = 0; c < 3; c++) if (!std::isfinite(vec[c])) return LF_ERR_INVALID;
  for (int c = 0; c < 6; c++) if (!std::isfinite(ray[c])) return LF_ERR_INVALID;
  *reach = kind == LF_LIGHT_POINT
               ? lfm::lf_point_shadow_reach(ray[3], ray[4], ray[5], ray[0], ray[1], ray[2], vec[0], vec[1], vec[2], world_per_mm)
               : (double)INFINITY;
  return LF_OK;
}

lf_status lf_ghost_ray_light_visibility(lf_ctx* ctx, size_t n, const float* rays, unsigned char* visible) {
  if (!ctx || (n > 0 && (!rays || !visible))) return LF_ERR_INVALID;
  if (n > 0x7fffffffull / LF_MAX_LIGHTS) return lf_fail(ctx, LF_ERR_INVALID, "lf_ghost_ray_light_visibility: too many rays for one call");
  if (!ctx->ghost_occlusion)
    return lf_fail(ctx, LF_ERR_STATE, "lf_ghost_ray_light_visibility: ghost occlusion is off (lf_set_ghost_occlusion gives the mapping its scale)");
  lf_status st = lf_occlusion_ready(ctx, "lf_ghost_ray_light_visibility");
  if (st != LF_OK) return st;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_ghost_ray_light_visibility before lf_set_lens");
  if (!ctx->sun_valid)
    return lf_fail(ctx, LF_ERR_STATE, "lf_ghost_ray_light_visibility: no light installed (lf_set_sun / lf_set_lights / lf_set_lights_ex)");
  st = lf_point_lights_fit(ctx, "lf_ghost_ray_light_visibility");
  if (st != LF_OK) return st;
  st = lf_occlusion_reach_ready(ctx, "lf_ghost_ray_light_visibility");
  if (st != LF_OK) return st;
  if (n == 0) return LF_OK;
  LfOcclDev o;
  st = lf_fill_occlusion(ctx, ctx->ghost_occl_wpm, &o);
  if (st != LF_OK) return st;
  LF_HIP(ctx, hipSetDevice(ctx->device));
  const size_t nl = (size_t)ctx->lens.n_lights;
  float* d_rays = nullptr;
  unsigned char* d_vis = nullptr;
  hipError_t e = hipMalloc((void**)&d_rays, n * 6 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_vis, n * nl);
  if (e == hipSuccess) e = hipMemcpy(d_rays, rays, n * 6 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpyAsync(ctx->lens_dev, &ctx->lens, sizeof(LfLensDev), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) st = lfk_ghost_ray_light_visibility(ctx, o, n, d_rays, d_vis);
  if (e == hipSuccess && st == LF_OK) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(visible, d_vis, n * nl, hipMemcpyDeviceToHost);
  if (d_rays) (void)hipFree(d_rays);
  if (d_vis) (void)hipFree(d_vis);
  if (st != LF_OK) return st;
  LF_HIP(ctx, e);
  return LF_OK;
}

lf_status lf_generate_lens_rays(lf_ctx* ctx, int lambda, size_t n, const float* sensor_xy_mm,
                                const float* pupil_uv, float* out) {
  if (!ctx || !sensor_xy_mm || !pupil_uv || !out) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_generate_lens_rays before lf_set_lens");
  if (!ctx->ap[LF_APERTURE_STARBURST].valid)
    return lf_fail(ctx, LF_ERR_STATE, "aperture mask (LF_APERTURE_STARBURST slot) not set");
  if (lambda < 0 || lambda >= ctx->lens.n_lambda || n > 0x7fffffffull)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_generate_lens_rays: wavelength index / count out of range");
  if (n == 0) return LF_OK;
  // (an aspheric lens: the primary table knows spheres only -- the same ray along the primary path's own sequence)
  if (ctx->asph.n > 0 || ctx->bic.n > 0) return lf_march_path_rays(ctx, lambda, -1, -1, n, sensor_xy_mm, pupil_uv, out);
  LF_HIP(ctx, hipSetDevice(ctx->device));
  float *d_xy = nullptr, *d_uv = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc((void**)&d_xy, n * 2 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_uv, n * 2 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, n * 8 * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(d_xy, sensor_xy_mm, n * 2 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_uv, pupil_uv, n * 2 * sizeof(float), hipMemcpyHostToDevice);
  lf_status st = LF_OK;
  if (e == hipSuccess) st = lfk_lens_rays(ctx, lambda, (int)n, d_xy, d_uv, d_out);
  if (e == hipSuccess && st == LF_OK) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(out, d_out, n * 8 * sizeof(float), hipMemcpyDeviceToHost);
  if (d_xy) (void)hipFree(d_xy);
  if (d_uv) (void)hipFree(d_uv);
  if (d_out) (void)hipFree(d_out);
  if (st != LF_OK) return st;
  LF_HIP(ctx, e);
  return LF_OK;
}

lf_status lf_march_tables(int n_surfaces, int stop_index, int n_lambda, const float* radius,
                          const float* thickness, const float* ior, const float* semi_aperture,
                          const int* pairs, int n_pairs, int include_primary, int* info,
                          float* rows, size_t rows_cap, int* skip, size_t skip_cap) {
  if (!info) return LF_ERR_INVALID;
  lf_ctx ctx;          // plain host state: nothing below touches the device
  ctx.W = ctx.H = 64;
  lf_status st = lf_set_lens(&ctx, n_surfaces, stop_index, n_lambda, radius, thickness, ior, semi_aperture, 36.0f);
  if (st == LF_OK && (pairs || !include_primary)) st = lf_set_ghost_pairs(&ctx, pairs, n_pairs, include_primary);
  std::vector<LfEventRow> r;
  std::vector<int> sk;
  if (st == LF_OK) st = lf_build_march_tables(&ctx, r, sk);
  if (st != LF_OK) return st;
  const LfPairsDev& P = ctx.pairs;
  info[0] = P.n; info[1] = P.total_events; info[2] = P.prog_off; info[3] = P.prog_rows;
  info[4] = (int)r.size(); info[5] = (int)sk.size();
  for (int q = 0; q < P.n && q < LF_MAX_PAIRS + 1; q++) {
    info[8 + 4 * q] = P.ij[q][0]; info[8 + 4 * q + 1] = P.ij[q][1];
    info[8 + 4 * q + 2] = P.ev_off[q]; info[8 + 4 * q + 3] = P.ev_cnt[q];
  }
  if (rows) {
    if (rows_cap < r.size() * 8) return LF_ERR_INVALID;
    for (size_t i = 0; i < r.size(); i++) std::memcpy(rows + 8 * i, &r[i], 8 * sizeof(float));   // the documented fields
  }
  if (skip) {
    if (skip_cap < sk.size()) return LF_ERR_INVALID;
    std::memcpy(skip, sk.data(), sk.size() * sizeof(int));
  }
  return LF_OK;
}

namespace {
// what Application::load hands the renderer, flattened for lf_set_scene / lf_set_scene_lights;
// returns an empty string, or why the device scene term cannot render the file
extern "C++" std::string flatten_collada(const lfamd::ColladaScene& sc, std::vector<double>& sph, std::vector<int>& sph_m,
                            std::vector<double>& tp, std::vector<double>& tn, std::vector<int>& tri_m,
                            std::vector<double>& mats, std::vector<double>& lights, std::vector<double>& suns) {
  // DiffuseBSDF and EmissionBSDF as they are.  Mirror / Refraction / Glass / Microfacet are unfilled
  // stubs in the reference: their f() returns 0 and they emit nothing (advanced_bsdf.cpp:17-133,
  // bsdf.h:183-254), and the reference's integrator is zero_bounce + one_bounce only
  // (pathtracer.cpp:282-302) -- such a surface IS a black occluder there, so that is what it is here:
  // diffuse with reflectance 0.
  for (const auto& m : sc.materials) {
    const bool lit = m.kind == lfamd::BSDF_DIFFUSE || m.kind == lfamd::BSDF_EMISSION;
    mats.push_back(m.kind == lfamd::BSDF_EMISSION ? 1.0 : 0.0);
    mats.push_back(lit ? m.rgb.x : 0.0); mats.push_back(lit ? m.rgb.y : 0.0); mats.push_back(lit ? m.rgb.z : 0.0);
  }
  for (const auto& s : sc.spheres) {
    sph.insert(sph.end(), {s.o.x, s.o.y, s.o.z, s.r});
    sph_m.push_back(s.material);
  }
  for (const auto& t : sc.triangles) {
    for (int k = 0; k < 3; k++) { tp.push_back(t.p[k].x); tp.push_back(t.p[k].y); tp.push_back(t.p[k].z); }
    for (int k = 0; k < 3; k++) { tn.push_back(t.n[k].x); tn.push_back(t.n[k].y); tn.push_back(t.n[k].z); }
    tri_m.push_back(t.material);
  }
  for (const auto& l : sc.lights) {
    double row[16] = {0};
    row[1] = l.radiance.x; row[2] = l.radiance.y; row[3] = l.radiance.z;
    auto put = [&](int at, const lfamd::ColladaVec3& v) { row[at] = v.x; row[at + 1] = v.y; row[at + 2] = v.z; };
    if (l.type == lfamd::LIGHT_DIRECTIONAL) {
      row[0] = 0; put(4, l.direction);
      suns.insert(suns.end(), {l.position.x, l.position.y, l.position.z, l.radiance.x, l.radiance.y, l.radiance.z});
    } else if (l.type == lfamd::LIGHT_POINT) {
      row[0] = 1; put(4, l.position);
    } else if (l.type == lfamd::LIGHT_HEMISPHERE) {
      row[0] = 2;
    } else if (l.type == lfamd::LIGHT_AREA) {
      row[0] = 3; put(4, l.position); put(7, l.direction); put(10, l.dim_x); put(13, l.dim_y);
    } else {
      return "spot lights are a stub in the reference (light.cpp:64-72) and are not rendered";
    }
    lights.insert(lights.end(), row, row + 16);
  }
  return "";
}
}  // namespace

lf_status lf_collada_check(const char* path, char* msg, size_t msg_cap) {
  if (!path) return LF_ERR_INVALID;
  lfamd::ColladaScene sc;
  std::string err;
  if (!lfamd::load_collada(path, sc, err)) err = "lf_load_collada: " + err;
  else {
    std::vector<double> a, c, d, e, f, g;
    std::vector<int> b, h;
    err = flatten_collada(sc, a, b, c, d, h, e, f, g);
  }
  if (msg && msg_cap) { std::strncpy(msg, err.c_str(), msg_cap - 1); msg[msg_cap - 1] = 0; }
  return err.empty() ? LF_OK : LF_ERR_INVALID;
}

lf_status lf_load_collada(lf_ctx* ctx, const char* path, lf_collada_camera* camera, double* sun_lights,
                          int max_sun_lights, int* n_sun_lights) {
  if (!ctx || !path) return LF_ERR_INVALID;
  lfamd::ColladaScene sc;
  std::string err;
  if (!lfamd::load_collada(path, sc, err)) return lf_fail(ctx, LF_ERR_INVALID, "lf_load_collada: " + err);
  std::vector<double> sph, tp, tn, mats, lights, suns;
  std::vector<int> sph_m, tri_m;
  err = flatten_collada(sc, sph, sph_m, tp, tn, tri_m, mats, lights, suns);
  if (!err.empty()) return lf_fail(ctx, LF_ERR_INVALID, "lf_load_collada: " + err);
  const int n_sun = (int)(suns.size() / 6);
  for (int k = 0; k < n_sun && sun_lights && k < max_sun_lights; k++)
    std::memcpy(sun_lights + 6 * k, suns.data() + 6 * k, 6 * sizeof(double));
  if (n_sun_lights) *n_sun_lights = n_sun;
  if (camera) {
    std::memset(camera, 0, sizeof(*camera));
    const auto& c = sc.camera;
    camera->present = c.present ? 1 : 0;
    camera->hfov = c.hFov; camera->vfov = c.vFov; camera->nclip = c.nClip; camera->fclip = c.fClip;
    camera->pos[0] = c.pos.x; camera->pos[1] = c.pos.y; camera->pos[2] = c.pos.z;
    camera->dir[0] = c.dir.x; camera->dir[1] = c.dir.y; camera->dir[2] = c.dir.z;
    camera->up[0] = c.up.x; camera->up[1] = c.up.y; camera->up[2] = c.up.z;
  }
  lf_status st = lf_set_scene(ctx, (int)sph_m.size(), sph.data(), sph_m.data(), (int)tri_m.size(), tp.data(),
                              tn.data(), tri_m.data(), (int)sc.materials.size(), mats.data(), 0, nullptr);
  if (st != LF_OK) return st;
  return lf_set_scene_lights(ctx, (int)(lights.size() / 16), lights.data());
}

lf_status lf_set_starburst_spectrum(lf_ctx* ctx, int n, const double* scale, const double* rgb_weights) {
  if (!ctx || n < 0 || n > LF_MAX_LAMBDA || (n > 0 && (!scale || !rgb_weights))) return LF_ERR_INVALID;
  LfStarSpectrum sp{};
  sp.n = n;
  for (int l = 0; l < n; l++) {
    if (!(scale[l] > 0.0) || !(scale[l] < 1e6))
      return lf_fail(ctx, LF_ERR_INVALID, "lf_set_starburst_spectrum: scale must be positive and finite");
    sp.scale[l] = scale[l];
    for (int c = 0; c < 3; c++) sp.rgb[l][c] = rgb_weights[3 * l + c];
  }
  ctx->star_spec = sp;
  ctx->sample_valid = false;
  return LF_OK;
}

// ---------------------------------------------------------------- helper members ---------------
// The reference declares its ghost / starburst helpers as public members (pathtracer.h:45-57,
// :95-101); a drop-in defines every one of them, on the device like the frame-level calls.
static lf_status ghost_helper_ready(lf_ctx* ctx, const char* who) {
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, std::string(who) + " before lf_set_frame");
  if (!ctx->ap[LF_APERTURE_GHOST].valid) return lf_fail(ctx, LF_ERR_STATE, std::string(who) + ": ghost aperture not set");
  { const lf_status js = lf_comm_join(ctx); if (js != LF_OK) return js; }
  LF_HIP(ctx, hipSetDevice(ctx->device));
  return LF_OK;
}

lf_status lf_clear_ghost_buffer(lf_ctx* ctx) {
  if (!ctx) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_clear_ghost_buffer before lf_set_frame");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  LF_HIP(ctx, hipMemsetAsync(ctx->ghost, 0, (size_t)ctx->W * ctx->H_alloc * 3 * sizeof(double), ctx->stream));
  ctx->ghost_valid = true;
  return LF_OK;
}

lf_status lf_draw_ghost(lf_ctx* ctx, int channel, float r1, float r2, int bbox[4]) {
  if (!ctx || channel < 0 || channel > 2) return LF_ERR_INVALID;
  lf_status st = ghost_helper_ready(ctx, "lf_draw_ghost");
  if (st != LF_OK) return st;
  if (!ctx->flares_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_draw_ghost: no flare state (axis_ray)");
  return lfk_draw_ghost(ctx, channel, r1, r2, bbox);
}

lf_status lf_rasterize_textured_triangle(lf_ctx* ctx, const float v[12], const double colour[3], int bbox[4]) {
  if (!ctx || !v || !colour) return LF_ERR_INVALID;
  lf_status st = ghost_helper_ready(ctx, "lf_rasterize_textured_triangle");
  if (st != LF_OK) return st;
  return lfk_raster_triangle(ctx, v, colour, bbox);
}

lf_status lf_fill_textured_pixel(lf_ctx* ctx, const float v[12], int x, int y, const double colour[3]) {
  if (!ctx || !v || !colour) return LF_ERR_INVALID;
  lf_status st = ghost_helper_ready(ctx, "lf_fill_textured_pixel");
  if (st != LF_OK) return st;
  // "assumes in bounds" (pathtracer.cpp:307): the reference would write past its buffer
  if (x < 0 || y < 0 || x >= ctx->W || y >= ctx->H) return lf_fail(ctx, LF_ERR_INVALID, "lf_fill_textured_pixel: pixel outside the frame");
  return lfk_fill_pixel(ctx, v, x, y, colour);
}

lf_status lf_shift_vertex(lf_ctx* ctx, float x, float y, float scale, float shift_amount, double out_xy[2]) {
  if (!ctx || !out_xy) return LF_ERR_INVALID;
  if (!ctx->flares_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_shift_vertex: no flare state (axis_ray)");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  return lfk_shift_vertex(ctx, x, y, scale, shift_amount, out_xy);
}

lf_status lf_compute_phase(lf_ctx* ctx, int flare, double u, double v, double out_re_im[2], double screen_pos[2]) {
  if (!ctx || !out_re_im || flare < 0 || flare >= LF_MAX_FLARES) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_compute_phase before lf_set_frame");
  if (!ctx->flares_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_compute_phase: no flare state");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  double o[4];
  lf_status st = lfk_compute_phase(ctx, flare, u, v, o);
  if (st != LF_OK) return st;
  out_re_im[0] = o[0]; out_re_im[1] = o[1];
  if (screen_pos) { screen_pos[0] = o[2]; screen_pos[1] = o[3]; }
  return LF_OK;
}

lf_status lf_irradiance_falloff(lf_ctx* ctx, int x, int y, double radius, double rgb[3]) {
  if (!ctx || !rgb) return LF_ERR_INVALID;
  if (ctx->W == 0) return lf_fail(ctx, LF_ERR_STATE, "lf_irradiance_falloff before lf_set_frame");
  if (x < 0 || y < 0 || x >= ctx->W || y >= ctx->H) return lf_fail(ctx, LF_ERR_INVALID, "lf_irradiance_falloff: pixel outside the frame");
  if (!ctx->flares_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_irradiance_falloff: no flare state");
  if (ctx->jitter_mode == 0 && !ctx->jitter_table_valid)
    return lf_fail(ctx, LF_ERR_STATE, "MT19937 jitter selected but no table (frame was resized?)");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  const LfFlares* fl = nullptr;
  const lf_status st = lf_flare_occlusion_update(ctx, "lf_irradiance_falloff", &fl, nullptr);
  if (st != LF_OK) return st;
  return lfk_irradiance_falloff(ctx, x, y, radius, rgb, fl);
}

// ---------------------------------------------------------------- stop-mask filter --------------
lf_status lf_set_mask_filter(lf_ctx* ctx, int filter) {
  if (!ctx) return LF_ERR_INVALID;
  if (filter != LF_MASK_NEAREST && filter != LF_MASK_BILINEAR)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_mask_filter: LF_MASK_NEAREST or LF_MASK_BILINEAR");
  if (filter == ctx->mask_filter) return LF_OK;
  ctx->mask_filter = filter;
  if (!ctx->ap[LF_APERTURE_STARBURST].valid) return LF_OK;   // (lf_set_aperture derives everything under the filter set)
  LF_HIP(ctx, hipSetDevice(ctx->device));
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));            // kernels in flight may read the support texture
  return derive_stop_mask(ctx);
}

lf_status lf_get_mask_filter(lf_ctx* ctx, int* filter) {
  if (!ctx || !filter) return LF_ERR_INVALID;
  *filter = ctx->mask_filter;
  return LF_OK;
}

lf_status lf_mask_lookup(const float* texels, int w, int h, int filter, float u, float v, float* value, int* open) {
  if (!texels || w <= 0 || h <= 0 || w > 4096 || h > 4096 || !std::isfinite(u) || !std::isfinite(v)) return LF_ERR_INVALID;
  if (filter != LF_MASK_NEAREST && filter != LF_MASK_BILINEAR) return LF_ERR_INVALID;
  // the stop event's mapping (stop_event, lf_march_events.h) with hx * inv_h = u
  const float fu = std::fmaf(u, 1.0f, 1.0f) * (0.5f * (float)w);
  const float fv = std::fmaf(v, 1.0f, 1.0f) * (0.5f * (float)h);
  if (!std::isfinite(fu) || !std::isfinite(fv)) return LF_ERR_INVALID;
  float a;
  bool alive;
  if (filter == LF_MASK_BILINEAR) {
    alive = lfm::lf_mask_bilinear(texels, w, h, fu, fv, a);
  } else {
    const int ix = std::min(std::max((int)std::min(std::max(fu, -1.0f), (float)w), 0), w - 1);
    const int iy = std::min(std::max((int)std::min(std::max(fv, -1.0f), (float)h), 0), h - 1);
    a = texels[(size_t)iy * w + ix];
    alive = a > 0.0f;
  }
  if (value) *value = a;
  if (open) *open = alive ? 1 : 0;
  return LF_OK;
}

// ---------------------------------------------------------------- coatings ----------------------
lf_status lf_set_lens_coatings(lf_ctx* ctx, int n_surfaces, int n_lambda, const float* lambda_nm,
                               const float* thickness_nm, const float* index) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_set_lens_coatings before lf_set_lens");
  if (!thickness_nm) {   // every interface bare
    ctx->coat = LfCoatings{};
    ctx->events_dirty = true;
    ctx->lenscam_dirty = true;
    return LF_OK;
  }
  const LfLensDev& L = ctx->lens;
  if (n_surfaces != ctx->raw_n || n_lambda != L.n_lambda || !lambda_nm || !index)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_coatings: sizes differ from the installed lens (or a NULL array)");
  for (int l = 0; l < n_lambda; l++)
    if (!std::isfinite(lambda_nm[l]) || !(lambda_nm[l] > 0.0f))
      return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_coatings: wavelengths must be finite and > 0 nm");
  LfCoatings C;
  for (int k = 0; k < n_surfaces; k++) {
    const float d = thickness_nm[k];
    if (!std::isfinite(d) || d < 0.0f || d > kCoatMaxThicknessNm)
      return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_coatings: a thickness must be finite and in [0, 10000] nm");
    if (d == 0.0f) continue;
    if (k == ctx->raw_stop) return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_coatings: the stop cannot carry a film");
    for (int l = 0; l < n_lambda; l++) {
      const float m = index[(size_t)l * n_surfaces + k];
      // m >= min(n, n') keeps the film's cosine real wherever the interface does not reflect totally
      if (!std::isfinite(m) || !(m >= std::min(L.surf[k].n_before[l], L.surf[k].n_after[l])))
        return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_coatings: a film index must be finite and >= the smaller index beside it");
    }
    C.n++;
  }
  for (int l = 0; l < n_lambda; l++) C.lambda_nm[l] = lambda_nm[l];
  for (int k = 0; k < n_surfaces; k++) {
    C.thickness_nm[k] = thickness_nm[k];
    for (int l = 0; l < n_lambda; l++)
      C.index[(size_t)l * n_surfaces + k] = thickness_nm[k] > 0.0f ? index[(size_t)l * n_surfaces + k] : 0.0f;
    if (thickness_nm[k] > 0.0f) {   // (lf_get_lens_coating_stacks reads a film as one layer)
      C.n_layers[k] = 1;
      C.layer_nm[k] = thickness_nm[k];
      for (int l = 0; l < n_lambda; l++) C.layer_index[(size_t)l * n_surfaces + k] = index[(size_t)l * n_surfaces + k];
    }
  }
  if (C.n == 0) C = LfCoatings{};
  ctx->coat = C;
  ctx->events_dirty = true;
  ctx->lenscam_dirty = true;
  return LF_OK;
}

lf_status lf_get_lens_coatings(lf_ctx* ctx, int n_surfaces, int n_lambda, float* lambda_nm, float* thickness_nm,
                               float* index, int* n_coated) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_get_lens_coatings before lf_set_lens");
  if (n_surfaces != ctx->raw_n || n_lambda != ctx->lens.n_lambda)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_get_lens_coatings: sizes differ from the installed lens");
  const LfCoatings& C = ctx->coat;
  if (C.n_stacked > 0)
    return lf_fail(ctx, LF_ERR_STATE, "lf_get_lens_coatings: an interface holds a stack of layers (lf_get_lens_coating_stacks)");
  if (lambda_nm) for (int l = 0; l < n_lambda; l++) lambda_nm[l] = C.lambda_nm[l];
  if (thickness_nm) for (int k = 0; k < n_surfaces; k++) thickness_nm[k] = C.thickness_nm[k];
  if (index) for (size_t i = 0; i < (size_t)n_lambda * n_surfaces; i++) index[i] = C.index[i];
  if (n_coated) *n_coated = C.n;
  return LF_OK;
}

lf_status lf_set_lens_coating_stacks(lf_ctx* ctx, int n_surfaces, int n_lambda, const float* lambda_nm,
                                     const int* n_layers, const float* thickness_nm, const float* index) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_set_lens_coating_stacks before lf_set_lens");
  if (!n_layers) {   // every interface bare
    ctx->coat = LfCoatings{};
    ctx->events_dirty = true;
    ctx->lenscam_dirty = true;
    return LF_OK;
  }
  const LfLensDev& L = ctx->lens;
  if (n_surfaces != ctx->raw_n || n_lambda != L.n_lambda || !lambda_nm || !thickness_nm || !index)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_coating_stacks: sizes differ from the installed lens (or a NULL array)");
  for (int l = 0; l < n_lambda; l++)
    if (!std::isfinite(lambda_nm[l]) || !(lambda_nm[l] > 0.0f))
      return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_coating_stacks: wavelengths must be finite and > 0 nm");
  LfCoatings C;
  for (int l = 0; l < n_lambda; l++) C.lambda_nm[l] = lambda_nm[l];
  for (int k = 0; k < n_surfaces; k++) {
    if (n_layers[k] < 0 || n_layers[k] > LF_MAX_COAT_LAYERS)
      return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_coating_stacks: an interface takes 0 .. LF_MAX_COAT_LAYERS layers");
    if (n_layers[k] > 0 && k == ctx->raw_stop)
      return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_coating_stacks: the stop cannot carry a layer");
    int kept = 0;
    for (int j = 0; j < n_layers[k]; j++) {
      const float d = thickness_nm[(size_t)j * n_surfaces + k];
      if (!std::isfinite(d) || d < 0.0f || d > kCoatMaxThicknessNm)
        return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_coating_stacks: a thickness must be finite and in [0, 10000] nm");
      if (d == 0.0f) continue;   // dropped (its index is not read): the layers behind it move up
      for (int l = 0; l < n_lambda; l++) {
        const float m = index[((size_t)j * n_lambda + l) * n_surfaces + k];
        // m >= min(n, n') keeps every layer's cosine real wherever the interface does not reflect totally
        if (!std::isfinite(m) || !(m >= std::min(L.surf[k].n_before[l], L.surf[k].n_after[l])))
          return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_coating_stacks: a layer index must be finite and >= the smaller index beside the interface");
      }
      C.layer_nm[(size_t)kept * n_surfaces + k] = d;
      for (int l = 0; l < n_lambda; l++)
        C.layer_index[((size_t)kept * n_lambda + l) * n_surfaces + k] = index[((size_t)j * n_lambda + l) * n_surfaces + k];
      kept++;
    }
    C.n_layers[k] = kept;
    if (kept > 0) C.n++;
    if (kept > 1) C.n_stacked++;
    if (kept == 1) {   // a single film: lf_set_lens_coatings' state, records and kernels
      C.thickness_nm[k] = C.layer_nm[k];
      for (int l = 0; l < n_lambda; l++) C.index[(size_t)l * n_surfaces + k] = C.layer_index[(size_t)l * n_surfaces + k];
    }
  }
  if (C.n == 0) C = LfCoatings{};
  ctx->coat = C;
  ctx->events_dirty = true;
  ctx->lenscam_dirty = true;
  return LF_OK;
}

lf_status lf_get_lens_coating_stacks(lf_ctx* ctx, int n_surfaces, int n_lambda, float* lambda_nm, int* n_layers,
                                     float* thickness_nm, float* index, int* n_stacked) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_get_lens_coating_stacks before lf_set_lens");
  if (n_surfaces != ctx->raw_n || n_lambda != ctx->lens.n_lambda)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_get_lens_coating_stacks: sizes differ from the installed lens");
  const LfCoatings& C = ctx->coat;
  if (lambda_nm) for (int l = 0; l < n_lambda; l++) lambda_nm[l] = C.lambda_nm[l];
  if (n_layers) for (int k = 0; k < n_surfaces; k++) n_layers[k] = C.n_layers[k];
  if (thickness_nm) for (size_t i = 0; i < (size_t)LF_MAX_COAT_LAYERS * n_surfaces; i++) thickness_nm[i] = C.layer_nm[i];
  if (index) for (size_t i = 0; i < (size_t)LF_MAX_COAT_LAYERS * n_lambda * n_surfaces; i++) index[i] = C.layer_index[i];
  if (n_stacked) *n_stacked = C.n_stacked;
  return LF_OK;
}

lf_status lf_coating_stack_reflectance(float n_in, int n_layers, const float* n_film, const float* thickness_nm,
                                       float n_out, float lambda_nm, float cos_in, float out[3]) {
  if (!out || n_layers < 0 || n_layers > LF_MAX_COAT_LAYERS || (n_layers > 0 && (!n_film || !thickness_nm)))
    return LF_ERR_INVALID;
  if (!std::isfinite(n_in) || !std::isfinite(n_out) || !std::isfinite(lambda_nm) || !std::isfinite(cos_in))
    return LF_ERR_INVALID;
  if (!(n_in >= 1.0f) || !(n_out >= 1.0f) || !(lambda_nm > 0.0f) || !(cos_in >= 0.0f) || !(cos_in <= 1.0f))
    return LF_ERR_INVALID;
  float m[LF_MAX_COAT_LAYERS], d[LF_MAX_COAT_LAYERS];
  int N = 0;
  for (int i = 0; i < n_layers; i++) {
    if (!std::isfinite(n_film[i]) || !std::isfinite(thickness_nm[i]) || thickness_nm[i] < 0.0f ||
        thickness_nm[i] > kCoatMaxThicknessNm || !(n_film[i] >= std::min(n_in, n_out)))
      return LF_ERR_INVALID;
    if (thickness_nm[i] == 0.0f) continue;
    m[N] = n_film[i]; d[N] = thickness_nm[i]; N++;
  }
  if (N <= 1) return lf_coating_reflectance(n_in, N ? m[0] : n_in, n_out, N ? d[0] : 0.0f, lambda_nm, cos_in, out);
  // the event's optical cosines, as lf_coating_reflectance
  const float sq = n_in * cos_in;
  const float n2 = n_in * n_in, np2 = n_out * n_out;
  const float k2 = sq * sq + (np2 - n2);
  if (k2 < 0.0f) { out[0] = out[1] = out[2] = 1.0f; return LF_OK; }   // total reflection
  const float ct = std::sqrt(k2);
  float rec[kStackDwords(LF_MAX_COAT_LAYERS)];
  lf_stack_constants(n_in, n_out, N, m, d, lambda_nm, rec);
  struct HostLoad {
    const float* p;
    int operator()(int i) const { int v; std::memcpy(&v, p + i, sizeof(int)); return v; }
  };
  float Rn, Rd, Ns, Ds, Np, Dp;
  lfm::stack_fraction(sq, ct, HostLoad{rec}, Rn, Rd, &Ns, &Ds, &Np, &Dp);
  out[0] = Ns / Ds;
  out[1] = Np / Dp;
  out[2] = Rn / Rd;
  return LF_OK;
}

lf_status lf_coating_reflectance(float n_in, float n_film, float n_out, float thickness_nm, float lambda_nm,
                                 float cos_in, float out[3]) {
  if (!out) return LF_ERR_INVALID;
  if (!std::isfinite(n_in) || !std::isfinite(n_film) || !std::isfinite(n_out) || !std::isfinite(thickness_nm) ||
      !std::isfinite(lambda_nm) || !std::isfinite(cos_in))
    return LF_ERR_INVALID;
  if (!(n_in >= 1.0f) || !(n_out >= 1.0f) || !(lambda_nm > 0.0f) || !(cos_in >= 0.0f) || !(cos_in <= 1.0f) ||
      thickness_nm < 0.0f || thickness_nm > kCoatMaxThicknessNm)
    return LF_ERR_INVALID;
  if (thickness_nm > 0.0f && !(n_film >= std::min(n_in, n_out))) return LF_ERR_INVALID;
  // the event's optical cosines: sq = n |cos t|, ct = n' cos t' = sqrt(sq^2 + n'^2 - n^2) (surface_event)
  const float sq = n_in * cos_in;
  const float n2 = n_in * n_in, np2 = n_out * n_out;
  const float k2 = sq * sq + (np2 - n2);
  if (k2 < 0.0f) { out[0] = out[1] = out[2] = 1.0f; return LF_OK; }   // total reflection
  const float ct = std::sqrt(k2);
  if (thickness_nm == 0.0f) {   // the bare fraction of surface_event<true>
    const float fs = 1.0f / (n_in + n_out), q = std::fmaf(np2, n_in, n2 * n_out), fo = np2 / q, fi = n2 / q;
    const float a = (sq - ct) * fs, b = (sq + ct) * fs;
    const float pc = fi * ct;
    const float A = std::fmaf(fo, sq, -pc), B = std::fmaf(fo, sq, pc);
    const float u = a * B, v = A * b;
    const float Rn = 0.5f * std::fmaf(u, u, v * v), bB = b * B;
    out[0] = (a / b) * (a / b);
    out[1] = (A / B) * (A / B);
    out[2] = Rn / (bB * bB);
    return LF_OK;
  }
  LfCoatK k;
  lf_coat_constants(n_in, n_film, n_out, thickness_nm, lambda_nm, &k);
  float Rn, Rd, Ns, Ds, Np, Dp;
  lfm::coated_fraction(sq, ct, k, Rn, Rd, &Ns, &Ds, &Np, &Dp);
  out[0] = Ns / Ds;
  out[1] = Np / Dp;
  out[2] = Rn / Rd;
  return LF_OK;
}

// ---------------------------------------------------------------- aspheres ----------------------
static lfm::LfAsphRec asph_record(float conic, int n_coef, const float* coef, int stride, int k) {
  lfm::LfAsphRec r{};
  r.kappa = conic;
  for (int m = 0; m < n_coef && m < LF_MAX_ASPH_COEF; m++) r.a[m] = coef ? coef[(size_t)m * stride + k] : 0.0f;
  return r;
}

lf_status lf_set_lens_aspheres(lf_ctx* ctx, int n_surfaces, const float* conic, int n_coef, const float* coef) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_set_lens_aspheres before lf_set_lens");
  if (!conic) {   // every interface a sphere
    ctx->asph = LfAspheres{};
    ctx->events_dirty = true;
    ctx->lenscam_dirty = true;
    return LF_OK;
  }
  if (n_surfaces != ctx->raw_n) return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_aspheres: n_surfaces differs from the installed lens");
  if (n_coef < 0 || n_coef > LF_MAX_ASPH_COEF || (n_coef > 0 && !coef))
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_aspheres: n_coef must be 0 .. LF_MAX_ASPH_COEF (with its array)");
  LfAspheres A;
  for (int k = 0; k < n_surfaces; k++) {
    const std::string who = "lf_set_lens_aspheres: interface " + std::to_string(k);
    bool any = conic[k] != 0.0f, finite = std::isfinite(conic[k]);
    for (int m = 0; m < n_coef; m++) {
      const float a = coef[(size_t)m * n_surfaces + k];
      any = any || a != 0.0f;
      finite = finite && std::isfinite(a);
    }
    if (!finite) return lf_fail(ctx, LF_ERR_INVALID, who + ": a value is not finite");
    if (!any) continue;
    if (k == ctx->raw_stop) return lf_fail(ctx, LF_ERR_INVALID, who + ": the stop cannot carry an aspheric record");
    if (ctx->bic.on[k]) return lf_fail(ctx, LF_ERR_INVALID, who + ": the interface carries a biconic record (lf_set_lens_biconics)");
    // the conic must cover the clear aperture: 1 - (1 + kappa) c^2 h^2 > 0 in the float arithmetic of the sag
    const LfSurfaceDev& s = ctx->lens.surf[k];
    const float kc2 = (1.0f + conic[k]) * (s.curv * s.curv);
    if (!(fmaf(-kc2, s.h2, 1.0f) > 0.0f))
      return lf_fail(ctx, LF_ERR_INVALID, who + ": 1 - (1 + kappa) c^2 h^2 is not positive at its semi-aperture (the conic ends inside the clear aperture)");
    A.kappa[k] = conic[k];
    for (int m = 0; m < n_coef; m++) A.coef[(size_t)m * n_surfaces + k] = coef[(size_t)m * n_surfaces + k];
    A.n++;
  }
  ctx->asph = A;
  ctx->events_dirty = true;
  ctx->lenscam_dirty = true;
  return LF_OK;
}

lf_status lf_get_lens_aspheres(lf_ctx* ctx, int n_surfaces, float* conic, float* coef, int* n_aspheric) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_get_lens_aspheres before lf_set_lens");
  if (n_surfaces != ctx->raw_n) return lf_fail(ctx, LF_ERR_INVALID, "lf_get_lens_aspheres: n_surfaces differs from the installed lens");
  const LfAspheres& A = ctx->asph;
  if (conic) for (int k = 0; k < n_surfaces; k++) conic[k] = A.kappa[k];
  if (coef) for (size_t i = 0; i < (size_t)LF_MAX_ASPH_COEF * n_surfaces; i++) coef[i] = A.coef[i];
  if (n_aspheric) *n_aspheric = A.n;
  return LF_OK;
}

static bool asph_args_ok(float curvature, float conic, int n_coef, const float* coef) {
  if (n_coef < 0 || n_coef > LF_MAX_ASPH_COEF || (n_coef > 0 && !coef)) return false;
  bool finite = std::isfinite(curvature) && std::isfinite(conic);
  for (int m = 0; m < n_coef; m++) finite = finite && std::isfinite(coef[m]);
  return finite;
}

lf_status lf_asphere_sag(float curvature, float conic, int n_coef, const float* coef, float r2, float* z, float* dz_dr2) {
  if (!asph_args_ok(curvature, conic, n_coef, coef) || !(r2 >= 0.0f)) return LF_ERR_INVALID;
  const lfm::LfAsphRec rec = asph_record(conic, n_coef, coef, 1, 0);
  float zz, zp;
  if (!lfm::lf_asph_sag(curvature, rec, r2, zz, zp)) return LF_ERR_INVALID;
  if (z) *z = zz;
  if (dz_dr2) *dz_dr2 = zp;
  return LF_OK;
}

// the sixteen constants of one event as the host twin and the kernel take them: {c, delta, h2, sgn, dzv, 0, 0, 0, record}
static bool asph_event_consts(float curvature, float conic, int n_coef, const float* coef, float semi_aperture, float n_in,
                              float n_out, int reflect, int forward, float dzv, float out[16]) {
  if (!asph_args_ok(curvature, conic, n_coef, coef) || !(semi_aperture > 0.0f) || !std::isfinite(semi_aperture) ||
      !(n_in >= 1.0f) || !(n_out >= 1.0f) || !std::isfinite(n_in) || !std::isfinite(n_out) || !std::isfinite(dzv))
    return false;
  const lfm::LfAsphRec rec = asph_record(conic, n_coef, coef, 1, 0);
  // (float products of the indices, as pack_program forms a row's delta -- a mirror row's too: its ct is the Fresnel code's)
  const float n_in2 = n_in * n_in, n_out2 = n_out * n_out;
  out[0] = curvature; out[1] = n_out2 - n_in2; out[2] = semi_aperture * semi_aperture; out[3] = forward ? 1.0f : -1.0f;
  out[4] = dzv; out[5] = out[6] = out[7] = 0.0f;
  std::memcpy(out + 8, &rec, sizeof(rec));
  return true;
}

lf_status lf_asphere_event(float curvature, float conic, int n_coef, const float* coef, float semi_aperture, float n_in,
                           float n_out, int reflect, int forward, float dzv, const float ray_in[6], float ray_out[6],
                           float* sq, float* ct, int* fate) {
  float k[16];
  if (!ray_in || !ray_out || !fate || !asph_event_consts(curvature, conic, n_coef, coef, semi_aperture, n_in, n_out, reflect, forward, dzv, k))
    return LF_ERR_INVALID;
  lfm::LfAsphRec rec;
  std::memcpy(&rec, k + 8, sizeof(rec));
  float px = ray_in[0], py = ray_in[1], hz = ray_in[2], dx = ray_in[3], dy = ray_in[4], dz = ray_in[5], r2;
  const lfm::AsphHit h = lfm::lf_asph_event(px, py, hz, r2, dx, dy, dz, k[4], k[0], rec, k[1], k[2], reflect != 0, k[3]);
  ray_out[0] = px; ray_out[1] = py; ray_out[2] = hz; ray_out[3] = dx; ray_out[4] = dy; ray_out[5] = dz;
  if (sq) *sq = h.sq;
  if (ct) *ct = h.ct;
  *fate = h.fate;
  return LF_OK;
}

lf_status lf_asphere_events(lf_ctx* ctx, float curvature, float conic, int n_coef, const float* coef, float semi_aperture,
                            float n_in, float n_out, int reflect, int forward, float dzv, size_t n, const float* rays,
                            float* out, int* fates) {
  if (!ctx || (n > 0 && (!rays || !out || !fates))) return LF_ERR_INVALID;
  float k[16];
  if (n > 0x7fffffffull / 8 || !asph_event_consts(curvature, conic, n_coef, coef, semi_aperture, n_in, n_out, reflect, forward, dzv, k))
    return lf_fail(ctx, LF_ERR_INVALID, "lf_asphere_events: constants not finite / out of range, or too many rays for one call");
  if (n == 0) return LF_OK;
  LF_HIP(ctx, hipSetDevice(ctx->device));
  float *d_rays = nullptr, *d_out = nullptr;
  int* d_fates = nullptr;
  hipError_t e = hipMalloc((void**)&d_rays, n * 6 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, n * 8 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_fates, n * sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(d_rays, rays, n * 6 * sizeof(float), hipMemcpyHostToDevice);
  lf_status st = LF_OK;
  if (e == hipSuccess) st = lfk_asphere_events(ctx, k, reflect, forward, n, d_rays, d_out, d_fates);
  if (e == hipSuccess && st == LF_OK) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(out, d_out, n * 8 * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(fates, d_fates, n * sizeof(int), hipMemcpyDeviceToHost);
  if (d_rays) (void)hipFree(d_rays);
  if (d_out) (void)hipFree(d_out);
  if (d_fates) (void)hipFree(d_fates);
  if (st != LF_OK) return st;
  LF_HIP(ctx, e);
  return LF_OK;
}

lf_status lf_march_path_rays(lf_ctx* ctx, int lambda, int i, int j, size_t n, const float* sensor_xy_mm,
                             const float* pupil_uv, float* out) {
  if (!ctx || !sensor_xy_mm || !pupil_uv || !out) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_march_path_rays before lf_set_lens");
  if (!ctx->ap[LF_APERTURE_STARBURST].valid)
    return lf_fail(ctx, LF_ERR_STATE, "aperture mask (LF_APERTURE_STARBURST slot) not set");
  if (lambda < 0 || lambda >= ctx->lens.n_lambda || n > 0x7fffffffull / 8)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_march_path_rays: wavelength index / count out of range");
  const int N = ctx->lens.n_surf, stop = ctx->lens.stop;
  const bool primary = i == -1 && j == -1;
  if (!primary && !(i >= 0 && i < j && j < N && i != stop && j != stop))
    return lf_fail(ctx, LF_ERR_INVALID, "lf_march_path_rays: a pair is two glass interfaces 0 <= i < j < n_surfaces (-1, -1: the primary path)");
  if (n == 0) return LF_OK;
  LF_HIP(ctx, hipSetDevice(ctx->device));
  float *d_xy = nullptr, *d_uv = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc((void**)&d_xy, n * 2 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_uv, n * 2 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, n * 8 * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(d_xy, sensor_xy_mm, n * 2 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_uv, pupil_uv, n * 2 * sizeof(float), hipMemcpyHostToDevice);
  lf_status st = LF_OK;
  if (e == hipSuccess) st = lfk_march_path_rays(ctx, lambda, i, j, (int)n, d_xy, d_uv, d_out);
  if (e == hipSuccess && st == LF_OK) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(out, d_out, n * 8 * sizeof(float), hipMemcpyDeviceToHost);
  if (d_xy) (void)hipFree(d_xy);
  if (d_uv) (void)hipFree(d_uv);
  if (d_out) (void)hipFree(d_out);
  if (st != LF_OK) return st;
  LF_HIP(ctx, e);
  return LF_OK;
}

// ---------------------------------------------------------------- sensor ghosts -----------------
lf_status lf_set_sensor_reflectance(lf_ctx* ctx, int n_lambda, const float* reflectance) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_set_sensor_reflectance before lf_set_lens");
  if (!reflectance) { ctx->sensor.n_refl = 0; return LF_OK; }
  if (n_lambda != ctx->lens.n_lambda)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_sensor_reflectance: one value per index column of the installed lens");
  for (int l = 0; l < n_lambda; l++)
    if (!std::isfinite(reflectance[l]) || reflectance[l] < 0.0f || reflectance[l] > 1.0f)
      return lf_fail(ctx, LF_ERR_INVALID, "lf_set_sensor_reflectance: a reflectance is a finite number in [0, 1]");
  for (int l = 0; l < n_lambda; l++) ctx->sensor.refl[l] = reflectance[l];
  ctx->sensor.n_refl = n_lambda;
  return LF_OK;
}

lf_status lf_get_sensor_reflectance(lf_ctx* ctx, int n_lambda, float* reflectance, int* installed) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_get_sensor_reflectance before lf_set_lens");
  if (installed) *installed = ctx->sensor.n_refl > 0 ? 1 : 0;
  if (reflectance) {
    if (n_lambda != ctx->lens.n_lambda)
      return lf_fail(ctx, LF_ERR_INVALID, "lf_get_sensor_reflectance: one value per index column of the installed lens");
    for (int l = 0; l < n_lambda; l++) reflectance[l] = ctx->sensor.n_refl > 0 ? ctx->sensor.refl[l] : 0.0f;
  }
  return LF_OK;
}

lf_status lf_set_sensor_ghosts(lf_ctx* ctx, int mode, const int* interfaces, int n) {
  if (!ctx) return LF_ERR_INVALID;
  if (mode != LF_SENSOR_GHOSTS_OFF && mode != LF_SENSOR_GHOSTS_ADD && mode != LF_SENSOR_GHOSTS_ONLY)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_sensor_ghosts: the mode is LF_SENSOR_GHOSTS_OFF, _ADD or _ONLY");
  if (!interfaces) {
    ctx->sensor.mode = mode;
    ctx->sensor.n_sel = -1;
    return LF_OK;
  }
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_set_sensor_ghosts with a list of interfaces before lf_set_lens");
  if (n < 1 || n > LF_MAX_SURFACES) return lf_fail(ctx, LF_ERR_INVALID, "lf_set_sensor_ghosts: the list holds 1 .. LF_MAX_SURFACES interfaces");
  for (int q = 0; q < n; q++) {
    if (interfaces[q] < 0 || interfaces[q] >= ctx->lens.n_surf || interfaces[q] == ctx->lens.stop)
      return lf_fail(ctx, LF_ERR_INVALID, "lf_set_sensor_ghosts: an interface is a glass interface 0 <= i < n_surfaces, never the stop");
    for (int r = 0; r < q; r++)
      if (interfaces[r] == interfaces[q]) return lf_fail(ctx, LF_ERR_INVALID, "lf_set_sensor_ghosts: an interface is listed twice");
  }
  ctx->sensor.mode = mode;
  ctx->sensor.n_sel = n;
  for (int q = 0; q < n; q++) ctx->sensor.sel[q] = interfaces[q];
  return LF_OK;
}

lf_status lf_get_sensor_ghosts(lf_ctx* ctx, int* mode, int* interfaces, int cap, int* n) {
  if (!ctx) return LF_ERR_INVALID;
  if (mode) *mode = ctx->sensor.mode;
  if (!interfaces && !n) return LF_OK;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_get_sensor_ghosts: the selection is resolved against a lens (lf_set_lens)");
  int sel[LF_MAX_SURFACES];
  const int m = lf_sensor_selection(ctx, sel);
  if (m < 0) return lf_fail(ctx, LF_ERR_STATE, "lf_get_sensor_ghosts: the selection does not fit the installed lens");
  if (n) *n = m;
  if (interfaces) {
    if (cap < m) return lf_fail(ctx, LF_ERR_INVALID, "lf_get_sensor_ghosts: the list does not fit");
    for (int q = 0; q < m; q++) interfaces[q] = sel[q];
  }
  return LF_OK;
}

lf_status lf_set_sensor_ghost_surfaces(lf_ctx* ctx, int which) {
  if (!ctx) return LF_ERR_INVALID;
  if (which != LF_SENSOR_SURFACES_CENTRED && which != LF_SENSOR_SURFACES_POSED)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_sensor_ghost_surfaces: LF_SENSOR_SURFACES_CENTRED (0) or LF_SENSOR_SURFACES_POSED (1)");
  ctx->sensor.surfaces = which;   // (the table's dirty test is by content: nothing to mark)
  return LF_OK;
}

lf_status lf_get_sensor_ghost_surfaces(lf_ctx* ctx, int* which) {
  if (!ctx || !which) return LF_ERR_INVALID;
  *which = ctx->sensor.surfaces;
  return LF_OK;
}

lf_status lf_sensor_path_sequence(int n_surfaces, int stop_index, int i, int* out, int cap, int* n_events) {
  if (n_surfaces < 1 || n_surfaces > LF_MAX_SURFACES || stop_index < -1 || stop_index >= n_surfaces || !out || !n_events)
    return LF_ERR_INVALID;
  if (i < 0 || i >= n_surfaces || i == stop_index) return LF_ERR_INVALID;
  const int n = n_surfaces, total = 3 * n - 2 * i;
  if (cap < total) return LF_ERR_INVALID;
  int m = 0;
  for (int k = n - 1; k > i; k--) out[m++] = k;
  out[m++] = i | 1 << 8;
  for (int k = i + 1; k < n; k++) out[m++] = k | 1 << 9;
  out[m++] = n | 1 << 8 | 1 << 9;          // the sensor's mirror, met travelling +z
  for (int k = n - 1; k >= 0; k--) out[m++] = k;
  *n_events = m;
  return LF_OK;
}

lf_status lf_sensor_mirror_event(const float ray_in[6], float dzv, float half_width_mm, float half_height_mm, float ray_out[6],
                                 int* inside) {
  if (!ray_in || !ray_out || !inside) return LF_ERR_INVALID;
  float px = ray_in[0], py = ray_in[1], hz = ray_in[2], dx = ray_in[3], dy = ray_in[4], dz = ray_in[5], r2;
  *inside = lfm::lf_sensor_mirror(px, py, hz, r2, dx, dy, dz, dzv, half_width_mm, half_height_mm) ? 1 : 0;
  ray_out[0] = px; ray_out[1] = py; ray_out[2] = hz; ray_out[3] = dx; ray_out[4] = dy; ray_out[5] = dz;
  return LF_OK;
}

lf_status lf_march_sensor_path_rays(lf_ctx* ctx, int lambda, int i, size_t n, const float* sensor_xy_mm, const float* pupil_uv,
                                    float* out) {
  if (!ctx || !sensor_xy_mm || !pupil_uv || !out) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_march_sensor_path_rays before lf_set_lens");
  if (!ctx->ap[LF_APERTURE_STARBURST].valid)
    return lf_fail(ctx, LF_ERR_STATE, "aperture mask (LF_APERTURE_STARBURST slot) not set");
  if (ctx->sensor.n_refl == 0)
    return lf_fail(ctx, LF_ERR_STATE, "lf_march_sensor_path_rays: the sensor has no reflectance (lf_set_sensor_reflectance)");
  if (ctx->pose.n > 0 && ctx->sensor.surfaces != LF_SENSOR_SURFACES_POSED)   // (as lf_trace_ghosts refuses the frame)
    return lf_fail(ctx, LF_ERR_UNSUPPORTED, "lf_march_sensor_path_rays: sensor paths are not marched through a lens with posed "
                                            "interfaces (lf_set_lens_poses) under LF_SENSOR_SURFACES_CENTRED; "
                                            "lf_set_sensor_ghost_surfaces(LF_SENSOR_SURFACES_POSED) marches them");
  if (lambda < 0 || lambda >= ctx->lens.n_lambda || n > 0x7fffffffull / 8)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_march_sensor_path_rays: wavelength index / count out of range");
  if (i < 0 || i >= ctx->lens.n_surf || i == ctx->lens.stop)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_march_sensor_path_rays: the mirror is a glass interface 0 <= i < n_surfaces, never the stop");
  if (n == 0) return LF_OK;
  LF_HIP(ctx, hipSetDevice(ctx->device));
  float *d_xy = nullptr, *d_uv = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc((void**)&d_xy, n * 2 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_uv, n * 2 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, n * 8 * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(d_xy, sensor_xy_mm, n * 2 * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_uv, pupil_uv, n * 2 * sizeof(float), hipMemcpyHostToDevice);
  lf_status st = LF_OK;
  if (e == hipSuccess) st = lfk_march_sensor_path_rays(ctx, lambda, i, (int)n, d_xy, d_uv, d_out);
  if (e == hipSuccess && st == LF_OK) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(out, d_out, n * 8 * sizeof(float), hipMemcpyDeviceToHost);
  if (d_xy) (void)hipFree(d_xy);
  if (d_uv) (void)hipFree(d_uv);
  if (d_out) (void)hipFree(d_out);
  if (st != LF_OK) return st;
  LF_HIP(ctx, e);
  return LF_OK;
}

lf_status lf_get_sensor_ghost_stats(lf_ctx* ctx, uint64_t out[4]) {
  if (!ctx || !out) return LF_ERR_INVALID;
  for (int k = 0; k < kSensorStats; k++) out[k] = 0;
  if (!ctx->sensor.stats_dev) return LF_OK;      // (no sensor launch yet)
  unsigned long long c[kSensorStats];
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LF_HIP(ctx, hipMemcpy(c, ctx->sensor.stats_dev, sizeof(c), hipMemcpyDeviceToHost));
  for (int k = 0; k < kSensorStats; k++) out[k] = c[k];
  return LF_OK;
}

// ---------------------------------------------------------------- biconic interfaces ------------
lf_status lf_set_lens_biconics(lf_ctx* ctx, int n_surfaces, const int* on, const float* radius_x, const float* conic_x,
                               const float* conic_y) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_set_lens_biconics before lf_set_lens");
  if (!on) {   // every interface a surface of revolution
    ctx->bic = LfBiconics{};
    ctx->events_dirty = true;
    ctx->lenscam_dirty = true;
    return LF_OK;
  }
  if (n_surfaces != ctx->raw_n) return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_biconics: n_surfaces differs from the installed lens");
  if (!radius_x) return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_biconics: radius_x is NULL");
  LfBiconics B;
  for (int k = 0; k < n_surfaces; k++) {
    if (!on[k]) continue;
    const std::string who = "lf_set_lens_biconics: interface " + std::to_string(k);
    const float rx = radius_x[k], kx = conic_x ? conic_x[k] : 0.0f, ky = conic_y ? conic_y[k] : 0.0f;
    if (!std::isfinite(rx) || !std::isfinite(kx) || !std::isfinite(ky)) return lf_fail(ctx, LF_ERR_INVALID, who + ": a value is not finite");
    if (k == ctx->raw_stop) return lf_fail(ctx, LF_ERR_INVALID, who + ": the stop cannot carry a biconic record");
    bool asph = ctx->asph.kappa[k] != 0.0f;
    for (int m = 0; m < LF_MAX_ASPH_COEF; m++) asph = asph || ctx->asph.coef[(size_t)m * n_surfaces + k] != 0.0f;
    if (asph) return lf_fail(ctx, LF_ERR_INVALID, who + ": the interface carries an aspheric record (lf_set_lens_aspheres)");
    // either meridian's conic must cover the clear aperture: 1 - (1 + k) c^2 h^2 > 0 in the float arithmetic of the sag
    // (on the disc x^2 + y^2 <= h^2 the root's argument is smallest on the axis of the larger (1 + k) c^2)
    const LfSurfaceDev& s = ctx->lens.surf[k];
    const float cx = rx == 0.0f ? 0.0f : 1.0f / rx;
    if (!(fmaf(-((1.0f + kx) * cx * cx), s.h2, 1.0f) > 0.0f))
      return lf_fail(ctx, LF_ERR_INVALID, who + ": 1 - (1 + kx) cx^2 h^2 is not positive at its semi-aperture (the x meridian's conic ends inside the clear aperture)");
    if (!(fmaf(-((1.0f + ky) * s.curv * s.curv), s.h2, 1.0f) > 0.0f))
      return lf_fail(ctx, LF_ERR_INVALID, who + ": 1 - (1 + ky) cy^2 h^2 is not positive at its semi-aperture (the y meridian's conic ends inside the clear aperture)");
    B.on[k] = 1; B.rx[k] = rx; B.kx[k] = kx; B.ky[k] = ky;
    B.n++;
  }
  ctx->bic = B;
  ctx->events_dirty = true;
  ctx->lenscam_dirty = true;
  return LF_OK;
}

lf_status lf_get_lens_biconics(lf_ctx* ctx, int n_surfaces, int* on, float* radius_x, float* conic_x, float* conic_y,
                               int* n_biconic) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_get_lens_biconics before lf_set_lens");
  if (n_surfaces != ctx->raw_n) return lf_fail(ctx, LF_ERR_INVALID, "lf_get_lens_biconics: n_surfaces differs from the installed lens");
  const LfBiconics& B = ctx->bic;
  for (int k = 0; k < n_surfaces; k++) {
    if (on) on[k] = B.on[k];
    if (radius_x) radius_x[k] = B.rx[k];
    if (conic_x) conic_x[k] = B.kx[k];
    if (conic_y) conic_y[k] = B.ky[k];
  }
  if (n_biconic) *n_biconic = B.n;
  return LF_OK;
}

lf_status lf_get_lens_meridian_scales(lf_ctx* ctx, double* scale_x, double* scale_y) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_get_lens_meridian_scales before lf_set_lens");
  float rx[LF_MAX_SURFACES];
  meridian_x_radii(ctx, rx);
  const float* ior = ctx->raw_ior + (size_t)(ctx->lens.n_lambda / 2) * ctx->raw_n;
  double sx = 0.0, sy = 0.0;
  if (!paraxial_image_scale(ctx->raw_n, ctx->raw_stop, ctx->raw_radius, ctx->raw_thickness, ior, &sy) ||
      !paraxial_image_scale(ctx->raw_n, ctx->raw_stop, rx, ctx->raw_thickness, ior, &sx))
    return lf_fail(ctx, LF_ERR_INVALID, "lf_get_lens_meridian_scales: a meridian of the prescription images no distant point on its sensor");
  if (scale_x) *scale_x = sx;
  if (scale_y) *scale_y = sy;
  return LF_OK;
}

static bool bic_args_ok(float cx, float cy, float kx, float ky) {
  return std::isfinite(cx) && std::isfinite(cy) && std::isfinite(kx) && std::isfinite(ky);
}

lf_status lf_biconic_sag(float curvature_x, float curvature_y, float conic_x, float conic_y, float x, float y, float* z,
                         float* dz_dx, float* dz_dy) {
  if (!bic_args_ok(curvature_x, curvature_y, conic_x, conic_y) || !std::isfinite(x) || !std::isfinite(y)) return LF_ERR_INVALID;
  float zz, zx, zy;
  if (!lfm::lf_bic_sag(curvature_x, curvature_y, conic_x, conic_y, x, y, zz, zx, zy)) return LF_ERR_INVALID;
  if (z) *z = zz;
  if (dz_dx) *dz_dx = zx;
  if (dz_dy) *dz_dy = zy;
  return LF_OK;
}

// the sixteen constants of one event as the host twin and the kernel take them: {cy, delta, h2, sgn, dzv, 0, 0, 0, cx, kx, ky, 0 ..}
static bool bic_event_consts(float cx, float cy, float kx, float ky, float semi_aperture, float n_in, float n_out, int forward,
                             float dzv, float out[16]) {
  if (!bic_args_ok(cx, cy, kx, ky) || !(semi_aperture > 0.0f) || !std::isfinite(semi_aperture) || !(n_in >= 1.0f) ||
      !(n_out >= 1.0f) || !std::isfinite(n_in) || !std::isfinite(n_out) || !std::isfinite(dzv))
    return false;
  const float n_in2 = n_in * n_in, n_out2 = n_out * n_out;   // (as pack_program forms a row's delta)
  for (int i = 0; i < 16; i++) out[i] = 0.0f;
  out[0] = cy; out[1] = n_out2 - n_in2; out[2] = semi_aperture * semi_aperture; out[3] = forward ? 1.0f : -1.0f;
  out[4] = dzv; out[8] = cx; out[9] = kx; out[10] = ky;
  return true;
}

lf_status lf_biconic_event(float curvature_x, float curvature_y, float conic_x, float conic_y, float semi_aperture, float n_in,
                           float n_out, int reflect, int forward, float dzv, const float ray_in[6], float ray_out[6],
                           float* sq, float* ct, int* fate) {
  float k[16];
  if (!ray_in || !ray_out || !fate || !bic_event_consts(curvature_x, curvature_y, conic_x, conic_y, semi_aperture, n_in, n_out, forward, dzv, k))
    return LF_ERR_INVALID;
  const lfm::LfBicRec rec{k[8], k[9], k[10], {}};
  float px = ray_in[0], py = ray_in[1], hz = ray_in[2], dx = ray_in[3], dy = ray_in[4], dz = ray_in[5], r2;
  const lfm::AsphHit h = lfm::lf_bic_event(px, py, hz, r2, dx, dy, dz, k[4], k[0], rec, k[1], k[2], reflect != 0, k[3]);
  ray_out[0] = px; ray_out[1] = py; ray_out[2] = hz; ray_out[3] = dx; ray_out[4] = dy; ray_out[5] = dz;
  if (sq) *sq = h.sq;
  if (ct) *ct = h.ct;
  *fate = h.fate;
  return LF_OK;
}

lf_status lf_biconic_events(lf_ctx* ctx, float curvature_x, float curvature_y, float conic_x, float conic_y, float semi_aperture,
                            float n_in, float n_out, int reflect, int forward, float dzv, size_t n, const float* rays,
                            float* out, int* fates) {
  if (!ctx || (n > 0 && (!rays || !out || !fates))) return LF_ERR_INVALID;
  float k[16];
  if (n > 0x7fffffffull / 8 || !bic_event_consts(curvature_x, curvature_y, conic_x, conic_y, semi_aperture, n_in, n_out, forward, dzv, k))
    return lf_fail(ctx, LF_ERR_INVALID, "lf_biconic_events: constants not finite / out of range, or too many rays for one call");
  if (n == 0) return LF_OK;
  LF_HIP(ctx, hipSetDevice(ctx->device));
  float *d_rays = nullptr, *d_out = nullptr;
  int* d_fates = nullptr;
  hipError_t e = hipMalloc((void**)&d_rays, n * 6 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, n * 8 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_fates, n * sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(d_rays, rays, n * 6 * sizeof(float), hipMemcpyHostToDevice);
  lf_status st = LF_OK;
  if (e == hipSuccess) st = lfk_biconic_events(ctx, k, reflect, n, d_rays, d_out, d_fates);
  if (e == hipSuccess && st == LF_OK) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(out, d_out, n * 8 * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(fates, d_fates, n * sizeof(int), hipMemcpyDeviceToHost);
  if (d_rays) (void)hipFree(d_rays);
  if (d_out) (void)hipFree(d_out);
  if (d_fates) (void)hipFree(d_fates);
  if (st != LF_OK) return st;
  LF_HIP(ctx, e);
  return LF_OK;
}

// ---------------------------------------------------------------- posed interfaces --------------
lf_status lf_set_lens_poses(lf_ctx* ctx, int n_surfaces, const int* on, const float* decentre, const float* tilt_deg) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_set_lens_poses before lf_set_lens");
  if (!on) {   // every interface centred
    ctx->pose = LfPoses{};
    ctx->events_dirty = true;
    ctx->lenscam_dirty = true;
    return LF_OK;
  }
  if (n_surfaces != ctx->raw_n) return lf_fail(ctx, LF_ERR_INVALID, "lf_set_lens_poses: n_surfaces differs from the installed lens");
  LfPoses P;
  for (int k = 0; k < n_surfaces; k++) {
    if (!on[k]) continue;
    const std::string who = "lf_set_lens_poses: interface " + std::to_string(k);
    float t[3], a[3];
    for (int m = 0; m < 3; m++) {
      t[m] = decentre ? decentre[3 * k + m] : 0.0f;
      a[m] = tilt_deg ? tilt_deg[3 * k + m] : 0.0f;
      if (!std::isfinite(t[m]) || !std::isfinite(a[m])) return lf_fail(ctx, LF_ERR_INVALID, who + ": a value is not finite");
    }
    if (k == ctx->raw_stop) return lf_fail(ctx, LF_ERR_INVALID, who + ": the stop cannot carry a pose record");
    if (!(std::fabs(a[0]) <= 30.0f) || !(std::fabs(a[1]) <= 30.0f))
      return lf_fail(ctx, LF_ERR_INVALID, who + ": |ax| and |ay| are at most 30 degrees");
    if (!(std::fabs(a[2]) <= 180.0f)) return lf_fail(ctx, LF_ERR_INVALID, who + ": az lies in [-180, 180] degrees");
    P.on[k] = 1;
    for (int m = 0; m < 3; m++) { P.t[3 * k + m] = t[m]; P.a[3 * k + m] = a[m]; }
    P.n++;
  }
  ctx->pose = P;
  ctx->events_dirty = true;
  ctx->lenscam_dirty = true;
  return LF_OK;
}

lf_status lf_get_lens_poses(lf_ctx* ctx, int n_surfaces, int* on, float* decentre, float* tilt_deg, int* n_posed) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_get_lens_poses before lf_set_lens");
  if (n_surfaces != ctx->raw_n) return lf_fail(ctx, LF_ERR_INVALID, "lf_get_lens_poses: n_surfaces differs from the installed lens");
  const LfPoses& P = ctx->pose;
  for (int k = 0; k < n_surfaces; k++) {
    if (on) on[k] = P.on[k];
    for (int m = 0; m < 3; m++) {
      if (decentre) decentre[3 * k + m] = P.t[3 * k + m];
      if (tilt_deg) tilt_deg[3 * k + m] = P.a[3 * k + m];
    }
  }
  if (n_posed) *n_posed = P.n;
  return LF_OK;
}

// the constants of one posed event as the host twin and the kernel take them: lf_biconic_event's sixteen (with the whole
// aspheric record in 8 .. 14 where aspheric), and the pose {R row-major, t, 0 ..}
static bool pose_event_consts(float cx, float cy, float kx, float ky, int aspheric, float kappa, const float* coef, int n_coef,
                              const float decentre[3], const float tilt_deg[3], float semi_aperture, float n_in, float n_out,
                              int forward, float dzv, float k[16], float pose[16]) {
  if (!decentre || !tilt_deg || n_coef < 0 || n_coef > LF_MAX_ASPH_COEF || (n_coef > 0 && !coef)) return false;
  if (!bic_event_consts(cx, cy, kx, ky, semi_aperture, n_in, n_out, forward, dzv, k)) return false;
  for (int m = 0; m < 3; m++)
    if (!std::isfinite(decentre[m]) || !std::isfinite(tilt_deg[m])) return false;
  if (aspheric) {
    if (!std::isfinite(kappa)) return false;
    k[8] = kappa; k[9] = k[10] = 0.0f;
    for (int m = 0; m < n_coef; m++) {
      if (!std::isfinite(coef[m])) return false;
      k[9 + m] = coef[m];
    }
  }
  const lfm::LfPoseRec p = lfm::lf_pose_make(decentre[0], decentre[1], decentre[2], tilt_deg[0], tilt_deg[1], tilt_deg[2]);
  for (int m = 0; m < 16; m++) pose[m] = 0.0f;
  for (int m = 0; m < 9; m++) pose[m] = p.r[m];
  for (int m = 0; m < 3; m++) pose[9 + m] = p.t[m];
  return true;
}

lf_status lf_pose_event(float curvature_x, float curvature_y, float conic_x, float conic_y, int aspheric, float kappa,
                        const float* coef, int n_coef, const float decentre[3], const float tilt_deg[3], float semi_aperture,
                        float n_in, float n_out, int reflect, int forward, float dzv, const float ray_in[6], float ray_out[6],
                        float* sq, float* ct, int* fate) {
  float k[16], pose[16];
  if (!ray_in || !ray_out || !fate ||
      !pose_event_consts(curvature_x, curvature_y, conic_x, conic_y, aspheric, kappa, coef, n_coef, decentre, tilt_deg, semi_aperture,
                         n_in, n_out, forward, dzv, k, pose))
    return LF_ERR_INVALID;
  lfm::LfAsphRec ka;
  ka.kappa = k[8];
  for (int m = 0; m < 6; m++) ka.a[m] = k[9 + m];
  ka.spare = 0.0f;
  const lfm::LfBicRec kb{k[8], k[9], k[10], {}};
  lfm::LfPoseRec p{};
  for (int m = 0; m < 9; m++) p.r[m] = pose[m];
  for (int m = 0; m < 3; m++) p.t[m] = pose[9 + m];
  float px = ray_in[0], py = ray_in[1], hz = ray_in[2], dx = ray_in[3], dy = ray_in[4], dz = ray_in[5], r2;
  const lfm::AsphHit h = lfm::lf_pose_event(px, py, hz, r2, dx, dy, dz, k[4], k[0], aspheric != 0, ka, kb, p, k[1], k[2], reflect != 0, k[3]);
  ray_out[0] = px; ray_out[1] = py; ray_out[2] = hz; ray_out[3] = dx; ray_out[4] = dy; ray_out[5] = dz;
  if (sq) *sq = h.sq;
  if (ct) *ct = h.ct;
  *fate = h.fate;
  return LF_OK;
}

lf_status lf_pose_events(lf_ctx* ctx, float curvature_x, float curvature_y, float conic_x, float conic_y, int aspheric, float kappa,
                         const float* coef, int n_coef, const float decentre[3], const float tilt_deg[3], float semi_aperture,
                         float n_in, float n_out, int reflect, int forward, float dzv, size_t n, const float* rays, float* out,
                         int* fates) {
  if (!ctx || (n > 0 && (!rays || !out || !fates))) return LF_ERR_INVALID;
  float k[16], pose[16];
  if (n > 0x7fffffffull / 8 ||
      !pose_event_consts(curvature_x, curvature_y, conic_x, conic_y, aspheric, kappa, coef, n_coef, decentre, tilt_deg, semi_aperture,
                         n_in, n_out, forward, dzv, k, pose))
    return lf_fail(ctx, LF_ERR_INVALID, "lf_pose_events: constants not finite / out of range, or too many rays for one call");
  if (n == 0) return LF_OK;
  LF_HIP(ctx, hipSetDevice(ctx->device));
  float *d_rays = nullptr, *d_out = nullptr;
  int* d_fates = nullptr;
  hipError_t e = hipMalloc((void**)&d_rays, n * 6 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_out, n * 8 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_fates, n * sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(d_rays, rays, n * 6 * sizeof(float), hipMemcpyHostToDevice);
  lf_status st = LF_OK;
  if (e == hipSuccess) st = lfk_pose_events(ctx, k, pose, reflect, aspheric, n, d_rays, d_out, d_fates);
  if (e == hipSuccess && st == LF_OK) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(out, d_out, n * 8 * sizeof(float), hipMemcpyDeviceToHost);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(fates, d_fates, n * sizeof(int), hipMemcpyDeviceToHost);
  if (d_rays) (void)hipFree(d_rays);
  if (d_out) (void)hipFree(d_out);
  if (d_fates) (void)hipFree(d_fates);
  if (st != LF_OK) return st;
  LF_HIP(ctx, e);
  return LF_OK;
}

// ---------------------------------------------------------------- lens file ---------------------
lf_status lf_load_lens_file(lf_ctx* ctx, const char* path) {
  if (!ctx || !path) return LF_ERR_INVALID;
  FILE* f = std::fopen(path, "r");
  if (!f) return lf_fail(ctx, LF_ERR_INVALID, std::string("lf_load_lens_file: cannot open ") + path);
  // rows: radius thickness n_1 ... n_L semi_aperture; '#' starts a comment; radius 0 with index 0 = the stop
  // optional: `lambda_nm l_1 .. l_L` (the wavelengths of the index columns) and
  // `coating k thickness_nm m_1 .. m_L | m` (a film on interface k: lf_set_lens_coatings; needs lambda_nm)
  // `layer k thickness_nm m_1 .. m_L | m` (appends a layer to interface k's stack, scene side first:
  // lf_set_lens_coating_stacks; needs lambda_nm; not on an interface with a `coating` line)
  // `asphere k kappa [A4 [A6 ...]]` (interface k's conic constant and even coefficients: lf_set_lens_aspheres)
  // `biconic k Rx [kx [ky]]` (interface k's x-meridian radius, 0 = flat in x, and conic constants: lf_set_lens_biconics)
  // `pose k dx dy dz ax ay az` (interface k's decentre in mm and tilt in degrees: lf_set_lens_poses)
  std::vector<std::vector<double>> rows, coats, layers, asphs, bics, sens, poses;
  std::vector<double> lambdas;
  bool lambda_line = false, lambda_bad = false;
  double sensor_w = 36.0;
  char line[1024];
  bool bad = false;
  while (std::fgets(line, sizeof(line), f)) {
    if (char* h = std::strchr(line, '#')) *h = 0;
    std::vector<double> v;
    char* p = line;
    int keyword = 0;   // 1 sensor_width_mm, 2 lambda_nm, 3 coating, 4 layer, 5 asphere, 6 biconic, 7 sensor_reflectance, 8 pose
    while (*p) {
      while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') p++;
      if (!*p) break;
      if (v.empty() && !keyword && std::strncmp(p, "sensor_reflectance", 18) == 0) { keyword = 7; p += 18; continue; }
      if (v.empty() && !keyword && std::strncmp(p, "sensor_width_mm", 15) == 0) { keyword = 1; p += 15; continue; }
      if (v.empty() && !keyword && std::strncmp(p, "lambda_nm", 9) == 0) { keyword = 2; p += 9; continue; }
      if (v.empty() && !keyword && std::strncmp(p, "coating", 7) == 0) { keyword = 3; p += 7; continue; }
      if (v.empty() && !keyword && std::strncmp(p, "layer", 5) == 0) { keyword = 4; p += 5; continue; }
      if (v.empty() && !keyword && std::strncmp(p, "asphere", 7) == 0) { keyword = 5; p += 7; continue; }
      if (v.empty() && !keyword && std::strncmp(p, "biconic", 7) == 0) { keyword = 6; p += 7; continue; }
      if (v.empty() && !keyword && std::strncmp(p, "pose", 4) == 0) { keyword = 8; p += 4; continue; }
      char* e = nullptr;
      const double d = std::strtod(p, &e);
      if (e == p) {
        // (the wavelengths are only read for a file with coatings: anything on the line is accepted otherwise)
        if (keyword == 2) { lambda_bad = true; break; }
        bad = true; break;
      }
      v.push_back(d);
      p = e;
    }
    if (bad) break;
    if (keyword == 2) { lambda_line = true; lambdas = v; continue; }
    if (keyword == 3) { coats.push_back(v); continue; }
    if (keyword == 4) { layers.push_back(v); continue; }
    if (keyword == 5) { asphs.push_back(v); continue; }
    if (keyword == 6) { bics.push_back(v); continue; }
    if (keyword == 7) { sens.push_back(v); continue; }
    if (keyword == 8) { poses.push_back(v); continue; }
    if (keyword == 1) { if (v.size() != 1) { bad = true; break; } sensor_w = v[0]; continue; }
    if (!v.empty()) rows.push_back(v);
  }
  std::fclose(f);
  const int n = (int)rows.size();
  if (bad || n < 1 || n > LF_MAX_SURFACES) return lf_fail(ctx, LF_ERR_INVALID, "lf_load_lens_file: malformed prescription");
  const int nl = (int)rows[0].size() - 3;
  if (nl < 1 || nl > LF_MAX_LAMBDA) return lf_fail(ctx, LF_ERR_INVALID, "lf_load_lens_file: a row is radius thickness n_1..n_L semi_aperture");
  float radius[LF_MAX_SURFACES], thick[LF_MAX_SURFACES], semi[LF_MAX_SURFACES], ior[LF_MAX_LAMBDA * LF_MAX_SURFACES];
  int stop = -1;
  for (int k = 0; k < n; k++) {
    if ((int)rows[k].size() != nl + 3) return lf_fail(ctx, LF_ERR_INVALID, "lf_load_lens_file: rows of different length");
    radius[k] = (float)rows[k][0]; thick[k] = (float)rows[k][1]; semi[k] = (float)rows[k][nl + 2];
    const bool is_stop = rows[k][0] == 0 && rows[k][2] == 0;
    if (is_stop && stop < 0) stop = k;
    for (int l = 0; l < nl; l++) ior[l * n + k] = (is_stop && stop == k) ? 1.0f : (float)rows[k][2 + l];
  }
  // `sensor_reflectance r_1 .. r_L | r` (the sensor's reflectance per index column: lf_set_sensor_reflectance; once)
  float srefl[LF_MAX_LAMBDA] = {};
  if (!sens.empty()) {
    const std::vector<double>& c = sens[0];
    bool ok = sens.size() == 1 && ((int)c.size() == 1 || (int)c.size() == nl);
    for (size_t m = 0; ok && m < c.size(); m++) ok = c[m] >= 0.0 && c[m] <= 1.0;   // (false for a NaN)
    if (!ok)
      return lf_fail(ctx, LF_ERR_INVALID, "lf_load_lens_file: a sensor_reflectance line is `sensor_reflectance r_1 .. r_L` or `sensor_reflectance r`, each in [0, 1] (once)");
    for (int l = 0; l < nl; l++) srefl[l] = (float)c[c.size() == 1 ? 0 : (size_t)l];
  }
  float lam[LF_MAX_LAMBDA] = {}, cth[LF_MAX_SURFACES] = {}, cidx[LF_MAX_LAMBDA * LF_MAX_SURFACES] = {};
  bool has_coating[LF_MAX_SURFACES] = {};   // interface k has a `coating` line (whatever its thickness)
  if (!coats.empty() || !layers.empty()) {
    if (!lambda_line || lambda_bad || (int)lambdas.size() != nl)
      return lf_fail(ctx, LF_ERR_INVALID, "lf_load_lens_file: coating / layer lines need a lambda_nm line with one wavelength per index column");
    for (int l = 0; l < nl; l++) lam[l] = (float)lambdas[l];
    for (const auto& c : coats) {
      const int k = c.size() >= 3 ? (int)c[0] : -1;
      if (k < 0 || k >= n || (double)k != c[0] || ((int)c.size() != 3 && (int)c.size() != nl + 2) || cth[k] != 0.0f)
        return lf_fail(ctx, LF_ERR_INVALID, "lf_load_lens_file: a coating line is `coating k thickness_nm m_1 .. m_L` or `coating k thickness_nm m` (once per interface)");
      cth[k] = (float)c[1];
      has_coating[k] = true;
      for (int l = 0; l < nl; l++) cidx[l * n + k] = (float)c[(int)c.size() == 3 ? 2 : 2 + l];
    }
  }
  // the stacks: a `coating` line is a stack of one layer (installed as that film: lf_set_lens_coating_stacks)
  std::vector<int> nlay((size_t)n, 0);
  std::vector<float> lth((size_t)LF_MAX_COAT_LAYERS * n, 0.0f), lidx((size_t)LF_MAX_COAT_LAYERS * nl * n, 0.0f);
  for (const auto& c : layers) {
    const int k = c.size() >= 3 ? (int)c[0] : -1;
    if (k < 0 || k >= n || (double)k != c[0] || ((int)c.size() != 3 && (int)c.size() != nl + 2) || has_coating[k] ||
        nlay[(size_t)k] >= LF_MAX_COAT_LAYERS)
      return lf_fail(ctx, LF_ERR_INVALID, "lf_load_lens_file: a layer line is `layer k thickness_nm m_1 .. m_L` or `layer k thickness_nm m`, at most LF_MAX_COAT_LAYERS per interface and none beside a coating line");
    const int j = nlay[(size_t)k]++;
    lth[(size_t)j * n + k] = (float)c[1];
    for (int l = 0; l < nl; l++) lidx[((size_t)j * nl + l) * n + k] = (float)c[(int)c.size() == 3 ? 2 : 2 + l];
  }
  if (!layers.empty())
    for (int k = 0; k < n; k++)
      if (cth[k] != 0.0f) {
        nlay[(size_t)k] = 1;
        lth[(size_t)k] = cth[k];
        for (int l = 0; l < nl; l++) lidx[(size_t)l * n + k] = cidx[l * n + k];
      }
  float akappa[LF_MAX_SURFACES] = {}, acoef[LF_MAX_ASPH_COEF * LF_MAX_SURFACES] = {};
  bool has_asph[LF_MAX_SURFACES] = {};
  for (const auto& c : asphs) {
    const int k = c.size() >= 2 ? (int)c[0] : -1;
    if (k < 0 || k >= n || (double)k != c[0] || (int)c.size() > 2 + LF_MAX_ASPH_COEF || has_asph[k])
      return lf_fail(ctx, LF_ERR_INVALID, "lf_load_lens_file: an asphere line is `asphere k kappa [A4 [A6 .. A14]]` (once per interface)");
    has_asph[k] = true;
    akappa[k] = (float)c[1];
    for (size_t m = 2; m < c.size(); m++) acoef[(m - 2) * (size_t)n + k] = (float)c[m];
  }
  int bon[LF_MAX_SURFACES] = {};
  float brx[LF_MAX_SURFACES] = {}, bkx[LF_MAX_SURFACES] = {}, bky[LF_MAX_SURFACES] = {};
  for (const auto& c : bics) {
    const int k = c.size() >= 2 ? (int)c[0] : -1;
    if (k < 0 || k >= n || (double)k != c[0] || (int)c.size() > 4 || bon[k])
      return lf_fail(ctx, LF_ERR_INVALID, "lf_load_lens_file: a biconic line is `biconic k Rx [kx [ky]]` (once per interface)");
    bon[k] = 1;
    brx[k] = (float)c[1];
    if (c.size() > 2) bkx[k] = (float)c[2];
    if (c.size() > 3) bky[k] = (float)c[3];
  }
  int pon[LF_MAX_SURFACES] = {};
  float pt[3 * LF_MAX_SURFACES] = {}, pa[3 * LF_MAX_SURFACES] = {};
  for (const auto& c : poses) {
    const int k = c.size() >= 1 ? (int)c[0] : -1;
    if (k < 0 || k >= n || (double)k != c[0] || (int)c.size() != 7 || pon[k])
      return lf_fail(ctx, LF_ERR_INVALID, "lf_load_lens_file: a pose line is `pose k dx dy dz ax ay az` (once per interface)");
    pon[k] = 1;
    for (int m = 0; m < 3; m++) { pt[3 * k + m] = (float)c[1 + m]; pa[3 * k + m] = (float)c[4 + m]; }
  }
  lf_status st = lf_set_lens(ctx, n, stop, nl, radius, thick, ior, semi, (float)sensor_w);
  if (st == LF_OK && !poses.empty()) {
    st = lf_set_lens_poses(ctx, n, pon, pt, pa);
    if (st != LF_OK) {   // the lens stays, centred
      const std::string why = ctx->err;
      return lf_fail(ctx, st, "lf_load_lens_file: " + why);
    }
  }
  if (st == LF_OK && !sens.empty()) st = lf_set_sensor_reflectance(ctx, nl, srefl);   // (the mode stays what it is)
  if (st == LF_OK && !bics.empty()) {   // (before the aspheres: an interface with both lines is refused by their setter)
    st = lf_set_lens_biconics(ctx, n, bon, brx, bkx, bky);
    if (st != LF_OK) {   // the lens stays, one of spheres
      const std::string why = ctx->err;
      (void)lf_set_lens_poses(ctx, 0, nullptr, nullptr, nullptr);
      return lf_fail(ctx, st, "lf_load_lens_file: " + why);
    }
  }
  if (st == LF_OK && !asphs.empty()) {
    st = lf_set_lens_aspheres(ctx, n, akappa, LF_MAX_ASPH_COEF, acoef);
    if (st != LF_OK) {   // the lens stays, one of spheres
      const std::string why = ctx->err;
      (void)lf_set_lens_biconics(ctx, 0, nullptr, nullptr, nullptr, nullptr);
      (void)lf_set_lens_poses(ctx, 0, nullptr, nullptr, nullptr);
      return lf_fail(ctx, st, "lf_load_lens_file: " + why);
    }
  }
  if (st != LF_OK || (coats.empty() && layers.empty())) return st;
  st = layers.empty() ? lf_set_lens_coatings(ctx, n, nl, lam, cth, cidx)
                      : lf_set_lens_coating_stacks(ctx, n, nl, lam, nlay.data(), lth.data(), lidx.data());
  if (st != LF_OK) {   // the lens stays, bare
    const std::string why = ctx->err;
    (void)lf_set_lens_coatings(ctx, n, nl, nullptr, nullptr, nullptr);
    return lf_fail(ctx, st, "lf_load_lens_file: " + why);
  }
  return LF_OK;
}

lf_status lf_get_lens_info(lf_ctx* ctx, int* n_surfaces, int* stop_index, int* n_lambda, float* sensor_width_mm,
                           double* efl_mm) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_get_lens_info before lf_set_lens");
  if (n_surfaces) *n_surfaces = ctx->raw_n;
  if (stop_index) *stop_index = ctx->raw_stop;
  if (n_lambda) *n_lambda = ctx->lens.n_lambda;
  if (sensor_width_mm) *sensor_width_mm = ctx->sensor_w_mm;
  if (efl_mm) {
    *efl_mm = 0.0;   // (an afocal prescription has none)
    (void)lf_paraxial_efl(ctx->raw_n, ctx->raw_stop, ctx->raw_radius, ctx->raw_thickness,
                          ctx->raw_ior + (size_t)(ctx->lens.n_lambda / 2) * ctx->raw_n, efl_mm);
  }
  return LF_OK;
}

// ---------------------------------------------------------------- pupil target -------------------
lf_status lf_set_pupil_target(lf_ctx* ctx, float radius_mm, float z_mm) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_set_pupil_target before lf_set_lens");
  if (radius_mm > 0.0f) {
    if (!(z_mm < ctx->lens.z_sensor) || !std::isfinite(z_mm) || !std::isfinite(radius_mm))
      return lf_fail(ctx, LF_ERR_INVALID, "pupil target: the disc must lie in front of the sensor plane");
    ctx->pupil_target_h = radius_mm; ctx->pupil_target_z = z_mm;
  } else {
    ctx->pupil_target_h = 0.0f; ctx->pupil_target_z = 0.0f;
  }
  lf_apply_pupil_target(ctx);
  return LF_OK;
}

lf_status lf_get_pupil_target(lf_ctx* ctx, float* radius_mm, float* z_mm, float* z_sensor_mm) {
  if (!ctx) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_get_pupil_target before lf_set_lens");
  if (radius_mm) *radius_mm = ctx->lens.pupil_h;
  if (z_mm) *z_mm = ctx->lens.pupil_z;
  if (z_sensor_mm) *z_sensor_mm = ctx->lens.z_sensor;
  return LF_OK;
}

lf_status lf_paraxial_exit_pupil(int n, int stop, const float* radius, const float* thickness, const float* ior_row,
                                 double* z_mm, double* magnification) {
  if (n < 1 || n > LF_MAX_SURFACES || stop < 0 || stop >= n || !radius || !thickness || !ior_row || !z_mm || !magnification)
    return LF_ERR_INVALID;
  // the stop's centre imaged by the interfaces behind it: ray (height y, angle u) from the stop plane,
  // T(d) = [[1, d], [0, 1]], R(c, n1, n2) = [[1, 0], [c (n1 - n2) / n2, n1 / n2]] (pathtracer.cpp:527-533)
  double A = 1, B = 0, Cc = 0, D = 1;   // system matrix stop plane -> rear vertex
  double n1 = 1.0, z = 0.0, z_stop = 0.0;
  for (int k = 0; k < n; k++) {
    if (k == stop) z_stop = z;
    if (k < stop) n1 = ior_row[k];      // the medium the stop sits in
    z += thickness[k];
  }
  double z_rear = z - thickness[n - 1];
  double nm = n1;
  for (int k = stop; k < n; k++) {
    if (k > stop) {
      const double c = radius[k] == 0.0f ? 0.0 : 1.0 / (double)radius[k], n2 = ior_row[k];
      if (!(n2 >= 1.0)) return LF_ERR_INVALID;
      const double r10 = c * (nm - n2) / n2, r11 = nm / n2;
      const double c2 = r10 * A + r11 * Cc, d2 = r10 * B + r11 * D;
      Cc = c2; D = d2;
      nm = n2;
    }
    if (k + 1 < n) {
      const double d = thickness[k];
      A += d * Cc; B += d * D;
    }
  }
  (void)z_stop;
  if (D == 0.0) return LF_ERR_INVALID;   // the stop is imaged at infinity (image-space telecentric)
  const double l = -B / D;               // image distance behind the rear vertex (+z = towards the sensor)
  *z_mm = z_rear + l;
  *magnification = A + l * Cc;
  return LF_OK;
}

lf_status lf_aim_at_exit_pupil(lf_ctx* ctx, float margin) {
  if (!ctx || !(margin > 0.0f)) return LF_ERR_INVALID;
  if (!ctx->lens_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_aim_at_exit_pupil before lf_set_lens");
  if (ctx->raw_stop < 0) return lf_fail(ctx, LF_ERR_INVALID, "lf_aim_at_exit_pupil: the prescription has no stop");
  if (!ctx->ap[LF_APERTURE_STARBURST].valid)
    return lf_fail(ctx, LF_ERR_STATE, "aperture mask (LF_APERTURE_STARBURST slot) not set");
  double z = 0, m = 0;
  lf_status st = lf_paraxial_exit_pupil(ctx->raw_n, ctx->raw_stop, ctx->raw_radius, ctx->raw_thickness,
                                        ctx->raw_ior + (size_t)(ctx->lens.n_lambda / 2) * ctx->raw_n, &z, &m);
  if (st != LF_OK) return lf_fail(ctx, LF_ERR_INVALID, "lf_aim_at_exit_pupil: the stop has no finite paraxial image");
  // the part of the stop that is open: the circle around the mask's non-zero texels, never more than
  // the housing
  const double open = std::min(1.0, ctx->ap[LF_APERTURE_STARBURST].open_radius);
  const double r = (double)ctx->lens.stop_h * open * std::fabs(m) * (double)margin;
  return lf_set_pupil_target(ctx, (float)r, (float)z);
}

lf_status lf_set_ghost_accumulate(lf_ctx* ctx, int on) {
  if (!ctx) return LF_ERR_INVALID;
  ctx->ghost_accumulate = on != 0;
  return LF_OK;
}

// one float in, one float out, as a device instruction computes it (lf_native_sqrt, lf_native_rcp)
static lf_status native_unary(lf_ctx* ctx, const float* x, float* y, size_t n,
                              lf_status (*launch)(lf_ctx*, const float*, float*, size_t)) {
  if (!ctx || (n && (!x || !y))) return LF_ERR_INVALID;
  if (n == 0) return LF_OK;
  LF_HIP(ctx, hipSetDevice(ctx->device));
  float *d_x = nullptr, *d_y = nullptr;
  hipError_t e = hipMalloc((void**)&d_x, n * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&d_y, n * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(d_x, x, n * sizeof(float), hipMemcpyHostToDevice);
  lf_status st = LF_OK;
  if (e == hipSuccess) st = launch(ctx, d_x, d_y, n);
  if (e == hipSuccess && st == LF_OK) e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess && st == LF_OK) e = hipMemcpy(y, d_y, n * sizeof(float), hipMemcpyDeviceToHost);
  if (d_x) (void)hipFree(d_x);
  if (d_y) (void)hipFree(d_y);
  if (st != LF_OK) return st;
  LF_HIP(ctx, e);
  return LF_OK;
}

lf_status lf_native_sqrt(lf_ctx* ctx, const float* x, float* y, size_t n) {
  return native_unary(ctx, x, y, n, lfk_native_sqrt);
}

lf_status lf_native_rcp(lf_ctx* ctx, const float* x, float* y, size_t n) {
  return native_unary(ctx, x, y, n, lfk_native_rcp);
}

lf_status lf_get_counters(lf_ctx* ctx, lf_counters* out) {
  if (!ctx || !out) return LF_ERR_INVALID;
  unsigned long long c[8];
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LF_HIP(ctx, hipMemcpy(c, ctx->counters_dev, sizeof(c), hipMemcpyDeviceToHost));
  out->rays_launched = c[0]; out->surface_events = c[1]; out->rays_clipped_stop = c[2];
  out->rays_vignetted = c[3]; out->rays_tir = c[4]; out->rays_reached_scene = c[5];
  out->rays_hit_light = c[6];
  return LF_OK;
}

lf_status lf_get_executed_events(lf_ctx* ctx, uint64_t* out) {
  if (!ctx || !out) return LF_ERR_INVALID;
  unsigned long long c = 0;
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LF_HIP(ctx, hipMemcpy(&c, ctx->counters_dev + 7, sizeof(c), hipMemcpyDeviceToHost));
  *out = c;
  return LF_OK;
}

lf_status lf_get_march_stats(lf_ctx* ctx, uint64_t out[4]) {
  if (!ctx || !out) return LF_ERR_INVALID;
  unsigned long long c[kMarchCounterSlots];
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LF_HIP(ctx, hipMemcpy(c, ctx->counters_dev, sizeof(c), hipMemcpyDeviceToHost));
  out[0] = c[7]; out[1] = c[8]; out[2] = c[9]; out[3] = 0;
#ifdef LF_EXPERIMENTS
  if (std::getenv("LF_MARCH_PRINT_HIST")) {   // instrumented builds only (LF_MARCH_LIVE_HIST / _PAIR_STATS): the slots stay 0 otherwise
    static const char* kinds[3] = {"refraction", "mirror_or_flat", "stop"};
    for (int k = 0; k < 3; k++) {
      std::fprintf(stderr, "LIVE_HIST %s", kinds[k]);
      for (int b = 0; b < 9; b++) std::fprintf(stderr, " %llu", c[kMarchHistSlot + 9 * k + b]);
      std::fprintf(stderr, "\n");
    }
    for (int q = 0; q < ctx->pairs.n && q < 64; q++)
      if (c[kMarchPairSlot + q] | c[kMarchPairSlot + 64 + q])
        std::fprintf(stderr, "PAIR_STAT %d %d %d %llu %llu %llu\n", q, ctx->pairs.ij[q][0], ctx->pairs.ij[q][1],
                     c[kMarchPairSlot + q], c[kMarchPairSlot + 64 + q], c[kMarchPairSlot + 128 + q]);
  }
#endif
  return LF_OK;
}

lf_status lf_reset_counters(lf_ctx* ctx) {
  if (!ctx) return LF_ERR_INVALID;
  LF_HIP(ctx, hipMemsetAsync(ctx->counters_dev, 0, kMarchCounterSlots * sizeof(unsigned long long), ctx->stream));
  if (ctx->sensor.stats_dev)
    LF_HIP(ctx, hipMemsetAsync(ctx->sensor.stats_dev, 0, kSensorStats * sizeof(unsigned long long), ctx->stream));
  ctx->cull_audit_rays = 0; ctx->cull_audit_lit = 0; ctx->cull_audit_tripped = 0;
  return LF_OK;
}

// ---------------------------------------------------------------- measurement ----------------
lf_status lf_timing_enable(lf_ctx* ctx, int on) {
  if (!ctx) return LF_ERR_INVALID;
  ctx->timing = on != 0;
  return LF_OK;
}

lf_status lf_timing_reset(lf_ctx* ctx) {
  if (!ctx) return LF_ERR_INVALID;
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (auto& t : ctx->timed) { ctx->event_pool.push_back(t.start); ctx->event_pool.push_back(t.stop); }
  ctx->timed.clear();
  for (int k = 0; k < LFK_COUNT; k++) { ctx->timed_ms[k] = 0.0; ctx->timed_n[k] = 0; }
  return LF_OK;
}

lf_status lf_timing_get(lf_ctx* ctx, const char* kernel, int* launches, double* total_ms) {
  if (!ctx || !kernel || !launches || !total_ms) return LF_ERR_INVALID;
  int id = -1;
  for (int k = 0; k < LFK_COUNT; k++) if (std::strcmp(kernel, kKernelNames[k]) == 0) id = k;
  if (id < 0) return lf_fail(ctx, LF_ERR_INVALID, "unknown kernel name");
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->comm_stream) LF_HIP(ctx, hipStreamSynchronize(ctx->comm_stream));   // "exchange" runs there
  timing_fold(ctx, true);
  *launches = ctx->timed_n[id];
  *total_ms = ctx->timed_ms[id];
  return LF_OK;
}

}  // extern "C"
