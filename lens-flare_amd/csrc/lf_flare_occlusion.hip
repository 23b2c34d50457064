// lf_flare_occlusion.hip -- FLARE OCCLUSION (lf_set_flare_occlusion; DESIGN.md section 4, "flare occlusion"): how much of
// each flare of the flare state the scene leaves visible, and the flare layer / the paraxial quads scaled by it.
//
//   k_flare_visibility        one lane per (flare, shadow ray): the ray from the resident sample table and the device flare
//                             state (lf_flare_ray, the __host__ __device__ definition lf_flare_shadow_rays exports), through the
//                             ghost march's own mapping and any-hit walk (lf_march_common.h ghost_ray_visible, unchanged);
//                             one ballot and one integer atomic per wave into count[flare]
//   k_flare_visibility_apply  one workgroup behind it on the same stream: visibility[k] = count[k] / R, the EFFECTIVE flare
//                             record (radiance[k][c] * visibility[k]) and the quad list with its colours times the
//                             visibility of the flare that supplied axis_ray
//
// The flare kernels and the rasteriser are the same code objects: they are handed the effective records instead of the
// installed ones.  Nothing here draws a random number; a visibility of 1 changes no bit of any buffer (x * 1.0 is exact).
#include <cmath>
#include <cstring>
#include <vector>

#include "lf_internal.h"
#include "lf_march_common.h"

// ---- the definitions, host and device from one text (-ffp-contract=off on both sides: + - * / sqrt only) -------------------
struct LfFlareRayArgs {
  int R, origin;
  double edge_x, edge_y;   // tan(0.5 fov pi / 180): k_frame_setup's expression, on the host
  double tan_alpha;        // tan((double)angular_radius), on the host
  float h0;                // the front interface's semi-aperture (LF_FLARE_ORIGIN_FRONT_ELEMENT)
  int pad;
};

// shadow ray r of the flare stored at screen position (nx, ny): sample = {a, b, c, d} of lf_flare_shadow_samples
__host__ __device__ inline void lf_flare_ray(double nx, double ny, const LfFlareRayArgs& A, const float* __restrict__ sample,
                                             float ray[6]) {
  const double vx = (2.0 * nx - 1.0) * A.edge_x, vy = (2.0 * ny - 1.0) * A.edge_y, vz = -1.0;
  const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
  const double sx = vx / vn, sy = vy / vn, sz = vz / vn;
  // e1 = unit(s.z, 0, -s.x), e2 = s x e1
  const double ux = sz, uy = 0.0, uz = -sx;
  const double un = sqrt((ux * ux + uy * uy) + uz * uz);
  const double e1x = ux / un, e1y = uy / un, e1z = uz / un;
  const double e2x = sy * e1z - sz * e1y, e2y = sz * e1x - sx * e1z, e2z = sx * e1y - sy * e1x;
  const double c = (double)sample[2], d = (double)sample[3];
  ray[3] = (float)(sx + A.tan_alpha * (c * e1x + d * e2x));
  ray[4] = (float)(sy + A.tan_alpha * (c * e1y + d * e2y));
  ray[5] = (float)(sz + A.tan_alpha * (c * e1z + d * e2z));
  if (A.origin == LF_FLARE_ORIGIN_FRONT_ELEMENT) {
    ray[0] = (float)((double)A.h0 * (double)sample[0]);
    ray[1] = (float)((double)A.h0 * (double)sample[1]);
  } else {
    ray[0] = 0.0f; ray[1] = 0.0f;
  }
  ray[2] = 0.0f;
}

static double van_der_corput(unsigned r, unsigned base) {
  double v = 0.0, f = 1.0 / (double)base;
  while (r) {
    v += f * (double)(r % base);
    r /= base;
    f /= (double)base;
  }
  return v;
}

static bool flare_rays_ok(int R) { return R >= 64 && R <= 4096 && (R & 63) == 0; }

static void flare_samples(int R, float* out) {
  const double two_pi = 2.0 * 3.14159265358979323846;
  for (int r = 0; r < R; r++) {
    const double u0 = ((double)r + 0.5) / (double)R, u1 = van_der_corput((unsigned)r, 2u), u2 = van_der_corput((unsigned)r, 3u),
                 u3 = van_der_corput((unsigned)r, 5u);
    const double ra = std::sqrt(u0), rl = std::sqrt(u2);
    out[4 * r + 0] = (float)(ra * std::cos(two_pi * u1));
    out[4 * r + 1] = (float)(ra * std::sin(two_pi * u1));
    out[4 * r + 2] = (float)(rl * std::cos(two_pi * u3));
    out[4 * r + 3] = (float)(rl * std::sin(two_pi * u3));
  }
}

static LfFlareRayArgs flare_ray_args(int R, double hfov_deg, double vfov_deg, float angular_radius, int origin, float h0) {
  const double PI_ = 3.14159265358979323;   // (k_frame_setup's literal)
  LfFlareRayArgs A;
  std::memset(&A, 0, sizeof(A));
  A.R = R; A.origin = origin;
  A.edge_x = std::tan(0.5 * (hfov_deg * (PI_ / 180.0)));
  A.edge_y = std::tan(0.5 * (vfov_deg * (PI_ / 180.0)));
  A.tan_alpha = std::tan((double)angular_radius);
  A.h0 = h0;
  return A;
}

namespace {

using lfm::ghost_ray_visible;

// One lane per (flare, ray); total = n_flares * R is a multiple of 64, so a wave is inside or outside as a whole and its 64
// rays belong to one flare.
__global__ __launch_bounds__(256) void k_flare_visibility(LfOcclDev o, const LfFlares* __restrict__ fl,
                                                          const float* __restrict__ samples, LfFlareRayArgs A, int total,
                                                          unsigned long long* __restrict__ count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int k = i / A.R, r = i - k * A.R;
  float ray[6];
  lf_flare_ray(fl->origin[k][0], fl->origin[k][1], A, samples + 4 * (size_t)r, ray);
  const bool vis = ghost_ray_visible(o, ray[0], ray[1], ray[2], ray[3], ray[4], ray[5]);
  const unsigned long long seen = __ballot(vis);
  if ((threadIdx.x & 63) == 0) atomicAdd(&count[k], (unsigned long long)__popcll(seen));
}

__global__ __launch_bounds__(256) void k_flare_visibility_apply(const LfFlares* __restrict__ fl, int R,
                                                                LfFlareVisDev* __restrict__ vd, LfFlares* __restrict__ eff,
                                                                const LfGhostList* __restrict__ gl, LfGhostList* __restrict__ gl_eff) {
  __shared__ double s_vis[LF_MAX_FLARES];
  const int n = min(max(fl->n_flares, 0), LF_MAX_FLARES);
  const int t = threadIdx.x;
  if (t < LF_MAX_FLARES) {
    const double v = t < n ? (double)vd->count[t] / (double)R : 0.0;
    vd->visibility[t] = v;
    s_vis[t] = v;
  }
  __syncthreads();
  if (t == 0) {
    LfFlares f = *fl;
    for (int k = 0; k < n; k++)
      for (int c = 0; c < 3; c++) f.radiance[k][c] = f.radiance[k][c] * s_vis[k];
    *eff = f;
  }
  // the quads are those of the flare that supplied axis_ray: the last one find_sun_pos kept
  const double q = n > 0 ? s_vis[n - 1] : 1.0;
  const int n_tris = min(max(gl->n_tris, 0), kMaxGhostTris);
  if (t == 0) { gl_eff->n_tris = n_tris; gl_eff->pad = 0; }
  for (int j = t; j < n_tris; j += blockDim.x) {
    LfGhostTri tr = gl->tri[j];
    tr.colour[0] = tr.colour[0] * q; tr.colour[1] = tr.colour[1] * q; tr.colour[2] = tr.colour[2] * q;
    gl_eff->tri[j] = tr;
  }
}

// what a consuming call needs installed while the setting is on
lf_status flare_occlusion_ready(const lf_ctx* ctx, const char* who) {
  std::string missing;
  if (ctx->flare_occl_origin == LF_FLARE_ORIGIN_FRONT_ELEMENT && !ctx->lens_valid) missing += " a lens (lf_set_lens)";
  if (!ctx->cam_valid) missing += std::string(missing.empty() ? "" : ",") + " a camera (lf_set_camera)";
  if (!ctx->scene_valid || ctx->scene_dev.n_prims < 1)
    missing += std::string(missing.empty() ? "" : ",") + " a scene of at least one primitive (lf_set_scene / lf_load_collada)";
  if (missing.empty()) return LF_OK;
  return lf_fail(ctx, LF_ERR_STATE, std::string(who) + ": flare occlusion needs" + missing);
}

}  // namespace

// The consuming calls' one entry: the setting off -> the installed records, nothing launched.  On -> the state is checked,
// the two kernels run on the context's stream from the state installed now, and the effective records are handed back;
// with no flare in the frame nothing is launched and the installed records (which hold no flare) are.
lf_status lf_flare_occlusion_update(lf_ctx* ctx, const char* who, const LfFlares** fl, const LfGhostList** gl) {
  if (fl) *fl = ctx->flares;
  if (gl) *gl = ctx->ghosts;
  if (!ctx->flare_occl) return LF_OK;
  lf_status st = flare_occlusion_ready(ctx, who);
  if (st != LF_OK) return st;
  if (ctx->flares_n_host < 0) {   // lf_find_sun_pos counted on the device: fetched once per flare state
    int n = 0;
    LF_HIP(ctx, hipMemcpyAsync(&n, &ctx->flares->n_flares, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->flares_n_host = std::min(std::max(n, 0), LF_MAX_FLARES);
  }
  const int n = ctx->flares_n_host;
  if (n == 0) return LF_OK;
  LfOcclDev o;
  float h0 = 0.0f;
  if (ctx->flare_occl_origin == LF_FLARE_ORIGIN_FRONT_ELEMENT) {
    st = lf_fill_occlusion(ctx, ctx->flare_occl_wpm, &o);
    if (st != LF_OK) return st;
    h0 = ctx->raw_semi_ap[0];
  } else {
    // the camera position itself: oc = 0 whatever the scale, no z_ref, no lens
    std::memset(&o, 0, sizeof(o));
    o.nodes = ctx->scene_dev.nodes; o.prims = ctx->scene_dev.prims;
    std::memcpy(o.c2w, ctx->cam.c2w, sizeof(o.c2w));
    std::memcpy(o.pos, ctx->cam.pos, sizeof(o.pos));
    o.wpm = 1.0;
  }
  o.stats = nullptr;   // (the march's tallies are not this feature's)
  const LfFlareRayArgs A = flare_ray_args(ctx->flare_occl_rays, ctx->cam.hfov_deg, ctx->cam.vfov_deg, ctx->flare_occl_alpha,
                                          ctx->flare_occl_origin, h0);
  const int total = n * A.R;
  LF_HIP(ctx, hipMemsetAsync(ctx->flare_vis_dev->count, 0, sizeof(ctx->flare_vis_dev->count), ctx->stream));
  hipEvent_t ev = lf_timing_begin(ctx, LFK_FLARE_VIS);
  hipLaunchKernelGGL(k_flare_visibility, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, o, ctx->flares,
                     ctx->flare_samples_dev, A, total, ctx->flare_vis_dev->count);
  hipLaunchKernelGGL(k_flare_visibility_apply, dim3(1), dim3(256), 0, ctx->stream, ctx->flares, A.R, ctx->flare_vis_dev,
                     ctx->flares_eff, ctx->ghosts, ctx->ghosts_eff);
  lf_timing_end(ctx, LFK_FLARE_VIS, ev);
  LF_HIP(ctx, hipGetLastError());
  if (fl) *fl = ctx->flares_eff;
  if (gl) *gl = ctx->ghosts_eff;
  return LF_OK;
}

void lf_flare_occlusion_free(lf_ctx* ctx) {
  void* ptrs[] = {ctx->flare_samples_dev, ctx->flare_vis_dev, ctx->flares_eff, ctx->ghosts_eff};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  ctx->flare_samples_dev = nullptr; ctx->flare_vis_dev = nullptr; ctx->flares_eff = nullptr; ctx->ghosts_eff = nullptr;
  ctx->flare_samples_n = 0;
}

extern "C" {

lf_status lf_set_flare_occlusion(lf_ctx* ctx, int on, int rays_per_light, float angular_radius, int origin, double world_per_mm) {
  if (!ctx) return LF_ERR_INVALID;
  if (on == 0) { ctx->flare_occl = false; return LF_OK; }   // (off: the other arguments are not looked at; the setting keeps them)
  if (!flare_rays_ok(rays_per_light))
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_flare_occlusion: rays_per_light must be a multiple of 64 in [64, 4096]");
  if (!std::isfinite(angular_radius) || !(angular_radius >= 0.0f) || !(angular_radius <= 0.5f))
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_flare_occlusion: angular_radius must be finite and in [0, 0.5]");
  if (origin != LF_FLARE_ORIGIN_CAMERA && origin != LF_FLARE_ORIGIN_FRONT_ELEMENT)
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_flare_occlusion: origin must be LF_FLARE_ORIGIN_CAMERA (0) or LF_FLARE_ORIGIN_FRONT_ELEMENT (1)");
  if (origin == LF_FLARE_ORIGIN_FRONT_ELEMENT && (!(world_per_mm > 0.0) || !std::isfinite(world_per_mm)))
    return lf_fail(ctx, LF_ERR_INVALID, "lf_set_flare_occlusion: world_per_mm must be > 0 and finite under LF_FLARE_ORIGIN_FRONT_ELEMENT");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->flare_vis_dev) {
    LF_HIP(ctx, hipMalloc((void**)&ctx->flare_vis_dev, sizeof(LfFlareVisDev)));
    LF_HIP(ctx, hipMemset(ctx->flare_vis_dev, 0, sizeof(LfFlareVisDev)));
  }
  if (!ctx->flares_eff) {
    LF_HIP(ctx, hipMalloc((void**)&ctx->flares_eff, sizeof(LfFlares)));
    LF_HIP(ctx, hipMemset(ctx->flares_eff, 0, sizeof(LfFlares)));
  }
  if (!ctx->ghosts_eff) {
    LF_HIP(ctx, hipMalloc((void**)&ctx->ghosts_eff, sizeof(LfGhostList)));
    LF_HIP(ctx, hipMemset(ctx->ghosts_eff, 0, sizeof(LfGhostList)));
  }
  if (ctx->flare_samples_n != rays_per_light) {   // the table: built once per setting, resident
    std::vector<float> table(4 * (size_t)rays_per_light);
    flare_samples(rays_per_light, table.data());
    LF_HIP(ctx, hipStreamSynchronize(ctx->stream));   // a visibility kernel in flight may read the old table
    if (ctx->flare_samples_dev) (void)hipFree(ctx->flare_samples_dev);
    ctx->flare_samples_dev = nullptr; ctx->flare_samples_n = 0;
    LF_HIP(ctx, hipMalloc((void**)&ctx->flare_samples_dev, table.size() * sizeof(float)));
    LF_HIP(ctx, hipMemcpy(ctx->flare_samples_dev, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    ctx->flare_samples_n = rays_per_light;
  }
  ctx->flare_occl = true;
  ctx->flare_occl_rays = rays_per_light;
  ctx->flare_occl_alpha = angular_radius;
  ctx->flare_occl_origin = origin;
  if (origin == LF_FLARE_ORIGIN_FRONT_ELEMENT) ctx->flare_occl_wpm = world_per_mm;
  return LF_OK;
}

lf_status lf_get_flare_occlusion(lf_ctx* ctx, int* on, int* rays_per_light, float* angular_radius, int* origin, double* world_per_mm) {
  if (!ctx) return LF_ERR_INVALID;
  if (on) *on = ctx->flare_occl ? 1 : 0;
  if (rays_per_light) *rays_per_light = ctx->flare_occl_rays;
  if (angular_radius) *angular_radius = ctx->flare_occl_alpha;
  if (origin) *origin = ctx->flare_occl_origin;
  if (world_per_mm) *world_per_mm = ctx->flare_occl_wpm;
  return LF_OK;
}

lf_status lf_get_flare_visibility(lf_ctx* ctx, int* n_flares, double* visibility, uint64_t* visible_rays) {
  if (!ctx || !n_flares) return LF_ERR_INVALID;
  if (!ctx->flare_occl)
    return lf_fail(ctx, LF_ERR_STATE, "lf_get_flare_visibility: flare occlusion is off (lf_set_flare_occlusion)");
  if (!ctx->flares_valid) return lf_fail(ctx, LF_ERR_STATE, "lf_get_flare_visibility: no flare state: call lf_find_sun_pos or lf_set_flares");
  LF_HIP(ctx, hipSetDevice(ctx->device));
  lf_status st = lf_flare_occlusion_update(ctx, "lf_get_flare_visibility", nullptr, nullptr);
  if (st != LF_OK) return st;
  const int n = ctx->flares_n_host;
  *n_flares = n;
  if (n == 0) return LF_OK;
  LfFlareVisDev v;
  LF_HIP(ctx, hipMemcpyAsync(&v, ctx->flare_vis_dev, sizeof(v), hipMemcpyDeviceToHost, ctx->stream));
  LF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < n; k++) {
    if (visibility) visibility[k] = v.visibility[k];
    if (visible_rays) visible_rays[k] = v.count[k];
  }
  return LF_OK;
}

lf_status lf_flare_shadow_samples(int rays_per_light, float* out) {
  if (!out || !flare_rays_ok(rays_per_light)) return LF_ERR_INVALID;
  flare_samples(rays_per_light, out);
  return LF_OK;
}

lf_status lf_flare_shadow_rays(int rays_per_light, const double flare_origin[2], double hfov_deg, double vfov_deg, float angular_radius,
                               int origin, float front_semi_aperture, float* rays) {
  if (!flare_origin || !rays || !flare_rays_ok(rays_per_light)) return LF_ERR_INVALID;
  if (!std::isfinite(angular_radius) || !(angular_radius >= 0.0f) || !(angular_radius <= 0.5f)) return LF_ERR_INVALID;
  if (origin != LF_FLARE_ORIGIN_CAMERA && origin != LF_FLARE_ORIGIN_FRONT_ELEMENT) return LF_ERR_INVALID;
  if (!std::isfinite(flare_origin[0]) || !std::isfinite(flare_origin[1]) || !std::isfinite(hfov_deg) || !std::isfinite(vfov_deg) ||
      !(hfov_deg > 0.0) || !(hfov_deg < 180.0) || !(vfov_deg > 0.0) || !(vfov_deg < 180.0))
    return LF_ERR_INVALID;
  if (origin == LF_FLARE_ORIGIN_FRONT_ELEMENT && (!std::isfinite(front_semi_aperture) || !(front_semi_aperture > 0.0f))) return LF_ERR_INVALID;
  std::vector<float> table(4 * (size_t)rays_per_light);
  flare_samples(rays_per_light, table.data());
  const LfFlareRayArgs A = flare_ray_args(rays_per_light, hfov_deg, vfov_deg, angular_radius, origin, front_semi_aperture);
  for (int r = 0; r < rays_per_light; r++) lf_flare_ray(flare_origin[0], flare_origin[1], A, table.data() + 4 * (size_t)r, rays + 6 * (size_t)r);
  return LF_OK;
}

}  // extern "C"
