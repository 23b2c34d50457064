/* lensflare.h -- C ABI of liblensflare_hip.so, the MI355X (gfx950) implementation of the
 * lens-flare hot path of aatifjiwani/lens-flare (src/pathtracer).
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ types, no exceptions, every
 * entry point returns an lf_status.  Each function names the reference interface it replaces
 * (file:line relative to the reference checkout).  The reference itself has no C ABI -- its
 * boundary is the public surface of `class PathTracer` inside libpt31.so
 * (CMakeLists.txt:20-33,139-142; src/pathtracer/pathtracer.h:25-143) -- so the C++ shim in
 * lens-flare_amd/host/ maps that surface 1:1 onto these calls.
 *
 * Threading contract (mirrors src/pathtracer/raytraced_renderer.cpp:300-311, :637-646): the
 * set-up and render calls are made from one thread per context; lf_read_* may then be called
 * concurrently from any number of threads.  One context drives one GPU; multi-GPU = one context
 * (and normally one process) per GPU, each rendering its own band of sensor rows.
 */
#ifndef LENSFLARE_H
#define LENSFLARE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LF_ABI_VERSION 1
#define LF_MAX_SURFACES 16   /* interfaces per prescription (incl. the stop) */
#define LF_MAX_LAMBDA 8      /* wavelengths per prescription */
#define LF_MAX_COAT_LAYERS 6 /* layers of a coating stack on one interface (lf_set_lens_coating_stacks) */
#define LF_MAX_ASPH_COEF 6   /* even coefficients A4 .. A14 of an aspheric interface (lf_set_lens_aspheres) */
#define LF_MAX_FLARES 8      /* in-frame directional lights */
#define LF_MAX_LIGHTS 8      /* lights one launch of the geometric march follows (lf_set_lights) */
#define LF_MAX_PAIRS 128     /* ghost pairs per trace call */

typedef struct lf_ctx lf_ctx;

typedef enum {
  LF_OK = 0,
  LF_ERR_INVALID = 1,   /* bad argument (null pointer, size out of range, ...) */
  LF_ERR_NO_DEVICE = 2, /* no gfx950 device / device index out of range */
  LF_ERR_HIP = 3,       /* a HIP runtime call failed; see lf_last_error */
  LF_ERR_STATE = 4,     /* call order violated (e.g. render before set_frame) */
  LF_ERR_OOM = 5,
  LF_ERR_UNSUPPORTED = 6 /* the call is valid but not built for the installed state (e.g. the lens camera on an aspheric lens) */
} lf_status;

typedef enum { LF_APERTURE_STARBURST = 0, LF_APERTURE_GHOST = 1 } lf_aperture_slot;

/* CameraApertureTexture (src/pathtracer/camera.h:18-88) */
typedef struct {
  int width, height;
  int min_x, min_y, max_x, max_y; /* bbox of texels > 0 (camera.h:54-72) */
  double total_value;             /* camera.h:61 */
} lf_aperture_stats;

/* device-side counters of the geometric march */
typedef struct {
  uint64_t rays_launched;   /* (sample, wavelength, pair) rays started */
  uint64_t surface_events;  /* ray-surface events (intersect + refract|reflect) of all paths, each path
                               counted on its own -- the legs that paths of one sample share are
                               computed once on the device, see lf_get_executed_events */
  uint64_t rays_clipped_stop;   /* killed by the aperture mask at the stop */
  uint64_t rays_vignetted;      /* outside a semi-aperture or missed a surface */
  uint64_t rays_tir;            /* total internal reflection */
  uint64_t rays_reached_scene;  /* left the front element */
  uint64_t rays_hit_light;      /* ... inside the light's angular lobe (non-zero radiance) */
} lf_counters;

/* ---------------------------------------------------------------- life cycle ------------- */
/* replaces: PathTracer::PathTracer / ~PathTracer (pathtracer.cpp:14-30).  device = HIP ordinal. */
lf_status lf_create(lf_ctx** out, int device);
lf_status lf_destroy(lf_ctx* ctx);
/* text of the last error on this context (never NULL); valid until the next call */
const char* lf_last_error(const lf_ctx* ctx);
int lf_abi_version(void);
/* optional: run every launch on a caller-owned hipStream_t (e.g. torch's current stream) */
lf_status lf_set_stream(lf_ctx* ctx, void* hip_stream);
lf_status lf_synchronize(lf_ctx* ctx);

/* ---------------------------------------------------------------- frame ------------------ */
/* replaces: PathTracer::set_frame_size (pathtracer.cpp:66-69) + clear (:71-79).  Deals the whole frame to this context
 * again (undoes lf_set_row_interleave / lf_set_block_deal); a cull table share set before (lf_comm_share_cull /
 * lf_set_cull_share) stays. */
lf_status lf_set_frame(lf_ctx* ctx, int width, int height);
/* multi-GPU sharding: this context renders sensor rows [y0, y1) only (default: all rows).
 * Mirrors the tile queue of raytraced_renderer.cpp:314-328, one band of tile rows per GPU. */
lf_status lf_set_band(lf_ctx* ctx, int y0, int y1);
/* finer multi-GPU sharding for the geometric march: of the band's 8-row sensor tile rows t = y/8
 * this context marches only those with t % period == phase (default period 1 = all).  Dealing
 * tile rows round-robin to the GPUs balances the vignetting-dependent ray survival. */
lf_status lf_set_row_interleave(lf_ctx* ctx, int phase, int period);
/* ... or by BLOCKS of 64 x 64 pixels (round 6): block b (row-major over the frame) belongs to rank b % nranks; a frame
 * narrower than a multiple of 64 has partial blocks at its right and lower edges.  The block is the path cull's: a rank
 * that owns whole blocks builds, audits and reads only its own rows of the cull table -- pre-pass, audit and march all
 * shrink with the number of ranks and the table never crosses a link (where lf_set_row_interleave needs
 * lf_comm_share_cull / lf_set_cull_share and a second collective per frame).  lf_comm_gather / lf_group_gather
 * exchange blocks then.  Pixels, counters summed over the ranks and the gathered frame are the single-GPU frame's.
 * lf_set_row_interleave (or lf_set_frame) switches back.  A frame dealt by blocks shares no table: refused (LF_ERR_STATE)
 * while lf_comm_share_cull / lf_set_cull_share(rank, N > 1) is on, and they are refused while it is dealt; its
 * lf_get_cull_table has zero rows for the blocks of other ranks. */
lf_status lf_set_block_deal(lf_ctx* ctx, int rank, int nranks);
/* replaces the public fields PathTracer::ns_aa, flare_radius, flare_intensity
 * (pathtracer.h:93-94,107) */
lf_status lf_set_params(lf_ctx* ctx, int ns_aa, double flare_radius, double flare_intensity);

/* ---------------------------------------------------------------- inputs ----------------- */
/* replaces: CameraApertureTexture::init (camera.h:26-83) minus the PNG decode: texels are the
 * float values the reference derives from the red channel (CGL/src/color.cpp:16-21).  bbox and
 * total_value are computed on the device. */
lf_status lf_set_aperture(lf_ctx* ctx, lf_aperture_slot slot, const float* texels, int width,
                          int height);
lf_status lf_get_aperture_stats(lf_ctx* ctx, lf_aperture_slot slot, lf_aperture_stats* out);
/* How the geometric march and the lens camera read the stop mask (the LF_APERTURE_STARBURST slot; no reference
 * counterpart).  LF_MASK_NEAREST, the default: the texel the ray hits, alive iff it is > 0 -- every texel a hard
 * edge in every ghost.  LF_MASK_BILINEAR: the float32 contract below.  With the stop hit (hx, hy) and the stop's
 * semi-aperture stop_h,
 *   fu = fmaf(hx, 1 / stop_h, 1) * (0.5f * w),  fv likewise with h      (texel i has its centre at i + 0.5)
 *   gx = fu - 0.5f,  i0 = floor(gx),  fx = gx - i0                      (and gy, j0, fy)
 *   t00 t10 t01 t11 = max(texel, 0) at (i0, j0) (i0 + 1, j0) (i0, j0 + 1) (i0 + 1, j0 + 1), indices clamped to the texture
 *   a0 = fmaf(fx, t10 - t00, t00),  a1 = fmaf(fx, t11 - t01, t01),  value = fmaf(fy, a1 - a0, a0)
 *   the ray is ALIVE iff max(t00, t10, t01, t11) > 0 -- any of the four texels open, not value > 0: a ray with
 *   fx == 0 beside an open texel is alive with weight 0.
 * The lit set therefore grows by half a texel around the open region (it contains the nearest filter's); the cull
 * pre-pass, the audit and lf_aim_at_exit_pupil's open radius follow it.  A setting of the context: it survives
 * lf_set_aperture, lf_set_lens and lf_set_frame.  It does NOT affect the starburst DFT, the LF_APERTURE_GHOST slot
 * or lf_get_aperture_stats, which keep reading the texels as they are.  Of the CPU oracles (oracle/) the float64 tracer follows
 * filtered frames and coated ones (lfo.g64_set_mask_filter, lfo.g64_set_films: tests/test_gpu_lens_camera_variants.py
 * holds the lens camera to it); the float32 bit-exact oracle follows neither.  Only the weighted re-march of a lit path and the lens
 * camera's primary path pay for the four loads: the bench frame (c3) takes 44.6 ms under LF_MASK_BILINEAR against
 * 43.6 ms (x 1.023, profiles/mask_filter_cost.json); a context under LF_MASK_NEAREST runs the kernels it always ran.
 * Other values of filter: LF_ERR_INVALID. */
typedef enum { LF_MASK_NEAREST = 0, LF_MASK_BILINEAR = 1 } lf_mask_filter;
lf_status lf_set_mask_filter(lf_ctx* ctx, int filter);
lf_status lf_get_mask_filter(lf_ctx* ctx, int* filter);
/* host arithmetic, no device (like lf_coating_reflectance): the float32 contract of the stop-mask lookup.
 * texels = w x h floats, row-major; u, v = stop-plane coordinates hx / stop_h, hy / stop_h (finite).  value = the
 * transmission the march multiplies into the weight, open = 1 iff the ray survives the mask (LF_MASK_NEAREST:
 * value = the texel hit, open = value > 0; LF_MASK_BILINEAR: as above).  Either output may be NULL. */
lf_status lf_mask_lookup(const float* texels, int w, int h, int filter, float u, float v,
                         float* value, int* open);

/* replaces the lens-table globals of pathtracer.cpp:541-556 (Ts, red/green/blue_refr,
 * curvatures) and the constants of trace_ray_auto_* (:619-633): n interfaces, ior[3][n] row-major.
 * Passing NULL arrays restores the reference's hard-coded table. */
lf_status lf_set_paraxial_lens(lf_ctx* ctx, int n, int stop_index, const float* thickness,
                               const float* curvature, const float* ior_rgb);

/* replaces Camera state read by find_sun_pos (camera.h:171-180; camera.cpp:245-273):
 * c2w row-major 3x3, position, fields of view in DEGREES (already fitted to the aspect ratio) */
lf_status lf_set_camera(lf_ctx* ctx, const double c2w[9], const double pos[3], double hfov_deg,
                        double vfov_deg);
/* replaces: PathTracer::find_sun_pos (pathtracer.cpp:32-64).  lights: n x {posLight xyz,
 * radiance rgb} of the scene's DirectionalLights (src/scene/light.h:16-29). */
lf_status lf_find_sun_pos(lf_ctx* ctx, const double* lights, int n_lights);
/* direct write / read of the public fields flare_origins, flare_radiance, axis_ray,
 * angle_to_sun (pathtracer.h:128-135).  origins: n x 2, radiance: n x 3. */
lf_status lf_set_flares(lf_ctx* ctx, int n, const double* origins, const double* radiance,
                        const double axis_ray[2], float angle_to_sun);
lf_status lf_get_flares(lf_ctx* ctx, int* n, double* origins, double* radiance,
                        double axis_ray[2], float* angle_to_sun);

/* sub-pixel jitter of calculate_irradiance_falloff (pathtracer.cpp:1043-1063).
 * MT19937: reproduce the reference's shared std::mt19937 (util/random_util.h:10-22) for a single
 * worker visiting `order` (pixel index x + y*W; NULL = the reference's 32x32 tile order,
 * raytraced_renderer.cpp:314-328,:637-641).  COUNTER: order-free Philox4x32-10 keyed by `key`. */
lf_status lf_set_jitter_mt19937(lf_ctx* ctx, uint32_t seed, const uint32_t* order, size_t n_order);
lf_status lf_set_jitter_counter(lf_ctx* ctx, uint64_t key);

/* optional scene-radiance term (est_radiance_global_illumination averaged as in
 * pathtracer.cpp:841-875) computed by the host: W*H*3 doubles, NULL = zero */
lf_status lf_set_scene_term(lf_ctx* ctx, const double* rgb);

/* ---------------------------------------------------------------- scene term (row f2) ---- */
/* The static scene the sample loop of raytrace_pixel shades (pathtracer.cpp:841-875): replaces
 * PathTracer::bvh / scene (pathtracer.h:116-124) for spheres (scene/sphere.h), triangles
 * (scene/triangle.h) with DiffuseBSDF / EmissionBSDF materials (pathtracer/bsdf.h:122-153,
 * :271-288) and DirectionalLight / PointLight (scene/light.h:16-29, :47-58).
 *   spheres        n x {cx, cy, cz, r}
 *   tri_positions  n x 9 (p1 p2 p3), tri_normals n x 9 (vertex normals n1 n2 n3)
 *   materials      n x {kind, r, g, b}: kind 0 = diffuse reflectance, 1 = emitted radiance,
 *                  2 = diffuse given as the BSDF value f = reflectance / pi (what DiffuseBSDF::f
 *                  returns, bsdf.cpp:52-60: for hosts that can call f() but not read `reflectance`)
 *   lights         n x {type, x, y, z, r, g, b}: type 0 = directional (xyz = dirToLight, unit),
 *                  1 = point (xyz = position); rgb = radiance.  Order = order in scene->lights.
 * Other light and BSDF types are refused (LF_ERR_INVALID): see lf_scene.hip. */
lf_status lf_set_scene(lf_ctx* ctx, int n_spheres, const double* spheres, const int* sphere_material,
                       int n_triangles, const double* tri_positions, const double* tri_normals,
                       const int* tri_material, int n_materials, const double* materials,
                       int n_lights, const double* lights);
/* The lights of the current scene in their general form (replaces the lights lf_set_scene took; the
 * order is the order of scene->lights): n x 16 doubles
 *   {type, r, g, b,  v0 xyz,  v1 xyz,  v2 xyz,  v3 xyz}
 *   type 0 DirectionalLight          v0 = dirToLight                       (scene/light.h:16-29)
 *        1 PointLight                v0 = position                         (:47-58)
 *        2 InfiniteHemisphereLight   (no vectors)                          (:31-44, light.cpp:26-48)
 *        3 AreaLight                 v0 = position, v1 = direction, v2 = dim_x, v3 = dim_y  (:78-97, light.cpp:74-101)
 *        4 EnvironmentLight          (no vectors, rgb unused: the map of lf_set_environment_map;
 *                                    scene/environment_light.cpp:140-171 -- the renderer appends
 *                                    it to scene->lights, raytraced_renderer.cpp:127-128)
 * Types 2, 3 and 4 are SAMPLED lights: lf_set_light_samples(ns_area_light) samples each per hit
 * (PathTracer::ns_area_light, pathtracer.h:108; estimate_direct_lighting_importance,
 * pathtracer.cpp:143-213), drawn from the counter RNG -- they need lf_set_jitter_counter (the
 * reference's shared MT19937 is consumed in hit order, which no parallel schedule reproduces) and are
 * validated statistically against reference frames, not bit for bit. */
/* the box around the scene's primitives (what Application::load asks GLScene::Scene::get_bbox for to
 * place its camera, application.cpp:277-300) and how many there are */
lf_status lf_scene_bounds(lf_ctx* ctx, double bmin[3], double bmax[3], int* n_primitives);
lf_status lf_set_scene_lights(lf_ctx* ctx, int n_lights, const double* rows);
lf_status lf_set_light_samples(lf_ctx* ctx, int ns_area_light);
/* PathTracer::envLight (pathtracer.h:119; `new EnvironmentLight(envmap)`, raytraced_renderer.cpp:
 * 80-84): the environment map.  rgb = HDRImageBuffer::data, w*h texels of 3 doubles, row-major (the
 * .exr decoder stays with the host).  A camera ray that hits nothing returns
 * EnvironmentLight::sample_dir (pathtracer.cpp:291-292; environment_light.cpp:173-182, bilinear
 * in (theta, phi) with its edge rules) -- deterministic, so it is also served in MT19937 parity mode;
 * listed as a light of type 4 it is importance-sampled through the tables of
 * EnvironmentLight::init (:19-59), built here in the reference's order of operations (the
 * probability_debug.png the reference writes as a side effect is not written).  w = h = 0 removes
 * the map.  Maps smaller than 2 x 2 or without any light are refused. */
lf_status lf_set_environment_map(lf_ctx* ctx, int w, int h, const double* rgb);
/* PathTracer::direct_hemisphere_sample (pathtracer.h:114, the -H flag): one_bounce_radiance
 * (pathtracer.cpp:222-232) uses estimate_direct_lighting_hemisphere (:86-138) -- uniform directions
 * over the hemisphere, lights.size() * ns_area_light per hit, collecting the emission of the
 * surfaces they reach -- instead of sampling the lights.  Counter RNG only, statistical parity. */
lf_status lf_set_direct_hemisphere_sample(lf_ctx* ctx, int on);
/* Row f3: a COLLADA file -> the static scene, in one call.  Replaces
 * Collada::ColladaParser::load (src/scene/collada/collada.cpp:131-218) + Application::load
 * (src/application/application.cpp:232-365) + the GLScene -> SceneObjects conversion behind them
 * (gl_scene/mesh.cpp, util/halfEdgeMesh.cpp, scene/object.cpp, gl_scene/ *_light.h): parses the file
 * on the host (lens-flare_amd/host/lf_collada.cpp; triangles, vertex normals, lights and camera come
 * out bit-identical to the reference's, tests/test_collada_loader.py) and hands the result to
 * lf_set_scene / lf_set_scene_lights.  Lights are uploaded in node order: directional, point, area
 * and ambient (= infinite hemisphere) lights.
 *   camera          (may be NULL) what Application::load derives from the file's camera node(s)
 *   sun_lights      (may be NULL) for lf_find_sun_pos: 6 doubles per DirectionalLight, posLight
 *                   xyz + radiance rgb; at most max_sun_lights are written, *n_sun_lights = found
 * Mirror / glass / refraction / microfacet BSDFs are unfilled stubs in the reference (f() = 0, no
 * emission, advanced_bsdf.cpp:17-133) under a direct-lighting-only integrator (pathtracer.cpp:
 * 282-302): such surfaces are black occluders there and are uploaded as exactly that.
 * LF_ERR_INVALID with a message if the file has a spot light (a stub in the reference whose
 * sample_L leaves its outputs uninitialised, light.cpp:64-72) or what the reference itself cannot
 * load (it exits or reads uninitialised memory there).  lf_collada_check answers the
 * same question for a file without a device (0 = renderable; msg receives the reason otherwise). */
typedef struct {
  int present;
  double hfov, vfov, nclip, fclip;
  double pos[3], dir[3], up[3];
} lf_collada_camera;
lf_status lf_load_collada(lf_ctx* ctx, const char* path, lf_collada_camera* camera,
                          double* sun_lights, int max_sun_lights, int* n_sun_lights);
lf_status lf_collada_check(const char* path, char* msg, size_t msg_cap);
/* replaces the public fields samplesPerBatch / maxTolerance (pathtracer.h:112-113) and
 * Camera::nClip / fClip (camera.h:188) */
lf_status lf_set_sampling(lf_ctx* ctx, int samples_per_batch, double max_tolerance, double n_clip,
                          double f_clip);
/* replaces the sample loop of PathTracer::raytrace_pixel (pathtracer.cpp:831-875) for every pixel
 * of the band: ns_aa jittered pinhole rays -> closest hit -> emission + direct lighting, adaptive
 * early-out, divided by the loop variable (ns_aa + 1 without early-out).  The result becomes the
 * scene term lf_render_flare_layer composes.  Pixel jitter follows lf_set_jitter_*. */
lf_status lf_render_scene_term(lf_ctx* ctx);

/* ---------------------------------------------------------------- render ----------------- */
/* replaces: PathTracer::generate_ghost_buffer (pathtracer.cpp:714-817): paraxial trace of the
 * 13 reflection pairs x 3 colours and rasterisation of the 39 textured quads */
lf_status lf_generate_ghost_buffer(lf_ctx* ctx);
/* replaces: PathTracer::raytrace_pixel (pathtracer.cpp:819-899) for every pixel of the band:
 * sample = scene + ghost_buffer + raytrace_starburst (incl. calculate_irradiance_falloff) */
lf_status lf_render_flare_layer(lf_ctx* ctx);

/* ---------------------------------------------------------------- helper members ---------- */
/* The reference declares the steps of generate_ghost_buffer / raytrace_starburst as public members
 * ("Testing functions", pathtracer.h:42-57, :95-101).  A replacement of pathtracer.cpp defines every
 * one of them; these are their device forms (one small launch each; the frame-level calls above do
 * not go through them).  The ghost helpers ADD to the device ghost buffer, triangle by triangle like
 * HDRImageBuffer::update_pixel_additive (util/image.h:145); bbox (may be NULL) receives the pixel
 * rectangle [x0, x1) x [y0, y1) the call can have touched, for a partial read-back.
 *
 * replaces: ghost_buffer.clear() (generate_ghost_buffer, pathtracer.cpp:719; util/image.h:233) */
lf_status lf_clear_ghost_buffer(lf_ctx* ctx);
/* replaces: PathTracer::draw_ghost(string color, float r1, float r2) (pathtracer.cpp:433-508):
 * channel 0 / 1 / 2 = "red" / "green" / any other string; uses axis_ray of the flare state */
lf_status lf_draw_ghost(lf_ctx* ctx, int channel, float r1, float r2, int bbox[4]);
/* replaces: PathTracer::rasterize_textured_triangle (pathtracer.cpp:346-410);
 * v = {x0, y0, u0, v0,  x1, y1, u1, v1,  x2, y2, u2, v2}, colour = ghost_color */
lf_status lf_rasterize_textured_triangle(lf_ctx* ctx, const float v[12], const double colour[3], int bbox[4]);
/* replaces: PathTracer::fill_textured_pixel (pathtracer.cpp:305-343): vertices as given (already
 * y-sorted and shifted by the caller), pixel (x, y) inside the frame */
lf_status lf_fill_textured_pixel(lf_ctx* ctx, const float v[12], int x, int y, const double colour[3]);
/* replaces: PathTracer::shift_vertex (pathtracer.cpp:412-430) */
lf_status lf_shift_vertex(lf_ctx* ctx, float x, float y, float scale, float shift_amount, double out_xy[2]);
/* replaces: PathTracer::compute_phase (pathtracer.cpp:917-931) with complex_exp (:901-915);
 * screen_pos (may be NULL) = the flare origin in pixels the member returns through its reference */
lf_status lf_compute_phase(lf_ctx* ctx, int flare, double u, double v, double out_re_im[2], double screen_pos[2]);
/* replaces: PathTracer::calculate_irradiance_falloff(x, y, radius) (pathtracer.cpp:1043-1063); the
 * 32 jitter draws are pixel (x, y)'s own (lf_set_jitter_*) */
lf_status lf_irradiance_falloff(lf_ctx* ctx, int x, int y, double radius, double rgb[3]);
/* Single-ray forms of the integrator members (pathtracer.h:66-77) on the device scene of
 * lf_set_scene.  ray = {origin xyz, direction xyz, min_t, max_t}.  Sampled lights draw from the
 * counter RNG, stream `seq` (any number; distinct calls should pass distinct values).
 * replaces: PathTracer::est_radiance_global_illumination (pathtracer.cpp:282-302) and the closest-hit
 * query of PathTracer::autofocus (:1065-1072): out = {hit (1/0), t, normal xyz, radiance rgb};
 * without a hit the radiance is the environment's (or 0). */
lf_status lf_scene_trace_ray(lf_ctx* ctx, const double ray[8], uint64_t seq, double out[8]);
/* replaces, for an intersection (t, n, material) the host found itself: what = 0
 * PathTracer::zero_bounce_radiance (:215-220), 1 one_bounce_radiance (:222-232, by
 * lf_set_direct_hemisphere_sample), 2 estimate_direct_lighting_hemisphere (:86-138),
 * 3 estimate_direct_lighting_importance (:142-213).  material = {kind, r, g, b} as lf_set_scene. */
lf_status lf_scene_shade(lf_ctx* ctx, int what, const double ray[8], double t, const double n[3],
                         const double material[4], uint64_t seq, double rgb[3]);

/* ---------------------------------------------------------------- read back -------------- */
/* replaces reads of PathTracer::sampleBuffer / ghost_buffer (util/image.h:139-151).
 * which: 0 = sampleBuffer, 1 = ghost_buffer, 2 = the value of raytrace_starburst(x,y)
 * (pathtracer.cpp:947-1004: starburst + irradiance falloff) on its own, so that a host which
 * computes its scene radiance per pixel can form (scene + ghost) + starburst exactly like
 * pathtracer.cpp:891; 3 = the scene-radiance term itself (what lf_render_scene_term or
 * lf_set_scene_term left: the average of est_radiance_global_illumination over the pixel's camera
 * rays, pathtracer.cpp:841-875; LF_ERR_STATE when there is none; under a row interleave only this
 * context's tile rows are filled -- the term is consumed by the flare layer, not exchanged).  dst receives (x1-x0)*(y1-y0) pixels, each
 * `pixel_stride` doubles apart (3 = packed Vector3D, 4 = the AVX build's 32-byte Vector3D). */
lf_status lf_read_tile(lf_ctx* ctx, int which, int x0, int y0, int x1, int y1, double* dst,
                       size_t pixel_stride);
lf_status lf_read_pixel(lf_ctx* ctx, int which, int x, int y, double rgb[3]);
/* replaces: PathTracer::write_to_framebuffer -> HDRImageBuffer::toColor (util/image.h:208-223,
 * :53-62): RGBA8 of the tile, dst rows `row_stride` uint32 apart */
lf_status lf_write_to_framebuffer(lf_ctx* ctx, int x0, int y0, int x1, int y1, uint32_t* dst,
                                  size_t row_stride);
/* replaces the pixel preparation of RaytracedRenderer::save_image
 * (raytraced_renderer.cpp:739-746): the whole tonemapped frame with rows flipped (PNG is top-down)
 * and alpha forced to 0xFF, W*H uint32 ready for lodepng::encode (the encoder stays with the host) */
lf_status lf_save_image_rgba(lf_ctx* ctx, uint32_t* dst);
/* device pointer of a buffer (for RCCL gathers over xGMI without a host hop);
 * which as in lf_read_tile; layout W*H*3 doubles row-major.  The allocation is padded to a
 * multiple of 64 rows (bytes reports the padded size) so that in-place all-gathers of whole
 * tile-row groups never run past the end. */
lf_status lf_device_buffer(lf_ctx* ctx, int which, void** dptr, size_t* bytes);

/* ---------------------------------------------------------------- multi-GPU -------------- */
/* Replaces the reference's scale-out, which lives in the host: a mutex-guarded queue of 32x32 tiles
 * drained by std::threads (src/pathtracer/raytraced_renderer.cpp:314-328, :352-354, :681-715;
 * src/util/work_queue.h:11-51).  The 8-row sensor tile rows are dealt round-robin to the GPUs
 * (lf_set_row_interleave), every GPU renders its tile rows, and ONE RCCL all-gather per frame (over
 * xGMI) completes the frame on every GPU; there is no other data-path collective.  RCCL is loaded at
 * first use (dlopen): LF_ERR_STATE if it is not installed.
 *
 * One process per GPU: rank 0 calls lf_comm_get_unique_id, the host shares the id (MPI,
 * torch.distributed, a file ...), every rank calls lf_comm_init_rank after lf_set_frame -- it also
 * sets the row interleave (rank, nranks).  lf_comm_gather(which) after rendering: buffer `which`
 * (as lf_read_tile) then holds the whole frame on every rank; it is enqueued on the context's stream. */
#define LF_COMM_ID_BYTES 128
lf_status lf_comm_get_unique_id(unsigned char id[LF_COMM_ID_BYTES]);
lf_status lf_comm_init_rank(lf_ctx* ctx, int nranks, int rank, const unsigned char id[LF_COMM_ID_BYTES]);
lf_status lf_comm_gather(lf_ctx* ctx, int which);
/* The same exchange on the context's second stream, so that it overlaps what the host queues next
 * (a sequence of frames: frame k + 1 is marched while frame k is exchanged).  The main stream waits
 * only until this rank's rows have been copied out; the rows the exchange fills in belong to other
 * ranks.  lf_comm_wait makes the main stream wait for the exchange; lf_synchronize and the read
 * functions (lf_read_tile / _pixel, lf_write_to_framebuffer, lf_save_image_rgba) do so themselves.
 * Until then the buffer's rows of the OTHER ranks are undefined; do not change the frame size, band or
 * interleave while an exchange is pending (those calls drain it first). */
lf_status lf_comm_gather_async(lf_ctx* ctx, int which);
/* What a rank hands to the collective for a communicator of `world` ranks, computed where lf_comm_gather,
 * lf_comm_gather_async and lf_group_gather (RCCL and the peer-copy stand-in alike) compute it: out =
 * {sendcount of the ncclAllGather in elements, bytes per element, byte offset of the receive area in the
 * staging buffer, staging bytes, groups of `world` consecutive tile rows, elements per tile row}.  Rank q's
 * sendcount elements arrive at receive area + q * sendcount.  Inspection for tests and hosts that bring
 * their own transport; nothing is allocated or sent. */
lf_status lf_comm_exchange_plan(lf_ctx* ctx, int world, uint64_t out[6]);
lf_status lf_comm_wait(lf_ctx* ctx);
lf_status lf_comm_destroy(lf_ctx* ctx);
/* LF_OK if RCCL can be loaded here (dlopen + every entry point): what every rank checks, and agrees
 * on over its control plane, BEFORE the first blocking RCCL call */
lf_status lf_comm_available(void);
/* what RCCL reports for the communicator the context is attached to (ncclCommCount,
 * ncclCommUserRank); nranks = 0, rank = -1 without one */
lf_status lf_comm_info(lf_ctx* ctx, int* nranks, int* rank);
/* non-blocking: has the last exchange (lf_comm_gather or _async) finished on the device?  Lets a host
 * wait for the first collective of a new communicator with a deadline instead of blocking in
 * lf_synchronize behind a peer that never joined */
lf_status lf_comm_test(lf_ctx* ctx, int* done);
/* ncclCommAbort: ends the collectives in flight on this rank and drops the communicator, so that the
 * context's streams drain; the recovery from a failed first exchange (every rank calls it) */
lf_status lf_comm_abort(lf_ctx* ctx);
/* bits = 64 (default): tile rows travel as the doubles they are (every rank holds the same bits);
 * 32: as floats -- half the bytes on the wire (SURVEY 8e budgets f32: 12.4 MB per rank at 4K), the
 * rows a rank receives are rounded to float, its own stay as rendered.  Same value on every rank. */
lf_status lf_comm_set_exchange_precision(lf_ctx* ctx, int bits);
/* Giving up on a communicator call that is BLOCKED in another host thread (ncclCommInitRank and a communicator's
 * first collective block until every peer has joined; a peer that died never does).  The thread that waited for
 * the deadline calls lf_comm_poison: from then on the blocked call -- should it ever return -- publishes nothing
 * into the context (a communicator that arrives late is aborted where it stands), every lf_comm_* call on the
 * context returns LF_ERR_STATE, lf_comm_abort still ends what can be ended, and lf_destroy returns LF_ERR_STATE
 * WITHOUT freeing anything while the blocked call has not come back (the context is leaked on purpose: the
 * blocked thread still stands on it).  There is no way back: the process falls back to another exchange or exits. */
lf_status lf_comm_poison(lf_ctx* ctx);
int lf_comm_is_poisoned(lf_ctx* ctx);
/* One process, n devices (a C++ host such as the CGL application): one context + stream per device
 * and one communicator over them (ncclCommInitAll).  Set-up calls go to every context
 * (lf_group_ctx); lf_group_set_frame = lf_set_frame + the round-robin deal on every context;
 * lf_group_for_each runs fn(ctx, rank, user) on one host thread per device, concurrently -- the
 * per-frame sequence (lf_find_sun_pos, lf_trace_ghosts, lf_render_flare_layer ...) goes there, like
 * the reference's worker threads; lf_group_gather exchanges the finished tile rows and returns when
 * every device holds the whole frame.  A device listed twice (a rehearsal on a one-GPU box) cannot
 * join an RCCL communicator: such a group exchanges with peer copies instead. */
typedef struct lf_group lf_group;
typedef lf_status (*lf_group_fn)(lf_ctx* ctx, int rank, void* user);
lf_status lf_group_create(lf_group** out, int n, const int* devices);
lf_status lf_group_destroy(lf_group* g);
int lf_group_size(const lf_group* g);
lf_ctx* lf_group_ctx(lf_group* g, int rank);
const char* lf_group_last_error(const lf_group* g);
lf_status lf_group_set_frame(lf_group* g, int width, int height);
lf_status lf_group_for_each(lf_group* g, lf_group_fn fn, void* user);
lf_status lf_group_gather(lf_group* g, int which);
/* the cull pre-pass of the group's next lf_trace_ghosts(spp) shared between its devices (see lf_set_cull_share): every
 * context builds its slab, one all-gather, every context takes the table over.  Call it before the lf_group_for_each
 * that renders, once per launch; without it every device builds the whole table (until lf_group_share_cull has been
 * used once: from then on a launch without it is refused, like any launch of a host-shared table). */
lf_status lf_group_share_cull(lf_group* g, int spp);
/* the group's frame dealt by blocks of 64 x 64 pixels (lf_set_block_deal on every context; 0: back to tile rows, the
 * default of lf_group_set_frame).  lf_group_share_cull has nothing to do then. */
lf_status lf_group_set_block_deal(lf_group* g, int on);

/* ---------------------------------------------------------------- geometric lens --------- */
/* The north-star path: real ray march through spherical interfaces -- or, with lf_set_lens_aspheres, through
 * conic and even-polynomial aspheres on the same vertex curvatures.  The reference has no
 * counterpart (its lens is paraxial, pathtracer.cpp:511-689; Camera::generate_ray_for_thin_lens
 * is a stub, camera_lens.cpp:22-30), so this replaces `generate_ghost_buffer` when selected.
 *   radius[k]      signed radius of curvature in mm (0 = flat; the stop is flat)
 *   thickness[k]   axial distance vertex k -> vertex k+1 (last: to the sensor)
 *   ior[l*n + k]   index of the medium BEHIND interface k at wavelength l
 *   semi_ap[k]     clear semi-aperture in mm
 * Interface order: scene side first.  */
lf_status lf_set_lens(lf_ctx* ctx, int n_surfaces, int stop_index, int n_lambda,
                      const float* radius, const float* thickness, const float* ior,
                      const float* semi_aperture, float sensor_width_mm);
/* The same from a prescription file (lens-flare_amd/data/ *.lens: `sensor_width_mm w`, then one row
 * per interface `radius thickness n_1 .. n_L semi_aperture`, '#' comments; radius 0 with index 0 is
 * the stop).  Replaces the hard-coded table of pathtracer.cpp:541-556 as an INPUT, which is what
 * lets a host that cannot change the reference's header select a lens (LF_LENS_FILE). */
lf_status lf_load_lens_file(lf_ctx* ctx, const char* path);
/* Single-layer thin-film (anti-reflection) coatings on the interfaces of the geometric lens (no reference
 * counterpart).  n_surfaces / n_lambda must be those of the installed lens.
 *   lambda_nm[l]        vacuum wavelength of index column l of lf_set_lens, nm (> 0, finite)
 *   thickness_nm[k]     physical film thickness on interface k, nm, in [0, 10000]; 0 = uncoated (the stop: 0)
 *   index[l*n + k]      film index at wavelength l (ignored where thickness is 0), >= the smaller of the two
 *                       indices beside interface k at that wavelength
 * thickness_nm == NULL clears every coating.  A film changes only the Fresnel WEIGHT of the march's rays
 * (reflection and transmission at that interface, both directions, every path and the lens camera's
 * primary path), never where they go: the cull table, the counters and the lit pixel set stay those of the
 * bare lens.  lf_set_lens clears the coatings (they belong to the prescription); lf_focus_lens keeps them.
 * A lens file may carry them: `coating k thickness_nm m_1 .. m_L` (or one m for all wavelengths) after a
 * `lambda_nm l_1 .. l_L` line (lf_load_lens_file).  Only the weighted re-march of a lit path pays for a film:
 * the bench frame (c3) takes 52.2 ms with eight quarter-wave films against 43.8 ms bare (x 1.19,
 * profiles/coating_cost.json); a lens without films runs the kernels it always ran. */
lf_status lf_set_lens_coatings(lf_ctx* ctx, int n_surfaces, int n_lambda, const float* lambda_nm,
                               const float* thickness_nm, const float* index);
/* what lf_set_lens_coatings installed (any array may be NULL): zeros and n_coated = 0 for a bare lens.
 * LF_ERR_STATE while some interface holds a stack of two or more layers (lf_get_lens_coating_stacks reads those). */
lf_status lf_get_lens_coatings(lf_ctx* ctx, int n_surfaces, int n_lambda, float* lambda_nm,
                               float* thickness_nm, float* index, int* n_coated);
/* Multi-layer anti-reflection STACKS: up to LF_MAX_COAT_LAYERS lossless layers per interface.
 *   n_layers[k]                 layers on interface k, 0 .. LF_MAX_COAT_LAYERS (the stop: 0)
 *   thickness_nm[j*n + k]       physical thickness of layer j of interface k, nm, in [0, 10000]
 *   index[(j*L + l)*n + k]      its index at wavelength l (L = n_lambda), finite and >= the smaller of the two indices
 *                               beside interface k at that wavelength
 * Layer j = 0 is the one on the SCENE side of the interface: the order is fixed in space, and a ray travelling towards
 * the scene meets the layers reversed (the library reverses them when it derives each direction's constants).
 * With cm_j^2 = (n cos t)^2 + m_j^2 - n^2 the rule on the indices keeps the optical cosine cm_j of every layer real
 * wherever the interface itself does not reflect totally: there is no frustrated total reflection inside a stack.
 * Layers of thickness 0 are dropped before anything else happens; an interface left with exactly ONE layer is installed
 * as that single film -- the records, the arithmetic and the kernels of lf_set_lens_coatings, its frames bit for bit --
 * and only a lens with two or more layers on some interface launches the kernels that evaluate a stack (the
 * recursive Airy sum of lf_march_events.h stack_fraction: float32, nothing divided, one loop over the layers).
 * n_layers == NULL clears the stacks.  The two setters replace each other's state; lf_set_lens clears it, lf_focus_lens
 * keeps it.  Like a film, a stack changes only the weight: the cull table, the counters and the lit pixel set stay those
 * of the bare lens.  A lens file carries stacks as `layer k thickness_nm m_1 .. m_L` lines (or one m for all
 * wavelengths), each appending a layer to interface k, scene side first, after a `lambda_nm` line; an interface takes
 * `layer` lines or a `coating` line, not both.  Not modelled: absorbing layers (complex indices), graded or
 * dispersive-by-formula films. */
lf_status lf_set_lens_coating_stacks(lf_ctx* ctx, int n_surfaces, int n_lambda, const float* lambda_nm,
                                     const int* n_layers, const float* thickness_nm, const float* index);
/* what is installed, after the drop of zero-thickness layers (a single film of lf_set_lens_coatings reads as one layer);
 * the arrays are sized as for the setter with LF_MAX_COAT_LAYERS layers (any may be NULL), n_stacked = the interfaces
 * with two or more layers */
lf_status lf_get_lens_coating_stacks(lf_ctx* ctx, int n_surfaces, int n_lambda, float* lambda_nm, int* n_layers,
                                     float* thickness_nm, float* index, int* n_stacked);
/* host arithmetic, no device (like lf_coating_reflectance): the reflectance of ONE stacked interface in the float32
 * contract of the march (stack_fraction itself) -- out = {R_s, R_p, R} for a ray arriving in n_in at cosine cos_in; the
 * layers n_film[i], thickness_nm[i] in the order the RAY meets them; layers of thickness 0 are dropped, one layer left is
 * lf_coating_reflectance bit for bit, none the bare interface; total reflection gives 1 */
lf_status lf_coating_stack_reflectance(float n_in, int n_layers, const float* n_film, const float* thickness_nm,
                                       float n_out, float lambda_nm, float cos_in, float out[3]);
/* host arithmetic, no device (like lf_paraxial_efl): the coated reflectance of ONE interface in the float32
 * contract of the march -- out = {R_s, R_p, R = (R_s + R_p) / 2} for a ray arriving in n_in at cosine
 * cos_in (in [0, 1]) of its angle of incidence; thickness 0 gives the bare interface, total reflection 1 */
lf_status lf_coating_reflectance(float n_in, float n_film, float n_out, float thickness_nm,
                                 float lambda_nm, float cos_in, float out[3]);
/* ASPHERIC INTERFACES (no reference counterpart).  Interface k of the installed lens becomes the surface of revolution
 *   z(r^2) = c r^2 / (1 + sqrt(1 - (1 + kappa) c^2 r^2)) + r^4 (A4 + r^2 (A6 + r^2 (... A14)))
 * with c = 1 / radius[k] as lf_set_lens holds it (c = 0 with coefficients: a corrector plate), z along the axis from
 * the interface's vertex, r the distance from the axis in mm.
 *   conic[k]              kappa of interface k (0: a sphere, -1: a paraboloid)
 *   coef[m*n + k]         A(4 + 2 m) of interface k in mm^(1 - (4 + 2 m)), m = 0 .. n_coef - 1, n_coef in 0 .. LF_MAX_ASPH_COEF
 * There is NO r^2 coefficient: the vertex curvature stays 1 / radius, so everything paraxial is unchanged --
 * lf_paraxial_efl, lf_paraxial_image_scale, lf_paraxial_exit_pupil / _entrance_pupil, lf_focus_lens,
 * lf_aim_at_exit_pupil and the sun hand-over of lf_set_sun_from_flares; lf_get_lens_info keeps its meaning.
 * conic == NULL clears the aspheres.  A record of all zeros is no record: a lens whose records are all zero has no
 * aspheres and launches exactly the kernels it launched before.  lf_set_lens clears the aspheres (they belong to the
 * prescription); lf_focus_lens keeps them.  Refused with LF_ERR_INVALID and a message that names the interface: a
 * value that is not finite, a record on the stop, n_coef outside 0 .. LF_MAX_ASPH_COEF, an interface whose
 * 1 - (1 + kappa) c^2 h^2 is not positive in float at its own semi-aperture h (the conic ends inside the clear aperture),
 * a non-zero record on an interface that carries a biconic record (lf_set_lens_biconics).
 * A lens file carries them as `asphere k kappa [A4 [A6 ...]]` lines (lf_load_lens_file).
 * A lens with an asphere is marched by a kernel of its own (k_march_asph: every path alone from the sensor, a fixed
 * number of Newton steps from the base sphere's intersection on the aspheric rows, the unchanged spherical event on all
 * others); no cull table is built for it (lf_get_cull_reason: LF_CULL_ASPHERIC).  Films and stacks, every kind of light,
 * ghost occlusion, bands and deals work as on any lens.  The lens camera's scene image (lf_set_lens_camera,
 * lf_render_scene_term) refuses an aspheric lens with LF_ERR_UNSUPPORTED under the default setting, and so does
 * lf_get_lens_camera while a lens-camera mode is on (it would calibrate that image); lf_generate_lens_rays works.
 * lf_set_lens_camera_surfaces(LF_LENSCAM_SURFACES_ALL) lifts the refusal: the scene kernel then marches the records. */
lf_status lf_set_lens_aspheres(lf_ctx* ctx, int n_surfaces, const float* conic, int n_coef, const float* coef);
/* what is installed (any pointer may be NULL): conic[n_surfaces], coef[LF_MAX_ASPH_COEF * n_surfaces] laid out as the
 * setter's with n_coef = LF_MAX_ASPH_COEF, n_aspheric = the interfaces whose record is not all zero */
lf_status lf_get_lens_aspheres(lf_ctx* ctx, int n_surfaces, float* conic, float* coef, int* n_aspheric);
/* host arithmetic, no device: the sag z (mm) and dz / d(r^2) (1 / mm) of such a surface at r2 = r^2, in the float32
 * arithmetic of the march (every multiply-add fused, IEEE root and division).  LF_ERR_INVALID beyond the conic's domain. */
lf_status lf_asphere_sag(float curvature, float conic, int n_coef, const float* coef, float r2, float* z, float* dz_dr2);
/* host arithmetic, no device: ONE event of ONE ray on such an interface, the definition the kernels run (bit for bit:
 * lf_asphere_events is its device twin).  The interface: curvature, conic, coef[n_coef], semi_aperture, the index n_in of
 * the medium the ray arrives in and n_out of the one behind the interface along the ray (a mirror event's too: its ct);
 * reflect 0 / 1; forward 1: the ray travels +z (towards the sensor), 0: -z.  ray_in = {x, y, z, Kx, Ky, Kz}: the
 * position relative to the vertex of the interface the ray sits on, which lies dzv = (its vertex z) - (this interface's
 * vertex z) from this one's, and the OPTICAL direction K = n_in d.  ray_out: the same six at the hit, relative to this
 * interface's vertex, K' in the medium the ray leaves in.  sq = n_in |cos(incidence)|, ct = n_out cos(refraction): what
 * the Fresnel code of the march takes.  fate: 0 alive, 1 missed (beyond the conic's domain, or the iteration did not
 * converge), 2 outside the clear aperture, 3 totally reflected (a refraction only).  Any pointer of sq, ct may be NULL. */
lf_status lf_asphere_event(float curvature, float conic, int n_coef, const float* coef, float semi_aperture, float n_in,
                           float n_out, int reflect, int forward, float dzv, const float ray_in[6], float ray_out[6],
                           float* sq, float* ct, int* fate);
/* the same event for n rays on the device: rays n x 6 as ray_in, out n x 8 = {ray_out, sq, ct}, fates n ints */
lf_status lf_asphere_events(lf_ctx* ctx, float curvature, float conic, int n_coef, const float* coef, float semi_aperture,
                            float n_in, float n_out, int reflect, int forward, float dzv, size_t n, const float* rays,
                            float* out, int* fates);
/* lf_generate_lens_rays generalised to the ghost path of pair (i, j): the ray of sensor point / pupil sample k is
 * marched along the pair's event sequence -- towards the scene down to interface i, mirrored there, back up to j > i,
 * mirrored again, out through the front element -- with the march's own events and weight (films, stacks, the stop
 * mask under the installed filter, aspheres).  i = j = -1: the primary path.  out: n x 8 floats as
 * lf_generate_lens_rays defines them.  Works for any lens; on an aspheric one lf_generate_lens_rays routes through it. */
lf_status lf_march_path_rays(lf_ctx* ctx, int lambda, int i, int j, size_t n, const float* sensor_xy_mm,
                             const float* pupil_uv, float* out);
/* SENSOR GHOSTS: the sensor as a mirror behind the lens (no reference counterpart).  A sensor's cover glass and silicon
 * reflect a few per cent of the focused image back into the lens, and the rear elements return it as a second, defocused
 * image of the light.  The sensor path of interface i (any interface but the stop) of a sensor sample is marched from the
 * sensor like every other path: interfaces n-1 .. i+1 refracted towards the scene, mirrored at i, i+1 .. n-1 refracted
 * towards the sensor, mirrored at the sensor plane, n-1 .. 0 refracted and out -- 3 n - 2 i events, every stop crossing the
 * stop's own event with its mask.  The sensor's event carries the ray to z = z_sensor and flips d_z; the weight is
 * multiplied by reflectance[lambda], one number per wavelength whatever the angle; a ray that lands outside the WHOLE
 * frame's rectangle |X| <= W pitch / 2, |Y| <= H pitch / 2 is lost; a wavelength whose reflectance is 0 is not marched.
 * The lit ray is what any ghost ray is: every kind of light, several lights, films, stacks, the bilinear stop, aspheric and
 * biconic records, ghost occlusion with both reaches, bands and deals are the code that exists.  The sensor paths ALWAYS aim
 * at the default disc -- the rear element's clear aperture at its vertex plane -- whatever lf_set_pupil_target or
 * lf_aim_at_exit_pupil holds for the ordinary paths: their first mirror lies behind the stop, or sends the light through it a
 * second and third time (the comment on lf_set_pupil_target).  They enter neither the pair selection nor the path tree nor the
 * cull table: every selected sensor path of every sample is marched on its own, unculled -- about 3 n - 2 i events per path,
 * sample and wavelength, a multiple of the default frame's cost.  Out of scope: angle- or polarisation-dependent reflectance,
 * diffuse or microlens-diffraction reflection, paths that meet the sensor twice.
 *
 * lf_set_sensor_reflectance: one value in [0, 1] per index column of the installed lens; NULL clears.  A wrong n_lambda, a
 * value that is not finite or out of range: LF_ERR_INVALID, the previous state stays.  lf_set_lens clears the values (they
 * belong to the prescription's columns), lf_focus_lens keeps them -- as the coatings.  The getter: *installed 0 / 1;
 * reflectance (n_lambda floats, may be NULL) zeros while none is installed. */
lf_status lf_set_sensor_reflectance(lf_ctx* ctx, int n_lambda, const float* reflectance);
lf_status lf_get_sensor_reflectance(lf_ctx* ctx, int n_lambda, float* reflectance, int* installed);
/* The mode, a setting of the context (it survives lf_set_lens): OFF, the default -- lf_trace_ghosts launches exactly the kernels
 * it always launched; ADD -- it marches the ordinary selection as ever and then adds the sensor paths to the ghost buffer;
 * ONLY -- the ordinary march is skipped, the sensor paths replace the buffer (or add to it under lf_set_ghost_accumulate).
 * interfaces: n distinct interfaces, none the stop or out of range (else LF_ERR_INVALID, the previous state stays); NULL: every
 * interface but the stop, of whatever lens is installed at the launch.  ADD or ONLY without a reflectance makes lf_trace_ghosts
 * return LF_ERR_STATE.  The getter: the interfaces a launch would march, in its order (cap: the list's room; any pointer may be
 * NULL). */
enum { LF_SENSOR_GHOSTS_OFF = 0, LF_SENSOR_GHOSTS_ADD = 1, LF_SENSOR_GHOSTS_ONLY = 2 };
lf_status lf_set_sensor_ghosts(lf_ctx* ctx, int mode, const int* interfaces, int n);
lf_status lf_get_sensor_ghosts(lf_ctx* ctx, int* mode, int* interfaces, int cap, int* n);
/* lf_march_path_rays' twin for the sensor path of interface i: the same eight floats per ray, the weight with
 * reflectance[lambda]; follows films, stacks, aspheric and biconic records and the mask filter; aims at the default disc.
 * A lens with pose records: LF_ERR_UNSUPPORTED under LF_SENSOR_SURFACES_CENTRED, marched under LF_SENSOR_SURFACES_POSED
 * (lf_set_sensor_ghost_surfaces, below). */
lf_status lf_march_sensor_path_rays(lf_ctx* ctx, int lambda, int i, size_t n, const float* sensor_xy_mm, const float* pupil_uv,
                                    float* out);
/* Which interfaces a sensor path may meet, a setting of the context (nothing clears it: not lf_set_lens, not lf_focus_lens):
 *   LF_SENSOR_SURFACES_CENTRED   the default: every interface on the axis.  A lens with pose records (lf_set_lens_poses) is
 *                                refused with LF_ERR_UNSUPPORTED by lf_trace_ghosts under LF_SENSOR_GHOSTS_ADD / _ONLY and by
 *                                lf_march_sensor_path_rays.
 *   LF_SENSOR_SURFACES_POSED     both march such a lens: every crossing of a posed interface -- three for one behind the
 *                                path's mirror: towards the scene, towards the sensor, towards the scene -- is
 *                                lf_march_path_rays' posed event (lf_pose_event) with the row's own direction of travel; a
 *                                ray that meets the face from behind is lost there.  The stop and the sensor carry no pose.
 *                                On a lens without pose records the setting changes nothing: the same kernels, the same bits.
 * Any other value: LF_ERR_INVALID, the previous one stays.  The sensor paths keep aiming at the default disc, and that disc
 * is the CENTRED rear element's clear aperture at its nominal vertex plane, also when that element is decentred -- the
 * convention of the ordinary march of a posed lens and of the lens camera: it says where the samples aim, the event itself
 * is not approximated. */
enum { LF_SENSOR_SURFACES_CENTRED = 0, LF_SENSOR_SURFACES_POSED = 1 };
lf_status lf_set_sensor_ghost_surfaces(lf_ctx* ctx, int which);
lf_status lf_get_sensor_ghost_surfaces(lf_ctx* ctx, int* which);
/* host only: the events of the sensor path of interface i in marching order, out[e] = interface | reflect << 8 | forward << 9
 * with n_surfaces standing for the sensor's mirror; *n_events = 3 n_surfaces - 2 i.  LF_ERR_INVALID: i the stop or out of range,
 * cap too small. */
lf_status lf_sensor_path_sequence(int n_surfaces, int stop_index, int i, int* out, int cap, int* n_events);
/* host only: the sensor's event on ONE ray, the kernels' own definition (bit for bit).  ray_in {x, y, z, Kx, Ky, Kz}: z relative to
 * the vertex the ray sits on, dzv = that vertex's z minus the sensor plane's, K any multiple of the direction, K_z > 0.
 * ray_out: the point on the plane (z = 0) and the mirrored direction; *inside: |x| <= half_width_mm and |y| <= half_height_mm. */
lf_status lf_sensor_mirror_event(const float ray_in[6], float dzv, float half_width_mm, float half_height_mm, float ray_out[6],
                                 int* inside);
/* Since the last lf_reset_counters: {sensor-path rays started, rays that reached the sensor's mirror, of those lost off the
 * rectangle there, lit (ray, light) contributions}.  lf_get_counters, lf_get_executed_events and lf_get_march_stats keep
 * describing the ordinary paths alone, under ADD too.  lf_timing_get's slot of the launch: "march_sensor"; "sensor_table"
 * counts the uploads of the sensor paths' table (one when its rows or pose records changed, none for an unchanged frame). */
lf_status lf_get_sensor_ghost_stats(lf_ctx* ctx, uint64_t out[4]);
/* BICONIC INTERFACES: cylinders, toroids, the anamorphic flare (no reference counterpart).  Interface k of the installed
 * lens becomes
 *   z(x, y) = (cx x^2 + cy y^2) / (1 + sqrt(1 - (1 + kx) cx^2 x^2 - (1 + ky) cy^2 y^2))
 * x and y the sensor's axes (no rotation angle, no polynomial terms), cy = 1 / radius[k] as lf_set_lens holds it (the y
 * meridian; 0 for a plane) and
 *   on[k]        != 0: interface k carries a record
 *   radius_x[k]  Rx, the x meridian's signed radius of curvature in mm (0 = flat in x), cx = 1 / Rx
 *   conic_x[k], conic_y[k]   the two conic constants (NULL: zeros)
 * A circular cylinder with power in x is a flat row with a record Rx != 0; one with power in y a curved row with the
 * record Rx = 0 -- which is why `on` says where a record is: a record of zeros is one.  So is a record whose 1 / Rx equals
 * cy with kx = ky = 0, a sphere: it takes the biconic route (the same surface through another event).
 * Everything paraxial keeps meaning the Y MERIDIAN and changes no bit: lf_paraxial_efl, lf_paraxial_image_scale, the
 * pupils, lf_focus_lens, lf_aim_at_exit_pupil, lf_get_lens_info's efl_mm; ghost occlusion keeps mapping its shadow rays
 * through the y-meridian entrance pupil.  The one exception is the hand-over of a flare to a light (lf_set_sun_from_flares,
 * lf_set_lights_from_flares, lf_set_lights_from_scene): with efl_mm <= 0 the x component of the direction takes the image
 * scale of the x meridian (lf_get_lens_meridian_scales); a caller's efl_mm > 0 serves both, as for any lens.
 * on == NULL clears the records; lf_set_lens clears them, lf_focus_lens keeps them.  Refused with LF_ERR_INVALID and a
 * message that names the interface: a value that is not finite, a record on the stop, a record on an interface with a
 * non-zero aspheric record (lf_set_lens_aspheres refuses the converse; different interfaces of one lens may carry either
 * kind), a meridian whose 1 - (1 + k) c^2 h^2 is not positive in float at the semi-aperture h.
 * A lens file carries them as `biconic k Rx [kx [ky]]` lines (lf_load_lens_file; data/dgauss11_anamorphic.lens).
 * Such a lens is marched by the aspheric lens's kernel with one more branch (k_march_asph<VAR, true>: a fixed number of
 * Newton steps from the root of a start quadric, lf_biconic.h); no cull table is built (LF_CULL_ANAMORPHIC); lights, films,
 * stacks, occlusion, bands and deals work as on any lens; lf_march_path_rays and lf_generate_lens_rays follow the
 * records; the lens camera's scene image, and lf_get_lens_camera under a lens-camera mode, refuse the lens with
 * LF_ERR_UNSUPPORTED under the default setting as they do an aspheric one (lf_set_lens_camera_surfaces lifts both). */
lf_status lf_set_lens_biconics(lf_ctx* ctx, int n_surfaces, const int* on, const float* radius_x, const float* conic_x,
                               const float* conic_y);
/* what is installed (any pointer may be NULL): arrays of n_surfaces, n_biconic = the interfaces with a record */
lf_status lf_get_lens_biconics(lf_ctx* ctx, int n_surfaces, int* on, float* radius_x, float* conic_x, float* conic_y,
                               int* n_biconic);
/* the paraxial image scales (mm per radian of field angle, lf_paraxial_image_scale at the middle wavelength) of the two
 * meridians of the installed lens: scale_y of the prescription as lf_set_lens holds it, scale_x of the one with Rx in
 * place of the radius wherever a biconic record is on (equal for a lens without records).  Either pointer may be NULL. */
lf_status lf_get_lens_meridian_scales(lf_ctx* ctx, double* scale_x, double* scale_y);
/* host arithmetic, no device: the sag z (mm) and its slopes dz/dx, dz/dy of such a surface at (x, y), in the float32
 * arithmetic of the march.  LF_ERR_INVALID beyond the conic's domain. */
lf_status lf_biconic_sag(float curvature_x, float curvature_y, float conic_x, float conic_y, float x, float y, float* z,
                         float* dz_dx, float* dz_dy);
/* host arithmetic, no device: ONE event of ONE ray on a biconic interface, the definition the kernels run (bit for bit:
 * lf_biconic_events is its device twin).  curvature_x = 1 / Rx (0: flat in x), curvature_y the row's; every other
 * argument, the ray's conventions, sq, ct and the fates as lf_asphere_event's. */
lf_status lf_biconic_event(float curvature_x, float curvature_y, float conic_x, float conic_y, float semi_aperture, float n_in,
                           float n_out, int reflect, int forward, float dzv, const float ray_in[6], float ray_out[6],
                           float* sq, float* ct, int* fate);
/* the same event for n rays on the device: rays n x 6 as ray_in, out n x 8 = {ray_out, sq, ct}, fates n ints */
lf_status lf_biconic_events(lf_ctx* ctx, float curvature_x, float curvature_y, float conic_x, float conic_y, float semi_aperture,
                            float n_in, float n_out, int reflect, int forward, float dzv, size_t n, const float* rays,
                            float* out, int* fates);
/* POSED INTERFACES: decentred, tilted and rotated surfaces (no reference counterpart).  Interface k of the installed lens
 * becomes the surface
 *   P = V_k + t + R q,   R = Rx(ax) Ry(ay) Rz(az)
 * q on the interface as lf_set_lens, lf_set_lens_aspheres and lf_set_lens_biconics define it (vertex at the origin), V_k its
 * nominal vertex on the axis, and
 *   on[k]                  != 0: interface k carries a record (a record of zeros is one, as for biconics)
 *   decentre[3 k .. 3 k+2] t = (dx, dy, dz) in mm                                         (NULL: zeros)
 *   tilt_deg[3 k .. 3 k+2] (ax, ay, az), right-handed, in degrees; |ax|, |ay| <= 30, az in [-180, 180]   (NULL: zeros)
 * The turn about the surface's own z comes first: az is what rotates a cylinder's axis (az = 90 turns power in x into
 * power in y).  Each interface is posed on its own -- a record is no cumulative coordinate break; an ELEMENT tilted about a
 * pivot needs different records on its faces (the Python helper pose_group writes them).
 * on == NULL clears the records; lf_set_lens clears them, lf_focus_lens keeps them.  Refused with LF_ERR_INVALID and a
 * message that names the interface, the previous state kept: a wrong n_surfaces, a value that is not finite, a record on
 * the stop (a turned iris is a turned mask texture; a decentred one would move the stop event and the pupil aim), an angle
 * out of range.
 * A lens file carries them as `pose k dx dy dz ax ay az` lines (lf_load_lens_file; data/dgauss11_decentred.lens).
 * Such a lens is marched by the aspheric lens's kernel with one more branch (k_march_asph<VAR, true, true>, lf_pose.h): the
 * ray is carried into the surface's frame, meets the interface through the aspheric or the biconic event (a sphere or a
 * plane as a biconic), and is carried back -- the clear aperture is the glass's own, a ray that meets the surface from
 * behind is vignetted.  No cull table is built (LF_CULL_POSED); lights, films, stacks, occlusion, bands and deals work as on
 * any lens; lf_march_path_rays and lf_generate_lens_rays follow the records.  Refused with LF_ERR_UNSUPPORTED under the
 * default settings: sensor ghosts under LF_SENSOR_GHOSTS_ADD / _ONLY (at lf_trace_ghosts) with lf_march_sensor_path_rays
 * (lf_set_sensor_ghost_surfaces(LF_SENSOR_SURFACES_POSED) lifts both), and the lens camera's scene image under every setting of
 * lf_set_lens_camera_surfaces but LF_LENSCAM_SURFACES_POSED.  Everything paraxial -- pupils, focus, efl, the hand-over of a flare to a light -- stays the
 * centred lens's. */
lf_status lf_set_lens_poses(lf_ctx* ctx, int n_surfaces, const int* on, const float* decentre, const float* tilt_deg);
/* what is installed (any pointer may be NULL): on n_surfaces, decentre and tilt_deg 3 n_surfaces, n_posed = the records */
lf_status lf_get_lens_poses(lf_ctx* ctx, int n_surfaces, int* on, float* decentre, float* tilt_deg, int* n_posed);
/* host arithmetic, no device: ONE event of ONE ray on a posed interface, the definition the kernels run (bit for bit:
 * lf_pose_events is its device twin).  The arguments of lf_biconic_event, plus an aspheric record -- aspheric != 0: the
 * interface is the surface of revolution of curvature_y with conic constant kappa and coef[0 .. n_coef) = A4, A6 .. (the
 * biconic arguments are then not read); aspheric == 0: the biconic (curvature_x = curvature_y, conics 0: a sphere) -- and
 * the pose as lf_set_lens_poses takes it.  Output and fates as lf_biconic_event's; the ray in lens coordinates, z from the
 * interface's NOMINAL vertex. */
lf_status lf_pose_event(float curvature_x, float curvature_y, float conic_x, float conic_y, int aspheric, float kappa,
                        const float* coef, int n_coef, const float decentre[3], const float tilt_deg[3], float semi_aperture,
                        float n_in, float n_out, int reflect, int forward, float dzv, const float ray_in[6], float ray_out[6],
                        float* sq, float* ct, int* fate);
/* the same event for n rays on the device: rays n x 6 as ray_in, out n x 8 = {ray_out, sq, ct}, fates n ints */
lf_status lf_pose_events(lf_ctx* ctx, float curvature_x, float curvature_y, float conic_x, float conic_y, int aspheric, float kappa,
                         const float* coef, int n_coef, const float decentre[3], const float tilt_deg[3], float semi_aperture,
                         float n_in, float n_out, int reflect, int forward, float dzv, size_t n, const float* rays, float* out,
                         int* fates);
/* what lf_set_lens / lf_load_lens_file installed (any pointer may be NULL); efl_mm = lf_paraxial_efl at
 * the middle wavelength (0 for an afocal prescription) */
lf_status lf_get_lens_info(lf_ctx* ctx, int* n_surfaces, int* stop_index, int* n_lambda, float* sensor_width_mm,
                           double* efl_mm);
/* RGB weight of each wavelength (n_lambda x 3); default: identity for n_lambda == 3.
 * RANGE CONTRACT of the march's accumulators (lf_set_lambda_rgb, lf_set_sun, lf_trace_ghosts): a pixel
 * channel is the sum of UNSIGNED 64-bit fixed-point contributions (u64)(v 2^bits), so every weight and every
 * radiance must be finite and >= 0 -- anything else is refused with LF_ERR_INVALID (a host whose colour
 * matrix has negative lobes renders the positive and the negative weights as two frames and subtracts).
 * The magnitude is free: lf_trace_ghosts chooses `bits` per launch -- 36 (a grid of 1.5e-11 per sample)
 * unless the largest sum the launch could produce, spp x paths x (pupil solid angle) x
 * max_c sum_l radiance[c] weights[l][c], would then reach 2^62; in that case the largest exponent that
 * keeps it below (a sun of radiance 1e9 at 1024 spp x 8 wavelengths: 2^17; on the fixed 2^-36 grid of rounds
 * 1-4 such a frame wrapped from a radiance of ~6e7 on).  No sum can wrap, and a
 * frame at 2^k x the radiance is 2^k x the frame, bit for bit, once both leave the default grid.
 * lf_get_march_fix_bits reports the last launch's exponent. */
lf_status lf_set_lambda_rgb(lf_ctx* ctx, const float* weights);
/* the light: unit direction from the lens towards the sun in lens space (z < 0), radiance (finite, >= 0: see
 * the range contract above), angular radius of its (smooth) lobe in radians */
lf_status lf_set_sun(lf_ctx* ctx, const float dir[3], const float radiance[3],
                     float angular_radius);
/* SEVERAL lights in ONE pass of the march: n_lights (1 .. LF_MAX_LIGHTS) lights, dir[3 k ..], radiance[3 k ..],
 * angular_radius[k] as lf_set_sun's one -- each validated and stored exactly as lf_set_sun does (z < 0, finite,
 * radiance >= 0, 0 < radius <= 1.5; the direction normalised in double, then narrowed).  The call replaces ALL
 * lights; a refusal (LF_ERR_INVALID) leaves the previous ones installed.  lf_set_sun IS lf_set_lights(1, ...).
 * The contract:
 *   - the rays, their events and their fates do not depend on any light; a ray that ends inside several lobes
 *     contributes to each one: per (ray, light k, channel c) ONE value
 *     (u64)(contrib_k x radiance_k[c] x lambda_rgb[l][c] x 2^bits) is added, contrib_k = weight x (1 - q_k)^2
 *     being the single light's arithmetic with light k in the sun's place;
 *   - hence a frame of K lights is the SUM of the K single-light frames under the same key, sampling
 *     specification and `bits`, bit for bit;
 *   - the range contract above takes the sum over the lights of the radiances as its worst case
 *     (lf_get_march_fix_bits); under an HDR launch every light's radiance is uploaded scaled;
 *   - lf_counters::rays_hit_light counts (ray, light) contributions; every other counter counts rays, as with
 *     one light;
 *   - the cull table is built for all lights (a path starts where it can reach ANY of them: the bitwise OR of
 *     the lights' own tables) and its audit refutes it if a dropped ray ends inside any light's lobe.
 * A context with one light launches exactly the kernels it launched before this call existed.  More lights than
 * LF_MAX_LIGHTS: compose launches with lf_set_ghost_accumulate.
 * COST (the bench frame, 1080p x 256 spp, table resolved and audited inside every frame; profiles/multi_light_cost.json):
 * one light 34.95 ms, through the parent commit's library 34.93 (spreads 0.07: the single-light kernels are the parent's);
 * 2 / 4 / 8 lights of 0.05 rad spread over the frame in ONE launch 53.3 / 87.2 / 231.6 ms against 66.2 / 127.9 / 247.3 ms as
 * 2 / 4 / 8 launches under lf_set_ghost_accumulate (x 0.81 / 0.68 / 0.94).  The union of the lights' tables starts 9.3 / 12.1 /
 * 15.9 % of all paths (one light: 7.7 %); at 8 such lights that is past the fraction where the launch takes the path tree,
 * which marches everything once -- still ahead of eight culled launches.  The resolve takes 0.58 / 0.69 / 0.85 / 1.10 ms
 * with 1 / 2 / 4 / 8 lights. */
lf_status lf_set_lights(lf_ctx* ctx, int n_lights, const float* dir, const float* radiance, const float* angular_radius);
/* what lf_set_lights / lf_set_sun installed (any pointer may be NULL; arrays of LF_MAX_LIGHTS lights): the unit
 * directions and radiances as stored, the angular radii as given; *n_lights = 0 before any light */
lf_status lf_get_lights(lf_ctx* ctx, int* n_lights, float* dir, float* radiance, float* angular_radius);
/* LIGHTS AT A FINITE DISTANCE (point lights).  lf_set_lights_ex is lf_set_lights with a kind per light:
 *   kind[k] == LF_LIGHT_DIRECTIONAL  vec[3 k ..] is the direction, validated and stored exactly as lf_set_lights does;
 *   kind[k] == LF_LIGHT_POINT        vec[3 k ..] is the light's POSITION in lens millimetres, the prescription's coordinates:
 *                                    front vertex at z = 0, the scene at z < 0.
 * angular_radius[k] is the lobe's angular radius as seen from EVERY exit point (one 1 / (1 - cos) per light, as ever).
 * With r_f = sqrt(h0^2 + sag(h0)^2), the largest distance from the front vertex to a point of the front element's clear
 * aperture (h0 its semi-aperture), a point light must be finite and have z <= -2 r_f and |L| >= 4 r_f: otherwise
 * LF_ERR_INVALID with a message that names the limit (before lf_set_lens: LF_ERR_STATE, the limits are the lens's).  The
 * call replaces ALL lights; a refusal leaves the previous ones installed.  lf_set_lights and lf_set_sun ARE lf_set_lights_ex
 * with every kind 0: the same state, the same kernels as before this call existed.
 * The per-ray contract (float32, every multiply-add an explicit fmaf): a ray has left the front element at
 * (px, py, z = front_zv + hz) along d; for a point light at L
 *     s = (Lx - px, Ly - py, Lz - z)   three float subtractions,     ss = |s|^2,
 *     q = the sun's lobe expression on (d, s, ss) -- |d x s|^2 / (|d|^2 ss + sqrt(|d|^2 ss) d.s) / (1 - cos alpha) -- with
 *         the correctly rounded root and division,
 *     inside iff d.s > 0 and q < 1,     contrib = (wn / wd) (1 - q)^2 as ever.
 * Everything else of the multi-light contract above holds with lights of mixed kinds: one fixed-point value per (ray,
 * light, channel); the frame of K lights is the sum of the K single-light frames, bit for bit; rays_hit_light counts
 * (ray, light) contributions; the range contract takes the sum of the radiances.  A point light has no distance falloff
 * (neither has the scene term's: the reference's PointLight::sample_L).
 * THE CULL TABLE takes a point light as the direction unit(L) from the front vertex, its radius widened by
 * r_f / (|L| - r_f): for P on the front cap |unit(L - P) - unit(L)| <= |P| / min(|L - P|, |L|).  The
 * audit decides "lit" by the exact per-ray test above.  A light so close that the widened table starts more than the
 * launch's limit takes the path tree (lf_get_cull_reason: LF_CULL_TABLE_TOO_FULL), as a very wide sun does.
 * KERNELS: a context with a point light -- also as its only light -- launches the kVarNear variants (march variant bits
 * 4 | 32, lf_get_ghost_occlusion's *march_variant); a context without one launches exactly what it launched before.
 * lf_set_lens KEEPS the installed lights; if the new front element is too close to an installed point light,
 * lf_trace_ghosts (and lf_cull_prepare, lf_ghost_ray_light_factors) refuse with LF_ERR_STATE until the lights or the lens
 * change.  GHOST OCCLUSION together with a point light needs shadow rays that end at the light:
 * lf_set_ghost_occlusion_reach(LF_OCCLUSION_REACH_LIGHT) below.  Under the default, LF_OCCLUSION_REACH_SKY, lf_trace_ghosts
 * refuses the combination with LF_ERR_STATE and names that call: a ray that runs on to the sky would let a wall BEHIND the
 * lamp hide it.
 * lf_get_lights reports a point light as the unit vector from the front vertex to its position; lf_get_lights_ex its kind
 * and its position as stored (any pointer may be NULL; arrays of LF_MAX_LIGHTS lights).
 * COST, as measured (the bench frame, 1080p x 256 spp, table rebuilt and audited inside every frame; profiles/near_light_cost.json):
 * the sun 34.96 ms, through the parent commit's library 35.01 (the kernels are the parent's); the sun replaced by a lamp of the
 * same 0.05 rad in the same direction 40.44 ms at 1 m, 46.36 ms at 300 mm (the table starts 8.2 / 9.9 % against the sun's 7.7 %),
 * 121.19 ms at 100 mm (16.5 %: the path tree); {sun, lamp at 1 m} 56.12 ms against 53.55 for two suns, four mixed lights 92.75
 * against 87.43 for four suns. */
typedef enum { LF_LIGHT_DIRECTIONAL = 0, LF_LIGHT_POINT = 1 } lf_light_kind;
lf_status lf_set_lights_ex(lf_ctx* ctx, int n_lights, const int* kind, const float* vec, const float* radiance,
                           const float* angular_radius);
lf_status lf_get_lights_ex(lf_ctx* ctx, int* n_lights, int* kind, float* vec, float* radiance, float* angular_radius);
/* Host arithmetic, no device: one light as lf_set_lights_ex validates it against a front element of the given radius
 * (0: flat) and semi-aperture -- LF_OK, or LF_ERR_INVALID with the refusal's text in message (may be NULL). */
lf_status lf_validate_light(int kind, const float vec[3], const float radiance[3], float angular_radius, float front_radius,
                            float front_semi_aperture, char* message, size_t message_size);
/* Host arithmetic, no device: the lobe factor of ONE exit ray {origin xyz in lens millimetres (z absolute), direction xyz}
 * for ONE light (vec, angular_radius as lf_set_lights_ex takes them): *q, and *inside = the ray contributes (either may
 * be NULL).  For a point light this is the definition the kernels call, bit for bit; for a directional light the device
 * takes the root with v_sqrt_f32 (1 ulp) where the host's is correctly rounded: q agrees to 2 ulp. */
lf_status lf_light_lobe_factor(int kind, const float vec[3], float angular_radius, const float ray[6], float* q, int* inside);
/* ... and on the device, for the lights INSTALLED: out[i n_lights + k] = (1 - q_k)^2 where exit ray i lies inside light k,
 * 0 elsewhere -- the lit epilogue's own test and factor, without a weight (as lf_ghost_ray_visibility is to occlusion).
 * Needs a lens and a light. */
lf_status lf_ghost_ray_light_factors(lf_ctx* ctx, size_t n, const float* rays, float* out);
/* GHOST OCCLUSION: hide a light's lens ghosts behind the scene.  Off by default (on = 0); a context with occlusion off
 * launches exactly the kernels it launched before this call existed.  on = 1 needs world_per_mm > 0 and finite (scene
 * units per lens millimetre, lf_set_lens_camera's), else LF_ERR_INVALID and the previous state stays.  A setting of the
 * context: it survives lf_set_lens, lf_set_lights, lf_focus_lens and lf_set_frame.  The contract, occlusion on:
 *   - lf_trace_ghosts needs a lens, lf_set_camera and a scene of at least one primitive (lf_set_scene / lf_load_collada),
 *     else LF_ERR_STATE with a message that names what is missing; a later lf_set_scene / lf_set_camera is picked up by
 *     the next launch;
 *   - everything before the lit epilogue is unchanged: the samples, the events and the fates, the cull table with its
 *     cache, resolve and audit, the weighted re-march, lf_get_march_fix_bits;
 *   - per (ray, light k) contrib_k is computed exactly as without occlusion and added, as the same u64 values, if and
 *     only if the ray's SHADOW RAY finds no primitive: the ray's own exit point on the front element along its own exit
 *     direction, from min_t = 0 to max_t = +inf (the camera's clip planes do not apply, as they do not clip a
 *     directional light's shadow ray in the scene term).  A ray walks once for all its lights: the ray is the same;
 *   - the mapping is the lens camera's, in double: with the re-marched ray's (px, py, z) in lens millimetres (z absolute
 *     in the prescription's coordinates, the front vertex at 0) and z_ref the paraxial entrance pupil's z at the
 *     reference wavelength (what lf_get_lens_camera reports), oc = (px wpm, py wpm, (z - z_ref) wpm), origin = pos +
 *     c2w oc, direction = c2w unit(dx, dy, dz) -- in a lens-camera frame a ghost's shadow ray and the scene image agree;
 *   - the primitive tests and the tree are the scene term's (the reference's double-precision sphere / triangle tests);
 *   - a frame of K lights stays the sum of the K single-light frames under the same occlusion setting, bit for bit;
 *   - lf_counters::rays_hit_light counts what was added; lf_get_ghost_occlusion_stats = {shadow tests made = (ray,
 *     light) pairs with contrib_k > 0, of those blocked}, reset by lf_reset_counters; every other counter,
 *     lf_get_executed_events, lf_get_cull_table and lf_get_cull_audit are those of the same launch with occlusion off.
 * Occluders are opaque.  The starburst, the falloff and the paraxial ghost quads of an occluded light are not this call's:
 * lf_set_flare_occlusion (below) hides them.
 * lf_get_ghost_occlusion (any pointer may be NULL): the setting, and *march_variant = the kernel variant the next launch
 * takes (bit 4, value 16, set exactly when occlusion is on). */
lf_status lf_set_ghost_occlusion(lf_ctx* ctx, int on, double world_per_mm);
lf_status lf_get_ghost_occlusion(lf_ctx* ctx, int* on, double* world_per_mm, int* march_variant);
lf_status lf_get_ghost_occlusion_stats(lf_ctx* ctx, uint64_t out[2]);
/* "would this exit ray see the sky": n rays, each {origin xyz in lens millimetres, direction xyz} (6 floats), through the
 * same mapping and the same any-hit walk as the march's shadow rays, on the state installed; visible[i] = 1 if ray i
 * meets no primitive, else 0.  Preconditions as lf_trace_ghosts' with occlusion on (which must be on: it carries
 * world_per_mm), except that no light is needed. */
lf_status lf_ghost_ray_visibility(lf_ctx* ctx, size_t n, const float* rays, unsigned char* visible);
/* FLARE OCCLUSION: hide the starburst, the irradiance falloff and the paraxial ghost quads of a light the scene blocks.
 * Off by default (on = 0: the other arguments are not looked at); a context with it off launches exactly the kernels it
 * launched before this call existed, with the same arguments.  on = 1 needs rays_per_light R a multiple of 64 in
 * [64, 4096], angular_radius finite in [0, 0.5] (radians: the light's disc), origin one of lf_flare_origin and, under
 * LF_FLARE_ORIGIN_FRONT_ELEMENT, world_per_mm > 0 and finite (ignored under LF_FLARE_ORIGIN_CAMERA) -- else
 * LF_ERR_INVALID and the previous state stays.  A setting of the context: it survives lf_set_frame, lf_set_lens,
 * lf_set_camera, lf_find_sun_pos and lf_set_flares.  The contract, while on:
 *   - SAMPLES (lf_flare_shadow_samples is the definition; host, double, narrowed to float): for r = 0 .. R-1,
 *     u0 = (r + 0.5) / R, u1, u2, u3 = the van der Corput radical inverse of r in base 2, 3, 5;
 *     (a, b) = sqrt(u0) (cos 2 pi u1, sin 2 pi u1), a point of the unit aperture disc; (c, d) = sqrt(u2) (cos 2 pi u3,
 *     sin 2 pi u3), a point of the light's unit disc.  The table is built once per setting and stays on the device;
 *   - RAYS of flare k, stored at screen position (nx, ny) as lf_get_flares returns it (lf_flare_shadow_rays is the definition,
 *     the kernel runs the same text: double, + - * / sqrt only, unfused, then narrowed to float): edge_x = tan(0.5 hfov
 *     pi / 180), edge_y likewise (host; lf_find_sun_pos' expression inverted); s = unit((2 nx - 1) edge_x, (2 ny - 1) edge_y,
 *     -1) -- x right, y up, the scene at -z, in camera space and in lens space alike; e1 = unit(s.z, 0, -s.x), e2 = s x e1;
 *     direction = s + tan(angular_radius) (c e1 + d e2), not normalised; origin = (h0 a, h0 b, 0) in lens millimetres
 *     under LF_FLARE_ORIGIN_FRONT_ELEMENT (h0 the front interface's semi-aperture: the front vertex plane; needs a lens),
 *     (0, 0, 0) under LF_FLARE_ORIGIN_CAMERA: the camera position itself (oc = 0: no z_ref, no lens);
 *   - DECISION: each float ray goes through the ghost march's shadow-ray mapping and any-hit walk unchanged (the contract
 *     of lf_set_ghost_occlusion above: the lens camera's mapping in double, min_t = 0, max_t = +inf, the scene term's
 *     double-precision primitive tests).  visible_rays[k] = the rays that meet nothing, visibility[k] = visible_rays[k] / R;
 *   - a flare is a light at infinity (what lf_find_sun_pos keeps); a lamp handed in through lf_set_flares is occluded as a
 *     sun in its direction;
 *   - EFFECT: lf_render_flare_layer (starburst, spectral starburst, falloff, buffer 2) and lf_irradiance_falloff read an
 *     effective flare record, radiance[k][c] * visibility[k] (one double multiply); lf_generate_ghost_buffer multiplies
 *     each quad's colour by the visibility of flare n_flares - 1, the one that supplied axis_ray (no flare: 1).
 *     lf_get_flares keeps returning the radiance as installed.  So with every visibility 1 every buffer is the one
 *     rendered with the setting off, bit for bit (MT19937 parity mode included: no random number is drawn), and
 *     otherwise buffers 0 and 2 are those of the setting off after lf_set_flares(origins, radiance[k] * visibility[k], ...);
 *   - visibility is computed on the context's stream from the state installed when a consuming call is made --
 *     lf_render_flare_layer, lf_generate_ghost_buffer, lf_irradiance_falloff, lf_get_flare_visibility -- at every such call
 *     (nothing is cached: two short launches, "flare_visibility" of lf_timing_get).  It then needs a camera and a scene of
 *     at least one primitive and, under LF_FLARE_ORIGIN_FRONT_ELEMENT, a lens: else LF_ERR_STATE, the message names what
 *     is missing.  With no flare in the frame nothing is launched;
 *   - every rank of a multi-GPU job computes the same integers; nothing is exchanged.
 * Out of scope: shadow rays that end at a lamp.  Measured (profiles/flare_occlusion_cost.json: one MI355X, the 1080p
 * reference flare frame of two consuming calls, 40 frames per leg): the two launches take 0.012 - 0.020 ms per consuming
 * call for 256 ... 32 768 rays that pass over the scene, 0.077 ms when they descend a tree of 50 801 triangles; the frame
 * 0.33 ms against 0.27 with one flare, 0.67 against 0.61 with eight; off, 0.272 against the parent library's 0.271 (DESIGN.md
 * section 7).
 * lf_get_flare_occlusion: any pointer may be NULL.  lf_get_flare_visibility (LF_ERR_STATE while the setting is off):
 * *n_flares and the first n_flares entries of visibility / visible_rays (room for LF_MAX_FLARES; either may be NULL). */
typedef enum { LF_FLARE_ORIGIN_CAMERA = 0, LF_FLARE_ORIGIN_FRONT_ELEMENT = 1 } lf_flare_origin;
lf_status lf_set_flare_occlusion(lf_ctx* ctx, int on, int rays_per_light, float angular_radius, int origin, double world_per_mm);
lf_status lf_get_flare_occlusion(lf_ctx* ctx, int* on, int* rays_per_light, float* angular_radius, int* origin, double* world_per_mm);
lf_status lf_get_flare_visibility(lf_ctx* ctx, int* n_flares, double* visibility, uint64_t* visible_rays);
/* Host arithmetic, no device -- the definitions the kernel reproduces bit for bit.  out: 4 floats per ray, a b c d;
 * rays: 6 floats per ray, origin xyz in lens millimetres and direction xyz, as lf_ghost_ray_visibility takes them.
 * LF_ERR_INVALID: a NULL pointer, R as above, angular_radius as above, a bad origin, a field of view outside (0, 180),
 * front_semi_aperture not > 0 under LF_FLARE_ORIGIN_FRONT_ELEMENT. */
lf_status lf_flare_shadow_samples(int rays_per_light, float* out);
lf_status lf_flare_shadow_rays(int rays_per_light, const double flare_origin[2], double hfov_deg, double vfov_deg,
                               float angular_radius, int origin, float front_semi_aperture, float* rays);
/* THE REACH OF A SHADOW RAY: ghost occlusion for point lights.  "Does this ray see the sky" is the wrong question for a lamp
 * in the room: a wall behind the lamp must not hide it, a wall between the lens and the lamp must.  A setting of the context
 * beside lf_set_ghost_occlusion, and separate from it:
 *   LF_OCCLUSION_REACH_SKY (default)  every shadow ray runs to max_t = +inf: the contract above, to the letter -- and with a
 *                                     point light installed and occlusion on, lf_trace_ghosts refuses with LF_ERR_STATE;
 *   LF_OCCLUSION_REACH_LIGHT          the shadow ray of light k runs from min_t = 0 to max_t = reach_k; with occlusion on and
 *                                     a point light installed lf_trace_ghosts launches (the kVarNear | kVarOccl kernels:
 *                                     *march_variant = 4 | 16 | 32 plus the coat / filter / stack bits).
 * Any other value: LF_ERR_INVALID, the previous state stays.  The setting survives lf_set_lens, lf_set_lights*, lf_focus_lens,
 * lf_set_frame and switching lf_set_ghost_occlusion off and on; it has no effect while occlusion is off, and none without a
 * point light: under LF_OCCLUSION_REACH_LIGHT directional lights alone launch the variant (4 | 16 | ...) and render the
 * frames they render under LF_OCCLUSION_REACH_SKY, bit for bit.
 * The contract per (ray, light k) is the occlusion contract above with ONE change, the end of the shadow ray:
 *   - a directional light: reach_k = +inf;
 *   - a point light stored at L (float32 lens millimetres, as lf_get_lights_ex reports it), the re-marched ray's exit point
 *     (px, py, z) (z absolute) and direction d, all in double and in this order:
 *         s = ((double)Lx - px, (double)Ly - py, (double)Lz - z),     dc = unit(d)  (d times 1 / |d|, the shadow ray's own dc),
 *         t = wpm ((s.x dc.x + s.y dc.y) + s.z dc.z),                 reach_k = t > 0 ? t : 0
 *     -- the ray parameter, in world units, of the point of the ray nearest the lamp (c2w is a rotation).  No epsilon is
 *     taken off either end.  A lamp many kilometres away behaves as the sun in its direction does;
 *   - origin and direction of the shadow ray are unchanged; contrib_k is computed as ever and added iff the any-hit walk
 *     over [0, reach_k], with the scene term's double-precision primitive tests, finds nothing;
 *   - the decision for light k does not depend on the other lights: a frame of K lights of mixed kinds is the sum of the K
 *     single-light frames under the same settings, bit for bit; the stats, rays_hit_light and every other counter keep
 *     their meaning.
 * A primitive that encloses the lamp blocks it, as it blocks the scene term's shadow rays to a PointLight. */
typedef enum { LF_OCCLUSION_REACH_SKY = 0, LF_OCCLUSION_REACH_LIGHT = 1 } lf_occlusion_reach;
lf_status lf_set_ghost_occlusion_reach(lf_ctx* ctx, int reach);
lf_status lf_get_ghost_occlusion_reach(lf_ctx* ctx, int* reach);
/* Host arithmetic, no device: reach_k of ONE exit ray {origin xyz in lens millimetres (z absolute), direction xyz} for ONE
 * light (kind, vec as lf_set_lights_ex takes them): +inf for LF_LIGHT_DIRECTIONAL, the definition above -- the one the
 * kernels call, bit for bit -- for LF_LIGHT_POINT.  world_per_mm not finite or <= 0, or a non-finite input: LF_ERR_INVALID. */
lf_status lf_ghost_shadow_reach(int kind, const float vec[3], const float ray[6], double world_per_mm, double* reach);
/* ... and on the device, for the state INSTALLED: visible[i n_lights + k] = 1 iff the shadow ray of exit ray i finds nothing
 * over [0, reach_k] -- the epilogue's own mapping, reach and walk, whether or not the ray lies in lobe k.  Preconditions as
 * lf_ghost_ray_visibility's, plus a lens and at least one light; with a point light installed under
 * LF_OCCLUSION_REACH_SKY it refuses as the launch does. */
lf_status lf_ghost_ray_light_visibility(lf_ctx* ctx, size_t n, const float* rays, unsigned char* visible);
/* Sun hand-over from the scene to the march: turn in-frame flare `flare` of lf_find_sun_pos /
 * lf_set_flares (normalised screen position flare_origins[flare], radiance flare_radiance[flare];
 * src/pathtracer/pathtracer.cpp:32-64, camera.cpp:245-273) into the lens-space light of
 * lf_set_sun, so that the geometric ghosts and the starburst agree about where the sun is: the
 * direction is the one a lens of focal length efl_mm images at that sensor point,
 *   (  (nx - 1/2) sensor_w / efl,  (ny - 1/2) sensor_w (H/W) / efl,  -1  )  normalised.
 * efl_mm <= 0 takes the paraxial image scale of the prescription at the middle wavelength: where the chief
 * ray of a distant point lands on the sensor per unit field angle -- the focal length (lf_paraxial_efl) while
 * the sensor sits in the focal plane, as in the shipped files, and what a sensor moved by lf_focus_lens really
 * sees otherwise.  Needs lf_set_frame, lf_set_lens and a flare state.  No reference counterpart (the
 * reference's ghosts take only `angle_to_sun`, pathtracer.cpp:50, :735-762). */
lf_status lf_set_sun_from_flares(lf_ctx* ctx, int flare, double efl_mm, float angular_radius);
/* ... and EVERY in-frame flare of the flare state as the lights of lf_set_lights, each by lf_set_sun_from_flares'
 * mapping, all with the same angular radius: every in-frame DirectionalLight gets its lens ghosts, as it gets its
 * starburst.  *n_taken (may be NULL) = the lights installed.  With one flare the installed state is exactly
 * lf_set_sun_from_flares(ctx, 0, ...)'s.  More in-frame lights than LF_MAX_LIGHTS: LF_ERR_INVALID (the message
 * names the limit; nothing is installed) -- such a host composes launches itself: lf_set_sun_from_flares /
 * lf_set_lights per group of lights under lf_set_ghost_accumulate. */
lf_status lf_set_lights_from_flares(lf_ctx* ctx, double efl_mm, float angular_radius, int* n_taken);
/* ... and the scene's POINT lights with them: first the in-frame flares of the flare state, exactly as
 * lf_set_lights_from_flares takes them (no flare state, or no flare in the frame: none), then every PointLight of the
 * installed scene lights (type 1 of lf_set_scene_lights / lf_set_scene) as an LF_LIGHT_POINT of lf_set_lights_ex: its world
 * position through the INVERSE of the lens camera's mapping, in double, then narrowed,
 *     p_lens = c2w^T (p_world - pos) / world_per_mm + (0, 0, z_ref),
 * z_ref the paraxial entrance pupil's z (what lf_get_lens_camera reports), its rgb as the lobe's radiance (no distance
 * falloff: the reference's point light has none either), all with the same angular radius.  A point light behind
 * lf_set_lights_ex's distance limits (behind the camera, or too close to the front element) is skipped and not counted.
 * *n_directional / *n_point (may be NULL) = the lights installed.  More than LF_MAX_LIGHTS in all: LF_ERR_INVALID, nothing is
 * installed; no light at all: LF_ERR_INVALID.  Needs lf_set_frame, lf_set_lens and lf_set_camera. */
lf_status lf_set_lights_from_scene(lf_ctx* ctx, double efl_mm, float angular_radius, double world_per_mm, int* n_directional,
                                   int* n_point);
/* AREA LIGHTS (rectangular emitters): the reference's AreaLight (scene/light.cpp:76-94), a one-sided rectangle -- the lamp of
 * its Cornell-box scenes -- as a light of the march.  LF_LIGHT_AREA is the third lf_light_kind.  The three-float calls above
 * (lf_set_lights_ex, lf_validate_light, lf_light_lobe_factor, lf_ghost_shadow_reach) keep refusing it: three floats cannot
 * describe a rectangle.  The calls below take LF_LIGHT_GEOM_FLOATS = 12 floats per light:
 *   kinds 0 and 1     floats 0..2 are the vec of lf_set_lights_ex, the rest are ignored and stored as 0;
 *   LF_LIGHT_AREA     floats 0..2 the centre C, 3..5 the direction it emits towards, 6..8 dim_x (e1) and 9..11 dim_y (e2), both
 *                     FULL edge vectors, all in lens millimetres (front vertex at z = 0, the scene at z < 0): the rectangle is
 *                     C + u e1 + v e2, u, v in [-1/2, 1/2], as the reference samples it.  The direction is stored normalised
 *                     (in double, then narrowed) and need not be the rectangle's normal (the reference does not ask for that
 *                     either); angular_radius[k] is ignored and reported back as 0.
 * lf_set_lights_geom replaces ALL lights; a refusal leaves the previous ones installed; lf_set_lights_ex IS lf_set_lights_geom
 * with only the first three floats filled.  An area light must have all 12 floats and its radiance finite, the radiance
 * >= 0, a direction that is not zero, |e1 x e2| >= 1e-6 |e1| |e2|, and each of its four corners C +- e1/2 +- e2/2 within the
 * point light's limits, z <= -2 r_f and |corner| >= 4 r_f: otherwise LF_ERR_INVALID with a message that names the limit
 * (before lf_set_lens: LF_ERR_STATE).  lf_set_lens keeps the installed lights; a front element that has come too close to an
 * installed rectangle makes the launch refuse with LF_ERR_STATE, as for a point light.  lf_get_lights_ex reports an area
 * light as kind 2 with vec = its centre, lf_get_lights the unit vector from the front vertex to the centre.
 * The per-ray contract (float32, every multiply-add an explicit fmaf, dot products nested fmaf(x, x', fmaf(y, y', z z'))): a
 * ray has left the front element at P = (px, py, front_zv + hz) along d;
 *     s = P - C          p = d x e2          det = e1 . p          a = s . p
 *     qv = s x e1        b = d . qv          tn = e2 . qv
 *     inside iff det != 0 and 2 |a| <= |det| and 2 |b| <= |det| and tn sign(det) > 0 and d . dir < 0
 *     contrib = wn / wd                      (factor 1: an area light has no lobe, radiance is constant along a ray)
 * -- the ray-parallelogram test without a division or a root; d . dir < 0 is the reference's cosTheta < 0.  Everything else
 * of the multi-light contract holds: one fixed-point value per (ray, light, channel), a frame of K lights of mixed kinds
 * is the sum of the K single-light frames bit for bit, rays_hit_light counts (ray, light) contributions, and the range
 * contract (lf_get_march_fix_bits) is unchanged, the factor being <= 1.  An in-focus ghost of a rectangle is a sharp quad.
 * THE CULL TABLE takes an area light as the cone lf_area_light_cull_cone returns: dir = unit(C) from the front vertex and
 * rho = max over the four corners of |unit(corner) - unit(C)| plus r_f / (dmin - r_f), dmin the distance from the front
 * vertex to the nearest point of the rectangle, with the point light's slack.  The audit keeps the
 * exact per-ray test.  A large or near rectangle fills the table and takes the path tree (LF_CULL_TABLE_TOO_FULL).
 * KERNELS: a context with an area light -- also as its only light -- launches the kVarArea variants (*march_variant =
 * 4 | 32 | 64 plus the coat, filter, stack and occlusion bits), which handle all three kinds; a context without one launches
 * exactly what it launched before.
 * OCCLUSION: under LF_OCCLUSION_REACH_SKY the launch refuses an area light as it refuses a point light.  Under
 * LF_OCCLUSION_REACH_LIGHT the shadow ray of an area light ends just before the rectangle: the expressions above in double
 * on the float-stored geometry and the ray, t = tn / det, reach = max(0, wpm t |d| - (double)0.00001f) -- the reference's
 * EPS_F, as its shadow rays to sampled lights take it off (pathtracer.cpp:195): an emissive mesh lying in the light's
 * plane, the Cornell lamp, does not shadow its own light.  Two limits: a mesh nearer the plane than EPS_F times the
 * obliquity is the host's to keep clear; and with the lens camera on an emissive mesh is already imaged by the scene term,
 * so such a host drops the primary path (lf_set_ghost_pairs include_primary = 0) or the lamp's direct image is added twice.
 * COST, as measured (the bench frame, 1080p x 256 spp, table rebuilt and audited inside every frame; profiles/area_light_cost.json):
 * the sun 35.01 ms, through the parent commit's library 34.92 (the kernels are the parent's); a 40 x 24 mm rectangle at 300 mm
 * 56.02 ms against 46.20 for the point light (0.05 rad) at its centre (the table starts 11.4 % against 9.9 %); a 500 x 500 mm panel
 * at 3 m 73.15 ms against 38.94 (11.3 % against 7.9 %; 1029 M against 306 M lit rays).  Under occlusion with
 * LF_OCCLUSION_REACH_LIGHT behind a wall over half the beam: 314.9 ms against 256.7, and 422.4 against 205.3.  The library's build
 * takes 7 min 05 s instead of 4 min 47 s (183 more kernels). */
#define LF_LIGHT_AREA 2             /* lf_light_kind's third value, known to the twelve-float calls alone */
#define LF_LIGHT_GEOM_FLOATS 12
lf_status lf_set_lights_geom(lf_ctx* ctx, int n_lights, const int* kind, const float* geom, const float* radiance,
                             const float* angular_radius);
/* (any pointer may be NULL; arrays of LF_MAX_LIGHTS lights; a directional light's floats 0..2 are its direction as stored) */
lf_status lf_get_lights_geom(lf_ctx* ctx, int* n_lights, int* kind, float* geom, float* radiance, float* angular_radius);
/* Host arithmetic, no device: one light as lf_set_lights_geom validates it (lf_validate_light's arguments otherwise). */
lf_status lf_validate_light_geom(int kind, const float* geom, const float radiance[3], float angular_radius, float front_radius,
                                 float front_semi_aperture, char* message, size_t message_size);
/* Host arithmetic, no device: ONE exit ray {origin xyz (z absolute), direction xyz} and ONE light.  *factor = what contrib is
 * multiplied by, (1 - q)^2 or, for an area light, 1, where the ray contributes and 0 elsewhere; *inside; *t = for an area
 * light the ray parameter of its plane, tn / det in double (P + t d; +inf for the other kinds).  Any of the three may be
 * NULL.  An area light's is the definition the kernels call, bit for bit. */
lf_status lf_light_geom_factor(int kind, const float* geom, float angular_radius, const float ray[6], float* factor, int* inside,
                               double* t);
/* ... and the pre-test that selects lanes for an area light's exact test, any superset of it: the rectangle's bounding
 * sphere seen from the exit point (host arithmetic, the kernels' own definition) */
lf_status lf_area_light_pretest(const float* geom, const float ray[6], int* admitted);
/* Host arithmetic, no device: lf_ghost_shadow_reach for the twelve-float kinds (kinds 0 and 1: the same values). */
lf_status lf_ghost_shadow_reach_geom(int kind, const float* geom, const float ray[6], double world_per_mm, double* reach);
/* Host arithmetic, no device: what the cull table takes an area light as, for a front element of the given radius (0:
 * flat) and semi-aperture.  A rectangle lf_validate_light_geom refuses: LF_ERR_INVALID. */
lf_status lf_area_light_cull_cone(const float* geom, float front_radius, float front_semi_aperture, float dir[3], float* rho);
/* lf_set_lights_from_scene plus every AreaLight of the installed scene lights (type 3): position as a point light's, direction
 * as c2w^T v, dim_x and dim_y as c2w^T v / world_per_mm, in double, then narrowed; its rgb is the radiance.  A rectangle that
 * fails validation is skipped and not counted; more than LF_MAX_LIGHTS in all: LF_ERR_INVALID, nothing is installed. */
lf_status lf_set_lights_from_scene_ex(lf_ctx* ctx, double efl_mm, float angular_radius, double world_per_mm, int* n_directional,
                                      int* n_point, int* n_area);
/* Paraxial effective focal length of a prescription at one wavelength (host arithmetic, no
 * device): the system matrix from the reference's own T / R operators (pathtracer.cpp:527-533);
 * ior_row = the n indices of that wavelength (media BEHIND each interface).  Arguments as
 * lf_set_lens. */
lf_status lf_paraxial_efl(int n_surfaces, int stop_index, const float* radius, const float* thickness,
                          const float* ior_row, double* efl_mm);
/* Paraxial image scale of a prescription AS ITS SENSOR SITS (host arithmetic, no device): the height at
 * which the chief ray of a distant point lands on the sensor per unit field angle -- what
 * lf_set_sun_from_flares(efl_mm <= 0) divides by.  Equal to lf_paraxial_efl when the last thickness puts the
 * sensor in the paraxial focal plane; a file focused elsewhere, or a sensor moved by lf_focus_lens, differs. */
lf_status lf_paraxial_image_scale(int n_surfaces, int stop_index, const float* radius, const float* thickness,
                                  const float* ior_row, double* scale_mm);
/* ghost pairs to enumerate: pairs = n x {i, j} interface indices (i < j, neither the stop);
 * i = j = -1 is the primary (no reflection) path.  n = 0 / NULL = all glass pairs. */
lf_status lf_set_ghost_pairs(lf_ctx* ctx, const int* pairs, int n_pairs, int include_primary);
/* Part of the sampling specification of lf_trace_ghosts (no reference
 * counterpart): each pupil stratum is split into 2^bits x 2^bits sub-cells and all 64 pixels of an
 * 8x8 sensor tile aim sample s at the same, randomly drawn sub-cell (coherent fate at the aperture
 * mask).  bits = 0 draws every pixel's pupil point independently inside its stratum; every value
 * is an unbiased estimator of the same image (tests/test_gpu_march_f64.py).  0..8; default 6 (64 x 64
 * sub-cells) since round 4 -- rounds 1-3 shipped 2 (4 x 4): a frame of those rounds is reproduced by
 * lf_set_pupil_subcells(2) + lf_set_tile_stride(1). */
lf_status lf_set_pupil_subcells(lf_ctx* ctx, int bits);
/* Part of the sampling specification (no reference counterpart): the disc every sensor sample aims its
 * pupil point at -- radius and axial position z in the prescription's coordinates (z = 0 at the first
 * vertex, growing towards the sensor).  Default (radius <= 0): the rear element's clear aperture at its
 * vertex plane, which is valid for EVERY path but wastes the samples that miss the exit pupil.  A
 * smaller disc is an unbiased estimator only for paths whose first crossing of the stop precedes their
 * first reflection (the primary path and the pairs (i, j) with i in front of the stop): the start
 * weight is the disc's solid angle, so nothing else changes.  Pairs with both mirrors behind the stop
 * must keep the default.  lf_aim_at_exit_pupil sets the disc to the paraxial image of the stop's open
 * part (the circle around the mask's non-zero texels) through the rear group, times `margin` (> 1
 * leaves room for pupil aberration off the axis).  lf_paraxial_exit_pupil: that image for a
 * prescription and one wavelength (host arithmetic with the reference's T / R operators,
 * pathtracer.cpp:527-533): its z and its lateral magnification. */
lf_status lf_set_pupil_target(lf_ctx* ctx, float radius_mm, float z_mm);
lf_status lf_get_pupil_target(lf_ctx* ctx, float* radius_mm, float* z_mm, float* z_sensor_mm);
lf_status lf_aim_at_exit_pupil(lf_ctx* ctx, float margin);
lf_status lf_paraxial_exit_pupil(int n_surfaces, int stop_index, const float* radius, const float* thickness,
                                 const float* ior_row, double* z_mm, double* magnification);
/* on: lf_trace_ghosts ADDS its pixels to ghost_buffer instead of replacing them (a frame composed of
 * launches with different pair sets / pupil targets).  Default off. */
lf_status lf_set_ghost_accumulate(lf_ctx* ctx, int on);
/* Which 64 pixels a wave of the march takes (part of the sampling specification, like the pupil
 * sub-cells: it decides which pixels share a sub-cell draw): 8 rows x 8 columns that are `stride` (1, 2, 4
 * or 8) apart; `stride` such waves interleave inside a block of 8 * stride columns.  stride 1 (the default
 * of rounds 1-3) = an 8 x 8 block of adjacent pixels, whose shared sub-cell correlates the noise of
 * neighbouring pixels (variance of an 8 x 8 tile mean = 38x independent pixels at 4 x 4 sub-cells);
 * stride 8 (THE DEFAULT since round 4) spreads a wave's pixels over 64 columns, so that the correlated noise
 * lands on pixels 8 apart (7.4x with the 64 x 64 sub-cells that are the default beside it).  Per-pixel
 * expectation and variance do not depend on it; the tile rows (multi-GPU deal) stay 8 rows.  The same key
 * gives DIFFERENT pixels under a different stride / sub-cell setting: a host or an oracle that wants the
 * frames of rounds 1-3 calls lf_set_tile_stride(1) + lf_set_pupil_subcells(2). */
lf_status lf_set_tile_stride(lf_ctx* ctx, int stride);
/* march `spp` sensor samples per pixel of the band through every selected pair and wavelength and
 * accumulate into ghost_buffer (replacing its content).  key seeds the counter RNG. */
lf_status lf_trace_ghosts(lf_ctx* ctx, int spp, uint64_t key);
/* PATH CULLING (round 5; no reference counterpart -- the reference enumerates 13 fixed pairs per channel and
 * draws each as one quad, pathtracer.cpp:735-762, :452-508).  lf_trace_ghosts does not start a path where it
 * cannot carry light: a pre-pass bounds, for every block of 64 x 64 sensor pixels (128 x 128 where that is still
 * <= 1.25 mm on the sensor and the launch has few samples: 4K below 256 spp x 3 wavelengths; 32 or 16 where 64 pixels
 * are more than 1.8 mm: frames narrower than 1280 pixels on 36 mm), every cell of the pupil square and every selected
 * path, where the rays of that 4-D box can go -- on each diaphragm of the path and in direction space at the exit --
 * and the march starts only the paths whose box may end inside the sun's lobe.  A path that is not started adds
 * exactly 0 IF the bound is right, and then ghost_buffer is the buffer of the full enumeration bit for bit.
 * WHAT STANDS BEHIND THE BOUND: it is a second-order estimate from 15 marched rays per box (DESIGN.md section 5 states the
 * assumption: the third order of the bundle's map is small against the measured second order away from the edges
 * where a ray ends, and boxes touching such an edge are never dropped), checked against the full enumeration on whole
 * frames and on 39 000 random frames of three design families (double Gauss, Cooke triplet, their 8-wavelength forms:
 * scaled 0.5 .. 2, bent 8 %, refocused, suns of 0.17 .. 17 degrees over the field, blocks of 0.6 .. 1.8 mm) -- and, on
 * EVERY launch, audited: lf_set_cull_audit below.  A host that wants the enumeration itself: mode 0.
 * lf_counters / lf_get_executed_events count the rays that were started.
 *   mode 1 (default): on; the table is reused while lens, pairs, sun, frame, pupil disc, mask and sample
 *                     count are unchanged.   2: on, rebuilt at every lf_trace_ghosts.
 *   What a rebuild recomputes: only what depends on the sun -- each surviving box's last test, its exit footprint against
 *   the lobe, in one pass over a tree the context keeps.  What it does NOT recompute: the marches of the boxes' 15 rays and
 *   every decision before that test (apertures, the mask's grid, lost samples), which depend on the lens, the frame, the
 *   blocks, the mask, the pairs and the rank's share alone: built by the first launch that sees them, rebuilt when one of
 *   them changes (a host that changes them at every launch pays no build per frame: after a tree that was never reused, the
 *   next is built only for inputs seen on two launches running), freed by lf_destroy.  The tree is device memory the context
 *   holds between launches: 4 bytes per (path, own block, cell) box of every level + 48 bytes per undecided box, under a
 *   budget of 8 GiB (the 1080p 46-path frame: DESIGN.md section 5); a tree beyond the budget is not kept and every rebuild
 *   marches its boxes as before.  The tables are the same bit for bit either way.
 *   mode 0: off -- every sample marches every selected path (rounds 1-4; the shared-leg path tree).
 * Applies to at most 128 paths and 4096 samples per pixel; beyond, lf_trace_ghosts marches everything (lf_get_cull_reason says why).
 * lf_get_cull_info: {mode, did the last lf_trace_ghosts cull, blocks_x, blocks_y, cells per block (the pupil
 * strata G x G), G, pre-pass cells per axis, block size in pixels}.  lf_get_cull_table: the masks the last
 * launch used, [blocks_y * blocks_x][cells + 1] (block side = info[7] pixels; bit q = path q of the selection in lf_set_ghost_pairs order,
 * the primary path first; entry `cells` = the union, used by the unstratified samples s >= G * G), so that a
 * checker can march exactly what the device marched. */
lf_status lf_set_march_culling(lf_ctx* ctx, int mode);
lf_status lf_get_cull_info(lf_ctx* ctx, int info[8]);
lf_status lf_get_cull_table(lf_ctx* ctx, uint64_t* out, size_t n_entries);
/* of all (block, cell, path) combinations, the fraction the last pre-pass found able to carry light.  Above
 * 0.10 + 1.6 / paths (0.135 with 46 paths, 0.18 with 21) lf_trace_ghosts marches everything after all (the path tree
 * shares legs and lets rays die early; the culled march starts each path alone): a very wide sun or a handful of
 * samples per pixel. */
lf_status lf_get_cull_started_fraction(lf_ctx* ctx, double* fraction);
/* WHY the last lf_trace_ghosts did, or did not, cull (informational: lf_trace_ghosts returns LF_OK either way and the
 * pixels are the same -- what changes is the time: the path tree marches every path of every sample). */
typedef enum {
  LF_CULL_APPLIED = 0,              /* the culled march ran */
  LF_CULL_OFF = 1,                  /* lf_set_march_culling(0) */
  LF_CULL_NO_STOP = 2,              /* the prescription has no stop: nothing bounds a pupil cell */
  LF_CULL_TOO_MANY_PATHS = 3,       /* more than 128 selected paths -- or more than 64 with a table that is not the context's
                                       alone (shared, lf_comm_share_cull / lf_set_cull_share, or dealt by blocks, lf_set_block_deal) */
  LF_CULL_TOO_MANY_SAMPLES = 4,     /* more than 4096 samples per pixel (64 x 64 strata) */
  LF_CULL_BLOCK_TOO_LARGE = 5,      /* even a block of 16 x 16 pixels is more than 1.8 mm on this sensor */
  LF_CULL_TABLE_TOO_FULL = 6,       /* the table starts more than 0.10 + 1.6 / paths of everything: the path tree is faster */
  LF_CULL_AUDIT_REFUTED = 7,        /* an audit ray of a dropped box reached the light: the table was not used (see below) */
  LF_CULL_DISPERSION = 8,           /* the index columns are not monotonic in the wavelength: the two ends of the spectrum
                                       do not bracket what lies between, the pre-pass's dispersion bound does not hold */
  LF_CULL_ASPHERIC = 9,             /* the lens has an aspheric interface (lf_set_lens_aspheres): the pre-pass's bounds were found
                                       on spherical designs, no table is built and neither pre-pass nor audit launches */
  LF_CULL_ANAMORPHIC = 10,          /* the lens has a biconic interface (lf_set_lens_biconics): likewise, and the pre-pass's boxes
                                       assume surfaces of revolution */
  LF_CULL_POSED = 11                /* the lens has a posed interface (lf_set_lens_poses): likewise, and the boxes assume a
                                       centred lens */
} lf_cull_reason;
lf_status lf_get_cull_reason(lf_ctx* ctx, int* reason);
/* THE AUDIT.  The pre-pass's bounds are second-order estimates from 15 rays per box: conservative on every
 * frame anyone has compared with the full enumeration, but not a proof.  Every table is therefore checked where it is
 * used: for each (block, cell, path) combination it does NOT start, `rays_per_dropped_box` rays of that box (a random
 * point of the block, a random point of the pupil cell, one of the launch's wavelengths) are marched with the march's
 * own events; one that ends inside the sun's lobe refutes the table -- the launch marches every path of every sample
 * instead (same pixels as always, the path tree's time), lf_get_cull_reason says LF_CULL_AUDIT_REFUTED and the counters
 * below say how often.  Default 1 ray (0.9 ms on the 1080p bench frame); 0 switches the audit off.
 * lf_get_cull_audit: rays marched / rays that reached the light / launches refuted, since lf_reset_counters. */
lf_status lf_set_cull_audit(lf_ctx* ctx, int rays_per_dropped_box);
lf_status lf_get_cull_audit(lf_ctx* ctx, uint64_t* rays, uint64_t* lit, int* launches_refuted);
/* TEST HOOK -- not for hosts.  The switches the test suite and bench.py's A/B legs need, by name (no environment
 * variable changes what this library computes):
 *   "cull_force" 0/1            keep the culled march whatever the table starts (small test frames)
 *   "cull_weights_first" 0/1    the Fresnel / mask weight on EVERY executed event (SURVEY 8d's unit), same pixels
 *   "cull_no_prefix" 0/1        every started path marched alone from the sensor (round 5's culled march), same pixels
 *   "cull_ignore_light" k       -1 (default): off; k: the cull pre-pass and the resolve leave light k of lf_set_lights out -- a
 *                               table wrong by construction; the march and the audit still see light k (the audit's test)
 *   "cull_no_widening" 0/1      1: a point light (lf_set_lights_ex) enters the cull table with a directional light's radius, not
 *                               widened by r_f / (|L| - r_f) -- a table wrong by construction for a light close to the lens
 *                               (an area light, lf_set_lights_geom: with its corners' reach alone, not widened by r_f / (dmin - r_f))
 *   "cull_cache" 0/1            0: no cached tree -- every pre-pass marches its boxes (the tree a context holds is kept), same table
 *   "cull_cache_max_mb" MiB     the cached tree's byte budget (default 8192)
 *   "cull_general_kernel" 0/1   build the table with the kernel that takes its rules as arguments (must give the shipped one's table)
 *   "cull_strict", "cull_strict_lost", "cull_slack", "cull_keep_partial", "cull_disable", "cull_margin", "cull_lobe_k",
 *   "cull_lost_rel", "cull_lost_abs"   the pre-pass rules round 5 REPLACED (they lose lit rays on some prescriptions:
 *                               what the audit is shown to catch, tests/test_gpu_cull.py)
 *   "scene_compact" -1/0/1      k_scene_lens's ray compaction: by the tree's size / off / on
 *   "scene_lens_strided" -1/0/1 k_scene_lens's wave tile: by the tree's size / 8 x 8 neighbours / the march's strided tile
 *   "bvh_median" 0/1, "bvh_leaf" 1..4   the scene tree of the next lf_set_scene: median splits (round 2), primitives per leaf
 *   "comm_force_exchange" 0/1   run the collectives with a single rank as well
 *   "march_tail_tiles" n, "march_tail_groups" g   the culled march splits its LAST n wave tiles over g workgroups each so that a
 *                               launch ends on short workgroups (-1 / -1: the default, half a round of resident workgroups x 4;
 *                               0 / 1: no split); same pixels and counters whatever the values
 *   "asph_force" 0/1            launch the aspheric lens's kernel (k_march_asph) on a lens WITHOUT aspheres: every curved glass row
 *                               takes the Newton path with a zero record -- what lets the float64 oracle judge that kernel
 * Unknown names are refused.  ctx == NULL: the value becomes the default of every context created afterwards (a
 * test that cannot reach the contexts a helper creates); 0 takes the default away. */
lf_status lf_test_knob(lf_ctx* ctx, const char* name, double value);
/* THE PRE-PASS OF A MULTI-GPU FRAME, SHARED.  The table covers the whole frame (a block of 64 sensor rows holds tile
 * rows of every rank), so N ranks that each build all of it spend the same time on it as one GPU does: the part of a
 * frame that does not shrink with N.  Shared, rank r builds the rows of the blocks b with b % N == r (dealt round
 * robin: what a block costs depends on the ghosts that cross it), the rows of one rank lie together (its slab; equal
 * slabs, the last ones padded) and ONE all-gather per table completes it on every rank -- the second and last
 * collective of a frame.  Every rank must make the same launches with the same inputs (lens, pairs, sun, frame,
 * mask, sample count): the exchange is collective.  ghost_buffer, counters and lf_get_cull_table (handed out in block
 * order whatever the layout) are those of a table built alone, bit for bit.
 *   lf_comm_share_cull(ctx, 1)     after lf_comm_init_rank: lf_trace_ghosts completes the table itself, by an
 *                                  ncclAllGather on the communicator's stream (in place, between pre-pass and march).
 *   lf_set_cull_share(rank, N)     the HOST owns the exchange (no usable RCCL communicator: torch.distributed, MPI,
 *                                  a rehearsal on one device): per launch lf_cull_prepare(spp) builds this rank's slab,
 *                                  lf_cull_table_view hands out the device table {pointer, entries, entries per rank}
 *                                  (all zero if this launch does not cull) for an in-place all-gather of slabs in rank
 *                                  order, lf_cull_commit takes the completed table over, and the lf_trace_ghosts that
 *                                  follows (same spp, same inputs) marches with it; a launch without them is refused.
 *                                  (1 rank: off.)
 * Both are refused (LF_ERR_STATE) on a frame dealt by blocks (lf_set_block_deal), which shares nothing. */
lf_status lf_comm_share_cull(lf_ctx* ctx, int on);
lf_status lf_set_cull_share(lf_ctx* ctx, int rank, int nranks);
lf_status lf_cull_prepare(lf_ctx* ctx, int spp);
lf_status lf_cull_table_view(lf_ctx* ctx, void** device_ptr, uint64_t* entries, uint64_t* entries_per_rank);
lf_status lf_cull_commit(lf_ctx* ctx);
/* the fixed-point exponent the last lf_trace_ghosts used (36 unless the range contract above lowered it) */
lf_status lf_get_march_fix_bits(lf_ctx* ctx, int* bits);
/* replaces: LensCamera::generate_ray of the north star / Camera::generate_ray_for_thin_lens
 * (declared camera.h:168, a stub in camera_lens.cpp:22-30), batched: for n sensor samples -- sensor
 * position in mm (x, y; the lens inverts the image) and a rear-pupil sample in [-1,1]^2 -- march the
 * primary path through the prescription at wavelength index `lambda`.  out: n x 8 floats
 * {origin xyz on the front element, unit direction xyz towards the scene, transmitted weight,
 * alive (1/0)} in lens space (optical axis = z, light travels +z, the scene lies at z < 0). */
lf_status lf_generate_lens_rays(lf_ctx* ctx, int lambda, size_t n, const float* sensor_xy_mm,
                                const float* pupil_uv, float* out);
/* How the flare layer evaluates the two powers of the reference's starburst / falloff code --
 * `radiance / pow(r, 1.5)` (calculate_irradiance_falloff, pathtracer.cpp:1056) and `pow(factor, 8.0)`
 * (raytrace_starburst, :982):
 *   1  exact: the double-precision pow the reference calls (the device's libm, <= 1 ulp like glibc's)
 *   2  fast:  rsqrt(r^3) and three squarings (~3 and ~4 ulp from exact; 0.34 -> 0.15 ms per 1080p frame)
 *   0  auto (default): exact in MT19937 parity mode -- the mode that exists to reproduce the reference's
 *      frames, where agreement must hold by construction -- fast with the counter RNG
 * Either way the result is far inside the north star's 1e-4 (and the parity tests' 1e-9). */
lf_status lf_set_flare_arithmetic(lf_ctx* ctx, int mode);
/* ---- the lens camera of the scene term (round 4) -----------------------------------------------
 * replaces: the call `camera->generate_ray(x, y)` in the sample loop of PathTracer::raytrace_pixel
 * (src/pathtracer/pathtracer.cpp:841-850) -- a pinhole in the reference (camera.cpp:278-305; its
 * thin-lens variant is a stub, camera_lens.cpp:22-30, declared camera.h:168) -- by the north star's
 * "for each sensor sample, march a ray through the lens prescription ... accumulate radiance into
 * the sensor buffer": with mode != 0 lf_render_scene_term starts sample s of pixel (x, y) exactly as
 * lf_trace_ghosts does (the same counter-RNG block, sensor point, pupil stratum and sub-cell; key =
 * lf_set_jitter_counter's, strata for ns_aa samples), marches its primary path N-1 .. 0 through the
 * prescription with the Fresnel / aperture weight (the arithmetic of lf_generate_lens_rays), carries
 * the exit ray into the scene by the camera's pose (lens space = camera space: x right, y up, scene
 * at -z; lens millimetres times world_per_mm; the centre of the paraxial entrance pupil sits at the
 * camera position) and weights the radiance it finds by exposure x transmitted weight.  A sample the
 * lens blocks contributes 0 and still counts in the mean (the division by the loop variable,
 * pathtracer.cpp:875, is unchanged).  The loop visits the march's samples 0 .. ns_aa-1 in a scattered
 * order (iteration i takes sample (i * step) mod ns_aa, step = the integer nearest ns_aa / 1.618 that is
 * coprime to ns_aa) so that the reference's adaptive early-out (:862-868) stops on a prefix that covers
 * the pupil, not on its rim.
 *   mode 0  off: the reference's pinhole camera (default)
 *   mode 1  one ray per sample at the reference wavelength (index n_lambda / 2) carries R, G and B
 *   mode 2  one ray per wavelength; channel c collects lambda_rgb[l][c] of wavelength l's radiance
 *           (lateral and axial colour show; n_lambda closest-hit searches per sample)
 * exposure <= 0 calibrates: 1 / (mean transmitted weight of the on-axis sensor point over a 64 x 64
 * grid of pupil points, reference wavelength), so that a scene of uniform radiance L renders as L at
 * the frame's centre -- what the reference's pinhole returns everywhere.  The calibration and the
 * interface table follow later changes of the lens, the stop mask and the pupil target.
 * Needs lf_set_lens / lf_load_lens_file, the stop mask (LF_APERTURE_STARBURST slot), lf_set_camera
 * and the counter RNG (MT19937 parity mode is refused: its table has no pupil draws).
 * lf_get_lens_camera: the settings in force (after calibration) and the entrance pupil's z (mm).  With a mode other
 * than 0 it brings table and calibration up to date first, as lf_render_scene_term does, and so fails as that call
 * would: on an aspheric lens (lf_set_lens_aspheres) or one with biconic interfaces (lf_set_lens_biconics) both return
 * LF_ERR_UNSUPPORTED under the default setting (lf_set_lens_camera_surfaces below) -- the calibration belongs to a
 * scene image that the default does not form for such a lens, and the getter reports no figure that no frame would use.
 * With mode 0 it succeeds on any lens. */
lf_status lf_set_lens_camera(lf_ctx* ctx, int mode, double world_per_mm, double exposure);
lf_status lf_get_lens_camera(lf_ctx* ctx, int* mode, double* world_per_mm, double* exposure,
                             double* entrance_pupil_z_mm);
/* Where the lens camera's samples aim.  margin <= 0 (default): at the march's disc (the rear element's clear
 * aperture, or lf_set_pupil_target's) -- the scene ray of a sample IS the march's primary path, and with a
 * pentagon stop about a quarter of the samples leaves the lens.  margin > 0: at the paraxial image of the
 * stop's open part through the rear group, times margin (as lf_aim_at_exit_pupil computes it; > 1 leaves room
 * for the pupil's aberration off the axis) -- an unbiased estimator for the primary path, the only path the
 * lens camera marches, under which more of the samples pass (1.2-1.8x with a pentagon stop, whose area is 76 %
 * of its circumscribed circle); the march's own sampling is not touched.  Same expectation; the exposure
 * calibration follows. */
lf_status lf_set_lens_camera_aim(lf_ctx* ctx, float margin);
/* Which interfaces the lens camera's primary path may meet (a setting of the context: nothing clears it).
 *   LF_LENSCAM_SURFACES_SPHERICAL (default)  spheres, flats and the stop: every refusal above, every message and every bit of
 *                                            a frame as they always were
 *   LF_LENSCAM_SURFACES_ALL                  lf_render_scene_term and lf_get_lens_camera also accept a lens with aspheric and / or
 *                                            biconic records: the scene kernel marches a recorded row with the event of
 *                                            lf_march_path_rays (a fixed number of Newton steps), every other row as before --
 *                                            the scene image such a lens forms: an anamorphic lens's squeeze and oval bokeh, where
 *                                            its ghosts belong.  A lens without records launches the kernels it always launched
 *                                            and renders the same frame bit for bit.
 *   LF_LENSCAM_SURFACES_POSED                everything LF_LENSCAM_SURFACES_ALL accepts, plus pose records (lf_set_lens_poses):
 *                                            the scene kernel marches a posed row with lf_march_path_rays' posed event, in the
 *                                            frame of the surface -- the image shifts, the field tilts, the bokeh goes lopsided.
 *                                            A lens without pose records launches what it launches under ALL, bit for bit.
 *                                            Under the two settings above a posed lens stays LF_ERR_UNSUPPORTED.
 * The value reads as bits -- 1: aspheric / biconic records, 2: poses -- and a posed face always runs in a recorded event's
 * frame, so 2 alone is no setting (LF_ERR_INVALID).
 * Focus (lf_focus_lens), the entrance pupil (where the camera position sits in the lens) and the exit-pupil aim
 * (lf_set_lens_camera_aim) keep meaning the y meridian's paraxial quantities: for an anamorphic lens a convention about
 * where the camera sits, not an approximation of the image, which real rays form.  The exposure calibration follows the
 * records (it goes through lf_generate_lens_rays).  The per-lane test kernel (lf_test_knob("scene_compact", 0)) has no
 * instantiation for records: LF_ERR_UNSUPPORTED.  Any other value: LF_ERR_INVALID.  A change re-derives table and calibration. */
typedef enum { LF_LENSCAM_SURFACES_SPHERICAL = 0, LF_LENSCAM_SURFACES_ALL = 1, LF_LENSCAM_SURFACES_POSED = 3 } lf_lenscam_surfaces;
lf_status lf_set_lens_camera_surfaces(lf_ctx* ctx, int which);
lf_status lf_get_lens_camera_surfaces(lf_ctx* ctx, int* which);
/* The lens camera's samples, as the device draws them: out[(i * ns_aa + s) * 4 ..] = {X, Y, pa, pb} -- the sensor point in mm
 * and the pupil-square coordinates in [-1, 1]^2 of the march's sample s = 0 .. ns_aa-1 of pixel pixels[i] = x + y W --
 * computed on the device by the functions the scene kernels call, so bit for bit the values their start ray is aimed from.
 * lf_generate_lens_rays(lambda, XY, uv) on them gives, bit for bit, the exit ray and weight the scene kernel carries into
 * the scene for that sample under the march's disc (lf_set_lens_camera_aim(0)): a host or a float64 tracer can follow the
 * lens camera sample by sample, for any kind of lens.  Needs lf_set_frame, lf_set_params (ns_aa >= 1) and lf_set_lens
 * (LF_ERR_STATE) and the counter RNG, lf_set_jitter_counter; the samples follow lf_set_tile_stride and
 * lf_set_pupil_subcells.  MT19937 parity mode or a pixel outside the frame: LF_ERR_INVALID. */
lf_status lf_lens_camera_samples(lf_ctx* ctx, size_t n_pixels, const int* pixels, float* out);
/* the paraxial image of the stop's centre through the interfaces IN FRONT of it (host arithmetic with
 * the reference's T / R operators, pathtracer.cpp:527-533): its z in lens space (the front vertex is
 * z = 0, the scene at z < 0; typically a few mm > 0, inside the lens) and its lateral magnification */
lf_status lf_paraxial_entrance_pupil(int n_surfaces, int stop_index, const float* radius, const float* thickness,
                                     const float* ior_row, double* z_mm, double* magnification);
/* replaces: Camera::focalDistance (camera.h:174; the -d flag) for a real lens: moves the sensor -- the
 * prescription's last thickness -- to the paraxial image (reference wavelength) of an axial object
 * object_distance_mm in front of the first vertex; <= 0 or infinite: focus at infinity.  The pair
 * selection, wavelength weights and a still-valid pupil target survive; march program, lens-camera
 * table and calibration are rebuilt on next use.  sensor_distance_mm: the new last thickness. */
lf_status lf_focus_lens(lf_ctx* ctx, double object_distance_mm, float* sensor_distance_mm);
/* the same with the distance measured from the CAMERA POSITION of the lens camera -- the centre of the paraxial
 * entrance pupil (lf_paraxial_entrance_pupil; 19.95 mm behind the double Gauss's first vertex) -- which is what
 * Camera::focalDistance means (camera.h:174: the drop-in passes it here) */
lf_status lf_focus_lens_from_pupil(lf_ctx* ctx, double distance_from_entrance_pupil_mm, float* sensor_distance_mm);
/* replaces: BVHAccel::total_rays / total_isects (src/scene/bvh.h:85,105,136; bvh.cpp:211), the numbers
 * behind the reference's end-of-frame log (raytraced_renderer.cpp:706-709), as the device's scene
 * kernel counts them since the last reset: out = {rays handed to the closest-hit / occlusion search
 * (camera + shadow + hemisphere rays), primitive tests of closest-hit searches, lens-camera samples
 * started (one per sample and traced wavelength), of those that left the front element} */
lf_status lf_get_scene_counters(lf_ctx* ctx, uint64_t out[4]);
lf_status lf_reset_scene_counters(lf_ctx* ctx);
/* Host logic of the march, inspectable WITHOUT a device (used by the CPU tests): builds what
 * lf_trace_ghosts uploads for a prescription and a pair selection (arguments as lf_set_lens /
 * lf_set_ghost_pairs; pairs = NULL selects every glass pair).
 *   info   int[8 + 4 (LF_MAX_PAIRS + 1)]: {n_paths, flat rows per wavelength, first program row,
 *          program rows per wavelength, total rows, jump-table entries, 0, 0} then per path
 *          {i, j, first flat row, flat rows}
 *   rows   8 x 4 bytes per row: dzv (vertex z of the interface the ray comes from, or of the sensor,
 *          minus this interface's), curv, h2, eta, sgn (floats), flags (int), radius, eta^2 (floats);
 *          n_lambda x flat sequences, then n_lambda x the path-tree program, then one spare row
 *   skip   one int per program row: (rows to jump << 2) | state to restore, for a wave that is dead
 * flags: 1 mirror, 2 stop, 4 flat, 8 restore slot 1 after END, 0x10 / 0x20 park in slot 0 / 1
 * before the event, 0x40 END of a path, 0x80 restore slot 0 after END; bits 8-15 run length,
 * 16-23 number of paths sharing the row, 24-31 the path an END row completes.
 * rows / skip may be NULL to query the sizes (info[4], info[5]) first. */
lf_status lf_march_tables(int n_surfaces, int stop_index, int n_lambda, const float* radius,
                          const float* thickness, const float* ior, const float* semi_aperture,
                          const int* pairs, int n_pairs, int include_primary, int* info,
                          float* rows, size_t rows_cap, int* skip, size_t skip_cap);
/* Spectral starburst (no reference counterpart -- the reference's
 * starburst, pathtracer.cpp:947-1000, is monochrome).  n = 0 restores the reference behaviour.
 * Wavelength l sees the reference's diffraction pattern magnified by 1 / scale[l]
 * (scale = lambda_ref / lambda_l), shaped like the reference's value and added with the weights
 * rgb_weights[3 l + {0,1,2}]; n <= LF_MAX_LAMBDA.  One wavelength with scale 1 and weights
 * (1,1,1) is the reference formula.  Takes effect at the next lf_render_flare_layer. */
lf_status lf_set_starburst_spectrum(lf_ctx* ctx, int n, const double* scale, const double* rgb_weights);
/* y[k] = the square root of x[k] exactly as the march computes it (the CDNA4 v_sqrt_f32
 * instruction, 1 ulp).  Host pointers.  No reference counterpart: the parity tests measure the
 * instruction's deviation from the correctly rounded root with this call and hand it to the CPU
 * oracle, which then follows the device bit for bit (oracle/lf_geo_oracle.c, geo_set_sqrt_table). */
lf_status lf_native_sqrt(lf_ctx* ctx, const float* x, float* y, size_t n);
/* y[k] = the reciprocal of x[k] exactly as the march computes it (v_rcp_f32, 1 ulp): its divisions on
 * the per-event and per-sample path are multiplications by this reciprocal (round 4).  As for the root,
 * the parity tests measure its deviation from the correctly rounded reciprocal -- a function of the
 * significand alone -- and hand it to the CPU oracle (geo_set_rcp_table). */
lf_status lf_native_rcp(lf_ctx* ctx, const float* x, float* y, size_t n);
lf_status lf_get_counters(lf_ctx* ctx, lf_counters* out);
lf_status lf_reset_counters(lf_ctx* ctx);
/* Ray-surface events the device actually computed since the last reset: the paths of one sensor
 * sample start with the same backward leg and the pairs (i, .) share the forward leg after the
 * reflection at i, and the march computes every shared leg once (no reference counterpart). */
lf_status lf_get_executed_events(lf_ctx* ctx, uint64_t* out);
/* What the counted events cost in full (no reference counterpart): the march's first pass computes
 * intersection + refraction / reflection for every event; the Fresnel / aperture WEIGHT of an event is
 * computed by marching a finished path a second time, and only for waves in which a lane reached the
 * light's lobe.  out = {executed events (= lf_get_executed_events), events of those second marches
 * counted for the lanes that needed them (= events that ever had a Fresnel factor evaluated), rows of
 * those second marches (each row is one event for all 64 lanes of a wave), 0}.  The second marches are
 * NOT part of `executed events`. */
lf_status lf_get_march_stats(lf_ctx* ctx, uint64_t out[4]);

/* ---------------------------------------------------------------- measurement ------------ */
/* HIP-event timing of the kernels launched since the last reset, on the context's stream.
 * kernel: "march", "flare_layer", "ghost_raster", "dft", "frame_setup", "tonemap", "scene_term",
 * "exchange" (pack -> all-gather -> unpack of lf_comm_gather / _async, on the stream it runs on),
 * "flare_visibility" (both launches of lf_set_flare_occlusion as one entry per consuming call; none while it is off). */
lf_status lf_timing_enable(lf_ctx* ctx, int on);
lf_status lf_timing_reset(lf_ctx* ctx);
lf_status lf_timing_get(lf_ctx* ctx, const char* kernel, int* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* LENSFLARE_H */
