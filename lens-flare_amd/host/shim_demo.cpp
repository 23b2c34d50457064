// shim_demo.cpp -- drives lfamd::PathTracer exactly the way the reference's
// RaytracedRenderer::start_raytracing / raytrace_tile do (src/pathtracer/raytraced_renderer.cpp
// :300-311, :314-328, :622-647) and dumps the buffers.  tests/test_gpu_host_shim.py feeds it the
// golden cases and compares against the real reference's output.
//
//   shim_demo <case.txt> <aperture.f32> <ghost.f32> <outprefix> [n_threads]
// case.txt: W H ns_aa flare_radius flare_intensity hFov vFov  pos(3)  c2w(9)  aw ah gw gh
//           n_lights  then n_lights x (posLight xyz, radiance rgb)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <fstream>
#include <thread>
#include <vector>

#include "lf_pathtracer.h"

using namespace lfamd;

static std::vector<float> read_f32(const char* path, size_t n) {
  std::vector<float> v(n);
  FILE* f = fopen(path, "rb");
  if (!f || fread(v.data(), sizeof(float), n, f) != n) { perror(path); exit(2); }
  fclose(f);
  return v;
}

template <typename T>
static void dump(const std::string& path, const T* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  fwrite(p, sizeof(T), n, f);
  fclose(f);
}

// shim_demo geo <lens.txt> <mask.f32> <mw> <mh> <W> <H> <spp> <sun x y z> <angular radius> <outprefix>
// lens.txt: n stop n_lambda sensor_w, then n rows {radius thickness semi_aperture ior[0..n_lambda)}
// The north star's plug-in surface through the C++ mirror: PathTracer::use_geometric_ghosts +
// generate_ghost_buffer (the geometric march fills ghost_buffer) and LensCamera::generate_rays
// (camera rays that really went through the prescription).
static int geo_main(int argc, char** argv) {
  if (argc < 14) return 1;
  std::ifstream in(argv[2]);
  int n, stop, nl;
  float sensor_w;
  in >> n >> stop >> nl >> sensor_w;
  std::vector<float> radius(n), thick(n), semi(n), ior((size_t)n * nl);
  for (int k = 0; k < n; k++) {
    in >> radius[k] >> thick[k] >> semi[k];
    for (int l = 0; l < nl; l++) in >> ior[(size_t)l * n + k];
  }
  const size_t mw = atoi(argv[4]), mh = atoi(argv[5]), W = atoi(argv[6]), H = atoi(argv[7]);
  const int spp = atoi(argv[8]);
  const float sun[3] = {(float)atof(argv[9]), (float)atof(argv[10]), (float)atof(argv[11])};
  const float alpha = (float)atof(argv[12]);
  const std::string out = argv[13];
  try {
    PathTracer pt(0);
    Camera cam;
    CameraApertureTexture ap;
    ap.init_from_texels(read_f32(argv[3], mw * mh).data(), mw, mh);
    cam.aperture_texture = &ap;
    cam.ghost_aperture_texture = &ap;
    pt.clear();
    pt.set_frame_size(W, H);
    pt.camera = &cam;
    pt.counter_jitter = true;
    pt.flare_radiance.emplace_back(1.0, 0.9, 0.5);       // the radiance the march takes for the sun
    pt.flare_origins.emplace_back(0.5, 0.5);
    pt.axis_ray = Vector2D(0.5, 0.5);
    pt.use_geometric_ghosts(n, stop, nl, radius.data(), thick.data(), ior.data(), semi.data(), sensor_w, sun,
                            alpha, spp);
    pt.generate_ghost_buffer();
    dump(out + ".ghost.f64", &pt.ghost_buffer.data[0].x, W * H * 3);
    // LensCamera: a grid of sensor positions x pupil samples
    LensCamera lc(&pt, sensor_w, sensor_w * (float)H / (float)W);
    std::vector<double> q;
    for (int i = 0; i < 16; i++)
      for (int j = 0; j < 16; j++) {
        q.push_back(0.1 + 0.8 * i / 15.0); q.push_back(0.1 + 0.8 * j / 15.0);
        q.push_back(0.05 + 0.9 * ((i * 7 + j * 3) % 16) / 15.0); q.push_back(0.05 + 0.9 * ((i * 5 + j * 11) % 16) / 15.0);
      }
    std::vector<Ray> rays;
    std::vector<double> w;
    lc.generate_rays(q.size() / 4, q.data(), &rays, &w, nl / 2);
    std::vector<double> flat;
    for (size_t i = 0; i < rays.size(); i++)
      flat.insert(flat.end(), {rays[i].o.x, rays[i].o.y, rays[i].o.z, rays[i].d.x, rays[i].d.y, rays[i].d.z, w[i],
                               (double)rays[i].depth});
    dump(out + ".rays.f64", flat.data(), flat.size());
    dump(out + ".query.f64", q.data(), q.size());
    Ray one;
    double w1 = 0;
    const bool alive = lc.generate_ray(0.5, 0.5, 0.5, 0.5, &one, &w1, nl / 2);   // the chief ray
    printf("chief ray alive=%d d=(%g, %g, %g) w=%g\n", (int)alive, one.d.x, one.d.y, one.d.z, w1);
  } catch (const std::exception& e) {
    fprintf(stderr, "shim_demo geo: %s\n", e.what());
    return 3;
  }
  return 0;
}

// shim_demo geolights <lens.txt> <mask.f32> <mw> <mh> <W> <H> <spp> <angular radius> <outprefix> <n> then n x {ox oy r g b}
// Several in-frame lights through the mirror's frame sequence: the flare state as a host leaves it in the public fields
// (normalised screen positions, radiances), PathTracer::use_lights_from_flares, generate_ghost_buffer -- every light gets
// its lens ghosts in ONE march.
static int geolights_main(int argc, char** argv) {
  if (argc < 12) return 1;
  std::ifstream in(argv[2]);
  int n, stop, nl;
  float sensor_w;
  in >> n >> stop >> nl >> sensor_w;
  std::vector<float> radius(n), thick(n), semi(n), ior((size_t)n * nl);
  for (int k = 0; k < n; k++) {
    in >> radius[k] >> thick[k] >> semi[k];
    for (int l = 0; l < nl; l++) in >> ior[(size_t)l * n + k];
  }
  const size_t mw = atoi(argv[4]), mh = atoi(argv[5]), W = atoi(argv[6]), H = atoi(argv[7]);
  const int spp = atoi(argv[8]);
  const float alpha = (float)atof(argv[9]);
  const std::string out = argv[10];
  const int n_lights = atoi(argv[11]);
  if (argc < 12 + 5 * n_lights) return 1;
  try {
    PathTracer pt(0);
    Camera cam;
    CameraApertureTexture ap;
    ap.init_from_texels(read_f32(argv[3], mw * mh).data(), mw, mh);
    cam.aperture_texture = &ap;
    cam.ghost_aperture_texture = &ap;
    pt.clear();
    pt.set_frame_size(W, H);
    pt.camera = &cam;
    pt.counter_jitter = true;
    for (int k = 0; k < n_lights; k++) {
      char** v = argv + 12 + 5 * k;
      pt.flare_origins.emplace_back(atof(v[0]), atof(v[1]));
      pt.flare_radiance.emplace_back(atof(v[2]), atof(v[3]), atof(v[4]));
    }
    pt.axis_ray = Vector2D(0.5, 0.5);
    const float placeholder[3] = {0.0f, 0.0f, -1.0f};      // (replaced by the flare state's lights at the frame)
    pt.use_geometric_ghosts(n, stop, nl, radius.data(), thick.data(), ior.data(), semi.data(), sensor_w, placeholder, alpha, spp);
    pt.use_lights_from_flares(alpha);
    pt.generate_ghost_buffer();
    dump(out + ".ghost.f64", &pt.ghost_buffer.data[0].x, W * H * 3);
  } catch (const std::exception& e) {
    fprintf(stderr, "shim_demo geolights: %s\n", e.what());
    return 3;
  }
  return 0;
}

// shim_demo geowall <lens.txt> <mask.f32> <mw> <mh> <W> <H> <spp> <sun x y z> <angular radius> <outprefix> <wall: 0 none, 1 hides the sun, 2 its left half>
// A wall in front of the sun: the march's ghosts under PathTracer::use_ghost_occlusion.  The wall is a 2 m x 2 m quad 5 m
// from the camera (identity pose at the origin, 1 scene unit = 1 m), square to the sun's direction and centred on it (1),
// or shifted so that its edge crosses the sun (2).  Dumps the ghost buffer and prints the shadow tests made / blocked.
static int geowall_main(int argc, char** argv) {
  if (argc < 15) return 1;
  std::ifstream in(argv[2]);
  int n, stop, nl;
  float sensor_w;
  in >> n >> stop >> nl >> sensor_w;
  std::vector<float> radius(n), thick(n), semi(n), ior((size_t)n * nl);
  for (int k = 0; k < n; k++) {
    in >> radius[k] >> thick[k] >> semi[k];
    for (int l = 0; l < nl; l++) in >> ior[(size_t)l * n + k];
  }
  const size_t mw = atoi(argv[4]), mh = atoi(argv[5]), W = atoi(argv[6]), H = atoi(argv[7]);
  const int spp = atoi(argv[8]);
  const float sun[3] = {(float)atof(argv[9]), (float)atof(argv[10]), (float)atof(argv[11])};
  const float alpha = (float)atof(argv[12]);
  const std::string out = argv[13];
  const int wall = atoi(argv[14]);
  try {
    PathTracer pt(0);
    Camera cam;
    CameraApertureTexture ap;
    ap.init_from_texels(read_f32(argv[3], mw * mh).data(), mw, mh);
    cam.aperture_texture = &ap;
    cam.ghost_aperture_texture = &ap;
    pt.clear();
    pt.set_frame_size(W, H);
    pt.camera = &cam;
    pt.counter_jitter = true;
    pt.flare_radiance.emplace_back(1.0, 0.9, 0.5);
    pt.flare_origins.emplace_back(0.5, 0.5);
    pt.axis_ray = Vector2D(0.5, 0.5);
    pt.use_geometric_ghosts(n, stop, nl, radius.data(), thick.data(), ior.data(), semi.data(), sensor_w, sun, alpha, spp);
    if (wall) {
      // the sun's direction s (lens space = camera space here), two unit vectors u, v square to it
      const double sl = std::sqrt((double)sun[0] * sun[0] + (double)sun[1] * sun[1] + (double)sun[2] * sun[2]);
      const double s[3] = {sun[0] / sl, sun[1] / sl, sun[2] / sl};
      double u[3] = {-s[2], 0.0, s[0]};                              // (s x y: the sun is never along y here, z < 0)
      const double ul = std::sqrt(u[0] * u[0] + u[2] * u[2]);
      u[0] /= ul; u[2] /= ul;
      const double v[3] = {s[1] * u[2] - s[2] * u[1], s[2] * u[0] - s[0] * u[2], s[0] * u[1] - s[1] * u[0]};
      const double shift = wall == 2 ? -1.0 : 0.0, dist = 5.0;
      double c[4][3];
      const double cu[4] = {-1.0 + shift, 1.0 + shift, 1.0 + shift, -1.0 + shift}, cv[4] = {-1.0, -1.0, 1.0, 1.0};
      for (int i = 0; i < 4; i++)
        for (int a = 0; a < 3; a++) c[i][a] = dist * s[a] + cu[i] * u[a] + cv[i] * v[a];
      double pos[18], nrm[18];
      const int idx[6] = {0, 1, 2, 0, 2, 3};
      for (int i = 0; i < 6; i++)
        for (int a = 0; a < 3; a++) { pos[3 * i + a] = c[idx[i]][a]; nrm[3 * i + a] = -s[a]; }
      const int tri_mat[2] = {0, 0};
      const double mats[4] = {0.0, 0.5, 0.5, 0.5};                   // diffuse grey
      pt.set_scene(0, nullptr, nullptr, 2, pos, nrm, tri_mat, 1, mats, 0, nullptr);
      pt.use_ghost_occlusion(true);
    }
    pt.generate_ghost_buffer();
    dump(out + ".ghost.f64", &pt.ghost_buffer.data[0].x, W * H * 3);
    uint64_t st[2] = {0, 0};
    if (lf_get_ghost_occlusion_stats(pt.context(), st) != LF_OK) throw std::runtime_error(pt.last_error());
    printf("shadow tests %llu blocked %llu\n", (unsigned long long)st[0], (unsigned long long)st[1]);
  } catch (const std::exception& e) {
    fprintf(stderr, "shim_demo geowall: %s\n", e.what());
    return 3;
  }
  return 0;
}

// shim_demo geolamp <lens.txt> <mask.f32> <mw> <mh> <W> <H> <spp> <lamp x y z> <angular radius> <outprefix>
//                   <wall: 0 none, 1 between camera and lamp, 2 across half the beam, 3 behind the lamp>
// A lamp in the room and a wall: the march's ghosts of a PointLight of the scene (use_lights_from_scene) under
// use_ghost_occlusion + use_ghost_occlusion_reach(LF_OCCLUSION_REACH_LIGHT).  The lamp stands at <x y z> in world units
// (identity pose at the origin, 1 scene unit = 1 m, z < 0); the wall is a quad square to the lamp's direction, its half
// side 0.4 of its distance: half way to the lamp and centred on it (1), or shifted so that its edge crosses the lamp's
// direction (2), or twice as far as the lamp (3).  Without a wall the scene holds one small sphere behind the camera and
// occlusion stays off.  Dumps the ghost buffer and prints the shadow tests made / blocked.
static int geolamp_main(int argc, char** argv) {
  if (argc < 15) return 1;
  std::ifstream in(argv[2]);
  int n, stop, nl;
  float sensor_w;
  in >> n >> stop >> nl >> sensor_w;
  std::vector<float> radius(n), thick(n), semi(n), ior((size_t)n * nl);
  for (int k = 0; k < n; k++) {
    in >> radius[k] >> thick[k] >> semi[k];
    for (int l = 0; l < nl; l++) in >> ior[(size_t)l * n + k];
  }
  const size_t mw = atoi(argv[4]), mh = atoi(argv[5]), W = atoi(argv[6]), H = atoi(argv[7]);
  const int spp = atoi(argv[8]);
  const double lamp[3] = {atof(argv[9]), atof(argv[10]), atof(argv[11])};
  const float alpha = (float)atof(argv[12]);
  const std::string out = argv[13];
  const int wall = atoi(argv[14]);
  try {
    PathTracer pt(0);
    Camera cam;
    CameraApertureTexture ap;
    ap.init_from_texels(read_f32(argv[3], mw * mh).data(), mw, mh);
    cam.aperture_texture = &ap;
    cam.ghost_aperture_texture = &ap;
    pt.clear();
    pt.set_frame_size(W, H);
    pt.camera = &cam;
    pt.counter_jitter = true;
    pt.axis_ray = Vector2D(0.5, 0.5);
    const float ahead[3] = {0.0f, 0.0f, -1.0f};                      // (replaced by the scene's lamp at the frame)
    pt.use_geometric_ghosts(n, stop, nl, radius.data(), thick.data(), ior.data(), semi.data(), sensor_w, ahead, alpha, spp);
    // the lamp's direction s from the camera, two unit vectors u, v square to it
    const double ll = std::sqrt(lamp[0] * lamp[0] + lamp[1] * lamp[1] + lamp[2] * lamp[2]);
    const double s[3] = {lamp[0] / ll, lamp[1] / ll, lamp[2] / ll};
    double u[3] = {-s[2], 0.0, s[0]};                                // (s x y: the lamp is never along y here, z < 0)
    const double ul = std::sqrt(u[0] * u[0] + u[2] * u[2]);
    u[0] /= ul; u[2] /= ul;
    const double v[3] = {s[1] * u[2] - s[2] * u[1], s[2] * u[0] - s[0] * u[2], s[0] * u[1] - s[1] * u[0]};
    const double light[7] = {1.0, lamp[0], lamp[1], lamp[2], 1.0, 0.9, 0.5};   // a PointLight
    const double mats[4] = {0.0, 0.5, 0.5, 0.5};                     // diffuse grey
    if (wall) {
      const double dist = wall == 3 ? 2.0 * ll : 0.5 * ll, half = 0.4 * dist, shift = wall == 2 ? -half : 0.0;
      double c[4][3];
      const double cu[4] = {-half + shift, half + shift, half + shift, -half + shift}, cv[4] = {-half, -half, half, half};
      for (int i = 0; i < 4; i++)
        for (int a = 0; a < 3; a++) c[i][a] = dist * s[a] + cu[i] * u[a] + cv[i] * v[a];
      double pos[18], nrm[18];
      const int idx[6] = {0, 1, 2, 0, 2, 3};
      for (int i = 0; i < 6; i++)
        for (int a = 0; a < 3; a++) { pos[3 * i + a] = c[idx[i]][a]; nrm[3 * i + a] = -s[a]; }
      const int tri_mat[2] = {0, 0};
      pt.set_scene(0, nullptr, nullptr, 2, pos, nrm, tri_mat, 1, mats, 1, light);
      pt.use_ghost_occlusion(true);
      pt.use_ghost_occlusion_reach(LF_OCCLUSION_REACH_LIGHT);
    } else {
      const double sphere[4] = {0.0, 0.0, 10.0, 0.1};
      const int sphere_mat[1] = {0};
      pt.set_scene(1, sphere, sphere_mat, 0, nullptr, nullptr, nullptr, 1, mats, 1, light);
    }
    pt.use_lights_from_scene(alpha);
    pt.generate_ghost_buffer();
    dump(out + ".ghost.f64", &pt.ghost_buffer.data[0].x, W * H * 3);
    uint64_t st[2] = {0, 0};
    if (lf_get_ghost_occlusion_stats(pt.context(), st) != LF_OK) throw std::runtime_error(pt.last_error());
    printf("shadow tests %llu blocked %llu\n", (unsigned long long)st[0], (unsigned long long)st[1]);
  } catch (const std::exception& e) {
    fprintf(stderr, "shim_demo geolamp: %s\n", e.what());
    return 3;
  }
  return 0;
}

// shim_demo flarewall <aperture.f32> <aw> <ah> <ghost.f32> <gw> <gh> <W> <H> <hFov> <vFov> <flare ox oy> <outprefix>
//                     <wall: 0 none, 1 hides the sun, 2 its left half> [rays per flare]
// A wall in front of the sun, for the flare layer: the starburst, the falloff and the paraxial quads under
// PathTracer::use_flare_occlusion (no prescription: the shadow rays leave from the camera position, over a disc of the
// mirror's default angular radius, 0.05 rad).  One flare of radiance
// (1, 0.9, 0.5) at the normalised screen position <ox oy>; the wall is geowall's, a 2 m x 2 m quad 5 m from the camera
// (identity pose at the origin), square to the flare's direction and centred on it (1) or shifted so that its edge crosses
// it (2).  Dumps the sample, ghost and starburst buffers and prints the flare's visibility.
static int flarewall_main(int argc, char** argv) {
  if (argc < 16) return 1;
  const size_t aw = atoi(argv[3]), ah = atoi(argv[4]), gw = atoi(argv[6]), gh = atoi(argv[7]), W = atoi(argv[8]), H = atoi(argv[9]);
  const double hfov = atof(argv[10]), vfov = atof(argv[11]), ox = atof(argv[12]), oy = atof(argv[13]);
  const std::string out = argv[14];
  const int wall = atoi(argv[15]), rays = argc > 16 ? atoi(argv[16]) : 1024;
  try {
    PathTracer pt(0);
    Camera cam;
    cam.hFov = hfov; cam.vFov = vfov;
    CameraApertureTexture ap, gh_tex;
    ap.init_from_texels(read_f32(argv[2], aw * ah).data(), aw, ah);
    gh_tex.init_from_texels(read_f32(argv[5], gw * gh).data(), gw, gh);
    cam.aperture_texture = &ap;
    cam.ghost_aperture_texture = &gh_tex;
    pt.clear();
    pt.set_frame_size(W, H);
    pt.camera = &cam;
    pt.counter_jitter = true;
    pt.flare_radiance.emplace_back(1.0, 0.9, 0.5);
    pt.flare_origins.emplace_back(ox, oy);
    pt.axis_ray = Vector2D(ox, oy);
    pt.angle_to_sun = (float)std::atan(oy / ox);
    // the flare's direction s from the camera, two unit vectors u, v square to it
    const double PI_ = 3.14159265358979323;
    double s[3] = {(2.0 * ox - 1.0) * std::tan(0.5 * hfov * PI_ / 180.0), (2.0 * oy - 1.0) * std::tan(0.5 * vfov * PI_ / 180.0), -1.0};
    const double sl = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    for (int a = 0; a < 3; a++) s[a] /= sl;
    double u[3] = {-s[2], 0.0, s[0]};
    const double ul = std::sqrt(u[0] * u[0] + u[2] * u[2]);
    u[0] /= ul; u[2] /= ul;
    const double v[3] = {s[1] * u[2] - s[2] * u[1], s[2] * u[0] - s[0] * u[2], s[0] * u[1] - s[1] * u[0]};
    const double mats[4] = {0.0, 0.5, 0.5, 0.5};                     // diffuse grey
    if (wall) {
      const double shift = wall == 2 ? -1.0 : 0.0, dist = 5.0;
      double c[4][3];
      const double cu[4] = {-1.0 + shift, 1.0 + shift, 1.0 + shift, -1.0 + shift}, cv[4] = {-1.0, -1.0, 1.0, 1.0};
      for (int i = 0; i < 4; i++)
        for (int a = 0; a < 3; a++) c[i][a] = dist * s[a] + cu[i] * u[a] + cv[i] * v[a];
      double pos[18], nrm[18];
      const int idx[6] = {0, 1, 2, 0, 2, 3};
      for (int i = 0; i < 6; i++)
        for (int a = 0; a < 3; a++) { pos[3 * i + a] = c[idx[i]][a]; nrm[3 * i + a] = -s[a]; }
      const int tri_mat[2] = {0, 0};
      pt.set_scene(0, nullptr, nullptr, 2, pos, nrm, tri_mat, 1, mats, 0, nullptr);
      pt.use_flare_occlusion(true, rays);
    }
    pt.generate_ghost_buffer();
    std::vector<double> sample(W * H * 3), star(W * H * 3);
    if (lf_read_tile(pt.context(), 0, 0, 0, (int)W, (int)H, sample.data(), 3) != LF_OK ||
        lf_read_tile(pt.context(), 2, 0, 0, (int)W, (int)H, star.data(), 3) != LF_OK)
      throw std::runtime_error(pt.last_error());
    dump(out + ".sample.f64", sample.data(), sample.size());
    dump(out + ".star.f64", star.data(), star.size());
    dump(out + ".ghost.f64", &pt.ghost_buffer.data[0].x, W * H * 3);
    if (wall) {
      int n = 0;
      double vis[LF_MAX_FLARES];
      uint64_t cnt[LF_MAX_FLARES];
      if (lf_get_flare_visibility(pt.context(), &n, vis, cnt) != LF_OK) throw std::runtime_error(pt.last_error());
      for (int k = 0; k < n; k++) printf("flare %d visibility %.17g visible rays %llu of %d\n", k, vis[k], (unsigned long long)cnt[k], rays);
    }
  } catch (const std::exception& e) {
    fprintf(stderr, "shim_demo flarewall: %s\n", e.what());
    return 3;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "flarewall") return flarewall_main(argc, argv);
  if (argc > 1 && std::string(argv[1]) == "geo") return geo_main(argc, argv);
  if (argc > 1 && std::string(argv[1]) == "geolamp") return geolamp_main(argc, argv);
  if (argc > 1 && std::string(argv[1]) == "geowall") return geowall_main(argc, argv);
  if (argc > 1 && std::string(argv[1]) == "geolights") return geolights_main(argc, argv);
  if (argc < 5) return 1;
  std::ifstream in(argv[1]);
  size_t W, H, ns_aa, aw, ah, gw, gh, n_lights;
  double radius, intensity;
  Camera cam;
  in >> W >> H >> ns_aa >> radius >> intensity >> cam.hFov >> cam.vFov;
  in >> cam.pos.x >> cam.pos.y >> cam.pos.z;
  for (int i = 0; i < 9; i++) in >> cam.c2w[i];
  in >> aw >> ah >> gw >> gh >> n_lights;
  std::string out = argv[4];
  int n_threads = argc > 5 ? atoi(argv[5]) : 4;
  try {
    PathTracer pt(0);
    for (size_t l = 0; l < n_lights; l++) {
      DirectionalLight d;
      in >> d.posLight.x >> d.posLight.y >> d.posLight.z >> d.radiance.x >> d.radiance.y >> d.radiance.z;
      pt.lights.push_back(d);
    }
    CameraApertureTexture ap, gh_tex;
    ap.init_from_texels(read_f32(argv[2], aw * ah).data(), aw, ah);
    gh_tex.init_from_texels(read_f32(argv[3], gw * gh).data(), gw, gh);
    cam.aperture_texture = &ap;
    cam.ghost_aperture_texture = &gh_tex;

    // ---- start_raytracing (raytraced_renderer.cpp:300-311) ----
    pt.clear();
    pt.set_frame_size(W, H);
    pt.camera = &cam;
    pt.ns_aa = ns_aa;
    pt.flare_radius = radius;
    pt.flare_intensity = intensity;
    pt.flare_origins.clear();
    pt.flare_radiance.clear();
    pt.find_sun_pos();
    pt.generate_ghost_buffer();

    // ---- tile queue + worker threads (:314-328, :352-354, :681-715) ----
    ImageBuffer fb(W, H);
    struct Tile { size_t x0, y0, x1, y1; };
    std::vector<Tile> tiles;
    const size_t T = 32;
    for (size_t y = 0; y < H; y += T)
      for (size_t x = 0; x < W; x += T) tiles.push_back({x, y, std::min(x + T, W), std::min(y + T, H)});
    std::vector<std::thread> workers;
    for (int t = 0; t < n_threads; t++)
      workers.emplace_back([&, t]() {
        for (size_t i = t; i < tiles.size(); i += n_threads) {
          const Tile& tl = tiles[i];
          for (size_t y = tl.y0; y < tl.y1; y++)
            for (size_t x = tl.x0; x < tl.x1; x++) pt.raytrace_pixel(x, y);   // raytrace_tile :637-641
          pt.write_to_framebuffer(fb, tl.x0, tl.y0, tl.x1, tl.y1);            // :646
        }
      });
    for (auto& w : workers) w.join();

    dump(out + ".sample.f64", &pt.sampleBuffer.data[0].x, W * H * 3);
    dump(out + ".ghost.f64", &pt.ghost_buffer.data[0].x, W * H * 3);
    dump(out + ".rgba.u32", fb.data.data(), W * H);
    FILE* f = fopen((out + ".flares.txt").c_str(), "w");
    fprintf(f, "%zu %a %a %a\n", pt.flare_origins.size(), pt.axis_ray.x, pt.axis_ray.y, (double)pt.angle_to_sun);
    for (size_t k = 0; k < pt.flare_origins.size(); k++)
      fprintf(f, "%a %a %a %a %a\n", pt.flare_origins[k].x, pt.flare_origins[k].y, pt.flare_radiance[k].x,
              pt.flare_radiance[k].y, pt.flare_radiance[k].z);
    fprintf(f, "aperture_bbox %d %d %d %d %a\n", ap.min_x, ap.min_y, ap.max_x, ap.max_y, ap.total_value);
    fclose(f);
    Ray r = cam.generate_ray(0.5, 0.5);
    printf("centre ray d = (%g, %g, %g)\n", r.d.x, r.d.y, r.d.z);
  } catch (const std::exception& e) {
    fprintf(stderr, "shim_demo: %s\n", e.what());
    return 3;
  }
  return 0;
}
