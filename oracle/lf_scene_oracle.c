/* TEST INFRASTRUCTURE -- CPU restatement of the scene-radiance term of PathTracer::raytrace_pixel
 * (SURVEY.md section 8 row f2).  Never linked into, imported by or shipped with the product.
 *
 * Follows, expression by expression (CGL::Vector3D operator order included):
 *   the sample loop                         src/pathtracer/pathtracer.cpp:831-875
 *   Camera::generate_ray                    src/pathtracer/camera.cpp:278-305
 *   Sphere::test / intersect                src/scene/sphere.cpp:11-111
 *   moller_trumbore / Triangle::intersect   src/scene/triangle.cpp:25-112
 *   est_radiance_global_illumination        src/pathtracer/pathtracer.cpp:282-302
 *   estimate_direct_lighting_importance     src/pathtracer/pathtracer.cpp:142-213
 *   make_coord_space, DiffuseBSDF::f        src/pathtracer/bsdf.cpp:21-60
 *   DirectionalLight / PointLight::sample_L src/scene/light.cpp:18-24, :52-60
 * The closest hit is found by brute force over the primitives (the reference's BVH only prunes).
 * PARITY STATUS: pinned -- tests/test_oracle_vs_reference.py checks it against frames rendered by
 * the real reference from programmatic scenes (tests/golden/s*.npz).  The sampled lights (second half of
 * this file: area, hemisphere and environment lights, the -H estimator) are pinned as well, draw for
 * draw: the same test file reproduces the single-threaded reference renders of tests/golden/a48x36*,
 * h48x36*, e48x36_envlight and s48x36*_hsample from one MT19937 consumed in the reference's order.
 */
#define _GNU_SOURCE
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "lf_oracle.h"

typedef struct { double x, y, z; } v3;
static v3 V(double x, double y, double z) { v3 r = {x, y, z}; return r; }
static v3 add(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
static v3 sub(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static v3 scl(v3 a, double c) { return V(a.x * c, a.y * c, a.z * c); }     /* Vector3D * double */
static v3 lscl(double c, v3 a) { return V(c * a.x, c * a.y, c * a.z); }    /* double * Vector3D */
static v3 mulv(v3 a, v3 b) { return V(a.x * b.x, a.y * b.y, a.z * b.z); }
static double dot(v3 a, v3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; } /* AVX: dp(x,y) + z */
static v3 cross(v3 u, v3 v) { return V(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x); }
static double norm(v3 a) { return sqrt(dot(a, a)); }
static v3 unit(v3 a) { double rn = 1. / norm(a); return scl(a, rn); }
static v3 divs(v3 a, double c) { double rc = 1.0 / c; return V(rc * a.x, rc * a.y, rc * a.z); }

typedef struct { v3 o, d; double min_t, max_t; } ray;
typedef struct { double t; v3 n; int mat; } isect;

typedef struct {
  int n_spheres; const double* spheres; const int* sph_mat;
  int n_tris; const double* tri_pos; const double* tri_nrm; const int* tri_mat;
  const double* materials; int n_lights; const double* lights;
} scene_t;

static int hit_sphere(const double* s, int mat, ray* r, isect* h) {
  v3 c = V(s[0], s[1], s[2]);
  double r2 = s[3] * s[3];
  v3 oc = sub(r->o, c);
  double a = dot(r->d, r->d), b = 2 * dot(oc, r->d), cc = dot(oc, oc) - r2, t1;
  if (b * b < 4.0 * a * cc) return 0;
  if (b * b == 4.0 * a * cc) {
    double root = (-b) / (2.0 * a);
    if (root < r->min_t || root > r->max_t) return 0;
    t1 = root;
  } else {
    double q = sqrt(b * b - 4.0 * a * cc);
    double r1 = (-b - q) / (2.0 * a), r2_ = (-b + q) / (2.0 * a);
    double p1 = r2_ < r1 ? r2_ : r1, p2 = r1 < r2_ ? r2_ : r1;
    if (p1 > r->max_t || p2 < r->min_t) return 0;
    if (p1 < r->min_t) { if (p2 > r->max_t) return 0; t1 = p2; } else t1 = p1;
  }
  r->max_t = t1;
  if (h) { h->t = t1; h->n = unit(sub(add(r->o, lscl(t1, r->d)), c)); h->mat = mat; }
  return 1;
}

static int hit_tri(const double* P, const double* N, int mat, ray* r, isect* h) {
  v3 p0 = V(P[0], P[1], P[2]), p1 = V(P[3], P[4], P[5]), p2 = V(P[6], P[7], P[8]);
  v3 e1 = sub(p1, p0), e2 = sub(p2, p0), s = sub(r->o, p0);
  v3 s1 = cross(r->d, e2), s2 = cross(s, e1);
  double rc = 1. / dot(s1, e1);
  double t = dot(s2, e2) * rc, b1 = dot(s1, s) * rc, b2 = dot(s2, r->d) * rc;
  if (t < r->min_t || t > r->max_t) return 0;
  if (b1 < 0 || b1 > 1) return 0;
  if (b2 < 0 || b2 > 1) return 0;
  if (b1 + b2 > 1) return 0;
  r->max_t = t;
  if (h) {
    double b0 = 1 - b1 - b2;
    v3 n1 = V(N[0], N[1], N[2]), n2 = V(N[3], N[4], N[5]), n3 = V(N[6], N[7], N[8]);
    h->t = t; h->n = unit(add(add(lscl(b0, n1), lscl(b1, n2)), lscl(b2, n3))); h->mat = mat;
  }
  return 1;
}

static int closest(const scene_t* S, ray* r, isect* h) {
  int any = 0;
  for (int i = 0; i < S->n_spheres; i++) any |= hit_sphere(S->spheres + 4 * i, S->sph_mat[i], r, h);
  for (int i = 0; i < S->n_tris; i++) any |= hit_tri(S->tri_pos + 9 * i, S->tri_nrm + 9 * i, S->tri_mat[i], r, h);
  return any;
}

static v3 radiance(const scene_t* S, ray r) {
  isect is;
  if (!closest(S, &r, &is)) return V(0, 0, 0);
  const double* m = S->materials + 4 * is.mat;
  v3 emission = m[0] == 1.0 ? V(m[1], m[2], m[3]) : V(0, 0, 0);
  /* make_coord_space */
  v3 z = is.n, hh = is.n;
  if (fabs(hh.x) <= fabs(hh.y) && fabs(hh.x) <= fabs(hh.z)) hh.x = 1.0;
  else if (fabs(hh.y) <= fabs(hh.x) && fabs(hh.y) <= fabs(hh.z)) hh.y = 1.0;
  else hh.z = 1.0;
  z = scl(z, 1. / norm(z));
  v3 y = cross(hh, z); y = scl(y, 1. / norm(y));
  v3 x = cross(z, y); x = scl(x, 1. / norm(x));
  v3 hit_p = add(r.o, scl(r.d, is.t));
  v3 L = V(0, 0, 0);
  const double eps = (double)0.00001f;
  for (int l = 0; l < S->n_lights; l++) {
    const double* lt = S->lights + 7 * l;
    v3 wi; double dist;
    if (lt[0] == 0.0) { wi = V(lt[1], lt[2], lt[3]); dist = INFINITY; }
    else { v3 d = sub(V(lt[1], lt[2], lt[3]), hit_p); wi = unit(d); dist = norm(d); }
    v3 wo = V((wi.x * x.x + wi.y * x.y) + wi.z * x.z, (wi.x * y.x + wi.y * y.y) + wi.z * y.z,
              (wi.x * z.x + wi.y * z.y) + wi.z * z.z);
    if (wo.z < 0) continue;
    ray sh = {hit_p, wi, eps, dist - eps};
    if (!closest(S, &sh, NULL)) {
      double cos_theta = unit(wo).z;
      double ipi = 1.0 / 3.14159265358979323;
      v3 f = m[0] == 0.0 ? mulv(V(ipi, ipi, ipi), V(m[1], m[2], m[3])) : V(0, 0, 0);
      L = add(L, divs(scl(mulv(f, V(lt[4], lt[5], lt[6])), cos_theta), 1.0));
    }
  }
  if (S->n_lights > 0) L = divs(L, (double)S->n_lights);
  return add(emission, L);
}

/* scene: W*H*3 doubles; visited pixels get the averaged radiance (sum / loop variable).  Draws per
 * visited pixel: 2*ns_aa (consumed here) + 32 (falloff), one std::mt19937 in visit order. */
void lfo_scene_term(int W, int H, int ns_aa, int samples_per_batch, double max_tol,
                    const double c2w[9], const double pos[3], double hfov, double vfov, double nclip,
                    double fclip, int n_spheres, const double* spheres, const int* sph_mat, int n_tris,
                    const double* tri_pos, const double* tri_nrm, const int* tri_mat,
                    const double* materials, int n_lights, const double* lights,
                    const uint32_t* order, size_t n_order, uint32_t seed, double* scene) {
  scene_t S = {n_spheres, spheres, sph_mat, n_tris, tri_pos, tri_nrm, tri_mat, materials, n_lights, lights};
  size_t per = 2 * (size_t)ns_aa + 32;
  uint32_t* raw = (uint32_t*)malloc(sizeof(uint32_t) * per * n_order);
  lfo_mt19937_raw(seed, 0, per * n_order, raw);
  const double PI_ = 3.14159265358979323;
  double edge_x = tan(0.5 * (hfov * (PI_ / 180.0))), edge_y = tan(0.5 * (vfov * (PI_ / 180.0)));
  for (size_t v = 0; v < n_order; v++) {
    size_t p = order[v];
    int px = (int)(p % (size_t)W), py = (int)(p / (size_t)W);
    const uint32_t* rw = raw + per * v;
    v3 total = V(0, 0, 0);
    float s1 = 0.0f, s2 = 0.0f;
    int sample;
    for (sample = 1; sample <= ns_aa; sample++) {
      /* first draw -> y (g++ evaluates Vector2D(random_uniform(), random_uniform()) right to left) */
      double sy = (double)py + lfo_random_uniform_from_raw(rw[2 * (sample - 1)]);
      double sx = (double)px + lfo_random_uniform_from_raw(rw[2 * (sample - 1) + 1]);
      double nx = sx / (double)W, ny = sy / (double)H;
      v3 dir = unit(V(edge_x * (2 * nx - 1), edge_y * (2 * ny - 1), -1));
      ray r;
      r.o = V(pos[0], pos[1], pos[2]);
      r.d = V((dir.x * c2w[0] + dir.y * c2w[1]) + dir.z * c2w[2], (dir.x * c2w[3] + dir.y * c2w[4]) + dir.z * c2w[5],
              (dir.x * c2w[6] + dir.y * c2w[7]) + dir.z * c2w[8]);
      r.min_t = nclip; r.max_t = fclip;
      v3 L = radiance(&S, r);
      float illum = (float)((0.2126f * L.x + 0.7152f * L.y) + 0.0722f * L.z);
      s1 += illum; s2 += illum * illum;
      total = add(total, L);
      if (sample > 1 && sample % samples_per_batch == 0) {
        float sd = (float)sqrt(1.0 / (sample - 1) * (double)(s2 - s1 * s1 / (float)sample));
        float ci = (float)(1.96 * (double)sd / sqrt((double)sample));
        if ((double)ci <= max_tol * (double)s1 / (double)sample) break;
      }
    }
    double rc = 1. / (double)sample;
    scene[3 * p] = total.x * rc; scene[3 * p + 1] = total.y * rc; scene[3 * p + 2] = total.z * rc;
  }
  free(raw);
}

/* est_radiance_global_illumination (pathtracer.cpp:282-302) for explicit rays: what the sample loop adds
 * for a camera ray, whoever generated it (the lens camera's exit rays, tests/test_gpu_lens_camera.py).
 * rays: n x 8 doubles {o xyz, d xyz, min_t, max_t}; rgb: n x 3 */
void lfo_scene_radiance_rays(int n_spheres, const double* spheres, const int* sph_mat, int n_tris,
                             const double* tri_pos, const double* tri_nrm, const int* tri_mat,
                             const double* materials, int n_lights, const double* lights, size_t n_rays,
                             const double* rays, double* rgb) {
  scene_t S = {n_spheres, spheres, sph_mat, n_tris, tri_pos, tri_nrm, tri_mat, materials, n_lights, lights};
  for (size_t i = 0; i < n_rays; i++) {
    const double* q = rays + 8 * i;
    ray r = {V(q[0], q[1], q[2]), V(q[3], q[4], q[5]), q[6], q[7]};
    v3 L = radiance(&S, r);
    rgb[3 * i] = L.x; rgb[3 * i + 1] = L.y; rgb[3 * i + 2] = L.z;
  }
}

/* ==========================================================================================
 * Sampled lights: the whole direct-lighting integrator, draw for draw.
 *
 *   AreaLight::AreaLight / sample_L                 src/scene/light.cpp:76-94
 *   InfiniteHemisphereLight (ctor, sample_L)        src/scene/light.cpp:28-43
 *   UniformGridSampler2D::get_sample                src/pathtracer/sampler.cpp:8-12
 *   UniformHemisphereSampler3D::get_sample          src/pathtracer/sampler.cpp:30-44
 *   EnvironmentLight::init                          src/scene/environment_light.cpp:18-60
 *   theta_phi_to_xy .. theta_phi_to_dir, bilerp     src/scene/environment_light.cpp:88-140
 *   EnvironmentLight::sample_L / sample_dir         src/scene/environment_light.cpp:143-182
 *   estimate_direct_lighting_hemisphere             src/pathtracer/pathtracer.cpp:86-140
 *   estimate_direct_lighting_importance             src/pathtracer/pathtracer.cpp:142-213
 *   zero_bounce / one_bounce_radiance               src/pathtracer/pathtracer.cpp:215-232
 *   Matrix3x3 * Vector3D                            CGL/src/matrix3x3.cpp:110-114
 *
 * Every random number comes from a draw source with two implementations:
 *   (a) the reference's: ONE std::mt19937 consumed strictly in order (pixel jitter, then whatever the
 *       hit draws, sample after sample, then the pixel's 32 falloff draws) -- pinned to frames the real
 *       reference rendered single-threaded (tests/test_oracle_vs_reference.py);
 *   (b) the device's: Philox4x32-10 of an explicit counter:
 *         light sample k of light l    (c.x, c.y, 0x11640000 + l, k)
 *         -H direction k               (c.x, c.y, 0x11650000, k)
 *         pixel jitter                 (p, sample, 0x5ce4e000, 0)
 *       with (c.x, c.y) = (pixel index, sample number) in a frame and whatever the caller says for
 *       explicit rays; a draw pair is words 0 and 1 of the block.
 * In (b) every evaluation is repeated with origin, direction and draws moved by +-1e-12 relative: a
 * result that moves by more than 1e-9 hangs on a discrete decision (an edge, a sign, a table bin, a float
 * cast) that one ulp of libm can flip, and is reported as fragile.
 * ========================================================================================== */
typedef struct {
  int n_spheres; const double* spheres; const int* sph_mat;
  int n_tris; const double* tri_pos; const double* tri_nrm; const int* tri_mat;
  const double* materials;            /* 4 per material: kind (0 diffuse, 1 emission, 2 f given), rgb */
  int n_lights; const double* lights; /* 16 per light: type, rgb, v, dir, dim_x, dim_y (lf_set_scene_lights) */
  int ns_area_light, hemisphere;
  int env_w, env_h; const double* env; /* h x w x 3, or NULL */
} lfo_scene_desc;

typedef struct { int w, h; const double* data; double *pdf, *conds, *marg; } env_t;

static const double PI_ = 3.14159265358979323846;   /* PI (CGL/include/CGL/misc.h) */

/* EnvironmentLight::init (environment_light.cpp:18-60); illum() returns a float (vector3D.h:231-233) */
static void env_init(env_t* E, int w, int h, const double* data) {
  E->w = w; E->h = h; E->data = data; E->pdf = E->conds = E->marg = NULL;
  if (!data || !w) { E->w = E->h = 0; return; }
  size_t n = (size_t)w * h;
  E->pdf = (double*)malloc(sizeof(double) * n);
  E->conds = (double*)malloc(sizeof(double) * n);
  E->marg = (double*)malloc(sizeof(double) * (size_t)h);
  double sum = 0;
  for (int j = 0; j < h; ++j)
    for (int i = 0; i < w; ++i) {
      const double* t = data + 3 * ((size_t)w * j + i);
      float illum = (float)((0.2126f * t[0] + 0.7152f * t[1]) + 0.0722f * t[2]);
      E->pdf[(size_t)w * j + i] = illum * sin(PI_ * (j + .5) / (uint32_t)h);
      sum += E->pdf[(size_t)w * j + i];
    }
  for (int j = 0; j < h; ++j)
    for (int i = 0; i < w; ++i) E->pdf[(size_t)w * j + i] /= sum;
  for (int j = 0; j < h; ++j) {
    E->marg[j] = (j == 0 ? 0 : E->marg[j - 1]);
    for (int i = 0; i < w; ++i) E->marg[j] += E->pdf[(size_t)w * j + i];
  }
  for (int j = 0; j < h; ++j) {
    double marginal_density = E->marg[j] - (j == 0 ? 0 : E->marg[j - 1]);
    for (int i = 0; i < w; ++i)
      E->conds[(size_t)w * j + i] = (i == 0 ? 0 : E->conds[(size_t)w * j + i - 1]) + E->pdf[(size_t)w * j + i] / marginal_density;
  }
}
static void env_free(env_t* E) { free(E->pdf); free(E->conds); free(E->marg); }

static v3 env_px(const env_t* E, long i) { return V(E->data[3 * i], E->data[3 * i + 1], E->data[3 * i + 2]); }

/* sample_dir (:173-182) = bilerp(theta_phi_to_xy(dir_to_theta_phi(r.d))) */
static v3 env_sample_dir(const env_t* E, v3 d) {
  v3 u = unit(d);
  double theta = acos(u.y), phi = atan2(-u.z, u.x) + PI_;          /* :104-109 */
  double x = phi / 2. / PI_ * (uint32_t)E->w, y = theta / PI_ * (uint32_t)E->h;   /* :88-93 */
  long right = lround(x), left, v = lround(y);                     /* :123-140 */
  double u1 = right - x + .5, v1;
  if (right == 0 || right == E->w) { left = E->w - 1; right = 0; } else left = right - 1;
  if (v == 0) { v = 1; v1 = 1; } else if (v == E->h) { v = E->h - 1; v1 = 0; } else v1 = v - y + .5;
  long bottom = (long)E->w * v, top = bottom - E->w;
  double u0 = 1 - u1;
  return add(scl(add(scl(env_px(E, top + left), u1), scl(env_px(E, top + right), u0)), v1),
             scl(add(scl(env_px(E, bottom + left), u1), scl(env_px(E, bottom + right), u0)), 1 - v1));
}

/* std::upper_bound: the first element greater than x */
static size_t upper_bound(const double* a, size_t n, double x) {
  size_t first = 0, len = n;
  while (len > 0) {
    size_t half = len >> 1;
    if (x < a[first + half]) len = half; else { first += half + 1; len -= half + 1; }
  }
  return first;
}

void geo_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);   /* lf_geo_oracle.c */

typedef struct {
  int counter;              /* 0: the reference's stream, 1: the device's counters */
  lfo_mt* mt; uint64_t pos; /* (a): the generator and how many draws it has handed out */
  uint32_t cx, cy, key[2];  /* (b) */
  double eps;               /* (b): relative shift of every draw, for the fragility variants */
} draws_t;

/* two consecutive random_uniform() values: first, second */
static void draw_pair(draws_t* D, uint32_t stream, uint32_t k, double* first, double* second) {
  if (!D->counter) {
    *first = lfo_random_uniform_from_raw(lfo_mt_draw(D->mt));
    *second = lfo_random_uniform_from_raw(lfo_mt_draw(D->mt));
    D->pos += 2;
    return;
  }
  uint32_t ctr[4] = {D->cx, D->cy, stream, k}, out[4];
  geo_philox(ctr, D->key, out);
  *first = lfo_random_uniform_from_raw(out[0]) * (1 + D->eps);
  *second = lfo_random_uniform_from_raw(out[1]) * (1 - D->eps);
}
/* UniformGridSampler2D::get_sample (sampler.cpp:8-12): Vector2D(random_uniform(), random_uniform()) -- g++
 * evaluates the arguments right to left, the reference's FIRST draw is y.  The device's block is (x, y). */
static void draw_grid(draws_t* D, uint32_t stream, uint32_t k, double* x, double* y) {
  if (!D->counter) draw_pair(D, stream, k, y, x); else draw_pair(D, stream, k, x, y);
}
/* UniformHemisphereSampler3D::get_sample (sampler.cpp:30-44): sinf / cosf take the double angles as floats
 * and their products are float products */
static v3 draw_hemisphere(draws_t* D, uint32_t stream, uint32_t k) {
  double Xi1, Xi2;
  draw_pair(D, stream, k, &Xi1, &Xi2);
  double theta = acos(Xi1);
  double phi = 2.0 * PI_ * Xi2;
  double xs = sinf((float)theta) * cosf((float)phi);
  double ys = sinf((float)theta) * sinf((float)phi);
  double zs = cosf((float)theta);
  return V(xs, ys, zs);
}
/* Matrix3x3 * Vector3D (matrix3x3.cpp:110-114): x.x * col0 + x.y * col1 + x.z * col2 */
static v3 mat_mul(v3 c0, v3 c1, v3 c2, v3 x) { return add(add(lscl(x.x, c0), lscl(x.y, c1)), lscl(x.z, c2)); }

enum { kStreamLight = 0x11640000u, kStreamHemi = 0x11650000u, kStreamJitter = 0x5ce4e000u };

/* what: bit 0 zero_bounce_radiance, bit 1 one_bounce_radiance; m = {kind, rgb} */
static v3 shade(const lfo_scene_desc* Q, const scene_t* S, const env_t* E, int hemisphere, ray r, double t,
                v3 n, const double* m, int what, draws_t* D) {
  v3 emission = (m[0] == 1.0 && (what & 1)) ? V(m[1], m[2], m[3]) : V(0, 0, 0);   /* get_emission (:219) */
  if (!(what & 2)) return emission;
  /* make_coord_space (bsdf.cpp:21-41): o2w columns x, y, z; w2o = o2w.T() */
  v3 z = n, hh = n;
  if (fabs(hh.x) <= fabs(hh.y) && fabs(hh.x) <= fabs(hh.z)) hh.x = 1.0;
  else if (fabs(hh.y) <= fabs(hh.x) && fabs(hh.y) <= fabs(hh.z)) hh.y = 1.0;
  else hh.z = 1.0;
  z = scl(z, 1. / norm(z));
  v3 y = cross(hh, z); y = scl(y, 1. / norm(y));
  v3 x = cross(z, y); x = scl(x, 1. / norm(x));
  v3 t0 = V(x.x, y.x, z.x), t1 = V(x.y, y.y, z.y), t2 = V(x.z, y.z, z.z);   /* columns of w2o */
  v3 hit_p = add(r.o, scl(r.d, t));
  const double eps = (double)0.00001f;   /* EPS_F */
  double ipi = 1.0 / PI_;
  /* DiffuseBSDF::f (bsdf.cpp:52-61), EmissionBSDF::f = 0 (:89-91); kind 2: f handed over as it is */
  v3 f = m[0] == 0.0 ? mulv(V(ipi, ipi, ipi), V(m[1], m[2], m[3])) : m[0] == 2.0 ? V(m[1], m[2], m[3]) : V(0, 0, 0);
  v3 L = V(0, 0, 0);
  if (hemisphere) {   /* pathtracer.cpp:86-140 */
    int num_samples = Q->n_lights * Q->ns_area_light;
    double p_w = 1.0 / (2.0 * PI_);
    for (int i = 0; i < num_samples; i++) {
      v3 wi = draw_hemisphere(D, kStreamHemi, (uint32_t)i);
      v3 wiw = mat_mul(x, y, z, wi);
      ray out = {hit_p, wiw, eps, INFINITY};
      isect is2;
      if (closest(S, &out, &is2)) {
        double cos_theta_out = unit(wi).z;
        const double* m2 = Q->materials + 4 * is2.mat;
        v3 em2 = m2[0] == 1.0 ? V(m2[1], m2[2], m2[3]) : V(0, 0, 0);
        L = add(L, divs(scl(mulv(f, em2), cos_theta_out), p_w));
      }
    }
    return add(emission, divs(L, (double)num_samples));
  }
  int total_samples = 0;   /* pathtracer.cpp:142-213 */
  for (int l = 0; l < Q->n_lights; l++) {
    const double* lt = Q->lights + 16 * l;
    int type = (int)lt[0];
    v3 rad = V(lt[1], lt[2], lt[3]), lv = V(lt[4], lt[5], lt[6]);
    int num_samples = type <= 1 ? 1 : Q->ns_area_light;   /* is_delta_light(): directional and point */
    total_samples += num_samples;
    for (int i = 0; i < num_samples; i++) {
      v3 wi, em = rad;
      double dist, pdf;
      if (type == 0) { wi = lv; dist = INFINITY; pdf = 1.0; }                              /* light.cpp:18-24 */
      else if (type == 1) { v3 d = sub(lv, hit_p); wi = unit(d); dist = norm(d); pdf = 1.0; } /* :50-58 */
      else if (type == 2) {                                                                /* :28-43 */
        v3 dir = draw_hemisphere(D, kStreamLight + (uint32_t)l, (uint32_t)i);
        wi = mat_mul(V(1, 0, 0), V(0, 0, -1), V(0, 1, 0), dir);
        dist = INFINITY;
        pdf = 1.0 / (2.0 * PI_);
      } else if (type == 3) {                                                              /* :76-94 */
        v3 ldir = V(lt[7], lt[8], lt[9]), dim_x = V(lt[10], lt[11], lt[12]), dim_y = V(lt[13], lt[14], lt[15]);
        double area = norm(dim_x) * norm(dim_y);
        double sx, sy;
        draw_grid(D, kStreamLight + (uint32_t)l, (uint32_t)i, &sx, &sy);
        sx = sx - (double)0.5f; sy = sy - (double)0.5f;
        v3 d = sub(add(add(lv, lscl(sx, dim_x)), lscl(sy, dim_y)), hit_p);
        double cosTheta = dot(d, ldir);
        double sqDist = dot(d, d);
        dist = sqrt(sqDist);
        wi = divs(d, dist);
        pdf = sqDist / (area * fabs(cosTheta));
        em = cosTheta < 0 ? rad : V(0, 0, 0);
      } else {                                                                             /* environment_light.cpp:159-170 */
        double sx, sy;
        draw_grid(D, kStreamLight + (uint32_t)l, (uint32_t)i, &sx, &sy);
        size_t yy = upper_bound(E->marg, (size_t)E->h, sy);
        if (yy >= (size_t)E->h) yy = (size_t)E->h - 1;   /* (one past the end in the reference: out of bounds there) */
        size_t xx = upper_bound(E->conds + (size_t)E->w * yy, (size_t)E->w, sx);
        if (xx >= (size_t)E->w) xx = (size_t)E->w - 1;
        double phi = (double)xx / (uint32_t)E->w * 2.0 * PI_;      /* xy_to_theta_phi :95-102 */
        double theta = (double)yy / (uint32_t)E->h * PI_;
        double dy = cos(theta);                                    /* theta_phi_to_dir :111-120 */
        double dx = cos(phi - PI_) * sin(theta);
        double dz = -sin(phi - PI_) * sin(theta);
        wi = V(dx, dy, dz);
        dist = INFINITY;
        pdf = E->pdf[(size_t)E->w * yy + xx] * (uint32_t)E->w * (uint32_t)E->h / 2. / PI_ / PI_ / sin(theta);
        em = env_px(E, (long)((size_t)E->w * yy + xx));
      }
      v3 wo = mat_mul(t0, t1, t2, wi);
      if (wo.z < 0) continue;                 /* dot(w, (0,0,1)) < 0 */
      ray sh = {hit_p, wi, eps, dist - eps};
      if (!closest(S, &sh, NULL)) {
        double cos_theta_out = unit(wo).z;
        L = add(L, divs(scl(mulv(f, em), cos_theta_out), pdf));
      }
    }
  }
  if (total_samples > 0) L = divs(L, (double)total_samples);   /* (as radiance() above: no light, no division) */
  return add(emission, L);
}

/* est_radiance_global_illumination (pathtracer.cpp:282-302) */
static v3 radiance_s(const lfo_scene_desc* Q, const scene_t* S, const env_t* E, ray r, draws_t* D, isect* hit,
                     int* did_hit) {
  isect is;
  int h = closest(S, &r, &is);
  if (did_hit) *did_hit = h;
  if (!h) return E->w ? env_sample_dir(E, r.d) : V(0, 0, 0);
  if (hit) *hit = is;
  return shade(Q, S, E, Q->hemisphere, r, is.t, is.n, Q->materials + 4 * is.mat, 3, D);
}

static scene_t geometry_of(const lfo_scene_desc* Q) {
  scene_t S = {Q->n_spheres, Q->spheres, Q->sph_mat, Q->n_tris, Q->tri_pos, Q->tri_nrm, Q->tri_mat, Q->materials, 0, NULL};
  return S;
}

/* the fragility variants: origin, direction (and, through D->eps, the draws) moved by e relative */
static ray shifted(ray r, double e) {
  r.o = V(r.o.x * (1 - e), r.o.y * (1 + e), r.o.z * (1 - e));
  r.d = V(r.d.x * (1 + e), r.d.y * (1 - e), r.d.z * (1 + e));
  return r;
}
static int moved1(double a, double b) {
  if (isnan(a) && isnan(b)) return 0;
  return !(fabs(a - b) <= 1e-9 * fabs(a));
}
static int moved(v3 a, v3 b) { return moved1(a.x, b.x) || moved1(a.y, b.y) || moved1(a.z, b.z); }
static const double kShift = 1e-12;

/* the sample loop (pathtracer.cpp:831-875) over the pixels of `order`.
 * counter = 0: one MT19937 (seed, `skip` draws thrown away first) in visit order; stream_pos[v] = draws
 *   handed out when visit v's 32 falloff draws begin (they are skipped here; lfo_render_pixels reads them).
 * counter = 1: the device's counters under `key`; flags[p] bit 0 = a sample of the pixel is fragile, bit 1 =
 *   an early-out comparison was closer than 1e-6 relative.
 * n_samples[p] = the loop variable at the end (ns_aa + 1 when the loop ran out). */
void lfo_scene_frame(const lfo_scene_desc* Q, int W, int H, int ns_aa, int samples_per_batch, double max_tol,
                     const double c2w[9], const double pos[3], double hfov, double vfov, double nclip, double fclip,
                     const uint32_t* order, size_t n_order, int counter, uint32_t seed, size_t skip, uint64_t key,
                     double* scene, uint64_t* stream_pos, uint8_t* flags, int* n_samples) {
  scene_t S = geometry_of(Q);
  env_t E;
  env_init(&E, Q->env_w, Q->env_h, Q->env);
  draws_t D = {counter, NULL, (uint64_t)skip, 0, 0, {(uint32_t)key, (uint32_t)(key >> 32)}, 0.0};
  if (!counter) D.mt = lfo_mt_open(seed, skip);
  double edge_x = tan(0.5 * (hfov * (PI_ / 180.0))), edge_y = tan(0.5 * (vfov * (PI_ / 180.0)));
  for (size_t v = 0; v < n_order; v++) {
    size_t p = order[v];
    int px = (int)(p % (size_t)W), py = (int)(p / (size_t)W);
    v3 total = V(0, 0, 0);
    float s1 = 0.0f, s2 = 0.0f;
    int sample, flag = 0;
    for (sample = 1; sample <= ns_aa; sample++) {
      v3 Lv[3];
      for (int var = 0; var < (counter ? 3 : 1); var++) {
        double e = var == 0 ? 0.0 : var == 1 ? kShift : -kShift;
        D.cx = (uint32_t)p; D.cy = (uint32_t)sample; D.eps = e;
        double jy, jx;   /* gridSampler->get_sample(): the first draw is y (both sources) */
        draw_pair(&D, kStreamJitter, 0, &jy, &jx);
        double sy = (double)py + jy, sx = (double)px + jx;
        double nx = sx / (double)W, ny = sy / (double)H;
        v3 dir = unit(V(edge_x * (2 * nx - 1), edge_y * (2 * ny - 1), -1));   /* camera.cpp:278-305 */
        ray r;
        r.o = V(pos[0], pos[1], pos[2]);
        r.d = V((dir.x * c2w[0] + dir.y * c2w[1]) + dir.z * c2w[2], (dir.x * c2w[3] + dir.y * c2w[4]) + dir.z * c2w[5],
                (dir.x * c2w[6] + dir.y * c2w[7]) + dir.z * c2w[8]);
        r.min_t = nclip; r.max_t = fclip;
        Lv[var] = radiance_s(Q, &S, &E, var ? shifted(r, e) : r, &D, NULL, NULL);
      }
      if (counter && (moved(Lv[0], Lv[1]) || moved(Lv[0], Lv[2]))) flag |= 1;
      v3 L = Lv[0];
      float illum = (float)((0.2126f * L.x + 0.7152f * L.y) + 0.0722f * L.z);
      s1 += illum; s2 += illum * illum;
      total = add(total, L);
      if (sample > 1 && sample % samples_per_batch == 0) {
        float sd = (float)sqrt(1.0 / (sample - 1) * (double)(s2 - s1 * s1 / (float)sample));
        float ci = (float)(1.96 * (double)sd / sqrt((double)sample));
        double lhs = (double)ci, rhs = max_tol * (double)s1 / (double)sample;
        if (!(lhs == 0.0 && rhs == 0.0) && fabs(lhs - rhs) <= 1e-6 * fmax(fabs(lhs), fabs(rhs))) flag |= 2;
        if (lhs <= rhs) break;
      }
    }
    double rc = 1. / (double)sample;
    scene[3 * p] = total.x * rc; scene[3 * p + 1] = total.y * rc; scene[3 * p + 2] = total.z * rc;
    if (flags) flags[p] = (uint8_t)flag;
    if (n_samples) n_samples[p] = sample;
    if (!counter) {
      if (stream_pos) stream_pos[v] = D.pos;
      for (int k = 0; k < 32; k++) (void)lfo_mt_draw(D.mt);   /* irradiance falloff (:1043-1063) */
      D.pos += 32;
    }
  }
  if (D.mt) lfo_mt_close(D.mt);
  env_free(&E);
}

/* est_radiance_global_illumination along explicit rays under the device's counters.  rays: n x 8
 * {o, d, min_t, max_t}; ctr: n x 2 {c.x, c.y}; out: n x 8 {hit, t, n xyz, radiance rgb} (lf_scene_trace_ray);
 * fragile: n */
void lfo_scene_rays(const lfo_scene_desc* Q, size_t n, const double* rays, const uint32_t* ctr, uint64_t key,
                    double* out, uint8_t* fragile) {
  scene_t S = geometry_of(Q);
  env_t E;
  env_init(&E, Q->env_w, Q->env_h, Q->env);
  for (size_t i = 0; i < n; i++) {
    const double* q = rays + 8 * i;
    ray r = {V(q[0], q[1], q[2]), V(q[3], q[4], q[5]), q[6], q[7]};
    v3 Lv[3];
    int hv[3];
    isect is0 = {0.0, {0, 0, 0}, 0};
    for (int var = 0; var < 3; var++) {
      double e = var == 0 ? 0.0 : var == 1 ? kShift : -kShift;
      draws_t D = {1, NULL, 0, ctr[2 * i], ctr[2 * i + 1], {(uint32_t)key, (uint32_t)(key >> 32)}, e};
      isect is = {0.0, {0, 0, 0}, 0};
      Lv[var] = radiance_s(Q, &S, &E, var ? shifted(r, e) : r, &D, &is, &hv[var]);
      if (var == 0) is0 = is;
    }
    double* o = out + 8 * i;
    o[0] = hv[0] ? 1.0 : 0.0; o[1] = hv[0] ? is0.t : 0.0;
    o[2] = hv[0] ? is0.n.x : 0.0; o[3] = hv[0] ? is0.n.y : 0.0; o[4] = hv[0] ? is0.n.z : 0.0;
    o[5] = Lv[0].x; o[6] = Lv[0].y; o[7] = Lv[0].z;
    fragile[i] = (uint8_t)(hv[0] != hv[1] || hv[0] != hv[2] || moved(Lv[0], Lv[1]) || moved(Lv[0], Lv[2]));
  }
  env_free(&E);
}

/* zero_bounce_radiance / one_bounce_radiance / the two estimators by name for an intersection the caller
 * found: what = 0 zero bounce, 1 one bounce (by Q->hemisphere), 2 the hemisphere estimator, 3 the importance
 * estimator (lf_scene_shade).  tn: n x 4 {t, normal}; mats: n x 4 {kind, rgb}; rgb: n x 3 */
void lfo_scene_shade(const lfo_scene_desc* Q, int what, size_t n, const double* rays, const double* tn,
                     const double* mats, const uint32_t* ctr, uint64_t key, double* rgb, uint8_t* fragile) {
  scene_t S = geometry_of(Q);
  env_t E;
  env_init(&E, Q->env_w, Q->env_h, Q->env);
  int bits = what == 0 ? 1 : 2;
  int hemi = what == 2 ? 1 : what == 3 ? 0 : Q->hemisphere;
  for (size_t i = 0; i < n; i++) {
    const double* q = rays + 8 * i;
    ray r = {V(q[0], q[1], q[2]), V(q[3], q[4], q[5]), q[6], q[7]};
    v3 Lv[3];
    for (int var = 0; var < 3; var++) {
      double e = var == 0 ? 0.0 : var == 1 ? kShift : -kShift;
      draws_t D = {1, NULL, 0, ctr[2 * i], ctr[2 * i + 1], {(uint32_t)key, (uint32_t)(key >> 32)}, e};
      Lv[var] = shade(Q, &S, &E, hemi, var ? shifted(r, e) : r, tn[4 * i], V(tn[4 * i + 1], tn[4 * i + 2], tn[4 * i + 3]),
                      mats + 4 * i, bits, &D);
    }
    rgb[3 * i] = Lv[0].x; rgb[3 * i + 1] = Lv[0].y; rgb[3 * i + 2] = Lv[0].z;
    fragile[i] = (uint8_t)(moved(Lv[0], Lv[1]) || moved(Lv[0], Lv[2]));
  }
  env_free(&E);
}
