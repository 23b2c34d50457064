/* TEST INFRASTRUCTURE -- an INDEPENDENT double-precision tracer for the geometric lens march.
 * Never linked into, imported by or shipped with the product library; only tests/ load it.
 *
 * Why it exists: the device march (lens-flare_amd/csrc/lf_march.hip) is compared bit for bit with
 * oracle/lf_geo_oracle.c, which restates the same float32 recipe and follows the device's
 * v_sqrt_f32 through a measured table.  That proves the two agree, not that either is right.  This
 * file is the second opinion at the north star's actual bar (<= 1e-4 relative per pixel): it
 * shares NO code, NO arithmetic recipe and NO square-root table with lf_geo_oracle.c --
 *   * float64 throughout, libm sqrt / sin / cos;
 *   * textbook formulations: sphere given by centre + radius and the quadratic in the ray
 *     parameter (both roots, the hit nearer the vertex plane is taken), the unit normal
 *     (hit - centre) / R, vector Snell d' = eta d + (eta cos_i - cos_t) n, mirror d' = d - 2 (d.n) n,
 *     Fresnel from the two amplitude coefficients r_s, r_p with the media's actual indices;
 *   * its own Philox4x32-10 (Salmon et al., SC'11) and its own pair sequencing.
 * The ONLY thing it takes from the specification is what defines the
 * estimator itself: which sensor point and which rear-pupil point sample (pixel, s) uses, and how a
 * ray that leaves the front element is weighted by the sun's lobe.
 *
 * PARITY STATUS: the reference has no geometric lens (src/pathtracer/camera_lens.cpp:22-30 is a
 * stub, advanced_bsdf.cpp:156-169 an empty refract), so like lf_geo_oracle.c this tracer is
 * "parity unpinned" against the reference; it is anchored by the same analytic known-answer tests
 * and by the small-angle agreement with the reference's own T / R / L matrices
 * (src/pathtracer/pathtracer.cpp:527-537, :588-689) -- tests/test_geo_f64_kat.py.
 *
 * Fragile rays.  Float32 and float64 disagree about the FATE of a ray that passes within rounding
 * distance of a decision boundary (edge of a clear aperture, edge of an aperture-mask texel whose
 * neighbour differs, critical angle, grazing miss).  Such decisions are taken as float64 takes
 * them, but the ray is marked fragile, followed as if every fragile decision had passed, and the
 * contribution it then could make is summed per pixel in `frag`.  A faithful float32 evaluation
 * then satisfies  |pixel32 - pixel64| <= tol * pixel64 + frag  with tol far below 1e-4.
 *
 * Films and the bilinear stop (lf_set_lens_coatings, lf_set_mask_filter): process-global settings, off by
 * default (g64_set_films, g64_set_mask_filter) -- with neither set every result is bit for bit what it was
 * before they existed.  A film changes the reflectance of its interface (Airy's single-film formula in complex
 * arithmetic, written from the textbook below), never the geometry.  Under the filter the stop's weight is
 * continuous across texel edges, so cause bit 2 is not raised; a ray carries a SLOPE ALLOWANCE instead: how
 * far a move of eps_mm at the stop can change its weight (stop_bilinear), added into `frag`.
 *
 * The light list (lf_set_lights, lf_set_lights_ex, lf_set_lights_geom): a process-global setting, off by default
 * (g64_set_lights) -- with none set g64_trace shades with the single sun of g64_lens and every result is bit for bit
 * what it was.  With a list, every ray that left the front element is tested against every light at its own float64
 * exit point r.o along r.d, written from the textbook: a directional light by q = (1 - unit(d).unit(s)) / (1 - cos
 * alpha), factor (1 - q)^2 where q < 1; a point light at L the same with s = L - r.o; an area light by the plane's
 * intersection and (u, v) through the Gram matrix of its edges, factor 1 (area_lit).  Contributions add, each with
 * its own light's radiance; counter 6 counts (ray, light) pairs.  A lobe falls to zero continuously and needs no
 * band; a rectangle's outline is a hard edge: a pair whose hit point lies within eps_light(t) = eps_exit + t eps_dir
 * + 2.4e-7 |P - C| millimetres of it (or whose ray grazes the plane's horizon, |d.dir| < eps_cos) is decided as
 * float64 decides, its weight goes into `frag` whichever way that was, and a ninth counter (light_edge_pairs) counts
 * it -- read with g64_light_edge_pairs(): the array handed to g64_trace keeps the eight slots older callers allocate.
 *
 * The occluder list (lf_set_ghost_occlusion, lf_set_ghost_occlusion_reach): a process-global setting, off by default
 * (g64_set_occlusion) -- with no primitive every result is bit for bit what it was.  With one, every (ray, light) pair that
 * would contribute is mapped to the world as the contract states it and tested by brute force over [0, reach of that light]
 * (textbook ray-sphere and ray-triangle, each light on its own); a blocked pair adds nothing and is not counted as lit.  An
 * occluder's outline is a hard edge like a rectangle's: a pair whose shadow ray passes within eps(t) = (eps_exit + t_mm
 * eps_dir) wpm of an outline, or whose root lies within it of an end of the segment, and which no primitive blocks firmly,
 * puts its weight into `frag` whichever way float64 decided, and is counted (g64_occlusion_pairs: tested, blocked, edge).
 */
#define _GNU_SOURCE
#include <complex.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define G64_MAX_SURF 16
#define G64_MAX_LAMBDA 8

typedef struct {
  int n_surf, stop, n_lambda;
  double radius[G64_MAX_SURF], thickness[G64_MAX_SURF], semi_ap[G64_MAX_SURF];
  double ior[G64_MAX_LAMBDA][G64_MAX_SURF]; /* medium BEHIND interface k (sensor side) */
  double sensor_w_mm;
  double sun_dir[3], sun_radiance[3], sun_angular_radius;
  double lambda_rgb[G64_MAX_LAMBDA][3];
  double eps_mm;    /* a geometric decision closer than this to its boundary is fragile */
  double eps_texel; /* ... in mask-texel units */
  double eps_cos;   /* ... for cos^2 of the refraction angle near the critical angle */
} g64_lens;

typedef struct { double x, y, z; } vec;
static vec V(double x, double y, double z) { vec v = {x, y, z}; return v; }
static vec add(vec a, vec b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
static vec sub(vec a, vec b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static vec scale(vec a, double s) { return V(a.x * s, a.y * s, a.z * s); }
static double dotp(vec a, vec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static vec normalise(vec a) { return scale(a, 1.0 / sqrt(dotp(a, a))); }

/* Philox4x32-10 with 128-bit products */
static void philox64(const uint32_t c_in[4], const uint32_t k_in[2], uint32_t out[4]) {
  uint32_t c[4] = {c_in[0], c_in[1], c_in[2], c_in[3]}, k[2] = {k_in[0], k_in[1]};
  for (int round = 0; round < 10; round++) {
    unsigned __int128 both = ((unsigned __int128)((uint64_t)0xCD9E8D57u * c[2]) << 64) |
                             (uint64_t)((uint64_t)0xD2511F53u * c[0]);
    uint64_t lo_prod = (uint64_t)both, hi_prod = (uint64_t)(both >> 64);
    uint32_t next[4] = {(uint32_t)(hi_prod >> 32) ^ c[1] ^ k[0], (uint32_t)hi_prod,
                        (uint32_t)(lo_prod >> 32) ^ c[3] ^ k[1], (uint32_t)lo_prod};
    memcpy(c, next, sizeof(c));
    k[0] += 0x9E3779B9u;
    k[1] += 0xBB67AE85u;
  }
  memcpy(out, c, sizeof(c));
}
void g64_philox(const uint32_t c[4], const uint32_t k[2], uint32_t out[4]) { philox64(c, k, out); }

/* ---- the optical system in world terms ---------------------------------------------------- */
typedef struct {
  double vertex_z[G64_MAX_SURF];
  double n_scene[G64_MAX_LAMBDA][G64_MAX_SURF];  /* index on the scene side (lower z) of interface k */
  double n_sensor[G64_MAX_LAMBDA][G64_MAX_SURF]; /* index on the sensor side */
  double sensor_z;
} g64_system;

static void lay_out(const g64_lens* L, g64_system* S) {
  double z = 0.0;
  for (int k = 0; k < L->n_surf; k++) { S->vertex_z[k] = z; z += L->thickness[k]; }
  S->sensor_z = z;
  for (int l = 0; l < L->n_lambda; l++) {
    double medium = 1.0; /* air in front of the lens */
    for (int k = 0; k < L->n_surf; k++) {
      S->n_scene[l][k] = medium;
      if (k != L->stop) medium = L->ior[l][k]; /* the stop sits inside one medium */
      S->n_sensor[l][k] = medium;
    }
  }
}

typedef struct {
  vec o, d;
  double w;      /* weight as float64 decides */
  double w_pot;  /* weight if every fragile decision passes (upper bound for texel choices) */
  int fragile;
  int dead;      /* 0 alive, else cause: 1 mask/stop, 2 aperture/miss, 3 total reflection */
  int cause;     /* why fragile, bits: 1 the rim of a clear aperture / of the stop's housing, 2 a mask texel's edge,
                    4 the critical angle, 8 a grazing miss of a sphere, 16 (filter) the edge of the open footprints */
  double slope;  /* (filter) how much a move of eps_mm at the stop can change the weight, first order */
} g64_ray;

/* single-layer films (lf_set_lens_coatings): float values held in doubles; n_surf == 0: none */
static int g64_film_n = 0;
static double g64_film_lambda[G64_MAX_LAMBDA], g64_film_d[G64_MAX_SURF], g64_film_m[G64_MAX_LAMBDA][G64_MAX_SURF];
/* index: n_lambda rows of n_surf film indices; thickness_nm[k] == 0: interface k is bare */
void g64_set_films(int n_surf, int n_lambda, const double* lambda_nm, const double* thickness_nm, const double* index) {
  g64_film_n = 0;
  if (n_surf <= 0 || n_surf > G64_MAX_SURF || n_lambda <= 0 || n_lambda > G64_MAX_LAMBDA) return;
  for (int l = 0; l < n_lambda; l++) {
    g64_film_lambda[l] = lambda_nm[l];
    for (int k = 0; k < n_surf; k++) g64_film_m[l][k] = index[l * n_surf + k];
  }
  for (int k = 0; k < n_surf; k++) g64_film_d[k] = thickness_nm[k];
  g64_film_n = n_surf;
}
/* how the stop's mask is read (lf_set_mask_filter): 0 the nearest texel, 1 bilinear */
static int g64_filter = 0;
void g64_set_mask_filter(int filter) { g64_filter = filter != 0; }

/* Airy's reflectance of one homogeneous film (index m, thickness d) between n1 (the ray arrives in it, at
 * cos_i) and n2, for light of vacuum wavelength lambda (d and lambda in the same unit): per polarisation the
 * two faces' Fresnel amplitudes r01, r12 and the round trip's phase 2 beta = 4 pi m d cos(theta_m) / lambda,
 *   r = (r01 + r12 e^{2 i beta}) / (1 + r01 r12 e^{2 i beta}),   R = (|r_s|^2 + |r_p|^2) / 2
 * (Born & Wolf, Principles of Optics, section 1.6.4; Hecht, Optics, section 9.7).  Not totally reflecting. */
static double film_reflectance(double n1, double m, double n2, double d, double lambda, double cos_i) {
  const double sin_i = sqrt(fmax(0.0, 1.0 - cos_i * cos_i));
  const double sin_m = n1 * sin_i / m, sin_t = n1 * sin_i / n2;      /* Snell, face by face */
  const double complex cos_m = csqrt(1.0 - sin_m * sin_m);            /* (evanescent in the film: imaginary) */
  const double cos_t = sqrt(fmax(0.0, 1.0 - sin_t * sin_t));
  const double complex round_trip = cexp(I * (4.0 * M_PI * m * d / lambda) * cos_m);
  const double complex s01 = (n1 * cos_i - m * cos_m) / (n1 * cos_i + m * cos_m);
  const double complex s12 = (m * cos_m - n2 * cos_t) / (m * cos_m + n2 * cos_t);
  const double complex p01 = (m * cos_i - n1 * cos_m) / (m * cos_i + n1 * cos_m);
  const double complex p12 = (n2 * cos_m - m * cos_t) / (n2 * cos_m + m * cos_t);
  const double complex rs = (s01 + s12 * round_trip) / (1.0 + s01 * s12 * round_trip);
  const double complex rp = (p01 + p12 * round_trip) / (1.0 + p01 * p12 * round_trip);
  const double Rs = creal(rs * conj(rs)), Rp = creal(rp * conj(rp));
  return 0.5 * (Rs + Rp);
}

/* one spherical (or flat) glass interface: refraction or mirror reflection */
static void glass(const g64_lens* L, const g64_system* S, int lam, int k, int mirror, g64_ray* r) {
  const double R = L->radius[k], h = L->semi_ap[k];
  double t;
  if (R == 0.0) {
    t = (S->vertex_z[k] - r->o.z) / r->d.z;
  } else {
    const vec centre = V(0.0, 0.0, S->vertex_z[k] + R);
    const vec oc = sub(r->o, centre);
    const double b = dotp(oc, r->d), c = dotp(oc, oc) - R * R;
    const double disc = b * b - c;
    if (disc < 0.0) {
      if (!r->dead) r->dead = 2;
      /* a grazing miss within rounding distance cannot be followed further: charge the whole
       * weight it carried as the fragile bound (rare: the clear apertures cut in long before) */
      if (disc > -L->eps_mm * fabs(R)) { r->fragile = 2; r->cause |= 8; }
      r->w = 0.0;
      return;
    }
    const double sq = sqrt(disc);
    const double t1 = -b - sq, t2 = -b + sq;
    const double z1 = r->o.z + t1 * r->d.z - S->vertex_z[k], z2 = r->o.z + t2 * r->d.z - S->vertex_z[k];
    t = fabs(z1) <= fabs(z2) ? t1 : t2; /* the intersection nearer the vertex plane */
  }
  const vec hit = add(r->o, scale(r->d, t));
  const double rho = sqrt(hit.x * hit.x + hit.y * hit.y);
  if (fabs(rho - h) < L->eps_mm) { r->fragile = 1; r->cause |= 1; }
  if (rho > h) {
    if (!r->dead) r->dead = 2;
    if (!r->fragile) { r->w = 0.0; return; }
    r->w = 0.0; /* float64 says vignetted; follow it for the potential weight only */
  }
  vec n = R == 0.0 ? V(0, 0, 1) : scale(sub(hit, V(0.0, 0.0, S->vertex_z[k] + R)), 1.0 / R);
  double cos_i = -dotp(r->d, n);
  if (cos_i < 0.0) { n = scale(n, -1.0); cos_i = -cos_i; } /* normal against the ray */
  /* media: a ray travelling +z goes from the scene side to the sensor side */
  const int towards_sensor = r->d.z > 0.0;
  const double n1 = towards_sensor ? S->n_scene[lam][k] : S->n_sensor[lam][k];
  const double n2 = towards_sensor ? S->n_sensor[lam][k] : S->n_scene[lam][k];
  const double eta = n1 / n2;
  const double sin2_t = eta * eta * (1.0 - cos_i * cos_i);
  const int tir = sin2_t > 1.0;
  if (fabs(1.0 - sin2_t) < L->eps_cos) { r->fragile = 1; r->cause |= 4; }
  double reflectance = 1.0, cos_t = 0.0;
  if (!tir) {
    cos_t = sqrt(1.0 - sin2_t);
    const double rs = (n1 * cos_i - n2 * cos_t) / (n1 * cos_i + n2 * cos_t);
    const double rp = (n2 * cos_i - n1 * cos_t) / (n2 * cos_i + n1 * cos_t);
    reflectance = 0.5 * (rs * rs + rp * rp);
    if (k < g64_film_n && g64_film_d[k] > 0.0)
      reflectance = film_reflectance(n1, g64_film_m[lam][k], n2, g64_film_d[k], g64_film_lambda[lam], cos_i);
  }
  if (mirror) {
    r->w *= reflectance;
    r->w_pot *= reflectance;
    r->slope *= reflectance;
    r->d = add(r->d, scale(n, 2.0 * cos_i));
  } else {
    if (tir) {
      if (!r->dead) r->dead = 3;
      r->w = 0.0;
      if (!r->fragile) return;
      cos_t = 0.0; /* follow the critical ray for the potential weight */
    }
    r->w *= 1.0 - reflectance;
    r->w_pot *= tir ? 1.0 : 1.0 - reflectance;
    r->slope *= tir ? 1.0 : 1.0 - reflectance;
    r->d = normalise(add(scale(r->d, eta), scale(n, eta * cos_i - cos_t)));
  }
  r->o = hit;
}

/* one cell of the bilinear mask ("Mask filter"): the four texels around grid point
 * (i0, j0) .. (i0 + 1, j0 + 1) -- texel centres at i + 1/2, indices clamped, negative texels count as 0 -- at
 * the fractions (fx, fy): the value, its partial derivatives per texel, and whether any of the four is open */
static int bilinear_cell(const float* mask, int mw, int mh, int i0, int j0, double fx, double fy, double* a,
                         double* da_du, double* da_dv) {
  const int xa = i0 < 0 ? 0 : i0 > mw - 1 ? mw - 1 : i0, xb = i0 + 1 < 0 ? 0 : i0 + 1 > mw - 1 ? mw - 1 : i0 + 1;
  const int ya = j0 < 0 ? 0 : j0 > mh - 1 ? mh - 1 : j0, yb = j0 + 1 < 0 ? 0 : j0 + 1 > mh - 1 ? mh - 1 : j0 + 1;
  const double t00 = fmax(mask[ya * mw + xa], 0.0), t10 = fmax(mask[ya * mw + xb], 0.0);
  const double t01 = fmax(mask[yb * mw + xa], 0.0), t11 = fmax(mask[yb * mw + xb], 0.0);
  *a = (1.0 - fy) * ((1.0 - fx) * t00 + fx * t10) + fy * ((1.0 - fx) * t01 + fx * t11);
  *da_du = (1.0 - fy) * (t10 - t00) + fy * (t11 - t01);
  *da_dv = (1.0 - fx) * (t01 - t00) + fx * (t11 - t10);
  return t00 > 0.0 || t10 > 0.0 || t01 > 0.0 || t11 > 0.0;
}

/* the stop under the bilinear filter.  The weight is continuous in the hit point, so no texel edge is a
 * decision; what float32's position error (eps_mm, in texels: delta) can do is move the weight along its slope.
 * The ray's allowance grows by  (the weight it arrives with) x (|da/dfu| delta_u + |da/dfv| delta_v),  the
 * derivatives those of the cell the ray is in -- and, within delta of a cell's border, the larger of both
 * sides', as the bilinear's slope jumps there.  Whether the ray is ALIVE (any of the four texels open) is
 * still a decision: within delta of a border beyond which that changes the ray is fragile (bit 16); its weight
 * there is within the allowance of 0, so following it costs next to nothing. */
static void stop_bilinear(const g64_lens* L, const g64_system* S, int k, const float* mask, int mw, int mh,
                          g64_ray* r) {
  const double t = (S->vertex_z[k] - r->o.z) / r->d.z;
  const vec hit = add(r->o, scale(r->d, t));
  const double h = L->semi_ap[k];
  const double rho = sqrt(hit.x * hit.x + hit.y * hit.y);
  if (fabs(rho - h) < L->eps_mm) { r->fragile = 1; r->cause |= 1; }
  const int outside = rho > h;
  const double gx = (hit.x / h + 1.0) * (0.5 * mw) - 0.5, gy = (hit.y / h + 1.0) * (0.5 * mh) - 0.5;
  const double i0 = floor(gx), j0 = floor(gy), fx = gx - i0, fy = gy - j0;
  const double delta_u = L->eps_mm / h * 0.5 * mw, delta_v = L->eps_mm / h * 0.5 * mh;
  double a, gu, gv;
  const int open = bilinear_cell(mask, mw, mh, (int)i0, (int)j0, fx, fy, &a, &gu, &gv);
  gu = fabs(gu); gv = fabs(gv);
  for (int sy = -1; sy <= 1; sy++)
    for (int sx = -1; sx <= 1; sx++) {
      if (!sx && !sy) continue;
      if ((sx < 0 && fx > delta_u) || (sx > 0 && 1.0 - fx > delta_u)) continue;
      if ((sy < 0 && fy > delta_v) || (sy > 0 && 1.0 - fy > delta_v)) continue;
      double b, bu, bv;
      if (bilinear_cell(mask, mw, mh, (int)i0 + sx, (int)j0 + sy, fx - sx, fy - sy, &b, &bu, &bv) != open) {
        r->fragile = 1; r->cause |= 16;
      }
      gu = fmax(gu, fabs(bu)); gv = fmax(gv, fabs(bv));
    }
  if (outside || !open) {
    if (!r->dead) r->dead = 1;
    r->w = 0.0;
    if (!r->fragile) return;
  }
  r->slope = r->slope * a + r->w_pot * (gu * delta_u + gv * delta_v);
  r->w *= a;
  r->w_pot *= a;
  r->o = hit;
}

/* the stop: a plane with a round housing and the aperture mask (nearest texel) */
static void stop_plane(const g64_lens* L, const g64_system* S, int k, const float* mask, int mw, int mh,
                       g64_ray* r) {
  if (g64_filter) { stop_bilinear(L, S, k, mask, mw, mh, r); return; }
  const double t = (S->vertex_z[k] - r->o.z) / r->d.z;
  const vec hit = add(r->o, scale(r->d, t));
  const double h = L->semi_ap[k];
  const double rho = sqrt(hit.x * hit.x + hit.y * hit.y);
  if (fabs(rho - h) < L->eps_mm) { r->fragile = 1; r->cause |= 1; }
  int outside = rho > h;
  const double fu = (hit.x / h + 1.0) * (0.5 * mw), fv = (hit.y / h + 1.0) * (0.5 * mh);
  int ix = (int)fu, iy = (int)fv; /* truncation, like the specification's (int) cast */
  if (ix < 0) ix = 0; if (ix > mw - 1) ix = mw - 1;
  if (iy < 0) iy = 0; if (iy > mh - 1) iy = mh - 1;
  const double a = mask[iy * mw + ix];
  /* texel neighbours a float32 evaluation could land in instead */
  double a_max = a, a_min = a;
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      if (!dx && !dy) continue;
      if (dx < 0 && fu - floor(fu) > L->eps_texel) continue;
      if (dx > 0 && ceil(fu) - fu > L->eps_texel && fu != floor(fu)) continue;
      if (dx > 0 && fu == floor(fu)) continue;
      if (dy < 0 && fv - floor(fv) > L->eps_texel) continue;
      if (dy > 0 && ceil(fv) - fv > L->eps_texel && fv != floor(fv)) continue;
      if (dy > 0 && fv == floor(fv)) continue;
      int jx = ix + dx, jy = iy + dy;
      if (jx < 0 || jy < 0 || jx >= mw || jy >= mh) continue;
      const double b = mask[jy * mw + jx];
      if (b > a_max) a_max = b;
      if (b < a_min) a_min = b;
    }
  if (a_max != a_min) { r->fragile = 1; r->cause |= 2; }
  if (outside || !(a > 0.0)) {
    if (!r->dead) r->dead = 1;
    r->w = 0.0;
    if (!r->fragile) return;
  }
  r->w *= a;
  r->w_pot *= a_max;
  r->o = hit;
}

/* the interfaces a ray meets, in order, for ghost pair (i, j); i < 0 = no reflection */
static int itinerary(int n, int i, int j, int* surf, int* is_mirror) {
  int m = 0;
  if (i < 0) {
    for (int k = n - 1; k >= 0; k--) { surf[m] = k; is_mirror[m++] = 0; }
    return m;
  }
  for (int k = n - 1; k > i; k--) { surf[m] = k; is_mirror[m++] = 0; }
  surf[m] = i; is_mirror[m++] = 1;
  for (int k = i + 1; k < j; k++) { surf[m] = k; is_mirror[m++] = 0; }
  surf[m] = j; is_mirror[m++] = 1;
  for (int k = j - 1; k >= 0; k--) { surf[m] = k; is_mirror[m++] = 0; }
  return m;
}

/* follow one ray along one itinerary; returns the events completed while (really) alive */
static int follow(const g64_lens* L, const g64_system* S, int lam, int i, int j, const float* mask,
                  int mw, int mh, g64_ray* r) {
  int surf[3 * G64_MAX_SURF], mir[3 * G64_MAX_SURF];
  const int m = itinerary(L->n_surf, i, j, surf, mir);
  int events = 0;
  for (int e = 0; e < m; e++) {
    const int was_dead = r->dead;
    if (surf[e] == L->stop) stop_plane(L, S, surf[e], mask, mw, mh, r);
    else glass(L, S, lam, surf[e], mir[e], r);
    if (!r->dead) events++;
    if (r->dead && !was_dead && !r->fragile) return events;  /* settled: nothing more to learn */
    if (r->fragile == 2) return events;                        /* cannot be followed */
    if (r->dead && !r->fragile) return events;
  }
  return events;
}

/* exported for the known-answer tests: one glass event / one whole path on a caller-supplied ray */
int g64_glass_event(const g64_lens* L, int lam, int k, int mirror, double p[3], double d[3], double* w) {
  g64_system S;
  lay_out(L, &S);
  g64_ray r = {V(p[0], p[1], p[2]), V(d[0], d[1], d[2]), *w, *w, 0, 0};
  glass(L, &S, lam, k, mirror, &r);
  p[0] = r.o.x; p[1] = r.o.y; p[2] = r.o.z; d[0] = r.d.x; d[1] = r.d.y; d[2] = r.d.z; *w = r.w;
  return r.dead;
}

int g64_trace_ray(const g64_lens* L, int lam, int i, int j, double p[3], double d[3], double* w,
                  const float* mask, int mw, int mh, int* n_events) {
  g64_system S;
  lay_out(L, &S);
  g64_ray r = {V(p[0], p[1], p[2]), V(d[0], d[1], d[2]), *w, *w, 0, 0};
  const int ev = follow(L, &S, lam, i, j, mask, mw, mh, &r);
  p[0] = r.o.x; p[1] = r.o.y; p[2] = r.o.z; d[0] = r.d.x; d[1] = r.d.y; d[2] = r.d.z; *w = r.w;
  if (n_events) *n_events = ev;
  return r.dead;
}

/* ... the same with the tracer's own verdict on how close the ray came to a decision boundary:
 * out = {fragile (0 / 1 / 2), potential weight} */
int g64_trace_ray_ex(const g64_lens* L, int lam, int i, int j, double p[3], double d[3], double* w,
                     const float* mask, int mw, int mh, int* n_events, double out[2]) {
  g64_system S;
  lay_out(L, &S);
  g64_ray r = {V(p[0], p[1], p[2]), V(d[0], d[1], d[2]), *w, *w, 0, 0};
  const int ev = follow(L, &S, lam, i, j, mask, mw, mh, &r);
  p[0] = r.o.x; p[1] = r.o.y; p[2] = r.o.z; d[0] = r.d.x; d[1] = r.d.y; d[2] = r.d.z; *w = r.w;
  if (n_events) *n_events = ev;
  out[0] = (double)r.fragile; out[1] = r.w_pot;
  return r.dead;
}

/* ... and the slope allowance of a ray that crossed a filtered stop: out = {fragile, potential weight, allowance} */
int g64_trace_ray_slope(const g64_lens* L, int lam, int i, int j, double p[3], double d[3], double* w,
                        const float* mask, int mw, int mh, int* n_events, double out[3]) {
  g64_system S;
  lay_out(L, &S);
  g64_ray r = {V(p[0], p[1], p[2]), V(d[0], d[1], d[2]), *w, *w, 0, 0};
  const int ev = follow(L, &S, lam, i, j, mask, mw, mh, &r);
  p[0] = r.o.x; p[1] = r.o.y; p[2] = r.o.z; d[0] = r.d.x; d[1] = r.d.y; d[2] = r.d.z; *w = r.w;
  if (n_events) *n_events = ev;
  out[0] = (double)r.fragile; out[1] = r.w_pot; out[2] = r.slope;
  return r.dead;
}

double g64_sensor_z(const g64_lens* L) {
  g64_system S;
  lay_out(L, &S);
  return S.sensor_z;
}

static double unit_interval(uint32_t bits) { return (double)(bits >> 8) / 16777216.0; }

/* the disc the sensor samples aim at (lf_set_pupil_target, float values held in doubles):
 * h <= 0 = the rear element's clear aperture at its vertex plane */
static double g64_pupil_h = 0.0, g64_pupil_z = 0.0;
void g64_set_pupil_target(double h, double z) { g64_pupil_h = h; g64_pupil_z = z; }
/* g64_trace only traces the pixels with x in [x0, x1) (the others stay 0 and launch nothing): a window of
 * a wide band keeps a full-sample-count check inside a test's time budget.  Default: every column. */
/* log2 of the pixel stride in x of a wave's tile (lf_set_tile_stride): which pixels share a sub-cell draw */
static int g64_xs = 3;   /* the library's default: columns 8 apart */
void g64_set_tile_stride_log2(int xs) { g64_xs = xs; }
static int g64_x0 = 0, g64_x1 = 1 << 30;
void g64_set_x_window(int x0, int x1) { g64_x0 = x0; g64_x1 = x1; }

/* the ray from the sensor point (X, Y) mm to the point (a, b) of the pupil square [-1, 1]^2, mapped to the
 * disc the samples aim at; returns the start weight: the disc's solid angle x cos^4 */
static double aim(const g64_lens* L, const g64_system* S, double X, double Y, double a, double b, vec* origin, vec* dir) {
  /* concentric square -> disc (Shirley & Chiu) */
  double qx = 0.0, qy = 0.0;
  if (a != 0.0 || b != 0.0) {
    if (fabs(a) > fabs(b)) { const double th = (M_PI / 4.0) * (b / a); qx = a * cos(th); qy = a * sin(th); }
    else { const double th = (M_PI / 4.0) * (a / b); qx = b * sin(th); qy = b * cos(th); }
  }
  const int last = L->n_surf - 1;
  const double pupil_h = g64_pupil_h > 0.0 ? g64_pupil_h : L->semi_ap[last];
  const double pupil_z = g64_pupil_h > 0.0 ? g64_pupil_z : S->vertex_z[last];
  *origin = V(X, Y, S->sensor_z);
  *dir = normalise(sub(V(pupil_h * qx, pupil_h * qy, pupil_z), *origin));
  const double dist = S->sensor_z - pupil_z;
  const double cos2 = dir->z * dir->z;
  return (M_PI * pupil_h * pupil_h / (dist * dist)) * cos2 * cos2;
}

/* The estimator's sample: sensor point and rear-pupil point of sample s of
 * pixel (x, y).  Returns the start direction and the start weight. */
static _Thread_local double t64_ua = 0.5, t64_ub = 0.5;   /* the pupil-square point of this thread's last sample_ray */
static double sample_ray(const g64_lens* L, const g64_system* S, int W, int H, int x, int y, int s, int spp,
                         int sub_bits, const uint32_t key[2], vec* origin, vec* dir) {
  const uint32_t ctr[4] = {(uint32_t)(y * W + x), (uint32_t)s, 0x6e5f1a2eu, 0u};
  uint32_t rnd[4];
  philox64(ctr, key, rnd);
  double ua = unit_interval(rnd[2]), ub = unit_interval(rnd[3]);
  int G = (int)floor(sqrt((double)spp));
  while ((G + 1) * (G + 1) <= spp) G++;
  while (G * G > spp) G--;
  if (s < G * G) {
    const int cy = s / G, cx = s % G;
    const int per_block = 1 << g64_xs, block_w = 8 * per_block;
    const int tiles_x = ((W + block_w - 1) / block_w) * per_block;
    const uint32_t tile = (uint32_t)((y / 8) * tiles_x + (x / block_w) * per_block + x % per_block);
    const uint32_t c2[4] = {tile, (uint32_t)s, 0x51bce110u, 0u};
    uint32_t r2[4];
    philox64(c2, key, r2);
    const double sub = (double)(1 << sub_bits);
    const double sx = sub_bits ? (double)(r2[0] >> (32 - sub_bits)) : 0.0;
    const double sy = sub_bits ? (double)(r2[1] >> (32 - sub_bits)) : 0.0;
    ua = (cx + (sx + ua) / sub) / G;
    ub = (cy + (sy + ub) / sub) / G;
  }
  t64_ua = ua; t64_ub = ub;
  const double pitch = L->sensor_w_mm / W;
  const double X = -((x + unit_interval(rnd[0])) - 0.5 * W) * pitch;
  const double Y = -((y + unit_interval(rnd[1])) - 0.5 * H) * pitch;
  return aim(L, S, X, Y, 2.0 * ua - 1.0, 2.0 * ub - 1.0, origin, dir);
}

/* The device's path culling (lf_get_cull_table), as in lf_geo_oracle.c: with a table installed the IMAGE is still
 * the full enumeration's -- the independent evidence that what the device skips adds nothing -- while the
 * counters count the rays the device starts (block = 64 x 64 pixels, entry = the sample's pupil stratum). */
static const uint64_t* g64_cull = NULL;
static int g64_cull_bx = 0, g64_cull_cells = 0, g64_cull_shift = 6;
/* W * H * 4 doubles (or NULL): per pixel, the fragile rays' potential weight (summed over the channels, / spp) by cause --
 * aperture rim, mask texel edge, critical angle, grazing miss: what tests/test_gpu_march_f64.py tabulates */
static double* g64_cause = NULL;
void g64_set_cause_buffer(double* buf) { g64_cause = buf; }
void g64_set_cull(const uint64_t* table, int blocks_x, int blocks_y, int cells, int block_px) {
  (void)blocks_y;
  g64_cull = table; g64_cull_bx = blocks_x; g64_cull_cells = cells;
  g64_cull_shift = block_px == 128 ? 7 : block_px == 32 ? 5 : block_px == 16 ? 4 : 6;
}

/* ---- the light list (lf_set_lights / lf_set_lights_ex / lf_set_lights_geom) -------------------------------------
 * A process-global setting, off by default: n = 0 restores the single sun of g64_lens, and every result is then bit
 * for bit what it was before the list existed.  Values as the device stores them (float32 held in doubles, what
 * lf_get_lights_geom reports): kind 0 directional (geom[0..2] the direction TO the light), 1 point (geom[0..2] its
 * position, lens millimetres, front vertex at z = 0, scene at z < 0), 2 area (geom = centre, direction, e1, e2). */
#define G64_MAX_LIGHTS 8
enum { G64_DIRECTIONAL = 0, G64_POINT = 1, G64_AREA = 2 };
static int g64_n_lights = 0;
static int g64_light_kind[G64_MAX_LIGHTS];
static double g64_light_geom[G64_MAX_LIGHTS][12], g64_light_rad[G64_MAX_LIGHTS][3], g64_light_alpha[G64_MAX_LIGHTS];
void g64_set_lights(int n, const int* kinds, const double* geom, const double* radiance, const double* angular_radius) {
  g64_n_lights = 0;
  if (n <= 0 || n > G64_MAX_LIGHTS) return;
  for (int k = 0; k < n; k++) {
    g64_light_kind[k] = kinds[k];
    memcpy(g64_light_geom[k], geom + 12 * k, sizeof(g64_light_geom[k]));
    memcpy(g64_light_rad[k], radiance + 3 * k, sizeof(g64_light_rad[k]));
    g64_light_alpha[k] = angular_radius[k];
  }
  g64_n_lights = n;
}
/* The edge band of a rectangle: how far (mm, in the rectangle's plane) the float32 march's hit point can lie from
 * the float64 one.  G64_EPS_EXIT / G64_EPS_DIR are G64_EPS_FACTOR times the largest deviation of the float32 oracle's
 * exit point (mm) / unit exit direction from this tracer's (g64_exit_deviation below), over the primary path and all
 * 45 ghost pairs x 3 wavelengths of every sample ray of one 64 x 48 x 64 spp frame (key 0xE95) per lens the tests
 * install a rectangle with, fragile rays skipped (4.58e6 rays compared per lens, no fate differs):
 *   dgauss11.lens, 64 pixels of the 36 mm / 1920 sensor          7.696e-5 mm   2.237e-6
 *   dgauss11_coated.lens, the same crop                          7.696e-5 mm   2.237e-6   (a film moves no ray)
 * -> 7.70e-5 mm and 2.24e-6, times the factor 10 that eps_mm takes over the march's accumulated error.  (The ghosts
 * make these figures: the 531 rays of tests/test_geo_rays_vs_f64.py stay within 7.6e-6 mm and 1.2e-6.  Other frames
 * need their own: the 80-pixel crop 8.84e-5 mm / 2.36e-6, the full 36 mm sensor 6.5e-4 mm / 7.3e-5 -- steep ghost
 * rays -- under which the band of a 12 x 8 mm rectangle 90 mm away would no longer be the exception.)  The third term
 * is the float32 test's own rounding, 4 * 2^-24 |P - C| (tests/test_area_ghosts_cpu.py). */
#define G64_EPS_FACTOR 10.0
#define G64_EPS_EXIT (G64_EPS_FACTOR * 7.70e-5)
#define G64_EPS_DIR (G64_EPS_FACTOR * 2.24e-6)
#define G64_EPS_TEST 2.4e-7
/* per light of the list, of the last g64_trace: its (ray, light) pairs with a positive contribution, and those in its edge band */
static uint64_t g64_pairs_lit[G64_MAX_LIGHTS], g64_pairs_edge[G64_MAX_LIGHTS];
void g64_light_pairs(uint64_t lit[G64_MAX_LIGHTS], uint64_t edge[G64_MAX_LIGHTS]) {
  memcpy(lit, g64_pairs_lit, sizeof(g64_pairs_lit));
  memcpy(edge, g64_pairs_edge, sizeof(g64_pairs_edge));
}
void g64_light_eps(double out[3]) { out[0] = G64_EPS_EXIT; out[1] = G64_EPS_DIR; out[2] = G64_EPS_TEST; }

/* Is the ray (P, unit d) one that ends on the lit side of the parallelogram C + u e1 + v e2, |u|, |v| <= 1/2, which
 * emits towards dir?  The plane's intersection t = n.(C - P) / (n.d), n = e1 x e2; (u, v) of the hit point from the
 * normal equations of (e1, e2) (their Gram matrix); lit iff inside, t > 0 and d.dir < 0.  *edge: the decision is one
 * float32 may take the other way -- the hit point lies within eps_light(t) = eps_exit + t eps_dir + 2.4e-7 |P - C|
 * of one of the four edge SEGMENTS (within it of the edge's line, and not further than it beyond the segment's
 * ends), on either side, or |d.dir| < eps_cos. */
static int area_lit(const double* g, vec P, vec d, double eps_cos, int* edge) {
  const vec C = V(g[0], g[1], g[2]), dir = normalise(V(g[3], g[4], g[5]));
  const vec e1 = V(g[6], g[7], g[8]), e2 = V(g[9], g[10], g[11]);
  const vec n = V(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
  const double facing = dotp(d, dir);
  const double t = dotp(n, sub(C, P)) / dotp(n, d);
  *edge = 0;
  if (!(t > 0.0) || !(t < INFINITY)) return 0; /* parallel to the plane, or the plane lies behind: the limits of
                                                  lf_validate_light_geom keep t far from 0 for a ray leaving the lens */
  const vec w = sub(add(P, scale(d, t)), C);
  const double g11 = dotp(e1, e1), g12 = dotp(e1, e2), g22 = dotp(e2, e2), b1 = dotp(w, e1), b2 = dotp(w, e2);
  const double det = g11 * g22 - g12 * g12; /* = |e1 x e2|^2 */
  const double u = (g22 * b1 - g12 * b2) / det, v = (g11 * b2 - g12 * b1) / det;
  const int inside = fabs(u) <= 0.5 && fabs(v) <= 0.5;
  /* one unit of u moves the point |e1 x e2| / |e2| mm away from the lines u = const, one of v |e1 x e2| / |e1| */
  const double mm_u = sqrt(det / g22), mm_v = sqrt(det / g11);
  const double eps = G64_EPS_EXIT + t * G64_EPS_DIR + G64_EPS_TEST * sqrt(dotp(sub(P, C), sub(P, C)));
  const double du = (fabs(u) - 0.5) * mm_u, dv = (fabs(v) - 0.5) * mm_v; /* signed: > 0 outside */
  const int near_edge = (fabs(du) < eps && dv < eps) || (fabs(dv) < eps && du < eps);
  if (fabs(facing) < eps_cos) { *edge = inside || near_edge; return inside && facing < 0.0; }
  if (!(facing < 0.0)) return 0; /* seen from behind: black, and firmly so */
  *edge = near_edge;
  return inside;
}

/* ---- the occluder list (lf_set_ghost_occlusion / lf_set_ghost_occlusion_reach) ------------------------------------------------
 * A process-global setting, off by default: without a primitive every result is bit for bit what it was before the list
 * existed.  It acts under a light list only, as the device's occlusion does (kVarOccl comes with kVarLights).  Spheres
 * (cx, cy, cz, r) and triangles (three vertices) are WORLD coordinates; the pose (row-major c2w, pos), world_per_mm and z_ref
 * are the lens camera's.  Everything below is written from DESIGN.md section 4 ("Ghost occlusion", "The reach of a shadow
 * ray", "Area lights: occlusion") and the textbook in plain double; it shares no expression with the device's walk: no
 * tree, no boxes, no reuse of one light's answer for another. */
enum { G64_REACH_SKY = 0, G64_REACH_LIGHT = 1 };
static int g64_occl_ns = 0, g64_occl_nt = 0, g64_occl_reach = G64_REACH_SKY;
static double *g64_occl_sph = NULL, *g64_occl_tri = NULL;
static double g64_occl_c2w[9], g64_occl_pos[3], g64_occl_wpm = 1.0, g64_occl_zref = 0.0;
void g64_set_occlusion(int n_spheres, const double* spheres, int n_tris, const double* tris, const double c2w[9],
                       const double pos[3], double world_per_mm, double z_ref_mm, int reach_mode) {
  free(g64_occl_sph); free(g64_occl_tri);
  g64_occl_sph = g64_occl_tri = NULL;
  g64_occl_ns = g64_occl_nt = 0;
  if (n_spheres < 0 || n_tris < 0 || n_spheres + n_tris == 0) return;
  if (n_spheres) { g64_occl_sph = (double*)malloc(sizeof(double) * 4 * (size_t)n_spheres); memcpy(g64_occl_sph, spheres, sizeof(double) * 4 * (size_t)n_spheres); }
  if (n_tris) { g64_occl_tri = (double*)malloc(sizeof(double) * 9 * (size_t)n_tris); memcpy(g64_occl_tri, tris, sizeof(double) * 9 * (size_t)n_tris); }
  memcpy(g64_occl_c2w, c2w, sizeof(g64_occl_c2w));
  memcpy(g64_occl_pos, pos, sizeof(g64_occl_pos));
  g64_occl_wpm = world_per_mm; g64_occl_zref = z_ref_mm;
  g64_occl_reach = reach_mode == G64_REACH_LIGHT ? G64_REACH_LIGHT : G64_REACH_SKY;
  g64_occl_ns = n_spheres; g64_occl_nt = n_tris;
}
/* the contract's mapping: the exit point P (lens mm, z absolute in the prescription's coordinates) and the unit direction d
 * to the world: oc = (px wpm, py wpm, (z - z_ref) wpm), origin = pos + c2w oc, direction = c2w d */
static vec rotate(const double* m, vec v) {
  return V(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z, m[6] * v.x + m[7] * v.y + m[8] * v.z);
}
static void occl_map(vec P, vec d, vec* O, vec* D) {
  const vec oc = V(P.x * g64_occl_wpm, P.y * g64_occl_wpm, (P.z - g64_occl_zref) * g64_occl_wpm);
  *O = add(V(g64_occl_pos[0], g64_occl_pos[1], g64_occl_pos[2]), rotate(g64_occl_c2w, oc));
  *D = rotate(g64_occl_c2w, d);
}
/* where light k's shadow ray ends, world units along the unit direction: +inf under the sky's reach and for a directional
 * light; the point of the ray nearest a lamp; just before a rectangle's plane ((double)0.00001f: the reference's EPS_F) */
static double occl_reach(int k, vec P, vec d) {
  if (g64_occl_reach != G64_REACH_LIGHT || k < 0 || g64_light_kind[k] == G64_DIRECTIONAL) return INFINITY;
  const double* g = g64_light_geom[k];
  double reach;
  if (g64_light_kind[k] == G64_POINT) {
    reach = g64_occl_wpm * dotp(sub(V(g[0], g[1], g[2]), P), d);
  } else {
    const vec e1 = V(g[6], g[7], g[8]), e2 = V(g[9], g[10], g[11]);
    const vec n = V(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
    reach = g64_occl_wpm * (dotp(n, sub(V(g[0], g[1], g[2]), P)) / dotp(n, d)) - (double)0.00001f;
  }
  return reach > 0.0 ? reach : 0.0;
}
/* how far (world units) the float32 march's shadow ray can lie from this one at ray parameter t: the two measured constants */
static double occl_eps(double t) { return (G64_EPS_EXIT + (fmax(t, 0.0) / g64_occl_wpm) * G64_EPS_DIR) * g64_occl_wpm; }
/* does the ray (O, unit D) over [0, reach] pass within eps(t) of the segment [a, b]?  The closest points of the two lines
 * (the textbook's 2 x 2 system), the segment's parameter clamped to [0, 1], the ray's then taken again and clamped to t >= 0 */
static int passes_segment(vec O, vec D, double reach, vec a, vec b) {
  const vec u = sub(b, a), w0 = sub(O, a);
  const double B = dotp(D, u), C = dotp(u, u), d = dotp(D, w0), e = dotp(u, w0);
  const double denom = C - B * B;                             /* (D.D = 1) */
  double s = denom > 1e-14 * C ? (e - B * d) / denom : 0.0;   /* parallel: any point of the segment */
  s = s < 0.0 ? 0.0 : s > 1.0 ? 1.0 : s;
  double t = s * B - d;
  if (t < 0.0) t = 0.0;
  const double eps = occl_eps(t);
  if (t > reach + eps) return 0;
  const vec off = sub(add(w0, scale(D, t)), scale(u, s));
  return sqrt(dotp(off, off)) < eps;
}
/* Is something within [0, reach] of the world ray (O, unit D)?  Brute force, every primitive.  A primitive answers
 * 0 (misses), 1 (blocks, but float32 could see it miss: `near`) or 2 (blocks FIRMLY: its root lies more than eps inside
 * [0, reach] and the ray passes more than eps inside its outline).  `near` is also raised by a primitive that misses although
 * the ray passes within eps(t) of its outline -- a sphere's silhouette | |closest approach| - r | < eps, a triangle's three
 * edge segments (the distance between the ray and the segment in space: never more than the distance in the triangle's plane,
 * and the same at normal incidence, as area_lit's) -- or has its root within eps of an end of the
 * segment.  *edge: the answer is one float32 may take the other way = some primitive is `near` and none blocks firmly (a ray
 * across the shared edge of two triangles of one wall is blocked firmly by neither, and is in the band; one across a mesh's
 * inner edge behind a wall that blocks it firmly is not). */
static int occl_any_hit(vec O, vec D, double reach, int* edge) {
  int blocked = 0, firm = 0, near = 0;
  for (int i = 0; i < g64_occl_ns; i++) {
    const double* s = g64_occl_sph + 4 * i;
    const vec oc = sub(O, V(s[0], s[1], s[2]));
    const double r = s[3], b = dotp(oc, D), c = dotp(oc, oc) - r * r, disc = b * b - c;
    const double t_ca = -b;                                   /* the ray parameter of the closest approach */
    if (c > 0.0 && t_ca < -r) continue;                       /* wholly behind the origin */
    const double approach = sqrt(fmax(dotp(oc, oc) - b * b, 0.0));
    const int silhouette = fabs(approach - r) < occl_eps(t_ca) && t_ca - r <= reach + occl_eps(t_ca);
    if (silhouette) near = 1;
    if (disc < 0.0) continue;
    const double sq = sqrt(disc), t1 = -b - sq, t2 = -b + sq;
    const double t = t1 >= 0.0 ? t1 : t2;                     /* the nearer root, the farther one from inside */
    const double eps = occl_eps(t);
    const int at_end = fabs(t - reach) < eps || fabs(t) < eps || (t1 < 0.0 && fabs(t1) < eps);
    if (at_end) near = 1;
    if (t >= 0.0 && t <= reach) { blocked = 1; if (!silhouette && !at_end) firm = 1; }
  }
  for (int i = 0; i < g64_occl_nt; i++) {
    const double* p = g64_occl_tri + 9 * i;
    const vec a = V(p[0], p[1], p[2]), bb = V(p[3], p[4], p[5]), cc = V(p[6], p[7], p[8]);
    const vec e1 = sub(bb, a), e2 = sub(cc, a);
    const vec n = V(e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x);
    const double nn = sqrt(dotp(n, n)), denom = dotp(n, D);
    if (!(fabs(denom) > 1e-12 * nn)) continue;                /* parallel to the plane (or a degenerate triangle) */
    const int on_outline = passes_segment(O, D, reach, a, bb) || passes_segment(O, D, reach, bb, cc) || passes_segment(O, D, reach, cc, a);
    if (on_outline) near = 1;
    const double t = dotp(n, sub(a, O)) / denom, eps = occl_eps(t);
    if (t < -eps || t > reach + eps) continue;
    const vec q = add(O, scale(D, t)), w = sub(q, a);
    /* barycentric coordinates from the normal equations of (e1, e2) */
    const double g11 = dotp(e1, e1), g12 = dotp(e1, e2), g22 = dotp(e2, e2), b1 = dotp(w, e1), b2 = dotp(w, e2);
    const double det = g11 * g22 - g12 * g12;
    const double u = (g22 * b1 - g12 * b2) / det, v = (g11 * b2 - g12 * b1) / det;
    const int inside = u >= 0.0 && v >= 0.0 && u + v <= 1.0;
    const int at_end = fabs(t - reach) < eps || fabs(t) < eps;
    if (on_outline || (inside && at_end)) near = 1;
    if (inside && t >= 0.0 && t <= reach) { blocked = 1; if (!on_outline && !at_end) firm = 1; }
  }
  *edge = near && !firm;
  return blocked;
}
/* per light of the list, of the last g64_trace under occlusion: the (ray, light) pairs tested (those that would contribute),
 * of those blocked, and those in the occluders' edge band; total[3] the sums */
static uint64_t g64_occl_tested[G64_MAX_LIGHTS], g64_occl_blocked[G64_MAX_LIGHTS], g64_occl_edge[G64_MAX_LIGHTS];
void g64_occlusion_pairs(uint64_t total[3], uint64_t tested[G64_MAX_LIGHTS], uint64_t blocked[G64_MAX_LIGHTS],
                         uint64_t edge[G64_MAX_LIGHTS]) {
  total[0] = total[1] = total[2] = 0;
  for (int k = 0; k < G64_MAX_LIGHTS; k++) {
    total[0] += g64_occl_tested[k]; total[1] += g64_occl_blocked[k]; total[2] += g64_occl_edge[k];
    if (tested) tested[k] = g64_occl_tested[k];
    if (blocked) blocked[k] = g64_occl_blocked[k];
    if (edge) edge[k] = g64_occl_edge[k];
  }
}
/* for the anchors: one exit ray (P lens mm, d any length) against the installed occluders, for light k of the installed list
 * (k < 0: the sky's reach).  out = {world origin xyz, world direction xyz, reach, in the edge band}; returns blocked */
int g64_occlusion_ray(const double p[3], const double d[3], int k, double out[8]) {
  const vec P = V(p[0], p[1], p[2]), dn = normalise(V(d[0], d[1], d[2]));
  vec O, D;
  int edge = 0;
  occl_map(P, dn, &O, &D);
  const double reach = occl_reach(k < g64_n_lights ? k : -1, P, dn);
  const int blocked = (g64_occl_ns + g64_occl_nt) ? occl_any_hit(O, D, reach, &edge) : 0;
  out[0] = O.x; out[1] = O.y; out[2] = O.z; out[3] = D.x; out[4] = D.y; out[5] = D.z; out[6] = reach; out[7] = (double)edge;
  return blocked;
}

/* image, frag: W*H*3 doubles (rows [y0, y1) are written); counters: launched, events, clipped at
 * the stop, vignetted, totally reflected, reached the scene, hit the light ((ray, light) pairs under a list),
 * fragile rays.  The array a caller passes keeps its EIGHT slots -- a binding written before the light list existed
 * allocates no more -- and the ninth counter, the (ray, light) pairs whose lit-or-unlit decision lies in a rectangle's
 * edge band, is read with g64_light_edge_pairs() after the call. */
static uint64_t g64_edge_pairs_last = 0;
uint64_t g64_light_edge_pairs(void) { return g64_edge_pairs_last; }
void g64_trace(const g64_lens* L, int W, int H, int y0, int y1, int spp, const uint32_t key[2],
               int sub_bits, const int* pairs, int n_pairs, const float* mask, int mw, int mh,
               double* image, double* frag, uint64_t counters[8], int n_threads) {
  g64_system S;
  lay_out(L, &S);
  const double lobe = 1.0 / (1.0 - cos(L->sun_angular_radius));
  const vec sun = normalise(V(L->sun_dir[0], L->sun_dir[1], L->sun_dir[2])); /* the angle is between directions */
  /* the list's directional lights and lobes, formed as the sun's are */
  const int n_lights = g64_n_lights;
  vec to_light[G64_MAX_LIGHTS];
  double lobe_of[G64_MAX_LIGHTS];
  for (int k = 0; k < n_lights; k++) {
    to_light[k] = normalise(V(g64_light_geom[k][0], g64_light_geom[k][1], g64_light_geom[k][2]));
    lobe_of[k] = 1.0 / (1.0 - cos(g64_light_alpha[k]));
  }
  uint64_t total[9] = {0};
  memset(g64_pairs_lit, 0, sizeof(g64_pairs_lit));
  memset(g64_pairs_edge, 0, sizeof(g64_pairs_edge));
  memset(g64_occl_tested, 0, sizeof(g64_occl_tested));
  memset(g64_occl_blocked, 0, sizeof(g64_occl_blocked));
  memset(g64_occl_edge, 0, sizeof(g64_occl_edge));
  const int occluders = g64_occl_ns + g64_occl_nt > 0;
  if (n_threads < 1) n_threads = 1;
  int G = (int)floor(sqrt((double)spp));
  while ((G + 1) * (G + 1) <= spp) G++;
  while (G * G > spp) G--;
  const int GG = G * G;
#pragma omp parallel num_threads(n_threads)
  {
    uint64_t counted[9] = {0}, skipped[9] = {0}, lit_k[G64_MAX_LIGHTS] = {0}, edge_k[G64_MAX_LIGHTS] = {0};
    uint64_t tested_k[G64_MAX_LIGHTS] = {0}, blocked_k[G64_MAX_LIGHTS] = {0}, oedge_k[G64_MAX_LIGHTS] = {0};
#pragma omp for schedule(dynamic, 16)
    for (long long p = (long long)y0 * W; p < (long long)y1 * W; p++) {
      const int x = (int)(p % W), y = (int)(p / W);
      if (x < g64_x0 || x >= g64_x1) continue;
      double sum[3] = {0, 0, 0}, fsum[3] = {0, 0, 0};
      for (int s = 0; s < spp; s++) {
        vec o, d;
        const double w0 = sample_ray(L, &S, W, H, x, y, s, spp, sub_bits, key, &o, &d);
        uint64_t started = ~(uint64_t)0;
        if (g64_cull) {
          /* P = G m table cells per axis; the cell of the sub-cell the pixel's wave tile aims sample s at */
          int entry = g64_cull_cells;
          const int P = (int)(sqrt((double)g64_cull_cells) + 0.5), m = P / G;
          if (s >= GG) {
            entry = g64_cull_cells;                 /* an unstratified sample: the block's union entry */
          } else if ((1 << sub_bits) < m) {         /* the cell of the pixel's own pupil point (the device: in float) */
            int fx = (int)(t64_ua * P), fy = (int)(t64_ub * P);
            if (fx > P - 1) fx = P - 1;
            if (fy > P - 1) fy = P - 1;
            entry = fy * P + fx;
          } else {
            const int cy = s / G, cx = s % G;
            const int per_block = 1 << g64_xs, block_w = 8 * per_block;
            const int tiles_x = ((W + block_w - 1) / block_w) * per_block;
            const uint32_t c2[4] = {(uint32_t)((y / 8) * tiles_x + (x / block_w) * per_block + x % per_block), (uint32_t)s, 0x51bce110u, 0u};
            uint32_t r2[4];
            philox64(c2, key, r2);
            const uint32_t sxi = sub_bits ? (r2[0] >> (32 - sub_bits)) : 0u, syi = sub_bits ? (r2[1] >> (32 - sub_bits)) : 0u;
            entry = (cy * m + (int)((syi * (uint32_t)m) >> sub_bits)) * P + cx * m + (int)((sxi * (uint32_t)m) >> sub_bits);
          }
          started = g64_cull[((size_t)(y >> g64_cull_shift) * g64_cull_bx + (x >> g64_cull_shift)) * (size_t)(g64_cull_cells + 1) + (size_t)entry];
        }
        for (int lam = 0; lam < L->n_lambda; lam++)
          for (int q = 0; q < n_pairs; q++) {
            uint64_t* const c = (q >= 64 || ((started >> q) & 1u)) ? counted : skipped;
            g64_ray r = {o, d, w0, w0, 0, 0, 0};
            c[0]++;
            c[1] += (uint64_t)follow(L, &S, lam, pairs[2 * q], pairs[2 * q + 1], mask, mw, mh, &r);
            if (r.fragile) c[7]++;
            if (r.dead == 1) c[2]++;
            else if (r.dead == 2) c[3]++;
            else if (r.dead == 3) c[4]++;
            else c[5]++;
            if (r.dead && !r.fragile) continue;
            if (n_lights > 0) {
              /* the list: every light tests the ray at its own exit point r.o along r.d; contributions add */
              const vec dn = normalise(r.d);
              for (int k = 0; k < n_lights; k++) {
                double shade = 1.0; /* a fragile ray that could not be followed: bound by its weight, for every light */
                int edge = 0, in = 1;
                if (r.fragile != 2) {
                  if (g64_light_kind[k] == G64_AREA) {
                    in = area_lit(g64_light_geom[k], r.o, dn, L->eps_cos, &edge);
                    if (!in && !edge) continue;
                  } else {
                    const vec s = g64_light_kind[k] == G64_POINT
                                      ? normalise(sub(V(g64_light_geom[k][0], g64_light_geom[k][1], g64_light_geom[k][2]), r.o))
                                      : to_light[k];
                    const double qq = (1.0 - dotp(dn, s)) * lobe_of[k];
                    if (!(qq < 1.0)) continue;
                    shade = (1.0 - qq) * (1.0 - qq);
                  }
                }
                /* the occluders: a pair that would contribute is tested over [0, reach_k], each light on its own */
                int blocked = 0, occl_edge = 0;
                if (occluders && !r.dead && in && r.w * shade > 0.0) {
                  vec O, D;
                  occl_map(r.o, dn, &O, &D);
                  blocked = occl_any_hit(O, D, occl_reach(k, r.o, dn), &occl_edge);
                  if (c == counted) { tested_k[k]++; blocked_k[k] += (uint64_t)blocked; oedge_k[k] += (uint64_t)occl_edge; }
                }
                if (!r.dead && in && !blocked && r.w * shade > 0.0) { c[6]++; if (c == counted) lit_k[k]++; }
                if (!r.dead && edge && r.w > 0.0) { c[8]++; if (c == counted) edge_k[k]++; }
                for (int ch = 0; ch < 3; ch++) {
                  const double colour = g64_light_rad[k][ch] * L->lambda_rgb[lam][ch];
                  if (!r.dead && in && !blocked) sum[ch] += r.w * shade * colour;
                  if (r.fragile) fsum[ch] += r.w_pot * shade * colour;
                  else if (edge || occl_edge) fsum[ch] += r.w * colour; /* whichever way float64 decided */
                  if (r.slope > 0.0) fsum[ch] += r.slope * shade * colour;
                  if (r.fragile && g64_cause)
                    for (int b = 0; b < 4; b++)
                      if (r.cause & (1 << b)) g64_cause[4 * (size_t)p + b] += r.w_pot * shade * colour / spp;
                }
              }
              continue;
            }
            double shade = 1.0; /* a fragile ray that could not be followed: bound by its weight */
            if (r.fragile != 2) {
              const double qq = (1.0 - dotp(normalise(r.d), sun)) * lobe;
              if (!(qq < 1.0)) continue;
              shade = (1.0 - qq) * (1.0 - qq);
            }
            if (!r.dead && r.w * shade > 0.0) c[6]++;
            for (int ch = 0; ch < 3; ch++) {
              const double colour = L->sun_radiance[ch] * L->lambda_rgb[lam][ch];
              if (!r.dead) sum[ch] += r.w * shade * colour;
              if (r.fragile) fsum[ch] += r.w_pot * shade * colour;
              if (r.slope > 0.0) fsum[ch] += r.slope * shade * colour;
              /* ... and by cause (a ray with several: each of them), if the caller asked (g64_set_cause_buffer) */
              if (r.fragile && g64_cause)
                for (int k = 0; k < 4; k++)
                  if (r.cause & (1 << k)) g64_cause[4 * (size_t)p + k] += r.w_pot * shade * colour / spp;
            }
          }
      }
      for (int ch = 0; ch < 3; ch++) {
        image[3 * p + ch] = sum[ch] / spp;
        frag[3 * p + ch] = fsum[ch] / spp;
      }
    }
#pragma omp critical
    {
      for (int k = 0; k < 9; k++) total[k] += counted[k];
      for (int k = 0; k < G64_MAX_LIGHTS; k++) { g64_pairs_lit[k] += lit_k[k]; g64_pairs_edge[k] += edge_k[k]; }
      for (int k = 0; k < G64_MAX_LIGHTS; k++) {
        g64_occl_tested[k] += tested_k[k]; g64_occl_blocked[k] += blocked_k[k]; g64_occl_edge[k] += oedge_k[k];
      }
    }
  }
  if (counters) memcpy(counters, total, 8 * sizeof(total[0]));
  g64_edge_pairs_last = total[8];
}

/* How far a float32 march's exit ray lies from this tracer's (what G64_EPS_EXIT / G64_EPS_DIR are measured with).
 * The sample rays of a W x H x spp frame, each start ray rounded to float32 and handed both to `f32` -- the float32
 * oracle's single-ray entry (geo_trace_ray of lf_geo_oracle.c, passed in by the caller with its own lens record:
 * nothing here links against it) -- and to follow(), along every listed path and wavelength.  Rays this tracer flags
 * fragile are skipped, and so are rays either side loses.  out = {largest |delta exit point| (mm, max norm), largest
 * |delta unit exit direction| (max norm), rays compared, rays whose fates differ although not fragile} */
typedef int (*g64_f32_ray_fn)(const void* L32, int lam, int i, int j, float p[3], float d[3], float* w, const float* mask,
                              int mw, int mh, int* n_events);
void g64_exit_deviation(const g64_lens* L, const void* L32, g64_f32_ray_fn f32, int W, int H, int spp, const uint32_t key[2],
                        int sub_bits, const int* pairs, int n_pairs, const float* mask, int mw, int mh, int n_threads,
                        double out[4]) {
  g64_system S;
  lay_out(L, &S);
  double worst_p = 0.0, worst_d = 0.0, n_cmp = 0.0, n_fate = 0.0;
  if (n_threads < 1) n_threads = 1;
#pragma omp parallel for schedule(dynamic, 16) num_threads(n_threads) reduction(max : worst_p, worst_d) reduction(+ : n_cmp, n_fate)
  for (long long p = 0; p < (long long)H * W; p++) {
    const int x = (int)(p % W), y = (int)(p / W);
    for (int s = 0; s < spp; s++) {
      vec o, d;
      sample_ray(L, &S, W, H, x, y, s, spp, sub_bits, key, &o, &d);
      const float o32[3] = {(float)o.x, (float)o.y, (float)o.z}, d32[3] = {(float)d.x, (float)d.y, (float)d.z};
      for (int lam = 0; lam < L->n_lambda; lam++)
        for (int q = 0; q < n_pairs; q++) {
          g64_ray r = {V(o32[0], o32[1], o32[2]), V(d32[0], d32[1], d32[2]), 1.0, 1.0, 0, 0, 0};
          follow(L, &S, lam, pairs[2 * q], pairs[2 * q + 1], mask, mw, mh, &r);
          if (r.fragile) continue;
          float pf[3] = {o32[0], o32[1], o32[2]}, df[3] = {d32[0], d32[1], d32[2]}, wf = 1.0f;
          int ev;
          const int st = f32(L32, lam, pairs[2 * q], pairs[2 * q + 1], pf, df, &wf, mask, mw, mh, &ev);
          if ((st != 0) != (r.dead != 0)) { n_fate += 1.0; continue; }
          if (st != 0) continue;
          const vec d64 = normalise(r.d), d32n = normalise(V(df[0], df[1], df[2]));
          const double ep = fmax(fabs(pf[0] - r.o.x), fmax(fabs(pf[1] - r.o.y), fabs(pf[2] - r.o.z)));
          const double ed = fmax(fabs(d32n.x - d64.x), fmax(fabs(d32n.y - d64.y), fabs(d32n.z - d64.z)));
          if (ep > worst_p) worst_p = ep;
          if (ed > worst_d) worst_d = ed;
          n_cmp += 1.0;
        }
    }
  }
  out[0] = worst_p; out[1] = worst_d; out[2] = n_cmp; out[3] = n_fate;
}

/* The lens camera of the scene term (lf_set_lens_camera): the primary path of sample s = 0 .. ns-1 of the
 * listed pixels at wavelength `lam`, in float64 with the textbook formulations above.
 * out: n_pix x ns x 10 doubles {origin xyz on the front element (mm, lens space), unit direction xyz,
 * weight as float64 decides (0 when blocked), weight if every fragile decision passes, fragile, dead} */
void g64_lens_samples(const g64_lens* L, int W, int H, int ns, const uint32_t key[2], int sub_bits, int lam,
                      const int* pixels, int n_pix, const float* mask, int mw, int mh, double* out) {
  g64_system S;
  lay_out(L, &S);
  for (int i = 0; i < n_pix; i++) {
    const int p = pixels[i], x = p % W, y = p / W;
    for (int s = 0; s < ns; s++) {
      vec o, d;
      const double w0 = sample_ray(L, &S, W, H, x, y, s, ns, sub_bits, key, &o, &d);
      g64_ray r = {o, d, w0, w0, 0, 0};
      follow(L, &S, lam, -1, -1, mask, mw, mh, &r);
      double* q = out + 10 * ((size_t)i * ns + s);
      const vec dn = normalise(r.d);
      q[0] = r.o.x; q[1] = r.o.y; q[2] = r.o.z; q[3] = dn.x; q[4] = dn.y; q[5] = dn.z;
      q[6] = r.dead ? 0.0 : r.w; q[7] = r.w_pot + r.slope; q[8] = (double)r.fragile; q[9] = (double)r.dead;
    }
  }
}

/* lf_generate_lens_rays in float64: the primary paths from n sensor points xy (mm) through the pupil-square
 * points uv in [-1, 1]^2 (both the float32 values the device is given); out: n x 10 as g64_lens_samples */
void g64_lens_rays(const g64_lens* L, int lam, int n, const float* xy, const float* uv, const float* mask, int mw,
                   int mh, double* out) {
  g64_system S;
  lay_out(L, &S);
  for (int i = 0; i < n; i++) {
    vec o, d;
    const double w0 = aim(L, &S, xy[2 * i], xy[2 * i + 1], uv[2 * i], uv[2 * i + 1], &o, &d);
    g64_ray r = {o, d, w0, w0, 0, 0};
    follow(L, &S, lam, -1, -1, mask, mw, mh, &r);
    double* q = out + 10 * (size_t)i;
    const vec dn = normalise(r.d);
    q[0] = r.o.x; q[1] = r.o.y; q[2] = r.o.z; q[3] = dn.x; q[4] = dn.y; q[5] = dn.z;
    q[6] = r.dead ? 0.0 : r.w; q[7] = r.w_pot + r.slope; q[8] = (double)r.fragile; q[9] = (double)r.dead;
  }
}
