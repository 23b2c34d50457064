// lf_march_events.h -- the surface events of the geometric lens march, shared by
// the ghost march (lf_march.hip: k_march, k_lens_rays) and by the lens-imaged scene term
// (lf_scene.hip: k_scene_term<.., LENS = true>, round 4): ONE definition of the float32 event
// arithmetic, so that the primary path of a sensor sample is the same bits wherever it is marched.
// Device code only; nothing here is part of the ABI.
#pragma once

#include <type_traits>

#include "lf_internal.h"

namespace lfm {

constexpr unsigned kDomainMarch = 0x6e5f1a2eu;
constexpr unsigned kDomainSubcell = 0x51bce110u;

__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    unsigned hi0 = __umulhi(0xD2511F53u, ctr.x), lo0 = 0xD2511F53u * ctr.x;
    unsigned hi1 = __umulhi(0xCD9E8D57u, ctr.z), lo1 = 0xCD9E8D57u * ctr.z;
    ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
    key.x += 0x9E3779B9u;
    key.y += 0xBB67AE85u;
  }
  return ctr;
}

// Square roots are the hardware's v_sqrt_f32: one transcendental-rate instruction, accurate to 1 ulp.
// A correctly rounded root costs 8 more VALU instructions (the +-1 ulp residual test), and the two
// roots of a surface event would then be 18 of its 48 instructions.  v_sqrt_f32 is deterministic
// and its deviation from the correctly rounded root depends only on the significand and the parity
// of the exponent, so the CPU oracle reproduces it exactly from a table measured once through
// lf_native_sqrt (oracle/lf_geo_oracle.c, geo_set_sqrt_table): the march stays bit-for-bit
// comparable with the oracle.
__device__ __forceinline__ float lf_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }

// Divisions on the per-event / per-sample path are multiplications by the hardware reciprocal v_rcp_f32
// (1 ulp; one quarter-rate instruction + a multiply where the IEEE division is ~10 instructions around the
// same v_rcp: round 4, the stop event's division alone was 2.2 % of the bench frame).  Like v_sqrt_f32 the
// instruction is deterministic and its deviation from the correctly rounded reciprocal depends only on the
// significand, so the CPU oracle follows it exactly through a table measured once (lf_native_rcp,
// geo_set_rcp_table).  The rare divisions whose accuracy matters most -- the weight's wn / wd and the lobe
// factor -- stay IEEE (__fdiv_rn).
__device__ __forceinline__ float lf_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

__device__ __forceinline__ float u01(unsigned r) { return (float)(r >> 8) * 5.9604644775390625e-8f; }

// ---- a coated interface ("coatings") -----------------------------------------
// cos(2 pi x) with a fixed polynomial, never v_cos_f32 (whose argument reduction is the hardware's): the exact
// reduction y = x - rint(x), |y| folded into [0, 1/4] with a sign (1/2 - |y| is exact there), then an even
// polynomial in b^2 (max error 1.1e-7 on [0, 1/4] in float).  Host and device: lf_coating_reflectance runs it too.
__host__ __device__ inline float lf_cos2pi(float x) {
  const float a = fabsf(x - rintf(x));
  const bool far = a > 0.25f;
  const float b = far ? 0.5f - a : a;
  const float z = b * b;
  const float c = fmaf(z, fmaf(z, fmaf(z, fmaf(z, fmaf(z, -24.9823456f, 60.1440353f), -85.4535751f), 64.9393463f),
                               -19.7392082f), 1.0f);
  return far ? -c : c;
}
// sin(2 pi x), the same way: the exact reduction y = x - rint(x), |y| folded into [0, 1/4] (sin 2 pi (1/2 - b) = sin 2 pi b:
// no sign change in the fold, the sign is y's), then a fixed odd polynomial b q(b^2) (max error 2.0e-7 on [0, 1/4] in
// float; 6.5e-8 of it is the polynomial's own, the rest the rounding of the Horner steps near sin = 1).  Never v_sin_f32.
__host__ __device__ inline float lf_sin2pi(float x) {
  const float y = x - rintf(x);
  const float a = fabsf(y);
  const float b = a > 0.25f ? 0.5f - a : a;
  const float z = b * b;
  const float s = b * fmaf(z, fmaf(z, fmaf(z, fmaf(z, fmaf(z, -14.3368559f, 41.9999619f), -76.7036667f), 81.6052094f),
                                -41.3417015f), 6.28318548f);
  return y < 0.0f ? -s : s;
}
__host__ __device__ inline float lf_coat_sqrt(float x) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_sqrtf(x);
#else
  return sqrtf(x);
#endif
}
// The unpolarised reflectance of a single film (index m, thickness d) between the media n and n', as ONE fraction
// Rn / Rd, from the optical cosines of the event: sq = n |cos t| (incidence), ct = n' cos t' (exit) and the film's
// cm = sqrt(sq^2 + dm).  Per polarisation the Airy sum r = (r01 + r12 e^{i delta}) / (1 + r01 r12 e^{i delta}) with
// r01 = a / b, r12 = e / f, C = cos delta = cos 2 pi (ph cm):  |r|^2 = N / D,
//   N = (a f)^2 + (e b)^2 + 2 (a b)(e f) C,   D = (b f)^2 + (a e)^2 + 2 (a b)(e f) C,
// amplitudes scaled by the row constants so that b = f = 1 at normal incidence (as fs / fo / fi scale the bare
// fraction); then Rn = Ns Dp + Np Ds, Rd = 2 Ds Dp.  Nothing is divided.
__host__ __device__ inline void coated_fraction(float sq, float ct, const LfCoatK& k, float& Rn, float& Rd,
                                                float* Ns_ = nullptr, float* Ds_ = nullptr, float* Np_ = nullptr,
                                                float* Dp_ = nullptr) {
  const float cm = lf_coat_sqrt(fmaxf(fmaf(sq, sq, k.dm), 0.0f));
  const float C = lf_cos2pi(k.ph * cm);
  float N[2], D[2];
#pragma unroll
  for (int p = 0; p < 2; p++) {
    float a, b, e, f;
    if (p == 0) {   // s
      a = (sq - cm) * k.s01; b = (sq + cm) * k.s01;
      e = (cm - ct) * k.s12; f = (cm + ct) * k.s12;
    } else {        // p
      const float u = k.p01b * cm, v = k.p12b * ct;
      a = fmaf(k.p01a, sq, -u); b = fmaf(k.p01a, sq, u);
      e = fmaf(k.p12a, cm, -v); f = fmaf(k.p12a, cm, v);
    }
    const float af = a * f, eb = e * b, bf = b * f, ae = a * e;
    const float x = 2.0f * ((a * b) * (e * f)) * C;
    N[p] = fmaf(af, af, fmaf(eb, eb, x));
    D[p] = fmaf(bf, bf, fmaf(ae, ae, x));
  }
  Rn = fmaf(N[0], D[1], N[1] * D[0]);
  Rd = 2.0f * (D[0] * D[1]);
  if (Ns_) { *Ns_ = N[0]; *Ds_ = D[0]; *Np_ = N[1]; *Dp_ = D[1]; }
}

// The unpolarised reflectance of a STACK of N lossless layers between the media n and n' (lf_set_lens_coating_stacks), as
// one fraction Rn / Rd like the single film's, from the same optical cosines sq and ct.  Layer i (i = 0 the one the ray
// meets first) has cm_i = sqrt(sq^2 + dm_i), dm_i = m_i^2 - n^2, and the round-trip phase delta_i = 2 pi ph_i cm_i,
// ph_i = 2 d_i / lambda.  The recursive Airy (Rouard) form, from the interface FARTHEST from the arriving ray: the complex
// amplitude reflected by what lies behind a layer is carried as numerator and denominator (P, Q) -- nothing is divided --
// starting at the last interface's a / b; crossing layer i and the interface in front of it (amplitude a / b, real)
//   P' = a Q + b P e^{i delta_i},   Q' = b Q + a P e^{i delta_i}
// per polarisation; |r|^2 = |P|^2 / |Q|^2, then Rn = Ns Dp + Np Ds, Rd = 2 Ds Dp.  The amplitudes are scaled by the
// record's constants so that every b is 1 at normal incidence (|Q| stays near 1), as coated_fraction's are.
// The record (lf_stack_constants, dwords): [0] N; [1 + 5 i ..] dm_i, ph_i and the scales s, pa, pb of the interface in
// FRONT of layer i; [1 + 5 N ..] the last interface's s, pa, pb.  ld(i) loads dword i -- a wave-uniform scalar load in
// the re-march, a plain load where the wavelength differs between lanes, an array on the host -- INSIDE the loop: its trip
// count is wave-uniform, and the live vector state is P and Q (complex, s and p: eight floats) and the previous cm,
// whatever N is.  Host and device: lf_coating_stack_reflectance runs it too.
__host__ __device__ inline float lf_bits_float(int v) { return __builtin_bit_cast(float, v); }
template <class LD>
__host__ __device__ inline void stack_fraction(float sq, float ct, const LD& ld, float& Rn, float& Rd,
                                               float* Ns_ = nullptr, float* Ds_ = nullptr, float* Np_ = nullptr,
                                               float* Dp_ = nullptr) {
  const int N = ld(0);
  const int last = 1 + 5 * N;
  float cm = lf_coat_sqrt(fmaxf(fmaf(sq, sq, lf_bits_float(ld(last - 5))), 0.0f));   // the farthest layer's
  float Psr, Psi = 0.0f, Qsr, Qsi = 0.0f, Ppr, Ppi = 0.0f, Qpr, Qpi = 0.0f;
  {
    const float s = lf_bits_float(ld(last)), pa = lf_bits_float(ld(last + 1)), pb = lf_bits_float(ld(last + 2));
    Psr = (cm - ct) * s; Qsr = (cm + ct) * s;
    const float v = pb * ct;
    Ppr = fmaf(pa, cm, -v); Qpr = fmaf(pa, cm, v);
  }
  for (int i = N - 1; i >= 0; --i) {   // wave-uniform
    const int o = 1 + 5 * i;
    const float ph = lf_bits_float(ld(o + 1)), s = lf_bits_float(ld(o + 2));
    const float pa = lf_bits_float(ld(o + 3)), pb = lf_bits_float(ld(o + 4));
    const float dprev = lf_bits_float(ld(i > 0 ? o - 5 : o));   // (layer i - 1's dm; unused in front of the first layer)
    const float x = ph * cm;
    const float C = lf_cos2pi(x), S = lf_sin2pi(x);
    // the optical cosine in front of the layer: the previous layer's, or the event's own in the medium of arrival
    const float cp = i > 0 ? lf_coat_sqrt(fmaxf(fmaf(sq, sq, dprev), 0.0f)) : sq;
    const float as = (cp - cm) * s, bs = (cp + cm) * s;
    const float u = pb * cm;
    const float ap = fmaf(pa, cp, -u), bp = fmaf(pa, cp, u);
    const float Esr = fmaf(Psr, C, -(Psi * S)), Esi = fmaf(Psr, S, Psi * C);
    const float Epr = fmaf(Ppr, C, -(Ppi * S)), Epi = fmaf(Ppr, S, Ppi * C);
    Psr = fmaf(as, Qsr, bs * Esr); Psi = fmaf(as, Qsi, bs * Esi);
    const float qsr = fmaf(bs, Qsr, as * Esr), qsi = fmaf(bs, Qsi, as * Esi);
    Ppr = fmaf(ap, Qpr, bp * Epr); Ppi = fmaf(ap, Qpi, bp * Epi);
    const float qpr = fmaf(bp, Qpr, ap * Epr), qpi = fmaf(bp, Qpi, ap * Epi);
    Qsr = qsr; Qsi = qsi; Qpr = qpr; Qpi = qpi;
    cm = cp;
  }
  const float Ns = fmaf(Psr, Psr, Psi * Psi), Ds = fmaf(Qsr, Qsr, Qsi * Qsi);
  const float Np = fmaf(Ppr, Ppr, Ppi * Ppi), Dp = fmaf(Qpr, Qpr, Qpi * Qpi);
  Rn = fmaf(Ns, Dp, Np * Ds);
  Rd = 2.0f * (Ds * Dp);
  if (Ns_) { *Ns_ = Ns; *Ds_ = Ds; *Np_ = Np; *Dp_ = Dp; }
}

// ---- the filtered stop mask ("mask filter") -------------------------------------
// The bilinear lookup of LF_MASK_BILINEAR at texel coordinates (fu, fv) (texel i has its centre at i + 0.5):
// the value a the weight is multiplied by, and whether the ray survives: ANY of the four texels open, not
// a > 0 (the geometry-only march reads that from the support texture, and both must agree).  The indices are
// clamped BEFORE the loads: a dead lane's NaN never addresses outside the texture.  Host and device:
// lf_mask_lookup runs it too.
__host__ __device__ inline bool lf_mask_bilinear(const float* __restrict__ mask, int mw, int mh, float fu, float fv,
                                                 float& a) {
  const float gx = fu - 0.5f, gy = fv - 0.5f;
  const float bx = floorf(gx), by = floorf(gy);
  const float fx = gx - bx, fy = gy - by;
  // clamped as floats, before the conversion (fmaxf drops a NaN: texel 0, as anywhere left of it)
  const int ix = (int)fminf(fmaxf(bx, -1.0f), (float)mw), iy = (int)fminf(fmaxf(by, -1.0f), (float)mh);
  const int x0 = ix < 0 ? 0 : ix > mw - 1 ? mw - 1 : ix, x1 = ix + 1 > mw - 1 ? mw - 1 : ix + 1;
  const int y0 = iy < 0 ? 0 : iy > mh - 1 ? mh - 1 : iy, y1 = iy + 1 > mh - 1 ? mh - 1 : iy + 1;
  const float t00 = fmaxf(mask[y0 * mw + x0], 0.0f), t10 = fmaxf(mask[y0 * mw + x1], 0.0f);
  const float t01 = fmaxf(mask[y1 * mw + x0], 0.0f), t11 = fmaxf(mask[y1 * mw + x1], 0.0f);
  const float a0 = fmaf(fx, t10 - t00, t00), a1 = fmaf(fx, t11 - t01, t01);
  a = fmaf(fy, a1 - a0, a0);
  return fmaxf(fmaxf(t00, t10), fmaxf(t01, t11)) > 0.0f;
}

// The transmitted weight is carried as a fraction wn / wd: every Fresnel factor is a ratio of
// two cheap products, so the march multiplies numerators and denominators separately and divides
// ONCE, and only for the ~0.4 % of rays that end inside the sun's lobe.
// Position: (px, py) and hz = z RELATIVE to the vertex of the interface the ray sits on (0 on the
// sensor / the stop plane), plus r2 = px^2 + py^2 of that point, which the previous event's aperture
// test has already computed and the next event's |o|^2 reuses.  A row carries dzv = (vertex z of the
// interface the ray comes from) - (vertex z of this one): one add gives the origin's z in this
// interface's frame, absolute z never exists (3 vector instructions per event less than tracking it,
// and less cancellation).  (dx, dy, dz) is the OPTICAL direction K = n d (see surface_event).
struct Ray {
  float px, py, hz, r2, dx, dy, dz, wn, wd;
};

// One glass-surface event, straight-line (no divergent branches): a lane that misses the surface,
// leaves the clear aperture or is totally reflected just gets ok = false -- its ray state turns
// into garbage/NaN that nobody reads again.  Liveness is kept as explicit 64-bit wave masks (one
// SGPR pair, plain s_and/s_or), not as per-lane bools: the compiler lowers loop-carried bools to
// exec-merge triples that tripled the scalar-unit load of the loop.  geom_ok tells a vignetted ray
// from a TIR one.
// sgn = +1 for a ray travelling +z, -1 for -z (wave-uniform, lives in an SGPR).
typedef unsigned long long lanemask;

// W = false is the geometry-only march (positions, directions, liveness); W = true additionally
// carries the Fresnel / aperture weight.  The frame runs W = false for every ray and repeats the
// sequence with W = true only for the waves in which some lane ended inside the sun's lobe (~1 % of
// the wave-sequences): the weight is ~16 vector instructions on top of an event's 27 and is read by
// 0.4 % of the rays.  Both instantiations do the same arithmetic on the ray itself, so the
// repeated march reproduces the first one bit for bit.
// ch = c / 2 and c2 = 2 c travel with the row (exact scalings): F = c |o|^2 - 2 o_z is formed as its
// half Fh = fma(ch, |o|^2, -o_z) -- the same bits, shifted by one exponent.
//
// The direction is the OPTICAL direction K = n d (|K| = n, the index of the medium the ray is in: a
// property of the row).  With the ray o + s K the vertex-form quadratic is
//   c n^2 s^2 - 2 s G + F = 0,   G = K_z - c (o . K)
// so disc = G^2 - (c n^2) F, the root next to the vertex is s = (G - sgn sqrt(disc)) R / n^2 for a
// curved interface and s = F / (G + sgn sqrt(disc)) for flat glass, and with N = (-c hx, -c hy,
// 1 - c hz) the unit normal at the hit, K . N = G - c n^2 s = sgn sqrt(disc) EXACTLY: sqrt(disc) is
// n |cos(incidence)|.  Snell: (n' cos t')^2 = disc + (n'^2 - n^2) -- one add, negative = total
// reflection -- and K' = K + sgn (n' cos t' - n cos t) N: no multiplication of K by an index ratio.
// Per event that is 27 vector instructions where the unit-direction form of rounds 1-2 had 31.
// cn22 = 2 c n^2, rn2 = R / n^2, delta = n'^2 - n^2, sc = sgn c come with the row.
// W = true additionally takes the Fresnel scale factors fs, fo, fi of the row (LfWeightRow) and where the
// row's film constants are, if it has any (CT: NoCoat, CoatRec, CoatPrimary below).  A coated row takes
// coated_fraction instead of the bare fraction behind a wave-uniform branch; a bare row runs the bare
// fraction as it always has.  NoCoat compiles to the bare event alone: the kernels are instantiated twice,
// and only a lens with a film launches the variant that can evaluate one (its temporaries, inlined in the
// re-march, would raise the register pressure of the shared-leg kernel for every frame: DESIGN.md section 4).
// A kernel whose variant has bit kVarStack as well (launched only for a lens with a STACK of two or more layers on some
// interface: lf_set_lens_coating_stacks) passes StackRec / StackPrimary: stacked() tells, wave-uniformly and from the dword
// the row has loaded anyway, a stack record from a film's LfCoatK, and a stacked row takes stack_fraction behind a second
// wave-uniform branch.  For every other CT stacked() is a constant false and the branch is not compiled.
struct NoStack {
  __device__ __forceinline__ int operator()(int) const { return 0; }
};
struct NoCoat {
  NoCoat() = default;
  __device__ __forceinline__ NoCoat(const void*, int, int) {}
  __device__ __forceinline__ bool on() const { return false; }
  __device__ __forceinline__ LfCoatK get() const { return LfCoatK{}; }
  __device__ __forceinline__ bool stacked() const { return false; }
  __device__ __forceinline__ NoStack stack() const { return NoStack{}; }
};
template <bool W, class CT = NoCoat>
__device__ __forceinline__ lanemask surface_event(Ray& r, float dzv, float c, float ch, float c2, float sc,
                                                  float cn22, float rn2, float delta, float h2, bool reflect,
                                                  bool flat, float sgn, lanemask& geom_ok, float fs = 1.0f,
                                                  float fo = 1.0f, float fi = 1.0f, const CT& coat = CT()) {
  const float oz = r.hz + dzv;
  const float od = fmaf(r.px, r.dx, fmaf(r.py, r.dy, oz * r.dz));
  const float oo = fmaf(oz, oz, r.r2);
  const float Fh = fmaf(ch, oo, -oz);            // F / 2, F = c |o|^2 - 2 o_z
  const float G = fmaf(-c, od, r.dz);
  const float cF = cn22 * Fh;                    // = c n^2 F
  const float disc = fmaf(G, G, -cF);
  const float sq = lf_sqrt(disc);                // n |cos(incidence)|
  float t;
  if (flat) t = (Fh + Fh) * lf_rcp(fmaf(sgn, sq, G));   // wave-uniform branch
  else t = fmaf(-sgn, sq, G) * rn2;
  const float hx = fmaf(t, r.dx, r.px), hy = fmaf(t, r.dy, r.py), hz = fmaf(t, r.dz, oz);
  const float r2 = fmaf(hx, hx, hy * hy);
  // a ray that misses the sphere (disc < 0) has sq = t = r2 = NaN, and NaN <= h2 is false
  geom_ok = __ballot(r2 <= h2);
  lanemask ok = geom_ok;
  float Rn = 0.0f, D = 1.0f, ct = 0.0f;
  bool no_tir = true;
  if (W || !reflect) {
    const float k2 = disc + delta;                 // (n' cos(refraction))^2
    no_tir = k2 >= 0.0f;
    // (a totally reflected ray only survives a mirror event, and only W = true reads ct there)
    ct = lf_sqrt(reflect ? fmaxf(k2, 0.0f) : k2);
    if (W && coat.on()) {   // wave-uniform: a film on this interface
      if (coat.stacked()) stack_fraction(sq, ct, coat.stack(), Rn, D);   // wave-uniform: ... a stack of them
      else coated_fraction(sq, ct, coat.get(), Rn, D);
      // a refraction transmits Rd - Rn: clamped at 0, a rounding-negative factor must not reach the unsigned sums
      if (!reflect) Rn = fminf(Rn, D);
    } else if (W) {
      // unpolarised Fresnel straight from the optical cosines sq = n cos t, ct = n' cos t':
      //   rs = (sq - ct) / (sq + ct),   rp = (n'^2 sq - n^2 ct) / (n'^2 sq + n^2 ct),   R = (rs^2 + rp^2) / 2
      // as ONE fraction R = Rn / D, Rn = ((a B)^2 + (A b)^2) / 2, D = (b B)^2, with the numerators and
      // denominators scaled by row constants so that b = B = 1 at normal incidence (the running
      // denominator of a path stays near 1): fs = 1 / (n + n'), fo = n'^2 / q, fi = n^2 / q,
      // q = n'^2 n + n^2 n'.  No true cosine, no index ratio: nothing is divided by n on the way.
      const float a = (sq - ct) * fs, b = (sq + ct) * fs;
      const float pc = fi * ct;
      const float A = fmaf(fo, sq, -pc), B = fmaf(fo, sq, pc);
      const float u = a * B, v = A * b;
      Rn = 0.5f * fmaf(u, u, v * v);
      const float bB = b * B;
      D = bB * bB;
    }
  }
  if (reflect) {  // wave-uniform: K' = K - 2 (K . N) N, K . N = sgn sqrt(disc)
    if (W) {
      r.wn *= no_tir ? Rn : 1.0f;  // total reflection: R = 1
      r.wd *= no_tir ? D : 1.0f;
    }
    const float m = sq * (c2 * sgn);
    r.dx = fmaf(m, hx, r.dx);
    r.dy = fmaf(m, hy, r.dy);
    r.dz = fmaf(m, hz, fmaf(-2.0f * sgn, sq, r.dz));
  } else {        // K' = K + sgn (ct - sq) N
    ok &= __ballot(no_tir);
    if (W) {
      r.wn *= D - Rn;
      r.wd *= D;
    }
    const float gs = ct - sq;
    const float gcs = gs * sc;                     // sgn (ct - sq) c
    r.dx = fmaf(-gcs, hx, r.dx);
    r.dy = fmaf(-gcs, hy, r.dy);
    r.dz = fmaf(-gcs, hz, fmaf(sgn, gs, r.dz));
  }
  r.px = hx; r.py = hy; r.hz = hz; r.r2 = r2;
  return ok;
}

// the stop: flat pass-through, clipped by its housing and by the aperture mask
// FILT (only with W: the weighted march of a context under LF_MASK_BILINEAR, lf_set_mask_filter) reads the mask
// through lf_mask_bilinear below instead of the nearest texel; every other instantiation is the nearest lookup.
template <bool W, bool FILT = false>
__device__ __forceinline__ lanemask stop_event(Ray& r, float dzv, float h2, float inv_h,
                                               const float* __restrict__ mask, int mw, int mh) {
  const float t = -(r.hz + dzv) * lf_rcp(r.dz);
  const float hx = fmaf(t, r.dx, r.px), hy = fmaf(t, r.dy, r.py);
  const float r2 = fmaf(hx, hx, hy * hy);
  const float fu = fmaf(hx, inv_h, 1.0f) * (0.5f * (float)mw);
  const float fv = fmaf(hy, inv_h, 1.0f) * (0.5f * (float)mh);
  if (W && FILT) {
    float a;
    const bool open = lf_mask_bilinear(mask, mw, mh, fu, fv, a);
    r.wn *= a;
    r.px = hx; r.py = hy; r.hz = 0.0f; r.r2 = r2;
    return __ballot(r2 <= h2) & __ballot(open);
  }
  int ix = (int)fu, iy = (int)fv;  // NaN / out-of-range of a dead lane is clamped, never faults
  ix = min(max(ix, 0), mw - 1);
  iy = min(max(iy, 0), mh - 1);
  const float a = mask[iy * mw + ix];
  if (W) r.wn *= a;
  r.px = hx; r.py = hy; r.hz = 0.0f; r.r2 = r2;
  return __ballot(r2 <= h2) & __ballot(a > 0.0f);
}

// ---- the kernel variants of the weighted march ------------------------------------------------------
// What the weight of a ray may have to evaluate beyond bare glass and the nearest texel is chosen at compile
// time, so that a context without it launches the kernels it always launched: bit 0 = a film somewhere on the
// lens (lf_set_lens_coatings), bit 1 = the bilinear stop mask (lf_set_mask_filter).
enum : int { kVarBare = 0, kVarCoat = 1, kVarFilt = 2, kVarCoatFilt = 3,
             kVarLights = 4,    // | kVarLights: the context holds several lights (lf_set_lights): the lobe pre-test and the lit epilogue loop over them
             kVarStack = 8,     // | kVarStack (only with kVarCoat): some interface holds a stack of layers (lf_set_lens_coating_stacks)
             kVarOccl = 16,     // | kVarOccl (only with kVarLights): a lit ray adds only what the scene does not block (lf_set_ghost_occlusion);
                                //   differs from its kVarLights twin in lights_epilogue alone (lf_march_common.h)
             kVarNear = 32,     // | kVarNear (only with kVarLights): some light is a POINT light (lf_set_lights_ex): the pre-test, the gate
                                //   and the lit epilogue form the direction to such a light per lane, from the ray's exit point
                                // kVarNear | kVarOccl (launched only under lf_set_ghost_occlusion_reach(LF_OCCLUSION_REACH_LIGHT)): the shadow
                                //   ray of a point light ends at the light (lf_point_shadow_reach below, lights_epilogue in lf_march_common.h)
             kVarArea = 64 };   // | kVarArea (only with kVarLights | kVarNear): some light is an AREA light (lf_set_lights_geom, LF_LIGHT_AREA):
                                //   such a light's pre-test, gate and epilogue are the ray-parallelogram test below (lf_area_inside); the
                                //   kernel handles all three kinds, a context without an area light never launches it

// ---- a light at a finite distance (lf_set_lights_ex, LF_LIGHT_POINT; DESIGN.md section 4, "point lights") -------------
// The lobe factor of a ray that has left the front element at (px, py, z) (z absolute: front vertex z + hz) along d, for a
// light at L: s = L - P (three float subtractions), ss = |s|^2, and the sun's expression (lf_march_common.h lobe_q) on the
// non-unit s -- with the IEEE root and division, so that the host (lf_light_lobe_factor) and the kernels, which all
// call THIS definition, agree bit for bit.  cg = d.s: the ray looks towards the light iff cg > 0.
__host__ __device__ inline float lf_point_lobe_q(float dx, float dy, float dz, float px, float py, float z, float Lx, float Ly,
                                                 float Lz, float inv_1mc, float& cg) {
  const float sx = Lx - px, sy = Ly - py, sz = Lz - z;
  const float ss = fmaf(sx, sx, fmaf(sy, sy, sz * sz));
  cg = fmaf(dx, sx, fmaf(dy, sy, dz * sz));
  const float cx = fmaf(dy, sz, -(dz * sy)), cy = fmaf(dz, sx, -(dx * sz)), cz = fmaf(dx, sy, -(dy * sx));
  const float c2 = fmaf(cx, cx, fmaf(cy, cy, cz * cz));
  const float dd = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
  const float ds = dd * ss;
  const float den = fmaf(sqrtf(ds), cg, ds);      // (correctly rounded on both sides: -fhip-fp32-correctly-rounded-divide-sqrt)
  return (c2 / den) * inv_1mc;
}
// ... and the cheap test that SELECTS lanes for it (any superset of cg > 0 && q < 1 will do): cos(theta) > thr, thr the
// directional pre-test's threshold (1/16 of the lobe and 4e-7 below cos(alpha), 0 < thr: lf_march_lobe_thr_of), as
// cg > 0 && cg^2 > thr^2 |d|^2 |s|^2 -- no root, no division.  The float error of cg^2 / (|d|^2 |s|^2) is below 4e-7
// relative (five roundings), 2e-7 in the cosine; thr^2 is taken 1e-6 smaller (5e-7 in the cosine) on top of thr's own
// margin, and the exact test's own rounding (q good to 1e-6 relative) moves its edge by 1e-6 (1 - cos(alpha)) at most.
__host__ __device__ inline bool lf_point_pretest(float dx, float dy, float dz, float px, float py, float z, float Lx, float Ly,
                                                 float Lz, float thr) {
  const float sx = Lx - px, sy = Ly - py, sz = Lz - z;
  const float ss = fmaf(sx, sx, fmaf(sy, sy, sz * sz));
  const float cg = fmaf(dx, sx, fmaf(dy, sy, dz * sz));
  const float dd = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
  return cg > 0.0f && cg * cg > ((thr * thr) * 0.999999f) * (dd * ss);
}
// How far the shadow ray of a POINT light reaches (lf_set_ghost_occlusion_reach, LF_OCCLUSION_REACH_LIGHT): the ray parameter, in
// world units, of the point of the ray nearest the light -- s = L - P in double, dc = unit(d) exactly as the shadow ray's own
// direction is formed (lf_march_common.h ghost_shadow_ray: multiply by 1 / norm), t = wpm (s . dc) with the scene's dot
// product order, never below 0.  The camera's c2w is a rotation, so t is the parameter of the world ray as well.  Double
// division and root are IEEE on both sides and nothing here contracts: the host (lf_ghost_shadow_reach) and the kernels,
// which all call THIS definition, agree bit for bit.  A wall behind the lamp (t_hit > reach) does not hide it.
__host__ __device__ inline double lf_point_shadow_reach(float dx, float dy, float dz, float px, float py, float z, float Lx, float Ly,
                                                        float Lz, double wpm) {
  const double sx = (double)Lx - px, sy = (double)Ly - py, sz = (double)Lz - z;
  const double ax = (double)dx, ay = (double)dy, az = (double)dz;
  const double rn = 1. / sqrt((ax * ax + ay * ay) + az * az);
  const double cx = ax * rn, cy = ay * rn, cz = az * rn;
  const double t = wpm * ((sx * cx + sy * cy) + sz * cz);
  return t > 0.0 ? t : 0.0;
}
// ---- an area light (lf_set_lights_geom, LF_LIGHT_AREA; DESIGN.md section 4, "area lights") -----------------------------
// A one-sided parallelogram C + u e1 + v e2, u, v in [-1/2, 1/2], emitting towards dir.  Is the ray that has left the front
// element at P = (px, py, z) (z absolute) along d one that ends on its lit side?  The ray-parallelogram test with no
// division and no root (Moeller-Trumbore's, every quotient cleared by |det|), in THIS order, every multiply-add an fmaf:
//   s  = P - C                                   three float subtractions
//   p  = d x e2     p.x = fmaf(d.y, e2.z, -(d.z * e2.y)),  p.y = fmaf(d.z, e2.x, -(d.x * e2.z)),  p.z = fmaf(d.x, e2.y, -(d.y * e2.x))
//   det = e1 . p    fmaf(e1.x, p.x, fmaf(e1.y, p.y, e1.z * p.z))          (every dot product in this x, y, z nesting)
//   a  = s . p                                   (u = a / det)
//   qv = s x e1     the same pattern as p
//   b  = d . qv     (v = b / det),     tn = e2 . qv     (the ray parameter t = tn / det),     cd = d . dir
//   inside iff det != 0 and 2 |a| <= |det| and 2 |b| <= |det| and tn sign(det) > 0 and cd < 0
// (2 |a| is exact; cd < 0 is the reference's cosTheta < 0, its d running from the shaded point to the light.)  C: the centre,
// g: direction (unit as stored), e1, e2 -- nine floats.  The host (lf_light_geom_factor) and the kernels all call THIS
// definition: they agree bit for bit.  A lit ray's factor is 1: radiance is constant along a ray, there is no lobe.
__host__ __device__ inline bool lf_area_inside(float dx, float dy, float dz, float px, float py, float z, const float* __restrict__ C,
                                               const float* __restrict__ g) {
  const float e1x = g[3], e1y = g[4], e1z = g[5], e2x = g[6], e2y = g[7], e2z = g[8];
  const float sx = px - C[0], sy = py - C[1], sz = z - C[2];
  const float qx = fmaf(dy, e2z, -(dz * e2y)), qy = fmaf(dz, e2x, -(dx * e2z)), qz = fmaf(dx, e2y, -(dy * e2x));
  const float det = fmaf(e1x, qx, fmaf(e1y, qy, e1z * qz));
  const float a = fmaf(sx, qx, fmaf(sy, qy, sz * qz));
  const float vx = fmaf(sy, e1z, -(sz * e1y)), vy = fmaf(sz, e1x, -(sx * e1z)), vz = fmaf(sx, e1y, -(sy * e1x));
  const float b = fmaf(dx, vx, fmaf(dy, vy, dz * vz));
  const float tn = fmaf(e2x, vx, fmaf(e2y, vy, e2z * vz));
  const float cd = fmaf(dx, g[0], fmaf(dy, g[1], dz * g[2]));
  const float ad = fabsf(det);
  return det != 0.0f && 2.0f * fabsf(a) <= ad && 2.0f * fabsf(b) <= ad && (det > 0.0f ? tn > 0.0f : tn < 0.0f) && cd < 0.0f;
}
// ... and the cheap test that SELECTS lanes for it (any superset of lf_area_inside will do): does the ray's line, taken
// forwards, meet the rectangle's bounding sphere -- centre C, radius^2 rb2 (the half diagonal's square, rounded up: the host's
// area_bound2, lf_api.hip)?  With s = C - P, ss = |s|^2, cg = d.s, dd = |d|^2: ss <= rb2 (P inside the sphere), or cg > 0 and
// cg^2 >= dd (ss - rb2) -- no root, no division.  cg^2 and dd ss carry five roundings each (below 4e-7 relative); ss is
// taken 1e-5 smaller, which covers both and the subtraction's own rounding.
__host__ __device__ inline bool lf_area_pretest(float dx, float dy, float dz, float px, float py, float z, const float* __restrict__ C,
                                                float rb2) {
  const float sx = C[0] - px, sy = C[1] - py, sz = C[2] - z;
  const float ss = fmaf(sx, sx, fmaf(sy, sy, sz * sz));
  const float cg = fmaf(dx, sx, fmaf(dy, sy, dz * sz));
  const float dd = fmaf(dx, dx, fmaf(dy, dy, dz * dz));
  return ss <= rb2 || (cg > 0.0f && cg * cg >= dd * fmaf(ss, 0.99999f, -rb2));
}
// How far the shadow ray of an AREA light reaches (LF_OCCLUSION_REACH_LIGHT): to just before the rectangle's plane.  The
// expressions of lf_area_inside again, in double, on the float-stored geometry and the ray: t = tn / det, reach = wpm t |d|
// minus the reference's EPS_F = (double)0.00001f -- what its shadow rays to sampled lights take off, and lf_scene.hip's: an
// emissive mesh lying in the light's plane does not shadow its own light -- never below 0 (a ray parallel to the plane, or
// leaving it behind: 0).  Plain double products and sums in the order written, nothing contracts: the host
// (lf_ghost_shadow_reach_geom) and the kernels, which all call THIS definition, agree bit for bit.  *t_out: t itself.
__host__ __device__ inline double lf_area_shadow_reach(float dx, float dy, float dz, float px, float py, float z, const float* __restrict__ C,
                                                       const float* __restrict__ g, double wpm, double* t_out = nullptr) {
  const double ax = (double)dx, ay = (double)dy, az = (double)dz;
  const double e1x = (double)g[3], e1y = (double)g[4], e1z = (double)g[5], e2x = (double)g[6], e2y = (double)g[7], e2z = (double)g[8];
  const double sx = (double)px - (double)C[0], sy = (double)py - (double)C[1], sz = (double)z - (double)C[2];
  const double qx = ay * e2z - az * e2y, qy = az * e2x - ax * e2z, qz = ax * e2y - ay * e2x;
  const double det = (e1x * qx + e1y * qy) + e1z * qz;
  const double vx = sy * e1z - sz * e1y, vy = sz * e1x - sx * e1z, vz = sx * e1y - sy * e1x;
  const double tn = (e2x * vx + e2y * vy) + e2z * vz;
  const double t = tn / det;
  if (t_out) *t_out = t;
  const double r = (wpm * t) * sqrt((ax * ax + ay * ay) + az * az) - (double)0.00001f;
  return r > 0.0 ? r : 0.0;   // (NaN -- det = 0 -- gives 0 as well)
}
// The stop of a kernel instantiated for variant VAR.  Under the filter the geometry-only march (W = false) runs
// the UNCHANGED nearest lookup on the support texture S (2 mw x 2 mh floats behind the texels, k_mask_support:
// S > 0 exactly where one of the four texels of the bilinear footprint is open), the weighted march the
// bilinear lookup on the texels: both find the same rays alive, bit for bit.
template <bool W, int VAR>
__device__ __forceinline__ lanemask stop_event_var(Ray& r, float dzv, float h2, float inv_h,
                                                   const float* __restrict__ mask, int mw, int mh) {
  if ((VAR & kVarFilt) && !W) return stop_event<false>(r, dzv, h2, inv_h, mask + mw * mh, 2 * mw, 2 * mh);
  return stop_event<W, (VAR & kVarFilt) != 0>(r, dzv, h2, inv_h, mask, mw, mh);
}

// ---- one sensor sample's start ray ("sample") --------------------------------
// What k_march's sample loop computes inline, as a function: the lens camera of the scene term
// (lf_scene.hip) starts its primary path from the SAME sample -- the same Philox block, the same
// stratum and sub-cell of the pupil, the same float expressions -- so that the ray which images the
// scene is bit for bit the ray whose ghosts the march accumulates.
struct SampleSpec {
  int W;               // frame width (the pixel index of the counter is x + y W)
  int G;               // G x G pupil strata; samples s >= G * G are unstratified
  float inv_G;
  int xs;              // log2 of the pixel stride in x of a wave's tile (lf_set_tile_stride)
  int sub_bits;        // 2^sub_bits x 2^sub_bits sub-cells per stratum, drawn per (wave tile, s)
  float inv_sub;
  uint2 key;
  float pitch, half_w, half_h;
  float pupil_h, vz;   // the disc the samples aim at: radius, z - z_sensor
  float geom_norm;     // its solid-angle factor pi h^2 / vz^2
};
struct StartRay { float X, Y, dx, dy, dz, w0; };

// the concentric square -> disc map with the fixed polynomials of the contract
__device__ __forceinline__ void pupil_disc(float pa, float pb, float& qx, float& qy) {
  qx = 0.0f; qy = 0.0f;
  if (pa != 0.0f || pb != 0.0f) {
    const bool wide = fabsf(pa) > fabsf(pb);
    const float rr = wide ? pa : pb;
    const float th = 0.78539816339744831f * ((wide ? pb : pa) * lf_rcp(rr));
    const float t2 = th * th;
    const float sn = th * fmaf(t2, fmaf(t2, fmaf(t2, fmaf(t2, 2.7557319e-6f, -1.9841270e-4f),
                                                 8.3333333e-3f), -1.6666667e-1f), 1.0f);
    const float cs = fmaf(t2, fmaf(t2, fmaf(t2, fmaf(t2, 2.4801587e-5f, -1.3888889e-3f),
                                            4.1666667e-2f), -0.5f), 1.0f);
    qx = wide ? rr * cs : rr * sn;
    qy = wide ? rr * sn : rr * cs;
  }
}

// sensor point X, Y (mm) + pupil square coordinates in [-1, 1]^2 -> unit start direction and weight
__device__ __forceinline__ StartRay aim_at_pupil(float X, float Y, float pa, float pb, float pupil_h,
                                                 float vz, float geom_norm) {
  float qx, qy;
  pupil_disc(pa, pb, qx, qy);
  const float vx = fmaf(pupil_h, qx, -X), vy = fmaf(pupil_h, qy, -Y);
  const float len = lf_sqrt(fmaf(vx, vx, fmaf(vy, vy, vz * vz)));
  const float rl = lf_rcp(len);
  StartRay s;
  s.X = X; s.Y = Y; s.dx = vx * rl; s.dy = vy * rl; s.dz = vz * rl;
  const float c2 = s.dz * s.dz;
  s.w0 = geom_norm * (c2 * c2);
  return s;
}

// the wave tile of pixel (x, y) as k_march numbers it: tile row y / 8, and along x block x / (8 * 2^xs) with phase
// x mod 2^xs
__device__ __forceinline__ unsigned sample_tile_id(const SampleSpec& a, int x, int y) {
  const int tiles_x = ((a.W + (8 << a.xs) - 1) >> (3 + a.xs)) << a.xs;
  const int tx = ((x >> (3 + a.xs)) << a.xs) + (x & ((1 << a.xs) - 1));
  return (unsigned)((y >> 3) * tiles_x + tx);
}
// the sub-cell of its stratum that wave tile `tile_id` draws for sample s (< G * G)
__device__ __forceinline__ void sample_subcell(const SampleSpec& a, unsigned tile_id, int s, unsigned& sxi, unsigned& syi) {
  const uint4 r2 = philox4x32_10(make_uint4(tile_id, (unsigned)s, kDomainSubcell, 0u), a.key);
  sxi = a.sub_bits ? (r2.x >> (32 - a.sub_bits)) : 0u;
  syi = a.sub_bits ? (r2.y >> (32 - a.sub_bits)) : 0u;
}
// ... and the sample itself, given its stratum (cx, cy) = (s mod G, s / G) and that sub-cell (all four unused for the
// unstratified samples s >= G * G)
// (in two steps: the sensor point and the pupil-square coordinates, which lf_lens_camera_samples hands out as they are,
// then the start ray aimed from them)
struct SamplePoint { float X, Y, pa, pb; };
__device__ __forceinline__ SamplePoint sample_point_in(const SampleSpec& a, int x, int y, int s, int cx, int cy, unsigned sxi,
                                                       unsigned syi) {
  const unsigned p = (unsigned)y * (unsigned)a.W + (unsigned)x;
  const uint4 rnd = philox4x32_10(make_uint4(p, (unsigned)s, kDomainMarch, 0u), a.key);
  const float jx = u01(rnd.x), jy = u01(rnd.y);
  float ua = u01(rnd.z), ub = u01(rnd.w);
  if (s < a.G * a.G) {
    ua = ((float)cx + ((float)sxi + ua) * a.inv_sub) * a.inv_G;
    ub = ((float)cy + ((float)syi + ub) * a.inv_sub) * a.inv_G;
  }
  const float pa = fmaf(2.0f, ua, -1.0f), pb = fmaf(2.0f, ub, -1.0f);
  const float X = -(((float)x + jx) - a.half_w) * a.pitch;
  const float Y = -(((float)y + jy) - a.half_h) * a.pitch;
  return SamplePoint{X, Y, pa, pb};
}
__device__ __forceinline__ StartRay sample_start_in(const SampleSpec& a, int x, int y, int s, int cx, int cy, unsigned sxi,
                                                    unsigned syi) {
  const SamplePoint q = sample_point_in(a, x, y, s, cx, cy, sxi, syi);
  return aim_at_pupil(q.X, q.Y, q.pa, q.pb, a.pupil_h, a.vz, a.geom_norm);
}
__device__ __forceinline__ StartRay sample_start(const SampleSpec& a, int x, int y, int s) {
  unsigned sxi = 0u, syi = 0u;
  const int cy = s / a.G, cx = s - cy * a.G;
  if (s < a.G * a.G) sample_subcell(a, sample_tile_id(a, x, y), s, sxi, syi);
  return sample_start_in(a, x, y, s, cx, cy, sxi, syi);
}
// ... and its sensor point and pupil-square coordinates alone (k_lenscam_samples, lf_lens_camera.hip)
__device__ __forceinline__ SamplePoint sample_point(const SampleSpec& a, int x, int y, int s) {
  unsigned sxi = 0u, syi = 0u;
  const int cy = s / a.G, cx = s - cy * a.G;
  if (s < a.G * a.G) sample_subcell(a, sample_tile_id(a, x, y), s, sxi, syi);
  return sample_point_in(a, x, y, s, cx, cy, sxi, syi);
}

// the film constants of a row of the weight re-march: wavelength j of record `off` (bytes from the weight
// records' start; 0 = bare glass; the offset is wave-uniform, read with load_wrec's scalar load)
typedef int lf_i8 __attribute__((ext_vector_type(8)));
struct CoatRec {
  const void* base;
  int off, j;
  __device__ __forceinline__ bool on() const { return off != 0; }
  __device__ __forceinline__ bool stacked() const { return false; }
  __device__ __forceinline__ NoStack stack() const { return NoStack{}; }
  __device__ __forceinline__ LfCoatK get() const {
    typedef const char __attribute__((address_space(4))) * cptr;
    const lf_i8 v = *(const lf_i8 __attribute__((address_space(4)))*)((cptr)(base) + (off + 32 * j));
    return LfCoatK{__int_as_float(v[0]), __int_as_float(v[1]), __int_as_float(v[2]), __int_as_float(v[3]),
                   __int_as_float(v[4]), __int_as_float(v[5]), __int_as_float(v[6]), __int_as_float(v[7])};
  }
};
// ... of a kernel that can evaluate a stack too: bit 0 of the (wave-uniform) offset marks a stack record -- its N in the
// first dword, wavelength j of the group at + j (16 + 20 N) bytes (pack_program) -- every dword a scalar load
struct StackLoad {
  const char __attribute__((address_space(4))) * p;
  __device__ __forceinline__ int operator()(int i) const { return *(const int __attribute__((address_space(4)))*)(p + 4 * i); }
};
struct StackRec {
  const void* base;
  int off, j;
  __device__ __forceinline__ bool on() const { return off != 0; }
  __device__ __forceinline__ bool stacked() const { return (off & 1) != 0; }
  __device__ __forceinline__ LfCoatK get() const { return CoatRec{base, off, j}.get(); }
  __device__ __forceinline__ StackLoad stack() const {
    typedef const char __attribute__((address_space(4))) * cptr;
    const cptr q = (cptr)(base) + (off & ~1);
    const int N = *(const int __attribute__((address_space(4)))*)(q);
    return StackLoad{q + j * (16 + 20 * N)};
  }
};
// what a kernel instantiated with / without film support (bits kVarCoat, kVarStack of its variant) passes to surface_event
template <int VAR> using CoatSel = typename std::conditional<(VAR & kVarStack) != 0, StackRec,
                                   typename std::conditional<(VAR & kVarCoat) != 0, CoatRec, NoCoat>::type>::type;
// ... and of a row of the primary table (the wavelength may differ between lanes: a plain load)
struct CoatPrimary {
  const LfPrimaryRow* row;
  int lambda;
  __device__ __forceinline__ bool on() const { return row->coated != 0; }
  __device__ __forceinline__ bool stacked() const { return false; }
  __device__ __forceinline__ NoStack stack() const { return NoStack{}; }
  __device__ __forceinline__ LfCoatK get() const { return row->coat[lambda]; }
};
// ... of a kernel that can evaluate a stack too: coated = 1 a film, else 2 | the byte offset FROM THE ROW of the interface's
// stack records behind the table (lf_upload_primary_table), wavelength l at + l (16 + 20 N) bytes
struct StackPlain {
  const int* p;
  __device__ __forceinline__ int operator()(int i) const { return p[i]; }
};
struct StackPrimary {
  const LfPrimaryRow* row;
  int lambda;
  __device__ __forceinline__ bool on() const { return row->coated != 0; }
  __device__ __forceinline__ bool stacked() const { return (row->coated & 2) != 0; }
  __device__ __forceinline__ LfCoatK get() const { return row->coat[lambda]; }
  __device__ __forceinline__ StackPlain stack() const {
    const char* q = (const char*)row + (row->coated & ~3);
    const int N = *(const int*)q;
    return StackPlain{(const int*)(q + lambda * (16 + 20 * N))};
  }
};

// ---- the primary path N-1 .. 0 with its weight (LensCamera::generate_ray) ---------------------------
// One lane = one ray; the interface table (LfPrimaryDev, built by the host with the float arithmetic
// of pack_program) is wave-uniform and arrives through the scalar cache.  Returns whether this
// lane's ray left the front element; r then holds the exit state (hz relative to interface 0's vertex,
// K = the unit direction in air) and wn / wd the transmitted weight.
template <int VAR>
__device__ __forceinline__ bool primary_path(const LfPrimaryDev* __restrict__ P, int lambda, Ray& r,
                                             const float* __restrict__ mask, int mw, int mh, int lane) {
  { const float ns = P->n_start[lambda]; r.dx *= ns; r.dy *= ns; r.dz *= ns; }   // K = n d
  bool alive = true;
  const int n = P->n;
  for (int e = 0; e < n; e++) {   // wave-uniform
    const LfPrimaryRow& w = P->row[e];
    lanemask ok, geom_ok;
    if (w.kind & LF_EV_STOP) {
      ok = stop_event<true, (VAR & kVarFilt) != 0>(r, w.dzv, w.h2, P->inv_stop_h, mask, mw, mh);
    } else {
      if (VAR & kVarStack)
        ok = surface_event<true>(r, w.dzv, w.curv, w.ch, w.c2, w.sc, w.cn22[lambda], w.rn2[lambda],
                                 w.delta[lambda], w.h2, false, (w.kind & LF_EV_FLAT) != 0, -1.0f, geom_ok,
                                 w.fs[lambda], w.fo[lambda], w.fi[lambda], StackPrimary{&w, lambda});
      else if (VAR & kVarCoat)
        ok = surface_event<true>(r, w.dzv, w.curv, w.ch, w.c2, w.sc, w.cn22[lambda], w.rn2[lambda],
                                 w.delta[lambda], w.h2, false, (w.kind & LF_EV_FLAT) != 0, -1.0f, geom_ok,
                                 w.fs[lambda], w.fo[lambda], w.fi[lambda], CoatPrimary{&w, lambda});
      else
        ok = surface_event<true>(r, w.dzv, w.curv, w.ch, w.c2, w.sc, w.cn22[lambda], w.rn2[lambda],
                                 w.delta[lambda], w.h2, false, (w.kind & LF_EV_FLAT) != 0, -1.0f, geom_ok,
                                 w.fs[lambda], w.fo[lambda], w.fi[lambda]);
    }
    alive = alive && ((ok >> lane) & 1ull) != 0ull;
    if (__ballot(alive) == 0ull) break;   // every lane of the wave is blocked (a closed part of the pupil): nothing left to march
  }
  return alive;
}

}  // namespace lfm
