// lf_path_table.h -- the self-contained row of a path marched for ONE wavelength: every constant of its event in the row
// itself, nothing shared with the march program.  Two tables are made of it: the per-ray query's (lf_march_path_rays,
// lf_march_asph.hip: build_path_table) and the sensor ghosts' (lf_march_sensor.hip: one row list per (sensor path,
// wavelength), resident on the device).  Host: lf_path_row_fill writes a row with the constants of pack_program.
// Nothing here is part of the ABI.
#pragma once

#include <cmath>
#include <cstddef>

#include "lf_internal.h"
#include "lf_march_events.h"
#include "lf_asphere.h"

namespace lfm {

// ... and, only in the kind word of a row of the sensor ghosts' table: the row is the sensor's mirror (lf_sensor_event.h);
// `fs` holds the sensor's reflectance at the row's wavelength.  No other table ever carries the bit.
enum { LF_EV_SENSOR = 32 };

struct alignas(32) LfPathRow {
  float dzv, curv, ch, c2, sc, h2, sgn;
  int kind;        // LF_EV_REFLECT | LF_EV_STOP | LF_EV_FLAT | LF_EV_ASPH | LF_EV_BICONIC (then `asph` holds {1/Rx, kx, ky})
  float cn22, rn2, delta, fs, fo, fi;
  int coated;      // 0 bare; 1: a film, `coat` holds its constants; else 2 | the byte offset, from this row, of its stack record
  int pad;
  LfCoatK coat;
  LfAsphRec asph;
};
static_assert(sizeof(LfPathRow) == 128, "four 32-byte loads");
constexpr int kPathRowsMax = 3 * LF_MAX_SURFACES;
struct LfPathDev {
  int n;
  float inv_stop_h, front_zv, n_start;
  int pad[4];
  LfPathRow row[kPathRowsMax];
};
constexpr size_t kPathStackRowBytes = 4 * (4 + 5 * LF_MAX_COAT_LAYERS);   // a row's stack record at its largest
constexpr size_t kPathStackBytes = (size_t)kPathRowsMax * kPathStackRowBytes;
struct PathCoat {
  const LfPathRow* row;
  __device__ __forceinline__ bool on() const { return row->coated != 0; }
  __device__ __forceinline__ bool stacked() const { return (row->coated & 2) != 0; }
  __device__ __forceinline__ LfCoatK get() const { return row->coat; }
  __device__ __forceinline__ StackPlain stack() const { return StackPlain{(const int*)((const char*)row + (row->coated & ~3))}; }
};

// host: the row of interface k at wavelength l for a ray that comes from interface `from` (>= n_surf: the sensor),
// travelling +z (fwd) or -z -- the order of lf_build_march_tables, the constants of pack_program.  The row lies at
// base + row_off; a stacked interface's record is appended at base + *next_stack (which moves on), never beyond cap.
inline lf_status lf_path_row_fill(const lf_ctx* ctx, int l, int k, int from, bool reflect, bool fwd, unsigned char* base,
                                  size_t row_off, size_t* next_stack, size_t cap) {
  const LfLensDev& L = ctx->lens;
  const LfCoatings& C = ctx->coat;
  const LfAspheres& A = ctx->asph;
  const LfSurfaceDev& s = L.surf[k];
  LfPathRow& w = *reinterpret_cast<LfPathRow*>(base + row_off);
  w.dzv = (from >= L.n_surf ? L.z_sensor : L.surf[from].zv) - s.zv;
  w.sgn = fwd ? 1.0f : -1.0f;
  w.curv = s.curv; w.ch = 0.5f * s.curv; w.c2 = 2.0f * s.curv; w.sc = w.sgn * s.curv; w.h2 = s.h2;
  w.kind = (reflect ? LF_EV_REFLECT : 0) | (s.is_stop != 0.0f ? LF_EV_STOP : 0) | (s.curv == 0.0f ? LF_EV_FLAT : 0);
  const float n_in = fwd ? s.n_before[l] : s.n_after[l], n_out = fwd ? s.n_after[l] : s.n_before[l];
  const float n_in2 = n_in * n_in, n_out2 = n_out * n_out;
  w.cn22 = w.c2 * n_in2;
  w.rn2 = s.curv == 0.0f ? 0.0f : s.radius / n_in2;
  w.delta = n_out2 - n_in2;
  const float q = std::fmaf(n_out2, n_in, n_in2 * n_out);
  w.fs = 1.0f / (n_in + n_out);
  w.fo = n_out2 / q;
  w.fi = n_in2 / q;
  if (s.is_stop != 0.0f) return LF_OK;
  w.coated = C.n > 0 && C.thickness_nm[k] > 0.0f ? 1 : 0;
  if (w.coated) lf_coat_constants(n_in, C.index[(size_t)l * L.n_surf + k], n_out, C.thickness_nm[k], C.lambda_nm[l], &w.coat);
  if (C.n_stacked > 0 && C.n_layers[k] >= 2) {
    const size_t sub = sizeof(float) * kStackDwords(C.n_layers[k]);
    if (*next_stack + sub > cap) return LF_ERR_STATE;
    w.coated = 2 | (int)(*next_stack - row_off);
    lf_stack_constants_of(C, L.n_surf, L.n_lambda, k, l, fwd, n_in, n_out, reinterpret_cast<float*>(base + *next_stack));
    *next_stack += sub;
  }
  const LfBiconics& B = ctx->bic;
  const int rec_kind = lf_surface_record_kind(ctx, k);
  if (rec_kind == LF_EV_BICONIC) {
    w.kind |= LF_EV_BICONIC;
    w.asph.kappa = B.rx[k] == 0.0f ? 0.0f : 1.0f / B.rx[k];
    w.asph.a[0] = B.kx[k];
    w.asph.a[1] = B.ky[k];
  } else if (rec_kind == LF_EV_ASPH) {
    w.kind |= LF_EV_ASPH;
    w.asph.kappa = A.kappa[k];
    for (int m = 0; m < LF_MAX_ASPH_COEF; m++) w.asph.a[m] = A.coef[(size_t)m * L.n_surf + k];
  }
  return LF_OK;
}

}  // namespace lfm
