// pose_sanitizer.hip -- the host side of lf_pose.h under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program
// (its own main, no library, no Python, no device) that runs lfm::lf_pose_event over a file of rays -- the rays of
// tests/test_poses_cpu.py, written by
//     python -c "import sys; sys.path[:0] = ['tests', '.']; import test_poses_cpu as t; t.dump_rays('rays.bin')"
// -- on a sphere (the biconic route), a general biconic and an aspheric record, refraction and reflection, both directions.
// The sanitizers stay on the host: the file is compiled for the host alone, and the bare flag goes to the link step only.
//     hipcc --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Ilens-flare_amd/csrc -fsanitize=address,undefined \
//           -fno-sanitize-recover=all -c profiles/pose_sanitizer.hip -o pose_sanitizer.o
//     hipcc -fsanitize=address,undefined pose_sanitizer.o -o pose_sanitizer && ./pose_sanitizer rays.bin
// The file: int32 n, then n records of {float cx, cy, kx, ky, h, n_in, n_out, dzv; int32 reflect, forward, aspheric; float t[3],
// a[3]; float ray[6]}.  Prints the fates' tally; the sanitizers abort on a finding.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lf_pose.h"

struct Rec {
  float cx, cy, kx, ky, h, n_in, n_out, dzv;
  int32_t reflect, forward, aspheric;
  float t[3], a[3], ray[6];
};

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: pose_sanitizer rays.bin\n"); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int32_t n = 0;
  if (std::fread(&n, sizeof(n), 1, f) != 1 || n < 0) { std::fclose(f); return 2; }
  std::vector<Rec> recs((size_t)n);
  const size_t got = std::fread(recs.data(), sizeof(Rec), (size_t)n, f);
  std::fclose(f);
  if (got != (size_t)n) { std::fprintf(stderr, "short file\n"); return 2; }
  long tally[4] = {0, 0, 0, 0};
  double sum = 0.0;
  for (const Rec& r : recs) {
    lfm::LfAsphRec ka{};
    if (r.aspheric) { ka.kappa = -0.6f; ka.a[0] = 2e-6f; ka.a[1] = -1e-8f; }
    const lfm::LfBicRec kb{r.cx, r.kx, r.ky, {}};
    const lfm::LfPoseRec p = lfm::lf_pose_make(r.t[0], r.t[1], r.t[2], r.a[0], r.a[1], r.a[2]);
    float px = r.ray[0], py = r.ray[1], hz = r.ray[2], dx = r.ray[3], dy = r.ray[4], dz = r.ray[5], r2 = 0.0f;
    const float n_in2 = r.n_in * r.n_in, n_out2 = r.n_out * r.n_out;
    const lfm::AsphHit h = lfm::lf_pose_event(px, py, hz, r2, dx, dy, dz, r.dzv, r.cy, r.aspheric != 0, ka, kb, p, n_out2 - n_in2,
                                              r.h * r.h, r.reflect != 0, r.forward ? 1.0f : -1.0f);
    tally[h.fate & 3]++;
    if (h.fate == lfm::kAsphAlive) sum += (double)px + (double)py + (double)hz + (double)dx + (double)dy + (double)dz + (double)r2;
  }
  std::printf("%d rays: alive %ld, missed %ld, outside the aperture %ld, totally reflected %ld (checksum %.6f)\n", n, tally[0],
              tally[1], tally[2], tally[3], sum);
  return 0;
}
