// The down-date of a TSDF cell and its FIT test (revo_amd/csrc/revo_tsdf_host.h) over a table of cells a test wrote: a
// plain C++ program, no GPU.
// Input file: the number of truncs (u32), then per trunc the voxel edge and trunc (2 floats); the number of cells (u32), then per
// cell sum (i32), weight (u32), sum_b, sum_g, sum_r, color weight (4 x u32), the number of updates (u32, at most 64), and per
// update confirmed (u32), q (i32) and the pixel's bytes B, G, R (3 x u8) with one byte of padding.
// Output (text, one record per line): "trunc good bits"; per cell "cell k kc q b g r fits color_fits" and, for a cell that fits
// with its colour, "down sum weight sum_b sum_g sum_r color_weight" -- the cell behind the down-date.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../revo_amd/csrc/revo_tsdf_host.h"

template <class T>
static bool rd(FILE* f, T* p, size_t n = 1) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n = 0;
  bool ok = rd(f, &n) && n <= 4096;
  for (uint32_t i = 0; ok && i < n; ++i) {
    float vt[2], out = 0.0f;
    ok = rd(f, vt, 2);
    if (!ok) break;
    const char* why = tsdf_unfuse_trunc(vt[1], vt[0], &out);
    uint32_t bits = 0;
    memcpy(&bits, &out, 4);
    printf("trunc %d %u\n", why ? 0 : 1, why ? 0u : bits);
  }
  ok = ok && rd(f, &n) && n <= 65536;
  for (uint32_t i = 0; ok && i < n; ++i) {
    int32_t sum = 0;
    uint32_t w[5], updates = 0;
    ok = rd(f, &sum) && rd(f, w, 5) && rd(f, &updates) && updates <= 64;
    if (!ok) break;
    TsdfDown d{0u, 0u, 0, 0u, 0u, 0u};
    for (uint32_t u = 0; ok && u < updates; ++u) {
      uint32_t confirmed = 0;
      int32_t q = 0;
      uint8_t px[4];
      ok = rd(f, &confirmed) && rd(f, &q) && rd(f, px, 4);
      if (ok) tsdf_down_add(d, confirmed != 0, q, confirmed ? px : nullptr);
    }
    if (!ok) break;
    const bool fits = d.k > 0 && tsdf_down_fits(sum, w[0], d);
    const bool cfits = d.k > 0 && tsdf_down_color_fits(w[0], w[1], w[2], w[3], w[4], d);
    printf("cell %u %u %d %u %u %u %d %d\n", d.k, d.kc, d.q, d.b, d.g, d.r, fits ? 1 : 0, cfits ? 1 : 0);
    if (fits && cfits) {
      tsdf_down_apply(sum, w[0], d);
      tsdf_down_color_apply(w[1], w[2], w[3], w[4], d);
      printf("down %d %u %u %u %u %u\n", sum, w[0], w[1], w[2], w[3], w[4]);
    }
  }
  fclose(f);
  return ok ? 0 : 1;
}
