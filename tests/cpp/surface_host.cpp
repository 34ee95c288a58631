// surface_host.cpp -- revo_tsdf_host.h's rules for the colour volume and the vertex attributes on the host: the program
// reads cases from a binary file and prints what the header makes of them, one line each, floats as their bits;
// tests/test_map_surface_cpu.py compares the lines with the specification's numbers.  The argument check is run on fixed cases.
// Build: c++ -std=c++17 -ffp-contract=off surface_host.cpp (with host sanitizers where the toolchain has them).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../revo_amd/csrc/revo_tsdf_host.h"

static unsigned bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}

template <typename T>
static bool get(FILE* f, T* out, size_t n = 1) { return fread(out, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned n = 0;
  // the colour update, tied to the TSDF update: sum, weight, q, confirmed | sum_b, sum_g, sum_r, weight | b, g, r
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    int32_t sq[2];
    uint32_t w, confirmed, col[4], px[3];
    if (!get(f, &sq[0]) || !get(f, &w) || !get(f, &sq[1]) || !get(f, &confirmed) || !get(f, col, 4) || !get(f, px, 3)) return 3;
    const uint8_t bgr[3] = {(uint8_t)px[0], (uint8_t)px[1], (uint8_t)px[2]};
    const unsigned dropped = tsdf_update(sq[0], w, sq[1]);
    const unsigned took = tsdf_color_update(col[0], col[1], col[2], col[3], confirmed != 0, dropped, bgr);
    printf("update %u %d %u %u %u %u %u %u\n", dropped, sq[0], w, took, col[0], col[1], col[2], col[3]);
  }
  // the field and a channel's mean: sum, weight
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    int32_t s;
    uint32_t w;
    if (!get(f, &s) || !get(f, &w)) return 3;
    printf("field %u %u\n", bits(tsdf_field(s, w)), bits(tsdf_channel((uint32_t)s, w)));
  }
  // one axis of the gradient: vm, fm, fc, vp, fp
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    uint32_t vm, vp;
    float fm, fc, fp;
    if (!get(f, &vm) || !get(f, &fm) || !get(f, &fc) || !get(f, &vp) || !get(f, &fp)) return 3;
    printf("grad %u\n", bits(tsdf_grad_axis(vm != 0, fm, fc, vp != 0, fp)));
  }
  // the interpolated, normalised gradient: g0, g1, a
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    float g[7], nx, ny, nz;
    if (!get(f, g, 7)) return 3;
    tsdf_normal(tsdf_lerp(g[0], g[3], g[6]), tsdf_lerp(g[1], g[4], g[6]), tsdf_lerp(g[2], g[5], g[6]), &nx, &ny, &nz);
    printf("normal %u %u %u\n", bits(nx), bits(ny), bits(nz));
  }
  // a colour byte: s0, w0, s1, w1, a
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    uint32_t c[4];
    float a;
    if (!get(f, c, 4) || !get(f, &a)) return 3;
    printf("byte %u %u\n", (unsigned)tsdf_color_byte(c[0], c[1], c[2], c[3], a), tsdf_color_k(c[1], c[3]));
  }
  fclose(f);
  // the colour image that goes with a view
  revo_map_carve_view v;
  memset(&v, 0, sizeof v);
  const float depth = 1.0f;
  const uint8_t img[3] = {1, 2, 3};
  v.depth = &depth;
  printf("bgr %d %d\n", tsdf_bgr_check(&v, img) == nullptr, tsdf_bgr_check(&v, nullptr) == nullptr);
  v.depth = nullptr;
  v.kf = (decltype(v.kf))&v;  // any pointer that is not NULL: the check does not follow it
  printf("bgr %d %d\n", tsdf_bgr_check(&v, img) == nullptr, tsdf_bgr_check(&v, nullptr) == nullptr);
  return 0;
}
