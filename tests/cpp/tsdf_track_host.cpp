// tsdf_track_host.cpp -- revo_tsdf_track_host.h's rules for tracking a depth frame against the surface on the host: the
// program reads cases from a binary file and prints what the header makes of them, one line each, floats as their bits;
// tests/test_map_tsdf_track_cpu.py compares the lines with the specification's numbers.
// Build: c++ -std=c++17 -ffp-contract=off tsdf_track_host.cpp (with host sanitizers where the toolchain has them).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../revo_amd/csrc/revo_tsdf_track_host.h"

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
  // the parameter rules: has, trunc, max_dist, stride, min_weight, centre, reserved
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    uint32_t has;
    float trunc;
    revo_map_tsdf_track_params p, out;
    if (!get(f, &has) || !get(f, &trunc) || !get(f, &p.max_dist) || !get(f, &p.stride) || !get(f, &p.min_weight) || !get(f, p.centre, 3) ||
        !get(f, p.reserved, 2))
      return 3;
    const char* why = tsdf_track_params_check(has ? &p : nullptr, trunc, &out);
    if (why) printf("params refused\n");
    else printf("params %u %u %u %u %u %u\n", bits(out.max_dist), out.stride, out.min_weight, bits(out.centre[0]), bits(out.centre[1]), bits(out.centre[2]));
  }
  // the pixels a stride visits: n, stride
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    int32_t len, stride;
    if (!get(f, &len) || !get(f, &stride)) return 3;
    printf("lattice %d\n", tsdf_track_lattice(len, stride));
  }
  // one axis of a point's place at the voxel edge 1/8, at the box's rims: g, lo, n
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    float g, r = 0.0f;
    int32_t lo, cells, b = 0;
    if (!get(f, &g) || !get(f, &lo) || !get(f, &cells)) return 3;
    const bool ok = tsdf_ray_axis_at(g, 0.125f, lo, cells, &b, &r);
    if (ok) printf("axis 1 %d %u\n", b, bits(r));
    else printf("axis 0\n");
  }
  // the cases: every visited pixel under every pose -> its class and, accepted, its 28 terms
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    TsdfTrackK a{};
    float trunc, cam[6];
    uint32_t stride, npose;
    int32_t w, h;
    if (!get(f, a.vol.box.lo, 3) || !get(f, a.vol.box.n, 3)) return 3;
    std::vector<revo_map_tsdf_cell> cells((size_t)a.vol.box.n[0] * a.vol.box.n[1] * a.vol.box.n[2]);
    if (!get(f, cells.data(), cells.size())) return 3;
    if (!get(f, &a.vol.voxel) || !get(f, &trunc) || !get(f, cam, 6)) return 3;
    if (!get(f, &a.max_dist) || !get(f, &stride) || !get(f, &a.vol.min_weight) || !get(f, a.centre, 3)) return 3;
    if (!get(f, &w) || !get(f, &h)) return 3;
    std::vector<float> depth((size_t)w * h);
    if (!get(f, depth.data(), depth.size()) || !get(f, &npose)) return 3;
    a.vol.tsdf = cells.data();
    a.cam = TsdfTrackCam{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5]};
    a.kq = tsdf_track_kq(trunc);
    for (unsigned k = 0; k < npose; ++k) {
      float P[12];  // R column-major, t
      if (!get(f, P, 12)) return 3;
      for (int y = 0; y < h; y += (int)stride)
        for (int x = 0; x < w; x += (int)stride) {
          float pw[3], e = 0.0f, g[3] = {0.0f, 0.0f, 0.0f};
          const int cls = tsdf_track_pixel(a, P, P + 9, x, y, depth[(size_t)y * w + x], pw, &e, g);
          printf("pixel %d", cls);
          if (cls == TSDF_TRACK_ACCEPTED) tsdf_track_terms(tsdf_track_row(a, pw, g), e, [](int, float term) { printf(" %u", bits(term)); });
          printf("\n");
        }
    }
  }
  fclose(f);
  return 0;
}
