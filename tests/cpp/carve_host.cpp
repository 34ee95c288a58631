// The host arithmetic of revo_map_carve_eval / revo_map_carve (revo_amd/csrc/revo_carve_host.h) over views, parameters and records
// a test wrote: a plain C++ program, no GPU.
// Input file: the context camera (6 floats: fx fy cx cy zmin zmax) and size (2 x i32); the number of views (u32), then per view
// has_kf, has_depth, width, height (4 x i32), 6 floats of intrinsics and 16 of T_w_c (column-major); the number of parameter sets
// (u32), then per set has_params (i32) and radius, min_views, min_count, max_count (i32, 3 x u32), margin, margin_rel (2 floats);
// the voxel edge (float); the number of records (u64) and the records (64 bytes each) in any order.
// Output file: per view one byte (1 accepted) and, when accepted, w, h (2 x i32) and Rc[9], tc[3], fx, fy, cx, cy, zmin, zmax
// (18 floats); per parameter set one byte and, when accepted, the six effective parameters as stored; the number of records
// (u64) and the records in ascending key order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../revo_amd/csrc/revo_carve_host.h"

template <class T>
static bool rd(FILE* f, T* p, size_t n = 1) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE* f, const T* p, size_t n = 1) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  static const float image[1] = {1.0f};  // a view's depth pointer is only tested against NULL
  float cam[6];
  int32_t size[2];
  uint32_t nv = 0, np = 0;
  bool ok = rd(f, cam, 6) && rd(f, size, 2) && rd(f, &nv) && nv <= 1024;
  const CarveCam ctx{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5]};
  for (uint32_t i = 0; ok && i < nv; ++i) {
    int32_t h[4];
    revo_map_carve_view v{};
    ok = rd(f, h, 4) && rd(f, &v.fx, 6) && rd(f, v.T_w_c, 16);
    if (!ok) break;
    v.kf = h[0] ? (const revo_pyr*)image : nullptr;  // never dereferenced
    v.depth = h[1] ? image : nullptr;
    v.width = h[2]; v.height = h[3];
    CarveView out{};
    const unsigned char good = carve_view_check(&v, ctx, size[0], size[1], &out) == nullptr;
    ok = wr(o, &good);
    if (good) ok = ok && wr(o, &out.w) && wr(o, &out.h) && wr(o, out.Rc, 9) && wr(o, out.tc, 3) && wr(o, &out.fx, 6);
  }
  ok = ok && rd(f, &np) && np <= 1024;
  std::vector<int32_t> has(np);
  std::vector<revo_map_carve_params> prm(np);
  for (uint32_t i = 0; ok && i < np; ++i) ok = rd(f, &has[i]) && rd(f, &prm[i]);
  float voxel = 0.0f;
  ok = ok && rd(f, &voxel);
  for (uint32_t i = 0; ok && i < np; ++i) {
    revo_map_carve_params out{};
    const unsigned char good = carve_params_check(has[i] ? &prm[i] : nullptr, voxel, &out) == nullptr;
    ok = wr(o, &good);
    if (good) ok = ok && wr(o, &out);
  }
  uint64_t n = 0;
  ok = ok && rd(f, &n) && n <= (1u << 24);
  std::vector<revo_map_voxel_raw> rec(ok ? (size_t)n : 0);
  ok = ok && rd(f, rec.data(), rec.size());
  fclose(f);
  const uint64_t m = carve_canonicalise(rec.data(), rec.size());
  ok = ok && wr(o, &m) && wr(o, rec.data(), (size_t)m);
  return fclose(o) == 0 && ok ? 0 : 2;
}
