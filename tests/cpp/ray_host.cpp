// The host arithmetic of revo_map_raycast / revo_map_cast_rays (revo_amd/csrc/revo_ray_host.h) over views and parameters a test
// wrote: a plain C++ program, no GPU.
// Input file: the context camera (6 floats: fx fy cx cy zmin zmax); the number of views (u32), then per view a revo_map_view
// (104 bytes); the number of groups (u32), then per group first, count (2 x u32): a run of the views whose common min_count is
// asked for; the number of parameter sets (u32), then per set has_params (i32) and a revo_map_ray_params (16 bytes).
// Output file: per view one byte (1 accepted) and, when accepted, w, h (2 x i32) and o[3], R[9], Rc[9], tc[3], fx, fy, cx, cy,
// zmin, zmax (30 floats); per group a u32 (the common min_count, 0: mixed); per parameter set one byte and, when accepted,
// max_steps (u32).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../revo_amd/csrc/revo_ray_host.h"

template <class T>
static bool rd(FILE* f, T* p, size_t n = 1) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE* f, const T* p, size_t n = 1) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  static_assert(sizeof(revo_map_view) == 104, "a view is 104 bytes");
  float cam[6];
  uint32_t nv = 0, ng = 0, np = 0;
  bool ok = rd(f, cam, 6) && rd(f, &nv) && nv <= 1024;
  const CarveCam ctx{cam[0], cam[1], cam[2], cam[3], cam[4], cam[5]};
  std::vector<revo_map_view> views(ok ? nv : 0);
  ok = ok && rd(f, views.data(), views.size());
  for (uint32_t i = 0; ok && i < nv; ++i) {
    RayView out{};
    const unsigned char good = ray_view_check(&views[i], ctx, &out) == nullptr;
    ok = wr(o, &good);
    if (good) ok = ok && wr(o, &out.w) && wr(o, &out.h) && wr(o, out.o, 3) && wr(o, out.R, 9) && wr(o, out.Rc, 9) && wr(o, out.tc, 3) && wr(o, &out.fx, 6);
  }
  ok = ok && rd(f, &ng) && ng <= 1024;
  for (uint32_t i = 0; ok && i < ng; ++i) {
    uint32_t g[2];
    ok = rd(f, g, 2) && g[1] >= 1 && g[0] <= nv && g[1] <= nv - g[0];
    if (!ok) break;
    const uint32_t mc = ray_views_min_count(views.data() + g[0], (int)g[1]);
    ok = wr(o, &mc);
  }
  ok = ok && rd(f, &np) && np <= 1024;
  for (uint32_t i = 0; ok && i < np; ++i) {
    int32_t has = 0;
    revo_map_ray_params prm{};
    ok = rd(f, &has) && rd(f, &prm);
    if (!ok) break;
    uint32_t max_steps = 0;
    const unsigned char good = ray_params_check(has ? &prm : nullptr, &max_steps) == nullptr;
    ok = wr(o, &good);
    if (good) ok = ok && wr(o, &max_steps);
  }
  fclose(f);
  return fclose(o) == 0 && ok ? 0 : 2;
}
