// The host arithmetic of revo_map_view_gain (revo_amd/csrc/revo_gain_host.h) over parameters and poses a test wrote, and the
// cull against brute force: a plain C++ program, no GPU.
// Input file: the voxel edge, zmin, zmax (3 floats); the number of parameter sets (u32), then per set has_params (i32) and the
// 32-byte record; the number of poses (u32), then per pose 16 floats (column-major); the number of cull trials (u32) and a seed
// (u32).
// Output file: per parameter set one byte (1 accepted) and, when accepted, the effective record; per pose one byte (1: it
// keeps the pose rules) and the descriptor's o, R, Rc, tc (24 floats; zeros for a refused pose); then four u64: the cull trials
// run, the cells looked at, the cells whose class is not OUTSIDE, and the VIOLATIONS -- such cells outside the cull's range,
// which must be 0 -- and a fifth: the cells the ranges leave to visit.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../revo_amd/csrc/revo_gain_host.h"
#include "../../revo_amd/csrc/revo_seen_host.h"

template <class T>
static bool rd(FILE* f, T* p, size_t n = 1) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE* f, const T* p, size_t n = 1) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

// Whether the class of the point p in the view is not OUTSIDE: the head of the per-view rule (include/revo_hip.h),
// float32 operation by operation (the program is built with -ffp-contract=off).
static bool inside(const RayView& c, int r, float px, float py, float pz) {
  const float x = ((c.Rc[0] * px + c.Rc[1] * py) + c.Rc[2] * pz) + c.tc[0];
  const float y = ((c.Rc[3] * px + c.Rc[4] * py) + c.Rc[5] * pz) + c.tc[1];
  const float z = ((c.Rc[6] * px + c.Rc[7] * py) + c.Rc[8] * pz) + c.tc[2];
  if (!std::isfinite(x) || !std::isfinite(y) || !(std::isfinite(z) && z > c.zmin && z < c.zmax)) return false;
  const float u = (c.fx * x) / z + c.cx;
  const float v = (c.fy * y) / z + c.cy;
  if (!(std::fabs(u) < 1048576.0f) || !(std::fabs(v) < 1048576.0f)) return false;
  const int iu = (int)std::floor(u + 0.5f), iv = (int)std::floor(v + 0.5f);
  return !(iu - r < 0 || iu + r > c.w - 1 || iv - r < 0 || iv + r > c.h - 1);
}

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  double uni(double a, double b) { return a + (b - a) * (next() / 2147483648.0); }
  int range(int a, int b) { return a + (int)(next() % (uint32_t)(b - a + 1)); }
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  float head[3] = {0, 0, 0};
  uint32_t n = 0;
  bool ok = rd(f, head, 3) && rd(f, &n) && n <= 4096;
  for (uint32_t i = 0; ok && i < n; ++i) {
    int32_t has = 0;
    revo_map_gain_params p{}, out{};
    ok = rd(f, &has) && rd(f, &p);
    if (!ok) break;
    const unsigned char good = gain_params_check(has ? &p : nullptr, head[0], head[1], head[2], &out) == nullptr;
    ok = wr(o, &good);
    if (good) ok = ok && wr(o, &out);
  }
  RayView cam{};
  cam.fx = 8.5f; cam.fy = 8.5f; cam.cx = 7.5f; cam.cy = 5.5f; cam.zmin = head[1]; cam.zmax = head[2]; cam.w = 16; cam.h = 12;
  ok = ok && rd(f, &n) && n <= 4096;
  for (uint32_t i = 0; ok && i < n; ++i) {
    float T[16];
    ok = rd(f, T, 16);
    if (!ok) break;
    RayView v{};
    const unsigned char good = gain_pose_view(cam, T, &v);
    float d[24] = {0};
    if (good) {
      for (int k = 0; k < 3; ++k) { d[k] = v.o[k]; d[21 + k] = v.tc[k]; }
      for (int k = 0; k < 9; ++k) { d[3 + k] = v.R[k]; d[12 + k] = v.Rc[k]; }
    }
    ok = wr(o, &good) && wr(o, d, 24) && (good ? v.w == 16 && v.h == 12 : v.w == 0 && v.h == 0);
  }
  uint32_t trials = 0, seed = 0;
  ok = ok && rd(f, &trials) && rd(f, &seed) && trials <= (1u << 20);
  uint64_t sums[5] = {0, 0, 0, 0, 0};
  Rng g{seed};
  const float voxels[4] = {0.02f, 0.125f, 0.5f, 1.0f / 3.0f};
  for (uint32_t t = 0; ok && t < trials; ++t) {
    const float voxel = voxels[g.range(0, 3)];
    revo_map_df_box box;
    const int far = g.range(0, 9) == 0 ? 1 : 0;  // some boxes at the rim of the index range, where float32 is coarse
    for (int k = 0; k < 3; ++k) {
      box.n[k] = g.range(1, 12);
      box.lo[k] = far ? (g.range(0, 1) ? (1 << 20) - box.n[k] : -(1 << 20)) : g.range(-40, 40);
    }
    RayView c{};
    c.w = g.range(1, 40); c.h = g.range(1, 30);
    c.fx = (float)g.uni(3.0, 60.0); c.fy = (float)g.uni(3.0, 60.0);
    c.cx = (float)g.uni(-4.0, c.w + 4.0); c.cy = (float)g.uni(-4.0, c.h + 4.0);
    c.zmin = g.range(0, 1) ? 0.0f : (float)g.uni(0.0, 0.5);
    c.zmax = c.zmin + (float)g.uni(0.05, 8.0) * (voxel > 0.1f ? 4.0f : 1.0f);
    const int radius = g.range(0, 3);
    // a rotation from an axis and an angle, and a position in or around the box
    double ax[3] = {g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)};
    const double len = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
    if (len < 1e-3) continue;
    for (double& a : ax) a /= len;
    const double th = g.uni(-3.2, 3.2), cs = std::cos(th), sn = std::sin(th);
    float T[16] = {0};
    for (int r = 0; r < 3; ++r)
      for (int q = 0; q < 3; ++q) {
        const double cross = r == q ? 0.0 : ((q - r + 3) % 3 == 1 ? -ax[3 - r - q] : ax[3 - r - q]);
        T[4 * q + r] = (float)(cs * (r == q) + (1 - cs) * ax[r] * ax[q] + sn * cross);
      }
    for (int k = 0; k < 3; ++k) T[12 + k] = (float)(((double)box.lo[k] + g.uni(-1.5, 2.5) * box.n[k]) * voxel);
    T[15] = 1.0f;
    if (g.range(0, 3)) {  // three times in four the camera is turned towards a point in the box
      double z[3], up[3] = {g.uni(-1, 1), g.uni(-1, 1), g.uni(-1, 1)}, x[3], zl = 0.0, xl = 0.0;
      for (int k = 0; k < 3; ++k) { z[k] = ((double)box.lo[k] + g.uni(0.0, 1.0) * box.n[k]) * voxel - (double)T[12 + k]; zl += z[k] * z[k]; }
      if (zl < 1e-12) continue;
      for (double& a : z) a /= std::sqrt(zl);
      x[0] = up[1] * z[2] - up[2] * z[1]; x[1] = up[2] * z[0] - up[0] * z[2]; x[2] = up[0] * z[1] - up[1] * z[0];
      for (double a : x) xl += a * a;
      if (xl < 1e-6) continue;
      for (double& a : x) a /= std::sqrt(xl);
      const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
      for (int k = 0; k < 3; ++k) { T[k] = (float)x[k]; T[4 + k] = (float)y[k]; T[8 + k] = (float)z[k]; }
    }
    RayView v{};
    if (!gain_pose_view(c, T, &v)) continue;
    const GainRange rg = gain_cull(v, radius, box, voxel);
    ++sums[0];
    sums[4] += (uint64_t)rg.n[0] * rg.n[1] * rg.n[2];
    for (int k = 0; k < 3; ++k)
      if (rg.n[k] && (rg.lo[k] < 0 || rg.lo[k] + rg.n[k] > box.n[k])) ++sums[3];  // a range that leaves the box
    for (int ix = 0; ix < box.n[0]; ++ix)
      for (int iy = 0; iy < box.n[1]; ++iy)
        for (int iz = 0; iz < box.n[2]; ++iz) {
          ++sums[1];
          if (!inside(v, radius, seen_centre(box.lo[0], ix, voxel), seen_centre(box.lo[1], iy, voxel), seen_centre(box.lo[2], iz, voxel))) continue;
          ++sums[2];
          const int a[3] = {ix, iy, iz};
          for (int k = 0; k < 3; ++k)
            if (a[k] < rg.lo[k] || a[k] >= rg.lo[k] + rg.n[k]) { ++sums[3]; break; }
        }
  }
  ok = ok && wr(o, sums, 5);
  fclose(f);
  if (fclose(o) != 0) ok = false;
  return ok ? 0 : 1;
}
