// tsdf_ray_host.cpp -- revo_tsdf_ray_host.h's rules for the surface ray cast on the host: the program reads cases from a
// binary file and prints what the header makes of them, one line each, floats as their bits; tests/test_map_tsdf_ray_cpu.py compares
// the lines with the specification's numbers.  The march runs twice over every ray, plain and through a block mask that the program
// builds from the mask's definition, cell by cell.
// Build: c++ -std=c++17 -ffp-contract=off tsdf_ray_host.cpp (with host sanitizers where the toolchain has them).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../revo_amd/csrc/revo_tsdf_ray_host.h"

static unsigned bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}

template <typename T>
static bool get(FILE* f, T* out, size_t n = 1) { return fread(out, sizeof(T), n, f) == n; }

static void print_march(const char* tag, int st, const TsdfRayOut& o) {
  printf("%s %d %u %u %u %u %u %u %u %u %u\n", tag, st, o.samples, bits(o.depth), bits(o.nx), bits(o.ny), bits(o.nz), (unsigned)o.b, (unsigned)o.g,
         (unsigned)o.r, o.colored);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  float voxel = 0.0f;
  unsigned n = 0;
  // the parameter rules: has, step, min_weight, max_steps, reserved
  if (!get(f, &voxel) || !get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    uint32_t has;
    revo_map_tsdf_ray_params p, out;
    if (!get(f, &has) || !get(f, &p.step) || !get(f, &p.min_weight) || !get(f, &p.max_steps) || !get(f, &p.reserved)) return 3;
    const char* why = tsdf_ray_params_check(has ? &p : nullptr, voxel, &out);
    if (why) printf("params refused\n");
    else printf("params %u %u %u\n", bits(out.step), out.min_weight, out.max_steps);
  }
  // a sample's depth: zmin, k, step
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    float zmin, step;
    uint32_t k;
    if (!get(f, &zmin) || !get(f, &k) || !get(f, &step)) return 3;
    printf("s %u\n", bits(tsdf_ray_s(zmin, k, step)));
  }
  // one axis of a sample's place, at the box's rims: o, s, d, lo, n
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    float o, s, d, r = 0.0f;
    int32_t lo, cells, b = 0;
    if (!get(f, &o) || !get(f, &s) || !get(f, &d) || !get(f, &lo) || !get(f, &cells)) return 3;
    const bool ok = tsdf_ray_axis(o, s, d, voxel, lo, cells, &b, &r);
    if (ok) printf("axis 1 %d %u\n", b, bits(r));
    else printf("axis 0\n");
  }
  // the nearest corner: b, r
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    int32_t b;
    float r;
    if (!get(f, &b) || !get(f, &r)) return 3;
    printf("near %d\n", tsdf_ray_near(b, r));
  }
  // the decision between two valid samples: Fp, F
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    float Fp, F;
    if (!get(f, &Fp) || !get(f, &F)) return 3;
    printf("decide %d\n", tsdf_ray_decide(Fp, F));
  }
  // the interpolant and its gradient in one cube: eight cells (x slowest, z fastest), rx, ry, rz, min_weight
  if (!get(f, &n)) return 3;
  for (unsigned i = 0; i < n; ++i) {
    revo_map_tsdf_cell cube[8];
    TsdfRayPlace p{true, 0, 0, 0, 0.0f, 0.0f, 0.0f};
    TsdfRayK a{};
    if (!get(f, cube, 8) || !get(f, &p.rx) || !get(f, &p.ry) || !get(f, &p.rz) || !get(f, &a.min_weight)) return 3;
    a.tsdf = cube;
    a.box = revo_map_df_box{{0, 0, 0}, {2, 2, 2}};
    TsdfRaySample smp;
    tsdf_ray_sample(a, p, 1.0f, &smp);
    printf("sample %d %u %u %u %u %u\n", (int)smp.valid, bits(smp.F), bits(smp.gx), bits(smp.gy), bits(smp.gz), smp.ccell);
  }
  // the march: lo, n, the cells, has_color, the colour cells, step, min_weight, max_steps, rays of ox oy oz dx dy dz zmin zmax
  unsigned volumes = 0;
  if (!get(f, &volumes)) return 3;
  for (unsigned v = 0; v < volumes; ++v) {
    TsdfRayK a{};
    uint32_t has_color = 0;
    if (!get(f, a.box.lo, 3) || !get(f, a.box.n, 3)) return 3;
    const size_t cells = (size_t)a.box.n[0] * a.box.n[1] * a.box.n[2];
    std::vector<revo_map_tsdf_cell> vol(cells);
    std::vector<revo_map_tsdf_color> col;
    if (!get(f, vol.data(), cells) || !get(f, &has_color)) return 3;
    if (has_color) {
      col.resize(cells);
      if (!get(f, col.data(), cells)) return 3;
    }
    if (!get(f, &a.step) || !get(f, &a.min_weight) || !get(f, &a.max_steps) || !get(f, &n)) return 3;
    a.tsdf = vol.data();
    a.color = has_color ? col.data() : nullptr;
    a.voxel = voxel;
    const int nbx = tsdf_ray_blocks(a.box.n[0]);
    a.nby = tsdf_ray_blocks(a.box.n[1]);
    a.nbz = tsdf_ray_blocks(a.box.n[2]);
    // the mask from its definition: a block is marked when it holds a base one of whose eight corners is an INSIDE cell
    std::vector<uint32_t> mask(((size_t)nbx * a.nby * a.nbz + 31) / 32, 0u);
    const size_t nz = (size_t)a.box.n[2], nyz = (size_t)a.box.n[1] * nz;
    unsigned marked = 0;
    for (int bx = 0; bx <= a.box.n[0] - 2; ++bx)
      for (int by = 0; by <= a.box.n[1] - 2; ++by)
        for (int bz = 0; bz <= a.box.n[2] - 2; ++bz) {
          bool any = false;
          for (int o = 0; o < 8; ++o) {
            const revo_map_tsdf_cell c = vol[(size_t)(bx + (o & 1)) * nyz + (size_t)(by + ((o >> 1) & 1)) * nz + (size_t)(bz + ((o >> 2) & 1))];
            any = any || tsdf_inside(c.sum, c.weight, a.min_weight);
          }
          if (!any) continue;
          const uint32_t blk = tsdf_ray_block(a.nby, a.nbz, bx, by, bz);
          if (blk >= (uint32_t)(nbx * a.nby * a.nbz)) return 4;
          marked += !((mask[blk >> 5] >> (blk & 31u)) & 1u);
          mask[blk >> 5] |= 1u << (blk & 31u);
        }
    a.mask = mask.data();
    printf("mask %d %d %d %u\n", nbx, a.nby, a.nbz, marked);
    for (unsigned i = 0; i < n; ++i) {
      float r[8];
      if (!get(f, r, 8)) return 3;
      const TsdfRay ray{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
      TsdfRayOut plain, masked;
      const int sp = tsdf_ray_march<false>(a, ray, &plain);
      const int sm = tsdf_ray_march<true>(a, ray, &masked);
      print_march("march", sp, plain);
      print_march("masked", sm, masked);
    }
  }
  fclose(f);
  return 0;
}
