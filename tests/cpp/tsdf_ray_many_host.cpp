// tsdf_ray_many_host.cpp -- revo_tsdf_ray_many_host.h's rules for the batched surface ray cast on the host: the plan of a
// call (the distinct volumes found, the masks' offsets, the first_block sums, the view rows) against a restatement by plain loops,
// for 1 job, 1024 jobs, every job sharing one volume and no two sharing; and the overlap check: touching ranges accepted, one
// shared byte refused, volumes allowed to share among themselves.  Prints one line per case and "ok" at the end.
// Build: c++ -std=c++17 tsdf_ray_many_host.cpp (with host sanitizers where the toolchain has them).
#include <cstdio>
#include <string>
#include <vector>

#include "../../revo_amd/csrc/revo_tsdf_ray_many_host.h"

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static revo_map_df_box box_of(int lo, int n0, int n1, int n2) {
  revo_map_df_box b;
  b.lo[0] = lo; b.lo[1] = -lo; b.lo[2] = 2 * lo;
  b.n[0] = n0; b.n[1] = n1; b.n[2] = n2;
  return b;
}

static bool same_volume(const TsdfRayManyIn& a, const TsdfRayManyIn& b) {
  if (a.tsdf != b.tsdf || a.min_weight != b.min_weight) return false;
  for (int k = 0; k < 3; ++k)
    if (a.box.lo[k] != b.box.lo[k] || a.box.n[k] != b.box.n[k]) return false;
  return true;
}

// The plan of `jobs` against the definition, by plain loops.  -> the number of distinct volumes.
static int check_plan(const char* name, const std::vector<TsdfRayManyIn>& jobs, bool use_mask) {
  TsdfRayManyPlan p;
  tsdf_ray_many_plan(jobs, use_mask, &p);
  const size_t n = jobs.size();
  EXPECT(p.vol_of_job.size() == n && p.first_view.size() == n);
  // the distinct volumes, in the order of the first job that names them
  std::vector<int> first;
  for (size_t i = 0; i < n; ++i) {
    int v = -1;
    for (size_t k = 0; k < first.size(); ++k)
      if (same_volume(jobs[first[k]], jobs[i])) v = (int)k;
    if (v < 0) { v = (int)first.size(); first.push_back((int)i); }
    EXPECT(p.vol_of_job[i] == v);
  }
  EXPECT(p.job_of_vol == first);
  // masks one after another, each the single call's size; blocks of 256 cells one volume after another
  size_t off = 0, blocks = 0;
  for (size_t k = 0; k < first.size(); ++k) {
    const revo_map_df_box& b = jobs[first[k]].box;
    EXPECT(p.mask_off[k] == off && p.first_block[k] == blocks && off % 256 == 0);
    const size_t bits = (size_t)tsdf_ray_blocks(b.n[0]) * tsdf_ray_blocks(b.n[1]) * tsdf_ray_blocks(b.n[2]);
    const size_t bytes = (((bits + 31) / 32) * 4 + 255) / 256 * 256;
    EXPECT(tsdf_ray_mask_bytes(b) == bytes && bytes >= (bits + 7) / 8);
    off += bytes;
    blocks += ((size_t)b.n[0] * b.n[1] * b.n[2] + 255) / 256;
  }
  EXPECT(p.mask_bytes == off && p.mask_blocks == blocks);
  // every block of the mask launch finds its volume, and its cells lie in it
  const size_t probe = blocks < 4096 ? 1 : blocks / 2048;
  for (size_t b = 0; b < blocks; b += probe) {
    const int v = tsdf_many_find((int)first.size(), (unsigned)b, [&](int j) { return p.first_block[j]; });
    const size_t end = (size_t)v + 1 < first.size() ? p.first_block[v + 1] : blocks;
    EXPECT(p.first_block[v] <= b && b < end);
  }
  // the view rows: job after job, a row names its job
  size_t views = 0;
  for (size_t i = 0; i < n; ++i) {
    EXPECT(p.first_view[i] == views);
    for (int v = 0; v < jobs[i].n_views; ++v) EXPECT(views + v < p.row_job.size() && p.row_job[views + v] == (int)i);
    views += (size_t)jobs[i].n_views;
  }
  EXPECT(p.row_job.size() == views);
  // the scratch: lines | hit words | masks, 256-byte aligned parts that do not overlap
  EXPECT(p.off_hits >= 4 * TSDF_RAY_MANY_LINE * n && p.off_hits % 256 == 0);
  EXPECT(p.off_masks >= p.off_hits + 4 * views && p.off_masks % 256 == 0);
  EXPECT(p.total == p.off_masks + (use_mask ? p.mask_bytes : 0));
  printf("%s: jobs %zu distinct volumes %zu mask bytes %zu mask blocks %zu views %zu\n", name, n, first.size(), p.mask_bytes, p.mask_blocks, views);
  return (int)first.size();
}

typedef std::vector<std::pair<uintptr_t, size_t>> Ranges;

int main() {
  // ---- the plan
  {
    std::vector<TsdfRayManyIn> one{{0x1000, box_of(-4, 9, 9, 17), 1u, 64}};
    EXPECT(check_plan("one job", one, true) == 1);
    EXPECT(check_plan("one job, plain march", one, false) == 1);
  }
  {
    std::vector<TsdfRayManyIn> jobs;
    for (int i = 0; i < 1024; ++i) jobs.push_back({(uintptr_t)0x10000 + 0x1000 * (uintptr_t)i, box_of(i % 7 - 3, 2 + i % 5, 2 + i % 3, 2 + i % 11), 1u, 1 + i % 4});
    EXPECT(check_plan("1024 jobs, no two sharing", jobs, true) == 1024);
  }
  {
    std::vector<TsdfRayManyIn> jobs(1024, TsdfRayManyIn{0x2000, box_of(0, 128, 128, 128), 1u, 4});
    EXPECT(check_plan("1024 jobs sharing one volume", jobs, true) == 1);
  }
  {
    // what makes a volume distinct: the pointer, the box's place, its size, the effective min_weight
    const revo_map_df_box b = box_of(-2, 5, 5, 7);
    revo_map_df_box moved = b, longer = b;
    moved.lo[2] += 1;
    longer.n[1] += 1;
    std::vector<TsdfRayManyIn> jobs{{0x3000, b, 1u, 1}, {0x3000, b, 3u, 2}, {0x3000, b, 1u, 3}, {0x4000, b, 1u, 1}, {0x3000, moved, 1u, 1},
                                    {0x3000, longer, 1u, 2}, {0x3000, b, 3u, 64}, {0x4000, b, 1u, 5}};
    EXPECT(check_plan("mixed sharing", jobs, true) == 5);
    TsdfRayManyPlan p;
    tsdf_ray_many_plan(jobs, true, &p);
    EXPECT((p.vol_of_job == std::vector<int>{0, 1, 0, 2, 3, 4, 1, 2}));
  }
  {
    std::vector<TsdfRayManyIn> jobs;
    for (int i = 0; i < 64; ++i) jobs.push_back({(uintptr_t)0x5000 + 64 * (uintptr_t)i, box_of(-1, 2, 2, 2), 1u, 64});
    EXPECT(check_plan("64 jobs x 64 views", jobs, true) == 64);
  }
  {
    std::vector<TsdfRayManyIn> jobs{{0x6000, box_of(0, 1024, 1024, 128), 1u, 1}, {0x7000, box_of(0, 1, 1, 1), 1u, 1}, {0x8000, box_of(0, 1024, 1024, 128), 2u, 1}};
    EXPECT(check_plan("the largest boxes", jobs, true) == 3);
  }
  // ---- the overlap check
  {
    const Ranges volumes{{0x10000, 0x1000}, {0x10000, 0x1000}, {0x10800, 0x1000}, {0x20000, 0x100}};  // volumes may share
    EXPECT(!tsdf_ray_many_overlap(Ranges{{0x1000, 64}, {0x1040, 64}, {0x1080, 4}}, volumes));       // outputs that touch
    EXPECT(!tsdf_ray_many_overlap(Ranges{{0xff00, 0x100}, {0x11800, 16}}, volumes));                // an output that touches a volume, either end
    EXPECT(!tsdf_ray_many_overlap(Ranges{{0x20100, 64}, {0x1ffc0, 64}}, volumes));
    EXPECT(tsdf_ray_many_overlap(Ranges{{0x1000, 65}, {0x1040, 64}}, volumes));                     // one shared byte between outputs
    EXPECT(tsdf_ray_many_overlap(Ranges{{0x1000, 64}, {0x1000, 64}}, volumes));                     // the same output twice
    EXPECT(tsdf_ray_many_overlap(Ranges{{0x1000, 256}, {0x1010, 16}}, volumes));                    // one inside the other
    EXPECT(tsdf_ray_many_overlap(Ranges{{0xff00, 0x101}}, volumes));                                // one byte into a volume's first
    EXPECT(tsdf_ray_many_overlap(Ranges{{0x117ff, 16}}, volumes));                                  // ... its last (of the union)
    EXPECT(tsdf_ray_many_overlap(Ranges{{0x10ff0, 16}}, volumes));                                  // inside two volumes at once
    EXPECT(tsdf_ray_many_overlap(Ranges{{0x200ff, 1}}, volumes));
    EXPECT(!tsdf_ray_many_overlap(Ranges{}, volumes));
    const Ranges u = tsdf_ray_many_union(volumes);
    EXPECT((u == Ranges{{0x10000, 0x1800}, {0x20000, 0x100}}));
    EXPECT((tsdf_ray_many_union(Ranges{{0x100, 0x10}, {0x110, 0x10}, {0x90, 0x10}}) == Ranges{{0x90, 0x10}, {0x100, 0x20}}));  // touching ranges join
    printf("overlap: touching accepted, one shared byte refused\n");
  }
  if (failures) {
    printf("%d FAILED\n", failures);
    return 1;
  }
  printf("ok\n");
  return 0;
}
