// revo_tsdf_ray_many_host.h -- the host rules of revo_map_tsdf_raycast_many (include/revo_hip.h), each written once: which
// jobs of a call share a block mask, where the masks, the counter lines and the views' hit words lie in the call's scratch, how the
// blocks of the mask launch and the view rows of the march launch are dealt out, and when an output shares a byte with another
// output or with a volume.  The march, the mask's blocks and the per-view rules are revo_tsdf_ray_host.h's and revo_ray_host.h's,
// which the single call uses.  Plain C++ with no device code: revo_map_tsdf_ray_many.hip runs it over the caller's jobs,
// tests/cpp/tsdf_ray_many_host.cpp over jobs a test wrote.  Internal.
#pragma once
#include <cstring>
#include <map>
#include <tuple>

#include "revo_tsdf_many_host.h"
#include "revo_tsdf_ray_host.h"

#define TSDF_RAY_MANY_MAX_VIEWS 4096
#define TSDF_RAY_MANY_LINE 32  // words from one job's counter line to the next: a revo_map_tsdf_ray_info (16 words), the job's ticket, room to 128 bytes
#define TSDF_RAY_MANY_LINE_TICKET 16

// What the planner needs of a checked job.
struct TsdfRayManyIn {
  uintptr_t tsdf;
  revo_map_df_box box;
  uint32_t min_weight;  // the effective one, >= 1
  int n_views;
};

// The bytes of the mask of a box: a bit per block, whole words, rounded up to 256 bytes (the single call's size).
inline size_t tsdf_ray_mask_bytes(const revo_map_df_box& box) {
  const size_t blocks = (size_t)tsdf_ray_blocks(box.n[0]) * tsdf_ray_blocks(box.n[1]) * tsdf_ray_blocks(box.n[2]);
  return (((blocks + 31) / 32) * 4 + 255) & ~(size_t)255;
}

// The plan of a call.  A distinct volume is a distinct (tsdf pointer, box, effective min_weight): what the mask is a function of
// besides the volume's bytes.  The distinct volumes are numbered in the order of the first job that names them.
struct TsdfRayManyPlan {
  std::vector<int> vol_of_job;            // job -> its distinct volume
  std::vector<int> job_of_vol;            // distinct volume -> the first job that names it
  std::vector<size_t> mask_off;           // distinct volume -> its mask's bytes from the first mask's
  std::vector<unsigned> first_block;      // distinct volume -> its first block of the mask launch (tsdf_many_find), 256 cells a block
  std::vector<unsigned> first_view;       // job -> its first view row
  std::vector<int> row_job;               // view row -> its job
  size_t mask_bytes = 0;                  // all masks
  size_t mask_blocks = 0;                 // the mask launch's grid
  // the scratch, cleared by one memset: the jobs' lines | the view rows' hit words | the masks
  size_t off_hits = 0, off_masks = 0, total = 0;
};

inline void tsdf_ray_many_plan(const std::vector<TsdfRayManyIn>& jobs, bool use_mask, TsdfRayManyPlan* p) {
  typedef std::tuple<uintptr_t, int, int, int, int, int, int, uint32_t> Key;
  std::map<Key, int> seen;
  const size_t n = jobs.size();
  *p = TsdfRayManyPlan{};
  p->vol_of_job.resize(n);
  p->first_view.resize(n);
  size_t views = 0;
  for (size_t i = 0; i < n; ++i) {
    const TsdfRayManyIn& j = jobs[i];
    const Key k(j.tsdf, j.box.lo[0], j.box.lo[1], j.box.lo[2], j.box.n[0], j.box.n[1], j.box.n[2], j.min_weight);
    auto it = seen.find(k);
    if (it == seen.end()) {
      it = seen.emplace(k, (int)p->job_of_vol.size()).first;
      p->job_of_vol.push_back((int)i);
      p->mask_off.push_back(p->mask_bytes);
      p->first_block.push_back((unsigned)p->mask_blocks);
      p->mask_bytes += tsdf_ray_mask_bytes(j.box);
      p->mask_blocks += ((size_t)j.box.n[0] * j.box.n[1] * j.box.n[2] + 255) / 256;
    }
    p->vol_of_job[i] = it->second;
    p->first_view[i] = (unsigned)views;
    for (int v = 0; v < j.n_views; ++v) p->row_job.push_back((int)i);
    views += (size_t)j.n_views;
  }
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  p->off_hits = up(sizeof(uint32_t) * TSDF_RAY_MANY_LINE * n);
  p->off_masks = p->off_hits + up(sizeof(uint32_t) * views);
  p->total = p->off_masks + (use_mask ? p->mask_bytes : 0);
}

// The union of byte ranges as disjoint ranges in ascending order: ranges that overlap or touch become one.
inline std::vector<std::pair<uintptr_t, size_t>> tsdf_ray_many_union(std::vector<std::pair<uintptr_t, size_t>> ranges) {
  std::sort(ranges.begin(), ranges.end());
  std::vector<std::pair<uintptr_t, size_t>> out;
  for (const auto& r : ranges) {
    if (!out.empty() && out.back().first + out.back().second >= r.first) {
      const uintptr_t end = std::max(out.back().first + out.back().second, r.first + r.second);
      out.back().second = (size_t)(end - out.back().first);
    } else {
      out.push_back(r);
    }
  }
  return out;
}

// Whether two outputs share a byte, or an output shares one with a volume.  Volumes may share bytes with each other: they are
// only read.  The volumes go in as their union, so the sorted-ranges check of revo_map_tsdf_fuse_many decides both questions.
inline bool tsdf_ray_many_overlap(const std::vector<std::pair<uintptr_t, size_t>>& outputs, const std::vector<std::pair<uintptr_t, size_t>>& volumes) {
  std::vector<std::pair<uintptr_t, size_t>> all = tsdf_ray_many_union(volumes);
  all.insert(all.end(), outputs.begin(), outputs.end());
  return tsdf_many_overlap(all);
}
