// revo_tsdf_many_host.h -- the rules of the batched surface calls (include/revo_hip.h) that host and device code share,
// each written once: how the blocks of one launch are dealt out to the jobs of a batched fuse and how a block finds its job, the
// counter line of a job, how many workgroups a pose of a batched tracking launch gets, and when two volumes share a byte.  The
// per-cell and per-pixel rules are not here: they are revo_tsdf_host.h's and revo_tsdf_track_host.h's, which the single calls use.
// Plain C++: revo_map_tsdf_many.hip compiles it for both sides, tests/cpp/align_stepper_host.cpp for the host alone.  Internal.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "revo_cell_run.h"
#include "revo_tsdf_host.h"

#define TSDF_MANY_MAX_JOBS 1024
#define TSDF_MANY_THREADS CELL_RUN_THREADS  // k_tsdf_fuse's block
// A job's counter line in the launch's scratch, 32 words: revo_map_tsdf_info | revo_map_tsdf_color_info | revo_map_carve_view_info.
#define TSDF_MANY_LINE 32
#define TSDF_MANY_STRIDE 64      // words from one job's line to the next: the line, the job's ticket, and room to 256 bytes
#define TSDF_MANY_LINE_TICKET 32 // the job's blocks that are done; beside the counters, so the same memory channel serves both
#define TSDF_MANY_LINE_CINFO 16
#define TSDF_MANY_LINE_VINFO 24

// The blocks a job of `cells` cells takes: k_tsdf_fuse's grid for that box.
TSDF_HD unsigned tsdf_many_blocks(size_t cells) { return cell_run_blocks(cells); }

// The jobs take the launch's blocks one after another: job j the blocks first(j) .. first(j) + blocks(j) - 1, first(0) = 0, every
// job at least one.  The job of `block` (< the total) is the last one whose first block is not behind it: a bisection over the
// table, uniform over the block.
template <class First>
TSDF_HD int tsdf_many_find(int n_jobs, unsigned block, First&& first) {
  int lo = 0, hi = n_jobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first(mid) <= block) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The workgroups every pose of a batched tracking launch gets: revo_map_tsdf_track_eval's rule on the largest lattice of the
// launch (blocks: its 32 x 8 pixel blocks) and all poses together.  forced > 0: REVO_MAP_TSDF_TRACK_GROUPS.
inline size_t tsdf_many_groups(size_t blocks, size_t n_poses, int forced, size_t max_groups, size_t max_total) {
  size_t G = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(blocks, max_groups), max_total / n_poses));
  if (forced > 0) G = std::max<size_t>(1, std::min<size_t>((size_t)forced, max_total / n_poses));
  return G;
}

// Whether two of the byte ranges [begin, begin + bytes) share a byte; the ranges are sorted in place.
inline bool tsdf_many_overlap(std::vector<std::pair<uintptr_t, size_t>>& ranges) {
  std::sort(ranges.begin(), ranges.end());
  for (size_t i = 1; i < ranges.size(); ++i)
    if (ranges[i - 1].first + ranges[i - 1].second > ranges[i].first) return true;
  return false;
}
