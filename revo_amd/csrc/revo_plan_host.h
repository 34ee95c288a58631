// revo_plan_host.h -- what revo_map_plan / revo_map_plan_paths (include/revo_hip.h) need no device for: the rules the
// arguments must meet before anything is enqueued, the classification of a seed, the geometry of the 8 x 8 x 8 tiles the
// relaxation works in, and the round loop -- written against a callback "run this many rounds, say how many tiles are marked
// for the next one".  Plain C++: revo_map_plan.hip runs it over the caller's arguments and its kernels (the functions marked
// PLAN_HD are the kernels' too), tests/cpp/plan_host.cpp over a CPU stand-in for the relaxation kernel.  Internal.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/revo_hip.h"

#if defined(__HIPCC__)
#define PLAN_HD __host__ __device__ inline
#else
#define PLAN_HD inline
#endif

#define PLAN_INF (1u << 30)      // a free cell no seed has reached: above every cost (< 2^24 + 5 * 2^27)
#define PLAN_BLOCKED (1u << 31)  // a cell that is not free, or outside the box: PLAN_BLOCKED + 5 does not wrap and stays above PLAN_INF
#define PLAN_TILE 8              // cells per tile edge: narrower corridors than this make a path re-enter tiles
#define PLAN_MAX_N 1024
#define PLAN_MAX_CELLS ((size_t)1 << 27)
#define PLAN_MAX_SEEDS ((size_t)1 << 20)
#define PLAN_MAX_COST0 (1u << 24)
#define PLAN_MAX_STARTS ((size_t)1 << 20)
#define PLAN_MAX_LEN (1u << 20)
#define PLAN_DEFAULT_ROUNDS 65536u
#define PLAN_GROUP 8u            // rounds enqueued between two looks at the marked-tile count

enum { PLAN_SEED_USED = 0, PLAN_SEED_OUTSIDE = 1, PLAN_SEED_BLOCKED = 2 };

// the box rules of revo_map_distance_field; nullptr if the box keeps them
inline const char* plan_box_check(const revo_map_df_box* box, size_t* cells) {
  size_t n = 1;
  for (int k = 0; k < 3; ++k) {
    if (box->n[k] < 1 || box->n[k] > PLAN_MAX_N) return "a box size must be 1 .. 1024 cells";
    if (box->lo[k] < -(1 << 20) || (long long)box->lo[k] + box->n[k] - 1 > (1 << 20) - 1) return "the box leaves the voxel index range [-2^20, 2^20 - 1]";
    n *= (size_t)box->n[k];
  }
  if (n > PLAN_MAX_CELLS) return "the box holds more than 2^27 cells";
  *cells = n;
  return nullptr;
}
inline bool plan_flag_ok(int flag) { return flag == 0 || flag == 1; }
inline bool plan_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// Why revo_map_plan refuses its arguments, or nullptr; *cells the box's cells, *rounds the round limit in force.
inline const char* plan_args_check(const void* m, const revo_map_df_box* box, const uint32_t* d2, int device_field, uint32_t r2, size_t n_seeds,
                                   const revo_map_plan_seed* seeds, uint32_t max_rounds, const uint32_t* cost, int device_out,
                                   const revo_map_plan_info* info, size_t* cells, uint32_t* rounds) {
  if (!m || !box || !d2 || !seeds || !cost) return "null argument";
  if (const char* why = plan_box_check(box, cells)) return why;
  if (r2 < 1) return "r2 must be >= 1";
  if (n_seeds < 1 || n_seeds > PLAN_MAX_SEEDS) return "n_seeds must be 1 .. 2^20";
  if (!plan_flag_ok(device_field)) return "device_field must be 0 or 1";
  if (!plan_flag_ok(device_out)) return "device_out must be 0 or 1";
  if (device_field && !plan_aligned16(d2)) return "the device field is not 16-byte aligned";
  if (device_out && (!plan_aligned16(cost) || !plan_aligned16(info))) return "a device output is not 16-byte aligned";
  for (size_t i = 0; i < n_seeds; ++i)
    if (seeds[i].cost0 > PLAN_MAX_COST0) return "a seed's cost0 is above 2^24";
  *rounds = max_rounds ? max_rounds : PLAN_DEFAULT_ROUNDS;
  return nullptr;
}

// Why revo_map_plan_paths refuses its arguments, or nullptr.
inline const char* plan_paths_args_check(const void* m, const revo_map_df_box* box, const uint32_t* cost, int device_cost, size_t n_starts,
                                         const int32_t* starts, uint32_t max_len, const int32_t* cells_out, const revo_map_plan_path* path_out,
                                         int device_out, size_t* cells) {
  if (!m || !box || !cost || !starts || !cells_out || !path_out) return "null argument";
  if (n_starts < 1 || n_starts > PLAN_MAX_STARTS) return "n_starts must be 1 .. 2^20";
  if (max_len < 1 || max_len > PLAN_MAX_LEN) return "max_len must be 1 .. 2^20";
  if (const char* why = plan_box_check(box, cells)) return why;
  if (!plan_flag_ok(device_cost)) return "device_cost must be 0 or 1";
  if (!plan_flag_ok(device_out)) return "device_out must be 0 or 1";
  if (device_cost && !plan_aligned16(cost)) return "the device cost field is not 16-byte aligned";
  if (device_out && (!plan_aligned16(cells_out) || !plan_aligned16(path_out))) return "a device output is not 16-byte aligned";
  return nullptr;
}

// The cell of a voxel index inside the box as an offset into the field's layout, or false: outside.
PLAN_HD bool plan_cell_index(const revo_map_df_box& box, int x, int y, int z, unsigned* at) {
  const unsigned dx = (unsigned)(x - box.lo[0]), dy = (unsigned)(y - box.lo[1]), dz = (unsigned)(z - box.lo[2]);
  if (dx >= (unsigned)box.n[0] || dy >= (unsigned)box.n[1] || dz >= (unsigned)box.n[2]) return false;
  *at = (dx * (unsigned)box.n[1] + dy) * (unsigned)box.n[2] + dz;
  return true;
}
// What becomes of a seed: `code` is the internal code of its cell (read only when the seed is inside).
template <typename Code>
PLAN_HD int plan_seed_class(const revo_map_df_box& box, const revo_map_plan_seed& s, Code code, unsigned* at) {
  if (!plan_cell_index(box, s.cell[0], s.cell[1], s.cell[2], at)) return PLAN_SEED_OUTSIDE;
  return code(*at) >= PLAN_BLOCKED ? PLAN_SEED_BLOCKED : PLAN_SEED_USED;
}
// the weight of the move (dx, dy, dz), each -1, 0, 1 and not all zero: 3, 4 or 5
PLAN_HD unsigned plan_weight(int dx, int dy, int dz) { return 2u + (unsigned)((dx != 0) + (dy != 0) + (dz != 0)); }

// The tiles of a box: t[k] = ceil(n[k] / 8) per axis, tile (tx, ty, tz) at (tx * t[1] + ty) * t[2] + tz.
struct PlanTiles {
  int t[3];
  unsigned count;
};
PLAN_HD PlanTiles plan_tiles(const revo_map_df_box& box) {
  PlanTiles g;
  for (int k = 0; k < 3; ++k) g.t[k] = (box.n[k] + PLAN_TILE - 1) / PLAN_TILE;
  g.count = (unsigned)g.t[0] * (unsigned)g.t[1] * (unsigned)g.t[2];
  return g;
}
PLAN_HD unsigned plan_tile_of_cell(const PlanTiles& g, unsigned dx, unsigned dy, unsigned dz) {
  return ((dx / PLAN_TILE) * (unsigned)g.t[1] + dy / PLAN_TILE) * (unsigned)g.t[2] + dz / PLAN_TILE;
}
// The neighbour tiles whose halo holds the cell at (cx, cy, cz) of its own tile, each 0 .. 7: bit (dx+1)*9 + (dy+1)*3 + (dz+1)
// for the tile at (dx, dy, dz), the own tile (bit 13) left out.  A step of -1 needs the coordinate 0, a step of +1 the coordinate 7.
PLAN_HD unsigned plan_halo_mask(int cx, int cy, int cz) {
  unsigned mask = 0;
  for (int dx = -1; dx <= 1; ++dx)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dz = -1; dz <= 1; ++dz) {
        const bool in = (dx == 0 || cx == (dx < 0 ? 0 : PLAN_TILE - 1)) && (dy == 0 || cy == (dy < 0 ? 0 : PLAN_TILE - 1)) &&
                        (dz == 0 || cz == (dz < 0 ? 0 : PLAN_TILE - 1));
        if (in && (dx | dy | dz)) mask |= 1u << ((dx + 1) * 9 + (dy + 1) * 3 + (dz + 1));
      }
  return mask;
}

// The round loop.  run(k, &marked) enqueues k rounds, waits for them and says how many tiles are marked for the round after
// them; 0 is the fixed point.  REVO_OK with *done the rounds run, REVO_ERR_CAPACITY when `limit` rounds were not enough, or
// run's own error.
template <typename Run>
inline int plan_round_loop(uint32_t limit, uint32_t group, Run run, uint32_t* done) {
  *done = 0;
  while (*done < limit) {
    const uint32_t k = limit - *done < group ? limit - *done : group;
    uint32_t marked = 0;
    if (const int rc = run(k, &marked)) return rc;
    *done += k;
    if (marked == 0) return REVO_OK;
  }
  return REVO_ERR_CAPACITY;
}
