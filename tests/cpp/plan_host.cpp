// The host side of revo_map_plan / revo_map_plan_paths (revo_amd/csrc/revo_plan_host.h) without a GPU: a plain C++ program.
//   plan_host rules          replays the argument rules; exit status 0 when every one holds
//   plan_host plan IN OUT    plans a recorded case: the header's seed classification, tile geometry and round loop over a CPU
//                            stand-in for the relaxation kernel (a tile is relaxed against its neighbours in place until nothing
//                            changes, and marks the tiles plan_halo_mask names for the next round)
// IN: lo[3], n[3] (i32), r2, n_seeds, max_rounds (u32), the seeds (16 bytes each), d2 (u32 per cell).
// OUT: the return code (i32), the rounds the loop ran (u32), the info record (64 bytes), the cost field (u32 per cell).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../revo_amd/csrc/revo_plan_host.h"

#define EXPECT(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int rules() {
  alignas(16) static uint32_t buf[64];
  int dummy = 0;
  const void* m = &dummy;
  const revo_map_df_box good{{-3, 0, 5}, {4, 3, 5}};
  revo_map_plan_seed seeds[2] = {{{0, 0, 5}, 0}, {{-3, 2, 9}, PLAN_MAX_COST0}};
  size_t cells = 0;
  uint32_t rounds = 0;
  const uint32_t* d2 = buf;
  uint32_t* cost = buf + 16;
  const revo_map_plan_info* info = (const revo_map_plan_info*)(buf + 32);
  auto plan = [&](const void* mm, const revo_map_df_box* b, const uint32_t* f, int df, uint32_t r2, size_t ns, const revo_map_plan_seed* s, uint32_t mr,
                  const uint32_t* c, int dout, const revo_map_plan_info* i) { return plan_args_check(mm, b, f, df, r2, ns, s, mr, c, dout, i, &cells, &rounds); };
  EXPECT(!plan(m, &good, d2, 0, 1, 2, seeds, 0, cost, 0, info) && cells == 60 && rounds == PLAN_DEFAULT_ROUNDS);
  EXPECT(!plan(m, &good, d2, 1, 9, 2, seeds, 7, cost, 1, nullptr) && rounds == 7);
  EXPECT(plan(nullptr, &good, d2, 0, 1, 2, seeds, 0, cost, 0, info) && plan(m, nullptr, d2, 0, 1, 2, seeds, 0, cost, 0, info));
  EXPECT(plan(m, &good, nullptr, 0, 1, 2, seeds, 0, cost, 0, info) && plan(m, &good, d2, 0, 1, 2, nullptr, 0, cost, 0, info));
  EXPECT(plan(m, &good, d2, 0, 1, 2, seeds, 0, nullptr, 0, info));
  EXPECT(plan(m, &good, d2, 0, 0, 2, seeds, 0, cost, 0, info));  // r2 = 0
  EXPECT(plan(m, &good, d2, 0, 1, 0, seeds, 0, cost, 0, info) && plan(m, &good, d2, 0, 1, PLAN_MAX_SEEDS + 1, seeds, 0, cost, 0, info));
  EXPECT(plan(m, &good, d2, 2, 1, 2, seeds, 0, cost, 0, info) && plan(m, &good, d2, 0, 1, 2, seeds, 0, cost, -1, info));
  EXPECT(plan(m, &good, d2 + 1, 1, 1, 2, seeds, 0, cost, 0, info) && !plan(m, &good, d2 + 1, 0, 1, 2, seeds, 0, cost, 0, info));
  EXPECT(plan(m, &good, d2, 0, 1, 2, seeds, 0, cost + 1, 1, info) && plan(m, &good, d2, 0, 1, 2, seeds, 0, cost, 1, (const revo_map_plan_info*)(buf + 33)));
  seeds[1].cost0 = PLAN_MAX_COST0 + 1;
  EXPECT(plan(m, &good, d2, 0, 1, 2, seeds, 0, cost, 0, info) && !plan(m, &good, d2, 0, 1, 1, seeds, 0, cost, 0, info));
  seeds[1].cost0 = 0;
  const int R = 1 << 20;
  const revo_map_df_box bad[] = {{{0, 0, 0}, {0, 3, 5}}, {{0, 0, 0}, {4, -1, 5}}, {{0, 0, 0}, {4, 3, 1025}}, {{0, 0, 0}, {1024, 1024, 129}}, {{-R - 1, 0, 0}, {4, 3, 5}},
                                 {{0, R - 2, 0}, {4, 3, 5}}, {{0, 0, R}, {1, 1, 1}}, {{INT32_MIN, 0, 0}, {4, 3, 5}}, {{INT32_MAX, 0, 0}, {4, 3, 5}}};
  const int32_t starts[3] = {0, 0, 0};
  const int32_t* out = (const int32_t*)buf;
  const revo_map_plan_path* rec = (const revo_map_plan_path*)(buf + 32);
  for (const revo_map_df_box& b : bad) {
    EXPECT(plan(m, &b, d2, 0, 1, 2, seeds, 0, cost, 0, info));
    EXPECT(plan_paths_args_check(m, &b, d2, 0, 1, starts, 8, out, rec, 0, &cells));
  }
  const revo_map_df_box rim{{-R, R - 4, -R}, {1024, 4, 1}}, full{{0, 0, 0}, {1024, 1024, 128}};
  EXPECT(!plan(m, &rim, d2, 0, 1, 2, seeds, 0, cost, 0, info) && !plan(m, &full, d2, 0, 1, 2, seeds, 0, cost, 0, info) && cells == PLAN_MAX_CELLS);
  // revo_map_plan_paths
  EXPECT(!plan_paths_args_check(m, &good, d2, 0, 1, starts, 1, out, rec, 0, &cells) && cells == 60);
  EXPECT(!plan_paths_args_check(m, &good, d2, 1, PLAN_MAX_STARTS, starts, PLAN_MAX_LEN, out, rec, 1, &cells));
  EXPECT(plan_paths_args_check(nullptr, &good, d2, 0, 1, starts, 1, out, rec, 0, &cells) && plan_paths_args_check(m, nullptr, d2, 0, 1, starts, 1, out, rec, 0, &cells));
  EXPECT(plan_paths_args_check(m, &good, nullptr, 0, 1, starts, 1, out, rec, 0, &cells) && plan_paths_args_check(m, &good, d2, 0, 1, nullptr, 1, out, rec, 0, &cells));
  EXPECT(plan_paths_args_check(m, &good, d2, 0, 1, starts, 1, nullptr, rec, 0, &cells) && plan_paths_args_check(m, &good, d2, 0, 1, starts, 1, out, nullptr, 0, &cells));
  EXPECT(plan_paths_args_check(m, &good, d2, 0, 0, starts, 1, out, rec, 0, &cells) && plan_paths_args_check(m, &good, d2, 0, PLAN_MAX_STARTS + 1, starts, 1, out, rec, 0, &cells));
  EXPECT(plan_paths_args_check(m, &good, d2, 0, 1, starts, 0, out, rec, 0, &cells) && plan_paths_args_check(m, &good, d2, 0, 1, starts, PLAN_MAX_LEN + 1, out, rec, 0, &cells));
  EXPECT(plan_paths_args_check(m, &good, d2, 2, 1, starts, 1, out, rec, 0, &cells) && plan_paths_args_check(m, &good, d2, 0, 1, starts, 1, out, rec, 3, &cells));
  EXPECT(plan_paths_args_check(m, &good, d2 + 2, 1, 1, starts, 1, out, rec, 0, &cells) && plan_paths_args_check(m, &good, d2, 0, 1, starts, 1, out + 1, rec, 1, &cells));
  EXPECT(plan_paths_args_check(m, &good, d2, 0, 1, starts, 1, out, (const revo_map_plan_path*)(buf + 34), 1, &cells));
  // the geometry: weights, tiles, halo masks
  EXPECT(plan_weight(1, 0, 0) == 3 && plan_weight(0, -1, 1) == 4 && plan_weight(-1, 1, -1) == 5);
  const revo_map_df_box t{{0, 0, 0}, {17, 8, 7}};
  const PlanTiles g = plan_tiles(t);
  EXPECT(g.t[0] == 3 && g.t[1] == 1 && g.t[2] == 1 && g.count == 3 && plan_tile_of_cell(g, 16, 7, 6) == 2 && plan_tile_of_cell(g, 7, 0, 0) == 0);
  EXPECT(plan_halo_mask(3, 4, 5) == 0 && plan_halo_mask(0, 4, 5) == 1u << 4 && plan_halo_mask(7, 4, 5) == 1u << 22);
  EXPECT(__builtin_popcount(plan_halo_mask(0, 0, 3)) == 3 && __builtin_popcount(plan_halo_mask(7, 0, 7)) == 7 && (plan_halo_mask(7, 7, 7) >> 26) == 1);
  unsigned at = 0;
  EXPECT(plan_cell_index(good, -3, 0, 5, &at) && at == 0 && plan_cell_index(good, 0, 2, 9, &at) && at == 59 && !plan_cell_index(good, 1, 0, 5, &at) && !plan_cell_index(good, 0, 0, 4, &at));
  return 0;
}

struct Plan {
  revo_map_df_box box;
  PlanTiles tiles;
  std::vector<uint32_t> cost;
  std::vector<unsigned char> flags[2];
  uint32_t round = 0;

  unsigned cell(int x, int y, int z) const { return ((unsigned)x * (unsigned)box.n[1] + (unsigned)y) * (unsigned)box.n[2] + (unsigned)z; }
  uint32_t at(int x, int y, int z) const {
    return x >= 0 && y >= 0 && z >= 0 && x < box.n[0] && y < box.n[1] && z < box.n[2] ? cost[cell(x, y, z)] : PLAN_BLOCKED;
  }
  // the stand-in for one workgroup of k_plan_relax: returns with the tile's cells settled against their neighbours
  void relax_tile(int tx, int ty, int tz, std::vector<unsigned char>& next) {
    unsigned mask = 0;
    for (bool any = true; any;) {
      any = false;
      for (int cx = 0; cx < PLAN_TILE; ++cx)
        for (int cy = 0; cy < PLAN_TILE; ++cy)
          for (int cz = 0; cz < PLAN_TILE; ++cz) {
            const int x = tx * PLAN_TILE + cx, y = ty * PLAN_TILE + cy, z = tz * PLAN_TILE + cz;
            const uint32_t cur = at(x, y, z);
            if (cur >= PLAN_BLOCKED) continue;
            uint32_t best = cur;
            for (int dx = -1; dx <= 1; ++dx)
              for (int dy = -1; dy <= 1; ++dy)
                for (int dz = -1; dz <= 1; ++dz)
                  if (dx | dy | dz) best = std::min(best, at(x + dx, y + dy, z + dz) + plan_weight(dx, dy, dz));
            if (best < cur) { cost[cell(x, y, z)] = best; mask |= plan_halo_mask(cx, cy, cz); any = true; }
          }
    }
    for (int b = 0; b < 27; ++b)
      if ((mask >> b) & 1u) {
        const int ux = tx + b / 9 - 1, uy = ty + b / 3 % 3 - 1, uz = tz + b % 3 - 1;
        if (ux >= 0 && uy >= 0 && uz >= 0 && ux < tiles.t[0] && uy < tiles.t[1] && uz < tiles.t[2])
          next[((unsigned)ux * (unsigned)tiles.t[1] + (unsigned)uy) * (unsigned)tiles.t[2] + (unsigned)uz] = 1;
      }
  }
  int run(uint32_t k, uint32_t* marked) {
    for (uint32_t j = 0; j < k; ++j, ++round) {
      std::vector<unsigned char>& cur = flags[round & 1];
      std::vector<unsigned char>& next = flags[(round + 1) & 1];
      for (unsigned t = 0; t < tiles.count; ++t)
        if (cur[t]) {
          cur[t] = 0;
          relax_tile((int)(t / ((unsigned)tiles.t[2] * (unsigned)tiles.t[1])), (int)(t / (unsigned)tiles.t[2] % (unsigned)tiles.t[1]), (int)(t % (unsigned)tiles.t[2]), next);
        }
    }
    *marked = 0;
    for (unsigned char f : flags[round & 1]) *marked += f;
    return REVO_OK;
  }
};

static int plan(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return 2;
  Plan p;
  uint32_t r2 = 0, n_seeds = 0, max_rounds = 0;
  bool ok = fread(&p.box, sizeof(p.box), 1, f) == 1 && fread(&r2, 4, 1, f) == 1 && fread(&n_seeds, 4, 1, f) == 1 && fread(&max_rounds, 4, 1, f) == 1 &&
            n_seeds <= PLAN_MAX_SEEDS;
  std::vector<revo_map_plan_seed> seeds(ok ? n_seeds : 0);
  ok = ok && fread(seeds.data(), sizeof(revo_map_plan_seed), seeds.size(), f) == seeds.size();
  size_t cells = 0;
  ok = ok && !plan_box_check(&p.box, &cells);
  std::vector<uint32_t> d2(ok ? cells : 0);
  ok = ok && fread(d2.data(), 4, cells, f) == cells;
  fclose(f);
  if (!ok) return 2;
  p.cost.assign(cells, 0);
  uint32_t limit = 0;
  revo_map_plan_info info{};
  if (const char* why = plan_args_check(&p, &p.box, d2.data(), 0, r2, n_seeds, seeds.data(), max_rounds, p.cost.data(), 0, &info, &cells, &limit)) {
    fprintf(stderr, "%s\n", why);
    return 3;
  }
  p.tiles = plan_tiles(p.box);
  p.flags[0].assign(p.tiles.count, 0);
  p.flags[1].assign(p.tiles.count, 0);
  info.cells = cells;
  for (size_t i = 0; i < cells; ++i) {  // k_plan_init
    const bool is_free = d2[i] >= r2;
    p.cost[i] = is_free ? PLAN_INF : PLAN_BLOCKED;
    info.free += is_free;
  }
  for (const revo_map_plan_seed& s : seeds) {  // k_plan_seed
    unsigned at = 0;
    const int cls = plan_seed_class(p.box, s, [&](unsigned c) { return p.cost[c]; }, &at);
    if (cls == PLAN_SEED_USED) {
      p.cost[at] = std::min(p.cost[at], s.cost0);
      p.flags[0][plan_tile_of_cell(p.tiles, (unsigned)(s.cell[0] - p.box.lo[0]), (unsigned)(s.cell[1] - p.box.lo[1]), (unsigned)(s.cell[2] - p.box.lo[2]))] = 1;
      ++info.seeds_used;
    } else if (cls == PLAN_SEED_OUTSIDE) {
      ++info.seeds_outside;
    } else {
      ++info.seeds_blocked;
    }
  }
  uint32_t done = 0;
  const int rc = plan_round_loop(limit, PLAN_GROUP, [&](uint32_t k, uint32_t* marked) { return p.run(k, marked); }, &done);
  if (rc == REVO_OK)
    for (uint32_t& c : p.cost) {  // k_plan_finish
      if (c < PLAN_INF) { ++info.reachable; info.max_cost = std::max<uint64_t>(info.max_cost, c); }
      else c = REVO_PLAN_NONE;
    }
  f = fopen(out, "wb");
  if (!f) return 2;
  const int32_t rc32 = rc;
  fwrite(&rc32, 4, 1, f); fwrite(&done, 4, 1, f); fwrite(&info, sizeof(info), 1, f); fwrite(p.cost.data(), 4, cells, f);
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "rules")) return rules();
  if (argc == 4 && !strcmp(argv[1], "plan")) return plan(argv[2], argv[3]);
  return 2;
}
