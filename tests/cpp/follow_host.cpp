// follow_host.cpp -- revo_tsdf_follow_host.h's rules for a box that follows the camera on the host, checked against
// brute force: for small boxes and every shift up to one past the box on every axis, the staying sub-box, every leaving cell's rank
// and the cell of every rank; EMPTY; FITS at its four limits and one past each; the key and its axes.  Prints one line per group
// and "ok"; tests/test_map_follow_cpu.py runs it.
// Build: c++ -std=c++17 follow_host.cpp (with host sanitizers where the toolchain has them).
#include <cstdio>
#include <vector>

#include "../../revo_amd/csrc/revo_tsdf_follow_host.h"

static int failures = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      if (++failures < 20) printf("FAILED line %d: %s\n", __LINE__, #c); \
    }                                                         \
  } while (0)

static void check_box(const int32_t n[3], const int32_t d[3]) {
  const FollowShift f = follow_shift(n, d);
  uint64_t staying = 0, rank = 0;
  std::vector<uint64_t> places;
  for (int x = 0; x < n[0]; ++x)
    for (int y = 0; y < n[1]; ++y)
      for (int z = 0; z < n[2]; ++z) {
        // brute force: the source cell stays when c - delta is a destination cell
        const long long tx = (long long)x - d[0], ty = (long long)y - d[1], tz = (long long)z - d[2];
        const bool stays = tx >= 0 && tx < n[0] && ty >= 0 && ty < n[1] && tz >= 0 && tz < n[2];
        CHECK(follow_stays(f, x, y, z) == stays);
        CHECK(follow_staying_before(f, x, y, z) == staying);
        const uint64_t place = ((uint64_t)x * n[1] + y) * n[2] + z;
        if (stays) {
          ++staying;
        } else {
          CHECK(follow_leaving_rank(f, x, y, z) == rank);
          CHECK(follow_leaving_place(f, rank) == place);
          ++rank;
        }
        // the destination cell (x, y, z) receives the source cell c + delta when that is a source cell
        const long long sx = (long long)x + d[0], sy = (long long)y + d[1], sz = (long long)z + d[2];
        CHECK(follow_receives(f, x, y, z) == (sx >= 0 && sx < n[0] && sy >= 0 && sy < n[1] && sz >= 0 && sz < n[2]));
      }
  CHECK(follow_staying(f) == staying);
  CHECK(follow_leaving(f) == rank);
  CHECK(follow_cells(f) == staying + rank);
  for (int k = 0; k < 3; ++k) {  // the sub-box itself
    CHECK(f.s_n[k] >= 0 && f.s_lo[k] >= 0 && f.s_lo[k] + f.s_n[k] <= n[k]);
    if (staying) CHECK(f.s_lo[k] == (d[k] > 0 ? d[k] : 0) && f.s_n[k] == n[k] - (d[k] < 0 ? -d[k] : d[k]));
    else CHECK(f.s_n[k] == 0);
  }
}

int main() {
  const int32_t boxes[][3] = {{1, 1, 1}, {3, 5, 7}, {3, 3, 4}, {2, 2, 9}, {4, 1, 5}, {1, 6, 2}};
  unsigned shifts = 0;
  for (const auto& n : boxes)
    for (int dx = -n[0] - 1; dx <= n[0] + 1; ++dx)
      for (int dy = -n[1] - 1; dy <= n[1] + 1; ++dy)
        for (int dz = -n[2] - 1; dz <= n[2] + 1; ++dz) {
          const int32_t d[3] = {dx, dy, dz};
          check_box(n, d);
          ++shifts;
        }
  const int32_t n357[3] = {3, 5, 7}, far[3] = {INT32_MIN, INT32_MAX, 1 << 21};  // far beyond the box: nothing stays, nothing overflows
  check_box(n357, far);
  printf("shifts %u\n", shifts + 1);

  CHECK(follow_empty(0, 0, 0, 0, 0, 0));
  CHECK(!follow_empty(-1, 0, 0, 0, 0, 0) && !follow_empty(0, 1, 0, 0, 0, 0) && !follow_empty(0, 0, 1, 0, 0, 0));
  CHECK(!follow_empty(0, 0, 0, 1, 0, 0) && !follow_empty(0, 0, 0, 0, 1, 0) && !follow_empty(0, 0, 0, 0, 0, 1));
  CHECK(!follow_empty(INT32_MIN, 0, 0, 0, 0, 0));
  printf("empty\n");

  const int64_t S = 1ll << 30;
  const uint64_t W = 1ull << 20, K = 255ull << 20;
  CHECK(follow_fits(S, W, K, K, K, W) && follow_fits(-S, W, K, K, K, W) && follow_fits(0, 0, 0, 0, 0, 0));
  CHECK(!follow_fits(S + 1, W, K, K, K, W) && !follow_fits(-S - 1, W, K, K, K, W));  // |sum| one past
  CHECK(!follow_fits(S, W + 1, K, K, K, W));                                         // weight one past
  CHECK(!follow_fits(S, W, K, K, K, W + 1));                                         // colour weight one past
  CHECK(!follow_fits(S, W, K + 1, K, K, W) && !follow_fits(S, W, K, K + 1, K, W) && !follow_fits(S, W, K, K, K + 1, W));  // each colour sum
  CHECK(!follow_fits(0, 1ull << 32, 0, 0, 0, 0) && !follow_fits(0, 0, 1ull << 32, 0, 0, 0));  // what 32 bits would wrap to 0
  printf("fits\n");

  const int rim[] = {-(1 << 20), -1, 0, 1, (1 << 20) - 1};
  uint64_t prev = 0;
  bool first = true;
  for (int x : rim)
    for (int y : rim)
      for (int z : rim) {
        const uint64_t k = follow_key(x, y, z);
        int a, b, c;
        follow_key_axes(k, &a, &b, &c);
        CHECK(a == x && b == y && c == z && !(k >> 63));
        CHECK(first || k > prev);  // ascending keys are ascending places
        prev = k;
        first = false;
      }
  CHECK(follow_key(-(1 << 20), -(1 << 20), -(1 << 20)) == 0);
  printf("keys\n");
  if (failures) printf("FAILED %d\n", failures);
  else printf("ok\n");
  return failures ? 1 : 0;
}
