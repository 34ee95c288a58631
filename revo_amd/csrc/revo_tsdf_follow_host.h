// revo_tsdf_follow_host.h -- the rules of moving the surface volume's box (include/revo_hip.h) that host and device code
// share, each written once: the staying sub-box of a shift, a leaving cell's rank among the leaving cells and the cell of a rank
// (both closed-form: the leaving set is the box minus the staying sub-box), when a cell is EMPTY and when a cell FITS.
// Plain C++: revo_map_tsdf_follow.hip compiles it for both sides, tests/cpp/follow_host.cpp for the host alone.  Internal.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/revo_hip.h"

#if defined(__HIPCC__)
#define FOLLOW_HD __host__ __device__ inline
#else
#define FOLLOW_HD inline
#endif

#define FOLLOW_W_MAX (1u << 20)           // a cell's weight and colour weight at most (revo_map_tsdf_fuse's)
#define FOLLOW_SUM_MAX (1ll << 30)        // |sum| at most: 2^20 updates of at most 1024
#define FOLLOW_COLOR_MAX (255ll << 20)    // a colour sum at most: 2^20 updates of at most 255

// A shift of the box (lo, n) by delta: the destination cell c' holds the source cell c' + delta.  The staying sub-box in SOURCE
// cells is [s_lo, s_lo + s_n) per axis; in destination cells it starts at s_lo - delta.  No staying cell: s_lo = s_n = 0.
struct FollowShift {
  int n[3], d[3];
  int s_lo[3], s_n[3];
};
FOLLOW_HD FollowShift follow_shift(const int32_t n[3], const int32_t delta[3]) {
  FollowShift f{};
  bool any = true;
  for (int k = 0; k < 3; ++k) {
    f.n[k] = n[k];
    f.d[k] = delta[k] > n[k] ? n[k] : (delta[k] < -n[k] ? -n[k] : delta[k]);  // beyond the box nothing stays: d keeps x + d an int
    f.s_lo[k] = f.d[k] > 0 ? f.d[k] : 0;
    f.s_n[k] = n[k] - (f.d[k] < 0 ? -f.d[k] : f.d[k]);
    any = any && f.s_n[k] > 0;
  }
  if (!any)
    for (int k = 0; k < 3; ++k) f.s_lo[k] = f.s_n[k] = 0;
  return f;
}
FOLLOW_HD uint64_t follow_cells(const FollowShift& f) { return (uint64_t)f.n[0] * (uint64_t)f.n[1] * (uint64_t)f.n[2]; }
FOLLOW_HD uint64_t follow_staying(const FollowShift& f) { return (uint64_t)f.s_n[0] * (uint64_t)f.s_n[1] * (uint64_t)f.s_n[2]; }
FOLLOW_HD uint64_t follow_leaving(const FollowShift& f) { return follow_cells(f) - follow_staying(f); }

// whether the source cell (x, y, z) stays
FOLLOW_HD bool follow_stays(const FollowShift& f, int x, int y, int z) {
  return (unsigned)(x - f.s_lo[0]) < (unsigned)f.s_n[0] && (unsigned)(y - f.s_lo[1]) < (unsigned)f.s_n[1] &&
         (unsigned)(z - f.s_lo[2]) < (unsigned)f.s_n[2];
}
// whether the destination cell (x, y, z) receives a source cell (otherwise it is entering)
FOLLOW_HD bool follow_receives(const FollowShift& f, int x, int y, int z) { return follow_stays(f, x + f.d[0], y + f.d[1], z + f.d[2]); }

FOLLOW_HD long long follow_clamp(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// The staying cells whose place (x * n1 + y) * n2 + z is smaller than the place of (x, y, z): whole staying planes before x, and in
// x's plane, when it holds staying cells, whole staying lines before y and in y's line, when it holds some, the staying cells before z.
FOLLOW_HD uint64_t follow_staying_before(const FollowShift& f, int x, int y, int z) {
  const long long ax = follow_clamp((long long)x - f.s_lo[0], f.s_n[0]);
  uint64_t c = (uint64_t)ax * (uint64_t)f.s_n[1] * (uint64_t)f.s_n[2];
  if ((unsigned)(x - f.s_lo[0]) < (unsigned)f.s_n[0]) {
    const long long ay = follow_clamp((long long)y - f.s_lo[1], f.s_n[1]);
    c += (uint64_t)ay * (uint64_t)f.s_n[2];
    if ((unsigned)(y - f.s_lo[1]) < (unsigned)f.s_n[1]) c += (uint64_t)follow_clamp((long long)z - f.s_lo[2], f.s_n[2]);
  }
  return c;
}
// The rank of the leaving source cell (x, y, z) among the leaving cells in place order: its place minus the staying cells before it.
FOLLOW_HD uint64_t follow_leaving_rank(const FollowShift& f, int x, int y, int z) {
  return ((uint64_t)x * (uint64_t)f.n[1] + (uint64_t)y) * (uint64_t)f.n[2] + (uint64_t)z - follow_staying_before(f, x, y, z);
}
// The inverse: the place of the leaving cell of rank r < follow_leaving(f).  Whole planes before the staying planes; then per staying
// plane the whole lines before the staying lines, per staying line the cells before and behind the staying run, the whole lines
// behind; then whole planes.
FOLLOW_HD uint64_t follow_leaving_place(const FollowShift& f, uint64_t r) {
  const uint64_t n2 = (uint64_t)f.n[2], plane = (uint64_t)f.n[1] * n2;
  const uint64_t before = (uint64_t)f.s_lo[0] * plane;
  if (r < before) return r;
  r -= before;
  const uint64_t lp = plane - (uint64_t)f.s_n[1] * (uint64_t)f.s_n[2];  // leaving cells of a staying plane
  const uint64_t mid = (uint64_t)f.s_n[0] * lp;
  if (r >= mid) return (uint64_t)(f.s_lo[0] + f.s_n[0]) * plane + (r - mid);
  const uint64_t xi = r / lp;
  uint64_t q = r - xi * lp;
  const uint64_t base = ((uint64_t)f.s_lo[0] + xi) * plane;
  const uint64_t lines_before = (uint64_t)f.s_lo[1] * n2;
  if (q < lines_before) return base + q;
  q -= lines_before;
  const uint64_t lr = n2 - (uint64_t)f.s_n[2];  // leaving cells of a staying line
  const uint64_t lmid = (uint64_t)f.s_n[1] * lr;
  if (q >= lmid) return base + (uint64_t)(f.s_lo[1] + f.s_n[1]) * n2 + (q - lmid);
  const uint64_t yi = q / lr, zz = q - yi * lr;
  return base + ((uint64_t)f.s_lo[1] + yi) * n2 + (zz < (uint64_t)f.s_lo[2] ? zz : zz + (uint64_t)f.s_n[2]);
}

// A cell is EMPTY when every byte of its TSDF cell is zero and, with a colour volume, every byte of its colour cell too.
FOLLOW_HD bool follow_empty(int32_t sum, uint32_t weight, uint32_t sb, uint32_t sg, uint32_t sr, uint32_t cw) {
  return ((uint32_t)sum | weight | sb | sg | sr | cw) == 0u;
}
// A cell FITS when the sums a fuse can reach hold it, decided in 64 bits: what revo_map_tsdf_refill asks of every cell it leaves.
FOLLOW_HD bool follow_fits(int64_t sum, uint64_t weight, uint64_t sb, uint64_t sg, uint64_t sr, uint64_t cw) {
  return weight <= (uint64_t)FOLLOW_W_MAX && sum <= FOLLOW_SUM_MAX && sum >= -FOLLOW_SUM_MAX && cw <= (uint64_t)FOLLOW_W_MAX &&
         sb <= (uint64_t)FOLLOW_COLOR_MAX && sg <= (uint64_t)FOLLOW_COLOR_MAX && sr <= (uint64_t)FOLLOW_COLOR_MAX;
}

// The packed key of a voxel index (map_key of revo_map_impl.h: 21 bits per axis biased by 2^20, x highest) and back.
FOLLOW_HD uint64_t follow_key(int kx, int ky, int kz) {
  return ((uint64_t)(kx + (1 << 20)) << 42) | ((uint64_t)(ky + (1 << 20)) << 21) | (uint64_t)(kz + (1 << 20));
}
FOLLOW_HD void follow_key_axes(uint64_t key, int* kx, int* ky, int* kz) {
  *kx = (int)((key >> 42) & 0x1fffffu) - (1 << 20);
  *ky = (int)((key >> 21) & 0x1fffffu) - (1 << 20);
  *kz = (int)(key & 0x1fffffu) - (1 << 20);
}
