// revo_pose_host.h -- the host arithmetic of revo_map_pose_raw / revo_map_merge_posed / revo_map_subtract_posed (include/revo_hip.h,
// DESIGN 18): the pose checks made before any table is touched, and the canonical form of posed records (ascending keys, equal
// keys summed).  Plain C++ with no device code: revo_map.hip runs it over k_map_pose's records, tests/cpp/pose_host.cpp over
// records a test wrote.  Internal.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/revo_hip.h"

// is_orthogonal of revo_track_dev.h (the rule of revo_map_align_eval) on the rotation of a column-major 4x4: float32, every
// operation rounded on its own (the library is built with -ffp-contract=off).
inline bool pose_is_orthogonal(const float* T) {
  const float R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};  // R[3 c + r]
  float n2 = 0.0f;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      float v = R[r] * R[c] + R[3 + r] * R[3 + c] + R[6 + r] * R[6 + c];
      v -= (r == c) ? 1.0f : 0.0f;
      n2 += v * v;
    }
  const float det = R[0] * (R[4] * R[8] - R[7] * R[5]) - R[3] * (R[1] * R[8] - R[7] * R[2]) + R[6] * (R[1] * R[5] - R[4] * R[2]);
  return std::sqrt(n2) < 1e-5f && det > 0.0f;
}
inline bool pose_is_finite(const float* T) {
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(T[i])) return false;
  return true;
}

// Records in any order, keys may repeat -> ascending keys, one record per key holding the integer sums of its records (the
// sums wrap as the device's 64-bit atomics do).  In place; returns the number of records left.
inline size_t pose_canonicalise(revo_map_voxel_raw* rec, size_t n) {
  std::sort(rec, rec + n, [](const revo_map_voxel_raw& a, const revo_map_voxel_raw& b) { return a.key < b.key; });
  size_t m = 0;
  for (size_t i = 0; i < n; ++i) {
    if (m && rec[m - 1].key == rec[i].key) {
      revo_map_voxel_raw& o = rec[m - 1];
      o.count += rec[i].count;
      for (int k = 0; k < 3; ++k) {
        o.sum_q[k] = (int64_t)((uint64_t)o.sum_q[k] + (uint64_t)rec[i].sum_q[k]);
        o.sum_bgr[k] += rec[i].sum_bgr[k];
      }
    } else {
      if (m != i) rec[m] = rec[i];
      ++m;
    }
  }
  return m;
}
