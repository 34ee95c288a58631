// revo_seen_host.h -- the arithmetic of the seen volume (include/revo_hip.h) that host and device code share, each
// rule written once: the parameters a call runs with, a cell's point, the update of a cell's byte, and what a byte says about a
// cell (free, known, frontier).  Plain C++: revo_map_seen.hip and revo_map_field.hip compile it for both sides,
// tests/cpp/seen_host.cpp for the host alone.  Internal.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/revo_hip.h"

#if defined(__HIPCC__)
#define SEEN_HD __host__ __device__ inline
#else
#define SEEN_HD inline
#endif

#define SEEN_VOTES 0x7Fu    // the low seven bits: free votes, saturating
#define SEEN_SURFACE 0x80u  // bit 7: a view measured a surface at the cell's centre

// The parameters a call runs with (NULL: radius 1, accumulate 0, margin = the voxel edge, 0), or why they are refused.
inline const char* seen_params_check(const revo_map_observe_params* prm, float voxel, revo_map_observe_params* out) {
  *out = prm ? *prm : revo_map_observe_params{1, 0u, voxel, 0.0f};
  if (out->radius < 0 || out->radius > 3) return "radius must be 0 .. 3";
  if (out->accumulate > 1u) return "accumulate must be 0 or 1";
  if (!std::isfinite(out->margin) || !(out->margin >= 0.0f)) return "margin must be finite and >= 0";
  if (!std::isfinite(out->margin_rel) || !(out->margin_rel >= 0.0f)) return "margin_rel must be finite and >= 0";
  return nullptr;
}

// One coordinate of the centre of the cell a of a box that starts at the voxel index lo: |lo + a| <= 2^20, so the sum is exact
// and the product is the one rounding.
SEEN_HD float seen_centre(int lo, int a, float voxel) { return ((float)(lo + a) + 0.5f) * voxel; }

// A cell's byte after a call: in the byte before (0 for a call that does not accumulate), f the views of the call in which the
// centre is FREE (<= 64), s whether it is CONFIRMED in any.
SEEN_HD uint8_t seen_byte(uint8_t in, unsigned f, unsigned s) {
  const unsigned votes = (in & SEEN_VOTES) + f;
  return (uint8_t)(((in | (s << 7)) & SEEN_SURFACE) | (votes < SEEN_VOTES ? votes : SEEN_VOTES));
}

// What a byte says.  min_views 0 counts as 1.  A solid cell is known whatever its byte; these are the rules for the others.
SEEN_HD bool seen_is_free(uint8_t b, uint32_t min_views) { return (b & SEEN_VOTES) >= (min_views < 1u ? 1u : min_views); }
SEEN_HD bool seen_is_known(uint8_t b, uint32_t min_views) { return seen_is_free(b, min_views) || (b & SEEN_SURFACE) != 0; }
SEEN_HD bool seen_is_unknown(bool solid, uint8_t b, uint32_t min_views) { return !solid && !seen_is_known(b, min_views); }
// A frontier cell: not solid, free, and `unknown_neighbours` of its (at most six) face neighbours inside the box are unknown.
SEEN_HD bool seen_is_frontier(bool solid, uint8_t b, uint32_t min_views, int unknown_neighbours) {
  return !solid && seen_is_free(b, min_views) && unknown_neighbours > 0;
}
