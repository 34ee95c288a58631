// revo_gain_host.h -- the arithmetic of revo_map_view_gain (include/revo_hip.h) that host and device code share, each
// rule written once: the parameters a call runs with, a pose's descriptor (the rays' origin and rotation and the world ->
// camera transform exactly as revo_map_raycast and revo_map_carve_eval form them, or "this pose breaks the rules"), and the
// cull -- the range of cells of the box outside which every centre is OUTSIDE the pose's view.  Plain C++:
// revo_map_gain.hip compiles it for both sides, tests/cpp/gain_host.cpp for the host alone.  Internal.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "revo_ray_host.h"

#if defined(__HIPCC__)
#define GAIN_HD __host__ __device__ inline
#else
#define GAIN_HD inline
#endif

#define GAIN_MAX_POSES ((size_t)4096)
#define GAIN_CHUNK 64  // poses of a launch: revo_map_raycast's views of a call

// The parameters a call runs with (NULL: radius 1, min_views 1, margin = the voxel edge, 0, no miss depth, 4096 steps), or why
// they are refused.  zmin, zmax: the checked camera's depth range.  min_views 0 counts as 1.
inline const char* gain_params_check(const revo_map_gain_params* prm, float voxel, float zmin, float zmax, revo_map_gain_params* out) {
  *out = prm ? *prm : revo_map_gain_params{1, 1u, voxel, 0.0f, 0.0f, RAY_DEFAULT_STEPS, {0u, 0u}};
  if (out->reserved[0] | out->reserved[1]) return "the reserved words of the parameters must be 0";
  if (out->radius < 0 || out->radius > 3) return "radius must be 0 .. 3";
  if (!std::isfinite(out->margin) || !(out->margin >= 0.0f)) return "margin must be finite and >= 0";
  if (!std::isfinite(out->margin_rel) || !(out->margin_rel >= 0.0f)) return "margin_rel must be finite and >= 0";
  if (out->miss_depth != 0.0f && !(out->miss_depth > zmin && out->miss_depth < zmax)) return "miss_depth must be 0 or inside (zmin, zmax)";
  if (out->max_steps < 1 || out->max_steps > RAY_MAX_STEPS) return "max_steps must be 1 .. 2^20";
  if (out->min_views < 1) out->min_views = 1;
  return nullptr;
}

// pose_is_finite and pose_is_orthogonal of revo_pose_host.h, for both sides: the same float32 operations in the same order.
GAIN_HD bool gain_pose_ok(const float* T) {
  for (int i = 0; i < 16; ++i)
    if (!(fabsf(T[i]) <= 3.402823466e38f)) return false;  // NaN and inf fail
  float n2 = 0.0f;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      float v = T[r] * T[c] + T[4 + r] * T[4 + c] + T[8 + r] * T[8 + c];
      v -= (r == c) ? 1.0f : 0.0f;
      n2 += v * v;
    }
  const float det = T[0] * (T[5] * T[10] - T[9] * T[6]) - T[4] * (T[1] * T[10] - T[9] * T[2]) + T[8] * (T[1] * T[6] - T[5] * T[2]);
  return sqrtf(n2) < 1e-5f && det > 0.0f;
}

// A pose's descriptor from the checked camera `cam` (its pose fields are not read): ray_view_check's and carve_view_check's
// arithmetic on T.  A pose that breaks the rules gets an empty image (w = h = 0: no ray, no cell inside).
GAIN_HD bool gain_pose_view(const RayView& cam, const float* T, RayView* out) {
  *out = cam;
  if (!gain_pose_ok(T)) { out->w = 0; out->h = 0; return false; }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) { out->R[3 * r + c] = T[4 * c + r]; out->Rc[3 * r + c] = T[4 * r + c]; }
    out->o[r] = T[12 + r];
    out->tc[r] = -(((out->Rc[3 * r] * T[12]) + (out->Rc[3 * r + 1] * T[13])) + (out->Rc[3 * r + 2] * T[14]));
  }
  return true;
}

// The cull of DESIGN 25: cells lo[k] .. lo[k] + n[k] - 1 per axis, relative to the box (n = 0: none).  Every cell of the box
// whose centre's class in the view is not OUTSIDE lies in the range; the proof is DESIGN 25's.  In short: such a centre's
// computed camera point lies in the hull of the camera centre and the four corners at zmax of the pixel rectangle widened by
// radius + 1; that hull goes to the world through R and o in double; `pad` bounds what float32 rounding and the 1e-5 the pose
// rules leave the rotation can move a point by; the range is the hull's box grown by pad, floored / ceiled, and by one cell.
struct GainRange { int lo[3], n[3]; };
GAIN_HD GainRange gain_cull(const RayView& v, int radius, const revo_map_df_box& box, float voxel) {
  GainRange g;
  for (int k = 0; k < 3; ++k) { g.lo[k] = 0; g.n[k] = 0; }
  if (v.w < 1 || v.h < 1) return g;
  const double grow = (double)(radius + 1);
  const double u0 = -grow, u1 = (double)(v.w - 1) + grow, v0 = -grow, v1 = (double)(v.h - 1) + grow;
  const double zf = (double)v.zmax;
  const double cx[2] = {(u0 - (double)v.cx) / (double)v.fx * zf, (u1 - (double)v.cx) / (double)v.fx * zf};
  const double cy[2] = {(v0 - (double)v.cy) / (double)v.fy * zf, (v1 - (double)v.cy) / (double)v.fy * zf};
  double corner = fabs(zf);  // the largest camera coordinate of the hull
  for (int i = 0; i < 2; ++i) { corner = fmax(corner, fabs(cx[i])); corner = fmax(corner, fabs(cy[i])); }
  double scale = corner;
  for (int k = 0; k < 3; ++k) {
    scale += fabs((double)v.o[k]) + fabs((double)v.tc[k]);
    const double a = fabs((double)box.lo[k]), b = fabs((double)box.lo[k] + (double)box.n[k]);
    scale += fmax(a, b) * (double)voxel;
  }
  const double pad = scale * 0x1p-14;
  for (int k = 0; k < 3; ++k) {
    double mn = (double)v.o[k], mx = mn;
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j) {
        const double w = ((double)v.R[3 * k] * cx[i] + (double)v.R[3 * k + 1] * cy[j]) + (double)v.R[3 * k + 2] * zf + (double)v.o[k];
        mn = fmin(mn, w); mx = fmax(mx, w);
      }
    double first = floor((mn - pad) / (double)voxel) - 1.0, last = ceil((mx + pad) / (double)voxel) + 1.0;
    const double b0 = (double)box.lo[k], b1 = b0 + (double)box.n[k] - 1.0;
    if (!(first == first) || !(last == last)) { first = b0; last = b1; }  // NaN: the whole axis
    first = fmax(first, b0); last = fmin(last, b1);
    if (!(first <= last)) { for (int q = 0; q < 3; ++q) g.n[q] = 0; return g; }
    g.lo[k] = (int)(first - b0);
    g.n[k] = (int)(last - first) + 1;
  }
  return g;
}
