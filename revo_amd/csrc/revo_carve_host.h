// revo_carve_host.h -- the host arithmetic of revo_map_carve_eval / revo_map_carve (include/revo_hip.h): the rules a
// view and the parameters must meet before anything is enqueued, the world -> camera transform exactly as revo_map_render
// forms it, and the canonical (ascending key) order of the host output.  Plain C++ with no device code: revo_map.hip runs it
// over the caller's views and k_map_carve's records, tests/cpp/carve_host.cpp over views and records a test wrote.  Internal.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "revo_pose_host.h"

struct CarveCam { float fx, fy, cx, cy, zmin, zmax; };  // a context's level-0 camera and depth range
struct CarveView {  // one checked view as the kernel takes it (the depth pointer is the caller's business)
  float Rc[9], tc[3];  // world -> camera, Rc row-major
  float fx, fy, cx, cy, zmin, zmax;
  int w, h;
};

// Why a view is refused, or NULL.  v->kf / v->depth: exactly one; a pyramid view takes the context's camera and size (ctx_w,
// ctx_h), a raw one its own size and either six zeros (the context's camera) or its own intrinsics.
inline const char* carve_view_check(const revo_map_carve_view* v, const CarveCam& ctx, int ctx_w, int ctx_h, CarveView* out) {
  if ((v->kf != nullptr) == (v->depth != nullptr)) return "exactly one of kf and depth must be given";
  CarveCam k = ctx;
  int w = ctx_w, h = ctx_h;
  if (!v->kf) {
    w = v->width; h = v->height;
    if (w < 1 || w > 2048 || h < 1 || h > 2048) return "width and height must be 1 .. 2048";
    const float f[6] = {v->fx, v->fy, v->cx, v->cy, v->zmin, v->zmax};
    bool zero = true, finite = true;
    for (float x : f) { zero = zero && x == 0.0f; finite = finite && std::isfinite(x); }
    if (!zero) {
      if (!finite) return "intrinsics and depth range must be finite";
      if (!(v->fx > 0.0f) || !(v->fy > 0.0f)) return "fx and fy must be > 0";
      k = CarveCam{v->fx, v->fy, v->cx, v->cy, v->zmin, v->zmax};
    }
  }
  if (!(k.zmin >= 0.0f) || !(k.zmin < k.zmax)) return "the depth range needs 0 <= zmin < zmax";
  const float* T = v->T_w_c;
  if (!pose_is_finite(T)) return "T_w_c is not finite";
  if (!pose_is_orthogonal(T)) return "the rotation of T_w_c is not orthogonal";
  // column-major: R(r, c) = T[4 c + r], so Rc(r, c) = R(c, r) = T[4 r + c] (revo_map_render)
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) out->Rc[3 * r + c] = T[4 * r + c];
    out->tc[r] = -(((out->Rc[3 * r] * T[12]) + (out->Rc[3 * r + 1] * T[13])) + (out->Rc[3 * r + 2] * T[14]));
  }
  out->fx = k.fx; out->fy = k.fy; out->cx = k.cx; out->cy = k.cy; out->zmin = k.zmin; out->zmax = k.zmax;
  out->w = w; out->h = h;
  return nullptr;
}

// The parameters a call runs with (NULL: radius 1, min_views 1, min_count 1, no max_count, margin = the voxel edge, 0), or why
// they are refused.  min_views and min_count 0 count as 1.
inline const char* carve_params_check(const revo_map_carve_params* prm, float voxel, revo_map_carve_params* out) {
  *out = prm ? *prm : revo_map_carve_params{1, 1u, 1u, 0u, voxel, 0.0f};
  if (out->radius < 0 || out->radius > 3) return "radius must be 0 .. 3";
  if (!std::isfinite(out->margin) || !(out->margin >= 0.0f)) return "margin must be finite and >= 0";
  if (!std::isfinite(out->margin_rel) || !(out->margin_rel >= 0.0f)) return "margin_rel must be finite and >= 0";
  if (out->min_views < 1) out->min_views = 1;
  if (out->min_count < 1) out->min_count = 1;
  return nullptr;
}

// The host output: the carved voxels' records in ascending key order (a voxel is carved once, so no two keys are equal and
// pose_canonicalise only sorts).
inline size_t carve_canonicalise(revo_map_voxel_raw* rec, size_t n) { return pose_canonicalise(rec, n); }
