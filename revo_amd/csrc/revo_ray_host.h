// revo_ray_host.h -- the host arithmetic of revo_map_raycast / revo_map_cast_rays (include/revo_hip.h): the rules the
// parameters and a view must meet before anything is enqueued, and a view's ray set-up -- the origin o and rotation R its pixels'
// rays are formed from, and the world -> camera transform Rc, tc exactly as revo_map_render forms it, which decides whether a
// voxel is solid to the view.  Plain C++ with no device code: revo_map.hip runs it over the caller's views,
// tests/cpp/ray_host.cpp over views a test wrote.  Internal.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "revo_carve_host.h"

#define RAY_MAX_VIEWS 64
#define RAY_MAX_RAYS ((size_t)1 << 24)
#define RAY_MAX_STEPS (1u << 20)
#define RAY_DEFAULT_STEPS 4096u

struct RayView {  // one checked view as the kernel takes it (the output pointers are the caller's business)
  float o[3], R[9];    // camera -> world: the rays' origin and rotation, R row-major
  float Rc[9], tc[3];  // world -> camera, Rc row-major
  float fx, fy, cx, cy, zmin, zmax;
  int w, h;
};

// The cells a ray may examine (NULL: 4096), or why the parameters are refused.
inline const char* ray_params_check(const revo_map_ray_params* prm, uint32_t* max_steps) {
  *max_steps = prm ? prm->max_steps : RAY_DEFAULT_STEPS;
  if (prm && (prm->reserved[0] | prm->reserved[1] | prm->reserved[2])) return "the reserved words of the parameters must be 0";
  if (*max_steps < 1 || *max_steps > RAY_MAX_STEPS) return "max_steps must be 1 .. 2^20";
  return nullptr;
}

// Why a view is refused, or NULL: revo_map_render's rules (splat_max is not read).  All six intrinsics zero: the context's.
inline const char* ray_view_check(const revo_map_view* v, const CarveCam& ctx, RayView* out) {
  if (v->width < 1 || v->width > 2048 || v->height < 1 || v->height > 2048) return "width and height must be 1 .. 2048";
  const float* T = v->T_w_c;
  if (!pose_is_finite(T)) return "T_w_c is not finite";
  CarveCam k = ctx;
  const float f[6] = {v->fx, v->fy, v->cx, v->cy, v->zmin, v->zmax};
  bool zero = true, finite = true;
  for (float x : f) { zero = zero && x == 0.0f; finite = finite && std::isfinite(x); }
  if (!zero) {
    if (!finite) return "intrinsics and depth range must be finite";
    if (!(v->fx > 0.0f) || !(v->fy > 0.0f)) return "fx and fy must be > 0";
    k = CarveCam{v->fx, v->fy, v->cx, v->cy, v->zmin, v->zmax};
  }
  if (!(k.zmin >= 0.0f) || !(k.zmin < k.zmax)) return "the depth range needs 0 <= zmin < zmax";
  // column-major: R(r, c) = T[4 c + r], so Rc(r, c) = R(c, r) = T[4 r + c] (revo_map_render)
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) { out->R[3 * r + c] = T[4 * c + r]; out->Rc[3 * r + c] = T[4 * r + c]; }
    out->o[r] = T[12 + r];
    out->tc[r] = -(((out->Rc[3 * r] * T[12]) + (out->Rc[3 * r + 1] * T[13])) + (out->Rc[3 * r + 2] * T[14]));
  }
  out->fx = k.fx; out->fy = k.fy; out->cx = k.cx; out->cy = k.cy; out->zmin = k.zmin; out->zmax = k.zmax;
  out->w = v->width; out->h = v->height;
  return nullptr;
}

// The one min_count (0 counts as 1) that every view of a call carries, or 0 when they differ.
inline uint32_t ray_views_min_count(const revo_map_view* views, int n) {
  const uint32_t mc = views[0].min_count < 1 ? 1u : views[0].min_count;
  for (int i = 1; i < n; ++i)
    if ((views[i].min_count < 1 ? 1u : views[i].min_count) != mc) return 0;
  return mc;
}
