// revo_tsdf_track_host.h -- the rules of revo_map_tsdf_track_eval (include/revo_hip.h) that host and device code share,
// each written once: the parameters a call runs with, the pixels a stride visits, a pixel's camera and world point, its residual
// and gradient from the field, the gate, and the 28 terms of an accepted pixel.  The place in the box, the interpolant and its
// gradient are revo_tsdf_ray_host.h's.  Plain C++: revo_map_tsdf_track.hip compiles it for both sides, tests/cpp/tsdf_track_host.cpp
// for the host alone.  Internal.
#pragma once
#include "revo_tsdf_ray_host.h"

#define TSDF_TRACK_MAX_POSES 4096
#define TSDF_TRACK_MAX_STRIDE 8u
enum { TSDF_TRACK_SKIPPED = 0, TSDF_TRACK_GATED = 1, TSDF_TRACK_ACCEPTED = 2 };

// The parameters a call runs with (NULL, and every zero: max_dist trunc / 2, stride 1, min_weight 1, centre 0), or why they are
// refused.  trunc is finite and > 0.
inline const char* tsdf_track_params_check(const revo_map_tsdf_track_params* prm, float trunc, revo_map_tsdf_track_params* out) {
  *out = prm ? *prm : revo_map_tsdf_track_params{0.0f, 0u, 0u, {0.0f, 0.0f, 0.0f}, {0u, 0u}};
  if (!std::isfinite(out->max_dist) || out->max_dist < 0.0f || out->max_dist > trunc) return "max_dist must be 0 (trunc / 2) or finite with 0 < max_dist <= trunc";
  if (out->stride > TSDF_TRACK_MAX_STRIDE) return "stride must be 0 (1) or 1 .. 8";
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(out->centre[i])) return "the centre is not finite";
  if (out->reserved[0] || out->reserved[1]) return "a reserved word of the parameters is not 0";
  if (out->max_dist == 0.0f) out->max_dist = trunc * 0.5f;
  if (out->stride < 1u) out->stride = 1u;
  if (out->min_weight < 1u) out->min_weight = 1u;
  return nullptr;
}

// The pixels a stride visits along an axis of n pixels: 0, stride, ... < n.
TSDF_HD int tsdf_track_lattice(int n, int stride) { return (n + stride - 1) / stride; }

// What every pixel of a call shares beside the volume (TsdfRayK: step, max_steps and the mask are not read).
struct TsdfTrackCam { float fx, fy, cx, cy, zmin, zmax; };
struct TsdfTrackK {
  TsdfRayK vol;
  TsdfTrackCam cam;
  float kq;        // trunc / 1024: metres per unit of the field
  float max_dist;
  float centre[3];
};
TSDF_HD float tsdf_track_kq(float trunc) { return tsdf_div(trunc, 1024.0f); }

// The carve rule on a depth: usable when finite and strictly inside the range.
TSDF_HD bool tsdf_track_depth_ok(float D, float zmin, float zmax) { return std::isfinite(D) && D > zmin && D < zmax; }

// Two cells that follow each other along z (adjacent 8-byte records) in one 16-byte read.
TSDF_HD void tsdf_track_pair(const revo_map_tsdf_cell* p, revo_map_tsdf_cell* c0, revo_map_tsdf_cell* c1) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned u4 __attribute__((ext_vector_type(4), aligned(8)));  // a cell is 8-byte aligned; global loads need no more
  const u4 q = *(const u4 __attribute__((address_space(1)))*)p;
  c0->sum = (int32_t)q.x; c0->weight = q.y; c1->sum = (int32_t)q.z; c1->weight = q.w;
#else
  *c0 = p[0]; *c1 = p[1];
#endif
}
// tsdf_ray_sample at a place, the eight cells read as four pairs.
TSDF_HD void tsdf_track_sample(const TsdfRayK& a, const TsdfRayPlace& p, TsdfRaySample* out) {
  out->valid = false; out->s = 0.0f; out->F = 0.0f; out->gx = 0.0f; out->gy = 0.0f; out->gz = 0.0f; out->ccell = 0u;
  if (!p.inbox) return;  // before any load: only a base with all eight cells inside the box is read
  const size_t nz = (size_t)a.box.n[2], nyz = (size_t)a.box.n[1] * nz;
  const revo_map_tsdf_cell* at = a.tsdf + ((size_t)p.bx * nyz + (size_t)p.by * nz + (size_t)p.bz);
  revo_map_tsdf_cell c000, c001, c010, c011, c100, c101, c110, c111;
  tsdf_track_pair(at, &c000, &c001);
  tsdf_track_pair(at + nz, &c010, &c011);
  tsdf_track_pair(at + nyz, &c100, &c101);
  tsdf_track_pair(at + nyz + nz, &c110, &c111);
  tsdf_ray_sample_cells(a, p, c000, c001, c010, c011, c100, c101, c110, c111, out);
}

// One pixel under one pose (R column-major, t) -> its class.  *e, g[3]: the residual and its gradient (from GATED on), pw[3]: the
// world point (always).  D is read by the caller: once per pixel.
TSDF_HD int tsdf_track_pixel(const TsdfTrackK& a, const float* R, const float* t, int x, int y, float D, float* pw, float* e, float* g) {
  pw[0] = 0.0f; pw[1] = 0.0f; pw[2] = 0.0f;
  if (!tsdf_track_depth_ok(D, a.cam.zmin, a.cam.zmax)) return TSDF_TRACK_SKIPPED;
  const float dcx = tsdf_div((float)x - a.cam.cx, a.cam.fx), dcy = tsdf_div((float)y - a.cam.cy, a.cam.fy);
  const float pcx = dcx * D, pcy = dcy * D, pcz = D;
  pw[0] = ((R[0] * pcx + R[3] * pcy) + R[6] * pcz) + t[0];
  pw[1] = ((R[1] * pcx + R[4] * pcy) + R[7] * pcz) + t[1];
  pw[2] = ((R[2] * pcx + R[5] * pcy) + R[8] * pcz) + t[2];
  TsdfRaySample s;
  tsdf_track_sample(a.vol, tsdf_ray_place_at(a.vol, pw[0], pw[1], pw[2]), &s);
  if (!s.valid) return TSDF_TRACK_SKIPPED;
  *e = s.F * a.kq;
  g[0] = tsdf_div(s.gx * a.kq, a.vol.voxel);
  g[1] = tsdf_div(s.gy * a.kq, a.vol.voxel);
  g[2] = tsdf_div(s.gz * a.kq, a.vol.voxel);
  return std::fabs(*e) <= a.max_dist ? TSDF_TRACK_ACCEPTED : TSDF_TRACK_GATED;
}

// The Jacobian row of an accepted pixel: J = (g, u x g), u = p' - centre.  Named scalars: two products and one subtraction each.
struct TsdfTrackJ { float j0, j1, j2, j3, j4, j5; };
TSDF_HD TsdfTrackJ tsdf_track_row(const TsdfTrackK& a, const float* pw, const float* g) {
  const float ux = pw[0] - a.centre[0], uy = pw[1] - a.centre[1], uz = pw[2] - a.centre[2];
  return TsdfTrackJ{g[0], g[1], g[2], uy * g[2] - uz * g[1], uz * g[0] - ux * g[2], ux * g[1] - uy * g[0]};
}
// The 28 terms in the record's order, each handed to f(slot, term): S[0..20] J_i*J_j (i <= j, row by row), S[21..26] J_i*e, S[27] e*e.
template <class Fn>
TSDF_HD void tsdf_track_terms(const TsdfTrackJ& J, float e, Fn&& f) {
  f(0, J.j0 * J.j0); f(1, J.j0 * J.j1); f(2, J.j0 * J.j2); f(3, J.j0 * J.j3); f(4, J.j0 * J.j4); f(5, J.j0 * J.j5);
  f(6, J.j1 * J.j1); f(7, J.j1 * J.j2); f(8, J.j1 * J.j3); f(9, J.j1 * J.j4); f(10, J.j1 * J.j5);
  f(11, J.j2 * J.j2); f(12, J.j2 * J.j3); f(13, J.j2 * J.j4); f(14, J.j2 * J.j5);
  f(15, J.j3 * J.j3); f(16, J.j3 * J.j4); f(17, J.j3 * J.j5);
  f(18, J.j4 * J.j4); f(19, J.j4 * J.j5);
  f(20, J.j5 * J.j5);
  f(21, J.j0 * e); f(22, J.j1 * e); f(23, J.j2 * e); f(24, J.j3 * e); f(25, J.j4 * e); f(26, J.j5 * e);
  f(27, e * e);
}
