// revo_tsdf_host.h -- the arithmetic of the TSDF volume and its mesh (include/revo_hip.h) that host and device code
// share, each rule written once: the parameters a call runs with, a view's update of a cell, what a cell says (valid, inside),
// the Kuhn tetrahedra of a cube, the cubes an edge belongs to, a tetrahedron's triangles and a vertex's place on its edge.
// DESIGN 27 added the colour update that goes with a TSDF update, the colour image a view needs, and a vertex's normal and colour.
// DESIGN 32 added the down-date of a cell and its FIT test (revo_map_tsdf_unfuse.hip, tests/cpp/tsdf_unfuse_host.cpp).
// Plain C++: revo_map_tsdf.hip compiles it for both sides, tests/cpp/tsdf_host.cpp and surface_host.cpp for the host alone.  Internal.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/revo_hip.h"

#if defined(__HIPCC__)
#define TSDF_HD __host__ __device__ inline
#else
#define TSDF_HD inline
#endif

#define TSDF_W_MAX (1u << 20)  // a cell with this weight takes no further update
#define TSDF_Q_ONE 1024        // the quantum of a FREE view: + trunc

// The parameters a call runs with (NULL: 4 x the voxel edge, accumulate 0), or why they are refused.
inline const char* tsdf_params_check(const revo_map_tsdf_params* prm, float voxel, revo_map_tsdf_params* out) {
  *out = prm ? *prm : revo_map_tsdf_params{4.0f * voxel, 0u, {0u, 0u}};
  if (!std::isfinite(out->trunc) || !(out->trunc > 0.0f)) return "trunc must be finite and > 0";
  if (out->accumulate > 1u) return "accumulate must be 0 or 1";
  if (out->reserved[0] || out->reserved[1]) return "a reserved word is not 0";
  return nullptr;
}

// The quantum of a view in which the cell's centre is CONFIRMED: dc the centre pixel's depth, z the centre's camera-space depth,
// |z - dc| <= trunc.  A difference, a quotient, a product and the rounding to the nearest integer (ties to even), each on its own.
TSDF_HD int32_t tsdf_quantum(float dc, float z, float trunc) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (int32_t)rintf(__fdiv_rn(dc - z, trunc) * 1024.0f);
#else
  const float d = dc - z;
  const float r = d / trunc;
  return (int32_t)std::nearbyint(r * 1024.0f);  // the default rounding mode: ties to even
#endif
}

// One update of a cell; returns 1 when it is dropped because the weight is full.
TSDF_HD unsigned tsdf_update(int32_t& sum, uint32_t& weight, int32_t q) {
  if (weight >= TSDF_W_MAX) return 1u;
  sum += q;
  weight += 1u;
  return 0u;
}

// The colour image that goes with a view (revo_map_tsdf_fuse_color): a pyramid view brings its own level-0 BGR plane,
// a raw view needs one.  Why the pair is refused, or NULL.
inline const char* tsdf_bgr_check(const revo_map_carve_view* v, const uint8_t* bgr) {
  if (v->kf && bgr) return "a pyramid view brings its own colour image: bgr must be NULL";
  if (!v->kf && !bgr) return "a raw view needs a colour image";
  return nullptr;
}

// The colour update that goes with one TSDF update of a cell: it takes place when the view's class is CONFIRMED and the TSDF
// update was not dropped (dropped: tsdf_update's result), so the colour weight never passes the TSDF weight.  px: the centre
// pixel's three bytes B, G, R.  Returns 1 when it took place.
TSDF_HD unsigned tsdf_color_update(uint32_t& sb, uint32_t& sg, uint32_t& sr, uint32_t& cw, bool confirmed, unsigned dropped, const uint8_t* px) {
  if (!confirmed || dropped) return 0u;
  sb += px[0];
  sg += px[1];
  sr += px[2];
  cw += 1u;
  return 1u;
}

// ---- views taken out again (revo_map_tsdf_unfuse): the down-date of a cell and the FIT test, one text for the
// kernel, the host restatement and tests/cpp/tsdf_unfuse_host.cpp ----
// The truncation distance an unfuse runs with (0: 4 x the voxel edge), or why it is refused.
inline const char* tsdf_unfuse_trunc(float trunc, float voxel, float* out) {
  *out = trunc == 0.0f ? 4.0f * voxel : trunc;
  if (!std::isfinite(*out) || !(*out > 0.0f)) return "trunc must be 0 (4 x the voxel edge) or finite and > 0";
  return nullptr;
}
// What the views of one call take from one cell: k updates, kc of them CONFIRMED, their quanta and their pixels' bytes.  At most
// 64 views: |q| <= 2^16 and every colour total is below 2^14.
struct TsdfDown {
  uint32_t k, kc;
  int32_t q;
  uint32_t b, g, r;
};
// One view's update of the cell joins the totals.  px: the centre pixel's three bytes B, G, R of a CONFIRMED update when there
// is a colour volume, else NULL.
TSDF_HD void tsdf_down_add(TsdfDown& d, bool confirmed, int32_t q, const uint8_t* px) {
  d.k += 1u;
  d.q += q;
  if (!confirmed) return;
  d.kc += 1u;
  if (px) { d.b += px[0]; d.g += px[1]; d.r += px[2]; }
}
// Whether a TSDF cell with d.k > 0 FITS: its weight is not full, no more views leave than came, and what is left is a state a
// fuse can reach (an emptied cell has sum 0).  64-bit integers throughout.
TSDF_HD bool tsdf_down_fits(int32_t sum, uint32_t weight, const TsdfDown& d) {
  if (weight >= TSDF_W_MAX) return false;
  const int64_t w = (int64_t)weight - (int64_t)d.k, s = (int64_t)sum - (int64_t)d.q;
  if (w < 0) return false;
  return (s < 0 ? -s : s) <= (int64_t)TSDF_Q_ONE * w;
}
// Whether the cell's colour cell FITS beside it: nothing goes below zero, the colour weight stays within the TSDF weight and
// every sum within 255 x the colour weight.
TSDF_HD bool tsdf_down_color_fits(uint32_t weight, uint32_t sb, uint32_t sg, uint32_t sr, uint32_t cw, const TsdfDown& d) {
  const int64_t w = (int64_t)weight - (int64_t)d.k, c = (int64_t)cw - (int64_t)d.kc;
  const int64_t b = (int64_t)sb - (int64_t)d.b, g = (int64_t)sg - (int64_t)d.g, r = (int64_t)sr - (int64_t)d.r;
  if (c < 0 || b < 0 || g < 0 || r < 0) return false;
  return c <= w && b <= 255 * c && g <= 255 * c && r <= 255 * c;
}
// The down-date of a cell that FITS.
TSDF_HD void tsdf_down_apply(int32_t& sum, uint32_t& weight, const TsdfDown& d) {
  sum -= d.q;
  weight -= d.k;
}
TSDF_HD void tsdf_down_color_apply(uint32_t& sb, uint32_t& sg, uint32_t& sr, uint32_t& cw, const TsdfDown& d) {
  sb -= d.b;
  sg -= d.g;
  sr -= d.r;
  cw -= d.kc;
}

// What a cell says.  min_weight 0 counts as 1.
TSDF_HD bool tsdf_valid(uint32_t weight, uint32_t min_weight) { return weight >= (min_weight < 1u ? 1u : min_weight); }
TSDF_HD bool tsdf_inside(int32_t sum, uint32_t weight, uint32_t min_weight) { return tsdf_valid(weight, min_weight) && sum < 0; }

// A cube's corners are numbered dx + 2 dy + 4 dz.  The tetrahedron k (the k-th permutation of (x, y, z) in lexicographic order)
// has the corners 0, e0, e0 | e1, 7: v1 and v2 packed as v1 | v2 << 4.
TSDF_HD unsigned tsdf_tetra_v12(int k) {
  return k == 0 ? 0x31u : k == 1 ? 0x51u : k == 2 ? 0x32u : k == 3 ? 0x62u : k == 4 ? 0x54u : 0x64u;
}
TSDF_HD unsigned tsdf_tetra_corner(int k, int i) {  // i: 0 .. 3
  return i == 0 ? 0u : i == 3 ? 7u : (tsdf_tetra_v12(k) >> (4 * (i - 1))) & 7u;
}
// The edge between two corners a, b of a tetrahedron (a's bits are among b's): it belongs to the cell of a and has the type
// (b ^ a) - 1.  Every pair of corners a within b is an edge of some tetrahedron of the cube, so the edge of type t at the cell e
// belongs to the cubes e - o for the corners o that share no bit with t + 1: four cubes for an axis edge, two for a face
// diagonal, one for the body diagonal.
TSDF_HD unsigned tsdf_edge_type(unsigned a, unsigned b) { return (a ^ b) - 1u; }
TSDF_HD bool tsdf_edge_in_cube(unsigned type, unsigned o) { return ((type + 1u) & o) == 0u; }

// The triangles of a tetrahedron.  code: bit i set when v_i is inside.  *n: how many (0 .. 2).  A triangle is three edges, each
// the pair (i, j), i < j, of corner indices packed as i | j << 2; tri[0 .. 2] the first, tri[3 .. 5] the second.  With one corner
// a apart from b < c < d: (ab, ac, ad); with a < b inside and c < d outside: (ac, ad, bd), (ac, bd, bc).
#define TSDF_E(i, j) ((unsigned)((i) < (j) ? (i) | ((j) << 2) : (j) | ((i) << 2)))
TSDF_HD int tsdf_case_count(unsigned code) {
  const unsigned k = (code & 1u) + ((code >> 1) & 1u) + ((code >> 2) & 1u) + ((code >> 3) & 1u);
  return k == 0u || k == 4u ? 0 : (k == 2u ? 2 : 1);
}
// The 6 x 16 table: bit `code` of TSDF_SWAP(k) says that the triangles of the tetrahedron k in that case are listed with their
// last two vertices swapped, so that the normal points from the inside corners to the outside corners (decided at the edge
// midpoints in exact arithmetic: tests/map_tsdf_ref.py swap_table, tests/cpp/tsdf_host.cpp).  Even permutations (k = 0, 3, 4)
// share one word and odd ones its complement over the cases 1 .. 14.
#define TSDF_SWAP_EVEN 0x4D24u
#define TSDF_SWAP_ODD 0x32DAu
TSDF_HD unsigned tsdf_swap_word(int k) { return (k == 0 || k == 3 || k == 4) ? TSDF_SWAP_EVEN : TSDF_SWAP_ODD; }

// The triangle j (0 or 1) of a case as three packed edges e0 | e1 << 4 | e2 << 8, before the swap.
TSDF_HD unsigned tsdf_case_triangle(unsigned code, int j) {
  const int k = tsdf_case_count(code);
  if (k == 1) {
    const unsigned one = (code & (code - 1u)) == 0u ? code : (~code & 15u);  // the lone corner's bit
    const int a = one == 1u ? 0 : one == 2u ? 1 : one == 4u ? 2 : 3;
    const int b = a == 0 ? 1 : 0, c = a <= 1 ? 2 : 1, d = a <= 2 ? 3 : 2;
    return TSDF_E(a, b) | (TSDF_E(a, c) << 4) | (TSDF_E(a, d) << 8);
  }
  // two inside: a < b inside, c < d outside
  int a = 0, b = 0, c = 0, d = 0;
  switch (code) {
    case 3: a = 0; b = 1; c = 2; d = 3; break;
    case 5: a = 0; b = 2; c = 1; d = 3; break;
    case 9: a = 0; b = 3; c = 1; d = 2; break;
    case 6: a = 1; b = 2; c = 0; d = 3; break;
    case 10: a = 1; b = 3; c = 0; d = 2; break;
    default: a = 2; b = 3; c = 0; d = 1; break;  // 12
  }
  return j == 0 ? TSDF_E(a, c) | (TSDF_E(a, d) << 4) | (TSDF_E(b, d) << 8) : TSDF_E(a, c) | (TSDF_E(b, d) << 4) | (TSDF_E(b, c) << 8);
}

// Where the vertex sits on its edge, from the lower end: (s0, w0) the lower end's cell, (s1, w1) the upper end's, one of them
// inside and the other not, both weights in 1 .. 2^20.  The products are exact in int64 (below 2^51), their difference too, and
// the quotient of the two doubles is rounded once to double and once to float.
TSDF_HD float tsdf_edge_alpha(int32_t s0, uint32_t w0, int32_t s1, uint32_t w1) {
  const int64_t n0 = (int64_t)s0 * (int64_t)w1, n1 = (int64_t)s1 * (int64_t)w0;
  return (float)((double)n0 / (double)(n0 - n1));
}
// One coordinate of a vertex: the cell's centre (revo_map_observe's), plus a along the axes the edge runs along.
TSDF_HD float tsdf_vertex_axis(int lo, int c, bool along, float a, float voxel) {
  return (((float)(lo + c) + 0.5f) + (along ? a : 0.0f)) * voxel;
}

// ---- the attributes of a vertex (revo_map_tsdf_mesh_attr): every float32 operation rounded on its own ----
TSDF_HD float tsdf_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fdiv_rn(a, b);
#else
  return a / b;
#endif
}
// (sqrtf, not __fsqrt_rn: without OCML's rounded operations that one is the hardware's approximate square root; sqrtf is
// correctly rounded under the compiler's default -fhip-fp32-correctly-rounded-divide-sqrt)
TSDF_HD float tsdf_sqrt(float a) {
#if defined(__HIP_DEVICE_COMPILE__)
  return sqrtf(a);
#else
  return std::sqrt(a);
#endif
}
// The field at a cell with weight > 0, in units of trunc / 1024; a colour channel's mean is the same quotient of a uint32 sum.
TSDF_HD float tsdf_field(int32_t sum, uint32_t weight) { return tsdf_div((float)sum, (float)weight); }
TSDF_HD float tsdf_channel(uint32_t sum, uint32_t weight) { return tsdf_div((float)sum, (float)weight); }
// One axis of the gradient at a cell: fc the cell's field, (vm, fm) and (vp, fp) whether the neighbours c - e and c + e are
// valid (a cell outside the box is not) and their fields.
TSDF_HD float tsdf_grad_axis(bool vm, float fm, float fc, bool vp, float fp) {
  if (vm && vp) return (fp - fm) * 0.5f;
  if (vp) return fp - fc;
  if (vm) return fc - fm;
  return 0.0f;
}
// Between the edge's two ends: x0 at the lower, x1 at the upper, a the vertex's place.
TSDF_HD float tsdf_lerp(float x0, float x1, float a) { return x0 + a * (x1 - x0); }
// The unit normal of a gradient; (0, 0, 0) when its squared length is 0 or not finite.
TSDF_HD void tsdf_normal(float gx, float gy, float gz, float* nx, float* ny, float* nz) {
  const float l2 = (gx * gx + gy * gy) + gz * gz;
  if (!(l2 > 0.0f) || !std::isfinite(l2)) { *nx = 0.0f; *ny = 0.0f; *nz = 0.0f; return; }
  const float l = tsdf_sqrt(l2);
  *nx = tsdf_div(gx, l);
  *ny = tsdf_div(gy, l);
  *nz = tsdf_div(gz, l);
}
// How many of an edge's two end cells carry a colour.
TSDF_HD unsigned tsdf_color_k(uint32_t cw0, uint32_t cw1) { return (cw0 > 0u ? 1u : 0u) + (cw1 > 0u ? 1u : 0u); }
// One channel's byte of a vertex: (s0, cw0) the lower end's sum and colour weight, (s1, cw1) the upper end's.
TSDF_HD uint8_t tsdf_color_byte(uint32_t s0, uint32_t cw0, uint32_t s1, uint32_t cw1, float a) {
  float v = 0.0f;
  if (cw0 > 0u && cw1 > 0u) v = tsdf_lerp(tsdf_channel(s0, cw0), tsdf_channel(s1, cw1), a);
  else if (cw0 > 0u) v = tsdf_channel(s0, cw0);
  else if (cw1 > 0u) v = tsdf_channel(s1, cw1);
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint8_t)rintf(fminf(fmaxf(v, 0.0f), 255.0f));
#else
  return (uint8_t)std::nearbyint(std::fmin(std::fmax(v, 0.0f), 255.0f));  // the default rounding mode: ties to even
#endif
}
