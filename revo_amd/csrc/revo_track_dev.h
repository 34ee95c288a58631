// revo_track_dev.h -- the per-point device code of the tracker that more than one kernel file uses: the projection, the
// 12-sample DT patch with the gradients formed on the fly, the reference's per-point terms of the normal equations
// (exact-sums form) and the double-double arithmetic they are summed with.  revo_track.hip (k_track) and
// revo_info.hip (k_pair_info) include it, so a pair's information matrix is made of the very terms its tracker summed.
// Everything is __forceinline__ in an unnamed namespace: a translation unit only pays for what it calls.
#pragma once
#include "revo_dev.h"
#include "revo_div.h"
#include "revo_track_px.h"  // the per-point arithmetic in register pairs: projection, patch terms, Jacobian, normal-equation updates

#define CSLOT 27  // float slots: 0..26 normal equations (21 + 6), CSLOT + j = good-point count of candidate j
#define XERR 27   // exact-sums layout: double-double slots 0..26 = normal equations, XERR + k = error slot k (DSLOT below)

namespace {

__device__ __forceinline__ bool is_orthogonal(const float* R) {  // rotation_matrix.hpp:14-24, so3.hpp:419-424
  float n2 = 0.0f;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = R[r] * R[c] + R[3 + r] * R[3 + c] + R[6 + r] * R[6 + c];
      v -= (r == c) ? 1.0f : 0.0f;
      n2 += v * v;
    }
  const float det = R[0] * (R[4] * R[8] - R[7] * R[5]) - R[3] * (R[1] * R[8] - R[7] * R[2]) + R[6] * (R[1] * R[5] - R[4] * R[2]);
  return sqrtf(n2) < 1e-5f && det > 0.0f;
}

// lane L <- the value of lane L ^ MASK (DPP inside a row of 16 lanes, ds_bpermute across rows); a double crosses as two words
template <int MASK>
__device__ __forceinline__ float lane_xor(float v) {
  const int s = (int)__float_as_uint(v);
  int r;
  if (MASK == 1) r = __builtin_amdgcn_update_dpp(0, s, 0xB1, 0xf, 0xf, true);        // quad_perm [1,0,3,2]
  else if (MASK == 2) r = __builtin_amdgcn_update_dpp(0, s, 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
  else if (MASK == 4) {
    r = __builtin_amdgcn_update_dpp(0, s, 0x104, 0xf, 0x5, false);                   // row_shl:4 into banks 0, 2 (lane bit 2 clear)
    r = __builtin_amdgcn_update_dpp(r, s, 0x114, 0xf, 0xa, false);                   // row_shr:4 into banks 1, 3
  } else if (MASK == 8) r = __builtin_amdgcn_update_dpp(0, s, 0x128, 0xf, 0xf, true);  // row_ror:8
  else return __shfl_xor(v, MASK);
  return __uint_as_float((unsigned)r);
}

// the slot a lane holds after a 32-value butterfly (reduce32 / reduce32x)
__device__ __forceinline__ int idx32(int lane) {
  return ((lane & 1) << 4) | ((lane & 2) << 2) | (lane & 4) | ((lane & 8) >> 2) | ((lane & 16) >> 4);
}

template <int MASK>
__device__ __forceinline__ double lane_xor_d(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const unsigned lo = __float_as_uint(lane_xor<MASK>(__uint_as_float((unsigned)u)));
  const unsigned hi = __float_as_uint(lane_xor<MASK>(__uint_as_float((unsigned)(u >> 32))));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// ---- the exact-sums variant: double-double arithmetic -------------------------------------------------------------
// dd_acc: (h, l) += x with Knuth's TwoSum -- the rounding error of h + x is formed exactly and lands in l.  The per-point
// terms are floats, so a thread's (h, l) is their exact sum up to l's own roundings (~2^-106 of the largest partial).
__device__ __forceinline__ void dd_acc(double& h, double& l, double x) {
  const double s = h + x, bb = s - h;
  l += (h - (s - bb)) + (x - bb);
  h = s;
}
// (h, l) += (h2, l2): TwoSum of the heads, the tails added to the error, renormalised (Fast2Sum).  Symmetric in its two
// operands (TwoSum's error is exact whatever the order), so the two lanes of a butterfly pair hold the same bits.
__device__ __forceinline__ void dd_add(double& h, double& l, double h2, double l2) {
  const double s = h + h2, bb = s - h;
  double e = (h - (s - bb)) + (h2 - bb);
  e += l + l2;
  h = s + e;
  l = e - (h - s);
}
// h + l rounded ONCE to float: h + l rounded to odd in double (53 >= 24 + 2 bits), then to nearest float.  A plain
// (float)(h + l) could round twice (to double, then to float) and miss the float nearest h + l at a midpoint.
__device__ __forceinline__ float dd_to_float(double h, double l) {
  const double s = h + l, bb = s - h;
  const double e = (h - (s - bb)) + (l - bb);
  long long bits = __double_as_longlong(s);
  if (e != 0.0 && (bits & 1) == 0 && __builtin_isfinite(s)) bits += ((e > 0.0) == (s > 0.0)) ? 1 : -1;
  return (float)__longlong_as_double(bits);
}
// 32 double-double values (h[], l[]): lane L ends with the wave total of value idx32(L) in h[0], l[0] -- reduce32's tree
template <int HALF, int MASK>
__device__ __forceinline__ void butterfly_step_x(double* h, double* l, int lane) {
  const bool up = (lane & MASK) != 0;
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const double sh = up ? h[i] : h[HALF + i], sl = up ? l[i] : l[HALF + i];
    double kh = up ? h[HALF + i] : h[i], kl = up ? l[HALF + i] : l[i];
    dd_add(kh, kl, lane_xor_d<MASK>(sh), lane_xor_d<MASK>(sl));
    h[i] = kh; l[i] = kl;
  }
}
__device__ __forceinline__ void reduce32x(double* h, double* l, int lane) {
  butterfly_step_x<16, 1>(h, l, lane);
  butterfly_step_x<8, 2>(h, l, lane);
  butterfly_step_x<4, 4>(h, l, lane);
  butterfly_step_x<2, 8>(h, l, lane);
  butterfly_step_x<1, 16>(h, l, lane);
  dd_add(h[0], l[0], lane_xor_d<32>(h[0]), lane_xor_d<32>(l[0]));
}

// explicit global address space: the pointers come out of the descriptor (generic), and
// flat loads would tie up both vmcnt and lgkmcnt
typedef float f4v __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(1)))* gf32p;
typedef const f4v __attribute__((address_space(1)))* gf4p;

// 4-byte aligned vector types: the middle rows of the patch are ONE dwordx4 gather each (global loads only need
// dword alignment) -- a gather instruction costs the vector L1 one tag lookup per distinct cache line among the 64
// lanes, whatever its width, and that lookup rate is part of what bounds the evaluation of the fine levels
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
typedef const f4u __attribute__((address_space(1)))* gf4up;
typedef const f2u __attribute__((address_space(1)))* gf2up;
__device__ __forceinline__ DtPatch load_patch(gf32p dt, int w, int ix, int iy) {
  gf32p p = dt + iy * w + ix;
  DtPatch q;  // rows iy-1 (2), iy (4), iy+1 (4), iy+2 (2): the register pairs of revo_track_px.h, as the loads deliver them
  const f2u a = *(gf2up)(p - w);
  const f4u b = *(gf4up)(p - 1);
  const f4u c = *(gf4up)(p + w - 1);
  const f2u d = *(gf2up)(p + 2 * w);
  q.a = tpx_mk(a.x, a.y);
  q.b01 = tpx_mk(b.x, b.y); q.b23 = tpx_mk(b.z, b.w);
  q.c01 = tpx_mk(c.x, c.y); q.c23 = tpx_mk(c.z, c.w);
  q.d = tpx_mk(d.x, d.y);
  return q;
}

// The candidate's error terms.  The LM's accept / stop decisions compare exactly these sums (optimizer.cpp:129-133,273-278:
// `error < lastErr`, `error / lastErr > 0.999`), so they are the one place where the ORDER of a float sum would show: the
// per-point terms are the reference's float values (w_r * res_2 rounded to float, res_2), and the sums are carried in DOUBLE from
// the first addition on -- per thread, through the butterflies, LDS and the cluster exchange -- and rounded to float once, like the
// reference's accumulator read at the end (~1e-16 relative whatever the order, the cluster size or the speculation depth: a pose
// has ONE error however it was evaluated).  The good-point count rides in the float butterfly (exact: < 2^24).
// Double slots of a pass: 0 = sum w r^2 of candidate 0, 1 = its sum r^2 (ResidualInfo::sumErrorUnweighted: reported, never
// compared), 1 + j = sum w r^2 of the error-only retry j (j = 1..KMAX-1; nothing reads a retry's unweighted sum).
#define DSLOT(j) ((j) == 0 ? 0 : 1 + (j))
template <bool WITH_UNWEIGHTED>
__device__ __forceinline__ void accumulate_error(float res, float wr, bool good, double* ed, float* cnt) {
  const float r2 = res * res;
  ed[0] += (double)(wr * r2);
  if (WITH_UNWEIGHTED) ed[1] += (double)r2;
  *cnt += good ? 1.0f : 0.0f;
}
// The exact variant: the same float terms into double-double slot XERR + k (k = the default layout's double slot); (r*r)*w is
// also LGS6::update's error term (LGSX.h:398).  cnt: the candidate's good count.
template <bool WITH_UNWEIGHTED>
__device__ __forceinline__ void accumulate_error_x(float res, float wr, bool good, double* xd, int k, float* cnt) {
  const float r2 = res * res;
  dd_acc(xd[XERR + k], xd[32 + XERR + k], (double)(r2 * wr));
  if (WITH_UNWEIGHTED) dd_acc(xd[XERR + k + 1], xd[32 + XERR + k + 1], (double)r2);
  *cnt += good ? 1.0f : 0.0f;
}

// The exact variant's per-point terms: calculateWarpUpdate (optimizer.cpp:211-228) and LGS6::update (LGSX.h:392-398) as the
// reference forms them -- z and z_sqr as two correctly rounded divisions, v[3] / v[4] evaluated in DOUBLE (the `1.0` literal
// promotes the expression) and rounded to float once, the terms (v[a]*v[c])*w and v[a]*(r*w) as separate float products.
// xd[k] / xd[32 + k]: head / tail of slot k (0..20: A, upper triangle; 21..26: sum v[a]*(r*w), b = its negation).
__device__ __forceinline__ void accumulate_terms_x(const PtState& s, float gx, float gy, float res, float wr, bool good, float* cnt,
                                                   double* xd) {
  const float px = s.XY.x, py = s.XY.y;
  const float z = revo_div_with(1.0f, s.Z, s.rz);  // 1.0f / pz
  const float zs = revo_div(1.0f, s.Z * s.Z);      // 1.0f / (pz*pz)
  float v[6];
  v[0] = z * gx;
  v[1] = z * gy;
  v[2] = (-px * zs) * gx + (-py * zs) * gy;
  v[3] = (float)((double)((-px * py * zs) * gx) + (-(1.0 + (double)(py * py * zs))) * (double)gy);
  v[4] = (float)((1.0 + (double)(px * px * zs)) * (double)gx + (double)((px * py * zs) * gy));
  v[5] = (-py * z) * gx + (px * z) * gy;
  {
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int c = a; c < 6; ++c) { dd_acc(xd[k], xd[32 + k], (double)((v[a] * v[c]) * wr)); ++k; }
  }
  const float rw = res * wr;
#pragma unroll
  for (int a = 0; a < 6; ++a) dd_acc(xd[21 + a], xd[53 + a], (double)(v[a] * rw));
  accumulate_error_x<true>(res, wr, good, xd, 0, cnt);
}

// calcErrorAndBuffers' interpolation + filter + Huber (optimizer.cpp:106-133, optimizer.h:156-185)
// fused with calculateWarpUpdate's Jacobian (optimizer.cpp:218-228) and LGS6::update (revo_track_px.h).
// EXACT: acc = the KMAX good counts, ed = the 32 double-double slots (heads, then tails).
template <bool EXACT>
__device__ __forceinline__ void accumulate_point(const PtState& s, const DtPatch& q, float fx, float fy, float edist, bool filt,
                                                 float huber, float* acc, double* ed) {
  const PtTerm t = point_term(s, q, fx, fy, edist, filt, huber);
  if constexpr (EXACT) {
    accumulate_terms_x(s, t.G.x, t.G.y, t.res, t.wr, t.good, acc, ed);
    return;
  }
  accumulate_normal(jacobian(s, t.G), t.wr, t.res, acc);
  accumulate_error<true>(t.res, t.wr, t.good, ed, acc + CSLOT);
}

template <bool EXACT>
__device__ __forceinline__ void full_point(const f4v p, gf32p dtm, const float* R, const float* T, const Cam& c, float edist,
                                           bool filt, float huber, float* acc, double* ed) {
  const PtState s = project_point(p.x, p.y, p.z, R, T, c, true);
  const DtPatch q = load_patch(dtm, c.w, s.ix, s.iy);
  accumulate_point<EXACT>(s, q, c.fx, c.fy, edist, filt, huber, acc, ed);
}

}  // namespace
