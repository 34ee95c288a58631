// revo_track_px.h -- the tracker's per-point arithmetic (projection, bilinear sample of the DT patch with the gradients formed
// on the fly, edge filter, Huber weight, Jacobian, normal-equation terms, the error-only retry), laid out in REGISTER PAIRS by
// hand.  Plain code that builds for the host and for the device: k_track / k_pair_info (through revo_track_dev.h) include the
// very code tests/test_track_px_cpu.py checks against the scalar form it replaced.
//
// gfx950 has packed float arithmetic (v_pk_mul/add/fma_f32: two IEEE operations per instruction on the halves of 64-bit
// register pairs).  Left to itself the SLP vectorizer finds such pairs in scalar code but builds their operands out of
// registers that are not adjacent: 50 of the 176 vector instructions of a full point were moves.  Here every packed operand is
//   * an aligned pair as a load delivers it (the patch rows arrive as dwordx4 / dwordx2: (b0,b1) (b2,b3) (c0,c1) (c2,c3) (a0,a1)
//     (d0,d1)), or as an earlier packed operation or two scalar results written side by side leave it,
//   * or a scalar broadcast (an op_sel of the instruction, no move),
// and the only swizzles are the two middle pairs (b1,b2), (c1,c2) of the patch and one half swap in the Jacobian.
//
// SAME BITS: every scalar result is the same IEEE operation on the same operands as in the scalar form (a product may have its
// factors commuted and a negation moved across it: both exact; only a NaN's sign bit could tell, and a valid point's terms are
// finite).  No contraction (-ffp-contract=off), fmaf only where the scalar
// form had it.  The lanes of a pair never mix: a pair operation is two independent scalar operations.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TPX_HD __host__ __device__ __forceinline__
#else
#define TPX_HD inline
#endif

namespace {

#if defined(__HIP_DEVICE_COMPILE__)
typedef float tpx_f2 __attribute__((ext_vector_type(2)));
TPX_HD tpx_f2 tpx_mk(float a, float b) { return tpx_f2{a, b}; }
TPX_HD tpx_f2 tpx_swap(tpx_f2 v) { return __builtin_shufflevector(v, v, 1, 0); }             // (v.y, v.x)
TPX_HD tpx_f2 tpx_hi_lo(tpx_f2 a, tpx_f2 b) { return __builtin_shufflevector(a, b, 1, 2); }  // (a.y, b.x)
TPX_HD tpx_f2 tpx_fma(tpx_f2 a, tpx_f2 b, tpx_f2 c) { return __builtin_elementwise_fma(a, b, c); }
TPX_HD float tpx_rcp(float d) { return __builtin_amdgcn_rcpf(d); }
// A value the optimiser must take as a scalar of its own (no instruction).  Without it the middle end re-joins scalar
// operations on the two halves of a pair into a packed one and then moves the results to where the source had put them.
TPX_HD float tpx_scalar(float v) { asm("" : "+v"(v)); return v; }
// some value, no matter which (and no instruction): what a register holds before an exec-masked load fills the lanes that need it
TPX_HD tpx_f2 tpx_any() { tpx_f2 v; return __builtin_nondeterministic_value(v); }
#else
// the host's two-float stand-in: lane-wise operators, nothing else
struct tpx_f2 { float x, y; };
TPX_HD tpx_f2 tpx_mk(float a, float b) { return tpx_f2{a, b}; }
TPX_HD tpx_f2 operator+(tpx_f2 a, tpx_f2 b) { return tpx_f2{a.x + b.x, a.y + b.y}; }
TPX_HD tpx_f2 operator-(tpx_f2 a, tpx_f2 b) { return tpx_f2{a.x - b.x, a.y - b.y}; }
TPX_HD tpx_f2 operator*(tpx_f2 a, tpx_f2 b) { return tpx_f2{a.x * b.x, a.y * b.y}; }
TPX_HD tpx_f2 operator-(tpx_f2 a) { return tpx_f2{-a.x, -a.y}; }
TPX_HD tpx_f2 tpx_swap(tpx_f2 v) { return tpx_f2{v.y, v.x}; }
TPX_HD tpx_f2 tpx_hi_lo(tpx_f2 a, tpx_f2 b) { return tpx_f2{a.y, b.x}; }
TPX_HD tpx_f2 tpx_fma(tpx_f2 a, tpx_f2 b, tpx_f2 c) { return tpx_f2{fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y)}; }
TPX_HD float tpx_scalar(float v) { return v; }
TPX_HD tpx_f2 tpx_any() { return tpx_f2{0.0f, 0.0f}; }
TPX_HD float tpx_rcp(float d) { return 1.0f / d; }  // stand-in for the hardware reciprocal (the tests compare FORMS, not it)
#endif
TPX_HD tpx_f2 tpx_splat(float a) { return tpx_mk(a, a); }
TPX_HD tpx_f2 tpx_sel(bool c, tpx_f2 a, tpx_f2 b) { return c ? a : b; }

// revo_div.h's sequences, scalar and on a pair of numerators over one denominator
TPX_HD float tpx_recip_refined(float d) {
  const float r0 = tpx_rcp(d);
  const float e0 = fmaf(-d, r0, 1.0f);
  return fmaf(e0, r0, r0);
}
TPX_HD float tpx_div_with(float n, float d, float r1) {
  const float q0 = n * r1;
  const float e1 = fmaf(-d, q0, n);
  const float q1 = fmaf(e1, r1, q0);
  const float e2 = fmaf(-d, q1, n);
  return fmaf(e2, r1, q1);
}
TPX_HD float tpx_div(float n, float d) { return tpx_div_with(n, d, tpx_recip_refined(d)); }
TPX_HD tpx_f2 tpx_div_with2(tpx_f2 n, float d, float r1) {
  const tpx_f2 md = tpx_splat(-d), r = tpx_splat(r1);
  const tpx_f2 q0 = n * r;
  const tpx_f2 e1 = tpx_fma(md, q0, n);
  const tpx_f2 q1 = tpx_fma(e1, r, q0);
  const tpx_f2 e2 = tpx_fma(md, q1, n);
  return tpx_fma(e2, r, q1);
}

struct Cam { float fx, fy, cx, cy, wlim, hlim; int w, h; };
// XY = (X, Y), d = (dx, dy); rz: refined 1/Z
struct PtState { tpx_f2 XY; float Z, rz; tpx_f2 d; int ix, iy; bool valid; };
// 12 DT samples around (ix,iy): rows iy-1 (2), iy (4), iy+1 (4), iy+2 (2), as the loads deliver them
struct DtPatch { tpx_f2 a, b01, b23, c01, c23, d; };

TPX_HD PtState project_point(float px, float py, float pz, const float* R, const float* T, const Cam& c, bool in_range) {
  PtState s;
  const tpx_f2 XY = ((tpx_mk(R[0], R[1]) * tpx_splat(px) + tpx_mk(R[3], R[4]) * tpx_splat(py)) + tpx_mk(R[6], R[7]) * tpx_splat(pz)) +
                    tpx_mk(T[0], T[1]);
  const float Z = ((R[2] * px + R[5] * py) + R[8] * pz) + T[2];
  // X/Z and Y/Z, correctly rounded, off ONE refined reciprocal (revo_div.h: the same bits as two IEEE divisions)
  const float rz = tpx_recip_refined(Z);
  const tpx_f2 uv = tpx_div_with2(XY, Z, rz) * tpx_mk(c.fx, c.fy) + tpx_mk(c.cx, c.cy);
  s.valid = in_range && (uv.x > 1.0f && uv.y > 1.0f && uv.x < c.wlim && uv.y < c.hlim);  // optimizer.cpp:100 (NaN-safe form)
  // an invalid point samples pixel (1, 1) with dx = dy = 0: (u, v) <- (1, 1) BEFORE the truncation gives ix = iy = 1 and
  // 1.0f - 1.0f = +0.0f, the values the scalar form selected afterwards
  const tpx_f2 t = tpx_sel(s.valid, uv, tpx_splat(1.0f));
  s.ix = (int)t.x;
  s.iy = (int)t.y;
  s.d = t - tpx_mk((float)s.ix, (float)s.iy);
  s.XY = tpx_sel(s.valid, XY, tpx_splat(0.0f));
  s.Z = s.valid ? Z : 1.0f;
  s.rz = s.valid ? rz : 1.0f;
  return s;
}

// The bilinear weights as x-corner pairs: W0 = (w00, w10) for row iy, W1 = (w01, w11) for row iy + 1 -- four scalar results
// written side by side
struct BiW { tpx_f2 W0, W1; };
TPX_HD BiW bilinear_weights(tpx_f2 d) {
  const float dx = tpx_scalar(d.x), dy = tpx_scalar(d.y);
  const float dxdy = dx * dy;
  BiW w;
  w.W0 = tpx_mk(((1.0f - dx) - dy) + dxdy, dx - dxdy);
  w.W1 = tpx_mk(dy - dxdy, dxdy);
  return w;
}
// ((w11*g11 + w01*g01) + w10*g10) + w00*g00 with G0 = (g00, g10), G1 = (g01, g11)
TPX_HD float bilinear(const BiW& w, tpx_f2 G0, tpx_f2 G1) {
  const tpx_f2 P0 = w.W0 * G0, P1 = w.W1 * G1;
  return ((P1.y + P1.x) + P0.y) + P0.x;
}

// What a full candidate's point contributes, before it is summed: calcErrorAndBuffers' interpolation + filter + Huber
// (optimizer.cpp:106-133, optimizer.h:156-185) and the image gradient scaled by the focal lengths
struct PtTerm { float r0, r1, res, wr; tpx_f2 G; bool good; };  // G = (fx*r0, fy*r1)
TPX_HD PtTerm point_term(const PtState& s, const DtPatch& q, float fx, float fy, float edist, bool filt, float huber) {
  // the reference's table entries at the four corners: (0.5(prev-next), 0.5(up-down), dt), x-corner pairs
  const tpx_f2 b12 = tpx_hi_lo(q.b01, q.b23), c12 = tpx_hi_lo(q.c01, q.c23), h = tpx_splat(0.5f);
  const tpx_f2 GX0 = h * (q.b01 - q.b23), GX1 = h * (q.c01 - q.c23);  // (gx00, gx10), (gx01, gx11)
  const tpx_f2 GY0 = h * (q.a - c12), GY1 = h * (b12 - q.d);          // (gy00, gy10), (gy01, gy11)
  const BiW w = bilinear_weights(s.d);
  PtTerm t;
  t.r0 = bilinear(w, GX0, GX1);
  t.r1 = bilinear(w, GY0, GY1);
  t.res = bilinear(w, b12, c12);  // (d00, d10) = (b1, b2), (d01, d11) = (c1, c2)
  t.good = s.valid && !(t.res > edist && filt);  // optimizer.cpp:108
  if (!t.good) { t.r0 = 0.0f; t.r1 = 0.0f; t.res = 0.0f; }
  t.wr = (t.res <= huber) ? 1.0f : tpx_div(huber, t.res);
  t.G = tpx_mk(fx, fy) * tpx_mk(t.r0, t.r1);
  return t;
}

// calculateWarpUpdate's Jacobian (optimizer.cpp:218-228) as three pairs (jv0,jv1) (jv2,jv3) (jv4,jv5); zs = z*z (the reference:
// 1/(pz*pz), optimizer.cpp:213; differs by <= 1 ulp)
struct Jac { tpx_f2 J01, J23, J45; };
TPX_HD Jac jacobian(const PtState& s, tpx_f2 G) {
  const float z = tpx_div_with(1.0f, s.Z, s.rz);
  const float zs = z * z;
  Jac j;
  j.J01 = tpx_splat(z) * G;                              // z*gx, z*gy
  const tpx_f2 B = ((-s.XY) * tpx_splat(zs)) * G;        // (-X*zs)*gx, (-Y*zs)*gy
  const tpx_f2 O = tpx_splat(1.0f) + (s.XY * s.XY) * tpx_splat(zs);  // 1 + X*X*zs, 1 + Y*Y*zs
  const float xyz = (s.XY.x * s.XY.y) * zs;              // X*Y*zs; -X*Y*zs = -(X*Y*zs) exactly
  const tpx_f2 P = tpx_splat(xyz) * G, U = O * G;        // (X*Y*zs)*gx, (X*Y*zs)*gy; (1 + X*X*zs)*gx, (1 + Y*Y*zs)*gy
  const tpx_f2 C = tpx_swap(s.XY * tpx_splat(z)) * G;    // (Y*z)*gx, (X*z)*gy
  j.J23 = tpx_mk(B.x + B.y, (-P.x) + (-U.y));
  j.J45 = tpx_mk(U.x + P.y, (-C.x) + C.y);
  return j;
}

// LGS6::update: acc[k] += (wr*jv[a]) * jv[c] for the upper triangle k = 0..20 (row a, c >= a), acc[21 + a] += (wr*jv[a]) * res.
// The rows are walked in the pairs the Jacobian lives in: (k, k+1) = w_a * (jv_c, jv_c+1) for c = 0, 2, 4 -- twelve pair
// updates and the three diagonal entries 6, 15, 20 that have no partner.
TPX_HD void fma_pair(float* acc, int k, tpx_f2 a, tpx_f2 b) {
  const tpx_f2 r = tpx_fma(a, b, tpx_mk(acc[k], acc[k + 1]));
  acc[k] = r.x;
  acc[k + 1] = r.y;
}
TPX_HD void accumulate_normal(const Jac& j, float wr, float res, float* acc) {
  const tpx_f2 wq = tpx_splat(wr);
  const tpx_f2 W01 = wq * j.J01, W23 = wq * j.J23, W45 = wq * j.J45;
  fma_pair(acc, 0, tpx_splat(W01.x), j.J01);
  fma_pair(acc, 2, tpx_splat(W01.x), j.J23);
  fma_pair(acc, 4, tpx_splat(W01.x), j.J45);
  acc[6] = fmaf(W01.y, j.J01.y, acc[6]);
  fma_pair(acc, 7, tpx_splat(W01.y), j.J23);
  fma_pair(acc, 9, tpx_splat(W01.y), j.J45);
  fma_pair(acc, 11, tpx_splat(W23.x), j.J23);
  fma_pair(acc, 13, tpx_splat(W23.x), j.J45);
  acc[15] = fmaf(W23.y, j.J23.y, acc[15]);
  fma_pair(acc, 16, tpx_splat(W23.y), j.J45);
  fma_pair(acc, 18, tpx_splat(W45.x), j.J45);
  acc[20] = fmaf(W45.y, j.J45.y, acc[20]);
  const tpx_f2 rq = tpx_splat(res);
  fma_pair(acc, 21, W01, rq);
  fma_pair(acc, 23, W23, rq);
  fma_pair(acc, 25, W45, rq);
}

// An error-only retry of the same point: its four DT samples as the pairs D0 = (d00, d10), D1 = (d01, d11)
struct RetryTerm { float res, wr; bool good; };
TPX_HD RetryTerm retry_term(const PtState& s, tpx_f2 D0, tpx_f2 D1, float edist, bool filt, float huber) {
  RetryTerm t;
  t.res = bilinear(bilinear_weights(s.d), D0, D1);
  t.good = s.valid && !(t.res > edist && filt);
  if (!t.good) t.res = 0.0f;
  t.wr = (t.res <= huber) ? 1.0f : tpx_div(huber, t.res);
  return t;
}
// A retry that lands on candidate 0's pixel (ix0, iy0) or a direct neighbour has its samples in the 12-sample patch: rows iy0 /
// iy0+1 shifted by -1, 0, 1, or rows iy0-1 / iy0, or rows iy0+1 / iy0+2 (same column)
TPX_HD bool retry_in_patch(int ix, int iy, int ix0, int iy0) {
  return (iy == iy0 && (unsigned)(ix - ix0 + 1) <= 2u) || (ix == ix0 && (unsigned)(iy - iy0 + 1) <= 2u);
}
// D0 = (d00, d10), D1 = (d01, d11) of a retry at (ix, iy) that is in the patch
TPX_HD void retry_pick(const DtPatch& q, int ix, int iy, int ix0, int iy0, tpx_f2& D0, tpx_f2& D1) {
  const bool same_row = iy == iy0, up = iy < iy0, left = ix < ix0, mid = ix == ix0;
  const tpx_f2 b12 = tpx_hi_lo(q.b01, q.b23), c12 = tpx_hi_lo(q.c01, q.c23);
  D0 = tpx_sel(same_row, tpx_sel(left, q.b01, tpx_sel(mid, b12, q.b23)), tpx_sel(up, q.a, c12));
  D1 = tpx_sel(same_row, tpx_sel(left, q.c01, tpx_sel(mid, c12, q.c23)), tpx_sel(up, b12, q.d));
}

}  // namespace
