// The per-pixel decision of cv::Canny's non-maximum suppression (imgpyramidrgbd.cpp:184), plain integer C++ that builds
// for the host and for the device: k_canny_nms4 (revo_pyramid.hip) includes the very code tests/test_nms_decision_cpu.py checks.
//
// Inputs of one pixel: its 3x3 neighbourhood of |grad|^2 (rows a, b, c; m is the centre), integers in [0, 2 * 1020^2] with 0 for
// a masked (outside / invalid) pixel, its own gradient packed as (dx & 0xffff) | dy << 16 with |dx|, |dy| <= 1020, and the two
// squared thresholds.  Output: candidate = non-maximum-suppressed and m > low; strong = candidate and m > high.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NMS_HD __host__ __device__ __forceinline__
#else
#define NMS_HD inline
#endif

#define NMS_TG22 13573  // (int)(0.41421356...*(1<<15) + 0.5)

// The gradient's direction class.  horiz: |dy| < tan(22.5) |dx|; vert: |dy| > tan(67.5) |dx| (= (2 + tan 22.5) |dx| in cv::Canny's
// fixed point); neither: a diagonal, `neg` (sign(dx) != sign(dy)) tells which.
struct NmsDir { bool horiz, vert, neg; };
// |dx| | |dy| << 16.  The device has the two 16-bit halves in one packed negate and one packed max; the host takes them apart.
NMS_HD uint32_t nms_abs2(uint32_t dxy) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef short nms_s2 __attribute__((ext_vector_type(2)));
  const nms_s2 v = __builtin_bit_cast(nms_s2, dxy), z = {0, 0};
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(v, z - v));
#else
  const int dx = (int16_t)(dxy & 0xffffu), dy = (int16_t)(dxy >> 16);
  return (uint32_t)(dx < 0 ? -dx : dx) | (uint32_t)(dy < 0 ? -dy : dy) << 16;
#endif
}
// cv::Canny compares |dy| << 15 with t22 = |dx| * TG22 and with t22 + (|dx| << 16).  Doubled, and with ab = |dx| + (|dy| << 16):
//   |dy| << 16 <  2 TG22 |dx|              <=>  ab < (2 TG22 + 1) |dx|
//   |dy| << 16 > (2 TG22 + (1 << 17)) |dx|  <=>  ab > (2 TG22 + (1 << 17) + 1) |dx|
// so the packed word is compared as it is (|dx| <= 1020: the products stay below 2^28).
NMS_HD NmsDir nms_dir(uint32_t dxy) {
  const uint32_t ab = nms_abs2(dxy);
  const uint32_t ax = ab & 0xffffu;
  NmsDir d;
  d.horiz = ab < ax * (2u * NMS_TG22 + 1u);
  d.vert = ab > ax * (2u * NMS_TG22 + (1u << 17) + 1u);
  d.neg = (int32_t)(dxy ^ (dxy << 16)) < 0;  // sign(dx) != sign(dy)
  return d;
}

// REFERENCE form (the kernel's decision until the threshold form replaced it; tests are its only caller): cv::Canny's own
// direction test, then pick the two neighbours a, b along the gradient: m > a && m >= b on the axes, m > a && m > b on the diagonals.
NMS_HD NmsDir nms_dir_ref(uint32_t dxy) {
  const int dx = (int16_t)(dxy & 0xffffu), dy = (int16_t)(dxy >> 16);
  const int ax = dx < 0 ? -dx : dx, ay15 = (dy < 0 ? -dy : dy) << 15;
  const int t22 = ax * NMS_TG22;
  NmsDir d;
  d.horiz = ay15 < t22;
  d.vert = ay15 > t22 + (ax << 16);
  d.neg = (dx ^ dy) < 0;
  return d;
}
NMS_HD void nms_px_ref(int aL, int aM, int aR, int bL, int m, int bR, int cL, int cM, int cR, uint32_t dxy, int low, int high,
                       bool& cand, bool& strong) {
  const NmsDir d = nms_dir_ref(dxy);
  const int diag_a = d.neg ? aR : aL;
  const int diag_b = d.neg ? cL : cR;
  const int a = d.horiz ? bL : (d.vert ? aM : diag_a);
  const int b = d.horiz ? bR : (d.vert ? cM : diag_b);
  const bool ge = d.horiz || d.vert;
  const bool is_max = (m > a) & (ge ? (m >= b) : (m > b));
  cand = (m > low) & is_max;
  strong = cand & (m > high);
}

// THRESHOLD form.  The magnitudes are integers, so `m >= b` is `m > b - 1` and the whole decision is one comparison of m
// against the largest of the values it must exceed:
//   axes:       m > a && m >= b   <=>  m > max(a, b - 1)
//   diagonals:  m > a && m >  b   <=>  m > max(a, b)
//   candidate:  m > max(t, low),   strong:  m > max(t, low, high)     (t = the direction's threshold)
// low and high are applied independently, as the reference does: low > high keeps working.
// The caller passes bR1 = bR - 1 and cM1 = cM - 1 (it forms B - 1 once per magnitude and shares it between the pixels that
// use it).  A masked neighbour's 0 may arrive as -1 or as 0: m = 0 is never a maximum (m > a with a >= 0 fails) and every
// m >= 1 exceeds both.
// The outcome is returned as the SIGN BIT of T - m (all values are below 2^22 in magnitude: no overflow), which the caller
// shifts into its bitmap nibble: no compare, no boolean algebra on lane masks.
struct NmsOut { uint32_t cand, strong; };  // bit 31 = the decision, the other bits are unspecified
NMS_HD int nms_max(int a, int b) { return a > b ? a : b; }
NMS_HD NmsOut nms_px_thr(int aL, int aM, int aR, int bL, int m, int bR1, int cL, int cM1, int cR, uint32_t dxy, int low, int low_high) {
  const NmsDir d = nms_dir(dxy);
  const int th = nms_max(bL, bR1);
  const int tv = nms_max(aM, cM1);
  const int tp = nms_max(aL, cR), tn = nms_max(aR, cL);
  const int td = d.neg ? tn : tp;
  const int t = d.horiz ? th : (d.vert ? tv : td);
  NmsOut o;
  o.cand = (uint32_t)nms_max(t, low) - (uint32_t)m;
  o.strong = (uint32_t)nms_max(t, low_high) - (uint32_t)m;   // low_high = max(low, high)
  return o;
}
// shifts a decision into the low end of a bitmap word under construction: w <- w << 1 | sign(v)
NMS_HD uint32_t nms_push(uint32_t w, uint32_t v) { return (w << 1) | (v >> 31); }
