// revo_edt_px.h -- the per-lane search of the EDT row pass, four pixels per lane from aligned 16-byte windows.  Plain integer
// code that builds for the host and for the device: k_edt_rows (revo_pyramid.hip) includes the very code
// tests/test_edt_px_cpu.py checks against a brute-force min_x' (x - x')^2 + g2(x').
//
// The row: [pad "no edge"][w values g2 = squared vertical distance][pad "no edge"] as int32, pad = w + 4, w a multiple of 4, the
// row start 16-byte aligned: every group of four pixels ("quad") is one aligned 16-byte word.  `row` points at pixel 0.
//
// Lane group q owns pixels 4q .. 4q+3.  Trip t covers the distances d = 4t + j, j = 0..3, for all four pixels at once:
//   right-hand sample of pixel i:  4q + 4t + (i + j)   -- in the aligned quads at 4q + 4t     (inner) and 4q + 4t + 4 (outer)
//   left-hand  sample of pixel i:  4q - 4t + (i - j)   -- in the aligned quads at 4q - 4t - 4 (outer) and 4q - 4t     (inner)
// The inner quad of a side is the previous trip's outer quad, still in registers: a trip reads two quads, at addresses that move
// by 16 bytes per trip, and indexes them with compile-time constants.  Trip 0 has the centre quad C as the inner quad of both
// sides.  The trips are unrolled by two so that the four quads swap roles without a move.
//
// A trip runs while 4t < w and (4t)^2 < best of SOME pixel of the lane.  EXACT: a pixel's minimum needs the distances d with
// d^2 < best (and d < w); every such d lies in a trip that runs ((4t)^2 <= d^2); more distances only add candidates
// d^2 + g2 >= the true minimum.  4t <= w - 4, so d <= w - 1 and the farthest samples are 2w - 1 and -w: inside the padding.
// EDT_INF + d^2 < 2^31 for every d < 2048.  min over integers does not care about the order.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EDT_HD __host__ __device__ __forceinline__
#define EDT_UNROLL _Pragma("unroll")
#else
#define EDT_HD inline
#define EDT_UNROLL
#endif

#define EDT_INF (1 << 29)

// four consecutive pixels of a row: one aligned 16-byte word.  On the device a register quadruple that the optimiser must take
// as it was loaded (edt_keep, no instruction): left alone it splits the 16-byte reads into the words each trip uses and reads
// the kept quads again, three to four LDS reads per trip and per-word addresses instead of two reads.
#if defined(__HIP_DEVICE_COMPILE__)
typedef int edt_quad __attribute__((ext_vector_type(4)));
EDT_HD void edt_keep(edt_quad& q) { asm volatile("" : "+v"(q)); }
#else
struct alignas(16) edt_quad {
  int v[4];
  int operator[](int i) const { return v[i]; }
};
EDT_HD void edt_keep(edt_quad&) {}
#endif

EDT_HD int edt_min(int a, int b) { return a < b ? a : b; }
EDT_HD int edt_max(int a, int b) { return a > b ? a : b; }

// the fill's rule: a 16-bit vertical distance, 0xffff = no edge in the column
EDT_HD int edt_g2(int d16) { return d16 == 0xffff ? EDT_INF : d16 * d16; }

// One trip.  in_r / in_l: the inner quads (registers), out_r / out_l: the outer quads, read here and kept for the next trip.
// pr / pl: the outer quads' addresses.  FIRST: trip 0, where j = 0 is the pixel itself (already in best).
template <bool FIRST>
EDT_HD void edt_trip(int t, const edt_quad* pr, const edt_quad* pl, const edt_quad& in_r, edt_quad& out_r, edt_quad& out_l,
                     const edt_quad& in_l, int best[4]) {
  out_r = *pr;
  out_l = *pl;
  edt_keep(out_r);
  edt_keep(out_l);
  const int R[8] = {in_r[0], in_r[1], in_r[2], in_r[3], out_r[0], out_r[1], out_r[2], out_r[3]};
  const int L[8] = {out_l[0], out_l[1], out_l[2], out_l[3], in_l[0], in_l[1], in_l[2], in_l[3]};
  const int d0 = 4 * t;
  int dd[4];  // (4t + j)^2: the same for every lane
EDT_UNROLL
  for (int j = 0; j < 4; ++j) dd[j] = (d0 + j) * (d0 + j);
EDT_UNROLL
  for (int i = 0; i < 4; ++i) {
    int m[4];
EDT_UNROLL
    for (int j = 0; j < 4; ++j) m[j] = edt_min(R[i + j], L[4 + i - j]) + dd[j];
    if (!FIRST) best[i] = edt_min(edt_min(best[i], m[0]), m[1]);
    else best[i] = edt_min(best[i], m[1]);
    best[i] = edt_min(edt_min(best[i], m[2]), m[3]);
  }
}

// does trip t (>= 1) still have something to find?
EDT_HD bool edt_more(int t, int w, const int best[4]) {
  const int d0 = 4 * t;
  return d0 < w && d0 * d0 < edt_max(edt_max(best[0], best[1]), edt_max(best[2], best[3]));
}

// best[i] = min_x' (4q + i - x')^2 + g2(x') for the four pixels of group q
EDT_HD void edt_search4(const int* row, int q, int w, int best[4]) {
  const edt_quad* c = reinterpret_cast<const edt_quad*>(row) + q;
  edt_quad A = c[0], B, O, I;
  edt_keep(A);
EDT_UNROLL
  for (int i = 0; i < 4; ++i) best[i] = A[i];
  edt_trip<true>(0, c + 1, c - 1, A, B, O, A, best);
  for (int t = 1;; t += 2) {
    if (!edt_more(t, w, best)) break;
    edt_trip<false>(t, c + t + 1, c - t - 1, B, A, I, O, best);
    if (!edt_more(t + 1, w, best)) break;
    edt_trip<false>(t + 1, c + t + 2, c - t - 2, A, B, O, I, best);
  }
}

// sqrtf of an integer-valued float in [0, 2^24) from an estimate s within 1 ulp of it (v_sqrt_f32): the +-1 ulp correction of the
// compiler's own sqrtf expansion, without its scaling of tiny inputs and its inf / nan / zero classification (x = 0 falls through
// both corrections: the residual of the lower neighbour is NaN, that of the upper one is not positive).  Same instructions on
// the same values as sqrtf(x) for x >= 1: correctly rounded.
EDT_HD float edt_sqrt_fix(float x, float s) {
  uint32_t si;
  __builtin_memcpy(&si, &s, 4);
  const uint32_t di = si - 1u, ui = si + 1u;
  float sd, su;
  __builtin_memcpy(&sd, &di, 4);
  __builtin_memcpy(&su, &ui, 4);
  const float rd = __builtin_fmaf(-sd, s, x), ru = __builtin_fmaf(-su, s, x);
  float r = (rd <= 0.0f) ? sd : s;
  r = (ru > 0.0f) ? su : r;
  return r;
}
EDT_HD float edt_sqrt_rn_int(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return edt_sqrt_fix(x, __builtin_amdgcn_sqrtf(x));
#else
  return edt_sqrt_fix(x, sqrtf(x));
#endif
}
// the DT value of a pixel: no edge in the whole image -> OpenCV's 1e15f sentinel
// (the root is taken in every lane and then selected: four short branches around it cost more than the roots they skip)
EDT_HD float edt_dt(int best) {
  const float r = edt_sqrt_rn_int((float)best);
  return best >= EDT_INF ? sqrtf(1e15f) : r;
}

// a / b for 0 <= a < 4096 and any b >= 1 without an integer division, from inv within 2 ulp of 1 / b: (a + 0.5) / b is at least
// 0.5 / b away from every integer and the product is off by less than (a + 0.5) / b * 2^-21, i.e. by less than 0.5 / b for
// a < 2^20 (tests/cpp/edt_px.cpp tries every a < 4096 with every b <= 1024)
EDT_HD int edt_div_small(int a, float inv) { return (int)(((float)a + 0.5f) * inv); }
