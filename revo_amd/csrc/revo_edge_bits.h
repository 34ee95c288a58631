// The two places where an edge BITMAP (one word per 32 pixels of a row, bit x & 31 of word y * wpr + (x >> 5)) stands in for the
// byte plane edgesPyr {0,255}: the bit -> byte expansion of k_edge_bytes / k_hyst, and fillInEdges' per-pixel condition
// (imgpyramidrgbd.cpp:111-145, gate 188-195) as k_fill evaluates it.  Plain integer C++ that builds for the host and for the
// device: revo_pyramid.hip includes the very code tests/test_edge_bytes_cpu.py checks against the byte forms.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EB_HD __host__ __device__ __forceinline__
#else
#define EB_HD inline
#endif

// four pixels' bits (bit k = pixel k) -> four bytes {0,255}, pixel 0 in the lowest byte
EB_HD uint32_t edge_bits4_to_bytes(uint32_t bits4) { return (((bits4 & 0xfu) * 0x00204081u) & 0x01010101u) * 0xffu; }

// The 16 bytes of pixels p .. p + 15 of a level of width w (a multiple of 4; p = y * w + x a multiple of 16, p + 16 <= w * h),
// row-major, as four little-endian words.  word_at(i) is bitmap word i of the level (row y, word column c: i = y * wpr + c).  Where w is a
// multiple of 16 the group lies in one half of one word; otherwise it may wrap into the next row(s), four pixels at a time.
template <class WordAt>
EB_HD void edge_bytes16(WordAt word_at, int w, int wpr, int y, int x, uint32_t o[4]) {
  if ((w & 15) == 0) {
    const uint32_t bits = (word_at(y * wpr + (x >> 5)) >> (x & 31)) & 0xffffu;
    for (int q = 0; q < 4; ++q) o[q] = edge_bits4_to_bytes(bits >> (4 * q));
  } else {
    for (int q = 0; q < 4; ++q) {
      int xx = x + 4 * q, yy = y;
      while (xx >= w) { xx -= w; yy += 1; }
      o[q] = edge_bits4_to_bytes(word_at(yy * wpr + (xx >> 5)) >> (xx & 31));
    }
  }
}

// fillInEdges' gate of one (level, frame): the share of non-empty histogram tiles is below nPercentage (float, as the kernel has it)
EB_HD bool fill_gate_open(int hist_nz, int hist_w, int hist_h, float n_percentage) {
  return (float)hist_nz / (float)(hist_w * hist_h) < n_percentage;
}
// ... and behind an open gate, whether coarse pixel (y, x) of level l becomes an edge: its tile of level l's histogram (indexed
// with the FINER level's patch size, as the reference does) is sparse and the finer level has an edge at (2y+1, 2x+1).
// top_at(yy, xx) says whether that finer pixel is an edge: a byte test or a bit test.
template <class TopAt>
EB_HD bool fill_in_pixel(int y, int x, int finer_patch, int hist_w, int hist_h, const uint8_t* hist, double thr, TopAt top_at) {
  const int yy = 2 * y + 1, xx = 2 * x + 1;
  const int ty = yy / finer_patch, tx = xx / finer_patch;
  if (ty >= hist_h || tx >= hist_w) return false;
  return (double)hist[(size_t)ty * hist_w + tx] < thr && top_at(yy, xx);
}
// the bit test of both: pixel (y, x) of a bitmap with wpr words per row
template <class WordAt>
EB_HD bool edge_bit(WordAt word_at, int wpr, int y, int x) { return (word_at(y * wpr + (x >> 5)) >> (x & 31)) & 1u; }
