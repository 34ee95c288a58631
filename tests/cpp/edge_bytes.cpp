// The bitmap forms of revo_amd/csrc/revo_edge_bits.h, built for the host, against the byte forms they replace: the bit -> byte
// expansion of k_edge_bytes against a per-pixel expansion, and k_fill's condition on the finer level's bitmap against the
// same condition on its byte plane (the kernel's former loop, written out below).  Prints one line per case family and exits
// non-zero on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../revo_amd/csrc/revo_edge_bits.h"

static unsigned long long g_cases = 0, g_bad = 0;
static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static inline uint32_t rnd() {  // xorshift64*
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545f4914f6cdd1dull) >> 32);
}

// a random w x h byte plane {0,255} of the given density (per 256) and its bitmap; the bits beyond w in the last word of a row
// are garbage on purpose: nothing may read them
static void random_plane(int w, int h, int density, std::vector<uint8_t>& bytes, std::vector<uint32_t>& bits) {
  const int wpr = (w + 31) / 32;
  bytes.assign((size_t)w * h, 0);
  bits.assign((size_t)wpr * h, 0u);
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < w; ++x)
      if ((int)(rnd() & 255u) < density) { bytes[(size_t)y * w + x] = 255; bits[(size_t)y * wpr + (x >> 5)] |= 1u << (x & 31); }
    if (w & 31) bits[(size_t)y * wpr + wpr - 1] |= rnd() << (w & 31);
  }
}

// ---- the expansion: every 16-pixel group of a plane
static void check_expand(int w, int h, int density) {
  std::vector<uint8_t> bytes; std::vector<uint32_t> bits;
  random_plane(w, h, density, bytes, bits);
  const int wpr = (w + 31) / 32;
  for (int p = 0; p + 16 <= w * h; p += 16) {
    const int y = p / w, x = p - y * w;
    uint32_t o[4];
    edge_bytes16([&](int k) { return bits[(size_t)k]; }, w, wpr, y, x, o);
    for (int k = 0; k < 16; ++k) {
      const uint8_t got = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
      ++g_cases;
      if (got != bytes[(size_t)p + k] && g_bad++ < 10)
        std::fprintf(stderr, "MISMATCH expand w %d h %d pixel %d: %d, bytes have %d\n", w, h, p + k, (int)got, (int)bytes[(size_t)p + k]);
    }
  }
}

// ---- fill-in of one (level, frame): finer level fw x fh, coarse level fw/2 x fh/2
static void check_fill(int fw, int fh, int finer_patch, int patch, int density, int gate /*0 closed, 1 open, 2 as the counts say*/) {
  std::vector<uint8_t> top; std::vector<uint32_t> topbits;
  random_plane(fw, fh, density, top, topbits);
  const int w = fw / 2, h = fh / 2, wpr = (w + 31) / 32, fwpr = (fw + 31) / 32;
  std::vector<uint8_t> mod; std::vector<uint32_t> modbits;
  random_plane(w, h, density / 4, mod, modbits);
  const int hist_w = w / patch, hist_h = h / patch;
  std::vector<uint8_t> hist((size_t)hist_w * hist_h);
  int nz = 0;
  for (auto& v : hist) { v = (rnd() & 3u) ? (uint8_t)(rnd() % 4u) : (uint8_t)(rnd() & 255u); nz += v != 0; }
  const double thr = (double)(patch * patch) * 0.05;
  const float frac = (float)nz / (float)(hist_w * hist_h);
  const float n_percentage = gate == 0 ? 0.0f : (gate == 1 ? 2.0f : 0.5f);
  // the byte form: k_fill's loop as it read the finer level's byte plane
  std::vector<uint8_t> want = mod;
  if (frac < n_percentage) {
    const int cw = fw / 2, ch = fh / 2;
    for (int i = 0; i < cw * ch; ++i) {
      const int y = i / cw, x = i % cw;
      const int yy = 2 * y + 1, xx = 2 * x + 1;
      const int ty = yy / finer_patch, tx = xx / finer_patch;
      if (ty >= hist_h || tx >= hist_w) continue;
      if ((double)hist[(size_t)ty * hist_w + tx] < thr && top[(size_t)yy * fw + xx] > 0) want[(size_t)y * w + x] = 255;
    }
  }
  // the bitmap form
  std::vector<uint32_t> got = modbits;
  if (fill_gate_open(nz, hist_w, hist_h, n_percentage)) {
    const int cw = fw / 2, ch = fh / 2;
    for (int i = 0; i < cw * ch; ++i) {
      const int y = i / cw, x = i % cw;
      if (fill_in_pixel(y, x, finer_patch, hist_w, hist_h, hist.data(), thr, [&](int yy, int xx) {
            return edge_bit([&](int k) { return topbits[(size_t)k]; }, fwpr, yy, xx); }))
        got[(size_t)y * wpr + (x >> 5)] |= 1u << (x & 31);
    }
  }
  int added = 0;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const bool b = edge_bit([&](int k) { return got[(size_t)k]; }, wpr, y, x);
      added += b && !mod[(size_t)y * w + x];
      ++g_cases;
      if (b != (want[(size_t)y * w + x] > 0) && g_bad++ < 10)
        std::fprintf(stderr, "MISMATCH fill fw %d fh %d gate %d pixel (%d, %d): bit %d, byte %d\n", fw, fh, gate, y, x, (int)b, (int)want[(size_t)y * w + x]);
    }
  if (gate == 0 && added) { ++g_bad; std::fprintf(stderr, "a closed gate added %d pixels\n", added); }
  if (gate == 1 && !added && density >= 64) { ++g_bad; std::fprintf(stderr, "an open gate added nothing (fw %d)\n", fw); }
}

int main() {
  const int widths[4] = {80, 96, 100, 160};
  unsigned long long before = g_cases;
  for (int w : widths)
    for (int h : {4, 12, 60})
      for (int density : {0, 1, 20, 128, 255, 256})
        for (int rep = 0; rep < 8; ++rep) check_expand(w, h, density);
  std::printf("expand: %llu pixels over widths 80 96 100 160\n", g_cases - before);
  before = g_cases;
  for (int fw : widths)
    for (int gate : {0, 1, 2})
      for (int density : {8, 64, 200})
        for (int rep = 0; rep < 16; ++rep) {
          check_fill(fw, 60, 10, 5, density, gate);   // the reference's patch ladder
          check_fill(fw, 64, 5, 5, density, gate);    // equal patches: tiles beyond the histogram are skipped
        }
  std::printf("fill: %llu pixels, gate closed / open / by the counts\n", g_cases - before);
  std::printf("cases %llu bad %llu\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
