// The per-pixel NMS decision of k_canny_nms4 (revo_amd/csrc/revo_nms_px.h), built for the host: the threshold form the kernel
// runs against the reference form, on both output bits.  Prints one line per case family and exits non-zero on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../revo_amd/csrc/revo_nms_px.h"

static const int MAXM = 2 * 1020 * 1020;  // 2 080 800: the largest |grad|^2
static unsigned long long g_cases = 0, g_bad = 0;

static inline uint32_t pack(int dx, int dy) { return ((uint32_t)dx & 0xffffu) | ((uint32_t)dy << 16); }

// one comparison: the 3x3 neighbourhood n[0..8] (rows a, b, c; n[4] is the centre), one gradient, one threshold pair
static inline void check(const int* n, uint32_t dxy, int low, int high) {
  bool rc, rs;
  nms_px_ref(n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], n[8], dxy, low, high, rc, rs);
  const NmsOut o = nms_px_thr(n[0], n[1], n[2], n[3], n[4], n[5] - 1, n[6], n[7] - 1, n[8], dxy, low, low > high ? low : high);
  const bool tc = (o.cand >> 31) != 0, ts = (o.strong >> 31) != 0;
  ++g_cases;
  if (tc != rc || ts != rs) {
    if (g_bad++ < 10)
      std::fprintf(stderr, "MISMATCH n = %d %d %d / %d %d %d / %d %d %d  dx %d dy %d  low %d high %d: reference %d%d threshold form %d%d\n",
                   n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7], n[8], (int)(int16_t)(dxy & 0xffffu), (int)(int16_t)(dxy >> 16), low, high,
                   (int)rc, (int)rs, (int)tc, (int)ts);
  }
}

// every 3x3 neighbourhood whose eight neighbours are drawn from {0, 1, 2, m - 1, m, m + 1, MAXM} (kept inside [0, MAXM]): all tie
// patterns, the zero of masked pixels, the largest magnitude; one gradient per direction class, threshold pairs around m
static void neighbourhoods() {
  static const int centres[] = {0, 1, 2, 3, 1000, MAXM - 1, MAXM};
  // horizontal, vertical, the two diagonals with either pair of signs
  static const int grads[][2] = {{900, 10}, {-7, 800}, {300, 300}, {-300, -300}, {300, -300}, {-300, 300}};
  for (int m : centres) {
    std::vector<int> vals;
    for (int v : {0, 1, 2, m - 1, m, m + 1, MAXM}) {
      if (v < 0 || v > MAXM) continue;
      bool seen = false;
      for (int u : vals) seen |= u == v;
      if (!seen) vals.push_back(v);
    }
    const int thr[][2] = {{0, 0}, {m - 1, m}, {m - 1, m - 1}, {m, m - 1}, {m - 1, m - 2}};  // 0, then <, ==, >, > around m
    const unsigned long long before = g_cases;
    const int V = (int)vals.size();
    static const int pos[8] = {0, 1, 2, 3, 5, 6, 7, 8};
    for (const auto& gr : grads) {
      const uint32_t dxy = pack(gr[0], gr[1]);
      for (const auto& t : thr) {
        int n[9], idx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 9; ++k) n[k] = vals[0];
        n[4] = m;
        for (;;) {
          check(n, dxy, t[0], t[1]);
          int k = 0;
          for (; k < 8; ++k) {  // the next neighbourhood, odometer fashion
            if (++idx[k] < V) { n[pos[k]] = vals[idx[k]]; break; }
            idx[k] = 0;
            n[pos[k]] = vals[0];
          }
          if (k == 8) break;
        }
      }
    }
    std::printf("neighbourhoods m = %d: %d values, %llu cases\n", m, V, g_cases - before);
  }
}

// every gradient of [-1020, 1020]^2 (so both sides of both tan 22.5 boundaries at every |dx|, all sign combinations, the zeros):
// the direction class itself, then the decision on a neighbourhood in which every direction has its own outcome
static void gradients() {
  const unsigned long long before = g_cases;
  unsigned long long dir_bad = 0;
  const int nb[2][9] = {{5, 9, 6, 9, 8, 8, 7, 7, 4}, {8, 7, 9, 8, 8, 6, 9, 8, 8}};
  for (int dy = -1020; dy <= 1020; ++dy)
    for (int dx = -1020; dx <= 1020; ++dx) {
      const uint32_t dxy = pack(dx, dy);
      const NmsDir a = nms_dir_ref(dxy), b = nms_dir(dxy);
      if (a.horiz != b.horiz || a.vert != b.vert || a.neg != b.neg) {
        if (dir_bad++ < 10) std::fprintf(stderr, "DIRECTION MISMATCH dx %d dy %d\n", dx, dy);
      }
      check(nb[0], dxy, 3, 7);
      check(nb[1], dxy, 7, 3);
    }
  g_bad += dir_bad;
  std::printf("gradients: 2041 x 2041 directions, %llu decisions\n", g_cases - before);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static inline uint32_t rnd() {  // splitmix64, seeded above
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

// 2 M seeded random cases: magnitudes from a narrow band (ties are common) or from the whole range, any gradient, thresholds in any order
static void random_cases() {
  const unsigned long long before = g_cases;
  for (int i = 0; i < 2000000; ++i) {
    int n[9];
    const uint32_t mode = rnd() % 3;
    const int base = (int)(rnd() % (uint32_t)(MAXM - 4));
    for (int k = 0; k < 9; ++k) n[k] = mode == 0 ? (int)(rnd() % 4) : mode == 1 ? base + (int)(rnd() % 4) : (int)(rnd() % (uint32_t)(MAXM + 1));
    if (rnd() % 8 == 0) n[rnd() % 9] = 0;
    const int dx = (int)(rnd() % 2041) - 1020, dy = (int)(rnd() % 2041) - 1020;
    int low, high;
    switch (rnd() % 4) {
      case 0: low = (int)(rnd() % (uint32_t)(MAXM + 1)); high = (int)(rnd() % (uint32_t)(MAXM + 1)); break;
      case 1: low = high = n[4] - (int)(rnd() % 3); break;
      case 2: low = n[4] - (int)(rnd() % 3); high = n[4] - (int)(rnd() % 3); break;
      default: low = 0; high = (int)(rnd() % 3) ? n[4] - 1 : 0; break;
    }
    check(n, pack(dx, dy), low, high);
  }
  std::printf("random: %llu cases\n", g_cases - before);
}

// the nibble the kernel assembles: pixel 3 is pushed first, so bit k is pixel k
static void push_order() {
  for (uint32_t bits = 0; bits < 16; ++bits) {
    uint32_t v[4];
    for (int k = 0; k < 4; ++k) v[k] = ((bits >> k) & 1u) ? 0x80000000u | rnd() : rnd() >> 1;
    const uint32_t w = nms_push(nms_push(nms_push(v[3] >> 31, v[2]), v[1]), v[0]);
    ++g_cases;
    if (w != bits) {
      ++g_bad;
      std::fprintf(stderr, "PUSH MISMATCH want %x got %x\n", bits, w);
    }
  }
}

int main() {
  neighbourhoods();
  gradients();
  random_cases();
  push_order();
  std::printf("cases %llu mismatches %llu\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
