// The per-lane search of the EDT row pass (revo_amd/csrc/revo_edt_px.h, the header k_edt_rows includes), built for the host,
// against a brute-force  min_x' (x - x')^2 + g2(x')  per row, as integers.  The rows are laid out as the kernel lays them out:
// [pad INF][w values g2][pad INF], pad = w + 4, filled from 16-bit column distances with the kernel's 0xffff -> INF rule, in a
// buffer with guard words on both sides that must never be read as data (they hold a value that would win every minimum).
// Also: edt_sqrt_rn_int against the correctly rounded root (double sqrt, rounded once: exact for integers below 2^24) for every
// `best` the cases produce, from estimates one ulp to either side of it as well; and edt_div_small against the integer division
// for every operand pair of its range.  Prints one line per case family, the first differing case, and exits non-zero on any.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../../revo_amd/csrc/revo_edt_px.h"

static long g_cases = 0, g_fail = 0;
static std::set<int> g_best;  // every finite minimum seen

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static const int GUARD = 8;         // words on either side of the row that the search must not touch
static const int POISON = -(1 << 30);  // read as data it would be the minimum of everything

// one row of 16-bit column distances (0xffff = no edge in the column) through the header's search, against brute force
static bool check_row(const std::vector<uint16_t>& d16, const char* what) {
  const int w = (int)d16.size();
  const int pad = w + 4, pitch = w + 2 * pad;
  std::vector<edt_quad> store((pitch + 2 * GUARD) / 4);
  int* buf = reinterpret_cast<int*>(store.data());
  for (int i = 0; i < pitch + 2 * GUARD; ++i) buf[i] = POISON;
  int* lds = buf + GUARD;
  for (int i = 0; i < pad; ++i) { lds[i] = EDT_INF; lds[pad + w + i] = EDT_INF; }
  for (int x = 0; x < w; ++x) lds[pad + x] = edt_g2(d16[x]);
  std::vector<int> g2(w);
  for (int x = 0; x < w; ++x) g2[x] = d16[x] == 0xffff ? EDT_INF : (int)d16[x] * (int)d16[x];
  // brute force, as 64-bit integers; nothing finite -> INF
  std::vector<int> want(w), finite;
  for (int xp = 0; xp < w; ++xp)
    if (g2[xp] < EDT_INF) finite.push_back(xp);
  for (int x = 0; x < w; ++x) {
    long long m = EDT_INF;
    for (int xp : finite) { const long long v = (long long)(x - xp) * (x - xp) + g2[xp]; if (v < m) m = v; }
    want[x] = (int)m;
  }
  ++g_cases;
  for (int q = 0; q < w / 4; ++q) {
    int best[4];
    edt_search4(lds + pad, q, w, best);
    for (int i = 0; i < 4; ++i) {
      const int x = 4 * q + i;
      const int got = best[i] >= EDT_INF ? EDT_INF : best[i];  // the kernel only asks `best >= EDT_INF`
      if (got != want[x]) {
        if (!g_fail++) {
          printf("DIFFERENT %s: w %d x %d: search %d, brute force %d\n  d16:", what, w, x, best[i], want[x]);
          for (int k = 0; k < w && k < 64; ++k) printf(" %d", d16[k]);
          printf("%s\n", w > 64 ? " ..." : "");
        }
        return false;
      }
      if (got < EDT_INF) g_best.insert(got);
      const float dt = edt_dt(best[i]);
      const float dt_want = want[x] >= EDT_INF ? sqrtf(1e15f) : (float)sqrt((double)want[x]);
      if (memcmp(&dt, &dt_want, 4) != 0) {
        if (!g_fail++) printf("DIFFERENT %s: w %d x %d: edt_dt(%d) = %.9g, expected %.9g\n", what, w, x, best[i], dt, dt_want);
        return false;
      }
    }
  }
  return true;
}

static const int WIDTHS[] = {4, 8, 12, 36, 80, 160, 640, 2048};

int main() {
  // ---- the fill's rule --------------------------------------------------------------------------------------------------
  if (edt_g2(0xffff) != EDT_INF || edt_g2(0) != 0 || edt_g2(1) != 1 || edt_g2(2047) != 2047 * 2047 ||
      (long long)EDT_INF + 2047ll * 2047ll >= (1ll << 31)) {
    printf("DIFFERENT: edt_g2 / EDT_INF\n");
    return 1;
  }
  long before = g_cases;
  for (int w : WIDTHS) {
    std::vector<uint16_t> d(w, 0xffff);
    check_row(d, "all INF");
    // one finite column: at x = 0, w-1, each position of a quad (first, a middle and the last quad), column distances 0, 1, 2047
    std::vector<int> xs = {0, 1, 2, 3, w - 4, w - 3, w - 2, w - 1};
    const int mid = (w / 8) * 4;
    for (int i = 0; i < 4; ++i) xs.push_back(mid + i);
    for (int x : xs)
      for (int dist : {0, 1, 2047}) {
        std::fill(d.begin(), d.end(), (uint16_t)0xffff);
        d[x] = (uint16_t)dist;
        check_row(d, "one finite column");
      }
    // finite columns only in the first or only in the last quad: the far end searches to d = w - 1 and into the padding
    for (int side = 0; side < 2; ++side)
      for (unsigned mask = 1; mask < 16; ++mask)
        for (int dist : {0, 1, 2047}) {
          std::fill(d.begin(), d.end(), (uint16_t)0xffff);
          for (int i = 0; i < 4; ++i)
            if (mask >> i & 1) d[(side ? w - 4 : 0) + i] = (uint16_t)(dist + (dist == 1 ? i : 0));
          check_row(d, "first / last quad only");
        }
    // all finite: 0 everywhere, 2047 everywhere, one 0 in a row of 2047 (the search runs far although every column is finite)
    std::fill(d.begin(), d.end(), (uint16_t)0); check_row(d, "all 0");
    std::fill(d.begin(), d.end(), (uint16_t)2047); check_row(d, "all 2047");
    d[0] = 0; check_row(d, "2047 and one 0");
    d[0] = 2047; d[w - 1] = 0; check_row(d, "2047 and one 0");
  }
  printf("edges of the layout: %ld rows (all INF, one finite column at x = 0, w-1 and every quad position, first / last quad only, "
         "column distances 0, 1, 2047)\n", g_cases - before);

  // ---- random rows: densities from one finite column per row to all finite, small and large column distances -------------
  before = g_cases;
  const long N_RANDOM = 200000;
  for (long n = 0; n < N_RANDOM && !g_fail; ++n) {
    // the wide rows are the expensive ones for the brute force: most rows are narrow, every width gets its share
    const uint32_t pick = rnd() % 1000;
    const int w = pick < 2 ? 2048 : pick < 12 ? 640 : pick < 62 ? 160 : pick < 262 ? 80 : WIDTHS[rnd() % 4];
    std::vector<uint16_t> d(w, 0xffff);
    const uint32_t kind = rnd() % 8;
    const int maxd = (rnd() & 1) ? 2047 : ((rnd() & 1) ? 40 : 4);
    if (kind == 0) {
      d[rnd() % w] = (uint16_t)(rnd() % (maxd + 1));
    } else if (kind == 7) {
      for (int x = 0; x < w; ++x) d[x] = (uint16_t)(rnd() % (maxd + 1));
    } else {
      // each column finite with probability 2^-kind .. and at least one
      const uint32_t thr = 1u << (2 * kind);  // 1/4 .. 1/4096
      for (int x = 0; x < w; ++x)
        if (rnd() % thr == 0) d[x] = (uint16_t)(rnd() % (maxd + 1));
      d[rnd() % w] = (uint16_t)(rnd() % (maxd + 1));
    }
    check_row(d, "random");
  }
  printf("random: %ld rows\n", g_cases - before);

  // ---- the root: correctly rounded for every minimum seen, from the estimate itself and from one ulp to either side ----------
  long roots = 0;
  for (int b : g_best) {
    const float x = (float)b;
    if ((int)x != b || b >= (1 << 24)) { printf("DIFFERENT: minimum %d is not an integer-valued float below 2^24\n", b); ++g_fail; break; }
    const float want = (float)sqrt((double)b);  // the double root of an integer < 2^24 rounds to float like the exact root
    const float s = sqrtf(x);
    float cand[3] = {s, nextafterf(s, 0.0f), nextafterf(s, INFINITY)};
    const int nc = b == 0 ? 1 : 3;  // the root of 0 is exact in hardware too
    for (int k = 0; k < nc; ++k) {
      const float got = edt_sqrt_fix(x, cand[k]);
      ++roots;
      if (memcmp(&got, &want, 4) != 0) {
        if (!g_fail++) printf("DIFFERENT: edt_sqrt_fix(%d, estimate %.9g) = %.9g, correctly rounded %.9g\n", b, cand[k], got, want);
        break;
      }
    }
    if (g_fail) break;
  }
  printf("roots: %zu distinct minima, %ld corrections\n", g_best.size(), roots);

  // ---- the group index without a division --------------------------------------------------------------------------------
  long divs = 0;
  for (int b = 1; b <= 1024 && !g_fail; ++b) {
    const float inv = 1.0f / (float)b;
    uint32_t bits;
    memcpy(&bits, &inv, 4);
    for (int e = -2; e <= 2; ++e) {
      const uint32_t eb = bits + (uint32_t)e;
      float iv;
      memcpy(&iv, &eb, 4);
      for (int a = 0; a < 4096; ++a, ++divs)
        if (edt_div_small(a, iv) != a / b) {
          if (!g_fail++) printf("DIFFERENT: edt_div_small(%d, 1/%d %+d ulp) = %d\n", a, b, e, edt_div_small(a, iv));
          break;
        }
    }
  }
  printf("divisions: %ld\n", divs);
  printf("cases %ld different %ld\n", g_cases, g_fail);
  return g_fail ? 1 : 0;
}
