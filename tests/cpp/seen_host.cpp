// The arithmetic of the seen volume (revo_amd/csrc/revo_seen_host.h) over parameters, cells and bytes a test wrote: a plain C++
// program, no GPU.
// Input file: the voxel edge (float); the number of parameter sets (u32), then per set has_params (i32) and radius, accumulate
// (i32, u32), margin, margin_rel (2 floats); the number of cells (u32), then per cell lo and a (2 x i32); the number of byte
// updates (u32), then per update in, f, s (3 x u32); the number of questions (u32), then per question solid, byte, min_views
// (3 x u32) and the unknown neighbours (i32).
// Output file: per parameter set one byte (1 accepted) and, when accepted, the four effective parameters as stored; per cell the
// centre's coordinate (float); per update the byte; per question four bytes: free, known, unknown, frontier.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../revo_amd/csrc/revo_seen_host.h"

template <class T>
static bool rd(FILE* f, T* p, size_t n = 1) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
static bool wr(FILE* f, const T* p, size_t n = 1) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) return 2;
  float voxel = 0.0f;
  uint32_t n = 0;
  bool ok = rd(f, &voxel) && rd(f, &n) && n <= 4096;
  for (uint32_t i = 0; ok && i < n; ++i) {
    int32_t has = 0;
    revo_map_observe_params p{}, out{};
    ok = rd(f, &has) && rd(f, &p);
    if (!ok) break;
    const unsigned char good = seen_params_check(has ? &p : nullptr, voxel, &out) == nullptr;
    ok = wr(o, &good);
    if (good) ok = ok && wr(o, &out);
  }
  ok = ok && rd(f, &n) && n <= (1u << 20);
  for (uint32_t i = 0; ok && i < n; ++i) {
    int32_t c[2];
    ok = rd(f, c, 2);
    if (!ok) break;
    const float p = seen_centre(c[0], c[1], voxel);
    ok = wr(o, &p);
  }
  ok = ok && rd(f, &n) && n <= (1u << 20);
  for (uint32_t i = 0; ok && i < n; ++i) {
    uint32_t q[3];
    ok = rd(f, q, 3);
    if (!ok) break;
    const uint8_t b = seen_byte((uint8_t)q[0], q[1], q[2]);
    ok = wr(o, &b);
  }
  ok = ok && rd(f, &n) && n <= (1u << 20);
  for (uint32_t i = 0; ok && i < n; ++i) {
    uint32_t q[3];
    int32_t nb = 0;
    ok = rd(f, q, 3) && rd(f, &nb);
    if (!ok) break;
    const uint8_t b = (uint8_t)q[1];
    const unsigned char a[4] = {seen_is_free(b, q[2]), seen_is_known(b, q[2]), seen_is_unknown(q[0] != 0, b, q[2]),
                                seen_is_frontier(q[0] != 0, b, q[2], nb)};
    ok = wr(o, a, 4);
  }
  fclose(f);
  if (fclose(o) != 0) ok = false;
  return ok ? 0 : 1;
}
