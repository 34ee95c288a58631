// The arithmetic of the TSDF volume and its mesh (revo_amd/csrc/revo_tsdf_host.h) over parameters, depths and cells a test wrote,
// and the header's tables against the rules they stand for: a plain C++ program, no GPU.
// Input file: the voxel edge (float); the number of parameter sets (u32), then per set has_params (i32), trunc (float), accumulate
// and two reserved words (3 x u32); the number of quanta (u32), then per quantum dc, z, trunc (3 floats); the number of edges
// (u32), then per edge s0 (i32), w0 (u32), s1 (i32), w1 (u32); the number of updates (u32), then per update sum (i32), weight
// (u32), q (i32).
// Output (text, one record per line): "param good truncbits accumulate"; "q value"; "alpha bits"; "update dropped sum weight";
// "swap k word" -- the header's table -- and "geo k word" -- the same word from the geometric rule, decided here at the edge
// midpoints in integers; "tri code j packed"; "own t mask" -- bit o: the header says the edge of type t at a cell belongs to the
// cube at cell - o -- and "chain t mask" -- the same from the tetrahedra's corners; "corner k c0 c1 c2 c3".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../revo_amd/csrc/revo_tsdf_host.h"

template <class T>
static bool rd(FILE* f, T* p, size_t n = 1) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static void offset(unsigned v, long o[3]) { o[0] = v & 1u; o[1] = (v >> 1) & 1u; o[2] = (v >> 2) & 1u; }

// Whether the triangle (three packed edges of the tetrahedron k), taken at twice the edges' midpoints, has its normal pointing
// from the inside corners (the bits of code) to the outside corners: all integers.
static int outward(int k, unsigned code, unsigned tri) {
  long p[3][3];
  for (int q = 0; q < 3; ++q) {
    const unsigned e = (tri >> (4 * q)) & 15u;
    long a[3], b[3];
    offset(tsdf_tetra_corner(k, (int)(e & 3u)), a);
    offset(tsdf_tetra_corner(k, (int)(e >> 2)), b);
    for (int i = 0; i < 3; ++i) p[q][i] = a[i] + b[i];
  }
  long u[3], v[3];
  for (int i = 0; i < 3; ++i) { u[i] = p[1][i] - p[0][i]; v[i] = p[2][i] - p[0][i]; }
  const long nrm[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  long in[3] = {0, 0, 0}, out[3] = {0, 0, 0}, nin = 0;
  for (int i = 0; i < 4; ++i) {
    long c[3];
    offset(tsdf_tetra_corner(k, i), c);
    const bool inside = (code >> i) & 1u;
    nin += inside;
    for (int d = 0; d < 3; ++d) (inside ? in : out)[d] += c[d];
  }
  long dot = 0;  // (out / (4 - nin) - in / nin) . nrm, times nin (4 - nin) > 0
  for (int d = 0; d < 3; ++d) dot += nrm[d] * (out[d] * nin - in[d] * (4 - nin));
  return dot > 0 ? 1 : (dot < 0 ? 0 : -1);
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  float voxel = 0.0f;
  uint32_t n = 0;
  bool ok = rd(f, &voxel) && rd(f, &n) && n <= 4096;
  for (uint32_t i = 0; ok && i < n; ++i) {
    int32_t has = 0;
    revo_map_tsdf_params p{}, out{};
    ok = rd(f, &has) && rd(f, &p);
    if (!ok) break;
    const int good = tsdf_params_check(has ? &p : nullptr, voxel, &out) == nullptr;
    uint32_t bits = 0;
    memcpy(&bits, &out.trunc, 4);
    printf("param %d %u %u\n", good, good ? bits : 0u, good ? out.accumulate : 0u);
  }
  ok = ok && rd(f, &n) && n <= (1u << 20);
  for (uint32_t i = 0; ok && i < n; ++i) {
    float v[3];
    ok = rd(f, v, 3);
    if (ok) printf("q %d\n", (int)tsdf_quantum(v[0], v[1], v[2]));
  }
  ok = ok && rd(f, &n) && n <= (1u << 20);
  for (uint32_t i = 0; ok && i < n; ++i) {
    int32_t s0 = 0, s1 = 0;
    uint32_t w0 = 0, w1 = 0;
    ok = rd(f, &s0) && rd(f, &w0) && rd(f, &s1) && rd(f, &w1);
    if (!ok) break;
    const float a = tsdf_edge_alpha(s0, w0, s1, w1);
    uint32_t bits = 0;
    memcpy(&bits, &a, 4);
    printf("alpha %u\n", bits);
  }
  ok = ok && rd(f, &n) && n <= (1u << 20);
  for (uint32_t i = 0; ok && i < n; ++i) {
    int32_t sum = 0, q = 0;
    uint32_t weight = 0;
    ok = rd(f, &sum) && rd(f, &weight) && rd(f, &q);
    if (!ok) break;
    const unsigned dropped = tsdf_update(sum, weight, q);
    printf("update %u %d %u\n", dropped, (int)sum, weight);
  }
  fclose(f);
  if (!ok) return 1;
  for (int k = 0; k < 6; ++k) {
    unsigned geo = 0;
    for (unsigned code = 1; code < 15; ++code)
      for (int j = 0; j < tsdf_case_count(code); ++j) {
        const unsigned tri = tsdf_case_triangle(code, j);
        printf("tri %u %d %u\n", code, j, tri);
        const int o = outward(k, code, tri);
        if (o < 0) return 3;  // a triangle on edge: the rule would not decide
        if (j == 0) geo |= (o ? 0u : 1u) << code;
        else if (((geo >> code) & 1u) != (o ? 0u : 1u)) return 4;  // the two triangles of a quad turn the same way
      }
    printf("swap %d %u\ngeo %d %u\n", k, tsdf_swap_word(k), k, geo);
    printf("corner %d %u %u %u %u\n", k, tsdf_tetra_corner(k, 0), tsdf_tetra_corner(k, 1), tsdf_tetra_corner(k, 2), tsdf_tetra_corner(k, 3));
  }
  for (unsigned t = 0; t < 7; ++t) {
    unsigned own = 0, chain = 0;
    const unsigned d = t + 1u;
    for (unsigned o = 0; o < 8; ++o) {
      own |= tsdf_edge_in_cube(t, o) ? 1u << o : 0u;
      // in the cube at cell - o the edge runs from the corner o to the corner o + d, if that is a corner at all
      if (o & d) continue;
      for (int k = 0; k < 6; ++k) {
        bool has_lo = false, has_hi = false;
        for (int i = 0; i < 4; ++i) {
          has_lo = has_lo || tsdf_tetra_corner(k, i) == o;
          has_hi = has_hi || tsdf_tetra_corner(k, i) == (o | d);
        }
        if (has_lo && has_hi && tsdf_edge_type(o, o | d) == t) chain |= 1u << o;
      }
    }
    printf("own %u %u\nchain %u %u\n", t, own, t, chain);
  }
  return 0;
}
