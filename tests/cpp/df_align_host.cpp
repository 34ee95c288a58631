// The host arithmetic of revo_map_df_align (revo_amd/csrc/revo_align_host.h) over RECORDED records: a plain C++ program, no
// GPU.  Input file: centre (3 floats), T_init (16 floats, column-major), max_iters (i32), eps_t, eps_r (f64), min_matched (u64),
// the number of records (i32), then the records (208 bytes each) in the order the specification's loop evaluated them.  The
// evaluator hands out record i at call i and notes how far the pose the loop asks for lies from the pose record i was taken at.
// Output file: T_out (16 floats), iterations, status, calls (i32 each), the largest pose deviation (f64), then for the first
// record its H (36 f64) and g (6 f64).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../revo_amd/csrc/revo_align_host.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  float centre[3], T0[16];
  revo_map_align_opts o{};
  int32_t n = 0;
  bool ok = fread(centre, 4, 3, f) == 3 && fread(T0, 4, 16, f) == 16 && fread(&o.max_iters, 4, 1, f) == 1 &&
            fread(&o.eps_t, 8, 1, f) == 1 && fread(&o.eps_r, 8, 1, f) == 1 && fread(&o.min_matched, 8, 1, f) == 1 &&
            fread(&n, 4, 1, f) == 1 && n >= 1;
  std::vector<revo_map_df_align_info> recs(ok ? n : 0);
  ok = ok && fread(recs.data(), sizeof(revo_map_df_align_info), recs.size(), f) == recs.size();
  fclose(f);
  if (!ok) return 2;
  int calls = 0;
  double worst = 0.0;
  auto eval = [&](const float* Tf, revo_map_df_align_info* rec) {
    if (calls >= n) return 3;  // the loop evaluates more often than the specification did
    const revo_map_df_align_info& r = recs[calls++];
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < 3; ++i) worst = std::max(worst, std::fabs((double)Tf[4 * c + i] - (double)r.R[3 * c + i]));
    for (int i = 0; i < 3; ++i) worst = std::max(worst, std::fabs((double)Tf[12 + i] - (double)r.T[i]));
    *rec = r;
    return 0;
  };
  float T[16];
  revo_map_df_align_info last;
  int it = -1, st = -1;
  const int rc = align_loop_over<revo_map_df_align_info>(T0, centre, o, align_df_system_fill, eval, T, &last, &it, &st);
  if (rc) return 10 + rc;
  double H[36], g[6];
  align_df_system_fill(&recs[0], H, g);
  f = fopen(argv[2], "wb");
  if (!f) return 2;
  const int32_t tail[3] = {it, st, calls};
  fwrite(T, 4, 16, f); fwrite(tail, 4, 3, f); fwrite(&worst, 8, 1, f); fwrite(H, 8, 36, f); fwrite(g, 8, 6, f);
  fclose(f);
  return 0;
}
