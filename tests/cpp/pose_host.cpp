// The host arithmetic of revo_map_pose_raw (revo_amd/csrc/revo_pose_host.h) over records a test wrote: a plain C++ program, no GPU.
// Input file: the number of poses (u32), the poses (16 floats each, column-major), the number of records (u64), the records
// (64 bytes each) in any order, keys may repeat.
// Output file: per pose one byte (bit0 finite, bit1 orthogonal), the number of canonical records (u64), then those records.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../revo_amd/csrc/revo_pose_host.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t np = 0;
  uint64_t n = 0;
  bool ok = fread(&np, 4, 1, f) == 1 && np <= 1024;
  std::vector<float> poses(ok ? 16 * (size_t)np : 0);
  ok = ok && (poses.empty() || fread(poses.data(), 4, poses.size(), f) == poses.size()) && fread(&n, 8, 1, f) == 1 && n <= (1u << 24);
  std::vector<revo_map_voxel_raw> rec(ok ? (size_t)n : 0);
  ok = ok && (rec.empty() || fread(rec.data(), sizeof(revo_map_voxel_raw), rec.size(), f) == rec.size());
  fclose(f);
  if (!ok) return 2;
  std::vector<unsigned char> flags(np);
  for (uint32_t i = 0; i < np; ++i) {
    const float* T = poses.data() + 16 * (size_t)i;
    flags[i] = (unsigned char)((pose_is_finite(T) ? 1 : 0) | (pose_is_finite(T) && pose_is_orthogonal(T) ? 2 : 0));
  }
  const uint64_t m = pose_canonicalise(rec.data(), rec.size());
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  ok = fwrite(flags.data(), 1, flags.size(), o) == flags.size() && fwrite(&m, 8, 1, o) == 1 &&
       (m == 0 || fwrite(rec.data(), sizeof(revo_map_voxel_raw), (size_t)m, o) == (size_t)m);
  return fclose(o) == 0 && ok ? 0 : 2;
}
