// revo_info.hip -- the information matrix of tracked poses (gfx950): k_pair_info and the host-side covariance.
//
// k_track forms, at every accepted pose, the 6x6 normal equations of the edge alignment (calculateWarpUpdate + LGS6::update,
// optimizer.cpp:192-234, LGSX.h:392-398) and keeps nothing of them.  k_pair_info evaluates them once more at a GIVEN pose, for
// all pairs of a call in one launch, and writes the sums themselves (not divided by the point count): H = sum w v v^T (upper
// triangle), g = sum v (r w), sum w r^2, sum r^2 and the good / bad counts -- a revo_pair_info record per pair.
//
// The per-point code is the tracker's own (revo_track_dev.h: projection, 12-sample DT patch, gradients on the fly, the
// exact-sums terms), so the record is made of the terms the tracker summed.  Every sum is carried as a double-double (TwoSum,
// DESIGN 4.1) from the first addition on -- per thread, through the wave butterfly, LDS and the per-workgroup partials -- and
// rounded to float once: the float nearest the exact sum, whatever the grid shape.
//
// Grid (G, pairs): workgroup g of a pair takes the chunks g, g + G, ... of INFO_CHUNK points of the level's tile-ordered list.
// No workgroup waits for another: each publishes its 64-double partial and good count (write-through stores), draws a ticket
// from the pair's counter, and the one that draws G - 1 -- whoever arrives last -- adds the G partials in index order and
// writes the record.  A pair without points (or with more workgroups than chunks) publishes zeros: its record has good = 0.
// No dense contraction (a 6-vector outer product per point): no MFMA.
#include <cfloat>
#include <cmath>
#include <cstring>

#include "revo_internal.h"
#include "revo_track_dev.h"

namespace {

typedef unsigned long long u64;
typedef u64 __attribute__((address_space(1)))* gu64p;
typedef unsigned __attribute__((address_space(1)))* gu32p;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define INFO_WAVES (INFO_THREADS / 64)
// words of a revo_pair_info record
enum { W_GOOD = 29, W_BAD = 30, W_LEVEL = 31, W_FLAGS = 32, W_R = 33, W_T = 42, W_END = 48 };
static_assert(sizeof(revo_pair_info) == 4 * W_END && offsetof(revo_pair_info, good) == 4 * W_GOOD &&
              offsetof(revo_pair_info, flags) == 4 * W_FLAGS && offsetof(revo_pair_info, R) == 4 * W_R &&
              offsetof(revo_pair_info, T) == 4 * W_T, "record layout");
static_assert(XERR + 2 <= 32 && INFO_PART_DOUBLES == 64 && INFO_CHUNK % INFO_THREADS == 0, "partial layout");

// word `lane` of the record's tail (level, flags, R, T, reserved): selects, so that the pose stays in registers
__device__ __forceinline__ unsigned tail_word(int lane, int level, unsigned flags, const unsigned* Rb, const unsigned* Tb) {
  unsigned w = 0u;
  w = lane == W_LEVEL ? (unsigned)level : w;
  w = lane == W_FLAGS ? flags : w;
#pragma unroll
  for (int i = 0; i < 9; ++i) w = lane == W_R + i ? Rb[i] : w;
#pragma unroll
  for (int i = 0; i < 3; ++i) w = lane == W_T + i ? Tb[i] : w;
  return w;
}

__global__ void __launch_bounds__(INFO_THREADS) k_pair_info(const PairDesc* __restrict__ descs, const unsigned* pose, int pose_stride,
                                                            int flag_word, InfoParams prm, double* part, int* cnt,
                                                            unsigned* ticket, revo_pair_info* out) {
  __shared__ double s_h[INFO_WAVES][32], s_l[INFO_WAVES][32];
  __shared__ float s_c[INFO_WAVES];
  const int pair = blockIdx.y, grp = blockIdx.x, G = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned* const rec = (unsigned*)(out + pair);

  // the pose, read by this kernel with vector loads (the records may be what the grid in front of it on the stream just wrote)
  gu32p src = (gu32p)(pose + (size_t)pair * pose_stride);
  unsigned Rb[9], Tb[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) Rb[i] = __hip_atomic_load(src + i, RLX_AGENT);
#pragma unroll
  for (int i = 0; i < 3; ++i) Tb[i] = __hip_atomic_load(src + 9 + i, RLX_AGENT);
  const unsigned src_flags = __hip_atomic_load(src + flag_word, RLX_AGENT);
  float R[9], T[3];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) { R[i] = __uint_as_float(Rb[i]); finite = finite && __builtin_isfinite(R[i]); }
#pragma unroll
  for (int i = 0; i < 3; ++i) { T[i] = __uint_as_float(Tb[i]); finite = finite && __builtin_isfinite(T[i]); }
  if ((src_flags & 10u) != 0u || !finite || !is_orthogonal(R)) {  // no evaluation: the same for every workgroup of the pair
    if (grp == 0 && tid < W_END) rec[tid] = tail_word(tid, prm.level, 1u, Rb, Tb);
    return;
  }

  const PairDesc& d = descs[pair];
  int N = d.npts[prm.level];
  N = N < 0 ? 0 : (N > prm.w * prm.h ? prm.w * prm.h : N);  // the list's capacity
  gf4p pts = (gf4p)d.pts[prm.level];
  gf32p dtm = (gf32p)d.dt[prm.level];
  Cam cam;
  cam.fx = prm.fx; cam.fy = prm.fy; cam.cx = prm.cx; cam.cy = prm.cy;
  cam.w = prm.w; cam.h = prm.h;
  cam.wlim = (float)(cam.w - 2); cam.hlim = (float)(cam.h - 2);
  const bool filt = prm.use_edge_filter != 0;

  double xd[64];  // 32 double-double slots: heads, then tails (0..26 normal equations, XERR: sum w r^2, XERR + 1: sum r^2)
#pragma unroll
  for (int k = 0; k < 64; ++k) xd[k] = 0.0;
  float good = 0.0f;
  const int nchunks = (N + INFO_CHUNK - 1) / INFO_CHUNK;
  for (int ch = grp; ch < nchunks; ch += G) {
    const int end = (ch + 1) * INFO_CHUNK < N ? (ch + 1) * INFO_CHUNK : N;
#pragma unroll 1
    for (int i = ch * INFO_CHUNK + tid; i < end; i += INFO_THREADS)
      full_point<true>(pts[i], dtm, R, T, cam, prm.edge_distance, filt, prm.huber_edge, &good, xd);
  }
  reduce32x(xd, xd + 32, lane);  // lane L: the wave's total of slot idx32(L)
  good += lane_xor<1>(good); good += lane_xor<2>(good); good += lane_xor<4>(good);
  good += lane_xor<8>(good); good += lane_xor<16>(good); good += lane_xor<32>(good);  // exact: < 2^24
  if (lane < 32) { s_h[wave][idx32(lane)] = xd[0]; s_l[wave][idx32(lane)] = xd[32]; }
  if (lane == 0) s_c[wave] = good;
  __syncthreads();
  if (wave != 0) return;

  // wave 0: the workgroup's partial (waves in index order), published write-through, then the ticket
  const int k = lane & 31;
  double h = s_h[0][k], l = s_l[0][k];
  float c = s_c[0];
#pragma unroll
  for (int w = 1; w < INFO_WAVES; ++w) { dd_add(h, l, s_h[w][k], s_l[w][k]); c += s_c[w]; }
  gu64p mine = (gu64p)(part + ((size_t)pair * INFO_MAX_GROUPS + grp) * INFO_PART_DOUBLES);
  if (lane < 32) {
    __hip_atomic_store(mine + k, (u64)__double_as_longlong(h), RLX_AGENT);
    __hip_atomic_store(mine + 32 + k, (u64)__double_as_longlong(l), RLX_AGENT);
  }
  gu32p cnts = (gu32p)(cnt + (size_t)pair * INFO_MAX_GROUPS);
  if (lane == 0) __hip_atomic_store(cnts + grp, (unsigned)(int)c, RLX_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial has left this CU before the ticket is drawn
  unsigned drawn = 0u;
  if (lane == 0) drawn = __hip_atomic_fetch_add((gu32p)(ticket + pair), 1u, RLX_AGENT);
  drawn = (unsigned)__builtin_amdgcn_readfirstlane((int)drawn);
  if (drawn != (unsigned)(G - 1)) return;

  // the last workgroup of the pair to arrive: every partial is published; add them in index order
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  gu64p all = (gu64p)(part + (size_t)pair * INFO_MAX_GROUPS * INFO_PART_DOUBLES);
  h = 0.0; l = 0.0;
  int n_good = 0;
  for (int g = 0; g < G; ++g) {
    const double gh = __longlong_as_double((long long)__hip_atomic_load(all + (size_t)g * INFO_PART_DOUBLES + k, RLX_AGENT));
    const double gl = __longlong_as_double((long long)__hip_atomic_load(all + (size_t)g * INFO_PART_DOUBLES + 32 + k, RLX_AGENT));
    dd_add(h, l, gh, gl);
    n_good += (int)__hip_atomic_load(cnts + g, RLX_AGENT);
  }
  const float f = dd_to_float(h, l);
  unsigned w = tail_word(lane, prm.level, 0u, Rb, Tb);
  w = lane < XERR + 2 ? __float_as_uint(f) : w;
  w = lane == W_GOOD ? (unsigned)n_good : w;
  w = lane == W_BAD ? (unsigned)(N - n_good) : w;
  if (lane < W_END) rec[lane] = w;
}

}  // namespace

void launch_pair_info(const PairDesc* d_descs, const void* d_pose, int pose_stride, int flag_word, const InfoParams& prm,
                      int n_pairs, double* d_part, int* d_cnt, unsigned* d_ticket, revo_pair_info* d_out, hipStream_t s) {
  // the tickets are counted within the call: zeroed in front of every launch (a block of its own, padded to 16 bytes)
  (void)hipMemsetAsync(d_ticket, 0, ((size_t)n_pairs * sizeof(unsigned) + 15) / 16 * 16, s);
  const dim3 grid((unsigned)info_groups(prm.w * prm.h), (unsigned)n_pairs);
  hipLaunchKernelGGL(k_pair_info, grid, dim3(INFO_THREADS), 0, s, d_descs, (const unsigned*)d_pose, pose_stride, flag_word, prm,
                     d_part, d_cnt, d_ticket, d_out);
}

// cov = sigma2 * H^-1, sigma2 = sum_w / (good - 6): host only, double Cholesky
extern "C" int revo_pair_info_covariance(const revo_pair_info* info, double cov[36], double* sigma2) {
  if (!info || !cov) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (info->flags & 1) return fail(REVO_ERR_INVALID_ARG, "the record carries no evaluation (flags bit0)");
  if (info->good <= 6) return fail(REVO_ERR_INVALID_ARG, "not more good points than unknowns");
  double A[6][6], L[6][6] = {};
  for (int a = 0, k = 0; a < 6; ++a)
    for (int c = a; c < 6; ++c, ++k) A[a][c] = A[c][a] = (double)info->H[k];
  for (int j = 0; j < 6; ++j) {
    double p = A[j][j];
    for (int k = 0; k < j; ++k) p -= L[j][k] * L[j][k];
    if (!(p > 64.0 * DBL_EPSILON * A[j][j]) || !std::isfinite(p))
      return fail(REVO_ERR_INVALID_ARG, "the information matrix is not positive definite (rank-deficient system)");
    L[j][j] = std::sqrt(p);
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  double X[6][6];  // H^-1, column by column: L y = e_c, L^T x = y
  for (int c = 0; c < 6; ++c) {
    double y[6];
    for (int i = 0; i < 6; ++i) {
      double v = i == c ? 1.0 : 0.0;
      for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
      y[i] = v / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
      double v = y[i];
      for (int k = i + 1; k < 6; ++k) v -= L[k][i] * X[k][c];
      X[i][c] = v / L[i][i];
    }
  }
  const double s2 = (double)info->sum_w / (double)(info->good - 6);
  for (int a = 0; a < 6; ++a)
    for (int c = 0; c < 6; ++c) cov[a * 6 + c] = s2 * (0.5 * (X[a][c] + X[c][a]));
  if (sigma2) *sigma2 = s2;
  return REVO_OK;
}
