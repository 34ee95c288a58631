// revo_tsdf_ray_dev.h -- the device bodies of the surface ray cast that revo_map_tsdf_ray.hip and
// revo_map_tsdf_ray_many.hip share, each written once: what one thread of the mask launch does with its cell, and what
// one block of the march launch does with its 32 x 8 pixels of a view.  The march and every rule of it are revo_tsdf_ray_host.h's;
// the kernels that call these say only where a block's volume, view and counter line come from.  Internal.
#pragma once
#include "revo_map_impl.h"
#include "revo_tsdf_ray_host.h"

struct TsdfRayView {  // one view of a launch, in device memory
  RayView v;
  float* depth; float* normal; uint8_t* bgr; unsigned* hits;  // normal, bgr: NULL when not asked for
};
enum { TR_RAYS = 0, TR_STATUS = 1, TR_SAMPLES = 5, TR_UNCOLORED = 6 };

// The cell c (< cells) of a volume: an INSIDE cell is a corner of the sample bases cell - {0, 1}^3 (those inside 0 .. n - 2), and
// marks the block of each.  A bit only ever goes from 0 to 1 during the launch, so a bit that a load finds set needs no atomic,
// and the mask is the same whatever the order: integer atomicOr only.
__device__ __forceinline__ void tsdf_ray_mask_cell(const revo_map_tsdf_cell* __restrict__ tsdf, const revo_map_df_box& box, unsigned c, unsigned min_weight,
                                                   int nby, int nbz, unsigned* mask) {
  const revo_map_tsdf_cell v = tsdf[c];
  if (!tsdf_inside(v.sum, v.weight, min_weight)) return;
  const unsigned ny = (unsigned)box.n[1], nz = (unsigned)box.n[2];
  const unsigned line = c / nz;
  const int iz = (int)(c - line * nz), ix = (int)(line / ny), iy = (int)(line - (unsigned)ix * ny);
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    const int bx = ix - (o & 1), by = iy - ((o >> 1) & 1), bz = iz - ((o >> 2) & 1);
    if (bx < 0 || bx > box.n[0] - 2 || by < 0 || by > box.n[1] - 2 || bz < 0 || bz > box.n[2] - 2) continue;
    const unsigned blk = tsdf_ray_block(nby, nbz, bx, by, bz), bit = 1u << (blk & 31u);
    if (!(__hip_atomic_load(&mask[blk >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(&mask[blk >> 5], bit);
  }
}

// The LDS counters of a march block.
struct TsdfRayTally {
  unsigned cnt[TSDF_RAY_STATUSES];
  unsigned unc;
  u64 samples;
};

// One block of 256 threads over the view vw: one thread per pixel.  A wave is an 8 x 8 pixel tile, so neighbouring rays read
// neighbouring cells and end after similar numbers of samples; a block is four tiles side by side.  blk: the block's number in
// the view, below its tiles (the caller has sent blocks past them away).  The statuses of a wave are counted by ballots, its
// samples and uncoloured hits by a wave sum, each into LDS with one atomic per wave; every counter takes one global atomic per
// block, into the line `info` and the view's hit word.
__device__ __forceinline__ void tsdf_ray_view_block(const TsdfRayK& a, const TsdfRayView& vw, unsigned blk, TsdfRayTally& s, u64* info) {
  const RayView& c = vw.v;
  const unsigned bw = (unsigned)(c.w + 31) / 32;
  if (threadIdx.x < TSDF_RAY_STATUSES) s.cnt[threadIdx.x] = 0;
  if (threadIdx.x == 4) s.samples = 0;
  if (threadIdx.x == 5) s.unc = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int x = (int)((blk % bw) * 32 + (threadIdx.x >> 6) * 8 + (lane & 7));
  const int y = (int)((blk / bw) * 8 + (lane >> 3));
  int status = -1;
  TsdfRayOut o{};
  if (x < c.w && y < c.h) {
    const float dcx = tsdf_div((float)x - c.cx, c.fx), dcy = tsdf_div((float)y - c.cy, c.fy);
    TsdfRay ray;
    ray.ox = c.o[0]; ray.oy = c.o[1]; ray.oz = c.o[2];
    ray.dx = ((c.R[0] * dcx) + (c.R[1] * dcy)) + c.R[2];
    ray.dy = ((c.R[3] * dcx) + (c.R[4] * dcy)) + c.R[5];
    ray.dz = ((c.R[6] * dcx) + (c.R[7] * dcy)) + c.R[8];
    ray.zmin = c.zmin; ray.zmax = c.zmax;
    status = a.mask ? tsdf_ray_march<true>(a, ray, &o) : tsdf_ray_march<false>(a, ray, &o);
    const size_t p = (size_t)y * c.w + x;
    vw.depth[p] = o.depth;  // 0 unless a hit
    if (vw.normal) {
      float* nrm = vw.normal + p * 3;
      nrm[0] = o.nx; nrm[1] = o.ny; nrm[2] = o.nz;
    }
    if (vw.bgr) {
      uint8_t* b = vw.bgr + p * 3;
      b[0] = o.b; b[1] = o.g; b[2] = o.r;
    }
  }
#pragma unroll
  for (int k = 0; k < TSDF_RAY_STATUSES; ++k) {
    const u64 b = __ballot(status == k);
    if (lane == 0 && b) atomicAdd(&s.cnt[k], (unsigned)__popcll(b));
  }
  const u64 unc = __ballot(status == TSDF_RAY_HIT && a.color && o.colored == 0u);
  if (lane == 0 && unc) atomicAdd(&s.unc, (unsigned)__popcll(unc));
  unsigned n = status < 0 ? 0u : o.samples;  // <= 2^20 per ray: a wave's sum fits
#pragma unroll
  for (int off = 32; off; off >>= 1) n += __shfl_down(n, off, 64);
  if (lane == 0 && n) atomicAdd(&s.samples, (u64)n);
  __syncthreads();
  if (threadIdx.x < TSDF_RAY_STATUSES && s.cnt[threadIdx.x]) atomicAdd(&info[TR_STATUS + threadIdx.x], (u64)s.cnt[threadIdx.x]);
  if (threadIdx.x == 4 && s.samples) atomicAdd(&info[TR_SAMPLES], s.samples);
  if (threadIdx.x == 5 && s.unc) atomicAdd(&info[TR_UNCOLORED], (u64)s.unc);
  if (threadIdx.x == 6) {
    const unsigned rays = s.cnt[0] + s.cnt[1] + s.cnt[2] + s.cnt[3];
    if (rays) atomicAdd(&info[TR_RAYS], (u64)rays);
  }
  if (threadIdx.x == 7 && s.cnt[TSDF_RAY_HIT]) atomicAdd(vw.hits, s.cnt[TSDF_RAY_HIT]);
}
