// revo_cell_run.h -- the walk over a box's cells that k_tsdf_fuse, k_tsdf_fuse_many, k_tsdf_unfuse, k_tsdf_unfuse_many and k_map_observe share, each
// piece written once: how the cells are dealt out to blocks and threads, where a thread's cells lie and which of them exist, how
// a run of TSDF and colour cells is read and written, and how a block counts -- a view's classes by ballots, a thread's own counts
// by a wave sum -- into LDS.  The batched fuse equals the single one and the unfuse inverts the fuse byte for byte because they
// own the same cells, at the same centres, through this text; the per-cell rules are revo_seen_host.h's and revo_tsdf_host.h's.
// The first part is plain C++ (revo_tsdf_many_host.h and with it tests/cpp/align_stepper_host.cpp compile it for the host); the
// device part is for the .hip units, behind revo_map_impl.h.  Internal.
#pragma once
#include <cstddef>

#define CELL_RUN 4            // consecutive cells of a thread (z fastest): two 16-byte words of a TSDF volume, one 32-bit word of a seen volume
#define CELL_RUN_THREADS 256  // threads of a block: a block owns CELL_RUN * CELL_RUN_THREADS cells that follow each other

#if defined(__HIPCC__)
#define CELL_HD __host__ __device__ inline
#else
#define CELL_HD inline
#endif

// The blocks of a launch over `cells` cells.
CELL_HD unsigned cell_run_blocks(size_t cells) {
  const size_t runs = (cells + CELL_RUN - 1) / CELL_RUN;
  return (unsigned)((runs + CELL_RUN_THREADS - 1) / CELL_RUN_THREADS);
}

#if defined(__HIPCC__)
#include "revo_map_impl.h"
#include "revo_seen_host.h"  // a cell's point is the seen volume's

// A thread's run: consecutive lanes take consecutive runs, so a wave's projections fall on neighbouring pixels.
struct CellRun {
  bool valid[CELL_RUN];  // the cell exists: a volume's cells need be no multiple of four
  float px[CELL_RUN], py[CELL_RUN], pz[CELL_RUN];  // the cells' centres; a missing cell has the centre of cell 0 and is not looked at
};
// The four cells exist, and a volume's word at the run's first cell is aligned as a whole run's.
__device__ __forceinline__ bool cell_run_whole(const CellRun& r) { return r.valid[CELL_RUN - 1]; }

// The first cell of this thread's run in the block `blk` of the volume (a single launch: blockIdx.x; a batched one: the block's
// number within its job).
__device__ __forceinline__ size_t cell_run_first(unsigned blk) { return (size_t)(blk * (unsigned)CELL_RUN_THREADS + threadIdx.x) * CELL_RUN; }
// The cell j of the run that starts at c0: whether it exists, and its centre.  A kernel calls it from its own `#pragma unroll`
// loop over the run, and the box goes by value.  Both are for the compiler, which reads the views' depth and colour images with
// global loads only while it can prove, early and with a bounded search, that nothing has written to them: a loop over the run
// in here would arrive in the kernel already unrolled, four times the stores to local arrays in front of that search, and a
// reference would bind to the kernel's argument record.  Either turned those loads into flat ones
// (profiles/cell_run_refactor_isa.txt).
__device__ __forceinline__ void cell_run_cell(size_t c0, int j, const revo_map_df_box box, unsigned cells, float voxel, CellRun& r) {
  const unsigned ny = (unsigned)box.n[1], nz = (unsigned)box.n[2];
  const size_t c = c0 + j;
  r.valid[j] = c < cells;
  const unsigned cc = r.valid[j] ? (unsigned)c : 0u;
  const unsigned line = cc / nz, iz = cc - line * nz;
  const unsigned ix = line / ny, iy = line - ix * ny;
  r.px[j] = seen_centre(box.lo[0], (int)ix, voxel);
  r.py[j] = seen_centre(box.lo[1], (int)iy, voxel);
  r.pz[j] = seen_centre(box.lo[2], (int)iz, voxel);
}

// The run's TSDF cells (tsdf: 16-byte aligned) from the one read to the one write: two 16-byte words for a whole run, 8-byte
// words for the tail of a volume.  A missing cell's sum and weight are left as they are.
__device__ __forceinline__ void cell_run_load(const int2* tsdf, size_t c0, const CellRun& r, int (&sum)[CELL_RUN], unsigned (&weight)[CELL_RUN]) {
  if (cell_run_whole(r)) {
    const int4 lo = *(const int4*)(tsdf + c0), hi = *(const int4*)(tsdf + c0 + 2);
    sum[0] = lo.x; weight[0] = (unsigned)lo.y; sum[1] = lo.z; weight[1] = (unsigned)lo.w;
    sum[2] = hi.x; weight[2] = (unsigned)hi.y; sum[3] = hi.z; weight[3] = (unsigned)hi.w;
  } else {
#pragma unroll
    for (int j = 0; j < CELL_RUN; ++j)
      if (r.valid[j]) { const int2 v = tsdf[c0 + j]; sum[j] = v.x; weight[j] = (unsigned)v.y; }
  }
}
__device__ __forceinline__ void cell_run_store(int2* tsdf, size_t c0, const CellRun& r, const int (&sum)[CELL_RUN], const unsigned (&weight)[CELL_RUN]) {
  if (cell_run_whole(r)) {
    *(int4*)(tsdf + c0) = make_int4(sum[0], (int)weight[0], sum[1], (int)weight[1]);
    *(int4*)(tsdf + c0 + 2) = make_int4(sum[2], (int)weight[2], sum[3], (int)weight[3]);
  } else {
#pragma unroll
    for (int j = 0; j < CELL_RUN; ++j)
      if (r.valid[j]) tsdf[c0 + j] = make_int2(sum[j], (int)weight[j]);
  }
}
// The run's colour cells, one 16-byte word each.  Without COLOR neither `color` nor `rgb` is looked at.
template <bool COLOR>
__device__ __forceinline__ void cell_run_load_color(const uint4* color, size_t c0, const CellRun& r, uint4 (&rgb)[CELL_RUN]) {
  if (!COLOR) return;
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j)
    if (r.valid[j]) rgb[j] = color[c0 + j];
}
template <bool COLOR>
__device__ __forceinline__ void cell_run_store_color(uint4* color, size_t c0, const CellRun& r, const uint4 (&rgb)[CELL_RUN]) {
  if (!COLOR) return;
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j)
    if (r.valid[j]) color[c0 + j] = rgb[j];
}

// The classes of one view over a wave's runs (cls[j]: the class of the cell j, -1 for a missing one), counted by ballots into the
// CARVE_CLASSES counters of the LDS row s_row.  Every lane of the wave calls it.
__device__ __forceinline__ void cell_run_count_classes(const int (&cls)[CELL_RUN], unsigned* s_row) {
#pragma unroll
  for (int k = 0; k < CARVE_CLASSES; ++k) {
    unsigned cnt = 0;
#pragma unroll
    for (int j = 0; j < CELL_RUN; ++j) cnt += (unsigned)__popcll(__ballot(cls[j] == k));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(s_row + k, cnt);
  }
}
// The sum of v over the wave, in lane 0.
__device__ __forceinline__ unsigned cell_wave_sum(unsigned v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
// The threads' counts n..., summed over the wave, into the LDS counters s_cnt[0], s_cnt[1], ...: lane 0 adds those that are not
// zero.  Every lane of the wave calls it.
template <typename... N>
__device__ __forceinline__ void cell_run_tally(unsigned* s_cnt, N... n) {
  const unsigned v[] = {cell_wave_sum(n)...};
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int i = 0; i < (int)sizeof...(N); ++i)
      if (v[i]) atomicAdd(s_cnt + i, v[i]);
  }
}
#endif
