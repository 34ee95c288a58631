// revo_map_seen.hip -- what has been looked at: revo_map_observe, the seen volume of a box of voxel indices from
// depth views (one byte per cell: free votes and the surface bit), and revo_map_frontiers, the free cells next to unseen space.
// revo_map_known_field, the distance field over solid + unseen cells, lives with the field's passes in revo_map_field.hip.
// Contracts: include/revo_hip.h.  Every value is an integer that float32 arithmetic with one definition decides.
#include "revo_map_impl.h"
#include "revo_cell_run.h"
#include "revo_seen_host.h"

struct MapObserveK {
  const MapCarveView* views; int n;
  int radius; unsigned accumulate;
  float margin, margin_rel, voxel;
  revo_map_df_box box;
  unsigned cells;
  uint8_t* seen;      // 4-byte aligned: thread t owns the word of the cells 4 t .. 4 t + 3
  u64* info;          // one 64-byte line: revo_map_observe_info
  unsigned* vinfo;    // 8 words per view: revo_map_carve_view_info
};
enum { OBS_CELLS = 0, OBS_FREE = 1, OBS_SURFACE = 2, OBS_VOTES = 3, OBS_NEW = 4 };

static_assert(sizeof(revo_map_observe_params) == 16 && offsetof(revo_map_observe_params, accumulate) == 4 && offsetof(revo_map_observe_params, margin) == 8 &&
              offsetof(revo_map_observe_params, margin_rel) == 12, "the parameter record is the documented layout");
static_assert(sizeof(revo_map_observe_info) == 64 && offsetof(revo_map_observe_info, cells) == 8 * OBS_CELLS &&
              offsetof(revo_map_observe_info, cells_free) == 8 * OBS_FREE && offsetof(revo_map_observe_info, cells_surface) == 8 * OBS_SURFACE &&
              offsetof(revo_map_observe_info, votes) == 8 * OBS_VOTES && offsetof(revo_map_observe_info, newly_known) == 8 * OBS_NEW &&
              offsetof(revo_map_observe_info, reserved) == 40, "the info record is the kernel's counter line");

// One thread per 32-bit word of the volume, over the walk of revo_cell_run.h: CELL_RUN cells that follow each other in memory (z
// fastest, so mostly along z, whatever n[2] is and wherever a z-line starts).  The views are read through uniform addresses one
// after another; a cell's votes and surface bit stay in two packed registers (a byte per cell: f <= 64 cannot carry).  A word
// inside the volume is read (when accumulating) and written as one word, the tail of a volume whose cells are no multiple of
// four byte by byte.  Per view the classes of a wave are counted by ballots into LDS; every counter takes one global atomic per
// block.  No atomic touches a cell.
__global__ void __launch_bounds__(CELL_RUN_THREADS) k_map_observe(const MapObserveK a) {
  __shared__ unsigned s_cls[CARVE_MAX_VIEWS * CARVE_CLASSES];
  __shared__ unsigned s_cnt[4];  // free, surface, votes, newly known
  for (int k = threadIdx.x; k < a.n * CARVE_CLASSES; k += CELL_RUN_THREADS) s_cls[k] = 0;
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  CellRun r;  // whole: seen + c0 is 4-byte aligned
  const size_t c0 = cell_run_first(blockIdx.x);
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j) cell_run_cell(c0, j, a.box, a.cells, a.voxel, r);
  unsigned votes = 0, surface = 0;  // byte j: the run's cell j
  for (int vi = 0; vi < a.n; ++vi) {  // uniform: the ballots see whole waves
    int cls[CELL_RUN];
#pragma unroll
    for (int j = 0; j < CELL_RUN; ++j) {
      cls[j] = r.valid[j] ? map_carve_class(r.px[j], r.py[j], r.pz[j], a.views[vi], a.radius, a.margin, a.margin_rel) : -1;
      votes += (cls[j] == CARVE_FREE ? 1u : 0u) << (8 * j);
      surface |= (cls[j] == CARVE_CONFIRMED ? SEEN_SURFACE : 0u) << (8 * j);
    }
    cell_run_count_classes(cls, s_cls + vi * CARVE_CLASSES);
  }
  unsigned in = 0;
  if (a.accumulate) {
    if (cell_run_whole(r)) {
      in = *(const unsigned*)(a.seen + c0);
    } else {
#pragma unroll
      for (int j = 0; j < CELL_RUN; ++j)
        if (r.valid[j]) in |= (unsigned)a.seen[c0 + j] << (8 * j);
    }
  }
  unsigned out = 0, n_free = 0, n_surface = 0, n_votes = 0, n_new = 0;
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j) {
    const unsigned f = (votes >> (8 * j)) & 0xffu, b_in = (in >> (8 * j)) & 0xffu;
    const unsigned b = seen_byte((uint8_t)b_in, f, (surface >> (8 * j + 7)) & 1u);
    out |= b << (8 * j);
    if (r.valid[j]) {
      n_free += (b & SEEN_VOTES) != 0;
      n_surface += (b & SEEN_SURFACE) != 0;
      n_votes += f;
      n_new += b_in == 0 && b != 0;
    }
  }
  if (cell_run_whole(r)) {
    *(unsigned*)(a.seen + c0) = out;
  } else {
#pragma unroll
    for (int j = 0; j < CELL_RUN; ++j)
      if (r.valid[j]) a.seen[c0 + j] = (uint8_t)(out >> (8 * j));
  }
  cell_run_tally(s_cnt, n_free, n_surface, n_votes, n_new);  // a block's votes: at most 256 * 4 * 64
  __syncthreads();
  if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&a.info[OBS_FREE + threadIdx.x], (u64)s_cnt[threadIdx.x]);
  if (blockIdx.x == 0 && threadIdx.x == 4) a.info[OBS_CELLS] = (u64)a.cells;
  for (int k = threadIdx.x; k < a.n * CARVE_CLASSES; k += CELL_RUN_THREADS)
    if (s_cls[k]) atomicAdd(&a.vinfo[(k / CARVE_CLASSES) * 8 + k % CARVE_CLASSES], s_cls[k]);
}

extern "C" int revo_map_observe(revo_map* m, const revo_map_df_box* box, int n, const revo_map_carve_view* views, int device_in,
                                const revo_map_observe_params* prm, uint8_t* seen, int device_seen, revo_map_observe_info* info,
                                revo_map_carve_view_info* view_info) {
  if (!m || !box || !views || !seen) return fail(REVO_ERR_INVALID_ARG, "null argument");
  size_t cells = 0;
  if (const char* why = map_df_box_check(box, &cells)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_observe: ") + why);
  if (n < 1 || n > CARVE_MAX_VIEWS) return fail(REVO_ERR_INVALID_ARG, "revo_map_observe: n must be 1 .. 64 views");
  TRY(map_check_side(device_in, "device_in"));
  TRY(map_check_side(device_seen, "device_seen"));
  if (device_seen) TRY(map_check_aligned((uintptr_t)seen | (uintptr_t)info | (uintptr_t)view_info, 16, "a device output is"));
  revo_map_observe_params pp;
  if (const char* why = seen_params_check(prm, m->voxel, &pp)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_observe: ") + why);
  std::vector<MapCarveView> hv(n);
  size_t up_bytes = 0;
  TRY(map_views_prepare(m, n, views, device_in, hv.data(), &up_bytes));
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t vinfo_bytes = sizeof(revo_map_carve_view_info) * (size_t)n;
  TRY(m->seen_views.reserve(n, s));  // waits until the previous call's upload has read the pinned rows
  TRY(m->seencnt.reserve(256 + sizeof(revo_map_carve_view_info) * CARVE_MAX_VIEWS, s));
  TRY(m->seenvol.reserve(device_seen ? 0 : cells, s));
  DevScratch images;  // host depth images of the call, uploaded; freed behind the wait below
  if (up_bytes) {
    TRY(images.alloc(up_bytes));
    TRY(map_views_upload(n, views, hv.data(), images.p, s));
  }
  memcpy(m->seen_views.h, hv.data(), sizeof(MapCarveView) * n);
  TRY(m->seen_views.upload(n, s));
  MapObserveK a{};
  a.views = m->seen_views.d; a.n = n;
  a.radius = pp.radius; a.accumulate = pp.accumulate;
  a.margin = pp.margin; a.margin_rel = pp.margin_rel; a.voxel = m->voxel;
  a.box = *box;
  a.cells = (unsigned)cells;
  a.seen = device_seen ? seen : (uint8_t*)m->seenvol.p;
  a.info = device_seen && info ? (u64*)info : (u64*)m->seencnt.p;
  a.vinfo = device_seen && view_info ? (unsigned*)view_info : (unsigned*)(m->seencnt.p + 256);
  if (!device_seen && pp.accumulate) HIPCHECK(hipMemcpyAsync(a.seen, seen, cells, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemsetAsync(a.info, 0, sizeof(revo_map_observe_info), s));
  HIPCHECK(hipMemsetAsync(a.vinfo, 0, vinfo_bytes, s));
  hipLaunchKernelGGL(k_map_observe, dim3(cell_run_blocks(cells)), dim3(CELL_RUN_THREADS), 0, s, a);
  HIPCHECK(hipGetLastError());
  if (!device_seen) {
    HIPCHECK(hipMemcpyAsync(seen, a.seen, cells, hipMemcpyDeviceToHost, s));
    if (info) HIPCHECK(hipMemcpyAsync(info, a.info, sizeof(revo_map_observe_info), hipMemcpyDeviceToHost, s));
    if (view_info) HIPCHECK(hipMemcpyAsync(view_info, a.vinfo, vinfo_bytes, hipMemcpyDeviceToHost, s));
  }
  if (!device_seen || up_bytes) HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

// ------------------------------------------------------------------------------------------------------------ frontiers --
struct MapFrontierK {
  const unsigned* bits; unsigned wz;  // the box's solid voxels, as k_df_occupancy leaves them
  const uint8_t* seen;
  revo_map_df_box box;
  unsigned cells, min_views;
  int4* out; unsigned cap_out;  // the records, at most cap_out of them (0: count only)
  u64* count;
};
static_assert(sizeof(revo_map_plan_seed) == sizeof(int4), "a frontier record is one 16-byte word");

__device__ __forceinline__ bool frontier_unknown(const MapFrontierK& a, unsigned line, unsigned iz, size_t c) {
  const bool solid = (a.bits[(size_t)line * a.wz + (iz >> 5)] >> (iz & 31)) & 1u;
  return seen_is_unknown(solid, a.seen[c], a.min_views);
}

// One thread per cell: its own byte and bit, then -- only for a free cell that is not solid -- those of the face neighbours
// inside the box.  The frontier cells are compacted as k_map_export compacts (LDS counter, one global atomic per block).
__global__ void __launch_bounds__(256) k_map_frontiers(const MapFrontierK a) {
  __shared__ unsigned s_n, s_base;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const unsigned c = blockIdx.x * 256u + threadIdx.x;
  const unsigned nx = (unsigned)a.box.n[0], ny = (unsigned)a.box.n[1], nz = (unsigned)a.box.n[2];
  bool sel = false;
  unsigned ix = 0, iy = 0, iz = 0;
  if (c < a.cells) {
    const unsigned line = c / nz;
    iz = c - line * nz; ix = line / ny; iy = line - ix * ny;
    const bool solid = (a.bits[(size_t)line * a.wz + (iz >> 5)] >> (iz & 31)) & 1u;
    const uint8_t b = a.seen[c];
    if (!solid && seen_is_free(b, a.min_views)) {
      int unknown = 0;
      if (iz > 0) unknown += frontier_unknown(a, line, iz - 1, (size_t)c - 1);
      if (iz + 1 < nz) unknown += frontier_unknown(a, line, iz + 1, (size_t)c + 1);
      if (iy > 0) unknown += frontier_unknown(a, line - 1, iz, (size_t)c - nz);
      if (iy + 1 < ny) unknown += frontier_unknown(a, line + 1, iz, (size_t)c + nz);
      if (ix > 0) unknown += frontier_unknown(a, line - ny, iz, (size_t)c - (size_t)ny * nz);
      if (ix + 1 < nx) unknown += frontier_unknown(a, line + ny, iz, (size_t)c + (size_t)ny * nz);
      sel = seen_is_frontier(solid, b, a.min_views, unknown);
    }
  }
  const unsigned j = map_compact(sel, s_n, s_base, a.count);
  if (sel && j < a.cap_out) a.out[j] = make_int4(a.box.lo[0] + (int)ix, a.box.lo[1] + (int)iy, a.box.lo[2] + (int)iz, 0);
}

extern "C" int revo_map_frontiers(revo_map* m, const revo_map_df_box* box, uint32_t min_count, const uint8_t* seen, int device_seen,
                                  uint32_t min_views, revo_map_plan_seed* cells_out, size_t cap, size_t* n_cells, int device_out) {
  if (!m || !box || !seen || !n_cells) return fail(REVO_ERR_INVALID_ARG, "null argument");
  size_t cells = 0;
  if (const char* why = map_df_box_check(box, &cells)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_frontiers: ") + why);
  TRY(map_check_side(device_seen, "device_seen"));
  TRY(map_check_side(device_out, "device_out"));
  if (device_seen) TRY(map_check_aligned((uintptr_t)seen, 16, "the device seen volume is"));
  if (device_out) TRY(map_check_aligned((uintptr_t)cells_out, 16, "the device output is"));
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  MapFrontierK a{};
  a.box = *box;
  a.cells = (unsigned)cells;
  a.min_views = min_views;
  TRY(map_df_solid_bits(m, box, min_count, s, &a.bits, &a.wz));
  TRY(m->seenvol.reserve(device_seen ? 0 : cells, s));
  if (!device_seen) HIPCHECK(hipMemcpyAsync(m->seenvol.p, seen, cells, hipMemcpyHostToDevice, s));
  a.seen = device_seen ? seen : (const uint8_t*)m->seenvol.p;
  a.count = (u64*)(m->dfcnt.p + 64);  // behind the field's info line
  const dim3 grid((unsigned)((cells + 255) / 256));
  u64 count = 0, again = 0;
  // nothing may be written when cap is too small: count first, then write
  HIPCHECK(hipMemsetAsync(a.count, 0, sizeof(u64), s));
  hipLaunchKernelGGL(k_map_frontiers, grid, dim3(256), 0, s, a);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(&count, a.count, sizeof(u64), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  *n_cells = (size_t)count;
  if (!cells_out || !count) return REVO_OK;
  if (cap < count) return fail(REVO_ERR_CAPACITY, "voxel map: the output holds fewer records than there are frontier cells");
  DevScratch recs;
  if (!device_out) TRY(recs.alloc(sizeof(revo_map_plan_seed) * count));
  a.out = device_out ? (int4*)cells_out : (int4*)recs.p;
  a.cap_out = (unsigned)count;
  HIPCHECK(hipMemsetAsync(a.count, 0, sizeof(u64), s));
  hipLaunchKernelGGL(k_map_frontiers, grid, dim3(256), 0, s, a);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(&again, a.count, sizeof(u64), hipMemcpyDeviceToHost, s));
  if (!device_out) HIPCHECK(hipMemcpyAsync(cells_out, recs.p, sizeof(revo_map_plan_seed) * count, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (again != count) return fail(REVO_ERR_HIP, "voxel map: two frontier launches over one volume disagree");
  if (!device_out) {  // the cell's place in the box: x, then y, then z
    std::sort(cells_out, cells_out + count, [](const revo_map_plan_seed& p, const revo_map_plan_seed& q) {
      return p.cell[0] != q.cell[0] ? p.cell[0] < q.cell[0] : (p.cell[1] != q.cell[1] ? p.cell[1] < q.cell[1] : p.cell[2] < q.cell[2]);
    });
  }
  return REVO_OK;
}
