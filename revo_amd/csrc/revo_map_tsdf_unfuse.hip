// revo_map_tsdf_unfuse.hip -- views taken out of the surface again: revo_map_tsdf_unfuse, the exact inverse of
// revo_map_tsdf_fuse and revo_map_tsdf_fuse_color, all or nothing.  Contract: include/revo_hip.h; the per-cell rule (the totals of
// a call's views, the FIT test, the down-date): revo_tsdf_host.h.  Every value is an integer; the classes and quanta are the fuse's,
// through the same map_carve_class_zd[p] and tsdf_quantum.
#include "revo_map_impl.h"
#include "revo_cell_run.h"
#include "revo_tsdf_host.h"

enum { UI_CELLS = 0, UI_UPDATES = 1, UI_WEIGHTED = 2, UI_INSIDE = 3, UI_MISFITS = 4, UI_CUPDATES = 5, UI_COLORED = 6 };

static_assert(sizeof(revo_map_tsdf_unfuse_info) == 64 && offsetof(revo_map_tsdf_unfuse_info, cells) == 8 * UI_CELLS &&
              offsetof(revo_map_tsdf_unfuse_info, updates) == 8 * UI_UPDATES && offsetof(revo_map_tsdf_unfuse_info, cells_weighted) == 8 * UI_WEIGHTED &&
              offsetof(revo_map_tsdf_unfuse_info, cells_inside) == 8 * UI_INSIDE && offsetof(revo_map_tsdf_unfuse_info, misfits) == 8 * UI_MISFITS &&
              offsetof(revo_map_tsdf_unfuse_info, color_updates) == 8 * UI_CUPDATES && offsetof(revo_map_tsdf_unfuse_info, cells_colored) == 8 * UI_COLORED &&
              offsetof(revo_map_tsdf_unfuse_info, reserved) == 56, "the info record is the kernel's counter line");
static_assert(sizeof(revo_map_tsdf_cell) == 8 && sizeof(int2) == 8 && sizeof(revo_map_tsdf_color) == 16 && sizeof(uint4) == 16, "the cells are one word each");

struct TsdfUnfuseK {
  const MapCarveView* views; int n;
  float trunc, voxel;
  revo_map_df_box box;
  unsigned cells;
  int2* tsdf;                 // 16-byte aligned: thread t owns the cells 4 t .. 4 t + 3
  uint4* color;               // COLOR: 16-byte aligned, sum_b, sum_g, sum_r, weight per cell
  const uint8_t* const* bgr;  // COLOR: per view h x w x 3 bytes
  u64* line;                  // one 64-byte line: UI_*
  unsigned* vinfo;            // the check pass: 8 words per view, revo_map_carve_view_info
};

// Both passes over k_tsdf_fuse's walk (revo_cell_run.h): one thread per run of CELL_RUN cells, the views read through uniform
// addresses one after another, the run's cells in registers from one read.  Per cell the views' updates are summed into a
// TsdfDown; behind the views the cell is tested (the check pass) or down-dated (the apply pass).
// The check pass (APPLY false) writes nothing to the volumes: it counts the cells that do not FIT, the volumes' cells as they
// stand, and per view the classes of a wave by ballots into LDS.  The apply pass runs only behind a check that found no misfit,
// writes every cell of a run once and counts what it took out and what is left.  Every counter takes one global atomic per block;
// no atomic touches a cell.
template <bool COLOR, bool APPLY>
__global__ void __launch_bounds__(CELL_RUN_THREADS) k_tsdf_unfuse(const TsdfUnfuseK a) {
  __shared__ unsigned s_cls[APPLY ? 1 : CARVE_MAX_VIEWS * CARVE_CLASSES];
  __shared__ unsigned s_cnt[8];  // UI_*
  if (!APPLY)
    for (int k = threadIdx.x; k < a.n * CARVE_CLASSES; k += CELL_RUN_THREADS) s_cls[k] = 0;
  if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  CellRun r;
  const size_t c0 = cell_run_first(blockIdx.x);
  int sum[CELL_RUN];
  unsigned weight[CELL_RUN];
  uint4 rgb[CELL_RUN];  // COLOR: the colour cells
  TsdfDown down[CELL_RUN];
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j) {
    cell_run_cell(c0, j, a.box, a.cells, a.voxel, r);
    sum[j] = 0;
    weight[j] = 0u;
    rgb[j] = make_uint4(0u, 0u, 0u, 0u);
    down[j] = TsdfDown{0u, 0u, 0, 0u, 0u, 0u};
  }
  cell_run_load(a.tsdf, c0, r, sum, weight);
  cell_run_load_color<COLOR>(a.color, c0, r, rgb);
  for (int vi = 0; vi < a.n; ++vi) {  // uniform: the ballots see whole waves
    int cls[CELL_RUN];
#pragma unroll
    for (int j = 0; j < CELL_RUN; ++j) {
      float z = 0.0f, dc = 0.0f;
      unsigned pix = 0u;
      if (COLOR) cls[j] = r.valid[j] ? map_carve_class_zdp(r.px[j], r.py[j], r.pz[j], a.views[vi], 0, a.trunc, 0.0f, &z, &dc, &pix) : -1;
      else cls[j] = r.valid[j] ? map_carve_class_zd(r.px[j], r.py[j], r.pz[j], a.views[vi], 0, a.trunc, 0.0f, &z, &dc) : -1;
      if (cls[j] == CARVE_FREE || cls[j] == CARVE_CONFIRMED) {
        const bool confirmed = cls[j] == CARVE_CONFIRMED;
        const int q = confirmed ? tsdf_quantum(dc, z, a.trunc) : TSDF_Q_ONE;
        tsdf_down_add(down[j], confirmed, q, COLOR && confirmed ? a.bgr[vi] + (size_t)pix * 3 : nullptr);
      }
    }
    if (!APPLY) cell_run_count_classes(cls, s_cls + vi * CARVE_CLASSES);
  }
  unsigned n_upd = 0, n_cupd = 0, n_misfit = 0, n_weighted = 0, n_inside = 0, n_col = 0;
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j) {
    if (!r.valid[j]) continue;
    if (down[j].k) {
      if (APPLY) {
        tsdf_down_apply(sum[j], weight[j], down[j]);
        n_upd += down[j].k;
        if (COLOR) {
          tsdf_down_color_apply(rgb[j].x, rgb[j].y, rgb[j].z, rgb[j].w, down[j]);
          n_cupd += down[j].kc;
        }
      } else {
        const bool fits = tsdf_down_fits(sum[j], weight[j], down[j]) &&
                          (!COLOR || tsdf_down_color_fits(weight[j], rgb[j].x, rgb[j].y, rgb[j].z, rgb[j].w, down[j]));
        n_misfit += fits ? 0u : 1u;
      }
    }
    n_weighted += weight[j] > 0u;
    n_inside += weight[j] > 0u && sum[j] < 0;
    if (COLOR) n_col += rgb[j].w > 0u;
  }
  if (APPLY) {
    cell_run_store(a.tsdf, c0, r, sum, weight);
    cell_run_store_color<COLOR>(a.color, c0, r, rgb);
  }
  // a block's updates: at most 256 * 4 * 64.  The counters in UI_*'s order, from UI_UPDATES on
  if (COLOR) cell_run_tally(s_cnt + UI_UPDATES, n_upd, n_weighted, n_inside, n_misfit, n_cupd, n_col);
  else cell_run_tally(s_cnt + UI_UPDATES, n_upd, n_weighted, n_inside, n_misfit);
  __syncthreads();
  if (threadIdx.x >= UI_UPDATES && threadIdx.x <= UI_COLORED && s_cnt[threadIdx.x]) atomicAdd(&a.line[threadIdx.x], (u64)s_cnt[threadIdx.x]);
  if (blockIdx.x == 0 && threadIdx.x == 8) a.line[UI_CELLS] = (u64)a.cells;
  if (!APPLY)
    for (int k = threadIdx.x; k < a.n * CARVE_CLASSES; k += CELL_RUN_THREADS)
      if (s_cls[k]) atomicAdd(&a.vinfo[(k / CARVE_CLASSES) * 8 + k % CARVE_CLASSES], s_cls[k]);
}

template <bool APPLY>
static void unfuse_launch(bool with_color, const TsdfUnfuseK& a, hipStream_t s) {
  const dim3 grid(cell_run_blocks(a.cells));
  if (with_color) hipLaunchKernelGGL((k_tsdf_unfuse<true, APPLY>), grid, dim3(CELL_RUN_THREADS), 0, s, a);
  else hipLaunchKernelGGL((k_tsdf_unfuse<false, APPLY>), grid, dim3(CELL_RUN_THREADS), 0, s, a);
}

extern "C" int revo_map_tsdf_unfuse(revo_map* m, const revo_map_df_box* box, int n, const revo_map_carve_view* views,
                                    const uint8_t* const* bgr, int device_in, float trunc, revo_map_tsdf_cell* tsdf,
                                    revo_map_tsdf_color* color, int device_tsdf, revo_map_tsdf_unfuse_info* info,
                                    revo_map_carve_view_info* view_info) {
  if (!m || !box || !views || !tsdf) return fail(REVO_ERR_INVALID_ARG, "null argument");
  const std::string who = "revo_map_tsdf_unfuse: ";
  if (!color != !bgr) return fail(REVO_ERR_INVALID_ARG, who + "bgr and color are both given or both NULL");
  const bool with_color = color != nullptr;
  size_t cells = 0;
  if (const char* why = map_df_box_check(box, &cells)) return fail(REVO_ERR_INVALID_ARG, who + why);
  if (n < 1 || n > CARVE_MAX_VIEWS) return fail(REVO_ERR_INVALID_ARG, who + "n must be 1 .. 64 views");
  TRY(map_check_side(device_in, "device_in"));
  TRY(map_check_side(device_tsdf, "device_tsdf"));
  if (device_tsdf) TRY(map_check_aligned((uintptr_t)tsdf | (uintptr_t)color | (uintptr_t)view_info, 16, "a device output is"));
  float tr = 0.0f;
  if (const char* why = tsdf_unfuse_trunc(trunc, m->voxel, &tr)) return fail(REVO_ERR_INVALID_ARG, who + why);
  MapTsdfViews v;
  TRY(map_tsdf_views_begin(m, who, cells, n, views, bgr, device_in, device_tsdf, &v));
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t vinfo_bytes = sizeof(revo_map_carve_view_info) * (size_t)n, vol_bytes = sizeof(revo_map_tsdf_cell) * cells;
  const size_t col_bytes = sizeof(revo_map_tsdf_color) * cells;
  TsdfUnfuseK a{};
  a.views = v.views; a.n = n;
  a.trunc = tr; a.voxel = m->voxel;
  a.box = *box;
  a.cells = (unsigned)cells;
  a.tsdf = device_tsdf ? (int2*)tsdf : (int2*)m->tsdfvol.p;
  a.line = (u64*)m->tsdfcnt.p;  // the check's line; the apply's is the next one
  a.vinfo = device_tsdf && view_info ? (unsigned*)view_info : (unsigned*)(m->tsdfcnt.p + 256);
  if (with_color) {
    a.bgr = v.bgr;
    a.color = device_tsdf ? (uint4*)color : (uint4*)m->tsdfcol.p;
    if (!device_tsdf) HIPCHECK(hipMemcpyAsync(a.color, color, col_bytes, hipMemcpyHostToDevice, s));
  }
  if (!device_tsdf) HIPCHECK(hipMemcpyAsync(a.tsdf, tsdf, vol_bytes, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemsetAsync(m->tsdfcnt.p, 0, 128, s));
  HIPCHECK(hipMemsetAsync(a.vinfo, 0, vinfo_bytes, s));
  unfuse_launch<false>(with_color, a, s);
  HIPCHECK(hipGetLastError());
  u64 line[8];
  HIPCHECK(hipMemcpyAsync(line, a.line, sizeof(line), hipMemcpyDeviceToHost, s));
  if (!device_tsdf && view_info) HIPCHECK(hipMemcpyAsync(view_info, a.vinfo, vinfo_bytes, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));  // the verdict
  line[7] = 0;
  if (line[UI_MISFITS]) {
    if (info) memcpy(info, line, sizeof(line));
    return fail(REVO_ERR_INVALID_ARG, who + std::to_string((unsigned long long)line[UI_MISFITS]) +
                                          " cells do not fit: a view that is not in them, a full weight, or sums no fuse can reach");
  }
  a.line = (u64*)(m->tsdfcnt.p + 64);
  unfuse_launch<true>(with_color, a, s);
  HIPCHECK(hipGetLastError());
  if (!device_tsdf) {
    HIPCHECK(hipMemcpyAsync(tsdf, a.tsdf, vol_bytes, hipMemcpyDeviceToHost, s));
    if (with_color) HIPCHECK(hipMemcpyAsync(color, a.color, col_bytes, hipMemcpyDeviceToHost, s));
  }
  if (info) HIPCHECK(hipMemcpyAsync(line, a.line, sizeof(line), hipMemcpyDeviceToHost, s));
  if (!device_tsdf || info || v.uploaded) HIPCHECK(hipStreamSynchronize(s));
  if (info) {
    line[7] = 0;
    memcpy(info, line, sizeof(line));
  }
  return REVO_OK;
}
