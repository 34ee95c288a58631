// revo_map_tsdf.hip -- a surface: revo_map_tsdf_fuse, the truncated signed distance volume of a box of voxel indices
// fused from depth views with integer sums, and revo_map_tsdf_mesh, the mesh of its zero level set over the Kuhn tetrahedra of
// the cells' cubes, in one canonical order; with them revo_map_tsdf_fuse_color, the colour volume fused in the same
// pass, and revo_map_tsdf_mesh_attr, the mesh with a normal and a colour per vertex.  Contracts: include/revo_hip.h.  Every value
// is an integer that float32 arithmetic with one definition decides, or (a vertex, a normal) a float that one chain of separately
// rounded operations gives.
#include "revo_map_impl.h"
#include "revo_cell_run.h"
#include "revo_tsdf_host.h"

struct TsdfFuseK {
  const MapCarveView* views; int n;
  unsigned accumulate;
  float trunc, voxel;
  revo_map_df_box box;
  unsigned cells;
  int2* tsdf;         // 16-byte aligned: thread t owns the cells 4 t .. 4 t + 3
  u64* info;          // one 64-byte line: revo_map_tsdf_info
  unsigned* vinfo;    // 8 words per view: revo_map_carve_view_info
};
struct TsdfColorK {     // what k_tsdf_fuse<true> takes beside TsdfFuseK
  const uint8_t* const* bgr;  // per view: h x w x 3 bytes
  uint4* color;               // 16-byte aligned: sum_b, sum_g, sum_r, weight per cell
  u64* info;                  // half a line: revo_map_tsdf_color_info
};
enum { TF_CELLS = 0, TF_UPDATES = 1, TF_WEIGHTED = 2, TF_INSIDE = 3, TF_SATURATED = 4 };

static_assert(sizeof(revo_map_tsdf_cell) == 8 && offsetof(revo_map_tsdf_cell, weight) == 4 && sizeof(int2) == 8, "a cell is one 8-byte word");
static_assert(sizeof(revo_map_tsdf_params) == 16 && offsetof(revo_map_tsdf_params, accumulate) == 4 && offsetof(revo_map_tsdf_params, reserved) == 8,
              "the parameter record is the documented layout");
static_assert(sizeof(revo_map_tsdf_info) == 64 && offsetof(revo_map_tsdf_info, cells) == 8 * TF_CELLS &&
              offsetof(revo_map_tsdf_info, updates) == 8 * TF_UPDATES && offsetof(revo_map_tsdf_info, cells_weighted) == 8 * TF_WEIGHTED &&
              offsetof(revo_map_tsdf_info, cells_inside) == 8 * TF_INSIDE && offsetof(revo_map_tsdf_info, saturated) == 8 * TF_SATURATED &&
              offsetof(revo_map_tsdf_info, reserved) == 40, "the info record is the kernel's counter line");
static_assert(sizeof(revo_map_tsdf_color) == 16 && offsetof(revo_map_tsdf_color, sum_g) == 4 && offsetof(revo_map_tsdf_color, sum_r) == 8 &&
              offsetof(revo_map_tsdf_color, weight) == 12 && sizeof(uint4) == 16, "a colour cell is one 16-byte word");
static_assert(sizeof(revo_map_tsdf_color_info) == 32 && offsetof(revo_map_tsdf_color_info, cells_colored) == 8 &&
              offsetof(revo_map_tsdf_color_info, reserved) == 16, "the colour info record is the kernel's two counters");

// The walk is revo_cell_run.h's: one thread per run of CELL_RUN cells that follow each other in memory.  The views are read through
// uniform addresses one after another; a cell's sum and weight stay in registers from the one read (when accumulating) to the one
// write.  Per view the classes of a wave are counted by ballots into LDS; every counter takes one global atomic per block.  No
// atomic touches a cell.
// COLOR (revo_map_tsdf_fuse_color): the run's four colour cells stay in registers the same way, one 16-byte word each; a view's
// three colour bytes are read where its update of a cell is a CONFIRMED one that was not dropped.  Without it `col` is not
// looked at and the kernel is what it was.
template <bool COLOR>
__global__ void __launch_bounds__(CELL_RUN_THREADS) k_tsdf_fuse(const TsdfFuseK a, const TsdfColorK col) {
  __shared__ unsigned s_cls[CARVE_MAX_VIEWS * CARVE_CLASSES];
  __shared__ unsigned s_cnt[4];  // updates, weighted, inside, saturated
  __shared__ unsigned s_col[2];  // colour updates, cells coloured
  for (int k = threadIdx.x; k < a.n * CARVE_CLASSES; k += CELL_RUN_THREADS) s_cls[k] = 0;
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
  if (COLOR && threadIdx.x < 2) s_col[threadIdx.x] = 0;
  __syncthreads();
  CellRun r;
  const size_t c0 = cell_run_first(blockIdx.x);
  int sum[CELL_RUN];
  unsigned weight[CELL_RUN];
  uint4 rgb[CELL_RUN];  // COLOR: the colour cells
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j) {
    cell_run_cell(c0, j, a.box, a.cells, a.voxel, r);
    sum[j] = 0;
    weight[j] = 0u;
    if (COLOR) rgb[j] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (a.accumulate) {
    cell_run_load(a.tsdf, c0, r, sum, weight);
    cell_run_load_color<COLOR>(col.color, c0, r, rgb);
  }
  unsigned n_upd = 0, n_sat = 0, n_cupd = 0;
  for (int vi = 0; vi < a.n; ++vi) {  // uniform: the ballots see whole waves
    int cls[CELL_RUN];
#pragma unroll
    for (int j = 0; j < CELL_RUN; ++j) {
      float z = 0.0f, dc = 0.0f;
      unsigned pix = 0u;
      if (COLOR) cls[j] = r.valid[j] ? map_carve_class_zdp(r.px[j], r.py[j], r.pz[j], a.views[vi], 0, a.trunc, 0.0f, &z, &dc, &pix) : -1;
      else cls[j] = r.valid[j] ? map_carve_class_zd(r.px[j], r.py[j], r.pz[j], a.views[vi], 0, a.trunc, 0.0f, &z, &dc) : -1;
      if (cls[j] == CARVE_FREE || cls[j] == CARVE_CONFIRMED) {
        const int q = cls[j] == CARVE_FREE ? TSDF_Q_ONE : tsdf_quantum(dc, z, a.trunc);
        const unsigned dropped = tsdf_update(sum[j], weight[j], q);
        n_sat += dropped;
        n_upd += 1u - dropped;
        if (COLOR) n_cupd += tsdf_color_update(rgb[j].x, rgb[j].y, rgb[j].z, rgb[j].w, cls[j] == CARVE_CONFIRMED, dropped, col.bgr[vi] + (size_t)pix * 3);
      }
    }
    cell_run_count_classes(cls, s_cls + vi * CARVE_CLASSES);
  }
  unsigned n_weighted = 0, n_inside = 0, n_col = 0;
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j)
    if (r.valid[j]) {
      n_weighted += weight[j] > 0u;
      n_inside += weight[j] > 0u && sum[j] < 0;
    }
  cell_run_store(a.tsdf, c0, r, sum, weight);
  cell_run_store_color<COLOR>(col.color, c0, r, rgb);
  if (COLOR) {
#pragma unroll
    for (int j = 0; j < CELL_RUN; ++j) n_col += r.valid[j] && rgb[j].w > 0u;
  }
  if (COLOR) cell_run_tally(s_col, n_cupd, n_col);
  cell_run_tally(s_cnt, n_upd, n_weighted, n_inside, n_sat);  // a block's updates: at most 256 * 4 * 64
  __syncthreads();
  if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&a.info[TF_UPDATES + threadIdx.x], (u64)s_cnt[threadIdx.x]);
  if (blockIdx.x == 0 && threadIdx.x == 4) a.info[TF_CELLS] = (u64)a.cells;
  if (COLOR && threadIdx.x >= 8 && threadIdx.x < 10 && s_col[threadIdx.x - 8]) atomicAdd(&col.info[threadIdx.x - 8], (u64)s_col[threadIdx.x - 8]);
  for (int k = threadIdx.x; k < a.n * CARVE_CLASSES; k += CELL_RUN_THREADS)
    if (s_cls[k]) atomicAdd(&a.vinfo[(k / CARVE_CLASSES) * 8 + k % CARVE_CLASSES], s_cls[k]);
}

int map_tsdf_views_begin(revo_map* m, const std::string& who, size_t cells, int n, const revo_map_carve_view* views, const uint8_t* const* bgr,
                         int device_in, int device_tsdf, MapTsdfViews* out) {
  const bool with_color = bgr != nullptr;
  std::vector<const uint8_t*> hb(n, nullptr);  // the views' colour images as the kernel reads them
  if (with_color)
    for (int i = 0; i < n; ++i) {
      if (const char* why = tsdf_bgr_check(&views[i], bgr[i])) return fail(REVO_ERR_INVALID_ARG, who + "view " + std::to_string(i) + ": " + why);
      hb[i] = bgr[i];
    }
  std::vector<MapCarveView> hv(n);
  size_t up_bytes = 0;
  TRY(map_views_prepare(m, n, views, device_in, hv.data(), &up_bytes, with_color ? hb.data() : nullptr));
  size_t up_bgr = 0;  // the host colour images behind the depth images in the one upload
  if (with_color && !device_in)
    for (int i = 0; i < n; ++i)
      if (bgr[i]) up_bgr += ((size_t)hv[i].v.w * hv[i].v.h * 3 + 255) & ~(size_t)255;
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  TRY(m->tsdf_views.reserve(n, s));  // waits until the previous call's upload has read the pinned rows
  if (with_color) TRY(m->tsdf_bgr.reserve(n, s));
  TRY(m->tsdfcnt.reserve(256 + sizeof(revo_map_carve_view_info) * CARVE_MAX_VIEWS, s));
  TRY(m->tsdfvol.reserve(device_tsdf ? 0 : sizeof(revo_map_tsdf_cell) * cells, s));
  if (with_color) TRY(m->tsdfcol.reserve(device_tsdf ? 0 : sizeof(revo_map_tsdf_color) * cells, s));
  out->uploaded = up_bytes + up_bgr != 0;
  if (out->uploaded) {
    TRY(out->images.alloc(up_bytes + up_bgr));
    TRY(map_views_upload(n, views, hv.data(), out->images.p, s));
    size_t o = up_bytes;
    for (int i = 0; up_bgr && i < n; ++i) {
      if (!bgr[i]) continue;
      const size_t bytes = (size_t)hv[i].v.w * hv[i].v.h * 3;
      HIPCHECK(hipMemcpyAsync(out->images.p + o, bgr[i], bytes, hipMemcpyHostToDevice, s));
      hb[i] = (const uint8_t*)(out->images.p + o);
      o += (bytes + 255) & ~(size_t)255;
    }
  }
  memcpy(m->tsdf_views.h, hv.data(), sizeof(MapCarveView) * n);
  TRY(m->tsdf_views.upload(n, s));
  out->views = m->tsdf_views.d;
  if (with_color) {
    memcpy(m->tsdf_bgr.h, hb.data(), sizeof(const uint8_t*) * n);
    TRY(m->tsdf_bgr.upload(n, s));
    out->bgr = m->tsdf_bgr.d;
  }
  return REVO_OK;
}

// Both fuse calls.  name: the entry point's, for its messages.  with_color: revo_map_tsdf_fuse_color -- bgr, color and cinfo are
// looked at and k_tsdf_fuse<true> runs.
static int tsdf_fuse_core(const char* name, bool with_color, revo_map* m, const revo_map_df_box* box, int n, const revo_map_carve_view* views,
                          const uint8_t* const* bgr, int device_in, const revo_map_tsdf_params* prm, revo_map_tsdf_cell* tsdf,
                          revo_map_tsdf_color* color, int device_tsdf, revo_map_tsdf_info* info, revo_map_tsdf_color_info* cinfo,
                          revo_map_carve_view_info* view_info) {
  if (!m || !box || !views || !tsdf || (with_color && (!bgr || !color))) return fail(REVO_ERR_INVALID_ARG, "null argument");
  const std::string who = std::string(name) + ": ";
  size_t cells = 0;
  if (const char* why = map_df_box_check(box, &cells)) return fail(REVO_ERR_INVALID_ARG, who + why);
  if (n < 1 || n > CARVE_MAX_VIEWS) return fail(REVO_ERR_INVALID_ARG, who + "n must be 1 .. 64 views");
  TRY(map_check_side(device_in, "device_in"));
  TRY(map_check_side(device_tsdf, "device_tsdf"));
  if (device_tsdf) TRY(map_check_aligned((uintptr_t)tsdf | (uintptr_t)info | (uintptr_t)view_info, 16, "a device output is"));
  if (device_tsdf && with_color) TRY(map_check_aligned((uintptr_t)color | (uintptr_t)cinfo, 16, "a device output is"));
  revo_map_tsdf_params pp;
  if (const char* why = tsdf_params_check(prm, m->voxel, &pp)) return fail(REVO_ERR_INVALID_ARG, who + why);
  MapTsdfViews v;
  TRY(map_tsdf_views_begin(m, who, cells, n, views, with_color ? bgr : nullptr, device_in, device_tsdf, &v));
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t vinfo_bytes = sizeof(revo_map_carve_view_info) * (size_t)n, vol_bytes = sizeof(revo_map_tsdf_cell) * cells;
  const size_t col_bytes = sizeof(revo_map_tsdf_color) * cells;
  TsdfFuseK a{};
  a.views = v.views; a.n = n;
  a.accumulate = pp.accumulate;
  a.trunc = pp.trunc; a.voxel = m->voxel;
  a.box = *box;
  a.cells = (unsigned)cells;
  a.tsdf = device_tsdf ? (int2*)tsdf : (int2*)m->tsdfvol.p;
  a.info = device_tsdf && info ? (u64*)info : (u64*)m->tsdfcnt.p;
  a.vinfo = device_tsdf && view_info ? (unsigned*)view_info : (unsigned*)(m->tsdfcnt.p + 256);
  TsdfColorK col{};
  if (with_color) {
    col.bgr = v.bgr;
    col.color = device_tsdf ? (uint4*)color : (uint4*)m->tsdfcol.p;
    col.info = device_tsdf && cinfo ? (u64*)cinfo : (u64*)(m->tsdfcnt.p + 64);
    if (!device_tsdf && pp.accumulate) HIPCHECK(hipMemcpyAsync(col.color, color, col_bytes, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(col.info, 0, sizeof(revo_map_tsdf_color_info), s));
  }
  if (!device_tsdf && pp.accumulate) HIPCHECK(hipMemcpyAsync(a.tsdf, tsdf, vol_bytes, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemsetAsync(a.info, 0, sizeof(revo_map_tsdf_info), s));
  HIPCHECK(hipMemsetAsync(a.vinfo, 0, vinfo_bytes, s));
  const dim3 grid(cell_run_blocks(cells));
  if (with_color) hipLaunchKernelGGL(k_tsdf_fuse<true>, grid, dim3(CELL_RUN_THREADS), 0, s, a, col);
  else hipLaunchKernelGGL(k_tsdf_fuse<false>, grid, dim3(CELL_RUN_THREADS), 0, s, a, col);
  HIPCHECK(hipGetLastError());
  if (!device_tsdf) {
    HIPCHECK(hipMemcpyAsync(tsdf, a.tsdf, vol_bytes, hipMemcpyDeviceToHost, s));
    if (info) HIPCHECK(hipMemcpyAsync(info, a.info, sizeof(revo_map_tsdf_info), hipMemcpyDeviceToHost, s));
    if (view_info) HIPCHECK(hipMemcpyAsync(view_info, a.vinfo, vinfo_bytes, hipMemcpyDeviceToHost, s));
    if (with_color) {
      HIPCHECK(hipMemcpyAsync(color, col.color, col_bytes, hipMemcpyDeviceToHost, s));
      if (cinfo) HIPCHECK(hipMemcpyAsync(cinfo, col.info, sizeof(revo_map_tsdf_color_info), hipMemcpyDeviceToHost, s));
    }
  }
  if (!device_tsdf || v.uploaded) HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_tsdf_fuse(revo_map* m, const revo_map_df_box* box, int n, const revo_map_carve_view* views, int device_in,
                                  const revo_map_tsdf_params* prm, revo_map_tsdf_cell* tsdf, int device_tsdf, revo_map_tsdf_info* info,
                                  revo_map_carve_view_info* view_info) {
  return tsdf_fuse_core("revo_map_tsdf_fuse", false, m, box, n, views, nullptr, device_in, prm, tsdf, nullptr, device_tsdf, info, nullptr, view_info);
}

extern "C" int revo_map_tsdf_fuse_color(revo_map* m, const revo_map_df_box* box, int n, const revo_map_carve_view* views,
                                        const uint8_t* const* bgr, int device_in, const revo_map_tsdf_params* prm,
                                        revo_map_tsdf_cell* tsdf, revo_map_tsdf_color* color, int device_tsdf, revo_map_tsdf_info* info,
                                        revo_map_tsdf_color_info* color_info, revo_map_carve_view_info* view_info) {
  return tsdf_fuse_core("revo_map_tsdf_fuse_color", true, m, box, n, views, bgr, device_in, prm, tsdf, color, device_tsdf, info, color_info,
                        view_info);
}

// ----------------------------------------------------------------------------------------------------------------- the mesh --
// The scratch of a call, all in m->meshwork: a byte per cell (bit 0 valid, bit 1 inside), a word per cell (below), a pair of
// totals per block of 256 cells -- after the scan the vertices and triangles before the block --, and the counter line.
// A cell's word: bits 0 .. 6 the types of the edges at the cell that carry a vertex, bit 7 the cell's cube is active, bits
// 8 .. 18 the vertices of the block before the cell (< 7 * 256), bits 19 .. 30 the triangles of the block before it (< 12 * 256).
enum { MI_CELLS = 0, MI_VALID = 1, MI_INSIDE = 2, MI_CUBES = 3, MI_ACTIVE = 4, MI_VERTICES = 5, MI_TRIANGLES = 6 };
static_assert(sizeof(revo_map_mesh_info) == 64 && offsetof(revo_map_mesh_info, valid) == 8 * MI_VALID && offsetof(revo_map_mesh_info, inside) == 8 * MI_INSIDE &&
              offsetof(revo_map_mesh_info, cubes_active) == 8 * MI_ACTIVE && offsetof(revo_map_mesh_info, vertices) == 8 * MI_VERTICES &&
              offsetof(revo_map_mesh_info, triangles) == 8 * MI_TRIANGLES && offsetof(revo_map_mesh_info, reserved) == 56, "the info record is the counter line");
#define MESH_ACTIVE 0x80u
#define MESH_VLOCAL(w) (((w) >> 8) & 0x7ffu)
#define MESH_TLOCAL(w) (((w) >> 19) & 0xfffu)

struct MeshK {
  const int2* tsdf;
  revo_map_df_box box;
  unsigned cells, min_weight, blocks;
  float voxel;
  uint8_t* flags;
  unsigned* words;
  uint2* totals;   // per block: vertices, triangles; exclusive prefixes behind k_mesh_scan
  u64* info;
  float* vertices;
  unsigned* triangles;
};

// The exclusive prefix of v over the block's threads and the block's total; s_w: one word per wave.
template <int WAVES>
__device__ __forceinline__ unsigned mesh_block_scan(unsigned v, unsigned* s_w, unsigned* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  unsigned base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const unsigned x = s_w[w];
    base += w < wave ? x : 0u;
    tot += x;
  }
  __syncthreads();  // s_w may be written again
  *total = tot;
  return base + inc - v;
}

// One thread per cell: what the cell says, as a byte.
__global__ void __launch_bounds__(256) k_mesh_flags(const MeshK a) {
  __shared__ unsigned s_cnt[2];
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const unsigned c = blockIdx.x * 256u + threadIdx.x;
  bool valid = false, inside = false;
  if (c < a.cells) {
    const int2 v = a.tsdf[c];
    valid = tsdf_valid((unsigned)v.y, a.min_weight);
    inside = tsdf_inside(v.x, (unsigned)v.y, a.min_weight);
    a.flags[c] = (uint8_t)((valid ? 1u : 0u) | (inside ? 2u : 0u));
  }
  const unsigned nv = (unsigned)__popcll(__ballot(valid)), ni = (unsigned)__popcll(__ballot(inside));
  if ((threadIdx.x & 63) == 0) {
    if (nv) atomicAdd(&s_cnt[0], nv);
    if (ni) atomicAdd(&s_cnt[1], ni);
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&a.info[MI_VALID + threadIdx.x], (u64)s_cnt[threadIdx.x]);
}

// the bit of the neighbour at the offset (dx, dy, dz), each in -1 .. 1, in a cell's 27-neighbourhood masks
__device__ __forceinline__ constexpr unsigned mesh_nb_bit(int dx, int dy, int dz) { return 1u << ((dx + 1) * 9 + (dy + 1) * 3 + (dz + 1)); }
// the neighbourhood bits of the corners of the cube at cell - o (o: a corner number)
__device__ __forceinline__ constexpr unsigned mesh_cube_bits(unsigned o) {
  unsigned m = 0;
  for (unsigned e = 0; e < 8; ++e) m |= mesh_nb_bit((int)(e & 1) - (int)(o & 1), (int)((e >> 1) & 1) - (int)((o >> 1) & 1), (int)((e >> 2) & 1) - (int)((o >> 2) & 1));
  return m;
}
__device__ __forceinline__ constexpr unsigned mesh_corner_bit(unsigned v) { return mesh_nb_bit((int)(v & 1), (int)((v >> 1) & 1), (int)((v >> 2) & 1)); }
// the case code of the tetrahedron k of the cube whose corners' inside flags are the bits of `in8` (bit v: corner v)
__device__ __forceinline__ unsigned mesh_tetra_code(unsigned in8, int k) {
  const unsigned v12 = tsdf_tetra_v12(k);
  return (in8 & 1u) | (((in8 >> (v12 & 7u)) & 1u) << 1) | (((in8 >> (v12 >> 4)) & 1u) << 2) | (((in8 >> 7) & 1u) << 3);
}

// One thread per cell.  The bytes of the cell's 27-neighbourhood (0 outside the box) go into two masks; from them the eight
// cubes the cell is a corner of are active or not, an edge at the cell carries a vertex or not, and the cell's own cube has its
// triangles counted.  The block's prefix sums go into the cell's word, its totals into the block's pair.
__global__ void __launch_bounds__(256) k_mesh_count(const MeshK a) {
  __shared__ unsigned s_w[4];
  const unsigned c = blockIdx.x * 256u + threadIdx.x;
  const int nx = a.box.n[0], ny = a.box.n[1], nz = a.box.n[2];
  unsigned mask = 0, active = 0, ntri = 0;
  if (c < a.cells) {
    const unsigned line = c / (unsigned)nz;
    const int iz = (int)(c - line * (unsigned)nz), ix = (int)(line / (unsigned)ny), iy = (int)(line - (unsigned)ix * (unsigned)ny);
    unsigned vmask = 0, imask = 0;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz) {
          const int x = ix + dx, y = iy + dy, z = iz + dz;
          if (x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz) {
            const unsigned f = a.flags[((size_t)x * ny + y) * nz + z];
            vmask |= (f & 1u) ? mesh_nb_bit(dx, dy, dz) : 0u;
            imask |= (f & 2u) ? mesh_nb_bit(dx, dy, dz) : 0u;
          }
        }
    unsigned cubes = 0;  // bit o: the cube at cell - o is active
#pragma unroll
    for (unsigned o = 0; o < 8; ++o) cubes |= (vmask & mesh_cube_bits(o)) == mesh_cube_bits(o) ? 1u << o : 0u;
    const bool in0 = (imask & mesh_corner_bit(0)) != 0;
#pragma unroll
    for (unsigned t = 0; t < 7; ++t) {
      unsigned owners = 0;
#pragma unroll
      for (unsigned o = 0; o < 8; ++o) owners |= tsdf_edge_in_cube(t, o) ? 1u << o : 0u;
      const bool in1 = (imask & mesh_corner_bit(t + 1u)) != 0;
      mask |= (in0 != in1 && (cubes & owners)) ? 1u << t : 0u;
    }
    active = cubes & 1u;
    if (active) {
      unsigned in8 = 0;
#pragma unroll
      for (unsigned v = 0; v < 8; ++v) in8 |= (imask & mesh_corner_bit(v)) ? 1u << v : 0u;
#pragma unroll
      for (int k = 0; k < 6; ++k) ntri += (unsigned)tsdf_case_count(mesh_tetra_code(in8, k));
    }
  }
  unsigned vtot = 0, ttot = 0;
  const unsigned vloc = mesh_block_scan<4>((unsigned)__popc(mask), s_w, &vtot);
  const unsigned tloc = mesh_block_scan<4>(ntri, s_w, &ttot);
  if (c < a.cells) a.words[c] = mask | (active ? MESH_ACTIVE : 0u) | (vloc << 8) | (tloc << 19);
  if (threadIdx.x == 0) a.totals[blockIdx.x] = make_uint2(vtot, ttot);
  const unsigned na = (unsigned)__popcll(__ballot(active != 0u));
  if ((threadIdx.x & 63) == 0 && na) atomicAdd(&a.info[MI_ACTIVE], (u64)na);
}

// One block: the exclusive prefix sums of the blocks' totals in place, 1024 at a time behind a running carry, and the two sums
// (at most 7 * 2^27 vertices and 12 * 2^27 triangles: they fit 32 bits) into the counter line.
__global__ void __launch_bounds__(1024) k_mesh_scan(const MeshK a) {
  __shared__ unsigned s_w[16];
  unsigned vcarry = 0, tcarry = 0;
  for (unsigned base = 0; base < a.blocks; base += 1024u) {
    const unsigned i = base + threadIdx.x;
    const uint2 t = i < a.blocks ? a.totals[i] : make_uint2(0u, 0u);
    unsigned vtot = 0, ttot = 0;
    const unsigned vex = mesh_block_scan<16>(t.x, s_w, &vtot);
    const unsigned tex = mesh_block_scan<16>(t.y, s_w, &ttot);
    if (i < a.blocks) a.totals[i] = make_uint2(vcarry + vex, tcarry + tex);
    vcarry += vtot;
    tcarry += ttot;
  }
  if (threadIdx.x == 0) { a.info[MI_VERTICES] = (u64)vcarry; a.info[MI_TRIANGLES] = (u64)tcarry; }
}

// One thread per cell: the vertices of the cell's edges, in the order of their types, at the cell's place in the list.
__global__ void __launch_bounds__(256) k_mesh_vertices(const MeshK a) {
  const unsigned c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.cells) return;
  const unsigned w = a.words[c], mask = w & 0x7fu;
  if (!mask) return;
  const unsigned ny = (unsigned)a.box.n[1], nz = (unsigned)a.box.n[2];
  const unsigned line = c / nz, iz = c - line * nz, ix = line / ny, iy = line - ix * ny;
  size_t at = (size_t)a.totals[blockIdx.x].x + MESH_VLOCAL(w);
  const int2 lo = a.tsdf[c];
#pragma unroll
  for (unsigned t = 0; t < 7; ++t) {
    if (!((mask >> t) & 1u)) continue;
    const unsigned d = t + 1u;  // the edge's end: inside the box, since an active cube holds the edge
    const int2 hi = a.tsdf[(size_t)c + ((d & 1u) ? (size_t)ny * nz : 0) + ((d & 2u) ? nz : 0u) + ((d & 4u) ? 1u : 0u)];
    const float al = tsdf_edge_alpha(lo.x, (unsigned)lo.y, hi.x, (unsigned)hi.y);
    float* out = a.vertices + 3 * at;
    out[0] = tsdf_vertex_axis(a.box.lo[0], (int)ix, (d & 1u) != 0, al, a.voxel);
    out[1] = tsdf_vertex_axis(a.box.lo[1], (int)iy, (d & 2u) != 0, al, a.voxel);
    out[2] = tsdf_vertex_axis(a.box.lo[2], (int)iz, (d & 4u) != 0, al, a.voxel);
    ++at;
  }
}

struct MeshAttrK {  // what k_mesh_attr takes beside MeshK
  const uint4* color;  // NULL: no colours
  float* normals;      // 3 floats per vertex, or NULL
  uint8_t* colors;     // 4 bytes per vertex, or NULL
};

// The field at the cell (x, y, z) and whether the cell is valid; a cell outside the box is not, and is not read.
__device__ __forceinline__ bool mesh_field(const MeshK& a, int x, int y, int z, float* f) {
  *f = 0.0f;
  if (x < 0 || x >= a.box.n[0] || y < 0 || y >= a.box.n[1] || z < 0 || z >= a.box.n[2]) return false;
  const int2 v = a.tsdf[((size_t)x * (unsigned)a.box.n[1] + (unsigned)y) * (unsigned)a.box.n[2] + (unsigned)z];
  if (!tsdf_valid((unsigned)v.y, a.min_weight)) return false;
  *f = tsdf_field(v.x, (unsigned)v.y);
  return true;
}
// The gradient at the valid cell (x, y, z) whose field is fc.
__device__ __forceinline__ void mesh_gradient(const MeshK& a, int x, int y, int z, float fc, float* gx, float* gy, float* gz) {
  float fm = 0.0f, fp = 0.0f;
  bool vm = mesh_field(a, x - 1, y, z, &fm), vp = mesh_field(a, x + 1, y, z, &fp);
  *gx = tsdf_grad_axis(vm, fm, fc, vp, fp);
  vm = mesh_field(a, x, y - 1, z, &fm); vp = mesh_field(a, x, y + 1, z, &fp);
  *gy = tsdf_grad_axis(vm, fm, fc, vp, fp);
  vm = mesh_field(a, x, y, z - 1, &fm); vp = mesh_field(a, x, y, z + 1, &fp);
  *gz = tsdf_grad_axis(vm, fm, fc, vp, fp);
}

// One thread per cell, as k_mesh_vertices: the normals and colours of the vertices of the cell's edges, in the order of their
// types, at the cell's place in the list.  The neighbourhoods of the edge's two ends are read from the volume directly.
__global__ void __launch_bounds__(256) k_mesh_attr(const MeshK a, const MeshAttrK b) {
  const unsigned c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.cells) return;
  const unsigned w = a.words[c], mask = w & 0x7fu;
  if (!mask) return;
  const unsigned ny = (unsigned)a.box.n[1], nz = (unsigned)a.box.n[2];
  const unsigned line = c / nz, iz = c - line * nz, ix = line / ny, iy = line - ix * ny;
  size_t at = (size_t)a.totals[blockIdx.x].x + MESH_VLOCAL(w);
  const int2 lo = a.tsdf[c];
  float g0x = 0.0f, g0y = 0.0f, g0z = 0.0f;
  if (b.normals) mesh_gradient(a, (int)ix, (int)iy, (int)iz, tsdf_field(lo.x, (unsigned)lo.y), &g0x, &g0y, &g0z);
  uint4 c0 = make_uint4(0u, 0u, 0u, 0u);
  if (b.colors) c0 = b.color[c];
#pragma unroll
  for (unsigned t = 0; t < 7; ++t) {
    if (!((mask >> t) & 1u)) continue;
    const unsigned d = t + 1u;  // the edge's end: inside the box and valid, since an active cube holds the edge
    const size_t e = (size_t)c + ((d & 1u) ? (size_t)ny * nz : 0) + ((d & 2u) ? nz : 0u) + ((d & 4u) ? 1u : 0u);
    const int2 hi = a.tsdf[e];
    const float al = tsdf_edge_alpha(lo.x, (unsigned)lo.y, hi.x, (unsigned)hi.y);
    if (b.normals) {
      float g1x, g1y, g1z, nx, nyv, nzv;
      mesh_gradient(a, (int)(ix + (d & 1u)), (int)(iy + ((d >> 1) & 1u)), (int)(iz + ((d >> 2) & 1u)), tsdf_field(hi.x, (unsigned)hi.y), &g1x, &g1y, &g1z);
      tsdf_normal(tsdf_lerp(g0x, g1x, al), tsdf_lerp(g0y, g1y, al), tsdf_lerp(g0z, g1z, al), &nx, &nyv, &nzv);
      float* out = b.normals + 3 * at;
      out[0] = nx; out[1] = nyv; out[2] = nzv;
    }
    if (b.colors) {
      const uint4 c1 = b.color[e];
      uchar4 px;
      px.x = tsdf_color_byte(c0.x, c0.w, c1.x, c1.w, al);
      px.y = tsdf_color_byte(c0.y, c0.w, c1.y, c1.w, al);
      px.z = tsdf_color_byte(c0.z, c0.w, c1.z, c1.w, al);
      px.w = (uint8_t)tsdf_color_k(c0.w, c1.w);
      ((uchar4*)b.colors)[at] = px;
    }
    ++at;
  }
}

// the corner number of v_i of the tetrahedron whose v1, v2 are packed in v12
__device__ __forceinline__ unsigned mesh_corner(unsigned v12, unsigned i) { return i == 0u ? 0u : i == 1u ? (v12 & 7u) : i == 2u ? (v12 >> 4) : 7u; }
// The index of the vertex on the edge between the corners lo and hi (lo's bits among hi's) of the cube at the cell c: the base of
// lo's cell and the edges of lower type that carry a vertex there.
__device__ __forceinline__ unsigned mesh_vertex_index(const MeshK& a, unsigned c, unsigned lo, unsigned hi) {
  const unsigned nz = (unsigned)a.box.n[2], nyz = (unsigned)a.box.n[1] * nz;
  const unsigned e = c + ((lo & 1u) ? nyz : 0u) + ((lo & 2u) ? nz : 0u) + ((lo & 4u) ? 1u : 0u);
  const unsigned w = a.words[e];
  return a.totals[e >> 8].x + MESH_VLOCAL(w) + (unsigned)__popc(w & 0x7fu & ((1u << tsdf_edge_type(lo, hi)) - 1u));
}

// One thread per cell: the triangles of the cell's cube when it is active, tetrahedron by tetrahedron, at the cube's place in the
// list.  A vertex index is looked up from the word and the block's base of the cell at the edge's lower end.
__global__ void __launch_bounds__(256) k_mesh_triangles(const MeshK a) {
  const unsigned c = blockIdx.x * 256u + threadIdx.x;
  if (c >= a.cells) return;
  const unsigned w = a.words[c];
  if (!(w & MESH_ACTIVE)) return;
  const unsigned nz = (unsigned)a.box.n[2], nyz = (unsigned)a.box.n[1] * nz;
  unsigned in8 = 0;
#pragma unroll
  for (unsigned v = 0; v < 8; ++v)  // an active cube's corners are inside the box
    in8 |= (a.flags[(size_t)c + ((v & 1u) ? nyz : 0u) + ((v & 2u) ? nz : 0u) + ((v & 4u) ? 1u : 0u)] & 2u) ? 1u << v : 0u;
  if (in8 == 0u || in8 == 0xffu) return;
  size_t at = (size_t)a.totals[blockIdx.x].y + MESH_TLOCAL(w);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const unsigned code = mesh_tetra_code(in8, k), v12 = tsdf_tetra_v12(k);
    const int cnt = tsdf_case_count(code);
    const bool swap = (tsdf_swap_word(k) >> code) & 1u;
    for (int j = 0; j < cnt; ++j) {
      const unsigned tri = tsdf_case_triangle(code, j);
      unsigned idx0 = 0, idx1 = 0, idx2 = 0;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const unsigned e = (tri >> (4 * q)) & 15u;
        const unsigned id = mesh_vertex_index(a, c, mesh_corner(v12, e & 3u), mesh_corner(v12, e >> 2));
        if (q == 0) idx0 = id; else if (q == 1) idx1 = id; else idx2 = id;
      }
      unsigned* out = a.triangles + 3 * at;
      out[0] = idx0;
      out[1] = swap ? idx2 : idx1;
      out[2] = swap ? idx1 : idx2;
      ++at;
    }
  }
}

// Both mesh calls.  name: the entry point's, for its messages; revo_map_tsdf_mesh passes no colour volume, normals or colours.
static int tsdf_mesh_core(const char* name, revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf, const revo_map_tsdf_color* color,
                          int device_tsdf, uint32_t min_weight, float* vertices, float* normals, uint8_t* colors, size_t cap_vertices,
                          uint32_t* triangles, size_t cap_triangles, size_t* n_vertices, size_t* n_triangles, int device_out,
                          revo_map_mesh_info* info) {
  if (!m || !box || !tsdf || !n_vertices || !n_triangles) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (colors && !color) return fail(REVO_ERR_INVALID_ARG, std::string(name) + ": colours need the colour volume");
  size_t cells = 0;
  if (const char* why = map_df_box_check(box, &cells)) return fail(REVO_ERR_INVALID_ARG, std::string(name) + ": " + why);
  TRY(map_check_side(device_tsdf, "device_tsdf"));
  TRY(map_check_side(device_out, "device_out"));
  if (device_tsdf) TRY(map_check_aligned((uintptr_t)tsdf | (uintptr_t)color, 16, "the device volume is"));
  if (device_out) TRY(map_check_aligned((uintptr_t)vertices | (uintptr_t)triangles | (uintptr_t)normals | (uintptr_t)colors, 16, "a device output is"));
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t vol_bytes = sizeof(revo_map_tsdf_cell) * cells, blocks = (cells + 255) / 256;
  // the scratch: counter line | totals | words | flags
  const size_t off_totals = 256, off_words = off_totals + ((sizeof(uint2) * blocks + 255) & ~(size_t)255);
  const size_t off_flags = off_words + ((sizeof(unsigned) * cells + 255) & ~(size_t)255);
  TRY(m->meshwork.reserve(off_flags + cells, s));
  TRY(m->tsdfvol.reserve(device_tsdf ? 0 : vol_bytes, s));
  if (!device_tsdf) HIPCHECK(hipMemcpyAsync(m->tsdfvol.p, tsdf, vol_bytes, hipMemcpyHostToDevice, s));
  MeshAttrK b{};
  if (colors) {  // the colour volume is only read for them
    const size_t col_bytes = sizeof(revo_map_tsdf_color) * cells;
    TRY(m->tsdfcol.reserve(device_tsdf ? 0 : col_bytes, s));
    if (!device_tsdf) HIPCHECK(hipMemcpyAsync(m->tsdfcol.p, color, col_bytes, hipMemcpyHostToDevice, s));
    b.color = device_tsdf ? (const uint4*)color : (const uint4*)m->tsdfcol.p;
  }
  MeshK a{};
  a.tsdf = device_tsdf ? (const int2*)tsdf : (const int2*)m->tsdfvol.p;
  a.box = *box;
  a.cells = (unsigned)cells; a.min_weight = min_weight; a.blocks = (unsigned)blocks;
  a.voxel = m->voxel;
  a.info = (u64*)m->meshwork.p;
  a.totals = (uint2*)(m->meshwork.p + off_totals);
  a.words = (unsigned*)(m->meshwork.p + off_words);
  a.flags = (uint8_t*)(m->meshwork.p + off_flags);
  const dim3 grid((unsigned)blocks);
  HIPCHECK(hipMemsetAsync(a.info, 0, 64, s));
  hipLaunchKernelGGL(k_mesh_flags, grid, dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_mesh_count, grid, dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(1024), 0, s, a);
  HIPCHECK(hipGetLastError());
  u64 line[8];
  HIPCHECK(hipMemcpyAsync(line, a.info, sizeof(line), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  line[MI_CELLS] = cells;
  line[MI_CUBES] = (u64)(box->n[0] - 1) * (u64)(box->n[1] - 1) * (u64)(box->n[2] - 1);
  line[7] = 0;
  const size_t nv = (size_t)line[MI_VERTICES], nt = (size_t)line[MI_TRIANGLES];
  *n_vertices = nv;
  *n_triangles = nt;
  if (info) memcpy(info, line, sizeof(line));
  if (!vertices && !triangles && !normals && !colors) return REVO_OK;
  if (((vertices || normals || colors) && cap_vertices < nv) || (triangles && cap_triangles < nt))
    return fail(REVO_ERR_CAPACITY, "tsdf mesh: an output holds fewer vertices or triangles than the mesh has");
  // a host call's device outputs: vertices | triangles | normals | colours
  const size_t vbytes = (12 * nv + 255) & ~(size_t)255, tbytes = (12 * nt + 255) & ~(size_t)255;
  if (!device_out) TRY(m->meshout.reserve(vbytes + tbytes + (normals ? vbytes : 0) + (colors ? 4 * nv : 0), s));
  a.vertices = device_out ? vertices : (float*)m->meshout.p;
  a.triangles = device_out ? triangles : (unsigned*)(m->meshout.p + vbytes);
  b.normals = !normals ? nullptr : device_out ? normals : (float*)(m->meshout.p + vbytes + tbytes);
  b.colors = !colors ? nullptr : device_out ? colors : (uint8_t*)(m->meshout.p + vbytes + tbytes + (normals ? vbytes : 0));
  if ((normals || colors) && nv) {
    hipLaunchKernelGGL(k_mesh_attr, grid, dim3(256), 0, s, a, b);
    if (!device_out && normals) HIPCHECK(hipMemcpyAsync(normals, b.normals, 12 * nv, hipMemcpyDeviceToHost, s));
    if (!device_out && colors) HIPCHECK(hipMemcpyAsync(colors, b.colors, 4 * nv, hipMemcpyDeviceToHost, s));
  }
  if (vertices && nv) {
    hipLaunchKernelGGL(k_mesh_vertices, grid, dim3(256), 0, s, a);
    if (!device_out) HIPCHECK(hipMemcpyAsync(vertices, a.vertices, 12 * nv, hipMemcpyDeviceToHost, s));
  }
  if (triangles && nt) {
    hipLaunchKernelGGL(k_mesh_triangles, grid, dim3(256), 0, s, a);
    if (!device_out) HIPCHECK(hipMemcpyAsync(triangles, a.triangles, 12 * nt, hipMemcpyDeviceToHost, s));
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_tsdf_mesh(revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf, int device_tsdf, uint32_t min_weight,
                                  float* vertices, size_t cap_vertices, uint32_t* triangles, size_t cap_triangles, size_t* n_vertices,
                                  size_t* n_triangles, int device_out, revo_map_mesh_info* info) {
  return tsdf_mesh_core("revo_map_tsdf_mesh", m, box, tsdf, nullptr, device_tsdf, min_weight, vertices, nullptr, nullptr, cap_vertices, triangles,
                        cap_triangles, n_vertices, n_triangles, device_out, info);
}

extern "C" int revo_map_tsdf_mesh_attr(revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf, const revo_map_tsdf_color* color,
                                       int device_tsdf, uint32_t min_weight, float* vertices, float* normals, uint8_t* colors, size_t cap_vertices,
                                       uint32_t* triangles, size_t cap_triangles, size_t* n_vertices, size_t* n_triangles, int device_out,
                                       revo_map_mesh_info* info) {
  return tsdf_mesh_core("revo_map_tsdf_mesh_attr", m, box, tsdf, color, device_tsdf, min_weight, vertices, normals, colors, cap_vertices, triangles,
                        cap_triangles, n_vertices, n_triangles, device_out, info);
}
