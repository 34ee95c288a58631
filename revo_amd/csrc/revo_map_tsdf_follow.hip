// revo_map_tsdf_follow.hip -- a box that follows the camera: revo_map_tsdf_shift, the surface volumes of a box moved
// out of place into the volumes of the shifted box, with the cells that leave as records in ascending key order, and
// revo_map_tsdf_refill, records added back into the cells of a box, all or nothing.  Contracts: include/revo_hip.h; the rules both
// sides share (the staying sub-box, a leaving cell's rank and its inverse, EMPTY, FITS): revo_tsdf_follow_host.h.  Every value is an
// integer; the order of the records comes from a scan over the leaving cells in place order.
#include "revo_map_impl.h"
#include "revo_tsdf_follow_host.h"

#define FOLLOW_RUN 4  // consecutive destination cells of a thread: two 16-byte words of the volume, as k_tsdf_fuse's

enum { FI_CELLS = 0, FI_STAYING = 1, FI_LEAVING = 2, FI_RECORDS = 3, FI_DROPPED = 4 };
enum { RI_APPLIED = 0, RI_ORDER = 1, RI_COLOR = 2, RI_FIT = 3 };  // the refill's counter line

static_assert(sizeof(revo_map_tsdf_record) == 32 && offsetof(revo_map_tsdf_record, sum) == 8 && offsetof(revo_map_tsdf_record, weight) == 12 &&
              offsetof(revo_map_tsdf_record, sum_b) == 16 && offsetof(revo_map_tsdf_record, color_weight) == 28 && sizeof(ulonglong2) == 16,
              "a record is two 16-byte words");
static_assert(sizeof(revo_map_tsdf_shift_info) == 64 && offsetof(revo_map_tsdf_shift_info, staying) == 8 * FI_STAYING &&
              offsetof(revo_map_tsdf_shift_info, leaving) == 8 * FI_LEAVING && offsetof(revo_map_tsdf_shift_info, records) == 8 * FI_RECORDS &&
              offsetof(revo_map_tsdf_shift_info, dropped) == 8 * FI_DROPPED && offsetof(revo_map_tsdf_shift_info, reserved) == 40,
              "the info record is the kernel's counter line");
static_assert(sizeof(revo_map_tsdf_refill_info) == 32 && offsetof(revo_map_tsdf_refill_info, applied) == 8 && offsetof(revo_map_tsdf_refill_info, outside) == 16,
              "the refill's info record is the documented layout");
static_assert(sizeof(revo_map_tsdf_cell) == 8 && sizeof(int2) == 8 && sizeof(revo_map_tsdf_color) == 16 && sizeof(uint4) == 16, "the cells are one word each");

struct FollowK {
  FollowShift f;
  int lo[3];             // the source box's first voxel index
  const int2* src;       // 16-byte aligned
  const uint4* scol;     // NULL: no colour volume
  int2* dst;             // 16-byte aligned: thread t owns the cells 4 t .. 4 t + 3
  uint4* dcol;
  unsigned cells, leaving;  // both at most 2^27
  unsigned blocks;          // of 256 leaving cells
  unsigned drop;            // the records the count finds are dropped ones too
  unsigned* totals;         // per block: its records; exclusive prefixes behind k_follow_scan
  u64* info;                // one 64-byte line: revo_map_tsdf_shift_info
  ulonglong2* records;
};

// The exclusive prefix of v over the block's threads and the block's total; s_w: one word per wave.
template <int WAVES>
__device__ __forceinline__ unsigned follow_block_scan(unsigned v, unsigned* s_w, unsigned* total) {
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

// The move.  One thread per run of FOLLOW_RUN destination cells that follow each other in memory (z fastest; consecutive lanes take
// consecutive runs).  A destination cell that receives a source cell reads it once; every destination cell is written once, an
// entering one as zeros by the same launch.  Where the four source cells follow each other from a 16-byte boundary (delta_z and n[2]
// multiples of four give that for every run) they are read as two 16-byte words, otherwise as 8-byte cells; a colour cell is one
// 16-byte word either way.  The tail of a volume whose cells are no multiple of four is written cell by cell.
__global__ void __launch_bounds__(256) k_follow_move(const FollowK a) {
  const size_t c0 = (size_t)(blockIdx.x * 256u + threadIdx.x) * FOLLOW_RUN;
  if (c0 >= a.cells) return;
  const unsigned n1 = (unsigned)a.f.n[1], n2 = (unsigned)a.f.n[2];
  const unsigned line = (unsigned)c0 / n2;
  int z = (int)((unsigned)c0 - line * n2), x = (int)(line / n1), y = (int)(line - (unsigned)x * n1);
  bool valid[FOLLOW_RUN], stay[FOLLOW_RUN];
  size_t src[FOLLOW_RUN];
#pragma unroll
  for (int j = 0; j < FOLLOW_RUN; ++j) {
    valid[j] = c0 + j < a.cells;
    stay[j] = valid[j] && follow_receives(a.f, x, y, z);
    src[j] = stay[j] ? ((size_t)(x + a.f.d[0]) * n1 + (size_t)(y + a.f.d[1])) * n2 + (size_t)(z + a.f.d[2]) : 0;
    if (++z == (int)n2) {
      z = 0;
      if (++y == (int)n1) { y = 0; ++x; }
    }
  }
  int2 v[FOLLOW_RUN];
  const bool run = stay[0] && stay[1] && stay[2] && stay[3] && src[1] == src[0] + 1 && src[2] == src[0] + 2 && src[3] == src[0] + 3 && !(src[0] & 1);
  if (run) {
    const int4 lo = *(const int4*)(a.src + src[0]), hi = *(const int4*)(a.src + src[0] + 2);
    v[0] = make_int2(lo.x, lo.y); v[1] = make_int2(lo.z, lo.w);
    v[2] = make_int2(hi.x, hi.y); v[3] = make_int2(hi.z, hi.w);
  } else {
#pragma unroll
    for (int j = 0; j < FOLLOW_RUN; ++j) v[j] = stay[j] ? a.src[src[j]] : make_int2(0, 0);
  }
  if (valid[FOLLOW_RUN - 1]) {  // the four cells exist, and dst + c0 is 16-byte aligned
    *(int4*)(a.dst + c0) = make_int4(v[0].x, v[0].y, v[1].x, v[1].y);
    *(int4*)(a.dst + c0 + 2) = make_int4(v[2].x, v[2].y, v[3].x, v[3].y);
  } else {
#pragma unroll
    for (int j = 0; j < FOLLOW_RUN; ++j)
      if (valid[j]) a.dst[c0 + j] = v[j];
  }
  if (a.scol) {
#pragma unroll
    for (int j = 0; j < FOLLOW_RUN; ++j)
      if (valid[j]) a.dcol[c0 + j] = stay[j] ? a.scol[src[j]] : make_uint4(0u, 0u, 0u, 0u);
  }
}

// The leaving cell of rank r: its place in the source box, and whether it is EMPTY.
__device__ __forceinline__ bool follow_leaving_cell(const FollowK& a, unsigned r, size_t* place, int2* v, uint4* col) {
  *place = (size_t)follow_leaving_place(a.f, (uint64_t)r);
  *v = a.src[*place];
  *col = a.scol ? a.scol[*place] : make_uint4(0u, 0u, 0u, 0u);
  return !follow_empty(v->x, (unsigned)v->y, col->x, col->y, col->z, col->w);
}

// One thread per leaving cell, in place order: the block's records into its total; the call's into the counter line -- a wave sum,
// one LDS atomic per wave, one global atomic per block.
__global__ void __launch_bounds__(256) k_follow_count(const FollowK a) {
  __shared__ unsigned s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const unsigned r = blockIdx.x * 256u + threadIdx.x;
  bool rec = false;
  if (r < a.leaving) {
    size_t place; int2 v; uint4 col;
    rec = follow_leaving_cell(a, r, &place, &v, &col);
  }
  const unsigned cnt = (unsigned)__popcll(__ballot(rec));
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (blockIdx.x < a.blocks) a.totals[blockIdx.x] = s_cnt;
    if (s_cnt) {
      atomicAdd(&a.info[FI_RECORDS], (u64)s_cnt);
      if (a.drop) atomicAdd(&a.info[FI_DROPPED], (u64)s_cnt);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 64) {
    a.info[FI_CELLS] = follow_cells(a.f);
    a.info[FI_STAYING] = follow_staying(a.f);
    a.info[FI_LEAVING] = follow_leaving(a.f);
  }
}

// One block: the exclusive prefix sums of the blocks' totals in place, 1024 at a time behind a running carry.
__global__ void __launch_bounds__(1024) k_follow_scan(const FollowK a) {
  __shared__ unsigned s_w[16];
  unsigned carry = 0;
  for (unsigned base = 0; base < a.blocks; base += 1024u) {
    const unsigned i = base + threadIdx.x;
    const unsigned t = i < a.blocks ? a.totals[i] : 0u;
    unsigned tot = 0;
    const unsigned ex = follow_block_scan<16>(t, s_w, &tot);
    if (i < a.blocks) a.totals[i] = carry + ex;
    carry += tot;
  }
}

// One thread per leaving cell, as k_follow_count: the record of a cell that is not EMPTY, at the block's base plus the cell's place
// among the block's records.
__global__ void __launch_bounds__(256) k_follow_emit(const FollowK a) {
  __shared__ unsigned s_w[4];
  const unsigned r = blockIdx.x * 256u + threadIdx.x;
  bool rec = false;
  size_t place = 0;
  int2 v = make_int2(0, 0);
  uint4 col = make_uint4(0u, 0u, 0u, 0u);
  if (r < a.leaving) rec = follow_leaving_cell(a, r, &place, &v, &col);
  unsigned tot = 0;
  const unsigned local = follow_block_scan<4>(rec ? 1u : 0u, s_w, &tot);
  if (!rec) return;
  const unsigned n1 = (unsigned)a.f.n[1], n2 = (unsigned)a.f.n[2];
  const unsigned line = (unsigned)place / n2, iz = (unsigned)place - line * n2, ix = line / n1, iy = line - ix * n1;
  const size_t at = (size_t)a.totals[blockIdx.x] + local;
  a.records[2 * at] = make_ulonglong2(follow_key(a.lo[0] + (int)ix, a.lo[1] + (int)iy, a.lo[2] + (int)iz), (u64)(unsigned)v.x | ((u64)(unsigned)v.y << 32));
  a.records[2 * at + 1] = make_ulonglong2((u64)col.x | ((u64)col.y << 32), (u64)col.z | ((u64)col.w << 32));
}

static bool follow_overlap(const void* p, const void* q, size_t bytes_p, size_t bytes_q) {
  if (!p || !q) return false;
  const uintptr_t x = (uintptr_t)p, y = (uintptr_t)q;
  return x < y + bytes_q && y < x + bytes_p;
}

extern "C" int revo_map_tsdf_shift(revo_map* m, const revo_map_df_box* box, const int32_t delta[3], const revo_map_tsdf_cell* src_tsdf,
                                   const revo_map_tsdf_color* src_color, revo_map_tsdf_cell* dst_tsdf, revo_map_tsdf_color* dst_color,
                                   int device_tsdf, revo_map_tsdf_record* records, size_t cap_records, size_t* n_records, int device_out,
                                   revo_map_tsdf_shift_info* info) {
  if (!m || !box || !delta || !src_tsdf || !dst_tsdf) return fail(REVO_ERR_INVALID_ARG, "null argument");
  const std::string who = "revo_map_tsdf_shift: ";
  if (!src_color != !dst_color) return fail(REVO_ERR_INVALID_ARG, who + "the colour volumes are both given or both NULL");
  if (records && !n_records) return fail(REVO_ERR_INVALID_ARG, who + "records need n_records");
  size_t cells = 0;
  if (const char* why = map_df_box_check(box, &cells)) return fail(REVO_ERR_INVALID_ARG, who + why);
  for (int k = 0; k < 3; ++k) {
    const long long l = (long long)box->lo[k] + delta[k];
    if (l < -(1 << 20) || l + box->n[k] - 1 > (1 << 20) - 1)
      return fail(REVO_ERR_INVALID_ARG, who + "the destination box leaves the voxel index range [-2^20, 2^20 - 1]");
  }
  TRY(map_check_side(device_tsdf, "device_tsdf"));
  TRY(map_check_side(device_out, "device_out"));
  const size_t vol_bytes = sizeof(revo_map_tsdf_cell) * cells, col_bytes = sizeof(revo_map_tsdf_color) * cells;
  if (follow_overlap(src_tsdf, dst_tsdf, vol_bytes, vol_bytes) || follow_overlap(src_tsdf, dst_color, vol_bytes, col_bytes) ||
      follow_overlap(src_color, dst_tsdf, col_bytes, vol_bytes) || follow_overlap(src_color, dst_color, col_bytes, col_bytes))
    return fail(REVO_ERR_INVALID_ARG, who + "source and destination overlap: the move is out of place");
  const bool drop = !records && !n_records, count_only = !records && n_records;  // otherwise: move and emit
  const bool waits = !drop || !device_tsdf;
  if (device_tsdf)
    TRY(map_check_aligned((uintptr_t)src_tsdf | (uintptr_t)src_color | (uintptr_t)dst_tsdf | (uintptr_t)dst_color, 16, "a device volume is"));
  if (device_out && records) TRY(map_check_aligned((uintptr_t)records, 16, "the device records are"));
  if (!waits) TRY(map_check_aligned((uintptr_t)info, 16, "the device info is"));
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  MapTsdfFollowScratch& w = m->tsdffol;
  FollowK a{};
  a.f = follow_shift(box->n, delta);
  for (int k = 0; k < 3; ++k) a.lo[k] = box->lo[k];
  a.cells = (unsigned)cells;
  a.leaving = (unsigned)follow_leaving(a.f);
  a.blocks = (a.leaving + 255u) / 256u;
  a.drop = drop ? 1u : 0u;
  TRY(w.work.reserve(256 + sizeof(unsigned) * (size_t)(a.blocks ? a.blocks : 1u), s));
  if (!device_tsdf) {
    TRY(m->tsdfvol.reserve(vol_bytes, s));
    if (src_color) TRY(m->tsdfcol.reserve(col_bytes, s));
    if (!count_only) {
      TRY(w.dst.reserve(vol_bytes, s));
      if (src_color) TRY(w.dstcol.reserve(col_bytes, s));
    }
    HIPCHECK(hipMemcpyAsync(m->tsdfvol.p, src_tsdf, vol_bytes, hipMemcpyHostToDevice, s));
    if (src_color) HIPCHECK(hipMemcpyAsync(m->tsdfcol.p, src_color, col_bytes, hipMemcpyHostToDevice, s));
  }
  a.src = device_tsdf ? (const int2*)src_tsdf : (const int2*)m->tsdfvol.p;
  a.scol = !src_color ? nullptr : device_tsdf ? (const uint4*)src_color : (const uint4*)m->tsdfcol.p;
  a.dst = device_tsdf ? (int2*)dst_tsdf : (int2*)w.dst.p;
  a.dcol = !src_color ? nullptr : device_tsdf ? (uint4*)dst_color : (uint4*)w.dstcol.p;
  a.totals = (unsigned*)(w.work.p + 256);
  a.info = !waits && info ? (u64*)info : (u64*)w.work.p;
  HIPCHECK(hipMemsetAsync(a.info, 0, sizeof(revo_map_tsdf_shift_info), s));
  hipLaunchKernelGGL(k_follow_count, dim3(a.blocks ? a.blocks : 1u), dim3(256), 0, s, a);
  if (!drop && a.blocks) hipLaunchKernelGGL(k_follow_scan, dim3(1), dim3(1024), 0, s, a);
  HIPCHECK(hipGetLastError());
  u64 line[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!drop) {
    HIPCHECK(hipMemcpyAsync(line, a.info, sizeof(line), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    const size_t nrec = (size_t)line[FI_RECORDS];
    *n_records = nrec;
    if (info) memcpy(info, line, sizeof(line));
    if (count_only) return REVO_OK;
    if (cap_records < nrec) return fail(REVO_ERR_CAPACITY, "tsdf shift: the records hold fewer cells than leave the box");
    if (nrec) {
      if (!device_out) TRY(w.recs.reserve(sizeof(revo_map_tsdf_record) * nrec, s));
      a.records = device_out ? (ulonglong2*)records : (ulonglong2*)w.recs.p;
      hipLaunchKernelGGL(k_follow_emit, dim3(a.blocks), dim3(256), 0, s, a);
      if (!device_out) HIPCHECK(hipMemcpyAsync(records, a.records, sizeof(revo_map_tsdf_record) * nrec, hipMemcpyDeviceToHost, s));
    }
  }
  const size_t runs = (cells + FOLLOW_RUN - 1) / FOLLOW_RUN;
  hipLaunchKernelGGL(k_follow_move, dim3((unsigned)((runs + 255) / 256)), dim3(256), 0, s, a);
  HIPCHECK(hipGetLastError());
  if (!device_tsdf) {
    HIPCHECK(hipMemcpyAsync(dst_tsdf, a.dst, vol_bytes, hipMemcpyDeviceToHost, s));
    if (src_color) HIPCHECK(hipMemcpyAsync(dst_color, a.dcol, col_bytes, hipMemcpyDeviceToHost, s));
    if (drop && info) HIPCHECK(hipMemcpyAsync(line, a.info, sizeof(line), hipMemcpyDeviceToHost, s));
  }
  if (waits) HIPCHECK(hipStreamSynchronize(s));
  if (drop && waits && info) memcpy(info, line, sizeof(line));
  return REVO_OK;
}

// ------------------------------------------------------------------------------------------------------------- the refill --
struct RefillK {
  int lo[3], n[3];
  int2* tsdf;
  uint4* color;  // NULL: no colour volume
  const ulonglong2* recs;
  size_t n_recs;
  u64* line;     // RI_*
};

// The record i and, when its key lies inside the box, its cell's place.
__device__ __forceinline__ bool refill_record(const RefillK& a, size_t i, ulonglong2* r0, ulonglong2* r1, size_t* place) {
  *r0 = a.recs[2 * i];
  *r1 = a.recs[2 * i + 1];
  int kx, ky, kz;
  follow_key_axes(r0->x, &kx, &ky, &kz);
  const int x = kx - a.lo[0], y = ky - a.lo[1], z = kz - a.lo[2];
  const bool in = !(r0->x >> 63) && (unsigned)x < (unsigned)a.n[0] && (unsigned)y < (unsigned)a.n[1] && (unsigned)z < (unsigned)a.n[2];
  *place = in ? ((size_t)x * (unsigned)a.n[1] + (unsigned)y) * (unsigned)a.n[2] + (unsigned)z : 0;
  return in;
}

// One thread per record: the order rule against the record before it, the colour rule, and for a record inside the box whether
// its cell FITS with the record added, in 64 bits.  Nothing is written but the counters.
__global__ void __launch_bounds__(256) k_refill_check(const RefillK a) {
  __shared__ unsigned s_cnt[4];
  if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  bool in = false, bad_order = false, bad_color = false, bad_fit = false;
  if (i < a.n_recs) {
    ulonglong2 r0, r1;
    size_t place;
    in = refill_record(a, i, &r0, &r1, &place);
    bad_order = (r0.x >> 63) != 0 || (i > 0 && a.recs[2 * (i - 1)].x >= r0.x);
    bad_color = !a.color && (r1.x | r1.y) != 0;
    if (in) {
      const int2 v = a.tsdf[place];
      const uint4 c = a.color ? a.color[place] : make_uint4(0u, 0u, 0u, 0u);
      bad_fit = !follow_fits((int64_t)v.x + (int64_t)(int32_t)(unsigned)r0.y, (uint64_t)(unsigned)v.y + (r0.y >> 32), (uint64_t)c.x + (r1.x & 0xffffffffu),
                             (uint64_t)c.y + (r1.x >> 32), (uint64_t)c.z + (r1.y & 0xffffffffu), (uint64_t)c.w + (r1.y >> 32));
    }
  }
  const unsigned n_in = (unsigned)__popcll(__ballot(in)), n_order = (unsigned)__popcll(__ballot(bad_order));
  const unsigned n_color = (unsigned)__popcll(__ballot(bad_color)), n_fit = (unsigned)__popcll(__ballot(bad_fit));
  if ((threadIdx.x & 63) == 0) {
    if (n_in) atomicAdd(&s_cnt[RI_APPLIED], n_in);
    if (n_order) atomicAdd(&s_cnt[RI_ORDER], n_order);
    if (n_color) atomicAdd(&s_cnt[RI_COLOR], n_color);
    if (n_fit) atomicAdd(&s_cnt[RI_FIT], n_fit);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&a.line[threadIdx.x], (u64)s_cnt[threadIdx.x]);
}

// One thread per record, behind a check that refused nothing: keys are unique, so a cell is read and written by one thread.
__global__ void __launch_bounds__(256) k_refill_apply(const RefillK a) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= a.n_recs) return;
  ulonglong2 r0, r1;
  size_t place;
  if (!refill_record(a, i, &r0, &r1, &place)) return;
  const int2 v = a.tsdf[place];
  a.tsdf[place] = make_int2((int)((unsigned)v.x + (unsigned)r0.y), (int)((unsigned)v.y + (unsigned)(r0.y >> 32)));
  if (a.color) {
    const uint4 c = a.color[place];
    a.color[place] = make_uint4(c.x + (unsigned)r1.x, c.y + (unsigned)(r1.x >> 32), c.z + (unsigned)r1.y, c.w + (unsigned)(r1.y >> 32));
  }
}

extern "C" int revo_map_tsdf_refill(revo_map* m, const revo_map_df_box* box, revo_map_tsdf_cell* tsdf, revo_map_tsdf_color* color, int device_tsdf,
                                    size_t n, const revo_map_tsdf_record* records, int device_in, revo_map_tsdf_refill_info* info) {
  if (!m || !box || !tsdf || (n && !records)) return fail(REVO_ERR_INVALID_ARG, "null argument");
  const std::string who = "revo_map_tsdf_refill: ";
  size_t cells = 0;
  if (const char* why = map_df_box_check(box, &cells)) return fail(REVO_ERR_INVALID_ARG, who + why);
  if (n > ((size_t)1 << 30)) return fail(REVO_ERR_INVALID_ARG, who + "n must be at most 2^30 records");
  TRY(map_check_side(device_tsdf, "device_tsdf"));
  TRY(map_check_side(device_in, "device_in"));
  if (device_tsdf) TRY(map_check_aligned((uintptr_t)tsdf | (uintptr_t)color, 16, "a device volume is"));
  if (device_in && n) TRY(map_check_aligned((uintptr_t)records, 16, "the device records are"));
  revo_map_tsdf_refill_info out{};
  out.records = n;
  if (!n) {
    if (info) *info = out;
    return REVO_OK;
  }
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  MapTsdfFollowScratch& w = m->tsdffol;
  const size_t vol_bytes = sizeof(revo_map_tsdf_cell) * cells, col_bytes = sizeof(revo_map_tsdf_color) * cells;
  TRY(w.work.reserve(256 + sizeof(unsigned), s));
  RefillK a{};
  for (int k = 0; k < 3; ++k) { a.lo[k] = box->lo[k]; a.n[k] = box->n[k]; }
  a.n_recs = n;
  a.line = (u64*)w.work.p;
  if (!device_in) {
    TRY(w.recs.reserve(sizeof(revo_map_tsdf_record) * n, s));
    HIPCHECK(hipMemcpyAsync(w.recs.p, records, sizeof(revo_map_tsdf_record) * n, hipMemcpyHostToDevice, s));
  }
  a.recs = device_in ? (const ulonglong2*)records : (const ulonglong2*)w.recs.p;
  if (!device_tsdf) {
    TRY(m->tsdfvol.reserve(vol_bytes, s));
    HIPCHECK(hipMemcpyAsync(m->tsdfvol.p, tsdf, vol_bytes, hipMemcpyHostToDevice, s));
    if (color) {
      TRY(m->tsdfcol.reserve(col_bytes, s));
      HIPCHECK(hipMemcpyAsync(m->tsdfcol.p, color, col_bytes, hipMemcpyHostToDevice, s));
    }
  }
  a.tsdf = device_tsdf ? (int2*)tsdf : (int2*)m->tsdfvol.p;
  a.color = !color ? nullptr : device_tsdf ? (uint4*)color : (uint4*)m->tsdfcol.p;
  const dim3 grid((unsigned)((n + 255) / 256));
  HIPCHECK(hipMemsetAsync(a.line, 0, 64, s));
  hipLaunchKernelGGL(k_refill_check, grid, dim3(256), 0, s, a);
  HIPCHECK(hipGetLastError());
  u64 line[8];
  HIPCHECK(hipMemcpyAsync(line, a.line, sizeof(line), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (line[RI_ORDER]) return fail(REVO_ERR_INVALID_ARG, who + "the records are not in strictly ascending key order (or a key has bit 63 set)");
  if (line[RI_COLOR]) return fail(REVO_ERR_INVALID_ARG, who + "a record carries colour words and there is no colour volume");
  if (line[RI_FIT]) return fail(REVO_ERR_INVALID_ARG, who + "a cell would pass the sums a fuse can reach");
  out.applied = line[RI_APPLIED];
  out.outside = n - out.applied;
  if (info) *info = out;
  if (!out.applied) return REVO_OK;
  hipLaunchKernelGGL(k_refill_apply, grid, dim3(256), 0, s, a);
  HIPCHECK(hipGetLastError());
  if (!device_tsdf) {
    HIPCHECK(hipMemcpyAsync(tsdf, a.tsdf, vol_bytes, hipMemcpyDeviceToHost, s));
    if (color) HIPCHECK(hipMemcpyAsync(color, a.color, col_bytes, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
  }
  return REVO_OK;
}
