// revo_map_field.hip -- the voxel map's distance field: the exact squared Euclidean distance, in cells, from every
// cell of a box of voxel indices to the nearest solid voxel inside the box (revo_map_distance_field), the index bounds of the
// solid voxels (revo_map_bounds) and point queries against a field (revo_map_df_sample).  Every value is an integer with one
// definition, so the bytes do not depend on the table, the order of integration or the launch.
//
// The field is built in the caller's buffer, in place: the table scan sets one bit per solid voxel of the box (atomicOr:
// order-free), pass z turns every z-line's bits into dz^2, passes y and x are the min-plus step d(i) = min_j (i - j)^2 + g(j)
// along their axis, and the last one writes the contract's values (clamp, REVO_DF_NONE) and feeds max_d2.
#include "revo_map_impl.h"
#include "revo_seen_host.h"

#include <climits>

#define DF_INF (1u << 30)  // "no solid voxel on this line so far": above 3 * 1023^2, and DF_INF + 1023^2 fits 32 bits
#define DF_MAX_N 1024
#define DF_MAX_CELLS (1ull << 27)
#define DF_MAX_POINTS (1ull << 24)
#define DF_TILE_WORDS 8192  // the LDS tile of a min-plus block: line length x strip width <= 8192 words (32 KB)

// info words: cells, solid, outside, below, max_d2 (revo_map_df_info), then unknown, known_free (revo_map_known_info)
enum { DF_CELLS = 0, DF_SOLID = 1, DF_OUTSIDE = 2, DF_BELOW = 3, DF_MAXD2 = 4, DF_UNKNOWN = 5, DF_KNOWN_FREE = 6 };

static_assert(sizeof(revo_map_df_box) == 24 && offsetof(revo_map_df_box, n) == 12, "the box is six 32-bit words");
static_assert(sizeof(revo_map_df_info) == 64 && offsetof(revo_map_df_info, cells) == 8 * DF_CELLS && offsetof(revo_map_df_info, solid) == 8 * DF_SOLID &&
              offsetof(revo_map_df_info, outside) == 8 * DF_OUTSIDE && offsetof(revo_map_df_info, below) == 8 * DF_BELOW &&
              offsetof(revo_map_df_info, max_d2) == 8 * DF_MAXD2 && offsetof(revo_map_df_info, reserved) == 40, "the info record is the kernels' counter line");
static_assert(sizeof(revo_map_known_info) == 64 && offsetof(revo_map_known_info, cells) == 8 * DF_CELLS && offsetof(revo_map_known_info, solid) == 8 * DF_SOLID &&
              offsetof(revo_map_known_info, outside) == 8 * DF_OUTSIDE && offsetof(revo_map_known_info, below) == 8 * DF_BELOW &&
              offsetof(revo_map_known_info, max_d2) == 8 * DF_MAXD2 && offsetof(revo_map_known_info, unknown) == 8 * DF_UNKNOWN &&
              offsetof(revo_map_known_info, known_free) == 8 * DF_KNOWN_FREE && offsetof(revo_map_known_info, reserved) == 56,
              "the known field's info record is the same line, two words longer");
static_assert(sizeof(revo_map_df_sample_t) == 16 && offsetof(revo_map_df_sample_t, grad) == 4, "a sample is one 16-byte word");
static_assert(REVO_DF_NONE == 0xffffffffu, "REVO_DF_NONE is all ones");

// One thread per slot of the table, as k_map_extract reads it: an occupied slot with count >= min_count is a solid voxel.
// Inside the box it sets its bit of the z-major bit volume (wz 32-bit words per z-line, bit = iz relative to the box);
// the three counters go through LDS, then one global atomic per block and counter.  Block 0 also states the cell count.
__global__ void __launch_bounds__(256) k_df_occupancy(const u64* __restrict__ keys, const MapVal* __restrict__ vals, unsigned cap, u64 min_count,
                                                      const revo_map_df_box box, unsigned wz, unsigned* bits, u64* info) {
  __shared__ unsigned s_cnt[3];  // solid, outside, below
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  const u64 key = i < cap ? keys[i] : MAP_EMPTY;
  int which = -1;
  if (key != MAP_EMPTY) {
    const u64 n = vals[i].n;
    if (n >= min_count) {
      int kx, ky, kz;
      map_key_axes(key, kx, ky, kz);
      const unsigned dx = (unsigned)(kx - box.lo[0]), dy = (unsigned)(ky - box.lo[1]), dz = (unsigned)(kz - box.lo[2]);
      if (dx < (unsigned)box.n[0] && dy < (unsigned)box.n[1] && dz < (unsigned)box.n[2]) {
        which = 0;
        atomicOr(&bits[((size_t)dx * box.n[1] + dy) * wz + (dz >> 5)], 1u << (dz & 31));
      } else {
        which = 1;
      }
    } else if (n) {  // a slot whose count is 0 holds no voxel (revo_map_export_raw gives none for it)
      which = 2;
    }
  }
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const u64 b = __ballot(which == k);
    if (lane == 0 && b) atomicAdd(&s_cnt[k], (unsigned)__popcll(b));
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&info[DF_SOLID + threadIdx.x], (u64)s_cnt[threadIdx.x]);
  if (blockIdx.x == 0 && threadIdx.x == 3) info[DF_CELLS] = (u64)box.n[0] * box.n[1] * box.n[2];
}

// revo_map_known_field: between k_df_occupancy and k_df_pass_z, the unknown cells join the bit volume.  One lane per 32-cell
// word: its solid bits, the (up to) 32 bytes of `seen` behind them, and the bits of the cells that are neither solid nor known
// ORed in (every word has one owner: a plain store).  unknown and known_free are counted by the wave, then one global atomic
// per block and counter, on the line k_df_occupancy and the passes write.
__global__ void __launch_bounds__(256) k_df_unknown(const uint8_t* __restrict__ seen, const revo_map_df_box box, unsigned wz, unsigned min_views,
                                                    unsigned* bits, u64* info) {
  __shared__ unsigned s_cnt[2];  // unknown, known_free
  if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const unsigned words = (unsigned)box.n[0] * (unsigned)box.n[1] * wz;
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  unsigned n_unknown = 0, n_free = 0;
  if (i < words) {
    const unsigned line = i / wz, w = i - line * wz;
    const unsigned nz = (unsigned)box.n[2], z0 = w * 32, len = min(32u, nz - z0);
    const uint8_t* row = seen + (size_t)line * nz + z0;
    const unsigned solid = bits[i];
    unsigned unknown = 0;
    for (unsigned k = 0; k < len; ++k)
      unknown |= (seen_is_unknown((solid >> k) & 1u, row[k], min_views) ? 1u : 0u) << k;
    if (unknown) bits[i] = solid | unknown;
    n_unknown = (unsigned)__popc(unknown);
    n_free = len - (unsigned)__popc(solid) - n_unknown;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) { n_unknown += __shfl_down(n_unknown, off, 64); n_free += __shfl_down(n_free, off, 64); }
  if ((threadIdx.x & 63) == 0) {
    if (n_unknown) atomicAdd(&s_cnt[0], n_unknown);
    if (n_free) atomicAdd(&s_cnt[1], n_free);
  }
  __syncthreads();
  if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&info[DF_UNKNOWN + threadIdx.x], (u64)s_cnt[threadIdx.x]);
}

// The same scan for revo_map_bounds: b[0..2] the smallest, b[3..5] the largest index per axis, cnt the solid voxels.  A wave
// folds its voxels first, so there is one global atomic per wave and word.
__global__ void __launch_bounds__(256) k_map_bounds(const u64* __restrict__ keys, const MapVal* __restrict__ vals, unsigned cap, u64 min_count,
                                                    int* b, u64* cnt) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  const u64 key = i < cap ? keys[i] : MAP_EMPTY;
  const bool solid = key != MAP_EMPTY && vals[i].n >= min_count;
  int lo0 = INT_MAX, lo1 = INT_MAX, lo2 = INT_MAX, hi0 = INT_MIN, hi1 = INT_MIN, hi2 = INT_MIN;
  if (solid) {
    map_key_axes(key, lo0, lo1, lo2);
    hi0 = lo0; hi1 = lo1; hi2 = lo2;
  }
  const u64 any = __ballot(solid);
  if (!any) return;
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    lo0 = min(lo0, __shfl_down(lo0, off, 64)); lo1 = min(lo1, __shfl_down(lo1, off, 64)); lo2 = min(lo2, __shfl_down(lo2, off, 64));
    hi0 = max(hi0, __shfl_down(hi0, off, 64)); hi1 = max(hi1, __shfl_down(hi1, off, 64)); hi2 = max(hi2, __shfl_down(hi2, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&b[0], lo0); atomicMin(&b[1], lo1); atomicMin(&b[2], lo2);
    atomicMax(&b[3], hi0); atomicMax(&b[4], hi1); atomicMax(&b[5], hi2);
    atomicAdd(cnt, (u64)__popcll(any));
  }
}

// Pass z.  A wave per z-line (nz <= 1024 cells: at most 32 words, lane w holds word w); a ballot says which words hold a bit,
// so a cell finds the nearest set bit on either side with two word fetches across the wave and clz / ffs, and a line without
// a bit is written as DF_INF at once.
__global__ void __launch_bounds__(256) k_df_pass_z(const unsigned* __restrict__ bits, unsigned lines, int nz, unsigned wz, unsigned* d2) {
  const int lane = threadIdx.x & 63;
  const unsigned wave = blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  for (unsigned line = wave; line < lines; line += nwaves) {  // wave-uniform
    const unsigned word = (unsigned)lane < wz ? bits[(size_t)line * wz + lane] : 0u;
    const unsigned nonzero = (unsigned)__ballot(word != 0);  // wz <= 32: the low half
    unsigned* out = d2 + (size_t)line * nz;
    for (int z0 = 0; z0 < nz; z0 += 64) {
      const int iz = z0 + lane;
      const int w = min(iz, nz - 1) >> 5, b = iz & 31;
      unsigned best = DF_INF;
      if (nonzero) {
        // below or at iz: the highest bit <= b of this word, else the highest bit of the nearest word below that has one
        const unsigned own = __shfl(word, w, 64);
        const unsigned at_or_below = own & (0xffffffffu >> (31 - b));
        const unsigned words_below = nonzero & ((1u << w) - 1u);
        const int wb = words_below ? 31 - __clz(words_below) : 0;
        const unsigned other_b = __shfl(word, wb, 64);
        int below = -1;
        if (at_or_below) below = w * 32 + 31 - __clz(at_or_below);
        else if (words_below) below = wb * 32 + 31 - __clz(other_b);
        // above iz: the lowest bit > b of this word, else the lowest bit of the nearest word above that has one
        const unsigned above_here = b == 31 ? 0u : own & (0xffffffffu << (b + 1));
        const unsigned words_above = w == 31 ? 0u : nonzero & (0xffffffffu << (w + 1));
        const int wa = words_above ? __ffs(words_above) - 1 : 0;
        const unsigned other_a = __shfl(word, wa, 64);
        int above = -1;
        if (above_here) above = w * 32 + __ffs(above_here) - 1;
        else if (words_above) above = wa * 32 + __ffs(other_a) - 1;
        if (below >= 0) { const unsigned d = (unsigned)(iz - below); best = d * d; }
        if (above >= 0) { const unsigned d = (unsigned)(above - iz); best = min(best, d * d); }
      }
      if (iz < nz) out[iz] = best;
    }
  }
}

// Passes y and x: d(i) = min_j (i - j)^2 + g(j) along lines of L cells whose neighbours in memory are `inner` consecutive
// words ([outer][L][inner]; y: nx x ny x nz, x: 1 x nx x ny nz).  A block stages L x S words in LDS (S = 1 << sh consecutive
// lines, L * S <= DF_TILE_WORDS) and overwrites them in global memory: the tile is its own.  A thread owns cells of one line
// and searches outwards from each, four offsets a round, ending once k^2 >= best; a line without a finite entry (the line's minimum, taken while
// staging) is written back as it is, so empty space costs one read and one write per cell.  LAST: the pass also writes the
// contract's values -- DF_INF becomes REVO_DF_NONE, the clamp applies -- and folds the largest one into info[DF_MAXD2].
template <bool LAST>
__global__ void __launch_bounds__(256) k_df_pass(unsigned* d2, int L, unsigned inner, int sh, unsigned strips, unsigned clamp, u64* info) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_g[];  // [L][S]
  __shared__ unsigned s_min[64];
  __shared__ unsigned s_max;
  const int S = 1 << sh, R = 256 >> sh;  // lines of the tile, rows a sweep of the block covers
  const unsigned strip = blockIdx.x % strips, o = blockIdx.x / strips;
  const int c = threadIdx.x & (S - 1), r = threadIdx.x >> sh;
  const unsigned col = strip * S + c;
  const bool live = col < inner;
  unsigned* base = d2 + (size_t)o * L * inner + col;
  if (threadIdx.x < 64) s_min[threadIdx.x] = DF_INF;
  if (threadIdx.x == 0) s_max = 0;
  __syncthreads();
  unsigned mine = DF_INF;
  for (int i = r; i < L; i += R) {
    const unsigned g = live ? base[(size_t)i * inner] : DF_INF;
    s_g[(i << sh) + c] = g;
    mine = min(mine, g);
  }
  if (mine < DF_INF) atomicMin(&s_min[c], mine);
  __syncthreads();
  const bool any = s_min[c] < DF_INF;
  unsigned top = 0;
  if (live) {
    for (int i = r; i < L; i += R) {
      unsigned best = s_g[(i << sh) + c];
      if (any) {
        const int reach = max(i, L - 1 - i);
        for (int k0 = 1; k0 <= reach && (unsigned)(k0 * k0) < best; k0 += 4) {
          unsigned cand[4];  // four offsets per round: eight independent LDS reads in flight, one test of the bound
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k = k0 + u;
            const unsigned a = i - k >= 0 ? s_g[((i - k) << sh) + c] : DF_INF;
            const unsigned b = i + k < L ? s_g[((i + k) << sh) + c] : DF_INF;
            cand[u] = (unsigned)(k * k) + min(a, b);  // DF_INF + 1026^2 < 2^31: no wrap, and never below a finite best
          }
          best = min(min(best, min(cand[0], cand[1])), min(cand[2], cand[3]));
        }
      }
      if (LAST) {
        if (best >= DF_INF) best = REVO_DF_NONE;
        else { if (clamp) best = min(best, clamp); top = max(top, best); }
      }
      base[(size_t)i * inner] = best;
    }
  }
  if (LAST) {
#pragma unroll
    for (int off = 32; off; off >>= 1) top = max(top, __shfl_down(top, off, 64));
    if ((threadIdx.x & 63) == 0 && top) atomicMax(&s_max, top);
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(&info[DF_MAXD2], (u64)s_max);
  }
}

// One thread per point: the cell's value and its two neighbours per axis (seven loads), float32 with every operation rounded
// on its own.
struct DfSampleK { revo_map_df_box box; float voxel; unsigned n; };
__global__ void __launch_bounds__(256) k_df_sample(const DfSampleK a, const unsigned* __restrict__ d2, const float* __restrict__ xyz, float4* out) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
  int c[3];
  bool inside = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float f = floorf(__fdiv_rn(p[k], a.voxel));
    inside = inside && isfinite(p[k]) && isfinite(f) && f >= (float)a.box.lo[k] && f <= (float)(a.box.lo[k] + a.box.n[k] - 1);
    c[k] = inside ? (int)f - a.box.lo[k] : 0;
  }
  float4 res = make_float4(-1.0f, 0.0f, 0.0f, 0.0f);
  if (inside) {
    const size_t sy = (size_t)a.box.n[2], sx = sy * a.box.n[1];
    const size_t at = c[0] * sx + c[1] * sy + c[2];
    const unsigned v = d2[at];
    if (v == REVO_DF_NONE) {
      res.x = INFINITY;
    } else {
      res.x = sqrtf((float)v) * a.voxel;
      float g[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const size_t st = k == 0 ? sx : (k == 1 ? sy : 1);
        const int lo = max(c[k] - 1, 0), hi = min(c[k] + 1, a.box.n[k] - 1);
        const int span = hi - lo;
        const size_t line = at - c[k] * st;
        g[k] = span == 0 ? 0.0f : __fdiv_rn(sqrtf((float)d2[line + hi * st]) - sqrtf((float)d2[line + lo * st]), (float)span);
      }
      res.y = g[0]; res.z = g[1]; res.w = g[2];
    }
  }
  out[i] = res;
}

// -------------------------------------------------------------------------------------------------------- entry points --
// the box rules of DESIGN 21; nullptr if the box keeps them
const char* map_df_box_check(const revo_map_df_box* box, size_t* cells) {
  size_t n = 1;
  for (int k = 0; k < 3; ++k) {
    if (box->n[k] < 1 || box->n[k] > DF_MAX_N) return "a box size must be 1 .. 1024 cells";
    if (box->lo[k] < -(1 << 20) || (long long)box->lo[k] + box->n[k] - 1 > (1 << 20) - 1) return "the box leaves the voxel index range [-2^20, 2^20 - 1]";
    n *= (size_t)box->n[k];
  }
  if (n > DF_MAX_CELLS) return "the box holds more than 2^27 cells";
  *cells = n;
  return nullptr;
}

// one min-plus pass over [outer][L][inner], in place
template <bool LAST>
static void df_launch_pass(hipStream_t s, unsigned* d2, unsigned outer, int L, unsigned inner, unsigned clamp, u64* info) {
  int sh = 6;  // the widest strip (64 lines, 256 B per row) whose tile fits
  while (sh > 3 && ((size_t)L << sh) > DF_TILE_WORDS) --sh;
  const unsigned strips = (inner + (1u << sh) - 1) >> sh;
  hipLaunchKernelGGL(k_df_pass<LAST>, dim3(outer * strips), dim3(256), sizeof(unsigned) * ((size_t)L << sh), s, d2, L, inner, sh, strips, clamp, info);
}

// The bit volume of the box's solid voxels on stream s, in m->dfbits, with k_df_occupancy's counters in `info` (NULL: the map's
// own line, m->dfcnt).  For the units that ask "is this cell solid" (revo_map_frontiers).
int map_df_solid_bits(revo_map* m, const revo_map_df_box* box, uint32_t min_count, hipStream_t s, const unsigned** bits, unsigned* wz, u64* info) {
  const unsigned w = (unsigned)(box->n[2] + 31) / 32;
  const size_t bit_bytes = sizeof(unsigned) * (size_t)box->n[0] * (size_t)box->n[1] * w;
  TRY(m->dfbits.reserve(bit_bytes, s));
  TRY(m->dfcnt.reserve(128, s));
  if (!info) info = (u64*)m->dfcnt.p;
  HIPCHECK(hipMemsetAsync(m->dfbits.p, 0, bit_bytes, s));
  HIPCHECK(hipMemsetAsync(info, 0, sizeof(revo_map_df_info), s));
  hipLaunchKernelGGL(k_df_occupancy, dim3((unsigned)std::max<size_t>((m->cap + 255) / 256, 1)), dim3(256), 0, s, m->d_keys, m->d_vals,
                     (unsigned)m->cap, (u64)std::max<uint32_t>(min_count, 1), *box, w, (unsigned*)m->dfbits.p, info);
  HIPCHECK(hipGetLastError());
  *bits = (const unsigned*)m->dfbits.p;
  *wz = w;
  return REVO_OK;
}

// The field of the box over the solid voxels and, with d_seen (the box's seen volume in device memory), the unknown cells
// too: the body of revo_map_distance_field and revo_map_known_field behind their argument checks.  timer: the handle's df_time
// for revo_map_distance_field, which owns it (revo_map_distance_field_last_ms describes its last call); NULL for the known field.
static int df_run(revo_map* m, const revo_map_df_box* box, size_t cells, uint32_t min_count, uint32_t clamp, const uint8_t* d_seen,
                  uint32_t min_views, uint32_t* d2, int device_out, void* info, bool wait, EventTimer* timer) {
  hipStream_t s = (hipStream_t)m->g.stream;
  const revo_map_df_box b = *box;
  const unsigned lines = (unsigned)b.n[0] * (unsigned)b.n[1];
  TRY(m->dfbits.reserve(sizeof(unsigned) * (size_t)lines * ((unsigned)(b.n[2] + 31) / 32), s));  // every allocation before the timed span
  TRY(m->dfcnt.reserve(128, s));
  TRY(m->dfout.reserve(device_out ? 0 : sizeof(unsigned) * cells, s));
  unsigned* d_out = device_out ? d2 : (unsigned*)m->dfout.p;
  u64* d_info = device_out && info ? (u64*)info : (u64*)m->dfcnt.p;
  if (timer) TRY(timer->begin(s));
  const unsigned* bits = nullptr;
  unsigned wz = 0;
  TRY(map_df_solid_bits(m, box, min_count, s, &bits, &wz, d_info));
  if (d_seen) {
    hipLaunchKernelGGL(k_df_unknown, dim3((lines * wz + 255) / 256), dim3(256), 0, s, d_seen, b, wz, min_views, (unsigned*)m->dfbits.p, d_info);
    HIPCHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_df_pass_z, dim3(std::min(lines / 4 + 1, 8192u)), dim3(256), 0, s, bits, lines, b.n[2], wz, d_out);
  HIPCHECK(hipGetLastError());
  df_launch_pass<false>(s, d_out, (unsigned)b.n[0], b.n[1], (unsigned)b.n[2], 0, d_info);
  HIPCHECK(hipGetLastError());
  df_launch_pass<true>(s, d_out, 1, b.n[0], (unsigned)b.n[1] * (unsigned)b.n[2], clamp, d_info);
  HIPCHECK(hipGetLastError());
  if (timer) TRY(timer->end(s));
  if (!device_out) {
    HIPCHECK(hipMemcpyAsync(d2, d_out, sizeof(unsigned) * cells, hipMemcpyDeviceToHost, s));
    if (info) HIPCHECK(hipMemcpyAsync(info, d_info, sizeof(revo_map_df_info), hipMemcpyDeviceToHost, s));
  }
  if (wait) HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_distance_field(revo_map* m, const revo_map_df_box* box, uint32_t min_count, uint32_t clamp, uint32_t* d2, int device_out,
                                       revo_map_df_info* info) {
  if (!m || !box || !d2) return fail(REVO_ERR_INVALID_ARG, "null argument");
  size_t cells = 0;
  if (const char* why = map_df_box_check(box, &cells)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_distance_field: ") + why);
  TRY(map_check_side(device_out, "device_out"));
  if (device_out) TRY(map_check_aligned((uintptr_t)d2 | (uintptr_t)info, 16, "a device output is"));
  HIPCHECK(hipSetDevice(m->g.device));
  return df_run(m, box, cells, min_count, clamp, nullptr, 0, d2, device_out, info, !device_out, &m->df_time);
}

extern "C" int revo_map_known_field(revo_map* m, const revo_map_df_box* box, uint32_t min_count, uint32_t clamp, const uint8_t* seen,
                                    int device_seen, uint32_t min_views, uint32_t* d2, int device_out, revo_map_known_info* info) {
  if (!m || !box || !d2 || !seen) return fail(REVO_ERR_INVALID_ARG, "null argument");
  size_t cells = 0;
  if (const char* why = map_df_box_check(box, &cells)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_known_field: ") + why);
  TRY(map_check_side(device_seen, "device_seen"));
  TRY(map_check_side(device_out, "device_out"));
  if (device_seen) TRY(map_check_aligned((uintptr_t)seen, 16, "the device seen volume is"));
  if (device_out) TRY(map_check_aligned((uintptr_t)d2 | (uintptr_t)info, 16, "a device output is"));
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  const uint8_t* d_seen = seen;
  if (!device_seen) {
    TRY(m->seenvol.reserve(cells, s));
    HIPCHECK(hipMemcpyAsync(m->seenvol.p, seen, cells, hipMemcpyHostToDevice, s));
    d_seen = (const uint8_t*)m->seenvol.p;
  }
  return df_run(m, box, cells, min_count, clamp, d_seen, min_views, d2, device_out, info, !device_out || !device_seen, nullptr);
}

extern "C" int revo_map_distance_field_last_ms(revo_map* m, float* ms) {
  if (!m || !ms) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!m->df_time.ready) return fail(REVO_ERR_INVALID_ARG, "the map has built no distance field yet");
  HIPCHECK(hipSetDevice(m->g.device));
  return m->df_time.last_ms(ms);
}

extern "C" int revo_map_bounds(revo_map* m, uint32_t min_count, int32_t lo[3], int32_t hi[3], size_t* n) {
  if (!m || !lo || !hi || !n) return fail(REVO_ERR_INVALID_ARG, "null argument");
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  TRY(m->dfcnt.reserve(128, s));
  struct Line { int b[6]; int pad[2]; u64 cnt; } h = {{INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN}, {0, 0}, 0};
  Line* d = (Line*)(m->dfcnt.p + 64);  // behind the field's info line
  HIPCHECK(hipMemcpyAsync(d, &h, sizeof(h), hipMemcpyHostToDevice, s));
  if (m->cap) {
    hipLaunchKernelGGL(k_map_bounds, dim3((unsigned)((m->cap + 255) / 256)), dim3(256), 0, s, m->d_keys, m->d_vals, (unsigned)m->cap,
                       (u64)std::max<uint32_t>(min_count, 1), d->b, &d->cnt);
    HIPCHECK(hipGetLastError());
  }
  HIPCHECK(hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  for (int k = 0; k < 3; ++k) { lo[k] = h.cnt ? h.b[k] : 0; hi[k] = h.cnt ? h.b[3 + k] : 0; }
  *n = (size_t)h.cnt;
  return REVO_OK;
}

extern "C" int revo_map_df_sample(revo_map* m, const revo_map_df_box* box, const uint32_t* d2, int device_field, size_t n, const float* xyz,
                                  int device_in, revo_map_df_sample_t* out, int device_out) {
  if (!m || !box || !d2 || !xyz || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n < 1 || n > DF_MAX_POINTS) return fail(REVO_ERR_INVALID_ARG, "revo_map_df_sample: n must be 1 .. 2^24 points");
  size_t cells = 0;
  if (const char* why = map_df_box_check(box, &cells)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_df_sample: ") + why);
  TRY(map_check_side(device_field, "device_field"));
  TRY(map_check_side(device_in, "device_in"));
  TRY(map_check_side(device_out, "device_out"));
  if (device_field) TRY(map_check_aligned((uintptr_t)d2, 16, "the device field is"));
  if (device_in) TRY(map_check_aligned((uintptr_t)xyz, 16, "the device points are"));
  if (device_out) TRY(map_check_aligned((uintptr_t)out, 16, "the device output is"));
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  DevScratch field, pts, res;  // freed after the wait below
  const unsigned* d_field = d2;
  const float* d_xyz = xyz;
  float4* d_res = (float4*)out;
  if (!device_field) {
    TRY(field.alloc(sizeof(unsigned) * cells));
    HIPCHECK(hipMemcpyAsync(field.p, d2, sizeof(unsigned) * cells, hipMemcpyHostToDevice, s));
    d_field = (const unsigned*)field.p;
  }
  if (!device_in) {
    TRY(pts.alloc(sizeof(float) * 3 * n));
    HIPCHECK(hipMemcpyAsync(pts.p, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, s));
    d_xyz = (const float*)pts.p;
  }
  if (!device_out) {
    TRY(res.alloc(sizeof(float4) * n));
    d_res = (float4*)res.p;
  }
  const bool waits = !device_field || !device_in || !device_out;
  const DfSampleK a{*box, m->voxel, (unsigned)n};
  hipLaunchKernelGGL(k_df_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, d_field, d_xyz, d_res);
  if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(s); return fail(REVO_ERR_HIP, "k_df_sample: the launch failed"); }
  if (!device_out) {
    const hipError_t e = hipMemcpyAsync(out, d_res, sizeof(float4) * n, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); return fail(REVO_ERR_HIP, std::string("revo_map_df_sample: ") + hipGetErrorString(e)); }
  }
  if (waits) HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}
