// revo_map_plan.hip -- planning through the map: the clearance-aware cost-to-go from a set of seed cells to every
// cell of a distance field's box under the 26 moves of the 3-4-5 chamfer (revo_map_plan), and the paths that descend it
// (revo_map_plan_paths).  A shortest-path cost over integer weights has one value per cell, so the bytes do not depend on the
// order in which the relaxation reaches it.
//
// The cost is relaxed in the caller's buffer, in place, as tile-wise Bellman-Ford over 8 x 8 x 8 tiles: a round is one launch
// of one workgroup per tile; a tile whose flag for the round is clear exits at once, an active one stages its cells and their
// halo in LDS, relaxes them there until nothing changes, writes the lowered cells back and marks, for the NEXT round, every
// neighbouring tile whose halo holds one of them.  Values only ever decrease, so a halo read that races with a neighbour's
// write-back of the same round is at worst a larger upper bound, and the mark plus the next launch's boundary repairs it.
// The host looks at the number of marked tiles after every few rounds and stops at zero (revo_plan_host.h).
#include "revo_map_impl.h"
#include "revo_plan_host.h"

// The LDS tile: cell (hx, hy, hz) of the 10 x 10 x 10 halo block at hx * PLAN_SX + hy * PLAN_SY + hz.  A thread's cell is
// z = t & 7, x = (t >> 3) & 7, y = t >> 6, so the 32 lanes that share an LDS cycle (ds_read_b32 and ds_write_b32 bank by
// (address / 4) % 32 within each half of the wave) hold 8 z by 4 x at one y: x stride 104 = 8 mod 32 puts their four runs of
// eight words on banks 0-7, 8-15, 16-23, 24-31, whatever the neighbour offset -- no conflict.  (The plain stride 100 = 4 mod
// 32 starts them four banks apart, so neighbouring runs overlap: two-way conflicts on every read.)
#define PLAN_SY 10
#define PLAN_SX 104
#define PLAN_LDS_WORDS (10 * PLAN_SX)
#define PLAN_SWEEPS 1024

// the head line of the work buffer, in 32-bit words: the info record (8 x u64), the marked-tile counts of the two round
// parities, the last round in which a tile ran
enum { PLAN_W_CNT = 16, PLAN_W_LAST = 18, PLAN_HEAD_WORDS = 32 };
// info words (revo_map_plan_info)
enum { PLAN_I_CELLS = 0, PLAN_I_FREE = 1, PLAN_I_REACH = 2, PLAN_I_MAX = 3, PLAN_I_USED = 4, PLAN_I_OUTSIDE = 5, PLAN_I_BLOCKED = 6 };

static_assert(sizeof(revo_map_plan_seed) == 16 && offsetof(revo_map_plan_seed, cost0) == 12, "a seed is one 16-byte word");
static_assert(sizeof(revo_map_plan_info) == 64 && offsetof(revo_map_plan_info, free) == 8 * PLAN_I_FREE &&
              offsetof(revo_map_plan_info, reachable) == 8 * PLAN_I_REACH && offsetof(revo_map_plan_info, max_cost) == 8 * PLAN_I_MAX &&
              offsetof(revo_map_plan_info, seeds_used) == 8 * PLAN_I_USED && offsetof(revo_map_plan_info, seeds_outside) == 8 * PLAN_I_OUTSIDE &&
              offsetof(revo_map_plan_info, seeds_blocked) == 8 * PLAN_I_BLOCKED && offsetof(revo_map_plan_info, reserved) == 56,
              "the info record is the kernels' counter line");
static_assert(sizeof(revo_map_plan_path) == 16 && offsetof(revo_map_plan_path, cost) == 8, "a path record is one 16-byte word");
static_assert(REVO_PLAN_NONE == 0xffffffffu && PLAN_SEED_USED == 0 && PLAN_SEED_BLOCKED == 2, "the codes the kernels count by");

struct PlanK {
  revo_map_df_box box;
  PlanTiles tiles;
  unsigned* flags;  // [2][tiles]: tile active in a round of even / odd number
  unsigned* head;   // PLAN_HEAD_WORDS words
};

__device__ __forceinline__ unsigned plan_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void plan_store(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// marks `tile` in the flag array `f`; the first to do so counts it
__device__ __forceinline__ void plan_mark(unsigned* f, unsigned tile, unsigned* count) {
  if (atomicExch(&f[tile], 1u) == 0u) atomicAdd(count, 1u);
}

// One thread per cell: the internal codes the relaxation reads -- PLAN_INF for a free cell, PLAN_BLOCKED for the others -- and
// the free count (ballot, LDS, one global atomic per block).
__global__ void __launch_bounds__(256) k_plan_init(const unsigned* __restrict__ d2, unsigned r2, unsigned cells, unsigned* __restrict__ cost, u64* info) {
  __shared__ unsigned s_free;
  if (threadIdx.x == 0) s_free = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  bool is_free = false;
  if (i < cells) {
    is_free = d2[i] >= r2;
    cost[i] = is_free ? PLAN_INF : PLAN_BLOCKED;
  }
  const u64 b = __ballot(is_free);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&s_free, (unsigned)__popcll(b));
  __syncthreads();
  if (threadIdx.x == 0 && s_free) atomicAdd(&info[PLAN_I_FREE], (u64)s_free);
  if (blockIdx.x == 0 && threadIdx.x == 1) info[PLAN_I_CELLS] = (u64)cells;
}

// One thread per seed: atomicMin into its cell when it is used, its tile marked for round 0, the three seed counts.
__global__ void __launch_bounds__(256) k_plan_seed(const PlanK a, unsigned* cost, const revo_map_plan_seed* __restrict__ seeds, unsigned n) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  int cls = -1;
  if (i < n) {
    const revo_map_plan_seed s = seeds[i];
    unsigned at = 0;
    cls = plan_seed_class(a.box, s, [&](unsigned c) { return plan_load(&cost[c]); }, &at);
    if (cls == PLAN_SEED_USED) {
      atomicMin(&cost[at], s.cost0);
      const unsigned tile = plan_tile_of_cell(a.tiles, (unsigned)(s.cell[0] - a.box.lo[0]), (unsigned)(s.cell[1] - a.box.lo[1]), (unsigned)(s.cell[2] - a.box.lo[2]));
      plan_mark(a.flags, tile, &a.head[PLAN_W_CNT]);
    }
  }
  u64* info = (u64*)a.head;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const u64 b = __ballot(cls == k);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&info[PLAN_I_USED + k], (u64)__popcll(b));
  }
}

// One round: a workgroup of 512 threads per tile, a thread per cell.
__global__ void __launch_bounds__(512) k_plan_relax(const PlanK a, unsigned* cost, unsigned round) {
  __shared__ unsigned s_c[PLAN_LDS_WORDS];
  __shared__ unsigned s_mask;
  const unsigned tile = blockIdx.x, ntiles = a.tiles.count;
  unsigned* cur_flags = a.flags + (round & 1u) * ntiles;
  unsigned* next_flags = a.flags + ((round + 1u) & 1u) * ntiles;
  unsigned* next_count = &a.head[PLAN_W_CNT + ((round + 1u) & 1u)];
  // this round's own count has been read (by the host, or by nobody); the round after next adds to the same word
  if (tile == 0 && threadIdx.x == 0) a.head[PLAN_W_CNT + (round & 1u)] = 0;
  const unsigned active = cur_flags[tile];
  __syncthreads();  // every thread has read the flag before it is cleared
  if (!active) return;
  if (threadIdx.x == 0) { cur_flags[tile] = 0; s_mask = 0; }

  const int t2 = a.tiles.t[2], t1 = a.tiles.t[1];
  const int tz = (int)(tile % (unsigned)t2), ty = (int)(tile / (unsigned)t2 % (unsigned)t1), tx = (int)(tile / ((unsigned)t2 * (unsigned)t1));
  const int n0 = a.box.n[0], n1 = a.box.n[1], n2 = a.box.n[2];
  for (int i = threadIdx.x; i < 1000; i += 512) {
    const int hx = i / 100, r = i - hx * 100, hy = r / 10, hz = r - hy * 10;
    const int gx = tx * PLAN_TILE - 1 + hx, gy = ty * PLAN_TILE - 1 + hy, gz = tz * PLAN_TILE - 1 + hz;
    const bool in = (unsigned)gx < (unsigned)n0 && (unsigned)gy < (unsigned)n1 && (unsigned)gz < (unsigned)n2;
    s_c[hx * PLAN_SX + hy * PLAN_SY + hz] = in ? plan_load(&cost[((unsigned)gx * (unsigned)n1 + (unsigned)gy) * (unsigned)n2 + (unsigned)gz]) : PLAN_BLOCKED;
  }
  __syncthreads();

  const int cz = threadIdx.x & 7, cx = (threadIdx.x >> 3) & 7, cy = threadIdx.x >> 6;
  const int idx = (cx + 1) * PLAN_SX + (cy + 1) * PLAN_SY + (cz + 1);
  const unsigned orig = s_c[idx];
  unsigned cur = orig;
  const bool is_free = orig < PLAN_BLOCKED;  // a cell outside the box is PLAN_BLOCKED too: such a thread never writes
  bool again = false;
  for (int sweep = 0;;) {
    unsigned best = cur;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
          if (dx | dy | dz) best = min(best, s_c[idx + dx * PLAN_SX + dy * PLAN_SY + dz] + plan_weight(dx, dy, dz));  // PLAN_BLOCKED + 5: no wrap
    const bool lower = is_free && best < cur;
    if (!__syncthreads_or(lower)) break;  // and every read of the sweep is done
    if (lower) { s_c[idx] = best; cur = best; }
    if (++sweep == PLAN_SWEEPS) { again = true; break; }  // uniform
    __syncthreads();
  }
  if (cur < orig) {
    const int gx = tx * PLAN_TILE + cx, gy = ty * PLAN_TILE + cy, gz = tz * PLAN_TILE + cz;
    plan_store(&cost[((unsigned)gx * (unsigned)n1 + (unsigned)gy) * (unsigned)n2 + (unsigned)gz], cur);
    const unsigned mask = plan_halo_mask(cx, cy, cz);
    if (mask) atomicOr(&s_mask, mask);
  }
  __syncthreads();
  if (threadIdx.x < 27) {
    const int dx = (int)threadIdx.x / 9 - 1, dy = (int)threadIdx.x / 3 % 3 - 1, dz = (int)threadIdx.x % 3 - 1;
    const int ux = tx + dx, uy = ty + dy, uz = tz + dz;
    const bool self = threadIdx.x == 13;
    const bool want = self ? again : ((s_mask >> threadIdx.x) & 1u) != 0;
    if (want && (unsigned)ux < (unsigned)a.tiles.t[0] && (unsigned)uy < (unsigned)t1 && (unsigned)uz < (unsigned)t2)
      plan_mark(next_flags, ((unsigned)ux * (unsigned)t1 + (unsigned)uy) * (unsigned)t2 + (unsigned)uz, next_count);
  }
  if (threadIdx.x == 32) atomicMax(&a.head[PLAN_W_LAST], round + 1u);
}

// One thread per cell: the contract's values -- every internal code at or above PLAN_INF becomes REVO_PLAN_NONE -- and the
// reachable count and largest cost: wave shuffle, LDS, one global atomic per block and word.
__global__ void __launch_bounds__(256) k_plan_finish(unsigned* __restrict__ cost, unsigned cells, u64* info) {
  __shared__ unsigned s_n, s_max;
  if (threadIdx.x == 0) { s_n = 0; s_max = 0; }
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  bool reached = false;
  unsigned top = 0;
  if (i < cells) {
    const unsigned v = cost[i];
    reached = v < PLAN_INF;
    if (reached) top = v; else cost[i] = REVO_PLAN_NONE;
  }
  const u64 b = __ballot(reached);
#pragma unroll
  for (int off = 32; off; off >>= 1) top = max(top, __shfl_down(top, off, 64));
  if ((threadIdx.x & 63) == 0 && b) { atomicAdd(&s_n, (unsigned)__popcll(b)); atomicMax(&s_max, top); }
  __syncthreads();
  if (threadIdx.x == 0 && s_n) { atomicAdd(&info[PLAN_I_REACH], (u64)s_n); atomicMax(&info[PLAN_I_MAX], (u64)s_max); }
}

// One thread per start: a serial walk down the cost field, bounded by max_len.
struct PlanPathK { revo_map_df_box box; unsigned n, max_len; };
__global__ void __launch_bounds__(64) k_plan_paths(const PlanPathK a, const unsigned* __restrict__ cost, const int* __restrict__ starts, int* cells_out,
                                                   uint4* path_out) {
  const unsigned i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  const int n0 = a.box.n[0], n1 = a.box.n[1], n2 = a.box.n[2];
  int x = starts[3 * (size_t)i] - a.box.lo[0], y = starts[3 * (size_t)i + 1] - a.box.lo[1], z = starts[3 * (size_t)i + 2] - a.box.lo[2];
  unsigned len = 0, status = REVO_PLAN_OUTSIDE, c0 = REVO_PLAN_NONE;
  if ((unsigned)x < (unsigned)n0 && (unsigned)y < (unsigned)n1 && (unsigned)z < (unsigned)n2) {
    unsigned c = cost[((unsigned)x * (unsigned)n1 + (unsigned)y) * (unsigned)n2 + (unsigned)z];
    c0 = c;
    status = REVO_PLAN_UNREACHABLE;
    if (c != REVO_PLAN_NONE) {
      int* out = cells_out + 3 * (size_t)i * a.max_len;
      for (;;) {
        out[3 * (size_t)len] = x + a.box.lo[0]; out[3 * (size_t)len + 1] = y + a.box.lo[1]; out[3 * (size_t)len + 2] = z + a.box.lo[2];
        ++len;
        bool found = false;
        int fx = 0, fy = 0, fz = 0;
        unsigned fc = 0;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz)
              if (dx | dy | dz) {
                const int ux = x + dx, uy = y + dy, uz = z + dz;
                if (!found && (unsigned)ux < (unsigned)n0 && (unsigned)uy < (unsigned)n1 && (unsigned)uz < (unsigned)n2) {
                  const unsigned v = cost[((unsigned)ux * (unsigned)n1 + (unsigned)uy) * (unsigned)n2 + (unsigned)uz];
                  if (v != REVO_PLAN_NONE && v + plan_weight(dx, dy, dz) == c) { found = true; fx = ux; fy = uy; fz = uz; fc = v; }
                }
              }
        if (!found) { status = REVO_PLAN_REACHED; break; }
        if (len == a.max_len) { status = REVO_PLAN_TRUNCATED; break; }
        x = fx; y = fy; z = fz; c = fc;  // c falls by at least 3 a step: the walk ends
      }
    }
  }
  path_out[i] = make_uint4(len, status, c0, 0u);
}

// -------------------------------------------------------------------------------------------------------- entry points --
extern "C" int revo_map_plan(revo_map* m, const revo_map_df_box* box, const uint32_t* d2, int device_field, uint32_t r2, size_t n_seeds,
                             const revo_map_plan_seed* seeds, uint32_t max_rounds, uint32_t* cost, int device_out, revo_map_plan_info* info) {
  size_t cells = 0;
  uint32_t limit = 0;
  if (const char* why = plan_args_check(m, box, d2, device_field, r2, n_seeds, seeds, max_rounds, cost, device_out, info, &cells, &limit))
    return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_plan: ") + why);
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  const PlanTiles tiles = plan_tiles(*box);
  const size_t work_bytes = sizeof(unsigned) * (PLAN_HEAD_WORDS + 2 * (size_t)tiles.count);
  TRY(m->planwork.reserve(work_bytes, s));
  TRY(m->planseeds.reserve(sizeof(revo_map_plan_seed) * n_seeds, s));
  TRY(m->plancost.reserve(device_out ? 0 : sizeof(unsigned) * cells, s));
  if (!m->plan_pin.p) TRY(m->plan_pin.alloc(PLAN_HEAD_WORDS + 4));
  TRY(m->plan_ev.create());
  DevScratch field;  // freed after the wait below
  const unsigned* d_field = d2;
  if (!device_field) {
    TRY(field.alloc(sizeof(unsigned) * cells));
    HIPCHECK(hipMemcpyAsync(field.p, d2, sizeof(unsigned) * cells, hipMemcpyHostToDevice, s));
    d_field = (const unsigned*)field.p;
  }
  unsigned* head = (unsigned*)m->planwork.p;
  unsigned* d_cost = device_out ? cost : (unsigned*)m->plancost.p;
  const PlanK a{*box, tiles, head + PLAN_HEAD_WORDS, head};
  unsigned* pin = m->plan_pin.p;
  HIPCHECK(hipMemcpyAsync(m->planseeds.p, seeds, sizeof(revo_map_plan_seed) * n_seeds, hipMemcpyHostToDevice, s));
  TRY(m->plan_time.begin(s));
  HIPCHECK(hipMemsetAsync(head, 0, work_bytes, s));
  hipLaunchKernelGGL(k_plan_init, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, d_field, r2, (unsigned)cells, d_cost, (u64*)head);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_plan_seed, dim3((unsigned)((n_seeds + 255) / 256)), dim3(256), 0, s, a, d_cost, (const revo_map_plan_seed*)m->planseeds.p, (unsigned)n_seeds);
  HIPCHECK(hipGetLastError());
  unsigned round = 0;
  auto run = [&](uint32_t k, uint32_t* marked) -> int {
    for (uint32_t j = 0; j < k; ++j) hipLaunchKernelGGL(k_plan_relax, dim3(tiles.count), dim3(512), 0, s, a, d_cost, round++);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(pin + PLAN_HEAD_WORDS, head + PLAN_W_CNT + (round & 1u), sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIPCHECK(hipEventRecord(m->plan_ev, s));
    HIPCHECK(hipEventSynchronize(m->plan_ev));
    *marked = pin[PLAN_HEAD_WORDS];
    return REVO_OK;
  };
  uint32_t done = 0;
  const int rc = plan_round_loop(limit, PLAN_GROUP, run, &done);
  if (rc == REVO_ERR_CAPACITY) {
    TRY(m->plan_time.end(s));
    HIPCHECK(hipStreamSynchronize(s));
    m->plan_rounds = done;
    return fail(REVO_ERR_CAPACITY, "revo_map_plan: no fixed point within " + std::to_string(limit) + " rounds");
  }
  if (rc) { (void)hipStreamSynchronize(s); return rc; }
  hipLaunchKernelGGL(k_plan_finish, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, d_cost, (unsigned)cells, (u64*)head);
  HIPCHECK(hipGetLastError());
  TRY(m->plan_time.end(s));
  HIPCHECK(hipMemcpyAsync(pin, head, sizeof(unsigned) * PLAN_HEAD_WORDS, hipMemcpyDeviceToHost, s));
  if (!device_out) HIPCHECK(hipMemcpyAsync(cost, d_cost, sizeof(unsigned) * cells, hipMemcpyDeviceToHost, s));
  else if (info) HIPCHECK(hipMemcpyAsync(info, head, sizeof(revo_map_plan_info), hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (!device_out && info) memcpy(info, pin, sizeof(revo_map_plan_info));
  m->plan_rounds = pin[PLAN_W_LAST];
  return REVO_OK;
}

extern "C" int revo_map_plan_last(revo_map* m, float* ms, uint32_t* rounds) {
  if (!m || (!ms && !rounds)) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!m->plan_time.ready) return fail(REVO_ERR_INVALID_ARG, "the map has planned nothing yet");
  HIPCHECK(hipSetDevice(m->g.device));
  if (ms) TRY(m->plan_time.last_ms(ms));
  if (rounds) *rounds = m->plan_rounds;
  return REVO_OK;
}

extern "C" int revo_map_plan_paths(revo_map* m, const revo_map_df_box* box, const uint32_t* cost, int device_cost, size_t n_starts,
                                   const int32_t* starts, uint32_t max_len, int32_t* cells_out, revo_map_plan_path* path_out, int device_out) {
  size_t cells = 0;
  if (const char* why = plan_paths_args_check(m, box, cost, device_cost, n_starts, starts, max_len, cells_out, path_out, device_out, &cells))
    return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_plan_paths: ") + why);
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  DevScratch field, res;  // freed after the wait below
  const size_t out_bytes = sizeof(int32_t) * 3 * n_starts * (size_t)max_len, rec_bytes = sizeof(revo_map_plan_path) * n_starts;
  TRY(m->planseeds.reserve(sizeof(int32_t) * 3 * n_starts, s));
  const unsigned* d_cost = cost;
  int* d_cells = cells_out;
  uint4* d_rec = (uint4*)path_out;
  if (!device_cost) {
    TRY(field.alloc(sizeof(unsigned) * cells));
    HIPCHECK(hipMemcpyAsync(field.p, cost, sizeof(unsigned) * cells, hipMemcpyHostToDevice, s));
    d_cost = (const unsigned*)field.p;
  }
  if (!device_out) {
    TRY(res.alloc(rec_bytes + out_bytes));
    d_rec = (uint4*)res.p;
    d_cells = (int*)(res.p + rec_bytes);
    HIPCHECK(hipMemcpyAsync(d_cells, cells_out, out_bytes, hipMemcpyHostToDevice, s));  // what the walk does not write stays
  }
  HIPCHECK(hipMemcpyAsync(m->planseeds.p, starts, sizeof(int32_t) * 3 * n_starts, hipMemcpyHostToDevice, s));
  const PlanPathK a{*box, (unsigned)n_starts, max_len};
  hipLaunchKernelGGL(k_plan_paths, dim3((unsigned)((n_starts + 63) / 64)), dim3(64), 0, s, a, d_cost, (const int*)m->planseeds.p, d_cells, d_rec);
  if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(s); return fail(REVO_ERR_HIP, "k_plan_paths: the launch failed"); }
  if (!device_out) {
    hipError_t e = hipMemcpyAsync(cells_out, d_cells, out_bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(path_out, d_rec, rec_bytes, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); return fail(REVO_ERR_HIP, std::string("revo_map_plan_paths: ") + hipGetErrorString(e)); }
  }
  if (!device_cost || !device_out) HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}
