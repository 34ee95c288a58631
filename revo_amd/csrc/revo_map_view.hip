// revo_map_view.hip -- looking at the voxel map: revo_map_render (splatted z-buffer views), revo_map_raycast and
// revo_map_cast_rays (rays marched through the table).  Contracts: include/revo_hip.h; DESIGN 12 and 20.
#include "revo_map_impl.h"
#include "revo_carve_host.h"
#include "revo_ray_host.h"

// ---------------------------------------------------------------------------------------------------------------- views --
// revo_map_render (contract: include/revo_hip.h).  A z-buffer word is (bits of z) << 32 | R << 16 | G << 8 | B; an
// untouched pixel holds MAP_EMPTY (z is finite and > 0, so no written word reaches it).  A pixel keeps the minimum word.
struct MapViewK {  // one view of a launch
  float Rc[9], tc[3];  // world -> camera, Rc row-major
  float fx, fy, cx, cy, zmin, zmax;
  float hv;            // 0.5f * voxel
  int w, h, splat;
  u64 min_count;
  u64* zbuf;
  float* depth; uint8_t* bgr; unsigned* covered;
};

// One thread per table slot and view (blockIdx.y = view): the voxel's point and colour as k_map_extract forms them, its
// projection, and one 64-bit atomicMin per footprint pixel.  SKIP: a load of the pixel first; the word stored there only ever
// decreases during the launch, so a stored word <= this one (however stale) means the atomic could not change it.
template <bool SKIP>
__global__ void __launch_bounds__(256) k_map_splat(const u64* __restrict__ keys, const MapVal* __restrict__ vals, unsigned cap,
                                                   const MapViewK* __restrict__ views) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cap || keys[i] == MAP_EMPTY) return;
  const MapViewK& vw = views[blockIdx.y];
  const MapVal v = vals[i];
  if (v.n < vw.min_count) return;
  const double inv = (double)v.n;
  const float px = map_mean(v.qx, inv), py = map_mean(v.qy, inv), pz = map_mean(v.qz, inv);
  float pc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) pc[k] = ((vw.Rc[3 * k] * px + vw.Rc[3 * k + 1] * py) + vw.Rc[3 * k + 2] * pz) + vw.tc[k];
  const float z = pc[2];
  if (!isfinite(pc[0]) || !isfinite(pc[1]) || !map_depth_ok(z, vw.zmin, vw.zmax)) return;
  const float u = __fdiv_rn(vw.fx * pc[0], z) + vw.cx;  // tracker.cpp:153-156
  const float w = __fdiv_rn(vw.fy * pc[1], z) + vw.cy;
  if (!(fabsf(u) < 1048576.0f) || !(fabsf(w) < 1048576.0f)) return;  // NaN / inf fail the comparison
  const int iu = (int)floorf(u), iv = (int)floorf(w);
  const int ru = (int)fminf((float)vw.splat, ceilf(__fdiv_rn(vw.hv * vw.fx, z)));
  const int rv = (int)fminf((float)vw.splat, ceilf(__fdiv_rn(vw.hv * vw.fy, z)));
  const int x0 = max(iu - ru, 0), x1 = min(iu + ru, vw.w - 1), y0 = max(iv - rv, 0), y1 = min(iv + rv, vw.h - 1);
  const u64 word = ((u64)__float_as_uint(z) << 32) | map_colour_bgr(v.n, v.sb, v.sg, v.sr);
  for (int y = y0; y <= y1; ++y) {
    u64* row = vw.zbuf + (size_t)y * vw.w;
    for (int x = x0; x <= x1; ++x) {
      if (SKIP && __hip_atomic_load(&row[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= word) continue;
      atomicMin(&row[x], word);
    }
  }
}

// One thread per pixel and view: z-buffer word -> depth / BGR, the word goes back to MAP_EMPTY for the next call, and the
// written pixels are counted per block in LDS, then one atomic per block.
__global__ void __launch_bounds__(256) k_map_view_resolve(const MapViewK* __restrict__ views) {
  __shared__ unsigned s_n;
  const MapViewK& vw = views[blockIdx.y];
  const unsigned npix = (unsigned)(vw.w * vw.h);
  if (blockIdx.x * 256u >= npix) return;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const unsigned p = blockIdx.x * 256 + threadIdx.x;
  if (p < npix) {
    const u64 word = vw.zbuf[p];
    const bool hit = word != MAP_EMPTY;
    vw.depth[p] = hit ? __uint_as_float((unsigned)(word >> 32)) : 0.0f;
    uint8_t* o = vw.bgr + (size_t)p * 3;
    o[0] = hit ? (uint8_t)word : 0; o[1] = hit ? (uint8_t)(word >> 8) : 0; o[2] = hit ? (uint8_t)(word >> 16) : 0;
    if (hit) { vw.zbuf[p] = MAP_EMPTY; atomicAdd(&s_n, 1u); }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(vw.covered, s_n);
}
// room for a call's views: descriptors, counters, z-buffer words (kept MAP_EMPTY), device outputs of a host-output call
static int render_reserve(revo_map* m, int n, size_t words, size_t out_bytes) {
  hipStream_t s = (hipStream_t)m->g.stream;
  TRY(m->views.reserve(n, s));
  TRY(m->cov.reserve(sizeof(unsigned) * n, s));
  if (sizeof(u64) * words > m->zbuf.bytes) m->zbuf_clean = false;
  TRY(m->zbuf.reserve(sizeof(u64) * words, s));
  if (!m->zbuf_clean) HIPCHECK(hipMemsetAsync(m->zbuf.p, 0xff, m->zbuf.bytes, s));
  return m->vout.reserve(out_bytes, s);
}

extern "C" int revo_map_render(revo_map* m, int n, const revo_map_view* views, float* const* depth, uint8_t* const* bgr,
                               uint32_t* covered, int device_out) {
  if (!m || !views || !depth || !bgr) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n < 1) return fail(REVO_ERR_INVALID_ARG, "revo_map_render: n must be >= 1");
  TRY(map_check_side(device_out, "device_out"));
  if (device_out) TRY(map_check_aligned((uintptr_t)covered, 16, "covered is"));
  std::vector<revo_map_view> vs(views, views + n);
  size_t words = 0, out_bytes = 0;
  int max_pix = 0;
  for (int i = 0; i < n; ++i) {
    revo_map_view& v = vs[i];
    const std::string at = "view " + std::to_string(i) + ": ";
    if (!depth[i] || !bgr[i]) return fail(REVO_ERR_INVALID_ARG, at + "null output");
    if (device_out) TRY(map_check_aligned((uintptr_t)depth[i] | (uintptr_t)bgr[i], 16, at + "a device output is"));
    if (v.width < 1 || v.width > 2048 || v.height < 1 || v.height > 2048)
      return fail(REVO_ERR_INVALID_ARG, at + "width and height must be 1 .. 2048");
    if (v.splat_max < 0 || v.splat_max > 8) return fail(REVO_ERR_INVALID_ARG, at + "splat_max must be 0 .. 8");
    if (!pose_is_finite(v.T_w_c)) return fail(REVO_ERR_INVALID_ARG, at + "T_w_c is not finite");
    const float k[6] = {v.fx, v.fy, v.cx, v.cy, v.zmin, v.zmax};
    bool zero = true, finite = true;
    for (float f : k) { zero = zero && f == 0.0f; finite = finite && std::isfinite(f); }
    if (zero) {
      v.fx = m->g.fx; v.fy = m->g.fy; v.cx = m->g.cx; v.cy = m->g.cy; v.zmin = m->g.dmin; v.zmax = m->g.dmax;
    } else {
      if (!finite) return fail(REVO_ERR_INVALID_ARG, at + "intrinsics and depth range must be finite");
      if (!(v.fx > 0.0f) || !(v.fy > 0.0f)) return fail(REVO_ERR_INVALID_ARG, at + "fx and fy must be > 0");
    }
    if (!(v.zmin >= 0.0f) || !(v.zmin < v.zmax)) return fail(REVO_ERR_INVALID_ARG, at + "the depth range needs 0 <= zmin < zmax");
    const size_t np = (size_t)v.width * v.height;
    words += np;
    out_bytes += (np * 7 + 15) & ~(size_t)15;
    max_pix = std::max(max_pix, (int)np);
  }
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  TRY(render_reserve(m, n, words, device_out ? 0 : out_bytes));
  unsigned* d_cov = device_out && covered ? covered : (unsigned*)m->cov.p;
  size_t zo = 0, oo = 0;
  for (int i = 0; i < n; ++i) {
    const revo_map_view& v = vs[i];
    MapViewK& d = m->views.h[i];
    const float* T = v.T_w_c;  // column-major: R(r, c) = T[4 c + r], so Rc(r, c) = R(c, r) = T[4 r + c]
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) d.Rc[3 * r + c] = T[4 * r + c];
      d.tc[r] = -(((d.Rc[3 * r] * T[12]) + (d.Rc[3 * r + 1] * T[13])) + (d.Rc[3 * r + 2] * T[14]));
    }
    d.fx = v.fx; d.fy = v.fy; d.cx = v.cx; d.cy = v.cy; d.zmin = v.zmin; d.zmax = v.zmax;
    d.hv = 0.5f * m->voxel;
    d.w = v.width; d.h = v.height; d.splat = v.splat_max;
    d.min_count = std::max<u64>(v.min_count, 1);
    const size_t np = (size_t)v.width * v.height;
    d.zbuf = (u64*)m->zbuf.p + zo;
    zo += np;
    if (device_out) { d.depth = depth[i]; d.bgr = bgr[i]; }
    else { d.depth = (float*)(m->vout.p + oo); d.bgr = (uint8_t*)(m->vout.p + oo + np * 4); oo += (np * 7 + 15) & ~(size_t)15; }
    d.covered = d_cov + i;
  }
  TRY(m->views.upload(n, s));
  HIPCHECK(hipMemsetAsync(d_cov, 0, sizeof(unsigned) * n, s));
  m->zbuf_clean = false;  // until the resolve launch that puts every word back is enqueued
  TRY(m->render_time.begin(s));
  const dim3 blk(256), sgrid((unsigned)((m->cap + 255) / 256), (unsigned)n), rgrid((unsigned)((max_pix + 255) / 256), (unsigned)n);
  // REVO_MAP_RENDER_SKIP=0: every footprint pixel takes its atomic without the load in front (profiles/map_render_rates.py)
  if (env_int("REVO_MAP_RENDER_SKIP", 1, 0, 1))
    hipLaunchKernelGGL(k_map_splat<true>, sgrid, blk, 0, s, m->d_keys, m->d_vals, (unsigned)m->cap, m->views.d);
  else
    hipLaunchKernelGGL(k_map_splat<false>, sgrid, blk, 0, s, m->d_keys, m->d_vals, (unsigned)m->cap, m->views.d);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_map_view_resolve, rgrid, blk, 0, s, m->views.d);
  HIPCHECK(hipGetLastError());
  m->zbuf_clean = true;
  TRY(m->render_time.end(s));
  if (device_out) return REVO_OK;
  oo = 0;
  for (int i = 0; i < n; ++i) {
    const size_t np = (size_t)vs[i].width * vs[i].height;
    HIPCHECK(hipMemcpyAsync(depth[i], m->vout.p + oo, np * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(bgr[i], m->vout.p + oo + np * 4, np * 3, hipMemcpyDeviceToHost, s));
    oo += (np * 7 + 15) & ~(size_t)15;
  }
  if (covered) HIPCHECK(hipMemcpyAsync(covered, d_cov, sizeof(unsigned) * n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_render_last_ms(revo_map* m, float* ms) {
  if (!m || !ms) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!m->render_time.ready) return fail(REVO_ERR_INVALID_ARG, "the map has rendered nothing yet");
  HIPCHECK(hipSetDevice(m->g.device));
  return m->render_time.last_ms(ms);
}
// --------------------------------------------------------------------------------------------- rays through the map (20) --
// revo_map_raycast / revo_map_cast_rays (contract: include/revo_hip.h).
struct MapRayOut { u64 key; float s; unsigned cells; float z; unsigned bgr; };  // z, bgr (B | G << 8 | R << 16): view rays only
enum { RAY_HIT = 0, RAY_RANGE = 1, RAY_OUTSIDE = 2, RAY_EXHAUSTED = 3, RAY_STATUSES = 4 };

// step, pos and the first crossing parameter of one axis
__device__ __forceinline__ void map_ray_axis(float o, float d, int k, float voxel, int& step, int& pos, float& inv, float& t) {
  inv = __fdiv_rn(1.0f, d);
  step = d > 0.0f ? 1 : (d < 0.0f ? -1 : 0);
  pos = d > 0.0f ? 1 : 0;
  if (!isfinite(inv)) step = 0;
  t = step ? ((float)(k + pos) * voxel - o) * inv : INFINITY;
}

// The one text of the contract's march.  VIEW: the voxel must also lie in the view's depth range (vw's Rc, tc, zmin, zmax).
// The axis choice is written with selects on scalars: no private array is indexed at run time.  The block table only decides
// whether the fine table is asked; the stepping does not know of it.
template <bool VIEW>
__device__ __forceinline__ int map_ray_march(const MapRayK& a, const RayView* vw, float ox, float oy, float oz, float s0, float dx,
                                             float dy, float dz, float s1, MapRayOut& out) {
  out.key = MAP_EMPTY; out.s = 0.0f; out.cells = 0; out.z = 0.0f; out.bgr = 0;
  const float gx = ox + s0 * dx, gy = oy + s0 * dy, gz = oz + s0 * dz;
  const float fx = floorf(__fdiv_rn(gx, a.voxel)), fy = floorf(__fdiv_rn(gy, a.voxel)), fz = floorf(__fdiv_rn(gz, a.voxel));
  if (!(s0 < s1) || !isfinite(s1) || !isfinite(gx) || !isfinite(gy) || !isfinite(gz)) return RAY_OUTSIDE;
  if (!(fx >= -1048576.0f && fx <= 1048575.0f && fy >= -1048576.0f && fy <= 1048575.0f && fz >= -1048576.0f && fz <= 1048575.0f))
    return RAY_OUTSIDE;
  int kx = (int)fx, ky = (int)fy, kz = (int)fz;
  int stx, sty, stz, psx, psy, psz;
  float ivx, ivy, ivz, tx, ty, tz;
  map_ray_axis(ox, dx, kx, a.voxel, stx, psx, ivx, tx);
  map_ray_axis(oy, dy, ky, a.voxel, sty, psy, ivy, ty);
  map_ray_axis(oz, dz, kz, a.voxel, stz, psz, ivz, tz);
  float s = s0;
  unsigned cells = 0;
  u64 last_block = MAP_EMPTY;  // no block key reaches it
  bool block_occupied = true;
  for (;;) {
    if (cells == a.max_steps) { out.cells = cells; return RAY_EXHAUSTED; }
    ++cells;
    out.s = s;
    const u64 key = map_key(kx, ky, kz);
    if (a.bkeys) {
      const u64 bk = map_key(kx >> 3, ky >> 3, kz >> 3);  // map_coarse_key(key, 3), as k_map_ray_blocks forms it
      if (bk != last_block) { last_block = bk; block_occupied = map_find(a.bkeys, a.bmask, bk) != ~0u; }
    }
    if (block_occupied) {
      const unsigned slot = map_find(a.keys, a.mask, key);
      if (slot != ~0u) {
        const ulonglong2* v = (const ulonglong2*)(a.vals + slot);
        const ulonglong2 p = v[0];  // n qx
        if (p.x >= a.min_count) {
          bool solid = true;
          if (VIEW) {
            const ulonglong2 q = v[1], c = v[2], e = v[3];  // qy qz | sb sg | sr -
            const double inv = (double)p.x;
            const float px = map_mean(p.y, inv), py = map_mean(q.x, inv), pz = map_mean(q.y, inv);
            const float x = ((vw->Rc[0] * px + vw->Rc[1] * py) + vw->Rc[2] * pz) + vw->tc[0];
            const float y = ((vw->Rc[3] * px + vw->Rc[4] * py) + vw->Rc[5] * pz) + vw->tc[1];
            const float z = ((vw->Rc[6] * px + vw->Rc[7] * py) + vw->Rc[8] * pz) + vw->tc[2];
            solid = isfinite(x) && isfinite(y) && map_depth_ok(z, vw->zmin, vw->zmax);
            if (solid) { out.z = z; out.bgr = (unsigned)map_colour_bgr(p.x, c.x, c.y, e.x); }
          }
          if (solid) { out.key = key; out.cells = cells; return RAY_HIT; }
        }
      }
    }
    int ax = 0;
    float sn = tx;
    if (ty < sn) { ax = 1; sn = ty; }
    if (tz < sn) { ax = 2; sn = tz; }
    if (!(sn < s1)) { out.cells = cells; return RAY_RANGE; }
    const int kn = (ax == 0 ? kx + stx : (ax == 1 ? ky + sty : kz + stz));
    if (kn < -(1 << 20) || kn > (1 << 20) - 1) { out.cells = cells; return RAY_OUTSIDE; }
    const int pn = kn + (ax == 0 ? psx : (ax == 1 ? psy : psz));
    const float tn = ((float)pn * a.voxel - (ax == 0 ? ox : (ax == 1 ? oy : oz))) * (ax == 0 ? ivx : (ax == 1 ? ivy : ivz));
    s = sn;
    if (ax == 0) { kx = kn; tx = tn; } else if (ax == 1) { ky = kn; ty = tn; } else { kz = kn; tz = tn; }
  }
}

// One thread per slot of the table: the key of the 8 x 8 x 8 block around every voxel with count >= min_count goes into a
// keys-only table of as many slots (a block holds at least one voxel, so its load is at most the map's).
__global__ void __launch_bounds__(256) k_map_ray_blocks(const u64* __restrict__ keys, const MapVal* __restrict__ vals, unsigned cap,
                                                        u64 min_count, u64* bkeys, unsigned bmask, u64* fault) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  const u64 key = keys[i];
  if (key == MAP_EMPTY || vals[i].n < min_count) return;
  map_slot<true>(bkeys, bmask, map_coarse_key(key, 3), nullptr, fault);
}

// The statuses and cells of a block's rays: ballots per wave into LDS, then one global atomic per counter.  Every thread of
// the block calls it (status < 0: no ray).
__device__ __forceinline__ void map_ray_count(const MapRayK& a, int status, unsigned cells, unsigned* s_cnt, u64* s_cells, unsigned* hits) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < RAY_STATUSES; ++k) {
    const u64 b = __ballot(status == k);
    if (lane == 0 && b) atomicAdd(&s_cnt[k], (unsigned)__popcll(b));
  }
  unsigned c = status < 0 ? 0u : cells;  // <= 2^20 per ray: a wave's sum fits
#pragma unroll
  for (int off = 32; off; off >>= 1) c += __shfl_down(c, off, 64);
  if (lane == 0 && c) atomicAdd(s_cells, (u64)c);
  __syncthreads();
  if (threadIdx.x < RAY_STATUSES && s_cnt[threadIdx.x]) atomicAdd(&a.info[1 + threadIdx.x], (u64)s_cnt[threadIdx.x]);
  if (threadIdx.x == 4 && *s_cells) atomicAdd(&a.info[5], *s_cells);
  if (threadIdx.x == 5) {
    const unsigned rays = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (rays) atomicAdd(&a.info[0], (u64)rays);
  }
  if (threadIdx.x == 6 && hits && s_cnt[RAY_HIT]) atomicAdd(hits, s_cnt[RAY_HIT]);
}

// One thread per pixel, blockIdx.y = view.  A wave is an 8 x 8 pixel tile (its rays end after similar numbers of steps), a
// block four tiles side by side; blocks past a view's tiles leave at once.
__global__ void __launch_bounds__(256) k_map_raycast(const MapRayK a, const MapRayView* __restrict__ views) {
  __shared__ unsigned s_cnt[RAY_STATUSES];
  __shared__ u64 s_cells;
  const MapRayView& vw = views[blockIdx.y];
  const RayView& c = vw.v;
  const unsigned bw = (unsigned)(c.w + 31) / 32, bh = (unsigned)(c.h + 7) / 8;
  if (blockIdx.x >= bw * bh) return;
  if (threadIdx.x < RAY_STATUSES) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 4) s_cells = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int x = (int)((blockIdx.x % bw) * 32 + (threadIdx.x >> 6) * 8 + (lane & 7));
  const int y = (int)((blockIdx.x / bw) * 8 + (lane >> 3));
  int status = -1;
  MapRayOut o{};
  if (x < c.w && y < c.h) {
    const float dcx = __fdiv_rn((float)x - c.cx, c.fx), dcy = __fdiv_rn((float)y - c.cy, c.fy);
    const float dx = ((c.R[0] * dcx) + (c.R[1] * dcy)) + c.R[2];
    const float dy = ((c.R[3] * dcx) + (c.R[4] * dcy)) + c.R[5];
    const float dz = ((c.R[6] * dcx) + (c.R[7] * dcy)) + c.R[8];
    status = map_ray_march<true>(a, &c, c.o[0], c.o[1], c.o[2], c.zmin, dx, dy, dz, c.zmax, o);
    const size_t p = (size_t)y * c.w + x;
    vw.depth[p] = o.z;  // 0 unless a hit
    if (vw.bgr) {
      uint8_t* b = vw.bgr + p * 3;
      b[0] = (uint8_t)o.bgr; b[1] = (uint8_t)(o.bgr >> 8); b[2] = (uint8_t)(o.bgr >> 16);
    }
    if (vw.key) vw.key[p] = o.key;
  }
  map_ray_count(a, status, o.cells, s_cnt, &s_cells, vw.hits);
}

// One thread per given ray: two 16-byte loads, the march, one 16-byte store.
__global__ void __launch_bounds__(256) k_map_cast_rays(const MapRayK a, const float4* __restrict__ rays, unsigned n, ulonglong2* out) {
  __shared__ unsigned s_cnt[RAY_STATUSES];
  __shared__ u64 s_cells;
  if (threadIdx.x < RAY_STATUSES) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 4) s_cells = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  int status = -1;
  MapRayOut o{};
  if (i < n) {
    const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];  // o s0 | d s1
    status = map_ray_march<false>(a, nullptr, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, o);
    out[i] = make_ulonglong2(o.key, (u64)__float_as_uint(o.s) | ((u64)(o.cells | ((unsigned)status << 30)) << 32));
  }
  map_ray_count(a, status, o.cells, s_cnt, &s_cells, nullptr);
}

static_assert(sizeof(revo_map_ray_params) == 16 && offsetof(revo_map_ray_params, max_steps) == 0 && offsetof(revo_map_ray_params, reserved) == 4,
              "the parameter record is the documented layout");
static_assert(sizeof(revo_map_ray) == 32 && offsetof(revo_map_ray, o) == 0 && offsetof(revo_map_ray, s0) == 12 &&
              offsetof(revo_map_ray, d) == 16 && offsetof(revo_map_ray, s1) == 28, "a ray is the kernel's two 16-byte words");
static_assert(sizeof(revo_map_ray_hit) == 16 && offsetof(revo_map_ray_hit, key) == 0 && offsetof(revo_map_ray_hit, s) == 8 &&
              offsetof(revo_map_ray_hit, cells) == 12, "a ray's result is the kernel's one 16-byte word");
static_assert(sizeof(revo_map_ray_info) == 64 && offsetof(revo_map_ray_info, rays) == 0 && offsetof(revo_map_ray_info, hits) == 8 * (1 + RAY_HIT) &&
              offsetof(revo_map_ray_info, range) == 8 * (1 + RAY_RANGE) && offsetof(revo_map_ray_info, outside) == 8 * (1 + RAY_OUTSIDE) &&
              offsetof(revo_map_ray_info, exhausted) == 8 * (1 + RAY_EXHAUSTED) && offsetof(revo_map_ray_info, cells) == 40 &&
              offsetof(revo_map_ray_info, reserved) == 48, "the info record is the kernel's counter line");
static_assert(REVO_RAY_HIT == RAY_HIT && REVO_RAY_RANGE == RAY_RANGE && REVO_RAY_OUTSIDE == RAY_OUTSIDE && REVO_RAY_EXHAUSTED == RAY_EXHAUSTED,
              "the header's statuses are the kernel's");

// Room for a call: the block table (as many slots as the map's table), the counter lines ([0, 64) the info line,
// [64, 64 + 4 x 64) the views' hits), the views' descriptors, the device outputs of a host-output call.
static int ray_reserve(revo_map* m, int n_views, size_t out_bytes) {
  hipStream_t s = (hipStream_t)m->g.stream;
  TRY(m->rcnt.reserve(512, s));
  TRY(m->rviews.reserve(n_views, s));
  TRY(m->bkeys.reserve(sizeof(u64) * m->cap, s));
  return m->rout.reserve(out_bytes, s);
}

// What both entry points share: the first event, the block table of the map as it is on the stream, the cleared counters.
// timer: the handle's ray_time for revo_map_raycast and revo_map_cast_rays, which own it; NULL for the march of another feature
// (map_ray_open), so that revo_map_raycast_last_ms keeps describing the last ray cast, or refuses where there was none.
// REVO_MAP_RAYCAST_BLOCKS=0: no block table, every cell is looked up (the exactness test and profiles/map_raycast_rates.py).
static int ray_begin(revo_map* m, MapRayK* a, u64 min_count, unsigned max_steps, u64* d_info, unsigned* d_hits, int n_hits, EventTimer* timer) {
  hipStream_t s = (hipStream_t)m->g.stream;
  a->keys = m->d_keys; a->vals = m->d_vals; a->mask = (unsigned)(m->cap - 1);
  a->min_count = min_count; a->max_steps = max_steps; a->voxel = m->voxel;
  a->info = d_info;
  if (timer) TRY(timer->begin(s));
  a->bkeys = nullptr; a->bmask = 0;
  if (env_int("REVO_MAP_RAYCAST_BLOCKS", 1, 0, 1)) {
    u64* bkeys = (u64*)m->bkeys.p;
    HIPCHECK(hipMemsetAsync(bkeys, 0xff, sizeof(u64) * m->cap, s));
    hipLaunchKernelGGL(k_map_ray_blocks, dim3((unsigned)((m->cap + 255) / 256)), dim3(256), 0, s, m->d_keys, m->d_vals, (unsigned)m->cap,
                       min_count, bkeys, (unsigned)(m->cap - 1), &m->d_st->fault);
    HIPCHECK(hipGetLastError());
    a->bkeys = bkeys; a->bmask = (unsigned)(m->cap - 1);
  }
  HIPCHECK(hipMemsetAsync(d_info, 0, sizeof(revo_map_ray_info), s));
  if (n_hits) HIPCHECK(hipMemsetAsync(d_hits, 0, sizeof(unsigned) * n_hits, s));
  return REVO_OK;
}

// For revo_map_gain.hip (declared in revo_map_impl.h): the same block table, march and counters over views the caller has
// written to device memory.
int map_ray_open(revo_map* m, MapRayK* a, uint32_t min_count, uint32_t max_steps, u64* d_info) {
  TRY(m->bkeys.reserve(sizeof(u64) * m->cap, (hipStream_t)m->g.stream));
  return ray_begin(m, a, std::max<u64>(min_count, 1), max_steps, d_info, nullptr, 0, nullptr);
}
int map_ray_views(revo_map* m, const MapRayK& a, int n, const MapRayView* d_views, int max_blocks) {
  hipStream_t s = (hipStream_t)m->g.stream;
  hipLaunchKernelGGL(k_map_raycast, dim3((unsigned)max_blocks, (unsigned)n), dim3(256), 0, s, a, d_views);
  HIPCHECK(hipGetLastError());
  return REVO_OK;
}

extern "C" int revo_map_raycast(revo_map* m, int n, const revo_map_view* views, const revo_map_ray_params* prm, float* const* depth,
                                uint8_t* const* bgr, uint64_t* const* key, uint32_t* hits, int device_out, revo_map_ray_info* info) {
  if (!m || !views || !depth) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n < 1 || n > RAY_MAX_VIEWS) return fail(REVO_ERR_INVALID_ARG, "revo_map_raycast: n must be 1 .. 64 views");
  TRY(map_check_side(device_out, "device_out"));
  if (device_out) TRY(map_check_aligned((uintptr_t)hits | (uintptr_t)info, 16, "hits or info is"));
  uint32_t max_steps = 0;
  if (const char* why = ray_params_check(prm, &max_steps)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_raycast: ") + why);
  const CarveCam cam{m->g.fx, m->g.fy, m->g.cx, m->g.cy, m->g.dmin, m->g.dmax};
  std::vector<RayView> rv(n);
  size_t out_bytes = 0;
  int max_blocks = 0;
  for (int i = 0; i < n; ++i) {
    const std::string at = "view " + std::to_string(i) + ": ";
    if (!depth[i] || (bgr && !bgr[i]) || (key && !key[i])) return fail(REVO_ERR_INVALID_ARG, at + "null output");
    if (device_out)
      TRY(map_check_aligned((uintptr_t)depth[i] | (uintptr_t)(bgr ? bgr[i] : nullptr) | (uintptr_t)(key ? key[i] : nullptr), 16,
                                at + "a device output is"));
    if (const char* why = ray_view_check(&views[i], cam, &rv[i])) return fail(REVO_ERR_INVALID_ARG, at + why);
    const size_t np = (size_t)rv[i].w * rv[i].h;
    out_bytes += (np * (4 + (bgr ? 3 : 0) + (key ? 8 : 0)) + 15) & ~(size_t)15;
    max_blocks = std::max(max_blocks, ((rv[i].w + 31) / 32) * ((rv[i].h + 7) / 8));
  }
  const uint32_t min_count = ray_views_min_count(views, n);
  if (!min_count) return fail(REVO_ERR_INVALID_ARG, "revo_map_raycast: every view of a call must carry the same min_count");
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  TRY(ray_reserve(m, n, device_out ? 0 : out_bytes));
  u64* d_info = device_out && info ? (u64*)info : (u64*)m->rcnt.p;
  unsigned* d_hits = device_out && hits ? hits : (unsigned*)(m->rcnt.p + 64);
  size_t oo = 0;
  for (int i = 0; i < n; ++i) {
    MapRayView& d = m->rviews.h[i];
    d.v = rv[i];
    const size_t np = (size_t)rv[i].w * rv[i].h;
    if (device_out) {
      d.depth = depth[i]; d.bgr = bgr ? bgr[i] : nullptr; d.key = key ? (u64*)key[i] : nullptr;
    } else {  // keys, depth, colour: the widest first
      char* b = m->rout.p + oo;
      d.key = key ? (u64*)b : nullptr;
      b += key ? np * 8 : 0;
      d.depth = (float*)b;
      d.bgr = bgr ? (uint8_t*)(b + np * 4) : nullptr;
      oo += (np * (4 + (bgr ? 3 : 0) + (key ? 8 : 0)) + 15) & ~(size_t)15;
    }
    d.hits = d_hits + i;
  }
  TRY(m->rviews.upload(n, s));
  MapRayK a{};
  TRY(ray_begin(m, &a, min_count, max_steps, d_info, d_hits, n, &m->ray_time));
  hipLaunchKernelGGL(k_map_raycast, dim3((unsigned)max_blocks, (unsigned)n), dim3(256), 0, s, a, m->rviews.d);
  HIPCHECK(hipGetLastError());
  TRY(m->ray_time.end(s));
  if (device_out) return REVO_OK;
  for (int i = 0; i < n; ++i) {
    const MapRayView& d = m->rviews.h[i];
    const size_t np = (size_t)rv[i].w * rv[i].h;
    HIPCHECK(hipMemcpyAsync(depth[i], d.depth, np * 4, hipMemcpyDeviceToHost, s));
    if (bgr) HIPCHECK(hipMemcpyAsync(bgr[i], d.bgr, np * 3, hipMemcpyDeviceToHost, s));
    if (key) HIPCHECK(hipMemcpyAsync(key[i], d.key, np * 8, hipMemcpyDeviceToHost, s));
  }
  if (hits) HIPCHECK(hipMemcpyAsync(hits, d_hits, sizeof(unsigned) * n, hipMemcpyDeviceToHost, s));
  if (info) HIPCHECK(hipMemcpyAsync(info, d_info, sizeof(revo_map_ray_info), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_cast_rays(revo_map* m, size_t n, const revo_map_ray* rays, int device_in, uint32_t min_count,
                                  const revo_map_ray_params* prm, revo_map_ray_hit* out, int device_out, revo_map_ray_info* info) {
  if (!m || !rays || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n < 1 || n > RAY_MAX_RAYS) return fail(REVO_ERR_INVALID_ARG, "revo_map_cast_rays: n must be 1 .. 2^24 rays");
  TRY(map_check_side(device_in, "device_in"));
  TRY(map_check_side(device_out, "device_out"));
  if (device_in) TRY(map_check_aligned((uintptr_t)rays, 16, "the device rays are"));
  if (device_out) TRY(map_check_aligned((uintptr_t)out | (uintptr_t)info, 16, "a device output is"));
  uint32_t max_steps = 0;
  if (const char* why = ray_params_check(prm, &max_steps)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_cast_rays: ") + why);
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  TRY(ray_reserve(m, 0, device_out ? 0 : sizeof(revo_map_ray_hit) * n));
  DevScratch up;  // freed after the wait below
  const float4* d_rays = (const float4*)rays;
  if (!device_in) {
    TRY(up.alloc(sizeof(revo_map_ray) * n));
    HIPCHECK(hipMemcpyAsync(up.p, rays, sizeof(revo_map_ray) * n, hipMemcpyHostToDevice, s));
    d_rays = (const float4*)up.p;
  }
  u64* d_info = device_out && info ? (u64*)info : (u64*)m->rcnt.p;
  ulonglong2* d_out = device_out ? (ulonglong2*)out : (ulonglong2*)m->rout.p;
  MapRayK a{};
  { const int rc = ray_begin(m, &a, std::max<u64>(min_count, 1), max_steps, d_info, nullptr, 0, &m->ray_time); if (rc) { (void)hipStreamSynchronize(s); return rc; } }
  hipLaunchKernelGGL(k_map_cast_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, d_rays, (unsigned)n, d_out);
  if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(s); return fail(REVO_ERR_HIP, "k_map_cast_rays: the launch failed"); }
  TRY(m->ray_time.end(s));
  if (!device_out) {
    HIPCHECK(hipMemcpyAsync(out, d_out, sizeof(revo_map_ray_hit) * n, hipMemcpyDeviceToHost, s));
    if (info) HIPCHECK(hipMemcpyAsync(info, d_info, sizeof(revo_map_ray_info), hipMemcpyDeviceToHost, s));
  }
  if (!device_out || !device_in) HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_raycast_last_ms(revo_map* m, float* ms) {
  if (!m || !ms) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!m->ray_time.ready) return fail(REVO_ERR_INVALID_ARG, "the map has cast nothing yet");
  HIPCHECK(hipSetDevice(m->g.device));
  return m->ray_time.last_ms(ms);
}
