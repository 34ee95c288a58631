// revo_map_gain.hip -- what a view would add: revo_map_view_gain, for a batch of candidate camera poses the unknown
// cells of a seen volume that one depth view from each pose would make known.  The predicted depth images come from
// revo_map_raycast's own launches (revo_map_view.hip), 64 poses at a time, into a scratch of the handle; k_map_gain then
// classifies the unknown cells of each pose's cull range against its image and counts.  Nothing but the records is written.
// Contract: include/revo_hip.h.  Every value is an integer that float32 arithmetic with one definition decides.
#include "revo_map_impl.h"
#include "revo_seen_host.h"
#include "revo_gain_host.h"

#define GAIN_RUN 4  // consecutive z-cells of a thread: one 32-bit word of the volume where the line's start allows it

struct MapGainPose {  // one pose of a launch, in device memory
  MapCarveView cv;    // the predicted view as map_carve_class takes it
  GainRange rg;       // the cull: the cells of the box the kernel visits
  int z0;             // rg.lo[2] rounded down to a multiple of GAIN_RUN
  unsigned wzr;       // runs per z-line of the range
  unsigned words;     // rg.n[0] * rg.n[1] * wzr (0: nothing to visit)
  unsigned pad;
};
struct MapGainK {
  const MapGainPose* poses;  // the launch's poses: blockIdx.y
  revo_map_gain* out;        // their records
  const unsigned* bits; unsigned wz;  // the box's solid voxels, as k_df_occupancy leaves them
  const uint8_t* seen;
  revo_map_df_box box;
  unsigned min_views;
  int radius;
  float margin, margin_rel, voxel;
  u64* info;  // one 64-byte line: revo_map_gain_info
};
enum { GAIN_POSES = 0, GAIN_CELLS = 1, GAIN_UNKNOWN = 2, GAIN_FREE = 3, GAIN_SURFACE = 4, GAIN_INSIDE = 5, GAIN_RAYS = 6, GAIN_RAY_HITS = 7 };

static_assert(sizeof(revo_map_gain_params) == 32 && offsetof(revo_map_gain_params, min_views) == 4 && offsetof(revo_map_gain_params, margin) == 8 &&
              offsetof(revo_map_gain_params, margin_rel) == 12 && offsetof(revo_map_gain_params, miss_depth) == 16 &&
              offsetof(revo_map_gain_params, max_steps) == 20 && offsetof(revo_map_gain_params, reserved) == 24, "the parameter record is the documented layout");
static_assert(sizeof(revo_map_gain) == 32 && offsetof(revo_map_gain, unknown_free) == 0 && offsetof(revo_map_gain, unknown_surface) == 4 &&
              offsetof(revo_map_gain, unknown_inside) == 8 && offsetof(revo_map_gain, hits) == 12 && offsetof(revo_map_gain, reserved) == 16,
              "a pose's record is the kernels' eight words");
static_assert(sizeof(revo_map_gain_info) == 64 && offsetof(revo_map_gain_info, poses) == 8 * GAIN_POSES && offsetof(revo_map_gain_info, cells) == 8 * GAIN_CELLS &&
              offsetof(revo_map_gain_info, unknown) == 8 * GAIN_UNKNOWN && offsetof(revo_map_gain_info, unknown_free) == 8 * GAIN_FREE &&
              offsetof(revo_map_gain_info, unknown_surface) == 8 * GAIN_SURFACE && offsetof(revo_map_gain_info, unknown_inside) == 8 * GAIN_INSIDE &&
              offsetof(revo_map_gain_info, rays) == 8 * GAIN_RAYS && offsetof(revo_map_gain_info, ray_hits) == 8 * GAIN_RAY_HITS,
              "the info record is the kernels' counter line");
static_assert(offsetof(revo_map_ray_info, rays) == 0 && offsetof(revo_map_ray_info, hits) == 8, "rays and hits of the ray line are copied as one piece");
static_assert(GAIN_CHUNK == RAY_MAX_VIEWS, "a launch's poses are one ray cast's views");

// The two records of pose i of the call: the ray view (its image is slot i % GAIN_CHUNK of the scratch, its hit counter the
// record's fourth word) and the gain pose.  One text for the host (poses in host memory) and k_gain_poses (device memory).
__host__ __device__ inline void gain_describe(const RayView& cam, const float* T, int radius, const revo_map_df_box& box, float voxel, float* depth,
                                              revo_map_gain* rec, MapRayView* rv, MapGainPose* gp) {
  gain_pose_view(cam, T, &rv->v);
  rv->depth = depth; rv->bgr = nullptr; rv->key = nullptr; rv->hits = &rec->hits;
  const RayView& v = rv->v;
  CarveView& c = gp->cv.v;
  for (int k = 0; k < 9; ++k) c.Rc[k] = v.Rc[k];
  for (int k = 0; k < 3; ++k) c.tc[k] = v.tc[k];
  c.fx = v.fx; c.fy = v.fy; c.cx = v.cx; c.cy = v.cy; c.zmin = v.zmin; c.zmax = v.zmax;
  c.w = v.w; c.h = v.h;
  gp->cv.depth = depth;
  gp->rg = gain_cull(v, radius, box, voxel);
  gp->z0 = gp->rg.lo[2] & ~(GAIN_RUN - 1);
  gp->wzr = gp->rg.n[2] ? (unsigned)(((gp->rg.lo[2] + gp->rg.n[2] - 1) - gp->z0) / GAIN_RUN + 1) : 0u;
  gp->words = (unsigned)gp->rg.n[0] * (unsigned)gp->rg.n[1] * gp->wzr;
  gp->pad = 0;
}

// One thread per pose of the call, for poses in device memory.
__global__ void __launch_bounds__(64) k_gain_poses(const RayView cam, const float* __restrict__ T_n16, unsigned n, int radius, const revo_map_df_box box,
                                                   float voxel, float* depth, size_t image, revo_map_gain* out, MapRayView* rv, MapGainPose* gp) {
  const unsigned i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  float T[16];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float4 c = ((const float4*)T_n16)[4 * (size_t)i + k];
    T[4 * k] = c.x; T[4 * k + 1] = c.y; T[4 * k + 2] = c.z; T[4 * k + 3] = c.w;
  }
  gain_describe(cam, T, radius, box, voxel, depth + (size_t)(i % GAIN_CHUNK) * image, out + i, rv + i, gp + i);
}

// miss_depth != 0: a pixel whose ray hit nothing (depth 0; a hit's depth is above zmin >= 0) reads as miss_depth.
__global__ void __launch_bounds__(256) k_gain_fill_miss(float* depth, size_t n, float miss_depth) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n && depth[i] == 0.0f) depth[i] = miss_depth;
}

// The unknown cells of the box: k_df_unknown's word logic without its store.  One lane per 32-cell word of the bit volume.
__global__ void __launch_bounds__(256) k_gain_unknown(const uint8_t* __restrict__ seen, const revo_map_df_box box, unsigned wz, unsigned min_views,
                                                      const unsigned* __restrict__ bits, unsigned n_poses, u64* info) {
  __shared__ unsigned s_cnt;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const unsigned words = (unsigned)box.n[0] * (unsigned)box.n[1] * wz;
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  unsigned n_unknown = 0;
  if (i < words) {
    const unsigned line = i / wz, w = i - line * wz;
    const unsigned nz = (unsigned)box.n[2], z0 = w * 32, len = min(32u, nz - z0);
    const uint8_t* row = seen + (size_t)line * nz + z0;
    const unsigned solid = bits[i];
    unsigned unknown = 0;
    for (unsigned k = 0; k < len; ++k)
      unknown |= (seen_is_unknown((solid >> k) & 1u, row[k], min_views) ? 1u : 0u) << k;
    n_unknown = (unsigned)__popc(unknown);
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) n_unknown += __shfl_down(n_unknown, off, 64);
  if ((threadIdx.x & 63) == 0 && n_unknown) atomicAdd(&s_cnt, n_unknown);
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(&info[GAIN_UNKNOWN], (u64)s_cnt);
  if (blockIdx.x == 0 && threadIdx.x == 1) {
    info[GAIN_POSES] = (u64)n_poses;
    info[GAIN_CELLS] = (u64)box.n[0] * box.n[1] * box.n[2];
  }
}

// blockIdx.y: the pose (its descriptor is read through a uniform address), blockIdx.x * 256 + threadIdx.x: a run of GAIN_RUN
// consecutive z-cells of the pose's cull range, z fastest, so a wave's centres project to neighbouring pixels.  A thread reads
// the run's seen bytes (one word where the run lies inside the line and its address is a multiple of four, else byte by byte)
// and leaves when none says unknown: a known cell costs that load.  Otherwise the solid bits join, and the cells still unknown
// are classified.  The grid is sized for the largest range of the launch (the whole box when the host has not seen the poses);
// blocks past a pose's range leave at once.  A run may stick out of the range along z: such cells are classified like the
// others -- the range only says where not to look.  Counting: three 10-bit fields (<= 4 per thread, <= 256 per wave) summed
// over the wave, then LDS, then one global atomic per block and counter.
__global__ void __launch_bounds__(256) k_map_gain(const MapGainK a) {
  __shared__ unsigned s_cnt[3];  // free, surface, inside
  const MapGainPose& g = a.poses[blockIdx.y];
  if (blockIdx.x * 256u >= g.words) return;  // the whole block
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  unsigned packed = 0;
  if (t < g.words) {
    const unsigned ny = (unsigned)a.box.n[1], nz = (unsigned)a.box.n[2];
    const unsigned lr = t / g.wzr, k = t - lr * g.wzr;
    const unsigned xr = lr / (unsigned)g.rg.n[1], yr = lr - xr * (unsigned)g.rg.n[1];
    const unsigned ix = (unsigned)g.rg.lo[0] + xr, iy = (unsigned)g.rg.lo[1] + yr, iz0 = (unsigned)g.z0 + GAIN_RUN * k;
    const unsigned line = ix * ny + iy;
    const size_t c0 = (size_t)line * nz + iz0;
    unsigned bytes = 0x80808080u;  // a cell past the line's end reads as known
    if (iz0 + GAIN_RUN <= nz && (c0 & 3) == 0) {
      bytes = *(const unsigned*)(a.seen + c0);
    } else {
#pragma unroll
      for (int j = 0; j < GAIN_RUN; ++j)
        if (iz0 + j < nz) bytes = (bytes & ~(0xffu << (8 * j))) | ((unsigned)a.seen[c0 + j] << (8 * j));
    }
    unsigned cand = 0;
#pragma unroll
    for (int j = 0; j < GAIN_RUN; ++j) cand |= (seen_is_known((uint8_t)(bytes >> (8 * j)), a.min_views) ? 0u : 1u) << j;
    if (cand) {
      const unsigned solid = (a.bits[(size_t)line * a.wz + (iz0 >> 5)] >> (iz0 & 31)) & 0xfu;  // iz0 is a multiple of four: one word
      cand &= ~solid;
    }
    if (cand) {
      const float px = seen_centre(a.box.lo[0], (int)ix, a.voxel), py = seen_centre(a.box.lo[1], (int)iy, a.voxel);
#pragma unroll
      for (int j = 0; j < GAIN_RUN; ++j) {
        if (!((cand >> j) & 1u)) continue;
        const int cls = map_carve_class(px, py, seen_centre(a.box.lo[2], (int)iz0 + j, a.voxel), g.cv, a.radius, a.margin, a.margin_rel);
        packed += (cls == CARVE_FREE ? 1u : 0u) | (cls == CARVE_CONFIRMED ? 1u << 10 : 0u) | (cls != CARVE_OUTSIDE ? 1u << 20 : 0u);
      }
    }
  }
  if (__ballot(packed != 0)) {  // uniform per wave
#pragma unroll
    for (int off = 32; off; off >>= 1) packed += __shfl_down(packed, off, 64);
    if ((threadIdx.x & 63) == 0) {
      if (packed & 0x3ffu) atomicAdd(&s_cnt[0], packed & 0x3ffu);
      if ((packed >> 10) & 0x3ffu) atomicAdd(&s_cnt[1], (packed >> 10) & 0x3ffu);
      if (packed >> 20) atomicAdd(&s_cnt[2], packed >> 20);
    }
  }
  __syncthreads();
  if (threadIdx.x < 3 && s_cnt[threadIdx.x]) {
    atomicAdd(&a.out[blockIdx.y].unknown_free + threadIdx.x, s_cnt[threadIdx.x]);
    atomicAdd(&a.info[GAIN_FREE + threadIdx.x], (u64)s_cnt[threadIdx.x]);
  }
}

// the runs of a whole box: what a launch's grid covers when the poses' ranges are not known on the host
static unsigned gain_box_words(const revo_map_df_box& b) {
  return (unsigned)b.n[0] * (unsigned)b.n[1] * (unsigned)((b.n[2] + GAIN_RUN - 1) / GAIN_RUN);
}

extern "C" int revo_map_view_gain(revo_map* m, const revo_map_df_box* box, const uint8_t* seen, int device_seen, const revo_map_view* cam,
                                  size_t n_poses, const float* T_w_c_n16, int device_in, const revo_map_gain_params* prm, revo_map_gain* out,
                                  int device_out, revo_map_gain_info* info) {
  if (!m || !box || !seen || !cam || !T_w_c_n16 || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  size_t cells = 0;
  if (const char* why = map_df_box_check(box, &cells)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_view_gain: ") + why);
  if (n_poses < 1 || n_poses > GAIN_MAX_POSES) return fail(REVO_ERR_INVALID_ARG, "revo_map_view_gain: n_poses must be 1 .. 4096");
  TRY(map_check_side(device_seen, "device_seen"));
  TRY(map_check_side(device_in, "device_in"));
  TRY(map_check_side(device_out, "device_out"));
  if (device_seen) TRY(map_check_aligned((uintptr_t)seen, 16, "the device seen volume is"));
  if (device_in) TRY(map_check_aligned((uintptr_t)T_w_c_n16, 16, "the device poses are"));
  if (device_out) TRY(map_check_aligned((uintptr_t)out | (uintptr_t)info, 16, "a device output is"));
  // the camera: revo_map_raycast's view rules, with the identity where a view carries its pose
  revo_map_view cv = *cam;
  for (int k = 0; k < 16; ++k) cv.T_w_c[k] = (k % 5 == 0) ? 1.0f : 0.0f;
  const CarveCam ctx{m->g.fx, m->g.fy, m->g.cx, m->g.cy, m->g.dmin, m->g.dmax};
  RayView rcam;
  if (const char* why = ray_view_check(&cv, ctx, &rcam)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_view_gain: ") + why);
  revo_map_gain_params pp;
  if (const char* why = gain_params_check(prm, m->voxel, rcam.zmin, rcam.zmax, &pp)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_view_gain: ") + why);
  const int n = (int)n_poses;
  if (!device_in)
    for (int i = 0; i < n; ++i)
      if (!gain_pose_ok(T_w_c_n16 + 16 * (size_t)i))
        return fail(REVO_ERR_INVALID_ARG, "revo_map_view_gain: pose " + std::to_string(i) + " is not finite or its rotation is not orthogonal");
  const uint32_t min_count = cam->min_count < 1 ? 1u : cam->min_count;
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t image = (size_t)rcam.w * rcam.h;
  const int chunk = std::min(n, GAIN_CHUNK);
  const size_t rv_bytes = (sizeof(MapRayView) * n_poses + 255) & ~(size_t)255;
  TRY(m->gaindepth.reserve(sizeof(float) * image * chunk, s));
  TRY(m->gaindesc.reserve(rv_bytes + sizeof(MapGainPose) * n_poses, s));
  TRY(m->gaincnt.reserve(256, s));
  TRY(m->seenvol.reserve(device_seen ? 0 : cells, s));
  TRY(m->gainout.reserve(device_out ? 0 : sizeof(revo_map_gain) * n_poses, s));
  float* d_depth = (float*)m->gaindepth.p;
  MapRayView* d_rv = (MapRayView*)m->gaindesc.p;
  MapGainPose* d_gp = (MapGainPose*)(m->gaindesc.p + rv_bytes);
  revo_map_gain* d_out = device_out ? out : (revo_map_gain*)m->gainout.p;
  u64* d_info = device_out && info ? (u64*)info : (u64*)m->gaincnt.p;
  u64* d_rayinfo = (u64*)(m->gaincnt.p + 64);
  const uint8_t* d_seen = seen;
  if (!device_seen) {
    HIPCHECK(hipMemcpyAsync(m->seenvol.p, seen, cells, hipMemcpyHostToDevice, s));
    d_seen = (const uint8_t*)m->seenvol.p;
  }
  HIPCHECK(hipMemsetAsync(d_out, 0, sizeof(revo_map_gain) * n_poses, s));
  HIPCHECK(hipMemsetAsync(d_info, 0, sizeof(revo_map_gain_info), s));
  // the poses' descriptors, and per launch the largest range
  std::vector<unsigned> grid_words((n + GAIN_CHUNK - 1) / GAIN_CHUNK, gain_box_words(*box));
  if (device_in) {
    hipLaunchKernelGGL(k_gain_poses, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, rcam, T_w_c_n16, (unsigned)n, pp.radius, *box, m->voxel, d_depth,
                       image, d_out, d_rv, d_gp);
    HIPCHECK(hipGetLastError());
  } else {
    std::vector<MapRayView> hr(n);
    std::vector<MapGainPose> hg(n);
    std::fill(grid_words.begin(), grid_words.end(), 0u);
    for (int i = 0; i < n; ++i) {
      gain_describe(rcam, T_w_c_n16 + 16 * (size_t)i, pp.radius, *box, m->voxel, d_depth + (size_t)(i % GAIN_CHUNK) * image, d_out + i, &hr[i], &hg[i]);
      grid_words[i / GAIN_CHUNK] = std::max(grid_words[i / GAIN_CHUNK], hg[i].words);
    }
    HIPCHECK(hipMemcpyAsync(d_rv, hr.data(), sizeof(MapRayView) * n_poses, hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemcpyAsync(d_gp, hg.data(), sizeof(MapGainPose) * n_poses, hipMemcpyHostToDevice, s));
    HIPCHECK(hipStreamSynchronize(s));  // the rows are the call's own: read before they go
  }
  MapGainK a{};
  a.seen = d_seen; a.box = *box;
  a.min_views = pp.min_views; a.radius = pp.radius;
  a.margin = pp.margin; a.margin_rel = pp.margin_rel; a.voxel = m->voxel;
  a.info = d_info;
  TRY(map_df_solid_bits(m, box, min_count, s, &a.bits, &a.wz));
  const unsigned bit_words = (unsigned)box->n[0] * (unsigned)box->n[1] * a.wz;
  hipLaunchKernelGGL(k_gain_unknown, dim3((bit_words + 255) / 256), dim3(256), 0, s, d_seen, *box, a.wz, pp.min_views, a.bits, (unsigned)n, d_info);
  HIPCHECK(hipGetLastError());
  MapRayK rk{};
  TRY(map_ray_open(m, &rk, min_count, pp.max_steps, d_rayinfo));
  const int max_blocks = ((rcam.w + 31) / 32) * ((rcam.h + 7) / 8);
  for (int i0 = 0; i0 < n; i0 += GAIN_CHUNK) {
    const int nc = std::min(GAIN_CHUNK, n - i0);
    TRY(map_ray_views(m, rk, nc, d_rv + i0, max_blocks));
    if (pp.miss_depth != 0.0f) {
      const size_t px = image * nc;
      hipLaunchKernelGGL(k_gain_fill_miss, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, d_depth, px, pp.miss_depth);
      HIPCHECK(hipGetLastError());
    }
    const unsigned words = grid_words[i0 / GAIN_CHUNK];
    if (!words) continue;
    a.poses = d_gp + i0; a.out = d_out + i0;
    hipLaunchKernelGGL(k_map_gain, dim3((words + 255) / 256, (unsigned)nc), dim3(256), 0, s, a);
    HIPCHECK(hipGetLastError());
  }
  HIPCHECK(hipMemcpyAsync(d_info + GAIN_RAYS, d_rayinfo, 2 * sizeof(u64), hipMemcpyDeviceToDevice, s));
  if (!device_out) {
    HIPCHECK(hipMemcpyAsync(out, d_out, sizeof(revo_map_gain) * n_poses, hipMemcpyDeviceToHost, s));
    if (info) HIPCHECK(hipMemcpyAsync(info, d_info, sizeof(revo_map_gain_info), hipMemcpyDeviceToHost, s));
  }
  if (!device_seen || !device_in || !device_out) HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}
