// revo_map_tsdf_ray.hip -- views of the surface: revo_map_tsdf_raycast, depth, normal and colour images ray-cast from
// the TSDF volume and its colour volume.  Contract: include/revo_hip.h.  The march and every rule of it are revo_tsdf_ray_host.h's,
// one text for both sides; the two kernels' bodies are revo_tsdf_ray_dev.h's, shared with the batched call; this unit
// holds the block mask's kernel, the kernel that gives every pixel its ray, and the entry point.
#include "revo_map_impl.h"
#include "revo_tsdf_ray_host.h"
#include "revo_tsdf_ray_dev.h"

static_assert(sizeof(revo_map_tsdf_ray_params) == 16 && offsetof(revo_map_tsdf_ray_params, step) == 0 && offsetof(revo_map_tsdf_ray_params, min_weight) == 4 &&
              offsetof(revo_map_tsdf_ray_params, max_steps) == 8 && offsetof(revo_map_tsdf_ray_params, reserved) == 12, "the parameter record is the documented layout");
static_assert(sizeof(revo_map_tsdf_ray_info) == 64 && offsetof(revo_map_tsdf_ray_info, rays) == 8 * TR_RAYS &&
              offsetof(revo_map_tsdf_ray_info, hits) == 8 * (TR_STATUS + TSDF_RAY_HIT) && offsetof(revo_map_tsdf_ray_info, range) == 8 * (TR_STATUS + TSDF_RAY_RANGE) &&
              offsetof(revo_map_tsdf_ray_info, backface) == 8 * (TR_STATUS + TSDF_RAY_BACKFACE) &&
              offsetof(revo_map_tsdf_ray_info, exhausted) == 8 * (TR_STATUS + TSDF_RAY_EXHAUSTED) && offsetof(revo_map_tsdf_ray_info, samples) == 8 * TR_SAMPLES &&
              offsetof(revo_map_tsdf_ray_info, uncolored) == 8 * TR_UNCOLORED && offsetof(revo_map_tsdf_ray_info, reserved) == 56,
              "the info record is the kernel's counter line");
static_assert(REVO_TSDF_RAY_HIT == TSDF_RAY_HIT && REVO_TSDF_RAY_RANGE == TSDF_RAY_RANGE && REVO_TSDF_RAY_BACKFACE == TSDF_RAY_BACKFACE &&
              REVO_TSDF_RAY_EXHAUSTED == TSDF_RAY_EXHAUSTED, "the header's statuses are the kernel's");
static_assert(sizeof(revo_map_tsdf_cell) == 8 && sizeof(revo_map_tsdf_color) == 16, "the volumes' cells are the documented words");

// One thread per cell: tsdf_ray_mask_cell (revo_tsdf_ray_dev.h).
__global__ void __launch_bounds__(256) k_tsdf_ray_mask(const revo_map_tsdf_cell* __restrict__ tsdf, const revo_map_df_box box, unsigned cells,
                                                       unsigned min_weight, int nby, int nbz, unsigned* mask) {
  const unsigned c = blockIdx.x * 256u + threadIdx.x;
  if (c >= cells) return;
  tsdf_ray_mask_cell(tsdf, box, c, min_weight, nby, nbz, mask);
}

// One thread per pixel, blockIdx.y = view; blocks past a view's tiles leave at once.  The view is read through uniform addresses.
// The block's work is tsdf_ray_view_block (revo_tsdf_ray_dev.h).
__global__ void __launch_bounds__(256) k_tsdf_raycast(const TsdfRayK a, const TsdfRayView* __restrict__ views, u64* info) {
  __shared__ TsdfRayTally s;
  const TsdfRayView& vw = views[blockIdx.y];
  const unsigned bw = (unsigned)(vw.v.w + 31) / 32, bh = (unsigned)(vw.v.h + 7) / 8;
  if (blockIdx.x >= bw * bh) return;
  tsdf_ray_view_block(a, vw, blockIdx.x, s, info);
}

// REVO_MAP_TSDF_RAY_MASK=0: no block mask, every sample is evaluated (the exactness test and profiles/map_tsdf_ray_rates.py).
extern "C" int revo_map_tsdf_raycast(revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf, const revo_map_tsdf_color* color,
                                     int device_tsdf, int n, const revo_map_view* views, const revo_map_tsdf_ray_params* prm,
                                     float* const* depth, float* const* normal, uint8_t* const* bgr, uint32_t* hits, int device_out,
                                     revo_map_tsdf_ray_info* info) {
  if (!m || !box || !tsdf || !views || !depth) return fail(REVO_ERR_INVALID_ARG, "null argument");
  const std::string who = "revo_map_tsdf_raycast: ";
  if (bgr && !color) return fail(REVO_ERR_INVALID_ARG, who + "colour images need the colour volume");
  size_t cells = 0;
  if (const char* why = map_df_box_check(box, &cells)) return fail(REVO_ERR_INVALID_ARG, who + why);
  if (n < 1 || n > TSDF_RAY_MAX_VIEWS) return fail(REVO_ERR_INVALID_ARG, who + "n must be 1 .. 64 views");
  TRY(map_check_side(device_tsdf, "device_tsdf"));
  TRY(map_check_side(device_out, "device_out"));
  if (device_tsdf) TRY(map_check_aligned((uintptr_t)tsdf | (uintptr_t)color, 16, "the device volume is"));
  if (device_out) TRY(map_check_aligned((uintptr_t)hits | (uintptr_t)info, 16, "hits or info is"));
  revo_map_tsdf_ray_params pp;
  if (const char* why = tsdf_ray_params_check(prm, m->voxel, &pp)) return fail(REVO_ERR_INVALID_ARG, who + why);
  const CarveCam cam{m->g.fx, m->g.fy, m->g.cx, m->g.cy, m->g.dmin, m->g.dmax};
  std::vector<RayView> rv(n);
  size_t out_bytes = 0;
  int max_blocks = 0;
  const size_t per_pixel = 4 + (normal ? 12 : 0) + (bgr ? 3 : 0);
  for (int i = 0; i < n; ++i) {
    const std::string at = "view " + std::to_string(i) + ": ";
    if (!depth[i] || (normal && !normal[i]) || (bgr && !bgr[i])) return fail(REVO_ERR_INVALID_ARG, at + "null output");
    if (device_out)
      TRY(map_check_aligned((uintptr_t)depth[i] | (uintptr_t)(normal ? normal[i] : nullptr) | (uintptr_t)(bgr ? bgr[i] : nullptr), 16,
                            at + "a device output is"));
    if (const char* why = ray_view_check(&views[i], cam, &rv[i])) return fail(REVO_ERR_INVALID_ARG, at + why);
    const size_t np = (size_t)rv[i].w * rv[i].h;
    out_bytes += (np * per_pixel + 15) & ~(size_t)15;
    max_blocks = std::max(max_blocks, ((rv[i].w + 31) / 32) * ((rv[i].h + 7) / 8));
  }
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  const int nbx = tsdf_ray_blocks(box->n[0]), nby = tsdf_ray_blocks(box->n[1]), nbz = tsdf_ray_blocks(box->n[2]);
  const size_t mask_bytes = ((((size_t)nbx * nby * nbz + 31) / 32) * 4 + 255) & ~(size_t)255;
  const bool use_mask = env_int("REVO_MAP_TSDF_RAY_MASK", 1, 0, 1) != 0;
  // the scratch: the info line | the views' hits (64 words) | the mask
  const size_t off_hits = 64, off_mask = 512;
  TRY(m->tsdfraywork.reserve(off_mask + mask_bytes, s));
  TRY(m->tsdfray_views.reserve(n, s));
  TRY(m->tsdfrayout.reserve(device_out ? 0 : out_bytes, s));
  const size_t vol_bytes = sizeof(revo_map_tsdf_cell) * cells, col_bytes = sizeof(revo_map_tsdf_color) * cells;
  const bool with_color = color != nullptr;  // a given colour volume is read: for the colour images and for the uncolored counter
  TRY(m->tsdfvol.reserve(device_tsdf ? 0 : vol_bytes, s));
  if (with_color) TRY(m->tsdfcol.reserve(device_tsdf ? 0 : col_bytes, s));
  if (!device_tsdf) {
    HIPCHECK(hipMemcpyAsync(m->tsdfvol.p, tsdf, vol_bytes, hipMemcpyHostToDevice, s));
    if (with_color) HIPCHECK(hipMemcpyAsync(m->tsdfcol.p, color, col_bytes, hipMemcpyHostToDevice, s));
  }
  u64* d_info = device_out && info ? (u64*)info : (u64*)m->tsdfraywork.p;
  unsigned* d_hits = device_out && hits ? hits : (unsigned*)(m->tsdfraywork.p + off_hits);
  unsigned* d_mask = (unsigned*)(m->tsdfraywork.p + off_mask);
  size_t oo = 0;
  for (int i = 0; i < n; ++i) {
    TsdfRayView& d = m->tsdfray_views.h[i];
    d.v = rv[i];
    const size_t np = (size_t)rv[i].w * rv[i].h;
    if (device_out) {
      d.depth = depth[i]; d.normal = normal ? normal[i] : nullptr; d.bgr = bgr ? bgr[i] : nullptr;
    } else {  // depth, normals, colour: the widest first
      char* b = m->tsdfrayout.p + oo;
      d.depth = (float*)b;
      d.normal = normal ? (float*)(b + np * 4) : nullptr;
      d.bgr = bgr ? (uint8_t*)(b + np * (normal ? 16 : 4)) : nullptr;
      oo += (np * per_pixel + 15) & ~(size_t)15;
    }
    d.hits = d_hits + i;
  }
  TRY(m->tsdfray_views.upload(n, s));
  TsdfRayK a{};
  a.tsdf = device_tsdf ? tsdf : (const revo_map_tsdf_cell*)m->tsdfvol.p;
  a.color = !with_color ? nullptr : device_tsdf ? color : (const revo_map_tsdf_color*)m->tsdfcol.p;
  a.mask = use_mask ? d_mask : nullptr;
  a.box = *box;
  a.nby = nby; a.nbz = nbz;
  a.voxel = m->voxel; a.step = pp.step;
  a.min_weight = pp.min_weight; a.max_steps = pp.max_steps;
  HIPCHECK(hipMemsetAsync(d_info, 0, sizeof(revo_map_tsdf_ray_info), s));
  HIPCHECK(hipMemsetAsync(d_hits, 0, sizeof(unsigned) * n, s));
  if (use_mask) {
    HIPCHECK(hipMemsetAsync(d_mask, 0, mask_bytes, s));
    hipLaunchKernelGGL(k_tsdf_ray_mask, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, a.tsdf, *box, (unsigned)cells, pp.min_weight, nby, nbz,
                       d_mask);
    HIPCHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_tsdf_raycast, dim3((unsigned)max_blocks, (unsigned)n), dim3(256), 0, s, a, m->tsdfray_views.d, d_info);
  HIPCHECK(hipGetLastError());
  if (!device_out) {
    for (int i = 0; i < n; ++i) {
      const TsdfRayView& d = m->tsdfray_views.h[i];
      const size_t np = (size_t)rv[i].w * rv[i].h;
      HIPCHECK(hipMemcpyAsync(depth[i], d.depth, np * 4, hipMemcpyDeviceToHost, s));
      if (normal) HIPCHECK(hipMemcpyAsync(normal[i], d.normal, np * 12, hipMemcpyDeviceToHost, s));
      if (bgr) HIPCHECK(hipMemcpyAsync(bgr[i], d.bgr, np * 3, hipMemcpyDeviceToHost, s));
    }
    if (hits) HIPCHECK(hipMemcpyAsync(hits, d_hits, sizeof(unsigned) * n, hipMemcpyDeviceToHost, s));
    if (info) HIPCHECK(hipMemcpyAsync(info, d_info, sizeof(revo_map_tsdf_ray_info), hipMemcpyDeviceToHost, s));
  }
  if (!device_out || !device_tsdf) HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}
