// revo_frame.hip -- single-frame pyramids (revo_pyramid_*): creation out of the caller's rows on the build stream, the
// keyframe calls, the accessors, the coloured cloud, and what the voxel map asks of a pyramid (revo_map_source_*).
#include "revo_host_impl.h"

// The in-place upload of a frame (revo_pyramid_create*, rows in page-locked host memory) as a KERNEL (REVO_H2D_KERNEL=1; the default
// is hipMemcpyAsync): 16 bytes per lane straight out of the caller's rows over PCIe into the set's input plane; same bytes, same
// stream, same event.  Why it exists: about one hipMemcpyAsync in 36 000 does not RETURN for 6-13 ms (profiles/r06_slow_run_probe.txt,
// per-section maxima of 54 000 frame submissions: every other HIP call of a submission stayed below 1.3 ms; inside bench.py a
// build's kernel launches were seen to take 9 ms once as well).  The IO thread sits in
// that call, the queue of four pyramids runs dry, the consumer waits: THE slow run of the sequential stream's 60-frame measurement
// (one run in 15-25 at 60-80 % of the median in every round since the second; on a long stream it is 7 ms in ~4 s, 0.2 %).  With the
// kernel there is no such stall -- 0 slow runs in 900, the longest gap between two poses 1.0 ms -- but the median drops from
// 4.06-4.20 k to 3.55-3.87 k frames/s (the shader's reads over PCIe run next to the tracker and the build; on the build stream or on
// a high-priority stream it is the same): a latency-critical consumer can switch it on, throughput keeps the DMA engine.
typedef unsigned v4u __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) k_upload_rows(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, size_t src_stride,
                                                     size_t row_bytes, int rows) {
  // row_bytes is a multiple of 4 for every plane type at every width the library accepts only when w % 4 == 0: handled per byte tail
  const size_t vec = row_bytes / 16, tail0 = vec * 16;
  for (int y = blockIdx.y; y < rows; y += gridDim.y) {
    const uint8_t* s = src + (size_t)y * src_stride;
    uint8_t* d = dst + (size_t)y * row_bytes;
    const bool aligned = (((uintptr_t)s | (uintptr_t)d) & 15) == 0;
    if (aligned) {
      for (size_t i = blockIdx.x * blockDim.x + threadIdx.x; i < vec; i += (size_t)gridDim.x * blockDim.x)
        ((v4u*)d)[i] = __builtin_nontemporal_load((const v4u*)s + i);
      for (size_t i = tail0 + blockIdx.x * blockDim.x + threadIdx.x; i < row_bytes; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
    } else {
      for (size_t i = blockIdx.x * blockDim.x + threadIdx.x; i < row_bytes; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
    }
  }
}
static hipError_t upload_rows(void* dst, const void* src, size_t src_stride, size_t row_bytes, int rows, int max_blocks, hipStream_t s) {
  void* dsrc = nullptr;
  hipError_t e = hipHostGetDevicePointer(&dsrc, const_cast<void*>(src), 0);  // (registered memory: the device's view of it)
  if (e != hipSuccess) { (void)hipGetLastError(); return e; }
  if (src_stride == row_bytes) {  // one contiguous block: treat it as a single long row
    const size_t bytes = row_bytes * rows;
    const int blocks = (int)std::min<size_t>((size_t)max_blocks, (bytes / 16 + 255) / 256 + 1);
    hipLaunchKernelGGL(k_upload_rows, dim3(blocks, 1), dim3(256), 0, s, (uint8_t*)dst, (const uint8_t*)dsrc, bytes, bytes, 1);
  } else {
    hipLaunchKernelGGL(k_upload_rows, dim3(2, std::min(rows, 128)), dim3(256), 0, s, (uint8_t*)dst, (const uint8_t*)dsrc, src_stride, row_bytes, rows);
  }
  return hipGetLastError();
}
// (debug: the longest time each section of a frame submission has taken so far -- profiles/slow_run_probe.py prints them)
static std::atomic<unsigned long long> g_sec_max_ns[12];
extern "C" void revo_debug_section_max_(unsigned long long out[12], int reset) {
  for (int i = 0; i < 12; ++i) { out[i] = g_sec_max_ns[i].load(); if (reset) g_sec_max_ns[i].store(0); }
}
extern "C" void revo_debug_section_note_(int i, unsigned long long ns) {
  if (i < 0 || i >= 12) return;
  unsigned long long cur = g_sec_max_ns[i].load(std::memory_order_relaxed);
  while (ns > cur && !g_sec_max_ns[i].compare_exchange_weak(cur, ns)) {}
}
struct SecTimer {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void lap(int i) {
    const auto n = std::chrono::steady_clock::now();
    revo_debug_section_note_(i, (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(n - t).count());
    t = n;
  }
};

static int pyramid_create_common(revo_ctx* c, const uint8_t* bgr, size_t bgr_stride, const void* depth,
                                 size_t depth_stride, bool is_u16, double scale, double ts, revo_pyr** out) {
  if (!c || !bgr || !depth || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  HIPCHECK(hipSetDevice(c->device));
  const int w = c->geom.lv[0].w, h = c->geom.lv[0].h;
  if (bgr_stride < (size_t)w * 3 || depth_stride < (size_t)w * (is_u16 ? 2 : 4))
    return fail(REVO_ERR_INVALID_ARG, "stride smaller than a row");
  FrameSet* fs = nullptr;
  SecTimer sec;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->pool.empty()) { fs = c->pool.back(); c->pool.pop_back(); }
  }
  sec.lap(0);  // the context's lock + the pool
  if (!fs) {
    TRY(frameset_create(c, 1, true, &fs));
    std::lock_guard<std::mutex> lk(c->mu);
    c->framesets_created += 1;
  }
  // The reference clones its inputs (imgpyramidrgbd.cpp:51,54): the caller may reuse its buffers when this returns.
  // Everything after the clone is asynchronous on the build stream, so building frame N+1 overlaps tracking frame N exactly
  // like the reference's IO thread (iowrapperRGBD.cpp:279, system.cpp:96).
  //   * rows in PAGE-LOCKED host memory (hipHostMalloc / hipHostRegister / torch pin_memory -- what a decoder thread that owns
  //     its buffers uses): the DMA engine reads them in place on a copy stream (next to the previous frame's build kernels),
  //     and the call returns when that copy has finished -- the device-side plane IS the clone.  No host-side copy at all
  //     (round 4: the 2.1 MB memcpy into the staging area was 0.18 ms of the IO thread's 0.26 ms per frame).
  //   * pageable rows: copied into the set's pinned staging area first, as before.
  const size_t brow = (size_t)w * 3, drow = (size_t)w * (is_u16 ? 2 : 4);
  hipStream_t bs = c->build_stream;
  auto page_locked = [](const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
  };
  const bool direct = c->knobs.direct_h2d && page_locked(bgr) && page_locked(depth) &&
                      page_locked(bgr + (size_t)(h - 1) * bgr_stride + brow - 1) &&
                      page_locked((const char*)depth + (size_t)(h - 1) * depth_stride + drow - 1);
  sec.lap(1);  // pointer attributes (and a new frame set, if the pool was empty)
  if (direct) {
    {
      std::lock_guard<std::mutex> lk(c->mu);
      if (!c->frame_copy_stream) TRY(c->frame_copy_stream.create());
    }
    TRY(fs->h2d.create());
    hipStream_t cs = c->frame_copy_stream;
    TRY(fs->ready.wait(cs));            // the previous build out of this set's input planes is done
    TRY(fs->wait_previous_users(cs));   // ... and its last consumers (depth level 0 is read in place)
    sec.lap(6);  // the copy stream's waits for the set's previous users
    // (memory the device cannot address through hipHostGetDevicePointer goes the old way)
    if (c->knobs.h2d_kernel && upload_rows(fs->d_bgr, bgr, bgr_stride, brow, h, c->knobs.upload_blocks, cs) == hipSuccess) {}
    else if (bgr_stride == brow) HIPCHECK(hipMemcpyAsync(fs->d_bgr, bgr, brow * h, hipMemcpyHostToDevice, cs));
    else HIPCHECK(hipMemcpy2DAsync(fs->d_bgr, brow, bgr, bgr_stride, brow, h, hipMemcpyHostToDevice, cs));
    sec.lap(7);  // upload, colour
    if (c->knobs.h2d_kernel && upload_rows(fs->d_depth, depth, depth_stride, drow, h, c->knobs.upload_blocks, cs) == hipSuccess) {}
    else if (depth_stride == drow) HIPCHECK(hipMemcpyAsync(fs->d_depth, depth, drow * h, hipMemcpyHostToDevice, cs));
    else HIPCHECK(hipMemcpy2DAsync(fs->d_depth, drow, depth, depth_stride, drow, h, hipMemcpyHostToDevice, cs));
    sec.lap(8);  // upload, depth
    HIPCHECK(hipEventRecord(fs->h2d, cs));
    sec.lap(9);  // hipEventRecord
    HIPCHECK(hipStreamWaitEvent(bs, fs->h2d, 0));
    sec.lap(2);  // the build stream's wait for the copies
    // the clone exists: the caller's buffers are free again
    TRY(wait_event_polled(fs->h2d));
    sec.lap(3);  // waiting for them
  } else {
    TRY(fs->ready.sync());  // previous upload out of this staging is done
    for (int y = 0; y < h; ++y) memcpy(fs->h_bgr + (size_t)y * brow, bgr + (size_t)y * bgr_stride, brow);
    for (int y = 0; y < h; ++y) memcpy((char*)fs->h_depth.p + (size_t)y * drow, (const char*)depth + (size_t)y * depth_stride, drow);
    TRY(fs->wait_previous_users(bs));  // the last consumers of the recycled set are done
    HIPCHECK(hipMemcpyAsync(fs->d_bgr, fs->h_bgr, brow * h, hipMemcpyHostToDevice, bs));
    HIPCHECK(hipMemcpyAsync(fs->d_depth, fs->h_depth, drow * h, hipMemcpyHostToDevice, bs));
  }
  const float alpha = is_u16 ? (float)(1.0f / scale) : 0.0f;  // iowrapperRGBD.cpp:327
  // (the f32 staging plane is the set's own memory: level 0 reads it in place)
  enqueue_build(c, fs, fs->d_bgr, is_u16 ? nullptr : fs->d_depth, is_u16 ? (const uint16_t*)fs->d_depth : nullptr, alpha, bs, true);
  HIPCHECK(hipGetLastError());
  TRY(fs->mark_built(bs));
  sec.lap(4);  // enqueueing the build
  revo_pyr* p = new revo_pyr{c, fs, 0, true, false, ts, false, false};
  ctx_ref(c);
  *out = p;
  return REVO_OK;
}

extern "C" int revo_pyramid_create(revo_ctx* ctx, const uint8_t* bgr, size_t bgr_stride, const float* depth_m,
                                   size_t depth_stride, double timestamp, revo_pyr** out) {
  return pyramid_create_common(ctx, bgr, bgr_stride, depth_m, depth_stride, false, 1.0, timestamp, out);
}
extern "C" int revo_pyramid_create_u16(revo_ctx* ctx, const uint8_t* bgr, size_t bgr_stride, const uint16_t* depth_raw,
                                       size_t depth_stride, double depth_scale_factor, double timestamp, revo_pyr** out) {
  if (!(depth_scale_factor > 0)) return fail(REVO_ERR_INVALID_ARG, "depth_scale_factor must be > 0");
  return pyramid_create_common(ctx, bgr, bgr_stride, depth_raw, depth_stride, true, depth_scale_factor, timestamp, out);
}

extern "C" void revo_pyramid_destroy(revo_pyr* p) {
  if (!p) return;
  if (p->owns_fs) {
    hipSetDevice(p->ctx->device);
    std::lock_guard<std::mutex> lk(p->ctx->mu);
    p->fs->release_to(p->ctx->pool, p->ctx->stream, p->ctx->vote_stream);
  }
  revo_ctx* c = p->owns_fs ? p->ctx : nullptr;
  delete p;
  if (c) ctx_unref(c);
}

extern "C" int revo_pyramid_make_keyframe(revo_pyr* p) {
  if (!p) return fail(REVO_ERR_INVALID_ARG, "null pyramid");
  HIPCHECK(hipSetDevice(p->ctx->device));
  TRY(wait_ready(p->ctx, p));
  if (!p->dt_ready) launch_keyframe(geom_of_set(p->ctx, p->fs), p->fs->p, p->frame, 1, 1, p->ctx->stream);
  HIPCHECK(hipGetLastError());
  p->dt_ready = false;  // (a second makeKeyframe computes again, like the reference)
  p->is_kf = true;
  p->table_built = false;
  return REVO_OK;
}
// The distance transforms of a frame that is LIKELY to become the keyframe (revo_vo.hip: the previous vote was close to a change),
// enqueued while the vote that decides it is still running; revo_pyramid_make_keyframe then finds them in place.  The frame is
// not a keyframe until that call; if it never comes the planes are simply never read (single-frame pyramids only).
extern "C" int revo_pyramid_prepare_keyframe_(revo_pyr* p) {
  if (!p) return fail(REVO_ERR_INVALID_ARG, "null pyramid");
  if (!p->owns_fs || p->is_kf || p->dt_ready) return REVO_OK;
  HIPCHECK(hipSetDevice(p->ctx->device));
  TRY(wait_ready(p->ctx, p));
  launch_keyframe(geom_of_set(p->ctx, p->fs), p->fs->p, p->frame, 1, 1, p->ctx->stream);
  HIPCHECK(hipGetLastError());
  p->dt_ready = true;
  return REVO_OK;
}
extern "C" int revo_pyramid_is_keyframe(const revo_pyr* p) { return p && p->is_kf; }
extern "C" double revo_pyramid_timestamp(const revo_pyr* p) { return p ? p->ts : 0.0; }

extern "C" int revo_pyramid_read(revo_pyr* p, revo_plane what, int lvl, void* dst, size_t cap, size_t* count) {
  if (!p) return fail(REVO_ERR_INVALID_ARG, "null pyramid");
  revo_ctx* c = p->ctx;
  HIPCHECK(hipSetDevice(c->device));
  if (lvl < 0 || lvl >= c->geom.n_levels) return fail(REVO_ERR_LEVEL, "level out of range");
  const LevelGeom& v = c->geom.lv[lvl];
  const FramePlanes& P = p->fs->p;
  const size_t f = (size_t)p->frame;
  TRY(wait_ready(c, p));
  // the byte edge planes themselves, and the reference-ordered walk that reads them (k_compact_walk)
  if (what == REVO_PLANE_EDGES || what == REVO_PLANE_EDGES_ORIG || what == REVO_PLANE_EDGES3D) TRY(ensure_edge_bytes(c, p->fs, c->stream));
  HIPCHECK(hipStreamSynchronize(c->stream));
  const void* src = nullptr;
  size_t n = v.npix, esz = 1;
  switch (what) {
    case REVO_PLANE_GRAY: src = P.gray[lvl] + f * v.npix; break;
    case REVO_PLANE_DEPTH: src = P.depth[lvl] + f * v.npix; esz = 4; break;
    case REVO_PLANE_EDGES: src = P.edges[lvl] + f * v.npix; break;
    case REVO_PLANE_EDGES_ORIG:  // returnOrigEdges, imgpyramidrgbd.h:67-75
      src = (v.has_orig ? P.edges_orig[lvl] : P.edges[lvl]) + f * v.npix;  // no fill-in at this level: the clone equals edgesPyr
      break;
    case REVO_PLANE_DT:
      if (!p->is_kf) return fail(REVO_ERR_NOT_KEYFRAME, "distance transform not built: call makeKeyframe");
      src = P.dt[lvl] + f * v.npix; esz = 4; break;
    case REVO_PLANE_GRADTABLE:
      if (!p->is_kf) return fail(REVO_ERR_NOT_KEYFRAME, "optimizationStructure not built");
      if (!p->table_built) {  // lazily materialised: the tracker itself samples the DT plane
        launch_grad_table(c->geom, P, p->frame, 1, 1, c->stream);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(c->stream));
        p->table_built = true;
      }
      src = P.table[lvl] + f * v.npix; esz = 16; break;
    case REVO_PLANE_EDGES3D: {
      if (!p->ref_list_built) {  // the reference's column-major order (imgpyramidrgbd.cpp:199-226): materialised for the accessor
        PyrGeom g1 = c->geom;
        g1.frame0 = p->frame;
        launch_compact(g1, P, 1, c->stream);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipStreamSynchronize(c->stream));
        p->ref_list_built = true;
      }
      int np = 0;
      HIPCHECK(hipMemcpy(&np, P.npts + f * REVO_L + lvl, sizeof(int), hipMemcpyDeviceToHost));
      n = (size_t)np; src = P.pts[lvl] + f * v.npix; esz = 16; break;
    }
    case REVO_PLANE_EDGES3D_TILED: {
      int np = 0;
      HIPCHECK(hipMemcpy(&np, P.npts + f * REVO_L + lvl, sizeof(int), hipMemcpyDeviceToHost));
      n = (size_t)np; src = P.pts_trk[lvl] + f * v.npix; esz = 16; break;
    }
    case REVO_PLANE_HIST:
      if (v.patch <= 0) { n = 0; src = P.hist[lvl]; break; }
      n = (size_t)v.hist_w * v.hist_h; src = P.hist[lvl] + f * n; break;
    default: return fail(REVO_ERR_INVALID_ARG, "unknown plane");
  }
  if (count) *count = n;
  if (dst) {
    if (n * esz > cap) return fail(REVO_ERR_CAPACITY, "host buffer too small");
    if (n) HIPCHECK(hipMemcpy(dst, src, n * esz, hipMemcpyDeviceToHost));
  }
  return REVO_OK;
}

// ImgPyramidRGBD::generateColoredPcl(lvl, clrPcl, densePcl), imgpyramidrgbd.cpp:279-327.
extern "C" int revo_pyramid_colored_pcl(revo_pyr* p, int lvl, int dense, float* dst8, size_t cap_points, size_t* count) {
  if (!p) return fail(REVO_ERR_INVALID_ARG, "null pyramid");
  revo_ctx* c = p->ctx;
  HIPCHECK(hipSetDevice(c->device));
  if (lvl < 0 || lvl >= c->geom.n_levels) return fail(REVO_ERR_LEVEL, "level out of range");
  if (!(p->owns_fs || p->has_colour) || !p->fs->d_bgr)
    return fail(REVO_ERR_INVALID_ARG, "batch views keep no colour image (rgbFullSize): use revo_pyramid_create");
  TRY(wait_ready(c, p));
  TRY(ensure_edge_bytes(c, p->fs, c->stream));  // k_pcl_walk reads edges[lvl]
  std::lock_guard<std::mutex> lk(c->mu);
  const PyrGeom& g = c->geom;
  const size_t n0 = g.lv[0].npix, slots = (size_t)g.lv[0].w * g.lv[0].nchunk;
  if (!c->d_pcl) {
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_out = take(n0 * 32), o_a = take(n0 / 4 * 3 + 3), o_b = take(n0 / 16 * 3 + 3), o_ch = take(slots * 4),
                 o_m = take(slots * 4), o_t = take(4);
    TRY(c->d_pcl.alloc(off));
    c->d_pcl_out = (float*)(c->d_pcl + o_out);
    c->d_pcl_clr[0] = (uint8_t*)(c->d_pcl + o_a); c->d_pcl_clr[1] = (uint8_t*)(c->d_pcl + o_b);
    c->d_pcl_chunk = (int*)(c->d_pcl + o_ch); c->d_pcl_mask = (unsigned*)(c->d_pcl + o_m); c->d_pcl_total = (int*)(c->d_pcl + o_t);
  }
  hipStream_t s = c->stream;
  const uint8_t* clr = p->fs->d_bgr + (size_t)p->frame * n0 * 3;  // the full-resolution clone (imgpyramidrgbd.cpp:51), pyrDown'ed lvl times
  for (int l = 0; l < lvl; ++l) {
    uint8_t* d = c->d_pcl_clr[l & 1];
    launch_pyrdown_bgr(clr, g.lv[l].w, g.lv[l].h, d, s);
    clr = d;
  }
  const int cap = (int)std::min<size_t>(dst8 ? cap_points : 0, (size_t)g.lv[lvl].npix);
  launch_colored_pcl(g, p->fs->p, p->frame, lvl, dense ? 1 : 0, clr, c->d_pcl_chunk, c->d_pcl_mask, c->d_pcl_total,
                     dst8 ? cap : g.lv[lvl].npix, c->d_pcl_out, s);
  HIPCHECK(hipGetLastError());
  int total = 0;
  HIPCHECK(hipMemcpyAsync(&total, c->d_pcl_total, sizeof(int), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (count) *count = (size_t)total;
  if (dst8) {
    if ((size_t)total > cap_points) return fail(REVO_ERR_CAPACITY, "host buffer too small");
    if (total) HIPCHECK(hipMemcpy(dst8, c->d_pcl_out, (size_t)total * 32, hipMemcpyDeviceToHost));
  }
  return REVO_OK;
}

// The voxel map (revo_map.hip) reads level 0 of a keyframe and its colour on the context's tracker stream, behind the build
// (and any deferred work) of the pyramid, like revo_pyramid_colored_pcl.  A single-frame pyramid's set goes back to the pool
// behind free_trk, recorded on that stream (revo_pyramid_destroy); a revo_vo_multi keyframe slot is rewritten on it.
extern "C" int revo_map_source_(revo_pyr* p, MapSource* out) {
  if (!p || !out) return fail(REVO_ERR_INVALID_ARG, "null pyramid");
  revo_ctx* c = p->ctx;
  HIPCHECK(hipSetDevice(c->device));
  if (!(p->owns_fs || p->has_colour) || !p->fs->d_bgr)
    return fail(REVO_ERR_INVALID_ARG, "batch views keep no colour image (rgbFullSize): use revo_pyramid_create");
  TRY(wait_ready(c, p));
  TRY(ensure_edge_bytes(c, p->fs, c->stream));  // the cloud fuse reads edges[0]
  const size_t n0 = c->geom.lv[0].npix, f = (size_t)p->frame;
  out->ctx = c;
  out->depth = p->fs->p.depth[0] + f * n0;
  out->edges = p->fs->p.edges[0] + f * n0;
  out->bgr = p->fs->d_bgr + f * n0 * 3;
  return REVO_OK;
}
// What revo_map_carve asks of a pyramid before anything is enqueued: its context, and whether it is a batch view whose planes
// the map calls do not take (the rule of revo_map_source_).  Touches no stream.
extern "C" int revo_map_source_kind_(const revo_pyr* p, const revo_ctx** ctx, int* batch_view) {
  if (!p || !ctx || !batch_view) return fail(REVO_ERR_INVALID_ARG, "null pyramid");
  *ctx = p->ctx;
  *batch_view = (!(p->owns_fs || p->has_colour) || !p->fs->d_bgr) ? 1 : 0;
  return REVO_OK;
}
extern "C" int revo_map_ctx_geom_(const revo_ctx* c, MapCtxGeom* out) {
  if (!c || !out) return fail(REVO_ERR_INVALID_ARG, "null context");
  const LevelGeom& l = c->geom.lv[0];
  *out = MapCtxGeom{c->device, l.w, l.h, l.fx, l.fy, l.cx, l.cy, c->geom.depth_min, c->geom.depth_max, (void*)c->stream};
  return REVO_OK;
}
