// revo_batch.hip -- batches of frame pairs in device memory (revo_batch_*): build, deferred work, tracker grids, the
// information matrices' workspace (InfoWs), and the two measuring entry points.
#include "revo_host_impl.h"

// -------------------------------------------------------------------- batch --
static bool env_defer() {  // read when a batch is created: REVO_EDT_DEFER=0 or REVO_DEFER=0 defers nothing
  // (round 4: 87.1 k -> 95.6 k frames/s together with a stream of their own for the deferred kernels and four batches in
  // rotation; measured, not kept: the other levels, profiles/r04_ab_defer_levels.txt)
  return env_int("REVO_EDT_DEFER", 1, 0, 1) && env_int("REVO_DEFER", 2, 0, 3) != 0;
}
extern "C" int revo_batch_create(revo_ctx* c, int n_pairs, revo_batch** out) {
  if (!c || !out || n_pairs <= 0) return fail(REVO_ERR_INVALID_ARG, "bad argument");
  HIPCHECK(hipSetDevice(c->device));
  Partial<revo_batch> b(new revo_batch());  // a failure below frees the partial batch
  b->ctx.hold(c); b->n_pairs = n_pairs;
  { FrameSet* fs = nullptr; TRY(frameset_create(c, 2 * n_pairs, false, &fs)); b->fs.reset(fs); }
  TRY(b->stream.create());
  TRY(b->ev0.create(hipEventDefault)); TRY(b->ev1.create(hipEventDefault));
  TRY(b->descs.create());
  TRY(b->trk.create());
  b->fs->trk_mark = &b->trk;
  b->cluster = pick_cluster(c, n_pairs);
  b->defer = env_defer();
  TRY(b->d_mail.alloc(mail_bytes(n_pairs, b->cluster) / sizeof(unsigned long long)));
  HIPCHECK(hipMemset(b->d_mail, 0, mail_bytes(n_pairs, b->cluster)));
  for (int f = 0; f < 2 * n_pairs; ++f) b->views.push_back(revo_pyr{c, b->fs.get(), f, false, (f % 2) == 0, 0.0, false, false});
  TRY(b->descs.reserve(n_pairs, b->stream));
  TRY(b->h_flags.alloc(n_pairs));
  for (int i = 0; i < n_pairs; ++i) fill_desc(&b->descs.h[i], &b->views[2 * i], &b->views[2 * i + 1], nullptr, nullptr);
  HIPCHECK(hipStreamSynchronize(c->stream));  // frameset_create's memset
  HIPCHECK(hipStreamSynchronize(nullptr));    // the mailbox zeroing (NULL stream; the batch's streams are non-blocking)
  *out = b.release();
  return REVO_OK;
}
revo_batch::~revo_batch() {
  hipSetDevice(ctx->device);
  if (stream) hipStreamSynchronize(stream);
}
extern "C" void revo_batch_destroy(revo_batch* b) {
  if (b) HandleDelete()(b);
}

static int batch_wait_tracker(revo_batch* b, hipStream_t s) { return b->trk.wait_elsewhere(s); }
// A tracker grid on a stream other than the build's: ordered behind the build whatever was deferred (with
// REVO_DEFER=0 / REVO_EDT_DEFER=0 nothing is pending, so run_pending_edt orders nothing -- and the edge lists, counts and DT
// planes the grid reads are written by the build stream).  Cheap and idempotent.
static int batch_wait_build(revo_batch* b, hipStream_t s) {
  // (with work deferred to the first consumer, run_pending_edt does the ordering: it either runs that work on s behind the
  // "built" event or waits for the "prepared" event of whoever ran it -- no second barrier packet on the tracker's stream)
  return b->defer ? REVO_OK : b->fs->ready.wait_elsewhere(s);
}
static int batch_mark_tracker(revo_batch* b, hipStream_t s) { return b->trk.record(s); }

static int enqueue_batch_tail(revo_batch* b, hipStream_t s) {
  const PyrGeom& g = b->ctx->geom;
  if (b->defer) {
    // Work left to the batch's first consumer (run_pending_edt: the tracker launch on ITS stream, revo_batch_prepare on a
    // stream of the caller's choice, an accessor, revo_batch_sync) -- the build stream is the critical chain of the
    // pipelined step: the depth half of the pyramid and the edge lists of the current frames (they only depend on the edge maps
    // and nothing on the build stream reads them) and the keyframes' EDT.  The keyframe-role frames' depth half and edge lists
    // wait for an accessor or a single-pair call on an even view.  REVO_EDT_DEFER=0 / REVO_DEFER=0: nothing is deferred.
    std::lock_guard<std::mutex> lk(b->fs->edt_mu);
    b->fs->edt_pending = true; b->fs->edt_count = b->n_pairs;
    b->fs->ref_lists_pending = true;
    b->fs->edge_bytes_pending = true;  // (the build ended at the edge bitmaps: ensure_edge_bytes)
  } else {
    launch_tile_points(g, b->fs->p, b->fs->B, s);
    launch_keyframe(g, b->fs->p, 0, 2, b->n_pairs, s);
  }
  return REVO_OK;
}

// one of d_depth / d_depth_u16 (raw depth: alpha = 1 / scale, the conversion runs inside the first build kernel)
static int batch_build(revo_batch* b, const uint8_t* d_bgr, const float* d_depth, const uint16_t* d_depth_u16, float alpha,
                       void* stream, bool borrow) {
  HIPCHECK(hipSetDevice(b->ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : b->stream;
  // (Splitting the batch into slices of pairs on 2 / 4 streams was measured in both rounds: no gain in round 1,
  // and with the round-2 kernels the step goes from 0.64 ms to 0.73 / 0.84 ms next to a tracker -- the build
  // kernels are throughput-limited, smaller launches only add tails.)
  // (last_results stays: a caller that pipelines track_only(k) -> build(k) -> sync still gets the flag-8 check of launch k;
  // the result buffer must stay valid until revo_batch_sync or the next revo_batch_track_only)
  TRY(wait_edt_before_rebuild(b->fs.get(), s));  // the previous build's deferred EDT still reads these planes
  // ... and its tracker grid still reads lists, counts and DT planes (PairDesc).  A build that defers writes none of them: gray,
  // depth level 0, the Canny words, hist / hist_nz and the hysteresis scratch are all its kernels touch, and run_pending_edt
  // waits for the grid on the stream that does write them -- the build stream, the step's critical chain, does not
  if (!b->defer) TRY(batch_wait_tracker(b, s));
  // (Measured and not kept: the two halves of the batch as two concurrent kernel chains -- 78.4 k -> 70.5 k frames/s.)
  enqueue_build(b->ctx, b->fs.get(), d_bgr, d_depth, d_depth_u16, alpha, s, borrow, false, 0, -1, b->defer);
  TRY(enqueue_batch_tail(b, s));
  HIPCHECK(hipGetLastError());
  TRY(b->fs->mark_built(s));  // accessors / single-pair calls on the batch's views wait for this
  for (auto& v : b->views) { v.table_built = false; v.ref_list_built = false; }
  return REVO_OK;
}
static int batch_build_f32(revo_batch* b, const uint8_t* d_bgr, const float* d_depth, void* stream, bool borrow) {
  if (!b || !d_bgr || !d_depth) return fail(REVO_ERR_INVALID_ARG, "null argument");
  return batch_build(b, d_bgr, d_depth, nullptr, 0.f, stream, borrow);
}
extern "C" int revo_batch_build(revo_batch* b, const uint8_t* d_bgr, const float* d_depth, void* stream) {
  return batch_build_f32(b, d_bgr, d_depth, stream, false);
}
extern "C" int revo_batch_build_borrow(revo_batch* b, const uint8_t* d_bgr, const float* d_depth, void* stream) {
  return batch_build_f32(b, d_bgr, d_depth, stream, true);
}

static int batch_upload_init(revo_batch* b, const float* h_init_RT, hipStream_t s) {
  if (!h_init_RT && b->identity_uploaded) return REVO_OK;  // same descriptors as last time: no copy on the stream
  b->identity_uploaded = (h_init_RT == nullptr);
  // the previous upload reads the pinned rows asynchronously: let it finish before rewriting the poses
  TRY(b->descs.reserve(b->n_pairs, s));
  for (int i = 0; i < b->n_pairs; ++i) {
    PairDesc& d = b->descs.h[i];
    if (h_init_RT) { memcpy(d.R, h_init_RT + 12 * i, sizeof(float) * 9); memcpy(d.T, h_init_RT + 12 * i + 9, sizeof(float) * 3); }
    else { memset(d.R, 0, sizeof(d.R)); d.R[0] = d.R[4] = d.R[8] = 1.f; memset(d.T, 0, sizeof(d.T)); }
  }
  return b->descs.upload(b->n_pairs, s);
}

extern "C" int revo_batch_prepare(revo_batch* b, void* stream) {
  if (!b) return fail(REVO_ERR_INVALID_ARG, "null argument");
  HIPCHECK(hipSetDevice(b->ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : b->stream;
  return run_pending_edt(b->ctx, b->fs.get(), s);
}

extern "C" int revo_batch_track_only(revo_batch* b, const float* h_init_RT, revo_pair_result* d_results, void* stream) {
  if (!b || !d_results) return fail(REVO_ERR_INVALID_ARG, "null argument");
  HIPCHECK(hipSetDevice(b->ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : b->stream;
  // an earlier grid of this batch on another stream still reads the descriptors and the mailbox
  TRY(batch_wait_tracker(b, s));
  int rc = batch_upload_init(b, h_init_RT, s);
  if (rc) return rc;
  TrackParams tp = b->ctx->tp;
  tp.eval_only = 0;
  TRY(batch_wait_build(b, s));
  TRY(run_pending_edt(b->ctx, b->fs.get(), s));   // the work deferred to this launch
  b->last_results = d_results;
  rc = chained_track_launch(b->ctx->device, b->ctx->knobs.track_depth, s, [&](unsigned* d_resident) {
    // (live timing, ADVICE r05: the pair sits INSIDE the chain -- behind the waits for older grids, the pose upload and the
    // resident gate, directly around the grid)
    if (b->tev0) (void)hipEventRecord(b->tev0, s);
    const int n_wg = launch_track(b->descs.d, tp, d_results, nullptr, b->n_pairs, b->d_mail, &b->mail_epoch, b->cluster, d_resident, s);
    if (b->tev1) (void)hipEventRecord(b->tev1, s);
    b->tev0 = b->tev1 = nullptr;
    return n_wg;
  });
  if (rc) return rc;
  return batch_mark_tracker(b, s);
}
// the next revo_batch_track_only of this batch records ev0 / ev1 (hipEvent_t) directly around its grid
extern "C" void revo_batch_time_next_grid_(revo_batch* b, void* ev0, void* ev1) {
  if (b) { b->tev0 = (hipEvent_t)ev0; b->tev1 = (hipEvent_t)ev1; }
}

// Same as revo_batch_build for raw 16-bit depth (the reference's on-disk format): the conversion
// depth = raw * (float)(1/scale) of iowrapperRGBD.cpp:326-327 runs inside the first build kernel.
extern "C" int revo_batch_build_u16(revo_batch* b, const uint8_t* d_bgr, const uint16_t* d_depth_raw,
                                    double depth_scale_factor, void* stream) {
  if (!b || !d_bgr || !d_depth_raw) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!(depth_scale_factor > 0.0)) return fail(REVO_ERR_INVALID_ARG, "depth_scale_factor must be positive");
  return batch_build(b, d_bgr, nullptr, d_depth_raw, (float)(1.0f / depth_scale_factor), stream, false);
}

extern "C" int revo_batch_track(revo_batch* b, const uint8_t* d_bgr, const float* d_depth, const float* h_init_RT,
                                revo_pair_result* d_results, void* stream) {
  int rc = revo_batch_build(b, d_bgr, d_depth, stream);
  if (rc) return rc;
  return revo_batch_track_only(b, h_init_RT, d_results, stream);
}

extern "C" int revo_batch_sync(revo_batch* b, void* stream) {
  if (!b) return fail(REVO_ERR_INVALID_ARG, "null batch");
  HIPCHECK(hipSetDevice(b->ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : b->stream;
  HIPCHECK(hipStreamSynchronize(s));
  if (b->fs->edt_pending) { int rc2 = run_pending_edt(b->ctx, b->fs.get(), s); if (rc2) return rc2; HIPCHECK(hipStreamSynchronize(s)); }
  // A record with bit 3 carries no pose (its workgroups could not exchange partial sums: device shared with
  // another process): that is an error of the call, not something to find by decoding flags.
  if (b->last_results) {
    //  the grid that wrote these records may have run on ANOTHER stream than s: finish it before reading
    TRY(batch_wait_tracker(b, s));
    HIPCHECK(hipMemcpyAsync(b->h_flags, b->last_results, sizeof(revo_pair_result) * b->n_pairs, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    b->last_results = nullptr;  // decoded once: the caller may free or reuse that buffer after this call
    for (int i = 0; i < b->n_pairs; ++i)
      if (b->h_flags[i].flags & 8)
        return fail(REVO_ERR_HIP, "tracker: pair " + std::to_string(i) + ": the workgroups of the pair could not exchange "
                    "partial sums in time (device shared with another process?) -- its pose is not valid");
  }
  return REVO_OK;
}

// ------------------------------------------------- information matrices --
int infows_create(int n, bool own_out, std::unique_ptr<InfoWs>* out) {
  Partial<InfoWs> w(new InfoWs());
  w->n = n;
  TRY(w->descs.reserve(n, nullptr));
  TRY(w->rt.reserve(n, nullptr));
  TRY(w->d_part.alloc(INFO_PART_DOUBLES * INFO_MAX_GROUPS * (size_t)n));
  TRY(w->d_cnt.alloc(INFO_MAX_GROUPS * (size_t)n));
  TRY(w->d_ticket.alloc(align_up((size_t)n, 4)));
  if (own_out) {
    TRY(w->d_out.alloc(n));
    TRY(w->h_out.alloc(n));
  }
  TRY(w->rt.create());
  TRY(w->ev_done.create());
  out->reset(w.release());
  return REVO_OK;
}
InfoParams info_params(const TrackParams& tp, int lvl) {
  InfoParams ip;
  ip.fx = tp.cam[lvl].fx; ip.fy = tp.cam[lvl].fy; ip.cx = tp.cam[lvl].cx; ip.cy = tp.cam[lvl].cy;
  ip.w = tp.cam[lvl].w; ip.h = tp.cam[lvl].h;
  ip.edge_distance = tp.edge_distance[lvl]; ip.huber_edge = tp.huber_edge;
  ip.use_edge_filter = tp.use_edge_filter; ip.level = lvl;
  return ip;
}
int infows_upload_rt(InfoWs* w, int n, const float* h_RT, hipStream_t s) {
  TRY(w->rt.reserve(n, s));  // the previous upload has read the pinned rows
  for (int i = 0; i < n; ++i) {
    memcpy(w->rt.h[i].v, h_RT + 12 * i, sizeof(float) * 12);
    memset(w->rt.h[i].v + 12, 0, sizeof(float) * 4);
  }
  return w->rt.upload(n, s);
}

extern "C" int revo_batch_pair_info(revo_batch* b, const revo_pair_result* d_results, const float* h_RT, int lvl,
                                    revo_pair_info* d_info, void* stream) {
  if (!b || !d_info) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if ((d_results != nullptr) == (h_RT != nullptr)) return fail(REVO_ERR_INVALID_ARG, "exactly one of d_results and h_RT must be given");
  if ((uintptr_t)d_info % 16) return fail(REVO_ERR_INVALID_ARG, "d_info is not 16-byte aligned");
  revo_ctx* c = b->ctx;
  if (lvl < 0 || lvl >= c->geom.n_levels) return fail(REVO_ERR_LEVEL, "level out of range");
  HIPCHECK(hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : b->stream;
  if (!b->info_ws) {
    TRY(infows_create(b->n_pairs, false, &b->info_ws));
    // the plane pointers of a batch's descriptors never change (the poses in them are not read here)
    HIPCHECK(hipMemcpy(b->info_ws->descs.d, b->descs.h, sizeof(PairDesc) * b->n_pairs, hipMemcpyHostToDevice));
  }
  InfoWs* w = b->info_ws.get();
  TRY(batch_wait_tracker(b, s));   // the grid that wrote d_results, and an earlier launch on this workspace
  if (h_RT) TRY(infows_upload_rt(w, b->n_pairs, h_RT, s));
  TRY(batch_wait_build(b, s));
  TRY(run_pending_edt(c, b->fs.get(), s));  // what the tracker needs; never the even views' lazy work
  InfoParams ip;
  { std::lock_guard<std::mutex> lk(c->mu); ip = info_params(c->tp, lvl); }
  launch_pair_info(w->descs.d, h_RT ? (const void*)w->rt.d : (const void*)d_results, h_RT ? 16 : (int)(sizeof(revo_pair_result) / 4),
                   h_RT ? 12 : (int)(offsetof(revo_pair_result, flags) / 4), ip, b->n_pairs, w->d_part, w->d_cnt, w->d_ticket, d_info, s);
  HIPCHECK(hipGetLastError());
  return batch_mark_tracker(b, s);  // the batch's next build (and its next grid on another stream) waits for this launch too
}

// Every kernel of the batch build ALONE, HIP events between the launches on one stream, mean of `reps` passes: the per-kernel
// table of bench.py's roofline (VERDICT r04 #6b: the kernel furthest below its roofline must be visible in the driver's record).
// Every launch covers all B frames (the byte model of the driver's table is per 2 x pairs frames), so it leaves the batch built
// like revo_batch_build_borrow + revo_batch_prepare PLUS the keyframe-role frames' edge lists.
extern "C" int revo_batch_profile_build(revo_batch* b, const uint8_t* d_bgr, const float* d_depth, int reps, revo_stage_times* out) {
  if (!b || !d_bgr || !d_depth || !out || reps <= 0) return fail(REVO_ERR_INVALID_ARG, "bad argument");
  revo_ctx* c = b->ctx;
  HIPCHECK(hipSetDevice(c->device));
  hipStream_t s = b->stream;
  TRY(wait_edt_before_rebuild(b->fs.get(), s));
  TRY(batch_wait_tracker(b, s));
  memset(out, 0, sizeof(*out));
  PyrGeom g = c->geom;
  g.frame0 = 0;
  FrameSet* fs = b->fs.get();
  g.edge_bytes_lazy = b->defer ? 1 : 0;  // the kernels as the batch's own builds launch them
  fs->lazy_edge_bytes = b->defer;
  const int B = fs->B, L = g.n_levels;
  fs->p.depth[0] = const_cast<float*>(d_depth);
  struct Stage { const char* name; int a, w; };
  std::vector<Stage> st;
  // (the order a pipelined batch runs them in: the gray half of the pyramid, Canny, fill-in on the build stream; the depth half,
  // the edge lists and the keyframes' EDT on the first consumer's)
  st.push_back({"k_gray_depth", 0, 0});
  for (int l = 1; l < L; ++l) st.push_back({"k_pyrdown_gray", l, 1});
  st.push_back({"k_canny_nms4", 0, 0});
  st.push_back({"hysteresis", 0, 0});
  st.push_back({"k_fill", 0, 0});
  // (as a pipelined batch runs it: the depth half stages the edge pixels' depths when the knob is on)
  const bool stage = c->knobs.stage_edge_depths && fs->p.stage[0] != nullptr && L > 1;
  PyrGeom gp = g;
  gp.pts_staged = stage ? 1 : 0;
  if (stage) st.push_back({"k_edge_prefix", 0, 0});
  for (int l = 1; l < L; ++l) st.push_back({"k_pyrdown_depth", l, 2});
  st.push_back({"k_tile_count", 0, 1});
  st.push_back({"k_pts_tiles", 0, 2});
  st.push_back({"k_edt_cols", 0, 1});
  st.push_back({"k_edt_rows", 0, 2});
  const int n = (int)st.size();
  if (n > REVO_MAX_STAGES) return fail(REVO_ERR_CAPACITY, "too many stages");
  std::vector<OwnedEvent> ev(n + 1);  // destroyed on every exit path (a HIPCHECK inside the loop used to leak them)
  for (auto& e : ev) TRY(e.create(hipEventDefault));
  std::vector<double> sum(n, 0.0);
  for (int r = 0; r < reps; ++r) {
    HIPCHECK(hipEventRecord(ev[0], s));
    for (int i = 0; i < n; ++i) {
      const std::string nm = st[i].name;
      if (nm == "k_gray_depth") launch_gray_depth(g, fs->p, d_bgr, d_depth, nullptr, 0.f, B, s);
      else if (nm == "k_pyrdown_gray") launch_pyrdown(g, fs->p, st[i].a, B, s, 1);
      else if (nm == "k_pyrdown_depth") launch_pyrdown(g, fs->p, st[i].a, B, s, 2, stage);
      else if (nm == "k_edge_prefix") launch_edge_prefix(g, fs->p, B, s);
      else if (nm == "k_canny_nms4") launch_canny_nms(g, fs->p, B, s);
      else if (nm == "hysteresis") launch_hyst(g, fs->p, B, s);
      else if (nm == "k_fill") launch_fill(g, fs->p, B, s);
      else if (nm == "k_tile_count" || nm == "k_pts_tiles") launch_tile_points(gp, fs->p, B, s, st[i].w);
      else launch_keyframe(g, fs->p, 0, 2, b->n_pairs, s, st[i].w);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipEventRecord(ev[i + 1], s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
      float ms = 0.f;
      HIPCHECK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
      sum[i] += ms * 1e3;
    }
  }
  out->n = n;
  for (int i = 0; i < n; ++i) {
    out->us[i] = (float)(sum[i] / reps);
    if (std::string(st[i].name).rfind("k_pyrdown", 0) == 0) snprintf(out->name[i], sizeof(out->name[i]), "%s[%d]", st[i].name, st[i].a);
    else snprintf(out->name[i], sizeof(out->name[i]), "%s", st[i].name);
  }
  {  // the state a build + prepare leaves behind
    std::lock_guard<std::mutex> lk(fs->edt_mu);
    fs->edt_pending = false;
    fs->ref_lists_pending = false;  // (every kernel above ran over all B frames)
    fs->edge_bytes_pending = b->defer;
    TRY(fs->edt.record(s));
    fs->ref.recorded = false;       // `edt` covers the even frames' lists too
  }
  TRY(fs->mark_built(s));
  for (auto& v : b->views) { v.table_built = false; v.ref_list_built = false; }
  return REVO_OK;
}

extern "C" int revo_batch_frame(revo_batch* b, int frame, revo_pyr** out) {
  if (!b || !out || frame < 0 || frame >= 2 * b->n_pairs) return fail(REVO_ERR_INVALID_ARG, "bad frame index");
  *out = &b->views[frame];
  return REVO_OK;
}

extern "C" int revo_batch_time_tracker(revo_batch* b, const float* h_init_RT, revo_pair_result* d_results, void* stream,
                                       int reps, float* ms_mean) {
  if (!b || !d_results || !ms_mean || reps <= 0) return fail(REVO_ERR_INVALID_ARG, "bad argument");
  HIPCHECK(hipSetDevice(b->ctx->device));
  hipStream_t s = stream ? (hipStream_t)stream : b->stream;
  // an earlier grid of this batch on another stream still reads the descriptors and the mailbox
  TRY(batch_wait_tracker(b, s));
  int rc = batch_upload_init(b, h_init_RT, s);
  if (rc) return rc;
  TrackParams tp = b->ctx->tp;
  tp.eval_only = 0;
  TRY(batch_wait_build(b, s));
  TRY(run_pending_edt(b->ctx, b->fs.get(), s));
  float total = 0.f;
  for (int r = 0; r < reps; ++r) {  // events bracket exactly one kernel on its own stream
    HIPCHECK(hipEventRecord(b->ev0, s));
    rc = chained_track_launch(b->ctx->device, b->ctx->knobs.track_depth, s, [&](unsigned* d_resident) {
      return launch_track(b->descs.d, tp, d_results, nullptr, b->n_pairs, b->d_mail, &b->mail_epoch, b->cluster, d_resident, s);
    });
    if (rc) return rc;
    HIPCHECK(hipEventRecord(b->ev1, s));
    HIPCHECK(hipEventSynchronize(b->ev1));
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, b->ev0, b->ev1));
    total += ms;
  }
  *ms_mean = total / (float)reps;
  return batch_mark_tracker(b, s);
}
