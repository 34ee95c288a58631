// revo_mdev.hip -- the device half of revo_vo_multi (revo_multi.h).
#include "revo_host_impl.h"

// ------------------------------------------------- multi-stream VO (device) --
// The device half of revo_vo_multi (revo_vo_multi.hip runs the per-stream REVO::start logic on top of it).
//   * Step sets: one FrameSet of n_streams frames per submit (one batched build), pooled.  The host side releases a set once
//     none of its frames is queued, current or previous any more; its reuse is ordered by free_trk / free_vote like a
//     single-frame set's.
//   * Keyframes: ONE persistent set of n_streams frames, slot s = stream s.  Promotion copies the frame's planes out of its
//     step set and runs the EDT on the slot, so a keyframe never pins a step set (n_streams keyframes in n_streams different
//     step sets would otherwise hold n_streams^2 frames).
//   * Past clouds: per stream, owned here (never revo_ctx::past: a revo_vo on the same context keeps its own).
//   * Streams: the context's tracker stream (grids, promotions), build stream (uploads and builds) and vote stream (votes,
//     cloud copies).  No graph capture.
//   * Tracker settings: a snapshot of the context's, taken when the handle is created (a later revo_ctx_set_tracker does
//     not reach the handle, and the handle never changes the context's).
struct revo_mdev {  // ~revo_mdev waits for the context's three streams first; the members go in reverse order
  CtxRef c;
  int S = 0, cluster = 1, hl = 0;
  TrackParams tp;
  revo_tracker_settings ts;  // the context's tracker settings when the handle was created (with tp: one consistent snapshot)
  std::vector<revo_pyr> kf_views;
  std::vector<FrameSet*> pool, all;
  unsigned mail_epoch = 0;
  unsigned seq = 0;
  std::vector<std::deque<Past>> past;
  std::vector<Past> past_pool;
  size_t cloud_cap = 0;
  OwnedEvent ev_trk, ev_h2d, ev_prod;
  std::unique_ptr<InfoWs> info_ws;  // revo_mdev_pair_info_*, allocated on first use
  HostRows<CopySeg> segs;
  HostRows<CloudCopyDesc> cdesc;
  PinnedMem<int> h_vout;  // [S][16]
  DevMem<unsigned> d_done; DevMem<int> d_hist8; DevMem<int> d_marks;
  HostRows<VoteDesc> vdesc;
  DevMem<unsigned long long> d_mail;
  PinnedMem<revo_pair_result> h_res; DevMem<revo_pair_result> d_res;
  HostRows<PairDesc> descs;  // no event: the grid's poses are waited for before the rows are written again
  std::unique_ptr<FrameSet> kf;
  ~revo_mdev() {
    hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->build_stream);
    (void)hipStreamSynchronize(c->vote_stream);
    for (FrameSet* fs : all) delete fs;
    for (auto& q : past) for (auto& p : q) past_free(p);
    for (auto& p : past_pool) past_free(p);
  }
};

extern "C" void revo_mdev_destroy_(revo_mdev* m) {
  if (m) HandleDelete()(m);
}

extern "C" int revo_mdev_create_(revo_ctx* c, int S, revo_mdev** out) {
  if (!c || !out || S < 1) return fail(REVO_ERR_INVALID_ARG, "bad argument");
  HIPCHECK(hipSetDevice(c->device));
  const int hl = c->ts.histogram_level;
  if (hl < 0 || hl >= c->geom.n_levels) return fail(REVO_ERR_LEVEL, "histogram_level outside the pyramid");
  Partial<revo_mdev> m(new revo_mdev());
  m->c.hold(c); m->S = S; m->hl = hl;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    m->tp = c->tp;
    m->ts = c->ts;
  }
  m->tp.eval_only = 0;
  // Fixed for the handle's lifetime, as for a batch of n_streams pairs (REVO_TRACK_CLUSTER applies): every grid partitions a
  // pair's point lists the same way whatever else it carries, so a stream's poses do not depend on its neighbours.  (A larger
  // cluster -- the single-grid share, since the handle waits for each of its grids -- was tried: it moves the float sums of the
  // partition, and one 640x480 test sequence moved from within 5e-4 to 9e-4 per frame of the CPU restatement.  Not kept.)
  m->cluster = pick_cluster(c, S);
  { FrameSet* kf = nullptr; TRY(frameset_create(c, S, true, &kf, false)); m->kf.reset(kf); }
  for (int s = 0; s < S; ++s) {
    revo_pyr v{c, m->kf.get(), s, false, true, 0.0, false, false};
    v.has_colour = true;
    m->kf_views.push_back(v);
  }
  TRY(m->descs.reserve(S, nullptr));
  TRY(m->d_res.alloc(S));
  TRY(m->h_res.alloc(S));
  TRY(m->d_mail.alloc(mail_bytes(S, m->cluster) / sizeof(unsigned long long)));
  HIPCHECK(hipMemset(m->d_mail, 0, mail_bytes(S, m->cluster)));
  const size_t np = (size_t)c->geom.lv[hl].npix;
  m->cloud_cap = np;
  TRY(m->vdesc.reserve(S, nullptr));
  TRY(m->d_marks.alloc(np * S));
  TRY(m->d_hist8.alloc(8 * (size_t)S));
  TRY(m->d_done.alloc(S));
  HIPCHECK(hipMemset(m->d_marks, 0, sizeof(int) * np * S));  // the vote kernels leave their scratch clean: zero it once
  HIPCHECK(hipMemset(m->d_hist8, 0, sizeof(int) * 8 * S));
  HIPCHECK(hipMemset(m->d_done, 0, sizeof(unsigned) * S));
  TRY(m->h_vout.alloc(16 * (size_t)S));
  memset(m->h_vout, 0, sizeof(int) * 16 * S);
  TRY(m->cdesc.reserve(S, nullptr));
  for (OwnedEvent* e : {&m->ev_trk, &m->ev_h2d, &m->ev_prod}) TRY(e->create());
  TRY(m->vdesc.create()); TRY(m->cdesc.create()); TRY(m->segs.create());
  m->past.resize(S);
  HIPCHECK(hipDeviceSynchronize());  // the zeroing above runs on the NULL stream; the context's streams are non-blocking
  *out = m.release();
  return REVO_OK;
}

extern "C" int revo_mdev_submit_(revo_mdev* m, int n, const revo_stream_frame* fr, int is_u16, double scale, int device_src,
                                 void* producer, void** set_out) {
  revo_ctx* c = m->c;
  HIPCHECK(hipSetDevice(c->device));
  FrameSet* fs = nullptr;
  if (!m->pool.empty()) { fs = m->pool.back(); m->pool.pop_back(); }
  else {
    int rc = frameset_create(c, m->S, true, &fs, false);
    if (rc) return rc;
    m->all.push_back(fs);
  }
  // the uploads go on the build stream, in front of the build that reads them (no stream of their own)
  hipStream_t cs = c->build_stream, bs = c->build_stream;
  // the set's last consumers (tracker, vote) are done with its planes (its previous build is on this stream already)
  TRY(fs->wait_previous_users(cs));
  if (device_src) {  // the producer's writes of the frames come first
    HIPCHECK(hipEventRecord(m->ev_prod, (hipStream_t)producer));
    HIPCHECK(hipStreamWaitEvent(cs, m->ev_prod, 0));
  }
  const hipMemcpyKind kind = device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const int w = c->geom.lv[0].w, h = c->geom.lv[0].h;
  const size_t npix = (size_t)w * h, brow = (size_t)w * 3, drow = (size_t)w * (is_u16 ? 2 : 4);
  // frames whose rows lie back to back in the caller's memory (a decoder filling one slab per plane type) go in one copy
  RowCopier rc_{kind, h, cs, SIZE_MAX}, rd_{kind, h, cs, SIZE_MAX};  // (no cap on a run)
  for (int i = 0; i < n; ++i) {
    HIPCHECK(rc_.add(fs->d_bgr + (size_t)i * npix * 3, fr[i].bgr, fr[i].bgr_stride, brow));
    HIPCHECK(rd_.add((char*)fs->d_depth + (size_t)i * npix * (is_u16 ? 2 : 4), fr[i].depth, fr[i].depth_stride, drow));
  }
  HIPCHECK(rc_.flush());
  HIPCHECK(rd_.flush());
  HIPCHECK(hipEventRecord(m->ev_h2d, cs));
  const float alpha = is_u16 ? (float)(1.0f / scale) : 0.0f;  // iowrapperRGBD.cpp:327, fused into the first build kernel
  enqueue_build(c, fs, fs->d_bgr, is_u16 ? nullptr : fs->d_depth, is_u16 ? (const uint16_t*)fs->d_depth : nullptr, alpha, bs, true,
                true, 0, n);
  HIPCHECK(hipGetLastError());
  TRY(fs->mark_built(bs));
  // the caller's rows (host or device) are consumed once the copies are done; the build runs on
  HIPCHECK(hipEventSynchronize(m->ev_h2d));
  *set_out = fs;
  return REVO_OK;
}

extern "C" void revo_mdev_release_set_(revo_mdev* m, void* set) {
  FrameSet* fs = (FrameSet*)set;
  revo_ctx* c = m->c;
  hipSetDevice(c->device);
  fs->release_to(m->pool, c->stream, c->vote_stream);
}

extern "C" int revo_mdev_track_(revo_mdev* m, int n, MultiTrack* pairs) {
  if (n <= 0) return REVO_OK;
  revo_ctx* c = m->c;
  HIPCHECK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  FrameSet* waited[64];
  int nw = 0;
  for (int i = 0; i < n; ++i) {
    FrameSet* fs = (FrameSet*)pairs[i].set;
    const revo_pyr curr{c, fs, pairs[i].frame, false, false, 0.0, false, false};
    fill_desc(&m->descs.h[i], &m->kf_views[pairs[i].stream], &curr, pairs[i].R, pairs[i].T);
    bool seen = false;
    for (int k = 0; k < nw && !seen; ++k) seen = waited[k] == fs;
    if (!seen) {
      TRY(fs->ready.wait(s));
      if (nw < 64) waited[nw++] = fs;
    }
  }
  // the previous grid read d_descs on this stream: the copy queues behind it
  TRY(m->descs.upload(n, s, false));
  if (m->mail_epoch > 0xffffffffu - 4 * 8192u) {  // the whole mailbox, before launch_track's own wrap (sized for n pairs) comes due
    HIPCHECK(hipMemsetAsync(m->d_mail, 0, mail_bytes(m->S, m->cluster), s));
    m->mail_epoch = 0;
  }
  int rc = chained_track_launch(c->device, c->knobs.track_depth, s, [&](unsigned* d_resident) {
    return launch_track(m->descs.d, m->tp, m->d_res, nullptr, n, m->d_mail, &m->mail_epoch, m->cluster, d_resident, s);
  });
  if (rc) return rc;
  HIPCHECK(hipMemcpyAsync(m->h_res, m->d_res, sizeof(revo_pair_result) * n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipEventRecord(m->ev_trk, s));
  if ((rc = wait_event_polled(m->ev_trk))) return rc;
  for (int i = 0; i < n; ++i) {
    const revo_pair_result& r = m->h_res[i];
    if (r.flags & 8)
      return fail(REVO_ERR_HIP, "tracker: stream " + std::to_string(pairs[i].stream) + ": the workgroups of the pair could not exchange "
                  "partial sums in time (device shared with another process?) -- its pose is not valid");
    if ((rc = decode_track(r, pairs[i].R, pairs[i].T, nullptr, &pairs[i].status, nullptr, nullptr))) return rc;
  }
  return REVO_OK;
}

// The level-0 information of the n pairs revo_mdev_track_ just tracked, at the poses its grid wrote: one k_pair_info launch
// on the tracker stream behind that grid (descriptors and records are still the step's), copied to pinned memory.
extern "C" int revo_mdev_pair_info_enqueue_(revo_mdev* m, int n) {
  if (n <= 0) return REVO_OK;
  revo_ctx* c = m->c;
  HIPCHECK(hipSetDevice(c->device));
  if (!m->info_ws) TRY(infows_create(m->S, true, &m->info_ws));
  InfoWs* w = m->info_ws.get();
  hipStream_t s = c->stream;
  launch_pair_info(m->descs.d, m->d_res, (int)(sizeof(revo_pair_result) / 4), (int)(offsetof(revo_pair_result, flags) / 4),
                   info_params(m->tp, 0), n, w->d_part, w->d_cnt, w->d_ticket, w->d_out, s);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(w->h_out, w->d_out, sizeof(revo_pair_info) * n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipEventRecord(w->ev_done, s));
  return REVO_OK;
}
// waits for that launch; out: its n records, in the order of revo_mdev_track_'s pairs
extern "C" int revo_mdev_pair_info_wait_(revo_mdev* m, int n, revo_pair_info* out) {
  if (n <= 0) return REVO_OK;
  if (!m->info_ws) return fail(REVO_ERR_INVALID_ARG, "no information launch to wait for");
  const int rc = wait_event_polled(m->info_ws->ev_done);
  if (rc) return rc;
  memcpy(out, m->info_ws->h_out, sizeof(revo_pair_info) * n);
  return REVO_OK;
}

// assessTrackingQuality (tracker.cpp:118-201) for n streams: one mark and one count launch
extern "C" int revo_mdev_vote_(revo_mdev* m, int n, MultiVote* votes) {
  revo_ctx* c = m->c;
  HIPCHECK(hipSetDevice(c->device));
  const int nfh = m->ts.n_frames_hist_voting;
  hipStream_t vs = c->vote_stream;
  TRY(m->vdesc.reserve(m->S, vs));  // the previous upload of the descriptors has read them
  int nv = 0, idx[1024];
  const LevelGeom& lv = c->geom.lv[m->hl];
  const int use_orig = lv.has_orig;  // returnOrigEdges(lvl), imgpyramidrgbd.h:67-75
  for (int i = 0; i < n; ++i) {
    MultiVote& v = votes[i];
    v.status = REVO_TRACKER_STATE_OK;
    const std::deque<Past>& past = m->past[v.stream];
    if (past.empty() || !m->ts.check_tracking_results) continue;  // nothing to vote on (tracker.cpp:121)
    FrameSet* fs = (FrameSet*)v.set;
    TRY(fs->ready.wait_elsewhere(vs));
    TRY(ensure_edge_bytes(c, fs, vs));  // (these sets are built with their byte planes: the choke point of every byte reader)
    VoteDesc& d = m->vdesc.h[nv];
    memset(&d, 0, sizeof(d));
    float inv[16];
    mat4_inverse(v.T_w_curr, inv);
    int nframes = 0;
    for (int fr = 0; fr < nfh && fr < (int)past.size() && fr < 3; ++fr) {
      vote_cloud_pose(inv, past[fr], d.RT[fr]);
      d.pts[fr] = past[fr].d_pts;
      d.n[fr] = past[fr].d_n;
      ++nframes;
    }
    d.n_clouds = nframes;
    const size_t f = (size_t)v.frame * lv.npix;
    d.edges = (use_orig ? fs->p.edges_orig[m->hl] : fs->p.edges[m->hl]) + f;
    d.depth = fs->p.depth[m->hl] + f;
    d.marks = m->d_marks + (size_t)v.stream * m->cloud_cap;
    d.hist8 = m->d_hist8 + 8 * v.stream;
    d.done = m->d_done + v.stream;
    d.host_out = m->h_vout + 16 * v.stream;
    idx[nv++] = i;
  }
  if (!nv) return REVO_OK;
  const unsigned seq = ++m->seq ? m->seq : ++m->seq;
  TRY(m->vdesc.upload(nv, vs));
  launch_vote_multi(c->geom, m->hl, nv, m->vdesc.d, seq, vs);
  HIPCHECK(hipGetLastError());
  for (int k = 0; k < nv; ++k) {
    MultiVote& v = votes[idx[k]];
    const int* o = m->h_vout + 16 * v.stream;
    { int rc = wait_seq(vs, (volatile unsigned*)(o + 8), seq); if (rc) return rc; }
    v.status = vote_decide(o + 4, m->vdesc.h[k].n_clouds, nullptr);
  }
  return REVO_OK;
}

// mPastPcl.push_back (tracker.cpp:209-223) for n streams, one copy launch.  Only 3 + N_FRAMES_HIST_VOTING clouds of a stream
// can ever matter: the vote reads the OLDEST min(N, 3) (tracker.cpp:138) and a keyframe change keeps the NEWEST N
// (tracker.cpp:248-257).  Beyond that the fourth-oldest is neither and goes back to the pool (the reference keeps it).
extern "C" int revo_mdev_add_clouds_(revo_mdev* m, int n, const MultiFrame* f) {
  if (n <= 0) return REVO_OK;
  revo_ctx* c = m->c;
  HIPCHECK(hipSetDevice(c->device));
  hipStream_t vs = c->vote_stream;
  TRY(m->cdesc.reserve(n, vs));  // the previous upload of the descriptors has read them
  const size_t keep = 3 + (size_t)std::max(0, m->ts.n_frames_hist_voting);
  for (int i = 0; i < n; ++i) {
    FrameSet* fs = (FrameSet*)f[i].set;
    TRY(fs->ready.wait_elsewhere(vs));
    Past p{};
    TRY(past_take(m->past_pool, m->cloud_cap, m->cloud_cap, &p, true));
    const size_t fr = (size_t)f[i].frame;
    m->cdesc.h[i] = CloudCopyDesc{p.d_pts, fs->p.pts_trk[m->hl] + fr * m->cloud_cap, p.d_n, fs->p.npts + fr * REVO_L + m->hl};
    p.n = -1;
    memcpy(p.T_w, f[i].T_w, sizeof(float) * 16);
    p.ts = f[i].ts;
    std::deque<Past>& q = m->past[f[i].stream];
    q.push_back(p);
    // (stream-ordered reuse: the next copy into a recycled buffer runs on the vote stream behind every vote that read it)
    if (q.size() > keep) { m->past_pool.push_back(q[3]); q.erase(q.begin() + 3); }
  }
  TRY(m->cdesc.upload(n, vs));
  launch_copy_cloud_multi(n, m->cdesc.d, vs);
  HIPCHECK(hipGetLastError());
  return REVO_OK;
}

// keep < 0: N_FRAMES_HIST_VOTING (clearPastLists, tracker.cpp:248-257); 0: a reset
extern "C" void revo_mdev_clear_past_(revo_mdev* m, int stream, int keep) {
  if (keep < 0) keep = m->ts.n_frames_hist_voting;
  std::deque<Past>& q = m->past[stream];
  while ((int)q.size() > std::max(0, keep)) { m->past_pool.push_back(q.front()); q.pop_front(); }
}

// kfPyr = prevPyr; kfPyr->makeKeyframe() (system.cpp:205-215) for n streams: the frames' planes into the streams' keyframe
// slots (one copy launch), then the distance transforms of each slot
extern "C" int revo_mdev_promote_(revo_mdev* m, int n, const MultiFrame* f) {
  if (n <= 0) return REVO_OK;
  revo_ctx* c = m->c;
  HIPCHECK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const PyrGeom& g = c->geom;
  std::vector<CopySeg> segs;
  for (int i = 0; i < n; ++i) {
    FrameSet* src = (FrameSet*)f[i].set;
    TRY(src->ready.wait_elsewhere(s));
    TRY(ensure_edge_bytes(c, src, s));  // the copies below take edges / edges_orig (these sets are built with them)
    const size_t sf = (size_t)f[i].frame, df = (size_t)f[i].stream;
    const FramePlanes& a = src->p;
    const FramePlanes& b = m->kf->p;
    auto add = [&](const void* sp, void* dp, size_t per_frame) {
      if (per_frame) segs.push_back(CopySeg{(const char*)sp + sf * per_frame, (char*)dp + df * per_frame, per_frame});
    };
    for (int l = 0; l < g.n_levels; ++l) {
      const LevelGeom& v = g.lv[l];
      const size_t np = (size_t)v.npix, words = (size_t)v.h * v.wpr, cols = (size_t)v.w * v.nchunk;
      add(a.gray[l], b.gray[l], np);
      add(a.depth[l], b.depth[l], np * 4);
      add(a.cs[l], b.cs[l], words * 8);
      add(a.edges[l], b.edges[l], np);
      add(a.edges_orig[l], b.edges_orig[l], np);
      add(a.pts_trk[l], b.pts_trk[l], np * 16);
      if (v.patch > 0) add(a.hist[l], b.hist[l], (size_t)v.hist_w * v.hist_h);
      add(a.chunk[l], b.chunk[l], cols * 4);
      add(a.cmask[l], b.cmask[l], cols * 4);
      if (l < g.n_levels - 1) add(a.vb[l], b.vb[l], np / 8);
    }
    add(a.npts, b.npts, sizeof(int) * REVO_L);
    add(a.hist_nz, b.hist_nz, sizeof(int) * REVO_L);
    add(a.strip_tot, b.strip_tot, sizeof(int) * (size_t)g.total_strips);
    add(a.tile_base, b.tile_base, sizeof(int) * (size_t)g.total_tiles);
    add(src->d_bgr, m->kf->d_bgr, (size_t)g.lv[0].npix * 3);  // rgbFullSize (the coloured cloud)
  }
  TRY(m->segs.reserve((int)segs.size(), s));
  memcpy(m->segs.h, segs.data(), sizeof(CopySeg) * segs.size());
  TRY(m->segs.upload((int)segs.size(), s));
  launch_copy_segments((int)segs.size(), m->segs.d, s);
  for (int i = 0; i < n; ++i) {
    launch_keyframe(g, m->kf->p, f[i].stream, 1, 1, s);
    revo_pyr& v = m->kf_views[f[i].stream];
    v.ts = f[i].ts; v.table_built = false; v.ref_list_built = false;
  }
  HIPCHECK(hipGetLastError());
  return REVO_OK;
}

extern "C" revo_pyr* revo_mdev_keyframe_(revo_mdev* m, int stream) { return &m->kf_views[stream]; }
