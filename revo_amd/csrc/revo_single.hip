// revo_single.hip -- the single-pair tracker on the context's tracker stream (revo_optimizer_*, revo_tracker_track_frames and
// the split calls of the VO driver's look-ahead), the quality vote, the past clouds, revo_tracker_pair_info.
#include "revo_host_impl.h"

// The vote stream's work on a pyramid `p` is enqueued.  A single-frame pyramid's planes are recycled behind free_vote
// (revo_pyramid_destroy); a batch view's planes belong to the caller, whose ordering promises are all about the tracker
// stream -- so that stream waits here (batch views are not what the sequential loop runs on).
static int vote_enqueued(revo_ctx* c, const revo_pyr* p) {
  if (p->owns_fs) return REVO_OK;
  HIPCHECK(hipEventRecord(c->ev_vote, c->vote_stream));
  HIPCHECK(hipStreamWaitEvent(c->stream, c->ev_vote, 0));
  return REVO_OK;
}

// One single-pair tracker launch into result slot `slot` (0 / 1: the VO driver's look-ahead, 2: the public single-pair
// calls, which may run on a context whose VO driver keeps a speculative launch outstanding); *seq_out identifies it for track_wait.
static int track_launch(revo_ctx* c, const revo_pyr* ref, const revo_pyr* curr, const float* R, const float* T,
                        const TrackParams& tp, int slot, unsigned* seq_out) {
  fill_desc(c->h_desc, ref, curr, R, T);
  TRY(wait_ready(c, ref)); TRY(wait_ready(c, curr));
  TrackParams tp1 = tp;
  tp1.redundant_n = c->knobs.redundant_one;
  // a single pair has the chip to itself: one more retry next to the candidate at the two finest levels costs its 16 workgroups
  // little and saves passes (sequential stream 4.23 -> 4.29 k frames/s, profiles/r06_single_stream_sweep.txt).  REVO_TRACK_KSPEC_ONE:
  // one digit per level (finest first) or one for all; an explicit REVO_TRACK_KSPEC applies to single pairs too.
  if (c->knobs.kspec_one_set)
    for (int i = 0; i < REVO_L; ++i) tp1.kspec[i] = c->knobs.kspec_one[i];
  const unsigned seq = c->seq_next++;
  if (c->seq_next == 0) c->seq_next = 1;
  const int rc = chained_track_launch(c->device, c->knobs.track_depth, c->stream, [&](unsigned* d_resident) {
    return launch_track_one(*c->h_desc, tp1, c->h_res + slot, c->h_eval, c->d_mail, &c->mail_epoch, pick_cluster(c, 1), c->h_seq + slot,
                            seq, d_resident, c->stream);
  });
  if (rc) return rc;
  *seq_out = seq;
  return REVO_OK;
}
static int track_wait(revo_ctx* c, int slot, unsigned seq) { return wait_seq(c->stream, c->h_seq + slot, seq); }

enum { SINGLE_SLOT = 2 };
static int run_single(revo_ctx* c, const revo_pyr* ref, const revo_pyr* curr, const float* R, const float* T,
                      const TrackParams& tp) {
  unsigned seq = 0;
  int rc = track_launch(c, ref, curr, R, T, tp, SINGLE_SLOT, &seq);
  if (rc) return rc;
  if (tp.eval_only) {  // the EvalOut record is written by many lanes: wait for the stream, not for a word
    HIPCHECK(hipStreamSynchronize(c->stream));
    return REVO_OK;
  }
  return track_wait(c, SINGLE_SLOT, seq);
}

int decode_track(const revo_pair_result& r, float R[9], float T[3], float* err, int* status, revo_residual_info* info,
                        int32_t* iters) {
  if (r.flags & 2) return fail(REVO_ERR_NOT_ORTHOGONAL, "R is not orthogonal (Sophus::SO3 precondition)");
  if (r.flags & 8) return fail(REVO_ERR_HIP, "tracker: the workgroups of the pair could not exchange partial sums in time (device shared?)");
  memcpy(R, r.R, sizeof(float) * 9); memcpy(T, r.T, sizeof(float) * 3);
  if (err) *err = r.err;
  if (status) *status = r.status;
  if (info) { info->good_pts_edges = r.good; info->bad_pts_edges = r.bad; info->sum_error_unweighted = 0.f; info->sum_error_weighted = 0.f; }
  if (iters) memcpy(iters, r.evals, sizeof(int32_t) * REVO_L);
  return REVO_OK;
}

// ---- split calls for the VO driver's look-ahead (revo_vo.hip); not part of the public ABI
extern "C" int revo_track_launch_(revo_ctx* c, const revo_pyr* ref, const revo_pyr* curr, const float R[9], const float T[3], int slot,
                                  unsigned* seq_out) {
  int rc = check_pair(c, ref, curr);
  if (rc) return rc;
  HIPCHECK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  TrackParams tp = c->tp;
  tp.eval_only = 0;
  return track_launch(c, ref, curr, R, T, tp, slot & 1, seq_out);
}
extern "C" int revo_track_wait_(revo_ctx* c, int slot, unsigned seq, float R[9], float T[3], float* err, int* status) {
  if (!c) return fail(REVO_ERR_INVALID_ARG, "null context");
  int rc = track_wait(c, slot & 1, seq);
  if (rc) return rc;
  return decode_track(c->h_res[slot & 1], R, T, err, status, nullptr, nullptr);
}

extern "C" int revo_optimizer_track_level(revo_ctx* c, const revo_pyr* ref, const revo_pyr* curr, float R[9], float T[3],
                                          int lvl, revo_residual_info* info, float* err) {
  int rc = check_pair(c, ref, curr);
  if (rc) return rc;
  if (!R || !T) return fail(REVO_ERR_INVALID_ARG, "null pose");
  if (lvl < 0 || lvl >= c->geom.n_levels) return fail(REVO_ERR_LEVEL, "level out of range");
  HIPCHECK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  TrackParams tp = c->tp;
  tp.lvl_begin = tp.lvl_end = lvl; tp.check_init = 0; tp.eval_only = 0;
  rc = run_single(c, ref, curr, R, T, tp);
  if (rc) return rc;
  return decode_track(c->h_res[SINGLE_SLOT], R, T, err, nullptr, info, nullptr);
}

extern "C" int revo_optimizer_eval(revo_ctx* c, const revo_pyr* ref, const revo_pyr* curr, const float R[9],
                                   const float T[3], int lvl, revo_residual_info* info, float* err, float A[36],
                                   float b[6]) {
  int rc = check_pair(c, ref, curr);
  if (rc) return rc;
  if (!R || !T) return fail(REVO_ERR_INVALID_ARG, "null pose");
  if (lvl < 0 || lvl >= c->geom.n_levels) return fail(REVO_ERR_LEVEL, "level out of range");
  HIPCHECK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  TrackParams tp = c->tp;
  tp.lvl_begin = tp.lvl_end = lvl; tp.check_init = 0; tp.eval_only = 1;
  rc = run_single(c, ref, curr, R, T, tp);
  if (rc) return rc;
  const EvalOut& e = *c->h_eval;
  if (info) { info->good_pts_edges = e.good; info->bad_pts_edges = e.bad; info->sum_error_unweighted = e.sum_u; info->sum_error_weighted = e.sum_w; }
  if (err) *err = e.mean_err;
  if (A) memcpy(A, e.A, sizeof(float) * 36);
  if (b) memcpy(b, e.b, sizeof(float) * 6);
  return REVO_OK;
}

// inc = A.ldlt().solve(b) with A(i,i) *= 1 + lambda (optimizer.cpp:258-262) for n systems, on the device
extern "C" int revo_optimizer_solve6(revo_ctx* c, int n, const float* A36_b6_lambda, float* x6) {
  if (!c || !A36_b6_lambda || !x6 || n <= 0) return fail(REVO_ERR_INVALID_ARG, "bad argument");
  HIPCHECK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  DevMem<float> in, out;  // freed on every path
  float *&d_in = in.p, *&d_out = out.p;
  HIPCHECK(hipMalloc((void**)&d_in, sizeof(float) * 43 * (size_t)n));
  hipError_t e = hipMalloc((void**)&d_out, sizeof(float) * 6 * (size_t)n);
  if (e == hipSuccess) e = hipMemcpyAsync(d_in, A36_b6_lambda, sizeof(float) * 43 * (size_t)n, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) { launch_solve6(d_in, n, d_out, c->stream); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipMemcpyAsync(x6, d_out, sizeof(float) * 6 * (size_t)n, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(REVO_ERR_HIP, std::string("revo_optimizer_solve6: ") + hipGetErrorString(e));
  return REVO_OK;
}

// profile builds (-DREVO_TRACK_PROFILE): the phase cycle counters the last single-pair launch left in the EvalOut record
extern "C" int revo_debug_track_profile_(revo_ctx* c, float out13[13]) {
  if (!c || !out13) return REVO_ERR_INVALID_ARG;
  memcpy(out13, c->h_eval->A, sizeof(float) * 13);
  return REVO_OK;
}

extern "C" int revo_tracker_track_frames(revo_ctx* c, const revo_pyr* ref, const revo_pyr* curr, float R[9], float T[3],
                                         float* err, int* status, revo_residual_info* info, int32_t iters[REVO_MAX_LEVELS]) {
  int rc = check_pair(c, ref, curr);
  if (rc) return rc;
  if (!R || !T) return fail(REVO_ERR_INVALID_ARG, "null pose");
  HIPCHECK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  TrackParams tp = c->tp;
  tp.eval_only = 0;
  rc = run_single(c, ref, curr, R, T, tp);
  if (rc) return rc;
  return decode_track(c->h_res[SINGLE_SLOT], R, T, err, status, info, iters);
}

// assessTrackingQuality (tracker.cpp:118-201) in two halves: enqueue the vote kernels / read the counts
static int assess_launch(revo_ctx* c, const float T_w_curr[16], const revo_pyr* curr, int* nframes_out, unsigned* seq_out) {
  *nframes_out = -1;  // -1: nothing to vote on (tracker.cpp:121)
  if (c->past.empty() || !c->ts.check_tracking_results) return REVO_OK;
  const int hl = c->ts.histogram_level;
  if (hl < 0 || hl >= c->geom.n_levels) return fail(REVO_ERR_LEVEL, "histogram_level outside the pyramid");
  hipStream_t vs = c->vote_stream;
  TRY(wait_ready_on(c, curr, vs));
  TRY(ensure_edge_bytes(c, curr->fs, vs));  // k_vote_hist reads edges / edges_orig of the histogram level
  float inv[16];
  mat4_inverse(T_w_curr, inv);
  int nframes = 0;
  VoteArgs va{};
  for (int fr = 0; fr < c->ts.n_frames_hist_voting && fr < (int)c->past.size() && fr < 3; ++fr) {
    vote_cloud_pose(inv, c->past[fr], va.RT[fr]);
    va.pts[fr] = c->past[fr].d_pts;
    va.n[fr] = c->past[fr].d_n;
    ++nframes;
  }
  const int use_orig = c->geom.lv[hl].has_orig;  // returnOrigEdges(lvl), imgpyramidrgbd.h:67-75 (elsewhere the clone equals edgesPyr)
  const unsigned seq = c->seq_next++;
  if (c->seq_next == 0) c->seq_next = 1;
  launch_vote(c->geom, curr->fs->p, curr->frame, hl, nframes, va, c->d_marks, c->d_hist8, c->d_vote_done, c->h_hist8, seq,
              use_orig, vs);
  HIPCHECK(hipGetLastError());
  TRY(vote_enqueued(c, curr));
  *nframes_out = nframes;
  *seq_out = seq;
  return REVO_OK;
}
// ratio_out (may be null): vote_decide's, +inf if nothing voted
static int assess_wait(revo_ctx* c, int nframes, unsigned seq, int* status, int32_t hist4[4], int32_t overlaps4[4], float* ratio_out) {
  if (status) *status = REVO_TRACKER_STATE_OK;
  if (ratio_out) *ratio_out = INFINITY;
  if (nframes < 0) return REVO_OK;
  hipStream_t vs = c->vote_stream;  // where assess_launch enqueued the vote
  TRY(wait_seq(vs, (volatile unsigned*)(c->h_hist8 + 8), seq));
  const int* hist = c->h_hist8;
  const int* ov = c->h_hist8 + 4;
  if (hist4) memcpy(hist4, hist, sizeof(int32_t) * 4);
  if (overlaps4) memcpy(overlaps4, ov, sizeof(int32_t) * 4);
  const int st = vote_decide(ov, nframes, ratio_out);
  if (status) *status = st;
  return REVO_OK;
}

extern "C" int revo_tracker_assess_quality(revo_ctx* c, const float T_w_curr[16], const revo_pyr* curr, int* status,
                                           int32_t hist4[4], int32_t overlaps4[4]) {
  if (!c || !T_w_curr || !curr) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (curr->ctx != c) return fail(REVO_ERR_INVALID_ARG, "pyramid belongs to another context");
  if (hist4) memset(hist4, 0, sizeof(int32_t) * 4);
  if (overlaps4) memset(overlaps4, 0, sizeof(int32_t) * 4);
  if (status) *status = REVO_TRACKER_STATE_OK;
  HIPCHECK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  int nframes = -1;
  unsigned seq = 0;
  int rc = assess_launch(c, T_w_curr, curr, &nframes, &seq);
  if (rc) return rc;
  return assess_wait(c, nframes, seq, status, hist4, overlaps4, nullptr);
}
// split form for the VO driver's look-ahead (revo_vo.hip); not part of the public ABI
extern "C" int revo_assess_launch_(revo_ctx* c, const float T_w_curr[16], const revo_pyr* curr, int* nframes_out, unsigned* seq_out) {
  if (!c || !T_w_curr || !curr || curr->ctx != c) return fail(REVO_ERR_INVALID_ARG, "bad argument");
  HIPCHECK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  return assess_launch(c, T_w_curr, curr, nframes_out, seq_out);
}
// ratio_out (may be null): overlapMeasure / overlaps[0] of this vote -- how far the frame is from asking for a new keyframe (< 1 does,
// tracker.cpp:184); +inf while fewer than three past clouds vote (the answer is OK whatever the numbers) or nothing voted
extern "C" int revo_assess_wait_(revo_ctx* c, int nframes, unsigned seq, int* status, float* ratio_out) {
  if (!c) return fail(REVO_ERR_INVALID_ARG, "null context");
  return assess_wait(c, nframes, seq, status, nullptr, nullptr, ratio_out);
}

// (revo_host_impl.h) the context's callers size a buffer for what is stored -- the histogram level's cloud, not level 0's
int past_take(std::vector<Past>& pool, size_t need, size_t cap, Past* out, bool newest) {
  for (size_t i = 0; i < pool.size(); ++i) {
    const size_t k = newest ? pool.size() - 1 - i : i;
    if (pool[k].cap >= need) { *out = pool[k]; pool.erase(pool.begin() + k); return REVO_OK; }
  }
  Past p{};
  p.cap = cap;
  HIPCHECK(hipMalloc((void**)&p.d_pts, sizeof(float4) * p.cap));
  hipError_t e = hipMalloc((void**)&p.d_n, sizeof(int));
  if (e != hipSuccess) { past_free(p); return fail(REVO_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e)); }
  *out = p;
  return REVO_OK;
}
void past_free(Past& p) { (void)hipFree(p.d_pts); (void)hipFree(p.d_n); }

extern "C" int revo_tracker_add_old_pcl(revo_ctx* c, const revo_pyr* src, int lvl, const float T_w[16], double ts) {
  if (!c || !src || !T_w) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (lvl < 0 || lvl >= c->geom.n_levels) return fail(REVO_ERR_LEVEL, "level out of range");
  HIPCHECK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  // the reference copies the Eigen matrix (tracker.cpp:219); the copy stays in HBM, in a
  // recycled buffer sized for the level
  hipStream_t vs = c->vote_stream;  // the votes that read the copy run there
  TRY(wait_ready_on(c, src, vs));
  Past p{};
  const size_t f = (size_t)src->frame, need = (size_t)c->geom.lv[lvl].npix;
  TRY(past_take(c->past_pool, need, std::max<size_t>(need, 1024), &p));
  // the count stays on the device: one kernel copies the n valid points and n (stream ordered)
  launch_copy_cloud(p.d_pts, src->fs->p.pts_trk[lvl] + f * c->geom.lv[lvl].npix, p.d_n, src->fs->p.npts + f * REVO_L + lvl,
                    vs);
  HIPCHECK(hipGetLastError());
  TRY(vote_enqueued(c, src));
  p.n = -1;
  memcpy(p.T_w, T_w, sizeof(float) * 16);
  p.ts = ts;
  c->past.push_back(p);
  return REVO_OK;
}

// addOldPclAndPose(const Eigen::MatrixXf& pcl, const Eigen::Matrix4f& worldPose, double timeStamp), tracker.cpp:209-223,
// with the cloud in host memory (4 x n column-major = n packed float4)
extern "C" int revo_tracker_add_old_pcl_host(revo_ctx* c, const float* pcl, size_t n, const float T_w[16], double ts) {
  if (!c || !T_w || (!pcl && n)) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n > (size_t)c->geom.lv[0].npix) return fail(REVO_ERR_CAPACITY, "more points than pixels");
  HIPCHECK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  Past p{};
  TRY(past_take(c->past_pool, n, std::max<size_t>(n, 1024), &p));
  const int ni = (int)n;
  // pageable source: the runtime has read it when the call returns (the caller's matrix may die right after)
  hipStream_t vs = c->vote_stream;
  if (n) HIPCHECK(hipMemcpyAsync(p.d_pts, pcl, sizeof(float4) * n, hipMemcpyHostToDevice, vs));
  HIPCHECK(hipMemcpyAsync(p.d_n, &ni, sizeof(int), hipMemcpyHostToDevice, vs));
  HIPCHECK(hipStreamSynchronize(vs));
  p.n = ni;
  memcpy(p.T_w, T_w, sizeof(float) * 16);
  p.ts = ts;
  c->past.push_back(p);
  return REVO_OK;
}

extern "C" int revo_tracker_clear_past(revo_ctx* c) {  // tracker.cpp:248-257
  if (!c) return fail(REVO_ERR_INVALID_ARG, "null context");
  HIPCHECK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  while ((int)c->past.size() > c->ts.n_frames_hist_voting) {  // stream-ordered reuse of the buffers
    c->past_pool.push_back(c->past.front());
    c->past.pop_front();
  }
  return REVO_OK;
}
// a new REVO::start builds a new TrackerNew (system.cpp:107): empty lists.  Internal (revo_vo.hip).
extern "C" void revo_tracker_reset_past_(revo_ctx* c) {
  if (!c) return;
  std::lock_guard<std::mutex> lk(c->mu);
  while (!c->past.empty()) { c->past_pool.push_back(c->past.front()); c->past.pop_front(); }
}
extern "C" int revo_tracker_past_size(const revo_ctx* c) { return c ? (int)c->past.size() : 0; }

// one launch for one pair of pyramids on the context's tracker stream, result in w->h_out[0]; waits
static int pair_info_single(revo_ctx* c, const revo_pyr* ref, const revo_pyr* curr, const float* R, const float* T, int lvl) {
  if (!c->info_ws) TRY(infows_create(1, true, &c->info_ws));
  InfoWs* w = c->info_ws.get();
  hipStream_t s = c->stream;
  TRY(wait_ready(c, ref)); TRY(wait_ready(c, curr));
  float rt[12];
  memcpy(rt, R, sizeof(float) * 9); memcpy(rt + 9, T, sizeof(float) * 3);
  TRY(infows_upload_rt(w, 1, rt, s));
  fill_desc(w->descs.h, ref, curr, R, T);  // (the previous call waited for its stream: nothing reads the pinned row any more)
  TRY(w->descs.upload(1, s, false));
  launch_pair_info(w->descs.d, w->rt.d, 16, 12, info_params(c->tp, lvl), 1, w->d_part, w->d_cnt, w->d_ticket, w->d_out, s);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(w->h_out, w->d_out, sizeof(revo_pair_info), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}
extern "C" int revo_tracker_pair_info(revo_ctx* c, const revo_pyr* ref, const revo_pyr* curr, const float R[9], const float T[3],
                                      int lvl, revo_pair_info* out) {
  int rc = check_pair(c, ref, curr);
  if (rc) return rc;
  if (!R || !T || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (lvl < 0 || lvl >= c->geom.n_levels) return fail(REVO_ERR_LEVEL, "level out of range");
  for (int i = 0; i < 3; ++i) if (!std::isfinite(T[i])) return fail(REVO_ERR_INVALID_ARG, "T is not finite");
  HIPCHECK(hipSetDevice(c->device));
  std::lock_guard<std::mutex> lk(c->mu);
  rc = pair_info_single(c, ref, curr, R, T, lvl);
  if (rc) return rc;
  if (c->info_ws->h_out[0].flags & 1) return fail(REVO_ERR_NOT_ORTHOGONAL, "R is not orthogonal (Sophus::SO3 precondition)");
  *out = c->info_ws->h_out[0];
  return REVO_OK;
}
