// revo_host_impl.h -- what the host core's translation units (revo_host.hip, revo_frame.hip, revo_single.hip, revo_batch.hip,
// revo_pairs.hip, revo_mdev.hip) share: the handles' structs (each defined here and nowhere else, its members released by its
// destructor through the owners of revo_internal.h), the functions that cross units, and the small ones of the hot host paths
// (the sequential stream is host-bound).  Internal: only the host core's units include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <atomic>
#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "revo_dev.h"
#include "revo_internal.h"
#include "revo_mat4.h"
#include "revo_multi.h"
#include "revo_map.h"

// ----------------------------------------------------------------- objects --
struct FrameSet {
  int B = 0;
  DevMem<char> blob;
  size_t blob_bytes = 0;
  FramePlanes p{};
  float* own_depth0 = nullptr;  // the set's own level-0 depth plane (p.depth[0] may point at a borrowed input instead)
  uint8_t* d_bgr = nullptr;   // input staging (single-frame API)
  float* d_depth = nullptr;   // input staging; aliased as u16 for the u16 entry point
  // asynchronous creation (single-frame API): pinned host staging, "built" and "released" marks
  PinnedMem<uint8_t> h_bgr;
  PinnedMem<float> h_depth;
  StreamMark ready;  // recorded on the build stream after the last build kernel (a consumer on that stream is ordered already)
  // (batches) the end of the build has been DEFERRED to whoever needs it first -- normally the tracker launch of the batch, on
  // the tracker's stream: the build stream is the critical one of the pipelined step and the tracker streams have slack.  The
  // build ran only the gray half of pyrDown; the depth half and the tile-ordered edge lists of the CURRENT frames (odd) and the
  // keyframes' EDT (even frames) are left to run_pending_edt -- that is all a tracker grid reads (PairDesc)
  std::mutex edt_mu;
  std::atomic<bool> edt_pending{false};  // set by a batch build, cleared under edt_mu by whoever runs the deferred work
  int edt_count = 0;              // keyframes: frames 0, 2, 4, ...
  // whoever ran the deferred EDT recorded this on ITS stream: consumers (and the next build into these planes) on any other
  // stream order themselves behind it (`edt_pending == false` alone says "enqueued somewhere", not "visible here")
  StreamMark edt;
  // ... and the KEYFRAME-role frames' depth half and edge lists (even frames: no tracker grid of the batch reads them) are left to
  // whoever asks for them through an even view (wait_ready_on): same kernels, same inputs, frames 0, 2, 4, ...  Same lock, same
  // mark discipline as the EDT: set by every batch build, cleared by whoever runs the work, `ref` for consumers on other streams
  std::atomic<bool> ref_lists_pending{false};
  StreamMark ref;
  // ... and the BYTE edge planes (edges / edges_orig) of a batch that defers: its hot path reads the edge bitmaps alone, so the
  // build ends at them (PyrGeom::edge_bytes_lazy) and ensure_edge_bytes expands them for whoever reads a byte plane through a
  // view.  Same lock, same mark discipline; `lazy_edge_bytes` says how the LAST build left the set (its bitmaps in cs[] are then
  // also what the deferred EDT reads at every width)
  bool lazy_edge_bytes = false;
  std::atomic<bool> edge_bytes_pending{false};
  StreamMark ebytes;
  // (batches) the batch's last tracker grid: the deferred work rewrites what it reads (lists, counts, DT planes), on whatever
  // stream runs it -- run_pending_edt orders itself behind this mark.  The build stream writes none of those planes.
  const StreamMark* trk_mark = nullptr;
  StreamMark free_trk;   // recorded on the tracker stream when the set goes back to the pool
  StreamMark free_vote;  // ... and on the vote stream (the quality vote and the cloud copy read the set there)
  OwnedEvent h2d;        // (single-frame API) the copy out of page-locked caller rows has finished; made on first use
  // s will rewrite a recycled set's planes: its last consumers (tracker, vote) are done with them first
  int wait_previous_users(hipStream_t s) const { TRY(free_trk.wait(s)); return free_vote.wait(s); }
  int mark_built(hipStream_t s) { return ready.record(s); }  // accessors, single-pair calls and votes wait for this
  // reuse is ordered by the two marks: the next build into this set waits for everything the consumer streams have enqueued
  // against it so far
  void release_to(std::vector<FrameSet*>& pool, hipStream_t trk, hipStream_t vote) {
    (void)free_trk.record(trk);
    (void)free_vote.record(vote);
    pool.push_back(this);
  }
};

// Scratch of k_pair_info launches for up to n pairs: created on first use by whoever owns it (a batch, the
// context's single-pair calls, a revo_vo_multi handle).  One launch at a time per workspace, ordered by the owner's stream.
struct InfoRt { float v[16]; };  // R (9), T (3), a zero flag word, padding
struct InfoWs {
  int n = 0;
  HostRows<PairDesc> descs;
  HostRows<InfoRt> rt;
  DevMem<double> d_part; DevMem<int> d_cnt; DevMem<unsigned> d_ticket;
  DevMem<revo_pair_info> d_out; PinnedMem<revo_pair_info> h_out;
  OwnedEvent ev_done;
};

struct Past {  // one entry of mPastPcl / mPastWorldPoses / mPastTimeStamps (tracker.h:92-95)
  float4* d_pts; int* d_n; int n; float T_w[16]; double ts;
  size_t cap;  // points the buffer holds
};

// Experiment knobs (environment variables), read ONCE PER CONTEXT when it is created (they used to be
// process-wide statics, so two contexts of one process could not differ): the defaults are what ships.
struct Knobs {
  int track_depth;     // REVO_TRACK_DEPTH (1..4, default 2; REVO_TRACK_SERIAL=1 forces 1): tracker grids the resident gate keeps in flight
  int cluster_one;     // REVO_TRACK_CLUSTER_ONE (0 = automatic): workgroups of the single-pair launch
  int redundant_one;   // REVO_TRACK_REDUNDANT_ONE: levels up to this many points are evaluated redundantly by the single-pair launch
  int direct_h2d;      // REVO_DIRECT_H2D (default 1): revo_pyramid_create reads page-locked caller rows in place (no staging copy)
  int h2d_max_run_mb;  // REVO_H2D_MAX_RUN_MB: host-buffer batches merge adjacent frames into copies of at most this many MB
  bool kspec_one_set;  // REVO_TRACK_KSPEC_ONE (or no REVO_TRACK_KSPEC at all): the single-pair launches' own speculation depths
  int kspec_one[REVO_L];
  int upload_blocks;   // REVO_UPLOAD_BLOCKS: workgroups of the upload kernel for one contiguous plane
  int h2d_kernel;      // REVO_H2D_KERNEL (default 0): 1 = the in-place frame upload is a copy KERNEL reading the page-locked rows, not hipMemcpyAsync
  int stage_edge_depths;  // REVO_STAGE_EDGE_DEPTHS (default 0): pipelined batches stage the edge pixels' depths in the depth pass
};

struct revo_ctx {
  // handles (pyramids, batches, VO drivers) keep their context alive: revo_ctx_destroy only drops
  // the owner's reference, the last handle to go frees the device state
  std::atomic<int> refs{1};
  int device;
  Knobs knobs;
  revo_pyr_settings ps; revo_opt_settings os; revo_tracker_settings ts;
  PyrGeom geom;
  TrackParams tp;
  std::mutex mu;
  int framesets_created = 0;    // single-frame FrameSets that exist (free or in use)
  unsigned seq_next = 1;
  unsigned mail_epoch = 0;      // next free epoch window of d_mail (launch_track_one)
  int num_cus, blocks_per_cu;
  unsigned long long jobs_submitted = 0;
  float* d_pcl_out; uint8_t* d_pcl_clr[2]; int* d_pcl_chunk; unsigned* d_pcl_mask; int* d_pcl_total;  // inside d_pcl
  // What the context owns.  ~revo_ctx waits for the build, tracker, vote and frame-copy streams, frees the past clouds and the
  // pooled sets, and then the members below go in reverse order: the tracker stream last.
  OwnedStream stream;        // tracker / consumer stream
  std::unique_ptr<InfoWs> info_ws;  // revo_tracker_pair_info, allocated on first use
  DevMem<char> d_pcl;        // coloured point cloud (generateColoredPcl), allocated on first use
  // vote
  DevMem<unsigned> d_vote_done; PinnedMem<int> h_hist8; DevMem<int> d_hist8; DevMem<int> d_marks;
  // single-pair tracker scratch
  // the kernel reads the descriptor from its argument segment and writes the result straight into
  // pinned host memory: one launch + one sync per trackFrames, no copies on the stream
  DevMem<unsigned long long> d_mail;  // cluster mailbox of the single-pair path
  PinnedMem<unsigned> h_seq;          // [4] pinned: sequence words the kernels write after their results (slots 0/1: the VO driver's look-ahead launches, 2: the public single-pair calls)
  PinnedMem<EvalOut> h_eval;
  PinnedMem<revo_pair_result> h_res;  // [3]: slots 0/1 = the VO driver's look-ahead launches, slot 2 = the public single-pair calls
  PinnedMem<PairDesc> h_desc;
  std::vector<FrameSet*> pool;  // free single-frame FrameSets
  OwnedStream build_stream;  // pyramid builds of the single-frame API (overlap with tracking, like the IO thread)
  std::vector<Past> past_pool;  // recycled past-cloud buffers (no hipMalloc per frame)
  std::deque<Past> past;
  OwnedStream frame_copy_stream;  // single-frame API: H2D straight out of page-locked caller rows (pyramid_create_common)
  // host-buffer batches (revo_track_pairs_*): up to 3 jobs in flight, slots recycled per (n, depth type)
  std::vector<struct revo_pairs_job*> jobs;
  OwnedStream copy_stream2, copy_stream, pair_streams[2];
  // The quality vote and the past-cloud copies run on a stream of their own: nothing the NEXT frame's tracker reads comes out
  // of them, so in the sequential loop tracker N+1 follows tracker N directly instead of queueing behind vote N and copy N-1
  // (profiles/r06_single_stream_timeline.txt: ~35 us of 240).
  OwnedEvent ev_vote;
  OwnedStream vote_stream;
  ~revo_ctx();
};
void ctx_ref(revo_ctx* c);
void ctx_unref(revo_ctx* c);
struct CtxRef {  // a handle's reference to its context: the first member, so the last thing the handle lets go of
  revo_ctx* c = nullptr;
  ~CtxRef() { if (c) ctx_unref(c); }
  void hold(revo_ctx* x) { ctx_ref(x); c = x; }
  revo_ctx* operator->() const { return c; }
  operator revo_ctx*() const { return c; }
};

struct revo_pyr {
  revo_ctx* ctx;
  FrameSet* fs;
  int frame;
  bool owns_fs;
  bool is_kf;
  double ts;
  bool table_built;
  bool ref_list_built;  // edges3DPyr in the reference's order (the hot path only writes the tile-ordered list)
  bool dt_ready = false;  // the distance transforms are already enqueued on the tracker stream (revo_pyramid_prepare_keyframe_)
  bool has_colour = false;  // a view whose set keeps the colour image of its frame (revo_vo_multi's keyframe slots)
};

struct revo_batch {  // ~revo_batch waits for its stream first; the members go in reverse order
  CtxRef ctx;
  int n_pairs = 0;
  std::unique_ptr<FrameSet> fs;
  std::vector<revo_pyr> views;
  OwnedStream stream;
  // the batch's last tracker grid: a later launch of the SAME batch on another stream shares its mailbox and descriptors,
  // and the next build rewrites what it reads -- both order themselves behind this mark
  StreamMark trk;
  OwnedEvent ev1, ev0;                             // with timing: revo_batch_time_tracker
  std::unique_ptr<InfoWs> info_ws;                 // revo_batch_pair_info, allocated on first use
  DevMem<unsigned long long> d_mail;
  HostRows<PairDesc> descs;                        // its event: the upload of the initial poses has read the pinned rows
  PinnedMem<revo_pair_result> h_flags;             // pinned scratch for last_results
  unsigned mail_epoch = 0;
  bool identity_uploaded = false;  // descs.d already holds the identity initial poses (nothing to upload)
  int cluster = 1;
  bool defer = true;               // REVO_DEFER / REVO_EDT_DEFER, read when the batch is created (env_defer)
  hipEvent_t tev0 = nullptr, tev1 = nullptr;       // (revo_batch_time_next_grid_) recorded directly around the NEXT tracker grid, then cleared
  const revo_pair_result* last_results = nullptr;  // device records of the last track launch (revo_batch_sync decodes their flags)
  ~revo_batch();
};

// ---------------------------------------------------- functions that cross units --
// revo_host.hip
int pick_cluster(const revo_ctx* c, int n_pairs);
int chained_track_launch_(int device, int depth, hipStream_t s, int (*launch)(void* f, unsigned* d_resident), void* f);
// launch(d_resident): enqueues the tracker grid on s and returns its workgroup count (the resident gate, revo_host.hip)
template <typename F>
int chained_track_launch(int device, int depth, hipStream_t s, F&& launch) {
  return chained_track_launch_(device, depth, s, [](void* f, unsigned* d) { return (*(std::remove_reference_t<F>*)f)(d); }, (void*)&launch);
}
int wait_seq(hipStream_t s, volatile unsigned* word, unsigned want);
int wait_event_polled(hipEvent_t ev);
// host_staging = false: device-side input planes only (inputs go straight from the caller's rows to the device)
int frameset_create(revo_ctx* c, int B, bool with_staging, FrameSet** out, bool host_staging = true);
void enqueue_build(revo_ctx* c, FrameSet* fs, const uint8_t* d_bgr, const float* d_depth_f32, const uint16_t* d_depth_u16,
                   float alpha, hipStream_t s, bool borrow_depth = false, bool with_points = true, int frame0 = 0,
                   int nframes = -1, bool gray_only = false);
int run_pending_edt(revo_ctx* c, FrameSet* fs, hipStream_t s, bool need_ref_lists = false);
int wait_edt_before_rebuild(FrameSet* fs, hipStream_t s);
// THE place where the byte edge planes of a lazily built set come into being: every reader of edges / edges_orig through a view
// calls it on its stream first (a no-op for sets whose build wrote them).  Behind the set's "built" event, i.e. behind fill-in.
int ensure_edge_bytes(revo_ctx* c, FrameSet* fs, hipStream_t s);
// the context's geometry for kernels that read a set's edges (the EDT's column pass): a lazily built set has its bitmaps only
inline PyrGeom geom_of_set(const revo_ctx* c, const FrameSet* fs) {
  PyrGeom g = c->geom;
  g.edge_bytes_lazy = fs->lazy_edge_bytes ? 1 : 0;
  return g;
}
// revo_single.hip
int decode_track(const revo_pair_result& r, float R[9], float T[3], float* err, int* status, revo_residual_info* info, int32_t* iters);
// A past-cloud buffer for at least `need` points out of `pool`: recycled if one is large enough (no hipMalloc per frame in
// the steady state), else a new one of `cap` points.  The oldest pooled one that fits, or the newest (revo_mdev's are all alike).
int past_take(std::vector<Past>& pool, size_t need, size_t cap, Past* out, bool newest = false);
void past_free(Past& p);
// revo_batch.hip.  own_out: the workspace also holds n output records on the device and their pinned host copy
int infows_create(int n, bool own_out, std::unique_ptr<InfoWs>* out);
InfoParams info_params(const TrackParams& tp, int lvl);
int infows_upload_rt(InfoWs* w, int n, const float* h_RT, hipStream_t s);  // n host poses (12 floats each) -> w->rt.d, on s
// revo_pairs.hip
void pairs_jobs_release(revo_ctx* c);

// --------------------------------------------------------- small and hot --
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// sized for the larger of the two tracker layouts: the exact-sums instantiation may run on any mailbox
inline size_t mail_bytes(int n_pairs, int cluster) { return sizeof(unsigned long long) * (size_t)n_pairs * 2 * cluster * TRACK_MAIL_NVAL; }

inline void fill_desc(PairDesc* d, const revo_pyr* ref, const revo_pyr* curr, const float* R, const float* T) {
  const PyrGeom& g = ref->ctx->geom;
  memset(d, 0, sizeof(*d));
  for (int l = 0; l < g.n_levels; ++l) {
    d->pts[l] = curr->fs->p.pts_trk[l] + (size_t)curr->frame * g.lv[l].npix;
    d->dt[l] = ref->fs->p.dt[l] + (size_t)ref->frame * g.lv[l].npix;
  }
  d->npts = curr->fs->p.npts + (size_t)curr->frame * REVO_L;
  if (R) memcpy(d->R, R, sizeof(float) * 9); else { d->R[0] = d->R[4] = d->R[8] = 1.f; }
  if (T) memcpy(d->T, T, sizeof(float) * 3);
}

inline int check_pair(const revo_ctx* c, const revo_pyr* ref, const revo_pyr* curr) {
  if (!c || !ref || !curr) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (ref->ctx != c || curr->ctx != c) return fail(REVO_ERR_INVALID_ARG, "pyramid belongs to another context");
  if (!ref->is_kf) return fail(REVO_ERR_NOT_KEYFRAME, "optimizationStructure not built! (reference frame is not a keyframe)");
  return REVO_OK;
}

// Order the consumer stream after the (asynchronous) build of a single-frame pyramid.
inline int wait_ready_on(revo_ctx* c, const revo_pyr* p, hipStream_t s) {
  // single-frame pyramids: built on the build stream; batch views: built on the batch's / the caller's stream
  // (revo_batch_build records the mark) -- either way the consumer stream is ordered behind the build
  TRY(p->fs->ready.wait(s));
  // an accessor / single-pair call on a batch view: runs the deferred EDT if it is still pending, waits for it otherwise; an
  // EVEN view (keyframe role) also gets its own edge lists and coarser depth levels, which the batch's trackers never needed
  return run_pending_edt(c, p->fs, s, (p->frame & 1) == 0);
}
inline int wait_ready(revo_ctx* c, const revo_pyr* p) { return wait_ready_on(c, p, c->stream); }

// Frames' planes into device memory on one stream, `rows` rows each.  Frames that lie back to back in the source (a decoder
// that fills one slab per plane type) and in the destination travel in ONE copy per run of adjacent frames, of at most
// max_run bytes; a frame whose rows are padded takes a strided copy of its own.  add() per frame, flush() behind the last.
struct RowCopier {
  hipMemcpyKind kind; int rows; hipStream_t stream; size_t max_run;
  char* dst = nullptr; const char* src = nullptr; size_t bytes = 0;  // the run so far
  hipError_t flush() {
    if (!bytes) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, stream);
    bytes = 0;
    return e;
  }
  hipError_t add(void* d, const void* s, size_t src_stride, size_t row_bytes) {
    if (src_stride != row_bytes) {  // padded rows: a strided copy of its own
      const hipError_t e = flush();
      if (e != hipSuccess) return e;
      return hipMemcpy2DAsync(d, row_bytes, s, src_stride, row_bytes, rows, kind, stream);
    }
    const size_t n = row_bytes * rows;
    if (bytes && bytes + n <= max_run && src + bytes == (const char*)s && dst + bytes == (char*)d) { bytes += n; return hipSuccess; }
    const hipError_t e = flush();
    if (e != hipSuccess) return e;
    dst = (char*)d; src = (const char*)s; bytes = n;
    return hipSuccess;
  }
};

// The vote (assessTrackingQuality, tracker.cpp:118-201), the two host pieces every path shares.  A past cloud seen from the
// current frame: RT = rotation (column-major 3 x 3) and translation of inv(T_w_curr) * T_w_past.
inline void vote_cloud_pose(const float inv[16], const Past& past, float RT[12]) {
  float tf[16];
  mat4_mul(inv, past.T_w, tf);
  for (int cc = 0; cc < 3; ++cc) for (int r = 0; r < 3; ++r) RT[cc * 3 + r] = tf[cc * 4 + r];
  RT[9] = tf[12]; RT[10] = tf[13]; RT[11] = tf[14];
}
// The decision from the overlaps ov[0..3] of a vote of nframes (<= 3) clouds.  ratio (may be null): overlapMeasure / ov[0],
// how far the frame is from asking for a new keyframe (< 1 does, tracker.cpp:184); +inf while fewer than three past clouds
// vote (the answer is OK whatever the numbers) or nothing overlaps.
inline int vote_decide(const int32_t ov[4], int nframes, float* ratio) {
  const float wts[4] = {0.f, 1.f, 1.25f, 1.5f};  // tracker.cpp:231-234
  float overlapMeasure = 0.0f;
  const int hsize = 1 + nframes;
  for (int k = 1; k < hsize; ++k) overlapMeasure += (ov[k] * wts[k]);
  if (ratio) *ratio = nframes >= 3 && ov[0] > 0 ? overlapMeasure / (float)ov[0] : INFINITY;
  return (overlapMeasure >= ov[0] || hsize < 4) ? REVO_TRACKER_STATE_OK : REVO_TRACKER_STATE_NEW_KF;  // tracker.cpp:184
}
