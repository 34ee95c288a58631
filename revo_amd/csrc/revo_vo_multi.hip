// revo_vo_multi.hip -- many independent REVO::start streams (system/system.cpp:84-305) advanced in lockstep.
// Host-only code: per stream the state of revo_vo.hip (keyframe, previous frame, the last two poses, the constant-velocity
// initialisation); the device work of a step -- one tracker grid, one quality vote, one cloud copy, the keyframe promotions --
// is what revo_mdev_* (revo_mdev.hip) enqueue for all streams at once.  No look-ahead: a step waits for its grid and its vote.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "revo_internal.h"
#include "revo_mat4.h"
#include "revo_multi.h"
#include "revo_map.h"
#include "revo_pose_host.h"
#include "revo_surface_ring.h"

namespace {
struct Ref { void* set; int frame; double ts; };  // a frame of a step set
bool on_device(const void* p, int dev) {  // device memory of `dev` (not host, not another device)
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice && a.device == dev;
}

// revo_vo's per-driver state, per stream
struct Stream {
  std::deque<Ref> queue;
  bool has_prev = false;
  Ref prev{nullptr, 0, 0.0};
  M4 T_w_kf = M4::identity();
  Pose last{M4::identity(), M4::identity()}, before_last{M4::identity(), M4::identity()};
  M4 T_NM1_N = M4::identity();
  float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, T[3] = {0, 0, 0};
  int no_frames = 0, n_keyframes = 0;
  bool just_added_kf = false;
  bool retrack = false;  // a keyframe change is owed its re-track of `cur` (the step after the vote that asked for it)
  Ref cur{nullptr, 0, 0.0};
  double kf_ts = 0.0;     // time stamp of the stream's keyframe
  bool has_info = false;  // revo_vo_multi_set_pair_info: the record of the last reported frame
  revo_pair_info info{};
  double info_kf_ts = 0.0;
};
// revo_vo_multi_attach_surface's per-stream state: the attachment, the last keyframe's report and the device record its fuse writes
// A view a windowed surface holds, as it can be named again: device copies of the keyframe's level-0 depth plane and colour image
// (allocated when the slot is first used; bgr stays NULL without a colour volume), the pose it was fused at, its time stamp.
struct KeptView {
  float* depth = nullptr;
  uint8_t* bgr = nullptr;
  float T[16] = {};
  double ts = 0.0;
};
struct Surface {
  bool on = false, has_last = false;
  revo_vo_multi_surface s{};
  revo_vo_multi_surface_report last{};
  revo_map_carve_view_info* d_vinfo = nullptr;  // device, 32 bytes: the view info of the last fuse
  // revo_vo_multi_surface_window: which views are held (revo_surface_ring.h), what names them again, and the device
  // record the last eviction's job writes
  SurfaceRing ring;
  std::vector<KeptView> kept;                   // ring.slots() of them
  revo_map_tsdf_unfuse_info* d_evict = nullptr; // device, 64 bytes
  double evict_ts = 0.0;
  bool evict_enqueued = false;                  // the last eviction's call was taken: d_evict holds (or will hold) its info
};
static_assert(sizeof(revo_vo_multi_surface_window_report) == 104 && offsetof(revo_vo_multi_surface_window_report, held) == 4 &&
              offsetof(revo_vo_multi_surface_window_report, evictions) == 8 && offsetof(revo_vo_multi_surface_window_report, evicted_timestamp) == 16 &&
              offsetof(revo_vo_multi_surface_window_report, evicted) == 24, "the window report is the documented layout");
// The window's slots and its record go back; the ring is off.  hipFree waits for the work that may still read them.
void window_free(Surface& f) {
  for (KeptView& k : f.kept) { (void)hipFree(k.depth); (void)hipFree(k.bgr); }
  f.kept.clear();
  (void)hipFree(f.d_evict);
  f.d_evict = nullptr;
  f.ring.set(0);
  f.evict_ts = 0.0; f.evict_enqueued = false;
}
static_assert(sizeof(revo_vo_multi_surface) == 120 && offsetof(revo_vo_multi_surface, trunc) == 32 && offsetof(revo_vo_multi_surface, tsdf) == 40 &&
              offsetof(revo_vo_multi_surface, track_prm) == 56 && offsetof(revo_vo_multi_surface, track_opts) == 88, "the surface record is the documented layout");
static_assert(sizeof(revo_vo_multi_surface_report) == 408 && offsetof(revo_vo_multi_surface_report, T_fused) == 72 && offsetof(revo_vo_multi_surface_report, track) == 136 &&
              offsetof(revo_vo_multi_surface_report, iterations) == 344 && offsetof(revo_vo_multi_surface_report, view_info) == 360 &&
              offsetof(revo_vo_multi_surface_report, keyframes_fused) == 392, "the report is the documented layout");
}  // namespace

struct revo_vo_multi {
  revo_ctx* ctx = nullptr;
  revo_mdev* dev = nullptr;
  int S = 0, max_queue = 1;
  std::vector<Stream> st;
  std::vector<std::pair<void*, int>> refs;  // step sets and how many queued / current / previous frames still point into them
  std::vector<revo_map*> maps;              // per stream: the voxel map its promoted keyframes go into (revo_vo_multi_attach_map)
  revo_map_stage* map_stage = nullptr;      // descriptors of the step's batched map integration
  bool pair_info = false;                   // revo_vo_multi_set_pair_info
  std::vector<Surface> surf;                // per stream: the surface its promoted keyframes are fused into (revo_vo_multi_attach_surface)
  int n_surf = 0;                           // how many streams have one
};

static void ref_add(revo_vo_multi* m, void* set) {
  for (auto& r : m->refs) if (r.first == set) { ++r.second; return; }
  m->refs.push_back({set, 1});
}
static void ref_drop(revo_vo_multi* m, void* set) {
  for (size_t k = 0; k < m->refs.size(); ++k)
    if (m->refs[k].first == set) {
      if (--m->refs[k].second == 0) { revo_mdev_release_set_(m->dev, set); m->refs.erase(m->refs.begin() + k); }
      return;
    }
}

extern "C" int revo_vo_multi_create(revo_ctx* ctx, int n_streams, int max_queue, revo_vo_multi** out) {
  if (!ctx || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n_streams < 1 || n_streams > 1024) return fail(REVO_ERR_INVALID_ARG, "n_streams must be 1..1024");
  if (max_queue < 1) return fail(REVO_ERR_INVALID_ARG, "max_queue must be >= 1");
  revo_mdev* d = nullptr;
  const int rc = revo_mdev_create_(ctx, n_streams, &d);
  if (rc) return rc;
  revo_vo_multi* m = new revo_vo_multi();
  m->ctx = ctx;
  revo_ctx_retain_(ctx);
  m->dev = d;
  m->S = n_streams;
  m->max_queue = max_queue;
  m->st.resize(n_streams);
  m->maps.assign(n_streams, nullptr);
  m->surf.resize(n_streams);
  *out = m;
  return REVO_OK;
}

extern "C" void revo_vo_multi_destroy(revo_vo_multi* m) {
  if (!m) return;
  for (int s = 0; s < m->S; ++s) {
    revo_map_note_attach_(m->maps[s], m, s, 0);
    if (m->surf[s].on) revo_map_note_attach_(m->surf[s].s.map, m, s, 0);
  }
  revo_mdev_destroy_(m->dev);  // (synchronises the context's streams; the step sets go with it)
  for (Surface& f : m->surf) { (void)hipFree(f.d_vinfo); window_free(f); }
  revo_map_stage_destroy_(m->map_stage);
  revo_ctx_release_(m->ctx);
  delete m;
}

static bool stream_ok(const revo_vo_multi* m, int s) { return m && s >= 0 && s < m->S; }

// A map knows the streams that hold it, as a voxel map or through a surface: told again whenever either changes.
static void renote(revo_vo_multi* m, int s, revo_map* map) {
  revo_map_note_attach_(map, m, s, (m->maps[s] == map || (m->surf[s].on && m->surf[s].s.map == map)) ? 1 : 0);
}
static void surface_detach(revo_vo_multi* m, int s) {
  Surface& f = m->surf[s];
  if (!f.on) return;
  revo_map* old = f.s.map;
  f.on = false; f.has_last = false;
  window_free(f);
  --m->n_surf;
  renote(m, s, old);
}

extern "C" int revo_vo_multi_pending(const revo_vo_multi* m, int s) {
  if (!stream_ok(m, s)) return -1;
  return (int)m->st[s].queue.size() + (m->st[s].retrack ? 1 : 0);
}
extern "C" int revo_vo_multi_num_keyframes(const revo_vo_multi* m, int s) { return stream_ok(m, s) ? m->st[s].n_keyframes : -1; }

extern "C" int revo_vo_multi_keyframe(const revo_vo_multi* m, int s, revo_pyr** kf, float T_w_kf[16]) {
  if (!stream_ok(m, s)) return fail(REVO_ERR_INVALID_ARG, "stream out of range");
  if (m->st[s].n_keyframes == 0) return fail(REVO_ERR_INVALID_ARG, "the stream has no keyframe yet");
  if (kf) *kf = revo_mdev_keyframe_(m->dev, s);
  if (T_w_kf) memcpy(T_w_kf, m->st[s].T_w_kf.m, sizeof(float) * 16);
  return REVO_OK;
}

extern "C" int revo_vo_multi_set_pair_info(revo_vo_multi* m, int on) {
  if (!m) return fail(REVO_ERR_INVALID_ARG, "null argument");
  m->pair_info = on != 0;
  if (!m->pair_info) for (Stream& x : m->st) x.has_info = false;
  return REVO_OK;
}
extern "C" int revo_vo_multi_pair_info(const revo_vo_multi* m, int s, revo_pair_info* out, double* kf_timestamp) {
  if (!stream_ok(m, s) || !out) return fail(REVO_ERR_INVALID_ARG, "bad argument");
  if (!m->pair_info || !m->st[s].has_info) return fail(REVO_ERR_INVALID_ARG, "no pair information: the option is off or the stream has reported nothing yet");
  *out = m->st[s].info;
  if (kf_timestamp) *kf_timestamp = m->st[s].info_kf_ts;
  return REVO_OK;
}

// a new sequence on this stream: REVO::start's fresh TrackerNew and empty pose graph (system.cpp:107)
extern "C" int revo_vo_multi_reset(revo_vo_multi* m, int s) {
  if (!stream_ok(m, s)) return fail(REVO_ERR_INVALID_ARG, "stream out of range");
  Stream& x = m->st[s];
  if (!x.queue.empty() || x.retrack) return fail(REVO_ERR_INVALID_ARG, "the stream still has frames pending");
  if (x.has_prev) ref_drop(m, x.prev.set);
  revo_mdev_clear_past_(m->dev, s, 0);
  x = Stream();
  revo_map_note_attach_(m->maps[s], m, s, 0);  // the next sequence starts without a map
  m->maps[s] = nullptr;
  surface_detach(m, s);                        // ... and without a surface
  return REVO_OK;
}

// The map's work (and the integration of promoted slots) is ordered on the tracker stream behind each promotion; a map
// attached here must live on the handle's context (its stream and its keyframe slots).
extern "C" int revo_vo_multi_attach_map(revo_vo_multi* m, int s, revo_map* map) {
  if (!stream_ok(m, s)) return fail(REVO_ERR_INVALID_ARG, "stream out of range");
  if (map && revo_map_ctx_(map) != m->ctx) return fail(REVO_ERR_INVALID_ARG, "the map belongs to another context than the handle");
  if (map && !m->map_stage) {
    const int rc = revo_map_stage_create_(&m->map_stage);
    if (rc) return rc;
  }
  revo_map* old = m->maps[s];
  m->maps[s] = map;
  renote(m, s, old);
  renote(m, s, map);
  return REVO_OK;
}
// revo_map_destroy of an attached map: the stream's surface on that map goes with it
extern "C" void revo_vo_multi_forget_map_(revo_vo_multi* m, int s, revo_map* map) {
  if (!stream_ok(m, s)) return;
  if (m->maps[s] == map) m->maps[s] = nullptr;
  if (m->surf[s].on && m->surf[s].s.map == map) { m->surf[s].on = false; m->surf[s].has_last = false; window_free(m->surf[s]); --m->n_surf; }
}

extern "C" int revo_vo_multi_attach_surface(revo_vo_multi* m, int s, const revo_vo_multi_surface* in) {
  if (!stream_ok(m, s)) return fail(REVO_ERR_INVALID_ARG, "stream out of range");
  if (!in) { surface_detach(m, s); return REVO_OK; }
  if (!in->map || revo_map_ctx_(in->map) != m->ctx) return fail(REVO_ERR_INVALID_ARG, "the surface's map is NULL or belongs to another context than the handle");
  if (in->track != 0 && in->track != 1) return fail(REVO_ERR_INVALID_ARG, "track must be 0 or 1");
  MapCtxGeom g;
  const int rc = revo_map_ctx_geom_(m->ctx, &g);
  if (rc) return rc;
  if (!in->tsdf || !on_device(in->tsdf, g.device) || (in->color && !on_device(in->color, g.device)))
    return fail(REVO_ERR_INVALID_ARG, "the surface's volumes must be in device memory of the handle's device");
  if (((uintptr_t)in->tsdf | (uintptr_t)in->color) & 15) return fail(REVO_ERR_INVALID_ARG, "the surface's volumes are not 16-byte aligned");
  for (int k = 0; k < 3; ++k)
    if (in->box.n[k] < 1 || in->box.n[k] > 1024 || in->box.lo[k] < -(1 << 20) || (long long)in->box.lo[k] + in->box.n[k] - 1 > (1 << 20) - 1)
      return fail(REVO_ERR_INVALID_ARG, "the surface's box breaks the box rules");
  if ((size_t)in->box.n[0] * (size_t)in->box.n[1] * (size_t)in->box.n[2] > ((size_t)1 << 27)) return fail(REVO_ERR_INVALID_ARG, "the surface's box holds more than 2^27 cells");
  if (!std::isfinite(in->trunc) || in->trunc < 0.0f) return fail(REVO_ERR_INVALID_ARG, "the surface's trunc must be 0 or finite and > 0");
  if (in->track && in->track_opts.max_iters < 0) return fail(REVO_ERR_INVALID_ARG, "max_iters must be >= 0");
  Surface& f = m->surf[s];
  if (!f.d_vinfo) HIPCHECK(hipMalloc((void**)&f.d_vinfo, sizeof(revo_map_carve_view_info)));
  surface_detach(m, s);
  f.s = *in;
  if (f.s.trunc == 0.0f) {  // the default, resolved once: the tracking jobs need the number
    float voxel = 0.0f;
    const int rv = revo_map_voxel_size(in->map, &voxel, nullptr);
    if (rv) return rv;
    f.s.trunc = 4.0f * voxel;
  }
  f.on = true; f.has_last = false;
  memset(&f.last, 0, sizeof(f.last));
  ++m->n_surf;
  renote(m, s, in->map);
  return REVO_OK;
}

extern "C" int revo_vo_multi_surface_last(revo_vo_multi* m, int s, revo_vo_multi_surface_report* out) {
  if (!stream_ok(m, s) || !out) return fail(REVO_ERR_INVALID_ARG, "bad argument");
  Surface& f = m->surf[s];
  if (!f.on || !f.has_last) return fail(REVO_ERR_INVALID_ARG, "no surface report: no surface is attached or the stream has promoted no keyframe since");
  if (f.last.fused) {  // the record of that step's fuse, behind it on the tracker stream
    MapCtxGeom g;
    const int rc = revo_map_ctx_geom_(m->ctx, &g);
    if (rc) return rc;
    HIPCHECK(hipStreamSynchronize((hipStream_t)g.stream));
    HIPCHECK(hipMemcpy(&f.last.view_info, f.d_vinfo, sizeof(f.last.view_info), hipMemcpyDeviceToHost));
  }
  *out = f.last;
  return REVO_OK;
}

extern "C" int revo_vo_multi_surface_window(revo_vo_multi* m, int s, int window) {
  if (!stream_ok(m, s)) return fail(REVO_ERR_INVALID_ARG, "stream out of range");
  Surface& f = m->surf[s];
  if (!f.on) return fail(REVO_ERR_INVALID_ARG, "revo_vo_multi_surface_window: no surface is attached to the stream");
  if (!SurfaceRing::valid(window)) return fail(REVO_ERR_INVALID_ARG, "revo_vo_multi_surface_window: window must be 0 (off) or 1 .. 1024 views");
  window_free(f);
  if (!window) return REVO_OK;
  HIPCHECK(hipMalloc((void**)&f.d_evict, sizeof(revo_map_tsdf_unfuse_info)));
  f.ring.set(window);
  f.kept.resize((size_t)f.ring.slots());
  return REVO_OK;
}

extern "C" int revo_vo_multi_surface_window_last(revo_vo_multi* m, int s, revo_vo_multi_surface_window_report* out) {
  if (!stream_ok(m, s) || !out) return fail(REVO_ERR_INVALID_ARG, "bad argument");
  Surface& f = m->surf[s];
  if (!f.on || !f.ring.on()) return fail(REVO_ERR_INVALID_ARG, "no window report: no surface is attached to the stream or it has no window");
  memset(out, 0, sizeof(*out));
  out->window = f.ring.window; out->held = f.ring.held;
  out->evictions = f.ring.evictions;
  if (!f.ring.evictions) return REVO_OK;
  out->evicted_timestamp = f.evict_ts;
  out->evicted.status = REVO_ERR_INVALID_ARG;  // a call that was not taken took nothing out
  if (f.evict_enqueued) {  // the record of that step's unfuse, behind it on the tracker stream
    MapCtxGeom g;
    const int rc = revo_map_ctx_geom_(m->ctx, &g);
    if (rc) return rc;
    HIPCHECK(hipStreamSynchronize((hipStream_t)g.stream));
    HIPCHECK(hipMemcpy(&out->evicted.info, f.d_evict, sizeof(out->evicted.info), hipMemcpyDeviceToHost));
    out->evicted.status = out->evicted.info.misfits ? REVO_ERR_INVALID_ARG : REVO_OK;
  }
  return REVO_OK;
}

// The windows of a step, behind its fuse on the tracker stream: every keyframe in `who` (streams whose keyframe was
// fused) that has a window is kept -- device copies of its slot's level-0 depth plane and colour image, T_fused -- and every
// stream that then holds more than its window has its oldest view taken out, all in one revo_map_tsdf_unfuse_many, as the raw view
// of the kept copies.  Nothing waits and nothing fails the step: a keyframe that cannot be kept is not held, and an eviction
// that the call or the device refuses forgets the view and leaves it in the volumes.
static void windows_step(revo_vo_multi* m, const std::vector<int>& who) {
  MapCtxGeom g;
  if (revo_map_ctx_geom_(m->ctx, &g) != REVO_OK) return;
  hipStream_t st = (hipStream_t)g.stream;
  const size_t px = (size_t)g.w * (size_t)g.h;
  std::vector<int> over;
  for (int s : who) {
    Surface& f = m->surf[s];
    if (!f.ring.on()) continue;
    MapSource src;
    if (revo_map_source_(revo_mdev_keyframe_(m->dev, s), &src) != REVO_OK) continue;
    KeptView& k = f.kept[(size_t)f.ring.next()];  // held only once its copies are enqueued
    if (!k.depth && hipMalloc((void**)&k.depth, px * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); k.depth = nullptr; continue; }
    if (f.s.color && !k.bgr && hipMalloc((void**)&k.bgr, px * 3) != hipSuccess) { (void)hipGetLastError(); k.bgr = nullptr; continue; }
    if (hipMemcpyAsync(k.depth, src.depth, px * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess ||
        (f.s.color && hipMemcpyAsync(k.bgr, src.bgr, px * 3, hipMemcpyDeviceToDevice, st) != hipSuccess)) { (void)hipGetLastError(); continue; }
    memcpy(k.T, f.last.T_fused, sizeof(k.T));
    k.ts = f.last.timestamp;
    (void)f.ring.push();
    if (f.ring.over()) over.push_back(s);
  }
  if (over.empty()) return;
  std::vector<revo_map_tsdf_unfuse_job> jobs(over.size());
  for (size_t i = 0; i < over.size(); ++i) {
    Surface& f = m->surf[over[i]];
    const KeptView& k = f.kept[(size_t)f.ring.oldest()];
    revo_map_tsdf_unfuse_job& j = jobs[i];
    memset(&j, 0, sizeof(j));
    j.map = f.s.map; j.box = f.s.box;
    j.trunc = f.s.trunc;
    j.tsdf = f.s.tsdf; j.color = f.s.color;
    j.view.depth = k.depth;  // a raw view with the context's camera and depth range: the bytes of the pyramid view it was fused as
    j.view.width = g.w; j.view.height = g.h;
    memcpy(j.view.T_w_c, k.T, sizeof(j.view.T_w_c));
    j.bgr = f.s.color ? k.bgr : nullptr;
    j.info = f.d_evict;
  }
  const bool ok = revo_map_tsdf_unfuse_many(jobs[0].map, (int)jobs.size(), jobs.data(), nullptr, 1) == REVO_OK;
  for (int s : over) {
    Surface& f = m->surf[s];
    f.evict_ts = f.kept[(size_t)f.ring.oldest()].ts;
    f.evict_enqueued = ok;
    (void)f.ring.evict();
  }
}

// The promoted keyframes of a step whose streams have a surface, as the sequential driver handles each (vo.REVO): tracked against
// the surface as it stands, all loops in lockstep; then fused, all in one launch, at the refined pose where the loop converged and
// at T_w_kf otherwise.  Nothing here fails the step: a call that is refused leaves its keyframes unfused and counted.
static void surfaces_step(revo_vo_multi* m, const std::vector<MultiFrame>& promote) {
  if (!m->n_surf) return;
  std::vector<int> on;  // indices into promote
  for (size_t i = 0; i < promote.size(); ++i)
    if (m->surf[promote[i].stream].on) on.push_back((int)i);
  if (on.empty()) return;
  for (int i : on) {
    const MultiFrame& p = promote[i];
    Surface& f = m->surf[p.stream];
    revo_vo_multi_surface_report& r = f.last;
    const uint64_t fused = r.keyframes_fused, skipped = r.keyframes_skipped;
    memset(&r, 0, sizeof(r));
    r.keyframes_fused = fused; r.keyframes_skipped = skipped;
    r.timestamp = p.ts;
    memcpy(r.T_w_kf, p.T_w, sizeof(r.T_w_kf));
    memcpy(r.T_fused, p.T_w, sizeof(r.T_fused));
    r.status = REVO_ALIGN_LOST;
    f.has_last = true;
  }
  // the loops, one call per set of options (one, unless the streams were given different ones)
  std::vector<int> todo;
  for (int i : on) {
    const Surface& f = m->surf[promote[i].stream];
    if (f.s.track && pose_is_finite(promote[i].T_w) && pose_is_orthogonal(promote[i].T_w)) todo.push_back(i);
  }
  auto opts_of = [](const Surface& f) {
    revo_map_align_opts o = f.s.track_opts;
    if (o.max_iters == 0) o = revo_map_align_opts{30, 0, 1e-6, 1e-6, 12};
    return o;
  };
  while (!todo.empty()) {
    const revo_map_align_opts o = opts_of(m->surf[promote[todo[0]].stream]);
    std::vector<int> now, later;
    for (int i : todo) {
      const revo_map_align_opts oi = opts_of(m->surf[promote[i].stream]);
      (oi.max_iters == o.max_iters && oi.eps_t == o.eps_t && oi.eps_r == o.eps_r && oi.min_matched == o.min_matched ? now : later).push_back(i);
    }
    std::vector<revo_map_tsdf_track_job> jobs(now.size());
    std::vector<revo_map_tsdf_track_result> res(now.size());
    for (size_t k = 0; k < now.size(); ++k) {
      const MultiFrame& p = promote[now[k]];
      const Surface& f = m->surf[p.stream];
      revo_map_tsdf_track_job& j = jobs[k];
      memset(&j, 0, sizeof(j));
      j.map = f.s.map; j.box = f.s.box;
      j.trunc = f.s.trunc;
      j.tsdf = f.s.tsdf;
      j.frame.kf = revo_mdev_keyframe_(m->dev, p.stream);
      j.prm = f.s.track_prm;
      j.poses = p.T_w;
    }
    if (revo_map_tsdf_track_many(jobs[0].map, (int)jobs.size(), jobs.data(), &o, res.data(), nullptr) == REVO_OK)
      for (size_t k = 0; k < now.size(); ++k) {
        revo_vo_multi_surface_report& r = m->surf[promote[now[k]].stream].last;
        r.track = res[k].info;
        r.iterations = res[k].iterations; r.status = res[k].status;
        r.tracked = 1;
        if (r.status == REVO_ALIGN_CONVERGED) memcpy(r.T_fused, res[k].T, sizeof(r.T_fused));
      }
    todo.swap(later);
  }
  // the fuse
  std::vector<revo_map_tsdf_fuse_job> jobs;
  std::vector<int> who;
  for (int i : on) {
    const MultiFrame& p = promote[i];
    Surface& f = m->surf[p.stream];
    if (!pose_is_finite(f.last.T_fused) || !pose_is_orthogonal(f.last.T_fused)) { ++f.last.keyframes_skipped; continue; }
    revo_map_tsdf_fuse_job j;
    memset(&j, 0, sizeof(j));
    j.map = f.s.map; j.box = f.s.box;
    j.trunc = f.s.trunc;
    j.tsdf = f.s.tsdf; j.color = f.s.color;
    j.view.kf = revo_mdev_keyframe_(m->dev, p.stream);
    memcpy(j.view.T_w_c, f.last.T_fused, sizeof(j.view.T_w_c));
    j.view_info = f.d_vinfo;
    jobs.push_back(j);
    who.push_back(p.stream);
  }
  if (jobs.empty()) return;
  const bool ok = revo_map_tsdf_fuse_many(jobs[0].map, (int)jobs.size(), jobs.data()) == REVO_OK;
  bool windows = false;
  for (int s : who) {
    revo_vo_multi_surface_report& r = m->surf[s].last;
    if (ok) { r.fused = 1; ++r.keyframes_fused; } else ++r.keyframes_skipped;
    windows = windows || m->surf[s].ring.on();
  }
  if (ok && windows) windows_step(m, who);  // without a window on any of them nothing more is enqueued
}

static int submit(revo_vo_multi* m, int n, const revo_stream_frame* frames, int depth_is_u16, double depth_scale_factor,
                  int device_src, void* producer) {
  if (!m || n < 0 || (n > 0 && !frames)) return fail(REVO_ERR_INVALID_ARG, "bad argument");
  if (n == 0) return REVO_OK;
  if (depth_is_u16 && !(depth_scale_factor > 0)) return fail(REVO_ERR_INVALID_ARG, "depth_scale_factor must be > 0");
  if (n > m->S) return fail(REVO_ERR_INVALID_ARG, "more frames than streams");
  std::vector<char> seen(m->S, 0);
  for (int i = 0; i < n; ++i) {
    const revo_stream_frame& f = frames[i];
    if (!stream_ok(m, f.stream)) return fail(REVO_ERR_INVALID_ARG, "stream out of range");
    if (seen[f.stream]) return fail(REVO_ERR_INVALID_ARG, "two frames for one stream in one submit");
    seen[f.stream] = 1;
    if (!f.bgr || !f.depth) return fail(REVO_ERR_INVALID_ARG, "null image pointer");
  }
  // strides are checked here, before anything is uploaded: a failed submit leaves every queue as it was
  float cam[6];
  { const int rc = revo_ctx_camera(m->ctx, 0, cam); if (rc) return rc; }
  const size_t w = (size_t)cam[4];
  for (int i = 0; i < n; ++i)
    if (frames[i].bgr_stride < w * 3 || frames[i].depth_stride < w * (depth_is_u16 ? 2 : 4))
      return fail(REVO_ERR_INVALID_ARG, "stride smaller than a row");
  if (device_src) {
    const int dev = revo_ctx_device_(m->ctx);
    const size_t esz = depth_is_u16 ? 2 : 4;
    for (int i = 0; i < n; ++i) {
      if (((uintptr_t)frames[i].depth | frames[i].depth_stride) % esz)
        return fail(REVO_ERR_INVALID_ARG, "depth rows not aligned to their element size");
      if (!on_device(frames[i].bgr, dev) || !on_device(frames[i].depth, dev))
        return fail(REVO_ERR_INVALID_ARG, "a frame pointer is not device memory of the context's device");
    }
  }
  for (int i = 0; i < n; ++i)
    if (revo_vo_multi_pending(m, frames[i].stream) >= m->max_queue)
      return fail(REVO_ERR_CAPACITY, "the stream's queue is full: call revo_vo_multi_step first");
  void* set = nullptr;
  const int rc = revo_mdev_submit_(m->dev, n, frames, depth_is_u16, depth_scale_factor, device_src, producer, &set);
  if (rc) return rc;
  for (int i = 0; i < n; ++i) {
    m->st[frames[i].stream].queue.push_back(Ref{set, i, frames[i].timestamp});
    ref_add(m, set);
  }
  return REVO_OK;
}

extern "C" int revo_vo_multi_submit(revo_vo_multi* m, int n, const revo_stream_frame* frames, int depth_is_u16,
                                    double depth_scale_factor) {
  return submit(m, n, frames, depth_is_u16, depth_scale_factor, 0, nullptr);
}

extern "C" int revo_vo_multi_submit_device(revo_vo_multi* m, int n, const revo_stream_frame* frames, int depth_is_u16,
                                           double depth_scale_factor, void* producer_stream) {
  return submit(m, n, frames, depth_is_u16, depth_scale_factor, 1, producer_stream);
}

// One body of the while loop of REVO::start (system.cpp:128-284) for every stream that has work, in revo_vo_track_next's order.
extern "C" int revo_vo_multi_step(revo_vo_multi* m, revo_stream_result* out, int* n_out) {
  if (!m || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n_out) *n_out = 0;
  const M4 I = M4::identity();
  std::vector<MultiTrack> trk;
  std::vector<MultiFrame> promote, clouds;
  std::vector<int> first;  // streams whose first frame becomes their keyframe this step
  int n_res = 0;
  auto report = [&](int s, const M4& pose, int new_kf, double ts) {
    revo_stream_result& r = out[n_res++];
    r.stream = s; r.new_keyframe = new_kf; r.timestamp = ts;
    memcpy(r.pose, pose.m, sizeof(pose.m));
  };
  for (int s = 0; s < m->S; ++s) {
    Stream& x = m->st[s];
    if (x.retrack) {  // the frame whose vote asked for a keyframe, against the new one, initialised with T_NM1_N (system.cpp:217-221)
      MultiTrack t{s, x.cur.set, x.cur.frame, {}, {}, 0};
      memcpy(t.R, x.R, sizeof(t.R)); memcpy(t.T, x.T, sizeof(t.T));
      trk.push_back(t);
      continue;
    }
    if (x.queue.empty()) continue;
    x.cur = x.queue.front();
    x.queue.pop_front();
    if (x.no_frames == 0) {  // system.cpp:151-175: the first frame is the keyframe
      first.push_back(s);
      continue;
    }
    ++x.no_frames;
    MultiTrack t{s, x.cur.set, x.cur.frame, {}, {}, 0};
    memcpy(t.R, x.R, sizeof(t.R)); memcpy(t.T, x.T, sizeof(t.T));
    trk.push_back(t);
  }
  int rc = revo_mdev_track_(m->dev, (int)trk.size(), trk.data());
  if (rc) return rc;
  // one k_pair_info launch behind the grid, at the poses it wrote, for every stream it tracked (the records of those that
  // report nothing this step -- a vote asking for a keyframe change -- are dropped below)
  std::vector<revo_pair_info> infos(m->pair_info ? trk.size() : 0);
  if (m->pair_info && (rc = revo_mdev_pair_info_enqueue_(m->dev, (int)trk.size()))) return rc;
  // the votes of the streams that tracked a new frame (a re-track's second vote is discarded by revo_vo: not run here)
  std::vector<MultiVote> votes;
  std::vector<M4> T_KF_N(trk.size()), world(trk.size());
  for (size_t k = 0; k < trk.size(); ++k) {
    Stream& x = m->st[trk[k].stream];
    memcpy(x.R, trk[k].R, sizeof(x.R)); memcpy(x.T, trk[k].T, sizeof(x.T));
    T_KF_N[k] = from_RT(x.R, x.T);
    world[k] = mul(x.T_w_kf, T_KF_N[k]);
    if (!x.retrack) {
      MultiVote v{trk[k].stream, trk[k].set, trk[k].frame, {}, 0};
      memcpy(v.T_w_curr, world[k].m, sizeof(v.T_w_curr));
      votes.push_back(v);
    }
  }
  if ((rc = revo_mdev_vote_(m->dev, (int)votes.size(), votes.data()))) return rc;
  if (m->pair_info && (rc = revo_mdev_pair_info_wait_(m->dev, (int)trk.size(), infos.data()))) return rc;
  size_t vk = 0;
  for (size_t k = 0; k < trk.size(); ++k) {
    const int s = trk[k].stream;
    Stream& x = m->st[s];
    int new_kf = 0;
    if (x.retrack) {
      x.retrack = false;
      x.just_added_kf = true;
      new_kf = 1;
    } else {
      const int status = votes[vk++].status;
      if (status == REVO_TRACKER_STATE_NEW_KF && !x.just_added_kf) {  // system.cpp:203-241, the re-track deferred to the next step
        x.T_w_kf = x.last.world();  // kfPyr->setTwf(mPoseGraph.back().getCurrToWorld())
        x.kf_ts = x.prev.ts;
        promote.push_back(MultiFrame{s, x.prev.set, x.prev.frame, {}, x.prev.ts});
        memcpy(promote.back().T_w, x.T_w_kf.m, sizeof(x.T_w_kf.m));
        x.last = Pose{I, x.T_w_kf};  // mPoseGraph.back().setKfFrame(kfPyr)
        ++x.n_keyframes;
        revo_mdev_clear_past_(m->dev, s, -1);  // clearPastLists: the newest N_FRAMES_HIST_VOTING stay
        to_RT(x.T_NM1_N, x.R, x.T);
        x.retrack = true;
        continue;
      }
      x.just_added_kf = false;
    }
    x.before_last = x.last;
    x.last = Pose{T_KF_N[k], x.T_w_kf};  // mPoseGraph.push_back(Pose(T_KF_N, ts, kfPyr))
    MultiFrame cl{s, x.cur.set, x.cur.frame, {}, x.cur.ts};
    memcpy(cl.T_w, world[k].m, sizeof(cl.T_w));
    clouds.push_back(cl);
    // T_NM1_N = graph[size-2].T_N_W() * graph.back().T_W_N(); T_init = back().T_kf_N() * T_NM1_N (system.cpp:267-271)
    const M4 w1 = x.last.world();
    x.T_NM1_N = mul(inverse(x.before_last.world()), w1);
    to_RT(mul(x.last.T_kf_curr, x.T_NM1_N), x.R, x.T);
    report(s, w1, new_kf, x.cur.ts);
    if (m->pair_info) { x.info = infos[k]; x.info_kf_ts = x.kf_ts; x.has_info = true; }
    if (x.has_prev) ref_drop(m, x.prev.set);  // prevPyr = currPyr
    x.prev = x.cur;
    x.has_prev = true;
  }
  for (int s : first) {
    Stream& x = m->st[s];
    x.T_w_kf = I;
    x.kf_ts = x.cur.ts;
    if (m->pair_info) {  // the first frame is its own keyframe: no evaluation (flags bit0), identity pose
      memset(&x.info, 0, sizeof(x.info));
      x.info.flags = 1;
      x.info.R[0] = x.info.R[4] = x.info.R[8] = 1.f;
      x.info_kf_ts = x.cur.ts;
      x.has_info = true;
    }
    promote.push_back(MultiFrame{s, x.cur.set, x.cur.frame, {}, x.cur.ts});
    memcpy(promote.back().T_w, I.m, sizeof(I.m));
    x.last = Pose{I, I};
    ++x.n_keyframes;
    ++x.no_frames;
    x.just_added_kf = true;
    MultiFrame cl{s, x.cur.set, x.cur.frame, {}, x.cur.ts};
    memcpy(cl.T_w, I.m, sizeof(cl.T_w));
    clouds.push_back(cl);
    report(s, I, 1, x.cur.ts);
    x.prev = x.cur;
    x.has_prev = true;
  }
  if ((rc = revo_mdev_promote_(m->dev, (int)promote.size(), promote.data()))) return rc;
  {  // MapDrawer's cloud of each new keyframe (system.cpp:165-167,235-237): one launch for every attached map, on the tracker
     // stream behind the promotion's copy and distance transforms; the next promotion into a slot queues behind it
    std::vector<revo_map*> maps;
    std::vector<revo_pyr*> kfs;
    std::vector<float> T;
    for (const MultiFrame& f : promote)
      if (m->maps[f.stream]) {
        maps.push_back(m->maps[f.stream]);
        kfs.push_back(revo_mdev_keyframe_(m->dev, f.stream));
        T.insert(T.end(), f.T_w, f.T_w + 16);
      }
    if (!maps.empty() && (rc = revo_map_integrate_views_(m->map_stage, (int)maps.size(), maps.data(), kfs.data(), T.data())))
      return rc;
  }
  surfaces_step(m, promote);  // the surfaces of the promoted streams: tracked and fused right behind the map integration
  if ((rc = revo_mdev_add_clouds_(m->dev, (int)clouds.size(), clouds.data()))) return rc;
  // results come out in stream order
  std::vector<revo_stream_result> tmp(out, out + n_res);
  std::sort(tmp.begin(), tmp.end(), [](const revo_stream_result& a, const revo_stream_result& b) { return a.stream < b.stream; });
  std::copy(tmp.begin(), tmp.end(), out);
  if (n_out) *n_out = n_res;
  return REVO_OK;
}
