// revo_host.hip -- host side of librevo_hip.so: the C ABI of include/revo_hip.h.
//
// Owns HBM (one blob per FrameSet, pooled), the per-context HIP streams, and the
// sequencing of the kernels in revo_pyramid.hip / revo_track.hip.  No torch, no
// Eigen, no OpenCV types cross this boundary.  This unit: errors, defaults, geometry, the resident gate, the host's waits,
// the context and the FrameSets; the handles built on them are revo_frame.hip (single-frame pyramids), revo_single.hip
// (single-pair tracker, vote, past clouds), revo_batch.hip, revo_pairs.hip and revo_mdev.hip, all over revo_host_impl.h.
#include "revo_host_impl.h"

// ------------------------------------------------------------------ errors --
static thread_local std::string g_err;
extern "C" const char* revo_last_error(void) { return g_err.c_str(); }
extern "C" const char* revo_version(void) { return "0.1.0 gfx950"; }
extern "C" void revo_set_error_(const char* msg) { g_err = msg ? msg : ""; }  // fail() of revo_internal.h: one string per thread

// ---------------------------------------------------------------- defaults --
extern "C" void revo_pyr_settings_default(revo_pyr_settings* s) {  // config/dataset_tum1.yaml
  memset(s, 0, sizeof(*s));
  s->width = 640; s->height = 480;
  s->fx = 517.306408f; s->fy = 516.469215f; s->cx = 318.643040f; s->cy = 255.313989f;
  s->pyr_min_lvl = 2; s->pyr_max_lvl = 0;
  s->canny_threshold1 = 150; s->canny_threshold2 = 100;
  s->depth_min = 0.1f; s->depth_max = 5.2f;
  s->use_edge_hist = 1; s->n_percentage = 0.3f;
  s->hist_patch[0] = 20; s->hist_patch[1] = 10; s->hist_patch[2] = 5;  // imgpyramidrgbd.cpp:50
}
extern "C" void revo_opt_settings_default(revo_opt_settings* s) {  // optimizer.h:46-85
  memset(s, 0, sizeof(*s));
  s->lambda_success_fac = 0.5f; s->lambda_fail_fac = 2.0f;
  const float ed[6] = {30, 20, 10, 5, 5, 5};
  for (int i = 0; i < REVO_L; ++i) {
    s->lambda_initial[i] = 0.f; s->step_size_min[i] = 1e-16f; s->convergence_eps[i] = 0.999f;
    s->max_its_per_lvl[i] = 100; s->edge_distance_lvl[i] = ed[i];
  }
  s->huber_edge = 0.3f;
  s->use_edge_filter = 1;  // config/revo_settings.yaml:11
}
extern "C" void revo_tracker_settings_default(revo_tracker_settings* s) {  // config/revo_settings.yaml:9-12
  s->check_tracking_results = 1; s->check_init_values = 1; s->n_frames_hist_voting = 3;
  s->histogram_level = 2;  // tracker.cpp:229
}

// ---------------------------------------------------------------- geometry --
static int build_geom(const revo_pyr_settings& s, PyrGeom* g, std::string* why) {
  memset(g, 0, sizeof(*g));
  g->fstride = 1;
  const int L = s.pyr_min_lvl - s.pyr_max_lvl + 1;  // camerapyr.h:68-71
  if (s.pyr_max_lvl != 0) { *why = "pyr_max_lvl must be 0 (the reference indexes per-level vectors by level)"; return -1; }
  if (L < 1 || L > REVO_L) { *why = "1..6 pyramid levels supported"; return -1; }
  // the reference truncates whatever it is given (camerapyr.h:98-103); here: up to 2048 x 2048 (the EDT's LDS rows, the
  // 64 x 32-row chunks of the column walks) with at most 2048 tiles of 32 x 32 pixels per level (k_tile_count)
  if (s.width <= 0 || s.height <= 0 || s.width > REVO_MAX_WIDTH || s.height > 2048 ||
      ((s.width + 31) / 32) * ((s.height + 31) / 32) > 2048) {
    *why = "image size must be within 2048 x 2048 and 2048 tiles of 32 x 32 pixels (1920 x 1080 fits, 2048 x 1536 does not)"; return -1;
  }
  if (s.width % (4 << (L - 1)) || s.height % (1 << (L - 1))) {
    *why = "width must be a multiple of 4*2^(levels-1) and height of 2^(levels-1)"; return -1;
  }
  g->n_levels = L;
  { const char* e = getenv("REVO_HYST_BANDED"); g->hyst_force = (e && *e) ? (*e != '0' ? 1 : 0) : -1; }
  // mixed hysteresis (round 6): where a level fits one workgroup, the frames whose level 0 has at least this many weak runs (the
  // launch lasts as long as the heaviest of them) are cut into bands inside the same launch.  Bit-exact and OFF by default (0):
  // the band / seam / output passes of the heavy frames cost more than the single workgroup they replace
  g->hyst_heavy_runs = env_int("REVO_HYST_HEAVY_RUNS", 0, 0, 1 << 30);  // measured and not kept as the default: profiles/r06_ab_mixed_hyst.txt
  g->depth_min = s.depth_min; g->depth_max = s.depth_max;
  // cv::Canny with L2gradient: low/high swapped if needed, squared (imgpyramidrgbd.cpp:184)
  double lo = s.canny_threshold1, hi = s.canny_threshold2;
  if (lo > hi) std::swap(lo, hi);
  lo = std::min(32767.0, lo); hi = std::min(32767.0, hi);
  if (lo > 0) lo *= lo;
  if (hi > 0) hi *= hi;
  g->canny_low = (int)std::floor(lo); g->canny_high = (int)std::floor(hi);
  g->use_edge_hist = s.use_edge_hist; g->n_percentage = s.n_percentage;
  int tile = 0, pix = 0, row = 0, col = 0, cc = 0, tiles32 = 0, bands = 0;
  bool bands_fit = true;
  for (int l = 0; l < L; ++l) {
    LevelGeom& v = g->lv[l];
    const float scale = 1.0f / (float)std::pow(2, l);  // camerapyr.h:142
    if (l == 0) { v.fx = s.fx; v.fy = s.fy; v.cx = s.cx; v.cy = s.cy; v.w = s.width; v.h = s.height; }
    else {
      v.fx = s.fx * scale; v.fy = s.fy * scale; v.cx = s.cx * scale; v.cy = s.cy * scale;
      v.w = (int)((float)s.width * scale); v.h = (int)((float)s.height * scale);
    }
    v.npix = v.w * v.h;
    if (v.npix % 16) { *why = "every level must have a multiple of 16 pixels"; return -1; }
    v.patch = s.hist_patch[l] > 0 ? s.hist_patch[l] : 0;
    if (v.patch > 0) {
      v.hist_w = v.w / v.patch; v.hist_h = v.h / v.patch;
      if (v.hist_w < 1 || v.hist_h < 1 || v.hist_w > 128) { *why = "hist_patch out of range for this level size"; return -1; }
    }
    g->fill_thr[l] = (double)(v.patch * v.patch) * 0.05;  // imgpyramidrgbd.cpp:133
    v.chunk_rows = 32; v.nchunk = (v.h + 31) / 32;
    v.wpr = (v.w + 31) / 32;
    v.nms_block_base = tile; tile += (8 * v.wpr * ((v.h + NMS_ROWS - 1) / NMS_ROWS) + 255) / 256;
    // (a level whose edge bitmap does not fit one workgroup's LDS takes the banded hysteresis; its last resort keeps the bitmap
    // in the scratch plane: launch_hyst)
    v.pix_base = pix; pix += v.npix;
    v.edt_rows = std::max(1, EDT_ROW_PX / v.w);
    v.edt_block_base = row; row += (v.h + v.edt_rows - 1) / v.edt_rows;
    v.strip_base = col; col += (v.w + 63) / 64;
    v.cc_base = cc; cc += v.w * v.nchunk;
    tiles32 += v.wpr * v.nchunk;
    // banded hysteresis: bands of about 2400 bitmap words, heights a multiple of the histogram patch and of 4 rows
    {
      int unit = v.patch > 0 ? v.patch : 4;
      while (unit % 4) unit *= 2;
      int rows = (env_int("REVO_HYST_BAND_WORDS", 2400, 64, 1 << 20) / v.wpr) / unit * unit;
      if (rows < unit) rows = unit;
      if (rows >= v.h) rows = v.h;
      if ((v.h + rows - 1) / rows > 32) rows = ((v.h + 31) / 32 + unit - 1) / unit * unit;  // k_hyst_seam holds at most 32 bands' flags
      v.band_rows = rows;
      v.nbands = (v.h + rows - 1) / rows;
      v.band_base = bands; bands += v.nbands;
      if (v.nbands > 1) g->any_banded = 1;
      // a band's bitmaps (weak words, 16-bit id bases, edge rows + halo) must leave room for tables in the 64 KB of a band workgroup
      const size_t nwb = (size_t)rows * v.wpr;
      if (nwb + (nwb + 2) / 2 + (size_t)(rows + 2) * v.wpr + 2 + 256 > 16384) bands_fit = false;
    }
  }
  g->total_tiles = tiles32;
  g->total_bands = bands_fit ? bands : 0;  // 0: no banded hysteresis for this geometry (k_hyst alone, as in round 2)
  for (int l = 1; l < L; ++l)  // fillInEdges' gate (imgpyramidrgbd.cpp:188-195 + the patch sizes that exist)
    g->lv[l].has_orig = (s.use_edge_hist && g->lv[l].patch > 0 && g->lv[l - 1].patch > 0) ? 1 : 0;
  g->total_nms_blocks = tile; g->total_pix = pix; g->total_edt_blocks = row; g->total_strips = col; g->total_cc = cc;
  return 0;
}

static void build_track_params(const revo_ctx* c, TrackParams* t) {
  memset(t, 0, sizeof(*t));
  t->pyr_min_lvl = c->ps.pyr_min_lvl; t->pyr_max_lvl = c->ps.pyr_max_lvl;
  t->lvl_begin = c->ps.pyr_min_lvl; t->lvl_end = c->ps.pyr_max_lvl;
  t->check_init = c->ts.check_init_values;
  t->lambda_success_fac = c->os.lambda_success_fac; t->lambda_fail_fac = c->os.lambda_fail_fac;
  for (int i = 0; i < REVO_L; ++i) {
    t->lambda_initial[i] = c->os.lambda_initial[i]; t->step_size_min[i] = c->os.step_size_min[i];
    t->convergence_eps[i] = c->os.convergence_eps[i]; t->max_its[i] = c->os.max_its_per_lvl[i];
    t->edge_distance[i] = c->os.edge_distance_lvl[i];
  }
  t->huber_edge = c->os.huber_edge; t->use_edge_filter = c->os.use_edge_filter;
  // speculation depth per level: REVO_TRACK_KSPEC = one digit for all levels or one digit per level (finest first)
  {
    const char* e = getenv("REVO_TRACK_KSPEC");
    const size_t n = e ? strlen(e) : 0;
    for (int i = 0; i < REVO_L; ++i) {
      // default: the two finest levels evaluate one retry next to the candidate (their points are what a pass costs),
      // the coarse ones three (profiles/r02_single_stream_sweep.txt)
      int k = i < 2 ? 2 : TRACK_KMAX;
      if (n == 1) k = e[0] - '0'; else if (n > 1) k = e[std::min<size_t>(i, n - 1)] - '0';
      t->kspec[i] = std::max(1, std::min(TRACK_KMAX, k));
    }
  }
  t->redundant_n = env_int("REVO_TRACK_REDUNDANT_BATCH", 400, 0, 1 << 30);
  for (int l = 0; l < c->geom.n_levels; ++l) {
    const LevelGeom& v = c->geom.lv[l];
    t->cam[l].fx = v.fx; t->cam[l].fy = v.fy; t->cam[l].cx = v.cx; t->cam[l].cy = v.cy; t->cam[l].w = v.w; t->cam[l].h = v.h;
  }
}

// Workgroups per frame-pair.  Every member of every cluster must be resident at once (they exchange partial sums inside
// the launch).  A batch grid takes HALF of what the device can hold for this kernel: the resident gate keeps the tracker
// grids of two consecutive batches in flight (the second fills the CUs the first one's finished pairs free), and two
// half-chip grids are resident together, whereas a 75 % grid (round 2) leaves the next one waiting with workgroups that
// hold CUs and spin (measured, 32 pairs, three batches in rotation: cluster 6 -> 68.5 k, 4 -> 78.2 k, 3 -> 79.2 k frames/s;
// a launch alone: 0.39 / 0.45 / 0.50 ms).  The in-kernel wait is bounded as a second line of defence.
// Tracker grids the resident gate keeps in flight per device (REVO_TRACK_DEPTH, default 2; 1 = one at a time, the round-2
// behaviour; up to 4 for experiments with small clusters: workgroup-time per pair falls with the cluster size -- the
// exchange and the decision are paid by every member -- but a grid of small clusters only fills a fraction of the chip).
static int env_track_depth() {
  const char* e = getenv("REVO_TRACK_SERIAL");
  if (e && *e && *e != '0') return 1;
  return env_int("REVO_TRACK_DEPTH", 2, 1, 4);
}
int pick_cluster(const revo_ctx* c, int n_pairs) {
  const int resident = c->num_cus * c->blocks_per_cu;
  // a batch grid takes 1/depth of what the device holds: `depth` grids are resident together
  // (depth 1 = one grid at a time: the round-2 shape, 75 % of the chip)
  const int depth = c->knobs.track_depth;
  const int share = n_pairs == 1 || depth == 1 ? (int)(0.75 * resident) : resident / depth;
  int cl = share / std::max(1, n_pairs);
  // a single pair: its members share one XCD (blockIdx % 8), i.e. 32 CUs -- 16 workgroups leave half of them
  // to the build kernels of the next frame
  if (n_pairs == 1) cl = std::min(cl, 16);
  if (cl > TRACK_MAX_CLUSTER) cl = TRACK_MAX_CLUSTER;
  {  // tuning knobs: REVO_TRACK_CLUSTER_ONE (per context), REVO_TRACK_CLUSTER (read when a batch is created)
    const int want = n_pairs == 1 ? c->knobs.cluster_one : env_int("REVO_TRACK_CLUSTER", 0, 0, TRACK_MAX_CLUSTER);
    const int hard = std::min(TRACK_MAX_CLUSTER, resident / std::max(1, n_pairs));
    if (want >= 1) cl = std::min(want, std::max(1, hard));
  }
  if (cl < 1) cl = 1;
  return cl;
}

// Tracker launches of one device are ordered by a RESIDENT GATE.  A cluster's workgroups exchange partial sums inside
// the launch, so two tracker grids must never be PARTIALLY resident at the same time (each would wait for members the
// other keeps off the CUs until the bounded spin gives up with flag 8).  Round 2 serialised the grids completely (launch
// n waited for launch n-1 to finish) -- and a launch lasts as long as its slowest pair (455 us against a mean of 294 us
// per pair), so a third of the tracker's CU time idled behind the tail.  Now launch n
//   * waits for launch n-2 to COMPLETE (at most two tracker grids are ever in flight), and
//   * waits, through a one-wave gate kernel in front of it, until every workgroup of launch n-1 has STARTED
//     (k_track counts its workgroups into a per-device census counter as they start).  A started workgroup holds its CU
//     until it exits, so from then on launch n-1 is complete on the chip and makes progress whatever else arrives;
//     launch n's workgroups fill the CUs that n-1's finished pairs free, and are themselves all resident once n-1 has
//     drained (192 <= 256 CUs; build kernels finish in finite time).  By induction the older of the two grids is always
//     fully resident: no cyclic wait.
// REVO_TRACK_DEPTH=n (1..4, default 2; read per context) sets how many grids may be in flight (launch n waits for launch
// n-depth to complete); REVO_TRACK_SERIAL=1 = depth 1 = the round-2 behaviour.  The chain itself is per DEVICE (the census
// counter is) and keeps the events of the last TRACK_MAX_DEPTH launches, so contexts with different depths may share a device:
// each launch applies its own context's depth.  (Other PROCESSES sharing the GPU are outside this library's reach: the
// bounded spin + flag 8 + REVO_ERR_HIP remain the answer there.)
#define TRACK_MAX_DEPTH 4
struct TrackChain {
  std::mutex mu;
  hipEvent_t ev[TRACK_MAX_DEPTH] = {};   // completion of the last TRACK_MAX_DEPTH launches (ring, slot = launch index % 4)
  hipStream_t st[TRACK_MAX_DEPTH] = {};
  bool has[TRACK_MAX_DEPTH] = {};
  unsigned long long n = 0;      // launches so far
  int depth_seen = 0;            // the depth of the first launch; `mixed` once a launch with another depth arrived
  bool mixed = false;
  unsigned* d_resident = nullptr;
  unsigned started_total = 0;    // workgroups of all launches enqueued so far (the census value once they have all started)
};
static TrackChain g_chain[64];
// launch(f, d_resident): enqueues the tracker grid on s and returns its workgroup count (chained_track_launch, revo_host_impl.h)
int chained_track_launch_(int device, int depth, hipStream_t s, int (*launch)(void* f, unsigned* d_resident), void* f) {
  TrackChain& ch = g_chain[device & 63];
  std::lock_guard<std::mutex> lk(ch.mu);
  depth = depth < 1 ? 1 : (depth > TRACK_MAX_DEPTH ? TRACK_MAX_DEPTH : depth);
  if (!ch.ev[0]) {
    for (int i = 0; i < TRACK_MAX_DEPTH; ++i) TRY(event_create(&ch.ev[i]));  // (they live as long as the process)
    HIPCHECK(hipMalloc((void**)&ch.d_resident, 2 * sizeof(unsigned)));  // [0] census, [1] gates that timed out
    // (hipMemset on device memory is asynchronous to the host and runs on the NULL stream; the tracker streams are non-blocking
    // streams, so the first grid could count itself into the census BEFORE the zeroing lands: finish it here, once per device)
    HIPCHECK(hipMemset(ch.d_resident, 0, 2 * sizeof(unsigned)));
    HIPCHECK(hipDeviceSynchronize());
  }
  // launch n-depth must be COMPLETE (at most `depth` grids in flight; with one depth in use every older launch completed
  // before it by induction -- only when contexts with DIFFERENT depths share the device are the older ring slots waited for
  // as well), launch n-1 must be fully RESIDENT: only the newest grid is ever partially on the chip, every older one holds
  // all its CUs and finishes whatever arrives -- no cyclic wait at any depth.  With depth 1 the two coincide: one grid at a time.
  if (!ch.depth_seen) ch.depth_seen = depth;
  if (depth != ch.depth_seen) ch.mixed = true;
  for (int back = depth; back <= (ch.mixed ? TRACK_MAX_DEPTH : depth); ++back) {
    if ((unsigned long long)back > ch.n) break;
    const int slot = (int)((ch.n - back) % TRACK_MAX_DEPTH);
    if (ch.has[slot] && ch.st[slot] != s) HIPCHECK(hipStreamWaitEvent(s, ch.ev[slot], 0));
  }
  const int prev = (int)((ch.n + TRACK_MAX_DEPTH - 1) % TRACK_MAX_DEPTH), cur = (int)(ch.n % TRACK_MAX_DEPTH);
  if (depth > 1 && ch.n > 0 && ch.has[prev] && ch.st[prev] != s) launch_track_gate(ch.d_resident, ch.started_total, s);
  const int n_wg = launch(f, ch.d_resident);
  HIPCHECK(hipGetLastError());              // (a refused launch adds nothing to the census: the next gate must not wait for it)
  ch.started_total += (unsigned)n_wg;
  HIPCHECK(hipEventRecord(ch.ev[cur], s));
  ch.has[cur] = true;
  ch.st[cur] = s;
  ch.n += 1;
  return REVO_OK;
}
// how many resident gates of this device gave up waiting so far (0 in a healthy process); -1: no tracker launch yet
extern "C" int revo_debug_gate_timeouts_(int device) {
  TrackChain& ch = g_chain[device & 63];
  std::lock_guard<std::mutex> lk(ch.mu);
  if (!ch.d_resident) return -1;
  unsigned v = 0;
  if (hipMemcpy(&v, ch.d_resident + 1, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return -2;
  return (int)v;
}
// diagnostics: out3 = {census (workgroups that have started), gates that timed out, workgroups of all launches enqueued so far}.
// After hipDeviceSynchronize census == enqueued in a healthy process.
extern "C" int revo_debug_census_(int device, unsigned out3[3]) {
  TrackChain& ch = g_chain[device & 63];
  std::lock_guard<std::mutex> lk(ch.mu);
  if (!ch.d_resident || !out3) return -1;
  if (hipMemcpy(out3, ch.d_resident, 2 * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return -2;
  out3[2] = ch.started_total;
  return 0;
}
// sized for the larger of the two tracker layouts: the exact-sums instantiation may run on any mailbox
// --------------------------------------------------------------- FrameSets --
// host_staging = false: device-side input planes only (inputs go straight from the caller's rows to the device)
int frameset_create(revo_ctx* c, int B, bool with_staging, FrameSet** out, bool host_staging) {
  const PyrGeom& g = c->geom;
  Partial<FrameSet> fs(new FrameSet());
  fs->B = B;
  // pass 1: size, pass 2: carve
  for (int pass = 0; pass < 2; ++pass) {
    size_t off = 0;
    auto take = [&](size_t bytes) -> void* {
      void* p = pass ? (void*)(fs->blob + off) : nullptr;
      off = align_up(off + bytes, 256);
      return p;
    };
    for (int l = 0; l < g.n_levels; ++l) {
      const LevelGeom& v = g.lv[l];
      const size_t n = (size_t)v.npix * B;
      fs->p.gray[l] = (uint8_t*)take(n);
      fs->p.depth[l] = (float*)take(n * 4);
      fs->p.cs[l] = (uint2*)take((size_t)v.h * v.wpr * 8 * B);
      fs->p.edges[l] = (uint8_t*)take(n);
      fs->p.edges_orig[l] = (uint8_t*)take(n);
      fs->p.scratch[l] = (int*)take(n * 4);
      fs->p.pts[l] = (float4*)take(n * 16);
      fs->p.pts_trk[l] = (float4*)take(n * 16);
      fs->p.dt[l] = (float*)take(n * 4);
      fs->p.table[l] = (float4*)take(n * 16);
      fs->p.hist[l] = (uint8_t*)take((size_t)std::max(1, v.hist_w * v.hist_h) * B);
      fs->p.chunk[l] = (int*)take((size_t)v.w * v.nchunk * B * 4);
      fs->p.cmask[l] = (unsigned*)take((size_t)v.w * v.nchunk * B * 4);
      fs->p.vb[l] = (uint8_t*)take((n + 7) / 8);
      fs->p.ebits[l] = (uint32_t*)take((size_t)v.h * v.wpr * 4 * B);
      if (B > 1 && l < g.n_levels - 1) {  // (batches only: the single-frame API builds its depth pyramid in front of Canny)
        fs->p.stage[l] = (float*)take(n * 4);
        fs->p.epre[l] = (unsigned short*)take((size_t)v.h * v.wpr * 2 * B);
      }
    }
    fs->own_depth0 = fs->p.depth[0];
    fs->p.npts = (int*)take(sizeof(int) * REVO_L * B);
    fs->p.hist_nz = (int*)take(sizeof(int) * REVO_L * B);
    fs->p.strip_tot = (int*)take(sizeof(int) * (size_t)g.total_strips * B);
    fs->p.tile_base = (int*)take(sizeof(int) * (size_t)g.total_tiles * B);
    fs->p.need_full = (int*)take(sizeof(int) * REVO_L * B);
    fs->p.hyst_heavy = (int*)take(sizeof(int) * B);
    fs->p.stage_base = (int*)take(sizeof(int) * (size_t)g.total_tiles * B);
    if (with_staging) {
      fs->d_bgr = (uint8_t*)take((size_t)g.lv[0].npix * 3 * B);
      fs->d_depth = (float*)take((size_t)g.lv[0].npix * 4 * B);
    }
    if (!pass) {
      fs->blob_bytes = off;
      hipError_t e = hipMalloc((void**)&fs->blob.p, off);
      if (e != hipSuccess) return fail(REVO_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
  }
  if (with_staging && host_staging) {
    TRY(fs->h_bgr.alloc((size_t)g.lv[0].npix * 3 * B));
    TRY(fs->h_depth.alloc((size_t)g.lv[0].npix * B));
  }
  for (StreamMark* m : {&fs->ready, &fs->free_trk, &fs->free_vote, &fs->edt, &fs->ref, &fs->ebytes}) TRY(m->create());
  // counts start at zero so an accessor on a not-yet-built pyramid is well defined
  hipMemsetAsync(fs->p.npts, 0, sizeof(int) * REVO_L * B, c->stream);
  HIPCHECK(hipStreamSynchronize(c->stream));
  *out = fs.release();
  return REVO_OK;
}

// enqueue the full per-frame build (imgpyramidrgbd.cpp:43-96) for all B frames.
// borrow_depth (f32 input only): the level-0 depth plane IS the input buffer -- the reference's level 0 is the input
// image too (imgpyramidrgbd.cpp:62-64), and copying 64 x 1.2 MB per batch was 208 of the 236 MB the first kernel moved.
// The caller guarantees the buffer stays valid and unchanged for as long as the pyramids are used.
// with_points = false: stops after fillInEdges; the caller enqueues launch_tile_points itself (batches run it next to the EDT)
void enqueue_build(revo_ctx* c, FrameSet* fs, const uint8_t* d_bgr, const float* d_depth_f32, const uint16_t* d_depth_u16,
                   float alpha, hipStream_t s, bool borrow_depth, bool with_points, int frame0, int nframes, bool gray_only) {
  PyrGeom g = c->geom;
  g.frame0 = frame0;
  const int B = nframes < 0 ? fs->B : nframes;
  // a batch that defers the end of its build also leaves the byte edge planes to their first reader (ensure_edge_bytes)
  g.edge_bytes_lazy = gray_only ? 1 : 0;
  fs->lazy_edge_bytes = gray_only;
  fs->p.depth[0] = (borrow_depth && d_depth_f32) ? const_cast<float*>(d_depth_f32) : fs->own_depth0;
  launch_gray_depth(g, fs->p, d_bgr, d_depth_f32, d_depth_u16, alpha, B, s);
  // gray_only (batches that defer): the depth half of the pyramid is left to the first consumer with the edge lists
  for (int l = 1; l < g.n_levels; ++l) launch_pyrdown(g, fs->p, l, B, s, gray_only ? 1 : 3);
  launch_canny_nms(g, fs->p, B, s);
  launch_hyst(g, fs->p, B, s);
  launch_fill(g, fs->p, B, s);
  if (with_points) launch_tile_points(g, fs->p, B, s);  // the tracker's (tile-ordered) edge list; the reference's order is built on demand
}

// ------------------------------------------------------------------ context --
extern "C" int revo_ctx_create(int device, const revo_pyr_settings* pyr, const revo_opt_settings* opt,
                               const revo_tracker_settings* trk, revo_ctx** out) {
  if (!pyr || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(REVO_ERR_HIP, "no HIP device: librevo_hip has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(REVO_ERR_INVALID_ARG, "device ordinal out of range");
  HIPCHECK(hipSetDevice(device));
  Partial<revo_ctx> owner(new revo_ctx());  // a failure below frees what exists so far
  revo_ctx* c = owner.get();
  c->device = device;
  c->ps = *pyr;
  c->knobs.track_depth = env_track_depth();
  c->knobs.cluster_one = env_int("REVO_TRACK_CLUSTER_ONE", 0, 0, TRACK_MAX_CLUSTER);
  c->knobs.redundant_one = env_int("REVO_TRACK_REDUNDANT_ONE", 1024, 0, 1 << 30);
  c->knobs.direct_h2d = env_int("REVO_DIRECT_H2D", 1, 0, 1);
  c->knobs.stage_edge_depths = env_int("REVO_STAGE_EDGE_DEPTHS", 0, 0, 1);  // built, bit-exact, 80 MB less traffic per step and 2.6 % SLOWER: off (profiles/r06_ab_stage_edge_depths.txt)
  {
    const char* e1 = getenv("REVO_TRACK_KSPEC_ONE");
    const char* eb = getenv("REVO_TRACK_KSPEC");
    const size_t n1 = e1 ? strlen(e1) : 0;
    c->knobs.kspec_one_set = n1 > 0 || !(eb && *eb);
    for (int i = 0; i < REVO_L; ++i) {
      int k = i < 2 ? 3 : TRACK_KMAX;
      if (n1 == 1) k = e1[0] - '0'; else if (n1 > 1) k = e1[std::min<size_t>(i, n1 - 1)] - '0';
      c->knobs.kspec_one[i] = std::max(1, std::min(TRACK_KMAX, k));
    }
  }
  c->knobs.upload_blocks = env_int("REVO_UPLOAD_BLOCKS", 64, 1, 4096);
  c->knobs.h2d_kernel = env_int("REVO_H2D_KERNEL", 0, 0, 1);
  c->knobs.h2d_max_run_mb = env_int("REVO_H2D_MAX_RUN_MB", 64, 1, 4096);  // (profiles/r06_h2d_run_sizes.txt: 2 / 8 / 24 / 64 MB / unbounded)
  if (opt) c->os = *opt; else revo_opt_settings_default(&c->os);
  if (trk) c->ts = *trk; else revo_tracker_settings_default(&c->ts);
  std::string why;
  if (build_geom(c->ps, &c->geom, &why)) return fail(REVO_ERR_INVALID_ARG, why);
  build_track_params(c, &c->tp);
  TRY(c->stream.create());
  TRY(c->build_stream.create());
  TRY(c->vote_stream.create());
  TRY(c->ev_vote.create());
  TRY(c->h_desc.alloc(1));
  TRY(c->h_res.alloc(3));
  TRY(c->h_seq.alloc(4));
  memset(c->h_seq, 0, sizeof(unsigned) * 4);
  TRY(c->h_eval.alloc(1));
  hipDeviceProp_t prop;
  HIPCHECK(hipGetDeviceProperties(&prop, device));
  c->num_cus = prop.multiProcessorCount;
  c->blocks_per_cu = std::min(track_blocks_per_cu(), 2);
  TRY(c->d_mail.alloc(mail_bytes(1, TRACK_MAX_CLUSTER) / sizeof(unsigned long long)));
  HIPCHECK(hipMemset(c->d_mail, 0, mail_bytes(1, TRACK_MAX_CLUSTER)));
  size_t maxpix = 0;
  for (int l = 0; l < c->geom.n_levels; ++l) maxpix = std::max(maxpix, (size_t)c->geom.lv[l].npix);
  TRY(c->d_marks.alloc(maxpix));
  TRY(c->d_hist8.alloc(8));
  TRY(c->d_vote_done.alloc(1));
  // the vote kernels leave their scratch clean: zero it once
  HIPCHECK(hipMemset(c->d_marks, 0, sizeof(int) * maxpix));
  HIPCHECK(hipMemset(c->d_hist8, 0, sizeof(int) * 8));
  HIPCHECK(hipMemset(c->d_vote_done, 0, sizeof(unsigned)));
  TRY(c->h_hist8.alloc(16));  // hist[4], overlaps[4], sequence word
  memset(c->h_hist8, 0, sizeof(int) * 16);
  HIPCHECK(hipDeviceSynchronize());  // the zeroing above runs on the NULL stream; the context's streams are non-blocking
  *out = owner.release();
  return REVO_OK;
}

// The order is behaviour: nothing is freed before the four streams have drained, and the tracker stream goes last (the
// members' order, revo_host_impl.h).
revo_ctx::~revo_ctx() {
  hipSetDevice(device);
  for (hipStream_t s : {(hipStream_t)build_stream, (hipStream_t)stream, (hipStream_t)vote_stream, (hipStream_t)frame_copy_stream})
    if (s) (void)hipStreamSynchronize(s);
  for (auto& p : past) past_free(p);
  for (auto& p : past_pool) past_free(p);
  for (FrameSet* fs : pool) delete fs;
}
void ctx_ref(revo_ctx* c) { c->refs.fetch_add(1); }
void ctx_unref(revo_ctx* c) { if (c->refs.fetch_sub(1) == 1) HandleDelete()(c); }
extern "C" void revo_ctx_destroy(revo_ctx* c) {
  if (!c) return;
  pairs_jobs_release(c);  // the job slots hold batches, and batches hold the context
  ctx_unref(c);
}
// Single-frame FrameSets (20 MB of HBM + 2 MB of pinned staging each) are pooled, but the pool only grew on demand: the
// first full-length run of a sequential driver paid a hipMalloc + hipHostMalloc per new frame in flight (bench r02:
// first run 5x slower than the rest).  A driver that knows its queue depth reserves them up front.
extern "C" int revo_ctx_reserve_framesets_(revo_ctx* c, int total) {
  if (!c) return fail(REVO_ERR_INVALID_ARG, "null context");
  HIPCHECK(hipSetDevice(c->device));
  for (;;) {
    {
      std::lock_guard<std::mutex> lk(c->mu);
      if (c->framesets_created >= total) return REVO_OK;
      c->framesets_created += 1;
    }
    FrameSet* fs = nullptr;
    const int rc = frameset_create(c, 1, true, &fs);
    std::lock_guard<std::mutex> lk(c->mu);
    if (rc) { c->framesets_created -= 1; return rc; }
    c->pool.push_back(fs);
  }
}
extern "C" int revo_ctx_device_(const revo_ctx* c) { return c ? c->device : -1; }
// used by revo_vo.hip / revo_pipeline.hip
extern "C" void revo_ctx_retain_(revo_ctx* c) { if (c) ctx_ref(c); }
extern "C" void revo_ctx_release_(revo_ctx* c) { if (c) ctx_unref(c); }

extern "C" int revo_ctx_set_tracker(revo_ctx* c, const revo_opt_settings* opt, const revo_tracker_settings* trk) {
  if (!c) return fail(REVO_ERR_INVALID_ARG, "null context");
  std::lock_guard<std::mutex> lk(c->mu);
  if (opt) c->os = *opt;
  if (trk) c->ts = *trk;
  const int exact = c->tp.exact_sums;  // not a tracker setting: it stays as revo_ctx_set_exact_sums left it
  build_track_params(c, &c->tp);
  c->tp.exact_sums = exact;
  // a new TrackerNew starts with empty past lists (tracker.h:92-95): the clouds an earlier tracker on this context added must
  // not vote for this one (stream-ordered reuse of the buffers, as in revo_tracker_clear_past)
  while (!c->past.empty()) { c->past_pool.push_back(c->past.front()); c->past.pop_front(); }
  return REVO_OK;
}

extern "C" int revo_ctx_histogram_level(const revo_ctx* c) { return c ? c->ts.histogram_level : -1; }

// Exact-sums mode: every tracker launch takes the instantiation from the TrackParams it copies, so the flag applies
// to the next launch of any path of this context; a revo_vo_multi handle keeps the value of its creation.
extern "C" int revo_ctx_set_exact_sums(revo_ctx* c, int on) {
  if (!c) return fail(REVO_ERR_INVALID_ARG, "null context");
  std::lock_guard<std::mutex> lk(c->mu);
  c->tp.exact_sums = on ? 1 : 0;
  return REVO_OK;
}
extern "C" int revo_ctx_exact_sums(const revo_ctx* c) { return c ? c->tp.exact_sums : -1; }

extern "C" int revo_ctx_camera(const revo_ctx* c, int lvl, float out6[6]) {
  if (!c || !out6) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (lvl < 0 || lvl >= c->geom.n_levels) return fail(REVO_ERR_LEVEL, "level out of range");
  const LevelGeom& v = c->geom.lv[lvl];
  out6[0] = v.fx; out6[1] = v.fy; out6[2] = v.cx; out6[3] = v.cy; out6[4] = (float)v.w; out6[5] = (float)v.h;
  return REVO_OK;
}

// ------------------------------------------- the deferred end of a batch build --
// The depth half + edge lists of the frames f0, f0 + fstride, ... (count frames)
static void enqueue_list_side(revo_ctx* c, FrameSet* fs, int f0, int fstride, int count, hipStream_t s) {
  // The depth half of the pyramid goes in front of the edge lists (nothing on the build stream reads the coarser depth levels
  // or the validity bits: they feed the edge lists only).  The edges are final by now, so the depth pass -- which streams every
  // depth of a level anyway -- can also leave the depths of the level's EDGE pixels behind, compact and in list order
  // (k_edge_prefix tells it where): the edge-list write then reads ~10 MB of staged depths instead of every 128-byte line of
  // the depth planes that holds an edge pixel (~100 MB per 64-frame batch).  Measured (profiles/r06_ab_stage_edge_depths.txt): k_pts_tiles
  // moves 61 MB instead of 141 (1.09x its algorithmic bytes), the step 72 MB less -- and is 2.6 % SLOWER: 2.3 M scattered
  // 4-byte stores and the prefix kernel cost the depth pass more time than the sparse line reads they replace, and no kernel
  // of this chain is bandwidth-bound.  Bit-exact, OFF by default (REVO_STAGE_EDGE_DEPTHS=1 turns it on).
  PyrGeom gp = c->geom;
  gp.frame0 = f0; gp.fstride = fstride;
  const bool stage = c->knobs.stage_edge_depths && fs->p.stage[0] != nullptr && c->geom.n_levels > 1;
  if (stage) launch_edge_prefix(gp, fs->p, count, s);
  for (int l = 1; l < c->geom.n_levels; ++l) launch_pyrdown(gp, fs->p, l, count, s, 2, stage);
  gp.pts_staged = stage ? 1 : 0;
  launch_tile_points(gp, fs->p, count, s);
}
// Runs the deferred end of a batch build on stream s (which is first ordered behind the build): the depth half of the pyramid
// and the edge lists of the CURRENT frames (odd), and the keyframes' EDT (even).  need_ref_lists (an accessor or a single-pair
// call on an EVEN view): also the depth half and the edge lists of the keyframe-role frames, which no tracker grid of the
// batch reads -- the same kernels over frames 0, 2, 4, ..., so what an accessor returns is what an eager build returns.
int run_pending_edt(revo_ctx* c, FrameSet* fs, hipStream_t s, bool need_ref_lists) {
  std::lock_guard<std::mutex> lk(fs->edt_mu);
  bool behind_build = false;  // s already waits for the build
  if (!fs->edt_pending) {
    // already enqueued by an earlier consumer: a consumer on ANOTHER stream must still wait for it
    TRY(fs->edt.wait_elsewhere(s));
  } else {
    TRY(fs->ready.wait(s));
    behind_build = true;
    // the set's previous tracker grid still reads the lists, counts and DT planes written below (the build stream, which
    // writes none of them, does not wait for it)
    if (fs->trk_mark) TRY(fs->trk_mark->wait_elsewhere(s));
    // (the edge lists and the EDT do not depend on each other; running the EDT first -- next to the memory-bound first kernels of
    // the following build instead of its VALU-bound NMS -- was measured equal: profiles/r04_ab_aux_order.txt)
    enqueue_list_side(c, fs, 1, 2, fs->edt_count, s);  // frame 2i + 1 is pair i's current frame: the only lists a grid reads
    launch_keyframe(geom_of_set(c, fs), fs->p, 0, 2, fs->edt_count, s);  // (a lazy set: the column pass reads bitmaps at every width)
    HIPCHECK(hipGetLastError());
    TRY(fs->edt.record(s));
    fs->edt_pending = false;
  }
  if (!need_ref_lists) return REVO_OK;
  if (!fs->ref_lists_pending) return fs->ref.wait_elsewhere(s);
  if (!behind_build) TRY(fs->ready.wait(s));
  enqueue_list_side(c, fs, 0, 2, fs->edt_count, s);
  HIPCHECK(hipGetLastError());
  TRY(fs->ref.record(s));
  fs->ref_lists_pending = false;
  return REVO_OK;
}
// the next build into a set's planes: the deferred EDT of the previous build may still be reading its edge maps on another
// stream, and so may the keyframe-role frames' edge lists (edge bitmaps, depth level 0)
int wait_edt_before_rebuild(FrameSet* fs, hipStream_t s) {
  std::lock_guard<std::mutex> lk(fs->edt_mu);
  TRY(fs->edt.wait_elsewhere(s));
  TRY(fs->ref.wait_elsewhere(s));
  return fs->ebytes.wait_elsewhere(s);  // an expansion of the byte edge planes that was started still reads the bitmaps
}
int ensure_edge_bytes(revo_ctx* c, FrameSet* fs, hipStream_t s) {
  std::lock_guard<std::mutex> lk(fs->edt_mu);
  if (!fs->edge_bytes_pending) return fs->ebytes.wait_elsewhere(s);  // written by the build, or expanded by an earlier reader
  TRY(fs->ready.wait(s));  // behind fill-in
  launch_edge_bytes(c->geom, fs->p, fs->B, s);
  HIPCHECK(hipGetLastError());
  TRY(fs->ebytes.record(s));
  fs->edge_bytes_pending = false;
  return REVO_OK;
}
// Waits for an event by POLLING it (the in-place frame upload, ~50-100 us): the IO thread gets its answer a few microseconds after the
// copy has finished instead of after hipEventSynchronize's park-and-wake; the sequential stream runs 1-3 % faster with it
// (profiles/r06_slow_run_probe.txt: 4.05-4.19 k frames/s with hipEventSynchronize against 4.09-4.24 k).
int wait_event_polled(hipEvent_t ev) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spin = 0;; ++spin) {
    const hipError_t e = hipEventQuery(ev);
    if (e == hipSuccess) return REVO_OK;
    if (e != hipErrorNotReady) { (void)hipGetLastError(); return fail(REVO_ERR_HIP, std::string("hipEventQuery: ") + hipGetErrorString(e)); }
    (void)hipGetLastError();
    for (int k = 0; k < 32; ++k) __builtin_ia32_pause();
    if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;  // something is wrong: block
  }
  HIPCHECK(hipEventSynchronize(ev));
  return REVO_OK;
}
// Waits for a sequence word a kernel writes (system scope) after its results in pinned host memory: a short spin
// (the kernel is usually about to finish: a stream synchronise costs a sleep / wake-up of the calling thread),
// then the stream `s` the kernel was launched on (the vote runs on the vote stream: synchronising the tracker's
// stream there returned before a vote queued behind other work had run).
// (debug: how often the spin below ran out and what the longest wait was -- profiles/slow_run_probe.py prints them)
static std::atomic<unsigned long long> g_wait_fallbacks{0}, g_wait_max_ns{0}, g_wait_calls{0};
extern "C" void revo_debug_wait_stats_(unsigned long long out[3]) {
  out[0] = g_wait_calls.load(); out[1] = g_wait_fallbacks.load(); out[2] = g_wait_max_ns.load();
}
int wait_seq(hipStream_t s, volatile unsigned* word, unsigned want) {
  static const int spin_limit = env_int("REVO_WAIT_SPINS", 200000, 1000, 2000000000);
  const auto t0 = std::chrono::steady_clock::now();
  g_wait_calls.fetch_add(1, std::memory_order_relaxed);
  auto note = [&]() {
    const unsigned long long ns = (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    unsigned long long cur = g_wait_max_ns.load(std::memory_order_relaxed);
    while (ns > cur && !g_wait_max_ns.compare_exchange_weak(cur, ns)) {}
  };
  for (int spin = 0; spin < spin_limit; ++spin) {
    if (*word == want) { std::atomic_thread_fence(std::memory_order_acquire); note(); return REVO_OK; }
    __builtin_ia32_pause();
  }
  g_wait_fallbacks.fetch_add(1, std::memory_order_relaxed);
  HIPCHECK(hipStreamSynchronize(s));
  note();
  if (*word != want) return fail(REVO_ERR_HIP, "a kernel finished without publishing its result");
  return REVO_OK;
}
