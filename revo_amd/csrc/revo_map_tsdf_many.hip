// revo_map_tsdf_many.hip -- surfaces for many sequences at once: revo_map_tsdf_fuse_many, n (volume, view) fuses in one
// launch; revo_map_tsdf_track_eval_many, the poses of n (volume, frame) jobs in one launch; revo_map_tsdf_track_many, the
// Gauss-Newton loops of n jobs in lockstep with one launch, one copy and one wait per round; revo_map_tsdf_unfuse_many,
// n (volume, view) unfuses in a check and an apply launch with no host wait between them.  Contract: include/revo_hip.h.  Every
// output is the single call's (revo_map_tsdf.hip, revo_map_tsdf_track.hip) byte for byte: the per-cell and per-pixel rules are the
// ones those kernels call, from the same headers; this unit holds the job tables, how a block finds its job, and the entry points.
#include "revo_map_impl.h"
#include "revo_track_dev.h"
#include "revo_align_host.h"
#include "revo_cell_run.h"
#include "revo_tsdf_host.h"
#include "revo_tsdf_track_host.h"
#include "revo_tsdf_many_host.h"

static_assert(sizeof(revo_map_tsdf_fuse_job) == 200 && offsetof(revo_map_tsdf_fuse_job, box) == 8 && offsetof(revo_map_tsdf_fuse_job, trunc) == 32 &&
              offsetof(revo_map_tsdf_fuse_job, reserved) == 36 && offsetof(revo_map_tsdf_fuse_job, tsdf) == 40 && offsetof(revo_map_tsdf_fuse_job, color) == 48 &&
              offsetof(revo_map_tsdf_fuse_job, view) == 56 && offsetof(revo_map_tsdf_fuse_job, bgr) == 168 && offsetof(revo_map_tsdf_fuse_job, info) == 176 &&
              offsetof(revo_map_tsdf_fuse_job, color_info) == 184 && offsetof(revo_map_tsdf_fuse_job, view_info) == 192, "the fuse job is the documented layout");
static_assert(sizeof(revo_map_tsdf_track_job) == 200 && offsetof(revo_map_tsdf_track_job, box) == 8 && offsetof(revo_map_tsdf_track_job, trunc) == 32 &&
              offsetof(revo_map_tsdf_track_job, n_poses) == 36 && offsetof(revo_map_tsdf_track_job, tsdf) == 40 && offsetof(revo_map_tsdf_track_job, frame) == 48 &&
              offsetof(revo_map_tsdf_track_job, prm) == 160 && offsetof(revo_map_tsdf_track_job, poses) == 192, "the track job is the documented layout");
static_assert(sizeof(revo_map_tsdf_track_result) == 288 && offsetof(revo_map_tsdf_track_result, info) == 64 && offsetof(revo_map_tsdf_track_result, iterations) == 272 &&
              offsetof(revo_map_tsdf_track_result, status) == 276 && offsetof(revo_map_tsdf_track_result, evaluations) == 280 &&
              offsetof(revo_map_tsdf_track_result, reserved) == 284, "the track result is the documented layout");
static_assert(sizeof(revo_map_tsdf_info) == 4 * TSDF_MANY_LINE_CINFO && sizeof(revo_map_tsdf_color_info) == 4 * (TSDF_MANY_LINE_VINFO - TSDF_MANY_LINE_CINFO) &&
              sizeof(revo_map_carve_view_info) == 4 * (TSDF_MANY_LINE - TSDF_MANY_LINE_VINFO), "a job's counter line is the three records side by side");
static_assert(offsetof(revo_map_tsdf_info, cells) == 0 && offsetof(revo_map_tsdf_info, updates) == 8 && offsetof(revo_map_tsdf_info, saturated) == 32 &&
              offsetof(revo_map_tsdf_color_info, color_updates) == 0 && offsetof(revo_map_tsdf_color_info, cells_colored) == 8, "the counters' places");

typedef unsigned __attribute__((address_space(1)))* tmy_gu32p;
typedef u64 __attribute__((address_space(1)))* tmy_gu64p;
#define TMY_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// =============================================================================================================== the fuse ==
struct TsdfManyFuseJob {  // one job of a launch, in device memory
  MapCarveView view;
  const uint8_t* bgr;   // the view's colour image; not read without a colour volume
  int2* tsdf;           // 16-byte aligned: thread t of the job's block b owns the cells 4 (256 b + t) .. + 3
  uint4* color;         // NULL: the job fuses no colour
  unsigned* info;       // the job's own records, or NULL: revo_map_tsdf_info, revo_map_tsdf_color_info, revo_map_carve_view_info
  unsigned* cinfo;
  unsigned* vinfo;
  revo_map_df_box box;
  unsigned cells;
  unsigned first_block, blocks;  // the job's blocks of the launch: tsdf_many_find
  float trunc, voxel;
};
struct TsdfManyFuseK {
  const TsdfManyFuseJob* jobs; int n;
  unsigned total_blocks;
  unsigned* lines;    // TSDF_MANY_STRIDE words per job, zero before the launch: the counters (TSDF_MANY_LINE words) and the job's ticket
};

// One block of one job: k_tsdf_fuse's body for one view into a volume that is read and updated, over the same walk
// (revo_cell_run.h).  The classes of a wave are counted by ballots into LDS.  blk: the block's number within the job.
template <bool COLOR>
__device__ __forceinline__ void tmy_fuse_block(const TsdfManyFuseJob& a, unsigned blk, unsigned* s_cls, unsigned* s_cnt, unsigned* s_col) {
  CellRun r;
  const size_t c0 = cell_run_first(blk);
  int sum[CELL_RUN];
  unsigned weight[CELL_RUN];
  uint4 rgb[CELL_RUN];  // COLOR: the colour cells
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j) {
    cell_run_cell(c0, j, a.box, a.cells, a.voxel, r);
    sum[j] = 0;
    weight[j] = 0u;
    if (COLOR) rgb[j] = make_uint4(0u, 0u, 0u, 0u);
  }
  cell_run_load(a.tsdf, c0, r, sum, weight);
  cell_run_load_color<COLOR>(a.color, c0, r, rgb);
  unsigned n_upd = 0, n_sat = 0, n_cupd = 0;
  int cls[CELL_RUN];
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j) {
    float z = 0.0f, dc = 0.0f;
    unsigned pix = 0u;
    if (COLOR) cls[j] = r.valid[j] ? map_carve_class_zdp(r.px[j], r.py[j], r.pz[j], a.view, 0, a.trunc, 0.0f, &z, &dc, &pix) : -1;
    else cls[j] = r.valid[j] ? map_carve_class_zd(r.px[j], r.py[j], r.pz[j], a.view, 0, a.trunc, 0.0f, &z, &dc) : -1;
    if (cls[j] == CARVE_FREE || cls[j] == CARVE_CONFIRMED) {
      const int q = cls[j] == CARVE_FREE ? TSDF_Q_ONE : tsdf_quantum(dc, z, a.trunc);
      const unsigned dropped = tsdf_update(sum[j], weight[j], q);
      n_sat += dropped;
      n_upd += 1u - dropped;
      if (COLOR) n_cupd += tsdf_color_update(rgb[j].x, rgb[j].y, rgb[j].z, rgb[j].w, cls[j] == CARVE_CONFIRMED, dropped, a.bgr + (size_t)pix * 3);
    }
  }
  cell_run_count_classes(cls, s_cls);  // uniform: the ballots see whole waves
  unsigned n_weighted = 0, n_inside = 0, n_col = 0;
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j)
    if (r.valid[j]) {
      n_weighted += weight[j] > 0u;
      n_inside += weight[j] > 0u && sum[j] < 0;
    }
  cell_run_store(a.tsdf, c0, r, sum, weight);
  cell_run_store_color<COLOR>(a.color, c0, r, rgb);
  if (COLOR) {
#pragma unroll
    for (int j = 0; j < CELL_RUN; ++j) n_col += r.valid[j] && rgb[j].w > 0u;
  }
  if (COLOR) cell_run_tally(s_col, n_cupd, n_col);
  cell_run_tally(s_cnt, n_upd, n_weighted, n_inside, n_sat);  // a block's updates: at most 256 * 4
}

// Grid: the blocks of all jobs, job after job (tsdf_many_find).  A block past the last job's returns before any barrier.  A
// block's counters go into its job's line of the scratch with one global atomic each; then it draws the job's ticket, and the
// block that draws the last one copies the line, complete by then, into the job's own records.  The order is k_map_tsdf_track's:
// device-scope atomics, the wait for them, then the ticket; only the last block pays for an acquire.  No fence that writes the
// L2 back stands in a block's way (a release fence per block cost five times the kernel: profiles/multi_surface_rates.txt).  No
// atomic touches a cell, and no block waits for another.
__global__ void __launch_bounds__(TSDF_MANY_THREADS) k_tsdf_fuse_many(const TsdfManyFuseK a) {
  __shared__ unsigned s_cls[CARVE_CLASSES];
  __shared__ unsigned s_cnt[4];  // updates, weighted, inside, saturated
  __shared__ unsigned s_col[2];  // colour updates, cells coloured
  __shared__ unsigned s_last;
  if (blockIdx.x >= a.total_blocks) return;
  const int job = tsdf_many_find(a.n, blockIdx.x, [&](int j) { return a.jobs[j].first_block; });
  const TsdfManyFuseJob J = a.jobs[job];  // a uniform address: scalar loads
  const unsigned tid = threadIdx.x;
  if (tid < CARVE_CLASSES) s_cls[tid] = 0;
  if (tid < 4) s_cnt[tid] = 0;
  if (tid < 2) s_col[tid] = 0;
  __syncthreads();
  const bool with_color = J.color != nullptr;
  if (with_color) tmy_fuse_block<true>(J, blockIdx.x - J.first_block, s_cls, s_cnt, s_col);
  else tmy_fuse_block<false>(J, blockIdx.x - J.first_block, s_cls, s_cnt, s_col);
  __syncthreads();
  unsigned* const line = a.lines + (size_t)job * TSDF_MANY_STRIDE;
  u64* const info = (u64*)line;
  u64* const cinfo = (u64*)(line + TSDF_MANY_LINE_CINFO);
  if (tid < 4 && s_cnt[tid]) atomicAdd(&info[1 + tid], (u64)s_cnt[tid]);  // updates, cells_weighted, cells_inside, saturated
  if (with_color && tid >= 8 && tid < 10 && s_col[tid - 8]) atomicAdd(&cinfo[tid - 8], (u64)s_col[tid - 8]);
  if (tid >= 16 && tid < 16 + CARVE_CLASSES && s_cls[tid - 16]) atomicAdd(&line[TSDF_MANY_LINE_VINFO + tid - 16], s_cls[tid - 16]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's counters have left this CU ...
  __syncthreads();                                  // ... and so have every thread's of the block, before its ticket is drawn
  if (tid == 0) s_last = __hip_atomic_fetch_add((tmy_gu32p)(line + TSDF_MANY_LINE_TICKET), 1u, TMY_RLX_AGENT) == J.blocks - 1u ? 1u : 0u;
  __syncthreads();
  if (!s_last || tid >= TSDF_MANY_LINE) return;
  // the last block of the job to arrive: every block's counters are in the line
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  unsigned w = __hip_atomic_load((tmy_gu32p)(line + tid), TMY_RLX_AGENT);
  if (tid == 0) w = J.cells;  // revo_map_tsdf_info.cells: below 2^32, its high word stays zero
  unsigned* const rec = tid < TSDF_MANY_LINE_CINFO ? J.info : (tid < TSDF_MANY_LINE_VINFO ? J.cinfo : J.vinfo);
  const unsigned at = tid < TSDF_MANY_LINE_CINFO ? tid : (tid < TSDF_MANY_LINE_VINFO ? tid - TSDF_MANY_LINE_CINFO : tid - TSDF_MANY_LINE_VINFO);
  if (rec) rec[at] = w;
}

namespace {
bool tmy_on_device(const void* p, int dev) {  // device memory of `dev` (not host, not another device)
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice && a.device == dev;
}

// A job's map: of m's context; NULL: m.
int tmy_job_map(revo_map* m, revo_map* jm, const std::string& at, revo_map** out) {
  *out = jm ? jm : m;
  if ((*out)->ctx != m->ctx) return fail(REVO_ERR_INVALID_ARG, at + "the job's map belongs to another context");
  return REVO_OK;
}

// One view or frame of a job: its own rules, a raw image in device memory of m's device, a pyramid of m's context that is no
// batch view.  Nothing is enqueued.
int tmy_view_check(revo_map* m, const revo_map_carve_view* v, const std::string& at, CarveView* out) {
  const CarveCam cam{m->g.fx, m->g.fy, m->g.cx, m->g.cy, m->g.dmin, m->g.dmax};
  if (const char* why = carve_view_check(v, cam, m->g.w, m->g.h, out)) return fail(REVO_ERR_INVALID_ARG, at + why);
  if (v->depth) {
    TRY(map_check_aligned((uintptr_t)v->depth, 4, at + "the device depth image is"));
    if (!tmy_on_device(v->depth, m->g.device)) return fail(REVO_ERR_INVALID_ARG, at + "the depth image is not in device memory of the map's device");
  } else {
    const revo_ctx* pc = nullptr;
    int batch_view = 0;
    TRY(revo_map_source_kind_(v->kf, &pc, &batch_view));
    if (pc != m->ctx) return fail(REVO_ERR_INVALID_ARG, at + "the pyramid belongs to another context than the map");
    if (batch_view) return fail(REVO_ERR_INVALID_ARG, at + "a batch view is not a keyframe the map calls take (pass its depth plane as a raw image)");
  }
  return REVO_OK;
}
}  // namespace

extern "C" int revo_map_tsdf_fuse_many(revo_map* m, int n_jobs, const revo_map_tsdf_fuse_job* jobs) {
  if (!m || !jobs) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n_jobs < 1 || n_jobs > TSDF_MANY_MAX_JOBS) return fail(REVO_ERR_INVALID_ARG, "revo_map_tsdf_fuse_many: n_jobs must be 1 .. 1024");
  std::vector<TsdfManyFuseJob> hj(n_jobs);
  std::vector<std::pair<uintptr_t, size_t>> ranges;
  ranges.reserve(2 * (size_t)n_jobs);
  size_t total_blocks = 0;
  for (int i = 0; i < n_jobs; ++i) {  // every job's own rules
    const revo_map_tsdf_fuse_job& j = jobs[i];
    TsdfManyFuseJob& d = hj[i];
    const std::string at = "revo_map_tsdf_fuse_many: job " + std::to_string(i) + ": ";
    revo_map* jm = nullptr;
    TRY(tmy_job_map(m, j.map, at, &jm));
    if (!j.tsdf) return fail(REVO_ERR_INVALID_ARG, at + "null volume");
    if (j.reserved) return fail(REVO_ERR_INVALID_ARG, at + "a reserved word is not 0");
    size_t cells = 0;
    if (const char* why = map_df_box_check(&j.box, &cells)) return fail(REVO_ERR_INVALID_ARG, at + why);
    TRY(map_check_aligned((uintptr_t)j.tsdf | (uintptr_t)j.color | (uintptr_t)j.info | (uintptr_t)j.color_info | (uintptr_t)j.view_info, 16, at + "a device output is"));
    revo_map_tsdf_params prm{j.trunc, 1u, {0u, 0u}}, pp;
    if (j.trunc == 0.0f) prm.trunc = 4.0f * jm->voxel;  // tsdf_params_check's default
    if (const char* why = tsdf_params_check(&prm, jm->voxel, &pp)) return fail(REVO_ERR_INVALID_ARG, at + why);
    if (j.color) {
      if (const char* why = tsdf_bgr_check(&j.view, j.bgr)) return fail(REVO_ERR_INVALID_ARG, at + why);
    } else if (j.bgr || j.color_info) {
      return fail(REVO_ERR_INVALID_ARG, at + "bgr and color_info go with a colour volume");
    }
    TRY(tmy_view_check(m, &j.view, at, &d.view.v));
    const int dev = m->g.device;
    if (!tmy_on_device(j.tsdf, dev) || (j.color && !tmy_on_device(j.color, dev)) || (j.bgr && !tmy_on_device(j.bgr, dev)) || (j.info && !tmy_on_device(j.info, dev)) ||
        (j.color_info && !tmy_on_device(j.color_info, dev)) || (j.view_info && !tmy_on_device(j.view_info, dev)))
      return fail(REVO_ERR_INVALID_ARG, at + "a volume, an image or a record is not in device memory of the map's device");
    ranges.emplace_back((uintptr_t)j.tsdf, sizeof(revo_map_tsdf_cell) * cells);
    if (j.color) ranges.emplace_back((uintptr_t)j.color, sizeof(revo_map_tsdf_color) * cells);
    d.view.depth = j.view.depth;
    d.bgr = j.color ? j.bgr : nullptr;
    d.tsdf = (int2*)j.tsdf; d.color = (uint4*)j.color;
    d.info = (unsigned*)j.info; d.cinfo = (unsigned*)j.color_info; d.vinfo = (unsigned*)j.view_info;
    d.box = j.box;
    d.cells = (unsigned)cells;
    d.first_block = (unsigned)total_blocks; d.blocks = tsdf_many_blocks(cells);
    d.trunc = pp.trunc; d.voxel = jm->voxel;
    total_blocks += d.blocks;
  }
  if (tsdf_many_overlap(ranges)) return fail(REVO_ERR_INVALID_ARG, "revo_map_tsdf_fuse_many: two volumes of the call share memory");
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  for (int i = 0; i < n_jobs; ++i) {  // the pyramids' planes: the tracker stream is ordered behind their builds
    if (!jobs[i].view.kf) continue;
    MapSource src;
    TRY(revo_map_source_(const_cast<revo_pyr*>(jobs[i].view.kf), &src));
    hj[i].view.depth = src.depth;
    if (jobs[i].color) hj[i].bgr = src.bgr;
  }
  MapTsdfManyScratch& w = m->tsdfmany;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t total = up(sizeof(unsigned) * TSDF_MANY_STRIDE * n_jobs);
  TRY(w.fuse_jobs.reserve(n_jobs, s));  // waits until the previous call's upload has read the pinned rows
  TRY(w.fuse_work.reserve(total, s));
  memcpy(w.fuse_jobs.h, hj.data(), sizeof(TsdfManyFuseJob) * n_jobs);
  TRY(w.fuse_jobs.upload(n_jobs, s));
  TsdfManyFuseK a{};
  a.jobs = w.fuse_jobs.d; a.n = n_jobs;
  a.total_blocks = (unsigned)total_blocks;
  a.lines = (unsigned*)w.fuse_work.p;
  HIPCHECK(hipMemsetAsync(w.fuse_work.p, 0, total, s));
  hipLaunchKernelGGL(k_tsdf_fuse_many, dim3((unsigned)total_blocks), dim3(TSDF_MANY_THREADS), 0, s, a);
  HIPCHECK(hipGetLastError());
  return REVO_OK;
}

// ============================================================================================================ the unfuse ==
// revo_map_tsdf_unfuse_many: the check pass and the apply pass of revo_map_tsdf_unfuse for n (volume, view) jobs, one
// launch each, with the verdict left on the device between them.
enum { TMU_CELLS = 0, TMU_UPDATES = 1, TMU_WEIGHTED = 2, TMU_INSIDE = 3, TMU_MISFITS = 4, TMU_CUPDATES = 5, TMU_COLORED = 6 };  // u64s of a revo_map_tsdf_unfuse_info
#define TMU_LINE_VINFO 16  // a job's counter line, words: revo_map_tsdf_unfuse_info | revo_map_carve_view_info (the check pass's line alone)
#define TMU_LINE 24
#define TMU_RES_WORDS 20   // a revo_map_tsdf_unfuse_result: the info, the status, three zero words
static_assert(sizeof(revo_map_tsdf_unfuse_job) == 192 && offsetof(revo_map_tsdf_unfuse_job, box) == 8 && offsetof(revo_map_tsdf_unfuse_job, trunc) == 32 &&
              offsetof(revo_map_tsdf_unfuse_job, reserved) == 36 && offsetof(revo_map_tsdf_unfuse_job, tsdf) == 40 && offsetof(revo_map_tsdf_unfuse_job, color) == 48 &&
              offsetof(revo_map_tsdf_unfuse_job, view) == 56 && offsetof(revo_map_tsdf_unfuse_job, bgr) == 168 && offsetof(revo_map_tsdf_unfuse_job, info) == 176 &&
              offsetof(revo_map_tsdf_unfuse_job, view_info) == 184, "the unfuse job is the documented layout");
static_assert(sizeof(revo_map_tsdf_unfuse_result) == 4 * TMU_RES_WORDS && offsetof(revo_map_tsdf_unfuse_result, info) == 0 &&
              offsetof(revo_map_tsdf_unfuse_result, status) == 64 && offsetof(revo_map_tsdf_unfuse_result, reserved) == 68, "the unfuse result is the documented layout");
static_assert(sizeof(revo_map_tsdf_unfuse_info) == 4 * TMU_LINE_VINFO && sizeof(revo_map_carve_view_info) == 4 * (TMU_LINE - TMU_LINE_VINFO) &&
              TMU_LINE <= TSDF_MANY_LINE_TICKET, "a job's counter line is the two records side by side, in front of its ticket");
static_assert(offsetof(revo_map_tsdf_unfuse_info, cells) == 8 * TMU_CELLS && offsetof(revo_map_tsdf_unfuse_info, updates) == 8 * TMU_UPDATES &&
              offsetof(revo_map_tsdf_unfuse_info, cells_weighted) == 8 * TMU_WEIGHTED && offsetof(revo_map_tsdf_unfuse_info, cells_inside) == 8 * TMU_INSIDE &&
              offsetof(revo_map_tsdf_unfuse_info, misfits) == 8 * TMU_MISFITS && offsetof(revo_map_tsdf_unfuse_info, color_updates) == 8 * TMU_CUPDATES &&
              offsetof(revo_map_tsdf_unfuse_info, cells_colored) == 8 * TMU_COLORED && offsetof(revo_map_tsdf_unfuse_info, reserved) == 56, "the counters' places");

struct TsdfManyUnfuseJob {  // one job of the two launches, in device memory
  MapCarveView view;
  const uint8_t* bgr;   // the view's colour image; not read without a colour volume
  int2* tsdf;           // 16-byte aligned: thread t of the job's block b owns the cells 4 (256 b + t) .. + 3
  uint4* color;         // NULL: the job's colour volume is not touched
  unsigned* info;       // the job's own records, or NULL: revo_map_tsdf_unfuse_info, revo_map_carve_view_info
  unsigned* vinfo;
  unsigned* res;        // the job's revo_map_tsdf_unfuse_result of the call's results, or NULL
  revo_map_df_box box;
  unsigned cells;
  unsigned first_block, blocks;  // the job's blocks of either launch: tsdf_many_find
  float trunc, voxel;
};
struct TsdfManyUnfuseK {
  const TsdfManyUnfuseJob* jobs; int n;
  unsigned total_blocks;
  unsigned* lines;    // 2 TSDF_MANY_STRIDE words per job, zero before the check launch: the check pass's line and ticket, then the apply pass's
};

// One block of one job: k_tsdf_unfuse's body for one view (revo_map_tsdf_unfuse.hip), over the same walk and through the same
// per-cell rules.  The check pass (APPLY false) writes nothing to the volumes; s_cnt: the TMU_* counters of the block.
template <bool COLOR, bool APPLY>
__device__ __forceinline__ void tmy_unfuse_block(const TsdfManyUnfuseJob& a, unsigned blk, unsigned* s_cls, unsigned* s_cnt) {
  CellRun r;
  const size_t c0 = cell_run_first(blk);
  int sum[CELL_RUN];
  unsigned weight[CELL_RUN];
  uint4 rgb[CELL_RUN];  // COLOR: the colour cells
  TsdfDown down[CELL_RUN];
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j) {
    cell_run_cell(c0, j, a.box, a.cells, a.voxel, r);
    sum[j] = 0;
    weight[j] = 0u;
    rgb[j] = make_uint4(0u, 0u, 0u, 0u);
    down[j] = TsdfDown{0u, 0u, 0, 0u, 0u, 0u};
  }
  cell_run_load(a.tsdf, c0, r, sum, weight);
  cell_run_load_color<COLOR>(a.color, c0, r, rgb);
  int cls[CELL_RUN];
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j) {
    float z = 0.0f, dc = 0.0f;
    unsigned pix = 0u;
    if (COLOR) cls[j] = r.valid[j] ? map_carve_class_zdp(r.px[j], r.py[j], r.pz[j], a.view, 0, a.trunc, 0.0f, &z, &dc, &pix) : -1;
    else cls[j] = r.valid[j] ? map_carve_class_zd(r.px[j], r.py[j], r.pz[j], a.view, 0, a.trunc, 0.0f, &z, &dc) : -1;
    if (cls[j] == CARVE_FREE || cls[j] == CARVE_CONFIRMED) {
      const bool confirmed = cls[j] == CARVE_CONFIRMED;
      const int q = confirmed ? tsdf_quantum(dc, z, a.trunc) : TSDF_Q_ONE;
      tsdf_down_add(down[j], confirmed, q, COLOR && confirmed ? a.bgr + (size_t)pix * 3 : nullptr);
    }
  }
  if (!APPLY) cell_run_count_classes(cls, s_cls);  // uniform: the ballots see whole waves
  unsigned n_upd = 0, n_cupd = 0, n_misfit = 0, n_weighted = 0, n_inside = 0, n_col = 0;
#pragma unroll
  for (int j = 0; j < CELL_RUN; ++j) {
    if (!r.valid[j]) continue;
    if (down[j].k) {
      if (APPLY) {
        tsdf_down_apply(sum[j], weight[j], down[j]);
        n_upd += down[j].k;
        if (COLOR) {
          tsdf_down_color_apply(rgb[j].x, rgb[j].y, rgb[j].z, rgb[j].w, down[j]);
          n_cupd += down[j].kc;
        }
      } else {
        const bool fits = tsdf_down_fits(sum[j], weight[j], down[j]) &&
                          (!COLOR || tsdf_down_color_fits(weight[j], rgb[j].x, rgb[j].y, rgb[j].z, rgb[j].w, down[j]));
        n_misfit += fits ? 0u : 1u;
      }
    }
    n_weighted += weight[j] > 0u;
    n_inside += weight[j] > 0u && sum[j] < 0;
    if (COLOR) n_col += rgb[j].w > 0u;
  }
  if (APPLY) {
    cell_run_store(a.tsdf, c0, r, sum, weight);
    cell_run_store_color<COLOR>(a.color, c0, r, rgb);
  }
  // the counters in TMU_*'s order, from TMU_UPDATES on
  if (COLOR) cell_run_tally(s_cnt + TMU_UPDATES, n_upd, n_weighted, n_inside, n_misfit, n_cupd, n_col);
  else cell_run_tally(s_cnt + TMU_UPDATES, n_upd, n_weighted, n_inside, n_misfit);
}

// Grid, job table, counters and ticket: k_tsdf_fuse_many's.  A job has two lines in the scratch, one per pass.
// The check pass: the block that draws a job's last ticket writes the job's view_info and the check line as its info -- the single
// call's refused info when there are misfits -- and the job's status into the results.
// The apply pass: a block first reads its job's misfit count from the check pass's line (a uniform address; the kernel boundary on
// the stream orders the read) and returns before it touches anything when the job is refused.  Otherwise it down-dates its cells,
// and the job's last block overwrites the info with the apply line.  No block waits for another; no atomic touches a cell.
template <bool APPLY>
__global__ void __launch_bounds__(TSDF_MANY_THREADS) k_tsdf_unfuse_many(const TsdfManyUnfuseK a) {
  __shared__ unsigned s_cls[CARVE_CLASSES];
  __shared__ unsigned s_cnt[8];  // TMU_*
  __shared__ unsigned s_last;
  if (blockIdx.x >= a.total_blocks) return;
  const int job = tsdf_many_find(a.n, blockIdx.x, [&](int j) { return a.jobs[j].first_block; });
  unsigned* const check_line = a.lines + (size_t)job * (2 * TSDF_MANY_STRIDE);
  if (APPLY && ((const u64*)check_line)[TMU_MISFITS] != 0) return;  // the job was refused: uniform over the block, before any barrier
  const TsdfManyUnfuseJob J = a.jobs[job];  // a uniform address: scalar loads
  const unsigned tid = threadIdx.x;
  if (tid < CARVE_CLASSES) s_cls[tid] = 0;
  if (tid < 8) s_cnt[tid] = 0;
  __syncthreads();
  const bool with_color = J.color != nullptr;
  if (with_color) tmy_unfuse_block<true, APPLY>(J, blockIdx.x - J.first_block, s_cls, s_cnt);
  else tmy_unfuse_block<false, APPLY>(J, blockIdx.x - J.first_block, s_cls, s_cnt);
  __syncthreads();
  unsigned* const line = check_line + (APPLY ? TSDF_MANY_STRIDE : 0);
  u64* const info = (u64*)line;
  if (tid >= TMU_UPDATES && tid <= TMU_COLORED && s_cnt[tid]) atomicAdd(&info[tid], (u64)s_cnt[tid]);
  if (!APPLY && tid >= 16 && tid < 16 + CARVE_CLASSES && s_cls[tid - 16]) atomicAdd(&line[TMU_LINE_VINFO + tid - 16], s_cls[tid - 16]);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's counters have left this CU ...
  __syncthreads();                                  // ... and so have every thread's of the block, before its ticket is drawn
  if (tid == 0) s_last = __hip_atomic_fetch_add((tmy_gu32p)(line + TSDF_MANY_LINE_TICKET), 1u, TMY_RLX_AGENT) == J.blocks - 1u ? 1u : 0u;
  __syncthreads();
  if (!s_last || tid >= TMU_LINE + 4) return;
  // the last block of the job to arrive in this pass: every block's counters are in the line
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (tid < TMU_LINE) {
    unsigned w = __hip_atomic_load((tmy_gu32p)(line + tid), TMY_RLX_AGENT);
    if (tid == 2 * TMU_CELLS) w = J.cells;  // revo_map_tsdf_unfuse_info.cells: below 2^32, its high word stays zero
    if (tid < TMU_LINE_VINFO) {
      if (J.info) J.info[tid] = w;
      if (J.res) J.res[tid] = w;
    } else if (!APPLY && J.vinfo) {
      J.vinfo[tid - TMU_LINE_VINFO] = w;
    }
  } else if (!APPLY && J.res) {  // the status and the three zero words behind it; the apply pass runs only for REVO_OK
    unsigned w = 0u;
    if (tid == TMU_LINE) {
      const unsigned lo = __hip_atomic_load((tmy_gu32p)(line + 2 * TMU_MISFITS), TMY_RLX_AGENT);
      const unsigned hi = __hip_atomic_load((tmy_gu32p)(line + 2 * TMU_MISFITS + 1), TMY_RLX_AGENT);
      w = (lo | hi) ? (unsigned)REVO_ERR_INVALID_ARG : (unsigned)REVO_OK;
    }
    J.res[TMU_LINE_VINFO + tid - TMU_LINE] = w;
  }
}

extern "C" int revo_map_tsdf_unfuse_many(revo_map* m, int n_jobs, const revo_map_tsdf_unfuse_job* jobs, revo_map_tsdf_unfuse_result* results,
                                         int device_out) {
  if (!m || !jobs) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n_jobs < 1 || n_jobs > TSDF_MANY_MAX_JOBS) return fail(REVO_ERR_INVALID_ARG, "revo_map_tsdf_unfuse_many: n_jobs must be 1 .. 1024");
  TRY(map_check_side(device_out, "device_out"));
  const int dev = m->g.device;
  if (results && device_out) {
    TRY(map_check_aligned((uintptr_t)results, 16, "the device results are"));
    if (!tmy_on_device(results, dev)) return fail(REVO_ERR_INVALID_ARG, "revo_map_tsdf_unfuse_many: the device results are not in device memory of the map's device");
  }
  std::vector<TsdfManyUnfuseJob> hj(n_jobs);
  std::vector<std::pair<uintptr_t, size_t>> ranges;
  ranges.reserve(2 * (size_t)n_jobs);
  size_t total_blocks = 0;
  for (int i = 0; i < n_jobs; ++i) {  // every job's own rules
    const revo_map_tsdf_unfuse_job& j = jobs[i];
    TsdfManyUnfuseJob& d = hj[i];
    const std::string at = "revo_map_tsdf_unfuse_many: job " + std::to_string(i) + ": ";
    revo_map* jm = nullptr;
    TRY(tmy_job_map(m, j.map, at, &jm));
    if (!j.tsdf) return fail(REVO_ERR_INVALID_ARG, at + "null volume");
    if (j.reserved) return fail(REVO_ERR_INVALID_ARG, at + "a reserved word is not 0");
    size_t cells = 0;
    if (const char* why = map_df_box_check(&j.box, &cells)) return fail(REVO_ERR_INVALID_ARG, at + why);
    TRY(map_check_aligned((uintptr_t)j.tsdf | (uintptr_t)j.color | (uintptr_t)j.info | (uintptr_t)j.view_info, 16, at + "a device output is"));
    float tr = 0.0f;
    if (const char* why = tsdf_unfuse_trunc(j.trunc, jm->voxel, &tr)) return fail(REVO_ERR_INVALID_ARG, at + why);
    if (j.color) {
      if (const char* why = tsdf_bgr_check(&j.view, j.bgr)) return fail(REVO_ERR_INVALID_ARG, at + why);
    } else if (j.bgr) {
      return fail(REVO_ERR_INVALID_ARG, at + "bgr goes with a colour volume");
    }
    TRY(tmy_view_check(m, &j.view, at, &d.view.v));
    if (!tmy_on_device(j.tsdf, dev) || (j.color && !tmy_on_device(j.color, dev)) || (j.bgr && !tmy_on_device(j.bgr, dev)) || (j.info && !tmy_on_device(j.info, dev)) ||
        (j.view_info && !tmy_on_device(j.view_info, dev)))
      return fail(REVO_ERR_INVALID_ARG, at + "a volume, an image or a record is not in device memory of the map's device");
    ranges.emplace_back((uintptr_t)j.tsdf, sizeof(revo_map_tsdf_cell) * cells);
    if (j.color) ranges.emplace_back((uintptr_t)j.color, sizeof(revo_map_tsdf_color) * cells);
    d.view.depth = j.view.depth;
    d.bgr = j.color ? j.bgr : nullptr;
    d.tsdf = (int2*)j.tsdf; d.color = (uint4*)j.color;
    d.info = (unsigned*)j.info; d.vinfo = (unsigned*)j.view_info;
    d.res = nullptr;
    d.box = j.box;
    d.cells = (unsigned)cells;
    d.first_block = (unsigned)total_blocks; d.blocks = tsdf_many_blocks(cells);
    d.trunc = tr; d.voxel = jm->voxel;
    total_blocks += d.blocks;
  }
  if (tsdf_many_overlap(ranges)) return fail(REVO_ERR_INVALID_ARG, "revo_map_tsdf_unfuse_many: two volumes of the call share memory");
  HIPCHECK(hipSetDevice(dev));
  hipStream_t s = (hipStream_t)m->g.stream;
  for (int i = 0; i < n_jobs; ++i) {  // the pyramids' planes: the tracker stream is ordered behind their builds
    if (!jobs[i].view.kf) continue;
    MapSource src;
    TRY(revo_map_source_(const_cast<revo_pyr*>(jobs[i].view.kf), &src));
    hj[i].view.depth = src.depth;
    if (jobs[i].color) hj[i].bgr = src.bgr;
  }
  MapTsdfManyScratch& w = m->tsdfmany;
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t total = up(sizeof(unsigned) * 2 * TSDF_MANY_STRIDE * n_jobs), res_bytes = sizeof(revo_map_tsdf_unfuse_result) * (size_t)n_jobs;
  TRY(w.unfuse_jobs.reserve(n_jobs, s));  // waits until the previous call's upload has read the pinned rows
  TRY(w.unfuse_work.reserve(total, s));
  unsigned* d_res = (unsigned*)results;
  if (results && !device_out) {
    TRY(w.unfuse_out.reserve(res_bytes, s));
    d_res = (unsigned*)w.unfuse_out.p;
  }
  if (d_res)
    for (int i = 0; i < n_jobs; ++i) hj[i].res = d_res + (size_t)TMU_RES_WORDS * i;
  memcpy(w.unfuse_jobs.h, hj.data(), sizeof(TsdfManyUnfuseJob) * n_jobs);
  TRY(w.unfuse_jobs.upload(n_jobs, s));
  TsdfManyUnfuseK a{};
  a.jobs = w.unfuse_jobs.d; a.n = n_jobs;
  a.total_blocks = (unsigned)total_blocks;
  a.lines = (unsigned*)w.unfuse_work.p;
  HIPCHECK(hipMemsetAsync(w.unfuse_work.p, 0, total, s));
  hipLaunchKernelGGL(k_tsdf_unfuse_many<false>, dim3((unsigned)total_blocks), dim3(TSDF_MANY_THREADS), 0, s, a);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_tsdf_unfuse_many<true>, dim3((unsigned)total_blocks), dim3(TSDF_MANY_THREADS), 0, s, a);
  HIPCHECK(hipGetLastError());
  if (results && !device_out) {
    HIPCHECK(hipMemcpyAsync(results, d_res, res_bytes, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));  // the call's one wait
  }
  return REVO_OK;
}

// ============================================================================================================== tracking ==
#define TMK_THREADS 256
#define TMK_WAVES (TMK_THREADS / 64)
#define TMK_MAX_GROUPS 1024   // workgroups per pose at most: revo_map_tsdf_track_eval's
#define TMK_MAX_TOTAL 16384   // ... and per launch
#define TMK_NS 32             // double-double slots: 28 sums, four stay zero (reduce32x's tree)
#define TMK_PART (2 * TMK_NS) // doubles of a workgroup's partial: heads, then tails
enum { MW_MATCHED = 28, MW_CONSIDERED = 30, MW_SKIPPED = 32, MW_CENTRE = 34, MW_MAXD = 37, MW_R = 38, MW_T = 47, MW_FLAGS = 50,
       MW_END = 52 };  // words of a revo_map_tsdf_track_info record
static_assert(sizeof(revo_map_tsdf_track_info) == 4 * MW_END && offsetof(revo_map_tsdf_track_info, matched) == 4 * MW_MATCHED &&
              offsetof(revo_map_tsdf_track_info, considered) == 4 * MW_CONSIDERED && offsetof(revo_map_tsdf_track_info, skipped) == 4 * MW_SKIPPED &&
              offsetof(revo_map_tsdf_track_info, centre) == 4 * MW_CENTRE && offsetof(revo_map_tsdf_track_info, max_dist) == 4 * MW_MAXD &&
              offsetof(revo_map_tsdf_track_info, R) == 4 * MW_R && offsetof(revo_map_tsdf_track_info, T) == 4 * MW_T &&
              offsetof(revo_map_tsdf_track_info, flags) == 4 * MW_FLAGS, "record layout");

struct TsdfManyTrackJob {  // one (volume, frame) of a launch, in device memory
  TsdfTrackK k;
  const float* depth;      // the frame: h rows of w floats
  int w, h, stride;
  int lw, lh;              // the strided lattice: tsdf_track_lattice of w and h
};
struct TsdfManyPose { float p[12]; int job; int pad[3]; };  // R column-major, t; the row's job
struct TsdfManyTrackK {
  const TsdfManyTrackJob* jobs;
  const TsdfManyPose* poses;
  double* part; unsigned* cnt; unsigned* ticket;
  unsigned* out;           // revo_map_tsdf_track_info records, one per pose row
};

// Grid (G, pose rows).  A pose row carries its job, the lattice comes from the job table; workgroup g of a pose takes the 32 x 8
// pixel blocks g, g + G, ... of its job's lattice, a wave an 8 x 8 tile (k_map_tsdf_track's layout and per-pixel calls).  A
// workgroup whose lattice has no block for it still publishes a zero partial and draws its ticket.  The finish is
// k_map_tsdf_track's: wave butterfly, LDS across the waves in index order, the partial published write-through, a ticket per
// pose; whoever draws the last one adds the G partials in a fixed order and one wave writes the record.  Nobody waits for
// another group's progress.
__global__ void __launch_bounds__(TMK_THREADS) k_map_tsdf_track_many(const TsdfManyTrackK a) {
  constexpr int NS = TMK_NS, PART = TMK_PART;
  __shared__ double s_h[TMK_WAVES][NS], s_l[TMK_WAVES][NS];
  __shared__ unsigned s_c[TMK_WAVES][2];
  const int pose = blockIdx.y, grp = blockIdx.x, G = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned* const rec = a.out + (size_t)pose * MW_END;

  const TsdfManyPose& row = a.poses[pose];
  const TsdfManyTrackJob J = a.jobs[row.job];  // a uniform address: scalar loads
  const float* P = row.p;
  float R[9], T[3];
  unsigned Rb[9], Tb[3];
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 9; ++i) { R[i] = P[i]; Rb[i] = __float_as_uint(R[i]); finite = finite && __builtin_isfinite(R[i]); }
#pragma unroll
  for (int i = 0; i < 3; ++i) { T[i] = P[9 + i]; Tb[i] = __float_as_uint(T[i]); finite = finite && __builtin_isfinite(T[i]); }
  const bool no_eval = !finite || !is_orthogonal(R);
  // the record's tail (centre, max_dist, pose, flags, reserved): the same whether or not the pose is evaluated
  unsigned tail = 0u;
#pragma unroll
  for (int i = 0; i < 3; ++i) tail = lane == MW_CENTRE + i ? __float_as_uint(J.k.centre[i]) : tail;
  tail = lane == MW_MAXD ? __float_as_uint(J.k.max_dist) : tail;
#pragma unroll
  for (int i = 0; i < 9; ++i) tail = lane == MW_R + i ? Rb[i] : tail;
#pragma unroll
  for (int i = 0; i < 3; ++i) tail = lane == MW_T + i ? Tb[i] : tail;
  tail = lane == MW_FLAGS ? (no_eval ? 1u : 0u) : tail;
  if (no_eval) {  // the same for every workgroup of the pose
    if (grp == 0 && tid < MW_END) rec[tid] = tail;
    return;
  }

  double xd[PART];  // the double-double slots: heads, then tails
#pragma unroll
  for (int k = 0; k < PART; ++k) xd[k] = 0.0;
  unsigned matched = 0, skipped = 0;
  const int lw = J.lw, lh = J.lh, stride = J.stride, w = J.w;
  const int bw = (lw + 31) / 32, bh = (lh + 7) / 8;
  const int nblocks = bw * bh;
  const gf32p depth = (gf32p)J.depth;
#pragma unroll 1
  for (int bt = grp; bt < nblocks; bt += G) {
    const int X = (bt % bw) * 32 + wave * 8 + (lane & 7), Y = (bt / bw) * 8 + (lane >> 3);
    if (X >= lw || Y >= lh) continue;
    const int x = X * stride, y = Y * stride;  // x < w and y < h: the lattice ends before the image does
    const float D = depth[(size_t)y * w + x];
    float pw[3], e = 0.0f, g[3] = {0.0f, 0.0f, 0.0f};
    const int cls = tsdf_track_pixel(J.k, R, T, x, y, D, pw, &e, g);
    if (cls == TSDF_TRACK_SKIPPED) { ++skipped; continue; }
    if (cls == TSDF_TRACK_GATED) continue;
    ++matched;
    tsdf_track_terms(tsdf_track_row(J.k, pw, g), e, [&](int slot, float term) { dd_acc(xd[slot], xd[NS + slot], (double)term); });
  }
  reduce32x(xd, xd + NS, lane);  // lane L: the wave's total of slot idx32(L & 31)
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { matched += __shfl_xor(matched, off, 64); skipped += __shfl_xor(skipped, off, 64); }
  if (lane < NS) {
    const int slot = idx32(lane);
    s_h[wave][slot] = xd[0]; s_l[wave][slot] = xd[NS];
  }
  if (lane == 0) { s_c[wave][0] = matched; s_c[wave][1] = skipped; }
  __syncthreads();
  if (wave != 0) return;

  // wave 0: the workgroup's partial (waves in index order), published write-through, then the ticket
  const int k = lane & (NS - 1);
  double h = s_h[0][k], l = s_l[0][k];
  unsigned cn = lane < 2 ? s_c[0][lane] : 0u;
#pragma unroll
  for (int wv = 1; wv < TMK_WAVES; ++wv) { dd_add(h, l, s_h[wv][k], s_l[wv][k]); cn += lane < 2 ? s_c[wv][lane] : 0u; }
  tmy_gu64p mine = (tmy_gu64p)(a.part + ((size_t)pose * G + grp) * PART);
  if (lane < NS) {
    __hip_atomic_store(mine + k, (u64)__double_as_longlong(h), TMY_RLX_AGENT);
    __hip_atomic_store(mine + NS + k, (u64)__double_as_longlong(l), TMY_RLX_AGENT);
  }
  tmy_gu32p cnts = (tmy_gu32p)(a.cnt + ((size_t)pose * G) * 2);
  if (lane < 2) __hip_atomic_store(cnts + 2 * grp + lane, cn, TMY_RLX_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial has left this CU before the ticket is drawn
  unsigned drawn = 0u;
  if (lane == 0) drawn = __hip_atomic_fetch_add((tmy_gu32p)(a.ticket + pose), 1u, TMY_RLX_AGENT);
  drawn = (unsigned)__builtin_amdgcn_readfirstlane((int)drawn);
  if (drawn != (unsigned)(G - 1)) return;

  // the last workgroup of the pose to arrive: every partial is published.  Lane L adds slot L & 31 of the groups L / 32,
  // L / 32 + 2, ... in index order; the two group sums meet across the half-waves.
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  tmy_gu64p all = (tmy_gu64p)(a.part + (size_t)pose * G * PART);
  h = 0.0; l = 0.0;
  u64 n_matched = 0, n_skipped = 0;
  for (int g = lane / NS; g < G; g += 64 / NS) {
    const double gh = __longlong_as_double((long long)__hip_atomic_load(all + (size_t)g * PART + k, TMY_RLX_AGENT));
    const double gl = __longlong_as_double((long long)__hip_atomic_load(all + (size_t)g * PART + NS + k, TMY_RLX_AGENT));
    dd_add(h, l, gh, gl);
  }
  dd_add(h, l, lane_xor_d<32>(h), lane_xor_d<32>(l));
  for (int g = 0; g < G; ++g) {
    n_matched += __hip_atomic_load(cnts + 2 * g, TMY_RLX_AGENT);
    n_skipped += __hip_atomic_load(cnts + 2 * g + 1, TMY_RLX_AGENT);
  }
  const u64 n_considered = (u64)lw * (u64)lh;
  const float f = dd_to_float(h, l);
  unsigned wd = tail;
  wd = lane < 28 ? __float_as_uint(f) : wd;
  wd = lane == MW_MATCHED ? (unsigned)n_matched : (lane == MW_MATCHED + 1 ? (unsigned)(n_matched >> 32) : wd);
  wd = lane == MW_CONSIDERED ? (unsigned)n_considered : (lane == MW_CONSIDERED + 1 ? (unsigned)(n_considered >> 32) : wd);
  wd = lane == MW_SKIPPED ? (unsigned)n_skipped : (lane == MW_SKIPPED + 1 ? (unsigned)(n_skipped >> 32) : wd);
  if (lane < MW_END) rec[lane] = wd;
}

namespace {
// What a checked track job is on the host: its launch constants but the depth plane of a pyramid frame, and its parameters.
struct TmyTrackJob {
  TsdfManyTrackJob d;
  revo_map_tsdf_track_params pp;
};

// Every job's own rules, in revo_map_tsdf_track_eval's order, with nothing enqueued.  who: the entry point's name.
int tmy_track_check(const char* who, revo_map* m, int n_jobs, const revo_map_tsdf_track_job* jobs, std::vector<TmyTrackJob>* out) {
  if (n_jobs < 1 || n_jobs > TSDF_MANY_MAX_JOBS) return fail(REVO_ERR_INVALID_ARG, std::string(who) + ": n_jobs must be 1 .. 1024");
  out->resize(n_jobs);
  for (int i = 0; i < n_jobs; ++i) {
    const revo_map_tsdf_track_job& j = jobs[i];
    TmyTrackJob& t = (*out)[i];
    const std::string at = std::string(who) + ": job " + std::to_string(i) + ": ";
    revo_map* jm = nullptr;
    TRY(tmy_job_map(m, j.map, at, &jm));
    if (!j.tsdf || !j.poses) return fail(REVO_ERR_INVALID_ARG, at + "null argument");
    size_t cells = 0;
    if (const char* why = map_df_box_check(&j.box, &cells)) return fail(REVO_ERR_INVALID_ARG, at + why);
    TRY(map_check_aligned((uintptr_t)j.tsdf, 16, at + "the device volume is"));
    if (!std::isfinite(j.trunc) || !(j.trunc > 0.0f)) return fail(REVO_ERR_INVALID_ARG, at + "trunc must be finite and > 0");
    if (const char* why = tsdf_track_params_check(&j.prm, j.trunc, &t.pp)) return fail(REVO_ERR_INVALID_ARG, at + why);
    revo_map_carve_view fv = j.frame;  // its pose is not read: an identity in its place
    for (int e = 0; e < 16; ++e) fv.T_w_c[e] = e % 5 == 0 ? 1.0f : 0.0f;
    CarveView v;
    TRY(tmy_view_check(m, &fv, at, &v));
    if (!tmy_on_device(j.tsdf, m->g.device)) return fail(REVO_ERR_INVALID_ARG, at + "the volume is not in device memory of the map's device");
    TsdfTrackK& k = t.d.k;
    k.vol = TsdfRayK{};
    k.vol.tsdf = j.tsdf;
    k.vol.box = j.box;
    k.vol.voxel = jm->voxel; k.vol.step = jm->voxel;
    k.vol.min_weight = t.pp.min_weight; k.vol.max_steps = 1u;
    k.cam = TsdfTrackCam{v.fx, v.fy, v.cx, v.cy, v.zmin, v.zmax};
    k.kq = tsdf_track_kq(j.trunc);
    k.max_dist = t.pp.max_dist;
    for (int e = 0; e < 3; ++e) k.centre[e] = t.pp.centre[e];
    t.d.depth = j.frame.depth;
    t.d.w = v.w; t.d.h = v.h; t.d.stride = (int)t.pp.stride;
    t.d.lw = tsdf_track_lattice(v.w, t.d.stride); t.d.lh = tsdf_track_lattice(v.h, t.d.stride);
  }
  return REVO_OK;
}

// The job table of a call on the device: the pyramid frames' planes (the tracker stream is ordered behind their builds), one
// upload.  *max_blocks: the 32 x 8 pixel blocks of the largest lattice.
int tmy_track_begin(revo_map* m, int n_jobs, const revo_map_tsdf_track_job* jobs, std::vector<TmyTrackJob>& tj, size_t* max_blocks) {
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  MapTsdfManyScratch& w = m->tsdfmany;
  *max_blocks = 1;
  for (int i = 0; i < n_jobs; ++i) {
    if (jobs[i].frame.kf) {
      MapSource src;
      TRY(revo_map_source_(const_cast<revo_pyr*>(jobs[i].frame.kf), &src));
      tj[i].d.depth = src.depth;
    }
    *max_blocks = std::max(*max_blocks, (size_t)((tj[i].d.lw + 31) / 32) * (size_t)((tj[i].d.lh + 7) / 8));
  }
  TRY(w.track_jobs.reserve(n_jobs, s));
  for (int i = 0; i < n_jobs; ++i) w.track_jobs.h[i] = tj[i].d;
  TRY(w.track_jobs.upload(n_jobs, s));
  return REVO_OK;
}

// n pose rows (job[i], T16 + 16 i: 4x4 column-major) in one launch, records to d_out (device memory), row after row.  Enqueues
// only: the rows go through the handle's pinned rows (their event is waited for before they are rewritten), the scratch is the
// handle's and is used in stream order.  REVO_MAP_TSDF_TRACK_GROUPS applies as it does to revo_map_tsdf_track_eval.
int tmy_track_launch(revo_map* m, size_t max_blocks, int n, const int* job, const float* const* T16, void* d_out) {
  hipStream_t s = (hipStream_t)m->g.stream;
  MapTsdfManyScratch& w = m->tsdfmany;
  const size_t G = tsdf_many_groups(max_blocks, (size_t)n, env_int("REVO_MAP_TSDF_TRACK_GROUPS", 0, 0, TMK_MAX_GROUPS), TMK_MAX_GROUPS, TMK_MAX_TOTAL);
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_tick = 0, o_cnt = o_tick + up(sizeof(unsigned) * n), o_part = o_cnt + up(sizeof(unsigned) * 2 * G * n),
               total = o_part + up(sizeof(double) * TMK_PART * G * n);
  TRY(w.track_work.reserve(total, s));
  TRY(w.poses.reserve(n, s));
  for (int i = 0; i < n; ++i) {
    const float* T = T16[i];
    TsdfManyPose& row = w.poses.h[i];
    for (int col = 0; col < 3; ++col)
      for (int r = 0; r < 3; ++r) row.p[3 * col + r] = T[4 * col + r];
    for (int r = 0; r < 3; ++r) row.p[9 + r] = T[12 + r];
    row.job = job[i];
    row.pad[0] = row.pad[1] = row.pad[2] = 0;
  }
  TRY(w.poses.upload(n, s));
  TsdfManyTrackK k{};
  k.jobs = w.track_jobs.d;
  k.poses = w.poses.d;
  k.ticket = (unsigned*)(w.track_work.p + o_tick);
  k.cnt = (unsigned*)(w.track_work.p + o_cnt);
  k.part = (double*)(w.track_work.p + o_part);
  k.out = (unsigned*)d_out;
  HIPCHECK(hipMemsetAsync(k.ticket, 0, up(sizeof(unsigned) * n), s));
  hipLaunchKernelGGL(k_map_tsdf_track_many, dim3((unsigned)G, (unsigned)n), dim3(TMK_THREADS), 0, s, k);
  if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(s); return fail(REVO_ERR_HIP, "k_map_tsdf_track_many: the launch failed"); }
  return REVO_OK;
}
}  // namespace

extern "C" int revo_map_tsdf_track_eval_many(revo_map* m, int n_jobs, const revo_map_tsdf_track_job* jobs, revo_map_tsdf_track_info* out,
                                             int device_out) {
  if (!m || !jobs || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  std::vector<TmyTrackJob> tj;
  TRY(tmy_track_check("revo_map_tsdf_track_eval_many", m, n_jobs, jobs, &tj));
  size_t n = 0;
  for (int i = 0; i < n_jobs; ++i) {
    if (jobs[i].n_poses < 1) return fail(REVO_ERR_INVALID_ARG, "revo_map_tsdf_track_eval_many: job " + std::to_string(i) + ": n_poses must be >= 1");
    n += (size_t)jobs[i].n_poses;
    if (n > TSDF_TRACK_MAX_POSES) return fail(REVO_ERR_INVALID_ARG, "revo_map_tsdf_track_eval_many: the jobs have more than 4096 poses in total");
  }
  TRY(map_check_side(device_out, "device_out"));
  if (device_out) TRY(map_check_aligned((uintptr_t)out, 16, "the device output is"));
  hipStream_t s = (hipStream_t)m->g.stream;
  std::vector<int> job(n);
  std::vector<const float*> T16(n);
  size_t at = 0;
  for (int i = 0; i < n_jobs; ++i)
    for (int p = 0; p < jobs[i].n_poses; ++p, ++at) { job[at] = i; T16[at] = jobs[i].poses + 16 * (size_t)p; }
  size_t max_blocks = 1;
  int rc = tmy_track_begin(m, n_jobs, jobs, tj, &max_blocks);
  void* d_out = out;
  if (!rc && !device_out) {
    rc = m->tsdfmany.out.reserve(sizeof(revo_map_tsdf_track_info) * n, s);
    d_out = m->tsdfmany.out.p;
  }
  if (!rc) rc = tmy_track_launch(m, max_blocks, (int)n, job.data(), T16.data(), d_out);
  if (!rc && !device_out) {
    const hipError_t e = hipMemcpyAsync(out, d_out, sizeof(revo_map_tsdf_track_info) * n, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) rc = fail(REVO_ERR_HIP, std::string("revo_map_tsdf_track_eval_many: ") + hipGetErrorString(e));
  }
  if (rc) { (void)hipStreamSynchronize(s); return rc; }
  if (!device_out) HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_tsdf_track_many(revo_map* m, int n_jobs, const revo_map_tsdf_track_job* jobs, const revo_map_align_opts* opt,
                                        revo_map_tsdf_track_result* results, int32_t* rounds) {
  if (!m || !jobs || !results) return fail(REVO_ERR_INVALID_ARG, "null argument");
  std::vector<TmyTrackJob> tj;
  TRY(tmy_track_check("revo_map_tsdf_track_many", m, n_jobs, jobs, &tj));
  for (int i = 0; i < n_jobs; ++i) {
    if (!pose_is_finite(jobs[i].poses)) return fail(REVO_ERR_INVALID_ARG, "revo_map_tsdf_track_many: job " + std::to_string(i) + ": T_init is not finite");
    if (jobs[i].n_poses < 0) return fail(REVO_ERR_INVALID_ARG, "revo_map_tsdf_track_many: job " + std::to_string(i) + ": its max_iters (n_poses) must be >= 0");
  }
  revo_map_align_opts o{30, 0, 1e-6, 1e-6, 12};
  if (opt) o = *opt;
  if (o.max_iters < 1) return fail(REVO_ERR_INVALID_ARG, "max_iters must be >= 1");
  hipStream_t s = (hipStream_t)m->g.stream;
  size_t max_blocks = 1;
  int rc = tmy_track_begin(m, n_jobs, jobs, tj, &max_blocks);
  if (!rc) rc = m->tsdfmany.out.reserve(sizeof(revo_map_tsdf_track_info) * n_jobs, s);
  std::vector<AlignStepper<revo_map_tsdf_track_info>> st(n_jobs);
  for (int i = 0; i < n_jobs; ++i) {
    revo_map_align_opts oi = o;
    if (jobs[i].n_poses > 0) oi.max_iters = jobs[i].n_poses;  // the job's own limit
    st[i].begin(jobs[i].poses, tj[i].pp.centre, oi);
  }
  std::vector<int> job(n_jobs);
  std::vector<const float*> T16(n_jobs);
  std::vector<revo_map_tsdf_track_info> recs(n_jobs);
  int32_t n_rounds = 0;
  auto fill = [](const revo_map_tsdf_track_info* r, double* H, double* g) { align_df_system_fill(reinterpret_cast<const revo_map_df_align_info*>(r), H, g); };
  while (!rc) {
    int n = 0;
    for (int i = 0; i < n_jobs; ++i)
      if (st[i].wants()) { job[n] = i; T16[n] = st[i].pose(); ++n; }
    if (!n) break;
    rc = tmy_track_launch(m, max_blocks, n, job.data(), T16.data(), m->tsdfmany.out.p);
    if (!rc) {
      hipError_t e = hipMemcpyAsync(recs.data(), m->tsdfmany.out.p, sizeof(revo_map_tsdf_track_info) * n, hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) rc = fail(REVO_ERR_HIP, std::string("revo_map_tsdf_track_many: ") + hipGetErrorString(e));
    }
    if (rc) break;
    for (int r = 0; r < n; ++r) st[job[r]].feed(recs[r], fill);
    ++n_rounds;
  }
  (void)hipStreamSynchronize(s);
  if (rc) return rc;
  for (int i = 0; i < n_jobs; ++i) {
    revo_map_tsdf_track_result& r = results[i];
    memcpy(r.T, st[i].pose(), sizeof(r.T));
    r.info = st[i].rec;
    r.iterations = st[i].it; r.status = st[i].st;
    r.evaluations = st[i].evals; r.reserved = 0;
  }
  if (rounds) *rounds = n_rounds;
  return REVO_OK;
}
