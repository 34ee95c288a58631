// revo_map_tsdf_ray_many.hip -- views of many surfaces in one call: revo_map_tsdf_raycast_many, the ray casts of n
// (volume, views) jobs in one mask launch over the distinct volumes and one march launch over all views.  Contract:
// include/revo_hip.h.  Every output is revo_map_tsdf_raycast's byte for byte: the mask's cell rule and the march block are the ones
// its kernels call (revo_tsdf_ray_dev.h), the per-job checks are its own functions; this unit holds the tables, how a block finds
// its volume or its job (revo_tsdf_ray_many_host.h), the finish that hands the counters to the jobs, and the entry point.
#include "revo_map_impl.h"
#include "revo_tsdf_ray_host.h"
#include "revo_tsdf_ray_dev.h"
#include "revo_tsdf_many_host.h"
#include "revo_tsdf_ray_many_host.h"

static_assert(sizeof(revo_map_tsdf_ray_job) == 120 && offsetof(revo_map_tsdf_ray_job, map) == 0 && offsetof(revo_map_tsdf_ray_job, box) == 8 &&
              offsetof(revo_map_tsdf_ray_job, prm) == 32 && offsetof(revo_map_tsdf_ray_job, tsdf) == 48 && offsetof(revo_map_tsdf_ray_job, color) == 56 &&
              offsetof(revo_map_tsdf_ray_job, n_views) == 64 && offsetof(revo_map_tsdf_ray_job, reserved) == 68 && offsetof(revo_map_tsdf_ray_job, views) == 72 &&
              offsetof(revo_map_tsdf_ray_job, depth) == 80 && offsetof(revo_map_tsdf_ray_job, normal) == 88 && offsetof(revo_map_tsdf_ray_job, bgr) == 96 &&
              offsetof(revo_map_tsdf_ray_job, hits) == 104 && offsetof(revo_map_tsdf_ray_job, info) == 112, "the ray job is the documented layout");
static_assert(sizeof(revo_map_tsdf_ray_info) == 4 * TSDF_RAY_MANY_LINE_TICKET && TSDF_RAY_MANY_LINE_TICKET < TSDF_RAY_MANY_LINE,
              "a job's counter line is the info record, in front of its ticket");

struct TsdfRayManyVol {  // one distinct volume of the mask launch, in device memory
  const revo_map_tsdf_cell* tsdf;
  unsigned* mask;
  revo_map_df_box box;
  unsigned cells, min_weight;
  int nby, nbz;
  unsigned first_block, pad;  // the volume's blocks of the launch: tsdf_many_find
};
struct TsdfRayManyJob {  // one job of the march launch, in device memory
  TsdfRayK k;            // with the mask of the job's distinct volume
  unsigned* info;        // the job's own record and hit words, or NULL
  unsigned* hits;
  unsigned first_view, n_views;  // the job's view rows
  unsigned blocks, pad;          // the blocks of the march launch that work for the job: its views' tiles
};
struct TsdfRayManyView {  // one view row of the march launch: the single unit's row, and the row's job
  TsdfRayView v;          // v.hits: the row's word of the scratch
  int job, pad;
};
struct TsdfRayManyK {
  const TsdfRayManyJob* jobs;
  const TsdfRayManyView* views;
  unsigned* lines;      // TSDF_RAY_MANY_LINE words per job, zero before the launch: the counters and the job's ticket
  unsigned* hit_words;  // one per view row, zero before the launch
};

// Grid: the cells of the distinct volumes, one volume after another, 256 cells a block (tsdf_many_find over first_block).  A block
// runs k_tsdf_ray_mask's body for its cells of its volume; the only atomic is the integer atomicOr, skipped where a load finds the
// bit set.
__global__ void __launch_bounds__(256) k_tsdf_ray_mask_many(const TsdfRayManyVol* __restrict__ vols, int n_vols) {
  const int vol = tsdf_many_find(n_vols, blockIdx.x, [&](int j) { return vols[j].first_block; });
  const TsdfRayManyVol V = vols[vol];  // a uniform address: scalar loads
  const unsigned c = (blockIdx.x - V.first_block) * 256u + threadIdx.x;
  if (c >= V.cells) return;
  tsdf_ray_mask_cell(V.tsdf, V.box, c, V.min_weight, V.nby, V.nbz, V.mask);
}

// The job's counter line and hit words into its own record and array; the threads 0 .. 15 take the line's words, the threads
// 64 .. 127 the hit words.  For a block of at least 128 threads.
__device__ __forceinline__ void trm_hand_over(const TsdfRayManyJob& J, const unsigned* line, const unsigned* hit_words) {
  const unsigned tid = threadIdx.x;
  if (tid < TSDF_RAY_MANY_LINE_TICKET && J.info) J.info[tid] = __hip_atomic_load(line + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (tid >= 64 && tid - 64 < J.n_views && J.hits)
    J.hits[tid - 64] = __hip_atomic_load(hit_words + J.first_view + (tid - 64), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Grid (the largest view's 32 x 8 blocks, all view rows of the call).  A row carries its job; blocks past a view's tiles leave at
// once.  The job's TsdfRayK and the view are read through uniform addresses; the body is k_tsdf_raycast's, with the job's line of
// the scratch as its counters and the row's word of the scratch as its hit count.
// TICKET: k_tsdf_fuse_many's finish -- the counters have left the CU, then the block draws the job's ticket, and the block that
// draws the last one hands the line and the hit words over.  No release fence stands in a block's way.  Without it a trailing
// launch (k_tsdf_ray_finish_many) hands them over.
template <bool TICKET>
__global__ void __launch_bounds__(256) k_tsdf_raycast_many(const TsdfRayManyK a) {
  __shared__ TsdfRayTally s;
  __shared__ unsigned s_last;
  const TsdfRayManyView& row = a.views[blockIdx.y];
  const unsigned bw = (unsigned)(row.v.v.w + 31) / 32, bh = (unsigned)(row.v.v.h + 7) / 8;
  if (blockIdx.x >= bw * bh) return;
  const int job = row.job;
  const TsdfRayK K = a.jobs[job].k;  // a uniform address: scalar loads
  unsigned* const line = a.lines + (size_t)job * TSDF_RAY_MANY_LINE;
  tsdf_ray_view_block(K, row.v, blockIdx.x, s, (u64*)line);
  if (!TICKET) return;
  const TsdfRayManyJob& J = a.jobs[job];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's counters have left this CU ...
  __syncthreads();                                  // ... and so have every thread's of the block, before its ticket is drawn
  if (threadIdx.x == 0)
    s_last = __hip_atomic_fetch_add(line + TSDF_RAY_MANY_LINE_TICKET, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == J.blocks - 1u ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  // the last block of the job to arrive: every block's counters are in the line and the hit words
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  trm_hand_over(J, line, a.hit_words);
}

// One block per job, behind the march launch on the stream: the kernel boundary orders the counters before the copy.
__global__ void __launch_bounds__(128) k_tsdf_ray_finish_many(const TsdfRayManyK a) {
  trm_hand_over(a.jobs[blockIdx.x], a.lines + (size_t)blockIdx.x * TSDF_RAY_MANY_LINE, a.hit_words);
}

namespace {
// Whether a pointer is device memory of `dev` (not host, not another device).  A call names thousands of pointers into a few
// allocations, so an allocation that has been asked about is remembered for the rest of the call.
struct TrmDeviceMemory {
  int dev;
  std::vector<std::pair<uintptr_t, size_t>> known;
  bool has(const void* p) {
    const uintptr_t u = (uintptr_t)p;
    for (const auto& r : known)
      if (u >= r.first && u - r.first < r.second) return true;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (a.type != hipMemoryTypeDevice || a.device != dev) return false;
    hipDeviceptr_t base = nullptr;
    size_t bytes = 0;
    if (hipMemGetAddressRange(&base, &bytes, (hipDeviceptr_t)const_cast<void*>(p)) == hipSuccess && bytes) known.emplace_back((uintptr_t)base, bytes);
    else (void)hipGetLastError();
    return true;
  }
};
}  // namespace

// REVO_MAP_TSDF_RAY_MASK=0: the plain march, as in the single call.  REVO_MAP_TSDF_RAY_MANY_TICKET=1: the ticket finish in place of
// the trailing launch (profiles/multi_surface_ray_rates.py measures both).
extern "C" int revo_map_tsdf_raycast_many(revo_map* m, int n_jobs, const revo_map_tsdf_ray_job* jobs) {
  if (!m || !jobs) return fail(REVO_ERR_INVALID_ARG, "null argument");
  const std::string who = "revo_map_tsdf_raycast_many: ";
  if (n_jobs < 1 || n_jobs > TSDF_MANY_MAX_JOBS) return fail(REVO_ERR_INVALID_ARG, who + "n_jobs must be 1 .. 1024");
  size_t total_views = 0;
  for (int i = 0; i < n_jobs; ++i) {
    if (jobs[i].n_views < 1 || jobs[i].n_views > TSDF_RAY_MAX_VIEWS) return fail(REVO_ERR_INVALID_ARG, who + "job " + std::to_string(i) + ": n_views must be 1 .. 64 views");
    total_views += (size_t)jobs[i].n_views;
  }
  if (total_views > TSDF_RAY_MANY_MAX_VIEWS) return fail(REVO_ERR_INVALID_ARG, who + "the jobs have more than 4096 views in total");
  const int dev = m->g.device;
  TrmDeviceMemory mem{dev, {}};
  const CarveCam cam{m->g.fx, m->g.fy, m->g.cx, m->g.cy, m->g.dmin, m->g.dmax};
  std::vector<TsdfRayManyJob> hj(n_jobs);
  std::vector<TsdfRayManyView> hv(total_views);
  std::vector<TsdfRayManyIn> in(n_jobs);
  std::vector<std::pair<uintptr_t, size_t>> outputs, volumes;
  outputs.reserve(3 * total_views + 2 * (size_t)n_jobs);
  volumes.reserve(2 * (size_t)n_jobs);
  int max_blocks = 0;
  size_t row = 0;
  for (int i = 0; i < n_jobs; ++i) {  // every job's own rules: the single call's, with its functions
    const revo_map_tsdf_ray_job& j = jobs[i];
    TsdfRayManyJob& d = hj[i];
    const std::string at = who + "job " + std::to_string(i) + ": ";
    revo_map* jm = j.map ? j.map : m;
    if (jm->ctx != m->ctx) return fail(REVO_ERR_INVALID_ARG, at + "the job's map belongs to another context");
    if (!j.tsdf || !j.views || !j.depth) return fail(REVO_ERR_INVALID_ARG, at + "null argument");
    if (j.reserved) return fail(REVO_ERR_INVALID_ARG, at + "a reserved word is not 0");
    if (j.bgr && !j.color) return fail(REVO_ERR_INVALID_ARG, at + "colour images need the colour volume");
    size_t cells = 0;
    if (const char* why = map_df_box_check(&j.box, &cells)) return fail(REVO_ERR_INVALID_ARG, at + why);
    TRY(map_check_aligned((uintptr_t)j.tsdf | (uintptr_t)j.color, 16, at + "the device volume is"));
    TRY(map_check_aligned((uintptr_t)j.hits | (uintptr_t)j.info, 16, at + "hits or info is"));
    revo_map_tsdf_ray_params pp;
    if (const char* why = tsdf_ray_params_check(&j.prm, jm->voxel, &pp)) return fail(REVO_ERR_INVALID_ARG, at + why);
    if (!mem.has(j.tsdf) || (j.color && !mem.has(j.color)) || (j.hits && !mem.has(j.hits)) || (j.info && !mem.has(j.info)))
      return fail(REVO_ERR_INVALID_ARG, at + "a volume or a record is not in device memory of the map's device");
    volumes.emplace_back((uintptr_t)j.tsdf, sizeof(revo_map_tsdf_cell) * cells);
    if (j.color) volumes.emplace_back((uintptr_t)j.color, sizeof(revo_map_tsdf_color) * cells);
    if (j.hits) outputs.emplace_back((uintptr_t)j.hits, sizeof(uint32_t) * (size_t)j.n_views);
    if (j.info) outputs.emplace_back((uintptr_t)j.info, sizeof(revo_map_tsdf_ray_info));
    unsigned blocks = 0;
    for (int v = 0; v < j.n_views; ++v, ++row) {
      const std::string vat = at + "view " + std::to_string(v) + ": ";
      float* const dp = j.depth[v];
      float* const np_ = j.normal ? j.normal[v] : nullptr;
      uint8_t* const bp = j.bgr ? j.bgr[v] : nullptr;
      if (!dp || (j.normal && !np_) || (j.bgr && !bp)) return fail(REVO_ERR_INVALID_ARG, vat + "null output");
      TRY(map_check_aligned((uintptr_t)dp | (uintptr_t)np_ | (uintptr_t)bp, 16, vat + "a device output is"));
      TsdfRayManyView& r = hv[row];
      if (const char* why = ray_view_check(&j.views[v], cam, &r.v.v)) return fail(REVO_ERR_INVALID_ARG, vat + why);
      if (!mem.has(dp) || (np_ && !mem.has(np_)) || (bp && !mem.has(bp)))
        return fail(REVO_ERR_INVALID_ARG, vat + "an image is not in device memory of the map's device");
      const size_t np = (size_t)r.v.v.w * r.v.v.h;
      outputs.emplace_back((uintptr_t)dp, np * 4);
      if (np_) outputs.emplace_back((uintptr_t)np_, np * 12);
      if (bp) outputs.emplace_back((uintptr_t)bp, np * 3);
      r.v.depth = dp; r.v.normal = np_; r.v.bgr = bp; r.v.hits = nullptr;
      r.job = i; r.pad = 0;
      const int vb = ((r.v.v.w + 31) / 32) * ((r.v.v.h + 7) / 8);
      blocks += (unsigned)vb;
      max_blocks = std::max(max_blocks, vb);
    }
    d.k = TsdfRayK{};
    d.k.tsdf = j.tsdf; d.k.color = j.color;
    d.k.box = j.box;
    d.k.nby = tsdf_ray_blocks(j.box.n[1]); d.k.nbz = tsdf_ray_blocks(j.box.n[2]);
    d.k.voxel = jm->voxel; d.k.step = pp.step;
    d.k.min_weight = pp.min_weight; d.k.max_steps = pp.max_steps;
    d.info = (unsigned*)j.info; d.hits = (unsigned*)j.hits;
    d.n_views = (unsigned)j.n_views;
    d.blocks = blocks; d.pad = 0;
    in[i] = TsdfRayManyIn{(uintptr_t)j.tsdf, j.box, pp.min_weight, j.n_views};
  }
  if (tsdf_ray_many_overlap(outputs, volumes)) return fail(REVO_ERR_INVALID_ARG, who + "two outputs of the call, or an output and a volume, share memory");
  const bool use_mask = env_int("REVO_MAP_TSDF_RAY_MASK", 1, 0, 1) != 0;
  const bool ticket = env_int("REVO_MAP_TSDF_RAY_MANY_TICKET", 0, 0, 1) != 0;
  TsdfRayManyPlan plan;
  tsdf_ray_many_plan(in, use_mask, &plan);
  const int n_vols = (int)plan.job_of_vol.size();
  HIPCHECK(hipSetDevice(dev));
  hipStream_t s = (hipStream_t)m->g.stream;
  MapTsdfRayManyScratch& w = m->tsdfraymany;
  TRY(w.jobs.reserve(n_jobs, s));  // waits until the previous call's upload has read the pinned rows
  TRY(w.views.reserve((int)total_views, s));
  TRY(w.vols.reserve(n_vols, s));
  TRY(w.work.reserve(plan.total, s));
  unsigned* const d_lines = (unsigned*)w.work.p;
  unsigned* const d_hits = (unsigned*)(w.work.p + plan.off_hits);
  char* const d_masks = w.work.p + plan.off_masks;
  for (int i = 0; i < n_jobs; ++i) {
    hj[i].first_view = plan.first_view[i];
    hj[i].k.mask = use_mask ? (const uint32_t*)(d_masks + plan.mask_off[plan.vol_of_job[i]]) : nullptr;
  }
  for (size_t r = 0; r < total_views; ++r) hv[r].v.hits = d_hits + r;
  memcpy(w.jobs.h, hj.data(), sizeof(TsdfRayManyJob) * n_jobs);
  memcpy(w.views.h, hv.data(), sizeof(TsdfRayManyView) * total_views);
  if (use_mask)
    for (int v = 0; v < n_vols; ++v) {
      const TsdfRayManyJob& J = hj[plan.job_of_vol[v]];
      TsdfRayManyVol& V = w.vols.h[v];
      V.tsdf = J.k.tsdf;
      V.mask = (unsigned*)(d_masks + plan.mask_off[v]);
      V.box = J.k.box;
      V.cells = (unsigned)((size_t)J.k.box.n[0] * J.k.box.n[1] * J.k.box.n[2]);
      V.min_weight = J.k.min_weight;
      V.nby = J.k.nby; V.nbz = J.k.nbz;
      V.first_block = plan.first_block[v]; V.pad = 0;
    }
  TRY(w.jobs.upload(n_jobs, s, false));
  if (use_mask) TRY(w.vols.upload(n_vols, s, false));
  TRY(w.views.upload((int)total_views, s));  // one event behind the three uploads guards the three sets of pinned rows
  TsdfRayManyK a{};
  a.jobs = w.jobs.d; a.views = w.views.d;
  a.lines = d_lines; a.hit_words = d_hits;
  HIPCHECK(hipMemsetAsync(w.work.p, 0, plan.total, s));  // the lines, the tickets, the hit words and the masks: one memset
  if (use_mask) {
    hipLaunchKernelGGL(k_tsdf_ray_mask_many, dim3((unsigned)plan.mask_blocks), dim3(256), 0, s, w.vols.d, n_vols);
    HIPCHECK(hipGetLastError());
  }
  const dim3 grid((unsigned)max_blocks, (unsigned)total_views);
  if (ticket) {
    hipLaunchKernelGGL(k_tsdf_raycast_many<true>, grid, dim3(256), 0, s, a);
    HIPCHECK(hipGetLastError());
  } else {
    hipLaunchKernelGGL(k_tsdf_raycast_many<false>, grid, dim3(256), 0, s, a);
    HIPCHECK(hipGetLastError());
    hipLaunchKernelGGL(k_tsdf_ray_finish_many, dim3((unsigned)n_jobs), dim3(128), 0, s, a);
    HIPCHECK(hipGetLastError());
  }
  return REVO_OK;
}
