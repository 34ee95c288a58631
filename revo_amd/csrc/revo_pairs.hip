// revo_pairs.hip -- host-buffer batches (revo_track_pairs_*): job slots over revo_batch, uploads out of the caller's rows.
#include "revo_host_impl.h"

struct revo_pairs_job {
  revo_ctx* ctx = nullptr;
  int n = 0, is_u16 = 0;
  bool busy = false;
  revo_batch* batch = nullptr;
  DevMem<uint8_t> d_bgr;   // [2n][H][W][3]
  DevMem<char> d_depth;    // [2n][H][W] f32 or u16
  DevMem<revo_pair_result> d_res;
  PinnedMem<revo_pair_result> h_res;
  std::vector<float> h_init;          // n x 12
  OwnedEvent ev_h2d, ev_h2d2, ev_done;
  hipStream_t stream = nullptr;       // compute stream of the job (alternates, so job k+1's build overlaps job k's tracker)
  ~revo_pairs_job() { revo_batch_destroy(batch); }
};

void pairs_jobs_release(revo_ctx* c) {
  std::vector<revo_pairs_job*> jobs;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    jobs.swap(c->jobs);
  }
  (void)hipSetDevice(c->device);
  for (revo_pairs_job* j : jobs) {
    if (j->busy && j->ev_done) (void)hipEventSynchronize(j->ev_done);
    delete j;
  }
}

extern "C" int revo_track_pairs_submit(revo_ctx* c, int n, const revo_pair_in* pairs, int depth_is_u16,
                                       double depth_scale_factor, revo_pairs_job** job_out) {
  if (!c || !pairs || !job_out || n <= 0) return fail(REVO_ERR_INVALID_ARG, "bad argument");
  if (depth_is_u16 && !(depth_scale_factor > 0.0)) return fail(REVO_ERR_INVALID_ARG, "depth_scale_factor must be positive");
  HIPCHECK(hipSetDevice(c->device));
  const int w = c->geom.lv[0].w, h = c->geom.lv[0].h;
  const size_t npix = (size_t)w * h, dsz = depth_is_u16 ? 2 : 4;
  for (int i = 0; i < n; ++i) {
    const revo_pair_in& p = pairs[i];
    if (!p.ref_bgr || !p.ref_depth || !p.cur_bgr || !p.cur_depth) return fail(REVO_ERR_INVALID_ARG, "null image pointer");
    if (p.ref_bgr_stride < (size_t)w * 3 || p.cur_bgr_stride < (size_t)w * 3 || p.ref_depth_stride < w * dsz || p.cur_depth_stride < w * dsz)
      return fail(REVO_ERR_INVALID_ARG, "stride smaller than a row");
  }
  revo_pairs_job* j = nullptr;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->copy_stream)
      for (OwnedStream* st : {&c->copy_stream, &c->copy_stream2, &c->pair_streams[0], &c->pair_streams[1]}) TRY(st->create());
    int in_flight = 0;
    for (revo_pairs_job* q : c->jobs) in_flight += q->busy ? 1 : 0;
    if (in_flight >= 3) return fail(REVO_ERR_CAPACITY, "three jobs are in flight: call revo_track_pairs_wait first");
    for (revo_pairs_job* q : c->jobs)
      if (!q->busy && q->n == n && q->is_u16 == (depth_is_u16 ? 1 : 0)) { j = q; break; }
    if (!j) {
      for (size_t k = 0; k < c->jobs.size(); ++k)  // a free slot of another shape makes room (HBM is finite)
        if (!c->jobs[k]->busy && c->jobs.size() >= 3) { delete c->jobs[k]; c->jobs.erase(c->jobs.begin() + k); break; }
      std::unique_ptr<revo_pairs_job> nj(new revo_pairs_job());
      nj->ctx = c; nj->n = n; nj->is_u16 = depth_is_u16 ? 1 : 0;
      TRY(revo_batch_create(c, n, &nj->batch));
      TRY(nj->d_bgr.alloc(2 * (size_t)n * npix * 3));
      TRY(nj->d_depth.alloc(2 * (size_t)n * npix * dsz));
      TRY(nj->d_res.alloc(n));
      TRY(nj->h_res.alloc(n));
      nj->h_init.resize(12 * (size_t)n);
      for (OwnedEvent* e : {&nj->ev_h2d, &nj->ev_h2d2, &nj->ev_done}) TRY(e->create());
      c->jobs.push_back(j = nj.release());
    }
    j->busy = true;
    j->stream = c->pair_streams[c->jobs_submitted++ & 1];
  }
  // H2D straight from the caller's rows (no host-side staging copy): one copy per plane (strided only when the
  // rows are padded), colour planes and depth planes on two streams so that two DMA engines work
  // HIP multiplexes its streams over a few hardware queues, and a copy stream that shares a queue with a compute stream
  // waits behind that stream's kernels: that, not the link, is why the f32 path reaches 20-24 GB/s where the u16 path
  // reaches 40 (profiles/r03_host_buffer_streams.txt: GPU_MAX_HW_QUEUES=8 lifts f32 to 45 GB/s -- and costs the pipelined
  // device-buffer batches a third of their throughput, so the library does not ask for it; swapping the planes' streams
  // helped in one order of events and not in another: the mapping depends on the process's stream history).
  hipStream_t cs = c->copy_stream, cs2 = c->copy_stream2;  // cs: colour, cs2: depth
  // Any failure below must not leave the slot busy for ever (three of those and the context only ever answers
  // REVO_ERR_CAPACITY), nor return while the DMA engines may still be reading the caller's buffers.
  struct SlotGuard {
    revo_ctx* c; revo_pairs_job* j; hipStream_t a, b;
    ~SlotGuard() {
      if (!j) return;
      (void)hipStreamSynchronize(a); (void)hipStreamSynchronize(b);
      if (j->stream) (void)hipStreamSynchronize(j->stream);
      std::lock_guard<std::mutex> lk(c->mu);
      j->busy = false;
    }
  } slot_guard{c, j, cs, cs2};
  bool any_init = false;
  // Frames that lie back to back in host memory (a decoder that fills one job-sized slab per plane type: [2n][H][W][3] colours,
  // [2n][H][W] depths) travel in ONE copy per run of adjacent frames instead of one per frame: the DMA engines reach the link's
  // rate only with large transfers (profiles/r03_h2d_chunk_rates.txt: 0.6 MB pieces 43 GB/s on two streams, 1.2 MB 53 GB/s; a
  // whole job's planes are 59 + 39 MB).  Frames that are not adjacent, or whose rows are padded, go one by one as before.
  // Runs are cut at 64 MB: measured (profiles/r06_h2d_run_sizes.txt) u16 depth 39 -> 49 GB/s, f32 43 -> 47 GB/s with the cut,
  // but 39 GB/s when a job's 78 MB f32 depth slab travels as ONE copy (it then monopolises its engine past the colour copy).
  const size_t max_run = (size_t)c->knobs.h2d_max_run_mb << 20;  // REVO_H2D_MAX_RUN_MB: upper bound of one merged copy
  RowCopier run_c{hipMemcpyHostToDevice, h, cs, max_run}, run_d{hipMemcpyHostToDevice, h, cs2, max_run};
  for (int i = 0; i < n; ++i) {
    const revo_pair_in& p = pairs[i];
    const uint8_t* bs[2] = {p.ref_bgr, p.cur_bgr};
    const size_t bst[2] = {p.ref_bgr_stride, p.cur_bgr_stride};
    const void* ds[2] = {p.ref_depth, p.cur_depth};
    const size_t dst[2] = {p.ref_depth_stride, p.cur_depth_stride};
    for (int k = 0; k < 2; ++k) {
      const size_t f = 2 * (size_t)i + k;
      HIPCHECK(run_c.add(j->d_bgr + f * npix * 3, bs[k], bst[k], (size_t)w * 3));
      HIPCHECK(run_d.add(j->d_depth + f * npix * dsz, ds[k], dst[k], w * dsz));
    }
    float* q = j->h_init.data() + 12 * (size_t)i;
    if (p.use_init) { memcpy(q, p.R_init, sizeof(float) * 9); memcpy(q + 9, p.T_init, sizeof(float) * 3); any_init = true; }
    else { const float I[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}; memcpy(q, I, sizeof(I)); }
  }
  HIPCHECK(run_c.flush());
  HIPCHECK(run_d.flush());
  HIPCHECK(hipEventRecord(j->ev_h2d2, cs2));
  HIPCHECK(hipStreamWaitEvent(cs, j->ev_h2d2, 0));
  HIPCHECK(hipEventRecord(j->ev_h2d, cs));
  hipStream_t s = j->stream;
  HIPCHECK(hipStreamWaitEvent(s, j->ev_h2d, 0));
  int rc = depth_is_u16 ? revo_batch_build_u16(j->batch, j->d_bgr, (const uint16_t*)j->d_depth.p, depth_scale_factor, s)
                        : revo_batch_build_borrow(j->batch, j->d_bgr, (const float*)j->d_depth.p, s);  // the job's own staging
  if (!rc) rc = revo_batch_track_only(j->batch, any_init ? j->h_init.data() : nullptr, j->d_res, s);
  if (rc) return rc;
  HIPCHECK(hipMemcpyAsync(j->h_res, j->d_res, sizeof(revo_pair_result) * n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipEventRecord(j->ev_done, s));
  // the caller's buffers are free again once the DMA has read them; the kernels keep running
  HIPCHECK(hipEventSynchronize(j->ev_h2d));
  slot_guard.j = nullptr;
  *job_out = j;
  return REVO_OK;
}

extern "C" int revo_track_pairs_wait(revo_pairs_job* j, revo_pair_out* out) {
  if (!j || !j->busy) return fail(REVO_ERR_INVALID_ARG, "not a job in flight");
  HIPCHECK(hipSetDevice(j->ctx->device));
  hipError_t e = hipEventSynchronize(j->ev_done);
  int rc = REVO_OK;
  if (e != hipSuccess) rc = fail(REVO_ERR_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(e));
  if (!rc) {
    if (out) memcpy(out, j->h_res, sizeof(revo_pair_result) * j->n);
    for (int i = 0; i < j->n && !rc; ++i)
      if (j->h_res[i].flags & 8)
        rc = fail(REVO_ERR_HIP, "tracker: pair " + std::to_string(i) + ": the workgroups of the pair could not exchange partial sums "
                  "in time (device shared with another process?) -- its pose is not valid");
  }
  std::lock_guard<std::mutex> lk(j->ctx->mu);
  j->busy = false;
  return rc;
}

extern "C" int revo_track_pairs(revo_ctx* c, int n, const revo_pair_in* pairs, int depth_is_u16, double depth_scale_factor,
                                revo_pair_out* out) {
  revo_pairs_job* j = nullptr;
  const int rc = revo_track_pairs_submit(c, n, pairs, depth_is_u16, depth_scale_factor, &j);
  if (rc) return rc;
  return revo_track_pairs_wait(j, out);
}
