// revo_map_edit.hip -- changing a map by what another map or a view says: revo_map_pose_raw, revo_map_merge_posed and
// revo_map_subtract_posed (a map under a rigid pose), revo_map_carve_eval and revo_map_carve (free-space carving).
// Contracts: include/revo_hip.h; DESIGN 18 and 19.
#include "revo_map_impl.h"

// ------------------------------------------------------------------------------------------- maps under a pose (18) --
struct MapPose { float r00, r01, r02, r10, r11, r12, r20, r21, r22, tx, ty, tz, voxel; };  // r_ij: row i, column j; the destination edge
struct MapPoseK {
  const u64* keys; const MapVal* vals; unsigned cap;  // the source table
  u64 min_count;
  MapPose T;
  ulonglong2* out; unsigned cap_out;  // the posed records, at most cap_out of them (0: count only)
  u64* info;                          // one 64-byte line: revo_map_pose_info's seven counters, then "a bad record was met"
};
enum { POSED_MOVED = 0, POSED_DROPPED = 1, POSED_SKIPPED = 2, POSED_BAD = 3 };

// one axis of k_map_walk's test: the voxel index of p, and whether p and the index are in range (NaN / inf fail every comparison)
__device__ __forceinline__ bool map_posed_axis(float p, float voxel, int& k) {
  const float f = floorf(__fdiv_rn(p, voxel));
  const bool ok = fabsf(p) < 2048.0f && f >= -1048576.0f && f <= 1048575.0f;
  k = ok ? (int)f : 0;
  return ok;
}
// The posed record of a voxel with count n >= 1 and coordinate sums sx, sy, sz: its key and its three sums n * q (the count
// and the colour sums are carried by the caller).  The one text of the contract's arithmetic.
__device__ __forceinline__ int map_posed_record(u64 n, u64 sx, u64 sy, u64 sz, const MapPose& T, u64 min_count, u64& key, u64& qx,
                                                u64& qy, u64& qz) {
  if (n >> 32) return POSED_BAD;
  if (n < min_count) return POSED_SKIPPED;
  const double inv = (double)n;
  const float px = map_mean(sx, inv), py = map_mean(sy, inv), pz = map_mean(sz, inv);
  const float x = ((T.r00 * px + T.r01 * py) + T.r02 * pz) + T.tx;
  const float y = ((T.r10 * px + T.r11 * py) + T.r12 * pz) + T.ty;
  const float z = ((T.r20 * px + T.r21 * py) + T.r22 * pz) + T.tz;
  int kx, ky, kz;
  bool ok = map_posed_axis(x, T.voxel, kx);
  ok = map_posed_axis(y, T.voxel, ky) && ok;
  ok = map_posed_axis(z, T.voxel, kz) && ok;
  if (!ok) return POSED_DROPPED;
  key = map_key(kx, ky, kz);
  const long long m = (long long)n;  // < 2^32, and |q| <= 2^31: the products are exact
  qx = (u64)(m * (long long)rintf(x * 1048576.0f));
  qy = (u64)(m * (long long)rintf(y * 1048576.0f));
  qz = (u64)(m * (long long)rintf(z * 1048576.0f));
  return POSED_MOVED;
}

// One thread per slot of the source table: the value as four 16-byte loads, the posed record in registers, the moved ones
// compacted as k_map_export compacts (LDS counter, one global atomic per block), the seven counters through LDS to the info
// line with one atomic per block and counter.
__global__ void __launch_bounds__(256) k_map_pose(const MapPoseK a) {
  __shared__ unsigned s_n, s_base, s_bad;
  __shared__ unsigned s_vox[4];  // voxels in, moved, dropped, skipped
  __shared__ u64 s_pts[3];       // points moved, dropped, skipped
  if (threadIdx.x < 4) s_vox[threadIdx.x] = 0;
  if (threadIdx.x < 3) s_pts[threadIdx.x] = 0;
  if (threadIdx.x == 0) { s_n = 0; s_bad = 0; }
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  const u64 skey = i < a.cap ? a.keys[i] : MAP_EMPTY;
  MapRec r{};
  int what = -1;
  if (skey != MAP_EMPTY) {
    r = map_rec_from_slot(a.vals + i, skey);
    if (r.n() != 0) {  // a committed voxel has count >= 1
      u64 key = 0, qx = 0, qy = 0, qz = 0;
      what = map_posed_record(r.n(), r.b.x, r.b.y, r.c.x, a.T, a.min_count, key, qx, qy, qz);
      r.a.x = key; r.b = make_ulonglong2(qx, qy); r.c.x = qz;  // the count and the colour sums stay
      if (what == POSED_BAD) {
        atomicOr(&s_bad, 1u);
      } else {
        atomicAdd(&s_vox[0], 1u);
        atomicAdd(&s_vox[1 + what], 1u);
        atomicAdd(&s_pts[what], r.n());
      }
    }
  }
  const bool sel = what == POSED_MOVED;
  const unsigned o = map_compact_begin(sel, s_n);
  __syncthreads();
  map_compact_end(s_n, s_base, &a.info[1]);  // voxels_moved doubles as the compaction's counter
  if (threadIdx.x == 1 && s_vox[0]) atomicAdd(&a.info[0], (u64)s_vox[0]);
  if ((threadIdx.x == 2 || threadIdx.x == 3) && s_vox[threadIdx.x]) atomicAdd(&a.info[threadIdx.x], (u64)s_vox[threadIdx.x]);
  if (threadIdx.x >= 4 && threadIdx.x < 7 && s_pts[threadIdx.x - 4]) atomicAdd(&a.info[threadIdx.x], s_pts[threadIdx.x - 4]);
  if (threadIdx.x == 7 && s_bad) atomicOr(&a.info[7], 1ull);
  __syncthreads();
  if (!sel) return;
  const unsigned j = s_base + o;
  if (j < a.cap_out) map_rec_store(a.out, j, r);
}

static_assert(sizeof(revo_map_pose_info) == 64 && offsetof(revo_map_pose_info, voxels_in) == 0 && offsetof(revo_map_pose_info, voxels_moved) == 8 &&
              offsetof(revo_map_pose_info, voxels_dropped) == 16 && offsetof(revo_map_pose_info, voxels_skipped) == 24 &&
              offsetof(revo_map_pose_info, points_moved) == 32 && offsetof(revo_map_pose_info, points_dropped) == 40 &&
              offsetof(revo_map_pose_info, points_skipped) == 48 && offsetof(revo_map_pose_info, reserved) == 56,
              "the info record is the kernel's counter line");

// the pose rules of the three calls, checked before any table is touched
static int pose_check(const float* T, float voxel_dst) {
  if (!std::isfinite(voxel_dst) || !(voxel_dst > 0.0f)) return fail(REVO_ERR_INVALID_ARG, "the destination's voxel edge must be finite and > 0");
  if (!pose_is_finite(T)) return fail(REVO_ERR_INVALID_ARG, "T_dst_src is not finite");
  if (!pose_is_orthogonal(T)) return fail(REVO_ERR_INVALID_ARG, "the rotation of T_dst_src is not orthogonal");
  return REVO_OK;
}

// One k_map_pose launch over src's table on stream s (src has been waited for), then the wait for its counters.  d_out NULL:
// the records go into the run's own buffer (room for every voxel of src), which lives as long as the run.
struct MapPoseRun {
  DevScratch buf;
  revo_map_pose_info info{};
  const ulonglong2* recs() const { return (const ulonglong2*)(buf.p + 256); }
};
static int pose_run(MapPoseRun* r, revo_map* src, hipStream_t s, size_t voxels, const float* T, float voxel_dst, size_t min_count,
                    ulonglong2* d_out, size_t cap_out, bool own) {
  const size_t room = own ? std::max<size_t>(voxels, 1) : 0;
  if (!r->buf.p) TRY(r->buf.alloc(256 + sizeof(revo_map_voxel_raw) * room));
  MapPoseK a{};
  a.keys = src->d_keys; a.vals = src->d_vals; a.cap = (unsigned)src->cap;
  a.min_count = (u64)std::max<size_t>(min_count, 1);
  a.T = MapPose{T[0], T[4], T[8], T[1], T[5], T[9], T[2], T[6], T[10], T[12], T[13], T[14], voxel_dst};
  a.out = own ? (ulonglong2*)(r->buf.p + 256) : d_out;
  a.cap_out = (unsigned)std::min<size_t>(own ? room : cap_out, MAP_MAX_CAP);
  a.info = (u64*)r->buf.p;
  HIPCHECK(hipMemsetAsync(r->buf.p, 0, sizeof(revo_map_pose_info), s));
  hipLaunchKernelGGL(k_map_pose, dim3((unsigned)((src->cap + 255) / 256)), dim3(256), 0, s, a);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(&r->info, r->buf.p, sizeof(revo_map_pose_info), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  const bool bad = r->info.reserved != 0;
  r->info.reserved = 0;
  if (bad) return fail(REVO_ERR_INVALID_ARG, "voxel map: a source voxel has a count of 2^32 or more (nothing posed)");
  return REVO_OK;
}

extern "C" int revo_map_pose_raw(revo_map* src, const float T[16], float voxel_dst, size_t min_count, revo_map_voxel_raw* out, size_t cap,
                                 size_t* n, int device_out, revo_map_pose_info* info) {
  if (!src || !T || !n) return fail(REVO_ERR_INVALID_ARG, "null argument");
  TRY(map_check_side(device_out, "device_out"));
  if (device_out) TRY(map_check_aligned((uintptr_t)out, 16, "the device output is"));
  TRY(pose_check(T, voxel_dst));
  MapStats ss;
  TRY(map_read_stats(src, &ss));
  hipStream_t s = (hipStream_t)src->g.stream;
  const size_t nv = (size_t)ss.occ;
  MapPoseRun r;
  if (device_out) {
    // nothing may be written when cap is too small or a source voxel is a bad record: count first, then write
    TRY(pose_run(&r, src, s, nv, T, voxel_dst, min_count, nullptr, 0, false));
    *n = (size_t)r.info.voxels_moved;
    if (info) *info = r.info;
    if (!out) return REVO_OK;
    if (cap < *n) return fail(REVO_ERR_CAPACITY, "voxel map: the output holds fewer records than voxels move");
    if (!*n) return REVO_OK;
    return pose_run(&r, src, s, nv, T, voxel_dst, min_count, (ulonglong2*)out, cap, false);
  }
  TRY(pose_run(&r, src, s, nv, T, voxel_dst, min_count, nullptr, 0, true));
  const size_t moved = (size_t)r.info.voxels_moved;
  std::vector<revo_map_voxel_raw> rec(moved);
  if (moved) HIPCHECK(hipMemcpy(rec.data(), r.recs(), sizeof(revo_map_voxel_raw) * moved, hipMemcpyDeviceToHost));
  const size_t m = pose_canonicalise(rec.data(), moved);
  *n = m;
  if (info) *info = r.info;
  if (!out) return REVO_OK;
  if (cap < m) return fail(REVO_ERR_CAPACITY, "voxel map: the output holds fewer records than the posed map has voxels");
  if (m) memcpy(out, rec.data(), sizeof(revo_map_voxel_raw) * m);
  return REVO_OK;
}

// merge_posed and subtract_posed: the argument rules, the wait for src, the posed records of src at dst's edge on dst's
// stream, then map_merge_core or map_subtract_core over them with src's counters plus the drops of the move.
static int posed_apply(revo_map* dst, revo_map* src, const float* T, size_t min_count, revo_map_pose_info* info, bool subtract) {
  if (!dst || !src || !T) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (dst == src) return fail(REVO_ERR_INVALID_ARG, "a map cannot be posed into itself");
  if (dst->g.device != src->g.device) return fail(REVO_ERR_INVALID_ARG, "the maps are on different devices");
  TRY(pose_check(T, dst->voxel));
  MapStats ss;  // waits for src: its table is complete, and its counters say what comes
  TRY(map_read_stats(src, &ss));
  if (ss.kfs > 0x7fffffffull) return fail(REVO_ERR_INVALID_ARG, "the source map's keyframe count does not fit");
  HIPCHECK(hipSetDevice(dst->g.device));
  hipStream_t s = (hipStream_t)dst->g.stream;
  MapPoseRun r;
  TRY(pose_run(&r, src, s, (size_t)ss.occ, T, dst->voxel, min_count, nullptr, 0, true));
  if (info) *info = r.info;
  const size_t moved = (size_t)r.info.voxels_moved;
  if (!moved) return REVO_OK;  // as revo_map_merge_raw / revo_map_subtract_raw with n == 0
  MapMergeK a{};
  a.recs = r.recs();
  a.n = (unsigned)moved;
  a.dropped = ss.drop + r.info.points_dropped;
  if (subtract) return map_subtract_core(dst, a, MERGE_RAW, a.dropped, ss.kfs);  // has waited: the records are read
  // device-made records need no validation: the device decides only when max_voxels is in reach
  const int rc = map_merge_core(dst, a, MERGE_RAW, moved, true, (int)ss.kfs);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) return fail(REVO_ERR_HIP, "hipStreamSynchronize failed");  // the records are read
  return rc;
}
extern "C" int revo_map_merge_posed(revo_map* dst, revo_map* src, const float T[16], size_t min_count, revo_map_pose_info* info) {
  return posed_apply(dst, src, T, min_count, info, false);
}
extern "C" int revo_map_subtract_posed(revo_map* dst, revo_map* src, const float T[16], size_t min_count, revo_map_pose_info* info) {
  return posed_apply(dst, src, T, min_count, info, true);
}

// ---------------------------------------------------------------------------------------------- free-space carving (19) --
// revo_map_carve_eval / revo_map_carve (contract: include/revo_hip.h).
struct MapCarveK {
  const u64* keys; const MapVal* vals; unsigned cap;  // the map's table
  const MapCarveView* views; int n;
  int radius; unsigned min_views;
  u64 min_count, max_count;  // max_count 0: no upper bound
  float margin, margin_rel;
  ulonglong2* out; unsigned cap_out;  // the carved records, at most cap_out of them (0: count only)
  u64* info;                          // one 64-byte line: revo_map_carve_info's four counters
  unsigned* vinfo;                    // 8 words per view: revo_map_carve_view_info
};
// One thread per slot of the table: the value as four 16-byte loads, the point once, then the views one after another with
// the votes in a register.  Per view the classes of a wave are counted by ballots into LDS; the carved records are compacted
// as k_map_export compacts (LDS counter, one global atomic per block); every counter takes one global atomic per block.
__global__ void __launch_bounds__(256) k_map_carve(const MapCarveK a) {
  __shared__ unsigned s_n, s_base, s_cand, s_votes;
  __shared__ u64 s_pts;
  __shared__ unsigned s_cls[CARVE_MAX_VIEWS * CARVE_CLASSES];
  for (int k = threadIdx.x; k < a.n * CARVE_CLASSES; k += 256) s_cls[k] = 0;
  if (threadIdx.x == 0) { s_n = 0; s_cand = 0; s_votes = 0; s_pts = 0; }
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const u64 key = i < a.cap ? a.keys[i] : MAP_EMPTY;
  MapRec r{};
  bool cand = false;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (key != MAP_EMPTY) {
    r = map_rec_from_slot(a.vals + i, key);
    cand = r.n() >= a.min_count && (a.max_count == 0 || r.n() <= a.max_count);  // min_count >= 1: a committed voxel
    if (cand) {
      const double inv = (double)r.n();
      px = map_mean(r.b.x, inv); py = map_mean(r.b.y, inv); pz = map_mean(r.c.x, inv);
    }
  }
  unsigned votes = 0;
  for (int vi = 0; vi < a.n; ++vi) {  // uniform: the ballots see whole waves
    const int cls = cand ? map_carve_class(px, py, pz, a.views[vi], a.radius, a.margin, a.margin_rel) : -1;
    votes += cls == CARVE_FREE ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < CARVE_CLASSES; ++k) {
      const u64 b = __ballot(cls == k);
      if (lane == 0 && b) atomicAdd(&s_cls[vi * CARVE_CLASSES + k], (unsigned)__popcll(b));
    }
  }
  const bool sel = cand && votes >= a.min_views;
  const u64 bc = __ballot(cand);
  if (lane == 0 && bc) atomicAdd(&s_cand, (unsigned)__popcll(bc));
  if (votes) atomicAdd(&s_votes, votes);
  if (sel) atomicAdd(&s_pts, r.n());
  const unsigned o = map_compact_begin(sel, s_n);
  __syncthreads();
  map_compact_end(s_n, s_base, &a.info[1]);  // voxels_carved doubles as the compaction's counter
  if (threadIdx.x == 1 && s_cand) atomicAdd(&a.info[0], (u64)s_cand);
  if (threadIdx.x == 2 && s_pts) atomicAdd(&a.info[2], s_pts);
  if (threadIdx.x == 3 && s_votes) atomicAdd(&a.info[3], (u64)s_votes);
  for (int k = threadIdx.x; k < a.n * CARVE_CLASSES; k += 256)
    if (s_cls[k]) atomicAdd(&a.vinfo[(k / CARVE_CLASSES) * 8 + k % CARVE_CLASSES], s_cls[k]);
  __syncthreads();
  if (!sel) return;
  const unsigned j = s_base + o;
  if (j < a.cap_out) map_rec_store(a.out, j, r);
}

static_assert(sizeof(revo_map_carve_info) == 64 && offsetof(revo_map_carve_info, voxels_considered) == 0 &&
              offsetof(revo_map_carve_info, voxels_carved) == 8 && offsetof(revo_map_carve_info, points_carved) == 16 &&
              offsetof(revo_map_carve_info, votes) == 24 && offsetof(revo_map_carve_info, reserved) == 32,
              "the info record is the kernel's counter line");
static_assert(sizeof(revo_map_carve_view_info) == 32 && offsetof(revo_map_carve_view_info, outside) == 4 * CARVE_OUTSIDE &&
              offsetof(revo_map_carve_view_info, unknown) == 4 * CARVE_UNKNOWN && offsetof(revo_map_carve_view_info, free_space) == 4 * CARVE_FREE &&
              offsetof(revo_map_carve_view_info, confirmed) == 4 * CARVE_CONFIRMED && offsetof(revo_map_carve_view_info, occluded) == 4 * CARVE_OCCLUDED &&
              offsetof(revo_map_carve_view_info, edge) == 4 * CARVE_EDGE && offsetof(revo_map_carve_view_info, reserved) == 24,
              "a view's record is the kernel's eight counter words");
static_assert(sizeof(revo_map_carve_view) == 112 && offsetof(revo_map_carve_view, kf) == 0 && offsetof(revo_map_carve_view, depth) == 8 &&
              offsetof(revo_map_carve_view, width) == 16 && offsetof(revo_map_carve_view, fx) == 24 && offsetof(revo_map_carve_view, T_w_c) == 48 &&
              sizeof(revo_map_carve_params) == 24, "the view and parameter records are the documented layout");

// One carve call's device memory: the counter lines, the view descriptors, the uploaded host images, the records.
struct MapCarveRun {
  DevScratch buf;     // [0, 64) the info line, [256, 256 + 32 n) the views' counters, then the descriptors
  DevScratch images;  // host depth images of the call, uploaded
  DevScratch recs;    // the carved records of a host-output call or of revo_map_carve
};

static int carve_launch(revo_map* m, hipStream_t s, MapCarveRun* r, MapCarveK a, revo_map_carve_info* info, revo_map_carve_view_info* vinfo) {
  char* buf = r->buf.p;
  a.info = (u64*)buf;
  a.vinfo = (unsigned*)(buf + 256);
  HIPCHECK(hipMemsetAsync(buf, 0, 256 + sizeof(revo_map_carve_view_info) * a.n, s));
  hipLaunchKernelGGL(k_map_carve, dim3((unsigned)((m->cap + 255) / 256)), dim3(256), 0, s, a);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(info, buf, sizeof(revo_map_carve_info), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(vinfo, buf + 256, sizeof(revo_map_carve_view_info) * a.n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

static int carve_apply(revo_map* m, int n, const revo_map_carve_view* views, int device_in, const revo_map_carve_params* prm,
                       revo_map_voxel_raw* records, size_t cap, size_t* n_records, int device_out, revo_map_carve_info* info,
                       revo_map_carve_view_info* view_info, bool remove) {
  if (!m || !views || !n_records) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n < 1 || n > CARVE_MAX_VIEWS) return fail(REVO_ERR_INVALID_ARG, "revo_map_carve: n must be 1 .. 64 views");
  TRY(map_check_side(device_in, "device_in"));
  TRY(map_check_side(device_out, "device_out"));
  if (device_out) TRY(map_check_aligned((uintptr_t)records, 16, "the device output is"));
  revo_map_carve_params pp;
  if (const char* why = carve_params_check(prm, m->voxel, &pp)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_carve: ") + why);
  std::vector<MapCarveView> hv(n);
  size_t up_bytes = 0;
  TRY(map_views_prepare(m, n, views, device_in, hv.data(), &up_bytes));
  MapStats st;  // waits for the map: its table is complete
  TRY(map_read_stats(m, &st));
  hipStream_t s = (hipStream_t)m->g.stream;
  MapCarveRun r;
  const size_t o_views = 256 + ((sizeof(revo_map_carve_view_info) * n + 255) & ~(size_t)255);
  TRY(r.buf.alloc(o_views + sizeof(MapCarveView) * n));
  if (up_bytes) {
    TRY(r.images.alloc(up_bytes));
    TRY(map_views_upload(n, views, hv.data(), r.images.p, s));
  }
  HIPCHECK(hipMemcpyAsync(r.buf.p + o_views, hv.data(), sizeof(MapCarveView) * n, hipMemcpyHostToDevice, s));
  MapCarveK a{};
  a.keys = m->d_keys; a.vals = m->d_vals; a.cap = (unsigned)m->cap;
  a.views = (const MapCarveView*)(r.buf.p + o_views); a.n = n;
  a.radius = pp.radius; a.min_views = pp.min_views;
  a.min_count = pp.min_count; a.max_count = pp.max_count;
  a.margin = pp.margin; a.margin_rel = pp.margin_rel;
  revo_map_carve_info ci{};
  std::vector<revo_map_carve_view_info> vi(n);
  // nothing may be written when cap is too small: count first, then write (carve_launch waits, so hv and the images are read)
  TRY(carve_launch(m, s, &r, a, &ci, vi.data()));
  const size_t carved = (size_t)ci.voxels_carved;
  *n_records = carved;
  if (info) *info = ci;
  if (view_info) memcpy(view_info, vi.data(), sizeof(revo_map_carve_view_info) * n);
  if (records && cap < carved) return fail(REVO_ERR_CAPACITY, "voxel map: the output holds fewer records than voxels are carved");
  if (!carved || (!records && !remove)) return REVO_OK;
  ulonglong2* d_rec = (ulonglong2*)records;
  if (!records || !device_out) {
    TRY(r.recs.alloc(sizeof(revo_map_voxel_raw) * carved));
    d_rec = (ulonglong2*)r.recs.p;
  }
  a.out = d_rec; a.cap_out = (unsigned)carved;
  revo_map_carve_info ci2{};
  TRY(carve_launch(m, s, &r, a, &ci2, vi.data()));
  if (ci2.voxels_carved != ci.voxels_carved) return fail(REVO_ERR_HIP, "voxel map: two carve launches over one table disagree");
  if (remove) {
    MapMergeK sub{};
    sub.recs = d_rec;
    sub.n = (unsigned)carved;
    const int rc = map_subtract_core(m, sub, MERGE_RAW, 0, 0);  // has waited: the records are read
    if (rc) return rc;  // nothing removed: the host output stays untouched
  }
  if (records && !device_out) {  // after the removal, so that host records are only ever records that left (or would leave) the map
    HIPCHECK(hipMemcpy(records, d_rec, sizeof(revo_map_voxel_raw) * carved, hipMemcpyDeviceToHost));
    carve_canonicalise(records, carved);
  }
  return REVO_OK;
}

extern "C" int revo_map_carve_eval(revo_map* m, int n, const revo_map_carve_view* views, int device_in, const revo_map_carve_params* prm,
                                   revo_map_voxel_raw* records, size_t cap, size_t* n_records, int device_out, revo_map_carve_info* info,
                                   revo_map_carve_view_info* view_info) {
  return carve_apply(m, n, views, device_in, prm, records, cap, n_records, device_out, info, view_info, false);
}
extern "C" int revo_map_carve(revo_map* m, int n, const revo_map_carve_view* views, int device_in, const revo_map_carve_params* prm,
                              revo_map_voxel_raw* records, size_t cap, size_t* n_records, int device_out, revo_map_carve_info* info,
                              revo_map_carve_view_info* view_info) {
  return carve_apply(m, n, views, device_in, prm, records, cap, n_records, device_out, info, view_info, true);
}
