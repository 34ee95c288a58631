// revo_map_tsdf_track.hip -- tracking a depth frame against the fused surface: revo_map_tsdf_track_eval /
// revo_map_tsdf_track_system / revo_map_tsdf_track.  Contract: include/revo_hip.h.  A pixel's rules are revo_tsdf_track_host.h's, one
// text for both sides; the sums, the finish and the loop above them are revo_map_df_align.hip's.  This unit holds the
// kernel that gives every pixel of the strided lattice its lane, and the entry points.
#include "revo_map_impl.h"
#include "revo_track_dev.h"
#include "revo_align_host.h"
#include "revo_tsdf_track_host.h"

#define TTK_THREADS 256
#define TTK_WAVES (TTK_THREADS / 64)
#define TTK_MAX_GROUPS 1024   // workgroups per pose at most
#define TTK_MAX_TOTAL 16384   // ... and per launch, where the poses leave room for more than one each
#define TTK_NS 32             // double-double slots: 28 sums, four stay zero (reduce32x's tree)
#define TTK_PART (2 * TTK_NS) // doubles of a workgroup's partial: heads, then tails
enum { TW_MATCHED = 28, TW_CONSIDERED = 30, TW_SKIPPED = 32, TW_CENTRE = 34, TW_MAXD = 37, TW_R = 38, TW_T = 47, TW_FLAGS = 50,
       TW_END = 52 };  // words of a revo_map_tsdf_track_info record: revo_map_df_align_info's
static_assert(sizeof(revo_map_tsdf_track_info) == 208 && sizeof(revo_map_tsdf_track_info) == 4 * TW_END && sizeof(revo_map_tsdf_track_info) % 16 == 0 &&
              offsetof(revo_map_tsdf_track_info, S) == 0 && offsetof(revo_map_tsdf_track_info, matched) == 4 * TW_MATCHED &&
              offsetof(revo_map_tsdf_track_info, considered) == 4 * TW_CONSIDERED && offsetof(revo_map_tsdf_track_info, skipped) == 4 * TW_SKIPPED &&
              offsetof(revo_map_tsdf_track_info, centre) == 4 * TW_CENTRE && offsetof(revo_map_tsdf_track_info, max_dist) == 4 * TW_MAXD &&
              offsetof(revo_map_tsdf_track_info, R) == 4 * TW_R && offsetof(revo_map_tsdf_track_info, T) == 4 * TW_T &&
              offsetof(revo_map_tsdf_track_info, flags) == 4 * TW_FLAGS && offsetof(revo_map_tsdf_track_info, reserved) == 4 * (TW_FLAGS + 1),
              "record layout");
static_assert(sizeof(revo_map_tsdf_track_info) == sizeof(revo_map_df_align_info) && offsetof(revo_map_tsdf_track_info, flags) == offsetof(revo_map_df_align_info, flags) &&
              offsetof(revo_map_tsdf_track_info, matched) == offsetof(revo_map_df_align_info, matched), "the record is revo_map_df_align_info's");
static_assert(TW_END <= 64, "a wave writes the record, one word per lane");
static_assert(sizeof(revo_map_tsdf_track_params) == 32 && offsetof(revo_map_tsdf_track_params, max_dist) == 0 && offsetof(revo_map_tsdf_track_params, stride) == 4 &&
              offsetof(revo_map_tsdf_track_params, min_weight) == 8 && offsetof(revo_map_tsdf_track_params, centre) == 12 &&
              offsetof(revo_map_tsdf_track_params, reserved) == 24, "the parameter record is the documented layout");

typedef u64 __attribute__((address_space(1)))* ttk_gu64p;
typedef unsigned __attribute__((address_space(1)))* ttk_gu32p;
#define TTK_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct TsdfTrackPose { float p[12]; };  // R column-major, t

struct TsdfTrackLaunch {  // what every pose of a launch shares
  TsdfTrackK k;
  const float* depth;                    // the frame: h rows of w floats
  int w, h, stride;
  int lw, lh;                            // the strided lattice: tsdf_track_lattice of w and h
  const TsdfTrackPose* poses;
  double* part; unsigned* cnt; unsigned* ticket;
  unsigned* out;                         // revo_map_tsdf_track_info records
};

// Grid (G, poses).  A wave takes an 8 x 8 tile of the strided pixel lattice, a workgroup four tiles side by side (k_tsdf_raycast's
// layout), workgroup g of a pose the blocks g, g + G, ...: neighbouring lanes read neighbouring pixels and, through one pose,
// neighbouring cells.  Per pixel: its depth (one load), tsdf_track_pixel -- the eight cells are read as tsdf_ray_sample names them,
// pairs of z-neighbours side by side --, and the 28 float terms into double-double sums.  The finish is k_map_df_align's: wave
// butterfly, LDS across the waves in index order, the partial published write-through, a ticket per pose; whoever draws the last
// one adds the G partials in a fixed order and one wave writes the record.
__global__ void __launch_bounds__(TTK_THREADS) k_map_tsdf_track(const TsdfTrackLaunch a) {
  constexpr int NS = TTK_NS, PART = TTK_PART;
  __shared__ double s_h[TTK_WAVES][NS], s_l[TTK_WAVES][NS];
  __shared__ unsigned s_c[TTK_WAVES][2];
  const int pose = blockIdx.y, grp = blockIdx.x, G = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned* const rec = a.out + (size_t)pose * TW_END;

  const float* P = a.poses[pose].p;
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
  for (int i = 0; i < 3; ++i) tail = lane == TW_CENTRE + i ? __float_as_uint(a.k.centre[i]) : tail;
  tail = lane == TW_MAXD ? __float_as_uint(a.k.max_dist) : tail;
#pragma unroll
  for (int i = 0; i < 9; ++i) tail = lane == TW_R + i ? Rb[i] : tail;
#pragma unroll
  for (int i = 0; i < 3; ++i) tail = lane == TW_T + i ? Tb[i] : tail;
  tail = lane == TW_FLAGS ? (no_eval ? 1u : 0u) : tail;
  if (no_eval) {  // the same for every workgroup of the pose
    if (grp == 0 && tid < TW_END) rec[tid] = tail;
    return;
  }

  double xd[PART];  // the double-double slots: heads, then tails
#pragma unroll
  for (int k = 0; k < PART; ++k) xd[k] = 0.0;
  unsigned matched = 0, skipped = 0;
  const int bw = (a.lw + 31) / 32, bh = (a.lh + 7) / 8;
  const int nblocks = bw * bh;
  const gf32p depth = (gf32p)a.depth;
#pragma unroll 1
  for (int bt = grp; bt < nblocks; bt += G) {
    const int X = (bt % bw) * 32 + wave * 8 + (lane & 7), Y = (bt / bw) * 8 + (lane >> 3);
    if (X >= a.lw || Y >= a.lh) continue;
    const int x = X * a.stride, y = Y * a.stride;  // x < w and y < h: the lattice ends before the image does
    const float D = depth[(size_t)y * a.w + x];
    float pw[3], e = 0.0f, g[3] = {0.0f, 0.0f, 0.0f};
    const int cls = tsdf_track_pixel(a.k, R, T, x, y, D, pw, &e, g);
    if (cls == TSDF_TRACK_SKIPPED) { ++skipped; continue; }
    if (cls == TSDF_TRACK_GATED) continue;
    ++matched;
    tsdf_track_terms(tsdf_track_row(a.k, pw, g), e, [&](int slot, float term) { dd_acc(xd[slot], xd[NS + slot], (double)term); });
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
  for (int wv = 1; wv < TTK_WAVES; ++wv) { dd_add(h, l, s_h[wv][k], s_l[wv][k]); cn += lane < 2 ? s_c[wv][lane] : 0u; }
  ttk_gu64p mine = (ttk_gu64p)(a.part + ((size_t)pose * G + grp) * PART);
  if (lane < NS) {
    __hip_atomic_store(mine + k, (u64)__double_as_longlong(h), TTK_RLX_AGENT);
    __hip_atomic_store(mine + NS + k, (u64)__double_as_longlong(l), TTK_RLX_AGENT);
  }
  ttk_gu32p cnts = (ttk_gu32p)(a.cnt + ((size_t)pose * G) * 2);
  if (lane < 2) __hip_atomic_store(cnts + 2 * grp + lane, cn, TTK_RLX_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial has left this CU before the ticket is drawn
  unsigned drawn = 0u;
  if (lane == 0) drawn = __hip_atomic_fetch_add((ttk_gu32p)(a.ticket + pose), 1u, TTK_RLX_AGENT);
  drawn = (unsigned)__builtin_amdgcn_readfirstlane((int)drawn);
  if (drawn != (unsigned)(G - 1)) return;

  // the last workgroup of the pose to arrive: every partial is published.  Lane L adds slot L & 31 of the groups L / 32,
  // L / 32 + 2, ... in index order; the two group sums meet across the half-waves.
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  ttk_gu64p all = (ttk_gu64p)(a.part + (size_t)pose * G * PART);
  h = 0.0; l = 0.0;
  u64 n_matched = 0, n_skipped = 0;
  for (int g = lane / NS; g < G; g += 64 / NS) {
    const double gh = __longlong_as_double((long long)__hip_atomic_load(all + (size_t)g * PART + k, TTK_RLX_AGENT));
    const double gl = __longlong_as_double((long long)__hip_atomic_load(all + (size_t)g * PART + NS + k, TTK_RLX_AGENT));
    dd_add(h, l, gh, gl);
  }
  dd_add(h, l, lane_xor_d<32>(h), lane_xor_d<32>(l));
  for (int g = 0; g < G; ++g) {
    n_matched += __hip_atomic_load(cnts + 2 * g, TTK_RLX_AGENT);
    n_skipped += __hip_atomic_load(cnts + 2 * g + 1, TTK_RLX_AGENT);
  }
  const u64 n_considered = (u64)a.lw * (u64)a.lh;
  const float f = dd_to_float(h, l);
  unsigned wd = tail;
  wd = lane < 28 ? __float_as_uint(f) : wd;
  wd = lane == TW_MATCHED ? (unsigned)n_matched : (lane == TW_MATCHED + 1 ? (unsigned)(n_matched >> 32) : wd);
  wd = lane == TW_CONSIDERED ? (unsigned)n_considered : (lane == TW_CONSIDERED + 1 ? (unsigned)(n_considered >> 32) : wd);
  wd = lane == TW_SKIPPED ? (unsigned)n_skipped : (lane == TW_SKIPPED + 1 ? (unsigned)(n_skipped >> 32) : wd);
  if (lane < TW_END) rec[lane] = wd;
}

// -------------------------------------------------------------------------------------------------------- entry points --
// Everything revo_map_tsdf_track_eval and revo_map_tsdf_track share but the poses and the output: the checks, in the order the
// contract lists them, with nothing enqueued.  *fv: the frame with an identity in the place of its pose, which is not read.
static int ttk_check(const char* name, revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf, int device_tsdf, float trunc,
                     const revo_map_carve_view* frame, int device_in, const revo_map_tsdf_track_params* prm, size_t* cells,
                     revo_map_tsdf_track_params* pp, revo_map_carve_view* fv) {
  if (!m || !box || !tsdf || !frame) return fail(REVO_ERR_INVALID_ARG, "null argument");
  const std::string who = std::string(name) + ": ";
  if (const char* why = map_df_box_check(box, cells)) return fail(REVO_ERR_INVALID_ARG, who + why);
  TRY(map_check_side(device_tsdf, "device_tsdf"));
  TRY(map_check_side(device_in, "device_in"));
  if (device_tsdf) TRY(map_check_aligned((uintptr_t)tsdf, 16, "the device volume is"));
  if (!std::isfinite(trunc) || !(trunc > 0.0f)) return fail(REVO_ERR_INVALID_ARG, who + "trunc must be finite and > 0");
  if (const char* why = tsdf_track_params_check(prm, trunc, pp)) return fail(REVO_ERR_INVALID_ARG, who + why);
  *fv = *frame;
  for (int i = 0; i < 16; ++i) fv->T_w_c[i] = i % 5 == 0 ? 1.0f : 0.0f;
  return REVO_OK;
}

// The volume and the frame of one call on the device (a host side goes into the handle's buffers once), and the launch's
// constants.  The frame's rules are checked here, before anything is enqueued.
static int ttk_begin(TsdfTrackLaunch* c, revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf, int device_tsdf, size_t cells,
                     float trunc, const revo_map_carve_view* fv, int device_in, const revo_map_tsdf_track_params& pp) {
  MapCarveView hv{};
  size_t up_bytes = 0;
  TRY(map_views_prepare(m, 1, fv, device_in, &hv, &up_bytes));  // a pyramid frame: the tracker stream is behind its build
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t vol_bytes = sizeof(revo_map_tsdf_cell) * cells;
  TRY(m->tsdfvol.reserve(device_tsdf ? 0 : vol_bytes, s));
  TRY(m->tsdftrk.frame.reserve(up_bytes, s));
  if (!device_tsdf) HIPCHECK(hipMemcpyAsync(m->tsdfvol.p, tsdf, vol_bytes, hipMemcpyHostToDevice, s));
  if (up_bytes) TRY(map_views_upload(1, fv, &hv, m->tsdftrk.frame.p, s));
  TsdfTrackK& k = c->k;
  k.vol = TsdfRayK{};
  k.vol.tsdf = device_tsdf ? tsdf : (const revo_map_tsdf_cell*)m->tsdfvol.p;
  k.vol.box = *box;
  k.vol.voxel = m->voxel; k.vol.step = m->voxel;
  k.vol.min_weight = pp.min_weight; k.vol.max_steps = 1u;
  k.cam = TsdfTrackCam{hv.v.fx, hv.v.fy, hv.v.cx, hv.v.cy, hv.v.zmin, hv.v.zmax};
  k.kq = tsdf_track_kq(trunc);
  k.max_dist = pp.max_dist;
  for (int i = 0; i < 3; ++i) k.centre[i] = pp.centre[i];
  c->depth = hv.depth;
  c->w = hv.v.w; c->h = hv.v.h; c->stride = (int)pp.stride;
  c->lw = tsdf_track_lattice(c->w, c->stride); c->lh = tsdf_track_lattice(c->h, c->stride);
  return REVO_OK;
}

// n poses (4x4 column-major) in one launch, records to d_out (device memory).  Enqueues only: the poses go through the handle's
// pinned rows (their event is waited for before they are rewritten), the scratch is the handle's and is used in stream order.
// REVO_MAP_TSDF_TRACK_GROUPS=n forces the workgroups per pose (the tests: the record does not depend on it).
static int ttk_launch(const TsdfTrackLaunch* c, revo_map* m, int n, const float* T16, void* d_out) {
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t blocks = (size_t)((c->lw + 31) / 32) * (size_t)((c->lh + 7) / 8);
  size_t G = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(blocks, TTK_MAX_GROUPS), TTK_MAX_TOTAL / (size_t)n));
  const int forced = env_int("REVO_MAP_TSDF_TRACK_GROUPS", 0, 0, TTK_MAX_GROUPS);
  if (forced > 0) G = std::max<size_t>(1, std::min<size_t>((size_t)forced, TTK_MAX_TOTAL / (size_t)n));
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_tick = 0, o_cnt = o_tick + up(sizeof(unsigned) * n), o_part = o_cnt + up(sizeof(unsigned) * 2 * G * n),
               total = o_part + up(sizeof(double) * TTK_PART * G * n);
  TRY(m->tsdftrk.work.reserve(total, s));
  TRY(m->tsdftrk.poses.reserve(n, s));
  for (int i = 0; i < n; ++i) {
    const float* T = T16 + 16 * (size_t)i;
    float* P = m->tsdftrk.poses.h[i].p;
    for (int col = 0; col < 3; ++col)
      for (int r = 0; r < 3; ++r) P[3 * col + r] = T[4 * col + r];
    for (int r = 0; r < 3; ++r) P[9 + r] = T[12 + r];
  }
  TRY(m->tsdftrk.poses.upload(n, s));
  TsdfTrackLaunch k = *c;
  k.poses = m->tsdftrk.poses.d;
  k.ticket = (unsigned*)(m->tsdftrk.work.p + o_tick);
  k.cnt = (unsigned*)(m->tsdftrk.work.p + o_cnt);
  k.part = (double*)(m->tsdftrk.work.p + o_part);
  k.out = (unsigned*)d_out;
  HIPCHECK(hipMemsetAsync(k.ticket, 0, up(sizeof(unsigned) * n), s));
  hipLaunchKernelGGL(k_map_tsdf_track, dim3((unsigned)G, (unsigned)n), dim3(TTK_THREADS), 0, s, k);
  if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(s); return fail(REVO_ERR_HIP, "k_map_tsdf_track: the launch failed"); }
  return REVO_OK;
}

extern "C" int revo_map_tsdf_track_eval(revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf, int device_tsdf, float trunc,
                                        const revo_map_carve_view* frame, int device_in, int nposes, const float* T,
                                        const revo_map_tsdf_track_params* prm, revo_map_tsdf_track_info* out, int device_out) {
  size_t cells = 0;
  revo_map_tsdf_track_params pp;
  revo_map_carve_view fv;
  if (!T || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  TRY(ttk_check("revo_map_tsdf_track_eval", m, box, tsdf, device_tsdf, trunc, frame, device_in, prm, &cells, &pp, &fv));
  if (nposes < 1 || nposes > TSDF_TRACK_MAX_POSES) return fail(REVO_ERR_INVALID_ARG, "revo_map_tsdf_track_eval: nposes must be 1 .. 4096");
  TRY(map_check_side(device_out, "device_out"));
  if (device_out) TRY(map_check_aligned((uintptr_t)out, 16, "the device output is"));
  hipStream_t s = (hipStream_t)m->g.stream;
  const bool waits = !device_tsdf || (frame->depth && !device_in) || !device_out;
  TsdfTrackLaunch c{};
  int rc = ttk_begin(&c, m, box, tsdf, device_tsdf, cells, trunc, &fv, device_in, pp);
  void* d_out = out;
  if (!rc && !device_out) {
    rc = m->tsdftrk.out.reserve(sizeof(revo_map_tsdf_track_info) * nposes, s);
    d_out = m->tsdftrk.out.p;
  }
  if (!rc) rc = ttk_launch(&c, m, nposes, T, d_out);
  if (!rc && !device_out) {
    const hipError_t e = hipMemcpyAsync(out, d_out, sizeof(revo_map_tsdf_track_info) * nposes, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) rc = fail(REVO_ERR_HIP, std::string("revo_map_tsdf_track_eval: ") + hipGetErrorString(e));
  }
  if (rc) { (void)hipStreamSynchronize(s); return rc; }  // the uploads may still read the caller's memory
  if (waits) HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_tsdf_track_system(const revo_map_tsdf_track_info* info, double H[36], double g[6]) {
  if (!info || !H || !g) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (info->flags & 1) return fail(REVO_ERR_INVALID_ARG, "the record carries no evaluation (flags bit0)");
  align_df_system_fill(reinterpret_cast<const revo_map_df_align_info*>(info), H, g);  // the same 208 bytes (static_assert above)
  return REVO_OK;
}

extern "C" int revo_map_tsdf_track(revo_map* m, const revo_map_df_box* box, const revo_map_tsdf_cell* tsdf, int device_tsdf, float trunc,
                                   const revo_map_carve_view* frame, int device_in, const float T_init[16],
                                   const revo_map_tsdf_track_params* prm, const revo_map_align_opts* opt, float T_out[16],
                                   revo_map_tsdf_track_info* info_out, int32_t* iterations, int32_t* status) {
  size_t cells = 0;
  revo_map_tsdf_track_params pp;
  revo_map_carve_view fv;
  if (!T_init || !T_out || !status) return fail(REVO_ERR_INVALID_ARG, "null argument");
  TRY(ttk_check("revo_map_tsdf_track", m, box, tsdf, device_tsdf, trunc, frame, device_in, prm, &cells, &pp, &fv));
  if (!pose_is_finite(T_init)) return fail(REVO_ERR_INVALID_ARG, "T_init is not finite");
  revo_map_align_opts o{30, 0, 1e-6, 1e-6, 12};
  if (opt) o = *opt;
  if (o.max_iters < 1) return fail(REVO_ERR_INVALID_ARG, "max_iters must be >= 1");
  hipStream_t s = (hipStream_t)m->g.stream;
  TsdfTrackLaunch c{};
  int rc = ttk_begin(&c, m, box, tsdf, device_tsdf, cells, trunc, &fv, device_in, pp);
  if (!rc) rc = m->tsdftrk.out.reserve(sizeof(revo_map_tsdf_track_info), s);
  int32_t it = 0;
  if (!rc)
    rc = align_loop_over<revo_map_tsdf_track_info>(
        T_init, pp.centre, o,
        [](const revo_map_tsdf_track_info* r, double* H, double* g) { align_df_system_fill(reinterpret_cast<const revo_map_df_align_info*>(r), H, g); },
        [&](const float* Tf, revo_map_tsdf_track_info* rec) {
          TRY(ttk_launch(&c, m, 1, Tf, m->tsdftrk.out.p));
          HIPCHECK(hipMemcpyAsync(rec, m->tsdftrk.out.p, sizeof(*rec), hipMemcpyDeviceToHost, s));
          HIPCHECK(hipStreamSynchronize(s));
          return (int)REVO_OK;
        },
        T_out, info_out, &it, status);
  (void)hipStreamSynchronize(s);
  if (rc) return rc;
  if (iterations) *iterations = it;
  return REVO_OK;
}
