// revo_map_df_align.hip -- registering point sets against the map's distance field: revo_map_df_align_eval /
// revo_map_df_align_system / revo_map_df_align.  Contract: include/revo_hip.h; DESIGN 22.  The residual of a point under a
// pose is the trilinear interpolant of sqrt(d2) at the moved point, so there is no neighbour search and the source is any
// packed float[3] array; the sums, the launch shape and the finish are k_map_align_plane's (revo_map_align.hip).
#include "revo_map_impl.h"
#include "revo_track_dev.h"
#include "revo_align_host.h"

#define DFA_THREADS 256
#define DFA_WAVES (DFA_THREADS / 64)
#define DFA_CHUNK 512         // points per chunk: workgroup g of a pose takes the chunks g, g + G, ...
#define DFA_MAX_GROUPS 1024   // workgroups per pose at most
#define DFA_MAX_TOTAL 16384   // ... and per launch, where the poses leave room for more than one each
#define DFA_NS 32             // double-double slots: 28 sums, four stay zero (reduce32x's tree)
#define DFA_PART (2 * DFA_NS) // doubles of a workgroup's partial: heads, then tails
#define DFA_MAX_POINTS (1ull << 24)
#define DFA_MAX_POSES 65535
enum { DW_MATCHED = 28, DW_CONSIDERED = 30, DW_SKIPPED = 32, DW_CENTRE = 34, DW_MAXD = 37, DW_R = 38, DW_T = 47, DW_FLAGS = 50,
       DW_END = 52 };  // words of a revo_map_df_align_info record: revo_map_plane_info's
static_assert(sizeof(revo_map_df_align_info) == 208 && sizeof(revo_map_df_align_info) == 4 * DW_END && sizeof(revo_map_df_align_info) % 16 == 0 &&
              offsetof(revo_map_df_align_info, S) == 0 && offsetof(revo_map_df_align_info, matched) == 4 * DW_MATCHED &&
              offsetof(revo_map_df_align_info, considered) == 4 * DW_CONSIDERED && offsetof(revo_map_df_align_info, skipped) == 4 * DW_SKIPPED &&
              offsetof(revo_map_df_align_info, centre) == 4 * DW_CENTRE && offsetof(revo_map_df_align_info, max_dist) == 4 * DW_MAXD &&
              offsetof(revo_map_df_align_info, R) == 4 * DW_R && offsetof(revo_map_df_align_info, T) == 4 * DW_T &&
              offsetof(revo_map_df_align_info, flags) == 4 * DW_FLAGS && offsetof(revo_map_df_align_info, reserved) == 4 * (DW_FLAGS + 1),
              "record layout");
static_assert(DW_END <= 64, "a wave writes the record, one word per lane");

typedef u64 __attribute__((address_space(1)))* dfa_gu64p;
typedef unsigned __attribute__((address_space(1)))* dfa_gu32p;
typedef const unsigned __attribute__((address_space(1)))* dfa_field_p;
// the two z-neighbours of a cell are adjacent words: one dwordx2 gather (global loads only need dword alignment)
typedef unsigned dfa_u2 __attribute__((ext_vector_type(2), aligned(4)));
typedef const dfa_u2 __attribute__((address_space(1)))* dfa_pair_p;
#define DFA_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct MapDfPose { float p[12]; };  // R column-major, t

struct DfAlignK {  // what every pose of a launch shares
  const float* xyz; unsigned npts;       // packed float[3] points, source frame
  const unsigned* d2;                    // the field, [n0][n1][n2]
  unsigned ny, nz;                       // cells along y and z: the strides
  float lo[3], top[3];                   // per axis (float)lo and (float)(n - 2): the interpolation cells are 0 .. n - 2
  float voxel, maxd, centre[3];
  const MapDfPose* poses;
  double* part; unsigned* cnt; unsigned* ticket;
  unsigned* out;                         // revo_map_df_align_info records
};

__device__ __forceinline__ float dfa_lerp(float x0, float x1, float w) { return x0 + w * (x1 - x0); }

// Grid (G, poses), k_map_align's shape: workgroup g of a pose takes the chunks g, g + G, ... of the points, one point per
// thread and round.  Per point: p', its interpolation cell, four dwordx2 gathers (the 8 corners), the interpolant and its
// derivative, the gate, and the 28 float terms into double-double sums.  The finish is k_map_align's, for 32 slots: wave
// butterfly, LDS across the waves, the partial published write-through, a ticket per pose; whoever draws the last one adds
// the G partials in a fixed order and writes the record.
__global__ void __launch_bounds__(DFA_THREADS) k_map_df_align(const DfAlignK a) {
  constexpr int NS = DFA_NS, PART = DFA_PART;
  __shared__ double s_h[DFA_WAVES][NS], s_l[DFA_WAVES][NS];
  __shared__ unsigned s_c[DFA_WAVES][2];
  const int pose = blockIdx.y, grp = blockIdx.x, G = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned* const rec = a.out + (size_t)pose * DW_END;

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
  for (int i = 0; i < 3; ++i) tail = lane == DW_CENTRE + i ? __float_as_uint(a.centre[i]) : tail;
  tail = lane == DW_MAXD ? __float_as_uint(a.maxd) : tail;
#pragma unroll
  for (int i = 0; i < 9; ++i) tail = lane == DW_R + i ? Rb[i] : tail;
#pragma unroll
  for (int i = 0; i < 3; ++i) tail = lane == DW_T + i ? Tb[i] : tail;
  tail = lane == DW_FLAGS ? (no_eval ? 1u : 0u) : tail;
  if (no_eval) {  // the same for every workgroup of the pose
    if (grp == 0 && tid < DW_END) rec[tid] = tail;
    return;
  }

  const unsigned N = a.npts;
  const dfa_field_p field = (dfa_field_p)a.d2;
  const gf32p xyz = (gf32p)a.xyz;
  const unsigned sy = a.nz, sx = a.ny * a.nz;
  double xd[PART];  // the double-double slots: heads, then tails
#pragma unroll
  for (int k = 0; k < PART; ++k) xd[k] = 0.0;
  unsigned matched = 0, skipped = 0;
  const unsigned nchunks = (N + DFA_CHUNK - 1) / DFA_CHUNK;
  for (unsigned ch = grp; ch < nchunks; ch += G) {
    const unsigned end = (ch + 1) * DFA_CHUNK < N ? (ch + 1) * DFA_CHUNK : N;
#pragma unroll 1
    for (unsigned i = ch * DFA_CHUNK + tid; i < end; i += DFA_THREADS) {
      const float px = xyz[3 * (size_t)i], py = xyz[3 * (size_t)i + 1], pz = xyz[3 * (size_t)i + 2];
      float pt[3], w[3];
      unsigned c[3];
      bool ok = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        pt[k] = ((R[k] * px + R[3 + k] * py) + R[6 + k] * pz) + T[k];
        const float g = __fdiv_rn(pt[k], a.voxel) - 0.5f;
        const float f = floorf(g);
        w[k] = g - f;
        const float af = f - a.lo[k];
        ok = ok && __builtin_isfinite(pt[k]) && __builtin_isfinite(g) && af >= 0.0f && af <= a.top[k];  // NaN fails every comparison
        c[k] = ok ? (unsigned)af : 0u;
      }
      if (!ok) { ++skipped; continue; }  // before any load: only a cell with all 8 corners inside the box is read
      const unsigned at = (c[0] * a.ny + c[1]) * a.nz + c[2];
      const dfa_u2 q00 = *(dfa_pair_p)(field + at), q01 = *(dfa_pair_p)(field + at + sy);
      const dfa_u2 q10 = *(dfa_pair_p)(field + at + sx), q11 = *(dfa_pair_p)(field + at + sx + sy);
      const unsigned worst = max(max(max(q00.x, q00.y), max(q01.x, q01.y)), max(max(q10.x, q10.y), max(q11.x, q11.y)));
      if (worst == REVO_DF_NONE) { ++skipped; continue; }
      const float s000 = sqrtf((float)q00.x), s001 = sqrtf((float)q00.y), s010 = sqrtf((float)q01.x), s011 = sqrtf((float)q01.y);
      const float s100 = sqrtf((float)q10.x), s101 = sqrtf((float)q10.y), s110 = sqrtf((float)q11.x), s111 = sqrtf((float)q11.y);
      // along z, then y, then x; a lerp's difference is also the derivative along its axis
      const float dz00 = s001 - s000, dz01 = s011 - s010, dz10 = s101 - s100, dz11 = s111 - s110;
      const float m00 = s000 + w[2] * dz00, m01 = s010 + w[2] * dz01, m10 = s100 + w[2] * dz10, m11 = s110 + w[2] * dz11;
      const float h0 = m01 - m00, h1 = m11 - m10;
      const float l0 = m00 + w[1] * h0, l1 = m10 + w[1] * h1;
      const float k0 = dfa_lerp(dz00, dz01, w[1]), k1 = dfa_lerp(dz10, dz11, w[1]);
      const float gx = l1 - l0;
      const float cc = l0 + w[0] * gx;
      const float gy = dfa_lerp(h0, h1, w[0]), gz = dfa_lerp(k0, k1, w[0]);
      const float e = cc * a.voxel;
      if (!(e <= a.maxd)) continue;  // gated
      ++matched;
      const float ux = pt[0] - a.centre[0], uy = pt[1] - a.centre[1], uz = pt[2] - a.centre[2];
      const float J[6] = {gx, gy, gz, uy * gz - uz * gy, uz * gx - ux * gz, ux * gy - uy * gx};
#define DFA_ACC(slot, term) dd_acc(xd[slot], xd[NS + (slot)], (double)(term))
      int k = 0;
#pragma unroll
      for (int i2 = 0; i2 < 6; ++i2)
#pragma unroll
        for (int j = i2; j < 6; ++j) { DFA_ACC(k, J[i2] * J[j]); ++k; }
#pragma unroll
      for (int i2 = 0; i2 < 6; ++i2) DFA_ACC(21 + i2, J[i2] * e);
      DFA_ACC(27, e * e);
#undef DFA_ACC
    }
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
  for (int wv = 1; wv < DFA_WAVES; ++wv) { dd_add(h, l, s_h[wv][k], s_l[wv][k]); cn += lane < 2 ? s_c[wv][lane] : 0u; }
  dfa_gu64p mine = (dfa_gu64p)(a.part + ((size_t)pose * G + grp) * PART);
  if (lane < NS) {
    __hip_atomic_store(mine + k, (u64)__double_as_longlong(h), DFA_RLX_AGENT);
    __hip_atomic_store(mine + NS + k, (u64)__double_as_longlong(l), DFA_RLX_AGENT);
  }
  dfa_gu32p cnts = (dfa_gu32p)(a.cnt + ((size_t)pose * G) * 2);
  if (lane < 2) __hip_atomic_store(cnts + 2 * grp + lane, cn, DFA_RLX_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial has left this CU before the ticket is drawn
  unsigned drawn = 0u;
  if (lane == 0) drawn = __hip_atomic_fetch_add((dfa_gu32p)(a.ticket + pose), 1u, DFA_RLX_AGENT);
  drawn = (unsigned)__builtin_amdgcn_readfirstlane((int)drawn);
  if (drawn != (unsigned)(G - 1)) return;

  // the last workgroup of the pose to arrive: every partial is published.  Lane L adds slot L & 31 of the groups L / 32,
  // L / 32 + 2, ... in index order; the two group sums meet across the half-waves.
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  dfa_gu64p all = (dfa_gu64p)(a.part + (size_t)pose * G * PART);
  h = 0.0; l = 0.0;
  u64 n_matched = 0, n_skipped = 0;
  for (int g = lane / NS; g < G; g += 64 / NS) {
    const double gh = __longlong_as_double((long long)__hip_atomic_load(all + (size_t)g * PART + k, DFA_RLX_AGENT));
    const double gl = __longlong_as_double((long long)__hip_atomic_load(all + (size_t)g * PART + NS + k, DFA_RLX_AGENT));
    dd_add(h, l, gh, gl);
  }
  dd_add(h, l, lane_xor_d<32>(h), lane_xor_d<32>(l));
  for (int g = 0; g < G; ++g) {
    n_matched += __hip_atomic_load(cnts + 2 * g, DFA_RLX_AGENT);
    n_skipped += __hip_atomic_load(cnts + 2 * g + 1, DFA_RLX_AGENT);
  }
  const float f = dd_to_float(h, l);
  unsigned wd = tail;
  wd = lane < 28 ? __float_as_uint(f) : wd;
  wd = lane == DW_MATCHED ? (unsigned)n_matched : (lane == DW_MATCHED + 1 ? (unsigned)(n_matched >> 32) : wd);
  wd = lane == DW_CONSIDERED ? N : wd;
  wd = lane == DW_SKIPPED ? (unsigned)n_skipped : (lane == DW_SKIPPED + 1 ? (unsigned)(n_skipped >> 32) : wd);
  if (lane < DW_END) rec[lane] = wd;
}

// -------------------------------------------------------------------------------------------------------- entry points --
// the box rules of DESIGN 21 (revo_map_field.hip states them for the field's own calls); nullptr if the box keeps them
static const char* dfa_box_check(const revo_map_df_box* box, size_t* cells) {
  size_t n = 1;
  for (int k = 0; k < 3; ++k) {
    if (box->n[k] < 1 || box->n[k] > 1024) return "a box size must be 1 .. 1024 cells";
    if (box->lo[k] < -(1 << 20) || (long long)box->lo[k] + box->n[k] - 1 > (1 << 20) - 1) return "the box leaves the voxel index range [-2^20, 2^20 - 1]";
    n *= (size_t)box->n[k];
  }
  if (n > (1ull << 27)) return "the box holds more than 2^27 cells";
  *cells = n;
  return nullptr;
}

// everything revo_map_df_align_eval and revo_map_df_align share but the poses and the output
static int dfa_check(const char* name, revo_map* m, const revo_map_df_box* box, const uint32_t* d2, int device_field, size_t npts,
                     const float* xyz, int device_in, const revo_map_align_params* prm, size_t* cells) {
  if (!m || !box || !d2 || !xyz || !prm) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (npts < 1 || npts > DFA_MAX_POINTS) return fail(REVO_ERR_INVALID_ARG, std::string(name) + ": npts must be 1 .. 2^24 points");
  if (const char* why = dfa_box_check(box, cells)) return fail(REVO_ERR_INVALID_ARG, std::string(name) + ": " + why);
  TRY(map_check_side(device_field, "device_field"));
  TRY(map_check_side(device_in, "device_in"));
  if (device_field) TRY(map_check_aligned((uintptr_t)d2, 16, "the device field is"));
  if (device_in) TRY(map_check_aligned((uintptr_t)xyz, 16, "the device points are"));
  if (!std::isfinite(prm->max_dist) || !(prm->max_dist > 0.0f)) return fail(REVO_ERR_INVALID_ARG, "max_dist must be finite and > 0");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(prm->centre[i])) return fail(REVO_ERR_INVALID_ARG, "the centre is not finite");
  if (prm->min_count_dst != 0 || prm->min_count_src != 0)
    return fail(REVO_ERR_INVALID_ARG, std::string(name) + ": min_count_dst and min_count_src must be 0 (the field and the points carry no counts)");
  return REVO_OK;
}

// The field and the points of one call on the device (a host side is uploaded once, into memory freed when the call
// returns: such a call waits), and the launch's constants.
struct DfAlignCall {
  DevScratch field, pts, out;
  DfAlignK k{};
  size_t npts = 0;
};

static int dfa_begin(DfAlignCall* c, revo_map* m, const revo_map_df_box* box, const uint32_t* d2, int device_field, size_t cells,
                     size_t npts, const float* xyz, int device_in, const revo_map_align_params* prm) {
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  DfAlignK& k = c->k;
  k.d2 = d2; k.xyz = xyz;
  if (!device_field) {
    TRY(c->field.alloc(sizeof(unsigned) * cells));
    HIPCHECK(hipMemcpyAsync(c->field.p, d2, sizeof(unsigned) * cells, hipMemcpyHostToDevice, s));
    k.d2 = (const unsigned*)c->field.p;
  }
  if (!device_in) {
    TRY(c->pts.alloc(sizeof(float) * 3 * npts));
    HIPCHECK(hipMemcpyAsync(c->pts.p, xyz, sizeof(float) * 3 * npts, hipMemcpyHostToDevice, s));
    k.xyz = (const float*)c->pts.p;
  }
  c->npts = npts;
  k.npts = (unsigned)npts;
  k.ny = (unsigned)box->n[1]; k.nz = (unsigned)box->n[2];
  for (int i = 0; i < 3; ++i) { k.lo[i] = (float)box->lo[i]; k.top[i] = (float)(box->n[i] - 2); k.centre[i] = prm->centre[i]; }
  k.voxel = m->voxel; k.maxd = prm->max_dist;
  return REVO_OK;
}

// n poses (4x4 column-major) in one launch, records to d_out (device memory).  Enqueues only: the poses go through the
// handle's pinned rows (their event is waited for before they are rewritten), the scratch is the handle's and is used in
// stream order.
static int dfa_launch(DfAlignCall* c, revo_map* m, int n, const float* T16, void* d_out) {
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t chunks = (c->npts + DFA_CHUNK - 1) / DFA_CHUNK;
  const size_t G = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(chunks, DFA_MAX_GROUPS), DFA_MAX_TOTAL / (size_t)n));
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t o_tick = 0, o_cnt = o_tick + up(sizeof(unsigned) * n), o_part = o_cnt + up(sizeof(unsigned) * 2 * G * n),
               total = o_part + up(sizeof(double) * DFA_PART * G * n);
  TRY(m->dfa_work.reserve(total, s));
  TRY(m->dfa_poses.reserve(n, s));
  for (int i = 0; i < n; ++i) {
    const float* T = T16 + 16 * (size_t)i;
    float* P = m->dfa_poses.h[i].p;
    for (int col = 0; col < 3; ++col)
      for (int r = 0; r < 3; ++r) P[3 * col + r] = T[4 * col + r];
    for (int r = 0; r < 3; ++r) P[9 + r] = T[12 + r];
  }
  TRY(m->dfa_poses.upload(n, s));
  DfAlignK k = c->k;
  k.poses = m->dfa_poses.d;
  k.ticket = (unsigned*)(m->dfa_work.p + o_tick);
  k.cnt = (unsigned*)(m->dfa_work.p + o_cnt);
  k.part = (double*)(m->dfa_work.p + o_part);
  k.out = (unsigned*)d_out;
  HIPCHECK(hipMemsetAsync(k.ticket, 0, up(sizeof(unsigned) * n), s));
  hipLaunchKernelGGL(k_map_df_align, dim3((unsigned)G, (unsigned)n), dim3(DFA_THREADS), 0, s, k);
  if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(s); return fail(REVO_ERR_HIP, "k_map_df_align: the launch failed"); }
  return REVO_OK;
}

extern "C" int revo_map_df_align_eval(revo_map* m, const revo_map_df_box* box, const uint32_t* d2, int device_field, size_t npts,
                                      const float* xyz, int device_in, int nposes, const float* T, const revo_map_align_params* prm,
                                      revo_map_df_align_info* out, int device_out) {
  size_t cells = 0;
  if (!T || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  TRY(dfa_check("revo_map_df_align_eval", m, box, d2, device_field, npts, xyz, device_in, prm, &cells));
  if (nposes < 1 || nposes > DFA_MAX_POSES) return fail(REVO_ERR_INVALID_ARG, "revo_map_df_align_eval: nposes must be 1 .. 65535");
  TRY(map_check_side(device_out, "device_out"));
  if (device_out) TRY(map_check_aligned((uintptr_t)out, 16, "the device output is"));
  hipStream_t s = (hipStream_t)m->g.stream;
  DfAlignCall c;  // freed after the wait below
  const bool waits = !device_field || !device_in || !device_out;
  int rc = dfa_begin(&c, m, box, d2, device_field, cells, npts, xyz, device_in, prm);
  void* d_out = out;
  if (!rc && !device_out) { rc = c.out.alloc(sizeof(revo_map_df_align_info) * nposes); d_out = c.out.p; }
  if (!rc) rc = dfa_launch(&c, m, nposes, T, d_out);
  if (!rc && !device_out) {
    const hipError_t e = hipMemcpyAsync(out, d_out, sizeof(revo_map_df_align_info) * nposes, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) rc = fail(REVO_ERR_HIP, std::string("revo_map_df_align_eval: ") + hipGetErrorString(e));
  }
  if (rc) { (void)hipStreamSynchronize(s); return rc; }  // the uploads may still read the temporary buffers
  if (waits) HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_df_align_system(const revo_map_df_align_info* info, double H[36], double g[6]) {
  if (!info || !H || !g) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (info->flags & 1) return fail(REVO_ERR_INVALID_ARG, "the record carries no evaluation (flags bit0)");
  align_df_system_fill(info, H, g);
  return REVO_OK;
}

extern "C" int revo_map_df_align(revo_map* m, const revo_map_df_box* box, const uint32_t* d2, int device_field, size_t npts,
                                 const float* xyz, int device_in, const float T_init[16], const revo_map_align_params* prm,
                                 const revo_map_align_opts* opt, float T_out[16], revo_map_df_align_info* info_out, int32_t* iterations,
                                 int32_t* status) {
  size_t cells = 0;
  if (!T_init || !T_out || !status) return fail(REVO_ERR_INVALID_ARG, "null argument");
  TRY(dfa_check("revo_map_df_align", m, box, d2, device_field, npts, xyz, device_in, prm, &cells));
  if (!pose_is_finite(T_init)) return fail(REVO_ERR_INVALID_ARG, "T_init is not finite");
  revo_map_align_opts o{30, 0, 1e-6, 1e-6, 12};
  if (opt) o = *opt;
  if (o.max_iters < 1) return fail(REVO_ERR_INVALID_ARG, "max_iters must be >= 1");
  hipStream_t s = (hipStream_t)m->g.stream;
  DfAlignCall c;  // freed after the wait below
  int rc = dfa_begin(&c, m, box, d2, device_field, cells, npts, xyz, device_in, prm);
  if (!rc) rc = c.out.alloc(sizeof(revo_map_df_align_info));
  int32_t it = 0;
  if (!rc)
    rc = align_loop_over<revo_map_df_align_info>(
        T_init, prm->centre, o, align_df_system_fill,
        [&](const float* Tf, revo_map_df_align_info* rec) {
          TRY(dfa_launch(&c, m, 1, Tf, c.out.p));
          HIPCHECK(hipMemcpyAsync(rec, c.out.p, sizeof(*rec), hipMemcpyDeviceToHost, s));
          HIPCHECK(hipStreamSynchronize(s));
          return (int)REVO_OK;
        },
        T_out, info_out, &it, status);
  (void)hipStreamSynchronize(s);
  if (rc) return rc;
  if (iterations) *iterations = it;
  return REVO_OK;
}
