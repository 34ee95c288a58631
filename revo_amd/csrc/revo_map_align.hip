// revo_map_align.hip -- registering voxel maps: revo_map_align_eval / revo_map_align (nearest voxel), revo_map_normals and
// revo_map_align_plane_eval / revo_map_align_plane (point to plane).  Contracts: include/revo_hip.h; DESIGN 16 and 17.
#include "revo_map_impl.h"
#include "revo_track_dev.h"
#include "revo_align_host.h"

// ------------------------------------------------------------------------------------------------- registration (16) --
// revo_map_align_eval / revo_map_align (contract: include/revo_hip.h; revo_map_coarsen is a merge: revo_map.hip).
#define ALIGN_THREADS 256
#define ALIGN_WAVES (ALIGN_THREADS / 64)
#define ALIGN_CHUNK 512        // source points per chunk: workgroup g of a pose takes the chunks g, g + G, ...
#define ALIGN_MAX_GROUPS 1024  // workgroups per pose at most
#define ALIGN_PART 32          // doubles of a workgroup's partial: 16 heads, 16 tails
enum { AW_MATCHED = 16, AW_CONSIDERED = 18, AW_SKIPPED = 20, AW_CENTRE = 22, AW_MAXD = 25, AW_R = 26, AW_T = 35, AW_FLAGS = 38,
       AW_END = 40 };  // words of a revo_map_align_info record
static_assert(sizeof(revo_map_align_info) == 4 * AW_END && sizeof(revo_map_align_info) % 16 == 0 &&
              offsetof(revo_map_align_info, matched) == 4 * AW_MATCHED && offsetof(revo_map_align_info, considered) == 4 * AW_CONSIDERED &&
              offsetof(revo_map_align_info, skipped) == 4 * AW_SKIPPED && offsetof(revo_map_align_info, centre) == 4 * AW_CENTRE &&
              offsetof(revo_map_align_info, max_dist) == 4 * AW_MAXD && offsetof(revo_map_align_info, R) == 4 * AW_R &&
              offsetof(revo_map_align_info, T) == 4 * AW_T && offsetof(revo_map_align_info, flags) == 4 * AW_FLAGS,
              "record layout");
static_assert(sizeof(revo_map_plane_info) == 208 && sizeof(revo_map_plane_info) == 4 * (AW_END + 12) && sizeof(revo_map_plane_info) % 16 == 0 &&
              offsetof(revo_map_plane_info, matched) == 4 * (AW_MATCHED + 12) && offsetof(revo_map_plane_info, considered) == 4 * (AW_CONSIDERED + 12) &&
              offsetof(revo_map_plane_info, skipped) == 4 * (AW_SKIPPED + 12) && offsetof(revo_map_plane_info, centre) == 4 * (AW_CENTRE + 12) &&
              offsetof(revo_map_plane_info, max_dist) == 4 * (AW_MAXD + 12) && offsetof(revo_map_plane_info, R) == 4 * (AW_R + 12) &&
              offsetof(revo_map_plane_info, T) == 4 * (AW_T + 12) && offsetof(revo_map_plane_info, flags) == 4 * (AW_FLAGS + 12) &&
              offsetof(revo_map_plane_info, dst_normals) == 4 * (AW_FLAGS + 13),
              "the plane record is the point record with 12 more sums and the normal count in its last word");

typedef u64 __attribute__((address_space(1)))* map_gu64p;
typedef unsigned __attribute__((address_space(1)))* map_gu32p;
#define MAP_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct MapAlignK {  // what every pose of a launch shares
  const float4* pts; const unsigned* npts;                   // the source's points, compacted (k_map_align_points)
  const u64* dkeys; const float4* dmean; unsigned dmask;     // the destination's keys and, per slot, its mean (k_map_align_means)
  float voxel, maxd, maxd2, centre[3];
  const float* poses;                                        // per pose 12 floats: R column-major, t
  double* part; unsigned* cnt; unsigned* ticket;
  void* out;                                                 // revo_map_align_info or, point-to-plane, revo_map_plane_info records
  const float4* dnorm; const unsigned* dnvalid;              // point-to-plane: per slot the normal (k_map_normals), and how many are valid
};

// The per-call caches.  Source: the points of the slots with count >= min_count, compacted in arrival order (every sum over
// them is exact, so the order cannot show).  Destination: per slot the mean and, in w, whether the voxel is a candidate
// (present and count >= min_count; a slot emptied by a subtraction in flight has count 0 and is absent).
__global__ void __launch_bounds__(256) k_map_align_points(const u64* __restrict__ keys, const MapVal* __restrict__ vals, unsigned cap,
                                                          u64 min_count, unsigned* total, float4* out, unsigned cap_out) {
  __shared__ unsigned s_n, s_base;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  MapVal v{};
  bool sel = false;
  if (i < cap && keys[i] != MAP_EMPTY) { v = vals[i]; sel = v.n >= min_count; }
  const unsigned j = map_compact(sel, s_n, s_base, total);
  if (!sel || j >= cap_out) return;
  const double n = (double)v.n;
  out[j] = make_float4(map_mean(v.qx, n), map_mean(v.qy, n), map_mean(v.qz, n), 0.0f);
}
__global__ void __launch_bounds__(256) k_map_align_means(const u64* __restrict__ keys, const MapVal* __restrict__ vals, unsigned cap,
                                                         u64 min_count, float4* out) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (keys[i] != MAP_EMPTY) {
    const MapVal v = vals[i];
    if (v.n >= min_count) { const double n = (double)v.n; m = make_float4(map_mean(v.qx, n), map_mean(v.qy, n), map_mean(v.qz, n), 1.0f); }
  }
  out[i] = m;
}

// ---- per-voxel normals (17): revo_map_normals' contract, operation for operation (tests/map_plane_ref.py restates it) ----
struct MapNormalsK {
  const u64* keys; const float4* mean; unsigned mask, cap;  // the table's keys and, per slot, its mean (k_map_align_means)
  unsigned min_nb; float planarity, min_spread;
  float4* normal;    // per slot: the normal, w = 1 "valid"; all zero for an invalid, absent or under-count slot
  float4* lam;       // NULL, or per slot l0, l1, l2 and the neighbour count's bits
  unsigned* nvalid;  // += the valid normals
};

// One cyclic Jacobi rotation of the pair (p, q), r the third index: a_pq becomes 0.
__device__ __forceinline__ void normals_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float& v0p, float& v0q,
                                               float& v1p, float& v1q, float& v2p, float& v2q) {
  if (apq == 0.0f) return;
  const float theta = (aqq - app) / (2.0f * apq);
  const float t = copysignf(1.0f, theta) / (fabsf(theta) + __builtin_sqrtf(theta * theta + 1.0f));
  const float c = 1.0f / __builtin_sqrtf(t * t + 1.0f), sn = t * c;
  const float h = t * apq;
  app = app - h; aqq = aqq + h; apq = 0.0f;
  float x = arp, y = arq;
  arp = c * x - sn * y; arq = sn * x + c * y;
  x = v0p; y = v0q; v0p = c * x - sn * y; v0q = sn * x + c * y;
  x = v1p; y = v1q; v1p = c * x - sn * y; v1q = sn * x + c * y;
  x = v2p; y = v2q; v2p = c * x - sn * y; v2q = sn * x + c * y;
}

// One thread per slot: 27 probes by map_find (bounded by the table size, touching nothing), the neighbours' means from the
// cache, nine sequential float sums, the covariance, six Jacobi sweeps in registers, the validity rule.
__global__ void __launch_bounds__(256) k_map_normals(const MapNormalsK a) {
  __shared__ unsigned s_n;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  const u64 key = i < a.cap ? a.keys[i] : MAP_EMPTY;
  float4 m0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (key != MAP_EMPTY) m0 = a.mean[i];
  float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f), lam = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (m0.w != 0.0f) {
    int k0, k1, k2;
    map_key_axes(key, k0, k1, k2);
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sxx = 0.0f, sxy = 0.0f, sxz = 0.0f, syy = 0.0f, syz = 0.0f, szz = 0.0f;
    unsigned nb = 0;
#pragma unroll 1
    for (int c = 0; c < 27; ++c) {
      const int kx = k0 + c / 9 - 1, ky = k1 + (c / 3) % 3 - 1, kz = k2 + c % 3 - 1;
      if (!map_key_in_range(kx, ky, kz)) continue;
      const unsigned s = map_find(a.keys, a.mask, map_key(kx, ky, kz));
      if (s == ~0u) continue;
      const float4 q = a.mean[s];
      if (q.w == 0.0f) continue;
      const float dx = q.x - m0.x, dy = q.y - m0.y, dz = q.z - m0.z;
      sx = sx + dx; sy = sy + dy; sz = sz + dz;
      sxx = sxx + dx * dx; sxy = sxy + dx * dy; sxz = sxz + dx * dz; syy = syy + dy * dy; syz = syz + dy * dz; szz = szz + dz * dz;
      ++nb;
    }
    const float fn = (float)nb;
    float a00 = sxx - (sx * sx) / fn, a01 = sxy - (sx * sy) / fn, a02 = sxz - (sx * sz) / fn;
    float a11 = syy - (sy * sy) / fn, a12 = syz - (sy * sz) / fn, a22 = szz - (sz * sz) / fn;
    float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v20 = 0.0f, v21 = 0.0f, v22 = 1.0f;
#pragma unroll 1
    for (int sweep = 0; sweep < 6; ++sweep) {
      normals_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);  // (0, 1), r = 2
      normals_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);  // (0, 2), r = 1
      normals_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);  // (1, 2), r = 0
    }
    // the smallest eigenvalue's column and the sorted triple, ties to the lower index
    float l0 = a00, l1 = a11, l2 = a22, nx = v00, ny = v10, nz = v20;
    if (l1 < l0) { const float t = l0; l0 = l1; l1 = t; nx = v01; ny = v11; nz = v21; }
    if (l2 < l0) { const float t = l0; l0 = l2; l2 = l1; l1 = t; nx = v02; ny = v12; nz = v22; }
    else if (l2 < l1) { const float t = l1; l1 = l2; l2 = t; }
    const float norm = __builtin_sqrtf((nx * nx + ny * ny) + nz * nz);
    nx = nx / norm; ny = ny / norm; nz = nz / norm;
    const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
    const float big = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
    if (big < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    const bool valid = nb >= a.min_nb && __builtin_isfinite(nx) && __builtin_isfinite(ny) && __builtin_isfinite(nz) && l1 > 0.0f &&
                       l0 <= a.planarity * l1 && l1 >= a.min_spread * l2;
    if (valid) { out = make_float4(nx, ny, nz, 1.0f); atomicAdd(&s_n, 1u); }
    lam = make_float4(l0, l1, l2, __uint_as_float(nb));
  }
  if (i < a.cap) {
    a.normal[i] = out;
    if (a.lam) a.lam[i] = lam;
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(a.nvalid, s_n);
}

// The voxels of k_map_extract's selection (mean.w != 0) with their normal rows, compacted in arrival order (the host sorts by
// key); at most cap_out are written.
__global__ void __launch_bounds__(256) k_map_normals_export(const u64* __restrict__ keys, const float4* __restrict__ mean,
                                                            const float4* __restrict__ normal, const float4* __restrict__ lam, unsigned cap,
                                                            unsigned* total, u64* okey, float4* omean, float4* onormal, float4* olam,
                                                            unsigned cap_out) {
  __shared__ unsigned s_n, s_base;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  const u64 key = i < cap ? keys[i] : MAP_EMPTY;
  float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (key != MAP_EMPTY) m = mean[i];
  const bool sel = m.w != 0.0f;
  const unsigned j = map_compact(sel, s_n, s_base, total);
  if (!sel || j >= cap_out) return;
  okey[j] = key; omean[j] = m; onormal[j] = normal[i]; olam[j] = lam[i];
}

// 16 double-double values: lane L ends with the wave total of value align_slot(L & 15) in h[0], l[0] (reduce32x's tree)
__device__ __forceinline__ int align_slot(int lane) { return ((lane & 1) << 3) | ((lane & 2) << 1) | ((lane & 4) >> 1) | ((lane & 8) >> 3); }
__device__ __forceinline__ void align_reduce16(double* h, double* l, int lane) {
  butterfly_step_x<8, 1>(h, l, lane);
  butterfly_step_x<4, 2>(h, l, lane);
  butterfly_step_x<2, 4>(h, l, lane);
  butterfly_step_x<1, 8>(h, l, lane);
  dd_add(h[0], l[0], lane_xor_d<16>(h[0]), lane_xor_d<16>(l[0]));
  dd_add(h[0], l[0], lane_xor_d<32>(h[0]), lane_xor_d<32>(l[0]));
}

// Grid (G, poses), revo_info.hip's shape: workgroup g of a pose takes the chunks g, g + G, ... of the source's points, one
// point per thread and round.  Per point: p', its voxel index in the destination, the nearest of the up to 27 candidates
// around it by (d2, key) -- a bounded probe per candidate that touches nothing, a miss being the normal case -- and, if the
// match is accepted, the point's float terms into 16 double-double sums.  Per workgroup: wave butterfly, LDS, the partial
// published write-through, a ticket; whoever draws the last one adds the G partials in a fixed order and writes the record.
//
// PLANE: the same kernel for the point-to-plane record.  A candidate also needs a valid normal; an accepted match
// contributes 28 terms (the upper triangle of J J^T, J e, e e) into 32 double-double slots (reduce32x's tree, four stay zero);
// the record's S is 12 words longer, so every word behind it moves by 12, and its last word counts the valid normals.
template <bool PLANE>
__device__ __forceinline__ void map_align_body(const MapAlignK& a) {
  constexpr int NS = PLANE ? 32 : 16;    // double-double slots
  constexpr int NSUM = PLANE ? 28 : 16;  // sums of the record
  constexpr int OFF = PLANE ? 12 : 0;    // where the words behind S lie
  constexpr int END = AW_END + OFF, PART = 2 * NS;
  __shared__ double s_h[ALIGN_WAVES][NS], s_l[ALIGN_WAVES][NS];
  __shared__ unsigned s_c[ALIGN_WAVES][2];
  const int pose = blockIdx.y, grp = blockIdx.x, G = gridDim.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  unsigned* const rec = (unsigned*)a.out + (size_t)pose * END;

  const float* P = a.poses + 12 * (size_t)pose;
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
  for (int i = 0; i < 3; ++i) tail = lane == AW_CENTRE + OFF + i ? __float_as_uint(a.centre[i]) : tail;
  tail = lane == AW_MAXD + OFF ? __float_as_uint(a.maxd) : tail;
#pragma unroll
  for (int i = 0; i < 9; ++i) tail = lane == AW_R + OFF + i ? Rb[i] : tail;
#pragma unroll
  for (int i = 0; i < 3; ++i) tail = lane == AW_T + OFF + i ? Tb[i] : tail;
  tail = lane == AW_FLAGS + OFF ? (no_eval ? 1u : 0u) : tail;
  if (no_eval) {  // the same for every workgroup of the pose
    if (grp == 0 && tid < END) rec[tid] = tail;
    return;
  }

  unsigned N = *a.npts;
  double xd[PART];  // the double-double slots: heads, then tails
#pragma unroll
  for (int k = 0; k < PART; ++k) xd[k] = 0.0;
  unsigned matched = 0, skipped = 0;
  const unsigned nchunks = (N + ALIGN_CHUNK - 1) / ALIGN_CHUNK;
  for (unsigned ch = grp; ch < nchunks; ch += G) {
    const unsigned end = (ch + 1) * ALIGN_CHUNK < N ? (ch + 1) * ALIGN_CHUNK : N;
#pragma unroll 1
    for (unsigned i = ch * ALIGN_CHUNK + tid; i < end; i += ALIGN_THREADS) {
      const float4 p = a.pts[i];
      float pt[3];
      int k[3];
      bool ok = true;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        pt[c] = ((R[c] * p.x + R[3 + c] * p.y) + R[6 + c] * p.z) + T[c];
        const float f = floorf(__fdiv_rn(pt[c], a.voxel));
        ok = ok && fabsf(pt[c]) < 2048.0f && f >= -1048576.0f && f <= 1048575.0f;  // NaN / inf fail every comparison
        k[c] = ok ? (int)f : 0;
      }
      if (!ok) { ++skipped; continue; }
      float best = 0.0f, bq[3] = {0.0f, 0.0f, 0.0f};
      u64 bkey = MAP_EMPTY;  // no candidate yet: every packed key is smaller
      unsigned bs = 0u;      // PLANE: the match's slot, for its normal
#pragma unroll 1
      for (int c = 0; c < 27; ++c) {
        const int kx = k[0] + c / 9 - 1, ky = k[1] + (c / 3) % 3 - 1, kz = k[2] + c % 3 - 1;
        if (!map_key_in_range(kx, ky, kz)) continue;
        const u64 key = map_key(kx, ky, kz);
        const unsigned s = map_find(a.dkeys, a.dmask, key);
        if (s == ~0u) continue;
        const float4 q = a.dmean[s];
        if (q.w == 0.0f) continue;
        if (PLANE && a.dnorm[s].w == 0.0f) continue;
        const float dx = pt[0] - q.x, dy = pt[1] - q.y, dz = pt[2] - q.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (bkey == MAP_EMPTY || d2 < best || (d2 == best && key < bkey)) { best = d2; bkey = key; bq[0] = q.x; bq[1] = q.y; bq[2] = q.z; if (PLANE) bs = s; }
      }
      if (bkey == MAP_EMPTY || !(best <= a.maxd2)) continue;
      ++matched;
      const float ux = pt[0] - a.centre[0], uy = pt[1] - a.centre[1], uz = pt[2] - a.centre[2];
      const float rx = pt[0] - bq[0], ry = pt[1] - bq[1], rz = pt[2] - bq[2];
#define ALIGN_ACC(slot, term) dd_acc(xd[slot], xd[NS + (slot)], (double)(term))
      if constexpr (PLANE) {
        const float4 nv = a.dnorm[bs];
        const float e = (nv.x * rx + nv.y * ry) + nv.z * rz;
        const float J[6] = {nv.x, nv.y, nv.z, uy * nv.z - uz * nv.y, uz * nv.x - ux * nv.z, ux * nv.y - uy * nv.x};
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = i; j < 6; ++j) { ALIGN_ACC(k, J[i] * J[j]); ++k; }
#pragma unroll
        for (int i = 0; i < 6; ++i) ALIGN_ACC(21 + i, J[i] * e);
        ALIGN_ACC(27, e * e);
        continue;
      }
      ALIGN_ACC(0, ux); ALIGN_ACC(1, uy); ALIGN_ACC(2, uz);
      ALIGN_ACC(3, ux * ux); ALIGN_ACC(4, ux * uy); ALIGN_ACC(5, ux * uz); ALIGN_ACC(6, uy * uy); ALIGN_ACC(7, uy * uz); ALIGN_ACC(8, uz * uz);
      ALIGN_ACC(9, rx); ALIGN_ACC(10, ry); ALIGN_ACC(11, rz);
      ALIGN_ACC(12, uy * rz); ALIGN_ACC(12, -(uz * ry));
      ALIGN_ACC(13, uz * rx); ALIGN_ACC(13, -(ux * rz));
      ALIGN_ACC(14, ux * ry); ALIGN_ACC(14, -(uy * rx));
      ALIGN_ACC(15, rx * rx); ALIGN_ACC(15, ry * ry); ALIGN_ACC(15, rz * rz);
#undef ALIGN_ACC
    }
  }
  if constexpr (PLANE) reduce32x(xd, xd + NS, lane);  // lane L: the wave's total of slot idx32(L & 31)
  else align_reduce16(xd, xd + NS, lane);             // lane L: the wave's total of slot align_slot(L & 15)
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { matched += __shfl_xor(matched, off, 64); skipped += __shfl_xor(skipped, off, 64); }
  if (lane < NS) {
    const int slot = PLANE ? idx32(lane) : align_slot(lane);
    s_h[wave][slot] = xd[0]; s_l[wave][slot] = xd[NS];
  }
  if (lane == 0) { s_c[wave][0] = matched; s_c[wave][1] = skipped; }
  __syncthreads();
  if (wave != 0) return;

  // wave 0: the workgroup's partial (waves in index order), published write-through, then the ticket
  const int k = lane & (NS - 1);
  double h = s_h[0][k], l = s_l[0][k];
  unsigned c = lane < 2 ? s_c[0][lane] : 0u;
#pragma unroll
  for (int w = 1; w < ALIGN_WAVES; ++w) { dd_add(h, l, s_h[w][k], s_l[w][k]); c += lane < 2 ? s_c[w][lane] : 0u; }
  map_gu64p mine = (map_gu64p)(a.part + ((size_t)pose * G + grp) * PART);
  if (lane < NS) {
    __hip_atomic_store(mine + k, (u64)__double_as_longlong(h), MAP_RLX_AGENT);
    __hip_atomic_store(mine + NS + k, (u64)__double_as_longlong(l), MAP_RLX_AGENT);
  }
  map_gu32p cnts = (map_gu32p)(a.cnt + ((size_t)pose * G) * 2);
  if (lane < 2) __hip_atomic_store(cnts + 2 * grp + lane, c, MAP_RLX_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the partial has left this CU before the ticket is drawn
  unsigned drawn = 0u;
  if (lane == 0) drawn = __hip_atomic_fetch_add((map_gu32p)(a.ticket + pose), 1u, MAP_RLX_AGENT);
  drawn = (unsigned)__builtin_amdgcn_readfirstlane((int)drawn);
  if (drawn != (unsigned)(G - 1)) return;

  // the last workgroup of the pose to arrive: every partial is published.  Lane L adds slot L & (NS - 1) of the groups L / NS,
  // L / NS + 64 / NS, ... in index order (16 slots: four lane groups; 32 slots: two); the group sums meet across the lanes.
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  map_gu64p all = (map_gu64p)(a.part + (size_t)pose * G * PART);
  h = 0.0; l = 0.0;
  u64 n_matched = 0, n_skipped = 0;
  for (int g = lane / NS; g < G; g += 64 / NS) {
    const double gh = __longlong_as_double((long long)__hip_atomic_load(all + (size_t)g * PART + k, MAP_RLX_AGENT));
    const double gl = __longlong_as_double((long long)__hip_atomic_load(all + (size_t)g * PART + NS + k, MAP_RLX_AGENT));
    dd_add(h, l, gh, gl);
  }
  if (!PLANE) dd_add(h, l, lane_xor_d<16>(h), lane_xor_d<16>(l));
  dd_add(h, l, lane_xor_d<32>(h), lane_xor_d<32>(l));
  for (int g = 0; g < G; ++g) {
    n_matched += __hip_atomic_load(cnts + 2 * g, MAP_RLX_AGENT);
    n_skipped += __hip_atomic_load(cnts + 2 * g + 1, MAP_RLX_AGENT);
  }
  const float f = dd_to_float(h, l);
  unsigned w = tail;
  w = lane < NSUM ? __float_as_uint(f) : w;
  w = lane == AW_MATCHED + OFF ? (unsigned)n_matched : (lane == AW_MATCHED + OFF + 1 ? (unsigned)(n_matched >> 32) : w);
  w = lane == AW_CONSIDERED + OFF ? N : w;
  w = lane == AW_SKIPPED + OFF ? (unsigned)n_skipped : (lane == AW_SKIPPED + OFF + 1 ? (unsigned)(n_skipped >> 32) : w);
  if constexpr (PLANE) {
    const unsigned nv = *a.dnvalid;
    w = lane == AW_FLAGS + OFF + 1 ? (nv < 0x7fffffffu ? nv : 0x7fffffffu) : w;
  }
  if (lane < END) rec[lane] = w;
}
__global__ void __launch_bounds__(ALIGN_THREADS) k_map_align(const MapAlignK a) { map_align_body<false>(a); }
__global__ void __launch_bounds__(ALIGN_THREADS) k_map_align_plane(const MapAlignK a) { map_align_body<true>(a); }

// The caches and scratch of one registration call: built once, used by every evaluation of the call, freed at its end.
struct MapAlignCall {
  revo_map* dst = nullptr;
  char* buf = nullptr;
  MapAlignK k{};
  float* h_pose = nullptr;  // pinned, n_max x 12
  float* d_pose = nullptr;
  void* d_out = nullptr;  // n_max records
  size_t rec_bytes = sizeof(revo_map_align_info);
  bool plane = false;     // point-to-plane: the normal table is part of the caches, the records are revo_map_plane_info
  int n_max = 0, groups = 1;
  ~MapAlignCall() {
    if (dst) { (void)hipStreamSynchronize((hipStream_t)dst->g.stream); }
    (void)hipFree(buf); (void)hipHostFree(h_pose);
    (void)hipGetLastError();
  }
};

static int align_check(revo_map* dst, revo_map* src, const revo_map_align_params* prm) {
  if (!dst || !src || !prm) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!std::isfinite(prm->max_dist) || !(prm->max_dist > 0.0f) || !(prm->max_dist <= dst->voxel))
    return fail(REVO_ERR_INVALID_ARG, "max_dist must be finite, > 0 and at most the destination's voxel edge");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(prm->centre[i])) return fail(REVO_ERR_INVALID_ARG, "the centre is not finite");
  if (dst->g.device != src->g.device) return fail(REVO_ERR_INVALID_ARG, "the maps are on different devices");
  return REVO_OK;
}

static int normals_check(const revo_map_normals_params* prm);
static void normals_launch(hipStream_t s, revo_map* m, const float4* d_mean, const revo_map_normals_params& prm, float4* d_normal,
                           float4* d_lam, unsigned* d_nvalid);

// Waits for src (as revo_map_merge does), then enqueues the cache launches on dst's stream: the source's points, the
// destination's means and, for the point-to-plane metric (nprm != NULL), its normals.
static int align_begin(MapAlignCall* c, revo_map* dst, revo_map* src, const revo_map_align_params* prm, int n_max,
                       const revo_map_normals_params* nprm = nullptr) {
  MapStats ss;
  TRY(map_read_stats(src, &ss));
  HIPCHECK(hipSetDevice(dst->g.device));
  hipStream_t s = (hipStream_t)dst->g.stream;
  const size_t npts = std::max<size_t>((size_t)ss.occ, 1);
  c->n_max = n_max;
  c->plane = nprm != nullptr;
  c->rec_bytes = c->plane ? sizeof(revo_map_plane_info) : sizeof(revo_map_align_info);
  const size_t part = c->plane ? 64 : ALIGN_PART;  // doubles of a workgroup's partial
  c->groups = (int)std::min<size_t>(ALIGN_MAX_GROUPS, (npts + ALIGN_CHUNK - 1) / ALIGN_CHUNK);
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  // the words a launch zeroes (tickets) and the point count open the allocation, each a block of its own
  const size_t o_tick = 0, o_npts = o_tick + up(sizeof(unsigned) * n_max), o_pts = o_npts + 256, o_mean = o_pts + up(sizeof(float4) * npts),
               o_pose = o_mean + up(sizeof(float4) * dst->cap), o_part = o_pose + up(sizeof(float) * 12 * n_max),
               o_cnt = o_part + up(sizeof(double) * part * c->groups * n_max), o_out = o_cnt + up(sizeof(unsigned) * 2 * c->groups * n_max),
               o_norm = o_out + up(c->rec_bytes * n_max), total = o_norm + (c->plane ? up(sizeof(float4) * dst->cap) : 0);
  HIPCHECK(hipMalloc((void**)&c->buf, total));
  HIPCHECK(hipHostMalloc((void**)&c->h_pose, sizeof(float) * 12 * n_max));
  c->dst = dst;
  MapAlignK& k = c->k;
  k.ticket = (unsigned*)(c->buf + o_tick);
  unsigned* d_npts = (unsigned*)(c->buf + o_npts);
  float4* d_pts = (float4*)(c->buf + o_pts);
  float4* d_mean = (float4*)(c->buf + o_mean);
  c->d_pose = (float*)(c->buf + o_pose);
  k.pts = d_pts; k.npts = d_npts; k.dkeys = dst->d_keys; k.dmean = d_mean; k.dmask = (unsigned)(dst->cap - 1);
  k.voxel = dst->voxel; k.maxd = prm->max_dist; k.maxd2 = prm->max_dist * prm->max_dist;
  for (int i = 0; i < 3; ++i) k.centre[i] = prm->centre[i];
  k.poses = c->d_pose;
  k.part = (double*)(c->buf + o_part); k.cnt = (unsigned*)(c->buf + o_cnt);
  c->d_out = c->buf + o_out;
  HIPCHECK(hipMemsetAsync(d_npts, 0, 16, s));  // the point count and, behind it, the count of valid normals
  hipLaunchKernelGGL(k_map_align_points, dim3((unsigned)((src->cap + 255) / 256)), dim3(256), 0, s, src->d_keys, src->d_vals,
                     (unsigned)src->cap, (u64)std::max<uint32_t>(prm->min_count_src, 1), d_npts, d_pts, (unsigned)npts);
  hipLaunchKernelGGL(k_map_align_means, dim3((unsigned)((dst->cap + 255) / 256)), dim3(256), 0, s, dst->d_keys, dst->d_vals,
                     (unsigned)dst->cap, (u64)std::max<uint32_t>(prm->min_count_dst, 1), d_mean);
  if (c->plane) {
    float4* d_norm = (float4*)(c->buf + o_norm);
    normals_launch(s, dst, d_mean, *nprm, d_norm, nullptr, d_npts + 1);
    k.dnorm = d_norm; k.dnvalid = d_npts + 1;
  }
  HIPCHECK(hipGetLastError());
  return REVO_OK;
}

// n <= n_max poses (4x4 column-major) in one launch; records to `out` (device memory) or, out == NULL, to the call's own.
static int align_launch(MapAlignCall* c, int n, const float* T16, void* d_out) {
  hipStream_t s = (hipStream_t)c->dst->g.stream;
  HIPCHECK(hipStreamSynchronize(s));  // the previous upload has read the pinned poses
  for (int i = 0; i < n; ++i) {
    const float* T = T16 + 16 * (size_t)i;
    float* P = c->h_pose + 12 * (size_t)i;
    for (int col = 0; col < 3; ++col)
      for (int r = 0; r < 3; ++r) P[3 * col + r] = T[4 * col + r];
    for (int r = 0; r < 3; ++r) P[9 + r] = T[12 + r];
  }
  HIPCHECK(hipMemcpyAsync(c->d_pose, c->h_pose, sizeof(float) * 12 * n, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemsetAsync(c->k.ticket, 0, (sizeof(unsigned) * n + 15) / 16 * 16, s));
  MapAlignK k = c->k;
  k.out = d_out ? d_out : c->d_out;
  if (c->plane) hipLaunchKernelGGL(k_map_align_plane, dim3((unsigned)c->groups, (unsigned)n), dim3(ALIGN_THREADS), 0, s, k);
  else hipLaunchKernelGGL(k_map_align, dim3((unsigned)c->groups, (unsigned)n), dim3(ALIGN_THREADS), 0, s, k);
  HIPCHECK(hipGetLastError());
  return REVO_OK;
}

static int align_eval_host(MapAlignCall* c, const float T[16], void* out) {
  TRY(align_launch(c, 1, T, nullptr));
  hipStream_t s = (hipStream_t)c->dst->g.stream;
  HIPCHECK(hipMemcpyAsync(out, c->d_out, c->rec_bytes, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

static int plane_params(const revo_map_align_params* prm, const revo_map_normals_params* nprm, revo_map_normals_params* out);

// revo_map_align_eval and, plane, revo_map_align_plane_eval (records of rec_bytes bytes): n poses, one launch
static int align_eval_any(const char* name, revo_map* dst, revo_map* src, int n, const float* T, const revo_map_align_params* prm,
                          bool plane, const revo_map_normals_params* nprm, void* out, size_t rec_bytes, int device_out) {
  TRY(align_check(dst, src, prm));
  if (!T || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n < 1 || n > 65535) return fail(REVO_ERR_INVALID_ARG, std::string(name) + ": n must be 1 .. 65535");
  TRY(map_check_side(device_out, "device_out"));
  if (device_out) TRY(map_check_aligned((uintptr_t)out, 16, "the device output is"));
  revo_map_normals_params np;
  if (plane) TRY(plane_params(prm, nprm, &np));
  MapAlignCall c;
  TRY(align_begin(&c, dst, src, prm, n, plane ? &np : nullptr));
  TRY(align_launch(&c, n, T, device_out ? out : nullptr));
  hipStream_t s = (hipStream_t)dst->g.stream;
  if (!device_out) HIPCHECK(hipMemcpyAsync(out, c.d_out, rec_bytes * n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}
extern "C" int revo_map_align_eval(revo_map* dst, revo_map* src, int n, const float* T, const revo_map_align_params* prm,
                                   revo_map_align_info* out, int device_out) {
  return align_eval_any("revo_map_align_eval", dst, src, n, T, prm, false, nullptr, out, sizeof(*out), device_out);
}

extern "C" int revo_map_align_system(const revo_map_align_info* info, double H[36], double g[6]) {
  if (!info || !H || !g) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (info->flags & 1) return fail(REVO_ERR_INVALID_ARG, "the record carries no evaluation (flags bit0)");
  align_system_fill(info, H, g);
  return REVO_OK;
}

extern "C" int revo_map_align(revo_map* dst, revo_map* src, const float T_init[16], const revo_map_align_params* prm,
                              const revo_map_align_opts* opt, float T_out[16], revo_map_align_info* info_out, int32_t* iterations,
                              int32_t* status) {
  TRY(align_check(dst, src, prm));
  if (!T_init || !T_out || !status) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!pose_is_finite(T_init)) return fail(REVO_ERR_INVALID_ARG, "T_init is not finite");
  revo_map_align_opts o{30, 0, 1e-6, 1e-6, 12};
  if (opt) o = *opt;
  if (o.max_iters < 1) return fail(REVO_ERR_INVALID_ARG, "max_iters must be >= 1");
  MapAlignCall c;
  TRY(align_begin(&c, dst, src, prm, 1));
  int32_t it = 0;
  const int rc = align_loop(T_init, prm->centre, o, [&](const float* Tf, revo_map_align_info* rec) { return align_eval_host(&c, Tf, rec); },
                            T_out, info_out, &it, status);
  if (rc) return rc;
  if (iterations) *iterations = it;
  return REVO_OK;
}

// ------------------------------------------------------------------------------------ point-to-plane registration (17) --
// revo_map_normals / revo_map_align_plane_eval / revo_map_align_plane (contract: include/revo_hip.h).
static int normals_check(const revo_map_normals_params* p) {
  if (p->min_neighbours < 3) return fail(REVO_ERR_INVALID_ARG, "min_neighbours must be >= 3");
  if (!std::isfinite(p->planarity) || !(p->planarity > 0.0f) || !(p->planarity < 1.0f))
    return fail(REVO_ERR_INVALID_ARG, "planarity must be finite, > 0 and < 1");
  if (!std::isfinite(p->min_spread) || !(p->min_spread >= 0.0f) || !(p->min_spread < 1.0f))
    return fail(REVO_ERR_INVALID_ARG, "min_spread must be finite, >= 0 and < 1");
  return REVO_OK;
}

// d_mean: k_map_align_means' table for max(prm.min_count, 1), enqueued before this on the same stream
static void normals_launch(hipStream_t s, revo_map* m, const float4* d_mean, const revo_map_normals_params& prm, float4* d_normal,
                           float4* d_lam, unsigned* d_nvalid) {
  MapNormalsK k{};
  k.keys = m->d_keys; k.mean = d_mean; k.mask = (unsigned)(m->cap - 1); k.cap = (unsigned)m->cap;
  k.min_nb = prm.min_neighbours; k.planarity = prm.planarity; k.min_spread = prm.min_spread;
  k.normal = d_normal; k.lam = d_lam; k.nvalid = d_nvalid;
  hipLaunchKernelGGL(k_map_normals, dim3((unsigned)((m->cap + 255) / 256)), dim3(256), 0, s, k);
}

extern "C" int revo_map_normals(revo_map* m, const revo_map_normals_params* prm, float* xyz, float* normal, float* lambda,
                                uint32_t* neighbours, size_t cap, size_t* n) {
  if (!m || !n) return fail(REVO_ERR_INVALID_ARG, "null argument");
  revo_map_normals_params p{1, 5, 0.1f, 0.1f};
  if (prm) p = *prm;
  TRY(normals_check(&p));
  MapStats st;
  TRY(map_read_stats(m, &st));
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t nv = std::max<size_t>((size_t)st.occ, 1), slots = m->cap;
  // per slot: mean, normal, lambda; per voxel: key and the same three rows, compacted; the two counters
  const size_t o_cnt = 0, o_mean = 256, o_norm = o_mean + 16 * slots, o_lam = o_norm + 16 * slots, o_key = o_lam + 16 * slots,
               o_xm = o_key + 16 * ((8 * nv + 15) / 16), o_xn = o_xm + 16 * nv, o_xl = o_xn + 16 * nv, total = o_xl + 16 * nv;
  DevScratch scratch;
  TRY(scratch.alloc(total));
  char* buf = scratch.p;
  unsigned* d_cnt = (unsigned*)(buf + o_cnt);  // [0] the voxels exported, [1] the valid normals
  float4* d_mean = (float4*)(buf + o_mean);
  HIPCHECK(hipMemsetAsync(d_cnt, 0, 16, s));
  hipLaunchKernelGGL(k_map_align_means, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, m->d_keys, m->d_vals, (unsigned)slots,
                     (u64)std::max<uint32_t>(p.min_count, 1), d_mean);
  normals_launch(s, m, d_mean, p, (float4*)(buf + o_norm), (float4*)(buf + o_lam), d_cnt + 1);
  hipLaunchKernelGGL(k_map_normals_export, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, m->d_keys, d_mean,
                     (const float4*)(buf + o_norm), (const float4*)(buf + o_lam), (unsigned)slots, d_cnt, (u64*)(buf + o_key),
                     (float4*)(buf + o_xm), (float4*)(buf + o_xn), (float4*)(buf + o_xl), (unsigned)nv);
  HIPCHECK(hipGetLastError());
  unsigned tot = 0;
  HIPCHECK(hipMemcpyAsync(&tot, d_cnt, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (tot > nv) return fail(REVO_ERR_HIP, "voxel map: the table holds more voxels than its counter says");
  *n = tot;
  if (!xyz && !normal && !lambda && !neighbours) return REVO_OK;
  if (cap < tot) return fail(REVO_ERR_CAPACITY, "voxel map: the output holds fewer voxels than the map has");
  std::vector<u64> key(tot);
  std::vector<float> pm(4 * (size_t)tot), pn(4 * (size_t)tot), pl(4 * (size_t)tot);
  if (tot) {
    HIPCHECK(hipMemcpy(key.data(), buf + o_key, 8 * (size_t)tot, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(pm.data(), buf + o_xm, 16 * (size_t)tot, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(pn.data(), buf + o_xn, 16 * (size_t)tot, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(pl.data(), buf + o_xl, 16 * (size_t)tot, hipMemcpyDeviceToHost));
  }
  std::vector<unsigned> idx(tot);
  std::iota(idx.begin(), idx.end(), 0u);
  std::sort(idx.begin(), idx.end(), [&](unsigned a, unsigned b) { return key[a] < key[b]; });  // keys are distinct
  for (size_t j = 0; j < tot; ++j) {
    const size_t i = idx[j];
    if (xyz) memcpy(xyz + 3 * j, &pm[4 * i], 12);
    if (normal) memcpy(normal + 3 * j, &pn[4 * i], 12);
    if (lambda) memcpy(lambda + 3 * j, &pl[4 * i], 12);
    if (neighbours) memcpy(neighbours + j, &pl[4 * i + 3], 4);
  }
  return REVO_OK;
}

// the normal parameters of a point-to-plane call: the defaults at the destination's count threshold, or the caller's checked
static int plane_params(const revo_map_align_params* prm, const revo_map_normals_params* nprm, revo_map_normals_params* out) {
  const uint32_t mc = std::max<uint32_t>(prm->min_count_dst, 1);
  *out = revo_map_normals_params{mc, 5, 0.1f, 0.1f};
  if (!nprm) return REVO_OK;
  *out = *nprm;
  if (nprm->min_count != mc) return fail(REVO_ERR_INVALID_ARG, "the normals' min_count must equal max(min_count_dst, 1)");
  return normals_check(out);
}

extern "C" int revo_map_align_plane_eval(revo_map* dst, revo_map* src, int n, const float* T, const revo_map_align_params* prm,
                                         const revo_map_normals_params* nprm, revo_map_plane_info* out, int device_out) {
  return align_eval_any("revo_map_align_plane_eval", dst, src, n, T, prm, true, nprm, out, sizeof(*out), device_out);
}

extern "C" int revo_map_align_plane_system(const revo_map_plane_info* info, double H[36], double g[6]) {
  if (!info || !H || !g) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (info->flags & 1) return fail(REVO_ERR_INVALID_ARG, "the record carries no evaluation (flags bit0)");
  align_plane_system_fill(info, H, g);
  return REVO_OK;
}

extern "C" int revo_map_align_plane(revo_map* dst, revo_map* src, const float T_init[16], const revo_map_align_params* prm,
                                    const revo_map_normals_params* nprm, const revo_map_align_opts* opt, float T_out[16],
                                    revo_map_plane_info* info_out, int32_t* iterations, int32_t* status) {
  TRY(align_check(dst, src, prm));
  if (!T_init || !T_out || !status) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!pose_is_finite(T_init)) return fail(REVO_ERR_INVALID_ARG, "T_init is not finite");
  revo_map_align_opts o{30, 0, 1e-6, 1e-6, 12};
  if (opt) o = *opt;
  if (o.max_iters < 1) return fail(REVO_ERR_INVALID_ARG, "max_iters must be >= 1");
  revo_map_normals_params np;
  TRY(plane_params(prm, nprm, &np));
  MapAlignCall c;
  TRY(align_begin(&c, dst, src, prm, 1, &np));
  int32_t it = 0;
  const int rc = align_loop_over<revo_map_plane_info>(T_init, prm->centre, o, align_plane_system_fill,
                                                      [&](const float* Tf, revo_map_plane_info* rec) { return align_eval_host(&c, Tf, rec); },
                                                      T_out, info_out, &it, status);
  if (rc) return rc;
  if (iterations) *iterations = it;
  return REVO_OK;
}
