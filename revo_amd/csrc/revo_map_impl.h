// revo_map_impl.h -- what the voxel map's translation units (revo_map.hip, revo_map_view.hip, revo_map_align.hip,
// revo_map_edit.hip, revo_map_field.hip, revo_map_df_align.hip, revo_map_plan.hip, revo_map_seen.hip, revo_map_gain.hip, revo_map_tsdf.hip, revo_map_tsdf_ray.hip, revo_map_tsdf_track.hip, revo_map_tsdf_follow.hip, revo_map_tsdf_many.hip, revo_map_tsdf_unfuse.hip) share: the table's device vocabulary (key, record, mean, compaction -- each contract written once), the
// map handle with the host pieces every entry point uses, and the host functions that cross units.  Internal: only the map's
// units include it.  The owners of device resources it is written with (DevBuf, DevScratch, HostRows, EventTimer, TRY) are the
// library's, of revo_internal.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <numeric>
#include <string>
#include <vector>

#include "revo_internal.h"
#include "revo_map.h"
#include "revo_pose_host.h"
#include "revo_carve_host.h"
#include "revo_ray_host.h"

#define MAP_EMPTY 0xffffffffffffffffull  // no packed key reaches bit 63
#define MAP_SHARDS 16                    // per-map batch counters, one 128-B line each (one global atomic per block and counter)
#define MAP_MAX_CAP (1ull << 31)
#define MAP_MAX_VOXELS (1ull << 28)
#define MAP_POISON (1ull << 40)  // > MAP_MAX_VOXELS: a batch whose new-voxel count holds it is refused by k_map_commit

typedef unsigned long long u64;

struct MapVal { u64 n, qx, qy, qz, sb, sg, sr, pad; };  // count, sum q (two's complement int64), sum B, G, R
struct MapStats {
  u64 occ, pts, drop, kfs, rejected, fault;
  u64 ok, bad;  // bad: k_map_merge met a record with count 0 or key bit 63 (the host clears it before such a launch)
  u64 shard[MAP_SHARDS][16];  // [0] new voxels, [1] points, [2] dropped points of the batch in flight
  // the subtraction in flight (behind the shards: no older field moves): refused, points taken, voxels whose count reached 0
  u64 sub_bad, sub_pts, sub_freed;
};
enum { MAP_FUSED = 0, MAP_INSERT = 1, MAP_ACCUM = 2 };
struct MapMergeK {
  const u64* skeys; const MapVal* svals;  // MERGE_TABLE: the source map's table, n slots
  const ulonglong2* recs;                 // MERGE_RAW: n records
  unsigned n;
  u64* keys; MapVal* vals; unsigned mask;
  MapStats* st;
  u64 dropped;  // joins the batch's dropped points once
  int shift;    // MERGE_COARSE: every axis index of a source key is shifted right by this (revo_map_coarsen)
};
enum { MERGE_RAW = 0, MERGE_TABLE = 1, MERGE_COARSE = 2 };  // MERGE_COARSE: MERGE_TABLE with the keys rewritten
static_assert(sizeof(revo_map_voxel_raw) == 64 && sizeof(MapVal) == 64, "a voxel record is four 16-byte words");

// ------------------------------------------------------------------------------------------------- device vocabulary --
__device__ __forceinline__ bool map_depth_ok(float Z, float dmin, float dmax) {
  return isfinite(Z) && Z > dmin && Z < dmax;  // depth_ok of revo_pyramid.hip (imgpyramidrgbd.cpp:208)
}
__device__ __forceinline__ u64 map_hash(u64 k) {  // splitmix64 finaliser
  k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
  k ^= k >> 27; k *= 0x94d049bb133111ebull;
  return k ^ (k >> 31);
}
// The slot of `key`, inserted if absent (INSERT) or looked up.  Probing is bounded by the table size (the host keeps the
// load <= 0.5, so a full table means a broken invariant: counted in fault, never a hang).
template <bool INSERT>
__device__ __forceinline__ unsigned map_slot(u64* keys, unsigned mask, u64 key, unsigned* n_new, u64* fault) {
  unsigned s = (unsigned)map_hash(key) & mask;
  for (unsigned i = 0; i <= mask; ++i) {
    u64 k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == key) return s;
    if (k == MAP_EMPTY) {
      if (!INSERT) break;
      k = atomicCAS(&keys[s], MAP_EMPTY, key);
      if (k == MAP_EMPTY) { if (n_new) atomicAdd(n_new, 1u); return s; }
      if (k == key) return s;
    }
    s = (s + 1) & mask;
  }
  atomicOr(fault, 1ull);
  return ~0u;
}
// The slot of `key`, or ~0u: a lookup that touches nothing (a miss is the caller's business, not a broken table).  For tables
// whose keys do not change while the kernel runs, so plain loads do.
__device__ __forceinline__ unsigned map_find(const u64* __restrict__ keys, unsigned mask, u64 key) {
  unsigned s = (unsigned)map_hash(key) & mask;
  for (unsigned i = 0; i <= mask; ++i) {
    const u64 k = keys[s];
    if (k == key) return s;
    if (k == MAP_EMPTY) break;
    s = (s + 1) & mask;
  }
  return ~0u;
}

// The packed key of the voxel index (kx, ky, kz), each in [-2^20, 2^20 - 1]: 21 bits per axis, biased by 2^20.
__device__ __forceinline__ u64 map_key(int kx, int ky, int kz) {
  return ((u64)(kx + (1 << 20)) << 42) | ((u64)(ky + (1 << 20)) << 21) | (u64)(kz + (1 << 20));
}
__device__ __forceinline__ void map_key_axes(u64 key, int& kx, int& ky, int& kz) {
  kx = (int)((key >> 42) & 0x1fffffu) - (1 << 20); ky = (int)((key >> 21) & 0x1fffffu) - (1 << 20); kz = (int)(key & 0x1fffffu) - (1 << 20);
}
// whether (kx, ky, kz) is a voxel index at all: the neighbours of a voxel at the rim are not
__device__ __forceinline__ bool map_key_in_range(int kx, int ky, int kz) {
  return !(((kx + (1 << 20)) | (ky + (1 << 20)) | (kz + (1 << 20))) >> 21);
}
// The key of the voxel of edge 2^shift times as long that holds this one: floor(k / 2^shift) per axis.
__device__ __forceinline__ u64 map_coarse_key(u64 key, int shift) {
  int kx, ky, kz;
  map_key_axes(key, kx, ky, kz);
  return map_key(kx >> shift, ky >> shift, kz >> shift);
}

// A raw record (revo_map_voxel_raw): key, count, sum q x y z, sum B G R -- eight 64-bit words, moved as four 16-byte words.
struct MapRec {
  ulonglong2 a, b, c, d;  // key n | qx qy | qz sb | sg sr
  __device__ __forceinline__ u64 key() const { return a.x; }
  __device__ __forceinline__ u64 n() const { return a.y; }
};
__device__ __forceinline__ MapRec map_rec_from_slot(const MapVal* val, u64 key) {
  const ulonglong2* v = (const ulonglong2*)val;
  const ulonglong2 p = v[0], q = v[1], c = v[2], d = v[3];  // n qx | qy qz | sb sg | sr -
  return MapRec{make_ulonglong2(key, p.x), make_ulonglong2(p.y, q.x), make_ulonglong2(q.y, c.x), make_ulonglong2(c.y, d.x)};
}
__device__ __forceinline__ MapRec map_rec_from_raw(const ulonglong2* recs, size_t i) {
  const ulonglong2* v = recs + 4 * i;
  return MapRec{v[0], v[1], v[2], v[3]};
}
__device__ __forceinline__ void map_rec_store(ulonglong2* out, size_t j, const MapRec& r) {
  ulonglong2* o = out + 4 * j;
  o[0] = r.a; o[1] = r.b; o[2] = r.c; o[3] = r.d;
}
// a raw record nobody has validated: count 0 or key bit 63 must never reach the table
__device__ __forceinline__ bool map_rec_bad(const MapRec& r) { return (r.a.x >> 63) != 0 || r.a.y == 0; }
// The record's seven sums into (out of) a slot: integer atomics, so no order of records can change the result.
__device__ __forceinline__ void map_rec_add(MapVal* v, const MapRec& r) {
  atomicAdd(&v->n, r.a.y);
  atomicAdd(&v->qx, r.b.x); atomicAdd(&v->qy, r.b.y); atomicAdd(&v->qz, r.c.x);
  atomicAdd(&v->sb, r.c.y); atomicAdd(&v->sg, r.d.x); atomicAdd(&v->sr, r.d.y);
}
__device__ __forceinline__ u64 map_rec_sub(MapVal* v, const MapRec& r) {  // returns the count the slot held before
  const u64 old = atomicAdd(&v->n, 0ull - r.a.y);
  atomicAdd(&v->qx, 0ull - r.b.x); atomicAdd(&v->qy, 0ull - r.b.y); atomicAdd(&v->qz, 0ull - r.c.x);
  atomicAdd(&v->sb, 0ull - r.c.y); atomicAdd(&v->sg, 0ull - r.d.x); atomicAdd(&v->sr, 0ull - r.d.y);
  return old;
}

// A voxel's point is the mean of its fixed-point sums, one axis at a time (n: the count as a double); its colour the rounded
// mean of each channel.  Two packings are in use and stay apart: the extracted cloud's R | G << 8 | B << 16, and the views'
// B | G << 8 | R << 16 (the low word of a z-buffer entry, the ray output).
__device__ __forceinline__ float map_mean(u64 q, double n) { return (float)((double)(long long)q / n * 0x1p-20); }
__device__ __forceinline__ u64 map_channel(u64 s, u64 n) { return (s + n / 2) / n; }
__device__ __forceinline__ unsigned map_colour_rgb(u64 n, u64 sb, u64 sg, u64 sr) {
  return (unsigned)map_channel(sr, n) | ((unsigned)map_channel(sg, n) << 8) | ((unsigned)map_channel(sb, n) << 16);
}
__device__ __forceinline__ u64 map_colour_bgr(u64 n, u64 sb, u64 sg, u64 sr) {
  return map_channel(sb, n) | (map_channel(sg, n) << 8) | (map_channel(sr, n) << 16);
}

// The per-view rule of DESIGN 19, for every unit that classifies a point in a view (revo_map_edit.hip: a voxel's mean;
// revo_map_seen.hip: a cell's centre): one text, so both compile the same arithmetic.
struct MapCarveView {  // one view of a launch, in device memory
  CarveView v;
  const float* depth;
};
enum { CARVE_OUTSIDE = 0, CARVE_UNKNOWN = 1, CARVE_FREE = 2, CARVE_CONFIRMED = 3, CARVE_OCCLUDED = 4, CARVE_EDGE = 5, CARVE_CLASSES = 6 };
#define CARVE_MAX_VIEWS 64

// The class of the point p in one view: the one text of the contract's rule.  Every read of the depth image lies inside a
// window that has been tested against the image size first, and |u|, |v| < 2^20 bounds the integers the test is made on.
// ZD: the camera-space depth z and (for a CONFIRMED point) the centre pixel's depth dc go out as well -- map_carve_class_zd, for
// revo_map_tsdf.hip; without it the two pointers are not looked at and the function is what it was.
// PIX: for a CONFIRMED, OCCLUDED or EDGE point the centre pixel's place iv * w + iu goes out too -- map_carve_class_zdp, for the
// colour of revo_map_tsdf_fuse_color.
template <bool ZD, bool PIX = false>
__device__ __forceinline__ int map_carve_class_t(float px, float py, float pz, const MapCarveView& vw, int r, float margin, float margin_rel,
                                                 float* z_out, float* dc_out, unsigned* pix_out = nullptr) {
  const CarveView& c = vw.v;
  const float x = ((c.Rc[0] * px + c.Rc[1] * py) + c.Rc[2] * pz) + c.tc[0];
  const float y = ((c.Rc[3] * px + c.Rc[4] * py) + c.Rc[5] * pz) + c.tc[1];
  const float z = ((c.Rc[6] * px + c.Rc[7] * py) + c.Rc[8] * pz) + c.tc[2];
  if (ZD) *z_out = z;
  if (!isfinite(x) || !isfinite(y) || !map_depth_ok(z, c.zmin, c.zmax)) return CARVE_OUTSIDE;
  const float u = __fdiv_rn(c.fx * x, z) + c.cx;
  const float v = __fdiv_rn(c.fy * y, z) + c.cy;
  if (!(fabsf(u) < 1048576.0f) || !(fabsf(v) < 1048576.0f)) return CARVE_OUTSIDE;  // NaN / inf fail the comparison
  const int iu = (int)floorf(u + 0.5f), iv = (int)floorf(v + 0.5f);
  if (iu - r < 0 || iu + r > c.w - 1 || iv - r < 0 || iv + r > c.h - 1) return CARVE_OUTSIDE;
  bool usable = true;
  float dmin = INFINITY;
  for (int dy = -r; dy <= r; ++dy) {
    const float* row = vw.depth + (size_t)(iv + dy) * c.w + iu;
    for (int dx = -r; dx <= r; ++dx) {
      const float d = row[dx];
      usable = usable && map_depth_ok(d, c.zmin, c.zmax);
      dmin = fminf(dmin, d);  // only looked at when every depth is usable
    }
  }
  if (!usable) return CARVE_UNKNOWN;
  if (z < dmin - (margin + margin_rel * dmin)) return CARVE_FREE;
  const float dc = vw.depth[(size_t)iv * c.w + iu];
  const float mc = margin + margin_rel * dc;
  if (ZD) *dc_out = dc;
  if (PIX) *pix_out = (unsigned)iv * (unsigned)c.w + (unsigned)iu;
  if (fabsf(z - dc) <= mc) return CARVE_CONFIRMED;
  return z > dc + mc ? CARVE_OCCLUDED : CARVE_EDGE;
}
__device__ __forceinline__ int map_carve_class(float px, float py, float pz, const MapCarveView& vw, int r, float margin, float margin_rel) {
  return map_carve_class_t<false>(px, py, pz, vw, r, margin, margin_rel, nullptr, nullptr);
}
// The same text, and beside the class the depths it was decided on: *z for every class (the camera-space depth), *dc where the
// class is CONFIRMED, OCCLUDED or EDGE (the centre pixel's depth).
__device__ __forceinline__ int map_carve_class_zd(float px, float py, float pz, const MapCarveView& vw, int r, float margin, float margin_rel,
                                                  float* z, float* dc) {
  return map_carve_class_t<true>(px, py, pz, vw, r, margin, margin_rel, z, dc);
}
__device__ __forceinline__ int map_carve_class_zdp(float px, float py, float pz, const MapCarveView& vw, int r, float margin, float margin_rel,
                                                   float* z, float* dc, unsigned* pix) {
  return map_carve_class_t<true, true>(px, py, pz, vw, r, margin, margin_rel, z, dc, pix);
}

// Block compaction in arrival order.  s_n (LDS) is zero behind the kernel's first barrier; every selected thread draws its
// place in the block; behind a barrier thread 0 draws the block's base from `counter` (an unsigned total, or the u64 word of
// an info line) with one global atomic; behind another barrier s_base + place is the thread's output index.  The pair leaves
// the barriers to the kernel (k_map_pose and k_map_carve flush their other counters between the same two); map_compact is
// the whole of it for a kernel with nothing else to flush.
__device__ __forceinline__ unsigned map_compact_begin(bool sel, unsigned& s_n) { return sel ? atomicAdd(&s_n, 1u) : 0u; }
template <typename C>
__device__ __forceinline__ void map_compact_end(unsigned& s_n, unsigned& s_base, C* counter) {
  if (threadIdx.x == 0) s_base = s_n ? (unsigned)atomicAdd(counter, (C)s_n) : 0u;
}
template <typename C>
__device__ __forceinline__ unsigned map_compact(bool sel, unsigned& s_n, unsigned& s_base, C* counter) {
  const unsigned o = map_compact_begin(sel, s_n);
  __syncthreads();
  map_compact_end(s_n, s_base, counter);
  __syncthreads();
  return s_base + o;
}

// ------------------------------------------------------------------------------------------------------- host pieces --
// the argument rules every entry point states the same way
inline int map_check_side(int flag, const char* name) {
  return flag != 0 && flag != 1 ? fail(REVO_ERR_INVALID_ARG, std::string(name) + " must be 0 or 1") : REVO_OK;
}
inline int map_check_aligned(uintptr_t bits, int align, const std::string& what) {  // what: "the device output is", ...
  return bits & (uintptr_t)(align - 1) ? fail(REVO_ERR_INVALID_ARG, what + " not " + std::to_string(align) + "-byte aligned") : REVO_OK;
}

struct MapDesc {  // one keyframe of a launch
  const float* depth; const uint8_t* edges; const uint8_t* bgr;
  float R[9], t[3];  // T_w_kf, R row-major
  float voxel; int dense;
  u64* keys; MapVal* vals; unsigned mask;
  MapStats* st;
};
struct MapCommit {  // one map of a launch
  MapStats* st; u64* pub; u64 max_voxels, seq; int n_kf, check;
};
// The descriptors of an integration or merge launch (a merge has no keyframe rows: nd = 0).  One event guards both sets of
// rows, `com`'s, recorded behind both uploads: a second hipEventRecord per integration would be stream work the launch never
// had.  Callers go through reserve() and upload(), which keep that order; h and d of the two members are theirs to fill.
struct revo_map_stage {
  HostRows<MapDesc> desc;
  HostRows<MapCommit> com;
  int reserve(int nd, int nc, hipStream_t s) { TRY(com.reserve(nc, s)); return desc.reserve(nd, s); }  // com: waits for the event
  int upload(int nd, int nc, hipStream_t s) { if (nd) TRY(desc.upload(nd, s, false)); return com.upload(nc, s); }
};
struct MapViewK;    // revo_map_view.hip: one view of a render launch
// revo_map_raycast's launch records, for revo_map_view.hip, which launches them, and revo_map_gain.hip, which fills views
// of its own on the device.
struct MapRayK {  // what every ray of a launch shares
  const u64* keys; const MapVal* vals; unsigned mask;  // the map's table
  const u64* bkeys; unsigned bmask;                    // the keys of the occupied 8 x 8 x 8 blocks (NULL: every cell is looked up)
  u64 min_count;                                       // >= 1
  unsigned max_steps;
  float voxel;
  u64* info;                                           // one 64-byte line: revo_map_ray_info's counters
};
struct MapRayView {  // one view of a launch, in device memory
  RayView v;
  float* depth; uint8_t* bgr; u64* key; unsigned* hits;  // bgr, key: NULL when not asked for
};
struct MapDfPose;   // revo_map_df_align.hip: one pose of a registration launch
struct TsdfRayView; // revo_map_tsdf_ray.hip: one view of a surface ray cast
struct TsdfTrackPose; // revo_map_tsdf_track.hip: one pose of a surface tracking launch
// revo_map_tsdf_track_eval / revo_map_tsdf_track (revo_map_tsdf_track.hip): the poses of a launch, its tickets, counts and
// published partials, the device copy of a host depth image, and the device records of a host-output call.  Only these two calls go
// through them; a host volume goes through the handle's tsdfvol, which revo_map_tsdf_fuse, _mesh and _raycast use too.
struct MapTsdfTrackScratch {
  HostRows<TsdfTrackPose> poses;
  DevBuf work, frame, out;
};

// revo_map_tsdf_shift / revo_map_tsdf_refill (revo_map_tsdf_follow.hip): the counter line and the block totals of the
// leaving cells, the device copy of a host destination (both volumes) and the device records of a host-side record list.  Only
// these two calls go through them; a host source volume goes through the handle's tsdfvol and tsdfcol.
struct MapTsdfFollowScratch {
  DevBuf work, dst, dstcol, recs;
};

// revo_map_tsdf_fuse_many / revo_map_tsdf_track_eval_many / revo_map_tsdf_track_many / revo_map_tsdf_unfuse_many (revo_map_tsdf_many.hip): the job
// tables of a launch and its pose rows, the fuse's counter lines and tickets, the tracker's tickets, counts and published
// partials, and the device records of a host-output call.  Only these four calls go through them.
struct TsdfManyFuseJob;   // revo_map_tsdf_many.hip: one job of a batched fuse
struct TsdfManyTrackJob;  // ... one job of a batched tracking launch
struct TsdfManyPose;      // ... one pose of it, with its job
struct TsdfManyUnfuseJob; // ... one job of a batched unfuse
struct MapTsdfManyScratch {
  HostRows<TsdfManyFuseJob> fuse_jobs;
  HostRows<TsdfManyTrackJob> track_jobs;
  HostRows<TsdfManyPose> poses;
  DevBuf fuse_work, track_work, out;
  // revo_map_tsdf_unfuse_many: its job table, two counter lines with a ticket each per job (the check pass's and the apply
  // pass's), and the device records of a call with host results
  HostRows<TsdfManyUnfuseJob> unfuse_jobs;
  DevBuf unfuse_work, unfuse_out;
};

// revo_map_tsdf_raycast_many (revo_map_tsdf_ray_many.hip): the job, view and distinct-volume tables of a call, and its
// scratch: the jobs' counter lines and tickets, the views' hit words and the block masks, cleared by one memset.  Only this call
// goes through them.
struct TsdfRayManyJob;   // revo_map_tsdf_ray_many.hip: one job of a batched ray cast
struct TsdfRayManyView;  // ... one view row of it, with its job
struct TsdfRayManyVol;   // ... one distinct volume of its mask launch
struct MapTsdfRayManyScratch {
  HostRows<TsdfRayManyJob> jobs;
  HostRows<TsdfRayManyView> views;
  HostRows<TsdfRayManyVol> vols;
  DevBuf work;
};

struct revo_map {
  revo_ctx* ctx = nullptr;
  MapCtxGeom g{};
  float voxel = 0.f;
  int dense = 0;
  size_t max_voxels = 0;
  u64* d_keys = nullptr; MapVal* d_vals = nullptr; size_t cap = 0;
  MapStats* d_st = nullptr;
  u64* h_pub = nullptr;  // pinned [4]: voxels, sequence of the batch that published them, that batch accepted
  u64 seq = 0;
  std::deque<std::pair<u64, size_t>> pending;  // (sequence, points bound) of batches the host has not seen published
  int rehashes = 0;
  revo_map_stage* stage = nullptr;
  std::vector<std::pair<revo_vo_multi*, int>> attached;
  // revo_map_render: z-buffers of a call's views (every word MAP_EMPTY between calls: the resolve kernel puts it back), the
  // device outputs of a host-output call, the views' descriptors and covered counters, the call's events
  DevBuf zbuf; bool zbuf_clean = false;
  DevBuf vout, cov;
  HostRows<MapViewK> views;
  EventTimer render_time;
  // revo_map_raycast / revo_map_cast_rays: the block table (as many slots as the map's), the counter lines, the views'
  // descriptors, the device outputs of a host-output call, the call's events
  DevBuf bkeys, rcnt, rout;
  HostRows<MapRayView> rviews;
  EventTimer ray_time;
  // revo_map_distance_field / revo_map_bounds (revo_map_field.hip): the bit volume of a call's box, the counter lines, the
  // device field of a host-output call, the call's events
  DevBuf dfbits, dfcnt, dfout;
  EventTimer df_time;
  // revo_map_df_align_eval / revo_map_df_align (revo_map_df_align.hip): the poses of a launch, and its tickets, counts and
  // published partials
  HostRows<MapDfPose> dfa_poses;
  DevBuf dfa_work;
  // revo_map_plan / revo_map_plan_paths (revo_map_plan.hip): the head line and tile flags, the seeds or starts of a call, the
  // device cost field of a host-output call, the pinned words the host reads between rounds behind the event, the call's events
  // and the last round of the last call in which a tile ran
  DevBuf planwork, planseeds, plancost;
  PinnedMem<unsigned> plan_pin;
  OwnedEvent plan_ev;
  EventTimer plan_time;
  uint32_t plan_rounds = 0;
  // revo_map_observe / revo_map_known_field / revo_map_frontiers (revo_map_seen.hip, revo_map_field.hip): the views of a
  // call, its counter lines, and the device copy of a host seen volume (in or out)
  HostRows<MapCarveView> seen_views;
  DevBuf seencnt, seenvol;
  // revo_map_view_gain (revo_map_gain.hip): the predicted depth images of a launch's poses, the poses' descriptors (ray views
  // and gain poses), the counter lines, and the device records of a host-output call
  DevBuf gaindepth, gaindesc, gaincnt, gainout;
  // revo_map_tsdf_fuse / revo_map_tsdf_mesh (revo_map_tsdf.hip): the views of a call, its counter lines, the device copy of a host
  // volume (in or out), and the mesh's scratch: a byte and a word per cell, the block totals, the device outputs of a host call
  HostRows<MapCarveView> tsdf_views;
  DevBuf tsdfcnt, tsdfvol, meshwork, meshout;
  // revo_map_tsdf_fuse_color / revo_map_tsdf_mesh_attr: the views' colour images, the device copy of a host colour volume
  HostRows<const uint8_t*> tsdf_bgr;
  DevBuf tsdfcol;
  // revo_map_tsdf_raycast (revo_map_tsdf_ray.hip): the counter lines and the block mask, the views' descriptors, the device outputs
  // of a host-output call; a host volume goes through tsdfvol and tsdfcol
  DevBuf tsdfraywork, tsdfrayout;
  HostRows<TsdfRayView> tsdfray_views;
  // revo_map_tsdf_track_eval / revo_map_tsdf_track: everything of theirs, in a type of its own
  MapTsdfTrackScratch tsdftrk;
  // revo_map_tsdf_shift / revo_map_tsdf_refill: everything of theirs, in a type of its own
  MapTsdfFollowScratch tsdffol;
  // revo_map_tsdf_fuse_many / revo_map_tsdf_track_eval_many / revo_map_tsdf_track_many: everything of theirs, in a type of its own
  MapTsdfManyScratch tsdfmany;
  // revo_map_tsdf_raycast_many: everything of the call, in a type of its own
  MapTsdfRayManyScratch tsdfraymany;
};

// The views of a carve or an observe call, checked and resolved in the order DESIGN 19 states: each view's own rules, then every
// pyramid's context and kind before any of them orders a stream, then the pyramids' depth planes (the tracker stream is
// ordered behind their builds; nothing is refused from there on).  hv[i].depth stays the caller's pointer for a raw image;
// *up_bytes: what the call's host images need in one upload, each rounded up to 256 bytes.
// bgr (revo_map_tsdf_fuse_color): where a pyramid view's level-0 colour plane goes, the other entries are left alone.
inline int map_views_prepare(revo_map* m, int n, const revo_map_carve_view* views, int device_in, MapCarveView* hv, size_t* up_bytes,
                             const uint8_t** bgr = nullptr) {
  const CarveCam cam{m->g.fx, m->g.fy, m->g.cx, m->g.cy, m->g.dmin, m->g.dmax};
  *up_bytes = 0;
  for (int i = 0; i < n; ++i) {
    const std::string at = "view " + std::to_string(i) + ": ";
    if (const char* why = carve_view_check(&views[i], cam, m->g.w, m->g.h, &hv[i].v)) return fail(REVO_ERR_INVALID_ARG, at + why);
    hv[i].depth = views[i].depth;
    if (views[i].depth) {
      if (device_in) TRY(map_check_aligned((uintptr_t)views[i].depth, 4, at + "the device depth image is"));
      if (!device_in) *up_bytes += ((size_t)hv[i].v.w * hv[i].v.h * sizeof(float) + 255) & ~(size_t)255;
    }
  }
  for (int i = 0; i < n; ++i) {
    if (!views[i].kf) continue;
    const revo_ctx* pc = nullptr;
    int batch_view = 0;
    TRY(revo_map_source_kind_(views[i].kf, &pc, &batch_view));
    const std::string at = "view " + std::to_string(i) + ": ";
    if (pc != m->ctx) return fail(REVO_ERR_INVALID_ARG, at + "the pyramid belongs to another context than the map");
    if (batch_view)
      return fail(REVO_ERR_INVALID_ARG, at + "a batch view is not a keyframe the map calls take (pass its depth plane as a raw image)");
  }
  for (int i = 0; i < n; ++i) {
    if (!views[i].kf) continue;
    MapSource src;
    TRY(revo_map_source_(const_cast<revo_pyr*>(views[i].kf), &src));
    hv[i].depth = src.depth;
    if (bgr) bgr[i] = src.bgr;
  }
  return REVO_OK;
}
// The host images of the call into `images` (room for up_bytes) on stream s; hv[i].depth then names the device copy.
inline int map_views_upload(int n, const revo_map_carve_view* views, MapCarveView* hv, char* images, hipStream_t s) {
  size_t o = 0;
  for (int i = 0; i < n; ++i) {
    if (!views[i].depth) continue;
    const size_t bytes = (size_t)hv[i].v.w * hv[i].v.h * sizeof(float);
    HIPCHECK(hipMemcpyAsync(images + o, views[i].depth, bytes, hipMemcpyHostToDevice, s));
    hv[i].depth = (const float*)(images + o);
    o += (bytes + 255) & ~(size_t)255;
  }
  return REVO_OK;
}

// revo_map.hip, for the other units.  map_read_stats waits for the map's stream; map_grow(live_only) is the compaction an
// accepted subtraction ends with; map_merge_core / map_subtract_core: one merge into (subtraction from) m of the input `a` names.
size_t map_occ_bound(revo_map* m);
int map_grow(revo_map* m, size_t newcap, bool live_only = false);
int map_read_stats(revo_map* m, MapStats* out);
int map_merge_core(revo_map* m, MapMergeK a, int src_kind, size_t bound, bool trusted, int keyframes);
int map_subtract_core(revo_map* m, MapMergeK a, int src_kind, u64 dropped, u64 keyframes);

// revo_map_field.hip, for revo_map_seen.hip: the box rules of DESIGN 21 (NULL if the box keeps them; *cells: its cells), and the
// bit volume of the box's solid voxels (z-major, wz 32-bit words per z-line) enqueued on stream s into m->dfbits, with
// k_df_occupancy's counters in `info` (NULL: m->dfcnt's line).
const char* map_df_box_check(const revo_map_df_box* box, size_t* cells);
int map_df_solid_bits(revo_map* m, const revo_map_df_box* box, uint32_t min_count, hipStream_t s, const unsigned** bits, unsigned* wz, u64* info = nullptr);

// revo_map_tsdf.hip, for revo_map_tsdf_unfuse.hip: the views of a TSDF call (revo_map_tsdf_fuse[_color], revo_map_tsdf_unfuse) on
// the device, behind the call's own argument checks.  bgr: the views' colour images, NULL for a call without colour; who: the
// entry point's prefix for the messages; cells: the box's.  In stream order: the reserves of the handle's rows, counter lines and
// host-volume copies (the rows' wait until the previous call's upload has read the pinned rows), one upload of the host images
// -- depth images, then colour images, each rounded up to 256 bytes --, then the view rows and the colour row.  The caller's
// copies, memsets and launch follow.
struct MapTsdfViews {
  DevScratch images;  // the host images of the call, uploaded; freed with this record, behind the caller's last wait
  const MapCarveView* views = nullptr;
  const uint8_t* const* bgr = nullptr;  // one pointer per view; NULL without colour
  bool uploaded = false;                // host images were: the caller waits for the stream before it returns
};
int map_tsdf_views_begin(revo_map* m, const std::string& who, size_t cells, int n, const revo_map_carve_view* views, const uint8_t* const* bgr,
                         int device_in, int device_tsdf, MapTsdfViews* out);

// revo_map_view.hip, for revo_map_gain.hip: revo_map_raycast's march over views that are in device memory already.  map_ray_open
// reserves and builds the block table of the map as it is on the stream, clears the info line d_info and fills *a;
// map_ray_views enqueues k_map_raycast over n (1 .. 64) views whose largest image takes max_blocks blocks.
int map_ray_open(revo_map* m, MapRayK* a, uint32_t min_count, uint32_t max_steps, u64* d_info);
int map_ray_views(revo_map* m, const MapRayK& a, int n, const MapRayView* d_views, int max_blocks);

// Room in m's table for `bound` more keys at a load <= 0.5 (the checked path inserts every new key before it decides: what
// the map may hold + all of them); *ub: the bound of the voxels it holds now.  what: "batch", "merge".
inline int map_need_slots(revo_map* m, size_t bound, const char* what, size_t* ub) {
  *ub = map_occ_bound(m);
  const size_t need = 2 * (std::min(*ub, m->max_voxels) + bound);
  if (need > MAP_MAX_CAP) return fail(REVO_ERR_CAPACITY, std::string("voxel map: a ") + what + " this large needs more than 2^31 table slots");
  if (m->cap >= need) return REVO_OK;
  size_t c = std::max<size_t>(m->cap * 2, 1024);
  while (c < need) c *= 2;
  return map_grow(m, c);
}
