// revo_map.hip -- world-frame voxel map fused on the device from keyframe clouds (revo_map_* in include/revo_hip.h).
//
// The reference draws every keyframe's coloured cloud at its keyframe pose (gui/MapDrawer.cc, fed by system.cpp:162-168,
// 232-238).  Here each keyframe is integrated straight from its level-0 planes into an open-addressing hash of voxels:
//   * keys: the voxel index packed into 63 bits ((kx + 2^20) << 42 | (ky + 2^20) << 21 | (kz + 2^20)), inserted by a 64-bit
//     CAS, linear probing from a mixed hash, table size a power of two at a load factor <= 0.5;
//   * values: count, the three 2^-20 m fixed-point coordinate sums (int64) and the three colour sums (u64), 64 B per slot,
//     updated by integer atomics only -- the sums are exact, so no launch order, batching or combining can change them;
//   * a wave first sums runs of equal keys among its 64 adjacent pixels (segmented shuffle reduction): in dense mode at small
//     voxels most neighbours share a voxel, and one lane per run does the atomics.
// Capacity: the host keeps an upper bound of the voxels (the last count the device published into pinned memory plus the
// points of every integration since), grows the table before an integration could pass a load of 0.5 (one rehash kernel into
// a table of the next power of two that fits), and only when the bound could pass max_voxels does it take the checked path:
// insert the keys, decide on the device (count <= max_voxels), take the new keys out again if refused, then accumulate.
// All of it runs on the context's tracker stream, behind the keyframe's build (revo_map_source_).
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
#include "revo_track_dev.h"
#include "revo_align_host.h"
#include "revo_pose_host.h"
#include "revo_carve_host.h"
#include "revo_ray_host.h"

#define MAP_EMPTY 0xffffffffffffffffull  // no packed key reaches bit 63
#define MAP_SHARDS 16                    // per-map batch counters, one 128-B line each (one global atomic per block and counter)
#define MAP_MAX_CAP (1ull << 31)
#define MAP_MAX_VOXELS (1ull << 28)

typedef unsigned long long u64;

struct MapVal { u64 n, qx, qy, qz, sb, sg, sr, pad; };  // count, sum q (two's complement int64), sum B, G, R
struct MapStats {
  u64 occ, pts, drop, kfs, rejected, fault;
  u64 ok, bad;  // bad: k_map_merge met a record with count 0 or key bit 63 (the host clears it before such a launch)
  u64 shard[MAP_SHARDS][16];  // [0] new voxels, [1] points, [2] dropped points of the batch in flight
  // the subtraction in flight (behind the shards: no older field moves): refused, points taken, voxels whose count reached 0
  u64 sub_bad, sub_pts, sub_freed;
};
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
struct MapGeomK { int w, npix; float fx, fy, cx, cy, dmin, dmax; };
enum { MAP_FUSED = 0, MAP_INSERT = 1, MAP_ACCUM = 2 };

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

// One thread per level-0 pixel of each keyframe (blockIdx.x / nb = keyframe): the selection of k_pcl_walk (dense || edge,
// usable depth), its back-projection, the world point, key and fixed point; then per wave a segmented sum over runs of equal
// keys and one lane per run updates the voxel.
template <int MODE>
__global__ void __launch_bounds__(256) k_map_walk(const MapDesc* __restrict__ descs, int nb, MapGeomK g) {
  __shared__ unsigned s_cnt[3];
  const int di = blockIdx.x / nb;
  const MapDesc& d = descs[di];
  if (MODE == MAP_ACCUM && !d.st->ok) return;  // refused: nothing of this map's batch is accumulated
  if (MODE != MAP_ACCUM) {
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    __syncthreads();
  }
  const int p = (blockIdx.x - di * nb) * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  u64 key = MAP_EMPTY;
  long long qx = 0, qy = 0, qz = 0;
  unsigned n = 0, cb = 0, cg = 0, cr = 0;
  bool dropped = false;
  if (p < g.npix) {
    const float Z = d.depth[p];
    if ((d.dense || d.edges[p]) && map_depth_ok(Z, g.dmin, g.dmax)) {
      const int x = p % g.w, y = p / g.w;
      const float X = __fdiv_rn(Z * ((float)x - g.cx), g.fx);  // k_pcl_walk<true>
      const float Y = __fdiv_rn(Z * ((float)y - g.cy), g.fy);
      float pw[3];
      int k[3];
      bool ok = true;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        pw[i] = ((d.R[3 * i] * X + d.R[3 * i + 1] * Y) + d.R[3 * i + 2] * Z) + d.t[i];
        const float f = floorf(__fdiv_rn(pw[i], d.voxel));
        ok = ok && fabsf(pw[i]) < 2048.0f && f >= -1048576.0f && f <= 1048575.0f;  // NaN / inf fail every comparison
        k[i] = ok ? (int)f : 0;
      }
      if (ok) {
        key = ((u64)(k[0] + (1 << 20)) << 42) | ((u64)(k[1] + (1 << 20)) << 21) | (u64)(k[2] + (1 << 20));
        qx = (long long)rintf(pw[0] * 1048576.0f);  // exact product; rint = llrintf's round-to-nearest-even
        qy = (long long)rintf(pw[1] * 1048576.0f);
        qz = (long long)rintf(pw[2] * 1048576.0f);
        const uint8_t* px = d.bgr + (size_t)p * 3;
        cb = px[0]; cg = px[1]; cr = px[2];
        n = 1;
      } else {
        dropped = true;
      }
    }
  }
  // runs of equal keys inside the wave: run id = number of run heads up to this lane; suffix sums restricted to the run
  const u64 kup = __shfl_up((unsigned long long)key, 1, 64);
  const bool head = lane == 0 || kup != key;
  const u64 hb = __ballot(head);
  const int rid = __popcll(lane == 63 ? hb : (hb & ((2ull << lane) - 1ull)));
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int ro = __shfl_down(rid, off, 64);
    const long long ax = __shfl_down(qx, off, 64), ay = __shfl_down(qy, off, 64), az = __shfl_down(qz, off, 64);
    const unsigned an = __shfl_down(n, off, 64), ab = __shfl_down(cb, off, 64), ag = __shfl_down(cg, off, 64),
                   ar = __shfl_down(cr, off, 64);
    if (lane + off < 64 && ro == rid) { qx += ax; qy += ay; qz += az; n += an; cb += ab; cg += ag; cr += ar; }
  }
  if (head && key != MAP_EMPTY) {
    const unsigned s = MODE == MAP_ACCUM ? map_slot<false>(d.keys, d.mask, key, nullptr, &d.st->fault)
                                         : map_slot<true>(d.keys, d.mask, key, &s_cnt[0], &d.st->fault);
    if (MODE != MAP_INSERT && s != ~0u) {
      MapVal* v = d.vals + s;
      atomicAdd(&v->n, (u64)n);
      atomicAdd(&v->qx, (u64)qx); atomicAdd(&v->qy, (u64)qy); atomicAdd(&v->qz, (u64)qz);
      atomicAdd(&v->sb, (u64)cb); atomicAdd(&v->sg, (u64)cg); atomicAdd(&v->sr, (u64)cr);
    }
    if (MODE != MAP_ACCUM) atomicAdd(&s_cnt[1], n);
  }
  if (MODE != MAP_ACCUM) {
    if (dropped) atomicAdd(&s_cnt[2], 1u);
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&d.st->shard[blockIdx.x & (MAP_SHARDS - 1)][threadIdx.x], (u64)s_cnt[threadIdx.x]);
  }
}

// One thread per map of the launch: fold the batch counters, decide (checked path: the new voxel count against max_voxels),
// publish the voxel count to the host (pinned memory, read as a lagged upper bound for the growth check).
__global__ void __launch_bounds__(64) k_map_commit(const MapCommit* __restrict__ cm, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const MapCommit c = cm[i];
  MapStats* s = c.st;
  u64 nw = 0, np = 0, nd = 0;
  for (int k = 0; k < MAP_SHARDS; ++k) {
    nw += s->shard[k][0]; np += s->shard[k][1]; nd += s->shard[k][2];
    s->shard[k][0] = 0; s->shard[k][1] = 0; s->shard[k][2] = 0;
  }
  const bool ok = !c.check || s->occ + nw <= c.max_voxels;
  s->ok = ok ? 1 : 0;
  if (ok) { s->occ += nw; s->pts += np; s->drop += nd; s->kfs += (u64)c.n_kf; }
  else s->rejected += (u64)c.n_kf;
  c.pub[0] = s->occ;
  c.pub[2] = ok ? 1 : 0;
  __threadfence_system();
  *(volatile u64*)&c.pub[1] = c.seq;  // the host reads the sequence word first
}

// Refused batch: its keys are exactly the occupied slots with count 0 (a committed voxel has count >= 1).  Taking them out
// restores the table as it was -- every older key's probe path only crosses keys older than itself.
__global__ void __launch_bounds__(256) k_map_rollback(u64* keys, const MapVal* vals, unsigned cap, const MapStats* st) {
  if (st->ok) return;
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i < cap && keys[i] != MAP_EMPTY && vals[i].n == 0) keys[i] = MAP_EMPTY;
}

__global__ void __launch_bounds__(256) k_map_rehash(const u64* __restrict__ okeys, const MapVal* __restrict__ ovals, unsigned ocap,
                                                    u64* nkeys, MapVal* nvals, unsigned nmask, u64* fault) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ocap) return;
  const u64 key = okeys[i];
  if (key == MAP_EMPTY) return;
  const unsigned s = map_slot<true>(nkeys, nmask, key, nullptr, fault);
  if (s != ~0u) nvals[s] = ovals[i];
}

// Occupied slots with count >= min_count, compacted in arrival order (the host sorts by key): key, xyz, packed RGB, count.
__global__ void __launch_bounds__(256) k_map_extract(const u64* __restrict__ keys, const MapVal* __restrict__ vals, unsigned cap,
                                                     u64 min_count, unsigned* total, u64* okey, float* oxyz, unsigned* orgb,
                                                     unsigned* ocount) {
  __shared__ unsigned s_n, s_base;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  const u64 key = i < cap ? keys[i] : MAP_EMPTY;
  MapVal v{};
  bool sel = false;
  if (key != MAP_EMPTY) { v = vals[i]; sel = v.n >= min_count; }
  const unsigned o = sel ? atomicAdd(&s_n, 1u) : 0u;
  __syncthreads();
  if (threadIdx.x == 0) s_base = s_n ? atomicAdd(total, s_n) : 0u;
  __syncthreads();
  if (!sel) return;
  const unsigned j = s_base + o;
  const double inv = (double)v.n;
  okey[j] = key;
  oxyz[3 * j + 0] = (float)((double)(long long)v.qx / inv * 0x1p-20);
  oxyz[3 * j + 1] = (float)((double)(long long)v.qy / inv * 0x1p-20);
  oxyz[3 * j + 2] = (float)((double)(long long)v.qz / inv * 0x1p-20);
  const u64 h = v.n / 2;
  orgb[j] = (unsigned)((v.sr + h) / v.n) | ((unsigned)((v.sg + h) / v.n) << 8) | ((unsigned)((v.sb + h) / v.n) << 16);
  ocount[j] = (unsigned)v.n;
}

// ------------------------------------------------------------------------------------------------- the map as data (13) --
// A raw record (revo_map_voxel_raw) is key, count, sum q x y z, sum B G R: eight 64-bit words, moved as four 16-byte words.
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

// The key of the voxel of edge 2^shift times as long that holds this one: floor(k / 2^shift) per axis on the unbiased index.
__device__ __forceinline__ u64 map_coarse_key(u64 key, int shift) {
  const int kx = (int)((key >> 42) & 0x1fffffu) - (1 << 20), ky = (int)((key >> 21) & 0x1fffffu) - (1 << 20),
            kz = (int)(key & 0x1fffffu) - (1 << 20);
  return ((u64)((kx >> shift) + (1 << 20)) << 42) | ((u64)((ky >> shift) + (1 << 20)) << 21) | (u64)((kz >> shift) + (1 << 20));
}
#define MAP_POISON (1ull << 40)  // > MAP_MAX_VOXELS: a batch whose new-voxel count holds it is refused by k_map_commit

// Occupied slots as raw records, compacted in arrival order (the host sorts by key); at most cap_out are written.
__global__ void __launch_bounds__(256) k_map_export(const u64* __restrict__ keys, const MapVal* __restrict__ vals, unsigned cap,
                                                    unsigned* total, ulonglong2* out, unsigned cap_out) {
  __shared__ unsigned s_n, s_base;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  const u64 key = i < cap ? keys[i] : MAP_EMPTY;
  const bool sel = key != MAP_EMPTY;
  const unsigned o = sel ? atomicAdd(&s_n, 1u) : 0u;
  __syncthreads();
  if (threadIdx.x == 0) s_base = s_n ? atomicAdd(total, s_n) : 0u;
  __syncthreads();
  if (!sel) return;
  const unsigned j = s_base + o;
  if (j >= cap_out) return;
  const ulonglong2* v = (const ulonglong2*)(vals + i);
  const ulonglong2 a = v[0], b = v[1], c = v[2], d = v[3];  // n qx | qy qz | sb sg | sr -
  ulonglong2* r = out + 4 * (size_t)j;
  r[0] = make_ulonglong2(key, a.x); r[1] = make_ulonglong2(a.y, b.x); r[2] = make_ulonglong2(b.y, c.x); r[3] = make_ulonglong2(c.y, d.x);
}

// One thread per input record (MERGE_RAW) or per slot of the source table (MERGE_TABLE): the voxel's sums are added to the
// slot of its key as k_map_walk adds a run's, in the same three modes, and the block's new voxels and points go through LDS
// to the map's sharded counters.  A record with count 0 or key bit 63 is never inserted (the rollback invariant is "a new
// key's slot has count 0"); the first one met poisons the batch's new-voxel count, so k_map_commit refuses the batch, and
// sets st->bad, so the host can tell why.  Only the checked path (MAP_INSERT) takes records that nobody has validated.
template <int MODE, int SRC>
__global__ void __launch_bounds__(256) k_map_merge(const MapMergeK a) {
  __shared__ unsigned s_new;
  __shared__ u64 s_pts;
  if (MODE == MAP_ACCUM && !a.st->ok) return;  // refused: nothing is accumulated
  if (MODE != MAP_ACCUM) {
    if (threadIdx.x == 0) { s_new = 0; s_pts = 0; }
    __syncthreads();
  }
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  u64 key = MAP_EMPTY;
  ulonglong2 r0{}, r1{}, r2{}, r3{};  // key n | qx qy | qz sb | sg sr
  bool bad = false;
  if (i < a.n) {
    if (SRC != MERGE_RAW) {
      key = a.skeys[i];
      if (key != MAP_EMPTY) {
        const ulonglong2* v = (const ulonglong2*)(a.svals + i);
        const ulonglong2 p = v[0], q = v[1], c = v[2], d = v[3];
        if (SRC == MERGE_COARSE) key = map_coarse_key(key, a.shift);
        r0 = make_ulonglong2(key, p.x); r1 = make_ulonglong2(p.y, q.x); r2 = make_ulonglong2(q.y, c.x); r3 = make_ulonglong2(c.y, d.x);
        if (r0.y == 0) key = MAP_EMPTY;  // a committed voxel has count >= 1
      }
    } else {
      const ulonglong2* v = a.recs + 4 * (size_t)i;
      r0 = v[0]; r1 = v[1]; r2 = v[2]; r3 = v[3];
      key = r0.x;
      bad = (key >> 63) != 0 || r0.y == 0;
      if (bad) key = MAP_EMPTY;
    }
  }
  if (key != MAP_EMPTY) {
    const unsigned s = MODE == MAP_ACCUM ? map_slot<false>(a.keys, a.mask, key, nullptr, &a.st->fault)
                                         : map_slot<true>(a.keys, a.mask, key, &s_new, &a.st->fault);
    if (MODE != MAP_INSERT && s != ~0u) {
      MapVal* v = a.vals + s;
      atomicAdd(&v->n, r0.y);
      atomicAdd(&v->qx, r1.x); atomicAdd(&v->qy, r1.y); atomicAdd(&v->qz, r2.x);
      atomicAdd(&v->sb, r2.y); atomicAdd(&v->sg, r3.x); atomicAdd(&v->sr, r3.y);
    }
    if (MODE != MAP_ACCUM) atomicAdd(&s_pts, r0.y);
  }
  if (MODE != MAP_ACCUM) {
    if (SRC == MERGE_RAW && bad && atomicOr(&a.st->bad, 1ull) == 0) atomicAdd(&a.st->shard[0][0], MAP_POISON);
    __syncthreads();
    if (threadIdx.x == 0) {
      u64* sh = a.st->shard[blockIdx.x & (MAP_SHARDS - 1)];
      if (s_new) atomicAdd(&sh[0], (u64)s_new);
      if (s_pts) atomicAdd(&sh[1], s_pts);
      if (blockIdx.x == 0 && a.dropped) atomicAdd(&sh[2], a.dropped);
    }
  }
}

// --------------------------------------------------------------------------------------- taking voxels out again (15) --
// revo_map_subtract_raw / revo_map_subtract: the inverse of k_map_merge.  Four launches and a decision between them:
//   k_map_sub<SRC, false>  every record's sums leave the slot of its key (looked up, never inserted);
//   k_map_sub_verify<SRC>  a slot left with count 0 must have every other sum 0;
//   k_map_sub_commit       decides, moves the counters, publishes as k_map_commit does;
//   k_map_sub<SRC, true>   refused: the same records are added back -- integer addition restores the table exactly;
//   k_map_rehash_live      accepted and voxels died: the live slots go into a fresh table of the same size (host: compact()).
struct MapSubCommit { MapStats* st; u64* pub; u64 seq, dropped, kfs; };

// The slot of `key`, or ~0u: a lookup that touches nothing (a miss is the caller's bad record, not a broken table).  No key
// of the table changes while a subtraction's passes run, so plain loads do.
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

// One thread per input record (MERGE_RAW) or per slot of the source table (MERGE_TABLE), loaded as k_map_merge loads them.
// The count's atomic returns what the voxel held before this record: less than the record takes means the voxel's records
// together take more than it has (the first record to cross zero always sees it, whatever the order); exactly as much means
// this record emptied it, and nothing may follow, so those are the freed voxels.  Block sums go through LDS.
template <int SRC, bool UNDO>
__global__ void __launch_bounds__(256) k_map_sub(const MapMergeK a) {
  __shared__ unsigned s_freed, s_bad;
  __shared__ u64 s_pts;
  if (UNDO && a.st->ok) return;  // accepted: nothing to put back
  if (!UNDO) {
    if (threadIdx.x == 0) { s_freed = 0; s_bad = 0; s_pts = 0; }
    __syncthreads();
  }
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  u64 key = MAP_EMPTY;
  ulonglong2 r0{}, r1{}, r2{}, r3{};  // key n | qx qy | qz sb | sg sr
  bool bad = false;
  if (i < a.n) {
    if (SRC == MERGE_TABLE) {
      key = a.skeys[i];
      if (key != MAP_EMPTY) {
        const ulonglong2* v = (const ulonglong2*)(a.svals + i);
        const ulonglong2 p = v[0], q = v[1], c = v[2], d = v[3];
        r0 = make_ulonglong2(key, p.x); r1 = make_ulonglong2(p.y, q.x); r2 = make_ulonglong2(q.y, c.x); r3 = make_ulonglong2(c.y, d.x);
        if (r0.y == 0) key = MAP_EMPTY;  // a committed voxel has count >= 1
      }
    } else {
      const ulonglong2* v = a.recs + 4 * (size_t)i;
      r0 = v[0]; r1 = v[1]; r2 = v[2]; r3 = v[3];
      key = r0.x;
      bad = (key >> 63) != 0 || r0.y == 0;
      if (bad) key = MAP_EMPTY;
    }
  }
  if (key != MAP_EMPTY) {
    const unsigned s = map_find(a.keys, a.mask, key);
    if (s == ~0u) {
      bad = true;
    } else {
      MapVal* v = a.vals + s;
      if (UNDO) {
        atomicAdd(&v->n, r0.y);
        atomicAdd(&v->qx, r1.x); atomicAdd(&v->qy, r1.y); atomicAdd(&v->qz, r2.x);
        atomicAdd(&v->sb, r2.y); atomicAdd(&v->sg, r3.x); atomicAdd(&v->sr, r3.y);
      } else {
        const u64 old = atomicAdd(&v->n, 0ull - r0.y);
        atomicAdd(&v->qx, 0ull - r1.x); atomicAdd(&v->qy, 0ull - r1.y); atomicAdd(&v->qz, 0ull - r2.x);
        atomicAdd(&v->sb, 0ull - r2.y); atomicAdd(&v->sg, 0ull - r3.x); atomicAdd(&v->sr, 0ull - r3.y);
        if (old < r0.y) bad = true;
        else if (old == r0.y) atomicAdd(&s_freed, 1u);
        atomicAdd(&s_pts, r0.y);
      }
    }
  }
  if (!UNDO) {
    if (bad) atomicOr(&s_bad, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
      if (s_bad) atomicOr(&a.st->sub_bad, 1ull);
      if (s_pts) atomicAdd(&a.st->sub_pts, s_pts);
      if (s_freed) atomicAdd(&a.st->sub_freed, (u64)s_freed);
    }
  }
}

// One thread per record or source slot again, behind every subtraction: the slot of its key, and if the count there is 0,
// the other six sums.  (Several records of one voxel check the same slot; a refusal is a flag, so that costs nothing.)
template <int SRC>
__global__ void __launch_bounds__(256) k_map_sub_verify(const MapMergeK a) {
  __shared__ unsigned s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  u64 key = MAP_EMPTY;
  if (i < a.n) {
    if (SRC == MERGE_TABLE) {
      key = a.skeys[i];
      if (key != MAP_EMPTY && a.svals[i].n == 0) key = MAP_EMPTY;
    } else {
      const ulonglong2 r0 = a.recs[4 * (size_t)i];
      key = r0.x;
      if ((key >> 63) != 0 || r0.y == 0) key = MAP_EMPTY;
    }
  }
  if (key != MAP_EMPTY) {
    const unsigned s = map_find(a.keys, a.mask, key);
    if (s != ~0u) {
      const ulonglong2* v = (const ulonglong2*)(a.vals + s);
      const ulonglong2 p = v[0];
      if (p.x == 0) {
        const ulonglong2 q = v[1], c = v[2], d = v[3];
        if (p.y | q.x | q.y | c.x | c.y | d.x) atomicOr(&s_bad, 1u);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_bad) atomicOr(&a.st->sub_bad, 1ull);
}

// One thread: the decision of a subtraction, its counters, and the publication of k_map_commit (voxels, accepted, the
// sequence word last) with the freed voxels in the fourth pinned word for the host, which then drops the dead slots.
__global__ void __launch_bounds__(64) k_map_sub_commit(const MapSubCommit c) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  MapStats* s = c.st;
  const u64 pts = s->sub_pts, freed = s->sub_freed;
  const bool ok = !s->sub_bad && pts <= s->pts && freed <= s->occ && c.dropped <= s->drop && c.kfs <= s->kfs;
  s->ok = ok ? 1 : 0;
  if (ok) { s->occ -= freed; s->pts -= pts; s->drop -= c.dropped; s->kfs -= c.kfs; }
  c.pub[0] = s->occ;
  c.pub[2] = ok ? 1 : 0;
  c.pub[3] = ok ? freed : 0;
  __threadfence_system();
  *(volatile u64*)&c.pub[1] = c.seq;
}

// An accepted subtraction that cannot get its fresh table is taken back: the counters here, the sums by k_map_sub<.., true>.
__global__ void __launch_bounds__(64) k_map_sub_revert(const MapSubCommit c) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  MapStats* s = c.st;
  if (!s->ok) return;
  s->occ += s->sub_freed; s->pts += s->sub_pts; s->drop += c.dropped; s->kfs += c.kfs;
  s->ok = 0;
  c.pub[0] = s->occ;
  c.pub[2] = 0;
  c.pub[3] = 0;
  __threadfence_system();
  *(volatile u64*)&c.pub[1] = c.seq;
}

// k_map_rehash that leaves the slots with count 0 behind: the new table holds the live voxels only, each reachable from its
// hash through occupied slots (it was inserted there), so it is a table no kernel can tell from one that never held the rest.
__global__ void __launch_bounds__(256) k_map_rehash_live(const u64* __restrict__ okeys, const MapVal* __restrict__ ovals, unsigned ocap,
                                                         u64* nkeys, MapVal* nvals, unsigned nmask, u64* fault) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ocap) return;
  const u64 key = okeys[i];
  if (key == MAP_EMPTY) return;
  const ulonglong2* v = (const ulonglong2*)(ovals + i);
  const ulonglong2 p = v[0];
  if (p.x == 0) return;
  const ulonglong2 q = v[1], c = v[2], d = v[3];
  const unsigned s = map_slot<true>(nkeys, nmask, key, nullptr, fault);
  if (s == ~0u) return;
  ulonglong2* o = (ulonglong2*)(nvals + s);
  o[0] = p; o[1] = q; o[2] = c; o[3] = d;
}

// ---------------------------------------------------------------------------------------------------------------- views --
// revo_map_render (contract: include/revo_hip.h).  A z-buffer word is (bits of z) << 32 | R << 16 | G << 8 | B; an
// untouched pixel holds MAP_EMPTY (z is finite and > 0, so no written word reaches it).  A pixel keeps the minimum word.
struct MapViewK {  // one view of a launch
  float Rc[9], tc[3];  // world -> camera, Rc row-major
  float fx, fy, cx, cy, zmin, zmax;
  float hv;            // 0.5f * voxel
  int w, h, splat;
  u64 min_count;
  u64* zbuf;
  float* depth; uint8_t* bgr; unsigned* covered;
};

// One thread per table slot and view (blockIdx.y = view): the voxel's point and colour as k_map_extract forms them, its
// projection, and one 64-bit atomicMin per footprint pixel.  SKIP: a load of the pixel first; the word stored there only ever
// decreases during the launch, so a stored word <= this one (however stale) means the atomic could not change it.
template <bool SKIP>
__global__ void __launch_bounds__(256) k_map_splat(const u64* __restrict__ keys, const MapVal* __restrict__ vals, unsigned cap,
                                                   const MapViewK* __restrict__ views) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cap || keys[i] == MAP_EMPTY) return;
  const MapViewK& vw = views[blockIdx.y];
  const MapVal v = vals[i];
  if (v.n < vw.min_count) return;
  const double inv = (double)v.n;
  const float px = (float)((double)(long long)v.qx / inv * 0x1p-20);
  const float py = (float)((double)(long long)v.qy / inv * 0x1p-20);
  const float pz = (float)((double)(long long)v.qz / inv * 0x1p-20);
  float pc[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) pc[k] = ((vw.Rc[3 * k] * px + vw.Rc[3 * k + 1] * py) + vw.Rc[3 * k + 2] * pz) + vw.tc[k];
  const float z = pc[2];
  if (!isfinite(pc[0]) || !isfinite(pc[1]) || !map_depth_ok(z, vw.zmin, vw.zmax)) return;
  const float u = __fdiv_rn(vw.fx * pc[0], z) + vw.cx;  // tracker.cpp:153-156
  const float w = __fdiv_rn(vw.fy * pc[1], z) + vw.cy;
  if (!(fabsf(u) < 1048576.0f) || !(fabsf(w) < 1048576.0f)) return;  // NaN / inf fail the comparison
  const int iu = (int)floorf(u), iv = (int)floorf(w);
  const int ru = (int)fminf((float)vw.splat, ceilf(__fdiv_rn(vw.hv * vw.fx, z)));
  const int rv = (int)fminf((float)vw.splat, ceilf(__fdiv_rn(vw.hv * vw.fy, z)));
  const int x0 = max(iu - ru, 0), x1 = min(iu + ru, vw.w - 1), y0 = max(iv - rv, 0), y1 = min(iv + rv, vw.h - 1);
  const u64 h = v.n / 2;
  const u64 word = ((u64)__float_as_uint(z) << 32) | (((v.sr + h) / v.n) << 16) | (((v.sg + h) / v.n) << 8) | ((v.sb + h) / v.n);
  for (int y = y0; y <= y1; ++y) {
    u64* row = vw.zbuf + (size_t)y * vw.w;
    for (int x = x0; x <= x1; ++x) {
      if (SKIP && __hip_atomic_load(&row[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= word) continue;
      atomicMin(&row[x], word);
    }
  }
}

// One thread per pixel and view: z-buffer word -> depth / BGR, the word goes back to MAP_EMPTY for the next call, and the
// written pixels are counted per block in LDS, then one atomic per block.
__global__ void __launch_bounds__(256) k_map_view_resolve(const MapViewK* __restrict__ views) {
  __shared__ unsigned s_n;
  const MapViewK& vw = views[blockIdx.y];
  const unsigned npix = (unsigned)(vw.w * vw.h);
  if (blockIdx.x * 256u >= npix) return;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const unsigned p = blockIdx.x * 256 + threadIdx.x;
  if (p < npix) {
    const u64 word = vw.zbuf[p];
    const bool hit = word != MAP_EMPTY;
    vw.depth[p] = hit ? __uint_as_float((unsigned)(word >> 32)) : 0.0f;
    uint8_t* o = vw.bgr + (size_t)p * 3;
    o[0] = hit ? (uint8_t)word : 0; o[1] = hit ? (uint8_t)(word >> 8) : 0; o[2] = hit ? (uint8_t)(word >> 16) : 0;
    if (hit) { vw.zbuf[p] = MAP_EMPTY; atomicAdd(&s_n, 1u); }
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(vw.covered, s_n);
}

// ------------------------------------------------------------------------------------------------------------ host side --
// pinned staging of a launch's descriptors (reused once the previous upload out of it has completed)
struct revo_map_stage {
  MapDesc* h_desc = nullptr; MapDesc* d_desc = nullptr; int cap_desc = 0;
  MapCommit* h_com = nullptr; MapCommit* d_com = nullptr; int cap_com = 0;
  hipEvent_t ev = nullptr; bool recorded = false;
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
  // device outputs of a host-output call, the views' descriptors (pinned + device) and the call's events
  u64* d_zbuf = nullptr; size_t zbuf_words = 0; bool zbuf_clean = false;
  char* d_vout = nullptr; size_t vout_bytes = 0;
  MapViewK* h_views = nullptr; MapViewK* d_views = nullptr; unsigned* d_cov = nullptr; int cap_views = 0;
  hipEvent_t ev_views = nullptr, ev_r0 = nullptr, ev_r1 = nullptr; bool views_recorded = false, rendered = false;
  // revo_map_raycast / revo_map_cast_rays: the block table (bcap slots), the counter lines, the views' descriptors (pinned +
  // device; struct MapRayView), the device outputs of a host-output call and the call's events
  u64* d_bkeys = nullptr; size_t bcap = 0;
  char* d_rcnt = nullptr;
  struct MapRayView* h_rviews = nullptr; struct MapRayView* d_rviews = nullptr; int cap_rviews = 0;
  char* d_rout = nullptr; size_t rout_bytes = 0;
  hipEvent_t ev_rviews = nullptr, ev_c0 = nullptr, ev_c1 = nullptr; bool rviews_recorded = false, raycast = false;
};

extern "C" int revo_map_stage_create_(revo_map_stage** out) {
  revo_map_stage* st = new revo_map_stage();
  if (hipEventCreateWithFlags(&st->ev, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    delete st;
    return fail(REVO_ERR_HIP, "hipEventCreate failed");
  }
  *out = st;
  return REVO_OK;
}
extern "C" void revo_map_stage_destroy_(revo_map_stage* st) {
  if (!st) return;
  if (st->recorded) (void)hipEventSynchronize(st->ev);
  hipHostFree(st->h_desc); hipFree(st->d_desc); hipHostFree(st->h_com); hipFree(st->d_com);
  hipEventDestroy(st->ev);
  (void)hipGetLastError();
  delete st;
}
static int stage_reserve(revo_map_stage* st, int nd, int nc) {
  if (st->recorded) HIPCHECK(hipEventSynchronize(st->ev));  // the previous upload has read the pinned rows
  if (nd > st->cap_desc) {
    (void)hipHostFree(st->h_desc); (void)hipFree(st->d_desc);
    st->h_desc = nullptr; st->d_desc = nullptr; st->cap_desc = 0;
    HIPCHECK(hipHostMalloc((void**)&st->h_desc, sizeof(MapDesc) * nd));
    HIPCHECK(hipMalloc((void**)&st->d_desc, sizeof(MapDesc) * nd));
    st->cap_desc = nd;
  }
  if (nc > st->cap_com) {
    (void)hipHostFree(st->h_com); (void)hipFree(st->d_com);
    st->h_com = nullptr; st->d_com = nullptr; st->cap_com = 0;
    HIPCHECK(hipHostMalloc((void**)&st->h_com, sizeof(MapCommit) * nc));
    HIPCHECK(hipMalloc((void**)&st->d_com, sizeof(MapCommit) * nc));
    st->cap_com = nc;
  }
  return REVO_OK;
}

// upper bound of the map's voxels: the last count the device published + the points of every batch enqueued after it
static size_t occ_bound(revo_map* m) {
  const u64 seen = *(volatile u64*)&m->h_pub[1];
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  const u64 occ = *(volatile u64*)&m->h_pub[0];  // written before the sequence word: at least as new
  while (!m->pending.empty() && m->pending.front().first <= seen) m->pending.pop_front();
  size_t b = (size_t)occ;
  for (auto& p : m->pending) b += p.second;
  return b;
}

// a table of `newcap` slots (power of two) holding every voxel of the old one; live_only: every voxel with count >= 1 (what
// an accepted subtraction leaves; not a growth, so not counted as a rehash)
static int grow(revo_map* m, size_t newcap, bool live_only = false) {
  hipStream_t s = (hipStream_t)m->g.stream;
  u64* nk = nullptr; MapVal* nv = nullptr;
  HIPCHECK(hipMalloc((void**)&nk, sizeof(u64) * newcap));
  if (hipMalloc((void**)&nv, sizeof(MapVal) * newcap) != hipSuccess) {
    (void)hipGetLastError(); hipFree(nk);
    return fail(REVO_ERR_HIP, "voxel map: no device memory for a table of " + std::to_string(newcap) + " slots");
  }
  HIPCHECK(hipMemsetAsync(nk, 0xff, sizeof(u64) * newcap, s));
  HIPCHECK(hipMemsetAsync(nv, 0, sizeof(MapVal) * newcap, s));
  if (m->cap) {
    if (live_only)
      hipLaunchKernelGGL(k_map_rehash_live, dim3((unsigned)((m->cap + 255) / 256)), dim3(256), 0, s, m->d_keys, m->d_vals,
                         (unsigned)m->cap, nk, nv, (unsigned)(newcap - 1), &m->d_st->fault);
    else
      hipLaunchKernelGGL(k_map_rehash, dim3((unsigned)((m->cap + 255) / 256)), dim3(256), 0, s, m->d_keys, m->d_vals,
                         (unsigned)m->cap, nk, nv, (unsigned)(newcap - 1), &m->d_st->fault);
    HIPCHECK(hipGetLastError());
    if (!live_only) ++m->rehashes;
    HIPCHECK(hipStreamSynchronize(s));  // the old table is free once the rehash has read it
  }
  hipFree(m->d_keys); hipFree(m->d_vals);
  m->d_keys = nk; m->d_vals = nv; m->cap = newcap;
  return REVO_OK;
}

static int integrate_core(revo_map_stage* st, int n, revo_map* const* maps, const MapSource* src, const float* T16,
                          std::vector<revo_map*>* checked) {
  if (n <= 0) return REVO_OK;
  const MapCtxGeom& g = maps[0]->g;
  hipStream_t s = (hipStream_t)g.stream;
  HIPCHECK(hipSetDevice(g.device));
  const size_t npix = (size_t)g.w * g.h;
  std::vector<revo_map*> dm;  // distinct maps, first appearance first
  std::vector<int> nk;
  for (int i = 0; i < n; ++i) {
    size_t j = std::find(dm.begin(), dm.end(), maps[i]) - dm.begin();
    if (j == dm.size()) { dm.push_back(maps[i]); nk.push_back(0); }
    ++nk[j];
  }
  std::vector<int> chk(dm.size(), 0);
  for (size_t j = 0; j < dm.size(); ++j) {
    revo_map* m = dm[j];
    const size_t ub = occ_bound(m), bound = (size_t)nk[j] * npix;
    chk[j] = ub + bound > m->max_voxels;
    // the checked path inserts every new key before it decides: room for what the map may hold + all points of the batch
    const size_t need = 2 * (std::min(ub, m->max_voxels) + bound);
    if (need > MAP_MAX_CAP) return fail(REVO_ERR_CAPACITY, "voxel map: a batch this large needs more than 2^31 table slots");
    if (m->cap < need) {
      size_t c = std::max<size_t>(m->cap * 2, 1024);
      while (c < need) c *= 2;
      const int rc = grow(m, c);
      if (rc) return rc;
    }
  }
  { const int rc = stage_reserve(st, n, (int)dm.size()); if (rc) return rc; }
  for (int i = 0; i < n; ++i) {
    revo_map* m = maps[i];
    MapDesc& d = st->h_desc[i];
    d.depth = src[i].depth; d.edges = src[i].edges; d.bgr = src[i].bgr;
    const float* T = T16 + 16 * (size_t)i;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) d.R[3 * r + c] = T[4 * c + r];
      d.t[r] = T[12 + r];
    }
    d.voxel = m->voxel; d.dense = m->dense;
    d.keys = m->d_keys; d.vals = m->d_vals; d.mask = (unsigned)(m->cap - 1);
    d.st = m->d_st;
  }
  bool any_check = false;
  for (size_t j = 0; j < dm.size(); ++j) {
    revo_map* m = dm[j];
    ++m->seq;
    st->h_com[j] = MapCommit{m->d_st, m->h_pub, (u64)m->max_voxels, m->seq, nk[j], chk[j]};
    m->pending.push_back({m->seq, (size_t)nk[j] * npix});
    any_check = any_check || chk[j];
    if (chk[j] && checked) checked->push_back(m);
  }
  HIPCHECK(hipMemcpyAsync(st->d_desc, st->h_desc, sizeof(MapDesc) * n, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(st->d_com, st->h_com, sizeof(MapCommit) * dm.size(), hipMemcpyHostToDevice, s));
  HIPCHECK(hipEventRecord(st->ev, s));
  st->recorded = true;
  const int nb = (int)((npix + 255) / 256);
  const MapGeomK gk{g.w, (int)npix, g.fx, g.fy, g.cx, g.cy, g.dmin, g.dmax};
  const dim3 grid((unsigned)(nb * n)), blk(256), cgrid((unsigned)((dm.size() + 63) / 64)), cblk(64);
  if (!any_check) {
    hipLaunchKernelGGL(k_map_walk<MAP_FUSED>, grid, blk, 0, s, st->d_desc, nb, gk);
    hipLaunchKernelGGL(k_map_commit, cgrid, cblk, 0, s, st->d_com, (int)dm.size());
  } else {
    hipLaunchKernelGGL(k_map_walk<MAP_INSERT>, grid, blk, 0, s, st->d_desc, nb, gk);
    hipLaunchKernelGGL(k_map_commit, cgrid, cblk, 0, s, st->d_com, (int)dm.size());
    for (size_t j = 0; j < dm.size(); ++j)
      if (chk[j])
        hipLaunchKernelGGL(k_map_rollback, dim3((unsigned)((dm[j]->cap + 255) / 256)), blk, 0, s, dm[j]->d_keys, dm[j]->d_vals,
                           (unsigned)dm[j]->cap, dm[j]->d_st);
    hipLaunchKernelGGL(k_map_walk<MAP_ACCUM>, grid, blk, 0, s, st->d_desc, nb, gk);
  }
  HIPCHECK(hipGetLastError());
  return REVO_OK;
}

static bool pose_finite(const float* T) {
  for (int i = 0; i < 16; ++i) if (!std::isfinite(T[i])) return false;
  return true;
}

extern "C" int revo_map_create(revo_ctx* ctx, float voxel, int dense, size_t initial_voxels, size_t max_voxels, revo_map** out) {
  if (!ctx || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!std::isfinite(voxel) || !(voxel > 0.0f)) return fail(REVO_ERR_INVALID_ARG, "voxel must be finite and > 0");
  if (dense != 0 && dense != 1) return fail(REVO_ERR_INVALID_ARG, "dense must be 0 or 1");
  if (max_voxels < 1 || max_voxels > MAP_MAX_VOXELS) return fail(REVO_ERR_INVALID_ARG, "max_voxels must be 1 .. 2^28");
  MapCtxGeom g;
  { const int rc = revo_map_ctx_geom_(ctx, &g); if (rc) return rc; }
  HIPCHECK(hipSetDevice(g.device));
  revo_map* m = new revo_map();
  m->ctx = ctx; m->g = g; m->voxel = voxel; m->dense = dense; m->max_voxels = max_voxels;
  revo_ctx_retain_(ctx);
  struct Guard { revo_map* m; ~Guard() { if (m) revo_map_destroy(m); } } guard{m};
  HIPCHECK(hipMalloc((void**)&m->d_st, sizeof(MapStats)));
  HIPCHECK(hipMemsetAsync(m->d_st, 0, sizeof(MapStats), (hipStream_t)g.stream));
  HIPCHECK(hipHostMalloc((void**)&m->h_pub, sizeof(u64) * 4));
  memset(m->h_pub, 0, sizeof(u64) * 4);
  { const int rc = revo_map_stage_create_(&m->stage); if (rc) return rc; }
  size_t c = 1024;
  const size_t want = std::min<size_t>(std::max<size_t>(initial_voxels, 1), max_voxels) * 2;
  while (c < want) c *= 2;
  { const int rc = grow(m, c); if (rc) return rc; }
  HIPCHECK(hipStreamSynchronize((hipStream_t)g.stream));
  guard.m = nullptr;
  *out = m;
  return REVO_OK;
}

extern "C" void revo_map_destroy(revo_map* m) {
  if (!m) return;
  const auto att = m->attached;
  for (auto& a : att) revo_vo_multi_forget_map_(a.first, a.second, m);
  hipSetDevice(m->g.device);
  (void)hipStreamSynchronize((hipStream_t)m->g.stream);
  revo_map_stage_destroy_(m->stage);
  hipFree(m->d_keys); hipFree(m->d_vals); hipFree(m->d_st); hipHostFree(m->h_pub);
  hipFree(m->d_zbuf); hipFree(m->d_vout); hipFree(m->d_views); hipFree(m->d_cov); hipHostFree(m->h_views);
  if (m->ev_views) hipEventDestroy(m->ev_views);
  if (m->ev_r0) hipEventDestroy(m->ev_r0);
  if (m->ev_r1) hipEventDestroy(m->ev_r1);
  hipFree(m->d_bkeys); hipFree(m->d_rcnt); hipFree(m->d_rviews); hipFree(m->d_rout); hipHostFree(m->h_rviews);
  if (m->ev_rviews) hipEventDestroy(m->ev_rviews);
  if (m->ev_c0) hipEventDestroy(m->ev_c0);
  if (m->ev_c1) hipEventDestroy(m->ev_c1);
  (void)hipGetLastError();
  revo_ctx_release_(m->ctx);
  delete m;
}

extern "C" int revo_map_integrate_many(revo_map* m, int n, const revo_pyr* const* kfs, const float* T) {
  if (!m || n < 0 || (n > 0 && (!kfs || !T))) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n == 0) return REVO_OK;
  for (int i = 0; i < n; ++i) {
    if (!kfs[i]) return fail(REVO_ERR_INVALID_ARG, "null pyramid");
    if (!pose_finite(T + 16 * (size_t)i)) return fail(REVO_ERR_INVALID_ARG, "T_w_kf is not finite");
  }
  std::vector<MapSource> src(n);
  for (int i = 0; i < n; ++i) {
    const int rc = revo_map_source_(const_cast<revo_pyr*>(kfs[i]), &src[i]);
    if (rc) return rc;
    if (src[i].ctx != m->ctx) return fail(REVO_ERR_INVALID_ARG, "the pyramid belongs to another context than the map");
  }
  std::vector<revo_map*> maps(n, m), checked;
  { const int rc = integrate_core(m->stage, n, maps.data(), src.data(), T, &checked); if (rc) return rc; }
  if (!checked.empty()) {  // the map could have reached max_voxels: the device has decided, wait for it
    HIPCHECK(hipStreamSynchronize((hipStream_t)m->g.stream));
    if (!m->h_pub[2]) return fail(REVO_ERR_CAPACITY, "voxel map: the keyframes would take it past max_voxels (not integrated)");
  }
  return REVO_OK;
}
extern "C" int revo_map_integrate(revo_map* m, const revo_pyr* kf, const float T[16]) {
  if (!m || !kf || !T) return fail(REVO_ERR_INVALID_ARG, "null argument");
  return revo_map_integrate_many(m, 1, &kf, T);
}

extern "C" int revo_map_integrate_views_(revo_map_stage* st, int n, revo_map* const* maps, revo_pyr* const* kfs, const float* T) {
  if (n <= 0) return REVO_OK;
  std::vector<MapSource> src(n);
  for (int i = 0; i < n; ++i) {
    const int rc = revo_map_source_(kfs[i], &src[i]);
    if (rc) return rc;
  }
  return integrate_core(st, n, maps, src.data(), T, nullptr);
}

extern "C" int revo_map_clear(revo_map* m) {
  if (!m) return fail(REVO_ERR_INVALID_ARG, "null map");
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  HIPCHECK(hipMemsetAsync(m->d_keys, 0xff, sizeof(u64) * m->cap, s));
  HIPCHECK(hipMemsetAsync(m->d_vals, 0, sizeof(MapVal) * m->cap, s));
  HIPCHECK(hipMemsetAsync(m->d_st, 0, sizeof(MapStats), s));
  HIPCHECK(hipStreamSynchronize(s));
  m->pending.clear();
  m->h_pub[0] = 0; m->h_pub[2] = 1; m->h_pub[1] = m->seq;
  m->rehashes = 0;
  return REVO_OK;
}

static int read_stats(revo_map* m, MapStats* out) {
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  HIPCHECK(hipStreamSynchronize(s));
  HIPCHECK(hipMemcpy(out, m->d_st, sizeof(MapStats), hipMemcpyDeviceToHost));
  if (out->fault) return fail(REVO_ERR_HIP, "voxel map: a probe ran through the whole table (load invariant broken)");
  return REVO_OK;
}

extern "C" int revo_map_info(revo_map* m, revo_map_info_t* out) {
  if (!m || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  MapStats st;
  { const int rc = read_stats(m, &st); if (rc) return rc; }
  out->voxels = (size_t)st.occ;
  out->points_integrated = (size_t)st.pts;
  out->points_dropped = (size_t)st.drop;
  out->capacity = m->cap;
  out->keyframes = (int32_t)st.kfs;
  out->keyframes_rejected = (int32_t)st.rejected;
  out->rehashes = m->rehashes;
  return REVO_OK;
}

extern "C" int revo_map_extract(revo_map* m, size_t min_count, float* xyz, uint8_t* rgb, uint32_t* count, size_t cap, size_t* n) {
  if (!m || !n) return fail(REVO_ERR_INVALID_ARG, "null argument");
  MapStats st;
  { const int rc = read_stats(m, &st); if (rc) return rc; }
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t nv = std::max<size_t>((size_t)st.occ, 1);
  char* buf = nullptr;
  const size_t o_key = 0, o_xyz = o_key + 8 * nv, o_rgb = o_xyz + 12 * nv, o_cnt = o_rgb + 4 * nv, o_tot = o_cnt + 4 * nv;
  HIPCHECK(hipMalloc((void**)&buf, o_tot + 256));
  struct Free { char* p; ~Free() { hipFree(p); } } fr{buf};
  unsigned* d_tot = (unsigned*)(buf + o_tot);
  HIPCHECK(hipMemsetAsync(d_tot, 0, sizeof(unsigned), s));
  hipLaunchKernelGGL(k_map_extract, dim3((unsigned)((m->cap + 255) / 256)), dim3(256), 0, s, m->d_keys, m->d_vals, (unsigned)m->cap,
                     (u64)std::max<size_t>(min_count, 1), d_tot, (u64*)(buf + o_key), (float*)(buf + o_xyz),
                     (unsigned*)(buf + o_rgb), (unsigned*)(buf + o_cnt));
  HIPCHECK(hipGetLastError());
  unsigned tot = 0;
  HIPCHECK(hipMemcpyAsync(&tot, d_tot, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  *n = tot;
  if (!xyz) return REVO_OK;
  if (cap < tot) return fail(REVO_ERR_CAPACITY, "voxel map: the output holds fewer voxels than the map has");
  std::vector<u64> key(tot);
  std::vector<float> p(3 * (size_t)tot);
  std::vector<unsigned> c(tot), k(tot);
  if (tot) {
    HIPCHECK(hipMemcpy(key.data(), buf + o_key, 8 * (size_t)tot, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(p.data(), buf + o_xyz, 12 * (size_t)tot, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(c.data(), buf + o_rgb, 4 * (size_t)tot, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(k.data(), buf + o_cnt, 4 * (size_t)tot, hipMemcpyDeviceToHost));
  }
  std::vector<unsigned> idx(tot);
  std::iota(idx.begin(), idx.end(), 0u);
  std::sort(idx.begin(), idx.end(), [&](unsigned a, unsigned b) { return key[a] < key[b]; });  // keys are distinct
  for (size_t j = 0; j < tot; ++j) {
    const unsigned i = idx[j];
    memcpy(xyz + 3 * j, &p[3 * (size_t)i], 12);
    if (rgb) { rgb[3 * j] = (uint8_t)c[i]; rgb[3 * j + 1] = (uint8_t)(c[i] >> 8); rgb[3 * j + 2] = (uint8_t)(c[i] >> 16); }
    if (count) count[j] = k[i];
  }
  return REVO_OK;
}

static_assert(sizeof(revo_map_voxel_raw) == 64 && sizeof(MapVal) == 64, "a voxel record is four 16-byte words");

extern "C" int revo_map_voxel_size(revo_map* m, float* voxel, int* dense) {
  if (!m) return fail(REVO_ERR_INVALID_ARG, "null map");
  if (voxel) *voxel = m->voxel;
  if (dense) *dense = m->dense;
  return REVO_OK;
}

extern "C" int revo_map_export_raw(revo_map* m, revo_map_voxel_raw* dst, size_t cap, size_t* n, int device_out) {
  if (!m || !n) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (device_out != 0 && device_out != 1) return fail(REVO_ERR_INVALID_ARG, "device_out must be 0 or 1");
  if (device_out && ((uintptr_t)dst & 15)) return fail(REVO_ERR_INVALID_ARG, "the device output is not 16-byte aligned");
  MapStats st;
  { const int rc = read_stats(m, &st); if (rc) return rc; }
  const size_t nv = (size_t)st.occ;
  *n = nv;
  if (!dst) return REVO_OK;
  if (cap < nv) return fail(REVO_ERR_CAPACITY, "voxel map: the output holds fewer records than the map has voxels");
  if (!nv) return REVO_OK;
  hipStream_t s = (hipStream_t)m->g.stream;
  char* buf = nullptr;  // the launch's counter, and the records of a host-output call behind it
  HIPCHECK(hipMalloc((void**)&buf, 256 + (device_out ? 0 : sizeof(revo_map_voxel_raw) * nv)));
  struct Free { char* p; ~Free() { hipFree(p); } } fr{buf};
  unsigned* d_tot = (unsigned*)buf;
  ulonglong2* d_rec = device_out ? (ulonglong2*)dst : (ulonglong2*)(buf + 256);
  HIPCHECK(hipMemsetAsync(d_tot, 0, sizeof(unsigned), s));
  hipLaunchKernelGGL(k_map_export, dim3((unsigned)((m->cap + 255) / 256)), dim3(256), 0, s, m->d_keys, m->d_vals, (unsigned)m->cap,
                     d_tot, d_rec, (unsigned)nv);
  HIPCHECK(hipGetLastError());
  unsigned tot = 0;
  HIPCHECK(hipMemcpyAsync(&tot, d_tot, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (tot != nv) return fail(REVO_ERR_HIP, "voxel map: the table holds " + std::to_string(tot) + " keys, its counter says " + std::to_string(nv));
  if (device_out) return REVO_OK;
  HIPCHECK(hipMemcpy(dst, d_rec, sizeof(revo_map_voxel_raw) * nv, hipMemcpyDeviceToHost));
  std::sort(dst, dst + nv, [](const revo_map_voxel_raw& a, const revo_map_voxel_raw& b) { return a.key < b.key; });  // keys are distinct
  return REVO_OK;
}

// One merge into m: `src` names the input (its table fields are filled here), `bound` its keys at most, `trusted` that no
// record can be bad (validated on the host, or a map's own table).  Grows for bound more keys, then the fused launch, or the
// checked path (insert, commit, rollback, accumulate) when the device has to decide -- max_voxels in reach, or records nobody
// has looked at -- and then waits for the decision.
template <int MODE>
static void launch_merge(int src_kind, dim3 grid, hipStream_t s, const MapMergeK& a) {
  if (src_kind == MERGE_TABLE) hipLaunchKernelGGL((k_map_merge<MODE, MERGE_TABLE>), grid, dim3(256), 0, s, a);
  else if (src_kind == MERGE_COARSE) hipLaunchKernelGGL((k_map_merge<MODE, MERGE_COARSE>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_map_merge<MODE, MERGE_RAW>), grid, dim3(256), 0, s, a);
}
static int merge_core(revo_map* m, MapMergeK a, int src_kind, size_t bound, bool trusted, int keyframes) {
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t ub = occ_bound(m);
  const bool chk = !trusted || ub + bound > m->max_voxels;
  const size_t need = 2 * (std::min(ub, m->max_voxels) + bound);
  if (need > MAP_MAX_CAP) return fail(REVO_ERR_CAPACITY, "voxel map: a merge this large needs more than 2^31 table slots");
  if (m->cap < need) {
    size_t c = std::max<size_t>(m->cap * 2, 1024);
    while (c < need) c *= 2;
    const int rc = grow(m, c);
    if (rc) return rc;
  }
  revo_map_stage* st = m->stage;
  { const int rc = stage_reserve(st, 0, 1); if (rc) return rc; }
  ++m->seq;
  st->h_com[0] = MapCommit{m->d_st, m->h_pub, (u64)m->max_voxels, m->seq, keyframes, chk ? 1 : 0};
  m->pending.push_back({m->seq, bound});
  HIPCHECK(hipMemcpyAsync(st->d_com, st->h_com, sizeof(MapCommit), hipMemcpyHostToDevice, s));
  HIPCHECK(hipEventRecord(st->ev, s));
  st->recorded = true;
  if (!trusted) HIPCHECK(hipMemsetAsync(&m->d_st->bad, 0, sizeof(u64), s));
  a.keys = m->d_keys; a.vals = m->d_vals; a.mask = (unsigned)(m->cap - 1); a.st = m->d_st;
  const dim3 grid((a.n + 255) / 256), blk(256);
  if (!chk) {
    launch_merge<MAP_FUSED>(src_kind, grid, s, a);
    hipLaunchKernelGGL(k_map_commit, dim3(1), dim3(64), 0, s, st->d_com, 1);
    HIPCHECK(hipGetLastError());
    return REVO_OK;
  }
  launch_merge<MAP_INSERT>(src_kind, grid, s, a);
  hipLaunchKernelGGL(k_map_commit, dim3(1), dim3(64), 0, s, st->d_com, 1);
  hipLaunchKernelGGL(k_map_rollback, dim3((unsigned)((m->cap + 255) / 256)), blk, 0, s, m->d_keys, m->d_vals, (unsigned)m->cap, m->d_st);
  launch_merge<MAP_ACCUM>(src_kind, grid, s, a);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));  // the device has decided
  if (m->h_pub[2]) return REVO_OK;
  u64 bad = 0;
  if (!trusted) HIPCHECK(hipMemcpy(&bad, &m->d_st->bad, sizeof(u64), hipMemcpyDeviceToHost));
  if (bad) return fail(REVO_ERR_INVALID_ARG, "voxel map: a record has count 0 or key bit 63 set (nothing merged)");
  return fail(REVO_ERR_CAPACITY, "voxel map: the merge would take it past max_voxels (nothing merged)");
}

extern "C" int revo_map_merge_raw(revo_map* m, const revo_map_voxel_raw* src, size_t n, int device_in, size_t points_dropped,
                                  int32_t keyframes) {
  if (!m) return fail(REVO_ERR_INVALID_ARG, "null map");
  if (device_in != 0 && device_in != 1) return fail(REVO_ERR_INVALID_ARG, "device_in must be 0 or 1");
  if (keyframes < 0) return fail(REVO_ERR_INVALID_ARG, "keyframes must be >= 0");
  if (n == 0) return REVO_OK;
  if (!src) return fail(REVO_ERR_INVALID_ARG, "null records");
  if (device_in && ((uintptr_t)src & 15)) return fail(REVO_ERR_INVALID_ARG, "the device records are not 16-byte aligned");
  if (n > MAP_MAX_CAP / 2) return fail(REVO_ERR_CAPACITY, "voxel map: a merge this large needs more than 2^31 table slots");
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  MapMergeK a{};
  a.n = (unsigned)n;
  a.dropped = (u64)points_dropped;
  if (device_in) {
    a.recs = (const ulonglong2*)src;
    return merge_core(m, a, MERGE_RAW, n, false, keyframes);
  }
  bool valid = true;  // a bad record still goes to the device, which refuses the merge and counts it
  for (size_t i = 0; i < n && valid; ++i) valid = src[i].count != 0 && !(src[i].key >> 63);
  char* buf = nullptr;
  HIPCHECK(hipMalloc((void**)&buf, sizeof(revo_map_voxel_raw) * n));
  struct Free { char* p; ~Free() { hipFree(p); } } fr{buf};
  HIPCHECK(hipMemcpyAsync(buf, src, sizeof(revo_map_voxel_raw) * n, hipMemcpyHostToDevice, s));
  a.recs = (const ulonglong2*)buf;
  const int rc = merge_core(m, a, MERGE_RAW, n, valid, keyframes);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) return fail(REVO_ERR_HIP, "hipStreamSynchronize failed");  // buf is read
  return rc;
}

extern "C" int revo_map_merge(revo_map* dst, revo_map* src) {
  if (!dst || !src) return fail(REVO_ERR_INVALID_ARG, "null map");
  if (dst == src) return fail(REVO_ERR_INVALID_ARG, "a map cannot be merged into itself");
  if (memcmp(&dst->voxel, &src->voxel, sizeof(float))) return fail(REVO_ERR_INVALID_ARG, "the maps' voxel edges differ");
  if (dst->g.device != src->g.device) return fail(REVO_ERR_INVALID_ARG, "the maps are on different devices");
  MapStats ss;  // waits for src: its table is complete, and its counters say what comes
  { const int rc = read_stats(src, &ss); if (rc) return rc; }
  if (ss.kfs > 0x7fffffffull) return fail(REVO_ERR_INVALID_ARG, "the source map's keyframe count does not fit");
  MapMergeK a{};
  a.skeys = src->d_keys; a.svals = src->d_vals; a.n = (unsigned)src->cap;
  a.dropped = ss.drop;
  const int rc = merge_core(dst, a, MERGE_TABLE, (size_t)ss.occ, true, (int)ss.kfs);
  // maps of two contexts run on two streams: src's table must outlive the launch that reads it
  if (dst->g.stream != src->g.stream && hipStreamSynchronize((hipStream_t)dst->g.stream) != hipSuccess && !rc)
    return fail(REVO_ERR_HIP, "hipStreamSynchronize failed");
  return rc;
}

// One subtraction from m (contract: include/revo_hip.h): `a` names the input as in merge_core.  Subtract, verify,
// decide, undo if refused -- all enqueued at once behind the map's pending work -- then the call waits for the decision, and
// an accepted one that emptied voxels moves the live ones into a fresh table of the same size.
static int subtract_core(revo_map* m, MapMergeK a, int src_kind, u64 dropped, u64 keyframes) {
  hipStream_t s = (hipStream_t)m->g.stream;
  ++m->seq;
  const MapSubCommit c{m->d_st, m->h_pub, m->seq, dropped, keyframes};
  HIPCHECK(hipMemsetAsync(&m->d_st->sub_bad, 0, 3 * sizeof(u64), s));
  a.keys = m->d_keys; a.vals = m->d_vals; a.mask = (unsigned)(m->cap - 1); a.st = m->d_st;
  const dim3 grid((a.n + 255) / 256), blk(256);
  const bool tab = src_kind == MERGE_TABLE;
  if (tab) {
    hipLaunchKernelGGL((k_map_sub<MERGE_TABLE, false>), grid, blk, 0, s, a);
    hipLaunchKernelGGL((k_map_sub_verify<MERGE_TABLE>), grid, blk, 0, s, a);
  } else {
    hipLaunchKernelGGL((k_map_sub<MERGE_RAW, false>), grid, blk, 0, s, a);
    hipLaunchKernelGGL((k_map_sub_verify<MERGE_RAW>), grid, blk, 0, s, a);
  }
  hipLaunchKernelGGL(k_map_sub_commit, dim3(1), dim3(64), 0, s, c);
  if (tab) hipLaunchKernelGGL((k_map_sub<MERGE_TABLE, true>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((k_map_sub<MERGE_RAW, true>), grid, blk, 0, s, a);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));  // the device has decided
  if (!m->h_pub[2])
    return fail(REVO_ERR_INVALID_ARG, "voxel map: the records are not part of the map -- a record with count 0 or key bit 63, a key "
                                      "the map does not hold, more than a voxel has, sums left in an emptied voxel, or more "
                                      "dropped points or keyframes than the map counts (nothing subtracted)");
  if (!m->h_pub[3]) return REVO_OK;
  const int rc = grow(m, m->cap, true);
  if (!rc) return REVO_OK;
  // no memory for the fresh table: the dead slots cannot stay, so the subtraction is taken back as a refused one is
  const std::string why = revo_last_error();
  ++m->seq;
  const MapSubCommit r{m->d_st, m->h_pub, m->seq, dropped, keyframes};
  hipLaunchKernelGGL(k_map_sub_revert, dim3(1), dim3(64), 0, s, r);
  if (tab) hipLaunchKernelGGL((k_map_sub<MERGE_TABLE, true>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((k_map_sub<MERGE_RAW, true>), grid, blk, 0, s, a);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));
  return fail(rc, why + " (nothing subtracted)");
}

extern "C" int revo_map_subtract_raw(revo_map* m, const revo_map_voxel_raw* src, size_t n, int device_in, size_t points_dropped,
                                     int32_t keyframes) {
  if (!m) return fail(REVO_ERR_INVALID_ARG, "null map");
  if (device_in != 0 && device_in != 1) return fail(REVO_ERR_INVALID_ARG, "device_in must be 0 or 1");
  if (keyframes < 0) return fail(REVO_ERR_INVALID_ARG, "keyframes must be >= 0");
  if (n == 0) return REVO_OK;
  if (!src) return fail(REVO_ERR_INVALID_ARG, "null records");
  if (device_in && ((uintptr_t)src & 15)) return fail(REVO_ERR_INVALID_ARG, "the device records are not 16-byte aligned");
  if (n > MAP_MAX_CAP) return fail(REVO_ERR_INVALID_ARG, "voxel map: more than 2^31 records in one subtraction");
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  MapMergeK a{};
  a.n = (unsigned)n;
  if (device_in) {
    a.recs = (const ulonglong2*)src;
    return subtract_core(m, a, MERGE_RAW, (u64)points_dropped, (u64)keyframes);
  }
  char* buf = nullptr;
  HIPCHECK(hipMalloc((void**)&buf, sizeof(revo_map_voxel_raw) * n));
  struct Free { char* p; ~Free() { hipFree(p); } } fr{buf};
  HIPCHECK(hipMemcpyAsync(buf, src, sizeof(revo_map_voxel_raw) * n, hipMemcpyHostToDevice, s));
  a.recs = (const ulonglong2*)buf;
  return subtract_core(m, a, MERGE_RAW, (u64)points_dropped, (u64)keyframes);  // has waited: buf is read
}

extern "C" int revo_map_subtract(revo_map* dst, revo_map* src) {
  if (!dst || !src) return fail(REVO_ERR_INVALID_ARG, "null map");
  if (dst == src) return fail(REVO_ERR_INVALID_ARG, "a map cannot be subtracted from itself (revo_map_clear empties it)");
  if (memcmp(&dst->voxel, &src->voxel, sizeof(float))) return fail(REVO_ERR_INVALID_ARG, "the maps' voxel edges differ");
  if (dst->g.device != src->g.device) return fail(REVO_ERR_INVALID_ARG, "the maps are on different devices");
  MapStats ss;  // waits for src: its table is complete, and its counters say what goes
  { const int rc = read_stats(src, &ss); if (rc) return rc; }
  HIPCHECK(hipSetDevice(dst->g.device));
  MapMergeK a{};
  a.skeys = src->d_keys; a.svals = src->d_vals; a.n = (unsigned)src->cap;
  return subtract_core(dst, a, MERGE_TABLE, ss.drop, ss.kfs);  // has waited for dst's stream: src's table is read
}

// room for a call's views: descriptors, counters, z-buffer words (kept MAP_EMPTY), device outputs of a host-output call
static int render_reserve(revo_map* m, int n, size_t words, size_t out_bytes) {
  hipStream_t s = (hipStream_t)m->g.stream;
  if (!m->ev_views) {
    HIPCHECK(hipEventCreateWithFlags(&m->ev_views, hipEventDisableTiming));
    HIPCHECK(hipEventCreate(&m->ev_r0));
    HIPCHECK(hipEventCreate(&m->ev_r1));
  }
  if (m->views_recorded) HIPCHECK(hipEventSynchronize(m->ev_views));  // the previous upload has read the pinned rows
  if (n > m->cap_views) {
    HIPCHECK(hipStreamSynchronize(s));  // the previous call's kernels read the descriptors
    (void)hipHostFree(m->h_views); (void)hipFree(m->d_views); (void)hipFree(m->d_cov);
    m->h_views = nullptr; m->d_views = nullptr; m->d_cov = nullptr; m->cap_views = 0;
    HIPCHECK(hipHostMalloc((void**)&m->h_views, sizeof(MapViewK) * n));
    HIPCHECK(hipMalloc((void**)&m->d_views, sizeof(MapViewK) * n));
    HIPCHECK(hipMalloc((void**)&m->d_cov, sizeof(unsigned) * n));
    m->cap_views = n;
  }
  if (words > m->zbuf_words) {
    HIPCHECK(hipStreamSynchronize(s));
    (void)hipFree(m->d_zbuf);
    m->d_zbuf = nullptr; m->zbuf_words = 0;
    HIPCHECK(hipMalloc((void**)&m->d_zbuf, sizeof(u64) * words));
    m->zbuf_words = words;
    m->zbuf_clean = false;
  }
  if (!m->zbuf_clean) HIPCHECK(hipMemsetAsync(m->d_zbuf, 0xff, sizeof(u64) * m->zbuf_words, s));
  if (out_bytes > m->vout_bytes) {
    HIPCHECK(hipStreamSynchronize(s));
    (void)hipFree(m->d_vout);
    m->d_vout = nullptr; m->vout_bytes = 0;
    HIPCHECK(hipMalloc((void**)&m->d_vout, out_bytes));
    m->vout_bytes = out_bytes;
  }
  return REVO_OK;
}

extern "C" int revo_map_render(revo_map* m, int n, const revo_map_view* views, float* const* depth, uint8_t* const* bgr,
                               uint32_t* covered, int device_out) {
  if (!m || !views || !depth || !bgr) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n < 1) return fail(REVO_ERR_INVALID_ARG, "revo_map_render: n must be >= 1");
  if (device_out != 0 && device_out != 1) return fail(REVO_ERR_INVALID_ARG, "device_out must be 0 or 1");
  if (device_out && ((uintptr_t)covered & 15)) return fail(REVO_ERR_INVALID_ARG, "covered is not 16-byte aligned");
  std::vector<revo_map_view> vs(views, views + n);
  size_t words = 0, out_bytes = 0;
  int max_pix = 0;
  for (int i = 0; i < n; ++i) {
    revo_map_view& v = vs[i];
    const std::string at = "view " + std::to_string(i) + ": ";
    if (!depth[i] || !bgr[i]) return fail(REVO_ERR_INVALID_ARG, at + "null output");
    if (device_out && (((uintptr_t)depth[i] | (uintptr_t)bgr[i]) & 15))
      return fail(REVO_ERR_INVALID_ARG, at + "a device output is not 16-byte aligned");
    if (v.width < 1 || v.width > 2048 || v.height < 1 || v.height > 2048)
      return fail(REVO_ERR_INVALID_ARG, at + "width and height must be 1 .. 2048");
    if (v.splat_max < 0 || v.splat_max > 8) return fail(REVO_ERR_INVALID_ARG, at + "splat_max must be 0 .. 8");
    if (!pose_finite(v.T_w_c)) return fail(REVO_ERR_INVALID_ARG, at + "T_w_c is not finite");
    const float k[6] = {v.fx, v.fy, v.cx, v.cy, v.zmin, v.zmax};
    bool zero = true, finite = true;
    for (float f : k) { zero = zero && f == 0.0f; finite = finite && std::isfinite(f); }
    if (zero) {
      v.fx = m->g.fx; v.fy = m->g.fy; v.cx = m->g.cx; v.cy = m->g.cy; v.zmin = m->g.dmin; v.zmax = m->g.dmax;
    } else {
      if (!finite) return fail(REVO_ERR_INVALID_ARG, at + "intrinsics and depth range must be finite");
      if (!(v.fx > 0.0f) || !(v.fy > 0.0f)) return fail(REVO_ERR_INVALID_ARG, at + "fx and fy must be > 0");
    }
    if (!(v.zmin >= 0.0f) || !(v.zmin < v.zmax)) return fail(REVO_ERR_INVALID_ARG, at + "the depth range needs 0 <= zmin < zmax");
    const size_t np = (size_t)v.width * v.height;
    words += np;
    out_bytes += (np * 7 + 15) & ~(size_t)15;
    max_pix = std::max(max_pix, (int)np);
  }
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  { const int rc = render_reserve(m, n, words, device_out ? 0 : out_bytes); if (rc) return rc; }
  unsigned* d_cov = device_out && covered ? covered : m->d_cov;
  size_t zo = 0, oo = 0;
  for (int i = 0; i < n; ++i) {
    const revo_map_view& v = vs[i];
    MapViewK& d = m->h_views[i];
    const float* T = v.T_w_c;  // column-major: R(r, c) = T[4 c + r], so Rc(r, c) = R(c, r) = T[4 r + c]
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) d.Rc[3 * r + c] = T[4 * r + c];
      d.tc[r] = -(((d.Rc[3 * r] * T[12]) + (d.Rc[3 * r + 1] * T[13])) + (d.Rc[3 * r + 2] * T[14]));
    }
    d.fx = v.fx; d.fy = v.fy; d.cx = v.cx; d.cy = v.cy; d.zmin = v.zmin; d.zmax = v.zmax;
    d.hv = 0.5f * m->voxel;
    d.w = v.width; d.h = v.height; d.splat = v.splat_max;
    d.min_count = std::max<u64>(v.min_count, 1);
    const size_t np = (size_t)v.width * v.height;
    d.zbuf = m->d_zbuf + zo;
    zo += np;
    if (device_out) { d.depth = depth[i]; d.bgr = bgr[i]; }
    else { d.depth = (float*)(m->d_vout + oo); d.bgr = (uint8_t*)(m->d_vout + oo + np * 4); oo += (np * 7 + 15) & ~(size_t)15; }
    d.covered = d_cov + i;
  }
  HIPCHECK(hipMemcpyAsync(m->d_views, m->h_views, sizeof(MapViewK) * n, hipMemcpyHostToDevice, s));
  HIPCHECK(hipEventRecord(m->ev_views, s));
  m->views_recorded = true;
  HIPCHECK(hipMemsetAsync(d_cov, 0, sizeof(unsigned) * n, s));
  m->zbuf_clean = false;  // until the resolve launch that puts every word back is enqueued
  HIPCHECK(hipEventRecord(m->ev_r0, s));
  const dim3 blk(256), sgrid((unsigned)((m->cap + 255) / 256), (unsigned)n), rgrid((unsigned)((max_pix + 255) / 256), (unsigned)n);
  // REVO_MAP_RENDER_SKIP=0: every footprint pixel takes its atomic without the load in front (profiles/map_render_rates.py)
  if (env_int("REVO_MAP_RENDER_SKIP", 1, 0, 1))
    hipLaunchKernelGGL(k_map_splat<true>, sgrid, blk, 0, s, m->d_keys, m->d_vals, (unsigned)m->cap, m->d_views);
  else
    hipLaunchKernelGGL(k_map_splat<false>, sgrid, blk, 0, s, m->d_keys, m->d_vals, (unsigned)m->cap, m->d_views);
  HIPCHECK(hipGetLastError());
  hipLaunchKernelGGL(k_map_view_resolve, rgrid, blk, 0, s, m->d_views);
  HIPCHECK(hipGetLastError());
  m->zbuf_clean = true;
  HIPCHECK(hipEventRecord(m->ev_r1, s));
  m->rendered = true;
  if (device_out) return REVO_OK;
  oo = 0;
  for (int i = 0; i < n; ++i) {
    const size_t np = (size_t)vs[i].width * vs[i].height;
    HIPCHECK(hipMemcpyAsync(depth[i], m->d_vout + oo, np * 4, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipMemcpyAsync(bgr[i], m->d_vout + oo + np * 4, np * 3, hipMemcpyDeviceToHost, s));
    oo += (np * 7 + 15) & ~(size_t)15;
  }
  if (covered) HIPCHECK(hipMemcpyAsync(covered, d_cov, sizeof(unsigned) * n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_render_last_ms(revo_map* m, float* ms) {
  if (!m || !ms) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!m->rendered) return fail(REVO_ERR_INVALID_ARG, "the map has rendered nothing yet");
  HIPCHECK(hipSetDevice(m->g.device));
  HIPCHECK(hipEventSynchronize(m->ev_r1));
  HIPCHECK(hipEventElapsedTime(ms, m->ev_r0, m->ev_r1));
  return REVO_OK;
}

extern "C" void revo_map_note_attach_(revo_map* m, revo_vo_multi* mv, int stream, int attach) {
  if (!m) return;
  auto it = std::find(m->attached.begin(), m->attached.end(), std::make_pair(mv, stream));
  if (attach && it == m->attached.end()) m->attached.push_back({mv, stream});
  if (!attach && it != m->attached.end()) m->attached.erase(it);
}
extern "C" const revo_ctx* revo_map_ctx_(const revo_map* m) { return m ? m->ctx : nullptr; }

// ------------------------------------------------------------------------------------------------- registration (16) --
// revo_map_coarsen / revo_map_align_eval / revo_map_align (contract: include/revo_hip.h).
extern "C" int revo_map_coarsen(revo_map* dst, revo_map* src, int shift) {
  if (!dst || !src) return fail(REVO_ERR_INVALID_ARG, "null map");
  if (dst == src) return fail(REVO_ERR_INVALID_ARG, "a map cannot be coarsened into itself");
  if (shift < 1 || shift > 20) return fail(REVO_ERR_INVALID_ARG, "shift must be 1 .. 20");
  const float want = std::ldexp(src->voxel, shift);  // exact, or inf
  if (memcmp(&dst->voxel, &want, sizeof(float)))
    return fail(REVO_ERR_INVALID_ARG, "the destination's voxel edge is not the source's times 2^shift");
  if (dst->g.device != src->g.device) return fail(REVO_ERR_INVALID_ARG, "the maps are on different devices");
  MapStats ss;  // waits for src: its table is complete, and its counters say what comes
  { const int rc = read_stats(src, &ss); if (rc) return rc; }
  if (ss.kfs > 0x7fffffffull) return fail(REVO_ERR_INVALID_ARG, "the source map's keyframe count does not fit");
  HIPCHECK(hipSetDevice(dst->g.device));
  MapMergeK a{};
  a.skeys = src->d_keys; a.svals = src->d_vals; a.n = (unsigned)src->cap;
  a.dropped = ss.drop;
  a.shift = shift;
  const int rc = merge_core(dst, a, MERGE_COARSE, (size_t)ss.occ, true, (int)ss.kfs);
  if (dst->g.stream != src->g.stream && hipStreamSynchronize((hipStream_t)dst->g.stream) != hipSuccess && !rc)
    return fail(REVO_ERR_HIP, "hipStreamSynchronize failed");
  return rc;
}

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

__device__ __forceinline__ float map_mean(u64 q, double n) { return (float)((double)(long long)q / n * 0x1p-20); }  // k_map_extract

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
  const unsigned o = sel ? atomicAdd(&s_n, 1u) : 0u;
  __syncthreads();
  if (threadIdx.x == 0) s_base = s_n ? atomicAdd(total, s_n) : 0u;
  __syncthreads();
  if (!sel) return;
  const unsigned j = s_base + o;
  if (j >= cap_out) return;
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
    const int k0 = (int)((key >> 42) & 0x1fffffu), k1 = (int)((key >> 21) & 0x1fffffu), k2 = (int)(key & 0x1fffffu);  // biased
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sxx = 0.0f, sxy = 0.0f, sxz = 0.0f, syy = 0.0f, syz = 0.0f, szz = 0.0f;
    unsigned nb = 0;
#pragma unroll 1
    for (int c = 0; c < 27; ++c) {
      const int kx = k0 + c / 9 - 1, ky = k1 + (c / 3) % 3 - 1, kz = k2 + c % 3 - 1;
      if ((kx | ky | kz) >> 21) continue;  // a biased index outside [0, 2^21 - 1] (-1 has every bit set)
      const unsigned s = map_find(a.keys, a.mask, ((u64)kx << 42) | ((u64)ky << 21) | (u64)kz);
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
  const unsigned o = sel ? atomicAdd(&s_n, 1u) : 0u;
  __syncthreads();
  if (threadIdx.x == 0) s_base = s_n ? atomicAdd(total, s_n) : 0u;
  __syncthreads();
  if (!sel) return;
  const unsigned j = s_base + o;
  if (j >= cap_out) return;
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
        if (((kx + (1 << 20)) | (ky + (1 << 20)) | (kz + (1 << 20))) >> 21) continue;  // an index outside [-2^20, 2^20 - 1]
        const u64 key = ((u64)(kx + (1 << 20)) << 42) | ((u64)(ky + (1 << 20)) << 21) | (u64)(kz + (1 << 20));
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
  { const int rc = read_stats(src, &ss); if (rc) return rc; }
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
  { const int rc = align_launch(c, 1, T, nullptr); if (rc) return rc; }
  hipStream_t s = (hipStream_t)c->dst->g.stream;
  HIPCHECK(hipMemcpyAsync(out, c->d_out, c->rec_bytes, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_align_eval(revo_map* dst, revo_map* src, int n, const float* T, const revo_map_align_params* prm,
                                   revo_map_align_info* out, int device_out) {
  { const int rc = align_check(dst, src, prm); if (rc) return rc; }
  if (!T || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n < 1 || n > 65535) return fail(REVO_ERR_INVALID_ARG, "revo_map_align_eval: n must be 1 .. 65535");
  if (device_out != 0 && device_out != 1) return fail(REVO_ERR_INVALID_ARG, "device_out must be 0 or 1");
  if (device_out && ((uintptr_t)out & 15)) return fail(REVO_ERR_INVALID_ARG, "the device output is not 16-byte aligned");
  MapAlignCall c;
  { const int rc = align_begin(&c, dst, src, prm, n); if (rc) return rc; }
  { const int rc = align_launch(&c, n, T, device_out ? out : nullptr); if (rc) return rc; }
  hipStream_t s = (hipStream_t)dst->g.stream;
  if (!device_out) HIPCHECK(hipMemcpyAsync(out, c.d_out, sizeof(revo_map_align_info) * n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
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
  { const int rc = align_check(dst, src, prm); if (rc) return rc; }
  if (!T_init || !T_out || !status) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!pose_finite(T_init)) return fail(REVO_ERR_INVALID_ARG, "T_init is not finite");
  revo_map_align_opts o{30, 0, 1e-6, 1e-6, 12};
  if (opt) o = *opt;
  if (o.max_iters < 1) return fail(REVO_ERR_INVALID_ARG, "max_iters must be >= 1");
  MapAlignCall c;
  { const int rc = align_begin(&c, dst, src, prm, 1); if (rc) return rc; }
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
  { const int rc = normals_check(&p); if (rc) return rc; }
  MapStats st;
  { const int rc = read_stats(m, &st); if (rc) return rc; }
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t nv = std::max<size_t>((size_t)st.occ, 1), slots = m->cap;
  // per slot: mean, normal, lambda; per voxel: key and the same three rows, compacted; the two counters
  const size_t o_cnt = 0, o_mean = 256, o_norm = o_mean + 16 * slots, o_lam = o_norm + 16 * slots, o_key = o_lam + 16 * slots,
               o_xm = o_key + 16 * ((8 * nv + 15) / 16), o_xn = o_xm + 16 * nv, o_xl = o_xn + 16 * nv, total = o_xl + 16 * nv;
  char* buf = nullptr;
  HIPCHECK(hipMalloc((void**)&buf, total));
  struct Free { char* p; ~Free() { hipFree(p); } } fr{buf};
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
  { const int rc = align_check(dst, src, prm); if (rc) return rc; }
  if (!T || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n < 1 || n > 65535) return fail(REVO_ERR_INVALID_ARG, "revo_map_align_plane_eval: n must be 1 .. 65535");
  if (device_out != 0 && device_out != 1) return fail(REVO_ERR_INVALID_ARG, "device_out must be 0 or 1");
  if (device_out && ((uintptr_t)out & 15)) return fail(REVO_ERR_INVALID_ARG, "the device output is not 16-byte aligned");
  revo_map_normals_params np;
  { const int rc = plane_params(prm, nprm, &np); if (rc) return rc; }
  MapAlignCall c;
  { const int rc = align_begin(&c, dst, src, prm, n, &np); if (rc) return rc; }
  { const int rc = align_launch(&c, n, T, device_out ? out : nullptr); if (rc) return rc; }
  hipStream_t s = (hipStream_t)dst->g.stream;
  if (!device_out) HIPCHECK(hipMemcpyAsync(out, c.d_out, sizeof(revo_map_plane_info) * n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
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
  { const int rc = align_check(dst, src, prm); if (rc) return rc; }
  if (!T_init || !T_out || !status) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!pose_finite(T_init)) return fail(REVO_ERR_INVALID_ARG, "T_init is not finite");
  revo_map_align_opts o{30, 0, 1e-6, 1e-6, 12};
  if (opt) o = *opt;
  if (o.max_iters < 1) return fail(REVO_ERR_INVALID_ARG, "max_iters must be >= 1");
  revo_map_normals_params np;
  { const int rc = plane_params(prm, nprm, &np); if (rc) return rc; }
  MapAlignCall c;
  { const int rc = align_begin(&c, dst, src, prm, 1, &np); if (rc) return rc; }
  int32_t it = 0;
  const int rc = align_loop_over<revo_map_plane_info>(T_init, prm->centre, o, align_plane_system_fill,
                                                      [&](const float* Tf, revo_map_plane_info* rec) { return align_eval_host(&c, Tf, rec); },
                                                      T_out, info_out, &it, status);
  if (rc) return rc;
  if (iterations) *iterations = it;
  return REVO_OK;
}

// ------------------------------------------------------------------------------------------- maps under a pose (18) --
// revo_map_pose_raw / revo_map_merge_posed / revo_map_subtract_posed (contract: include/revo_hip.h).
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
  key = ((u64)(kx + (1 << 20)) << 42) | ((u64)(ky + (1 << 20)) << 21) | (u64)(kz + (1 << 20));
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
  ulonglong2 r0{}, r1{}, r2{}, r3{};  // key n | qx qy | qz sb | sg sr
  int what = -1;
  if (skey != MAP_EMPTY) {
    const ulonglong2* v = (const ulonglong2*)(a.vals + i);
    const ulonglong2 p = v[0], q = v[1], c = v[2], d = v[3];  // n qx | qy qz | sb sg | sr -
    if (p.x != 0) {  // a committed voxel has count >= 1
      u64 key = 0, qx = 0, qy = 0, qz = 0;
      what = map_posed_record(p.x, p.y, q.x, q.y, a.T, a.min_count, key, qx, qy, qz);
      r0 = make_ulonglong2(key, p.x); r1 = make_ulonglong2(qx, qy); r2 = make_ulonglong2(qz, c.x); r3 = make_ulonglong2(c.y, d.x);
      if (what == POSED_BAD) {
        atomicOr(&s_bad, 1u);
      } else {
        atomicAdd(&s_vox[0], 1u);
        atomicAdd(&s_vox[1 + what], 1u);
        atomicAdd(&s_pts[what], p.x);
      }
    }
  }
  const bool sel = what == POSED_MOVED;
  const unsigned o = sel ? atomicAdd(&s_n, 1u) : 0u;
  __syncthreads();
  if (threadIdx.x == 0) s_base = s_n ? (unsigned)atomicAdd(&a.info[1], (u64)s_n) : 0u;  // voxels_moved doubles as the compaction's counter
  if (threadIdx.x == 1 && s_vox[0]) atomicAdd(&a.info[0], (u64)s_vox[0]);
  if ((threadIdx.x == 2 || threadIdx.x == 3) && s_vox[threadIdx.x]) atomicAdd(&a.info[threadIdx.x], (u64)s_vox[threadIdx.x]);
  if (threadIdx.x >= 4 && threadIdx.x < 7 && s_pts[threadIdx.x - 4]) atomicAdd(&a.info[threadIdx.x], s_pts[threadIdx.x - 4]);
  if (threadIdx.x == 7 && s_bad) atomicOr(&a.info[7], 1ull);
  __syncthreads();
  if (!sel) return;
  const unsigned j = s_base + o;
  if (j >= a.cap_out) return;
  ulonglong2* r = a.out + 4 * (size_t)j;
  r[0] = r0; r[1] = r1; r[2] = r2; r[3] = r3;
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
  char* buf = nullptr;
  revo_map_pose_info info{};
  ~MapPoseRun() { (void)hipFree(buf); (void)hipGetLastError(); }
  const ulonglong2* recs() const { return (const ulonglong2*)(buf + 256); }
};
static int pose_run(MapPoseRun* r, revo_map* src, hipStream_t s, size_t voxels, const float* T, float voxel_dst, size_t min_count,
                    ulonglong2* d_out, size_t cap_out, bool own) {
  const size_t room = own ? std::max<size_t>(voxels, 1) : 0;
  if (!r->buf) HIPCHECK(hipMalloc((void**)&r->buf, 256 + sizeof(revo_map_voxel_raw) * room));
  MapPoseK a{};
  a.keys = src->d_keys; a.vals = src->d_vals; a.cap = (unsigned)src->cap;
  a.min_count = (u64)std::max<size_t>(min_count, 1);
  a.T = MapPose{T[0], T[4], T[8], T[1], T[5], T[9], T[2], T[6], T[10], T[12], T[13], T[14], voxel_dst};
  a.out = own ? (ulonglong2*)(r->buf + 256) : d_out;
  a.cap_out = (unsigned)std::min<size_t>(own ? room : cap_out, MAP_MAX_CAP);
  a.info = (u64*)r->buf;
  HIPCHECK(hipMemsetAsync(r->buf, 0, sizeof(revo_map_pose_info), s));
  hipLaunchKernelGGL(k_map_pose, dim3((unsigned)((src->cap + 255) / 256)), dim3(256), 0, s, a);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(&r->info, r->buf, sizeof(revo_map_pose_info), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  const bool bad = r->info.reserved != 0;
  r->info.reserved = 0;
  if (bad) return fail(REVO_ERR_INVALID_ARG, "voxel map: a source voxel has a count of 2^32 or more (nothing posed)");
  return REVO_OK;
}

extern "C" int revo_map_pose_raw(revo_map* src, const float T[16], float voxel_dst, size_t min_count, revo_map_voxel_raw* out, size_t cap,
                                 size_t* n, int device_out, revo_map_pose_info* info) {
  if (!src || !T || !n) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (device_out != 0 && device_out != 1) return fail(REVO_ERR_INVALID_ARG, "device_out must be 0 or 1");
  if (device_out && ((uintptr_t)out & 15)) return fail(REVO_ERR_INVALID_ARG, "the device output is not 16-byte aligned");
  { const int rc = pose_check(T, voxel_dst); if (rc) return rc; }
  MapStats ss;
  { const int rc = read_stats(src, &ss); if (rc) return rc; }
  hipStream_t s = (hipStream_t)src->g.stream;
  const size_t nv = (size_t)ss.occ;
  MapPoseRun r;
  if (device_out) {
    // nothing may be written when cap is too small or a source voxel is a bad record: count first, then write
    { const int rc = pose_run(&r, src, s, nv, T, voxel_dst, min_count, nullptr, 0, false); if (rc) return rc; }
    *n = (size_t)r.info.voxels_moved;
    if (info) *info = r.info;
    if (!out) return REVO_OK;
    if (cap < *n) return fail(REVO_ERR_CAPACITY, "voxel map: the output holds fewer records than voxels move");
    if (!*n) return REVO_OK;
    return pose_run(&r, src, s, nv, T, voxel_dst, min_count, (ulonglong2*)out, cap, false);
  }
  { const int rc = pose_run(&r, src, s, nv, T, voxel_dst, min_count, nullptr, 0, true); if (rc) return rc; }
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
// stream, then merge_core or subtract_core over them with src's counters plus the drops of the move.
static int posed_apply(revo_map* dst, revo_map* src, const float* T, size_t min_count, revo_map_pose_info* info, bool subtract) {
  if (!dst || !src || !T) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (dst == src) return fail(REVO_ERR_INVALID_ARG, "a map cannot be posed into itself");
  if (dst->g.device != src->g.device) return fail(REVO_ERR_INVALID_ARG, "the maps are on different devices");
  { const int rc = pose_check(T, dst->voxel); if (rc) return rc; }
  MapStats ss;  // waits for src: its table is complete, and its counters say what comes
  { const int rc = read_stats(src, &ss); if (rc) return rc; }
  if (ss.kfs > 0x7fffffffull) return fail(REVO_ERR_INVALID_ARG, "the source map's keyframe count does not fit");
  HIPCHECK(hipSetDevice(dst->g.device));
  hipStream_t s = (hipStream_t)dst->g.stream;
  MapPoseRun r;
  { const int rc = pose_run(&r, src, s, (size_t)ss.occ, T, dst->voxel, min_count, nullptr, 0, true); if (rc) return rc; }
  if (info) *info = r.info;
  const size_t moved = (size_t)r.info.voxels_moved;
  if (!moved) return REVO_OK;  // as revo_map_merge_raw / revo_map_subtract_raw with n == 0
  MapMergeK a{};
  a.recs = r.recs();
  a.n = (unsigned)moved;
  a.dropped = ss.drop + r.info.points_dropped;
  if (subtract) return subtract_core(dst, a, MERGE_RAW, a.dropped, ss.kfs);  // has waited: the records are read
  // device-made records need no validation: the device decides only when max_voxels is in reach
  const int rc = merge_core(dst, a, MERGE_RAW, moved, true, (int)ss.kfs);
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
struct MapCarveView {  // one view of a launch, in device memory
  CarveView v;
  const float* depth;
};
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
enum { CARVE_OUTSIDE = 0, CARVE_UNKNOWN = 1, CARVE_FREE = 2, CARVE_CONFIRMED = 3, CARVE_OCCLUDED = 4, CARVE_EDGE = 5, CARVE_CLASSES = 6 };
#define CARVE_MAX_VIEWS 64

// The class of the point p in one view: the one text of the contract's rule.  Every read of the depth image lies inside a
// window that has been tested against the image size first, and |u|, |v| < 2^20 bounds the integers the test is made on.
__device__ __forceinline__ int map_carve_class(float px, float py, float pz, const MapCarveView& vw, int r, float margin, float margin_rel) {
  const CarveView& c = vw.v;
  const float x = ((c.Rc[0] * px + c.Rc[1] * py) + c.Rc[2] * pz) + c.tc[0];
  const float y = ((c.Rc[3] * px + c.Rc[4] * py) + c.Rc[5] * pz) + c.tc[1];
  const float z = ((c.Rc[6] * px + c.Rc[7] * py) + c.Rc[8] * pz) + c.tc[2];
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
  if (fabsf(z - dc) <= mc) return CARVE_CONFIRMED;
  return z > dc + mc ? CARVE_OCCLUDED : CARVE_EDGE;
}

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
  ulonglong2 p{}, q{}, c{}, d{};  // n qx | qy qz | sb sg | sr -
  bool cand = false;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (key != MAP_EMPTY) {
    const ulonglong2* v = (const ulonglong2*)(a.vals + i);
    p = v[0]; q = v[1]; c = v[2]; d = v[3];
    cand = p.x >= a.min_count && (a.max_count == 0 || p.x <= a.max_count);  // min_count >= 1: a committed voxel
    if (cand) {
      const double inv = (double)p.x;
      px = map_mean(p.y, inv); py = map_mean(q.x, inv); pz = map_mean(q.y, inv);
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
  if (sel) atomicAdd(&s_pts, p.x);
  const unsigned o = sel ? atomicAdd(&s_n, 1u) : 0u;
  __syncthreads();
  if (threadIdx.x == 0) s_base = s_n ? (unsigned)atomicAdd(&a.info[1], (u64)s_n) : 0u;  // voxels_carved doubles as the compaction's counter
  if (threadIdx.x == 1 && s_cand) atomicAdd(&a.info[0], (u64)s_cand);
  if (threadIdx.x == 2 && s_pts) atomicAdd(&a.info[2], s_pts);
  if (threadIdx.x == 3 && s_votes) atomicAdd(&a.info[3], (u64)s_votes);
  for (int k = threadIdx.x; k < a.n * CARVE_CLASSES; k += 256)
    if (s_cls[k]) atomicAdd(&a.vinfo[(k / CARVE_CLASSES) * 8 + k % CARVE_CLASSES], s_cls[k]);
  __syncthreads();
  if (!sel) return;
  const unsigned j = s_base + o;
  if (j >= a.cap_out) return;
  ulonglong2* r = a.out + 4 * (size_t)j;
  r[0] = make_ulonglong2(key, p.x); r[1] = make_ulonglong2(p.y, q.x); r[2] = make_ulonglong2(q.y, c.x); r[3] = make_ulonglong2(c.y, d.x);
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
  char* buf = nullptr;      // [0, 64) the info line, [256, 256 + 32 n) the views' counters, then the descriptors
  char* images = nullptr;   // host depth images of the call, uploaded
  char* recs = nullptr;     // the carved records of a host-output call or of revo_map_carve
  ~MapCarveRun() { (void)hipFree(buf); (void)hipFree(images); (void)hipFree(recs); (void)hipGetLastError(); }
};

static int carve_launch(revo_map* m, hipStream_t s, MapCarveRun* r, MapCarveK a, revo_map_carve_info* info, revo_map_carve_view_info* vinfo) {
  a.info = (u64*)r->buf;
  a.vinfo = (unsigned*)(r->buf + 256);
  HIPCHECK(hipMemsetAsync(r->buf, 0, 256 + sizeof(revo_map_carve_view_info) * a.n, s));
  hipLaunchKernelGGL(k_map_carve, dim3((unsigned)((m->cap + 255) / 256)), dim3(256), 0, s, a);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(info, r->buf, sizeof(revo_map_carve_info), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(vinfo, r->buf + 256, sizeof(revo_map_carve_view_info) * a.n, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

static int carve_apply(revo_map* m, int n, const revo_map_carve_view* views, int device_in, const revo_map_carve_params* prm,
                       revo_map_voxel_raw* records, size_t cap, size_t* n_records, int device_out, revo_map_carve_info* info,
                       revo_map_carve_view_info* view_info, bool remove) {
  if (!m || !views || !n_records) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n < 1 || n > CARVE_MAX_VIEWS) return fail(REVO_ERR_INVALID_ARG, "revo_map_carve: n must be 1 .. 64 views");
  if (device_in != 0 && device_in != 1) return fail(REVO_ERR_INVALID_ARG, "device_in must be 0 or 1");
  if (device_out != 0 && device_out != 1) return fail(REVO_ERR_INVALID_ARG, "device_out must be 0 or 1");
  if (device_out && ((uintptr_t)records & 15)) return fail(REVO_ERR_INVALID_ARG, "the device output is not 16-byte aligned");
  revo_map_carve_params pp;
  if (const char* why = carve_params_check(prm, m->voxel, &pp)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_carve: ") + why);
  const CarveCam cam{m->g.fx, m->g.fy, m->g.cx, m->g.cy, m->g.dmin, m->g.dmax};
  std::vector<MapCarveView> hv(n);
  size_t up_bytes = 0;
  for (int i = 0; i < n; ++i) {
    const std::string at = "view " + std::to_string(i) + ": ";
    if (const char* why = carve_view_check(&views[i], cam, m->g.w, m->g.h, &hv[i].v)) return fail(REVO_ERR_INVALID_ARG, at + why);
    hv[i].depth = views[i].depth;
    if (views[i].depth) {
      if (device_in && ((uintptr_t)views[i].depth & 3)) return fail(REVO_ERR_INVALID_ARG, at + "the device depth image is not 4-byte aligned");
      if (!device_in) up_bytes += ((size_t)hv[i].v.w * hv[i].v.h * sizeof(float) + 255) & ~(size_t)255;
    }
  }
  for (int i = 0; i < n; ++i) {  // every pyramid's context and kind, before any of them orders a stream
    if (!views[i].kf) continue;
    const revo_ctx* pc = nullptr;
    int batch_view = 0;
    { const int rc = revo_map_source_kind_(views[i].kf, &pc, &batch_view); if (rc) return rc; }
    const std::string at = "view " + std::to_string(i) + ": ";
    if (pc != m->ctx) return fail(REVO_ERR_INVALID_ARG, at + "the pyramid belongs to another context than the map");
    if (batch_view)
      return fail(REVO_ERR_INVALID_ARG, at + "a batch view is not a keyframe the map calls take (pass its depth plane as a raw image)");
  }
  for (int i = 0; i < n; ++i) {  // nothing is refused from here on: the tracker stream is ordered behind the pyramids' builds
    if (!views[i].kf) continue;
    MapSource src;
    { const int rc = revo_map_source_(const_cast<revo_pyr*>(views[i].kf), &src); if (rc) return rc; }
    hv[i].depth = src.depth;
  }
  MapStats st;  // waits for the map: its table is complete
  { const int rc = read_stats(m, &st); if (rc) return rc; }
  hipStream_t s = (hipStream_t)m->g.stream;
  MapCarveRun r;
  const size_t o_views = 256 + ((sizeof(revo_map_carve_view_info) * n + 255) & ~(size_t)255);
  HIPCHECK(hipMalloc((void**)&r.buf, o_views + sizeof(MapCarveView) * n));
  if (up_bytes) {
    HIPCHECK(hipMalloc((void**)&r.images, up_bytes));
    size_t o = 0;
    for (int i = 0; i < n; ++i) {
      if (!views[i].depth) continue;
      const size_t bytes = (size_t)hv[i].v.w * hv[i].v.h * sizeof(float);
      HIPCHECK(hipMemcpyAsync(r.images + o, views[i].depth, bytes, hipMemcpyHostToDevice, s));
      hv[i].depth = (const float*)(r.images + o);
      o += (bytes + 255) & ~(size_t)255;
    }
  }
  HIPCHECK(hipMemcpyAsync(r.buf + o_views, hv.data(), sizeof(MapCarveView) * n, hipMemcpyHostToDevice, s));
  MapCarveK a{};
  a.keys = m->d_keys; a.vals = m->d_vals; a.cap = (unsigned)m->cap;
  a.views = (const MapCarveView*)(r.buf + o_views); a.n = n;
  a.radius = pp.radius; a.min_views = pp.min_views;
  a.min_count = pp.min_count; a.max_count = pp.max_count;
  a.margin = pp.margin; a.margin_rel = pp.margin_rel;
  revo_map_carve_info ci{};
  std::vector<revo_map_carve_view_info> vi(n);
  // nothing may be written when cap is too small: count first, then write (carve_launch waits, so hv and the images are read)
  { const int rc = carve_launch(m, s, &r, a, &ci, vi.data()); if (rc) return rc; }
  const size_t carved = (size_t)ci.voxels_carved;
  *n_records = carved;
  if (info) *info = ci;
  if (view_info) memcpy(view_info, vi.data(), sizeof(revo_map_carve_view_info) * n);
  if (records && cap < carved) return fail(REVO_ERR_CAPACITY, "voxel map: the output holds fewer records than voxels are carved");
  if (!carved || (!records && !remove)) return REVO_OK;
  ulonglong2* d_rec = (ulonglong2*)records;
  if (!records || !device_out) {
    HIPCHECK(hipMalloc((void**)&r.recs, sizeof(revo_map_voxel_raw) * carved));
    d_rec = (ulonglong2*)r.recs;
  }
  a.out = d_rec; a.cap_out = (unsigned)carved;
  revo_map_carve_info ci2{};
  { const int rc = carve_launch(m, s, &r, a, &ci2, vi.data()); if (rc) return rc; }
  if (ci2.voxels_carved != ci.voxels_carved) return fail(REVO_ERR_HIP, "voxel map: two carve launches over one table disagree");
  if (remove) {
    MapMergeK sub{};
    sub.recs = d_rec;
    sub.n = (unsigned)carved;
    const int rc = subtract_core(m, sub, MERGE_RAW, 0, 0);  // has waited: the records are read
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

// --------------------------------------------------------------------------------------------- rays through the map (20) --
// revo_map_raycast / revo_map_cast_rays (contract: include/revo_hip.h).
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
struct MapRayOut { u64 key; float s; unsigned cells; float z; unsigned bgr; };  // z, bgr (B | G << 8 | R << 16): view rays only
enum { RAY_HIT = 0, RAY_RANGE = 1, RAY_OUTSIDE = 2, RAY_EXHAUSTED = 3, RAY_STATUSES = 4 };

__device__ __forceinline__ u64 map_ray_key(int kx, int ky, int kz) {
  return ((u64)(kx + (1 << 20)) << 42) | ((u64)(ky + (1 << 20)) << 21) | (u64)(kz + (1 << 20));
}
// step, pos and the first crossing parameter of one axis
__device__ __forceinline__ void map_ray_axis(float o, float d, int k, float voxel, int& step, int& pos, float& inv, float& t) {
  inv = __fdiv_rn(1.0f, d);
  step = d > 0.0f ? 1 : (d < 0.0f ? -1 : 0);
  pos = d > 0.0f ? 1 : 0;
  if (!isfinite(inv)) step = 0;
  t = step ? ((float)(k + pos) * voxel - o) * inv : INFINITY;
}

// The one text of the contract's march.  VIEW: the voxel must also lie in the view's depth range (vw's Rc, tc, zmin, zmax).
// The axis choice is written with selects on scalars: no private array is indexed at run time.  The block table only decides
// whether the fine table is asked; the stepping does not know of it.
template <bool VIEW>
__device__ __forceinline__ int map_ray_march(const MapRayK& a, const RayView* vw, float ox, float oy, float oz, float s0, float dx,
                                             float dy, float dz, float s1, MapRayOut& out) {
  out.key = MAP_EMPTY; out.s = 0.0f; out.cells = 0; out.z = 0.0f; out.bgr = 0;
  const float gx = ox + s0 * dx, gy = oy + s0 * dy, gz = oz + s0 * dz;
  const float fx = floorf(__fdiv_rn(gx, a.voxel)), fy = floorf(__fdiv_rn(gy, a.voxel)), fz = floorf(__fdiv_rn(gz, a.voxel));
  if (!(s0 < s1) || !isfinite(s1) || !isfinite(gx) || !isfinite(gy) || !isfinite(gz)) return RAY_OUTSIDE;
  if (!(fx >= -1048576.0f && fx <= 1048575.0f && fy >= -1048576.0f && fy <= 1048575.0f && fz >= -1048576.0f && fz <= 1048575.0f))
    return RAY_OUTSIDE;
  int kx = (int)fx, ky = (int)fy, kz = (int)fz;
  int stx, sty, stz, psx, psy, psz;
  float ivx, ivy, ivz, tx, ty, tz;
  map_ray_axis(ox, dx, kx, a.voxel, stx, psx, ivx, tx);
  map_ray_axis(oy, dy, ky, a.voxel, sty, psy, ivy, ty);
  map_ray_axis(oz, dz, kz, a.voxel, stz, psz, ivz, tz);
  float s = s0;
  unsigned cells = 0;
  u64 last_block = MAP_EMPTY;  // no block key reaches it
  bool block_occupied = true;
  for (;;) {
    if (cells == a.max_steps) { out.cells = cells; return RAY_EXHAUSTED; }
    ++cells;
    out.s = s;
    const u64 key = map_ray_key(kx, ky, kz);
    if (a.bkeys) {
      const u64 bk = map_ray_key(kx >> 3, ky >> 3, kz >> 3);  // map_coarse_key(key, 3)
      if (bk != last_block) { last_block = bk; block_occupied = map_find(a.bkeys, a.bmask, bk) != ~0u; }
    }
    if (block_occupied) {
      const unsigned slot = map_find(a.keys, a.mask, key);
      if (slot != ~0u) {
        const ulonglong2* v = (const ulonglong2*)(a.vals + slot);
        const ulonglong2 p = v[0];  // n qx
        if (p.x >= a.min_count) {
          bool solid = true;
          if (VIEW) {
            const ulonglong2 q = v[1], c = v[2], e = v[3];  // qy qz | sb sg | sr -
            const double inv = (double)p.x;
            const float px = map_mean(p.y, inv), py = map_mean(q.x, inv), pz = map_mean(q.y, inv);
            const float x = ((vw->Rc[0] * px + vw->Rc[1] * py) + vw->Rc[2] * pz) + vw->tc[0];
            const float y = ((vw->Rc[3] * px + vw->Rc[4] * py) + vw->Rc[5] * pz) + vw->tc[1];
            const float z = ((vw->Rc[6] * px + vw->Rc[7] * py) + vw->Rc[8] * pz) + vw->tc[2];
            solid = isfinite(x) && isfinite(y) && map_depth_ok(z, vw->zmin, vw->zmax);
            if (solid) {
              const u64 h = p.x / 2;
              out.z = z;
              out.bgr = (unsigned)((c.x + h) / p.x) | ((unsigned)((c.y + h) / p.x) << 8) | ((unsigned)((e.x + h) / p.x) << 16);
            }
          }
          if (solid) { out.key = key; out.cells = cells; return RAY_HIT; }
        }
      }
    }
    int ax = 0;
    float sn = tx;
    if (ty < sn) { ax = 1; sn = ty; }
    if (tz < sn) { ax = 2; sn = tz; }
    if (!(sn < s1)) { out.cells = cells; return RAY_RANGE; }
    const int kn = (ax == 0 ? kx + stx : (ax == 1 ? ky + sty : kz + stz));
    if (kn < -(1 << 20) || kn > (1 << 20) - 1) { out.cells = cells; return RAY_OUTSIDE; }
    const int pn = kn + (ax == 0 ? psx : (ax == 1 ? psy : psz));
    const float tn = ((float)pn * a.voxel - (ax == 0 ? ox : (ax == 1 ? oy : oz))) * (ax == 0 ? ivx : (ax == 1 ? ivy : ivz));
    s = sn;
    if (ax == 0) { kx = kn; tx = tn; } else if (ax == 1) { ky = kn; ty = tn; } else { kz = kn; tz = tn; }
  }
}

// One thread per slot of the table: the key of the 8 x 8 x 8 block around every voxel with count >= min_count goes into a
// keys-only table of as many slots (a block holds at least one voxel, so its load is at most the map's).
__global__ void __launch_bounds__(256) k_map_ray_blocks(const u64* __restrict__ keys, const MapVal* __restrict__ vals, unsigned cap,
                                                        u64 min_count, u64* bkeys, unsigned bmask, u64* fault) {
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cap) return;
  const u64 key = keys[i];
  if (key == MAP_EMPTY || vals[i].n < min_count) return;
  map_slot<true>(bkeys, bmask, map_coarse_key(key, 3), nullptr, fault);
}

// The statuses and cells of a block's rays: ballots per wave into LDS, then one global atomic per counter.  Every thread of
// the block calls it (status < 0: no ray).
__device__ __forceinline__ void map_ray_count(const MapRayK& a, int status, unsigned cells, unsigned* s_cnt, u64* s_cells, unsigned* hits) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < RAY_STATUSES; ++k) {
    const u64 b = __ballot(status == k);
    if (lane == 0 && b) atomicAdd(&s_cnt[k], (unsigned)__popcll(b));
  }
  unsigned c = status < 0 ? 0u : cells;  // <= 2^20 per ray: a wave's sum fits
#pragma unroll
  for (int off = 32; off; off >>= 1) c += __shfl_down(c, off, 64);
  if (lane == 0 && c) atomicAdd(s_cells, (u64)c);
  __syncthreads();
  if (threadIdx.x < RAY_STATUSES && s_cnt[threadIdx.x]) atomicAdd(&a.info[1 + threadIdx.x], (u64)s_cnt[threadIdx.x]);
  if (threadIdx.x == 4 && *s_cells) atomicAdd(&a.info[5], *s_cells);
  if (threadIdx.x == 5) {
    const unsigned rays = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (rays) atomicAdd(&a.info[0], (u64)rays);
  }
  if (threadIdx.x == 6 && hits && s_cnt[RAY_HIT]) atomicAdd(hits, s_cnt[RAY_HIT]);
}

// One thread per pixel, blockIdx.y = view.  A wave is an 8 x 8 pixel tile (its rays end after similar numbers of steps), a
// block four tiles side by side; blocks past a view's tiles leave at once.
__global__ void __launch_bounds__(256) k_map_raycast(const MapRayK a, const MapRayView* __restrict__ views) {
  __shared__ unsigned s_cnt[RAY_STATUSES];
  __shared__ u64 s_cells;
  const MapRayView& vw = views[blockIdx.y];
  const RayView& c = vw.v;
  const unsigned bw = (unsigned)(c.w + 31) / 32, bh = (unsigned)(c.h + 7) / 8;
  if (blockIdx.x >= bw * bh) return;
  if (threadIdx.x < RAY_STATUSES) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 4) s_cells = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int x = (int)((blockIdx.x % bw) * 32 + (threadIdx.x >> 6) * 8 + (lane & 7));
  const int y = (int)((blockIdx.x / bw) * 8 + (lane >> 3));
  int status = -1;
  MapRayOut o{};
  if (x < c.w && y < c.h) {
    const float dcx = __fdiv_rn((float)x - c.cx, c.fx), dcy = __fdiv_rn((float)y - c.cy, c.fy);
    const float dx = ((c.R[0] * dcx) + (c.R[1] * dcy)) + c.R[2];
    const float dy = ((c.R[3] * dcx) + (c.R[4] * dcy)) + c.R[5];
    const float dz = ((c.R[6] * dcx) + (c.R[7] * dcy)) + c.R[8];
    status = map_ray_march<true>(a, &c, c.o[0], c.o[1], c.o[2], c.zmin, dx, dy, dz, c.zmax, o);
    const size_t p = (size_t)y * c.w + x;
    vw.depth[p] = o.z;  // 0 unless a hit
    if (vw.bgr) {
      uint8_t* b = vw.bgr + p * 3;
      b[0] = (uint8_t)o.bgr; b[1] = (uint8_t)(o.bgr >> 8); b[2] = (uint8_t)(o.bgr >> 16);
    }
    if (vw.key) vw.key[p] = o.key;
  }
  map_ray_count(a, status, o.cells, s_cnt, &s_cells, vw.hits);
}

// One thread per given ray: two 16-byte loads, the march, one 16-byte store.
__global__ void __launch_bounds__(256) k_map_cast_rays(const MapRayK a, const float4* __restrict__ rays, unsigned n, ulonglong2* out) {
  __shared__ unsigned s_cnt[RAY_STATUSES];
  __shared__ u64 s_cells;
  if (threadIdx.x < RAY_STATUSES) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 4) s_cells = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  int status = -1;
  MapRayOut o{};
  if (i < n) {
    const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];  // o s0 | d s1
    status = map_ray_march<false>(a, nullptr, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, o);
    out[i] = make_ulonglong2(o.key, (u64)__float_as_uint(o.s) | ((u64)(o.cells | ((unsigned)status << 30)) << 32));
  }
  map_ray_count(a, status, o.cells, s_cnt, &s_cells, nullptr);
}

static_assert(sizeof(revo_map_ray_params) == 16 && offsetof(revo_map_ray_params, max_steps) == 0 && offsetof(revo_map_ray_params, reserved) == 4,
              "the parameter record is the documented layout");
static_assert(sizeof(revo_map_ray) == 32 && offsetof(revo_map_ray, o) == 0 && offsetof(revo_map_ray, s0) == 12 &&
              offsetof(revo_map_ray, d) == 16 && offsetof(revo_map_ray, s1) == 28, "a ray is the kernel's two 16-byte words");
static_assert(sizeof(revo_map_ray_hit) == 16 && offsetof(revo_map_ray_hit, key) == 0 && offsetof(revo_map_ray_hit, s) == 8 &&
              offsetof(revo_map_ray_hit, cells) == 12, "a ray's result is the kernel's one 16-byte word");
static_assert(sizeof(revo_map_ray_info) == 64 && offsetof(revo_map_ray_info, rays) == 0 && offsetof(revo_map_ray_info, hits) == 8 * (1 + RAY_HIT) &&
              offsetof(revo_map_ray_info, range) == 8 * (1 + RAY_RANGE) && offsetof(revo_map_ray_info, outside) == 8 * (1 + RAY_OUTSIDE) &&
              offsetof(revo_map_ray_info, exhausted) == 8 * (1 + RAY_EXHAUSTED) && offsetof(revo_map_ray_info, cells) == 40 &&
              offsetof(revo_map_ray_info, reserved) == 48, "the info record is the kernel's counter line");
static_assert(REVO_RAY_HIT == RAY_HIT && REVO_RAY_RANGE == RAY_RANGE && REVO_RAY_OUTSIDE == RAY_OUTSIDE && REVO_RAY_EXHAUSTED == RAY_EXHAUSTED,
              "the header's statuses are the kernel's");

// Room for a call: the block table (as many slots as the map's table), the counter lines, the views' descriptors (pinned +
// device), the device outputs of a host-output call.
static int ray_reserve(revo_map* m, int n_views, size_t out_bytes) {
  hipStream_t s = (hipStream_t)m->g.stream;
  if (!m->ev_rviews) {
    HIPCHECK(hipEventCreateWithFlags(&m->ev_rviews, hipEventDisableTiming));
    HIPCHECK(hipEventCreate(&m->ev_c0));
    HIPCHECK(hipEventCreate(&m->ev_c1));
    HIPCHECK(hipMalloc((void**)&m->d_rcnt, 512));  // [0, 64) the info line, [64, 64 + 4 x 64) the views' hits
  }
  if (m->rviews_recorded) HIPCHECK(hipEventSynchronize(m->ev_rviews));  // the previous upload has read the pinned rows
  if (n_views > m->cap_rviews) {
    HIPCHECK(hipStreamSynchronize(s));  // the previous call's kernel reads the descriptors
    (void)hipHostFree(m->h_rviews); (void)hipFree(m->d_rviews);
    m->h_rviews = nullptr; m->d_rviews = nullptr; m->cap_rviews = 0;
    HIPCHECK(hipHostMalloc((void**)&m->h_rviews, sizeof(MapRayView) * n_views));
    HIPCHECK(hipMalloc((void**)&m->d_rviews, sizeof(MapRayView) * n_views));
    m->cap_rviews = n_views;
  }
  if (m->cap > m->bcap) {
    HIPCHECK(hipStreamSynchronize(s));
    (void)hipFree(m->d_bkeys);
    m->d_bkeys = nullptr; m->bcap = 0;
    HIPCHECK(hipMalloc((void**)&m->d_bkeys, sizeof(u64) * m->cap));
    m->bcap = m->cap;
  }
  if (out_bytes > m->rout_bytes) {
    HIPCHECK(hipStreamSynchronize(s));
    (void)hipFree(m->d_rout);
    m->d_rout = nullptr; m->rout_bytes = 0;
    HIPCHECK(hipMalloc((void**)&m->d_rout, out_bytes));
    m->rout_bytes = out_bytes;
  }
  return REVO_OK;
}

// What both entry points share: the first event, the block table of the map as it is on the stream, the cleared counters.
// REVO_MAP_RAYCAST_BLOCKS=0: no block table, every cell is looked up (the exactness test and profiles/map_raycast_rates.py).
static int ray_begin(revo_map* m, MapRayK* a, u64 min_count, unsigned max_steps, u64* d_info, unsigned* d_hits, int n_hits) {
  hipStream_t s = (hipStream_t)m->g.stream;
  a->keys = m->d_keys; a->vals = m->d_vals; a->mask = (unsigned)(m->cap - 1);
  a->min_count = min_count; a->max_steps = max_steps; a->voxel = m->voxel;
  a->info = d_info;
  HIPCHECK(hipEventRecord(m->ev_c0, s));
  a->bkeys = nullptr; a->bmask = 0;
  if (env_int("REVO_MAP_RAYCAST_BLOCKS", 1, 0, 1)) {
    HIPCHECK(hipMemsetAsync(m->d_bkeys, 0xff, sizeof(u64) * m->cap, s));
    hipLaunchKernelGGL(k_map_ray_blocks, dim3((unsigned)((m->cap + 255) / 256)), dim3(256), 0, s, m->d_keys, m->d_vals, (unsigned)m->cap,
                       min_count, m->d_bkeys, (unsigned)(m->cap - 1), &m->d_st->fault);
    HIPCHECK(hipGetLastError());
    a->bkeys = m->d_bkeys; a->bmask = (unsigned)(m->cap - 1);
  }
  HIPCHECK(hipMemsetAsync(d_info, 0, sizeof(revo_map_ray_info), s));
  if (n_hits) HIPCHECK(hipMemsetAsync(d_hits, 0, sizeof(unsigned) * n_hits, s));
  return REVO_OK;
}

extern "C" int revo_map_raycast(revo_map* m, int n, const revo_map_view* views, const revo_map_ray_params* prm, float* const* depth,
                                uint8_t* const* bgr, uint64_t* const* key, uint32_t* hits, int device_out, revo_map_ray_info* info) {
  if (!m || !views || !depth) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n < 1 || n > RAY_MAX_VIEWS) return fail(REVO_ERR_INVALID_ARG, "revo_map_raycast: n must be 1 .. 64 views");
  if (device_out != 0 && device_out != 1) return fail(REVO_ERR_INVALID_ARG, "device_out must be 0 or 1");
  if (device_out && (((uintptr_t)hits | (uintptr_t)info) & 15)) return fail(REVO_ERR_INVALID_ARG, "hits or info is not 16-byte aligned");
  uint32_t max_steps = 0;
  if (const char* why = ray_params_check(prm, &max_steps)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_raycast: ") + why);
  const CarveCam cam{m->g.fx, m->g.fy, m->g.cx, m->g.cy, m->g.dmin, m->g.dmax};
  std::vector<RayView> rv(n);
  size_t out_bytes = 0;
  int max_blocks = 0;
  for (int i = 0; i < n; ++i) {
    const std::string at = "view " + std::to_string(i) + ": ";
    if (!depth[i] || (bgr && !bgr[i]) || (key && !key[i])) return fail(REVO_ERR_INVALID_ARG, at + "null output");
    if (device_out && (((uintptr_t)depth[i] | (uintptr_t)(bgr ? bgr[i] : nullptr) | (uintptr_t)(key ? key[i] : nullptr)) & 15))
      return fail(REVO_ERR_INVALID_ARG, at + "a device output is not 16-byte aligned");
    if (const char* why = ray_view_check(&views[i], cam, &rv[i])) return fail(REVO_ERR_INVALID_ARG, at + why);
    const size_t np = (size_t)rv[i].w * rv[i].h;
    out_bytes += (np * (4 + (bgr ? 3 : 0) + (key ? 8 : 0)) + 15) & ~(size_t)15;
    max_blocks = std::max(max_blocks, ((rv[i].w + 31) / 32) * ((rv[i].h + 7) / 8));
  }
  const uint32_t min_count = ray_views_min_count(views, n);
  if (!min_count) return fail(REVO_ERR_INVALID_ARG, "revo_map_raycast: every view of a call must carry the same min_count");
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  { const int rc = ray_reserve(m, n, device_out ? 0 : out_bytes); if (rc) return rc; }
  u64* d_info = device_out && info ? (u64*)info : (u64*)m->d_rcnt;
  unsigned* d_hits = device_out && hits ? hits : (unsigned*)(m->d_rcnt + 64);
  size_t oo = 0;
  for (int i = 0; i < n; ++i) {
    MapRayView& d = m->h_rviews[i];
    d.v = rv[i];
    const size_t np = (size_t)rv[i].w * rv[i].h;
    if (device_out) {
      d.depth = depth[i]; d.bgr = bgr ? bgr[i] : nullptr; d.key = key ? (u64*)key[i] : nullptr;
    } else {  // keys, depth, colour: the widest first
      char* b = m->d_rout + oo;
      d.key = key ? (u64*)b : nullptr;
      b += key ? np * 8 : 0;
      d.depth = (float*)b;
      d.bgr = bgr ? (uint8_t*)(b + np * 4) : nullptr;
      oo += (np * (4 + (bgr ? 3 : 0) + (key ? 8 : 0)) + 15) & ~(size_t)15;
    }
    d.hits = d_hits + i;
  }
  HIPCHECK(hipMemcpyAsync(m->d_rviews, m->h_rviews, sizeof(MapRayView) * n, hipMemcpyHostToDevice, s));
  HIPCHECK(hipEventRecord(m->ev_rviews, s));
  m->rviews_recorded = true;
  MapRayK a{};
  { const int rc = ray_begin(m, &a, min_count, max_steps, d_info, d_hits, n); if (rc) return rc; }
  hipLaunchKernelGGL(k_map_raycast, dim3((unsigned)max_blocks, (unsigned)n), dim3(256), 0, s, a, m->d_rviews);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord(m->ev_c1, s));
  m->raycast = true;
  if (device_out) return REVO_OK;
  for (int i = 0; i < n; ++i) {
    const MapRayView& d = m->h_rviews[i];
    const size_t np = (size_t)rv[i].w * rv[i].h;
    HIPCHECK(hipMemcpyAsync(depth[i], d.depth, np * 4, hipMemcpyDeviceToHost, s));
    if (bgr) HIPCHECK(hipMemcpyAsync(bgr[i], d.bgr, np * 3, hipMemcpyDeviceToHost, s));
    if (key) HIPCHECK(hipMemcpyAsync(key[i], d.key, np * 8, hipMemcpyDeviceToHost, s));
  }
  if (hits) HIPCHECK(hipMemcpyAsync(hits, d_hits, sizeof(unsigned) * n, hipMemcpyDeviceToHost, s));
  if (info) HIPCHECK(hipMemcpyAsync(info, d_info, sizeof(revo_map_ray_info), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_cast_rays(revo_map* m, size_t n, const revo_map_ray* rays, int device_in, uint32_t min_count,
                                  const revo_map_ray_params* prm, revo_map_ray_hit* out, int device_out, revo_map_ray_info* info) {
  if (!m || !rays || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n < 1 || n > RAY_MAX_RAYS) return fail(REVO_ERR_INVALID_ARG, "revo_map_cast_rays: n must be 1 .. 2^24 rays");
  if (device_in != 0 && device_in != 1) return fail(REVO_ERR_INVALID_ARG, "device_in must be 0 or 1");
  if (device_out != 0 && device_out != 1) return fail(REVO_ERR_INVALID_ARG, "device_out must be 0 or 1");
  if (device_in && ((uintptr_t)rays & 15)) return fail(REVO_ERR_INVALID_ARG, "the device rays are not 16-byte aligned");
  if (device_out && (((uintptr_t)out | (uintptr_t)info) & 15)) return fail(REVO_ERR_INVALID_ARG, "a device output is not 16-byte aligned");
  uint32_t max_steps = 0;
  if (const char* why = ray_params_check(prm, &max_steps)) return fail(REVO_ERR_INVALID_ARG, std::string("revo_map_cast_rays: ") + why);
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  { const int rc = ray_reserve(m, 0, device_out ? 0 : sizeof(revo_map_ray_hit) * n); if (rc) return rc; }
  struct Upload { void* p = nullptr; ~Upload() { (void)hipFree(p); (void)hipGetLastError(); } } up;  // freed after the wait below
  const float4* d_rays = (const float4*)rays;
  if (!device_in) {
    HIPCHECK(hipMalloc(&up.p, sizeof(revo_map_ray) * n));
    HIPCHECK(hipMemcpyAsync(up.p, rays, sizeof(revo_map_ray) * n, hipMemcpyHostToDevice, s));
    d_rays = (const float4*)up.p;
  }
  u64* d_info = device_out && info ? (u64*)info : (u64*)m->d_rcnt;
  ulonglong2* d_out = device_out ? (ulonglong2*)out : (ulonglong2*)m->d_rout;
  MapRayK a{};
  { const int rc = ray_begin(m, &a, std::max<u64>(min_count, 1), max_steps, d_info, nullptr, 0); if (rc) { (void)hipStreamSynchronize(s); return rc; } }
  hipLaunchKernelGGL(k_map_cast_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, d_rays, (unsigned)n, d_out);
  if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(s); return fail(REVO_ERR_HIP, "k_map_cast_rays: the launch failed"); }
  HIPCHECK(hipEventRecord(m->ev_c1, s));
  m->raycast = true;
  if (!device_out) {
    HIPCHECK(hipMemcpyAsync(out, d_out, sizeof(revo_map_ray_hit) * n, hipMemcpyDeviceToHost, s));
    if (info) HIPCHECK(hipMemcpyAsync(info, d_info, sizeof(revo_map_ray_info), hipMemcpyDeviceToHost, s));
  }
  if (!device_out || !device_in) HIPCHECK(hipStreamSynchronize(s));
  return REVO_OK;
}

extern "C" int revo_map_raycast_last_ms(revo_map* m, float* ms) {
  if (!m || !ms) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!m->raycast) return fail(REVO_ERR_INVALID_ARG, "the map has cast nothing yet");
  HIPCHECK(hipSetDevice(m->g.device));
  HIPCHECK(hipEventSynchronize(m->ev_c1));
  HIPCHECK(hipEventElapsedTime(ms, m->ev_c0, m->ev_c1));
  return REVO_OK;
}
