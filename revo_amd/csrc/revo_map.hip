// revo_map.hip -- world-frame voxel map fused on the device from keyframe clouds (revo_map_* in include/revo_hip.h).
//
// The reference draws every keyframe's coloured cloud at its keyframe pose (gui/MapDrawer.cc, fed by system.cpp:162-168,
// 232-238).  Here each keyframe is integrated straight from its level-0 planes into an open-addressing hash of voxels:
//   * keys: the voxel index packed into 63 bits (21 bits per axis, biased by 2^20: map_key), inserted by a 64-bit
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
// This unit: the table, integration, commit / rollback / rehash, create / destroy / clear / info / extract, export, merge and
// subtract.  The views are in revo_map_view.hip, registration in revo_map_align.hip, posed maps and carving in
// revo_map_edit.hip; what they share is revo_map_impl.h.
#include "revo_map_impl.h"

struct MapGeomK { int w, npix; float fx, fy, cx, cy, dmin, dmax; };

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
        key = map_key(k[0], k[1], k[2]);
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
    if (MODE != MAP_INSERT && s != ~0u)
      map_rec_add(d.vals + s, MapRec{make_ulonglong2(key, n), make_ulonglong2((u64)qx, (u64)qy), make_ulonglong2((u64)qz, cb), make_ulonglong2(cg, cr)});
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
  const unsigned j = map_compact(sel, s_n, s_base, total);
  if (!sel) return;
  const double inv = (double)v.n;
  okey[j] = key;
  oxyz[3 * j + 0] = map_mean(v.qx, inv);
  oxyz[3 * j + 1] = map_mean(v.qy, inv);
  oxyz[3 * j + 2] = map_mean(v.qz, inv);
  orgb[j] = map_colour_rgb(v.n, v.sb, v.sg, v.sr);
  ocount[j] = (unsigned)v.n;
}

// ------------------------------------------------------------------------------------------------- the map as data (13) --
// Occupied slots as raw records, compacted in arrival order (the host sorts by key); at most cap_out are written.
__global__ void __launch_bounds__(256) k_map_export(const u64* __restrict__ keys, const MapVal* __restrict__ vals, unsigned cap,
                                                    unsigned* total, ulonglong2* out, unsigned cap_out) {
  __shared__ unsigned s_n, s_base;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const unsigned i = blockIdx.x * 256 + threadIdx.x;
  const u64 key = i < cap ? keys[i] : MAP_EMPTY;
  const bool sel = key != MAP_EMPTY;
  const unsigned j = map_compact(sel, s_n, s_base, total);
  if (!sel || j >= cap_out) return;
  map_rec_store(out, j, map_rec_from_slot(vals + i, key));
}

// One thread per input record (MERGE_RAW) or per slot of the source table (MERGE_TABLE): the voxel's sums are added to the
// slot of its key as k_map_walk adds a run's, in the same three modes, and the block's new voxels and points go through LDS
// to the map's sharded counters.  A record with count 0 or key bit 63 is never inserted (the rollback invariant is "a new
// key's slot has count 0"); the first one met poisons the batch's new-voxel count, so k_map_commit refuses the batch, and
// sets st->bad, so the host can tell why.  Only the checked path (MAP_INSERT) takes records that nobody has validated.
// The input of thread i of a merge or subtract launch: the record of a raw input, or of an occupied slot of the source table
// (MERGE_COARSE: under its coarse key).  Returns its key, or MAP_EMPTY: no input here, a slot with count 0 (a committed voxel
// has count >= 1), or a raw record with count 0 or key bit 63, which is `bad`.
template <int SRC>
__device__ __forceinline__ u64 map_merge_input(const MapMergeK& a, unsigned i, MapRec& r, bool& bad) {
  if (i >= a.n) return MAP_EMPTY;
  if (SRC == MERGE_RAW) {
    r = map_rec_from_raw(a.recs, i);
    bad = map_rec_bad(r);
    return bad ? MAP_EMPTY : r.key();
  }
  u64 key = a.skeys[i];
  if (key == MAP_EMPTY) return MAP_EMPTY;
  if (SRC == MERGE_COARSE) key = map_coarse_key(key, a.shift);
  r = map_rec_from_slot(a.svals + i, key);
  return r.n() == 0 ? MAP_EMPTY : key;
}

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
  MapRec r{};
  bool bad = false;
  const u64 key = map_merge_input<SRC>(a, i, r, bad);
  if (key != MAP_EMPTY) {
    const unsigned s = MODE == MAP_ACCUM ? map_slot<false>(a.keys, a.mask, key, nullptr, &a.st->fault)
                                         : map_slot<true>(a.keys, a.mask, key, &s_new, &a.st->fault);
    if (MODE != MAP_INSERT && s != ~0u) map_rec_add(a.vals + s, r);
    if (MODE != MAP_ACCUM) atomicAdd(&s_pts, r.n());
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
  MapRec r{};
  bool bad = false;
  const u64 key = map_merge_input<SRC>(a, i, r, bad);
  if (key != MAP_EMPTY) {
    const unsigned s = map_find(a.keys, a.mask, key);
    if (s == ~0u) {
      bad = true;
    } else if (UNDO) {
      map_rec_add(a.vals + s, r);
    } else {
      const u64 old = map_rec_sub(a.vals + s, r);
      if (old < r.n()) bad = true;
      else if (old == r.n()) atomicAdd(&s_freed, 1u);
      atomicAdd(&s_pts, r.n());
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
  MapRec r{};
  bool bad = false;
  const u64 key = map_merge_input<SRC>(a, i, r, bad);  // only the key and the count are looked at
  if (key != MAP_EMPTY) {
    const unsigned s = map_find(a.keys, a.mask, key);
    if (s != ~0u) {
      const MapRec left = map_rec_from_slot(a.vals + s, key);
      if (left.n() == 0 && (left.b.x | left.b.y | left.c.x | left.c.y | left.d.x | left.d.y)) atomicOr(&s_bad, 1u);
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

// ------------------------------------------------------------------------------------------------------------ host side --
extern "C" int revo_map_stage_create_(revo_map_stage** out) {
  revo_map_stage* st = new revo_map_stage();
  if (const int rc = st->com.create()) { (void)hipGetLastError(); delete st; return rc; }  // here, not in the first launch
  *out = st;
  return REVO_OK;
}
extern "C" void revo_map_stage_destroy_(revo_map_stage* st) {
  if (!st) return;
  delete st;  // the rows and the event go with their members
  (void)hipGetLastError();
}

// upper bound of the map's voxels: the last count the device published + the points of every batch enqueued after it
size_t map_occ_bound(revo_map* m) {
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
int map_grow(revo_map* m, size_t newcap, bool live_only) {
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
    const size_t bound = (size_t)nk[j] * npix;
    size_t ub = 0;
    TRY(map_need_slots(m, bound, "batch", &ub));
    chk[j] = ub + bound > m->max_voxels;
  }
  TRY(st->reserve(n, (int)dm.size(), s));
  for (int i = 0; i < n; ++i) {
    revo_map* m = maps[i];
    MapDesc& d = st->desc.h[i];
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
    st->com.h[j] = MapCommit{m->d_st, m->h_pub, (u64)m->max_voxels, m->seq, nk[j], chk[j]};
    m->pending.push_back({m->seq, (size_t)nk[j] * npix});
    any_check = any_check || chk[j];
    if (chk[j] && checked) checked->push_back(m);
  }
  TRY(st->upload(n, (int)dm.size(), s));
  const int nb = (int)((npix + 255) / 256);
  const MapGeomK gk{g.w, (int)npix, g.fx, g.fy, g.cx, g.cy, g.dmin, g.dmax};
  const dim3 grid((unsigned)(nb * n)), blk(256), cgrid((unsigned)((dm.size() + 63) / 64)), cblk(64);
  if (!any_check) {
    hipLaunchKernelGGL(k_map_walk<MAP_FUSED>, grid, blk, 0, s, st->desc.d, nb, gk);
    hipLaunchKernelGGL(k_map_commit, cgrid, cblk, 0, s, st->com.d, (int)dm.size());
  } else {
    hipLaunchKernelGGL(k_map_walk<MAP_INSERT>, grid, blk, 0, s, st->desc.d, nb, gk);
    hipLaunchKernelGGL(k_map_commit, cgrid, cblk, 0, s, st->com.d, (int)dm.size());
    for (size_t j = 0; j < dm.size(); ++j)
      if (chk[j])
        hipLaunchKernelGGL(k_map_rollback, dim3((unsigned)((dm[j]->cap + 255) / 256)), blk, 0, s, dm[j]->d_keys, dm[j]->d_vals,
                           (unsigned)dm[j]->cap, dm[j]->d_st);
    hipLaunchKernelGGL(k_map_walk<MAP_ACCUM>, grid, blk, 0, s, st->desc.d, nb, gk);
  }
  HIPCHECK(hipGetLastError());
  return REVO_OK;
}

extern "C" int revo_map_create(revo_ctx* ctx, float voxel, int dense, size_t initial_voxels, size_t max_voxels, revo_map** out) {
  if (!ctx || !out) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (!std::isfinite(voxel) || !(voxel > 0.0f)) return fail(REVO_ERR_INVALID_ARG, "voxel must be finite and > 0");
  if (dense != 0 && dense != 1) return fail(REVO_ERR_INVALID_ARG, "dense must be 0 or 1");
  if (max_voxels < 1 || max_voxels > MAP_MAX_VOXELS) return fail(REVO_ERR_INVALID_ARG, "max_voxels must be 1 .. 2^28");
  MapCtxGeom g;
  TRY(revo_map_ctx_geom_(ctx, &g));
  HIPCHECK(hipSetDevice(g.device));
  revo_map* m = new revo_map();
  m->ctx = ctx; m->g = g; m->voxel = voxel; m->dense = dense; m->max_voxels = max_voxels;
  revo_ctx_retain_(ctx);
  struct Guard { revo_map* m; ~Guard() { if (m) revo_map_destroy(m); } } guard{m};
  HIPCHECK(hipMalloc((void**)&m->d_st, sizeof(MapStats)));
  HIPCHECK(hipMemsetAsync(m->d_st, 0, sizeof(MapStats), (hipStream_t)g.stream));
  HIPCHECK(hipHostMalloc((void**)&m->h_pub, sizeof(u64) * 4));
  memset(m->h_pub, 0, sizeof(u64) * 4);
  TRY(revo_map_stage_create_(&m->stage));
  size_t c = 1024;
  const size_t want = std::min<size_t>(std::max<size_t>(initial_voxels, 1), max_voxels) * 2;
  while (c < want) c *= 2;
  TRY(map_grow(m, c));
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
  revo_ctx* ctx = m->ctx;
  delete m;  // the views' and rays' buffers, rows and events go with their members, on the map's device
  (void)hipGetLastError();
  revo_ctx_release_(ctx);
}

extern "C" int revo_map_integrate_many(revo_map* m, int n, const revo_pyr* const* kfs, const float* T) {
  if (!m || n < 0 || (n > 0 && (!kfs || !T))) return fail(REVO_ERR_INVALID_ARG, "null argument");
  if (n == 0) return REVO_OK;
  for (int i = 0; i < n; ++i) {
    if (!kfs[i]) return fail(REVO_ERR_INVALID_ARG, "null pyramid");
    if (!pose_is_finite(T + 16 * (size_t)i)) return fail(REVO_ERR_INVALID_ARG, "T_w_kf is not finite");
  }
  std::vector<MapSource> src(n);
  for (int i = 0; i < n; ++i) {
    const int rc = revo_map_source_(const_cast<revo_pyr*>(kfs[i]), &src[i]);
    if (rc) return rc;
    if (src[i].ctx != m->ctx) return fail(REVO_ERR_INVALID_ARG, "the pyramid belongs to another context than the map");
  }
  std::vector<revo_map*> maps(n, m), checked;
  TRY(integrate_core(m->stage, n, maps.data(), src.data(), T, &checked));
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

int map_read_stats(revo_map* m, MapStats* out) {
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
  TRY(map_read_stats(m, &st));
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
  TRY(map_read_stats(m, &st));
  hipStream_t s = (hipStream_t)m->g.stream;
  const size_t nv = std::max<size_t>((size_t)st.occ, 1);
  const size_t o_key = 0, o_xyz = o_key + 8 * nv, o_rgb = o_xyz + 12 * nv, o_cnt = o_rgb + 4 * nv, o_tot = o_cnt + 4 * nv;
  DevScratch scratch;
  TRY(scratch.alloc(o_tot + 256));
  char* const buf = scratch.p;
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

extern "C" int revo_map_voxel_size(revo_map* m, float* voxel, int* dense) {
  if (!m) return fail(REVO_ERR_INVALID_ARG, "null map");
  if (voxel) *voxel = m->voxel;
  if (dense) *dense = m->dense;
  return REVO_OK;
}

extern "C" int revo_map_export_raw(revo_map* m, revo_map_voxel_raw* dst, size_t cap, size_t* n, int device_out) {
  if (!m || !n) return fail(REVO_ERR_INVALID_ARG, "null argument");
  TRY(map_check_side(device_out, "device_out"));
  if (device_out) TRY(map_check_aligned((uintptr_t)dst, 16, "the device output is"));
  MapStats st;
  TRY(map_read_stats(m, &st));
  const size_t nv = (size_t)st.occ;
  *n = nv;
  if (!dst) return REVO_OK;
  if (cap < nv) return fail(REVO_ERR_CAPACITY, "voxel map: the output holds fewer records than the map has voxels");
  if (!nv) return REVO_OK;
  hipStream_t s = (hipStream_t)m->g.stream;
  DevScratch scratch;  // the launch's counter, and the records of a host-output call behind it
  TRY(scratch.alloc(256 + (device_out ? 0 : sizeof(revo_map_voxel_raw) * nv)));
  char* buf = scratch.p;
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
int map_merge_core(revo_map* m, MapMergeK a, int src_kind, size_t bound, bool trusted, int keyframes) {
  hipStream_t s = (hipStream_t)m->g.stream;
  size_t ub = 0;
  TRY(map_need_slots(m, bound, "merge", &ub));
  const bool chk = !trusted || ub + bound > m->max_voxels;
  HostRows<MapCommit>& com = m->stage->com;
  TRY(m->stage->reserve(0, 1, s));
  ++m->seq;
  com.h[0] = MapCommit{m->d_st, m->h_pub, (u64)m->max_voxels, m->seq, keyframes, chk ? 1 : 0};
  m->pending.push_back({m->seq, bound});
  TRY(m->stage->upload(0, 1, s));
  if (!trusted) HIPCHECK(hipMemsetAsync(&m->d_st->bad, 0, sizeof(u64), s));
  a.keys = m->d_keys; a.vals = m->d_vals; a.mask = (unsigned)(m->cap - 1); a.st = m->d_st;
  const dim3 grid((a.n + 255) / 256), blk(256);
  if (!chk) {
    launch_merge<MAP_FUSED>(src_kind, grid, s, a);
    hipLaunchKernelGGL(k_map_commit, dim3(1), dim3(64), 0, s, com.d, 1);
    HIPCHECK(hipGetLastError());
    return REVO_OK;
  }
  launch_merge<MAP_INSERT>(src_kind, grid, s, a);
  hipLaunchKernelGGL(k_map_commit, dim3(1), dim3(64), 0, s, com.d, 1);
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
  TRY(map_check_side(device_in, "device_in"));
  if (keyframes < 0) return fail(REVO_ERR_INVALID_ARG, "keyframes must be >= 0");
  if (n == 0) return REVO_OK;
  if (!src) return fail(REVO_ERR_INVALID_ARG, "null records");
  if (device_in) TRY(map_check_aligned((uintptr_t)src, 16, "the device records are"));
  if (n > MAP_MAX_CAP / 2) return fail(REVO_ERR_CAPACITY, "voxel map: a merge this large needs more than 2^31 table slots");
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  MapMergeK a{};
  a.n = (unsigned)n;
  a.dropped = (u64)points_dropped;
  if (device_in) {
    a.recs = (const ulonglong2*)src;
    return map_merge_core(m, a, MERGE_RAW, n, false, keyframes);
  }
  bool valid = true;  // a bad record still goes to the device, which refuses the merge and counts it
  for (size_t i = 0; i < n && valid; ++i) valid = src[i].count != 0 && !(src[i].key >> 63);
  DevScratch up;
  TRY(up.alloc(sizeof(revo_map_voxel_raw) * n));
  HIPCHECK(hipMemcpyAsync(up.p, src, sizeof(revo_map_voxel_raw) * n, hipMemcpyHostToDevice, s));
  a.recs = (const ulonglong2*)up.p;
  const int rc = map_merge_core(m, a, MERGE_RAW, n, valid, keyframes);
  if (hipStreamSynchronize(s) != hipSuccess && !rc) return fail(REVO_ERR_HIP, "hipStreamSynchronize failed");  // the upload is read
  return rc;
}

// revo_map_merge and revo_map_coarsen behind their own argument rules: src's table into dst, MERGE_COARSE under the keys of
// the voxels 2^shift times as long.
static int merge_table(revo_map* dst, revo_map* src, int src_kind, int shift) {
  if (dst->g.device != src->g.device) return fail(REVO_ERR_INVALID_ARG, "the maps are on different devices");
  MapStats ss;  // waits for src: its table is complete, and its counters say what comes
  TRY(map_read_stats(src, &ss));
  if (ss.kfs > 0x7fffffffull) return fail(REVO_ERR_INVALID_ARG, "the source map's keyframe count does not fit");
  HIPCHECK(hipSetDevice(dst->g.device));
  MapMergeK a{};
  a.skeys = src->d_keys; a.svals = src->d_vals; a.n = (unsigned)src->cap;
  a.dropped = ss.drop;
  a.shift = shift;
  const int rc = map_merge_core(dst, a, src_kind, (size_t)ss.occ, true, (int)ss.kfs);
  // maps of two contexts run on two streams: src's table must outlive the launch that reads it
  if (dst->g.stream != src->g.stream && hipStreamSynchronize((hipStream_t)dst->g.stream) != hipSuccess && !rc)
    return fail(REVO_ERR_HIP, "hipStreamSynchronize failed");
  return rc;
}
extern "C" int revo_map_merge(revo_map* dst, revo_map* src) {
  if (!dst || !src) return fail(REVO_ERR_INVALID_ARG, "null map");
  if (dst == src) return fail(REVO_ERR_INVALID_ARG, "a map cannot be merged into itself");
  if (memcmp(&dst->voxel, &src->voxel, sizeof(float))) return fail(REVO_ERR_INVALID_ARG, "the maps' voxel edges differ");
  return merge_table(dst, src, MERGE_TABLE, 0);
}
extern "C" int revo_map_coarsen(revo_map* dst, revo_map* src, int shift) {
  if (!dst || !src) return fail(REVO_ERR_INVALID_ARG, "null map");
  if (dst == src) return fail(REVO_ERR_INVALID_ARG, "a map cannot be coarsened into itself");
  if (shift < 1 || shift > 20) return fail(REVO_ERR_INVALID_ARG, "shift must be 1 .. 20");
  const float want = std::ldexp(src->voxel, shift);  // exact, or inf
  if (memcmp(&dst->voxel, &want, sizeof(float)))
    return fail(REVO_ERR_INVALID_ARG, "the destination's voxel edge is not the source's times 2^shift");
  return merge_table(dst, src, MERGE_COARSE, shift);
}

// One subtraction from m (contract: include/revo_hip.h): `a` names the input as in map_merge_core.  Subtract, verify,
// decide, undo if refused -- all enqueued at once behind the map's pending work -- then the call waits for the decision, and
// an accepted one that emptied voxels moves the live ones into a fresh table of the same size.
int map_subtract_core(revo_map* m, MapMergeK a, int src_kind, u64 dropped, u64 keyframes) {
  hipStream_t s = (hipStream_t)m->g.stream;
  ++m->seq;
  const MapSubCommit c{m->d_st, m->h_pub, m->seq, dropped, keyframes};
  HIPCHECK(hipMemsetAsync(&m->d_st->sub_bad, 0, 3 * sizeof(u64), s));
  a.keys = m->d_keys; a.vals = m->d_vals; a.mask = (unsigned)(m->cap - 1); a.st = m->d_st;
  const dim3 grid((a.n + 255) / 256), blk(256);
  const bool tab = src_kind == MERGE_TABLE;
  auto undo = [&] {
    if (tab) hipLaunchKernelGGL((k_map_sub<MERGE_TABLE, true>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((k_map_sub<MERGE_RAW, true>), grid, blk, 0, s, a);
  };
  if (tab) hipLaunchKernelGGL((k_map_sub<MERGE_TABLE, false>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((k_map_sub<MERGE_RAW, false>), grid, blk, 0, s, a);
  if (tab) hipLaunchKernelGGL((k_map_sub_verify<MERGE_TABLE>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((k_map_sub_verify<MERGE_RAW>), grid, blk, 0, s, a);
  hipLaunchKernelGGL(k_map_sub_commit, dim3(1), dim3(64), 0, s, c);
  undo();
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));  // the device has decided
  if (!m->h_pub[2])
    return fail(REVO_ERR_INVALID_ARG, "voxel map: the records are not part of the map -- a record with count 0 or key bit 63, a key "
                                      "the map does not hold, more than a voxel has, sums left in an emptied voxel, or more "
                                      "dropped points or keyframes than the map counts (nothing subtracted)");
  if (!m->h_pub[3]) return REVO_OK;
  const int rc = map_grow(m, m->cap, true);
  if (!rc) return REVO_OK;
  // no memory for the fresh table: the dead slots cannot stay, so the subtraction is taken back as a refused one is
  const std::string why = revo_last_error();
  ++m->seq;
  const MapSubCommit r{m->d_st, m->h_pub, m->seq, dropped, keyframes};
  hipLaunchKernelGGL(k_map_sub_revert, dim3(1), dim3(64), 0, s, r);
  undo();
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));
  return fail(rc, why + " (nothing subtracted)");
}

extern "C" int revo_map_subtract_raw(revo_map* m, const revo_map_voxel_raw* src, size_t n, int device_in, size_t points_dropped,
                                     int32_t keyframes) {
  if (!m) return fail(REVO_ERR_INVALID_ARG, "null map");
  TRY(map_check_side(device_in, "device_in"));
  if (keyframes < 0) return fail(REVO_ERR_INVALID_ARG, "keyframes must be >= 0");
  if (n == 0) return REVO_OK;
  if (!src) return fail(REVO_ERR_INVALID_ARG, "null records");
  if (device_in) TRY(map_check_aligned((uintptr_t)src, 16, "the device records are"));
  if (n > MAP_MAX_CAP) return fail(REVO_ERR_INVALID_ARG, "voxel map: more than 2^31 records in one subtraction");
  HIPCHECK(hipSetDevice(m->g.device));
  hipStream_t s = (hipStream_t)m->g.stream;
  MapMergeK a{};
  a.n = (unsigned)n;
  if (device_in) {
    a.recs = (const ulonglong2*)src;
    return map_subtract_core(m, a, MERGE_RAW, (u64)points_dropped, (u64)keyframes);
  }
  DevScratch up;
  TRY(up.alloc(sizeof(revo_map_voxel_raw) * n));
  HIPCHECK(hipMemcpyAsync(up.p, src, sizeof(revo_map_voxel_raw) * n, hipMemcpyHostToDevice, s));
  a.recs = (const ulonglong2*)up.p;
  return map_subtract_core(m, a, MERGE_RAW, (u64)points_dropped, (u64)keyframes);  // has waited: the upload is read
}

extern "C" int revo_map_subtract(revo_map* dst, revo_map* src) {
  if (!dst || !src) return fail(REVO_ERR_INVALID_ARG, "null map");
  if (dst == src) return fail(REVO_ERR_INVALID_ARG, "a map cannot be subtracted from itself (revo_map_clear empties it)");
  if (memcmp(&dst->voxel, &src->voxel, sizeof(float))) return fail(REVO_ERR_INVALID_ARG, "the maps' voxel edges differ");
  if (dst->g.device != src->g.device) return fail(REVO_ERR_INVALID_ARG, "the maps are on different devices");
  MapStats ss;  // waits for src: its table is complete, and its counters say what goes
  TRY(map_read_stats(src, &ss));
  HIPCHECK(hipSetDevice(dst->g.device));
  MapMergeK a{};
  a.skeys = src->d_keys; a.svals = src->d_vals; a.n = (unsigned)src->cap;
  return map_subtract_core(dst, a, MERGE_TABLE, ss.drop, ss.kfs);  // has waited for dst's stream: src's table is read
}
extern "C" void revo_map_note_attach_(revo_map* m, revo_vo_multi* mv, int stream, int attach) {
  if (!m) return;
  auto it = std::find(m->attached.begin(), m->attached.end(), std::make_pair(mv, stream));
  if (attach && it == m->attached.end()) m->attached.push_back({mv, stream});
  if (!attach && it != m->attached.end()) m->attached.erase(it);
}
extern "C" const revo_ctx* revo_map_ctx_(const revo_map* m) { return m ? m->ctx : nullptr; }
