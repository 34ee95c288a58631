// revo_tsdf_ray_host.h -- the rules of revo_map_tsdf_raycast (include/revo_hip.h) that host and device code share, each
// written once: the parameters a call runs with, a sample's depth and its place in the box, the interpolant and its gradient, the
// decision between two samples, a hit's depth, normal and colour, the samples a ray counts, the block a sample's base falls in,
// and the march itself -- plain, or asking the block mask first.  The field, the interpolation step, the normal and the colour
// byte are revo_tsdf_host.h's.  Plain C++: revo_map_tsdf_ray.hip compiles it for both sides, tests/cpp/tsdf_ray_host.cpp for the
// host alone.  Internal.
#pragma once
#include "revo_tsdf_host.h"

#define TSDF_RAY_MAX_VIEWS 64
#define TSDF_RAY_MAX_STEPS (1u << 20)
#define TSDF_RAY_DEFAULT_STEPS 4096u
#define TSDF_RAY_BLOCK 3  // log2 of a mask block's edge in sample bases
enum { TSDF_RAY_HIT = 0, TSDF_RAY_RANGE = 1, TSDF_RAY_BACKFACE = 2, TSDF_RAY_EXHAUSTED = 3, TSDF_RAY_STATUSES = 4 };

// The parameters a call runs with (NULL, and every zero: the voxel edge, min_weight 1, 4096 samples), or why they are refused.
inline const char* tsdf_ray_params_check(const revo_map_tsdf_ray_params* prm, float voxel, revo_map_tsdf_ray_params* out) {
  *out = prm ? *prm : revo_map_tsdf_ray_params{0.0f, 0u, 0u, 0u};
  if (!std::isfinite(out->step) || out->step < 0.0f) return "step must be finite and >= 0 (0: the voxel edge)";
  if (out->max_steps > TSDF_RAY_MAX_STEPS) return "max_steps must be 0 (4096) or 1 .. 2^20";
  if (out->reserved) return "the reserved word of the parameters must be 0";
  if (out->step == 0.0f) out->step = voxel;
  if (out->min_weight < 1u) out->min_weight = 1u;
  if (out->max_steps == 0u) out->max_steps = TSDF_RAY_DEFAULT_STEPS;
  return nullptr;
}

// What every ray of a call shares.
struct TsdfRayK {
  const revo_map_tsdf_cell* tsdf;
  const revo_map_tsdf_color* color;  // NULL: no colour is read
  const uint32_t* mask;              // a bit per block of sample bases (tsdf_ray_block); not looked at by the plain march
  revo_map_df_box box;
  int nby, nbz;                      // the mask's blocks along y and z
  float voxel, step;
  uint32_t min_weight, max_steps;    // both >= 1
};
struct TsdfRay { float ox, oy, oz, dx, dy, dz, zmin, zmax; };
// One evaluated sample: where it sits, whether it is valid, and for a valid one the interpolant, its gradient and the place of
// its colour cell in the volume.
struct TsdfRaySample { bool valid; float s, F, gx, gy, gz; uint32_t ccell; };
// A sample's place: whether its base lies in the box (every u finite, 0 <= b <= n - 2), the base and the fractions.
struct TsdfRayPlace { bool inbox; int bx, by, bz; float rx, ry, rz; };
struct TsdfRayOut { float depth, nx, ny, nz; uint8_t b, g, r; uint32_t colored; uint32_t samples; };  // colored: k of a hit

// The blocks the mask has along an axis of n cells: the bases are 0 .. n - 2; an axis of 1 has none and gets one empty block.
TSDF_HD int tsdf_ray_blocks(int n) { return n < 2 ? 1 : (n - 1 + (1 << TSDF_RAY_BLOCK) - 1) >> TSDF_RAY_BLOCK; }
TSDF_HD uint32_t tsdf_ray_block(int nby, int nbz, int bx, int by, int bz) {
  return (uint32_t)(((bx >> TSDF_RAY_BLOCK) * nby + (by >> TSDF_RAY_BLOCK)) * nbz + (bz >> TSDF_RAY_BLOCK));
}

// Sample k's depth: from the integer, never accumulated.
TSDF_HD float tsdf_ray_s(float zmin, uint32_t k, float step) { return zmin + (float)k * step; }

// One axis of a place: cell centres sit at integers.  g: the world coordinate.
TSDF_HD bool tsdf_ray_axis_at(float g, float voxel, int lo, int n, int* b, float* r) {
  const float u = tsdf_div(g, voxel) - ((float)lo + 0.5f);
  const float f = std::floor(u);
  *r = u - f;
  const bool ok = std::isfinite(u) && f >= 0.0f && f <= (float)(n - 2);
  *b = ok ? (int)f : 0;
  return ok;
}
// ... of a sample: the coordinate is o + s * d.
TSDF_HD bool tsdf_ray_axis(float o, float s, float d, float voxel, int lo, int n, int* b, float* r) {
  return tsdf_ray_axis_at(o + s * d, voxel, lo, n, b, r);
}
// The place of a world point (revo_map_tsdf_track).
TSDF_HD TsdfRayPlace tsdf_ray_place_at(const TsdfRayK& a, float gx, float gy, float gz) {
  TsdfRayPlace p;
  const bool okx = tsdf_ray_axis_at(gx, a.voxel, a.box.lo[0], a.box.n[0], &p.bx, &p.rx);
  const bool oky = tsdf_ray_axis_at(gy, a.voxel, a.box.lo[1], a.box.n[1], &p.by, &p.ry);
  const bool okz = tsdf_ray_axis_at(gz, a.voxel, a.box.lo[2], a.box.n[2], &p.bz, &p.rz);
  p.inbox = okx && oky && okz;
  return p;
}
TSDF_HD TsdfRayPlace tsdf_ray_place(const TsdfRayK& a, const TsdfRay& ray, float s) {
  TsdfRayPlace p;
  const bool okx = tsdf_ray_axis(ray.ox, s, ray.dx, a.voxel, a.box.lo[0], a.box.n[0], &p.bx, &p.rx);
  const bool oky = tsdf_ray_axis(ray.oy, s, ray.dy, a.voxel, a.box.lo[1], a.box.n[1], &p.by, &p.ry);
  const bool okz = tsdf_ray_axis(ray.oz, s, ray.dz, a.voxel, a.box.lo[2], a.box.n[2], &p.bz, &p.rz);
  p.inbox = okx && oky && okz;
  return p;
}

// Four values over two axes: along the first with r0, then along the second with r1.  v01: the far end of the first axis.
TSDF_HD float tsdf_ray_bilerp(float v00, float v01, float v10, float v11, float r0, float r1) {
  return tsdf_lerp(tsdf_lerp(v00, v01, r0), tsdf_lerp(v10, v11, r0), r1);
}
// The nearest corner of an axis; r == 0.5 goes up.
TSDF_HD int tsdf_ray_near(int b, float r) { return b + (r >= 0.5f ? 1 : 0); }

// The sample at the place p (its base in the box) from its eight cells, named c<x><y><z>: valid when all eight are.  *out holds
// tsdf_ray_sample's "not valid" on entry.
TSDF_HD void tsdf_ray_sample_cells(const TsdfRayK& a, const TsdfRayPlace& p, const revo_map_tsdf_cell& c000, const revo_map_tsdf_cell& c001,
                                   const revo_map_tsdf_cell& c010, const revo_map_tsdf_cell& c011, const revo_map_tsdf_cell& c100,
                                   const revo_map_tsdf_cell& c101, const revo_map_tsdf_cell& c110, const revo_map_tsdf_cell& c111, TsdfRaySample* out) {
  const size_t nz = (size_t)a.box.n[2], nyz = (size_t)a.box.n[1] * nz;
  const uint32_t mw = a.min_weight;
  if (!(tsdf_valid(c000.weight, mw) && tsdf_valid(c001.weight, mw) && tsdf_valid(c010.weight, mw) && tsdf_valid(c011.weight, mw) &&
        tsdf_valid(c100.weight, mw) && tsdf_valid(c101.weight, mw) && tsdf_valid(c110.weight, mw) && tsdf_valid(c111.weight, mw)))
    return;
  const float f000 = tsdf_field(c000.sum, c000.weight), f001 = tsdf_field(c001.sum, c001.weight);
  const float f010 = tsdf_field(c010.sum, c010.weight), f011 = tsdf_field(c011.sum, c011.weight);
  const float f100 = tsdf_field(c100.sum, c100.weight), f101 = tsdf_field(c101.sum, c101.weight);
  const float f110 = tsdf_field(c110.sum, c110.weight), f111 = tsdf_field(c111.sum, c111.weight);
  out->valid = true;
  // along z, then y, then x
  out->F = tsdf_lerp(tsdf_ray_bilerp(f000, f001, f010, f011, p.rz, p.ry), tsdf_ray_bilerp(f100, f101, f110, f111, p.rz, p.ry), p.rx);
  // the interpolant's own gradient: the differences along an axis, interpolated over the other two in the same order
  out->gx = tsdf_ray_bilerp(f100 - f000, f101 - f001, f110 - f010, f111 - f011, p.rz, p.ry);
  out->gy = tsdf_ray_bilerp(f010 - f000, f011 - f001, f110 - f100, f111 - f101, p.rz, p.rx);
  out->gz = tsdf_ray_bilerp(f001 - f000, f011 - f010, f101 - f100, f111 - f110, p.ry, p.rx);
  out->ccell = (uint32_t)((size_t)tsdf_ray_near(p.bx, p.rx) * nyz + (size_t)tsdf_ray_near(p.by, p.ry) * nz + (size_t)tsdf_ray_near(p.bz, p.rz));
}

// The sample at the place p: valid when its base lies in the box and its eight cells are valid.
TSDF_HD void tsdf_ray_sample(const TsdfRayK& a, const TsdfRayPlace& p, float s, TsdfRaySample* out) {
  out->valid = false; out->s = s; out->F = 0.0f; out->gx = 0.0f; out->gy = 0.0f; out->gz = 0.0f; out->ccell = 0u;
  if (!p.inbox) return;
  const size_t nz = (size_t)a.box.n[2], nyz = (size_t)a.box.n[1] * nz;
  const size_t c = (size_t)p.bx * nyz + (size_t)p.by * nz + (size_t)p.bz;
  const revo_map_tsdf_cell c000 = a.tsdf[c], c001 = a.tsdf[c + 1], c010 = a.tsdf[c + nz], c011 = a.tsdf[c + nz + 1];
  const revo_map_tsdf_cell c100 = a.tsdf[c + nyz], c101 = a.tsdf[c + nyz + 1], c110 = a.tsdf[c + nyz + nz], c111 = a.tsdf[c + nyz + nz + 1];
  tsdf_ray_sample_cells(a, p, c000, c001, c010, c011, c100, c101, c110, c111, out);
}

// What two valid samples that follow each other decide: -1 nothing, else the status that ends the ray.
TSDF_HD int tsdf_ray_decide(float Fp, float F) {
  if (Fp >= 0.0f && F < 0.0f) return TSDF_RAY_HIT;
  if (Fp < 0.0f && F >= 0.0f) return TSDF_RAY_BACKFACE;
  return -1;
}
// The samples a ray counts: those whose place was formed.  k: the sample that ended it.
TSDF_HD uint32_t tsdf_ray_samples(int status, uint32_t k) { return status == TSDF_RAY_HIT || status == TSDF_RAY_BACKFACE ? k + 1u : k; }

// A hit between the samples p (the previous one) and c, from the two alone.
TSDF_HD void tsdf_ray_hit(const TsdfRayK& a, const TsdfRaySample& p, const TsdfRaySample& c, TsdfRayOut* out) {
  const float al = tsdf_div(p.F, p.F - c.F);
  out->depth = p.s + al * a.step;
  tsdf_normal(tsdf_lerp(p.gx, c.gx, al), tsdf_lerp(p.gy, c.gy, al), tsdf_lerp(p.gz, c.gz, al), &out->nx, &out->ny, &out->nz);
  if (a.color) {
    const revo_map_tsdf_color c0 = a.color[p.ccell], c1 = a.color[c.ccell];
    out->b = tsdf_color_byte(c0.sum_b, c0.weight, c1.sum_b, c1.weight, al);
    out->g = tsdf_color_byte(c0.sum_g, c0.weight, c1.sum_g, c1.weight, al);
    out->r = tsdf_color_byte(c0.sum_r, c0.weight, c1.sum_r, c1.weight, al);
    out->colored = tsdf_color_k(c0.weight, c1.weight);
  }
}

// The march of one ray -> its status; *out: a miss's zeros or the hit, and the samples.
// MASK: a sample is evaluated only where it can decide the ray.  A sample whose base lies in a block without a mark (or outside the
// box) is invalid or has F >= 0 -- interpolating corners that are all >= 0 with fractions in [0, 1] cannot round below 0 -- so it is
// neither the end of a HIT nor the negative end of a BACKFACE: it matters only as the sample behind a valid one with F < 0.  When
// an evaluated sample's predecessor was skipped, the predecessor is evaluated from its integer k first.  The decisions are made
// on the same pairs of samples with the same numbers as the plain march makes them, and `samples` is counted from the k that ends
// the ray.
template <bool MASK>
TSDF_HD int tsdf_ray_march(const TsdfRayK& a, const TsdfRay& ray, TsdfRayOut* out) {
  out->depth = 0.0f; out->nx = 0.0f; out->ny = 0.0f; out->nz = 0.0f; out->b = 0; out->g = 0; out->r = 0; out->colored = 0u; out->samples = 0u;
  TsdfRaySample prev, cur;
  prev.valid = false; prev.s = 0.0f; prev.F = 0.0f; prev.gx = 0.0f; prev.gy = 0.0f; prev.gz = 0.0f; prev.ccell = 0u;
  bool have_prev = true;  // "no previous sample" is known, and not valid
  for (uint32_t k = 0;; ++k) {
    if (k == a.max_steps) { out->samples = tsdf_ray_samples(TSDF_RAY_EXHAUSTED, k); return TSDF_RAY_EXHAUSTED; }
    const float s = tsdf_ray_s(ray.zmin, k, a.step);
    if (!(s < ray.zmax)) { out->samples = tsdf_ray_samples(TSDF_RAY_RANGE, k); return TSDF_RAY_RANGE; }
    const TsdfRayPlace p = tsdf_ray_place(a, ray, s);
    if (MASK) {
      bool need = have_prev && prev.valid && prev.F < 0.0f;
      if (!need && p.inbox) {
        const uint32_t blk = tsdf_ray_block(a.nby, a.nbz, p.bx, p.by, p.bz);
        need = ((a.mask[blk >> 5] >> (blk & 31u)) & 1u) != 0u;
      }
      if (!need) { have_prev = false; continue; }
      if (!have_prev) {  // k > 0: the first sample has a known predecessor
        const float sp = tsdf_ray_s(ray.zmin, k - 1u, a.step);
        tsdf_ray_sample(a, tsdf_ray_place(a, ray, sp), sp, &prev);
        have_prev = true;
      }
    }
    tsdf_ray_sample(a, p, s, &cur);
    if (cur.valid && prev.valid) {
      const int st = tsdf_ray_decide(prev.F, cur.F);
      if (st >= 0) {
        out->samples = tsdf_ray_samples(st, k);
        if (st == TSDF_RAY_HIT) tsdf_ray_hit(a, prev, cur, out);
        return st;
      }
    }
    prev = cur;
  }
}
