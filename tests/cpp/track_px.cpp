// The tracker's per-point arithmetic in register pairs (revo_amd/csrc/revo_track_px.h, the header k_track and k_pair_info
// include), built for the host, against the scalar form it replaced -- transcribed below as the REFERENCE form -- bit for bit:
// every field of the projected point, r0, r1, res, good, wr, the six Jacobian entries, the 27 normal-equation sums after the
// point, the error / count terms, and for the error-only retries the patch rule, the four samples, res, good, wr and the error
// term.  The hardware reciprocal is a host stand-in (1.0f / d) in both forms: this
// proves the equality of the FORMS.  (Inputs stay where a valid point's terms are finite, Z >= 2^-6: a NaN would be a NaN in both
// forms, but a negation moved across a product may flip its sign bit.)  Prints one line per case family and exits non-zero at the first differing bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../revo_amd/csrc/revo_track_px.h"

// ---- the reference form: the scalar code of revo_track_dev.h / revo_track.hip before the pair form -------------------------
namespace ref {
static inline float recip_refined(float d) {
  const float r0 = 1.0f / d;
  const float e0 = fmaf(-d, r0, 1.0f);
  return fmaf(e0, r0, r0);
}
static inline float div_with(float n, float d, float r1) {
  const float q0 = n * r1;
  const float e1 = fmaf(-d, q0, n);
  const float q1 = fmaf(e1, r1, q0);
  const float e2 = fmaf(-d, q1, n);
  return fmaf(e2, r1, q1);
}
static inline float div(float n, float d) { return div_with(n, d, recip_refined(d)); }
struct Patch { float a0, a1, b0, b1, b2, b3, c0, c1, c2, c3, d0, d1; };
struct Pt { float X, Y, Z, rz, dx, dy; int ix, iy; bool valid; };
struct P3 { float x, y, z; };
static inline Pt project_point(const P3 p, const float* R, const float* T, const Cam& c, bool in_range) {
  Pt s;
  s.X = ((R[0] * p.x + R[3] * p.y) + R[6] * p.z) + T[0];
  s.Y = ((R[1] * p.x + R[4] * p.y) + R[7] * p.z) + T[1];
  s.Z = ((R[2] * p.x + R[5] * p.y) + R[8] * p.z) + T[2];
  s.rz = recip_refined(s.Z);
  const float u = div_with(s.X, s.Z, s.rz) * c.fx + c.cx;
  const float v = div_with(s.Y, s.Z, s.rz) * c.fy + c.cy;
  s.valid = in_range && (u > 1.0f && v > 1.0f && u < c.wlim && v < c.hlim);
  s.ix = s.valid ? (int)u : 1;
  s.iy = s.valid ? (int)v : 1;
  s.dx = u - (float)s.ix;
  s.dy = v - (float)s.iy;
  if (!s.valid) { s.X = 0.0f; s.Y = 0.0f; s.Z = 1.0f; s.rz = 1.0f; s.dx = 0.0f; s.dy = 0.0f; }
  return s;
}
struct Term { float r0, r1, res, wr, jv[6]; bool good; };
static inline Term accumulate_point(const Pt& s, const Patch& q, float fx, float fy, float edist, bool filt, float huber, float* acc) {
  Term t;
  const float gx00 = 0.5f * (q.b0 - q.b2), gy00 = 0.5f * (q.a0 - q.c1), d00 = q.b1;
  const float gx10 = 0.5f * (q.b1 - q.b3), gy10 = 0.5f * (q.a1 - q.c2), d10 = q.b2;
  const float gx01 = 0.5f * (q.c0 - q.c2), gy01 = 0.5f * (q.b1 - q.d0), d01 = q.c1;
  const float gx11 = 0.5f * (q.c1 - q.c3), gy11 = 0.5f * (q.b2 - q.d1), d11 = q.c2;
  const float dxdy = s.dx * s.dy;
  const float w11 = dxdy, w01 = s.dy - dxdy, w10 = s.dx - dxdy, w00 = ((1.0f - s.dx) - s.dy) + dxdy;
  float r0 = ((w11 * gx11 + w01 * gx01) + w10 * gx10) + w00 * gx00;
  float r1 = ((w11 * gy11 + w01 * gy01) + w10 * gy10) + w00 * gy00;
  float res = ((w11 * d11 + w01 * d01) + w10 * d10) + w00 * d00;
  const bool good = s.valid && !(res > edist && filt);
  if (!good) { r0 = 0.0f; r1 = 0.0f; res = 0.0f; }
  const float wr = (res <= huber) ? 1.0f : div(huber, res);
  const float gx = fx * r0, gy = fy * r1;
  const float z = div_with(1.0f, s.Z, s.rz);
  const float zs = z * z;
  float* jv = t.jv;
  jv[0] = z * gx;
  jv[1] = z * gy;
  jv[2] = (-s.X * zs) * gx + (-s.Y * zs) * gy;
  jv[3] = (-s.X * s.Y * zs) * gx + (-(1.0f + s.Y * s.Y * zs)) * gy;
  jv[4] = (1.0f + s.X * s.X * zs) * gx + (s.X * s.Y * zs) * gy;
  jv[5] = (-s.Y * z) * gx + (s.X * z) * gy;
  float wv[6];
  for (int a = 0; a < 6; ++a) wv[a] = wr * jv[a];
  {
    int k = 0;
    for (int a = 0; a < 6; ++a)
      for (int c = a; c < 6; ++c) { acc[k] = fmaf(wv[a], jv[c], acc[k]); ++k; }
  }
  for (int a = 0; a < 6; ++a) acc[21 + a] = fmaf(wv[a], res, acc[21 + a]);
  t.r0 = r0; t.r1 = r1; t.res = res; t.wr = wr; t.good = good;
  return t;
}
struct Retry { float d00, d10, d01, d11, res, wr; bool hit, good; };
// g[4]: what the exec-masked gather brings for a retry that is not in the patch
static inline Retry retry(const Pt& s0, const Pt& sj, const Patch& q, const float* g, float edist, bool filt, float huber) {
  Retry t;
  const int ddx = sj.ix - s0.ix, ddy = sj.iy - s0.iy;
  t.hit = (ddy == 0 && ddx >= -1 && ddx <= 1) || (ddx == 0 && (ddy == 1 || ddy == -1));
  float d00 = g[0], d10 = g[1], d01 = g[2], d11 = g[3];
  if (t.hit) {
    const bool same_row = ddy == 0, up = ddy < 0, left = ddx < 0, mid = ddx == 0;
    d00 = same_row ? (left ? q.b0 : (mid ? q.b1 : q.b2)) : (up ? q.a0 : q.c1);
    d10 = same_row ? (left ? q.b1 : (mid ? q.b2 : q.b3)) : (up ? q.a1 : q.c2);
    d01 = same_row ? (left ? q.c0 : (mid ? q.c1 : q.c2)) : (up ? q.b1 : q.d0);
    d11 = same_row ? (left ? q.c1 : (mid ? q.c2 : q.c3)) : (up ? q.b2 : q.d1);
  }
  const float dxdy = sj.dx * sj.dy;
  const float w11 = dxdy, w01 = sj.dy - dxdy, w10 = sj.dx - dxdy, w00 = ((1.0f - sj.dx) - sj.dy) + dxdy;
  float res = ((w11 * d11 + w01 * d01) + w10 * d10) + w00 * d00;
  t.good = sj.valid && !(res > edist && filt);
  if (!t.good) res = 0.0f;
  t.wr = (res <= huber) ? 1.0f : div(huber, res);
  t.res = res; t.d00 = d00; t.d10 = d10; t.d01 = d01; t.d11 = d11;
  return t;
}
}  // namespace ref

// ---- one case ---------------------------------------------------------------------------------------------------------------
struct Case {
  ref::P3 p;
  float R[4][9], T[4][3];  // candidate 0 and three retries
  Cam cam;
  ref::Patch q;
  float g[3][4];
  float edist, huber;
  bool filt;
  float acc0[27];
};
static unsigned long long g_cases = 0;
static const char* g_family = "";

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static void fail(const Case& c, const char* what, int idx, double a, double b) {
  std::fprintf(stderr, "MISMATCH in %s, case %llu: %s[%d] reference %.9g (%a) pair form %.9g (%a)\n", g_family, g_cases, what, idx, a, a, b, b);
  std::fprintf(stderr, "  p = %a %a %a  cam fx %a fy %a cx %a cy %a wlim %a hlim %a  edist %a filt %d huber %a\n", c.p.x, c.p.y, c.p.z,
               c.cam.fx, c.cam.fy, c.cam.cx, c.cam.cy, c.cam.wlim, c.cam.hlim, c.edist, (int)c.filt, c.huber);
  for (int j = 0; j < 4; ++j) {
    std::fprintf(stderr, "  pose %d: R", j);
    for (int i = 0; i < 9; ++i) std::fprintf(stderr, " %a", c.R[j][i]);
    std::fprintf(stderr, "  T %a %a %a\n", c.T[j][0], c.T[j][1], c.T[j][2]);
  }
  const float* q = &c.q.a0;
  std::fprintf(stderr, "  patch");
  for (int i = 0; i < 12; ++i) std::fprintf(stderr, " %a", q[i]);
  std::fprintf(stderr, "\n");
  std::exit(1);
}
#define EQF(what, idx, a, b) do { if (bits(a) != bits(b)) fail(c, what, idx, a, b); } while (0)
#define EQI(what, idx, a, b) do { if ((a) != (b)) fail(c, what, idx, (double)(a), (double)(b)); } while (0)

static void same_point(const Case& c, const char* what, const ref::Pt& r, const PtState& s) {
  char name[64];
  std::snprintf(name, sizeof name, "%s", what);
  EQF(name, 0, r.X, s.XY.x); EQF(name, 1, r.Y, s.XY.y); EQF(name, 2, r.Z, s.Z); EQF(name, 3, r.rz, s.rz);
  EQF(name, 4, r.dx, s.d.x); EQF(name, 5, r.dy, s.d.y); EQI(name, 6, r.ix, s.ix); EQI(name, 7, r.iy, s.iy); EQI(name, 8, r.valid, s.valid);
}

static void check(const Case& c) {
  ++g_cases;
  // the projections
  ref::Pt rp[4];
  PtState sp[4];
  for (int j = 0; j < 4; ++j) {
    rp[j] = ref::project_point(c.p, c.R[j], c.T[j], c.cam, true);
    sp[j] = project_point(c.p.x, c.p.y, c.p.z, c.R[j], c.T[j], c.cam, true);
    same_point(c, "project_point", rp[j], sp[j]);
  }
  const ref::Pt out = ref::project_point(c.p, c.R[0], c.T[0], c.cam, false);  // in_range = false: a point past the list's end
  same_point(c, "project_point out of range", out, project_point(c.p.x, c.p.y, c.p.z, c.R[0], c.T[0], c.cam, false));
  // candidate 0 in full
  DtPatch q;
  q.a = tpx_mk(c.q.a0, c.q.a1); q.b01 = tpx_mk(c.q.b0, c.q.b1); q.b23 = tpx_mk(c.q.b2, c.q.b3);
  q.c01 = tpx_mk(c.q.c0, c.q.c1); q.c23 = tpx_mk(c.q.c2, c.q.c3); q.d = tpx_mk(c.q.d0, c.q.d1);
  float ra[27], na[27];
  std::memcpy(ra, c.acc0, sizeof ra);
  std::memcpy(na, c.acc0, sizeof na);
  const ref::Term rt = ref::accumulate_point(rp[0], c.q, c.cam.fx, c.cam.fy, c.edist, c.filt, c.huber, ra);
  const PtTerm nt = point_term(sp[0], q, c.cam.fx, c.cam.fy, c.edist, c.filt, c.huber);
  const Jac nj = jacobian(sp[0], nt.G);
  accumulate_normal(nj, nt.wr, nt.res, na);
  EQF("r0", 0, rt.r0, nt.r0); EQF("r1", 0, rt.r1, nt.r1); EQF("res", 0, rt.res, nt.res); EQF("wr", 0, rt.wr, nt.wr);
  EQI("good", 0, rt.good, nt.good);
  const float njv[6] = {nj.J01.x, nj.J01.y, nj.J23.x, nj.J23.y, nj.J45.x, nj.J45.y};
  for (int a = 0; a < 6; ++a) EQF("jv", a, rt.jv[a], njv[a]);
  for (int k = 0; k < 27; ++k) EQF("acc", k, ra[k], na[k]);
  EQF("error term w r^2", 0, rt.wr * (rt.res * rt.res), nt.wr * (nt.res * nt.res));
  EQF("error term r^2", 0, rt.res * rt.res, nt.res * nt.res);
  // the retries: the patch rule, the samples, the term
  tpx_f2 D0[3], D1[3];
  ref::Retry rr[3];
  for (int j = 0; j < 3; ++j) {
    rr[j] = ref::retry(rp[0], rp[1 + j], c.q, c.g[j], c.edist, c.filt, c.huber);
    const PtState& s = sp[1 + j];
    const bool hit = retry_in_patch(s.ix, s.iy, sp[0].ix, sp[0].iy);
    EQI("retry hit", j, rr[j].hit, hit);
    retry_pick(q, s.ix, s.iy, sp[0].ix, sp[0].iy, D0[j], D1[j]);
    D0[j] = tpx_sel(hit, D0[j], tpx_mk(c.g[j][0], c.g[j][1]));
    D1[j] = tpx_sel(hit, D1[j], tpx_mk(c.g[j][2], c.g[j][3]));
    EQF("retry d00", j, rr[j].d00, D0[j].x); EQF("retry d10", j, rr[j].d10, D0[j].y);
    EQF("retry d01", j, rr[j].d01, D1[j].x); EQF("retry d11", j, rr[j].d11, D1[j].y);
    const RetryTerm t = retry_term(s, D0[j], D1[j], c.edist, c.filt, c.huber);
    EQF("retry res", j, rr[j].res, t.res); EQF("retry wr", j, rr[j].wr, t.wr); EQI("retry good", j, rr[j].good, t.good);
    EQF("retry error term", j, rr[j].wr * (rr[j].res * rr[j].res), t.wr * (t.res * t.res));
  }
}

// ---- inputs -----------------------------------------------------------------------------------------------------------------
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}
static float uni(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() >> 8) * (1.0f / 16777216.0f); }
static const float NO_EDGE = sqrtf(1e15f);

static void small_pose(float* R, float* T, float rot, float tr) {  // column-major, first order in the angles (need not be orthogonal)
  const float a = uni(-rot, rot), b = uni(-rot, rot), g = uni(-rot, rot);
  const float M[9] = {1.0f, g, -b, -g, 1.0f, a, b, -a, 1.0f};
  std::memcpy(R, M, sizeof M);
  for (int i = 0; i < 3; ++i) T[i] = uni(-tr, tr);
}
static void identity_pose(float* R, float* T) {
  const float M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::memcpy(R, M, sizeof M);
  T[0] = T[1] = T[2] = 0.0f;
}
static Cam camera(float fx, float fy, float cx, float cy, int w, int h) {
  Cam c;
  c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy; c.w = w; c.h = h; c.wlim = (float)(w - 2); c.hlim = (float)(h - 2);
  return c;
}
static void random_patch(Case& c, int no_edge_every) {
  float* q = &c.q.a0;
  for (int i = 0; i < 12; ++i) q[i] = (no_edge_every && rnd() % no_edge_every == 0) ? NO_EDGE : uni(0.0f, 40.0f);
  for (auto& g : c.g)
    for (float& v : g) v = (no_edge_every && rnd() % no_edge_every == 0) ? NO_EDGE : uni(0.0f, 40.0f);
}
static void defaults(Case& c) {
  c.cam = camera(262.5f, 262.5f, 159.75f, 119.75f, 320, 240);
  c.edist = 20.0f; c.huber = 0.3f; c.filt = true;
  for (float& a : c.acc0) a = 0.0f;
}

static void family(const char* name) { g_family = name; }
static void done(unsigned long long before) { std::printf("%s: %llu cases\n", g_family, g_cases - before); }

static void random_cases(unsigned long long n) {
  family("random");
  const unsigned long long before = g_cases;
  for (unsigned long long i = 0; i < n; ++i) {
    Case c;
    defaults(c);
    const float z = uni(0.4f, 6.0f);
    c.p = {uni(-0.75f, 0.75f) * z, uni(-0.6f, 0.6f) * z, z};  // a good part projects outside the image
    small_pose(c.R[0], c.T[0], 0.05f, 0.05f);
    // the retries: shorter steps from the same pose -- mostly the same pixel or a neighbour, sometimes far
    for (int j = 1; j < 4; ++j) {
      const float s = (rnd() % 8 == 0) ? 0.05f : 0.002f;
      float dR[9], dT[3];
      small_pose(dR, dT, s, s);
      for (int k = 0; k < 9; ++k) c.R[j][k] = c.R[0][k] + (dR[k] - ((k % 4 == 0) ? 1.0f : 0.0f));
      for (int k = 0; k < 3; ++k) c.T[j][k] = c.T[0][k] + dT[k];
    }
    random_patch(c, (i % 4 == 0) ? 6 : 0);
    c.filt = (rnd() & 1) != 0;
    c.edist = uni(2.0f, 30.0f);
    c.huber = uni(0.05f, 5.0f);
    if (i & 1) for (float& a : c.acc0) a = uni(-100.0f, 100.0f);
    check(c);
  }
  done(before);
}

// fx = fy = 1, cx = cy = 0, identity pose, Z = 1: (u, v) = (X, Y) exactly
static void bounds_cases() {
  family("bounds, Z = 0 and negative Z");
  const unsigned long long before = g_cases;
  const float wl = 318.0f, hl = 238.0f;
  const float us[] = {-3.0f, 0.0f, 0.5f, std::nextafter(1.0f, 0.0f), 1.0f, std::nextafter(1.0f, 2.0f), 1.5f, 100.25f,
                      std::nextafter(wl, 0.0f), wl, std::nextafter(wl, 1e9f), wl + 1.0f, 1e9f};
  const float vs[] = {-3.0f, 0.0f, 0.5f, std::nextafter(1.0f, 0.0f), 1.0f, std::nextafter(1.0f, 2.0f), 1.5f, 77.75f,
                      std::nextafter(hl, 0.0f), hl, std::nextafter(hl, 1e9f), hl + 1.0f, 1e9f};
  const float zs[] = {1.0f, 0.0f, -0.0f, -1.0f, -2.5f, 0.015625f, 3.0f};
  for (float z : zs)
    for (float u : us)
      for (float v : vs)
        for (int f = 0; f < 2; ++f) {
          Case c;
          defaults(c);
          c.cam = camera(1.0f, 1.0f, 0.0f, 0.0f, 320, 240);
          c.p = {u * (z == 1.0f ? 1.0f : z), v * (z == 1.0f ? 1.0f : z), z};
          identity_pose(c.R[0], c.T[0]);
          for (int j = 1; j < 4; ++j) { identity_pose(c.R[j], c.T[j]); c.T[j][0] = 0.75f * (float)(j - 2); c.T[j][1] = 0.5f * (float)(2 - j); }
          random_patch(c, 0);
          c.filt = f != 0;
          check(c);
        }
  done(before);
}

// dx = dy = 0 and a constant patch v: res = v exactly -- v just below, at and above a threshold
static void threshold_cases() {
  family("res around edge_distance and huber");
  const unsigned long long before = g_cases;
  for (int which = 0; which < 2; ++which)
    for (int step = -2; step <= 2; ++step)
      for (int f = 0; f < 2; ++f)
        for (int frac = 0; frac < 2; ++frac) {
          Case c;
          defaults(c);
          c.cam = camera(1.0f, 1.0f, 0.0f, 0.0f, 320, 240);
          c.edist = 12.5f; c.huber = 0.3f; c.filt = f != 0;
          float v = which ? c.huber : c.edist;
          for (int k = 0; k < (step < 0 ? -step : step); ++k) v = std::nextafter(v, step < 0 ? 0.0f : 1e9f);
          c.p = {50.0f + 0.25f * (float)frac, 60.0f + 0.5f * (float)frac, 1.0f};  // frac: an interior sample of the constant patch
          identity_pose(c.R[0], c.T[0]);
          for (int j = 1; j < 4; ++j) { identity_pose(c.R[j], c.T[j]); c.T[j][0] = (float)(j - 2); }
          float* q = &c.q.a0;
          for (int i = 0; i < 12; ++i) q[i] = v;
          for (auto& g : c.g)
            for (float& x : g) x = v;
          for (float& a : c.acc0) a = uni(-10.0f, 10.0f);
          check(c);
        }
  done(before);
}

static void patch_cases() {
  family("all-zero patches, the no-edge value in some and in all samples, every neighbour offset");
  const unsigned long long before = g_cases;
  for (int kind = 0; kind < 4; ++kind)
    for (int ox = -2; ox <= 2; ++ox)
      for (int oy = -2; oy <= 2; ++oy)
        for (int f = 0; f < 2; ++f)
          for (int rep = 0; rep < 16; ++rep) {
            Case c;
            defaults(c);
            c.cam = camera(1.0f, 1.0f, 0.0f, 0.0f, 320, 240);
            c.filt = f != 0;
            c.p = {uni(20.0f, 300.0f), uni(20.0f, 200.0f), 1.0f};
            identity_pose(c.R[0], c.T[0]);
            for (int j = 1; j < 4; ++j) { identity_pose(c.R[j], c.T[j]); }
            c.T[1][0] = (float)ox; c.T[1][1] = (float)oy;  // retry 1 at every offset of [-2, 2]^2, retries 2 and 3 across it
            c.T[2][0] = (float)oy; c.T[2][1] = (float)-ox;
            c.T[3][0] = uni(-1.5f, 1.5f); c.T[3][1] = uni(-1.5f, 1.5f);
            float* q = &c.q.a0;
            random_patch(c, kind == 2 ? 3 : 0);
            if (kind == 0) { for (int i = 0; i < 12; ++i) q[i] = 0.0f; for (auto& g : c.g) for (float& x : g) x = 0.0f; }
            if (kind == 3) { for (int i = 0; i < 12; ++i) q[i] = NO_EDGE; for (auto& g : c.g) for (float& x : g) x = NO_EDGE; }
            check(c);
          }
  done(before);
}

int main() {
  bounds_cases();
  threshold_cases();
  patch_cases();
  random_cases(2000000ull);
  std::printf("cases %llu mismatches 0\n", g_cases);
  return 0;
}
