// revo_align_host.h -- the host arithmetic of revo_map_align and revo_map_align_plane (include/revo_hip.h): the Gauss-Newton system of a
// record, its Cholesky solve, the SE(3) exponential and the iteration itself, over any evaluator of records.  Plain C++ with no
// device code: revo_map.hip runs it over k_map_align, tests/cpp/align_host.cpp over recorded records.  Internal.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/revo_hip.h"

// revo_map_align_system's arithmetic: the one place that fixes the signs
inline void align_system_fill(const revo_map_align_info* info, double H[36], double g[6]) {
  const float* S = info->S;
  const double n = (double)info->matched, ux = S[0], uy = S[1], uz = S[2];
  const double xx = S[3], xy = S[4], xz = S[5], yy = S[6], yz = S[7], zz = S[8];
  for (int i = 0; i < 36; ++i) H[i] = 0.0;
  H[0] = H[7] = H[14] = n;
  // top right: -[Su]x; bottom left: [Su]x, its transpose
  H[0 * 6 + 4] = uz;  H[0 * 6 + 5] = -uy;
  H[1 * 6 + 3] = -uz; H[1 * 6 + 5] = ux;
  H[2 * 6 + 3] = uy;  H[2 * 6 + 4] = -ux;
  for (int a = 0; a < 3; ++a)
    for (int b = 3; b < 6; ++b) H[b * 6 + a] = H[a * 6 + b];
  // bottom right: S(|u|^2 I - u u^T)
  H[3 * 6 + 3] = yy + zz; H[4 * 6 + 4] = xx + zz; H[5 * 6 + 5] = xx + yy;
  H[3 * 6 + 4] = H[4 * 6 + 3] = -xy;
  H[3 * 6 + 5] = H[5 * 6 + 3] = -xz;
  H[4 * 6 + 5] = H[5 * 6 + 4] = -yz;
  for (int i = 0; i < 6; ++i) g[i] = (double)S[9 + i];
}

// H x = -g by the Cholesky factorisation and pivot rule of revo_pair_info_covariance (revo_info.hip); false: rank-deficient.
inline bool align_solve(const double H[36], const double g[6], double x[6]) {
  double L[6][6] = {};
  for (int j = 0; j < 6; ++j) {
    double p = H[j * 6 + j];
    for (int k = 0; k < j; ++k) p -= L[j][k] * L[j][k];
    if (!(p > 64.0 * 2.220446049250313e-16 * H[j * 6 + j]) || !std::isfinite(p)) return false;
    L[j][j] = std::sqrt(p);
    for (int i = j + 1; i < 6; ++i) {
      double v = H[i * 6 + j];
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / L[j][j];
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double v = -g[i];
    for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
    y[i] = v / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double v = y[i];
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
    x[i] = v / L[i][i];
  }
  for (int i = 0; i < 6; ++i) if (!std::isfinite(x[i])) return false;
  return true;
}

// row-major 4x4 doubles
inline void mat4_mul(const double* A, const double* B, double* C) {
  double r[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double v = 0.0;
      for (int k = 0; k < 4; ++k) v += A[4 * i + k] * B[4 * k + j];
      r[4 * i + j] = v;
    }
  memcpy(C, r, sizeof(r));
}
// expm(hat(x)), x = (v, w): Rodrigues and the left Jacobian V, t = V v (the convention of the tracker's increment)
inline void se3_exp_d(const double x[6], double* E) {
  const double* v = x; const double* w = x + 3;
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double W[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double W2[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) W2[3 * i + j] = W[3 * i] * W[j] + W[3 * i + 1] * W[3 + j] + W[3 * i + 2] * W[6 + j];
  double a = 1.0, b = 0.0, c = 0.5, d = 0.0;  // R = I + a W + b W^2, V = I + c W + d W^2
  if (!(th < 1e-10)) {
    a = std::sin(th) / th; b = (1.0 - std::cos(th)) / (th * th);
    c = b; d = (th - std::sin(th)) / (th * th * th);
  }
  for (int i = 0; i < 16; ++i) E[i] = 0.0;
  E[15] = 1.0;
  for (int i = 0; i < 3; ++i) {
    double t = 0.0;
    for (int j = 0; j < 3; ++j) {
      const double I = i == j ? 1.0 : 0.0;
      E[4 * i + j] = I + a * W[3 * i + j] + b * W2[3 * i + j];
      t += (I + c * W[3 * i + j] + d * W2[3 * i + j]) * v[j];
    }
    E[4 * i + 3] = t;
  }
}

// revo_map_align_plane_system's arithmetic: H = sum J J^T from its upper triangle, g = sum J e
inline void align_plane_system_fill(const revo_map_plane_info* info, double H[36], double g[6]) {
  const float* S = info->S;
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { H[i * 6 + j] = H[j * 6 + i] = (double)S[k]; ++k; }
  for (int i = 0; i < 6; ++i) g[i] = (double)S[21 + i];
}

// revo_map_df_align_system's arithmetic: the record carries the same 28 sums, so it is align_plane_system_fill's
inline void align_df_system_fill(const revo_map_df_align_info* info, double H[36], double g[6]) {
  const float* S = info->S;
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) { H[i * 6 + j] = H[j * 6 + i] = (double)S[k]; ++k; }
  for (int i = 0; i < 6; ++i) g[i] = (double)S[21 + i];
}

// The Gauss-Newton loop of revo_map_align, revo_map_align_plane and revo_map_df_align over records of type Rec (flags, matched) and their system
// fill(const Rec*, H, g).  eval(T column-major float[16], Rec*) -> 0 or an error code, which ends the loop and is returned.
template <class Rec, class Fill, class Eval>
inline int align_loop_over(const float T_init[16], const float centre[3], const revo_map_align_opts& o, Fill&& fill, Eval&& eval,
                           float T_out[16], Rec* rec_out, int* iterations, int* status) {
  double T[16], Tsys[16];  // row-major: the current pose, and the last pose that had a system
  for (int r = 0; r < 4; ++r)
    for (int col = 0; col < 4; ++col) T[4 * r + col] = (double)T_init[4 * col + r];
  memcpy(Tsys, T, sizeof(T));
  const double cx = centre[0], cy = centre[1], cz = centre[2];
  const double Cp[16] = {1, 0, 0, cx, 0, 1, 0, cy, 0, 0, 1, cz, 0, 0, 0, 1}, Cm[16] = {1, 0, 0, -cx, 0, 1, 0, -cy, 0, 0, 1, -cz, 0, 0, 0, 1};
  auto to_float = [](const double* M, float* F) {
    for (int r = 0; r < 4; ++r)
      for (int col = 0; col < 4; ++col) F[4 * col + r] = (float)M[4 * r + col];
  };
  int st = REVO_ALIGN_ITER_LIMIT, it = 0;
  Rec rec;
  float Tf[16];
  while (it < o.max_iters) {
    to_float(T, Tf);
    { const int rc = eval(Tf, &rec); if (rc) return rc; }
    double H[36], g[6], x[6];
    bool have = !(rec.flags & 1) && rec.matched >= o.min_matched;
    if (have) { fill(&rec, H, g); have = align_solve(H, g, x); }
    if (!have) {
      st = REVO_ALIGN_LOST;
      memcpy(T, Tsys, sizeof(T));
      break;
    }
    ++it;
    memcpy(Tsys, T, sizeof(T));
    double E[16], M[16];
    se3_exp_d(x, E);
    mat4_mul(Cp, E, M);
    mat4_mul(M, Cm, M);
    mat4_mul(M, T, T);
    double mv = 0.0, mw = 0.0;
    for (int i = 0; i < 3; ++i) { mv = std::max(mv, std::fabs(x[i])); mw = std::max(mw, std::fabs(x[3 + i])); }
    if (mv < o.eps_t && mw < o.eps_r) { st = REVO_ALIGN_CONVERGED; break; }
  }
  to_float(T, Tf);
  { const int rc = eval(Tf, &rec); if (rc) return rc; }
  memcpy(T_out, Tf, sizeof(Tf));
  if (rec_out) *rec_out = rec;
  if (iterations) *iterations = it;
  *status = st;
  return 0;
}

// align_loop_over turned inside out, for a caller that evaluates many loops' poses together (revo_map_tsdf_track_many):
// the same state (T, Tsys, it, status), the same arithmetic in the same order, but the caller feeds it one record at a time.
//   begin(T_init, centre, o);  while (s.wants()) { evaluate a record at s.pose(); s.feed(record, fill); }
// then pose() is T_out, rec the closing record, it and st the iterations and the status.  The records it asks for are
// align_loop_over's evaluations, one for one: `evals` of them, it + 1, or it + 2 when the status is LOST.
// tests/cpp/align_stepper_host.cpp holds the two against each other.
template <class Rec>
struct AlignStepper {
  double T[16], Tsys[16], Cp[16], Cm[16];
  revo_map_align_opts o;
  int it, st, evals;
  int phase;  // 0: the next record is an iteration's; 1: the next record is the closing one; 2: done
  float Tf[16];
  Rec rec;

  void begin(const float T_init[16], const float centre[3], const revo_map_align_opts& opts) {
    for (int r = 0; r < 4; ++r)
      for (int col = 0; col < 4; ++col) T[4 * r + col] = (double)T_init[4 * col + r];
    memcpy(Tsys, T, sizeof(T));
    const double cx = centre[0], cy = centre[1], cz = centre[2];
    const double cp[16] = {1, 0, 0, cx, 0, 1, 0, cy, 0, 0, 1, cz, 0, 0, 0, 1}, cm[16] = {1, 0, 0, -cx, 0, 1, 0, -cy, 0, 0, 1, -cz, 0, 0, 0, 1};
    memcpy(Cp, cp, sizeof(cp));
    memcpy(Cm, cm, sizeof(cm));
    o = opts;
    st = REVO_ALIGN_ITER_LIMIT; it = 0; evals = 0;
    phase = it < o.max_iters ? 0 : 1;
    to_float();
  }
  bool wants() const { return phase != 2; }
  const float* pose() const { return Tf; }  // column-major: where the next record is wanted; T_out once nothing is
  template <class Fill>
  void feed(const Rec& r, Fill&& fill) {
    rec = r;
    ++evals;
    if (phase == 1) { phase = 2; return; }
    double H[36], g[6], x[6];
    bool have = !(rec.flags & 1) && rec.matched >= o.min_matched;
    if (have) { fill(&rec, H, g); have = align_solve(H, g, x); }
    if (!have) {
      st = REVO_ALIGN_LOST;
      memcpy(T, Tsys, sizeof(T));
      phase = 1;
      to_float();
      return;
    }
    ++it;
    memcpy(Tsys, T, sizeof(T));
    double E[16], M[16];
    se3_exp_d(x, E);
    mat4_mul(Cp, E, M);
    mat4_mul(M, Cm, M);
    mat4_mul(M, T, T);
    double mv = 0.0, mw = 0.0;
    for (int i = 0; i < 3; ++i) { mv = std::max(mv, std::fabs(x[i])); mw = std::max(mw, std::fabs(x[3 + i])); }
    if (mv < o.eps_t && mw < o.eps_r) { st = REVO_ALIGN_CONVERGED; phase = 1; }
    else if (!(it < o.max_iters)) phase = 1;
    to_float();
  }

 private:
  void to_float() {
    for (int r = 0; r < 4; ++r)
      for (int col = 0; col < 4; ++col) Tf[4 * col + r] = (float)T[4 * r + col];
  }
};

// revo_map_align's loop: point-to-point records
template <class Eval>
inline int align_loop(const float T_init[16], const float centre[3], const revo_map_align_opts& o, Eval&& eval, float T_out[16],
                      revo_map_align_info* rec_out, int* iterations, int* status) {
  return align_loop_over<revo_map_align_info>(T_init, centre, o, align_system_fill, eval, T_out, rec_out, iterations, status);
}
