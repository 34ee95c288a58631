// revo_mat4.h -- column-major 4x4 float helpers shared by the host code (the units over revo_host_impl.h, revo_vo.hip, revo_vo_multi.hip).
// Eigen semantics: Matrix4f::inverse() is the general cofactor inverse in float (tracker.cpp:142,
// imgpyramidrgbd.h:129), products accumulate left to right.
#pragma once
#include <cstring>

static inline void mat4_inverse(const float* m, float* inv) {
  float o[16];
  o[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
  o[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
  o[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
  o[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
  o[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
  o[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
  o[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
  o[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
  o[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
  o[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
  o[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
  o[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
  o[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
  o[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
  o[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
  o[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
  const float det = m[0] * o[0] + m[1] * o[4] + m[2] * o[8] + m[3] * o[12];
  const float idet = 1.0f / det;
  for (int i = 0; i < 16; ++i) inv[i] = o[i] * idet;
}
static inline void mat4_mul(const float* A, const float* B, float* out) {
  float o[16];
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r)
      o[c * 4 + r] = A[0 * 4 + r] * B[c * 4 + 0] + A[1 * 4 + r] * B[c * 4 + 1] + A[2 * 4 + r] * B[c * 4 + 2] + A[3 * 4 + r] * B[c * 4 + 3];
  memcpy(out, o, sizeof(o));
}

// The pose arithmetic of the two VO drivers (revo_vo.hip, revo_vo_multi.hip): one copy, so that both compute the same bits.
struct M4 {  // column-major 4x4, Eigen::Matrix4f storage
  float m[16];
  static M4 identity() { M4 o; memset(o.m, 0, sizeof(o.m)); o.m[0] = o.m[5] = o.m[10] = o.m[15] = 1.f; return o; }
};
static inline M4 mul(const M4& A, const M4& B) { M4 o; mat4_mul(A.m, B.m, o.m); return o; }
static inline M4 inverse(const M4& A) { M4 o; mat4_inverse(A.m, o.m); return o; }  // Eigen Matrix4f::inverse()
static inline M4 from_RT(const float* R, const float* T) {  // transformFromRT
  M4 o = M4::identity();
  for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) o.m[c * 4 + r] = R[c * 3 + r];
  o.m[12] = T[0]; o.m[13] = T[1]; o.m[14] = T[2];
  return o;
}
static inline void to_RT(const M4& M, float* R, float* T) {
  for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) R[c * 3 + r] = M.m[c * 4 + r];
  T[0] = M.m[12]; T[1] = M.m[13]; T[2] = M.m[14];
}
struct Pose { M4 T_kf_curr, T_w_kf; M4 world() const { return mul(T_w_kf, T_kf_curr); } };  // REVO::Pose, system.h:89-152
