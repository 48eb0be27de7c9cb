// The 6-parameter Gauss-Newton machinery that K28 (pnp.hip, reprojection residuals) and K29 (depth_icp.hip, point-to-plane residuals)
// share: fp64 3-vectors, the wave butterfly sum, the 6x6 Cholesky with the pivot rule, and one damped step of the update
// x' = x + w x x + v in the camera frame (parameters (w, v)) followed by the exponential map and Gram-Schmidt.  Everything is evaluated
// as written (the library is built without contraction): both users get the same bits from the same sums.
#pragma once
#include "tp_common.h"
#include <math.h>

namespace {
struct V3 { double x, y, z; };
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 scaled(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 unit(V3 a) { return scaled(a, 1.0 / sqrt(dot(a, a))); }

constexpr int kGnSums = 29;                            // 21 (J^T J, upper triangle, row-major) + 6 (J^T r) + sum |r|^2 + count
constexpr int kGnPart = 32;                            // doubles per partial record
constexpr double kGnPivotTol = 1e-10;

__device__ __forceinline__ double wave_sum(double v) {                           // butterfly: the same order, and the same sum, in every lane
  for (int m = 1; m < tp::kWave; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// wave_sum of K values at once, step-major: the K exchanges of a step are in flight together instead of K x 6 round trips one after
// the other; value by value the same additions in the same order as wave_sum, hence the same bits
template <int K>
__device__ __forceinline__ void wave_sum_all(double (&v)[K]) {
#pragma unroll
  for (int m = 1; m < tp::kWave; m <<= 1) {
    double o[K];
#pragma unroll
    for (int k = 0; k < K; ++k) o[k] = __shfl_xor(v[k], m);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += o[k];
  }
}

// Cholesky of the 6x6 matrix A (full storage, lower triangle written); false where a pivot is not finite or <= tol x its diagonal
__device__ bool cholesky6(double (&A)[6][6], double tol) {
  for (int j = 0; j < 6; ++j) {
    const double diag = A[j][j];
    double d = diag;
    for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
    if (!isfinite(d) || !(d > tol * diag) || !(d > 0.0)) return false;
    const double l = sqrt(d);
    A[j][j] = l;
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
      for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
      A[i][j] = v / l;
    }
  }
  return true;
}

// the 21 upper-triangle sums as a full symmetric matrix
__device__ __forceinline__ void gn_matrix(const double* sum, double (&A)[6][6]) {
  int e = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) { A[r][c] = A[c][r] = sum[e]; ++e; }
}

// One damped Gauss-Newton step from the 27 sums (21 of J^T J, then 6 of J^T r) at the pose cur [12] ([R|t] row-major):
// J^T J is factored by Cholesky with the pivot rule (not positive definite: false, Pn untouched), (J^T J + lambda diag J^T J) d = -J^T r
// is solved by Cholesky, R <- exp(w) R, t <- exp(w) t + v with Rodrigues' formula, Gram-Schmidt on R's first two columns, the third
// their cross product.  false also where the new pose is not finite.
__device__ bool gn_step(const double* sum, const double* cur, double lambda, double (&Pn)[12]) {
  double A[6][6], D[6][6];
  int e = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) { A[r][c] = A[c][r] = sum[e]; D[r][c] = D[c][r] = sum[e]; ++e; }
  for (int r = 0; r < 6; ++r) D[r][r] = A[r][r] + lambda * A[r][r];
  if (!cholesky6(A, kGnPivotTol) || !cholesky6(D, 0.0)) return false;
  double d[6];
  for (int i = 0; i < 6; ++i) {                                            // L y = -J^T r
    double v = -sum[21 + i];
    for (int k = 0; k < i; ++k) v -= D[i][k] * d[k];
    d[i] = v / D[i][i];
  }
  for (int i = 5; i >= 0; --i) {                                           // L^T d = y
    double v = d[i];
    for (int k = i + 1; k < 6; ++k) v -= D[k][i] * d[k];
    d[i] = v / D[i][i];
  }
  const double wx = d[0], wy = d[1], wz = d[2];
  const double th2 = (wx * wx + wy * wy) + wz * wz, th = sqrt(th2);
  const double sa = th > 1e-8 ? sin(th) / th : 1.0 - th2 / 6.0;
  const double sb = th > 1e-8 ? (1.0 - cos(th)) / th2 : 0.5 - th2 / 24.0;
  // exp(w) = I + sa [w]x + sb [w]x^2
  const double E[9] = {1.0 - sb * (wy * wy + wz * wz), -sa * wz + sb * wx * wy, sa * wy + sb * wx * wz,
                       sa * wz + sb * wx * wy, 1.0 - sb * (wx * wx + wz * wz), -sa * wx + sb * wy * wz,
                       -sa * wy + sb * wx * wz, sa * wx + sb * wy * wz, 1.0 - sb * (wx * wx + wy * wy)};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 4; ++c) Pn[4 * r + c] = (E[3 * r] * cur[c] + E[3 * r + 1] * cur[4 + c]) + E[3 * r + 2] * cur[8 + c];
    Pn[4 * r + 3] += d[3 + r];
  }
  V3 c1 = unit(V3{Pn[0], Pn[4], Pn[8]});
  V3 c2 = {Pn[1], Pn[5], Pn[9]};
  c2 = unit(c2 - scaled(c1, dot(c1, c2)));
  const V3 c3 = cross(c1, c2);
  Pn[0] = c1.x; Pn[4] = c1.y; Pn[8] = c1.z; Pn[1] = c2.x; Pn[5] = c2.y; Pn[9] = c2.z; Pn[2] = c3.x; Pn[6] = c3.y; Pn[10] = c3.z;
  bool ok = true;
  for (int k = 0; k < 12; ++k) ok = ok && isfinite(Pn[k]);
  return ok;
}
}  // namespace
