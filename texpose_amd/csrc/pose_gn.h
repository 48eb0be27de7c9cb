// The 6-parameter Gauss-Newton core of the three pose refiners: K28 (pnp.hip, reprojection residuals), K29 (depth_icp.hip, point-to-plane
// residuals) and K30 (photo_align.hip, colour residuals).  A refiner supplies its residual rows; everything after them is here:
//   - fp64 3-vectors, the wave butterfly sum, the 6x6 Cholesky with the pivot rule, and one damped step of the update
//     x' = x + w x x + v in the camera frame (parameters (w, v)) followed by the exponential map and Gram-Schmidt;
//   - the row accumulation into the 29 sums (gn_add_row), their reduction over a workgroup into one 32-double record
//     (gn_block_reduce) and the gather of an image's records in ascending tile order (gn_gather);
//   - for the pixel-tiled refiners K29 and K30: the tiling constants, the frame choice (gn_frame_of), the workspace size, the
//     step / evaluate kernel with its count, status and pass-through rules (gn_solve_kernel) and the host's argument checks.
// Everything is evaluated as written (the library is built without contraction) and every sum has one fixed order: all users get the
// same bits from the same sums, and their outputs are a function of the inputs alone.
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

// The wave's sum of each of K values by an xor butterfly (v += shfl_xor(v, 1), 2, 4 .. 32: the same order, and the same sum, in every
// lane), step-major: the K exchanges of a step are in flight together instead of K x 6 round trips one after the other; value by
// value the additions and their order are those of K butterflies run one at a time, hence the same bits
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

// ---------------------------------------------------------------------------------------------------------------- the 29 sums
// one residual row: the 21 products of J^T J's upper triangle, the 6 of J^T r and r^2, each added to its sum; the count is the caller's
__device__ __forceinline__ void gn_add_row(double (&s)[kGnSums], const double (&J)[6], double r) {
  int e = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int c = i; c < 6; ++c) s[e++] += J[i] * J[c];
#pragma unroll
  for (int i = 0; i < 6; ++i) s[21 + i] += J[i] * r;
  s[27] += r * r;
}

// The sums of a workgroup of WAVES waves -> record [32]: xor-butterfly inside the wave (step-major), lane 0 to LDS, the waves in
// ascending order by 29 threads.  `any`: this thread added something; a wave without one skips its butterflies and stores the
// 29 zeros (+0.0) they would have given.  Every thread of the workgroup must call it.
template <int WAVES>
__device__ __forceinline__ void gn_block_reduce(double (&s)[kGnSums], bool any, double (&wave_part)[WAVES][kGnPart], double* record) {
  const int lane = threadIdx.x & (tp::kWave - 1), wave = threadIdx.x / tp::kWave;
  if (__ballot(any) != 0ull) {                                                   // (uniform per wave)
    wave_sum_all(s);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < kGnSums; ++k) wave_part[wave][k] = s[k];
    }
  } else if (lane < kGnSums) {
    wave_part[wave][lane] = 0.0;
  }
  __syncthreads();
  if (threadIdx.x < kGnSums) {
    double t = wave_part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) t += wave_part[w][threadIdx.x];
    record[threadIdx.x] = t;
  }
}

constexpr int kGnStage = 64;                           // records gn_gather stages through LDS at a time

// One wave: the G records at rec -> sum [0 .. 28].  The records come through LDS 64 at a time as whole 512-byte rows (coalesced, 32
// loads in flight per thread); 29 threads add them in ascending tile order.  sum is ready for every thread on return.
__device__ __forceinline__ void gn_gather(const double* rec, int G, double (&stage)[kGnStage][kGnPart], double (&sum)[kGnPart]) {
  double t = 0.0;
  for (int g0 = 0; g0 < G; g0 += kGnStage) {
    const int n = G - g0 < kGnStage ? G - g0 : kGnStage;
    double v[kGnStage / 2];
#pragma unroll
    for (int u = 0; u < kGnStage / 2; ++u) {
      const int e = (int)threadIdx.x + tp::kWave * u;                            // element e of the batch: record e / 32, entry e % 32
      v[u] = e / kGnPart < n ? rec[(int64_t)g0 * kGnPart + e] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kGnStage / 2; ++u) (&stage[0][0])[(int)threadIdx.x + tp::kWave * u] = v[u];
    __syncthreads();
    if (threadIdx.x < kGnSums)
      for (int g = 0; g < n; ++g) t += stage[g][threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x < kGnSums) sum[threadIdx.x] = t;
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------- the pixel-tiled refiners
// K29 and K30: a workgroup of 256 threads owns a tile of 1024 flat pixels, four consecutive ones per thread; their args structs name
// the shared fields alike (B, Ft, H, W, frame, pose, damping, evaluate_only, pose_out, inliers, rms, status, workspace).
constexpr int kGnBlock = 256, kGnPix = 4, kGnTile = kGnBlock * kGnPix, kGnWaves = kGnBlock / tp::kWave;
constexpr int kGnMinCount = 6;

__host__ __device__ inline int64_t gn_tiles(int64_t n) { return (n + kGnTile - 1) / kGnTile; }
inline size_t gn_workspace_bytes(int B, int64_t tiles) {                         // one record per (image, tile)
  const size_t bytes = (size_t)B * (size_t)tiles * kGnPart * sizeof(double);
  return (bytes + 15) & ~(size_t)15;
}

// the measured plane of image b: the only one, its own, or frame[b] (out of range is the caller's error: clamped, never read past)
template <class Args>
__device__ __forceinline__ int gn_frame_of(const Args& a, int b) {
  int fr = a.Ft == 1 ? 0 : b;
  if (a.frame) {
    fr = a.frame[b];
    fr = fr < 0 ? 0 : (fr >= a.Ft ? a.Ft - 1 : fr);
  }
  return fr;
}

// The decision of a solve kernel's thread 0 on the 29 sums of one image at pose T: fewer than six kept pixels: status 1; with
// evaluate_only the pivot rule alone decides between 0 and 3; else one damped step, status 3 where it fails or leaves fp32's range.
// out: the stepped pose in fp32, or T bit for bit with evaluate_only or a non-zero status.  -> the status.
__device__ inline int gn_decide(const double* sum, const float* T, double damping, bool evaluate_only, float (&out)[12]) {
  int status = 0;
  double Pn[12];
  if (sum[28] < (double)kGnMinCount) {
    status = 1;
  } else if (evaluate_only) {
    double A[6][6];
    gn_matrix(sum, A);
    if (!cholesky6(A, kGnPivotTol)) status = 3;
  } else {
    double cur[12];
    for (int k = 0; k < 12; ++k) cur[k] = (double)T[k];
    bool ok = gn_step(sum, cur, damping, Pn);
    for (int k = 0; k < 12; ++k) ok = ok && isfinite((float)Pn[k]);
    if (!ok) status = 3;
  }
  const bool stepped = status == 0 && !evaluate_only;
  for (int k = 0; k < 12; ++k) out[k] = stepped ? (float)Pn[k] : T[k];
  return status;
}

// grid B, one wave: gathers the image's G records, then thread 0 decides (gn_decide).  inliers and rms (NaN without a pixel) are
// those of the pose that came in; pose_out is the stepped pose, or the input bit for bit.
template <class Args>
__global__ __launch_bounds__(tp::kWave) void gn_solve_kernel(Args a, const double* part, int G) {
  __shared__ double sum[kGnPart], stage[kGnStage][kGnPart];
  const int b = blockIdx.x;
  gn_gather(part + (int64_t)b * G * kGnPart, G, stage, sum);
  if (threadIdx.x != 0) return;
  const double count = sum[28];
  float out[12];
  const int status = gn_decide(sum, a.pose + (int64_t)b * 12, (double)a.damping, a.evaluate_only != 0, out);
  a.inliers[b] = (int)count;
  a.rms[b] = count > 0.0 ? (float)sqrt(sum[27] / count) : __int_as_float(0x7fc00000);
  a.status[b] = status;
  if (a.pose_out)
    for (int k = 0; k < 12; ++k) a.pose_out[(int64_t)b * 12 + k] = out[k];
}

// The host checks both step calls make after their own size check, in the order callers see them.  `tau` is the caller's threshold
// under the name `tau_word`; `missing`: one of the pointers the caller requires is null (each has its own list).
template <class Args>
bool gn_step_args_ok(const char* who, const Args& a, const char* tau_word, float tau, bool missing) {
  if (!a.frame && a.Ft != 1 && a.Ft != a.B) {
    tp::set_error("%s: Ft = %d is neither 1 nor B = %d and there is no frame map", who, a.Ft, a.B);
    return false;
  }
  if (!(tau > 0.f) || !isfinite(tau)) { tp::set_error("%s: %s must be finite and positive", who, tau_word); return false; }
  if (!(a.damping >= 0.f) || !isfinite(a.damping)) { tp::set_error("%s: damping must be finite and not negative", who); return false; }
  if (missing || !a.pose || !a.intr || !a.inliers || !a.rms || !a.status || !a.workspace || (!a.pose_out && !a.evaluate_only)) {
    tp::set_error("%s: null pointer", who);
    return false;
  }
  if ((uintptr_t)a.workspace & 15u) { tp::set_error("%s: workspace must be 16-byte aligned", who); return false; }
  if (a.pose_out) {
    const uintptr_t in = (uintptr_t)a.pose, out = (uintptr_t)a.pose_out, bytes = (uintptr_t)a.B * 12 * sizeof(float);
    if (in < out + bytes && out < in + bytes) { tp::set_error("%s: pose_out must not overlap pose", who); return false; }
  }
  return true;
}
}  // namespace
