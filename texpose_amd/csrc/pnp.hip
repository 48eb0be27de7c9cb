// K28 batched PnP-RANSAC: poses from dense 2D-3D correspondence (NOCS) maps (the public functions are in
// texpose_amd/pnp.py, the rules in include/texpose_amd.h).
//
//   tp_corr_from_nocs   map -> dense correspondence list in scan order: wave ballots, per-tile counts, prefix sums (no atomic cursor)
//   tp_pnp_hypotheses   one thread per hypothesis: four distinct Philox indices, P3P in fp64 (Grunert's quartic, Ferrari + Newton)
//   tp_pnp_score        the hot kernel: a workgroup keeps 1024 points in registers and walks all T poses (scalar loads); per pose a
//                       ballot + popcount, integer LDS sums across the waves, one integer atomic per (workgroup, pose); the inlier
//                       mask of one chosen pose per image is a small launch of its own
//   tp_pnp_refine       selection, then Gauss-Newton in fp64: a reduce launch (fixed-order partial sums into the workspace) and a
//                       solve launch per step, keep-best, one final evaluation; the block reduce, the record gather and the step
//                       are pose_gn.h's, shared with K29 and K30
// Integer atomics only; every fp64 sum has one fixed order, so all outputs are a function of the inputs alone.
#include "tp_common.h"
#include "pose_gn.h"
#include <math.h>

namespace {
constexpr int kBlock = 256, kWaves = kBlock / tp::kWave;
constexpr int kCorrTile = kBlock;                      // pixels per workgroup of tp_corr_from_nocs
constexpr int kPts = 4, kTile = kBlock * kPts;         // points per workgroup of the score and reduce kernels
constexpr int kState = 32;                             // doubles per image: cur [12], best [12], best cost, best count, status, n, frozen
constexpr int S_CUR = 0, S_BEST = 12, S_COST = 24, S_COUNT = 25, S_STATUS = 26, S_N = 27, S_FROZEN = 28;
constexpr double kLambda = 1e-3;                      // the damping handed to pose_gn.h's step

__host__ __device__ inline int64_t tiles_of(int64_t n, int tile) { return (n + tile - 1) / tile; }
__device__ __forceinline__ int clamped_count(const int32_t* count, int b, int N) {
  const int n = count[b];
  return n < 0 ? 0 : (n > N ? N : n);
}
__device__ __forceinline__ int lane_id() { return threadIdx.x & (tp::kWave - 1); }
__device__ __forceinline__ int rank_below(unsigned long long ballot) {          // set bits of the lanes below this one
  return __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// ---------------------------------------------------------------------------------------------------------------- corr_from_nocs
struct CorrP {
  const float* nocs; const void* mask; int mask_is_float;
  float ct[3], sc[3];
  int B, H, W, stride, Ws, N, tiles;
  float* xy; float* xyz; int32_t* count; int32_t* tile_count;
};

__device__ __forceinline__ bool corr_keep(const CorrP& p, int b, int64_t k64, int& r, int& j, float (&q)[3]) {
  if (k64 >= p.N) return false;                                                  // (formed in 64 bits: N may be within a tile of 2^31)
  const int k = (int)k64;
  r = (k / p.Ws) * p.stride;
  j = (k % p.Ws) * p.stride;
  const int64_t pix = ((int64_t)b * p.H + r) * p.W + j;
  const bool m = p.mask_is_float ? (static_cast<const float*>(p.mask)[pix] != 0.f) : (static_cast<const uint8_t*>(p.mask)[pix] != 0);
  if (!m) return false;
  q[0] = p.nocs[3 * pix]; q[1] = p.nocs[3 * pix + 1]; q[2] = p.nocs[3 * pix + 2];
  return isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]);
}

// grid (tiles, B)
__global__ __launch_bounds__(kBlock) void corr_count_kernel(CorrP p) {
  __shared__ int wave_n[kWaves];
  const int b = blockIdx.y, tile = blockIdx.x;
  int r = 0, j = 0;
  float q[3];
  const bool keep = corr_keep(p, b, (int64_t)tile * kCorrTile + (int)threadIdx.x, r, j, q);
  const unsigned long long ballot = __ballot(keep);
  if (lane_id() == 0) wave_n[threadIdx.x / tp::kWave] = __popcll(ballot);
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int w = 0; w < kWaves; ++w) n += wave_n[w];
    p.tile_count[(int64_t)b * p.tiles + tile] = n;
  }
}

__global__ __launch_bounds__(kBlock) void corr_write_kernel(CorrP p) {
  __shared__ int wave_n[kWaves];
  __shared__ int before;
  const int b = blockIdx.y, tile = blockIdx.x;
  if (threadIdx.x == 0) before = 0;
  __syncthreads();
  int part = 0;
  for (int t = threadIdx.x; t < tile; t += kBlock) part += p.tile_count[(int64_t)b * p.tiles + t];
  if (part) atomicAdd(&before, part);                                            // (integers in LDS: the order does not matter)
  int r = 0, j = 0;
  float q[3] = {0.f, 0.f, 0.f};
  const bool keep = corr_keep(p, b, (int64_t)tile * kCorrTile + (int)threadIdx.x, r, j, q);
  const unsigned long long ballot = __ballot(keep);
  const int wave = threadIdx.x / tp::kWave;
  if (lane_id() == 0) wave_n[wave] = __popcll(ballot);
  __syncthreads();
  int o = before, total = 0;
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) o += wave_n[w];
    total += wave_n[w];
  }
  if (keep) {
    o += rank_below(ballot);                                                     // < N: at most one entry per strided pixel
    float* xy = p.xy + ((int64_t)b * p.N + o) * 2;
    float* xyz = p.xyz + ((int64_t)b * p.N + o) * 3;
    xy[0] = (float)j + 0.5f;
    xy[1] = (float)r + 0.5f;
    for (int c = 0; c < 3; ++c) xyz[c] = (2.0f * q[c] - 1.0f) * p.sc[c] + p.ct[c];
  }
  if (tile == p.tiles - 1 && threadIdx.x == 0) p.count[b] = before + total;
}

// ---------------------------------------------------------------------------------------------------------------- hypotheses
// real roots of y^2 + B y + C (a discriminant that is negative by rounding alone counts as zero)
__device__ __forceinline__ int quadratic_roots(double B, double C, double* y) {
  double disc = B * B - 4.0 * C;
  if (disc < 0.0 && disc > -1e-10 * (B * B + 4.0 * fabs(C))) disc = 0.0;
  if (!(disc >= 0.0)) return 0;
  const double qq = -0.5 * (B + copysign(sqrt(disc), B));
  y[0] = qq;
  y[1] = qq != 0.0 ? C / qq : 0.0;
  return 2;
}

// real roots of a4 x^4 + .. + a0: Ferrari through the largest root of the resolvent cubic, then two Newton steps on the quartic
__device__ int quartic_roots(double a4, double a3, double a2, double a1, double a0, double* x) {
  if (!(fabs(a4) > 0.0)) return 0;
  const double b = a3 / a4, c = a2 / a4, d = a1 / a4, e = a0 / a4;
  if (!isfinite(((b + c) + d) + e)) return 0;
  const double b2 = b * b;
  const double p = c - 0.375 * b2;
  const double q = (d - 0.5 * b * c) + 0.125 * b2 * b;
  const double r = ((e - 0.25 * b * d) + 0.0625 * b2 * c) - (3.0 / 256.0) * b2 * b2;
  // m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8 = 0 has a root m >= 0; with it the quartic is a difference of two squares
  const double c2 = p, c1 = 0.25 * p * p - r, c0 = -0.125 * q * q;
  const double P = c1 - c2 * c2 / 3.0, Q = (2.0 * c2 * c2 * c2 / 27.0 - c2 * c1 / 3.0) + c0;
  const double D = 0.25 * Q * Q + P * P * P / 27.0;
  double t = 0.0;
  if (D > 0.0) {
    const double s = sqrt(D);
    t = cbrt(-0.5 * Q + s) + cbrt(-0.5 * Q - s);
  } else if (P < 0.0) {
    const double k = sqrt(-P / 3.0);
    double arg = (1.5 * Q / P) / k;
    arg = arg > 1.0 ? 1.0 : (arg < -1.0 ? -1.0 : arg);
    t = 2.0 * k * cos(acos(arg) / 3.0);
  }
  double m = t - c2 / 3.0;
  for (int it = 0; it < 3; ++it) {
    const double f = ((m + c2) * m + c1) * m + c0, fp = (3.0 * m + 2.0 * c2) * m + c1;
    if (fp != 0.0 && isfinite(f / fp)) m -= f / fp;
  }
  int n = 0;
  double y[4];
  if (m > 1e-14 * (fabs(p) + sqrt(fabs(r)) + 1e-300)) {
    const double s = sqrt(2.0 * m), h = q / (2.0 * s);
    n += quadratic_roots(-s, (0.5 * p + m) + h, y + n);
    n += quadratic_roots(s, (0.5 * p + m) - h, y + n);
  } else {                                              // biquadratic: y^4 + p y^2 + r
    double z[2];
    const int nz = quadratic_roots(p, r, z);
    for (int k = 0; k < nz; ++k)
      if (z[k] >= 0.0) { y[n++] = sqrt(z[k]); y[n++] = -sqrt(z[k]); }
  }
  for (int k = 0; k < n; ++k) {
    double v = y[k] - 0.25 * b;
    for (int it = 0; it < 2; ++it) {
      const double f = (((v + b) * v + c) * v + d) * v + e, fp = ((4.0 * v + 3.0 * b) * v + 2.0 * c) * v + d;
      if (fp != 0.0 && isfinite(f / fp)) v -= f / fp;
    }
    x[k] = v;
  }
  return n;
}

// grid (ceil(T / 64), B), one thread per hypothesis
__global__ __launch_bounds__(tp::kWave) void pnp_hypotheses_kernel(tp_pnp_hypotheses_args a) {
  const int b = blockIdx.y, h = blockIdx.x * tp::kWave + threadIdx.x;
  if (h >= a.T) return;
  const int64_t bh = (int64_t)b * a.T + h;
  int32_t* idx_out = a.sample_idx + bh * 4;
  float* out = a.hyp + bh * 12;
  for (int k = 0; k < 12; ++k) out[k] = 0.f;
  a.hyp_valid[bh] = 0;
  const int n = clamped_count(a.count, b, a.N);
  if (n < 4) {
    for (int k = 0; k < 4; ++k) idx_out[k] = -1;
    return;
  }
  const uint4 w = tp::philox4x32_10(make_uint4((uint32_t)b, (uint32_t)h, 0x706E7034u, 0u), make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32)));
  int i0 = (int)__umulhi(w.x, (uint32_t)n);
  int i1 = (int)__umulhi(w.y, (uint32_t)(n - 1));
  int i2 = (int)__umulhi(w.z, (uint32_t)(n - 2));
  int i3 = (int)__umulhi(w.w, (uint32_t)(n - 3));
  if (i1 >= i0) ++i1;
  int s0 = i0 < i1 ? i0 : i1, s1 = i0 < i1 ? i1 : i0;                           // the earlier indices, ascending
  if (i2 >= s0) ++i2;
  if (i2 >= s1) ++i2;
  int s2 = i2;                                                                   // insert i2
  if (s2 < s0) { const int t = s0; s0 = s2; s2 = t; }
  if (s2 < s1) { const int t = s1; s1 = s2; s2 = t; }
  if (i3 >= s0) ++i3;
  if (i3 >= s1) ++i3;
  if (i3 >= s2) ++i3;
  const int idx[4] = {i0, i1, i2, i3};                                           // each in [0, n): n <= N
  for (int k = 0; k < 4; ++k) idx_out[k] = idx[k];

  const float* K = a.intr + (int64_t)b * 9;
  const double fx = (double)K[0], fy = (double)K[4], cx = (double)K[2], cy = (double)K[5];
  double u[4], v[4];
  V3 X[4];
  bool finite = isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy);
  for (int k = 0; k < 4; ++k) {
    const float* pxy = a.xy + ((int64_t)b * a.N + idx[k]) * 2;
    const float* pX = a.xyz + ((int64_t)b * a.N + idx[k]) * 3;
    u[k] = (double)pxy[0]; v[k] = (double)pxy[1];
    X[k] = {(double)pX[0], (double)pX[1], (double)pX[2]};
    finite = finite && isfinite(pxy[0]) && isfinite(pxy[1]) && isfinite(pX[0]) && isfinite(pX[1]) && isfinite(pX[2]);
  }
  if (!finite) return;
  const double e12x = u[1] - u[0], e12y = v[1] - v[0], e13x = u[2] - u[0], e13y = v[2] - v[0];
  const double area2 = fabs(e12x * e13y - e13x * e12y);
  if (!(area2 > 1e-9 * ((e12x * e12x + e12y * e12y) + (e13x * e13x + e13y * e13y)))) return;
  V3 f[3];
  for (int k = 0; k < 3; ++k) f[k] = unit(V3{(u[k] - cx) / fx, (v[k] - cy) / fy, 1.0});
  const V3 d23 = X[1] - X[2], d13 = X[0] - X[2], d12 = X[0] - X[1];
  const double a2 = dot(d23, d23), b2 = dot(d13, d13), c2 = dot(d12, d12);
  const double ca = dot(f[1], f[2]), cb = dot(f[0], f[2]), cg = dot(f[0], f[1]);
  const double k1 = (a2 - c2) / b2, kc = c2 / b2;
  // u = Nn(v) / Dd(v);  Nn^2 - 2 cos g Nn Dd + Dd^2 (1 - kc (1 - 2 cos b v + v^2)) = 0
  const double n0 = 1.0 + k1, n1 = -2.0 * k1 * cb, n2 = k1 - 1.0;
  const double d0 = 2.0 * cg, d1 = -2.0 * ca;
  const double w0 = 1.0 - kc, w1 = 2.0 * kc * cb, w2 = -kc;
  const double e0 = d0 * d0, e1 = 2.0 * d0 * d1, e2 = d1 * d1;
  const double A0 = (n0 * n0 - 2.0 * cg * (n0 * d0)) + e0 * w0;
  const double A1 = (2.0 * n0 * n1 - 2.0 * cg * (n0 * d1 + n1 * d0)) + (e0 * w1 + e1 * w0);
  const double A2 = ((n1 * n1 + 2.0 * n0 * n2) - 2.0 * cg * (n1 * d1 + n2 * d0)) + ((e0 * w2 + e1 * w1) + e2 * w0);
  const double A3 = (2.0 * n1 * n2 - 2.0 * cg * (n2 * d1)) + (e1 * w2 + e2 * w1);
  const double A4 = n2 * n2 + e2 * w2;
  double roots[4];
  const int nr = quartic_roots(A4, A3, A2, A1, A0, roots);
  // the model triangle's frame
  const V3 m1 = unit(X[1] - X[0]);
  const V3 m3 = unit(cross(X[1] - X[0], X[2] - X[0]));
  const V3 m2 = cross(m3, m1);
  double best_err = 0.0, best_v = 0.0, best[12];
  bool have = false;
  for (int k = 0; k < nr; ++k) {
    const double vv = roots[k];
    if (!(vv > 0.0) || !isfinite(vv)) continue;
    const double uu = ((n2 * vv + n1) * vv + n0) / (d0 + d1 * vv);
    if (!(uu > 0.0) || !isfinite(uu)) continue;
    const double s1 = sqrt(b2 / ((1.0 + vv * vv) - 2.0 * vv * cb));
    if (!(s1 > 0.0) || !isfinite(s1)) continue;
    // two Newton steps on the three distance equations themselves: the quartic's coefficients cancel where two roots are close
    double d1s = s1, d2s = uu * s1, d3s = vv * s1;
    for (int it = 0; it < 2; ++it) {
      const double F1 = ((d2s * d2s + d3s * d3s) - 2.0 * d2s * d3s * ca) - a2;
      const double F2 = ((d1s * d1s + d3s * d3s) - 2.0 * d1s * d3s * cb) - b2;
      const double F3 = ((d1s * d1s + d2s * d2s) - 2.0 * d1s * d2s * cg) - c2;
      const double j12 = 2.0 * (d2s - d3s * ca), j13 = 2.0 * (d3s - d2s * ca);
      const double j21 = 2.0 * (d1s - d3s * cb), j23 = 2.0 * (d3s - d1s * cb);
      const double j31 = 2.0 * (d1s - d2s * cg), j32 = 2.0 * (d2s - d1s * cg);
      const double det = j12 * j23 * j31 + j13 * j21 * j32;                       // rows (0, j12, j13), (j21, 0, j23), (j31, j32, 0)
      const double e1s = ((-j23 * j32) * F1 + (j13 * j32) * F2 + (j12 * j23) * F3) / det;
      const double e2s = ((j23 * j31) * F1 + (-j13 * j31) * F2 + (j13 * j21) * F3) / det;
      const double e3s = ((j21 * j32) * F1 + (j12 * j31) * F2 + (-j12 * j21) * F3) / det;
      const double n1s = d1s - e1s, n2s = d2s - e2s, n3s = d3s - e3s;
      if (!(isfinite(n1s) && isfinite(n2s) && isfinite(n3s) && n1s > 0.0 && n2s > 0.0 && n3s > 0.0)) break;
      d1s = n1s; d2s = n2s; d3s = n3s;
    }
    const V3 P0 = scaled(f[0], d1s), P1 = scaled(f[1], d2s), P2 = scaled(f[2], d3s);
    const V3 g1 = unit(P1 - P0);
    const V3 g3 = unit(cross(P1 - P0, P2 - P0));
    const V3 g2 = cross(g3, g1);
    double R[9] = {(g1.x * m1.x + g2.x * m2.x) + g3.x * m3.x, (g1.x * m1.y + g2.x * m2.y) + g3.x * m3.y, (g1.x * m1.z + g2.x * m2.z) + g3.x * m3.z,
                   (g1.y * m1.x + g2.y * m2.x) + g3.y * m3.x, (g1.y * m1.y + g2.y * m2.y) + g3.y * m3.y, (g1.y * m1.z + g2.y * m2.z) + g3.y * m3.z,
                   (g1.z * m1.x + g2.z * m2.x) + g3.z * m3.x, (g1.z * m1.y + g2.z * m2.y) + g3.z * m3.y, (g1.z * m1.z + g2.z * m2.z) + g3.z * m3.z};
    const double tx = P0.x - ((R[0] * X[0].x + R[1] * X[0].y) + R[2] * X[0].z);
    const double ty = P0.y - ((R[3] * X[0].x + R[4] * X[0].y) + R[5] * X[0].z);
    const double tz = P0.z - ((R[6] * X[0].x + R[7] * X[0].y) + R[8] * X[0].z);
    bool ok = isfinite(tx) && isfinite(ty) && isfinite(tz);
    for (int c = 0; c < 9; ++c) ok = ok && isfinite(R[c]);
    if (!ok) continue;
    const double x4 = ((R[0] * X[3].x + R[1] * X[3].y) + R[2] * X[3].z) + tx;
    const double y4 = ((R[3] * X[3].x + R[4] * X[3].y) + R[5] * X[3].z) + ty;
    const double z4 = ((R[6] * X[3].x + R[7] * X[3].y) + R[8] * X[3].z) + tz;
    double err = INFINITY;
    if (z4 > 0.0) {
      const double du = (fx * x4 / z4 + cx) - u[3], dv = (fy * y4 / z4 + cy) - v[3];
      err = du * du + dv * dv;
      if (!isfinite(err)) err = INFINITY;
    }
    if (!have || err < best_err || (err == best_err && vv < best_v)) {
      have = true; best_err = err; best_v = vv;
      for (int c = 0; c < 3; ++c) { best[4 * c] = R[3 * c]; best[4 * c + 1] = R[3 * c + 1]; best[4 * c + 2] = R[3 * c + 2]; }
      best[3] = tx; best[7] = ty; best[11] = tz;
    }
  }
  if (!have) return;
  bool ok = true;
  for (int k = 0; k < 12; ++k) ok = ok && isfinite((float)best[k]);
  if (!ok) return;
  for (int k = 0; k < 12; ++k) out[k] = (float)best[k];
  a.hyp_valid[bh] = 1;
}

// ---------------------------------------------------------------------------------------------------------------- score
__global__ __launch_bounds__(kBlock) void pnp_zero_kernel(int32_t* p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) p[i] = 0;
}

// the contract's test of one entry against one pose, fp32 as written
__device__ __forceinline__ bool pnp_inlier(const float (&P)[12], float fx, float fy, float cx, float cy, float tau2, float u, float v, float X,
                                           float Y, float Z) {
  const float x = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
  const float y = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
  const float z = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
  const float du = (__fdiv_rn(fx * x, z) + cx) - u, dv = (__fdiv_rn(fy * y, z) + cy) - v;
  return (z > 0.f) & (z <= 3.402823466e+38f) & (du * du + dv * dv <= tau2);          // (no short circuit: straight-line code)
}

// grid (ceil(N / 1024), B).  The kernel stores to LDS and, after the loop, through integer atomics only: nothing it writes can alias
// the poses, so the compiler keeps the uniform pose loads on the scalar unit (s_load_dwordx8 + s_load_dwordx4 per pose in the ISA).  The
// inlier mask of a chosen pose is a launch of its own (pnp_mask_kernel) for that reason: a byte store in this loop turned them into
// vector loads with a full wait per pose.
__global__ __launch_bounds__(kBlock) void pnp_score_kernel(const float* __restrict__ xy, const float* __restrict__ xyz, const int32_t* __restrict__ count,
                                                           const float* __restrict__ intr, const float* __restrict__ all_poses,
                                                           const uint8_t* __restrict__ all_valid, int N, int T, float tau_px, int32_t* inliers) {
  __shared__ int acc[TP_PNP_MAX_HYP];
  const int b = blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const int n = clamped_count(count, b, N);
  if (base >= n) return;                                                         // (uniform)
  for (int h = threadIdx.x; h < T; h += kBlock) acc[h] = 0;
  float u[kPts], v[kPts], X[kPts], Y[kPts], Z[kPts];
  bool live[kPts];
#pragma unroll
  for (int k = 0; k < kPts; ++k) {
    const int64_t i = base + k * kBlock + (int)threadIdx.x;
    live[k] = i < n;
    const int64_t o = (int64_t)b * N + (live[k] ? i : 0);
    u[k] = xy[o * 2]; v[k] = xy[o * 2 + 1];
    X[k] = xyz[o * 3]; Y[k] = xyz[o * 3 + 1]; Z[k] = xyz[o * 3 + 2];
  }
  const float* K = intr + (int64_t)b * 9;
  const float fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  const float tau2 = tau_px * tau_px;
  __syncthreads();
  const float* poses = all_poses + (int64_t)b * T * 12;
  const uint8_t* valid = all_valid ? all_valid + (int64_t)b * T : nullptr;
  for (int h0 = 0; h0 < T; h0 += tp::kWave) {
    // the valid bytes of 64 poses as one ballot (gfx9 has no scalar byte load): a scalar mask, one vector load per 64 poses
    const int hl = h0 + lane_id();
    const unsigned long long todo = __ballot(hl < T && (!valid || valid[hl] != 0));
    for (int h = h0; h < h0 + tp::kWave; ++h) {                                  // h is uniform
      if (!((todo >> (h - h0)) & 1ull)) continue;
      float P[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) P[k] = poses[(int64_t)h * 12 + k];
      int c = 0;
#pragma unroll
      for (int k = 0; k < kPts; ++k) c += __popcll(__ballot(live[k] & pnp_inlier(P, fx, fy, cx, cy, tau2, u[k], v[k], X[k], Y[k], Z[k])));
      if (c && lane_id() == 0) atomicAdd(&acc[h], c);
    }
  }
  __syncthreads();
  for (int h = threadIdx.x; h < T; h += kBlock)
    if (acc[h]) atomicAdd(&inliers[(int64_t)b * T + h], acc[h]);
}

// grid (ceil(N / 256), B): inlier_mask[b, i] for the one pose sel[b]; every i < N is written
__global__ __launch_bounds__(kBlock) void pnp_mask_kernel(tp_pnp_score_args a) {
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.N) return;
  const int n = clamped_count(a.count, b, a.N);
  const int sel = a.sel ? a.sel[b] : -1;
  bool in = false;
  if (i < n && sel >= 0 && sel < a.T && (!a.valid || a.valid[(int64_t)b * a.T + sel])) {
    float P[12];
    for (int k = 0; k < 12; ++k) P[k] = a.poses[((int64_t)b * a.T + sel) * 12 + k];
    const float* K = a.intr + (int64_t)b * 9;
    const int64_t o = (int64_t)b * a.N + i;
    in = pnp_inlier(P, K[0], K[4], K[2], K[5], a.tau_px * a.tau_px, a.xy[o * 2], a.xy[o * 2 + 1], a.xyz[o * 3], a.xyz[o * 3 + 1], a.xyz[o * 3 + 2]);
  }
  a.inlier_mask[(int64_t)b * a.N + i] = in ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- refine
// grid B: the winner -> state
__global__ __launch_bounds__(kBlock) void pnp_select_kernel(tp_pnp_refine_args a, double* state) {
  __shared__ int best_c[kBlock], best_h[kBlock];
  const int b = blockIdx.x;
  int bc = -1, bh = 0x7fffffff;
  for (int h = threadIdx.x; h < a.T; h += kBlock) {                              // ascending h: a strict > keeps the lowest
    if (a.hyp_valid && !a.hyp_valid[(int64_t)b * a.T + h]) continue;
    const int c = a.hyp_inliers[(int64_t)b * a.T + h];
    if (c > bc) { bc = c; bh = h; }
  }
  best_c[threadIdx.x] = bc; best_h[threadIdx.x] = bh;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const int oc = best_c[threadIdx.x + s], oh = best_h[threadIdx.x + s];
      if (oc > best_c[threadIdx.x] || (oc == best_c[threadIdx.x] && oh < best_h[threadIdx.x])) { best_c[threadIdx.x] = oc; best_h[threadIdx.x] = oh; }
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  double* st = state + (int64_t)b * kState;
  const int n = clamped_count(a.count, b, a.N);
  const bool found = best_h[0] != 0x7fffffff;
  for (int k = 0; k < 12; ++k) {
    const double p = (n >= 4 && found) ? (double)a.hyp[((int64_t)b * a.T + best_h[0]) * 12 + k] : 0.0;
    st[S_CUR + k] = p; st[S_BEST + k] = p;
  }
  st[S_COST] = 0.0; st[S_COUNT] = -1.0;
  st[S_STATUS] = n < 4 ? 1.0 : (found ? 0.0 : 2.0);
  st[S_N] = (double)n;
  st[S_FROZEN] = 0.0;
}

// grid (ceil(N / 1024), B): the sums of the current pose over this workgroup's points -> part [b][tile][32]
__global__ __launch_bounds__(kBlock) void pnp_reduce_kernel(tp_pnp_refine_args a, const double* state, double* part, int G) {
  __shared__ double wave_part[kWaves][kGnPart];
  const int b = blockIdx.y;
  const int64_t base = (int64_t)blockIdx.x * kTile;
  const double* st = state + (int64_t)b * kState;
  const int status = (int)st[S_STATUS];
  if (status == 1 || status == 2) return;                                        // (uniform) nothing reads these partials
  const int n = (int)st[S_N];
  const float* K = a.intr + (int64_t)b * 9;
  const double fx = (double)K[0], fy = (double)K[4], cx = (double)K[2], cy = (double)K[5];
  const double tau2 = (double)a.tau_px * (double)a.tau_px;
  double s[kGnSums];
#pragma unroll
  for (int k = 0; k < kGnSums; ++k) s[k] = 0.0;
  bool any = false;
  for (int k = 0; k < kPts; ++k) {
    const int64_t i = base + k * kBlock + (int)threadIdx.x;
    if (i >= n) continue;
    const int64_t o = (int64_t)b * a.N + i;
    const double X = (double)a.xyz[o * 3], Y = (double)a.xyz[o * 3 + 1], Z = (double)a.xyz[o * 3 + 2];
    const double x = ((st[0] * X + st[1] * Y) + st[2] * Z) + st[3];
    const double y = ((st[4] * X + st[5] * Y) + st[6] * Z) + st[7];
    const double z = ((st[8] * X + st[9] * Y) + st[10] * Z) + st[11];
    if (!(z > 0.0) || !isfinite(z)) continue;
    const double iz = 1.0 / z;
    const double ru = (fx * x * iz + cx) - (double)a.xy[o * 2], rv = (fy * y * iz + cy) - (double)a.xy[o * 2 + 1];
    if (!(ru * ru + rv * rv <= tau2)) continue;
    const double xz = x * iz, yz = y * iz;
    const double ju[6] = {-fx * xz * yz, fx + fx * xz * xz, -fx * yz, fx * iz, 0.0, -fx * xz * iz};
    const double jv[6] = {-fy - fy * yz * yz, fy * xz * yz, fy * xz, 0.0, fy * iz, -fy * yz * iz};
    int e = 0;                                                                   // (both rows as one term per sum: not two gn_add_row)
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) s[e++] += ju[r] * ju[c] + jv[r] * jv[c];
#pragma unroll
    for (int r = 0; r < 6; ++r) s[21 + r] += ju[r] * ru + jv[r] * rv;
    s[27] += ru * ru + rv * rv;
    s[28] += 1.0;
    any = true;
  }
  gn_block_reduce(s, any, wave_part, part + ((int64_t)b * G + blockIdx.x) * kGnPart);
}

// grid B, one wave: the partials in ascending order, keep-best, then (unless `last`) one damped Gauss-Newton step; `last` writes the outputs
__global__ __launch_bounds__(tp::kWave) void pnp_solve_kernel(tp_pnp_refine_args a, double* state, const double* part, int G, int last) {
  __shared__ double sum[kGnPart], stage[kGnStage][kGnPart];
  const int b = blockIdx.x;
  double* st = state + (int64_t)b * kState;
  const int status = (int)st[S_STATUS];
  const bool dead = status == 1 || status == 2;
  if (!dead) gn_gather(part + (int64_t)b * G * kGnPart, G, stage, sum);          // (uniform; nothing wrote a dead image's records)
  if (threadIdx.x != 0) return;
  if (!dead && st[S_FROZEN] == 0.0) {
    const double count = sum[28], cost = sum[27];
    if (st[S_COUNT] < 0.0 || count > st[S_COUNT] || (count == st[S_COUNT] && cost < st[S_COST])) {
      for (int k = 0; k < 12; ++k) st[S_BEST + k] = st[S_CUR + k];
      st[S_COUNT] = count; st[S_COST] = cost;
    }
    if (!last) {
      double Pn[12];
      if (gn_step(sum, st + S_CUR, kLambda, Pn)) {
        for (int k = 0; k < 12; ++k) st[S_CUR + k] = Pn[k];
      } else {
        st[S_STATUS] = 3.0; st[S_FROZEN] = 1.0;
      }
    }
  }
  if (last) {
    const float nan = __int_as_float(0x7fc00000);
    for (int k = 0; k < 12; ++k) a.pose[(int64_t)b * 12 + k] = dead ? nan : (float)st[S_BEST + k];
    a.inliers[b] = dead ? 0 : (int)st[S_COUNT];
    a.rms[b] = dead ? nan : (float)sqrt(st[S_COST] / st[S_COUNT]);
    a.status[b] = (int)st[S_STATUS];
  }
}

bool sizes_ok(const char* who, int B, int N, int T) {
  if (B <= 0 || B > 65535 || N <= 0 || T <= 0 || T > TP_PNP_MAX_HYP) {
    tp::set_error("%s: bad sizes (B 1..65535, N > 0, T 1..%d)", who, TP_PNP_MAX_HYP);
    return false;
  }
  return true;
}
bool tau_ok(const char* who, float tau) {
  if (!(tau > 0.f) || !isfinite(tau)) { tp::set_error("%s: tau_px must be finite and positive", who); return false; }
  return true;
}
// workspace: state [B][32] doubles, partials [B][G][32] doubles, tile counts [B][ceil(N / 256)] int32
size_t state_bytes(int B) { return (size_t)B * kState * sizeof(double); }
size_t part_bytes(int B, int N) { return (size_t)B * (size_t)tiles_of(N, kTile) * kGnPart * sizeof(double); }
}  // namespace

extern "C" size_t tp_pnp_workspace_bytes(int B, int N, int T) {
  if (B <= 0 || N <= 0 || T <= 0) return 0;
  const size_t bytes = state_bytes(B) + part_bytes(B, N) + (size_t)B * (size_t)tiles_of(N, kCorrTile) * sizeof(int32_t);
  return (bytes + 15) & ~(size_t)15;
}

extern "C" int tp_corr_from_nocs(const tp_corr_from_nocs_args* a, tp_stream_t stream) {
  if (!a) { tp::set_error("tp_corr_from_nocs: null args"); return -1; }
  if (a->B <= 0 || a->B > 65535 || a->H <= 0 || a->W <= 0 || a->stride <= 0 || (int64_t)a->H * a->W > 0x7FFFFFFFll) {
    tp::set_error("tp_corr_from_nocs: bad sizes (B 1..65535, H > 0, W > 0, stride > 0, H * W < 2^31)");
    return -1;
  }
  if (!a->nocs || !a->mask || !a->xy || !a->xyz || !a->count || !a->workspace) { tp::set_error("tp_corr_from_nocs: null pointer"); return -1; }
  CorrP p;
  p.nocs = a->nocs; p.mask = a->mask; p.mask_is_float = a->mask_is_float;
  for (int c = 0; c < 3; ++c) { p.ct[c] = a->centre[c]; p.sc[c] = a->scale[c]; }
  p.B = a->B; p.H = a->H; p.W = a->W; p.stride = a->stride;
  const int Hs = (int)tiles_of(a->H, a->stride);
  p.Ws = (int)tiles_of(a->W, a->stride);
  p.N = Hs * p.Ws;
  p.tiles = (int)tiles_of(p.N, kCorrTile);
  p.xy = a->xy; p.xyz = a->xyz; p.count = a->count;
  p.tile_count = reinterpret_cast<int32_t*>(static_cast<char*>(a->workspace) + state_bytes(a->B) + part_bytes(a->B, p.N));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(corr_count_kernel, dim3(p.tiles, a->B), dim3(kBlock), 0, st, p);
  hipLaunchKernelGGL(corr_write_kernel, dim3(p.tiles, a->B), dim3(kBlock), 0, st, p);
  return tp::check_launch("tp_corr_from_nocs");
}

extern "C" int tp_pnp_hypotheses(const tp_pnp_hypotheses_args* a, tp_stream_t stream) {
  if (!a) { tp::set_error("tp_pnp_hypotheses: null args"); return -1; }
  if (!sizes_ok("tp_pnp_hypotheses", a->B, a->N, a->T)) return -1;
  if (!a->xy || !a->xyz || !a->count || !a->intr || !a->sample_idx || !a->hyp || !a->hyp_valid) { tp::set_error("tp_pnp_hypotheses: null pointer"); return -1; }
  hipLaunchKernelGGL(pnp_hypotheses_kernel, dim3((a->T + tp::kWave - 1) / tp::kWave, a->B), dim3(tp::kWave), 0, (hipStream_t)stream, *a);
  return tp::check_launch("tp_pnp_hypotheses");
}

extern "C" int tp_pnp_score(const tp_pnp_score_args* a, tp_stream_t stream) {
  if (!a) { tp::set_error("tp_pnp_score: null args"); return -1; }
  if (!sizes_ok("tp_pnp_score", a->B, a->N, a->T) || !tau_ok("tp_pnp_score", a->tau_px)) return -1;
  if (!a->xy || !a->xyz || !a->count || !a->intr || !a->poses || !a->inliers) { tp::set_error("tp_pnp_score: null pointer"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  const int64_t n = (int64_t)a->B * a->T;
  hipLaunchKernelGGL(pnp_zero_kernel, dim3((unsigned)tiles_of(n, kBlock)), dim3(kBlock), 0, st, a->inliers, n);
  hipLaunchKernelGGL(pnp_score_kernel, dim3((unsigned)tiles_of(a->N, kTile), a->B), dim3(kBlock), 0, st, a->xy, a->xyz, a->count, a->intr, a->poses,
                     a->valid, a->N, a->T, a->tau_px, a->inliers);
  if (a->inlier_mask) hipLaunchKernelGGL(pnp_mask_kernel, dim3((unsigned)tiles_of(a->N, kBlock), a->B), dim3(kBlock), 0, st, *a);
  return tp::check_launch("tp_pnp_score");
}

extern "C" int tp_pnp_refine(const tp_pnp_refine_args* a, tp_stream_t stream) {
  if (!a) { tp::set_error("tp_pnp_refine: null args"); return -1; }
  if (!sizes_ok("tp_pnp_refine", a->B, a->N, a->T) || !tau_ok("tp_pnp_refine", a->tau_px)) return -1;
  if (a->iters < 0 || a->iters > TP_PNP_MAX_ITERS) { tp::set_error("tp_pnp_refine: iters = %d, 0 .. %d expected", a->iters, TP_PNP_MAX_ITERS); return -1; }
  if (!a->xy || !a->xyz || !a->count || !a->intr || !a->hyp || !a->hyp_inliers || !a->pose || !a->inliers || !a->rms || !a->status || !a->workspace) {
    tp::set_error("tp_pnp_refine: null pointer");
    return -1;
  }
  if ((uintptr_t)a->workspace & 15u) { tp::set_error("tp_pnp_refine: workspace must be 16-byte aligned"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  double* state = static_cast<double*>(a->workspace);
  double* part = state + (int64_t)a->B * kState;
  const int G = (int)tiles_of(a->N, kTile);
  hipLaunchKernelGGL(pnp_select_kernel, dim3(a->B), dim3(kBlock), 0, st, *a, state);
  for (int it = 0; it <= a->iters; ++it) {
    hipLaunchKernelGGL(pnp_reduce_kernel, dim3(G, a->B), dim3(kBlock), 0, st, *a, (const double*)state, part, G);
    hipLaunchKernelGGL(pnp_solve_kernel, dim3(a->B), dim3(tp::kWave), 0, st, *a, state, (const double*)part, G, it == a->iters ? 1 : 0);
  }
  return tp::check_launch("tp_pnp_refine");
}
