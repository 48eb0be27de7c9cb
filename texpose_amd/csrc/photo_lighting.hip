// K40 tp_photo_lighting: per-image, per-channel first-order spherical-harmonic shading (ambient + directional) and a bias between B
// renderings and their photographs, and the renderings under that fit (the public function is ops.photo_lighting in
// texpose_amd/ops/refine.py, the rules in include/texpose_amd.h).  K37's sibling (photo_exposure.hip): the same tiling, load paths and
// order of sums, a record of 64 doubles in place of 32.
//
//   lighting_reduce grid (ceil(H * W / 1024), B) x 256: K37's reduce plus, per pixel that is still a candidate after the mask and the
//                   six colours, the face index, its three vertex indices (checked) and nine coordinates: the face's normal in the
//                   camera frame.  A thread first decides which of its four pixels are kept and holds their normals (12 doubles);
//                   then three passes, one per channel, of 21 fp64 sums over the same registers, each ended by its butterfly and
//                   lane 0's store to LDS: 21 live accumulators (and the butterfly's 21 partners) instead of 63 (section 30 has the
//                   resource table of both layouts).
//   lighting_solve  grid B x 64: thread t adds entry t of the image's records in ascending tile order (a gather of its own: gn_gather
//                   is 32 wide and stops at 29), threads 0 .. 2 solve one channel each (5 x 5 Cholesky, fully unrolled: no indexed
//                   private array), thread 0 decides the status and writes the outputs.
//   lighting_apply  grid (ceil(H * W / 1024), B) x 256, four pixels per thread; light[b] is wave-uniform.
// No atomics; every fp64 sum has one fixed order (K30's), so all outputs are a function of the inputs alone.
#include "tp_common.h"
#include "pose_gn.h"
#include "pose_terms.h"
#include "face_normal.h"

namespace {
constexpr int kLitRecord = 64;                         // n, then per channel 15 (x x^T, upper triangle, row-major) + 5 (x o) + o o
constexpr int kLitChannel = 21;
constexpr int kLitMinCount = 6;

__device__ __forceinline__ bool covered(float z) { return z > 0.f && isfinite(z); }

// One channel's 21 sums over the thread's kept pixels, the wave's butterfly and lane 0's store; the caller's wave has a kept pixel
template <int CH>
__device__ __forceinline__ void channel_pass(unsigned keep, const float (&cs)[kGnPix * 3], const float (&os)[kGnPix * 3], const V3 (&nrm)[kGnPix],
                                             double* wave_row) {
  double s[kLitChannel];
#pragma unroll
  for (int e = 0; e < kLitChannel; ++e) s[e] = 0.0;
#pragma unroll
  for (int k = 0; k < kGnPix; ++k) {
    if (!(keep >> k & 1u)) continue;
    const double c = (double)cs[3 * k + CH], o = (double)os[3 * k + CH];
    const double x[5] = {c, c * nrm[k].x, c * nrm[k].y, c * nrm[k].z, 1.0};
    int e = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
      for (int j = i; j < 5; ++j) s[e++] += x[i] * x[j];
#pragma unroll
    for (int i = 0; i < 5; ++i) s[15 + i] += x[i] * o;
    s[20] += o * o;
  }
  wave_sum_all(s);
  if ((threadIdx.x & (tp::kWave - 1)) == 0) {
#pragma unroll
    for (int e = 0; e < kLitChannel; ++e) wave_row[1 + kLitChannel * CH + e] = s[e];
  }
}

// VEC: H * W is a multiple of four and face / zbuf / rgb / image are 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kGnBlock) void lighting_reduce_kernel(tp_photo_lighting_args a, double* part) {
  __shared__ double wave_part[kGnWaves][kLitRecord];
  const int b = blockIdx.y;
  const int fr = gn_frame_of(a, b);
  const int64_t plane = (int64_t)a.H * a.W;
  const float* pz = a.zbuf + (int64_t)b * plane;
  const float* pc = a.rgb + (int64_t)b * plane * 3;
  const int32_t* pf = a.face + (int64_t)b * plane;
  const float* po = a.image + (int64_t)fr * plane * 3;
  const uint8_t* pm = a.mask ? a.mask + (int64_t)fr * plane : nullptr;
  const float* T = a.pose + (int64_t)b * 12;
  const double tau2 = (double)a.tau * (double)a.tau;

  const int64_t p0 = (int64_t)blockIdx.x * kGnTile + (int)threadIdx.x * kGnPix;            // (< H * W + 1024 < 2^31 + 1024)
  float zs[kGnPix];
  load_four<VEC, float, float4>(pz, p0, plane, -1.f, zs);

  // the interior pixels with a rendered surface (a pixel past the plane has i >= H)
  const int i0 = (int)((uint32_t)p0 / (uint32_t)a.W), j0 = (int)((uint32_t)p0 - (uint32_t)i0 * (uint32_t)a.W);
  unsigned cand = 0u;                                                            // bit k: pixel k is a candidate
  {
    int i = i0, j = j0;
#pragma unroll
    for (int k = 0; k < kGnPix; ++k) {
      if (i >= 1 && i <= a.H - 2 && j >= 1 && j <= a.W - 2 && covered(zs[k])) cand |= 1u << k;
      if (++j == a.W) { j = 0; ++i; }
    }
  }

  float cs[kGnPix * 3], os[kGnPix * 3];
  int fs[kGnPix];
#pragma unroll
  for (int k = 0; k < kGnPix * 3; ++k) { cs[k] = 0.f; os[k] = 0.f; }
#pragma unroll
  for (int k = 0; k < kGnPix; ++k) fs[k] = -1;
  if (cand != 0u) {
    if constexpr (VEC) {                                                         // (p0 * 12 bytes: a multiple of 48)
      const float4* c4 = reinterpret_cast<const float4*>(pc + p0 * 3);
      const float4* o4 = reinterpret_cast<const float4*>(po + p0 * 3);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const float4 c = c4[q], o = o4[q];
        cs[4 * q] = c.x; cs[4 * q + 1] = c.y; cs[4 * q + 2] = c.z; cs[4 * q + 3] = c.w;
        os[4 * q] = o.x; os[4 * q + 1] = o.y; os[4 * q + 2] = o.z; os[4 * q + 3] = o.w;
      }
      load_four<true, int, int4>(pf, p0, plane, -1, fs);
    } else {
#pragma unroll
      for (int k = 0; k < kGnPix; ++k)
        if (cand >> k & 1u) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) { cs[3 * k + ch] = pc[(p0 + k) * 3 + ch]; os[3 * k + ch] = po[(p0 + k) * 3 + ch]; }
          fs[k] = pf[p0 + k];
        }
    }
  }

  // which pixels are kept, and their normals
  V3 nrm[kGnPix];
  unsigned keep = 0u;
  if (cand != 0u) {
    double lin[15];
#pragma unroll
    for (int e = 0; e < 15; ++e) lin[e] = a.light_in ? (double)a.light_in[b * 15 + e] : (e % 5 == 0 ? 1.0 : 0.0);
#pragma unroll
    for (int k = 0; k < kGnPix; ++k) {
      nrm[k] = {0.0, 0.0, 0.0};
      if (!(cand >> k & 1u)) continue;
      if (pm && pm[p0 + k] == 0) continue;
      if (!(finite3(cs + 3 * k) && finite3(os + 3 * k))) continue;
      V3 n;
      if (!face_normal(a.verts, a.faces, a.V, a.F, fs[k], T, n)) continue;
      double res[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const double c = (double)cs[3 * k + ch], o = (double)os[3 * k + ch];
        const double* l = lin + 5 * ch;
        res[ch] = o - ((((l[0] * c + l[1] * (c * n.x)) + l[2] * (c * n.y)) + l[3] * (c * n.z)) + l[4]);
      }
      if (!((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2] <= tau2)) continue;
      nrm[k] = n;
      keep |= 1u << k;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kGnPix; ++k) nrm[k] = {0.0, 0.0, 0.0};
  }

  // the workgroup's sums -> one record: per channel a butterfly inside the wave and lane 0 to LDS, then the waves in ascending order; a
  // wave that kept nothing stores the zeros its butterflies would have given
  const int lane = threadIdx.x & (tp::kWave - 1), wave = threadIdx.x / tp::kWave;
  if (__ballot(keep != 0u) != 0ull) {                                            // (uniform per wave)
    double n1[1] = {(double)__popc(keep)};                                       // (+ 1 per kept pixel: exact)
    wave_sum_all(n1);
    if (lane == 0) wave_part[wave][0] = n1[0];
    channel_pass<0>(keep, cs, os, nrm, wave_part[wave]);
    channel_pass<1>(keep, cs, os, nrm, wave_part[wave]);
    channel_pass<2>(keep, cs, os, nrm, wave_part[wave]);
  } else {
    wave_part[wave][lane] = 0.0;                                                 // (64 lanes, 64 entries)
  }
  __syncthreads();
  if (threadIdx.x < kLitRecord) {
    double t = wave_part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kGnWaves; ++w) t += wave_part[w][threadIdx.x];
    part[((int64_t)b * gridDim.x + blockIdx.x) * kLitRecord + threadIdx.x] = t;
  }
}

// One channel of the solve: sums [21] (15 + 5 + 1) and n -> x [5], sse, the channel's flag bits (unshifted)
__device__ __forceinline__ void solve_channel(const double* s, double n, double lo, double hi, double min_var, double (&x)[5], double& sse, int& bits) {
  double A[5][5], L[5][5], r[5];
  {
    int e = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i)
#pragma unroll
      for (int j = i; j < 5; ++j) { A[i][j] = s[e]; A[j][i] = s[e]; L[i][j] = s[e]; L[j][i] = s[e]; ++e; }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) r[i] = s[15 + i];
  const double Soo = s[20];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 5; ++j) {                                                  // cholesky6's rule on 5 x 5, lower triangle written
    const double diag = L[j][j];
    double d = diag;
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    ok = ok && isfinite(d) && d > kGnPivotTol * diag && d > 0.0;
    const double l = sqrt(ok ? d : 1.0);                                         // (a failed factorisation's values are never used)
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 5; ++i) {
      double v = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v / l;
    }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {                                                  // L y = r
    double v = r[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i][k] * x[k];
    x[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = 4; i >= 0; --i) {                                                 // L^T x = y
    double v = x[i];
#pragma unroll
    for (int k = i + 1; k < 5; ++k) v -= L[k][i] * x[k];
    x[i] = v / L[i][i];
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) ok = ok && isfinite(x[i]);
  ok = ok && lo <= x[0] && x[0] <= hi && sqrt((x[1] * x[1] + x[2] * x[2]) + x[3] * x[3]) <= x[0];
  bits = 0;
  if (!ok) {                                                                     // K37's closed form on the record's own sub-sums
    bits = TP_LIGHTING_FALLBACK;
    const double Sc = A[0][4], So = r[4], Scc = A[0][0], Sco = r[0];
    const double mc = Sc / n, mo = So / n;
    const double var = Scc / n - mc * mc, cov = Sco / n - mc * mo;
    double g = 1.0;
    if (var > min_var) {
      const double q = cov / var;
      g = fmin(fmax(q, lo), hi);
      if (g != q) bits |= TP_EXPOSURE_CLAMPED;
    } else {
      bits |= TP_EXPOSURE_FLAT;
    }
    x[0] = g; x[1] = 0.0; x[2] = 0.0; x[3] = 0.0; x[4] = mo - g * mc;
  }
  const double xr = (((x[0] * r[0] + x[1] * r[1]) + x[2] * r[2]) + x[3] * r[3]) + x[4] * r[4];
  double xAx = 0.0;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const double Ax = (((A[i][0] * x[0] + A[i][1] * x[1]) + A[i][2] * x[2]) + A[i][3] * x[3]) + A[i][4] * x[4];
    xAx = i == 0 ? x[0] * Ax : xAx + x[i] * Ax;
  }
  sse = (Soo - 2.0 * xr) + xAx;
}

// grid B, one wave: thread t gathers entry t of the image's G records, threads 0 .. 2 solve a channel each, thread 0 writes
__global__ __launch_bounds__(tp::kWave) void lighting_solve_kernel(tp_photo_lighting_args a, const double* part, int G) {
  __shared__ double sum[kLitRecord], sol[3][6];
  __shared__ int bits[3];
  const int b = blockIdx.x;
  {
    const double* rec = part + (int64_t)b * G * kLitRecord + threadIdx.x;       // (a record is one coalesced 512-byte row)
    double t = 0.0;
#pragma unroll 8
    for (int g = 0; g < G; ++g) t += rec[(int64_t)g * kLitRecord];               // ascending tile order
    sum[threadIdx.x] = t;
  }
  __syncthreads();
  const double n = sum[0];
  if (threadIdx.x < 3) {
    double x[5], sse;
    int flag;
    solve_channel(sum + 1 + kLitChannel * (int)threadIdx.x, n, (double)a.gain_min, (double)a.gain_max, (double)a.min_var, x, sse, flag);
#pragma unroll
    for (int i = 0; i < 5; ++i) sol[threadIdx.x][i] = x[i];
    sol[threadIdx.x][5] = sse;
    bits[threadIdx.x] = flag << threadIdx.x;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float rms = (float)sqrt(fmax(0.0, (sol[0][5] + sol[1][5]) + sol[2][5]) / n);      // (0 / 0 at n = 0: NaN)
  bool finite = isfinite(rms);
  for (int e = 0; e < 15; ++e) finite = finite && isfinite((float)sol[e / 5][e % 5]);
  const int status = n < (double)kLitMinCount ? 1 : (finite ? 0 : 3);
  for (int e = 0; e < 15; ++e)
    a.light[b * 15 + e] = status == 0 ? (float)sol[e / 5][e % 5] : (a.light_in ? a.light_in[b * 15 + e] : (e % 5 == 0 ? 1.f : 0.f));
  a.count[b] = (int)n;
  a.rms[b] = rms;
  a.status[b] = status;
  a.flags[b] = bits[0] | bits[1] | bits[2];
}

// INPLACE: rgb_out is rgb; a pixel without a surface is then not written
template <bool VEC, bool INPLACE>
__global__ __launch_bounds__(kGnBlock) void lighting_apply_kernel(tp_photo_lighting_args a) {
  const int b = blockIdx.y;
  const int64_t plane = (int64_t)a.H * a.W;
  const float* pz = a.zbuf + (int64_t)b * plane;
  const float* pc = a.rgb + (int64_t)b * plane * 3;
  const int32_t* pf = a.face + (int64_t)b * plane;
  float* pd = a.rgb_out + (int64_t)b * plane * 3;
  const float* T = a.pose + (int64_t)b * 12;
  float l[15];
#pragma unroll
  for (int e = 0; e < 15; ++e) l[e] = a.light[b * 15 + e];
  const int64_t p0 = (int64_t)blockIdx.x * kGnTile + (int)threadIdx.x * kGnPix;
  if (p0 >= plane) return;
  float zs[kGnPix];
  load_four<VEC, float, float4>(pz, p0, plane, -1.f, zs);
  unsigned cov = 0u;
#pragma unroll
  for (int k = 0; k < kGnPix; ++k)
    if (covered(zs[k])) cov |= 1u << k;                                          // (a pixel past the plane holds -1)
  if (INPLACE && cov == 0u) return;
  if constexpr (VEC) {
    float v[kGnPix * 3];
    int fs[kGnPix];
    const float4* c4 = reinterpret_cast<const float4*>(pc + p0 * 3);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float4 c = c4[q];
      v[4 * q] = c.x; v[4 * q + 1] = c.y; v[4 * q + 2] = c.z; v[4 * q + 3] = c.w;
    }
    load_four<true, int, int4>(pf, p0, plane, -1, fs);
#pragma unroll
    for (int k = 0; k < kGnPix; ++k) {
      if (!(cov >> k & 1u)) continue;
      float s[3];
      shade_of(a.verts, a.faces, a.V, a.F, l, fs[k], T, s);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) v[3 * k + ch] = tp::add_rn(tp::mul_rn(s[ch], v[3 * k + ch]), l[5 * ch + 4]);
    }
    if (!INPLACE || cov == 0xFu) {
      float4* d4 = reinterpret_cast<float4*>(pd + p0 * 3);
#pragma unroll
      for (int q = 0; q < 3; ++q) d4[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    } else {
#pragma unroll
      for (int k = 0; k < kGnPix; ++k)
        if (cov >> k & 1u) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) pd[(p0 + k) * 3 + ch] = v[3 * k + ch];
        }
    }
  } else {
#pragma unroll
    for (int k = 0; k < kGnPix; ++k) {
      if (p0 + k >= plane) break;
      const bool on = cov >> k & 1u;
      if (INPLACE && !on) continue;
      float s[3] = {0.f, 0.f, 0.f};
      if (on) shade_of(a.verts, a.faces, a.V, a.F, l, pf[p0 + k], T, s);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float c = pc[(p0 + k) * 3 + ch];
        pd[(p0 + k) * 3 + ch] = on ? tp::add_rn(tp::mul_rn(s[ch], c), l[5 * ch + 4]) : c;
      }
    }
  }
}

bool overlap(const void* x, size_t nx, const void* y, size_t ny) {
  const uintptr_t p = (uintptr_t)x, q = (uintptr_t)y;
  return x && y && p < q + ny && q < p + nx;
}

bool lighting_args_ok(const tp_photo_lighting_args& a) {
  const char* who = "tp_photo_lighting";
  if (a.B <= 0 || a.B > 65535 || a.H <= 0 || a.W <= 0 || a.Ft <= 0 || (int64_t)a.H * a.W > 0x7FFFFFFFll || a.V <= 0 || a.F <= 0) {
    tp::set_error("%s: bad sizes (B 1..65535, Ft > 0, H > 0, W > 0, H * W < 2^31, V > 0, F > 0)", who);
    return false;
  }
  if (!a.frame && a.Ft != 1 && a.Ft != a.B) {
    tp::set_error("%s: Ft = %d is neither 1 nor B = %d and there is no frame map", who, a.Ft, a.B);
    return false;
  }
  if (!(a.tau > 0.f) || !isfinite(a.tau)) { tp::set_error("%s: tau must be finite and positive", who); return false; }
  if (!(a.gain_min > 0.f) || !(a.gain_min <= 1.f) || !(a.gain_max >= 1.f) || !isfinite(a.gain_max)) {
    tp::set_error("%s: gain_min and gain_max must hold 0 < gain_min <= 1 <= gain_max < inf", who);
    return false;
  }
  if (!(a.min_var >= 0.f) || !isfinite(a.min_var)) { tp::set_error("%s: min_var must be finite and not negative", who); return false; }
  if (!a.verts || !a.faces || !a.face || !a.zbuf || !a.rgb || !a.pose || !a.image || !a.light || !a.count || !a.rms || !a.status || !a.flags ||
      !a.workspace) {
    tp::set_error("%s: null pointer", who);
    return false;
  }
  if ((uintptr_t)a.workspace & 15u) { tp::set_error("%s: workspace must be 16-byte aligned", who); return false; }
  const size_t planes = (size_t)a.B * (size_t)a.H * (size_t)a.W * 3 * sizeof(float), fit = (size_t)a.B * 15 * sizeof(float);
  if (a.rgb_out && a.rgb_out != a.rgb && overlap(a.rgb_out, planes, a.rgb, planes)) {
    tp::set_error("%s: rgb_out must be rgb itself or must not overlap it", who);
    return false;
  }
  if (overlap(a.light, fit, a.light_in, fit)) { tp::set_error("%s: light must not overlap light_in", who); return false; }
  return true;
}

size_t lighting_workspace_bytes(int B, int H, int W) {                           // one 64-double record per (image, tile)
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const size_t bytes = (size_t)B * (size_t)gn_tiles((int64_t)H * W) * kLitRecord * sizeof(double);
  return (bytes + 15) & ~(size_t)15;
}

void lighting_launch(const tp_photo_lighting_args& a, hipStream_t st) {
  const int64_t plane = (int64_t)a.H * a.W;
  const int G = (int)gn_tiles(plane);
  double* part = static_cast<double*>(a.workspace);
  const bool quads = plane % kGnPix == 0 && (((uintptr_t)a.zbuf | (uintptr_t)a.rgb | (uintptr_t)a.face) & 15u) == 0;
  if (quads && ((uintptr_t)a.image & 15u) == 0) hipLaunchKernelGGL(lighting_reduce_kernel<true>, dim3(G, a.B), dim3(kGnBlock), 0, st, a, part);
  else hipLaunchKernelGGL(lighting_reduce_kernel<false>, dim3(G, a.B), dim3(kGnBlock), 0, st, a, part);
  hipLaunchKernelGGL(lighting_solve_kernel, dim3(a.B), dim3(tp::kWave), 0, st, a, (const double*)part, G);
  if (!a.rgb_out) return;
  const bool inplace = a.rgb_out == a.rgb;
  if (quads && ((uintptr_t)a.rgb_out & 15u) == 0) {
    if (inplace) hipLaunchKernelGGL((lighting_apply_kernel<true, true>), dim3(G, a.B), dim3(kGnBlock), 0, st, a);
    else hipLaunchKernelGGL((lighting_apply_kernel<true, false>), dim3(G, a.B), dim3(kGnBlock), 0, st, a);
  } else {
    if (inplace) hipLaunchKernelGGL((lighting_apply_kernel<false, true>), dim3(G, a.B), dim3(kGnBlock), 0, st, a);
    else hipLaunchKernelGGL((lighting_apply_kernel<false, false>), dim3(G, a.B), dim3(kGnBlock), 0, st, a);
  }
}
}  // namespace

extern "C" size_t tp_photo_lighting_workspace_bytes(int B, int H, int W) { return lighting_workspace_bytes(B, H, W); }

extern "C" int tp_photo_lighting(const tp_photo_lighting_args* a, tp_stream_t stream) {
  return tp::term_step("tp_photo_lighting", a, lighting_args_ok, lighting_launch, stream);
}
