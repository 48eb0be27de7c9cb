// K37 tp_photo_exposure: per-image, per-channel gain and bias between B renderings and their photographs, and the renderings under
// that fit (the public function is ops.photo_exposure in texpose_amd/ops/refine.py, the rules in
// include/texpose_amd.h).
//
//   exposure_reduce grid (ceil(H * W / 1024), B) x 256: K30's reduce without the Jacobians.  A thread owns four consecutive flat
//                   pixels: one 16-byte load of the rendered depth where the plane allows it, else guarded 4-byte loads; a thread
//                   without an interior covered pixel leaves after those 4 bytes per pixel.  The others read the 12 rendered and the
//                   12 photographed colour values as three 16-byte loads each (guarded 4-byte loads of the pixels left on the other
//                   path) and per pixel the mask byte.  The fit that came in and the frame index are wave-uniform and are read
//                   before the kernel's only global store, so they come through scalar loads.  Each kept pixel adds to 16 fp64 sums.
//   exposure_solve  grid B x 64: gathers an image's records in ascending tile order (gn_gather), thread 0 solves the three 2 x 2
//                   systems in closed form and writes the outputs.
//   exposure_apply  grid (ceil(H * W / 1024), B) x 256, four pixels per thread as above; gain[b] and bias[b] are wave-uniform.
// No atomics; every fp64 sum has one fixed order (K30's), so all outputs are a function of the inputs alone.
#include "tp_common.h"
#include "pose_gn.h"
#include "pose_terms.h"

namespace {
constexpr int kExpSums = 16;                           // n, then per channel: c, o, c c, c o, o o
constexpr int kExpMinCount = 6;

__device__ __forceinline__ bool finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }
__device__ __forceinline__ bool covered(float z) { return z > 0.f && isfinite(z); }

// the four depths of a thread's pixels from p0 on, -1 past the plane
template <bool VEC>
__device__ __forceinline__ void load_depths(const float* pz, int64_t p0, int64_t plane, float (&zs)[kGnPix]) {
#pragma unroll
  for (int k = 0; k < kGnPix; ++k) zs[k] = -1.f;
  if constexpr (VEC) {
    if (p0 < plane) {                                                            // (plane % 4 == 0: the four are inside together)
      const float4 z4 = *reinterpret_cast<const float4*>(pz + p0);
      zs[0] = z4.x; zs[1] = z4.y; zs[2] = z4.z; zs[3] = z4.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kGnPix; ++k)
      if (p0 + k < plane) zs[k] = pz[p0 + k];
  }
}

// VEC: H * W is a multiple of four and zbuf / rgb / image are 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kGnBlock) void exposure_reduce_kernel(tp_photo_exposure_args a, double* part) {
  __shared__ double wave_part[kGnWaves][kExpSums];
  const int b = blockIdx.y;
  const int fr = gn_frame_of(a, b);
  const int64_t plane = (int64_t)a.H * a.W;
  const float* pz = a.zbuf + (int64_t)b * plane;
  const float* pc = a.rgb + (int64_t)b * plane * 3;
  const float* po = a.image + (int64_t)fr * plane * 3;
  const uint8_t* pm = a.mask ? a.mask + (int64_t)fr * plane : nullptr;
  double gin[3], bin[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    gin[ch] = a.gain_in ? (double)a.gain_in[b * 3 + ch] : 1.0;
    bin[ch] = a.bias_in ? (double)a.bias_in[b * 3 + ch] : 0.0;
  }
  const double tau2 = (double)a.tau * (double)a.tau;

  const int64_t p0 = (int64_t)blockIdx.x * kGnTile + (int)threadIdx.x * kGnPix;            // (< H * W + 1024 < 2^31 + 1024)
  float zs[kGnPix];
  load_depths<VEC>(pz, p0, plane, zs);

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
#pragma unroll
  for (int k = 0; k < kGnPix * 3; ++k) { cs[k] = 0.f; os[k] = 0.f; }
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
    } else {
#pragma unroll
      for (int k = 0; k < kGnPix; ++k)
        if (cand >> k & 1u) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) { cs[3 * k + ch] = pc[(p0 + k) * 3 + ch]; os[3 * k + ch] = po[(p0 + k) * 3 + ch]; }
        }
    }
  }

  double s[kExpSums];
#pragma unroll
  for (int k = 0; k < kExpSums; ++k) s[k] = 0.0;
  bool any = false;
#pragma unroll
  for (int k = 0; k < kGnPix; ++k) {
    if (!(cand >> k & 1u)) continue;
    if (pm && pm[p0 + k] == 0) continue;
    if (!(finite3(cs + 3 * k) && finite3(os + 3 * k))) continue;
    double c[3], o[3], res[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      c[ch] = (double)cs[3 * k + ch];
      o[ch] = (double)os[3 * k + ch];
      res[ch] = o[ch] - (gin[ch] * c[ch] + bin[ch]);
    }
    if (!((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2] <= tau2)) continue;
    s[0] += 1.0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      s[1 + 5 * ch] += c[ch];
      s[2 + 5 * ch] += o[ch];
      s[3 + 5 * ch] += c[ch] * c[ch];
      s[4 + 5 * ch] += c[ch] * o[ch];
      s[5 + 5 * ch] += o[ch] * o[ch];
    }
    any = true;
  }

  // the workgroup's sums -> one record: butterfly inside the wave, lane 0 to LDS, the waves in ascending order; a wave that added
  // nothing stores the zeros its butterflies would have given.  Entries 16 .. 31 of the record are zero.
  const int lane = threadIdx.x & (tp::kWave - 1), wave = threadIdx.x / tp::kWave;
  if (__ballot(any) != 0ull) {                                                   // (uniform per wave)
    wave_sum_all(s);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < kExpSums; ++k) wave_part[wave][k] = s[k];
    }
  } else if (lane < kExpSums) {
    wave_part[wave][lane] = 0.0;
  }
  __syncthreads();
  if (threadIdx.x < kGnPart) {
    double t = 0.0;
    if (threadIdx.x < kExpSums) {
      t = wave_part[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < kGnWaves; ++w) t += wave_part[w][threadIdx.x];
    }
    part[((int64_t)b * gridDim.x + blockIdx.x) * kGnPart + threadIdx.x] = t;
  }
}

// grid B, one wave: gathers the image's G records, then thread 0 solves per channel and writes the image's outputs
__global__ __launch_bounds__(tp::kWave) void exposure_solve_kernel(tp_photo_exposure_args a, const double* part, int G) {
  __shared__ double sum[kGnPart], stage[kGnStage][kGnPart];
  const int b = blockIdx.x;
  gn_gather(part + (int64_t)b * G * kGnPart, G, stage, sum);
  if (threadIdx.x != 0) return;
  const double n = sum[0];
  const double lo = (double)a.gain_min, hi = (double)a.gain_max, min_var = (double)a.min_var;
  float g32[3], b32[3];
  double sse[3];
  int flags = 0;
  bool finite = true;
  for (int ch = 0; ch < 3; ++ch) {
    const double Sc = sum[1 + 5 * ch], So = sum[2 + 5 * ch], Scc = sum[3 + 5 * ch], Sco = sum[4 + 5 * ch], Soo = sum[5 + 5 * ch];
    const double mc = Sc / n, mo = So / n;
    const double var = Scc / n - mc * mc, cov = Sco / n - mc * mo, voo = Soo / n - mo * mo;
    double g = 1.0;
    if (var > min_var) {
      const double q = cov / var;
      g = fmin(fmax(q, lo), hi);
      if (g != q) flags |= TP_EXPOSURE_CLAMPED << ch;
    } else {
      flags |= TP_EXPOSURE_FLAT << ch;
    }
    const double bias = mo - g * mc;
    sse[ch] = n * ((voo - 2.0 * (g * cov)) + (g * g) * var);
    g32[ch] = (float)g;
    b32[ch] = (float)bias;
    finite = finite && isfinite(g32[ch]) && isfinite(b32[ch]);
  }
  const float rms = (float)sqrt(fmax(0.0, (sse[0] + sse[1]) + sse[2]) / n);      // (0 / 0 at n = 0: NaN)
  const int status = n < (double)kExpMinCount ? 1 : (finite && isfinite(rms) ? 0 : 3);
  for (int ch = 0; ch < 3; ++ch) {
    a.gain[b * 3 + ch] = status == 0 ? g32[ch] : (a.gain_in ? a.gain_in[b * 3 + ch] : 1.f);
    a.bias[b * 3 + ch] = status == 0 ? b32[ch] : (a.bias_in ? a.bias_in[b * 3 + ch] : 0.f);
  }
  a.count[b] = (int)n;
  a.rms[b] = rms;
  a.status[b] = status;
  a.flags[b] = flags;
}

// INPLACE: rgb_out is rgb; a pixel without a surface is then not written
template <bool VEC, bool INPLACE>
__global__ __launch_bounds__(kGnBlock) void exposure_apply_kernel(tp_photo_exposure_args a) {
  const int b = blockIdx.y;
  const int64_t plane = (int64_t)a.H * a.W;
  const float* pz = a.zbuf + (int64_t)b * plane;
  const float* pc = a.rgb + (int64_t)b * plane * 3;
  float* pd = a.rgb_out + (int64_t)b * plane * 3;
  float g[3], d[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) { g[ch] = a.gain[b * 3 + ch]; d[ch] = a.bias[b * 3 + ch]; }
  const int64_t p0 = (int64_t)blockIdx.x * kGnTile + (int)threadIdx.x * kGnPix;
  if (p0 >= plane) return;
  float zs[kGnPix];
  load_depths<VEC>(pz, p0, plane, zs);
  unsigned cov = 0u;
#pragma unroll
  for (int k = 0; k < kGnPix; ++k)
    if (covered(zs[k])) cov |= 1u << k;                                          // (a pixel past the plane holds -1)
  if (INPLACE && cov == 0u) return;
  if constexpr (VEC) {
    float v[kGnPix * 3];
    const float4* c4 = reinterpret_cast<const float4*>(pc + p0 * 3);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float4 c = c4[q];
      v[4 * q] = c.x; v[4 * q + 1] = c.y; v[4 * q + 2] = c.z; v[4 * q + 3] = c.w;
    }
#pragma unroll
    for (int k = 0; k < kGnPix; ++k)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float w = tp::add_rn(tp::mul_rn(g[ch], v[3 * k + ch]), d[ch]);
        v[3 * k + ch] = (cov >> k & 1u) ? w : v[3 * k + ch];
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
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float c = pc[(p0 + k) * 3 + ch];
        pd[(p0 + k) * 3 + ch] = on ? tp::add_rn(tp::mul_rn(g[ch], c), d[ch]) : c;
      }
    }
  }
}

bool overlap(const void* x, size_t nx, const void* y, size_t ny) {
  const uintptr_t p = (uintptr_t)x, q = (uintptr_t)y;
  return x && y && p < q + ny && q < p + nx;
}

bool exposure_args_ok(const tp_photo_exposure_args& a) {
  const char* who = "tp_photo_exposure";
  if (a.B <= 0 || a.B > 65535 || a.H <= 0 || a.W <= 0 || a.Ft <= 0 || (int64_t)a.H * a.W > 0x7FFFFFFFll) {
    tp::set_error("%s: bad sizes (B 1..65535, Ft > 0, H > 0, W > 0, H * W < 2^31)", who);
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
  if (!a.zbuf || !a.rgb || !a.image || !a.gain || !a.bias || !a.count || !a.rms || !a.status || !a.flags || !a.workspace) {
    tp::set_error("%s: null pointer", who);
    return false;
  }
  if ((uintptr_t)a.workspace & 15u) { tp::set_error("%s: workspace must be 16-byte aligned", who); return false; }
  const size_t planes = (size_t)a.B * (size_t)a.H * (size_t)a.W * 3 * sizeof(float), fit = (size_t)a.B * 3 * sizeof(float);
  if (a.rgb_out && a.rgb_out != a.rgb && overlap(a.rgb_out, planes, a.rgb, planes)) {
    tp::set_error("%s: rgb_out must be rgb itself or must not overlap it", who);
    return false;
  }
  if (overlap(a.gain, fit, a.gain_in, fit) || overlap(a.gain, fit, a.bias_in, fit) || overlap(a.bias, fit, a.gain_in, fit) ||
      overlap(a.bias, fit, a.bias_in, fit)) {
    tp::set_error("%s: gain and bias must not overlap gain_in or bias_in", who);
    return false;
  }
  return true;
}

void exposure_launch(const tp_photo_exposure_args& a, hipStream_t st) {
  const int64_t plane = (int64_t)a.H * a.W;
  const int G = (int)gn_tiles(plane);
  double* part = static_cast<double*>(a.workspace);
  const bool quads = plane % kGnPix == 0 && (((uintptr_t)a.zbuf | (uintptr_t)a.rgb) & 15u) == 0;
  if (quads && ((uintptr_t)a.image & 15u) == 0) hipLaunchKernelGGL(exposure_reduce_kernel<true>, dim3(G, a.B), dim3(kGnBlock), 0, st, a, part);
  else hipLaunchKernelGGL(exposure_reduce_kernel<false>, dim3(G, a.B), dim3(kGnBlock), 0, st, a, part);
  hipLaunchKernelGGL(exposure_solve_kernel, dim3(a.B), dim3(tp::kWave), 0, st, a, (const double*)part, G);
  if (!a.rgb_out) return;
  const bool inplace = a.rgb_out == a.rgb;
  if (quads && ((uintptr_t)a.rgb_out & 15u) == 0) {
    if (inplace) hipLaunchKernelGGL((exposure_apply_kernel<true, true>), dim3(G, a.B), dim3(kGnBlock), 0, st, a);
    else hipLaunchKernelGGL((exposure_apply_kernel<true, false>), dim3(G, a.B), dim3(kGnBlock), 0, st, a);
  } else {
    if (inplace) hipLaunchKernelGGL((exposure_apply_kernel<false, true>), dim3(G, a.B), dim3(kGnBlock), 0, st, a);
    else hipLaunchKernelGGL((exposure_apply_kernel<false, false>), dim3(G, a.B), dim3(kGnBlock), 0, st, a);
  }
}
}  // namespace

extern "C" size_t tp_photo_exposure_workspace_bytes(int B, int H, int W) { return tp::term_workspace_bytes(B, H, W); }

extern "C" int tp_photo_exposure(const tp_photo_exposure_args* a, tp_stream_t stream) {
  return tp::term_step("tp_photo_exposure", a, exposure_args_ok, exposure_launch, stream);
}
