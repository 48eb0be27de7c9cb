// K23: the Lab chroma term of the generator step (loss_weight.lab; reference model/nerf_adapt_st_gan.py:772-773, layers/lab_loss.py) in
// one launch each way.  As torch ops the term is ~40 element-wise / reduction launches forward and as many backward on the render's
// backward chain -- the pattern K8 (csrc/nerf_losses.hip) replaced for the photometric terms.
//   forward:  both normalised Lab triples per pixel in registers (csrc/lab_math.h), SmoothL1 of the two chroma channels, masked sum and
//             mask count reduced per wavefront, per block and -- by the block that arrives last -- over the blocks in ascending
//             order, all in double; optionally the two maps the reference returns for logging.
//   backward: g_rgb = g * d loss / d rgb from the inputs and sums[1] alone (no activation record); every element is written.
// A thread owns one pixel, or four consecutive ones (VEC4: 16-byte loads and stores) where P, the strides and the pointers allow.
// rgb is read where the composite left it ([B,P,3]); the real image and the mask are planes at caller-given strides: channels 3..5 and
// 13 of the patch gather's [B,14,P] in patch mode, dense tensors in full-image mode.
#include "tp_common.h"
#include "lab_math.h"

namespace {
constexpr int kBlock = 256, kWaves = kBlock / tp::kWave;

struct Pixel { float fake[3], real[3], mask; };

// the pixels q .. q + V - 1 of image b (V = 4: one aligned group inside the image, V = 1: any pixel)
template <int V>
__device__ __forceinline__ void load_pixels(const tp_lab_loss_args& a, int64_t b, int64_t p, Pixel (&px)[V]) {
  const float* rgb = a.rgb + (b * a.P + p) * 3;
  const float* real = a.real + b * a.real_batch_stride + p;
  if constexpr (V == 4) {
    float v[12];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 t = reinterpret_cast<const float4*>(rgb)[k];
      v[4 * k] = t.x; v[4 * k + 1] = t.y; v[4 * k + 2] = t.z; v[4 * k + 3] = t.w;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float4 t = *reinterpret_cast<const float4*>(real + c * a.real_channel_stride);
      px[0].real[c] = t.x; px[1].real[c] = t.y; px[2].real[c] = t.z; px[3].real[c] = t.w;
    }
    float4 m = make_float4(1.f, 1.f, 1.f, 1.f);
    if (a.mask) m = *reinterpret_cast<const float4*>(a.mask + b * a.mask_batch_stride + p);
    px[0].mask = m.x; px[1].mask = m.y; px[2].mask = m.z; px[3].mask = m.w;
#pragma unroll
    for (int i = 0; i < V; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) px[i].fake[c] = v[3 * i + c];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) { px[0].fake[c] = rgb[c]; px[0].real[c] = real[c * a.real_channel_stride]; }
    px[0].mask = a.mask ? a.mask[b * a.mask_batch_stride + p] : 1.f;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = tp::kWave >> 1; o > 0; o >>= 1) v += __shfl_down(v, o, tp::kWave);
  return v;                                   // (lane 0 holds the total)
}

// The last-block hand-over is K8's (csrc/nerf_losses.hip; the gfx950 agent-scope store / load contract of csrc/patch_conv.hip): the
// ticket lives in caller-owned memory, one word per stream, zero between launches.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "the last-block hand-over below relies on the gfx950 agent-scope store / load contract (csrc/patch_conv.hip)"
#endif
template <int V>
__global__ __launch_bounds__(kBlock) void lab_loss_fwd_kernel(tp_lab_loss_args a, unsigned long long* partial) {
  __shared__ double wave_part[2][kWaves];
  __shared__ double fin[2][kBlock];
  __shared__ bool last;
  const int64_t n_units = (int64_t)a.B * a.P / V;
  double s_l = 0.0, s_m = 0.0;
  for (int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * kBlock) {
    const int64_t q = u * V, b = q / a.P, p = q - b * a.P;
    Pixel px[V];
    load_pixels<V>(a, b, p, px);
    float fl[3][V], rl[3][V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      double lf[3], lr[3], unused3[3];
      tp_lab::rgb_to_lab_norm<false>(px[i].fake, lf, unused3, unused3);
      tp_lab::rgb_to_lab_norm<false>(px[i].real, lr, unused3, unused3);
      const double l = tp_lab::smooth_l1(lf[1] - lr[1]) + tp_lab::smooth_l1(lf[2] - lr[2]);
      s_l += l * (double)px[i].mask;
      s_m += (double)px[i].mask;
      fl[0][i] = (float)lr[0]; fl[1][i] = (float)lf[1]; fl[2][i] = (float)lf[2];       // (the L plane of the fake map is the real one's)
      rl[0][i] = (float)lr[0]; rl[1][i] = (float)lr[1]; rl[2][i] = (float)lr[2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int64_t o = (b * 3 + c) * a.P + p;
      if constexpr (V == 4) {
        if (a.fake_lab) *reinterpret_cast<float4*>(a.fake_lab + o) = make_float4(fl[c][0], fl[c][1], fl[c][2], fl[c][3]);
        if (a.real_lab) *reinterpret_cast<float4*>(a.real_lab + o) = make_float4(rl[c][0], rl[c][1], rl[c][2], rl[c][3]);
      } else {
        if (a.fake_lab) a.fake_lab[o] = fl[c][0];
        if (a.real_lab) a.real_lab[o] = rl[c][0];
      }
    }
  }
  s_l = wave_sum(s_l);
  s_m = wave_sum(s_m);
  const int lane = threadIdx.x & (tp::kWave - 1), wave = threadIdx.x / tp::kWave;
  if (lane == 0) { wave_part[0][wave] = s_l; wave_part[1][wave] = s_m; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t_l = wave_part[0][0], t_m = wave_part[1][0];
    for (int w = 1; w < kWaves; ++w) { t_l += wave_part[0][w]; t_m += wave_part[1][w]; }
    __hip_atomic_store(partial + blockIdx.x * 2, (unsigned long long)__double_as_longlong(t_l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(partial + blockIdx.x * 2 + 1, (unsigned long long)__double_as_longlong(t_m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  if (threadIdx.x == 0) __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // the partials of all blocks, added in ascending block order (gridDim.x <= TP_LAB_LOSS_MAX_BLOCKS = kBlock: one per thread)
  if (threadIdx.x < gridDim.x) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
      fin[k][threadIdx.x] = __longlong_as_double((long long)__hip_atomic_load(partial + threadIdx.x * 2 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t_l = 0.0, t_m = 0.0;
    for (unsigned i = 0; i < gridDim.x; ++i) { t_l += fin[0][i]; t_m += fin[1][i]; }
    if (!a.mask) t_m = 2.0 * (double)a.B * (double)a.P;          // (the mean over both chroma channels)
    a.sums[0] = t_l; a.sums[1] = t_m;
    a.loss[0] = (float)(t_l / t_m);
  }
}

template <int V>
__global__ __launch_bounds__(kBlock) void lab_loss_bwd_kernel(tp_lab_loss_args a, const float* g, float* g_rgb) {
  const int64_t n_units = (int64_t)a.B * a.P / V;
  const double scale = (double)g[0] / a.sums[1];             // (an empty mask: g / 0, and 0 * inf = NaN below, as the rule has it)
  for (int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x; u < n_units; u += (int64_t)gridDim.x * kBlock) {
    const int64_t q = u * V, b = q / a.P, p = q - b * a.P;
    Pixel px[V];
    load_pixels<V>(a, b, p, px);
    float out[3 * V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
      double lf[3], lr[3], dlin[3], df[3], unused3[3], gc[3];
      tp_lab::rgb_to_lab_norm<true>(px[i].fake, lf, dlin, df);
      tp_lab::rgb_to_lab_norm<false>(px[i].real, lr, unused3, unused3);
      const double k = scale * (double)px[i].mask;
      tp_lab::chroma_grad(k * tp_lab::smooth_l1_grad(lf[1] - lr[1]), k * tp_lab::smooth_l1_grad(lf[2] - lr[2]), dlin, df, gc);
#pragma unroll
      for (int c = 0; c < 3; ++c) out[3 * i + c] = (float)gc[c];
    }
    float* o = g_rgb + (b * a.P + p) * 3;
    if constexpr (V == 4) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        reinterpret_cast<float4*>(o)[k] = make_float4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = out[c];
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// four pixels per thread: groups of four must not straddle images and every 16-byte access must be aligned
bool vec4_ok(const tp_lab_loss_args* a, const float* g_rgb) {
  return a->P % 4 == 0 && aligned16(a->rgb) && aligned16(a->real) && a->real_batch_stride % 4 == 0 && a->real_channel_stride % 4 == 0
         && (!a->mask || (aligned16(a->mask) && a->mask_batch_stride % 4 == 0)) && aligned16(a->fake_lab) && aligned16(a->real_lab)
         && aligned16(g_rgb);
}
int grid_for(const tp_lab_loss_args* a, int v) {
  const int64_t units = (int64_t)a->B * a->P / v, g = (units + kBlock - 1) / kBlock;
  return (int)(g < 1 ? 1 : (g > TP_LAB_LOSS_MAX_BLOCKS ? TP_LAB_LOSS_MAX_BLOCKS : g));
}
int check(const tp_lab_loss_args* a, const char* what) {
  if (!a || !a->rgb || !a->real || !a->sums) { tp::set_error("%s: null pointer", what); return -1; }
  if (a->B <= 0 || a->P <= 0) { tp::set_error("%s: bad sizes", what); return -1; }
  if (a->real_channel_stride < a->P || a->real_batch_stride < a->P || (a->mask && a->mask_batch_stride < a->P)) {
    tp::set_error("%s: a plane stride below P", what);
    return -1;
  }
  return 0;
}
}  // namespace

static_assert(TP_LAB_LOSS_MAX_BLOCKS <= kBlock, "the last block loads one partial per thread");

extern "C" int tp_lab_loss_fwd(const tp_lab_loss_args* a, tp_stream_t stream) {
  if (int rc = check(a, "tp_lab_loss_fwd")) return rc;
  if (!a->workspace || !a->loss) { tp::set_error("tp_lab_loss_fwd: null pointer"); return -1; }
  if (!a->ticket) { tp::set_error("tp_lab_loss_fwd: args.ticket (a zero-filled device word owned by the calling stream) is required"); return -1; }
  if (vec4_ok(a, nullptr))
    hipLaunchKernelGGL(lab_loss_fwd_kernel<4>, dim3(grid_for(a, 4)), dim3(kBlock), 0, (hipStream_t)stream, *a, (unsigned long long*)a->workspace);
  else
    hipLaunchKernelGGL(lab_loss_fwd_kernel<1>, dim3(grid_for(a, 1)), dim3(kBlock), 0, (hipStream_t)stream, *a, (unsigned long long*)a->workspace);
  return tp::check_launch("tp_lab_loss_fwd");
}

extern "C" int tp_lab_loss_bwd(const tp_lab_loss_args* a, const float* g, float* g_rgb, tp_stream_t stream) {
  if (int rc = check(a, "tp_lab_loss_bwd")) return rc;
  if (!g || !g_rgb) { tp::set_error("tp_lab_loss_bwd: null gradient pointer"); return -1; }
  tp_lab_loss_args b = *a;
  b.fake_lab = b.real_lab = nullptr;                      // (forward outputs: no part of the backward's alignment)
  if (vec4_ok(&b, g_rgb))
    hipLaunchKernelGGL(lab_loss_bwd_kernel<4>, dim3(grid_for(a, 4)), dim3(kBlock), 0, (hipStream_t)stream, b, g, g_rgb);
  else
    hipLaunchKernelGGL(lab_loss_bwd_kernel<1>, dim3(grid_for(a, 1)), dim3(kBlock), 0, (hipStream_t)stream, b, g, g_rgb);
  return tp::check_launch("tp_lab_loss_bwd");
}
