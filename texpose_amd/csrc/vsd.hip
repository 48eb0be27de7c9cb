// K26 tp_vsd: the per-pixel part of BOP's Visible Surface Discrepancy (the public functions are in
// texpose_amd/pose_error.py, the rules in include/texpose_amd.h).
//
// A streaming reduction: three depth planes in, 2 + T integers per pose pair out.  Grid (pixel tiles, B); a workgroup of 256 threads
// owns 1,024 pixels, a thread four consecutive pixels of one row -- one 16-byte load per plane where W is a multiple of four and the
// planes are 16-byte aligned, else four guarded 4-byte loads -- so the row term of the distance factor is formed once per thread.
// Everything between the fp32 inputs and the predicates is fp64 in one fixed operation order (the library is built without
// contraction).  Each predicate of each of the four pixels becomes one wave ballot (on this target a vector compare already leaves
// its 64-bit lane mask in a scalar register pair) and a population count added to a wave-uniform counter; the T tolerances are
// wave-uniform too, so the T comparisons per pixel cost one compare, one mask AND and one count each.  The four wavefronts' counters
// meet in LDS and 2 + T threads add the workgroup's totals to counts[b] with integer atomics: sums of integers do not depend on the
// order of arrival, so the result is a function of the inputs alone.  The call clears counts itself (first launch) and a last tiny
// launch forms err; three launches, no allocation, no host synchronisation.
#include "tp_common.h"

namespace {
constexpr int kVsdBlock = 256, kVsdPix = 4, kVsdWaves = kVsdBlock / tp::kWave, kVsdMaxT = TP_VSD_MAX_TAUS, kVsdOut = 2 + kVsdMaxT;

__global__ __launch_bounds__(kVsdBlock) void vsd_init_kernel(int32_t* counts, int n) {
  const int i = blockIdx.x * kVsdBlock + threadIdx.x;
  if (i < n) counts[i] = 0;
}

__device__ __forceinline__ int ballot_count(bool p) { return __popcll(__ballot(p)); }

// grid (ceil(H * quads_per_row / 256), B); VEC: rows are whole quads and the planes 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kVsdBlock) void vsd_kernel(tp_vsd_args a, int quads_per_row, int n_quads) {
  __shared__ int part[kVsdWaves][kVsdOut];
  const int b = blockIdx.y, T = a.T;
  int fr = a.Ft == 1 ? 0 : b;
  if (a.frame) {                                                     // out of range is the caller's error: clamped, never read past
    fr = a.frame[b];
    fr = fr < 0 ? 0 : (fr >= a.Ft ? a.Ft - 1 : fr);
  }
  const int64_t plane = (int64_t)a.H * a.W;
  const float* pe = a.z_est + (int64_t)b * plane;
  const float* pg = a.z_gt + (int64_t)b * plane;
  const float* pt = a.depth_test + (int64_t)fr * plane;

  // (no thread leaves before the ballots: one without pixels carries background, which is in no set)
  float ze[kVsdPix], zg[kVsdPix], dt[kVsdPix];
#pragma unroll
  for (int k = 0; k < kVsdPix; ++k) { ze[k] = -1.f; zg[k] = -1.f; dt[k] = 0.f; }
  const int q = blockIdx.x * kVsdBlock + threadIdx.x;
  int i = 0, j0 = 0;
  if (q < n_quads) {
    i = q / quads_per_row;
    j0 = (q - i * quads_per_row) * kVsdPix;
    const int64_t o = (int64_t)i * a.W + j0;
    if constexpr (VEC) {
      const float4 e = *reinterpret_cast<const float4*>(pe + o), g = *reinterpret_cast<const float4*>(pg + o),
                   d = *reinterpret_cast<const float4*>(pt + o);
      ze[0] = e.x; ze[1] = e.y; ze[2] = e.z; ze[3] = e.w;
      zg[0] = g.x; zg[1] = g.y; zg[2] = g.z; zg[3] = g.w;
      dt[0] = d.x; dt[1] = d.y; dt[2] = d.z; dt[3] = d.w;
    } else {
#pragma unroll
      for (int k = 0; k < kVsdPix; ++k)
        if (j0 + k < a.W) { ze[k] = pe[o + k]; zg[k] = pg[o + k]; dt[k] = pt[o + k]; }
    }
  }

  const float* K = a.intr + (int64_t)b * 9;
  const double fx = (double)K[0], cx = (double)K[2], fy = (double)K[4], cy = (double)K[5];
  const double delta = (double)a.delta_mm;
  const double v = (((double)i + 0.5) - cy) / fy;
  const double vv = v * v;                                           // f = sqrt((u * u + v * v) + 1)

  int cnt[kVsdOut];
#pragma unroll
  for (int k = 0; k < kVsdOut; ++k) cnt[k] = 0;
#pragma unroll
  for (int k = 0; k < kVsdPix; ++k) {
    const bool ok_e = ze[k] > 0.f, ok_g = zg[k] > 0.f;               // (a NaN is not ok)
    bool vis_g = false, vis_e = false;
    double diff = 0.0;
    if (ok_e || ok_g) {
      const double u = (((double)(j0 + k) + 0.5) - cx) / fx;
      const double f = sqrt((u * u + vv) + 1.0);
      const bool missing = !(dt[k] > 0.f);                           // 0, negative, NaN
      const double Dt = (double)dt[k] * f, De = (double)ze[k] * f, Dg = (double)zg[k] * f;
      vis_g = ok_g && (missing || Dg - Dt <= delta);
      vis_e = ok_e && (missing || De - Dt <= delta || vis_g);
      diff = fabs(Dg - De);
    }
    const bool in_i = vis_g && vis_e;
    cnt[0] += ballot_count(vis_g || vis_e);
    cnt[1] += ballot_count(in_i);
#pragma unroll
    for (int t = 0; t < kVsdMaxT; ++t)
      if (t < T) cnt[2 + t] += ballot_count(in_i && diff >= (double)a.tau_mm[(int64_t)b * T + t]);      // (uniform branch and load)
  }

  const int lane = threadIdx.x & (tp::kWave - 1), wave = threadIdx.x / tp::kWave;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kVsdOut; ++k) part[wave][k] = cnt[k];
  }
  __syncthreads();
  if (threadIdx.x < 2 + T) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < kVsdWaves; ++w) s += part[w][threadIdx.x];
    if (s) atomicAdd(a.counts + (int64_t)b * (2 + T) + threadIdx.x, s);
  }
}

// one thread per (b, t): e = (c_t + n_U - n_I) / n_U in fp64, rounded once; 1 where the union is empty
__global__ __launch_bounds__(kVsdBlock) void vsd_final_kernel(tp_vsd_args a) {
  const int o = blockIdx.x * kVsdBlock + threadIdx.x;
  if (o >= a.B * a.T) return;
  const int b = o / a.T, t = o - b * a.T;
  const int32_t* c = a.counts + (int64_t)b * (2 + a.T);
  const int n_u = c[0], n_i = c[1];
  a.err[o] = n_u == 0 ? 1.f : (float)((double)((int64_t)c[2 + t] + n_u - n_i) / (double)n_u);
}
}  // namespace

extern "C" int tp_vsd(const tp_vsd_args* a, tp_stream_t stream) {
  if (!a) { tp::set_error("tp_vsd: null args"); return -1; }
  if (a->T < 1 || a->T > TP_VSD_MAX_TAUS) { tp::set_error("tp_vsd: T = %d tolerances, 1 .. %d expected", a->T, TP_VSD_MAX_TAUS); return -1; }
  if (!a->z_est || !a->z_gt || !a->depth_test || !a->intr || !a->tau_mm || !a->counts || !a->err) {
    tp::set_error("tp_vsd: null pointer");
    return -1;
  }
  if (a->B <= 0 || a->B > 65535 || a->H <= 0 || a->W <= 0 || a->Ft <= 0 || (int64_t)a->H * a->W > 0x7FFFFFFFll - 4 * kVsdBlock) {
    tp::set_error("tp_vsd: bad sizes (B 1..65535, Ft > 0, H > 0, W > 0, H * W < 2^31)");
    return -1;
  }
  if (!a->frame && a->Ft != 1 && a->Ft != a->B) { tp::set_error("tp_vsd: Ft = %d is neither 1 nor B = %d and there is no frame map", a->Ft, a->B); return -1; }
  hipStream_t st = (hipStream_t)stream;
  const int n_out = a->B * (2 + a->T), n_err = a->B * a->T;
  const int qpr = (a->W + kVsdPix - 1) / kVsdPix;
  const int64_t n_quads = (int64_t)a->H * qpr;                       // (<= H * W: fits)
  const bool vec = a->W % kVsdPix == 0 && (((uintptr_t)a->z_est | (uintptr_t)a->z_gt | (uintptr_t)a->depth_test) & 15u) == 0;
  const dim3 grid((unsigned)((n_quads + kVsdBlock - 1) / kVsdBlock), a->B);
  hipLaunchKernelGGL(vsd_init_kernel, dim3((n_out + kVsdBlock - 1) / kVsdBlock), dim3(kVsdBlock), 0, st, a->counts, n_out);
  if (vec) hipLaunchKernelGGL(vsd_kernel<true>, grid, dim3(kVsdBlock), 0, st, *a, qpr, (int)n_quads);
  else hipLaunchKernelGGL(vsd_kernel<false>, grid, dim3(kVsdBlock), 0, st, *a, qpr, (int)n_quads);
  hipLaunchKernelGGL(vsd_final_kernel, dim3((n_err + kVsdBlock - 1) / kVsdBlock), dim3(kVsdBlock), 0, st, *a);
  return tp::check_launch("tp_vsd");
}
