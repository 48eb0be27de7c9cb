// K35 tp_face_texel_shade: colour the pixels of a rasterised mesh from a per-face texel texture ("mesh colours"; the
// public functions are in texpose_amd/face_texels.py, the rule in include/texpose_amd.h, restated in tests/face_texels_ref.py).
//
// The texture: resolution R (1 .. 64); face f with vertices (v0, v1, v2) in its own order carries the nodes (i, j), i, j >= 0,
// i + j <= R, node (i, j) at the barycentric weights ((R - i - j) / R, i / R, j / R), stored at n(i, j) = j (R + 1) - j (j - 1) / 2 + i
// of the face's T(R) = (R + 1)(R + 2) / 2 texels.  The nodes of all faces are the vertices of the mesh subdivided R times.
//
// A pixel whose winning face (K19's face plane) is f:
//   1. u_k, v_k, 1 / z_k of the three vertices in fp64 exactly as face_setup_kernel of mesh_raster.hip forms them; twice the area;
//      the edge functions b_k at the pixel centre (j + 0.5, i + 0.5) over twice the area; t_k = b_k / z_k; w_k = t_k / ((t_0 + t_1) + t_2);
//      negative w_k become 0 and the three are divided by their sum ((w_0 + w_1) + w_2).
//   2. a = R w_1, b = R w_2, i = min(floor(a), R - 1), j = min(floor(b), R - 1 - i), fa = a - i, fb = b - j.  Where fa + fb > 1 and the
//      cell (i, j) has an upper triangle (i + j <= R - 2):  c = (fa + fb - 1) N(i+1, j+1) + (1 - fb) N(i+1, j) + (1 - fa) N(i, j+1);
//      otherwise  c = (1 - fa - fb) N(i, j) + fa N(i+1, j) + fb N(i, j+1).  (On the last diagonal fa + fb exceeds 1 by rounding alone.)
//   3. every step fp64 as written (the library is built without contraction), rounded to fp32 once.
// Zeros are written, and nothing else is read, for face < 0 or >= F, a vertex index outside 0 .. V-1, a vertex at z <= 0, |twice the
// area| <= 1e-10 or any non-finite intermediate (a non-finite colour included).
//
// A gather: 4 B read and 12 B written per pixel; a covered pixel gathers 3 indices, 9 vertex floats and 9 texel floats, which
// neighbouring pixels of a face share.  One thread per pixel, the image index uniform over the workgroup (pose[b] and intr[b] are scalar
// loads).  One launch; no LDS, no atomics, no workspace: the output is a function of the inputs alone.
//
// K36 tp_face_texel_shade_bwd: the adjoint of K35 with respect to the texels (restated in tests/face_texel_fit_ref.py).
// K35 is linear in the texels: a pixel that it shades by rule reads three slots n_a, n_b, n_c of its face f with the weights w_a, w_b,
// w_c of step 2 (face_texel_cell of face_texel_cell.h, the ONE source of steps 1 and 2 for K35, K36 and K43b).  The adjoint adds w_k g_p (3
// channels) to the
// destination d(f, n_k): the slot f T + n_k itself, or node_index[f T + n_k] where a node index is given (entries outside 0 .. U-1 are
// skipped); `weight` is the same sum with g = 1 (the coverage: the lumped diagonal of S^T S).  A pixel contributes nothing where K35
// writes zeros by its geometric rules, and nothing where a component of its grad_rgb is not finite.  K35's "non-finite colour -> zero"
// rule depends on the texel VALUES; the adjoint reads no texels and ignores it.
//
// Deterministic without float atomics: 64-bit fixed point.  Integer addition is associative, so the arrival order of the atomics, and
// a graph replay, cannot change a bit.  Launches, all on the caller's stream, no host synchronisation, no allocation:
//   1. one asynchronous memset clears the workspace: acc int64 [N,3], wacc int64 [N] (where weight is wanted), the word gmax;
//   2. gmax = max over the contributing pixels of max_c |g_c|, as the float's bit pattern under an unsigned atomic max (non-negative
//      floats order like their bits), one atomic per wavefront;
//   3. e = max(floor(log2 gmax), -126) (the float's exponent field; -126 for a subnormal or zero gmax).  Every contribution is
//      q = llrint((w_k (double)g_c) 2^(36 - e)): an fp64 product, rounded to nearest even, |q| <= 2^37 (1 + 2^-50); it is added to
//      acc[3 d + c] by a 64-bit integer atomic.  Weights use e = 0: llrint(w_k 2^36).  A zero q is not sent;
//   4. grad[3 d + c] = (float)((double)acc 2^(e - 36)), rounded once; weight[d] likewise.
// Overflow: the three weights of a pixel are >= -2^-50 and add up to 1 within 2^-50, so whatever node_index maps them to, one pixel adds
// at most 2^37 (1 + 2^-49) in magnitude to one destination, and B H W <= 2^25 pixels at most 2^62 (1 + 2^-49) < 2^63: larger B H W is
// refused.  Error: each q is within 1/2 of its exact value, so acc 2^(e-36) is within n_d 2^(e-37) <= n_d gmax 2^-37 of the exact sum
// over the n_d contributions to d (weights: n_d 2^-37), plus the one fp32 rounding of the result.
// One thread per pixel, 256 per workgroup, the image index uniform over the workgroup, no LDS.  A background pixel returns after one
// 4-byte load; a pixel whose gradient is all zeros (a masked one) after 16 bytes unless the coverage is wanted.
#include "tp_common.h"
#include "face_texel_cell.h"

namespace {
constexpr int kShadeBlock = 256;

__global__ __launch_bounds__(kShadeBlock) void face_texel_shade_kernel(tp_face_texel_shade_args a, int blocks_per_image, int T) {
  const int b = (int)(blockIdx.x / (unsigned)blocks_per_image);                  // workgroup-uniform
  const int64_t hw = (int64_t)a.H * a.W;
  const int64_t rem = (int64_t)(blockIdx.x - (unsigned)b * (unsigned)blocks_per_image) * kShadeBlock + threadIdx.x;
  if (rem >= hw) return;
  const int64_t pix = (int64_t)b * hw + rem;
  float* out = a.rgb + 3 * pix;
  double col[3] = {0.0, 0.0, 0.0};
  const int f = a.face[pix];
  if (f >= 0 && f < a.F) {
    const int i = (int)(rem / a.W), j = (int)(rem - (int64_t)i * a.W);
    TexelCell cell;
    if (face_texel_cell(a.verts, a.faces, a.pose + 12 * (int64_t)b, a.intr + 9 * (int64_t)b, a.V, a.R, f, i, j, cell)) {
      face_texel_colour(a.texels + 3 * ((int64_t)f * T), cell, col);
      if (!(isfinite(col[0]) && isfinite(col[1]) && isfinite(col[2]))) col[0] = col[1] = col[2] = 0.0;
    }
  }
  out[0] = (float)col[0];
  out[1] = (float)col[1];
  out[2] = (float)col[2];
}

// ---- K36
constexpr int kFixedBits = 36;                    // fractional bits below 2^e (gradient) or below 1 (coverage)
constexpr int64_t kBwdMaxPixels = 1ll << 25;      // (see the overflow bound above)

__device__ __forceinline__ int gmax_exponent(unsigned bits) {
  const int biased = (int)((bits >> 23) & 0xFFu);
  return (biased > 0 ? biased : 1) - 127;
}

// the pixel's gradient where it is finite -> max_c |g_c| as bits; false where a component is not finite
__device__ __forceinline__ bool finite_grad(const float* __restrict__ g, float out[3], unsigned& mag) {
  out[0] = g[0];
  out[1] = g[1];
  out[2] = g[2];
  if (!(isfinite(out[0]) && isfinite(out[1]) && isfinite(out[2]))) return false;
  mag = __float_as_uint(fmaxf(fmaxf(fabsf(out[0]), fabsf(out[1])), fabsf(out[2])));
  return true;
}

__global__ __launch_bounds__(kShadeBlock) void face_texel_gmax_kernel(tp_face_texel_shade_bwd_args a, int blocks_per_image, unsigned* gmax) {
  const int b = (int)(blockIdx.x / (unsigned)blocks_per_image);
  const int64_t hw = (int64_t)a.H * a.W;
  const int64_t rem = (int64_t)(blockIdx.x - (unsigned)b * (unsigned)blocks_per_image) * kShadeBlock + threadIdx.x;
  unsigned m = 0;
  if (rem < hw) {
    const int64_t pix = (int64_t)b * hw + rem;
    const int f = a.face[pix];
    float g[3];
    unsigned mag = 0;
    if (f >= 0 && f < a.F && finite_grad(a.grad_rgb + 3 * pix, g, mag) && mag != 0) {      // (a zero gradient cannot raise the maximum)
      const int i = (int)(rem / a.W), j = (int)(rem - (int64_t)i * a.W);
      TexelCell cell;
      if (face_texel_cell(a.verts, a.faces, a.pose + 12 * (int64_t)b, a.intr + 9 * (int64_t)b, a.V, a.R, f, i, j, cell)) m = mag;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {           // every lane of the wavefront is here: no lane returned above
    const unsigned o = (unsigned)__shfl_xor((int)m, off, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(gmax, m);
}

__global__ __launch_bounds__(kShadeBlock) void face_texel_scatter_kernel(tp_face_texel_shade_bwd_args a, int blocks_per_image, int T, int64_t N,
                                                                         unsigned long long* acc, unsigned long long* wacc, const unsigned* gmax) {
  const int b = (int)(blockIdx.x / (unsigned)blocks_per_image);
  const int64_t hw = (int64_t)a.H * a.W;
  const int64_t rem = (int64_t)(blockIdx.x - (unsigned)b * (unsigned)blocks_per_image) * kShadeBlock + threadIdx.x;
  if (rem >= hw) return;
  const int64_t pix = (int64_t)b * hw + rem;
  const int f = a.face[pix];
  if (f < 0 || f >= a.F) return;
  float g[3];
  unsigned mag = 0;
  if (!finite_grad(a.grad_rgb + 3 * pix, g, mag)) return;
  if (mag == 0 && !wacc) return;                      // nothing to add
  const int i = (int)(rem / a.W), j = (int)(rem - (int64_t)i * a.W);
  TexelCell cell;
  if (!face_texel_cell(a.verts, a.faces, a.pose + 12 * (int64_t)b, a.intr + 9 * (int64_t)b, a.V, a.R, f, i, j, cell)) return;
  const double scale = ldexp(1.0, kFixedBits - gmax_exponent(*gmax));
  const double one = ldexp(1.0, kFixedBits);
  for (int k = 0; k < 3; ++k) {
    const int64_t slot = (int64_t)f * T + cell.n[k];
    int64_t d = slot;
    if (a.node_index) {
      d = a.node_index[slot];
      if (d < 0 || d >= N) continue;
    }
    if (mag != 0) {
      for (int c = 0; c < 3; ++c) {
        const long long q = llrint((cell.w[k] * (double)g[c]) * scale);
        if (q != 0) atomicAdd(acc + 3 * d + c, (unsigned long long)q);
      }
    }
    if (wacc) {
      const long long q = llrint(cell.w[k] * one);
      if (q != 0) atomicAdd(wacc + d, (unsigned long long)q);
    }
  }
}

__global__ __launch_bounds__(kShadeBlock) void face_texel_finalise_kernel(const long long* acc, const long long* wacc, const unsigned* gmax, int64_t N,
                                                                          float* grad, float* weight) {
  const int64_t t = (int64_t)blockIdx.x * kShadeBlock + threadIdx.x;
  if (t < 3 * N) grad[t] = (float)ldexp((double)acc[t], gmax_exponent(*gmax) - kFixedBits);
  if (wacc && t < N) weight[t] = (float)ldexp((double)wacc[t], -kFixedBits);
}
}  // namespace

extern "C" int tp_face_texel_count(int R) {
  return R >= 1 && R <= TP_FACE_TEXEL_MAX_R ? (R + 1) * (R + 2) / 2 : 0;
}

extern "C" int tp_face_texel_shade(const tp_face_texel_shade_args* a, tp_stream_t stream) {
  if (!a) { tp::set_error("tp_face_texel_shade: null args"); return -1; }
  if (!a->verts || !a->faces || !a->texels || !a->pose || !a->intr || !a->face || !a->rgb) {
    tp::set_error("tp_face_texel_shade: null pointer");
    return -1;
  }
  const int T = tp_face_texel_count(a->R);
  if (a->B <= 0 || a->H <= 0 || a->W <= 0 || a->V <= 0 || a->F <= 0 || T == 0 || (int64_t)a->H * a->W > 0x7FFFFFFFll ||
      (int64_t)a->F * T > 0x7FFFFFFFll) {
    tp::set_error("tp_face_texel_shade: bad sizes (B, H, W, V, F > 0, R 1..%d, H * W < 2^31, F * T(R) < 2^31)", TP_FACE_TEXEL_MAX_R);
    return -1;
  }
  const int64_t bpi = ((int64_t)a->H * a->W + kShadeBlock - 1) / kShadeBlock;
  if (bpi * a->B > 0x7FFFFFFFll) { tp::set_error("tp_face_texel_shade: bad sizes (B * ceil(H * W / 256) < 2^31)"); return -1; }
  hipLaunchKernelGGL(face_texel_shade_kernel, dim3((unsigned)(bpi * a->B)), dim3(kShadeBlock), 0, (hipStream_t)stream, *a, (int)bpi, T);
  return tp::check_launch("tp_face_texel_shade");
}

extern "C" size_t tp_face_texel_shade_bwd_workspace(int64_t N, int want_weight) {
  if (N <= 0 || N > 0x7FFFFFFFll / 3) return 0;
  return (size_t)8 * (size_t)(3 * N + (want_weight ? N : 0) + 1);
}

extern "C" int tp_face_texel_shade_bwd(const tp_face_texel_shade_bwd_args* a, tp_stream_t stream) {
  const char* name = "tp_face_texel_shade_bwd";
  if (!a) { tp::set_error("%s: null args", name); return -1; }
  if (!a->verts || !a->faces || !a->pose || !a->intr || !a->face || !a->grad_rgb || !a->grad) {
    tp::set_error("%s: null pointer", name);
    return -1;
  }
  const int T = tp_face_texel_count(a->R);
  if (a->B <= 0 || a->H <= 0 || a->W <= 0 || a->V <= 0 || a->F <= 0 || T == 0 || (int64_t)a->H * a->W > 0x7FFFFFFFll ||
      (int64_t)a->F * T > 0x7FFFFFFFll) {
    tp::set_error("%s: bad sizes (B, H, W, V, F > 0, R 1..%d, H * W < 2^31, F * T(R) < 2^31)", name, TP_FACE_TEXEL_MAX_R);
    return -1;
  }
  if ((int64_t)a->B * a->H * a->W > kBwdMaxPixels) {
    tp::set_error("%s: bad sizes (B * H * W <= 2^25: the 64-bit fixed-point sums cannot overflow below that)", name);
    return -1;
  }
  if (a->node_index && a->U <= 0) { tp::set_error("%s: bad sizes (U > 0 with a node index)", name); return -1; }
  const int64_t N = a->node_index ? (int64_t)a->U : (int64_t)a->F * T;
  if (3 * N >= 0x80000000ll) { tp::set_error("%s: bad sizes (3 N < 2^31 destinations)", name); return -1; }
  if (!a->workspace || ((uintptr_t)a->workspace & 7u)) { tp::set_error("%s: workspace null or not 8-byte aligned", name); return -1; }
  const int64_t bpi = ((int64_t)a->H * a->W + kShadeBlock - 1) / kShadeBlock;      // (B * bpi <= 2^25 + B < 2^31)
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* acc = (unsigned long long*)a->workspace;
  unsigned long long* wacc = a->weight ? acc + 3 * N : nullptr;
  unsigned* gmax = (unsigned*)(acc + 3 * N + (a->weight ? N : 0));
  hipError_t e = hipMemsetAsync(a->workspace, 0, tp_face_texel_shade_bwd_workspace(N, a->weight != nullptr), s);
  if (e != hipSuccess) { tp::set_error("%s: hipMemsetAsync: %s", name, hipGetErrorString(e)); return (int)e; }
  hipLaunchKernelGGL(face_texel_gmax_kernel, dim3((unsigned)(bpi * a->B)), dim3(kShadeBlock), 0, s, *a, (int)bpi, gmax);
  hipLaunchKernelGGL(face_texel_scatter_kernel, dim3((unsigned)(bpi * a->B)), dim3(kShadeBlock), 0, s, *a, (int)bpi, T, N, acc, wacc, (const unsigned*)gmax);
  hipLaunchKernelGGL(face_texel_finalise_kernel, dim3((unsigned)((3 * N + kShadeBlock - 1) / kShadeBlock)), dim3(kShadeBlock), 0, s,
                     (const long long*)acc, (const long long*)wacc, (const unsigned*)gmax, N, a->grad, a->weight);
  return tp::check_launch(name);
}
