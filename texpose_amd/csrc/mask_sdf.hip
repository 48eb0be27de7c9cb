// K31a tp_mask_sdf: the exact signed Euclidean distance field of F masks (the public functions are in
// texpose_amd/silhouette.py, the rules in include/texpose_amd.h).
//
//   sdf_columns grid F * ceil(W / 256) x 256.  A thread owns a column: one sweep down and one up leave, per pixel, the vertical
//               distance to the nearest set and to the nearest clear pixel of the column as two 16-bit halves of one word of the
//               workspace (0xFFFF: the column has none; H <= 8192 keeps every real distance below it).  Neighbouring threads read and
//               write neighbouring words.
//   sdf_rows    grid F * H x 256.  A workgroup owns a row: its W words go to LDS, and a thread takes, for each of its pixels
//               j = t, t + 256, ..., the minimum over j' of (j - j')^2 + g[j']^2 of the field the pixel's sign asks for (a clear pixel
//               needs the set pixels, a set pixel the clear ones), walking outwards from j until (j - j')^2 reaches the best so far.
// Integer minima: any order gives the same bits.  No atomics, vector stores only.
//
// K31c tp_mask_sdf_known: the same two kernels with a third class of pixel, UNKNOWN (known == 0), which is neither
//   set nor clear.  In the column sweeps an unknown pixel advances both distances, so the two halves of its word are both non-zero:
//   the row kernel tells the classes apart as ds == 0: set, dc == 0: clear, neither: unknown, and stores a quiet NaN there without a
//   scan.  The <false> instances are tp_mask_sdf's kernels as they were.
// K32 tp_mask_known_from_others: the known planes of the N instance masks of one frame from their fields.
//   known_from_others grid ceil(ceil(H * W / 4) / 256) x 256.  A thread owns four consecutive flat pixels: it walks the N planes once,
//               keeping per pixel the number of instances the pixel is near to and the index of one of them, then writes the N x 4
//               bytes.  With H * W a multiple of 4 (and the pointers aligned) a plane's four values are one 16-byte load and one
//               4-byte store; otherwise four scalar ones.
#include "tp_common.h"

namespace {
constexpr int kSdfBlock = 256;
constexpr int kSdfMax = 8192;                          // H, W at most: distances fit 16 bits, a row's words fit 32 KiB of LDS
constexpr uint32_t kNone = 0xFFFFu;

__device__ __forceinline__ uint32_t step_from(uint32_t d) { return d == kNone ? kNone : d + 1u; }
__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }

template <bool kKnown>
__global__ __launch_bounds__(kSdfBlock) void sdf_columns_kernel(const uint8_t* mask, const uint8_t* known, uint32_t* ws, int H, int W, int strips) {
  const int f = blockIdx.x / strips;                   // (strips = ceil(W / 256) workgroups per plane)
  const int j = (blockIdx.x - f * strips) * kSdfBlock + threadIdx.x;
  if (j >= W) return;
  const int64_t plane = (int64_t)H * W;
  const uint8_t* pm = mask + (int64_t)f * plane + j;
  const uint8_t* pk = kKnown ? known + (int64_t)f * plane + j : nullptr;
  uint32_t* pw = ws + (int64_t)f * plane + j;
  uint32_t ds = kNone, dc = kNone;                     // distance to the last set / clear pixel met
  for (int i = 0; i < H; ++i) {
    const bool set = pm[(int64_t)i * W] != 0;
    const bool unknown = kKnown && pk[(int64_t)i * W] == 0;  // (neither set nor clear: both distances go on)
    ds = set && !unknown ? 0u : step_from(ds);
    dc = set || unknown ? step_from(dc) : 0u;
    pw[(int64_t)i * W] = ds | dc << 16;
  }
  ds = kNone; dc = kNone;
  for (int i = H - 1; i >= 0; --i) {
    const uint32_t down = pw[(int64_t)i * W];          // (this thread's own store)
    const bool set = (down & 0xFFFFu) == 0u;
    const bool unknown = kKnown && !set && (down >> 16) != 0u;
    ds = set ? 0u : step_from(ds);
    dc = set || unknown ? step_from(dc) : 0u;
    pw[(int64_t)i * W] = umin32(down & 0xFFFFu, ds) | umin32(down >> 16, dc) << 16;
  }
}

template <bool kKnown>
__global__ __launch_bounds__(kSdfBlock) void sdf_rows_kernel(const uint32_t* ws, float* sdf, int H, int W) {
  extern __shared__ uint32_t row[];                    // [W]
  const int64_t base = (int64_t)blockIdx.x * W;        // (row blockIdx.x of the F * H rows; < 2^31)
  for (int j = threadIdx.x; j < W; j += kSdfBlock) row[j] = ws[base + j];
  __syncthreads();
  const uint32_t none2 = (uint32_t)H * (uint32_t)H + (uint32_t)W * (uint32_t)W;          // (<= 2^27)
  for (int j = threadIdx.x; j < W; j += kSdfBlock) {
    const bool set = (row[j] & 0xFFFFu) == 0u;
    if (kKnown && !set && (row[j] >> 16) != 0u) {        // unknown: neither distance is 0
      sdf[base + j] = __builtin_nanf("");
      continue;
    }
    const int shift = set ? 16 : 0;                    // a set pixel looks for the clear ones
    const uint32_t g0 = row[j] >> shift & 0xFFFFu;
    uint32_t best = g0 == kNone ? none2 : g0 * g0;
    for (int d = 1; (uint32_t)d * (uint32_t)d < best && (j - d >= 0 || j + d < W); ++d) {
      const uint32_t d2 = (uint32_t)d * (uint32_t)d;
      if (j - d >= 0) {
        const uint32_t g = row[j - d] >> shift & 0xFFFFu;
        if (g != kNone) best = umin32(best, d2 + g * g);
      }
      if (j + d < W) {
        const uint32_t g = row[j + d] >> shift & 0xFFFFu;
        if (g != kNone) best = umin32(best, d2 + g * g);
      }
    }
    // sqrtf correctly rounded whatever the build's fp32 sqrt is: the fp64 root rounded to fp32 is (53 >= 2 x 24 + 2 bits; best < 2^28 is exact in both)
    const float v = (float)sqrt((double)best) - 0.5f;
    sdf[base + j] = set ? -v : v;
  }
}

template <bool kVec>
__global__ __launch_bounds__(kSdfBlock) void known_from_others_kernel(const float* sdf, uint8_t* known, int N, int plane, float band_px) {
  const int64_t p0 = ((int64_t)blockIdx.x * kSdfBlock + threadIdx.x) * 4;      // this thread's pixels p0 .. p0 + 3 of every plane
  if (p0 >= plane) return;
  const int mine = kVec ? 4 : (plane - p0 < 4 ? (int)(plane - p0) : 4);         // (kVec: plane is a multiple of 4)
  const float limit = band_px - 0.5f;                                          // near(m, p): sdf[m,p] <= band_px - 0.5f, in fp32
  int count[4] = {0, 0, 0, 0}, index[4] = {0, 0, 0, 0};                        // instances the pixel is near to, and one of them
  for (int m = 0; m < N; ++m) {
    const float* ps = sdf + (int64_t)m * plane + p0;
    float v[4];
    if (kVec) {
      const float4 q = *reinterpret_cast<const float4*>(ps);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = k < mine ? ps[k] : __builtin_nanf("");
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (v[k] <= limit) { ++count[k]; index[k] = m; }                           // (a NaN is not near)
  }
  for (int n = 0; n < N; ++n) {
    uint8_t* pk = known + (int64_t)n * plane + p0;
    uint32_t b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = count[k] > 1 || (count[k] == 1 && index[k] != n) ? 0u : 1u;
    if (kVec) {
      *reinterpret_cast<uint32_t*>(pk) = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < mine) pk[k] = (uint8_t)b[k];
    }
  }
}

// what tp_mask_sdf and tp_mask_sdf_known share: the refusals and the two launches (without with_known every pixel is a measurement and
// `known` is not looked at)
int mask_sdf_launch(const char* what, const uint8_t* mask, const uint8_t* known, bool with_known, float* sdf, int F, int H, int W, void* workspace,
                    tp_stream_t stream) {
  if (F <= 0 || H <= 0 || W <= 0 || H > kSdfMax || W > kSdfMax || (int64_t)F * H * W > 0x7FFFFFFFll) {
    tp::set_error("%s: bad sizes (F > 0, H and W 1..8192, F * H * W < 2^31)", what);
    return -1;
  }
  if (!mask || !sdf || !workspace || (with_known && !known)) { tp::set_error("%s: null pointer", what); return -1; }
  if ((uintptr_t)workspace & 15u) { tp::set_error("%s: workspace must be 16-byte aligned", what); return -1; }
  const uintptr_t n = (uintptr_t)F * H * W, m0 = (uintptr_t)mask, k0 = (uintptr_t)known, s0 = (uintptr_t)sdf;
  if (m0 < s0 + n * sizeof(float) && s0 < m0 + n) { tp::set_error("%s: sdf must not overlap mask", what); return -1; }
  if (with_known && k0 < s0 + n * sizeof(float) && s0 < k0 + n) { tp::set_error("%s: sdf must not overlap known", what); return -1; }
  hipStream_t st = (hipStream_t)stream;
  uint32_t* ws = static_cast<uint32_t*>(workspace);
  const int strips = (W + kSdfBlock - 1) / kSdfBlock;                            // (F * strips <= F * W < 2^31)
  const size_t lds = (size_t)W * sizeof(uint32_t);
  if (with_known) {
    hipLaunchKernelGGL(sdf_columns_kernel<true>, dim3(F * strips), dim3(kSdfBlock), 0, st, mask, known, ws, H, W, strips);
    hipLaunchKernelGGL(sdf_rows_kernel<true>, dim3(F * H), dim3(kSdfBlock), lds, st, (const uint32_t*)ws, sdf, H, W);
  } else {
    hipLaunchKernelGGL(sdf_columns_kernel<false>, dim3(F * strips), dim3(kSdfBlock), 0, st, mask, known, ws, H, W, strips);
    hipLaunchKernelGGL(sdf_rows_kernel<false>, dim3(F * H), dim3(kSdfBlock), lds, st, (const uint32_t*)ws, sdf, H, W);
  }
  return tp::check_launch(what);
}
}  // namespace

extern "C" size_t tp_mask_sdf_workspace_bytes(int F, int H, int W) {
  if (F <= 0 || H <= 0 || W <= 0) return 0;
  const size_t bytes = (size_t)F * (size_t)H * (size_t)W * sizeof(uint32_t);
  return (bytes + 15) & ~(size_t)15;
}

extern "C" int tp_mask_sdf(const uint8_t* mask, float* sdf, int F, int H, int W, void* workspace, tp_stream_t stream) {
  return mask_sdf_launch("tp_mask_sdf", mask, nullptr, false, sdf, F, H, W, workspace, stream);
}

extern "C" int tp_mask_sdf_known(const uint8_t* mask, const uint8_t* known, float* sdf, int F, int H, int W, void* workspace, tp_stream_t stream) {
  return mask_sdf_launch("tp_mask_sdf_known", mask, known, true, sdf, F, H, W, workspace, stream);
}

extern "C" int tp_mask_known_from_others(const float* sdf, uint8_t* known, int N, int H, int W, float band_px, tp_stream_t stream) {
  const char* what = "tp_mask_known_from_others";
  if (N <= 0 || H <= 0 || W <= 0 || N > 65535 || (int64_t)N * H * W > 0x7FFFFFFFll) {
    tp::set_error("%s: bad sizes (N 1..65535, H and W > 0, N * H * W < 2^31)", what);
    return -1;
  }
  if (!sdf || !known) { tp::set_error("%s: null pointer", what); return -1; }
  if (!(band_px >= 0.0f) || !(band_px <= 3.402823466e38f)) { tp::set_error("%s: band_px must be finite and >= 0", what); return -1; }
  const uintptr_t n = (uintptr_t)N * H * W, k0 = (uintptr_t)known, s0 = (uintptr_t)sdf;
  if (k0 < s0 + n * sizeof(float) && s0 < k0 + n) { tp::set_error("%s: known must not overlap sdf", what); return -1; }
  hipStream_t st = (hipStream_t)stream;
  const int plane = H * W;                                                       // (< 2^31)
  const int blocks = (int)((((int64_t)plane + 3) / 4 + kSdfBlock - 1) / kSdfBlock);
  if (plane % 4 == 0 && (s0 & 15u) == 0 && (k0 & 3u) == 0)
    hipLaunchKernelGGL(known_from_others_kernel<true>, dim3(blocks), dim3(kSdfBlock), 0, st, sdf, known, N, plane, band_px);
  else
    hipLaunchKernelGGL(known_from_others_kernel<false>, dim3(blocks), dim3(kSdfBlock), 0, st, sdf, known, N, plane, band_px);
  return tp::check_launch(what);
}
