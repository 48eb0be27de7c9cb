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
#include "tp_common.h"

namespace {
constexpr int kSdfBlock = 256;
constexpr int kSdfMax = 8192;                          // H, W at most: distances fit 16 bits, a row's words fit 32 KiB of LDS
constexpr uint32_t kNone = 0xFFFFu;

__device__ __forceinline__ uint32_t step_from(uint32_t d) { return d == kNone ? kNone : d + 1u; }
__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }

__global__ __launch_bounds__(kSdfBlock) void sdf_columns_kernel(const uint8_t* mask, uint32_t* ws, int H, int W, int strips) {
  const int f = blockIdx.x / strips;                   // (strips = ceil(W / 256) workgroups per plane)
  const int j = (blockIdx.x - f * strips) * kSdfBlock + threadIdx.x;
  if (j >= W) return;
  const int64_t plane = (int64_t)H * W;
  const uint8_t* pm = mask + (int64_t)f * plane + j;
  uint32_t* pw = ws + (int64_t)f * plane + j;
  uint32_t ds = kNone, dc = kNone;                     // distance to the last set / clear pixel met
  for (int i = 0; i < H; ++i) {
    const bool set = pm[(int64_t)i * W] != 0;
    ds = set ? 0u : step_from(ds);
    dc = set ? step_from(dc) : 0u;
    pw[(int64_t)i * W] = ds | dc << 16;
  }
  ds = kNone; dc = kNone;
  for (int i = H - 1; i >= 0; --i) {
    const uint32_t down = pw[(int64_t)i * W];          // (this thread's own store)
    const bool set = (down & 0xFFFFu) == 0u;
    ds = set ? 0u : step_from(ds);
    dc = set ? step_from(dc) : 0u;
    pw[(int64_t)i * W] = umin32(down & 0xFFFFu, ds) | umin32(down >> 16, dc) << 16;
  }
}

__global__ __launch_bounds__(kSdfBlock) void sdf_rows_kernel(const uint32_t* ws, float* sdf, int H, int W) {
  extern __shared__ uint32_t row[];                    // [W]
  const int64_t base = (int64_t)blockIdx.x * W;        // (row blockIdx.x of the F * H rows; < 2^31)
  for (int j = threadIdx.x; j < W; j += kSdfBlock) row[j] = ws[base + j];
  __syncthreads();
  const uint32_t none2 = (uint32_t)H * (uint32_t)H + (uint32_t)W * (uint32_t)W;          // (<= 2^27)
  for (int j = threadIdx.x; j < W; j += kSdfBlock) {
    const bool set = (row[j] & 0xFFFFu) == 0u;
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
}  // namespace

extern "C" size_t tp_mask_sdf_workspace_bytes(int F, int H, int W) {
  if (F <= 0 || H <= 0 || W <= 0) return 0;
  const size_t bytes = (size_t)F * (size_t)H * (size_t)W * sizeof(uint32_t);
  return (bytes + 15) & ~(size_t)15;
}

extern "C" int tp_mask_sdf(const uint8_t* mask, float* sdf, int F, int H, int W, void* workspace, tp_stream_t stream) {
  if (F <= 0 || H <= 0 || W <= 0 || H > kSdfMax || W > kSdfMax || (int64_t)F * H * W > 0x7FFFFFFFll) {
    tp::set_error("tp_mask_sdf: bad sizes (F > 0, H and W 1..8192, F * H * W < 2^31)");
    return -1;
  }
  if (!mask || !sdf || !workspace) { tp::set_error("tp_mask_sdf: null pointer"); return -1; }
  if ((uintptr_t)workspace & 15u) { tp::set_error("tp_mask_sdf: workspace must be 16-byte aligned"); return -1; }
  const uintptr_t n = (uintptr_t)F * H * W, m0 = (uintptr_t)mask, s0 = (uintptr_t)sdf;
  if (m0 < s0 + n * sizeof(float) && s0 < m0 + n) { tp::set_error("tp_mask_sdf: sdf must not overlap mask"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  uint32_t* ws = static_cast<uint32_t*>(workspace);
  const int strips = (W + kSdfBlock - 1) / kSdfBlock;                            // (F * strips <= F * W < 2^31)
  hipLaunchKernelGGL(sdf_columns_kernel, dim3(F * strips), dim3(kSdfBlock), 0, st, mask, ws, H, W, strips);
  hipLaunchKernelGGL(sdf_rows_kernel, dim3(F * H), dim3(kSdfBlock), (size_t)W * sizeof(uint32_t), st, (const uint32_t*)ws, sdf, H, W);
  return tp::check_launch("tp_mask_sdf");
}
