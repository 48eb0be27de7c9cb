// K22  per-object annotations of a scene of K objects at B novel poses (tp_scene_annotate), and the 8-bit / 16-bit images of a rendered
// view (tp_view_images): what a BOP scene folder stores per frame, made on the device from K21's inputs and outputs.
//
// tp_scene_annotate.  Inputs: tp_mesh_raster's zbuf planes [K,B,H,W] (mm, <= 0 or NaN on background), K21's label [B,H*W], ids [K]
// (distinct).  Per object k, pose b and pixel p:
//   all_k(p)   = zbuf[k,b,p] > 0                      (the full silhouette inside the image)
//   visib_k(p) = all_k(p) && label[b,p] == ids[k]     (the part no nearer object hides)
//   info[b,k]  = { |all_k|, |visib_k|, xmin, ymin, xmax, ymax of all_k, xmin, ymin, xmax, ymax of visib_k }   (int32 x 10)
//                inclusive pixel indices, x = column, y = row; an empty set gives -1 in its four extents
//   mask[b,k,p] = all_k(p) ? 255 : 0,  mask_visib[b,k,p] = visib_k(p) ? 255 : 0                              (uint8, optional)
//
// Two launches inside the call.  The first writes the neutral element of every entry of info (0 for the counts, -1 for the extents).
// The second runs one block of 256 threads per (object, row band, pose): a thread owns V consecutive pixels of a row per step
// (V = 4 when W is a multiple of four and the buffers are aligned: one 16-byte load of the plane and of the label, one 4-byte store
// per mask; else V = 1).  Counts are summed per wavefront with ballot + popcount (they never occupy a vector register), the extents
// are kept per thread and reduced across the 64 lanes at the end, then across the four wavefronts through 160 bytes of LDS, and ten
// lanes of the first wavefront issue the block's ten integer atomics: add for the counts, signed max for xmax / ymax, UNSIGNED min
// for xmin / ymin -- -1 is the largest unsigned value, so the neutral element of the minimum is also the value an empty set must
// report and no finalising pass is needed.  A block that saw no pixel of its object issues nothing.  Integer add / min / max are
// associative and commutative: the result does not depend on the grid, the band height or the arrival order.
//
// Object is the fastest grid dimension: the K blocks that read one band of `label` are dispatched together, so the re-reads are
// served by L2 / the Infinity Cache and HBM sees the algorithmic 4 K + 4 bytes read and 2 K bytes written per pixel.
//
// tp_view_images.  rgb [B,H*W,3] -> rgb8 [B,H,W,3] = uint8(trunc(clamp(x, 0, 1) * 255)); depth [B,H*W] (NeRF units) -> depth16
// [B,H,W] = uint16(trunc(clamp((d / depth_scale) * png_per_metre, 0, 65535))); NaN gives 0; every step one rounded fp32 operation.
// One launch, four values per thread where the sizes and the alignment allow.
#include "tp_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / tp::kWave;
constexpr int kInfo = TP_SCENE_INFO_FIELDS;
constexpr int kBandPixels = 8192;             // pixels of one object a block reduces before it touches memory

struct Params {
  const float* zbuf; const int32_t* label; const int32_t* ids;
  int B, H, W, K, rows_per_band;
  int32_t* info; uint8_t* mask; uint8_t* mask_visib;
};

__global__ void __launch_bounds__(kThreads) scene_annotate_init_kernel(int32_t* info, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) info[i] = (i % kInfo) < 2 ? 0 : -1;
}

template <int V> struct Vec;
template <> struct Vec<1> { using F = float; using I = int32_t; using U8 = uint8_t; };
template <> struct Vec<4> { using F = float4; using I = int4; using U8 = uchar4; };

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)v, s, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ int32_t wave_max_i32(int32_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) { const int32_t o = __shfl_xor(v, s, 64); v = o > v ? o : v; }
  return v;
}

template <int V>
__global__ void __launch_bounds__(kThreads) scene_annotate_kernel(Params p) {
  using VF = typename Vec<V>::F;
  using VI = typename Vec<V>::I;
  using VB = typename Vec<V>::U8;
  const int k = blockIdx.x, band = blockIdx.y, b = blockIdx.z;
  const int row0 = band * p.rows_per_band;
  const int rows = min(p.rows_per_band, p.H - row0);
  const int n = rows * p.W;                                          // pixels of the band (V = 4: a multiple of four)
  const int64_t hw = (int64_t)p.H * p.W;
  const int64_t band0 = (int64_t)row0 * p.W;
  const float* plane = p.zbuf + ((int64_t)k * p.B + b) * hw + band0;
  const int32_t* label = p.label + (int64_t)b * hw + band0;
  const int64_t mask0 = ((int64_t)b * p.K + k) * hw + band0;
  const int32_t id = p.ids[k];

  uint32_t cnt_all = 0, cnt_vis = 0;                                 // wave-uniform
  uint32_t xmin[2] = {0xffffffffu, 0xffffffffu}, ymin[2] = {0xffffffffu, 0xffffffffu};
  int32_t xmax[2] = {-1, -1}, ymax[2] = {-1, -1};                    // [0]: all_k, [1]: visib_k
  // every thread of a wavefront runs the same number of steps (the ballots need the whole wavefront); lanes past the end hold nothing
  for (int q0 = 0; q0 < n; q0 += kThreads * V) {
    const int q = q0 + (int)threadIdx.x * V;
    const bool live = q < n;
    float z[V];
    int32_t l[V];
#pragma unroll
    for (int e = 0; e < V; ++e) { z[e] = -1.0f; l[e] = 0; }
    if (live) {
      const VF zv = *reinterpret_cast<const VF*>(plane + q);
      const VI lv = *reinterpret_cast<const VI*>(label + q);
      __builtin_memcpy(z, &zv, sizeof(zv));
      __builtin_memcpy(l, &lv, sizeof(lv));
    }
    const int r = q / p.W;                                           // (V = 4: W is a multiple of four, the vector lies in one row)
    const int y = row0 + r, x = q - r * p.W;
    uint8_t m_all[V], m_vis[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const bool a = z[e] > 0.0f;                                    // (NaN counts as background)
      const bool v = a && l[e] == id;
      cnt_all += (uint32_t)__popcll(__ballot(a));
      cnt_vis += (uint32_t)__popcll(__ballot(v));
      m_all[e] = a ? 255 : 0;
      m_vis[e] = v ? 255 : 0;
      if (a) { xmin[0] = min(xmin[0], (uint32_t)(x + e)); xmax[0] = max(xmax[0], x + e); }
      if (v) { xmin[1] = min(xmin[1], (uint32_t)(x + e)); xmax[1] = max(xmax[1], x + e); }
    }
    bool any_a = false, any_v = false;
#pragma unroll
    for (int e = 0; e < V; ++e) { any_a |= m_all[e] != 0; any_v |= m_vis[e] != 0; }
    if (any_a) { ymin[0] = min(ymin[0], (uint32_t)y); ymax[0] = max(ymax[0], y); }
    if (any_v) { ymin[1] = min(ymin[1], (uint32_t)y); ymax[1] = max(ymax[1], y); }
    if (live && p.mask) {
      VB o;
      __builtin_memcpy(&o, m_all, sizeof(o));
      *reinterpret_cast<VB*>(p.mask + mask0 + q) = o;
    }
    if (live && p.mask_visib) {
      VB o;
      __builtin_memcpy(&o, m_vis, sizeof(o));
      *reinterpret_cast<VB*>(p.mask_visib + mask0 + q) = o;
    }
  }

  // info order: count_all, count_visib, (xmin, ymin, xmax, ymax) of all_k, the same of visib_k
  __shared__ int32_t part[kWaves][kInfo];
  const int lane = threadIdx.x & (tp::kWave - 1), wave = threadIdx.x / tp::kWave;
  int32_t mine[kInfo];
  mine[0] = (int32_t)cnt_all; mine[1] = (int32_t)cnt_vis;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    mine[2 + 4 * s] = (int32_t)wave_min_u32(xmin[s]);
    mine[3 + 4 * s] = (int32_t)wave_min_u32(ymin[s]);
    mine[4 + 4 * s] = wave_max_i32(xmax[s]);
    mine[5 + 4 * s] = wave_max_i32(ymax[s]);
  }
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < kInfo; ++j) part[wave][j] = mine[j];
  }
  __syncthreads();
  if (threadIdx.x < kInfo) {
    const int j = threadIdx.x;
    const bool is_count = j < 2, is_min = !is_count && ((j - 2) & 2) == 0;
    int32_t v = part[0][j];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      const int32_t o = part[w][j];
      v = is_count ? v + o : is_min ? (int32_t)min((uint32_t)v, (uint32_t)o) : max(v, o);
    }
    if (part[0][0] + part[1][0] + part[2][0] + part[3][0] > 0) {     // the block saw its object: else every value is neutral
      int32_t* dst = p.info + ((int64_t)b * p.K + k) * kInfo + j;
      if (is_count) atomicAdd(dst, v);
      else if (is_min) atomicMin(reinterpret_cast<uint32_t*>(dst), (uint32_t)v);
      else atomicMax(dst, v);
    }
  }
}
static_assert(kWaves == 4, "the block total above sums four wavefronts");

struct ImageParams {
  const float* rgb; const float* depth;
  int64_t n_rgb, n_depth;                                            // values: 3 B H W and B H W
  float depth_scale, png_per_metre;
  uint8_t* rgb8; uint16_t* depth16;
};

__device__ __forceinline__ uint8_t to_u8(float x) {
  x = x > 0.0f ? x : 0.0f;                                           // (NaN -> 0)
  x = x < 1.0f ? x : 1.0f;
  return (uint8_t)(int)tp::mul_rn(x, 255.0f);
}
__device__ __forceinline__ uint16_t to_u16(float d, float scale, float per_metre) {
  float m = tp::mul_rn(tp::div_rn(d, scale), per_metre);
  m = m > 0.0f ? m : 0.0f;                                           // (NaN -> 0)
  m = m < 65535.0f ? m : 65535.0f;
  return (uint16_t)(int)m;
}

template <int V>
__global__ void __launch_bounds__(kThreads) view_images_kernel(ImageParams p) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i < p.n_rgb) {
    if (V == 4) {
      const float4 x = *reinterpret_cast<const float4*>(p.rgb + i);
      *reinterpret_cast<uchar4*>(p.rgb8 + i) = make_uchar4(to_u8(x.x), to_u8(x.y), to_u8(x.z), to_u8(x.w));
    } else {
      p.rgb8[i] = to_u8(p.rgb[i]);
    }
  }
  if (i < p.n_depth) {
    if (V == 4) {
      const float4 d = *reinterpret_cast<const float4*>(p.depth + i);
      *reinterpret_cast<ushort4*>(p.depth16 + i) =
          make_ushort4(to_u16(d.x, p.depth_scale, p.png_per_metre), to_u16(d.y, p.depth_scale, p.png_per_metre),
                       to_u16(d.z, p.depth_scale, p.png_per_metre), to_u16(d.w, p.depth_scale, p.png_per_metre));
    } else {
      p.depth16[i] = to_u16(p.depth[i], p.depth_scale, p.png_per_metre);
    }
  }
}

inline bool aligned(const void* q, uintptr_t a) { return ((uintptr_t)q & (a - 1)) == 0; }

}  // namespace

extern "C" int tp_scene_annotate(const tp_scene_annotate_args* a, tp_stream_t stream) {
  TP_REQUIRE(a, "null pointer");
  TP_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->H <= 16384 && a->W <= 16384 && a->B <= 65535, "bad sizes");
  TP_REQUIRE(a->K >= 1 && a->K <= TP_SCENE_MAX_OBJECTS, "1 <= K <= 32 objects expected");
  TP_REQUIRE(a->zbuf && a->label && a->ids, "null pointer (zbuf / label / ids)");
  TP_REQUIRE(a->info, "null output pointer (info)");
  const int64_t hw = (int64_t)a->H * a->W;
  TP_REQUIRE((int64_t)a->B * hw <= (int64_t)INT32_MAX, "bad sizes (more than 2^31 - 1 pixels)");
  Params p;
  p.zbuf = a->zbuf; p.label = a->label; p.ids = a->ids;
  p.B = a->B; p.H = a->H; p.W = a->W; p.K = a->K;
  p.info = a->info; p.mask = a->mask; p.mask_visib = a->mask_visib;
  p.rows_per_band = (kBandPixels + a->W - 1) / a->W;
  if (p.rows_per_band > a->H) p.rows_per_band = a->H;
  const int bands = (a->H + p.rows_per_band - 1) / p.rows_per_band;
  TP_REQUIRE(bands <= 65535, "bad sizes");
  const int n_info = a->B * a->K * kInfo;
  hipLaunchKernelGGL(scene_annotate_init_kernel, dim3((unsigned)((n_info + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     a->info, n_info);
  const dim3 grid((unsigned)a->K, (unsigned)bands, (unsigned)a->B);
  const bool vec4 = (a->W & 3) == 0 && aligned(a->zbuf, 16) && aligned(a->label, 16) && (!a->mask || aligned(a->mask, 4)) &&
                    (!a->mask_visib || aligned(a->mask_visib, 4));
  if (vec4) {
    hipLaunchKernelGGL(scene_annotate_kernel<4>, grid, dim3(kThreads), 0, (hipStream_t)stream, p);
  } else {
    hipLaunchKernelGGL(scene_annotate_kernel<1>, grid, dim3(kThreads), 0, (hipStream_t)stream, p);
  }
  return tp::check_launch("tp_scene_annotate");
}

extern "C" int tp_view_images(const tp_view_images_args* a, tp_stream_t stream) {
  TP_REQUIRE(a, "null pointer");
  TP_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->H <= 16384 && a->W <= 16384, "bad sizes");
  TP_REQUIRE((a->rgb != nullptr) == (a->rgb8 != nullptr) && (a->depth != nullptr) == (a->depth16 != nullptr),
             "rgb with rgb8 and depth with depth16 expected (a pair may be left out as a whole)");
  TP_REQUIRE(a->rgb || a->depth, "null pointer (neither rgb nor depth)");
  TP_REQUIRE(!a->depth || (a->depth_scale > 0.0f && a->png_per_metre > 0.0f), "depth_scale and png_per_metre must be positive");
  const int64_t n = (int64_t)a->B * a->H * a->W;
  TP_REQUIRE(n <= (int64_t)INT32_MAX, "bad sizes (more than 2^31 - 1 pixels)");
  ImageParams p;
  p.rgb = a->rgb; p.depth = a->depth; p.rgb8 = a->rgb8; p.depth16 = a->depth16;
  p.n_rgb = a->rgb ? 3 * n : 0; p.n_depth = a->depth ? n : 0;
  p.depth_scale = a->depth_scale; p.png_per_metre = a->png_per_metre;
  const int64_t longest = p.n_rgb > p.n_depth ? p.n_rgb : p.n_depth;
  const bool vec4 = (n & 3) == 0 && (!a->rgb || (aligned(a->rgb, 16) && aligned(a->rgb8, 4))) &&
                    (!a->depth || (aligned(a->depth, 16) && aligned(a->depth16, 8)));
  if (vec4) {
    hipLaunchKernelGGL(view_images_kernel<4>, dim3((unsigned)((longest / 4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, p);
  } else {
    hipLaunchKernelGGL(view_images_kernel<1>, dim3((unsigned)((longest + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, p);
  }
  return tp::check_launch("tp_view_images");
}
