// K20  the data layer's finish of the surfel maps: what data/lm.py makes of the files compute_surfelinfo.py wrote, on the device
// ref: data/lm.py:196-253 (get_predicted_synthetic_image / _nocs / _normal: 8-bit decode, alpha > 0, smooth_geo),
//      data/lm.py:497-521 (get_edge, smooth_geo), compute_surfelinfo.py:118-140 (the 8-bit encode of the files).
//
// One launch, one thread per pixel, no allocation, no host synchronisation.  Inputs are tp_mesh_raster's interleaved outputs
// ([B,H,W,3]); outputs are planar ([B,3,H,W]), the layout the trainer reads.  Consecutive lanes take consecutive pixels of a row:
// a wavefront reads 768 contiguous bytes per input map (three dword loads at a 12-byte lane stride, every cache line used whole)
// and writes 256 contiguous bytes per output plane.
//
// Per pixel:
//   q(x)        = float(uint8(trunc(x * 255))) / 255: the fp32 product the writer forms ((x * 255).astype(uint8)), truncated toward
//                 zero, and the correctly rounded fp32 quotient the reader forms (to_tensor / `np.float32 / 255`).  The integer is
//                 clamped to [0, 255]; numpy's cast is undefined outside that range (NaN gives 0 here).
//   image_syn   = q(rgb) (never smoothed; zero without rgb), mask_syn = zbuf > 0.
//   nocs_pred   = smooth_geo(q(nocs)), normal_pred = smooth_geo(normal) (the .npz holds float32: no quantisation).
//   smooth_geo  : mask = (channel 0 of the map being smoothed) != 0; a pixel is an edge if it is in the mask and one of its four
//                 neighbours inside the image is not; an edge pixel's channels become the medians of the 3x3 neighbourhood of the
//                 unsmoothed map with replicated borders (cv2.medianBlur(x, 3)); every other pixel keeps its value.
// Only edge pixels (a few per cent) load the 3x3 neighbourhood and run the median network; the others load their own pixel and the
// first channel of four neighbours.
#include "tp_common.h"

namespace {

struct FinishParams {
  const float* rgb; const float* nocs; const float* normal; const float* zbuf;
  int B, H, W, quantize;
  float* image_syn; float* mask_syn; float* nocs_pred; float* normal_pred;
};

__device__ __forceinline__ float quant8(float x) {
  const float t = __fmul_rn(x, 255.0f);
  int k = (t >= 255.0f) ? 255 : (t > 0.0f) ? (int)t : 0;      // trunc toward zero; NaN and negatives -> 0
  return __fdiv_rn((float)k, 255.0f);
}

__device__ __forceinline__ void sort2(float& a, float& b) {
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo; b = hi;
}

// median of nine: the classic 19-exchange network (the exact middle value, as any sort gives)
__device__ __forceinline__ float median9(float (&p)[9]) {
  sort2(p[1], p[2]); sort2(p[4], p[5]); sort2(p[7], p[8]);
  sort2(p[0], p[1]); sort2(p[3], p[4]); sort2(p[6], p[7]);
  sort2(p[1], p[2]); sort2(p[4], p[5]); sort2(p[7], p[8]);
  sort2(p[0], p[3]); sort2(p[5], p[8]); sort2(p[4], p[7]);
  sort2(p[3], p[6]); sort2(p[1], p[4]); sort2(p[2], p[5]);
  sort2(p[4], p[7]); sort2(p[4], p[2]); sort2(p[6], p[4]);
  sort2(p[4], p[2]);
  return p[4];
}

// smooth_geo of one map at pixel (i, j) of an image whose first pixel is `src` ([H,W,3]); QUANT: the map is q(src)
template <bool QUANT>
__device__ __forceinline__ void smooth_geo_pixel(const float* src, int H, int W, int i, int j, float (&out)[3]) {
  auto at = [&](int ii, int jj, int c) {
    const float v = src[3 * ((int64_t)ii * W + jj) + c];
    return QUANT ? quant8(v) : v;
  };
  for (int c = 0; c < 3; ++c) out[c] = at(i, j, c);
  if (!(out[0] != 0.0f)) return;                               // outside the mask: never an edge
  bool edge = false;
  if (i > 0) edge |= !(at(i - 1, j, 0) != 0.0f);
  if (i < H - 1) edge |= !(at(i + 1, j, 0) != 0.0f);
  if (j > 0) edge |= !(at(i, j - 1, 0) != 0.0f);
  if (j < W - 1) edge |= !(at(i, j + 1, 0) != 0.0f);
  if (!edge) return;
  const int i0 = max(i - 1, 0), i1 = min(i + 1, H - 1), j0 = max(j - 1, 0), j1 = min(j + 1, W - 1);
  const int rows[3] = {i0, i, i1}, cols[3] = {j0, j, j1};
  for (int c = 0; c < 3; ++c) {
    float p[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) p[3 * r + s] = at(rows[r], cols[s], c);
    out[c] = median9(p);
  }
}

__global__ void __launch_bounds__(256) surfel_finish_kernel(FinishParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t hw = (int64_t)p.H * p.W;
  if (gid >= (int64_t)p.B * hw) return;
  const int b = (int)(gid / hw);
  const int64_t rem = gid - (int64_t)b * hw;
  const int i = (int)(rem / p.W), j = (int)(rem - (int64_t)i * p.W);
  const int64_t plane = 3 * (int64_t)b * hw + rem;            // channel c of this pixel: plane + c * hw
  if (p.mask_syn) p.mask_syn[gid] = p.zbuf[gid] > 0.0f ? 1.0f : 0.0f;
  if (p.image_syn) {
    for (int c = 0; c < 3; ++c) {
      float v = 0.0f;
      if (p.rgb) {
        v = p.rgb[3 * gid + c];
        if (p.quantize) v = quant8(v);
      }
      p.image_syn[plane + c * hw] = v;
    }
  }
  if (p.nocs_pred) {
    float o[3];
    if (p.quantize) smooth_geo_pixel<true>(p.nocs + 3 * (int64_t)b * hw, p.H, p.W, i, j, o);
    else smooth_geo_pixel<false>(p.nocs + 3 * (int64_t)b * hw, p.H, p.W, i, j, o);
    for (int c = 0; c < 3; ++c) p.nocs_pred[plane + c * hw] = o[c];
  }
  if (p.normal_pred) {
    float o[3];
    smooth_geo_pixel<false>(p.normal + 3 * (int64_t)b * hw, p.H, p.W, i, j, o);
    for (int c = 0; c < 3; ++c) p.normal_pred[plane + c * hw] = o[c];
  }
}

}  // namespace

extern "C" int tp_surfel_finish(const tp_surfel_finish_args* a, tp_stream_t stream) {
  TP_REQUIRE(a, "null pointer");
  TP_REQUIRE(a->B > 0 && a->B <= 65535 && a->H > 0 && a->W > 0 && a->H <= 16384 && a->W <= 16384, "bad sizes");
  TP_REQUIRE(a->zbuf, "null pointer (zbuf)");
  TP_REQUIRE(a->nocs_pred == nullptr || a->nocs != nullptr, "nocs_pred requested without a nocs input");
  TP_REQUIRE(a->normal_pred == nullptr || a->normal != nullptr, "normal_pred requested without a normal input");
  FinishParams p;
  p.rgb = a->rgb; p.nocs = a->nocs; p.normal = a->normal; p.zbuf = a->zbuf;
  p.B = a->B; p.H = a->H; p.W = a->W; p.quantize = a->quantize;
  p.image_syn = a->image_syn; p.mask_syn = a->mask_syn; p.nocs_pred = a->nocs_pred; p.normal_pred = a->normal_pred;
  const int64_t np = (int64_t)a->B * a->H * a->W;
  TP_REQUIRE(np <= (int64_t)INT32_MAX, "bad sizes (more than 2^31 - 1 pixels)");
  hipLaunchKernelGGL(surfel_finish_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
  return tp::check_launch("tp_surfel_finish");
}
