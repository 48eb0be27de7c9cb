// K38 tp_image_down / tp_surface_down / tp_mask_down: one level down an image pyramid for the photograph, the rendering and the mask
// of the photometric alignment (the public functions are ops.image_down / surface_down / mask_down in
// texpose_amd/ops/refine.py, the rules in include/texpose_amd.h).
//
//   down_kernel      grid (ceil(h * ceil(w / 2) / 256), N) x 256.  A thread owns the two coarse pixels (I, J0) and (I, J0 + 1), J0 even:
//                    their taps are the six fine columns 2 J0 - 1 .. 2 J0 + 4 of four fine rows, every index clamped.  Per row and
//                    plane it reads the four middle columns as one 16-byte load (depth) or three (colour) where W is a multiple of
//                    four and the planes are 16-byte aligned; the two outer columns are 4-byte loads, except the image's, which are
//                    the neighbour lanes' (a lane exchange; the first and last lane of a wave load theirs, a row's ends clamp onto
//                    the thread's own columns).  Else all six come through guarded 4-byte loads.  In surface mode the 24 depth taps come first: a thread whose two pixels both have a tap
//                    without a surface stores the background and leaves without touching the colours.  The filter runs in fp64 in
//                    the header's order (per tap row the four columns ascending, then the four rows ascending) through the
//                    non-contracting intrinsics, and is rounded to fp32 once.
//   mask_down_kernel grid (ceil(h * w / 256), N) x 256, a thread per coarse pixel, 16 clamped byte loads; where W is a multiple of
//                    eight and the planes are aligned, mask_down4_kernel: a thread per four coarse pixels, per row one 8-byte
//                    load and at most two byte loads, one 4-byte store.
// One launch per call, no atomics, no LDS, no workspace: every output is a function of the inputs alone.
#include "tp_common.h"

namespace {
constexpr int kDownBlock = 256;
constexpr double kW0 = 0.125, kW1 = 0.375;                                       // (1, 3, 3, 1) / 8

__device__ __forceinline__ bool covered(float z) { return z > 0.f && isfinite(z); }
__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

// ((w0 a + w1 b) + w1 c) + w0 d
__device__ __forceinline__ double tap4(double a, double b, double c, double d) {
  return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(kW0, a), __dmul_rn(kW1, b)), __dmul_rn(kW1, c)), __dmul_rn(kW0, d));
}
// the rows' sums: acc after row r is ((w0 s0 + w1 s1) + w1 s2) + w0 s3 up to r
__device__ __forceinline__ double add_row(int r, double acc, double s) {
  const double t = __dmul_rn(r == 0 || r == 3 ? kW0 : kW1, s);
  return r == 0 ? t : __dadd_rn(acc, t);
}

// Where a thread's outer colour columns come from on the image's wide path.  Lanes l - 1 and l + 1 of the wave own the pixel pairs to
// the left and right in the same row, and their 16-byte loads hold this thread's outer columns: they come through a lane exchange.
// At a row's ends the clamp lands on the thread's own first / last column; only the first and the last lane of a wave load theirs.
struct Edge { bool own_left, own_right, load_left, load_right; };
__device__ __forceinline__ Edge edge_of(int jp, int wp) {
  const int lane = threadIdx.x & (tp::kWave - 1);
  Edge e;
  e.own_left = jp == 0; e.own_right = jp == wp - 1;
  e.load_left = !e.own_left && lane == 0; e.load_right = !e.own_right && lane == tp::kWave - 1;
  return e;
}
// the six taps of a row of a one-channel plane: columns col[0 .. 5] = clamp(2 J0 - 1 .. 2 J0 + 4).  The outer columns are 4-byte loads
// on both paths: they sit in the neighbours' cache lines, and the lane exchange measured 9 % slower here.
template <bool VEC>
__device__ __forceinline__ void load_row1(const float* row, int J0, const int (&col)[6], float (&v)[6]) {
  if constexpr (VEC) {                                                           // (W % 4 == 0, J0 even: 2 J0 .. 2 J0 + 3 are inside and aligned)
    const float4 m = *reinterpret_cast<const float4*>(row + 2 * J0);
    v[0] = row[col[0]];
    v[1] = m.x; v[2] = m.y; v[3] = m.z; v[4] = m.w;
    v[5] = row[col[5]];
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = row[col[k]];
  }
}

// the same of a three-channel plane: v[3 k + ch].  EXCHANGE: every lane of the wave that is inside the plane is here (the image: no
// divergence above), so the outer columns come from the neighbour lanes; without it (the surface's colours, which only the threads
// with a surface pixel read) they are 4-byte loads.
template <bool VEC, bool EXCHANGE>
__device__ __forceinline__ void load_row3(const float* row, int J0, const int (&col)[6], const Edge& e, float (&v)[18]) {
  if constexpr (VEC) {                                                           // (6 J0 floats: a multiple of 48 bytes)
    const float4* m4 = reinterpret_cast<const float4*>(row + 6 * J0);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float4 m = m4[q];
      v[3 + 4 * q] = m.x; v[4 + 4 * q] = m.y; v[5 + 4 * q] = m.z; v[6 + 4 * q] = m.w;
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if constexpr (EXCHANGE) {
        const float left = __shfl_up(v[12 + ch], 1), right = __shfl_down(v[3 + ch], 1);
        v[ch] = e.own_left ? v[3 + ch] : e.load_left ? row[3 * col[0] + ch] : left;
        v[15 + ch] = e.own_right ? v[12 + ch] : e.load_right ? row[3 * col[5] + ch] : right;
      } else {
        v[ch] = row[3 * col[0] + ch];
        v[15 + ch] = row[3 * col[5] + ch];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) v[3 * k + ch] = row[3 * col[k] + ch];
  }
}

// VEC: W % 4 == 0 (so w is even and every thread owns two pixels), inputs 16-byte and outputs 8-byte aligned.
// SURFACE: zbuf / rgb -> zbuf_out / rgb_out under the all-16-taps rule; else rgb -> rgb_out, plain.
template <bool VEC, bool SURFACE>
__global__ __launch_bounds__(kDownBlock) void down_kernel(tp_pyramid_down_args a) {
  const int h = a.H >> 1, w = a.W >> 1, wp = (w + 1) >> 1;
  const uint32_t q = blockIdx.x * (uint32_t)kDownBlock + threadIdx.x;            // (h * wp < 2^29)
  if (q >= (uint32_t)h * (uint32_t)wp) return;
  const int I = (int)(q / (uint32_t)wp), jp = (int)(q - (uint32_t)I * (uint32_t)wp), J0 = 2 * jp;
  const Edge e = edge_of(jp, wp);
  const int64_t n = blockIdx.y, plane = (int64_t)a.H * a.W, out0 = n * ((int64_t)h * w) + (int64_t)I * w + J0;
  const bool two = VEC || J0 + 1 < w;
  int col[6], row[4];
#pragma unroll
  for (int k = 0; k < 6; ++k) col[k] = clampi(2 * J0 - 1 + k, a.W - 1);
#pragma unroll
  for (int r = 0; r < 4; ++r) row[r] = clampi(2 * I - 1 + r, a.H - 1);

  bool on0 = true, on1 = true;
  if constexpr (SURFACE) {
    const float* pz = a.zbuf + n * plane;
    double z0 = 0.0, z1 = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v[6];
      load_row1<VEC>(pz + (int64_t)row[r] * a.W, J0, col, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) { on0 = on0 && covered(v[k]); on1 = on1 && covered(v[k + 2]); }
      z0 = add_row(r, z0, tap4(v[0], v[1], v[2], v[3]));
      z1 = add_row(r, z1, tap4(v[2], v[3], v[4], v[5]));
    }
    const float y0 = on0 ? (float)z0 : -1.f, y1 = on1 ? (float)z1 : -1.f;
    if constexpr (VEC) {
      *reinterpret_cast<float2*>(a.zbuf_out + out0) = make_float2(y0, y1);
    } else {
      a.zbuf_out[out0] = y0;
      if (two) a.zbuf_out[out0 + 1] = y1;
    }
  }

  float y[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) y[k] = 0.f;
  if (!SURFACE || on0 || on1) {
    const float* pc = a.rgb + n * plane * 3;
    double acc[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v[18];
      load_row3<VEC, !SURFACE>(pc + (int64_t)row[r] * a.W * 3, J0, col, e, v);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        acc[ch] = add_row(r, acc[ch], tap4(v[ch], v[3 + ch], v[6 + ch], v[9 + ch]));
        acc[3 + ch] = add_row(r, acc[3 + ch], tap4(v[6 + ch], v[9 + ch], v[12 + ch], v[15 + ch]));
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      y[ch] = on0 ? (float)acc[ch] : 0.f;
      y[3 + ch] = on1 ? (float)acc[3 + ch] : 0.f;
    }
  }
  float* po = a.rgb_out + out0 * 3;
  if constexpr (VEC) {                                                           // (out0 is even: 24-byte steps from an 8-byte aligned base)
    float2* p2 = reinterpret_cast<float2*>(po);
    p2[0] = make_float2(y[0], y[1]); p2[1] = make_float2(y[2], y[3]); p2[2] = make_float2(y[4], y[5]);
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k)
      if (k < 3 || two) po[k] = y[k];
  }
}

__global__ __launch_bounds__(kDownBlock) void mask_down_kernel(tp_pyramid_down_args a) {
  const int h = a.H >> 1, w = a.W >> 1;
  const uint32_t q = blockIdx.x * (uint32_t)kDownBlock + threadIdx.x;            // (h * w < 2^29)
  if (q >= (uint32_t)h * (uint32_t)w) return;
  const int I = (int)(q / (uint32_t)w), J = (int)(q - (uint32_t)I * (uint32_t)w);
  const int64_t n = blockIdx.y;
  const uint8_t* pm = a.mask + n * ((int64_t)a.H * a.W);
  bool on = true;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint8_t* prow = pm + (int64_t)clampi(2 * I - 1 + r, a.H - 1) * a.W;
#pragma unroll
    for (int k = 0; k < 4; ++k) on = on && prow[clampi(2 * J - 1 + k, a.W - 1)] != 0;
  }
  a.mask_out[n * ((int64_t)h * w) + q] = on ? 1 : 0;
}

// W % 8 == 0, mask 8-byte and mask_out 4-byte aligned: a thread owns the coarse pixels 4 jq .. 4 jq + 3 of row I, whose taps are the
// fine columns 8 jq - 1 .. 8 jq + 8
__global__ __launch_bounds__(kDownBlock) void mask_down4_kernel(tp_pyramid_down_args a) {
  const int h = a.H >> 1, w = a.W >> 1, wq = w >> 2;
  const uint32_t q = blockIdx.x * (uint32_t)kDownBlock + threadIdx.x;            // (h * wq < 2^27)
  if (q >= (uint32_t)h * (uint32_t)wq) return;
  const int I = (int)(q / (uint32_t)wq), jq = (int)(q - (uint32_t)I * (uint32_t)wq);
  const int64_t n = blockIdx.y;
  const uint8_t* pm = a.mask + n * ((int64_t)a.H * a.W);
  unsigned on = 0xFu;                                                            // bit k: every tap of pixel 4 jq + k so far is non-zero
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint8_t* prow = pm + (int64_t)clampi(2 * I - 1 + r, a.H - 1) * a.W + 8 * jq;
    const uint64_t m = *reinterpret_cast<const uint64_t*>(prow);
    unsigned nz = 0u;                                                            // bit c: fine column 8 jq - 1 + c is non-zero, c = 0 .. 9
#pragma unroll
    for (int c = 0; c < 8; ++c) nz |= ((m >> (8 * c)) & 0xFFull) != 0 ? 2u << c : 0u;
    nz |= (jq == 0 ? (nz >> 1) & 1u : prow[-1] != 0 ? 1u : 0u);                  // (column -1 clamps onto column 0)
    nz |= (jq == wq - 1 ? (nz >> 8) & 1u : prow[8] != 0 ? 1u : 0u) << 9;         // (column W clamps onto column W - 1)
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (((nz >> (2 * k)) & 0xFu) != 0xFu) on &= ~(1u << k);
  }
  const uint32_t packed = (on & 1u) | ((on >> 1) & 1u) << 8 | ((on >> 2) & 1u) << 16 | ((on >> 3) & 1u) << 24;
  *reinterpret_cast<uint32_t*>(a.mask_out + n * ((int64_t)h * w) + (int64_t)I * w + 4 * jq) = packed;
}

bool overlap(const void* x, size_t nx, const void* y, size_t ny) {
  const uintptr_t p = (uintptr_t)x, q = (uintptr_t)y;
  return x && y && p < q + ny && q < p + nx;
}

bool sizes_ok(const char* who, const tp_pyramid_down_args& a) {
  if (a.N <= 0 || a.N > 65535 || a.H < 2 || a.W < 2 || (int64_t)a.H * a.W > 0x7FFFFFFFll) {
    tp::set_error("%s: bad sizes (N 1..65535, H >= 2, W >= 2, H * W < 2^31)", who);
    return false;
  }
  return true;
}

struct Extent { size_t in1, in3, out1, out3; };                                  // elements of a one- / three-channel input / output
Extent extent(const tp_pyramid_down_args& a) {
  const size_t in1 = (size_t)a.N * (size_t)a.H * (size_t)a.W, out1 = (size_t)a.N * (size_t)(a.H / 2) * (size_t)(a.W / 2);
  return {in1, in1 * 3, out1, out1 * 3};
}

int colour_down(const char* who, const tp_pyramid_down_args* a, bool surface, tp_stream_t stream) {
  if (!a) { tp::set_error("%s: null args", who); return -1; }
  if (!sizes_ok(who, *a)) return -1;
  if (!a->rgb || !a->rgb_out || (surface && (!a->zbuf || !a->zbuf_out))) { tp::set_error("%s: null pointer", who); return -1; }
  const Extent e = extent(*a);
  const size_t f = sizeof(float);
  bool bad = overlap(a->rgb_out, e.out3 * f, a->rgb, e.in3 * f);
  if (surface)
    bad = bad || overlap(a->rgb_out, e.out3 * f, a->zbuf, e.in1 * f) || overlap(a->zbuf_out, e.out1 * f, a->rgb, e.in3 * f) ||
          overlap(a->zbuf_out, e.out1 * f, a->zbuf, e.in1 * f) || overlap(a->zbuf_out, e.out1 * f, a->rgb_out, e.out3 * f);
  if (bad) { tp::set_error("%s: an output must not overlap an input or the other output", who); return -1; }
  const int h = a->H / 2, w = a->W / 2;
  const dim3 grid((unsigned)(((int64_t)h * ((w + 1) / 2) + kDownBlock - 1) / kDownBlock), (unsigned)a->N), block(kDownBlock);
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = a->W % 4 == 0 && (((uintptr_t)a->rgb | (surface ? (uintptr_t)a->zbuf : 0)) & 15u) == 0 &&
                   (((uintptr_t)a->rgb_out | (surface ? (uintptr_t)a->zbuf_out : 0)) & 7u) == 0;
  if (surface) {
    if (vec) hipLaunchKernelGGL((down_kernel<true, true>), grid, block, 0, st, *a);
    else hipLaunchKernelGGL((down_kernel<false, true>), grid, block, 0, st, *a);
  } else {
    if (vec) hipLaunchKernelGGL((down_kernel<true, false>), grid, block, 0, st, *a);
    else hipLaunchKernelGGL((down_kernel<false, false>), grid, block, 0, st, *a);
  }
  return tp::check_launch(who);
}
}  // namespace

extern "C" int tp_image_down(const tp_pyramid_down_args* a, tp_stream_t stream) { return colour_down("tp_image_down", a, false, stream); }

extern "C" int tp_surface_down(const tp_pyramid_down_args* a, tp_stream_t stream) { return colour_down("tp_surface_down", a, true, stream); }

extern "C" int tp_mask_down(const tp_pyramid_down_args* a, tp_stream_t stream) {
  const char* who = "tp_mask_down";
  if (!a) { tp::set_error("%s: null args", who); return -1; }
  if (!sizes_ok(who, *a)) return -1;
  if (!a->mask || !a->mask_out) { tp::set_error("%s: null pointer", who); return -1; }
  const Extent e = extent(*a);
  if (overlap(a->mask_out, e.out1, a->mask, e.in1)) { tp::set_error("%s: an output must not overlap an input or the other output", who); return -1; }
  const int h = a->H / 2, w = a->W / 2;
  if (a->W % 8 == 0 && ((uintptr_t)a->mask & 7u) == 0 && ((uintptr_t)a->mask_out & 3u) == 0)
    hipLaunchKernelGGL(mask_down4_kernel, dim3((unsigned)(((int64_t)h * (w / 4) + kDownBlock - 1) / kDownBlock), (unsigned)a->N), dim3(kDownBlock),
                       0, (hipStream_t)stream, *a);
  else
    hipLaunchKernelGGL(mask_down_kernel, dim3((unsigned)(((int64_t)h * w + kDownBlock - 1) / kDownBlock), (unsigned)a->N), dim3(kDownBlock), 0,
                       (hipStream_t)stream, *a);
  return tp::check_launch(who);
}
