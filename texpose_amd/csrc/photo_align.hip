// K30 tp_photo_align_step: one step of batched photometric alignment, B poses against a photograph (the public
// functions are in texpose_amd/photo_align.py, the rules in include/texpose_amd.h).
//
//   photo_reduce grid (ceil(H * W / 1024), B) x 256.  A thread owns four consecutive flat pixels: one 16-byte load of the rendered
//                depth where the plane allows it, else guarded 4-byte loads.  A pixel on the image's border or without a rendered
//                surface leaves before anything else is read (most of a frame is background); a thread with a pixel left reads the
//                12 rendered and the 12 photographed colour values of its four pixels as three 16-byte loads each (guarded 4-byte
//                loads of the pixels left where the planes do not allow it), then per pixel the mask byte and the photograph's four
//                neighbours: the left and right ones of a thread's inner pixels are already in its registers, the rows above and
//                below are the neighbouring threads' own lines in the cache.  The intrinsics and the frame index are wave-uniform
//                and are read before the kernel's only global store, so they come through scalar loads; the pose is not needed.
//                Each kept pixel gives three rows (one per channel) of the 6-parameter system.
// The rest is pose_gn.h's, shared with K28 and K29: the workgroup's 29 fp64 sums become one record (gn_block_reduce), and
// gn_solve_kernel (grid B x 64) gathers an image's records, factors, steps and writes the outputs.
// No atomics; every fp64 sum has one fixed order, so all outputs are a function of the inputs alone.
#include "tp_common.h"
#include "pose_gn.h"
#include "pose_terms.h"

namespace {
__device__ __forceinline__ bool finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// VEC: H * W is a multiple of four and zbuf / rgb / image are 16-byte aligned.  Three waves per SIMD (at most 168 VGPRs) is what the
// guarded path was tuned to; asked for here, since left to itself the allocator takes 174 once the rows go through gn_add_row (the
// vector path fits either way and is left alone)
template <bool VEC>
__global__ __launch_bounds__(kGnBlock, VEC ? 1 : 3) void photo_reduce_kernel(tp_photo_align_args a, double* part) {
  __shared__ double wave_part[kGnWaves][kGnPart];
  const int b = blockIdx.y;
  const int fr = gn_frame_of(a, b);
  const int64_t plane = (int64_t)a.H * a.W;
  const float* pz = a.zbuf + (int64_t)b * plane;
  const float* pc = a.rgb + (int64_t)b * plane * 3;
  const float* po = a.image + (int64_t)fr * plane * 3;
  const uint8_t* pm = a.mask ? a.mask + (int64_t)fr * plane : nullptr;
  const float* K = a.intr + (int64_t)b * 9;
  const double fx = (double)K[0], cx = (double)K[2], fy = (double)K[4], cy = (double)K[5];
  const double tau2 = (double)a.tau * (double)a.tau;

  const int64_t p0 = (int64_t)blockIdx.x * kGnTile + (int)threadIdx.x * kGnPix;            // (< H * W + 1024 < 2^31 + 1024)
  float zs[kGnPix];
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

  // steps 1 and 2: the interior pixels with a rendered surface (a pixel past the plane has i >= H)
  const int i0 = (int)((uint32_t)p0 / (uint32_t)a.W), j0 = (int)((uint32_t)p0 - (uint32_t)i0 * (uint32_t)a.W);
  unsigned cand = 0u;                                                            // bit k: pixel k is a candidate
  {
    int i = i0, j = j0;
#pragma unroll
    for (int k = 0; k < kGnPix; ++k) {
      if (i >= 1 && i <= a.H - 2 && j >= 1 && j <= a.W - 2 && zs[k] > 0.f && isfinite(zs[k])) cand |= 1u << k;
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

  double s[kGnSums];
#pragma unroll
  for (int k = 0; k < kGnSums; ++k) s[k] = 0.0;
  bool any = false;
  int pi = i0, pj = j0 - 1;                                                      // row and column of pixel k, walked as above
#pragma unroll
  for (int k = 0; k < kGnPix; ++k) {
    if (++pj == a.W) { pj = 0; ++pi; }
    if (!(cand >> k & 1u)) continue;
    const int64_t p = p0 + k;                                                    // (interior: p - W >= 0, p + W < plane, p -+ 1 in its row)
    if (pm && pm[p] == 0) continue;
    float lf[3], rt[3], up[3], dn[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if (VEC && k > 0) lf[ch] = os[3 * (k - 1) + ch]; else lf[ch] = po[(p - 1) * 3 + ch];
      if (VEC && k < kGnPix - 1) rt[ch] = os[3 * (k + 1) + ch]; else rt[ch] = po[(p + 1) * 3 + ch];
      up[ch] = po[(p - a.W) * 3 + ch];
      dn[ch] = po[(p + a.W) * 3 + ch];
    }
    if (!(finite3(cs + 3 * k) && finite3(os + 3 * k) && finite3(lf) && finite3(rt) && finite3(up) && finite3(dn))) continue;
    double res[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) res[ch] = (double)os[3 * k + ch] - (double)cs[3 * k + ch];
    if (!((res[0] * res[0] + res[1] * res[1]) + res[2] * res[2] <= tau2)) continue;
    const double z = (double)zs[k];
    const double rx = (((double)pj + 0.5) - cx) / fx, ry = (((double)pi + 0.5) - cy) / fy;
    const V3 P = {z * rx, z * ry, z};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const double gx = 0.5 * ((double)rt[ch] - (double)lf[ch]), gy = 0.5 * ((double)dn[ch] - (double)up[ch]);
      const double gfx = gx * fx, gfy = gy * fy;
      const V3 av = {gfx / z, gfy / z, -(gfx * rx + gfy * ry) / z};
      const V3 pa = cross(P, av);
      const double J[6] = {pa.x, pa.y, pa.z, av.x, av.y, av.z};
      gn_add_row(s, J, res[ch]);
    }
    s[28] += 1.0;
    any = true;
  }

  gn_block_reduce(s, any, wave_part, part + ((int64_t)b * gridDim.x + blockIdx.x) * kGnPart);
}
}  // namespace

extern "C" size_t tp_photo_align_workspace_bytes(int B, int H, int W) { return tp::term_workspace_bytes(B, H, W); }

bool tp::photo_align_args_ok(const tp_photo_align_args& a) {
  if (a.B <= 0 || a.B > 65535 || a.H <= 0 || a.W <= 0 || a.Ft <= 0 || (int64_t)a.H * a.W > 0x7FFFFFFFll) {
    tp::set_error("tp_photo_align_step: bad sizes (B 1..65535, Ft > 0, H > 0, W > 0, H * W < 2^31)");
    return false;
  }
  const bool missing = !a.zbuf || !a.rgb || !a.image;
  return gn_step_args_ok("tp_photo_align_step", a, "tau", a.tau, missing);
}

void tp::photo_align_launch(const tp_photo_align_args& a, hipStream_t st) {
  const int64_t plane = (int64_t)a.H * a.W;
  const int G = (int)gn_tiles(plane);
  double* part = static_cast<double*>(a.workspace);
  const bool vec = plane % kGnPix == 0 && (((uintptr_t)a.zbuf | (uintptr_t)a.rgb | (uintptr_t)a.image) & 15u) == 0;
  if (vec) hipLaunchKernelGGL(photo_reduce_kernel<true>, dim3(G, a.B), dim3(kGnBlock), 0, st, a, part);
  else hipLaunchKernelGGL(photo_reduce_kernel<false>, dim3(G, a.B), dim3(kGnBlock), 0, st, a, part);
  hipLaunchKernelGGL(gn_solve_kernel<tp_photo_align_args>, dim3(a.B), dim3(tp::kWave), 0, st, a, (const double*)part, G);
}

extern "C" int tp_photo_align_step(const tp_photo_align_args* a, tp_stream_t stream) {
  return tp::term_step("tp_photo_align_step", a, tp::photo_align_args_ok, tp::photo_align_launch, stream);
}
