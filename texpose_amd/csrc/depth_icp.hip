// K29 tp_depth_icp_step: one step of batched projective point-to-plane ICP against measured depth (the public
// functions are in texpose_amd/icp.py, the rules in include/texpose_amd.h).
//
//   icp_reduce   grid (ceil(H * W / 1024), B) x 256.  A thread owns four consecutive flat pixels: one 16-byte load of the rendered
//                depth and one of the measured depth where the planes allow it, else guarded 4-byte loads.  A pixel without a rendered
//                surface or without a measurement leaves before anything else is read (most of a frame is background); the others read
//                their mask byte, their face index, the face's three vertex indices and the vertices.  The pose and the intrinsics of the
//                image are wave-uniform and are read before the kernel's only global store, so they come through scalar loads.  Each
//                kept pixel gives one row of the 6-parameter system.
// The rest is pose_gn.h's, shared with K28 and K30: the workgroup's 29 fp64 sums become one record (gn_block_reduce), and
// gn_solve_kernel (grid B x 64) gathers an image's records, factors, steps and writes the outputs.
// No atomics; every fp64 sum has one fixed order, so all outputs are a function of the inputs alone.
#include "tp_common.h"
#include "pose_gn.h"
#include "pose_terms.h"

namespace {
// VEC: H * W is a multiple of four and zbuf / depth are 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kGnBlock) void icp_reduce_kernel(tp_depth_icp_args a, double* part) {
  __shared__ double wave_part[kGnWaves][kGnPart];
  const int b = blockIdx.y;
  const int fr = gn_frame_of(a, b);
  const int64_t plane = (int64_t)a.H * a.W;
  const float* pz = a.zbuf + (int64_t)b * plane;
  const int32_t* pf = a.face + (int64_t)b * plane;
  const float* pd = a.depth + (int64_t)fr * plane;
  const uint8_t* pm = a.mask ? a.mask + (int64_t)fr * plane : nullptr;
  const float* K = a.intr + (int64_t)b * 9;
  const float* T = a.pose + (int64_t)b * 12;
  const double fx = (double)K[0], cx = (double)K[2], fy = (double)K[4], cy = (double)K[5];
  double R[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) { R[3 * r] = (double)T[4 * r]; R[3 * r + 1] = (double)T[4 * r + 1]; R[3 * r + 2] = (double)T[4 * r + 2]; }
  const double tau2 = (double)a.tau_mm * (double)a.tau_mm;

  const int64_t p0 = (int64_t)blockIdx.x * kGnTile + (int)threadIdx.x * kGnPix;          // (< H * W + 1024 < 2^31 + 1024)
  float zs[kGnPix], ds[kGnPix];
#pragma unroll
  for (int k = 0; k < kGnPix; ++k) { zs[k] = -1.f; ds[k] = 0.f; }
  if constexpr (VEC) {
    if (p0 < plane) {                                                            // (plane % 4 == 0: the four are inside together)
      const float4 z4 = *reinterpret_cast<const float4*>(pz + p0), d4 = *reinterpret_cast<const float4*>(pd + p0);
      zs[0] = z4.x; zs[1] = z4.y; zs[2] = z4.z; zs[3] = z4.w;
      ds[0] = d4.x; ds[1] = d4.y; ds[2] = d4.z; ds[3] = d4.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kGnPix; ++k)
      if (p0 + k < plane) { zs[k] = pz[p0 + k]; ds[k] = pd[p0 + k]; }
  }

  double s[kGnSums];
#pragma unroll
  for (int k = 0; k < kGnSums; ++k) s[k] = 0.0;
  bool any = false;
#pragma unroll
  for (int k = 0; k < kGnPix; ++k) {
    const float zf = zs[k], df = ds[k];
    if (!(zf > 0.f) || !isfinite(zf) || !(df > 0.f) || !isfinite(df)) continue;            // steps 1 and 3: nothing else was read
    const int64_t p = p0 + k;                                                    // (< plane: the others kept -1 / 0)
    if (pm && pm[p] == 0) continue;
    const int f = pf[p];
    if (f < 0 || f >= a.F) continue;
    const int i0 = a.faces[(int64_t)f * 3], i1 = a.faces[(int64_t)f * 3 + 1], i2 = a.faces[(int64_t)f * 3 + 2];
    if (i0 < 0 || i0 >= a.V || i1 < 0 || i1 >= a.V || i2 < 0 || i2 >= a.V) continue;
    const int i = (int)(p / a.W), j = (int)(p - (int64_t)i * a.W);
    const double z = (double)zf, d = (double)df;
    const double rx = (((double)j + 0.5) - cx) / fx, ry = (((double)i + 0.5) - cy) / fy;
    const double q = (rx * rx + ry * ry) + 1.0;
    const double dz = d - z;
    if (!((dz * dz) * q <= tau2)) continue;
    const float* w0 = a.verts + (int64_t)i0 * 3;
    const float* w1 = a.verts + (int64_t)i1 * 3;
    const float* w2 = a.verts + (int64_t)i2 * 3;
    const V3 v0 = {(double)w0[0], (double)w0[1], (double)w0[2]};
    const V3 c = cross(V3{(double)w1[0], (double)w1[1], (double)w1[2]} - v0, V3{(double)w2[0], (double)w2[1], (double)w2[2]} - v0);
    const V3 m = {(R[0] * c.x + R[1] * c.y) + R[2] * c.z, (R[3] * c.x + R[4] * c.y) + R[5] * c.z, (R[6] * c.x + R[7] * c.y) + R[8] * c.z};
    const double mm = dot(m, m);
    if (!isfinite(mm) || !(mm > 0.0)) continue;
    V3 n = scaled(m, 1.0 / sqrt(mm));
    if ((n.x * rx + n.y * ry) + n.z > 0.0) n = {-n.x, -n.y, -n.z};
    const V3 P = {z * rx, z * ry, z}, Q = {d * rx, d * ry, d};
    const double res = dot(n, P - Q);
    const V3 pn = cross(P, n);
    const double J[6] = {pn.x, pn.y, pn.z, n.x, n.y, n.z};
    gn_add_row(s, J, res);
    s[28] += 1.0;
    any = true;
  }

  gn_block_reduce(s, any, wave_part, part + ((int64_t)b * gridDim.x + blockIdx.x) * kGnPart);
}
}  // namespace

extern "C" size_t tp_depth_icp_workspace_bytes(int B, int H, int W) { return tp::term_workspace_bytes(B, H, W); }

bool tp::depth_icp_args_ok(const tp_depth_icp_args& a) {
  if (a.B <= 0 || a.B > 65535 || a.H <= 0 || a.W <= 0 || a.Ft <= 0 || a.V <= 0 || a.F <= 0 || (int64_t)a.H * a.W > 0x7FFFFFFFll) {
    tp::set_error("tp_depth_icp_step: bad sizes (B 1..65535, Ft > 0, V > 0, F > 0, H > 0, W > 0, H * W < 2^31)");
    return false;
  }
  const bool missing = !a.verts || !a.faces || !a.zbuf || !a.face || !a.depth;
  return gn_step_args_ok("tp_depth_icp_step", a, "tau_mm", a.tau_mm, missing);
}

void tp::depth_icp_launch(const tp_depth_icp_args& a, hipStream_t st) {
  const int64_t plane = (int64_t)a.H * a.W;
  const int G = (int)gn_tiles(plane);
  double* part = static_cast<double*>(a.workspace);
  const bool vec = plane % kGnPix == 0 && (((uintptr_t)a.zbuf | (uintptr_t)a.depth) & 15u) == 0;
  if (vec) hipLaunchKernelGGL(icp_reduce_kernel<true>, dim3(G, a.B), dim3(kGnBlock), 0, st, a, part);
  else hipLaunchKernelGGL(icp_reduce_kernel<false>, dim3(G, a.B), dim3(kGnBlock), 0, st, a, part);
  hipLaunchKernelGGL(gn_solve_kernel<tp_depth_icp_args>, dim3(a.B), dim3(tp::kWave), 0, st, a, (const double*)part, G);
}

extern "C" int tp_depth_icp_step(const tp_depth_icp_args* a, tp_stream_t stream) {
  return tp::term_step("tp_depth_icp_step", a, tp::depth_icp_args_ok, tp::depth_icp_launch, stream);
}
