// K29 tp_depth_icp_step: one step of batched projective point-to-plane ICP against measured depth (the public
// functions are in texpose_amd/icp.py, the rules in include/texpose_amd.h).
//
//   icp_reduce   grid (ceil(H * W / 1024), B) x 256.  A thread owns four consecutive flat pixels: one 16-byte load of the rendered
//                depth and one of the measured depth where the planes allow it, else guarded 4-byte loads.  A pixel without a rendered
//                surface or without a measurement leaves before anything else is read (most of a frame is background); the others read
//                their mask byte, their face index, the face's three vertex indices and the vertices.  The pose and the intrinsics of the
//                image are wave-uniform and are read before the kernel's only global store, so they come through scalar loads.  The 29
//                fp64 sums of a thread are reduced in pnp_reduce's order: xor-butterfly inside the wave (step-major: the 29 exchanges
//                of a step are in flight together), the four waves in ascending order through LDS, one 32-double record per workgroup.
//                A wave none of whose pixels is kept skips its butterflies: its sums are 29 zeros either way.
//   icp_solve    grid B x 64.  The records come through LDS 64 at a time (coalesced, 32 loads in flight per thread), 29 threads add them
//                in ascending tile order, thread 0 factors, steps (pose_gn.h, shared with K28) and writes the outputs.
// No atomics; every fp64 sum has one fixed order, so all outputs are a function of the inputs alone.
#include "tp_common.h"
#include "pose_gn.h"

namespace {
constexpr int kIcpBlock = 256, kIcpPix = 4, kIcpTile = kIcpBlock * kIcpPix, kIcpWaves = kIcpBlock / tp::kWave;
constexpr int kIcpMinCount = 6;
constexpr int kIcpStage = 64;                         // records the solve kernel stages through LDS at a time

__host__ __device__ inline int64_t icp_tiles(int64_t n) { return (n + kIcpTile - 1) / kIcpTile; }

// VEC: H * W is a multiple of four and zbuf / depth are 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(kIcpBlock) void icp_reduce_kernel(tp_depth_icp_args a, double* part) {
  __shared__ double wave_part[kIcpWaves][kGnPart];
  const int b = blockIdx.y;
  int fr = a.Ft == 1 ? 0 : b;
  if (a.frame) {                                                                 // out of range is the caller's error: clamped, never read past
    fr = a.frame[b];
    fr = fr < 0 ? 0 : (fr >= a.Ft ? a.Ft - 1 : fr);
  }
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

  const int64_t p0 = (int64_t)blockIdx.x * kIcpTile + (int)threadIdx.x * kIcpPix;          // (< H * W + 1024 < 2^31 + 1024)
  float zs[kIcpPix], ds[kIcpPix];
#pragma unroll
  for (int k = 0; k < kIcpPix; ++k) { zs[k] = -1.f; ds[k] = 0.f; }
  if constexpr (VEC) {
    if (p0 < plane) {                                                            // (plane % 4 == 0: the four are inside together)
      const float4 z4 = *reinterpret_cast<const float4*>(pz + p0), d4 = *reinterpret_cast<const float4*>(pd + p0);
      zs[0] = z4.x; zs[1] = z4.y; zs[2] = z4.z; zs[3] = z4.w;
      ds[0] = d4.x; ds[1] = d4.y; ds[2] = d4.z; ds[3] = d4.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kIcpPix; ++k)
      if (p0 + k < plane) { zs[k] = pz[p0 + k]; ds[k] = pd[p0 + k]; }
  }

  double s[kGnSums];
#pragma unroll
  for (int k = 0; k < kGnSums; ++k) s[k] = 0.0;
  bool any = false;
#pragma unroll
  for (int k = 0; k < kIcpPix; ++k) {
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
    int e = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int cc = r; cc < 6; ++cc) s[e++] += J[r] * J[cc];
#pragma unroll
    for (int r = 0; r < 6; ++r) s[21 + r] += J[r] * res;
    s[27] += res * res;
    s[28] += 1.0;
    any = true;
  }

  const int lane = threadIdx.x & (tp::kWave - 1), wave = threadIdx.x / tp::kWave;
  if (__ballot(any) != 0ull) {                                                   // (uniform per wave)
    wave_sum_all(s);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < kGnSums; ++k) wave_part[wave][k] = s[k];
    }
  } else if (lane < kGnSums) {
    wave_part[wave][lane] = 0.0;                                                 // what the butterflies of 64 zeros give
  }
  __syncthreads();
  if (threadIdx.x < kGnSums) {
    double t = wave_part[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kIcpWaves; ++w) t += wave_part[w][threadIdx.x];
    part[((int64_t)b * gridDim.x + blockIdx.x) * kGnPart + threadIdx.x] = t;
  }
}

// grid B, one wave
__global__ __launch_bounds__(tp::kWave) void icp_solve_kernel(tp_depth_icp_args a, const double* part, int G) {
  __shared__ double sum[kGnPart], stage[kIcpStage][kGnPart];
  const int b = blockIdx.x;
  const double* rec = part + (int64_t)b * G * kGnPart;
  double t = 0.0;
  for (int g0 = 0; g0 < G; g0 += kIcpStage) {                                    // 64 records in flight as whole 512-byte rows
    const int n = G - g0 < kIcpStage ? G - g0 : kIcpStage;
    double v[kIcpStage / 2];
#pragma unroll
    for (int u = 0; u < kIcpStage / 2; ++u) {
      const int e = (int)threadIdx.x + tp::kWave * u;                            // element e of the batch: record e / 32, entry e % 32
      v[u] = e / kGnPart < n ? rec[(int64_t)g0 * kGnPart + e] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kIcpStage / 2; ++u) (&stage[0][0])[(int)threadIdx.x + tp::kWave * u] = v[u];
    __syncthreads();
    if (threadIdx.x < kGnSums)
      for (int g = 0; g < n; ++g) t += stage[g][threadIdx.x];                    // ascending tile order
    __syncthreads();
  }
  if (threadIdx.x < kGnSums) sum[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float* T = a.pose + (int64_t)b * 12;
  const double count = sum[28];
  int status = 0;
  double Pn[12];
  if (count < (double)kIcpMinCount) {
    status = 1;
  } else if (a.evaluate_only) {
    double A[6][6];
    gn_matrix(sum, A);
    if (!cholesky6(A, kGnPivotTol)) status = 3;
  } else {
    double cur[12];
    for (int k = 0; k < 12; ++k) cur[k] = (double)T[k];
    bool ok = gn_step(sum, cur, (double)a.damping, Pn);
    for (int k = 0; k < 12; ++k) ok = ok && isfinite((float)Pn[k]);
    if (!ok) status = 3;
  }
  a.inliers[b] = (int)count;
  a.rms[b] = count > 0.0 ? (float)sqrt(sum[27] / count) : __int_as_float(0x7fc00000);
  a.status[b] = status;
  if (a.pose_out) {
    const bool stepped = status == 0 && !a.evaluate_only;
    for (int k = 0; k < 12; ++k) a.pose_out[(int64_t)b * 12 + k] = stepped ? (float)Pn[k] : T[k];
  }
}
}  // namespace

extern "C" size_t tp_depth_icp_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const size_t bytes = (size_t)B * (size_t)icp_tiles((int64_t)H * W) * kGnPart * sizeof(double);
  return (bytes + 15) & ~(size_t)15;
}

extern "C" int tp_depth_icp_step(const tp_depth_icp_args* a, tp_stream_t stream) {
  if (!a) { tp::set_error("tp_depth_icp_step: null args"); return -1; }
  if (a->B <= 0 || a->B > 65535 || a->H <= 0 || a->W <= 0 || a->Ft <= 0 || a->V <= 0 || a->F <= 0 || (int64_t)a->H * a->W > 0x7FFFFFFFll) {
    tp::set_error("tp_depth_icp_step: bad sizes (B 1..65535, Ft > 0, V > 0, F > 0, H > 0, W > 0, H * W < 2^31)");
    return -1;
  }
  if (!a->frame && a->Ft != 1 && a->Ft != a->B) {
    tp::set_error("tp_depth_icp_step: Ft = %d is neither 1 nor B = %d and there is no frame map", a->Ft, a->B);
    return -1;
  }
  if (!(a->tau_mm > 0.f) || !isfinite(a->tau_mm)) { tp::set_error("tp_depth_icp_step: tau_mm must be finite and positive"); return -1; }
  if (!(a->damping >= 0.f) || !isfinite(a->damping)) { tp::set_error("tp_depth_icp_step: damping must be finite and not negative"); return -1; }
  if (!a->verts || !a->faces || !a->zbuf || !a->face || !a->pose || !a->intr || !a->depth || !a->inliers || !a->rms || !a->status || !a->workspace ||
      (!a->pose_out && !a->evaluate_only)) {
    tp::set_error("tp_depth_icp_step: null pointer");
    return -1;
  }
  if ((uintptr_t)a->workspace & 15u) { tp::set_error("tp_depth_icp_step: workspace must be 16-byte aligned"); return -1; }
  if (a->pose_out) {
    const uintptr_t in = (uintptr_t)a->pose, out = (uintptr_t)a->pose_out, bytes = (uintptr_t)a->B * 12 * sizeof(float);
    if (in < out + bytes && out < in + bytes) { tp::set_error("tp_depth_icp_step: pose_out must not overlap pose"); return -1; }
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t plane = (int64_t)a->H * a->W;
  const int G = (int)icp_tiles(plane);
  double* part = static_cast<double*>(a->workspace);
  const bool vec = plane % kIcpPix == 0 && (((uintptr_t)a->zbuf | (uintptr_t)a->depth) & 15u) == 0;
  if (vec) hipLaunchKernelGGL(icp_reduce_kernel<true>, dim3(G, a->B), dim3(kIcpBlock), 0, st, *a, part);
  else hipLaunchKernelGGL(icp_reduce_kernel<false>, dim3(G, a->B), dim3(kIcpBlock), 0, st, *a, part);
  hipLaunchKernelGGL(icp_solve_kernel, dim3(a->B), dim3(tp::kWave), 0, st, *a, (const double*)part, G);
  return tp::check_launch("tp_depth_icp_step");
}
