// K31b tp_silhouette_align_step: one step of batched silhouette alignment, B poses against the outline of a mask (DESIGN section 21;
// the public functions are in texpose_amd/silhouette.py, the rules in include/texpose_amd.h).
//
//   sil_reduce grid (ceil(H * W / 1024), B) x 256.  A thread owns four consecutive flat pixels.  Every pixel reads its rendered depth
//              and the measured field once: they decide "covered" and "inside", whose ballots give the image's intersection and
//              union counts.  A covered interior pixel then reads the depth of its four neighbours (the rows above and below are the
//              neighbouring threads' own lines in the cache); only a rim pixel, a few per row, goes on to the mask byte, the field's
//              four neighbours and the one row of the 6-parameter system.  The intrinsics and the frame index are wave-uniform.
//   sil_counts grid B x 64.  Adds the image's per-tile counts as integers.
// The rest is pose_gn.h's, shared with K28 .. K30: the workgroup's 29 fp64 sums become one record (gn_block_reduce, entries 0 .. 28;
// the two counts ride in the record's free entries 29 and 30), and gn_solve_kernel (grid B x 64) gathers an image's records, factors,
// steps and writes the outputs.  No atomics; every fp64 sum has one fixed order, the counts are integers.
#include "tp_common.h"
#include "pose_gn.h"
#include "pose_terms.h"

namespace {
constexpr int kSilInter = 29, kSilUnion = 30;          // the record's entries of the two counts (exact: at most 1024 each)

__device__ __forceinline__ bool covered(float z) { return z > 0.f && isfinite(z); }

__global__ __launch_bounds__(kGnBlock) void sil_reduce_kernel(tp_silhouette_align_args a, double* part) {
  __shared__ double wave_part[kGnWaves][kGnPart];
  __shared__ int wave_count[kGnWaves][2];
  const int b = blockIdx.y;
  const int fr = gn_frame_of(a, b);
  const int64_t plane = (int64_t)a.H * a.W;
  const float* pz = a.zbuf + (int64_t)b * plane;
  const float* pd = a.sdf + (int64_t)fr * plane;
  const uint8_t* pm = a.mask ? a.mask + (int64_t)fr * plane : nullptr;
  const float* K = a.intr + (int64_t)b * 9;
  const double fx = (double)K[0], cx = (double)K[2], fy = (double)K[4], cy = (double)K[5];
  const double tau = (double)a.tau_px;

  const int64_t p0 = (int64_t)blockIdx.x * kGnTile + (int)threadIdx.x * kGnPix;            // (< H * W + 1024 < 2^31 + 1024)
  float zs[kGnPix], ds[kGnPix];
  int n_inter = 0, n_union = 0;                                                  // the wave's counts, the same in every lane
#pragma unroll
  for (int k = 0; k < kGnPix; ++k) {
    const bool in_plane = p0 + k < plane;
    zs[k] = in_plane ? pz[p0 + k] : -1.f;
    ds[k] = in_plane ? pd[p0 + k] : 1.f;
    const bool cov = covered(zs[k]), inside = ds[k] < 0.f && isfinite(ds[k]);
    n_inter += __popcll(__ballot(cov && inside));
    n_union += __popcll(__ballot(cov || inside));
  }

  double s[kGnSums];
#pragma unroll
  for (int k = 0; k < kGnSums; ++k) s[k] = 0.0;
  bool any = false;
  const int i0 = (int)((uint32_t)p0 / (uint32_t)a.W), j0 = (int)((uint32_t)p0 - (uint32_t)i0 * (uint32_t)a.W);
  int pi = i0, pj = j0 - 1;                                                      // row and column of pixel k (a pixel past the plane has i >= H)
#pragma unroll
  for (int k = 0; k < kGnPix; ++k) {
    if (++pj == a.W) { pj = 0; ++pi; }
    if (!(pi >= 1 && pi <= a.H - 2 && pj >= 1 && pj <= a.W - 2 && covered(zs[k]))) continue;
    const int64_t p = p0 + k;                                                    // (interior: p - W >= 0, p + W < plane, p -+ 1 in its row)
    const bool rim = !(covered(pz[p - 1]) && covered(pz[p + 1]) && covered(pz[p - a.W]) && covered(pz[p + a.W]));
    if (!rim) continue;
    if (pm && pm[p] == 0) continue;
    const float lf = pd[p - 1], rt = pd[p + 1], up = pd[p - a.W], dn = pd[p + a.W];
    if (!(isfinite(ds[k]) && isfinite(lf) && isfinite(rt) && isfinite(up) && isfinite(dn))) continue;
    const double r = (double)ds[k] + 0.5;
    if (!(fabs(r) <= tau)) continue;
    const double z = (double)zs[k];
    const double rx = (((double)pj + 0.5) - cx) / fx, ry = (((double)pi + 0.5) - cy) / fy;
    const V3 P = {z * rx, z * ry, z};
    const double gx = 0.5 * ((double)rt - (double)lf), gy = 0.5 * ((double)dn - (double)up);
    const double gfx = gx * fx, gfy = gy * fy;
    const V3 av = {gfx / z, gfy / z, -(gfx * rx + gfy * ry) / z};
    const V3 pa = cross(P, av);
    const double J[6] = {pa.x, pa.y, pa.z, av.x, av.y, av.z};
    gn_add_row(s, J, r);
    s[28] += 1.0;
    any = true;
  }

  const int lane = threadIdx.x & (tp::kWave - 1), wave = threadIdx.x / tp::kWave;
  if (lane == 0) { wave_count[wave][0] = n_inter; wave_count[wave][1] = n_union; }
  double* record = part + ((int64_t)b * gridDim.x + blockIdx.x) * kGnPart;
  gn_block_reduce(s, any, wave_part, record);                                    // (its barrier also orders wave_count)
  if (threadIdx.x == kSilInter || threadIdx.x == kSilUnion) {
    const int c = threadIdx.x - kSilInter;
    int t = 0;
#pragma unroll
    for (int w = 0; w < kGnWaves; ++w) t += wave_count[w][c];
    record[threadIdx.x] = (double)t;
  }
}

// grid B, one wave: the image's G records' counts, added as integers
__global__ __launch_bounds__(tp::kWave) void sil_counts_kernel(tp_silhouette_align_args a, const double* part, int G) {
  const int b = blockIdx.x;
  const double* rec = part + (int64_t)b * G * kGnPart;
  int n_inter = 0, n_union = 0;
  for (int g = threadIdx.x; g < G; g += tp::kWave) {
    n_inter += (int)rec[(int64_t)g * kGnPart + kSilInter];
    n_union += (int)rec[(int64_t)g * kGnPart + kSilUnion];
  }
#pragma unroll
  for (int m = 1; m < tp::kWave; m <<= 1) {
    n_inter += __shfl_xor(n_inter, m);
    n_union += __shfl_xor(n_union, m);
  }
  if (threadIdx.x == 0) { a.inter[b] = n_inter; a.uni[b] = n_union; }
}
}  // namespace

extern "C" size_t tp_silhouette_align_workspace_bytes(int B, int H, int W) { return tp::term_workspace_bytes(B, H, W); }

bool tp::silhouette_align_args_ok(const tp_silhouette_align_args& a) {
  if (a.B <= 0 || a.B > 65535 || a.H <= 0 || a.W <= 0 || a.Ft <= 0 || (int64_t)a.H * a.W > 0x7FFFFFFFll) {
    tp::set_error("tp_silhouette_align_step: bad sizes (B 1..65535, Ft > 0, H > 0, W > 0, H * W < 2^31)");
    return false;
  }
  const bool missing = !a.zbuf || !a.sdf || !a.inter || !a.uni;
  return gn_step_args_ok("tp_silhouette_align_step", a, "tau_px", a.tau_px, missing);
}

void tp::silhouette_align_launch(const tp_silhouette_align_args& a, hipStream_t st) {
  const int G = (int)gn_tiles((int64_t)a.H * a.W);
  double* part = static_cast<double*>(a.workspace);
  hipLaunchKernelGGL(sil_reduce_kernel, dim3(G, a.B), dim3(kGnBlock), 0, st, a, part);
  hipLaunchKernelGGL(gn_solve_kernel<tp_silhouette_align_args>, dim3(a.B), dim3(tp::kWave), 0, st, a, (const double*)part, G);
  hipLaunchKernelGGL(sil_counts_kernel, dim3(a.B), dim3(tp::kWave), 0, st, a, (const double*)part, G);
}

extern "C" int tp_silhouette_align_step(const tp_silhouette_align_args* a, tp_stream_t stream) {
  return tp::term_step("tp_silhouette_align_step", a, tp::silhouette_align_args_ok, tp::silhouette_align_launch, stream);
}
