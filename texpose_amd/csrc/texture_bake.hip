// K27 tp_texture_bake: project B posed images back onto the V vertices of a mesh as weighted colour sums (the
// public functions are in texpose_amd/texture_bake.py, the rules in include/texpose_amd.h).
//
// A gather: per (vertex, view) pair a 3x4 transform, two rejections that touch no image memory (behind the camera, facing away),
// then up to four taps of the depth plane and, where a tap passes the depth test, of the image (and the weight plane).  Grid
// (vertex tiles, S): a thread owns one vertex and one slice of L consecutive views, so pose[b] and intr[b] are wave-uniform (scalar
// loads) and neighbouring lanes -- neighbouring vertices of the mesh -- gather from neighbouring pixels.  Everything between the
// fp32 inputs and a pair's four products is fp64 in one fixed operation order (the library is built without contraction); the
// thread adds its pairs in ascending b in fp64 and stores four doubles and a count to the workspace.  A second launch adds a
// vertex's S partial sums in ascending order into acc / count.  No atomics anywhere, and S = f(V, B) only: the outputs are a
// function of the inputs alone.  Two launches, no allocation, no host synchronisation.
#include "tp_common.h"

namespace {
constexpr int kBakeBlock = 256, kBakeMinSlice = 4, kBakeThreads = 65536;

// L = max(4, ceil(B / ceil(65536 / V))), at most B: ~65,536 threads (256 per compute unit of the largest part) where B allows it
__host__ __device__ inline int bake_slice_len(int V, int B) {
  const int want = (kBakeThreads + V - 1) / V;
  int L = (B + want - 1) / want;
  L = L < kBakeMinSlice ? kBakeMinSlice : L;
  return L > B ? B : L;
}

struct Sums { double r, g, b, w; int n; };

// one (vertex, view) pair, as the header states it
__device__ __forceinline__ void bake_pair(const tp_texture_bake_args& a, int b, double vx, double vy, double vz, double nx, double ny,
                                          double nz, Sums& s) {
  const float* P = a.pose + (int64_t)b * 12;
  const float* K = a.intr + (int64_t)b * 9;
  const double x = (((double)P[0] * vx + (double)P[1] * vy) + (double)P[2] * vz) + (double)P[3];
  const double y = (((double)P[4] * vx + (double)P[5] * vy) + (double)P[6] * vz) + (double)P[7];
  const double z = (((double)P[8] * vx + (double)P[9] * vy) + (double)P[10] * vz) + (double)P[11];
  if (!(z > 0.0)) return;
  const double rnx = ((double)P[0] * nx + (double)P[1] * ny) + (double)P[2] * nz;
  const double rny = ((double)P[4] * nx + (double)P[5] * ny) + (double)P[6] * nz;
  const double rnz = ((double)P[8] * nx + (double)P[9] * ny) + (double)P[10] * nz;
  const double len = sqrt((x * x + y * y) + z * z);
  const double c = -(((rnx * x + rny * y) + rnz * z) / len);
  if (!(c >= (double)a.cos_min)) return;
  const double q0 = ((double)K[0] * x + (double)K[1] * y) + (double)K[2] * z;
  const double q1 = ((double)K[3] * x + (double)K[4] * y) + (double)K[5] * z;
  const double q2 = ((double)K[6] * x + (double)K[7] * y) + (double)K[8] * z;
  const double su = q0 / q2 - 0.5, sv = q1 / q2 - 0.5;
  if (!(su >= -1.0 && su < (double)a.W && sv >= -1.0 && sv < (double)a.H)) return;       // (a NaN too) no tap inside the image
  const double fj = floor(su), fr = floor(sv);
  const int j0 = (int)fj, r0 = (int)fr;                                                  // -1 .. W-1, -1 .. H-1
  const double al = su - fj, be = sv - fr;
  const double fmin = (double)(K[0] < K[4] ? K[0] : K[4]);
  const double om = 1.0 - c * c;
  const double tol = (double)a.z_tol_mm + (((double)a.slope * (z / fmin)) * sqrt(om > 0.0 ? om : 0.0)) / c;
  const int64_t plane = (int64_t)a.H * a.W;
  const float* zb = a.zbuf + (int64_t)b * plane;
  const float* im = a.rgb + (int64_t)b * plane * 3;
  const float* wp = a.weight ? a.weight + (int64_t)b * plane : nullptr;
  double cover = 0.0, cr = 0.0, cg = 0.0, cb = 0.0, cw = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int dr = t >> 1, dj = t & 1;
    const int r = r0 + dr, j = j0 + dj;
    if (r < 0 || r >= a.H || j < 0 || j >= a.W) continue;
    const int64_t o = (int64_t)r * a.W + j;
    const float zt = zb[o];
    if (!(zt > 0.f) || !(fabs((double)zt - z) <= tol)) continue;
    const float pr = im[o * 3], pg = im[o * 3 + 1], pb = im[o * 3 + 2];
    const float pw = wp ? wp[o] : 1.f;
    if (!(isfinite(pr) && isfinite(pg) && isfinite(pb) && isfinite(pw))) continue;
    const double w = (dj ? al : 1.0 - al) * (dr ? be : 1.0 - be);
    cover += w;
    cr += w * (double)pr; cg += w * (double)pg; cb += w * (double)pb; cw += w * (double)pw;
  }
  if (!(cover >= (double)a.cover_min)) return;
  double wb = c * cover;
  if (wp) wb = wb * (cw / cover);
  s.r += wb * (cr / cover); s.g += wb * (cg / cover); s.b += wb * (cb / cover); s.w += wb;
  s.n += 1;
}

// grid (ceil(V / 256), S); workspace: part [S][V][4] doubles, then cnt [S][V] int32
__global__ __launch_bounds__(kBakeBlock) void bake_slice_kernel(tp_texture_bake_args a, int L, double* part, int32_t* cnt) {
  const int i = blockIdx.x * kBakeBlock + threadIdx.x;
  if (i >= a.V) return;
  const int s = blockIdx.y;
  const int b0 = s * L, b1 = b0 + L < a.B ? b0 + L : a.B;
  const double vx = (double)a.verts[(int64_t)i * 3], vy = (double)a.verts[(int64_t)i * 3 + 1], vz = (double)a.verts[(int64_t)i * 3 + 2];
  const double nx = (double)a.normals[(int64_t)i * 3], ny = (double)a.normals[(int64_t)i * 3 + 1], nz = (double)a.normals[(int64_t)i * 3 + 2];
  Sums sum = {0.0, 0.0, 0.0, 0.0, 0};
  for (int b = b0; b < b1; ++b) bake_pair(a, b, vx, vy, vz, nx, ny, nz, sum);
  const int64_t o = (int64_t)s * a.V + i;
  double2* p = reinterpret_cast<double2*>(part + o * 4);
  p[0] = make_double2(sum.r, sum.g);
  p[1] = make_double2(sum.b, sum.w);
  cnt[o] = sum.n;
}

// one thread per vertex: the S partial sums in ascending order
__global__ __launch_bounds__(kBakeBlock) void bake_sum_kernel(tp_texture_bake_args a, int S, const double* part, const int32_t* cnt) {
  const int i = blockIdx.x * kBakeBlock + threadIdx.x;
  if (i >= a.V) return;
  double r = 0.0, g = 0.0, bl = 0.0, w = 0.0;
  int n = 0;
  for (int s = 0; s < S; ++s) {
    const int64_t o = (int64_t)s * a.V + i;
    const double2* p = reinterpret_cast<const double2*>(part + o * 4);
    const double2 p0 = p[0], p1 = p[1];
    r += p0.x; g += p0.y; bl += p1.x; w += p1.y;
    n += cnt[o];
  }
  float4* out = reinterpret_cast<float4*>(a.acc) + i;
  if (a.clear) {
    *out = make_float4((float)r, (float)g, (float)bl, (float)w);
    a.count[i] = n;
  } else {
    const float4 old = *out;
    *out = make_float4((float)((double)old.x + r), (float)((double)old.y + g), (float)((double)old.z + bl), (float)((double)old.w + w));
    a.count[i] += n;
  }
}
}  // namespace

extern "C" int tp_texture_bake_slices(int V, int B) {
  if (V <= 0 || B <= 0) return 0;
  const int L = bake_slice_len(V, B);
  return (B + L - 1) / L;
}

extern "C" size_t tp_texture_bake_workspace_bytes(int V, int B) {
  const int S = tp_texture_bake_slices(V, B);
  return (size_t)S * (size_t)(V > 0 ? V : 0) * (4 * sizeof(double) + sizeof(int32_t));
}

extern "C" int tp_texture_bake(const tp_texture_bake_args* a, tp_stream_t stream) {
  if (!a) { tp::set_error("tp_texture_bake: null args"); return -1; }
  if (!a->verts || !a->normals || !a->pose || !a->intr || !a->rgb || !a->zbuf || !a->acc || !a->count || !a->workspace) {
    tp::set_error("tp_texture_bake: null pointer");
    return -1;
  }
  if (a->V <= 0 || a->V > (1 << 30) || a->B <= 0 || a->B > 65535 || a->H <= 0 || a->W <= 0 || (int64_t)a->H * a->W > 0x7FFFFFFFll) {
    tp::set_error("tp_texture_bake: bad sizes (V 1..2^30, B 1..65535, H > 0, W > 0, H * W < 2^31)");
    return -1;
  }
  if (!(a->cos_min > 0.f && a->cos_min <= 1.f) || !(a->cover_min > 0.f && a->cover_min <= 1.f) || !(a->z_tol_mm >= 0.f) || !(a->slope >= 0.f)) {
    tp::set_error("tp_texture_bake: cos_min and cover_min in (0, 1], z_tol_mm >= 0 and slope >= 0 expected");
    return -1;
  }
  if (((uintptr_t)a->workspace | (uintptr_t)a->acc) & 15u) { tp::set_error("tp_texture_bake: workspace and acc must be 16-byte aligned"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  const int L = bake_slice_len(a->V, a->B), S = (a->B + L - 1) / L;
  double* part = static_cast<double*>(a->workspace);
  int32_t* cnt = reinterpret_cast<int32_t*>(part + (int64_t)S * a->V * 4);
  const unsigned tiles = (unsigned)((a->V + kBakeBlock - 1) / kBakeBlock);
  hipLaunchKernelGGL(bake_slice_kernel, dim3(tiles, S), dim3(kBakeBlock), 0, st, *a, L, part, cnt);
  hipLaunchKernelGGL(bake_sum_kernel, dim3(tiles), dim3(kBakeBlock), 0, st, *a, S, (const double*)part, (const int32_t*)cnt);
  return tp::check_launch("tp_texture_bake");
}
