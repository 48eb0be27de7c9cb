// K41 tp_face_texel_light: the per-pixel step between K35's shading and K36's adjoint when face texels are fitted as an albedo under one
// first-order SH light per view (the public function is ops.face_texel_light in texpose_amd/ops/scene.py, the rule in
// include/texpose_amd.h).  K40's apply kernel (photo_lighting.hip) grown by the weight, the residual and the diagonal: the same tiling and
// load paths, the same normal and shading (face_normal.h), K30's order of sums.
//
//   texel_light  grid (ceil(H * W / 1024), B) x 256, four consecutive pixels per thread.  The 16-byte face load comes first; a thread
//                without a covered pixel loads nothing more and stores its zeros.  light[b] and pose[b] are wave-uniform.  With SUMS
//                the thread's two fp64 sums go through the wave's butterfly, lane 0 to LDS, the four waves in ascending order: one
//                record of two doubles per (image, tile).
//   texel_light_gather  grid B x 64: threads 0 and 1 add entry 0 / 1 of the image's records in ascending tile order.
// No atomics; every output is a function of the inputs alone.
#include "tp_common.h"
#include "pose_gn.h"
#include "pose_terms.h"
#include "face_normal.h"

namespace {
constexpr int kFtlRecord = 2;                          // sum m |e|^2, sum m

// VEC: H * W is a multiple of four and every plane given is 16-byte aligned; RESID: image given; SUMS: sums given (RESID only)
template <bool VEC, bool RESID, bool SUMS>
__global__ __launch_bounds__(kGnBlock) void texel_light_kernel(tp_face_texel_light_args a, double* part) {
  const int b = blockIdx.y;
  const int64_t plane = (int64_t)a.H * a.W;
  const int32_t* pf = a.face + (int64_t)b * plane;
  const float* pc = a.colour + (int64_t)b * plane * 3;
  const float* po = RESID ? a.image + (int64_t)b * plane * 3 : nullptr;
  const float* pw = a.weight ? a.weight + (int64_t)b * plane : nullptr;
  float* pg = a.grad + (int64_t)b * plane * 3;
  float* pd = a.diag ? a.diag + (int64_t)b * plane * 3 : nullptr;
  const float* T = a.pose + (int64_t)b * 12;
  const int64_t p0 = (int64_t)blockIdx.x * kGnTile + (int)threadIdx.x * kGnPix;            // (< H * W + 1024 < 2^31 + 1024)
  double acc[kFtlRecord] = {0.0, 0.0};

  if (p0 < plane) {
    int fs[kGnPix];
    load_four<VEC, int, int4>(pf, p0, plane, -1, fs);
    unsigned cov = 0u;                                                           // bit k: pixel k holds a face (past the plane: -1)
#pragma unroll
    for (int k = 0; k < kGnPix; ++k)
      if ((unsigned)fs[k] < (unsigned)a.F) cov |= 1u << k;

    float g[kGnPix * 3], d[kGnPix * 3];
#pragma unroll
    for (int k = 0; k < kGnPix * 3; ++k) { g[k] = 0.f; d[k] = 0.f; }
    if (cov != 0u) {
      float l[15];
#pragma unroll
      for (int e = 0; e < 15; ++e) l[e] = a.light[b * 15 + e];
      float ms[kGnPix], cs[kGnPix * 3], os[kGnPix * 3];
#pragma unroll
      for (int k = 0; k < kGnPix; ++k) ms[k] = 1.f;
      if (pw) load_four<VEC, float, float4>(pw, p0, plane, 0.f, ms);
#pragma unroll
      for (int k = 0; k < kGnPix * 3; ++k) { cs[k] = 0.f; os[k] = 0.f; }
      if constexpr (VEC) {                                                       // (p0 * 12 bytes: a multiple of 48)
        const float4* c4 = reinterpret_cast<const float4*>(pc + p0 * 3);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float4 c = c4[q];
          cs[4 * q] = c.x; cs[4 * q + 1] = c.y; cs[4 * q + 2] = c.z; cs[4 * q + 3] = c.w;
        }
        if constexpr (RESID) {
          const float4* o4 = reinterpret_cast<const float4*>(po + p0 * 3);
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const float4 o = o4[q];
            os[4 * q] = o.x; os[4 * q + 1] = o.y; os[4 * q + 2] = o.z; os[4 * q + 3] = o.w;
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < kGnPix; ++k)
          if (cov >> k & 1u) {                                                   // (a covered pixel lies inside the plane)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              cs[3 * k + ch] = pc[(p0 + k) * 3 + ch];
              if constexpr (RESID) os[3 * k + ch] = po[(p0 + k) * 3 + ch];
            }
          }
      }
#pragma unroll
      for (int k = 0; k < kGnPix; ++k) {
        if (!(cov >> k & 1u)) continue;
        const float m = ms[k];
        if (!(isfinite(m) && m > 0.f) || !finite3(cs + 3 * k)) continue;
        if (RESID && !finite3(os + 3 * k)) continue;
        float s[3], e[3] = {0.f, 0.f, 0.f};
        shade_of(a.verts, a.faces, a.V, a.F, l, fs[k], T, s);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float w = tp::mul_rn(m, s[ch]);
          const float q = tp::mul_rn(s[ch], cs[3 * k + ch]);
          if constexpr (RESID) {
            e[ch] = tp::sub_rn(os[3 * k + ch], tp::add_rn(q, l[5 * ch + 4]));
            g[3 * k + ch] = tp::mul_rn(w, e[ch]);
          } else {
            g[3 * k + ch] = tp::mul_rn(w, q);
          }
          d[3 * k + ch] = tp::mul_rn(w, s[ch]);
        }
        if constexpr (SUMS) {
          const double e0 = (double)e[0], e1 = (double)e[1], e2 = (double)e[2];
          acc[0] += (double)m * ((e0 * e0 + e1 * e1) + e2 * e2);
          acc[1] += (double)m;
        }
      }
    }

    if constexpr (VEC) {
      float4* g4 = reinterpret_cast<float4*>(pg + p0 * 3);
#pragma unroll
      for (int q = 0; q < 3; ++q) g4[q] = make_float4(g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]);
      if (pd) {
        float4* d4 = reinterpret_cast<float4*>(pd + p0 * 3);
#pragma unroll
        for (int q = 0; q < 3; ++q) d4[q] = make_float4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]);
      }
    } else {
#pragma unroll
      for (int k = 0; k < kGnPix; ++k) {
        if (p0 + k >= plane) break;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          pg[(p0 + k) * 3 + ch] = g[3 * k + ch];
          if (pd) pd[(p0 + k) * 3 + ch] = d[3 * k + ch];
        }
      }
    }
  }

  if constexpr (SUMS) {                                                          // (every thread of the workgroup arrives here)
    __shared__ double wave_part[kGnWaves][kFtlRecord];
    wave_sum_all(acc);
    const int lane = threadIdx.x & (tp::kWave - 1), wave = threadIdx.x / tp::kWave;
    if (lane == 0) { wave_part[wave][0] = acc[0]; wave_part[wave][1] = acc[1]; }
    __syncthreads();
    if (threadIdx.x < kFtlRecord) {
      double t = wave_part[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < kGnWaves; ++w) t += wave_part[w][threadIdx.x];
      part[((int64_t)b * gridDim.x + blockIdx.x) * kFtlRecord + threadIdx.x] = t;
    }
  }
}

// grid B, one wave: thread t < 2 adds entry t of the image's G records in ascending tile order
__global__ __launch_bounds__(tp::kWave) void texel_light_gather_kernel(const double* part, int G, double* sums) {
  if (threadIdx.x >= kFtlRecord) return;
  const double* rec = part + (int64_t)blockIdx.x * G * kFtlRecord + threadIdx.x;
  double t = 0.0;
#pragma unroll 8
  for (int g = 0; g < G; ++g) t += rec[(int64_t)g * kFtlRecord];                 // ascending tile order (the loads of a group in flight together)
  sums[blockIdx.x * kFtlRecord + threadIdx.x] = t;
}

size_t texel_light_workspace_bytes(int B, int H, int W) {                        // one record of two doubles per (image, tile)
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * (size_t)gn_tiles((int64_t)H * W) * kFtlRecord * sizeof(double);
}

struct Span { const void* p; size_t n; const char* name; };

bool texel_light_args_ok(const tp_face_texel_light_args& a) {
  const char* who = "tp_face_texel_light";
  if (a.B <= 0 || a.B > 65535 || a.H <= 0 || a.W <= 0 || (int64_t)a.H * a.W > 0x7FFFFFFFll || a.V <= 0 || a.F <= 0) {
    tp::set_error("%s: bad sizes (B 1..65535, H > 0, W > 0, H * W < 2^31, V > 0, F > 0)", who);
    return false;
  }
  if (!a.verts || !a.faces || !a.face || !a.pose || !a.light || !a.colour || !a.grad) { tp::set_error("%s: null pointer", who); return false; }
  if (a.sums && !a.image) { tp::set_error("%s: sums need image (residual mode)", who); return false; }
  if (a.sums && !a.workspace) { tp::set_error("%s: sums need a workspace", who); return false; }
  if (a.sums && ((uintptr_t)a.workspace & 7u)) { tp::set_error("%s: workspace must be 8-byte aligned", who); return false; }
  const size_t px = (size_t)a.B * (size_t)a.H * (size_t)a.W, planes = px * 3 * sizeof(float);
  const Span in[] = {{a.verts, (size_t)a.V * 12, "verts"},   {a.faces, (size_t)a.F * 12, "faces"}, {a.face, px * 4, "face"},
                     {a.pose, (size_t)a.B * 48, "pose"},     {a.light, (size_t)a.B * 60, "light"}, {a.colour, planes, "colour"},
                     {a.image, planes, "image"},             {a.weight, px * 4, "weight"}};
  const Span out[] = {{a.grad, planes, "grad"},
                      {a.diag, planes, "diag"},
                      {a.sums, (size_t)a.B * kFtlRecord * sizeof(double), "sums"},
                      {a.sums ? a.workspace : nullptr, texel_light_workspace_bytes(a.B, a.H, a.W), "workspace"}};
  auto overlap = [](const Span& x, const Span& y) {
    const uintptr_t p = (uintptr_t)x.p, q = (uintptr_t)y.p;
    return x.p && y.p && p < q + y.n && q < p + x.n;
  };
  for (size_t i = 0; i < sizeof(out) / sizeof(out[0]); ++i) {
    for (const Span& s : in)
      if (overlap(out[i], s)) { tp::set_error("%s: %s overlaps %s", who, out[i].name, s.name); return false; }
    for (size_t j = i + 1; j < sizeof(out) / sizeof(out[0]); ++j)
      if (overlap(out[i], out[j])) { tp::set_error("%s: %s overlaps %s", who, out[i].name, out[j].name); return false; }
  }
  return true;
}

template <bool VEC>
void texel_light_launch_as(const tp_face_texel_light_args& a, int G, double* part, hipStream_t st) {
  const dim3 grid(G, a.B), block(kGnBlock);
  if (!a.image) hipLaunchKernelGGL((texel_light_kernel<VEC, false, false>), grid, block, 0, st, a, part);
  else if (!a.sums) hipLaunchKernelGGL((texel_light_kernel<VEC, true, false>), grid, block, 0, st, a, part);
  else hipLaunchKernelGGL((texel_light_kernel<VEC, true, true>), grid, block, 0, st, a, part);
}

void texel_light_launch(const tp_face_texel_light_args& a, hipStream_t st) {
  const int64_t plane = (int64_t)a.H * a.W;
  const int G = (int)gn_tiles(plane);
  double* part = a.sums ? static_cast<double*>(a.workspace) : nullptr;
  const uintptr_t planes = (uintptr_t)a.face | (uintptr_t)a.colour | (uintptr_t)a.image | (uintptr_t)a.weight | (uintptr_t)a.grad | (uintptr_t)a.diag;
  if (plane % kGnPix == 0 && (planes & 15u) == 0) texel_light_launch_as<true>(a, G, part, st);      // (a null pointer is aligned)
  else texel_light_launch_as<false>(a, G, part, st);
  if (a.sums) hipLaunchKernelGGL(texel_light_gather_kernel, dim3(a.B), dim3(tp::kWave), 0, st, (const double*)part, G, a.sums);
}
}  // namespace

extern "C" size_t tp_face_texel_light_workspace_bytes(int B, int H, int W) { return texel_light_workspace_bytes(B, H, W); }

extern "C" int tp_face_texel_light(const tp_face_texel_light_args* a, tp_stream_t stream) {
  return tp::term_step("tp_face_texel_light", a, texel_light_args_ok, texel_light_launch, stream);
}
