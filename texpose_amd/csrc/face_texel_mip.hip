// K43: mip levels of a face-texel texture, a minification filter for K35's shading (the public functions are in
// texpose_amd/face_texels.py, the rules in include/texpose_amd.h, restated in tests/face_texel_mip_ref.py).
//
// The chain: level l has resolution R_l = R >> l (it exists while R_(l-1) is even) and is a contiguous [F, T(R_l), 3] block of ONE packed
// fp32 buffer at element offset 3 F sum_{k<l} T(R_k).  Coarse node (I, J) of a face is fine node (2I, 2J) of the same face.
//
// K43a tp_face_texel_mip_reduce: one level down.  One thread per UNIQUE coarse node u; its slots come from a CSR pair built on the host.
// For every slot (f, n -> (I, J)) in list order and every coarse cell of f at that corner -- the pairs of consecutive lattice directions
// d_k, d_(k+1) whose two end nodes are in the coarse grid -- acc += (2 x(2I,2J) + 3 x((2I,2J) + d_k)) + 3 x((2I,2J) + d_(k+1)), wacc += 8,
// fp64 as written, x face f's own fine texels.  (float)(acc / wacc) goes to every slot of u: full weighting on the triangular lattice, the
// same rule at mesh vertices, edges and open boundaries, no valence needed.  The thread owns its node: no atomics, no reduction across
// threads.  A node reads three fine texels (36 B) per incident cell -- six cells around an inner node -- and writes 12 B per slot.
//
// K43b tp_face_texel_shade_mip: K35 with a level chosen per pixel.  Step 1 of K35 (face_texel_weights, the same device function) gives
// the weights once and the footprint d in closed form from values it has formed already; the level pair and the blend weight come from
// d's exponent and an exact scaling (no transcendental); step 2 and the three-texel sum run once per level that is read.  A magnified
// pixel (d <= 1) is K35's pixel: one level, the same expression.  One thread per pixel, 256 per workgroup, K35's grid, the image index
// uniform over the workgroup (pose[b] and intr[b] are scalar loads); no LDS, no atomics.  Beyond K35 a blending pixel gathers three more
// texels (36 B) and spends about a dozen fp64 operations on d, t and the blend.
#include "tp_common.h"
#include "face_texel_cell.h"

namespace {
constexpr int kMipBlock = 256;

__host__ __device__ __forceinline__ int texel_count_of(int R) { return (R + 1) * (R + 2) / 2; }

// ---- K43a
__global__ __launch_bounds__(kMipBlock) void face_texel_mip_reduce_kernel(tp_face_texel_mip_reduce_args a, int Tf, int Tc) {
  const int64_t u = (int64_t)blockIdx.x * kMipBlock + threadIdx.x;
  if (u >= a.U) return;
  const int Rf = a.Rf, Rc = a.Rf >> 1;
  const int64_t slots = (int64_t)a.F * Tc;                     // (< 2^31: checked by the caller)
  int64_t beg = a.slot_ptr[u], end = a.slot_ptr[u + 1];
  beg = beg < 0 ? 0 : beg;
  end = end > slots ? slots : end;
  const int dx[6] = {1, 0, -1, -1, 0, 1}, dy[6] = {0, 1, 1, 0, -1, -1};
  double acc[3] = {0.0, 0.0, 0.0}, wacc = 0.0;
  for (int64_t p = beg; p < end; ++p) {
    const int s = a.slot_list[p];
    if (s < 0 || s >= slots) continue;
    const int f = s / Tc;
    int I = s - f * Tc, J = 0;                                 // n -> (I, J): row J holds Rc + 1 - J nodes
    while (I >= Rc + 1 - J) {
      I -= Rc + 1 - J;
      ++J;
    }
    const float* x = a.fine + 3 * ((int64_t)f * Tf);
    const int fi = 2 * I, fj = 2 * J;
    const int nc = fj * (Rf + 1) - (fj * (fj - 1)) / 2 + fi;
    const double xc[3] = {(double)x[3 * nc], (double)x[3 * nc + 1], (double)x[3 * nc + 2]};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int k1 = (k + 1) % 6;
      const int ai = I + dx[k], aj = J + dy[k], bi = I + dx[k1], bj = J + dy[k1];
      if (ai < 0 || aj < 0 || ai + aj > Rc || bi < 0 || bj < 0 || bi + bj > Rc) continue;
      const int pi = fi + dx[k], pj = fj + dy[k], qi = fi + dx[k1], qj = fj + dy[k1];          // the two edge midpoints: fine nodes of f
      const float* xa = x + 3 * (int64_t)(pj * (Rf + 1) - (pj * (pj - 1)) / 2 + pi);
      const float* xb = x + 3 * (int64_t)(qj * (Rf + 1) - (qj * (qj - 1)) / 2 + qi);
      for (int c = 0; c < 3; ++c) acc[c] = acc[c] + ((2.0 * xc[c] + 3.0 * (double)xa[c]) + 3.0 * (double)xb[c]);
      wacc = wacc + 8.0;
    }
  }
  if (!(wacc > 0.0)) return;                                   // no valid slot: nothing to write
  const float out[3] = {(float)(acc[0] / wacc), (float)(acc[1] / wacc), (float)(acc[2] / wacc)};
  for (int64_t p = beg; p < end; ++p) {
    const int s = a.slot_list[p];
    if (s < 0 || s >= slots) continue;
    float* o = a.coarse + 3 * (int64_t)s;
    o[0] = out[0];
    o[1] = out[1];
    o[2] = out[2];
  }
}

// ---- K43b
__global__ __launch_bounds__(kMipBlock) void face_texel_shade_mip_kernel(tp_face_texel_shade_mip_args a, int blocks_per_image) {
  const int b = (int)(blockIdx.x / (unsigned)blocks_per_image);                  // workgroup-uniform
  const int64_t hw = (int64_t)a.H * a.W;
  const int64_t rem = (int64_t)(blockIdx.x - (unsigned)b * (unsigned)blocks_per_image) * kMipBlock + threadIdx.x;
  if (rem >= hw) return;
  const int64_t pix = (int64_t)b * hw + rem;
  float* out = a.rgb + 3 * pix;
  double col[3] = {0.0, 0.0, 0.0};
  const int f = a.face[pix];
  if (f >= 0 && f < a.F) {
    const int i = (int)(rem / a.W), j = (int)(rem - (int64_t)i * a.W);
    TexelWeights g;
    if (face_texel_weights(a.verts, a.faces, a.pose + 12 * (int64_t)b, a.intr + 9 * (int64_t)b, a.V, f, i, j, g)) {
      const double as = fabs(g.sum);
      const double d = (((double)a.footprint * (double)(a.R * a.R)) * fabs(g.iz3)) / (fabs(g.area) * ((as * as) * as));
      int l0 = 0;
      double t = 0.0;
      if (a.L > 1 && d > 1.0 && isfinite(d)) {
        const int e = (int)((__double_as_longlong(d) >> 52) & 0x7FF) - 1023;      // ilogb of a finite d > 1
        l0 = e >> 1;
        if (l0 >= a.L - 1) l0 = a.L - 1;
        else t = (ldexp(d, -2 * l0) - 1.0) / 3.0;
      }
      int64_t before = 0;                                       // slots per face in the levels before l0
      int Rl = a.R;
      for (int k = 0; k < l0; ++k) {
        before += texel_count_of(Rl);
        Rl >>= 1;
      }
      const int Tl = texel_count_of(Rl);
      const float* tex = a.mips + 3 * ((int64_t)a.F * before + (int64_t)f * Tl);
      TexelCell cell;
      face_texel_cell_at(g.w, Rl, cell);
      face_texel_colour(tex, cell, col);
      if (t > 0.0) {                                            // (then l0 + 1 <= L - 1: the next level exists)
        const int Rn = Rl >> 1;
        const float* next = a.mips + 3 * ((int64_t)a.F * (before + Tl) + (int64_t)f * texel_count_of(Rn));
        double cn[3];
        face_texel_cell_at(g.w, Rn, cell);
        face_texel_colour(next, cell, cn);
        for (int c = 0; c < 3; ++c) col[c] = (1.0 - t) * col[c] + t * cn[c];
      }
      if (!(isfinite(col[0]) && isfinite(col[1]) && isfinite(col[2]))) col[0] = col[1] = col[2] = 0.0;
    }
  }
  out[0] = (float)col[0];
  out[1] = (float)col[1];
  out[2] = (float)col[2];
}
}  // namespace

extern "C" int64_t tp_face_texel_mip_elems(int F, int R, int L) {
  if (F <= 0 || R < 1 || R > TP_FACE_TEXEL_MAX_R || L < 1 || L > 7 || (R & ((1 << (L - 1)) - 1)) != 0) return 0;
  int64_t per_face = 0;
  for (int l = 0; l < L; ++l) per_face += texel_count_of(R >> l);
  if ((int64_t)F * per_face > 0x7FFFFFFFll) return 0;
  return 3 * (int64_t)F * per_face;
}

extern "C" int tp_face_texel_mip_reduce(const tp_face_texel_mip_reduce_args* a, tp_stream_t stream) {
  const char* name = "tp_face_texel_mip_reduce";
  if (!a) { tp::set_error("%s: null args", name); return -1; }
  if (!a->fine || !a->slot_ptr || !a->slot_list || !a->coarse) { tp::set_error("%s: null pointer", name); return -1; }
  if (a->F <= 0 || a->U <= 0 || a->Rf < 2 || a->Rf > TP_FACE_TEXEL_MAX_R || (a->Rf & 1) ||
      (int64_t)a->F * texel_count_of(a->Rf) > 0x7FFFFFFFll) {
    tp::set_error("%s: bad sizes (F, U > 0, Rf even in 2..%d, F * T(Rf) < 2^31)", name, TP_FACE_TEXEL_MAX_R);
    return -1;
  }
  const int Tf = texel_count_of(a->Rf), Tc = texel_count_of(a->Rf >> 1);
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(a->coarse, 0, sizeof(float) * 3 * (size_t)a->F * (size_t)Tc, s);
  if (e != hipSuccess) { tp::set_error("%s: hipMemsetAsync: %s", name, hipGetErrorString(e)); return (int)e; }
  const unsigned blocks = (unsigned)(((int64_t)a->U + kMipBlock - 1) / kMipBlock);
  hipLaunchKernelGGL(face_texel_mip_reduce_kernel, dim3(blocks), dim3(kMipBlock), 0, s, *a, Tf, Tc);
  return tp::check_launch(name);
}

extern "C" int tp_face_texel_shade_mip(const tp_face_texel_shade_mip_args* a, tp_stream_t stream) {
  const char* name = "tp_face_texel_shade_mip";
  if (!a) { tp::set_error("%s: null args", name); return -1; }
  if (!a->verts || !a->faces || !a->mips || !a->pose || !a->intr || !a->face || !a->rgb) { tp::set_error("%s: null pointer", name); return -1; }
  if (a->B <= 0 || a->H <= 0 || a->W <= 0 || a->V <= 0 || a->F <= 0 || (int64_t)a->H * a->W > 0x7FFFFFFFll ||
      tp_face_texel_mip_elems(a->F, a->R, a->L) == 0) {
    tp::set_error("%s: bad sizes (B, H, W, V, F > 0, R 1..%d, L >= 1 with R %% 2^(L-1) == 0, H * W < 2^31, F * sum T(R_l) < 2^31)", name,
                  TP_FACE_TEXEL_MAX_R);
    return -1;
  }
  if (!(a->footprint > 0.0f && a->footprint <= 3.402823466e38f)) { tp::set_error("%s: footprint must be finite and > 0", name); return -1; }
  const int64_t bpi = ((int64_t)a->H * a->W + kMipBlock - 1) / kMipBlock;
  if (bpi * a->B > 0x7FFFFFFFll) { tp::set_error("%s: bad sizes (B * ceil(H * W / 256) < 2^31)", name); return -1; }
  hipLaunchKernelGGL(face_texel_shade_mip_kernel, dim3((unsigned)(bpi * a->B)), dim3(kMipBlock), 0, (hipStream_t)stream, *a, (int)bpi);
  return tp::check_launch(name);
}
