// K35 tp_face_texel_shade: colour the pixels of a rasterised mesh from a per-face texel texture ("mesh colours"; the
// public functions are in texpose_amd/face_texels.py, the rule in include/texpose_amd.h, restated in tests/face_texels_ref.py).
//
// The texture: resolution R (1 .. 64); face f with vertices (v0, v1, v2) in its own order carries the nodes (i, j), i, j >= 0,
// i + j <= R, node (i, j) at the barycentric weights ((R - i - j) / R, i / R, j / R), stored at n(i, j) = j (R + 1) - j (j - 1) / 2 + i
// of the face's T(R) = (R + 1)(R + 2) / 2 texels.  The nodes of all faces are the vertices of the mesh subdivided R times.
//
// A pixel whose winning face (K19's face plane) is f:
//   1. u_k, v_k, 1 / z_k of the three vertices in fp64 exactly as face_setup_kernel of mesh_raster.hip forms them; twice the area;
//      the edge functions b_k at the pixel centre (j + 0.5, i + 0.5) over twice the area; t_k = b_k / z_k; w_k = t_k / ((t_0 + t_1) + t_2);
//      negative w_k become 0 and the three are divided by their sum ((w_0 + w_1) + w_2).
//   2. a = R w_1, b = R w_2, i = min(floor(a), R - 1), j = min(floor(b), R - 1 - i), fa = a - i, fb = b - j.  Where fa + fb > 1 and the
//      cell (i, j) has an upper triangle (i + j <= R - 2):  c = (fa + fb - 1) N(i+1, j+1) + (1 - fb) N(i+1, j) + (1 - fa) N(i, j+1);
//      otherwise  c = (1 - fa - fb) N(i, j) + fa N(i+1, j) + fb N(i, j+1).  (On the last diagonal fa + fb exceeds 1 by rounding alone.)
//   3. every step fp64 as written (the library is built without contraction), rounded to fp32 once.
// Zeros are written, and nothing else is read, for face < 0 or >= F, a vertex index outside 0 .. V-1, a vertex at z <= 0, |twice the
// area| <= 1e-10 or any non-finite intermediate (a non-finite colour included).
//
// A gather: 4 B read and 12 B written per pixel; a covered pixel gathers 3 indices, 9 vertex floats and 9 texel floats, which
// neighbouring pixels of a face share.  One thread per pixel, the image index uniform over the workgroup (pose[b] and intr[b] are scalar
// loads).  One launch; no LDS, no atomics, no workspace: the output is a function of the inputs alone.
#include "tp_common.h"

namespace {
constexpr int kShadeBlock = 256;

__global__ __launch_bounds__(kShadeBlock) void face_texel_shade_kernel(tp_face_texel_shade_args a, int blocks_per_image, int T) {
  const int b = (int)(blockIdx.x / (unsigned)blocks_per_image);                  // workgroup-uniform
  const int64_t hw = (int64_t)a.H * a.W;
  const int64_t rem = (int64_t)(blockIdx.x - (unsigned)b * (unsigned)blocks_per_image) * kShadeBlock + threadIdx.x;
  if (rem >= hw) return;
  const int64_t pix = (int64_t)b * hw + rem;
  float* out = a.rgb + 3 * pix;
  double col[3] = {0.0, 0.0, 0.0};
  const int f = a.face[pix];
  bool ok = f >= 0 && f < a.F;
  if (ok) {
    const int i = (int)(rem / a.W), j = (int)(rem - (int64_t)i * a.W);
    const float* P = a.pose + 12 * (int64_t)b;
    const float* K = a.intr + 9 * (int64_t)b;
    double u[3], v[3], iz[3];
    for (int k = 0; k < 3 && ok; ++k) {
      const int vi = a.faces[3 * (int64_t)f + k];
      if (vi < 0 || vi >= a.V) { ok = false; break; }
      const double X = a.verts[3 * (int64_t)vi], Y = a.verts[3 * (int64_t)vi + 1], Z = a.verts[3 * (int64_t)vi + 2];
      double c[3];
      for (int r = 0; r < 3; ++r) c[r] = (double)P[4 * r] * X + (double)P[4 * r + 1] * Y + (double)P[4 * r + 2] * Z + (double)P[4 * r + 3];
      if (!(c[2] > 0.0) || !isfinite(c[0]) || !isfinite(c[1]) || !isfinite(c[2])) { ok = false; break; }
      const double q0 = (double)K[0] * c[0] + (double)K[1] * c[1] + (double)K[2] * c[2];
      const double q1 = (double)K[3] * c[0] + (double)K[4] * c[1] + (double)K[5] * c[2];
      const double q2 = (double)K[6] * c[0] + (double)K[7] * c[1] + (double)K[8] * c[2];
      u[k] = q0 / q2;
      v[k] = q1 / q2;
      iz[k] = 1.0 / c[2];
    }
    double w[3] = {0.0, 0.0, 0.0};
    if (ok) {
      const double area = (u[1] - u[0]) * (v[2] - v[0]) - (v[1] - v[0]) * (u[2] - u[0]);
      ok = isfinite(area) && fabs(area) > 1e-10;
      if (ok) {
        const double px = (double)j + 0.5, py = (double)i + 0.5;
        double t[3];
        for (int k = 0; k < 3; ++k) {
          const int s = (k + 1) % 3, e = (k + 2) % 3;       // b_k: the edge opposite vertex k, from vertex s to vertex e
          const double ex = u[e] - u[s], ey = v[e] - v[s];
          t[k] = ((ex * (py - v[s]) - ey * (px - u[s])) / area) * iz[k];
        }
        const double sum = (t[0] + t[1]) + t[2];
        for (int k = 0; k < 3; ++k) {
          w[k] = t[k] / sum;
          w[k] = w[k] < 0.0 ? 0.0 : w[k];
        }
        const double s2 = (w[0] + w[1]) + w[2];
        for (int k = 0; k < 3; ++k) w[k] = w[k] / s2;
        ok = isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]);     // (then every w_k is in [0, 1])
      }
    }
    if (ok) {
      const int R = a.R;
      const double ta = (double)R * w[1], tb = (double)R * w[2];
      int ci = (int)floor(ta), cj = (int)floor(tb);
      ci = ci < R - 1 ? ci : R - 1;
      cj = cj < R - 1 - ci ? cj : R - 1 - ci;
      const double fa = ta - (double)ci, fb = tb - (double)cj;
      const bool upper = fa + fb > 1.0 && ci + cj <= R - 2;
      // node (i, j) at j (R + 1) - j (j - 1) / 2 + i; the row above starts R + 1 - j further on
      const int n00 = cj * (R + 1) - (cj * (cj - 1)) / 2 + ci;
      const int n01 = n00 + (R + 1 - cj);                   // (i, j + 1)
      const float* tex = a.texels + 3 * ((int64_t)f * T);
      const float* A = tex + 3 * (int64_t)(upper ? n01 + 1 : n00);   // (i + 1, j + 1) or (i, j)
      const float* Bn = tex + 3 * (int64_t)(n00 + 1);                // (i + 1, j)
      const float* Cn = tex + 3 * (int64_t)n01;                      // (i, j + 1)
      const double wa = upper ? (fa + fb) - 1.0 : (1.0 - fa) - fb;
      const double wb = upper ? 1.0 - fb : fa;
      const double wc = upper ? 1.0 - fa : fb;
      for (int c = 0; c < 3; ++c) col[c] = (wa * (double)A[c] + wb * (double)Bn[c]) + wc * (double)Cn[c];
      if (!(isfinite(col[0]) && isfinite(col[1]) && isfinite(col[2]))) col[0] = col[1] = col[2] = 0.0;
    }
  }
  out[0] = (float)col[0];
  out[1] = (float)col[1];
  out[2] = (float)col[2];
}
}  // namespace

extern "C" int tp_face_texel_count(int R) {
  return R >= 1 && R <= TP_FACE_TEXEL_MAX_R ? (R + 1) * (R + 2) / 2 : 0;
}

extern "C" int tp_face_texel_shade(const tp_face_texel_shade_args* a, tp_stream_t stream) {
  if (!a) { tp::set_error("tp_face_texel_shade: null args"); return -1; }
  if (!a->verts || !a->faces || !a->texels || !a->pose || !a->intr || !a->face || !a->rgb) {
    tp::set_error("tp_face_texel_shade: null pointer");
    return -1;
  }
  const int T = tp_face_texel_count(a->R);
  if (a->B <= 0 || a->H <= 0 || a->W <= 0 || a->V <= 0 || a->F <= 0 || T == 0 || (int64_t)a->H * a->W > 0x7FFFFFFFll ||
      (int64_t)a->F * T > 0x7FFFFFFFll) {
    tp::set_error("tp_face_texel_shade: bad sizes (B, H, W, V, F > 0, R 1..%d, H * W < 2^31, F * T(R) < 2^31)", TP_FACE_TEXEL_MAX_R);
    return -1;
  }
  const int64_t bpi = ((int64_t)a->H * a->W + kShadeBlock - 1) / kShadeBlock;
  if (bpi * a->B > 0x7FFFFFFFll) { tp::set_error("tp_face_texel_shade: bad sizes (B * ceil(H * W / 256) < 2^31)"); return -1; }
  hipLaunchKernelGGL(face_texel_shade_kernel, dim3((unsigned)(bpi * a->B)), dim3(kShadeBlock), 0, (hipStream_t)stream, *a, (int)bpi, T);
  return tp::check_launch("tp_face_texel_shade");
}
