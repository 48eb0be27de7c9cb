// Steps 1 and 2 of K35's rule (include/texpose_amd.h), for every kernel that shades from a face-texel texture: K35 and K36
// (face_texels.hip) and K43b (face_texel_mip.hip).  One source, so that all of them give the same bits: step 1 (the pixel's three
// perspective-correct weights) is face_texel_weights, step 2 (the cell of a grid of resolution R under those weights) is
// face_texel_cell_at, and face_texel_cell is the two in a row, which is what K35 and K36 call.  K43b takes the weights once and the
// cell once per mip level, and reads the footprint from the values step 1 has already formed.
#pragma once
#include "tp_common.h"

namespace {
// the three slots of the face's T texels and their weights, in the order the forward adds them (A, B, C)
struct TexelCell {
  int n[3];
  double w[3];
};

// step 1's result: the clamped, renormalised weights and what the footprint of K43b is made of (1/z of the three vertices multiplied
// left to right, twice the signed screen area, S = (t_0 + t_1) + t_2 before the clamp)
struct TexelWeights {
  double w[3];
  double iz3, area, sum;
};

// Step 1 for pixel (row i, column j) under face f, 0 <= f < F.  false: the pixel is one that K35 shades to zero by rule.
__device__ __forceinline__ bool face_texel_weights(const float* __restrict__ verts, const int32_t* __restrict__ faces, const float* P, const float* K,
                                                   int V, int f, int i, int j, TexelWeights& g) {
  double u[3], v[3], iz[3];
  for (int k = 0; k < 3; ++k) {
    const int vi = faces[3 * (int64_t)f + k];
    if (vi < 0 || vi >= V) return false;
    const double X = verts[3 * (int64_t)vi], Y = verts[3 * (int64_t)vi + 1], Z = verts[3 * (int64_t)vi + 2];
    double c[3];
    for (int r = 0; r < 3; ++r) c[r] = (double)P[4 * r] * X + (double)P[4 * r + 1] * Y + (double)P[4 * r + 2] * Z + (double)P[4 * r + 3];
    if (!(c[2] > 0.0) || !isfinite(c[0]) || !isfinite(c[1]) || !isfinite(c[2])) return false;
    const double q0 = (double)K[0] * c[0] + (double)K[1] * c[1] + (double)K[2] * c[2];
    const double q1 = (double)K[3] * c[0] + (double)K[4] * c[1] + (double)K[5] * c[2];
    const double q2 = (double)K[6] * c[0] + (double)K[7] * c[1] + (double)K[8] * c[2];
    u[k] = q0 / q2;
    v[k] = q1 / q2;
    iz[k] = 1.0 / c[2];
  }
  const double area = (u[1] - u[0]) * (v[2] - v[0]) - (v[1] - v[0]) * (u[2] - u[0]);
  if (!(isfinite(area) && fabs(area) > 1e-10)) return false;
  const double px = (double)j + 0.5, py = (double)i + 0.5;
  double t[3], w[3];
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
  if (!(isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]))) return false;     // (then every w_k is in [0, 1])
  g.w[0] = w[0];
  g.w[1] = w[1];
  g.w[2] = w[2];
  g.iz3 = (iz[0] * iz[1]) * iz[2];
  g.area = area;
  g.sum = sum;
  return true;
}

// Step 2: the cell of the grid of resolution R under the weights w of step 1.
__device__ __forceinline__ void face_texel_cell_at(const double (&w)[3], int R, TexelCell& cell) {
  const double ta = (double)R * w[1], tb = (double)R * w[2];
  int ci = (int)floor(ta), cj = (int)floor(tb);
  ci = ci < R - 1 ? ci : R - 1;
  cj = cj < R - 1 - ci ? cj : R - 1 - ci;
  const double fa = ta - (double)ci, fb = tb - (double)cj;
  const bool upper = fa + fb > 1.0 && ci + cj <= R - 2;
  // node (i, j) at j (R + 1) - j (j - 1) / 2 + i; the row above starts R + 1 - j further on
  const int n00 = cj * (R + 1) - (cj * (cj - 1)) / 2 + ci;
  const int n01 = n00 + (R + 1 - cj);                   // (i, j + 1)
  cell.n[0] = upper ? n01 + 1 : n00;                    // (i + 1, j + 1) or (i, j)
  cell.n[1] = n00 + 1;                                  // (i + 1, j)
  cell.n[2] = n01;                                      // (i, j + 1)
  cell.w[0] = upper ? (fa + fb) - 1.0 : (1.0 - fa) - fb;
  cell.w[1] = upper ? 1.0 - fb : fa;
  cell.w[2] = upper ? 1.0 - fa : fb;
}

// Steps 1 and 2 of the rule for pixel (row i, column j) under face f, 0 <= f < F.  false: the pixel is one that K35 shades to zero by rule.
__device__ __forceinline__ bool face_texel_cell(const float* __restrict__ verts, const int32_t* __restrict__ faces, const float* P, const float* K,
                                                int V, int R, int f, int i, int j, TexelCell& cell) {
  TexelWeights g;
  if (!face_texel_weights(verts, faces, P, K, V, f, i, j, g)) return false;
  face_texel_cell_at(g.w, R, cell);
  return true;
}

// K35's colour of one cell: the three products added left to right, fp64 as written
__device__ __forceinline__ void face_texel_colour(const float* __restrict__ tex, const TexelCell& cell, double (&col)[3]) {
  const float* A = tex + 3 * (int64_t)cell.n[0];
  const float* Bn = tex + 3 * (int64_t)cell.n[1];
  const float* Cn = tex + 3 * (int64_t)cell.n[2];
  for (int c = 0; c < 3; ++c) col[c] = (cell.w[0] * (double)A[c] + cell.w[1] * (double)Bn[c]) + cell.w[2] * (double)Cn[c];
}
}  // namespace
