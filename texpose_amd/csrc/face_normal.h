// The valid normal of a pixel's face in the camera frame and the first-order SH shading under it, as K40 (photo_lighting.hip) states
// them in include/texpose_amd.h (steps 5 - 7 and the apply rule), for every kernel that shades by the face's own normal: K40 itself and
// K41 (face_texel_light.hip).  One source, so that both give the same bits.  Also the four-pixel load of the streaming kernels.
#pragma once
#include "tp_common.h"
#include "pose_gn.h"

namespace {
__device__ __forceinline__ bool finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// the four values of a thread's pixels from p0 on, `past` beyond the plane
template <bool VEC, class T, class T4>
__device__ __forceinline__ void load_four(const T* p, int64_t p0, int64_t plane, T past, T (&v)[kGnPix]) {
#pragma unroll
  for (int k = 0; k < kGnPix; ++k) v[k] = past;
  if constexpr (VEC) {
    if (p0 < plane) {                                                            // (plane % 4 == 0: the four are inside together)
      const T4 q = *reinterpret_cast<const T4*>(p + p0);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < kGnPix; ++k)
      if (p0 + k < plane) v[k] = p[p0 + k];
  }
}

// The valid normal of face f at the pose T [12] (steps 5 - 7 of K40's header block): false where f or one of its vertex indices is out
// of range or the normal has no finite positive length; nothing is read out of bounds.
__device__ __forceinline__ bool face_normal(const float* verts, const int32_t* faces, int V, int F, int f, const float* T, V3& n) {
  if (f < 0 || f >= F) return false;
  const int32_t* idx = faces + (int64_t)f * 3;
  const int i0 = idx[0], i1 = idx[1], i2 = idx[2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
  const float *p0 = verts + (int64_t)i0 * 3, *p1 = verts + (int64_t)i1 * 3, *p2 = verts + (int64_t)i2 * 3;
  const V3 v0 = {(double)p0[0], (double)p0[1], (double)p0[2]}, v1 = {(double)p1[0], (double)p1[1], (double)p1[2]},
           v2 = {(double)p2[0], (double)p2[1], (double)p2[2]};
  const V3 m = cross(v1 - v0, v2 - v0);
  const V3 r0 = {(double)T[0], (double)T[1], (double)T[2]}, r1 = {(double)T[4], (double)T[5], (double)T[6]},
           r2 = {(double)T[8], (double)T[9], (double)T[10]};
  V3 u = {dot(r0, m), dot(r1, m), dot(r2, m)};
  const double d = dot(u, u);
  if (!(isfinite(d) && d > 0.0)) return false;
  const double len = sqrt(d);
  u = {u.x / len, u.y / len, u.z / len};
  const V3 xc = {dot(r0, v0) + (double)T[3], dot(r1, v0) + (double)T[7], dot(r2, v0) + (double)T[11]};
  if (dot(u, xc) > 0.0) u = {-u.x, -u.y, -u.z};
  n = u;
  return true;
}

// the three shadings of a pixel of face f under the light l [3][5]: fp64 from the fp32 light and the valid normal, rounded once; l0
// itself without a normal
__device__ __forceinline__ void shade_of(const float* verts, const int32_t* faces, int V, int F, const float (&l)[15], int f, const float* T,
                                         float (&s)[3]) {
  V3 n;
  const bool valid = face_normal(verts, faces, V, F, f, T, n);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float* q = l + 5 * ch;
    s[ch] = valid ? (float)((((double)q[0] + (double)q[1] * n.x) + (double)q[2] * n.y) + (double)q[3] * n.z) : q[0];
  }
}
}  // namespace
