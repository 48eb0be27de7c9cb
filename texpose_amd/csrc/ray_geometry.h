// The camera algebra of a pixel ray and the slab test, shared by the ray generation (K1, raygen.hip) and the scene bounds (K21,
// scene_bounds.hip): one definition, so that bounds evaluated per pixel are bit-identical to the bounds of the rays that get rendered.
// Every operation is a single rounded fp32 step in the reference's order (camera.py:266-277,308-314,415-433; DESIGN "numerics").
#pragma once
#include "tp_common.h"

namespace tp_ray {

struct Cam {
  float kinv[9];
  float rt[9];    // R^T
  float tinv[3];  // -R^T t
};

__device__ __forceinline__ void load_cam(const float* __restrict__ intr, const float* __restrict__ pose, int b, Cam& c) {
  const float* K = intr + 9 * b;
  const float a = K[0], bb = K[1], cc = K[2], d = K[3], e = K[4], f = K[5], g = K[6], h = K[7], i = K[8];
  const float A = e * i - f * h, Bc = -(d * i - f * g), C = d * h - e * g;
  const float det = a * A + bb * Bc + cc * C;
  const float r = 1.0f / det;
  c.kinv[0] = A * r;  c.kinv[1] = -(bb * i - cc * h) * r;  c.kinv[2] = (bb * f - cc * e) * r;
  c.kinv[3] = Bc * r; c.kinv[4] = (a * i - cc * g) * r;    c.kinv[5] = -(a * f - cc * d) * r;
  c.kinv[6] = C * r;  c.kinv[7] = -(a * h - bb * g) * r;   c.kinv[8] = (a * e - bb * d) * r;
  const float* P = pose + 12 * b;
#pragma unroll
  for (int r_ = 0; r_ < 3; ++r_)
#pragma unroll
    for (int c_ = 0; c_ < 3; ++c_) c.rt[r_ * 3 + c_] = P[c_ * 4 + r_];
  const float t0 = P[3], t1 = P[7], t2 = P[11];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float acc = tp::mul_rn(-c.rt[j * 3 + 0], t0);
    acc = tp::fma_rn(-c.rt[j * 3 + 1], t1, acc);
    acc = tp::fma_rn(-c.rt[j * 3 + 2], t2, acc);
    c.tinv[j] = acc;
  }
}

// the ray through image position (u, v): g = K^-1 [u,v,1];  world = R^T g + tinv;  o = tinv, d = world - tinv
// (a pixel (row i, column j) is sampled at u = j + 0.5, v = i + 0.5)
__device__ __forceinline__ void pixel_ray(const Cam& cam, float u, float v, float* o, float* d) {
  float g[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float acc = tp::mul_rn(u, cam.kinv[j * 3 + 0]);
    acc = tp::fma_rn(v, cam.kinv[j * 3 + 1], acc);
    g[j] = tp::add_rn(acc, cam.kinv[j * 3 + 2]);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    float acc = tp::mul_rn(g[0], cam.rt[j * 3 + 0]);
    acc = tp::fma_rn(g[1], cam.rt[j * 3 + 1], acc);
    acc = tp::fma_rn(g[2], cam.rt[j * 3 + 2], acc);
    const float world = tp::add_rn(acc, cam.tinv[j]);
    o[j] = cam.tinv[j];
    d[j] = tp::sub_rn(world, cam.tinv[j]);
  }
}

__device__ __forceinline__ void slab(const float* amin, const float* amax, const float* o, const float* d,
                                     float& tn, float& tf, bool& valid) {
  tn = -INFINITY; tf = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float inv = tp::div_rn(1.0f, d[a]);
    const float ta = tp::mul_rn(tp::sub_rn(amin[a], o[a]), inv);
    const float tb = tp::mul_rn(tp::sub_rn(amax[a], o[a]), inv);
    // torch.minimum/maximum propagate NaN (0*inf when the origin sits on a slab plane of a parallel ray)
    const float lo = (ta != ta || tb != tb) ? NAN : fminf(ta, tb);
    const float hi = (ta != ta || tb != tb) ? NAN : fmaxf(ta, tb);
    tn = (tn != tn || lo != lo) ? NAN : fmaxf(tn, lo);
    tf = (tf != tf || hi != hi) ? NAN : fminf(tf, hi);
  }
  valid = (tf > 0.0f) && (tf > tn);
}

}  // namespace tp_ray
