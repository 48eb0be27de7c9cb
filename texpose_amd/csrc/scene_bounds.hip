// K21  per-pixel depth bounds, object labels and blended mesh depth of a scene of K objects at B novel poses: the z-buffer blend of
// the reference's novel-view loop on the device, in one launch.
// ref: model/nerf_pretrain.py:307-416 (the same code in nerf_pretrain_env.py): per object a slab test of its box against the pixel
//      rays (camera.py:292-314,415-433) and a depth render of its mesh, then torch.where / min / gather / where over the stack;
//      data/lm.py:352-356 (the 0.8 / 1.2 rule of range_source 'render').
//
// Inputs are tp_mesh_raster's zbuf planes ([K,B,H,W], view-space z in mm, <= 0 on background).  Per pixel:
//   z_k      = zbuf_k > 0 ? zbuf_k : 100000;   winner = the first k with the smallest z_k;   covered = zbuf_winner > 0
//   depth    = covered ? (z_winner / 1000) * depth_scale : 0          (two rounded fp32 steps)
//   label    = covered ? ids[winner] : 0
//   box      : label > 0 ? (slab valid ? (t_near, t_far) : (0, 0)) of the winner's box on the pixel ray : background range
//   render   : covered ? (depth * 0.8f, depth * 1.2f) : background range
//   none     : background range
// The pixel ray and the slab test are ray_geometry.h's, the ones tp_raygen runs: the box bounds of a pixel are bit-identical to the
// TP_BOUNDS_AABB bounds of the ray that gets rendered through it.
//
// HBM-bound stream: 4 K bytes read and 16 bytes written per pixel; no LDS, no atomics, no workspace.  A thread owns V consecutive
// pixels of the flat [B*H*W] index: V = 4 (one 16-byte load per plane and one 16-byte store per output and lane, 1 KiB per wavefront
// and instruction) when H*W is a multiple of four and the buffers are 16-byte aligned, else V = 1 (consecutive lanes on consecutive
// dwords).  The K loop is uniform across the launch; it is unrolled four planes deep so that four loads are in flight per lane.
// The winner's box and id are gathered from a K-row table (at most 896 bytes: one or two cache lines per wavefront).
#include "tp_common.h"
#include "ray_geometry.h"

namespace {

struct Params {
  const float* pose; const float* intr; const float* zbuf; const float* boxes; const int32_t* ids;
  int B, H, W, K, source;
  float depth_scale, bg_near, bg_far;
  float* z_near; float* z_far; int32_t* label; float* depth;
};

template <int V> struct Vec;
template <> struct Vec<1> { using F = float; using I = int32_t; };
template <> struct Vec<4> { using F = float4; using I = int4; };

constexpr float kFarAway = 100000.0f;     // the reference's stand-in for "no surface" (mm)

template <int V>
__global__ void __launch_bounds__(256) scene_bounds_kernel(Params p) {
  using VF = typename Vec<V>::F;
  using VI = typename Vec<V>::I;
  const int64_t hw = (int64_t)p.H * p.W, total = (int64_t)p.B * hw;
  const int64_t q0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (q0 >= total) return;                                    // (V = 4: total is a multiple of four, a vector is never ragged)
  float zmin[V], zraw[V];
  int win[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { zmin[e] = INFINITY; zraw[e] = -1.0f; win[e] = 0; }
  const float* plane = p.zbuf + q0;
#pragma unroll 4
  for (int k = 0; k < p.K; ++k, plane += total) {
    float z[V];
    const VF zv = *reinterpret_cast<const VF*>(plane);
    __builtin_memcpy(z, &zv, sizeof(zv));
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const float zk = z[e] > 0.0f ? z[e] : kFarAway;         // (NaN counts as background)
      const bool nearer = zk < zmin[e];                       // strict: ties stay with the lowest object index
      zmin[e] = nearer ? zk : zmin[e];
      zraw[e] = nearer ? z[e] : zraw[e];
      win[e] = nearer ? k : win[e];
    }
  }
  float near[V], far[V], depth[V];
  int32_t label[V];
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const bool covered = zraw[e] > 0.0f;
    depth[e] = covered ? tp::mul_rn(tp::div_rn(zmin[e], 1000.0f), p.depth_scale) : 0.0f;
    label[e] = covered ? p.ids[win[e]] : 0;
    near[e] = p.bg_near; far[e] = p.bg_far;
    if (p.source == TP_SCENE_RENDER && covered) {
      near[e] = tp::mul_rn(depth[e], 0.8f);
      far[e] = tp::mul_rn(depth[e], 1.2f);
    }
  }
  if (p.source == TP_SCENE_BOX) {
    const int b = (int)(q0 / hw);                             // (V = 4: hw is a multiple of four, the vector lies in one image)
    const int64_t rem = q0 - (int64_t)b * hw;
    const int row = (int)(rem / p.W), col = (int)(rem - (int64_t)row * p.W);
    tp_ray::Cam cam;
    tp_ray::load_cam(p.intr, p.pose, b, cam);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (label[e] <= 0) continue;
      int r = row, c = col + e;                               // (a vector may run over the end of an image row)
      while (c >= p.W) { c -= p.W; ++r; }
      float o[3], d[3], lo[3], hi[3];
      tp_ray::pixel_ray(cam, (float)c + 0.5f, (float)r + 0.5f, o, d);
      const float* box = p.boxes + 6 * win[e];
#pragma unroll
      for (int j = 0; j < 3; ++j) { lo[j] = box[j]; hi[j] = box[3 + j]; }
      float tn, tf; bool ok;
      tp_ray::slab(lo, hi, o, d, tn, tf, ok);
      near[e] = ok ? tn : 0.0f;
      far[e] = ok ? tf : 0.0f;
    }
  }
  VF out_near, out_far, out_depth;
  VI out_label;
  __builtin_memcpy(&out_near, near, sizeof(out_near));
  __builtin_memcpy(&out_far, far, sizeof(out_far));
  __builtin_memcpy(&out_label, label, sizeof(out_label));
  __builtin_memcpy(&out_depth, depth, sizeof(out_depth));
  *reinterpret_cast<VF*>(p.z_near + q0) = out_near;
  *reinterpret_cast<VF*>(p.z_far + q0) = out_far;
  *reinterpret_cast<VI*>(p.label + q0) = out_label;
  *reinterpret_cast<VF*>(p.depth + q0) = out_depth;
}

inline bool aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

}  // namespace

extern "C" int tp_scene_bounds(const tp_scene_bounds_args* a, tp_stream_t stream) {
  TP_REQUIRE(a, "null pointer");
  TP_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->H <= 16384 && a->W <= 16384, "bad sizes");
  TP_REQUIRE(a->K >= 1 && a->K <= TP_SCENE_MAX_OBJECTS, "1 <= K <= 32 objects expected");
  TP_REQUIRE(a->source == TP_SCENE_BOX || a->source == TP_SCENE_RENDER || a->source == TP_SCENE_NONE, "unknown source");
  TP_REQUIRE(a->zbuf && a->ids, "null pointer (zbuf / ids)");
  TP_REQUIRE(a->source != TP_SCENE_BOX || (a->pose && a->intr && a->boxes), "source box: pose, intr and boxes expected");
  TP_REQUIRE(a->z_near && a->z_far && a->label && a->depth, "null output pointer");
  const int64_t hw = (int64_t)a->H * a->W, total = (int64_t)a->B * hw;
  TP_REQUIRE(total <= (int64_t)INT32_MAX, "bad sizes (more than 2^31 - 1 pixels)");
  Params p;
  p.pose = a->pose; p.intr = a->intr; p.zbuf = a->zbuf; p.boxes = a->boxes; p.ids = a->ids;
  p.B = a->B; p.H = a->H; p.W = a->W; p.K = a->K; p.source = a->source;
  p.depth_scale = a->depth_scale; p.bg_near = a->bg_near; p.bg_far = a->bg_far;
  p.z_near = a->z_near; p.z_far = a->z_far; p.label = a->label; p.depth = a->depth;
  const bool vec4 = (hw & 3) == 0 && aligned16(a->zbuf) && aligned16(a->z_near) && aligned16(a->z_far) && aligned16(a->label) && aligned16(a->depth);
  if (vec4) {
    hipLaunchKernelGGL(scene_bounds_kernel<4>, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
  } else {
    hipLaunchKernelGGL(scene_bounds_kernel<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
  }
  return tp::check_launch("tp_scene_bounds");
}
