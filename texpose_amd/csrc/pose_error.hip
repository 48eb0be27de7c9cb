// K24 / K25: pose-error metrics on the device (the public module is texpose_amd/pose_error.py).
//
// K24 tp_nn1: brute-force 1-nearest / 1-farthest neighbour in 3-D.  A workgroup of 256 threads owns 1,024 queries of one batch
//   element (four per thread, in registers, optionally mapped by the linear part of the batch element's affine A on the way in) and
//   walks the targets in tiles of TP_NN1_TILE staged in LDS as (x, y, z, -) quadruples, A's translation taken off them on the way.  In the inner loop every lane reads the SAME tile entry -- one
//   16-byte broadcast read, no bank conflicts -- and evaluates it against its four queries: three subtractions, a product, two fused
//   multiply-adds, a compare and two selects per pair, so the vector ALU and not the LDS sets the pace.  Where queries x batch give too
//   few workgroups the targets are split into slices over gridDim.z and the slices' winners meet in a 64-bit key per query (bits of
//   the non-negative d2, then the index) through integer atomic min / max: the result depends on neither grid shape nor arrival order.
//   The direct form dx*dx + dy*dy + dz*dz is used, never |q|^2 + |y|^2 - 2 q.y.
//   Tie and NaN rules without extra instructions: targets are visited in ascending index and a later one must be strictly better;
//   `nearest` compares the bit patterns of d2 as unsigned integers against a start value one above +inf's pattern, so every NaN
//   (pattern above +inf's, or with the sign bit) loses and +inf itself can still win; `farthest` compares floats against -inf, which
//   a NaN never beats.  Queries past x_len (or NaN) are NaN in registers, tile entries past y_len are NaN in LDS: no bounds test
//   inside the loop.
//
// K25 tp_pose_errors: ADD, MSSD, MSPD and the mean projection error.  One workgroup owns one (pose pair b, symmetry s), composes
//   P_g S_s once and walks the M model points in a fixed order; everything between the fp32 inputs and the fp32 outputs is fp64
//   (the reason is K23's: a bar with a one-ulp floor at M = B = 1 is met by a correctly rounded result only), reduced by a fixed tree:
//   per thread in point order, down the wavefront, over the four wavefronts in order.  A second tiny launch takes the minimum over s
//   (lowest index on ties) from the [B,S,4] workspace.  No atomics at all, bit-identical from run to run and under graph replay.
#include "tp_common.h"

namespace {
// ------------------------------------------------------------------------------------------ K24
constexpr int kBlock = 256, kQ = 4, kTile = TP_NN1_TILE, kUnroll = 4;
static_assert(kBlock * kQ == TP_NN1_QUERIES_PER_BLOCK, "the header publishes the queries a workgroup owns");
static_assert(kTile % kBlock == 0 && kTile % kUnroll == 0, "a tile is staged in whole rounds of the workgroup and walked in whole unrolled steps");
constexpr uint32_t kInfBits = 0x7F800000u;
constexpr uint32_t kNearStart = kInfBits + 1u;             // every non-NaN d2 >= 0 has a smaller pattern, every NaN a larger or equal one
constexpr unsigned long long kNearNone = ~0ull, kFarNone = 0ull;      // keys no candidate can have (index < 2^31)

__device__ __forceinline__ int clamp_len(const int32_t* len, int i, int P) {
  if (!len) return P;
  const int v = len[i];
  return v < 0 ? 0 : (v > P ? P : v);
}

template <bool FAR>
__device__ __forceinline__ void decode(unsigned long long key, float& d2, int32_t& idx) {
  if (key == (FAR ? kFarNone : kNearNone)) {
    d2 = FAR ? -INFINITY : INFINITY;
    idx = -1;
  } else {
    d2 = __uint_as_float((uint32_t)(key >> 32));
    idx = (int32_t)(FAR ? 0xFFFFFFFFu - (uint32_t)key : (uint32_t)key);
  }
}

__global__ __launch_bounds__(kBlock) void nn1_init_kernel(unsigned long long* keys, int64_t n, unsigned long long value) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) keys[i] = value;
}

template <bool FAR>
__global__ __launch_bounds__(kBlock) void nn1_decode_kernel(const unsigned long long* keys, int64_t n, float* d2, int32_t* idx) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i < n) decode<FAR>(keys[i], d2[i], idx[i]);
}

// grid (query tiles, B, slices); SPLIT: the winners go to keys [B,P1] by atomic min / max, else straight to d2 / idx
template <bool FAR, bool SPLIT>
__global__ __launch_bounds__(kBlock) void nn1_kernel(tp_nn1_args a, int tiles_per_slice, unsigned long long* keys) {
  __shared__ float4 tile[kTile];
  const int b = blockIdx.y, bt = a.Bt == 1 ? 0 : b;
  const int x_len = clamp_len(a.x_len, b, a.P1), y_len = clamp_len(a.y_len, bt, a.P2);
  const int64_t i0 = (int64_t)blockIdx.x * (kBlock * kQ) + threadIdx.x;          // this thread's queries: i0 + k * kBlock
  float qx[kQ], qy[kQ], qz[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    const int64_t i = i0 + k * kBlock;
    qx[k] = qy[k] = qz[k] = NAN;
    if (i < x_len) {
      const float* p = a.x + ((int64_t)(a.Bx == 1 ? 0 : b) * a.P1 + i) * 3;
      const float x = p[0], y = p[1], z = p[2];
      if (a.A) {
        // the linear part of A in fp64, rounded once; the translation is taken off the targets instead (below): the mapped cloud
        // exists in these registers only
        const float* A = a.A + (int64_t)b * 12;
        float q[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
          q[r] = (float)__fma_rn((double)A[4 * r], (double)x, __fma_rn((double)A[4 * r + 1], (double)y, (double)A[4 * r + 2] * (double)z));
        qx[k] = q[0]; qy[k] = q[1]; qz[k] = q[2];
      } else {
        qx[k] = x; qy[k] = y; qz[k] = z;
      }
    }
  }
  uint32_t best_bits[kQ];
  float best[kQ];
  int32_t best_idx[kQ];
#pragma unroll
  for (int k = 0; k < kQ; ++k) { best_bits[k] = kNearStart; best[k] = -INFINITY; best_idx[k] = -1; }

  const float* yb = a.y + (int64_t)bt * a.P2 * 3;
  // with A the comparison happens in the frame before A's translation t: (A3 x + t) - y = A3 x - (y - t).  Both sides are then of
  // the model's size, not of the camera distance, and the fp32 roundings of q and of the differences shrink with them
  float tx = 0.f, ty = 0.f, tz = 0.f;
  if (a.A) { const float* A = a.A + (int64_t)b * 12; tx = A[3]; ty = A[7]; tz = A[11]; }
  const int tile_first = blockIdx.z * tiles_per_slice;
  for (int t = tile_first; t < tile_first + tiles_per_slice; ++t) {
    const int64_t j0 = (int64_t)t * kTile;
    if (j0 >= y_len) break;                                  // (uniform: y_len and t are the same in every lane)
    __syncthreads();                                         // the previous tile has been read by every wavefront
#pragma unroll
    for (int m = 0; m < kTile / kBlock; ++m) {
      const int l = m * kBlock + threadIdx.x;
      const int64_t j = j0 + l;
      float4 v = make_float4(NAN, NAN, NAN, 0.f);
      if (j < y_len) { const float* p = yb + j * 3; v = make_float4(p[0] - tx, p[1] - ty, p[2] - tz, 0.f); }
      tile[l] = v;
    }
    __syncthreads();
    const int64_t left = (int64_t)y_len - j0;
    const int n = left < kTile ? (int)((left + kUnroll - 1) / kUnroll * kUnroll) : kTile;      // (the NaN entries past y_len lose)
    for (int j = 0; j < n; j += kUnroll) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const float4 v = tile[j + u];
        const int32_t idx = (int32_t)j0 + j + u;
#pragma unroll
        for (int k = 0; k < kQ; ++k) {
          const float dx = qx[k] - v.x, dy = qy[k] - v.y, dz = qz[k] - v.z;
          const float d2 = __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, dx * dx));
          if constexpr (FAR) {
            const bool win = d2 > best[k];
            best[k] = win ? d2 : best[k];
            best_idx[k] = win ? idx : best_idx[k];
          } else {
            const uint32_t bits = __float_as_uint(d2);
            const bool win = bits < best_bits[k];
            best_bits[k] = win ? bits : best_bits[k];
            best_idx[k] = win ? idx : best_idx[k];
          }
        }
      }
    }
  }

#pragma unroll
  for (int k = 0; k < kQ; ++k) {
    const int64_t i = i0 + k * kBlock;
    if (i >= a.P1) continue;
    const int64_t o = (int64_t)b * a.P1 + i;
    const uint32_t bits = FAR ? __float_as_uint(best[k]) : best_bits[k];
    if constexpr (SPLIT) {
      if (best_idx[k] < 0) continue;                         // (the initial key already says "no winner")
      const unsigned long long key = ((unsigned long long)bits << 32) | (FAR ? 0xFFFFFFFFu - (uint32_t)best_idx[k] : (uint32_t)best_idx[k]);
      if constexpr (FAR) __hip_atomic_fetch_max(keys + o, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else __hip_atomic_fetch_min(keys + o, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      const bool none = best_idx[k] < 0;
      a.d2[o] = none ? (FAR ? -INFINITY : INFINITY) : __uint_as_float(bits);
      a.idx[o] = best_idx[k];
    }
  }
}

struct Nn1Plan { int q_tiles, tiles, slices, tiles_per_slice; };

// the grid of a call, a function of the shapes and args.target_slices alone
int nn1_plan(const tp_nn1_args* a, Nn1Plan* p, const char* what) {
  if (!a) { tp::set_error("%s: null args", what); return -1; }
  if (a->B <= 0 || a->B > 65535 || a->P1 <= 0 || a->P2 <= 0 || (a->Bt != 1 && a->Bt != a->B) || (a->Bx != 1 && a->Bx != a->B)) {
    tp::set_error("%s: bad sizes (B 1..65535, P1 > 0, P2 > 0, Bx and Bt 1 or B)", what);
    return -1;
  }
  if (a->mode != TP_NN1_NEAREST && a->mode != TP_NN1_FARTHEST) { tp::set_error("%s: bad mode", what); return -1; }
  if (a->target_slices < 0) { tp::set_error("%s: target_slices < 0", what); return -1; }
  p->q_tiles = (a->P1 + kBlock * kQ - 1) / (kBlock * kQ);
  p->tiles = (a->P2 + kTile - 1) / kTile;
  int want = a->target_slices;
  if (want == 0) {
    // enough workgroups to fill the 256 compute units a few times over, from the shapes alone
    const int64_t groups = (int64_t)p->q_tiles * a->B;
    want = groups >= 512 ? 1 : (int)((1024 + groups - 1) / groups);
  }
  if (want > p->tiles) want = p->tiles;
  if (want > 65535) want = 65535;
  p->tiles_per_slice = (p->tiles + want - 1) / want;
  p->slices = (p->tiles + p->tiles_per_slice - 1) / p->tiles_per_slice;
  return 0;
}

// ------------------------------------------------------------------------------------------ K25
constexpr int kPoseBlock = 256, kPoseWaves = kPoseBlock / tp::kWave;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = tp::kWave >> 1; o > 0; o >>= 1) v += __shfl_down(v, o, tp::kWave);
  return v;                                    // (lane 0 holds the total)
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = tp::kWave >> 1; o > 0; o >>= 1) { const double w = __shfl_down(v, o, tp::kWave); v = w > v ? w : v; }
  return v;
}

// grid (S, B): ws[b][s] = { sum_x |e - g|, max_x |e - g|, sum_x |pi(e) - pi(g)|, max_x |pi(e) - pi(g)| } with e = P_e x, g = P_g S_s x;
// the two pixel entries are NaN where a point has Z <= 0 (or NaN) under either pose
__global__ __launch_bounds__(kPoseBlock) void pose_errors_kernel(tp_pose_errors_args a, double* ws) {
  __shared__ double part[4][kPoseWaves];
  __shared__ int part_bad[kPoseWaves];
  const int s = blockIdx.x, b = blockIdx.y;
  double Pe[12], Pg[12], Ss[12], G[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    Pe[i] = (double)a.pose_est[(int64_t)b * 12 + i];
    Pg[i] = (double)a.pose_gt[(int64_t)b * 12 + i];
    Ss[i] = (double)a.sym[(int64_t)s * 12 + i];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double v = __fma_rn(Pg[4 * r], Ss[c], __fma_rn(Pg[4 * r + 1], Ss[4 + c], Pg[4 * r + 2] * Ss[8 + c]));
      if (c == 3) v += Pg[4 * r + 3];
      G[4 * r + c] = v;
    }
  }
  const bool pix = a.intr != nullptr;
  double fx = 0.0, fy = 0.0, cx = 0.0, cy = 0.0;
  if (pix) {
    const float* K = a.intr + (int64_t)b * 9;
    fx = (double)K[0]; cx = (double)K[2]; fy = (double)K[4]; cy = (double)K[5];
  }
  double sum3 = 0.0, max3 = 0.0, sum2 = 0.0, max2 = 0.0;
  int bad = 0;
  for (int i = threadIdx.x; i < a.M; i += kPoseBlock) {
    const float* p = a.pts + (int64_t)i * 3;
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    double e[3], g[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      e[r] = __fma_rn(Pe[4 * r], x, __fma_rn(Pe[4 * r + 1], y, __fma_rn(Pe[4 * r + 2], z, Pe[4 * r + 3])));
      g[r] = __fma_rn(G[4 * r], x, __fma_rn(G[4 * r + 1], y, __fma_rn(G[4 * r + 2], z, G[4 * r + 3])));
    }
    const double dx = e[0] - g[0], dy = e[1] - g[1], dz = e[2] - g[2];
    const double d3 = sqrt(__fma_rn(dz, dz, __fma_rn(dy, dy, dx * dx)));
    sum3 += d3;
    max3 = d3 > max3 ? d3 : max3;
    if (pix) {
      if (!(e[2] > 0.0) || !(g[2] > 0.0)) {
        bad = 1;
      } else {
        const double du = (__fma_rn(fx, e[0] / e[2], cx)) - (__fma_rn(fx, g[0] / g[2], cx));
        const double dv = (__fma_rn(fy, e[1] / e[2], cy)) - (__fma_rn(fy, g[1] / g[2], cy));
        const double d2 = sqrt(__fma_rn(dv, dv, du * du));
        sum2 += d2;
        max2 = d2 > max2 ? d2 : max2;
      }
    }
  }
  sum3 = wave_sum(sum3); max3 = wave_max(max3); sum2 = wave_sum(sum2); max2 = wave_max(max2);
  bad = __any(bad) ? 1 : 0;
  const int lane = threadIdx.x & (tp::kWave - 1), wave = threadIdx.x / tp::kWave;
  if (lane == 0) { part[0][wave] = sum3; part[1][wave] = max3; part[2][wave] = sum2; part[3][wave] = max2; part_bad[wave] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kPoseWaves; ++w) {
      sum3 += part[0][w]; max3 = part[1][w] > max3 ? part[1][w] : max3;
      sum2 += part[2][w]; max2 = part[3][w] > max2 ? part[3][w] : max2;
      bad |= part_bad[w];
    }
    double* o = ws + ((int64_t)b * a.S + s) * 4;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    o[0] = sum3; o[1] = max3; o[2] = bad ? nan : sum2; o[3] = bad ? nan : max2;
  }
}

// one thread per b: the minimum over s, lowest index on ties
__global__ __launch_bounds__(kPoseBlock) void pose_errors_min_kernel(tp_pose_errors_args a, const double* ws) {
  const int b = blockIdx.x * kPoseBlock + threadIdx.x;
  if (b >= a.B) return;
  const double* w = ws + (int64_t)b * a.S * 4;
  double best3 = w[1], best2 = w[3];
  int s3 = 0, s2 = 0;
  bool bad = best2 != best2;
  for (int s = 1; s < a.S; ++s) {
    const double m3 = w[4 * s + 1], m2 = w[4 * s + 3];
    if (m3 < best3) { best3 = m3; s3 = s; }
    if (m2 < best2) { best2 = m2; s2 = s; }
    bad = bad || m2 != m2;
  }
  a.out[(int64_t)b * 4] = (float)(w[0] / (double)a.M);
  a.out[(int64_t)b * 4 + 1] = (float)best3;
  a.s_mssd[b] = s3;
  if (a.intr) {
    a.out[(int64_t)b * 4 + 2] = bad ? NAN : (float)best2;
    a.out[(int64_t)b * 4 + 3] = bad ? NAN : (float)(w[2] / (double)a.M);
    a.s_mspd[b] = bad ? -1 : s2;
  }
}
}  // namespace

extern "C" size_t tp_nn1_workspace_bytes(const tp_nn1_args* a) {
  Nn1Plan p;
  if (nn1_plan(a, &p, "tp_nn1_workspace_bytes")) return 0;
  return p.slices > 1 ? (size_t)a->B * (size_t)a->P1 * sizeof(unsigned long long) : 0;
}

extern "C" int tp_nn1(const tp_nn1_args* a, tp_stream_t stream) {
  Nn1Plan p;
  if (int rc = nn1_plan(a, &p, "tp_nn1")) return rc;
  if (!a->x || !a->y || !a->d2 || !a->idx) { tp::set_error("tp_nn1: null pointer"); return -1; }
  const bool split = p.slices > 1, far = a->mode == TP_NN1_FARTHEST;
  if (split && !a->workspace) { tp::set_error("tp_nn1: %d target slices need args.workspace (tp_nn1_workspace_bytes)", p.slices); return -1; }
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* keys = (unsigned long long*)a->workspace;
  const int64_t n = (int64_t)a->B * a->P1;
  const dim3 flat((unsigned)((n + kBlock - 1) / kBlock)), grid(p.q_tiles, a->B, p.slices);
  if (split) hipLaunchKernelGGL(nn1_init_kernel, flat, dim3(kBlock), 0, st, keys, n, far ? kFarNone : kNearNone);
  if (far) {
    if (split) hipLaunchKernelGGL((nn1_kernel<true, true>), grid, dim3(kBlock), 0, st, *a, p.tiles_per_slice, keys);
    else hipLaunchKernelGGL((nn1_kernel<true, false>), grid, dim3(kBlock), 0, st, *a, p.tiles_per_slice, keys);
    if (split) hipLaunchKernelGGL(nn1_decode_kernel<true>, flat, dim3(kBlock), 0, st, keys, n, a->d2, a->idx);
  } else {
    if (split) hipLaunchKernelGGL((nn1_kernel<false, true>), grid, dim3(kBlock), 0, st, *a, p.tiles_per_slice, keys);
    else hipLaunchKernelGGL((nn1_kernel<false, false>), grid, dim3(kBlock), 0, st, *a, p.tiles_per_slice, keys);
    if (split) hipLaunchKernelGGL(nn1_decode_kernel<false>, flat, dim3(kBlock), 0, st, keys, n, a->d2, a->idx);
  }
  return tp::check_launch("tp_nn1");
}

extern "C" int tp_pose_errors(const tp_pose_errors_args* a, tp_stream_t stream) {
  if (!a || !a->pts || !a->pose_est || !a->pose_gt || !a->sym || !a->out || !a->s_mssd || !a->workspace) {
    tp::set_error("tp_pose_errors: null pointer");
    return -1;
  }
  if (a->intr && !a->s_mspd) { tp::set_error("tp_pose_errors: intr without s_mspd"); return -1; }
  if (a->M <= 0 || a->B <= 0 || a->B > 65535 || a->S <= 0) { tp::set_error("tp_pose_errors: bad sizes (M > 0, B 1..65535, S > 0)"); return -1; }
  if (a->S > TP_POSE_ERRORS_MAX_SYM) {
    tp::set_error("tp_pose_errors: %d symmetry transforms, at most %d (subsample them: pose_error.symmetry_transforms)", a->S, TP_POSE_ERRORS_MAX_SYM);
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pose_errors_kernel, dim3(a->S, a->B), dim3(kPoseBlock), 0, st, *a, (double*)a->workspace);
  hipLaunchKernelGGL(pose_errors_min_kernel, dim3((a->B + kPoseBlock - 1) / kPoseBlock), dim3(kPoseBlock), 0, st, *a, (const double*)a->workspace);
  return tp::check_launch("tp_pose_errors");
}
