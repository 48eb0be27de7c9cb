// K42 tp_robust_weight: IRLS weights (Tukey, Huber) of a photometric residual, scaled per image by the exact lower median of the mean
// squared colour error q (the public function is ops.robust_weight in texpose_amd/ops/scene.py, the rule in
// include/texpose_amd.h).  The median is a three-level radix select on the bit patterns of q >= 0 (11 + 11 + 10 bits):
//
//   robust_clear    grid B x 256: zeroes the image's three histograms and its state; with scale_in it writes count = 0, median_q = 0 and
//                   the scale instead (no histogram is used).
//   robust_count    grid (ceil(H * W / 1024), B) x 256, four consecutive pixels per thread, one launch per LEVEL.  Level 0 forms q from
//                   model, image and weight and stores its bits (all ones: not counted) in the workspace; levels 1 and 2 read them back.
//                   A key that carries the prefix found so far adds one to the bin of its next digit in the workgroup's LDS histogram;
//                   the non-zero bins go to the image's histogram with integer atomics.
//   robust_search   grid B x 256, after every count: a scan over the histogram finds the bin that holds the rank, extends the prefix and
//                   reduces the rank.  Level 0 also takes n (the histogram's total) and sets rank = (n - 1) / 2; level 2 ends with the
//                   median's bits and writes median_q, scale, count and s2.
//   robust_apply    grid as robust_count: the weight from q (the stored bits, or formed here with scale_in) and s2.
// Integer atomics only: every output is a function of the inputs alone.  The image index is uniform per workgroup.
#include "tp_common.h"
#include <math.h>

namespace {
constexpr int kRwBlock = 256, kRwPix = 4, kRwTile = kRwBlock * kRwPix;
constexpr int kRwBits[3] = {11, 11, 10};
constexpr int kRwShift[3] = {21, 10, 0};
constexpr int kRwHistWords = (1 << 11) + (1 << 11) + (1 << 10);                // per image: 5120 counters
constexpr int kRwHistAt[3] = {0, 1 << 11, 2 << 11};
constexpr uint32_t kRwOff = 0xFFFFFFFFu;                                        // the key of a pixel that is not counted (q >= 0: never a key)

struct RwState {                                                               // per image, 32 bytes
  uint32_t prefix;           // the bits found so far (right-aligned)
  uint32_t rank;             // the rank that is left inside the prefix's bin
  uint32_t n;                // counted pixels
  uint32_t pad;
  double s2;                 // after level 2: the squared scale
  double pad2;
};

__host__ __device__ inline int64_t rw_tiles(int64_t n) { return (n + kRwTile - 1) / kRwTile; }
inline size_t rw_keys_bytes(int B, int H, int W) { return ((size_t)B * (size_t)H * (size_t)W * 4 + 15) & ~(size_t)15; }
size_t robust_workspace_bytes(int B, int H, int W) {                           // keys | histograms | state
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return rw_keys_bytes(B, H, W) + (size_t)B * (kRwHistWords * 4 + sizeof(RwState));
}

struct RwSpace { uint32_t* keys; uint32_t* hist; RwState* state; };
inline RwSpace rw_space(const tp_robust_weight_args& a) {
  char* base = static_cast<char*>(a.workspace);
  RwSpace s;
  s.keys = reinterpret_cast<uint32_t*>(base);
  s.hist = reinterpret_cast<uint32_t*>(base + rw_keys_bytes(a.B, a.H, a.W));
  s.state = reinterpret_cast<RwState*>(s.hist + (size_t)a.B * kRwHistWords);
  return s;
}

__device__ __forceinline__ double rw_s2(double sq, float sigma_min) { return fmax(sq, (double)sigma_min * (double)sigma_min); }

// the key of one pixel: the bits of q where it is counted, kRwOff elsewhere (rule 1 and 2 of the header)
__device__ __forceinline__ uint32_t rw_key(float base, const float* m, const float* o) {
  if (!(isfinite(base) && base > 0.f)) return kRwOff;
  if (!(isfinite(m[0]) && isfinite(m[1]) && isfinite(m[2]) && isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]))) return kRwOff;
  const double e0 = (double)o[0] - (double)m[0], e1 = (double)o[1] - (double)m[1], e2 = (double)o[2] - (double)m[2];
  const float q = (float)(((e0 * e0 + e1 * e1) + e2 * e2) / 3.0);
  return isfinite(q) ? __float_as_uint(q) : kRwOff;
}

// the four keys of a thread's pixels from p0 on (kRwOff past the plane), formed from the planes
template <bool VEC>
__device__ __forceinline__ void rw_form_keys(const float* pm, const float* po, const float* pw, int64_t p0, int64_t plane, uint32_t (&key)[kRwPix]) {
  float ws[kRwPix], ms[kRwPix * 3], os[kRwPix * 3];
#pragma unroll
  for (int k = 0; k < kRwPix; ++k) ws[k] = 1.f;
  if constexpr (VEC) {                                                         // (plane % 4 == 0: the four are inside together)
    if (pw) { const float4 w = *reinterpret_cast<const float4*>(pw + p0); ws[0] = w.x; ws[1] = w.y; ws[2] = w.z; ws[3] = w.w; }
    const float4* m4 = reinterpret_cast<const float4*>(pm + p0 * 3);           // (p0 * 12 bytes: a multiple of 48)
    const float4* o4 = reinterpret_cast<const float4*>(po + p0 * 3);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float4 m = m4[q], o = o4[q];
      ms[4 * q] = m.x; ms[4 * q + 1] = m.y; ms[4 * q + 2] = m.z; ms[4 * q + 3] = m.w;
      os[4 * q] = o.x; os[4 * q + 1] = o.y; os[4 * q + 2] = o.z; os[4 * q + 3] = o.w;
    }
#pragma unroll
    for (int k = 0; k < kRwPix; ++k) key[k] = rw_key(ws[k], ms + 3 * k, os + 3 * k);
  } else {
#pragma unroll
    for (int k = 0; k < kRwPix; ++k) {
      key[k] = kRwOff;
      if (p0 + k < plane) {
        if (pw) ws[k] = pw[p0 + k];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { ms[3 * k + ch] = pm[(p0 + k) * 3 + ch]; os[3 * k + ch] = po[(p0 + k) * 3 + ch]; }
        key[k] = rw_key(ws[k], ms + 3 * k, os + 3 * k);
      }
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void rw_load_keys(const uint32_t* pk, int64_t p0, int64_t plane, uint32_t (&key)[kRwPix]) {
  if constexpr (VEC) {
    const uint4 v = *reinterpret_cast<const uint4*>(pk + p0);
    key[0] = v.x; key[1] = v.y; key[2] = v.z; key[3] = v.w;
  } else {
#pragma unroll
    for (int k = 0; k < kRwPix; ++k) key[k] = p0 + k < plane ? pk[p0 + k] : kRwOff;
  }
}

// grid B: the image's histograms and state to zero; DIRECT (scale_in given): the outputs that no later launch writes
template <bool DIRECT>
__global__ __launch_bounds__(kRwBlock) void robust_clear_kernel(tp_robust_weight_args a, uint32_t* hist, RwState* state) {
  const int b = blockIdx.x;
  if constexpr (DIRECT) {
    if (threadIdx.x == 0) {
      const double s = (double)a.scale_in[b];
      a.count[b] = 0;
      a.median_q[b] = 0.f;
      a.scale[b] = (float)sqrt(rw_s2(s * s, a.sigma_min));
    }
  } else {
    uint32_t* h = hist + (size_t)b * kRwHistWords;
    for (int i = threadIdx.x; i < kRwHistWords; i += kRwBlock) h[i] = 0u;
    if (threadIdx.x == 0) { RwState s = {0u, 0u, 0u, 0u, 0.0, 0.0}; state[b] = s; }
  }
}

// one level of the select: LEVEL 0 forms the keys and stores them, the others read them; keys under the prefix count their next digit
template <int LEVEL, bool VEC>
__global__ __launch_bounds__(kRwBlock) void robust_count_kernel(tp_robust_weight_args a, uint32_t* keys, uint32_t* hist, const RwState* state) {
  constexpr int kBits = kRwBits[LEVEL], kShift = kRwShift[LEVEL], kBins = 1 << kBits;
  __shared__ uint32_t bins[kBins];
  const int b = blockIdx.y;
  const int64_t plane = (int64_t)a.H * a.W;
  const int64_t p0 = (int64_t)blockIdx.x * kRwTile + (int)threadIdx.x * kRwPix;   // (< H * W + 1024 < 2^31 + 1024)
  uint32_t* pk = keys + (int64_t)b * plane;
  for (int i = threadIdx.x; i < kBins; i += kRwBlock) bins[i] = 0u;
  __syncthreads();
  uint32_t key[kRwPix] = {kRwOff, kRwOff, kRwOff, kRwOff};
  if (p0 < plane) {
    if constexpr (LEVEL == 0) {
      rw_form_keys<VEC>(a.model + (int64_t)b * plane * 3, a.image + (int64_t)b * plane * 3, a.weight ? a.weight + (int64_t)b * plane : nullptr, p0,
                        plane, key);
      if constexpr (VEC) {
        *reinterpret_cast<uint4*>(pk + p0) = make_uint4(key[0], key[1], key[2], key[3]);
      } else {
#pragma unroll
        for (int k = 0; k < kRwPix; ++k)
          if (p0 + k < plane) pk[p0 + k] = key[k];
      }
    } else {
      rw_load_keys<VEC>(pk, p0, plane, key);
    }
  }
  const uint32_t prefix = LEVEL == 0 ? 0u : state[b].prefix;                    // (wave-uniform)
#pragma unroll
  for (int k = 0; k < kRwPix; ++k) {
    if (key[k] == kRwOff) continue;
    if (LEVEL > 0 && (key[k] >> (kShift + kBits)) != prefix) continue;
    atomicAdd(&bins[(key[k] >> kShift) & (kBins - 1)], 1u);
  }
  __syncthreads();
  constexpr int kAt = kRwHistAt[LEVEL];
  uint32_t* h = hist + (size_t)b * kRwHistWords + kAt;
  for (int i = threadIdx.x; i < kBins; i += kRwBlock) {
    const uint32_t c = bins[i];
    if (c) atomicAdd(h + i, c);
  }
}

// grid B x 256: the bin of the level's histogram that holds the rank.  Thread t owns kBins / 256 consecutive bins; an inclusive scan of
// the threads' totals in LDS; the one thread whose span holds the rank walks its bins.
template <int LEVEL>
__global__ __launch_bounds__(kRwBlock) void robust_search_kernel(tp_robust_weight_args a, const uint32_t* hist, RwState* state) {
  constexpr int kBits = kRwBits[LEVEL], kAt = kRwHistAt[LEVEL], kBins = 1 << kBits, kOwn = kBins / kRwBlock;
  __shared__ uint32_t scan[2][kRwBlock];
  const int b = blockIdx.x, t = threadIdx.x;
  const uint32_t* h = hist + (size_t)b * kRwHistWords + kAt + t * kOwn;
  uint32_t own[kOwn], total = 0u;
#pragma unroll
  for (int i = 0; i < kOwn; ++i) { own[i] = h[i]; total += own[i]; }
  scan[0][t] = total;
  __syncthreads();
  int cur = 0;
#pragma unroll
  for (int d = 1; d < kRwBlock; d <<= 1) {                                      // Hillis-Steele, double-buffered
    scan[cur ^ 1][t] = scan[cur][t] + (t >= d ? scan[cur][t - d] : 0u);
    cur ^= 1;
    __syncthreads();
  }
  const uint32_t upto = scan[cur][t], before = upto - total, n_level = scan[cur][kRwBlock - 1];
  const RwState s = state[b];                                                   // (read by every thread before the one below writes)
  __syncthreads();
  const uint32_t n = LEVEL == 0 ? n_level : s.n;
  const uint32_t rank = LEVEL == 0 ? (n ? (n - 1u) / 2u : 0u) : s.rank;
  if (n == 0u || n_level == 0u) {                                               // no counted pixel: the median is 0
    if (t == 0) {
      if constexpr (LEVEL == 0) { state[b].n = 0u; }
      if constexpr (LEVEL == 2) {
        const double s2 = rw_s2(0.0, a.sigma_min);
        state[b].s2 = s2;
        a.median_q[b] = 0.f; a.scale[b] = (float)sqrt(s2); a.count[b] = 0;
      }
    }
    return;
  }
  if (rank >= before && rank < upto) {                                          // exactly one thread: rank < n_level
    uint32_t acc = before;
    int bin = 0;
#pragma unroll
    for (int i = 0; i < kOwn; ++i) {
      if (rank >= acc + own[i]) { acc += own[i]; bin = i + 1; }
      else break;
    }
    const uint32_t prefix = ((LEVEL == 0 ? 0u : s.prefix) << kBits) | (uint32_t)(t * kOwn + bin);
    state[b].prefix = prefix;
    state[b].rank = rank - acc;
    if constexpr (LEVEL == 0) state[b].n = n;
    if constexpr (LEVEL == 2) {
      const float med = __uint_as_float(prefix);
      const double s2 = rw_s2((1.4826 * 1.4826) * (double)med, a.sigma_min);
      state[b].s2 = s2;
      a.median_q[b] = med; a.scale[b] = (float)sqrt(s2); a.count[b] = (int32_t)n;
    }
  }
}

// rule 5 of the header
template <int KIND>
__device__ __forceinline__ float rw_weight(float base, uint32_t key, double denom) {
  if (key == kRwOff) return 0.f;
  const double u2 = (double)__uint_as_float(key) / denom;
  double w;
  if constexpr (KIND == TP_ROBUST_TUKEY) w = u2 < 1.0 ? (1.0 - u2) * (1.0 - u2) : 0.0;
  else w = u2 <= 1.0 ? 1.0 : 1.0 / sqrt(u2);
  return (float)((double)base * w);
}

// DIRECT (scale_in given): the keys are formed here and the image's count is added up; else they come from the workspace
template <int KIND, bool DIRECT, bool VEC>
__global__ __launch_bounds__(kRwBlock) void robust_apply_kernel(tp_robust_weight_args a, const uint32_t* keys, const RwState* state) {
  const int b = blockIdx.y;
  const int64_t plane = (int64_t)a.H * a.W;
  const int64_t p0 = (int64_t)blockIdx.x * kRwTile + (int)threadIdx.x * kRwPix;
  const float* pw = a.weight ? a.weight + (int64_t)b * plane : nullptr;
  float* pout = a.out + (int64_t)b * plane;
  double s2;
  if constexpr (DIRECT) { const double s = (double)a.scale_in[b]; s2 = rw_s2(s * s, a.sigma_min); }
  else s2 = state[b].s2;
  const double denom = ((double)a.c * (double)a.c) * s2;
  int counted = 0;
  if (p0 < plane) {
    uint32_t key[kRwPix];
    float ws[kRwPix] = {1.f, 1.f, 1.f, 1.f};
    if constexpr (DIRECT) rw_form_keys<VEC>(a.model + (int64_t)b * plane * 3, a.image + (int64_t)b * plane * 3, pw, p0, plane, key);
    else rw_load_keys<VEC>(keys + (int64_t)b * plane, p0, plane, key);
    if (pw) {
      if constexpr (VEC) { const float4 w = *reinterpret_cast<const float4*>(pw + p0); ws[0] = w.x; ws[1] = w.y; ws[2] = w.z; ws[3] = w.w; }
      else {
#pragma unroll
        for (int k = 0; k < kRwPix; ++k)
          if (p0 + k < plane) ws[k] = pw[p0 + k];
      }
    }
    float o[kRwPix];
#pragma unroll
    for (int k = 0; k < kRwPix; ++k) { o[k] = rw_weight<KIND>(ws[k], key[k], denom); counted += key[k] != kRwOff; }
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(pout + p0) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int k = 0; k < kRwPix; ++k)
        if (p0 + k < plane) pout[p0 + k] = o[k];
    }
  }
  if constexpr (DIRECT) {                                                       // (every thread of the workgroup arrives here)
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    if (counted) atomicAdd(&total, counted);
    __syncthreads();
    if (threadIdx.x == 0 && total) atomicAdd(a.count + b, total);
  }
}

struct Span { const void* p; size_t n; const char* name; };

bool robust_args_ok(const tp_robust_weight_args& a) {
  const char* who = "tp_robust_weight";
  if (a.B <= 0 || a.B > 65535 || a.H <= 0 || a.W <= 0 || (int64_t)a.H * a.W > 0x7FFFFFFFll) {
    tp::set_error("%s: bad sizes (B 1..65535, H > 0, W > 0, H * W < 2^31)", who);
    return false;
  }
  if (!a.model || !a.image || !a.out || !a.median_q || !a.scale || !a.count) { tp::set_error("%s: null pointer", who); return false; }
  if (a.kind != TP_ROBUST_TUKEY && a.kind != TP_ROBUST_HUBER) { tp::set_error("%s: unknown kind %d", who, a.kind); return false; }
  if (!(std::isfinite(a.c) && a.c > 0.f)) { tp::set_error("%s: c must be finite and > 0", who); return false; }
  if (!(std::isfinite(a.sigma_min) && a.sigma_min > 0.f)) { tp::set_error("%s: sigma_min must be finite and > 0", who); return false; }
  if (!a.scale_in && !a.workspace) { tp::set_error("%s: null pointer (a workspace is needed without scale_in)", who); return false; }
  if (!a.scale_in && ((uintptr_t)a.workspace & 15u)) { tp::set_error("%s: workspace must be 16-byte aligned", who); return false; }
  const size_t px = (size_t)a.B * (size_t)a.H * (size_t)a.W, planes = px * 3 * sizeof(float), per = (size_t)a.B * 4;
  const Span in[] = {{a.model, planes, "model"}, {a.image, planes, "image"}, {a.weight, px * 4, "weight"}, {a.scale_in, per, "scale_in"}};
  const Span out[] = {{a.out, px * 4, "out"},
                      {a.median_q, per, "median_q"},
                      {a.scale, per, "scale"},
                      {a.count, per, "count"},
                      {a.scale_in ? nullptr : a.workspace, robust_workspace_bytes(a.B, a.H, a.W), "workspace"}};
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

template <int LEVEL, bool VEC>
void robust_level(const tp_robust_weight_args& a, const RwSpace& s, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL((robust_count_kernel<LEVEL, VEC>), grid, dim3(kRwBlock), 0, st, a, s.keys, s.hist, (const RwState*)s.state);
  hipLaunchKernelGGL((robust_search_kernel<LEVEL>), dim3(a.B), dim3(kRwBlock), 0, st, a, (const uint32_t*)s.hist, s.state);
}

template <bool DIRECT, bool VEC>
void robust_apply(const tp_robust_weight_args& a, const RwSpace& s, dim3 grid, hipStream_t st) {
  if (a.kind == TP_ROBUST_TUKEY)
    hipLaunchKernelGGL((robust_apply_kernel<TP_ROBUST_TUKEY, DIRECT, VEC>), grid, dim3(kRwBlock), 0, st, a, (const uint32_t*)s.keys, (const RwState*)s.state);
  else
    hipLaunchKernelGGL((robust_apply_kernel<TP_ROBUST_HUBER, DIRECT, VEC>), grid, dim3(kRwBlock), 0, st, a, (const uint32_t*)s.keys, (const RwState*)s.state);
}

template <bool VEC>
void robust_launch_as(const tp_robust_weight_args& a, hipStream_t st) {
  const dim3 grid((unsigned)rw_tiles((int64_t)a.H * a.W), a.B);
  if (a.scale_in) {
    const RwSpace none = {nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(robust_clear_kernel<true>, dim3(a.B), dim3(kRwBlock), 0, st, a, (uint32_t*)nullptr, (RwState*)nullptr);
    robust_apply<true, VEC>(a, none, grid, st);
    return;
  }
  const RwSpace s = rw_space(a);
  hipLaunchKernelGGL(robust_clear_kernel<false>, dim3(a.B), dim3(kRwBlock), 0, st, a, s.hist, s.state);
  robust_level<0, VEC>(a, s, grid, st);
  robust_level<1, VEC>(a, s, grid, st);
  robust_level<2, VEC>(a, s, grid, st);
  robust_apply<false, VEC>(a, s, grid, st);
}

void robust_launch(const tp_robust_weight_args& a, hipStream_t st) {
  const int64_t plane = (int64_t)a.H * a.W;                                     // (the keys of image b start at 4 b H W bytes: aligned with the plane)
  const uintptr_t planes = (uintptr_t)a.model | (uintptr_t)a.image | (uintptr_t)a.weight | (uintptr_t)a.out;
  if (plane % kRwPix == 0 && (planes & 15u) == 0) robust_launch_as<true>(a, st);   // (a null pointer is aligned; so is the workspace)
  else robust_launch_as<false>(a, st);
}
}  // namespace

extern "C" size_t tp_robust_weight_workspace_bytes(int B, int H, int W) { return robust_workspace_bytes(B, H, W); }

extern "C" int tp_robust_weight(const tp_robust_weight_args* a, tp_stream_t stream) {
  if (!a) { tp::set_error("tp_robust_weight: null args"); return -1; }
  if (!robust_args_ok(*a)) return -1;
  robust_launch(*a, (hipStream_t)stream);
  return tp::check_launch("tp_robust_weight");
}
