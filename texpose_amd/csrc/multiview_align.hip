// K39 tp_multiview_align_step / tp_pose_compose: one Gauss-Newton step for ONE object pose per group of views with known cameras
// (the public functions are in texpose_amd/multiview.py, the rules in include/texpose_amd.h).
//
//   the terms     as in K33 (joint_align.hip): each present term runs its own launches (pose_terms.h) with evaluate_only set and no
//                 pose_out, at the composed poses T_i = C_i o M_group[i] the caller rendered at.
//   view_sums     grid B x 64.  Gathers each term's G records with gn_gather through one 16 KiB LDS stage and forms the weighted sums
//                 exactly as joint_solve_kernel does, then rewrites them for a world-frame increment: H' = A^T H A, g' = A^T g with
//                 A = [[Rc, 0], [[tc]x Rc, Rc]] in fp64 (a cam of exactly [I|0]: no transform, the sums bit for bit), and stores one
//                 32-double record per view.
//   group_solve   grid Gr x 64.  29 threads add the group's member records in ascending order, thread 0 applies gn_decide with the
//                 group's model pose as the current one.
//   compose       grid Gr x 64 over the members: pose_out[i] = cam[i] o model_out[g].
// Two stages because one wave per group gathering every tile record of every view would serialise views x tiles.  No atomics; every
// fp64 sum has one fixed order, so all outputs are a function of the inputs alone.  member and group_start are device arrays the host
// cannot check: every start, end and member index is clamped before it is used.
#include "tp_common.h"
#include "pose_gn.h"
#include "pose_terms.h"

namespace {
constexpr int kTerms = 3;                              // silhouette, photometric, depth: the order of the sum

struct ViewTerms {
  const double* part[kTerms];                          // the term's records [B,G,32], or null: absent or weight 0, not in the sum
  double w[kTerms];
};

// cam [12] is bit-exactly [I|0]: the words of 1.0f on the diagonal and of +0.0f elsewhere
__device__ __forceinline__ bool is_identity(const float* cam) {
  bool same = true;
#pragma unroll
  for (int k = 0; k < 12; ++k) same = same && __float_as_uint(cam[k]) == ((k == 0 || k == 5 || k == 10) ? 0x3f800000u : 0u);
  return same;
}

// out [12] = cam o model: fp64, every dot product left to right, + tc last, rounded once; a copy of model where cam is [I|0]
__device__ __forceinline__ void compose_one(const float* cam, const float* model, float* out) {
  if (is_identity(cam)) {
#pragma unroll
    for (int k = 0; k < 12; ++k) out[k] = model[k];
    return;
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double a = (double)cam[4 * r], b = (double)cam[4 * r + 1], c = (double)cam[4 * r + 2];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double v = (a * (double)model[k] + b * (double)model[4 + k]) + c * (double)model[8 + k];
      if (k == 3) v = v + (double)cam[4 * r + 3];
      out[4 * r + k] = (float)v;
    }
  }
}

__device__ __forceinline__ int clamped(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(tp::kWave) void pose_compose_kernel(tp_pose_compose_args a) {
  const int i = blockIdx.x * tp::kWave + threadIdx.x;
  if (i >= a.B) return;
  const int g = clamped(a.group[i], 0, a.Gr - 1);
  compose_one(a.cam + (int64_t)i * 12, a.model + (int64_t)g * 12, a.out + (int64_t)i * 12);
}

// entry (r, c) of A = [[Rc, 0], [[tc]x Rc, Rc]] from the fp32 cam [12]
__device__ __forceinline__ double a_entry(const float* cam, int r, int c) {
  const int rr = r % 3, cc = c % 3;
  if (r < 3) return c < 3 ? (double)cam[4 * rr + cc] : 0.0;
  if (c >= 3) return (double)cam[4 * rr + cc];
  const double tx = (double)cam[3], ty = (double)cam[7], tz = (double)cam[11];
  const double r0 = (double)cam[cc], r1 = (double)cam[4 + cc], r2 = (double)cam[8 + cc];
  if (rr == 0) return (-tz) * r1 + ty * r2;
  if (rr == 1) return tz * r0 + (-tx) * r2;
  return (-ty) * r0 + tx * r1;
}

__global__ __launch_bounds__(tp::kWave) void view_sums_kernel(tp_multiview_args mv, ViewTerms t, int G, double* record) {
  __shared__ double sum[kGnPart], term[kGnPart], stage[kGnStage][kGnPart];
  __shared__ double A[6][6], Hm[6][6], P[6][6];
  const int b = blockIdx.x, k = threadIdx.x;
  double s = 0.0;                                                                // thread k < 29: sum[k], as joint_solve_kernel forms it
  bool first = true;
  for (int i = 0; i < kTerms; ++i) {                                             // (uniform: t is a kernel argument)
    if (!t.part[i]) continue;
    gn_gather(t.part[i] + (int64_t)b * G * kGnPart, G, stage, term);
    if (k < kGnSums) {
      const double v = k < kGnSums - 1 ? t.w[i] * term[k] : term[k];             // (the count is not weighted)
      s = first ? v : s + v;
    }
    first = false;
    __syncthreads();                                                             // term is free for the next gather
  }
  double* out = record + (int64_t)b * kGnPart;
  const float* cam = mv.cam + (int64_t)b * 12;
  if (is_identity(cam)) {                                                        // (uniform per block) no transform: the sums bit for bit
    if (k < kGnPart) out[k] = k < kGnSums ? s : 0.0;
    return;
  }
  if (k < kGnSums) sum[k] = s;
  if (k < 36) A[k / 6][k % 6] = a_entry(cam, k / 6, k % 6);
  __syncthreads();
  if (k < 36) {                                                                  // the 21 sums as the full symmetric matrix
    const int r = k / 6, c = k % 6, lo = r < c ? r : c, hi = r < c ? c : r;
    Hm[r][c] = sum[lo * 6 - lo * (lo - 1) / 2 + (hi - lo)];
  }
  __syncthreads();
  if (k < 36) {                                                                  // P = H A, the inner index ascending
    const int r = k / 6, c = k % 6;
    double v = Hm[r][0] * A[0][c];
    for (int m = 1; m < 6; ++m) v = v + Hm[r][m] * A[m][c];
    P[r][c] = v;
  }
  __syncthreads();
  double v = 0.0;
  if (k < 36) {                                                                  // Q = A^T P; its upper triangle is kept
    const int r = k / 6, c = k % 6;
    v = A[0][r] * P[0][c];
    for (int m = 1; m < 6; ++m) v = v + A[m][r] * P[m][c];
    if (c >= r) out[r * 6 - r * (r - 1) / 2 + (c - r)] = v;
  } else if (k < 42) {                                                           // g' = A^T g
    const int r = k - 36;
    v = A[0][r] * sum[21];
    for (int m = 1; m < 6; ++m) v = v + A[m][r] * sum[21 + m];
    out[21 + r] = v;
  } else if (k < 44) {
    out[27 + (k - 42)] = sum[27 + (k - 42)];                                     // chi2 and the count unchanged
  } else if (k < 47) {
    out[29 + (k - 44)] = 0.0;
  }
}

__global__ __launch_bounds__(tp::kWave) void group_solve_kernel(tp_multiview_args mv, const double* record) {
  __shared__ double sum[kGnPart];
  const int g = blockIdx.x, k = threadIdx.x;
  const int start = clamped(mv.group_start[g], 0, mv.B), end = clamped(mv.group_start[g + 1], start, mv.B);
  if (k < kGnSums) {
    double s = 0.0;                                                              // (a group without members: zeros, status 1)
    int seen = 0;
    for (int m = start; m < end; ++m) {
      const int i = clamped(mv.member[m], 0, mv.B - 1);
      const double v = record[(int64_t)i * kGnPart + k];
      s = m == start ? v : s + v;                                                // the first record is assigned
      seen += v > 0.0 ? 1 : 0;
    }
    sum[k] = s;
    if (k == kGnSums - 1) mv.views[g] = seen;                                    // (thread 28 reads the counts)
  }
  __syncthreads();
  if (k != 0) return;
  float out[12];
  const int status = gn_decide(sum, mv.model + (int64_t)g * 12, (double)mv.damping, mv.evaluate_only != 0, out);
  mv.inliers[g] = (int)sum[28];
  mv.chi2[g] = (float)sum[27];
  mv.status[g] = status;
  if (mv.model_out)
    for (int e = 0; e < 12; ++e) mv.model_out[(int64_t)g * 12 + e] = out[e];
}

__global__ __launch_bounds__(tp::kWave) void member_compose_kernel(tp_multiview_args mv, const float* model) {
  const int g = blockIdx.x;
  const int start = clamped(mv.group_start[g], 0, mv.B), end = clamped(mv.group_start[g + 1], start, mv.B);
  for (int m = start + (int)threadIdx.x; m < end; m += tp::kWave) {
    const int i = clamped(mv.member[m], 0, mv.B - 1);
    compose_one(mv.cam + (int64_t)i * 12, model + (int64_t)g * 12, mv.pose_out + (int64_t)i * 12);
  }
}

// what the step needs to know of a term, whichever struct it is
struct TermView {
  const char* name;
  bool present;
  float w;
  int B, H, W;
  const float *pose, *intr;
  void* workspace;
};

template <class Args>
TermView view_of(const char* name, const Args* a, float w) {
  if (!a) return {name, false, w, 0, 0, 0, nullptr, nullptr, nullptr};
  return {name, true, w, a->B, a->H, a->W, a->pose, a->intr, a->workspace};
}

// the term as the step runs it: evaluating, writing no pose
template <class Args>
Args evaluating(const Args* a) {
  Args e = *a;
  e.evaluate_only = 1;
  e.pose_out = nullptr;
  return e;
}

bool overlap(const void* p, size_t np, const void* q, size_t nq) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + nq && b < a + np;
}
}  // namespace

extern "C" int tp_pose_compose(const tp_pose_compose_args* a, tp_stream_t stream) {
  const char* who = "tp_pose_compose";
  if (!a) { tp::set_error("%s: null args", who); return -1; }
  if (!a->cam || !a->model || !a->group || !a->out) { tp::set_error("%s: null pointer", who); return -1; }
  if (a->B <= 0 || a->B > (1 << 24) || a->Gr <= 0) { tp::set_error("%s: bad sizes (B 1..2^24, Gr >= 1)", who); return -1; }
  const size_t views = (size_t)a->B * 12 * sizeof(float), models = (size_t)a->Gr * 12 * sizeof(float);
  if (overlap(a->out, views, a->cam, views) || overlap(a->out, views, a->model, models)) {
    tp::set_error("%s: out must not overlap cam or model", who);
    return -1;
  }
  hipLaunchKernelGGL(pose_compose_kernel, dim3((a->B + tp::kWave - 1) / tp::kWave), dim3(tp::kWave), 0, (hipStream_t)stream, *a);
  return tp::check_launch(who);
}

extern "C" size_t tp_multiview_workspace_bytes(int B) { return B <= 0 ? 0 : (size_t)B * kGnPart * sizeof(double); }

extern "C" int tp_multiview_align_step(const tp_multiview_args* mv, const tp_silhouette_align_args* sil, const tp_photo_align_args* photo,
                                       const tp_depth_icp_args* icp, tp_stream_t stream) {
  const char* who = "tp_multiview_align_step";
  if (!mv) { tp::set_error("%s: null args", who); return -1; }
  const TermView v[kTerms] = {view_of("silhouette", sil, mv->w_sil), view_of("photo", photo, mv->w_photo), view_of("icp", icp, mv->w_icp)};
  bool any = false, weighted = false;
  for (const TermView& t : v) {
    if (!(t.w >= 0.f) || !isfinite(t.w)) { tp::set_error("%s: the %s weight must be finite and not negative", who, t.name); return -1; }
    any = any || t.present;
    weighted = weighted || (t.present && t.w > 0.f);
  }
  if (!any) { tp::set_error("%s: no term is present", who); return -1; }
  if (!weighted) { tp::set_error("%s: no present term has a weight > 0", who); return -1; }
  if (!(mv->damping >= 0.f) || !isfinite(mv->damping)) { tp::set_error("%s: damping must be finite and not negative", who); return -1; }
  if (!mv->cam || !mv->pose || !mv->model || !mv->member || !mv->group_start || !mv->status || !mv->inliers || !mv->chi2 || !mv->views ||
      !mv->workspace || (!mv->model_out && !mv->evaluate_only)) {
    tp::set_error("%s: null pointer", who);
    return -1;
  }
  if (mv->B <= 0 || mv->B > 65535) { tp::set_error("%s: bad sizes (B 1..65535)", who); return -1; }
  if (mv->Gr <= 0 || mv->Gr > mv->B) { tp::set_error("%s: bad sizes (Gr 1..B = %d, got %d)", who, mv->B, mv->Gr); return -1; }
  if ((uintptr_t)mv->workspace & 15u) { tp::set_error("%s: workspace must be 16-byte aligned", who); return -1; }
  const size_t views = (size_t)mv->B * 12 * sizeof(float), models = (size_t)mv->Gr * 12 * sizeof(float);
  if (mv->model_out && overlap(mv->model_out, models, mv->model, models)) { tp::set_error("%s: model_out must not overlap model", who); return -1; }
  if (mv->pose_out && (overlap(mv->pose_out, views, mv->pose, views) || overlap(mv->pose_out, views, mv->cam, views))) {
    tp::set_error("%s: pose_out must not overlap pose or cam", who);
    return -1;
  }
  // every term's own refusals, on the term as it will run
  tp_silhouette_align_args es;
  tp_photo_align_args ep;
  tp_depth_icp_args ei;
  if (sil) { es = evaluating(sil); if (!tp::silhouette_align_args_ok(es)) return -1; }
  if (photo) { ep = evaluating(photo); if (!tp::photo_align_args_ok(ep)) return -1; }
  if (icp) { ei = evaluating(icp); if (!tp::depth_icp_args_ok(ei)) return -1; }
  // one batch, one pose, one camera, one image size; a workspace each
  const TermView* ref = nullptr;
  for (const TermView& t : v) {
    if (!t.present) continue;
    if (t.B != mv->B) { tp::set_error("%s: the %s term's B = %d differs from args' B = %d", who, t.name, t.B, mv->B); return -1; }
    if (t.pose != mv->pose) { tp::set_error("%s: the %s term's pose differs from args' pose", who, t.name); return -1; }
    if (!ref) { ref = &t; continue; }
    if (t.H != ref->H || t.W != ref->W) {
      tp::set_error("%s: the %s term is %d x %d, the %s term %d x %d", who, t.name, t.H, t.W, ref->name, ref->H, ref->W);
      return -1;
    }
    if (t.intr != ref->intr) { tp::set_error("%s: the %s term's intr differs from the %s term's", who, t.name, ref->name); return -1; }
  }
  const int G = (int)gn_tiles((int64_t)ref->H * ref->W);
  const size_t ws_bytes = gn_workspace_bytes(mv->B, G), own_bytes = tp_multiview_workspace_bytes(mv->B);
  for (int a = 0; a < kTerms; ++a) {
    if (!v[a].present) continue;
    if (overlap(mv->workspace, own_bytes, v[a].workspace, ws_bytes)) {
      tp::set_error("%s: the multi-view workspace overlaps the %s term's", who, v[a].name);
      return -1;
    }
    for (int c = a + 1; c < kTerms; ++c)
      if (v[c].present && overlap(v[a].workspace, ws_bytes, v[c].workspace, ws_bytes)) {
        tp::set_error("%s: the %s and the %s term share a workspace", who, v[a].name, v[c].name);
        return -1;
      }
  }

  hipStream_t st = (hipStream_t)stream;
  if (sil) tp::silhouette_align_launch(es, st);
  if (photo) tp::photo_align_launch(ep, st);
  if (icp) tp::depth_icp_launch(ei, st);
  ViewTerms t;
  for (int i = 0; i < kTerms; ++i) {
    t.part[i] = v[i].present && v[i].w > 0.f ? static_cast<const double*>(v[i].workspace) : nullptr;
    t.w[i] = (double)v[i].w;
  }
  double* record = static_cast<double*>(mv->workspace);
  hipLaunchKernelGGL(view_sums_kernel, dim3(mv->B), dim3(tp::kWave), 0, st, *mv, t, G, record);
  hipLaunchKernelGGL(group_solve_kernel, dim3(mv->Gr), dim3(tp::kWave), 0, st, *mv, (const double*)record);
  if (mv->pose_out)
    hipLaunchKernelGGL(member_compose_kernel, dim3(mv->Gr), dim3(tp::kWave), 0, st, *mv, mv->model_out ? (const float*)mv->model_out : mv->model);
  return tp::check_launch(who);
}
