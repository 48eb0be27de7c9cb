// K33 tp_joint_align_step: one joint Gauss-Newton step of the render-and-compare refiners, the rows of the silhouette (K31b), the
// photometric (K30) and the depth term (K29) in one normal system (the public functions are in
// texpose_amd/joint.py, the rules in include/texpose_amd.h).
//
//   the terms    each present term runs its own launches (pose_terms.h) with evaluate_only set and no pose_out: its reduce kernel
//                writes the term's records into the term's workspace and its gn_solve_kernel the term's inliers, rms and status,
//                exactly as the standalone call would.
//   joint_solve  grid B x 64.  Gathers each term's G records with gn_gather (ascending tile order; silhouette, photometric, depth),
//                29 threads form sum[k] = w_a S_a[k] + w_b S_b[k] + w_c S_c[k] over the weighted terms in fp64 as written, and
//                thread 0 applies gn_solve_kernel's rules to the combined sums (pose_gn.h's gn_decide: count, pivot rule, gn_step,
//                fp32 rounding, the pass-through of a failed pose).
// No atomics; every fp64 sum has one fixed order, so all outputs are a function of the inputs alone.
#include "tp_common.h"
#include "pose_gn.h"
#include "pose_terms.h"

namespace {
constexpr int kTerms = 3;                              // silhouette, photometric, depth: the order of the sum

struct JointTerms {
  const double* part[kTerms];                          // the term's records [B,G,32], or null: absent or weight 0, not in the sum
  double w[kTerms];
};

__global__ __launch_bounds__(tp::kWave) void joint_solve_kernel(tp_joint_align_args j, JointTerms t, int G) {
  __shared__ double sum[kGnPart], term[kGnPart], stage[kGnStage][kGnPart];
  const int b = blockIdx.x;
  double s = 0.0;                                                                // thread k < 29: sum[k]
  bool first = true;
  for (int i = 0; i < kTerms; ++i) {                                             // (uniform: t is a kernel argument)
    if (!t.part[i]) continue;
    gn_gather(t.part[i] + (int64_t)b * G * kGnPart, G, stage, term);
    if (threadIdx.x < kGnSums) {
      const double v = threadIdx.x < kGnSums - 1 ? t.w[i] * term[threadIdx.x] : term[threadIdx.x];        // (the count is not weighted)
      s = first ? v : s + v;
    }
    first = false;
    __syncthreads();                                                             // term is free for the next gather
  }
  if (threadIdx.x < kGnSums) sum[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  float out[12];
  const int status = gn_decide(sum, j.pose + (int64_t)b * 12, (double)j.damping, j.evaluate_only != 0, out);          // gn_solve_kernel's rules
  j.inliers[b] = (int)sum[28];
  j.chi2[b] = (float)sum[27];
  j.status[b] = status;
  if (j.pose_out)
    for (int k = 0; k < 12; ++k) j.pose_out[(int64_t)b * 12 + k] = out[k];
}

// what the joint step needs to know of a term, whichever struct it is
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

// the term as the joint step runs it: evaluating, writing no pose
template <class Args>
Args evaluating(const Args* a) {
  Args e = *a;
  e.evaluate_only = 1;
  e.pose_out = nullptr;
  return e;
}
}  // namespace

extern "C" int tp_joint_align_step(const tp_joint_align_args* j, const tp_silhouette_align_args* sil, const tp_photo_align_args* photo,
                                   const tp_depth_icp_args* icp, tp_stream_t stream) {
  const char* who = "tp_joint_align_step";
  if (!j) { tp::set_error("%s: null args", who); return -1; }
  const TermView v[kTerms] = {view_of("silhouette", sil, j->w_sil), view_of("photo", photo, j->w_photo), view_of("icp", icp, j->w_icp)};
  bool any = false, weighted = false;
  for (const TermView& t : v) {
    if (!(t.w >= 0.f) || !isfinite(t.w)) { tp::set_error("%s: the %s weight must be finite and not negative", who, t.name); return -1; }
    any = any || t.present;
    weighted = weighted || (t.present && t.w > 0.f);
  }
  if (!any) { tp::set_error("%s: no term is present", who); return -1; }
  if (!weighted) { tp::set_error("%s: no present term has a weight > 0", who); return -1; }
  if (!(j->damping >= 0.f) || !isfinite(j->damping)) { tp::set_error("%s: damping must be finite and not negative", who); return -1; }
  if (!j->pose || !j->status || !j->inliers || !j->chi2 || (!j->pose_out && !j->evaluate_only)) {
    tp::set_error("%s: null pointer", who);
    return -1;
  }
  if (j->B <= 0 || j->B > 65535) { tp::set_error("%s: bad sizes (B 1..65535)", who); return -1; }
  if (j->pose_out) {
    const uintptr_t in = (uintptr_t)j->pose, out = (uintptr_t)j->pose_out, bytes = (uintptr_t)j->B * 12 * sizeof(float);
    if (in < out + bytes && out < in + bytes) { tp::set_error("%s: pose_out must not overlap pose", who); return -1; }
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
    if (t.B != j->B) { tp::set_error("%s: the %s term's B = %d differs from args' B = %d", who, t.name, t.B, j->B); return -1; }
    if (t.pose != j->pose) { tp::set_error("%s: the %s term's pose differs from args' pose", who, t.name); return -1; }
    if (!ref) { ref = &t; continue; }
    if (t.H != ref->H || t.W != ref->W) {
      tp::set_error("%s: the %s term is %d x %d, the %s term %d x %d", who, t.name, t.H, t.W, ref->name, ref->H, ref->W);
      return -1;
    }
    if (t.intr != ref->intr) { tp::set_error("%s: the %s term's intr differs from the %s term's", who, t.name, ref->name); return -1; }
  }
  const int G = (int)gn_tiles((int64_t)ref->H * ref->W);
  const uintptr_t ws_bytes = (uintptr_t)gn_workspace_bytes(j->B, G);
  for (int a = 0; a < kTerms; ++a)
    for (int c = a + 1; c < kTerms; ++c) {
      if (!v[a].present || !v[c].present) continue;
      const uintptr_t p = (uintptr_t)v[a].workspace, q = (uintptr_t)v[c].workspace;
      if (p < q + ws_bytes && q < p + ws_bytes) {
        tp::set_error("%s: the %s and the %s term share a workspace", who, v[a].name, v[c].name);
        return -1;
      }
    }

  hipStream_t st = (hipStream_t)stream;
  if (sil) tp::silhouette_align_launch(es, st);
  if (photo) tp::photo_align_launch(ep, st);
  if (icp) tp::depth_icp_launch(ei, st);
  JointTerms t;
  for (int i = 0; i < kTerms; ++i) {
    t.part[i] = v[i].present && v[i].w > 0.f ? static_cast<const double*>(v[i].workspace) : nullptr;
    t.w[i] = (double)v[i].w;
  }
  hipLaunchKernelGGL(joint_solve_kernel, dim3(j->B), dim3(tp::kWave), 0, st, *j, t, G);
  return tp::check_launch(who);
}
