// The three pixel-tiled terms of the pose refiners (K31b silhouette_align.hip, K30 photo_align.hip, K29 depth_icp.hip) as the joint
// step K33 (joint_align.hip) reaches them: each term's host side in two halves.  `*_args_ok` is every check of the term's public step
// (false: tp_last_error says why; nothing was launched); `*_launch` is its launches on args that passed: the reduce kernel(s) into
// the term's workspace and gn_solve_kernel, which honours evaluate_only and pose_out.  The public `tp_*_step` is the one after the
// other, so the joint step runs the same kernels on the same grids: the same records, the same bits.
#pragma once
#include "tp_common.h"
#include "pose_gn.h"

namespace tp {
bool silhouette_align_args_ok(const tp_silhouette_align_args& a);
void silhouette_align_launch(const tp_silhouette_align_args& a, hipStream_t st);
bool photo_align_args_ok(const tp_photo_align_args& a);
void photo_align_launch(const tp_photo_align_args& a, hipStream_t st);
bool depth_icp_args_ok(const tp_depth_icp_args& a);
void depth_icp_launch(const tp_depth_icp_args& a, hipStream_t st);

// The body of every term's public `tp_*_step` and `tp_*_workspace_bytes`.
template <class Args>
int term_step(const char* who, const Args* a, bool (*args_ok)(const Args&), void (*launch)(const Args&, hipStream_t), tp_stream_t stream) {
  if (!a) { tp::set_error("%s: null args", who); return -1; }
  if (!args_ok(*a)) return -1;
  launch(*a, (hipStream_t)stream);
  return tp::check_launch(who);
}

inline size_t term_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return gn_workspace_bytes(B, gn_tiles((int64_t)H * W));
}
}  // namespace tp
