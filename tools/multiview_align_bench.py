#!/usr/bin/env python3
"""Time the multi-view step (tp_multiview_align_step, K39) and the multi-view loop beside the joint step and loop they extend, on the
same device in the same run, with tools/joint_align_bench.py's protocol and scene: B = 8 and 64 renders of the 12,800-vertex torus at
480 x 640, silhouette + photometric at the default weights, the measured masks and photographs rendered at poses about 2 degrees and
5 mm from the start.  The B views form groups of 8: each group is one object in the world, its first view's camera is [I|0] and view i's
is truth_i o truth_first^-1, so the composed poses at the true model are the joint benchmark's true poses.  With every camera [I|0] and
one view per group the step's model must equal the joint step's pose bit for bit before anything is timed.  Device events around many
iterations after a warm-up, three repeats per route, alternating, medians; the shader clock comes from ops.clock_probe before and after.

    python tools/multiview_align_bench.py [--out profiles/multiview/multiview.json] [--iters 50]

Reports, per batch size, microseconds per call of: the multi-view step and the joint step on the same planes; ops.pose_compose; the
rasteriser's one call per pass; the multi-view loop and the joint loop (20 steps and the final evaluation each).  No speed target is set
for K39: it adds two small launches and a compose per pass to a loop bound by the rasteriser."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kernel_bench as KB  # noqa: E402
from icp_bench import rodrigues, torus  # noqa: E402

VIEWS_PER_GROUP = 8


def _inverse(P):
    Rt = P[:, :3].T
    return np.concatenate([Rt, -(Rt @ P[:, 3:])], 1)


def _times(P, Q):
    return np.concatenate([P[:, :3] @ Q[:, :3], P[:, :3] @ Q[:, 3:] + P[:, 3:]], 1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=50, warmup=5, repeats=3)
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("multiview_align_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    clock_before = KB.shader_clock()
    t_start = time.time()
    H, W, tau_px, tau = 480, 640, 4.0, 0.5
    verts, faces = torus(160, 80)
    vcolor = (0.5 + 0.5 * np.sin(verts.astype(np.float64) / 8.0 + np.array([0.0, 1.0, 2.0]))).astype(np.float32)
    verts_d, faces_d, vcolor_d = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(vcolor).to(dev)
    K1 = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)
    rows = []
    for B in (8, 64):
        Gr = B // VIEWS_PER_GROUP
        truth, start = np.zeros((B, 3, 4)), np.zeros((B, 3, 4))
        for b in range(B):
            q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
            if np.linalg.det(q) < 0:
                q[:, 0] *= -1
            t = rs.uniform(-40, 40, 3) + [0.0, 0.0, 400.0]
            w, dt = rs.normal(size=3), rs.normal(size=3)
            truth[b] = np.concatenate([q, t[:, None]], 1)
            start[b] = np.concatenate([rodrigues(w * np.radians(2.0) / np.linalg.norm(w)) @ q, (t + dt * 5.0 / np.linalg.norm(dt))[:, None]], 1)
        group = np.arange(B) // VIEWS_PER_GROUP
        cam = np.stack([_times(truth[b], _inverse(truth[group[b] * VIEWS_PER_GROUP])) for b in range(B)])
        cam[::VIEWS_PER_GROUP] = np.eye(3, 4)
        up = lambda x, dtype=np.float32: torch.from_numpy(np.ascontiguousarray(x, dtype)).to(dev)
        truth_d, start_d, K = up(truth), up(start), up(np.tile(K1, (B, 1, 1)))
        cam_d, group_d, model0 = up(cam), up(group, np.int32), up(start[::VIEWS_PER_GROUP])          # (the first view's start, in the world frame)
        pose0 = ops.pose_compose(cam_d, model0, group_d)
        raster = lambda pose=pose0: ops.mesh_raster(verts_d, faces_d, pose, K, H=H, W=W, vcolor=vcolor_d, face_ids=False, normals=False)
        shot = raster(truth_d)
        image = torch.where((shot["zbuf"] > 0)[..., None], shot["rgb"], torch.full_like(shot["rgb"], 0.5)).contiguous()
        sdf = ops.mask_sdf((shot["zbuf"] > 0).to(torch.uint8))
        r = raster()
        ws = ops.multiview_align_workspace(B, H, W, dev, terms=2)
        index = ops.multiview_group_index(group_d, Gr)
        sil, photo = dict(zbuf=r["zbuf"], sdf=sdf, tau_px=tau_px), dict(zbuf=r["zbuf"], rgb=r["rgb"], image=image, tau=tau)
        multi_step = lambda: ops.multiview_align_step(model0, cam_d, group_d, K, silhouette=sil, photo=photo, workspace=ws, pose=pose0, index=index)
        joint_step = lambda: ops.joint_align_step(pose0, K, silhouette=sil, photo=photo, workspace=ws)
        compose = lambda: ops.pose_compose(cam_d, model0, group_d)
        multi_loop = lambda: ops.multiview_align(verts_d, faces_d, model0, cam_d, group_d, K, vcolor=vcolor_d, sdf=sdf, image=image, tau_px=tau_px,
                                                 tau=tau, iters=20, workspace=ws)
        joint_loop = lambda: ops.joint_align(verts_d, faces_d, pose0, K, vcolor=vcolor_d, sdf=sdf, image=image, tau_px=tau_px, tau=tau, iters=20,
                                             workspace=ws)
        # the identity before anything is timed: identity cameras and singletons are the joint step
        eye, each = up(np.tile(np.eye(3, 4), (B, 1, 1))), up(np.arange(B), np.int32)
        plain, joint = ops.multiview_align_step(pose0, eye, each, K, silhouette=sil, photo=photo), joint_step()
        if not all(torch.equal(plain[k].view(torch.int32), joint[j].view(torch.int32)) for k, j in (("model", "pose"), ("status", "status"),
                                                                                                   ("inliers", "inliers"), ("chi2", "chi2"))):
            raise SystemExit("multiview_align_bench: identity cameras and singletons differ from the joint step at B = %d; nothing was timed" % B)
        fin, alone = multi_loop(), joint_loop()
        gap = lambda P: float(((P - truth_d).abs().reshape(B, -1).max(1).values).max())
        few = max(3, a.iters // 10)
        fns = {"tp_multiview_align_step": multi_step, "tp_joint_align_step": joint_step, "tp_pose_compose": compose, "mesh_raster_rgb": raster,
               "multiview_align_20": multi_loop, "joint_align_20": joint_loop}
        med, times = KB.race(fns, {k: few if k.endswith("_20") else a.iters for k in fns}, a.warmup, a.repeats)
        rows.append(dict(B=B, Gr=Gr, H=H, W=W, V=len(verts), F=len(faces), tau_px=tau_px, tau=tau, weights=list(ops.JOINT_WEIGHTS), us=med,
                         us_all_repeats=times, multiview_step_over_joint_step=med["tp_multiview_align_step"] / med["tp_joint_align_step"],
                         multiview_loop_over_joint_loop=med["multiview_align_20"] / med["joint_align_20"], identity_bit_equal=True,
                         multiview_final_status_ok=int((fin["status"] == 0).sum()), joint_final_status_ok=int((alone["status"] == 0).sum()),
                         multiview_pose_max_abs_gap=gap(fin["pose"]), joint_pose_max_abs_gap=gap(alone["pose"])))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(bench="multiview_align", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, repeats=a.repeats,
               shader_clock_ghz_before=clock_before, shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start, rows=rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
