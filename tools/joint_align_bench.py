#!/usr/bin/env python3
"""Time the joint step (tp_joint_align_step, K33) and the joint loop beside the route they replace, the terms one after the other, on
the same device in the same run: B = 8 and 64 renders of the 12,800-vertex torus with the colours 0.5 + 0.5 sin(v / 8 + (0, 1, 2)) at
480 x 640; the measured masks and photographs are the rasteriser's render of poses about 2 degrees and 5 mm away (the photograph over a
0.5 background), one per pose.  Silhouette + photometric, the default weights.  The joint step's per-term outputs must equal the
standalone evaluations bit for bit before anything is timed.  Device events around many iterations after a warm-up, three repeats per
route, alternating, medians; the shader clock comes from ops.clock_probe before and after.

    python tools/joint_align_bench.py [--out profiles/joint/joint.json] [--iters 50]

Reports, per batch size, microseconds per call of: the joint step; the silhouette step and the photometric step alone (their sum is
what one pass of both terms costs today); the rasteriser asked for depth + colour (the joint loop's one call per pass) and for depth
alone; the joint loop (20 steps and the final evaluation, one rasteriser call per pass); and the sequential route (ops.silhouette_align,
10 steps, then ops.photo_align, 10 steps, from its poses).  No speed target is set for K33: the joint solve is one wave per image after
the terms' own launches."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kernel_bench as KB  # noqa: E402
from icp_bench import rodrigues, torus  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=50, warmup=5, repeats=3)
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("joint_align_bench: needs a GPU (a CPU run cannot give a time)")
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
        truth, start = np.zeros((B, 3, 4), np.float32), np.zeros((B, 3, 4), np.float32)
        for b in range(B):
            q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
            if np.linalg.det(q) < 0:
                q[:, 0] *= -1
            t = rs.uniform(-40, 40, 3) + [0.0, 0.0, 400.0]
            w, dt = rs.normal(size=3), rs.normal(size=3)
            truth[b] = np.concatenate([q, t[:, None]], 1)
            start[b] = np.concatenate([rodrigues(w * np.radians(2.0) / np.linalg.norm(w)) @ q, (t + dt * 5.0 / np.linalg.norm(dt))[:, None]], 1)
        truth, start, K = torch.from_numpy(truth).to(dev), torch.from_numpy(start).to(dev), torch.from_numpy(np.tile(K1, (B, 1, 1))).to(dev)
        raster_rgb = lambda pose=start: ops.mesh_raster(verts_d, faces_d, pose, K, H=H, W=W, vcolor=vcolor_d, face_ids=False, normals=False)
        raster_z = lambda pose=start: ops.mesh_raster(verts_d, faces_d, pose, K, H=H, W=W, face_ids=False, normals=False)
        shot = raster_rgb(truth)
        image = torch.where((shot["zbuf"] > 0)[..., None], shot["rgb"], torch.full_like(shot["rgb"], 0.5)).contiguous()
        sdf = ops.mask_sdf((shot["zbuf"] > 0).to(torch.uint8))
        r = raster_rgb()
        ws = ops.joint_align_workspace(B, H, W, dev, terms=2)
        sil, photo = dict(zbuf=r["zbuf"], sdf=sdf, tau_px=tau_px), dict(zbuf=r["zbuf"], rgb=r["rgb"], image=image, tau=tau)
        joint_step = lambda: ops.joint_align_step(start, K, silhouette=sil, photo=photo, workspace=ws)
        sil_step = lambda: ops.silhouette_align_step(r["zbuf"], start, K, sdf, tau_px=tau_px, workspace=ws)
        photo_step = lambda: ops.photo_align_step(r["zbuf"], r["rgb"], start, K, image, tau=tau, workspace=ws)
        joint_loop = lambda: ops.joint_align(verts_d, faces_d, start, K, vcolor=vcolor_d, sdf=sdf, image=image, tau_px=tau_px, tau=tau, iters=20,
                                             workspace=ws)

        def sequential():
            first = ops.silhouette_align(verts_d, faces_d, start, K, sdf, tau_px=tau_px, iters=10, workspace=ws)
            return ops.photo_align(verts_d, faces_d, vcolor_d, first["pose"], K, image, tau=tau, iters=10, workspace=ws)

        got = joint_step()
        own_s = ops.silhouette_align_step(r["zbuf"], start, K, sdf, tau_px=tau_px, evaluate_only=True)
        own_p = ops.photo_align_step(r["zbuf"], r["rgb"], start, K, image, tau=tau, evaluate_only=True)
        same = all(torch.equal(got[p + k].view(torch.int32), own[k].view(torch.int32))
                   for p, own in (("sil_", own_s), ("photo_", own_p)) for k in ("inliers", "rms", "status"))
        if not same:
            raise SystemExit("joint_align_bench: the joint step's terms differ from their standalone evaluations at B = %d; nothing was timed" % B)
        fin, seq = joint_loop(), sequential()
        gap = lambda P: float(((P - truth).abs().reshape(B, -1).max(1).values).max())
        few = max(3, a.iters // 10)
        fns = {"tp_joint_align_step": joint_step, "tp_silhouette_align_step": sil_step, "tp_photo_align_step": photo_step,
               "mesh_raster_rgb": raster_rgb, "mesh_raster_depth": raster_z, "joint_align_20": joint_loop, "silhouette_10_then_photo_10": sequential}
        med, times = KB.race(fns, {k: few if k in ("joint_align_20", "silhouette_10_then_photo_10") else a.iters for k in fns}, a.warmup, a.repeats)
        rows.append(dict(B=B, H=H, W=W, V=len(verts), F=len(faces), tau_px=tau_px, tau=tau, weights=list(ops.JOINT_WEIGHTS), us=med, us_all_repeats=times,
                         joint_step_over_sum_of_term_steps=med["tp_joint_align_step"] / (med["tp_silhouette_align_step"] + med["tp_photo_align_step"]),
                         joint_loop_over_sequential=med["joint_align_20"] / med["silhouette_10_then_photo_10"], terms_bit_equal=True,
                         inliers_mean=float(got["inliers"].float().mean()), joint_final_status_ok=int((fin["status"] == 0).sum()),
                         sequential_final_status_ok=int((seq["status"] == 0).sum()), joint_pose_max_abs_gap=gap(fin["pose"]),
                         sequential_pose_max_abs_gap=gap(seq["pose"])))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(bench="joint_align", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, repeats=a.repeats,
               shader_clock_ghz_before=clock_before, shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start, rows=rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
