#!/usr/bin/env python3
"""Time the photometric-alignment step (tp_photo_align_step, K30: two launches in one call) against `photo_align.step_torch`, the same
rules in plain torch ops in fp64, on the same device in the same run: B = 8 and 64 renders of the 12,800-vertex torus with the colours
0.5 + 0.5 sin(v / 8 + (0, 1, 2)) at 480 x 640, the photograph the rasteriser's render of poses about 2 degrees and 5 mm away over a
0.5 background, one photograph per pose.  Both routes read the same planes; their counts and statuses must be equal before anything
is timed.  Device events around many iterations after a warm-up, three repeats per route, alternating, medians; the shader clock comes
from ops.clock_probe before and after.

    python tools/photo_align_bench.py [--out profiles/photo_align/photo_align.json] [--iters 50]

Reports, per batch size: microseconds per step of both routes and their ratio; the step's share of the 8 TB/s HBM peak from its
algorithmic bytes, 28 x H x W per pose (rendered depth 4, rendered colour 12, photograph 12; the photograph's neighbour rows are
counted once, as the cache should serve them; a share of peak of the CALL: both launches and the gap between them are inside the
events); microseconds per rasteriser call with rgb; and microseconds per full ops.photo_align call (10 steps and the final evaluation,
the rasteriser included) with the share of it the eleven step calls take.  DEPTH_ICP_CONTEXT repeats DESIGN section 19's figures for
tp_depth_icp_step at 12 bytes per pixel, as context only."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kernel_bench as KB  # noqa: E402
from icp_bench import rodrigues, torus  # noqa: E402

HBM_PEAK = 8.0e12
DEPTH_ICP_CONTEXT = {"tp_depth_icp_step_us": {"8": 36.0, "64": 109.1}, "bytes_per_pixel": 12, "source": "DESIGN section 19"}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=50, warmup=5, repeats=3)
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import ops, photo_align
    if not torch.cuda.is_available():
        raise SystemExit("photo_align_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    clock_before = KB.shader_clock()
    t_start = time.time()
    H, W, tau, iters = 480, 640, 0.5, 10
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
        raster = lambda pose=start: ops.mesh_raster(verts_d, faces_d, pose, K, H=H, W=W, vcolor=vcolor_d, face_ids=False, normals=False)
        shot = raster(truth)
        image = torch.where((shot["zbuf"] > 0)[..., None], shot["rgb"], torch.full_like(shot["rgb"], 0.5)).contiguous()
        r = raster()
        ws = ops.photo_align_workspace(B, H, W, dev)
        out = dict(pose=torch.empty(B, 3, 4, device=dev), inliers=torch.empty(B, dtype=torch.int32, device=dev), rms=torch.empty(B, device=dev),
                   status=torch.empty(B, dtype=torch.int32, device=dev))
        kernel = lambda: ops.photo_align_step(r["zbuf"], r["rgb"], start, K, image, tau=tau, workspace=ws, out=out)
        plain = lambda: photo_align.step_torch(r["zbuf"], r["rgb"], start, K, image, tau)
        loop = lambda: ops.photo_align(verts_d, faces_d, vcolor_d, start, K, image, tau=tau, iters=iters, workspace=ws)
        got, want = kernel(), plain()
        if not (torch.equal(got["inliers"], want["inliers"]) and torch.equal(got["status"], want["status"])):
            raise SystemExit("photo_align_bench: the two routes disagree at B = %d; nothing was timed" % B)
        pose_gap = float((got["pose"] - want["pose"]).abs().max())
        fin = loop()
        few = max(3, a.iters // 10)
        med, times = KB.race({"tp_photo_align_step": kernel, "torch": plain, "photo_align": loop, "mesh_raster_rgb": raster},
                             {"tp_photo_align_step": a.iters, "torch": few, "photo_align": few, "mesh_raster_rgb": a.iters}, a.warmup, a.repeats)
        nbytes = 28 * H * W * B
        step_us = med["tp_photo_align_step"]
        rows.append(dict(B=B, H=H, W=W, V=len(verts), F=len(faces), tau=tau, iters=iters, us=med, us_all_repeats=times,
                         torch_over_tp_photo_align_step=med["torch"] / step_us, algorithmic_bytes=nbytes, bytes_per_second=nbytes / (step_us * 1e-6),
                         hbm_fraction_of_8TBps=nbytes / (step_us * 1e-6) / HBM_PEAK, step_share_of_photo_align=(iters + 1) * step_us / med["photo_align"],
                         counts_equal=True, inliers_mean=float(want["inliers"].float().mean()), covered_fraction=float((r["zbuf"] > 0).float().mean()),
                         step_pose_max_abs_gap=pose_gap, rms0_mean=float(fin["rms0"].mean()), rms_final_mean=float(fin["rms"].mean()),
                         final_status_ok=int((fin["status"] == 0).sum())))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(bench="photo_align", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, repeats=a.repeats,
               shader_clock_ghz_before=clock_before, shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start,
               depth_icp_context=DEPTH_ICP_CONTEXT, rows=rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
