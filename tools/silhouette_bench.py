#!/usr/bin/env python3
"""Time the two kernels of the silhouette refiner (K31: tp_mask_sdf, two launches, and tp_silhouette_align_step, three launches in one
call) at 128 x 128 and 480 x 640 with B = 64 poses, the step against `silhouette.step_torch`, the same rules in plain torch ops in
fp64, on the same device in the same run: 64 renders of the 12,800-vertex torus, the measured masks the rasteriser's coverage at poses
about 2 degrees and 5 mm away, one mask per pose.  Both routes of the step read the same planes; their counts and statuses must be
equal before anything is timed.  Device events around many iterations after a warm-up, three repeats per route, alternating, medians;
the shader clock comes from ops.clock_probe before and after.

    python tools/silhouette_bench.py [--out profiles/silhouette/silhouette.json] [--iters 50]

Reports, per image size: microseconds per call of tp_mask_sdf (64 masks) and of both routes of the step with their ratio; the step's
share of the 8 TB/s HBM peak from its algorithmic bytes, 8 x H x W per pose (rendered depth 4, field 4; the neighbour rows are counted
once, as the cache should serve them; a share of peak of the CALL: its launches and the gaps between them are inside the events); and
microseconds per full ops.silhouette_align call (10 steps and the final evaluation, the rasteriser included) with the share of it the
eleven step calls take."""
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=50, warmup=5, repeats=3)
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import ops, silhouette
    if not torch.cuda.is_available():
        raise SystemExit("silhouette_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    clock_before = KB.shader_clock()
    t_start = time.time()
    B, tau, iters = 64, 4.0, 10
    verts, faces = torus(160, 80)
    verts_d, faces_d = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
    rows = []
    for H, W in ((128, 128), (480, 640)):
        s = H / 480.0                                            # LineMOD's intrinsics, scaled with the image
        K1 = np.array([[572.4114 * s, 0.0, 325.2611 * W / 640.0], [0.0, 573.57043 * s, 242.04899 * s], [0.0, 0.0, 1.0]], np.float32)
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
        raster = lambda pose=start: ops.mesh_raster(verts_d, faces_d, pose, K, H=H, W=W, face_ids=False, normals=False)
        mask = (raster(truth)["zbuf"] > 0).to(torch.uint8).contiguous()
        sdf, sdf_ws = torch.empty(B, H, W, device=dev), ops.mask_sdf_workspace(B, H, W, dev)
        field = lambda: ops.mask_sdf(mask, out=sdf, workspace=sdf_ws)
        field()
        r = raster()
        ws = ops.silhouette_align_workspace(B, H, W, dev)
        out = dict(pose=torch.empty(B, 3, 4, device=dev), inliers=torch.empty(B, dtype=torch.int32, device=dev), rms=torch.empty(B, device=dev),
                   status=torch.empty(B, dtype=torch.int32, device=dev), inter=torch.empty(B, dtype=torch.int32, device=dev),
                   uni=torch.empty(B, dtype=torch.int32, device=dev))
        kernel = lambda: ops.silhouette_align_step(r["zbuf"], start, K, sdf, tau_px=tau, workspace=ws, out=out)
        plain = lambda: silhouette.step_torch(r["zbuf"], start, K, sdf, tau)
        loop = lambda: ops.silhouette_align(verts_d, faces_d, start, K, sdf, tau_px=tau, iters=iters, workspace=ws)
        got, want = kernel(), plain()
        if not all(torch.equal(got[k], want[k]) for k in ("inliers", "status", "inter", "uni")):
            raise SystemExit("silhouette_bench: the two routes disagree at %d x %d; nothing was timed" % (H, W))
        pose_gap = float((got["pose"] - want["pose"]).abs().max())
        fin = loop()
        few = max(3, a.iters // 10)
        med, times = KB.race({"tp_mask_sdf": field, "tp_silhouette_align_step": kernel, "torch": plain, "silhouette_align": loop, "mesh_raster_z": raster},
                             {"tp_mask_sdf": a.iters, "tp_silhouette_align_step": a.iters, "torch": few, "silhouette_align": few, "mesh_raster_z": a.iters},
                             a.warmup, a.repeats)
        nbytes = 8 * H * W * B
        step_us = med["tp_silhouette_align_step"]
        rows.append(dict(B=B, H=H, W=W, V=len(verts), F=len(faces), tau_px=tau, iters=iters, us=med, us_all_repeats=times,
                         torch_over_tp_silhouette_align_step=med["torch"] / step_us, algorithmic_bytes=nbytes,
                         bytes_per_second=nbytes / (step_us * 1e-6), hbm_fraction_of_8TBps=nbytes / (step_us * 1e-6) / HBM_PEAK,
                         step_share_of_silhouette_align=(iters + 1) * step_us / med["silhouette_align"], counts_equal=True,
                         inliers_mean=float(want["inliers"].float().mean()), covered_fraction=float((r["zbuf"] > 0).float().mean()),
                         step_pose_max_abs_gap=pose_gap, rms0_mean=float(fin["rms0"].nanmean()), rms_final_mean=float(fin["rms"].nanmean()),
                         final_without_rim_pixel=int(fin["rms"].isnan().sum()),
                         iou0_mean=float(fin["iou0"].mean()), iou_final_mean=float(fin["iou"].mean()), final_status_ok=int((fin["status"] == 0).sum())))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(bench="silhouette", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, repeats=a.repeats,
               shader_clock_ghz_before=clock_before, shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start, rows=rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
