#!/usr/bin/env python3
"""Time the depth-ICP step (tp_depth_icp_step, K29: two launches in one call) against `icp.step_torch`, the same rules in plain torch
ops in fp64, on the same device in the same run: B = 8 and 64 renders of the 12,800-vertex torus at 480 x 640, the measured depth the
render of poses about 2 degrees and 5 mm away, one plane per pose.  Both routes read the same planes; their counts and statuses must be
equal before anything is timed.  Device events around many iterations after a warm-up, three repeats per route, alternating, medians;
the shader clock comes from ops.clock_probe before and after.

    python tools/icp_bench.py [--out profiles/icp/icp.json] [--iters 50]

Reports, per batch size: microseconds per step of both routes and their ratio; the step's share of the 8 TB/s HBM peak from its
algorithmic bytes, 3 x 4 x H x W per pose (rendered depth, face index, measured depth; a share of peak of the CALL: both launches and
the gap between them are inside the events); and microseconds per full ops.depth_icp call (5 steps and the final evaluation, the
rasteriser included) with the share of it the six ICP calls take."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kernel_bench as KB  # noqa: E402

HBM_PEAK = 8.0e12


def torus(n_major, n_minor, R=45.0, r=16.0):
    u, w = np.linspace(0, 2 * np.pi, n_major, endpoint=False), np.linspace(0, 2 * np.pi, n_minor, endpoint=False)
    U, Wm = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(Wm)) * np.cos(U), (R + r * np.cos(Wm)) * np.sin(U), r * np.sin(Wm)], -1).reshape(-1, 3)
    idx = np.arange(n_major * n_minor).reshape(n_major, n_minor)
    a, b = idx, np.roll(idx, -1, axis=0)
    c, d = np.roll(idx, -1, axis=1), np.roll(np.roll(idx, -1, axis=0), -1, axis=1)
    return v.astype(np.float32), np.concatenate([np.stack([a, b, d], -1), np.stack([a, d, c], -1)]).reshape(-1, 3).astype(np.int32)


def rodrigues(w):
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * (Wx @ Wx)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=50, warmup=5, repeats=3)
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import icp, ops
    if not torch.cuda.is_available():
        raise SystemExit("icp_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    clock_before = KB.shader_clock()
    t_start = time.time()
    H, W, tau, iters = 480, 640, 20.0, 5
    verts, faces = torus(160, 80)
    verts_d, faces_d = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev)
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
        depth = ops.mesh_raster(verts_d, faces_d, truth, K, H=H, W=W, face_ids=False, normals=False)["zbuf"].clamp(min=0.0)
        r = ops.mesh_raster(verts_d, faces_d, start, K, H=H, W=W, face_ids=True, normals=False)
        ws = ops.depth_icp_workspace(B, H, W, dev)
        out = dict(pose=torch.empty(B, 3, 4, device=dev), inliers=torch.empty(B, dtype=torch.int32, device=dev), rms=torch.empty(B, device=dev),
                   status=torch.empty(B, dtype=torch.int32, device=dev))
        kernel = lambda: ops.depth_icp_step(verts_d, faces_d, r["zbuf"], r["face"], start, K, depth, tau_mm=tau, workspace=ws, out=out)
        plain = lambda: icp.step_torch(verts_d, faces_d, r["zbuf"], r["face"], start, K, depth, tau)
        loop = lambda: ops.depth_icp(verts_d, faces_d, start, K, depth, tau_mm=tau, iters=iters, workspace=ws)
        raster = lambda: ops.mesh_raster(verts_d, faces_d, start, K, H=H, W=W, face_ids=True, normals=False)
        got, want = kernel(), plain()
        if not (torch.equal(got["inliers"], want["inliers"]) and torch.equal(got["status"], want["status"])):
            raise SystemExit("icp_bench: the two routes disagree at B = %d; nothing was timed" % B)
        pose_gap = float((got["pose"] - want["pose"]).abs().max())
        fin = loop()
        few = max(3, a.iters // 10)
        med, times = KB.race({"tp_depth_icp_step": kernel, "torch": plain, "depth_icp": loop, "mesh_raster": raster},
                             {"tp_depth_icp_step": a.iters, "torch": few, "depth_icp": few, "mesh_raster": a.iters}, a.warmup, a.repeats)
        nbytes = 3 * 4 * H * W * B
        step_us = med["tp_depth_icp_step"]
        rows.append(dict(B=B, H=H, W=W, V=len(verts), F=len(faces), tau_mm=tau, iters=iters, us=med, us_all_repeats=times,
                         torch_over_tp_depth_icp_step=med["torch"] / step_us, algorithmic_bytes=nbytes, bytes_per_second=nbytes / (step_us * 1e-6),
                         hbm_fraction_of_8TBps=nbytes / (step_us * 1e-6) / HBM_PEAK, icp_share_of_depth_icp=(iters + 1) * step_us / med["depth_icp"],
                         counts_equal=True, inliers_mean=float(want["inliers"].float().mean()), covered_fraction=float((r["zbuf"] > 0).float().mean()),
                         step_pose_max_abs_gap=pose_gap, rms0_mean_mm=float(fin["rms0"].mean()), rms_final_mean_mm=float(fin["rms"].mean()),
                         final_status_ok=int((fin["status"] == 0).sum())))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(bench="icp", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, repeats=a.repeats,
               shader_clock_ghz_before=clock_before, shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start, rows=rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
