#!/usr/bin/env python3
"""Time the texture bake (tp_texture_bake, K27: two launches in one call) against `texture_bake.bake_torch`, the same contract in plain
torch ops in fp64, on the same device in the same run: rippled spheres of V = 20,000 and 200,000 vertices, B = 64 Fibonacci views of
480 x 640 rendered by the rasteriser from a vertex-coloured copy, a random weight plane.  The outputs are compared before anything is
timed: counts may differ only where a decision sits on a rounding tie (at most 0.01 % of the vertices; the two routes order their fp64
operations differently), colours where the counts agree within 1e-4.  Device events around many iterations after a warm-up, three
repeats per route, alternating, medians; the shader clock comes from ops.clock_probe before and after.

    python tools/texture_bake_bench.py [--out profiles/texture_bake/bake.json] [--iters 50]

Reports, per shape: microseconds per call of both routes, their ratio, the share of (vertex, view) pairs that reached their taps and the
gather rate pairs x 64 B / s (four taps of depth, colour and weight: 4 x (4 + 12) B).  Then the figure a user sees, in the same run:
seconds for TextureBaker to take the 64 views (its own depth planes included) and hand back filled colours, against frames per second of
the baked mesh through SurfelRenderer at the same resolution."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import kernel_bench as KB  # noqa: E402
from texture_bake_ref import uv_sphere  # noqa: E402  (numpy only: the tests' mesh generators; needs the repository's tests/ folder)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=50, warmup=5, repeats=3)
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import ops, texture_bake as TB
    from texpose_amd.surfel import SurfelRenderer
    if not torch.cuda.is_available():
        raise SystemExit("texture_bake_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")

    clock_before = KB.shader_clock()
    t_start = time.time()
    H, W, B, focal, dist = 480, 640, 64, 1000.0, 400.0
    pose = torch.from_numpy(TB.sphere_view_poses(B, dist).astype(np.float32)).to(dev)
    K = torch.tensor([[focal, 0.0, W / 2.0], [0.0, focal, H / 2.0], [0.0, 0.0, 1.0]], device=dev)
    weight = torch.from_numpy(np.random.RandomState(0).uniform(0.2, 1.0, (B, H, W)).astype(np.float32)).to(dev)
    rows, end_to_end = [], []
    for n_lat, n_lon in ((99, 200), (399, 500)):
        v_np, f_np = uv_sphere(n_lat, n_lon, ripple=0.15)
        V = len(v_np)
        verts, faces = torch.from_numpy(v_np).to(dev), torch.from_numpy(f_np).to(dev)
        normals = torch.from_numpy(TB.vertex_normals(v_np, f_np)).to(dev)
        vcol = (0.5 + 0.5 * torch.sin(verts / 25.0 + torch.tensor([0.0, 1.0, 2.0], device=dev))).contiguous()
        r = ops.mesh_raster(verts, faces, pose, K, H=H, W=W, vcolor=vcol, face_ids=False, normals=False)
        rgb, zbuf = r["rgb"], r["zbuf"]
        out = dict(acc=torch.empty(V, 4, device=dev), count=torch.empty(V, dtype=torch.int32, device=dev))
        ws = ops.texture_bake_workspace(V, B, dev)
        kernel = lambda: ops.texture_bake(verts, normals, pose, K, rgb, zbuf, weight, acc=out["acc"], count=out["count"], clear=True, workspace=ws)
        plain = lambda: TB.bake_torch(verts, normals, pose, K, rgb, zbuf, weight)
        got, want = kernel(), plain()
        differ = int((got["count"] != want["count"]).sum())
        same = (got["count"] == want["count"]) & (want["count"] > 0) & (want["acc"][:, 3] > 0)
        dcol = float(((got["acc"][:, :3] / got["acc"][:, 3:].clamp(min=1e-30)) - (want["acc"][:, :3] / want["acc"][:, 3:].clamp(min=1e-30)))[same].abs().max())
        if differ > 1e-4 * V or not dcol <= 1e-4 or not bool(torch.isfinite(got["acc"]).all()):
            raise SystemExit("texture_bake_bench: the two routes disagree at V = %d (%d counts differ, colours by %.3g); nothing was timed"
                             % (V, differ, dcol))
        reached = int(want["reached"])
        med, times = KB.race({"tp_texture_bake": kernel, "torch": plain}, {"tp_texture_bake": a.iters, "torch": max(3, a.iters // 10)}, a.warmup, a.repeats)
        gather = reached * 64
        rows.append(dict(V=V, F=len(f_np), B=B, H=H, W=W, slices=int(ops._lib.load().tp_texture_bake_slices(V, B)), us=med, us_all_repeats=times,
                         torch_over_tp_texture_bake=med["torch"] / med["tp_texture_bake"], pairs=V * B, pairs_reaching_taps=reached,
                         pairs_used=int(want["count"].sum()), gather_bytes=gather, gather_bytes_per_second=gather / (med["tp_texture_bake"] * 1e-6),
                         counts_differing=differ, max_colour_difference=dcol, vertices_seen=int((want["count"] > 0).sum())))
        print(json.dumps(rows[-1]), flush=True)
        # what a user sees: views in, filled colours out (depth planes by the baker's own rasteriser call), then the mesh through SurfelRenderer
        baker = TB.TextureBaker(v_np, f_np, H, W, dev)
        baker.add_views(rgb, pose, K, weight=weight)
        baker.result(fill=True)                                      # warm-up
        bake_s = []
        for _ in range(a.repeats):
            baker.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            baker.add_views(rgb, pose, K, weight=weight)
            res = baker.result(fill=True)
            torch.cuda.synchronize()
            bake_s.append(time.perf_counter() - t0)
        renderer = SurfelRenderer(v_np, f_np, res.vcolor.cpu().numpy(), H, W, dev)
        pose_nerf = TB.poses_to_nerf_units(pose, 10.0).contiguous()
        frame_us = statistics.median(KB.timed(lambda: renderer(pose_nerf, K, 10.0), max(3, a.iters // 5), a.warmup) for _ in range(a.repeats))
        err = float((res.vcolor - vcol).abs()[res.seen].max())
        end_to_end.append(dict(V=V, views=B, H=H, W=W, bake_seconds=statistics.median(bake_s), bake_seconds_all=bake_s, filled=res.filled, unseen=res.unseen,
                               max_error_against_the_source_colours=err, surfel_renderer_us_per_64_frames=frame_us,
                               surfel_renderer_frames_per_second=B / (frame_us * 1e-6)))
        print(json.dumps(end_to_end[-1]), flush=True)
    res = dict(bench="texture_bake", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, repeats=a.repeats,
               shader_clock_ghz_before=clock_before, shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start, rows=rows, end_to_end=end_to_end)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
