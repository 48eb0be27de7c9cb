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
tp_depth_icp_step at 12 bytes per pixel, as context only.

    python tools/photo_align_bench.py --exposure [--out profiles/photo_exposure/exposure.json]

times K37 instead (tp_photo_exposure) on the same workload, the photograph under gain (0.75, 0.80, 0.70) and bias
(0.05, 0.10, 0.08): ops.photo_exposure (fit and apply in place: three launches) against `photo_align.exposure_torch`, whose counts,
statuses and flags must be equal first, and the full ops.photo_align call with and without exposure=True in the same run, with their
ratio.  Its algorithmic bytes per pose are 8 x H x W (the rendered depth, read by the fit and by the apply) and 48 per covered
pixel (the fit reads rendered colour and photograph, the apply reads and writes the rendered colour): most of a frame is background,
which neither pass reads beyond its depth.

    python tools/photo_align_bench.py --pyramid [--out profiles/photo_pyramid/pyramid.json]

times K38 (tp_surface_down, tp_image_down, tp_mask_down) on the same workload: the down calls of one coarse pass
(the rendering from level 0 to 1 and from 1 to 2) and of the once-per-call pyramids (photograph and mask, level 0 to 1) against
`photo_align.pyramid_torch`, whose planes must be equal bit for bit first, and the full ops.photo_align call with and without
pyramid=(4, 3, 3) in the same run, with their ratio.  Algorithmic bytes per fine pixel of a level: 20 for a rendering (depth 4 and
colour 12 read, 4 written: a quarter as many pixels of 16 bytes), 15 for a photograph (12 read, 3 written), 1.25 for a mask; each level
has a quarter of the pixels of the one below.  The rendering's call reads the colours only where a coarse pixel is a surface, so what
it moves on this workload is reported too: 8 bytes per fine pixel (depth read, background written) and 12 more where it is covered."""
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


def exposure_row(a, B, H, W, tau, iters, r, image, raster, loop, truth):
    """One batch size of --exposure: ``r`` the rendering at the start poses, ``image`` the unchanged photographs, ``loop(image, **kw)``
    the full ops.photo_align call."""
    import torch
    from texpose_amd import ops, photo_align
    dev = image.device
    gain, bias = torch.tensor([0.75, 0.80, 0.70], device=dev), torch.tensor([0.05, 0.10, 0.08], device=dev)
    changed = (image * gain + bias).contiguous()
    ws = ops.photo_exposure_workspace(B, H, W, dev)
    out = {k: torch.empty((B, 3) if k in ("gain", "bias") else (B,), device=dev, dtype=torch.float32 if k in ("gain", "bias", "rms") else torch.int32)
           for k in ops.PHOTO_EXPOSURE_KEYS}
    lit = r["rgb"].clone()                                       # (rewritten by every timed call: the time does not depend on the values)
    kernel = lambda: ops.photo_exposure(r["zbuf"], lit, changed, tau=2.0, inplace=True, workspace=ws, out=out)
    plain = lambda: photo_align.exposure_torch(r["zbuf"], r["rgb"], changed, 2.0)
    got, want = ops.photo_exposure(r["zbuf"], r["rgb"], changed, tau=2.0), plain()
    if not all(torch.equal(got[k], want[k]) for k in ("count", "status", "flags")):
        raise SystemExit("photo_align_bench: the two routes disagree at B = %d; nothing was timed" % B)
    with_fit, without = loop(changed, exposure=True), loop(changed)
    err = lambda res: float((res["pose"][:, :, 3] - truth[:, :, 3]).norm(dim=1).mean())
    few = max(3, a.iters // 10)
    med, times = KB.race({"tp_photo_exposure": kernel, "exposure_torch": plain, "photo_align": lambda: loop(changed),
                          "photo_align_exposure": lambda: loop(changed, exposure=True), "mesh_raster_rgb": raster},
                         {"tp_photo_exposure": a.iters, "exposure_torch": few, "photo_align": few, "photo_align_exposure": few, "mesh_raster_rgb": a.iters},
                         a.warmup, a.repeats)
    covered = float((r["zbuf"] > 0).float().mean())
    nbytes = int((8 + 48 * covered) * H * W * B)
    us = med["tp_photo_exposure"]
    return dict(B=B, H=H, W=W, tau=tau, iters=iters, us=med, us_all_repeats=times, torch_over_tp_photo_exposure=med["exposure_torch"] / us,
                algorithmic_bytes=nbytes, bytes_per_second=nbytes / (us * 1e-6), hbm_fraction_of_8TBps=nbytes / (us * 1e-6) / HBM_PEAK,
                exposure_loop_over_plain_loop=med["photo_align_exposure"] / med["photo_align"],
                exposure_share_of_its_loop=(iters + 1) * us / med["photo_align_exposure"], counts_equal=True, covered_fraction=covered,
                count_mean=float(want["count"].float().mean()), gain_max_abs_gap=float((got["gain"] - want["gain"]).abs().max()),
                gain_recovered_mean=[float(v) for v in with_fit["gain"].mean(0)], translation_error_mm_mean=dict(start=5.0, plain_loop=err(without),
                                                                                                               exposure_loop=err(with_fit)),
                final_status_ok=int((with_fit["status"] == 0).sum()))


def pyramid_row(a, B, H, W, tau, iters, r, image, raster, loop, truth):
    """One batch size of --pyramid: ``r`` the rendering at the start poses, ``image`` the photographs, ``loop(image, **kw)`` the full
    ops.photo_align call."""
    import torch
    from texpose_amd import ops, photo_align
    dev = image.device
    mask = torch.ones(B, H, W, dtype=torch.uint8, device=dev)
    lvl1 = ops.surface_down(r["zbuf"], r["rgb"])
    empty = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    out1, out2 = dict(zbuf=empty(B, H // 2, W // 2), rgb=empty(B, H // 2, W // 2, 3)), dict(zbuf=empty(B, H // 4, W // 4), rgb=empty(B, H // 4, W // 4, 3))
    out_i, out_m = empty(B, H // 2, W // 2, 3), empty(B, H // 2, W // 2, dtype=torch.uint8)
    calls = {"tp_surface_down_0_to_1": lambda: ops.surface_down(r["zbuf"], r["rgb"], out=out1),
             "tp_surface_down_1_to_2": lambda: ops.surface_down(lvl1["zbuf"], lvl1["rgb"], out=out2),
             "tp_image_down_0_to_1": lambda: ops.image_down(image, out=out_i), "tp_mask_down_0_to_1": lambda: ops.mask_down(mask, out=out_m),
             "torch_surface_down_0_to_1": lambda: photo_align.pyramid_torch(zbuf=r["zbuf"], rgb=r["rgb"]),
             "torch_image_down_0_to_1": lambda: photo_align.pyramid_torch(image=image),
             "photo_align": lambda: loop(image), "photo_align_pyramid": lambda: loop(image, pyramid=(4, 3, 3)), "mesh_raster_rgb": raster}
    got, want = calls["tp_surface_down_0_to_1"](), calls["torch_surface_down_0_to_1"]()
    if not (torch.equal(got["zbuf"], want["zbuf"]) and torch.equal(got["rgb"], want["rgb"]) and torch.equal(calls["tp_image_down_0_to_1"](),
                                                                                                         calls["torch_image_down_0_to_1"]()["image"])):
        raise SystemExit("photo_align_bench: the two routes disagree at B = %d; nothing was timed" % B)
    with_pyramid, without = loop(image, pyramid=(4, 3, 3)), loop(image)
    err = lambda res: float((res["pose"][:, :, 3] - truth[:, :, 3]).norm(dim=1).mean())
    few = max(3, a.iters // 10)
    med, times = KB.race(calls, {k: few if k.startswith(("torch", "photo_align")) else a.iters for k in calls}, a.warmup, a.repeats)
    covered, coarse = float((r["zbuf"] > 0).float().mean()), float((got["zbuf"] > 0).float().mean())
    pixels = H * W * B
    full = {"tp_surface_down_0_to_1": 20 * pixels, "tp_surface_down_1_to_2": 20 * pixels // 4, "tp_image_down_0_to_1": 15 * pixels,
            "tp_mask_down_0_to_1": 5 * pixels // 4}
    moved = int((8 + 12 * covered) * pixels)
    rate = {k: v / (med[k] * 1e-6) for k, v in full.items()}
    pass_us = med["tp_surface_down_0_to_1"] + med["tp_surface_down_1_to_2"]
    return dict(B=B, H=H, W=W, tau=tau, iters=iters, pyramid=[4, 3, 3], us=med, us_all_repeats=times, planes_equal=True,
                torch_over_tp_surface_down=med["torch_surface_down_0_to_1"] / med["tp_surface_down_0_to_1"],
                torch_over_tp_image_down=med["torch_image_down_0_to_1"] / med["tp_image_down_0_to_1"], algorithmic_bytes=full,
                bytes_per_second=rate, hbm_fraction_of_8TBps={k: v / HBM_PEAK for k, v in rate.items()},
                surface_down_0_to_1_bytes_moved=moved, surface_down_0_to_1_moved_fraction_of_8TBps=moved / (med["tp_surface_down_0_to_1"] * 1e-6) / HBM_PEAK,
                level_2_pass_down_us=pass_us, pyramid_loop_over_plain_loop=med["photo_align_pyramid"] / med["photo_align"],
                raster_share_of_plain_loop=(iters + 1) * med["mesh_raster_rgb"] / med["photo_align"], covered_fraction=covered,
                covered_fraction_level_1=coarse, translation_error_mm_mean=dict(start=5.0, plain_loop=err(without), pyramid_loop=err(with_pyramid)),
                final_status_ok=int((with_pyramid["status"] == 0).sum()))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=50, warmup=5, repeats=3)
    ap.add_argument("--exposure", action="store_true", help="time tp_photo_exposure (K37) and the loop with and without exposure=True")
    ap.add_argument("--pyramid", action="store_true", help="time the K38 down calls and the loop with and without pyramid=(4, 3, 3)")
    a = ap.parse_args(argv)
    if a.exposure and a.pyramid:
        raise SystemExit("photo_align_bench: --exposure or --pyramid, one at a time")
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
        if a.exposure or a.pyramid:
            rows.append((exposure_row if a.exposure else pyramid_row)(a, B, H, W, tau, iters, r, image, raster, lambda im, **kw: ops.photo_align(
                verts_d, faces_d, vcolor_d, start, K, im, tau=tau, iters=iters, workspace=ws, **kw), truth))
            print(json.dumps(rows[-1]), flush=True)
            continue
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
    res = dict(bench="photo_exposure" if a.exposure else "photo_pyramid" if a.pyramid else "photo_align", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, repeats=a.repeats,
               shader_clock_ghz_before=clock_before, shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start,
               depth_icp_context=DEPTH_ICP_CONTEXT, rows=rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
