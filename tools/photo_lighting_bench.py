#!/usr/bin/env python3
"""Time K40 (tp_photo_lighting) by section 27's method on section 27's workload: B = 8 and 64 renders of the
12,800-vertex torus with the colours 0.5 + 0.5 sin(v / 8 + (0, 1, 2)) at 480 x 640, poses about 2 degrees and 5 mm off; the photograph
is the rasteriser's render of the true poses over a 0.5 background under a tinted ambient + directional light (0.45 of the ambient,
from the upper left, in front) and K37's bias.  Device events around many iterations after a warm-up, three repeats per route,
alternating, medians; the shader clock comes from ops.clock_probe before and after.

    python tools/photo_lighting_bench.py [--out profiles/photo_lighting/lighting.json] [--iters 50]

Timed in the same run, per batch size: ops.photo_lighting (fit and apply in place: three launches); ops.photo_exposure on the same
planes; `photo_align.lighting_torch`, the same rule in plain torch ops (counts, statuses and flags must be equal first); the fits alone
(apply=False) of both kernels, and the lighting fit on a face plane that names ONE face wherever a surface is (every gather of the
mesh then hits the same lines: what is left of the gap to the exposure fit is the wider record and the normal's arithmetic); the
rasteriser with and without the face index; the full ops.photo_align call plain, with exposure=True and with lighting=True.

Algorithmic bytes per pose: 8 x H x W (the rendered depth, read by the fit and by the apply) and 56 per covered pixel (the fit reads
rendered colour 12, photograph 12 and face index 4; the apply reads colour 12 and face 4 and writes colour 12); the gathers from the
mesh (12 bytes of indices and 36 of coordinates per covered pixel and pass) come from a mesh of 150 KB + 150 KB that stays in cache and
are reported apart."""
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
AMBIENT, STRENGTH, BIAS = (0.70, 0.75, 0.65), 0.45, (0.05, 0.10, 0.08)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=50, warmup=5, repeats=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 64])
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import ops, photo_align
    if not torch.cuda.is_available():
        raise SystemExit("photo_lighting_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    clock_before = KB.shader_clock()
    t_start = time.time()
    H, W, tau, iters = 480, 640, 0.5, 10
    verts, faces = torus(160, 80)
    vcolor = (0.5 + 0.5 * np.sin(verts.astype(np.float64) / 8.0 + np.array([0.0, 1.0, 2.0]))).astype(np.float32)
    verts_d, faces_d, vcolor_d = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(vcolor).to(dev)
    K1 = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)
    amb = torch.tensor(AMBIENT, device=dev)
    direction = torch.tensor([-1.0, -1.0, -1.0], device=dev) / 3.0 ** 0.5
    bias = torch.tensor(BIAS, device=dev)
    rows = []
    for B in a.batches:
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
        raster = lambda pose=start, ids=True: ops.mesh_raster(verts_d, faces_d, pose, K, H=H, W=W, vcolor=vcolor_d, face_ids=ids, normals=False)
        shot = raster(truth)
        nrm, valid = photo_align._pixel_normals_torch(verts_d, faces_d, shot["face"], truth)
        shade = amb * (1.0 + STRENGTH * (nrm.float() * direction).sum(-1, keepdim=True))      # [B,H,W,3]; ambient alone without a normal
        base = torch.where((shot["zbuf"] > 0)[..., None], shot["rgb"], torch.full_like(shot["rgb"], 0.5))
        image = (shade * base + bias).contiguous()
        del nrm, valid, shade, base, shot
        r = raster()
        one_face = torch.where(r["zbuf"] > 0, torch.full_like(r["face"], 4321), r["face"])
        ws = ops.photo_lighting_workspace(B, H, W, dev)
        ws_loop = ops.photo_align_workspace(B, H, W, dev, lighting=True)
        empty = lambda shape, dtype=torch.float32: torch.empty(shape, device=dev, dtype=dtype)
        out_l = dict(light=empty((B, 3, 5)), count=empty((B,), torch.int32), rms=empty((B,)), status=empty((B,), torch.int32), flags=empty((B,), torch.int32))
        out_x = dict(gain=empty((B, 3)), bias=empty((B, 3)), count=empty((B,), torch.int32), rms=empty((B,)), status=empty((B,), torch.int32),
                     flags=empty((B,), torch.int32))
        lit, lit_x = r["rgb"].clone(), r["rgb"].clone()         # (rewritten by every timed call: the time does not depend on the values)
        call = lambda face=r["face"], rgb=r["rgb"], **kw: ops.photo_lighting(verts_d, faces_d, face, r["zbuf"], rgb, start, image, tau=2.0,
                                                                             workspace=ws, out=out_l, **kw)
        plain = lambda: photo_align.lighting_torch(verts_d, faces_d, r["face"], r["zbuf"], r["rgb"], start, image, 2.0)
        got = ops.photo_lighting(verts_d, faces_d, r["face"], r["zbuf"], r["rgb"], start, image, tau=2.0)
        want = plain()
        if not all(torch.equal(got[k], want[k]) for k in ("count", "status", "flags")):
            raise SystemExit("photo_lighting_bench: the two routes disagree at B = %d; nothing was timed" % B)
        light_gap = float((got["light"] - want["light"]).abs().max())
        del want
        loop = lambda **kw: ops.photo_align(verts_d, faces_d, vcolor_d, start, K, image, tau=tau, iters=iters, workspace=ws_loop, **kw)
        ends = dict(plain_loop=loop(), exposure_loop=loop(exposure=True), lighting_loop=loop(lighting=True))
        err = lambda res: float((res["pose"][:, :, 3] - truth[:, :, 3]).norm(dim=1).mean())
        few = max(3, a.iters // 10)
        routes = {"tp_photo_lighting": lambda: call(rgb=lit, inplace=True),
                  "tp_photo_exposure": lambda: ops.photo_exposure(r["zbuf"], lit_x, image, tau=2.0, inplace=True, workspace=ws, out=out_x),
                  "lighting_torch": plain,
                  "tp_photo_lighting_fit_only": lambda: call(apply=False),
                  "tp_photo_lighting_fit_only_one_face": lambda: call(one_face, apply=False),
                  "tp_photo_exposure_fit_only": lambda: ops.photo_exposure(r["zbuf"], r["rgb"], image, tau=2.0, apply=False, workspace=ws, out=out_x),
                  "mesh_raster_rgb": lambda: raster(ids=False), "mesh_raster_rgb_face": raster,
                  "photo_align": loop, "photo_align_exposure": lambda: loop(exposure=True), "photo_align_lighting": lambda: loop(lighting=True)}
        counts = {k: few if k in ("lighting_torch", "photo_align", "photo_align_exposure", "photo_align_lighting") else a.iters for k in routes}
        med, times = KB.race(routes, counts, a.warmup, a.repeats)
        covered = float((r["zbuf"] > 0).float().mean())
        nbytes, gathers = int((8 + 56 * covered) * H * W * B), int(2 * 48 * covered * H * W * B)
        us = med["tp_photo_lighting"]
        rows.append(dict(B=B, H=H, W=W, V=len(verts), F=len(faces), tau=tau, iters=iters, us=med, us_all_repeats=times,
                         torch_over_tp_photo_lighting=med["lighting_torch"] / us, lighting_over_exposure=us / med["tp_photo_exposure"],
                         fit_only_lighting_over_exposure=med["tp_photo_lighting_fit_only"] / med["tp_photo_exposure_fit_only"],
                         fit_only_one_face_over_real_faces=med["tp_photo_lighting_fit_only_one_face"] / med["tp_photo_lighting_fit_only"],
                         algorithmic_bytes=nbytes, bytes_per_covered_pixel=56, cached_gather_bytes=gathers, bytes_per_second=nbytes / (us * 1e-6),
                         hbm_fraction_of_8TBps=nbytes / (us * 1e-6) / HBM_PEAK,
                         lighting_loop_over_plain_loop=med["photo_align_lighting"] / med["photo_align"],
                         lighting_loop_over_exposure_loop=med["photo_align_lighting"] / med["photo_align_exposure"],
                         fit_share_of_its_pass=us / (med["photo_align_lighting"] / (iters + 1)),
                         face_plane_cost_per_raster_us=med["mesh_raster_rgb_face"] - med["mesh_raster_rgb"], counts_equal=True, covered_fraction=covered,
                         count_mean=float(got["count"].float().mean()), light_max_abs_gap_to_torch=light_gap,
                         light_recovered_mean=[[float(v) for v in row] for row in ends["lighting_loop"]["light"].mean(0)],
                         translation_error_mm_mean=dict(start=5.0, **{k: err(v) for k, v in ends.items()}),
                         final_status_ok=int((ends["lighting_loop"]["status"] == 0).sum()),
                         fallback_channels=int((ends["lighting_loop"]["lighting_flags"] != 0).sum())))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(bench="photo_lighting", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, repeats=a.repeats,
               shader_clock_ghz_before=clock_before, shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start, rows=rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
