#!/usr/bin/env python3
"""Time the scene annotations (tp_scene_annotate, K22: two launches in one call) with and without the mask stacks against the torch
route written out plainly: per object a compare, the label test, two sums, row / column `any` with min / max of their indices for both
boxes, and the casts of the two masks.  K = 3, 8, 32 objects, B = 10 poses, at 480 x 640 and 128 x 128; all three routes in the same
run on the same box, reading the same [K,B,H,W] planes and the same label.  Also tp_view_images against the chain tools/novel_views.py
uses for its loose files (clamp, scale, cast per map).  Device events around many iterations after a warm-up, each route timed twice,
alternating; the shader clock is read before and after.

    python tools/scene_annotate_bench.py [--out profiles/scene_annotate/scene_annotate_bench.json] [--iters 100]

Reports, per shape: microseconds per call of every route (medians over the repeats), the ratios to the torch route of the same run, and
K22's share of the 8 TB/s HBM peak from its algorithmic bytes, (4 K + 4) read + 2 K written per pixel with masks, (4 K + 4) read
without (a share of peak of the CALL: both launches and the gap between them are inside the events)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kernel_bench as KB  # noqa: E402

HBM_PEAK = 8.0e12


def sclk():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if "sclk" in k.lower()}
    except Exception as e:                                          # the clock is context, not a result
        return {"error": repr(e)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=100, warmup=10, repeats=3)
    ap.add_argument("--B", type=int, default=10)
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("scene_annotate_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    B = a.B
    rs = np.random.RandomState(0)

    # ms_per_step of the box: a fixed torch workload, so that records from different boxes can be told apart
    x = torch.randn(4096, 4096, device=dev)
    box_ms = KB.timed(lambda: x @ x, 20, a.warmup) / 1e3
    rows, image_rows = [], []
    clock_before = sclk()
    t_start = time.time()
    for H, W in ((480, 640), (128, 128)):
        for K in (3, 8, 32):
            z = rs.uniform(400.0, 1500.0, size=(K, B, H, W)).astype(np.float32)
            z[rs.uniform(size=z.shape) < 0.6] = -1.0
            zbuf = torch.from_numpy(z).to(dev)
            ids = torch.arange(1, K + 1, dtype=torch.int32, device=dev)
            label = ops.scene_bounds(zbuf, None, ids, depth_scale=10.0, bg_range=(0.0, 30.0), source="none")["label"]
            out = dict(info=torch.empty(B, K, 10, dtype=torch.int32, device=dev), mask=torch.empty(B, K, H, W, dtype=torch.uint8, device=dev),
                       mask_visib=torch.empty(B, K, H, W, dtype=torch.uint8, device=dev))
            lean = dict(info=torch.empty(B, K, 10, dtype=torch.int32, device=dev))
            cols, rws = torch.arange(W, device=dev), torch.arange(H, device=dev)
            lab = label.view(B, H, W)

            def k22_masks():
                return ops.scene_annotate(zbuf, label, ids, out=out)

            def k22_lean():
                return ops.scene_annotate(zbuf, label, ids, masks=False, out=lean)

            def box(m):                                             # m [B,H,W] bool -> [B,4], -1 where empty
                cx, cy = m.any(1), m.any(2)
                big = 1 << 30
                xmin = torch.where(cx, cols, big).amin(1); xmax = torch.where(cx, cols, -1).amax(1)
                ymin = torch.where(cy, rws, big).amin(1); ymax = torch.where(cy, rws, -1).amax(1)
                empty = xmax < 0
                return torch.stack([torch.where(empty, -1, xmin), torch.where(empty, -1, ymin), xmax, ymax], -1)

            def torch_route():
                info, masks, visib = [], [], []
                for k in range(K):
                    full = zbuf[k] > 0
                    vis = full & (lab == ids[k])
                    info.append(torch.cat([full.sum((1, 2))[:, None], vis.sum((1, 2))[:, None], box(full), box(vis)], -1))
                    masks.append(full.to(torch.uint8) * 255)
                    visib.append(vis.to(torch.uint8) * 255)
                return dict(info=torch.stack(info, 1).int(), mask=torch.stack(masks, 1), mask_visib=torch.stack(visib, 1))

            r_new, r_old = k22_masks(), torch_route()
            same = {k: bool(torch.equal(r_new[k], r_old[k])) for k in r_new}
            same["info_without_masks"] = bool(torch.equal(k22_lean()["info"], r_old["info"]))
            iters = a.iters if H * W * K < 3e6 else max(10, a.iters // 4)
            med, raw = KB.race(dict(k22_masks=k22_masks, k22_no_masks=k22_lean, torch=torch_route), iters, a.warmup, a.repeats)
            px = B * H * W
            bytes_masks, bytes_lean = (4 * K + 4 + 2 * K) * px, (4 * K + 4) * px
            rows.append(dict(K=K, B=B, H=H, W=W, us=med, us_all_repeats=raw, torch_over_k22_masks=med["torch"] / med["k22_masks"],
                             torch_over_k22_no_masks=med["torch"] / med["k22_no_masks"], algorithmic_bytes_masks=bytes_masks,
                             algorithmic_bytes_no_masks=bytes_lean, hbm_fraction_of_8TBps_masks=bytes_masks / (med["k22_masks"] * 1e-6) / HBM_PEAK,
                             hbm_fraction_of_8TBps_no_masks=bytes_lean / (med["k22_no_masks"] * 1e-6) / HBM_PEAK, outputs_equal_to_torch_route=same))
            print(json.dumps(rows[-1]), flush=True)
            del zbuf, out, r_new, r_old
        rgb = torch.from_numpy(rs.uniform(-0.1, 1.1, size=(B, H * W, 3)).astype(np.float32)).to(dev)
        depth = torch.from_numpy(rs.uniform(0.0, 20.0, size=(B, H * W)).astype(np.float32)).to(dev)
        img = dict(rgb8=torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev), depth16=torch.empty(B, H, W, dtype=torch.uint16, device=dev))

        def images_new():
            return ops.view_images(rgb, depth, H=H, W=W, depth_scale=10.0, png_per_metre=2000, out=img)

        def images_torch():                                         # the tool's chain, per pose as the tool runs it, without the copies to the host
            res = []
            for i in range(B):
                res.append(((rgb[i].view(H, W, 3).clamp(0, 1) * 255).byte(), ((depth[i].view(H, W) / 10.0) * 2000).clamp(0, 65535).to(torch.int32)))
            return res

        med, raw = KB.race(dict(view_images=images_new, torch=images_torch), a.iters, a.warmup, a.repeats)
        old = images_torch()
        got = images_new()
        same = dict(rgb8=bool(all(torch.equal(got["rgb8"][i], old[i][0]) for i in range(B))),
                    depth16_max_abs_diff=int(max((got["depth16"][i].to(torch.int32) - old[i][1]).abs().max() for i in range(B))))
        nbytes = (12 + 3 + 4 + 2) * B * H * W
        image_rows.append(dict(B=B, H=H, W=W, us=med, us_all_repeats=raw, torch_over_view_images=med["torch"] / med["view_images"],
                               algorithmic_bytes=nbytes, hbm_fraction_of_8TBps=nbytes / (med["view_images"] * 1e-6) / HBM_PEAK, agreement=same))
        print(json.dumps(image_rows[-1]), flush=True)
    res = dict(bench="scene_annotate", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, repeats=a.repeats,
               ms_per_step_of_the_box_4096_matmul=box_ms, seconds=time.time() - t_start, sclk_before=clock_before, sclk_after=sclk(),
               rows=rows, view_images=image_rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
