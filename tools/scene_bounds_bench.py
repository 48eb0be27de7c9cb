#!/usr/bin/env python3
"""Time the scene-bounds blend (tp_scene_bounds, one launch) against the route that existed before it: K calls of
geometry.online_box_range plus the torch stack / where / min / gather / where composition of the same four outputs.
K = 1, 3 and 8 objects at 480 x 640 and B = 16 poses, source 'box'; the rasterisation is excluded from both routes (both read the
same [K,B,H,W] zbuf planes).  Device events around many iterations after a warm-up; the shader clock is read before and after.

    python tools/scene_bounds_bench.py [--out profiles/scene_bounds/scene_bounds_bench.json] [--iters 200]

Reports, per K: microseconds per call of both routes, their ratio, and the new launch's share of the 8 TB/s HBM peak computed from its
algorithmic bytes (4 K + 16) * B * H * W (a share of peak of the KERNEL, launch gaps included since it is timed with events)."""
import argparse
import json
import os
import subprocess
import sys

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
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--H", type=int, default=480)
    ap.add_argument("--W", type=int, default=640)
    a = ap.parse_args(argv)
    import torch
    from oracle import texpose_oracle as O
    from texpose_amd import ops
    from texpose_amd.geometry import online_box_range
    if not torch.cuda.is_available():
        raise SystemExit("scene_bounds_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    B, H, W = a.B, a.H, a.W
    sc = O.synthetic_scene(H, W, B=B, seed=1)
    pose, intr = sc["pose"].to(dev).contiguous(), sc["intr"].to(dev).contiguous()
    bg = (0.0, 30.0)
    rs = np.random.RandomState(0)
    rows = []
    clock_before = sclk()
    for K in (1, 3, 8):
        z = rs.uniform(400.0, 1500.0, size=(K, B, H, W)).astype(np.float32)
        z[rs.uniform(size=z.shape) < 0.6] = -1.0
        zbuf = torch.from_numpy(z).to(dev)
        c = rs.uniform(-0.6, 0.6, size=(K, 1, 3))
        h = rs.uniform(0.2, 0.8, size=(K, 1, 3))
        boxes_h = np.concatenate([c - h, c + h], axis=1).astype(np.float32)
        boxes = torch.from_numpy(boxes_h).to(dev)
        ids = torch.arange(1, K + 1, dtype=torch.int32, device=dev)
        out = {k: torch.empty(B, H * W, device=dev, dtype=torch.int32 if k == "label" else torch.float32) for k in ops.SCENE_BOUNDS_KEYS}

        def new_route():
            return ops.scene_bounds(zbuf, boxes, ids, depth_scale=10.0, bg_range=bg, source="box", pose=pose, intr=intr, out=out)

        def old_route():
            nears, fars = [], []
            for k in range(K):
                n, f = online_box_range(intr, pose, boxes_h[k, 0], boxes_h[k, 1], H, W, bg_range=(0.0, 0.0))
                nears.append(n); fars.append(f)
            zz = zbuf.view(K, B, H * W)
            covered = zz > 0
            labels = covered * ids.view(K, 1, 1)
            zs = torch.where(covered, zz, 100000 * torch.ones_like(zz))
            zmin, idx = torch.min(zs, dim=0)
            label = torch.gather(labels, 0, idx[None])[0]
            near = torch.where(label > 0, torch.gather(torch.stack(nears), 0, idx[None])[0], torch.full_like(zmin, bg[0]))
            far = torch.where(label > 0, torch.gather(torch.stack(fars), 0, idx[None])[0], torch.full_like(zmin, bg[1]))
            depth = torch.where(label > 0, (zmin / 1000) * 10.0, torch.zeros_like(zmin))
            return dict(z_near=near, z_far=far, label=label, depth=depth)

        r_new, r_old = new_route(), old_route()
        same = {k: bool(torch.equal(r_new[k], r_old[k].to(r_new[k].dtype))) for k in ops.SCENE_BOUNDS_KEYS}
        times = {}
        for name, fn in (("new", new_route), ("old", old_route), ("new_again", new_route), ("old_again", old_route)):
            times[name] = KB.timed(fn, a.iters, a.warmup)
        nbytes = (4 * K + 16) * B * H * W
        t_new = min(times["new"], times["new_again"])
        t_old = min(times["old"], times["old_again"])
        rows.append(dict(K=K, B=B, H=H, W=W, us_new=times["new"], us_new_again=times["new_again"], us_old=times["old"],
                         us_old_again=times["old_again"], speedup=t_old / t_new, algorithmic_bytes=nbytes,
                         hbm_fraction_of_8TBps=nbytes / (t_new * 1e-6) / HBM_PEAK, outputs_equal_to_old_route=same))
        print(json.dumps(rows[-1]))
    res = dict(bench="scene_bounds", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, source="box",
               sclk_before=clock_before, sclk_after=sclk(), rows=rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
