#!/usr/bin/env python3
"""Time the VSD kernel (tp_vsd, K26: three launches in one call) against `pose_error.vsd_torch`, the same definition in plain torch
ops in fp64, on the same device in the same run: 480 x 640, B = 8 and 64 pose pairs with a test plane each (Ft = B), T = 10 tolerances.
Both routes read the same planes; their counts must be equal (planes of integer millimetres under intrinsics whose distance factor is
exactly 1, so no decision is near a tie) and their errors equal before anything is timed.  Device events around many iterations after
a warm-up, three repeats per route, alternating, medians; the shader clock comes from ops.clock_probe before and after.

    python tools/vsd_bench.py [--out profiles/pose_errors/vsd.json] [--iters 50]

Reports, per shape: microseconds per call of both routes, their ratio, and the kernel's share of the 8 TB/s HBM peak from its algorithmic
bytes, 3 x 4 x H x W per pose pair (a share of peak of the CALL: the three launches and the gaps between them are inside the events)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kernel_bench as KB  # noqa: E402

HBM_PEAK = 8.0e12


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=50, warmup=5, repeats=3)
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import ops, pose_error as PE
    if not torch.cuda.is_available():
        raise SystemExit("vsd_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)

    clock_before = KB.shader_clock()
    t_start = time.time()
    H, W, T = 480, 640, 10
    rows = []
    for B in (8, 64):
        zg = rs.randint(400, 1201, (B, H, W)).astype(np.float32)
        ze = zg + rs.randint(-40, 41, zg.shape).astype(np.float32)
        dt = zg + rs.randint(-30, 31, zg.shape).astype(np.float32)
        for plane, value, share in ((zg, -1.0, 0.6), (ze, -1.0, 0.6), (dt, 0.0, 0.05)):
            plane[rs.uniform(size=plane.shape) < share] = value
        K = np.tile(np.array([[2.0 ** 40, 0.0, W / 2], [0.0, 2.0 ** 40, H / 2], [0.0, 0.0, 1.0]], np.float32), (B, 1, 1))
        tau = np.tile(np.arange(1, T + 1, dtype=np.float32)[None] * 4.0, (B, 1))
        ze, zg, dt, K, tau = (torch.from_numpy(x).to(dev) for x in (ze, zg, dt, K, tau))
        out = dict(err=torch.empty(B, T, device=dev), counts=torch.empty(B, 2 + T, dtype=torch.int32, device=dev))
        kernel = lambda: ops.vsd(ze, zg, dt, K, tau, delta_mm=15.0, out=out)
        plain = lambda: PE.vsd_torch(ze, zg, dt, K, tau, 15.0)
        got, want = kernel(), plain()
        if not (torch.equal(got["counts"], want["counts"]) and torch.equal(got["err"], want["err"])):
            raise SystemExit("vsd_bench: the two routes disagree at B = %d; nothing was timed" % B)
        med, times = KB.race({"tp_vsd": kernel, "torch": plain}, {"tp_vsd": a.iters, "torch": max(3, a.iters // 10)}, a.warmup, a.repeats)
        nbytes = 3 * 4 * H * W * B
        rows.append(dict(B=B, Ft=B, H=H, W=W, T=T, us=med, us_all_repeats=times, torch_over_tp_vsd=med["torch"] / med["tp_vsd"],
                         algorithmic_bytes=nbytes, bytes_per_second=nbytes / (med["tp_vsd"] * 1e-6),
                         hbm_fraction_of_8TBps=nbytes / (med["tp_vsd"] * 1e-6) / HBM_PEAK, outputs_equal=True,
                         n_U=int(want["counts"][:, 0].sum()), n_I=int(want["counts"][:, 1].sum())))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(bench="vsd", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, repeats=a.repeats,
               shader_clock_ghz_before=clock_before, shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start, rows=rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
