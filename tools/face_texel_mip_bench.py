#!/usr/bin/env python3
"""Time the mip shade (K43b tp_face_texel_shade_mip) against the point-sampled shade (K35 tp_face_texel_shade) in the
same run, on the rippled sphere of the bake bench (V = 20,000, F = 39,200) with an R = 8 texture and its four levels, 8 and 64
Fibonacci views of 480 x 640 on one device:

  k35 B=n            tp_face_texel_shade on the face plane: the comparator
  mip B=n magnified  tp_face_texel_shade_mip with every pixel at d <= 1 (footprint 2^-20): one level, K35's own work plus d
  mip B=n blending   ... at the bench's own distance with footprint 4: most covered pixels blend two levels
  mip B=n beyond     ... with every pixel beyond the last level (footprint 2^40): one level, the coarsest
  build_mips         face_texels.build_mips of the texture: the three K43a launches alone (device events), and the whole call with
                     the host's CSR build (host clock around a synchronise)

    python tools/face_texel_mip_bench.py [--out profiles/face_texel_mip/mip.json] [--iters 20]

Before anything is timed the three cases are checked: magnified equals K35 bit for bit, beyond equals K35 on the last level's texels bit
for bit, and the share of covered pixels of the blending case that equal no single level's K35 render (those that blend) is counted.
Each row carries the ratio to K35 of the same run and batch, and the streamed bytes (4 B face read + 12 B rgb written per pixel; the
gathers are cache traffic) with their share of 8 TB/s.  Device events around many calls after a warm-up, three repeats per route,
alternating, medians; the shader clock comes from ops.clock_probe before and after."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import kernel_bench as KB  # noqa: E402
from texture_bake_ref import uv_sphere  # noqa: E402  (numpy only: the tests' mesh generators; needs the repository's tests/ folder)

CASES = {"magnified": 2.0 ** -20, "blending": 4.0, "beyond": 2.0 ** 40}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=20, warmup=3, repeats=3)
    ap.add_argument("--lat", type=int, default=99)
    ap.add_argument("--lon", type=int, default=200)
    ap.add_argument("--H", type=int, default=480)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--res", type=int, default=8, metavar="R")
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import face_texels as FT, ops, texture_bake as TB
    if not torch.cuda.is_available():
        raise SystemExit("face_texel_mip_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    clock_before = KB.shader_clock()
    t_start = time.time()
    H, W, R, focal, dist = a.H, a.W, a.res, 1000.0 * a.W / 640.0, 400.0
    v_np, f_np = uv_sphere(a.lat, a.lon, ripple=0.15)
    colour = lambda p: (0.5 + 0.5 * np.sin(np.asarray(p, np.float64) / 3.0 + np.array([0.0, 1.0, 2.0]))).astype(np.float32)      # 3 mm period
    verts, faces = torch.from_numpy(v_np).to(dev), torch.from_numpy(f_np).to(dev)
    vs, _, ni = FT.subdivide(v_np, f_np, R)
    texels = torch.from_numpy(FT.texels_from_nodes(colour(vs), ni)).to(dev)
    t0 = time.time()
    mips = FT.build_mips(v_np, f_np, texels)
    torch.cuda.synchronize()
    first_build_s = time.time() - t0
    slot_pairs = [tuple(torch.from_numpy(t).to(dev) for t in FT.mip_slots(v_np, f_np, R >> l)) for l in range(1, mips.L)]

    def reduce_all():
        for l, (ptr, lst) in enumerate(slot_pairs, 1):
            ops.face_texel_mip_reduce(mips.level(l - 1), ptr, lst, out=mips.level(l))

    def build_whole():
        FT.build_mips(v_np, f_np, texels)
        torch.cuda.synchronize()

    routes, checks, batches = {}, {}, {}
    for B in (8, 64):
        pose = torch.from_numpy(TB.sphere_view_poses(64, dist).astype(np.float32))[:B].contiguous().to(dev)
        K = torch.tensor([[focal, 0.0, W / 2.0], [0.0, focal, H / 2.0], [0.0, 0.0, 1.0]], device=dev)[None].repeat(B, 1, 1).contiguous()
        face = ops.mesh_raster(verts, faces, pose, K, H=H, W=W, normals=False)["face"]
        covered = (face >= 0) & (face < len(f_np))
        out = torch.empty(B, H, W, 3, device=dev)
        single = [ops.face_texel_shade(face, verts, faces, mips.level(l).contiguous(), pose, K) for l in range(mips.L)]
        got = {name: ops.face_texel_shade_mip(face, verts, faces, mips, pose, K, footprint=fp) for name, fp in CASES.items()}
        same = lambda x, y: bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))
        blends = covered.clone()
        for s in single:
            blends &= (got["blending"] != s).any(-1)
        checks["B=%d" % B] = dict(magnified_equals_k35=same(got["magnified"], single[0]), beyond_equals_k35_on_last_level=same(got["beyond"], single[-1]),
                                  blending_share_of_covered=float(blends.sum()) / max(1, int(covered.sum())))
        if not (checks["B=%d" % B]["magnified_equals_k35"] and checks["B=%d" % B]["beyond_equals_k35_on_last_level"]):
            raise SystemExit("face_texel_mip_bench: B = %d: the mip shade's single-level ends differ from K35 (%s); nothing was timed" % (B, checks["B=%d" % B]))
        batches[B] = dict(pixels=B * H * W, covered_pixels=int(covered.sum()))
        level0 = mips.level(0)
        routes["k35 B=%d" % B] = lambda face=face, pose=pose, K=K, out=out: ops.face_texel_shade(face, verts, faces, level0, pose, K, out=out)
        for name, fp in CASES.items():
            routes["mip B=%d %s" % (B, name)] = lambda face=face, pose=pose, K=K, out=out, fp=fp: ops.face_texel_shade_mip(face, verts, faces, mips, pose, K,
                                                                                                                      footprint=fp, out=out)
    routes["build_mips launches"] = reduce_all
    med, times = KB.race(routes, a.iters, a.warmup, a.repeats)
    whole = []
    for _ in range(a.repeats):
        t0 = time.time()
        build_whole()
        whole.append((time.time() - t0) * 1e6)
    rows = []
    for name in routes:
        row = dict(route=name, us_per_call=med[name], us_all_repeats=times[name])
        if " B=" in name:
            B = int(name.split("B=")[1].split()[0])
            moved = 16 * batches[B]["pixels"]
            row.update(streamed_bytes=moved, share_of_8_tb_per_s=moved / (med[name] * 1e-6) / 8e12, k35_us_same_run=med["k35 B=%d" % B],
                       ratio_to_k35=med[name] / med["k35 B=%d" % B])
        rows.append(row)
        print(json.dumps(row), flush=True)
    rows.append(dict(route="build_mips whole call (host clock)", us_per_call=float(np.median(whole)), us_all_repeats=whole, first_call_us=first_build_s * 1e6))
    print(json.dumps(rows[-1]), flush=True)
    res = dict(bench="face_texel_mip", device=torch.cuda.get_device_name(0), V=len(v_np), F=len(f_np), R=R, L=mips.L, H=H, W=W, batches=batches,
               chain_bytes=int(mips.packed.numel() * 4), iters=a.iters, warmup=a.warmup, repeats=a.repeats, shader_clock_ghz_before=clock_before,
               shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start, checks=checks, rows=rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
