#!/usr/bin/env python3
"""Time the three ways to render colour detail below the mesh's vertex spacing (K35) on the rippled sphere of the
bake bench (V = 20,000, F = 39,200), B = 64 Fibonacci views of 480 x 640, in one run on one device:

  base          ops.mesh_raster(vcolor=) of the base mesh: today's vertex colours (the resolution limit)
  texels R      ops.mesh_raster(texels=) of the base mesh: depth + face plane + tp_face_texel_shade, R in {1, 4, 8}, plain and cull=True
  shade R       tp_face_texel_shade alone on a given face plane (the kernel's own time: 16 B per pixel + the gather)
  subdivided R  ops.mesh_raster(vcolor=) of the mesh subdivided R times (F R^2 faces), plain and cull=True, R in {4, 8}

    python tools/face_texel_bench.py [--out profiles/face_texels/shade.json] [--iters 20]

The outputs are compared before anything is timed: R = 1 against the base route within 1e-5; the texel route against the subdivided
route on the pixels where both see the same surface: at most 0.01 % of them may differ by more than 5e-5 (the bar of
tests/test_gpu_face_texels.py) and none by more than 2e-3, with coverage differing on at most 0.5 %.  The gate is wider than the tests'
because the subdivided route shades with the rasteriser's fp32 barycentrics, and its sub-faces at the silhouette of a 480 x 640 view
project to slivers far thinner than a pixel; the kernel itself is held to the fp64 restatement by the tests.  Device events around
many calls after a warm-up, three repeats per route, alternating, medians; the shader clock comes from ops.clock_probe before and after.

--fit: the adjoint instead (K36 tp_face_texel_shade_bwd), on the same workload with a dense random gradient:

  shade R          tp_face_texel_shade alone, as above: the forward beside which every adjoint time is read
  adjoint R        ops.face_texel_shade_bwd per slot ([F,T,3]), R in {1, 4, 8}; "+weight" with the coverage output
  adjoint nodes R  the same through the node index of the subdivided mesh ([U,3])
  fit R=4          FaceTexelFitter.fit over the 64 views with 0 and with 1 iteration: the difference is one iteration

    python tools/face_texel_bench.py --fit [--out profiles/face_texel_fit/adjoint.json]

Each adjoint row carries the forward's time of the same run and the atomic bytes per second: 9 (12 with the coverage) 64-bit atomics, 72
(96) bytes, per covered pixel.  Before anything is timed the identity <shade(t), g> = <t, adjoint(g)> is checked in fp64 on the host.

--fit --lighting: the lit fit instead (K41 tp_face_texel_light), on the same workload, the R = 8 render relit view by
view as the photographs:

  light B=n <mode>   ops.face_texel_light on n views: "residual" (image given), "+sums", "operator" (no image), "+diag"
  torch B=n <mode>   the same rule composed in torch -- the comparator, not the code under test: the shading plane from
                     ops.photo_lighting's apply of an all-ones rendering (a fit that keeps nothing applies the incoming light), then the
                     elementwise passes; checked bit for bit against the fused call before anything is timed
  fit R=4 ...        FaceTexelFitter.fit plain with 0 and 1 iteration, and lit (one round) with 0 and 1 iteration and without the
                     light step: the differences are one plain iteration, one lit iteration and one light step

    python tools/face_texel_bench.py --fit --lighting [--out profiles/face_texel_light/light.json]

Each K41 row carries the bytes it moves (8 B per pixel for face and weight, 12 B per pixel for grad, 12 more with diag, 12 B per covered
pixel for colour and 12 more for image) and their share of 8 TB/s.

--fit --robust: the robust weights instead (K42 tp_robust_weight), on the same workload: the R = 8 render as the
photographs, the R = 4 render as the model, the inner pixels as the base weight:

  robust B=n <kind>      ops.robust_weight on n views (8 and all): "tukey", "huber", "tukey scale_in" (no median), and "tukey perfect fit"
                         (model = photograph: every q is 0, every key of a wave lands in one histogram bin at every level)
  torch B=n tukey        the same rule composed in torch -- the comparator, not the code under test: q in fp64, torch.kthvalue per image
                         over the counted pixels (which reads each image's count back), the weight in fp64; checked bit for bit against the
                         call before anything is timed
  fit R=4 ...            FaceTexelFitter.fit plain and robust (one round) with 0 iterations: the difference is one weight step

    python tools/face_texel_bench.py --fit --robust [--out profiles/robust_weight/robust.json]

Each K42 row carries the bytes its passes move -- 52 B per pixel: 24 B model and image, 4 B weight and 4 B of key written by the first pass,
4 B of key read by each of the second and third, 4 B key, 4 B weight and 4 B out by the last (44 B without a weight, 36 B with scale_in: one
pass) -- and their share of 8 TB/s, the floor if every pass went to HBM."""
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


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=20, warmup=3, repeats=3)
    ap.add_argument("--lat", type=int, default=99)
    ap.add_argument("--lon", type=int, default=200)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--H", type=int, default=480)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--fit", action="store_true", help="time the adjoint (K36) and one fitter iteration instead")
    ap.add_argument("--lighting", action="store_true", help="with --fit: time K41 and the lit fit instead")
    ap.add_argument("--robust", action="store_true", help="with --fit: time K42 and the robust fit's weight step instead")
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import face_texels as FT, ops, texture_bake as TB
    if not torch.cuda.is_available():
        raise SystemExit("face_texel_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    clock_before = KB.shader_clock()
    t_start = time.time()
    H, W, B, focal, dist = a.H, a.W, a.views, 1000.0 * a.W / 640.0, 400.0
    pose = torch.from_numpy(TB.sphere_view_poses(B, dist).astype(np.float32)).to(dev)
    K = torch.tensor([[focal, 0.0, W / 2.0], [0.0, focal, H / 2.0], [0.0, 0.0, 1.0]], device=dev)[None].repeat(B, 1, 1).contiguous()
    v_np, f_np = uv_sphere(a.lat, a.lon, ripple=0.15)
    colour = lambda p: (0.5 + 0.5 * np.sin(np.asarray(p, np.float64) / 3.0 + np.array([0.0, 1.0, 2.0]))).astype(np.float32)      # 3 mm period
    verts, faces = torch.from_numpy(v_np).to(dev), torch.from_numpy(f_np).to(dev)
    vcol = torch.from_numpy(colour(v_np)).to(dev)
    raster = lambda **kw: ops.mesh_raster(verts, faces, pose, K, H=H, W=W, face_ids=False, normals=False, **kw)
    base = raster(vcolor=vcol)
    covered = base["zbuf"] > 0
    n_cov = int(covered.sum())
    if a.lighting and not a.fit:
        ap.error("--lighting comes with --fit")
    if a.robust and (not a.fit or a.lighting):
        ap.error("--robust comes with --fit and without --lighting")
    if a.fit:
        return (bench_robust if a.robust else bench_light if a.lighting else bench_fit)(a, locals())
    routes, iters, checks, meshes = {"base": lambda: raster(vcolor=vcol), "base cull": lambda: raster(vcolor=vcol, cull=True)}, {}, {}, {}
    heavy = max(2, a.iters // 10)
    for R in (1, 4, 8):
        vs, fs, ni = FT.subdivide(v_np, f_np, R)
        texels = torch.from_numpy(FT.texels_from_nodes(colour(vs), ni)).to(dev)
        got = raster(texels=texels)
        face = got["face"]
        out = torch.empty(B, H, W, 3, device=dev)
        routes["texels R=%d" % R] = lambda texels=texels: raster(texels=texels)
        routes["texels R=%d cull" % R] = lambda texels=texels: raster(texels=texels, cull=True)
        routes["shade R=%d" % R] = lambda texels=texels, face=face, out=out: ops.face_texel_shade(face, verts, faces, texels, pose, K, out=out)
        meshes[R] = dict(R=R, texels_per_face=int(texels.shape[1]), texel_bytes=int(texels.numel() * 4), nodes=len(vs), faces_subdivided=len(fs))
        if R == 1:
            d = float((got["rgb"] - base["rgb"]).abs().max())
            checks["R=1 against base"] = d
            if not d <= 1e-5:
                raise SystemExit("face_texel_bench: R = 1 differs from the vertex-colour route by %.3g; nothing was timed" % d)
            continue
        vs_d, fs_d, col_d = torch.from_numpy(vs).to(dev), torch.from_numpy(fs).to(dev), torch.from_numpy(colour(vs)).to(dev)
        sub = lambda cull, vs_d=vs_d, fs_d=fs_d, col_d=col_d: ops.mesh_raster(vs_d, fs_d, pose, K, H=H, W=W, vcolor=col_d, face_ids=False, normals=False, cull=cull)
        for cull in (False, True):
            s = sub(cull)
            # the same surface won in both routes: at a fold of the rippled sphere the two meshes' fp32 depth tests may pick different
            # layers for a pixel, which is the rasteriser's difference, not the shading's; such pixels count as differing coverage
            both = covered & (s["zbuf"] > 0) & ((got["zbuf"] - s["zbuf"]).abs() <= 1e-4 * got["zbuf"].abs())
            diff = (got["rgb"] - s["rgb"]).abs()[both]
            d, above = float(diff.max()), int((diff.max(-1).values > 5e-5).sum())
            differ = int((covered != (s["zbuf"] > 0)).sum()) + int((covered & (s["zbuf"] > 0) & ~both).sum())
            checks["R=%d against subdivided%s" % (R, " cull" if cull else "")] = dict(max_colour_difference=d, pixels_above_5e_5=above, pixels_compared=int(both.sum()),
                                                                                   coverage_differs=differ)
            if not d <= 2e-3 or above > 1e-4 * int(both.sum()) or differ > 0.005 * n_cov:
                raise SystemExit("face_texel_bench: R = %d: the texel route and the subdivided route disagree (%.3g, %d pixels); nothing was timed" % (R, d, differ))
            name = "subdivided R=%d%s" % (R, " cull" if cull else "")
            routes[name] = lambda cull=cull, sub=sub: sub(cull)
            if not cull:
                iters[name] = heavy
    iters = {name: iters.get(name, a.iters) for name in routes}
    med, times = KB.race(routes, iters, a.warmup, a.repeats)
    pixels = B * H * W
    rows = [dict(route=name, us_per_call=med[name], us_all_repeats=times[name], frames_per_second=B / (med[name] * 1e-6), iters=iters[name]) for name in routes]
    for row in rows:
        if row["route"].startswith("shade"):
            row["streamed_bytes"] = 16 * pixels                      # 4 B face read + 12 B rgb written per pixel
            row["streamed_bytes_per_second"] = 16 * pixels / (row["us_per_call"] * 1e-6)
        print(json.dumps(row), flush=True)
    res = dict(bench="face_texels", device=torch.cuda.get_device_name(0), V=len(v_np), F=len(f_np), B=B, H=H, W=W, covered_pixels=n_cov,
               covered_share=n_cov / pixels, iters=a.iters, warmup=a.warmup, repeats=a.repeats, shader_clock_ghz_before=clock_before,
               shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start, textures=list(meshes.values()), checks=checks, rows=rows)
    KB.finish(res, a.out)


def bench_fit(a, env):
    import torch
    from texpose_amd import face_texels as FT, ops
    dev, B, H, W, pose, K, verts, faces = (env[k] for k in ("dev", "B", "H", "W", "pose", "K", "verts", "faces"))
    v_np, f_np, colour, covered, n_cov = (env[k] for k in ("v_np", "f_np", "colour", "covered", "n_cov"))
    face = ops.mesh_raster(verts, faces, pose, K, H=H, W=W, normals=False)["face"]
    g = torch.randn(B, H, W, 3, device=dev)
    routes, checks, meshes = {}, {}, []
    for R in (1, 4, 8):
        vs, _, ni = FT.subdivide(v_np, f_np, R)
        U = len(vs)
        ni_d = torch.from_numpy(ni).to(dev).to(torch.int32)
        texels = torch.from_numpy(FT.texels_from_nodes(colour(vs), ni)).to(dev)
        out, grad, grad_n = torch.empty(B, H, W, 3, device=dev), torch.empty_like(texels), torch.empty(U, 3, device=dev)
        lhs = float((ops.face_texel_shade(face, verts, faces, texels, pose, K).double() * g.double()).sum())
        rhs = float((texels.double() * ops.face_texel_shade_bwd(face, verts, faces, g, pose, K, R=R).double()).sum())
        checks["R=%d adjoint identity" % R] = dict(lhs=lhs, rhs=rhs)
        if not abs(lhs - rhs) <= 1e-6 * float(g.abs().double().sum()):
            raise SystemExit("face_texel_bench: R = %d: <S t, g> = %.9g but <t, S^T g> = %.9g; nothing was timed" % (R, lhs, rhs))
        bwd = lambda R=R, **kw: ops.face_texel_shade_bwd(face, verts, faces, g, pose, K, R=R, **kw)
        routes["shade R=%d" % R] = lambda texels=texels, out=out: ops.face_texel_shade(face, verts, faces, texels, pose, K, out=out)
        routes["adjoint R=%d" % R] = lambda bwd=bwd, grad=grad: bwd(out=grad)
        routes["adjoint R=%d +weight" % R] = lambda bwd=bwd, grad=grad: bwd(out=grad, weight=True)
        routes["adjoint nodes R=%d" % R] = lambda bwd=bwd, ni_d=ni_d, U=U, grad_n=grad_n: bwd(node_index=ni_d, U=U, out=grad_n)
        routes["adjoint nodes R=%d +weight" % R] = lambda bwd=bwd, ni_d=ni_d, U=U, grad_n=grad_n: bwd(node_index=ni_d, U=U, out=grad_n, weight=True)
        meshes.append(dict(R=R, slots=int(texels.shape[0] * texels.shape[1]), nodes=U))
    photo = ops.face_texel_shade(face, verts, faces, texels, pose, K)            # (the R = 8 render: a photograph finer than the R = 4 fit)
    fitters = {}
    for iters in (0, 1):
        fitters[iters] = FT.FaceTexelFitter(v_np, f_np, 4, H, W, dev, iters=iters)
        for c in range(0, B, 16):
            fitters[iters].add_views(photo[c:c + 16], pose[c:c + 16], K[c:c + 16], face=face[c:c + 16])
        routes["fit R=4 iters=%d" % iters] = fitters[iters].fit
    med, times = KB.race(routes, a.iters, a.warmup, a.repeats)
    rows = []
    for name in routes:
        row = dict(route=name, us_per_call=med[name], us_all_repeats=times[name])
        if name.startswith("adjoint"):
            per_pixel = 96 if name.endswith("+weight") else 72
            row.update(forward_us_same_run=med["shade R=%s" % name.split("R=")[1].split()[0]], atomic_bytes=per_pixel * n_cov,
                       atomic_bytes_per_second=per_pixel * n_cov / (med[name] * 1e-6))
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(bench="face_texel_fit", device=torch.cuda.get_device_name(0), V=len(v_np), F=len(f_np), B=B, H=H, W=W, covered_pixels=n_cov,
               covered_share=n_cov / (B * H * W), iters=a.iters, warmup=a.warmup, repeats=a.repeats, shader_clock_ghz_before=env["clock_before"],
               shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - env["t_start"], textures=meshes, checks=checks,
               fit_iteration_us=med["fit R=4 iters=1"] - med["fit R=4 iters=0"], rows=rows)
    KB.finish(res, a.out)


def bench_light(a, env):
    import torch
    from texpose_amd import face_texels as FT, ops
    dev, B, H, W, pose, K, verts, faces = (env[k] for k in ("dev", "B", "H", "W", "pose", "K", "verts", "faces"))
    v_np, f_np, colour, n_cov = (env[k] for k in ("v_np", "f_np", "colour", "n_cov"))
    F = len(f_np)
    face = ops.mesh_raster(verts, faces, pose, K, H=H, W=W, normals=False)["face"]
    covered = (face >= 0) & (face < F)
    zbuf = torch.where(covered, 1.0, -1.0).float()
    nothing = torch.zeros(B, H, W, dtype=torch.uint8, device=dev)
    vs, _, ni = FT.subdivide(v_np, f_np, 8)
    texels = torch.from_numpy(FT.texels_from_nodes(colour(vs), ni)).to(dev)
    unlit = ops.face_texel_shade(face, verts, faces, texels, pose, K)
    rs = np.random.RandomState(0)                                    # one light per view: ambient, a directional part of 0.45 of it, a bias
    amb = np.array([0.70, 0.75, 0.65]) * rs.uniform(0.8, 1.25, (B, 1))
    d = rs.randn(B, 3)
    d[:, 2] = -np.abs(d[:, 2]) - 0.3
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    light = torch.from_numpy(np.concatenate([amb[:, :, None], 0.45 * amb[:, :, None] * d[:, None, :],
                                             (np.array([0.05, 0.10, 0.08]) * rs.uniform(0, 1, (B, 1)))[:, :, None]], 2).astype(np.float32)).to(dev)
    apply = lambda rgb, l, n: ops.photo_lighting(verts, faces, face[:n], zbuf[:n], rgb, pose[:n], rgb, tau=0.5, light=l, mask=nothing[:n])["rgb"]
    photo = apply(unlit, light, B)
    weight = FT.inner_coverage(face, F).float()
    colour_plane = (unlit * 0.9).contiguous()                        # a rendering that leaves a residual
    unbiased = light.clone()
    unbiased[:, :, 4] = 0.0
    ones = torch.ones(B, H, W, 3, device=dev)
    off = torch.zeros((), device=dev)
    on = (covered & (weight > 0))[..., None]                         # (an uncovered or unweighted pixel is +0, whatever the products' signs)

    def composed(n, image, diag=False, sums=False):
        s = apply(ones[:n], unbiased[:n], n)
        ms = weight[:n, ..., None] * s
        q = s * colour_plane[:n]
        out = {}
        if image:
            e = photo[:n] - (q + light[:n, None, None, :, 4])
            out["grad"] = torch.where(on[:n], ms * e, off)
            if sums:
                e64 = e.double()
                t = weight[:n].double() * ((e64[..., 0] * e64[..., 0] + e64[..., 1] * e64[..., 1]) + e64[..., 2] * e64[..., 2])
                out["sums"] = torch.stack([(t * covered[:n]).sum((1, 2)), (weight[:n].double() * covered[:n]).sum((1, 2))], 1)
        else:
            out["grad"] = torch.where(on[:n], ms * q, off)
        if diag:
            out["diag"] = torch.where(on[:n], ms * s, off)
        return out

    routes, checks = {}, {}
    modes = {"residual": dict(image=True), "residual +sums": dict(image=True, sums=True), "residual +diag +sums": dict(image=True, diag=True, sums=True),
             "operator": dict(image=False), "operator +diag": dict(image=False, diag=True)}
    for n in (B, 8):
        outs = dict(grad=torch.empty(n, H, W, 3, device=dev), diag=torch.empty(n, H, W, 3, device=dev), sums=torch.empty(n, 2, device=dev, dtype=torch.float64))
        ws = ops.face_texel_light_workspace(n, H, W, dev)
        for name, m in modes.items():
            kw = dict(image=photo[:n] if m["image"] else None, weight=weight[:n], diag=m.get("diag", False), sums=m.get("sums", False))
            fused = lambda n=n, kw=kw, outs=outs, ws=ws: ops.face_texel_light(face[:n], verts, faces, colour_plane[:n], pose[:n], light[:n], workspace=ws,
                                                                              out={k: outs[k] for k in ("grad",) + (("diag",) if kw["diag"] else ()) + (("sums",) if kw["sums"] else ())}, **kw)
            torch_way = lambda n=n, m=m: composed(n, m["image"], m.get("diag", False), m.get("sums", False))
            got, want = fused(), torch_way()
            equal = {k: bool(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32))) if k != "sums"
                     else float(((got[k] - want[k]).abs() / want[k].abs().clamp_min(1e-300)).max()) for k in got}
            checks["B=%d %s" % (n, name)] = equal
            if not all(v is True or (v is not False and v <= 1e-12) for v in equal.values()):
                raise SystemExit("face_texel_bench: B = %d %s: the fused call and the torch composition disagree (%s); nothing was timed" % (n, name, equal))
            routes["light B=%d %s" % (n, name)] = fused
            routes["torch B=%d %s" % (n, name)] = torch_way
    def fitter(**kw):
        f = FT.FaceTexelFitter(v_np, f_np, 4, H, W, dev, **kw)
        for c in range(0, B, 16):
            f.add_views(photo[c:c + 16], pose[c:c + 16], K[c:c + 16], face=face[c:c + 16])
        return f

    for iters in (0, 1):
        routes["fit R=4 plain iters=%d" % iters] = fitter(iters=iters).fit
        routes["fit R=4 lit rounds=1 iters=%d" % iters] = fitter(iters=iters, lighting=True, rounds=1).fit
    held = fitter(iters=0, lighting=True, rounds=1)
    routes["fit R=4 lit rounds=1 iters=0 no light step"] = lambda: held.fit(lights=light, light_step=False)
    med, times = KB.race(routes, a.iters, a.warmup, a.repeats)
    rows = []
    for name in routes:
        row = dict(route=name, us_per_call=med[name], us_all_repeats=times[name])
        if name.startswith("light"):
            n = int(name.split("B=")[1].split()[0])
            cov = int(covered[:n].sum())
            moved = n * H * W * (8 + 12 + (12 if "+diag" in name else 0)) + cov * (24 if "residual" in name else 12)
            row.update(bytes_moved=moved, share_of_8_tb_per_s=moved / (med[name] * 1e-6) / 8e12, torch_us_same_run=med["torch" + name[5:]],
                       speedup_over_torch=med["torch" + name[5:]] / med[name])
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(bench="face_texel_light", device=torch.cuda.get_device_name(0), V=len(v_np), F=F, B=B, H=H, W=W, covered_pixels=n_cov,
               covered_share=n_cov / (B * H * W), iters=a.iters, warmup=a.warmup, repeats=a.repeats, shader_clock_ghz_before=env["clock_before"],
               shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - env["t_start"], checks=checks,
               plain_iteration_us=med["fit R=4 plain iters=1"] - med["fit R=4 plain iters=0"],
               lit_iteration_us=med["fit R=4 lit rounds=1 iters=1"] - med["fit R=4 lit rounds=1 iters=0"],
               light_step_us=med["fit R=4 lit rounds=1 iters=0"] - med["fit R=4 lit rounds=1 iters=0 no light step"], rows=rows)
    KB.finish(res, a.out)


def bench_robust(a, env):
    import torch
    from texpose_amd import face_texels as FT, ops
    dev, B, H, W, pose, K, verts, faces = (env[k] for k in ("dev", "B", "H", "W", "pose", "K", "verts", "faces"))
    v_np, f_np, colour, n_cov = (env[k] for k in ("v_np", "f_np", "colour", "n_cov"))
    F = len(f_np)
    face = ops.mesh_raster(verts, faces, pose, K, H=H, W=W, normals=False)["face"]

    def shade(R):
        vs, _, ni = FT.subdivide(v_np, f_np, R)
        return ops.face_texel_shade(face, verts, faces, torch.from_numpy(FT.texels_from_nodes(colour(vs), ni)).to(dev), pose, K)

    photo, model = shade(8), shade(4)
    weight = FT.inner_coverage(face, F).float()
    sigma = torch.full((B,), 0.03, device=dev)
    c_tukey, sigma_min = 4.685, 1.0 / 255.0

    def composed(n):
        """the header's rule for Tukey's weight, image by image"""
        e = photo[:n].double() - model[:n].double()
        q = (((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) / 3.0).float()
        counted = torch.isfinite(weight[:n]) & (weight[:n] > 0) & torch.isfinite(q)
        out, med, cnt = torch.zeros(n, H, W, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev, dtype=torch.int32)
        for b in range(n):
            qb = q[b][counted[b]]
            cnt[b] = qb.numel()
            if qb.numel():
                med[b] = torch.kthvalue(qb, (qb.numel() - 1) // 2 + 1).values
        s2 = torch.clamp_min((1.4826 * 1.4826) * med.double(), float(np.float32(sigma_min)) ** 2)
        u2 = q.double() / ((float(np.float32(c_tukey)) ** 2) * s2)[:, None, None]
        w = torch.where(u2 < 1.0, (1.0 - u2) * (1.0 - u2), torch.zeros_like(u2))
        out = torch.where(counted, (weight[:n].double() * w).float(), out)
        return dict(weight=out, median_q=med, scale=torch.sqrt(s2).float(), count=cnt)

    routes, checks, moved = {}, {}, {}
    for n in (B, 8):
        ws = ops.robust_weight_workspace(n, H, W, dev)
        outs = dict(weight=torch.empty(n, H, W, device=dev), median_q=torch.empty(n, device=dev), scale=torch.empty(n, device=dev),
                    count=torch.empty(n, device=dev, dtype=torch.int32))
        call = lambda n=n, ws=ws, outs=outs, m=model, **kw: ops.robust_weight(m[:n], photo[:n], weight=weight[:n], workspace=ws, out=outs, **kw)
        got, want = {k: v.clone() for k, v in call().items()}, composed(n)
        equal = {k: bool(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32))) for k in ("weight", "median_q", "count")}
        checks["B=%d tukey" % n] = dict(equal, median_q=got["median_q"].tolist()[:4], kept=float(got["weight"].sum() / weight[:n].sum()))
        if not all(equal.values()):
            raise SystemExit("face_texel_bench: B = %d: the call and the torch composition disagree (%s); nothing was timed" % (n, equal))
        routes["robust B=%d tukey" % n] = call
        routes["robust B=%d huber" % n] = lambda call=call: call(kind="huber")
        routes["robust B=%d tukey scale_in" % n] = lambda call=call, n=n: call(scale_in=sigma[:n])
        routes["robust B=%d tukey perfect fit" % n] = lambda call=call: call(m=photo)
        routes["torch B=%d tukey" % n] = lambda n=n: composed(n)
        for name in ("tukey", "huber", "tukey perfect fit"):
            moved["robust B=%d %s" % (n, name)] = 52 * n * H * W
        moved["robust B=%d tukey scale_in" % n] = 36 * n * H * W

    def fitter(**kw):
        f = FT.FaceTexelFitter(v_np, f_np, 4, H, W, dev, iters=0, **kw)
        for c in range(0, B, 16):
            f.add_views(photo[c:c + 16], pose[c:c + 16], K[c:c + 16], face=face[c:c + 16])
        return f

    routes["fit R=4 plain iters=0"] = fitter().fit
    routes["fit R=4 robust rounds=1 iters=0"] = fitter(robust="tukey", robust_rounds=1).fit
    med, times = KB.race(routes, a.iters, a.warmup, a.repeats)
    rows = []
    for name in routes:
        row = dict(route=name, us_per_call=med[name], us_all_repeats=times[name])
        if name in moved:
            row.update(bytes_moved=moved[name], share_of_8_tb_per_s=moved[name] / (med[name] * 1e-6) / 8e12)
        if name.endswith(" tukey") and name.startswith("robust"):
            row.update(torch_us_same_run=med["torch" + name[6:]], speedup_over_torch=med["torch" + name[6:]] / med[name])
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(bench="robust_weight", device=torch.cuda.get_device_name(0), V=len(v_np), F=F, B=B, H=H, W=W, covered_pixels=n_cov,
               covered_share=n_cov / (B * H * W), weighted_share=float(weight.sum()) / (B * H * W), iters=a.iters, warmup=a.warmup, repeats=a.repeats,
               shader_clock_ghz_before=env["clock_before"], shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - env["t_start"], checks=checks,
               weight_step_us=med["fit R=4 robust rounds=1 iters=0"] - med["fit R=4 plain iters=0"], rows=rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
