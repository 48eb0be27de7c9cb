#!/usr/bin/env python3
"""Bake the texture a checkpoint has learned onto the object's CAD mesh as vertex colours: a coloured .ply that SurfelRenderer,
SceneBounds, the BOP writer and any BOP tool render at rasteriser speed (texpose_amd.texture_bake, K27 tp_texture_bake).

    python tools/bake_texture.py --checkpoint model.ckpt --ply 5=obj_000005.ply --scene scene.npz --out textured.ply --report bake.json

--scene: an .npz with pose [N,3,4] (the training poses, t in nerf.depth.scale units) and intr [3,3] or [N,3,3]; the default source of
views -- a field trained on an upper hemisphere should not be baked from below.  --sphere N --distance-mm D instead: N Fibonacci
look-at views around the model origin with a pinhole of --focal pixels (default 1.5 x the longer image side) centred in the image.
Per chunk of --chunk views: depth bounds, mask and the mesh's depth planes from SceneBounds, Graph.render_by_slices(mode="eval"), and
rgb_static is baked with opacity_static as the weight against those depth planes.  One --light-index per bake.
--report JSON: vertices, views, coverage (share of vertices some view reached), coloured (share with a positive weight), mean views per
vertex, filled and unseen counts, thresholds, seconds.  --verify re-renders the baked mesh with ops.mesh_raster at the bake poses and
prints (and stores) the PSNR against the NeRF views inside the mask; nothing is asserted on it.
--texel-res R (1 .. 64): also bake a face-texel texture of resolution R (texpose_amd.face_texels, K35: R x finer than
the vertices along every edge, no UV unwrap) from the same views and write it as <out>.texels.npz beside the PLY (texels, R and the
faces it belongs to; refine_poses.py --texels reads it).  The PLY still holds the vertex colours, now the texture's corner nodes;
--verify then re-renders through the texels, and the report gains 'texels' (R, nodes, coloured, filled, unseen, file).
--texel-mips [L] (with --texel-res): build the texture's mip chain (face_texels.build_mips, K43; L levels, default as
many as R allows) and let --verify re-render through ops.mesh_raster(texel_mips=), the shading with a minification filter; the report's
'texels' gains 'mip_levels'.  The files written are the same: the chain is rebuilt from level 0 wherever it is wanted.
--fit ITERS [--fit-lambda L] (with --texel-res): the views also go into a face_texels.FaceTexelFitter (inner pixels
of the mask, weight 1), and after the bake ITERS steps of preconditioned conjugate gradients from the baked nodes, with the baked nodes
as the prior (weight L, default 0.1), minimise the difference between the texel render and the views (K36 tp_face_texel_shade_bwd).
The fitted texels, clamped to [0, 1], are what <out>.texels.npz holds and the PLY's vertex colours are the fitted corner nodes; the
report gains 'fit' (iters, lam, rms_before, rms_after, on_prior: nodes too little seen to leave the prior); --verify prints and stores
the PSNR through the baked and through the fitted texels.  Without --fit nothing changes.
--fit-photos NPZ (with --fit): the fit runs against the photographs of an .npz with rgb [N,H,W,3] in [0, 1], pose [N,3,4] (object to
camera, t in mm) and intr [3,3] or [N,3,3] instead of the checkpoint's renders (inner pixels of the mesh's own coverage, weight 1); the
bake of the checkpoint's renders stays the prior and the start.  --fit-lighting [ROUNDS] (default 6): the texels are
fitted as an albedo under one first-order SH light per view (FaceTexelFitter(lighting=True), K41 tp_face_texel_light), ROUNDS
alternations of a light step and ITERS steps of CG; for photographs taken under lights that differ from view to view.  The report's
'fit' gains 'rms' (the whole series) and, with --fit-lighting, 'lighting' (rounds, light [N,3,5], status, flags, gain).
--fit-robust [tukey|huber] (default tukey) with --fit-robust-rounds N (default 6): the fit reweights every pixel round
by round by the robust weight of its residual (FaceTexelFitter(robust=...), K42 tp_robust_weight), for photographs with occluders or
highlights; N rounds of ITERS steps; 'fit' gains 'robust' (kind, rounds, scale and kept per view).  Not together with --fit-lighting.
Out of scope: texture atlases, view-dependent textures, reading a BOP scene's photographs (--fit-photos takes an .npz)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--ply", required=True, metavar="ID=PATH", help="the one object of the bake")
    ap.add_argument("--scene", default=None, help=".npz with pose [N,3,4] (NeRF units) and intr")
    ap.add_argument("--sphere", type=int, default=None, metavar="N", help="N Fibonacci views instead of --scene")
    ap.add_argument("--distance-mm", type=float, default=None, help="camera distance of the --sphere views")
    ap.add_argument("--focal", type=float, default=None, help="focal length in pixels of the --sphere views")
    ap.add_argument("--out", required=True, help="the coloured .ply")
    ap.add_argument("--report", default=None, metavar="JSON")
    ap.add_argument("--verify", action="store_true", help="re-render the baked mesh and print the PSNR against the NeRF views")
    ap.add_argument("--texel-res", type=int, default=None, metavar="R", help="also write <out>.texels.npz: face texels of resolution R")
    ap.add_argument("--texel-mips", type=int, nargs="?", const=0, default=None, metavar="L",
                    help="with --texel-res: --verify renders through the texture's mip chain of L levels (default: all R allows)")
    ap.add_argument("--fit", type=int, default=None, metavar="ITERS", help="with --texel-res: fit the texels to the views by ITERS steps of CG")
    ap.add_argument("--fit-lambda", type=float, default=0.1, metavar="L", help="weight of the baked texture as the fit's prior")
    ap.add_argument("--fit-photos", default=None, metavar="NPZ", help="with --fit: fit to these photographs (rgb, pose in mm, intr)")
    ap.add_argument("--fit-lighting", type=int, nargs="?", const=6, default=None, metavar="ROUNDS",
                    help="with --fit: fit an albedo under one SH-1 light per view, ROUNDS alternations (default 6)")
    ap.add_argument("--fit-robust", nargs="?", const="tukey", default=None, choices=("tukey", "huber"),
                    help="with --fit: reweight the pixels round by round with Tukey's (default) or Huber's weight of their residual")
    ap.add_argument("--fit-robust-rounds", type=int, default=None, metavar="N", help="with --fit-robust: rounds of reweighting (default 6)")
    ap.add_argument("--H", type=int, default=480)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--samples", type=int, default=None, help="nerf.sample_intvs")
    ap.add_argument("--source", choices=["box", "render", "none"], default=None, help="nerf.depth.range_source of the renders")
    ap.add_argument("--precision", choices=["fp32", "f16x3", "f16"], default=None)
    ap.add_argument("--light-index", type=int, default=0, help="row of latent_vars_light the views are lit with")
    ap.add_argument("--chunk", type=int, default=8, help="views per SceneBounds / bake call")
    ap.add_argument("--cos-min", type=float, default=None)
    ap.add_argument("--cover-min", type=float, default=None)
    ap.add_argument("--z-tol-mm", type=float, default=None)
    ap.add_argument("--slope", type=float, default=None)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if (a.scene is None) == (a.sphere is None):
        ap.error("either --scene or --sphere N --distance-mm D expected")
    if a.sphere is not None and not (a.sphere >= 1 and a.distance_mm and a.distance_mm > 0):
        ap.error("--sphere N needs N >= 1 and --distance-mm D > 0")
    if a.texel_res is not None and not 1 <= a.texel_res <= 64:
        ap.error("--texel-res R needs R in 1 .. 64")
    if a.texel_mips is not None:
        allowed = 0 if a.texel_res is None else (a.texel_res & -a.texel_res).bit_length()      # 1 + the number of times 2 divides R
        if not 0 <= a.texel_mips <= allowed or (a.texel_mips == 0 and a.texel_res is None):
            ap.error("--texel-mips [L] needs --texel-res R and 1 <= L <= %d (R must be a multiple of 2^(L-1))" % max(allowed, 1))
    if a.fit is not None and (a.texel_res is None or a.fit < 1 or not a.fit_lambda > 0):
        ap.error("--fit ITERS needs --texel-res R, ITERS >= 1 and --fit-lambda L > 0")
    if a.fit is None and (a.fit_photos is not None or a.fit_lighting is not None):
        ap.error("--fit-photos and --fit-lighting need --fit ITERS")
    if a.fit_lighting is not None and a.fit_lighting < 1:
        ap.error("--fit-lighting ROUNDS needs ROUNDS >= 1")
    if a.fit is None and (a.fit_robust is not None or a.fit_robust_rounds is not None):
        ap.error("--fit-robust and --fit-robust-rounds need --fit ITERS")
    if a.fit_robust is not None and a.fit_lighting is not None:
        ap.error("--fit-robust does not go together with --fit-lighting (DESIGN section 32, left out)")
    if a.fit_robust_rounds is not None and (a.fit_robust is None or a.fit_robust_rounds < 1):
        ap.error("--fit-robust-rounds N needs --fit-robust and N >= 1")
    import torch
    from texpose_amd import checkpoint as ck, ops
    from texpose_amd import face_texels as ft
    from texpose_amd import texture_bake as tb
    from texpose_amd.graph import Graph
    from texpose_amd.options import default_options
    from texpose_amd.scene_bounds import SceneBounds
    from texpose_amd.surfel import SurfelRenderer, load_ply
    dev = torch.device(a.device)
    opt = default_options(H=a.H, W=a.W, device=a.device)
    if a.samples:
        opt.nerf.sample_intvs = a.samples
    opt.nerf.sample_stratified = False
    if a.precision:
        opt.arch.mlp_precision = a.precision
    source = a.source or opt.nerf.depth.range_source
    blob = torch.load(a.checkpoint, map_location=dev, weights_only=False)
    graph = Graph(opt).to(dev)
    graph.attach_latents(blob["graph"]["latent_vars_light.weight"].shape[0], opt)
    ck.restore_checkpoint(graph, blob, resume=False)
    oid, path = a.ply.split("=", 1)
    verts, faces, _ = load_ply(path)
    scale = float(opt.nerf.depth.scale)
    if a.scene is not None:
        scene = np.load(a.scene)
        pose = torch.from_numpy(np.asarray(scene["pose"], dtype=np.float32).reshape(-1, 3, 4))
        intr = torch.from_numpy(np.asarray(scene["intr"], dtype=np.float32))
    else:
        pose = tb.poses_to_nerf_units(torch.from_numpy(tb.sphere_view_poses(a.sphere, a.distance_mm)), scale).float()
        f = a.focal or 1.5 * max(a.H, a.W)
        intr = torch.tensor([[f, 0.0, a.W / 2.0], [0.0, f, a.H / 2.0], [0.0, 0.0, 1.0]])
    N = pose.shape[0]
    intr = (intr[None].expand(N, 3, 3) if intr.dim() == 2 else intr).contiguous().to(dev)
    pose = pose.contiguous().to(dev)
    bg = tuple(float(v) * scale for v in opt.nerf.depth.range)
    bounds = SceneBounds({int(oid): (SurfelRenderer(verts, faces, None, a.H, a.W, a.device), verts.min(axis=0), verts.max(axis=0))},
                         a.H, a.W, scale, bg)
    thresholds = {k: v for k, v in dict(cos_min=a.cos_min, cover_min=a.cover_min, z_tol_mm=a.z_tol_mm, slope=a.slope).items() if v is not None}
    # with --texel-res the nodes of the subdivided mesh are baked; its first V rows are the mesh's vertices, so the PLY comes from them
    texel_baker = None if a.texel_res is None else ft.FaceTexelBaker(verts, faces, a.texel_res, a.H, a.W, a.device, **thresholds)
    baker = tb.TextureBaker(verts, faces, a.H, a.W, a.device, **thresholds) if texel_baker is None else texel_baker.nodes
    fit_mode = dict(lighting=True, rounds=a.fit_lighting) if a.fit_lighting is not None else {}
    if a.fit_robust is not None:
        fit_mode = dict(robust=a.fit_robust, robust_rounds=6 if a.fit_robust_rounds is None else a.fit_robust_rounds)
    fitter = None if a.fit is None else ft.FaceTexelFitter(verts, faces, a.texel_res, a.H, a.W, a.device, lam=a.fit_lambda, iters=a.fit, **fit_mode)
    light = torch.tensor(a.light_index, device=dev)
    kept = []                                                         # (rgb, mask) of every view, for --verify
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    with torch.no_grad():
        for c in range(0, N, a.chunk):
            p, k = pose[c:c + a.chunk], intr[c:c + a.chunk]
            n = p.shape[0]
            sb = bounds(p, k, source)
            rgb = torch.empty(n, a.H, a.W, 3, device=dev)
            weight = torch.empty(n, a.H, a.W, device=dev)
            for i in range(n):
                dr = (sb.depth_range[0][i:i + 1], sb.depth_range[1][i:i + 1])
                ret = graph.render_by_slices(opt, p[i:i + 1], intr=k[i:i + 1], depth_range=dr, object_mask=sb.object_mask[i:i + 1],
                                             sample_idx=light, mode="eval")
                rgb[i] = ret.rgb_static.view(a.H, a.W, 3)
                weight[i] = ret.opacity_static.view(a.H, a.W)
            baker.add_views(rgb, tb.poses_to_mm(p, scale), k, zbuf=sb.zbuf[0], weight=weight)      # (the base mesh's depth planes)
            if fitter is not None and a.fit_photos is None:
                pose_mm = tb.poses_to_mm(p, scale).contiguous()
                face = ops.mesh_raster(fitter.verts, fitter.faces, pose_mm, k, H=a.H, W=a.W, normals=False)["face"]
                inside = sb.object_mask.view(n, a.H, a.W) & (sb.zbuf[0] > 0)
                fitter.add_views(rgb.clamp(0, 1), pose_mm, k, face=face, weight=(ft.inner_coverage(face, len(faces)) & inside).float())
            if a.verify:
                kept.append((rgb, sb.object_mask.view(n, a.H, a.W) & (sb.zbuf[0] > 0)))
        if fitter is not None and a.fit_photos is not None:
            photos = np.load(a.fit_photos)
            prgb = np.asarray(photos["rgb"], dtype=np.float32)
            ppose = np.asarray(photos["pose"], dtype=np.float32).reshape(-1, 3, 4)
            pintr = np.asarray(photos["intr"], dtype=np.float32)
            if prgb.shape != (len(ppose), a.H, a.W, 3) or pintr.shape not in ((3, 3), (len(ppose), 3, 3)):
                sys.exit("bake_texture: --fit-photos holds rgb %s, pose %s and intr %s; rgb [N,%d,%d,3], pose [N,3,4] and intr [3,3] or [N,3,3] expected"
                         % (prgb.shape, ppose.shape, pintr.shape, a.H, a.W))
            for c in range(0, len(ppose), a.chunk):
                fitter.add_views(torch.from_numpy(prgb[c:c + a.chunk]), torch.from_numpy(ppose[c:c + a.chunk]),
                                 torch.from_numpy(pintr if pintr.ndim == 2 else pintr[c:c + a.chunk]))
    V = len(verts)
    texels = None
    if texel_baker is None:
        res = baker.result(fill=True)
    else:
        sub = texel_baker.result(fill=True)
        texels = sub.texels
        res = tb.AttrDict(vcolor=sub.vcolor_sub[:V].contiguous(), count=sub.count[:V], seen=sub.seen[:V], filled=sub.filled, unseen=sub.unseen)
    baked_texels, fit = texels, None
    if fitter is not None:
        got = fitter.fit(prior=sub.vcolor_sub, start=sub.vcolor_sub)
        nodes = got.nodes.clamp(0, 1)
        texels, res.vcolor = ft.texels_from_nodes(nodes, fitter.node_index), nodes[:V].contiguous()
        fit = dict(iters=a.fit, lam=a.fit_lambda, rms_before=float(got.rms[0]), rms_after=float(got.rms[-1]), on_prior=got.on_prior,
                   rms=[float(v) for v in got.rms.tolist()], views=fitter.views, photos=a.fit_photos)
        if a.fit_lighting is not None:
            fit["lighting"] = dict(rounds=a.fit_lighting, light=got.light.tolist(), status=got.lighting_status.tolist(),
                                   flags=got.lighting_flags.tolist(), gain=got.gain.tolist())
        if a.fit_robust is not None:
            fit["robust"] = dict(kind=a.fit_robust, rounds=fitter.robust_rounds, scale=got.scale.tolist(), kept=got.kept.tolist(),
                                 count=got.robust_count.tolist())
    torch.cuda.synchronize(dev)
    seconds = time.perf_counter() - t0
    ops.check_mlp_status(dev)
    tb.write_ply(a.out, verts, faces, res.vcolor.cpu().numpy())
    report = dict(vertices=V, faces=int(len(faces)), views=N, H=a.H, W=a.W, coverage=float((res.count > 0).sum()) / V,
                  coloured=float(res.seen.sum()) / V, mean_views_per_vertex=float(res.count.double().mean()), filled=res.filled,
                  unseen=res.unseen, thresholds=baker.thresholds, seconds_render_and_bake=seconds, mlp=graph.nerf.precision, out=a.out)
    if texels is not None:
        texel_file = os.path.splitext(a.out)[0] + ".texels.npz"
        ft.save_texels(texel_file, texels, faces)
        U = len(texel_baker.verts_sub)
        report["texels"] = dict(R=a.texel_res, per_face=int(texels.shape[1]), nodes=U, coloured=float(sub.seen.sum()) / U, filled=sub.filled,
                                unseen=sub.unseen, file=texel_file)
        if a.texel_mips is not None:
            report["texels"]["mip_levels"] = a.texel_mips or ft.mip_levels(a.texel_res)
    if fit is not None:
        report["fit"] = fit
        print("bake_texture: fit of %d nodes, %d iterations, lambda %g: training rms %.5f -> %.5f, %d nodes on the prior"
              % (len(texel_baker.verts_sub), a.fit, a.fit_lambda, fit["rms_before"], fit["rms_after"], fit["on_prior"]))
        if a.fit_lighting is not None:
            print("bake_texture: %d rounds under one light per view: mean ambient gain %s, %d of %d light fits ok"
                  % (a.fit_lighting, " ".join("%.3f" % g for g in fit["lighting"]["gain"]), sum(s == 0 for s in fit["lighting"]["status"]), fitter.views))
        if a.fit_robust is not None:
            print("bake_texture: %d rounds of %s weights: sigma per view %.4f .. %.4f, weight kept per view %.3f .. %.3f"
                  % (fit["robust"]["rounds"], a.fit_robust, min(fit["robust"]["scale"]), max(fit["robust"]["scale"]), min(fit["robust"]["kept"]),
                     max(fit["robust"]["kept"])))
    if a.verify:
        base_verts, base_faces = (baker.verts, baker.faces) if texel_baker is None else (texel_baker.verts, texel_baker.faces)

        def rerender(texels):
            se, px = 0.0, 0
            mips = None if texels is None or a.texel_mips is None else ft.build_mips(base_verts, base_faces, texels, a.texel_mips or None)
            with torch.no_grad():
                for c, (rgb, mask) in zip(range(0, N, a.chunk), kept):
                    r = ops.mesh_raster(base_verts, base_faces, tb.poses_to_mm(pose[c:c + a.chunk], scale).contiguous(), intr[c:c + a.chunk],
                                        H=a.H, W=a.W, vcolor=res.vcolor if texels is None else None, texels=texels, texel_mips=mips, face_ids=False,
                                        normals=False)
                    m = mask & (r["zbuf"] > 0)
                    se += float((((r["rgb"] - rgb.clamp(0, 1)) ** 2).sum(-1) * m).double().sum())
                    px += int(m.sum())
            mse = se / max(1, 3 * px)
            return px, mse, ((float("inf") if mse == 0 else -10.0 * float(np.log10(mse))) if px else None)

        px, mse, psnr = rerender(texels)
        report["verify"] = dict(pixels=px, mse=mse, psnr_db=psnr)
        if fit is not None:
            report["verify"]["psnr_db_baked"] = rerender(baked_texels)[2]
            print("bake_texture: re-rendered mesh through the BAKED texels against the NeRF views inside the mask: PSNR %s dB over %d pixels"
                  % ("%.2f" % report["verify"]["psnr_db_baked"] if px else "n/a", px))
        print("bake_texture: re-rendered mesh%s against the NeRF views inside the mask: PSNR %s dB over %d pixels"
              % (" through the FITTED texels" if fit is not None else "", "%.2f" % psnr if px else "n/a", px))
    if a.report:
        with open(a.report, "w") as fh:
            json.dump(report, fh, indent=1)
    print("bake_texture: %d views %dx%d -> %s: %d vertices, coverage %.4f, %.2f views per vertex, %d filled, %d unseen, %.2f s"
          % (N, a.H, a.W, a.out, V, report["coverage"], report["mean_views_per_vertex"], res.filled, res.unseen, seconds))


if __name__ == "__main__":
    main()
