#!/usr/bin/env python3
"""Render a checkpoint at a sweep of novel object poses, with the depth bounds and object masks made on the device from the CAD
meshes (texpose_amd.scene_bounds.SceneBounds -> Graph.render_by_slices); the novel-view loop of the reference's
model/nerf_pretrain.py:268-283, 307-435 without PyTorch3D and OpenCV.

    python tools/novel_views.py --checkpoint model.ckpt --scene scene.npz --ply 5=obj_000005.ply --ply 9=obj_000009.ply --out novel_view

--scene: an .npz with pose_anchor [3,4] (t in nerf.depth.scale units) and intr [3,3].  --ply ID=PATH, once per object of the scene
(the meshes share the scene frame; the box of an object is the extent of its vertices).  Written to --out, as the reference names them:
novel_pose.npy [N,3,4], rgb_{i}.png, depth_{i}.png (uint16, metres x 2000), inv_depth_{i}.png.  --precision sets arch.mlp_precision
(default: the option's own default); --source is nerf.depth.range_source (box | render | none).
--bop DIR also writes the views as an annotated BOP scene folder (texpose_amd.bop_scene: rgb/, depth/, mask/, mask_visib/ and the
scene_*.json files; masks, boxes and pixel counts from SceneBounds.annotate, image bytes from ops.view_images); --out may then be left
out.  --name ID=NAME, once per object, adds scene_object.json; --verify reads the written scene back and checks its files against each
other.
Out of scope: videos."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--scene", required=True)
    ap.add_argument("--ply", action="append", required=True, metavar="ID=PATH")
    ap.add_argument("--out", default=None, help="folder of the loose files")
    ap.add_argument("--bop", default=None, metavar="DIR", help="write the views as a BOP scene folder")
    ap.add_argument("--name", action="append", default=None, metavar="ID=NAME", help="model names for scene_object.json (with --bop)")
    ap.add_argument("--verify", action="store_true", help="read the BOP scene back and check it (with --bop)")
    ap.add_argument("--N", type=int, default=10, help="poses of the sweep")
    ap.add_argument("--H", type=int, default=480)
    ap.add_argument("--W", type=int, default=640)
    ap.add_argument("--samples", type=int, default=None, help="nerf.sample_intvs")
    ap.add_argument("--source", choices=["box", "render", "none"], default=None)
    ap.add_argument("--precision", choices=["fp32", "f16x3", "f16"], default=None)
    ap.add_argument("--light-index", type=int, default=0, help="row of latent_vars_light the views are lit with")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not a.out and not a.bop:
        ap.error("--out or --bop expected")
    import torch
    from PIL import Image
    from texpose_amd import checkpoint as ck, ops
    from texpose_amd.graph import Graph
    from texpose_amd.options import default_options
    from texpose_amd.scene_bounds import SceneBounds, novel_view_poses_obj
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
    scene = np.load(a.scene)
    intr = torch.from_numpy(scene["intr"].astype(np.float32)).to(dev)
    objects = {}
    for item in a.ply:
        oid, path = item.split("=", 1)
        verts, faces, _ = load_ply(path)
        objects[int(oid)] = (SurfelRenderer(verts, faces, None, a.H, a.W, a.device), verts.min(axis=0), verts.max(axis=0))
    scale = float(opt.nerf.depth.scale)
    bg = tuple(float(v) * scale for v in opt.nerf.depth.range)
    bounds = SceneBounds(objects, a.H, a.W, scale, bg)
    pose_novel = novel_view_poses_obj(torch.from_numpy(scene["pose_anchor"].astype(np.float32)), a.N)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        np.save(os.path.join(a.out, "novel_pose.npy"), pose_novel.numpy())
    pose_dev = pose_novel.to(dev)
    sb = bounds(pose_dev, intr, source)                             # every pose of the sweep in one batch
    writer = None
    if a.bop:
        from texpose_amd.bop_scene import BopSceneWriter, verify_bop_scene
        names = None if a.name is None else {int(item.split("=", 1)[0]): item.split("=", 1)[1] for item in a.name}
        writer = BopSceneWriter(a.bop, intr, scale, png_per_metre=2000, names=names)
        ann = bounds.annotate(sb)                                   # masks, boxes and counts of every pose: geometry only
    light = torch.tensor(a.light_index, device=dev)
    eps = 1e-10
    with torch.no_grad():
        for i in range(a.N):
            dr = (sb.depth_range[0][i:i + 1], sb.depth_range[1][i:i + 1])
            ret = graph.render_by_slices(opt, pose_dev[i:i + 1], intr=intr[None], depth_range=dr, object_mask=sb.object_mask[i:i + 1],
                                         sample_idx=light, mode="eval")
            if writer is not None:
                img = ops.view_images(ret.rgb, ret.depth, H=a.H, W=a.W, depth_scale=scale, png_per_metre=2000)
                writer.add_views(pose_dev[i:i + 1], bounds.object_ids, ann.info[i:i + 1], ann.mask[i:i + 1], ann.mask_visib[i:i + 1],
                                 img["rgb8"], img["depth16"])
            if not a.out:
                continue
            rgb = ret.rgb.view(a.H, a.W, 3).clamp(0, 1)
            depth_m = ret.depth.view(a.H, a.W) / scale                     # metres
            inv = torch.nan_to_num(1 / (ret.depth / ret.opacity + eps), nan=0.0, posinf=0.0).view(a.H, a.W).clamp(0, 1)
            Image.fromarray((rgb * 255).byte().cpu().numpy(), "RGB").save(os.path.join(a.out, "rgb_%d.png" % i))
            Image.fromarray((depth_m * 2000).clamp(0, 65535).cpu().numpy().astype(np.uint16)).save(os.path.join(a.out, "depth_%d.png" % i))
            Image.fromarray((inv * 255).byte().cpu().numpy(), "L").save(os.path.join(a.out, "inv_depth_%d.png" % i))
    ops.check_mlp_status(dev)
    if writer is not None:
        writer.close()
        if a.verify:
            print("novel_views: %d frames of %s read back and consistent" % (verify_bop_scene(a.bop), a.bop))
    print("novel_views: %d poses, %d objects, %dx%d, source %s, mlp %s -> %s" % (a.N, len(objects), a.H, a.W, source, graph.nerf.precision,
                                                                                   " + ".join(d for d in (a.out, a.bop) if d)))


if __name__ == "__main__":
    main()
