#!/usr/bin/env python3
"""Refine the estimated poses of a BOP results CSV against the depth images of a scene folder by batched projective ICP on the GPU
(texpose_amd.icp, K29), written as the same CSV format, so that tools/pose_errors.py --est scores it unchanged.

    python tools/refine_poses.py --scene SCENE_DIR --ply [ID=]PATH [--ply ID=PATH ...] --est RESULTS.csv --out REFINED.csv
                                 [--silhouette [--occluders | --known DIR] [--depth | --rgb]] [--rgb]
                                 [--joint [--iters-joint N] [--weights SIL RGB DEPTH]] [--cull-raster] [--texels [ID=]PATH]
                                 [--exposure | --lighting] [--pyramid N ...] [--multiview]

--scene: a BOP scene folder with scene_camera.json (cam_K and depth_scale per frame) and depth/{frame:06d}.png (16 bit; 0: no
measurement).  --est: scene_id,im_id,obj_id,score,R,t,time rows (the file tools/pnp_poses.py writes); --scene-id keeps the rows of one
scene where the file holds several.  --ply: the object's mesh; a bare PATH serves every object id of the CSV, ID=PATH that object alone;
rows of an object without a mesh are copied unchanged.  Each kept row is refined by --iters Gauss-Newton steps (the mesh rendered at
the current pose, the covered pixels within --tau-mm of the measurement along their ray against the faces' normals; several --tau-mm
values: a coarse-to-fine schedule of iters + 1 entries) and written with its score unchanged and the per-pose time of its batch added
to its time.  --use-mask-visib: only the pixels of mask_visib/{frame:06d}_{k:06d}.png are used, k the object's first instance of the
frame in scene_gt.json.  A pose whose last step failed (fewer than six usable pixels, a rank-deficient system) is written as the loop
left it; the tool prints how many.

--rgb: refine against the scene's rgb/{frame:06d}.png instead of its depth (texpose_amd.photo_align, K30): --ply is
then the vertex-coloured mesh (texture_bake's output; the tool exits if it has no colours), the photograph is the 8-bit image / 255,
the vertex colours' own range, and every interior covered pixel whose rendered colour lies within --tau-rgb of the photograph's pulls
on the pose through the photograph's gradient, for --iters-rgb steps (--tau-rgb: one value or iters-rgb + 1).  --use-mask-visib,
--damping, --batch and the output are as above; --tau-mm and --iters are not used.

--silhouette: first refine against the OUTLINE of the object's mask (texpose_amd.silhouette, K31): --ply may be a
textureless mesh, the masks are the scene's mask_visib/{frame:06d}_{k:06d}.png (k the object's first instance of the frame in
scene_gt.json) or the files of the same names in --masks DIR, and every rim pixel of the rendering within --tau-px of the mask's
outline pulls on the pose through the gradient of the mask's distance field, for --iters-sil steps (--tau-px: one value or iters-sil +
1).  Alone it is the whole refinement (no depth, no colours: adaptation loop 0); with --depth or --rgb that refiner then starts from
the silhouette's poses.  It closes the outline, not necessarily the pose (a symmetric shape, depth at a small radius), and a mask cut
by an occluder misleads it.  The tool prints the mean intersection over union of rendering and mask before and after.

--occluders (with --silhouette): mask_visib is the VISIBLE mask, and where another object hides part of this one
its edge is not the object's.  Per frame the masks of EVERY instance in scene_gt.json are read (from --masks DIR or mask_visib/), and
a pixel within --occluder-band pixels (default 1.0; not tuned on anything) of another instance's mask becomes UNKNOWN: neither set
nor clear in the distance field, and no rim pixel there pulls on the pose.  Conservative: where two instances touch, both lose the
contour between them, the one in front too.  --known DIR gives such planes directly: PNGs with the mask files' names, non-zero:
the pixel was measured.  The two exclude each other.  With either the tool also prints the mean visible IoU, the IoU over the known
pixels only, before and after.  With less than about half of an object visible the outline still closes and the pose need not.

--joint: the terms named by --silhouette, --rgb and --depth (at least two; --rgb and --depth may go together here)
in ONE loop of --iters-joint steps (default 20), all their residual rows in one Gauss-Newton system per step (texpose_amd.joint, K33),
instead of one refiner after the other: under occlusion the silhouette stage alone walks off and the next stage cannot come back.
--weights SIL RGB DEPTH: 1 / sigma^2 of each term's residual unit, default 1 100 0.04 (the photometric weight is the one that
converged on the occluded cases of section 23; the depth weight is sigma = 5 mm and is not tuned on anything).  --tau-px, --tau-rgb and
--tau-mm are the terms' thresholds (one value or iters-joint + 1 each); --occluders, --known and --use-mask-visib apply as above and
also mask the other terms.  Without --joint nothing changes.

--cull-raster: every refiner renders with the culled rasteriser (ops.mesh_raster(cull=True), K34), which skips whole
chunks of 256 faces per 16 x 16 tile.  The planes are the same bit for bit, so the poses written are the same; only the time differs.

--texels [ID=]PATH (with --rgb): the mesh's face-texel texture, the .texels.npz that bake_texture.py --texel-res
writes beside its PLY (keyed like --ply).  The photometric renders then take their colour from the texels (K35) instead of the vertex
colours, --ply may be colourless, and the file is refused if it was baked for other faces than the mesh's.

--exposure (with --rgb, alone or under --joint): the photographs were taken under another exposure, white balance or
light than the mesh's colours.  Every pass first fits a gain and a bias per image and channel between rendering and photograph
(ops.photo_exposure, K37) and compares the colours under them.

--lighting (with --rgb, alone, under --joint or with --multiview; not together with --exposure, whose model it
contains): the photographs were taken under a light with a direction, a lamp on one side of the object.  Every pass first fits ambient +
directional shading on the faces' normals and a bias per image and channel (ops.photo_lighting, K40) and compares the colours under them.

--pyramid N [N ...] (with --rgb, not under --joint): coarse to fine on an image pyramid, for estimates further off
than the texture's detail lets the one-pixel gradient see.  The step counts per level, the coarsest first, adding up to --iters-rgb:
--pyramid 4 3 3 takes 4 steps at a quarter of the size, 3 at half and 3 at full size (ops.photo_align's pyramid=, K38).  The object
should cover some hundreds of pixels at the coarsest level.

--multiview: the frames of a scene show the SAME rigid objects, and scene_camera.json carries each frame's camera
pose (cam_R_w2c, cam_t_w2c in mm).  All rows of one object id in one scene are then views of ONE pose in the world frame: they are
refined together (texpose_amd.multiview, K39), every view's residual rows in one Gauss-Newton system, with the terms named by
--silhouette, --rgb and --depth (one is enough), --iters-joint steps and --weights as under --joint.  The group starts from the row with
the highest score (the first on a tie), taken into the world frame; every row is written with its camera's pose of the group's result.
The tool exits where a frame lacks the camera pose and where one frame holds two rows of one object id (which instance is which across
frames is then unknown).  --pyramid does not go with it.  Without --multiview nothing changes."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_rows(path, scene_id=None):
    """The CSV's rows in file order: [scene_id, im_id, obj_id, score, R [3,3], t [3], time]."""
    rows = []
    with open(path, newline="") as f:
        for row in csv.reader(f):
            if not row or not row[0].strip().lstrip("-").isdigit():          # (the header line, blank lines)
                continue
            sid = int(row[0])
            if scene_id is not None and sid != scene_id:
                continue
            R, t = np.array(row[4].split(), dtype=np.float64), np.array(row[5].split(), dtype=np.float64)
            if R.size != 9 or t.size != 3:
                raise ValueError("%s: R must hold 9 and t 3 numbers (frame %s, object %s)" % (path, row[1], row[2]))
            rows.append([sid, int(row[1]), int(row[2]), float(row[3]), R.reshape(3, 3), t, float(row[6]) if len(row) > 6 and row[6].strip() else 0.0])
    return rows


def write_rows(path, rows):
    with open(path, "w") as f:
        f.write("scene_id,im_id,obj_id,score,R,t,time\n")
        for sid, frame, oid, score, R, t, dt in rows:
            f.write("%d,%d,%d,%.6f,%s,%s,%.6f\n" % (sid, frame, oid, score, " ".join("%.9g" % v for v in np.reshape(R, -1)),
                                                     " ".join("%.9g" % v for v in np.reshape(t, -1)), dt))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", required=True, metavar="SCENE_DIR")
    ap.add_argument("--ply", action="append", required=True, metavar="[ID=]PATH")
    ap.add_argument("--est", required=True, metavar="CSV")
    ap.add_argument("--out", required=True, metavar="CSV")
    ap.add_argument("--scene-id", type=int, default=None)
    ap.add_argument("--tau-mm", type=float, nargs="+", default=[20.0])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--damping", type=float, default=1e-6)
    ap.add_argument("--use-mask-visib", action="store_true")
    ap.add_argument("--rgb", action="store_true")
    ap.add_argument("--tau-rgb", type=float, nargs="+", default=[0.5])
    ap.add_argument("--iters-rgb", type=int, default=10)
    ap.add_argument("--silhouette", action="store_true")
    ap.add_argument("--depth", action="store_true", help="with --silhouette: go on with the depth refinement")
    ap.add_argument("--tau-px", type=float, nargs="+", default=[4.0])
    ap.add_argument("--iters-sil", type=int, default=10)
    ap.add_argument("--masks", default=None, metavar="DIR")
    ap.add_argument("--occluders", action="store_true", help="with --silhouette: pixels near another instance's mask are unknown")
    ap.add_argument("--occluder-band", type=float, default=1.0, metavar="PX")
    ap.add_argument("--known", default=None, metavar="DIR", help="with --silhouette: PNGs with the mask files' names, non-zero: known")
    ap.add_argument("--joint", action="store_true", help="the terms named by --silhouette, --rgb, --depth in one loop")
    ap.add_argument("--iters-joint", type=int, default=20)
    ap.add_argument("--weights", type=float, nargs=3, default=None, metavar=("SIL", "RGB", "DEPTH"))
    ap.add_argument("--cull-raster", action="store_true", help="render with the culled rasteriser: the same poses, faster on large meshes")
    ap.add_argument("--texels", action="append", default=[], metavar="[ID=]PATH", help="with --rgb: face texels (bake_texture --texel-res)")
    ap.add_argument("--exposure", action="store_true", help="with --rgb: fit a gain and a bias per image and channel in every pass")
    ap.add_argument("--lighting", action="store_true", help="with --rgb: fit ambient + directional shading and a bias per image and channel in every pass")
    ap.add_argument("--pyramid", type=int, nargs="+", default=None, metavar="N", help="with --rgb: steps per pyramid level, the coarsest first")
    ap.add_argument("--multiview", action="store_true", help="all rows of one object are views of one pose (needs cam_R_w2c / cam_t_w2c)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not a.device.startswith("cuda"):
        sys.exit("refine_poses: the refinement runs the HIP kernels, which have no CPU route; use --device cuda:N")
    if a.multiview and a.silhouette + a.rgb + a.depth < 1:
        sys.exit("refine_poses: --multiview needs at least one of --silhouette, --rgb and --depth")
    one_loop = a.joint or a.multiview                            # every named term in ONE loop (K33's sums)
    if one_loop:
        if not a.multiview and a.silhouette + a.rgb + a.depth < 2:
            sys.exit("refine_poses: --joint combines at least two of --silhouette, --rgb and --depth")
        for name, values in (("--tau-px", a.tau_px), ("--tau-rgb", a.tau_rgb), ("--tau-mm", a.tau_mm)):
            if len(values) not in (1, a.iters_joint + 1):
                sys.exit("refine_poses: with --joint %s takes one value or iters-joint + 1 = %d values" % (name, a.iters_joint + 1))
        a.iters = a.iters_rgb = a.iters_sil = a.iters_joint      # (the per-stage checks below then say the same)
    elif a.weights is not None:
        sys.exit("refine_poses: --weights goes with --joint")
    if len(a.tau_mm) not in (1, a.iters + 1):
        sys.exit("refine_poses: --tau-mm takes one value or iters + 1 = %d values" % (a.iters + 1))
    if a.rgb and len(a.tau_rgb) not in (1, a.iters_rgb + 1):
        sys.exit("refine_poses: --tau-rgb takes one value or iters-rgb + 1 = %d values" % (a.iters_rgb + 1))
    if a.silhouette and len(a.tau_px) not in (1, a.iters_sil + 1):
        sys.exit("refine_poses: --tau-px takes one value or iters-sil + 1 = %d values" % (a.iters_sil + 1))
    if a.rgb and a.depth and not one_loop:
        sys.exit("refine_poses: --depth and --rgb exclude each other")
    if a.occluders and a.known:
        sys.exit("refine_poses: --occluders and --known exclude each other")
    if a.texels and not a.rgb:
        sys.exit("refine_poses: --texels goes with --rgb")
    if a.exposure and not a.rgb:
        sys.exit("refine_poses: --exposure goes with --rgb")
    if a.lighting and not a.rgb:
        sys.exit("refine_poses: --lighting goes with --rgb")
    if a.lighting and a.exposure:
        sys.exit("refine_poses: --lighting or --exposure, not both (the lighting model contains the exposure's)")
    if a.pyramid and (not a.rgb or one_loop):
        sys.exit("refine_poses: --pyramid goes with --rgb" + (", and not under --joint" if a.joint else ", and not with --multiview" if a.multiview else ""))
    if a.pyramid and (min(a.pyramid) < 0 or sum(a.pyramid) != a.iters_rgb):
        sys.exit("refine_poses: the steps of --pyramid must be >= 0 and add up to --iters-rgb = %d" % a.iters_rgb)
    if (a.occluders or a.known) and not a.silhouette:
        sys.exit("refine_poses: --occluders and --known go with --silhouette")
    import torch
    from PIL import Image
    from texpose_amd import icp, joint, multiview, ops, photo_align, silhouette
    from texpose_amd.pose_error import depth_from_png
    from texpose_amd.face_texels import load_texels
    from texpose_amd.surfel import load_ply
    if not torch.cuda.is_available():
        sys.exit("refine_poses: needs a GPU")
    by_id = lambda item: (lambda oid, sep, path: (int(oid), path) if sep and oid.strip().isdigit() else (None, item))(*item.partition("="))
    texel_files = dict(by_id(item) for item in a.texels)
    meshes = {}
    for item in a.ply:
        oid, sep, path = item.partition("=")
        key, path = (int(oid), path) if sep and oid.strip().isdigit() else (None, item)
        mesh = load_ply(path)
        if a.rgb and key in texel_files:                         # (colour from the face texels: the PLY's own colours are not used)
            mesh = (mesh[0], mesh[1], None, load_texels(texel_files[key], mesh[1])[0])
        elif a.rgb and mesh[2] is None:
            sys.exit("refine_poses: --rgb needs a vertex-coloured mesh (or --texels) and %s has no colours" % path)
        meshes[key] = (tuple(mesh) + (None,))[:4] if a.rgb else mesh[:2]
    if set(texel_files) - set(meshes):
        sys.exit("refine_poses: --texels names an object without a --ply: %s" % sorted(map(str, set(texel_files) - set(meshes))))
    cam = json.load(open(os.path.join(a.scene, "scene_camera.json")))
    gt = None
    if a.use_mask_visib or a.silhouette:
        gt = json.load(open(os.path.join(a.scene, "scene_gt.json")))
    rows = read_rows(a.est, a.scene_id)
    jobs = {}                                                   # object id -> indices into rows
    for i, row in enumerate(rows):
        if row[2] in meshes or None in meshes:
            if str(row[1]) not in cam:
                sys.exit("refine_poses: frame %d is not in scene_camera.json" % row[1])
            jobs.setdefault(row[2], []).append(i)
    if a.multiview:                                              # a view needs its camera, a group one row per frame
        seen = set()
        for idx in jobs.values():
            for i in idx:
                sid, frame, oid = rows[i][:3]
                if "cam_R_w2c" not in cam[str(frame)] or "cam_t_w2c" not in cam[str(frame)]:
                    sys.exit("refine_poses: --multiview: frame %d has no cam_R_w2c / cam_t_w2c in scene_camera.json" % frame)
                if (sid, frame, oid) in seen:
                    sys.exit("refine_poses: --multiview: frame %d holds two rows of object %d: which instance is which across frames is unknown"
                             % (frame, oid))
                seen.add((sid, frame, oid))
    tau = a.tau_mm[0] if len(a.tau_mm) == 1 else a.tau_mm
    tau_rgb = a.tau_rgb[0] if len(a.tau_rgb) == 1 else a.tau_rgb
    tau_px = a.tau_px[0] if len(a.tau_px) == 1 else a.tau_px
    second = not one_loop and (a.rgb or a.depth or not a.silhouette)          # the depth / RGB refinement runs (after the silhouette's, if any)
    iou_sum, visible_sum = np.zeros(2), np.zeros(2)
    refined = failed = 0
    dev = a.device
    for oid, idx in jobs.items():
        verts, faces = meshes.get(oid, meshes.get(None))[:2]
        vcolor, texels = meshes.get(oid, meshes.get(None))[2:4] if a.rgb else (None, None)
        refiner = outline = None
        parts = [idx[s:s + a.batch] for s in range(0, len(idx), a.batch)]
        if a.multiview:                                          # whole groups (the rows of one scene id): a batch is closed once it holds --batch rows
            by_scene, parts = {}, [[]]
            for i in idx:
                by_scene.setdefault(rows[i][0], []).append(i)
            for members in by_scene.values():
                if parts[-1] and len(parts[-1]) + len(members) > a.batch:
                    parts.append([])
                parts[-1] += members
        for part in parts:
            frames = sorted({rows[i][1] for i in part})
            def masks_of(folder, option):
                ms = []
                for f in frames:
                    ks = [k for k, e in enumerate(gt[str(f)]) if int(e["obj_id"]) == oid]
                    path = os.path.join(folder, "%06d_%06d.png" % (f, ks[0])) if ks else None
                    if path is None or not os.path.exists(path):
                        sys.exit("refine_poses: %s: no %s image of object %d in frame %d" % (option, os.path.basename(os.path.normpath(folder)), oid, f))
                    ms.append((np.asarray(Image.open(path)) != 0).astype(np.uint8))
                return torch.from_numpy(np.stack(ms)).to(dev)

            mask = masks_of(os.path.join(a.scene, "mask_visib"), "--use-mask-visib") if a.use_mask_visib else None
            measured = masks_of(a.masks or os.path.join(a.scene, "mask_visib"), "--silhouette") if a.silhouette else None
            known = masks_of(a.known, "--known") if a.known else None
            if a.occluders:                                      # per frame: every instance's mask -> their fields -> who is near whom
                folder, per_frame = a.masks or os.path.join(a.scene, "mask_visib"), []
                for f in frames:
                    paths = [os.path.join(folder, "%06d_%06d.png" % (f, k)) for k in range(len(gt[str(f)]))]
                    for path in paths:
                        if not os.path.exists(path):
                            sys.exit("refine_poses: --occluders: no %s image %s" % (os.path.basename(os.path.normpath(folder)), os.path.basename(path)))
                    every = torch.from_numpy(np.stack([(np.asarray(Image.open(path)) != 0).astype(np.uint8) for path in paths])).to(dev)
                    own = [k for k, e in enumerate(gt[str(f)]) if int(e["obj_id"]) == oid][0]
                    per_frame.append(ops.mask_known_from_others(ops.mask_sdf(every), a.occluder_band)[own])
                known = torch.stack(per_frame)
            read_rgb = lambda: [torch.from_numpy(np.asarray(Image.open(os.path.join(a.scene, "rgb", "%06d.png" % f)).convert("RGB"), np.float32) / 255.0)
                                for f in frames]
            read_depth = lambda: [depth_from_png(np.asarray(Image.open(os.path.join(a.scene, "depth", "%06d.png" % f))), float(cam[str(f)]["depth_scale"]))
                                  for f in frames]
            if one_loop:
                photos = torch.stack(read_rgb()).to(dev) if a.rgb else None
                ranges = torch.stack(read_depth()).to(dev) if a.depth else None
                depth = measured if a.silhouette else photos if a.rgb else ranges          # (any of the measured planes: the size)
            else:
                if a.rgb:
                    planes = read_rgb()
                elif second:
                    planes = read_depth()
                depth = torch.stack(planes) if second else measured  # (with --rgb: the photographs [Ft,H,W,3])
            H, W = depth.shape[1:3]
            if one_loop and (refiner is None or (refiner.H, refiner.W) != (H, W)):
                refiner = (multiview.MultiViewRefiner if a.multiview else joint.JointRefiner)(verts, faces, H, W, dev, vcolor=vcolor, texels=texels,
                                             weights=a.weights or ops.JOINT_WEIGHTS, tau_px=tau_px, tau=tau_rgb, tau_mm=tau, iters=a.iters_joint,
                                             damping=a.damping, cull=a.cull_raster, exposure=a.exposure, lighting=a.lighting)
            if a.silhouette and not one_loop and (outline is None or (outline.H, outline.W) != (H, W)):
                outline = silhouette.SilhouetteRefiner(verts, faces, H, W, dev, tau_px=tau_px, iters=a.iters_sil, damping=a.damping, cull=a.cull_raster)
            if second and (refiner is None or (refiner.H, refiner.W) != (H, W)):
                if a.rgb:
                    refiner = photo_align.PhotoRefiner(verts, faces, vcolor, H, W, dev, tau=tau_rgb, iters=a.iters_rgb,
                                                       damping=a.damping, cull=a.cull_raster, texels=texels, exposure=a.exposure,
                                                       pyramid=a.pyramid, lighting=a.lighting)
                else:
                    refiner = icp.DepthRefiner(verts, faces, H, W, dev, tau_mm=tau, iters=a.iters, damping=a.damping, cull=a.cull_raster)
            pose = np.stack([np.concatenate([rows[i][4], rows[i][5].reshape(3, 1)], 1) for i in part]).astype(np.float32)
            K = np.stack([np.array(cam[str(rows[i][1])]["cam_K"], np.float32).reshape(3, 3) for i in part])
            index = torch.tensor([frames.index(rows[i][1]) for i in part], dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            t0 = time.time()
            start, K = torch.from_numpy(pose).to(dev), torch.from_numpy(K).to(dev)
            if a.multiview:
                w2c = np.stack([np.concatenate([np.array(cam[str(rows[i][1])]["cam_R_w2c"], np.float64).reshape(3, 3),
                                                np.array(cam[str(rows[i][1])]["cam_t_w2c"], np.float64).reshape(3, 1)], 1) for i in part])
                scenes = sorted({rows[i][0] for i in part})
                group = torch.tensor([scenes.index(rows[i][0]) for i in part], dtype=torch.int32, device=dev)
                w2c = torch.from_numpy(w2c.astype(np.float32)).to(dev)
                score = torch.tensor([rows[i][3] for i in part], dtype=torch.float64, device=dev)
                r = refiner.refine(multiview.init_model(start, w2c, group, score, groups=len(scenes)), w2c, group, K, mask_or_sdf=measured, known=known,
                                   image=photos, depth=ranges, frame=index, masks=None if mask is None else dict(silhouette=mask, photo=mask, depth=mask))
                r = type(r)(dict(r, status=r["status"][group.long()]))          # (a row's status is its group's)
            elif a.joint:
                r = refiner.refine(start, K, mask_or_sdf=measured, known=known, image=photos, depth=ranges, frame=index,
                                   masks=None if mask is None else dict(silhouette=mask, photo=mask, depth=mask))
            elif a.silhouette:
                r = outline.refine(start, K, measured, frame=index, mask=mask, known=known)
                start = r.pose
            if a.silhouette:
                iou_sum += [float(r.iou0.double().sum()), float(r.iou.double().sum())]
                if known is not None:
                    visible_sum += [float(r.iou0_visible.double().sum()), float(r.iou_visible.double().sum())]
            if second:
                r = refiner.refine(start, K, depth.to(dev), frame=index, mask=mask)
            out, status = r.pose.double().cpu().numpy(), r.status.cpu().numpy()
            dt = (time.time() - t0) / len(part)
            for k, i in enumerate(part):
                rows[i][4], rows[i][5], rows[i][6] = out[k, :, :3], out[k, :, 3], rows[i][6] + dt
                refined += 1
                failed += int(status[k] != 0)
    write_rows(a.out, rows)
    if a.silhouette and refined:
        print("refine_poses: --silhouette: mean IoU %.4f -> %.4f" % (iou_sum[0] / refined, iou_sum[1] / refined))
        if a.occluders or a.known:
            print("refine_poses: --silhouette: mean visible IoU %.4f -> %.4f" % (visible_sum[0] / refined, visible_sum[1] / refined))
    print("refine_poses: %d rows, %d refined (%d with a failed last step) -> %s" % (len(rows), refined, failed, a.out))
    return rows


if __name__ == "__main__":
    main()
