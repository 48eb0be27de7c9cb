#!/usr/bin/env python3
"""Object poses from the NOCS maps of a scene folder by batched PnP-RANSAC on the GPU (texpose_amd.pnp, K28), written
as a BOP results CSV that tools/pose_errors.py --est reads unchanged.

    python tools/pnp_poses.py --scene SCENE_DIR --loop L --ply ID=PATH [--ply ID=PATH ...] --out poses.csv [--scene-id 1]

--scene: a folder with scene_camera.json (cam_K per frame) and nocs_<L>/NAME.png: the files texpose_amd.surfel.write_surfel_frame
writes (8-bit RGB = the x, y, z model coordinates mapped to [0, 1] by surfel.nocs_normalisation of the mesh), or a pose estimator's
maps in the same layout.  NAME is `{frame:06d}` (one object: the single --ply) or `{frame:06d}_{k:06d}` (instance k of the frame: its
object id is read from scene_gt.json, or is the single --ply where that file is absent).  The mask of a map is, in this order: the
file of the same name under --masks DIR (non-zero pixels; relative to the scene), the alpha channel of rgbsyn_<L>/NAME.png,
mask_visib/NAME.png, or the pixels whose three NOCS bytes are not all zero.  --ply ID=PATH: the object's mesh, for the normalisation.
Each row of the CSV is scene_id,im_id,obj_id,score,R,t,time with score = inliers / correspondences, R as 9 and t as 3 space-separated
numbers (mm) and time = the seconds of the batch the map was solved in, divided by its size.  Maps with fewer than four usable pixels
or without any valid hypothesis get no row.  --hypotheses, --tau-px, --iters, --seed, --stride: the solver's settings;
--nocs-offset: added to every NOCS byte before the division by 255 (0.5 undoes the truncation of write_surfel_frame on average)."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAME = re.compile(r"(\d{6})(?:_(\d{6}))?\.png")


def find_mask(scene, loop, masks, name, nocs8):
    from PIL import Image
    if masks:
        return np.asarray(Image.open(os.path.join(scene, masks, name))) != 0
    rgba = os.path.join(scene, "rgbsyn_{}".format(loop), name)
    if os.path.exists(rgba):
        im = np.asarray(Image.open(rgba))
        if im.ndim == 3 and im.shape[2] == 4:
            return im[..., 3] > 0
    visib = os.path.join(scene, "mask_visib", name)
    if os.path.exists(visib):
        return np.asarray(Image.open(visib)) != 0
    return nocs8.any(-1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scene", required=True, metavar="SCENE_DIR")
    ap.add_argument("--loop", required=True, help="the maps are read from nocs_<loop>/")
    ap.add_argument("--ply", action="append", required=True, metavar="ID=PATH")
    ap.add_argument("--out", required=True, metavar="CSV")
    ap.add_argument("--scene-id", type=int, default=1)
    ap.add_argument("--masks", default=None, metavar="DIR")
    ap.add_argument("--hypotheses", type=int, default=256)
    ap.add_argument("--tau-px", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--nocs-offset", type=float, default=0.0)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not a.device.startswith("cuda"):
        sys.exit("pnp_poses: the solver runs the HIP kernels, which have no CPU route; use --device cuda:N")
    import torch
    from PIL import Image
    from texpose_amd import pnp
    from texpose_amd.surfel import load_ply, nocs_normalisation
    if not torch.cuda.is_available():
        sys.exit("pnp_poses: needs a GPU")
    norm = {}
    for item in a.ply:
        oid, path = item.split("=", 1)
        norm[int(oid)] = nocs_normalisation(load_ply(path)[0])
    cam = json.load(open(os.path.join(a.scene, "scene_camera.json")))
    gt_path = os.path.join(a.scene, "scene_gt.json")
    gt = json.load(open(gt_path)) if os.path.exists(gt_path) else None
    folder = os.path.join(a.scene, "nocs_{}".format(a.loop))
    jobs = {}                                                   # (obj_id, H, W) -> [(frame, file name)]
    for name in sorted(os.listdir(folder)):
        m = NAME.fullmatch(name)
        if not m:
            continue
        frame = int(m.group(1))
        if m.group(2) is not None and gt is not None:
            oid = int(gt[str(frame)][int(m.group(2))]["obj_id"])
        elif len(norm) == 1:
            oid = next(iter(norm))
        else:
            sys.exit("pnp_poses: %s: which object? (several --ply and no scene_gt.json / instance number)" % name)
        if oid not in norm:
            continue
        if str(frame) not in cam:
            sys.exit("pnp_poses: frame %d is not in scene_camera.json" % frame)
        W, H = Image.open(os.path.join(folder, name)).size
        jobs.setdefault((oid, H, W), []).append((frame, name))
    rows, solvers = [], {}
    for (oid, H, W), items in jobs.items():
        solver = solvers.setdefault((H, W), pnp.PnPSolver(H, W, a.device, T=a.hypotheses, tau_px=a.tau_px, iters=a.iters, seed=a.seed))
        centre, scale = norm[oid]
        for s in range(0, len(items), a.batch):
            part = items[s:s + a.batch]
            nocs8 = np.stack([np.asarray(Image.open(os.path.join(folder, name)).convert("RGB")) for _, name in part])
            mask = np.stack([find_mask(a.scene, a.loop, a.masks, name, n8) for (_, name), n8 in zip(part, nocs8)])
            K = np.stack([np.array(cam[str(frame)]["cam_K"], np.float32).reshape(3, 3) for frame, _ in part])
            torch.cuda.synchronize()
            t0 = time.time()
            nocs = (torch.from_numpy(nocs8).to(a.device).float() + a.nocs_offset) / 255.0
            r = solver.solve_nocs(nocs, torch.from_numpy(mask.astype(np.uint8)).to(a.device), torch.from_numpy(K).to(a.device), centre, scale,
                                  stride=a.stride)
            pose, score, status = r.pose.double().cpu().numpy(), r.score.cpu().numpy(), r.status.cpu().numpy()
            dt = (time.time() - t0) / len(part)
            for i, (frame, _) in enumerate(part):
                if status[i] in (1, 2):
                    continue
                rows.append((a.scene_id, frame, oid, float(score[i]), pose[i, :, :3].reshape(-1), pose[i, :, 3], dt))
    rows.sort(key=lambda r: (r[1], r[2]))
    with open(a.out, "w") as f:
        f.write("scene_id,im_id,obj_id,score,R,t,time\n")
        for sid, frame, oid, score, R, t, dt in rows:
            f.write("%d,%d,%d,%.6f,%s,%s,%.6f\n" % (sid, frame, oid, score, " ".join("%.9g" % v for v in R), " ".join("%.9g" % v for v in t), dt))
    print("pnp_poses: %d maps, %d poses -> %s" % (sum(len(v) for v in jobs.values()), len(rows), a.out))
    return rows


if __name__ == "__main__":
    main()
