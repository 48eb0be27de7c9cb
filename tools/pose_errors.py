#!/usr/bin/env python3
"""Score a set of estimated object poses against the ground truth of a BOP scene folder: ADD, ADD-S, MSSD, MSPD, the mean projection
error, rotation and translation error per pose, and the recalls the literature reports, per object (texpose_amd.pose_error; on a GPU
the errors come from the project's kernels).

    python tools/pose_errors.py --gt SCENE_DIR --est EST --ply ID=PATH [--ply ID=PATH ...] [--models-info models_info.json] [--device cuda:0]

--gt: a BOP scene folder (scene_gt.json, scene_camera.json; one written by tools/novel_views.py --bop included).  --est: a second
scene folder (its scene_gt.json holds the estimates; instances of one object in a frame pair up in file order) or a BOP results CSV
(scene_id,im_id,obj_id,score,R,t,time with R as 9 and t as 3 space-separated numbers; the best-scored row per frame and object is
taken; --scene-id selects the scene when the file holds several).  --ply ID=PATH, once per object to score: its vertices are the model
points.  --models-info: the dataset's models_info.json, for the symmetry transforms (without it: the identity alone).
Per object: the diameter (computed from the vertices), mean / median of every error over the matched poses, the ADD and ADD-S recall
at --add-thresholds x diameter (the first is the headline), the --proj-px recall of the projection error and the --te-mm / --re-deg
recall.  A ground-truth pose without an estimate counts as a failure in every recall.  --json OUT also writes the table and the
per-pose errors.  Units: the models' (mm), pixels, degrees.

--vsd adds BOP's third error and the BOP average recall (GPU only, the mesh is rendered by the HIP rasteriser): per
matched pose the frame's depth PNG of --gt is read, the --ply mesh is rendered at the estimate and at the ground truth, and the Visible
Surface Discrepancy is taken at the ten BOP tolerances (--delta-mm: the visibility tolerance).  The table gains the mean / median VSD at
tau = 0.2 x diameter and ar_vsd, ar_mssd, ar_mspd and ar = their mean; a ground-truth instance without an estimate is a miss.
--min-visib drops from the AR rows (and from nothing else) the instances whose visib_fract in --gt's scene_gt_info.json is below it;
where that file or the field is absent every instance counts."""
import argparse
import csv
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ERRORS = ("add", "adds", "mssd", "mspd", "proj", "re", "te")
BATCH = 64          # poses per call


def read_estimates_csv(path, scene_id=None):
    """frame -> {obj_id: (R [3,3], t [3])}: the best-scored row per frame and object."""
    best = {}
    scenes = set()
    with open(path, newline="") as f:
        for row in csv.reader(f):
            if not row or not row[0].strip().lstrip("-").isdigit():          # (the header line, blank lines)
                continue
            sid, im, obj, score = int(row[0]), int(row[1]), int(row[2]), float(row[3])
            scenes.add(sid)
            if scene_id is not None and sid != scene_id:
                continue
            R, t = np.array(row[4].split(), dtype=np.float64), np.array(row[5].split(), dtype=np.float64)
            if R.size != 9 or t.size != 3:
                raise ValueError("%s: R must hold 9 and t 3 numbers (frame %d, object %d)" % (path, im, obj))
            if (im, obj) not in best or score > best[(im, obj)][0]:
                best[(im, obj)] = (score, R.reshape(3, 3), t)
    if scene_id is None and len(scenes) > 1:
        raise ValueError("%s holds the scenes %s: pick one with --scene-id" % (path, sorted(scenes)))
    out = {}
    for (im, obj), (_, R, t) in best.items():
        out.setdefault(im, {}).setdefault(obj, []).append((R, t))
    return out


def read_estimates_scene(root):
    from texpose_amd.bop_scene import read_bop_poses
    out = {}
    for frame, fr in read_bop_poses(root, camera=False).items():
        for obj, R, t in zip(fr["obj_id"], fr["cam_R_m2c"], fr["cam_t_m2c"]):
            out.setdefault(frame, {}).setdefault(int(obj), []).append((R, t))
    return out


def score_object(pts, gt, est, intr, sym, device, dtype):
    """gt / est [N,3,4], intr [N,3,3] (numpy) -> {error: [N] list} in BATCH-sized calls."""
    import torch
    from texpose_amd import pose_error as PE
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    pts_d, sym_d = dev(pts), dev(sym)
    out = {k: [] for k in ERRORS}
    for i in range(0, len(gt), BATCH):
        e, g, K = dev(est[i:i + BATCH]), dev(gt[i:i + BATCH]), dev(intr[i:i + BATCH])
        r = PE.pose_errors(pts_d, e, g, sym_d, K)
        re, te = PE.re_te(e, g)
        got = dict(add=r["add"], mssd=r["mssd"], mspd=r["mspd"], proj=r["proj"], adds=PE.adds(pts_d, e, g), re=torch.rad2deg(re), te=te)
        for k in ERRORS:
            out[k] += [float(v) for v in got[k].double().cpu()]
    return out


VSD_HEAD_TAU = 0.2          # the tolerance (x diameter) whose VSD the table shows


def score_vsd(root, verts, faces, frames, gt, est, intr, diameter, delta_mm, device):
    """(per matched pose the VSD at the ten BOP tolerances [N,10] (lists), the image width): the frames' depth PNGs of ``root`` as the
    test depth, the mesh rendered at gt / est [N,3,4] in BATCH-sized calls."""
    import torch
    from PIL import Image
    from texpose_amd import pose_error as PE
    cam = json.load(open(os.path.join(root, "scene_camera.json")))
    dev = lambda a, dtype=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    verts_d, faces_d = dev(verts), dev(faces, torch.int32)
    out, W = [], 640
    for i in range(0, len(frames), BATCH):
        ids = sorted(set(frames[i:i + BATCH]))
        planes = [PE.depth_from_png(np.asarray(Image.open(os.path.join(root, "depth", "%06d.png" % f))), float(cam[str(f)]["depth_scale"]))
                  for f in ids]
        depth = torch.stack(planes).to(device)
        H, W = depth.shape[1:]
        index = dev([ids.index(f) for f in frames[i:i + BATCH]], torch.int32)
        r = PE.vsd(verts_d, faces_d, dev(est[i:i + BATCH]), dev(gt[i:i + BATCH]), dev(intr[i:i + BATCH]), depth, diameter, H=H, W=W,
                   delta=delta_mm, frame=index)
        out += r["err"].double().cpu().tolist()
    return out, W


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gt", required=True, metavar="SCENE_DIR")
    ap.add_argument("--est", required=True, metavar="SCENE_DIR|CSV")
    ap.add_argument("--ply", action="append", required=True, metavar="ID=PATH")
    ap.add_argument("--models-info", default=None)
    ap.add_argument("--scene-id", type=int, default=None, help="the scene of a results CSV")
    ap.add_argument("--max-sym-disc-step", type=float, default=0.01, help="discretisation of continuous symmetries (BOP: 0.01)")
    ap.add_argument("--add-thresholds", type=float, nargs="+", default=[0.1, 0.02, 0.05], help="fractions of the diameter")
    ap.add_argument("--proj-px", type=float, default=5.0)
    ap.add_argument("--te-mm", type=float, default=50.0)
    ap.add_argument("--re-deg", type=float, default=5.0)
    ap.add_argument("--json", default=None, metavar="OUT")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--vsd", action="store_true", help="add the Visible Surface Discrepancy and the BOP average recall (GPU only)")
    ap.add_argument("--delta-mm", type=float, default=15.0, help="--vsd: the visibility tolerance (BOP: 15)")
    ap.add_argument("--min-visib", type=float, default=0.1, help="--vsd: the least visib_fract of an instance in the AR rows (BOP: 0.1)")
    a = ap.parse_args(argv)
    if a.vsd and not a.device.startswith("cuda"):
        sys.exit("pose_errors: --vsd renders the meshes with the HIP rasteriser, which has no CPU route; use --device cuda:N")
    import torch
    from texpose_amd import pose_error as PE
    from texpose_amd.bop_scene import read_bop_poses
    from texpose_amd.surfel import load_ply
    device = torch.device(a.device)
    dtype = torch.float32 if device.type == "cuda" else torch.float64          # (the CPU route computes in the tensors' dtype)
    gt = read_bop_poses(a.gt)
    est = read_estimates_scene(a.est) if os.path.isdir(a.est) else read_estimates_csv(a.est, a.scene_id)
    info = {int(k): v for k, v in json.load(open(a.models_info)).items()} if a.models_info else {}
    gt_info = {}
    if a.vsd and os.path.exists(os.path.join(a.gt, "scene_gt_info.json")):
        gt_info = {int(k): v for k, v in json.load(open(os.path.join(a.gt, "scene_gt_info.json"))).items()}
    report = {}
    for item in a.ply:
        oid, path = item.split("=", 1)
        oid = int(oid)
        mesh = load_ply(path)
        pts = mesh[0].astype(np.float64)
        frames, P_gt, P_est, intr, missing = [], [], [], [], []
        visib = {True: [], False: []}          # visib_fract (None: not recorded) of the matched / the missing instances, in their order
        for frame in sorted(gt):
            fr = gt[frame]
            cands = list(est.get(frame, {}).get(oid, []))
            for k in np.nonzero(fr["obj_id"] == oid)[0]:
                entry = gt_info.get(frame, [])
                visib[bool(cands)].append(entry[k].get("visib_fract") if k < len(entry) else None)
                if not cands:
                    missing.append(frame)
                    continue
                R, t = cands.pop(0)
                frames.append(frame)
                P_gt.append(np.concatenate([fr["cam_R_m2c"][k], fr["cam_t_m2c"][k][:, None]], 1))
                P_est.append(np.concatenate([R, np.reshape(t, (3, 1))], 1))
                intr.append(fr["cam_K"])
        sym = PE.symmetry_transforms(info.get(oid, {}), a.max_sym_disc_step).numpy()
        diameter = float(PE.model_diameter(torch.from_numpy(pts).to(device=device, dtype=dtype)))
        n_gt = len(frames) + len(missing)
        if n_gt == 0:
            print("object %d: no ground-truth pose in %s" % (oid, a.gt))
            continue
        err = score_object(pts, np.stack(P_gt), np.stack(P_est), np.stack(intr), sym, device, dtype) if frames else {k: [] for k in ERRORS}
        lost = [math.inf] * len(missing)
        rec = lambda e, th: PE.recall(e + lost, th)
        row = dict(object=oid, vertices=len(pts), symmetries=len(sym), diameter=diameter, poses=n_gt, missing=missing, frames=frames, errors=err)
        for k in ERRORS:
            row["mean_" + k] = statistics.fmean(err[k]) if err[k] else float("nan")
            row["median_" + k] = statistics.median(err[k]) if err[k] else float("nan")
        for th in a.add_thresholds:
            row["recall_add_%g" % th] = rec(err["add"], th * diameter)
            row["recall_adds_%g" % th] = rec(err["adds"], th * diameter)
        row["recall_proj_%gpx" % a.proj_px] = rec(err["proj"], a.proj_px)
        both = [max(r / a.re_deg, t / a.te_mm) for r, t in zip(err["re"], err["te"])]          # < 1: inside both bounds
        row["recall_%gmm_%gdeg" % (a.te_mm, a.re_deg)] = rec(both, 1.0)
        head = a.add_thresholds[0] * diameter
        row["failed_add"] = sorted(set(missing) | {f for f, e in zip(frames, err["add"]) if not e < head})
        if a.vsd:
            e_vsd, width = score_vsd(a.gt, mesh[0], mesh[1], frames, np.stack(P_gt), np.stack(P_est), np.stack(intr), diameter, a.delta_mm,
                                     device) if frames else ([], 640)          # (no estimate at all: every instance is a miss at any width)
            head_vsd = [e[PE.BOP19_TAUS.index(VSD_HEAD_TAU)] for e in e_vsd]
            row["errors"]["vsd"] = e_vsd
            row["mean_vsd"] = statistics.fmean(head_vsd) if head_vsd else float("nan")
            row["median_vsd"] = statistics.median(head_vsd) if head_vsd else float("nan")
            keep = lambda v: v is None or v >= a.min_visib
            found, lost_n = [i for i, v in enumerate(visib[True]) if keep(v)], sum(1 for v in visib[False] if keep(v))
            nan_row = [math.nan] * len(PE.BOP19_TAUS)
            row.update(PE.average_recall([e_vsd[i] for i in found] + [nan_row] * lost_n, [err["mssd"][i] for i in found] + [math.nan] * lost_n,
                                         [err["mspd"][i] for i in found] + [math.nan] * lost_n, diameter, width,
                                         valid=[True] * len(found) + [False] * lost_n))
            row["ar_instances"] = len(found) + lost_n
        report[oid] = row
    cols = ["mean_" + k for k in ERRORS] + ["median_" + k for k in ERRORS] + (["mean_vsd", "median_vsd"] if a.vsd else [])
    recalls = [k for k in next(iter(report.values()), {}) if k.startswith("recall_")] + (["ar_vsd", "ar_mssd", "ar_mspd", "ar"] if a.vsd else [])
    print(" ".join(["%6s %6s %9s" % ("object", "poses", "diameter")] + ["%11s" % c for c in cols] + ["%18s" % c for c in recalls]))
    for oid, row in report.items():
        print(" ".join(["%6d %6d %9.3f" % (oid, row["poses"], row["diameter"])] + ["%11.4f" % row[c] for c in cols]
                       + ["%18.4f" % row[c] for c in recalls]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(gt=a.gt, est=a.est, device=str(device), objects=list(report.values())), f, indent=1)
    return report


if __name__ == "__main__":
    main()
