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
per-pose errors.  Units: the models' (mm), pixels, degrees."""
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
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import pose_error as PE
    from texpose_amd.bop_scene import read_bop_poses
    from texpose_amd.surfel import load_ply
    device = torch.device(a.device)
    dtype = torch.float32 if device.type == "cuda" else torch.float64          # (the CPU route computes in the tensors' dtype)
    gt = read_bop_poses(a.gt)
    est = read_estimates_scene(a.est) if os.path.isdir(a.est) else read_estimates_csv(a.est, a.scene_id)
    info = {int(k): v for k, v in json.load(open(a.models_info)).items()} if a.models_info else {}
    report = {}
    for item in a.ply:
        oid, path = item.split("=", 1)
        oid = int(oid)
        pts = load_ply(path)[0].astype(np.float64)
        frames, P_gt, P_est, intr, missing = [], [], [], [], []
        for frame in sorted(gt):
            fr = gt[frame]
            cands = list(est.get(frame, {}).get(oid, []))
            for k in np.nonzero(fr["obj_id"] == oid)[0]:
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
        report[oid] = row
    cols = ["mean_" + k for k in ERRORS] + ["median_" + k for k in ERRORS]
    recalls = [k for k in next(iter(report.values()), {}) if k.startswith("recall_")]
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
