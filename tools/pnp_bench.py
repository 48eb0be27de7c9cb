#!/usr/bin/env python3
"""Time the PnP-RANSAC kernels (K28) on the correspondence lists of rendered NOCS maps: 480 x 640 renders of a torus
by the HIP rasteriser (K19) at B = 64 poses, about 20,000 covered pixels each, T = 256 hypotheses.

  * `ops.pnp_score` (all T poses of all B images, two launches) against `pnp.score_torch`, the same rule in plain torch ops in fp32, on
    the same device in the same run.  The counts are compared before anything is timed: the number that differ and the largest
    difference are recorded, and a difference above 0.1 % of the entries ends the run.
  * `ops.pnp_ransac` (hypotheses, scores, selection and five Gauss-Newton steps; 16 launches) as a whole: microseconds per batch and
    poses per second; nothing in plain torch stands beside it.
  * `ops.corr_from_nocs` on the 64 maps.

Device events around many iterations after a warm-up, three repeats per route, alternating, medians; the shader clock comes from
ops.clock_probe before and after.  The lists are cut to the largest count of the batch (N' entries per image) before the timed calls.

    python tools/pnp_bench.py [--out profiles/pnp/pnp.json] [--iters 20] [--end-to-end]

--end-to-end also solves the tests' 64 x 80 renders (torus and rippled sphere, clean and with 30 % of the NOCS values replaced) and
records the pose error against the truth of the kernels and of the numpy restatement tests/pnp_ref.py on the same lists (needs the
repository's tests/ folder; nothing is timed there)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import kernel_bench as KB  # noqa: E402
from texture_bake_ref import torus  # noqa: E402  (numpy only: the tests' mesh generators; needs the repository's tests/ folder)

LINEMOD_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)


def rotation(rs):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def pose_error(pose, truth):
    M = pose[:, :3] @ truth[:, :3].T
    sin = 0.5 * np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.degrees(np.arctan2(sin, (np.trace(M) - 1.0) / 2.0))), float(np.linalg.norm(pose[:, 3] - truth[:, 3]))


def end_to_end(torch, ops, dev):
    """The case of tests/pnp_ref.py::end_to_end_inputs (what the GPU test solves), both routes' errors against the truth."""
    import pnp_ref as REF                                       # (numpy only: the restatement and the case's inputs)
    from texpose_amd.surfel import nocs_normalisation
    t = lambda x, dtype=torch.float32: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dtype)
    rows = []
    for mesh in ("torus", "sphere"):
        c = REF.end_to_end_inputs(mesh)
        c["norm"] = nocs_normalisation(c["verts"])
        r = ops.mesh_raster(t(c["verts"]), t(c["faces"], torch.int32), t(c["P"]), t(c["K"]), H=c["H"], W=c["W"], nocs_norm=c["norm"], face_ids=False,
                            normals=False)
        c["mask"] = r["zbuf"] > 0
        for dirty in (False, True):
            nocs, kept = r["nocs"].clone(), c["mask"].cpu().numpy()
            if dirty:
                touched, values = REF.end_to_end_corruption(kept)
                nocs[t(touched, torch.bool)] = t(values)
            corr = ops.corr_from_nocs(nocs, c["mask"], *c["norm"])
            Kb = np.tile(c["K"], (2, 1, 1))
            got = ops.pnp_ransac(corr["xy"], corr["xyz"], corr["count"], torch.from_numpy(Kb).to(dev), T=256, tau_px=2.0, iters=5, seed=1)
            want = REF.ransac_ref(corr["xy"].cpu().numpy(), corr["xyz"].cpu().numpy(), corr["count"].cpu().numpy(), Kb, T=256, tau=2.0, iters=5, seed=1)
            for b in range(2):
                re, te = pose_error(got["pose"][b].double().cpu().numpy(), c["P"][b].astype(np.float64))
                re_w, te_w = pose_error(want["pose32"][b].astype(np.float64), c["P"][b].astype(np.float64))
                rows.append(dict(mesh=mesh, dirty=dirty, image=b, n=int(corr["count"][b]), inliers=int(got["inliers"][b]), inliers_restatement=int(want["inliers"][b]),
                                 rot_err_deg=re, trans_err_mm=te, rot_err_deg_restatement=re_w, trans_err_mm_restatement=te_w))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    KB.add_timing_args(ap, iters=20, warmup=3, repeats=3)
    ap.add_argument("--end-to-end", action="store_true")
    a = ap.parse_args(argv)
    import torch
    from texpose_amd import ops, pnp
    from texpose_amd.surfel import nocs_normalisation
    if not torch.cuda.is_available():
        raise SystemExit("pnp_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)

    clock_before = KB.shader_clock()
    t_start = time.time()
    B, T, H, W, tau = 64, 256, 480, 640, 2.0
    verts, faces = torus(160, 80)
    norm = nocs_normalisation(verts)
    P = np.stack([np.concatenate([rotation(rs), rs.uniform(-20, 20, (3, 1)) + [[0.0], [0.0], [340.0]]], 1) for _ in range(B)]).astype(np.float32)
    t = lambda x, dtype=torch.float32: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dtype)
    K = t(np.tile(LINEMOD_K, (B, 1, 1)))
    r = ops.mesh_raster(t(verts), t(faces, torch.int32), t(P), K, H=H, W=W, nocs_norm=norm, face_ids=False, normals=False)
    nocs, mask = r["nocs"], (r["zbuf"] > 0).to(torch.uint8)
    ws_full = ops.pnp_workspace(B, H * W, T, dev)
    corr_out = dict(xy=torch.zeros(B, H * W, 2, device=dev), xyz=torch.zeros(B, H * W, 3, device=dev), count=torch.empty(B, device=dev, dtype=torch.int32))
    corr_call = lambda: ops.corr_from_nocs(nocs, mask, *norm, workspace=ws_full, out=corr_out)
    corr = corr_call()
    count = corr["count"]
    n_max = int(count.max())
    xy, xyz = corr["xy"][:, :n_max].contiguous(), corr["xyz"][:, :n_max].contiguous()
    ws = ops.pnp_workspace(B, n_max, T, dev)
    first = ops.pnp_ransac(xy, xyz, count, K, T=T, tau_px=tau, iters=5, seed=0)
    out = {k: torch.empty_like(v) for k, v in first.items()}
    ransac = lambda: ops.pnp_ransac(xy, xyz, count, K, T=T, tau_px=tau, iters=5, seed=0, workspace=ws, out=out)
    hyp, valid = first["hyp"], first["hyp_valid"]
    inl = torch.empty(B, T, device=dev, dtype=torch.int32)
    kernel = lambda: ops.pnp_score(xy, xyz, count, K, hyp, tau_px=tau, valid=valid, inliers=inl)
    plain = lambda: pnp.score_torch(xy, xyz, count, K, hyp, tau, valid)
    got, want = kernel().clone(), plain()
    differ, largest = int((got != want).sum()), int((got - want).abs().max())
    if largest > 1e-3 * n_max:                                      # (a count off by one: a decision that two fp32 divisions round apart)
        raise SystemExit("pnp_bench: the two scoring routes disagree on %d of %d counts (largest difference %d); nothing was timed"
                         % (differ, B * T, largest))
    med, times = KB.race({"tp_pnp_score": kernel, "torch": plain, "pnp_ransac": ransac, "corr_from_nocs": corr_call},
                         {"tp_pnp_score": a.iters, "torch": max(2, a.iters // 10), "pnp_ransac": a.iters, "corr_from_nocs": a.iters}, a.warmup, a.repeats)
    n_sum = int(count.sum())
    errs = [pose_error(first["pose"][b].double().cpu().numpy(), P[b].astype(np.float64)) for b in range(B)]
    row = dict(B=B, T=T, H=H, W=W, tau_px=tau, iters=5, n_mean=n_sum / B, n_max=n_max, us=med, us_all_repeats=times,
               torch_over_tp_pnp_score=med["torch"] / med["tp_pnp_score"], reprojections=n_sum * T,
               reprojections_per_second=n_sum * T / (med["tp_pnp_score"] * 1e-6), poses_per_second=B / (med["pnp_ransac"] * 1e-6),
               counts_equal=differ == 0, counts_differing=differ, largest_count_difference=largest, valid_hypotheses=int(valid.sum()), status_ok=int((first["status"] == 0).sum()),
               mean_inlier_share=float((first["inliers"].float() / count.float()).mean()),
               max_rot_err_deg=max(e[0] for e in errs), max_trans_err_mm=max(e[1] for e in errs))
    print(json.dumps(row), flush=True)
    res = dict(bench="pnp", device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, repeats=a.repeats,
               shader_clock_ghz_before=clock_before, shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start, rows=[row])
    if a.end_to_end:
        res["end_to_end_64x80"] = end_to_end(torch, ops, dev)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
