#!/usr/bin/env python3
"""Time the culled rasteriser (tp_mesh_raster_culled, K34) against the plain one (tp_mesh_raster) on the same device
in the same run: ops.mesh_raster with cull=False and cull=True on the same inputs, whose planes must be equal bit for bit before
anything is timed.  Device events around enough calls to fill about --window seconds after a warm-up of every shape, --repeats repeats
per route, alternating, medians; the shader clock comes from ops.clock_probe before and after.

    python tools/raster_cull_bench.py [--out profiles/raster_cull/raster_cull.json] [--repeats 3] [--window 0.3]

Cases:
  (a) tools/surfel_bench.py's four: bumpy_sphere at 20,160 and 199,808 faces, 480 x 640, B = 1 and 64, colours + NOCS + normals, and
      the same with zbuf + rgb only;
  (b) the 20 k mesh on 128 x 128 crops, B = 64;
  (c) the 12,800-vertex torus of tools/joint_align_bench.py at 480 x 640, B = 8 and 64: the rasteriser alone (depth + colour), and
      ops.joint_align (silhouette + photometric, 20 steps) with cull off and on;
  (d) (a) with texpose_amd.surfel.coherent_face_order applied to the faces.
Per case also: the (tile, chunk) pairs a workgroup enters with and without the chunk test for the first pose (tests/raster_cull_ref.py,
counts of work on the host), and the bytes the call must store (B H W 4 per scalar plane, 12 per vector plane) with the time they
take at 8 TB/s, as a floor."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import kernel_bench as KB  # noqa: E402
from icp_bench import rodrigues, torus  # noqa: E402
from surfel_bench import bumpy_sphere  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of calls per timed repeat")
    ap.add_argument("--skip-counts", action="store_true", help="leave out the host-side chunk-iteration counts")
    a = ap.parse_args(argv)
    import torch
    import raster_cull_ref as CULL
    from oracle.texpose_oracle import LINEMOD_K, rotation_from_axis_angle
    from texpose_amd import ops
    from texpose_amd.surfel import coherent_face_order, nocs_normalisation
    if not torch.cuda.is_available():
        raise SystemExit("raster_cull_bench: needs a GPU (a CPU run cannot give a time)")
    dev = torch.device("cuda:0")
    clock_before = KB.shader_clock()
    t_start = time.time()
    K1 = np.array(LINEMOD_K, dtype=np.float32)
    rows = []

    def race(routes):
        """name -> callable: each warmed up, its iteration count sized from one timed call to fill the window; alternating repeats."""
        iters = {}
        for name, fn in routes.items():
            one = KB.timed(fn, 1, a.warmup) * 1e-6
            iters[name] = int(min(400, max(3, a.window / max(one, 1e-6))))
        med, times = KB.race(routes, iters, 1, a.repeats)
        return med, times, iters

    def raster_case(tag, verts, faces, pose, K, H, W, planes, order):
        B = pose.shape[0]
        v, f = torch.from_numpy(verts).to(dev), torch.from_numpy(np.ascontiguousarray(faces)).to(dev)
        P, Kd = torch.from_numpy(pose).to(dev), torch.from_numpy(K).to(dev)
        kw = dict(face_ids=False, normals=False)
        vector_planes = 0
        if "rgb" in planes:
            kw["vcolor"] = torch.from_numpy(np.random.RandomState(1).uniform(size=verts.shape).astype(np.float32)).to(dev)
            vector_planes += 1
        if "nocs" in planes:
            kw["nocs_norm"] = nocs_normalisation(verts)
            vector_planes += 1
        if "normal" in planes:
            kw["normals"] = True
            vector_planes += 1
        plain = lambda: ops.mesh_raster(v, f, P, Kd, H=H, W=W, cull=False, **kw)
        culled = lambda: ops.mesh_raster(v, f, P, Kd, H=H, W=W, cull=True, **kw)
        x, y = plain(), culled()
        torch.cuda.synchronize()
        if set(x) != set(y) or not all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for k in x):
            raise SystemExit("raster_cull_bench: %s: the culled planes differ from the plain ones; nothing was timed" % tag)
        med, times, iters = race({"plain": plain, "culled": culled})
        store = B * H * W * (4 + 12 * vector_planes)
        row = dict(case=tag, faces=int(len(faces)), order=order, B=B, H=H, W=W, planes=sorted(planes | {"zbuf"}), us=med, us_all_repeats=times, iters=iters,
                   plain_over_culled=med["plain"] / med["culled"], planes_bit_equal=True, covered_fraction=float((x["zbuf"] > 0).float().mean()),
                   bytes_stored=store, store_floor_us=store / HBM_BYTES_PER_S * 1e6,
                   workspace_mb=dict(plain=B * len(faces) * 64 / 2 ** 20, culled=(B * len(faces) * 64 + 16 * B * -(-len(faces) // 256)) / 2 ** 20))
        # faster by more than the spread between the repeats: the slowest culled repeat against the fastest plain one
        row["culled_faster_beyond_spread"] = bool(max(times["culled"]) < min(times["plain"]))
        if not a.skip_counts:
            c = CULL.counts(verts, faces, pose[0], K if K.ndim == 2 else K[0], H, W)
            row["chunk_iterations_first_pose"] = dict(plain=c["plain"], culled=c["culled"], faces_per_busy_tile_mean=c["faces_mean"],
                                                      faces_per_busy_tile_max=c["faces_max"])
        rows.append(row)
        print(json.dumps(row), flush=True)

    def surfel_poses(rs, B, xy, z):
        return np.stack([np.concatenate([rotation_from_axis_angle(rs.uniform(-2, 2, 3)),
                                         [[rs.uniform(-xy[0], xy[0])], [rs.uniform(-xy[1], xy[1])], [rs.uniform(*z)]]], 1) for _ in range(B)]).astype(np.float32)

    everything, colour = {"rgb", "nocs", "normal"}, {"rgb"}
    # (a), (d): surfel_bench's meshes and pose ranges at 480 x 640; (b): the crops
    for n_lat, n_lon in ((71, 144), (224, 448)):
        verts, faces = bumpy_sphere(n_lat, n_lon)
        perm = coherent_face_order(verts, faces)
        for B in (1, 64):
            pose = surfel_poses(np.random.RandomState(100 + B), B, (40.0, 30.0), (600.0, 900.0))
            for planes in (everything, colour):
                raster_case("a", verts, faces, pose, K1, 480, 640, planes, "mesh")
                raster_case("d", verts, faces[perm], pose, K1, 480, 640, planes, "morton")
        if n_lat == 71:
            crop = K1.copy()
            crop[0, 2] = crop[1, 2] = 64.0
            pose = surfel_poses(np.random.RandomState(7), 64, (2.0, 2.0), (600.0, 900.0))
            for order, fc in (("mesh", faces), ("morton", faces[perm])):
                raster_case("b", verts, fc, pose, crop, 128, 128, everything, order)
    # (c): joint_align_bench's torus, alone and inside the joint loop
    H, W = 480, 640
    verts, faces = torus(160, 80)
    vcolor = (0.5 + 0.5 * np.sin(verts.astype(np.float64) / 8.0 + np.array([0.0, 1.0, 2.0]))).astype(np.float32)
    verts_d, faces_d, vcolor_d = torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), torch.from_numpy(vcolor).to(dev)
    rs = np.random.RandomState(0)
    for B in (8, 64):
        truth, start = np.zeros((B, 3, 4), np.float32), np.zeros((B, 3, 4), np.float32)
        for b in range(B):
            q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
            if np.linalg.det(q) < 0:
                q[:, 0] *= -1
            t = rs.uniform(-40, 40, 3) + [0.0, 0.0, 400.0]
            w, dt = rs.normal(size=3), rs.normal(size=3)
            truth[b] = np.concatenate([q, t[:, None]], 1)
            start[b] = np.concatenate([rodrigues(w * np.radians(2.0) / np.linalg.norm(w)) @ q, (t + dt * 5.0 / np.linalg.norm(dt))[:, None]], 1)
        raster_case("c", verts, faces, start, np.tile(K1, (B, 1, 1)), H, W, colour, "mesh")
        truth_d, start_d, K = torch.from_numpy(truth).to(dev), torch.from_numpy(start).to(dev), torch.from_numpy(np.tile(K1, (B, 1, 1))).to(dev)
        shot = ops.mesh_raster(verts_d, faces_d, truth_d, K, H=H, W=W, vcolor=vcolor_d, face_ids=False, normals=False)
        image = torch.where((shot["zbuf"] > 0)[..., None], shot["rgb"], torch.full_like(shot["rgb"], 0.5)).contiguous()
        sdf = ops.mask_sdf((shot["zbuf"] > 0).to(torch.uint8))
        ws = ops.joint_align_workspace(B, H, W, dev, terms=2)
        loop = lambda cull: ops.joint_align(verts_d, faces_d, start_d, K, vcolor=vcolor_d, sdf=sdf, image=image, tau_px=4.0, tau=0.5, iters=20,
                                            workspace=ws, cull=cull)
        x, y = loop(False), loop(True)
        torch.cuda.synchronize()
        if set(x) != set(y) or not all(torch.equal(x[k].view(torch.uint8), y[k].view(torch.uint8)) for k in x):
            raise SystemExit("raster_cull_bench: joint_align with cull differs from joint_align without at B = %d; nothing was timed" % B)
        med, times, iters = race({"plain": lambda: loop(False), "culled": lambda: loop(True)})
        rows.append(dict(case="c_joint_align_20", faces=int(len(faces)), order="mesh", B=B, H=H, W=W, us=med, us_all_repeats=times, iters=iters,
                         plain_over_culled=med["plain"] / med["culled"], results_bit_equal=True, status_ok=int((x["status"] == 0).sum()),
                         culled_faster_beyond_spread=bool(max(times["culled"]) < min(times["plain"]))))
        print(json.dumps(rows[-1]), flush=True)
    res = dict(bench="raster_cull", device=torch.cuda.get_device_name(0), repeats=a.repeats, warmup=a.warmup, window_s=a.window,
               shader_clock_ghz_before=clock_before, shader_clock_ghz_after=KB.shader_clock(), seconds=time.time() - t_start, rows=rows)
    KB.finish(res, a.out)


if __name__ == "__main__":
    main()
