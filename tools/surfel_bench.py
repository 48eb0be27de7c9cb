#!/usr/bin/env python3
"""Surfel-map rasteriser speed (tp_mesh_raster: face setup + raster / shading + normals) at 480x640 for a generated closed mesh of
~20 k and ~200 k faces, B = 1 and B = 64 poses per call, timed with HIP events.  Prints one JSON document.

--online: instead, the two routes by which the maps of B = 64 frames reach a training step, for the same two meshes at 480x640 and for
128x128 crops: SurfelRenderer.data_layer_maps (tp_mesh_raster + tp_surfel_finish; HIP events, 5 calls after one warm-up, also split into
the two stages) and the file route of the reference (raw render -> write_surfel_frame -> read_surfel_frame -> upload; wall time of one pass).
--out PATH also writes the JSON document to PATH."""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bumpy_sphere(n_lat, n_lon, radius=50.0):
    """UV sphere with a radial ripple (self-occluding, every face small): 2 n_lon (n_lat - 1) faces."""
    th = np.linspace(0, math.pi, n_lat + 1)
    ph = np.linspace(0, 2 * math.pi, n_lon, endpoint=False)
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = radius * (1 + 0.08 * np.sin(7 * T) * np.cos(5 * P))
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.sin(T) * np.sin(P), r * np.cos(T)], -1).reshape(-1, 3)
    idx = np.arange((n_lat + 1) * n_lon).reshape(n_lat + 1, n_lon)
    a, b = idx[:-1], np.roll(idx[:-1], -1, axis=1)
    c, d = idx[1:], np.roll(idx[1:], -1, axis=1)
    f = np.concatenate([np.stack([a, c, d], -1)[:-1], np.stack([a, d, b], -1)[1:]]).reshape(-1, 3)   # no pole-to-pole slivers
    return v.astype(np.float32), f.astype(np.int32)


def _events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def online():
    import tempfile
    import time
    import torch
    from oracle.texpose_oracle import LINEMOD_K, rotation_from_axis_angle
    from texpose_amd import ops
    from texpose_amd.surfel import MAP_KEYS, SurfelRenderer, read_surfel_frame, write_surfel_frame
    dev = torch.device("cuda:0")
    B, reps, depth_scale = 64, 5, 10.0
    rs = np.random.RandomState(0)
    res = {"B": B, "device": torch.cuda.get_device_name(0), "cases": []}
    run = None
    for n_lat, n_lon, H, W in ((71, 144, 480, 640), (224, 448, 480, 640), (71, 144, 128, 128)):
        verts, faces = bumpy_sphere(n_lat, n_lon)
        vcol = rs.uniform(size=verts.shape).astype(np.float32)
        r = SurfelRenderer(verts, faces, vcol, H, W, dev)
        crop = H == 128
        K = np.array(LINEMOD_K, dtype=np.float32)
        if crop:                                               # crop-like intrinsics: the object fills much of the image
            K[0, 2], K[1, 2] = W / 2.0, H / 2.0
        xy = (2.0, 2.0) if crop else (40.0, 30.0)
        pose = np.stack([np.concatenate([rotation_from_axis_angle(rs.uniform(-2, 2, 3)),
                                         [[rs.uniform(-xy[0], xy[0]) / 100], [rs.uniform(-xy[1], xy[1]) / 100], [rs.uniform(6.0, 9.0)]]], 1)
                         for _ in range(B)])                   # t in nerf.depth.scale units (dm at depth_scale 10)
        pose = torch.from_numpy(pose.astype(np.float32)).to(dev)
        K = torch.from_numpy(K).to(dev)
        run = lambda: r.data_layer_maps(pose, K, depth_scale)
        ms_both = _events_ms(run, reps)
        ms_raster = _events_ms(lambda: r._raster(pose, K, depth_scale), reps)
        ras = r._raster(pose, K, depth_scale)
        ms_finish = _events_ms(lambda: ops.surfel_finish(ras["zbuf"], ras["nocs"], ras["normal"], ras["rgb"]), reps)
        maps = run()
        with tempfile.TemporaryDirectory() as root:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            raw = r(pose, K, depth_scale)
            for b in range(B):
                write_surfel_frame(root, "bench", b, raw, b)
            t1 = time.perf_counter()
            dec = [read_surfel_frame(root, "bench", b) for b in range(B)]
            up = {k: torch.stack([d[k] for d in dec]).to(dev) for k in MAP_KEYS}
            torch.cuda.synchronize()
            t2 = time.perf_counter()
        equal = all(torch.equal(up[k], maps[k]) for k in MAP_KEYS)
        res["cases"].append({"faces": int(len(faces)), "H": H, "W": W, "online_ms": round(ms_both, 3), "raster_ms": round(ms_raster, 3),
                             "finish_ms": round(ms_finish, 3), "file_route_ms": round((t2 - t0) * 1e3, 1),
                             "file_write_ms": round((t1 - t0) * 1e3, 1), "file_read_upload_ms": round((t2 - t1) * 1e3, 1),
                             "routes_bit_identical": bool(equal), "covered_fraction": round(float(maps.mask_syn.mean()), 4)})
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        words = ops.clock_probe(windows=16, window_us=5000)
    for _ in range(max(2, int(100.0 / res["cases"][-1]["online_ms"]) + 1)):
        run()
    torch.cuda.synchronize()
    res["clock_ghz_last_case"] = round(ops.clock_ghz_from_probe(words), 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--online", action="store_true", help="time data_layer_maps against the file route instead of the rasteriser alone")
    ap.add_argument("--out", default=None, help="also write the JSON document to this path")
    a = ap.parse_args()
    res = online() if a.online else raster()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res) + "\n")


def raster():
    import torch
    from oracle.texpose_oracle import LINEMOD_K, rotation_from_axis_angle
    from texpose_amd import ops
    from texpose_amd.surfel import nocs_normalisation
    dev = torch.device("cuda:0")
    H, W, reps = 480, 640, 5
    rs = np.random.RandomState(0)
    res = {"H": H, "W": W, "device": torch.cuda.get_device_name(0), "cases": []}
    for n_lat, n_lon in ((71, 144), (224, 448)):
        verts, faces = bumpy_sphere(n_lat, n_lon)
        vcol = rs.uniform(size=verts.shape).astype(np.float32)
        norm = nocs_normalisation(verts)
        v, f, c = (torch.from_numpy(x).to(dev) for x in (verts, faces, vcol))
        for B in (1, 64):
            pose = np.stack([np.concatenate([rotation_from_axis_angle(rs.uniform(-2, 2, 3)),
                                             [[rs.uniform(-40, 40)], [rs.uniform(-30, 30)], [rs.uniform(600, 900)]]], 1) for _ in range(B)])
            pose = torch.from_numpy(pose.astype(np.float32)).to(dev)
            K = torch.tensor(LINEMOD_K, dtype=torch.float32, device=dev)
            run = lambda: ops.mesh_raster(v, f, pose, K, H=H, W=W, vcolor=c, nocs_norm=norm, face_ids=False, normals=True)
            out = run()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                run()
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / reps
            res["cases"].append({"faces": int(len(faces)), "B": B, "ms_per_call": round(ms, 3), "ms_per_image": round(ms / B, 4),
                                 "images_per_s": round(1000.0 * B / ms, 1),
                                 "covered_fraction": round(float((out["zbuf"] > 0).float().mean()), 4),
                                 "workspace_mb": round(B * len(faces) * 64 / 2 ** 20, 1)})
    # outside the timed region: the shader clock held while the last case runs (tp_clock_probe on a side stream, 16 x 5 ms windows)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        words = ops.clock_probe(windows=16, window_us=5000)
    for _ in range(max(2, int(100.0 / res["cases"][-1]["ms_per_call"]) + 1)):
        run()
    torch.cuda.synchronize()
    res["clock_ghz_last_case"] = round(ops.clock_ghz_from_probe(words), 3)
    return res


if __name__ == "__main__":
    main()
