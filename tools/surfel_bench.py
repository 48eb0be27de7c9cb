#!/usr/bin/env python3
"""Surfel-map rasteriser speed (tp_mesh_raster: face setup + raster / shading + normals) at 480x640 for a generated closed mesh of
~20 k and ~200 k faces, B = 1 and B = 64 poses per call, timed with HIP events.  Prints one JSON document."""
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


def main():
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
    print(json.dumps(res))


if __name__ == "__main__":
    main()
