#!/usr/bin/env python3
"""G21: the reference's normals from a rendered depth map (compute_surfelinfo.normal_from_depth, rays from
compute_box.get_center_and_ray), the third of the four surfel maps an adaptation loop reads.

Run in the build container only:   python tests/golden/make_golden_g21_surfel_normals.py

The reference modules are imported with make_golden's stubs plus stand-ins for the renderer-side imports the two functions never
call (pytorch3d.io / renderer / structures, open3d, tools.mvrenderer, data.cad_model).  The depth map (60 x 80, mm) holds
background (-1, as PyTorch3D's zbuf), two silhouettes, a roof crease and a step between two surfaces.  Every input is a short dyadic
number (focal length 64, integer principal point, a signed-permutation rotation, depths on a 1/64 grid), so the reference's fp32
rays and points are exact and an fp64 restatement agrees with its output to the rounding of the final cross product."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG                                            # noqa: E402


def _stub(name, **attrs):
    m = sys.modules.get(name) or types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _depth_map(H=60, W=80):
    ii, jj = np.mgrid[0:H, 0:W].astype(np.float64)
    d = 600.0 + np.abs(jj - 40.0) * 0.5 + ii * 0.25                 # roof: crease along column 40
    d = np.where(jj > 58, d - 9.0, d)                                # a step between two surfaces
    inside = (ii >= 8) & (ii <= 50) & (jj >= 10) & (jj <= 70)
    inside &= ~((ii > 30) & (jj < 22))                               # a notch: more silhouette
    d = np.round(d * 64.0) / 64.0
    return np.where(inside, d, -1.0).astype(np.float32)


def main():
    MG._install_stubs()
    _stub("pytorch3d.structures", Meshes=object)
    _stub("pytorch3d.io", load_ply=None, load_obj=None)
    _stub("pytorch3d.renderer", TexturesVertex=object, Textures=object)
    _stub("open3d")
    _stub("tqdm", tqdm=lambda x, **k: x)
    data = _stub("data")
    data.cad_model = _stub("data.cad_model", CAD_Model=object)
    tools = _stub("tools")
    tools.__path__ = []
    tools.mvrenderer = _stub("tools.mvrenderer", Pose=object, MVRenderer=object)
    sys.path.insert(0, MG.REF)
    os.chdir(MG.REF)
    import compute_surfelinfo as CS                                  # noqa: E402
    import mesh_raster_ref as REF                                    # noqa: E402  (the restatement, to report its agreement)
    H, W = 60, 80
    depth = _depth_map(H, W)
    K = np.array([[64.0, 0.0, 40.0], [0.0, 64.0, 30.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    R = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, -1.0], [-1.0, 0.0, 0.0]], dtype=np.float32)   # det +1
    t = np.array([12.0, -20.0, 580.0], dtype=np.float32)
    pose = np.concatenate([R, t[:, None]], axis=1)
    normal = CS.normal_from_depth(torch.from_numpy(pose)[None], torch.from_numpy(depth)[None], torch.from_numpy(K)[None], h=H, w=W)
    normal = normal[0].permute(1, 2, 0).numpy().astype(np.float32)   # [H,W,3] as compute_surfelinfo.py:122 stores it
    err = np.abs(REF.normal_from_depth(depth, pose, K) - normal).max()
    print("restatement vs reference: max |diff| %.3g; covered pixels %d" % (err, int((depth > 0).sum())))
    MG._save("g21_surfel_normals", depth=depth, pose=pose, K=K, normal=normal)


if __name__ == "__main__":
    main()
