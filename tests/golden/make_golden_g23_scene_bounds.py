#!/usr/bin/env python3
"""G23: the callable parts of the reference's novel-view bounds (model/nerf_pretrain.py:307-416) on a small scene -- 2 poses, 3 boxes,
24 x 32 pixels:
  (a) camera.get_center_and_ray: the pixel rays of both poses;
  (b) camera.aabb_ray_intersection of every box (passed as the loop passes them: bb_mm * depth.scale / 1000) against those rays;
  (c) camera.get_novel_view_poses_obj: the rotation sweep around an anchor pose (N = 10 as the loop calls it, and an odd N = 7).
The blend of the objects is inline in a trainer method that renders with PyTorch3D and cannot be called here: it is NOT in this file
(tests/scene_bounds_ref.py restates it).

    python tests/golden/make_golden_g23_scene_bounds.py         (build container only; needs the reference checkout)

Inputs and expected outputs are stored; only data is committed.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                                           # noqa: E402


def main():
    opt, camera, M, NeRF, RaySampler, FlexPatchSampler = MG._load_reference()
    torch.set_num_threads(4)
    T = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    B, H, W, scale = 2, 24, 32, 10.0
    sc = MG._scene(B, H, W, seed=23)                                # object origin 0.8 m in front of the camera
    opt.H, opt.W = H, W
    center, ray = camera.get_center_and_ray(opt, sc["pose"], intr=sc["intr"])
    # three boxes in mm (object frame): one around the origin, one off to the side and partly out of view, one thin slab
    bb_mm = T([[[-60.0, -45.0, -50.0], [60.0, 45.0, 50.0]],
               [[30.0, -120.0, -20.0], [150.0, -40.0, 60.0]],
               [[-200.0, 60.0, -5.0], [40.0, 75.0, 5.0]]])
    boxes = (bb_mm * scale) / 1000
    tn, tf, ok = [], [], []
    for k in range(3):
        a, b, v = camera.aabb_ray_intersection(boxes[k, 0][None, None], boxes[k, 1][None, None], center, ray)
        tn.append(a); tf.append(b); ok.append(v.to(torch.uint8))
    anchor = sc["pose"][1]
    novel10 = camera.get_novel_view_poses_obj(opt, anchor, N=10)
    novel7 = camera.get_novel_view_poses_obj(opt, anchor, N=7)
    MG._save("g23_scene_bounds", H=H, W=W, depth_scale=np.float32(scale), intr=sc["intr"], pose=sc["pose"], center=center, ray=ray,
             bb_mm=bb_mm, boxes=boxes, t_near=torch.stack(tn), t_far=torch.stack(tf), valid=torch.stack(ok),
             anchor=anchor, novel10=novel10, novel7=novel7)


if __name__ == "__main__":
    main()
