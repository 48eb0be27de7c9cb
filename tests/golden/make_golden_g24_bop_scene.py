#!/usr/bin/env python3
"""G24: what the reference's data layer (data/lm.py) takes from the JSON files of a BOP scene folder, pinned on a tiny hand-written
scene of 2 frames x 3 objects (tests/golden/g24_bop_scene/: scene_gt.json, scene_gt_info.json, scene_camera.json, scene_object.json;
no images).

Run in the build container only:   python tests/golden/make_golden_g24_bop_scene.py

data/lm.py is imported with make_golden's stubs (plyfile stubbed as for G16 and G22) and its own Dataset.get_2d_bbox (lm.py:161-180) and
Dataset.get_all_camera_poses(source='gt') (lm.py:91-110, through its parse_raw_camera) are CALLED on an object that carries the
attributes Dataset.initialize_meta would have loaded from the folder: so the key names (cam_R_m2c, cam_t_m2c, bbox_obj), the list order
(scene_object.json's index into the frame's gt list), the units (mm / 1000, then * nerf.depth.scale) and the order of the box's fields
are the reference's code.  cv2 is not installed: the methods that read images (get_image, get_depth, get_obj_mask) cannot be called and
are NOT in this file (tests/bop_reader_ref.py restates what they take from the PNG files).

Only data is stored: the split list, the options used and what the two methods returned."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                                            # noqa: E402

SCENE = os.path.join(HERE, "g24_bop_scene")
RES, DEPTH_SCALE = 128, 10.0


def main():
    MG._install_stubs()
    sys.modules["plyfile"] = types.ModuleType("plyfile")
    sys.path.insert(0, MG.REF)
    os.chdir(MG.REF)
    import data.lm as L                                              # noqa: E402
    D = L.Dataset
    load = lambda name: json.load(open(os.path.join(SCENE, name + ".json")))
    objects = load("scene_object")
    # the split list as the reference writes it: "<model name> <folder> <frame>"
    lines = ["%s g24_bop_scene %d" % (name, int(frame)) for frame in sorted(objects, key=int) for name in sorted(objects[frame])]
    me = types.SimpleNamespace(list=lines, multi_obj=True, scene_obj_all=objects, scene_gt_all=load("scene_gt"),
                               scene_info_all=load("scene_gt_info"), parse_raw_camera=D.parse_raw_camera)
    opt = MG._AttrDict(H=RES, W=RES, data=dict(box_format=None), nerf=dict(depth=dict(scale=DEPTH_SCALE)))
    poses = D.get_all_camera_poses(me, opt, source="gt")             # [6,3,4], t in nerf.depth.scale units
    out = dict(frame=[], gt_index=[], model=[])
    for fmt in ("none", "wh"):
        out.update({"center_" + fmt: [], "scale_" + fmt: [], "resize_" + fmt: []})
    for idx, line in enumerate(lines):
        name, _, frame = line.split()
        k = int(objects[frame][name])
        out["frame"].append(int(frame)); out["gt_index"].append(k); out["model"].append(name)
        for fmt in ("none", "wh"):
            opt.data.box_format = None if fmt == "none" else fmt
            center, scale, resize = D.get_2d_bbox(me, opt, idx, k)
            out["center_" + fmt].append(np.asarray(center, dtype=np.int64)); out["scale_" + fmt].append(int(scale))
            out["resize_" + fmt].append(float(resize))
    for i, line in enumerate(lines):
        print(line, "->", out["gt_index"][i], poses[i, :, 3].tolist(), out["center_none"][i].tolist(), out["scale_none"][i], out["center_wh"][i].tolist())
    MG._save("g24_bop_scene", res=np.int64(RES), depth_scale_opt=np.float32(DEPTH_SCALE), frame=np.array(out["frame"], dtype=np.int64),
             gt_index=np.array(out["gt_index"], dtype=np.int64), pose=poses.float(),
             **{k: (np.stack(v) if k.startswith("center") else np.array(v, dtype=np.int64 if k.startswith("scale") else np.float64))
                for k, v in out.items() if k[:6] in ("center", "scale_", "resize")})


if __name__ == "__main__":
    main()
