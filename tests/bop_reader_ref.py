"""numpy / PIL statement of what the reference's data layer (data/lm.py) takes from a BOP scene folder, for the tests.  The JSON parts
(pose, box) are pinned to the reference's own methods by golden G24; the image parts restate its expressions without its crop and
resize (cv2 is not installed, so those methods cannot be called).

    pose   lm.py:103-107   eye(4) with R = cam_R_m2c as [3,3] float32 and t = float32(cam_t_m2c) / 1000 (metres)
    box    lm.py:161-180   bbox_obj -> center (row, column), scale, resize for a square crop of side `res`
    mask   lm.py:272-300   the PNG > 0, at native size
    depth  lm.py:255-270   PNG / 1000 * depth_scale (metres), at native size
"""
import json
import os

import numpy as np

F = np.float32


def load_scene(root):
    out = {}
    for name in ("scene_gt", "scene_gt_info", "scene_camera", "scene_object"):
        path = os.path.join(root, name + ".json")
        if os.path.exists(path):
            with open(path) as f:
                out[name] = json.load(f)
    return out


def gt_index(scene, frame, model_name=None):
    """lm.py:99-102: the entry of the frame's gt list -- scene_object.json's for a multi-object scene, else 0."""
    return 0 if model_name is None else int(scene["scene_object"][str(frame)][model_name])


def raw_pose(scene, frame, index):
    """[4,4] float32: rotation as stored, translation in metres (float32 of the stored mm, then / 1000)."""
    entry = scene["scene_gt"][str(frame)][index]
    R = np.asarray(entry["cam_R_m2c"], dtype=np.float64).reshape(3, 3).astype(F)
    t = np.asarray(entry["cam_t_m2c"], dtype=np.float64).astype(F) / F(1000)
    return np.concatenate([np.concatenate([R, t[:, None]], axis=1), np.array([[0, 0, 0, 1]], dtype=F)], axis=0)


def get_2d_bbox(scene, frame, index, res, box_format=None):
    """-> (center [2] as (row, column), side of the square crop, res / side).  The reference names the box's last two fields (h, w)
    unless data.box_format is 'wh'; the crop's side is one and a half times the longer of the two, truncated."""
    if box_format not in (None, "hw", "wh"):
        raise NotImplementedError(box_format)
    left, top, third, fourth = scene["scene_gt_info"][str(frame)][index]["bbox_obj"]
    tall, wide = (fourth, third) if box_format == "wh" else (third, fourth)
    side = int(max(tall, wide) * 1.5)
    return np.array([int(top + tall / 2), int(left + wide / 2)]), side, res / side


def mask_of(root, frame, index, sub="mask"):
    from PIL import Image
    return np.asarray(Image.open(os.path.join(root, sub, "%06d_%06d.png" % (frame, index)))) > 0


def depth_metres(root, scene, frame):
    from PIL import Image
    png = np.asarray(Image.open(os.path.join(root, "depth", "%06d.png" % frame)))
    return png / 1000. * scene["scene_camera"][str(frame)]["depth_scale"]
