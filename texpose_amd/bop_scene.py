"""Novel views as an annotated BOP scene folder, the layout the reference's data layer (data/lm.py) reads its frames from:

    rgb/{frame:06d}.png                          8-bit RGB
    depth/{frame:06d}.png                        16-bit; png * depth_scale = mm
    mask/{frame:06d}_{gt_index:06d}.png          0 / 255: the object's full silhouette inside the image
    mask_visib/{frame:06d}_{gt_index:06d}.png    0 / 255: the part no nearer object hides
    scene_camera.json    frame -> {cam_K (row-major), depth_scale = 1000 / png_per_metre}
    scene_gt.json        frame -> [{obj_id, cam_R_m2c (9 values), cam_t_m2c (mm)}] in blend order
    scene_gt_info.json   frame -> [{bbox_obj, bbox_visib ([xmin, ymin, xmax - xmin, ymax - ymin], or four times -1 when empty),
                                    px_count_all, px_count_valid (= px_count_all), px_count_visib, visib_fract}]
    scene_object.json    frame -> {name: gt_index}     (only when names are given)

Every number comes from the device: the pixel counts, extents and masks are tp_scene_annotate's (SceneBounds.annotate), the image bytes
tp_view_images' (ops.view_images).  The writer only encodes files.  Rules, units and what is pinned to what: DESIGN.md, "Novel views as
a BOP scene".
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch

from ._lib import SCENE_INFO_FIELDS as INFO_FIELDS          # the columns ops.SCENE_INFO_KEYS names


def _host(x) -> np.ndarray:
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _bbox(xmin: int, ymin: int, xmax: int, ymax: int) -> List[int]:
    """[x, y, w, h] with w = xmax - xmin and h = ymax - ymin (the BOP toolkit's calc_2d_bbox), four times -1 for an empty set."""
    if xmax < 0:
        return [-1, -1, -1, -1]
    return [int(xmin), int(ymin), int(xmax - xmin), int(ymax - ymin)]


def gt_info_entry(row: Sequence[int]) -> dict:
    """One scene_gt_info.json entry from one row of ``info`` (ops.SCENE_INFO_KEYS order)."""
    n_all, n_vis = int(row[0]), int(row[1])
    return dict(bbox_obj=_bbox(*(int(v) for v in row[2:6])), bbox_visib=_bbox(*(int(v) for v in row[6:10])), px_count_all=n_all,
                px_count_valid=n_all, px_count_visib=n_vis, visib_fract=(n_vis / n_all if n_all > 0 else 0.0))


class BopSceneWriter:
    """``root``: the scene folder (created).  ``intr`` [3,3]: the camera of every view.  ``depth_scale_opt``: options nerf.depth.scale
    (NeRF units per metre; poses come in those units).  ``png_per_metre``: depth PNG units per metre.  ``names``: {object id: model
    name} -> scene_object.json.  Frames are numbered from ``first_frame`` in the order they are added."""

    def __init__(self, root: str, intr, depth_scale_opt: float, png_per_metre: float = 2000, names: Optional[Mapping[int, str]] = None,
                 first_frame: int = 0):
        self.root = str(root)
        self.cam_K = [float(v) for v in _host(intr).astype(np.float32).reshape(9)]
        self.depth_scale_opt, self.png_per_metre = float(depth_scale_opt), float(png_per_metre)
        self.names = None if names is None else {int(k): str(v) for k, v in names.items()}
        self.next_frame = int(first_frame)
        self.camera: Dict[str, dict] = {}
        self.gt: Dict[str, list] = {}
        self.gt_info: Dict[str, list] = {}
        self.objects: Dict[str, dict] = {}
        for sub in ("rgb", "depth", "mask", "mask_visib"):
            os.makedirs(os.path.join(self.root, sub), exist_ok=True)

    def add_views(self, pose, object_ids, info, mask, mask_visib, rgb8, depth16, cam_w2c=None) -> List[int]:
        """pose [B,3,4] (t in NeRF units), object_ids [K] in blend order, info [B,K,10] int32, mask / mask_visib [B,K,H,W] uint8,
        rgb8 [B,H,W,3] uint8, depth16 [B,H,W] uint16; device tensors or host arrays.  ``cam_w2c`` [B,3,4] (world -> camera, t in mm):
        each frame's camera pose, written as BOP's cam_R_w2c / cam_t_w2c into scene_camera.json (None: the keys are not written).
        Returns the frame numbers written."""
        from PIL import Image
        pose = torch.as_tensor(pose, dtype=torch.float32) if not torch.is_tensor(pose) else pose.detach().float()
        if pose.dim() == 2:
            pose = pose[None]
        # metres x depth.scale -> mm with the expression and on the device SceneBounds.rasterise uses: the scene's poses are bit for
        # bit the poses the masks were rasterised at
        t_mm = _host((pose[:, :, 3] / self.depth_scale_opt) * 1000).astype(np.float32)
        rot = _host(pose[:, :, :3]).astype(np.float32)
        ids = [int(v) for v in _host(object_ids).reshape(-1)]
        info, mask, mask_visib, rgb8, depth16 = (_host(x) for x in (info, mask, mask_visib, rgb8, depth16))
        B, K = rot.shape[0], len(ids)
        H, W = rgb8.shape[1:3]
        if cam_w2c is not None:
            cam_w2c = _host(cam_w2c).astype(np.float64)
            if cam_w2c.shape != (B, 3, 4):
                raise ValueError("BopSceneWriter.add_views: cam_w2c [B=%d,3,4] expected, got %s" % (B, cam_w2c.shape))
        if info.shape != (B, K, INFO_FIELDS) or mask.shape != (B, K, H, W) or mask_visib.shape != (B, K, H, W) or \
                rgb8.shape != (B, H, W, 3) or depth16.shape != (B, H, W):
            raise ValueError("BopSceneWriter.add_views: shapes do not agree (B %d, K %d, H %d, W %d)" % (B, K, H, W))
        if mask.dtype != np.uint8 or mask_visib.dtype != np.uint8 or rgb8.dtype != np.uint8 or depth16.dtype != np.uint16:
            raise ValueError("BopSceneWriter.add_views: uint8 masks and rgb8, uint16 depth16 expected")
        if self.names is not None and any(k not in self.names for k in ids):
            raise ValueError("BopSceneWriter.add_views: an object id without a name")
        frames = []
        for b in range(B):
            frame = self.next_frame
            self.next_frame += 1
            key = str(frame)
            Image.fromarray(np.ascontiguousarray(rgb8[b]), "RGB").save(os.path.join(self.root, "rgb", "%06d.png" % frame))
            Image.fromarray(np.ascontiguousarray(depth16[b])).save(os.path.join(self.root, "depth", "%06d.png" % frame))
            for k in range(K):
                Image.fromarray(np.ascontiguousarray(mask[b, k]), "L").save(os.path.join(self.root, "mask", "%06d_%06d.png" % (frame, k)))
                Image.fromarray(np.ascontiguousarray(mask_visib[b, k]), "L").save(os.path.join(self.root, "mask_visib", "%06d_%06d.png" % (frame, k)))
            self.camera[key] = dict(cam_K=self.cam_K, depth_scale=1000.0 / self.png_per_metre)
            if cam_w2c is not None:
                self.camera[key].update(cam_R_w2c=[float(v) for v in cam_w2c[b, :, :3].reshape(9)], cam_t_w2c=[float(v) for v in cam_w2c[b, :, 3]])
            # the meshes share the scene frame: every object of a view carries the view's pose
            self.gt[key] = [dict(obj_id=ids[k], cam_R_m2c=[float(v) for v in rot[b].reshape(9)], cam_t_m2c=[float(v) for v in t_mm[b]])
                            for k in range(K)]
            self.gt_info[key] = [gt_info_entry(info[b, k]) for k in range(K)]
            if self.names is not None:
                self.objects[key] = {self.names[ids[k]]: k for k in range(K)}
            frames.append(frame)
        return frames

    def close(self) -> None:
        files = dict(scene_camera=self.camera, scene_gt=self.gt, scene_gt_info=self.gt_info)
        if self.names is not None:
            files["scene_object"] = self.objects
        for name, content in files.items():
            with open(os.path.join(self.root, name + ".json"), "w") as f:
                json.dump(content, f, indent=1)


def read_bop_frame(root: str, frame: int) -> dict:
    """The host decode of one frame of a scene folder: cam_K [3,3] float32, depth_scale, obj_id [K], cam_R_m2c [K,3,3] and cam_t_m2c
    [K,3] float32 (mm), info (the scene_gt_info.json entries), rgb [H,W,3] uint8, depth [H,W] uint16, mask / mask_visib [K,H,W] uint8,
    objects ({name: gt_index}, or None without scene_object.json)."""
    from PIL import Image
    load = lambda name: json.load(open(os.path.join(root, name + ".json")))
    key = str(int(frame))
    cam, info = load("scene_camera")[key], load("scene_gt_info")[key]
    poses = read_bop_poses(root)[int(frame)]                # the one reader of the pose fields (float64 there, float32 here)
    png = lambda sub, name: np.asarray(Image.open(os.path.join(root, sub, name)))
    K = len(poses["obj_id"])
    out = dict(cam_K=poses["cam_K"].astype(np.float32), depth_scale=float(cam["depth_scale"]), obj_id=poses["obj_id"],
               cam_R_m2c=poses["cam_R_m2c"].astype(np.float32), cam_t_m2c=poses["cam_t_m2c"].astype(np.float32), info=info,
               rgb=png("rgb", "%06d.png" % frame), depth=png("depth", "%06d.png" % frame),
               mask=np.stack([png("mask", "%06d_%06d.png" % (frame, k)) for k in range(K)]),
               mask_visib=np.stack([png("mask_visib", "%06d_%06d.png" % (frame, k)) for k in range(K)]), objects=None)
    if os.path.exists(os.path.join(root, "scene_object.json")):
        out["objects"] = load("scene_object")[key]
    return out


def read_bop_poses(root: str, camera: bool = True) -> Dict[int, dict]:
    """The poses of a scene folder from its json files alone (no image is opened): frame -> obj_id [K] int64, cam_R_m2c [K,3,3],
    cam_t_m2c [K,3] float64 (mm) in the order of scene_gt.json and, with ``camera``, cam_K [3,3] float64 from scene_camera.json."""
    load = lambda name: json.load(open(os.path.join(root, name + ".json")))
    gt = load("scene_gt")
    cam = load("scene_camera") if camera else None
    out = {}
    for key, entries in gt.items():
        K = len(entries)
        out[int(key)] = dict(obj_id=np.array([g["obj_id"] for g in entries], dtype=np.int64),
                             cam_R_m2c=np.array([g["cam_R_m2c"] for g in entries], dtype=np.float64).reshape(K, 3, 3),
                             cam_t_m2c=np.array([g["cam_t_m2c"] for g in entries], dtype=np.float64).reshape(K, 3))
        if camera:
            out[int(key)]["cam_K"] = np.array(cam[key]["cam_K"], dtype=np.float64).reshape(3, 3)
    return out


def verify_bop_scene(root: str) -> int:
    """Read every frame back and check the files against each other: image sizes and types, masks of 0 / 255 only, the visible mask
    inside the full one, and the counts, boxes and fractions of scene_gt_info.json recomputed from the mask files.  Returns the number
    of frames; raises ValueError at the first disagreement."""
    frames = sorted(int(k) for k in json.load(open(os.path.join(root, "scene_gt.json"))))

    def fail(frame, what):
        raise ValueError("%s, frame %d: %s" % (root, frame, what))

    for frame in frames:
        fr = read_bop_frame(root, frame)
        H, W = fr["depth"].shape
        if fr["rgb"].shape != (H, W, 3) or fr["rgb"].dtype != np.uint8 or fr["depth"].dtype != np.uint16:
            fail(frame, "rgb must be 8-bit RGB and depth 16-bit, of one size")
        if len(fr["info"]) != len(fr["obj_id"]) or fr["mask"].shape != (len(fr["obj_id"]), H, W) or fr["mask_visib"].shape != fr["mask"].shape:
            fail(frame, "scene_gt.json, scene_gt_info.json and the mask files disagree on the objects")
        for k, entry in enumerate(fr["info"]):
            full, vis = fr["mask"][k], fr["mask_visib"][k]
            if not np.isin(full, (0, 255)).all() or not np.isin(vis, (0, 255)).all() or (vis > full).any():
                fail(frame, "object %d: masks must be 0 / 255 and the visible mask must lie inside the full one" % k)
            row = [int((full > 0).sum()), int((vis > 0).sum())]
            for m in (full > 0, vis > 0):
                ys, xs = np.nonzero(m)
                row += [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())] if xs.size else [-1] * 4
            if gt_info_entry(row) != entry:
                fail(frame, "object %d: scene_gt_info.json says %r, the masks give %r" % (k, entry, gt_info_entry(row)))
        if fr["objects"] is not None and sorted(fr["objects"].values()) != list(range(len(fr["obj_id"]))):
            fail(frame, "scene_object.json must name every gt entry once")
    return len(frames)
