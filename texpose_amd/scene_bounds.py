"""Depth bounds, object labels and mesh depth of a multi-object scene at poses nobody photographed: what ``Graph.render_by_slices``
needs as ``depth_range`` / ``object_mask`` for a novel view, made on the device from the CAD meshes.

The reference builds these in its novel-view loop (model/nerf_pretrain.py:307-416): per object a slab test of the box against the
pixel rays and a depth render of the mesh, blended by z-buffer.  Here each object is rasterised once (tp_mesh_raster, depth only)
into one plane of a [K,B,H,W] stack and a single launch (tp_scene_bounds, K21) blends the stack.  Rules, units and what is pinned
to what: DESIGN.md, "Scene bounds for novel views".
"""
from __future__ import annotations

import math
from typing import Dict, Mapping, Sequence, Tuple

import torch

from . import _lib, ops
from .geometry import compose_poses, make_pose
from .options import AttrDict


def novel_view_poses_obj(pose_anchor: torch.Tensor, N: int = 10) -> torch.Tensor:
    """N poses that spin the object about its own z axis under the anchor camera (reference camera.py:394-402): angles
    (k - N/2) / N * pi/2 for k = 0 .. N-1, each rotation applied before ``pose_anchor`` [3,4].  Returns [N,3,4] on the CPU."""
    theta = torch.arange(-N / 2, N / 2) / N * 0.5 * math.pi
    c, s, zero, one = theta.cos(), theta.sin(), torch.zeros_like(theta), torch.ones_like(theta)
    R_z = torch.stack([torch.stack([c, -s, zero], dim=-1), torch.stack([s, c, zero], dim=-1), torch.stack([zero, zero, one], dim=-1)], dim=-2)
    return compose_poses(make_pose(R=R_z), pose_anchor.detach().cpu().float()[None])


def distinct_object_ids(ids) -> list:
    """The ids as a list of ints, after checking what the scene kernels take for granted: every id positive (0 labels the background)
    and no id twice (tp_scene_annotate tells the objects apart by their label)."""
    ids = [int(k) for k in ids]
    if not ids or min(ids) <= 0:
        raise ValueError("SceneBounds: object ids must be positive (0 labels the background)")
    if len(set(ids)) != len(ids):
        raise ValueError("SceneBounds: duplicate object ids %s" % sorted(k for k in set(ids) if ids.count(k) > 1))
    return ids


class SceneBounds:
    """``objects``: {object id (> 0): (SurfelRenderer, bb_min_mm, bb_max_mm)} in blend order (ties go to the earlier object; they only
    occur between backgrounds); every renderer renders H x W on one device.  ``depth_scale_opt``: options nerf.depth.scale (NeRF
    units per metre).  ``bg_range``: the range of uncovered pixels in NeRF units (nerf.depth.range * nerf.depth.scale).

    Calling it with (pose [B,3,4] in NeRF units, intr [B,3,3] or [3,3], source) returns
    ``depth_range`` = (z_near [B,HW,1], z_far [B,HW,1]), ``label`` [B,HW] int32, ``object_mask`` [B,HW] bool (label > 0) and
    ``depth`` [B,HW] (nearest mesh depth, NeRF units, 0 where uncovered) -- the arguments of
    ``Graph.render_by_slices(opt, pose, intr=, depth_range=, object_mask=)``.  The buffers are allocated once per (B, K) and
    overwritten by the next call with the same B: copy what has to outlive it."""

    def __init__(self, objects: Mapping[int, Tuple[object, Sequence[float], Sequence[float]]], H: int, W: int, depth_scale_opt: float,
                 bg_range: Tuple[float, float]):
        if not 1 <= len(objects) <= _lib.SCENE_MAX_OBJECTS:
            raise ValueError(f"SceneBounds: 1 .. {_lib.SCENE_MAX_OBJECTS} objects expected, not {len(objects)}")
        self.H, self.W, self.depth_scale = int(H), int(W), float(depth_scale_opt)
        self.bg_range = (float(bg_range[0]), float(bg_range[1]))
        self.object_ids = distinct_object_ids(objects)
        self.renderers = [objects[k][0] for k in objects]
        for r in self.renderers:
            if (r.H, r.W) != (self.H, self.W) or r.device != self.renderers[0].device:
                raise ValueError("SceneBounds: every renderer must render %d x %d on the same device" % (self.H, self.W))
        self.device = self.renderers[0].device
        # the box table as the reference forms it (nerf_pretrain.py:321-322): (bb_mm * depth.scale) / 1000 in fp32
        bb = torch.tensor([[list(map(float, objects[k][1])), list(map(float, objects[k][2]))] for k in objects], dtype=torch.float32)
        self.boxes = ((bb * self.depth_scale) / 1000).contiguous().to(self.device)
        self.ids = torch.tensor(self.object_ids, dtype=torch.int32, device=self.device)
        self._buffers: Dict[int, dict] = {}
        self._annotations: Dict[int, dict] = {}

    def _buffers_for(self, B: int) -> dict:
        buf = self._buffers.get(B)
        if buf is None:
            K, HW = len(self.renderers), self.H * self.W
            f32 = lambda *shape: torch.empty(*shape, device=self.device, dtype=torch.float32)
            buf = dict(zbuf=f32(K, B, self.H, self.W), mask=torch.empty(B, HW, device=self.device, dtype=torch.bool),
                       out=dict(z_near=f32(B, HW), z_far=f32(B, HW), label=torch.empty(B, HW, device=self.device, dtype=torch.int32),
                                depth=f32(B, HW)))
            self._buffers[B] = buf
        return buf

    def rasterise(self, pose: torch.Tensor, intr: torch.Tensor) -> torch.Tensor:
        """zbuf [K,B,H,W] (mm, -1 on background) of every object at ``pose`` (NeRF units), in the instance's buffer."""
        buf = self._buffers_for(pose.shape[0])
        # the rasteriser works in mm (nerf_pretrain.py:334-336): t / depth.scale * 1000, the rotation as it is
        pose_mm = torch.cat([pose[:, :, :3], (pose[:, :, 3:] / self.depth_scale) * 1000], dim=-1).contiguous()
        for k, r in enumerate(self.renderers):
            ops.mesh_raster(r.verts, r.faces, pose_mm, intr, H=self.H, W=self.W, face_ids=False, normals=False, zbuf_out=buf["zbuf"][k])
        return buf["zbuf"]

    def __call__(self, pose: torch.Tensor, intr: torch.Tensor, source: str = "box") -> AttrDict:
        pose = torch.as_tensor(pose, dtype=torch.float32).to(self.device)
        if pose.dim() == 2:
            pose = pose[None]
        pose = pose.contiguous()
        B = pose.shape[0]
        intr = torch.as_tensor(intr, dtype=torch.float32).to(self.device)
        if intr.dim() == 2:
            intr = intr[None].expand(B, 3, 3)
        intr = intr.contiguous()
        buf = self._buffers_for(B)
        zbuf = self.rasterise(pose, intr)
        out = ops.scene_bounds(zbuf, self.boxes, self.ids, depth_scale=self.depth_scale, bg_range=self.bg_range, source=source,
                               pose=pose, intr=intr, out=buf["out"])
        torch.gt(out["label"], 0, out=buf["mask"])
        return AttrDict(depth_range=(out["z_near"][..., None], out["z_far"][..., None]), label=out["label"], object_mask=buf["mask"],
                        depth=out["depth"], zbuf=zbuf)

    def annotate(self, sb: AttrDict, masks: bool = True) -> AttrDict:
        """The per-object annotations of the views a call returned (tp_scene_annotate, K22): ``info`` [B,K,10] int32 (columns
        ``ops.SCENE_INFO_KEYS``: pixel counts and inclusive extents of the full and of the visible silhouette, -1 where empty) and, with
        ``masks``, ``mask`` / ``mask_visib`` [B,K,H,W] uint8 (0 / 255), objects in blend order.  Needs ``sb.zbuf`` and ``sb.label`` as the
        call left them; the results live in buffers kept per (B, K) like the call's own."""
        K, B = sb.zbuf.shape[:2]
        buf = self._annotations.get(B)
        if buf is None:
            buf = dict(info=torch.empty(B, K, _lib.SCENE_INFO_FIELDS, device=self.device, dtype=torch.int32))
            self._annotations[B] = buf
        if masks and "mask" not in buf:
            for k in ("mask", "mask_visib"):
                buf[k] = torch.empty(B, K, self.H, self.W, device=self.device, dtype=torch.uint8)
        out = ops.scene_annotate(sb.zbuf, sb.label, self.ids, masks=masks, out=buf)
        return AttrDict(info=out["info"], mask=out.get("mask"), mask_visib=out.get("mask_visib"))
