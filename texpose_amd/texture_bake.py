"""Bake rendered views of an object back onto its CAD mesh as vertex colours: the output form of a learned texture.

A trained field is a radiance field behind ``Graph.render_by_slices``; the project's rasteriser renders a vertex-coloured mesh three
orders of magnitude faster.  ``TextureBaker`` closes the gap: views with known poses (NeRF renders, or any images) are projected onto
the vertices by K27 (``ops.texture_bake``: visibility from the mesh's own depth plane with a bias derived from the vertex normal,
bilinear taps, weights cos x cover x opacity), ``fill_unseen`` colours what no view reached from its neighbours, and ``write_ply``
stores the result so that ``surfel.load_ply`` -- and ``SurfelRenderer``, ``SceneBounds``, the BOP writer -- read it back.
Rules, slice rule and what is pinned to what: include/texpose_amd.h (K27) and DESIGN.md section 17.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import ops
from .options import AttrDict

THRESHOLDS = dict(cos_min=0.3, cover_min=0.5, z_tol_mm=0.5, slope=2.0)


def vertex_normals(verts, faces) -> np.ndarray:
    """Area-weighted unit vertex normals [V,3] float32 on the host in fp64: the sum of the (unnormalised) cross products of the
    incident faces, in face order.  A vertex without a face of non-zero area gets (0, 0, 0), which no view passes."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, f[:, k], fn)                                   # (unbuffered and in index order: deterministic)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(length > 0, n / np.maximum(length, 1e-300), 0.0).astype(np.float32)


def sphere_view_poses(n: int, distance_mm: float) -> np.ndarray:
    """n look-at poses [n,3,4] float64 (model -> camera, OpenCV axes, t in mm: the rasteriser's convention) from a Fibonacci lattice
    on the sphere of radius ``distance_mm`` about the model origin: direction i has z = 1 - (2 i + 1) / n and azimuth i x the golden
    angle; the camera's optical axis passes through the origin and its x axis is horizontal (perpendicular to the model's z)."""
    if n < 1 or not distance_mm > 0:
        raise ValueError("sphere_view_poses: n >= 1 and distance_mm > 0 expected")
    golden = math.pi * (3.0 - math.sqrt(5.0))
    out = np.zeros((n, 3, 4))
    for i in range(n):
        z = 1.0 - (2 * i + 1) / n
        r = math.sqrt(max(0.0, 1.0 - z * z))
        d = np.array([r * math.cos(i * golden), r * math.sin(i * golden), z])      # from the origin towards the camera
        fwd = -d
        right = np.cross(fwd, np.array([0.0, 0.0, 1.0]))
        if np.linalg.norm(right) < 1e-9:
            right = np.array([1.0, 0.0, 0.0])
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])
        out[i, :, :3] = R
        out[i, :, 3] = -R @ (d * distance_mm)
    return out


def poses_to_nerf_units(pose_mm, depth_scale: float):
    """[R|t] with t in mm -> t in nerf.depth.scale units (t x depth_scale / 1000), the inverse of calibrate_pose's scaling."""
    pose_mm = torch.as_tensor(pose_mm)
    return torch.cat([pose_mm[..., :3], pose_mm[..., 3:] * float(depth_scale) / 1000.0], dim=-1)


def poses_to_mm(pose, depth_scale: float):
    """[R|t] with t in nerf.depth.scale units -> t in mm (t x 1000 / depth_scale, as calibrate_pose scales; the rotation as it is)."""
    pose = torch.as_tensor(pose)
    return torch.cat([pose[..., :3], pose[..., 3:] * 1000.0 / float(depth_scale)], dim=-1)


def mesh_edges(faces) -> np.ndarray:
    """The undirected edges [E,2] of a triangle mesh, each once, sorted."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    e = np.sort(e[e[:, 0] != e[:, 1]], axis=1)
    return np.unique(e, axis=0)


def fill_unseen(vcolor, seen, faces) -> Tuple[np.ndarray, np.ndarray, int]:
    """Vertices no view reached take the mean of their already-coloured edge neighbours, swept (every sweep reads the colours of the
    sweep before) until none is left or nothing changes.  Host, fp64, deterministic.  -> (vcolor [V,3] float32, coloured [V] bool,
    number of vertices filled).  A component without a seen vertex stays as it was and is not coloured."""
    col = np.asarray(vcolor, dtype=np.float64).copy()
    done = np.asarray(seen, dtype=bool).copy()
    e = mesh_edges(faces)
    src, dst = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    filled = 0
    while not done.all():
        use = done[src] & ~done[dst]
        if not use.any():
            break
        total, n = np.zeros_like(col), np.zeros(len(col))
        np.add.at(total, dst[use], col[src[use]])
        np.add.at(n, dst[use], 1.0)
        new = n > 0
        col[new] = total[new] / n[new, None]
        done |= new
        filled += int(new.sum())
    return col.astype(np.float32), done, filled


def write_ply(path: str, verts, faces, vcolor) -> None:
    """Binary little-endian PLY: float x y z, uchar red green blue (round(255 c) of the colours clamped to [0, 1]), triangle faces as
    `list uchar int vertex_indices` -- what surfel.load_ply and BOP tools read."""
    v = np.asarray(verts, dtype="<f4").reshape(-1, 3)
    f = np.asarray(faces, dtype="<i4").reshape(-1, 3)
    c = np.rint(np.clip(np.nan_to_num(np.asarray(vcolor, dtype=np.float64).reshape(-1, 3)), 0.0, 1.0) * 255.0).astype(np.uint8)
    if len(c) != len(v):
        raise ValueError("write_ply: %d colours for %d vertices" % (len(c), len(v)))
    vert = np.empty(len(v), dtype=[("p", "<f4", 3), ("c", "u1", 3)])
    vert["p"], vert["c"] = v, c
    face = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", 3)])
    face["n"], face["i"] = 3, f
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
              "property list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


def bake_torch(verts: Tensor, normals: Tensor, pose: Tensor, intr: Tensor, rgb: Tensor, zbuf: Tensor, weight: Optional[Tensor] = None, *,
               cos_min: float = 0.3, cover_min: float = 0.5, z_tol_mm: float = 0.5, slope: float = 2.0) -> Dict[str, Tensor]:
    """ops.texture_bake's rules (include/texpose_amd.h, K27) in plain torch ops in fp64 on the tensors' device, all views in one
    sum -> {'acc' [V,4] float32, 'count' [V] int32, 'reached': the number of pairs that got as far as their taps}.  What the kernel
    is timed against (tools/texture_bake_bench.py)."""
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))     # (the kernel takes the scalars as fp32)
    cos_min, cover_min, z_tol_mm, slope = f32(cos_min), f32(cover_min), f32(z_tol_mm), f32(slope)
    B, H, W = zbuf.shape
    dev = verts.device
    P, K, v, n = pose.double(), intr.double(), verts.double(), normals.double()
    if K.dim() == 2:
        K = K[None].expand(B, 3, 3)
    x = torch.einsum("bij,vj->bvi", P[:, :, :3], v) + P[:, None, :, 3]                  # [B,V,3]
    z = x[..., 2]
    c = -(torch.einsum("bij,vj->bvi", P[:, :, :3], n) * x).sum(-1) / x.norm(dim=-1)
    q = torch.einsum("bij,bvj->bvi", K, x)
    su, sv = q[..., 0] / q[..., 2] - 0.5, q[..., 1] / q[..., 2] - 0.5
    ok = (z > 0) & (c >= cos_min) & (su >= -1) & (su < W) & (sv >= -1) & (sv < H)
    su, sv = torch.where(ok, su, torch.zeros_like(su)), torch.where(ok, sv, torch.zeros_like(sv))
    cs = torch.where(ok, c, torch.ones_like(c))
    fj, fr = su.floor(), sv.floor()
    al, be = su - fj, sv - fr
    fmin = torch.minimum(K[:, 0, 0], K[:, 1, 1])[:, None]
    tol = z_tol_mm + slope * (z / fmin) * (1 - cs * cs).clamp(min=0).sqrt() / cs
    base = torch.arange(B, device=dev)[:, None] * (H * W)
    zb, im = zbuf.reshape(-1), rgb.reshape(-1, 3)
    wp = None if weight is None else weight.reshape(-1)
    cover = torch.zeros_like(z)
    cw = torch.zeros_like(z)
    col = torch.zeros(z.shape + (3,), dtype=torch.float64, device=dev)
    for dr in (0, 1):
        for dj in (0, 1):
            r, j = fr.long() + dr, fj.long() + dj
            inside = ok & (r >= 0) & (r < H) & (j >= 0) & (j < W)
            o = base + r.clamp(0, H - 1) * W + j.clamp(0, W - 1)
            zt, px = zb[o], im[o]
            valid = inside & (zt > 0) & ((zt.double() - z).abs() <= tol) & torch.isfinite(px).all(-1)
            pw = torch.ones_like(z) if wp is None else wp[o].double()
            if wp is not None:
                valid = valid & torch.isfinite(pw)
            w = torch.where(valid, (al if dj else 1 - al) * (be if dr else 1 - be), torch.zeros_like(z))
            cover = cover + w
            col = col + w[..., None] * torch.where(valid[..., None], px.double(), torch.zeros_like(col))
            cw = cw + w * torch.where(valid, pw, torch.zeros_like(pw))
    take = ok & (cover >= cover_min)
    safe = torch.where(take, cover, torch.ones_like(cover))
    wb = cs * cover
    if wp is not None:
        wb = wb * (cw / safe)
    wb = torch.where(take, wb, torch.zeros_like(wb))
    acc = torch.cat([(wb[..., None] * (col / safe[..., None])).sum(0), wb.sum(0)[:, None]], dim=1)
    return dict(acc=acc.float(), count=take.sum(0).to(torch.int32), reached=ok.sum())


class TextureBaker:
    """Accumulates views of one mesh into vertex colours.  ``verts`` [V,3] (mm) and ``faces`` [F,3] as load_ply returns them; every view
    is H x W; ``thresholds``: cos_min, cover_min, z_tol_mm, slope of K27.  The normals are made once on the host (vertex_normals); the
    accumulators and the workspace live on the device and no call reads anything back before ``result``."""

    def __init__(self, verts, faces, H: int, W: int, device="cuda:0", **thresholds):
        unknown = set(thresholds) - set(THRESHOLDS)
        if unknown:
            raise TypeError("TextureBaker: unknown thresholds %s" % sorted(unknown))
        self.thresholds = {**THRESHOLDS, **thresholds}
        self.device = torch.device(device)
        self.H, self.W = int(H), int(W)
        self.verts_host = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
        self.faces_host = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
        self.verts = torch.from_numpy(self.verts_host).to(self.device)
        self.faces = torch.from_numpy(self.faces_host).to(self.device)
        self.normals = torch.from_numpy(vertex_normals(self.verts_host, self.faces_host)).to(self.device)
        V = self.verts.shape[0]
        self.acc = torch.zeros(V, 4, device=self.device)
        self.count = torch.zeros(V, device=self.device, dtype=torch.int32)
        self.views = 0
        self._workspaces: Dict[int, Tensor] = {}

    def reset(self) -> None:
        self.acc.zero_()
        self.count.zero_()
        self.views = 0

    def add_views(self, rgb: Tensor, pose_mm: Tensor, intr: Tensor, zbuf: Optional[Tensor] = None, weight: Optional[Tensor] = None) -> None:
        """rgb [B,H,W,3] in [0,1], pose_mm [B,3,4] (model -> camera, t in mm), intr [B,3,3] or [3,3], zbuf [B,H,W] (the mesh's depth
        at these poses in mm; rasterised here when None), weight [B,H,W] (e.g. the field's opacity) or None."""
        pose_mm = torch.as_tensor(pose_mm, dtype=torch.float32).to(self.device).contiguous()
        intr = torch.as_tensor(intr, dtype=torch.float32).to(self.device)
        B = pose_mm.shape[0]
        rgb = torch.as_tensor(rgb, dtype=torch.float32).to(self.device).reshape(B, self.H, self.W, 3)
        if zbuf is None:
            zbuf = ops.mesh_raster(self.verts, self.faces, pose_mm, intr, H=self.H, W=self.W, face_ids=False, normals=False)["zbuf"]
        else:
            zbuf = torch.as_tensor(zbuf, dtype=torch.float32).to(self.device).reshape(B, self.H, self.W)
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32).to(self.device).reshape(B, self.H, self.W)
        ws = self._workspaces.get(B)
        if ws is None:
            ws = self._workspaces[B] = ops.texture_bake_workspace(self.verts.shape[0], B, self.device)
        ops.texture_bake(self.verts, self.normals, pose_mm, intr, rgb, zbuf, weight, acc=self.acc, count=self.count, clear=False,
                         workspace=ws, **self.thresholds)
        self.views += B

    def result(self, fill: bool = True) -> AttrDict:
        """vcolor [V,3] float32 in [0,1] (acc_rgb / acc_w where a view contributed weight, 0 elsewhere; with ``fill`` the rest from
        fill_unseen), weight [V] (the summed weights), count [V] int32, seen [V] bool -- tensors on the device -- and the numbers of
        filled and still uncoloured vertices.  Reads the accumulators back when ``fill`` is set."""
        w = self.acc[:, 3]
        seen = (self.count > 0) & (w > 0)
        vcolor = torch.where(seen[:, None], self.acc[:, :3] / torch.where(seen, w, torch.ones_like(w))[:, None],
                             torch.zeros_like(self.acc[:, :3])).clamp(0, 1)
        filled, coloured = 0, seen
        if fill and not bool(seen.all()):
            col, done, filled = fill_unseen(vcolor.cpu().numpy(), seen.cpu().numpy(), self.faces_host)
            vcolor, coloured = torch.from_numpy(col).to(self.device), torch.from_numpy(done).to(self.device)
        return AttrDict(vcolor=vcolor, weight=w.clone(), count=self.count.clone(), seen=seen, filled=int(filled),
                        unseen=int((~coloured).sum()))
