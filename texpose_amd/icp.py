"""Pose refinement against measured depth: batched projective point-to-plane ICP on the device (K29).

The step between "PnP gave a pose" (texpose_amd.pnp) and "score it" (texpose_amd.pose_error): the mesh is rendered at the current
poses by the HIP rasteriser, every covered pixel with a measurement within ``tau_mm`` along its ray gives one point-to-plane residual
against the face's own normal, and one damped Gauss-Newton step in fp64 moves the pose (``ops.depth_icp_step``; ``ops.depth_icp`` is
the loop).  ``DepthRefiner`` keeps the mesh and the workspace of a batch size.  ``step_torch`` says the step again in plain torch ops
in fp64: the comparator of tools/icp_bench.py, and the one piece that also runs without a GPU.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _gn_torch, ops
from ._gn_torch import MIN_COUNT, PIVOT_TOL  # noqa: F401  (the header's constants, under the names callers know)
from ._refiner import _MeshRefiner
from .options import AttrDict

Tensor = torch.Tensor


def step_torch(verts: Tensor, faces: Tensor, zbuf: Tensor, face: Tensor, pose: Tensor, intr: Tensor, depth: Tensor, tau_mm: float,
               damping: float = 1e-6, frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, evaluate_only: bool = False) -> Dict[str, Tensor]:
    """ops.depth_icp_step's rules (include/texpose_amd.h, K29) in plain torch ops in fp64 on the tensors' device: the same arguments ->
    'pose' [B,3,4] float32, 'inliers' [B] int32, 'rms' [B] float32, 'status' [B] int32.  The sums run in torch's order, not the
    kernel's: counts and statuses agree, the rest to rounding."""
    JtJ, Jtr, cost, count, pose32 = sums_torch(verts, faces, zbuf, face, pose, intr, depth, tau_mm, frame, mask)
    return _gn_torch.solve(JtJ, Jtr, cost, count, pose32, damping, evaluate_only)


def sums_torch(verts: Tensor, faces: Tensor, zbuf: Tensor, face: Tensor, pose: Tensor, intr: Tensor, depth: Tensor, tau_mm: float,
               frame: Optional[Tensor] = None, mask: Optional[Tensor] = None):
    """The sums of step_torch before the solve (what joint.step_torch weights and adds) -> (JtJ [B,6,6], Jtr [B,6], cost [B] fp64,
    count [B], pose32 [B,3,4])."""
    f64 = torch.float64
    B, H, W, pose32, intr, depth, fr, tau, zf = _gn_torch.sums_head(zbuf, pose, intr, depth, 0, frame, "depth must hold 1 or B = %d planes", tau_mm)
    V, F = verts.shape[0], faces.shape[0]
    verts64, faces = verts.float().to(f64), faces.long()
    d_all = depth[fr]                                                                       # [B,H,W]
    cand = _gn_torch.masked((zf > 0) & torch.isfinite(zf) & (d_all > 0) & torch.isfinite(d_all) & (face >= 0) & (face < F), mask, fr)
    bi, ii, ji = torch.nonzero(cand, as_tuple=True)
    tri = faces[face[bi, ii, ji].long()]                                                    # [n,3]
    good = ((tri >= 0) & (tri < V)).all(-1)
    bi, ii, ji, tri = bi[good], ii[good], ji[good], tri[good]
    z, d = zf[bi, ii, ji].to(f64), d_all[bi, ii, ji].to(f64)
    K = intr.to(f64)
    rx = ((ji.to(f64) + 0.5) - K[bi, 0, 2]) / K[bi, 0, 0]
    ry = ((ii.to(f64) + 0.5) - K[bi, 1, 2]) / K[bi, 1, 1]
    q = (rx * rx + ry * ry) + 1.0
    dz = d - z
    v0, v1, v2 = verts64[tri[:, 0]], verts64[tri[:, 1]], verts64[tri[:, 2]]
    c = torch.cross(v1 - v0, v2 - v0, dim=-1)
    R = pose32[:, :, :3].to(f64)[bi]                                                        # [n,3,3]
    mvec = (R[:, :, 0] * c[:, None, 0] + R[:, :, 1] * c[:, None, 1]) + R[:, :, 2] * c[:, None, 2]
    mm = (mvec[:, 0] * mvec[:, 0] + mvec[:, 1] * mvec[:, 1]) + mvec[:, 2] * mvec[:, 2]
    keep = ((dz * dz) * q <= tau * tau) & torch.isfinite(mm) & (mm > 0)
    bi, rx, ry, z, d, mvec, mm = bi[keep], rx[keep], ry[keep], z[keep], d[keep], mvec[keep], mm[keep]
    n = mvec * (1.0 / torch.sqrt(mm))[:, None]
    flip = (n[:, 0] * rx + n[:, 1] * ry) + n[:, 2] > 0
    n = torch.where(flip[:, None], -n, n)
    ray = torch.stack([rx, ry, torch.ones_like(rx)], -1)
    P, Q = ray * z[:, None], ray * d[:, None]
    r = (n * (P - Q)).sum(-1)
    J = torch.cat([torch.cross(P, n, dim=-1), n], -1)                                       # [n,6]
    return _gn_torch.normal_sums(B, bi, J, r) + (torch.bincount(bi, minlength=B), pose32)


class DepthRefiner(_MeshRefiner):
    """Depth ICP for batches of poses of one mesh at H x W with the mesh on the device and a workspace per batch size.

    ``tau_mm`` (one value or ``iters`` + 1 for a coarse-to-fine schedule; 20.0), ``iters`` (Gauss-Newton steps, 5), ``damping``
    (relative, 1e-6).  ``refine`` returns pose [B,3,4] ([R|t] model -> camera, mm), inliers [B] (pixels within tau of the
    measurement), rms [B] (mm, point-to-plane), status [B] (0 ok, 1 fewer than 6 kept pixels, 3 the last step's system was not
    positive definite: the pose went through unchanged) and inliers0 / rms0 of the start pose.  ``cull``: render with the culled
    rasteriser (ops.mesh_raster(cull=True)), same bits."""
    _new_workspace = staticmethod(ops.depth_icp_workspace)

    def __init__(self, verts: Tensor, faces: Tensor, H: int, W: int, device="cuda:0", *, tau_mm=20.0, iters: int = 5, damping: float = 1e-6,
                 cull: bool = False):
        super().__init__(verts, faces, H, W, device, cull=cull)
        self.tau_mm, self.iters, self.damping = tau_mm, int(iters), float(damping)

    def refine(self, pose: Tensor, intr: Tensor, depth: Tensor, frame: Optional[Tensor] = None, mask: Optional[Tensor] = None) -> AttrDict:
        """pose [B,3,4], intr [B,3,3] or [3,3], depth [Ft,H,W] (mm; 0: no measurement), frame [B] int32 (the plane of each pose; without
        it Ft is 1 or B), mask [Ft,H,W] uint8 / bool (0: do not use the pixel)."""
        depth = depth if depth.dim() == 3 else depth[None]
        if tuple(depth.shape[1:]) != (self.H, self.W):
            raise ValueError("DepthRefiner.refine: depth planes of %d x %d expected, got %s" % (self.H, self.W, tuple(depth.shape)))
        return AttrDict(ops.depth_icp(self.verts, self.faces, pose, intr, depth, tau_mm=self.tau_mm, iters=self.iters, damping=self.damping,
                                      frame=frame, mask=mask, workspace=self._workspace(pose.shape[0]), cull=self.cull))
