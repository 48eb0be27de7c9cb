"""Poses from dense 2D-3D correspondence maps: batched PnP with RANSAC on the device (K28).

The pose estimators this project's texture-learning loop feeds (GDR-Net, Self6D++) predict a NOCS / model-coordinate image and a
mask; a pose comes out of that map by PnP with RANSAC.  ``PnPSolver`` does that step for a batch of images with the project's
kernels: ``ops.corr_from_nocs`` (map -> correspondence list), ``ops.pnp_hypotheses`` (minimal samples, P3P), ``ops.pnp_score`` (inlier
counts of every hypothesis) and ``ops.pnp_refine`` (selection and Gauss-Newton).  ``score_torch`` says the scoring rule again in plain
torch ops: the comparator of tools/pnp_bench.py, and the one piece that also runs without a GPU.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops
from .options import AttrDict

Tensor = torch.Tensor


def score_torch(xy: Tensor, xyz: Tensor, count: Tensor, intr: Tensor, poses: Tensor, tau_px: float = 2.0, valid: Optional[Tensor] = None,
                chunk: int = 16) -> Tensor:
    """ops.pnp_score's rule (include/texpose_amd.h, K28) in plain torch ops in fp32 on the tensors' device, ``chunk`` hypotheses at a
    time: xy [B,N,2], xyz [B,N,3], count [B], intr [B,3,3] or [3,3], poses [B,T,12] or [B,T,3,4] -> inliers [B,T] int32."""
    xy, xyz, poses = xy.float(), xyz.float(), poses.float()
    B, N = xy.shape[:2]
    poses = poses.reshape(B, -1, 12)
    T = poses.shape[1]
    intr = intr.float()
    if intr.dim() == 2:
        intr = intr[None].expand(B, 3, 3)
    n = count.to(torch.int64).clamp(0, N)
    live = (torch.arange(N, device=xy.device)[None] < n[:, None])[:, None]                  # [B,1,N]
    u, v = xy[:, None, :, 0], xy[:, None, :, 1]
    X, Y, Z = xyz[:, None, :, 0], xyz[:, None, :, 1], xyz[:, None, :, 2]
    fx, fy, cx, cy = (intr[:, i, j][:, None, None] for i, j in ((0, 0), (1, 1), (0, 2), (1, 2)))
    tau2 = torch.tensor(tau_px, dtype=torch.float32, device=xy.device) ** 2
    out = torch.zeros(B, T, dtype=torch.int32, device=xy.device)
    for h0 in range(0, T, chunk):
        P = poses[:, h0:h0 + chunk, :, None]                                               # [B,c,12,1]
        x = ((P[:, :, 0] * X + P[:, :, 1] * Y) + P[:, :, 2] * Z) + P[:, :, 3]
        y = ((P[:, :, 4] * X + P[:, :, 5] * Y) + P[:, :, 6] * Z) + P[:, :, 7]
        z = ((P[:, :, 8] * X + P[:, :, 9] * Y) + P[:, :, 10] * Z) + P[:, :, 11]
        du = ((fx * x) / z + cx) - u
        dv = ((fy * y) / z + cy) - v
        ok = live & (z > 0) & torch.isfinite(z) & (du * du + dv * dv <= tau2)
        out[:, h0:h0 + chunk] = ok.sum(-1).to(torch.int32)
    if valid is not None:
        out = torch.where(valid.to(out.device) != 0, out, torch.zeros_like(out))
    return out


class PnPSolver:
    """PnP-RANSAC for batches of H x W correspondence maps (or ready correspondence lists) with preallocated buffers.

    ``defaults``: T (hypotheses per image, 256), tau_px (inlier threshold, 2.0), iters (Gauss-Newton steps, 5), seed (0).  The buffers
    of a batch size (workspace, correspondence lists, hypotheses, outputs) are allocated at its first use and reused.  A solve still makes
    two small tensors, n and score [B], and an expanded copy of a [3,3] intr; under torch.cuda.graph these come from the graph's pool.
    Both routes return pose [B,3,4] ([R|t] model -> camera, mm), inliers [B], n [B] (usable correspondences), rms [B] (px over the
    inliers), status [B] (0 ok, 1 fewer than 4 correspondences, 2 no valid hypothesis, 3 refinement stopped at a system that was not
    positive definite) and score = inliers / max(n, 1).  The tensors belong to the solver: the next solve overwrites them."""

    def __init__(self, H: int, W: int, device="cuda:0", *, T: int = 256, tau_px: float = 2.0, iters: int = 5, seed: int = 0):
        self.H, self.W, self.device = int(H), int(W), torch.device(device)
        if self.device.type != "cuda":
            raise ops._lib.TexposeLibraryError("PnPSolver runs the HIP kernels: a GPU device is needed (score_torch alone has a CPU route)")
        self.T, self.tau_px, self.iters, self.seed = int(T), float(tau_px), int(iters), int(seed)
        self._buffers: Dict[tuple, dict] = {}

    def _for(self, B: int, N: int) -> dict:
        key = (B, N)
        if key not in self._buffers:
            dev, T = self.device, self.T
            i32 = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
            self._buffers[key] = dict(
                workspace=ops.pnp_workspace(B, N, T, dev),
                corr=dict(xy=torch.zeros(B, N, 2, device=dev), xyz=torch.zeros(B, N, 3, device=dev), count=i32(B)),
                out=dict(pose=torch.empty(B, 3, 4, device=dev), inliers=i32(B), rms=torch.empty(B, device=dev), status=i32(B),
                         sample_idx=i32(B, T, 4), hyp=torch.empty(B, T, 12, device=dev), hyp_valid=torch.empty(B, T, device=dev, dtype=torch.uint8),
                         hyp_inliers=i32(B, T)))
        return self._buffers[key]

    def _result(self, r: dict, count: Tensor, N: int) -> AttrDict:
        n = count.clamp(0, N)
        return AttrDict(pose=r["pose"], inliers=r["inliers"], n=n, rms=r["rms"], status=r["status"],
                        score=r["inliers"].float() / n.clamp(min=1).float())

    def solve(self, xy: Tensor, xyz: Tensor, count: Tensor, intr: Tensor) -> AttrDict:
        """xy [B,N,2] (pixel centres at (j + 0.5, r + 0.5)), xyz [B,N,3] (mm), count [B] int32, intr [B,3,3] or [3,3]."""
        B, N = xy.shape[:2]
        buf = self._for(B, N)
        r = ops.pnp_ransac(xy, xyz, count, intr, T=self.T, tau_px=self.tau_px, iters=self.iters, seed=self.seed, workspace=buf["workspace"],
                           out=buf["out"])
        return self._result(r, count, N)

    def solve_nocs(self, nocs: Tensor, mask: Tensor, intr: Tensor, centre, scale, stride: int = 1) -> AttrDict:
        """nocs [B,H,W,3] (or [B,3,H,W]) in [0, 1], mask [B,H,W] (non-zero: use the pixel), ``centre`` / ``scale`` as
        surfel.nocs_normalisation(verts) returns them, every ``stride``-th pixel of every ``stride``-th row."""
        if nocs.dim() == 4 and nocs.shape[1] == 3 and nocs.shape[3] != 3:
            nocs = nocs.permute(0, 2, 3, 1)
        if tuple(nocs.shape[1:3]) != (self.H, self.W):
            raise ValueError("PnPSolver.solve_nocs: maps of %d x %d expected, got %s" % (self.H, self.W, tuple(nocs.shape)))
        B = nocs.shape[0]
        N = -(-self.H // stride) * -(-self.W // stride)
        buf = self._for(B, N)
        c = ops.corr_from_nocs(nocs, mask, centre, scale, stride=stride, workspace=buf["workspace"], out=buf["corr"])
        return self.solve(c["xy"], c["xyz"], c["count"], intr)
