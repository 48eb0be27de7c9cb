"""Pose refinement against a mask: the exact distance field of the mask and batched silhouette alignment on the device (K31; DESIGN
section 21).

The refiner for where there is neither a depth sensor (texpose_amd.icp) nor a coloured mesh (texpose_amd.photo_align): a textureless
mesh, a pose estimate and the object's measured mask.  ``ops.mask_sdf`` turns the masks into their exact signed Euclidean distance
fields (pixels, negative inside); the mesh is rendered at the current poses by the HIP rasteriser, every interior rim pixel of the
rendering within ``tau_px`` of the measured outline gives one residual, its distance to that outline, against the field's own
central-difference gradient, and one damped Gauss-Newton step in fp64 moves the pose (``ops.silhouette_align_step``;
``ops.silhouette_align`` is the loop).  ``SilhouetteRefiner`` keeps the mesh and the workspaces of a batch size.  ``step_torch`` and
``sdf_torch`` say the step and the field again in plain torch ops: the comparators of tools/silhouette_bench.py, and the pieces that
also run without a GPU.

What it does is close the outline.  On a shape with a symmetry the outline closes and the pose need not (a rotation about the
symmetry axis is invisible, and so, at a radius of some thirty pixels, is most of the depth).  It is the step before photo_align,
whose basin is about a pixel, not a replacement for it or for the depth ICP.

Occlusion (K31c, K32).  A VISIBLE mask cut by an occluder has a false edge, and the plain field of it pulls rim
pixels to that edge: the loop diverges.  Say which pixels were measured instead: ``ops.mask_sdf(mask, known=...)`` treats the rest
as neither set nor clear, so no distance is measured to them and the field is NaN on them, which the step already drops;
``SilhouetteRefiner.refine(..., known=...)`` does that and also returns the IoU over the known pixels.
``ops.mask_known_from_others`` makes the known planes of a frame from the fields of all its instance masks (unknown: within a band
of another instance; conservative, the contour between two touching instances is lost to both).  ``known_from_others_torch`` says
it again in torch.  With this the outline over the visible part closes; with less than about half of the object visible the pose
still need not follow.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _gn_torch, ops
from ._refiner import _MeshRefiner
from .options import AttrDict

Tensor = torch.Tensor


def sdf_torch(mask: Tensor, known: Optional[Tensor] = None) -> Tensor:
    """ops.mask_sdf's rules (include/texpose_amd.h, K31a and K31c) by brute force over all pixel pairs of a plane, for small planes:
    mask [F,H,W] or [H,W], non-zero: set, known of the same shape, zero: the pixel is neither set nor clear -> sdf float32 of the same
    shape on the mask's device, NaN on the unknown pixels."""
    m = mask if mask.dim() == 3 else mask[None]
    k = torch.ones_like(m, dtype=torch.bool) if known is None else (known if known.dim() == 3 else known[None]) != 0
    if k.shape != m.shape:
        raise ValueError("sdf_torch: known of mask's shape expected, got %s and %s" % (tuple(known.shape), tuple(mask.shape)))
    F, H, W = m.shape
    ii, jj = torch.meshgrid(torch.arange(H, device=m.device), torch.arange(W, device=m.device), indexing="ij")
    pts = torch.stack([ii.reshape(-1), jj.reshape(-1)], 1)                                  # [n,2] int64
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)                                 # [n,n]
    none2 = H * H + W * W
    out = torch.empty(F, H * W, dtype=torch.float32, device=m.device)
    for f in range(F):
        seen = k[f].reshape(-1)
        is_set, is_clear = (m[f].reshape(-1) != 0) & seen, (m[f].reshape(-1) == 0) & seen
        to_set = torch.where(is_set[None, :], d2, torch.full_like(d2, none2)).min(1).values
        to_clear = torch.where(is_clear[None, :], d2, torch.full_like(d2, none2)).min(1).values
        out[f] = torch.where(is_set, -(torch.sqrt(to_clear.float()) - 0.5), torch.sqrt(to_set.float()) - 0.5)
        out[f][~seen] = float("nan")
    return out.reshape(mask.shape)


def known_from_others_torch(sdf: Tensor, band_px: float) -> Tensor:
    """ops.mask_known_from_others' rule (include/texpose_amd.h, K32) in plain torch ops: sdf [N,H,W] float32, the fields of one
    frame's instance masks -> known [N,H,W] uint8, 0 where another instance has sdf <= band_px - 0.5 (fp32) at the pixel."""
    near = sdf.float() <= (torch.tensor(band_px, dtype=torch.float32) - torch.tensor(0.5, dtype=torch.float32)).to(sdf.device)
    others = near.sum(0, keepdim=True) - near.to(torch.int64)                                # the near instances besides n itself
    return (others == 0).to(torch.uint8)


def step_torch(zbuf: Tensor, pose: Tensor, intr: Tensor, sdf: Tensor, tau_px: float, damping: float = 1e-6,
               frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, evaluate_only: bool = False) -> Dict[str, Tensor]:
    """ops.silhouette_align_step's rules (include/texpose_amd.h, K31b) in plain torch ops in fp64 on the tensors' device: the same
    arguments -> 'pose' [B,3,4] float32, 'inliers' [B] int32, 'rms' [B] float32, 'status', 'inter', 'uni' [B] int32.  The sums run in
    torch's order, not the kernel's: the counts and statuses agree, the rest to rounding."""
    JtJ, Jtr, cost, count, pose32, inter, uni = sums_torch(zbuf, pose, intr, sdf, tau_px, frame, mask)
    res = _gn_torch.solve(JtJ, Jtr, cost, count, pose32, damping, evaluate_only)
    res.update(inter=inter, uni=uni)
    return res


def sums_torch(zbuf: Tensor, pose: Tensor, intr: Tensor, sdf: Tensor, tau_px: float, frame: Optional[Tensor] = None,
               mask: Optional[Tensor] = None):
    """The sums of step_torch before the solve (what joint.step_torch weights and adds) -> (JtJ [B,6,6], Jtr [B,6], cost [B] fp64,
    count [B], pose32 [B,3,4], inter, uni [B] int32)."""
    f64 = torch.float64
    B, H, W, pose32, intr, sdf, fr, tau, zf = _gn_torch.sums_head(zbuf, pose, intr, sdf, 0, frame, "sdf must hold 1 or B = %d planes", tau_px)
    cov = (zf > 0) & torch.isfinite(zf)
    field = sdf[fr]                                                                         # [B,H,W]
    inside = (field < 0) & torch.isfinite(field)
    inter, uni = (cov & inside).reshape(B, -1).sum(1), (cov | inside).reshape(B, -1).sum(1)
    cand = torch.zeros_like(cov)
    if H >= 3 and W >= 3:
        c = cov[:, 1:-1, 1:-1]
        all_four = cov[:, 1:-1, :-2] & cov[:, 1:-1, 2:] & cov[:, :-2, 1:-1] & cov[:, 2:, 1:-1]
        cand[:, 1:-1, 1:-1] = c & ~all_four
    bi, ii, ji = torch.nonzero(_gn_torch.masked(cand, mask, fr), as_tuple=True)             # (interior: ii -+ 1 and ji -+ 1 exist)
    d = field[bi, ii, ji].to(f64)
    lf, rt, up, dn = (field[bi, ii, ji - 1].to(f64), field[bi, ii, ji + 1].to(f64), field[bi, ii - 1, ji].to(f64),
                      field[bi, ii + 1, ji].to(f64))
    r = d + 0.5
    keep = torch.isfinite(torch.stack([d, lf, rt, up, dn], -1)).all(-1) & (r.abs() <= tau)
    bi, ii, ji, r, lf, rt, up, dn = bi[keep], ii[keep], ji[keep], r[keep], lf[keep], rt[keep], up[keep], dn[keep]
    J = _gn_torch.image_gradient_rows(zf, intr, bi, ii, ji, lf[:, None], rt[:, None], up[:, None], dn[:, None])          # [n,6]
    return _gn_torch.normal_sums(B, bi, J, r) + (torch.bincount(bi, minlength=B), pose32, inter.to(torch.int32), uni.to(torch.int32))


class SilhouetteRefiner(_MeshRefiner):
    """Silhouette alignment for batches of poses of one mesh at H x W with the mesh on the device and a workspace per batch size.

    ``tau_px`` (one value or ``iters`` + 1 for a coarse-to-fine schedule; 4 pixels), ``iters`` (Gauss-Newton steps, 10), ``damping``
    (relative, 1e-6).  ``refine`` returns pose [B,3,4] ([R|t] model -> camera, mm), inliers [B] (rim pixels of the rendering within
    tau_px of the measured outline), rms [B] (pixels), status [B] (0 ok, 1 fewer than 6 kept pixels, 3 the last step's system was not
    positive definite: the pose went through unchanged), inliers0 / rms0 of the start pose and iou / iou0 [B], the intersection over
    union of rendering and mask at the last and the start pose; with ``known`` also iou_visible / iou0_visible [B], the same over the
    known pixels only."""
    _new_workspace = staticmethod(ops.silhouette_align_workspace)

    def __init__(self, verts: Tensor, faces: Tensor, H: int, W: int, device="cuda:0", *, tau_px=4.0, iters: int = 10, damping: float = 1e-6,
                 cull: bool = False):
        super().__init__(verts, faces, H, W, device, cull=cull)
        self.tau_px, self.iters, self.damping = tau_px, int(iters), float(damping)

    def refine(self, pose: Tensor, intr: Tensor, mask_or_sdf: Tensor, frame: Optional[Tensor] = None, mask: Optional[Tensor] = None,
               known: Optional[Tensor] = None) -> AttrDict:
        """pose [B,3,4], intr [B,3,3] or [3,3], mask_or_sdf [Ft,H,W]: the measured masks (uint8 or bool; run through ops.mask_sdf
        first) or their distance fields (a float tensor, taken as it is), frame [B] int32 (the plane of each pose; without it Ft is 1
        or B), mask [Ft,H,W] uint8 / bool (0: do not use the pixel), known [Ft,H,W] uint8 / bool (0: the mask's value there is no
        measurement, the pixel is behind an occluder, say; ops.mask_known_from_others makes such planes from a frame's instance masks).
        ``known`` goes with masks only (a field already says what it knows) and adds iou_visible / iou0_visible [B], the IoU over the
        known pixels."""
        planes, known = self._field_of(mask_or_sdf, known)
        return AttrDict(ops.silhouette_align(self.verts, self.faces, pose, intr, planes, tau_px=self.tau_px, iters=self.iters,
                                             damping=self.damping, frame=frame, mask=mask, workspace=self._workspace(pose.shape[0]),
                                             visible_iou=known is not None, cull=self.cull))
