"""Joint pose refinement: silhouette, colour and depth in one Gauss-Newton step (K33).

texpose_amd.silhouette, texpose_amd.photo_align and texpose_amd.icp each state where they stop: the silhouette closes the outline and
the pose need not follow (with part of the object hidden it ends tens of degrees away while the visible IoU rises), the photometric
term has the basin its texture's smoothness gives, the depth term cannot see a rotation about a symmetry axis.  Run one after the
other under occlusion the first walks off and the second cannot come back.  Here all residual rows go into ONE normal system per step:
the three terms already share the six parameters and the 29 fp64 sums, so a step is each term's own reduce followed by one small
kernel that adds the sums with weights and solves (``ops.joint_align_step``; ``ops.joint_align`` is the loop, one rasteriser call per
pass).  A weight is 1 / sigma^2 of the term's residual unit; the defaults are ``ops.JOINT_WEIGHTS`` = (1, 100, 1 / 25): the photometric
one is the only one of 25, 100 and 400 that converged on all twelve occluded cases of DESIGN section 23, the depth one is sigma = 5 mm
and is not tuned on anything.  ``JointRefiner`` keeps the mesh and the workspace of a batch size.  ``step_torch`` says the step again
in plain torch ops: each term's ``sums_torch``, weighted and added, then the shared solve.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _gn_torch, ops
from . import icp as _icp, photo_align as _photo, silhouette as _sil
from ._refiner import _MeshRefiner
from .options import AttrDict

Tensor = torch.Tensor


def sums_torch(pose: Tensor, intr: Tensor, *, silhouette: Optional[dict] = None, photo: Optional[dict] = None, depth: Optional[dict] = None,
               weights=ops.JOINT_WEIGHTS, damping: float = 1e-6):
    """The combined sums of every image: each present term's ``sums_torch`` at ``pose``, weighted and added over the terms with a
    weight > 0 -> ((JtJ [B,6,6], Jtr [B,6], cost [B], count [B]) fp64, each present term's own evaluation under its prefix, pose as
    float32 [B,3,4])."""
    w = ops._joint_weights("step_torch", weights)
    terms = (("sil_", silhouette, w[0], lambda t: _sil.sums_torch(t["zbuf"], pose, intr, t["sdf"], t["tau_px"], t.get("frame"), t.get("mask"))),
             ("photo_", photo, w[1], lambda t: _photo.sums_torch(t["zbuf"], t["rgb"], pose, intr, t["image"], t["tau"], t.get("frame"), t.get("mask"))),
             ("icp_", depth, w[2], lambda t: _icp.sums_torch(t["verts"], t["faces"], t["zbuf"], t["face"], pose, intr, t["depth"], t["tau_mm"],
                                                            t.get("frame"), t.get("mask"))))
    if not any(t is not None and x > 0 for _, t, x, _ in terms):
        raise ValueError("step_torch: no present term has a weight > 0")
    total, res, pose32 = None, {}, None
    for prefix, t, x, sums in terms:
        if t is None:
            continue
        s = sums(t)
        JtJ, Jtr, cost, count, pose32 = s[:5]
        own = _gn_torch.solve(JtJ, Jtr, cost, count, pose32, damping, True)
        res.update({prefix + k: own[k] for k in ("inliers", "rms", "status")})
        if prefix == "sil_":
            res["sil_inter"], res["sil_uni"] = s[5:]
        if x > 0:
            part = (x * JtJ, x * Jtr, x * cost, count)
            total = part if total is None else tuple(a + b for a, b in zip(total, part))
    return total, res, pose32


def step_torch(pose: Tensor, intr: Tensor, *, silhouette: Optional[dict] = None, photo: Optional[dict] = None,
               depth: Optional[dict] = None, weights=ops.JOINT_WEIGHTS, damping: float = 1e-6, evaluate_only: bool = False) -> Dict[str, Tensor]:
    """ops.joint_align_step's rules (include/texpose_amd.h, K33) in plain torch ops in fp64 on the tensors' device: the terms are the
    dicts ops.joint_align_step takes -> 'pose' [B,3,4] float32, 'inliers', 'status' [B]
    int32, 'chi2' [B] float32 and each present term's own evaluation under its prefix ('sil_', 'photo_', 'icp_').  A term that is
    absent or has weight 0 takes no part in the sum."""
    total, res, pose32 = sums_torch(pose, intr, silhouette=silhouette, photo=photo, depth=depth, weights=weights, damping=damping)
    out = _gn_torch.solve(*total, pose32, damping, evaluate_only)
    return dict(res, pose=out["pose"], inliers=out["inliers"], status=out["status"], chi2=total[2].float())


class JointRefiner(_MeshRefiner):
    """Joint refinement for batches of poses of one mesh at H x W with the mesh (and its colours) on the device and a workspace per
    batch size.

    ``weights`` (w_sil, w_photo, w_icp; ops.JOINT_WEIGHTS), ``tau_px`` / ``tau`` / ``tau_mm`` (each term's threshold, one value or
    ``iters`` + 1), ``iters`` (Gauss-Newton steps, 20), ``damping`` (relative, 1e-6), ``exposure`` (the photometric term fits the
    photograph's gain and bias per image and channel in every pass: ops.photo_exposure, K37) or, in its place, ``lighting`` (ambient +
    directional shading on the faces' normals and a bias: ops.photo_lighting, K40).  ``refine`` returns ops.joint_align's dict."""
    _new_workspace = staticmethod(ops.joint_align_workspace)

    def __init__(self, verts: Tensor, faces: Tensor, H: int, W: int, device="cuda:0", *, vcolor: Optional[Tensor] = None,
                 weights=ops.JOINT_WEIGHTS, tau_px=4.0, tau=0.5, tau_mm=20.0, iters: int = 20, damping: float = 1e-6, cull: bool = False,
                 texels: Optional[Tensor] = None, exposure: bool = False, exposure_tau0: float = 2.0, lighting: bool = False):
        if exposure and lighting:                                # (host arguments: refused before anything touches the device)
            raise ValueError("JointRefiner: exposure= and lighting= exclude each other (the lighting model contains the exposure's)")
        super().__init__(verts, faces, H, W, device, cull=cull)
        if vcolor is not None and texels is not None:
            raise ValueError("JointRefiner: vcolor= or texels=, not both")
        self._colours(vcolor, texels)
        self.weights = ops._joint_weights("JointRefiner", weights)
        self.tau_px, self.tau, self.tau_mm, self.iters, self.damping = tau_px, tau, tau_mm, int(iters), float(damping)
        self.exposure, self.exposure_tau0, self.lighting = bool(exposure), float(exposure_tau0), bool(lighting)

    def refine(self, pose: Tensor, intr: Tensor, *, mask_or_sdf: Optional[Tensor] = None, known: Optional[Tensor] = None,
               image: Optional[Tensor] = None, depth: Optional[Tensor] = None, frame: Optional[Tensor] = None,
               masks: Optional[dict] = None) -> AttrDict:
        """pose [B,3,4], intr [B,3,3] or [3,3]; the terms are the measurements given: mask_or_sdf [Ft,H,W] (the measured masks, uint8 or
        bool, run through ops.mask_sdf first, or their fields, a float tensor taken as it is), image [Ft,H,W,3] (needs the refiner's
        vcolor), depth [Ft,H,W] (mm).  frame [B] int32: the plane of each pose.  known [Ft,H,W] uint8 / bool (0: the pixel was not
        measured: behind an occluder, say) goes with masks only: the field is built with ops.mask_sdf(known=), the photometric and the
        depth term take ``known`` as their mask (ANDed with their plane of ``masks``, if any), and the result has iou_visible / iou0_visible as SilhouetteRefiner's.  masks:
        dict(silhouette=, photo=, depth=) of further [Ft,H,W] planes (0: the term skips the pixel)."""
        planes = None
        masks = dict(masks or {})
        if known is not None and mask_or_sdf is None:
            raise ValueError("JointRefiner.refine: known= goes with the measured masks (mask_or_sdf=)")
        if mask_or_sdf is not None:
            planes, known = self._field_of(mask_or_sdf, known)
            if known is not None:
                for term in ("photo", "depth"):                  # (with a mask of the caller's: both must allow the pixel)
                    own = masks.get(term)
                    masks[term] = known if own is None else ((own if own.dim() == 3 else own[None]).to(self.device) != 0) & (known != 0)
        if image is not None and self.vcolor is None and self.texels is None:
            raise ValueError("JointRefiner.refine: image= needs the refiner's vcolor= or texels=")
        masks = {k: v for k, v in masks.items() if (k == "silhouette" and planes is not None) or (k == "photo" and image is not None)
                 or (k == "depth" and depth is not None)}
        return AttrDict(ops.joint_align(self.verts, self.faces, pose, intr, vcolor=self.vcolor, texels=self.texels, sdf=planes, image=image, depth=depth,
                                        weights=self.weights, tau_px=self.tau_px, tau=self.tau, tau_mm=self.tau_mm, iters=self.iters,
                                        damping=self.damping, frame=frame, masks=masks, workspace=self._workspace(pose.shape[0]),
                                        visible_iou=known is not None, cull=self.cull, exposure=self.exposure, exposure_tau0=self.exposure_tau0,
                                        lighting=self.lighting))
