"""Multi-view pose refinement: ONE object pose from several cameras (K39).

Every refiner of K29-K38 treats an image as its own problem: B poses in, B unrelated poses out.  A BOP scene is hundreds of frames of
the same rigid objects with each frame's camera pose in scene_camera.json (cam_R_w2c, cam_t_w2c), and what a single image cannot pin --
the pose behind a closed outline, an object half hidden, translation along the optical axis -- another view usually can.  Here all
views of an object put their residual rows into one normal system for one pose: views i with fixed cameras C_i (world -> camera) are
grouped, group g has the unknown M_g (model -> world), view i is rendered and evaluated at T_i = C_i o M_group[i]
(``ops.pose_compose``), and one step (``ops.multiview_align_step``) is each term's own reduce at T_i, K33's weighted sums per view,
the change of variables H' = A^T H A, g' = A^T g with A_i = [[Rc, 0], [[tc]x Rc, Rc]] that rewrites a view's camera-frame increment
as the group's world-frame increment, the sum over the group's views and K29's solve at M_g.  ``ops.multiview_align`` is the loop (one
rasteriser call per pass over all views), ``MultiViewRefiner`` keeps the mesh and a workspace per batch size, ``init_model`` picks a
start from per-view estimates, and ``step_torch`` says the step again in plain torch ops.  The cameras are taken as exact: camera
poses as unknowns, per-view robust weights and instance association across frames are out of scope.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _gn_torch, ops
from . import joint as _joint
from ._refiner import _MeshRefiner
from .options import AttrDict

Tensor = torch.Tensor


def _is_identity(cam32: Tensor) -> Tensor:
    """cam [B,3,4] float32 -> [B] bool: bit-exactly [I|0] (the words of 1.0f and +0.0f: a -0.0 is not)."""
    want = torch.eye(3, 4, dtype=torch.float32, device=cam32.device).view(torch.int32)
    return (cam32.contiguous().view(torch.int32) == want[None]).reshape(cam32.shape[0], -1).all(-1)


def compose_torch(cam: Tensor, model: Tensor, group: Tensor) -> Tensor:
    """ops.pose_compose's rule in torch fp64: cam [B,3,4], model [Gr,3,4], group [B] -> [B,3,4] float32."""
    cam32, model32 = cam.float(), model.float()
    m32 = model32[group.long().clamp(0, model32.shape[0] - 1)]
    c, m = cam32.double(), m32.double()
    T = (c[:, :, 0:1] * m[:, 0:1, :] + c[:, :, 1:2] * m[:, 1:2, :]) + c[:, :, 2:3] * m[:, 2:3, :]
    T[:, :, 3] = T[:, :, 3] + c[:, :, 3]
    return torch.where(_is_identity(cam32)[:, None, None], m32, T.float())


def adjoint_torch(cam: Tensor) -> Tensor:
    """A [B,6,6] fp64 of the header's change of variables, from cam [B,3,4]: [[Rc, 0], [[tc]x Rc, Rc]]."""
    c = cam.float().double()
    R, t = c[:, :, :3], c[:, :, 3]
    X = torch.stack([(-t[:, 2:3]) * R[:, 1] + t[:, 1:2] * R[:, 2], t[:, 2:3] * R[:, 0] + (-t[:, 0:1]) * R[:, 2],
                     (-t[:, 1:2]) * R[:, 0] + t[:, 0:1] * R[:, 1]], 1)
    A = torch.zeros(c.shape[0], 6, 6, dtype=torch.float64, device=c.device)
    A[:, :3, :3], A[:, 3:, :3], A[:, 3:, 3:] = R, X, R
    return A


def step_torch(model: Tensor, cam: Tensor, group: Tensor, intr: Tensor, *, silhouette: Optional[dict] = None, photo: Optional[dict] = None,
               depth: Optional[dict] = None, weights=ops.JOINT_WEIGHTS, damping: float = 1e-6, evaluate_only: bool = False) -> Dict[str, Tensor]:
    """ops.multiview_align_step's rules (include/texpose_amd.h, K39) in plain torch ops in fp64 on the tensors' device: the terms are
    joint.step_torch's dicts with planes rendered at compose_torch(cam, model, group) -> 'model' [Gr,3,4] and 'pose' [B,3,4] float32,
    'inliers', 'status', 'views' [Gr] int32, 'chi2' [Gr] float32 and each present term's own evaluation [B] under its prefix."""
    Gr = model.shape[0]
    ids = group.long().clamp(0, Gr - 1)
    pose = compose_torch(cam, model, group)
    (JtJ, Jtr, cost, count), res, _ = _joint.sums_torch(pose, intr, silhouette=silhouette, photo=photo, depth=depth, weights=weights, damping=damping)
    A = adjoint_torch(cam)
    plain = _is_identity(cam.float())
    JtJ = torch.where(plain[:, None, None], JtJ, A.transpose(1, 2) @ (JtJ @ A))
    Jtr = torch.where(plain[:, None], Jtr, (A.transpose(1, 2) @ Jtr[:, :, None])[:, :, 0])
    f64, dev = torch.float64, JtJ.device
    gJ = torch.zeros(Gr, 6, 6, dtype=f64, device=dev).index_add_(0, ids, JtJ)
    gr = torch.zeros(Gr, 6, dtype=f64, device=dev).index_add_(0, ids, Jtr)
    gc = torch.zeros(Gr, dtype=f64, device=dev).index_add_(0, ids, cost)
    gn = torch.zeros(Gr, dtype=count.dtype, device=dev).index_add_(0, ids, count)
    views = torch.zeros(Gr, dtype=torch.int32, device=dev).index_add_(0, ids, (count > 0).to(torch.int32))
    out = _gn_torch.solve(gJ, gr, gc, gn, model.float().reshape(Gr, 3, 4), damping, evaluate_only)
    return dict(res, model=out["pose"], pose=compose_torch(cam, out["pose"], group), inliers=out["inliers"], status=out["status"],
                chi2=gc.float(), views=views)


def init_model(pose: Tensor, cam: Tensor, group: Tensor, score: Optional[Tensor] = None, groups: Optional[int] = None) -> Tensor:
    """A start for the groups' models from per-view estimates: pose [B,3,4] (model -> camera i), cam [B,3,4], group [B] ->
    [Gr,3,4] float32: per group the view with the highest ``score`` [B] (ties, and no score, go to the lowest view index) gives
    C^-1 o T in fp64.  ``groups``: Gr (default: the largest id + 1, a host read).  A group without a view gets the identity."""
    ids = group.long()
    Gr = int(ids.max()) + 1 if groups is None else int(groups)
    B, dev = pose.shape[0], pose.device
    s = torch.zeros(B, dtype=torch.float64, device=dev) if score is None else score.double()
    best = torch.full((Gr,), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce(0, ids, s, "amax", include_self=True)
    index = torch.arange(B, device=dev)
    cand = torch.where(s == best[ids], index, torch.full_like(index, B))
    pick = torch.full((Gr,), B, dtype=index.dtype, device=dev).scatter_reduce(0, ids, cand, "amin", include_self=True)
    some = pick < B
    pick = pick.clamp(max=B - 1)
    c, T = cam.float().double()[pick], pose.float().double()[pick]
    Rt = c[:, :, :3].transpose(1, 2)
    M = torch.cat([Rt @ T[:, :, :3], Rt @ (T[:, :, 3:] - c[:, :, 3:])], 2)
    eye = torch.eye(3, 4, dtype=torch.float64, device=dev)[None]
    return torch.where(some[:, None, None], M, eye).float()


class MultiViewRefiner(_MeshRefiner):
    """Multi-view refinement for batches of views of one mesh at H x W with the mesh (and its colours) on the device and a workspace per
    batch size; the keywords are JointRefiner's (``lighting`` fits one light per VIEW).  ``refine`` returns ops.multiview_align's dict: 'model' [Gr,3,4], the per-view 'pose'
    [B,3,4], and the rest."""
    _new_workspace = staticmethod(ops.multiview_align_workspace)

    def __init__(self, verts: Tensor, faces: Tensor, H: int, W: int, device="cuda:0", *, vcolor: Optional[Tensor] = None,
                 weights=ops.JOINT_WEIGHTS, tau_px=4.0, tau=0.5, tau_mm=20.0, iters: int = 20, damping: float = 1e-6, cull: bool = False,
                 texels: Optional[Tensor] = None, exposure: bool = False, exposure_tau0: float = 2.0, lighting: bool = False):
        if exposure and lighting:                                # (host arguments: refused before anything touches the device)
            raise ValueError("MultiViewRefiner: exposure= and lighting= exclude each other (the lighting model contains the exposure's)")
        super().__init__(verts, faces, H, W, device, cull=cull)
        if vcolor is not None and texels is not None:
            raise ValueError("MultiViewRefiner: vcolor= or texels=, not both")
        self._colours(vcolor, texels)
        self.weights = ops._joint_weights("MultiViewRefiner", weights)
        self.tau_px, self.tau, self.tau_mm, self.iters, self.damping = tau_px, tau, tau_mm, int(iters), float(damping)
        self.exposure, self.exposure_tau0, self.lighting = bool(exposure), float(exposure_tau0), bool(lighting)

    def refine(self, model: Tensor, cam: Tensor, group: Tensor, intr: Tensor, *, mask_or_sdf: Optional[Tensor] = None,
               known: Optional[Tensor] = None, image: Optional[Tensor] = None, depth: Optional[Tensor] = None,
               frame: Optional[Tensor] = None, masks: Optional[dict] = None) -> AttrDict:
        """model [Gr,3,4], cam [B,3,4], group [B] int32, intr [B,3,3] or [3,3]; the measurements are JointRefiner.refine's, one plane
        per VIEW (or by ``frame`` [B]): mask_or_sdf, known, image, depth, masks."""
        planes = None
        masks = dict(masks or {})
        if known is not None and mask_or_sdf is None:
            raise ValueError("MultiViewRefiner.refine: known= goes with the measured masks (mask_or_sdf=)")
        if mask_or_sdf is not None:
            planes, known = self._field_of(mask_or_sdf, known)
            if known is not None:
                for term in ("photo", "depth"):                  # (with a mask of the caller's: both must allow the pixel)
                    own = masks.get(term)
                    masks[term] = known if own is None else ((own if own.dim() == 3 else own[None]).to(self.device) != 0) & (known != 0)
        if image is not None and self.vcolor is None and self.texels is None:
            raise ValueError("MultiViewRefiner.refine: image= needs the refiner's vcolor= or texels=")
        masks = {k: v for k, v in masks.items() if (k == "silhouette" and planes is not None) or (k == "photo" and image is not None)
                 or (k == "depth" and depth is not None)}
        return AttrDict(ops.multiview_align(self.verts, self.faces, model, cam, group, intr, vcolor=self.vcolor, texels=self.texels, sdf=planes,
                                            image=image, depth=depth, weights=self.weights, tau_px=self.tau_px, tau=self.tau, tau_mm=self.tau_mm,
                                            iters=self.iters, damping=self.damping, frame=frame, masks=masks, workspace=self._workspace(cam.shape[0]),
                                            visible_iou=known is not None, cull=self.cull, exposure=self.exposure, exposure_tau0=self.exposure_tau0,
                                            lighting=self.lighting))
