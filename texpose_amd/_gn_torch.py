"""The per-image half of the Gauss-Newton refiners in plain torch ops in fp64, shared by the step_torch of icp, photo_align, silhouette
and joint: the frame choice, the 6x6 Cholesky with the header's pivot rule, the exponential map and everything from the summed system
to the output dict (count and status rules, the damped step, Gram-Schmidt, the fp32 rounding, the pass-through of a failed pose).
Each refiner builds its residual rows between ``sums_head`` and ``normal_sums`` (the two with an image gradient through
``image_gradient_rows``) and calls ``solve``."""
from typing import Dict, Optional

import torch

Tensor = torch.Tensor
PIVOT_TOL = 1e-10
MIN_COUNT = 6


def _cholesky6(A: Tensor, tol: float):
    """Batched Cholesky of A [B,6,6] with the header's pivot rule -> (L [B,6,6], ok [B] bool); rows of a failed matrix hold garbage."""
    B = A.shape[0]
    L = torch.zeros_like(A)
    ok = torch.ones(B, dtype=torch.bool, device=A.device)
    for j in range(6):
        diag = A[:, j, j]
        d = diag - (L[:, j, :j] * L[:, j, :j]).sum(-1)
        ok = ok & torch.isfinite(d) & (d > tol * diag) & (d > 0)
        l = torch.sqrt(torch.where(ok, d, torch.ones_like(d)))
        L[:, j, j] = l
        for i in range(j + 1, 6):
            L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(-1)) / l
    return L, ok


def _exp_so3(w: Tensor) -> Tensor:
    th2 = (w * w).sum(-1)
    th = torch.sqrt(th2)
    big = th > 1e-8
    safe, safe2 = torch.where(big, th, torch.ones_like(th)), torch.where(big, th2, torch.ones_like(th2))
    sa = torch.where(big, torch.sin(safe) / safe, 1.0 - th2 / 6.0)[:, None, None]
    sb = torch.where(big, (1.0 - torch.cos(safe)) / safe2, 0.5 - th2 / 24.0)[:, None, None]
    Wx = torch.zeros(w.shape[0], 3, 3, dtype=w.dtype, device=w.device)
    Wx[:, 0, 1], Wx[:, 0, 2], Wx[:, 1, 0], Wx[:, 1, 2], Wx[:, 2, 0], Wx[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    return torch.eye(3, dtype=w.dtype, device=w.device)[None] + sa * Wx + sb * (Wx @ Wx)


def frames_of(B: int, Ft: int, frame: Optional[Tensor], what: str, device=None) -> Tensor:
    """The measured plane of each of B images among Ft [B] long: the only one, its own, or ``frame`` clamped into range; ``what``
    names the planes in the error ('depth must hold 1 or B = 3 planes')."""
    if frame is None:
        if Ft not in (1, B):
            raise ValueError("step_torch: %s without frame=, got %d" % (what % B, Ft))
        return torch.zeros(B, dtype=torch.long, device=device) if Ft == 1 else torch.arange(B, device=device)
    return frame.long().clamp(0, Ft - 1)


def sums_head(zbuf: Tensor, pose: Tensor, intr: Tensor, planes: Tensor, trailing: int, frame: Optional[Tensor], what: str, tau: float):
    """What every sums_torch starts from: ``planes`` the measured planes [Ft,H,W] + ``trailing`` dimensions (or one plane), ``what``
    their name for frames_of -> (B, H, W, pose32 [B,3,4], intr [B,3,3] float32, planes [Ft,...] float32, fr [B] long, tau rounded to
    fp32, zbuf as float32)."""
    B, H, W = zbuf.shape
    pose32 = pose.float().reshape(B, 3, 4)
    intr = intr.float()
    if intr.dim() == 2:
        intr = intr[None].expand(B, 3, 3)
    planes = planes.float()
    if planes.dim() == 2 + trailing:
        planes = planes[None]
    fr = frames_of(B, planes.shape[0], frame, what, zbuf.device)
    return B, H, W, pose32, intr, planes, fr, float(torch.tensor(tau, dtype=torch.float32)), zbuf.float()


def masked(cand: Tensor, mask: Optional[Tensor], fr: Tensor) -> Tensor:
    """``cand`` [B,H,W] without the pixels whose mask [Ft,H,W] (or one [H,W]) is 0 in the image's plane."""
    if mask is None:
        return cand
    m = mask if mask.dim() == 3 else mask[None]
    return cand & (m[fr] != 0)


def image_gradient_rows(zf: Tensor, intr: Tensor, bi: Tensor, ii: Tensor, ji: Tensor, lf: Tensor, rt: Tensor, up: Tensor, dn: Tensor) -> Tensor:
    """The Jacobian rows of n interior pixels (bi, ii, ji) whose residuals are read off an image with C channels: lf, rt, up, dn [n,C]
    fp64, the image at the four neighbours (central differences) -> J [n C,6], the channels of a pixel one after the other."""
    f64 = torch.float64
    z = zf[bi, ii, ji].to(f64)
    K = intr.to(f64)
    fx, fy = K[bi, 0, 0], K[bi, 1, 1]
    rx = ((ji.to(f64) + 0.5) - K[bi, 0, 2]) / fx
    ry = ((ii.to(f64) + 0.5) - K[bi, 1, 2]) / fy
    P = torch.stack([z * rx, z * ry, z], -1)[:, None, :].expand(-1, lf.shape[1], -1)        # [n,C,3]
    gfx, gfy = (0.5 * (rt - lf)) * fx[:, None], (0.5 * (dn - up)) * fy[:, None]             # [n,C]
    av = torch.stack([gfx / z[:, None], gfy / z[:, None], -(gfx * rx[:, None] + gfy * ry[:, None]) / z[:, None]], -1)
    return torch.cat([torch.cross(P, av, dim=-1), av], -1).reshape(-1, 6)


def normal_sums(B: int, bi: Tensor, J: Tensor, r: Tensor):
    """The rows J [n,6] with residuals r [n] of images bi [n] summed per image -> (JtJ [B,6,6], Jtr [B,6], cost [B]) fp64."""
    f64, dev = torch.float64, J.device
    JtJ = torch.zeros(B, 6, 6, dtype=f64, device=dev).index_add_(0, bi, J[:, :, None] * J[:, None, :])
    Jtr = torch.zeros(B, 6, dtype=f64, device=dev).index_add_(0, bi, J * r[:, None])
    cost = torch.zeros(B, dtype=f64, device=dev).index_add_(0, bi, r * r)
    return JtJ, Jtr, cost


def solve(JtJ: Tensor, Jtr: Tensor, cost: Tensor, count: Tensor, pose32: Tensor, damping: float, evaluate_only: bool) -> Dict[str, Tensor]:
    """JtJ [B,6,6], Jtr [B,6], cost [B] (fp64 sums over the kept rows), count [B] (kept pixels), pose32 [B,3,4] float32 -> 'pose'
    [B,3,4] float32, 'inliers' [B] int32, 'rms' [B] float32, 'status' [B] int32 by the header's rules."""
    f64 = torch.float64
    B, dev = pose32.shape[0], pose32.device
    lam = float(torch.tensor(damping, dtype=torch.float32))
    rms = torch.sqrt(cost / count.to(f64))                                                  # (0 / 0: NaN)
    few = count < MIN_COUNT
    _, pd = _cholesky6(JtJ, PIVOT_TOL)
    status = torch.where(few, 1, torch.where(pd, 0, 3))
    out_pose = pose32.clone()
    if not evaluate_only:
        Dm = JtJ + lam * torch.diag_embed(torch.diagonal(JtJ, dim1=1, dim2=2))
        L, ok = _cholesky6(Dm, 0.0)
        ok = ok & pd & ~few
        eye = torch.eye(6, dtype=f64, device=dev)[None]
        L = torch.where(ok[:, None, None], L, eye)
        y = torch.linalg.solve_triangular(L, -Jtr[:, :, None], upper=False)
        delta = torch.linalg.solve_triangular(L.transpose(1, 2), y, upper=True)[:, :, 0]
        delta = torch.where(ok[:, None], delta, torch.zeros_like(delta))                    # (such a pose is passed through below)
        Pn = _exp_so3(delta[:, :3]) @ pose32.to(f64)
        Pn[:, :, 3] = Pn[:, :, 3] + delta[:, 3:]
        c1 = Pn[:, :, 0] / torch.linalg.norm(Pn[:, :, 0], dim=-1, keepdim=True)
        c2 = Pn[:, :, 1] - c1 * (c1 * Pn[:, :, 1]).sum(-1, keepdim=True)
        c2 = c2 / torch.linalg.norm(c2, dim=-1, keepdim=True)
        Pn = torch.stack([c1, c2, torch.cross(c1, c2, dim=-1), Pn[:, :, 3]], -1)
        new32 = Pn.float()
        ok = ok & torch.isfinite(new32).reshape(B, -1).all(-1)
        status = torch.where(few, 1, torch.where(ok, 0, 3))
        out_pose = torch.where(ok[:, None, None], new32, pose32)
    return dict(pose=out_pose, inliers=count.to(torch.int32), rms=rms.float(), status=status.to(torch.int32))
