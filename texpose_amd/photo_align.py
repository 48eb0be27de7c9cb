"""Pose refinement against the photograph: batched photometric alignment on the device (K30).

The RGB sibling of texpose_amd.icp: the vertex-coloured mesh (texpose_amd.texture_bake gives one from a checkpoint) is rendered at the
current poses by the HIP rasteriser, every interior covered pixel whose rendered colour lies within ``tau`` of the photograph's gives
three residuals, one per channel, against the photograph's own central-difference gradient, and one damped Gauss-Newton step in fp64
moves the pose (``ops.photo_align_step``; ``ops.photo_align`` is the loop).  ``PhotoRefiner`` keeps the mesh and the workspace of a
batch size.  ``step_torch`` says the step again in plain torch ops in fp64: the comparator of tools/photo_align_bench.py, and the one
piece that also runs without a GPU.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _gn_torch, ops
from ._refiner import _MeshRefiner
from .options import AttrDict

Tensor = torch.Tensor


def step_torch(zbuf: Tensor, rgb: Tensor, pose: Tensor, intr: Tensor, image: Tensor, tau: float, damping: float = 1e-6,
               frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, evaluate_only: bool = False) -> Dict[str, Tensor]:
    """ops.photo_align_step's rules (include/texpose_amd.h, K30) in plain torch ops in fp64 on the tensors' device: the same arguments
    -> 'pose' [B,3,4] float32, 'inliers' [B] int32, 'rms' [B] float32, 'status' [B] int32.  The sums run in torch's order, not the
    kernel's: counts and statuses agree, the rest to rounding."""
    JtJ, Jtr, cost, count, pose32 = sums_torch(zbuf, rgb, pose, intr, image, tau, frame, mask)
    return _gn_torch.solve(JtJ, Jtr, cost, count, pose32, damping, evaluate_only)


def sums_torch(zbuf: Tensor, rgb: Tensor, pose: Tensor, intr: Tensor, image: Tensor, tau: float, frame: Optional[Tensor] = None,
               mask: Optional[Tensor] = None):
    """The sums of step_torch before the solve (what joint.step_torch weights and adds) -> (JtJ [B,6,6], Jtr [B,6], cost [B] fp64,
    count [B], pose32 [B,3,4])."""
    f64 = torch.float64
    B, H, W, pose32, intr, image, fr, tau, zf = _gn_torch.sums_head(zbuf, pose, intr, image, 1, frame, "image must hold 1 or B = %d photographs", tau)
    cand = (zf > 0) & torch.isfinite(zf)
    cand[:, :1], cand[:, H - 1:], cand[:, :, :1], cand[:, :, W - 1:] = False, False, False, False
    cand = _gn_torch.masked(cand, mask, fr)
    bi, ii, ji = torch.nonzero(cand, as_tuple=True)                                         # (interior: ii -+ 1 and ji -+ 1 exist)
    fi = fr[bi]
    c, o = rgb.float()[bi, ii, ji].to(f64), image[fi, ii, ji].to(f64)                       # [n,3]
    lf, rt = image[fi, ii, ji - 1].to(f64), image[fi, ii, ji + 1].to(f64)
    up, dn = image[fi, ii - 1, ji].to(f64), image[fi, ii + 1, ji].to(f64)
    res = o - c
    fin = torch.isfinite(torch.cat([c, o, lf, rt, up, dn], -1)).all(-1)
    keep = fin & ((res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1]) + res[:, 2] * res[:, 2] <= tau * tau)
    bi, ii, ji, res, lf, rt, up, dn = bi[keep], ii[keep], ji[keep], res[keep], lf[keep], rt[keep], up[keep], dn[keep]
    J = _gn_torch.image_gradient_rows(zf, intr, bi, ii, ji, lf, rt, up, dn)                 # [3n,6]
    return _gn_torch.normal_sums(B, bi.repeat_interleave(3), J, res.reshape(-1)) + (torch.bincount(bi, minlength=B), pose32)


def exposure_torch(zbuf: Tensor, rgb: Tensor, image: Tensor, tau: float, gain: Optional[Tensor] = None, bias: Optional[Tensor] = None,
                   frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, gain_range=(0.25, 4.0), min_var: float = 1e-6,
                   apply: bool = True) -> Dict[str, Tensor]:
    """ops.photo_exposure's rules (include/texpose_amd.h, K37) in plain torch ops in fp64 on the tensors' device: the same arguments
    -> 'gain' / 'bias' [B,3] float32, 'count' [B] int32, 'rms' [B] float32, 'status', 'flags' [B] int32 and, with ``apply``, 'rgb'
    [B,H,W,3] float32 (a new tensor).  The sums run in torch's order, not the kernel's: counts, statuses and flags agree, the rest to
    rounding; 'rgb' is the kernel's bit for bit from the same gain and bias."""
    f64, f32 = torch.float64, torch.float32
    B, H, W = zbuf.shape
    zf, c32, image = zbuf.float(), rgb.float(), image.float()
    image = image if image.dim() == 4 else image[None]
    fr = _gn_torch.frames_of(B, image.shape[0], frame, "image must hold 1 or B = %d photographs", zbuf.device)
    as_f32 = lambda v: float(torch.tensor(v, dtype=f32))
    tau, lo, hi, min_var = as_f32(tau), as_f32(gain_range[0]), as_f32(gain_range[1]), as_f32(min_var)
    g_in = torch.ones(B, 3, dtype=f32, device=zbuf.device) if gain is None else gain.float()
    b_in = torch.zeros(B, 3, dtype=f32, device=zbuf.device) if bias is None else bias.float()
    covered = (zf > 0) & torch.isfinite(zf)
    cand = covered.clone()
    cand[:, :1], cand[:, H - 1:], cand[:, :, :1], cand[:, :, W - 1:] = False, False, False, False
    cand = _gn_torch.masked(cand, mask, fr)
    c, o = c32.to(f64), image[fr].to(f64)                                                   # [B,H,W,3]
    res = o - (g_in.to(f64)[:, None, None, :] * c + b_in.to(f64)[:, None, None, :])
    keep = cand & torch.isfinite(c).all(-1) & torch.isfinite(o).all(-1) & ((res[..., 0] * res[..., 0] + res[..., 1] * res[..., 1])
                                                                          + res[..., 2] * res[..., 2] <= tau * tau)
    k3 = keep[..., None]
    zero = torch.zeros((), dtype=f64, device=zbuf.device)
    total = lambda v: torch.where(k3, v, zero).flatten(1, 2).sum(1)                         # [B,3]
    n = keep.flatten(1).sum(1).to(f64)[:, None]
    mc, mo = total(c) / n, total(o) / n
    var, cov, voo = total(c * c) / n - mc * mc, total(c * o) / n - mc * mo, total(o * o) / n - mo * mo
    live = var > min_var
    q = cov / torch.where(live, var, torch.ones_like(var))
    g = torch.where(live, q.clamp(lo, hi), torch.ones_like(q))
    ch = torch.arange(3, device=zbuf.device)
    flags = ((live & (g != q)).long() << ch).sum(1) + ((~live).long() << (3 + ch)).sum(1)
    b = mo - g * mc
    sse = n * ((voo - 2.0 * (g * cov)) + (g * g) * var)
    rms = torch.sqrt(((sse[:, 0] + sse[:, 1]) + sse[:, 2]).clamp_min(0.0) / n[:, 0]).to(f32)
    g32, b32 = g.to(f32), b.to(f32)
    few = n[:, 0] < _gn_torch.MIN_COUNT
    fine = torch.isfinite(g32).all(1) & torch.isfinite(b32).all(1) & torch.isfinite(rms)
    status = torch.where(few, 1, torch.where(fine, 0, 3)).to(torch.int32)
    ok = (status == 0)[:, None]
    out = dict(gain=torch.where(ok, g32, g_in), bias=torch.where(ok, b32, b_in), count=n[:, 0].to(torch.int32), rms=rms, status=status,
               flags=flags.to(torch.int32))
    if apply:
        lit = out["gain"][:, None, None, :] * c32                                           # (two fp32 operations)
        out["rgb"] = torch.where(covered[..., None], lit + out["bias"][:, None, None, :], c32)
    return out


def _pixel_normals_torch(verts: Tensor, faces: Tensor, face: Tensor, pose: Tensor):
    """K40's valid normal of every pixel in fp64: face [B,H,W] -> (n [B,H,W,3], valid [B,H,W]); invalid pixels hold 0."""
    f64 = torch.float64
    v, P = verts.float().to(f64), pose.float().to(f64)
    idx = faces.long()
    V, F = v.shape[0], idx.shape[0]
    ok = ((idx >= 0) & (idx < V)).all(1)                                                    # [F]
    safe = torch.where(ok[:, None], idx, torch.zeros_like(idx))
    v0, v1, v2 = v[safe[:, 0]], v[safe[:, 1]], v[safe[:, 2]]
    a, b = v1 - v0, v2 - v0
    m = torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    R, t = P[:, None, :, :3], P[:, None, :, 3]                                              # [B,1,3,3], [B,1,3]
    rows = lambda x: (R[..., 0] * x[None, :, None, 0] + R[..., 1] * x[None, :, None, 1]) + R[..., 2] * x[None, :, None, 2]     # [B,F,3]
    n = rows(m)
    d = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
    good = ok[None] & torch.isfinite(d) & (d > 0)
    n = n / torch.sqrt(torch.where(good, d, torch.ones_like(d)))[..., None]
    xc = rows(v0) + t
    away = (n[..., 0] * xc[..., 0] + n[..., 1] * xc[..., 1]) + n[..., 2] * xc[..., 2] > 0
    n = torch.where(good[..., None], torch.where(away[..., None], -n, n), torch.zeros_like(n))
    fi = face.long()
    inside = (fi >= 0) & (fi < F)
    g = torch.where(inside, fi, torch.zeros_like(fi))
    bi = torch.arange(face.shape[0], device=face.device)[:, None, None]
    valid = inside & good[bi, g]
    return torch.where(valid[..., None], n[bi, g], torch.zeros((), dtype=f64, device=face.device)), valid


def lighting_torch(verts: Tensor, faces: Tensor, face: Tensor, zbuf: Tensor, rgb: Tensor, pose: Tensor, image: Tensor, tau: float,
                   light: Optional[Tensor] = None, frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, gain_range=(0.25, 4.0),
                   min_var: float = 1e-6, apply: bool = True) -> Dict[str, Tensor]:
    """ops.photo_lighting's rules (include/texpose_amd.h, K40) in plain torch ops in fp64 on the tensors' device: the same arguments ->
    'light' [B,3,5] float32, 'count' [B] int32, 'rms' [B] float32, 'status', 'flags' [B] int32 and, with ``apply``, 'rgb' [B,H,W,3]
    float32 (a new tensor).  The sums run in torch's order, not the kernel's: counts, statuses and flags agree, the rest to rounding;
    'rgb' is the kernel's from the same light."""
    f64, f32 = torch.float64, torch.float32
    dev = zbuf.device
    B, H, W = zbuf.shape
    zf, c32, image = zbuf.float(), rgb.float(), image.float()
    image = image if image.dim() == 4 else image[None]
    fr = _gn_torch.frames_of(B, image.shape[0], frame, "image must hold 1 or B = %d photographs", dev)
    as_f32 = lambda v: float(torch.tensor(v, dtype=f32))
    tau, lo, hi, min_var = as_f32(tau), as_f32(gain_range[0]), as_f32(gain_range[1]), as_f32(min_var)
    l_in = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0], dtype=f32, device=dev).expand(B, 3, 5).contiguous() if light is None else light.float()
    nrm, valid = _pixel_normals_torch(verts, faces, face, pose)
    covered = (zf > 0) & torch.isfinite(zf)
    cand = covered.clone()
    cand[:, :1], cand[:, H - 1:], cand[:, :, :1], cand[:, :, W - 1:] = False, False, False, False
    cand = _gn_torch.masked(cand, mask, fr) & valid
    c, o = c32.to(f64), image[fr].to(f64)                                                   # [B,H,W,3]
    X = torch.stack([c, c * nrm[..., 0:1], c * nrm[..., 1:2], c * nrm[..., 2:3], torch.ones_like(c)], -1)       # [B,H,W,3,5]
    q = l_in.to(f64)[:, None, None]                                                         # [B,1,1,3,5]
    pred = (((q[..., 0] * X[..., 0] + q[..., 1] * X[..., 1]) + q[..., 2] * X[..., 2]) + q[..., 3] * X[..., 3]) + q[..., 4]
    res = o - pred
    keep = cand & torch.isfinite(c).all(-1) & torch.isfinite(o).all(-1) & ((res[..., 0] * res[..., 0] + res[..., 1] * res[..., 1])
                                                                          + res[..., 2] * res[..., 2] <= tau * tau)
    zero = torch.zeros((), dtype=f64, device=dev)
    total = lambda v: torch.where(keep.reshape(keep.shape + (1,) * (v.dim() - 3)), v, zero).flatten(1, 2).sum(1)
    n = keep.flatten(1).sum(1).to(f64)                                                      # [B]
    iu, ju = torch.triu_indices(5, 5, device=dev)
    A = torch.zeros(B, 3, 5, 5, dtype=f64, device=dev)
    A[:, :, iu, ju] = total(X[..., iu] * X[..., ju])
    A[:, :, ju, iu] = A[:, :, iu, ju]
    r, Soo = total(X * o[..., None]), total(o * o)                                          # [B,3,5], [B,3]
    L, passed = A.clone(), torch.ones(B, 3, dtype=torch.bool, device=dev)
    for j in range(5):                                                                      # K29's pivot rule
        diag = L[..., j, j]
        d = diag - (L[..., j, :j] * L[..., j, :j]).sum(-1)
        passed &= torch.isfinite(d) & (d > 1e-10 * diag) & (d > 0)
        lj = torch.sqrt(torch.where(passed, d, torch.ones_like(d)))
        L[..., j, j] = lj
        for i in range(j + 1, 5):
            L[..., i, j] = (L[..., i, j] - (L[..., i, :j] * L[..., j, :j]).sum(-1)) / lj
    L = torch.tril(L)
    y = torch.linalg.solve_triangular(L, r[..., None], upper=False)
    x = torch.linalg.solve_triangular(L.transpose(-1, -2), y, upper=True)[..., 0]           # [B,3,5]
    accepted = (passed & torch.isfinite(x).all(-1) & (x[..., 0] >= lo) & (x[..., 0] <= hi)
                & (torch.sqrt((x[..., 1] * x[..., 1] + x[..., 2] * x[..., 2]) + x[..., 3] * x[..., 3]) <= x[..., 0]))
    n1 = n[:, None]
    mc, mo = A[..., 0, 4] / n1, r[..., 4] / n1
    var, cov = A[..., 0, 0] / n1 - mc * mc, r[..., 0] / n1 - mc * mo
    live = var > min_var
    ratio = cov / torch.where(live, var, torch.ones_like(var))
    g = torch.where(live, ratio.clamp(lo, hi), torch.ones_like(ratio))
    closed = torch.stack([g, torch.zeros_like(g), torch.zeros_like(g), torch.zeros_like(g), mo - g * mc], -1)
    x = torch.where(accepted[..., None], x, closed)
    ch = torch.arange(3, device=dev)
    fell = ~accepted
    flags = ((fell.long() * 64 + (fell & live & (g != ratio)).long() + (fell & ~live).long() * 8) << ch).sum(1)
    dot5 = lambda u, w: (((u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]) + u[..., 3] * w[..., 3]) + u[..., 4] * w[..., 4]
    Ax = torch.stack([dot5(A[..., i, :], x) for i in range(5)], -1)
    sse = (Soo - 2.0 * dot5(x, r)) + dot5(x, Ax)
    rms = torch.sqrt(((sse[:, 0] + sse[:, 1]) + sse[:, 2]).clamp_min(0.0) / n).to(f32)
    x32 = x.to(f32)
    status = torch.where(n < _gn_torch.MIN_COUNT, 1, torch.where(torch.isfinite(x32).flatten(1).all(1) & torch.isfinite(rms), 0, 3)).to(torch.int32)
    out = dict(light=torch.where((status == 0)[:, None, None], x32, l_in), count=n.to(torch.int32), rms=rms, status=status, flags=flags.to(torch.int32))
    if apply:
        l = out["light"]
        w = l.to(f64)[:, None, None]
        s = ((w[..., 0] + w[..., 1] * nrm[..., 0:1]) + w[..., 2] * nrm[..., 1:2]) + w[..., 3] * nrm[..., 2:3]          # [B,H,W,3]
        s32 = torch.where(valid[..., None], s.to(f32), l[:, None, None, :, 0])
        lit = s32 * c32                                                                     # (two fp32 operations)
        out["rgb"] = torch.where(covered[..., None], lit + l[:, None, None, :, 4], c32)
    return out


def pyramid_torch(*, image: Optional[Tensor] = None, zbuf: Optional[Tensor] = None, rgb: Optional[Tensor] = None,
                  mask: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """ops.image_down / surface_down / mask_down's rules (include/texpose_amd.h, K38) in plain torch ops in fp64 on the tensors' device,
    one level down for whichever planes are given: ``image`` [N,H,W,3] -> 'image' [N,H//2,W//2,3]; ``zbuf`` [B,H,W] with ``rgb``
    [B,H,W,3] -> 'zbuf', 'rgb'; ``mask`` [N,H,W] -> 'mask' uint8.  The sums run in the header's order, every product is a torch op of
    its own and the weights are dyadic, so the float planes are the kernels' bit for bit (NaN payloads apart)."""
    f64 = torch.float64

    def taps(n, dev):                                                                       # [n // 2, 4], clamped
        return (2 * torch.arange(n // 2, device=dev)[:, None] - 1 + torch.arange(4, device=dev)[None, :]).clamp(0, n - 1)

    def gather(x):                                                                          # [N,H,W,C] -> [N,h,4 rows,w,4 columns,C]
        return x[:, taps(x.shape[1], x.device)][:, :, :, taps(x.shape[2], x.device)]

    def filtered(x):                                                                        # [N,H,W,C] float32 -> [N,h,w,C] float32
        t = gather(x.float().to(f64))
        w0, w1 = 0.125, 0.375
        s = ((w0 * t[:, :, :, :, 0] + w1 * t[:, :, :, :, 1]) + w1 * t[:, :, :, :, 2]) + w0 * t[:, :, :, :, 3]
        return (((w0 * s[:, :, 0] + w1 * s[:, :, 1]) + w1 * s[:, :, 2]) + w0 * s[:, :, 3]).float()

    out = {}
    if image is not None:
        out["image"] = filtered(image)
    if zbuf is not None:
        z = zbuf.float()
        surface = gather(((z > 0) & torch.isfinite(z))[..., None]).all(4).all(2)           # [N,h,w,1]
        out["zbuf"] = torch.where(surface[..., 0], filtered(z[..., None])[..., 0], torch.full((), -1.0, device=z.device))
        out["rgb"] = torch.where(surface, filtered(rgb), torch.zeros((), device=z.device))
    if mask is not None:
        out["mask"] = gather((mask != 0)[..., None]).all(4).all(2)[..., 0].to(torch.uint8)
    return out


class PhotoRefiner(_MeshRefiner):
    """Photometric alignment for batches of poses of one vertex-coloured mesh at H x W with the mesh on the device and a workspace per
    batch size.

    ``tau`` (one value or ``iters`` + 1 for a coarse-to-fine schedule; 0.5, in the colours' units), ``iters`` (Gauss-Newton steps, 10),
    ``damping`` (relative, 1e-6).  ``refine`` returns pose [B,3,4] ([R|t] model -> camera, mm), inliers [B] (interior covered pixels
    within tau of the photograph), rms [B] (colour units), status [B] (0 ok, 1 fewer than 6 kept pixels, 3 the last step's system was
    not positive definite: the pose went through unchanged) and inliers0 / rms0 of the start pose.  ``exposure``: every pass first fits
    the photograph's gain and bias per image and channel (ops.photo_exposure, K37) and ``refine`` also returns gain / bias [B,3] and
    exposure_status [B]; for photographs whose exposure, white balance or light differ from the colours'.  ``pyramid``: coarse to
    fine (ops.photo_align's ``pyramid``, K38): step counts per level, the coarsest first, adding up to ``iters``; inliers0 / rms0 are
    then the first pass's, at its own level.  ``lighting``: in place of ``exposure``, for a light with a direction: every pass first
    fits ambient + directional shading and a bias per image and channel on the faces' normals (ops.photo_lighting, K40) and ``refine``
    also returns light [B,3,5], lighting_status and lighting_flags [B]."""
    _new_workspace = staticmethod(ops.photo_align_workspace)

    def __init__(self, verts: Tensor, faces: Tensor, vcolor: Optional[Tensor], H: int, W: int, device="cuda:0", *, tau=0.5, iters: int = 10,
                 damping: float = 1e-6, cull: bool = False, texels: Optional[Tensor] = None, exposure: bool = False, exposure_tau0: float = 2.0,
                 pyramid=None, lighting: bool = False):
        if exposure and lighting:                                # (host arguments: refused before anything touches the device)
            raise ValueError("PhotoRefiner: exposure= and lighting= exclude each other (the lighting model contains the exposure's)")
        if pyramid is not None:
            ops.refine._pass_levels("PhotoRefiner", pyramid, int(iters))
        super().__init__(verts, faces, H, W, device, cull=cull)
        if (vcolor is None) == (texels is None):
            raise ValueError("PhotoRefiner: exactly one of vcolor [V,3] and texels= [F,T,3] (face texels, K35) expected")
        self._colours(vcolor, texels)
        self.tau, self.iters, self.damping = tau, int(iters), float(damping)
        self.exposure, self.exposure_tau0, self.lighting = bool(exposure), float(exposure_tau0), bool(lighting)
        self.pyramid = None if pyramid is None else tuple(pyramid)

    def refine(self, pose: Tensor, intr: Tensor, image: Tensor, frame: Optional[Tensor] = None, mask: Optional[Tensor] = None) -> AttrDict:
        """pose [B,3,4], intr [B,3,3] or [3,3], image [Ft,H,W,3] (channels last, the vertex colours' units), frame [B] int32 (the
        photograph of each pose; without it Ft is 1 or B), mask [Ft,H,W] uint8 / bool (0: do not use the pixel)."""
        image = image if image.dim() == 4 else image[None]
        if tuple(image.shape[1:]) != (self.H, self.W, 3):
            raise ValueError("PhotoRefiner.refine: photographs of %d x %d x 3 expected, got %s" % (self.H, self.W, tuple(image.shape)))
        return AttrDict(ops.photo_align(self.verts, self.faces, self.vcolor, pose, intr, image, tau=self.tau, iters=self.iters,
                                        damping=self.damping, frame=frame, mask=mask, workspace=self._workspace(pose.shape[0]), cull=self.cull,
                                        texels=self.texels, exposure=self.exposure, exposure_tau0=self.exposure_tau0, pyramid=self.pyramid,
                                        lighting=self.lighting))
