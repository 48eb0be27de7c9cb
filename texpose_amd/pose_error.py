"""Pose-error metrics: ADD, ADD-S, the BOP errors MSSD and MSPD, the mean projection error, rotation / translation error, the model
diameter and the one-directional chamfer distance `camera.p2p_distance` of the reference (camera.py:469-586, without normals).

CUDA tensors go through the project's kernels (K24 `tp_nn1`: the nearest / farthest neighbour search, K25 `tp_pose_errors`: the
fused per-pose reductions; csrc/pose_error.hip).  CPU tensors run the same definitions in plain torch ops in the tensors' own dtype,
chunked so that no block above ~64 MB is formed -- that route is also the yardstick the kernels are measured against
(tools/pose_error_bench.py runs it on the device).  Nothing here is differentiable: inputs are detached.

The BOP definitions and `p2p_distance` are RESTATED (tests/pose_error_ref.py says them again in numpy fp64): neither bop_toolkit nor
PyTorch3D is a dependency, and nothing is pinned to a call of either.  Rules and what is pinned to what: DESIGN.md section 15.

The third BOP error, the Visible Surface Discrepancy, and the BOP average recall are at the end of this file: `vsd` renders the model
at both poses (K19 `tp_mesh_raster`) and `vsd_from_depth` turns the two renders and the measured depth into errors (K26 `tp_vsd` on
CUDA tensors, `vsd_torch` on CPU tensors; restated in tests/vsd_ref.py).  Rules and what is pinned to what: DESIGN.md section 16.

Poses are [B,3,4] = [R|t], model -> camera, t in the model's unit (mm for BOP models); a single [3,4] pose is taken as B = 1."""
from __future__ import annotations

import math
import warnings
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import geometry

Tensor = torch.Tensor
CHUNK_BYTES = 64 << 20          # the largest intermediate block of the torch route
MAX_SYM = 64                    # tp_pose_errors takes at most this many symmetry transforms (TP_POSE_ERRORS_MAX_SYM)
BOP19_TAUS = tuple(round(0.05 * i, 2) for i in range(1, 11))               # VSD's misalignment tolerances, fractions of the diameter
BOP19_THRESHOLDS = tuple(round(0.05 * i, 2) for i in range(1, 11))         # the thresholds of correctness of VSD and (x diameter) MSSD
BOP19_MSPD_PX = tuple(range(5, 51, 5))                                     # MSPD's thresholds in pixels of a 640-pixel-wide image


def _poses(p: Tensor, name: str) -> Tensor:
    p = p.detach()
    if p.dim() == 2:
        p = p[None]
    if p.dim() != 3 or tuple(p.shape[1:]) != (3, 4):
        raise ValueError("%s: [B,3,4] expected, got %s" % (name, tuple(p.shape)))
    return p


def _points(pts: Tensor) -> Tensor:
    pts = pts.detach()
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] == 0:
        raise ValueError("pts: [M,3] expected, got %s" % (tuple(pts.shape),))
    return pts


# ----------------------------------------------------------------------------- the search
def nn1_torch(x: Tensor, y: Tensor, x_len: Optional[Tensor] = None, y_len: Optional[Tensor] = None, A: Optional[Tensor] = None,
              mode: str = "nearest") -> Tuple[Tensor, Tensor]:
    """ops.nn1's rules in plain torch ops on x's device and in x's dtype: `(q[:, :, None] - y[:, None]).square().sum(-1)` and its
    min / max over the targets, in chunks of queries.  -> (d2 [B,P1], idx [B,P1] int32)."""
    far = {"nearest": False, "farthest": True}[mode]
    B, P1, P2 = (x.shape[0] if A is None else A.shape[0]), x.shape[1], y.shape[1]
    q = x if A is None else x @ A[:, :, :3].to(x.dtype).transpose(1, 2) + A[:, None, :, 3].to(x.dtype)
    none = -math.inf if far else math.inf
    d2 = torch.full((B, P1), none, dtype=x.dtype, device=x.device)
    idx = torch.full((B, P1), -1, dtype=torch.int32, device=x.device)
    absent = None if y_len is None else torch.arange(P2, device=x.device)[None, None] >= y_len.view(-1, 1, 1)       # [Bt,1,P2]
    step = max(1, CHUNK_BYTES // (B * P2 * 3 * x.element_size()))
    for i0 in range(0, P1, step):
        d = (q[:, i0:i0 + step, None] - y[:, None]).square().sum(-1)                                   # [B,c,P2]
        lost = torch.isnan(d) if absent is None else torch.isnan(d) | absent
        d = torch.where(lost, torch.full_like(d, none), d)
        v, j = d.max(-1) if far else d.min(-1)                                                         # (the first of equal values)
        won = ~lost.all(-1)
        if x_len is not None:
            won &= torch.arange(i0, i0 + d.shape[1], device=x.device)[None] < x_len.view(-1, 1)
        d2[:, i0:i0 + step] = torch.where(won, v, torch.full_like(v, none))
        idx[:, i0:i0 + step] = torch.where(won, j, torch.full_like(j, -1)).to(torch.int32)
    return d2, idx


def nn1(x: Tensor, y: Tensor, x_len: Optional[Tensor] = None, y_len: Optional[Tensor] = None, A: Optional[Tensor] = None,
        mode: str = "nearest") -> Tuple[Tensor, Tensor]:
    """The nearest (farthest) target of every query: K24 on CUDA tensors, `nn1_torch` on CPU tensors.  Shapes and rules: ops.nn1."""
    x, y = x.detach(), y.detach()
    if x.is_cuda:
        from . import ops
        i32 = lambda t: None if t is None else t.to(device=x.device, dtype=torch.int32)
        return ops.nn1(x, y, x_len=i32(x_len), y_len=i32(y_len), A=A, mode=mode)
    return nn1_torch(x, y, x_len, y_len, None if A is None else A.detach(), mode)


def relative_pose(pose_est: Tensor, pose_gt: Tensor) -> Tensor:
    """A = P_g^-1 o P_e per b, [B,3,4] in fp64 (a few tiny element-wise ops: the 3 x 3 inverse by cofactors, no solver call)."""
    e, g = pose_est.double(), pose_gt.double()
    r0, r1, r2 = g[:, 0, :3], g[:, 1, :3], g[:, 2, :3]
    c0, c1, c2 = torch.cross(r1, r2, dim=-1), torch.cross(r2, r0, dim=-1), torch.cross(r0, r1, dim=-1)
    inv = torch.stack([c0, c1, c2], dim=-1) / (r0 * c0).sum(-1)[:, None, None]                         # columns / determinant
    rel = torch.cat([e[:, :, :3], e[:, :, 3:] - g[:, :, 3:]], dim=-1)
    return (inv[:, :, :, None] * rel[:, None]).sum(2)                                                  # inv @ rel, element-wise


def adds(pts: Tensor, pose_est: Tensor, pose_gt: Tensor) -> Tensor:
    """ADD-S [B]: mean_x min_y |P_e x - P_g y| = mean_x min_y |P_g^-1 P_e x - y| -- one search of the posed model against the model
    itself, the target set shared by every b."""
    pts, pose_est, pose_gt = _points(pts), _poses(pose_est, "pose_est"), _poses(pose_gt, "pose_gt")
    A = relative_pose(pose_est, pose_gt).to(pts.dtype)
    d2, _ = nn1(pts[None], pts[None], A=A)
    return d2.sqrt().mean(-1)


def model_diameter(pts: Tensor) -> Tensor:
    """The largest distance between two model points (0-dim): one farthest-neighbour search of the set against itself."""
    pts = _points(pts)
    d2, _ = nn1(pts[None], pts[None], mode="farthest")
    return d2.max().sqrt()


# ----------------------------------------------------------------------------- the fused reductions
def _project(X: Tensor, K: Tensor) -> Tensor:
    """pi(X) = (fx X / Z + cx, fy Y / Z + cy) for X [b,...,3] and K [b,3,3]."""
    k = lambda r, c: K[:, r, c].view(-1, *[1] * (X.dim() - 2))
    return torch.stack([k(0, 0) * X[..., 0] / X[..., 2] + k(0, 2), k(1, 1) * X[..., 1] / X[..., 2] + k(1, 2)], -1)


def pose_errors_torch(pts: Tensor, pose_est: Tensor, pose_gt: Tensor, sym: Tensor, intr: Optional[Tensor]) -> Dict[str, Tensor]:
    """ops.pose_errors' rules in plain torch ops in pts' dtype, in chunks of poses."""
    M, B, S = pts.shape[0], pose_est.shape[0], sym.shape[0]
    dt = pts.dtype
    pose_est, pose_gt, sym = pose_est.to(dt), pose_gt.to(dt), sym.to(dt)
    moved = pts @ sym[:, :, :3].transpose(1, 2) + sym[:, None, :, 3]                                     # [S,M,3]: S_s x
    res = {k: torch.empty(B, dtype=dt, device=pts.device) for k in ("add", "mssd") + (("mspd", "proj") if intr is not None else ())}
    res.update({k: torch.empty(B, dtype=torch.int32, device=pts.device) for k in ("s_mssd",) + (("s_mspd",) if intr is not None else ())})
    step = max(1, CHUNK_BYTES // (S * M * 3 * pts.element_size()))
    for b0 in range(0, B, step):
        sl = slice(b0, b0 + step)
        e = pts @ pose_est[sl, :, :3].transpose(1, 2) + pose_est[sl, None, :, 3]                          # [b,M,3]
        g = moved[None] @ pose_gt[sl, None, :, :3].transpose(2, 3) + pose_gt[sl, None, None, :, 3]         # [b,S,M,3]
        d3 = (e[:, None] - g).square().sum(-1).sqrt()                                                   # [b,S,M]
        res["add"][sl] = d3[:, 0].mean(-1)
        v, s = d3.max(-1).values.min(-1)
        res["mssd"][sl], res["s_mssd"][sl] = v, s.to(torch.int32)
        if intr is not None:
            K = intr[sl].to(dt)
            d2 = (_project(e, K)[:, None] - _project(g, K)).square().sum(-1).sqrt()                     # [b,S,M]
            bad = ~((e[..., 2] > 0).all(-1) & (g[..., 2] > 0).all(-1).all(-1))                           # [b]
            nan = torch.full_like(d2[:, 0, 0], math.nan)
            v, s = d2.max(-1).values.min(-1)
            res["mspd"][sl], res["s_mspd"][sl] = torch.where(bad, nan, v), torch.where(bad, torch.full_like(s, -1), s).to(torch.int32)
            res["proj"][sl] = torch.where(bad, nan, d2[:, 0].mean(-1))
    return res


def symmetry_identity(like: Tensor) -> Tensor:
    return torch.eye(3, 4, dtype=like.dtype, device=like.device)[None]


def pose_errors(pts: Tensor, pose_est: Tensor, pose_gt: Tensor, sym: Optional[Tensor] = None, intr: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """Every search-free error from one K25 call: 'add' = mean_x |P_e x - P_g x|, 'mssd' = min_s max_x |P_e x - P_g S_s x| with
    's_mssd' the winning symmetry (lowest index on ties) and, with ``intr`` [B,3,3] (or one [3,3]), 'mspd' = min_s max_x |pi(P_e x) -
    pi(P_g S_s x)|, 'proj' = mean_x |pi(P_e x) - pi(P_g x)| and 's_mspd', pi(X) = (fx X / Z + cx, fy Y / Z + cy).  All [B].
    ``sym`` [S,3,4]: `symmetry_transforms`' output, row 0 the identity (None: the identity alone).  A point at Z <= 0 under either pose
    makes the pixel terms of that b NaN (s_mspd -1); add and mssd are unaffected."""
    pts, pose_est, pose_gt = _points(pts), _poses(pose_est, "pose_est"), _poses(pose_gt, "pose_gt")
    if pose_est.shape != pose_gt.shape:
        raise ValueError("pose_est and pose_gt: the same number of poses expected")
    sym = symmetry_identity(pts) if sym is None else sym.detach()
    if sym.dim() != 3 or tuple(sym.shape[1:]) != (3, 4) or sym.shape[0] == 0:
        raise ValueError("sym: [S,3,4] expected, got %s" % (tuple(sym.shape),))
    if intr is not None:
        intr = intr.detach()
        intr = intr[None].expand(pose_est.shape[0], -1, -1) if intr.dim() == 2 else intr
    if pts.is_cuda:
        from . import ops
        return ops.pose_errors(pts, pose_est, pose_gt, sym.to(pts.device), None if intr is None else intr.contiguous())
    return pose_errors_torch(pts, pose_est, pose_gt, sym, intr)


def add(pts: Tensor, pose_est: Tensor, pose_gt: Tensor) -> Tensor:
    """ADD [B]: the mean distance between the model points under the two poses."""
    return pose_errors(pts, pose_est, pose_gt)["add"]


def mssd(pts: Tensor, pose_est: Tensor, pose_gt: Tensor, sym: Optional[Tensor] = None) -> Tensor:
    """BOP's maximum symmetry-aware surface distance [B]."""
    return pose_errors(pts, pose_est, pose_gt, sym)["mssd"]


def mspd(pts: Tensor, pose_est: Tensor, pose_gt: Tensor, intr: Tensor, sym: Optional[Tensor] = None) -> Tensor:
    """BOP's maximum symmetry-aware projection distance [B], pixels."""
    return pose_errors(pts, pose_est, pose_gt, sym, intr)["mspd"]


def proj(pts: Tensor, pose_est: Tensor, pose_gt: Tensor, intr: Tensor) -> Tensor:
    """The mean 2-D projection error [B], pixels (the '5 px' metric's error)."""
    return pose_errors(pts, pose_est, pose_gt, None, intr)["proj"]


def re_te(pose_est: Tensor, pose_gt: Tensor) -> Tuple[Tensor, Tensor]:
    """(rotation error [B] in radians -- geometry.rotation_distance, the geodesic angle --, translation error [B] = |t_e - t_g|)."""
    pose_est, pose_gt = _poses(pose_est, "pose_est"), _poses(pose_gt, "pose_gt")
    return (geometry.rotation_distance(pose_est[:, :, :3], pose_gt[:, :, :3]),
            (pose_est[:, :, 3] - pose_gt[:, :, 3]).square().sum(-1).sqrt())


# ----------------------------------------------------------------------------- camera.p2p_distance
def p2p_distance(x: Tensor, y: Tensor, x_lengths: Optional[Tensor] = None, y_lengths: Optional[Tensor] = None, x_normals=None,
                 y_normals=None, weights: Optional[Tensor] = None, batch_reduction: Optional[str] = "mean", point_reduction: str = "mean"):
    """The reference's `camera.p2p_distance` without normals: the one-directional chamfer term from x [N,P1,3] to y [N,P2,3] -- per
    cloud the sum (``point_reduction`` 'sum') or mean over its x_lengths points ('mean') of the SQUARED distance to the nearest of its
    y_lengths targets, times weights [N]; then over the batch the sum, the mean (divided by the weights' sum, or by N) or, with
    ``batch_reduction`` None, nothing.  Entries past the lengths count as zero; weights that sum to zero return zeros at once.  As in
    the reference, 'mean' divides by x_lengths unguarded: a cloud of length 0 gives NaN there (0 under 'sum').
    -> (cham_x, None).  NOT differentiable (the search is a kernel without a backward): the result is detached."""
    if x_normals is not None or y_normals is not None:
        raise NotImplementedError("p2p_distance: normals are not supported")
    if batch_reduction not in ("mean", "sum", None) or point_reduction not in ("mean", "sum"):
        raise ValueError("p2p_distance: batch_reduction must be 'mean', 'sum' or None and point_reduction 'mean' or 'sum'")
    x, y = x.detach(), y.detach()
    if x.dim() != 3 or y.dim() != 3 or x.shape[2] != 3 or y.shape[0] != x.shape[0] or y.shape[2] != 3:
        raise ValueError("p2p_distance: x [N,P1,3] and y [N,P2,3] expected, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    N, P1 = x.shape[0], x.shape[1]
    if weights is not None:
        weights = weights.detach().to(x.dtype)
        if weights.shape != (N,):
            raise ValueError("p2p_distance: weights must be of shape (N,)")
        if not bool((weights >= 0).all()):
            raise ValueError("p2p_distance: weights cannot be negative")
        if float(weights.sum()) == 0.0:
            zero = x.new_zeros(()) if batch_reduction is not None else x.new_zeros(N)
            return zero, None
    count = x.new_full((N,), float(P1)) if x_lengths is None else x_lengths.to(x.dtype)
    d2, _ = nn1(x, y, x_lengths, y_lengths)
    if x_lengths is not None:
        d2 = torch.where(torch.arange(P1, device=x.device)[None] < x_lengths.view(-1, 1), d2, torch.zeros_like(d2))
    if weights is not None:
        d2 = d2 * weights[:, None]
    cham = d2.sum(1)
    if point_reduction == "mean":
        cham = cham / count
    if batch_reduction is not None:
        cham = cham.sum()
        if batch_reduction == "mean":
            cham = cham / (weights.sum() if weights is not None else N)
    return cham, None


# ----------------------------------------------------------------------------- host helpers
def _axis_rotation(axis, angle: float) -> torch.Tensor:
    k = torch.as_tensor(axis, dtype=torch.float64)
    k = k / k.norm()
    Kx = torch.tensor([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * (Kx @ Kx)      # Rodrigues


def symmetry_transforms(models_info_entry: dict, max_sym_disc_step: float = 0.01, diameter: Optional[float] = None) -> torch.Tensor:
    """The symmetry set [S,3,4] (float64, host) of one models_info.json entry, as the BOP toolkit documents it: the identity, then
    `symmetries_discrete` (16 row-major floats each, a 4 x 4 transform), each combined with every step of every `symmetries_continuous`
    entry: n = ceil(pi / max_sym_disc_step) rotations by 2 pi i / n about the axis through `offset` (x -> R (x - o) + o).  The step is
    a fraction of the diameter a surface point may move, pi d / (step d): ``diameter`` cancels and is accepted for the record only.
    Order: continuous steps outermost, so rows 0 .. D are the identity and the discrete transforms.  More than 64 transforms (the
    kernel's limit) are subsampled evenly, row 0 kept, with a warning."""
    eye = torch.eye(4, dtype=torch.float64)
    disc = [eye] + [torch.tensor(s, dtype=torch.float64).reshape(4, 4) for s in models_info_entry.get("symmetries_discrete", [])]
    cont = [eye]
    n = int(math.ceil(math.pi / float(max_sym_disc_step)))
    for entry in models_info_entry.get("symmetries_continuous", []):
        o = torch.tensor(entry["offset"], dtype=torch.float64).reshape(3)
        steps = []
        for i in range(n):
            T = torch.eye(4, dtype=torch.float64)
            T[:3, :3] = _axis_rotation(entry["axis"], 2.0 * math.pi * i / n) if i else torch.eye(3, dtype=torch.float64)
            T[:3, 3] = o - T[:3, :3] @ o
            steps.append(T)
        cont = [c @ s for c in cont for s in steps]
    out = torch.stack([c @ d for c in cont for d in disc])[:, :3]
    if out.shape[0] > MAX_SYM:
        keep = [int(i * out.shape[0] / MAX_SYM) for i in range(MAX_SYM)]
        warnings.warn("symmetry_transforms: %d transforms subsampled evenly to %d" % (out.shape[0], MAX_SYM))
        out = out[keep]
    return out.contiguous()


def _host_list(v) -> list:
    return [float(e) for e in (v.detach().reshape(-1).tolist() if torch.is_tensor(v) else (list(v) if hasattr(v, "__iter__") else [v]))]


def recall(errors, thresholds):
    """The share of ``errors`` strictly below each threshold (a NaN error never passes): a float for one threshold, else a list."""
    e = _host_list(errors)
    one = thresholds.dim() == 0 if torch.is_tensor(thresholds) else not hasattr(thresholds, "__iter__")
    r = [sum(1 for v in e if v < t) / len(e) if e else math.nan for t in _host_list(thresholds)]
    return r[0] if one else r


def auc(errors, max_threshold: float) -> float:
    """The area under the recall-over-threshold curve on [0, max_threshold], divided by max_threshold: the mean of
    max(0, 1 - e / max_threshold), exactly (a NaN error contributes 0)."""
    e = _host_list(errors)
    T = float(max_threshold)
    return sum(max(0.0, 1.0 - v / T) for v in e if v == v) / len(e) if e else math.nan


# ----------------------------------------------------------------------------- VSD and the BOP average recall
def depth_from_png(depth16: Tensor, depth_scale: float) -> Tensor:
    """A scene folder's 16-bit depth image(s) -> float32 mm on the input's device: png * depth_scale (bop_scene.read_bop_frame's
    'depth' and 'depth_scale'; a numpy uint16 array is accepted); 0 stays 0, "no measurement"."""
    if not torch.is_tensor(depth16):
        import numpy as np
        depth16 = torch.from_numpy(np.ascontiguousarray(depth16).astype(np.int32))
    return depth16.detach().to(torch.float32) * float(depth_scale)


def vsd_torch(z_est: Tensor, z_gt: Tensor, depth_test: Tensor, intr: Tensor, tau_mm: Tensor, delta_mm: float = 15.0,
              frame: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """ops.vsd's rules (include/texpose_amd.h, K26) in plain torch ops in fp64 on the tensors' device: z_est, z_gt [B,H,W],
    depth_test [Ft,H,W] (Ft 1 or B, or indexed by ``frame`` [B], clamped into range), intr [B,3,3], tau_mm [B,T]
    -> {'err' [B,T] float32, 'counts' [B,2+T] int32}."""
    B, H, W = z_est.shape
    dev = z_est.device
    if frame is not None:
        depth_test = depth_test[frame.to(device=dev, dtype=torch.int64).clamp(0, depth_test.shape[0] - 1)]
    elif depth_test.shape[0] not in (1, B):
        raise ValueError("vsd: depth_test must hold 1 or B = %d planes without frame=, got %d" % (B, depth_test.shape[0]))
    K = intr.double()
    j = torch.arange(W, device=dev, dtype=torch.float64)[None, None, :]
    i = torch.arange(H, device=dev, dtype=torch.float64)[None, :, None]
    k = lambda r, c: K[:, r, c].view(B, 1, 1)
    u, v = ((j + 0.5) - k(0, 2)) / k(0, 0), ((i + 0.5) - k(1, 2)) / k(1, 1)
    f = ((u * u + v * v) + 1.0).sqrt()
    ok_e, ok_g, missing = z_est > 0, z_gt > 0, ~(depth_test > 0)
    D_e, D_g, D_t = z_est.double() * f, z_gt.double() * f, depth_test.double() * f
    delta = float(torch.tensor(delta_mm, dtype=torch.float32))              # (the kernel takes it as fp32)
    vis_g = ok_g & (missing | (D_g - D_t <= delta))
    vis_e = ok_e & (missing | (D_e - D_t <= delta) | vis_g)
    inter = vis_g & vis_e
    diff = (D_g - D_e).abs()
    n_u, n_i = (vis_g | vis_e).sum((1, 2)), inter.sum((1, 2))
    c = torch.stack([(inter & (diff >= tau_mm[:, t].double().view(B, 1, 1))).sum((1, 2)) for t in range(tau_mm.shape[1])], 1)      # [B,T]
    err = torch.where(n_u[:, None] > 0, (c + (n_u - n_i)[:, None]).double() / n_u.clamp(min=1)[:, None].double(),
                      torch.ones((), dtype=torch.float64, device=dev))
    return dict(err=err.float(), counts=torch.cat([n_u[:, None], n_i[:, None], c], 1).to(torch.int32))


def vsd_from_depth(z_est: Tensor, z_gt: Tensor, depth_test: Tensor, intr: Tensor, diameter, *, taus: Sequence[float] = BOP19_TAUS,
                   delta: float = 15.0, frame: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """BOP's Visible Surface Discrepancy (cost 'step', visibility 'bop19') from depth planes: z_est, z_gt [B,H,W] the model's
    view-space depth in mm at the estimated and the true pose (<= 0 or NaN on background: ops.mesh_raster's zbuf), depth_test
    [Ft,H,W] the measured depth in mm (0: no value; Ft 1 or B, or indexed by ``frame`` [B]), intr [B,3,3] or [3,3], ``diameter``
    a float or a [B] tensor, ``taus`` at most 16 fractions of it, ``delta`` the visibility tolerance in mm
    -> 'err' [B,T] float32 in [0, 1] and 'counts' [B,2+T] int32 (n_U, n_I, c_t).  tau_mm = taus x diameter is formed on the tensors'
    device; nothing is read back.  CUDA tensors: K26 (ops.vsd); CPU tensors: `vsd_torch`."""
    z_est, z_gt, depth_test, intr = z_est.detach(), z_gt.detach(), depth_test.detach(), intr.detach()
    if z_est.dim() != 3 or z_gt.shape != z_est.shape or depth_test.dim() != 3 or depth_test.shape[1:] != z_est.shape[1:]:
        raise ValueError("vsd: z_est, z_gt [B,H,W] and depth_test [Ft,H,W] expected, got %s, %s and %s"
                         % (tuple(z_est.shape), tuple(z_gt.shape), tuple(depth_test.shape)))
    B, dev = z_est.shape[0], z_est.device
    if not 1 <= len(taus) <= 16:
        raise ValueError("vsd: 1 .. 16 taus expected, got %d" % len(taus))
    d = diameter.detach().to(device=dev, dtype=torch.float32).reshape(-1) if torch.is_tensor(diameter) else \
        torch.full((1,), float(diameter), dtype=torch.float32, device=dev)
    if d.numel() not in (1, B):
        raise ValueError("vsd: diameter must be a number or a [B] tensor")
    tau_mm = (torch.tensor([float(t) for t in taus], dtype=torch.float32, device=dev)[None] * d[:, None]).expand(B, -1).contiguous()
    if z_est.is_cuda:
        from . import ops
        return ops.vsd(z_est, z_gt, depth_test.to(dev), intr.to(dev), tau_mm, delta_mm=delta,
                       frame=None if frame is None else frame.to(device=dev, dtype=torch.int32))
    return vsd_torch(z_est, z_gt, depth_test, intr[None].expand(B, -1, -1) if intr.dim() == 2 else intr, tau_mm, delta, frame)


def vsd(verts: Tensor, faces: Tensor, pose_est: Tensor, pose_gt: Tensor, intr: Tensor, depth_test: Tensor, diameter, *, H: int, W: int,
        taus: Sequence[float] = BOP19_TAUS, delta: float = 15.0, frame: Optional[Tensor] = None, cull: bool = False) -> Dict[str, Tensor]:
    """VSD of B pose pairs of one mesh: ONE ops.mesh_raster call renders the 2 B stacked poses (depth only), `vsd_from_depth` does the
    rest.  verts [V,3] (mm), faces [F,3], pose_est / pose_gt [B,3,4] (t in mm), intr [B,3,3] or [3,3]; the other arguments are
    `vsd_from_depth`'s.  ``cull``: render with ops.mesh_raster(cull=True) (K34), the same depth bit for bit.  GPU only: the rasteriser
    has no CPU route."""
    pose_est, pose_gt = _poses(pose_est, "pose_est"), _poses(pose_gt, "pose_gt")
    if pose_est.shape != pose_gt.shape:
        raise ValueError("pose_est and pose_gt: the same number of poses expected")
    if not verts.is_cuda:
        raise ValueError("vsd: the mesh is rendered by the HIP rasteriser, which has no CPU route; pass CUDA tensors "
                         "(depth planes rendered elsewhere can be scored on the CPU with vsd_from_depth)")
    from . import ops
    B = pose_est.shape[0]
    intr = intr.detach()
    z = ops.mesh_raster(verts.detach(), faces, torch.cat([pose_est, pose_gt]).to(verts.device),
                        (intr if intr.dim() == 2 else torch.cat([intr, intr])).to(verts.device), H=H, W=W, face_ids=False, normals=False,
                        cull=cull)["zbuf"]
    return vsd_from_depth(z[:B], z[B:], depth_test, intr, diameter, taus=taus, delta=delta, frame=frame)


def average_recall(vsd_err, mssd, mspd, diameter, width: int, valid=None) -> Dict[str, float]:
    """The BOP average recall over G ground-truth instances: vsd_err [G,T] (`vsd`'s 'err'), mssd [G], mspd [G], diameter [G] (or one
    number), ``width`` the image width in pixels, valid [G] (False: the instance has no estimate) ->
      ar_vsd  = mean over T x BOP19_THRESHOLDS of the share of instances with err < theta,
      ar_mssd = mean over BOP19_THRESHOLDS of the share with mssd < theta x diameter,
      ar_mspd = mean over r in 5, 10 .. 50 of the share with mspd < r x width / 640,
      ar      = their mean.
    An instance without an estimate, or with a NaN error, is a miss.  Host-side, like `recall`."""
    rows = vsd_err.detach().double().cpu().tolist() if torch.is_tensor(vsd_err) else [[float(x) for x in r] for r in vsd_err]
    ms, mp = _host_list(mssd), _host_list(mspd)
    G = len(rows)
    d = _host_list(diameter)
    d = d * G if len(d) == 1 else d
    ok = [True] * G if valid is None else [bool(x) for x in (valid.detach().reshape(-1).tolist() if torch.is_tensor(valid) else valid)]
    if not (len(ms) == len(mp) == len(d) == len(ok) == G):
        raise ValueError("average_recall: vsd_err [G,T], mssd, mspd, diameter and valid [G] expected")
    if G == 0:
        return dict(ar_vsd=math.nan, ar_mssd=math.nan, ar_mspd=math.nan, ar=math.nan)
    T = len(rows[0])
    hits = sum(1 for g in range(G) if ok[g] for e in rows[g] for th in BOP19_THRESHOLDS if e < th)
    ar_vsd = hits / (G * T * len(BOP19_THRESHOLDS))
    ar_mssd = sum(1 for g in range(G) if ok[g] for th in BOP19_THRESHOLDS if ms[g] < th * d[g]) / (G * len(BOP19_THRESHOLDS))
    ar_mspd = sum(1 for g in range(G) if ok[g] for r in BOP19_MSPD_PX if mp[g] < r * width / 640.0) / (G * len(BOP19_MSPD_PX))
    return dict(ar_vsd=ar_vsd, ar_mssd=ar_mssd, ar_mspd=ar_mspd, ar=(ar_vsd + ar_mssd + ar_mspd) / 3.0)
