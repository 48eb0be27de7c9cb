"""K24-K26, K28: nearest neighbours, the pose errors, VSD and PnP-RANSAC.  (The render-and-compare refiners, K29-K33, are in refine.py.)"""
from typing import Dict, Optional

import torch

from .. import _lib
from ._base import Tensor, _call, _f32, _float3, _intr_per_view, _lengths, _on_tensor_device, _outputs, _points, _poses, _ptr, _want_gpu, _workspace_arg

__all__ = ["NN1_MODES", "nn1", "pose_errors", "vsd", "PNP_MAX_HYP", "PNP_MAX_ITERS", "pnp_workspace", "_pnp_common", "corr_from_nocs",
           "pnp_hypotheses", "pnp_score", "pnp_refine", "PNP_RANSAC_KEYS", "pnp_ransac"]

# ------------------------------------------------------------------------------------------ K24, K25
NN1_MODES = {"nearest": _lib.NN1_NEAREST, "farthest": _lib.NN1_FARTHEST}


@_on_tensor_device
def nn1(x: Tensor, y: Tensor, *, x_len: Optional[Tensor] = None, y_len: Optional[Tensor] = None, A: Optional[Tensor] = None,
        mode: str = "nearest", target_slices: int = 0):
    """Brute-force 1-nearest (``mode`` 'farthest': 1-farthest) neighbour in 3-D (tp_nn1): queries x [Bx,P1,3], targets y [Bt,P2,3] with
    Bx, Bt 1 (shared by every b) or B (B: A's batch size, else x's), optional int32 lengths x_len [B] / y_len [Bt] for ragged sets, optional A [B,3,4] applied to the
    queries in registers (q = A[:, :3] x + A[:, 3]; evaluated before A's translation, which is taken off the targets) -> (d2 [B,P1] float32, idx [B,P1] int32): the squared distance in the direct form
    and the winner's index, the lowest on equal d2; +inf (-inf for 'farthest') and -1 where there is no winner (a NaN query, a query
    past x_len, no target).  ``target_slices``: 0 lets the library split the targets over workgroups from the shapes; the result does
    not depend on it.  Not differentiable.  No allocation beyond the outputs and the split's key buffer, safe under torch.cuda.graph."""
    if mode not in NN1_MODES:
        raise ValueError(f"nn1: mode must be one of {sorted(NN1_MODES)}, not {mode!r}")
    x, y = _f32(x.detach(), "x"), _f32(y.detach(), "y")
    if x.dim() != 3 or y.dim() != 3 or x.shape[2] != 3 or y.shape[2] != 3 or x.shape[1] == 0 or y.shape[1] == 0 or x.shape[0] == 0:
        raise ValueError("nn1: x [Bx,P1,3] and y [Bt,P2,3] expected, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
    Bx, P1, Bt, P2 = x.shape[0], x.shape[1], y.shape[0], y.shape[1]
    B = Bx if A is None else A.shape[0]
    if Bx not in (1, B) or Bt not in (1, B):
        raise ValueError("nn1: x and y must hold 1 or B = %d sets, got %d and %d" % (B, Bx, Bt))
    x_len, y_len = _lengths("nn1", x_len, "x_len", B, x), _lengths("nn1", y_len, "y_len", Bt, x)
    a = _lib.Nn1Args()
    if A is not None:
        A = _poses("nn1", A, "A", B)
        a.A = A.data_ptr()
    d2 = torch.empty(B, P1, device=x.device)
    idx = torch.empty(B, P1, device=x.device, dtype=torch.int32)
    a.x, a.y, a.x_len, a.y_len = x.data_ptr(), y.data_ptr(), _ptr(x_len), _ptr(y_len)
    a.B, a.Bx, a.Bt, a.P1, a.P2, a.mode, a.target_slices = B, Bx, Bt, P1, P2, NN1_MODES[mode], int(target_slices)
    a.d2, a.idx = d2.data_ptr(), idx.data_ptr()
    n_ws = _lib.load().tp_nn1_workspace_bytes(a)
    ws = torch.empty(n_ws // 8, device=x.device, dtype=torch.int64) if n_ws else None
    a.workspace = _ptr(ws)
    _call("tp_nn1", a)
    return d2, idx


@_on_tensor_device
def pose_errors(pts: Tensor, pose_est: Tensor, pose_gt: Tensor, sym: Optional[Tensor] = None, intr: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """ADD, MSSD, MSPD and the mean projection error of B pose pairs over one model (tp_pose_errors): pts [M,3], pose_est / pose_gt
    [B,3,4], sym [S,3,4] (row 0 the identity; None: the identity alone; at most 64), intr [B,3,3] or None -> 'add', 'mssd' [B] float32
    and 's_mssd' [B] int32 (the winning symmetry, the lowest on ties) and, with ``intr``, 'mspd', 'proj' and 's_mspd' (pixels; NaN /
    -1 for a b with a point at Z <= 0 under either pose).  Not differentiable.  Two launches, safe under torch.cuda.graph."""
    pts, pose_est = _points("pose_errors", pts, "pts"), _poses("pose_errors", pose_est, "pose_est")
    M, B = pts.shape[0], pose_est.shape[0]
    pose_gt = _poses("pose_errors", pose_gt, "pose_gt", B)
    if sym is None:
        sym = torch.eye(3, 4, device=pts.device)[None]
    sym = _f32(sym.detach(), "sym")
    if sym.dim() != 3 or tuple(sym.shape[1:]) != (3, 4) or sym.shape[0] == 0:
        raise ValueError("pose_errors: sym [S,3,4] expected, got %s" % (tuple(sym.shape),))
    S = sym.shape[0]
    a = _lib.PoseErrorsArgs()
    if intr is not None:
        intr = _intr_per_view("pose_errors", intr, B, allow_single=False)
        a.intr = intr.data_ptr()
    out = torch.empty(B, 4, device=pts.device)
    s_out = torch.empty(2, B, device=pts.device, dtype=torch.int32)
    ws = torch.empty(B * min(S, _lib.POSE_ERRORS_MAX_SYM) * 4, device=pts.device, dtype=torch.float64)
    a.pts, a.pose_est, a.pose_gt, a.sym = pts.data_ptr(), pose_est.data_ptr(), pose_gt.data_ptr(), sym.data_ptr()
    a.M, a.B, a.S = M, B, S
    a.out, a.s_mssd, a.s_mspd, a.workspace = out.data_ptr(), s_out[0].data_ptr(), s_out[1].data_ptr(), ws.data_ptr()
    _call("tp_pose_errors", a)          # (S > 64: the library's error)
    res = dict(add=out[:, 0], mssd=out[:, 1], s_mssd=s_out[0])
    if intr is not None:
        res.update(mspd=out[:, 2], proj=out[:, 3], s_mspd=s_out[1])
    return res


# ------------------------------------------------------------------------------------------ K26
@_on_tensor_device
def vsd(z_est: Tensor, z_gt: Tensor, depth_test: Tensor, intr: Tensor, tau_mm: Tensor, *, delta_mm: float = 15.0,
        frame: Optional[Tensor] = None, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """The per-pixel part of BOP's Visible Surface Discrepancy for B pose pairs and T tolerances (tp_vsd; the rules are in the header):
    z_est, z_gt [B,H,W] (mesh_raster's zbuf: mm, <= 0 or NaN on background), depth_test [Ft,H,W] (the measured depth in mm, 0: no
    value; Ft 1 or B, or any Ft with ``frame`` [B] int32, the plane of each b), intr [B,3,3] or one [3,3], tau_mm [B,T] (or [T] for
    every b), T <= 16 -> 'err' [B,T] float32 and 'counts' [B,2+T] int32 (n_U, n_I, c_0 .. c_{T-1}).  ``out``: the two tensors to write
    into (neither needs clearing).  Not differentiable.  Three launches, no allocation beyond fresh outputs, safe under
    torch.cuda.graph."""
    z_est, z_gt, depth_test = _f32(z_est.detach(), "z_est"), _f32(z_gt.detach(), "z_gt"), _f32(depth_test.detach(), "depth_test")
    if z_est.dim() != 3 or z_est.numel() == 0 or z_gt.shape != z_est.shape:
        raise ValueError("vsd: z_est and z_gt [B,H,W] expected, got %s and %s" % (tuple(z_est.shape), tuple(z_gt.shape)))
    B, H, W = z_est.shape
    if depth_test.dim() != 3 or tuple(depth_test.shape[1:]) != (H, W) or depth_test.shape[0] == 0:
        raise ValueError("vsd: depth_test [Ft,H=%d,W=%d] expected, got %s" % (H, W, tuple(depth_test.shape)))
    Ft = depth_test.shape[0]
    frame = _lengths("vsd", frame, "frame", B, z_est)
    if frame is None and Ft not in (1, B):
        raise ValueError("vsd: depth_test must hold 1 or B = %d planes without frame=, got %d" % (B, Ft))
    intr, tau_mm = _intr_per_view("vsd", intr, B), _f32(tau_mm.detach(), "tau_mm")
    if tau_mm.dim() == 1:
        tau_mm = tau_mm[None].expand(B, -1).contiguous()
    if tau_mm.dim() != 2 or tau_mm.shape[0] != B:
        raise ValueError("vsd: tau_mm [B=%d,T] or [T] expected, got %s" % (B, tuple(tau_mm.shape)))
    T = tau_mm.shape[1]
    res = _outputs("vsd", out, {"err": (torch.float32, (B, T)), "counts": (torch.int32, (B, 2 + T))}, z_est.device)
    a = _lib.VsdArgs()
    a.z_est, a.z_gt, a.depth_test, a.frame = z_est.data_ptr(), z_gt.data_ptr(), depth_test.data_ptr(), _ptr(frame)
    a.intr, a.tau_mm, a.delta_mm = intr.data_ptr(), tau_mm.data_ptr(), float(delta_mm)
    a.B, a.Ft, a.H, a.W, a.T = B, Ft, H, W, T
    a.counts, a.err = res["counts"].data_ptr(), res["err"].data_ptr()
    _call("tp_vsd", a)                          # (T outside 1 .. 16: the library's error)
    return res


# ------------------------------------------------------------------------------------------ K28
PNP_MAX_HYP, PNP_MAX_ITERS = _lib.PNP_MAX_HYP, _lib.PNP_MAX_ITERS


def pnp_workspace(B: int, N: int, T: int, device) -> Tensor:
    """A workspace for corr_from_nocs / pnp_refine / pnp_ransac at B images, N entries and T hypotheses (tp_pnp_workspace_bytes);
    needs no clearing."""
    return _workspace_arg("pnp", None, int(_lib.load().tp_pnp_workspace_bytes(B, N, T)), device)


def _pnp_common(op: str, xy: Tensor, xyz: Tensor, count: Tensor, intr: Tensor):
    xy, xyz = _f32(xy.detach(), "xy"), _f32(xyz.detach(), "xyz")
    if xy.dim() != 3 or xy.shape[2] != 2 or xy.shape[0] == 0 or xy.shape[1] == 0 or tuple(xyz.shape) != tuple(xy.shape[:2]) + (3,):
        raise ValueError("%s: xy [B,N,2] and xyz [B,N,3] expected, got %s and %s" % (op, tuple(xy.shape), tuple(xyz.shape)))
    B, N = xy.shape[:2]
    return xy, xyz, _lengths(op, count, "count", B, xy, required=True), _intr_per_view(op, intr, B), B, N


@_on_tensor_device
def corr_from_nocs(nocs: Tensor, mask: Tensor, centre, scale, *, stride: int = 1, workspace: Optional[Tensor] = None,
                   out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """A NOCS map as a dense 2D-3D correspondence list (tp_corr_from_nocs; the rules are in the header): nocs [B,H,W,3], mask [B,H,W]
    (uint8, bool or float; non-zero: use the pixel), ``centre`` / ``scale`` [3] as surfel.nocs_normalisation returns them -> 'xy'
    [B,N,2] (pixel centres), 'xyz' [B,N,3] (mm) and 'count' [B] int32 with N = ceil(H / stride) * ceil(W / stride), the kept pixels in
    scan order; entries from count[b] on are not written.  ``workspace``: pnp_workspace(B, N, 1).  Two launches, no atomics, safe
    under torch.cuda.graph."""
    nocs = _f32(nocs.detach(), "nocs")
    if nocs.dim() != 4 or nocs.shape[3] != 3 or nocs.numel() == 0:
        raise ValueError("corr_from_nocs: nocs [B,H,W,3] expected, got %s" % (tuple(nocs.shape),))
    B, H, W = nocs.shape[:3]
    if not torch.is_tensor(mask) or not mask.is_cuda or tuple(mask.shape) != (B, H, W):
        raise ValueError("corr_from_nocs: mask must be a GPU tensor of shape %s" % ((B, H, W),))
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8) if mask.is_contiguous() else mask.to(torch.uint8)
    elif mask.dtype not in (torch.uint8, torch.float32):
        mask = mask.float()
    mask = mask.contiguous()
    stride = int(stride)
    if stride < 1:
        raise ValueError("corr_from_nocs: stride >= 1 expected, got %d" % stride)
    N = -(-H // stride) * -(-W // stride)
    dev = nocs.device
    res = _outputs("corr_from_nocs", out, {"xy": (torch.float32, (B, N, 2)), "xyz": (torch.float32, (B, N, 3)), "count": (torch.int32, (B,))}, dev, partial=True)
    workspace = _workspace_arg("corr_from_nocs", workspace, int(_lib.load().tp_pnp_workspace_bytes(B, N, 1)), dev, align=16)
    a = _lib.CorrFromNocsArgs()
    a.nocs, a.mask, a.mask_is_float = nocs.data_ptr(), mask.data_ptr(), int(mask.dtype == torch.float32)
    a.centre, a.scale = _float3(centre), _float3(scale)
    a.B, a.H, a.W, a.stride = B, H, W, stride
    a.xy, a.xyz, a.count, a.workspace = res["xy"].data_ptr(), res["xyz"].data_ptr(), res["count"].data_ptr(), workspace.data_ptr()
    _call("tp_corr_from_nocs", a)
    return res


@_on_tensor_device
def pnp_hypotheses(xy: Tensor, xyz: Tensor, count: Tensor, intr: Tensor, *, T: int = 256, seed: int = 0,
                   out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """T minimal-sample pose hypotheses per image (tp_pnp_hypotheses; the rules are in the header): xy [B,N,2], xyz [B,N,3], count [B]
    int32, intr [B,3,3] or one [3,3] -> 'sample_idx' [B,T,4] int32 (four distinct Philox draws, a function of seed, b, h and the
    count alone), 'hyp' [B,T,12] ([R|t] row-major, P3P in fp64) and 'hyp_valid' [B,T] uint8.  One launch, safe under torch.cuda.graph."""
    xy, xyz, count, intr, B, N = _pnp_common("pnp_hypotheses", xy, xyz, count, intr)
    T = int(T)
    dev = xy.device
    res = _outputs("pnp_hypotheses", out, {"sample_idx": (torch.int32, (B, max(T, 0), 4)), "hyp": (torch.float32, (B, max(T, 0), 12)),
                                           "hyp_valid": (torch.uint8, (B, max(T, 0)))}, dev, partial=True)
    a = _lib.PnpHypothesesArgs()
    a.xy, a.xyz, a.count, a.intr = xy.data_ptr(), xyz.data_ptr(), count.data_ptr(), intr.data_ptr()
    a.B, a.N, a.T, a.seed = B, N, T, int(seed) & (2 ** 64 - 1)
    a.sample_idx, a.hyp, a.hyp_valid = res["sample_idx"].data_ptr(), res["hyp"].data_ptr(), res["hyp_valid"].data_ptr()
    _call("tp_pnp_hypotheses", a)     # (T outside 1 .. 4096: the library's error)
    return res


@_on_tensor_device
def pnp_score(xy: Tensor, xyz: Tensor, count: Tensor, intr: Tensor, poses: Tensor, *, tau_px: float = 2.0, valid: Optional[Tensor] = None,
              sel: Optional[Tensor] = None, inliers: Optional[Tensor] = None, inlier_mask: Optional[Tensor] = None):
    """Inlier counts of T poses per image (tp_pnp_score; the rules are in the header): poses [B,T,12] or [B,T,3,4] -> inliers [B,T]
    int32 (the entries reprojected within tau_px, in fp32).  ``valid`` [B,T] uint8: poses with 0 count 0.  ``sel`` [B] int32: also
    return inlier_mask [B,N] uint8 of pose sel[b] (then the result is the pair).  ``inliers`` / ``inlier_mask``: the tensors to
    write into (neither needs clearing).  Integer atomics only: bit-identical from run to run.  Two launches, three with the mask;
    safe under torch.cuda.graph."""
    xy, xyz, count, intr, B, N = _pnp_common("pnp_score", xy, xyz, count, intr)
    poses = _f32(poses.detach(), "poses")
    if poses.dim() == 4 and tuple(poses.shape[2:]) == (3, 4):
        poses = poses.reshape(B, -1, 12)
    if poses.dim() != 3 or poses.shape[0] != B or poses.shape[2] != 12:
        raise ValueError("pnp_score: poses [B=%d,T,12] or [B,T,3,4] expected, got %s" % (B, tuple(poses.shape)))
    T = poses.shape[1]
    dev = xy.device
    if valid is not None:
        valid = _want_gpu("pnp_score", valid, "valid", torch.uint8, (B, T))
    sel = _lengths("pnp_score", sel, "sel", B, xy)
    inliers = torch.empty(B, T, device=dev, dtype=torch.int32) if inliers is None else _want_gpu("pnp_score", inliers, "inliers", torch.int32, (B, T))
    if sel is not None:
        inlier_mask = torch.empty(B, N, device=dev, dtype=torch.uint8) if inlier_mask is None else _want_gpu("pnp_score", inlier_mask, "inlier_mask", torch.uint8, (B, N))
    elif inlier_mask is not None:
        raise ValueError("pnp_score: inlier_mask needs sel")
    a = _lib.PnpScoreArgs()
    a.xy, a.xyz, a.count, a.intr, a.poses, a.valid = xy.data_ptr(), xyz.data_ptr(), count.data_ptr(), intr.data_ptr(), poses.data_ptr(), _ptr(valid)
    a.B, a.N, a.T, a.tau_px = B, N, T, float(tau_px)
    a.inliers, a.sel, a.inlier_mask = inliers.data_ptr(), _ptr(sel), _ptr(inlier_mask)
    _call("tp_pnp_score", a)               # (T, tau_px out of range: the library's error)
    return inliers if sel is None else (inliers, inlier_mask)


@_on_tensor_device
def pnp_refine(xy: Tensor, xyz: Tensor, count: Tensor, intr: Tensor, hyp: Tensor, hyp_inliers: Optional[Tensor] = None,
               hyp_valid: Optional[Tensor] = None, *, tau_px: float = 2.0, iters: int = 5, workspace: Optional[Tensor] = None,
               out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """Pick each image's winner among hyp [B,T,12] by hyp_inliers [B,T] int32 (ties: the lowest h; hyp_valid [B,T] uint8 = 0 is never
    picked) and refine it by ``iters`` keep-best Gauss-Newton steps in fp64 on its inliers at tau_px (tp_pnp_refine; the rules are in
    the header).  One start pose per image: hyp [B,3,4] (or [B,12]) alone.  -> 'pose' [B,3,4], 'inliers' [B] int32, 'rms' [B] (px),
    'status' [B] int32 (0 ok, 1 fewer than 4 entries, 2 no valid hypothesis, 3 a system was not positive definite: the best pose so
    far).  ``workspace``: pnp_workspace(B, N, T).  3 + 2 iters launches, no atomics, safe under torch.cuda.graph."""
    xy, xyz, count, intr, B, N = _pnp_common("pnp_refine", xy, xyz, count, intr)
    hyp = _f32(hyp.detach(), "hyp")
    if hyp.dim() == 4 and tuple(hyp.shape[2:]) == (3, 4):
        hyp = hyp.reshape(B, -1, 12)
    elif tuple(hyp.shape) in ((B, 3, 4), (B, 12)) and hyp_inliers is None:
        hyp = hyp.reshape(B, 1, 12)
    if hyp.dim() != 3 or hyp.shape[0] != B or hyp.shape[2] != 12:
        raise ValueError("pnp_refine: hyp [B=%d,T,12], or one start pose [B,3,4] per image, expected, got %s" % (B, tuple(hyp.shape)))
    T = hyp.shape[1]
    dev = xy.device
    if hyp_inliers is None:
        if T != 1:
            raise ValueError("pnp_refine: hyp_inliers [B,T] is needed to pick among T = %d hypotheses" % T)
        hyp_inliers = torch.zeros(B, 1, device=dev, dtype=torch.int32)
    hyp_inliers = _want_gpu("pnp_refine", hyp_inliers, "hyp_inliers", torch.int32, (B, T))
    if hyp_valid is not None:
        hyp_valid = _want_gpu("pnp_refine", hyp_valid, "hyp_valid", torch.uint8, (B, T))
    res = _outputs("pnp_refine", out, {"pose": (torch.float32, (B, 3, 4)), "inliers": (torch.int32, (B,)), "rms": (torch.float32, (B,)),
                                       "status": (torch.int32, (B,))}, dev, partial=True)
    workspace = _workspace_arg("pnp_refine", workspace, int(_lib.load().tp_pnp_workspace_bytes(B, N, T)), dev, align=16)
    a = _lib.PnpRefineArgs()
    a.xy, a.xyz, a.count, a.intr = xy.data_ptr(), xyz.data_ptr(), count.data_ptr(), intr.data_ptr()
    a.hyp, a.hyp_valid, a.hyp_inliers = hyp.data_ptr(), _ptr(hyp_valid), hyp_inliers.data_ptr()
    a.B, a.N, a.T, a.tau_px, a.iters = B, N, T, float(tau_px), int(iters)
    a.pose, a.inliers, a.rms, a.status, a.workspace = (res["pose"].data_ptr(), res["inliers"].data_ptr(), res["rms"].data_ptr(),
                                                       res["status"].data_ptr(), workspace.data_ptr())
    _call("tp_pnp_refine", a)             # (tau_px, iters out of range: the library's error)
    return res


PNP_RANSAC_KEYS = ("pose", "inliers", "rms", "status", "sample_idx", "hyp", "hyp_valid", "hyp_inliers")


@_on_tensor_device
def pnp_ransac(xy: Tensor, xyz: Tensor, count: Tensor, intr: Tensor, *, T: int = 256, tau_px: float = 2.0, iters: int = 5, seed: int = 0,
               workspace: Optional[Tensor] = None, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """PnP with RANSAC for B images at once: pnp_hypotheses, pnp_score and pnp_refine in a row (the rules are in the header).
    -> pnp_refine's 'pose', 'inliers', 'rms', 'status' and the intermediate 'sample_idx', 'hyp', 'hyp_valid', 'hyp_inliers'.
    ``out``: any of these tensors to write into; ``workspace``: pnp_workspace(B, N, T).  With both given nothing is allocated.
    6 + 2 iters launches, bit-identical from run to run, safe under torch.cuda.graph."""
    hy = pnp_hypotheses(xy, xyz, count, intr, T=T, seed=seed, out=out)
    inl = pnp_score(xy, xyz, count, intr, hy["hyp"], tau_px=tau_px, valid=hy["hyp_valid"], inliers=None if out is None else out.get("hyp_inliers"))
    res = pnp_refine(xy, xyz, count, intr, hy["hyp"], inl, hy["hyp_valid"], tau_px=tau_px, iters=iters, workspace=workspace, out=out)
    res.update(hy, hyp_inliers=inl)
    return res
