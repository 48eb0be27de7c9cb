"""K24-K26, K28-K33: nearest neighbours, the pose errors, VSD, PnP-RANSAC, the depth ICP, the photometric alignment, the masks' distance
field, the silhouette alignment and the joint step of the last three."""
from typing import Dict, Optional

import torch

from .. import _lib
from ._base import (Tensor, _call, _f32, _float3, _intr_per_view, _lengths, _on_tensor_device, _outputs, _points, _poses, _ptr, _want_gpu,
                    _workspace_arg)

__all__ = ["NN1_MODES", "nn1", "pose_errors", "vsd", "PNP_MAX_HYP", "PNP_MAX_ITERS", "pnp_workspace", "_pnp_common", "corr_from_nocs",
           "pnp_hypotheses", "pnp_score", "pnp_refine", "PNP_RANSAC_KEYS", "pnp_ransac", "depth_icp_workspace", "depth_icp_step",
           "DEPTH_ICP_KEYS", "depth_icp", "photo_align_workspace", "photo_align_step", "PHOTO_ALIGN_KEYS", "photo_align", "mask_sdf_workspace", "mask_sdf",
           "mask_known_from_others", "silhouette_align_workspace", "silhouette_align_step", "SILHOUETTE_ALIGN_KEYS", "silhouette_align",
           "JOINT_TERMS", "JOINT_WEIGHTS", "_joint_weights", "joint_align_workspace", "joint_align_step", "JOINT_ALIGN_KEYS", "joint_align"]

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


# ------------------------------------------------------------------------------------------ K29, K30: what the two refiners share
def _frame_planes(op: str, name: str, planes: Tensor, trailing_shape: tuple, frame: Optional[Tensor], mask: Optional[Tensor], B: int, H: int,
                  W: int, like: Tensor):
    """The measured planes ``name`` [Ft,H,W] + trailing_shape (one plane: Ft = 1), the frame map and the mask [Ft,H,W] of a step ->
    (planes, frame, mask, Ft)."""
    planes = _f32(planes.detach(), name)
    if planes.dim() == 2 + len(trailing_shape):
        planes = planes[None]
    if planes.dim() != 3 + len(trailing_shape) or tuple(planes.shape[1:]) != (H, W) + trailing_shape or planes.shape[0] == 0:
        layout = "[Ft,H=%d,W=%d,3] (channels last)" % (H, W) if trailing_shape else "[Ft,H=%d,W=%d]" % (H, W)
        raise ValueError("%s: %s %s expected, got %s" % (op, name, layout, tuple(planes.shape)))
    Ft = planes.shape[0]
    frame = _lengths(op, frame, "frame", B, like)
    if frame is None and Ft not in (1, B):
        raise ValueError("%s: %s must hold 1 or B = %d %s without frame=, got %d" % (op, name, B, "photographs" if trailing_shape else "planes", Ft))
    if mask is not None:
        if torch.is_tensor(mask) and mask.dtype == torch.bool:
            mask = mask.view(torch.uint8) if mask.is_contiguous() else mask.to(torch.uint8)
        if torch.is_tensor(mask) and mask.dim() == 2:
            mask = mask[None]
        mask = _want_gpu(op, mask, "mask", torch.uint8, (Ft, H, W))
    return planes, frame, mask, Ft


def _gn_step_outputs(op: str, a, out: Optional[Dict[str, Tensor]], workspace: Optional[Tensor], B: int, dev, workspace_bytes: int,
                     with_pose: bool = True) -> Dict[str, Tensor]:
    """The four outputs of a step (fresh, or those of ``out``) and its workspace, entered into the args struct ``a``; without
    ``with_pose`` (a term of the joint step, which writes no pose of its own) the three others and a null pose_out -> (outputs, workspace)."""
    spec = {"pose": (torch.float32, (B, 3, 4)), "inliers": (torch.int32, (B,)), "rms": (torch.float32, (B,)), "status": (torch.int32, (B,))}
    if not with_pose:
        del spec["pose"]
    res = _outputs(op, out, spec, dev, partial=True)
    workspace = _workspace_arg(op, workspace, workspace_bytes, dev, align=16)
    a.pose_out, a.inliers, a.rms, a.status, a.workspace = (_ptr(res.get("pose")), res["inliers"].data_ptr(), res["rms"].data_ptr(),
                                                           res["status"].data_ptr(), workspace.data_ptr())
    return res, workspace


def _tau_schedule(op: str, tau, tau_name: str, iters: int):
    """A loop's thresholds, checked before anything else of the call: one value or ``iters`` + 1 host values -> iters + 1 floats."""
    iters = int(iters)
    if iters < 0:
        raise ValueError("%s: iters >= 0 expected, got %d" % (op, iters))
    taus = [float(tau)] * (iters + 1) if isinstance(tau, (int, float)) else [float(t) for t in tau]
    if len(taus) != iters + 1:
        raise ValueError("%s: %s must be one value or iters + 1 = %d values, got %d" % (op, tau_name, iters + 1, len(taus)))
    return taus


def _refine_loop(pose: Tensor, taus, raster, step) -> Dict[str, Tensor]:
    """One pass per threshold of ``raster(pose)`` and ``step(planes, pose, tau, evaluate_only)`` from ``pose`` on, the last
    evaluate-only -> the last pass's pose, inliers and rms, the status of the last step taken (of the evaluation where there is no
    step) and inliers0 / rms0 of the first pass."""
    iters = len(taus) - 1
    res, first, status = None, None, None
    for it, t in enumerate(taus):
        res = step(raster(pose), pose, t, it == iters)
        first = res if first is None else first
        status = res["status"] if it < iters or status is None else status
        pose = res["pose"]
    return dict(pose=res["pose"], inliers=res["inliers"], rms=res["rms"], status=status, inliers0=first["inliers"], rms0=first["rms"])


# ------------------------------------------------------------------------------------------ K29
def depth_icp_workspace(B: int, H: int, W: int, device) -> Tensor:
    """A workspace for depth_icp_step / depth_icp at B images of H x W (tp_depth_icp_workspace_bytes); needs no clearing."""
    return _workspace_arg("depth_icp", None, int(_lib.load().tp_depth_icp_workspace_bytes(B, H, W)), device)


@_on_tensor_device
def depth_icp_step(verts: Tensor, faces: Tensor, zbuf: Tensor, face: Tensor, pose: Tensor, intr: Tensor, depth: Tensor, *, tau_mm: float,
                   damping: float = 1e-6, frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, evaluate_only: bool = False,
                   workspace: Optional[Tensor] = None, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """One step of projective point-to-plane ICP for B poses (tp_depth_icp_step; the rules are in the header): verts [V,3], faces [F,3]
    int32, zbuf / face [B,H,W] (mesh_raster's planes of the mesh at ``pose``; taken as they are), pose [B,3,4], intr [B,3,3] or one
    [3,3], depth [Ft,H,W] (the measured depth in mm; <= 0, NaN, Inf: no value; Ft 1 or B, or any Ft with ``frame`` [B] int32), mask
    [Ft,H,W] uint8 or bool (0: skip the pixel) -> 'pose' [B,3,4] (the stepped pose; ``pose`` itself, bit for bit, with
    ``evaluate_only`` or a non-zero status), 'inliers' [B] int32 and 'rms' [B] (mm) of ``pose`` over the pixels within tau_mm along
    the ray, 'status' [B] int32 (0 ok, 1 fewer than 6 kept pixels, 3 not positive definite).  ``workspace``:
    depth_icp_workspace(B, H, W); ``out``: any of the four tensors to write into (out['pose'] must not be ``pose``).  Two launches, no
    atomics, bit-identical from run to run, safe under torch.cuda.graph."""
    a, res, _alive = _depth_icp_args("depth_icp_step", verts, faces, zbuf, face, pose, intr, depth, tau_mm=tau_mm, damping=damping, frame=frame, mask=mask,
                                     evaluate_only=evaluate_only, workspace=workspace, out=out)
    _call("tp_depth_icp_step", a)         # (tau_mm, damping out of range, out['pose'] overlapping pose: the library's error)
    return res


def _depth_icp_args(op: str, verts, faces, zbuf, face, pose, intr, depth, *, tau_mm, damping=1e-6, frame=None, mask=None, evaluate_only=False,
                    workspace=None, out=None, with_pose=True):
    """depth_icp_step's arguments, checked, as (the filled tp_depth_icp_args, its outputs, the tensors it points into)."""
    verts, pose = _points(op, verts, "verts"), _poses(op, pose, "pose")
    B = pose.shape[0]
    faces = _want_gpu(op, faces, "faces", torch.int32, None)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
        raise ValueError("%s: faces [F,3] expected, got %s" % (op, tuple(faces.shape)))
    zbuf = _want_gpu(op, zbuf, "zbuf", torch.float32, None)
    if zbuf.dim() != 3 or zbuf.shape[0] != B or zbuf.numel() == 0:
        raise ValueError("%s: zbuf [B=%d,H,W] expected, got %s" % (op, B, tuple(zbuf.shape)))
    H, W = zbuf.shape[1:]
    face = _want_gpu(op, face, "face", torch.int32, (B, H, W))
    intr = _intr_per_view(op, intr, B)
    depth, frame, mask, Ft = _frame_planes(op, "depth", depth, (), frame, mask, B, H, W, zbuf)
    a = _lib.DepthIcpArgs()
    res, workspace = _gn_step_outputs(op, a, out, workspace, B, zbuf.device, int(_lib.load().tp_depth_icp_workspace_bytes(B, H, W)), with_pose)
    a.verts, a.faces, a.zbuf, a.face, a.pose, a.intr = verts.data_ptr(), faces.data_ptr(), zbuf.data_ptr(), face.data_ptr(), pose.data_ptr(), intr.data_ptr()
    a.depth, a.frame, a.mask = depth.data_ptr(), _ptr(frame), _ptr(mask)
    a.V, a.F, a.B, a.Ft, a.H, a.W = verts.shape[0], faces.shape[0], B, Ft, H, W
    a.tau_mm, a.damping, a.evaluate_only = float(tau_mm), float(damping), int(bool(evaluate_only))
    return a, res, (workspace, verts, faces, zbuf, face, pose, intr, depth, frame, mask)       # (the struct holds addresses only)


DEPTH_ICP_KEYS = ("pose", "inliers", "rms", "status", "inliers0", "rms0")


@_on_tensor_device
def depth_icp(verts: Tensor, faces: Tensor, pose: Tensor, intr: Tensor, depth: Tensor, *, tau_mm=20.0, iters: int = 5, damping: float = 1e-6,
              frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, workspace: Optional[Tensor] = None,
              cull: bool = False) -> Dict[str, Tensor]:
    """Refine B poses of one mesh against measured depth (the rules are in the header, K29): ``iters`` + 1 passes of mesh_raster at the
    current poses (depth and face index, H x W = depth's) followed by depth_icp_step, the last with evaluate_only.  ``tau_mm``: one
    value, or ``iters`` + 1 host values for a coarse-to-fine schedule (the last is the final evaluation's).  -> 'pose' [B,3,4], its
    'inliers' [B] int32 and 'rms' [B] (mm), 'status' [B] int32 of the last step taken (of the evaluation where iters = 0) and
    'inliers0' / 'rms0' of the start pose.  A step that fails passes its pose on.  2 (iters + 1) launches besides the rasteriser's,
    bit-identical from run to run, safe under torch.cuda.graph.  ``cull``: the passes render with mesh_raster(cull=True), same bits."""
    op = "depth_icp"
    taus = _tau_schedule(op, tau_mm, "tau_mm", iters)
    verts, pose = _points(op, verts, "verts"), _poses(op, pose, "pose")
    B = pose.shape[0]
    faces = faces.to(device=verts.device, dtype=torch.int32).contiguous()
    depth = _f32(depth.detach(), "depth")
    if depth.dim() == 2:
        depth = depth[None]
    if depth.dim() != 3 or depth.numel() == 0:
        raise ValueError("%s: depth [Ft,H,W] expected, got %s" % (op, tuple(depth.shape)))
    H, W = depth.shape[1:]
    intr = _intr_per_view(op, intr, B)
    depth, frame, mask, _ = _frame_planes(op, "depth", depth, (), frame, mask, B, H, W, pose)
    workspace = _workspace_arg(op, workspace, int(_lib.load().tp_depth_icp_workspace_bytes(B, H, W)), pose.device, align=16)
    from .scene import mesh_raster
    raster = lambda P: mesh_raster(verts, faces, P, intr, H=H, W=W, face_ids=True, normals=False, cull=cull)
    step = lambda r, P, t, last: depth_icp_step(verts, faces, r["zbuf"], r["face"], P, intr, depth, tau_mm=t, damping=damping,
                                                frame=frame, mask=mask, evaluate_only=last, workspace=workspace)
    return _refine_loop(pose, taus, raster, step)


# ------------------------------------------------------------------------------------------ K30
def photo_align_workspace(B: int, H: int, W: int, device) -> Tensor:
    """A workspace for photo_align_step / photo_align at B images of H x W (tp_photo_align_workspace_bytes); needs no clearing."""
    return _workspace_arg("photo_align", None, int(_lib.load().tp_photo_align_workspace_bytes(B, H, W)), device)


@_on_tensor_device
def photo_align_step(zbuf: Tensor, rgb: Tensor, pose: Tensor, intr: Tensor, image: Tensor, *, tau: float, damping: float = 1e-6,
                     frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, evaluate_only: bool = False,
                     workspace: Optional[Tensor] = None, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """One step of photometric alignment for B poses (tp_photo_align_step; the rules are in the header): zbuf [B,H,W] / rgb [B,H,W,3]
    (mesh_raster's planes of the vertex-coloured mesh at ``pose``; taken as they are), pose [B,3,4], intr [B,3,3] or one [3,3], image
    [Ft,H,W,3] (the photograph, channels last, in rgb's units; Ft 1 or B, or any Ft with ``frame`` [B] int32), mask [Ft,H,W] uint8 or
    bool (0: skip the pixel) -> 'pose' [B,3,4] (the stepped pose; ``pose`` itself, bit for bit, with ``evaluate_only`` or a non-zero
    status), 'inliers' [B] int32 and 'rms' [B] (colour units) of ``pose`` over the interior covered pixels whose colours differ by at
    most ``tau``, 'status' [B] int32 (0 ok, 1 fewer than 6 kept pixels, 3 not positive definite).  ``workspace``:
    photo_align_workspace(B, H, W); ``out``: any of the four tensors to write into (out['pose'] must not be ``pose``).  Two launches,
    no atomics, bit-identical from run to run, safe under torch.cuda.graph."""
    a, res, _alive = _photo_align_args("photo_align_step", zbuf, rgb, pose, intr, image, tau=tau, damping=damping, frame=frame, mask=mask,
                                       evaluate_only=evaluate_only, workspace=workspace, out=out)
    _call("tp_photo_align_step", a)       # (tau, damping out of range, out['pose'] overlapping pose: the library's error)
    return res


def _photo_align_args(op: str, zbuf, rgb, pose, intr, image, *, tau, damping=1e-6, frame=None, mask=None, evaluate_only=False, workspace=None,
                      out=None, with_pose=True):
    """photo_align_step's arguments, checked, as (the filled tp_photo_align_args, its outputs, the tensors it points into)."""
    pose = _poses(op, pose, "pose")
    B = pose.shape[0]
    zbuf = _want_gpu(op, zbuf, "zbuf", torch.float32, None)
    if zbuf.dim() != 3 or zbuf.shape[0] != B or zbuf.numel() == 0:
        raise ValueError("%s: zbuf [B=%d,H,W] expected, got %s" % (op, B, tuple(zbuf.shape)))
    H, W = zbuf.shape[1:]
    rgb = _want_gpu(op, rgb, "rgb", torch.float32, (B, H, W, 3))
    intr = _intr_per_view(op, intr, B)
    image, frame, mask, Ft = _frame_planes(op, "image", image, (3,), frame, mask, B, H, W, zbuf)
    a = _lib.PhotoAlignArgs()
    res, workspace = _gn_step_outputs(op, a, out, workspace, B, zbuf.device, int(_lib.load().tp_photo_align_workspace_bytes(B, H, W)), with_pose)
    a.zbuf, a.rgb, a.pose, a.intr = zbuf.data_ptr(), rgb.data_ptr(), pose.data_ptr(), intr.data_ptr()
    a.image, a.frame, a.mask = image.data_ptr(), _ptr(frame), _ptr(mask)
    a.B, a.Ft, a.H, a.W = B, Ft, H, W
    a.tau, a.damping, a.evaluate_only = float(tau), float(damping), int(bool(evaluate_only))
    return a, res, (workspace, zbuf, rgb, pose, intr, image, frame, mask)       # (the struct holds addresses only)


PHOTO_ALIGN_KEYS = ("pose", "inliers", "rms", "status", "inliers0", "rms0")


@_on_tensor_device
def photo_align(verts: Tensor, faces: Tensor, vcolor: Tensor, pose: Tensor, intr: Tensor, image: Tensor, *, tau=0.5, iters: int = 10,
                damping: float = 1e-6, frame: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                workspace: Optional[Tensor] = None, cull: bool = False, texels: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """Refine B poses of one vertex-coloured mesh against a photograph (the rules are in the header, K30): ``iters`` + 1 passes of
    mesh_raster at the current poses (depth and colour, H x W = image's) followed by photo_align_step, the last with evaluate_only.
    ``tau``: one value, or ``iters`` + 1 host values for a coarse-to-fine schedule (the last is the final evaluation's).  -> 'pose'
    [B,3,4], its 'inliers' [B] int32 and 'rms' [B] (colour units), 'status' [B] int32 of the last step taken (of the evaluation where
    iters = 0) and 'inliers0' / 'rms0' of the start pose.  A step that fails passes its pose on.  2 (iters + 1) launches besides the
    rasteriser's, bit-identical from run to run, safe under torch.cuda.graph.  ``cull``: the passes render with
    mesh_raster(cull=True), same bits.  ``texels`` [F,T,3] with ``vcolor`` None: the passes colour the mesh from its face texels
    (mesh_raster(texels=), K35); exactly one of the two."""
    op = "photo_align"
    if (vcolor is None) == (texels is None):
        raise ValueError("%s: exactly one of vcolor [V,3] and texels= [F,T,3] expected" % op)
    taus = _tau_schedule(op, tau, "tau", iters)
    verts, pose = _points(op, verts, "verts"), _poses(op, pose, "pose")
    B = pose.shape[0]
    faces = faces.to(device=verts.device, dtype=torch.int32).contiguous()
    vcolor = None if vcolor is None else _f32(vcolor.detach(), "vcolor")
    texels = None if texels is None else _f32(texels.detach(), "texels")
    image = _f32(image.detach(), "image")
    if image.dim() == 3:
        image = image[None]
    if image.dim() != 4 or image.shape[3] != 3 or image.numel() == 0:
        raise ValueError("%s: image [Ft,H,W,3] (channels last) expected, got %s" % (op, tuple(image.shape)))
    H, W = image.shape[1:3]
    intr = _intr_per_view(op, intr, B)
    image, frame, mask, _ = _frame_planes(op, "image", image, (3,), frame, mask, B, H, W, pose)
    workspace = _workspace_arg(op, workspace, int(_lib.load().tp_photo_align_workspace_bytes(B, H, W)), pose.device, align=16)
    from .scene import mesh_raster
    raster = lambda P: mesh_raster(verts, faces, P, intr, H=H, W=W, vcolor=vcolor, texels=texels, face_ids=False, normals=False, cull=cull)
    step = lambda r, P, t, last: photo_align_step(r["zbuf"], r["rgb"], P, intr, image, tau=t, damping=damping, frame=frame,
                                                  mask=mask, evaluate_only=last, workspace=workspace)
    return _refine_loop(pose, taus, raster, step)


# ------------------------------------------------------------------------------------------ K31
def mask_sdf_workspace(F: int, H: int, W: int, device) -> Tensor:
    """A workspace for mask_sdf at F masks of H x W (tp_mask_sdf_workspace_bytes); needs no clearing."""
    return _workspace_arg("mask_sdf", None, int(_lib.load().tp_mask_sdf_workspace_bytes(F, H, W)), device)


@_on_tensor_device
def mask_sdf(mask: Tensor, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None, known: Optional[Tensor] = None) -> Tensor:
    """The exact signed Euclidean distance field of F masks (tp_mask_sdf; the rules are in the header): mask [F,H,W] (or one [H,W])
    uint8 or bool, non-zero: set -> sdf float32 of mask's shape, in pixels: sqrt(d2_set) - 0.5 on a clear pixel, -(sqrt(d2_clear) -
    0.5) on a set one, with the squared distances to the nearest set / clear pixel of the plane (H^2 + W^2 where it has none).
    ``out``: the tensor to write into; ``workspace``: mask_sdf_workspace(F, H, W).  H, W <= 8192.  Two launches, no atomics, a function
    of the mask alone, safe under torch.cuda.graph.  ``known`` (uint8 or bool, of mask's shape, non-zero: the pixel's mask value is a
    measurement) makes the rest UNKNOWN, neither set nor clear (tp_mask_sdf_known, K31c): no distance is measured to such a pixel and
    its own value is NaN, which silhouette_align_step drops; with every pixel known the field is the plain one bit for bit."""
    op = "mask_sdf"
    if torch.is_tensor(mask) and not mask.is_cuda:
        raise _lib.TexposeLibraryError("mask must live on the GPU (texpose_amd has no CPU path)")
    if torch.is_tensor(mask) and mask.dtype == torch.bool:
        mask = mask.view(torch.uint8) if mask.is_contiguous() else mask.to(torch.uint8)
    mask = _want_gpu(op, mask, "mask", torch.uint8, None)
    if known is not None:
        if torch.is_tensor(known) and known.dtype == torch.bool:
            known = known.view(torch.uint8) if known.is_contiguous() else known.to(torch.uint8)
        known = _want_gpu(op, known, "known", torch.uint8, tuple(mask.shape))
    if mask.dim() not in (2, 3) or mask.numel() == 0:
        raise ValueError("%s: mask [F,H,W] or [H,W] expected, got %s" % (op, tuple(mask.shape)))
    F, H, W = (1,) + tuple(mask.shape) if mask.dim() == 2 else tuple(mask.shape)
    sdf = torch.empty(mask.shape, device=mask.device) if out is None else _want_gpu(op, out, "out", torch.float32, tuple(mask.shape))
    workspace = _workspace_arg(op, workspace, int(_lib.load().tp_mask_sdf_workspace_bytes(F, H, W)), mask.device, align=16)
    if known is None:
        _call("tp_mask_sdf", mask.data_ptr(), sdf.data_ptr(), F, H, W, workspace.data_ptr())      # (H or W > 8192: the library's error)
    else:
        _call("tp_mask_sdf_known", mask.data_ptr(), known.data_ptr(), sdf.data_ptr(), F, H, W, workspace.data_ptr())
    return sdf


@_on_tensor_device
def mask_known_from_others(sdf: Tensor, band_px: float = 0.0, out: Optional[Tensor] = None) -> Tensor:
    """Who hides whom among the N instances of ONE frame (tp_mask_known_from_others, K32; the rules are in the header): sdf [N,H,W]
    float32, mask_sdf's fields of the frame's instance masks (taken as they are) -> known [N,H,W] uint8: 0 where the pixel lies within
    ``band_px`` pixels of a set pixel of ANOTHER instance (sdf[m,p] <= band_px - 0.5 in fp32 for some m != n; a NaN is not near), else
    1: mask_sdf's ``known``.  Conservative: where two instances touch, both lose the contour between them.  ``out``: the uint8 tensor
    to write into.  One launch, no workspace, no atomics, safe under torch.cuda.graph."""
    op = "mask_known_from_others"
    if torch.is_tensor(sdf) and not sdf.is_cuda:
        raise _lib.TexposeLibraryError("sdf must live on the GPU (texpose_amd has no CPU path)")
    sdf = _want_gpu(op, sdf, "sdf", torch.float32, None)
    if sdf.dim() != 3 or sdf.numel() == 0:
        raise ValueError("%s: sdf [N,H,W] expected, got %s" % (op, tuple(sdf.shape)))
    N, H, W = sdf.shape
    known = torch.empty(sdf.shape, device=sdf.device, dtype=torch.uint8) if out is None else _want_gpu(op, out, "out", torch.uint8, tuple(sdf.shape))
    _call("tp_mask_known_from_others", sdf.data_ptr(), known.data_ptr(), N, H, W, float(band_px))  # (band_px, N > 65535: the library's error)
    return known


def silhouette_align_workspace(B: int, H: int, W: int, device) -> Tensor:
    """A workspace for silhouette_align_step / silhouette_align at B images of H x W (tp_silhouette_align_workspace_bytes); needs no
    clearing."""
    return _workspace_arg("silhouette_align", None, int(_lib.load().tp_silhouette_align_workspace_bytes(B, H, W)), device)


@_on_tensor_device
def silhouette_align_step(zbuf: Tensor, pose: Tensor, intr: Tensor, sdf: Tensor, *, tau_px: float, damping: float = 1e-6,
                          frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, evaluate_only: bool = False,
                          workspace: Optional[Tensor] = None, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """One step of silhouette alignment for B poses (tp_silhouette_align_step; the rules are in the header): zbuf [B,H,W]
    (mesh_raster's depth of the mesh at ``pose``; taken as it is), pose [B,3,4], intr [B,3,3] or one [3,3], sdf [Ft,H,W] (mask_sdf's
    field of the measured masks: pixels, negative inside; Ft 1 or B, or any Ft with ``frame`` [B] int32), mask [Ft,H,W] uint8 or bool
    (0: the pixel gives no row) -> 'pose' [B,3,4] (the stepped pose; ``pose`` itself, bit for bit, with ``evaluate_only`` or a
    non-zero status), 'inliers' [B] int32 and 'rms' [B] (pixels) of ``pose`` over the interior rim pixels of the rendering within
    ``tau_px`` of the measured outline, 'status' [B] int32 (0 ok, 1 fewer than 6 kept pixels, 3 not positive definite), 'inter' and
    'uni' [B] int32 (the pixels covered and inside the measured mask, and those with either: IoU = inter / uni).  ``workspace``:
    silhouette_align_workspace(B, H, W); ``out``: any of the six tensors to write into (out['pose'] must not be ``pose``).  Three
    launches, no atomics, bit-identical from run to run, safe under torch.cuda.graph."""
    a, res, _alive = _silhouette_align_args("silhouette_align_step", zbuf, pose, intr, sdf, tau_px=tau_px, damping=damping, frame=frame, mask=mask,
                                            evaluate_only=evaluate_only, workspace=workspace, out=out)
    _call("tp_silhouette_align_step", a)  # (tau_px, damping out of range, out['pose'] overlapping pose: the library's error)
    return res


def _silhouette_align_args(op: str, zbuf, pose, intr, sdf, *, tau_px, damping=1e-6, frame=None, mask=None, evaluate_only=False, workspace=None,
                           out=None, with_pose=True):
    """silhouette_align_step's arguments, checked, as (the filled tp_silhouette_align_args, its outputs, the tensors it points into)."""
    pose = _poses(op, pose, "pose")
    B = pose.shape[0]
    zbuf = _want_gpu(op, zbuf, "zbuf", torch.float32, None)
    if zbuf.dim() != 3 or zbuf.shape[0] != B or zbuf.numel() == 0:
        raise ValueError("%s: zbuf [B=%d,H,W] expected, got %s" % (op, B, tuple(zbuf.shape)))
    H, W = zbuf.shape[1:]
    intr = _intr_per_view(op, intr, B)
    sdf, frame, mask, Ft = _frame_planes(op, "sdf", sdf, (), frame, mask, B, H, W, zbuf)
    a = _lib.SilhouetteAlignArgs()
    counts = _outputs(op, None if out is None else {k: v for k, v in out.items() if k in ("inter", "uni")},
                      {"inter": (torch.int32, (B,)), "uni": (torch.int32, (B,))}, zbuf.device, partial=True)
    res, workspace = _gn_step_outputs(op, a, None if out is None else {k: v for k, v in out.items() if k not in ("inter", "uni")}, workspace, B,
                                      zbuf.device, int(_lib.load().tp_silhouette_align_workspace_bytes(B, H, W)), with_pose)
    res.update(counts)
    a.zbuf, a.pose, a.intr, a.sdf, a.frame, a.mask = zbuf.data_ptr(), pose.data_ptr(), intr.data_ptr(), sdf.data_ptr(), _ptr(frame), _ptr(mask)
    a.B, a.Ft, a.H, a.W = B, Ft, H, W
    a.tau_px, a.damping, a.evaluate_only = float(tau_px), float(damping), int(bool(evaluate_only))
    a.inter, a.uni = res["inter"].data_ptr(), res["uni"].data_ptr()
    return a, res, (workspace, zbuf, pose, intr, sdf, frame, mask)       # (the struct holds addresses only)


SILHOUETTE_ALIGN_KEYS = ("pose", "inliers", "rms", "status", "inliers0", "rms0", "iou", "iou0")


@_on_tensor_device
def silhouette_align(verts: Tensor, faces: Tensor, pose: Tensor, intr: Tensor, sdf: Tensor, *, tau_px=4.0, iters: int = 10,
                     damping: float = 1e-6, frame: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                     workspace: Optional[Tensor] = None, visible_iou: bool = False, cull: bool = False) -> Dict[str, Tensor]:
    """Refine B poses of one mesh against the outlines of measured masks (the rules are in the header, K31): ``iters`` + 1 passes of
    mesh_raster at the current poses (depth alone, H x W = sdf's) followed by silhouette_align_step, the last with evaluate_only.
    ``sdf`` [Ft,H,W]: mask_sdf of the measured masks.  ``tau_px``: one value, or ``iters`` + 1 host values for a coarse-to-fine schedule
    (the last is the final evaluation's).  -> 'pose' [B,3,4], its 'inliers' [B] int32 and 'rms' [B] (pixels), 'status' [B] int32 of the
    last step taken (of the evaluation where iters = 0), 'inliers0' / 'rms0' of the start pose and 'iou' / 'iou0' [B] float32, the
    intersection over union of the rendering's coverage and the measured mask at the last and at the start pose (NaN where both are
    empty).  A step that fails passes its pose on.  It closes the OUTLINE: a pose parameter the outline does not see (a rotation about
    a symmetry axis, depth at a small radius) stays where it was, and a measured mask cut by an occluder pulls the rim to the cut.
    3 (iters + 1) launches besides the rasteriser's, bit-identical from run to run, safe under torch.cuda.graph.
    ``visible_iou``: for a field with unknown pixels (mask_sdf's ``known``; NaN there) also 'iou_visible' / 'iou0_visible' [B] float32,
    inter / (uni - hidden) at the last and at the start pose, ``hidden`` the covered pixels of the plane whose field value is NaN: the
    IoU over the pixels that were measured (NaN where none is left).  Exact integer counts by torch reductions on the first and the
    last rendering; without the flag nothing else runs and the keys are those above.  ``cull``: the passes render with
    mesh_raster(cull=True), same bits."""
    op = "silhouette_align"
    taus = _tau_schedule(op, tau_px, "tau_px", iters)
    verts, pose = _points(op, verts, "verts"), _poses(op, pose, "pose")
    B = pose.shape[0]
    faces = faces.to(device=verts.device, dtype=torch.int32).contiguous()
    sdf = _f32(sdf.detach(), "sdf")
    if sdf.dim() == 2:
        sdf = sdf[None]
    if sdf.dim() != 3 or sdf.numel() == 0:
        raise ValueError("%s: sdf [Ft,H,W] expected, got %s" % (op, tuple(sdf.shape)))
    H, W = sdf.shape[1:]
    intr = _intr_per_view(op, intr, B)
    sdf, frame, mask, _ = _frame_planes(op, "sdf", sdf, (), frame, mask, B, H, W, pose)
    workspace = _workspace_arg(op, workspace, int(_lib.load().tp_silhouette_align_workspace_bytes(B, H, W)), pose.device, align=16)
    from .scene import mesh_raster
    passes, hidden = [], []
    if visible_iou:
        unknown = torch.isnan(sdf)                               # [Ft,H,W]; the plane of image b by the step's frame rule
        if frame is not None:
            unknown = unknown[frame.clamp(0, sdf.shape[0] - 1).long()]
    raster = lambda P: mesh_raster(verts, faces, P, intr, H=H, W=W, face_ids=False, normals=False, cull=cull)

    def step(r, P, t, last):
        passes.append(silhouette_align_step(r["zbuf"], P, intr, sdf, tau_px=t, damping=damping, frame=frame, mask=mask, evaluate_only=last,
                                            workspace=workspace))
        if visible_iou and (len(passes) == 1 or last):
            z = r["zbuf"]
            hidden.append(((z > 0) & torch.isfinite(z) & unknown).flatten(1).sum(1))
        return passes[-1]

    res = _refine_loop(pose, taus, raster, step)
    iou = lambda r: r["inter"].float() / r["uni"].float()
    res.update(iou=iou(passes[-1]), iou0=iou(passes[0]))
    if visible_iou:
        def seen(r, h):
            left = r["uni"] - h                                  # (>= inter: a hidden pixel is covered and not inside)
            return torch.where(left == 0, torch.full_like(left, float("nan"), dtype=torch.float32), r["inter"].float() / left.float())
        res.update(iou_visible=seen(passes[-1], hidden[-1]), iou0_visible=seen(passes[0], hidden[0]))
    return res


# ------------------------------------------------------------------------------------------ K33
JOINT_TERMS = ("silhouette", "photo", "depth")           # the order of the weights and of the sum; their result prefixes:
_JOINT_PREFIX = {"silhouette": "sil_", "photo": "photo_", "depth": "icp_"}
# 1 / sigma^2 per residual unit (pixels, colour units, mm).  w_photo = 100 is the only one of 25, 100 and 400 with which the twelve
# occluded cases of DESIGN section 23 all converged; w_icp = 1 / 25 is sigma = 5 mm and is NOT tuned on anything.
JOINT_WEIGHTS = (1.0, 100.0, 1.0 / 25.0)


def _joint_weights(op: str, weights) -> tuple:
    try:
        w = tuple(float(x) for x in weights)
    except TypeError:
        w = ()
    if len(w) != 3:
        raise ValueError("%s: weights must be three host values (silhouette, photo, depth), got %r" % (op, weights))
    if not all(x >= 0.0 and x != float("inf") for x in w):
        raise ValueError("%s: weights must be finite and not negative, got %r" % (op, w))
    return w


def joint_align_workspace(B: int, H: int, W: int, device, terms: int = 3) -> Tensor:
    """A workspace for joint_align_step / joint_align at B images of H x W with ``terms`` terms present (each term's own
    ``*_workspace_bytes``, one after the other); needs no clearing."""
    lib = _lib.load()
    sizes = (lib.tp_silhouette_align_workspace_bytes, lib.tp_photo_align_workspace_bytes, lib.tp_depth_icp_workspace_bytes)
    return _workspace_arg("joint_align", None, sum(int(f(B, H, W)) for f in sizes[:int(terms)]), device)


@_on_tensor_device
def joint_align_step(pose: Tensor, intr: Tensor, *, silhouette: Optional[dict] = None, photo: Optional[dict] = None, depth: Optional[dict] = None,
                     weights=JOINT_WEIGHTS, damping: float = 1e-6, evaluate_only: bool = False, out: Optional[Dict[str, Tensor]] = None,
                     workspace: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """One JOINT Gauss-Newton step for B poses: the rows of the silhouette, the photometric and the depth term in one normal system
    (tp_joint_align_step, K33; the rules are in the header).  pose [B,3,4], intr [B,3,3] or one [3,3]; each term that takes part is a
    dict of that term's own step arguments (planes rendered at ``pose``, threshold, and optionally ``frame`` and ``mask``):
    ``silhouette`` = dict(zbuf, sdf, tau_px), ``photo`` = dict(zbuf, rgb, image, tau), ``depth`` = dict(verts, faces, zbuf, face, depth,
    tau_mm).  ``weights`` (w_sil, w_photo, w_icp): 1 / sigma^2 of the term's residual unit; a present term with weight 0 is evaluated
    but takes no part in the step.  -> 'pose' [B,3,4] (the stepped pose; ``pose`` itself, bit for bit, with ``evaluate_only`` or a
    non-zero status), 'status' [B] int32 (0 ok, 1 fewer than 6 kept pixels over the weighted terms, 3 not positive definite),
    'inliers' [B] int32 (their kept pixels, added), 'chi2' [B] (the weighted sum of squares), and per present term that term's own
    evaluation of ``pose``, bit for bit its ``*_step(evaluate_only=True)``: 'sil_inliers', 'sil_rms', 'sil_status', 'sil_inter',
    'sil_uni', 'photo_inliers', 'photo_rms', 'photo_status', 'icp_inliers', 'icp_rms', 'icp_status'.  ``workspace``:
    joint_align_workspace(B, H, W, terms present); ``out``: any of these tensors to write into (out['pose'] must not be ``pose``).
    With one term at weight 1 'pose' and 'status' are that term's own step's bit for bit.  Each term's launches and one more, no
    atomics, bit-identical from run to run, safe under torch.cuda.graph."""
    op = "joint_align_step"
    w = _joint_weights(op, weights)
    given = dict(zip(JOINT_TERMS, (silhouette, photo, depth)))
    if all(v is None for v in given.values()):
        raise ValueError("%s: no term: give at least one of silhouette=, photo=, depth=" % op)
    if not any(v is not None and x > 0 for v, x in zip(given.values(), w)):
        raise ValueError("%s: no present term has a weight > 0 (weights %r)" % (op, w))
    pose = _poses(op, pose, "pose")
    B = pose.shape[0]
    intr = _intr_per_view(op, intr, B)
    shapes = {name: tuple(t["zbuf"].shape) if torch.is_tensor(t.get("zbuf")) else None for name, t in given.items() if t is not None}
    shape = next(iter(shapes.values()))
    if len(set(shapes.values())) != 1 or shape is None or len(shape) != 3:
        raise ValueError("%s: every term needs a zbuf [B,H,W] of one shape, got %r" % (op, shapes))
    H, W = shape[1:]
    dev = pose.device
    lib = _lib.load()
    sizes = dict(zip(JOINT_TERMS, (lib.tp_silhouette_align_workspace_bytes, lib.tp_photo_align_workspace_bytes, lib.tp_depth_icp_workspace_bytes)))
    need = {name: (int(sizes[name](B, H, W)) + 15) // 16 * 16 for name in shapes}
    workspace = _workspace_arg(op, workspace, sum(need.values()), dev, align=16)
    raw, offset = workspace.view(torch.uint8).reshape(-1), 0
    builders = dict(silhouette=(_silhouette_align_args, ("zbuf",), ("sdf",), "tau_px"), photo=(_photo_align_args, ("zbuf", "rgb"), ("image",), "tau"),
                    depth=(_depth_icp_args, ("verts", "faces", "zbuf", "face"), ("depth",), "tau_mm"))
    res, structs, alive = {}, {}, [workspace]
    for name in JOINT_TERMS:
        t = given[name]
        if t is None:
            structs[name] = None
            continue
        build, before, after, tau_name = builders[name]
        unknown = set(t) - set(before) - set(after) - {tau_name, "frame", "mask"}
        missing = [k for k in before + after + (tau_name,) if k not in t]
        if unknown or missing:
            raise ValueError("%s: the %s term takes %s, frame and mask; missing %s, unknown %s"
                             % (op, name, ", ".join(before + after + (tau_name,)), missing, sorted(unknown)))
        prefix = _JOINT_PREFIX[name]
        term_out = None if out is None else {k[len(prefix):]: v for k, v in out.items() if k.startswith(prefix)}
        a, r, keep = build("%s (%s)" % (op, name), *[t[k] for k in before], pose, intr, *[t[k] for k in after], **{tau_name: t[tau_name]},
                           damping=damping, frame=t.get("frame"), mask=t.get("mask"), evaluate_only=True,
                           workspace=raw[offset:offset + need[name]], out=term_out, with_pose=False)
        offset += need[name]
        structs[name] = a
        alive.append(keep)
        res.update({prefix + k: v for k, v in r.items()})
    joint = _outputs(op, None if out is None else {k: v for k, v in out.items() if k in ("pose", "status", "inliers", "chi2")},
                     {"pose": (torch.float32, (B, 3, 4)), "status": (torch.int32, (B,)), "inliers": (torch.int32, (B,)), "chi2": (torch.float32, (B,))},
                     dev, partial=True)
    j = _lib.JointAlignArgs()
    j.B, j.pose, j.w_sil, j.w_photo, j.w_icp, j.damping, j.evaluate_only = B, pose.data_ptr(), w[0], w[1], w[2], float(damping), int(bool(evaluate_only))
    j.pose_out, j.status, j.inliers, j.chi2 = joint["pose"].data_ptr(), joint["status"].data_ptr(), joint["inliers"].data_ptr(), joint["chi2"].data_ptr()
    _call("tp_joint_align_step", j, structs["silhouette"], structs["photo"], structs["depth"])
    return dict(joint, **res)


JOINT_ALIGN_KEYS = ("pose", "inliers", "chi2", "status", "inliers0", "chi20")


@_on_tensor_device
def joint_align(verts: Tensor, faces: Tensor, pose: Tensor, intr: Tensor, *, vcolor: Optional[Tensor] = None, sdf: Optional[Tensor] = None,
                image: Optional[Tensor] = None, depth: Optional[Tensor] = None, weights=JOINT_WEIGHTS, tau_px=4.0, tau=0.5, tau_mm=20.0,
                iters: int = 20, damping: float = 1e-6, frame: Optional[Tensor] = None, masks: Optional[dict] = None,
                workspace: Optional[Tensor] = None, visible_iou: bool = False, cull: bool = False,
                texels: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """Refine B poses of one mesh against whichever of the measured outline (``sdf`` [Ft,H,W], mask_sdf's field), the photograph
    (``image`` [Ft,H,W,3], with the mesh's ``vcolor`` [V,3]) and the measured depth (``depth`` [Ft,H,W], mm) are given, ALL rows in
    one Gauss-Newton system per step (K33): ``iters`` + 1 passes of ONE mesh_raster call at the current poses, asked
    only for the planes the present terms need, followed by joint_align_step, the last with evaluate_only.  The outline gives the
    basin, the texture or the depth pins what the outline leaves loose: under occlusion the terms run one after the other end far
    away where this loop converges.  ``weights`` (w_sil, w_photo, w_icp) = 1 / sigma^2 per residual unit, default (1, 100, 1 / 25):
    w_photo = 100 is the only one of 25, 100 and 400 with which all twelve occluded cases of DESIGN section 23 converged; w_icp is
    sigma = 5 mm and is NOT tuned on anything.  ``tau_px`` / ``tau`` / ``tau_mm``: each term's threshold, one value or ``iters`` + 1
    host values.  ``frame`` [B] int32: the measured plane of each pose, for every term.  ``masks``: dict(silhouette=, photo=, depth=)
    of [Ft,H,W] uint8 / bool planes (0: the term skips the pixel).  -> 'pose' [B,3,4], its 'inliers' [B] int32 and 'chi2' [B],
    'status' [B] int32 of the last step taken (of the evaluation where iters = 0), 'inliers0' / 'chi20' of the start pose, and the
    last pass's per-term keys of joint_align_step; with ``sdf`` also 'iou' / 'iou0', and with ``visible_iou`` 'iou_visible' /
    'iou0_visible', as silhouette_align.  A step that fails passes its pose on.  Bit-identical from run to run, safe under
    torch.cuda.graph.  ``cull``: the passes render with mesh_raster(cull=True), same bits.  ``texels`` [F,T,3] in place of ``vcolor``:
    the photometric term's renders take their colour from the mesh's face texels (mesh_raster(texels=), K35); at most one of the two."""
    op = "joint_align"
    if vcolor is not None and texels is not None:
        raise ValueError("%s: vcolor= or texels=, not both" % op)
    w = _joint_weights(op, weights)
    iters = int(iters)
    taus = list(zip(_tau_schedule(op, tau_px, "tau_px", iters), _tau_schedule(op, tau, "tau", iters), _tau_schedule(op, tau_mm, "tau_mm", iters)))
    if sdf is None and image is None and depth is None:
        raise ValueError("%s: no term: give at least one of sdf=, image=, depth=" % op)
    if image is not None and vcolor is None and texels is None:
        raise ValueError("%s: image= needs vcolor=, the mesh's colours [V,3], or texels= [F,T,3]" % op)
    masks = dict(masks or {})
    if set(masks) - set(JOINT_TERMS):
        raise ValueError("%s: masks takes the keys %s, got %s" % (op, JOINT_TERMS, sorted(masks)))
    verts, pose = _points(op, verts, "verts"), _poses(op, pose, "pose")
    B = pose.shape[0]
    faces = faces.to(device=verts.device, dtype=torch.int32).contiguous()
    intr = _intr_per_view(op, intr, B)
    planes = {}
    for name, t, trailing in (("sdf", sdf, ()), ("image", image, (3,)), ("depth", depth, ())):
        if t is None:
            continue
        t = _f32(t.detach(), name)
        t = t[None] if t.dim() == 2 + len(trailing) else t
        if t.dim() != 3 + len(trailing) or t.numel() == 0 or tuple(t.shape[3:]) != trailing:
            raise ValueError("%s: %s [Ft,H,W%s] expected, got %s" % (op, name, ",3" if trailing else "", tuple(t.shape)))
        planes[name] = t
    sizes = {tuple(t.shape[1:3]) for t in planes.values()}
    if len(sizes) != 1:
        raise ValueError("%s: the measured planes must be of one size H x W, got %s" % (op, {k: tuple(v.shape) for k, v in planes.items()}))
    H, W = sizes.pop()
    term_of = dict(sdf="silhouette", image="photo", depth="depth")
    for name, trailing in (("sdf", ()), ("image", (3,)), ("depth", ())):
        if name in planes:
            planes[name], _, masks[term_of[name]], _ = _frame_planes(op, name, planes[name], trailing, frame, masks.get(term_of[name]), B, H, W, pose)
    if vcolor is not None:
        vcolor = _f32(vcolor.detach(), "vcolor")
    if texels is not None:
        texels = _f32(texels.detach(), "texels")
    lib = _lib.load()
    need = sum((int(f(B, H, W)) + 15) // 16 * 16 for f, name in ((lib.tp_silhouette_align_workspace_bytes, "sdf"), (lib.tp_photo_align_workspace_bytes, "image"),
                                                                 (lib.tp_depth_icp_workspace_bytes, "depth")) if name in planes)
    workspace = _workspace_arg(op, workspace, need, pose.device, align=16)
    from .scene import mesh_raster
    raster = lambda P: mesh_raster(verts, faces, P, intr, H=H, W=W, vcolor=vcolor if "image" in planes else None,
                                   texels=texels if "image" in planes else None, face_ids="depth" in planes, normals=False, cull=cull)
    passes, hidden = [], []
    if visible_iou:
        if "sdf" not in planes:
            raise ValueError("%s: visible_iou needs sdf=" % op)
        unknown = torch.isnan(planes["sdf"])
        if frame is not None:
            unknown = unknown[frame.clamp(0, planes["sdf"].shape[0] - 1).long()]

    def step(r, P, t, last):
        terms = {}
        if "sdf" in planes:
            terms["silhouette"] = dict(zbuf=r["zbuf"], sdf=planes["sdf"], tau_px=t[0], frame=frame, mask=masks.get("silhouette"))
        if "image" in planes:
            terms["photo"] = dict(zbuf=r["zbuf"], rgb=r["rgb"], image=planes["image"], tau=t[1], frame=frame, mask=masks.get("photo"))
        if "depth" in planes:
            terms["depth"] = dict(verts=verts, faces=faces, zbuf=r["zbuf"], face=r["face"], depth=planes["depth"], tau_mm=t[2], frame=frame,
                                  mask=masks.get("depth"))
        got = joint_align_step(P, intr, weights=w, damping=damping, evaluate_only=last, workspace=workspace, **terms)
        got["rms"] = got["chi2"]                                 # (_refine_loop's name for the cost it carries)
        passes.append(got)
        if visible_iou and (len(passes) == 1 or last):
            z = r["zbuf"]
            hidden.append(((z > 0) & torch.isfinite(z) & unknown).flatten(1).sum(1))
        return got

    res = _refine_loop(pose, taus, raster, step)
    res["chi2"], res["chi20"] = res.pop("rms"), res.pop("rms0")
    res.update({k: v for k, v in passes[-1].items() if k.startswith(tuple(_JOINT_PREFIX.values()))})
    if "sdf" in planes:
        iou = lambda r: r["sil_inter"].float() / r["sil_uni"].float()
        res.update(iou=iou(passes[-1]), iou0=iou(passes[0]))
    if visible_iou:
        def seen(r, h):
            left = r["sil_uni"] - h                              # (>= inter: a hidden pixel is covered and not inside)
            return torch.where(left == 0, torch.full_like(left, float("nan"), dtype=torch.float32), r["sil_inter"].float() / left.float())
        res.update(iou_visible=seen(passes[-1], hidden[-1]), iou0_visible=seen(passes[0], hidden[0]))
    return res
