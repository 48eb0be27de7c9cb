"""The pose-error definitions of DESIGN section 15 in numpy fp64, in this project's own words: every search is a full [P1,P2] brute
force with argmin / argmax (numpy returns the FIRST of equal values: the lowest index wins ties).  The BOP errors (ADD, ADD-S, MSSD,
MSPD) and the reference's one-directional chamfer distance `camera.p2p_distance` are restated here; nothing is pinned to a call of
bop_toolkit or PyTorch3D.  Inputs of any float dtype are taken as they are and widened: the fp32 inputs of a kernel are exact here."""
import math

import numpy as np


def f64(a):
    return np.asarray(a, dtype=np.float64)


def apply(T, pts):
    """[3,4] (or [...,3,4]) applied to [M,3] -> [...,M,3]."""
    T, pts = f64(T), f64(pts)
    return pts @ np.swapaxes(T[..., :3], -1, -2) + T[..., None, :, 3]


def nn1(x, y, x_len=None, y_len=None, A=None, mode="nearest", second=False):
    """x [Bx,P1,3], y [Bt,P2,3] (Bx, Bt: 1 or B), lengths [B] / [Bt], A [B,3,4] -> d2 [B,P1] float64, idx [B,P1] int32; with
    ``second`` also the runner-up's d2 (the best after the winner is removed; the no-winner value where there is none)."""
    x, y = f64(x), f64(y)
    far = {"nearest": False, "farthest": True}[mode]
    B = x.shape[0] if A is None else len(A)
    P1, P2 = x.shape[1], y.shape[1]
    none = -math.inf if far else math.inf
    d2, idx, d2_second = np.full((B, P1), none), np.full((B, P1), -1, np.int32), np.full((B, P1), none)
    for b in range(B):
        q = x[b if x.shape[0] > 1 else 0]
        if A is not None:
            q = apply(A[b], q)
        bt = b if y.shape[0] > 1 else 0
        n1 = P1 if x_len is None else min(max(int(x_len[b]), 0), P1)
        n2 = P2 if y_len is None else min(max(int(y_len[bt]), 0), P2)
        if n1 == 0 or n2 == 0:
            continue
        for i0 in range(0, n1, 1024):                                            # the full [n1,n2] table, 1,024 rows at a time
            sl = slice(i0, min(i0 + 1024, n1))
            raw = sum((q[sl, None, c] - y[bt, None, :n2, c]) ** 2 for c in range(3))
            live = ~np.isnan(raw)
            d = np.where(live, raw, none)
            j = d.argmax(1) if far else d.argmin(1)
            rows = np.arange(d.shape[0])
            won = live.any(1)
            d2[b, sl] = np.where(won, d[rows, j], none)
            idx[b, sl] = np.where(won, j, -1)
            d[rows, j] = none                                                    # the runner-up: the best once the winner is gone
            live[rows, j] = False
            runner = d.max(1) if far else d.min(1)
            d2_second[b, sl] = np.where(live.any(1), runner, none)
    return (d2, idx, d2_second) if second else (d2, idx)


def add(pts, pose_est, pose_gt):
    return np.sqrt(((apply(pose_est, pts) - apply(pose_gt, pts)) ** 2).sum(-1)).mean(-1)


def adds(pts, pose_est, pose_gt):
    """mean_x min_y |P_e x - P_g y|, both clouds posed (no inverse is formed)."""
    e, g = apply(pose_est, pts), apply(pose_gt, pts)
    out = np.empty(len(e))
    for b in range(len(e)):
        d2, _ = nn1(e[b][None], g[b][None])
        out[b] = np.sqrt(d2[0]).mean()
    return out


def project(X, K):
    K = f64(K)
    return np.stack([K[0, 0] * X[..., 0] / X[..., 2] + K[0, 2], K[1, 1] * X[..., 1] / X[..., 2] + K[1, 2]], -1)


def pose_errors(pts, pose_est, pose_gt, sym=None, intr=None):
    """-> dict of add, mssd [B], s_mssd [B] int32, per_sym_mssd [B,S] and, with intr [B,3,3], mspd, proj, s_mspd, per_sym_mspd."""
    pts, pose_est, pose_gt = f64(pts), f64(pose_est), f64(pose_gt)
    sym = np.eye(3, 4)[None] if sym is None else f64(sym)
    B, S = len(pose_est), len(sym)
    out = dict(add=np.empty(B), mssd=np.empty(B), s_mssd=np.empty(B, np.int32), per_sym_mssd=np.empty((B, S)))
    if intr is not None:
        out.update(mspd=np.empty(B), proj=np.empty(B), s_mspd=np.empty(B, np.int32), per_sym_mspd=np.empty((B, S)))
    for b in range(B):
        e = apply(pose_est[b], pts)
        g = np.stack([apply(pose_gt[b], apply(sym[s], pts)) for s in range(S)])             # [S,M,3]
        d3 = np.sqrt(((e[None] - g) ** 2).sum(-1))
        out["add"][b] = d3[0].mean()
        out["per_sym_mssd"][b] = d3.max(-1)
        out["s_mssd"][b] = np.argmin(out["per_sym_mssd"][b])
        out["mssd"][b] = out["per_sym_mssd"][b].min()
        if intr is not None:
            if not ((e[:, 2] > 0).all() and (g[..., 2] > 0).all()):
                out["mspd"][b] = out["proj"][b] = out["per_sym_mspd"][b] = math.nan
                out["s_mspd"][b] = -1
                continue
            with np.errstate(all="ignore"):
                d2 = np.sqrt(((project(e, intr[b])[None] - project(g, intr[b])) ** 2).sum(-1))
            out["per_sym_mspd"][b] = d2.max(-1)
            out["s_mspd"][b] = np.argmin(out["per_sym_mspd"][b])
            out["mspd"][b] = out["per_sym_mspd"][b].min()
            out["proj"][b] = d2[0].mean()
    return out


def re_te(pose_est, pose_gt):
    pose_est, pose_gt = f64(pose_est), f64(pose_gt)
    d = pose_est[:, :, :3] @ np.swapaxes(pose_gt[:, :, :3], 1, 2)
    tr = d[:, 0, 0] + d[:, 1, 1] + d[:, 2, 2]
    return np.arccos(np.clip((tr - 1) / 2, -1 + 1e-7, 1 - 1e-7)), np.linalg.norm(pose_est[:, :, 3] - pose_gt[:, :, 3], axis=-1)


def model_diameter(pts):
    d2, _ = nn1(f64(pts)[None], f64(pts)[None], mode="farthest")
    return math.sqrt(d2.max())


def p2p_distance(x, y, x_lengths=None, y_lengths=None, weights=None, batch_reduction="mean", point_reduction="mean", d2=None):
    """``d2``: nn1(x, y, x_lengths, y_lengths)[0] where the caller has it already."""
    x = f64(x)
    N, P1 = x.shape[:2]
    if weights is not None and f64(weights).sum() == 0:
        return 0.0 if batch_reduction is not None else np.zeros(N)
    if d2 is None:
        d2, _ = nn1(x, y, x_lengths, y_lengths)
    n = np.full(N, P1) if x_lengths is None else np.asarray(x_lengths)
    d2 = np.where(np.arange(P1)[None] < n[:, None], d2, 0.0)
    if weights is not None:
        d2 = d2 * f64(weights)[:, None]
    cham = d2.sum(1)
    if point_reduction == "mean":
        cham = cham / n
    if batch_reduction is None:
        return cham
    cham = cham.sum()
    return cham / (f64(weights).sum() if weights is not None else N) if batch_reduction == "mean" else cham


def rotation(axis, angle):
    k = f64(axis) / np.linalg.norm(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


def symmetry_transforms(entry, max_sym_disc_step=0.01):
    """Identity, the discrete transforms, and each of them under every step of every continuous symmetry (steps outermost);
    no subsampling here."""
    disc = [np.eye(4)] + [f64(s).reshape(4, 4) for s in entry.get("symmetries_discrete", [])]
    n = int(math.ceil(math.pi / max_sym_disc_step))
    cont = [np.eye(4)]
    for c in entry.get("symmetries_continuous", []):
        steps = []
        for i in range(n):
            T = np.eye(4)
            T[:3, :3] = rotation(c["axis"], 2 * math.pi * i / n) if i else np.eye(3)
            T[:3, 3] = f64(c["offset"]) - T[:3, :3] @ f64(c["offset"])
            steps.append(T)
        cont = [a @ s for a in cont for s in steps]
    return np.stack([c @ d for c in cont for d in disc])[:, :3]
