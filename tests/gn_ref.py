"""What the restatements of the three pose refiners (tests/pnp_ref.py, tests/icp_ref.py, tests/photo_ref.py) share, in numpy fp64 from
the rules in include/texpose_amd.h: the Cholesky with the pivot rule, the exponential map, one damped Gauss-Newton update, the
per-image part of a K29 / K30 step, their loop, and the bars the GPU tests hold a step to."""
import numpy as np

PIVOT_TOL = 1e-10
MIN_COUNT = 6


def _cholesky(A, tol):
    A = A.copy()
    for j in range(6):
        diag = A[j, j]
        d = diag - (A[j, :j] ** 2).sum()
        if not np.isfinite(d) or not d > tol * diag or not d > 0:
            return None
        A[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            A[i, j] = (A[i, j] - A[i, :j] @ A[j, :j]) / A[j, j]
    return np.tril(A)


def _exp_so3(w):
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    sa, sb = (np.sin(th) / th, (1 - np.cos(th)) / th ** 2) if th > 1e-8 else (1 - th * th / 6, 0.5 - th * th / 24)
    return np.eye(3) + sa * Wx + sb * (Wx @ Wx)


def gn_update(JtJ, Jtr, cur, lam):
    """One damped step from the pose cur [3,4] (fp64): J^T J must pass the pivot rule, (J^T J + lam diag J^T J) d = -J^T r, R <-
    exp(w) R, t <- exp(w) t + v, Gram-Schmidt -> the new pose [3,4] fp64, or None where a factorisation fails or it is not finite."""
    L = _cholesky(JtJ, PIVOT_TOL)
    Ld = _cholesky(JtJ + lam * np.diag(np.diag(JtJ)), 0.0) if L is not None else None
    if Ld is None:
        return None
    d = np.linalg.solve(Ld.T, np.linalg.solve(Ld, -Jtr))
    P = _exp_so3(d[:3]) @ cur
    P[:, 3] += d[3:]
    c1 = P[:, 0] / np.linalg.norm(P[:, 0])
    c2 = P[:, 1] - c1 * (c1 @ P[:, 1])
    c2 /= np.linalg.norm(c2)
    P[:, 0], P[:, 1], P[:, 2] = c1, c2, np.cross(c1, c2)
    return P if np.isfinite(P).all() else None


def solve_ref(s, pose, damping, evaluate_only):
    """The per-image part of a K29 / K30 step: sums (JtJ, Jtr, cost, count) -> (pose_out fp32 [3,4], inliers, rms, status)."""
    pose32 = np.asarray(pose, np.float32).reshape(3, 4)
    with np.errstate(all="ignore"):
        rms = np.sqrt(np.float64(s["cost"]) / np.float64(s["count"]))
    if s["count"] < MIN_COUNT:
        return pose32.copy(), s["count"], rms, 1
    if _cholesky(s["JtJ"], PIVOT_TOL) is None:
        return pose32.copy(), s["count"], rms, 3
    if evaluate_only:
        return pose32.copy(), s["count"], rms, 0
    Pn = gn_update(s["JtJ"], s["Jtr"], pose32.astype(np.float64), float(np.float32(damping)))
    with np.errstate(all="ignore"):
        new32 = None if Pn is None else Pn.astype(np.float32)
    if new32 is None or not np.isfinite(new32).all():
        return pose32.copy(), s["count"], rms, 3
    return new32, s["count"], rms, 0


def loop_ref(render, step, pose, tau, iters):
    """The loop of ops.depth_icp / ops.photo_align: iters + 1 passes of render(pose [B,3,4]) -> planes and step(planes, pose, tau,
    evaluate_only) -> a step_ref dict, the pose rounded to fp32 between them, the last evaluate-only -> dict(pose [B,3,4] float32,
    inliers, rms, status (of the last step taken), inliers0, rms0, near_ties (largest over the passes))."""
    pose = np.asarray(pose, np.float32).copy()
    taus = [float(tau)] * (iters + 1) if np.isscalar(tau) else [float(t) for t in tau]
    assert len(taus) == iters + 1
    first, status, ties, r = None, None, np.zeros(len(pose), np.int64), None
    for it, t in enumerate(taus):
        r = step(render(pose), pose, t, it == iters)
        first = r if first is None else first
        status = r["status"] if it < iters or status is None else status
        ties = np.maximum(ties, r["near_ties"])
        pose = r["pose"]
    return dict(pose=r["pose"], inliers=r["inliers"], rms=r["rms"], status=status, inliers0=first["inliers"], rms0=first["rms"], near_ties=ties)


# ----------------------------------------------------------------------------------------------------------------- the GPU tests' side
def cu(x, dtype=None, device="cuda:0"):
    import torch
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x, dtype=dtype).to(device)


def host(t):
    return t.detach().cpu().numpy()


def compare(got, want, pose_in):
    """The bars of a K29 / K30 step against its restatement (fp64 sums, then fp32): counts and statuses equal, rms to 1e-5 relative,
    the pose to 1e-5 in R's entries and in t relative; a failed step returns its input bit for bit."""
    assert (want["near_ties"] == 0).all(), "a near-tie in the case: change its seed"
    assert np.array_equal(host(got["inliers"]), want["inliers"]), (host(got["inliers"]), want["inliers"])
    assert np.array_equal(host(got["status"]), want["status"]), (host(got["status"]), want["status"])
    rms = host(got["rms"]).astype(np.float64)
    assert np.array_equal(np.isnan(rms), np.isnan(want["rms"]))
    ok = ~np.isnan(rms)
    assert (np.abs(rms[ok] - want["rms"][ok]) <= 1e-5 * want["rms"][ok] + 1e-30).all(), (rms, want["rms"])
    pose = host(got["pose"])
    for b in range(len(pose)):
        if want["status"][b] != 0:
            assert np.array_equal(pose[b].view(np.uint32), np.asarray(pose_in[b], np.float32).view(np.uint32)), b
        else:
            assert np.abs(pose[b, :, :3] - want["pose"][b, :, :3]).max() <= 1e-5, b
            assert np.abs(pose[b, :, 3] - want["pose"][b, :, 3]).max() <= 1e-5 * np.abs(want["pose"][b, :, 3]).max(), b
