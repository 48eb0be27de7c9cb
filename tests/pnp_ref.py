"""The PnP-RANSAC contract of DESIGN section 18 (kernels K28: tp_corr_from_nocs, tp_pnp_hypotheses, tp_pnp_score, tp_pnp_refine), said
again in numpy -- written from the rules in include/texpose_amd.h, not from the kernels.  Where the kernels are free to choose, this
file chooses differently: the P3P quartic is assembled with np.polymul and solved with np.roots (the kernel expands it by hand and
uses Ferrari's closed form), and the two triangles are aligned with an SVD (the kernel uses orthonormal frames).

Besides the results it reports what decides whether a comparison with fp32 / differently ordered arithmetic can be exact:
near-ties (entries whose reprojection error is within NEAR_TIE px of tau) and ill-conditioned minimal samples (image triangle below
1 px^2, or two roots of the quartic closer than 1e-6 relative)."""
import math

import numpy as np

from gn_ref import PIVOT_TOL, _cholesky, _exp_so3, gn_update  # noqa: F401  (tests reach them through this module)
from oracle.texpose_oracle import LINEMOD_K, philox4x32

NEAR_TIE = 1e-3          # px
LAMBDA = 1e-3
PNP4 = 0x706E7034        # 'pnp4'


# ----------------------------------------------------------------------------------------------------------------- corr_from_nocs
def corr_from_nocs_ref(nocs, mask, centre, scale, stride):
    """nocs [B,H,W,3] float32, mask [B,H,W] -> (xy [B,N,2], xyz [B,N,3] float32 (zeros past count), count [B] int32)."""
    nocs = np.asarray(nocs, np.float32)
    B, H, W, _ = nocs.shape
    centre, scale = np.asarray(centre, np.float32), np.asarray(scale, np.float32)
    Hs, Ws = -(-H // stride), -(-W // stride)
    N = Hs * Ws
    xy, xyz, count = np.zeros((B, N, 2), np.float32), np.zeros((B, N, 3), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        r, j = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
        r, j = r.reshape(-1), j.reshape(-1)                          # ascending r * W + j
        q = nocs[b, r, j]
        keep = (np.asarray(mask)[b, r, j] != 0) & np.isfinite(q).all(-1)
        r, j, q = r[keep], j[keep], q[keep]
        n = len(r)
        count[b] = n
        xy[b, :n, 0] = j.astype(np.float32) + np.float32(0.5)
        xy[b, :n, 1] = r.astype(np.float32) + np.float32(0.5)
        xyz[b, :n] = (np.float32(2.0) * q - np.float32(1.0)) * scale + centre
    return xy, xyz, count


# ----------------------------------------------------------------------------------------------------------------- sampling
def sample_indices(seed, b, T, n):
    """[T,4] int32: the four distinct indices of the hypotheses 0 .. T-1 of image b at n usable entries (four -1 where n < 4)."""
    if n < 4:
        return np.full((T, 4), -1, np.int32)
    ctr = np.zeros((T, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = b, np.arange(T), PNP4
    w = philox4x32(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).astype(np.uint64)
    raw = np.stack([(w[:, k] * np.uint64(n - k)) >> np.uint64(32) for k in range(4)], 1).astype(np.int64)
    out = np.zeros((T, 4), np.int32)
    for h in range(T):
        chosen = []
        for k in range(4):
            i = int(raw[h, k])
            for e in sorted(chosen):
                if i >= e:
                    i += 1
            chosen.append(i)
        out[h] = chosen
    return out


def clamp_counts(count, N):
    return np.clip(np.asarray(count, np.int64), 0, N)


# ----------------------------------------------------------------------------------------------------------------- P3P
def _kabsch(Xm, Pc):
    """The rigid motion taking the model triangle Xm [3,3] onto the camera triangle Pc [3,3] (rows are points)."""
    mx, mp = Xm.mean(0), Pc.mean(0)
    Hm = (Xm - mx).T @ (Pc - mp)
    # a triangle is planar: complete the rank-2 problem with the two normals
    nx, npc = np.cross(Xm[1] - Xm[0], Xm[2] - Xm[0]), np.cross(Pc[1] - Pc[0], Pc[2] - Pc[0])
    Hm = Hm + np.outer(nx / np.linalg.norm(nx), npc / np.linalg.norm(npc)) * np.trace(np.abs(Hm))
    U, _, Vt = np.linalg.svd(Hm)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, mp - R @ mx


def p3p_ref(uv, X, K):
    """uv [4,2], X [4,3] (fp64), K [3,3] -> dict(valid, pose [3,4], ill, depths, n_real): the P3P solution of the first three points
    with the smallest reprojection error on the fourth, by the header's rules."""
    out = dict(valid=False, pose=np.zeros((3, 4)), ill=False, depths=None, n_real=0)
    uv, X, K = np.asarray(uv, np.float64), np.asarray(X, np.float64), np.asarray(K, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    if not (np.isfinite(uv).all() and np.isfinite(X).all() and np.isfinite([fx, fy, cx, cy]).all()):
        return out
    e12, e13 = uv[1] - uv[0], uv[2] - uv[0]
    area2 = abs(e12[0] * e13[1] - e13[0] * e12[1])
    out["ill"] = bool(0.5 * area2 < 1.0)
    if not area2 > 1e-9 * (e12 @ e12 + e13 @ e13):
        return out
    f = np.stack([(uv[:3, 0] - cx) / fx, (uv[:3, 1] - cy) / fy, np.ones(3)], 1)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        a2, b2, c2 = ((X[1] - X[2]) ** 2).sum(), ((X[0] - X[2]) ** 2).sum(), ((X[0] - X[1]) ** 2).sum()
        ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
        k1, kc = (a2 - c2) / b2, c2 / b2
        Nn = np.array([k1 - 1.0, -2.0 * k1 * cb, 1.0 + k1])          # highest power first
        Dd = np.array([-2.0 * ca, 2.0 * cg])
        Wv = np.array([-kc, 2.0 * kc * cb, 1.0 - kc])
        quartic = np.polyadd(np.polysub(np.polymul(Nn, Nn), 2.0 * cg * np.polymul(Nn, Dd)), np.polymul(np.polymul(Dd, Dd), Wv))
    if not np.isfinite(quartic).all() or len(quartic) != 5 or quartic[0] == 0.0:
        return out
    roots = np.roots(quartic)
    for i in range(len(roots)):
        for j in range(i):
            if abs(roots[i] - roots[j]) <= 1e-6 * max(abs(roots[i]), abs(roots[j])):
                out["ill"] = True
    best = None
    for z in roots:
        if abs(z.imag) > 1e-7 * max(1.0, abs(z.real)):
            continue
        v = z.real
        out["n_real"] += 1
        with np.errstate(all="ignore"):
            u = np.polyval(Nn, v) / np.polyval(Dd, v)
            s1 = np.sqrt(b2 / (1.0 + v * v - 2.0 * v * cb))
        if not (v > 0 and u > 0 and s1 > 0 and np.isfinite([u, v, s1]).all()):
            continue
        depths = np.array([s1, u * s1, v * s1])
        R, t = _kabsch(X[:3], f * depths[:, None])
        if not (np.isfinite(R).all() and np.isfinite(t).all()):
            continue
        x4 = R @ X[3] + t
        err = np.inf
        if x4[2] > 0:
            err = (fx * x4[0] / x4[2] + cx - uv[3, 0]) ** 2 + (fy * x4[1] / x4[2] + cy - uv[3, 1]) ** 2
            err = err if np.isfinite(err) else np.inf
        if best is None or (err, v) < best[0]:
            best = ((err, v), R, t, depths)
    if best is None:
        return out
    pose = np.concatenate([best[1], best[2][:, None]], 1)
    if not np.isfinite(pose.astype(np.float32)).all():
        return out
    out.update(valid=True, pose=pose, depths=best[3])
    return out


def hypotheses_ref(xy, xyz, count, intr, T, seed):
    """-> dict(sample_idx [B,T,4], hyp [B,T,3,4] fp64, valid [B,T] bool, ill [B,T] bool)."""
    B, N = xy.shape[:2]
    n = clamp_counts(count, N)
    idx = np.stack([sample_indices(seed, b, T, int(n[b])) for b in range(B)])
    hyp, valid, ill = np.zeros((B, T, 3, 4)), np.zeros((B, T), bool), np.zeros((B, T), bool)
    for b in range(B):
        if n[b] < 4:
            continue
        for h in range(T):
            r = p3p_ref(xy[b, idx[b, h]], xyz[b, idx[b, h]], intr[b])
            hyp[b, h], valid[b, h], ill[b, h] = r["pose"], r["valid"], r["ill"]
    return dict(sample_idx=idx, hyp=hyp, valid=valid, ill=ill)


# ----------------------------------------------------------------------------------------------------------------- score
def score_ref(xy, xyz, count, intr, poses, tau, valid=None, want_mask=False):
    """The scoring rule in numpy fp32, operation by operation as the header writes it: inliers [B,T] int32, and per image the
    largest number of near-ties (fp64 error within NEAR_TIE px of tau) any pose has."""
    xy, xyz, intr = np.asarray(xy, np.float32), np.asarray(xyz, np.float32), np.asarray(intr, np.float32)
    poses = np.asarray(poses, np.float32).reshape(xy.shape[0], -1, 12)
    B, N = xy.shape[:2]
    T = poses.shape[1]
    n = clamp_counts(count, N)
    tau32 = np.float32(tau)
    tau2 = tau32 * tau32
    inl, ties = np.zeros((B, T), np.int32), np.zeros(B, np.int64)
    masks = np.zeros((B, T, N), bool) if want_mask else None
    with np.errstate(all="ignore"):
        for b in range(B):
            u, v = xy[b, :n[b], 0], xy[b, :n[b], 1]
            X, Y, Z = xyz[b, :n[b], 0], xyz[b, :n[b], 1], xyz[b, :n[b], 2]
            fx, fy, cx, cy = intr[b, 0, 0], intr[b, 1, 1], intr[b, 0, 2], intr[b, 1, 2]
            for h in range(T):
                if valid is not None and not valid[b, h]:
                    continue
                P = poses[b, h]
                x = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3]
                y = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7]
                z = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11]
                du = ((fx * x) / z + cx) - u
                dv = ((fy * y) / z + cy) - v
                ok = (z > 0) & np.isfinite(z) & (du * du + dv * dv <= tau2)
                inl[b, h] = ok.sum()
                if want_mask:
                    masks[b, h, :n[b]] = ok
                P64 = P.astype(np.float64)
                x64 = np.stack([X, Y, Z], 1).astype(np.float64) @ P64.reshape(3, 4)[:, :3].T + P64.reshape(3, 4)[:, 3]
                e = np.hypot(float(fx) * x64[:, 0] / x64[:, 2] + float(cx) - u, float(fy) * x64[:, 1] / x64[:, 2] + float(cy) - v)
                ties[b] = max(ties[b], int((np.abs(e - float(tau32)) <= NEAR_TIE).sum()))
    return (inl, ties, masks) if want_mask else (inl, ties)


# ----------------------------------------------------------------------------------------------------------------- refine
def _sums(xy, xyz, K, pose, tau):
    """J^T J [6,6], J^T r [6], sum |r|^2, count and the near-tie number of `pose` [3,4] over the given entries, in fp64."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    with np.errstate(all="ignore"):
        x = xyz @ pose[:, :3].T + pose[:, 3]
        z = x[:, 2]
        ru, rv = fx * x[:, 0] / z + cx - xy[:, 0], fy * x[:, 1] / z + cy - xy[:, 1]
        e2 = ru * ru + rv * rv
        ok = (z > 0) & np.isfinite(z) & (e2 <= tau * tau)
        ties = int(((z > 0) & (np.abs(np.sqrt(e2) - tau) <= NEAR_TIE)).sum())
    x, ru, rv = x[ok], ru[ok], rv[ok]
    iz = 1.0 / x[:, 2]
    xz, yz = x[:, 0] * iz, x[:, 1] * iz
    o = np.zeros_like(iz)
    Ju = np.stack([-fx * xz * yz, fx + fx * xz * xz, -fx * yz, fx * iz, o, -fx * xz * iz], 1)
    Jv = np.stack([-fy - fy * yz * yz, fy * xz * yz, fy * xz, o, fy * iz, -fy * yz * iz], 1)
    J = np.concatenate([Ju, Jv])
    r = np.concatenate([ru, rv])
    return J.T @ J, J.T @ r, float(r @ r), int(ok.sum()), ties


def refine_ref(xy, xyz, n, K, pose0, tau, iters):
    """One image: entries 0 .. n-1, start pose [3,4] -> dict(pose fp64, inliers, rms, status, near_ties: the largest near-tie number
    over the poses evaluated)."""
    xy, xyz, K = np.asarray(xy, np.float32)[:n].astype(np.float64), np.asarray(xyz, np.float32)[:n].astype(np.float64), np.asarray(K, np.float32).astype(np.float64)
    tau = float(np.float32(tau))
    cur = np.asarray(pose0, np.float32).astype(np.float64).reshape(3, 4)
    best, best_key, status, ties = cur.copy(), None, 0, 0
    for it in range(iters + 1):
        JtJ, Jtr, cost, count, t = _sums(xy, xyz, K, cur, tau)
        ties = max(ties, t)
        if best_key is None or count > best_key[0] or (count == best_key[0] and cost < best_key[1]):
            best, best_key = cur.copy(), (count, cost)
        if it == iters:
            break
        P = gn_update(JtJ, Jtr, cur, LAMBDA)
        if P is None:
            status = 3
            break
        cur = P
    count, cost = best_key
    with np.errstate(all="ignore"):
        rms = np.sqrt(np.float64(cost) / np.float64(count))
    return dict(pose=best, inliers=count, rms=rms, status=status, near_ties=ties)


def select_ref(inliers, valid):
    """The winner per image: the valid hypothesis with the largest count, the lowest h among equals; -1 without a valid one."""
    out = np.full(inliers.shape[0], -1, np.int64)
    for b in range(inliers.shape[0]):
        hs = np.nonzero(valid[b])[0]
        if len(hs):
            out[b] = hs[np.argmax(inliers[b, hs])]                   # (argmax returns the first maximum)
    return out


def ransac_ref(xy, xyz, count, intr, T=256, tau=2.0, iters=5, seed=0):
    """The whole chain -> dict(pose [B,3,4] fp64 (NaN at status 1 / 2), pose32: the same after the final fp32 store, inliers, rms,
    status, winner, near_ties)."""
    B, N = xy.shape[:2]
    n = clamp_counts(count, N)
    hy = hypotheses_ref(xy, xyz, count, intr, T, seed)
    inl, _ = score_ref(xy, xyz, count, intr, hy["hyp"].astype(np.float32), tau, hy["valid"])
    win = select_ref(inl, hy["valid"])
    out = dict(pose=np.full((B, 3, 4), np.nan), inliers=np.zeros(B, np.int64), rms=np.full(B, np.nan), status=np.zeros(B, np.int64),
               winner=win, near_ties=np.zeros(B, np.int64), hyp=hy)
    for b in range(B):
        if n[b] < 4:
            out["status"][b] = 1
        elif win[b] < 0:
            out["status"][b] = 2
        else:
            r = refine_ref(xy[b], xyz[b], int(n[b]), intr[b], hy["hyp"][b, win[b]].astype(np.float32), tau, iters)
            out["pose"][b], out["inliers"][b], out["rms"][b], out["status"][b], out["near_ties"][b] = r["pose"], r["inliers"], r["rms"], r["status"], r["near_ties"]
    out["pose32"] = out["pose"].astype(np.float32)
    return out


def pose_error(pose, truth):
    """(rotation error in degrees, translation error in mm) of pose [3,4] against truth [3,4].  The angle comes from atan2 of the
    skew part and the trace of R R_truth^T: arccos of the trace alone cannot resolve angles below ~1e-6 deg in fp64 (and reads 0)."""
    pose, truth = np.asarray(pose, np.float64), np.asarray(truth, np.float64)
    M = pose[:, :3] @ truth[:, :3].T
    sin = 0.5 * np.linalg.norm([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    return float(np.degrees(np.arctan2(sin, (np.trace(M) - 1.0) / 2.0))), float(np.linalg.norm(pose[:, 3] - truth[:, 3]))


# ----------------------------------------------------------------------------------------------------------------- end-to-end case
def _uv_sphere(n_lat, n_lon, radius=50.0, ripple=0.0):
    th, ph = np.linspace(0, math.pi, n_lat + 1), np.linspace(0, 2 * math.pi, n_lon, endpoint=False)
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = radius * (1 + ripple * np.sin(5 * T) * np.cos(3 * P))
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.sin(T) * np.sin(P), r * np.cos(T)], -1).reshape(-1, 3)
    idx = np.arange((n_lat + 1) * n_lon).reshape(n_lat + 1, n_lon)
    a, b, c, d = idx[:-1], np.roll(idx[:-1], -1, axis=1), idx[1:], np.roll(idx[1:], -1, axis=1)
    f = np.concatenate([np.stack([a, c, d], -1)[:-1], np.stack([a, d, b], -1)[1:]]).reshape(-1, 3)
    return v.astype(np.float32), f.astype(np.int32)


def _torus(n_major, n_minor, R=45.0, r=16.0):
    u, w = np.linspace(0, 2 * math.pi, n_major, endpoint=False), np.linspace(0, 2 * math.pi, n_minor, endpoint=False)
    U, Wm = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(Wm)) * np.cos(U), (R + r * np.cos(Wm)) * np.sin(U), r * np.sin(Wm)], -1).reshape(-1, 3)
    idx = np.arange(n_major * n_minor).reshape(n_major, n_minor)
    a, b = idx, np.roll(idx, -1, axis=0)
    c, d = np.roll(idx, -1, axis=1), np.roll(np.roll(idx, -1, axis=0), -1, axis=1)
    return v.astype(np.float32), np.concatenate([np.stack([a, b, d], -1), np.stack([a, d, c], -1)]).reshape(-1, 3).astype(np.int32)


def end_to_end_inputs(mesh):
    """What the end-to-end case renders (numpy only; the GPU test and tools/pnp_bench.py --end-to-end both start here): a torus or a
    rippled sphere, crop-like LineMOD intrinsics for 64 x 80, two poses about 900 mm away."""
    H, W, B = 64, 80, 2
    verts, faces = _uv_sphere(24, 32, 50.0, ripple=0.1) if mesh == "sphere" else _torus(40, 20)
    rs = np.random.RandomState(len(mesh))
    K = np.array(LINEMOD_K, dtype=np.float64)
    K[:2] *= H / 128.0
    K[0, 2], K[1, 2] = W / 2.0, H / 2.0
    P = []
    for _ in range(B):
        q, _r = np.linalg.qr(rs.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        P.append(np.concatenate([q, rs.uniform(-15, 15, (3, 1)) + [[0.0], [0.0], [900.0]]], 1))
    return dict(verts=verts, faces=faces, K=K.astype(np.float32), P=np.stack(P).astype(np.float32), H=H, W=W)


def end_to_end_corruption(kept):
    """(touched [B,H,W] bool, values [n,3]): 30 % of the kept pixels and the uniform NOCS values that replace theirs."""
    rs = np.random.RandomState(11)
    touched = kept & (rs.uniform(size=kept.shape) < 0.3)
    return touched, rs.uniform(0, 1, (int(touched.sum()), 3))
