"""The depth-ICP contract of DESIGN section 19 (kernel K29: tp_depth_icp_step), said again in numpy fp64 -- written from the rules in
include/texpose_amd.h, not from the kernels.  Where the kernel is free to choose, this file chooses differently: the sums are matrix
products over the kept pixels of an image at once (the kernel adds per thread, wave, workgroup and tile), the systems are solved with
np.linalg.solve on the Cholesky factors, and the loop renders with the brute-force rasteriser of tests/mesh_raster_ref.py.

Besides the results it reports what decides whether a comparison of counts can be exact: near-ties, kept-or-dropped decisions whose
margin | |d - z| |ray| - tau | is below NEAR_TIE mm."""
import numpy as np

import mesh_raster_ref as RR
from gn_ref import MIN_COUNT, PIVOT_TOL, _exp_so3, loop_ref, solve_ref  # noqa: F401  (tests reach them through this module)

NEAR_TIE = 1e-6          # mm


def frame_index(B, Ft, frame):
    if frame is None:
        assert Ft in (1, B)
        return np.zeros(B, np.int64) if Ft == 1 else np.arange(B)
    return np.clip(np.asarray(frame, np.int64), 0, Ft - 1)


def sums_ref(verts, faces, zbuf, face, pose, K, depth, tau, mask=None):
    """One image: zbuf / face / depth / mask [H,W], pose [3,4], K [3,3] (fp32 values) -> dict(JtJ [6,6], Jtr [6], cost, count,
    near_ties, kept [H,W] bool)."""
    verts, faces = np.asarray(verts, np.float32).astype(np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(verts), len(faces)
    z32, d32, face = np.asarray(zbuf, np.float32), np.asarray(depth, np.float32), np.asarray(face, np.int64)
    H, W = z32.shape
    pose, K = np.asarray(pose, np.float32).astype(np.float64), np.asarray(K, np.float32).astype(np.float64)
    tau = float(np.float32(tau))
    with np.errstate(all="ignore"):
        cand = (z32 > 0) & np.isfinite(z32) & (d32 > 0) & np.isfinite(d32) & (face >= 0) & (face < F)
        if mask is not None:
            cand &= np.asarray(mask) != 0
        ii, ji = np.nonzero(cand)
        tri = faces[face[ii, ji]]
        good = ((tri >= 0) & (tri < V)).all(-1)
        ii, ji, tri = ii[good], ji[good], tri[good]
        z, d = z32[ii, ji].astype(np.float64), d32[ii, ji].astype(np.float64)
        ray = np.stack([((ji + 0.5) - K[0, 2]) / K[0, 0], ((ii + 0.5) - K[1, 2]) / K[1, 1], np.ones(len(ii))], 1)
        q = (ray[:, 0] ** 2 + ray[:, 1] ** 2) + 1.0
        dz = d - z
        m = np.cross(verts[tri[:, 1]] - verts[tri[:, 0]], verts[tri[:, 2]] - verts[tri[:, 0]]) @ pose[:, :3].T
        mm = (m * m).sum(-1)
        near = (dz * dz) * q <= tau * tau
        solid = np.isfinite(mm) & (mm > 0)
        ties = int((solid & (np.abs(np.abs(dz) * np.sqrt(q) - tau) < NEAR_TIE)).sum())
        keep = near & solid
    ii, ji, z, d, ray, m, mm = ii[keep], ji[keep], z[keep], d[keep], ray[keep], m[keep], mm[keep]
    n = m / np.sqrt(mm)[:, None]
    n[(n * ray).sum(-1) > 0] *= -1.0
    P, Q = ray * z[:, None], ray * d[:, None]
    r = (n * (P - Q)).sum(-1)
    J = np.concatenate([np.cross(P, n), n], 1)
    kept = np.zeros((H, W), bool)
    kept[ii, ji] = True
    return dict(JtJ=J.T @ J, Jtr=J.T @ r, cost=float(r @ r), count=len(r), near_ties=ties, kept=kept)


def step_ref(verts, faces, zbuf, face, pose, K, depth, tau, damping=1e-6, frame=None, mask=None, evaluate_only=False):
    """The whole call: zbuf / face [B,H,W], pose [B,3,4], K [B,3,3], depth (and mask) [Ft,H,W] -> dict(pose [B,3,4] float32, inliers
    [B], rms [B] fp64, status [B], near_ties [B], kept [B,H,W])."""
    B = len(pose)
    depth = np.asarray(depth, np.float32)
    fr = frame_index(B, len(depth), frame)
    out = dict(pose=np.zeros((B, 3, 4), np.float32), inliers=np.zeros(B, np.int64), rms=np.zeros(B), status=np.zeros(B, np.int64),
               near_ties=np.zeros(B, np.int64), kept=np.zeros(np.asarray(zbuf).shape, bool))
    for b in range(B):
        s = sums_ref(verts, faces, zbuf[b], face[b], pose[b], K[b], depth[fr[b]], tau, None if mask is None else np.asarray(mask)[fr[b]])
        out["pose"][b], out["inliers"][b], out["rms"][b], out["status"][b] = solve_ref(s, pose[b], damping, evaluate_only)
        out["near_ties"][b], out["kept"][b] = s["near_ties"], s["kept"]
    return out


def render_ref(verts, faces, pose, K, H, W):
    """zbuf [H,W] float32 (-1 background) and face [H,W] int32 of one pose by the brute-force rasteriser."""
    r = RR.rasterize(verts, faces, np.asarray(pose, np.float64), np.asarray(K, np.float64), H, W)
    return r["zbuf"].reshape(H, W).astype(np.float32), r["face"].reshape(H, W).astype(np.int32)


def icp_ref(verts, faces, pose, K, depth, tau=20.0, iters=5, damping=1e-6, frame=None, mask=None):
    """The loop of ops.depth_icp with its own raster: iters + 1 passes, the pose rounded to fp32 between them, the last evaluate-only
    -> dict(pose [B,3,4] float32, inliers, rms, status (of the last step taken), inliers0, rms0, near_ties (largest over the passes))."""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape[1:]
    render = lambda P: [render_ref(verts, faces, P[b], K[b], H, W) for b in range(len(P))]
    step = lambda planes, P, t, last: step_ref(verts, faces, np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes]), P, K, depth, t,
                                               damping, frame, mask, evaluate_only=last)
    return loop_ref(render, step, pose, tau, iters)


# ----------------------------------------------------------------------------------------------------------------- the loop's case
def perturbed(P, rs, angle_deg=3.0):
    """P [B,3,4] moved by angle_deg about a random axis and 4 to 11 mm: a random direction scaled to a length in that range."""
    out = np.asarray(P, np.float64).copy()
    for b in range(len(out)):
        w = rs.normal(size=3)
        w *= np.radians(angle_deg) / np.linalg.norm(w)
        t = rs.normal(size=3)
        t *= rs.uniform(4.0, 11.0) / np.linalg.norm(t)
        out[b, :, :3] = _exp_so3(w) @ out[b, :, :3]
        out[b, :, 3] += t
    return out.astype(np.float32)


def corrupted(depth, rs, W):
    """The loop's noisy case: 1 mm Gaussian noise, 5 % holes, an occluder at 700 mm over the columns left of W / 2 - 6."""
    d = np.asarray(depth, np.float32).copy()
    hit = d > 0
    d[hit] += rs.normal(0.0, 1.0, int(hit.sum())).astype(np.float32)
    d[rs.uniform(size=d.shape) < 0.05] = 0.0
    d[..., :W // 2 - 6] = 700.0
    return d


# ----------------------------------------------------------------------------------------------------------------- one step, exact inputs
def one_step_case(seed, B, H, W, frames="one", with_mask=False):
    """Hand-built planes for one step (no rasteriser): a small torus, per image a pose about 900 mm away, zbuf 880 .. 920 mm on 60 % of
    the pixels, random face indices, depth = zbuf + U(-30, 30) (tau = 20 keeps about two thirds), and the bad values the contract
    names: NaN / Inf / zero / negative depth, face -1 / F / 2^30, a face with a vertex index >= V, a zero-area face, NaN zbuf.
    ``frames``: 'one' (Ft = 1), 'each' (Ft = B) or 'map' (Ft = 2 and a repeating frame map)."""
    from pnp_ref import _torus
    rs = np.random.RandomState(seed)
    verts, faces = _torus(8, 6)
    V = len(verts)
    faces = np.concatenate([faces, [[0, 1, V + 5], [3, 3, 7], [2, -1, 4]]]).astype(np.int32)          # out of range, zero area, negative
    F = len(faces)
    f = min(H, W) * 9.0 + 300.0
    K = np.tile(np.array([[f, 0.0, W / 2.0 + 0.25], [0.0, f * 1.01, H / 2.0 - 0.25], [0.0, 0.0, 1.0]], np.float32), (B, 1, 1))
    pose = np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        pose[b] = np.concatenate([q, rs.uniform(-15, 15, (3, 1)) + [[0.0], [0.0], [900.0]]], 1)
    Ft = dict(one=1, each=B, map=2)[frames]
    frame = (np.arange(B) % 2).astype(np.int32)[::-1].copy() if frames == "map" else None
    fr = frame_index(B, Ft, frame)
    n = H * W
    zbuf = rs.uniform(880.0, 920.0, (B, H, W)).astype(np.float32)
    zbuf[rs.uniform(size=zbuf.shape) < 0.4] = -1.0
    face = rs.randint(0, F, (B, H, W)).astype(np.int32)
    base = rs.uniform(880.0, 920.0, (Ft, H, W)).astype(np.float32)
    depth = base.copy()
    for b in range(B):                                           # (with a shared plane the later images overwrite: still a valid case)
        hit = zbuf[b] > 0
        depth[fr[b]][hit] = zbuf[b][hit] + rs.uniform(-30.0, 30.0, int(hit.sum())).astype(np.float32)
    flat_d, flat_z, flat_f = depth.reshape(Ft, n), zbuf.reshape(B, n), face.reshape(B, n)
    flat_d[rs.uniform(size=flat_d.shape) < 0.02] = np.nan
    for k, value in enumerate((np.inf, 0.0, -5.0, -np.inf)):
        flat_d[rs.randint(Ft), rs.randint(n)] = value
    for value in (-1, F, 2 ** 30, -2 ** 31):
        flat_f[rs.randint(B), rs.randint(n)] = value
    flat_z[rs.randint(B), rs.randint(n)] = np.nan
    flat_z[rs.randint(B), rs.randint(n)] = np.inf
    mask = (rs.uniform(size=(Ft, H, W)) < 0.8).astype(np.uint8) if with_mask else None
    return dict(verts=verts, faces=faces, zbuf=zbuf, face=face, pose=pose, K=K, depth=depth, frame=frame, mask=mask, tau=20.0)
