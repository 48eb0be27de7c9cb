"""fp64 numpy restatement of the hard mesh rasteriser (tp_mesh_raster) and of the reference's surfel
arithmetic (compute_surfelinfo.normal_from_depth, SoftPhongNOCSShader's normalisation, MVRenderer.calibrate_pose's 6D round
trip).  Brute force: every face is tested at every requested pixel centre."""
import numpy as np


def project(verts, faces, pose, K):
    """-> u, v, z [F,3] (screen position, view-space z of each face vertex), twice the signed area [F] and valid [F] (no vertex
    at z <= 0, not degenerate)."""
    verts, pose, K = (np.asarray(x, dtype=np.float64) for x in (verts, pose, K))
    xc = verts @ pose[:, :3].T + pose[:, 3]
    q = xc @ K.T
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    U, Vv, Z = u[faces], v[faces], xc[:, 2][faces]
    area = (U[:, 1] - U[:, 0]) * (Vv[:, 2] - Vv[:, 0]) - (Vv[:, 1] - Vv[:, 0]) * (U[:, 2] - U[:, 0])
    valid = (Z > 0).all(1) & np.isfinite(area) & (np.abs(area) > 1e-10)
    return U, Vv, Z, area, valid


def _bary(U, Vv, area, px, py):
    """b [..., 3] with b_k from the edge opposite vertex k (U, Vv, area broadcast against px, py)."""
    b = []
    for k in range(3):
        s, e = (k + 1) % 3, (k + 2) % 3
        ex, ey = U[..., e] - U[..., s], Vv[..., e] - Vv[..., s]
        b.append((ex * (py - Vv[..., s]) - ey * (px - U[..., s])) / area)
    return np.stack(b, axis=-1)


def nocs_normalisation(verts):
    """mvrenderer.py:702-708 in fp64: per-axis mean and max |v - mean|."""
    v = np.asarray(verts, dtype=np.float64)
    ct = v.mean(0)
    return ct, np.abs(v - ct).max(0)


def nocs_vertices(verts, ct, sc):
    """mvrenderer.py:710-716: ((v - ct) / sc + 1) / 2 per vertex."""
    return ((np.asarray(verts, dtype=np.float64) - np.asarray(ct, dtype=np.float64)) / np.asarray(sc, dtype=np.float64) + 1.0) / 2.0


def rasterize(verts, faces, pose, K, H, W, pixels=None, vcolor=None, nocs_norm=None, chunk=None):
    """Brute-force hard raster at the pixel indices ``pixels`` (flat row-major, default all): face [P] (-1 background), zbuf [P]
    (-1 background), min_bary [P] (of the winning face), rgb / nocs [P,3] (0 on background) when vcolor / nocs_norm are given."""
    pixels = np.arange(H * W) if pixels is None else np.asarray(pixels)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    U, Vv, Z, area, valid = project(verts, faces, pose, K)
    fid = np.nonzero(valid)[0]
    U, Vv, Z, area = U[fid], Vv[fid], Z[fid], area[fid]
    P = len(pixels)
    chunk = chunk or max(1, min(256, 2000000 // max(1, len(fid))))      # ~50 MB per [p, F, 3] array
    face, zbuf, minb, bw = np.full(P, -1), np.full(P, -1.0), np.zeros(P), np.zeros((P, 3))
    for s in range(0, P if len(fid) else 0, chunk):
        pix = pixels[s:s + chunk]
        px, py = ((pix % W) + 0.5)[:, None], ((pix // W) + 0.5)[:, None]
        b = _bary(U[None], Vv[None], area[None], px, py)          # [p, F, 3]
        cov = (b > 0).all(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(cov, 1.0 / (b / Z[None]).sum(-1), np.inf)
        z = np.where(z > 1e-8, z, np.inf)
        zmin = z.min(1)
        rows = np.nonzero(np.isfinite(zmin))[0]
        win = np.argmax(z == zmin[:, None], axis=1)[rows]         # first = smallest face index among equal depths
        face[s + rows] = fid[win]
        zbuf[s + rows] = zmin[rows]
        bb = b[rows, win]
        minb[s + rows] = bb.min(-1)
        w = bb / Z[win]
        bw[s + rows] = w / w.sum(-1, keepdims=True)
    out = dict(face=face, zbuf=zbuf, min_bary=minb)
    hit = face >= 0
    fv = faces[np.maximum(face, 0)]

    def interp(attr):
        a = np.asarray(attr, dtype=np.float64)[fv]                 # [P, 3 vertices, 3]
        return np.where(hit[:, None], (bw[:, :, None] * a).sum(1), 0.0)

    if vcolor is not None:
        out["rgb"] = interp(vcolor)
    if nocs_norm is not None:
        out["nocs"] = interp(nocs_vertices(verts, *nocs_norm))
    return out


def face_bary_at(verts, faces, pose, K, W, face_idx, pixels):
    """fp64 barycentrics [P,3] of face ``face_idx[p]`` at pixel ``pixels[p]`` (flat row-major)."""
    U, Vv, Z, area, _ = project(verts, np.asarray(faces).reshape(-1, 3)[np.asarray(face_idx)], pose, K)
    pixels = np.asarray(pixels)
    return _bary(U, Vv, area, (pixels % W) + 0.5, (pixels // W) + 0.5)


def calibrate_pose(pose, depth_scale):
    """compute_surfelinfo.py:107 + pytorch3d's matrix_to_rotation_6d / rotation_6d_to_matrix on R^T (rows of R^T = columns of R),
    fp64: Gram-Schmidt of R's first two columns, third column their cross product; t * 1000 / depth_scale."""
    pose = np.asarray(pose, dtype=np.float64)
    out = np.empty_like(pose)
    for b in range(pose.shape[0]):
        a1, a2 = pose[b, :, 0], pose[b, :, 1]
        b1 = a1 / max(np.linalg.norm(a1), 1e-12)
        b2 = a2 - (b1 @ a2) * b1
        b2 = b2 / max(np.linalg.norm(b2), 1e-12)
        out[b, :, :3] = np.stack([b1, b2, np.cross(b1, b2)], axis=1)
        out[b, :, 3] = pose[b, :, 3] * 1000.0 / depth_scale
    return out


def normal_from_depth(depth, pose, K):
    """compute_surfelinfo.normal_from_depth for one image, fp64: depth [H,W] (mm, <= 0 background), pose [3,4], K [3,3] ->
    normal [H,W,3].  Rays as compute_box.get_center_and_ray: centre = -R^T t, ray = R^T K^-1 (j + .5, i + .5, 1); neighbours are
    not masked; tu = p[i, j+1] - p[i, j-1], tv = p[i+1, j] - p[i-1, j]; normalize(tu x tv, eps 1e-12); third component negated;
    border and depth <= 0 zero."""
    depth = np.asarray(depth, dtype=np.float64)
    H, W = depth.shape
    pose, K = np.asarray(pose, dtype=np.float64), np.asarray(K, dtype=np.float64)
    R, t = pose[:, :3], pose[:, 3]
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    g = np.stack([jj, ii, np.ones_like(jj)], -1) @ np.linalg.inv(K).T
    p = -R.T @ t + (g @ R) * depth[..., None]                      # centre + (R^T g) * depth
    tu = p[1:-1, 2:] - p[1:-1, :-2]
    tv = p[2:, 1:-1] - p[:-2, 1:-1]
    n = np.cross(tu, tv)
    n = n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-12)
    out = np.zeros((H, W, 3))
    out[1:-1, 1:-1] = n
    out[..., 2] *= -1
    return out * (depth > 0)[..., None]
