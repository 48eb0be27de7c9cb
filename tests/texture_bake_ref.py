"""fp64 numpy restatement of K27 tp_texture_bake, written from the contract in include/texpose_amd.h (not from the kernel), and
exact ray casting (Moeller-Trumbore) for the visibility the contract approximates with a depth plane and a normal-derived bias."""
import numpy as np

DEFAULTS = dict(cos_min=0.3, cover_min=0.5, z_tol_mm=0.5, slope=2.0)


def bake(verts, normals, pose, intr, rgb, zbuf, weight=None, cos_min=0.3, cover_min=0.5, z_tol_mm=0.5, slope=2.0):
    """-> dict(acc [V,4] fp64, count [V], used [V,B] bool (the pair contributed), margin [V,B]: the smallest relative distance of the
    pair to any decision it went through -- |z| / |x| for z > 0, |c - cos_min| / cos_min, per in-image tap with a positive depth
    ||dz| - tol| / tol, |cover - cover_min| / cover_min; inf where a decision does not depend on arithmetic --, reached [V,B] bool
    (the pair got as far as its taps) and colour [V,B,3] of the pairs used).  The scalars are taken as fp32, like the kernel's."""
    f = lambda x: np.asarray(x, dtype=np.float64)
    cos_min, cover_min, z_tol_mm, slope = (float(np.float32(x)) for x in (cos_min, cover_min, z_tol_mm, slope))
    verts, normals, pose, intr, rgb, zbuf = f(verts), f(normals), f(pose), f(intr), f(rgb), f(zbuf)
    weight = None if weight is None else f(weight)
    V, B = verts.shape[0], pose.shape[0]
    if intr.ndim == 2:
        intr = np.broadcast_to(intr, (B, 3, 3))
    H, W = zbuf.shape[1:]
    acc, count = np.zeros((V, 4)), np.zeros(V, dtype=np.int64)
    used, reached = np.zeros((V, B), dtype=bool), np.zeros((V, B), dtype=bool)
    margin = np.full((V, B), np.inf)
    colour = np.zeros((V, B, 3))
    for b in range(B):
        R, t, K = pose[b, :, :3], pose[b, :, 3], intr[b]
        for i in range(V):
            x = R @ verts[i] + t
            z = x[2]
            dist = np.sqrt(x @ x)
            m = abs(z) / dist if dist > 0 else 0.0
            if not z > 0:
                margin[i, b] = m
                continue
            c = -((R @ normals[i]) @ x) / dist
            m = min(m, abs(c - cos_min) / cos_min)
            if not c >= cos_min:
                margin[i, b] = m
                continue
            q = K @ x
            su, sv = q[0] / q[2] - 0.5, q[1] / q[2] - 0.5
            if not (-1 <= su < W and -1 <= sv < H):
                margin[i, b] = m
                continue
            reached[i, b] = True
            j0, r0 = int(np.floor(su)), int(np.floor(sv))
            a, be = su - j0, sv - r0
            tol = z_tol_mm + slope * (z / min(K[0, 0], K[1, 1])) * np.sqrt(max(0.0, 1 - c * c)) / c
            cover, cw, col = 0.0, 0.0, np.zeros(3)
            for dr in (0, 1):
                for dj in (0, 1):
                    r, j = r0 + dr, j0 + dj
                    if not (0 <= r < H and 0 <= j < W):
                        continue
                    zt = zbuf[b, r, j]
                    if not zt > 0:
                        continue
                    w = (a if dj else 1 - a) * (be if dr else 1 - be)
                    if np.isfinite(zt) and w > 0:
                        m = min(m, abs(abs(zt - z) - tol) / tol)
                    if not abs(zt - z) <= tol:
                        continue
                    if not np.isfinite(rgb[b, r, j]).all() or (weight is not None and not np.isfinite(weight[b, r, j])):
                        continue
                    cover += w
                    col += w * rgb[b, r, j]
                    if weight is not None:
                        cw += w * weight[b, r, j]
            m = min(m, abs(cover - cover_min) / cover_min)
            margin[i, b] = m
            if not cover >= cover_min:
                continue
            wb = c * cover
            if weight is not None:
                wb *= cw / cover
            col = col / cover
            acc[i, :3] += wb * col
            acc[i, 3] += wb
            count[i] += 1
            used[i, b] = True
            colour[i, b] = col
    return dict(acc=acc, count=count, used=used, margin=margin, reached=reached, colour=colour)


def vcolor_of(acc):
    """acc [V,4] -> (vcolor [V,3], seen [V])."""
    seen = acc[:, 3] > 0
    return np.where(seen[:, None], acc[:, :3] / np.where(seen, acc[:, 3], 1.0)[:, None], 0.0), seen


def ray_hits(origin, targets, verts, faces, skip):
    """Moeller-Trumbore: for each target point k, the smallest parameter s in (1e-9, inf) at which the ray origin + s (target_k -
    origin) meets a face not listed for it in ``skip`` [K,F] bool; inf without a hit.  s < 1: the hit lies before the target."""
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    v0, e1, e2 = verts[faces[:, 0]], verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]]
    d = np.asarray(targets, dtype=np.float64) - origin                                   # [K,3]
    p = np.cross(d[:, None, :], e2[None])                                                # [K,F,3]
    det = (p * e1[None]).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tv = origin - v0                                                                 # [F,3]
        u = (p * tv[None]).sum(-1) * inv
        qv = np.cross(tv, e1)                                                            # [F,3]
        w = (d[:, None, :] * qv[None]).sum(-1) * inv
        s = (qv * e2).sum(-1)[None] * inv
    hit = (np.abs(det) > 1e-12) & (u >= 0) & (w >= 0) & (u + w <= 1) & (s > 1e-9) & ~skip
    return np.where(hit, s, np.inf).min(1)


def incident(faces, V):
    """[V,F] bool: face f has vertex i."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    m = np.zeros((V, len(faces)), dtype=bool)
    for k in range(3):
        m[faces[:, k], np.arange(len(faces))] = True
    return m


# ---- the test meshes (those of the rasteriser's tests) and views
def uv_sphere(n_lat, n_lon, radius=50.0, ripple=0.0):
    th = np.linspace(0, np.pi, n_lat + 1)
    ph = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    T, P = np.meshgrid(th, ph, indexing="ij")
    r = radius * (1 + ripple * np.sin(5 * T) * np.cos(3 * P))
    v = np.stack([r * np.sin(T) * np.cos(P), r * np.sin(T) * np.sin(P), r * np.cos(T)], -1).reshape(-1, 3)
    idx = np.arange((n_lat + 1) * n_lon).reshape(n_lat + 1, n_lon)
    a, b, c, d = idx[:-1], np.roll(idx[:-1], -1, axis=1), idx[1:], np.roll(idx[1:], -1, axis=1)
    f = np.concatenate([np.stack([a, c, d], -1)[:-1], np.stack([a, d, b], -1)[1:]]).reshape(-1, 3)
    return v.astype(np.float32), f.astype(np.int32)


def torus(n_major, n_minor, R=45.0, r=16.0):
    u = np.linspace(0, 2 * np.pi, n_major, endpoint=False)
    w = np.linspace(0, 2 * np.pi, n_minor, endpoint=False)
    U, Wm = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(Wm)) * np.cos(U), (R + r * np.cos(Wm)) * np.sin(U), r * np.sin(Wm)], -1).reshape(-1, 3)
    idx = np.arange(n_major * n_minor).reshape(n_major, n_minor)
    a, b = idx, np.roll(idx, -1, axis=0)
    c, d = np.roll(idx, -1, axis=1), np.roll(np.roll(idx, -1, axis=0), -1, axis=1)
    f = np.concatenate([np.stack([a, b, d], -1), np.stack([a, d, c], -1)]).reshape(-1, 3)
    return v.astype(np.float32), f.astype(np.int32)


def pinhole(H, W, f):
    return np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]], dtype=np.float32)


def test_colours(verts):
    """0.5 + 0.5 sin(v / 25 + (0, 1, 2)) per vertex."""
    return (0.5 + 0.5 * np.sin(np.asarray(verts, dtype=np.float64) / 25.0 + np.array([0.0, 1.0, 2.0]))).astype(np.float32)


test_colours.__test__ = False


def smooth_image(B, H, W):
    """An analytic smooth function of the pixel position in [0, 1]: [B,H,W,3] float32."""
    r, j = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    b = np.arange(B)[:, None, None]
    ch = [0.5 + 0.5 * np.sin(0.31 * j[None] + 0.17 * r[None] + 0.9 * b), 0.5 + 0.5 * np.cos(0.23 * r[None] - 0.11 * j[None] + 0.4 * b),
          0.5 + 0.5 * np.sin(0.05 * (j[None] * r[None]) ** 0.5 + b)]
    return np.stack(ch, -1).astype(np.float32)
