"""fp64 numpy restatement of K35 (tp_face_texel_shade) and of face_texels.subdivide, written from the contract in
include/texpose_amd.h and the docstring (not from the kernel or the module): plain loops where the module is vectorised."""
import numpy as np


def texel_count(R):
    return (R + 1) * (R + 2) // 2


def node(i, j, R):
    return j * (R + 1) - j * (j - 1) // 2 + i


def node_list(R):
    """[(i, j)] in storage order."""
    out = [None] * texel_count(R)
    for j in range(R + 1):
        for i in range(R + 1 - j):
            out[node(i, j, R)] = (i, j)
    return out


def shade(face, verts, faces, texels, pose, intr, H, W):
    """face [B,H,W] int, pose [B,3,4], intr [B,3,3] or [3,3], texels [F,T,3] -> rgb [B,H,W,3] float64 BEFORE the rounding to fp32
    (the caller compares against .astype(float32))."""
    face = np.asarray(face).reshape(-1, H, W)
    B = face.shape[0]
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    texels = np.asarray(texels, dtype=np.float64)
    pose = np.asarray(pose, dtype=np.float64).reshape(B, 3, 4)
    intr = np.broadcast_to(np.asarray(intr, dtype=np.float64), (B, 3, 3))
    V, F, T = len(verts), len(faces), texels.shape[1]
    R = (int(np.sqrt(8 * T + 1)) - 3) // 2
    assert texel_count(R) == T
    out = np.zeros((B, H, W, 3))
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        for b in range(B):
            fb_ = face[b].astype(np.int64)
            ok = (fb_ >= 0) & (fb_ < F)
            f = np.where(ok, fb_, 0)
            vi = faces[f]                                                   # [H,W,3]
            ok &= ((vi >= 0) & (vi < V)).all(-1)
            vi = np.clip(vi, 0, V - 1)
            P, K = pose[b], intr[b]
            X = verts[vi]                                                   # [H,W,3 vertices,3]
            c = [P[r, 0] * X[..., 0] + P[r, 1] * X[..., 1] + P[r, 2] * X[..., 2] + P[r, 3] for r in range(3)]
            ok &= ((c[2] > 0) & np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2])).all(-1)
            q = [K[r, 0] * c[0] + K[r, 1] * c[1] + K[r, 2] * c[2] for r in range(3)]
            u, v, iz = q[0] / q[2], q[1] / q[2], 1.0 / c[2]
            area = (u[..., 1] - u[..., 0]) * (v[..., 2] - v[..., 0]) - (v[..., 1] - v[..., 0]) * (u[..., 2] - u[..., 0])
            ok &= np.isfinite(area) & (np.abs(area) > 1e-10)
            px, py = jj + 0.5, ii + 0.5
            t = []
            for k in range(3):
                s, e = (k + 1) % 3, (k + 2) % 3
                ex, ey = u[..., e] - u[..., s], v[..., e] - v[..., s]
                t.append(((ex * (py - v[..., s]) - ey * (px - u[..., s])) / area) * iz[..., k])
            tot = (t[0] + t[1]) + t[2]
            w = [tk / tot for tk in t]
            w = [np.where(wk < 0, 0.0, wk) for wk in w]
            s2 = (w[0] + w[1]) + w[2]
            w = [wk / s2 for wk in w]
            ok &= np.isfinite(w[0]) & np.isfinite(w[1]) & np.isfinite(w[2])
            w = [np.where(ok, wk, 0.0) for wk in w]
            a, bb = R * w[1], R * w[2]
            ci = np.minimum(np.floor(a).astype(np.int64), R - 1)
            cj = np.minimum(np.floor(bb).astype(np.int64), R - 1 - ci)
            fa, fb = a - ci, bb - cj
            upper = (fa + fb > 1.0) & (ci + cj <= R - 2)
            N = lambda i, j: texels[f, np.clip(node(i, j, R), 0, T - 1)]    # (the clip only matters where the branch is not taken)
            lo = ((1.0 - fa) - fb)[..., None] * N(ci, cj) + fa[..., None] * N(ci + 1, cj) + fb[..., None] * N(ci, cj + 1)
            up = ((fa + fb) - 1.0)[..., None] * N(ci + 1, cj + 1) + (1.0 - fb)[..., None] * N(ci + 1, cj) + (1.0 - fa)[..., None] * N(ci, cj + 1)
            col = np.where(upper[..., None], up, lo)
            ok &= np.isfinite(col).all(-1)
            out[b] = np.where(ok[..., None], col, 0.0)
    return out


def mesh_edges(faces):
    """sorted unique undirected edges [E,2]"""
    s = set()
    for f in np.asarray(faces, dtype=np.int64).reshape(-1, 3):
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            if a != b:
                s.add((min(a, b), max(a, b)))
    return np.array(sorted(s), dtype=np.int64).reshape(-1, 2)


def subdivide(verts, faces, R):
    """-> verts_sub [U,3] float32, faces_sub [F R^2,3], node_index [F,T] by the canonical rule of face_texels.subdivide."""
    v32 = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    v = v32.astype(np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, F = len(v), len(faces)
    edges = mesh_edges(faces)
    eid = {tuple(e): n for n, e in enumerate(edges)}
    E = len(edges)
    nodes = node_list(R)
    n_inner = (R - 1) * (R - 2) // 2
    pos = [row for row in v32]
    for p, q in edges:
        for k in range(1, R):
            pos.append((((R - k) * v[p] + k * v[q]) / R).astype(np.float32))
    node_index = np.zeros((F, len(nodes)), dtype=np.int64)

    def on_edge(a, b, k):                       # k steps from vertex a towards vertex b
        if a == b:
            return a
        if a > b:
            a, b, k = b, a, R - k
        return V + eid[(a, b)] * (R - 1) + k - 1

    for fi, (v0, v1, v2) in enumerate(faces):
        inner = 0
        for n, (i, j) in enumerate(nodes):
            if (i, j) == (0, 0):
                node_index[fi, n] = v0
            elif (i, j) == (R, 0):
                node_index[fi, n] = v1
            elif (i, j) == (0, R):
                node_index[fi, n] = v2
            elif j == 0:
                node_index[fi, n] = on_edge(v0, v1, i)
            elif i == 0:
                node_index[fi, n] = on_edge(v0, v2, j)
            elif i + j == R:
                node_index[fi, n] = on_edge(v1, v2, j)
            else:
                node_index[fi, n] = V + E * (R - 1) + fi * n_inner + inner
                inner += 1
                pos.append(((((R - i - j) * v[v0] + i * v[v1]) + j * v[v2]) / R).astype(np.float32))
    faces_sub = []
    for fi in range(F):
        for j in range(R):
            for i in range(R - j):
                faces_sub.append([node_index[fi, node(i, j, R)], node_index[fi, node(i + 1, j, R)], node_index[fi, node(i, j + 1, R)]])
                if i + j <= R - 2:
                    faces_sub.append([node_index[fi, node(i + 1, j, R)], node_index[fi, node(i + 1, j + 1, R)], node_index[fi, node(i, j + 1, R)]])
    return np.array(pos, dtype=np.float32).reshape(-1, 3), np.array(faces_sub, dtype=np.int64).reshape(-1, 3), node_index


def fine_colour(points, period_mm=3.0):
    """0.5 + 0.5 sin(x / period + (0, 1, 2)): detail far below the test meshes' vertex spacing."""
    return 0.5 + 0.5 * np.sin(np.asarray(points, dtype=np.float64) / period_mm + np.array([0.0, 1.0, 2.0]))


# ---- the refinement case: photo_align / joint_align with texels on a photograph rendered from the same texels
# pnp_ref.end_to_end_inputs("sphere") (the rippled sphere, two poses about 900 mm away, 64 x 80: a pixel is about 3 mm on the object and
# a face 2 .. 3 pixels), R = 2 (a texel about a pixel), the texels photo_ref.vertex_colours' function (period 8 mm) evaluated at the
# nodes, the photograph the restatement's render of the true poses over photo_ref.BACKGROUND, the start icp_ref.perturbed(P,
# RandomState(5), 3.0): 3 degrees and 6.1 / 8.1 mm away.  Chosen on the CPU: photo_ref's loop (10 steps, tau 0.5, damping 1e-6) with the
# restated shading converges from there to the errors below; with a 4 mm period the second pose stops 0.16 degrees / 0.44 mm away from
# the same start (and from 1 degree too), so the finer texture's basin is narrower than this offset.
LOOP_R, LOOP_ANGLE_DEG = 2, 3.0
LOOP_FINAL = ((7.9e-4, 9.1e-4), (3.8e-4, 3.2e-4))          # (degrees, mm) of the CPU loop's final poses, measured


def loop_inputs():
    import photo_ref as PH
    import pnp_ref as PREF
    from texpose_amd import face_texels as FT
    e = PREF.end_to_end_inputs("sphere")
    K = np.tile(e["K"], (2, 1, 1))
    verts_sub, _, node_index = FT.subdivide(e["verts"], e["faces"], LOOP_R)
    texels = FT.texels_from_nodes(PH.vertex_colours(verts_sub), node_index)
    image = np.stack([loop_render(e, texels, e["P"][b], K[b], PH.BACKGROUND)[1] for b in range(2)])
    return dict(e, K=K, texels=texels, image=image, start=PH.perturbed(e["P"], np.random.RandomState(5), LOOP_ANGLE_DEG))


def loop_render(c, texels, pose, K, background=None):
    """zbuf [H,W] and rgb [H,W,3] float32 of one pose: the brute-force raster's face plane, shaded by the restatement"""
    import mesh_raster_ref as RAST
    H, W = c["H"], c["W"]
    r = RAST.rasterize(c["verts"], c["faces"], pose, K, H, W)
    face = r["face"].reshape(1, H, W)
    rgb = shade(face, c["verts"], c["faces"], texels, np.asarray(pose)[None], K, H, W)[0]
    if background is not None:
        rgb = np.where((face[0] >= 0)[..., None], rgb, background)
    return r["zbuf"].reshape(H, W).astype(np.float32), rgb.astype(np.float32)


def loop_ref(c):
    """photo_ref's loop with the restated shading as its renderer -> its result dict"""
    import photo_ref as PH
    render = lambda P: [loop_render(c, c["texels"], np.asarray(P[b], np.float32), c["K"][b]) for b in range(len(P))]
    step = lambda planes, P, t, last: PH.step_ref(np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes]), P, c["K"], c["image"], t, 1e-6,
                                                  None, None, evaluate_only=last)
    return PH.loop_ref(render, step, c["start"], 0.5, 10)
