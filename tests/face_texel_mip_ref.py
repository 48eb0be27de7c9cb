"""fp64 numpy restatement of K43 (tp_face_texel_mip_reduce, tp_face_texel_shade_mip), written from the contract in
include/texpose_amd.h (not from the kernels): plain loops for the reduce, vectorised per image for the shade.  The operations are in
the order the header writes them, so that a kernel built without contraction gives the same bits."""
import numpy as np

from face_texels_ref import node, node_list, texel_count

DIRS = ((1, 0), (0, 1), (-1, 1), (-1, 0), (0, -1), (1, -1))


# ---- the test meshes
def tetrahedron():
    v = 40.0 * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float32)
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)


def octahedron():
    v = 50.0 * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
    f = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]
    return v, np.array(f, dtype=np.int32)


def icosphere():
    """the 20-face icosphere (an icosahedron), radius 50"""
    p = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([[-1, p, 0], [1, p, 0], [-1, -p, 0], [1, -p, 0], [0, -1, p], [0, 1, p], [0, -1, -p], [0, 1, -p], [p, 0, -1], [p, 0, 1],
                  [-p, 0, -1], [-p, 0, 1]])
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    return (50.0 * v / np.linalg.norm(v[0])).astype(np.float32), np.array(f, dtype=np.int32)


def triangle():
    return np.array([[-40, -30, 0], [45, -25, 5], [0, 50, -5]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)


def strip():
    """two triangles sharing the edge (1, 2): open boundaries all round"""
    return (np.array([[-40, -30, 0], [45, -25, 5], [0, 50, -5], [70, 40, 10]], dtype=np.float32),
            np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32))


MESHES = {"tetrahedron": tetrahedron, "octahedron": octahedron, "icosphere": icosphere, "triangle": triangle, "strip": strip}
CLOSED = ("tetrahedron", "octahedron", "icosphere")


# ---- the chain
def mip_elems(F, R, L):
    if F <= 0 or not 1 <= R <= 64 or L < 1 or L > 7 or R % (1 << (L - 1)):
        return 0
    per_face = sum(texel_count(R >> l) for l in range(L))
    return 0 if F * per_face >= 1 << 31 else 3 * F * per_face


def slots_of(node_index):
    """the CSR pair of a node index [F,Tc] by plain loops: slot_ptr [U+1], slot_list [F Tc], the slots of a node ascending"""
    flat = np.asarray(node_index).reshape(-1)
    U = int(flat.max()) + 1
    lists = [[] for _ in range(U)]
    for s, u in enumerate(flat):
        lists[u].append(s)
    ptr = np.cumsum([0] + [len(l) for l in lists])
    return ptr.astype(np.int32), np.array([s for l in lists for s in l], dtype=np.int32)


def reduce_cells(F, Rf, slot_ptr, slot_list):
    """The rule's terms: per unique node u the list of (slot s, [(fine slot of the centre, of the midpoint along d_k, of the midpoint
    along d_(k+1)) per coarse cell at that corner, k ascending]) over its valid slots in list order."""
    Rc = Rf // 2
    Tf, Tc = texel_count(Rf), texel_count(Rc)
    ij = node_list(Rc)
    inside = lambda i, j: i >= 0 and j >= 0 and i + j <= Rc
    out = []
    for u in range(len(slot_ptr) - 1):
        terms = []
        for p in range(max(int(slot_ptr[u]), 0), min(int(slot_ptr[u + 1]), F * Tc)):
            s = int(slot_list[p])
            if s < 0 or s >= F * Tc:
                continue
            f, n = divmod(s, Tc)
            I, J = ij[n]
            cells = []
            for k in range(6):
                (ax, ay), (bx, by) = DIRS[k], DIRS[(k + 1) % 6]
                if inside(I + ax, J + ay) and inside(I + bx, J + by):
                    cells.append((f * Tf + node(2 * I, 2 * J, Rf), f * Tf + node(2 * I + ax, 2 * J + ay, Rf), f * Tf + node(2 * I + bx, 2 * J + by, Rf)))
            terms.append((s, cells))
        out.append(terms)
    return out


def reduce(fine, slot_ptr, slot_list):
    """fine [F,T(Rf),3] float32 -> coarse [F,T(Rf/2),3] float32 (zeros where no node names a slot)"""
    fine = np.asarray(fine, dtype=np.float32)
    F, Tf = fine.shape[:2]
    Rf = (int(np.sqrt(8 * Tf + 1)) - 3) // 2
    assert texel_count(Rf) == Tf and Rf % 2 == 0
    x = fine.reshape(-1, 3).astype(np.float64)
    coarse = np.zeros((F * texel_count(Rf // 2), 3), dtype=np.float32)
    with np.errstate(all="ignore"):
        for terms in reduce_cells(F, Rf, slot_ptr, slot_list):
            acc, wacc = np.zeros(3), 0.0
            for _, cells in terms:
                for c, a, b in cells:
                    acc = acc + ((2.0 * x[c] + 3.0 * x[a]) + 3.0 * x[b])
                    wacc = wacc + 8.0
            if not wacc > 0:
                continue
            value = (acc / wacc).astype(np.float32)
            for s, _ in terms:
                coarse[s] = value
    return coarse.reshape(F, -1, 3)


def reduce_matrix(F, Rf, slot_ptr, slot_list):
    """the filter as a dense matrix [U, F T(Rf)] (small meshes only): row u holds the weights of the fine slots in node u's value"""
    M = np.zeros((len(slot_ptr) - 1, F * texel_count(Rf)))
    for u, terms in enumerate(reduce_cells(F, Rf, slot_ptr, slot_list)):
        n = sum(len(cells) for _, cells in terms)
        for _, cells in terms:
            for c, a, b in cells:
                M[u, c] += 2.0 / (8.0 * n)
                M[u, a] += 3.0 / (8.0 * n)
                M[u, b] += 3.0 / (8.0 * n)
    return M


def chain(texels, node_index_of):
    """every level that exists below texels [F,T(R),3]: [level 0, level 1, ...] float32; node_index_of(Rc) -> [F,T(Rc)]"""
    levels = [np.asarray(texels, dtype=np.float32)]
    R = (int(np.sqrt(8 * levels[0].shape[1] + 1)) - 3) // 2
    while R % 2 == 0:
        R //= 2
        levels.append(reduce(levels[-1], *slots_of(node_index_of(R))))
    return levels


def pack(levels):
    return np.concatenate([np.asarray(l, dtype=np.float32).reshape(-1) for l in levels])


# ---- the shade
def weights(face, verts, faces, pose, intr, H, W):
    """K35's step 1 per pixel of one image -> ok [H,W], f [H,W] (0 where not ok), w (3 x [H,W], 0 where not ok) and the footprint's
    ingredients iz3 = (iz_0 iz_1) iz_2, area, S (before the clamp)"""
    V, F = len(verts), len(faces)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fb_ = face.astype(np.int64)
    ok = (fb_ >= 0) & (fb_ < F)
    f = np.where(ok, fb_, 0)
    vi = faces[f]
    ok &= ((vi >= 0) & (vi < V)).all(-1)
    vi = np.clip(vi, 0, V - 1)
    P, K = pose, intr
    X = verts[vi]
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
    S = (t[0] + t[1]) + t[2]
    w = [tk / S for tk in t]
    w = [np.where(wk < 0, 0.0, wk) for wk in w]
    s2 = (w[0] + w[1]) + w[2]
    w = [wk / s2 for wk in w]
    ok &= np.isfinite(w[0]) & np.isfinite(w[1]) & np.isfinite(w[2])
    w = [np.where(ok, wk, 0.0) for wk in w]
    return ok, f, w, (iz[..., 0] * iz[..., 1]) * iz[..., 2], area, S


def cell_colour(w, f, texels, R):
    """K35's step 2 and three-product sum on texels [F,T(R),3] (fp64) under the weights w"""
    T = texels.shape[1]
    a, bb = R * w[1], R * w[2]
    ci = np.minimum(np.floor(a).astype(np.int64), R - 1)
    cj = np.minimum(np.floor(bb).astype(np.int64), R - 1 - ci)
    fa, fb = a - ci, bb - cj
    upper = (fa + fb > 1.0) & (ci + cj <= R - 2)
    N = lambda i, j: texels[f, np.clip(node(i, j, R), 0, T - 1)]
    lo = ((1.0 - fa) - fb)[..., None] * N(ci, cj) + fa[..., None] * N(ci + 1, cj) + fb[..., None] * N(ci, cj + 1)
    up = ((fa + fb) - 1.0)[..., None] * N(ci + 1, cj + 1) + (1.0 - fb)[..., None] * N(ci + 1, cj) + (1.0 - fa)[..., None] * N(ci, cj + 1)
    return np.where(upper[..., None], up, lo)


def select(d, L):
    """the level rule -> l0 [..] int, t [..] fp64 (0 where one level is read)"""
    with np.errstate(all="ignore"):
        one = ~(d > 1.0) | ~np.isfinite(d) | (L == 1)
        ds = np.where(one, 2.0, d)
        e = np.frexp(ds)[1].astype(np.int64) - 1                    # ilogb
        l0 = np.minimum(e >> 1, L - 1)
        t = (np.ldexp(ds, (-2 * l0).astype(np.int32)) - 1.0) / 3.0
        t = np.where(one | (l0 == L - 1), 0.0, t)
        return np.where(one, 0, l0), t


def shade(face, verts, faces, levels, pose, intr, H, W, footprint=1.0, details=False):
    """face [B,H,W] int, levels [level 0 .. level L-1] each [F,T(R_l),3] -> rgb [B,H,W,3] float64 BEFORE the rounding to fp32
    (``details``: also d, l0, t per pixel)"""
    face = np.asarray(face).reshape(-1, H, W)
    B = face.shape[0]
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    levels = [np.asarray(l, dtype=np.float32).astype(np.float64) for l in levels]
    L = len(levels)
    R = (int(np.sqrt(8 * levels[0].shape[1] + 1)) - 3) // 2
    assert all(l.shape[1] == texel_count(R >> k) for k, l in enumerate(levels)) and R % (1 << (L - 1)) == 0
    pose = np.asarray(pose, dtype=np.float64).reshape(B, 3, 4)
    intr = np.broadcast_to(np.asarray(intr, dtype=np.float64), (B, 3, 3))
    fp = float(np.float32(footprint))
    out, ds, ls, ts = np.zeros((B, H, W, 3)), np.zeros((B, H, W)), np.zeros((B, H, W), dtype=np.int64), np.zeros((B, H, W))
    with np.errstate(all="ignore"):
        for b in range(B):
            ok, f, w, iz3, area, S = weights(face[b], verts, faces, pose[b], intr[b], H, W)
            aS = np.abs(S)
            d = ((fp * float(R * R)) * np.abs(iz3)) / (np.abs(area) * ((aS * aS) * aS))
            l0, t = select(d, L)
            cols = [cell_colour(w, f, levels[l], R >> l) for l in range(L)]
            col = np.zeros((H, W, 3))
            for l in range(L):
                here = (l0 == l)[..., None]
                nxt = cols[min(l + 1, L - 1)]
                blend = (1.0 - t)[..., None] * cols[l] + t[..., None] * nxt
                col = np.where(here, np.where((t > 0)[..., None], blend, cols[l]), col)
            ok &= np.isfinite(col).all(-1)
            out[b] = np.where(ok[..., None], col, 0.0)
            ds[b], ls[b], ts[b] = d, l0, t
    return (out, ds, ls, ts) if details else out


def bary_at(tri, pose, intr, px, py):
    """the perspective-correct weights (no clamp) of one triangle tri [3,3] at continuous screen positions px, py -> w [3, ...], S"""
    tri, P, K = (np.asarray(x, dtype=np.float64) for x in (tri, pose, intr))
    c = tri @ P[:, :3].T + P[:, 3]
    q = c @ K.T
    u, v, iz = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], 1.0 / c[:, 2]
    area = (u[1] - u[0]) * (v[2] - v[0]) - (v[1] - v[0]) * (u[2] - u[0])
    t = []
    for k in range(3):
        s, e = (k + 1) % 3, (k + 2) % 3
        t.append((((u[e] - u[s]) * (py - v[s]) - (v[e] - v[s]) * (px - u[s])) / area) * iz[k])
    S = (t[0] + t[1]) + t[2]
    return np.stack([tk / S for tk in t]), S
