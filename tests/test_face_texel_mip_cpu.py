"""No GPU: K43's binding and refusals, the host side of the mip chain (face_texels.mip_levels, mip_slots) and the fp64 restatement of
both rules (tests/face_texel_mip_ref.py) against independent statements of what they mean: the reduce against the closed-manifold
formula and a brute-force cell sum, the footprint against a finite difference, the level rule against K35's restatement at both ends,
and the filter's quality against a supersampled render."""
import ctypes as C

import numpy as np
import pytest

import face_texel_mip_ref as MREF
import face_texels_ref as REF
import mesh_raster_ref as RAST
from texpose_amd import _lib
from texpose_amd import face_texels as FT
from texpose_amd import texture_bake as TB


def test_binding_counts_and_refusals_without_a_gpu():
    assert _lib.ABI_VERSION == 16
    for s in ("tp_face_texel_mip_elems", "tp_face_texel_mip_reduce", "tp_face_texel_shade_mip"):
        assert s in _lib.SYMBOLS
    assert [f[0] for f in _lib.FaceTexelMipReduceArgs._fields_] == ["fine", "slot_ptr", "slot_list", "F", "Rf", "U", "coarse"]
    assert [f[0] for f in _lib.FaceTexelShadeMipArgs._fields_] == ["verts", "faces", "mips", "pose", "intr", "face", "B", "H", "W", "V", "F", "R", "L",
                                                                    "footprint", "rgb"]
    lib = _lib.load()
    T = FT.texel_count
    # R = 1: one level; 2: two; 6: two (6, 3); 64: seven
    assert [FT.mip_levels(R) for R in (1, 2, 6, 64, 3, 48)] == [1, 2, 2, 7, 1, 5]
    for F in (1, 20):
        assert lib.tp_face_texel_mip_elems(F, 1, 1) == 3 * F * 3 and lib.tp_face_texel_mip_elems(F, 1, 2) == 0
        assert lib.tp_face_texel_mip_elems(F, 2, 1) == 3 * F * 6 and lib.tp_face_texel_mip_elems(F, 2, 2) == 3 * F * 9 and lib.tp_face_texel_mip_elems(F, 2, 3) == 0
        assert lib.tp_face_texel_mip_elems(F, 6, 2) == 3 * F * (T(6) + T(3)) and lib.tp_face_texel_mip_elems(F, 6, 3) == 0
        assert lib.tp_face_texel_mip_elems(F, 64, 7) == 3 * F * sum(T(64 >> l) for l in range(7)) and lib.tp_face_texel_mip_elems(F, 64, 8) == 0
        for R in (1, 2, 6, 64):
            for L in range(0, 9):
                assert lib.tp_face_texel_mip_elems(F, R, L) == MREF.mip_elems(F, R, L), (F, R, L)
    assert [lib.tp_face_texel_mip_elems(*a) for a in ((0, 8, 1), (-1, 8, 1), (4, 0, 1), (4, 65, 1), (4, 8, 0), (4, 8, -1), (4, 3, 2), ((1 << 31) // 2145 + 1, 64, 1))] == [0] * 8

    # the reduce
    assert lib.tp_face_texel_mip_reduce(None, None) == -1 and b"null args" in lib.tp_last_error()
    assert lib.tp_face_texel_mip_reduce(C.byref(_lib.FaceTexelMipReduceArgs()), None) == -1 and b"null pointer" in lib.tp_last_error()

    def reduce_refused(word=b"bad sizes", **change):
        a = _lib.FaceTexelMipReduceArgs()
        a.fine = a.slot_ptr = a.slot_list = a.coarse = 64             # never dereferenced: every case is refused
        for k, v in {**dict(F=1, Rf=2, U=3), **change}.items():
            setattr(a, k, v)
        return lib.tp_face_texel_mip_reduce(C.byref(a), None) == -1 and word in lib.tp_last_error() and b"tp_face_texel_mip_reduce" in lib.tp_last_error()

    for change in (dict(F=0), dict(F=-1), dict(U=0), dict(U=-2), dict(Rf=0), dict(Rf=1), dict(Rf=3), dict(Rf=63), dict(Rf=66), dict(Rf=-2),
                   dict(F=(1 << 31) // 2145 + 1, Rf=64)):
        assert reduce_refused(**change), change
    for p in ("fine", "slot_ptr", "slot_list", "coarse"):
        assert reduce_refused(b"null pointer", **{p: None}), p

    # the shade
    assert lib.tp_face_texel_shade_mip(None, None) == -1 and b"null args" in lib.tp_last_error()
    assert lib.tp_face_texel_shade_mip(C.byref(_lib.FaceTexelShadeMipArgs()), None) == -1 and b"null pointer" in lib.tp_last_error()
    good = dict(B=1, H=8, W=8, V=3, F=1, R=8, L=4, footprint=1.0)

    def shade_refused(word=b"bad sizes", **change):
        a = _lib.FaceTexelShadeMipArgs()
        a.verts = a.faces = a.mips = a.pose = a.intr = a.face = a.rgb = 64
        for k, v in {**good, **change}.items():
            setattr(a, k, v)
        return lib.tp_face_texel_shade_mip(C.byref(a), None) == -1 and word in lib.tp_last_error() and b"tp_face_texel_shade_mip" in lib.tp_last_error()

    for k in ("B", "H", "W", "V", "F", "R", "L"):
        assert shade_refused(**{k: 0}) and shade_refused(**{k: -1}), k
    assert shade_refused(R=65, L=1) and shade_refused(R=7, L=2) and shade_refused(R=8, L=5) and shade_refused(R=6, L=3) and shade_refused(R=64, L=8)
    assert shade_refused(H=1 << 16, W=1 << 15) and shade_refused(B=1 << 30, H=64, W=64)
    assert shade_refused(F=(1 << 31) // (2145 + 561) + 1, R=64, L=2)
    for fp in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert shade_refused(b"footprint", footprint=fp), fp
    for p in ("verts", "faces", "mips", "pose", "intr", "face", "rgb"):
        assert shade_refused(b"null pointer", **{p: None}), p


_sub = {}


def subdivided(name, R):
    if (name, R) not in _sub:
        verts, faces = MREF.MESHES[name]()
        _sub[name, R] = (verts, faces) + FT.subdivide(verts, faces, R)
    return _sub[name, R]


@pytest.mark.parametrize("name", list(MREF.MESHES))
def test_mip_slots_is_a_stable_permutation(name):
    for Rc in (1, 2, 3, 4, 32):
        verts, faces, vs, _, ni = subdivided(name, Rc)
        ptr, lst = FT.mip_slots(verts, faces, Rc)
        again = FT.mip_slots(verts, faces, Rc)
        assert ptr.dtype == np.int32 and lst.dtype == np.int32 and (ptr == again[0]).all() and (lst == again[1]).all()
        assert ptr.shape == (len(vs) + 1,) and ptr[0] == 0 and ptr[-1] == ni.size and (np.diff(ptr) >= 1).all()
        assert (np.sort(lst) == np.arange(ni.size)).all()                               # a permutation of the slots
        for u in range(len(vs)):
            mine = lst[ptr[u]:ptr[u + 1]]
            assert (ni.reshape(-1)[mine] == u).all() and (np.diff(mine) > 0).all()         # node u's slots, ascending
        want = MREF.slots_of(ni)
        assert (ptr == want[0]).all() and (lst == want[1]).all()


def node_values(name, R, seed):
    """random values on the unique nodes, gathered per face: a texture that is continuous across edges"""
    _, _, vs, _, ni = subdivided(name, R)
    return np.random.RandomState(seed).rand(len(vs), 3).astype(np.float32)[ni]


@pytest.mark.parametrize("Rf", [2, 4, 8])
@pytest.mark.parametrize("name", MREF.CLOSED)
def test_reduce_on_closed_meshes_is_quarter_centre_plus_three_quarter_edge_midpoints(name, Rf):
    """On a closed manifold every coarse node has as many incident coarse cells as incident coarse edges and each edge lies in two of
    them, so the cell rule is x_c / 4 + 3/4 mean(midpoints of the coarse MESH's incident edges): computed here from
    mesh_edges(faces_sub) and the subdivided mesh's geometry alone (the midpoint of a coarse edge is found by position)."""
    verts, faces, vs_c, fs_c, ni_c = subdivided(name, Rf // 2)
    _, _, vs_f, _, ni_f = subdivided(name, Rf)
    x_nodes = np.random.RandomState(Rf).rand(len(vs_f), 3).astype(np.float32)
    fine = x_nodes[ni_f]
    got = MREF.reduce(fine, *FT.mip_slots(verts, faces, Rf // 2))
    # fine node of a position: exact fp64 positions are not shared between the two subdivisions, so match to 1e-3 mm
    pos_f = vs_f.astype(np.float64)
    find = lambda p: int(np.argmin(((pos_f - p) ** 2).sum(1)))
    edges = TB.mesh_edges(fs_c)
    mids = [[] for _ in range(len(vs_c))]
    for a, b in edges:
        m = find(0.5 * (vs_c[a].astype(np.float64) + vs_c[b]))
        assert np.abs(pos_f[m] - 0.5 * (vs_c[a].astype(np.float64) + vs_c[b])).max() < 1e-3
        mids[a].append(m)
        mids[b].append(m)
    want = np.zeros((len(vs_c), 3))
    for u in range(len(vs_c)):
        c = find(vs_c[u].astype(np.float64))
        want[u] = 0.25 * x_nodes[c].astype(np.float64) + 0.75 * x_nodes[mids[u]].astype(np.float64).mean(0)
    # fp64 rounding of <= 12 cells' sums of values in [0, 1], then one rounding to fp32 (half an ulp of 1: 6e-8)
    d = np.abs(got.astype(np.float64) - want[ni_c]).max()
    print("%s Rf=%d: max |cell rule - closed-manifold formula| %.2e" % (name, Rf, d))
    assert d <= 6e-8 + 1e-14


@pytest.mark.parametrize("name", ["triangle", "strip"])
def test_reduce_on_open_meshes_is_the_brute_force_cell_sum(name):
    """every coarse cell (sub-face of the mesh subdivided Rc times) adds 2 x corner + 3 x (the midpoints of its two edges at that corner)
    to each of its three corners, weight 8: summed per unique node over faces_sub, midpoints found by position"""
    for Rf in (2, 4, 8):
        verts, faces, vs_c, fs_c, ni_c = subdivided(name, Rf // 2)
        _, _, vs_f, _, ni_f = subdivided(name, Rf)
        x_nodes = np.random.RandomState(10 + Rf).rand(len(vs_f), 3).astype(np.float32).astype(np.float64)
        pos_f = vs_f.astype(np.float64)
        find = lambda p: int(np.argmin(((pos_f - p) ** 2).sum(1)))
        acc, wacc = np.zeros((len(vs_c), 3)), np.zeros(len(vs_c))
        for tri in fs_c:
            for k in range(3):
                c, a, b = tri[k], tri[(k + 1) % 3], tri[(k + 2) % 3]
                pc = vs_c[c].astype(np.float64)
                acc[c] += 2.0 * x_nodes[find(pc)] + 3.0 * x_nodes[find(0.5 * (pc + vs_c[a]))] + 3.0 * x_nodes[find(0.5 * (pc + vs_c[b]))]
                wacc[c] += 8.0
        got = MREF.reduce(x_nodes.astype(np.float32)[ni_f], *FT.mip_slots(verts, faces, Rf // 2))
        d = np.abs(got.astype(np.float64) - (acc / wacc[:, None])[ni_c]).max()
        print("%s Rf=%d: max |cell rule - brute force over faces_sub| %.2e" % (name, Rf, d))
        assert d <= 6e-8 + 1e-14


@pytest.mark.parametrize("name", list(MREF.MESHES))
def test_reduce_constants_shared_nodes_and_weights(name):
    verts, faces = MREF.MESHES[name]()
    F = len(faces)
    for R in (8, 6):
        const = np.empty((F, FT.texel_count(R), 3), dtype=np.float32)
        const[:] = np.float32([0.1, 0.7, 1.0 / 3.0])
        for level in MREF.chain(const, lambda Rc: subdivided(name, Rc)[4]):
            assert (level.view(np.uint32) == const[:, :level.shape[1]].view(np.uint32)).all()       # a constant comes back bit for bit
        levels = MREF.chain(node_values(name, R, 3), lambda Rc: subdivided(name, Rc)[4])
        assert [l.shape[1] for l in levels] == [FT.texel_count(R >> l) for l in range(FT.mip_levels(R))]
        for l, level in enumerate(levels[1:], 1):
            ni = subdivided(name, R >> l)[4]
            per_node = FT.nodes_from_texels(level, ni)
            assert (per_node[ni].view(np.uint32) == level.view(np.uint32)).all()                 # faces sharing a node hold equal bits
    for Rf in (2, 4, 6):
        ptr, lst = FT.mip_slots(verts, faces, Rf // 2)
        M = MREF.reduce_matrix(F, Rf, ptr, lst)
        assert (M >= 0).all() and np.abs(M.sum(1) - 1.0).max() <= 1e-15


def test_reduce_propagates_non_finite_and_skips_bad_slots():
    verts, faces = MREF.octahedron()
    fine = node_values("octahedron", 4, 5).copy()
    ptr, lst = FT.mip_slots(verts, faces, 2)
    base = MREF.reduce(fine, ptr, lst)
    fine[0, REF.node(1, 0, 4)] = np.nan                     # a midpoint of face 0's first coarse edge
    got = MREF.reduce(fine, ptr, lst)
    touched = ~np.isfinite(got).all(-1)
    assert touched[0, REF.node(0, 0, 2)] and touched[0, REF.node(1, 0, 2)] and touched.sum() < touched.size / 2
    assert (got[~touched] == base[~touched]).all()
    bad = lst.copy()
    bad[[0, 5]] = [-1, len(lst)]
    skipped = MREF.reduce(node_values("octahedron", 4, 5), ptr, bad)
    assert (skipped.reshape(-1, 3)[lst[[0, 5]]] == 0).all() and np.isfinite(skipped).all()


# ---- the shade
def tilted():
    """one face tilted about both axes under a short focal length: the perspective map is far from affine"""
    verts, faces = MREF.triangle()
    a, b = 0.9, -0.5
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    pose = np.concatenate([Rx @ Ry, [[2.0], [-3.0], [140.0]]], axis=1).astype(np.float32)
    return verts, faces, pose


def test_footprint_against_a_central_difference():
    """d (footprint = 1) is |det d(R w_1, R w_2) / d(px, py)|.  The check: a central difference over +-1/2 pixel of the unclamped
    weights.  Each w is N / S with N and S affine in the pixel, and the central difference of such a quotient with step h along x is
    EXACTLY the derivative over (1 - (h S_x / S)^2); so the difference quotient's determinant is d / ((1 - e_x)(1 - e_y)), e = (S_x /
    (2 S))^2, (S_y / (2 S))^2: its truncation error relative to d is e_x + e_y to first order.  The tolerance is twice that per pixel
    (the higher orders; e < 0.1 is asserted) plus 1e-9 for the fp64 cancellation in differences of weights 1/2 pixel apart."""
    verts, faces, pose = tilted()
    H, W, R = 37, 53, 8
    K = np.array([[60.0, 0, W / 2.0], [0, 60.0, H / 2.0], [0, 0, 1]], dtype=np.float32)
    face = RAST.rasterize(verts, faces, pose, K, H, W)["face"].reshape(1, H, W)
    levels = [np.zeros((1, FT.texel_count(R >> l), 3), dtype=np.float32) for l in range(4)]
    _, d, _, _ = MREF.shade(face, verts, faces, levels, pose[None], K, H, W, details=True)
    ii, jj = np.nonzero(face[0] >= 0)
    assert len(ii) >= 150
    px, py = jj + 0.5, ii + 0.5
    tri = verts[faces[0]]
    h = 0.5
    wxp, Sxp = MREF.bary_at(tri, pose, K, px + h, py)
    wxm, Sxm = MREF.bary_at(tri, pose, K, px - h, py)
    wyp, Syp = MREF.bary_at(tri, pose, K, px, py + h)
    wym, Sym = MREF.bary_at(tri, pose, K, px, py - h)
    S = MREF.bary_at(tri, pose, K, px, py)[1]
    ax, ay = R * (wxp[1] - wxm[1]) / (2 * h), R * (wyp[1] - wym[1]) / (2 * h)
    bx, by = R * (wxp[2] - wxm[2]) / (2 * h), R * (wyp[2] - wym[2]) / (2 * h)
    fd = np.abs(ax * by - ay * bx)
    ex, ey = (h * (Sxp - Sxm) / (2 * h) / S) ** 2, (h * (Syp - Sym) / (2 * h) / S) ** 2
    rel = np.abs(fd / d[0, ii, jj] - 1.0)
    print("footprint: d in %.3g .. %.3g, max |fd / d - 1| %.2e, truncation e_x + e_y up to %.2e" % (d[0, ii, jj].min(), d[0, ii, jj].max(), rel.max(), (ex + ey).max()))
    assert (ex + ey).max() < 0.1 and d[0, ii, jj].max() / d[0, ii, jj].min() > 1.5       # a real perspective change across the face
    assert (rel <= 2.0 * (ex + ey) + 1e-9).all()
    exact = np.abs(fd * (1.0 - ex) * (1.0 - ey) / d[0, ii, jj] - 1.0).max()                   # the identity itself, to fp64 cancellation
    print("footprint: the exact identity holds to %.2e" % exact)
    assert exact <= 1e-9


def test_level_rule_ends_are_k35s_restatement_bit_for_bit():
    verts, faces = MREF.icosphere()
    H, W, R = 37, 53, 8
    poses = TB.sphere_view_poses(3, 400.0).astype(np.float32)
    texels = node_values("icosphere", R, 11)
    levels = MREF.chain(texels, lambda Rc: subdivided("icosphere", Rc)[4])
    assert len(levels) == 4
    face = np.zeros((3, H, W), dtype=np.int64)
    face[:] = (np.arange(H * W).reshape(H, W) % 23 - 2)[None]                          # valid faces, -2, -1 and 20 (= F): every pixel decided
    # magnified: a long focal length
    K = np.array([[900.0, 0, W / 2.0], [0, 900.0, H / 2.0], [0, 0, 1]], dtype=np.float32)
    want = REF.shade(face, verts, faces, texels, poses, K, H, W)
    got, d, l0, t = MREF.shade(face, verts, faces, levels, poses, K, H, W, details=True)
    near = d <= 1                                                                      # (the plane hands pixels to oblique faces too)
    assert near.mean() > 0.5 and (got[near] == want[near]).all() and (want[near] != 0).any()
    one = MREF.shade(face, verts, faces, levels[:1], poses, K, H, W)                  # L = 1: K35 at any distance
    assert (one == want).all()
    Kfar = np.array([[3.0, 0, W / 2.0], [0, 3.0, H / 2.0], [0, 0, 1]], dtype=np.float32)
    assert (MREF.shade(face, verts, faces, levels[:1], poses, Kfar, H, W) == REF.shade(face, verts, faces, texels, poses, Kfar, H, W)).all()
    # far: d >= 4^(L-1) = 64 wherever it is finite
    got, d, l0, t = MREF.shade(face, verts, faces, levels, poses, Kfar, H, W, details=True)
    far = np.isfinite(d) & (d >= 64)
    last = REF.shade(face, verts, faces, levels[-1], poses, Kfar, H, W)
    assert far.mean() > 0.2 and (l0[far] == 3).all() and (t[far] == 0).all()
    assert (got[far] == last[far]).all() and (last[far] != 0).any()
    # in between: t in [0, 1) and the blend lies between its two levels
    Kmid = np.array([[40.0, 0, W / 2.0], [0, 40.0, H / 2.0], [0, 0, 1]], dtype=np.float32)
    got, d, l0, t = MREF.shade(face, verts, faces, levels, poses, Kmid, H, W, details=True)
    mid = np.isfinite(d) & (d > 1) & (d < 64)
    assert mid.mean() > 0.3 and (t >= 0).all() and (t < 1).all() and set(np.unique(l0[mid])) <= {0, 1, 2} and len(np.unique(l0[mid])) >= 2
    assert (4.0 ** l0[mid] <= d[mid]).all() and (d[mid] < 4.0 ** (l0[mid] + 1)).all()
    assert np.abs(t[mid] - (d[mid] / 4.0 ** l0[mid] - 1.0) / 3.0).max() <= 1e-15


def test_select_rule():
    d = np.array([0.0, 0.5, 1.0, np.nextafter(1.0, 2), 2.5, 4.0, 15.999, 16.0, 63.0, 64.0, 1e6, np.inf, np.nan, -1.0])
    l0, t = MREF.select(d, 4)
    assert l0.tolist() == [0, 0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 0, 0, 0]
    assert t[[0, 1, 2, 5, 7, 9, 10, 11, 12, 13]].tolist() == [0.0] * 10 and t[4] == 0.5 and 0 < t[3] < 1e-15 and 0.99 < t[6] < 1 and t[8] == (63.0 / 16.0 - 1.0) / 3.0
    l0, t = MREF.select(d, 1)
    assert not l0.any() and not t.any()
    l0, t = MREF.select(d, 2)
    assert l0.tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0] and t[5] == 0


# ---- quality
def box_down(img, k):
    H, W = img.shape[0] // k, img.shape[1] // k
    return img.reshape(H, k, W, k, -1).mean((1, 3))


QUALITY = {}


def quality():
    """The icosphere at R = 16 under a texel-scale checker and a sine (wavelength about three texels), seen from six directions at the
    three distances where a face's d is about 4, 16 and 64 (24 x 24 pixels, focal length 100): rms of the point-sampled and of the mip
    render against the truth -- the point-sampled render at 8 x the image size, box-filtered down -- over the pixels whose 64
    sub-pixels are all covered.  -> {(texture, d): (rms point, rms mip, pixels)}"""
    if QUALITY:
        return QUALITY
    verts, faces = MREF.icosphere()
    R, H, W, S, focal = 16, 24, 24, 8, 100.0
    vs, _, ni = subdivided("icosphere", R)[2:]
    cell = FT.mean_edge_length(verts, faces) / R
    p = vs.astype(np.float64)
    checker = ((np.floor(p / cell).sum(1) % 2)[:, None] * np.ones(3)).astype(np.float32)
    textures = {"checker": checker[ni], "sine": REF.fine_colour(vs, period_mm=cell * 3.0 / (2.0 * np.pi)).astype(np.float32)[ni]}
    edge = FT.mean_edge_length(verts, faces)
    for name, texels in textures.items():
        levels = MREF.chain(texels, lambda Rc: subdivided("icosphere", Rc)[4])
        for target in (4.0, 16.0, 64.0):
            # fronto-parallel: d = R^2 / (twice the face's area in pixels) = R^2 / (sqrt(3) / 2 (edge focal / D)^2)
            D = edge * focal / np.sqrt(R * R / (target * np.sqrt(3.0) / 2.0))
            poses = TB.sphere_view_poses(6, D).astype(np.float32)
            K = np.array([[focal, 0, W / 2.0], [0, focal, H / 2.0], [0, 0, 1]], dtype=np.float32)
            Kbig = (np.diag([S, S, 1.0]) @ K).astype(np.float32)
            face = np.stack([RAST.rasterize(verts, faces, P, K, H, W)["face"].reshape(H, W) for P in poses])
            big = np.stack([RAST.rasterize(verts, faces, P, Kbig, H * S, W * S)["face"].reshape(H * S, W * S) for P in poses])
            truth = np.stack([box_down(im, S) for im in REF.shade(big, verts, faces, texels, poses, Kbig, H * S, W * S)])
            full = np.stack([box_down((b >= 0)[..., None].astype(np.float64), S)[..., 0] == 1.0 for b in big]) & (face >= 0)
            point = REF.shade(face, verts, faces, texels, poses, K, H, W)
            mip, d, _, _ = MREF.shade(face, verts, faces, levels, poses, K, H, W, details=True)
            rms = lambda im: float(np.sqrt(((im - truth)[full] ** 2).mean()))
            QUALITY[name, target] = (rms(point), rms(mip), int(full.sum()), float(np.median(d[full])))
    return QUALITY


@pytest.mark.parametrize("target", [4.0, 16.0, 64.0])
@pytest.mark.parametrize("texture", ["checker", "sine"])
def test_mip_render_is_closer_to_the_supersampled_truth_than_point_sampling(texture, target):
    point, mip, n, d = quality()[texture, target]
    print("%s at d ~ %g (median d %.3g over %d pixels): rms point-sampled %.4f, mip %.4f" % (texture, target, d, n, point, mip))
    assert n >= 20 and 0.4 * target <= d <= 2.5 * target
    assert mip < point
