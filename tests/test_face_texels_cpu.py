"""No GPU: the fp64 restatement of K35 (tests/face_texels_ref.py) and the host side of texpose_amd.face_texels -- the grid of
resolution R on every face is the vertex set of the mesh subdivided R times, so shading the base mesh with texels must equal
rasterising the subdivided mesh with vertex colours (mesh_raster_ref.rasterize on both routes)."""
import ctypes as C

import numpy as np
import pytest

import face_texels_ref as REF
import mesh_raster_ref as RAST
import texture_bake_ref as TREF
from texpose_amd import _lib
from texpose_amd import face_texels as FT
from texpose_amd import texture_bake as TB

MESHES = {"sphere": lambda: TREF.uv_sphere(12, 16), "torus": lambda: TREF.torus(24, 12)}
FOCAL = {"sphere": 200.0, "torus": 260.0}
_sub = {}


def subdivided(name, R):
    if (name, R) not in _sub:
        verts, faces = MESHES[name]()
        _sub[name, R] = (verts, faces) + FT.subdivide(verts, faces, R)
    return _sub[name, R]


def test_symbols_counts_and_refusals_without_a_gpu():
    assert _lib.ABI_VERSION == 16 and _lib.FACE_TEXEL_MAX_R == 64 == FT.MAX_R
    assert "tp_face_texel_shade" in _lib.SYMBOLS and "tp_face_texel_count" in _lib.SYMBOLS
    assert [f[0] for f in _lib.FaceTexelShadeArgs._fields_] == ["verts", "faces", "texels", "pose", "intr", "face", "B", "H", "W", "V", "F", "R", "rgb"]
    lib = _lib.load()
    assert lib.tp_abi_version() == 16
    assert [lib.tp_face_texel_count(R) for R in (1, 2, 8, 64, 0, 65, -3)] == [3, 6, 45, 2145, 0, 0, 0]
    assert [FT.texel_count(R) for R in (1, 2, 8, 64)] == [3, 6, 45, 2145] and [FT.resolution_of(T) for T in (3, 6, 45, 2145)] == [1, 2, 8, 64]
    for bad in (0, 65):
        with pytest.raises(ValueError):
            FT.texel_count(bad)
    with pytest.raises(ValueError):
        FT.resolution_of(7)
    assert lib.tp_face_texel_shade(None, None) == -1 and b"null args" in lib.tp_last_error()
    a = _lib.FaceTexelShadeArgs()
    assert lib.tp_face_texel_shade(C.byref(a), None) == -1 and b"null pointer" in lib.tp_last_error()
    good = dict(B=1, H=8, W=8, V=3, F=1, R=1)

    def refused(**change):
        a = _lib.FaceTexelShadeArgs()
        a.verts = a.faces = a.texels = a.pose = a.intr = a.face = a.rgb = 64         # never dereferenced: every case is refused
        for k, v in {**good, **change}.items():
            setattr(a, k, v)
        return lib.tp_face_texel_shade(C.byref(a), None) == -1 and b"bad sizes" in lib.tp_last_error()

    for k in good:
        assert refused(**{k: 0}) and refused(**{k: -1}), k
    assert refused(R=65)
    assert refused(H=1 << 16, W=1 << 15)                       # H * W = 2^31
    assert refused(F=(1 << 31) // 2145 + 1, R=64)              # F * T >= 2^31
    assert refused(F=715827883, R=1)                           # 3 F >= 2^31
    assert refused(B=1 << 30, H=64, W=64)                      # more workgroups than a grid holds


def test_node_layout():
    for R in (1, 2, 3, 8, 64):
        ij, w = FT.node_ij(R), FT.node_weights(R)
        assert len(ij) == FT.texel_count(R) and [tuple(x) for x in ij] == REF.node_list(R)
        assert (ij[:, 1] * (R + 1) - ij[:, 1] * (ij[:, 1] - 1) // 2 + ij[:, 0] == np.arange(len(ij))).all()
        assert np.allclose(w.sum(1), 1, atol=1e-15) and (w >= 0).all()
        assert (w[REF.node(0, 0, R)] == (1, 0, 0)).all() and (w[REF.node(R, 0, R)] == (0, 1, 0)).all() and (w[REF.node(0, R, R)] == (0, 0, 1)).all()
    assert FT.resolution_for(10.0, 600.0, 750.0) == 8 and FT.resolution_for(1.0, 100.0, 1000.0) == 1 and FT.resolution_for(500.0, 600.0, 100.0) == 64
    v, f = TREF.torus(8, 5)
    e = TB.mesh_edges(f)
    assert np.isclose(FT.mean_edge_length(v, f), np.linalg.norm(v[e[:, 0]].astype(np.float64) - v[e[:, 1]], axis=1).mean())


@pytest.mark.parametrize("R", [1, 2, 3, 8])
@pytest.mark.parametrize("name", list(MESHES))
def test_subdivide_invariants(name, R):
    verts, faces, vs, fs, ni = subdivided(name, R)
    V, F, E = len(verts), len(faces), len(TB.mesh_edges(faces))
    T = FT.texel_count(R)
    assert vs.dtype == np.float32 and vs.shape == (V + E * (R - 1) + F * (R - 1) * (R - 2) // 2, 3)
    assert fs.shape == (F * R * R, 3) and ni.shape == (F, T) and ni.min() == 0 and ni.max() == len(vs) - 1
    assert len(np.unique(ni)) == len(vs)                                    # every row is some face's node
    if R == 1:
        assert (vs == verts).all() and (fs == faces).all() and (ni == faces).all()
    # the restatement's loops give the same mesh, bit for bit
    rv, rf, rn = REF.subdivide(verts, faces, R)
    assert (rv == vs).all() and (rf == fs).all() and (rn == ni).all()
    # node positions: within 1 ulp (fp32) of the weights' combination of the face's vertices, for every face that names the node
    w = FT.node_weights(R)
    want = np.einsum("tk,fkc->ftc", w, verts.astype(np.float64)[faces])
    got = vs[ni].astype(np.float64)
    # (1 ulp of the largest of the three coordinates combined: where they cancel, the fp64 rounding of the terms is all that is left)
    ulp = np.spacing(np.abs(verts[faces]).max(1))[:, None, :].astype(np.float64)
    assert (np.abs(got - want) <= ulp).all()
    # the two faces of every edge index the same edge nodes: each inner edge node row is named by exactly the faces at its edge
    if R > 1:
        ij = FT.node_ij(R)
        on_edge = lambda a, b: [REF.node(*p, R) for p in ([(k, 0) for k in range(1, R)] if (a, b) == (0, 1) else
                                                          [(0, k) for k in range(1, R)] if (a, b) == (0, 2) else
                                                          [(R - k, k) for k in range(1, R)])]
        seen = {}
        for f_i, face in enumerate(faces):
            for a, b in ((0, 1), (0, 2), (1, 2)):
                rows = ni[f_i, on_edge(a, b)]
                if face[a] > face[b]:
                    rows = rows[::-1]
                key = (min(face[a], face[b]), max(face[a], face[b]))
                if key[0] == key[1]:
                    continue
                assert (seen.setdefault(key, rows) == rows).all(), key
                assert (rows >= V).all() and (rows < V + E * (R - 1)).all()
        assert len(seen) == E
        assert len(ij) == T
    # sub-faces keep the face's orientation and tile it: their areas add up to the face's
    area = lambda v, f: np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    a_sub = area(vs.astype(np.float64), fs).reshape(F, R * R).sum(1)
    assert np.allclose(a_sub, area(verts.astype(np.float64), faces), rtol=1e-5, atol=1e-4)
    back = FT.nodes_from_texels(FT.texels_from_nodes(vs, ni), ni, len(vs))
    assert (back == vs).all()


# (frame, R): 64 x 80 as measured for the issue; R = 8 on a smaller frame to keep the brute-force raster of F R^2 faces short (even sizes: with
# an odd width the pixel centres of the middle column lie ON the projected meridian edges of these symmetric meshes, where coverage is
# decided by the last bit of a vertex and the two routes legitimately differ)
@pytest.mark.parametrize("R,H,W,scale", [(1, 64, 80, 1.0), (2, 64, 80, 1.0), (3, 64, 80, 1.0), (8, 36, 52, 0.6)])
@pytest.mark.parametrize("name", list(MESHES))
def test_texels_on_the_base_mesh_equal_vertex_colours_on_the_subdivided_one(name, R, H, W, scale):
    verts, faces, vs, fs, ni = subdivided(name, R)
    K = TREF.pinhole(H, W, FOCAL[name] * scale)
    pose = TB.sphere_view_poses(5, 400.0).astype(np.float32)[2]
    col = REF.fine_colour(vs)                                               # 3 mm period: far below the vertex spacing
    base = RAST.rasterize(verts, faces, pose, K, H, W)
    sub = RAST.rasterize(vs, fs, pose, K, H, W, vcolor=col)
    rgb = REF.shade(base["face"].reshape(1, H, W), verts, faces, FT.texels_from_nodes(col, ni), pose[None], K, H, W).reshape(-1, 3)
    covered = base["face"] >= 0
    assert ((sub["face"] >= 0) == covered).all() and covered.sum() > 300
    assert (sub["face"][covered] // (R * R) == base["face"][covered]).all()  # and the winning sub-face lies in the winning face
    diff = np.abs(rgb - sub["rgb"])[covered].max()
    print(name, R, "max |texel route - subdivided route| %.3g on %d pixels" % (diff, covered.sum()))
    assert diff <= 5e-5
    assert (rgb[~covered] == 0).all()


def test_shade_zero_rules_of_the_restatement():
    verts, faces = TREF.uv_sphere(6, 8)
    H, W = 16, 20
    K, pose = TREF.pinhole(H, W, 60.0), TB.sphere_view_poses(3, 400.0).astype(np.float32)[:1]
    tex = np.random.RandomState(0).rand(len(faces), 6, 3)
    face = RAST.rasterize(verts, faces, pose[0], K, H, W)["face"].reshape(1, H, W)
    ok = REF.shade(face, verts, faces, tex, pose, K, H, W)
    assert (ok[face >= 0] != 0).any() and (ok[face < 0] == 0).all()
    for bad in (-1, -5, len(faces), 1 << 30):
        assert (REF.shade(np.full_like(face, bad), verts, faces, tex, pose, K, H, W) == 0).all()
    behind = pose.copy()
    behind[0, 2, 3] = -400.0
    for P in (behind, pose * np.nan, pose * np.inf):
        assert (REF.shade(face, verts, faces, tex, P, K, H, W) == 0).all()
    f2 = faces.copy()
    f2[:, 1] = len(verts)
    assert (REF.shade(face, verts, f2, tex, pose, K, H, W) == 0).all()


# ---- bake round trip on the restatement: analytic-colour renders (3 mm period) of the sphere at 14 Fibonacci views, 96 x 96 at
# f = 300 (1.3 mm pixels at 400 mm: every node of every R below is seen), baked onto the nodes by texture_bake_ref.bake with the base
# mesh's depth planes, shaded at a held-out view by the restatement.  Measured PSNR over the covered pixels of the held-out view:
#   R = 1: 9.54 dB (today's vertex colours),  R = 4: 27.34 dB,  R = 8: 35.94 dB
MEASURED_PSNR = {1: 9.54, 4: 27.34, 8: 35.94}
_bake = {}


def analytic_view(verts, faces, pose, K, H, W):
    """the analytic colour at the true surface point of every pixel (from the depth plane), the depth and the face plane"""
    r = RAST.rasterize(verts, faces, pose, K, H, W)
    z = r["zbuf"].reshape(H, W)
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    pc = np.stack([jj, ii, np.ones_like(jj)], -1) @ np.linalg.inv(K.astype(np.float64)).T * z[..., None]
    P = pose.astype(np.float64)
    rgb = np.where((z > 0)[..., None], REF.fine_colour((pc - P[:, 3]) @ P[:, :3]), 0.0)
    return rgb.astype(np.float32), z.astype(np.float32), r["face"].reshape(H, W)


def bake_psnr(R):
    if not _bake:
        verts, faces = MESHES["sphere"]()
        H = W = 96
        K = TREF.pinhole(H, W, 300.0)
        poses = TB.sphere_view_poses(14, 400.0).astype(np.float32)
        views = [analytic_view(verts, faces, p, K, H, W) for p in poses]
        held = TB.sphere_view_poses(5, 400.0).astype(np.float32)[1]
        _bake.update(verts=verts, faces=faces, H=H, W=W, K=K, poses=poses, rgb=np.stack([v[0] for v in views]),
                     zbuf=np.stack([v[1] for v in views]), held=held, target=analytic_view(verts, faces, held, K, H, W), psnr={})
    c = _bake
    if R not in c["psnr"]:
        _, _, vs, fs, ni = subdivided("sphere", R)
        col, seen = TREF.vcolor_of(TREF.bake(vs, TB.vertex_normals(vs, fs), c["poses"], c["K"], c["rgb"], c["zbuf"])["acc"])
        assert seen.all()                                                   # every node is seen: no fill enters the figure
        hrgb, _, hface = c["target"]
        img = REF.shade(hface[None], c["verts"], c["faces"], FT.texels_from_nodes(col, ni), c["held"][None], c["K"], c["H"], c["W"])[0]
        c["psnr"][R] = 10 * np.log10(1.0 / ((img - hrgb.astype(np.float64))[hface >= 0] ** 2).mean())
    return c["psnr"][R]


def test_bake_round_trip_gains_detail():
    got = {R: bake_psnr(R) for R in (1, 4, 8)}
    print("bake round trip PSNR (dB):", {R: round(v, 2) for R, v in got.items()})
    for R, v in got.items():
        assert v >= MEASURED_PSNR[R] - 1.0, (R, v)
    assert got[4] - got[1] >= 0.5 * (MEASURED_PSNR[4] - MEASURED_PSNR[1])


def test_save_load_round_trip_and_foreign_mesh(tmp_path):
    verts, faces = TREF.torus(8, 5)
    tex = np.random.RandomState(1).rand(len(faces), FT.texel_count(4), 3).astype(np.float32)
    path = str(tmp_path / "t.texels.npz")
    FT.save_texels(path, tex, faces)
    got, R = FT.load_texels(path, faces)
    assert R == 4 and got.dtype == np.float32 and (got == tex).all()
    other = faces.copy()
    other[3] = other[3][[1, 2, 0]]                                          # the same triangle, another vertex order: other texels
    with pytest.raises(ValueError, match="another mesh"):
        FT.load_texels(path, other)
    with pytest.raises(ValueError, match="another mesh"):
        FT.load_texels(path, faces[:-1])
    with pytest.raises(ValueError):
        FT.save_texels(path, tex[:, :7], faces)                            # 7 is no T(R)
    with pytest.raises(ValueError):
        FT.save_texels(path, tex[:-1], faces)
    # the PLY for tools that only read PLY: the subdivided mesh with the texture as 8-bit vertex colours
    from texpose_amd.surfel import load_ply
    ply = str(tmp_path / "t.sub.ply")
    FT.write_subdivided_ply(ply, verts, faces, tex[:, :6])
    vs, fs, ni = FT.subdivide(verts, faces, 2)
    v, f, c = load_ply(ply)
    assert (v == vs).all() and (f == fs).all() and c.shape == (len(vs), 3)


def test_refinement_case_converges_on_the_cpu():
    """The start offset of the device refinement tests (tests/test_gpu_face_texels.py) is one from which photo_ref's loop with the
    restated shading converges; the figures that test adds its tolerance to are the ones measured here."""
    import pnp_ref as PREF
    c = REF.loop_inputs()
    want = REF.loop_ref(c)
    assert (want["status"] == 0).all() and (want["inliers"] > 500).all()
    for b in range(2):
        re0, te0 = PREF.pose_error(c["start"][b], c["P"][b])
        re, te = PREF.pose_error(want["pose"][b], c["P"][b])
        print("pose %d: start %.3f deg %.3f mm -> %.2e deg %.2e mm, rms %.4f -> %.6f" % (b, re0, te0, re, te, want["rms0"][b], want["rms"][b]))
        assert abs(re0 - REF.LOOP_ANGLE_DEG) < 1e-5 and 4.0 <= te0 <= 11.0
        assert re <= 1.05 * REF.LOOP_FINAL[b][0] and te <= 1.05 * REF.LOOP_FINAL[b][1]        # (as measured, to the digits written down)
