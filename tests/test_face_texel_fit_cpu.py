"""No GPU: the fp64 restatement of K36 (tests/face_texel_fit_ref.py) -- the adjoint identity, the 64-bit fixed-point scheme against
its bound, the library's refusals without a device, and the figures of the fit (the conjugate-gradient loop of FaceTexelFitter restated)
that the device tests take as their yardstick."""
import ctypes as C

import numpy as np
import pytest

import face_texel_fit_ref as FIT
import face_texels_ref as REF
import mesh_raster_ref as RAST
import test_face_texels_cpu as K35T                      # the round-trip case and its helpers, as they are
import texture_bake_ref as TREF
from texpose_amd import _lib
from texpose_amd import face_texels as FT
from texpose_amd import texture_bake as TB

H, W = 37, 53
FOCAL = {"sphere": 120.0, "torus": 150.0}
_case = {}


def case(name, R):
    """mesh, two poses, the brute-force face planes and the subdivision, once per key"""
    if name not in _case:
        verts, faces = K35T.MESHES[name]()
        K = TREF.pinhole(H, W, FOCAL[name])
        poses = TB.sphere_view_poses(5, 400.0).astype(np.float32)[1:3]
        face = np.stack([RAST.rasterize(verts, faces, p, K, H, W)["face"].reshape(H, W) for p in poses])
        _case[name] = dict(verts=verts, faces=faces, K=K, poses=poses, face=face)
    c = dict(_case[name])
    _, _, _, _, c["node_index"] = K35T.subdivided(name, R)
    c["U"] = int(c["node_index"].max()) + 1
    return c


def adjoint_args(c, R, per_node):
    return (c["face"], c["verts"], c["faces"]), (c["poses"], c["K"], H, W, R) + ((c["node_index"], c["U"]) if per_node else ())


@pytest.mark.parametrize("per_node", [False, True], ids=["slot", "node"])
@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_adjoint_identity_and_fixed_point_bound(name, R, per_node):
    c = case(name, R)
    rs = np.random.RandomState(R)
    head, tail = adjoint_args(c, R, per_node)
    F, T = len(c["faces"]), FT.texel_count(R)
    assert (c["face"] >= 0).sum() > 300
    # the cell restates K35's rule: by linearity S t = sum_k w_k t[slot_k] must equal the shading restatement
    slots, weights, valid = FIT.cell(c["face"], c["verts"], c["faces"], c["poses"], c["K"], H, W, R)
    assert (valid == (c["face"] >= 0)).all()
    values = rs.rand(c["U"], 3) if per_node else rs.rand(F, T, 3)
    texels = values[c["node_index"]] if per_node else values
    rows = np.where(valid, c["face"], 0)[..., None] * T + slots
    by_cell = (weights[..., None] * texels.reshape(-1, 3)[rows]).sum(-2)
    shaded = REF.shade(c["face"], c["verts"], c["faces"], texels, c["poses"], c["K"], H, W)
    assert np.abs(by_cell - shaded).max() <= 1e-14
    # <S t, g> = <t, S^T g>
    g = rs.randn(2, H, W, 3)
    want = FIT.shade_bwd(*head, g, *tail)
    lhs, rhs = (shaded * g).sum(), (values.reshape(-1, 3) * want["grad"]).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    assert want["count"].sum() == 3 * valid.sum() and np.allclose(want["weight"].sum(), valid.sum(), rtol=1e-12)
    # the fixed point stays within n_d gmax 2^-37 of the exact sum (+ the fp32 rounding of the result), at every gradient scale
    for scale in (1e-7, 1.0, 1e6):
        gs = (g * scale).astype(np.float32)
        exact, fixed = FIT.shade_bwd(*head, gs, *tail), FIT.shade_bwd_fixed(*head, gs, *tail)
        bound = exact["count"][:, None] * exact["gmax"] * 2.0 ** -37
        d = np.abs(fixed["grad"].astype(np.float64) - exact["grad"])
        print("%s R=%d %s scale %g: max error / bound %.3f" % (name, R, "node" if per_node else "slot", scale, (d / (bound + np.spacing(np.abs(exact["grad"]).astype(np.float32)))).max()))
        assert (d <= bound + np.spacing(np.abs(exact["grad"]).astype(np.float32))).all()
        dw = np.abs(fixed["weight"].astype(np.float64) - exact["weight"])
        assert (dw <= exact["count"] * 2.0 ** -37 + np.spacing(exact["weight"].astype(np.float32))).all()
    # pixels with a non-finite gradient drop out alone
    gs = g.astype(np.float32)
    gs[0, ::3, ::2, 1] = np.nan
    gs[1, 1::3, ::2, 2] = np.inf
    bad = ~np.isfinite(gs).all(-1)
    clean = np.where(bad[..., None], 0.0, gs)
    dropped, zeroed = FIT.shade_bwd(*head, gs, *tail), FIT.shade_bwd(*head, clean, *tail)
    assert np.isfinite(dropped["grad"]).all() and np.abs(dropped["grad"] - zeroed["grad"]).max() <= 1e-12
    assert dropped["count"].sum() == 3 * (valid & ~bad).sum()


def test_symbols_and_refusals_without_a_gpu():
    assert _lib.ABI_VERSION == 16
    assert "tp_face_texel_shade_bwd" in _lib.SYMBOLS and "tp_face_texel_shade_bwd_workspace" in _lib.SYMBOLS
    assert [f[0] for f in _lib.FaceTexelShadeBwdArgs._fields_] == ["verts", "faces", "pose", "intr", "face", "grad_rgb", "node_index", "B", "H", "W", "V",
                                                                   "F", "R", "U", "workspace", "grad", "weight"]
    lib = _lib.load()
    assert lib.tp_face_texel_shade_bwd_workspace(10, 0) == 8 * 31 and lib.tp_face_texel_shade_bwd_workspace(10, 1) == 8 * 41
    assert lib.tp_face_texel_shade_bwd_workspace(0, 0) == 0 and lib.tp_face_texel_shade_bwd_workspace(715827883, 0) == 0
    assert lib.tp_face_texel_shade_bwd(None, None) == -1 and b"tp_face_texel_shade_bwd: null args" in lib.tp_last_error()
    good = dict(B=1, H=8, W=8, V=3, F=1, R=1, U=0)

    def refused(text=b"bad sizes", **change):
        a = _lib.FaceTexelShadeBwdArgs()
        a.verts = a.faces = a.pose = a.intr = a.face = a.grad_rgb = a.workspace = a.grad = 64      # never dereferenced: every case is refused
        for k, v in {**good, **change}.items():
            setattr(a, k, v)
        return lib.tp_face_texel_shade_bwd(C.byref(a), None) == -1 and b"tp_face_texel_shade_bwd" in lib.tp_last_error() and text in lib.tp_last_error()

    for k in ("B", "H", "W", "V", "F", "R"):                        # everything K35 refuses
        assert refused(**{k: 0}) and refused(**{k: -1}), k
    assert refused(R=65) and refused(H=1 << 16, W=1 << 15) and refused(F=(1 << 31) // 2145 + 1, R=64)
    assert refused(B=1 << 30, H=64, W=64)
    assert refused(b"2^25", B=2, H=4096, W=4096 + 1) and refused(b"2^25", B=1 << 25, H=1, W=2)      # B H W > 2^25
    assert refused(b"U > 0", node_index=64, U=0) and refused(b"U > 0", node_index=64, U=-3)
    assert refused(b"3 N", F=300000000, R=1) and refused(b"3 N", node_index=64, U=715827883)        # 3 N >= 2^31
    assert refused(b"workspace", workspace=None) and refused(b"workspace", workspace=68)           # null, not 8-byte aligned
    for name in ("grad_rgb", "grad", "verts", "faces", "pose", "intr", "face"):
        assert refused(b"null pointer", **{name: None}), name


# ---- the fit on the restatement
_round = {}


def round_trip(R, size=96, focal=300.0):
    """The bake round trip of tests/test_face_texels_cpu.py (its helpers, its meshes, its views) at a given frame -> the stored views
    as FIT.Views with the default weights, the baked node colours and the held-out view."""
    if size not in _round:
        verts, faces = K35T.MESHES["sphere"]()
        K = TREF.pinhole(size, size, focal)
        poses = TB.sphere_view_poses(14, 400.0).astype(np.float32)
        views = [K35T.analytic_view(verts, faces, p, K, size, size) for p in poses]
        held = TB.sphere_view_poses(5, 400.0).astype(np.float32)[1]
        _round[size] = dict(verts=verts, faces=faces, K=K, poses=poses, held=held, rgb=np.stack([v[0] for v in views]), zbuf=np.stack([v[1] for v in views]),
                            face=np.stack([v[2] for v in views]), target=K35T.analytic_view(verts, faces, held, K, size, size), fits={})
    c = _round[size]
    if R not in c["fits"]:
        _, _, vs, fs, ni = K35T.subdivided("sphere", R)
        bake, seen = TREF.vcolor_of(TREF.bake(vs, TB.vertex_normals(vs, fs), c["poses"], c["K"], c["rgb"], c["zbuf"])["acc"])
        views = FIT.Views(c["face"], c["verts"], c["faces"], c["poses"], c["K"], size, size, R, ni, len(vs), c["rgb"],
                          FIT.inner_coverage(c["face"], len(c["faces"])))
        c["fits"][R] = dict(views=views, bake=bake, seen=seen, node_index=ni, U=len(vs))
    return c, c["fits"][R]


def held_out_psnr(c, node_index, nodes, size):
    hrgb, _, hface = c["target"]
    img = REF.shade(hface[None], c["verts"], c["faces"], nodes[node_index], c["held"][None], c["K"], size, size)[0]
    return FIT.psnr(img, hrgb, hface >= 0)


def measure_round_trip(R, size=96, focal=300.0, lam=0.1, iters=4):
    c, f = round_trip(R, size, focal)
    fit = FIT.fit_loop(f["views"], f["bake"], f["bake"], lam, iters)
    return (held_out_psnr(c, f["node_index"], f["bake"], size), held_out_psnr(c, f["node_index"], fit["nodes"], size), fit["rms"][0], fit["rms"][-1],
            int((fit["coverage"] < lam).sum()))


@pytest.mark.parametrize("R,size,focal,table", [(4, 96, 300.0, "ROUND_TRIP"), (8, 96, 300.0, "ROUND_TRIP"), (4, 64, 200.0, "ROUND_TRIP_SMALL")])
def test_round_trip_fit_gains_over_the_bake(R, size, focal, table):
    psnr_bake, psnr_fit, rms_bake, rms_fit, on_prior = measure_round_trip(R, size, focal)
    want = getattr(FIT, table)[R]
    print("round trip %dx%d R=%d: held-out PSNR bake %.2f dB, fit %.2f dB; training rms bake %.4f, fit %.4f; %d nodes on the prior | recorded %s"
          % (size, size, R, psnr_bake, psnr_fit, rms_bake, rms_fit, on_prior, want))
    if size == 96:
        assert abs(psnr_bake - K35T.MEASURED_PSNR[R]) <= 0.05            # the same case: the bake's figure is K35's
    assert psnr_fit >= want[1] - 1.0
    assert psnr_fit - psnr_bake >= 0.5 * (want[1] - want[0])
    assert rms_fit <= 1.02 * want[3] + 1e-5 and rms_fit < rms_bake


_consistent = {}


def consistent_system():
    """Photographs that ARE S x* for random node colours: sphere, 14 views, 64 x 64, f = 200, R = 2, every covered pixel weighted 1."""
    if not _consistent:
        size, R = 64, 2
        verts, faces = K35T.MESHES["sphere"]()
        K = TREF.pinhole(size, size, 200.0)
        poses = TB.sphere_view_poses(14, 400.0).astype(np.float32)
        face = np.stack([RAST.rasterize(verts, faces, p, K, size, size)["face"].reshape(size, size) for p in poses])
        _, _, vs, fs, ni = K35T.subdivided("sphere", R)
        truth = np.random.RandomState(11).rand(len(vs), 3)
        rgb = REF.shade(face, verts, faces, truth[ni], poses, K, size, size)
        _consistent.update(verts=verts, faces=faces, K=K, poses=poses, face=face, node_index=ni, U=len(vs), truth=truth, rgb=rgb, R=R, size=size,
                           views=FIT.Views(face, verts, faces, poses, K, size, size, R, ni, len(vs), rgb, face >= 0))
    return _consistent


def test_consistent_system_is_recovered():
    c = consistent_system()
    U = c["U"]
    errors = {}
    for dtype in (np.float64, np.float32):
        fit = FIT.fit_loop(c["views"], np.full((U, 3), 0.5), np.zeros((U, 3)), 1e-6, 32, dtype=dtype)
        seen = fit["coverage"] >= 1
        errors[dtype] = np.abs(fit["nodes"].astype(np.float64) - c["truth"])[seen].max()
        print("consistent system, %s vectors: max |x - x*| %.3e on %d of %d nodes; rms %.3e -> %.3e" % (dtype.__name__, errors[dtype], seen.sum(), U, fit["rms"][0], fit["rms"][-1]))
        assert seen.sum() >= 0.9 * U
    assert errors[np.float64] <= 1.05 * FIT.CONSISTENT_ERROR and FIT.CONSISTENT_ERROR <= 1e-3
    assert errors[np.float32] <= 1.05 * FIT.CONSISTENT_ERROR_FP32
    assert FIT.CONSISTENT_ERROR_FP32 <= 4 * FIT.CONSISTENT_ERROR + 1e-4           # the device test's bar holds for fp32 vectors on the CPU
