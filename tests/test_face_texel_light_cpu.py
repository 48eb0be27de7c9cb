"""K41 (tp_face_texel_light) and the lit fit without a GPU: the restatement's operator identity, the alternation on the relit round trip
against the recorded figures, the consistent system, and the library's symbols, struct fields and refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import face_texel_fit_ref as FIT
import face_texel_light_ref as LT
import face_texels_ref as REF
import test_face_texel_fit_cpu as K36T                  # the round trip and the consistent system, as they are
import test_face_texels_cpu as K35T
import texture_bake_ref as TREF
from texpose_amd import _lib
from texpose_amd import texture_bake as TB

SIZE, R = 64, 4


# ---- the relit round trip
@functools.lru_cache(maxsize=None)
def relit_case(name):
    """Section 26's shrunk round trip with every photograph relit by its own light -> the views (plain and as planes), the bake of the
    relit photographs, and the held-out truth."""
    strength, sigma = LT.CASES[name]
    c, f = K36T.round_trip(R, SIZE, 200.0)
    lights = LT.view_lights(len(c["poses"]), strength)
    rgb = LT.relight(c["verts"], c["faces"], c["face"], c["poses"], c["rgb"], lights, sigma)
    _, _, vs, fs, ni = K35T.subdivided("sphere", R)
    bake, _ = TREF.vcolor_of(TREF.bake(vs, TB.vertex_normals(vs, fs), c["poses"], c["K"], rgb, c["zbuf"])["acc"])
    weight = FIT.inner_coverage(c["face"], len(c["faces"]))
    views = FIT.Views(c["face"], c["verts"], c["faces"], c["poses"], c["K"], SIZE, SIZE, R, ni, len(vs), rgb, weight)
    planes = dict(verts=c["verts"], faces=c["faces"], face=c["face"], pose=c["poses"], rgb=rgb, weight=weight.astype(np.float32))
    return dict(c=c, views=views, planes=planes, bake=bake, node_index=ni, U=len(vs), lights=lights, rgb=rgb)


def held_out(case, nodes):
    c = case["c"]
    hrgb, _, hface = c["target"]
    img = REF.shade(hface[None], c["verts"], c["faces"], np.asarray(nodes, np.float64)[case["node_index"]], c["held"][None], c["K"], SIZE, SIZE)[0]
    return LT.affine_psnr(img, hrgb, hface >= 0)


@functools.lru_cache(maxsize=None)
def measure(name):
    case = relit_case(name)
    plain = FIT.fit_loop(case["views"], case["bake"], case["bake"], LT.LAM, LT.ITERS)
    lit = LT.lit_fit_loop(case["views"], case["planes"], case["bake"], case["bake"], LT.LAM, LT.ITERS, LT.ROUNDS)
    return dict(plain=plain, lit=lit, figures=(plain["rms"][-1], lit["rms"][-1], held_out(case, plain["nodes"]), held_out(case, lit["nodes"])))


@pytest.mark.parametrize("name", list(LT.CASES))
def test_lit_fit_beats_the_plain_fit_on_relit_photographs(name):
    m = measure(name)
    rms_plain, rms_lit, psnr_plain, psnr_lit = m["figures"]
    want = LT.RELIT[name]
    print("relit round trip %s: training rms plain %.4f (from %.4f), lit %.4f (from %.4f); held-out gauge-free PSNR plain %.2f dB, lit %.2f dB; "
          "status %s gain %s | recorded %s" % (name, rms_plain, m["plain"]["rms"][0], rms_lit, m["lit"]["rms"][0], psnr_plain, psnr_lit,
                                               m["lit"]["status"].tolist(), np.round(m["lit"]["gain"], 3).tolist(), want))
    print("  lit rms series:", np.round(m["lit"]["rms"], 5).tolist())
    assert psnr_lit >= want[3] - 1.0
    assert rms_lit <= 1.02 * want[1]
    assert want[3] > want[2] and psnr_lit - psnr_plain >= 0.5 * (want[3] - want[2])
    ends = m["lit"]["rms"][::LT.ITERS]                               # the start and the end of every round
    assert len(m["lit"]["rms"]) == LT.ROUNDS * LT.ITERS + 1 and (np.diff(ends) <= 1e-6).all(), ends
    g = dict(np.load(LT.GOLDEN))
    np.testing.assert_allclose(g[name], want, rtol=0, atol=1e-12)    # the file and the table say the same


# ---- the operator
def test_operator_identity():
    """<D S t, u> = <t, S^T D u> with D = m s^2 of the case's true lights, and K41's restatement is that D on the planes."""
    case = relit_case("clean")
    views, pl = case["views"], case["planes"]
    valid = views.valid
    s = np.stack([LT.shading_ref(pl["verts"], pl["faces"], pl["face"][b], pl["pose"][b], case["lights"][b]) for b in range(len(valid))])[valid]
    D = views.m[:, None] * s.astype(np.float64) ** 2
    rs = np.random.RandomState(3)
    t, u = rs.normal(size=(case["U"], 3)), rs.normal(size=(valid.sum(), 3))
    lhs, rhs = (D * views.shade(t) * u).sum(), (t * views.adjoint(D * u)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    colour = np.zeros(valid.shape + (3,), np.float32)
    colour[valid] = views.shade(t).astype(np.float32)
    out = LT.light_ref(pl["verts"], pl["faces"], pl["face"], pl["pose"], case["lights"], colour, None, pl["weight"])
    np.testing.assert_allclose(out["grad"][valid], D * colour[valid], rtol=4e-7, atol=0)            # three fp32 roundings
    np.testing.assert_allclose(out["diag"][valid], D, rtol=3e-7, atol=0)
    assert not out["grad"][~out["on"]].any() and not out["diag"][~out["on"]].any()


def test_residual_mode_is_the_applied_rendering():
    """p of the residual mode is photo_lighting_ref.apply_ref bit for bit, and sums are the weighted residual."""
    case = relit_case("clean")
    pl = case["planes"]
    F = len(pl["faces"])
    rs = np.random.RandomState(5)
    colour = rs.rand(*pl["rgb"].shape).astype(np.float32)
    out = LT.light_ref(pl["verts"], pl["faces"], pl["face"], pl["pose"], case["lights"], colour, pl["rgb"], None)
    for b in (0, 7):
        zbuf = np.where((pl["face"][b] >= 0) & (pl["face"][b] < F), 1.0, -1.0).astype(np.float32)
        P = LT.LREF.apply_ref(pl["verts"], pl["faces"], pl["face"][b], zbuf, colour[b], pl["pose"][b], case["lights"][b])
        s = LT.shading_ref(pl["verts"], pl["faces"], pl["face"][b], pl["pose"][b], case["lights"][b])
        want = np.where((zbuf > 0)[..., None], s * (pl["rgb"][b] - P), 0.0).astype(np.float32)
        assert np.array_equal(out["grad"][b], want)
        e = (pl["rgb"][b] - P).astype(np.float64)[zbuf > 0]
        assert abs(out["sums"][b, 0] - (e * e).sum()) <= 1e-12 * (e * e).sum() and out["sums"][b, 1] == (zbuf > 0).sum()


# ---- the consistent system
@functools.lru_cache(maxsize=None)
def lit_consistent_system():
    """Section 26's consistent system with the photographs relit through the restatement's own apply under view_lights."""
    c = K36T.consistent_system()
    lights = LT.view_lights(len(c["poses"]))
    rgb = LT.relight(c["verts"], c["faces"], c["face"], c["poses"], c["rgb"].astype(np.float32), lights)
    weight = (c["face"] >= 0).astype(np.float32)
    views = FIT.Views(c["face"], c["verts"], c["faces"], c["poses"], c["K"], c["size"], c["size"], c["R"], c["node_index"], c["U"], rgb, weight)
    planes = dict(verts=c["verts"], faces=c["faces"], face=c["face"], pose=c["poses"], rgb=rgb, weight=weight)
    return dict(c=c, views=views, planes=planes, lights=lights, rgb=rgb)


def test_consistent_system_is_recovered_under_the_true_lights():
    s = lit_consistent_system()
    c, U = s["c"], s["c"]["U"]
    errors = {}
    for dtype in (np.float64, np.float32):
        fit = LT.lit_fit_loop(s["views"], s["planes"], np.full((U, 3), 0.5), np.zeros((U, 3)), 1e-6, 32, 1, lights=s["lights"], light_step=False,
                              dtype=dtype)
        seen = fit["coverage"] >= 1
        errors[dtype] = np.abs(fit["nodes"].astype(np.float64) - c["truth"])[seen].max()
        print("lit consistent system, %s vectors: max |x - x*| %.3e on %d of %d nodes; rms %.3e -> %.3e"
              % (dtype.__name__, errors[dtype], seen.sum(), U, fit["rms"][0], fit["rms"][-1]))
        assert seen.sum() >= 0.9 * U
    assert errors[np.float64] <= 1.05 * LT.CONSISTENT_ERROR and LT.CONSISTENT_ERROR <= 1e-3
    assert errors[np.float32] <= 1.05 * LT.CONSISTENT_ERROR_FP32
    assert LT.CONSISTENT_ERROR_FP32 <= 4 * LT.CONSISTENT_ERROR + 1e-4              # the device test's bar holds for fp32 vectors on the CPU


# ---- the library without a device
def test_symbols_and_refusals_without_a_gpu():
    assert _lib.ABI_VERSION == 16
    assert "tp_face_texel_light" in _lib.SYMBOLS and "tp_face_texel_light_workspace_bytes" in _lib.SYMBOLS
    assert [f[0] for f in _lib.FaceTexelLightArgs._fields_] == ["verts", "faces", "face", "pose", "light", "colour", "image", "weight", "V", "F", "B", "H",
                                                                "W", "grad", "diag", "sums", "workspace"]
    lib = _lib.load()
    assert lib.tp_face_texel_light_workspace_bytes(3, 33, 257) == 16 * 3 * 9 and lib.tp_face_texel_light_workspace_bytes(1, 1, 1) == 16
    assert lib.tp_face_texel_light_workspace_bytes(0, 4, 4) == 0 and lib.tp_face_texel_light_workspace_bytes(1, -1, 4) == 0
    assert lib.tp_face_texel_light(None, None) == -1 and b"tp_face_texel_light: null args" in lib.tp_last_error()
    # addresses that are never dereferenced (every case is refused), 1 MiB apart so that nothing overlaps by accident
    names = ("verts", "faces", "face", "pose", "light", "colour", "image", "weight", "grad", "diag", "sums", "workspace")
    good = dict({n: (i + 1) << 20 for i, n in enumerate(names)}, V=3, F=1, B=2, H=8, W=8)

    def refused(text, **change):
        a = _lib.FaceTexelLightArgs()
        for k, v in {**good, **change}.items():
            setattr(a, k, v)
        return lib.tp_face_texel_light(C.byref(a), None) == -1 and b"tp_face_texel_light" in lib.tp_last_error() and text in lib.tp_last_error()

    for k in ("V", "F", "B", "H", "W"):
        assert refused(b"bad sizes", **{k: 0}) and refused(b"bad sizes", **{k: -1}), k
    assert refused(b"bad sizes", B=65536) and refused(b"bad sizes", H=1 << 16, W=1 << 15)
    for k in ("verts", "faces", "face", "pose", "light", "colour", "grad"):
        assert refused(b"null pointer", **{k: None}), k
    assert refused(b"sums need image", image=None)
    assert refused(b"sums need a workspace", workspace=None) and refused(b"8-byte aligned", workspace=good["workspace"] + 4)
    planes, px = 2 * 8 * 8 * 12, 2 * 8 * 8 * 4
    for out, size in (("grad", planes), ("diag", planes), ("sums", 32), ("workspace", 32)):
        for inp, isize in (("verts", 36), ("faces", 12), ("face", px), ("pose", 96), ("light", 120), ("colour", planes), ("image", planes), ("weight", px)):
            last = good[inp] + isize - 4                          # the input's last word; the doubles start on the input itself
            assert refused(b"overlaps", **{out: last if out in ("grad", "diag") else good[inp]}), (out, inp)
            assert refused(b"overlaps", **{out: good[inp] - size + 8}), (out, inp)
    assert refused(b"overlaps", diag=good["grad"] + planes - 4) and refused(b"overlaps", sums=good["grad"] + 8)
    assert refused(b"overlaps", workspace=good["diag"]) and refused(b"overlaps", workspace=good["sums"] + 8)
