"""No GPU: the numpy restatement of K31 (tests/silhouette_ref.py) against independent facts and against the prototype's figures,
`silhouette.sdf_torch` and `silhouette.step_torch` against the restatement, and the host side of the entry points: the header-derived
binding and the argument checks, which launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import pnp_ref as PREF
import silhouette_ref as REF

# the prototype's table (numpy fp64, its own raster): (mesh, image) -> rim pixels, rms first and last, IoU first and last, deg, mm last
PROTOTYPE = {("bent sphere", 0): (86, 0.443, 0.000, 0.961, 1.000, 0.58, 0.22), ("bent sphere", 1): (81, 1.151, 0.046, 0.857, 0.998, 1.99, 1.82),
             ("bent torus", 0): (61, 0.474, 0.075, 0.925, 0.990, 0.71, 6.03), ("bent torus", 1): (88, 1.515, 0.000, 0.727, 0.998, 0.75, 0.40)}


# ----------------------------------------------------------------------------- the binding and the argument checks
def test_binding_has_the_new_entry_points():
    from texpose_amd import _lib
    for name in ("tp_mask_sdf_workspace_bytes", "tp_mask_sdf", "tp_silhouette_align_workspace_bytes", "tp_silhouette_align_step"):
        assert name in _lib.SYMBOLS
    for name in ("tp_mask_sdf_workspace_bytes", "tp_silhouette_align_workspace_bytes"):
        restype, argtypes = _lib.HEADER.prototypes[name]
        assert restype is C.c_size_t and argtypes == [C.c_int] * 3
    restype, argtypes = _lib.HEADER.prototypes["tp_mask_sdf"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    fields = ("zbuf", "pose", "intr", "sdf", "frame", "mask", "B", "Ft", "H", "W", "tau_px", "damping", "evaluate_only", "pose_out",
              "inliers", "rms", "status", "inter", "uni", "workspace")
    assert tuple(n for n, _ in _lib.SilhouetteAlignArgs._fields_) == fields
    assert C.sizeof(_lib.SilhouetteAlignArgs) == 6 * 8 + 4 * 4 + 2 * 4 + 4 + 4 + 7 * 8          # (4 bytes of padding before pose_out)
    lib = _lib.load()
    assert hasattr(lib, "tp_mask_sdf") and hasattr(lib, "tp_silhouette_align_step")
    assert lib.tp_abi_version() == _lib.ABI_VERSION               # (the declarations add to the ABI and change nothing in it)


def test_workspace_bytes():
    from texpose_amd import _lib
    ws = _lib.load().tp_silhouette_align_workspace_bytes
    for B, H, W in ((1, 1, 1), (3, 33, 257), (64, 480, 640), (2, 32, 32), (2, 1, 1025)):
        want = 256 * B * -(-H * W // 1024)
        assert ws(B, H, W) == (want + 15) // 16 * 16
    assert ws(0, 5, 5) == 0 and ws(5, 0, 5) == 0 and ws(5, 5, -1) == 0
    ws = _lib.load().tp_mask_sdf_workspace_bytes
    for F, H, W in ((1, 1, 1), (3, 33, 257), (64, 480, 640), (1, 5, 1030), (1, 8192, 8192)):
        assert ws(F, H, W) == (4 * F * H * W + 15) // 16 * 16
    assert ws(0, 5, 5) == 0 and ws(5, 0, 5) == 0 and ws(5, 5, -1) == 0


def _aligned_buffer(n):
    buf = C.create_string_buffer(n + 16)
    return buf, C.addressof(buf) + (-C.addressof(buf)) % 16


def test_sdf_argument_errors_launch_nothing():
    """Every pointer is a host buffer: a launch would fault, a refusal returns before anything reads them."""
    from texpose_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer(8192)
    err = lambda: lib.tp_last_error()
    mask, sdf, ws = p, p + 1024, p + 4096
    for F, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 8193, 4), (1, 4, 8193), (32, 8192, 8192), (2 ** 20, 64, 32)):
        assert lib.tp_mask_sdf(mask, sdf, F, H, W, ws, None) == -1 and b"bad sizes" in err(), (F, H, W)
    for args in ((None, sdf, ws), (mask, None, ws), (mask, sdf, None)):
        assert lib.tp_mask_sdf(args[0], args[1], 2, 4, 4, args[2], None) == -1 and b"null pointer" in err()
    assert lib.tp_mask_sdf(mask, sdf, 2, 4, 4, ws + 8, None) == -1 and b"aligned" in err()
    for m, s in ((p, p), (p + 16, p), (p, p + 31), (p + 127, p)):          # mask 32 bytes, sdf 128 bytes
        assert lib.tp_mask_sdf(m, s, 2, 4, 4, ws, None) == -1 and b"overlap" in err(), (m - p, s - p)


def test_step_argument_errors_launch_nothing():
    from texpose_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer(8192)
    good = dict(B=2, Ft=2, H=4, W=4, tau_px=4.0, damping=1e-6, evaluate_only=0)

    def filled(**kw):
        a = _lib.SilhouetteAlignArgs()
        for k, (name, t) in enumerate(_lib.SilhouetteAlignArgs._fields_):
            if t is C.c_void_p:
                setattr(a, name, p + 256 * k)
        for k, v in {**good, **kw}.items():
            setattr(a, k, v)
        return a

    err = lambda: lib.tp_last_error()
    call = lambda a: lib.tp_silhouette_align_step(C.byref(a), None)
    assert lib.tp_silhouette_align_step(None, None) == -1 and b"null args" in err()
    for bad in (dict(B=0), dict(B=65536), dict(H=0), dict(W=-1), dict(Ft=0), dict(H=65536, W=32768)):
        assert call(filled(**bad)) == -1 and b"bad sizes" in err(), bad
    assert call(filled(Ft=3, frame=None)) == -1 and b"frame map" in err()
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert call(filled(tau_px=tau)) == -1 and b"tau_px" in err(), tau
    for damping in (-1e-3, float("nan"), float("inf")):
        assert call(filled(damping=damping)) == -1 and b"damping" in err(), damping
    for name in ("zbuf", "pose", "intr", "sdf", "pose_out", "inliers", "rms", "status", "inter", "uni", "workspace"):
        assert call(filled(**{name: None})) == -1 and b"null pointer" in err(), name
    assert call(filled(workspace=p + 8)) == -1 and b"aligned" in err()
    a = filled()
    a.pose_out = a.pose
    assert call(a) == -1 and b"overlap" in err()
    a.pose_out = a.pose + 48                                     # the second pose of the input
    assert call(a) == -1 and b"overlap" in err()


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from texpose_amd import _lib, ops, silhouette
    verts, faces = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    z, pose, K, sdf = torch.zeros(1, 4, 4), torch.zeros(1, 3, 4), torch.eye(3), torch.zeros(1, 4, 4)
    for call in (lambda: ops.silhouette_align_step(z, pose, K, sdf, tau_px=4.0), lambda: ops.silhouette_align(verts, faces, pose, K, sdf),
                 lambda: ops.mask_sdf(torch.zeros(1, 4, 4, dtype=torch.uint8))):
        with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
            call()
    with pytest.raises(_lib.TexposeLibraryError):
        silhouette.SilhouetteRefiner(verts, faces, 4, 4, "cpu")
    with pytest.raises(ValueError, match="iters"):
        ops.silhouette_align(verts, faces, pose, K, sdf, iters=-1)
    with pytest.raises(ValueError, match="tau_px"):
        ops.silhouette_align(verts, faces, pose, K, sdf, iters=2, tau_px=[6.0, 4.0])


# ----------------------------------------------------------------------------- the distance field
def test_sdf_ref_on_cases_done_by_hand():
    m = np.zeros((3, 5), np.uint8)
    m[1, 1] = 7
    to_set, to_clear = REF.d2_ref(m)
    assert to_set.tolist() == [[2, 1, 2, 5, 10], [1, 0, 1, 4, 9], [2, 1, 2, 5, 10]]
    assert to_clear[1, 1] == 1 and (np.delete(to_clear.reshape(-1), 6) == 0).all()
    s = REF.sdf_ref(m)
    assert s[1, 1] == -0.5 and s[1, 2] == 0.5 and s[1, 3] == 1.5 and s[0, 0] == np.float32(np.sqrt(np.float32(2.0))) - np.float32(0.5)
    assert s.dtype == np.float32


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (2, 5), (9, 13)])
def test_sdf_torch_equals_the_restatement(H, W):
    from texpose_amd import silhouette
    rs = np.random.RandomState(H * 100 + W)
    masks = np.stack([rs.uniform(size=(H, W)) < 0.5, rs.uniform(size=(H, W)) < 0.1, np.zeros((H, W), bool), np.ones((H, W), bool)])
    masks = masks.astype(np.uint8) * np.uint8(255)
    want = REF.sdf_ref(masks)
    got = silhouette.sdf_torch(torch.from_numpy(masks)).numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want)
    none = np.float32(np.sqrt(np.float32(H * H + W * W))) - np.float32(0.5)          # an empty and a full plane: the sentinel
    assert (want[2] == none).all() and (want[3] == -none).all() and np.isfinite(want).all()
    assert np.array_equal(want < 0, masks != 0)
    assert np.array_equal(silhouette.sdf_torch(torch.from_numpy(masks[0])).numpy(), want[0])          # one [H,W] plane


# ----------------------------------------------------------------------------- step_torch
def torch_step(c, **kw):
    from texpose_amd import silhouette
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x))
    return silhouette.step_torch(t(c["zbuf"]), t(c["pose"]), t(c["K"]), t(c["sdf"]), c["tau"], 1e-6, t(c["frame"]), t(c["mask"]), **kw)


def ref_step(c, **kw):
    return REF.step_ref(c["zbuf"], c["pose"], c["K"], c["sdf"], c["tau"], 1e-6, c["frame"], c["mask"], **kw)


@pytest.mark.parametrize("frames,with_mask,evaluate_only,field", [("one", False, False, "shifted"), ("each", True, False, "random"),
                                                                  ("map", False, True, "random"), ("map", True, False, "shifted")])
def test_step_torch_equals_the_restatement(frames, with_mask, evaluate_only, field):
    """Planted NaN / Inf in zbuf and (the random field) in sdf, a mask and a frame map whose entries clamp."""
    c = REF.one_step_case(5, 3, 33, 65, frames, with_mask, field)
    want, got = ref_step(c, evaluate_only=evaluate_only), torch_step(c, evaluate_only=evaluate_only)
    assert not np.isfinite(c["zbuf"]).all() and (field == "shifted" or not np.isfinite(c["sdf"]).all())
    rims = sum(int(REF.rim_ref(z).sum()) for z in c["zbuf"])
    assert 30 < want["inliers"].sum() < rims                      # (tau, the mask or a bad value dropped some)
    assert got["inliers"].dtype == torch.int32 and np.array_equal(got["inliers"].numpy(), want["inliers"])
    assert np.array_equal(got["status"].numpy(), want["status"])
    assert got["inter"].dtype == torch.int32 and np.array_equal(got["inter"].numpy(), want["inter"]) and np.array_equal(got["uni"].numpy(), want["uni"])
    assert (want["uni"] > want["inter"]).all() and want["inter"].max() > 100          # (a shared plane is the last image's)
    rms = got["rms"].numpy().astype(np.float64)
    assert np.array_equal(np.isnan(rms), np.isnan(want["rms"]))
    np.testing.assert_allclose(rms[~np.isnan(rms)], want["rms"][~np.isnan(rms)], rtol=1e-6)
    stepped = (want["status"] == 0) & (not evaluate_only)
    assert evaluate_only or stepped.any()
    for b in range(3):
        if not stepped[b]:
            assert np.array_equal(got["pose"].numpy()[b], c["pose"][b]) and np.array_equal(want["pose"][b], c["pose"][b])
        else:
            assert np.abs(got["pose"].numpy()[b, :, :3] - want["pose"][b, :, :3]).max() <= 1e-6
            np.testing.assert_allclose(got["pose"].numpy()[b, :, 3], want["pose"][b, :, 3], rtol=1e-6)
            assert np.abs(want["pose"][b] - c["pose"][b]).max() > 1e-4          # (a step was taken)


def test_an_image_without_interior_keeps_nothing():
    c = REF.one_step_case(2, 2, 2, 5, "each", False)
    c["zbuf"][:] = 900.0
    c["zbuf"][:, 0, 0] = -1.0
    for r in (ref_step(c), torch_step(c)):
        assert np.asarray(r["inliers"]).tolist() == [0, 0] and np.asarray(r["status"]).tolist() == [1, 1]
        assert np.isnan(np.asarray(r["rms"])).all() and np.array_equal(np.asarray(r["pose"]), c["pose"])
        assert (np.asarray(r["uni"]) >= 9).all()                  # (the counts run over the border too)


# ----------------------------------------------------------------------------- anchors that need no library
@pytest.mark.parametrize("name", REF.MESHES)
def test_the_renderings_own_coverage_as_the_mask_has_no_residual(name):
    c = REF.loop_inputs(name)
    zbuf = np.stack([REF.render_ref(name, c["P"][b], c["K"][b], c["H"], c["W"]) for b in range(2)])
    rims = np.array([REF.rim_ref(z).sum() for z in zbuf])
    case = dict(zbuf=zbuf, pose=c["P"], K=c["K"], sdf=c["sdf"], frame=None, mask=None, tau=4.0)
    for r in (ref_step(case, evaluate_only=True), torch_step(case, evaluate_only=True)):
        assert np.array_equal(np.asarray(r["inliers"]), rims) and (rims > 50).all()
        assert (np.asarray(r["rms"]) == 0).all() and np.array_equal(np.asarray(r["inter"]), np.asarray(r["uni"]))
        assert np.array_equal(np.asarray(r["inter"]), (zbuf > 0).reshape(2, -1).sum(1))
        assert np.asarray(r["status"]).tolist() == [0, 0]


@pytest.mark.parametrize("name", REF.MESHES)
def test_loop_reproduces_the_prototype(name):
    """From 3 deg and 6 .. 8 mm on the bent (asymmetric) meshes: status 0, the last rms at most a quarter of the first (the
    prototype's worst ratio is 0.158), IoU does not fall and ends >= 0.97 (worst 0.990), the rotation error falls (worst 1.99 deg from
    3).  Translation is printed, not asserted: at a 30-pixel radius the outline barely sees depth."""
    c = REF.loop_case(name)
    w = c["want"]
    assert (w["status"] == 0).all()
    for b in range(2):
        re0, te0 = PREF.pose_error(c["start"][b], c["P"][b])
        re, te = PREF.pose_error(w["pose"][b], c["P"][b])
        print("%s %d: %d rim pixels, rms %.3f -> %.3f px, IoU %.3f -> %.3f, %.2f -> %.2f deg, %.2f -> %.2f mm"
              % (name, b, w["inliers0"][b], w["rms0"][b], w["rms"][b], w["iou0"][b], w["iou"][b], re0, re, te0, te))
        assert 2.9 < re0 < 3.1 and 6.0 < te0 < 8.2
        assert w["rms"][b] <= 0.25 * w["rms0"][b]
        assert w["iou"][b] >= w["iou0"][b] and w["iou"][b] >= 0.97
        assert re < re0
        rim, rms0_p, rms_p, iou0_p, iou_p, re_p, te_p = PROTOTYPE[name, b]
        assert w["inliers0"][b] == rim
        assert abs(w["rms0"][b] - rms0_p) <= 1e-3 and abs(w["rms"][b] - rms_p) <= 1e-3 and abs(w["iou0"][b] - iou0_p) <= 1e-3
        assert abs(w["iou"][b] - iou_p) <= 1e-3 and abs(re - re_p) <= 1e-2 and abs(te - te_p) <= 1e-2
