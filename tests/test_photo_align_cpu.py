"""No GPU: the numpy restatement of K30 (tests/photo_ref.py) against independent facts and against the prototype's figures,
`photo_align.step_torch` against the restatement, and the host side of the entry points: the header-derived binding and the argument
checks, which launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import photo_ref as REF
import pnp_ref as PREF

# the prototype's table (numpy fp64, its own raster): (mesh, image) -> kept pixels, clean end (deg, mm), clean rms first and last
PROTOTYPE = {("sphere", 0): (827, 0.0008, 0.001, 0.109, 0.0001), ("sphere", 1): (851, 0.0001, 0.0001, 0.323, 0.0000),
             ("torus", 0): (403, 0.037, 0.027, 0.149, 0.003), ("torus", 1): (727, 0.0000, 0.0001, 0.319, 0.0000)}


# ----------------------------------------------------------------------------- the binding and the argument checks
def test_binding_has_the_new_entry_points():
    from texpose_amd import _lib
    for name in ("tp_photo_align_workspace_bytes", "tp_photo_align_step"):
        assert name in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 16
    restype, argtypes = _lib.HEADER.prototypes["tp_photo_align_workspace_bytes"]
    assert restype is C.c_size_t and argtypes == [C.c_int] * 3
    fields = ("zbuf", "rgb", "pose", "intr", "image", "frame", "mask", "B", "Ft", "H", "W", "tau", "damping", "evaluate_only", "pose_out",
              "inliers", "rms", "status", "workspace")
    assert tuple(n for n, _ in _lib.PhotoAlignArgs._fields_) == fields
    assert C.sizeof(_lib.PhotoAlignArgs) == 7 * 8 + 4 * 4 + 2 * 4 + 4 + 4 + 5 * 8          # (4 bytes of padding before pose_out)
    lib = _lib.load()
    assert hasattr(lib, "tp_photo_align_step")


def test_workspace_bytes():
    from texpose_amd import _lib
    ws = _lib.load().tp_photo_align_workspace_bytes
    for B, H, W in ((1, 1, 1), (3, 33, 257), (64, 480, 640), (2, 32, 32), (2, 1, 1025)):
        want = 256 * B * -(-H * W // 1024)
        assert ws(B, H, W) == (want + 15) // 16 * 16
    assert ws(0, 5, 5) == 0 and ws(5, 0, 5) == 0 and ws(5, 5, -1) == 0


def test_argument_errors_launch_nothing():
    """Every pointer is a host buffer: a launch would fault, a refusal returns before anything reads them."""
    from texpose_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(8192)
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    good = dict(B=2, Ft=2, H=4, W=4, tau=0.5, damping=1e-6, evaluate_only=0)

    def filled(**kw):
        a = _lib.PhotoAlignArgs()
        for k, (name, t) in enumerate(_lib.PhotoAlignArgs._fields_):
            if t is C.c_void_p:
                setattr(a, name, p + 256 * k)
        for k, v in {**good, **kw}.items():
            setattr(a, k, v)
        return a

    err = lambda: lib.tp_last_error()
    call = lambda a: lib.tp_photo_align_step(C.byref(a), None)
    assert lib.tp_photo_align_step(None, None) == -1 and b"null args" in err()
    for bad in (dict(B=0), dict(B=65536), dict(H=0), dict(W=-1), dict(Ft=0), dict(H=65536, W=32768)):
        assert call(filled(**bad)) == -1 and b"bad sizes" in err(), bad
    assert call(filled(Ft=3, frame=None)) == -1 and b"frame map" in err()
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert call(filled(tau=tau)) == -1 and b"tau" in err(), tau
    for damping in (-1e-3, float("nan"), float("inf")):
        assert call(filled(damping=damping)) == -1 and b"damping" in err(), damping
    for name in ("zbuf", "rgb", "pose", "intr", "image", "pose_out", "inliers", "rms", "status", "workspace"):
        assert call(filled(**{name: None})) == -1 and b"null pointer" in err(), name
    assert call(filled(workspace=p + 8)) == -1 and b"aligned" in err()
    a = filled()
    a.pose_out = a.pose
    assert call(a) == -1 and b"overlap" in err()
    a.pose_out = a.pose + 48                                     # the second pose of the input
    assert call(a) == -1 and b"overlap" in err()


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from texpose_amd import _lib, ops, photo_align
    verts, faces, vcolor = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    z, c, pose, K, im = torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, 3), torch.zeros(1, 3, 4), torch.eye(3), torch.zeros(1, 4, 4, 3)
    for call in (lambda: ops.photo_align_step(z, c, pose, K, im, tau=0.5), lambda: ops.photo_align(verts, faces, vcolor, pose, K, im)):
        with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
            call()
    with pytest.raises(_lib.TexposeLibraryError):
        photo_align.PhotoRefiner(verts, faces, vcolor, 4, 4, "cpu")
    with pytest.raises(ValueError, match="iters"):
        ops.photo_align(verts, faces, vcolor, pose, K, im, iters=-1)
    with pytest.raises(ValueError, match="tau"):
        ops.photo_align(verts, faces, vcolor, pose, K, im, iters=2, tau=[0.6, 0.5])


# ----------------------------------------------------------------------------- step_torch
def torch_step(c, **kw):
    from texpose_amd import photo_align
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x))
    return photo_align.step_torch(t(c["zbuf"]), t(c["rgb"]), t(c["pose"]), t(c["K"]), t(c["image"]), c["tau"], 1e-6, t(c["frame"]), t(c["mask"]), **kw)


def ref_step(c, **kw):
    return REF.step_ref(c["zbuf"], c["rgb"], c["pose"], c["K"], c["image"], c["tau"], 1e-6, c["frame"], c["mask"], **kw)


@pytest.mark.parametrize("frames,with_mask,evaluate_only", [("one", False, False), ("each", True, False), ("map", False, True), ("map", True, False)])
def test_step_torch_equals_the_restatement(frames, with_mask, evaluate_only):
    """Planted NaN / Inf in every plane, a mask and a frame map whose entries clamp."""
    c = REF.one_step_case(5, 3, 16, 65, frames, with_mask)
    want, got = ref_step(c, evaluate_only=evaluate_only), torch_step(c, evaluate_only=evaluate_only)
    assert not np.isfinite(c["zbuf"]).all() and not np.isfinite(c["rgb"]).all() and not np.isfinite(c["image"]).all()
    assert (want["near_ties"] == 0).all() and want["inliers"].sum() > 100
    assert got["inliers"].dtype == torch.int32 and np.array_equal(got["inliers"].numpy(), want["inliers"])
    assert np.array_equal(got["status"].numpy(), want["status"])
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
    c["rgb"][:] = c["image"][:] = 0.25
    for r in (ref_step(c), torch_step(c)):
        assert np.asarray(r["inliers"]).tolist() == [0, 0] and np.asarray(r["status"]).tolist() == [1, 1]
        assert np.isnan(np.asarray(r["rms"])).all() and np.array_equal(np.asarray(r["pose"]), c["pose"])


# ----------------------------------------------------------------------------- anchors that need no library
@pytest.fixture(scope="module")
def sphere():
    c = REF.loop_inputs("sphere", False)
    planes = [REF.render_ref(c["verts"], c["faces"], c["vcolor"], c["P"][b], c["K"][b], c["H"], c["W"]) for b in range(2)]
    return dict(c, zbuf=np.stack([p[0] for p in planes]), rgb=np.stack([p[1] for p in planes]))


def test_render_at_its_own_pose_has_no_residual(sphere):
    s = sphere
    r = REF.step_ref(s["zbuf"], s["rgb"], s["P"], s["K"], s["rgb"], 0.5, evaluate_only=True)
    covered = (s["zbuf"][:, 1:-1, 1:-1] > 0).reshape(2, -1).sum(1)
    assert np.array_equal(r["inliers"], covered) and (covered > 500).all()
    assert (r["rms"] == 0).all() and np.array_equal(r["pose"], s["P"])
    got = torch_step(dict(s, pose=s["P"], image=s["rgb"], frame=None, mask=None, tau=0.5), evaluate_only=True)
    assert np.array_equal(got["inliers"].numpy(), covered) and (got["rms"].numpy() == 0).all()


def test_a_constant_image_has_no_gradient_and_fails_the_pivot_rule(sphere):
    s = sphere
    image = np.full_like(s["rgb"], 0.5)
    c = dict(s, pose=s["P"], image=image, frame=None, mask=None, tau=2.0)
    for r in (ref_step(c), torch_step(c)):
        assert (np.asarray(r["inliers"]) > 500).all() and np.asarray(r["status"]).tolist() == [3, 3]
        assert np.array_equal(np.asarray(r["pose"]).view(np.uint32), s["P"].view(np.uint32))
        assert (np.asarray(r["rms"]) > 0).all()


def test_the_count_is_per_pixel_and_the_cost_per_channel(sphere):
    s = sphere
    image = s["rgb"] + np.array([0.1, -0.2, 0.2], np.float32)
    r = REF.step_ref(s["zbuf"], s["rgb"], s["P"], s["K"], image, 0.5, evaluate_only=True)
    covered = (s["zbuf"][:, 1:-1, 1:-1] > 0).reshape(2, -1).sum(1)
    assert np.array_equal(r["inliers"], covered)
    np.testing.assert_allclose(r["rms"], 0.3, rtol=1e-6)         # sqrt(0.01 + 0.04 + 0.04) per kept pixel
    r = REF.step_ref(s["zbuf"], s["rgb"], s["P"], s["K"], image, 0.29, evaluate_only=True)
    assert r["inliers"].tolist() == [0, 0] and r["status"].tolist() == [1, 1]


@pytest.mark.parametrize("mesh", ["sphere", "torus"])
def test_loop_reproduces_the_prototype(mesh):
    """From 3 deg and 6 .. 8 mm: the clean cases land on the prototype's table to its rounding, every case ends below a quarter of
    its start (the prototype's worst ratio is 0.045), the noisy cases' rms is the noise's, sigma sqrt(3)."""
    for noisy in (False, True):
        c = REF.loop_case(mesh, noisy)
        w = c["want"]
        assert (w["status"] == 0).all() and (w["near_ties"] == 0).all()
        for b in range(2):
            re0, te0 = PREF.pose_error(c["start"][b], c["P"][b])
            re, te = PREF.pose_error(w["pose"][b], c["P"][b])
            print("%s %s %d: %d kept pixels, %.4f deg %.4f mm <- %.3f deg %.3f mm, rms %.4f <- %.4f"
                  % ("noisy" if noisy else "clean", mesh, b, w["inliers"][b], re, te, re0, te0, w["rms"][b], w["rms0"][b]))
            assert 2.9 < re0 < 3.1 and 6.0 < te0 < 8.2
            assert re < 0.25 * re0 and te < 0.25 * te0
            kept, re_p, te_p, rms0_p, rms_p = PROTOTYPE[mesh, b]
            if not noisy:
                assert w["inliers"][b] == kept
                assert abs(re - re_p) <= 1e-3 and abs(te - te_p) <= 1e-3 and abs(w["rms0"][b] - rms0_p) <= 1e-3 and abs(w["rms"][b] - rms_p) <= 1e-3
            else:
                assert abs(w["rms"][b] - REF.NOISE_SIGMA * np.sqrt(3.0)) <= 0.1 * REF.NOISE_SIGMA * np.sqrt(3.0)
