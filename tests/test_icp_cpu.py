"""No GPU: the numpy restatement of K29 (tests/icp_ref.py) against independent facts, `icp.step_torch` against the restatement, and the
host side of the entry points: the header-derived binding and the argument checks, which launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import icp_ref as REF
import pnp_ref as PREF


# ----------------------------------------------------------------------------- the binding and the argument checks
def test_binding_has_the_new_entry_points():
    from texpose_amd import _lib
    for name in ("tp_depth_icp_workspace_bytes", "tp_depth_icp_step"):
        assert name in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 16
    restype, argtypes = _lib.HEADER.prototypes["tp_depth_icp_workspace_bytes"]
    assert restype is C.c_size_t and argtypes == [C.c_int] * 3
    fields = ("verts", "faces", "zbuf", "face", "pose", "intr", "depth", "frame", "mask", "V", "F", "B", "Ft", "H", "W", "tau_mm", "damping",
              "evaluate_only", "pose_out", "inliers", "rms", "status", "workspace")
    assert tuple(n for n, _ in _lib.DepthIcpArgs._fields_) == fields
    assert C.sizeof(_lib.DepthIcpArgs) == 9 * 8 + 6 * 4 + 2 * 4 + 4 + 4 + 5 * 8          # (4 bytes of padding before pose_out)
    lib = _lib.load()
    assert hasattr(lib, "tp_depth_icp_step")


def test_workspace_bytes():
    from texpose_amd import _lib
    ws = _lib.load().tp_depth_icp_workspace_bytes
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
    good = dict(V=4, F=2, B=2, Ft=2, H=4, W=4, tau_mm=20.0, damping=1e-6, evaluate_only=0)

    def filled(**kw):
        a = _lib.DepthIcpArgs()
        for k, (name, t) in enumerate(_lib.DepthIcpArgs._fields_):
            if t is C.c_void_p:
                setattr(a, name, p + 256 * k)
        for k, v in {**good, **kw}.items():
            setattr(a, k, v)
        return a

    err = lambda: lib.tp_last_error()
    call = lambda a: lib.tp_depth_icp_step(C.byref(a), None)
    assert lib.tp_depth_icp_step(None, None) == -1 and b"null args" in err()
    for bad in (dict(B=0), dict(B=65536), dict(H=0), dict(W=-1), dict(Ft=0), dict(V=0), dict(F=0), dict(H=65536, W=32768)):
        assert call(filled(**bad)) == -1 and b"bad sizes" in err(), bad
    assert call(filled(Ft=3, frame=None)) == -1 and b"frame map" in err()
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert call(filled(tau_mm=tau)) == -1 and b"tau_mm" in err(), tau
    for damping in (-1e-3, float("nan"), float("inf")):
        assert call(filled(damping=damping)) == -1 and b"damping" in err(), damping
    for name in ("verts", "faces", "zbuf", "face", "pose", "intr", "depth", "pose_out", "inliers", "rms", "status", "workspace"):
        assert call(filled(**{name: None})) == -1 and b"null pointer" in err(), name
    assert call(filled(workspace=p + 8)) == -1 and b"aligned" in err()
    a = filled()
    a.pose_out = a.pose
    assert call(a) == -1 and b"overlap" in err()
    a.pose_out = a.pose + 48                                     # the second pose of the input
    assert call(a) == -1 and b"overlap" in err()


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from texpose_amd import _lib, icp, ops
    verts, faces = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    z, f, pose, K, d = torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, 3, 4), torch.eye(3), torch.zeros(1, 4, 4)
    for call in (lambda: ops.depth_icp_step(verts, faces, z, f, pose, K, d, tau_mm=20.0), lambda: ops.depth_icp(verts, faces, pose, K, d)):
        with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
            call()
    with pytest.raises(_lib.TexposeLibraryError):
        icp.DepthRefiner(verts, faces, 4, 4, "cpu")
    with pytest.raises(ValueError, match="iters"):
        ops.depth_icp(verts, faces, pose, K, d, iters=-1)
    with pytest.raises(ValueError, match="tau_mm"):
        ops.depth_icp(verts, faces, pose, K, d, iters=2, tau_mm=[30.0, 20.0])


# ----------------------------------------------------------------------------- step_torch
@pytest.mark.parametrize("frames,with_mask,evaluate_only", [("one", False, False), ("each", True, False), ("map", False, True), ("map", True, False)])
def test_step_torch_equals_the_restatement(frames, with_mask, evaluate_only):
    from texpose_amd import icp
    c = REF.one_step_case(5, 3, 7, 65, frames, with_mask)
    want = REF.step_ref(c["verts"], c["faces"], c["zbuf"], c["face"], c["pose"], c["K"], c["depth"], c["tau"], 1e-6, c["frame"], c["mask"], evaluate_only)
    t = lambda x: None if x is None else torch.from_numpy(x)
    got = icp.step_torch(t(c["verts"]), t(c["faces"]), t(c["zbuf"]), t(c["face"]), t(c["pose"]), t(c["K"]), t(c["depth"]), c["tau"], 1e-6,
                         t(c["frame"]), t(c["mask"]), evaluate_only)
    assert (want["near_ties"] == 0).all() and (want["inliers"] > 100).all()
    assert got["inliers"].dtype == torch.int32 and np.array_equal(got["inliers"].numpy(), want["inliers"])
    assert np.array_equal(got["status"].numpy(), want["status"]) and (want["status"] == 0).all()
    np.testing.assert_allclose(got["rms"].numpy(), want["rms"], rtol=1e-6)
    if evaluate_only:
        assert np.array_equal(got["pose"].numpy(), c["pose"])
    else:
        assert np.abs(got["pose"].numpy()[:, :, :3] - want["pose"][:, :, :3]).max() <= 1e-6
        np.testing.assert_allclose(got["pose"].numpy()[:, :, 3], want["pose"][:, :, 3], rtol=1e-6)
        assert np.abs(want["pose"] - c["pose"]).max() > 1e-3          # (a step was taken)


def test_step_torch_statuses_pass_the_pose_through():
    from texpose_amd import icp
    c = REF.one_step_case(6, 3, 1, 63, "each", False)
    c["zbuf"][0, 0, 5:] = -1.0                                   # image 0: at most five pixels
    c["face"][1] = 0                                             # image 1: one face, one normal: rank 3
    want = REF.step_ref(c["verts"], c["faces"], c["zbuf"], c["face"], c["pose"], c["K"], c["depth"], c["tau"])
    t = torch.from_numpy
    got = icp.step_torch(t(c["verts"]), t(c["faces"]), t(c["zbuf"]), t(c["face"]), t(c["pose"]), t(c["K"]), t(c["depth"]), c["tau"])
    assert want["status"].tolist() == [1, 3, 0] and got["status"].tolist() == [1, 3, 0]
    assert np.array_equal(got["inliers"].numpy(), want["inliers"]) and want["inliers"][0] < 6 <= want["inliers"][1]
    for b in (0, 1):
        assert np.array_equal(got["pose"].numpy()[b], c["pose"][b]) and np.array_equal(want["pose"][b], c["pose"][b])


# ----------------------------------------------------------------------------- anchors that need no library
@pytest.fixture(scope="module")
def sphere():
    e = PREF.end_to_end_inputs("sphere")
    K = np.tile(e["K"], (2, 1, 1))
    planes = [REF.render_ref(e["verts"], e["faces"], e["P"][b], K[b], e["H"], e["W"]) for b in range(2)]
    return dict(e, K=K, zbuf=np.stack([p[0] for p in planes]), face=np.stack([p[1] for p in planes]))


def test_truth_pose_on_its_own_render_has_no_residual(sphere):
    s = sphere
    depth = s["zbuf"].copy()
    depth[:, ::7, ::5] = 0.0                                     # holes in the measurement
    r = REF.step_ref(s["verts"], s["faces"], s["zbuf"], s["face"], s["P"], s["K"], depth, 20.0)
    covered = ((s["zbuf"] > 0) & (depth > 0)).reshape(2, -1).sum(1)
    assert np.array_equal(r["inliers"], covered) and (covered > 500).all() and (r["status"] == 0).all()
    assert (r["rms"] == 0).all()
    for b in range(2):
        re, te = PREF.pose_error(r["pose"][b], s["P"][b])
        assert re < 1e-5 and te < 1e-4                           # (J^T r = 0: the step is the fp32 rounding of the Gram-Schmidt alone)


def test_plane_seen_head_on_is_rank_three():
    verts = np.array([[-200, -200, 0], [200, -200, 0], [200, 200, 0], [-200, 200, 0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    H, W = 12, 16
    K = np.array([[[300.0, 0, W / 2], [0, 300.0, H / 2], [0, 0, 1]]], np.float32)
    pose = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 500.0]]], np.float32)
    zbuf = np.full((H, W), 500.0, np.float32)                    # what a raster of the plane gives, hand-built: no edge pixels
    face = (np.arange(H * W).reshape(H, W) % 2).astype(np.int32)
    r = REF.step_ref(verts, faces, zbuf[None], face[None], pose, K, zbuf[None] + 3.0, 20.0)
    assert r["inliers"][0] == H * W and r["status"][0] == 3 and np.array_equal(r["pose"], pose)
    assert abs(r["rms"][0] - 3.0) < 1e-12                        # r = (z - d) (n . ray) with n = (0, 0, -1)
    r = REF.step_ref(verts, faces, zbuf[None], face[None], pose, K, zbuf[None] + 3.0, 2.0)
    assert r["inliers"][0] == 0 and r["status"][0] == 1 and np.isnan(r["rms"][0])          # 3 |ray| > 2 everywhere


def test_fewer_than_six_pixels_pass_the_pose_through(sphere):
    s = sphere
    depth = np.zeros_like(s["zbuf"])
    ii, ji = np.nonzero(s["zbuf"][0] > 0)
    depth[0, ii[:5], ji[:5]] = s["zbuf"][0, ii[:5], ji[:5]] + 1.0
    depth[1, ii[:6], ji[:6]] = 0.0
    r = REF.step_ref(s["verts"], s["faces"], s["zbuf"], s["face"], s["P"], s["K"], depth, 20.0)
    assert r["inliers"].tolist() == [5, 0] and r["status"].tolist() == [1, 1] and np.array_equal(r["pose"], s["P"])
    assert r["rms"][0] > 0 and np.isnan(r["rms"][1])


def test_rippled_sphere_is_recovered(sphere):
    """The loop on its own raster, clean depth: from 3 deg and 4 .. 11 mm to below the fp32 floor of the pose (1e-3 deg, 1e-3 mm: about
    16 ulp of a 900 mm depth and the angle it subtends on the 50 mm object); and with 1 mm noise, holes and an occluder to well below
    the noise."""
    s = sphere
    start = REF.perturbed(s["P"], np.random.RandomState(3))
    for b in range(2):
        re, te = PREF.pose_error(start[b], s["P"][b])
        assert 2.9 < re < 3.1 and 3.9 < te < 11.1
    r = REF.icp_ref(s["verts"], s["faces"], start, s["K"], s["zbuf"], 20.0, 5, 1e-6)
    assert (r["status"] == 0).all() and (r["inliers"] >= r["inliers0"]).all() and (r["inliers"] > 500).all()
    assert (r["rms"] < 1e-3).all() and (r["rms0"] > 0.5).all()
    for b in range(2):
        re, te = PREF.pose_error(r["pose"][b], s["P"][b])
        print("clean: image %d ends at %.3g deg, %.3g mm, %d pixels" % (b, re, te, r["inliers"][b]))
        assert re < 1e-3 and te < 1e-3
    noisy = REF.corrupted(s["zbuf"], np.random.RandomState(4), s["W"])
    r = REF.icp_ref(s["verts"], s["faces"], start, s["K"], noisy, 20.0, 5, 1e-6)
    assert (r["status"] == 0).all()
    for b in range(2):
        re, te = PREF.pose_error(r["pose"][b], s["P"][b])
        print("noisy: image %d ends at %.3g deg, %.3g mm, %d pixels, rms %.3f mm" % (b, re, te, r["inliers"][b], r["rms"][b]))
        assert re < 1.0 and te < 0.5 and 0.5 < r["rms"][b] < 1.0          # (1 mm of noise seen through n . ray)
