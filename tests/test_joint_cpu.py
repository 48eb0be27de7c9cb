"""No GPU: the host side of K33 (the header-derived binding of tp_joint_align_step and its refusals, which launch nothing),
`joint.step_torch` against the numpy restatement (tests/joint_ref.py) on all seven term subsets, and the restatement's loop on the
twelve occluded images, which regenerates the table of DESIGN section 23."""
import ctypes as C

import numpy as np
import pytest
import torch

import joint_ref as JREF


# ----------------------------------------------------------------------------- the binding and the argument checks
def test_binding_has_the_joint_step():
    from texpose_amd import _lib
    assert _lib.ABI_VERSION == 16 and "tp_joint_align_step" in _lib.SYMBOLS
    restype, argtypes = _lib.HEADER.prototypes["tp_joint_align_step"]
    assert restype is C.c_int
    assert argtypes == [C.POINTER(_lib.JointAlignArgs), C.POINTER(_lib.SilhouetteAlignArgs), C.POINTER(_lib.PhotoAlignArgs),
                        C.POINTER(_lib.DepthIcpArgs), C.c_void_p]
    fields = [("B", C.c_int), ("pose", C.c_void_p), ("w_sil", C.c_float), ("w_photo", C.c_float), ("w_icp", C.c_float), ("damping", C.c_float),
              ("evaluate_only", C.c_int), ("pose_out", C.c_void_p), ("status", C.c_void_p), ("inliers", C.c_void_p), ("chi2", C.c_void_p)]
    assert list(_lib.JointAlignArgs._fields_) == fields
    assert C.sizeof(_lib.JointAlignArgs) == 4 + 4 + 8 + 4 * 4 + 4 + 4 + 4 * 8          # (4 bytes of padding after B and before pose_out)
    # the three term structs are the existing ones, untouched
    assert len(_lib.PhotoAlignArgs._fields_) == 19 and C.sizeof(_lib.PhotoAlignArgs) == 128
    assert len(_lib.SilhouetteAlignArgs._fields_) == 20 and C.sizeof(_lib.SilhouetteAlignArgs) == 136
    assert len(_lib.DepthIcpArgs._fields_) == 23 and C.sizeof(_lib.DepthIcpArgs) == 152
    lib = _lib.load()
    assert hasattr(lib, "tp_joint_align_step") and lib.tp_abi_version() == 16


def _aligned_buffer(n):
    buf = C.create_string_buffer(n + 16)
    return buf, C.addressof(buf) + (-C.addressof(buf)) % 16


def test_argument_errors_launch_nothing():
    """Every pointer is a host buffer: a launch would fault, a refusal returns before anything reads them."""
    from texpose_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer(1 << 16)
    pose, intr = p, p + 1024
    sizes = dict(B=2, Ft=2, H=4, W=4, damping=1e-6, evaluate_only=0)

    def term(cls, base, **kw):
        a = cls()
        for k, (name, t) in enumerate(cls._fields_):
            if t is C.c_void_p:
                setattr(a, name, base + 512 * k)                 # (workspaces: 2 images x 1 tile x 256 bytes, 16-byte aligned)
        a.pose, a.intr = pose, intr
        for k, v in {**sizes, **kw}.items():
            setattr(a, k, v)
        return a

    sil = lambda **kw: term(_lib.SilhouetteAlignArgs, p + 0x2000, **{**dict(tau_px=4.0), **kw})
    photo = lambda **kw: term(_lib.PhotoAlignArgs, p + 0x6000, **{**dict(tau=0.5), **kw})
    icp = lambda **kw: term(_lib.DepthIcpArgs, p + 0xA000, **{**dict(tau_mm=20.0, V=5, F=3), **kw})

    def joint(**kw):
        j = _lib.JointAlignArgs()
        j.B, j.pose, j.w_sil, j.w_photo, j.w_icp, j.damping, j.evaluate_only = 2, pose, 1.0, 100.0, 0.04, 1e-6, 0
        j.pose_out, j.status, j.inliers, j.chi2 = p + 0xF000, p + 0xF100, p + 0xF200, p + 0xF300
        for k, v in kw.items():
            setattr(j, k, v)
        return j

    ref = lambda a: None if a is None else C.byref(a)
    err = lambda: lib.tp_last_error()
    call = lambda j, s=None, ph=None, i=None: lib.tp_joint_align_step(ref(j), ref(s), ref(ph), ref(i), None)
    refused = lambda word, *a: call(*a) == -1 and word in err() and b"tp_joint_align_step" in err()

    assert call(None, sil(), photo(), icp()) == -1 and b"null args" in err()
    assert refused(b"no term is present", joint())
    assert refused(b"weight > 0", joint(w_sil=0.0), sil())
    assert refused(b"weight > 0", joint(w_sil=0.0, w_photo=0.0), sil(), photo())          # (the depth weight counts only with the term)
    for name in ("w_sil", "w_photo", "w_icp"):
        for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
            assert refused(b"weight must be finite and not negative", joint(**{name: bad}), sil(), photo(), icp()), (name, bad)
    for bad in (-1e-3, float("nan"), float("inf")):
        assert refused(b"damping", joint(damping=bad), sil(), photo())
    for name in ("pose", "status", "inliers", "chi2", "pose_out"):
        assert refused(b"null pointer", joint(**{name: None}), sil(), photo()), name
    for B in (0, -1, 65536):
        assert refused(b"bad sizes", joint(B=B), sil(), photo())
    for out in (pose, pose + 48, pose - 48):
        assert refused(b"pose_out must not overlap pose", joint(pose_out=out), sil(), photo())
    # a term that differs from the others or from the joint arguments
    assert refused(b"B = 3 differs", joint(), sil(B=3, Ft=3), photo())
    assert refused(b"B = 3 differs", joint(), sil(), photo(), icp(B=3, Ft=3))
    assert refused(b"photo term's pose differs", joint(), sil(), photo(pose=pose + 96))
    assert refused(b"silhouette term's pose differs", joint(pose=pose + 96), sil(), photo(pose=pose + 96))
    assert refused(b"the photo term is 4 x 5, the silhouette term 4 x 4", joint(), sil(), photo(W=5))
    assert refused(b"the icp term is 8 x 4, the photo term 4 x 4", joint(), None, photo(), icp(H=8))
    assert refused(b"icp term's intr differs from the silhouette term's", joint(), sil(), None, icp(intr=intr + 72))
    # two terms sharing a workspace (each 512 bytes here), wholly or in part
    ws = sil().workspace
    for other in (ws, ws + 256, ws - 496):
        assert refused(b"the silhouette and the photo term share a workspace", joint(), sil(), photo(workspace=other)), other - ws
        assert refused(b"the silhouette and the icp term share a workspace", joint(), sil(), None, icp(workspace=other))
    assert refused(b"the photo and the icp term share a workspace", joint(), sil(), photo(), icp(workspace=photo().workspace))
    # whatever a term's own step refuses, under that step's name
    own = lambda word, *a: call(*a) == -1 and word in err()
    assert own(b"tp_silhouette_align_step: tau_px", joint(), sil(tau_px=0.0), photo())
    assert own(b"tp_photo_align_step: tau", joint(), sil(), photo(tau=float("nan")))
    assert own(b"tp_depth_icp_step: tau_mm", joint(), sil(), photo(), icp(tau_mm=-1.0))
    assert own(b"tp_depth_icp_step: bad sizes", joint(), sil(), photo(), icp(V=0))
    assert own(b"tp_photo_align_step: null pointer", joint(), sil(), photo(rgb=None))
    assert own(b"tp_silhouette_align_step: null pointer", joint(), sil(inter=None), photo())
    assert own(b"tp_photo_align_step: workspace must be 16-byte aligned", joint(), sil(), photo(workspace=photo().workspace + 8))
    assert own(b"frame map", joint(), sil(Ft=3, frame=None), photo())
    # (a term's own pose_out and evaluate_only are ignored, so a null or an overlapping pose_out there refuses nothing: such a call
    # passes every check and launches, which is test_gpu_joint.py's to make)


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from texpose_amd import _lib, joint, ops
    verts, faces = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    z, pose, K, sdf = torch.zeros(1, 4, 4), torch.zeros(1, 3, 4), torch.eye(3), torch.zeros(1, 4, 4)
    sil = dict(zbuf=z, sdf=sdf, tau_px=4.0)
    for call in (lambda: ops.joint_align_step(pose, K, silhouette=sil), lambda: ops.joint_align(verts, faces, pose, K, sdf=sdf)):
        with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
            call()
    with pytest.raises(_lib.TexposeLibraryError):
        joint.JointRefiner(verts, faces, 4, 4, "cpu")
    for bad in ((1.0, -1.0, 0.0), (float("nan"), 1.0, 1.0), (1.0, float("inf"), 1.0), (1.0, 2.0), 3.0):
        with pytest.raises(ValueError, match="weights"):
            ops.joint_align_step(pose, K, silhouette=sil, weights=bad)
        with pytest.raises(ValueError, match="weights"):
            ops.joint_align(verts, faces, pose, K, sdf=sdf, weights=bad)
    with pytest.raises(ValueError, match="no term"):
        ops.joint_align_step(pose, K)
    with pytest.raises(ValueError, match="no term"):
        ops.joint_align(verts, faces, pose, K)
    with pytest.raises(ValueError, match="weight > 0"):
        ops.joint_align_step(pose, K, silhouette=sil, weights=(0.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="vcolor"):
        ops.joint_align(verts, faces, pose, K, sdf=sdf, image=torch.zeros(1, 4, 4, 3))
    with pytest.raises(ValueError, match="iters"):
        ops.joint_align(verts, faces, pose, K, sdf=sdf, iters=-1)
    with pytest.raises(ValueError, match="tau_px"):
        ops.joint_align(verts, faces, pose, K, sdf=sdf, iters=2, tau_px=[6.0, 4.0])
    assert ops.JOINT_WEIGHTS == (1.0, 100.0, 1.0 / 25.0) == JREF.WEIGHTS


# ----------------------------------------------------------------------------- step_torch
def as_torch(term):
    return None if term is None else {k: torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v for k, v in term.items()}


def torch_step(c, subset, weights, **kw):
    from texpose_amd import joint
    t = {name: as_torch(c[name]) if name in subset else None for name in JREF.TERMS}
    return joint.step_torch(torch.from_numpy(c["pose"]), torch.from_numpy(c["K"]), silhouette=t["sil"], photo=t["photo"], depth=t["icp"],
                            weights=weights, **kw)


def ref_step(c, subset, weights, **kw):
    return JREF.step_ref(c["pose"], c["K"], *[c[name] if name in subset else None for name in JREF.TERMS], weights=weights, **kw)


def close(got, want, pose_in):
    """step_torch against the restatement: both sum in fp64 in their own order; counts and statuses equal, the rest to rounding."""
    assert (want["near_ties"] == 0).all(), "a near-tie in the case: change its seed"
    for k in want:
        if k.endswith(("inliers", "status", "inter", "uni")):
            assert np.array_equal(got[k].numpy(), want[k]), (k, got[k], want[k])
        elif k.endswith("_rms") or k == "chi2":
            g = got[k].numpy().astype(np.float64)
            assert np.array_equal(np.isnan(g), np.isnan(want[k])), k
            ok = ~np.isnan(g)
            assert (np.abs(g[ok] - want[k][ok]) <= 1e-6 * np.abs(want[k][ok]) + 1e-30).all(), (k, g, want[k])
    pose = got["pose"].numpy()
    for b in range(len(pose)):
        if want["status"][b] != 0:
            assert np.array_equal(pose[b].view(np.uint32), pose_in[b].view(np.uint32)), b
        else:
            assert np.abs(pose[b, :, :3] - want["pose"][b, :, :3]).max() <= 1e-6, b
            assert np.abs(pose[b, :, 3] - want["pose"][b, :, 3]).max() <= 1e-6 * np.abs(want["pose"][b, :, 3]).max(), b


@pytest.mark.parametrize("subset", JREF.SUBSETS, ids="+".join)
def test_step_torch_equals_the_restatement(subset):
    """All seven non-empty term subsets on the shared one-step case (33 x 65, B = 3, frame maps that clamp, masks, planted NaN / Inf),
    with the default weights, a step and an evaluation."""
    c = JREF.one_step_case(11, 3, 33, 65, "map", True)
    for evaluate_only in (False, True):
        want = ref_step(c, subset, JREF.WEIGHTS, evaluate_only=evaluate_only)
        got = torch_step(c, subset, JREF.WEIGHTS, evaluate_only=evaluate_only)
        assert set(got) == set(want) - {"near_ties", "rms"}
        close(got, want, c["pose"])
    assert (want["inliers"] == sum(want[name + "_inliers"] for name in subset)).all() and (want["inliers"] > 0).all()


def test_weight_zero_equals_absent_and_one_term_at_weight_one_is_that_term():
    from texpose_amd import icp, photo_align, silhouette
    c = JREF.one_step_case(12, 2, 16, 40, "each", False)
    everything = ("sil", "photo", "icp")
    for absent, weights in ((("icp",), (1.0, 100.0, 0.0)), (("sil",), (0.0, 100.0, 0.04)), (("sil", "icp"), (0.0, 3.0, 0.0))):
        with_zero = torch_step(c, everything, weights)
        without = torch_step(c, tuple(n for n in everything if n not in absent), weights)
        for k in ("pose", "inliers", "status", "chi2"):
            assert torch.equal(with_zero[k], without[k]), (absent, k)
        assert set(with_zero) > set(without)                     # (a present term is still evaluated)
        want = ref_step(c, everything, weights)
        assert np.array_equal(want["pose"], ref_step(c, tuple(n for n in everything if n not in absent), weights)["pose"])
    pose, K = torch.from_numpy(c["pose"]), torch.from_numpy(c["K"])
    s, p, i = (as_torch(c[name]) for name in everything)
    alone = dict(sil=silhouette.step_torch(s["zbuf"], pose, K, s["sdf"], s["tau_px"], 1e-6, s["frame"], s["mask"]),
                 photo=photo_align.step_torch(p["zbuf"], p["rgb"], pose, K, p["image"], p["tau"], 1e-6, p["frame"], p["mask"]),
                 icp=icp.step_torch(i["verts"], i["faces"], i["zbuf"], i["face"], pose, K, i["depth"], i["tau_mm"], 1e-6, i["frame"], i["mask"]))
    for n, name in enumerate(everything):
        got = torch_step(c, (name,), tuple(1.0 if k == n else 7.0 for k in range(3)))
        assert torch.equal(got["pose"], alone[name]["pose"]) and torch.equal(got["status"], alone[name]["status"]), name
        assert torch.equal(got["inliers"], alone[name]["inliers"]) and (got["status"] == 0).all()
        assert not torch.equal(got["pose"], pose)


# ----------------------------------------------------------------------------- the loop: DESIGN section 23's table
def test_the_table_joint_converges_where_photometric_alone_does_not():
    """The twelve occluded images (two bent meshes x two images x bottom third / corner disc / right half hidden) from 8 degrees and
    6 .. 8 mm, texture v / 3, tau_px 4, tau 0.5, damping 1e-6.  Asserted on the restatement: the joint loop at the default weights ends
    every image within 1 degree and 5 mm with status 0 (the issue's prototype: worst 0.28 deg and 2.41 mm), and on the three images the
    issue names the photometric term alone ends more than 5 degrees away (prototype: 15.98, 10.68, 19.08 deg)."""
    print("\n" + "\n".join(JREF.table(routes=("photometric 20", "joint 20, w_photo 100"))))
    worst_deg = worst_mm = 0.0
    for name, kind in JREF.CASES:
        joint, alone = JREF.table_route(name, kind, "joint 20, w_photo 100"), JREF.table_route(name, kind, "photometric 20")
        for b in range(2):
            print("%s %d, %s: joint %.3f deg / %.3f mm (status %d) | photometric alone %.3f deg / %.3f mm"
                  % (name, b, kind, *joint["err"][b], joint["status"][b], *alone["err"][b]))
            assert joint["status"][b] == 0 and JREF.converged(joint["err"][b]), (name, b, kind, joint["err"][b])
            worst_deg, worst_mm = max(worst_deg, joint["err"][b][0]), max(worst_mm, joint["err"][b][1])
            if (name, b, kind) in JREF.PHOTO_ALONE_FAILS:
                assert alone["err"][b][0] > 5.0, (name, b, kind, alone["err"][b])
    print("joint, w_photo 100: worst %.2f deg, worst %.3g mm" % (worst_deg, worst_mm))
    assert worst_deg <= 0.28 + 0.005 and worst_mm <= 2.41 + 0.005          # (the prototype's worst figures, to the printed digits)


def test_the_table_other_rows_are_printed():
    """Silhouette alone, the sequential route (silhouette, then photometric from where it ended) and the joint loop at w_photo 25 and
    400: printed for DESIGN section 23, never asserted beyond the runs ending."""
    lines = JREF.table(routes=("silhouette 10", "silhouette 10, then photometric 10", "joint 20, w_photo 25", "joint 20, w_photo 400"))
    print("\n" + "\n".join(lines))
    assert len(lines) == 4
