"""No GPU: the numpy restatement of K40 (tests/photo_lighting_ref.py) against independent facts, against K37's restatement where the two
must agree, and against its recorded loop table (tests/golden/photo_lighting_loops.npz), and the host side of the entry point: the
header-derived binding and the argument checks, which launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import photo_exposure_ref as XREF
import photo_lighting_ref as REF


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


# ----------------------------------------------------------------------------- the binding and the argument checks
def test_binding_has_the_new_entry_points():
    from texpose_amd import _lib, ops
    for name in ("tp_photo_lighting_workspace_bytes", "tp_photo_lighting"):
        assert name in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 16                                # (additions only, as K37 - K39)
    restype, argtypes = _lib.HEADER.prototypes["tp_photo_lighting_workspace_bytes"]
    assert restype is C.c_size_t and argtypes == [C.c_int] * 3
    fields = ("verts", "faces", "face", "zbuf", "rgb", "pose", "image", "frame", "mask", "light_in", "V", "F", "B", "Ft", "H", "W", "tau", "gain_min",
              "gain_max", "min_var", "light", "count", "rms", "status", "flags", "rgb_out", "workspace")
    assert tuple(n for n, _ in _lib.PhotoLightingArgs._fields_) == fields
    assert C.sizeof(_lib.PhotoLightingArgs) == 10 * 8 + 6 * 4 + 4 * 4 + 7 * 8
    assert (_lib.EXPOSURE_CLAMPED, _lib.EXPOSURE_FLAT, _lib.LIGHTING_FALLBACK) == (REF.CLAMPED, REF.FLAT, REF.FALLBACK)
    assert hasattr(_lib.load(), "tp_photo_lighting")
    assert {"photo_lighting", "photo_lighting_workspace", "PHOTO_LIGHTING_KEYS"} <= set(ops.refine.__all__)
    assert ops.photo_lighting is ops.refine.photo_lighting and ops.PHOTO_LIGHTING_KEYS == ("light", "count", "rms", "status", "flags")


def test_workspace_bytes():
    from texpose_amd import _lib
    ws = _lib.load().tp_photo_lighting_workspace_bytes
    for B, H, W in ((1, 1, 1), (3, 33, 257), (64, 480, 640), (2, 32, 32), (2, 1, 1025)):
        assert ws(B, H, W) == 512 * B * -(-H * W // 1024) == 2 * _lib.load().tp_photo_exposure_workspace_bytes(B, H, W)
    assert ws(0, 5, 5) == 0 and ws(5, 0, 5) == 0 and ws(5, 5, -1) == 0


def test_argument_errors_launch_nothing():
    """Every pointer is a host buffer: a launch would fault, a refusal returns before anything reads them."""
    from texpose_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(32768)
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    good = dict(V=4, F=2, B=2, Ft=2, H=4, W=4, tau=0.5, gain_min=0.25, gain_max=4.0, min_var=1e-6)

    def filled(**kw):
        a = _lib.PhotoLightingArgs()
        for k, (name, t) in enumerate(_lib.PhotoLightingArgs._fields_):
            if t is C.c_void_p:
                setattr(a, name, p + 512 * k)                    # (rgb is 2 * 4 * 4 * 3 * 4 = 384 bytes: nothing overlaps)
        for k, v in {**good, **kw}.items():
            setattr(a, k, v)
        return a

    err = lambda: lib.tp_last_error()
    call = lambda a: lib.tp_photo_lighting(C.byref(a), None)
    assert lib.tp_photo_lighting(None, None) == -1 and b"null args" in err()
    for bad in (dict(B=0), dict(B=65536), dict(H=0), dict(W=-1), dict(Ft=0), dict(H=65536, W=32768), dict(V=0), dict(F=0), dict(V=-3), dict(F=-1)):
        assert call(filled(**bad)) == -1 and b"bad sizes" in err(), bad
    assert call(filled(Ft=3, frame=None)) == -1 and b"frame map" in err()
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert call(filled(tau=tau)) == -1 and b"tau" in err(), tau
    for bad in (dict(gain_min=0.0), dict(gain_min=-1.0), dict(gain_min=1.5), dict(gain_min=float("nan")), dict(gain_max=0.5),
                dict(gain_max=float("inf")), dict(gain_max=float("nan"))):
        assert call(filled(**bad)) == -1 and b"gain_min" in err(), bad
    for min_var in (-1e-3, float("nan"), float("inf")):
        assert call(filled(min_var=min_var)) == -1 and b"min_var" in err(), min_var
    for name in ("verts", "faces", "face", "zbuf", "rgb", "pose", "image", "light", "count", "rms", "status", "flags", "workspace"):
        assert call(filled(**{name: None})) == -1 and b"null pointer" in err(), name
    assert call(filled(workspace=p + 8)) == -1 and b"aligned" in err()
    a = filled()
    a.rgb_out = a.rgb + 48                                       # overlapping rgb without being rgb
    assert call(a) == -1 and b"rgb_out" in err()
    a = filled()
    a.light = a.light_in + 60                                    # the second image's light of the input
    assert call(a) == -1 and b"overlap" in err()


def test_ops_refuse_cpu_tensors_and_both_keywords():
    """exposure= with lighting= is a host error, raised before anything could touch a device: the tensors here are on the CPU."""
    from texpose_amd import _lib, joint, multiview, ops, photo_align
    verts, faces, vcolor = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    z, c, pose, K, im = torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, 3), torch.zeros(1, 3, 4), torch.eye(3), torch.zeros(1, 4, 4, 3)
    with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
        ops.photo_lighting(verts, faces, torch.zeros(1, 4, 4, dtype=torch.int32), z, c, pose, im, tau=0.5)
    with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
        ops.photo_align(verts, faces, vcolor, pose, K, im, lighting=True)
    both = dict(exposure=True, lighting=True)
    for call in (lambda: ops.photo_align(verts, faces, vcolor, pose, K, im, **both),
                 lambda: ops.joint_align(verts, faces, pose, K, vcolor=vcolor, image=im, **both),
                 lambda: ops.multiview_align(verts, faces, pose, pose, torch.zeros(1, dtype=torch.int32), K, vcolor=vcolor, image=im, **both),
                 lambda: photo_align.PhotoRefiner(verts, faces, vcolor, 4, 4, "cpu", **both),
                 lambda: joint.JointRefiner(verts, faces, 4, 4, "cpu", vcolor=vcolor, **both),
                 lambda: multiview.MultiViewRefiner(verts, faces, 4, 4, "cpu", vcolor=vcolor, **both)):
        with pytest.raises(ValueError, match="exclude each other"):
            call()


# ----------------------------------------------------------------------------- lighting_torch
def torch_call(c, **kw):
    from texpose_amd import photo_align
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x))
    return photo_align.lighting_torch(*(t(c[k]) for k in ("verts", "faces", "face", "zbuf", "rgb", "pose", "image")), c["tau"], t(c["light_in"]),
                                      t(c["frame"]), t(c["mask"]), **kw)


@pytest.mark.parametrize("frames,with_mask,with_fit", [("one", False, False), ("each", True, True), ("map", False, True), ("map", True, False)])
def test_lighting_torch_equals_the_restatement(frames, with_mask, with_fit):
    """Planted NaN / Inf in every plane, a mask, a frame map whose entries clamp, and face and vertex indices out of range."""
    c = REF.one_call_case(5, 3, 16, 65, frames, with_mask, with_fit)
    c["faces"] = c["faces"].copy()
    c["faces"][3] = [0, 1, len(c["verts"])]
    c["face"][:, 5, 7:11] = [-1, len(c["faces"]), 2 ** 31 - 1, -2 ** 31]
    want, got = REF.call_ref(c), torch_call(c)
    assert want["count"].sum() > 100 and 0 in want["status"] and (want["near_ties"] == 0).all()
    for k in ("count", "status", "flags"):
        assert got[k].dtype == torch.int32 and np.array_equal(got[k].numpy(), want[k]), k
    assert got["light"].dtype == torch.float32 and (np.abs(got["light"].numpy() - want["light"]) <= 1e-6 * np.maximum(1.0, np.abs(want["light"]))).all()
    rms = got["rms"].numpy().astype(np.float64)
    assert (np.abs(rms - want["rms"]) <= 1e-5 * want["rms"] + 1e-6).all()
    lit = np.stack([REF.apply_ref(c["verts"], c["faces"], c["face"][b], c["zbuf"][b], c["rgb"][b], c["pose"][b], got["light"].numpy()[b]) for b in range(3)])
    assert same_bits(got["rgb"].numpy(), lit) and "rgb" not in torch_call(c, apply=False)
    c2 = exact_case(mesh=REF.quad_mesh())                        # the fallback's flags and words
    got, want = torch_call(c2), REF.call_ref(c2)
    assert np.array_equal(got["flags"].numpy(), want["flags"]) and (want["flags"] == 7 * REF.FALLBACK).all()
    assert np.abs(got["light"].numpy() - want["light"]).max() <= 1e-6


# ----------------------------------------------------------------------------- anchors that need no library
def exact_case(H=12, W=17, B=2, mesh=None, light=None, seed=3):
    """Colours in multiples of 1 / 256, every pixel covered, a face plane uniform over the mesh's faces, random poses; the photograph
    is the restatement's own apply under ``light`` [B,3,5] (None: image = 0.75 rgb + 0.125, exact in fp32)."""
    rs = np.random.RandomState(seed)
    verts, faces = REF.bumpy_mesh(seed) if mesh is None else mesh
    rgb = (rs.randint(1, 257, (B, H, W, 3)) / 256.0).astype(np.float32)
    zbuf = np.full((B, H, W), 900.0, np.float32)
    face = rs.randint(0, len(faces), (B, H, W)).astype(np.int32)
    pose = np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        pose[b] = np.concatenate([q, [[3.0], [-5.0], [900.0]]], 1)
    if light is None:
        image = (0.75 * rgb + 0.125).astype(np.float32)
    else:
        image = np.stack([REF.apply_ref(verts, faces, face[b], zbuf[b], rgb[b], pose[b], light[b]) for b in range(B)])
    return dict(verts=verts, faces=faces, face=face, zbuf=zbuf, rgb=rgb, pose=pose, image=image, frame=None, mask=None, light_in=None, tau=2.0)


KNOWN = np.array([[[0.7, -0.2, 0.1, -0.15, 0.05], [0.9, 0.1, 0.25, -0.1, -0.02], [1.2, -0.3, -0.3, -0.3, 0.1]],
                  [[0.5, 0.0, 0.0, -0.25, 0.0], [1.0, 0.3, -0.2, 0.1, 0.03], [0.8, 0.05, 0.05, 0.05, -0.05]]], np.float32)


def test_normals_are_unit_face_the_camera_and_ignore_the_winding():
    c = exact_case()
    n, ok = REF.face_normals_ref(c["verts"], c["faces"], c["pose"][0])
    assert ok.all() and np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-12
    P = c["pose"][0].astype(np.float64)
    centre = c["verts"][c["faces"]].astype(np.float64).mean(1) @ P[:, :3].T + P[:, 3]
    assert ((n * centre).sum(1) < 0).all()                       # towards the camera at the origin
    flipped, _ = REF.face_normals_ref(c["verts"], c["faces"][:, ::-1], c["pose"][0])
    assert np.abs(flipped - n).max() <= 1e-12
    assert len({tuple(np.round(v, 6)) for v in n}) == len(n)     # (the builder's faces all differ: the 5 x 5 systems are regular)


def test_exact_recovery():
    """The photograph is the restatement's own apply at the same pose: the light comes back to the photograph's fp32 rounding (2^-24
    relative per value, through a well-conditioned 5 x 5 system: 1e-5 is generous), rms ~ 0."""
    c = exact_case(light=KNOWN)
    r = REF.call_ref(c)
    assert r["status"].tolist() == [0, 0] and r["flags"].tolist() == [0, 0] and r["count"].tolist() == [10 * 15] * 2
    assert np.abs(r["light"].astype(np.float64) - KNOWN).max() <= 1e-5, r["light"] - KNOWN
    assert (r["rms"] <= 1e-6).all(), r["rms"]
    relit = np.stack([REF.apply_ref(c["verts"], c["faces"], c["face"][b], c["zbuf"][b], c["rgb"][b], c["pose"][b], KNOWN[b]) for b in range(2)])
    assert same_bits(relit, c["image"]) and np.abs(r["rgb"] - c["image"]).max() <= 1e-5


def test_without_a_directional_part_it_is_the_exposure_fit():
    c = exact_case()
    r = REF.call_ref(c)
    x = XREF.exposure_ref(c["zbuf"], c["rgb"], c["image"], c["tau"])
    assert r["status"].tolist() == [0, 0] and r["flags"].tolist() == [0, 0] and np.array_equal(r["count"], x["count"])
    L = r["light"].astype(np.float64)
    assert np.abs(L[..., 0] - 0.75).max() <= 1e-6 and np.abs(L[..., 4] - 0.125).max() <= 1e-6 and np.abs(L[..., 1:4]).max() <= 1e-6
    assert np.abs(L[..., 0] - x["gain"]).max() <= 1e-6 and np.abs(L[..., 4] - x["bias"]).max() <= 1e-6


def test_a_coplanar_mesh_falls_back_to_the_exposure_fit_bit_for_bit():
    """Two coplanar triangles: the normal is one vector, the regressors c n_x, c n_y, c n_z are multiples of c and the 5 x 5 system is
    singular: every channel takes K37's closed form on the record's own sub-sums -- same kept set, same sums, same order."""
    rs = np.random.RandomState(8)
    c = exact_case(mesh=REF.quad_mesh())
    c["image"] = (c["image"] + rs.uniform(-0.05, 0.05, c["image"].shape)).astype(np.float32)
    for tau, light_in, x_in in ((2.0, None, (None, None)), (0.06, np.tile(np.float32([0.75, 0, 0, 0, 0.125]), (2, 3, 1)),
                                                            (np.full((2, 3), 0.75, np.float32), np.full((2, 3), 0.125, np.float32)))):
        r = REF.lighting_ref(c["verts"], c["faces"], c["face"], c["zbuf"], c["rgb"], c["pose"], c["image"], tau, light_in)
        x = XREF.exposure_ref(c["zbuf"], c["rgb"], c["image"], tau, *x_in)
        assert np.array_equal(r["kept"], x["kept"]) and np.array_equal(r["count"], x["count"]) and (r["count"] > 50).all()
        assert r["status"].tolist() == [0, 0] and (r["flags"] == (x["flags"] | (7 * REF.FALLBACK))).all()
        assert same_bits(r["light"][..., 0], x["gain"]) and same_bits(r["light"][..., 4], x["bias"]) and (r["light"][..., 1:4] == 0).all()
        assert same_bits(r["rgb"], x["rgb"])                     # a light without a direction applies as K37's
        assert np.abs(r["rms"] - x["rms"]).max() <= 1e-9
    assert 0 < r["count"].min() and r["count"].max() < 150       # (the second round's tau dropped pixels)


def test_decision_paths():
    c = exact_case(H=3, W=7, light=KNOWN)                        # five interior pixels: status 1, the light passed through
    c["light_in"] = (KNOWN + 0.01).astype(np.float32)
    r = REF.call_ref(c)
    assert r["count"].tolist() == [5, 5] and r["status"].tolist() == [1, 1] and same_bits(r["light"], c["light_in"])
    assert same_bits(r["rgb"], np.stack([REF.apply_ref(c["verts"], c["faces"], c["face"][b], c["zbuf"][b], c["rgb"][b], c["pose"][b], c["light_in"][b])
                                         for b in range(2)]))
    c["light_in"] = None
    r = REF.call_ref(c)
    assert r["status"].tolist() == [1, 1] and same_bits(r["light"], np.tile(REF.IDENTITY, (2, 3, 1))) and same_bits(r["rgb"], c["rgb"])
    c = exact_case(H=2, W=5)                                     # no interior at all: NaN rms, every channel flat and fallen back
    r = REF.call_ref(c)
    assert r["count"].tolist() == [0, 0] and r["status"].tolist() == [1, 1] and np.isnan(r["rms"]).all()
    assert r["flags"].tolist() == [7 * (REF.FALLBACK | REF.FLAT)] * 2

    c = exact_case()                                             # an ambient term outside gain_range: the fallback, clamped
    c["image"], c["tau"] = (8.0 * c["rgb"]).astype(np.float32), 100.0
    r = REF.call_ref(c)
    x = XREF.exposure_ref(c["zbuf"], c["rgb"], c["image"], c["tau"])
    assert r["status"].tolist() == [0, 0] and r["flags"].tolist() == [7 * (REF.FALLBACK | REF.CLAMPED)] * 2
    assert (r["light"][..., 0] == 4.0).all() and (r["light"][..., 1:4] == 0).all() and same_bits(r["light"][..., 4], x["bias"])

    strong = KNOWN.copy()                                        # |l_dir| > l0 in channel 1 of image 0 alone
    strong[0, 1, 1:4] = [0.9, -0.6, 0.5]
    c = exact_case(light=strong)
    r = REF.call_ref(c)
    assert r["status"].tolist() == [0, 0] and r["flags"][1] == 0 and r["flags"][0] & (7 * REF.FALLBACK) == REF.FALLBACK << 1
    assert (r["light"][0, 1, 1:4] == 0).all() and np.abs(r["light"][0, [0, 2]].astype(np.float64) - strong[0, [0, 2]]).max() <= 1e-5
    inside = REF.call_ref(c, gain_range=(0.95, 4.0))             # l0 = 0.7, 0.9, ... below a gain_min of 0.95
    assert inside["flags"][0] & (7 * REF.FALLBACK) == 7 * REF.FALLBACK - (REF.FALLBACK << 2)          # (channel 2's 1.2 is inside)


def test_the_incoming_light_decides_what_is_kept():
    c = exact_case(light=KNOWN)
    c["tau"] = 0.01
    assert REF.call_ref(c)["count"].sum() < 40
    c["light_in"] = KNOWN
    assert REF.call_ref(c)["count"].tolist() == [150, 150]


def test_bad_indices_are_pixels_without_a_normal():
    """A face plane holding -1, F, INT_MAX and INT_MIN, and faces with an index >= V or < 0: skipped by the fit; the apply gives them the
    ambient form."""
    c = exact_case(light=KNOWN)
    F, V = len(c["faces"]), len(c["verts"])
    c["faces"] = c["faces"].copy()
    c["faces"][3] = [0, 1, V]
    c["faces"][5] = [-1, 2, 3]
    c["faces"][7] = [2 ** 31 - 1, 2, 3]
    c["face"][:, 4, 3:9] = [-1, F, 2 ** 31 - 1, -2 ** 31, 3, 5]
    c["face"][:, 6, 3] = 7
    n, valid = REF.pixel_normals_ref(c["verts"], c["faces"], c["face"][0], c["pose"][0])
    assert not valid[4, 3:9].any() and not valid[6, 3] and (n[~valid] == 0).all()
    r = REF.call_ref(c)
    assert not r["kept"][:, 4, 3:9].any() and not r["kept"][:, 6, 3].any() and (r["count"] < 150).all() and (r["count"] >= 150 - 7 - 12).all()
    assert np.abs(r["light"].astype(np.float64) - KNOWN).max() <= 1e-5
    l = r["light"]
    assert same_bits(r["rgb"][:, 4, 3:9], l[:, None, :, 0] * c["rgb"][:, 4, 3:9] + l[:, None, :, 4])


# ----------------------------------------------------------------------------- the loop's figures
@pytest.mark.parametrize("mesh", REF.MESHES)
def test_loop_reproduces_the_recorded_table(mesh):
    """The reason for the feature, and its effect: under ambient + a directional light of 0.45 of it (and K37's bias) the lighting
    loop ends every clean and every noisy case below a quarter of its start in rotation and in translation; the recorded plain loop and
    the recorded exposure=True loop miss that bar on every image, in rotation or in translation (tests/golden holds this file's own
    results; the lighting loops run again here and must reproduce them)."""
    g = REF.golden()
    start = g["start_err/%s" % mesh]
    for noisy in (False, True):
        c = REF.loop_case(mesh, noisy)
        w = c["want"]
        key = "%.2f/%s/%s/" % (REF.STRENGTH, mesh, "noisy" if noisy else "clean")
        assert (w["status"] == 0).all() and (w["lighting_status"] == 0).all() and (w["near_ties"] == 0).all() and (w["lighting_flags"] == 0).all()
        err = np.array(REF.errors(c, w["pose"]))
        assert np.abs(err - g[key + "lighting/err"]).max() <= 1e-3 and np.abs(w["light"] - g[key + "lighting/light"]).max() <= 1e-4
        for b in range(2):
            (re0, te0), (re, te) = start[b], err[b]
            print("%s %s %d: lighting %.4f deg %.4f mm <- %.3f deg %.3f mm | exposure %s | plain %s | light %s"
                  % ("noisy" if noisy else "clean", mesh, b, re, te, re0, te0, g[key + "exposure/err"][b].round(3), g[key + "plain/err"][b].round(3),
                     w["light"][b].round(3).tolist()))
            assert 2.9 < re0 < 3.1 and 6.0 < te0 < 8.2
            assert re <= 0.25 * re0 and te <= 0.25 * te0
            for other in ("plain", "exposure"):
                re_o, te_o = g[key + other + "/err"][b]
                assert re_o > 0.25 * re0 or te_o > 0.25 * te0, other
            if not noisy:
                assert np.abs(w["light"][b] - REF.true_light()).max() <= 1e-2
        strong = "%.2f/%s/%s/" % (REF.STRONG, mesh, "noisy" if noisy else "clean")         # the recorded stronger row
        assert (g[strong + "lighting/err"] <= 0.25 * start).all() and (g[strong + "lighting/flags"] == 0).all()
