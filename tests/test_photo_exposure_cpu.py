"""No GPU: the numpy restatement of K37 (tests/photo_exposure_ref.py) against independent facts and against its pinned figures,
`photo_align.exposure_torch` against the restatement, and the host side of the entry point: the header-derived binding and the
argument checks, which launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import photo_exposure_ref as REF


# ----------------------------------------------------------------------------- the binding and the argument checks
def test_binding_has_the_new_entry_points():
    from texpose_amd import _lib, ops
    for name in ("tp_photo_exposure_workspace_bytes", "tp_photo_exposure"):
        assert name in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 16
    restype, argtypes = _lib.HEADER.prototypes["tp_photo_exposure_workspace_bytes"]
    assert restype is C.c_size_t and argtypes == [C.c_int] * 3
    fields = ("zbuf", "rgb", "image", "frame", "mask", "gain_in", "bias_in", "B", "Ft", "H", "W", "tau", "gain_min", "gain_max", "min_var",
              "gain", "bias", "count", "rms", "status", "flags", "rgb_out", "workspace")
    assert tuple(n for n, _ in _lib.PhotoExposureArgs._fields_) == fields
    assert C.sizeof(_lib.PhotoExposureArgs) == 7 * 8 + 4 * 4 + 4 * 4 + 8 * 8
    assert (_lib.EXPOSURE_CLAMPED, _lib.EXPOSURE_FLAT) == (REF.CLAMPED, REF.FLAT)
    assert hasattr(_lib.load(), "tp_photo_exposure")
    assert {"photo_exposure", "photo_exposure_workspace"} <= set(ops.refine.__all__) and ops.photo_exposure is ops.refine.photo_exposure


def test_workspace_bytes():
    from texpose_amd import _lib
    ws = _lib.load().tp_photo_exposure_workspace_bytes
    for B, H, W in ((1, 1, 1), (3, 33, 257), (64, 480, 640), (2, 32, 32), (2, 1, 1025)):
        want = 256 * B * -(-H * W // 1024)
        assert ws(B, H, W) == (want + 15) // 16 * 16 == _lib.load().tp_photo_align_workspace_bytes(B, H, W)
    assert ws(0, 5, 5) == 0 and ws(5, 0, 5) == 0 and ws(5, 5, -1) == 0


def test_argument_errors_launch_nothing():
    """Every pointer is a host buffer: a launch would fault, a refusal returns before anything reads them."""
    from texpose_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(16384)
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    good = dict(B=2, Ft=2, H=4, W=4, tau=0.5, gain_min=0.25, gain_max=4.0, min_var=1e-6)

    def filled(**kw):
        a = _lib.PhotoExposureArgs()
        for k, (name, t) in enumerate(_lib.PhotoExposureArgs._fields_):
            if t is C.c_void_p:
                setattr(a, name, p + 512 * k)                    # (rgb is 2 * 4 * 4 * 3 * 4 = 384 bytes: nothing overlaps)
        for k, v in {**good, **kw}.items():
            setattr(a, k, v)
        return a

    err = lambda: lib.tp_last_error()
    call = lambda a: lib.tp_photo_exposure(C.byref(a), None)
    assert lib.tp_photo_exposure(None, None) == -1 and b"null args" in err()
    for bad in (dict(B=0), dict(B=65536), dict(H=0), dict(W=-1), dict(Ft=0), dict(H=65536, W=32768)):
        assert call(filled(**bad)) == -1 and b"bad sizes" in err(), bad
    assert call(filled(Ft=3, frame=None)) == -1 and b"frame map" in err()
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert call(filled(tau=tau)) == -1 and b"tau" in err(), tau
    for bad in (dict(gain_min=0.0), dict(gain_min=-1.0), dict(gain_min=1.5), dict(gain_min=float("nan")), dict(gain_max=0.5),
                dict(gain_max=float("inf")), dict(gain_max=float("nan"))):
        assert call(filled(**bad)) == -1 and b"gain_min" in err(), bad
    for min_var in (-1e-3, float("nan"), float("inf")):
        assert call(filled(min_var=min_var)) == -1 and b"min_var" in err(), min_var
    for name in ("zbuf", "rgb", "image", "gain", "bias", "count", "rms", "status", "flags", "workspace"):
        assert call(filled(**{name: None})) == -1 and b"null pointer" in err(), name
    assert call(filled(workspace=p + 8)) == -1 and b"aligned" in err()
    a = filled()
    a.rgb_out = a.rgb + 48                                       # overlapping rgb without being rgb
    assert call(a) == -1 and b"rgb_out" in err()
    for out, given in (("gain", "gain_in"), ("gain", "bias_in"), ("bias", "gain_in"), ("bias", "bias_in")):
        a = filled()
        setattr(a, out, getattr(a, given) + 12)                  # the second image's fit of the input
        assert call(a) == -1 and b"overlap" in err(), (out, given)


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from texpose_amd import _lib, ops, photo_align
    verts, faces, vcolor = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    z, c, pose, K, im = torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, 3), torch.zeros(1, 3, 4), torch.eye(3), torch.zeros(1, 4, 4, 3)
    with pytest.raises(ValueError, match="GPU"):
        ops.photo_exposure(z, c, im, tau=0.5)
    with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
        ops.photo_align(verts, faces, vcolor, pose, K, im, exposure=True)
    with pytest.raises(_lib.TexposeLibraryError):
        photo_align.PhotoRefiner(verts, faces, vcolor, 4, 4, "cpu", exposure=True)


# ----------------------------------------------------------------------------- exposure_torch
def torch_call(c, **kw):
    from texpose_amd import photo_align
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x))
    return photo_align.exposure_torch(t(c["zbuf"]), t(c["rgb"]), t(c["image"]), c["tau"], t(c["gain_in"]), t(c["bias_in"]), t(c["frame"]), t(c["mask"]), **kw)


def ref_call(c, **kw):
    return REF.exposure_ref(c["zbuf"], c["rgb"], c["image"], c["tau"], c["gain_in"], c["bias_in"], c["frame"], c["mask"], **kw)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def agree(got, want):
    """exposure_torch against the restatement: integers equal, the fit to a few fp32 roundings, the applied colours from the fit."""
    assert (want["near_ties"] == 0).all()
    for k in ("count", "status", "flags"):
        assert got[k].dtype == torch.int32 and np.array_equal(got[k].numpy(), want[k]), k
    for k in ("gain", "bias"):
        assert got[k].dtype == torch.float32
        assert (np.abs(got[k].numpy() - want[k]) <= 1e-6 * np.maximum(1.0, np.abs(want[k]))).all(), k
    rms = got["rms"].numpy().astype(np.float64)
    assert np.array_equal(np.isnan(rms), np.isnan(want["rms"]))
    ok = ~np.isnan(rms)
    assert (np.abs(rms[ok] - want["rms"][ok]) <= 1e-5 * want["rms"][ok] + 1e-6).all()


@pytest.mark.parametrize("frames,with_mask,with_fit", [("one", False, False), ("each", True, True), ("map", False, True), ("map", True, False)])
def test_exposure_torch_equals_the_restatement(frames, with_mask, with_fit):
    """Planted NaN / Inf in every plane, a mask and a frame map whose entries clamp."""
    c = REF.one_call_case(5, 3, 16, 65, frames, with_mask, with_fit)
    assert not np.isfinite(c["zbuf"]).all() and not np.isfinite(c["rgb"]).all() and not np.isfinite(c["image"]).all()
    want, got = ref_call(c), torch_call(c)
    assert want["count"].sum() > 100 and 0 in want["status"]
    agree(got, want)
    z, lit = c["zbuf"], REF.apply_ref(c["zbuf"], c["rgb"], got["gain"].numpy(), got["bias"].numpy())
    assert same_bits(got["rgb"].numpy(), lit) and same_bits(lit[~((z > 0) & np.isfinite(z))], c["rgb"][~((z > 0) & np.isfinite(z))])
    assert "rgb" not in torch_call(c, apply=False)


# ----------------------------------------------------------------------------- anchors that need no library
def exact_case(H=12, W=17, B=2):
    """Colours in multiples of 1 / 256, every pixel covered: g c + b is exact in fp32 for g = 3 / 4, b = 1 / 8."""
    rs = np.random.RandomState(3)
    rgb = (rs.randint(0, 257, (B, H, W, 3)) / 256.0).astype(np.float32)
    return dict(zbuf=np.full((B, H, W), 900.0, np.float32), rgb=rgb, image=(0.75 * rgb + 0.125).astype(np.float32), frame=None, mask=None,
                gain_in=None, bias_in=None, tau=2.0)


def test_exact_recovery():
    c = exact_case()
    for r in (ref_call(c), {k: np.asarray(v) for k, v in torch_call(c).items()}):
        assert np.abs(r["gain"].astype(np.float64) - 0.75).max() <= 1e-12 and np.abs(r["bias"].astype(np.float64) - 0.125).max() <= 1e-12
        assert (r["rms"] <= 1e-7).all() and r["status"].tolist() == [0, 0] and r["flags"].tolist() == [0, 0]
        assert r["count"].tolist() == [10 * 15] * 2              # the interior
        assert same_bits(r["rgb"], c["image"])                   # border pixels included: they are covered


def test_a_flat_channel_keeps_gain_one():
    c = exact_case()
    c["rgb"][..., 1] = 0.5
    c["image"][..., 1] = 0.625
    for r in (ref_call(c), {k: np.asarray(v) for k, v in torch_call(c).items()}):
        assert r["flags"].tolist() == [REF.FLAT << 1] * 2 and r["status"].tolist() == [0, 0]
        assert (r["gain"][:, 1] == 1.0).all() and (r["bias"][:, 1] == 0.125).all()          # the mean difference
        assert np.abs(r["gain"][:, [0, 2]].astype(np.float64) - 0.75).max() <= 1e-12


def test_a_gain_out_of_range_is_clamped():
    c = exact_case()
    c["image"] = (8.0 * c["rgb"]).astype(np.float32)
    c["tau"] = 100.0
    for r in (ref_call(c), {k: np.asarray(v) for k, v in torch_call(c).items()}):
        assert (r["gain"] == 4.0).all() and r["flags"].tolist() == [7, 7] and r["status"].tolist() == [0, 0]
        mc = c["rgb"][:, 1:-1, 1:-1].astype(np.float64).mean((1, 2))
        np.testing.assert_allclose(r["bias"], 4.0 * mc, rtol=1e-6)                           # b = mo - g mc = 8 mc - 4 mc
        assert (r["rms"] > 0.1).all()
    c["image"] = (0.125 * c["rgb"]).astype(np.float32)
    assert (ref_call(c)["gain"] == 0.25).all() and ref_call(c)["flags"].tolist() == [7, 7]


def test_fewer_than_six_pixels_pass_the_fit_through():
    c = exact_case(H=2, W=5)                                     # no interior
    c["gain_in"] = np.array([[0.9, 1.1, 1.2], [0.8, 0.7, 1.3]], np.float32)
    c["bias_in"] = np.array([[0.01, -0.02, 0.03], [0.0, 0.1, -0.1]], np.float32)
    for r in (ref_call(c), {k: np.asarray(v) for k, v in torch_call(c).items()}):
        assert r["count"].tolist() == [0, 0] and r["status"].tolist() == [1, 1] and np.isnan(r["rms"]).all()
        assert same_bits(r["gain"], c["gain_in"]) and same_bits(r["bias"], c["bias_in"])
        assert same_bits(r["rgb"], REF.apply_ref(c["zbuf"], c["rgb"], c["gain_in"], c["bias_in"]))
    c = exact_case(H=3, W=7)                                     # five interior pixels, no fit given: the identity
    for r in (ref_call(c), {k: np.asarray(v) for k, v in torch_call(c).items()}):
        assert r["count"].tolist() == [5, 5] and r["status"].tolist() == [1, 1] and not np.isnan(r["rms"]).any()
        assert (r["gain"] == 1.0).all() and (r["bias"] == 0.0).all() and same_bits(r["rgb"], c["rgb"])


def test_the_incoming_fit_decides_what_is_kept():
    """tau judges o - (a c + d): with the true fit coming in every pixel is kept at a tau that keeps none without it."""
    c = exact_case()
    c["tau"] = 0.01
    assert ref_call(c)["count"].sum() < 20
    c["gain_in"], c["bias_in"] = np.full((2, 3), 0.75, np.float32), np.full((2, 3), 0.125, np.float32)
    assert ref_call(c)["count"].tolist() == [150, 150]


# ----------------------------------------------------------------------------- the loop's figures
@pytest.mark.parametrize("mesh", ["sphere", "torus"])
def test_loop_reproduces_the_pinned_table(mesh):
    """The reason for the feature, and its effect: on the exposure-changed photographs the plain K30 loop ends no closer in translation
    than half its start; with the fit in front of each step every clean and every noisy case ends below a quarter of its start in
    rotation and in translation; on unchanged photographs the fit does no harm."""
    plain = REF.loop_case(mesh, False, compensated=False)
    same = REF.loop_case(mesh, False, exposed=False)
    for noisy in (False, True):
        c = REF.loop_case(mesh, noisy)
        w = c["want"]
        assert (w["status"] == 0).all() and (w["exposure_status"] == 0).all() and (w["near_ties"] == 0).all()
        for b, ((re0, te0), (re, te), (re_p, te_p), (re_s, te_s)) in enumerate(zip(REF.errors(c, c["start"]), REF.errors(c, w["pose"]),
                                                                                  REF.errors(plain, plain["want"]["pose"]),
                                                                                  REF.errors(same, same["want"]["pose"]))):
            print("%s %s %d: %.4f deg %.4f mm <- %.3f deg %.3f mm, rms %.4f, gain %s bias %s | plain loop %.4f deg %.4f mm | unchanged photograph %.4f deg %.4f mm"
                  % ("noisy" if noisy else "clean", mesh, b, re, te, re0, te0, w["rms"][b], w["gain"][b].round(4), w["bias"][b].round(4), re_p, te_p,
                     re_s, te_s))
            assert 2.9 < re0 < 3.1 and 6.0 < te0 < 8.2
            assert re <= 0.25 * re0 and te <= 0.25 * te0
            assert te_p >= 0.5 * te0
            assert re_s <= 0.05 and te_s <= 0.05
            if not noisy:
                pinned = REF.TABLE[mesh, b]
                assert np.abs(np.array([re_p, te_p, re, te]) - pinned).max() <= 1e-3, ((re_p, te_p, re, te), pinned)
                assert np.abs(w["gain"][b] - REF.EXPOSURE_GAIN).max() <= 2e-3 and np.abs(w["bias"][b] - REF.EXPOSURE_BIAS).max() <= 2e-3
