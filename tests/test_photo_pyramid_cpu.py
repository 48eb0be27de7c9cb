"""No GPU: the numpy restatement of K38 (tests/photo_pyramid_ref.py) against independent facts and against its pinned figures,
`photo_align.pyramid_torch` against the restatement, and the host side of the entry points: the header-derived binding and the
argument checks, which launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import photo_pyramid_ref as REF
import photo_ref as PR


# ----------------------------------------------------------------------------- the binding and the argument checks
def test_binding_has_the_new_entry_points():
    from texpose_amd import _lib, ops, photo_align
    for name in ("tp_image_down", "tp_surface_down", "tp_mask_down"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
        restype, argtypes = _lib.HEADER.prototypes[name]
        assert restype is C.c_int and argtypes == [C.POINTER(_lib.PyramidDownArgs), C.c_void_p]
    assert _lib.ABI_VERSION == 16
    assert tuple(n for n, _ in _lib.PyramidDownArgs._fields_) == ("zbuf", "rgb", "mask", "N", "H", "W", "zbuf_out", "rgb_out", "mask_out")
    assert C.sizeof(_lib.PyramidDownArgs) == 3 * 8 + 3 * 4 + 4 + 3 * 8           # (4 bytes of padding in front of zbuf_out)
    assert {"image_down", "surface_down", "mask_down", "image_pyramid", "mask_pyramid"} <= set(ops.refine.__all__)
    assert ops.surface_down is ops.refine.surface_down and callable(photo_align.pyramid_torch)


def test_argument_errors_launch_nothing():
    """Every pointer is a host buffer: a launch would fault, a refusal returns before anything reads them."""
    from texpose_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(16384)
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    own = dict(tp_image_down=("rgb", "rgb_out"), tp_surface_down=("zbuf", "rgb", "zbuf_out", "rgb_out"), tp_mask_down=("mask", "mask_out"))

    def filled(**kw):
        a = _lib.PyramidDownArgs()
        for k, (name, t) in enumerate(_lib.PyramidDownArgs._fields_):
            if t is C.c_void_p:
                setattr(a, name, p + 1024 * k)                   # (rgb is 2 * 4 * 6 * 3 * 4 = 576 bytes: nothing overlaps)
        for k, v in {**dict(N=2, H=4, W=6), **kw}.items():
            setattr(a, k, v)
        return a

    err = lambda: lib.tp_last_error()
    for entry, fields in own.items():
        call = lambda a: getattr(lib, entry)(C.byref(a), None)
        assert getattr(lib, entry)(None, None) == -1 and b"null args" in err()
        for bad in (dict(N=0), dict(N=65536), dict(H=1), dict(W=1), dict(H=0), dict(W=-2), dict(H=65536, W=32768)):
            assert call(filled(**bad)) == -1 and b"bad sizes" in err() and entry.encode() in err(), (entry, bad)
        for name in fields:
            assert call(filled(**{name: None})) == -1 and b"null pointer" in err(), (entry, name)
        ins, outs = [f for f in fields if not f.endswith("_out")], [f for f in fields if f.endswith("_out")]
        for o in outs:
            for i in ins:
                a = filled()
                setattr(a, o, getattr(a, i) + 16)                # the output inside the input
                assert call(a) == -1 and b"overlap" in err(), (entry, o, i)
                a = filled()
                setattr(a, i, getattr(a, o) + 4)                 # the input inside the output
                assert call(a) == -1 and b"overlap" in err(), (entry, o, i)
    a = filled()
    a.zbuf_out = a.rgb_out + 8                                   # the two outputs of tp_surface_down on each other
    assert lib.tp_surface_down(C.byref(a), None) == -1 and b"overlap" in err()


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from texpose_amd import _lib, ops, photo_align
    verts, faces, vcolor = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3)
    pose, K, im = torch.zeros(1, 3, 4), torch.eye(3), torch.zeros(1, 8, 8, 3)
    for bad in (lambda: ops.image_down(im), lambda: ops.surface_down(torch.zeros(1, 8, 8), im), lambda: ops.mask_down(torch.ones(1, 8, 8, dtype=torch.uint8)),
                lambda: ops.image_pyramid(im, 2), lambda: ops.mask_pyramid(torch.ones(1, 8, 8, dtype=torch.bool), 2)):
        with pytest.raises(ValueError, match="GPU"):
            bad()
    for pyramid in ((4, 3, 2), (10, 1), (), (5.5, 4.5), (11, -1), 10, "433"):
        with pytest.raises(ValueError, match="pyramid"):
            ops.photo_align(verts, faces, vcolor, pose, K, im, iters=10, pyramid=pyramid)
        with pytest.raises(ValueError, match="pyramid"):
            photo_align.PhotoRefiner(verts, faces, vcolor, 8, 8, "cpu", iters=10, pyramid=pyramid)
    with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
        ops.photo_align(verts, faces, vcolor, pose, K, im, iters=10, pyramid=(4, 3, 3))
    with pytest.raises(TypeError):
        ops.joint_align(verts, faces, pose, K, image=im, vcolor=vcolor, pyramid=(4, 3, 3))          # the joint loop does not take it
    assert ops.refine._pass_levels("x", (4, 3, 3), 10) == REF.pass_levels((4, 3, 3)) == [2] * 4 + [1] * 3 + [0] * 4
    assert ops.refine._pass_levels("x", (0, 2), 2) == [0, 0, 0] and ops.refine._pass_levels("x", (3,), 3) == [0] * 4


# ----------------------------------------------------------------------------- the filter
def both(**planes):
    """The restatement's and pyramid_torch's outputs of one level down -> [(name, dict)]."""
    from texpose_amd import photo_align
    ref = {}
    if "image" in planes:
        ref["image"] = REF.image_down_ref(planes["image"])
    if "zbuf" in planes:
        ref["zbuf"], ref["rgb"] = REF.surface_down_ref(planes["zbuf"], planes["rgb"])
    if "mask" in planes:
        ref["mask"] = REF.mask_down_ref(planes["mask"])
    got = photo_align.pyramid_torch(**{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in planes.items()})
    return [("restatement", ref), ("pyramid_torch", {k: v.numpy() for k, v in got.items()})]


def test_a_constant_image_stays_constant():
    for H, W in ((2, 2), (5, 7), (16, 16)):
        image = np.full((2, H, W, 3), np.float32(0.3), np.float32) * np.array([1.0, 2.0, -7.0], np.float32)
        for name, r in both(image=image, zbuf=np.full((2, H, W), 901.25, np.float32), rgb=image):
            assert r["image"].shape == (2, H // 2, W // 2, 3) and r["image"].dtype == np.float32
            assert REF.same(r["image"], image[:, :H // 2, :W // 2]), name           # (the weights add up to 1 exactly: not one bit moves)
            assert REF.same(r["rgb"], r["image"]) and (r["zbuf"] == np.float32(901.25)).all(), name


def test_a_linear_ramp_maps_to_the_ramp_at_the_coarse_centres():
    """Coarse pixel (I, J) sits at fine coordinate 2 (J + 1/2, I + 1/2), i.e. between fine pixels 2 J and 2 J + 1: away from the
    border (where taps clamp) a ramp a j + b i + c comes back as a (2 J + 1/2) + b (2 I + 1/2) + c, exactly for dyadic a, b, c.  The
    same statement gives the level's intrinsics: u_coarse = u_fine / 2 with the + .5 convention on both sides."""
    H, W = 12, 18
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ramp = (0.25 * j - 0.125 * i + 3.0).astype(np.float32)
    image = np.stack([ramp, 2 * ramp, -ramp], -1)[None]
    I, J = np.meshgrid(np.arange(H // 2), np.arange(W // 2), indexing="ij")
    want = (0.25 * (2 * J + 0.5) - 0.125 * (2 * I + 0.5) + 3.0).astype(np.float32)
    for name, r in both(image=image):
        got = r["image"][0]
        assert np.array_equal(got[1:-1, 1:-1, 0], want[1:-1, 1:-1]) and np.array_equal(got[1:-1, 1:-1, 2], -want[1:-1, 1:-1]), name
        assert np.array_equal(got[0, 1:-1, 0], want[0, 1:-1] - np.float32(0.125 * 0.125)), name   # row -1 clamps to row 0: the tap of weight 1/8 reads b 0, not b (-1)
    K = np.array([[572.4, 0.0, 80.0], [0.0, 573.6, 64.0], [0.0, 0.0, 1.0]], np.float32)
    K2 = REF.level_K(K, 2)
    assert np.array_equal(K2[:2], K[:2] * np.float32(0.25)) and np.array_equal(K2[2], K[2]) and np.array_equal(REF.level_K(K, 0), K)


def test_odd_sizes_drop_the_last_row_and_column_but_tap_them():
    """5 x 7 -> 2 x 3: coarse (1, 2) taps the rows 1 .. 4 and the columns 3 .. 6, the last of each included; by hand in the stated order."""
    rs = np.random.RandomState(2)
    image = rs.uniform(-1.0, 1.0, (1, 5, 7, 3)).astype(np.float32)
    w = [0.125, 0.375, 0.375, 0.125]
    rows, cols = [1, 2, 3, 4], [3, 4, 5, 6]
    s = [((w[0] * float(image[0, r, cols[0], 1]) + w[1] * float(image[0, r, cols[1], 1])) + w[2] * float(image[0, r, cols[2], 1]))
         + w[3] * float(image[0, r, cols[3], 1]) for r in rows]
    want = np.float32(((w[0] * s[0] + w[1] * s[1]) + w[2] * s[2]) + w[3] * s[3])
    assert REF.taps(5).tolist() == [[0, 0, 1, 2], [1, 2, 3, 4]] and REF.taps(7).tolist() == [[0, 0, 1, 2], [1, 2, 3, 4], [3, 4, 5, 6]]
    assert REF.taps(2).tolist() == [[0, 0, 1, 1]]                # the single output whose taps all clamp
    for name, r in both(image=image):
        assert r["image"].shape == (1, 2, 3, 3) and r["image"][0, 1, 2, 1] == want, name
    moved = image.copy()
    moved[0, 4, 6] += 1.0                                        # the dropped corner is a tap of (1, 2) alone
    changed = REF.image_down_ref(moved) != REF.image_down_ref(image)
    assert changed[0, 1, 2].all() and changed.sum() == 3


def test_the_surface_rule():
    """A coarse pixel is a surface iff all 16 taps have z > 0 and finite: planted -1, 0, NaN, +-Inf each take out exactly the coarse
    pixels they are a tap of; the others hold the filtered values, rgb's NaN included; off the surface z = -1 and rgb = 0."""
    rs = np.random.RandomState(3)
    H, W = 12, 16
    z = rs.uniform(880.0, 920.0, (1, H, W)).astype(np.float32)
    rgb = rs.uniform(0.0, 1.0, (1, H, W, 3)).astype(np.float32)
    planted = {(2, 3): -1.0, (5, 8): 0.0, (9, 13): np.nan, (0, 15): np.inf, (11, 0): -np.inf}
    for (i, j), v in planted.items():
        z[0, i, j] = v
    rgb[0, 6, 2, 1] = np.nan                                     # a colour, not a depth: it propagates, the pixel stays a surface
    off = np.zeros((H // 2, W // 2), bool)
    for (i, j) in planted:
        for I in range(H // 2):
            for J in range(W // 2):
                if i in REF.taps(H)[I] and j in REF.taps(W)[J]:
                    off[I, J] = True
    assert 4 * 3 + 2 <= off.sum() <= 4 * 5
    for name, r in both(zbuf=z, rgb=rgb):
        assert np.array_equal(r["zbuf"][0] == -1.0, off), name
        assert (r["rgb"][0][off] == 0.0).all() and not np.signbit(r["rgb"][0][off]).any(), name
        assert REF.same(r["zbuf"][0][~off], REF.filter_ref(z[..., None])[0, ..., 0][~off]), name
        assert REF.same(r["rgb"][0][~off], REF.filter_ref(rgb)[0][~off]), name
        assert np.isnan(r["rgb"][0][~off]).sum() == 4 and np.isfinite(r["zbuf"]).all(), name


def test_the_mask_rule():
    mask = np.ones((2, 9, 11), np.uint8)
    mask[0, 4, 5], mask[1, 0, 0], mask[1, 8, 10] = 0, 0, 0       # (row 8 and column 10 are taps of the last coarse row and column)
    mask[0, 1, 1] = 200                                          # any non-zero value counts
    for name, r in both(mask=mask):
        m = r["mask"]
        assert m.dtype == np.uint8 and m.shape == (2, 4, 5) and set(np.unique(m)) == {0, 1}, name
        assert np.argwhere(m[0] == 0).tolist() == [[1, 2], [1, 3], [2, 2], [2, 3]], name
        assert np.argwhere(m[1] == 0).tolist() == [[0, 0], [3, 4]], name


@pytest.mark.parametrize("H,W", [(2, 2), (2, 3), (5, 7), (7, 65), (16, 16), (33, 257)])
def test_pyramid_torch_equals_the_restatement(H, W):
    """On the GPU suite's planes: 60 % covered in blocks, 2 % NaN / +-Inf in every plane; bit for bit, NaN positions included."""
    c = REF.one_down_case(H * 1000 + W, 3, H, W)
    (_, want), (_, got) = both(**c)
    assert not np.isfinite(c["zbuf"]).all() and not np.isfinite(c["rgb"]).all() and not np.isfinite(c["image"]).all()
    for k in ("image", "zbuf", "rgb"):
        assert REF.same(got[k], want[k]), k
    assert np.array_equal(got["mask"], want["mask"])
    if H * W >= 7 * 65:
        assert (want["zbuf"] > 0).sum() > 20 and (want["zbuf"] == -1).sum() > 20 and np.isnan(want["image"]).any()


# ----------------------------------------------------------------------------- the identity the tests lean on
def test_the_residual_at_the_true_pose_is_exactly_zero_at_every_level():
    """photo_ref's 64 x 80 sphere: the photograph is the render over 0.5.  At the true pose every kept pixel of levels 1 and 2 has the
    same 16 values on both sides in the same arithmetic: rms == 0.0, with pixels kept.  (Where it stops, measured: level 2 of this
    size keeps 21 / 24 pixels -- too few for the loop, see the restatement's docstring.)"""
    c = dict(PR.loop_inputs("sphere", False))
    for level, floor in ((0, 500), (1, 100), (2, 15)):
        inliers, rms = REF.kept_at_level(c, c["P"], level)
        print("level %d at the true pose: kept %s, rms %s" % (level, inliers.tolist(), rms.tolist()))
        assert (inliers > floor).all() and (rms == 0.0).all()
    inliers, rms = REF.kept_at_level(c, c["start"], 2)
    assert (rms > 0.0).all() and (inliers < 30).all()


# ----------------------------------------------------------------------------- the loop's figures
@pytest.mark.parametrize("mesh,f,noisy", REF.PINNED)
def test_loop_reproduces_the_pinned_table(mesh, f, noisy):
    """The reason for the feature and its effect, on the pinned cases (the three noisy ones and the clean sphere f = 2): the pyramid
    ends every image below a quarter of its start in rotation and in translation; the plain loop leaves image 1 of the sphere cases
    above a quarter of its start in translation."""
    plain, pyr = REF.loop_case(mesh, f, noisy, pyramid=None), REF.loop_case(mesh, f, noisy)
    start, end_plain, end = REF.errors(pyr, pyr["start"]), REF.errors(plain, plain["want"]["pose"]), REF.errors(pyr, pyr["want"]["pose"])
    assert (pyr["want"]["status"] == 0).all() and (pyr["want"]["near_ties"] == 0).all()
    for b in range(2):
        (re0, te0), (re_p, te_p), (re, te) = start[b], end_plain[b], end[b]
        print("%s f = %g %s %d: %.3f deg %.3f mm -> plain %.4f deg %.4f mm | pyramid %s %.4f deg %.4f mm (kept %d at level 2, %d at the end)"
              % (mesh, f, "noisy" if noisy else "clean", b, re0, te0, re_p, te_p, REF.PYRAMID, re, te, pyr["want"]["inliers0"][b], pyr["want"]["inliers"][b]))
        assert 2.9 < re0 < 3.1 and 6.0 < te0 < 8.2
        assert re <= 0.25 * re0 and te <= 0.25 * te0
        pinned = REF.TABLE[mesh, f, noisy]
        assert np.abs(np.array([re_p, te_p]) - pinned[b]).max() <= 2e-3 and np.abs(np.array([re, te]) - pinned[2 + b]).max() <= 2e-3
    if mesh == "sphere":
        assert end_plain[1][1] > 0.25 * start[1][1]                                       # the premise
    stored = REF.golden_want(mesh, f, noisy)                                             # what the GPU suite compares against
    assert np.abs(stored["pose"] - pyr["want"]["pose"]).max() <= 1e-4 and np.array_equal(stored["near_ties"], pyr["want"]["near_ties"])
    assert np.abs(stored["inliers"] - pyr["want"]["inliers"]).max() <= 2 and np.array_equal(stored["inliers0"], pyr["want"]["inliers0"])
