"""K42 (tp_robust_weight) and the robust fit without a GPU: the restated radix select against a sort, the robust loop on the corrupted round
trip against the recorded figures, and the library's symbols, struct fields and refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import face_texel_fit_ref as FIT
import robust_weight_ref as RW
import test_face_texel_fit_cpu as K36T                  # the round trip, as it is
import test_face_texels_cpu as K35T
import texture_bake_ref as TREF
from texpose_amd import _lib
from texpose_amd import texture_bake as TB

SIZE, R = 64, 4


# ---- the select
def lower_median(q):
    return np.sort(q)[(len(q) - 1) // 2]


def select_inputs():
    rs = np.random.RandomState(0)
    yield "random", (rs.rand(5001).astype(np.float32) ** 4)
    yield "random, even n", rs.rand(4096).astype(np.float32)
    yield "wide range", np.exp(rs.uniform(-80, 80, 3000)).astype(np.float32)
    yield "with zeros and denormals", np.concatenate([np.zeros(40, np.float32), np.full(30, 1e-42, np.float32), rs.rand(50).astype(np.float32)])
    yield "all equal", np.full(1000, 0.37, np.float32)
    yield "all zero", np.zeros(77, np.float32)
    for share in (0.3, 0.5, 0.7):
        yield "two values %.1f" % share, np.where(rs.rand(1001) < share, np.float32(0.25), np.float32(3.5)).astype(np.float32)
    yield "two values, even split", np.array([2.0, 1.0] * 8, np.float32)
    for n in (1, 2, 3):
        yield "n = %d" % n, rs.rand(n).astype(np.float32)
    low = (np.float32(0.0123).view(np.uint32) & ~np.uint32(1023)) | rs.randint(0, 1024, 999).astype(np.uint32)
    yield "lowest 10 bits", low.view(np.float32)
    yield "lowest 10 bits, few", low[:7].view(np.float32)
    mid = (np.float32(0.0123).view(np.uint32) & ~np.uint32((1 << 21) - 1)) | rs.randint(0, 1 << 21, 999).astype(np.uint32)
    yield "lowest 21 bits", mid.view(np.float32)


@pytest.mark.parametrize("name,q", list(select_inputs()), ids=[n for n, _ in select_inputs()])
def test_radix_select_is_the_lower_median(name, q):
    got, bins = RW.radix_select(q)
    want = lower_median(q)
    assert got.dtype == np.float32 and got.view(np.uint32) == want.view(np.uint32), (name, got, want)
    key = int(want.view(np.uint32))
    assert bins == (key >> 21, (key >> 10) & 2047, key & 1023)


def test_radix_select_finds_every_rank():
    q = np.random.RandomState(1).rand(257).astype(np.float32) ** 3
    order = np.sort(q)
    assert all(RW.radix_select(q, k)[0] == order[k] for k in range(len(q)))
    assert RW.radix_select(np.zeros(0, np.float32))[0] == 0


def test_rule_on_planted_planes():
    """counted pixels, the median over them, sigma's floor, scale_in, and both weight functions on a plane small enough to do by hand"""
    model = np.zeros((2, 2, 3, 3), np.float32)
    image = np.zeros((2, 2, 3, 3), np.float32)
    image[0, :, :, 0] = [[0.1, 0.2, 0.3], [0.4, 0.5, np.nan]]
    image[0, 1, 1, 2] = np.inf
    weight = np.ones((2, 2, 3), np.float32)
    weight[0, 0, 0], weight[1] = -1.0, 0.0
    out = RW.robust_weight_ref(model, image, weight)
    assert out["count"].tolist() == [3, 0] and out["median_q"][1] == 0 and out["scale"][1] == RW.SIGMA_MIN
    q = (np.array([0.2, 0.3, 0.4], np.float32).astype(np.float64) ** 2 / 3.0).astype(np.float32)
    assert out["median_q"][0] == q[1] and abs(out["scale"][0] - 1.4826 * 0.3 / np.sqrt(3)) < 1e-7
    u2 = q.astype(np.float64) / (4.685 ** 2 * 1.4826 ** 2 * q[1])
    want = np.zeros((2, 3), np.float32)
    want[0, 1], want[0, 2], want[1, 0] = ((1 - u2) ** 2).astype(np.float32)
    assert np.allclose(out["weight"][0], want, rtol=1e-6, atol=0) and not out["weight"][1].any()
    given = RW.robust_weight_ref(model, image, weight, RW.HUBER, scale_in=np.array([0.1, 0.0], np.float32))
    assert given["count"].tolist() == [3, 0] and not given["median_q"].any() and given["scale"].tolist() == [np.float32(0.1), RW.SIGMA_MIN]
    u = np.sqrt(q.astype(np.float64)) / (1.345 * np.float64(np.float32(0.1)))
    assert np.allclose(given["weight"][0, [0, 0, 1], [1, 2, 0]], np.where(u <= 1, 1.0, 1.0 / u), rtol=1e-6)


# ---- the robust loop on the corrupted round trip
@functools.lru_cache(maxsize=None)
def robust_case(name):
    """Section 26's shrunk round trip with the issue's corruption painted into the photographs ('corrupted'), with sigma = 0.02 noise on
    every pixel besides ('noisy'), or as it is ('clean') -> the photographs, the views, their bake and the default weights."""
    c, _ = K36T.round_trip(R, SIZE, 200.0)
    covered = c["face"] >= 0
    rgb = np.asarray(c["rgb"], np.float32) if name == "clean" else RW.corrupt(c["rgb"], covered, noise=0.02 if name == "noisy" else 0.0)
    _, _, vs, fs, ni = K35T.subdivided("sphere", R)
    bake, _ = TREF.vcolor_of(TREF.bake(vs, TB.vertex_normals(vs, fs), c["poses"], c["K"], rgb, c["zbuf"])["acc"])
    weight = FIT.inner_coverage(c["face"], len(c["faces"])).astype(np.float32)
    views = FIT.Views(c["face"], c["verts"], c["faces"], c["poses"], c["K"], SIZE, SIZE, R, ni, len(vs), rgb, weight)
    return dict(c=c, rgb=rgb, weight=weight, views=views, bake=bake, node_index=ni, U=len(vs))


def held_out(case, nodes):
    return K36T.held_out_psnr(case["c"], case["node_index"], np.asarray(nodes, np.float64), SIZE)


@functools.lru_cache(maxsize=None)
def measure(name):
    case = robust_case(name)
    plain = FIT.fit_loop(case["views"], case["bake"], case["bake"], RW.LAM, RW.ITERS)
    robust = RW.robust_fit_loop(case["views"], case["rgb"], case["weight"], case["bake"], case["bake"])
    return dict(plain=plain, robust=robust, figures=(held_out(case, case["bake"]), held_out(case, plain["nodes"]), held_out(case, robust["nodes"])))


@pytest.mark.parametrize("name", ["corrupted", "noisy"])
def test_robust_fit_beats_the_plain_fit_on_corrupted_photographs(name):
    case, m = robust_case(name), measure(name)
    psnr_bake, psnr_plain, psnr_robust = m["figures"]
    want = RW.ROBUST_FIT[name]
    share = RW.corrupted_share(case["c"]["rgb"], case["rgb"], case["weight"])
    print("corrupted round trip %s: held-out PSNR bake %.2f dB, plain fit %.2f dB, Tukey %d x %d %.2f dB | recorded %s; corrupted share per view "
          "%.3f .. %.3f; kept %s" % (name, psnr_bake, psnr_plain, RW.ROUNDS, RW.ITERS, psnr_robust, want, share.min(), share.max(),
                                     np.round(m["robust"]["kept"], 3).tolist()))
    print("  rms series:", np.round(m["robust"]["rms"], 5).tolist())
    assert (share < 0.25).all() and share.max() > 0.05                 # far below the median's breakdown, and there is something to reject
    assert want[2] > want[1] and psnr_robust - psnr_plain >= 0.5 * (want[2] - want[1])
    assert psnr_robust >= want[2] - 1.0 and abs(psnr_plain - want[1]) <= 0.05 and abs(psnr_bake - want[0]) <= 0.05
    assert m["robust"]["rms"].shape == (RW.ROUNDS * RW.ITERS + 1,)
    assert (m["robust"]["count"] == (case["weight"] > 0).sum((1, 2))).all() and (m["robust"]["kept"] < 0.95).all()
    g = dict(np.load(RW.GOLDEN))
    np.testing.assert_allclose(g[name], want, rtol=0, atol=1e-12)      # the file and the table say the same
    if name == "corrupted":
        np.testing.assert_allclose(g["by_round"], RW.ROBUST_FIT_BY_ROUND, rtol=0, atol=1e-12)
        np.testing.assert_allclose(g["scale"], RW.ROBUST_FIT_SCALE, rtol=0, atol=1e-12)
        np.testing.assert_allclose(m["robust"]["scale"], RW.ROBUST_FIT_SCALE, rtol=1e-3)
        by_round = [held_out(case, RW.robust_fit_loop(case["views"], case["rgb"], case["weight"], case["bake"], case["bake"], rounds=k)["nodes"])
                    for k in (1, 3)]
        print("  after rounds 1 and 3: %.2f, %.2f dB | recorded %s" % (by_round[0], by_round[1], RW.ROBUST_FIT_BY_ROUND))
        assert abs(by_round[0] - RW.ROBUST_FIT_BY_ROUND[0]) <= 0.1 and abs(by_round[1] - RW.ROBUST_FIT_BY_ROUND[2]) <= 0.1


def test_robust_fit_does_not_hurt_on_clean_photographs():
    m = measure("clean")
    _, psnr_plain, psnr_robust = m["figures"]
    want = RW.ROBUST_FIT["clean"]
    print("uncorrupted round trip: held-out PSNR plain fit %.2f dB, Tukey %.2f dB | recorded %s" % (psnr_plain, psnr_robust, want))
    assert abs(psnr_robust - psnr_plain) <= 0.1 and abs(psnr_plain - FIT.ROUND_TRIP_SMALL[R][1]) <= 0.05
    np.testing.assert_allclose(dict(np.load(RW.GOLDEN))["clean"], want, rtol=0, atol=1e-12)


# ---- the library without a device
def test_symbols_and_refusals_without_a_gpu():
    assert _lib.ABI_VERSION == 16
    assert "tp_robust_weight" in _lib.SYMBOLS and "tp_robust_weight_workspace_bytes" in _lib.SYMBOLS
    assert (_lib.ROBUST_TUKEY, _lib.ROBUST_HUBER) == (0, 1)
    assert [f[0] for f in _lib.RobustWeightArgs._fields_] == ["model", "image", "weight", "scale_in", "B", "H", "W", "kind", "c", "sigma_min", "out",
                                                              "median_q", "scale", "count", "workspace"]
    lib = _lib.load()
    per_image = 4 * (2048 + 2048 + 1024) + 32
    assert lib.tp_robust_weight_workspace_bytes(3, 33, 257) == (4 * 3 * 33 * 257 + 15) // 16 * 16 + 3 * per_image
    assert lib.tp_robust_weight_workspace_bytes(1, 1, 1) == 16 + per_image and lib.tp_robust_weight_workspace_bytes(2, 64, 80) == 4 * 2 * 64 * 80 + 2 * per_image
    assert lib.tp_robust_weight_workspace_bytes(0, 4, 4) == 0 and lib.tp_robust_weight_workspace_bytes(1, -1, 4) == 0
    assert lib.tp_robust_weight(None, None) == -1 and b"tp_robust_weight: null args" in lib.tp_last_error()
    # addresses that are never dereferenced (every case is refused), 1 MiB apart so that nothing overlaps by accident
    names = ("model", "image", "weight", "scale_in", "out", "median_q", "scale", "count", "workspace")
    good = dict({n: (i + 1) << 20 for i, n in enumerate(names)}, B=2, H=8, W=8, kind=_lib.ROBUST_TUKEY, c=4.685, sigma_min=1.0 / 255.0)

    def refused(text, **change):
        a = _lib.RobustWeightArgs()
        for k, v in {**good, **change}.items():
            setattr(a, k, v)
        return lib.tp_robust_weight(C.byref(a), None) == -1 and b"tp_robust_weight" in lib.tp_last_error() and text in lib.tp_last_error()

    for k in ("B", "H", "W"):
        assert refused(b"bad sizes", **{k: 0}) and refused(b"bad sizes", **{k: -1}), k
    assert refused(b"bad sizes", B=65536) and refused(b"bad sizes", H=1 << 16, W=1 << 15)
    for k in ("model", "image", "out", "median_q", "scale", "count"):
        assert refused(b"null pointer", **{k: None}), k
    assert refused(b"null pointer", workspace=None, scale_in=None)            # (with scale_in no workspace is needed)
    assert refused(b"unknown kind", kind=2) and refused(b"unknown kind", kind=-1)
    for k in ("c", "sigma_min"):
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert refused(b": %s must be finite and > 0" % k.encode(), **{k: bad}), (k, bad)
    assert refused(b"16-byte aligned", workspace=good["workspace"] + 8, scale_in=None)
    planes, px, per = 2 * 8 * 8 * 12, 2 * 8 * 8 * 4, 8
    ws = 4 * 2 * 8 * 8 + 2 * per_image
    inputs = (("model", planes), ("image", planes), ("weight", px), ("scale_in", per))
    for out, size in (("out", px), ("median_q", per), ("scale", per), ("count", per)):
        for inp, isize in inputs:
            assert refused(b"overlaps", **{out: good[inp] + isize - 4}), (out, inp)          # the input's last word
            assert refused(b"overlaps", **{out: good[inp] - size + 4}), (out, inp)           # its first
    for inp, isize in inputs[:3]:                                                             # the workspace (used without scale_in)
        assert refused(b"overlaps", workspace=good[inp] + (isize - 4) // 16 * 16, scale_in=None), inp
        assert refused(b"overlaps", workspace=good[inp] - ws + 16, scale_in=None), inp
    assert refused(b"overlaps", median_q=good["out"] + px - 4) and refused(b"overlaps", scale=good["median_q"] + 4)
    assert refused(b"overlaps", count=good["scale"]) and refused(b"overlaps", workspace=good["out"], scale_in=None)
    assert refused(b"overlaps", workspace=good["count"] - ws + 16, scale_in=None)
