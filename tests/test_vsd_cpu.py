"""CPU: the Visible Surface Discrepancy (tests/vsd_ref.py, numpy fp64) against anchors that need no library; `vsd_torch`, the CPU
route of texpose_amd/pose_error.py, against that helper; `average_recall` on hand-built arrays; the binding of K26 `tp_vsd` as
texpose_amd/_lib.py derives it from the header; tools/pose_errors.py with and without --vsd.

Helper and `vsd_torch` evaluate the same fp64 expressions in the same order, so counts AND errors are compared for equality."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import vsd_ref as V
from test_pose_error_cpu import _tool, scene  # noqa: F401  (the scene fixture: a BopSceneWriter folder and its models)
from texpose_amd import pose_error as PE

K_REAL = np.array([[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]], np.float32)
H, W = 12, 16


def k_flat(cx=0.0, cy=0.0):
    """fx = fy = 2^40: u^2 + v^2 + 1 rounds to 1, so f = 1 exactly and D = z."""
    return np.array([[2.0 ** 40, 0.0, cx], [0.0, 2.0 ** 40, cy], [0.0, 0.0, 1.0]], np.float32)


def plane(value=-1.0, rect=None, inside=None):
    z = np.full((1, H, W), value, np.float32)
    if rect is not None:
        r0, r1, c0, c1 = rect
        z[0, r0:r1, c0:c1] = inside
    return z


TAUS = np.array([[5.0, 10.0, 20.0, 40.0]], np.float32)


# ----------------------------------------------------------------------------- the helper against library-free anchors
def test_identical_planes_fully_visible_give_zero():
    z = plane(rect=(2, 9, 3, 12), inside=700.0)
    r = V.vsd_ref(z, z, z, K_REAL, TAUS)
    assert r["counts"][0].tolist() == [63, 63, 0, 0, 0, 0] and (r["err"] == 0).all()


def test_offset_patch_at_the_principal_point_steps_at_s_f():
    s = 12.0
    rect = (4, 8, 6, 10)                                     # 4 x 4 pixels around (cx, cy) = (8, 6)
    K = np.array([[600.0, 0.0, 8.0], [0.0, 600.0, 6.0], [0.0, 0.0, 1.0]], np.float32)
    zg = plane(rect=rect, inside=800.0)
    ze = plane(rect=rect, inside=800.0 + s)
    f_max = math.sqrt(2 * (1.5 / 600.0) ** 2 + 1)           # the corner pixels' centres are 1.5 px from the principal point
    taus = np.array([[1.0, s * 0.999999, s, s * f_max * 1.000001, 50.0]], np.float32)
    r = V.vsd_ref(ze, zg, zg, K, taus)
    assert r["counts"][0, :2].tolist() == [16, 16]
    assert r["err"][0].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0]          # (tau = s itself: every f >= 1, so s f >= s)


def test_test_depth_in_front_of_both_hides_everything():
    zg, ze = plane(rect=(2, 9, 3, 12), inside=700.0), plane(rect=(3, 10, 2, 11), inside=710.0)
    r = V.vsd_ref(ze, zg, plane(600.0), K_REAL, TAUS, delta_mm=15.0)
    assert r["counts"][0].tolist() == [0] * 6 and (r["err"] == 1).all()


def test_disjoint_silhouettes_give_one():
    zg, ze = plane(rect=(1, 5, 1, 6), inside=700.0), plane(rect=(6, 11, 8, 15), inside=700.0)
    r = V.vsd_ref(ze, zg, plane(700.0), K_REAL, TAUS)
    assert r["counts"][0, :2].tolist() == [20 + 35, 0] and (r["err"] == 1).all()


def test_a_missing_test_depth_counts_as_visible():
    z = plane(rect=(2, 9, 3, 12), inside=700.0)
    for hole in (0.0, -3.0, np.nan):                         # the test depth would hide the models; a hole does not
        r = V.vsd_ref(z, z, plane(hole), K_REAL, TAUS)
        assert r["counts"][0, :2].tolist() == [63, 63] and (r["err"] == 0).all(), hole
    assert V.vsd_ref(z, z, plane(100.0), K_REAL, TAUS)["counts"][0, 0] == 0


def test_an_estimate_hidden_where_ground_truth_is_visible_is_in_v_est():
    rect = (2, 9, 3, 12)
    zg, ze = plane(rect=rect, inside=700.0), plane(rect=rect, inside=800.0)          # 100 mm behind the measured surface: hidden by itself
    r = V.vsd_ref(ze, zg, zg, k_flat(), np.array([[99.0, 100.0, 101.0]], np.float32), delta_mm=15.0)
    assert r["counts"][0].tolist() == [63, 63, 63, 63, 0] and r["err"][0].tolist() == [1.0, 1.0, 0.0]
    # without a visible ground truth under it the same estimate is in no set
    r = V.vsd_ref(ze, plane(), zg, k_flat(), TAUS)
    assert r["counts"][0, :2].tolist() == [0, 0] and (r["err"] == 1).all()


def test_two_overlapping_rectangles_counted_by_hand():
    zg = plane(rect=(2, 6, 2, 8), inside=500.0)              # 4 x 6 = 24
    ze = plane(rect=(4, 8, 5, 11), inside=520.0)             # 4 x 6 = 24, 2 x 3 = 6 shared
    ze[0, 0, 0] = np.nan                                     # a NaN is background
    r = V.vsd_ref(ze, zg, plane(0.0), k_flat(), np.array([[10.0, 20.0, 30.0]], np.float32))
    assert r["counts"][0].tolist() == [42, 6, 6, 6, 0]
    assert r["err64"][0].tolist() == [42 / 42, 42 / 42, 36 / 42]
    # a measured surface at 505 mm and delta 15: both rectangles stay visible at equality (520 - 505 <= 15); at 504 the estimate's
    # own pixels are hidden and only the shared ones remain in V_est
    assert V.vsd_ref(ze, zg, plane(505.0), k_flat(), TAUS, delta_mm=15.0)["counts"][0, :2].tolist() == [42, 6]
    assert V.vsd_ref(ze, zg, plane(504.0), k_flat(), TAUS, delta_mm=15.0)["counts"][0, :2].tolist() == [24, 6]
    assert r["near_ties"][0] == 6                            # |520 - 500| against tau = 20 on the shared pixels


# ----------------------------------------------------------------------------- vsd_torch against the helper
def random_case(seed, B, Ft, T, h=37, w=53, flat=False):
    rs = np.random.RandomState(seed)
    zg = rs.randint(200, 1201, (B, h, w)).astype(np.float32) if flat else rs.uniform(600, 900, (B, h, w)).astype(np.float32)
    ze = (zg + rs.randint(-30, 31, zg.shape)).astype(np.float32) if flat else (zg + rs.normal(0, 15, zg.shape)).astype(np.float32)
    dt = (zg[np.arange(Ft) % B] + rs.randint(-30, 31, (Ft, h, w))).astype(np.float32)
    for a, share in ((zg, 0.3), (ze, 0.3), (dt, 0.1)):
        a[rs.uniform(size=a.shape) < share] = 0.0 if a is dt else -1.0
    ze[rs.uniform(size=ze.shape) < 0.02] = np.nan
    dt[rs.uniform(size=dt.shape) < 0.02] = np.nan
    K = np.tile(k_flat() if flat else K_REAL, (B, 1, 1))
    if not flat:
        K[:, 0, 2], K[:, 1, 2] = w / 2 + rs.uniform(-3, 3, B), h / 2 + rs.uniform(-3, 3, B)
    tau = (rs.randint(1, 31, (B, T)) if flat else rs.uniform(2, 40, (B, T))).astype(np.float32)
    return ze, zg, dt, K, tau


@pytest.mark.parametrize("B,Ft,T,flat,frame", [(3, 3, 10, False, None), (3, 1, 1, False, None), (4, 2, 16, True, [1, 0, 1, 1]),
                                               (2, 2, 5, True, None), (2, 3, 4, False, [7, -2])])
def test_vsd_torch_equals_the_helper(B, Ft, T, flat, frame):
    ze, zg, dt, K, tau = random_case(B * 100 + T, B, Ft, T, flat=flat)
    want = V.vsd_ref(ze, zg, dt, K, tau, delta_mm=15.0, frame=frame)
    t = torch.from_numpy
    got = PE.vsd_torch(t(ze), t(zg), t(dt), t(K), t(tau), 15.0, None if frame is None else torch.tensor(frame))
    assert got["counts"].dtype == torch.int32 and got["err"].dtype == torch.float32
    assert want["counts"][:, 0].min() > 100
    assert np.array_equal(got["counts"].numpy(), want["counts"])
    assert np.array_equal(got["err"].numpy(), want["err"])


def test_vsd_from_depth_on_cpu_tensors():
    ze, zg, dt, K, _ = random_case(5, 3, 3, 1)
    t = torch.from_numpy
    d = torch.tensor([100.0, 120.0, 80.0])
    got = PE.vsd_from_depth(t(ze), t(zg), t(dt), t(K), d)
    tau = (np.array(PE.BOP19_TAUS, np.float32)[None] * d.numpy()[:, None]).astype(np.float32)
    want = V.vsd_ref(ze, zg, dt, K, tau)
    assert got["err"].shape == (3, 10) and np.array_equal(got["counts"].numpy(), want["counts"]) and np.array_equal(got["err"].numpy(), want["err"])
    one = PE.vsd_from_depth(t(ze), t(zg), t(dt[:1]), t(K[0]), 100.0, taus=(0.1, 0.3), delta=10.0)       # a float, one intr, one plane
    want = V.vsd_ref(ze, zg, dt[:1], K[0], np.tile(np.array([[0.1, 0.3]], np.float32) * np.float32(100.0), (3, 1)), delta_mm=10.0)
    assert np.array_equal(one["counts"].numpy(), want["counts"])
    with pytest.raises(ValueError):
        PE.vsd_from_depth(t(ze), t(zg), t(dt), t(K), 100.0, taus=[0.1] * 17)
    with pytest.raises(ValueError, match="no CPU route"):
        PE.vsd(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, 3, 4), torch.zeros(1, 3, 4), t(K[0]), t(dt[:1]), 100.0, H=37, W=53)


def test_depth_from_png_and_constants():
    d16 = np.array([[0, 1, 65535]], np.uint16)
    mm = PE.depth_from_png(d16, 0.5)
    assert mm.dtype == torch.float32 and mm.tolist() == [[0.0, 0.5, 32767.5]]
    assert PE.depth_from_png(torch.tensor([[7]], dtype=torch.int32), 2.0).tolist() == [[14.0]]
    want = [0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5]
    assert list(PE.BOP19_TAUS) == want and list(PE.BOP19_THRESHOLDS) == want


# ----------------------------------------------------------------------------- the average recall
def test_average_recall_on_hand_built_arrays():
    G = 4
    zero = PE.average_recall(torch.zeros(G, 10), torch.zeros(G), torch.zeros(G), 100.0, 640)
    assert zero == dict(ar_vsd=1.0, ar_mssd=1.0, ar_mspd=1.0, ar=1.0)
    gone = PE.average_recall(torch.zeros(G, 10), torch.zeros(G), torch.zeros(G), 100.0, 640, valid=[False] * G)
    assert gone == dict(ar_vsd=0.0, ar_mssd=0.0, ar_mspd=0.0, ar=0.0)
    nan = PE.average_recall(torch.full((G, 10), math.nan), [math.nan] * G, [math.nan] * G, torch.full((G,), 100.0), 640)
    assert nan == gone
    # one instance of two straddles: err 0.3 passes theta in {0.35 .. 0.5} (4 of 10), mssd 22 of diameter 100 passes theta >= 0.25 (6 of
    # 10), mspd 12 px at width 1280 (thresholds 10, 20 .. 100) passes 9 of 10; `<` is strict: err 0.3 fails theta = 0.3
    r = PE.average_recall([[0.0] * 10, [0.3] * 10], [0.0, 22.0], [0.0, 12.0], [50.0, 100.0], 1280)
    assert r["ar_vsd"] == pytest.approx((1.0 + 0.4) / 2) and r["ar_mssd"] == pytest.approx((1.0 + 0.6) / 2)
    assert r["ar_mspd"] == pytest.approx((1.0 + 0.9) / 2) and r["ar"] == pytest.approx((0.7 + 0.8 + 0.95) / 3)
    half = PE.average_recall(torch.zeros(2, 10), [0.0, 0.0], [0.0, 0.0], 100.0, 640, valid=torch.tensor([True, False]))
    assert half["ar"] == 0.5


# ----------------------------------------------------------------------------- the binding
def test_binding_of_tp_vsd_is_derived_from_the_header():
    from texpose_amd import _lib
    assert "tp_vsd" in _lib.SYMBOLS
    assert _lib.VSD_MAX_TAUS == 16 and _lib.TP_VSD_MAX_TAUS == 16
    assert _lib.ABI_VERSION == 16                            # the declaration adds to the ABI and changes nothing in it
    fields = _lib.VsdArgs._fields_
    assert [n for n, _ in fields] == ["z_est", "z_gt", "depth_test", "frame", "intr", "tau_mm", "delta_mm", "B", "Ft", "H", "W", "T", "counts", "err"]
    assert C.sizeof(_lib.VsdArgs) == sum(C.sizeof(t) for _, t in fields)          # no padding: the layout is the field list
    restype, argtypes = _lib.HEADER.prototypes["tp_vsd"]
    assert restype is C.c_int and argtypes[0]._type_ is _lib.VsdArgs


def test_library_refuses_bad_vsd_arguments_without_a_gpu():
    from texpose_amd import _lib, ops
    lib = _lib.load()
    a = _lib.VsdArgs()
    dummy = C.c_double()
    for f in ("z_est", "z_gt", "depth_test", "intr", "tau_mm", "counts", "err"):
        setattr(a, f, C.addressof(dummy))
    a.B, a.Ft, a.H, a.W = 2, 2, 4, 4
    for T in (0, 17):
        a.T = T
        assert lib.tp_vsd(C.byref(a), None) == -1 and b"1 .. 16" in lib.tp_last_error()
    a.T, a.Ft = 10, 3
    assert lib.tp_vsd(C.byref(a), None) == -1 and b"neither 1 nor B" in lib.tp_last_error()
    a.Ft, a.W = 2, 0
    assert lib.tp_vsd(C.byref(a), None) == -1 and b"bad sizes" in lib.tp_last_error()
    a.W, a.err = 4, None
    assert lib.tp_vsd(C.byref(a), None) == -1 and b"null pointer" in lib.tp_last_error()
    with pytest.raises(_lib.TexposeLibraryError):
        ops.vsd(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.eye(3), torch.ones(1, 3))


# ----------------------------------------------------------------------------- the tool
KEYS_WITHOUT_VSD = ["object", "vertices", "symmetries", "diameter", "poses", "missing", "frames", "errors"] + \
    [s + k for k in ("add", "adds", "mssd", "mspd", "proj", "re", "te") for s in ("mean_", "median_")] + \
    ["recall_add_0.1", "recall_adds_0.1", "recall_add_0.02", "recall_adds_0.02", "recall_add_0.05", "recall_adds_0.05", "recall_proj_5px",
     "recall_50mm_5deg", "failed_add"]


def test_tool_vsd_on_the_cpu_exits_with_a_message(scene, capsys):  # noqa: F811
    with pytest.raises(SystemExit) as e:
        _tool().main(["--gt", scene["root"], "--est", scene["root"], "--device", "cpu", "--vsd"] + scene["ply_args"])
    assert e.value.code not in (0, None) and "--vsd" in str(e.value.code) and "no CPU route" in str(e.value.code)
    assert capsys.readouterr().out == ""                     # nothing was scored first


def test_tool_without_vsd_is_unchanged(scene, capsys):  # noqa: F811
    out = str(scene["tmp"] / "report.json")
    _tool().main(["--gt", scene["root"], "--est", scene["root"], "--device", "cpu", "--json", out] + scene["ply_args"])
    table = capsys.readouterr().out.splitlines()
    assert len(table[0].split()) == 3 + 14 + 8               # no VSD and no AR column
    saved = json.load(open(out))
    assert sorted(saved) == ["device", "est", "gt", "objects"]
    for row in saved["objects"]:
        assert list(row) == KEYS_WITHOUT_VSD and sorted(row["errors"]) == sorted(["add", "adds", "mssd", "mspd", "proj", "re", "te"])
