"""No GPU: the numpy restatement of K31c / K32 (tests/occlusion_ref.py) against facts done by hand, `silhouette.sdf_torch(mask, known)`
and `silhouette.known_from_others_torch` against the restatement, the host side of the two new entry points (the header-derived
binding and the argument checks, which launch nothing), and the restatement's loop on occluded masks, which regenerates the table of
DESIGN section 22."""
import ctypes as C

import numpy as np
import pytest
import torch

import occlusion_ref as OREF
import silhouette_ref as REF


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- the binding and the argument checks
def test_binding_has_the_two_new_entry_points():
    from texpose_amd import _lib
    assert _lib.ABI_VERSION == 16
    for name in ("tp_mask_sdf_known", "tp_mask_known_from_others"):
        assert name in _lib.SYMBOLS
    restype, argtypes = _lib.HEADER.prototypes["tp_mask_sdf_known"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    restype, argtypes = _lib.HEADER.prototypes["tp_mask_known_from_others"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p]
    assert C.sizeof(_lib.SilhouetteAlignArgs) == 136 and len(_lib.SilhouetteAlignArgs._fields_) == 20          # (no struct is touched)
    lib = _lib.load()
    assert hasattr(lib, "tp_mask_sdf_known") and hasattr(lib, "tp_mask_known_from_others")
    assert lib.tp_abi_version() == 16


def _aligned_buffer(n):
    buf = C.create_string_buffer(n + 16)
    return buf, C.addressof(buf) + (-C.addressof(buf)) % 16


def test_sdf_known_argument_errors_launch_nothing():
    """Every pointer is a host buffer: a launch would fault, a refusal returns before anything reads them."""
    from texpose_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer(8192)
    err = lambda: lib.tp_last_error()
    mask, known, sdf, ws = p, p + 512, p + 1024, p + 4096
    for F, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 8193, 4), (1, 4, 8193), (32, 8192, 8192), (2 ** 20, 64, 32)):
        assert lib.tp_mask_sdf_known(mask, known, sdf, F, H, W, ws, None) == -1 and b"bad sizes" in err(), (F, H, W)
        assert b"tp_mask_sdf_known" in err()
    for args in ((None, known, sdf, ws), (mask, None, sdf, ws), (mask, known, None, ws), (mask, known, sdf, None)):
        assert lib.tp_mask_sdf_known(args[0], args[1], args[2], 2, 4, 4, args[3], None) == -1 and b"null pointer" in err()
    assert lib.tp_mask_sdf_known(mask, known, sdf, 2, 4, 4, ws + 8, None) == -1 and b"aligned" in err()
    for m, s in ((p, p), (p + 16, p), (p, p + 31), (p + 127, p)):          # mask 32 bytes, sdf 128 bytes
        assert lib.tp_mask_sdf_known(m, p + 2048, s, 2, 4, 4, ws, None) == -1 and b"overlap mask" in err(), (m - p, s - p)
    for k, s in ((p, p), (p + 16, p), (p, p + 31), (p + 127, p)):          # known 32 bytes, sdf 128 bytes
        assert lib.tp_mask_sdf_known(p + 2048, k, s, 2, 4, 4, ws, None) == -1 and b"overlap known" in err(), (k - p, s - p)


def test_known_from_others_argument_errors_launch_nothing():
    from texpose_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer(8192)
    err = lambda: lib.tp_last_error()
    sdf, known = p, p + 4096
    band = C.c_float(1.0)
    for N, H, W in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (65536, 4, 4), (32, 8192, 8192), (2 ** 15, 2 ** 8, 2 ** 8)):
        assert lib.tp_mask_known_from_others(sdf, known, N, H, W, band, None) == -1 and b"bad sizes" in err(), (N, H, W)
    for a, b in ((None, known), (sdf, None)):
        assert lib.tp_mask_known_from_others(a, b, 2, 4, 4, band, None) == -1 and b"null pointer" in err()
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), float("-inf")):
        assert lib.tp_mask_known_from_others(sdf, known, 2, 4, 4, C.c_float(bad), None) == -1 and b"band_px" in err(), bad
    for k, s in ((p, p), (p + 16, p), (p, p + 31), (p + 127, p)):          # known 32 bytes, sdf 128 bytes
        assert lib.tp_mask_known_from_others(s, k, 2, 4, 4, band, None) == -1 and b"overlap" in err(), (k - p, s - p)


def test_ops_refuse_cpu_tensors():
    from texpose_amd import _lib, ops
    m = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
        ops.mask_sdf(m, known=torch.ones_like(m))
    with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
        ops.mask_known_from_others(torch.zeros(2, 4, 4))


# ----------------------------------------------------------------------------- the field
def test_a_plane_done_by_hand():
    """3 x 5: one set pixel at (1, 1), column 2 unknown.  Distances to SET and CLEAR pixels pass over the unknown column; nothing
    measures a distance TO it."""
    m = np.zeros((3, 5), np.uint8)
    m[1, 1] = 7
    m[0, 2] = 9                                                  # (unknown: whatever mask holds)
    k = np.ones((3, 5), np.uint8)
    k[:, 2] = 0
    to_set, to_clear = OREF.d2_known_ref(m, k)
    assert to_set.tolist() == [[2, 1, 2, 5, 10], [1, 0, 1, 4, 9], [2, 1, 2, 5, 10]]
    assert to_clear.tolist() == [[0, 0, 1, 0, 0], [0, 1, 1, 0, 0], [0, 0, 1, 0, 0]]
    s = OREF.sdf_known_ref(m, k)
    assert s.dtype == np.float32 and np.array_equal(np.isnan(s), k == 0)
    assert s[1, 1] == -0.5 and s[1, 0] == 0.5 and s[1, 3] == 1.5 and s[0, 0] == np.float32(np.sqrt(np.float32(2.0))) - np.float32(0.5)
    # today's field of the same mask sees (0, 2) as set: (0, 3) is next to it there, and sqrt(1 + 4) from the set pixel here
    assert REF.sdf_ref(m)[0, 3] == 0.5 and s[0, 3] == np.float32(np.sqrt(np.float32(5.0))) - np.float32(0.5)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (2, 5), (9, 13)])
def test_sdf_torch_with_known_equals_the_restatement(H, W):
    from texpose_amd import silhouette
    rs = np.random.RandomState(H * 100 + W)
    masks = np.stack([rs.uniform(size=(H, W)) < 0.5, rs.uniform(size=(H, W)) < 0.1, np.zeros((H, W), bool), np.ones((H, W), bool)])
    masks = masks.astype(np.uint8) * np.uint8(255)
    t = torch.from_numpy
    # 30 % unknown
    known = (rs.uniform(size=masks.shape) >= 0.3).astype(np.uint8) * rs.choice(np.array([1, 7, 255], np.uint8), masks.shape)
    want = OREF.sdf_known_ref(masks, known)
    got = silhouette.sdf_torch(t(masks), t(known)).numpy()
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert np.array_equal(np.isnan(want), known == 0) and np.array_equal(want < 0, (masks != 0) & (known != 0))
    assert np.array_equal(bits(silhouette.sdf_torch(t(masks[0]), t(known[0] != 0)).numpy()), bits(want[0]))          # one plane, bool
    # all known: today's field
    ones = np.ones_like(masks)
    plain = REF.sdf_ref(masks)
    assert np.array_equal(bits(OREF.sdf_known_ref(masks, ones)), bits(plain))
    assert np.array_equal(bits(silhouette.sdf_torch(t(masks), t(ones)).numpy()), bits(plain))
    assert np.array_equal(bits(silhouette.sdf_torch(t(masks)).numpy()), bits(plain))
    # all unknown: all NaN
    assert np.isnan(OREF.sdf_known_ref(masks, 0 * ones)).all() and np.isnan(silhouette.sdf_torch(t(masks), t(0 * ones)).numpy()).all()
    with pytest.raises(ValueError):
        silhouette.sdf_torch(t(masks), t(known[:1]))


def test_the_sentinel_is_reached_across_an_unknown_column():
    """Set pixels left of an unknown column, clear ones right of it: real distances pass over it.  Then with the clear side unknown
    too, the set pixels have no clear pixel at all: the sentinel."""
    from texpose_amd import silhouette
    H, W = 4, 7
    m = np.zeros((H, W), np.uint8)
    m[:, :3] = 1
    k = np.ones((H, W), np.uint8)
    k[:, 3] = 0
    s = OREF.sdf_known_ref(m, k)
    assert s[0, 2] == -1.5 and s[0, 4] == 1.5 and np.isnan(s[:, 3]).all()          # (2 pixels apart, not 1)
    k[:, 3:] = 0
    s = OREF.sdf_known_ref(m, k)
    none = np.float32(np.sqrt(np.float32(H * H + W * W))) - np.float32(0.5)
    assert (s[:, :3] == -none).all() and np.isnan(s[:, 3:]).all()
    assert np.array_equal(bits(silhouette.sdf_torch(torch.from_numpy(m), torch.from_numpy(k)).numpy()), bits(s))


# ----------------------------------------------------------------------------- who hides whom
@pytest.mark.parametrize("N", [1, 2, 5])
def test_known_from_others_torch_equals_the_restatement(N):
    from texpose_amd import silhouette
    H, W = 12, 17
    rs = np.random.RandomState(N)
    sdf = REF.sdf_ref(REF.discs(rs, (N, H, W)).astype(np.uint8))
    sdf[0, 3, 4] = np.nan                                        # not near, whatever the band
    unknown = []
    for band in (0.0, 1.0, 2.0, 2.5):
        want = OREF.known_from_others_ref(sdf, band)
        got = silhouette.known_from_others_torch(torch.from_numpy(sdf), band).numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want) and set(np.unique(want)) <= {0, 1}
        unknown.append(int((want == 0).sum()))
    if N == 1:
        assert unknown == [0] * 4                                # nobody else: everything is known
    else:
        assert all(a <= b for a, b in zip(unknown, unknown[1:])) and 0 < unknown[0] < unknown[-1] < N * H * W


def test_known_from_others_by_hand():
    """Two instances of one pixel each, 2 pixels apart in a row: d2 = 4, sdf = 1.5 at the other's pixel.  Band 2 makes the comparison
    an equality (1.5 <= 2 - 0.5), and it reads "near"."""
    m = np.zeros((2, 1, 5), np.uint8)
    m[0, 0, 1] = m[1, 0, 3] = 1
    sdf = REF.sdf_ref(m)
    assert sdf[0, 0, 3] == 1.5 and sdf[1, 0, 1] == 1.5
    assert OREF.known_from_others_ref(sdf, 0.0).tolist() == [[[1, 1, 1, 0, 1]], [[1, 0, 1, 1, 1]]]
    assert OREF.known_from_others_ref(sdf, 1.0).tolist() == [[[1, 1, 0, 0, 0]], [[0, 0, 0, 1, 1]]]
    assert OREF.known_from_others_ref(sdf, 2.0).tolist() == [[[1, 0, 0, 0, 0]], [[0, 0, 0, 0, 1]]]
    assert OREF.known_from_others_ref(sdf, np.nextafter(np.float32(2.0), np.float32(0))).tolist() == OREF.known_from_others_ref(sdf, 1.0).tolist()


# ----------------------------------------------------------------------------- the loop: DESIGN section 22's table
# the issue's prototype: (mesh, image, occluder) -> visible share, naive then known: rms first, last; visible IoU last; deg, mm last
PROTOTYPE = {("bent sphere", 0, "bottom third"): (0.72, (1.072, 1.021, 0.859, 45.12, 19.4), (0.424, 0.000, 1.000, 1.37, 2.85)),
             ("bent sphere", 1, "bottom third"): (0.65, (1.385, 0.888, 0.847, 40.59, 285.0), (0.974, 0.177, 0.992, 21.79, 31.3)),
             ("bent torus", 0, "bottom third"): (0.77, (1.182, 0.908, 0.816, 13.36, 180.0), (0.307, 0.000, 0.992, 1.28, 7.53)),
             ("bent torus", 1, "bottom third"): (0.66, (1.851, np.nan, 0.000, 101.4, 754.0), (1.616, 0.000, 0.993, 1.76, 11.2)),
             ("bent sphere", 0, "corner disc"): (0.79, (1.015, 0.814, 0.906, 36.30, 74.9), (0.447, 0.203, 0.987, 3.82, 21.8)),
             ("bent sphere", 1, "corner disc"): (0.90, (1.454, 1.017, 0.948, 14.37, 7.68), (1.236, 0.198, 0.992, 2.87, 3.53)),
             ("bent torus", 0, "corner disc"): (0.95, (0.903, 0.500, 0.940, 7.13, 46.2), (0.366, 0.058, 0.993, 0.44, 6.49)),
             ("bent torus", 1, "corner disc"): (0.87, (1.678, 0.929, 0.844, 10.55, 122.0), (1.593, 0.000, 0.998, 0.58, 2.99))}


def check_image_space(row):
    """The conditions on one image of a loop with the known field (the issue's bars: the worst measured rms ratio is 0.45, the worst
    visible IoU 0.987)."""
    assert row["status"] == 0
    assert row["rms"] <= 0.6 * row["rms0"]
    assert row["viou"] >= row["viou0"] and row["viou"] >= 0.98


@pytest.mark.parametrize("kind", OREF.ASSERTED)
@pytest.mark.parametrize("name", REF.MESHES)
def test_loop_on_occluded_masks_reproduces_the_table(name, kind):
    """From 3 deg and 6 .. 8 mm with the lower third or a corner disc of the object hidden (0.65 .. 0.95 of it visible): with the
    field that knows what is unknown the outline of the visible part closes; with today's field of the same cut mask it does not."""
    c = OREF.occluded_case(name, kind)
    for b in range(2):
        print(OREF.table_line(c, b))
    for b in range(2):
        n, k = c["naive"]["rows"][b], c["known"]["rows"][b]
        check_image_space(k)
        assert k["viou"] > n["viou"] and k["re"] < n["re"]
        visible, pn, pk = PROTOTYPE[name, b, kind]
        assert abs(c["visible"][b] - visible) <= 5e-3
        for row, p in ((n, pn), (k, pk)):
            assert abs(row["rms0"] - p[0]) <= 1e-3 and (np.isnan(row["rms"]) if np.isnan(p[1]) else abs(row["rms"] - p[1]) <= 1e-3)
            assert abs(row["viou"] - p[2]) <= 1e-3 and abs(row["re"] - p[3]) <= 0.06 and abs(row["te"] - p[4]) <= 0.006 * p[4] + 0.006


@pytest.mark.parametrize("name", REF.MESHES)
def test_loop_with_the_right_half_hidden_is_the_stated_limit(name, capsys):
    """0.43 .. 0.53 of the object visible: the outline over the visible part still closes better than with today's field, the pose
    does not follow.  Printed for DESIGN section 22, not asserted beyond the run ending."""
    c = OREF.occluded_case(name, "right half")
    for b in range(2):
        print(OREF.table_line(c, b))
        assert 0.4 < c["visible"][b] < 0.55
