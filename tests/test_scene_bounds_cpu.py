"""CPU: the scene-bounds rules.  Golden G23 pins what can be called of the reference's novel-view loop (pixel rays, slab values, the
pose sweep); tests/scene_bounds_ref.py restates the z-buffer blend, which the reference has inline next to a PyTorch3D render, and is
itself pinned here to G23's slab values and to hand-built cases.  The GPU kernel is compared with that helper in
tests/test_gpu_scene_bounds.py."""
import re
import os

import numpy as np
import torch

import scene_bounds_ref as SB
from conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_helper_slab_matches_g23():
    """Same bar as test_oracle_golden.test_aabb_g3: validity exact, t_near / t_far rtol 1e-6, atol 1e-6."""
    g = load_golden("g23_scene_bounds")
    o, d = g["center"].numpy(), g["ray"].numpy()
    for k in range(3):
        lo, hi = g["boxes"][k, 0].numpy(), g["boxes"][k, 1].numpy()
        tn, tf, ok = SB.slab(lo, hi, o, d)
        assert np.array_equal(ok.astype(np.uint8), g["valid"][k].numpy())
        torch.testing.assert_close(torch.from_numpy(tn), g["t_near"][k], rtol=1e-6, atol=1e-6, equal_nan=True)
        torch.testing.assert_close(torch.from_numpy(tf), g["t_far"][k], rtol=1e-6, atol=1e-6, equal_nan=True)
        assert 0 < ok.sum() < ok.size
    # the box table is the reference's expression of the mm boxes
    assert torch.equal((g["bb_mm"] * g["depth_scale"]) / 1000, g["boxes"])


def _hand_case():
    """One image of six pixels, three objects (ids 7, 3, 9).  Rays run along +z from z = 0 at x = pixel index, y = 0; the boxes are
    x-intervals at different depths, so the slab interval is the box's z interval where x lies inside it and invalid elsewhere.
        pixel      0      1      2      3      4      5
        object 7   2000   2000   -1     -1     2000   -1        box x in [-0.5, 1.5], z in [19, 21]
        object 3   -1     1500   1500   -1     2000   0         box x in [0.5, 2.5],  z in [14, 16]
        object 9   -1     -1     -1     -1     2500   -1        box x in [3.5, 4.5],  z in [24, 26]
    """
    m = -1.0
    zbuf = np.array([[2000, 2000, m, m, 2000, m], [m, 1500, 1500, m, 2000, 0], [m, m, m, m, 2500, m]], dtype=F)[:, None, :]
    ids = np.array([7, 3, 9], dtype=np.int32)
    boxes = np.array([[[-0.5, -1, 19], [1.5, 1, 21]], [[0.5, -1, 14], [2.5, 1, 16]], [[3.5, -1, 24], [4.5, 1, 26]]], dtype=F)
    o = np.stack([np.arange(6), np.zeros(6), np.zeros(6)], -1).astype(F)[None]
    d = np.tile(np.array([0, 0, 1], dtype=F), (1, 6, 1))
    return zbuf, ids, boxes, (o, d)


def test_helper_blend_hand_cases():
    zbuf, ids, boxes, rays = _hand_case()
    bg = (0.5, 30.0)
    # occlusion order: the nearest surface owns the pixel; equal depths go to the earlier object; -1 and 0 are background
    r = SB.blend(zbuf, ids, "box", 10.0, bg, boxes=boxes, rays=rays)
    assert r["label"].tolist() == [[7, 3, 3, 0, 7, 0]]
    np.testing.assert_array_equal(r["depth"], np.array([[20, 15, 15, 0, 20, 0]], dtype=F))
    # box: pixel 0 and 1 and 2 lie inside their winner's x interval; pixel 4 is owned by object 7 whose box ends at x = 1.5 ->
    # invalid slab -> 0 / 0 on a covered pixel; pixels 3 and 5 are background
    np.testing.assert_array_equal(r["z_near"], np.array([[19, 14, 14, 0.5, 0, 0.5]], dtype=F))
    np.testing.assert_array_equal(r["z_far"], np.array([[21, 16, 16, 30, 0, 30]], dtype=F))
    # render: 0.8 x and 1.2 x the blended depth as single fp32 products
    r = SB.blend(zbuf, ids, "render", 10.0, bg)
    d = np.array([20, 15, 15, 0, 20, 0], dtype=F)
    cov = d > 0
    np.testing.assert_array_equal(r["z_near"][0], np.where(cov, d * F(0.8), F(0.5)))
    np.testing.assert_array_equal(r["z_far"][0], np.where(cov, d * F(1.2), F(30.0)))
    assert r["label"].tolist() == [[7, 3, 3, 0, 7, 0]]
    # none: the background range everywhere, label and depth still there
    r = SB.blend(zbuf, ids, "none", 10.0, bg)
    assert (r["z_near"] == F(0.5)).all() and (r["z_far"] == F(30.0)).all()
    assert r["label"].tolist() == [[7, 3, 3, 0, 7, 0]] and r["depth"][0, 0] == 20
    # the unit conversion is two rounded steps: (z / 1000) * scale, not z * (scale / 1000)
    z = np.full((1, 1, 1), 1234.567, dtype=F)
    assert SB.blend(z, [1], "none", 10.0, bg)["depth"][0, 0] == (F(1234.567) / F(1000)) * F(10)


def test_novel_view_poses_obj_matches_g23():
    from texpose_amd.scene_bounds import novel_view_poses_obj
    g = load_golden("g23_scene_bounds")
    for N, key in ((10, "novel10"), (7, "novel7")):
        p = novel_view_poses_obj(g["anchor"], N)
        assert p.shape == (N, 3, 4)
        torch.testing.assert_close(p, g[key], rtol=1e-6, atol=1e-6)
    # the middle pose of an even sweep is the anchor itself (angle 0)
    torch.testing.assert_close(novel_view_poses_obj(g["anchor"], 10)[5], g["anchor"], rtol=0, atol=1e-7)


def test_scene_bounds_in_header_exports_and_binding():
    import ctypes as C
    from texpose_amd import _lib
    header = open(os.path.join(REPO, "include", "texpose_amd.h")).read()
    abi = int(re.search(r"#define TP_ABI_VERSION (\d+)", header).group(1))
    assert abi == _lib.ABI_VERSION
    assert re.search(r"\bint tp_scene_bounds\(const tp_scene_bounds_args\* args, tp_stream_t stream\);", header)
    assert "tp_scene_bounds" in _lib.SYMBOLS
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "tp_scene_bounds")
    lib.tp_abi_version.restype = C.c_int
    assert lib.tp_abi_version() == abi
    m = re.search(r"#define TP_SCENE_MAX_OBJECTS (\d+)", header)
    assert m and int(m.group(1)) == _lib.SCENE_MAX_OBJECTS == 32
    # the struct the binding declares has the header's fields in the header's order
    body = re.search(r"typedef struct tp_scene_bounds_args \{(.*?)\} tp_scene_bounds_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().lstrip("*") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace("float*", "").replace("int32_t*", "").split(",")]
    names = [n.split()[-1].lstrip("*") for n in names]
    assert names == [f[0] for f in _lib.SceneBoundsArgs._fields_]
    # null arguments are rejected with the library's negative code before anything is launched
    lib.tp_scene_bounds.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.tp_scene_bounds(None, None) < 0
    a = _lib.SceneBoundsArgs()
    a.B, a.H, a.W, a.K = 1, 4, 4, 33
    assert lib.tp_scene_bounds(C.byref(a), None) < 0
    lib.tp_last_error.restype = C.c_char_p
    assert b"32" in lib.tp_last_error()
