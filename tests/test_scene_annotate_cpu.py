"""CPU: the rules of the scene annotations (tp_scene_annotate, tp_view_images) and the BOP scene writer.  tests/scene_annotate_ref.py
restates both kernels and is pinned here to hand-built cases; tests/bop_reader_ref.py restates what the reference's data layer takes from
a scene folder and is pinned to golden G24 (the reference's own get_2d_bbox and get_all_camera_poses on a hand-written scene); the
writer is checked from host arrays through read_bop_frame and that helper.  The GPU kernels are compared with the restatement in
tests/test_gpu_scene_annotate.py."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import bop_reader_ref as RD
import scene_annotate_ref as SA
from conftest import GOLDEN, load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def hand_scene():
    """One 6 x 8 image, six objects (ids 4, 9, 2, 7, 5, 3), depths in mm; label is the nearest covered object's id.
        object 4: rows 1-3, columns 1-4 at 900: partly hidden by object 9
        object 9: rows 2-4, columns 3-6 at 700: in front of everything it meets
        object 2: rows 2-3, columns 4-5 at 1200: fully hidden behind object 9
        object 7: every pixel at 2000: touches all four borders, hidden wherever another object is
        object 5: absent (-1 everywhere, one NaN and one 0)
        object 3: the single pixel (0, 7) at 500
    """
    H, W = 6, 8
    z = np.full((6, 1, H, W), -1.0, dtype=F)
    z[0, 0, 1:4, 1:5] = 900
    z[1, 0, 2:5, 3:7] = 700
    z[2, 0, 2:4, 4:6] = 1200
    z[3, 0] = 2000
    z[4, 0, 0, 0], z[4, 0, 5, 7] = np.nan, 0.0
    z[5, 0, 0, 7] = 500
    ids = np.array([4, 9, 2, 7, 5, 3], dtype=np.int32)
    near = np.where(z > 0, z, F(1e5))
    label = ids[np.argmin(near, axis=0)].astype(np.int32)           # object 7 covers every pixel: no background here
    return z, label.reshape(1, H * W), ids


def test_helper_annotate_hand_cases():
    z, label, ids = hand_scene()
    info, mask, vis = SA.annotate(z, label, ids)
    assert info.shape == (1, 6, 10) and info.dtype == np.int32 and mask.dtype == np.uint8
    rows = info[0].tolist()
    # partly occluded: 12 pixels, 8 of them visible (rows 2-3, columns 3-4 belong to object 9); the visible box loses nothing
    assert rows[0] == [12, 8, 1, 1, 4, 3, 1, 1, 4, 3]
    assert rows[1] == [12, 12, 3, 2, 6, 4, 3, 2, 6, 4]
    # fully hidden: counted and boxed, nothing visible
    assert rows[2] == [4, 0, 4, 2, 5, 3, -1, -1, -1, -1]
    # all four borders: extents 0 .. W-1, 0 .. H-1 for both sets (the visible part still reaches every border)
    assert rows[3] == [48, 48 - 12 - 8 - 1, 0, 0, 7, 5, 0, 0, 7, 5]
    # absent: NaN, 0 and -1 are background
    assert rows[4] == [0, 0] + [-1] * 8
    # one pixel: xmin == xmax, ymin == ymax
    assert rows[5] == [1, 1, 7, 0, 7, 0, 7, 0, 7, 0]
    assert set(np.unique(mask)) <= {0, 255} and (vis <= mask).all()
    assert (mask[0, 0] == 255).sum() == 12 and mask[0, 0, 1, 1] == 255 and mask[0, 0, 0, 0] == 0
    assert vis[0, 0, 2, 3] == 0 and vis[0, 0, 2, 2] == 255 and vis[0, 1, 2, 3] == 255
    assert not mask[0, 4].any() and not vis[0, 2].any()
    # a label that names nobody (0: background) makes nothing visible, the silhouettes stay
    info0, _, vis0 = SA.annotate(z, np.zeros_like(label), ids)
    assert not vis0.any() and (info0[0, :, 1] == 0).all() and (info0[0, :, 0] == info[0, :, 0]).all()


def test_helper_annotate_32_objects():
    rs = np.random.RandomState(32)
    K, B, H, W = 32, 2, 9, 11
    z = rs.uniform(300, 900, size=(K, B, H, W)).astype(F)
    z[rs.uniform(size=z.shape) < 0.7] = -1
    ids = (rs.permutation(K) + 1).astype(np.int32)
    near = np.where(z > 0, z, F(1e5))
    w = np.argmin(near, axis=0)
    label = np.where(np.take_along_axis(z, w[None], 0)[0] > 0, ids[w], 0).astype(np.int32).reshape(B, H * W)
    info, mask, vis = SA.annotate(z, label, ids)
    assert info.shape == (B, K, 10)
    # every covered pixel is visible for exactly one object, an uncovered one for none
    assert np.array_equal((vis > 0).sum(1), (label.reshape(B, H, W) > 0).astype(int))
    assert np.array_equal(info[..., 0], (z > 0).sum((2, 3)).T) and np.array_equal(info[..., 1], (vis > 0).sum((2, 3)))
    for b in range(B):
        for k in range(K):
            ys, xs = np.nonzero(z[k, b] > 0)
            assert info[b, k, 2:6].tolist() == [xs.min(), ys.min(), xs.max(), ys.max()]


def test_helper_image_rules():
    x = np.array([[[0.0, 1.0, 1.5], [-0.25, np.nan, 0.5], [0.999, 1 / 255, 0.003921568], [np.inf, -np.inf, 254.5 / 255]]], dtype=F)
    got = SA.rgb8(x, 2, 2).reshape(4, 3).tolist()
    assert got[0] == [0, 255, 255] and got[1] == [0, 0, 127]
    assert got[2] == [int(F(0.999) * F(255)), int(F(1 / 255) * F(255)), int(F(0.003921568) * F(255))]           # truncation, of the fp32 product
    assert got[2][0] == 254 and got[2][2] == 0
    assert got[3] == [255, 0, 254]
    # the tool's present chain gives the same bytes wherever it is defined
    t = torch.from_numpy(np.nan_to_num(x, nan=0.0))
    assert np.array_equal((t.clamp(0, 1) * 255).byte().numpy().reshape(1, 2, 2, 3), SA.rgb8(np.nan_to_num(x, nan=0.0), 2, 2))
    # depth: NeRF units / scale * 2000; 65535 is reached at 327.675 units of scale 10
    scale = 10.0
    d = np.array([[0.0, 8.0, -1.0, np.nan, 327.67, 327.68, 1e9, np.inf, 0.00499, 0.005]], dtype=F)
    got = SA.depth16(d, 2, 5, scale).reshape(-1).tolist()
    want_mid = int(np.trunc((F(327.67) / F(10)) * F(2000)))
    assert got == [0, 1600, 0, 0, want_mid, 65535, 65535, 65535, int((F(0.00499) / F(10)) * F(2000)), int((F(0.005) / F(10)) * F(2000))]
    assert 65530 <= want_mid < 65535
    # two rounded steps, in this order: (d / scale) * per_metre, not d * (per_metre / scale)
    v = F(1.2345678)
    assert SA.depth16(np.array([[v]], dtype=F), 1, 1, 3.0)[0, 0, 0] == int((v / F(3)) * F(2000))


def g24_lines():
    objects = json.load(open(os.path.join(GOLDEN, "g24_bop_scene", "scene_object.json")))
    return [(name, int(frame)) for frame in sorted(objects, key=int) for name in sorted(objects[frame])]


def test_reader_helper_matches_g24():
    """The reference's own get_all_camera_poses(source='gt') and get_2d_bbox on the hand-written scene: key names, the gt list order
    through scene_object.json, mm -> metres -> nerf.depth.scale units, the order of the box's fields under both box formats."""
    g = load_golden("g24_bop_scene")
    scene = RD.load_scene(os.path.join(GOLDEN, "g24_bop_scene"))
    lines = g24_lines()
    assert len(lines) == 6 and [f for _, f in lines] == g["frame"].tolist()
    for i, (name, frame) in enumerate(lines):
        k = RD.gt_index(scene, frame, name)
        assert k == int(g["gt_index"][i])
        pose = RD.raw_pose(scene, frame, k)
        assert pose.dtype == F and pose[3].tolist() == [0, 0, 0, 1]
        # parse_raw_camera composes with the identity and scales t by nerf.depth.scale
        np.testing.assert_allclose(pose[:3, :3], g["pose"][i, :, :3].numpy(), rtol=0, atol=1e-7)
        np.testing.assert_allclose(pose[:3, 3] * F(g["depth_scale_opt"]), g["pose"][i, :, 3].numpy(), rtol=1e-6, atol=0)
        for fmt in ("none", "wh"):
            center, side, resize = RD.get_2d_bbox(scene, frame, k, g["res"], None if fmt == "none" else fmt)
            assert center.tolist() == g["center_" + fmt][i].tolist() and side == int(g["scale_" + fmt][i])
            assert resize == float(g["resize_" + fmt][i])
    assert not torch.equal(g["center_none"], g["center_wh"])         # the scene has boxes that are not square
    assert RD.gt_index(scene, 3) == 0


def host_scene(rs, B=2, H=12, W=20):
    """A scene as the device would deliver it, from the restatement alone: three objects (ids 5, 2, 8), object 8 absent in view 1."""
    z = np.full((3, B, H, W), -1.0, dtype=F)
    z[0, :, 2:9, 3:12] = 800
    z[1, :, 5:11, 8:20] = 650                                       # hides a corner of object 5, touches two borders
    z[2, 0, 0:2, 0:3] = 900
    ids = np.array([5, 2, 8], dtype=np.int32)
    near = np.where(z > 0, z, F(1e5))
    w = np.argmin(near, axis=0)
    label = np.where(np.take_along_axis(z, w[None], 0)[0] > 0, ids[w], 0).astype(np.int32).reshape(B, H * W)
    info, mask, vis = SA.annotate(z, label, ids)
    rgb = rs.uniform(-0.1, 1.1, size=(B, H * W, 3)).astype(F)
    depth = (np.where(label > 0, np.take_along_axis(near, w[None], 0)[0].reshape(B, H * W), 0) / F(1000) * F(10)).astype(F)
    return dict(ids=ids, info=info, mask=mask, mask_visib=vis, rgb8=SA.rgb8(rgb, H, W), depth16=SA.depth16(depth, H, W, 10.0), depth=depth)


def test_writer_round_trip_from_host_arrays(tmp_path):
    from texpose_amd.bop_scene import BopSceneWriter, read_bop_frame, verify_bop_scene
    rs = np.random.RandomState(5)
    B, H, W, scale = 2, 12, 20, 10.0
    s = host_scene(rs, B, H, W)
    intr = np.array([[572.4114, 0, 9.75], [0, 573.57043, 6.25], [0, 0, 1]], dtype=F)
    pose = rs.normal(size=(B, 3, 4)).astype(F)
    pose[:, :, 3] = [[0.123456, -0.25, 8.0], [1.5, 0.333333, 7.77]]
    root = str(tmp_path / "scene")
    w = BopSceneWriter(root, intr, scale, png_per_metre=2000, names={5: "ape", 2: "can", 8: "duck"}, first_frame=7)
    assert w.add_views(pose[:1], s["ids"], s["info"][:1], s["mask"][:1], s["mask_visib"][:1], s["rgb8"][:1], s["depth16"][:1]) == [7]
    assert w.add_views(torch.from_numpy(pose[1:]), torch.from_numpy(s["ids"]), torch.from_numpy(s["info"][1:]), s["mask"][1:],
                       s["mask_visib"][1:], torch.from_numpy(s["rgb8"][1:]), s["depth16"][1:]) == [8]
    w.close()
    assert sorted(os.listdir(root)) == ["depth", "mask", "mask_visib", "rgb", "scene_camera.json", "scene_gt.json", "scene_gt_info.json",
                                        "scene_object.json"]
    assert sorted(os.listdir(os.path.join(root, "mask"))) == ["%06d_%06d.png" % (f, k) for f in (7, 8) for k in range(3)]
    assert sorted(os.listdir(os.path.join(root, "rgb"))) == sorted(os.listdir(os.path.join(root, "depth"))) == ["000007.png", "000008.png"]
    assert verify_bop_scene(root) == 2
    scene = RD.load_scene(root)
    for b, frame in enumerate((7, 8)):
        fr = read_bop_frame(root, frame)
        # every PNG byte
        assert fr["rgb"].dtype == np.uint8 and np.array_equal(fr["rgb"], s["rgb8"][b])
        assert fr["depth"].dtype == np.uint16 and np.array_equal(fr["depth"], s["depth16"][b])
        assert fr["mask"].dtype == np.uint8 and np.array_equal(fr["mask"], s["mask"][b]) and np.array_equal(fr["mask_visib"], s["mask_visib"][b])
        # scene_camera.json: png x depth_scale = mm
        cam = scene["scene_camera"][str(frame)]
        assert sorted(cam) == ["cam_K", "depth_scale"] and cam["depth_scale"] == 0.5
        assert np.array_equal(np.array(cam["cam_K"], dtype=F).reshape(3, 3), intr) and np.array_equal(fr["cam_K"], intr)
        mm = fr["depth"].astype(np.float64) * fr["depth_scale"]
        np.testing.assert_allclose(mm, s["depth"][b].reshape(H, W).astype(np.float64) / scale * 1000, rtol=0, atol=0.5 + 1e-3)
        np.testing.assert_allclose(RD.depth_metres(root, scene, frame), mm / 1000, rtol=1e-12)
        # scene_gt.json: every object carries the view's pose, t in mm by the rasteriser's expression
        assert fr["obj_id"].tolist() == [5, 2, 8] and fr["objects"] == {"ape": 0, "can": 1, "duck": 2}
        t_mm = (torch.from_numpy(pose[b, :, 3]) / scale) * 1000
        for k, entry in enumerate(scene["scene_gt"][str(frame)]):
            assert sorted(entry) == ["cam_R_m2c", "cam_t_m2c", "obj_id"] and len(entry["cam_R_m2c"]) == 9 and len(entry["cam_t_m2c"]) == 3
            assert np.array_equal(fr["cam_R_m2c"][k], pose[b, :, :3]) and np.array_equal(fr["cam_t_m2c"][k], t_mm.numpy())
            raw = RD.raw_pose(scene, frame, RD.gt_index(scene, frame, ["ape", "can", "duck"][k]))
            assert np.array_equal(raw[:3, :3], pose[b, :, :3])
            np.testing.assert_allclose(raw[:3, 3] * F(scale), pose[b, :, 3], rtol=3e-7, atol=0)      # two roundings each way
        # scene_gt_info.json: every field
        for k, entry in enumerate(scene["scene_gt_info"][str(frame)]):
            row = s["info"][b, k].tolist()
            assert sorted(entry) == ["bbox_obj", "bbox_visib", "px_count_all", "px_count_valid", "px_count_visib", "visib_fract"]
            assert entry["px_count_all"] == entry["px_count_valid"] == row[0] and entry["px_count_visib"] == row[1]
            assert isinstance(entry["visib_fract"], float) and entry["visib_fract"] == (row[1] / row[0] if row[0] else 0.0)
            for key, e in (("bbox_obj", row[2:6]), ("bbox_visib", row[6:10])):
                assert entry[key] == ([-1] * 4 if e[2] < 0 else [e[0], e[1], e[2] - e[0], e[3] - e[1]])
                assert all(isinstance(v, int) for v in entry[key])
            # what the reference's data layer would take: the mask as png > 0, the crop box from bbox_obj
            assert np.array_equal(RD.mask_of(root, frame, k), s["mask"][b, k] > 0)
            assert np.array_equal(RD.mask_of(root, frame, k, "mask_visib"), s["mask_visib"][b, k] > 0)
            if row[0]:
                center, side, _ = RD.get_2d_bbox(scene, frame, k, 128, "wh")
                x, y, wd, ht = entry["bbox_obj"]
                assert center.tolist() == [int(y + ht / 2), int(x + wd / 2)] and side == int(1.5 * max(wd, ht))
    info = scene["scene_gt_info"]
    assert 0 < info["7"][0]["visib_fract"] < 1 and info["7"][1]["visib_fract"] == 1.0
    assert info["8"][2] == dict(bbox_obj=[-1] * 4, bbox_visib=[-1] * 4, px_count_all=0, px_count_valid=0, px_count_visib=0, visib_fract=0.0)
    # verify notices a file that disagrees with the JSON
    from PIL import Image
    bad = s["mask"][0, 0].copy()
    bad[0, 0] = 255
    Image.fromarray(bad, "L").save(os.path.join(root, "mask", "000007_000000.png"))
    with pytest.raises(ValueError, match="frame 7"):
        verify_bop_scene(root)
    # shapes and types are checked, a name is needed for every id
    with pytest.raises(ValueError):
        w.add_views(pose[:1], s["ids"], s["info"][:1], s["mask"][:1], s["mask_visib"][:1], s["rgb8"][:1], s["depth16"][:1].astype(np.int32))
    with pytest.raises(ValueError):
        w.add_views(pose[:1], s["ids"][:2], s["info"][:1], s["mask"][:1], s["mask_visib"][:1], s["rgb8"][:1], s["depth16"][:1])
    with pytest.raises(ValueError, match="name"):
        BopSceneWriter(str(tmp_path / "other"), intr, scale, names={5: "ape"}).add_views(
            pose[:1], s["ids"], s["info"][:1], s["mask"][:1], s["mask_visib"][:1], s["rgb8"][:1], s["depth16"][:1])


def test_writer_without_names_writes_no_scene_object(tmp_path):
    from texpose_amd.bop_scene import BopSceneWriter, read_bop_frame
    s = host_scene(np.random.RandomState(1))
    w = BopSceneWriter(str(tmp_path), np.eye(3, dtype=F), 10.0)
    w.add_views(np.zeros((2, 3, 4), dtype=F), s["ids"], s["info"], s["mask"], s["mask_visib"], s["rgb8"], s["depth16"])
    w.close()
    assert not os.path.exists(str(tmp_path / "scene_object.json"))
    assert read_bop_frame(str(tmp_path), 1)["objects"] is None and read_bop_frame(str(tmp_path), 0)["mask"].shape == (3, 12, 20)


def header_struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?\w+\s*\*?", "", decl, count=1).split(",")]
    return fields


def test_scene_annotate_in_header_exports_and_binding():
    from texpose_amd import _lib, ops
    header = open(os.path.join(REPO, "include", "texpose_amd.h")).read()
    abi = int(re.search(r"#define TP_ABI_VERSION (\d+)", header).group(1))
    assert abi == _lib.ABI_VERSION == 16
    assert re.search(r"\bint tp_scene_annotate\(const tp_scene_annotate_args\* args, tp_stream_t stream\);", header)
    assert re.search(r"\bint tp_view_images\(const tp_view_images_args\* args, tp_stream_t stream\);", header)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("tp_scene_annotate", "tp_view_images"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    lib.tp_abi_version.restype = C.c_int
    assert lib.tp_abi_version() == 16
    m = re.search(r"#define TP_SCENE_INFO_FIELDS (\d+)", header)
    assert m and int(m.group(1)) == _lib.SCENE_INFO_FIELDS == len(ops.SCENE_INFO_KEYS) == 10
    assert header_struct_fields(header, "tp_scene_annotate_args") == [f[0] for f in _lib.SceneAnnotateArgs._fields_]
    assert header_struct_fields(header, "tp_view_images_args") == [f[0] for f in _lib.ViewImagesArgs._fields_]
    assert C.sizeof(_lib.SceneAnnotateArgs) == 3 * 8 + 4 * 4 + 3 * 8
    assert C.sizeof(_lib.ViewImagesArgs) == 2 * 8 + 3 * 4 + 2 * 4 + 4 + 2 * 8          # (the int / float run is padded to 8)


def test_argument_validation_without_gpu():
    from texpose_amd import _lib
    from texpose_amd.scene_bounds import SceneBounds, distinct_object_ids
    lib = _lib.load()
    one = C.c_void_p(16)                                            # never dereferenced: validation comes before any launch
    assert lib.tp_scene_annotate(None, None) < 0 and lib.tp_view_images(None, None) < 0

    def annotate_args(**kw):
        a = _lib.SceneAnnotateArgs()
        a.zbuf, a.label, a.ids, a.info = one, one, one, one
        a.B, a.H, a.W, a.K = 1, 4, 4, 3
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert lib.tp_scene_annotate(C.byref(annotate_args(K=33)), None) < 0
    assert b"32" in lib.tp_last_error()
    assert lib.tp_scene_annotate(C.byref(annotate_args(K=0)), None) < 0
    assert lib.tp_scene_annotate(C.byref(annotate_args(H=0)), None) < 0
    assert b"bad sizes" in lib.tp_last_error()
    for missing in ("zbuf", "label", "ids", "info"):
        assert lib.tp_scene_annotate(C.byref(annotate_args(**{missing: None})), None) < 0, missing
        assert b"null" in lib.tp_last_error()
    v = _lib.ViewImagesArgs()
    v.B, v.H, v.W, v.depth_scale, v.png_per_metre = 1, 4, 4, 10.0, 2000.0
    assert lib.tp_view_images(C.byref(v), None) < 0 and b"null" in lib.tp_last_error()          # neither pair
    v.rgb = one
    assert lib.tp_view_images(C.byref(v), None) < 0                                             # rgb without rgb8
    v.rgb8, v.depth, v.depth16, v.depth_scale = one, one, one, 0.0
    assert lib.tp_view_images(C.byref(v), None) < 0 and b"positive" in lib.tp_last_error()
    v.depth_scale, v.W = 10.0, 0
    assert lib.tp_view_images(C.byref(v), None) < 0 and b"bad sizes" in lib.tp_last_error()
    # duplicate ids are rejected by the Python layer, before anything touches a device
    assert distinct_object_ids([5, 2, 9]) == [5, 2, 9]
    with pytest.raises(ValueError, match="duplicate"):
        distinct_object_ids([5, 2, 5])
    with pytest.raises(ValueError, match="positive"):
        distinct_object_ids([5, 0])
    with pytest.raises(ValueError, match="duplicate"):
        SceneBounds({5: (None, [0] * 3, [1] * 3), "5": (None, [0] * 3, [1] * 3)}, 8, 8, 10.0, (0.0, 30.0))


def test_ops_refuse_cpu_tensors():
    from texpose_amd import ops
    z, label, ids = torch.ones(2, 1, 4, 4), torch.zeros(1, 16, dtype=torch.int32), torch.tensor([1, 2], dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        ops.scene_annotate(z, label, ids)
    with pytest.raises(ValueError, match="GPU"):
        ops.view_images(torch.zeros(1, 16, 3), torch.zeros(1, 16), H=4, W=4, depth_scale=10.0)
    with pytest.raises(ValueError):
        ops.view_images(None, None, H=4, W=4)
