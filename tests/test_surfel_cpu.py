"""CPU: the surfel-map host side (texpose_amd.surfel: PLY reader, NOCS normalisation, pose calibration, file writer) and the fp64
restatements the GPU rasteriser is tested against (tests/mesh_raster_ref.py), pinned to golden G21 (the reference's normals) and to
analytic answers."""
import os
import struct

import numpy as np
import pytest
import torch

import mesh_raster_ref as REF
from texpose_amd import surfel
from texpose_amd.options import AttrDict

VERTS = np.array([[0, 0, 0], [1.5, 0, 0], [1.5, 2, 0], [0, 2, 0], [0.5, 0.5, 3.25]], dtype=np.float32)
COLORS = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 20, 30], [200, 100, 50]], dtype=np.uint8)
POLYS = [[0, 1, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4]]       # one quad + three triangles
TRIS = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [2, 3, 4]], dtype=np.int32)


def _write_ply(path, binary, count_type="uchar", index_type="int", color=True, extra=True):
    props = ["property float x", "property float y", "property float z"]
    if extra:
        props += ["property float nx", "property float ny", "property float nz"]
    if color:
        props += ["property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    head = ["ply", "format %s 1.0" % ("binary_little_endian" if binary else "ascii"), "comment written by the test",
            "element vertex %d" % len(VERTS)] + props + \
           ["element face %d" % len(POLYS), "property list %s %s vertex_indices" % (count_type, index_type), "end_header"]
    ct = {"uchar": "B", "int": "i"}[count_type]
    it = {"int": "i", "uint": "I"}[index_type]
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode())
        for v, c in zip(VERTS, COLORS):
            vals = list(v) + ([0.0, 0.0, 1.0] if extra else [])
            if binary:
                f.write(struct.pack("<%df" % len(vals), *vals))
                if color:
                    f.write(struct.pack("<4B", *c, 255))
            else:
                f.write((" ".join(repr(float(x)) for x in vals) + (" %d %d %d 255" % tuple(c) if color else "") + "\n").encode())
        for p in POLYS:
            if binary:
                f.write(struct.pack("<" + ct + it * len(p), len(p), *p))
            else:
                f.write((" ".join(str(x) for x in [len(p)] + p) + "\n").encode())


@pytest.mark.parametrize("binary", [False, True], ids=["ascii", "binary"])
@pytest.mark.parametrize("count_type,index_type", [("uchar", "int"), ("int", "uint")])
def test_load_ply_round_trip(tmp_path, binary, count_type, index_type):
    path = str(tmp_path / "m.ply")
    _write_ply(path, binary, count_type, index_type)
    verts, faces, vcolor = surfel.load_ply(path)
    assert verts.dtype == np.float32 and faces.dtype == np.int32 and vcolor.dtype == np.float32
    np.testing.assert_array_equal(verts, VERTS)
    np.testing.assert_array_equal(faces, TRIS)                     # the quad split into (0,1,2), (0,2,3)
    np.testing.assert_array_equal(vcolor, COLORS.astype(np.float32) / 255.0)


@pytest.mark.parametrize("binary", [False, True], ids=["ascii", "binary"])
def test_load_ply_without_colour(tmp_path, binary):
    path = str(tmp_path / "m.ply")
    _write_ply(path, binary, color=False, extra=False)
    verts, faces, vcolor = surfel.load_ply(path)
    assert vcolor is None
    np.testing.assert_array_equal(verts, VERTS)
    np.testing.assert_array_equal(faces, TRIS)


def test_load_ply_all_triangles_binary(tmp_path):
    # the one-read path of the binary reader (every face a triangle), BOP's layout: x y z nx ny nz red green blue alpha
    path = str(tmp_path / "t.ply")
    rs = np.random.RandomState(3)
    v = rs.normal(size=(50, 3)).astype(np.float32) * 40
    f = rs.randint(0, 50, size=(97, 3)).astype(np.int32)
    c = rs.randint(0, 256, size=(50, 3)).astype(np.uint8)
    head = "ply\nformat binary_little_endian 1.0\nelement vertex 50\nproperty float x\nproperty float y\nproperty float z\n" \
           "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n" \
           "property uchar alpha\nelement face 97\nproperty list uchar int vertex_indices\nend_header\n"
    with open(path, "wb") as fh:
        fh.write(head.encode())
        for k in range(50):
            fh.write(struct.pack("<6f4B", *v[k], 0, 0, 1, *c[k], 255))
        for k in range(97):
            fh.write(struct.pack("<B3i", 3, *f[k]))
    verts, faces, vcolor = surfel.load_ply(path)
    np.testing.assert_array_equal(verts, v)
    np.testing.assert_array_equal(faces, f)
    np.testing.assert_array_equal(vcolor, c.astype(np.float32) / 255.0)


def test_nocs_normalisation_matches_restatement():
    rs = np.random.RandomState(0)
    v = (rs.normal(size=(500, 3)) * [30, 50, 20] + [5, -7, 11]).astype(np.float32)
    ct, sc = surfel.nocs_normalisation(v)
    ct_r, sc_r = REF.nocs_normalisation(v)
    np.testing.assert_allclose(ct, ct_r, rtol=0, atol=1e-4)
    np.testing.assert_allclose(sc, sc_r, rtol=1e-5)
    x = REF.nocs_vertices(v, ct_r, sc_r)
    assert x.min() >= 0 and x.max() <= 1 and np.isclose(x.min(0), 0).sum() + np.isclose(x.max(0), 1).sum() == 3


def test_calibrate_pose_matches_restatement():
    rs = np.random.RandomState(1)
    from oracle.texpose_oracle import rotation_from_axis_angle
    poses = []
    for _ in range(4):
        R = rotation_from_axis_angle(rs.uniform(-2, 2, size=3)) + rs.normal(size=(3, 3)) * 1e-3     # slightly off SO(3)
        poses.append(np.concatenate([R, rs.uniform(-1, 1, size=(3, 1)) + [[0], [0], [8]]], axis=1))
    poses = np.stack(poses).astype(np.float32)
    got = surfel.calibrate_pose(torch.from_numpy(poses), 10.0).numpy()
    ref = REF.calibrate_pose(poses, 10.0)
    np.testing.assert_allclose(got[:, :, :3], ref[:, :, :3], atol=2e-6)
    np.testing.assert_allclose(got[:, :, 3], ref[:, :, 3], rtol=1e-6)
    for R in got[:, :, :3]:
        np.testing.assert_allclose(R.T @ R, np.eye(3), atol=1e-6)
        assert np.linalg.det(R) > 0


def test_normal_restatement_matches_g21(golden):
    g = golden("g21_surfel_normals")
    n = REF.normal_from_depth(g["depth"].numpy(), g["pose"].numpy(), g["K"].numpy())
    np.testing.assert_allclose(n, g["normal"].numpy(), rtol=0, atol=1e-6)
    assert (np.abs(g["normal"].numpy()).sum(-1) > 0).sum() > 1000      # the fixture is not mostly zeros


def test_writer_files_decode_to_the_truncation_rule(tmp_path):
    from PIL import Image
    rs = np.random.RandomState(2)
    B, H, W = 2, 5, 7
    depth = torch.from_numpy(np.where(rs.uniform(size=(B, H, W)) > 0.3, rs.uniform(500, 700, size=(B, H, W)), -1).astype(np.float32))
    cov = (depth > 0).float()[:, None]
    out = AttrDict(rgb_syn=torch.rand(B, 3, H, W) * cov, nocs=torch.rand(B, 3, H, W) * cov, depth=depth,
                   normal=torch.randn(B, 3, H, W) * cov, mask_syn=cov[:, 0])
    surfel.write_surfel_frame(str(tmp_path), 2, 17, out, 1)
    surfel.write_surfel_frame(str(tmp_path), "GT", 17, out, 0, obj_scene_id=4)
    rgba = np.asarray(Image.open(os.path.join(str(tmp_path), "rgbsyn_2", "000017.png")))
    nocs = np.asarray(Image.open(os.path.join(str(tmp_path), "nocs_2", "000017.png")))
    normal = np.load(os.path.join(str(tmp_path), "normal_2", "000017.npz"))["data"]
    assert rgba.shape == (H, W, 4) and nocs.shape == (H, W, 3) and normal.shape == (H, W, 3) and normal.dtype == np.float32
    hwc = lambda t: t[1].permute(1, 2, 0).numpy()
    np.testing.assert_array_equal(rgba[..., :3], (hwc(out.rgb_syn) * 255).astype(np.uint8))
    np.testing.assert_array_equal(rgba[..., 3], np.where(depth[1].numpy() > 0, 255, 0))
    np.testing.assert_array_equal(nocs, (hwc(out.nocs) * 255).astype(np.uint8))
    np.testing.assert_array_equal(normal, hwc(out.normal))
    assert os.path.exists(os.path.join(str(tmp_path), "rgbsyn_GT", "000017_000004.png"))
    assert os.path.exists(os.path.join(str(tmp_path), "normal_GT", "000017_000004.npz"))


def test_bruteforce_fronto_parallel_triangle():
    H, W, z0 = 40, 50, 500.0
    K = np.array([[100.0, 0, 25.0], [0, 100.0, 20.0], [0, 0, 1]])
    px = np.array([[4.2, 3.1], [44.7, 9.9], [15.3, 36.6]])          # screen positions
    verts = np.concatenate([(px - K[:2, 2]) / 100.0 * z0, np.full((3, 1), z0)], axis=1)
    pose = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    r = REF.rasterize(verts, [[0, 1, 2]], pose, K, H, W, vcolor=np.eye(3), nocs_norm=(np.zeros(3), np.ones(3)))
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    T = np.array([[px[0, 0] - px[2, 0], px[1, 0] - px[2, 0]], [px[0, 1] - px[2, 1], px[1, 1] - px[2, 1]]])
    l01 = np.linalg.solve(T, np.stack([jj.ravel() - px[2, 0], ii.ravel() - px[2, 1]]))
    bary = np.stack([l01[0], l01[1], 1 - l01[0] - l01[1]], axis=1)
    inside = (bary > 0).all(1)
    assert inside.sum() > 300
    np.testing.assert_array_equal(r["face"] == 0, inside)
    np.testing.assert_allclose(r["zbuf"][inside], z0, rtol=1e-12)
    assert (r["zbuf"][~inside] == -1).all()
    np.testing.assert_allclose(r["rgb"][inside], bary[inside], atol=1e-9)      # constant z: no perspective correction
    assert (r["rgb"][~inside] == 0).all()


def _convex_hull(p):
    p = sorted(map(tuple, p))
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for q in p:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], q) <= 0:
            lower.pop()
        lower.append(q)
    for q in reversed(p):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], q) <= 0:
            upper.pop()
        upper.append(q)
    return np.array(lower[:-1] + upper[:-1])


def cube_mesh(half=40.0):
    v = np.array([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], dtype=np.float32)
    quads = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]
    return v, np.array([[q[0], q[1], q[2]] for q in quads] + [[q[0], q[2], q[3]] for q in quads], dtype=np.int32)


def test_bruteforce_cube_silhouette():
    from oracle.texpose_oracle import rotation_from_axis_angle
    H, W = 64, 80
    verts, faces = cube_mesh()
    K = np.array([[300.0, 0, 41.3], [0, 300.0, 30.7], [0, 0, 1]])
    pose = np.concatenate([rotation_from_axis_angle(np.array([0.5, -0.8, 0.3])), [[3.0], [-2.0], [620.0]]], axis=1)
    r = REF.rasterize(verts, faces, pose, K, H, W)
    xc = verts.astype(np.float64) @ pose[:, :3].T + pose[:, 3]
    uv = (xc @ K.T)[:, :2] / xc[:, 2:]
    hull = _convex_hull(uv)
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    p = np.stack([jj.ravel(), ii.ravel()], 1)
    inside = np.ones(len(p), bool)
    for a, b in zip(hull, np.roll(hull, -1, axis=0)):
        inside &= (b[0] - a[0]) * (p[:, 1] - a[1]) - (b[1] - a[1]) * (p[:, 0] - a[0]) > 0
    assert inside.sum() > 1000
    assert (r["face"] >= 0).sum() == inside.sum()
    np.testing.assert_array_equal(r["face"] >= 0, inside)
    # the visible surface is the near one: the winning face's outward normal points at the camera
    c = xc[faces[r["face"][inside]]]
    n = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    n *= np.sign((n * (c.mean(1) - xc.mean(0))).sum(-1))[:, None]   # outward
    assert ((n * c[:, 0]).sum(-1) < 0).all()
