"""No GPU: the fp64 restatement of K27 (tests/texture_bake_ref.py) and the host side of texpose_amd.texture_bake against independent
geometry -- a round trip through the brute-force rasteriser, visibility against exact ray casting, and the helpers."""
import numpy as np
import pytest

import mesh_raster_ref as RAST
import texture_bake_ref as REF
from texpose_amd import _lib
from texpose_amd import texture_bake as TB
from texpose_amd.surfel import load_ply

DIST = 400.0
# (name, mesh, H, W, focal, views)
CASES = {
    "sphere64": (lambda: REF.uv_sphere(12, 16), 64, 64, 200.0, 14),
    "sphere37x53": (lambda: REF.uv_sphere(12, 16), 37, 53, 120.0, 14),
    "torus": (lambda: REF.torus(24, 12), 64, 80, 200.0, 14),
    "ripple": (lambda: REF.uv_sphere(20, 24, ripple=0.15), 96, 96, 300.0, 20),
}
_cache = {}


def baked(name):
    """Render the coloured mesh with the brute-force rasteriser at Fibonacci views and bake it with the restatement: once per case."""
    if name not in _cache:
        mesh, H, W, f, n = CASES[name]
        verts, faces = mesh()
        col = REF.test_colours(verts)
        poses, K = TB.sphere_view_poses(n, DIST).astype(np.float32), REF.pinhole(H, W, f)
        rgb, zbuf = np.zeros((n, H, W, 3), dtype=np.float32), np.zeros((n, H, W), dtype=np.float32)
        for b in range(n):
            r = RAST.rasterize(verts, faces, poses[b], K, H, W, vcolor=col)
            rgb[b], zbuf[b] = r["rgb"].reshape(H, W, 3), r["zbuf"].reshape(H, W)
        normals = TB.vertex_normals(verts, faces)
        out = REF.bake(verts, normals, poses, K, rgb, zbuf)
        _cache[name] = dict(verts=verts, faces=faces, col=col, poses=poses, K=K, H=H, W=W, normals=normals, rgb=rgb, zbuf=zbuf, out=out)
    return _cache[name]


# measured with this reference on these inputs (max |baked - vertex colour|; every vertex seen), cap 0.03:
#   sphere64 0.0080, sphere37x53 0.0188, torus 0.0110, ripple 0.0094
@pytest.mark.parametrize("name", list(CASES))
def test_round_trip(name):
    c = baked(name)
    vcolor, seen = REF.vcolor_of(c["out"]["acc"])
    err = np.abs(vcolor - c["col"])[seen].max()
    print(name, "round-trip max error %.4f, seen %d of %d" % (err, seen.sum(), len(seen)))
    assert seen.all()
    assert err <= 0.03


# measured (caps: 5 % of the occluded front-facing pairs, 2 % of the visible ones): torus 2 of 117 occluded pairs contributed, 2 of
# 1,140 visible pairs dropped; ripple 1 of 239 and 25 of 2,483; sphere64 no occluded pair, 0 of 693 -- all at silhouettes of the
# occluder, where part of the 2 x 2 footprint is legitimately free.  Front-facing: z > 0 and c >= cos_min; occluded: a non-incident
# face more than 5 mm nearer on the ray to the vertex; visible: no such face at all, c >= 0.35, projection >= 2 px inside the image
@pytest.mark.parametrize("name", ["torus", "ripple", "sphere64"])
def test_visibility_against_ray_casting(name):
    c = baked(name)
    verts, faces, out = c["verts"].astype(np.float64), c["faces"], c["out"]
    V, H, W = len(verts), c["H"], c["W"]
    skip = REF.incident(faces, V)
    occluded = contributed = visible = dropped = 0
    for b, P in enumerate(c["poses"].astype(np.float64)):
        R, t = P[:, :3], P[:, 3]
        centre = -R.T @ t
        s = REF.ray_hits(centre, verts, verts, faces, skip)
        x = verts @ R.T + t
        dist = np.linalg.norm(x, axis=1)
        cosv = -((c["normals"].astype(np.float64) @ R.T) * x).sum(1) / dist
        q = x @ c["K"].astype(np.float64).T
        u, v = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        front = (x[:, 2] > 0) & (cosv >= 0.3)
        occ = front & (s < 1) & ((1 - s) * dist > 5.0)
        free = ~(s < 1) & (x[:, 2] > 0) & (cosv >= 0.35) & (u >= 2) & (u <= W - 2) & (v >= 2) & (v <= H - 2)
        occluded += occ.sum()
        contributed += (occ & out["used"][:, b]).sum()
        visible += free.sum()
        dropped += (free & ~out["used"][:, b]).sum()
    print(name, "occluded but contributed %d of %d, visible but dropped %d of %d" % (contributed, occluded, dropped, visible))
    assert visible > 500
    assert contributed <= 0.05 * occluded
    assert dropped <= 0.02 * visible
    if name != "sphere64":
        assert occluded > 50                                         # the case does exercise occlusion


def test_write_ply_round_trip(tmp_path):
    verts, faces = REF.torus(8, 5)
    col = np.random.RandomState(0).randint(0, 256, size=(len(verts), 3)).astype(np.float32) / 255.0
    path = str(tmp_path / "t.ply")
    TB.write_ply(path, verts, faces, col)
    v, f, c = load_ply(path)
    assert v.dtype == np.float32 and (v == verts).all() and (f == faces).all()
    assert c is not None and c.shape == col.shape and (c == col).all()
    TB.write_ply(path, verts, faces, col * 3 - 1)                      # out of range: clamped, not wrapped
    c2 = load_ply(path)[2]
    assert c2.min() == 0 and c2.max() == 1
    with pytest.raises(ValueError):
        TB.write_ply(path, verts, faces, col[:-1])


def test_vertex_normals_on_a_sphere():
    verts, faces = REF.uv_sphere(12, 16)
    n = TB.vertex_normals(verts, faces)
    radial = verts / np.linalg.norm(verts, axis=1, keepdims=True)
    # "within 1e-2 of the radial direction" is read as 1 - n . r <= 1e-2, the reading under which area weighting can meet it on this
    # mesh.  Measured: 8.9e-3 at the poles (uv_sphere keeps 16 coincident pole vertices, each in ONE face, so its normal is that
    # face's: 7.6 degrees off), 1.2e-3 at the first ring, 0 on the equator.  As a Euclidean distance |n - r| the same normals are
    # 0.133 at the poles and 0.050 at the first ring: area weighting on rings of unequal height is that far off, at any welding.
    dev = (1.0 - (n.astype(np.float64) * radial).sum(1)).max()
    print("vertex normals vs radial: 1 - cos %.2e, |n - r| %.2e" % (dev, np.linalg.norm(n - radial, axis=1).max()))
    assert n.dtype == np.float32 and np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-6)
    assert dev <= 1e-2
    assert (n * radial).sum(1).min() > 0                               # outward, as the mesh is wound
    # a vertex without faces: zero normal (no view passes cos_min with it)
    n2 = TB.vertex_normals(np.concatenate([verts, [[1.0, 2.0, 3.0]]]), faces)
    assert (n2[-1] == 0).all() and (n2[:-1] == n).all()


def test_sphere_view_poses():
    for n in (1, 6, 14):
        P = TB.sphere_view_poses(n, 400.0)
        assert P.shape == (n, 3, 4)
        for R, t in zip(P[:, :, :3], P[:, :, 3]):
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(R), 1.0)
            assert np.allclose(t, [0, 0, 400.0], atol=1e-9)            # the origin sits on the optical axis at distance_mm
            assert np.isclose(np.linalg.norm(-R.T @ t), 400.0)
    centres = np.stack([-R.T @ t for R, t in zip(P[:, :, :3], P[:, :, 3])])
    assert centres[:, 2].max() > 300 and centres[:, 2].min() < -300     # both hemispheres
    import torch
    back = TB.poses_to_mm(TB.poses_to_nerf_units(torch.from_numpy(P), 10.0), 10.0)
    assert torch.allclose(back, torch.from_numpy(P), atol=1e-9)
    assert torch.allclose(TB.poses_to_nerf_units(torch.from_numpy(P), 10.0)[:, :, 3], torch.from_numpy(P[:, :, 3]) / 100.0)
    with pytest.raises(ValueError):
        TB.sphere_view_poses(0, 400.0)


def test_fill_unseen_strip_and_island():
    # a strip of 8 quads along x: vertices 2k (bottom) and 2k + 1 (top) at x = k; an isolated triangle after it
    k = np.arange(9)
    verts = np.concatenate([np.stack([k, 0 * k, 0 * k], 1), np.stack([k, 0 * k + 1, 0 * k], 1)]).astype(np.float32)
    bot, top = np.arange(9), 9 + np.arange(9)
    faces = np.concatenate([np.stack([bot[:-1], bot[1:], top[1:]], 1), np.stack([bot[:-1], top[1:], top[:-1]], 1)])
    faces = np.concatenate([faces, [[18, 19, 20]]])
    col = np.zeros((21, 3))
    col[:, 0] = np.concatenate([k, k, [0, 0, 0]]) / 8.0
    seen = np.ones(21, dtype=bool)
    run = [3, 4, 5, 9 + 3, 9 + 4, 9 + 5]                                # columns 3 .. 5 unseen
    seen[run] = False
    seen[18:] = False                                                  # the island: no seen vertex in its component
    col[~seen] = 0
    out, done, filled = TB.fill_unseen(col, seen, faces)
    assert filled == 6 and done[:18].all() and not done[18:].any() and (out[18:] == 0).all()
    assert (out[seen] == col[seen].astype(np.float32)).all()           # seen vertices are not touched
    assert (out[run, 0] > 2 / 8.0 - 1e-6).all() and (out[run, 0] < 6 / 8.0 + 1e-6).all()     # means of their neighbours
    assert abs(out[4, 0] - 0.5) < 0.1 and abs(out[13, 0] - 0.5) < 0.1   # the middle column, filled in the second sweep
    again = TB.fill_unseen(col, seen, faces)
    assert (again[0] == out).all() and again[2] == filled              # deterministic
    none = TB.fill_unseen(col, np.zeros(21, dtype=bool), faces)
    assert none[2] == 0 and not none[1].any()


def test_binding_is_derived_from_the_header():
    assert "tp_texture_bake" in _lib.SYMBOLS and "tp_texture_bake_workspace_bytes" in _lib.SYMBOLS
    fields = [f[0] for f in _lib.TextureBakeArgs._fields_]
    assert fields == ["verts", "normals", "pose", "intr", "rgb", "zbuf", "weight", "V", "B", "H", "W", "clear", "cos_min", "cover_min",
                      "z_tol_mm", "slope", "acc", "count", "workspace"]
    assert TB.THRESHOLDS == REF.DEFAULTS


def test_slice_rule_and_refusals_without_a_gpu():
    import ctypes as C
    lib = _lib.load()
    S = lib.tp_texture_bake_slices
    rule = lambda V, B: -(-B // min(B, max(4, -(-B // -(-65536 // V)))))
    for V, B in [(1, 1), (1, 14), (257, 14), (504, 14), (504, 13), (5000, 64), (20000, 64), (200000, 64), (65536, 8), (3, 65535)]:
        assert S(V, B) == rule(V, B), (V, B)
        assert lib.tp_texture_bake_workspace_bytes(V, B) == S(V, B) * V * 36
    assert (S(504, 14), S(20000, 64), S(200000, 64)) == (4, 4, 1)
    assert S(0, 4) == 0 and S(4, 0) == 0 and lib.tp_texture_bake_workspace_bytes(0, 4) == 0
    a = _lib.TextureBakeArgs()
    assert lib.tp_texture_bake(C.byref(a), None) == -1 and b"null pointer" in lib.tp_last_error()
