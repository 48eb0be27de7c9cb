"""GPU: the hard mesh rasteriser behind the surfel maps (tp_mesh_raster, texpose_amd.surfel) against the fp64 brute force of
tests/mesh_raster_ref.py on every pixel, against golden G21 (the reference's normals), against the NeRF's own rays, and end to
end through tools/surfel_maps.py and the decoding rules of the reference's data layer."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_raster_ref as REF
from texture_bake_ref import torus, uv_sphere  # noqa: F401  (other test modules import them from here)
from oracle.texpose_oracle import LINEMOD_K, rotation_from_axis_angle

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def soup(n, rs, extent=60.0):
    """Heavily overlapping triangles, each nearly parallel to the image plane at its own depth slab (no two intersect)."""
    z = rs.permutation(n) * 2.0 - n
    c = rs.uniform(-extent / 2, extent / 2, size=(n, 1, 2))
    xy = c + rs.uniform(-extent / 2, extent / 2, size=(n, 3, 2))
    zz = z[:, None] + rs.uniform(-0.4, 0.4, size=(n, 3))
    v = np.concatenate([xy, zz[..., None]], -1).reshape(-1, 3)
    return v.astype(np.float32), np.arange(3 * n).reshape(n, 3).astype(np.int32)


def pose_of(w, t):
    return np.concatenate([rotation_from_axis_angle(np.asarray(w, dtype=np.float64)), np.asarray(t, dtype=np.float64)[:, None]],
                          axis=1).astype(np.float32)


def K_for(H, W, f=None, dc=(0.0, 0.0)):
    K = np.array(LINEMOD_K, dtype=np.float64)
    K[:2] *= H / 128.0                                               # crop-like: the object fills much of a small image
    if f is not None:
        K[0, 0] = K[1, 1] = f
    K[0, 2], K[1, 2] = W / 2.0 + dc[0], H / 2.0 + dc[1]
    return K.astype(np.float32)


def gpu_raster(verts, faces, pose, K, H, W, vcolor=None, nocs_norm=None, normals=False):
    from texpose_amd import ops
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    r = ops.mesh_raster(t(verts), t(faces), t(pose), t(K), H=H, W=W, vcolor=None if vcolor is None else t(vcolor),
                        nocs_norm=nocs_norm, face_ids=True, normals=normals)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def check_against_bruteforce(verts, faces, pose, K, H, W, vcolor=None, nocs=True, pixels=None, min_hit=1):
    """Every requested pixel of every image: face ids agree on >= 99.9 % and every disagreement sits on an edge (min barycentric
    < 1e-5 in fp64 of a face involved); where they agree, zbuf to 1e-5 relative, rgb / nocs to 1e-5."""
    norm = REF.nocs_normalisation(verts) if nocs else None
    norm32 = None if norm is None else tuple(np.asarray(x, dtype=np.float32) for x in norm)
    g = gpu_raster(verts, faces, pose, K, H, W, vcolor, norm32)
    B = pose.shape[0]
    Ks = np.broadcast_to(K, (B, 3, 3)) if K.ndim == 2 else K
    hits = 0
    for b in range(B):
        pix = np.arange(H * W) if pixels is None else pixels
        r = REF.rasterize(verts, faces, pose[b], Ks[b], H, W, pixels=pix, vcolor=vcolor, nocs_norm=norm32)
        gf = g["face"][b].reshape(-1)[pix]
        agree = gf == r["face"]
        assert agree.mean() >= 0.999, (b, agree.mean())
        for p in np.nonzero(~agree)[0]:
            m = []
            if r["face"][p] >= 0:
                m.append(r["min_bary"][p])
            if gf[p] >= 0:
                m.append(REF.face_bary_at(verts, faces, pose[b], Ks[b], W, [gf[p]], [pix[p]]).min())
            assert min(m) < 1e-5, (b, pix[p], gf[p], r["face"][p], m)
        hit = agree & (gf >= 0)
        hits += hit.sum()
        gz = g["zbuf"][b].reshape(-1)[pix]
        np.testing.assert_allclose(gz[hit], r["zbuf"][hit], rtol=1e-5)
        assert (gz[agree & (gf < 0)] == -1).all()
        for key in ("rgb", "nocs"):
            if key in r:
                np.testing.assert_allclose(g[key][b].reshape(-1, 3)[pix][agree], r[key][agree], rtol=0, atol=1e-5)
    assert hits >= min_hit
    return g


def test_uv_sphere_random_colours():
    rs = np.random.RandomState(0)
    v, f = uv_sphere(24, 48, ripple=0.1)
    col = rs.uniform(size=v.shape).astype(np.float32)
    check_against_bruteforce(v, f, pose_of([0.3, -0.5, 0.2], [4, -3, 620])[None], K_for(120, 160), 120, 160, vcolor=col, min_hit=2000)


def test_torus_self_occluding():
    v, f = torus(48, 24)
    check_against_bruteforce(v, f, pose_of([1.2, 0.2, 0.0], [0, 5, 560])[None], K_for(120, 160), 120, 160, min_hit=1500)


def test_triangle_soup_heavy_overlap():
    rs = np.random.RandomState(1)
    v, f = soup(400, rs)
    col = rs.uniform(size=v.shape).astype(np.float32)
    check_against_bruteforce(v, f, pose_of([0.05, -0.03, 0.4], [0, 0, 900])[None], K_for(120, 160), 120, 160, vcolor=col, min_hit=3000)


def test_batch_of_poses_with_different_intrinsics():
    rs = np.random.RandomState(2)
    v, f = uv_sphere(16, 32, ripple=0.15)
    col = rs.uniform(size=v.shape).astype(np.float32)
    pose = np.stack([pose_of(rs.uniform(-2, 2, 3), [rs.uniform(-10, 10), rs.uniform(-10, 10), rs.uniform(500, 800)]) for _ in range(5)])
    K = np.stack([K_for(64, 80, f=rs.uniform(250, 400), dc=rs.uniform(-5, 5, 2)) for _ in range(5)])
    check_against_bruteforce(v, f, pose, K, 64, 80, vcolor=col, min_hit=2000)


@pytest.mark.parametrize("H,W", [(37, 53), (120, 160)])
def test_odd_and_plain_sizes(H, W):
    rs = np.random.RandomState(3)
    v, f = uv_sphere(12, 24, ripple=0.2)
    col = rs.uniform(size=v.shape).astype(np.float32)
    check_against_bruteforce(v, f, pose_of([0.7, 0.1, -0.4], [2, 1, 650])[None], K_for(H, W), H, W, vcolor=col, min_hit=200)


def test_mesh_partly_and_entirely_outside():
    rs = np.random.RandomState(4)
    v, f = uv_sphere(16, 32)
    col = rs.uniform(size=v.shape).astype(np.float32)
    K = K_for(96, 128)
    g = check_against_bruteforce(v, f, pose_of([0.2, 0.4, 0.0], [95, -60, 600])[None], K, 96, 128, vcolor=col, min_hit=200)
    assert (g["face"] < 0).mean() > 0.5
    g = gpu_raster(v, f, pose_of([0.2, 0.4, 0.0], [900, 0, 600])[None], K, 96, 128, col, REF.nocs_normalisation(v), normals=True)
    assert (g["face"] == -1).all() and (g["zbuf"] == -1).all()
    assert (g["rgb"] == 0).all() and (g["nocs"] == 0).all() and (g["normal"] == 0).all()


def test_large_image_20k_faces_strided():
    rs = np.random.RandomState(5)
    v, f = uv_sphere(71, 144, radius=90.0, ripple=0.08)
    assert len(f) >= 20000
    col = rs.uniform(size=v.shape).astype(np.float32)
    pixels = np.arange(0, 480 * 640, 31)
    check_against_bruteforce(v, f, pose_of([0.4, -0.9, 0.3], [10, -5, 700])[None], K_for(480, 640, f=1400.0), 480, 640, vcolor=col,
                             pixels=pixels, min_hit=1500)


def test_more_than_100k_faces_in_one_tile():
    rs = np.random.RandomState(6)
    n, H, W = 120000, 64, 96
    K = np.array([[100.0, 0, 0.0], [0, 100.0, 0.0], [0, 0, 1]], dtype=np.float32)       # identity pose: pixel = 100 x/z
    z = (400.0 + rs.permutation(n) * 0.01).astype(np.float64)
    c = np.stack([rs.uniform(32.5, 47.5, n), rs.uniform(16.5, 31.5, n)], 1)             # the tile of columns 32-47, rows 16-31
    uv = c[:, None] + rs.uniform(-1.6, 1.6, size=(n, 3, 2))
    v = np.concatenate([uv / 100.0 * z[:, None, None], np.broadcast_to(z[:, None, None], (n, 3, 1))], -1).reshape(-1, 3)
    v, f = v.astype(np.float32), np.arange(3 * n).reshape(n, 3).astype(np.int32)
    col = rs.uniform(size=v.shape).astype(np.float32)
    pose = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)[None]
    tile = np.array([i * W + j for i in range(14, 34) for j in range(30, 50)])           # the tile and a ring around it
    g = check_against_bruteforce(v, f, pose, K, H, W, vcolor=col, nocs=False, pixels=tile, min_hit=250)
    assert (g["face"].reshape(-1)[np.setdiff1d(np.arange(H * W), tile)] == -1).all()


def test_normals_match_restatement_and_g21(golden):
    from texpose_amd import ops
    rs = np.random.RandomState(7)
    v, f = torus(64, 32)
    pose = np.stack([pose_of([1.0, 0.3, 0.2], [3, -4, 600]), pose_of([0.2, -1.1, 0.5], [-6, 2, 520])])
    K = K_for(96, 128)
    g = gpu_raster(v, f, pose, K, 96, 128, normals=True)
    for b in range(2):
        ref = REF.normal_from_depth(g["zbuf"][b], pose[b], K)
        np.testing.assert_allclose(g["normal"][b], ref, rtol=0, atol=1e-5)
        assert (np.abs(ref).sum(-1) > 0).sum() > 1000
    d = golden("g21_surfel_normals")
    n = ops.normals_from_depth(d["depth"][None].to(DEV), d["pose"][None].to(DEV), d["K"][None].to(DEV))
    np.testing.assert_allclose(n[0].cpu().numpy(), d["normal"].numpy(), rtol=0, atol=1e-5)
    del rs


def test_alignment_with_the_nerf_rays():
    """centre + ray * zbuf from the trainer's own ray generation lies on the plane of the face the kernel reports, inside it."""
    from texpose_amd import ops
    v, f = uv_sphere(20, 40, ripple=0.15)
    H, W = 96, 128
    pose = np.stack([pose_of([0.6, -0.2, 0.9], [5, -7, 640]), pose_of([-1.3, 0.4, 0.1], [-9, 3, 580])])
    K = np.stack([K_for(H, W), K_for(H, W, f=300.0, dc=(3.3, -2.1))])
    g = gpu_raster(v, f, pose, K, H, W)
    idx = torch.arange(H * W, device=DEV)[None].expand(2, -1).contiguous()
    center, ray, _, _, _ = ops.raygen(torch.from_numpy(K).to(DEV), torch.from_numpy(pose).to(DEV), H=H, W=W, ray_idx=idx)
    center, ray = center.cpu().numpy().astype(np.float64), ray.cpu().numpy().astype(np.float64)
    for b in range(2):
        fid = g["face"][b].reshape(-1)
        hit = np.nonzero(fid >= 0)[0]
        assert len(hit) > 1000
        z = g["zbuf"][b].reshape(-1)[hit].astype(np.float64)
        X = center[b, hit] + ray[b, hit] * z[:, None]
        tri = v[f[fid[hit]]].astype(np.float64)                      # [P,3,3] object frame
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        dist = np.abs((n * (X - tri[:, 0])).sum(-1))
        assert (dist <= 1e-4 * z).all(), dist.max()
        # inside: barycentrics of X in the face's plane
        e0, e1, p = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], X - tri[:, 0]
        d00, d01, d11 = (e0 * e0).sum(-1), (e0 * e1).sum(-1), (e1 * e1).sum(-1)
        d20, d21 = (p * e0).sum(-1), (p * e1).sum(-1)
        den = d00 * d11 - d01 * d01
        l1, l2 = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
        lam = np.stack([1 - l1 - l2, l1, l2], -1)
        # distance outside the face (barycentric x altitude), against the same 1e-4 x depth: the rays are fp32 differences of
        # ~600 mm world points (ray error ~6e-5, i.e. ~0.04 mm at the surface), as the reference's own rays are
        area2 = np.linalg.norm(np.cross(e0, e1), axis=-1)
        opp = np.stack([tri[:, 2] - tri[:, 1], tri[:, 0] - tri[:, 2], tri[:, 1] - tri[:, 0]], 1)
        alt = area2[:, None] / np.linalg.norm(opp, axis=-1)
        outside = np.maximum(-lam, 0) * alt
        assert (outside.max(-1) <= 1e-4 * z).all(), outside.max()
        assert (lam.min(-1) > 0).mean() > 0.95


def test_determinism_capture_and_mask():
    from texpose_amd import ops
    from texpose_amd.surfel import SurfelRenderer
    rs = np.random.RandomState(8)
    v, f = soup(300, rs)
    col = rs.uniform(size=v.shape).astype(np.float32)
    vt, ft, ct = (torch.from_numpy(x).to(DEV) for x in (v, f, col))
    pose = torch.from_numpy(np.stack([pose_of([0.05, 0.0, 0.3], [0, 0, 900]), pose_of([0.0, 0.08, -0.2], [3, 1, 950])])).to(DEV)
    K = torch.from_numpy(K_for(120, 160)).to(DEV)
    norm = REF.nocs_normalisation(v)
    run = lambda: ops.mesh_raster(vt, ft, pose, K, H=120, W=160, vcolor=ct, nocs_norm=norm, face_ids=True, normals=True)
    a, b = run(), run()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = run()
    for t in c.values():
        t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], c[k]), k
    out = SurfelRenderer(v, f, col, 120, 160, DEV)(pose.cpu(), K.cpu(), 1000.0)
    assert torch.equal(out.mask_syn, (out.depth > 0).float())
    assert out.mask_syn.sum() > 1000 and out.rgb_syn.shape == (2, 3, 120, 160) and out.normal.shape == (2, 3, 120, 160)


def _write_binary_ply(path, v, f, col):
    head = "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" \
           "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\nproperty list uchar int vertex_indices\n" \
           "end_header\n" % (len(v), len(f))
    with open(path, "wb") as fh:
        fh.write(head.encode())
        for k in range(len(v)):
            fh.write(struct.pack("<3f3B", *v[k], *col[k]))
        for k in range(len(f)):
            fh.write(struct.pack("<B3i", 3, *f[k]))


def test_surfel_maps_tool_end_to_end(tmp_path):
    from PIL import Image
    from texpose_amd.surfel import SurfelRenderer, load_ply
    rs = np.random.RandomState(9)
    v, f = uv_sphere(18, 36, ripple=0.1)
    col8 = rs.randint(0, 256, size=v.shape).astype(np.uint8)
    ply = str(tmp_path / "obj_000001.ply")
    _write_binary_ply(ply, v, f, col8)
    depth_scale = 10.0
    pose = np.stack([pose_of(rs.uniform(-2, 2, 3), [rs.uniform(-0.1, 0.1), rs.uniform(-0.1, 0.1), rs.uniform(6.0, 7.5)]) for _ in range(3)])
    frames = np.array([3, 29, 117])
    K = K_for(120, 160)
    np.savez(str(tmp_path / "poses.npz"), frame_index=frames, pose=pose, intr=K)
    out_dir = str(tmp_path / "seq")
    cmd = [sys.executable, os.path.join(REPO, "tools", "surfel_maps.py"), "--ply", ply, "--poses", str(tmp_path / "poses.npz"),
           "--depth-scale", str(depth_scale), "--H", "120", "--W", "160", "--loop", "1", "--out", out_dir, "--batch", "2"]
    res = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    verts, faces, vcolor = load_ply(ply)
    want = SurfelRenderer(verts, faces, vcolor, 120, 160, DEV)(torch.from_numpy(pose), torch.from_numpy(K), depth_scale)
    for b, fr in enumerate(frames):
        name = "%06d" % fr
        # data/lm.py:212-214: cv2.imread(-1)[..., :3][..., [2, 1, 0]] = the file's R, G, B; to_tensor / 255; alpha > 0
        rgba = np.asarray(Image.open(os.path.join(out_dir, "rgbsyn_1", name + ".png")))
        image = rgba[..., :3].astype(np.float32).transpose(2, 0, 1) / 255.0
        alpha = (rgba[..., 3] > 0).astype(np.float32)
        # :231: cv2.imread(-1)[..., [2, 1, 0]] / 255 (smooth_geo not applied)
        nocs = np.asarray(Image.open(os.path.join(out_dir, "nocs_1", name + ".png"))).astype(np.float32).transpose(2, 0, 1) / 255.0
        normal = np.load(os.path.join(out_dir, "normal_1", name + ".npz"))["data"].transpose(2, 0, 1)
        np.testing.assert_array_equal(alpha, want.mask_syn[b].cpu().numpy())
        assert alpha.sum() > 500
        assert np.abs(image - want.rgb_syn[b].cpu().numpy()).max() <= 1.0 / 255 + 1e-6
        assert np.abs(nocs - want.nocs[b].cpu().numpy()).max() <= 1.0 / 255 + 1e-6
        np.testing.assert_allclose(normal, want.normal[b].cpu().numpy(), rtol=0, atol=1e-6)
