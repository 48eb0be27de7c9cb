"""GPU: tp_scene_bounds (K21), texpose_amd.scene_bounds.SceneBounds and tools/novel_views.py.

The blend is compared with tests/scene_bounds_ref.py (a numpy fp32 restatement of the rules; the reference has them inline next to a
PyTorch3D render and cannot be called) on identical inputs: labels, the blended depth and the 'render' bounds exactly.  The 'box'
bounds are bit-identical to what tp_raygen's TP_BOUNDS_AABB mode gives for the winning object's box, and agree with golden G23 and
the helper at the bar of test_gpu_parity.test_aabb_g3 / test_raygen_aabb_bounds (rtol 1e-6, atol 1e-6)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_bounds_ref as SB
from conftest import load_golden
from oracle import texpose_oracle as O
from test_gpu_surfel import K_for, pose_of, torus, uv_sphere

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BAR = dict(rtol=1e-6, atol=1e-6)          # test_aabb_g3, test_raygen_aabb_bounds
BG = (0.25, 30.0)
SCALE = 10.0


def cu(x):
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(DEV)


def camera(B, H, W, seed):
    sc = O.synthetic_scene(H, W, B=B, seed=seed)                     # object origin 8 units in front of the camera
    K = sc["intr"].clone()
    K[:, 0, 0] = K[:, 1, 1] = 700.0 * H / 128.0
    K[:, 0, 2], K[:, 1, 2] = W / 2.0 - 0.3, H / 2.0 + 0.2
    return sc["pose"].contiguous(), K.contiguous()


def synthetic_planes(K, B, H, W, rs):
    """[K,B,H,W] planes as the rasteriser writes them: -1 on background; some zeros, some exact ties between objects."""
    z = rs.uniform(400.0, 1500.0, size=(K, B, H, W)).astype(np.float32)
    z[rs.uniform(size=z.shape) < 0.6] = -1.0
    z[rs.uniform(size=z.shape) < 0.02] = 0.0
    if K > 1:
        tie = rs.uniform(size=(B, H, W)) < 0.05
        z[1][tie] = z[0][tie]
    return z


def random_boxes(K, rs):
    c = rs.uniform(-0.6, 0.6, size=(K, 1, 3))
    h = rs.uniform(0.2, 0.8, size=(K, 1, 3))
    return np.concatenate([c - h, c + h], axis=1).astype(np.float32)              # [K,2,3], far from the camera at distance 8


def all_rays(ops, pose, intr, H, W):
    B = pose.shape[0]
    every = torch.arange(H * W, device=DEV).expand(B, -1).contiguous()
    c, r, _, _, _ = ops.raygen(intr, pose, H=H, W=W, ray_idx=every)
    return c, r, every


def check_against_helper_and_raygen(ops, zbuf, boxes, ids, pose, intr, H, W):
    """All three sources of one scene.  Returns the 'box' result (numpy) and the helper's."""
    K, B = zbuf.shape[:2]
    zb, bx, idt = cu(zbuf), cu(boxes), cu(ids.astype(np.int32))
    c, r, every = all_rays(ops, pose, intr, H, W)
    rays = (c.cpu().numpy(), r.cpu().numpy())
    res = {}
    for source in ("box", "render", "none"):
        out = ops.scene_bounds(zb, bx, idt, depth_scale=SCALE, bg_range=BG, source=source, pose=pose, intr=intr)
        ref = SB.blend(zbuf.reshape(K, B, H * W), ids, source, SCALE, BG, boxes=boxes, rays=rays)
        assert out["label"].dtype == torch.int32 and out["label"].shape == (B, H * W)
        assert torch.equal(out["label"].cpu(), torch.from_numpy(ref["label"])), source
        assert torch.equal(out["depth"].cpu(), torch.from_numpy(ref["depth"])), source
        if source != "box":
            assert torch.equal(out["z_near"].cpu(), torch.from_numpy(ref["z_near"])), source
            assert torch.equal(out["z_far"].cpu(), torch.from_numpy(ref["z_far"])), source
        res[source] = ({k: v.cpu() for k, v in out.items()}, ref)
    out, ref = res["box"]
    owned = torch.from_numpy(ref["label"] > 0)
    winner = torch.from_numpy(ref["winner"])
    # unlabelled pixels: exactly the background range
    assert (out["z_near"][~owned] == np.float32(BG[0])).all() and (out["z_far"][~owned] == np.float32(BG[1])).all()
    # labelled pixels: bit-identical to the ray generation's own box bounds of the winning object (misses -> 0 there as here)
    seen = 0
    for k in range(K):
        m = owned & (winner == k)
        if not m.any():
            continue
        lo, hi = boxes[k, 0].tolist(), boxes[k, 1].tolist()
        _, _, zn, zf, _ = ops.raygen(intr, pose, H=H, W=W, ray_idx=every, aabb=(lo, hi), bg_range=(0.0, 0.0))
        assert torch.equal(out["z_near"][m], zn.cpu()[m]), k
        assert torch.equal(out["z_far"][m], zf.cpu()[m]), k
        seen += int(m.sum())
    assert seen == int(owned.sum()) > 0
    # and the helper's slab values on the same rays, at the bar of test_raygen_aabb_bounds
    print("box vs helper: max |d near| %.3g, max |d far| %.3g" % (float((out["z_near"] - torch.from_numpy(ref["z_near"])).abs().max()),
                                                                  float((out["z_far"] - torch.from_numpy(ref["z_far"])).abs().max())))
    torch.testing.assert_close(out["z_near"], torch.from_numpy(ref["z_near"]), **BAR)
    torch.testing.assert_close(out["z_far"], torch.from_numpy(ref["z_far"]), **BAR)
    return res


@pytest.fixture(scope="module")
def ops():
    from texpose_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("HW", [(37, 53), (128, 128)])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("K", [1, 3, 32])
def test_synthetic_planes(ops, K, B, HW):
    H, W = HW
    rs = np.random.RandomState(1000 * K + 10 * B + H)
    pose, intr = camera(B, H, W, seed=K + B)
    zbuf = synthetic_planes(K, B, H, W, rs)
    ids = (rs.permutation(K) + 1 + (K == 1) * 6).astype(np.int32)
    res = check_against_helper_and_raygen(ops, zbuf, random_boxes(K, rs), ids, cu(pose), cu(intr), H, W)
    out, ref = res["box"]
    assert (out["label"] == 0).any() or K == 32
    assert (out["label"] > 0).sum() > 100
    if K > 1:                                                       # ties between covered objects went to the lower index
        tie = (zbuf[0] == zbuf[1]) & (zbuf[0] > 0)
        first = torch.from_numpy((ref["winner"].reshape(B, H, W) != 1) | ~tie)
        assert tie.any() and first.all()


def test_box_bounds_agree_with_g23(ops):
    """Golden G23 (the reference's rays and slab values of 2 poses x 3 boxes at 24 x 32): whichever object owns a pixel, the kernel's
    bounds are the reference's slab values of that object's box, 0 where the reference's test is invalid."""
    g = load_golden("g23_scene_bounds")
    H, W, K, B = g["H"], g["W"], 3, 2
    rs = np.random.RandomState(23)
    zbuf = synthetic_planes(K, B, H, W, rs)
    ids = np.array([4, 9, 2], dtype=np.int32)
    pose, intr = cu(g["pose"]), cu(g["intr"])
    out = ops.scene_bounds(cu(zbuf), cu(g["boxes"]), cu(ids), depth_scale=float(g["depth_scale"]), bg_range=BG, source="box", pose=pose,
                           intr=intr)
    ref = SB.blend(zbuf.reshape(K, B, H * W), ids, "none", SCALE, BG)
    assert torch.equal(out["label"].cpu(), torch.from_numpy(ref["label"]))
    win = torch.from_numpy(ref["winner"])[None]
    ok = torch.gather(g["valid"], 0, win)[0] > 0
    tn = torch.where(ok, torch.gather(g["t_near"], 0, win)[0], torch.zeros(()))
    tf = torch.where(ok, torch.gather(g["t_far"], 0, win)[0], torch.zeros(()))
    owned = torch.from_numpy(ref["label"] > 0)
    assert (ok & owned).sum() > 50 and (~ok & owned).sum() > 50
    print("box vs G23: max |d near| %.3g, max |d far| %.3g" % (float((out["z_near"].cpu() - tn)[owned].abs().max()),
                                                               float((out["z_far"].cpu() - tf)[owned].abs().max())))
    torch.testing.assert_close(out["z_near"].cpu()[owned], tn[owned], **BAR)
    torch.testing.assert_close(out["z_far"].cpu()[owned], tf[owned], **BAR)
    # the same scene through the full comparison (helper on the kernel's rays, ray-gen bit identity)
    check_against_helper_and_raygen(ops, zbuf, g["boxes"].numpy(), ids, pose, intr, H, W)


def two_mesh_scene(H=120, W=160):
    """The sphere and the torus of the surfel tests in one scene frame: the torus sits 150 mm nearer to the camera and 30 mm to the
    side, so it hides a ring of the sphere while the sphere shows through its hole."""
    from texpose_amd.surfel import SurfelRenderer
    vs, fs = uv_sphere(24, 48)
    vt, ft = torus(48, 24)
    vt = (vt + np.array([30.0, 0.0, -150.0], dtype=np.float32)).astype(np.float32)
    objects = {5: (SurfelRenderer(vs, fs, None, H, W, DEV), vs.min(0), vs.max(0)),
               2: (SurfelRenderer(vt, ft, None, H, W, DEV), vt.min(0), vt.max(0))}
    # poses in NeRF units (t = 0.8 m * depth scale), nearly frontal so that the torus stays in front
    pose = np.stack([pose_of([0.1, -0.15, 0.3], [0.1, -0.05, 8.0]), pose_of([-0.2, 0.1, -0.4], [-0.2, 0.1, 8.3])])
    return objects, torch.from_numpy(pose), torch.from_numpy(K_for(H, W)), H, W


def test_real_meshes(ops):
    from texpose_amd.scene_bounds import SceneBounds
    objects, pose, K, H, W = two_mesh_scene()
    sb = SceneBounds(objects, H, W, SCALE, BG)
    r = sb(pose, K, "box")
    zbuf = r.zbuf.cpu().numpy()
    B = pose.shape[0]
    assert zbuf.shape == (2, B, H, W)
    cov = zbuf > 0
    label = r.label.cpu().view(B, H, W).numpy()
    for b in range(B):                                              # the inputs are what this test is about
        assert (label[b] == 5).sum() >= 200 and (label[b] == 2).sum() >= 200, (b, (label[b] == 5).sum(), (label[b] == 2).sum())
        assert (cov[0, b] & cov[1, b]).sum() >= 50, (b, (cov[0, b] & cov[1, b]).sum())
        assert (~cov[0, b] & ~cov[1, b]).sum() > 0
    assert torch.equal(r.object_mask.cpu(), r.label.cpu() > 0)
    assert r.depth_range[0].shape == (B, H * W, 1) and r.depth_range[1].shape == (B, H * W, 1)
    intr = cu(K)[None].expand(B, 3, 3).contiguous()
    check_against_helper_and_raygen(ops, zbuf, sb.boxes.cpu().numpy(), np.array(sb.object_ids, dtype=np.int32), cu(pose), intr, H, W)
    # the blended depth is the rasteriser's z of the nearer mesh, in NeRF units
    near_mm = np.where(cov, zbuf, np.float32(100000.0)).min(0)
    np.testing.assert_array_equal(r.depth.cpu().view(B, H, W).numpy()[near_mm < 1e5],
                                  ((near_mm / np.float32(1000)) * np.float32(SCALE))[near_mm < 1e5])
    # buffers are allocated once per batch size
    p0 = r.label.data_ptr()
    assert sb(pose, K, "render").label.data_ptr() == p0


def test_capture_replay_and_limits(ops):
    from texpose_amd import _lib
    K, B, H, W = 3, 2, 48, 64
    rs = np.random.RandomState(7)
    pose, intr = (cu(t) for t in camera(B, H, W, seed=4))
    zb = cu(synthetic_planes(K, B, H, W, rs))
    bx, ids = cu(random_boxes(K, rs)), cu(np.array([3, 1, 2], dtype=np.int32))
    for source in ("box", "render"):
        eager = ops.scene_bounds(zb, bx, ids, depth_scale=SCALE, bg_range=BG, source=source, pose=pose, intr=intr)
        static = {k: torch.zeros_like(v) for k, v in eager.items()}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ops.scene_bounds(zb, bx, ids, depth_scale=SCALE, bg_range=BG, source=source, pose=pose, intr=intr, out=static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ops.scene_bounds(zb, bx, ids, depth_scale=SCALE, bg_range=BG, source=source, pose=pose, intr=intr, out=static)
        for v in static.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(static[k], eager[k]), (source, k)
        # new planes behind the same pointers: the replay follows them
        zb2 = cu(synthetic_planes(K, B, H, W, rs))
        want = ops.scene_bounds(zb2, bx, ids, depth_scale=SCALE, bg_range=BG, source=source, pose=pose, intr=intr)
        keep = zb.clone()
        zb.copy_(zb2)
        graph.replay()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(static[k], want[k]), (source, k)
        zb.copy_(keep)
    # K = 33: the library's own error
    zb33 = torch.full((33, 1, 8, 8), -1.0, device=DEV)
    with pytest.raises(_lib.TexposeLibraryError, match="32"):
        ops.scene_bounds(zb33, torch.zeros(33, 2, 3, device=DEV), torch.ones(33, dtype=torch.int32, device=DEV), depth_scale=SCALE,
                         bg_range=BG, source="render")
    # shape / dtype / contiguity are checked, nothing is converted
    with pytest.raises(ValueError):
        ops.scene_bounds(zb.double(), bx, ids, depth_scale=SCALE, bg_range=BG, source="render")
    with pytest.raises(ValueError):
        ops.scene_bounds(zb.transpose(2, 3), bx, ids, depth_scale=SCALE, bg_range=BG, source="render")
    with pytest.raises(ValueError):
        ops.scene_bounds(zb, bx, ids.long(), depth_scale=SCALE, bg_range=BG, source="render")
    with pytest.raises(ValueError):
        ops.scene_bounds(zb, bx[:2], ids, depth_scale=SCALE, bg_range=BG, source="box", pose=pose, intr=intr)
    with pytest.raises(ValueError):
        ops.scene_bounds(zb, bx, ids, depth_scale=SCALE, bg_range=BG, source="sensor")


def small_graph(H, W, N, opaque=False):
    from texpose_amd.graph import Graph
    from texpose_amd.options import default_options
    opt = default_options(H=H, W=W, device=DEV)
    opt.nerf.sample_intvs, opt.nerf.sample_stratified = N, False
    opt.arch.mlp_precision = "fp32"
    graph = Graph(opt).to(DEV)
    params = O.make_params(3)
    if opaque:
        params["mlp_feat.7.bias"][0] = 200.0                       # static density softplus(~200) at every sample
    graph.nerf.load_state_dict({**graph.nerf.state_dict(), **{k: v.to(DEV) for k, v in params.items()}})
    graph.attach_latents(4, opt)
    return opt, graph


def torch_composed_bounds(zbuf, boxes, ids, pose, intr, H, W, bg):
    """What a user had to write before tp_scene_bounds: one box-range launch per object, then the stack / min / gather / where chain
    (zbuf [K,B,H,W] in mm, everything on the device)."""
    from texpose_amd.geometry import online_box_range
    K, B = zbuf.shape[:2]
    nears, fars = [], []
    for k in range(K):
        n, f = online_box_range(intr, pose, boxes[k, 0].cpu(), boxes[k, 1].cpu(), H, W, bg_range=(0.0, 0.0))
        nears.append(n); fars.append(f)
    z = zbuf.view(K, B, H * W)
    labels = (z > 0) * ids.view(K, 1, 1)
    zz = torch.where(z > 0, z, 100000 * torch.ones_like(z))
    _, idx = torch.min(zz, dim=0)
    pick = lambda t: torch.gather(t, 0, idx[None])[0]
    label = pick(labels)
    near = torch.where(label > 0, pick(torch.stack(nears)), torch.full_like(nears[0], bg[0]))
    far = torch.where(label > 0, pick(torch.stack(fars)), torch.full_like(fars[0], bg[1]))
    return near, far, label


def test_end_to_end_render_matches_torch_composed_bounds():
    from texpose_amd.scene_bounds import SceneBounds
    H = W = 64
    objects, pose, K, _, _ = two_mesh_scene(H, W)
    opt, graph = small_graph(H, W, 32)
    sb = SceneBounds(objects, H, W, SCALE, BG)
    pose1, intr1 = cu(pose[:1]), cu(K)[None]
    r = sb(pose1, intr1, "box")
    assert 200 < int(r.object_mask.sum()) < H * W
    light = torch.tensor(2, device=DEV)
    with torch.no_grad():
        ours = graph.render_by_slices(opt, pose1, intr=intr1, depth_range=r.depth_range, object_mask=r.object_mask, sample_idx=light, mode="eval")
        near, far, label = torch_composed_bounds(r.zbuf, sb.boxes, sb.ids, pose1, intr1, H, W, BG)
        assert torch.equal(label.int(), r.label)
        assert torch.equal(near, r.depth_range[0][..., 0]) and torch.equal(far, r.depth_range[1][..., 0])
        theirs = graph.render_by_slices(opt, pose1, intr=intr1, depth_range=(near[..., None], far[..., None]), object_mask=(label > 0).float(),
                                        sample_idx=light, mode="eval")
    for k in ("rgb", "depth", "opacity", "density"):
        assert torch.equal(ours[k], theirs[k]), k
    assert float(ours.opacity.sum()) > 0


def test_end_to_end_render_source_brackets_opaque_depth():
    from texpose_amd.scene_bounds import SceneBounds
    H = W = 64
    objects, pose, K, _, _ = two_mesh_scene(H, W)
    opt, graph = small_graph(H, W, 32, opaque=True)
    sb = SceneBounds(objects, H, W, SCALE, BG)
    pose1, intr1 = cu(pose[:1]), cu(K)[None]
    r = sb(pose1, intr1, "render")
    with torch.no_grad():
        ret = graph.render_by_slices(opt, pose1, intr=intr1, depth_range=r.depth_range, object_mask=r.object_mask,
                                     sample_idx=torch.tensor(0, device=DEV), mode="eval")
    m = r.label[0] > 0
    assert int(m.sum()) > 200
    d, zn, zf = ret.depth[0, :, 0][m], r.depth_range[0][0, :, 0][m], r.depth_range[1][0, :, 0][m]
    assert float(ret.opacity[0, :, 0][m].min()) > 0.999
    print("opaque depth: min (d - near) %.4g, min (far - d) %.4g" % (float((d - zn).min()), float((zf - d).min())))
    assert (d >= zn).all() and (d <= zf).all()
    # and the bounds are within 20 % of the mesh surface
    s = r.depth[0][m]
    assert torch.equal(zn, s * 0.8) and torch.equal(zf, s * 1.2)


def write_ascii_ply(path, verts, faces):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n" % len(verts))
        f.write("element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(faces))
        for v in verts:
            f.write("%r %r %r\n" % (float(v[0]), float(v[1]), float(v[2])))
        for t in faces:
            f.write("3 %d %d %d\n" % (int(t[0]), int(t[1]), int(t[2])))


def test_novel_views_tool(tmp_path):
    from PIL import Image
    from texpose_amd import checkpoint as ck
    H = W = 48
    N, n_views = 16, 3
    opt, graph = small_graph(H, W, N)
    ck.save_checkpoint(str(tmp_path / "model.ckpt"), graph, epoch=1, it=10)
    vs, fs = uv_sphere(12, 24)
    vt, ft = torus(24, 12)
    vt = (vt + np.array([30.0, 0.0, -150.0], dtype=np.float32)).astype(np.float32)
    write_ascii_ply(str(tmp_path / "sphere.ply"), vs, fs)
    write_ascii_ply(str(tmp_path / "torus.ply"), vt, ft)
    np.savez(str(tmp_path / "scene.npz"), pose_anchor=pose_of([0.1, -0.15, 0.3], [0.1, -0.05, 8.0]), intr=K_for(H, W))
    out = tmp_path / "novel_view"
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "tools", "novel_views.py"), "--checkpoint", str(tmp_path / "model.ckpt"),
           "--scene", str(tmp_path / "scene.npz"), "--ply", "5=" + str(tmp_path / "sphere.ply"), "--ply", "2=" + str(tmp_path / "torus.ply"),
           "--out", str(out), "--N", str(n_views), "--H", str(H), "--W", str(W), "--samples", str(N), "--precision", "fp32", "--source", "render"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    poses = np.load(str(out / "novel_pose.npy"))
    assert poses.shape == (n_views, 3, 4) and poses.dtype == np.float32
    for i in range(n_views):
        rgb = np.asarray(Image.open(str(out / ("rgb_%d.png" % i))))
        depth = np.asarray(Image.open(str(out / ("depth_%d.png" % i))))
        inv = np.asarray(Image.open(str(out / ("inv_depth_%d.png" % i))))
        assert rgb.shape == (H, W, 3) and rgb.dtype == np.uint8
        assert depth.shape == (H, W) and depth.dtype == np.uint16
        assert inv.shape == (H, W) and inv.dtype == np.uint8
        assert depth.max() < 2 * 2000 and rgb.any()              # metres x 2000 of an object 0.8 m away
    assert sorted(os.listdir(str(out))) == sorted(["novel_pose.npy"] + ["%s_%d.png" % (k, i) for k in ("rgb", "depth", "inv_depth") for i in range(n_views)])
