"""GPU: tp_scene_annotate (K22), tp_view_images, SceneBounds.annotate, the BOP scene writer and tools/novel_views.py --bop.

Both kernels are compared with tests/scene_annotate_ref.py (numpy restatement of the rules) on identical inputs; every comparison is
torch.equal: the annotations are integers, the image rules single rounded fp32 steps."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_annotate_ref as SA
from test_gpu_scene_bounds import BG, SCALE, cu, small_graph, synthetic_planes, write_ascii_ply
from test_gpu_surfel import K_for, pose_of, torus, uv_sphere

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F = np.float32


@pytest.fixture(scope="module")
def ops():
    from texpose_amd import ops as _ops
    return _ops


def device_label(ops, zb, ids):
    """label as K21 writes it (source 'none' needs no camera)."""
    return ops.scene_bounds(zb, None, ids, depth_scale=SCALE, bg_range=BG, source="none")["label"]


def check_against_helper(ops, zbuf, ids):
    K, B, H, W = zbuf.shape
    zb, idt = cu(zbuf), cu(np.asarray(ids, dtype=np.int32))
    label = device_label(ops, zb, idt)
    info, mask, vis = (torch.from_numpy(x) for x in SA.annotate(zbuf, label.cpu().numpy(), ids))
    # into buffers full of garbage: the call initialises info itself
    out = dict(info=torch.full((B, K, 10), 12345, dtype=torch.int32, device=DEV), mask=torch.full((B, K, H, W), 7, dtype=torch.uint8, device=DEV),
               mask_visib=torch.full((B, K, H, W), 9, dtype=torch.uint8, device=DEV))
    got = ops.scene_annotate(zb, label, idt, out=out)
    assert got["info"].data_ptr() == out["info"].data_ptr()
    assert torch.equal(got["info"].cpu(), info) and torch.equal(got["mask"].cpu(), mask) and torch.equal(got["mask_visib"].cpu(), vis)
    # the mask stacks skipped: the same info, nothing else
    lean = ops.scene_annotate(zb, label, idt, masks=False)
    assert sorted(lean) == ["info"] and lean["info"].dtype == torch.int32 and torch.equal(lean["info"].cpu(), info)
    # twice into the same buffer: nothing accumulates across calls
    again = ops.scene_annotate(zb, label, idt, out=out)
    assert torch.equal(again["info"].cpu(), info)
    return info, label


@pytest.mark.parametrize("HW", [(37, 53), (128, 128)])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("K", [1, 3, 32])
def test_synthetic_planes(ops, K, B, HW):
    H, W = HW
    rs = np.random.RandomState(2000 * K + 10 * B + H)
    zbuf = synthetic_planes(K, B, H, W, rs)
    zbuf[rs.uniform(size=zbuf.shape) < 0.01] = np.nan
    if K == 32:
        zbuf[K - 1, 0] = -1.0                                       # an absent object
    if K > 1:
        zbuf[K - 2, B - 1] = -1.0
        zbuf[K - 2, B - 1, H - 1, W - 1] = 10.0                     # a one-pixel object in the last corner, nearer than anything
    ids = (rs.permutation(K) + 1 + (K == 1) * 6).astype(np.int32)
    info, label = check_against_helper(ops, zbuf, ids)
    assert (info[..., 0] > 0).any() and (info[..., 1] < info[..., 0]).any() == (K > 1)
    if K == 32:
        assert info[0, K - 1].tolist() == [0, 0] + [-1] * 8
    if K > 1:
        assert info[B - 1, K - 2].tolist() == [1, 1] + [W - 1, H - 1] * 4
    # every covered pixel is visible for exactly one object
    assert int(info[..., 1].sum()) == int((label > 0).sum())


def mesh_scene(H=72, W=96):
    """The sphere and the torus of the surfel tests, four placements in one scene frame (poses chosen with tests/mesh_raster_ref.py):
    sphere 5 at the origin, partly hidden by torus 2, which sits 150 mm nearer and runs over the image border; sphere 8, small, behind
    sphere 5 and fully hidden; sphere 3 up and to the side, across the right border in view 0 and the top border in view 1."""
    from texpose_amd.surfel import SurfelRenderer
    vs, fs = uv_sphere(16, 32)
    vt, ft = torus(32, 16)
    sh = lambda v, d, s=1.0: (v * s + np.array(d, dtype=F)).astype(F)
    meshes = {5: (vs, fs), 2: (sh(vt, [30.0, 0.0, -150.0]), ft), 8: (sh(vs, [-5.0, 5.0, 120.0], 0.3), fs), 3: (sh(vs, [125.0, -75.0, 40.0], 0.7), fs)}
    objects = {i: (SurfelRenderer(v, f, None, H, W, DEV), v.min(0), v.max(0)) for i, (v, f) in meshes.items()}
    pose = np.stack([pose_of([0.1, -0.15, 0.3], [0.1, -0.05, 8.0]), pose_of([-0.2, 0.1, -0.4], [-0.2, 0.1, 8.3])])
    return objects, meshes, torch.from_numpy(pose), torch.from_numpy(K_for(H, W)), H, W


def test_real_meshes(ops):
    from texpose_amd.scene_bounds import SceneBounds
    objects, _, pose, K, H, W = mesh_scene()
    sb = SceneBounds(objects, H, W, SCALE, BG)
    r = sb(pose, K, "box")
    ann = sb.annotate(r)
    B, n = pose.shape[0], len(objects)
    assert ann.info.shape == (B, n, 10) and ann.mask.shape == (B, n, H, W) and ann.mask_visib.dtype == torch.uint8
    info, mask, vis = (torch.from_numpy(x) for x in SA.annotate(r.zbuf.cpu().numpy(), r.label.cpu().numpy(), sb.object_ids))
    assert torch.equal(ann.info.cpu(), info) and torch.equal(ann.mask.cpu(), mask) and torch.equal(ann.mask_visib.cpu(), vis)
    # the inputs are what this test is about: a partly hidden, a fully hidden and a border-crossing object in every view
    assert sb.object_ids == [5, 2, 8, 3]
    n_all, n_vis = info[..., 0], info[..., 1]
    print("px_count_all", n_all.tolist(), "px_count_visib", n_vis.tolist())
    for b in range(B):
        assert 0 < n_vis[b, 0] < n_all[b, 0]                        # sphere 5: 0 < visib_fract < 1
        assert n_all[b, 2] >= 50 and n_vis[b, 2] == 0               # sphere 8: visib_fract == 0
        assert info[b, 2, 6:].tolist() == [-1] * 4
        for k in (0, 1, 3):                                         # every object that is not hidden: >= 50 visible pixels
            assert n_vis[b, k] >= 50, (b, k)
        assert info[b, 1, 4] == W - 1 or info[b, 1, 3] == 0         # the torus reaches a border
    assert info[0, 3, 4] == W - 1 and info[1, 3, 3] == 0            # sphere 3: the right border, then the top border
    # buffers are kept per batch size; without masks the same info
    assert sb.annotate(r).info.data_ptr() == ann.info.data_ptr()
    lean = sb.annotate(r, masks=False)
    assert lean.mask is None and torch.equal(lean.info.cpu(), info)


def test_capture_and_replay(ops):
    K, B, H, W = 3, 2, 48, 64
    rs = np.random.RandomState(11)
    zb = cu(synthetic_planes(K, B, H, W, rs))
    ids = cu(np.array([3, 1, 2], dtype=np.int32))
    label = device_label(ops, zb, ids).clone()
    eager = ops.scene_annotate(zb, label, ids)
    static = {k: torch.zeros_like(v) for k, v in eager.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.scene_annotate(zb, label, ids, out=static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.scene_annotate(zb, label, ids, out=static)
    for v in static.values():
        v.fill_(77)
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert torch.equal(static[k], eager[k]), k
    # two replays on changed inputs behind the same pointers, each bit-identical to eager
    for seed in (12, 13):
        zb2 = cu(synthetic_planes(K, B, H, W, np.random.RandomState(seed)))
        label2 = device_label(ops, zb2, ids)
        want = ops.scene_annotate(zb2, label2, ids)
        assert not torch.equal(want["info"], eager["info"])
        zb.copy_(zb2)
        label.copy_(label2)
        graph.replay()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(static[k], want[k]), (seed, k)


def test_limits_and_argument_checks(ops):
    from texpose_amd import _lib
    zb = torch.full((33, 1, 8, 8), -1.0, device=DEV)
    with pytest.raises(_lib.TexposeLibraryError, match="32"):
        ops.scene_annotate(zb, torch.zeros(1, 64, dtype=torch.int32, device=DEV), torch.ones(33, dtype=torch.int32, device=DEV))
    zb, label, ids = zb[:2].contiguous(), torch.zeros(1, 64, dtype=torch.int32, device=DEV), torch.tensor([1, 2], dtype=torch.int32, device=DEV)
    for bad in (lambda: ops.scene_annotate(zb.double(), label, ids), lambda: ops.scene_annotate(zb, label.long(), ids),
                lambda: ops.scene_annotate(zb, label[:, :60], ids), lambda: ops.scene_annotate(zb, label, ids[:1]),
                lambda: ops.scene_annotate(zb, label, ids, out=dict(info=torch.zeros(1, 2, 10, device=DEV))),
                lambda: ops.view_images(torch.zeros(1, 64, 3, device=DEV), torch.zeros(1, 60, device=DEV), H=8, W=8),
                lambda: ops.view_images(torch.zeros(1, 64, 4, device=DEV), None, H=8, W=8)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("BHW", [(1, 37, 53), (3, 32, 48)])
def test_view_images_against_helper(ops, BHW):
    B, H, W = BHW
    rs = np.random.RandomState(B + H)
    rgb = rs.uniform(-0.2, 1.2, size=(B, H * W, 3)).astype(F)
    depth = rs.uniform(-1.0, 20.0, size=(B, H * W)).astype(F)
    edges = np.array([0.0, 1.0, 1.5, -0.5, np.nan, np.inf, -np.inf, 1 / 255, 0.999999, 254.5 / 255], dtype=F)
    rgb.reshape(-1)[rs.choice(rgb.size, 200, replace=False)] = np.tile(edges, 20)
    scale = 10.0                                                    # 65535 is reached at 327.675 units
    dedges = np.array([0.0, -3.0, np.nan, np.inf, 327.67, 327.675, 327.68, 1e9, 0.005, 0.00499], dtype=F)
    depth.reshape(-1)[rs.choice(depth.size, 200, replace=False)] = np.tile(dedges, 20)
    got = ops.view_images(cu(rgb), cu(depth), H=H, W=W, depth_scale=scale, png_per_metre=2000)
    assert got["rgb8"].dtype == torch.uint8 and got["rgb8"].shape == (B, H, W, 3)
    assert got["depth16"].dtype == torch.uint16 and got["depth16"].shape == (B, H, W)
    want8, want16 = SA.rgb8(rgb, H, W), SA.depth16(depth, H, W, scale)
    assert np.array_equal(got["rgb8"].cpu().numpy(), want8) and np.array_equal(got["depth16"].cpu().numpy(), want16)
    assert want16.max() == 65535 and want8.max() == 255 and want8.min() == 0
    # the tool's present torch chain gives the same bytes wherever it is defined (finite values)
    fin = np.nan_to_num(rgb, nan=0.0, posinf=2.0, neginf=-1.0)
    assert torch.equal((cu(fin).clamp(0, 1) * 255).byte().view(B, H, W, 3), ops.view_images(cu(fin), None, H=H, W=W)["rgb8"])
    dfin = np.nan_to_num(depth, nan=0.0, posinf=1e9)
    chain = ((cu(dfin) / scale) * 2000).clamp(0, 65535).cpu().numpy().astype(np.uint16).reshape(B, H, W)
    only = ops.view_images(None, cu(dfin)[..., None], H=H, W=W, depth_scale=scale)
    assert sorted(only) == ["depth16"]
    # (torch divides by a host scalar as a product with its reciprocal: one unit of difference is possible there, no more)
    diff = np.abs(chain.astype(np.int64) - only["depth16"].cpu().numpy().astype(np.int64))
    assert diff.max() <= 1 and np.array_equal(only["depth16"].cpu().numpy(), SA.depth16(dfin, H, W, scale))


def test_end_to_end_scene(ops, tmp_path):
    from texpose_amd.bop_scene import BopSceneWriter, read_bop_frame, verify_bop_scene
    from texpose_amd.scene_bounds import SceneBounds
    H = W = 64
    objects, _, pose, K, _, _ = mesh_scene(H, W)
    opt, graph = small_graph(H, W, 16)
    sb = SceneBounds(objects, H, W, SCALE, BG)
    pose_dev, intr = cu(pose), cu(K)
    r = sb(pose_dev, intr, "box")
    ann = sb.annotate(r)
    names = {5: "sphere", 2: "torus", 8: "pea", 3: "moon"}
    writer = BopSceneWriter(str(tmp_path), intr, SCALE, png_per_metre=2000, names=names)
    kept = []
    with torch.no_grad():
        for i in range(pose.shape[0]):
            dr = (r.depth_range[0][i:i + 1], r.depth_range[1][i:i + 1])
            ret = graph.render_by_slices(opt, pose_dev[i:i + 1], intr=intr[None], depth_range=dr, object_mask=r.object_mask[i:i + 1],
                                         sample_idx=torch.tensor(1, device=DEV), mode="eval")
            img = ops.view_images(ret.rgb, ret.depth, H=H, W=W, depth_scale=SCALE, png_per_metre=2000)
            assert torch.equal(img["rgb8"], (ret.rgb.clamp(0, 1) * 255).byte().view(1, H, W, 3)) and img["rgb8"].any()
            assert writer.add_views(pose_dev[i:i + 1], sb.object_ids, ann.info[i:i + 1], ann.mask[i:i + 1], ann.mask_visib[i:i + 1],
                                    img["rgb8"], img["depth16"]) == [i]
            kept.append({k: v.cpu().numpy() for k, v in img.items()})
    writer.close()
    assert verify_bop_scene(str(tmp_path)) == 2
    t_mm = ((pose_dev[:, :, 3] / SCALE) * 1000).cpu().numpy()       # the rasteriser's expression, on the device
    info = ann.info.cpu().numpy()
    for i in range(pose.shape[0]):
        fr = read_bop_frame(str(tmp_path), i)
        assert np.array_equal(fr["rgb"], kept[i]["rgb8"][0]) and np.array_equal(fr["depth"], kept[i]["depth16"][0])
        assert np.array_equal(fr["mask"], ann.mask[i].cpu().numpy()) and np.array_equal(fr["mask_visib"], ann.mask_visib[i].cpu().numpy())
        assert fr["obj_id"].tolist() == sb.object_ids and fr["objects"] == {names[k]: j for j, k in enumerate(sb.object_ids)}
        assert np.array_equal(fr["cam_K"], K.numpy()) and fr["depth_scale"] == 0.5
        for k in range(len(sb.object_ids)):
            assert np.array_equal(fr["cam_R_m2c"][k], pose[i, :, :3].numpy()) and np.array_equal(fr["cam_t_m2c"][k], t_mm[i])
            e, row = fr["info"][k], info[i, k].tolist()
            assert (e["px_count_all"], e["px_count_valid"], e["px_count_visib"]) == (row[0], row[0], row[1])
            assert e["visib_fract"] == (row[1] / row[0] if row[0] else 0.0)
            assert e["bbox_obj"] == ([-1] * 4 if row[4] < 0 else [row[2], row[3], row[4] - row[2], row[5] - row[3]])
            assert e["bbox_visib"] == ([-1] * 4 if row[8] < 0 else [row[6], row[7], row[8] - row[6], row[9] - row[7]])
        assert fr["info"][2]["visib_fract"] == 0.0 and 0 < fr["info"][0]["visib_fract"] < 1


def test_novel_views_tool_writes_a_bop_scene(tmp_path):
    from texpose_amd import checkpoint as ck
    from texpose_amd.bop_scene import read_bop_frame, verify_bop_scene
    H = W = 48
    N, n_views = 16, 2
    opt, graph = small_graph(H, W, N)
    ck.save_checkpoint(str(tmp_path / "model.ckpt"), graph, epoch=1, it=10)
    vs, fs = uv_sphere(12, 24)
    vt, ft = torus(24, 12)
    vt = (vt + np.array([30.0, 0.0, -150.0], dtype=F)).astype(F)
    write_ascii_ply(str(tmp_path / "sphere.ply"), vs, fs)
    write_ascii_ply(str(tmp_path / "torus.ply"), vt, ft)
    np.savez(str(tmp_path / "scene.npz"), pose_anchor=pose_of([0.1, -0.15, 0.3], [0.1, -0.05, 8.0]), intr=K_for(H, W))
    bop = tmp_path / "bop"
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "tools", "novel_views.py"), "--checkpoint", str(tmp_path / "model.ckpt"),
           "--scene", str(tmp_path / "scene.npz"), "--ply", "5=" + str(tmp_path / "sphere.ply"), "--ply", "2=" + str(tmp_path / "torus.ply"),
           "--bop", str(bop), "--name", "5=sphere", "--name", "2=torus", "--verify", "--N", str(n_views), "--H", str(H), "--W", str(W),
           "--samples", str(N), "--precision", "fp32", "--source", "render"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "2 frames" in p.stdout and "consistent" in p.stdout
    assert verify_bop_scene(str(bop)) == n_views
    for i in range(n_views):
        fr = read_bop_frame(str(bop), i)
        assert fr["rgb"].shape == (H, W, 3) and fr["rgb"].any() and fr["depth"].dtype == np.uint16 and 0 < fr["depth"].max() < 2 * 2000
        assert fr["obj_id"].tolist() == [5, 2] and fr["objects"] == {"sphere": 0, "torus": 1}
        assert fr["info"][1]["visib_fract"] == 1.0 and 0 < fr["info"][0]["visib_fract"] < 1      # the torus is in front
    assert sorted(os.listdir(str(bop))) == ["depth", "mask", "mask_visib", "rgb", "scene_camera.json", "scene_gt.json", "scene_gt_info.json",
                                            "scene_object.json"]
