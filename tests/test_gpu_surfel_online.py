"""GPU: the surfel maps delivered on the device as the reference's data layer would load them (tp_surfel_finish,
SurfelRenderer.data_layer_maps, SurfelMapStore) against the file route: write_surfel_frame -> the data layer's decode restated in
tests/surfel_reader_ref.py (pinned to the reference's get_edge / smooth_geo by golden G22).  Everything is compared with
torch.equal: the in-process route has to be bit for bit what the files give."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import surfel_reader_ref as RD
from test_gpu_surfel import K_for, REPO, _write_binary_ply, pose_of, torus, uv_sphere

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEYS = ("image_syn", "mask_syn", "nocs_pred", "normal_pred")
DEPTH_SCALE = 10.0                                                   # pose translations below are in dm: 6.5 = 650 mm


def _mesh(kind, colours=True, seed=0):
    rs = np.random.RandomState(seed)
    v, f = uv_sphere(24, 48, ripple=0.1) if kind == "sphere" else torus(48, 24)
    return v, f, (rs.uniform(size=v.shape).astype(np.float32) if colours else None)


def _poses(n, seed, shift_last=True):
    """n poses around 650 mm; the last one, nearly face-on, sits 60 mm to the right so that the object runs across the image border."""
    rs = np.random.RandomState(seed)
    out = [pose_of(rs.uniform(-2, 2, 3), [rs.uniform(-0.1, 0.1), rs.uniform(-0.1, 0.1), rs.uniform(6.0, 7.0)]) for _ in range(n)]
    if shift_last:
        out[-1] = pose_of([0.4, -0.3, 0.2], [0.6, 0.0, 6.5])
    return torch.from_numpy(np.stack(out))


def _file_route(renderer, pose, K, root, loop=1, frames=None):
    """The reference's detour: raw render -> write_surfel_frame -> the data layer's decode.  -> list of decode_frame dicts."""
    from texpose_amd.surfel import surfel_file_name, write_surfel_frame
    raw = renderer(pose, K, DEPTH_SCALE)
    frames = list(range(pose.shape[0])) if frames is None else frames
    out = []
    for b, fr in enumerate(frames):
        write_surfel_frame(str(root), loop, fr, raw, b)
        out.append(RD.decode_frame(str(root), loop, surfel_file_name(fr)))
    return raw, out


def _stack(decoded, key):
    return torch.from_numpy(np.stack([d[key] for d in decoded])).to(DEV)


@pytest.mark.parametrize("H,W", [(128, 128), (120, 160)])
@pytest.mark.parametrize("kind", ["sphere", "torus"])
def test_file_round_trip_is_bit_identical(tmp_path, kind, H, W):
    """The acceptance test: all four tensors of data_layer_maps equal what the data layer decodes from the files, for three poses of
    which one crosses the image border; every frame has >= 50 edge pixels in both smoothed maps and edge pixels the median changed."""
    from texpose_amd.surfel import SurfelRenderer
    v, f, col = _mesh(kind)
    r = SurfelRenderer(v, f, col, H, W, DEV)
    pose, K = _poses(3, seed=H + len(kind)), torch.from_numpy(K_for(H, W))
    _, dec = _file_route(r, pose, K, tmp_path)
    maps = r.data_layer_maps(pose, K, DEPTH_SCALE)
    torch.cuda.synchronize()
    assert set(KEYS) <= set(maps.keys()) and "depth" in maps
    for key in KEYS:
        want = _stack(dec, key)
        assert maps[key].shape == want.shape and maps[key].dtype == torch.float32 and maps[key].is_contiguous(), key
        assert torch.equal(maps[key], want), (key, int((maps[key] != want).sum()))
    for b, d in enumerate(dec):                                     # the comparison is not vacuous
        assert d["mask_syn"].sum() > 1000, b
        for name in ("nocs", "normal"):
            edge, raw_map, smooth = d[name + "_edge"], d[name + "_raw"], d[name + "_pred"].transpose(1, 2, 0)
            changed = (smooth != raw_map).any(-1)
            print("%s %dx%d frame %d %s: %d edge pixels, %d changed by the median" % (kind, H, W, b, name, edge.sum(), changed.sum()))
            assert edge.sum() >= 50, (b, name, int(edge.sum()))
            assert (changed & edge).sum() >= 1 and not (changed & ~edge).any(), (b, name)
    covered = dec[-1]["mask_syn"] > 0
    assert covered[:, -1].any() and not covered[:, 0].any()         # the last pose runs over the right image border
    assert (dec[0]["image_syn"] > 0).any()


def test_quantize_false_keeps_fp32_colour_and_nocs():
    from texpose_amd.surfel import SurfelRenderer
    v, f, col = _mesh("sphere")
    r = SurfelRenderer(v, f, col, 120, 160, DEV)
    pose, K = _poses(2, seed=3), torch.from_numpy(K_for(120, 160))
    raw = r(pose, K, DEPTH_SCALE)
    m = r.data_layer_maps(pose, K, DEPTH_SCALE, quantize=False)
    q = r.data_layer_maps(pose, K, DEPTH_SCALE)
    assert torch.equal(m.image_syn, raw.rgb_syn.contiguous()) and not torch.equal(m.image_syn, q.image_syn)
    assert torch.equal(m.mask_syn, raw.mask_syn) and torch.equal(m.depth, raw.depth)
    nocs = raw.nocs.permute(0, 2, 3, 1).cpu().numpy()
    want = np.stack([RD.smooth_geo(nocs[b]).transpose(2, 0, 1) for b in range(2)])
    assert torch.equal(m.nocs_pred, torch.from_numpy(want).to(DEV))
    assert sum(int(RD.get_edge(nocs[b]).sum()) for b in range(2)) >= 100
    assert torch.equal(m.normal_pred, q.normal_pred)               # normals are never quantised


def test_mesh_without_colours_gives_zero_image():
    from texpose_amd.surfel import SurfelRenderer
    v, f, col = _mesh("torus")
    pose, K = _poses(2, seed=4), torch.from_numpy(K_for(128, 128))
    with_c = SurfelRenderer(v, f, col, 128, 128, DEV).data_layer_maps(pose, K, DEPTH_SCALE)
    without = SurfelRenderer(v, f, None, 128, 128, DEV).data_layer_maps(pose, K, DEPTH_SCALE)
    assert without.image_syn.shape == (2, 3, 128, 128) and not without.image_syn.any() and with_c.image_syn.any()
    for key in ("mask_syn", "nocs_pred", "normal_pred", "depth"):
        assert torch.equal(with_c[key], without[key]), key


def test_surfel_map_store_batches_and_refreshes_in_place():
    from texpose_amd.surfel import SurfelMapStore, SurfelRenderer
    v, f, col = _mesh("sphere", seed=5)
    H, W, N = 64, 80, 10
    r = SurfelRenderer(v, f, col, H, W, DEV)
    rs = np.random.RandomState(6)
    K = torch.from_numpy(np.stack([K_for(H, W, f=rs.uniform(250, 330), dc=rs.uniform(-4, 4, 2)) for _ in range(N)]))
    pose = _poses(N, seed=7)
    store = SurfelMapStore(r, pose, K, DEPTH_SCALE, batch=4)        # 4 + 4 + 2: a ragged last batch
    idx = torch.from_numpy(rs.permutation(N)[:6].astype(np.int64)).to(DEV)
    got = store.batch(idx)
    want = r.data_layer_maps(pose[idx.cpu()], K[idx.cpu()], DEPTH_SCALE)
    assert set(got.keys()) == set(KEYS)
    for key in KEYS:
        assert torch.equal(got[key], want[key]), key
        assert got[key].data_ptr() != store.maps[key].data_ptr()    # a gathered copy, not a view of the store
    assert got.mask_syn.sum() > 500
    ptrs = {k: store.maps[k].data_ptr() for k in KEYS}
    pose2 = _poses(N, seed=8)
    store.refresh(pose2)
    fresh = SurfelMapStore(r, pose2, K, DEPTH_SCALE, batch=16)
    for key in KEYS:
        assert store.maps[key].data_ptr() == ptrs[key], key
        assert torch.equal(store.maps[key], fresh.maps[key]), key
        assert not torch.equal(store.maps[key], r.data_layer_maps(pose, K, DEPTH_SCALE)[key]), key
    shared = SurfelMapStore(r, pose2, K[0], DEPTH_SCALE, batch=3)   # one [3,3] intrinsics matrix for all frames
    assert torch.equal(shared.batch(torch.tensor([0]))["nocs_pred"], fresh.batch(torch.tensor([0]))["nocs_pred"])
    with pytest.raises(ValueError):
        store.refresh(pose2[:4])


def test_raster_and_finish_replay_from_a_graph():
    from texpose_amd.surfel import SurfelRenderer
    v, f, col = _mesh("torus", seed=9)
    r = SurfelRenderer(v, f, col, 120, 160, DEV)
    K = torch.from_numpy(K_for(120, 160)).to(DEV)
    sets = [_poses(3, seed=s).to(DEV) for s in (10, 11, 12)]
    pose = sets[0].clone()
    run = lambda p: r.data_layer_maps(p, K, DEPTH_SCALE)
    eager = [run(p) for p in sets]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(pose)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(pose)
    for n in (1, 2):                                                # two replays, each after the poses were overwritten in place
        pose.copy_(sets[n])
        for t in out.values():
            t.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for key in KEYS + ("depth",):
            assert torch.equal(out[key], eager[n][key]), (n, key)
    assert not torch.equal(eager[1].nocs_pred, eager[2].nocs_pred)


def test_surfel_maps_tool_verifies_its_files_online(tmp_path):
    rs = np.random.RandomState(15)
    v, f = uv_sphere(18, 36, ripple=0.1)
    ply = str(tmp_path / "obj_000001.ply")
    _write_binary_ply(ply, v, f, rs.randint(0, 256, size=v.shape).astype(np.uint8))
    np.savez(str(tmp_path / "poses.npz"), frame_index=np.array([2, 40, 41]), pose=_poses(3, seed=16).numpy(), intr=K_for(120, 160))
    cmd = [sys.executable, os.path.join(REPO, "tools", "surfel_maps.py"), "--ply", ply, "--poses", str(tmp_path / "poses.npz"),
           "--depth-scale", str(DEPTH_SCALE), "--H", "120", "--W", "160", "--loop", "1", "--out", str(tmp_path / "seq"), "--batch", "2",
           "--verify-online"]
    res = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-2000:])
    assert "verify-online: 3 frames x 4 tensors, all equal" in res.stdout
    # a file that no longer matches the poses is reported: exit status 1
    seq = str(tmp_path / "seq")
    os.replace(os.path.join(seq, "nocs_1", "000040.png"), os.path.join(seq, "nocs_1", "tmp.png"))
    os.replace(os.path.join(seq, "nocs_1", "000041.png"), os.path.join(seq, "nocs_1", "000040.png"))
    from texpose_amd.surfel import MAP_KEYS, SurfelRenderer, load_ply, read_surfel_frame
    verts, faces, vcolor = load_ply(ply)
    maps = SurfelRenderer(verts, faces, vcolor, 120, 160, DEV).data_layer_maps(_poses(3, seed=16)[1:2], torch.from_numpy(K_for(120, 160)), DEPTH_SCALE)
    dec = read_surfel_frame(seq, "1", 40)
    assert [k for k in MAP_KEYS if not torch.equal(maps[k][0].cpu(), dec[k])] == ["nocs_pred"]


@pytest.mark.parametrize("form,H,B,N,n_train", [("eager", 32, 2, 16, 7), ("graphed", 128, 4, 64, 12)])
def test_trainer_step_on_store_maps_equals_the_file_route(tmp_path, form, H, B, N, n_train):
    """One GAN iteration on synthetic data whose image_syn / mask_syn / nocs_pred / normal_pred come from a SurfelMapStore: finite
    losses, and bit for bit the losses of the same step fed with the tensors decoded from the files."""
    from texpose_amd.gan_modules import Discriminator, PerceptualLoss
    from texpose_amd.graph import Graph
    from texpose_amd.options import AttrDict, default_options
    from texpose_amd.surfel import SurfelMapStore, SurfelRenderer
    from texpose_amd.synthetic import training_batch
    from texpose_amd.trainer import GanTrainer, GraphedGanTrainer
    v, f, col = _mesh("sphere", seed=13)
    r = SurfelRenderer(v, f, col, H, H, DEV)
    pose, K = _poses(n_train, seed=14, shift_last=False), torch.from_numpy(K_for(H, H))
    batch = training_batch(B, H, H, n_train=n_train, seed=1, device=DEV)
    store = SurfelMapStore(r, pose, K, DEPTH_SCALE, batch=5)
    online = store.batch(batch.idx)
    frames = batch.idx.cpu().tolist()
    _, dec = _file_route(r, pose[batch.idx.cpu()], K, tmp_path, frames=frames)
    files = {key: _stack(dec, key) for key in KEYS}
    for key in KEYS:
        assert torch.equal(online[key], files[key]), key
    assert online.mask_syn.sum() > 100
    # the step's own draws (patch scale / shifts, stratified jitter) are pinned: eager steps number their Philox calls per process
    gen = torch.Generator().manual_seed(12)
    patch_u, jitter = torch.rand(3, B, 1, 1, 1, generator=gen).to(DEV), torch.rand(B, 256, N, 1, generator=gen).to(DEV)

    def step(maps):
        torch.manual_seed(0)
        opt = default_options(H=H, W=H, device=DEV)
        opt.batch_size, opt.patch_size, opt.nerf.sample_intvs = B, 16, N
        graph = Graph(opt, discriminator=Discriminator(opt), perceptual_loss=PerceptualLoss()).to(torch.device(DEV))
        tr = (GanTrainer if form == "eager" else GraphedGanTrainer)(opt, graph, n_train=n_train)
        var = AttrDict(dict(batch))
        var.update({key: maps[key].clone() for key in KEYS})
        var.patch_u, var.jitter_rand = patch_u, jitter
        _, loss = tr.train_iteration(var)
        if form == "graphed":
            tr.finish()
        torch.cuda.synchronize()
        return {k: x.detach().clone() for k, x in loss.items() if torch.is_tensor(x)}

    a, b = step(online), step(files)
    assert len(a) >= 3 and set(a) == set(b)
    for k in a:
        assert torch.isfinite(a[k]).all(), (k, a[k])
        assert torch.equal(a[k], b[k]), (k, a[k], b[k])
