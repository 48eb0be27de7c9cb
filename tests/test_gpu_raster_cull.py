"""K34 on the GPU: tp_mesh_raster_culled against tp_mesh_raster on the same inputs, bit for bit on every requested plane, at the edges
of the new code (chunk counts, two cooperative rounds, dead chunks, tile borders, image sizes, batches, plane subsets, face orders),
coherent_face_order, determinism and graph replay, and the layers above with cull=True against cull=False.  tp_mesh_raster itself is
held to the fp64 brute force by tests/test_gpu_surfel.py."""
import types

import numpy as np
import pytest
import torch

import icp_ref as IREF
import mesh_raster_ref as REF
import pnp_ref as PREF
import raster_cull_ref as CULL
from gn_ref import cu, host
from test_gpu_surfel import K_for, pose_of, soup, torus, uv_sphere

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PLANES = ("zbuf", "face", "rgb", "nocs", "normal")
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
K100 = np.array([[100.0, 0, 0.0], [0, 100.0, 0.0], [0, 0, 1]], dtype=np.float32)       # identity pose: pixel position = 100 (x, y) / z


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        if not torch.equal(bits(a[k]), bits(b[k])):
            where = torch.nonzero(bits(a[k]) != bits(b[k]))
            raise AssertionError("plane %s differs at %d places, first %s" % (k, len(where), where[0].tolist()))


def colours(verts):
    return np.random.RandomState(len(verts)).uniform(size=np.shape(verts)).astype(np.float32)


def raster(verts, faces, pose, K, H, W, cull, full=True, **kw):
    """ops.mesh_raster on numpy inputs; ``full``: all five planes (random vertex colours, the mesh's NOCS normalisation)."""
    from texpose_amd import ops
    if full:
        kw = dict(dict(vcolor=cu(colours(verts)), nocs_norm=tuple(np.asarray(x, np.float32) for x in REF.nocs_normalisation(verts)),
                       face_ids=True, normals=True), **kw)
    pose = np.asarray(pose, np.float32)
    return ops.mesh_raster(cu(np.asarray(verts, np.float32)), cu(np.asarray(faces, np.int32)), cu(pose if pose.ndim == 3 else pose[None]),
                           cu(np.asarray(K, np.float32)), H=H, W=W, cull=cull, **kw)


def both(verts, faces, pose, K, H, W, **kw):
    """The plain and the culled call on the same inputs: equal bits on every plane -> the plain call's planes."""
    plain, culled = raster(verts, faces, pose, K, H, W, False, **kw), raster(verts, faces, pose, K, H, W, True, **kw)
    same(plain, culled)
    return plain


def covered(r):
    return int((r["zbuf"] > 0).sum())


# ----------------------------------------------------------------------------- chunk counts and rounds
@pytest.mark.parametrize("H,W", [(37, 53), (120, 160)])
@pytest.mark.parametrize("F", [1, 255, 256, 257, 513])
def test_chunk_counts(F, H, W):
    v, f = uv_sphere(12, 24, ripple=0.2)
    assert len(f) >= 513
    r = both(v, f[:F], pose_of([0.7, 0.1, -0.4], [2, 1, 650]), K_for(H, W), H, W)
    assert set(r) == set(PLANES) and (F == 1 or covered(r) > 20)


def tiled_soup(n, H, W, rs):
    """n small triangles (about 3 pixels wide, each at its own depth; H and W multiples of 16) ordered by the 16 x 16 tile of their
    centre, which keeps 2 pixels from the tile's border: a chunk of 256 consecutive ones reaches into one tile, or into two where the
    order passes from a tile to the next; K100 and the identity pose."""
    z = (400.0 + rs.permutation(n) * 0.01).astype(np.float64)
    tile = np.sort(rs.randint(0, (H // 16) * (W // 16), n))
    c = np.stack([(tile % (W // 16)) * 16, (tile // (W // 16)) * 16], 1) + rs.uniform(2.0, 14.0, (n, 2))
    uv = c[:, None] + rs.uniform(-1.6, 1.6, size=(n, 3, 2))
    v = np.concatenate([uv / 100.0 * z[:, None, None], np.broadcast_to(z[:, None, None], (n, 3, 1))], -1).reshape(-1, 3)
    return v.astype(np.float32), np.arange(3 * n).reshape(n, 3).astype(np.int32)


def test_two_rounds_of_chunk_boxes_spread_over_the_image():
    """65,537 faces = 257 chunks: the second round of 256 boxes holds one, of one face.  Every tile keeps a few chunks (about 11 of the
    257), and the last tile the last."""
    H, W, n = 64, 96, 65537
    v, f = tiled_soup(n, H, W, np.random.RandomState(11))
    count = CULL.counts(v, f, EYE, K100, H, W)
    assert count["plain"] == 24 * 257 and (count["per_tile"] >= 9).all() and count["per_tile"].max() <= 14, count["per_tile"]
    last = CULL.overlaps(CULL.chunk_boxes(CULL.face_boxes(v, f, EYE, K100, H, W))[256:], CULL.tiles_of(H, W))[:, 0]
    assert last.tolist() == [False] * 23 + [True]               # the lone box of round two survives in the last tile only
    r = both(v, f, EYE, K100, H, W)
    assert covered(r) > 0.5 * H * W
    assert int(r["face"].max()) >= 65536 - 256                   # faces of the last chunks are seen


def test_two_rounds_with_every_chunk_in_one_tile():
    """The construction of test_more_than_100k_faces_in_one_tile: 120,000 faces = 469 chunks, all of which survive in the tile of
    columns 32-47, rows 16-31 and, but for the ring of tiles their 1.6 pixel reach touches, nowhere else."""
    rs = np.random.RandomState(6)
    n, H, W = 120000, 64, 96
    z = (400.0 + rs.permutation(n) * 0.01).astype(np.float64)
    c = np.stack([rs.uniform(32.5, 47.5, n), rs.uniform(16.5, 31.5, n)], 1)
    uv = c[:, None] + rs.uniform(-1.6, 1.6, size=(n, 3, 2))
    v = np.concatenate([uv / 100.0 * z[:, None, None], np.broadcast_to(z[:, None, None], (n, 3, 1))], -1).reshape(-1, 3)
    v, f = v.astype(np.float32), np.arange(3 * n).reshape(n, 3).astype(np.int32)
    count = CULL.counts(v, f, EYE, K100, H, W).pop("per_tile").reshape(4, 6)
    assert count[1, 2] == 469 and (count[3] == 0).all() and (count[:, [0, 4, 5]] == 0).all()
    r = both(v, f, EYE, K100, H, W)
    inside = torch.zeros(H, W, dtype=torch.bool, device=DEV)
    inside[14:34, 30:50] = True
    assert covered(r) > 250 and (r["face"][0][~inside] == -1).all()


def test_dead_chunks():
    """Five chunks: live, wholly behind the camera, every index out of range, wholly off-screen, live."""
    H, W = 48, 64
    rs = np.random.RandomState(12)
    v, f = tiled_soup(5 * 256, H, W, rs)
    v = v.copy()
    v[3 * 256:3 * 512, 2] *= -1.0                                 # chunk 1: z < 0
    f = f.copy()
    f[512:768] = rs.choice(np.array([-1, len(v), len(v) + 7, np.iinfo(np.int32).max, np.iinfo(np.int32).min]), size=(256, 3))      # chunk 2
    v[3 * 768:3 * 1024, 0] += 500.0                              # chunk 3: to the right of the image
    cb = CULL.chunk_boxes(CULL.face_boxes(v, f, EYE, K100, H, W))
    assert [tuple(b) == CULL.EMPTY for b in cb] == [False, True, True, True, False]
    r = both(v, f, EYE, K100, H, W)
    seen = torch.unique(r["face"]).tolist()
    assert covered(r) > 100 and all(i == -1 or i < 256 or i >= 1024 for i in seen) and max(seen) >= 1024
    # with the live chunks dead as well: all background
    f[:256] = -1
    f[1024:] = len(v)
    r = both(v, f, EYE, K100, H, W)
    assert covered(r) == 0 and (r["face"] == -1).all()


def test_mesh_entirely_outside_the_image():
    v, f = uv_sphere(16, 32)
    r = both(v, f, pose_of([0.2, 0.4, 0.0], [900, 0, 600]), K_for(96, 128), 96, 128)
    assert set(r) == set(PLANES)
    assert (r["face"] == -1).all() and (r["zbuf"] == -1).all() and (r["rgb"] == 0).all() and (r["nocs"] == 0).all() and (r["normal"] == 0).all()


def test_nan_pose_in_a_batch():
    v, f = uv_sphere(16, 32, ripple=0.1)
    good = pose_of([0.3, -0.5, 0.2], [4, -3, 620])
    for entry in ((0, 0), (2, 3), (1, 1)):
        bad = good.copy()
        bad[entry] = np.nan
        pose = np.stack([good, bad, pose_of([-0.8, 0.2, 0.1], [-5, 6, 700])])
        r = both(v, f, pose, K_for(64, 80), 64, 80)
        assert (r["zbuf"][1] == -1).all() and (r["face"][1] == -1).all() and (r["rgb"][1] == 0).all() and (r["nocs"][1] == 0).all()
        assert (r["normal"][1] == 0).all() and covered({"zbuf": r["zbuf"][0]}) > 500 and covered({"zbuf": r["zbuf"][2]}) > 300
        alone = raster(v, f, pose[[0, 2]], K_for(64, 80), 64, 80, True)
        same({k: t[[0, 2]] for k, t in r.items()}, alone)


def test_tile_borders():
    """One-pixel triangles at columns 15 / 16 x rows 15 / 16 of a 33 x 33 image (and at the last column and row, a tile of one pixel's
    width), each alone in a chunk of dead faces: the inclusive comparisons on both sides of a tile edge."""
    H = W = 33
    spots = [(15, 15), (16, 15), (15, 16), (16, 16), (32, 16), (15, 32), (32, 32), (0, 0)]          # (column, row)
    places = [0, 255, 100, 7, 64, 63, 128, 254]                  # the live face's place in its chunk
    n = len(spots) * 256
    f = np.full((n, 3), -1, np.int32)
    v = np.zeros((3 * len(spots), 3), np.float32)
    ids = []
    for k, ((j, i), at) in enumerate(zip(spots, places)):
        z = 400.0 + k
        tri = np.array([[j + 0.05, i + 0.1], [j + 0.95, i + 0.1], [j + 0.5, i + 0.95]])
        v[3 * k:3 * k + 3] = np.concatenate([tri / 100.0 * z, np.full((3, 1), z)], 1)
        f[256 * k + at] = [3 * k, 3 * k + 1, 3 * k + 2]
        ids.append(256 * k + at)
    box = CULL.face_boxes(v, f, EYE, K100, H, W)
    assert [box[i].tolist() for i in ids] == [[j, j, i, i] for j, i in spots]
    assert CULL.chunk_boxes(box).tolist() == [[j, j, i, i] for j, i in spots]
    r = both(v, f, EYE, K100, H, W)
    want = np.full((H, W), -1, np.int32)
    for (j, i), face in zip(spots, ids):
        want[i, j] = face
    assert np.array_equal(host(r["face"][0]), want)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 3), (16, 16), (17, 17), (480, 640)])
def test_image_sizes_with_the_20k_sphere(H, W):
    v, f = uv_sphere(71, 144, ripple=0.08)
    assert len(f) == 20160
    if H == 480:
        r = both(v, f, pose_of([0.4, -0.9, 0.3], [10, -5, 750]), CULL.LINEMOD_K, H, W)
        assert covered(r) > 3500
    else:
        r = both(v, f, pose_of([0.4, -0.9, 0.3], [1, -1, 300]), K_for(H, W, f=150.0), H, W)
        assert covered(r) >= min(H * W, 150)


def test_batch_of_five_with_their_own_intrinsics():
    rs = np.random.RandomState(2)                                # the case of test_batch_of_poses_with_different_intrinsics
    v, f = uv_sphere(16, 32, ripple=0.15)
    pose = np.stack([pose_of(rs.uniform(-2, 2, 3), [rs.uniform(-10, 10), rs.uniform(-10, 10), rs.uniform(500, 800)]) for _ in range(5)])
    K = np.stack([K_for(64, 80, f=rs.uniform(250, 400), dc=rs.uniform(-5, 5, 2)) for _ in range(5)])
    r = both(v, f, pose, K, 64, 80)
    assert all(int((r["zbuf"][b] > 0).sum()) > 300 for b in range(5))
    for b in (0, 4):                                             # an image of the batch is the image alone
        same({k: t[b:b + 1] for k, t in r.items()}, raster(v, f, pose[b], K[b], 64, 80, True))


def test_plane_subsets():
    v, f = torus(48, 24)
    pose, K, H, W = np.stack([pose_of([1.2, 0.2, 0.0], [0, 5, 560]), pose_of([0.1, 0.9, -0.3], [6, -2, 600])]), K_for(120, 160), 120, 160
    everything = both(v, f, pose, K, H, W)
    col = cu(colours(v))
    for kw, keys in ((dict(face_ids=False, normals=False), {"zbuf"}), (dict(face_ids=True, normals=False), {"zbuf", "face"}),
                     (dict(face_ids=False, normals=False, vcolor=col), {"zbuf", "rgb"}), (dict(face_ids=False, normals=True), {"zbuf", "normal"})):
        r = both(v, f, pose, K, H, W, full=False, **kw)
        assert set(r) == keys
        same(r, {k: everything[k] for k in keys})
    stack = torch.full((3, 2, H, W), 7.0, device=DEV)
    r = raster(v, f, pose, K, H, W, True, full=False, face_ids=False, normals=False, zbuf_out=stack[1])
    assert r["zbuf"].data_ptr() == stack[1].data_ptr() and torch.equal(bits(stack[1]), bits(everything["zbuf"]))
    assert (stack[0] == 7).all() and (stack[2] == 7).all()


def test_shuffled_face_order():
    v, f = uv_sphere(71, 144, ripple=0.08)
    pose, K = pose_of([0.4, -0.9, 0.3], [10, -5, 750]), CULL.LINEMOD_K
    shuffled = f[np.random.RandomState(0).permutation(len(f))]
    r, base = both(v, shuffled, pose, K, 480, 640), raster(v, f, pose, K, 480, 640, True)
    for k in ("zbuf", "rgb", "nocs", "normal"):                  # the nearest face is the nearest face in any order
        assert torch.equal(bits(r[k]), bits(base[k])), k


# ----------------------------------------------------------------------------- coherent_face_order
@pytest.mark.parametrize("mesh", ["sphere", "torus"])
def test_coherent_face_order_keeps_the_depth_and_names_the_same_faces(mesh):
    from texpose_amd.surfel import coherent_face_order
    v, f = uv_sphere(24, 48, ripple=0.1) if mesh == "sphere" else torus(48, 24)
    pose = pose_of([0.3, -0.5, 0.2], [4, -3, 620]) if mesh == "sphere" else pose_of([1.2, 0.2, 0.0], [0, 5, 560])
    perm = coherent_face_order(v, f)
    assert not np.array_equal(perm, np.arange(len(f)))
    base, sorted_ = both(v, f, pose, K_for(120, 160), 120, 160), both(v, f[perm], pose, K_for(120, 160), 120, 160)
    for k in ("zbuf", "rgb", "nocs", "normal"):
        assert torch.equal(bits(base[k]), bits(sorted_[k])), k
    hit = base["zbuf"] > 0
    assert int(hit.sum()) > 1500 and torch.equal(sorted_["face"] >= 0, hit)
    back = cu(perm)[sorted_["face"][hit].long()]
    differ = torch.nonzero(back != base["face"][hit].long())
    assert len(differ) == 0, "%d pixels name another face: an exact z tie between two faces, or a bug" % len(differ)


# ----------------------------------------------------------------------------- determinism and capture
def raw_call(name, verts, faces, pose, K, out, ws, vcolor, norm):
    """The C entry point ``name`` on device tensors, writing into ``out`` (all five planes) with the caller's workspace."""
    from texpose_amd import _lib
    from texpose_amd.ops._base import _call, _float3
    a = _lib.MeshRasterArgs()
    a.verts, a.faces, a.vcolor, a.pose, a.intr = verts.data_ptr(), faces.data_ptr(), vcolor.data_ptr(), pose.data_ptr(), K.data_ptr()
    a.nocs_center, a.nocs_scale = _float3(norm[0]), _float3(norm[1])
    a.B, a.H, a.W, a.V, a.F = pose.shape[0], out["zbuf"].shape[1], out["zbuf"].shape[2], verts.shape[0], faces.shape[0]
    a.zbuf, a.face, a.rgb, a.nocs, a.normal = (out[k].data_ptr() for k in PLANES)
    a.workspace = ws.data_ptr()
    _call(name, a)


def test_two_runs_and_graph_replay_are_bit_equal():
    from texpose_amd import _lib
    rs = np.random.RandomState(8)
    v, f = soup(700, rs)                                        # three chunks, heavy overlap
    H, W, B = 120, 160, 2
    pose = np.stack([pose_of([0.05, 0.0, 0.3], [0, 0, 900]), pose_of([0.0, 0.08, -0.2], [3, 1, 950])])
    a, b = raster(v, f, pose, K_for(H, W), H, W, True), raster(v, f, pose, K_for(H, W), H, W, True)
    same(a, b)
    same(a, raster(v, f, pose, K_for(H, W), H, W, False))
    assert covered(a) > 3000
    vt, ft, ct, pt = cu(v), cu(f), cu(colours(v)), cu(pose)
    Kt = cu(np.tile(K_for(H, W), (B, 1, 1)))
    norm = tuple(np.asarray(x, np.float32) for x in REF.nocs_normalisation(v))
    need = int(_lib.load().tp_mesh_raster_culled_workspace_bytes(B, H, W, len(f)))
    assert need == 64 * B * 700 + 16 * B * 3
    ws = torch.empty(need // 4, device=DEV)
    out = {k: torch.empty_like(a[k]) for k in PLANES}
    run = lambda: raw_call("tp_mesh_raster_culled", vt, ft, pt, Kt, out, ws, ct, norm)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    same(a, out)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for _ in range(2):
        for t in out.values():
            t.view(torch.uint8).fill_(0xAB)
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        same(a, out)
    # the plain entry point on the culled call's (larger) workspace: the face records are laid out as before
    for t in out.values():
        t.view(torch.uint8).fill_(0xAB)
    raw_call("tp_mesh_raster", vt, ft, pt, Kt, out, ws, ct, norm)
    torch.cuda.synchronize()
    same(a, out)


# ----------------------------------------------------------------------------- the layers above
@pytest.fixture(scope="module")
def loop_inputs():
    """pnp_ref.end_to_end_inputs (the rippled sphere, 64 x 80, two poses about 900 mm away), coloured; the measurements are the plain
    rasteriser's planes at the true poses, the start 3 degrees and 4 .. 11 mm away."""
    from texpose_amd import ops
    e = PREF.end_to_end_inputs("sphere")
    K = np.tile(e["K"], (2, 1, 1))
    vcolor = (0.5 + 0.5 * np.sin(e["verts"].astype(np.float64) / 8.0 + np.array([0.0, 1.0, 2.0]))).astype(np.float32)
    truth = ops.mesh_raster(cu(e["verts"]), cu(e["faces"]), cu(e["P"]), cu(K), H=e["H"], W=e["W"], vcolor=cu(vcolor), face_ids=False, normals=False)
    hit = truth["zbuf"] > 0
    assert int(hit.sum()) > 1000
    return dict(e, K=cu(K), vcolor=vcolor, start=cu(IREF.perturbed(e["P"], np.random.RandomState(3))), depth=truth["zbuf"].clamp(min=0.0),
                image=torch.where(hit[..., None], truth["rgb"], torch.full_like(truth["rgb"], 0.5)), mask=hit.to(torch.uint8))


def counted(fn):
    """fn() with mesh_raster wrapped where the loops (ops.scene) and the modules (ops) look it up -> (its result, the ``cull`` of every
    rasteriser call)."""
    from texpose_amd import ops
    calls, real = [], ops.scene.mesh_raster
    assert ops.mesh_raster is real

    def wrapper(*a, **kw):
        calls.append(bool(kw.get("cull", False)))
        return real(*a, **kw)
    ops.scene.mesh_raster = ops.mesh_raster = wrapper
    try:
        return fn(), calls
    finally:
        ops.scene.mesh_raster = ops.mesh_raster = real


@pytest.mark.parametrize("which", ["depth", "photo", "silhouette", "joint"])
def test_refiners_with_cull_return_the_same_bits(loop_inputs, which):
    from texpose_amd import icp, joint, photo_align, silhouette
    c = loop_inputs
    mesh = (c["verts"], c["faces"])

    def run(cull):
        if which == "depth":
            return icp.DepthRefiner(*mesh, c["H"], c["W"], DEV, cull=cull).refine(c["start"], c["K"], c["depth"])
        if which == "photo":
            return photo_align.PhotoRefiner(*mesh, c["vcolor"], c["H"], c["W"], DEV, cull=cull).refine(c["start"], c["K"], c["image"])
        if which == "silhouette":
            return silhouette.SilhouetteRefiner(*mesh, c["H"], c["W"], DEV, cull=cull).refine(c["start"], c["K"], c["mask"])
        return joint.JointRefiner(*mesh, c["H"], c["W"], DEV, vcolor=c["vcolor"], cull=cull).refine(c["start"], c["K"], mask_or_sdf=c["mask"],
                                                                                                 image=c["image"], depth=c["depth"])
    (plain, calls_plain), (culled, calls_culled) = counted(lambda: run(False)), counted(lambda: run(True))
    passes = dict(depth=6, photo=11, silhouette=11, joint=21)[which]                 # iters + 1, one call per pass
    assert calls_plain == [False] * passes and calls_culled == [True] * passes
    assert set(plain) == set(culled) and "pose" in plain
    for k in plain:
        assert plain[k].dtype == culled[k].dtype and torch.equal(plain[k].view(torch.uint8), culled[k].view(torch.uint8)), k
    assert (plain["status"] == 0).all() and not torch.equal(plain["pose"], c["start"])


def test_surfel_renderer_store_and_vsd_with_cull_return_the_same_bits(loop_inputs):
    from texpose_amd import pose_error
    from texpose_amd.surfel import SurfelMapStore, SurfelRenderer
    c = loop_inputs
    pose = torch.as_tensor(c["P"]).clone()
    pose[:, :, 3] /= 100.0                                       # nerf.depth.scale 10: mm / 100
    maps, stores, errs = [], [], []
    for cull in (False, True):
        r = SurfelRenderer(c["verts"], c["faces"], c["vcolor"], c["H"], c["W"], DEV, cull=cull)
        assert r.cull is cull
        (m, calls) = counted(lambda: r.data_layer_maps(pose, c["K"], 10.0))
        assert calls == [cull]
        maps.append(m)
        stores.append(SurfelMapStore(r, pose, c["K"], 10.0, batch=1).maps)
        (e, calls) = counted(lambda: pose_error.vsd(cu(c["verts"]), cu(c["faces"]), c["start"], cu(c["P"]), c["K"], c["depth"], 100.0,
                                                    H=c["H"], W=c["W"], cull=cull))
        assert calls == [cull]
        errs.append(e)
    for pair in (maps, stores, errs):
        assert set(pair[0]) == set(pair[1]) and len(pair[0]) >= 2
        for k in pair[0]:
            assert torch.equal(pair[0][k].contiguous().view(torch.uint8), pair[1][k].contiguous().view(torch.uint8)), k
    assert set(maps[0]) == {"depth", "image_syn", "mask_syn", "nocs_pred", "normal_pred"} and float(maps[0]["mask_syn"].sum()) > 1000
    assert torch.isfinite(errs[0]["err"]).all()


# ----------------------------------------------------------------------------- the tool
def test_tool_with_cull_raster_writes_the_same_csv(tmp_path, capsys):
    """DESIGN section 22's three-frame scene of two instances through tools/refine_poses.py --joint --silhouette --rgb --occluders:
    the CSV written with --cull-raster is the CSV written without, byte for byte.  (The tool adds the wall-clock time of each batch to
    the rows' last column; its clock is held still here, so that the files can be compared whole.)"""
    import joint_ref as JREF
    import silhouette_ref as SREF
    from test_gpu_joint import TOOL_FRAMES, TOOL_H, TOOL_OCCLUDER_OID, TOOL_OID, TOOL_W, _load_tool, _write_ply, tool_scene
    from texpose_amd import ops
    from texpose_amd.bop_scene import BopSceneWriter
    from texpose_amd.surfel import load_ply
    H, W, F, oid = TOOL_H, TOOL_W, TOOL_FRAMES, TOOL_OID
    verts, faces = SREF.mesh_of("bent sphere")
    K, gt, front, moved = tool_scene()
    root, ply, est_csv = str(tmp_path / "scene"), str(tmp_path / "obj_000007.ply"), str(tmp_path / "est.csv")
    _write_ply(ply, verts, faces, np.rint(JREF.vertex_colours(verts) * 255.0).astype(np.uint8))
    vcolor = load_ply(ply)[2]
    target = ops.mesh_raster(cu(verts), cu(faces), cu(gt), cu(K), H=H, W=W, vcolor=cu(np.asarray(vcolor, np.float32)), face_ids=False, normals=False)
    whole = host(target["zbuf"]) > 0
    occ = host(ops.mesh_raster(cu(SREF.mesh_of("sphere")[0]), cu(SREF.mesh_of("sphere")[1]), cu(front), cu(K), H=H, W=W, face_ids=False,
                               normals=False)["zbuf"]) > 0
    photo = np.where(whole[..., None], host(target["rgb"]), 0.5)
    photo[occ] = JREF.OCCLUDER_COLOUR
    rgb8 = np.rint(np.clip(photo, 0.0, 1.0) * 255.0).astype(np.uint8)
    visib = np.stack([whole & ~occ, occ], 1).astype(np.uint8) * np.uint8(255)
    full = np.stack([whole, occ], 1).astype(np.uint8) * np.uint8(255)
    w = BopSceneWriter(root, K, 10.0, png_per_metre=2000)
    info = np.zeros((F, 2, 10), np.int32)
    info[:, :, 0], info[:, :, 1] = full.astype(bool).sum((2, 3)), visib.astype(bool).sum((2, 3))
    frames = []
    for k in range(F):
        pose = gt[k].copy()
        pose[:, 3] /= 100.0
        frames += w.add_views(pose[None], [oid, TOOL_OCCLUDER_OID], info[k][None], full[k][None], visib[k][None], rgb8[k][None],
                              np.zeros((1, H, W), np.uint16))
    w.close()
    refine = _load_tool("refine_poses")
    refine.time = types.SimpleNamespace(time=lambda: 0.0)
    refine.write_rows(est_csv, [(1, frames[k], oid, 0.5, moved[k, :, :3], moved[k, :, 3], 0.0) for k in range(F)])
    common = ["--scene", root, "--ply", "%d=%s" % (oid, ply), "--est", est_csv, "--device", DEV, "--joint", "--silhouette", "--rgb", "--occluders"]
    (_, calls_plain) = counted(lambda: refine.main(common + ["--out", str(tmp_path / "plain.csv")]))
    said_plain = capsys.readouterr().out
    (_, calls_culled) = counted(lambda: refine.main(common + ["--out", str(tmp_path / "culled.csv"), "--cull-raster"]))
    said_culled = capsys.readouterr().out
    assert calls_plain == [False] * 21 and calls_culled == [True] * 21
    assert "3 refined (0 with a failed last step)" in said_plain
    assert said_plain.replace("plain.csv", "X") == said_culled.replace("culled.csv", "X")
    plain, culled = open(str(tmp_path / "plain.csv"), "rb").read(), open(str(tmp_path / "culled.csv"), "rb").read()
    assert plain == culled and plain.count(b"\n") == 1 + F and plain != open(est_csv, "rb").read()
