"""GPU: the argument helpers of texpose_amd/ops/_base.py through the scene / pose entry points that use them, at the smallest shapes that reach
every branch: B = 2 views of 8 x 8, K = 2 objects, a tetrahedron, N = 64 correspondences, T = 4 hypotheses.  A caller's ``out`` tensors
come back as the same objects with the bits of a call that allocated its own; partial ``out`` dicts; workspaces that are too short or
badly aligned; one [3,3] intr against its [B,3,3] expansion; no allocation with ``out`` and ``workspace`` given.  Every refused call is
refused on the host, before any launch.  And the launch helper `_call` behind every wrapper: it launches on the current stream, and a
refusal of the library's own surfaces as TexposeLibraryError with the entry point's name, the ``_pair`` one for a paired launch."""
import numpy as np
import pytest
import torch

from texpose_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, H, W, K, N, T = 2, 8, 8, 2, 64, 4
DEPTH_SCALE, BG = 10.0, (0.0, 30.0)


def cu(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


def bits(t):
    """For an equality of bits (a NaN equals itself): float32 as int32, and the unsigned 16-bit pixels widened."""
    return t.view(torch.int32) if t.dtype == torch.float32 else t.to(torch.int32) if t.dtype == torch.uint16 else t


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def marked(t):
    """A tensor like ``t`` with every byte set to 77: what a call does not write stays visible."""
    m = torch.empty_like(t)
    m.view(torch.uint8).fill_(77)
    return m


def rot(axis, angle):
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


@pytest.fixture(scope="module")
def scene():
    """Made once and left unchanged: the mesh, the views, their rasters and a correspondence list."""
    verts = np.array([[30, 30, 30], [30, -30, -30], [-30, 30, -30], [-30, -30, 30]], np.float32)           # mm
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    normals = (verts / np.linalg.norm(verts, axis=1, keepdims=True)).astype(np.float32)
    pose_mm = np.stack([np.concatenate([rot((1, 2, 3), 0.3 + b), [[2.0 * b], [-3.0], [200.0 + 20 * b]]], 1) for b in range(B)]).astype(np.float32)
    k1 = np.array([[20.0, 0, W / 2], [0, 20.0, H / 2], [0, 0, 1]], np.float32)
    s = dict(verts=cu(verts), faces=cu(faces, torch.int32), normals=cu(normals), pose_mm=cu(pose_mm), k1=cu(k1), kb=cu(np.tile(k1, (B, 1, 1))))
    s["norm"] = (tuple(verts.mean(0)), (31.0, 31.0, 31.0))
    s["vcolor"] = cu((verts + 30) / 60)
    r = ops.mesh_raster(s["verts"], s["faces"], s["pose_mm"], s["kb"], H=H, W=W, vcolor=s["vcolor"], nocs_norm=s["norm"])
    shifted = s["pose_mm"].clone()
    shifted[:, 0, 3] += 25.0
    r2 = ops.mesh_raster(s["verts"], s["faces"], shifted, s["kb"], H=H, W=W, face_ids=False, normals=False)
    assert int((r["zbuf"] > 0).sum()) >= 4 and int((r2["zbuf"] > 0).sum()) >= 4
    s["raster"] = r
    s["zstack"] = torch.stack([r["zbuf"], r2["zbuf"]]).contiguous()                                        # [K,B,H,W]
    s["ids"] = torch.tensor([3, 7], dtype=torch.int32, device=DEV)
    s["boxes"] = cu(np.array([[[-0.3] * 3, [0.3] * 3], [[-0.05, -0.3, -0.3], [0.55, 0.3, 0.3]]], np.float32))   # NeRF units
    pose_nerf = pose_mm.copy()
    pose_nerf[:, :, 3] *= DEPTH_SCALE / 1000
    s["pose_nerf"] = cu(pose_nerf)
    rs = np.random.RandomState(5)
    xyz = rs.uniform(-30, 30, (B, N, 3)).astype(np.float32)
    cam = np.einsum("bij,bnj->bni", pose_mm[:, :, :3], xyz) + pose_mm[:, None, :, 3]
    xy = (cam[..., :2] / cam[..., 2:]) * 20.0 + [W / 2, H / 2]
    s.update(xy=cu(xy), xyz=cu(xyz), count=torch.tensor([N, 50], dtype=torch.int32, device=DEV))
    s["nocs"] = cu(rs.uniform(0, 1, (B, H, W, 3)))
    s["mask"] = cu(rs.uniform(size=(B, H, W)) < 0.6, torch.uint8)
    s["depth_test"] = r["zbuf"].clamp(min=0) + 3.0
    s["tau"] = cu(np.tile(np.array([[2.0, 5.0, 20.0]], np.float32), (B, 1)))
    s["ray_rgb"] = cu(rs.uniform(-0.1, 1.1, (B, H * W, 3)))
    s["ray_depth"] = cu(rs.uniform(0, 20, (B, H * W)))
    return s


def calls(s):
    """name -> (call(out=None or a dict), the part of key k's tensor that the call writes)."""
    r = s["raster"]
    whole = lambda res, k: res[k]
    hy = ops.pnp_hypotheses(s["xy"], s["xyz"], s["count"], s["kb"], T=T, seed=3)
    inl = ops.pnp_score(s["xy"], s["xyz"], s["count"], s["kb"], hy["hyp"], valid=hy["hyp_valid"])
    label = ops.scene_bounds(s["zstack"], None, s["ids"], depth_scale=DEPTH_SCALE, bg_range=BG, source="none")["label"]

    def bake(out=None):
        return ops.texture_bake(s["verts"], s["normals"], s["pose_mm"], s["kb"], r["rgb"], r["zbuf"],
                                **({} if out is None else dict(acc=out.get("acc"), count=out.get("count"))))

    def corr_written(res, k):                                       # entries from count[b] on are not written
        return res[k] if k == "count" else torch.cat([res[k][b, :int(res["count"][b])] for b in range(B)])

    return {
        "surfel_finish": (lambda out=None: ops.surfel_finish(r["zbuf"], r["nocs"], r["normal"], r["rgb"], out=out), whole),
        "scene_bounds": (lambda out=None: ops.scene_bounds(s["zstack"], s["boxes"], s["ids"], depth_scale=DEPTH_SCALE, bg_range=BG, source="box",
                                                           pose=s["pose_nerf"], intr=s["kb"], out=out), whole),
        "scene_annotate": (lambda out=None: ops.scene_annotate(s["zstack"], label, s["ids"], out=out), whole),
        "view_images": (lambda out=None: ops.view_images(s["ray_rgb"], s["ray_depth"], H=H, W=W, depth_scale=DEPTH_SCALE, out=out), whole),
        "vsd": (lambda out=None: ops.vsd(r["zbuf"], s["zstack"][1], s["depth_test"], s["kb"], s["tau"], out=out), whole),
        "texture_bake": (bake, whole),
        "corr_from_nocs": (lambda out=None: ops.corr_from_nocs(s["nocs"], s["mask"], *s["norm"], out=out), corr_written),
        "pnp_hypotheses": (lambda out=None: ops.pnp_hypotheses(s["xy"], s["xyz"], s["count"], s["kb"], T=T, seed=3, out=out), whole),
        "pnp_refine": (lambda out=None: ops.pnp_refine(s["xy"], s["xyz"], s["count"], s["kb"], hy["hyp"], inl, hy["hyp_valid"], out=out), whole),
    }


PARTIAL_KEY = {"corr_from_nocs": "count", "pnp_hypotheses": "hyp", "pnp_refine": "rms"}


@pytest.mark.parametrize("name", ["surfel_finish", "scene_bounds", "scene_annotate", "view_images", "vsd", "texture_bake", "corr_from_nocs",
                                  "pnp_hypotheses", "pnp_refine"])
def test_out_tensors_are_the_callers_and_hold_the_same_bits(scene, name):
    call, written = calls(scene)[name]
    first = call()
    mine = {k: marked(v) for k, v in first.items()}
    second = call(mine)
    assert set(second) == set(first)
    for k in first:
        assert second[k] is mine[k], k
        assert same(written(second, k), written(first, k)), k
    if name in PARTIAL_KEY:                                         # the PnP entry points take any subset of their outputs
        k = PARTIAL_KEY[name]
        one = {k: marked(first[k])}
        third = call(one)
        assert set(third) == set(first) and third[k] is one[k]
        assert all(same(written(third, j), written(first, j)) for j in first)
    else:                                                           # the others want them all: a missing key is the KeyError
        with pytest.raises(ValueError if name == "texture_bake" else KeyError):      # (acc and count are arguments: they come together)
            call({k: v for k, v in mine.items() if k != next(iter(mine))})
    wrong = dict(mine)
    k = next(iter(mine))
    for bad in (mine[k].double() if mine[k].dtype != torch.float64 else mine[k].float(), mine[k][..., :-1].contiguous(), mine[k].cpu(),
                torch.empty(mine[k].shape + (2,), dtype=mine[k].dtype, device=DEV)[..., 0]):
        wrong[k] = bad
        with pytest.raises(ValueError, match=name + ".*" + k):
            call(wrong)


def test_workspaces_too_short_or_misaligned(scene):
    s, r = scene, scene["raster"]
    lib = _lib.load()
    V = s["verts"].shape[0]
    hy = ops.pnp_hypotheses(s["xy"], s["xyz"], s["count"], s["kb"], T=T, seed=3)
    inl = ops.pnp_score(s["xy"], s["xyz"], s["count"], s["kb"], hy["hyp"], valid=hy["hyp_valid"])
    bake = lambda ws: ops.texture_bake(s["verts"], s["normals"], s["pose_mm"], s["kb"], r["rgb"], r["zbuf"], workspace=ws)
    refine = lambda ws: ops.pnp_refine(s["xy"], s["xyz"], s["count"], s["kb"], hy["hyp"], inl, hy["hyp_valid"], workspace=ws)
    corr = lambda ws: ops.corr_from_nocs(s["nocs"], s["mask"], *s["norm"], workspace=ws)
    ransac = lambda ws: ops.pnp_ransac(s["xy"], s["xyz"], s["count"], s["kb"], T=T, seed=3, workspace=ws)
    need_bake, need_pnp = int(lib.tp_texture_bake_workspace_bytes(V, B)), int(lib.tp_pnp_workspace_bytes(B, N, T))
    assert ops.texture_bake_workspace(V, B, DEV).numel() * 8 >= need_bake and ops.pnp_workspace(B, N, T, DEV).numel() * 8 >= need_pnp
    byte_buf = lambda n: torch.empty(n, dtype=torch.uint8, device=DEV)
    for call, need in ((bake, need_bake), (refine, need_pnp)):
        assert set(call(byte_buf(need))) == set(call(None))                                 # exactly enough is enough
        with pytest.raises(ValueError, match="workspace"):
            call(byte_buf(need - 1))
        for bad in (byte_buf(2 * need + 2)[::2], byte_buf(need).cpu(), "ws"):
            with pytest.raises(ValueError, match="workspace"):
                call(bad)
    off8 = byte_buf(max(need_bake, need_pnp) + 16)[8:]
    assert off8.data_ptr() % 16 == 8 and off8.is_contiguous()
    for call in (refine, corr, ransac):
        with pytest.raises(ValueError, match="16-byte aligned"):
            call(off8)
    # texture_bake's wrapper takes the view, as it always has; the alignment rule is then the library's own, on the host before a launch
    with pytest.raises(_lib.TexposeLibraryError, match="16-byte aligned"):
        bake(off8)


def test_one_intr_equals_its_expansion(scene):
    s, r = scene, scene["raster"]
    assert torch.equal(s["k1"][None].expand(B, 3, 3), s["kb"])
    for call in (lambda k: ops.mesh_raster(s["verts"], s["faces"], s["pose_mm"], k, H=H, W=W, vcolor=s["vcolor"], nocs_norm=s["norm"]),
                 lambda k: ops.vsd(r["zbuf"], s["zstack"][1], s["depth_test"], k, s["tau"]),
                 lambda k: ops.texture_bake(s["verts"], s["normals"], s["pose_mm"], k, r["rgb"], r["zbuf"]),
                 lambda k: ops.pnp_hypotheses(s["xy"], s["xyz"], s["count"], k, T=T, seed=3)):
        one, each = call(s["k1"]), call(s["kb"])
        assert set(one) == set(each) and all(same(one[k], each[k]) for k in one)
        for bad in (s["kb"][:1], torch.cat([s["kb"], s["kb"][:1]])):
            with pytest.raises(ValueError, match=r"intr \[B=2,3,3\] or \[3,3\] expected"):
                call(bad)
        with pytest.raises(_lib.TexposeLibraryError, match="intr must live on the GPU"):      # the device rule first, whatever the shape
            call(s["kb"].cpu()[:1])
    for bad, single in ((torch.zeros(2, 3, 3, device=DEV), True), (s["k1"], False)):        # the helper itself, at B = 3
        with pytest.raises(ValueError, match=r"some_op: intr \[B=3,3,3\]%s expected, got" % (r" or \[3,3\]" if single else "")):
            ops._intr_per_view("some_op", bad, 3, allow_single=single)
    with pytest.raises(ValueError, match=r"pose_errors: intr \[B=2,3,3\] expected"):         # no single intr where none was taken before
        ops.pose_errors(s["verts"], s["pose_mm"], s["pose_mm"], None, s["k1"])
    with pytest.raises(ValueError, match=r"normals_from_depth: intr \[B=2,3,3\] expected"):
        ops.normals_from_depth(r["zbuf"], s["pose_mm"], s["k1"])


def test_nothing_is_allocated_with_out_and_workspace_given(scene):
    s = scene
    label = ops.scene_bounds(s["zstack"], None, s["ids"], depth_scale=DEPTH_SCALE, bg_range=BG, source="none")["label"]
    ws = ops.pnp_workspace(B, N, T, DEV)
    routes = {
        "pnp_ransac": lambda out: ops.pnp_ransac(s["xy"], s["xyz"], s["count"], s["kb"], T=T, seed=3, workspace=ws, out=out),
        "vsd": lambda out: ops.vsd(s["raster"]["zbuf"], s["zstack"][1], s["depth_test"], s["kb"], s["tau"], out=out),
        "scene_bounds": lambda out: ops.scene_bounds(s["zstack"], s["boxes"], s["ids"], depth_scale=DEPTH_SCALE, bg_range=BG, source="box",
                                                     pose=s["pose_nerf"], intr=s["kb"], out=out),
        "scene_annotate": lambda out: ops.scene_annotate(s["zstack"], label, s["ids"], out=out),
    }
    for name, call in routes.items():
        out = {k: torch.empty_like(v) for k, v in call(None).items()}
        assert name != "pnp_ransac" or set(out) == set(ops.PNP_RANSAC_KEYS)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        res = call(out)
        assert torch.cuda.memory_allocated() == before, name
        assert torch.cuda.max_memory_allocated() == before, name    # not for a moment either
        assert all(res[k] is out[k] for k in out)
        del res, out                                                # (freed here, not inside the next route's measurement)


BCE_CAPTURE_NODES = 1       # measured on the commit before ops became a package: one captured ops.bce_logits_fwd call adds one kernel node


def test_launches_go_to_the_current_stream():
    x = torch.linspace(-3, 3, 64, device=DEV)
    eager = ops.bce_logits_fwd(x, 1.0)                              # (warm: nothing is loaded or made inside the capture)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(device=DEV), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        before = ops.capture_node_count()                           # counts the nodes of the stream that is current: the side stream
        out = ops.bce_logits_fwd(x, 1.0)
        rise = ops.capture_node_count() - before
    assert before is not None and rise == BCE_CAPTURE_NODES and ops.capture_node_count() is None
    graph.replay()
    torch.cuda.synchronize()
    assert same(out, eager)


def test_the_librarys_refusal_names_its_entry_point():
    z = torch.full((1, 4, 4), 500.0, device=DEV)
    with pytest.raises(_lib.TexposeLibraryError, match=r"^tp_vsd failed \(rc=-1\): tp_vsd: T = 17 tolerances, 1 \.\. 16 expected$"):
        ops.vsd(z, z, z, torch.eye(3, device=DEV), torch.ones(1, _lib.VSD_MAX_TAUS + 1, device=DEV))
    # a pair of the fused tail with one row more than it takes: refused by the library's size check, in front of the launch
    M, Kt, Nt, L, Ht = ops.DISC_TAIL_MAX_ROWS + 1, 8, 4, 1, 4
    zeros = lambda *shape: torch.zeros(*shape, device=DEV)
    tail = lambda: ops.disc_tail_fwd(zeros(M, Kt), zeros(Nt, Kt), zeros(M), zeros(Ht, Nt + 2 * L + 1), zeros(Ht, Ht), zeros(1, Ht), L, 0.2)
    with pytest.raises(_lib.TexposeLibraryError, match=r"^tp_disc_tail_fwd_pair failed \(rc=-1\): tp_disc_tail_fwd_pair: bad sizes \(at most 16 rows"):
        with ops.paired():
            tail()                                                  # held back: the second call launches both
            tail()
    assert not ops._pair_state["active"] and ops._pair_state["pending"] is None
    with pytest.raises(_lib.TexposeLibraryError, match=r"^tp_disc_tail_fwd failed \(rc=-1\): tp_disc_tail_fwd: bad sizes"):
        tail()
