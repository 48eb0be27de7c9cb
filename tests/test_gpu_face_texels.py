"""GPU: K35 tp_face_texel_shade (ops.face_texel_shade, ops.mesh_raster(texels=), texpose_amd.face_texels) against the fp64 restatement of
its contract in tests/face_texels_ref.py on the face planes of ops.mesh_raster (the rasteriser is not under test), on exact nodes, against
the rasteriser's own vertex colours at R = 1 and on the subdivided mesh, at its edges, captured, through the baker, the refiners and
the two tools."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import face_texels_ref as REF
import pnp_ref as PREF
import texture_bake_ref as TREF
from texpose_amd import _lib
from texpose_amd import face_texels as FT
from texpose_amd import texture_bake as TB

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DIST = 400.0
RE_FLOOR, TE_FLOOR = 1e-3, 1e-3          # deg, mm: the floors of tests/test_gpu_photo_align.py for the same geometry


def cu(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x, dtype=dtype).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def triangle():
    """one triangle that fills every frame used here from every pose of triangle_poses"""
    return np.array([[-2000.0, -1500.0, 0.0], [2000.0, -1500.0, 0.0], [0.0, 3000.0, 0.0]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)


def triangle_poses(B):
    out = np.zeros((B, 3, 4), dtype=np.float32)
    for b in range(B):
        a = 0.1 * b
        out[b] = [[1, 0, 0, 3.0 * b], [0, np.cos(a), -np.sin(a), -2.0 * b], [0, np.sin(a), np.cos(a), 400.0 + 50.0 * b]]
    return out


# the sub-pixel mesh: 1,472 faces on a sphere of radius 10 mm, 6 .. 10 pixels across in these frames: a face is at most about a pixel
MESHES = {"sphere": lambda: TREF.uv_sphere(12, 16), "torus": lambda: TREF.torus(24, 12), "triangle": triangle,
          "subpixel": lambda: TREF.uv_sphere(24, 32, radius=10.0)}
SIZES = {(37, 53): 120.0, (64, 80): 200.0}
_planes = {}


def planes(mesh, H, W, B):
    """fp32 inputs and the face plane of ops.mesh_raster, once per key"""
    key = (mesh, H, W, B)
    if key not in _planes:
        from texpose_amd import ops
        verts, faces = MESHES[mesh]()
        poses = triangle_poses(B) if mesh == "triangle" else TB.sphere_view_poses(max(B, 2), DIST).astype(np.float32)[:B]
        K = TREF.pinhole(H, W, SIZES[H, W])
        r = ops.mesh_raster(cu(verts), cu(faces), cu(poses), cu(K), H=H, W=W, normals=False)
        _planes[key] = dict(verts=verts, faces=faces, poses=poses, K=K, face=host(r["face"]), zbuf=host(r["zbuf"]), H=H, W=W, B=B)
    return _planes[key]


def shade(c, texels, face=None, **kw):
    from texpose_amd import ops
    names = ("verts", "faces", "poses", "K")
    v, f, p, k = (cu(kw.pop(n, c[n])) for n in names)
    out = ops.face_texel_shade(cu(c["face"] if face is None else face, torch.int32), v, f, cu(texels), p, k, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("size", list(SIZES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mesh", list(MESHES))
def test_kernel_against_the_restatement(mesh, size):
    """every pixel within 1e-6: the fp32 rounding of the output (colours in [0, 1]: half an ulp is 3e-8) over fp64 noise far below"""
    H, W = size
    rs = np.random.RandomState(7)
    for B in (1, 3):
        c = planes(mesh, H, W, B)
        covered = c["face"] >= 0
        assert covered.sum() >= (15 if mesh == "subpixel" else 300) * B and (mesh == "triangle") == bool(covered.all())
        for R in (1, 2, 3, 8, 64):
            texels = rs.rand(len(c["faces"]), FT.texel_count(R), 3).astype(np.float32)
            want = REF.shade(c["face"], c["verts"], c["faces"], texels, c["poses"], c["K"], H, W)
            got = host(shade(c, texels)).astype(np.float64)
            d = np.abs(got - want).max()
            print("%s %dx%d B=%d R=%d: max |kernel - restatement| %.2e on %d covered pixels" % (mesh, H, W, B, R, d, covered.sum()))
            assert got.shape == (B, H, W, 3) and d <= 1e-6
            assert (got[~covered] == 0).all() and (got[covered] != 0).any()


def test_exact_nodes():
    """A fronto-parallel right triangle whose R = 8 nodes fall on pixel centres (every quantity a small dyadic number, so the fp64 steps
    are exact): on a hand-made plane that gives the face its edge pixels too, those pixels equal the node texels bit for bit."""
    R, H, W = 8, 24, 24
    verts = np.array([[0, 0, 0], [16, 0, 0], [0, 16, 0]], dtype=np.float32)
    faces = np.array([[0, 1, 2]], dtype=np.int32)
    pose = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 64.0]]], dtype=np.float32)
    K = np.array([[64.0, 0, 4.5], [0, 64.0, 4.5], [0, 0, 1]], dtype=np.float32)          # vertex 0 at the centre of pixel (4, 4), 2 px per node
    texels = np.random.RandomState(2).rand(1, FT.texel_count(R), 3).astype(np.float32)
    c = dict(verts=verts, faces=faces, poses=pose, K=K)
    got = host(shade(c, texels, face=np.zeros((1, H, W), dtype=np.int32)))
    for n, (i, j) in enumerate(REF.node_list(R)):
        assert (got[0, 4 + 2 * j, 4 + 2 * i] == texels[0, n]).all(), (i, j)
    mid = got[0, 5, 5].astype(np.float64)                                                # halfway along the first cell's diagonal
    assert np.abs(mid - 0.5 * (texels[0, REF.node(1, 0, R)].astype(np.float64) + texels[0, REF.node(0, 1, R)])).max() <= 1e-7


def test_identities_with_the_rasterisers_vertex_colours():
    from texpose_amd import ops
    H, W = 64, 80
    for mesh in ("sphere", "torus"):
        c = planes(mesh, H, W, 3)
        v, f, p, k = cu(c["verts"]), cu(c["faces"]), cu(c["poses"]), cu(c["K"])
        vcolor = REF.fine_colour(c["verts"]).astype(np.float32)
        base = ops.mesh_raster(v, f, p, k, H=H, W=W, vcolor=cu(vcolor), normals=False)
        d1 = float((shade(c, vcolor[c["faces"]]) - base["rgb"]).abs().max())
        print("%s R=1 against mesh_raster(vcolor=): %.2e" % (mesh, d1))
        assert d1 <= 1e-5                                                                # the rasteriser's fp32 barycentrics
        covered = base["zbuf"] > 0
        for R in (2, 8):
            vs, fs, ni = FT.subdivide(c["verts"], c["faces"], R)
            col = REF.fine_colour(vs).astype(np.float32)
            rgb = shade(c, FT.texels_from_nodes(col, ni))
            for cull in (False, True):
                sub = ops.mesh_raster(cu(vs), cu(fs), p, k, H=H, W=W, vcolor=cu(col), normals=False, cull=cull)
                both = covered & (sub["zbuf"] > 0)
                differ = int((covered != (sub["zbuf"] > 0)).sum())
                d = float((rgb - sub["rgb"]).abs()[both].max())
                print("%s R=%d cull=%s against the subdivided mesh: %.2e on %d pixels, coverage differs on %d" % (mesh, R, cull, d, int(both.sum()), differ))
                assert d <= 5e-5 and differ <= 0.005 * int(covered.sum())


def guarded(B, H, W):
    """rgb [B,H,W,3] inside a buffer with guard bands of 4096 floats on both sides, all 0xAB bytes"""
    n, g = B * H * W * 3, 4096
    buf = torch.empty(n + 2 * g, device=DEV)
    buf.view(torch.uint8).fill_(0xAB)
    return buf, buf[g:g + n].view(B, H, W, 3), g


def guards_intact(buf, g):
    b = buf.view(torch.uint8)
    return bool((b[:4 * g] == 0xAB).all()) and bool((b[-4 * g:] == 0xAB).all())


def test_edges_write_zeros_and_nothing_else():
    H, W, B = 37, 53, 3
    c = planes("sphere", H, W, B)
    F = len(c["faces"])
    texels = np.random.RandomState(3).rand(F, FT.texel_count(8), 3).astype(np.float32)
    full = np.zeros((B, H, W), dtype=np.int32)                       # a hand-made plane: every pixel claims a face
    full[:] = (np.arange(H * W).reshape(H, W) % F)[None]
    # background and the plane's own values
    buf, out, g = guarded(B, H, W)
    shade(c, texels, out=out)
    assert guards_intact(buf, g) and bool((out[cu(c["face"] < 0)] == 0).all()) and bool(out.abs().sum() > 0)
    # a hand-made plane holding -1, -5, F and 2^30 beside valid entries
    plane = full.copy()
    bad = np.zeros((B, H, W), dtype=bool)
    for k, value in enumerate((-1, -5, F, 1 << 30)):
        bad[:, :, k::7] = True
        plane[:, :, k::7] = value
    buf, out, g = guarded(B, H, W)
    shade(c, texels, face=plane, out=out)
    want = REF.shade(plane, c["verts"], c["faces"], texels, c["poses"], c["K"], H, W)
    assert guards_intact(buf, g) and bool((out[cu(bad)] == 0).all()) and np.abs(host(out) - want).max() <= 1e-6
    assert (want[~bad] != 0).any()
    # NaN, Inf and behind-camera poses under the full plane
    poses = c["poses"].copy()
    poses[0, 1, 2] = np.nan
    poses[1, :, 3] = [np.inf, 0.0, 400.0]
    poses[2, 2, 3] = -400.0
    buf, out, g = guarded(B, H, W)
    shade(c, texels, face=full, poses=poses, out=out)
    assert guards_intact(buf, g) and bool((out == 0).all())
    huge = c["poses"].copy()
    huge[:, :, 3] = [1e30, -1e30, 1.0]
    buf, out, g = guarded(B, H, W)
    shade(c, texels, face=full, poses=huge, out=out)
    assert guards_intact(buf, g) and bool(torch.isfinite(out).all())         # (whatever such a pose shades to: finite, in place)
    # faces with an out-of-range vertex: zeros there, the rest as before
    faces = c["faces"].copy()
    faces[::3, 1] = len(c["verts"])
    faces[1::3, 2] = -1
    buf, out, g = guarded(B, H, W)
    shade(c, texels, face=full, faces=faces, out=out)
    broken = (np.arange(F) % 3 != 2)[full]
    want = REF.shade(full, c["verts"], faces, texels, c["poses"], c["K"], H, W)
    assert guards_intact(buf, g) and bool((out[cu(broken)] == 0).all()) and np.abs(host(out) - want).max() <= 1e-6 and (want != 0).any()
    # NaN and Inf texels: zeros where they are touched
    bad_tex = texels.copy()
    bad_tex[::2] = np.nan
    bad_tex[1::4] = np.inf
    buf, out, g = guarded(B, H, W)
    shade(c, bad_tex, face=full, out=out)
    assert guards_intact(buf, g) and bool(torch.isfinite(out).all()) and bool((out[cu(full % 2 == 0)] == 0).all())


def test_refused_arguments_launch_nothing():
    from texpose_amd import ops
    c = planes("sphere", 37, 53, 1)
    F, V = len(c["faces"]), len(c["verts"])
    t = dict(verts=cu(c["verts"]), faces=cu(c["faces"]), texels=torch.rand(F, 6, 3, device=DEV), pose=cu(c["poses"]), intr=cu(c["K"][None]),
             face=cu(c["face"]))
    buf, out, g = guarded(1, 37, 53)
    lib = _lib.load()

    def call(**kw):
        a = _lib.FaceTexelShadeArgs()
        for k, v in t.items():
            setattr(a, k, v.data_ptr())
        a.B, a.H, a.W, a.V, a.F, a.R, a.rgb = 1, 37, 53, V, F, 2, out.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.tp_face_texel_shade(C.byref(a), None), lib.tp_last_error().decode()

    for kw in (dict(B=0), dict(H=-1), dict(W=0), dict(V=0), dict(F=0), dict(R=0), dict(R=65), dict(H=65536, W=32768), dict(F=1 << 30, R=8),
               dict(rgb=None), dict(texels=None), dict(face=None)):
        rc, msg = call(**kw)
        assert rc == -1 and "tp_face_texel_shade" in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.uint8) == 0xAB).all())                # a refused call launches nothing
    assert call()[0] == 0
    torch.cuda.synchronize()
    assert guards_intact(buf, g) and bool(torch.isfinite(out).all())
    args = (t["face"], t["verts"], t["faces"], t["texels"], t["pose"], t["intr"])
    with pytest.raises(ValueError):
        ops.face_texel_shade(args[0], args[1], args[2], t["texels"][:, :5], *args[4:])          # 5 is no T(R)
    with pytest.raises(ValueError):
        ops.face_texel_shade(args[0], args[1], args[2], t["texels"][:-1], *args[4:])
    with pytest.raises(ValueError):
        ops.face_texel_shade(args[0].float(), *args[1:])
    with pytest.raises(ValueError):
        ops.face_texel_shade(*args, out=torch.empty(1, 37, 53, 4, device=DEV))
    with pytest.raises(ValueError):
        ops.mesh_raster(t["verts"], t["faces"], t["pose"], t["intr"], H=37, W=53, vcolor=torch.rand(V, 3, device=DEV), texels=t["texels"])
    with pytest.raises(ValueError):
        ops.photo_align(t["verts"], t["faces"], None, t["pose"], t["intr"], torch.rand(1, 37, 53, 3, device=DEV))
    with pytest.raises(ValueError):
        ops.photo_align(t["verts"], t["faces"], torch.rand(V, 3, device=DEV), t["pose"], t["intr"], torch.rand(1, 37, 53, 3, device=DEV), texels=t["texels"])


def test_determinism_graph_replay_and_mesh_raster_texels():
    from texpose_amd import ops
    H, W, B = 64, 80, 3
    c = planes("torus", H, W, B)
    v, f, p, k = cu(c["verts"]), cu(c["faces"]), cu(c["poses"]), cu(c["K"][None].repeat(B, 0))
    texels = torch.rand(len(c["faces"]), FT.texel_count(8), 3, device=DEV)
    face = cu(c["face"])
    first, again = ops.face_texel_shade(face, v, f, texels, p, k), ops.face_texel_shade(face, v, f, texels, p, k)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32))
    cap = torch.empty_like(first)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.face_texel_shade(face, v, f, texels, p, k, out=cap)
    for _ in range(2):
        cap.view(torch.uint8).fill_(0xAB)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap.view(torch.int32), first.view(torch.int32))
    # mesh_raster(texels=) is the two-call route, bit for bit, with and without cull and whatever face_ids says
    for cull in (False, True):
        plain = ops.mesh_raster(v, f, p, k, H=H, W=W, normals=False, cull=cull)
        assert torch.equal(plain["face"], face)
        for ids in (False, True):
            one = ops.mesh_raster(v, f, p, k, H=H, W=W, normals=False, cull=cull, texels=texels, face_ids=ids)
            assert torch.equal(one["rgb"].view(torch.int32), first.view(torch.int32)) and torch.equal(one["face"], face)
            assert torch.equal(one["zbuf"].view(torch.int32), plain["zbuf"].view(torch.int32))
    from texpose_amd.surfel import SurfelRenderer
    pose_nerf = TB.poses_to_nerf_units(torch.from_numpy(c["poses"]), 10.0).float()
    r = SurfelRenderer(c["verts"], c["faces"], None, H, W, DEV, texels=texels)(pose_nerf, c["K"], 10.0)
    assert r.rgb_syn.shape == (B, 3, H, W) and float(r.rgb_syn.abs().sum()) > 0 and bool((~(r.rgb_syn != 0).any(1) | (r.depth > 0)).all())
    with pytest.raises(ValueError):
        SurfelRenderer(c["verts"], c["faces"], np.zeros_like(c["verts"]), H, W, DEV, texels=texels)


def test_face_texel_baker_against_the_restatement():
    """FaceTexelBaker = K27 on the nodes of the subdivided mesh with the base mesh's depth planes: section 17's tolerances (the counts
    equal wherever no pair lies in the 1e-4 margin band, which holds <= 0.5 % of the pairs; colours within 8 ulp32(max(H, W)) + 1e-6)."""
    from texpose_amd import ops
    R, H, W, B = 2, 64, 64, 14
    verts, faces = TREF.uv_sphere(12, 16)
    poses, K = TB.sphere_view_poses(B, DIST).astype(np.float32), TREF.pinhole(H, W, 200.0)
    rgb = TREF.smooth_image(B, H, W)
    baker = FT.FaceTexelBaker(verts, faces, R, H, W, DEV)
    baker.add_views(cu(rgb[:5]), cu(poses[:5]), cu(K))
    baker.add_views(cu(rgb[5:]), cu(poses[5:]), cu(K))
    assert baker.views == B
    res = baker.result(fill=True)
    vs, fs, ni = REF.subdivide(verts, faces, R)
    assert (baker.verts_sub == vs).all() and (baker.faces_sub == fs).all() and (baker.node_index_host == ni).all()
    zbuf = host(ops.mesh_raster(cu(verts), cu(faces), cu(poses), cu(K), H=H, W=W, face_ids=False, normals=False)["zbuf"])
    ref = TREF.bake(vs, TB.vertex_normals(vs, fs), poses, K, rgb, zbuf)
    band = (ref["margin"] < 1e-4).sum(1)
    clean = band == 0
    count = host(res.count).astype(np.int64)
    assert band.sum() <= 0.005 * ref["margin"].size and (count[clean] == ref["count"][clean]).all() and (np.abs(count - ref["count"]) <= band).all()
    want, seen = TREF.vcolor_of(ref["acc"])
    both = clean & seen & host(res.seen)
    tol = 8.0 * float(np.spacing(np.float32(max(H, W)))) + 1e-6
    d = np.abs(host(res.vcolor_sub) - np.clip(want, 0, 1))[both].max()
    print("FaceTexelBaker R=%d: %d of %d nodes compared, max |dcolour| %.2e (tol %.2e), filled %d, unseen %d" % (R, both.sum(), len(vs), d, tol, res.filled, res.unseen))
    assert both.sum() >= 0.95 * len(vs) and d <= tol and res.unseen == 0
    # the texture is the nodes' colours gathered per face: continuous across edges by construction
    assert res.texels.shape == (len(faces), FT.texel_count(R), 3) and torch.equal(res.texels, res.vcolor_sub[cu(ni)])
    baker.reset()
    assert baker.views == 0 and not bool(baker.nodes.acc.any())


def test_refiners_with_texels():
    """photo_align(texels=) and joint_align(texels=) from the start face_texels_ref.loop_inputs documents, on the photograph rendered
    from the same texels.  The bar: the CPU loop's final errors (face_texels_ref.LOOP_FINAL, checked by the CPU tests) plus what the
    photo tests allow between device and restatement -- once more that error and the floors: 2 x error + floor.  No comparison with
    the vertex-colour route is asserted (a finer texture narrows the basin); both are printed."""
    from texpose_amd import joint, ops, photo_align
    import photo_ref as PH
    c = REF.loop_inputs()
    v, f, K, start, image, texels = (cu(c[k]) for k in ("verts", "faces", "K", "start", "image", "texels"))
    runs = {"photo_align(texels=)": ops.photo_align(v, f, None, start, K, image, tau=0.5, iters=10, damping=1e-6, texels=texels),
            "joint_align(texels=)": ops.joint_align(v, f, start, K, image=image, texels=texels, weights=(0.0, 1.0, 0.0), tau=0.5, iters=10, damping=1e-6)}
    runs["PhotoRefiner"] = photo_align.PhotoRefiner(c["verts"], c["faces"], None, c["H"], c["W"], DEV, tau=0.5, iters=10, texels=c["texels"]).refine(start, K, image)
    runs["JointRefiner"] = joint.JointRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV, texels=c["texels"], weights=(0.0, 1.0, 0.0), tau=0.5,
                                              iters=10).refine(start, K, image=image)
    for name, got in runs.items():
        assert host(got["status"]).tolist() == [0, 0], name
        for b in range(2):
            re, te = PREF.pose_error(host(got["pose"])[b], c["P"][b])
            print("%s pose %d: %.3g deg %.3g mm (%d pixels) | CPU loop %.3g deg %.3g mm" % ((name, b, re, te, int(got["inliers"][b])) + REF.LOOP_FINAL[b]))
            assert re <= 2 * REF.LOOP_FINAL[b][0] + RE_FLOOR and te <= 2 * REF.LOOP_FINAL[b][1] + TE_FLOOR, name
            assert int(got["inliers"][b]) >= 300
    assert torch.equal(runs["PhotoRefiner"]["pose"], runs["photo_align(texels=)"]["pose"])
    assert torch.equal(runs["JointRefiner"]["pose"], runs["joint_align(texels=)"]["pose"])
    # for the record: the vertex-colour route on ITS own photograph from the same start
    vcolor = cu(PH.vertex_colours(c["verts"]))
    photo = ops.mesh_raster(v, f, cu(c["P"]), K, H=c["H"], W=c["W"], vcolor=vcolor, face_ids=False, normals=False)
    photo = torch.where((photo["zbuf"] > 0)[..., None], photo["rgb"], torch.full_like(photo["rgb"], PH.BACKGROUND))
    plain = ops.photo_align(v, f, vcolor, start, K, photo, tau=0.5, iters=10, damping=1e-6)
    for b in range(2):
        print("vertex colours pose %d: %.3g deg %.3g mm" % ((b,) + PREF.pose_error(host(plain["pose"])[b], c["P"][b])))


def test_tools_bake_with_texel_res_then_refine_with_texels(tmp_path):
    """bake_texture --texel-res 4 on a random-weight checkpoint, then refine_poses --rgb --texels on a scene rendered from the baked
    texels: files and shapes, not quality."""
    import oracle.texpose_oracle as O
    from texpose_amd import checkpoint as ck, ops
    from texpose_amd.bop_scene import BopSceneWriter
    from texpose_amd.graph import Graph
    from texpose_amd.options import default_options
    from texpose_amd.surfel import load_ply
    H, W, N, oid = 48, 64, 8, 5
    opt = default_options(H=H, W=W, device=DEV)
    opt.nerf.sample_intvs, opt.nerf.sample_stratified = N, False
    opt.arch.mlp_precision = "fp32"
    graph = Graph(opt).to(DEV)
    graph.nerf.load_state_dict({**graph.nerf.state_dict(), **{k: v.to(DEV) for k, v in O.make_params(3).items()}})
    graph.attach_latents(4, opt)
    torch.save(ck.make_checkpoint(graph, epoch=1, it=10), str(tmp_path / "model.ckpt"))
    verts, faces = TREF.uv_sphere(12, 16)
    TB.write_ply(str(tmp_path / "sphere.ply"), verts, faces, np.zeros_like(verts))
    out, report = tmp_path / "textured.ply", tmp_path / "bake.json"
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "tools", "bake_texture.py"), "--checkpoint", str(tmp_path / "model.ckpt"),
           "--ply", "%d=%s" % (oid, tmp_path / "sphere.ply"), "--sphere", "6", "--distance-mm", "400", "--focal", "150", "--H", str(H), "--W", str(W),
           "--samples", str(N), "--precision", "fp32", "--out", str(out), "--report", str(report), "--verify", "--texel-res", "4"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    v, f, col = load_ply(str(out))
    assert (v == verts).all() and (f == faces).all() and col is not None and col.shape == (len(verts), 3)
    texel_file = tmp_path / "textured.texels.npz"
    texels, R = FT.load_texels(str(texel_file), faces)
    rep = json.loads(report.read_text())
    assert R == 4 and texels.shape == (len(faces), 15, 3) and np.isfinite(texels).all() and texels.min() >= 0 and texels.max() <= 1
    assert rep["texels"]["R"] == 4 and rep["texels"]["nodes"] == len(FT.subdivide(verts, faces, 4)[0]) and rep["texels"]["file"] == str(texel_file)
    assert "PSNR" in p.stdout and rep["verify"]["pixels"] > 0
    corner = texels[:, [0, 4, 14]]                                     # nodes (0,0), (R,0), (0,R): the PLY's vertex colours at 8 bits
    assert np.abs(corner - col[faces]).max() <= 0.5 / 255 + 1e-6
    # a scene of three frames rendered from the texels, estimates a little off
    K = TREF.pinhole(H, W, 150.0)
    gt = TB.sphere_view_poses(3, 400.0).astype(np.float32)
    r = ops.mesh_raster(cu(verts), cu(faces), cu(gt), cu(K), H=H, W=W, texels=cu(texels), normals=False)
    z = host(r["zbuf"])
    rgb8 = np.where((z > 0)[..., None], np.rint(np.clip(host(r["rgb"]), 0.0, 1.0) * 255.0), 128.0).astype(np.uint8)
    depth16 = np.where(z > 0, np.rint(z / 0.5), 0).astype(np.uint16)
    root, est_csv, out_csv = str(tmp_path / "scene"), str(tmp_path / "est.csv"), str(tmp_path / "refined.csv")
    w = BopSceneWriter(root, K, 10.0, png_per_metre=2000)
    info = np.zeros((3, 10), np.int32)
    info[:, 0] = info[:, 1] = (z > 0).sum((1, 2))
    frames = []
    for k in range(3):
        pose = gt[k].copy()
        pose[:, 3] /= 100.0
        frames += w.add_views(pose[None], [oid], info[k][None, None], np.zeros((1, 1, H, W), np.uint8), np.zeros((1, 1, H, W), np.uint8),
                              rgb8[k][None], depth16[k][None])
    w.close()
    spec = importlib.util.spec_from_file_location("refine_poses_tool", os.path.join(REPO, "tools", "refine_poses.py"))
    refine = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(refine)
    moved = gt.astype(np.float64).copy()
    moved[:, :, 3] += [1.0, -1.0, 2.0]
    refine.write_rows(est_csv, [(1, frames[k], oid, 0.5, moved[k, :, :3], moved[k, :, 3], 0.0) for k in range(3)])
    # the colourless PLY serves: the colour comes from the texels
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "tools", "refine_poses.py"), "--scene", root, "--ply",
                          str(tmp_path / "sphere.ply"), "--est", est_csv, "--out", out_csv, "--device", DEV, "--rgb", "--iters-rgb", "3", "--texels",
                          "%d=%s" % (oid, texel_file)], capture_output=True, text=True)
    assert run.returncode != 0 and "names an object without a --ply" in run.stderr        # keyed like --ply: a bare --ply has no id 5
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "tools", "refine_poses.py"), "--scene", root, "--ply",
                          str(tmp_path / "sphere.ply"), "--est", est_csv, "--out", out_csv, "--device", DEV, "--rgb", "--iters-rgb", "3", "--texels",
                          str(texel_file)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "3 rows, 3 refined" in run.stdout
    rows = refine.read_rows(out_csv)
    assert len(rows) == 3 and all(np.isfinite(row[4]).all() and np.isfinite(row[5]).all() and row[4].shape == (3, 3) for row in rows)
    ops.check_mlp_status(torch.device(DEV))
