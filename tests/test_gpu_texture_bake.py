"""GPU: K27 tp_texture_bake (ops.texture_bake, texpose_amd.texture_bake) against the fp64 restatement of its contract in
tests/texture_bake_ref.py on the same fp32 inputs and the same depth planes (the rasteriser is not under test), at its edges,
streamed, captured, round-tripped through the rasteriser, and end to end through tools/bake_texture.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import texture_bake_ref as REF
from texpose_amd import _lib
from texpose_amd import texture_bake as TB

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DIST = 400.0
BAND = 1e-4                                                          # relative margin below which a decision may flip


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def colour_tol(H, W):
    """8 ulp32(max(H, W)) + 1e-6: the bilinear fraction is a difference of numbers of size <= max(H, W); images are in [0, 1]."""
    return 8.0 * float(np.spacing(np.float32(max(H, W)))) + 1e-6


MESHES = {"torus": lambda: REF.torus(24, 12), "ripple": lambda: REF.uv_sphere(20, 24, ripple=0.15), "sphere": lambda: REF.uv_sphere(12, 16)}
_cases = {}


def case(mesh, H, W, f, B, V=None, weighted=False, vertex0=0):
    """Inputs (fp32, as the kernel gets them), the depth planes of ops.mesh_raster for the WHOLE mesh, and the restatement's result for
    the first V vertices from ``vertex0``: made once per key and left unchanged."""
    key = (mesh, H, W, f, B, V, weighted, vertex0)
    if key not in _cases:
        from texpose_amd import ops
        verts, faces = MESHES[mesh]()
        normals = TB.vertex_normals(verts, faces)
        poses, K = TB.sphere_view_poses(max(B, 2), DIST).astype(np.float32)[:B], REF.pinhole(H, W, f)
        zbuf = host(ops.mesh_raster(cu(verts), cu(faces), cu(poses), cu(K), H=H, W=W, face_ids=False, normals=False)["zbuf"])
        rgb = REF.smooth_image(B, H, W)
        weight = None
        if weighted:
            r, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
            weight = np.broadcast_to(0.55 + 0.45 * np.sin(0.2 * r + 0.13 * j)[None], (B, H, W)).astype(np.float32).copy()
        sl = slice(vertex0, vertex0 + (V or len(verts)))
        c = dict(verts=verts[sl].copy(), normals=normals[sl].copy(), faces=faces, all_verts=verts, poses=poses, K=K, rgb=rgb, zbuf=zbuf, weight=weight,
                 H=H, W=W, B=B)
        c["ref"] = REF.bake(c["verts"], c["normals"], poses, K, rgb, zbuf, weight)
        _cases[key] = c
    return _cases[key]


def run_kernel(c, **kw):
    from texpose_amd import ops
    names = ("verts", "normals", "poses", "K", "rgb", "zbuf")
    out = ops.texture_bake(*[cu(kw.get(k, c[k])) for k in names], None if kw.get("weight", c["weight"]) is None else cu(kw.get("weight", c["weight"])),
                           **{k: v for k, v in kw.items() if k not in names + ("weight",)})
    torch.cuda.synchronize()
    return out


def compare(c, out, ref=None, label=""):
    """count equal wherever no pair of the vertex lies in the margin band (and within the number of band pairs elsewhere); the band holds
    <= 0.5 % of the pairs; vcolor within colour_tol and the weight sum within 1e-5 relative where both saw the vertex."""
    ref = c["ref"] if ref is None else ref
    acc, count = host(out["acc"]).astype(np.float64), host(out["count"]).astype(np.int64)
    band = (ref["margin"] < BAND).sum(1)
    share = band.sum() / ref["margin"].size
    clean = band == 0
    tol = colour_tol(c["H"], c["W"])
    both = clean & (count > 0) & (ref["count"] > 0) & (ref["acc"][:, 3] > 0)
    vg, vr = acc[:, :3] / np.where(both, acc[:, 3], 1)[:, None], ref["acc"][:, :3] / np.where(both, ref["acc"][:, 3], 1)[:, None]
    dcol = np.abs(vg - vr)[both].max() if both.any() else 0.0
    dw = (np.abs(acc[:, 3] - ref["acc"][:, 3]) / np.where(both, ref["acc"][:, 3], 1))[both].max() if both.any() else 0.0
    print("%s: band share %.2e, count mismatches %d (clean %d), max |dcolour| %.2e (tol %.2e), max rel dw %.2e, used pairs %d of %d"
          % (label, share, (count != ref["count"]).sum(), (count != ref["count"])[clean].sum(), dcol, tol, dw, ref["used"].sum(), ref["used"].size))
    assert share <= 0.005
    assert (count[clean] == ref["count"][clean]).all()
    assert (np.abs(count - ref["count"]) <= band).all()
    assert np.isfinite(acc).all()
    assert dcol <= tol
    assert dw <= 1e-5
    assert (acc[clean & (ref["count"] == 0)] == 0).all()
    return both


# slices: L = max(4, ...) = 4 at these sizes, so B = 14 and 13 end in a short slice, B = 1 is one slice of one view
SHAPES = [
    ("ripple", 64, 80, 200.0, 14, None, False, 0),                   # V = 504 (two vertex tiles)
    ("torus", 37, 53, 120.0, 14, 257, True, 0),                      # a sub-mesh of 257 vertices: one thread into the second tile
    ("ripple", 37, 53, 120.0, 1, None, True, 0),
    ("torus", 64, 80, 200.0, 13, None, False, 0),                    # V = 288
    ("torus", 64, 80, 200.0, 14, 1, False, 7),                       # V = 1
    ("ripple", 64, 80, 200.0, 1, 1, False, 100),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s-%dx%d-B%d-V%s%s" % (s[0], s[1], s[2], s[4], s[5] or "all", "-w" if s[6] else ""))
def test_kernel_against_the_restatement(shape):
    c = case(*shape)
    lib = _lib.load()
    V, B = len(c["verts"]), c["B"]
    assert lib.tp_texture_bake_slices(V, B) == -(-B // min(B, 4))
    both = compare(c, run_kernel(c), label=str(shape))
    if V > 1:                                                        # the views do reach the mesh (one view: a good part of one side)
        assert both.sum() >= (0.9 if B >= 13 else 0.15) * V
        assert c["ref"]["used"].sum() >= (0.2 if B >= 13 else 0.15) * c["ref"]["used"].size


def test_behind_the_camera_and_outside_the_image():
    c = dict(case("sphere", 64, 64, 200.0, 2))
    # the camera inside the sphere's hull: part of the mesh at z <= 0
    near = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 20.0]]], dtype=np.float32)
    from texpose_amd import ops
    z = host(ops.mesh_raster(cu(c["all_verts"]), cu(c["faces"]), cu(near), cu(c["K"]), H=64, W=64, face_ids=False, normals=False)["zbuf"])
    c.update(poses=near, zbuf=z, rgb=REF.smooth_image(1, 64, 64), B=1)
    ref = REF.bake(c["verts"], c["normals"], near, c["K"], c["rgb"], z)
    out = run_kernel(c)
    compare(c, out, ref, "behind")
    behind = c["verts"][:, 2] + 20.0 <= 0
    assert behind.sum() > 50 and (host(out["count"])[behind] == 0).all() and (host(out["acc"])[behind] == 0).all()
    # far off to the side, far away, NaN and Inf poses: no tap inside the image, nothing counted, nothing read
    away = np.repeat(near, 6, 0)
    away[0, :, 3] = [5000.0, 0, 400.0]
    away[1, :, 3] = [0, -5000.0, 400.0]
    away[2, :, 3] = [1e30, 1e30, 1.0]
    away[3, 0, 0] = np.nan
    away[4, :, 3] = [np.inf, 0, 400.0]
    away[5, :, 3] = [0, 0, -400.0]
    c.update(poses=away, zbuf=np.full((6, 64, 64), 400.0, dtype=np.float32), rgb=REF.smooth_image(6, 64, 64), B=6)
    out = run_kernel(c)
    assert (host(out["count"]) == 0).all() and (host(out["acc"]) == 0).all()
    # the image edge: a principal point that puts the sphere across the border, taps at -1 and at H / W
    c2 = dict(case("sphere", 64, 64, 200.0, 14))
    K = c2["K"].copy()
    K[0, 2], K[1, 2] = 3.0, 61.5
    z = host(ops.mesh_raster(cu(c2["all_verts"]), cu(c2["faces"]), cu(c2["poses"]), cu(K), H=64, W=64, face_ids=False, normals=False)["zbuf"])
    c2.update(K=K, zbuf=z)
    ref = REF.bake(c2["verts"], c2["normals"], c2["poses"], K, c2["rgb"], z)
    assert ref["used"].sum() > 100 and (ref["reached"] & ~ref["used"]).sum() > 0
    compare(c2, run_kernel(c2), ref, "border")


def test_nan_and_inf_in_the_images_and_a_zero_weight_plane():
    c = dict(case("torus", 64, 80, 200.0, 14, None, True))
    rs = np.random.RandomState(3)
    rgb, zbuf, weight = c["rgb"].copy(), c["zbuf"].copy(), c["weight"].copy()
    bad = rs.rand(*rgb.shape) < 0.02
    rgb[bad] = rs.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
    badz = rs.rand(*zbuf.shape) < 0.03
    zbuf[badz] = rs.choice([np.nan, np.inf, -np.inf, 0.0], size=int(badz.sum()))
    badw = rs.rand(*weight.shape) < 0.02
    weight[badw] = rs.choice([np.nan, np.inf], size=int(badw.sum()))
    weight[5] = 0.0                                                  # one view without weight
    c.update(rgb=rgb, zbuf=zbuf, weight=weight)
    ref = REF.bake(c["verts"], c["normals"], c["poses"], c["K"], rgb, zbuf, weight)
    clean = case("torus", 64, 80, 200.0, 14, None, True)["ref"]
    assert ref["used"].sum() < clean["used"].sum() and ref["used"][:, 5].sum() > 20      # taps were dropped; view 5 still counts
    out = run_kernel(c)
    compare(c, out, ref, "nan/inf")
    # the zero-weight view adds nothing: the same sums without it (other slices, so to rounding), its pairs only in count
    keep = [b for b in range(14) if b != 5]
    c6 = dict(c, poses=c["poses"][keep], rgb=rgb[keep], zbuf=zbuf[keep], weight=weight[keep], B=13)
    out6 = run_kernel(c6)
    a, a6 = host(out["acc"]).astype(np.float64), host(out6["acc"]).astype(np.float64)
    assert np.abs(a - a6).max() <= 1e-6 * max(1.0, np.abs(a).max())
    assert ((host(out["count"]) - host(out6["count"])) == ref["used"][:, 5]).all()
    one = dict(c, poses=c["poses"][5:6], rgb=rgb[5:6], zbuf=zbuf[5:6], weight=weight[5:6], B=1)
    o1 = run_kernel(one)
    assert (host(o1["acc"]) == 0).all() and (host(o1["count"]) == ref["used"][:, 5]).all()


def test_refused_arguments():
    from texpose_amd import ops
    c = case("sphere", 64, 64, 200.0, 2)
    for bad in (dict(cos_min=0.0), dict(cos_min=1.5), dict(cover_min=0.0), dict(cover_min=float("nan")), dict(z_tol_mm=-1.0), dict(slope=-0.5)):
        with pytest.raises(_lib.TexposeLibraryError, match="tp_texture_bake"):
            run_kernel(c, **bad)
    lib = _lib.load()
    t = {k: cu(c[k]) for k in ("verts", "normals", "poses", "K", "rgb", "zbuf")}
    acc, count = torch.zeros(len(c["verts"]), 4, device=DEV), torch.zeros(len(c["verts"]), device=DEV, dtype=torch.int32)
    ws = ops.texture_bake_workspace(len(c["verts"]), 2, DEV)

    def call(**kw):
        a = _lib.TextureBakeArgs()
        a.verts, a.normals, a.pose, a.intr, a.rgb, a.zbuf = (t[k].data_ptr() for k in ("verts", "normals", "poses", "K", "rgb", "zbuf"))
        a.V, a.B, a.H, a.W, a.clear = len(c["verts"]), 2, 64, 64, 1
        a.cos_min, a.cover_min, a.z_tol_mm, a.slope = 0.3, 0.5, 0.5, 2.0
        a.acc, a.count, a.workspace = acc.data_ptr(), count.data_ptr(), ws.data_ptr()
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.tp_texture_bake(C.byref(a), None), lib.tp_last_error().decode()

    for kw in (dict(V=0), dict(B=0), dict(B=-3), dict(H=0), dict(W=-1), dict(H=65536, W=32768), dict(B=65536), dict(acc=None), dict(workspace=None)):
        rc, msg = call(**kw)
        assert rc == -1 and "tp_texture_bake" in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert (acc == 0).all() and (count == 0).all()                    # a refused call launches nothing
    with pytest.raises(ValueError):
        ops.texture_bake(t["verts"], t["normals"][:-1], t["poses"], t["K"], t["rgb"], t["zbuf"])
    with pytest.raises(ValueError):
        ops.texture_bake(t["verts"], t["normals"], t["poses"], t["K"], t["rgb"][:, :-1], t["zbuf"])
    with pytest.raises(ValueError):
        ops.texture_bake(t["verts"], t["normals"], t["poses"], t["K"], t["rgb"], t["zbuf"], clear=False)
    with pytest.raises(_lib.TexposeLibraryError):
        ops.texture_bake(t["verts"].cpu(), t["normals"], t["poses"], t["K"], t["rgb"], t["zbuf"])


def baker_for(c, chunks):
    baker = TB.TextureBaker(c["all_verts"], c["faces"], c["H"], c["W"], DEV)
    rgb, pose, K, zbuf = cu(c["rgb"]), cu(c["poses"]), cu(c["K"]), cu(c["zbuf"])
    for s in range(0, c["B"], chunks):
        baker.add_views(rgb[s:s + chunks], pose[s:s + chunks], K, zbuf=zbuf[s:s + chunks])
    torch.cuda.synchronize()
    return baker


def test_streaming_determinism_and_graph_replay():
    c = case("ripple", 64, 80, 200.0, 14)
    first, again = run_kernel(c), run_kernel(c)
    assert torch.equal(first["acc"], again["acc"]) and torch.equal(first["count"], again["count"])
    tol = colour_tol(64, 80)
    results = {}
    for chunks in (1, 5, 14):
        b1, b2 = baker_for(c, chunks), baker_for(c, chunks)
        assert torch.equal(b1.acc, b2.acc) and torch.equal(b1.count, b2.count)          # the same chunking twice: the same bits
        assert b1.views == 14
        results[chunks] = b1.result(fill=False)
    assert torch.equal(baker_for(c, 14).acc, first["acc"])           # one chunk into cleared accumulators: the kernel's own sums
    for chunks in (1, 5):
        assert torch.equal(results[chunks].count, results[14].count)
        d = (results[chunks].vcolor - results[14].vcolor).abs().max()
        print("chunks of %d against one call: max |dcolour| %.2e" % (chunks, float(d)))
        assert float(d) <= tol
    # add_views without zbuf rasterises the mesh itself; captured and replayed it equals the eager call bit for bit
    rgb, pose, K = cu(c["rgb"]), cu(c["poses"]), cu(c["K"])
    eager = TB.TextureBaker(c["all_verts"], c["faces"], 64, 80, DEV)
    eager.add_views(rgb, pose, K)
    torch.cuda.synchronize()
    assert torch.equal(eager.acc, first["acc"])                      # (the same depth planes as the case's)
    cap = TB.TextureBaker(c["all_verts"], c["faces"], 64, 80, DEV)
    cap.add_views(rgb, pose, K)                                      # warm-up: the workspace exists before the capture
    cap.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap.add_views(rgb, pose, K)
    for _ in range(2):
        cap.reset()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap.acc, eager.acc) and torch.equal(cap.count, eager.count)
    eager.reset()
    assert not eager.acc.any() and not eager.count.any() and eager.views == 0


def test_round_trip_through_the_rasteriser():
    from texpose_amd import ops
    verts, faces = REF.uv_sphere(12, 16)
    H = W = 64
    col = REF.test_colours(verts)
    poses, K = TB.sphere_view_poses(14, DIST).astype(np.float32), REF.pinhole(H, W, 200.0)
    r = ops.mesh_raster(cu(verts), cu(faces), cu(poses), cu(K), H=H, W=W, vcolor=cu(col), face_ids=False, normals=False)
    baker = TB.TextureBaker(verts, faces, H, W, DEV)
    baker.add_views(r["rgb"], cu(poses), cu(K), zbuf=r["zbuf"])
    res = baker.result(fill=True)
    assert bool(res.seen.all()) and res.filled == 0 and res.unseen == 0
    # the bar: the restatement's own round-trip error on the same inputs, plus the kernel-against-restatement tolerance
    ref = REF.bake(verts, TB.vertex_normals(verts, faces), poses, K, host(r["rgb"]), host(r["zbuf"]))
    vref, seen = REF.vcolor_of(ref["acc"])
    bar = np.abs(vref - col)[seen].max() + colour_tol(H, W)
    err = np.abs(host(res.vcolor) - col).max()
    print("device round trip: max error %.4f, bar %.4f" % (err, bar))
    assert seen.all() and bar <= 0.03 + colour_tol(H, W)
    assert err <= bar
    again = ops.mesh_raster(cu(verts), cu(faces), cu(poses), cu(K), H=H, W=W, vcolor=res.vcolor, face_ids=False, normals=False)
    assert torch.equal(again["zbuf"], r["zbuf"])
    m = r["zbuf"] > 0
    d = float((again["rgb"] - r["rgb"]).abs()[m].max())
    print("re-rendered against the original renders inside the mask: max error %.4f" % d)
    assert int(m.sum()) > 14 * 1500 and d <= bar


def test_bake_texture_tool(tmp_path):
    import oracle.texpose_oracle as O
    from texpose_amd import checkpoint as ck, ops
    from texpose_amd.graph import Graph
    from texpose_amd.options import default_options
    from texpose_amd.surfel import load_ply
    H, W, N = 48, 64, 8
    opt = default_options(H=H, W=W, device=DEV)
    opt.nerf.sample_intvs, opt.nerf.sample_stratified = N, False
    opt.arch.mlp_precision = "fp32"
    graph = Graph(opt).to(DEV)
    graph.nerf.load_state_dict({**graph.nerf.state_dict(), **{k: v.to(DEV) for k, v in O.make_params(3).items()}})
    graph.attach_latents(4, opt)
    torch.save(ck.make_checkpoint(graph, epoch=1, it=10), str(tmp_path / "model.ckpt"))
    verts, faces = REF.uv_sphere(12, 16)
    TB.write_ply(str(tmp_path / "sphere.ply"), verts, faces, np.zeros_like(verts))
    out, report = tmp_path / "textured.ply", tmp_path / "bake.json"
    cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "tools", "bake_texture.py"), "--checkpoint", str(tmp_path / "model.ckpt"),
           "--ply", "5=" + str(tmp_path / "sphere.ply"), "--sphere", "6", "--distance-mm", "400", "--focal", "150", "--H", str(H), "--W", str(W),
           "--samples", str(N), "--precision", "fp32", "--out", str(out), "--report", str(report), "--verify"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    print(p.stdout)
    v, f, c = load_ply(str(out))
    assert (v == verts).all() and (f == faces).all() and c is not None and c.shape == (len(verts), 3)
    rep = json.loads(report.read_text())
    assert rep["coverage"] == 1.0 and rep["vertices"] == len(verts) and rep["views"] == 6 and rep["unseen"] == 0
    assert rep["mean_views_per_vertex"] >= 1.0 and "PSNR" in p.stdout and rep["verify"]["pixels"] > 0
    r = ops.mesh_raster(cu(v), cu(f), cu(TB.sphere_view_poses(2, 400.0).astype(np.float32)), cu(REF.pinhole(H, W, 150.0)), H=H, W=W, vcolor=cu(c),
                        face_ids=False, normals=False)
    assert bool(torch.isfinite(r["rgb"]).all()) and int((r["zbuf"] > 0).sum()) > 500
    ops.check_mlp_status(torch.device(DEV))
