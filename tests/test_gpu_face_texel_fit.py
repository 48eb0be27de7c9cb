"""GPU: K36 tp_face_texel_shade_bwd (ops.face_texel_shade_bwd, autograd_ops.face_texel_shade, face_texels.shade_nodes) against the fp64
restatement of its contract in tests/face_texel_fit_ref.py on the face planes of ops.mesh_raster, within the fixed-point bound of the
header; its edges, refusals, determinism and capture; FaceTexelFitter against the restated loop's recorded figures; the bake tool."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import face_texel_fit_ref as FIT
import face_texels_ref as REF
import test_gpu_face_texels as K35G                     # its meshes, sizes and cached face planes, as they are
import texture_bake_ref as TREF
from texpose_amd import _lib
from texpose_amd import face_texels as FT
from texpose_amd import texture_bake as TB

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
cu, host, planes = K35G.cu, K35G.host, K35G.planes
_sub = {}


def node_index_of(mesh, R):
    if (mesh, R) not in _sub:
        verts, faces = K35G.MESHES[mesh]()
        ni = FT.subdivide(verts, faces, R)[2]
        _sub[mesh, R] = (ni, int(ni.max()) + 1)
    return _sub[mesh, R]


def bwd(c, g, R, node_index=None, U=None, face=None, **kw):
    from texpose_amd import ops
    v, f, p, k = (cu(kw.pop(n, c[n])) for n in ("verts", "faces", "poses", "K"))
    if node_index is not None:
        kw.update(node_index=cu(node_index), U=U)
    out = ops.face_texel_shade_bwd(cu(c["face"] if face is None else face, torch.int32), v, f, g if torch.is_tensor(g) else cu(g), p, k, R=R, **kw)
    torch.cuda.synchronize()
    return out


def ref_args(c, g, R, node_index=None, U=None, face=None, **kw):
    return (c["face"] if face is None else face, kw.get("verts", c["verts"]), kw.get("faces", c["faces"]), g, kw.get("poses", c["poses"]), c["K"],
            c["H"], c["W"], R) + (() if node_index is None else (node_index, U))


def within_bound(got, got_w, want):
    """every destination within n_d gmax 2^-37 + ulp32(|want|) (the coverage: n_d 2^-37 + ulp32) -> the largest error over its bound"""
    n = want["count"].astype(np.float64)
    tol = n[:, None] * want["gmax"] * 2.0 ** -37 + np.spacing(np.abs(want["grad"]).astype(np.float32))
    d = np.abs(host(got).reshape(-1, 3).astype(np.float64) - want["grad"])
    worst = float((d / tol).max())
    assert (d <= tol).all(), worst
    if got_w is not None:
        tol_w = n * 2.0 ** -37 + np.spacing(want["weight"].astype(np.float32))
        dw = np.abs(host(got_w).reshape(-1).astype(np.float64) - want["weight"])
        assert (dw <= tol_w).all(), float((dw / tol_w).max())
    return worst


@pytest.mark.parametrize("size", list(K35G.SIZES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mesh", list(K35G.MESHES))
def test_kernel_against_the_restatement(mesh, size):
    H, W = size
    rs = np.random.RandomState(5)
    for B in (1, 3):
        c = planes(mesh, H, W, B)
        g = rs.randn(B, H, W, 3).astype(np.float32)
        for R in (1, 2, 3, 8, 64):
            for per_node in (False, True):
                idx = node_index_of(mesh, R) if per_node else ()
                want = FIT.shade_bwd(*ref_args(c, g, R, *idx))
                fixed = FIT.shade_bwd_fixed(*ref_args(c, g, R, *idx))
                grad, weight = bwd(c, g, R, *idx, weight=True)
                alone = bwd(c, g, R, *idx)
                assert grad.shape == ((idx[1], 3) if per_node else (len(c["faces"]), FT.texel_count(R), 3)) and weight.shape == grad.shape[:-1]
                assert torch.equal(alone.view(torch.int32), grad.view(torch.int32))          # the coverage output changes nothing
                worst = within_bound(grad, weight, want)
                same = int((host(grad).reshape(-1, 3) == fixed["grad"]).all(-1).sum())
                print("%s %dx%d B=%d R=%d %s: worst error / bound %.3f; %d of %d destinations equal the int64 emulation bit for bit (%d touched)"
                      % (mesh, H, W, B, R, "node" if per_node else "slot", worst, same, len(fixed["grad"]), int((want["count"] > 0).sum())))
                assert (want["count"] > 0).sum() >= 3 and (host(grad).reshape(-1, 3)[want["count"] == 0] == 0).all()


def test_adjoint_identity_on_the_device():
    """<shade(t), g> against <t, bwd(g)>, both summed in fp64 on the host, within the two kernels' bounds: the forward's 1e-6 per value
    (tests/test_gpu_face_texels.py) times |g|, the adjoint's bound times |t|"""
    rs = np.random.RandomState(6)
    for mesh, R in (("sphere", 3), ("torus", 8)):
        c = planes(mesh, 64, 80, 3)
        t = rs.rand(len(c["faces"]), FT.texel_count(R), 3).astype(np.float32)
        g = rs.randn(3, 64, 80, 3).astype(np.float32)
        shaded = host(K35G.shade(c, t)).astype(np.float64)
        grad = host(bwd(c, g, R)).astype(np.float64)
        want = FIT.shade_bwd(*ref_args(c, g, R))
        bound_bwd = want["count"][:, None] * want["gmax"] * 2.0 ** -37 + np.spacing(np.abs(want["grad"]).astype(np.float32))
        tol = 1e-6 * np.abs(g.astype(np.float64)).sum() + (bound_bwd * t.reshape(-1, 3)).sum()
        lhs, rhs = (shaded * g).sum(), (t.astype(np.float64) * grad).sum()
        print("%s R=%d: <S t, g> = %.9g, <t, S^T g> = %.9g, difference %.3g (tolerance %.3g)" % (mesh, R, lhs, rhs, abs(lhs - rhs), tol))
        assert abs(lhs - rhs) <= tol and abs(lhs) > 1.0


def exact_triangle():
    R, H, W = 8, 24, 24
    return dict(verts=np.array([[0, 0, 0], [16, 0, 0], [0, 16, 0]], dtype=np.float32), faces=np.array([[0, 1, 2]], dtype=np.int32),
                poses=np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 64.0]]], dtype=np.float32),
                K=np.array([[64.0, 0, 4.5], [0, 64.0, 4.5], [0, 0, 1]], dtype=np.float32), face=np.zeros((1, H, W), dtype=np.int32), H=H, W=W, B=1), R


def test_exact_case():
    """the fronto-parallel triangle of K35's test_exact_nodes: a gradient of k / 256 at the pixel centre of node n alone comes back as
    grad[n] bit for bit (the weight there is exactly 1 and every product a small dyadic number)"""
    c, R = exact_triangle()
    T = FT.texel_count(R)
    g = np.zeros((1, c["H"], c["W"], 3), dtype=np.float32)
    values = ((np.arange(3 * T).reshape(T, 3) * 7) % 255 + 1).astype(np.float32) / 256.0
    for n, (i, j) in enumerate(REF.node_list(R)):
        g[0, 4 + 2 * j, 4 + 2 * i] = values[n]
    grad, weight = bwd(c, g, R, weight=True)
    assert (host(grad)[0] == values).all()
    want = FIT.shade_bwd(*ref_args(c, g, R))
    within_bound(grad, weight, want)
    assert (host(weight) >= 1).all()


def test_contention_three_texels():
    c = planes("triangle", 64, 80, 3)
    g = np.random.RandomState(8).randn(3, 64, 80, 3).astype(np.float32)
    first, w1 = bwd(c, g, 1, weight=True)
    again, w2 = bwd(c, g, 1, weight=True)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32)) and torch.equal(w1.view(torch.int32), w2.view(torch.int32))
    want = FIT.shade_bwd(*ref_args(c, g, 1))
    assert want["count"].tolist() == [15360] * 3
    within_bound(first, w1, want)


# ---- the raw entry point on guarded buffers
def guarded(nbytes):
    """nbytes inside a buffer with guard bands of 16 KiB on both sides, all 0xAB bytes -> the buffer, the inner view (uint8)"""
    g = 16384
    buf = torch.empty(nbytes + 2 * g, device=DEV, dtype=torch.uint8)
    buf.fill_(0xAB)
    return buf, buf[g:g + nbytes]


def guards_intact(buf):
    return bool((buf[:16384] == 0xAB).all()) and bool((buf[-16384:] == 0xAB).all())


class Raw:
    """tp_face_texel_shade_bwd through ctypes with its outputs and its workspace inside guard bands"""

    def __init__(self, c, R, node_index=None, U=None, weight=True):
        self.c, self.R, self.lib = c, R, _lib.load()
        self.t = dict(verts=cu(c["verts"]), faces=cu(c["faces"]), pose=cu(c["poses"]), intr=cu(np.broadcast_to(c["K"], (c["B"], 3, 3)).copy()))
        self.node_index, self.U = (None, 0) if node_index is None else (cu(node_index, torch.int32), U)
        self.N = len(c["faces"]) * FT.texel_count(R) if node_index is None else U
        self.want_weight = weight
        self.bufs = {}

    def __call__(self, plane, g, /, **change):
        c = self.c
        face, g = cu(plane, torch.int32), cu(g, torch.float32)
        ws_bytes = int(self.lib.tp_face_texel_shade_bwd_workspace(self.N, int(self.want_weight)))
        self.bufs = dict(grad=guarded(12 * self.N), weight=guarded(4 * self.N), workspace=guarded(ws_bytes))
        a = _lib.FaceTexelShadeBwdArgs()
        for k, v in self.t.items():
            setattr(a, k, v.data_ptr())
        a.face, a.grad_rgb, a.node_index = face.data_ptr(), g.data_ptr(), None if self.node_index is None else self.node_index.data_ptr()
        a.B, a.H, a.W, a.V, a.F, a.R, a.U = c["B"], c["H"], c["W"], len(c["verts"]), len(c["faces"]), self.R, self.U
        a.workspace, a.grad = self.bufs["workspace"][1].data_ptr(), self.bufs["grad"][1].data_ptr()
        a.weight = self.bufs["weight"][1].data_ptr() if self.want_weight else None
        for k, v in change.items():
            setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
        rc = self.lib.tp_face_texel_shade_bwd(C.byref(a), None)
        msg = self.lib.tp_last_error().decode()
        torch.cuda.synchronize()
        return rc, msg

    @property
    def grad(self):
        return self.bufs["grad"][1].view(torch.float32).view(self.N, 3)

    @property
    def weight(self):
        return self.bufs["weight"][1].view(torch.float32)

    def intact(self):
        return all(guards_intact(b[0]) for b in self.bufs.values())

    def untouched(self):
        return all(bool((b[0] == 0xAB).all()) for b in self.bufs.values())


def test_edges_contribute_nothing_and_write_nothing_else():
    H, W, B, R = 37, 53, 3, 8
    c = planes("sphere", H, W, B)
    F = len(c["faces"])
    g = np.random.RandomState(9).randn(B, H, W, 3).astype(np.float32)
    full = np.zeros((B, H, W), dtype=np.int32)                       # a hand-made plane: every pixel claims a face
    full[:] = (np.arange(H * W).reshape(H, W) % F)[None]
    raw = Raw(c, R)

    def check(face, g, idx=(), **kw):
        ref = {k: v for k, v in kw.items() if k in ("faces", "poses")}
        dev = {dict(faces="faces", poses="pose")[k]: cu(v) for k, v in ref.items()}
        rc, msg = raw(face, g, **dev)
        assert rc == 0, msg
        assert raw.intact()
        want = FIT.shade_bwd(*ref_args(c, g, R, *idx, face=face, **ref))
        within_bound(raw.grad, raw.weight, want)
        assert bool(torch.isfinite(raw.grad).all())
        return want

    # the plane's own values, and a hand-made plane holding -1, -5, F and 2^30 beside valid entries
    assert check(c["face"], g)["count"].sum() == 3 * (c["face"] >= 0).sum()
    plane, bad = full.copy(), np.zeros((B, H, W), dtype=bool)
    for k, value in enumerate((-1, -5, F, 1 << 30)):
        bad[:, :, k::7] = True
        plane[:, :, k::7] = value
    assert check(plane, g)["count"].sum() == 3 * (~bad).sum()
    # an all-background plane: zeros
    assert check(np.full_like(full, -1), g)["count"].sum() == 0 and bool((raw.grad == 0).all()) and bool((raw.weight == 0).all())
    # NaN, Inf and behind-camera poses under the full plane: nothing contributes
    poses = c["poses"].copy()
    poses[0, 1, 2] = np.nan
    poses[1, :, 3] = [np.inf, 0.0, 400.0]
    poses[2, 2, 3] = -400.0
    assert check(full, g, poses=poses)["count"].sum() == 0 and bool((raw.grad == 0).all()) and bool((raw.weight == 0).all())
    # faces with an out-of-range vertex contribute nothing, the rest as before
    faces = c["faces"].copy()
    faces[::3, 1] = len(c["verts"])
    faces[1::3, 2] = -1
    assert check(full, g, faces=faces)["count"].sum() == 3 * (np.arange(F) % 3 == 2)[full].sum()
    # NaN / Inf in grad_rgb drop that pixel only (from the coverage too)
    gb = g.copy()
    gb[0, ::3, ::2, 1] = np.nan
    gb[1, 1::3, ::2, 2] = np.inf
    gb[2, 2::3, 1::2, 0] = -np.inf
    dropped = check(c["face"], gb)
    assert dropped["count"].sum() == 3 * ((c["face"] >= 0) & np.isfinite(gb).all(-1)).sum() > 0
    # node_index entries of -1 and U are skipped
    ni, U = node_index_of("sphere", R)
    holes = ni.copy()
    holes[::2, ::5] = -1
    holes[1::2, 1::5] = U
    raw = Raw(c, R, holes, U)
    want = check(c["face"], g, (holes, U))
    assert 0 < want["count"].sum() < 3 * (c["face"] >= 0).sum()
    # without the coverage output its buffer stays as it was
    raw = Raw(c, R, weight=False)
    assert raw(c["face"], g)[0] == 0 and raw.intact() and bool((raw.bufs["weight"][0] == 0xAB).all())
    within_bound(raw.grad, None, FIT.shade_bwd(*ref_args(c, g, R)))


def test_refused_arguments_launch_nothing():
    from texpose_amd import ops
    c = planes("sphere", 37, 53, 1)
    F, V = len(c["faces"]), len(c["verts"])
    g = np.ones((1, 37, 53, 3), dtype=np.float32)
    raw = Raw(c, 2)
    ni = cu(node_index_of("sphere", 2)[0], torch.int32)
    for kw in (dict(B=0), dict(H=-1), dict(W=0), dict(V=0), dict(F=0), dict(R=0), dict(R=65), dict(H=65536, W=32768), dict(F=1 << 30, R=8),
               dict(B=1 << 30, H=64, W=64), dict(B=3, H=4096, W=4096), dict(node_index=ni, U=0), dict(node_index=ni, U=-1), dict(F=300000000, R=1),
               dict(node_index=ni, U=715827883), dict(workspace=None), dict(grad_rgb=None), dict(grad=None), dict(face=None), dict(verts=None)):
        rc, msg = raw(c["face"], g, **kw)
        assert rc == -1 and "tp_face_texel_shade_bwd" in msg, (kw, rc, msg)
        assert raw.untouched(), kw                                    # a refused call launches nothing
    rc, msg = raw(c["face"], g, workspace=raw.bufs["workspace"][1].data_ptr() + 4)       # (the buffers of the previous call: misaligned)
    assert rc == -1 and "workspace" in msg
    assert raw(c["face"], g)[0] == 0 and raw.intact() and bool(torch.isfinite(raw.grad).all())
    args = dict(face=cu(c["face"]), verts=cu(c["verts"]), faces=cu(c["faces"]), grad_rgb=cu(g), pose=cu(c["poses"]), intr=cu(c["K"]))
    call = lambda R=2, **kw: ops.face_texel_shade_bwd(*[kw.pop(k, args[k]) for k in ("face", "verts", "faces", "grad_rgb", "pose", "intr")], R=R, **kw)
    assert call().shape == (F, 6, 3)
    for kw in (dict(face=args["face"].float()), dict(grad_rgb=args["grad_rgb"][..., :2]), dict(grad_rgb=args["grad_rgb"].long()), dict(R=0), dict(R=65),
               dict(node_index=ni), dict(node_index=ni, U=0), dict(node_index=ni[:, :5], U=10), dict(node_index=ni.float(), U=10), dict(U=10),
               dict(out=torch.empty(F, 6, 4, device=DEV)), dict(out=torch.empty(F, 6, 3, device=DEV, dtype=torch.float64)), dict(pose=args["pose"][:, :2]),
               dict(faces=args["faces"][:, :2])):
        with pytest.raises(ValueError):
            call(**kw)


def test_determinism_and_graph_replay():
    from texpose_amd import ops
    H, W, B, R = 64, 80, 3, 8
    c = planes("torus", H, W, B)
    v, f, p, k, face = cu(c["verts"]), cu(c["faces"]), cu(c["poses"]), cu(c["K"][None].repeat(B, 0)), cu(c["face"])
    ni, U = node_index_of("torus", R)
    ni = cu(ni, torch.int32)
    base = torch.randn(B, H, W, 3, device=DEV)
    g = base.clone()
    eager = {}
    for scale in (1.0, 3e-5, 7e4):
        g.copy_(base * scale)
        first = ops.face_texel_shade_bwd(face, v, f, g, p, k, R=R, node_index=ni, U=U, weight=True)
        again = ops.face_texel_shade_bwd(face, v, f, g, p, k, R=R, node_index=ni, U=U, weight=True)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))
        eager[scale] = first
    assert not torch.equal(eager[1.0][0], eager[7e4][0]) and torch.equal(eager[1.0][1], eager[7e4][1])
    cap = torch.empty(U, 3, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, cap_w = ops.face_texel_shade_bwd(face, v, f, g, p, k, R=R, node_index=ni, U=U, weight=True, out=cap)
    for scale in (1.0, 3e-5, 7e4, 1.0):                              # the gradient's scale is read on the device at every replay
        g.copy_(base * scale)
        cap.view(torch.uint8).fill_(0xAB)
        cap_w.view(torch.uint8).fill_(0xAB)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap.view(torch.int32), eager[scale][0].view(torch.int32)) and torch.equal(cap_w.view(torch.int32), eager[scale][1].view(torch.int32))


def test_autograd_routes():
    from texpose_amd import autograd_ops, ops
    H, W, B, R = 37, 53, 3, 3
    c = planes("sphere", H, W, B)
    v, f, p, k, face = cu(c["verts"]), cu(c["faces"]), cu(c["poses"]), cu(c["K"]), cu(c["face"])
    g = torch.randn(B, H, W, 3, device=DEV)
    texels = torch.rand(len(c["faces"]), FT.texel_count(R), 3, device=DEV, requires_grad=True)
    rgb = autograd_ops.face_texel_shade(face, v, f, texels, p, k)
    assert torch.equal(rgb.detach(), ops.face_texel_shade(face, v, f, texels, p, k))
    (rgb * g).sum().backward()
    per_slot = ops.face_texel_shade_bwd(face, v, f, g, p, k, R=R)
    assert torch.equal(texels.grad.view(torch.int32), per_slot.view(torch.int32))
    assert not ops.face_texel_shade(face, v, f, texels, p, k).requires_grad          # the plain op keeps its contract
    ni, U = node_index_of("sphere", R)
    nodes = torch.rand(U, 3, device=DEV, requires_grad=True)
    rgb = FT.shade_nodes(face, v, f, nodes, ni, p, k)
    assert torch.equal(rgb.detach(), ops.face_texel_shade(face, v, f, nodes.detach()[cu(ni)], p, k))
    (rgb * g).sum().backward()
    per_node = ops.face_texel_shade_bwd(face, v, f, g, p, k, R=R, node_index=cu(ni), U=U)
    assert torch.equal(nodes.grad.view(torch.int32), per_node.view(torch.int32))
    # the per-slot gradient summed over each node's slots in fp64 on the host, within the two calls' bounds
    summed = np.zeros((U, 3))
    np.add.at(summed, ni.reshape(-1), host(per_slot).reshape(-1, 3).astype(np.float64))
    want = FIT.shade_bwd(*ref_args(c, host(g), R, ni, U))
    slot = FIT.shade_bwd(*ref_args(c, host(g), R))
    slot_tol = np.zeros((U, 3))
    np.add.at(slot_tol, ni.reshape(-1), slot["count"][:, None] * slot["gmax"] * 2.0 ** -37 + np.spacing(np.abs(slot["grad"]).astype(np.float32)))
    tol = want["count"][:, None] * want["gmax"] * 2.0 ** -37 + np.spacing(np.abs(want["grad"]).astype(np.float32)) + slot_tol
    assert (np.abs(host(nodes.grad).astype(np.float64) - summed) <= tol).all() and np.abs(summed).max() > 0


def test_fitter_recovers_a_consistent_system():
    """photographs rendered by ops.face_texel_shade from random node colours x*: the bar is 4 x the restated loop's recorded error + 1e-4
    (fp32 vectors against fp64: FIT.CONSISTENT_ERROR_FP32, measured on the CPU, lies below it)"""
    from texpose_amd import ops
    import test_face_texel_fit_cpu as CPU
    c = CPU.consistent_system()
    size, R, U = c["size"], c["R"], c["U"]
    fitter = FT.FaceTexelFitter(c["verts"], c["faces"], R, size, size, DEV, lam=1e-6, iters=32)
    v, f, p, k = cu(c["verts"]), cu(c["faces"]), cu(c["poses"]), cu(c["K"])
    face = ops.mesh_raster(v, f, p, k, H=size, W=size, normals=False)["face"]
    truth = cu(c["truth"].astype(np.float32))
    photo = ops.face_texel_shade(face, v, f, truth[cu(c["node_index"])], p, k)
    fitter.add_views(photo[:5], c["poses"][:5], c["K"], face=face[:5], weight=(face[:5] >= 0).float())
    fitter.add_views(photo[5:], c["poses"][5:], c["K"], weight=(face[5:] >= 0).float())           # (rasterised by the fitter: the same plane)
    assert fitter.views == 14
    res = fitter.fit(prior=None, start=torch.zeros(U, 3, device=DEV))
    seen = res.coverage >= 1
    err = float((res.nodes - truth).abs()[seen].max())
    rms = host(res.rms).astype(np.float64)
    print("consistent system on the device: max |x - x*| %.3e on %d of %d nodes (CPU loop fp64 %.3e, fp32 %.3e); rms %.3e -> %.3e"
          % (err, int(seen.sum()), U, FIT.CONSISTENT_ERROR, FIT.CONSISTENT_ERROR_FP32, rms[0], rms[-1]))
    assert int(seen.sum()) >= 0.9 * U and err <= 4 * FIT.CONSISTENT_ERROR + 1e-4
    assert rms.shape == (33,) and (rms[2:] <= rms[1:-1] + 1e-6).all() and rms[-1] < 1e-3 * rms[0]
    assert res.texels.shape == (len(c["faces"]), FT.texel_count(R), 3) and torch.equal(res.texels, res.nodes[cu(c["node_index"])])
    again = fitter.fit(prior=None, start=torch.zeros(U, 3, device=DEV))
    assert torch.equal(again.nodes.view(torch.int32), res.nodes.view(torch.int32))               # a fit is bit-identical from run to run


def test_fitter_against_the_bake():
    """the bake round trip shrunk to 64 x 64, f = 200, R = 4: FaceTexelBaker, then the fit from the bake, against the restated loop's
    figures for this case (FIT.ROUND_TRIP_SMALL)"""
    from texpose_amd import ops
    import test_face_texel_fit_cpu as CPU
    size, R = 64, 4
    c, _ = CPU.round_trip(R, size, 200.0)
    psnr_bake_cpu, psnr_fit_cpu, _, rms_fit_cpu = FIT.ROUND_TRIP_SMALL[R]
    baker = FT.FaceTexelBaker(c["verts"], c["faces"], R, size, size, DEV)
    baker.add_views(cu(c["rgb"]), cu(c["poses"]), cu(c["K"]))
    bake = baker.result(fill=True)
    fitter = FT.FaceTexelFitter(c["verts"], c["faces"], R, size, size, DEV)                    # lam = 0.1, 4 iterations
    fitter.add_views(cu(c["rgb"]), c["poses"], c["K"])
    res = fitter.fit(prior=bake.vcolor_sub, start=bake.vcolor_sub)
    rms = host(res.rms)
    hrgb, _, hface = c["target"]
    held = ops.mesh_raster(cu(c["verts"]), cu(c["faces"]), cu(c["held"][None]), cu(c["K"]), H=size, W=size, normals=False)
    covered = (host(held["face"])[0] >= 0) & (hface >= 0)
    through = lambda texels: FIT.psnr(host(ops.face_texel_shade(held["face"], cu(c["verts"]), cu(c["faces"]), texels, cu(c["held"][None]), cu(c["K"])))[0], hrgb, covered)
    psnr_bake, psnr_fit = through(bake.texels), through(res.texels)
    print("fit against the bake %dx%d R=%d: training rms %.5f -> %.5f (CPU loop %.5f); held-out PSNR bake %.2f dB, fit %.2f dB (CPU %.2f, %.2f) over %d pixels; %d nodes on the prior"
          % (size, size, R, rms[0], rms[-1], rms_fit_cpu, psnr_bake, psnr_fit, psnr_bake_cpu, psnr_fit_cpu, covered.sum(), res.on_prior))
    assert rms[-1] <= rms_fit_cpu * 1.02 + 1e-5
    assert psnr_fit >= psnr_bake and psnr_fit >= psnr_fit_cpu - 1.0
    assert res.nodes.shape == bake.vcolor_sub.shape and isinstance(res.on_prior, int)


def test_tool_bake_with_fit(tmp_path):
    """bake_texture --texel-res 4 --fit 3 --verify on the random-weight checkpoint of K35's tool test: files, shapes and the report;
    the same command without --fit writes what FaceTexelBaker gives"""
    import oracle.texpose_oracle as O
    from texpose_amd import checkpoint as ck
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
    run = {}
    for name, extra in (("fit", ["--fit", "3"]), ("plain", [])):
        out, report = tmp_path / (name + ".ply"), tmp_path / (name + ".json")
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "tools", "bake_texture.py"), "--checkpoint", str(tmp_path / "model.ckpt"),
               "--ply", "%d=%s" % (oid, tmp_path / "sphere.ply"), "--sphere", "6", "--distance-mm", "400", "--focal", "150", "--H", str(H), "--W", str(W),
               "--samples", str(N), "--precision", "fp32", "--out", str(out), "--report", str(report), "--verify", "--texel-res", "4"] + extra
        p = subprocess.run(cmd, capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        texels, R = FT.load_texels(str(tmp_path / (name + ".texels.npz")), faces)
        assert R == 4 and texels.shape == (len(faces), 15, 3) and np.isfinite(texels).all() and texels.min() >= 0 and texels.max() <= 1
        run[name] = dict(texels=texels, report=json.loads(report.read_text()), stdout=p.stdout, ply=load_ply(str(out)))
    fit = run["fit"]["report"]["fit"]
    print(run["fit"]["stdout"])
    assert fit["iters"] == 3 and fit["lam"] == 0.1 and fit["rms_after"] <= fit["rms_before"] and fit["on_prior"] >= 0
    assert run["fit"]["report"]["verify"]["psnr_db_baked"] is not None and run["fit"]["stdout"].count("PSNR") >= 2
    corner = run["fit"]["texels"][:, [0, 4, 14]]                       # the PLY's vertex colours are the fitted corner nodes at 8 bits
    assert np.abs(corner - run["fit"]["ply"][2][faces]).max() <= 0.5 / 255 + 1e-6
    assert "fit" not in run["plain"]["report"] and not np.array_equal(run["plain"]["texels"], run["fit"]["texels"])
    # without --fit: today's route.  The tool's views in-process: the same renders baked by FaceTexelBaker give the same file
    assert run["plain"]["report"]["texels"]["R"] == 4 and "psnr_db_baked" not in run["plain"]["report"]["verify"]
    from texpose_amd import ops
    from texpose_amd.scene_bounds import SceneBounds
    from texpose_amd.surfel import SurfelRenderer
    scale = float(opt.nerf.depth.scale)
    pose = TB.poses_to_nerf_units(torch.from_numpy(TB.sphere_view_poses(6, 400.0)), scale).float().contiguous().to(DEV)
    intr = torch.tensor([[150.0, 0.0, W / 2.0], [0.0, 150.0, H / 2.0], [0.0, 0.0, 1.0]], device=DEV)[None].expand(6, 3, 3).contiguous()
    bounds = SceneBounds({oid: (SurfelRenderer(verts, faces, None, H, W, DEV), verts.min(axis=0), verts.max(axis=0))}, H, W, scale,
                         tuple(float(v) * scale for v in opt.nerf.depth.range))
    baker = FT.FaceTexelBaker(verts, faces, 4, H, W, DEV)
    with torch.no_grad():
        sb = bounds(pose, intr, opt.nerf.depth.range_source)
        rgb, weight = torch.empty(6, H, W, 3, device=DEV), torch.empty(6, H, W, device=DEV)
        for i in range(6):
            ret = graph.render_by_slices(opt, pose[i:i + 1], intr=intr[i:i + 1], depth_range=(sb.depth_range[0][i:i + 1], sb.depth_range[1][i:i + 1]),
                                         object_mask=sb.object_mask[i:i + 1], sample_idx=torch.tensor(0, device=DEV), mode="eval")
            rgb[i], weight[i] = ret.rgb_static.view(H, W, 3), ret.opacity_static.view(H, W)
        baker.nodes.add_views(rgb, TB.poses_to_mm(pose, scale), intr, zbuf=sb.zbuf[0], weight=weight)
    assert np.array_equal(host(baker.result(fill=True).texels), run["plain"]["texels"])
    ops.check_mlp_status(torch.device(DEV))
