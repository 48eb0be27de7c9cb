"""K41 (tp_face_texel_light) and FaceTexelFitter(lighting=True) on the device against tests/face_texel_light_ref.py: the call bit for bit,
its two device routes, memory and replay, refusals, and the lit fit against the restated loop's recorded figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import face_texel_light_ref as LT
import photo_lighting_ref as LREF
import texture_bake_ref as TREF
from gn_ref import cu, host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 16384
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31


def bits(t):
    return t.contiguous().view(torch.uint8) if torch.is_tensor(t) else np.ascontiguousarray(t).view(np.uint8)


def same_bits(a, b):
    a, b = (host(x) if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- one call, exact inputs
def call_case(seed, mesh, B, H, W, clean=False):
    """Planes taken as they are (no rasteriser): a face plane uniform over the mesh's faces with -1, F, F + 1, INT_MAX and INT_MIN
    planted, faces with an index >= V or < 0, random poses about 900 mm away, a random light per image, colour and image in [0, 1] with 2 %
    NaN / +-Inf, weights in (0.1, 2) with 0, negatives and NaN.  ``clean``: finite planes, every face index good."""
    rs = np.random.RandomState(seed)
    verts, faces = LREF.bumpy_mesh(seed) if mesh == "bumpy" else TREF.uv_sphere(12, 16)
    verts, faces = np.asarray(verts, np.float32), np.array(faces, np.int32)
    V, F = len(verts), len(faces)
    face = rs.randint(0, F, (B, H, W)).astype(np.int32)
    colour, image = rs.rand(B, H, W, 3).astype(np.float32), rs.rand(B, H, W, 3).astype(np.float32)
    weight = rs.uniform(0.1, 2.0, (B, H, W)).astype(np.float32)
    if not clean:
        faces[rs.randint(0, F, 4), rs.randint(0, 3, 4)] = [V, -1, V + 7, INT_MIN]
        where = rs.rand(B, H, W)
        for k, v in enumerate([-1, F, F + 1, INT_MAX, INT_MIN]):
            face[(where >= 0.04 * k) & (where < 0.04 * (k + 1))] = v
        for plane in (colour, image):
            u = rs.rand(*plane.shape)
            plane[u < 0.007], plane[(u >= 0.007) & (u < 0.014)], plane[(u >= 0.014) & (u < 0.02)] = np.nan, np.inf, -np.inf
        u = rs.rand(B, H, W)
        weight[u < 0.03], weight[(u >= 0.03) & (u < 0.06)], weight[(u >= 0.06) & (u < 0.09)] = 0.0, -0.5, np.nan
    pose = np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        pose[b] = np.concatenate([q, rs.uniform(-15, 15, (3, 1)) + [[0.0], [0.0], [900.0]]], 1)
    amb = rs.uniform(0.6, 1.4, (B, 3))
    d = rs.normal(size=(B, 3, 3))
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * rs.uniform(0.1, 0.5, (B, 3, 1)) * amb[..., None]
    light = np.concatenate([amb[..., None], d, rs.uniform(-0.1, 0.1, (B, 3, 1))], -1).astype(np.float32)
    return dict(verts=verts, faces=faces, face=face, colour=colour, image=image, weight=weight, pose=pose, light=light)


def gpu_call(c, image=True, weight=True, **kw):
    from texpose_amd import ops
    return ops.face_texel_light(cu(c["face"]), cu(c["verts"]), cu(c["faces"]), cu(c["colour"]), cu(c["pose"]), cu(c["light"]),
                                image=cu(c["image"]) if image else None, weight=cu(c["weight"]) if weight else None, **kw)


def ref_call(c, image=True, weight=True):
    return LT.light_ref(c["verts"], c["faces"], c["face"], c["pose"], c["light"], c["colour"], c["image"] if image else None,
                        c["weight"] if weight else None)


def compare(got, want):
    assert same_bits(got["grad"], want["grad"])
    if "diag" in got:
        assert same_bits(got["diag"], want["diag"])
    if "sums" in got:
        s = host(got["sums"])
        assert s.dtype == np.float64 and (np.abs(s - want["sums"]) <= 1e-12 * np.abs(want["sums"])).all(), (s, want["sums"])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 7), (33, 257), (64, 80)])
@pytest.mark.parametrize("mesh", ["bumpy", "sphere"])
def test_call_equals_the_restatement(mesh, H, W, B):
    """64 x 80 takes the vector path, the others (H W no multiple of four) the guarded one; 33 x 257 spans nine tiles with a partial last
    one; both modes, with and without weight, diag and sums."""
    c = call_case(1000 * H + 10 * W + B, mesh, B, H, W)
    on = 0
    for image in (True, False):
        for weight in (True, False):
            want = ref_call(c, image, weight)
            on += int(want["on"].sum())
            for diag in (False, True):
                for sums in ((False, True) if image else (False,)):
                    got = gpu_call(c, image, weight, diag=diag, sums=sums)
                    assert set(got) == {"grad"} | ({"diag"} if diag else set()) | ({"sums"} if sums else set())
                    compare(got, want)
    torch.cuda.synchronize()                                         # the calls ended clean
    if H * W >= 33 * 257:
        assert on > 0.5 * 4 * B * H * W and np.abs(want["grad"]).max() > 0


def test_misaligned_planes_take_the_guarded_path():
    """colour, then face, as a view 4 bytes into its storage: 16 x 16 would take the vector path."""
    from texpose_amd import ops
    c = call_case(7, "bumpy", 2, 16, 16)
    d = {k: cu(v) for k, v in c.items()}
    call = lambda d: ops.face_texel_light(d["face"], d["verts"], d["faces"], d["colour"], d["pose"], d["light"], image=d["image"], weight=d["weight"],
                                          diag=True, sums=True)
    aligned = call(d)
    compare(aligned, ref_call(c))
    for off in ("colour", "face"):
        e = dict(d)
        store = torch.empty(d[off].numel() + 1, device=DEV, dtype=d[off].dtype)
        view = store[1:].view(d[off].shape)
        view.copy_(d[off])
        e[off] = view
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        got = call(e)
        for k in aligned:
            assert same_bits(got[k], aligned[k]), (off, k)


# ----------------------------------------------------------------------------- two device routes
def test_residual_mode_is_the_shading_times_the_applied_residual():
    """grad of the residual mode without weight = s (I - P) bit for bit, P ops.photo_lighting's applied rendering under the same light (a
    fit that keeps nothing returns the incoming light and applies it), s its apply of an all-ones rendering with the bias zeroed; under
    the identity light the two modes are m (I - c) and m c exactly."""
    from texpose_amd import ops
    B, H, W = 3, 33, 257
    c = call_case(11, "bumpy", B, H, W, clean=True)
    c["face"][:, :, ::5] = -1
    d = {k: cu(v) for k, v in c.items()}
    F = len(c["faces"])
    covered = (d["face"] >= 0) & (d["face"] < F)
    zbuf = torch.where(covered, 1.0, -1.0).float()
    nothing = torch.zeros(B, H, W, dtype=torch.uint8, device=DEV)
    apply = lambda rgb, light: ops.photo_lighting(d["verts"], d["faces"], d["face"], zbuf, rgb, d["pose"], d["image"], tau=0.5, light=light, mask=nothing)
    lit = apply(d["colour"], d["light"])
    assert (lit["status"] == 1).all() and same_bits(lit["light"], d["light"])
    unbiased = d["light"].clone()
    unbiased[:, :, 4] = 0.0
    s = apply(torch.ones_like(d["colour"]), unbiased)["rgb"]
    want = torch.where(covered[..., None], s * (d["image"] - lit["rgb"]), torch.zeros_like(s))
    got = gpu_call(c, True, False, diag=True)
    assert same_bits(got["grad"], want) and float(got["grad"].abs().max()) > 0
    assert same_bits(got["diag"], torch.where(covered[..., None], s * s, torch.zeros_like(s)))
    c["light"] = np.tile(LREF.IDENTITY, (B, 3, 1)).astype(np.float32)
    m = d["weight"][..., None]
    zero = torch.zeros_like(s)
    assert same_bits(gpu_call(c, True, True)["grad"], torch.where(covered[..., None], m * (d["image"] - d["colour"]), zero))
    assert same_bits(gpu_call(c, False, True, diag=True)["grad"], torch.where(covered[..., None], m * d["colour"], zero))
    assert same_bits(gpu_call(c, False, True, diag=True)["diag"], torch.where(covered[..., None], m.expand_as(s), zero))


# ----------------------------------------------------------------------------- memory, determinism, capture
def banded(shape, dtype):
    """A tensor between two 16-KiB bands of 0xAB -> (the tensor, a check that the bands are untouched)."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    pad = (-n) % 16
    raw = torch.full((BAND + n + pad + BAND,), 0xAB, dtype=torch.uint8, device=DEV)
    t = raw[BAND:BAND + n].view(dtype).view(shape)

    def untouched():
        return bool((raw[:BAND] == 0xAB).all()) and bool((raw[BAND + n:] == 0xAB).all())
    return t, untouched


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 7, 65), (3, 33, 257)])
def test_nothing_is_written_outside_the_outputs(B, H, W):
    """16-KiB bands of 0xAB around every output and the workspace; the workspace comes in filled with NaN."""
    from texpose_amd import ops
    c = call_case(21, "bumpy", B, H, W)
    want = gpu_call(c, diag=True, sums=True)
    out, checks = {}, []
    for k, (shape, dtype) in dict(grad=((B, H, W, 3), torch.float32), diag=((B, H, W, 3), torch.float32), sums=((B, 2), torch.float64)).items():
        out[k], check = banded(shape, dtype)
        checks.append(check)
    need = ops.face_texel_light_workspace(B, H, W, DEV).numel() * 8
    assert need == 16 * B * -(-H * W // 1024)
    ws, check = banded((need // 8,), torch.float64)
    checks.append(check)
    ws.fill_(float("nan"))
    got = gpu_call(c, diag=True, sums=True, workspace=ws, out=out)
    torch.cuda.synchronize()
    assert all(check() for check in checks)
    for k in out:
        assert got[k] is out[k] and same_bits(got[k], want[k]), k
    grad, check = banded((B, H, W, 3), torch.float32)                # operator mode: one output, no workspace
    gpu_call(c, False, True, out=dict(grad=grad))
    torch.cuda.synchronize()
    assert check() and same_bits(grad, gpu_call(c, False, True)["grad"])


def test_two_calls_and_graph_replay_are_bit_equal():
    from texpose_amd import ops
    B, H, W = 3, 33, 257
    c = call_case(31, "bumpy", B, H, W)
    d = {k: cu(v) for k, v in c.items()}
    call = lambda **kw: ops.face_texel_light(d["face"], d["verts"], d["faces"], d["colour"], d["pose"], d["light"], image=d["image"], weight=d["weight"],
                                             diag=True, sums=True, **kw)
    eager, again = call(), call()
    for k in eager:
        assert same_bits(eager[k], again[k]), k
    ws = ops.face_texel_light_workspace(B, H, W, DEV)
    cap = {k: torch.empty_like(v) for k, v in eager.items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(workspace=ws, out=cap)
    for _ in range(2):
        for v in cap.values():
            v.view(torch.uint8).fill_(0xAB)
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert same_bits(cap[k], eager[k]), k
    assert float(eager["sums"][:, 1].min()) > 0


def test_bad_arguments_are_refused():
    from texpose_amd import _lib, ops
    B, H, W = 2, 7, 65
    c = call_case(1, "bumpy", B, H, W)
    d = {k: cu(v) for k, v in c.items()}
    names = ("face", "verts", "faces", "colour", "pose", "light")
    args = lambda **over: [over.get(k, d[k]) for k in names]
    poisoned = torch.full((B, H, W, 3), 7.0, device=DEV)
    sums = torch.full((B, 2), 7.0, device=DEV, dtype=torch.float64)
    for kw in (dict(out=dict(grad=d["colour"])), dict(image=d["image"], out=dict(grad=d["image"])),       # an output that is an input
               dict(diag=True, out=dict(grad=poisoned, diag=poisoned)),                                   # two outputs in one place
               dict(image=d["image"], sums=True, out=dict(grad=poisoned, sums=sums), workspace=sums.view(-1))):
        with pytest.raises(_lib.TexposeLibraryError):
            ops.face_texel_light(*args(), **kw)
    torch.cuda.synchronize()
    assert (poisoned == 7.0).all() and (sums == 7.0).all()          # nothing was launched
    for bad in (lambda: ops.face_texel_light(*args(face=d["face"].long())), lambda: ops.face_texel_light(*args(face=d["face"][0])),
                lambda: ops.face_texel_light(*args(faces=d["faces"].long())), lambda: ops.face_texel_light(*args(faces=d["faces"][:, :2])),
                lambda: ops.face_texel_light(*args(faces=d["faces"][:0])), lambda: ops.face_texel_light(*args(verts=d["verts"][:, :2])),
                lambda: ops.face_texel_light(*args(colour=d["colour"].double())), lambda: ops.face_texel_light(*args(colour=d["colour"][:1])),
                lambda: ops.face_texel_light(*args(colour=d["colour"].permute(0, 3, 1, 2).contiguous())),
                lambda: ops.face_texel_light(*args(pose=d["pose"][:1])), lambda: ops.face_texel_light(*args(pose=d["pose"][:, :, :3])),
                lambda: ops.face_texel_light(*args(light=d["light"][:, :, :4])), lambda: ops.face_texel_light(*args(light=d["light"].double())),
                lambda: ops.face_texel_light(*args(), image=d["image"][:, :5]), lambda: ops.face_texel_light(*args(), image=d["image"].half()),
                lambda: ops.face_texel_light(*args(), weight=d["weight"] > 0), lambda: ops.face_texel_light(*args(), weight=d["weight"][..., None]),
                lambda: ops.face_texel_light(*args(), sums=True),                                                  # sums without image
                lambda: ops.face_texel_light(*args(), image=d["image"], sums=True, workspace=torch.empty(1, device=DEV)),   # too small
                lambda: ops.face_texel_light(*args(), out=dict(grad=torch.empty(B, H, W, 3, device=DEV, dtype=torch.float64))),
                lambda: ops.face_texel_light(*args(), diag=True, out=dict(diag=torch.empty(B, H, W, device=DEV)))):
        with pytest.raises(ValueError):
            bad()


# ----------------------------------------------------------------------------- the fitter
def test_fitter_recovers_a_consistent_system_under_the_true_lights():
    """photographs ops.face_texel_shade renders from random node colours x*, relit by the restatement's own apply under the case's lights;
    the true lights given, one round, the light step skipped: the bar is 4 x the restated loop's recorded error + 1e-4"""
    from texpose_amd import face_texels as FT, ops
    import test_face_texel_fit_cpu as K36T
    c = K36T.consistent_system()
    size, R, U = c["size"], c["R"], c["U"]
    lights = LT.view_lights(len(c["poses"]))
    v, f, p, k = cu(c["verts"]), cu(c["faces"]), cu(c["poses"]), cu(c["K"])
    face = ops.mesh_raster(v, f, p, k, H=size, W=size, normals=False)["face"]
    truth = cu(c["truth"].astype(np.float32))
    unlit = ops.face_texel_shade(face, v, f, truth[cu(c["node_index"])], p, k)
    photo = cu(LT.relight(c["verts"], c["faces"], host(face), c["poses"], host(unlit), lights))
    fitter = FT.FaceTexelFitter(c["verts"], c["faces"], R, size, size, DEV, lam=1e-6, iters=32, lighting=True, rounds=1)
    fitter.add_views(photo[:5], c["poses"][:5], c["K"], face=face[:5], weight=(face[:5] >= 0).float())
    fitter.add_views(photo[5:], c["poses"][5:], c["K"], weight=(face[5:] >= 0).float())           # (rasterised by the fitter: the same plane)
    res = fitter.fit(prior=None, start=torch.zeros(U, 3, device=DEV), lights=cu(lights), light_step=False)
    seen = res.coverage >= 1
    err = float((res.nodes - truth).abs()[seen].max())
    rms = host(res.rms).astype(np.float64)
    print("lit consistent system on the device: max |x - x*| %.3e on %d of %d nodes (CPU loop fp64 %.3e, fp32 %.3e); rms %.3e -> %.3e"
          % (err, int(seen.sum()), U, LT.CONSISTENT_ERROR, LT.CONSISTENT_ERROR_FP32, rms[0], rms[-1]))
    assert int(seen.sum()) >= 0.9 * U and err <= 4 * LT.CONSISTENT_ERROR + 1e-4
    assert rms.shape == (33,) and rms[-1] < 1e-3 * rms[0]
    assert same_bits(res.light, lights) and (res.lighting_status == 0).all()
    with pytest.raises(ValueError):
        FT.FaceTexelFitter(c["verts"], c["faces"], R, size, size, DEV).fit(lights=cu(lights))


def test_lit_fit_on_relit_photographs():
    """the relit round trip at 64 x 64 (R = 4, 14 views, each under its own light) against the restated loop's recorded figures
    (LT.RELIT['clean']); the plain fit on the same photographs; two fits are bit-equal; lighting=False is the fitter without the keyword"""
    from texpose_amd import face_texels as FT, ops
    import test_face_texel_light_cpu as CPU
    case = CPU.relit_case("clean")
    c, size, R = case["c"], CPU.SIZE, CPU.R
    rms_plain_cpu, rms_lit_cpu, psnr_plain_cpu, psnr_lit_cpu = LT.RELIT["clean"]
    rgb = cu(case["rgb"])
    baker = FT.FaceTexelBaker(c["verts"], c["faces"], R, size, size, DEV)
    baker.add_views(rgb, cu(c["poses"]), cu(c["K"]))
    bake = baker.result(fill=True).vcolor_sub

    def fit(**kw):
        fitter = FT.FaceTexelFitter(c["verts"], c["faces"], R, size, size, DEV, **kw)            # lam = 0.1, 4 iterations, 6 rounds
        fitter.add_views(rgb, c["poses"], c["K"])
        return fitter.fit(prior=bake, start=bake)

    lit, again, plain, keyword = fit(lighting=True), fit(lighting=True), fit(), fit(lighting=False)
    hrgb, _, hface = c["target"]
    held = ops.mesh_raster(cu(c["verts"]), cu(c["faces"]), cu(c["held"][None]), cu(c["K"]), H=size, W=size, normals=False)
    covered = (host(held["face"])[0] >= 0) & (hface >= 0)
    through = lambda texels: LT.affine_psnr(host(ops.face_texel_shade(held["face"], cu(c["verts"]), cu(c["faces"]), texels, cu(c["held"][None]),
                                                                      cu(c["K"])))[0], hrgb, covered)
    psnr_plain, psnr_lit = through(plain.texels), through(lit.texels)
    rms, rms_plain = host(lit.rms).astype(np.float64), host(plain.rms)
    print("lit fit on relit photographs %dx%d R=%d: training rms plain %.5f -> %.5f (CPU %.5f), lit %.5f -> %.5f (CPU %.5f); held-out gauge-free "
          "PSNR plain %.2f dB, lit %.2f dB (CPU %.2f, %.2f); gain %s; status %s flags %s"
          % (size, size, R, rms_plain[0], rms_plain[-1], rms_plain_cpu, rms[0], rms[-1], rms_lit_cpu, psnr_plain, psnr_lit, psnr_plain_cpu, psnr_lit_cpu,
             host(lit.gain).round(3).tolist(), host(lit.lighting_status).tolist(), host(lit.lighting_flags).tolist()))
    print("  lit rms series:", rms.round(5).tolist())
    assert psnr_lit >= psnr_lit_cpu - 1.0
    assert rms[-1] <= 1.02 * rms_lit_cpu + 1e-5
    assert psnr_lit - psnr_plain >= 0.5 * (psnr_lit_cpu - psnr_plain_cpu)
    assert rms.shape == (LT.ROUNDS * LT.ITERS + 1,) and lit.light.shape == (14, 3, 5) and lit.gain.shape == (3,)
    assert lit.lighting_status.shape == (14,) and lit.lighting_flags.shape == (14,) and isinstance(lit.on_prior, int)
    assert torch.allclose(lit.gain, lit.light[:, :, 0].mean(0), atol=1e-6)
    for k in ("nodes", "light", "rms", "coverage", "lighting_status", "lighting_flags", "gain"):
        assert same_bits(lit[k], again[k]), k
    for k in ("nodes", "rms", "coverage", "texels"):
        assert same_bits(plain[k], keyword[k]), k
    assert same_bits(lit.coverage, plain.coverage) and lit.on_prior == plain.on_prior and "light" not in plain


def test_tool_bake_fit_photos_with_lighting(tmp_path):
    """bake_texture --texel-res 4 --fit 4 --fit-photos ... --fit-lighting 3 on a random-weight checkpoint, the photographs being its own
    bake relit view by view: the texels are written and the final rms is below that of the same command without --fit-lighting"""
    import oracle.texpose_oracle as O
    from texpose_amd import checkpoint as ck, face_texels as FT, ops, texture_bake as TB
    from texpose_amd.graph import Graph
    from texpose_amd.options import default_options
    H, W, N, oid, views = 48, 64, 8, 5, 6
    opt = default_options(H=H, W=W, device=DEV)
    opt.nerf.sample_intvs, opt.nerf.sample_stratified = N, False
    opt.arch.mlp_precision = "fp32"
    graph = Graph(opt).to(DEV)
    graph.nerf.load_state_dict({**graph.nerf.state_dict(), **{k: v.to(DEV) for k, v in O.make_params(3).items()}})
    graph.attach_latents(4, opt)
    torch.save(ck.make_checkpoint(graph, epoch=1, it=10), str(tmp_path / "model.ckpt"))
    verts, faces = TREF.uv_sphere(12, 16)
    TB.write_ply(str(tmp_path / "sphere.ply"), verts, faces, np.zeros_like(verts))

    def tool(name, extra):
        out, report = tmp_path / (name + ".ply"), tmp_path / (name + ".json")
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "tools", "bake_texture.py"), "--checkpoint", str(tmp_path / "model.ckpt"),
               "--ply", "%d=%s" % (oid, tmp_path / "sphere.ply"), "--sphere", str(views), "--distance-mm", "400", "--focal", "150", "--H", str(H), "--W", str(W),
               "--samples", str(N), "--precision", "fp32", "--out", str(out), "--report", str(report), "--texel-res", "4"] + extra
        p = subprocess.run(cmd, capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        texels, R = FT.load_texels(str(tmp_path / (name + ".texels.npz")), faces)
        assert R == 4 and texels.shape == (len(faces), 15, 3) and np.isfinite(texels).all() and texels.min() >= 0 and texels.max() <= 1
        return texels, json.loads(report.read_text()), p.stdout

    baked, _, _ = tool("bake", [])
    pose = TB.sphere_view_poses(views, 400.0).astype(np.float32)
    K = np.array([[150.0, 0.0, W / 2.0], [0.0, 150.0, H / 2.0], [0.0, 0.0, 1.0]], np.float32)
    planes = ops.mesh_raster(cu(verts), cu(faces), cu(pose), cu(K)[None].expand(views, 3, 3).contiguous(), H=H, W=W, texels=cu(baked), normals=False)
    photos = LT.relight(verts, faces, host(planes["face"]), pose, host(planes["rgb"]), LT.view_lights(views)).clip(0, 1)
    with open(tmp_path / "photos.npz", "wb") as fh:
        np.savez(fh, rgb=photos, pose=pose, intr=K)
    common = ["--fit", "4", "--fit-photos", str(tmp_path / "photos.npz")]
    lit_texels, lit, stdout = tool("lit", common + ["--fit-lighting", "3"])
    plain_texels, plain, _ = tool("plain", common)
    print(stdout)
    fit = lit["fit"]
    assert fit["iters"] == 4 and fit["views"] == views and len(fit["rms"]) == 3 * 4 + 1 and fit["rms_after"] == fit["rms"][-1]
    assert fit["lighting"]["rounds"] == 3 and np.asarray(fit["lighting"]["light"]).shape == (views, 3, 5) and len(fit["lighting"]["gain"]) == 3
    assert len(fit["lighting"]["status"]) == views and "lighting" not in plain["fit"] and len(plain["fit"]["rms"]) == 5
    print("tool: final rms %.5f with --fit-lighting 3, %.5f without" % (fit["rms_after"], plain["fit"]["rms_after"]))
    assert fit["rms_after"] < plain["fit"]["rms_after"]
    assert not np.array_equal(lit_texels, plain_texels)
