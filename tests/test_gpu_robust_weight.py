"""K42 (tp_robust_weight) and FaceTexelFitter(robust=...) on the device against tests/robust_weight_ref.py: the call bit for bit on planted
inputs, memory and replay, refusals, the robust fit against the restated loop's recorded figures, and the tool's switches."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import robust_weight_ref as RW
import texture_bake_ref as TREF
from gn_ref import cu, host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 16384
ULP = 2.0 ** -23
VARIANTS = ("general", "none", "one", "equal", "lowbits")


def bits(t):
    return t.contiguous().view(torch.uint8) if torch.is_tensor(t) else np.ascontiguousarray(t).view(np.uint8)


def same_bits(a, b):
    a, b = (host(x) if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ----------------------------------------------------------------------------- one call, planted inputs
def call_case(seed, B, H, W, layout=0):
    """model and image in [0, 1] with 2 % NaN / +-Inf each, weights in (0.1, 2) with 0, negatives and NaN; image b is of the kind
    VARIANTS[(layout + b) % 5]: 'general' as drawn; 'none' without a counted pixel (every image value NaN); 'one' with exactly one;
    'equal' with one q everywhere (every level of the select has a single bin); 'lowbits' with q that differ in their lowest 10 bits only
    (grey values half an ulp-step apart around 0.5 against a black model)."""
    rs = np.random.RandomState(seed)
    model, image = rs.rand(B, H, W, 3).astype(np.float32), rs.rand(B, H, W, 3).astype(np.float32)
    weight = rs.uniform(0.1, 2.0, (B, H, W)).astype(np.float32)
    for plane in (model, image):
        u = rs.rand(*plane.shape)
        plane[u < 0.007], plane[(u >= 0.007) & (u < 0.014)], plane[(u >= 0.014) & (u < 0.02)] = np.nan, np.inf, -np.inf
    u = rs.rand(B, H, W)
    weight[u < 0.03], weight[(u >= 0.03) & (u < 0.06)], weight[(u >= 0.06) & (u < 0.09)] = 0.0, -0.5, np.nan
    kinds = [VARIANTS[(layout + b) % len(VARIANTS)] for b in range(B)]
    for b, kind in enumerate(kinds):
        if kind in ("none", "one"):
            image[b] = np.nan
            if kind == "one":
                y, x = rs.randint(H), rs.randint(W)
                model[b, y, x], image[b, y, x], weight[b, y, x] = rs.rand(3), rs.rand(3), 0.7
        elif kind == "equal":
            model[b], image[b] = 0.25, 0.5
        elif kind == "lowbits":
            grey = (np.float32(0.5).view(np.uint32) + rs.randint(0, 300, (H, W)).astype(np.uint32)).view(np.float32)
            model[b], image[b] = 0.0, grey[..., None]
    scale_in = np.array([0.05, 0.0, np.nan, 0.5, 3e-3], np.float32)[np.arange(B) % 5]
    return dict(model=model, image=image, weight=weight, scale_in=scale_in, kinds=kinds)


def gpu_call(case, weight=True, scale_in=False, **kw):
    from texpose_amd import ops
    return ops.robust_weight(cu(case["model"]), cu(case["image"]), weight=cu(case["weight"]) if weight else None,
                             scale_in=cu(case["scale_in"]) if scale_in else None, **kw)


def ref_call(c, weight=True, scale_in=False, kind="tukey", c_tune=None):
    return RW.robust_weight_ref(c["model"], c["image"], c["weight"] if weight else None, kind, c_tune, scale_in=c["scale_in"] if scale_in else None)


def compare(got, want, kind):
    assert set(got) == {"weight", "median_q", "scale", "count"}
    assert same_bits(got["median_q"], want["median_q"]), (host(got["median_q"]), want["median_q"])
    assert same_bits(got["count"], want["count"]), (host(got["count"]), want["count"])
    np.testing.assert_allclose(host(got["scale"]), want["scale"], rtol=ULP, atol=0)
    if kind == "tukey":
        assert same_bits(got["weight"], want["weight"])
    else:
        np.testing.assert_allclose(host(got["weight"]), want["weight"], rtol=ULP, atol=0)
        assert not host(got["weight"])[~want["counted"]].any()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 7), (33, 257), (64, 80)])
def test_call_equals_the_restatement(H, W, B):
    """64 x 80 takes the vector path, the others (H W no multiple of four) the guarded one; 33 x 257 spans nine tiles with a partial last
    one; every kind of image, with and without weight and scale_in, both weight functions."""
    seen, counted = set(), 0
    for layout in range(len(VARIANTS)):
        c = call_case(1000 * H + 10 * W + B + 7 * layout, B, H, W, layout)
        seen.update(c["kinds"])
        for kind in ("tukey", "huber"):
            for weight in (True, False):
                for scale_in in (False, True):
                    want = ref_call(c, weight, scale_in, kind)
                    compare(gpu_call(c, weight, scale_in, kind=kind), want, kind)
                    counted += int(want["count"].sum())
                    if not scale_in:
                        for b, k in enumerate(c["kinds"]):
                            n = int(want["count"][b])
                            assert (k != "none" or n == 0) and (k != "one" or n == 1), (k, n)
                            if k in ("equal", "lowbits") and n >= 2:
                                q = want["q"][b][want["counted"][b]].view(np.uint32)
                                assert (q.max() == q.min()) if k == "equal" else (q.max() > q.min() and (q.max() >> 10) == (q.min() >> 10))
    torch.cuda.synchronize()                                         # the calls ended clean
    assert seen == set(VARIANTS)
    if H * W >= 33 * 257:
        assert counted > 0.3 * 40 * B * H * W


def test_tuning_constants_and_the_floor():
    """c and sigma_min reach the kernel; a perfect fit (q = 0 everywhere) sits on the floor and keeps every weight"""
    c = call_case(5, 2, 33, 257)
    for kind, c_tune, sigma_min in (("tukey", 2.0, 0.05), ("huber", 0.7, 1e-4), ("tukey", 9.5, 0.5)):
        want = RW.robust_weight_ref(c["model"], c["image"], c["weight"], kind, c_tune, np.float32(sigma_min))
        compare(gpu_call(c, kind=kind, c=c_tune, sigma_min=sigma_min), want, kind)
    same = torch.rand(2, 64, 80, 3, device=DEV)
    base = torch.rand(2, 64, 80, device=DEV) + 0.5
    got = gpu_call(dict(model=host(same), image=host(same), weight=host(base)))
    assert same_bits(got["weight"], base) and not got["median_q"].any() and (got["count"] == 64 * 80).all()
    assert same_bits(got["scale"], torch.full((2,), 1.0 / 255.0, device=DEV))


def test_misaligned_planes_take_the_guarded_path():
    """image, then weight, as a view 4 bytes into its storage: 16 x 16 would take the vector path."""
    from texpose_amd import ops
    c = call_case(7, 2, 16, 16)
    d = {k: cu(c[k]) for k in ("model", "image", "weight")}
    aligned = ops.robust_weight(d["model"], d["image"], weight=d["weight"])
    compare(aligned, ref_call(c), "tukey")
    for off in ("image", "weight"):
        e = dict(d)
        store = torch.empty(d[off].numel() + 1, device=DEV)
        view = store[1:].view(d[off].shape)
        view.copy_(d[off])
        e[off] = view
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        got = ops.robust_weight(e["model"], e["image"], weight=e["weight"])
        for k in aligned:
            assert same_bits(got[k], aligned[k]), (off, k)


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


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 7, 65), (3, 33, 257), (2, 64, 80)])
def test_nothing_is_written_outside_the_outputs(B, H, W):
    """16-KiB bands of 0xAB around every output and the workspace; the workspace comes in filled with 0xFF."""
    from texpose_amd import _lib, ops
    c = call_case(21, B, H, W)
    need = int(_lib.load().tp_robust_weight_workspace_bytes(B, H, W))
    assert need == (4 * B * H * W + 15) // 16 * 16 + B * (4 * 5120 + 32) and ops.robust_weight_workspace(B, H, W, DEV).numel() * 8 >= need
    for scale_in in (False, True):
        want = gpu_call(c, scale_in=scale_in)
        out, checks = {}, []
        for k, (shape, dtype) in dict(weight=((B, H, W), torch.float32), median_q=((B,), torch.float32), scale=((B,), torch.float32),
                                      count=((B,), torch.int32)).items():
            out[k], check = banded(shape, dtype)
            out[k].view(torch.uint8).fill_(0xCD)
            checks.append(check)
        ws, check = banded((need,), torch.uint8)
        checks.append(check)
        ws.fill_(0xFF)
        got = gpu_call(c, scale_in=scale_in, workspace=ws, out=out)
        torch.cuda.synchronize()
        assert all(check() for check in checks)
        for k in out:
            assert got[k] is out[k] and same_bits(got[k], want[k]), k
        if scale_in:
            assert (ws == 0xFF).all()                                # (with scale_in the workspace is not used)


def test_two_calls_and_graph_replay_are_bit_equal():
    from texpose_amd import ops
    B, H, W = 3, 33, 257
    c = call_case(31, B, H, W)
    d = {k: cu(c[k]) for k in ("model", "image", "weight", "scale_in")}
    for scale_in in (None, d["scale_in"]):
        call = lambda **kw: ops.robust_weight(d["model"], d["image"], weight=d["weight"], scale_in=scale_in, **kw)
        eager, again = call(), call()
        for k in eager:
            assert same_bits(eager[k], again[k]), k
        ws = ops.robust_weight_workspace(B, H, W, DEV)
        cap = {k: torch.empty_like(v) for k, v in eager.items()}
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call(workspace=ws, out=cap)
        for _ in range(2):
            for v in cap.values():
                v.view(torch.uint8).fill_(0xAB)
            ws.view(torch.uint8).fill_(0xFF)
            g.replay()
            torch.cuda.synchronize()
            for k in eager:
                assert same_bits(cap[k], eager[k]), k
        assert int(eager["count"].max()) > 1000                      # (the case holds an image without a counted pixel and one with one)


def test_bad_arguments_are_refused():
    from texpose_amd import _lib, ops
    B, H, W = 2, 7, 65
    c = call_case(1, B, H, W)
    d = {k: cu(c[k]) for k in ("model", "image", "weight", "scale_in")}
    poisoned = torch.full((B, H, W), 7.0, device=DEV)
    for kw in (dict(weight=d["weight"], out=dict(weight=d["weight"])),                       # an output that is an input
               dict(out=dict(weight=poisoned, median_q=poisoned.view(-1)[:B])),              # two outputs in one place
               dict(out=dict(weight=poisoned), c=0.0), dict(out=dict(weight=poisoned), c=-4.685),
               dict(out=dict(weight=poisoned), c=float("nan")), dict(out=dict(weight=poisoned), sigma_min=0.0),
               dict(out=dict(weight=poisoned), sigma_min=float("inf"))):
        with pytest.raises(_lib.TexposeLibraryError):
            ops.robust_weight(d["model"], d["image"], **kw)
    torch.cuda.synchronize()
    assert (poisoned == 7.0).all()                                   # nothing was launched
    for bad in (lambda: ops.robust_weight(d["model"].double(), d["image"]), lambda: ops.robust_weight(d["model"][0], d["image"][0]),
                lambda: ops.robust_weight(d["model"], d["image"][:1]), lambda: ops.robust_weight(d["model"], d["image"].half()),
                lambda: ops.robust_weight(d["model"].permute(0, 3, 1, 2).contiguous(), d["image"]),
                lambda: ops.robust_weight(d["model"], d["image"], weight=d["weight"] > 0),
                lambda: ops.robust_weight(d["model"], d["image"], weight=d["weight"][..., None]),
                lambda: ops.robust_weight(d["model"], d["image"], scale_in=d["scale_in"][:1]),
                lambda: ops.robust_weight(d["model"], d["image"], scale_in=d["scale_in"].double()),
                lambda: ops.robust_weight(d["model"], d["image"], kind="cauchy"),
                lambda: ops.robust_weight(d["model"], d["image"], workspace=torch.empty(1, device=DEV)),            # too small
                lambda: ops.robust_weight(d["model"], d["image"], workspace=ops.robust_weight_workspace(B, H, W, DEV).view(torch.uint8)[8:]),
                lambda: ops.robust_weight(d["model"], d["image"], out=dict(weight=torch.empty(B, H, W, device=DEV, dtype=torch.float64))),
                lambda: ops.robust_weight(d["model"], d["image"], out=dict(count=torch.empty(B, device=DEV)))):
        with pytest.raises(ValueError):
            bad()


# ----------------------------------------------------------------------------- the fitter
def test_robust_fit_on_corrupted_photographs():
    """the corrupted round trip at 64 x 64 (R = 4, 14 views) against the restated loop's recorded figures (RW.ROBUST_FIT['corrupted']); two
    robust fits are bit-equal; robust=None is the fitter without the keyword; robust with lighting is refused"""
    from texpose_amd import face_texels as FT, ops
    import face_texel_fit_ref as FIT
    import test_robust_weight_cpu as CPU
    case = CPU.robust_case("corrupted")
    c, size, R = case["c"], CPU.SIZE, CPU.R
    _, psnr_plain_cpu, psnr_robust_cpu = RW.ROBUST_FIT["corrupted"]
    rgb = cu(case["rgb"])
    baker = FT.FaceTexelBaker(c["verts"], c["faces"], R, size, size, DEV)
    baker.add_views(rgb, cu(c["poses"]), cu(c["K"]))
    bake = baker.result(fill=True).vcolor_sub

    def fit(**kw):
        fitter = FT.FaceTexelFitter(c["verts"], c["faces"], R, size, size, DEV, **kw)            # lam = 0.1, 4 iterations, 6 rounds
        fitter.add_views(rgb[:5], c["poses"][:5], c["K"])
        fitter.add_views(rgb[5:], c["poses"][5:], c["K"])
        return fitter.fit(prior=bake, start=bake)

    robust, again, plain, keyword = fit(robust="tukey"), fit(robust="tukey"), fit(), fit(robust=None)
    hrgb, _, hface = c["target"]
    held = ops.mesh_raster(cu(c["verts"]), cu(c["faces"]), cu(c["held"][None]), cu(c["K"]), H=size, W=size, normals=False)
    covered = (host(held["face"])[0] >= 0) & (hface >= 0)
    through = lambda texels: FIT.psnr(host(ops.face_texel_shade(held["face"], cu(c["verts"]), cu(c["faces"]), texels, cu(c["held"][None]), cu(c["K"])))[0],
                                      hrgb, covered)
    psnr_plain, psnr_robust = through(plain.texels), through(robust.texels)
    rms, scale, kept = host(robust.rms).astype(np.float64), host(robust.scale), host(robust.kept)
    print("robust fit on corrupted photographs %dx%d R=%d: held-out PSNR plain %.2f dB, Tukey %.2f dB (CPU %.2f, %.2f); kept %s"
          % (size, size, R, psnr_plain, psnr_robust, psnr_plain_cpu, psnr_robust_cpu, kept.round(3).tolist()))
    print("  scale:", scale.round(5).tolist(), "| recorded", RW.ROBUST_FIT_SCALE)
    print("  rms series:", rms.round(5).tolist())
    assert abs(psnr_robust - psnr_robust_cpu) <= 1.0
    np.testing.assert_allclose(scale, RW.ROBUST_FIT_SCALE, rtol=0.02)
    assert rms.shape == (RW.ROUNDS * RW.ITERS + 1,) and scale.shape == kept.shape == (14,) and robust.robust_count.shape == (14,)
    np.testing.assert_allclose(host(robust.robust_count), (case["weight"] > 0).sum((1, 2)), rtol=0.01)       # (the device's own face planes)
    assert robust.robust_count.dtype == torch.int32 and (kept > 0.5).all() and (kept < 0.95).all()
    for k in ("nodes", "rms", "coverage", "texels", "scale", "kept", "robust_count"):
        assert same_bits(robust[k], again[k]), k
    for k in ("nodes", "rms", "coverage", "texels"):
        assert same_bits(plain[k], keyword[k]), k
    assert same_bits(robust.coverage, plain.coverage) and robust.on_prior == plain.on_prior and "scale" not in plain and set(plain) == set(keyword)
    with pytest.raises(ValueError):
        FT.FaceTexelFitter(c["verts"], c["faces"], R, size, size, DEV, robust="tukey", lighting=True)
    with pytest.raises(ValueError):
        FT.FaceTexelFitter(c["verts"], c["faces"], R, size, size, DEV, robust="cauchy")


def test_tool_bake_fit_robust(tmp_path):
    """bake_texture --texel-res 4 --fit 4 --fit-photos ... on a random-weight checkpoint, the photographs being its own bake with the
    corruption painted in: --fit-robust is refused with --fit-lighting; without --fit-robust the file is what FaceTexelFitter without the
    keyword gives from the same prior, bit for bit, and the report has no 'robust'; with it the report carries scale and kept per view"""
    import oracle.texpose_oracle as O
    from texpose_amd import checkpoint as ck, face_texels as FT, ops, texture_bake as TB
    from texpose_amd.graph import Graph
    from texpose_amd.options import default_options
    H, W, N, oid, views = 64, 64, 8, 5, 6
    opt = default_options(H=H, W=W, device=DEV)
    opt.nerf.sample_intvs, opt.nerf.sample_stratified = N, False
    opt.arch.mlp_precision = "fp32"
    graph = Graph(opt).to(DEV)
    graph.nerf.load_state_dict({**graph.nerf.state_dict(), **{k: v.to(DEV) for k, v in O.make_params(3).items()}})
    graph.attach_latents(4, opt)
    torch.save(ck.make_checkpoint(graph, epoch=1, it=10), str(tmp_path / "model.ckpt"))
    verts, faces = TREF.uv_sphere(12, 16)
    TB.write_ply(str(tmp_path / "sphere.ply"), verts, faces, np.zeros_like(verts))

    def command(name, extra):
        return ["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "tools", "bake_texture.py"), "--checkpoint", str(tmp_path / "model.ckpt"),
                "--ply", "%d=%s" % (oid, tmp_path / "sphere.ply"), "--sphere", str(views), "--distance-mm", "400", "--focal", "200", "--H", str(H), "--W", str(W),
                "--samples", str(N), "--precision", "fp32", "--out", str(tmp_path / (name + ".ply")), "--report", str(tmp_path / (name + ".json")),
                "--texel-res", "4"] + extra

    def tool(name, extra):
        p = subprocess.run(command(name, extra), capture_output=True, text=True)
        assert p.returncode == 0, p.stdout + p.stderr
        texels, R = FT.load_texels(str(tmp_path / (name + ".texels.npz")), faces)
        assert R == 4 and texels.shape == (len(faces), 15, 3) and np.isfinite(texels).all() and texels.min() >= 0 and texels.max() <= 1
        return texels, json.loads((tmp_path / (name + ".json")).read_text()), p.stdout

    p = subprocess.run(command("refused", ["--fit", "4", "--fit-robust", "--fit-lighting", "3"]), capture_output=True, text=True)
    assert p.returncode == 2 and "--fit-lighting" in p.stderr and not (tmp_path / "refused.ply").exists()
    baked, _, _ = tool("bake", [])
    pose = TB.sphere_view_poses(views, 400.0).astype(np.float32)
    K = np.array([[200.0, 0.0, W / 2.0], [0.0, 200.0, H / 2.0], [0.0, 0.0, 1.0]], np.float32)
    planes = ops.mesh_raster(cu(verts), cu(faces), cu(pose), cu(K)[None].expand(views, 3, 3).contiguous(), H=H, W=W, texels=cu(baked), normals=False)
    photos = RW.corrupt(host(planes["rgb"]), host(planes["face"]) >= 0)
    with open(tmp_path / "photos.npz", "wb") as fh:
        np.savez(fh, rgb=photos, pose=pose, intr=K)
    common = ["--fit", "4", "--fit-photos", str(tmp_path / "photos.npz")]
    plain_texels, plain, _ = tool("plain", common)
    robust_texels, robust, stdout = tool("robust", common + ["--fit-robust", "--fit-robust-rounds", "3"])
    print(stdout)
    # the plain route: the fitter as it was, from the same prior (the baked nodes) and the same photographs
    fitter = FT.FaceTexelFitter(verts, faces, 4, H, W, DEV, lam=0.1, iters=4)
    fitter.add_views(torch.from_numpy(photos), torch.from_numpy(pose), torch.from_numpy(K))
    prior = cu(FT.nodes_from_texels(baked, fitter.node_index_host, fitter.U))
    want = FT.texels_from_nodes(fitter.fit(prior=prior, start=prior).nodes.clamp(0, 1), fitter.node_index)
    assert same_bits(plain_texels, host(want)) and "robust" not in plain["fit"] and len(plain["fit"]["rms"]) == 5
    fit = robust["fit"]
    assert fit["robust"]["kind"] == "tukey" and fit["robust"]["rounds"] == 3 and len(fit["rms"]) == 3 * 4 + 1
    assert len(fit["robust"]["scale"]) == len(fit["robust"]["kept"]) == len(fit["robust"]["count"]) == views
    assert all(s >= 1.0 / 255.0 - 1e-9 for s in fit["robust"]["scale"]) and all(0.0 < k <= 1.0 for k in fit["robust"]["kept"])
    assert not np.array_equal(robust_texels, plain_texels)
