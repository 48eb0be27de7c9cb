"""The inference-only single-product MLP arithmetic (arch.mlp_precision = "f16", TP_MLP_F16) through the product API -> C ABI:
its arithmetic pinned against an fp16-operand emulation of the oracle, its accuracy against the fp64 oracle, full-image
synthesis at 480x640 against the exact-fp32 kernel, the range fallback, the one-call C entry point and its absence from
training."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

from f16_emulation import emulate_f16, posenc64 as _posenc64, rays as _rays, rel_l2
from oracle import texpose_oracle as O

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def cu(t):
    return t.to(dev())


@pytest.fixture(scope="module")
def ops():
    from texpose_amd import ops as _ops
    return _ops


def _graph(params, n_train=5, emb_seed=77, H=16, W=16, N=8, precision="f16"):
    from texpose_amd.graph import Graph
    from texpose_amd.options import default_options
    opt = default_options(H=H, W=W, device="cuda:0")
    opt.nerf.sample_intvs = N
    opt.arch.mlp_precision = precision
    g = Graph(opt).to(dev())
    g.nerf.load_state_dict({**g.nerf.state_dict(), **{k: cu(v) for k, v in params.items()}})
    g.attach_latents(n_train, opt)
    ers = np.random.RandomState(emb_seed)
    with torch.no_grad():
        g.latent_vars_trans.weight.copy_(torch.from_numpy(ers.normal(size=(n_train, 16)).astype(np.float32)))
        g.latent_vars_light.weight.copy_(torch.from_numpy(ers.normal(size=(n_train, 48)).astype(np.float32)))
    return g, opt


# ------------------------------------------------------------------------------------------ 1. arithmetic pinned
@pytest.mark.parametrize("form", ["A_plain_N64", "A_ray_bias_N128", "B"])
def test_f16_kernel_matches_fp16_operand_emulation(ops, form):
    params = O.make_params(41)
    N = 128 if form == "A_ray_bias_N128" else 64
    center, ray, depth, pts, unit, lt, ll = _rays(3, 2, 7, N)
    rb = form == "A_ray_bias_N128"
    assert ops.ray_bias_applies("f16", N, False, True) == rb
    packed = ops.pack_weights({k: cu(v) for k, v in params.items()}, precision="f16", ray_bias=rb)
    ops.mlp_status(dev()).zero_()
    if form == "B":
        out = ops.mlp_forward(packed, cu(lt), cu(ll), points=cu(pts), ray_unit=cu(unit), precision="f16")
    else:
        out = ops.mlp_forward(packed, cu(lt), cu(ll), center=cu(center), ray=cu(ray), depth=cu(depth), precision="f16", ray_bias=rb)
    ops.check_mlp_status(dev())
    emu = emulate_f16(params, pts, unit, lt, ll, ray_bias=rb)
    exact = emulate_f16(params, pts, unit, lt, ll, ray_bias=rb, rounded=False)
    # Bars: a layout / permutation error gives O(1); round-toward-zero operands or unrounded layers put the kernel as far from the
    # emulation as the emulation is from exact arithmetic.  The floor is set by fp16 rounding flips: two implementations that both
    # accumulate the SAME rounded operands in fp32 and fp64 differ by 1.1e-4 / 0.9e-4 / 2.0e-4 (rgb / density / uncert) on these
    # inputs, so uncert (three more layers behind its softplus) gets 2e-4 instead of 1e-4
    for a, e, x, name, bar in zip(out, emu, exact, ("rgb", "density", "uncert"), (1e-4, 1e-4, 2e-4)):
        err, budget = rel_l2(a, e), rel_l2(e, x)
        print(form, name, "rel-L2 vs fp16-operand emulation %.2e (emulation vs exact arithmetic %.2e)" % (err, budget))
        assert err <= bar and err <= 0.5 * budget, (form, name, err, budget)


def _check_vs_emulation(tag, out, emu, exact):
    """the bars and rule of test_f16_kernel_matches_fp16_operand_emulation on each output AND on each channel of rgb / density
    (channel 0 static, 1 transient: the transient channels come from the head that also gives uncert, so they get its bar)"""
    res = []
    for a, e, x, name, bar in zip(out, emu, exact, ("rgb", "density", "uncert"), (1e-4, 1e-4, 2e-4)):
        parts = [(name, a, e, x, bar)]
        if name != "uncert":
            parts += [("%s[%d]" % (name, c), a[..., c], e[..., c], x[..., c], (1e-4, 2e-4)[c]) for c in (0, 1)]
        for what, a_, e_, x_, bar_ in parts:
            err, budget = rel_l2(a_, e_), rel_l2(e_, x_)
            print(tag, what, "rel-L2 vs fp16-operand emulation %.2e (bar %.0e, emulation vs exact arithmetic %.2e)" % (err, bar_, budget))
            res.append((what, err, bar_, budget))
    for what, err, bar_, budget in res:
        assert err <= bar_ and err <= 0.5 * budget, (tag, what, err, bar_, budget)


@pytest.mark.parametrize("B,R,N", [(3, 45, 1), (1, 77, 5), (3, 13, 33), (1, 9, 100), (3, 7, 100)])
def test_f16_plain_tiling_edges_match_emulation(ops, B, R, N):
    """plain stream, forms A and B: S % 128 != 0 tails, tiles that straddle rays and images (distinct latents per image), N = 1 and N
    not a multiple of the 32-sample wave tile.  Form A and form B are bit-identical (as test_mlp_vs_oracle_forms asks of fp32)."""
    params = O.make_params(43)
    center, ray, depth, pts, unit, lt, ll = _rays(B * 1000 + R * 10 + N, B, R, N)
    assert not ops.ray_bias_applies("f16", N, False, True)
    packed = ops.pack_weights({k: cu(v) for k, v in params.items()}, precision="f16")
    ops.mlp_status(dev()).zero_()
    out_a = ops.mlp_forward(packed, cu(lt), cu(ll), center=cu(center), ray=cu(ray), depth=cu(depth), precision="f16")
    out_b = ops.mlp_forward(packed, cu(lt), cu(ll), points=cu(pts), ray_unit=cu(unit), precision="f16")
    ops.check_mlp_status(dev())
    for a, b, name in zip(out_a, out_b, ("rgb", "density", "uncert")):
        assert torch.equal(a, b), ("form A vs form B", name)
    _check_vs_emulation("B=%d R=%d N=%d" % (B, R, N), out_a, emulate_f16(params, pts, unit, lt, ll),
                        emulate_f16(params, pts, unit, lt, ll, rounded=False))


@pytest.mark.parametrize("B,R,N", [(1, 1, 128), (1, 31, 256), (3, 11, 128), (3, 11, 256), (1, 33, 256), (1, 65, 128)])
def test_f16_ray_bias_partial_ray_blocks_match_emulation(ops, B, R, N):
    """ray-bias stream with B*R in {1, 31, 33, 65}: the per-ray pre-kernel's last 32-ray block (kRbRays) is partial, and with B = 3
    a block spans images (per-image light code)"""
    params = O.make_params(44)
    center, ray, depth, pts, unit, lt, ll = _rays(B * 1000 + R * 10 + N // 128, B, R, N)
    assert ops.ray_bias_applies("f16", N, False, True)
    packed = ops.pack_weights({k: cu(v) for k, v in params.items()}, precision="f16", ray_bias=True)
    ops.mlp_status(dev()).zero_()
    out = ops.mlp_forward(packed, cu(lt), cu(ll), center=cu(center), ray=cu(ray), depth=cu(depth), precision="f16", ray_bias=True)
    ops.check_mlp_status(dev())
    _check_vs_emulation("ray bias B=%d R=%d N=%d" % (B, R, N), out, emulate_f16(params, pts, unit, lt, ll, ray_bias=True),
                        emulate_f16(params, pts, unit, lt, ll, ray_bias=True, rounded=False))


@pytest.mark.parametrize("rb", [False, True], ids=["plain", "ray_bias"])
def test_f16_many_tiles_persistent(ops, rb):
    """the f16 twin of test_mlp_many_tiles_persistent: >= 3x the CU count in tiles and a tile count that is not a multiple of the
    grid, so every workgroup runs several tiles and wraps its weight stream (60 / 55 chunks) from the last chunk back to chunk 0;
    a strided subset of rays against the emulation, and bit-identical repeat runs"""
    B, R, N = 2, 1201, 128
    n_tiles, cus = B * R * N // 128, torch.cuda.get_device_properties(dev()).multi_processor_count
    assert n_tiles >= 3 * cus and n_tiles % cus, (n_tiles, cus)
    params = O.make_params(45)
    center, ray, depth, pts, unit, lt, ll = _rays(17, B, R, N)
    packed = ops.pack_weights({k: cu(v) for k, v in params.items()}, precision="f16", ray_bias=rb)
    ops.mlp_status(dev()).zero_()
    args = dict(center=cu(center), ray=cu(ray), depth=cu(depth), precision="f16", ray_bias=rb)
    out = ops.mlp_forward(packed, cu(lt), cu(ll), **args)
    again = ops.mlp_forward(packed, cu(lt), cu(ll), **args)
    ops.check_mlp_status(dev())
    for a, b, name in zip(out, again, ("rgb", "density", "uncert")):
        assert torch.equal(a, b), ("run to run", name)
    sel = torch.arange(R - 1, -1, -47).flip(0)                    # (the last ray, i.e. the last tile of each image, included)
    emu = emulate_f16(params, pts[:, sel], unit[:, sel], lt, ll, ray_bias=rb)
    exact = emulate_f16(params, pts[:, sel], unit[:, sel], lt, ll, ray_bias=rb, rounded=False)
    _check_vs_emulation("%d tiles on %d CUs, %s" % (n_tiles, cus, "ray bias" if rb else "plain"), [o.cpu()[:, sel] for o in out], emu, exact)


# ------------------------------------------------------------------------------------------ 2. accuracy vs the fp64 oracle
def _per_ray_errors(ops, graph, opt, params64, sc, K, H, W):
    """render_by_slices(mode="val") with the f16 kernel vs the fp64 oracle on the rays the HIP ray-gen produced"""
    c = cu
    dr = (c(sc["z_near"])[:, :, None], c(sc["z_far"])[:, :, None])
    mask = torch.ones(1, H, W, device=dev())
    N = opt.nerf.sample_intvs
    idx = c(torch.arange(H * W)[None])
    center, ray, _, _, depth = ops.raygen(c(K), c(sc["pose"]), H=H, W=W, n_samples=N, ray_idx=idx, z_near=dr[0], z_far=dr[1])
    et = graph.latent_vars_trans.weight.detach().cpu()[:1].double()
    el = graph.latent_vars_light.weight.detach().cpu()[:1].double()
    saved = O.posenc
    O.posenc = _posenc64
    try:
        with torch.no_grad():
            r_o, d_o, u_o = O.forward_samples(params64, center.cpu().double(), ray.cpu().double(), depth.cpu().double()[..., None], et, el)
            ref = O.composite(ray.cpu().double(), r_o, d_o, depth.cpu().double()[..., None], u_o, 0.05)
    finally:
        O.posenc = saved
    graph.nerf.precision = "f16"
    with torch.no_grad():
        ret = graph.render_by_slices(opt, c(sc["pose"]), intr=c(K), depth_range=dr, object_mask=mask, sample_idx=None, mode="val")
    ops.check_mlp_status(dev())
    out = {}
    for name, i in (("rgb", 0), ("rgb_static", 1)):
        d = ret[name].cpu().double().reshape(-1, 3) - ref[i].reshape(-1, 3)
        out[name] = (float(d.abs().max()), float(d.pow(2).mean().sqrt()))
    out["opacity"] = float((ret["opacity"].cpu().double().reshape(-1) - ref[4].reshape(-1)).abs().max())
    out["depth"] = rel_l2(ret["depth"].reshape(-1), ref[3].reshape(-1))
    return out


def _check_accuracy(errs, what):
    print(what, errs)
    for name in ("rgb", "rgb_static"):
        mx, rms = errs[name]
        assert mx <= 4e-3 and rms <= 1e-3, (what, name, mx, rms)
    assert errs["opacity"] <= 4e-3, (what, errs["opacity"])
    assert errs["depth"] <= 1e-3, (what, errs["depth"])


def test_f16_accuracy_vs_fp64_oracle_random_weights(ops):
    H, W, N = 48, 64, 64
    sc = O.synthetic_scene(H, W, B=1, seed=1)
    K = sc["intr"].clone()
    K[:, 0, 0] = K[:, 1, 1] = 700.0 * H / 128.0
    K[:, 0, 2], K[:, 1, 2] = W / 2.0, H / 2.0
    params = O.make_params(3)
    graph, opt = _graph(params, H=H, W=W, N=N)
    opt.nerf.sample_stratified = False
    _check_accuracy(_per_ray_errors(ops, graph, opt, {k: v.double() for k, v in params.items()}, sc, K, H, W), "make_params")


def test_f16_accuracy_vs_fp64_oracle_trained_network(ops):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import trained_weights as TW
    graph, trainer, _ = TW.train_heads(dev(), iters=200)
    assert trainer.skipped_steps == 0
    from texpose_amd.options import default_options
    H, W, N = 48, 64, 64
    opt = default_options(H=H, W=W, device="cuda:0")
    opt.nerf.sample_intvs, opt.nerf.sample_stratified = N, False
    sc = O.synthetic_scene(H, W, B=1, seed=1)
    K = sc["intr"].clone()
    K[:, 0, 0] = K[:, 1, 1] = 700.0 * H / 128.0
    K[:, 0, 2], K[:, 1, 2] = W / 2.0, H / 2.0
    params64 = {k: v.detach().cpu().double() for k, v in graph.nerf.state_dict().items() if k.startswith("mlp_")}
    graph.eval()
    _check_accuracy(_per_ray_errors(ops, graph, opt, params64, sc, K, H, W), "trained network")


# ------------------------------------------------------------------------------------------ 3. full image at C2
@pytest.mark.parametrize("N", [128, 64])
def test_f16_full_image_480x640(ops, N):
    import bench
    from texpose_amd.graph import Graph
    H, W = 480, 640
    sc, params, emb_t, emb_l = bench.build_scene(dev(), 0)
    graph, opt = bench.make_graph(dev(), params, emb_t, emb_l)
    opt.nerf.sample_intvs, opt.nerf.sample_stratified = N, False
    pose, intr = cu(sc["pose"]), cu(sc["intr"])
    dr = (cu(sc["z_near"])[:, :, None], cu(sc["z_far"])[:, :, None])
    mask = torch.ones(1, H, W, device=dev())
    sidx = torch.tensor(0, device=dev())

    def render(prec, slice_rays=None):
        graph.nerf.precision = prec
        opt.nerf.slice_rays = slice_rays
        with torch.no_grad():
            return graph.render_by_slices(opt, pose, intr=intr, depth_range=dr, object_mask=mask, sample_idx=sidx, mode="eval_noalign")

    exact = render("fp32")
    got = render("f16")
    again = render("f16")
    sliced = render("f16", slice_rays=2048)
    ops.check_mlp_status(dev())
    assert isinstance(graph, Graph) and getattr(graph, "range_fallbacks", 0) == 0
    for k in ("rgb", "rgb_static", "depth", "opacity", "uncert"):
        assert torch.equal(got[k], again[k]), ("run to run", k)
        assert torch.equal(got[k], sliced[k]), ("2048-ray slices", k)
    e8 = (exact["rgb_static"].clamp(0, 1) * 255).byte().int()
    g8 = (got["rgb_static"].clamp(0, 1) * 255).byte().int()
    d8 = (g8 - e8).abs()
    print("N=%d: 8-bit max diff %d, share differing %.2e" % (N, int(d8.max()), float((d8 > 0).double().mean())))
    assert int(d8.max()) <= 1
    gen = torch.Generator().manual_seed(5)
    target = (exact["rgb_static"].view(1, H, W, 3).permute(0, 3, 1, 2) + cu(torch.randn(1, 3, H, W, generator=gen)) * 0.02).clamp(0, 1)
    ps_e, ss_e, _ = ops.eval_metrics(exact["rgb_static"].view(1, H * W, 3), target.contiguous(), mask, H, W)
    ps_g, ss_g, _ = ops.eval_metrics(got["rgb_static"].view(1, H * W, 3), target.contiguous(), mask, H, W)
    print("N=%d: PSNR %.4f vs %.4f, SSIM %.6f vs %.6f" % (N, float(ps_g), float(ps_e), float(ss_g), float(ss_e)))
    assert abs(float(ps_g - ps_e)) <= 0.05 and abs(float(ss_g - ss_e)) <= 1e-3


# ------------------------------------------------------------------------------------------ 4. range flag
def test_f16_range_flag_falls_back_to_fp32_in_render_by_slices(ops):
    H, W, N = 16, 16, 32
    sc = O.synthetic_scene(H, W, B=1, seed=1)
    K = sc["intr"].clone()
    K[:, 0, 0] = K[:, 1, 1] = 700.0 * H / 128.0
    K[:, 0, 2], K[:, 1, 2] = W / 2.0, H / 2.0
    params = O.make_params(31)
    big = {k: (v * 300.0 if k in ("mlp_feat.2.weight", "mlp_feat.3.weight") else v) for k, v in params.items()}
    graph, opt = _graph(big, H=H, W=W, N=N)
    opt.nerf.sample_stratified = False
    graph.eval()
    dr = (cu(sc["z_near"])[:, :, None], cu(sc["z_far"])[:, :, None])
    mask = torch.ones(1, H, W, device=dev())
    ops.mlp_status(dev()).zero_()
    graph.nerf.precision = "fp32"
    with torch.no_grad():
        want = graph.render_by_slices(opt, cu(sc["pose"]), intr=cu(K), depth_range=dr, object_mask=mask, sample_idx=None, mode="val")
    graph.nerf.precision = "f16"
    graph.range_fallbacks = 0
    with torch.no_grad(), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = graph.render_by_slices(opt, cu(sc["pose"]), intr=cu(K), depth_range=dr, object_mask=mask, sample_idx=None, mode="val")
    assert any("fp16 range" in str(w.message) for w in caught)
    assert graph.range_fallbacks == 1 and graph.nerf.precision == "f16"
    for k in ("rgb", "rgb_static", "depth", "uncert", "density", "alpha_static"):
        assert torch.equal(got[k], want[k]), k
    assert int(ops.mlp_status(dev()).item()) == 0


# ------------------------------------------------------------------------------------------ 5. one-call path
def test_f16_render_eval_one_call_equals_mirror(ops):
    rs = np.random.RandomState(8)
    H, W, B = 24, 32, 2
    sc = O.synthetic_scene(H, W, B=B, seed=6)
    params = O.make_params(25)
    idx = torch.from_numpy(rs.randint(0, H * W, size=(B, 301)).astype(np.int64))
    for N in (16, 128):
        g, opt = _graph(params, H=H, W=W, N=N)
        opt.nerf.sample_stratified = False
        rb = ops.ray_bias_applies("f16", N, False, True)
        assert rb == (N == 128)
        lat_t = g.latent_vars_trans.weight[0][None].expand(B, -1).contiguous()
        lat_l = g.latent_vars_light.weight[0][None].expand(B, -1).contiguous()
        with torch.no_grad():
            ref = g.render(opt, cu(sc["pose"]), intr=cu(sc["intr"]), ray_idx=cu(idx),
                           depth_range=(cu(sc["z_near"])[:, :, None], cu(sc["z_far"])[:, :, None]), sample_idx=None, mode="val")
            out = ops.render_eval(g.nerf.packed_weights("f16", ray_bias=rb), cu(sc["intr"]), cu(sc["pose"]), cu(idx), cu(sc["z_near"]),
                                  cu(sc["z_far"]), lat_t, lat_l, H=H, W=W, n_samples=N, precision="f16", ray_bias=rb)
        for name, lo, hi in ops.COMPOSITE_RAY_FIELDS:
            assert torch.equal(out[..., lo:hi], ref[name]), (N, name)
    ops.check_mlp_status(dev())


# ------------------------------------------------------------------------------------------ 6. stays out of training
def test_f16_precision_leaves_training_render_and_backward_unchanged(ops):
    H, W, N = 16, 16, 16
    sc = O.synthetic_scene(H, W, B=1, seed=1)
    params = O.make_params(5)
    rs = np.random.RandomState(0)
    coords = cu(torch.from_numpy(rs.uniform(-0.8, 0.8, size=(1, 4, 4, 2)).astype(np.float32)))
    res = {}
    for prec in ("f16", "f16x3"):
        g, opt = _graph(params, H=H, W=W, N=N, precision=prec)
        opt.nerf.sample_stratified = False
        opt.nerf.density_noise_reg = None
        assert g.nerf.precision == prec and g.nerf.train_precision == "f16x3"
        torch.manual_seed(0)
        ret = g.render(opt, cu(sc["pose"]), intr=cu(sc["intr"]), ray_idx=coords,
                       depth_range=(cu(sc["z_near"])[:, :, None], cu(sc["z_far"])[:, :, None]),
                       sample_idx=cu(torch.tensor([2])), mode="train")
        (ret.rgb.sum() + ret.density[..., 1].mean()).backward()
        res[prec] = (ret.rgb.detach().clone(), ret.density.detach().clone(),
                     [p.grad.clone() for _, p in g.nerf.head_parameters()],
                     g.latent_vars_light.weight.grad.clone())
    a, b = res["f16"], res["f16x3"]
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    assert torch.equal(a[3], b[3])


# ------------------------------------------------------------------------------------------ 7. stream packing: partial repacks
@pytest.mark.parametrize("part", ["heads", "trunk"])
@pytest.mark.parametrize("precision,rb", [("f16", False), ("f16", True), ("f16x3", False), ("f16x3", True)],
                         ids=["f16", "f16_ray_bias", "f16x3", "f16x3_ray_bias"])
def test_partial_repack_equals_full_pack(ops, precision, rb, part):
    """pack(A, ALL) then pack(B, part) == pack({A outside part, B inside it}, ALL), bit for bit, from zero-filled buffers: the part's
    chunk range (kFirstHeadChunk16 / ...RB for f16), its biases, head scalars and aux rows are rewritten and nothing else is.
    (B is passed whole: a repack that read the other part would show as a difference.)"""
    pa, pb = O.make_params(51), O.make_params(52)
    mask = ops.PACK_HEADS if part == "heads" else ops.PACK_TRUNK
    mixed = {k: (pb if k.startswith("mlp_feat") == (part == "trunk") else pa)[k] for k in pa}
    n = ops.packed_bytes() // 4
    got, want = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    ops.pack_weights({k: cu(v) for k, v in pa.items()}, packed=got, precision=precision, ray_bias=rb)
    ops.pack_weights({k: cu(v) for k, v in pb.items()}, packed=got, parts=mask, precision=precision, ray_bias=rb)
    ops.pack_weights({k: cu(v) for k, v in mixed.items()}, packed=want, precision=precision, ray_bias=rb)
    diff = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
    assert diff.numel() == 0, ("first differing float", int(diff[0]), "of", n)
    full_a, full_b = ({k: cu(v) for k, v in p.items()} for p in (pa, pb))
    full_a = ops.pack_weights(full_a, packed=torch.zeros(n, device=dev()), precision=precision, ray_bias=rb)
    full_b = ops.pack_weights(full_b, packed=torch.zeros(n, device=dev()), precision=precision, ray_bias=rb)
    assert not torch.equal(got, full_a) and not torch.equal(got, full_b)


def test_f16_render_after_training_step_uses_current_heads(ops):
    """NeRF.packed_weights repacks only the heads of the cached f16 streams (PACK_HEADS | PACK_F16) when an optimiser step bumped a
    head version -- what a training run does when it renders a validation view with precision = "f16".  One eager f16x3 training
    step, then f16 renders (plain stream at N = 64, ray-bias stream at N = 128) through the cached streams must be bit-identical to
    those of a freshly built graph loaded with the stepped weights."""
    H, W, B = 16, 16, 1
    sc = O.synthetic_scene(H, W, B=B, seed=2)
    params = O.make_params(53)
    rs = np.random.RandomState(4)
    idx = cu(torch.from_numpy(rs.randint(0, H * W, size=(B, 97)).astype(np.int64)))
    dr = (cu(sc["z_near"])[:, :, None], cu(sc["z_far"])[:, :, None])
    g, opt = _graph(params, H=H, W=W, N=16, precision="f16")
    opt.nerf.sample_stratified = False
    opt.nerf.density_noise_reg = None

    def render(graph, N):
        opt.nerf.sample_intvs = N
        with torch.no_grad():
            return graph.render(opt, cu(sc["pose"]), intr=cu(sc["intr"]), ray_idx=idx, depth_range=dr, sample_idx=None, mode="val")

    before = {N: render(g, N) for N in (64, 128)}                   # builds and caches both f16 streams
    heads = [p for _, p in g.nerf.head_parameters()]
    optim = torch.optim.Adam(heads, lr=1e-2)
    opt.nerf.sample_intvs = 16
    coords = cu(torch.from_numpy(rs.uniform(-0.8, 0.8, size=(B, 4, 4, 2)).astype(np.float32)))
    ret = g.render(opt, cu(sc["pose"]), intr=cu(sc["intr"]), ray_idx=coords, depth_range=dr, sample_idx=cu(torch.tensor([1])),
                   mode="train")
    (ret.rgb.sum() + ret.density[..., 1].mean()).backward()
    optim.step()
    fresh, _ = _graph({k: v.detach().cpu() for k, v in g.nerf.state_dict().items() if k.startswith("mlp_")}, H=H, W=W, N=16)
    for N in (64, 128):
        got, want = render(g, N), render(fresh, N)
        assert not torch.equal(got["rgb"], before[N]["rgb"]), N          # the step changed what is rendered
        for name, _, _ in ops.COMPOSITE_RAY_FIELDS:
            assert torch.equal(got[name], want[name]), (N, name)
    ops.check_mlp_status(dev())
