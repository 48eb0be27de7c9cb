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

from oracle import texpose_oracle as O

pytestmark = pytest.mark.gpu

WIDE_OUT = 256


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def cu(t):
    return t.to(dev())


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


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


def _posenc64(x, L):
    freq = (2 ** torch.arange(L, dtype=torch.float32)) * np.pi
    spec = (x.float()[..., None] * freq).double()          # the fp32-rounded argument the kernel encodes
    return torch.stack([spec.sin(), spec.cos()], dim=-2).reshape(*x.shape[:-1], -1)


def emulate_f16(params, points, ray_unit, lat_trans, lat_light, ray_bias=False, rounded=True):
    """The oracle in fp64 with the operands of every 256-wide layer rounded to fp16 (nearest even): weights and inputs of
    mlp_feat.0-7 (without the density row of mlp_feat.7), mlp_rgb.0-2, mlp_trans.0-2.  The narrow output layers stay exact.
    ``ray_bias``: the ray-constant columns (mlp_rgb.0 view encoding 256..282 and light code 286..333, mlp_trans.0 transient code
    256..271) are contracted unrounded, as the per-ray bias pre-kernels do.  ``rounded=False``: no rounding at all (fp64 oracle)."""
    p64 = {k: v.double() for k, v in params.items()}
    names = {id(v): k for k, v in p64.items()}
    exact_cols = {"mlp_rgb.0.weight": list(range(256, 283)) + list(range(286, 334)), "mlp_trans.0.weight": list(range(256, 272))}
    lin = torch.nn.functional.linear

    def linear(x, w, b=None):
        name = names.get(id(w), "")
        if w.shape[0] < WIDE_OUT or not rounded:
            return lin(x, w, b)                                   # narrow output layer: exact
        keep = torch.zeros(w.shape[1], dtype=torch.bool)
        if ray_bias and name in exact_cols:
            keep[exact_cols[name]] = True
        xr = torch.where(keep, x, x.half().double())
        wr = torch.where(keep, w, w.half().double())
        out = lin(xr, wr, b)
        if w.shape[0] == WIDE_OUT + 1:                            # mlp_feat.7: row 0 is the density head
            out[..., 0] = lin(x, w[:1], None if b is None else b[:1])[..., 0]
        return out

    saved = O.posenc, torch.nn.functional.linear
    O.posenc, torch.nn.functional.linear = _posenc64, linear
    try:
        with torch.no_grad():
            return O.mlp_forward(p64, points.double(), ray_unit.double(), lat_trans.double(), lat_light.double())
    finally:
        O.posenc, torch.nn.functional.linear = saved


def _rays(seed, B, R, N):
    """form-A inputs (center, ray, depth) and the points / unit directions the kernel derives from them in fp32"""
    rs = np.random.RandomState(seed)
    center = torch.from_numpy(rs.uniform(-0.3, 0.3, size=(B, R, 3)).astype(np.float32))
    ray = torch.from_numpy(rs.normal(size=(B, R, 3)).astype(np.float32))
    depth = torch.from_numpy(np.sort(rs.uniform(0.2, 1.4, size=(B, R, N)), axis=-1).astype(np.float32))
    pts = center[:, :, None] + ray[:, :, None] * depth[..., None]
    unit = (ray / ray.norm(dim=-1, keepdim=True).clamp_min(1e-12))[:, :, None].expand(B, R, N, 3).contiguous()
    lt = torch.from_numpy(rs.normal(size=(B, 16)).astype(np.float32))
    ll = torch.from_numpy(rs.normal(size=(B, 48)).astype(np.float32))
    return center, ray, depth, pts, unit, lt, ll


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
