"""The range guard and the activation maximum of the two fp16 MLP arithmetics (f16x3, f16), layer by layer.

Networks are rescaled with ReLU's positive homogeneity (f16_emulation.rescale): one hidden output is multiplied by 2^k and its
consumers divide it back out, so the network function is unchanged and only that layer's activations move -- to about half the fp16
range ("inside": the flag stays clear and the result keeps its accuracy bar) or past it ("outside": check_mlp_status raises).

The f16x3 stream carries W * 2^8 as fp16 hi + lo, so it holds weights below 2^8 in magnitude only (include/texpose_amd.h).  Scaling
a layer's rows by 2^13 would leave that range, so for f16x3 the layer that FEEDS the scaled one is lifted by 2^c as well (the
scaled layer's rows then only grow by 2^(k - c)); mlp_feat.0, mlp_feat.4 and mlp_rgb.0 also read encodings, which cannot be lifted,
so their f16x3 cases stay at the largest k the weight range allows (inside only).  Where the rescaling leaves lo halves subnormal,
f16x3 is held to the narrower accuracy contract of include/texpose_amd.h (_check_f16x3).  In the ray-bias form the two heads over
mlp_trans.2 / mlp_rgb.2 are fp32 dot products: those activations are never fp16 operands, so there the flag stays clear even past
the range, and the result stays accurate."""
import math

import pytest
import torch

from f16_emulation import FP16_RANGE, HIDDEN, emulate_f16, hidden_maxima, rays, rel_l2, rescale
from oracle import texpose_oracle as O

pytestmark = pytest.mark.gpu

# what feeds each hidden output (lifted by 2^c for f16x3); None: it also reads an encoding
SOURCES = {**{"mlp_feat.%d" % i: ("mlp_feat.%d" % (i - 1),) for i in (1, 2, 3, 5, 6, 7)}, "mlp_feat.0": None, "mlp_feat.4": None,
           "mlp_trans.0": ("mlp_feat.7", "lat_trans"), "mlp_trans.1": ("mlp_trans.0",), "mlp_trans.2": ("mlp_trans.1",),
           "mlp_rgb.0": None, "mlp_rgb.1": ("mlp_rgb.0",), "mlp_rgb.2": ("mlp_rgb.1",)}
FP32_HEADS_RB = ("mlp_trans.2", "mlp_rgb.2")     # ray-bias form: read by the fp32 head dot products only
F16X3_WMAX = 2.0 ** 7                            # (half the f16x3 stream's weight range, 2^8)
B, R, N = 1, 3, 128                              # 3 tiles; N % 128 == 0 so that both forms run on the same samples


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def cu(t):
    return t.to(dev())


@pytest.fixture(scope="module")
def ops():
    from texpose_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def base():
    params = O.make_params(61)
    center, ray, depth, pts, unit, lt, ll = rays(7, B, R, N)
    return params, (center, ray, depth, pts, unit, lt, ll), hidden_maxima(params, pts, unit, lt, ll)


def _wide_wmax(params, rb):
    """largest |W| the f16x3 stream carries in fp16 (ray-bias form: without the ray-constant columns of mlp_rgb.0 / mlp_trans.0 and
    the narrow output layers, which go to fp32 tables)"""
    m = 0.0
    for k, v in params.items():
        if not k.endswith(".weight"):
            continue
        if rb and (v.shape[0] < 256 or k == "mlp_feat.7.weight"):
            v = v[1:] if k == "mlp_feat.7.weight" else v[:0]
        if rb and k == "mlp_rgb.0.weight":
            v = torch.cat([v[:, :256], v[:, 283:286]], dim=1)
        if rb and k == "mlp_trans.0.weight":
            v = v[:, :256]
        if v.numel():
            m = max(m, float(v.abs().max()))
    return m


def _plan(params, maxima, layer, target, precision, rb):
    """exponents {name: k} that put `layer`'s largest activation near `target` (f16: 2^k alone; f16x3: with the lift of its sources
    that keeps the stream's weights within F16X3_WMAX, or a smaller k where the sources cannot be lifted)"""
    k = (math.ceil if target > FP16_RANGE else round)(math.log2(target / maxima[layer]))
    if precision == "f16":
        return {layer: k}
    if SOURCES[layer] is None:
        while _wide_wmax(rescale(params, {layer: k}), rb) > F16X3_WMAX:
            k -= 1
        return {layer: k}
    for c in range(0, k + 1):
        ks = {layer: k, **{s: c for s in SOURCES[layer]}}
        if _wide_wmax(rescale(params, ks), rb) <= F16X3_WMAX:
            return ks
    raise AssertionError(("no lift keeps the f16x3 weights in range", layer, k))


def _inputs(inp, ks):
    center, ray, depth, pts, unit, lt, ll = inp
    return center, ray, depth, pts, unit, lt * 2.0 ** ks.get("lat_trans", 0), ll * 2.0 ** ks.get("lat_light", 0)


def _run(ops, params, inp, precision, rb):
    center, ray, depth, pts, unit, lt, ll = inp
    packed = ops.pack_weights({k: cu(v) for k, v in params.items()}, precision=precision, ray_bias=rb)
    return ops.mlp_forward(packed, cu(lt), cu(ll), center=cu(center), ray=cu(ray), depth=cu(depth), precision=precision, ray_bias=rb)


def _check_f16(tag, out, params, inp, rb):
    """the bars of test_f16_kernel_matches_fp16_operand_emulation against the emulation of these (rescaled) weights"""
    _, _, _, pts, unit, lt, ll = inp
    emu = emulate_f16(params, pts, unit, lt, ll, ray_bias=rb)
    exact = emulate_f16(params, pts, unit, lt, ll, ray_bias=rb, rounded=False)
    for a, e, x, name, bar in zip(out, emu, exact, ("rgb", "density", "uncert"), (1e-4, 1e-4, 2e-4)):
        err, budget = rel_l2(a, e), rel_l2(e, x)
        print(tag, name, "rel-L2 vs fp16-operand emulation %.2e (bar %.0e, emulation vs exact arithmetic %.2e)" % (err, bar, budget))
        assert err <= bar and err <= 0.5 * budget, (tag, name, err, bar, budget)


def _check_f16x3(tag, out, params, inp, ks):
    """the fp32-grade bar of test_mlp_f16x3_matches_oracle: rtol 1e-4 / atol 1e-6 against the torch-fp32 oracle and an error
    against the fp64 oracle within 4x of torch-fp32's own -- while every layer's lo halves stay normal fp16 numbers.  A layer
    scaled by 2^k with k > 9 leaves its consumers' weights at 2^-k of their size, k < 0 its activations: their lo halves go
    subnormal and lose bits, and the contract (include/texpose_amd.h) is the rtol / atol bar and 32x torch-fp32's error."""
    _, _, _, pts, unit, lt, ll = inp
    ratio = 4 if all(0 <= k <= 9 for k in ks.values()) else 32
    with torch.no_grad():
        r32 = O.mlp_forward(params, pts, unit, lt, ll)
    r64 = emulate_f16(params, pts, unit, lt, ll, rounded=False)
    for a, f, x, name in zip(out, r32, r64, ("rgb", "density", "uncert")):
        e16, e32 = rel_l2(a, x), rel_l2(f, x)
        print(tag, name, "rel-L2 vs fp64 oracle %.2e (bar %d x torch-fp32's %.2e + 1e-7)" % (e16, ratio, e32))
        torch.testing.assert_close(a.cpu(), f, rtol=1e-4, atol=1e-6)
        assert e16 < ratio * e32 + 1e-7, (tag, name, e16, e32)


def _act_max_bounds(precision, acts, rb):
    """(lo, hi) for take_activation_max: the largest activation the kernel converts to fp16 (ray-bias form: not those of
    FP32_HEADS_RB).  f16x3: the guard sees the hi half, truncated to 11 bits (2^-10 below at most), above only by fp32 rounding;
    f16: within one fp16 step of the emulated maximum (round to nearest even; the narrow heads truncate)"""
    m = max(v for k, v in acts.items() if not (rb and k in FP32_HEADS_RB))
    if precision == "f16x3":
        return m * (1 - 2.0 ** -10) * (1 - 1e-5), m * (1 + 1e-5)
    step = 2.0 ** (math.floor(math.log2(m)) - 10)
    return m - step, m + step


def _take_act_max(ops):
    got = ops.take_activation_max(dev())
    assert ops.take_activation_max(dev()) == 0.0, "take_activation_max must clear the word"
    return got


# ------------------------------------------------------------------------------------------ 3. range guard per layer
@pytest.mark.parametrize("rb", [False, True], ids=["plain", "ray_bias"])
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
@pytest.mark.parametrize("layer", HIDDEN)
def test_range_guard_per_layer(ops, base, layer, precision, rb):
    params, inp, maxima = base
    ops.mlp_status(dev()).zero_()
    ops.take_activation_max(dev())
    fp32_head = rb and layer in FP32_HEADS_RB
    # inside: about half the range; the flag stays clear, the accuracy bar holds, act_max finds this layer's maximum
    ks = _plan(params, maxima, layer, 0.5 * FP16_RANGE, precision, rb)
    p_in, i_in = rescale(params, ks), _inputs(inp, ks)
    acts = {}
    if precision == "f16":
        emulate_f16(p_in, i_in[3], i_in[4], i_in[5], i_in[6], ray_bias=rb, acts=acts)
    else:
        acts = hidden_maxima(p_in, i_in[3], i_in[4], i_in[5], i_in[6])
    tag = "%s %s %s inside %s: max activation %.4g" % (layer, precision, "ray bias" if rb else "plain", ks, acts[layer])
    assert max(acts, key=acts.get) == layer and acts[layer] < 0.75 * FP16_RANGE, (tag, acts)
    if ks[layer] == round(math.log2(0.5 * FP16_RANGE / maxima[layer])):
        assert acts[layer] > 0.25 * FP16_RANGE, tag
    ops.track_activation_max(True)
    try:
        out = _run(ops, p_in, i_in, precision, rb)
        got = _take_act_max(ops)
    finally:
        ops.track_activation_max(False)
    assert ops.take_mlp_status(dev()) == 0, (tag, "flag raised inside the range")
    if precision == "f16":
        _check_f16(tag, out, p_in, i_in, rb)
    else:
        _check_f16x3(tag, out, p_in, i_in, ks)
    lo, hi = _act_max_bounds(precision, acts, rb)
    print(tag, "act_max %.6g in [%.6g, %.6g]" % (got, lo, hi))
    assert lo <= got <= hi, (tag, got, lo, hi)

    # outside: about 1.5x the range
    if precision == "f16x3" and SOURCES[layer] is None:
        return                      # (beyond the f16x3 stream's weight range: see the module docstring)
    ks = _plan(params, maxima, layer, 1.5 * FP16_RANGE, precision, rb)
    p_out, i_out = rescale(params, ks), _inputs(inp, ks)
    m = hidden_maxima(p_out, i_out[3], i_out[4], i_out[5], i_out[6])
    assert m[layer] > FP16_RANGE and max(v for k, v in m.items() if k != layer) < 0.1 * FP16_RANGE, (layer, ks, m)
    out = _run(ops, p_out, i_out, precision, rb)
    if fp32_head:
        assert ops.take_mlp_status(dev()) == 0, (layer, "the fp32 heads of the ray-bias form read no fp16 operand")
        tag = "%s %s ray bias outside %s" % (layer, precision, ks)
        if precision == "f16":
            _check_f16(tag, out, p_out, i_out, rb)
        else:
            _check_f16x3(tag, out, p_out, i_out, ks)
        return
    with pytest.raises(Exception, match="fp16 range"):
        ops.check_mlp_status(dev())
    ops.check_mlp_status(dev())                                  # the report cleared the flag


@pytest.mark.parametrize("layer", ["mlp_feat.2", "mlp_trans.1", "mlp_rgb.0"])
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_range_guard_scaled_down_layer(ops, base, layer, precision):
    """k < 0: one layer's activations at 2^-6 of their size (small fp16 operands, subnormal lo halves); the inside bars hold"""
    params, inp, _ = base
    ops.mlp_status(dev()).zero_()
    p = rescale(params, {layer: -6})
    for rb in (False, True):
        out = _run(ops, p, inp, precision, rb)
        assert ops.take_mlp_status(dev()) == 0
        tag = "%s %s %s scaled by 2^-6" % (layer, precision, "ray bias" if rb else "plain")
        if precision == "f16":
            _check_f16(tag, out, p, inp, rb)
        else:
            _check_f16x3(tag, out, p, inp, {layer: -6})


@pytest.mark.parametrize("rb", [False, True], ids=["plain", "ray_bias"])
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_range_guard_one_image_of_three_last_tiles(ops, precision, rb):
    """a light code that drives mlp_rgb.0 past the range in the LAST image of three (its tiles are the last ones of a many-tile
    call; in the ray-bias form the code goes through the per-image pre-kernel): the flag is raised.  The code is aligned with the
    weight row of one feature, so that it stays well inside the fp16 range itself."""
    Bi, Ri, Ni = 3, 340, 128
    params = O.make_params(62)
    center, ray, depth, pts, unit, lt, ll = rays(9, Bi, Ri, Ni)
    packed = ops.pack_weights({k: cu(v) for k, v in params.items()}, precision=precision, ray_bias=rb)
    args = dict(center=cu(center), ray=cu(ray), depth=cu(depth), precision=precision, ray_bias=rb)
    ops.mlp_status(dev()).zero_()
    ops.mlp_forward(packed, cu(lt), cu(ll), **args)
    ops.check_mlp_status(dev())                                  # control: the unmodified codes stay inside
    w = params["mlp_rgb.0.weight"][:, 286:334]
    f = int(w.abs().sum(1).argmax())
    s = 2.0 ** math.ceil(math.log2(2 * FP16_RANGE / float(w[f].abs().sum())))
    assert s <= 2 ** 15, s                                   # (the code itself stays an fp16 number)
    ll_big = ll.clone()
    ll_big[2] = torch.sign(w[f]) * s
    ops.mlp_forward(packed, cu(lt), cu(ll_big), **args)
    with pytest.raises(Exception, match="fp16 range"):
        ops.check_mlp_status(dev())
    ops.check_mlp_status(dev())


@pytest.mark.parametrize("where", ["inside", "outside"])
def test_render_by_slices_f16_per_layer_fallback(ops, base, where):
    """a per-layer rescaled network (mlp_trans.1) through render_by_slices with f16: inside, no fall-back; outside, the image is
    re-rendered with the exact-fp32 kernel and equals the fp32 render bit for bit"""
    import warnings
    from test_gpu_f16_synthesis import _graph
    params = base[0]
    H, W, Ns = 16, 16, 32
    sc = O.synthetic_scene(H, W, B=1, seed=1)
    K = sc["intr"].clone()
    K[:, 0, 0] = K[:, 1, 1] = 700.0 * H / 128.0
    K[:, 0, 2], K[:, 1, 2] = W / 2.0, H / 2.0
    dr = (cu(sc["z_near"])[:, :, None], cu(sc["z_far"])[:, :, None])
    graph, opt = _graph(params, H=H, W=W, N=Ns)
    # the layer's largest activation on the samples this render evaluates (its rays and depths from the HIP ray generation)
    center, ray, _, _, depth = ops.raygen(cu(K), cu(sc["pose"]), H=H, W=W, n_samples=Ns, ray_idx=cu(torch.arange(H * W)[None]),
                                          z_near=dr[0], z_far=dr[1])
    pts = center.cpu()[:, :, None] + ray.cpu()[:, :, None] * depth.cpu()[..., None]
    unit = torch.nn.functional.normalize(ray.cpu(), dim=-1)[:, :, None].expand_as(pts)
    m = hidden_maxima(params, pts, unit, graph.latent_vars_trans.weight.detach().cpu()[:1], graph.latent_vars_light.weight.detach().cpu()[:1])
    k = round(math.log2((0.5 if where == "inside" else 1.5) * FP16_RANGE / m["mlp_trans.1"]))
    graph, opt = _graph(rescale(params, {"mlp_trans.1": k}), H=H, W=W, N=Ns)
    opt.nerf.sample_stratified = False
    graph.eval()
    mask = torch.ones(1, H, W, device=dev())
    ops.mlp_status(dev()).zero_()

    def render(prec):
        graph.nerf.precision = prec
        with torch.no_grad():
            return graph.render_by_slices(opt, cu(sc["pose"]), intr=cu(K), depth_range=dr, object_mask=mask, sample_idx=None, mode="val")

    want = render("fp32")
    graph.range_fallbacks = 0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = render("f16")
    fell_back = any("fp16 range" in str(w_.message) for w_ in caught)
    print("mlp_trans.1 x 2^%d (%s): fall-backs %d" % (k, where, graph.range_fallbacks))
    assert fell_back == (where == "outside") and graph.range_fallbacks == (where == "outside")
    if where == "outside":
        for name in ("rgb", "rgb_static", "depth", "uncert", "density", "alpha_static"):
            assert torch.equal(got[name], want[name]), name
    else:
        assert float((got["rgb"] - want["rgb"]).abs().max()) <= 4e-3
    assert int(ops.mlp_status(dev()).item()) == 0


# ------------------------------------------------------------------------------------------ 4. act_max
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
@pytest.mark.parametrize("shape", [(1, 3, 128), (3, 13, 33)], ids=["plain_call", "ragged_tail"])
def test_activation_max_matches_reference(ops, precision, shape):
    """take_activation_max after one call: the largest hidden activation (f16x3: of the fp64 oracle, f16: of the emulation), and
    the take clears the word; without tracking nothing is folded in"""
    Bs, Rs, Ns = shape
    params = O.make_params(63)
    center, ray, depth, pts, unit, lt, ll = rays(11, Bs, Rs, Ns)
    acts = {}
    if precision == "f16":
        emulate_f16(params, pts, unit, lt, ll, acts=acts)
    else:
        acts = hidden_maxima(params, pts, unit, lt, ll)
    ops.mlp_status(dev()).zero_()
    ops.take_activation_max(dev())
    ops.track_activation_max(True)
    try:
        _run(ops, params, (center, ray, depth, pts, unit, lt, ll), precision, False)
        got = _take_act_max(ops)
    finally:
        ops.track_activation_max(False)
    _run(ops, params, (center, ray, depth, pts, unit, lt, ll), precision, False)
    assert ops.take_activation_max(dev()) == 0.0, "an untracked call folded its maximum in"
    ops.check_mlp_status(dev())
    lo, hi = _act_max_bounds(precision, acts, False)
    print(precision, shape, "act_max %.6g in [%.6g, %.6g] (largest at %s)" % (got, lo, hi, max(acts, key=acts.get)))
    assert lo <= got <= hi, (got, lo, hi)
