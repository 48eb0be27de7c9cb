"""GPU: the small kernels that end every training iteration -- K8 csrc/nerf_losses.hip, K10 csrc/rmsprop.hip and the K13 pieces of
csrc/train_misc.hip (BCE terms, feature-pair loss, R1 value, max-pool, the input stacks, latent rows, the weighted sum with the step
gate, tp_step_inputs, tp_grad_pack, fused Adam) -- against their fp64 restatements (tests/step_ref.py) at the sizes that sit on their
constants: the 256- and 1024-thread blocks and the 64-lane butterflies of `block_total`, the grid caps (256 x 4 Adam, 4096 RMSprop, 1024
grad_pack / sumsq_mean_fwd_bwd / K8, 2048 step_inputs), the table sizes (32 / 16 / 32 / 24) with the wrappers' chunking behind them,
Adam's binary search over its LDS table and the last-block hand-overs of K8 and Adam.  Called through texpose_amd.ops, autograd_ops and
the two fused optimisers only.

How accuracy is judged (no tolerance of this file's own):
  * elementwise outputs (gradients, maps, parameters, moments, packed buffers): the project's fp32 rule e_k <= 2 e_t + floor
    (`within_rule` of tests/test_gpu_lab_loss.py), e_t the error of the SAME restatement evaluated by torch in float32 on the CPU -- for
    the optimisers stock torch.optim.RMSprop / Adam in float32 on the CPU -- never the code under test;
  * pure data movement / selection (disc_inputs, latent_rows forward, maxpool2 value and argmax and gradient, the fake_patch cotangent,
    step_inputs): bit-equal to the fp64 restatement rounded to float32.  feat_inputs forward ends in (v - mean) / std, two fp32
    roundings that one rounding of the fp64 result cannot reproduce: it is bit-equal to the restatement evaluated in float32 (what
    test_feat_and_disc_input_kernels_match_torch asserts with torch.equal), and meets the rule against fp64;
  * scalar sums (loss values, K8's four sums, sumsq_mean, weighted_sum): |err| <= (h + c) 2^-24 sum |t_i| (`sum_rule`), sum |t_i| in
    fp64, h the longest addition chain of the kernel's code, c the fp32 roundings in one term (expf, log1pf, logf count 2), both written
    next to each case with the source line they were read from.  Roundings applied to the finished sum (the division of a mean, K8's
    `5 +`) are `final` roundings of the value itself.

Largest e_k / e_t per kernel on the MI355X (printed behind the last test), and the largest |err| / bound of the scalar sums:
    bce_bwd 1.014   gan_disc_losses 1.014   feat_pair_bwd 1.000   sumsq_bwd 1.000   sumsq_fwd_bwd 1.000   nerf_losses_bwd 4.322
    feat_inputs 1.000   feat_inputs_bwd 1.000   latent_rows_bwd 1.000   grad_pack 1.000   rmsprop 1.331   adam 1.510
    sums: bce_fwd 0.080   gan_disc_losses 0.080   feat_pair_loss 0.125   sumsq_mean 0.070   sumsq_fwd_bwd 0.095   nerf_losses 0.533
          weighted_sum 0.291
nerf_losses_bwd's 4.322 (g_rgb, B1 P256 N1, all-ones mask, spiked pixels left out) is an error of 0.9 fp32 spacings of the largest value
where torch's own is 0.2 of one -- the floor's case; every other ratio above 2 there is of the same kind.
"""
import functools
import math

import numpy as np
import pytest
import torch

import step_ref as R
from test_gpu_lab_loss import within_rule

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MAX_RATIO = {}                               # kernel -> largest e_k / e_t seen (printed; the docstring quotes it)
MAX_BOUND = {}                               # kernel -> largest |err| / bound of its scalar sums


@pytest.fixture(scope="module")
def ops():
    from texpose_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def aops():
    from texpose_amd import autograd_ops
    return autograd_ops


@pytest.fixture(scope="module", autouse=True)
def _print_largest_ratios():
    yield
    for k in sorted(MAX_RATIO):
        print("largest e_k / e_t of %-16s %s" % (k, "%.3f" % MAX_RATIO[k] if math.isfinite(MAX_RATIO[k]) else "inf (e_t = 0)"))
    for k in sorted(MAX_BOUND):
        print("largest |err| / bound of %-16s %.3f" % (k, MAX_BOUND[k]))


def cu(a, dtype=None):
    x = R.t(a) if isinstance(a, np.ndarray) else a
    return x.to(DEV) if dtype is None else x.to(DEV, dtype)


def f64(a):
    return R.t(a).double()


def f32(a):
    return R.t(a).float()


def rule(name, got, want, torch32):
    """`within_rule`, and the largest e_k / e_t per kernel (the part of `name` before the first blank)."""
    g, w, t = (x.detach().double().cpu().reshape(-1) for x in (got, want, torch32))
    e_k, e_t = float((g - w).abs().max()), float((t - w).abs().max())
    key = name.split(" ")[0]
    MAX_RATIO[key] = max(MAX_RATIO.get(key, 0.0), e_k / e_t if e_t > 0 else (0.0 if e_k == 0 else float("inf")))
    within_rule(name, g, w, t)


def rule_rest(name, got, want, torch32, spikes, per=1):
    """`rule` on the whole output and again without the spiked elements (`per` values each): the floor is one fp32 spacing of the
    LARGEST reference value, which the spikes would otherwise set for every ordinary element."""
    rule(name, got, want, torch32)
    g, w, t = (x.detach().cpu().reshape(-1, per) for x in (got, want, torch32))
    keep = torch.ones(g.shape[0], dtype=torch.bool)
    keep[list(spikes)] = False
    if bool(keep.any()):
        rule(name + " rest", g[keep], w[keep], t[keep])


def sum_rule(name, got, want, h, c, abs_sum, final=0):
    """|got - want| <= (h + c) 2^-24 sum |t_i| + final 2^-24 |want|; prints the figures first."""
    got, want = float(got.detach()), float(want)
    assert math.isfinite(got) and math.isfinite(want), (name, got, want)
    e_k, bound = abs(got - want), R.sum_bound(h, c, abs_sum) + final * R.U32 * abs(want)
    print("%-44s e_k %.3e  bound %.3e  (h %d, c %d, final %d)" % (name, e_k, bound, h, c, final))
    key = name.split(" ")[0]
    MAX_BOUND[key] = max(MAX_BOUND.get(key, 0.0), e_k / bound if bound > 0 else (0.0 if e_k == 0 else float("inf")))
    assert e_k <= bound, (name, got, want, e_k, bound)


def bits(x):
    """The tensor's bit patterns (NaNs and the sign of zero compare as what they are)."""
    x = x.detach().contiguous().cpu()
    return x.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[x.element_size()]) if x.is_floating_point() else x


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def poison(*shapes):
    """NaN-filled blocks of the given shapes, handed back to the caching allocator: the wrappers' next torch.empty of these sizes
    gets them, so an output element the kernel does not write shows as NaN."""
    blocks = [torch.full(s, float("nan"), device=DEV) for s in shapes]
    torch.cuda.synchronize()
    del blocks


# ------------------------------------------------------------------------------------------ BCE terms
# bce_logits_fwd_kernel / gan_disc_losses_kernel (train_misc.hip:48-58, 411-430), one workgroup of 256 threads:
#   h = ceil(n / 256) adds per thread (:51, :420) + 6 butterfly steps (:26) + 3 wavefront sums (:31)
#   c = expf 2 + log1pf 2 + the subtraction inside ls 1 + (1 - t) v 1 + the outer subtraction 1 = 7 (:53-54);  final = 1: tot / n (:57)
BCE_SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 5001)
BCE_C = 7


def bce_h(n):
    return -(-n // 256) + 6 + 3


def check_bce_value(name, got, x, target):
    x64 = f64(x)
    sum_rule(name, got, R.bce_logits_mean(x64, target), bce_h(x.size), BCE_C, R.bce_terms(x64, target).abs().sum() / x.size, final=1)


def check_bce_grad(name, got, x, target, w):
    w32 = torch.tensor(w, dtype=torch.float32)
    rule(name, got, R.bce_logits_grad(f64(x), target, w32.double()), R.bce_logits_grad(f32(x), target, w32))


@pytest.mark.parametrize("target", [0.0, 1.0])
@pytest.mark.parametrize("n", BCE_SIZES + ("extreme13", "extreme257"))
def test_bce_logits_mean_forward_and_backward(aops, n, target):
    """Value by the summation bound, gradient (upstream weight 1.3 / 0.9) by the rule; the extreme logits {0, +-1e-8, +-20, +-87, +-89,
    +-104, +-1e4} give a finite loss and finite gradients."""
    extreme = isinstance(n, str)
    x = R.logits_case(int(n[7:]) if extreme else n, target, extreme)
    w = 1.3 if target == 0.0 else 0.9
    xd = cu(x).requires_grad_()
    loss = aops.bce_logits_mean(xd, target)
    (gx,) = torch.autograd.grad(loss * w, xd)
    assert loss.shape == () and gx.shape == xd.shape and torch.isfinite(gx).all() and torch.isfinite(loss)
    tag = "n %s target %d" % (n, target)
    check_bce_value("bce_fwd " + tag, loss, x, target)
    check_bce_grad("bce_bwd " + tag, gx, x, target, w)


@pytest.mark.parametrize("n", BCE_SIZES + ("extreme13",))
def test_gan_disc_losses_equals_the_two_single_term_launches(ops, n):
    """Both values by the bound, both weighted cotangents by the rule, and all four bit-equal to the single-term launches."""
    extreme = isinstance(n, str)
    xr, xf = (R.logits_case(int(n[7:]) if extreme else n, t, extreme) for t in (1.0, 0.0))
    dr, df = cu(xr), cu(xf)
    out2, gr, gf = ops.gan_disc_losses(dr, df, 0.9, 1.3)
    check_bce_value("gan_disc_losses real n %s" % (n,), out2[0], xr, 1.0)
    check_bce_value("gan_disc_losses fake n %s" % (n,), out2[1], xf, 0.0)
    check_bce_grad("gan_disc_losses g_real n %s" % (n,), gr, xr, 1.0, 0.9)
    check_bce_grad("gan_disc_losses g_fake n %s" % (n,), gf, xf, 0.0, 1.3)
    assert same_bits(out2[0], ops.bce_logits_fwd(dr, 1.0)) and same_bits(out2[1], ops.bce_logits_fwd(df, 0.0))
    assert same_bits(gr, ops.bce_logits_bwd(dr, 1.0, torch.tensor(0.9, device=DEV)))
    assert same_bits(gf, ops.bce_logits_bwd(df, 0.0, torch.tensor(1.3, device=DEV)))
    o_r, o_f = torch.full_like(dr, float("nan")), torch.full_like(df, float("nan"))                 # the out= form writes every element
    ops.gan_disc_losses(dr, df, 0.9, 1.3, g_real_out=o_r, g_fake_out=o_f)
    assert same_bits(o_r, gr) and same_bits(o_f, gf)


# ------------------------------------------------------------------------------------------ feature-pair loss
# feat_pair_loss_fwd_kernel (train_misc.hip:305-323), one workgroup of 1024 threads:
#   h = ceil(n / 1024) adds per thread (:308-311) + the 10 levels of the 1024-wide tree (:315)
#   c = subtraction 1 + square 1 = 2 (:309-310);  final: parts 1 (/ n, :320), loss 3 (/ n, w2 *, +, :320-321)
FEAT_SIZES = (1, 1023, 1024, 1025, 2 * 1024 + 1, 16384)


@pytest.mark.parametrize("n", FEAT_SIZES)
def test_feat_pair_loss_value_parts_and_gradient(aops, n):
    f = R.feat_case(n)
    fd = cu(f).requires_grad_()
    loss, parts = aops.feat_pair_loss(fd, 5.0)
    g = torch.tensor(0.7, device=DEV)
    (gf,) = torch.autograd.grad(loss * g, fd)
    f64_, h = f64(f), -(-n // 1024) + 10
    want = R.feat_pair_loss(f64_, 5.0)
    t1, t2 = ((f64_[0] - f64_[2]) ** 2).sum() / n, ((f64_[1] - f64_[3]) ** 2).sum() / n
    sum_rule("feat_pair_loss value n %d" % n, loss, want[0], h, 2, t1 + 5.0 * t2, final=3)
    sum_rule("feat_pair_loss l1 n %d" % n, parts[0], want[1], h, 2, t1, final=1)
    sum_rule("feat_pair_loss l2 n %d" % n, parts[1], want[2], h, 2, t2, final=1)
    assert not parts.requires_grad
    w64, w32 = R.feat_pair_loss_grad(f64_, 5.0, g.cpu().double()), R.feat_pair_loss_grad(f32(f), 5.0, g.cpu())
    spikes = R.spike_indices(n, 1024)
    rule_rest("feat_pair_bwd fake1 n %d" % n, gf[0], w64[0], w32[0], spikes)
    rule_rest("feat_pair_bwd fake2 n %d" % n, gf[1], w64[1], w32[1], spikes)
    assert not bits(gf[2:]).any()                                                            # the real quarters: exact (+)zeros


# ------------------------------------------------------------------------------------------ R1 value
# sumsq_mean_fwd_kernel / sumsq_mean_fwd_bwd_kernel block 0 (train_misc.hip:347-353, 396-406), one workgroup of 1024 threads:
#   h = ceil(n / 1024) adds per thread (:350, :403) + 6 butterfly steps (:26) + 15 wavefront sums (:31)
#   c = the square 1 (:350);  final = 1: tot / B (:352), and 1 more for the weighted value w * out[0] (:405)
SUMSQ_SIZES = (1, 1023, 1024, 1025, 9 * 16 * 16 * 4, 1024 * 1024 + 3)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", SUMSQ_SIZES)
def test_sumsq_mean_forward_backward_and_fused(ops, aops, n, B):
    """g [B, n] (B n elements flat: B = 1 sits on the constants, B = 3 runs the fused form's grid-stride loop up to four rounds)."""
    x = R.sumsq_case(n, B)
    xd = cu(x).requires_grad_()
    val = aops.sumsq_mean(xd)
    cot = torch.tensor(0.8, device=DEV)
    (gx,) = torch.autograd.grad(val * cot, xd)
    x64, h = f64(x), -(-B * n // 1024) + 6 + 15
    abs_sum = (x64 * x64).sum() / B
    tag = "n %d B %d" % (n, B)
    sum_rule("sumsq_mean " + tag, val, R.sumsq_mean(x64), h, 1, abs_sum, final=1)
    spikes = R.spike_indices(B * n, 1024)
    rule_rest("sumsq_bwd " + tag, gx, R.sumsq_mean_grad(x64, cot.cpu().double()), R.sumsq_mean_grad(f32(x), cot.cpu()), spikes)
    w = 0.35
    out_g = torch.full_like(xd.detach(), float("nan"))
    out, og = ops.sumsq_mean_fwd_bwd(xd.detach(), w, out_g=out_g)
    assert og.data_ptr() == out_g.data_ptr() and same_bits(out[0], val)                       # the fused value IS the single forward's
    w32 = torch.tensor(w, dtype=torch.float32)
    sum_rule("sumsq_fwd_bwd weighted " + tag, out[1], R.sumsq_mean(x64) * w32.double(), h, 1, abs_sum * float(w32), final=2)
    rule_rest("sumsq_fwd_bwd " + tag, og, R.sumsq_mean_fwd_bwd(x64, w32.double())[1], R.sumsq_mean_fwd_bwd(f32(x), w32)[1], spikes)


# ------------------------------------------------------------------------------------------ K8
# nerf_losses_fwd_kernel (nerf_losses.hip:66-101), grid = min(ceil(B P N / 256), 1024) workgroups of 256 threads (:165-169):
#   h = ceil(n / (grid 256)) adds per thread (pixels :72-85, density :87) + the 8 levels of the 256-wide tree (:20)
#       + the second stage, ceil(grid / 256) adds per thread (:36) + its 8 levels (:43) (in double: counted all the same)
#   c: sum 0: per channel subtraction 1 + square 1, the two adds of se, u * u, the division, m * = 7 (:79-82); sum 1: 0 (:83);
#      sum 2: u * u 1 + logf 2 = 3 (:84); sum 3: 0 (:87)
#   losses (:52-55): render = float(s0) / (float(s1) + 1e-5): final 3;  uncert = 5 + float(s2) / n / 2: the sum's bound halved and
#   divided by n with 2 more roundings in c, final 1 (the `5 +`);  trans_reg = float(s3) / n: final 2
NERF_SHAPES = ((1, 1, 1), (1, 255, 1), (1, 256, 1), (1, 257, 1), (1, 256, 256), (1, 257, 256), (1, 1024, 256), (2, 513, 256))


def nerf_grid(B, P, N):
    return max(1, min(-(-B * P * N // 256), 1024))


@functools.lru_cache(maxsize=None)
def nerf_ref(B, P, N, kind):
    """fp64 and fp32 restatements of one K8 case: shared, never written to."""
    c = R.nerf_case(B, P, N, kind)
    a64 = [f64(c[k]) for k in ("rgb", "uncert", "density", "gathered")]
    a32 = [f32(c[k]) for k in ("rgb", "uncert", "density", "gathered")]
    g32 = f32(c["g"])
    return dict(terms=[x.abs().sum() for x in R.nerf_terms(*a64)], fwd=R.nerf_losses(*a64),
                bwd64=R.nerf_losses_grad(*a64, tuple(g32.double())), bwd32=R.nerf_losses_grad(*a32, tuple(g32)))


@pytest.mark.parametrize("kind", R.MASK_KINDS)
@pytest.mark.parametrize("B, P, N", NERF_SHAPES)
def test_nerf_losses_forward_and_backward(ops, aops, B, P, N, kind):
    c, ref = R.nerf_case(B, P, N, kind), nerf_ref(B, P, N, kind)
    rgb, unc, den, gat = (cu(c[k]) for k in ("rgb", "uncert", "density", "gathered"))
    g = cu(c["g"])
    sums, losses = ops.nerf_losses_fwd(rgb, unc, den, gat, want_losses=True)
    sums_b, losses_b = ops.nerf_losses_fwd(rgb, unc, den, gat, want_losses=True)              # back to back: the ticket was reset
    assert same_bits(sums, sums_b) and same_bits(losses, losses_b) and sums.dtype == torch.float64
    assert same_bits(ops.nerf_losses_fwd(rgb, unc, den, gat), sums)
    grid, n_pix, n_den = nerf_grid(B, P, N), B * P, B * P * N
    second = -(-grid // 256) + 8
    h_pix, h_den = -(-n_pix // (grid * 256)) + 8 + second, -(-n_den // (grid * 256)) + 8 + second
    tag = "B%d P%d N%d %s" % (B, P, N, kind)
    want_s, want_l = ref["fwd"]
    for k, (h, cc) in enumerate(((h_pix, 7), (h_pix, 0), (h_pix, 3), (h_den, 0))):
        sum_rule("nerf_losses sum%d %s" % (k, tag), sums[k], want_s[k], h, cc, ref["terms"][k])
    sum_rule("nerf_losses render " + tag, losses[0], want_l[0], h_pix, 7, ref["terms"][0] / (want_s[1] + 1e-5), final=3)
    sum_rule("nerf_losses uncert " + tag, losses[1], want_l[1], h_pix, 3 + 2, ref["terms"][2] / (2 * n_pix), final=1)
    sum_rule("nerf_losses trans_reg " + tag, losses[2], want_l[2], h_den, 0, ref["terms"][3] / n_den, final=2)
    if kind == "zeros":
        assert float(losses[0]) == 0.0 and float(sums[0]) == 0.0 and float(sums[1]) == 0.0
    grads = ops.nerf_losses_bwd(rgb, unc, den, gat, sums, g)
    rule_rest("nerf_losses_bwd g_rgb " + tag, grads[0], ref["bwd64"][0], ref["bwd32"][0], c["spikes"], per=3)
    rule_rest("nerf_losses_bwd g_uncert " + tag, grads[1], ref["bwd64"][1], ref["bwd32"][1], c["spikes"])
    rule("nerf_losses_bwd g_density " + tag, grads[2], ref["bwd64"][2], ref["bwd32"][2])
    assert not bits(grads[2][..., 0]).any()
    # the autograd form: the same launches
    r, u, d = rgb.clone().requires_grad_(), unc.clone().requires_grad_(), den.clone().requires_grad_()
    out = aops.nerf_losses(r, u, d, gat)
    assert all(same_bits(out[k], losses[k]) for k in range(3))
    got = torch.autograd.grad(out[0] * g[0] + out[1] * g[1] + out[2] * g[2], (r, u, d))
    assert got[1].shape == unc.shape
    assert all(same_bits(a.reshape(-1), b.reshape(-1)) for a, b in zip(got, grads))


# ------------------------------------------------------------------------------------------ MaxPool2d(2, 2)
POOL_CASES = [(1, 2, 2, "relu"), (3, 2, 6, "relu"), (5, 8, 12, "relu"), (2, 4, 130, "relu"), (7, 6, 2, "relu"), (5, 8, 12, "special")]


@pytest.mark.parametrize("n, H, W, values", POOL_CASES)
def test_maxpool2_value_argmax_and_gradient_are_bit_equal(ops, aops, n, H, W, values):
    c = R.pool_case(n, H, W, values)
    y_ref, arg_ref = R.maxpool2(f64(c["x"]))
    gx_ref = R.maxpool2_grad(f64(c["gy"]), arg_ref).float()
    xd, gy = cu(c["x"]).reshape(1, n, H, W), cu(c["gy"]).reshape(1, n, H // 2, W // 2)
    y, arg = ops.maxpool2_fwd(xd)
    assert same_bits(y[0], y_ref.float()) and arg.dtype == torch.uint8 and torch.equal(arg[0].cpu(), arg_ref)
    poison((1, n, H, W))
    gx = ops.maxpool2_bwd(gy, arg)                                                           # writes all four inputs of every window
    assert same_bits(gx[0], gx_ref)
    xg = xd.clone().requires_grad_()
    ya = aops.maxpool2(xg)
    poison((1, n, H, W))
    (ga,) = torch.autograd.grad(ya, xg, grad_outputs=gy)
    assert same_bits(ya, y) and same_bits(ga[0], gx_ref)


# ------------------------------------------------------------------------------------------ input stacks
STACK_SHAPES = ((1, 1, 1), (1, 1, 255), (2, 16, 16), (3, 3, 86))


@pytest.mark.parametrize("B, h, w", STACK_SHAPES)
def test_feat_inputs_forward_and_gradient(aops, B, h, w):
    c = R.stack_case(B, h, w)
    rgb, gat, cot = cu(c["rgb"]).requires_grad_(), cu(c["gathered"]), cu(c["cot"])
    x = aops.feat_inputs(rgb, gat, [float(np.float32(v)) for v in R.MEAN], [float(np.float32(v)) for v in R.STD], (h, w))
    (g,) = torch.autograd.grad(x, rgb, grad_outputs=cot)
    x64, x32 = R.feat_inputs(f64(c["rgb"]), f64(c["gathered"])), R.feat_inputs(f32(c["rgb"]), f32(c["gathered"]))
    assert same_bits(x, x32)                                              # every operation correctly rounded, in the model's order
    rule("feat_inputs B%d %dx%d" % (B, h, w), x, x64, x32)
    rule("feat_inputs_bwd B%d %dx%d" % (B, h, w), g, R.feat_inputs_grad(f64(c["rgb"]), f64(c["gathered"]), f64(c["cot"])),
         R.feat_inputs_grad(f32(c["rgb"]), f32(c["gathered"]), f32(c["cot"])))


@pytest.mark.parametrize("geo", [True, False])
@pytest.mark.parametrize("B, h, w", STACK_SHAPES)
def test_disc_inputs_and_the_fake_patch_cotangent_are_bit_equal(ops, aops, B, h, w, geo):
    c = R.stack_case(B, h, w)
    rgb, gat = cu(c["rgb"]), cu(c["gathered"])
    real64, fake64 = R.disc_inputs(f64(c["rgb"]), f64(c["gathered"]), geo)
    real, fake = ops.disc_inputs(rgb, gat, (h, w), geo)
    assert same_bits(real, real64.float()) and same_bits(fake, fake64.float())
    stack, fake2 = ops.disc_inputs(rgb, gat, (h, w), geo, stacked=True)
    assert stack.shape[0] == 2 * B and same_bits(stack[:B], real) and same_bits(fake2, fake)
    r = rgb.clone().requires_grad_()
    real_a, fake_a, stack_a = aops.disc_patches(r, gat, (h, w), geo)
    assert same_bits(real_a, real) and same_bits(fake_a, fake) and not stack_a.requires_grad
    cot = c["cot_fake"][:, :9 if geo else 3]
    poison((B, h * w, 3))
    (g,) = torch.autograd.grad(fake_a, r, grad_outputs=cu(np.ascontiguousarray(cot)))
    assert same_bits(g, R.fake_patch_grad(f64(np.ascontiguousarray(cot))).float())


# ------------------------------------------------------------------------------------------ latent rows
@pytest.mark.parametrize("idx_dtype", [torch.int64, torch.int32])
def test_latent_rows_forward_and_dense_gradient(aops, idx_dtype):
    """B = 5 with a repeated row and rows never hit, n_rows (Ct + Cl) = 270 > 256: two workgroups in the backward."""
    c = R.latent_case(5, 9, 17, 13)
    wt, wl = cu(c["w_trans"]).requires_grad_(), cu(c["w_light"]).requires_grad_()
    idx_cpu = R.t(c["idx"])
    never = sorted(set(range(9)) - set(idx_cpu.tolist()))
    assert never and len(set(idx_cpu.tolist())) < 5 and 9 * (17 + 13) > 256
    poison((5, 17), (5, 13))
    ot, ol = aops.latent_rows(wt, wl, idx_cpu.to(DEV, idx_dtype))
    ot64, ol64 = R.latent_rows(f64(c["w_trans"]), f64(c["w_light"]), idx_cpu)
    assert same_bits(ot, ot64.float()) and same_bits(ol, ol64.float())
    poison((9, 17), (9, 13))
    gwt, gwl = torch.autograd.grad([ot, ol], [wt, wl], grad_outputs=[cu(c["g_trans"]), cu(c["g_light"])])
    w64 = R.latent_rows_grad(f64(c["g_trans"]), f64(c["g_light"]), idx_cpu, 9)
    w32 = R.latent_rows_grad(f32(c["g_trans"]), f32(c["g_light"]), idx_cpu, 9)
    rule("latent_rows_bwd trans %s" % idx_dtype, gwt, w64[0], w32[0])
    rule("latent_rows_bwd light %s" % idx_dtype, gwl, w64[1], w32[1])
    assert not bits(gwt[never]).any() and not bits(gwl[never]).any()                          # exact zeros, no fill before the launch


# ------------------------------------------------------------------------------------------ weighted sum + step gate
# weighted_sum_kernel / weighted_sum_flags_kernel (train_misc.hip:434-452): one thread, h = n adds (:437, :447), c = 1: t_k * w_k
@pytest.mark.parametrize("n", [1, 2, 16])
def test_weighted_sum_and_its_gate_words(ops, n):
    terms, weights = R.terms_case(n)
    td = [cu(terms)[k] for k in range(n)]
    ws = [float(w) for w in weights]
    want = R.weighted_sum(list(f64(terms)), ws)
    abs_sum = (f64(terms) * f64(weights)).abs().sum()
    sum_rule("weighted_sum n %d" % n, ops.weighted_sum(td, ws), want, n, 1, abs_sum)
    n_bad, word_status, word_finite = 4, 1, 2
    bad, snap = torch.zeros(n_bad, dtype=torch.int32, device=DEV), torch.full((n_bad,), -1, dtype=torch.int32, device=DEV)
    status, counter = torch.zeros(1, dtype=torch.int32, device=DEV), torch.tensor([41], dtype=torch.int64, device=DEV)
    flags = dict(bad=bad, snapshot=snap, word_finite=word_finite, status=status, word_status=word_status, step_counter=counter)
    total = ops.weighted_sum(td, ws, flags=flags)
    sum_rule("weighted_sum flags n %d" % n, total, want, n, 1, abs_sum)
    assert bad.tolist() == [0, 0, 0, 0] and snap.tolist() == [0, 0, 0, 0] and counter.item() == 42
    bad[3] = 7                                                                               # a word already set stays as it is
    expect, count = [0, 0, 0, 7], 42
    # (poisoned last term, status word, start again from clear words): +-inf and NaN totals each set word_finite, a set status sets
    # word_status, and a clean step on top of set words leaves them set
    for poisoned, st, reset in ((float("inf"), 0, True), (None, 1, True), (float("-inf"), 0, False), (None, 0, False),
                                (float("nan"), 0, True), (None, 0, True)):
        if reset:
            bad.copy_(torch.tensor([0, 0, 0, 7], dtype=torch.int32))
            expect = [0, 0, 0, 7]
        tt = list(td)
        if poisoned is not None:
            tt[n - 1] = torch.tensor(poisoned, device=DEV)
            expect[word_finite] = 1
        status.fill_(st)
        if st:
            expect[word_status] = 1
        total = ops.weighted_sum(tt, ws, flags=flags)
        count += 1
        assert bad.tolist() == expect and snap.tolist() == expect and counter.item() == count, (poisoned, st, reset)
        if poisoned is None:
            assert same_bits(total, ops.weighted_sum(td, ws))


# ------------------------------------------------------------------------------------------ grad_pack
PACK_NUMELS = (1, 3, 255, 256, 1025)
PACK_TABLES = {
    "1": [1025],
    "32": [None if k in (0, 13, 31) else PACK_NUMELS[k % 5] for k in range(32)],
    "33": [None if k in (0, 17, 32) else PACK_NUMELS[k % 5] for k in range(33)],               # two launches
    "second_round": [1024 * 256 * 2, None, 1024 * 256 * 2 - 3],                                # total 1024 256 4 + 5 with the None's 8
}


@pytest.mark.parametrize("table", sorted(PACK_TABLES))
def test_grad_pack_scales_concatenates_and_keeps_a_sticky_tail(ops, table):
    spec = PACK_TABLES[table]
    rs = np.random.RandomState(len(spec))
    grads_cpu = [(None, 8 if table == "second_round" else 5) if n is None else torch.from_numpy(rs.normal(size=n).astype(np.float32)) for n in spec]
    total = sum(g[1] if isinstance(g, tuple) else g.numel() for g in grads_cpu)
    assert table != "second_round" or total == 1024 * 256 * 4 + 5
    scale, n_words = 1.0 / 3.0, 3
    flat = torch.full((total + n_words + 4,), -77.0, device=DEV)
    tail = flat[total:total + n_words]
    tail.copy_(torch.tensor([0.0, 0.0, 2.0]))                                                 # a word left set by an earlier step
    words = torch.tensor([0, 5, 0], dtype=torch.int32, device=DEV)
    grads_dev = [g if isinstance(g, tuple) else g.to(DEV) for g in grads_cpu]
    ops.grad_pack(grads_dev, flat, scale, words, tail)
    w64, tail_ref = R.grad_pack([g if isinstance(g, tuple) else g.double() for g in grads_cpu], scale, words.cpu(), torch.tensor([0.0, 0.0, 2.0]))
    w32, _ = R.grad_pack(grads_cpu, scale)
    rule("grad_pack table %s" % table, flat[:total], w64, w32)
    assert same_bits(flat[:total], w32)                                                       # one correctly rounded product per element
    assert tail.tolist() == tail_ref.tolist() == [0.0, 1.0, 1.0]
    assert flat[total + n_words:].tolist() == [-77.0] * 4                                     # nothing behind the tail is touched
    words.copy_(torch.tensor([3, 0, 0], dtype=torch.int32))
    ops.grad_pack(grads_dev, flat, scale, words, tail)                                        # sticky across calls
    assert tail.tolist() == [1.0, 1.0, 1.0] and same_bits(flat[:total], w32)
    tail.zero_()
    ops.grad_pack(grads_dev, flat, scale, torch.zeros(3, dtype=torch.int32, device=DEV), tail)
    assert tail.tolist() == [0.0, 0.0, 0.0]


# ------------------------------------------------------------------------------------------ step_inputs
BIG_COPY = 2048 * 256 * 16 + 32                                                               # one 16-byte lane round above the grid cap
COPY_SIZES = ((1, torch.bool), (15, torch.bool), (16, torch.float32), (17, torch.bool), (4097, torch.bool), (24, torch.int64),
              (4, torch.float32), (8, torch.int64))
SENTINEL = 0xA5


@pytest.mark.parametrize("n_copies, big", [(24, False), (25, False), (24, True), (1, True)])
def test_step_inputs_copies_exactly_the_bytes_it_was_given(ops, n_copies, big):
    """Every destination is a view inside a sentinel-filled buffer, 16 bytes of guard on each side (the ragged tail of the 16-byte
    lanes); 25 copies are two launches; scalars and the gate words travel with the first."""
    rs = np.random.RandomState(n_copies + 100 * big)
    copies, checks = [], []
    for k in range(n_copies):
        nbytes, dtype = (BIG_COPY, torch.float32) if (big and k == n_copies // 2) else COPY_SIZES[k % len(COPY_SIZES)]
        padded = (nbytes + 15) // 16 * 16
        buf = torch.full((padded + 32,), SENTINEL, dtype=torch.uint8, device=DEV)
        raw = torch.from_numpy(rs.randint(0, 2 if dtype == torch.bool else 256, size=nbytes).astype(np.uint8))
        src_buf = torch.zeros(padded, dtype=torch.uint8, device=DEV)
        src_buf[:nbytes] = raw.to(DEV)
        dst, src = buf[16:16 + nbytes].view(dtype), src_buf[:nbytes].view(dtype)
        assert dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0 and dst.numel() * dst.element_size() == nbytes
        copies.append((dst, src))
        checks.append((buf, raw, nbytes))
    scalars = [(torch.full((), -1.0, device=DEV), 0.625), (torch.full((), -1.0, device=DEV), 3.0e-4)]
    words = torch.tensor([0, 9, 0, -2], dtype=torch.int32, device=DEV)
    words_host = torch.full((4,), 111, dtype=torch.int32).pin_memory()
    ops.step_inputs(copies, scalars, words, words_host)
    torch.cuda.synchronize()
    for k, (buf, raw, nbytes) in enumerate(checks):
        b = buf.cpu()
        assert torch.equal(b[16:16 + nbytes], raw), k
        assert (b[:16] == SENTINEL).all() and (b[16 + nbytes:] == SENTINEL).all(), (k, nbytes)
    assert [float(s[0]) for s in scalars] == [float(np.float32(0.625)), float(np.float32(3.0e-4))]
    assert words_host.tolist() == [0, 9, 0, -2]


# ------------------------------------------------------------------------------------------ optimisers
LR_RMS, LR_ADAM = 2.0 ** -10, 2.0 ** -11                                                      # exact in float32
RMS_NUMELS = (4099, 1, 2, 255, 256, 257)
RMS_TABLES = {"1": (4099,), "16": tuple(RMS_NUMELS[k % 6] for k in range(16)), "17": tuple(RMS_NUMELS[k % 6] for k in range(17)),
              "cap+1": (4099, 600000, 4096 * 256 + 1 - 4099 - 600000)}
ADAM_NUMELS = (1, 3, 63, 65, 1000)
ADAM_TABLES = {"1": (1000,), "32": tuple(ADAM_NUMELS[k % 5] for k in range(32)), "33": tuple(ADAM_NUMELS[k % 5] for k in range(33))}
for _name, _total in (("round-1", 256 * 256 * 4 - 1), ("round", 256 * 256 * 4), ("round+1", 256 * 256 * 4 + 1), ("2rounds+7", 2 * 256 * 256 * 4 + 7)):
    ADAM_TABLES[_name] = ADAM_NUMELS + (_total - sum(ADAM_NUMELS),)


@functools.lru_cache(maxsize=None)
def optim_ref(kind, numels, n_steps, scale_exp0, tiny):
    """(fp64 restatement, stock torch.optim in float32 on the CPU) after n_steps: [(p, state...)] flat; shared, never written to."""
    c = R.optim_case(numels, n_steps, scale_exp0, tiny)
    p, gs = f64(c["p"]), f64(c["g"])
    a, b = torch.zeros_like(p), torch.zeros_like(p)
    params = [torch.nn.Parameter(x.clone()) for x in f32(c["p"]).split(list(numels))]
    opt = (torch.optim.RMSprop(params, lr=LR_RMS, alpha=0.99, eps=1e-8) if kind == "rmsprop"
           else torch.optim.Adam(params, lr=LR_ADAM, betas=(0.9, 0.999), eps=1e-8))
    for it in range(n_steps):
        if kind == "rmsprop":
            p, a = R.rmsprop_step(p, gs[it], a, LR_RMS)
        else:
            p, a, b = R.adam_step(p, gs[it], a, b, it + 1, LR_ADAM)
        for q, g in zip(params, f32(c["g"])[it].split(list(numels))):
            q.grad = g.clone()
        opt.step()
    keys = ("square_avg",) if kind == "rmsprop" else ("exp_avg", "exp_avg_sq")
    stock = [torch.cat([q.detach() for q in params])] + [torch.cat([opt.state[q][k] for q in params]) for k in keys]
    return ([p, a] if kind == "rmsprop" else [p, a, b]), stock


@pytest.mark.parametrize("via", ["ops", "fused"])
@pytest.mark.parametrize("table", sorted(RMS_TABLES))
def test_rmsprop_three_steps(ops, table, via):
    """Three steps with gradients of 10^(it - 2); the first tensor's gradients are exactly 0 / about 1e-20 (sq goes denormal, eps alone
    keeps the quotient finite); a host learning rate through ops, a device one through FusedRMSprop for the odd tables and vice versa."""
    from texpose_amd.trainer import FusedRMSprop
    numels = RMS_TABLES[table]
    c = R.optim_case(numels, 3, -2, True)
    lr_on_device = (sorted(RMS_TABLES).index(table) + (via == "fused")) % 2 == 1
    lr = torch.tensor(LR_RMS, device=DEV) if lr_on_device else LR_RMS
    ps = [torch.nn.Parameter(x.clone()) for x in cu(c["p"]).split(list(numels))]
    gs = cu(c["g"])
    if via == "fused":
        opt = FusedRMSprop(ps, lr=lr, alpha=0.99, eps=1e-8, capturable=True)
    else:
        sqs, steps = [torch.zeros_like(p) for p in ps], [torch.zeros((), device=DEV) for _ in ps]
    for it in range(3):
        grads = [g.clone() for g in gs[it].split(list(numels))]
        if via == "fused":
            for p, g in zip(ps, grads):
                p.grad = g
            opt.step()
        else:
            ops.rmsprop_step([p.data for p in ps], grads, sqs, lr, 0.99, 1e-8, steps=steps)
    if via == "fused":
        sqs, steps = [opt.state[p]["square_avg"] for p in ps], [opt.state[p]["step"] for p in ps]
    assert [float(s) for s in steps] == [3.0] * len(ps)                                       # + 1 per step, in both chunks
    ref64, stock = optim_ref("rmsprop", numels, 3, -2, True)
    got = [torch.cat([p.detach() for p in ps]), torch.cat(sqs)]
    assert all(torch.isfinite(x).all() for x in got)
    for name, g, w64, w32 in zip(("p", "sq"), got, ref64, stock):
        rule("rmsprop %s table %s %s %s lr" % (name, table, via, "device" if lr_on_device else "host"), g, w64, w32)


@pytest.mark.parametrize("via", ["ops", "fused"])
@pytest.mark.parametrize("table", sorted(ADAM_TABLES))
def test_adam_five_steps(ops, table, via):
    """Five steps back to back (the ticket is reused without a synchronise) with gradients of 10^(it - 3); tensor boundaries inside a
    wavefront; totals around one full round of 256 workgroups x 256 threads x 4 elements."""
    from texpose_amd.trainer import FusedAdam
    numels = ADAM_TABLES[table]
    c = R.optim_case(numels, 5, -3)
    ps = [torch.nn.Parameter(x.clone()) for x in cu(c["p"]).split(list(numels))]
    gs = cu(c["g"])
    if via == "fused":
        opt = FusedAdam(ps, lr=torch.tensor(LR_ADAM, device=DEV), betas=(0.9, 0.999), eps=1e-8, capturable=True)
    else:
        ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
        steps = [torch.zeros((), device=DEV) for _ in ps]
    for it in range(5):
        grads = [g.clone() for g in gs[it].split(list(numels))]
        if via == "fused":
            for p, g in zip(ps, grads):
                p.grad = g
            opt.step()
        else:
            ops.adam_step([p.data for p in ps], grads, ms, vs, steps, LR_ADAM, 0.9, 0.999, 1e-8)
    if via == "fused":
        ms, vs = [opt.state[p]["exp_avg"] for p in ps], [opt.state[p]["exp_avg_sq"] for p in ps]
        steps = [opt.state[p]["step"] for p in ps]
    assert [float(s) for s in steps] == [5.0] * len(ps)
    ref64, stock = optim_ref("adam", numels, 5, -3, False)
    got = [torch.cat([p.detach() for p in ps]), torch.cat(ms), torch.cat(vs)]
    for name, g, w64, w32 in zip(("p", "m", "v"), got, ref64, stock):
        rule("adam %s table %s %s" % (name, table, via), g, w64, w32)


def test_adam_per_tensor_step_counts_and_a_shared_counter(ops):
    """One launch over tensors that start at step 0 and at step 1000 (per-tensor bias corrections), against stock Adam with the same
    state loaded; two table entries that share one counter advance it once per launch."""
    numels, starts = (65, 1000, 3, 63), (0.0, 1000.0, 1000.0, 0.0)
    rs = np.random.RandomState(77)
    p0 = [rs.normal(size=n).astype(np.float32) for n in numels]
    g0 = [rs.normal(size=n).astype(np.float32) for n in numels]
    m0 = [(0.1 * rs.normal(size=n) * (s > 0)).astype(np.float32) for n, s in zip(numels, starts)]
    v0 = [(0.01 * rs.uniform(size=n) * (s > 0)).astype(np.float32) for n, s in zip(numels, starts)]
    ps, gsd, ms, vs = ([cu(x) for x in xs] for xs in (p0, g0, m0, v0))
    steps = [torch.tensor(s, device=DEV) for s in starts]
    ops.adam_step(ps, gsd, ms, vs, steps, LR_ADAM, 0.9, 0.999, 1e-8)
    assert [float(s) for s in steps] == [s + 1 for s in starts]
    params = [torch.nn.Parameter(torch.from_numpy(x.copy())) for x in p0]
    opt = torch.optim.Adam(params, lr=LR_ADAM, betas=(0.9, 0.999), eps=1e-8)
    for q, g, m, v, s in zip(params, g0, m0, v0, starts):
        q.grad = torch.from_numpy(g.copy())
        opt.state[q] = dict(step=torch.tensor(s), exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
    opt.step()
    for k, s in enumerate(starts):
        w64 = R.adam_step(*(torch.from_numpy(x[k]).double() for x in (p0, g0, m0, v0)), s + 1, LR_ADAM)
        stock = (params[k].detach(), opt.state[params[k]]["exp_avg"], opt.state[params[k]]["exp_avg_sq"])
        for name, g, a, b in zip(("p", "m", "v"), (ps[k], ms[k], vs[k]), w64, stock):
            rule("adam %s tensor %d from step %d" % (name, k, s), g, a, b)
    shared = torch.zeros((), device=DEV)
    steps = [shared, torch.zeros((), device=DEV), shared, shared]
    for it in range(2):
        ops.adam_step(ps, gsd, ms, vs, steps, LR_ADAM, 0.9, 0.999, 1e-8)
    assert float(shared) == 2.0 and float(steps[1]) == 2.0


GATES = [(1, 0), (3, 0), (3, 1), (3, 2), (64, 0), (64, 31), (64, 63)]


@pytest.mark.parametrize("n_gate, set_word", GATES)
@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_a_set_gate_word_withholds_the_whole_step(ops, kind, n_gate, set_word):
    """With any one gate word set, parameters, moments and step counters stay bit for bit; with all words clear the step applies."""
    numels = (1000, 65, 3, 1)
    c = R.optim_case(numels, 1, 0)
    ps, gs = list(cu(c["p"]).clone().split(list(numels))), list(cu(c["g"])[0].clone().split(list(numels)))
    ps, gs = [p.contiguous() for p in ps], [g.contiguous() for g in gs]
    state = [[torch.full_like(p, 0.25) for p in ps] for _ in range(1 if kind == "rmsprop" else 2)]
    steps = [torch.full((), 7.0, device=DEV) for _ in ps]
    gate = torch.zeros(n_gate, dtype=torch.int32, device=DEV)
    gate[set_word] = 1 if set_word % 2 == 0 else -(2 ** 31)

    def step():
        if kind == "rmsprop":
            ops.rmsprop_step(ps, gs, state[0], LR_RMS, 0.99, 1e-8, gate=gate, steps=steps)
        else:
            ops.adam_step(ps, gs, state[0], state[1], steps, LR_ADAM, 0.9, 0.999, 1e-8, gate=gate)

    before = [x.clone() for x in ps + sum(state, []) + steps]
    step()
    assert all(same_bits(a, b) for a, b in zip(ps + sum(state, []) + steps, before))
    gate.zero_()
    step()
    assert [float(s) for s in steps] == [8.0] * len(ps)
    assert all(not same_bits(a, b) for a, b in zip(ps + sum(state, []), before))
    if kind == "adam":                                                                       # the withheld launch left the ticket clear
        step()
        assert [float(s) for s in steps] == [9.0] * len(ps)


# ------------------------------------------------------------------------------------------ determinism
def test_every_kernel_repeats_its_bits_at_its_largest_case(ops, aops):
    def twice(fn):
        a, b = fn(), fn()
        a, b = (list(x) if isinstance(x, (tuple, list)) else [x] for x in (a, b))
        assert all(same_bits(x, y) for x, y in zip(a, b) if x is not None)

    x = cu(R.logits_case(5001, 1.0))
    twice(lambda: ops.bce_logits_fwd(x, 1.0))
    twice(lambda: ops.bce_logits_bwd(x, 1.0, torch.tensor(0.9, device=DEV)))
    twice(lambda: ops.gan_disc_losses(x, cu(R.logits_case(5001, 0.0)), 0.9, 1.3))
    f = cu(R.feat_case(16384))
    twice(lambda: ops.feat_pair_loss_fwd(f, 5.0))
    twice(lambda: ops.feat_pair_loss_bwd(f, 5.0, torch.tensor(0.7, device=DEV)))
    s = cu(R.sumsq_case(1024 * 1024 + 3, 3))
    twice(lambda: ops.sumsq_mean_fwd(s))
    twice(lambda: ops.sumsq_mean_bwd(s, torch.tensor(0.8, device=DEV)))
    twice(lambda: ops.sumsq_mean_fwd_bwd(s, 0.35))
    c = R.nerf_case(2, 513, 256, "random")
    rgb, unc, den, gat = (cu(c[k]) for k in ("rgb", "uncert", "density", "gathered"))
    twice(lambda: ops.nerf_losses_fwd(rgb, unc, den, gat, want_losses=True))
    sums = ops.nerf_losses_fwd(rgb, unc, den, gat)
    twice(lambda: ops.nerf_losses_bwd(rgb, unc, den, gat, sums, cu(c["g"])))
    p = R.pool_case(2, 4, 130)
    px = cu(p["x"]).reshape(1, 2, 4, 130)
    twice(lambda: ops.maxpool2_fwd(px))
    twice(lambda: ops.maxpool2_bwd(cu(p["gy"]).reshape(1, 2, 2, 65), ops.maxpool2_fwd(px)[1]))
    k = R.stack_case(3, 3, 86)
    mean, std = [float(np.float32(v)) for v in R.MEAN], [float(np.float32(v)) for v in R.STD]
    twice(lambda: ops.feat_inputs_fwd(cu(k["rgb"]), cu(k["gathered"]), mean, std, (3, 86)))
    twice(lambda: ops.feat_inputs_bwd(cu(k["rgb"]), cu(k["gathered"]), mean, std, cu(k["cot"])))
    twice(lambda: ops.disc_inputs(cu(k["rgb"]), cu(k["gathered"]), (3, 86), True))
    twice(lambda: ops.fake_patch_bwd(cu(k["cot_fake"]), 3, 3 * 86))
    lat = R.latent_case(5, 9, 17, 13)
    idx = cu(lat["idx"])
    twice(lambda: ops.latent_rows_fwd(cu(lat["w_trans"]), cu(lat["w_light"]), idx))
    twice(lambda: ops.latent_rows_bwd(cu(lat["g_trans"]), cu(lat["g_light"]), idx, 9))
    terms, weights = R.terms_case(16)
    td = [cu(terms)[i] for i in range(16)]
    twice(lambda: ops.weighted_sum(td, [float(w) for w in weights]))
    g = cu(R.sumsq_case(1024 * 1024 + 3, 1)).reshape(-1)

    def inputs():
        dst = torch.empty(BIG_COPY // 4 + 1, device=DEV)
        ops.step_inputs([(dst[:BIG_COPY // 4], s.reshape(-1)[:BIG_COPY // 4]), (dst[BIG_COPY // 4:], g[:1])])
        return dst
    twice(inputs)

    def pack():
        flat = torch.empty(g.numel() + 7, device=DEV)
        ops.grad_pack([g[:1025], (None, 7), g[1025:]], flat, 1.0 / 3.0)
        return flat
    twice(pack)

    def optimiser(kind, numels):
        c = R.optim_case(numels, 1, 0)
        ps, gs = list(cu(c["p"]).clone().split(list(numels))), list(cu(c["g"])[0].split(list(numels)))
        ps, gs = [q.contiguous() for q in ps], [q.contiguous() for q in gs]
        a, b = [torch.zeros_like(q) for q in ps], [torch.zeros_like(q) for q in ps]
        steps = [torch.zeros((), device=DEV) for _ in ps]
        if kind == "rmsprop":
            ops.rmsprop_step(ps, gs, a, LR_RMS, 0.99, 1e-8, steps=steps)
        else:
            ops.adam_step(ps, gs, a, b, steps, LR_ADAM, 0.9, 0.999, 1e-8)
        return ps + a + b
    twice(lambda: optimiser("rmsprop", RMS_TABLES["cap+1"]))
    twice(lambda: optimiser("adam", ADAM_TABLES["2rounds+7"]))
