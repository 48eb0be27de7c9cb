"""CPU: tests/norm_ref.py (the fp64 restatements the GPU tests of csrc/spectral_norm.hip and csrc/inorm_lrelu.hip compare with) against
torch's own modules in fp64, and the properties of the GPU test's seeded inputs that only the reference can vouch for."""
import pytest
import torch

import norm_ref as R

RAGGED = [(5, 19), (17, 241), (65, 7)]


def _stock_sn(W, u, v, training, cot):
    """torch.nn.utils.spectral_norm on a Linear in fp64: (weight, u, v after the forward, d <weight, cot> / d weight_orig)."""
    lin = torch.nn.utils.spectral_norm(torch.nn.Linear(W.shape[1], W.shape[0], bias=False)).double()
    with torch.no_grad():
        lin.weight_orig.copy_(W)
        lin.weight_u.copy_(u)
        lin.weight_v.copy_(v)
    lin.train(training)
    lin(torch.zeros(1, W.shape[1], dtype=torch.float64))                       # the pre-forward hook computes .weight
    (g,) = torch.autograd.grad((lin.weight * cot).sum(), lin.weight_orig)
    return lin.weight.detach(), lin.weight_u.clone(), lin.weight_v.clone(), g


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("rows, cols", RAGGED)
def test_sn_reference_equals_torch_spectral_norm_in_fp64(rows, cols, training):
    W, u, v, G, G2, prior = (t.double() for t in R.sn_case(rows, cols))
    w_t, u_t, v_t, g_t = _stock_sn(W, u, v, training, G)
    w_r, u_r, v_r, sigma = R.sn_forward(W, u, v, training)
    for name, a, b in (("W_sn", w_r, w_t), ("u", u_r, u_t), ("v", v_r, v_t), ("dW", R.sn_backward(G, w_r, u_r, v_r, sigma), g_t)):
        assert float((a - b).abs().max()) <= 1e-12, (name, float((a - b).abs().max()))
    if not training:
        assert torch.equal(u_r, u) and torch.equal(v_r, v)
    # the second instance and the accumulate form are sums of the plain form
    (w1, u1, v1, s1), (w2, u2, v2, s2) = R.sn_forward_sets(W, u, v, 2)
    both = R.sn_backward(G, w1, u1, v1, s1, second=(G2, w2, u2, v2, s2), accumulate_into=prior)
    assert torch.equal(both, prior + (R.sn_backward(G, w1, u1, v1, s1) + R.sn_backward(G2, w2, u2, v2, s2)))
    # two forwards in a row of the stock module are the reference applied twice
    lin_w, lin_u, lin_v, _ = _stock_sn(W, u1, v1, True, G)
    assert float((lin_w - w2).abs().max()) <= 1e-12 and float((lin_u - u2).abs().max()) <= 1e-12 and float((lin_v - v2).abs().max()) <= 1e-12


@pytest.mark.parametrize("n_inst, H, W", [(3, 1, 2), (5, 5, 13), (4, 7, 9), (2, 8, 8)])
def test_inorm_reference_equals_fp64_autograd_up_to_second_order(n_inst, H, W):
    """Forward, gradient, the double backward for an arbitrary cotangent of gx, and the R1-style second-order gradients (gradient of
    |d out / d x|^2 wrt x and wrt an upstream weight, as test_inorm_lrelu_matches_torch_up_to_second_order forms them)."""
    c = R.inorm_case(n_inst, H, W, "normal")
    hw = H * W
    stock = torch.nn.Sequential(torch.nn.InstanceNorm2d(n_inst), torch.nn.LeakyReLU(R.SLOPE)).double()
    x = c["x"].double().requires_grad_()
    gy = c["gy"].double().requires_grad_()
    u = c["ggx"].double()
    y = stock(x.view(1, n_inst, H, W)).view(n_inst, hw)
    (gx,) = torch.autograd.grad(y, x, gy, create_graph=True)
    g_x, g_gy = torch.autograd.grad((gx * u).sum(), (x, gy))
    ref = c["ref"]
    for name, a, b in (("y", ref["y"], y.detach()), ("gx", ref["gx"], gx.detach()), ("g_gy", ref["g_gy"], g_gy), ("g_x", ref["g_x"], g_x)):
        assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max())), (name, float((a - b).abs().max()))
    # R1 style: h = x * w upstream, reg = |d out / d x|^2
    x = c["x"].double().requires_grad_()
    w = c["addend"].double().requires_grad_()
    cot = c["gy"].double()
    h = x * w
    out = (stock(h.view(1, n_inst, H, W)).view(n_inst, hw) * cot).sum()
    (gx,) = torch.autograd.grad(out, x, create_graph=True)
    d_x, d_w = torch.autograd.grad(gx.pow(2).sum(), (x, w))
    # the same from the closed forms: gx = w gh, reg = sum (w gh)^2, cotangent of gh = 2 w^2 gh
    hd, wd, xd = h.detach(), w.detach(), x.detach()
    xhat, rstd, _ = R.inorm_lrelu_fwd(hd, R.EPS, R.SLOPE)
    gh = R.inorm_lrelu_bwd(xhat, rstd, cot, R.SLOPE)
    _, g_h = R.inorm_lrelu_bwd_bwd(xhat, rstd, cot, 2 * wd * wd * gh, R.SLOPE)
    for name, a, b in (("gx", wd * gh, gx.detach()), ("d reg / d x", g_h * wd, d_x), ("d reg / d w", g_h * xd + 2 * wd * gh * gh, d_w)):
        assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max())), (name, float((a - b).abs().max()))


def test_inorm_reference_at_one_element_per_instance():
    """hw = 1 (stock InstanceNorm2d refuses it): y = 0, rstd = eps^-1/2, every gradient with respect to x is 0."""
    c = R.inorm_case(5, 1, 1, "mean1e3")
    ref = c["ref"]
    assert bool(c["exact"].all()) and not bool(c["mask"].any())
    assert torch.equal(ref["y"], torch.zeros(5, 1, dtype=torch.float64)) and torch.equal(ref["xhat"], torch.zeros(5, 1, dtype=torch.float64))
    assert torch.equal(ref["rstd"], torch.full((5,), R.EPS ** -0.5, dtype=torch.float64))
    assert not bool(ref["gx"].any()) and not bool(ref["g_x"].any()) and not bool(ref["g_gy"].any())
    # and by autograd through the restated forward (differentiable torch code), with a cotangent that is not masked
    x = c["x"].double().requires_grad_()
    gy = torch.ones(5, 1, dtype=torch.float64, requires_grad=True)
    _, _, y = R.inorm_lrelu_fwd(x, R.EPS, R.SLOPE)
    (gx,) = torch.autograd.grad(y, x, gy, create_graph=True)
    assert not bool(gx.any())


def test_constant_instance_is_exact_in_the_reference():
    c = R.inorm_case(5, 5, 13, "one_constant")
    (r,) = R.constant_rows("one_constant", 5)
    assert c["exact"].tolist() == [i == r for i in range(5)]
    assert not bool(c["ref"]["xhat"][r].any()) and not bool(c["ref"]["y"][r].any()) and float(c["ref"]["rstd"][r]) == R.EPS ** -0.5
    # the gate of the whole instance is `slope`: gx of it is rstd * slope * (gy - mean gy)
    gy = c["gy"][r].double()
    assert float((c["ref"]["gx"][r] - R.EPS ** -0.5 * R.SLOPE * (gy - gy.mean())).abs().max()) < 1e-9


@pytest.mark.parametrize("values", R.INORM_VALUES)
def test_share_of_elements_next_to_the_kink_in_the_gpu_tests_inputs(values):
    """The GPU test zeroes gy and ggx where |xhat_ref| < 1e-5 (an fp32 xhat may sit on the other side of LeakyReLU's kink there): at most
    0.1 % of the elements of any of its cases, with the very seeds it uses."""
    for n_inst, H, W in R.INORM_SHAPES:
        c = R.inorm_case(n_inst, H, W, values)
        share = float(c["mask"].double().mean())
        assert share <= R.GATE_SHARE, (n_inst, H, W, values, share)
        assert not bool(c["gy"][c["mask"]].any()) and not bool(c["ggx"][c["mask"]].any())
        assert int(c["exact"].sum()) == (n_inst if H * W == 1 else len(R.constant_rows(values, n_inst)))
