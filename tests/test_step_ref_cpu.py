"""CPU: tests/step_ref.py (the fp64 restatements the GPU tests of csrc/nerf_losses.hip, csrc/rmsprop.hip and csrc/train_misc.hip compare
with) against torch's own functions and optimisers in fp64, and the properties of the GPU test's seeded inputs that only the reference
can vouch for: each spike's share of its sum, finite losses, the all-zero mask, finite gradients at the extreme logits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import step_ref as R
from oracle import texpose_oracle as O

TOL = 1e-12
RAGGED = [5, 67, 1031]


def close(name, a, b, tol=TOL):
    err = float((torch.as_tensor(a).detach() - torch.as_tensor(b).detach()).abs().max())
    assert err <= tol, (name, err)


def d(a):
    return R.t(a).double()


@pytest.mark.parametrize("target", [0.0, 1.0])
@pytest.mark.parametrize("n", RAGGED)
def test_bce_reference_equals_torch_in_fp64(n, target):
    x = (d(R.logits_case(n, target)) / 100).requires_grad_()                      # (the spikes scaled back to size 4: inputs of order 1)
    want = F.binary_cross_entropy_with_logits(x, torch.full_like(x, target))
    close("value", R.bce_logits_mean(x, target), want)
    g = torch.tensor(1.3, dtype=torch.float64)
    (gx,) = torch.autograd.grad(want * g, x)
    close("grad", R.bce_logits_grad(x.detach(), target, g), gx)
    xr, xf = x.detach(), -x.detach().flip(0)
    out, gr, gf = R.gan_disc_losses(xr, xf, 0.9, 1.3)
    close("disc values", out, torch.stack([F.binary_cross_entropy_with_logits(xr, torch.ones_like(xr)),
                                           F.binary_cross_entropy_with_logits(xf, torch.zeros_like(xf))]))
    assert torch.equal(gr, R.bce_logits_grad(xr, 1.0, torch.tensor(0.9, dtype=torch.float64)))
    assert torch.equal(gf, R.bce_logits_grad(xf, 0.0, torch.tensor(1.3, dtype=torch.float64)))


@pytest.mark.parametrize("n", RAGGED)
def test_feat_pair_and_sumsq_references_equal_torch_in_fp64(n):
    f = (d(R.feat_case(n)) / 50).requires_grad_()
    want = F.mse_loss(f[0], f[2].detach()) + 5.0 * F.mse_loss(f[1], f[3].detach())
    loss, l1, l2 = R.feat_pair_loss(f, 5.0)
    close("loss", loss, want)
    close("parts", torch.stack([l1, l2]), torch.stack([F.mse_loss(f[0], f[2]), F.mse_loss(f[1], f[3])]))
    g = torch.tensor(0.7, dtype=torch.float64)
    (gf,) = torch.autograd.grad(want * g, f)
    got = R.feat_pair_loss_grad(f.detach(), 5.0, g)
    close("grad", got, gf)
    assert not got[2:].any()
    for B in (1, 3):
        x = (d(R.sumsq_case(n, B)) / 300).requires_grad_()
        want = x.pow(2).reshape(B, -1).sum(1).mean()
        close("sumsq", R.sumsq_mean(x), want)
        (gx,) = torch.autograd.grad(want * g, x)
        close("sumsq grad", R.sumsq_mean_grad(x.detach(), g), gx)
        out, og = R.sumsq_mean_fwd_bwd(x.detach(), 0.35)
        (gw,) = torch.autograd.grad(0.35 * x.pow(2).sum() / B, x)
        close("fused", out, torch.stack([want, 0.35 * want]).detach())
        close("fused grad", og, gw)


@pytest.mark.parametrize("mask_kind", R.MASK_KINDS)
@pytest.mark.parametrize("B, p, N", [(1, 1, 1), (2, 3, 5), (3, 5, 7)])
def test_nerf_losses_reference_equals_the_oracle_in_fp64(B, p, N, mask_kind):
    c = R.nerf_case(B, p * p, N, mask_kind)
    rgb, unc, den, gat = (d(c[k]) for k in ("rgb", "uncert", "density", "gathered"))
    rgb = (gat.reshape(B, 14, -1)[:, 0:3].permute(0, 2, 1) + (rgb - gat.reshape(B, 14, -1)[:, 0:3].permute(0, 2, 1)) / 10)   # order 1
    rgb, unc, den = rgb.requires_grad_(), unc.requires_grad_(), (den / 100).requires_grad_()
    g4 = gat.reshape(B, 14, p, p)
    want = O.nerf_losses(rgb, unc, den, dict(image=g4[:, 0:3], mask=g4[:, 12:13]))
    sums, losses = R.nerf_losses(rgb, unc, den, gat)
    tol = TOL * max(1.0, float(losses.detach().abs().max()))
    close("losses", losses, torch.stack([want["render"], want["uncert"], want["trans_reg"]]), tol)
    gl = d(c["g"])
    total = gl[0] * want["render"] + gl[1] * want["uncert"] + gl[2] * want["trans_reg"]
    grads = torch.autograd.grad(total, (rgb, unc, den))
    got = R.nerf_losses_grad(rgb.detach(), unc.detach(), den.detach(), gat, tuple(gl))
    for name, a, b in zip(("g_rgb", "g_uncert", "g_density"), got, grads):
        close(name, a.reshape(b.shape), b, TOL * max(1.0, float(b.abs().max())))
    assert not got[2][..., 0].any()
    one = R.nerf_losses_grad(rgb.detach(), unc.detach(), den.detach(), gat, (gl[0], None, None))
    (only,) = torch.autograd.grad(gl[0] * O.nerf_losses(rgb, unc, den, dict(image=g4[:, 0:3], mask=g4[:, 12:13]))["render"], rgb)
    close("None = 0", one[0], only, TOL * max(1.0, float(only.abs().max())))


@pytest.mark.parametrize("values", R.POOL_VALUES)
@pytest.mark.parametrize("n, H, W", [(3, 2, 6), (5, 8, 12), (7, 6, 2)])
def test_maxpool_reference_equals_torch_bit_for_bit(n, H, W, values):
    c = R.pool_case(n, H, W, values)
    x, gy = d(c["x"]).requires_grad_(), d(c["gy"])
    want, idx = F.max_pool2d(x[None], 2, 2, return_indices=True)
    y, arg = R.maxpool2(x.detach())
    assert torch.equal(torch.nan_to_num(y, nan=123.0), torch.nan_to_num(want[0].detach(), nan=123.0))
    assert torch.equal(torch.signbit(y), torch.signbit(want[0].detach()))
    oy, ox = torch.meshgrid(torch.arange(H // 2), torch.arange(W // 2), indexing="ij")
    flat = (2 * oy + arg.long() // 2) * W + 2 * ox + arg.long() % 2
    assert torch.equal(flat, idx[0])
    (gx,) = torch.autograd.grad((want[0] * gy).sum(), x)
    assert torch.equal(R.maxpool2_grad(gy, arg), gx)


@pytest.mark.parametrize("B, h, w", [(1, 1, 5), (2, 3, 7), (3, 5, 2)])
def test_input_stack_references_equal_the_model_expressions_in_fp64(B, h, w):
    c = R.stack_case(B, h, w)
    rgb0, g, cot = d(c["rgb"]), d(c["gathered"]), d(c["cot"])
    mt = torch.tensor(np.float32(R.MEAN)).double().view(1, 3, 1, 1)
    st = torch.tensor(np.float32(R.STD)).double().view(1, 3, 1, 1)
    image, image_syn, obj_mask, mask_syn = g[:, 0:3], g[:, 3:6], g[:, 12:13], g[:, 13:14]
    r = rgb0.clone().requires_grad_()
    rgb = r.view(B, h, w, 3).permute(0, 3, 1, 2)
    pad = torch.logical_and(mask_syn == 1, obj_mask == 0).double()
    x = torch.cat([rgb, rgb * obj_mask + image * (1 - obj_mask), image * obj_mask + image_syn * pad, image], 0)
    x = (x - mt) / st
    (gr,) = torch.autograd.grad((x * cot).sum(), r)
    close("feat_inputs", R.feat_inputs(rgb0, g), x.detach())
    close("feat_inputs grad", R.feat_inputs_grad(rgb0, g, cot), gr)
    assert float(pad.sum()) > 0
    for geo in (True, False):
        real, fake = R.disc_inputs(rgb0, g, geo)
        rgbd = rgb.detach()
        real_t, fake_t = image * obj_mask + rgbd * pad, rgbd
        if geo:
            real_t, fake_t = torch.cat([real_t, g[:, 6:9], g[:, 9:12]], 1), torch.cat([fake_t, g[:, 6:9], g[:, 9:12]], 1)
        assert torch.equal(real, real_t) and torch.equal(fake, fake_t.contiguous())
    cf = d(c["cot_fake"]).requires_grad_(False)
    f = R.disc_inputs(r, g, True)[1]
    (gf,) = torch.autograd.grad((f * cf).sum(), r)
    assert torch.equal(R.fake_patch_grad(cf), gf)


@pytest.mark.parametrize("B, n_rows, Ct, Cl", [(5, 9, 17, 13), (3, 2, 1, 5), (7, 4, 3, 1)])
def test_latent_rows_weighted_sum_and_grad_pack_references(B, n_rows, Ct, Cl):
    c = R.latent_case(B, n_rows, Ct, Cl)
    wt, wl, gt, gl = (d(c[k]) for k in ("w_trans", "w_light", "g_trans", "g_light"))
    idx = R.t(c["idx"])
    ot, ol = R.latent_rows(wt, wl, idx)
    assert torch.equal(ot, wt.index_select(0, idx)) and torch.equal(ol, wl.index_select(0, idx))
    for got, g in zip(R.latent_rows_grad(gt, gl, idx, n_rows), (gt, gl)):
        want = torch.zeros(n_rows, g.shape[1], dtype=torch.float64).index_add_(0, idx, g)
        close("latent grad", got, want)
        never = sorted(set(range(n_rows)) - set(idx.tolist()))
        assert not got[never].any()
    for n in (1, 2, 16):
        terms, weights = R.terms_case(n)
        tt, ww = d(terms), torch.tensor(np.float32(weights)).double()
        close("weighted_sum", R.weighted_sum(list(tt), weights), torch.dot(tt, ww))
    grads = [d(c["g_trans"]), (None, 3), d(c["g_light"]), (None, 1)]
    words, tail = torch.tensor([0, 5, 0, -1], dtype=torch.int32), torch.tensor([0.0, 0.0, 2.0, 1.0], dtype=torch.float64)
    flat, tail2 = R.grad_pack(grads, 0.25, words, tail)
    want = torch.cat([grads[0].reshape(-1) * 0.25, torch.zeros(3, dtype=torch.float64), grads[2].reshape(-1) * 0.25,
                      torch.zeros(1, dtype=torch.float64)])
    assert torch.equal(flat, want) and tail2.tolist() == [0.0, 1.0, 1.0, 1.0]
    assert R.grad_pack(grads, 0.25, torch.zeros(4, dtype=torch.int32), tail2)[1].tolist() == [0.0, 1.0, 1.0, 1.0]      # sticky


@pytest.mark.parametrize("numels", [(5,), (67, 1, 3), (1031, 2)])
def test_optimiser_references_equal_torch_optim_in_fp64_over_five_steps(numels):
    c = R.optim_case(numels, 5, -3)
    lr = 2.0 ** -10
    p0, gs = d(c["p"]), d(c["g"])
    for kind in ("rmsprop", "adam"):
        params = [torch.nn.Parameter(x.clone()) for x in p0.split(list(numels))]
        opt = (torch.optim.RMSprop(params, lr=lr, alpha=0.99, eps=1e-8) if kind == "rmsprop"
               else torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999), eps=1e-8))
        p, a, b = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for it in range(5):
            for q, g in zip(params, gs[it].split(list(numels))):
                q.grad = g.clone()
            opt.step()
            if kind == "rmsprop":
                p, a = R.rmsprop_step(p, gs[it], a, lr)
            else:
                p, a, b = R.adam_step(p, gs[it], a, b, it + 1, lr)
            close(kind + " p", p, torch.cat([q.detach() for q in params]))
        state = [opt.state[q] for q in params]
        if kind == "rmsprop":
            close("sq", a, torch.cat([s["square_avg"] for s in state]))
        else:
            close("m", a, torch.cat([s["exp_avg"] for s in state]))
            close("v", b, torch.cat([s["exp_avg_sq"] for s in state]))


# ------------------------------------------------------------------------------------------ what only the reference can say of the cases
def _share(terms, spikes, h_plus_c):
    """Every spike is >= 100 x the typical (median) term and its share of sum |t| is >= 10 x the relative summation bound."""
    a = terms.reshape(-1).abs()
    rest = torch.ones_like(a, dtype=torch.bool)
    rest[list(spikes)] = False
    typical = float(a[rest].median()) if bool(rest.any()) else 0.0
    for i in spikes:
        assert float(a[i]) >= 100 * typical, (i, float(a[i]), typical)
        assert float(a[i]) / float(a.sum()) >= 10 * h_plus_c * R.U32, (i, float(a[i]) / float(a.sum()))


def test_spikes_carry_their_share_and_every_loss_is_finite():
    for n in (1, 63, 64, 65, 255, 256, 257, 513, 5001):
        for target in (0.0, 1.0):
            x = d(R.logits_case(n, target))
            _share(R.bce_terms(x, target), R.spike_indices(n, 256), 40)
            assert torch.isfinite(R.bce_logits_mean(x, target))
    for n in (1, 1023, 1024, 1025, 2049, 16384):
        f = d(R.feat_case(n))
        _share((f[0] - f[2]) ** 2, R.spike_indices(n, 1024), 40)
        _share((f[1] - f[3]) ** 2, R.spike_indices(n, 1024), 40)
        assert all(torch.isfinite(v) for v in R.feat_pair_loss(f, 5.0))
    for n in (1, 1023, 1024, 1025, 9 * 16 * 16 * 4, 1024 * 1024 + 3):
        for B in (1, 3):
            g = d(R.sumsq_case(n, B))
            _share(g * g, R.spike_indices(B * n, 1024), -(-B * n // 1024) + 23)
    for shape in ((1, 1, 1), (1, 255, 1), (1, 256, 1), (1, 257, 1), (1, 256, 256), (1, 257, 256), (1, 1024, 256), (2, 513, 256)):
        for kind in R.MASK_KINDS:
            c = R.nerf_case(*shape, kind)
            args = [d(c[k]) for k in ("rgb", "uncert", "density", "gathered")]
            t0, t1, t2, t3 = R.nerf_terms(*args)
            sums, losses = R.nerf_losses(*args)
            assert torch.isfinite(losses).all() and torch.isfinite(sums).all()
            assert float(args[1].min()) >= 0.05 - 1e-7 and float(args[1].max()) <= 1.5
            if kind in ("random", "ones"):
                _share(t0, c["spikes"], 40)
            if kind == "zeros":
                assert float(losses[0]) == 0.0 and float(sums[0]) == 0.0 and float(sums[1]) == 0.0
            _share(t2, c["spikes"], 40)
            _share(t3, R.spike_indices(t3.numel(), 256), 300)


def test_extreme_logits_have_finite_fp64_losses_and_gradients():
    for n in (13, 257):
        for target in (0.0, 1.0):
            x = d(R.logits_case(n, target, True))
            assert {float(np.float32(v)) for v in R.EXTREME_LOGITS} <= set(x.tolist())
            assert torch.isfinite(R.bce_logits_mean(x, target))
            g = R.bce_logits_grad(x, target, torch.tensor(1.3, dtype=torch.float64))
            assert torch.isfinite(g).all()
            want = F.binary_cross_entropy_with_logits(x, torch.full_like(x, target))
            close("extreme value", R.bce_logits_mean(x, target), want, 1e-12 * float(want))
