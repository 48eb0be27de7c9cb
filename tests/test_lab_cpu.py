"""CPU: the Lab chroma loss (loss_weight.lab).  tests/lab_ref.py (numpy fp64) against anchors that need no library; texpose_amd.lab
(torch) and the per-pixel arithmetic of the K23 kernels (csrc/lab_math.h, compiled for the host) against lab_ref; the argument
checks of the two C entry points; Graph.compute_loss on CPU tensors."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import lab_ref as R
from texpose_amd import _lib, lab
from texpose_amd.graph import Graph, summarize_loss
from texpose_amd.options import AttrDict, default_options

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _px(*rgb):
    return np.array(rgb, dtype=np.float64).reshape(1, 3, 1, 1)


def _inputs(seed=0, shape=(2, 3, 7, 9), margins=(1e-3, 1e-4)):
    rs = np.random.RandomState(seed)
    fake, _ = R.draw_colours(rs, shape, *margins)
    real, _ = R.draw_colours(rs, shape)
    mask = (rs.uniform(size=(shape[0], 1) + shape[2:]) > 0.3).astype(np.float64)
    return fake.astype(np.float64), real.astype(np.float64), mask


# ------------------------------------------------------------------ the fp64 restatement
def test_ref_anchors():
    black = R.rgb_to_lab(_px(0, 0, 0)).ravel()
    assert np.abs(black).max() < 1e-13                                  # (116 * 4/29 - 16 in fp64)
    white = R.rgb_to_lab(_px(1, 1, 1)).ravel()
    assert abs(white[0] - 100.0) < 1e-9 and abs(white[1]) < 0.01 and abs(white[2]) < 0.01      # (the matrix rows do not sum to the white point)
    for rgb, want in (((1, 0, 0), (53.24, 80.09, 67.20)), ((0, 1, 0), (87.73, -86.18, 83.18)), ((0, 0, 1), (32.30, 79.19, -107.86))):
        got = R.rgb_to_lab(_px(*rgb)).ravel()                           # the published sRGB / D65 values
        assert np.abs(got - np.array(want)).max() < 0.02, (rgb, got)
    n = R.normalize_lab(R.rgb_to_lab(_px(1, 0, 0))).ravel()
    np.testing.assert_allclose(n, [0.5324058790, (80.0923082 + 127) / 254, (67.2027510 + 127) / 254], atol=1e-7)


def test_ref_branches_and_rejection():
    rs = np.random.RandomState(3)
    c, rounds = R.draw_colours(rs, (2, 3, 50, 50), 1e-3, 1e-4)
    assert c.dtype == np.float32 and 1 <= rounds < 20                   # the rejection terminates
    assert c.min() < 0 and c.max() > 1
    c64 = c.astype(np.float64)
    t = R.xyz_normalised(c64)
    assert np.abs(c64 - R.SRGB_THRESHOLD).min() >= 1e-3 and np.abs(t - R.LAB_THRESHOLD).min() >= 1e-4
    for values, thr in ((c64, R.SRGB_THRESHOLD), (t, R.LAB_THRESHOLD)):          # both sides of both thresholds stay populated
        assert (values > thr).mean() > 0.02 and (values < thr).mean() > 0.02
    # continuity across the thresholds (the value is, the derivative is not)
    lo, hi = R.linearise(np.array([R.SRGB_THRESHOLD - 1e-9])), R.linearise(np.array([R.SRGB_THRESHOLD + 1e-9]))
    assert abs(hi - lo) < 1e-7


@pytest.mark.parametrize("masked", [False, True])
def test_ref_gradient_matches_central_differences(masked):
    fake, real, mask = _inputs(1, (2, 3, 4, 5))
    fake[0, :, 0, 0], real[0, :, 0, 0] = (5.0, -0.5, 5.0), (-0.5, 5.0, -0.5)          # |d| >= 1: the linear branch of SmoothL1
    mask[0, 0, 0, 0] = 1.0
    mask_ = mask if masked else None
    g = R.lab_loss_grad(fake, real, mask_)
    fl, rl = R.normalize_lab(R.rgb_to_lab(fake)), R.normalize_lab(R.rgb_to_lab(real))
    assert np.abs(fl[0, 1:, 0, 0] - rl[0, 1:, 0, 0]).max() >= 1.0
    h, num = 1e-6, np.zeros_like(fake)
    for i in np.ndindex(*fake.shape):
        xp, xm = fake.copy(), fake.copy()
        xp[i] += h
        xm[i] -= h
        num[i] = (R.lab_loss(xp, real, mask_)[0] - R.lab_loss(xm, real, mask_)[0]) / (2 * h)
    assert np.abs(num - g).max() < 1e-9 * max(1.0, np.abs(g).max()), np.abs(num - g).max()


# ------------------------------------------------------------------ the torch module
@pytest.mark.parametrize("masked", [False, True])
def test_torch_module_matches_ref_fp64(masked):
    fake, real, mask = _inputs(2)
    fake[1, :, 2, 3], real[1, :, 2, 3] = (5.0, -0.5, 5.0), (-0.5, 5.0, -0.5)
    mask[1, 0, 2, 3] = 1.0
    mask = mask if masked else None
    want, want_fake, want_real = R.lab_loss(fake, real, mask)
    ft = torch.tensor(fake, requires_grad=True)
    rt = torch.tensor(real, requires_grad=True)
    loss, fake_lab, real_lab = lab.LabLoss()(ft, rt, mask=None if mask is None else torch.tensor(mask))
    assert abs(float(loss.detach()) - want) < 1e-12
    assert not fake_lab.requires_grad and not real_lab.requires_grad
    assert np.abs(fake_lab.numpy() - want_fake).max() < 1e-12 and np.abs(real_lab.numpy() - want_real).max() < 1e-12
    assert np.array_equal(fake_lab[:, 0].numpy(), real_lab[:, 0].numpy())          # the L plane is the real image's
    loss.backward()
    g = R.lab_loss_grad(fake, real, mask)
    assert np.isfinite(g).all() and np.abs(ft.grad.numpy() - g).max() < 1e-12 * max(1.0, np.abs(g).max())
    assert lab.LabLoss()(ft, rt, return_lab=False).shape == ()


def test_torch_module_empty_mask_and_negative_colours():
    fake, real, mask = _inputs(4)
    loss, _, _ = lab.LabLoss()(torch.tensor(fake), torch.tensor(real), mask=torch.zeros(2, 1, 7, 9, dtype=torch.float64))
    assert torch.isnan(loss) and np.isnan(R.lab_loss(fake, real, np.zeros((2, 1, 7, 9)))[0])      # no epsilon, as in the reference
    # a channel below -0.055: the unselected power has a negative base; the gradient still follows the selected branch
    ft = torch.full((1, 3, 2, 2), -0.09, requires_grad=True)
    lab.LabLoss()(ft, torch.full((1, 3, 2, 2), 0.5))[0].backward()
    assert torch.isfinite(ft.grad).all() and float(ft.grad.abs().sum()) > 0
    with pytest.raises(ValueError):
        lab.rgb_to_lab(torch.zeros(2, 4, 3, 3))


# ------------------------------------------------------------------ the kernels' arithmetic, compiled for the host
_PROBE = r"""
#include <stdio.h>
#include "lab_math.h"
int main(void) {
  float c[3]; double ga, gb;
  while (scanf("%f %f %f %lf %lf", &c[0], &c[1], &c[2], &ga, &gb) == 5) {
    double lab[3], dlin[3], df[3], g[3];
    tp_lab::rgb_to_lab_norm<true>(c, lab, dlin, df);
    tp_lab::chroma_grad(ga, gb, dlin, df, g);
    printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", lab[0], lab[1], lab[2], g[0], g[1], g[2]);
  }
  printf("%.17g %.17g %.17g %.17g\n", tp_lab::smooth_l1(0.25), tp_lab::smooth_l1(-3.0), tp_lab::smooth_l1_grad(0.25), tp_lab::smooth_l1_grad(-3.0));
  return 0;
}
"""


def test_kernel_arithmetic_matches_ref(tmp_path):
    """csrc/lab_math.h is what both K23 kernels evaluate per pixel (in fp64 registers, rounded once on the way out)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("/opt/rocm/lib/llvm/bin/clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "probe.cpp").write_text(_PROBE)
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(REPO, "texpose_amd", "csrc"), "-o", str(tmp_path / "probe"),
                    str(tmp_path / "probe.cpp"), "-lm"], check=True)
    rs = np.random.RandomState(5)
    c, _ = R.draw_colours(rs, (1, 3, 40, 50))
    c = np.concatenate([c.reshape(3, -1).T, np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [5, -0.5, 5], [1e-6, 2e-6, 3e-6]], dtype=np.float32)])
    gab = rs.normal(size=(len(c), 2))
    text = "".join("%.9g %.9g %.9g %.17g %.17g\n" % (*row, *g) for row, g in zip(c, gab))
    out = subprocess.run([str(tmp_path / "probe")], input=text, check=True, capture_output=True, text=True).stdout.split("\n")
    got = np.array([[float(x) for x in line.split()] for line in out[:len(c)]])
    img = c.astype(np.float64).T.reshape(1, 3, -1)
    want_lab = R.normalize_lab(R.rgb_to_lab(img))[0].T
    # the chroma cotangents through the conversion: lab_loss_grad's chain with (ga, gb) in place of the SmoothL1 factors
    t = R.xyz_normalised(img)
    root = t > R.LAB_THRESHOLD
    df = np.where(root, np.cbrt(np.where(root, t, 1.0)) / (3.0 * np.where(root, t, 1.0)), 7.787)
    ga, gb = gab[:, 0][None] * (500.0 / 254.0), gab[:, 1][None] * (200.0 / 254.0)
    g_t = np.stack([ga, gb - ga, -gb], axis=1) * df
    g_lin = np.einsum("kc,bkn->bcn", R.RGB_TO_XYZ, g_t / R.WHITE.reshape(1, 3, 1))
    gamma = img > R.SRGB_THRESHOLD
    want_g = (g_lin * np.where(gamma, (2.4 / 1.055) * np.where(gamma, (img + 0.055) / 1.055, 1.0) ** 1.4, 1.0 / 12.92))[0].T
    assert np.abs(got[:, :3] - want_lab).max() < 2e-11 * max(1.0, np.abs(want_lab).max()), np.abs(got[:, :3] - want_lab).max()
    assert np.abs(got[:, 3:] - want_g).max() < 2e-11 * np.abs(want_g).max(), np.abs(got[:, 3:] - want_g).max()
    assert [float(x) for x in out[len(c)].split()] == [0.03125, 2.5, 0.25, -1.0]


# ------------------------------------------------------------------ the C entry points reject bad arguments without a GPU
def test_c_entry_points_reject_bad_arguments():
    lib = _lib.load()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)

    def good():
        a = _lib.LabLossArgs()
        a.rgb = a.real = a.mask = a.workspace = a.sums = a.loss = a.ticket = p
        a.B, a.P, a.real_batch_stride, a.real_channel_stride, a.mask_batch_stride = 1, 1, 3, 1, 1
        return a

    def rejected(a, *extra, fwd=True, text=b""):
        rc = lib.tp_lab_loss_fwd(C.byref(a), None) if fwd else lib.tp_lab_loss_bwd(C.byref(a), *extra, None)
        return rc < 0 and text in lib.tp_last_error()

    for field in ("rgb", "real", "sums", "workspace", "loss"):
        a = good()
        setattr(a, field, None)
        assert rejected(a, text=b"null pointer"), field
    for field in ("B", "P"):
        for bad in (0, -3):
            a = good()
            setattr(a, field, bad)
            assert rejected(a, text=b"bad sizes") and rejected(a, p, p, fwd=False, text=b"bad sizes")
    a = good()
    a.ticket = None
    assert rejected(a, text=b"ticket")
    a = good()
    a.real_channel_stride = 0
    assert rejected(a, text=b"stride")
    for field in ("rgb", "real", "sums"):
        a = good()
        setattr(a, field, None)
        assert rejected(a, p, p, fwd=False, text=b"null pointer")
    assert rejected(good(), None, p, fwd=False, text=b"null gradient pointer") and rejected(good(), p, None, fwd=False, text=b"null gradient pointer")
    assert C.sizeof(_lib.LabLossArgs) == 3 * 8 + 3 * 8 + 2 * 4 + 6 * 8 and _lib.LAB_LOSS_MAX_BLOCKS == 256 and _lib.ABI_VERSION == 16


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from texpose_amd import autograd_ops, ops
    rgb, real = torch.zeros(2, 16, 3), torch.zeros(2, 3, 4, 4)
    with pytest.raises(_lib.TexposeLibraryError):
        ops.lab_loss_fwd(rgb, real)
    with pytest.raises(_lib.TexposeLibraryError):
        ops.lab_loss_bwd(rgb, real, None, torch.zeros(2, dtype=torch.float64), torch.ones(()))
    with pytest.raises(_lib.TexposeLibraryError):
        autograd_ops.lab_loss(rgb, real, None)


# ------------------------------------------------------------------ Graph.compute_loss on CPU tensors
def _cpu_graph_and_var(patch):
    B, H, W, N = 2, 8, 8, 3
    opt = default_options(H=H, W=W, device="cpu")
    opt.batch_size, opt.patch_size = B, 4
    opt.loss_weight.update(feat=None, gan_nerf=None, lab=0)
    graph = Graph(opt)
    fake, real, mask = _inputs(6, (B, 3, H, W) if not patch else (B, 3, 4, 4))
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    hw = fake.shape[2] * fake.shape[3]
    var = AttrDict(idx=torch.arange(B))
    var.rgb = f32(fake).permute(0, 2, 3, 1).reshape(B, hw, 3).clone().requires_grad_()
    var.uncert, var.density = torch.full((B, hw, 1), 0.5), torch.rand(B, hw, N, 2)
    if patch:
        # the gather of the patch route done by hand (ops.patch_gather is a HIP kernel): gather_patches finds the samples in place
        var.ray_idx = torch.zeros(B, 4, 4, 2)
        var.gathered_for = var.ray_idx
        var.image_sample, var.image_syn_sample = torch.rand(B, 3, 4, 4), f32(real)
        var.mask_sample, var.mask_syn_sample = torch.ones(B, 1, 4, 4), f32(mask)
    else:
        var.image, var.obj_mask = torch.rand(B, 3, H * W), torch.ones(B, H * W, 1)
        var.image_syn, var.mask_syn = f32(real).reshape(B, 3, H * W), f32(mask).reshape(B, H * W, 1)
    return opt, graph, var, f32(fake), f32(real), f32(mask)


@pytest.mark.parametrize("patch", [False, True])
def test_compute_loss_runs_the_lab_term_on_cpu(patch):
    opt, graph, var, fake, real, mask = _cpu_graph_and_var(patch)
    assert graph.lab_loss is None
    loss = graph.compute_loss(opt, var, mode="train" if patch else "val", train_step="nerf")
    want, want_fake, want_real = R.lab_loss(fake.double().numpy(), real.double().numpy(), mask.double().numpy())
    assert loss.lab.shape == () and abs(float(loss.lab) - want) < 1e-5 * abs(want)
    assert var.rgb_lab.shape == fake.shape and var.img_syn_lab.shape == fake.shape
    assert np.abs(var.rgb_lab.numpy() - want_fake).max() < 1e-5 and np.abs(var.img_syn_lab.numpy() - want_real).max() < 1e-5
    assert not var.rgb_lab.requires_grad and not var.img_syn_lab.requires_grad
    total = summarize_loss(opt, loss).all                       # loss_weight.lab = 0: the term enters with weight 1
    (g,) = torch.autograd.grad(loss.lab, var.rgb, retain_graph=True)
    want_g = torch.tensor(R.lab_loss_grad(fake.double().numpy(), real.double().numpy(), mask.double().numpy()))
    want_g = want_g.permute(0, 2, 3, 1).reshape(g.shape)
    assert float((g.double() - want_g).abs().max()) < 1e-4 * float(want_g.abs().max())
    assert torch.isfinite(total) and "lab" in loss
    assert "_lab_module" not in dict(graph.named_modules()) and not any("lab" in k for k in graph.state_dict())


def test_compute_loss_calls_an_injected_module_like_the_reference():
    opt, graph, var, fake, real, mask = _cpu_graph_and_var(False)
    calls = []

    def stub(rgb, image_syn, mask=None):
        calls.append((rgb, image_syn, mask))
        return rgb.sum() * 0 + 7.0, "fake map", "real map"

    graph.lab_loss = stub
    loss = graph.compute_loss(opt, var, mode="val", train_step="nerf")
    assert len(calls) == 1 and float(loss.lab) == 7.0 and (var.rgb_lab, var.img_syn_lab) == ("fake map", "real map")
    rgb, image_syn, m = calls[0]
    assert torch.equal(rgb, fake) and torch.equal(image_syn, real) and torch.equal(m, mask) and m.shape == (2, 1, 8, 8)
