"""Plain torch restatements of the two reduction families of the PatchGAN half of a training step (csrc/spectral_norm.hip, kernels A-E;
csrc/inorm_lrelu.hip, forward / backward / double backward) for the tests: CPU only, no code under test.

Every function computes in the dtype of its inputs: with float64 inputs it is the reference, with the same inputs cast to float32 it is
the "plain fp32 evaluation of the same formulas" of the project's accuracy rule (`within_rule`).  The restatements are
closed against torch's own modules in fp64 by tests/test_norm_ref_cpu.py.

Also here: the seeded inputs of tests/test_gpu_norm_kernels.py (`sn_case`, `inorm_case`), so that the CPU test can check properties of
the very inputs the GPU test uses (the share of elements next to the LeakyReLU kink)."""
import functools

import numpy as np
import torch

SN_EPS = 1e-12                 # torch.nn.utils.spectral_norm's default eps (F.normalize clamps the NORM with it)
GATE_BAND = 1e-5               # |xhat| below this: an fp32 xhat may sit on the other side of the kink
GATE_SHARE = 1e-3              # at most this share of a case's elements may be that close


# ------------------------------------------------------------------------------------------ spectral norm
def normalize(x, eps=SN_EPS):
    """F.normalize(x, dim=0, eps): x / max(|x|_2, eps)."""
    return x / torch.sqrt((x * x).sum()).clamp_min(eps)


def sn_forward(W, u, v, training):
    """One forward of torch.nn.utils.spectral_norm on W.view(rows, -1): (W_sn, u, v, sigma); in training mode one power iteration first
    (v <- normalize(W^T u), u <- normalize(W v)), in eval mode u and v are returned untouched.  `n_sets` iterations in a row are this
    function applied to its own u, v repeatedly."""
    W2 = W.reshape(W.shape[0], -1)
    if training:
        v = normalize(W2.t() @ u)
        u = normalize(W2 @ v)
    sigma = torch.dot(u, W2 @ v)
    return W / sigma, u, v, sigma


def sn_forward_sets(W, u, v, n_sets):
    """[(W_sn, u, v, sigma)] of n_sets training-mode forwards in a row."""
    out = []
    for _ in range(n_sets):
        out.append(sn_forward(W, u, v, True))
        u, v = out[-1][1], out[-1][2]
    return out


def sn_backward(G, W_sn, u, v, sigma, second=None, accumulate_into=None):
    """dL/dW from G = dL/dW_sn with u, v constants (torch detaches them): (G - <G, W_sn> u v^T) / sigma.  ``second`` = (G2, W_sn2, u2, v2,
    sigma2): a second normalised instance of the same weight, its term added; ``accumulate_into``: prior contents the result is added to."""
    out = (G - (G * W_sn).sum() * torch.outer(u, v).reshape(G.shape)) / sigma
    if second is not None:
        out = out + sn_backward(*second)
    if accumulate_into is not None:
        out = accumulate_into + out
    return out


# ------------------------------------------------------------------------------------------ InstanceNorm2d + LeakyReLU
def gate_of(xhat, slope):
    """LeakyReLU's derivative as torch's leaky_relu backward takes it: 1 where xhat > 0, else slope (at xhat == 0 too)."""
    return torch.where(xhat > 0, torch.ones_like(xhat), torch.full_like(xhat, slope))


def inorm_lrelu_fwd(x, eps, slope):
    """x [n_inst, hw] -> (xhat, rstd [n_inst], y): biased variance, rstd = (var + eps)^-1/2, y = xhat * gate."""
    mean = x.mean(1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(1, keepdim=True) + eps)
    xhat = d * rstd
    return xhat, rstd[:, 0], xhat * gate_of(xhat, slope)


def inorm_lrelu_bwd(xhat, rstd, gy, slope, addend=None, gate=None):
    """gx = rstd P(gy * gate) (+ addend), P(v) = v - mean(v) - xhat mean(v xhat).  ``gate``: taken as given instead of from xhat."""
    s = gate_of(xhat, slope) if gate is None else gate
    a = gy * s
    gx = rstd[:, None] * (a - a.mean(1, keepdim=True) - xhat * (a * xhat).mean(1, keepdim=True))
    return gx if addend is None else gx + addend


def inorm_lrelu_bwd_bwd(xhat, rstd, gy, ggx, slope, gate=None):
    """Cotangent ggx of gx -> (g_gy, g_x), the header comment of csrc/inorm_lrelu.hip."""
    n = xhat.shape[1]
    s = gate_of(xhat, slope) if gate is None else gate
    r = rstd[:, None]
    a, u = gy * s, ggx
    mu, ma = u.mean(1, keepdim=True), a.mean(1, keepdim=True)
    A = (u * a).sum(1, keepdim=True) - n * mu * ma
    C, D = (u * xhat).mean(1, keepdim=True), (a * xhat).mean(1, keepdim=True)
    g_gy = s * r * (u - mu - xhat * C)
    g_x = -(r * r / n) * xhat * (A - n * C * D) - r * r * (D * (u - mu) + C * (a - ma) - 2.0 * C * D * xhat)
    return g_gy, g_x


def inorm_lrelu(x, eps, slope, gy=None, ggx=None, addend=None):
    """Everything of one x [n_inst, hw]: dict(xhat, rstd, y[, gx][, g_gy, g_x]) -- the forward, the backward for the cotangent gy of y
    and the double backward for the cotangent ggx of gx."""
    xhat, rstd, y = inorm_lrelu_fwd(x, eps, slope)
    out = dict(xhat=xhat, rstd=rstd, y=y)
    if gy is not None:
        out["gx"] = inorm_lrelu_bwd(xhat, rstd, gy, slope, addend)
        if ggx is not None:
            out["g_gy"], out["g_x"] = inorm_lrelu_bwd_bwd(xhat, rstd, gy, ggx, slope)
    return out


# ------------------------------------------------------------------------------------------ seeded inputs shared by the CPU and GPU tests
def unit(rs, n):
    x = rs.normal(size=n)
    return (x / np.linalg.norm(x)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sn_case(rows, cols, scale_log2=0):
    """(W, u, v, G, G2, prior) float32 CPU tensors: normal weight scaled by 1 / sqrt(cols) (times 2^scale_log2, exact), unit u and v, two
    cotangents and prior contents for the accumulate form.  Shared and never written to (callers clone)."""
    rs = np.random.RandomState(100003 * rows + cols)
    W = (rs.normal(size=(rows, cols)) / np.sqrt(cols)).astype(np.float32) * np.float32(2.0 ** scale_log2)
    u, v = unit(rs, rows), unit(rs, cols)
    G, G2, prior = (rs.normal(size=(rows, cols)).astype(np.float32) for _ in range(3))
    return tuple(torch.from_numpy(a) for a in (W, u, v, G, G2, prior))


INORM_VALUES = ("normal", "mean1e3", "spread1e-3", "spread1e3", "one_constant")
INORM_N = (1, 3, 4, 5, 9)                                   # around the four instances of a workgroup
INORM_HW = ((1, 1), (1, 2), (7, 9), (8, 8), (5, 13), (1, 127), (63, 65), (64, 64))      # hw 1, 2, 63, 64, 65, 127, 4095, 4096
# every hw at 5 instances, every instance count at hw 65
INORM_SHAPES = tuple((5, h, w) for h, w in INORM_HW) + tuple((n, 5, 13) for n in INORM_N if n != 5)


def constant_rows(values, n_inst):
    """Indices of the instances `inorm_case` makes constant (one among random ones: none if there is only one instance)."""
    return (1,) if values == "one_constant" and n_inst > 1 else ()


@functools.lru_cache(maxsize=None)
def inorm_case(n_inst, H, W, values):
    """dict(x, gy, ggx, addend [n_inst, hw] float32; exact [n_inst] bool; mask [n_inst, hw] bool; ref: `inorm_lrelu` in fp64 of the
    MASKED cotangents).  mask: |xhat_ref| < GATE_BAND outside the instances whose xhat is exactly 0 (constant ones, hw == 1: their gate is
    `slope` with no rounding involved); gy and ggx are zero there, as every user of the case must keep them."""
    hw = H * W
    rs = np.random.RandomState(7919 * n_inst + 31 * hw + INORM_VALUES.index(values))
    z = rs.normal(size=(n_inst, hw))
    x = {"normal": z, "mean1e3": 1e3 + z, "spread1e-3": 1e-3 * z, "spread1e3": 1e3 * z, "one_constant": z}[values].astype(np.float32)
    for r in constant_rows(values, n_inst):
        x[r] = 3.0
    gy, ggx, addend = (rs.normal(size=(n_inst, hw)).astype(np.float32) for _ in range(3))
    x = torch.from_numpy(x)
    xhat, _, _ = inorm_lrelu_fwd(x.double(), EPS, SLOPE)
    exact = (xhat == 0).all(1)
    mask = (xhat.abs() < GATE_BAND) & ~exact[:, None]
    gy, ggx, addend = torch.from_numpy(gy), torch.from_numpy(ggx), torch.from_numpy(addend)
    gy[mask] = 0.0
    ggx[mask] = 0.0
    ref = inorm_lrelu(x.double(), EPS, SLOPE, gy.double(), ggx.double())
    return dict(x=x, gy=gy, ggx=ggx, addend=addend, exact=exact, mask=mask, ref=ref)


EPS, SLOPE = 1e-5, 0.2          # nn.InstanceNorm2d's default eps, the PatchGAN's LeakyReLU(0.2)
