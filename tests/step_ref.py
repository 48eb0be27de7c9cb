"""Plain torch restatements of the small per-step kernels that end a training iteration (csrc/nerf_losses.hip K8, csrc/rmsprop.hip K10,
csrc/train_misc.hip K13) for the tests: CPU only, no code under test (this module does not import texpose_amd).

Every function computes in the dtype of its inputs: with float64 inputs it is the reference, with the same inputs in float32 it is the
"plain fp32 evaluation of the same formulas" of the project's accuracy rule (`within_rule`).  The formulas are the
kernels' header comments and the reference model lines they cite; tests/test_step_ref_cpu.py closes them against torch's own functions
and optimisers in fp64.

Also here: the seeded inputs of tests/test_gpu_step_kernels.py.  Every reduction case SPIKES four elements -- flat index 0, the last
element of the first block, the first element of the second block (where they exist) and n - 1 -- with terms at least 100 times the
typical one, so that a dropped or doubled partial sum moves the result far outside the summation bound at every size used."""
import functools
import math

import numpy as np
import torch

U32 = 2.0 ** -24               # unit roundoff of float32
MEAN = (0.485, 0.456, 0.406)   # ImageNet statistics of the feature network's input (layers/perceptual_loss.py:19-20)
STD = (0.229, 0.224, 0.225)
EXTREME_LOGITS = (0.0, 1e-8, -1e-8, 20.0, -20.0, 87.0, -87.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4)


def spike_indices(n, block):
    """Flat indices 0, block - 1, block, n - 1 as far as they exist (sorted, distinct)."""
    return sorted({i for i in (0, block - 1, block, n - 1) if 0 <= i < n})


def sum_bound(h, c, abs_terms_sum):
    """A-priori bound of an fp32 sum: h the longest addition chain, c the fp32 roundings inside one term, sum |t_i| in fp64."""
    return (h + c) * U32 * float(abs_terms_sum)


def _ro(a, dtype=np.float32):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.setflags(write=False)
    return a


def t(a):
    """A read-only numpy case array as a fresh (writable) torch tensor."""
    return torch.from_numpy(np.array(a))


# ------------------------------------------------------------------------------------------ BCE with logits, constant target
def bce_terms(x, target):
    """(1 - t) x - log_sigmoid(x), log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|))  (torch's stable form)."""
    return (1 - target) * x - (x.clamp(max=0) - torch.log1p(torch.exp(-x.abs())))


def bce_logits_mean(x, target):
    return bce_terms(x, target).sum() / x.numel()


def bce_logits_grad(x, target, g):
    """d mean / d x times the upstream g: (sigmoid(x) - t) g / n."""
    return (1 / (1 + torch.exp(-x)) - target) * g / x.numel()


def gan_disc_losses(d_real, d_fake, w_real, w_fake):
    """([bce(d_real, 1), bce(d_fake, 0)], w_real d bce / d d_real, w_fake d bce / d d_fake)  (model/nerf_adapt_st_gan.py:139-160)."""
    out = torch.stack([bce_logits_mean(d_real, 1.0), bce_logits_mean(d_fake, 0.0)])
    one = torch.ones((), dtype=d_real.dtype)
    return out, bce_logits_grad(d_real, 1.0, one * w_real), bce_logits_grad(d_fake, 0.0, one * w_fake)


# ------------------------------------------------------------------------------------------ feature-pair loss, R1 value
def feat_pair_loss(feat, w2):
    """feat [4, n] = [fake1 | fake2 | real1 | real2] -> (l1 + w2 l2, l1, l2), l_i = mean((fake_i - real_i)^2)."""
    f = feat.reshape(4, -1)
    n = f.shape[1]
    l1, l2 = ((f[0] - f[2]) ** 2).sum() / n, ((f[1] - f[3]) ** 2).sum() / n
    return l1 + w2 * l2, l1, l2


def feat_pair_loss_grad(feat, w2, g):
    """2 (fake1 - real1) g / n | 2 w2 (fake2 - real2) g / n | 0 | 0: the targets are detached, their quarters exact zeros."""
    f = feat.reshape(4, -1)
    s = 2 * g / f.shape[1]
    z = torch.zeros_like(f[0])
    return torch.stack([s * (f[0] - f[2]), s * w2 * (f[1] - f[3]), z, z]).reshape(feat.shape)


def sumsq_mean(g):
    """sum(g^2) / B for g [B, ...]."""
    return (g * g).sum() / g.shape[0]


def sumsq_mean_grad(g, cot):
    return 2 * cot / g.shape[0] * g


def sumsq_mean_fwd_bwd(g, w):
    """([value, w value], 2 w g / B)."""
    v = sumsq_mean(g)
    return torch.stack([v, w * v]), 2 * w / g.shape[0] * g


# ------------------------------------------------------------------------------------------ K8
def nerf_terms(rgb, uncert, density, gathered):
    """The terms of the four sums: m se / u^2 [B,P], m [B,P], log u^2 [B,P], sigma_transient [B,P,N]."""
    B, P = rgb.shape[0], rgb.shape[1]
    g = gathered.reshape(B, 14, P)
    u = uncert.reshape(B, P)
    d = g[:, 0:3].permute(0, 2, 1) - rgb
    se = (d * d).sum(-1)
    m = g[:, 12]
    return m * (se / (u * u)), m, torch.log(u * u), density[..., 1]


def nerf_losses(rgb, uncert, density, gathered):
    """(sums [4], losses [3] = render, uncert, trans_reg)  (model/nerf_adapt_st_gan.py:747-760)."""
    B, P, N = density.shape[:3]
    sums = torch.stack([x.sum() for x in nerf_terms(rgb, uncert, density, gathered)])
    losses = torch.stack([sums[0] / (sums[1] + 1e-5), 5 + sums[2] / (B * P) / 2, sums[3] / (B * P * N)])
    return sums, losses


def nerf_losses_grad(rgb, uncert, density, gathered, g_losses):
    """(d/d rgb [B,P,3], d/d uncert [B,P], d/d density [B,P,N,2]) for upstream gradients (g_render, g_unc, g_trans); None = 0."""
    B, P, N = density.shape[:3]
    g = gathered.reshape(B, 14, P)
    u = uncert.reshape(B, P)
    m = g[:, 12]
    zero = torch.zeros((), dtype=rgb.dtype)
    g_render, g_unc, g_trans = (zero if x is None else x for x in g_losses)
    gr, gu, gt = g_render / (m.sum() + 1e-5), g_unc / (B * P), g_trans / (B * P * N)
    d = rgb - g[:, 0:3].permute(0, 2, 1)
    se = (d * d).sum(-1)
    iu2 = 1 / (u * u)
    g_rgb = gr * 2 * m[..., None] * d * iu2[..., None]
    g_u = -2 * gr * m * se * iu2 / u + gu / u
    g_d = torch.zeros_like(density)
    g_d[..., 1] = gt
    return g_rgb, g_u, g_d


# ------------------------------------------------------------------------------------------ MaxPool2d(2, 2)
def maxpool2(x):
    """x [n, H, W] -> (y [n, H/2, W/2], arg uint8): the first maximum of each window in row-major order; a NaN replaces whatever is
    held (torch's kernel: `val > max || isnan(val)`), so the last NaN of a window wins."""
    n, H, W = x.shape
    v = x.reshape(n, H // 2, 2, W // 2, 2).permute(0, 1, 3, 2, 4).reshape(n, H // 2, W // 2, 4)
    best, arg = v[..., 0].clone(), torch.zeros(v.shape[:-1], dtype=torch.uint8)
    for k in (1, 2, 3):
        take = (v[..., k] > best) | torch.isnan(v[..., k])
        best = torch.where(take, v[..., k], best)
        arg = torch.where(take, torch.full_like(arg, k), arg)
    return best, arg


def maxpool2_grad(gy, arg):
    """gx [n, H, W]: gy at the window position `arg`, zero at the other three."""
    n, oh, ow = gy.shape
    hit = torch.stack([arg == k for k in range(4)], -1)
    v = torch.where(hit, gy[..., None], torch.zeros((), dtype=gy.dtype))
    return v.reshape(n, oh, ow, 2, 2).permute(0, 1, 3, 2, 4).reshape(n, 2 * oh, 2 * ow)


# ------------------------------------------------------------------------------------------ input stacks
def _consts(like):
    mean = torch.tensor(np.float32(MEAN)).to(like.dtype).view(1, 3, 1, 1)      # the kernel receives float32 statistics
    std = torch.tensor(np.float32(STD)).to(like.dtype).view(1, 3, 1, 1)
    return mean, std


def feat_inputs(rgb, gathered):
    """rgb [B,P,3], gathered [B,14,h,w] -> [4B,3,h,w] = normalised [rgb | rgb m + image (1 - m) | image m + image_syn pad | image],
    pad = (mask_syn == 1 and m == 0)  (model/nerf_adapt_st_gan.py:758-766, layers/perceptual_loss.py:31-37)."""
    B, _, h, w = gathered.shape
    r = rgb.reshape(B, h, w, 3).permute(0, 3, 1, 2)
    image, image_syn, m, ms = gathered[:, 0:3], gathered[:, 3:6], gathered[:, 12:13], gathered[:, 13:14]
    pad = torch.logical_and(ms == 1, m == 0).to(rgb.dtype)
    x = torch.cat([r, r * m + image * (1 - m), image * m + image_syn * pad, image], 0)
    mean, std = _consts(rgb)
    return (x - mean) / std


def feat_inputs_grad(rgb, gathered, g_out):
    """d/d rgb [B,P,3] = (g[fake1] + g[fake2] m) / std."""
    B, _, h, w = gathered.shape
    _, std = _consts(rgb)
    g = g_out[:B] / std + g_out[B:2 * B] / std * gathered[:, 12:13]
    return g.permute(0, 2, 3, 1).reshape(B, h * w, 3)


def disc_inputs(rgb, gathered, geo):
    """(real, fake) [B, 9 or 3, h, w]: real = image m + rgb pad, fake = rgb, both followed by channels 6..11 with `geo`
    (model/nerf_adapt_st_gan.py:478-497)."""
    B, _, h, w = gathered.shape
    r = rgb.reshape(B, h, w, 3).permute(0, 3, 1, 2)
    m, ms = gathered[:, 12:13], gathered[:, 13:14]
    pad = torch.logical_and(ms == 1, m == 0).to(rgb.dtype)
    real, fake = gathered[:, 0:3] * m + r * pad, r
    if geo:
        real, fake = torch.cat([real, gathered[:, 6:12]], 1), torch.cat([fake, gathered[:, 6:12]], 1)
    return real.contiguous(), fake.contiguous()


def fake_patch_grad(g_fake):
    """g_rgb [B,P,3] = channels 0..2 of the cotangent of the fake stack [B,nc,h,w], transposed."""
    B = g_fake.shape[0]
    return g_fake[:, 0:3].reshape(B, 3, -1).permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------------------------------ latent rows, totals, packing
def latent_rows(w_trans, w_light, idx):
    """Embedding.weight[idx] of both tables (model/nerf_adapt_st_gan.py:589-593)."""
    idx = idx.long()
    return w_trans[idx], w_light[idx]


def latent_rows_grad(g_trans, g_light, idx, n_rows):
    """Dense [n_rows, C] tables: row r = the sum over the images b with idx[b] == r in ascending b; rows never hit are zero."""
    out = []
    for g in (g_trans, g_light):
        table = torch.zeros(n_rows, g.shape[1], dtype=g.dtype)
        for b in range(idx.numel()):
            table[int(idx[b])] = table[int(idx[b])] + g[b]
        out.append(table)
    return out


def weighted_sum(terms, weights):
    """sum_k w_k term_k in ascending k; the weights reach the kernel as float32."""
    acc = torch.zeros((), dtype=terms[0].dtype)
    for term, w in zip(terms, weights):
        acc = acc + term * torch.tensor(np.float32(w)).to(term.dtype)
    return acc


def grad_pack(grads, scale, words=None, tail=None):
    """(flat, tail): the concatenation of the gradients times the float32 scale, zeros for (None, numel) entries; tail word k is 1 where
    words[k] != 0 or it was non-zero already (sticky), else 0."""
    dtype = next(g.dtype for g in grads if not isinstance(g, tuple))
    s = torch.tensor(np.float32(scale)).to(dtype)
    flat = torch.cat([torch.zeros(g[1], dtype=dtype) if isinstance(g, tuple) else g.reshape(-1) * s for g in grads])
    if tail is None:
        return flat, None
    set_ = tail != 0
    if words is not None:
        set_ = set_ | (words != 0)
    return flat, set_.to(dtype)


# ------------------------------------------------------------------------------------------ optimisers
def rmsprop_step(p, g, sq, lr, alpha=0.99, eps=1e-8):
    """torch.optim.RMSprop (no momentum, not centred, no weight decay): sq = alpha sq + (1 - alpha) g^2; p -= lr g / (sqrt(sq) + eps).
    -> (p, sq)."""
    sq = alpha * sq + (1 - alpha) * g * g
    return p - lr * (g / (torch.sqrt(sq) + eps)), sq


def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam (no weight decay, no amsgrad); ``step``: this update's number (steps taken before + 1).  -> (p, m, v)."""
    m = m + (g - m) * (1 - beta1)
    v = v * beta2 + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    denom = torch.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


# ------------------------------------------------------------------------------------------ seeded cases (float32, read-only, shared)
@functools.lru_cache(maxsize=None)
def logits_case(n, target, extreme=False):
    """Logits of size about 4 for the BCE kernels (one workgroup of 256 threads); the spikes are logits of 400 on the costly side of
    ``target`` (term 400 against a typical term of about 2).  ``extreme``: the EXTREME_LOGITS, tiled to n, no spikes."""
    rs = np.random.RandomState(1009 * n + 7 * int(target) + 3)
    if extreme:
        return _ro(np.resize(np.array(EXTREME_LOGITS), n))
    x = 4.0 * rs.normal(size=n)
    x[spike_indices(n, 256)] = 400.0 * (1 - 2 * target)
    return _ro(x)


@functools.lru_cache(maxsize=None)
def feat_case(n):
    """feat [4, n] of size about 1 (ReLU outputs: half of them zero); spikes: differences of 50 in both pairs (2500 against about 1)."""
    rs = np.random.RandomState(2003 * n + 1)
    f = np.maximum(rs.normal(size=(4, n)), 0.0)
    for i in spike_indices(n, 1024):
        f[0, i], f[1, i] = f[2, i] + 50.0, f[3, i] - 50.0
    return _ro(f)


@functools.lru_cache(maxsize=None)
def sumsq_case(n, B):
    """g [B, n] float32 of size about 1 (B n elements: the kernels' flat size); spikes of 300 at the flat positions (9e4 against about 1)."""
    rs = np.random.RandomState((3001 * n + B) % (2 ** 31))
    g = rs.normal(size=B * n)
    g[spike_indices(B * n, 1024)] = 300.0
    return _ro(g.reshape(B, n))


MASK_KINDS = ("random", "ones", "zeros", "image0_zero")


@functools.lru_cache(maxsize=None)
def nerf_case(B, P, N, mask_kind="random"):
    """dict(rgb [B,P,3], uncert [B,P,1], density [B,P,N,2], gathered [B,14,P], g [3]) for K8.  uncert in [0.05, 1.5]: seven pixels of
    eight within 3 % of 1 (|log u^2| about 0.03), the others uniform over the whole range.  Spikes at pixels 0, 255, 256, B P - 1: colour
    differences of 10 at u = 0.05 (term 1.2e5 against about 0.5; log u^2 = -6 against 0.03; their mask entry is 1 unless the mask kind
    zeroes it); at density elements 0, 255, 256, B P N - 1: sigma_t = 100 against about 0.5."""
    rs = np.random.RandomState(4001 * B + 17 * P + N + 101 * MASK_KINDS.index(mask_kind))
    rgb = rs.uniform(size=(B, P, 3))
    gathered = rs.uniform(size=(B, 14, P))
    u = np.where(rs.uniform(size=(B, P)) < 0.125, rs.uniform(0.05, 1.5, size=(B, P)), rs.uniform(0.97, 1.03, size=(B, P)))
    density = rs.uniform(size=(B, P, N, 2))
    mask = (rs.uniform(size=(B, P)) > 0.4).astype(np.float64)
    spikes = spike_indices(B * P, 256)
    for q in spikes:
        b, p = divmod(q, P)
        rgb[b, p] = gathered[b, 0:3, p] + 10.0 * np.array([1.0, -1.0, 1.0])
        u[b, p] = 0.05
        mask[b, p] = 1.0
    if mask_kind == "ones":
        mask[:] = 1.0
    elif mask_kind == "zeros":
        mask[:] = 0.0
    elif mask_kind == "image0_zero":
        mask[0] = 0.0
    gathered[:, 12] = mask
    dflat = density.reshape(-1, 2)
    dflat[spike_indices(B * P * N, 256), 1] = 100.0
    return dict(rgb=_ro(rgb), uncert=_ro(u.reshape(B, P, 1)), density=_ro(density), gathered=_ro(gathered),
                g=_ro(np.array([0.9, 1.3, -0.7])), spikes=tuple(spikes))


POOL_VALUES = ("relu", "special")


@functools.lru_cache(maxsize=None)
def pool_case(n, H, W, values="relu"):
    """dict(x [n,H,W], gy [n,H/2,W/2]).  "relu": max(normal, 0) quantised to eighths -- ties in most windows.  "special": the same with
    the leading windows (cyclically) holding +0 / -0 ties, +-inf, and a NaN at each of the four window positions."""
    rs = np.random.RandomState(5003 * n + 31 * H + W + POOL_VALUES.index(values))
    x = np.round(np.maximum(rs.normal(size=(n, H, W)), 0.0) * 8) / 8
    if values == "special":
        windows = [(0.0, -0.0, -0.0, 0.0), (-0.0, 0.0, 0.0, -0.0), (np.inf, 1.0, np.inf, 0.0), (-np.inf, -np.inf, -np.inf, -np.inf),
                   (-np.inf, 2.0, np.inf, 2.0), (np.nan, 1.0, 2.0, 3.0), (3.0, np.nan, 2.0, 1.0), (1.0, 3.0, np.nan, 2.0),
                   (1.0, 2.0, 3.0, np.nan), (np.nan, np.inf, np.nan, 1.0)]
        k = 0
        for img in range(n):
            for oy in range(H // 2):
                for ox in range(W // 2):
                    if k < 2 * len(windows):
                        x[img, 2 * oy:2 * oy + 2, 2 * ox:2 * ox + 2] = np.array(windows[k % len(windows)]).reshape(2, 2)
                    k += 1
    return dict(x=_ro(x), gy=_ro(rs.normal(size=(n, H // 2, W // 2))))


@functools.lru_cache(maxsize=None)
def stack_case(B, h, w):
    """dict(rgb [B,P,3], gathered [B,14,h,w], cot [4B,3,h,w], cot_fake [B,9,h,w]) for the feature / discriminator input stacks.  The two
    masks take the values 0, 1 (half of the pixels each way) and non-binary ones (0.5, 0.999, 1e-7, 1.0000001): the kernels test == 1
    and == 0."""
    rs = np.random.RandomState(6007 * B + 37 * h + w)
    P = h * w
    gathered = rs.uniform(size=(B, 14, h, w))
    values = np.array([0.0, 1.0, 0.0, 1.0, 0.5, 0.999, 1e-7, 1.0000001])
    gathered[:, 12] = values[rs.randint(0, len(values), size=(B, h, w))]
    gathered[:, 13] = values[rs.randint(0, len(values), size=(B, h, w))]
    gathered[-1, 12:14, -1, -1] = 1.0                    # (both masks set, and below: the padded kind, in every case however small)
    gathered[0, 12, 0, 0], gathered[0, 13, 0, 0] = 0.0, 1.0
    return dict(rgb=_ro(rs.uniform(size=(B, P, 3))), gathered=_ro(gathered), cot=_ro(rs.normal(size=(4 * B, 3, h, w))),
                cot_fake=_ro(rs.normal(size=(B, 9, h, w))))


@functools.lru_cache(maxsize=None)
def latent_case(B=5, n_rows=9, Ct=17, Cl=13):
    """dict(w_trans [n_rows,Ct], w_light [n_rows,Cl], idx [B] int64 with a repeated row and rows never hit, g_trans, g_light)."""
    rs = np.random.RandomState(7001 * B + 41 * n_rows + Ct + Cl)
    idx = rs.randint(0, n_rows, size=B)
    idx[-1] = idx[0]                                     # a repeated row: two images add into it
    return dict(w_trans=_ro(rs.normal(size=(n_rows, Ct))), w_light=_ro(rs.normal(size=(n_rows, Cl))), idx=_ro(idx, np.int64),
                g_trans=_ro(rs.normal(size=(B, Ct))), g_light=_ro(rs.normal(size=(B, Cl))))


@functools.lru_cache(maxsize=None)
def terms_case(n):
    """(terms [n], weights [n]) of size about 1 for the weighted loss sum."""
    rs = np.random.RandomState(8009 + n)
    return _ro(rs.normal(size=n)), _ro(rs.uniform(0.5, 2.0, size=n))


def split_total(total, numels):
    """``numels`` repeated cyclically until they add up to ``total`` (the last one cut or extended to fit)."""
    out, k = [], 0
    while sum(out) < total:
        out.append(min(numels[k % len(numels)], total - sum(out)))
        k += 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def optim_case(numels, n_steps, scale_exp0, tiny=False):
    """dict(p [total], g [n_steps, total]) for an optimiser run over tensors of the given numels (flat; callers split): parameters of
    size about 1, gradients normal times 10^(it + scale_exp0) at step it.  ``tiny``: the first tensor's gradients are exactly 0 in their
    first half and about 1e-20 in the second (the squared average goes denormal; eps alone keeps the quotient finite)."""
    total = int(sum(numels))
    rs = np.random.RandomState((9001 * total + 43 * len(numels) + n_steps) % (2 ** 31))
    p = rs.normal(size=total)
    g = np.stack([rs.normal(size=total) * 10.0 ** (it + scale_exp0) for it in range(n_steps)])
    if tiny:
        n0 = numels[0]
        g[:, :n0 // 2] = 0.0
        g[:, n0 // 2:n0] = 1e-20 * rs.normal(size=(n_steps, n0 - n0 // 2))
    return dict(p=_ro(p), g=_ro(g))
