"""numpy restatement of K42 (tp_robust_weight) -- the rule, the three-level radix select -- and of FaceTexelFitter's robust loop, written
from the contract in include/texpose_amd.h (not from the kernel or the module), with the corruption recipe of the round trip and the
figures the tests pin."""
import os

import numpy as np

import face_texel_fit_ref as FIT

TUKEY, HUBER = "tukey", "huber"
DEFAULT_C = {TUKEY: 4.685, HUBER: 1.345}
SIGMA_MIN = np.float32(1.0 / 255.0)
LAM, ITERS, ROUNDS = 0.1, 4, 6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robust_fit.npz")


# ---- the rule
def q_of(model, image, weight=None):
    """-> q [B,H,W] float32 (rule 1: fp64, rounded once) and counted [B,H,W] bool (rule 2)"""
    model, image = np.asarray(model, np.float32), np.asarray(image, np.float32)
    with np.errstate(all="ignore"):
        e = image.astype(np.float64) - model.astype(np.float64)
        q = (((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]) / 3.0).astype(np.float32)
        counted = np.isfinite(model).all(-1) & np.isfinite(image).all(-1) & np.isfinite(q)
        if weight is not None:
            w = np.asarray(weight, np.float32)
            counted &= np.isfinite(w) & (w > 0)
    return q, counted


def radix_select(q, rank=None):
    """The element of rank (n - 1) // 2 of the non-negative float32 values ``q`` [n] WITHOUT a sort: three levels over the bit patterns
    (the upper 11 bits, the next 11, the last 10), each one histogram and a walk along its cumulative counts -> (value float32, the three
    bins).  n = 0: 0."""
    keys = np.ascontiguousarray(np.asarray(q, np.float32)).view(np.uint32).astype(np.int64)
    n = len(keys)
    if n == 0:
        return np.float32(0.0), ()
    rank = (n - 1) // 2 if rank is None else int(rank)
    prefix, bins = 0, []
    for bits, shift in ((11, 21), (11, 10), (10, 0)):
        under = keys[(keys >> (shift + bits)) == prefix]
        hist = np.bincount((under >> shift) & ((1 << bits) - 1), minlength=1 << bits)
        upto = np.cumsum(hist)
        b = int(np.searchsorted(upto, rank, side="right"))              # the first bin whose cumulative count exceeds the rank
        rank -= int(upto[b] - hist[b])
        prefix = (prefix << bits) | b
        bins.append(b)
    return np.array([prefix], np.uint32).view(np.float32)[0], tuple(bins)


def robust_weight_ref(model, image, weight=None, kind=TUKEY, c=None, sigma_min=SIGMA_MIN, scale_in=None, select=radix_select):
    """The header's K42 block -> dict(weight [B,H,W] float32, median_q [B] float32, scale [B] float32, count [B] int32, q, counted)."""
    q, counted = q_of(model, image, weight)
    B = q.shape[0]
    c = np.float32(DEFAULT_C[kind] if c is None else c)
    base = np.ones(q.shape, np.float32) if weight is None else np.asarray(weight, np.float32)
    floor = np.float64(np.float32(sigma_min)) * np.float64(np.float32(sigma_min))
    out, median_q, scale, count = np.zeros(q.shape, np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros(B, np.int32)
    for b in range(B):
        on = counted[b]
        count[b] = on.sum()
        if scale_in is None:
            median_q[b] = select(q[b][on])[0]
            s2 = np.fmax((1.4826 * 1.4826) * np.float64(median_q[b]), floor)
        else:
            s = np.float64(np.float32(scale_in[b]))
            with np.errstate(all="ignore"):
                s2 = np.fmax(s * s, floor)
        scale[b] = np.float32(np.sqrt(s2))
        with np.errstate(all="ignore"):
            u2 = q[b][on].astype(np.float64) / ((np.float64(c) * np.float64(c)) * s2)
            if kind == TUKEY:
                w = np.where(u2 < 1.0, (1.0 - u2) * (1.0 - u2), 0.0)
            else:
                w = np.where(u2 <= 1.0, 1.0, 1.0 / np.sqrt(u2))
        out[b][on] = (base[b][on].astype(np.float64) * w).astype(np.float32)
    return dict(weight=out, median_q=median_q, scale=scale, count=count, q=q, counted=counted)


# ---- the corruption of the round trip (the issue's recipe, literally)
def corrupt(rgb, covered, noise=0.0, seed=42):
    """rgb [B,H,W,3] in [0, 1], covered [B,H,W] bool -> the photographs with a constant-colour rectangle in every third view and a Gaussian
    highlight in every view, both on covered pixels only; ``noise``: sigma of the sensor noise added to EVERY pixel afterwards."""
    rgb = np.array(rgb, dtype=np.float32)
    B, H, W = covered.shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for b in range(B):
        if b % 3 == 0:
            y, x = 18 + 3 * (b % 4), 20 + 2 * (b % 5)
            box = np.zeros((H, W), bool)
            box[y:y + 18, x:x + 16] = True
            rgb[b][box & covered[b]] = (0.9, 0.1, 0.1) if b % 2 == 0 else (0.05, 0.05, 0.05)
        cy, cx = 26 + (5 * b) % 11, 36 - (3 * b) % 9                    # (row, column), as the rectangle is given
        glow = 0.7 * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2.0 * 2.5 ** 2))
        lit = np.minimum(rgb[b] + glow[..., None].astype(np.float32), np.float32(1.0))
        rgb[b] = np.where(covered[b][..., None], lit, rgb[b])
    if noise > 0:
        rgb = rgb + np.random.RandomState(seed).normal(0.0, noise, rgb.shape).astype(np.float32)
    return rgb


def corrupted_share(clean, dirty, weight):
    """per view: the share of the weighted pixels that changed by more than 0.05 in a channel"""
    changed = (np.abs(np.asarray(dirty, np.float64) - np.asarray(clean, np.float64)).max(-1) > 0.05) & (np.asarray(weight) > 0)
    return changed.sum((1, 2)) / np.maximum((np.asarray(weight) > 0).sum((1, 2)), 1)


# ---- the robust loop
def robust_fit_loop(views, rgb, weight, prior, start, lam=LAM, iters=ITERS, rounds=ROUNDS, kind=TUKEY, c=None, sigma_min=SIGMA_MIN,
                    weighted_preconditioner=True, dtype=np.float64):
    """FaceTexelFitter(robust=kind).fit: per round the weights of the header's rule from the current x per view (the model plane is S x in
    float32, zero where nothing is shaded), then ``iters`` steps of conjugate gradients on (S^T w S + lam) x = S^T w I + lam prior from x,
    preconditioned with S^T (w) + lam -> dict(nodes, coverage, rms [rounds * iters + 1], scale, kept, count).  ``views``: a
    face_texel_fit_ref.Views of the same rgb [B,H,W,3] and weight [B,H,W] planes."""
    valid = views.valid
    rgb32, base32 = np.asarray(rgb, np.float32), np.asarray(weight, np.float32)
    x, prior = np.array(start, dtype=dtype), np.asarray(prior, dtype=dtype)
    S = lambda v: views.shade(v.astype(np.float64)).astype(dtype)
    St = lambda g: views.adjoint(g.astype(np.float64)).astype(dtype)
    image = views.rgb.astype(dtype)
    coverage, rms = views.coverage(), []
    for _ in range(rounds):
        model = np.zeros(valid.shape + (3,), np.float32)
        model[valid] = S(x).astype(np.float32)
        fit = robust_weight_ref(model, rgb32, base32, kind, c, sigma_min)
        w64 = fit["weight"][valid].astype(np.float64)
        w, total = w64.astype(dtype)[:, None], float(w64.sum())
        rms_of = lambda v: float(np.sqrt((w64[:, None] * (S(v).astype(np.float64) - views.rgb) ** 2).sum() / (3.0 * max(total, 1e-300))))
        if not rms:
            rms.append(rms_of(x))
        pre = np.bincount(views.dest.reshape(-1), (views.w * w64[:, None]).reshape(-1), views.U) if weighted_preconditioner else coverage
        m_inv = (1.0 / (pre[:, None] + lam)).astype(dtype)
        r = St(w * (image - S(x))) + dtype(lam) * (prior - x)
        x = FIT.pcg(x, r, m_inv, lambda p: St(w * S(p)) + dtype(lam) * p, lambda v: rms.append(rms_of(v)), iters, dtype)
    kept = fit["weight"].astype(np.float64).sum((1, 2)) / np.maximum(np.where(base32 > 0, base32, 0).astype(np.float64).sum((1, 2)), 1e-300)
    return dict(nodes=x, coverage=coverage, rms=np.array(rms), scale=fit["scale"], kept=kept, count=fit["count"])


# ---- measured by tests/test_robust_weight_cpu.py with this file's loop (fp64 vectors), pinned there and in tests/golden/robust_fit.npz
# Section 26's shrunk round trip (sphere, 14 Fibonacci views, 64 x 64, f = 200, R = 4, lam = 0.1; prior and start the bake of the photographs
# themselves; held-out view sphere_view_poses(5, 400)[1]) with corrupt() painted into the photographs; Tukey, 6 rounds x 4 iterations:
#   case: (held-out PSNR of the bake, of the plain fit (4 iterations), of the robust fit)
ROBUST_FIT = {"corrupted": (19.62, 20.60, 32.97), "noisy": (19.61, 20.57, 32.95), "clean": (26.05, 34.10, 34.08)}
#   ("noisy": sigma = 0.02 sensor noise on every pixel besides; "clean": the photographs as they are -- the robust fit costs 0.02 dB there)
#   the robust fit's held-out PSNR after every round ("corrupted"), and sigma per view after the last
ROBUST_FIT_BY_ROUND = (25.78, 29.08, 30.55, 31.55, 32.35, 32.97)
ROBUST_FIT_SCALE = (0.020839, 0.019721, 0.020885, 0.025166, 0.024716, 0.025150, 0.026157, 0.025350, 0.023392, 0.024813, 0.022820, 0.021048, 0.022307,
                    0.017488)
# the same loop with Huber's weight ends at 29.03 dB, with Tukey's and the unweighted preconditioner coverage + lam at 30.95 dB; between 5.5 %
# and 19.0 % of a view's weighted pixels are changed by more than 0.05 (9.7 % overall; with the noise up to 22.6 %)
