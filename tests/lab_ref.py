"""The Lab chroma loss in numpy fp64, with its analytic gradient: what tests/test_lab_cpu.py and tests/test_gpu_lab_loss.py measure
texpose_amd/lab.py and the K23 kernels against.

The rule (reference layers/lab_loss.py:13-48 around kornia.color.rgb_to_lab as published; kornia itself is not a dependency, so
nothing here is pinned to a call of it):
  linear  = c > 0.04045 ? ((c + 0.055) / 1.055) ** 2.4 : c / 12.92                               per channel (R, G, B)
  X, Y, Z = the sRGB / D65 matrix below times linear;   t = (X / 0.95047, Y, Z / 1.08883)
  f(t)    = t > 0.008856 ? cbrt(max(t, 0.008856)) : 7.787 t + 4 / 29        (the gradient follows the selected branch)
  L = 116 f(Y) - 16,  a = 500 (f(X) - f(Y)),  b = 200 (f(Y) - f(Z));   normalised: L / 100, (a + 127) / 254, (b + 127) / 254
  loss    = SmoothL1(beta = 1) of the two normalised chroma channels, fake against real; with a mask [B,1,h,w]
            sum(l * mask) / sum(mask) (no epsilon: an empty mask gives NaN), else the mean over all 2 B h w elements
Images are [B,3,...] with any trailing shape."""
import numpy as np

SRGB_THRESHOLD, LAB_THRESHOLD = 0.04045, 0.008856
RGB_TO_XYZ = np.array([[0.412453, 0.357580, 0.180423],
                       [0.212671, 0.715160, 0.072169],
                       [0.019334, 0.119193, 0.950227]])
WHITE = np.array([0.95047, 1.0, 1.08883])


def _cshape(img):
    return (1, 3) + (1,) * (img.ndim - 2)


def linearise(img):
    img = np.asarray(img, dtype=np.float64)
    gamma = img > SRGB_THRESHOLD
    u = np.where(gamma, (img + 0.055) / 1.055, 1.0)
    return np.where(gamma, u ** 2.4, img / 12.92)


def xyz_normalised(img):
    """t = XYZ / white of an sRGB image [B,3,...]."""
    lin = linearise(img)
    return np.einsum("kc,bc...->bk...", RGB_TO_XYZ, lin) / WHITE.reshape(_cshape(lin))


def _f(t):
    root = t > LAB_THRESHOLD
    return np.where(root, np.cbrt(np.where(root, t, 1.0)), 7.787 * t + 4.0 / 29.0)


def rgb_to_lab(img):
    f = _f(xyz_normalised(img))
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    return np.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)], axis=1)


def normalize_lab(lab):
    lo = np.array([0.0, -127.0, -127.0]).reshape(_cshape(lab))
    hi = np.array([100.0, 127.0, 127.0]).reshape(_cshape(lab))
    return (lab - lo) / (hi - lo)


def smooth_l1(d):
    a = np.abs(d)
    return np.where(a < 1.0, 0.5 * d * d, a - 0.5)


def lab_loss(fake, real, mask=None):
    """-> (loss, fake_lab with real_lab's L plane, real_lab)."""
    fl, rl = normalize_lab(rgb_to_lab(fake)), normalize_lab(rgb_to_lab(real))
    l = smooth_l1(fl[:, 1:] - rl[:, 1:])
    if mask is None:
        loss = l.mean()
    else:
        mask = np.asarray(mask, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            loss = (l * mask).sum() / mask.sum()
    vis = fl.copy()
    vis[:, 0] = rl[:, 0]
    return loss, vis, rl


def lab_loss_grad(fake, real, mask=None):
    """d loss / d fake, analytic, with the shape of ``fake``."""
    fake = np.asarray(fake, dtype=np.float64)
    fl, rl = normalize_lab(rgb_to_lab(fake)), normalize_lab(rgb_to_lab(real))
    d = fl[:, 1:] - rl[:, 1:]
    g_chroma = np.where(np.abs(d) < 1.0, d, np.sign(d))                       # d l / d (a_n, b_n)
    with np.errstate(invalid="ignore", divide="ignore"):
        if mask is None:
            g_chroma = g_chroma / d.size
        else:
            mask = np.asarray(mask, dtype=np.float64)
            g_chroma = g_chroma * (mask / mask.sum())
        ga, gb = g_chroma[:, 0] * (500.0 / 254.0), g_chroma[:, 1] * (200.0 / 254.0)
        t = xyz_normalised(fake)
        root = t > LAB_THRESHOLD
        df = np.where(root, np.cbrt(np.where(root, t, 1.0)) / (3.0 * np.where(root, t, 1.0)), 7.787)
        g_t = np.stack([ga, gb - ga, -gb], axis=1) * df                       # wrt t = (X / Xn, Y, Z / Zn)
        g_lin = np.einsum("kc,bk...->bc...", RGB_TO_XYZ, g_t / WHITE.reshape(_cshape(t)))
        gamma = fake > SRGB_THRESHOLD
        u = np.where(gamma, (fake + 0.055) / 1.055, 1.0)
        return g_lin * np.where(gamma, (2.4 / 1.055) * u ** 1.4, 1.0 / 12.92)


def draw_colours(rs, shape, margin_srgb=0.0, margin_lab=0.0, max_rounds=100):
    """Seeded colours [B,3,...] (float32): uniform in [0,1] with every eighth pixel in the band [-0.1, 0) and every eighth in
    (1, 1.2].  With margins, pixels with a channel within ``margin_srgb`` of 0.04045 or a normalised X / Y / Z within ``margin_lab``
    of 0.008856 are redrawn (the derivative jumps by ~1 % across either threshold): -> (colours, number of rounds needed)."""
    B, n = shape[0], int(np.prod(shape[2:]))

    def draw(count):
        c = rs.uniform(0.0, 1.0, size=(count, 3))
        kind = rs.randint(0, 8, size=count)
        c[kind == 0] = rs.uniform(-0.1, 0.0, size=(int((kind == 0).sum()), 3))
        c[kind == 1] = 1.2 - rs.uniform(0.0, 0.2, size=(int((kind == 1).sum()), 3))           # (1, 1.2]
        dark = kind == 2                                  # (some pixels dark enough for the linear branch of f)
        c[dark] = rs.uniform(0.0, 0.12, size=(int(dark.sum()), 3))
        return c.astype(np.float32)

    def near(c):
        t = xyz_normalised(c.astype(np.float64)[:, :, None])[:, :, 0]
        return (np.abs(c.astype(np.float64) - SRGB_THRESHOLD) < margin_srgb).any(1) | (np.abs(t - LAB_THRESHOLD) < margin_lab).any(1)

    c = draw(B * n)
    rounds = 1
    while margin_srgb > 0 or margin_lab > 0:
        bad = near(c)
        if not bad.any():
            break
        if rounds >= max_rounds:
            raise RuntimeError("draw_colours: the rejection did not terminate")
        c[bad] = draw(int(bad.sum()))
        rounds += 1
    return np.ascontiguousarray(c.reshape(B, n, 3).transpose(0, 2, 1)).reshape(shape), rounds
