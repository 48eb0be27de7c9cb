"""The exposure contract of DESIGN section 27 (kernel K37: tp_photo_exposure), said again in numpy fp64 -- written from the rules in
include/texpose_amd.h, not from the kernels.  Where the kernel is free to choose, this file chooses differently: the keep rule is a
whole-plane mask, the sixteen sums are np.sum over an image's kept pixels at once (the kernel adds per thread, wave, workgroup and
tile), and the loop is tests/photo_ref.py's, on its brute-force raster, with the fit in front of each step_ref.

Besides the results it reports what decides whether a comparison of counts can be exact: near-ties, kept-or-dropped decisions whose
margin | |o - (a c + d)| - tau | is below NEAR_TIE colour units.

FIGURES, measured on this file's loops (CPU, numpy, photo_ref's raster; tests/test_photo_exposure_cpu.py asserts them against TABLE):
photo_ref's four loop cases at 64 x 80, start 3 deg and 6.08 / 8.06 mm away, tau 0.5, ten steps, the photograph replaced by
EXPOSURE_GAIN * image + EXPOSURE_BIAS per channel, background included.
    case       plain photo_ref loop, end     this file's loop, end         recovered gain, worst channel
    sphere 0   0.355 deg  7.506 mm           0.1386 deg  0.3104 mm         0.7482 for 0.75
    sphere 1   1.290 deg  5.618 mm           0.0001 deg  0.0001 mm         exact to fp32
    torus 0    0.363 deg  8.909 mm           0.0661 deg  0.5498 mm         0.6991 for 0.70
    torus 1    0.324 deg 12.706 mm           0.0000 deg  0.0001 mm         exact to fp32
The plain loop ends no closer in translation than 0.69 of its start (rms 0.19 throughout); the compensated loop below a quarter of its
start on all four.  With photo_ref's noise (sigma 0.02, added after the change) it ends at <= 0.27 deg and <= 0.39 mm; on the
unchanged photographs at <= 0.039 deg and <= 0.031 mm, where the plain loop ends at <= 0.037 deg and <= 0.027 mm.  The prototype's
table in the feature's request agrees to its rounding except for the rotations of the two cases '1' (0.006 and 0.007 deg there): here
every pass refits, the final evaluation included, and those two cases recover gain and bias to fp32 rounding."""
import functools

import numpy as np

import photo_ref as PR
import pnp_ref as PREF
from gn_ref import loop_ref
from icp_ref import frame_index

NEAR_TIE = 1e-9          # colour units
MIN_COUNT = 6
CLAMPED, FLAT = 1, 8     # flags: << channel

EXPOSURE_GAIN = np.array([0.75, 0.80, 0.70])
EXPOSURE_BIAS = np.array([0.05, 0.10, 0.08])

# (mesh, image) -> the plain loop's end (deg, mm) and this file's loop's end (deg, mm) on the clean exposure-changed photographs
TABLE = {("sphere", 0): (0.355, 7.506, 0.1386, 0.3104), ("sphere", 1): (1.290, 5.618, 0.0001, 0.0001),
         ("torus", 0): (0.363, 8.909, 0.0661, 0.5498), ("torus", 1): (0.324, 12.706, 0.0000, 0.0001)}


def fit_ref(zbuf, rgb, image, tau, gain_in=None, bias_in=None, mask=None, gain_range=(0.25, 4.0), min_var=1e-6):
    """One image: zbuf / mask [H,W], rgb / image [H,W,3], gain_in / bias_in [3] or None -> dict(gain [3] float32, bias [3] float32,
    count, rms (fp64), status, flags, near_ties, kept [H,W] bool)."""
    z32, c32, o32 = np.asarray(zbuf, np.float32), np.asarray(rgb, np.float32), np.asarray(image, np.float32)
    H, W = z32.shape
    a32 = np.ones(3, np.float32) if gain_in is None else np.asarray(gain_in, np.float32)
    d32 = np.zeros(3, np.float32) if bias_in is None else np.asarray(bias_in, np.float32)
    tau, lo, hi, min_var = (float(np.float32(v)) for v in (tau, gain_range[0], gain_range[1], min_var))
    with np.errstate(all="ignore"):
        c, o = c32.astype(np.float64), o32.astype(np.float64)
        keep = np.zeros((H, W), bool)
        keep[1:-1, 1:-1] = True                                  # (H < 3 or W < 3: nothing)
        keep &= (z32 > 0) & np.isfinite(z32)
        if mask is not None:
            keep &= np.asarray(mask) != 0
        keep &= np.isfinite(c).all(-1) & np.isfinite(o).all(-1)
        r = o - (a32.astype(np.float64) * c + d32.astype(np.float64))
        d2 = (r[..., 0] ** 2 + r[..., 1] ** 2) + r[..., 2] ** 2
        ties = int((keep & (np.abs(np.sqrt(d2) - tau) < NEAR_TIE)).sum())
        keep &= d2 <= tau * tau
        n = float(keep.sum())
        ck, ok = c[keep], o[keep]                                # [n,3]
        mc, mo = ck.sum(0) / n, ok.sum(0) / n
        var, cov, voo = (ck * ck).sum(0) / n - mc * mc, (ck * ok).sum(0) / n - mc * mo, (ok * ok).sum(0) / n - mo * mo
        g, flags = np.ones(3), 0
        for k in range(3):
            if var[k] > min_var:
                q = cov[k] / var[k]
                g[k] = min(max(q, lo), hi)
                flags |= (CLAMPED << k) if g[k] != q else 0
            else:
                flags |= FLAT << k
        b = mo - g * mc
        sse = n * ((voo - 2.0 * (g * cov)) + (g * g) * var)
        rms = np.sqrt(np.maximum(0.0, (sse[0] + sse[1]) + sse[2]) / n)
        g32, b32 = g.astype(np.float32), b.astype(np.float32)
    status = 1 if n < MIN_COUNT else (0 if np.isfinite(g32).all() and np.isfinite(b32).all() and np.isfinite(np.float32(rms)) else 3)
    return dict(gain=g32 if status == 0 else a32.copy(), bias=b32 if status == 0 else d32.copy(), count=int(n), rms=float(rms), status=status,
                flags=flags, near_ties=ties, kept=keep)


def apply_ref(zbuf, rgb, gain, bias):
    """rgb [..,H,W,3] under gain / bias [..,3] (fp32: a product, then a sum) on the pixels with a surface, the rest unchanged."""
    z32, c32 = np.asarray(zbuf, np.float32), np.asarray(rgb, np.float32)
    with np.errstate(all="ignore"):
        lit = np.asarray(gain, np.float32)[..., None, None, :] * c32
        lit = lit + np.asarray(bias, np.float32)[..., None, None, :]
        return np.where(((z32 > 0) & np.isfinite(z32))[..., None], lit, c32).astype(np.float32)


def exposure_ref(zbuf, rgb, image, tau, gain_in=None, bias_in=None, frame=None, mask=None, gain_range=(0.25, 4.0), min_var=1e-6):
    """The whole call: zbuf [B,H,W], rgb [B,H,W,3], image [Ft,H,W,3] (and mask [Ft,H,W]), gain_in / bias_in [B,3] or None ->
    dict(gain, bias [B,3] float32, count, status, flags, near_ties [B], rms [B] fp64, kept [B,H,W], rgb [B,H,W,3] float32)."""
    B = len(zbuf)
    image = np.asarray(image, np.float32)
    fr = frame_index(B, len(image), frame)
    per = [fit_ref(zbuf[b], rgb[b], image[fr[b]], tau, None if gain_in is None else gain_in[b], None if bias_in is None else bias_in[b],
                   None if mask is None else np.asarray(mask)[fr[b]], gain_range, min_var) for b in range(B)]
    out = {k: np.stack([np.asarray(p[k]) for p in per]) for k in per[0]}
    out["rgb"] = apply_ref(zbuf, rgb, out["gain"], out["bias"])
    return out


def photo_exposure_loop_ref(verts, faces, vcolor, pose, K, image, tau=0.5, iters=10, damping=1e-6, frame=None, mask=None, tau0=2.0,
                            gain_range=(0.25, 4.0), min_var=1e-6):
    """ops.photo_align(exposure=True) on photo_ref's own raster: every pass fits (the first within tau0 of the plain colours, the
    later ones within that pass's tau of the fit before), rewrites the rendered colours and hands them to step_ref -> loop_ref's
    dict and gain, bias [B,3], exposure_status [B] of the last pass; near_ties counts the fits' too."""
    image = np.asarray(image, np.float32)
    H, W = image.shape[1:3]
    fit, ties = {}, [np.zeros(len(pose), np.int64)]
    render = lambda P: [PR.render_ref(verts, faces, vcolor, P[b], K[b], H, W) for b in range(len(P))]

    def step(planes, P, t, last):
        zbuf, rgb = np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])
        e = exposure_ref(zbuf, rgb, image, t if fit else tau0, fit.get("gain"), fit.get("bias"), frame, mask, gain_range, min_var)
        fit.update(gain=e["gain"], bias=e["bias"], exposure_status=e["status"])
        ties[0] = np.maximum(ties[0], e["near_ties"])
        return PR.step_ref(zbuf, e["rgb"], P, K, image, t, damping, frame, mask, evaluate_only=last)

    out = loop_ref(render, step, pose, tau, iters)
    return dict(out, near_ties=np.maximum(out["near_ties"], ties[0]), **fit)


# ----------------------------------------------------------------------------------------------------------------- the loop's cases
def changed(image, gain=EXPOSURE_GAIN, bias=EXPOSURE_BIAS):
    """The photograph under another exposure: gain * image + bias per channel in fp64, background included, rounded to fp32."""
    return (np.asarray(image, np.float64) * gain + bias).astype(np.float32)


@functools.lru_cache(maxsize=None)
def loop_inputs(mesh, noisy):
    """photo_ref.loop_inputs with the exposure-changed photograph; where ``noisy``, photo_ref's own noise (sigma 0.02) is added AFTER
    the change, at its full size, as a sensor would."""
    c, clean = PR.loop_inputs(mesh, noisy), PR.loop_inputs(mesh, False)["image"]
    noise = c["image"].astype(np.float64) - clean
    return dict(c, image=(changed(clean).astype(np.float64) + noise).astype(np.float32), plain_image=c["image"])


@functools.lru_cache(maxsize=None)
def loop_case(mesh, noisy, compensated=True, exposed=True):
    """One loop (10 steps, tau 0.5, damping 1e-6), run once per case and shared by the test files: ``compensated`` this file's loop,
    else photo_ref's plain one; ``exposed`` on the exposure-changed photograph, else on photo_ref's own."""
    c = loop_inputs(mesh, noisy)
    image = c["image"] if exposed else c["plain_image"]
    loop = photo_exposure_loop_ref if compensated else PR.photo_ref
    return dict(c, image=image, want=loop(c["verts"], c["faces"], c["vcolor"], c["start"], c["K"], image, 0.5, 10, 1e-6))


def errors(c, pose):
    """[(deg, mm)] per image of ``pose`` against the case's truth."""
    return [PREF.pose_error(np.asarray(pose)[b], c["P"][b]) for b in range(len(c["P"]))]


# ----------------------------------------------------------------------------------------------------------------- one call, exact inputs
def one_call_case(seed, B, H, W, frames="one", with_mask=False, with_fit=False):
    """Hand-built planes for one call, as photo_ref.one_step_case: zbuf 880 .. 920 mm on 60 % of the pixels, rgb uniform in [0, 1],
    image = g rgb + b + U(-0.2, 0.2) with g in [0.6, 1.4] and b in [-0.1, 0.1] per image and channel, 2 % of the values of zbuf, rgb
    and image NaN or +-Inf plus one of each planted by hand.  ``with_fit``: gain_in / bias_in near (g, b), as a pass before would have
    left them (tau = 0.5 then keeps most pixels; without them it judges by the plain colour difference)."""
    rs = np.random.RandomState(seed)
    Ft = dict(one=1, each=B, map=2)[frames]
    frame = np.array([7, -3, 1, 0, 2 ** 30, -2 ** 31][:B] if B <= 6 else np.arange(B) % 2, np.int32) if frames == "map" else None
    fr = frame_index(B, Ft, frame)
    zbuf = rs.uniform(880.0, 920.0, (B, H, W)).astype(np.float32)
    zbuf[rs.uniform(size=zbuf.shape) < 0.4] = -1.0
    rgb = rs.uniform(0.0, 1.0, (B, H, W, 3)).astype(np.float32)
    g, b = rs.uniform(0.6, 1.4, (B, 3)), rs.uniform(-0.1, 0.1, (B, 3))
    image = rs.uniform(0.0, 1.0, (Ft, H, W, 3)).astype(np.float32)
    for i in range(B):                                           # (with a shared photograph the later images overwrite: still a valid case)
        image[fr[i]] = (g[i] * rgb[i] + b[i] + rs.uniform(-0.2, 0.2, (H, W, 3))).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    for plane in (zbuf, rgb, image):
        flat = plane.reshape(-1)
        hit = rs.uniform(size=flat.shape) < 0.02
        flat[hit] = bad[rs.randint(0, 3, int(hit.sum()))]
        for value in bad:
            flat[rs.randint(len(flat))] = value
    mask = (rs.uniform(size=(Ft, H, W)) < 0.8).astype(np.uint8) if with_mask else None
    gain_in = (g + rs.uniform(-0.05, 0.05, (B, 3))).astype(np.float32) if with_fit else None
    bias_in = (b + rs.uniform(-0.02, 0.02, (B, 3))).astype(np.float32) if with_fit else None
    return dict(zbuf=zbuf, rgb=rgb, image=image, frame=frame, mask=mask, gain_in=gain_in, bias_in=bias_in, tau=0.5, true_gain=g, true_bias=b)


# ----------------------------------------------------------------------------------------------------------------- the joint loop
# One of DESIGN section 23's occluded cases (joint_ref.CASES).  Measured on joint_case() below for all six, from 8 degrees at the fine
# texture (v / 3), errors in deg / mm per image:       exposure-changed, this file's loop        unchanged, joint_ref's loop
#   bent sphere, bottom third                          0.056 / 0.086   0.925 / 12.272            0.057 / 0.064   0.159 / 0.331
#   bent torus,  bottom third                          0.248 / 0.751   21.4  / 329.8             0.129 / 0.105   0.177 / 0.381
#   bent sphere, corner disc                           0.026 / 0.164   0.198 / 0.123             0.031 / 0.198   0.063 / 0.121
#   bent torus,  corner disc                           0.063 / 0.063   11.1  / 205.8             0.074 / 0.076   0.130 / 0.198
#   bent sphere, right half                            0.076 / 0.261   0.912 / 5.677             0.107 / 0.282   0.282 / 1.231
#   bent torus,  right half                            0.031 / 0.922   10.3  / 27.7              0.134 / 2.411   0.136 / 0.217
# Image 1 of the bent torus is LOST with the fit in the loop: that far from the pose the fine texture is uncorrelated with the
# photograph, the regression's gain falls to the clamp (0.25) with a large bias, the rendering goes flat and the photometric term
# stops pulling.  The GPU test takes the case whose two images both converge here.
JOINT_CASE = ("bent sphere", "corner disc")


def joint_exposure_loop_ref(name, texture, pose, K, sdf, image, photo_mask, weights=None, tau_px=4.0, tau=0.5, iters=20, damping=1e-6, tau0=2.0):
    """joint_ref.joint_ref (silhouette + photometric, its own raster) with the fit in front of each step, as
    ops.joint_align(exposure=True): the photometric term's mask is the fit's -> loop_ref's dict and photo_gain, photo_bias [B,3],
    photo_exposure_status [B] of the last pass."""
    import joint_ref as JREF
    H, W = np.asarray(sdf).shape[1:3]
    fit = {}
    render = lambda P: [JREF.render_ref(name, texture, P[b], K[b], H, W) for b in range(len(P))]

    def step(r, P, t, last):
        z, rgb = np.stack([p[0] for p in r]), np.stack([p[1] for p in r])
        e = exposure_ref(z, rgb, image, tau if fit else tau0, fit.get("photo_gain"), fit.get("photo_bias"), None, photo_mask)
        fit.update(photo_gain=e["gain"], photo_bias=e["bias"], photo_exposure_status=e["status"])
        got = JREF.step_ref(P, K, sil=dict(zbuf=z, sdf=sdf, tau_px=tau_px), photo=dict(zbuf=z, rgb=e["rgb"], image=image, tau=tau, mask=photo_mask),
                            weights=JREF.WEIGHTS if weights is None else weights, damping=damping, evaluate_only=last)
        got["rms"] = got["chi2"]
        return got

    return dict(loop_ref(render, step, pose, 0.0, iters), **fit)


@functools.lru_cache(maxsize=None)
def joint_case(compensated=True):
    """JOINT_CASE of joint_ref's table (two images, the occluder's pixels unknown, noise 0.02, start 8 degrees away) with the
    photograph under EXPOSURE_GAIN / EXPOSURE_BIAS (occluder, background and noise included), through this file's joint loop, or
    through joint_ref's plain one; run once and shared."""
    import joint_ref as JREF
    c = JREF.table_inputs(*JOINT_CASE)
    image = changed(c["image"])
    with np.errstate(all="ignore"):
        if compensated:
            want = joint_exposure_loop_ref(JOINT_CASE[0], c["texture"], c["start"], c["K"], c["field"], image, c["known"])
        else:
            want = JREF.joint_ref(JOINT_CASE[0], c["texture"], c["start"], c["K"], sdf=c["field"], image=image, photo_mask=c["known"])
    return dict(c, image=image, want=want, err=JREF.pose_errors(c, want["pose"]))
