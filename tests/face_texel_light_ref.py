"""K41 (tp_face_texel_light) and FaceTexelFitter(lighting=True) restated in numpy: the rule of include/texpose_amd.h with fp32 operations in
the stated order (bit equality is asked of the device), and the alternation of DESIGN section 31 as face_texel_fit_ref.fit_loop's sibling."""
import os

import numpy as np

import face_texel_fit_ref as FIT
import photo_lighting_ref as LREF

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "face_texel_light_fit.npz")


# ----------------------------------------------------------------------------------------------------------------- one call
def shading_ref(verts, faces, face, pose, light):
    """One image: face [H,W] (anything), pose [3,4], light [3,5] -> s [H,W,3] float32: K40's apply shading, fp64 from the fp32 light and the
    valid normal, rounded once; l0 itself where the pixel has no valid normal."""
    l32 = np.asarray(light, np.float32).reshape(3, 5)
    nrm, valid = LREF.pixel_normals_ref(verts, faces, face, pose)
    with np.errstate(all="ignore"):
        l = l32.astype(np.float64)
        s = ((l[:, 0] + l[:, 1] * nrm[..., 0:1]) + l[:, 2] * nrm[..., 1:2]) + l[:, 3] * nrm[..., 2:3]
        return np.where(valid[..., None], s.astype(np.float32), l32[:, 0]).astype(np.float32)


def light_ref(verts, faces, face, pose, light, colour, image=None, weight=None):
    """The whole call: face [B,H,W], pose [B,3,4], light [B,3,5], colour [B,H,W,3], image [B,H,W,3] or None, weight [B,H,W] or None ->
    dict(grad, diag [B,H,W,3] float32, on [B,H,W] bool and, in residual mode, sums [B,2] float64)."""
    face = np.asarray(face)
    B, H, W = face.shape
    F = len(np.asarray(faces).reshape(-1, 3))
    c32 = np.asarray(colour, np.float32)
    o32 = None if image is None else np.asarray(image, np.float32)
    m32 = np.ones((B, H, W), np.float32) if weight is None else np.asarray(weight, np.float32)
    l32 = np.asarray(light, np.float32).reshape(B, 3, 5)
    grad, diag = np.zeros((B, H, W, 3), np.float32), np.zeros((B, H, W, 3), np.float32)
    on_all, sums = np.zeros((B, H, W), bool), np.zeros((B, 2))
    with np.errstate(all="ignore"):
        for b in range(B):
            f = face[b].astype(np.int64)
            on = (f >= 0) & (f < F) & np.isfinite(m32[b]) & (m32[b] > 0) & np.isfinite(c32[b]).all(-1)
            if o32 is not None:
                on &= np.isfinite(o32[b]).all(-1)
            s = shading_ref(verts, faces, face[b], pose[b], l32[b])
            a = m32[b][..., None] * s                                    # fp32 from here on, one rounding per operation
            q = s * c32[b]
            if o32 is not None:
                p = q + l32[b, :, 4]
                e = o32[b] - p
                g = a * e
                e64 = e.astype(np.float64)
                t = m32[b].astype(np.float64) * ((e64[..., 0] * e64[..., 0] + e64[..., 1] * e64[..., 1]) + e64[..., 2] * e64[..., 2])
                sums[b] = t[on].sum(), m32[b].astype(np.float64)[on].sum()
            else:
                g = a * q
            d = a * s
            grad[b], diag[b], on_all[b] = np.where(on[..., None], g, 0.0), np.where(on[..., None], d, 0.0), on
    out = dict(grad=grad.astype(np.float32), diag=diag.astype(np.float32), on=on_all)
    if o32 is not None:
        out["sums"] = sums
    return out


# ----------------------------------------------------------------------------------------------------------------- the loop
def lit_fit_loop(views, planes, prior, start, lam, iters, rounds, tau=0.5, tau0=2.0, gain_range=(0.25, 4.0), lights=None, light_step=True,
                 dtype=np.float64):
    """FaceTexelFitter(lighting=True).fit: ``rounds`` alternations of a light step (photo_lighting_ref.fit_ref per view on the unlit render
    S x against the view's photograph, mask = weight > 0, the depth plane 1 on covered pixels, tau0 in round 0 and tau afterwards, the
    light of the round before as light_in) and ``iters`` steps of conjugate gradients on (S^T m s^2 S + lam) x = S^T m s (I - beta) + lam
    prior, restarted from the current x, preconditioned per node and channel with S^T (m s^2) + lam.  ``views``: face_texel_fit_ref.Views
    of all stored views; ``planes``: dict(verts, faces, face [B,H,W], pose [B,3,4], rgb [B,H,W,3], weight [B,H,W]) of the same views;
    ``lights`` [B,3,5]: the lights to start from (None: the identity); ``light_step=False`` keeps them
    -> dict(nodes, coverage, light [B,3,5] float32, status [B], flags [B], gain [3], rms [rounds * iters + 1])."""
    x, prior = np.array(start, dtype=dtype), np.asarray(prior, dtype=dtype)
    verts, faces, face, pose = planes["verts"], planes["faces"], np.asarray(planes["face"]), np.asarray(planes["pose"], np.float32)
    photo, weight = np.asarray(planes["rgb"], np.float32), np.asarray(planes["weight"], np.float32)
    B, H, W = face.shape
    F = len(faces)
    valid = views.valid.reshape(B, H, W)
    S = lambda v: views.shade(v.astype(np.float64)).astype(dtype)
    St = lambda g: views.adjoint(g.astype(np.float64)).astype(dtype)
    m, total = views.m.astype(dtype)[:, None], float(views.m.sum())
    img = views.rgb.astype(dtype)
    zbuf = np.where((face >= 0) & (face < F), 1.0, -1.0).astype(np.float32)
    light = np.tile(LREF.IDENTITY, (B, 3, 1)) if lights is None else np.array(lights, np.float32).reshape(B, 3, 5)
    status, flags = np.zeros(B, np.int32), np.zeros(B, np.int32)
    first = lights is None
    rms = []
    for rnd in range(rounds):
        if light_step:
            render = np.zeros((B, H, W, 3), np.float32)
            render[valid] = S(x).astype(np.float32)
            for b in range(B):
                fit = LREF.fit_ref(verts, faces, face[b], zbuf[b], render[b], pose[b], photo[b], tau0 if rnd == 0 else tau,
                                   None if (first and rnd == 0) else light[b], weight[b] > 0, gain_range)
                status[b], flags[b] = fit["status"], fit["flags"]
                if rnd == 0 or not fit["flags"] & (7 * LREF.FALLBACK):  # (an ambient-only fallback never replaces a light of a round before)
                    light[b] = fit["light"]
        s = np.stack([shading_ref(verts, faces, face[b], pose[b], light[b]) for b in range(B)])[valid].astype(dtype)
        beta = np.broadcast_to(light[:, None, None, :, 4], (B, H, W, 3))[valid].astype(dtype)
        resid = lambda v: img - (s * S(v) + beta)
        rms_of = lambda v: float(np.sqrt((views.m[:, None] * resid(v).astype(np.float64) ** 2).sum() / (3.0 * total)))
        if rnd == 0:
            rms.append(rms_of(x))
        r = St(m * s * resid(x)) + dtype(lam) * (prior - x)
        m_inv = (1.0 / (St(m * s * s) + dtype(lam))).astype(dtype)
        x = FIT.pcg(x, r, m_inv, lambda p: St(m * s * (s * S(p))) + dtype(lam) * p, lambda v: rms.append(rms_of(v)), iters, dtype)
    return dict(nodes=x, coverage=views.coverage(), light=light, status=status, flags=flags, gain=light[:, :, 0].astype(np.float64).mean(0),
                rms=np.array(rms))


# ----------------------------------------------------------------------------------------------------------------- the relit round trip
AMBIENT = np.array([0.70, 0.75, 0.65])
BIAS = np.array([0.05, 0.10, 0.08])
STRENGTH, STRONG, SIGMA = 0.45, 0.9, 0.02
ROUNDS, ITERS, LAM = 6, 4, 0.1


def view_lights(n, strength=STRENGTH, seed=0):
    """One light per view [n,3,5] float32 from RandomState(seed), drawn view by view: ambient AMBIENT * U(0.8, 1.25); the direction a
    randn(3) vector with z := -|z| - 0.3, normalised (camera frame: towards the camera's side); the directional part ``strength`` of the
    ambient; bias BIAS * U(0, 1)."""
    rs = np.random.RandomState(seed)
    out = np.zeros((n, 3, 5))
    for b in range(n):
        amb = AMBIENT * rs.uniform(0.8, 1.25)
        d = rs.randn(3)
        d[2] = -abs(d[2]) - 0.3
        d /= np.linalg.norm(d)
        out[b] = np.concatenate([amb[:, None], strength * amb[:, None] * d[None, :], (BIAS * rs.uniform(0.0, 1.0))[:, None]], 1)
    return out.astype(np.float32)


def relight(verts, faces, face, pose, rgb, lights, sigma=0.0, seed=1):
    """Photographs rgb [B,H,W,3] relit view by view: a covered pixel becomes s(n) rgb + beta by photo_lighting_ref.apply_ref, the rest
    stays; then noise of ``sigma`` from RandomState(seed) on every pixel, as a sensor would add it."""
    F = len(faces)
    out = np.stack([LREF.apply_ref(verts, faces, face[b], np.where((face[b] >= 0) & (face[b] < F), 1.0, -1.0).astype(np.float32), rgb[b], pose[b],
                                   lights[b]) for b in range(len(face))])
    if sigma > 0:
        out = out.astype(np.float64) + np.random.RandomState(seed).normal(0.0, sigma, out.shape)
    return out.astype(np.float32)


def affine_psnr(img, want, mask):
    """The PSNR of ``img`` against ``want`` over ``mask`` after the best per-channel affine map of img (closed form): the figure does not
    depend on the gauge of the albedo."""
    a, b = np.asarray(img, np.float64)[mask], np.asarray(want, np.float64)[mask]
    out = np.empty_like(a)
    for k in range(3):
        A = np.stack([a[:, k], np.ones(len(a))], 1)
        coef = np.linalg.lstsq(A, b[:, k], rcond=None)[0]
        out[:, k] = A @ coef
    return 10 * np.log10(1.0 / ((out - b) ** 2).mean())


CASES = {"clean": (STRENGTH, 0.0), "noisy": (STRENGTH, SIGMA), "strong": (STRONG, 0.0)}

# ---- measured by tests/test_face_texel_light_cpu.py with this file's loop (fp64 vectors), pinned there and in golden/face_texel_light_fit.npz
# Section 26's shrunk round trip (sphere uv_sphere(12, 16), 14 Fibonacci views, 64 x 64, f = 200, R = 4, lam = 0.1, held-out view
# sphere_view_poses(5, 400)[1]) with every photograph relit by view_lights; prior and start: the bake of the relit photographs;
# plain: fit_loop, 4 iterations; lit: lit_fit_loop, 6 rounds x 4 iterations, tau0 2.0, tau 0.5.
#   case: (training rms of the plain fit, of the lit fit, held-out gauge-free PSNR of the plain fit, of the lit fit)
RELIT = {"clean": (0.09412, 0.01683, 30.51, 31.91), "noisy": (0.09608, 0.02518, 30.32, 31.54), "strong": (0.16320, 0.02270, 27.35, 31.56)}
# (the bake of the relit photographs starts the plain fit at rms 0.1021 / 0.1040 / 0.1705; the lit series starts at 0.0299 / 0.0357 / 0.0586
#  after the first light step and falls in every round; at 0.9 one channel of one view still takes K40's fallback in the last round)
# The consistent system: section 26's (R = 2, photographs S x* for x* = RandomState(11).rand(U, 3)) relit by view_lights(14) through this
# file's own apply, the true lights given, the light step skipped, lam 1e-6, prior 0.5, from zeros, one round of 32 iterations: max |x -
# x*| over the nodes with coverage >= 1 with fp64 and with fp32 vectors.  The device bar is 4 x the first + 1e-4.
CONSISTENT_ERROR = 2.10e-6                      # 767 of 768 nodes have coverage >= 1; training rms 0.468 -> 3.0e-8
CONSISTENT_ERROR_FP32 = 2.23e-6                 # below 4 x 2.10e-6 + 1e-4, the device test's bar
