"""The image-pyramid contract of DESIGN section 28 (kernels K38: tp_image_down, tp_surface_down, tp_mask_down), said again in numpy --
written from the rules in include/texpose_amd.h, not from the kernels.  The filter's arithmetic has ONE stated order (fp64 from the fp32
inputs, per tap row the four columns ascending, then the four rows ascending, one rounding to fp32), and every weight is dyadic, so
this file's whole-plane gathers give the kernels' results bit for bit; the tests compare bits, NaN positions apart.  The loop is
tests/photo_ref.py's on its brute-force raster: every pass renders at full size, filters the rendering down to the pass's level and
hands step_ref the level's planes, photograph and intrinsics.

FIGURES, measured on this file's loops (CPU, numpy, photo_ref's raster; tests/test_photo_pyramid_cpu.py asserts the pinned cases
against TABLE; `python tests/photo_pyramid_ref.py` prints all of them).  128 x 160 (pnp_ref.end_to_end_inputs with K's first two rows,
H and W doubled), colours 0.5 + 0.5 sin(v / f + (0, 1, 2)) over a 0.5 background, start 3 deg and 6.08 / 8.06 mm away, tau 0.5,
damping 1e-6, ten steps on every route; errors in deg / mm, image 0 then image 1.
    case                      plain, 10 steps                      pyramid (4, 3, 3)
    sphere f = 3 clean        0.0206 / 0.0310   2.4682 / 8.0151    0.0213 / 0.0299   0.0092 / 0.0371
    sphere f = 2 clean        0.0141 / 0.0310   6.8899 / 17.5481   0.0147 / 0.0297   0.0021 / 0.0018
    torus  f = 3 clean        0.0001 / 0.0002   0.2701 / 1.1017    0.0031 / 0.0132   0.0001 / 0.0005
    sphere f = 3 sigma 0.02   0.0370 / 0.0423   2.4783 / 7.6510    0.0339 / 0.0473   0.0248 / 0.0342
    sphere f = 2 sigma 0.02   0.0252 / 0.0130   6.5553 / 17.2332   0.0254 / 0.0129   0.0139 / 0.0184
    torus  f = 3 sigma 0.02   0.0157 / 0.1313   0.3955 / 1.4414    0.0148 / 0.1154   0.0074 / 0.1179
The plain loop loses image 1 of all four sphere cases (it ends no closer in translation than 0.94 of its start); the pyramid ends every
image of every case below 0.04 deg and 0.12 mm.  The translations are the feature request's prototype's to its rounding; its rotations
differ from these by up to 0.02 deg.
PINNED (run by the CPU suite, one loop takes 10 - 15 s): the three noisy cases and the clean sphere f = 2, pyramid and plain route.
Under section 27's gain and bias (photo_exposure_ref.changed, the noise added after) the sphere f = 2 sigma 0.02 case ends with the
exposure fit and the pyramid at 0.0247 / 0.0291 and 0.0182 / 0.0314, gains within 1e-3 of (0.75, 0.80, 0.70): the premise of the GPU
suite's exposure test holds.

WHERE IT STOPS, measured, no bar (sphere f = 3 clean):
    from 6 deg and 12.2 / 16.1 mm: plain 0.0208 / 0.0314 and 1.4660 / 19.1417, pyramid 0.0213 / 0.0291 and 11.4136 / 30.1792 -- image
    1 is lost by both routes; the pyramid widens the basin, it does not remove it;
    at 64 x 80 (photo_ref's own size) level 2 keeps 21 / 22 pixels at the start and 21 / 24 at the true pose (rms exactly 0), and the
    (4, 3, 3) loop DIVERGES (0.13 / 0.93 and 43.9 / 415.3) where the plain loop ends at 0.0494 / 0.1323 and 0.0958 / 0.0882: a level
    needs enough pixels."""
import functools
import os
import sys

import numpy as np

import photo_ref as PR
import pnp_ref as PREF
from gn_ref import loop_ref

WEIGHTS = np.array([1.0, 3.0, 3.0, 1.0]) / 8.0
BACKGROUND_Z = -1.0

# (mesh, f, noisy) -> ((plain deg, mm) image 0, image 1, (pyramid deg, mm) image 0, image 1)
TABLE = {("sphere", 3.0, False): ((0.0206, 0.0310), (2.4682, 8.0151), (0.0213, 0.0299), (0.0092, 0.0371)),
         ("sphere", 2.0, False): ((0.0141, 0.0310), (6.8899, 17.5481), (0.0147, 0.0297), (0.0021, 0.0018)),
         ("torus", 3.0, False): ((0.0001, 0.0002), (0.2701, 1.1017), (0.0031, 0.0132), (0.0001, 0.0005)),
         ("sphere", 3.0, True): ((0.0370, 0.0423), (2.4783, 7.6510), (0.0339, 0.0473), (0.0248, 0.0342)),
         ("sphere", 2.0, True): ((0.0252, 0.0130), (6.5553, 17.2332), (0.0254, 0.0129), (0.0139, 0.0184)),
         ("torus", 3.0, True): ((0.0157, 0.1313), (0.3955, 1.4414), (0.0148, 0.1154), (0.0074, 0.1179))}
PINNED = (("sphere", 3.0, True), ("sphere", 2.0, True), ("torus", 3.0, True), ("sphere", 2.0, False))
PYRAMID = (4, 3, 3)


# ----------------------------------------------------------------------------------------------------------------- one level down
def taps(n):
    """[n // 2, 4]: the fine rows (or columns) clamp(2 I - 1 .. 2 I + 2, 0, n - 1) of every coarse row I."""
    return np.clip(2 * np.arange(n // 2)[:, None] - 1 + np.arange(4)[None, :], 0, n - 1)


def _gather(x):
    """x [N,H,W,C] -> [N,h,4 rows,w,4 columns,C]"""
    return x[:, taps(x.shape[1])][:, :, :, taps(x.shape[2])]


def filter_ref(x):
    """x [N,H,W,C] float32 -> [N,H//2,W//2,C] float32: the (1, 3, 3, 1) / 8 filter in both directions in the stated order."""
    x = np.asarray(x, np.float32)
    assert x.ndim == 4 and x.shape[1] >= 2 and x.shape[2] >= 2
    w = WEIGHTS
    with np.errstate(all="ignore"):
        t = _gather(x.astype(np.float64))
        s = ((w[0] * t[:, :, :, :, 0] + w[1] * t[:, :, :, :, 1]) + w[2] * t[:, :, :, :, 2]) + w[3] * t[:, :, :, :, 3]      # [N,h,4,w,C]
        return (((w[0] * s[:, :, 0] + w[1] * s[:, :, 1]) + w[2] * s[:, :, 2]) + w[3] * s[:, :, 3]).astype(np.float32)


def image_down_ref(image):
    """[N,H,W,3] -> [N,h,w,3]; non-finite taps propagate as IEEE arithmetic gives."""
    return filter_ref(image)


def surface_down_ref(zbuf, rgb):
    """zbuf [B,H,W], rgb [B,H,W,3] -> ([B,h,w], [B,h,w,3]): a coarse pixel is a surface iff all 16 taps have z > 0 and finite; there z
    and rgb are filtered, elsewhere z = -1 and rgb = 0."""
    z32, c32 = np.asarray(zbuf, np.float32), np.asarray(rgb, np.float32)
    with np.errstate(all="ignore"):
        surface = _gather(((z32 > 0) & np.isfinite(z32))[..., None]).all((2, 4))[..., 0]
    z = np.where(surface, filter_ref(z32[..., None])[..., 0], np.float32(BACKGROUND_Z))
    return z.astype(np.float32), np.where(surface[..., None], filter_ref(c32), np.float32(0.0)).astype(np.float32)


def mask_down_ref(mask):
    """[N,H,W] uint8 -> [N,h,w] uint8: 1 iff all 16 taps are non-zero, else 0."""
    return _gather((np.asarray(mask) != 0)[..., None]).all((2, 4))[..., 0].astype(np.uint8)


def same(a, b):
    """Bit-equal float32 arrays, NaN positions equal (a NaN's payload is not part of the contract)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def image_pyramid_ref(image, levels):
    out = [np.asarray(image, np.float32)]
    for _ in range(levels - 1):
        out.append(image_down_ref(out[-1]))
    return out


def mask_pyramid_ref(mask, levels):
    out = [np.asarray(mask, np.uint8)]
    for _ in range(levels - 1):
        out.append(mask_down_ref(out[-1]))
    return out


def level_K(K, level):
    """Level l's intrinsics: rows 0 and 1 times 2^-l (exact in fp32)."""
    K = np.asarray(K, np.float32).copy()
    K[..., :2, :] *= np.float32(0.5 ** level)
    return K


def pass_levels(pyramid):
    """(4, 3, 3) -> [2, 2, 2, 2, 1, 1, 1, 0, 0, 0, 0]: the level of every pass, the final evaluation's 0 included."""
    return [len(pyramid) - 1 - k for k, n in enumerate(pyramid) for _ in range(int(n))] + [0]


# ----------------------------------------------------------------------------------------------------------------- one call, exact inputs
def one_down_case(seed, N, H, W):
    """Hand-built planes for one level down (no rasteriser): zbuf 880 .. 920 mm on 60 % of the pixels, in blocks of 6 x 6 so that
    coarse pixels with all 16 taps on the surface exist, rgb and image uniform in [0, 1], 2 % of the values of zbuf, rgb and image NaN
    or +-Inf plus one of each planted by hand, and a mask with 15 % of its 6 x 6 blocks and 2 % of its pixels zero."""
    rs = np.random.RandomState(seed)
    blocks = lambda p: np.repeat(np.repeat(rs.uniform(size=(N, -(-H // 6), -(-W // 6))) < p, 6, 1), 6, 2)[:, :H, :W]
    zbuf = rs.uniform(880.0, 920.0, (N, H, W)).astype(np.float32)
    zbuf[blocks(0.4)] = -1.0
    rgb = rs.uniform(0.0, 1.0, (N, H, W, 3)).astype(np.float32)
    image = rs.uniform(0.0, 1.0, (N, H, W, 3)).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    for plane in (zbuf, rgb, image):
        flat = plane.reshape(-1)
        hit = rs.uniform(size=flat.shape) < 0.02
        flat[hit] = bad[rs.randint(0, 3, int(hit.sum()))]
        for value in bad:
            flat[rs.randint(len(flat))] = value
    mask = (~blocks(0.15) & (rs.uniform(size=(N, H, W)) >= 0.02)).astype(np.uint8) * rs.randint(1, 256, (N, H, W)).astype(np.uint8)
    return dict(zbuf=zbuf, rgb=rgb, image=image, mask=mask)


# ----------------------------------------------------------------------------------------------------------------- the loop
def photo_pyramid_ref(verts, faces, vcolor, pose, K, image, pyramid, tau=0.5, damping=1e-6, frame=None, mask=None, exposure=False, tau0=2.0):
    """ops.photo_align(pyramid=...) on photo_ref's own raster: iters = sum(pyramid) steps and the final evaluation at level 0; every pass
    renders at full size, applies surface_down_ref level times and steps on the level's planes -> loop_ref's dict (inliers0 / rms0 are
    the first pass's, at its level); ``exposure``: the fit of photo_exposure_ref on the level's planes in front of each step."""
    image = np.asarray(image, np.float32)
    H, W = image.shape[1:3]
    levels = pass_levels(pyramid)
    images = image_pyramid_ref(image, len(pyramid))
    masks = [None] * len(pyramid) if mask is None else mask_pyramid_ref(mask, len(pyramid))
    render = lambda P: [PR.render_ref(verts, faces, vcolor, P[b], K[b], H, W) for b in range(len(P))]
    at, fit = [0], {}

    def step(planes, P, t, last):
        level = levels[at[0]]
        at[0] += 1
        zbuf, rgb = np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes])
        for _ in range(level):
            zbuf, rgb = surface_down_ref(zbuf, rgb)
        if exposure:
            import photo_exposure_ref as XR
            e = XR.exposure_ref(zbuf, rgb, images[level], t if fit else tau0, fit.get("gain"), fit.get("bias"), frame, masks[level])
            fit.update(gain=e["gain"], bias=e["bias"], exposure_status=e["status"])
            rgb = e["rgb"]
        return PR.step_ref(zbuf, rgb, P, level_K(K, level), images[level], t, damping, frame, masks[level], evaluate_only=last)

    return dict(loop_ref(render, step, pose, tau, len(levels) - 1), **fit)


# ----------------------------------------------------------------------------------------------------------------- the loop's cases
def vertex_colours(verts, f):
    return (0.5 + 0.5 * np.sin(np.asarray(verts, np.float64) / f + np.array([0.0, 1.0, 2.0]))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def loop_inputs(mesh, f, noisy, scale=2, start_deg=3.0, exposed=False):
    """pnp_ref.end_to_end_inputs(mesh) with K's first two rows, H and W times ``scale`` and the colours of wavelength f: the photograph
    is the brute-force render of the true poses over 0.5 (sigma 0.02 Gaussian noise on every value where ``noisy``), the start
    ``start_deg`` degrees and 6 .. 8 mm away (at 6 degrees twice that, as the request's limit was measured); ``exposed``: the clean
    photograph under photo_exposure_ref's gain and bias, the noise added after."""
    e = PREF.end_to_end_inputs(mesh)
    H, W = e["H"] * scale, e["W"] * scale
    K1 = e["K"].copy()
    K1[:2] *= scale
    K = np.tile(K1, (2, 1, 1))
    vcolor = vertex_colours(e["verts"], f)
    image = np.stack([PR.render_ref(e["verts"], e["faces"], vcolor, e["P"][b], K[b], H, W, PR.BACKGROUND)[1] for b in range(2)])
    noise = np.random.RandomState(4).normal(0.0, PR.NOISE_SIGMA, image.shape) if noisy else 0.0
    if exposed:
        import photo_exposure_ref as XR
        image = XR.changed(image)
    image = (image + noise).astype(np.float32)
    start = PR.perturbed(e["P"], np.random.RandomState(5), start_deg)
    if start_deg > 3.0:
        start[:, :, 3] = e["P"][:, :, 3] + 2.0 * (start[:, :, 3] - e["P"][:, :, 3])
    return dict(e, H=H, W=W, K=K, vcolor=vcolor, image=image, start=start)


@functools.lru_cache(maxsize=None)
def loop_case(mesh, f, noisy, pyramid=PYRAMID, scale=2, start_deg=3.0, exposure=False):
    """One loop (ten steps, tau 0.5, damping 1e-6), run once per case and shared by the test files: ``pyramid`` None is photo_ref's
    plain loop."""
    c = loop_inputs(mesh, f, noisy, scale, start_deg, exposure)
    if pyramid is None:
        want = PR.photo_ref(c["verts"], c["faces"], c["vcolor"], c["start"], c["K"], c["image"], 0.5, 10, 1e-6)
    else:
        want = photo_pyramid_ref(c["verts"], c["faces"], c["vcolor"], c["start"], c["K"], c["image"], pyramid, 0.5, 1e-6, exposure=exposure)
    return dict(c, want=want)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photo_pyramid_loops.npz")
GOLDEN_KEYS = ("pose", "inliers", "inliers0", "rms", "status", "near_ties")
EXPOSED = ("sphere", 2.0, True)                                  # the case of the GPU suite's exposure test


def golden_name(mesh, f, noisy, exposure=False):
    return "%s_f%g_%s%s" % (mesh, f, "noisy" if noisy else "clean", "_exposed" if exposure else "")


def golden_want(mesh, f, noisy, exposure=False):
    """The pyramid loop's result on a pinned case as stored in tests/golden/ (a loop takes 10 - 15 s here, and the GPU suite needs only
    its figures): GOLDEN_KEYS of loop_case(...)['want'].  tests/test_photo_pyramid_cpu.py recomputes every pinned case and compares;
    `python tests/photo_pyramid_ref.py --golden` writes the file."""
    with np.load(GOLDEN) as z:
        return {k: z[golden_name(mesh, f, noisy, exposure) + "/" + k] for k in GOLDEN_KEYS}


def write_golden():
    out = {}
    for key, exposure in [(k, False) for k in PINNED] + [(EXPOSED, True)]:
        want = loop_case(*key, exposure=exposure)["want"]
        out.update({golden_name(*key, exposure) + "/" + k: np.asarray(want[k]) for k in GOLDEN_KEYS})
    np.savez(GOLDEN, **out)


def errors(c, pose):
    """[(deg, mm)] per image of ``pose`` against the case's truth."""
    return [PREF.pose_error(np.asarray(pose)[b], c["P"][b]) for b in range(len(c["P"]))]


def kept_at_level(c, pose, level):
    """The kept pixels per image of an evaluation of ``pose`` at ``level``, and its rms."""
    zbuf, rgb = (np.stack(p) for p in zip(*[PR.render_ref(c["verts"], c["faces"], c["vcolor"], pose[b], c["K"][b], c["H"], c["W"]) for b in range(len(pose))]))
    for _ in range(level):
        zbuf, rgb = surface_down_ref(zbuf, rgb)
    r = PR.step_ref(zbuf, rgb, pose, level_K(c["K"], level), image_pyramid_ref(c["image"], level + 1)[level], 0.5, evaluate_only=True)
    return r["inliers"], r["rms"]


# ----------------------------------------------------------------------------------------------------------------- the tool's scene
# The premise of the tool test's bar, measured once on this file's loops (tool_premise() below; CPU, 40 s): the 8-bit photographs of
# tool_scene(), ten steps, tau 0.5.  ADD of the mesh's vertices, start -> end, frames 0, 1, 2:
TOOL_PREMISE = ("6.435 / 8.286 / 8.286 mm -> plain loop 0.032 / 17.992 / 16.967 mm (frames 1 and 2 are lost), pyramid (4, 3, 3) 0.031 / 0.0017 / "
                "0.027 mm (ratios 0.0002 .. 0.005): 8-bit quantisation leaves the pyramid far below a quarter, so the quarter stands")


@functools.lru_cache(maxsize=None)
def tool_scene():
    """The f = 2 sphere with its colours at 8 bits at 128 x 160, the size at which the plain loop loses image 1: loop_inputs' two
    poses and starts, and as a third frame image 1 turned by 25 degrees about the optical axis -> verts, faces, colour8 [V,3] uint8,
    K [3,3], gt [3,3,4], start [3,3,4], H, W."""
    c = loop_inputs("sphere", 2.0, False)
    a = np.radians(25.0)
    Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    turn = lambda P: np.concatenate([P.astype(np.float64), (Rz @ P[1].astype(np.float64))[None]]).astype(np.float32)
    return dict(verts=c["verts"], faces=c["faces"], colour8=np.rint(c["vcolor"] * 255.0).astype(np.uint8), K=c["K"][0], gt=turn(c["P"]),
                start=turn(c["start"]), H=c["H"], W=c["W"])


def tool_premise():
    s = tool_scene()
    vcolor, K = s["colour8"].astype(np.float32) / 255.0, np.tile(s["K"], (3, 1, 1))
    shot = np.stack([PR.render_ref(s["verts"], s["faces"], vcolor, s["gt"][b], K[b], s["H"], s["W"], 128.0 / 255.0)[1] for b in range(3)])
    image = (np.rint(np.clip(shot, 0.0, 1.0) * 255.0) / 255.0).astype(np.float32)
    add = lambda P: [float(np.linalg.norm((s["verts"] @ P[b][:, :3].T + P[b][:, 3]) - (s["verts"] @ s["gt"][b][:, :3].T + s["gt"][b][:, 3]), axis=1).mean())
                     for b in range(3)]
    plain = PR.photo_ref(s["verts"], s["faces"], vcolor, s["start"], K, image, 0.5, 10, 1e-6)
    pyr = photo_pyramid_ref(s["verts"], s["faces"], vcolor, s["start"], K, image, PYRAMID)
    return dict(start=add(s["start"].astype(np.float64)), plain=add(plain["pose"].astype(np.float64)), pyramid=add(pyr["pose"].astype(np.float64)))


if __name__ == "__main__":
    if sys.argv[1:] == ["--golden"]:
        sys.exit(write_golden())
    print("tool premise, ADD mm:", tool_premise(), flush=True)

    fmt = lambda e: "   ".join("%.4f / %.4f" % p for p in e)
    for key in TABLE:
        plain, pyr = loop_case(*key, pyramid=None), loop_case(*key)
        print(key, "plain", fmt(errors(plain, plain["want"]["pose"])), "| pyramid", fmt(errors(pyr, pyr["want"]["pose"])), flush=True)
    x = loop_case("sphere", 2.0, True, exposure=True)
    print("exposure + pyramid, sphere f = 2 noisy:", fmt(errors(x, x["want"]["pose"])), x["want"]["gain"], flush=True)
    for kw in (dict(start_deg=6.0), dict(scale=1)):
        plain, pyr = loop_case("sphere", 3.0, False, pyramid=None, **kw), loop_case("sphere", 3.0, False, **kw)
        print(kw, "start", fmt(errors(pyr, pyr["start"])), "plain", fmt(errors(plain, plain["want"]["pose"])), "| pyramid",
              fmt(errors(pyr, pyr["want"]["pose"])), "kept at level 2: start", kept_at_level(pyr, pyr["start"], 2)[0], "truth",
              kept_at_level(pyr, pyr["P"], 2), flush=True)
