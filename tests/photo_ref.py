"""The photometric-alignment contract of DESIGN section 20 (kernel K30: tp_photo_align_step), said again in numpy fp64 -- written from
the rules in include/texpose_amd.h, not from the kernels.  Where the kernel is free to choose, this file chooses differently: the
gradients are whole-plane slices, the sums are matrix products over the kept pixels of an image at once (the kernel adds per thread,
wave, workgroup and tile), the systems are solved with np.linalg.solve on the Cholesky factors, and the loop renders with the
brute-force rasteriser of tests/mesh_raster_ref.py.  The per-image part (status, step, Gram-Schmidt, fp32 rounding) is K29's word for
word: both use gn_ref.solve_ref.

Besides the results it reports what decides whether a comparison of counts can be exact: near-ties, kept-or-dropped decisions whose
margin | |o - c| - tau | is below NEAR_TIE colour units."""
import functools

import numpy as np

import mesh_raster_ref as RR
import pnp_ref as PREF
from gn_ref import MIN_COUNT, loop_ref, solve_ref  # noqa: F401  (the per-image part is K29's word for word)
from icp_ref import frame_index, perturbed  # noqa: F401  (the loop's start poses)

NEAR_TIE = 1e-9          # colour units
BACKGROUND = 0.5


def sums_ref(zbuf, rgb, K, image, tau, mask=None):
    """One image: zbuf / mask [H,W], rgb / image [H,W,3], K [3,3] (fp32 values) -> dict(JtJ [6,6], Jtr [6], cost, count, near_ties,
    kept [H,W] bool)."""
    z32, c32, o32 = np.asarray(zbuf, np.float32), np.asarray(rgb, np.float32), np.asarray(image, np.float32)
    H, W = z32.shape
    K = np.asarray(K, np.float32).astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    tau = float(np.float32(tau))
    kept = np.zeros((H, W), bool)
    empty = dict(JtJ=np.zeros((6, 6)), Jtr=np.zeros(6), cost=0.0, count=0, near_ties=0, kept=kept)
    if H < 3 or W < 3:
        return empty
    with np.errstate(all="ignore"):
        o = o32.astype(np.float64)
        zi = z32[1:-1, 1:-1]
        cand = (zi > 0) & np.isfinite(zi)
        if mask is not None:
            cand &= np.asarray(mask)[1:-1, 1:-1] != 0
        c, oc = c32[1:-1, 1:-1].astype(np.float64), o[1:-1, 1:-1]
        lf, rt, up, dn = o[1:-1, :-2], o[1:-1, 2:], o[:-2, 1:-1], o[2:, 1:-1]
        cand &= np.isfinite(np.concatenate([c, oc, lf, rt, up, dn], -1)).all(-1)
        res = oc - c
        d2 = (res[..., 0] ** 2 + res[..., 1] ** 2) + res[..., 2] ** 2
        ties = int((cand & (np.abs(np.sqrt(d2) - tau) < NEAR_TIE)).sum())
        keep = cand & (d2 <= tau * tau)
    ii, ji = np.nonzero(keep)                                    # (indices into the interior block)
    if len(ii) == 0:
        return dict(empty, near_ties=ties)
    kept[ii + 1, ji + 1] = True
    z = zi[ii, ji].astype(np.float64)
    rx, ry = (((ji + 1) + 0.5) - cx) / fx, (((ii + 1) + 0.5) - cy) / fy
    P = np.stack([z * rx, z * ry, z], 1)                         # [n,3]
    gx, gy = 0.5 * (rt[ii, ji] - lf[ii, ji]), 0.5 * (dn[ii, ji] - up[ii, ji])          # [n,3 channels]
    gfx, gfy = gx * fx, gy * fy
    a = np.stack([gfx / z[:, None], gfy / z[:, None], -(gfx * rx[:, None] + gfy * ry[:, None]) / z[:, None]], -1)      # [n,3 channels,3]
    J = np.concatenate([np.cross(P[:, None, :], a), a], -1).reshape(-1, 6)
    r = res[ii, ji].reshape(-1)
    return dict(JtJ=J.T @ J, Jtr=J.T @ r, cost=float(r @ r), count=len(ii), near_ties=ties, kept=kept)


def step_ref(zbuf, rgb, pose, K, image, tau, damping=1e-6, frame=None, mask=None, evaluate_only=False):
    """The whole call: zbuf [B,H,W], rgb [B,H,W,3], pose [B,3,4], K [B,3,3], image [Ft,H,W,3] (and mask [Ft,H,W]) -> dict(pose
    [B,3,4] float32, inliers [B], rms [B] fp64, status [B], near_ties [B], kept [B,H,W])."""
    B = len(pose)
    image = np.asarray(image, np.float32)
    fr = frame_index(B, len(image), frame)
    out = dict(pose=np.zeros((B, 3, 4), np.float32), inliers=np.zeros(B, np.int64), rms=np.zeros(B), status=np.zeros(B, np.int64),
               near_ties=np.zeros(B, np.int64), kept=np.zeros(np.asarray(zbuf).shape, bool))
    for b in range(B):
        s = sums_ref(zbuf[b], rgb[b], K[b], image[fr[b]], tau, None if mask is None else np.asarray(mask)[fr[b]])
        out["pose"][b], out["inliers"][b], out["rms"][b], out["status"][b] = solve_ref(s, pose[b], damping, evaluate_only)
        out["near_ties"][b], out["kept"][b] = s["near_ties"], s["kept"]
    return out


def render_ref(verts, faces, vcolor, pose, K, H, W, background=None):
    """zbuf [H,W] float32 (-1 background) and rgb [H,W,3] float32 of one pose by the brute-force rasteriser, asked only for the pixels
    of the projected vertices' bounding box (no other pixel can be covered); ``background``: the colour of the pixels without a
    surface (None: the rasteriser's 0)."""
    pose, K = np.asarray(pose, np.float64), np.asarray(K, np.float64)
    cam = np.asarray(verts, np.float64) @ pose[:, :3].T + pose[:, 3]
    assert (cam[:, 2] > 1.0).all()                               # (in front of the camera: the box below holds every covered pixel)
    u, v = K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2], K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]
    j0, j1 = max(0, int(np.floor(u.min())) - 1), min(W, int(np.ceil(u.max())) + 2)
    i0, i1 = max(0, int(np.floor(v.min())) - 1), min(H, int(np.ceil(v.max())) + 2)
    pixels = (np.arange(i0, i1)[:, None] * W + np.arange(j0, j1)[None, :]).reshape(-1)
    zbuf, rgb = np.full(H * W, -1.0), np.full((H * W, 3), 0.0 if background is None else float(background))
    if len(pixels):
        r = RR.rasterize(verts, faces, pose, K, H, W, pixels=pixels, vcolor=vcolor)
        hit = r["face"] >= 0
        zbuf[pixels[hit]], rgb[pixels[hit]] = r["zbuf"][hit], r["rgb"][hit]
    return zbuf.reshape(H, W).astype(np.float32), rgb.reshape(H, W, 3).astype(np.float32)


def photo_ref(verts, faces, vcolor, pose, K, image, tau=0.5, iters=10, damping=1e-6, frame=None, mask=None):
    """The loop of ops.photo_align with its own raster: iters + 1 passes, the pose rounded to fp32 between them, the last
    evaluate-only -> dict(pose [B,3,4] float32, inliers, rms, status (of the last step taken), inliers0, rms0, near_ties (largest over
    the passes))."""
    image = np.asarray(image, np.float32)
    H, W = image.shape[1:3]
    render = lambda P: [render_ref(verts, faces, vcolor, P[b], K[b], H, W) for b in range(len(P))]
    step = lambda planes, P, t, last: step_ref(np.stack([p[0] for p in planes]), np.stack([p[1] for p in planes]), P, K, image, t, damping, frame,
                                               mask, evaluate_only=last)
    return loop_ref(render, step, pose, tau, iters)


# ----------------------------------------------------------------------------------------------------------------- the loop's cases
def vertex_colours(verts):
    """The smooth texture of the loop's cases: 0.5 + 0.5 sin(v / 8 + (0, 1, 2)) per vertex, in [0, 1]."""
    return (0.5 + 0.5 * np.sin(np.asarray(verts, np.float64) / 8.0 + np.array([0.0, 1.0, 2.0]))).astype(np.float32)


NOISE_SIGMA = 0.02


@functools.lru_cache(maxsize=None)
def loop_inputs(mesh, noisy):
    """pnp_ref.end_to_end_inputs(mesh) with the colours above: the photograph is the brute-force render of the true poses over a 0.5
    background (with Gaussian noise of sigma 0.02 on every value where ``noisy``), the start 3 degrees and 6 .. 8 mm away."""
    e = PREF.end_to_end_inputs(mesh)
    K = np.tile(e["K"], (2, 1, 1))
    vcolor = vertex_colours(e["verts"])
    image = np.stack([render_ref(e["verts"], e["faces"], vcolor, e["P"][b], K[b], e["H"], e["W"], BACKGROUND)[1] for b in range(2)])
    if noisy:
        image = (image + np.random.RandomState(4).normal(0.0, NOISE_SIGMA, image.shape)).astype(np.float32)
    start = perturbed(e["P"], np.random.RandomState(5), 3.0)
    return dict(e, K=K, vcolor=vcolor, image=image, start=start)


@functools.lru_cache(maxsize=None)
def loop_case(mesh, noisy):
    """The restatement's loop (10 steps, tau 0.5, damping 1e-6) on loop_inputs, run once per case and shared by the test files."""
    c = loop_inputs(mesh, noisy)
    want = photo_ref(c["verts"], c["faces"], c["vcolor"], c["start"], c["K"], c["image"], 0.5, 10, 1e-6)
    return dict(c, want=want)


# ----------------------------------------------------------------------------------------------------------------- one step, exact inputs
def one_step_case(seed, B, H, W, frames="one", with_mask=False):
    """Hand-built planes for one step (no rasteriser): per image a pose about 900 mm away, zbuf 880 .. 920 mm on 60 % of the pixels,
    rgb uniform in [0, 1], image = rgb + U(-0.4, 0.4) (tau = 0.5 keeps about two thirds), and the bad values the contract names: 2 %
    of the values of zbuf, rgb and image (hence of the neighbours of kept pixels) are NaN or +-Inf, plus one of each planted by hand.
    ``frames``: 'one' (Ft = 1), 'each' (Ft = B) or 'map' (Ft = 2 and a frame map with entries out of range, which clamp)."""
    rs = np.random.RandomState(seed)
    f = min(H, W) * 9.0 + 300.0
    K = np.tile(np.array([[f, 0.0, W / 2.0 + 0.25], [0.0, f * 1.01, H / 2.0 - 0.25], [0.0, 0.0, 1.0]], np.float32), (B, 1, 1))
    pose = np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        pose[b] = np.concatenate([q, rs.uniform(-15, 15, (3, 1)) + [[0.0], [0.0], [900.0]]], 1)
    Ft = dict(one=1, each=B, map=2)[frames]
    frame = np.array([7, -3, 1, 0, 2 ** 30, -2 ** 31][:B] if B <= 6 else np.arange(B) % 2, np.int32) if frames == "map" else None
    fr = frame_index(B, Ft, frame)
    n = H * W
    zbuf = rs.uniform(880.0, 920.0, (B, H, W)).astype(np.float32)
    zbuf[rs.uniform(size=zbuf.shape) < 0.4] = -1.0
    rgb = rs.uniform(0.0, 1.0, (B, H, W, 3)).astype(np.float32)
    image = rs.uniform(0.0, 1.0, (Ft, H, W, 3)).astype(np.float32)
    for b in range(B):                                           # (with a shared photograph the later images overwrite: still a valid case)
        image[fr[b]] = rgb[b] + rs.uniform(-0.4, 0.4, (H, W, 3)).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    for plane in (zbuf, rgb, image):
        flat = plane.reshape(-1)
        hit = rs.uniform(size=flat.shape) < 0.02
        flat[hit] = bad[rs.randint(0, 3, int(hit.sum()))]
        for value in bad:
            flat[rs.randint(len(flat))] = value
    mask = (rs.uniform(size=(Ft, H, W)) < 0.8).astype(np.uint8) if with_mask else None
    return dict(zbuf=zbuf, rgb=rgb, pose=pose, K=K, image=image, frame=frame, mask=mask, tau=0.5, n=n)
