"""The silhouette-alignment contract of DESIGN section 21 (kernels K31a tp_mask_sdf and K31b tp_silhouette_align_step), said again in
numpy fp64 -- written from the rules in include/texpose_amd.h, not from the kernels.  Where the kernels are free to choose, this file
chooses differently: the distance field is brute force over all pixel pairs (the kernels sweep columns, then rows), the rim test and
the gradients are whole-plane slices, the sums are matrix products over the kept pixels of an image at once (the kernel adds per
thread, wave, workgroup and tile), the counts are numpy's, and the loop renders with the brute-force rasteriser of
tests/mesh_raster_ref.py.  The per-image part (status, step, Gram-Schmidt, fp32 rounding) is K29's word for word: gn_ref.solve_ref.

r = d + 0.5 is one fp64 addition of an fp32 value on both sides and tau_px an fp32 value: keep-or-drop decisions are exact, and no
census of near-ties is needed (the `near_ties` entries the shared loop and bars ask for are zeros)."""
import functools

import numpy as np

import mesh_raster_ref as RR
import pnp_ref as PREF
from gn_ref import loop_ref, solve_ref
from icp_ref import frame_index, perturbed


# ----------------------------------------------------------------------------------------------------------------- K31a
def d2_ref(mask):
    """One plane [H,W] (non-zero: set) -> (d2_set, d2_clear) [H,W] int64: the squared distance of every pixel to the nearest set /
    clear pixel of the plane, H^2 + W^2 where there is none; brute force over all pairs."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    ii, jj = np.mgrid[0:H, 0:W]
    pi, pj = ii.reshape(-1).astype(np.int32), jj.reshape(-1).astype(np.int32)
    out = []
    for sel in (m.reshape(-1), ~m.reshape(-1)):
        qi, qj = pi[sel], pj[sel]
        best = np.full(H * W, H * H + W * W, np.int64)
        if len(qi):
            chunk = max(1, 4000000 // len(qi))
            for s in range(0, H * W, chunk):
                best[s:s + chunk] = ((pi[s:s + chunk, None] - qi[None, :]) ** 2 + (pj[s:s + chunk, None] - qj[None, :]) ** 2).min(1)
        out.append(best.reshape(H, W))
    return out[0], out[1]


def sdf_ref(mask):
    """mask [F,H,W] or [H,W] -> sdf float32 of the same shape: sqrtf(d2_set) - 0.5 on a clear pixel, -(sqrtf(d2_clear) - 0.5) on a
    set one, in fp32 arithmetic."""
    m = np.asarray(mask)
    planes = m[None] if m.ndim == 2 else m
    out = np.empty(planes.shape, np.float32)
    for f, plane in enumerate(planes):
        to_set, to_clear = d2_ref(plane)
        half = np.float32(0.5)
        out[f] = np.where(plane != 0, -(np.sqrt(to_clear.astype(np.float32)) - half), np.sqrt(to_set.astype(np.float32)) - half)
    return out.reshape(m.shape)


# ----------------------------------------------------------------------------------------------------------------- K31b
def covered(z32):
    with np.errstate(all="ignore"):
        return (z32 > 0) & np.isfinite(z32)


def rim_ref(zbuf):
    """[H,W] bool: the interior covered pixels with a neighbour (left, right, above, below) that is not covered."""
    cov = covered(np.asarray(zbuf, np.float32))
    rim = np.zeros_like(cov)
    if cov.shape[0] >= 3 and cov.shape[1] >= 3:
        rim[1:-1, 1:-1] = cov[1:-1, 1:-1] & ~(cov[1:-1, :-2] & cov[1:-1, 2:] & cov[:-2, 1:-1] & cov[2:, 1:-1])
    return rim


def sums_ref(zbuf, K, sdf, tau_px, mask=None):
    """One image: zbuf / sdf / mask [H,W], K [3,3] (fp32 values) -> dict(JtJ [6,6], Jtr [6], cost, count, inter, uni, near_ties = 0,
    kept [H,W] bool)."""
    z32, d32 = np.asarray(zbuf, np.float32), np.asarray(sdf, np.float32)
    H, W = z32.shape
    K = np.asarray(K, np.float32).astype(np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    tau = float(np.float32(tau_px))
    cov = covered(z32)
    with np.errstate(all="ignore"):
        inside = (d32 < 0) & np.isfinite(d32)
    kept = np.zeros((H, W), bool)
    out = dict(JtJ=np.zeros((6, 6)), Jtr=np.zeros(6), cost=0.0, count=0, inter=int((cov & inside).sum()), uni=int((cov | inside).sum()),
               near_ties=0, kept=kept)
    cand = rim_ref(z32)
    if mask is not None:
        cand &= np.asarray(mask) != 0
    d = d32.astype(np.float64)
    fin = np.isfinite(d)
    ok5 = np.zeros((H, W), bool)
    if H >= 3 and W >= 3:
        ok5[1:-1, 1:-1] = fin[1:-1, 1:-1] & fin[1:-1, :-2] & fin[1:-1, 2:] & fin[:-2, 1:-1] & fin[2:, 1:-1]
    with np.errstate(all="ignore"):
        r_all = d + 0.5
        keep = cand & ok5 & (np.abs(r_all) <= tau)
    ii, ji = np.nonzero(keep)
    if len(ii) == 0:
        return out
    kept[ii, ji] = True
    z = z32[ii, ji].astype(np.float64)
    rx, ry = ((ji + 0.5) - cx) / fx, ((ii + 0.5) - cy) / fy
    P = np.stack([z * rx, z * ry, z], 1)
    gx, gy = 0.5 * (d[ii, ji + 1] - d[ii, ji - 1]), 0.5 * (d[ii + 1, ji] - d[ii - 1, ji])
    gfx, gfy = gx * fx, gy * fy
    a = np.stack([gfx / z, gfy / z, -(gfx * rx + gfy * ry) / z], 1)
    J = np.concatenate([np.cross(P, a), a], 1)
    r = r_all[ii, ji]
    out.update(JtJ=J.T @ J, Jtr=J.T @ r, cost=float(r @ r), count=len(ii))
    return out


def step_ref(zbuf, pose, K, sdf, tau_px, damping=1e-6, frame=None, mask=None, evaluate_only=False):
    """The whole call: zbuf [B,H,W], pose [B,3,4], K [B,3,3], sdf [Ft,H,W] (and mask [Ft,H,W]) -> dict(pose [B,3,4] float32, inliers
    [B], rms [B] fp64, status [B], inter [B], uni [B], near_ties [B] (zeros), kept [B,H,W])."""
    B = len(pose)
    sdf = np.asarray(sdf, np.float32)
    sdf = sdf[None] if sdf.ndim == 2 else sdf
    fr = frame_index(B, len(sdf), frame)
    out = dict(pose=np.zeros((B, 3, 4), np.float32), inliers=np.zeros(B, np.int64), rms=np.zeros(B), status=np.zeros(B, np.int64),
               inter=np.zeros(B, np.int64), uni=np.zeros(B, np.int64), near_ties=np.zeros(B, np.int64), kept=np.zeros(np.asarray(zbuf).shape, bool))
    for b in range(B):
        s = sums_ref(zbuf[b], K[b], sdf[fr[b]], tau_px, None if mask is None else np.asarray(mask)[fr[b]])
        out["pose"][b], out["inliers"][b], out["rms"][b], out["status"][b] = solve_ref(s, pose[b], damping, evaluate_only)
        out["inter"][b], out["uni"][b], out["kept"][b] = s["inter"], s["uni"], s["kept"]
    return out


def iou_of(r):
    with np.errstate(all="ignore"):
        return r["inter"] / r["uni"].astype(np.float64)


# ----------------------------------------------------------------------------------------------------------------- the loop
def bent(v):
    """The loop's meshes, made asymmetric: y *= 0.6, z += 0.006 x^2 - 8, x += 0.3 y + 0.2 |z|, in that order, each with the values
    already updated."""
    v = np.asarray(v, np.float64).copy()
    v[:, 1] *= 0.6
    v[:, 2] += 0.006 * v[:, 0] ** 2 - 8.0
    v[:, 0] += 0.3 * v[:, 1] + 0.2 * np.abs(v[:, 2])
    return v.astype(np.float32)


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    """'sphere', 'torus' (pnp_ref.end_to_end_inputs' meshes) or 'bent sphere', 'bent torus' -> (verts, faces)."""
    e = PREF.end_to_end_inputs(name.split()[-1])
    return (bent(e["verts"]) if name.startswith("bent") else e["verts"]), e["faces"]


@functools.lru_cache(maxsize=None)
def _render_cached(name, pose_bytes, K_bytes, H, W):
    verts, faces = mesh_of(name)
    pose, K = np.frombuffer(pose_bytes, np.float32).reshape(3, 4).astype(np.float64), np.frombuffer(K_bytes, np.float32).reshape(3, 3).astype(np.float64)
    cam = np.asarray(verts, np.float64) @ pose[:, :3].T + pose[:, 3]
    assert (cam[:, 2] > 1.0).all()                               # (in front of the camera: the box below holds every covered pixel)
    u, v = K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2], K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]
    j0, j1 = max(0, int(np.floor(u.min())) - 1), min(W, int(np.ceil(u.max())) + 2)
    i0, i1 = max(0, int(np.floor(v.min())) - 1), min(H, int(np.ceil(v.max())) + 2)
    pixels = (np.arange(i0, i1)[:, None] * W + np.arange(j0, j1)[None, :]).reshape(-1)
    zbuf = np.full(H * W, -1.0)
    if len(pixels):
        r = RR.rasterize(verts, faces, pose, K, H, W, pixels=pixels)
        hit = r["face"] >= 0
        zbuf[pixels[hit]] = r["zbuf"][hit]
    zbuf = zbuf.reshape(H, W).astype(np.float32)
    zbuf.setflags(write=False)
    return zbuf


def render_ref(name, pose, K, H, W):
    """zbuf [H,W] float32 (-1 background; read-only, shared) of mesh ``name`` at one fp32 pose by the brute-force rasteriser, asked
    only for the pixels of the projected vertices' bounding box, as photo_ref.render_ref; cached across the test files."""
    return _render_cached(name, np.ascontiguousarray(pose, np.float32).tobytes(), np.ascontiguousarray(K, np.float32).tobytes(), H, W)


def silhouette_ref(name, pose, K, sdf, tau_px=4.0, iters=10, damping=1e-6, frame=None, mask=None):
    """The loop of ops.silhouette_align with its own raster -> loop_ref's dict plus iou, iou0 [B] and the per-pass list `passes`."""
    sdf = np.asarray(sdf, np.float32)
    H, W = sdf.shape[-2:]
    passes = []
    render = lambda P: np.stack([render_ref(name, P[b], K[b], H, W) for b in range(len(P))])

    def step(planes, P, t, last):
        passes.append(step_ref(planes, P, K, sdf, t, damping, frame, mask, evaluate_only=last))
        return passes[-1]

    out = loop_ref(render, step, pose, tau_px, iters)
    return dict(out, iou=iou_of(passes[-1]), iou0=iou_of(passes[0]), passes=passes)


MESHES = ("bent sphere", "bent torus")


@functools.lru_cache(maxsize=None)
def loop_inputs(name):
    """pnp_ref.end_to_end_inputs (64 x 80, two poses about 900 mm away) with mesh ``name``: the measured masks are the brute-force
    coverage at the true poses, sdf their brute-force field, the start 3 degrees and 6 .. 8 mm away."""
    e = PREF.end_to_end_inputs(name.split()[-1])
    verts, faces = mesh_of(name)
    K = np.tile(e["K"], (2, 1, 1))
    mask = np.stack([render_ref(name, e["P"][b], K[b], e["H"], e["W"]) > 0 for b in range(2)]).astype(np.uint8)
    start = perturbed(e["P"], np.random.RandomState(5), 3.0)
    return dict(e, name=name, verts=verts, faces=faces, K=K, mask=mask, sdf=sdf_ref(mask), start=start)


@functools.lru_cache(maxsize=None)
def loop_case(name):
    """The restatement's loop (10 steps, tau 4 px, damping 1e-6) on loop_inputs, run once per case and shared by the test files."""
    c = loop_inputs(name)
    return dict(c, want=silhouette_ref(name, c["start"], c["K"], c["sdf"], 4.0, 10, 1e-6))


# ----------------------------------------------------------------------------------------------------------------- one step, exact inputs
def discs(rs, shape, n=3):
    """[B,H,W] bool: a few random discs per plane (radius up to a third of the smaller side), so that rims exist."""
    B, H, W = shape
    ii, jj = np.mgrid[0:H, 0:W]
    out = np.zeros(shape, bool)
    for b in range(B):
        for _ in range(n):
            ci, cj, rad = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(1.0, max(1.5, min(H, W) / 3.0))
            out[b] |= (ii - ci) ** 2 + (jj - cj) ** 2 <= rad * rad
    return out


def one_step_case(seed, B, H, W, frames="one", with_mask=False, field="shifted"):
    """Hand-built planes for one step (no rasteriser): per image a pose about 900 mm away, zbuf 880 .. 920 mm inside a few random
    discs, 2 % of its values NaN or +-Inf plus one of each planted by hand.  ``field`` 'shifted': sdf is the distance field of the
    coverage moved by (1, -1) pixels, `measured` (sdf_ref here; 'measured' leaves it to the caller: the GPU test takes the kernel's);
    'random': U(-3, 3) with 2 % NaN / Inf.
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
    inside = discs(rs, (B, H, W))
    zbuf = np.where(inside, rs.uniform(880.0, 920.0, (B, H, W)), -1.0).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf], np.float32)
    measured = np.zeros((Ft, H, W), np.uint8)
    for b in range(B):                                           # (with a shared plane the later images overwrite: still a valid case)
        measured[fr[b]] = np.roll(inside[b], (1, -1), (0, 1))
    if field == "shifted":
        sdf = sdf_ref(measured)
    elif field == "measured":                                    # the caller's: the kernel's field of `measured`
        sdf = None
    else:
        sdf = rs.uniform(-3.0, 3.0, (Ft, H, W)).astype(np.float32)
    for plane in (zbuf,) + ((sdf,) if field == "random" else ()):
        flat = plane.reshape(-1)
        hit = rs.uniform(size=flat.shape) < 0.02
        flat[hit] = bad[rs.randint(0, 3, int(hit.sum()))]
        for value in bad:
            flat[rs.randint(len(flat))] = value
    mask = (rs.uniform(size=(Ft, H, W)) < 0.8).astype(np.uint8) if with_mask else None
    # tau: below the largest |r| of either field (about 2.4 px one diagonal pixel away, 3.5 px for the random one): both decisions occur
    return dict(zbuf=zbuf, pose=pose, K=K, sdf=sdf, measured=measured, frame=frame, mask=mask, tau=2.0 if field == "random" else 1.0)
