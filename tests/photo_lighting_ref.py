"""The lighting contract of DESIGN section 30 (kernel K40: tp_photo_lighting), said again in numpy fp64 -- written from the rules in
include/texpose_amd.h, not from the kernels.  Where the kernel is free to choose, this file chooses differently: the face normals are
computed for all F faces at once and looked up per pixel, the keep rule is a whole-plane mask, the 64 sums are np.sum over an image's
kept pixels at once (the kernel adds per thread, wave, workgroup and tile), and the loop is tests/photo_ref.py's, on its brute-force
raster, with the fit in front of each step_ref.

Besides the results it reports what decides whether a comparison of counts can be exact: near-ties, kept-or-dropped decisions whose
margin | |o - (l . x + beta)| - tau | is below NEAR_TIE colour units.

FIGURES: tests/golden/photo_lighting_loops.npz holds this file's own loop results (golden_arrays() below wrote it); DESIGN section 30
has the table and tests/test_photo_lighting_cpu.py asserts it."""
import functools
import os

import numpy as np

import mesh_raster_ref as RR
import photo_exposure_ref as XREF
import photo_ref as PR
import pnp_ref as PREF
from gn_ref import loop_ref
from icp_ref import frame_index

NEAR_TIE = 1e-9          # colour units
MIN_COUNT = 6
PIVOT_TOL = 1e-10        # cholesky6's
CLAMPED, FLAT, FALLBACK = 1, 8, 64     # flags: << channel
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 0.0], np.float32)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photo_lighting_loops.npz")


# ----------------------------------------------------------------------------------------------------------------- normals
def face_normals_ref(verts, faces, pose):
    """verts [V,3], faces [F,3] (any integers), pose [3,4] -> (n [F,3] fp64: the face's own normal in the camera frame, unit, facing
    the camera; valid [F]: every index in [0, V) and dot(n, n) finite and > 0).  Invalid rows hold 0."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    P = np.asarray(pose, np.float32).astype(np.float64)
    V = len(v)
    ok = ((f >= 0) & (f < V)).all(1)
    g = np.where(ok[:, None], f, 0)
    with np.errstate(all="ignore"):
        v0, v1, v2 = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
        a, b = v1 - v0, v2 - v0
        m = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        n = np.stack([(P[r, 0] * m[:, 0] + P[r, 1] * m[:, 1]) + P[r, 2] * m[:, 2] for r in range(3)], 1)
        d = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        ok &= np.isfinite(d) & (d > 0)
        n = n / np.sqrt(d)[:, None]
        xc = np.stack([((P[r, 0] * v0[:, 0] + P[r, 1] * v0[:, 1]) + P[r, 2] * v0[:, 2]) + P[r, 3] for r in range(3)], 1)
        away = (n[:, 0] * xc[:, 0] + n[:, 1] * xc[:, 1]) + n[:, 2] * xc[:, 2] > 0
        n = np.where(away[:, None], -n, n)
    return np.where(ok[:, None], n, 0.0), ok


def pixel_normals_ref(verts, faces, face, pose):
    """face [H,W] int (anything) -> (n [H,W,3] fp64, valid [H,W]) by the rule above; a face index outside [0, F) is invalid."""
    n, ok = face_normals_ref(verts, faces, pose)
    f = np.asarray(face).astype(np.int64)
    inside = (f >= 0) & (f < len(n))
    g = np.where(inside, f, 0)
    valid = inside & ok[g]
    return np.where(valid[..., None], n[g], 0.0), valid


# ----------------------------------------------------------------------------------------------------------------- the fit
def _cholesky_solve(A, r):
    """The 5 x 5 system by Cholesky with cholesky6's pivot rule -> x [5] or None."""
    L = A.copy()
    for j in range(5):
        diag = L[j, j]
        d = diag - (L[j, :j] ** 2).sum()
        if not np.isfinite(d) or not d > PIVOT_TOL * diag or not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, 5):
            L[i, j] = (L[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    L = np.tril(L)
    return np.linalg.solve(L.T, np.linalg.solve(L, r))


def fit_ref(verts, faces, face, zbuf, rgb, pose, image, tau, light_in=None, mask=None, gain_range=(0.25, 4.0), min_var=1e-6):
    """One image: face / zbuf / mask [H,W], rgb / image [H,W,3], pose [3,4], light_in [3,5] or None -> dict(light [3,5] float32, count,
    rms (fp64), status, flags, near_ties, kept [H,W] bool)."""
    z32, c32, o32 = np.asarray(zbuf, np.float32), np.asarray(rgb, np.float32), np.asarray(image, np.float32)
    H, W = z32.shape
    l32 = np.tile(IDENTITY, (3, 1)) if light_in is None else np.asarray(light_in, np.float32).reshape(3, 5)
    tau, lo, hi, min_var = (float(np.float32(v)) for v in (tau, gain_range[0], gain_range[1], min_var))
    nrm, valid = pixel_normals_ref(verts, faces, face, pose)
    with np.errstate(all="ignore"):
        c, o = c32.astype(np.float64), o32.astype(np.float64)
        keep = np.zeros((H, W), bool)
        keep[1:-1, 1:-1] = True                                  # (H < 3 or W < 3: nothing)
        keep &= (z32 > 0) & np.isfinite(z32)
        if mask is not None:
            keep &= np.asarray(mask) != 0
        keep &= np.isfinite(c).all(-1) & np.isfinite(o).all(-1)
        keep &= valid
        X = np.stack([c, c * nrm[..., 0:1], c * nrm[..., 1:2], c * nrm[..., 2:3], np.ones_like(c)], -1)      # [H,W,3 channels,5]
        l = l32.astype(np.float64)
        pred = (((l[:, 0] * X[..., 0] + l[:, 1] * X[..., 1]) + l[:, 2] * X[..., 2]) + l[:, 3] * X[..., 3]) + l[:, 4]
        r = o - pred
        d2 = (r[..., 0] ** 2 + r[..., 1] ** 2) + r[..., 2] ** 2
        ties = int((keep & (np.abs(np.sqrt(d2) - tau) < NEAR_TIE)).sum())
        keep &= d2 <= tau * tau
        n = float(keep.sum())
        Xk, ok = X[keep], o[keep]                                # [n,3,5], [n,3]
        iu, ju = np.triu_indices(5)                              # row-major upper triangle
        SA = (Xk[..., iu] * Xk[..., ju]).sum(0)                  # [3,15]   (every sum runs over the pixels in ascending order, as
        Sr = (Xk * ok[..., None]).sum(0)                         # [3,5]     photo_exposure_ref's do: the sub-sums are its bits)
        Soo3 = (ok * ok).sum(0)                                  # [3]
        light, sse, flags = np.zeros((3, 5)), np.zeros(3), 0
        for k in range(3):
            A = np.zeros((5, 5))
            A[iu, ju] = A[ju, iu] = SA[k]
            rhs, Soo = Sr[k], Soo3[k]
            x = _cholesky_solve(A, rhs) if n > 0 else None
            if x is not None and not (np.isfinite(x).all() and lo <= x[0] <= hi and np.sqrt((x[1] * x[1] + x[2] * x[2]) + x[3] * x[3]) <= x[0]):
                x = None
            if x is None:                                        # K37's closed form on the record's own sub-sums
                flags |= FALLBACK << k
                Sc, So, Scc, Sco = A[0, 4], rhs[4], A[0, 0], rhs[0]
                mc, mo = Sc / n, So / n
                var, cov = Scc / n - mc * mc, Sco / n - mc * mo
                g = 1.0
                if var > min_var:
                    q = cov / var
                    g = min(max(q, lo), hi)
                    flags |= (CLAMPED << k) if g != q else 0
                else:
                    flags |= FLAT << k
                x = np.array([g, 0.0, 0.0, 0.0, mo - g * mc])
            xr = (((x[0] * rhs[0] + x[1] * rhs[1]) + x[2] * rhs[2]) + x[3] * rhs[3]) + x[4] * rhs[4]
            Ax = [(((A[i, 0] * x[0] + A[i, 1] * x[1]) + A[i, 2] * x[2]) + A[i, 3] * x[3]) + A[i, 4] * x[4] for i in range(5)]
            xAx = (((x[0] * Ax[0] + x[1] * Ax[1]) + x[2] * Ax[2]) + x[3] * Ax[3]) + x[4] * Ax[4]
            sse[k] = (Soo - 2.0 * xr) + xAx
            light[k] = x
        rms = np.sqrt(np.maximum(0.0, (sse[0] + sse[1]) + sse[2]) / n)
        new32 = light.astype(np.float32)
    status = 1 if n < MIN_COUNT else (0 if np.isfinite(new32).all() and np.isfinite(np.float32(rms)) else 3)
    return dict(light=new32 if status == 0 else l32.copy(), count=int(n), rms=float(rms), status=status, flags=flags, near_ties=ties, kept=keep)


def apply_ref(verts, faces, face, zbuf, rgb, pose, light):
    """One image's rgb [H,W,3] under light [3,5] on the pixels with a surface, the rest unchanged: the shading s = ((l0 + l1 n_x) + l2
    n_y) + l3 n_z in fp64, rounded to fp32 once (l0 itself where the pixel has no valid normal), then two fp32 operations, s * c and
    + beta."""
    z32, c32, l32 = np.asarray(zbuf, np.float32), np.asarray(rgb, np.float32), np.asarray(light, np.float32).reshape(3, 5)
    nrm, valid = pixel_normals_ref(verts, faces, face, pose)
    with np.errstate(all="ignore"):
        l = l32.astype(np.float64)
        s = ((l[:, 0] + l[:, 1] * nrm[..., 0:1]) + l[:, 2] * nrm[..., 1:2]) + l[:, 3] * nrm[..., 2:3]        # [H,W,3]
        s32 = np.where(valid[..., None], s.astype(np.float32), l32[:, 0])
        lit = s32 * c32
        lit = lit + l32[:, 4]
        return np.where(((z32 > 0) & np.isfinite(z32))[..., None], lit, c32).astype(np.float32)


def lighting_ref(verts, faces, face, zbuf, rgb, pose, image, tau, light_in=None, frame=None, mask=None, gain_range=(0.25, 4.0), min_var=1e-6):
    """The whole call: face / zbuf [B,H,W], rgb [B,H,W,3], pose [B,3,4], image [Ft,H,W,3] (and mask [Ft,H,W]), light_in [B,3,5] or None
    -> dict(light [B,3,5] float32, count, status, flags, near_ties [B], rms [B] fp64, kept [B,H,W], rgb [B,H,W,3] float32)."""
    B = len(zbuf)
    image = np.asarray(image, np.float32)
    fr = frame_index(B, len(image), frame)
    per = [fit_ref(verts, faces, face[b], zbuf[b], rgb[b], pose[b], image[fr[b]], tau, None if light_in is None else light_in[b],
                   None if mask is None else np.asarray(mask)[fr[b]], gain_range, min_var) for b in range(B)]
    out = {k: np.stack([np.asarray(p[k]) for p in per]) for k in per[0]}
    out["rgb"] = np.stack([apply_ref(verts, faces, face[b], zbuf[b], rgb[b], pose[b], out["light"][b]) for b in range(B)])
    return out


# ----------------------------------------------------------------------------------------------------------------- the loop
def render_ref(verts, faces, vcolor, pose, K, H, W, background=None):
    """photo_ref.render_ref with the face plane: zbuf [H,W] float32 (-1 background), rgb [H,W,3] float32, face [H,W] int32 (-1)."""
    pose, K = np.asarray(pose, np.float64), np.asarray(K, np.float64)
    cam = np.asarray(verts, np.float64) @ pose[:, :3].T + pose[:, 3]
    assert (cam[:, 2] > 1.0).all()
    u, v = K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2], K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]
    j0, j1 = max(0, int(np.floor(u.min())) - 1), min(W, int(np.ceil(u.max())) + 2)
    i0, i1 = max(0, int(np.floor(v.min())) - 1), min(H, int(np.ceil(v.max())) + 2)
    pixels = (np.arange(i0, i1)[:, None] * W + np.arange(j0, j1)[None, :]).reshape(-1)
    zbuf, rgb = np.full(H * W, -1.0), np.full((H * W, 3), 0.0 if background is None else float(background))
    face = np.full(H * W, -1, np.int32)
    if len(pixels):
        r = RR.rasterize(verts, faces, pose, K, H, W, pixels=pixels, vcolor=vcolor)
        hit = r["face"] >= 0
        zbuf[pixels[hit]], rgb[pixels[hit]], face[pixels[hit]] = r["zbuf"][hit], r["rgb"][hit], r["face"][hit]
    return zbuf.reshape(H, W).astype(np.float32), rgb.reshape(H, W, 3).astype(np.float32), face.reshape(H, W)


def photo_lighting_loop_ref(verts, faces, vcolor, pose, K, image, tau=0.5, iters=10, damping=1e-6, frame=None, mask=None, tau0=2.0,
                            gain_range=(0.25, 4.0), min_var=1e-6):
    """ops.photo_align(lighting=True) on the brute-force raster: every pass fits (the first within tau0 of the plain colours, the later
    ones within that pass's tau of the fit before), rewrites the rendered colours and hands them to step_ref -> loop_ref's dict and
    light [B,3,5], lighting_status, lighting_flags [B] of the last pass; near_ties counts the fits' too."""
    image = np.asarray(image, np.float32)
    H, W = image.shape[1:3]
    fit, ties = {}, [np.zeros(len(pose), np.int64)]
    render = lambda P: [render_ref(verts, faces, vcolor, P[b], K[b], H, W) for b in range(len(P))]

    def step(planes, P, t, last):
        zbuf, rgb, face = (np.stack([p[k] for p in planes]) for k in range(3))
        e = lighting_ref(verts, faces, face, zbuf, rgb, P, image, t if fit else tau0, fit.get("light"), frame, mask, gain_range, min_var)
        fit.update(light=e["light"], lighting_status=e["status"], lighting_flags=e["flags"])
        ties[0] = np.maximum(ties[0], e["near_ties"])
        return PR.step_ref(zbuf, e["rgb"], P, K, image, t, damping, frame, mask, evaluate_only=last)

    out = loop_ref(render, step, pose, tau, iters)
    return dict(out, near_ties=np.maximum(out["near_ties"], ties[0]), **fit)


# ----------------------------------------------------------------------------------------------------------------- the loop's cases
AMBIENT = np.array([0.70, 0.75, 0.65])                           # tinted
DIRECTION = np.array([-1.0, -1.0, -1.0]) / np.sqrt(3.0)          # towards the lamp, camera frame (x right, y down, z forward): upper left, in front
STRENGTH = 0.45                                                  # the directional magnitude over the ambient
STRONG = 0.9                                                     # the stronger row
BIAS = XREF.EXPOSURE_BIAS
MESHES = ("sphere", "torus")
LOOPS = ("plain", "exposure", "lighting")


def true_light(strength=STRENGTH):
    """[3,5] float32: ambient, ambient * strength * DIRECTION, K37's bias."""
    return np.concatenate([AMBIENT[:, None], AMBIENT[:, None] * strength * DIRECTION[None, :], BIAS[:, None]], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def loop_inputs(mesh, noisy, strength=STRENGTH):
    """photo_ref.loop_inputs with the photograph relit: the true-pose rendering over the 0.5 background under true_light(strength) by
    this file's apply (background pixels, which have no normal, take the ambient form by hand); where ``noisy``, photo_ref's own noise
    (sigma 0.02) is added AFTER, as a sensor would."""
    c, clean = PR.loop_inputs(mesh, noisy), PR.loop_inputs(mesh, False)["image"]
    noise = c["image"].astype(np.float64) - clean
    L = true_light(strength)
    lit = []
    for b in range(len(c["P"])):
        z, rgb, face = render_ref(c["verts"], c["faces"], c["vcolor"], c["P"][b], c["K"][b], c["H"], c["W"], PR.BACKGROUND)
        img = apply_ref(c["verts"], c["faces"], face, z, rgb, c["P"][b], L)
        lit.append(np.where((z > 0)[..., None], img, L[:, 0] * rgb + L[:, 4]).astype(np.float32))
    return dict(c, image=(np.stack(lit).astype(np.float64) + noise).astype(np.float32), plain_image=c["image"], light=L)


@functools.lru_cache(maxsize=None)
def loop_case(mesh, noisy, loop="lighting", strength=STRENGTH):
    """One loop (10 steps, tau 0.5, damping 1e-6), run once per case and shared by the test files: ``loop`` one of LOOPS."""
    c = loop_inputs(mesh, noisy, strength)
    run = dict(plain=PR.photo_ref, exposure=XREF.photo_exposure_loop_ref, lighting=photo_lighting_loop_ref)[loop]
    return dict(c, want=run(c["verts"], c["faces"], c["vcolor"], c["start"], c["K"], c["image"], 0.5, 10, 1e-6))


def errors(c, pose):
    """[(deg, mm)] per image of ``pose`` against the case's truth."""
    return [PREF.pose_error(np.asarray(pose)[b], c["P"][b]) for b in range(len(c["P"]))]


# ----------------------------------------------------------------------------------------------------------------- the joint and the multi-view loop
JOINT_CASE = XREF.JOINT_CASE                                     # K37's: ("bent sphere", "corner disc")


def relit(c, image, P, strength=STRENGTH):
    """Photographs ``image`` [B,H,W,3] of the case ``c`` (verts, faces, vcolor, K, H, W) taken at the poses P under true_light(strength):
    a pixel the mesh covers at P is shaded by its face's normal, every other pixel takes the ambient form; occluder, background and noise
    included, as K37's ``changed``."""
    L = true_light(strength)
    out = []
    for b in range(len(P)):
        z, _, face = render_ref(c["verts"], c["faces"], c["vcolor"], P[b], c["K"][b], c["H"], c["W"])
        lit = apply_ref(c["verts"], c["faces"], face, z, image[b], P[b], L)
        out.append(np.where((z > 0)[..., None], lit, L[:, 0] * np.asarray(image[b], np.float32) + L[:, 4]).astype(np.float32))
    return np.stack(out)


def _lit_step(c, image, mask, fit, prefix, tau, tau0):
    """render and the fit in front of a joint / multi-view step: P -> (zbuf, lit rgb) with ``fit`` updated."""
    def run(P):
        planes = [render_ref(c["verts"], c["faces"], c["vcolor"], P[b], c["K"][b], c["H"], c["W"]) for b in range(len(P))]
        z, rgb, face = (np.stack([p[k] for p in planes]) for k in range(3))
        e = lighting_ref(c["verts"], c["faces"], face, z, rgb, P, image, tau if fit else tau0, fit.get(prefix + "light"), None, mask)
        fit.update({prefix + "light": e["light"], prefix + "lighting_status": e["status"], prefix + "lighting_flags": e["flags"]})
        return z, e["rgb"]
    return run


def joint_lighting_loop_ref(c, image, weights=None, tau_px=4.0, tau=0.5, iters=20, damping=1e-6, tau0=2.0):
    """joint_ref.joint_ref (silhouette + photometric) with the fit in front of each step, as ops.joint_align(lighting=True): the
    photometric term's mask is the fit's -> loop_ref's dict and photo_light, photo_lighting_status, photo_lighting_flags."""
    import joint_ref as JREF
    fit = {}
    lit = _lit_step(c, image, c["known"], fit, "photo_", tau, tau0)

    def step(P_again, P, t, last):
        z, rgb = lit(P)
        got = JREF.step_ref(P, c["K"], sil=dict(zbuf=z, sdf=c["field"], tau_px=tau_px), photo=dict(zbuf=z, rgb=rgb, image=image, tau=tau, mask=c["known"]),
                            weights=JREF.WEIGHTS if weights is None else weights, damping=damping, evaluate_only=last)
        got["rms"] = got["chi2"]
        return got

    return dict(loop_ref(lambda P: P, step, c["start"], 0.0, iters), **fit)


@functools.lru_cache(maxsize=None)
def joint_inputs():
    """K37's joint case with the photographs relit (plain_image: as they were)."""
    import joint_ref as JREF
    c = JREF.table_inputs(*JOINT_CASE)
    return dict(c, image=relit(c, c["image"], c["P"]), plain_image=c["image"])


@functools.lru_cache(maxsize=None)
def multiview_inputs():
    """multiview_ref's two-view group of JOINT_CASE with the photographs relit, each view under the same camera-frame light."""
    import multiview_ref as MREF
    c = MREF.loop_inputs(*JOINT_CASE)
    return dict(c, image=relit(c, c["image"], c["P"]), plain_image=c["image"])


@functools.lru_cache(maxsize=None)
def joint_case():
    """K37's joint case (two images, the occluder's pixels unknown, noise 0.02, start 8 degrees away) relit, through the loop above."""
    import joint_ref as JREF
    c = joint_inputs()
    with np.errstate(all="ignore"):
        want = joint_lighting_loop_ref(c, c["image"])
    return dict(c, want=want, err=JREF.pose_errors(c, want["pose"]))


def multiview_lighting_loop_ref(c, image, weights=(1.0, 100.0, 0.0), tau_px=4.0, tau=0.5, iters=20, damping=1e-6, tau0=2.0):
    """multiview_ref.multiview_ref (silhouette + photometric) with the fit in front of each step at the composed poses, one light per
    view -> its dict and photo_light, photo_lighting_status, photo_lighting_flags."""
    import multiview_ref as MREF
    fit = {}
    lit = _lit_step(c, image, c["known"], fit, "photo_", tau, tau0)
    model = np.asarray(c["model_start"], np.float32).copy()
    first = status = got = None
    for it in range(iters + 1):
        z, rgb = lit(MREF.compose_ref(c["cam"], model, c["group"]))
        got = MREF.step_ref(model, c["cam"], c["group"], c["K"], sil=dict(zbuf=z, sdf=c["field"], tau_px=tau_px),
                            photo=dict(zbuf=z, rgb=rgb, image=image, tau=tau, mask=c["known"]), weights=weights, damping=damping, evaluate_only=it == iters)
        first = got if first is None else first
        status = got["status"] if it < iters or status is None else status
        model = got["model"]
    return dict(model=got["model"], pose=got["pose"], inliers=got["inliers"], chi2=got["chi2"], views=got["views"], status=status,
                inliers0=first["inliers"], chi20=first["chi2"], **fit)


@functools.lru_cache(maxsize=None)
def multiview_case():
    """multiview_inputs() through the loop above."""
    c = multiview_inputs()
    with np.errstate(all="ignore"):
        want = multiview_lighting_loop_ref(c, c["image"])
    return dict(c, want=want, err=PREF.pose_error(want["model"][0], c["model_true"]))


def golden_more():
    """The joint and the multi-view loop's recorded results."""
    j, m = joint_case(), multiview_case()
    return {"joint/pose": j["want"]["pose"], "joint/err": np.array(j["err"]), "joint/light": j["want"]["photo_light"],
            "joint/status": np.asarray(j["want"]["status"], np.int64), "joint/lighting_status": np.asarray(j["want"]["photo_lighting_status"], np.int64),
            "multiview/model": m["want"]["model"], "multiview/err": np.array(m["err"]), "multiview/light": m["want"]["photo_light"],
            "multiview/status": np.asarray(m["want"]["status"], np.int64)}


def golden_arrays(strengths=(STRENGTH, STRONG)):
    """What tests/golden/photo_lighting_loops.npz holds: per strength, mesh, noise and loop the restatement's final poses [2,3,4], their
    errors [2,2] (deg, mm) and, for the lighting loop, the light [2,3,5]; 'start_err' per mesh; golden_more()'s joint and multi-view
    results.  np.savez_compressed(GOLDEN, **golden_arrays()) writes the file (about three minutes)."""
    out = {}
    for mesh in MESHES:
        out["start_err/%s" % mesh] = np.array(errors(loop_inputs(mesh, False), loop_inputs(mesh, False)["start"]))
        for s in strengths:
            for noisy in (False, True):
                for loop in LOOPS:
                    c = loop_case(mesh, noisy, loop, s)
                    key = "%.2f/%s/%s/%s" % (s, mesh, "noisy" if noisy else "clean", loop)
                    out[key + "/pose"] = c["want"]["pose"]
                    out[key + "/err"] = np.array(errors(c, c["want"]["pose"]))
                    if loop == "lighting":
                        out[key + "/light"] = c["want"]["light"]
                        out[key + "/flags"] = np.asarray(c["want"]["lighting_flags"], np.int64)
    out.update(golden_more())
    return out


def golden():
    return dict(np.load(GOLDEN))


# ----------------------------------------------------------------------------------------------------------------- one call, exact inputs
def bumpy_mesh(seed=0, n=9):
    """A small height field with random heights: (n - 1)^2 * 2 faces whose normals all differ, ~100 mm across, centred."""
    rs = np.random.RandomState(seed)
    g = np.linspace(-50.0, 50.0, n)
    X, Y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([X, Y, rs.uniform(-12.0, 12.0, X.shape)], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
    f = np.concatenate([np.stack([a, b, d], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])     # (the two halves wind oppositely)
    return v, f.astype(np.int32)


def quad_mesh():
    """Two coplanar triangles."""
    v = np.array([[-40, -40, 0], [40, -40, 0], [40, 40, 0], [-40, 40, 0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def one_call_case(seed, B, H, W, frames="one", with_mask=False, with_fit=False, mesh=None):
    """photo_exposure_ref.one_call_case's planes plus a mesh (bumpy_mesh), a face plane uniform over its faces (no rasteriser: the call
    takes the planes as they are), random poses about 900 mm away, and the photograph made from a random light per image: image =
    s(n) rgb + beta + U(-0.2, 0.2) with ambient in [0.6, 1.4], a directional part of up to 0.5 of it and beta in [-0.1, 0.1], then the
    NaN / Inf of that builder.  ``with_fit``: light_in near the truth."""
    c = XREF.one_call_case(seed, B, H, W, frames, with_mask, False)
    rs = np.random.RandomState(seed + 1000)
    verts, faces = bumpy_mesh(seed) if mesh is None else mesh
    face = rs.randint(0, len(faces), (B, H, W)).astype(np.int32)
    pose = np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        pose[b] = np.concatenate([q, rs.uniform(-15, 15, (3, 1)) + [[0.0], [0.0], [900.0]]], 1)
    amb = rs.uniform(0.6, 1.4, (B, 3))
    d = rs.normal(size=(B, 3, 3))
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * rs.uniform(0.1, 0.5, (B, 3, 1)) * amb[..., None]
    light = np.concatenate([amb[..., None], d, rs.uniform(-0.1, 0.1, (B, 3, 1))], -1)
    fr = frame_index(B, len(c["image"]), c["frame"])
    image = c["image"].copy()
    bad = ~np.isfinite(image)
    with np.errstate(all="ignore"):
        for b in range(B):
            lit = apply_ref(verts, faces, face[b], np.full((H, W), 900.0, np.float32), np.nan_to_num(c["rgb"][b], nan=0.5, posinf=0.5, neginf=0.5), pose[b],
                            light[b])
            image[fr[b]] = (lit + rs.uniform(-0.2, 0.2, (H, W, 3))).astype(np.float32)
    image[bad] = c["image"][bad]                                 # the planted NaN / Inf stay where they were
    light_in = (light + rs.uniform(-0.02, 0.02, light.shape)).astype(np.float32) if with_fit else None
    return dict(verts=verts, faces=faces, face=face, zbuf=c["zbuf"], rgb=c["rgb"], pose=pose, image=image, frame=c["frame"], mask=c["mask"],
                light_in=light_in, tau=0.5, true_light=light)


def call_ref(c, **kw):
    return lighting_ref(c["verts"], c["faces"], c["face"], c["zbuf"], c["rgb"], c["pose"], c["image"], c["tau"], c["light_in"], c["frame"], c["mask"], **kw)
