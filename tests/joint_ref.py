"""The joint-step contract of DESIGN section 23 (kernel K33: tp_joint_align_step), said again in numpy fp64 -- written from the rules in
include/texpose_amd.h, not from the kernels.  The terms' sums are the three restatements' own (silhouette_ref.sums_ref,
photo_ref.sums_ref, icp_ref.sums_ref: matrix products over the kept pixels of an image at once), the combination is the weighted sum
of those dicts in the order silhouette, photometric, depth over the terms that are present and have a weight > 0, and the per-image
part is K29's word for word: gn_ref.solve_ref.  The loop renders with the brute-force rasteriser of tests/mesh_raster_ref.py, one
render per pass for all terms.

The cases of the section's table are tests/occlusion_ref.py's (two bent meshes x two images x three occluders) with a finer texture, a
farther start and a photograph that shows the occluder."""
import functools

import numpy as np

import icp_ref as IREF
import occlusion_ref as OREF
import photo_ref as PHREF
import pnp_ref as PREF
import silhouette_ref as REF
from gn_ref import loop_ref, solve_ref

TERMS = ("sil", "photo", "icp")                                  # the order of the weights and of the sum
WEIGHTS = (1.0, 100.0, 1.0 / 25.0)


# ----------------------------------------------------------------------------------------------------------------- one step
def weighted_sums(sums, weights):
    """sums: the terms' sums_ref dicts in TERMS order (None: absent), weights: three fp32 values -> the combined dict (JtJ, Jtr, cost,
    count, near_ties) over the present terms with a weight > 0, added left to right; None where there is no such term."""
    out = None
    for s, w in zip(sums, weights):
        w = float(np.float32(w))
        if s is None or not w > 0:
            continue
        part = dict(JtJ=w * s["JtJ"], Jtr=w * s["Jtr"], cost=w * s["cost"], count=s["count"], near_ties=s["near_ties"])
        out = part if out is None else {k: out[k] + part[k] for k in part}
    return out


def term_sums(b, K, pose, sil=None, photo=None, icp=None):
    """Image b's sums of each present term (a dict of that term's step_ref arguments, planes batched) in TERMS order."""
    def plane(t, key):
        p = np.asarray(t[key])
        return p[IREF.frame_index(len(pose), len(p), t.get("frame"))[b]]
    mask = lambda t: None if t.get("mask") is None else plane(t, "mask")
    out = [None, None, None]
    if sil is not None:
        sdf = np.asarray(sil["sdf"], np.float32)
        sil = dict(sil, sdf=sdf[None] if sdf.ndim == 2 else sdf)
        out[0] = REF.sums_ref(sil["zbuf"][b], K[b], plane(sil, "sdf"), sil["tau_px"], mask(sil))
    if photo is not None:
        out[1] = PHREF.sums_ref(photo["zbuf"][b], photo["rgb"][b], K[b], plane(photo, "image"), photo["tau"], mask(photo))
    if icp is not None:
        out[2] = IREF.sums_ref(icp["verts"], icp["faces"], icp["zbuf"][b], icp["face"][b], pose[b], K[b], plane(icp, "depth"), icp["tau_mm"], mask(icp))
    return out


def step_ref(pose, K, sil=None, photo=None, icp=None, weights=WEIGHTS, damping=1e-6, evaluate_only=False):
    """The whole call: pose [B,3,4], K [B,3,3] and the present terms -> dict(pose [B,3,4] float32, inliers, status [B], chi2 [B] fp64,
    near_ties [B], rms [B] (NaN: the joint step has none; gn_ref.compare skips it) and per present term '<term>_inliers', '_rms',
    '_status' (its own evaluation of pose) and 'sil_inter', 'sil_uni')."""
    B = len(pose)
    assert any(t is not None and float(np.float32(w)) > 0 for t, w in zip((sil, photo, icp), weights))
    out = dict(pose=np.zeros((B, 3, 4), np.float32), inliers=np.zeros(B, np.int64), status=np.zeros(B, np.int64), chi2=np.zeros(B),
               near_ties=np.zeros(B, np.int64), rms=np.full(B, np.nan))
    for name, t in zip(TERMS, (sil, photo, icp)):
        if t is not None:
            out.update({name + "_inliers": np.zeros(B, np.int64), name + "_rms": np.zeros(B), name + "_status": np.zeros(B, np.int64)})
    if sil is not None:
        out.update(sil_inter=np.zeros(B, np.int64), sil_uni=np.zeros(B, np.int64))
    for b in range(B):
        sums = term_sums(b, K, pose, sil, photo, icp)
        for name, s in zip(TERMS, sums):
            if s is not None:
                _, out[name + "_inliers"][b], out[name + "_rms"][b], out[name + "_status"][b] = solve_ref(s, pose[b], damping, True)
                out["near_ties"][b] += s["near_ties"]            # (a near-tie of any present term: its own outputs are compared too)
        if sums[0] is not None:
            out["sil_inter"][b], out["sil_uni"][b] = sums[0]["inter"], sums[0]["uni"]
        s = weighted_sums(sums, weights)
        out["pose"][b], out["inliers"][b], _, out["status"][b] = solve_ref(s, pose[b], damping, evaluate_only)
        out["chi2"][b] = s["cost"]
    return out


# ----------------------------------------------------------------------------------------------------------------- the loop
@functools.lru_cache(maxsize=None)
def _render_cached(name, texture, pose_bytes, K_bytes, H, W):
    verts, faces = REF.mesh_of(name)
    pose, K = np.frombuffer(pose_bytes, np.float32).reshape(3, 4), np.frombuffer(K_bytes, np.float32).reshape(3, 3)
    z, rgb = PHREF.render_ref(verts, faces, vertex_colours(verts, texture), pose, K, H, W)
    z.setflags(write=False)
    rgb.setflags(write=False)
    return z, rgb


def render_ref(name, texture, pose, K, H, W):
    """(zbuf [H,W], rgb [H,W,3]) float32 (read-only, shared) of mesh ``name`` with vertex_colours(.., texture) at one fp32 pose by the
    brute-force rasteriser; cached: the routes of the table start from the same poses."""
    return _render_cached(name, texture, np.ascontiguousarray(pose, np.float32).tobytes(), np.ascontiguousarray(K, np.float32).tobytes(), H, W)


def joint_ref(name, texture, pose, K, sdf=None, image=None, photo_mask=None, weights=WEIGHTS, tau_px=4.0, tau=0.5, iters=20, damping=1e-6):
    """The loop of ops.joint_align on the silhouette and / or the photometric term with its own raster: iters + 1 passes, one render
    per pass, the pose rounded to fp32 between them, the last evaluate-only -> loop_ref's dict (its rms / rms0 are chi2 / chi20) plus
    the per-pass list `passes`."""
    planes = sdf if sdf is not None else image
    H, W = np.asarray(planes).shape[1:3]
    passes = []
    render = lambda P: [render_ref(name, texture, P[b], K[b], H, W) for b in range(len(P))]

    def step(r, P, t, last):
        z, rgb = np.stack([p[0] for p in r]), np.stack([p[1] for p in r])
        got = step_ref(P, K, sil=None if sdf is None else dict(zbuf=z, sdf=sdf, tau_px=tau_px),
                       photo=None if image is None else dict(zbuf=z, rgb=rgb, image=image, tau=tau, mask=photo_mask),
                       weights=weights, damping=damping, evaluate_only=last)
        got["rms"] = got["chi2"]
        passes.append(got)
        return got

    out = loop_ref(render, step, pose, 0.0, iters)               # (the thresholds are the terms' own, fixed over the passes)
    return dict(out, passes=passes)


# ----------------------------------------------------------------------------------------------------------------- the table's cases
TEXTURE = 3.0            # the table's texture: 0.5 + 0.5 sin(v / 3 + (0, 1, 2)); photo_ref's smooth one is 8.0
START_DEG = 8.0
OCCLUDER_COLOUR = 0.2
CASES = tuple((name, kind) for kind in OREF.OCCLUDERS for name in REF.MESHES)
PHOTO_ALONE_FAILS = (("bent torus", 1, "bottom third"), ("bent torus", 1, "corner disc"), ("bent sphere", 1, "right half"))


def vertex_colours(verts, texture=TEXTURE):
    return (0.5 + 0.5 * np.sin(np.asarray(verts, np.float64) / texture + np.array([0.0, 1.0, 2.0]))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def table_inputs(name, kind, texture=TEXTURE, start_deg=START_DEG):
    """occlusion_ref.occluded_inputs(name, kind) with the bent vertices coloured: the photograph is the brute-force render at the
    true pose over a 0.5 background, the occluder's pixels then set to 0.2, then N(0, 0.02) from RandomState(4) added to every
    value; the start ``start_deg`` degrees and 6 .. 8 mm away (perturbed, RandomState(5)); field = sdf_known_ref(cut, known)."""
    c = OREF.occluded_inputs(name, kind)
    vcolor = vertex_colours(c["verts"], texture)
    image = np.stack([PHREF.render_ref(c["verts"], c["faces"], vcolor, c["P"][b], c["K"][b], c["H"], c["W"], PHREF.BACKGROUND)[1] for b in range(2)])
    image[c["occ"]] = OCCLUDER_COLOUR
    image = (image + np.random.RandomState(4).normal(0.0, PHREF.NOISE_SIGMA, image.shape)).astype(np.float32)
    start = IREF.perturbed(c["P"], np.random.RandomState(5), start_deg)
    return dict(c, texture=texture, vcolor=vcolor, image=image, start=start, field=OREF.sdf_known_ref(c["cut"], c["known"]))


def pose_errors(c, pose):
    return [PREF.pose_error(pose[b], c["P"][b]) for b in range(2)]


ROUTES = ("silhouette 10", "silhouette 10, then photometric 10", "photometric 20", "joint 20, w_photo 25", "joint 20, w_photo 100",
          "joint 20, w_photo 400")


@functools.lru_cache(maxsize=None)
def table_route(name, kind, route, texture=TEXTURE, start_deg=START_DEG):
    """One route of the table on one case (two images) -> dict(status [2], err [(deg, mm)] * 2, want: the loop's dict); tau_px 4,
    tau 0.5, damping 1e-6; run once and shared by the test files."""
    c = table_inputs(name, kind, texture, start_deg)
    args = (name, texture)
    both = dict(sdf=c["field"], image=c["image"], photo_mask=c["known"])
    with np.errstate(all="ignore"):
        if route == "silhouette 10":
            want = joint_ref(*args, c["start"], c["K"], sdf=c["field"], iters=10)
        elif route == "silhouette 10, then photometric 10":
            first = table_route(name, kind, "silhouette 10", texture, start_deg)["want"]
            want = joint_ref(*args, first["pose"], c["K"], image=c["image"], photo_mask=c["known"], weights=(0.0, 1.0, 0.0), iters=10)
        elif route == "photometric 20":
            want = joint_ref(*args, c["start"], c["K"], image=c["image"], photo_mask=c["known"], weights=(0.0, 1.0, 0.0), iters=20)
        else:
            want = joint_ref(*args, c["start"], c["K"], weights=(1.0, float(route.split()[-1]), 0.0), iters=20, **both)
    return dict(status=[int(s) for s in want["status"]], err=pose_errors(c, want["pose"]), want=want)


def converged(err):
    return err[0] <= 1.0 and err[1] <= 5.0


def table(texture=TEXTURE, start_deg=START_DEG, routes=ROUTES):
    """The section's table as text lines: per route the images ending <= 1 deg and <= 5 mm, and the worst image (by rotation)."""
    lines = []
    for route in routes:
        rows = [(e, name, b, kind) for name, kind in CASES for b, e in enumerate(table_route(name, kind, route, texture, start_deg)["err"])]
        worst = max(rows, key=lambda r: r[0][0])
        lines.append("| %s | %d of %d | %.2f deg / %.3g mm (%s %d, %s) |" % (route, sum(converged(r[0]) for r in rows), len(rows), worst[0][0], worst[0][1],
                                                                             worst[1], worst[2], worst[3]))
    return lines


# ----------------------------------------------------------------------------------------------------------------- one step, exact inputs
def one_step_case(seed, B, H, W, frames="one", with_mask=False):
    """The three terms' hand-built one-step cases (silhouette_ref, photo_ref, icp_ref .one_step_case: planted NaN / Inf, bad face
    indices, frame maps that clamp) on SHARED zbuf, pose and K, the silhouette case's: discs with rims, so every term keeps pixels ->
    dict(pose, K, sil, photo, icp): the terms as step_ref takes them, each with its own planes, threshold, frame map and mask."""
    s = REF.one_step_case(seed, B, H, W, frames, with_mask)
    p = PHREF.one_step_case(seed + 1, B, H, W, frames, with_mask)
    i = IREF.one_step_case(seed + 2, B, H, W, frames, with_mask)
    zbuf = s["zbuf"]
    return dict(pose=s["pose"], K=s["K"],
                sil=dict(zbuf=zbuf, sdf=s["sdf"], tau_px=s["tau"], frame=s["frame"], mask=s["mask"]),
                photo=dict(zbuf=zbuf, rgb=p["rgb"], image=p["image"], tau=p["tau"], frame=p["frame"], mask=p["mask"]),
                icp=dict(verts=i["verts"], faces=i["faces"], zbuf=zbuf, face=i["face"], depth=i["depth"], tau_mm=i["tau"], frame=i["frame"], mask=i["mask"]))


SUBSETS = (("sil",), ("photo",), ("icp",), ("sil", "photo"), ("sil", "icp"), ("photo", "icp"), ("sil", "photo", "icp"))
