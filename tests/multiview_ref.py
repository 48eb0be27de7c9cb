"""The multi-view contract of DESIGN section 29 (kernel K39: tp_pose_compose, tp_multiview_align_step), said again in numpy fp64 --
written from the rules in include/texpose_amd.h, not from the kernels.  A view's combined sums are joint_ref's (term_sums,
weighted_sums) at the composed pose; the change of variables is spelled out entry by entry in the header's order (P = H A, Q = A^T P,
g' = A^T g, inner index ascending); a group's sums are its member views' in ascending view index, the first assigned; the per-group
part is K29's word for word (gn_ref.solve_ref).  The loop renders with the brute-force rasteriser through joint_ref.render_ref.

The loop cases are joint_ref's twelve occluded images read as six two-view problems: the two images of one shape under one occluder
are two views of one object."""
import functools

import numpy as np

import joint_ref as JREF
import pnp_ref as PREF
from gn_ref import solve_ref

WEIGHTS = JREF.WEIGHTS
IDENTITY = np.eye(3, 4, dtype=np.float32)


# ----------------------------------------------------------------------------------------------------------------- compose
def is_identity(cam):
    """cam [3,4] float32 is bit-exactly [I|0]: the words of 1.0f and of +0.0f (a -0.0 is not)."""
    return np.array_equal(np.ascontiguousarray(cam, np.float32).view(np.uint32), IDENTITY.view(np.uint32))


def compose_one(cam, model):
    cam, model = np.asarray(cam, np.float32), np.asarray(model, np.float32)
    if is_identity(cam):
        return model.copy()
    c, m = cam.astype(np.float64), model.astype(np.float64)
    T = np.zeros((3, 4))
    for r in range(3):
        for k in range(4):
            v = (c[r, 0] * m[0, k] + c[r, 1] * m[1, k]) + c[r, 2] * m[2, k]
            T[r, k] = v + c[r, 3] if k == 3 else v
    return T.astype(np.float32)


def compose_ref(cam, model, group):
    """cam [B,3,4], model [Gr,3,4], group [B] (clamped) -> [B,3,4] float32: cam[i] o model[group[i]]."""
    ids = np.clip(np.asarray(group, np.int64), 0, len(model) - 1)
    return np.stack([compose_one(cam[i], model[ids[i]]) for i in range(len(cam))])


# ----------------------------------------------------------------------------------------------------------------- change of variables
def adjoint_ref(cam):
    """A = [[Rc, 0], [[tc]x Rc, Rc]] fp64 from the fp32 cam [3,4]."""
    c = np.asarray(cam, np.float32).astype(np.float64)
    R, (tx, ty, tz) = c[:, :3], c[:, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = R
    A[3, :3] = (-tz) * R[1] + ty * R[2]
    A[4, :3] = tz * R[0] + (-tx) * R[2]
    A[5, :3] = (-ty) * R[0] + tx * R[1]
    return A


def transform_ref(s, cam):
    """The view's sums for a world-frame increment: H' = A^T H A (upper triangle of Q = A^T (H A), mirrored), g' = A^T g; cost, count
    and near_ties unchanged; a cam of exactly [I|0]: the sums themselves."""
    if is_identity(cam):
        return dict(s)
    A, H, g = adjoint_ref(cam), np.asarray(s["JtJ"], np.float64), np.asarray(s["Jtr"], np.float64)
    P, Q, g2 = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros(6)
    with np.errstate(all="ignore"):
        for r in range(6):
            for c in range(6):
                v = H[r, 0] * A[0, c]
                for m in range(1, 6):
                    v = v + H[r, m] * A[m, c]
                P[r, c] = v
        for r in range(6):
            for c in range(r, 6):
                v = A[0, r] * P[0, c]
                for m in range(1, 6):
                    v = v + A[m, r] * P[m, c]
                Q[r, c] = Q[c, r] = v
            v = A[0, r] * g[0]
            for m in range(1, 6):
                v = v + A[m, r] * g[m]
            g2[r] = v
    return dict(s, JtJ=Q, Jtr=g2)


EMPTY = dict(JtJ=np.zeros((6, 6)), Jtr=np.zeros(6), cost=0.0, count=0, near_ties=0)


def group_sums(views, ids, g):
    """The sums of group g: its member views' (ids == g) in ascending view index, the first assigned; no member: zeros."""
    total = None
    for i in np.flatnonzero(ids == g):
        v = views[i]
        part = {k: v[k] for k in EMPTY}
        total = part if total is None else {k: total[k] + part[k] for k in EMPTY}
    return dict(EMPTY) if total is None else total


# ----------------------------------------------------------------------------------------------------------------- one step
def step_ref(model, cam, group, K, sil=None, photo=None, icp=None, weights=WEIGHTS, damping=1e-6, evaluate_only=False):
    """The whole call: model [Gr,3,4], cam [B,3,4], group [B], K [B,3,3] and the present terms (joint_ref.step_ref's dicts, planes per
    view) -> dict(model [Gr,3,4] and pose [B,3,4] float32, inliers, status, views, near_ties [Gr], chi2 [Gr] fp64, rms [Gr] (NaN, as
    joint_ref) and per present term '<term>_inliers', '_rms', '_status' [B] (and 'sil_inter', 'sil_uni'): its evaluation at the composed
    pose)."""
    B, Gr = len(cam), len(model)
    model = np.asarray(model, np.float32)
    ids = np.clip(np.asarray(group, np.int64), 0, Gr - 1)
    pose = compose_ref(cam, model, group)
    assert any(t is not None and float(np.float32(w)) > 0 for t, w in zip((sil, photo, icp), weights))
    out = dict(model=np.zeros((Gr, 3, 4), np.float32), inliers=np.zeros(Gr, np.int64), status=np.zeros(Gr, np.int64), chi2=np.zeros(Gr),
               views=np.zeros(Gr, np.int64), near_ties=np.zeros(Gr, np.int64), rms=np.full(Gr, np.nan))
    for name, t in zip(JREF.TERMS, (sil, photo, icp)):
        if t is not None:
            out.update({name + "_inliers": np.zeros(B, np.int64), name + "_rms": np.zeros(B), name + "_status": np.zeros(B, np.int64)})
    if sil is not None:
        out.update(sil_inter=np.zeros(B, np.int64), sil_uni=np.zeros(B, np.int64))
    views = []
    for b in range(B):
        sums = JREF.term_sums(b, K, pose, sil, photo, icp)
        ties = 0
        for name, s in zip(JREF.TERMS, sums):
            if s is not None:
                _, out[name + "_inliers"][b], out[name + "_rms"][b], out[name + "_status"][b] = solve_ref(s, pose[b], damping, True)
                ties += s["near_ties"]
        if sums[0] is not None:
            out["sil_inter"][b], out["sil_uni"][b] = sums[0]["inter"], sums[0]["uni"]
        s = JREF.weighted_sums(sums, weights)
        views.append(dict(transform_ref(s, cam[b]), near_ties=ties))
    for g in range(Gr):
        s = group_sums(views, ids, g)
        out["model"][g], out["inliers"][g], _, out["status"][g] = solve_ref(s, model[g], damping, evaluate_only)
        out["chi2"][g], out["near_ties"][g] = s["cost"], s["near_ties"]
        out["views"][g] = sum(1 for i in np.flatnonzero(ids == g) if views[i]["count"] > 0)
    out["pose"] = compose_ref(cam, out["model"], group)
    return out


# ----------------------------------------------------------------------------------------------------------------- rigid helpers
def invert(P):
    P = np.asarray(P, np.float64)
    Rt = P[:, :3].T
    return np.concatenate([Rt, -(Rt @ P[:, 3:])], 1)


def times(P, Q):
    """P o Q for two [3,4] poses in fp64."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    return np.concatenate([P[:, :3] @ Q[:, :3], P[:, :3] @ Q[:, 3:] + P[:, 3:]], 1)


def rotation_deg(R):
    return float(np.degrees(np.arccos(np.clip((np.trace(np.asarray(R, np.float64)) - 1.0) / 2.0, -1.0, 1.0))))


def init_model_ref(pose, cam, group, score=None):
    """Per group the view with the highest score (ties and None: the lowest index): C^-1 o T in fp64 -> [Gr,3,4] float32."""
    group = np.asarray(group, np.int64)
    out = np.tile(IDENTITY, (int(group.max()) + 1, 1, 1))
    score = np.zeros(len(group)) if score is None else np.asarray(score, np.float64)
    for g in range(len(out)):
        members = np.flatnonzero(group == g)
        if len(members):
            i = members[int(np.argmax(score[members]))]
            out[g] = times(invert(np.asarray(cam[i], np.float32)), np.asarray(pose[i], np.float32)).astype(np.float32)
    return out


def grouped_case(c, group, Gr, seed, plain=()):
    """A multi-view case on top of a joint one-step case ``c`` (joint_ref.one_step_case: planes hand-built at c['pose']): per group a
    random model M_g 200 .. 600 mm and tens of degrees away from the camera frames, per view the camera C_i = pose_i o M_g^-1 rounded
    to fp32, so that the composed poses are c['pose'] to rounding; a view in ``plain`` that is the first of its group has the camera
    [I|0] exactly and gives its group's model.  group ids outside 0 .. Gr-1 clamp -> (model [Gr,3,4], cam [B,3,4]) float32."""
    rs = np.random.RandomState(seed)
    B = len(c["pose"])
    ids = np.clip(np.asarray(group, np.int64), 0, Gr - 1)
    model, cam = np.zeros((Gr, 3, 4), np.float32), np.zeros((B, 3, 4), np.float32)
    for g in range(Gr):
        members = np.flatnonzero(ids == g)
        q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
        q = q * np.sign(np.linalg.det(q))
        M = np.concatenate([q, rs.uniform(-1, 1, (3, 1)) * rs.uniform(200, 600)], 1)
        if len(members) and members[0] in plain:
            M = c["pose"][members[0]].astype(np.float64)
        model[g] = M.astype(np.float32)
        for i in members:
            cam[i] = IDENTITY if i == members[0] and i in plain else times(c["pose"][i], invert(model[g])).astype(np.float32)
    return model, cam


GROUPINGS = {"one group": ([0, 0, 0, 0, 0], 1), "singletons": ([0, 1, 2, 3, 4], 5), "interleaved": ([1, 0, 1, 0, 1], 2),
             "an empty group": ([0, 2, 0, 2, 2], 3)}


# ----------------------------------------------------------------------------------------------------------------- the loop
def multiview_ref(name, texture, model, cam, group, K, sdf=None, image=None, photo_mask=None, weights=WEIGHTS, tau_px=4.0, tau=0.5, iters=20,
                  damping=1e-6):
    """The loop of ops.multiview_align on the silhouette and / or the photometric term with the brute-force raster: iters + 1 passes,
    one render per view and pass at the composed pose, the model rounded to fp32 between them, the last evaluate-only -> dict(model,
    pose, inliers, chi2, views, status (of the last step taken), inliers0, chi20, near_ties (largest over the passes))."""
    H, W = np.asarray(sdf if sdf is not None else image).shape[1:3]
    model = np.asarray(model, np.float32).copy()
    first = status = got = None
    ties = np.zeros(len(model), np.int64)
    for it in range(iters + 1):
        pose = compose_ref(cam, model, group)
        r = [JREF.render_ref(name, texture, pose[b], K[b], H, W) for b in range(len(pose))]
        z, rgb = np.stack([p[0] for p in r]), np.stack([p[1] for p in r])
        got = step_ref(model, cam, group, K, sil=None if sdf is None else dict(zbuf=z, sdf=sdf, tau_px=tau_px),
                       photo=None if image is None else dict(zbuf=z, rgb=rgb, image=image, tau=tau, mask=photo_mask),
                       weights=weights, damping=damping, evaluate_only=it == iters)
        first = got if first is None else first
        status = got["status"] if it < iters or status is None else status
        ties = np.maximum(ties, got["near_ties"])
        model = got["model"]
    return dict(model=got["model"], pose=got["pose"], inliers=got["inliers"], chi2=got["chi2"], views=got["views"], status=status,
                inliers0=first["inliers"], chi20=first["chi2"], near_ties=ties)


MIN_TURN_DEG = 30.0
ROUTES = ("silhouette 10", "joint 20, w_photo 100")


@functools.lru_cache(maxsize=None)
def loop_inputs(name, kind):
    """joint_ref.table_inputs(name, kind) as ONE object seen by two cameras: cam_0 = [I|0], cam_1 = P_1 o P_0^-1, model = P_0, start =
    perturbed(P_0, RandomState(5), 8 degrees).  Where P_1 o P_0^-1 turns by less than 30 degrees the two images show almost the same
    side: view 1 is then replaced by view 0's camera turned 90 degrees about its y axis through the object's centre (P_0's translation),
    re-rendered with the brute-force raster under the same occluder pixels, noise and field rule (``replaced`` says so)."""
    import icp_ref as IREF
    import occlusion_ref as OREF
    import photo_ref as PHREF
    c = dict(JREF.table_inputs(name, kind))
    P0, P1 = c["P"][0].astype(np.float64), c["P"][1].astype(np.float64)
    rel = times(P1, invert(P0))
    replaced = rotation_deg(rel[:, :3]) < MIN_TURN_DEG
    if replaced:
        Ry = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])
        centre = P0[:, 3]
        rel = np.concatenate([Ry, (centre - Ry @ centre)[:, None]], 1)         # x_1 = Ry (x_0 - centre) + centre
        P1 = times(rel, P0)
        H, W = c["H"], c["W"]
        z, rgb = PHREF.render_ref(c["verts"], c["faces"], c["vcolor"], P1.astype(np.float32), c["K"][1], H, W, PHREF.BACKGROUND)
        whole = z > 0
        occ = OREF.occluder(whole, kind)                                          # (the same occluder rule on the new view's own mask)
        known = ~occ
        image = rgb.copy()
        image[occ] = JREF.OCCLUDER_COLOUR
        image = (image + np.random.RandomState(4).normal(0.0, PHREF.NOISE_SIGMA, (2,) + image.shape)[1]).astype(np.float32)
        cut = (whole & ~occ).astype(np.uint8)
        c["P"] = np.stack([c["P"][0], P1.astype(np.float32)])
        c["image"] = np.stack([c["image"][0], image])
        c["cut"] = np.stack([np.asarray(c["cut"][0]).astype(np.uint8), cut])
        c["field"] = np.stack([c["field"][0], OREF.sdf_known_ref(cut, known.astype(np.uint8))])
        c["occ"] = np.stack([c["occ"][0], occ])
        c["known"] = np.stack([np.asarray(c["known"][0]).astype(np.uint8), known.astype(np.uint8)])
        c["visible"] = np.array([c["visible"][0], cut.sum() / whole.sum()])
    cam = np.stack([IDENTITY, rel.astype(np.float32)])
    start = IREF.perturbed(c["P"][:1], np.random.RandomState(5), JREF.START_DEG)
    return dict(c, cam=cam, group=np.zeros(2, np.int32), model_true=c["P"][0].copy(), model_start=np.asarray(start, np.float32), replaced=replaced,
                turn_deg=rotation_deg(rel[:, :3]))


@functools.lru_cache(maxsize=None)
def loop_route(name, kind, route):
    """One route on one two-view case -> dict(status, err (deg, mm) of the model, views, near_ties, want: the loop's dict)."""
    c = loop_inputs(name, kind)
    with np.errstate(all="ignore"):
        if route == "silhouette 10":
            want = multiview_ref(name, c["texture"], c["model_start"], c["cam"], c["group"], c["K"], sdf=c["field"], iters=10)
        else:
            want = multiview_ref(name, c["texture"], c["model_start"], c["cam"], c["group"], c["K"], sdf=c["field"], image=c["image"],
                                 photo_mask=c["known"], weights=(1.0, 100.0, 0.0), iters=20)
    return dict(status=int(want["status"][0]), err=PREF.pose_error(want["model"][0], c["model_true"]), views=int(want["views"][0]),
                view_err=[PREF.pose_error(want["pose"][b], c["P"][b]) for b in range(2)], near_ties=int(want["near_ties"][0]), want=want)


def golden_arrays():
    """What tests/golden/multiview_loops.npz holds: per case and route the restatement's final model, errors and counts, and per route
    the number of groups whose two composed poses both end nearer the truth than section 23's single-view loops do."""
    out = {}
    for route in ROUTES:
        nearer = 0
        for name, kind in JREF.CASES:
            c, r = loop_inputs(name, kind), loop_route(name, kind, route)
            key = "%s|%s|%s|" % (name, kind, route)
            out.update({key + "err": np.array(r["err"]), key + "view_err": np.array(r["view_err"]), key + "model": r["want"]["model"],
                        key + "inliers": r["want"]["inliers"], key + "inliers0": r["want"]["inliers0"], key + "chi2": r["want"]["chi2"],
                        key + "views": r["want"]["views"], key + "near_ties": r["want"]["near_ties"], key + "status": r["want"]["status"]})
            single = JREF.table_route(name, kind, route)["err"]
            nearer += all(r["view_err"][b][0] < single[b][0] and r["view_err"][b][1] < single[b][1] for b in range(2) if b == 0 or not c["replaced"])
        out["nearer|" + route] = np.int64(nearer)
    return out
