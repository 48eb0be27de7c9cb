"""The occlusion contract of DESIGN section 22 (kernels K31c tp_mask_sdf_known and K32 tp_mask_known_from_others, and the visible IoU
of ops.silhouette_align), said again in numpy -- written from the rules in include/texpose_amd.h, not from the kernels.  Where the
kernels are free to choose, this file chooses differently: the field is brute force over all pixel pairs on the SET and the CLEAR
selections (the kernels sweep columns, then rows, and know an unknown pixel by its two column distances), "another instance is near"
is a whole-array expression over all N x N pairs of planes (the kernel counts once per pixel), and the visible IoU is taken from
the masks (the wrapper takes it from the field's NaNs and K31b's counts).  The loop is tests/silhouette_ref.py's, unchanged: K31b
needs nothing new for a field with NaNs.

The occluders of the table are defined on the bounding box [r0..r1] x [c0..c1] of the full mask."""
import functools

import numpy as np

import pnp_ref as PREF
import silhouette_ref as REF


# ----------------------------------------------------------------------------------------------------------------- K31c
def _d2_to(sel):
    """sel [H,W] bool -> [H,W] int64: the squared distance of every pixel to the nearest selected pixel, H^2 + W^2 where there is
    none; brute force over all pairs (silhouette_ref.d2_ref's approach, on one selection)."""
    H, W = sel.shape
    ii, jj = np.mgrid[0:H, 0:W]
    pi, pj = ii.reshape(-1).astype(np.int32), jj.reshape(-1).astype(np.int32)
    qi, qj = pi[sel.reshape(-1)], pj[sel.reshape(-1)]
    best = np.full(H * W, H * H + W * W, np.int64)
    if len(qi):
        chunk = max(1, 4000000 // len(qi))
        for s in range(0, H * W, chunk):
            best[s:s + chunk] = ((pi[s:s + chunk, None] - qi[None, :]) ** 2 + (pj[s:s + chunk, None] - qj[None, :]) ** 2).min(1)
    return best.reshape(H, W)


def d2_known_ref(mask, known):
    """One plane: (d2_set, d2_clear) [H,W] int64 over the SET (mask and known) and the CLEAR (not mask, and known) pixels only."""
    m, k = np.asarray(mask) != 0, np.asarray(known) != 0
    return _d2_to(m & k), _d2_to(~m & k)


def field_from_d2(mask, known, to_set, to_clear):
    """One plane and its two integers -> sdf [H,W] float32: -(sqrtf(d2_clear) - 0.5) on a SET pixel, sqrtf(d2_set) - 0.5 on a CLEAR
    one, in fp32 arithmetic, NaN on an UNKNOWN one."""
    half = np.float32(0.5)
    field = np.where(np.asarray(mask) != 0, -(np.sqrt(to_clear.astype(np.float32)) - half), np.sqrt(to_set.astype(np.float32)) - half)
    return np.where(np.asarray(known) != 0, field, np.float32(np.nan)).astype(np.float32)


def sdf_known_ref(mask, known):
    """mask, known [F,H,W] or [H,W] -> sdf float32 of the same shape (field_from_d2 of d2_known_ref, plane by plane)."""
    m, k = np.asarray(mask), np.asarray(known)
    assert m.shape == k.shape
    mp, kp = (m[None], k[None]) if m.ndim == 2 else (m, k)
    out = np.empty(mp.shape, np.float32)
    for f in range(len(mp)):
        out[f] = field_from_d2(mp[f], kp[f], *d2_known_ref(mp[f], kp[f]))
    return out.reshape(m.shape)


# ----------------------------------------------------------------------------------------------------------------- K32
def known_from_others_ref(sdf, band_px):
    """sdf [N,H,W] float32 -> known [N,H,W] uint8: 0 iff some m != n has sdf[m] <= band_px - 0.5 (fp32; NaN is not near).  All N x N
    pairs of planes at once, on purpose."""
    sdf = np.asarray(sdf, np.float32)
    N = len(sdf)
    with np.errstate(invalid="ignore"):
        near = sdf <= np.float32(band_px) - np.float32(0.5)                                     # [N,H,W]
    other = ~np.eye(N, dtype=bool)                                                             # [n,m]: m is another instance
    hidden = (near[None, :, :, :] & other[:, :, None, None]).any(1)                            # [n,H,W]
    return (~hidden).astype(np.uint8)


# ----------------------------------------------------------------------------------------------------------------- the visible IoU
def visible_iou_ref(zbuf, mask, known):
    """One image: the IoU of the rendering's coverage and the measured mask over the KNOWN pixels only, as the fp32 quotient of the
    two integer counts (NaN where the denominator is 0) -> (iou float32, inter, left)."""
    cov, m, k = REF.covered(np.asarray(zbuf, np.float32)), np.asarray(mask) != 0, np.asarray(known) != 0
    inter, left = int((cov & m & k).sum()), int(((cov | m) & k).sum())
    return (np.float32(inter) / np.float32(left) if left else np.float32(np.nan)), inter, left


# ----------------------------------------------------------------------------------------------------------------- the occluders
OCCLUDERS = ("bottom third", "corner disc", "right half")
ASSERTED = ("bottom third", "corner disc")                       # with "right half" less than about half is visible: printed only


def occluder(full, kind):
    """full [H,W] (the whole object's mask) -> occ [H,W] bool."""
    full = np.asarray(full) != 0
    rows, cols = np.nonzero(full.any(1))[0], np.nonzero(full.any(0))[0]
    r0, r1, c0, c1 = int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])
    ii, jj = np.mgrid[0:full.shape[0], 0:full.shape[1]]
    if kind == "right half":
        return jj >= (c0 + c1 + 1) // 2
    if kind == "bottom third":
        return ii >= r0 + (r1 - r0) * 2 // 3
    assert kind == "corner disc"
    return (ii - r1) ** 2 + (jj - c1) ** 2 <= (0.45 * (c1 - c0)) ** 2


@functools.lru_cache(maxsize=None)
def occluded_inputs(name, kind, band_px=0.0):
    """silhouette_ref.loop_inputs(name) with its two masks cut by occluder ``kind``: occ [2,H,W] bool, cut = full & ~occ (what
    mask_visib holds), known = ~occ, or with ``band_px`` > 0 the pixels further than band_px from the occluder (the field of occ
    thresholded, as K32 does), visible: the share of the object's pixels that are left."""
    c = REF.loop_inputs(name)
    occ = np.stack([occluder(m, kind) for m in c["mask"]])
    cut = (c["mask"] != 0) & ~occ
    known = ~occ if band_px == 0 else ~(REF.sdf_ref(occ.astype(np.uint8)) <= np.float32(band_px) - np.float32(0.5))
    return dict(c, kind=kind, occ=occ, cut=cut.astype(np.uint8), known=known.astype(np.uint8),
                visible=cut.reshape(2, -1).sum(1) / (c["mask"] != 0).reshape(2, -1).sum(1))


def _summary(c, want):
    """The table's columns of one loop: per image rms, visible IoU, rotation and translation error at both ends."""
    rows = []
    for b in range(2):
        z0 = REF.render_ref(c["name"], c["start"][b], c["K"][b], c["H"], c["W"])
        z1 = REF.render_ref(c["name"], want["pose"][b], c["K"][b], c["H"], c["W"])
        re0, te0 = PREF.pose_error(c["start"][b], c["P"][b])
        re, te = PREF.pose_error(want["pose"][b], c["P"][b])
        rows.append(dict(status=int(want["status"][b]), rms0=float(want["rms0"][b]), rms=float(want["rms"][b]),
                         viou0=float(visible_iou_ref(z0, c["cut"][b], c["known"][b])[0]), viou=float(visible_iou_ref(z1, c["cut"][b], c["known"][b])[0]),
                         re0=re0, te0=te0, re=re, te=te))
    return rows


@functools.lru_cache(maxsize=None)
def occluded_case(name, kind, band_px=0.0):
    """The restatement's loop (ten steps, tau 4 px, damping 1e-6, from loop_inputs' start) against the cut masks of occluded_inputs,
    once with today's field of the cut mask ('naive') and once with the field that knows what is unknown ('known'); run once per
    case and shared by the test files."""
    c = occluded_inputs(name, kind, band_px)
    out = dict(c)
    for field, sdf in (("naive", REF.sdf_ref(c["cut"])), ("known", sdf_known_ref(c["cut"], c["known"]))):
        with np.errstate(all="ignore"):
            want = REF.silhouette_ref(name, c["start"], c["K"], sdf, 4.0, 10, 1e-6)
        out[field] = dict(sdf=sdf, want=want, rows=_summary(c, want))
    return out


def table_line(case, b):
    n, k = case["naive"]["rows"][b], case["known"]["rows"][b]
    return ("%s %d, %s (%.2f) | rms %.3f -> %.3f / %.3f -> %.3f | visible IoU %.3f -> %.3f / %.3f -> %.3f | %.2f deg -> %.2f / %.2f | %.2f mm -> %.3g / %.3g"
            " | status %d / %d" % (case["name"], b, case["kind"], case["visible"][b], n["rms0"], n["rms"], k["rms0"], k["rms"], n["viou0"], n["viou"],
                                   k["viou0"], k["viou"], n["re0"], n["re"], k["re"], n["te0"], n["te"], k["te"], n["status"], k["status"]))
