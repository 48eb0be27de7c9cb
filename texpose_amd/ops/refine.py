"""K29-K33: the render-and-compare pose refiners -- the depth ICP, the photometric alignment, the masks' distance field, the silhouette
alignment and the joint step of the three -- behind one table of terms: what a term's step takes, asks of the rasteriser and returns
is said once in ``_TERMS``; one builder fills any term's args struct, one helper sizes every workspace and one driver runs all four
loops.  K37, the exposure fit that a loop with a photometric term may run in front of each step (photo_exposure), its sibling K40 for
a light with a direction (photo_lighting), and K38, the image pyramid of the photometric loop (image_down, surface_down, mask_down),
are here too."""
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from .. import _lib
from ._base import Tensor, _call, _f32, _intr_per_view, _lengths, _on_tensor_device, _outputs, _points, _poses, _ptr, _want_gpu, _workspace_arg

__all__ = ["depth_icp_workspace", "depth_icp_step", "DEPTH_ICP_KEYS", "depth_icp", "photo_align_workspace", "photo_align_step", "PHOTO_ALIGN_KEYS",
           "photo_align", "photo_exposure_workspace", "photo_exposure", "PHOTO_EXPOSURE_KEYS", "photo_lighting_workspace", "photo_lighting",
           "PHOTO_LIGHTING_KEYS", "image_down", "surface_down", "mask_down",
           "image_pyramid", "mask_pyramid", "mask_sdf_workspace", "mask_sdf",
           "mask_known_from_others", "silhouette_align_workspace", "silhouette_align_step", "SILHOUETTE_ALIGN_KEYS", "silhouette_align",
           "JOINT_TERMS", "JOINT_WEIGHTS", "_joint_weights", "joint_align_workspace", "joint_align_step", "JOINT_ALIGN_KEYS", "joint_align",
           "pose_compose", "multiview_group_index", "multiview_align_workspace", "multiview_align_step", "MULTIVIEW_ALIGN_KEYS", "multiview_align"]


# ------------------------------------------------------------------------------------------ the terms
@dataclass(frozen=True)
class _Term:
    """One residual term of the refiners, as its step (tp_<...>_step) and the layers above see it."""
    name: str                    # as joint_align_step's keyword and in masks=
    prefix: str                  # of its keys in the joint results (and, less the '_', of its weight in tp_joint_align_args)
    args: type                   # the step's args struct
    workspace_bytes: str         # the library's size query (B, H, W)
    rendered: tuple              # the inputs before ``pose``: the mesh and mesh_raster's planes at the pose
    plane: str                   # the measured planes [Ft,H,W] + trailing ...
    trailing: tuple
    word: str                    # ... and what the messages call them
    threshold: str               # its threshold's name
    counts: tuple = ()           # int32 [B] outputs beyond inliers / rms / status
    colour: bool = False         # asks mesh_raster for rgb
    face_ids: bool = False       # asks mesh_raster for the face index


_TERMS = (_Term("silhouette", "sil_", _lib.SilhouetteAlignArgs, "tp_silhouette_align_workspace_bytes", ("zbuf",), "sdf", (), "planes", "tau_px",
                counts=("inter", "uni")),
          _Term("photo", "photo_", _lib.PhotoAlignArgs, "tp_photo_align_workspace_bytes", ("zbuf", "rgb"), "image", (3,), "photographs", "tau", colour=True),
          _Term("depth", "icp_", _lib.DepthIcpArgs, "tp_depth_icp_workspace_bytes", ("verts", "faces", "zbuf", "face"), "depth", (), "planes", "tau_mm",
                face_ids=True))
_SILHOUETTE, _PHOTO, _DEPTH = _TERMS
JOINT_TERMS = tuple(t.name for t in _TERMS)              # the order of the weights and of the sum


def _term_bytes(terms, B: int, H: int, W: int, align: int = 1) -> list:
    """Each term's ``*_workspace_bytes`` at B images of H x W, rounded up to ``align``."""
    lib = _lib.load()
    return [(int(getattr(lib, t.workspace_bytes)(B, H, W)) + align - 1) // align * align for t in terms]


def _new_workspace(op: str, terms, B: int, H: int, W: int, device, lighting: bool = False, tail_bytes: int = 0, align: int = 1) -> Tensor:
    """``lighting``: for a loop with lighting=True, whose fit (K40) runs in the same bytes and may need more than the terms."""
    need = sum(_term_bytes(terms, B, H, W, align)) + tail_bytes
    if lighting:
        need = max(need, int(_lib.load().tp_photo_lighting_workspace_bytes(B, H, W)))
    return _workspace_arg(op, None, need, device)


def _frame_planes(op: str, term: _Term, planes: Tensor, frame: Optional[Tensor], mask: Optional[Tensor], B: int, H: int, W: int, like: Tensor):
    """The measured planes of ``term`` [Ft,H,W] + trailing (one plane: Ft = 1), the frame map and the mask [Ft,H,W] of a step ->
    (planes, frame, mask, Ft)."""
    name, trailing = term.plane, term.trailing
    planes = _f32(planes.detach(), name)
    if planes.dim() == 2 + len(trailing):
        planes = planes[None]
    if planes.dim() != 3 + len(trailing) or tuple(planes.shape[1:]) != (H, W) + trailing or planes.shape[0] == 0:
        layout = "[Ft,H=%d,W=%d,3] (channels last)" % (H, W) if trailing else "[Ft,H=%d,W=%d]" % (H, W)
        raise ValueError("%s: %s %s expected, got %s" % (op, name, layout, tuple(planes.shape)))
    Ft = planes.shape[0]
    frame = _lengths(op, frame, "frame", B, like)
    if frame is None and Ft not in (1, B):
        raise ValueError("%s: %s must hold 1 or B = %d %s without frame=, got %d" % (op, name, B, term.word, Ft))
    if mask is not None:
        if torch.is_tensor(mask) and mask.dtype == torch.bool:
            mask = mask.view(torch.uint8) if mask.is_contiguous() else mask.to(torch.uint8)
        if torch.is_tensor(mask) and mask.dim() == 2:
            mask = mask[None]
        mask = _want_gpu(op, mask, "mask", torch.uint8, (Ft, H, W))
    return planes, frame, mask, Ft


def _term_args(term: _Term, op: str, tensors: dict, *, threshold, damping=1e-6, frame=None, mask=None, evaluate_only=False, workspace=None, out=None,
               with_pose=True):
    """The arguments of ``term``'s step, checked: ``tensors`` holds its rendered inputs, ``pose``, ``intr`` and its measured planes by
    name -> (the filled args struct, its outputs, the tensors it points into).  Without ``with_pose`` (a term of the joint step, which
    writes no pose of its own) there is no 'pose' among the outputs and pose_out is null."""
    t = dict(tensors)
    if "verts" in t:
        t["verts"] = _points(op, t["verts"], "verts")
    pose = t["pose"] = _poses(op, t["pose"], "pose")
    B = pose.shape[0]
    if "faces" in t:
        faces = _want_gpu(op, t["faces"], "faces", torch.int32, None)
        if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
            raise ValueError("%s: faces [F,3] expected, got %s" % (op, tuple(faces.shape)))
    zbuf = _want_gpu(op, t["zbuf"], "zbuf", torch.float32, None)
    if zbuf.dim() != 3 or zbuf.shape[0] != B or zbuf.numel() == 0:
        raise ValueError("%s: zbuf [B=%d,H,W] expected, got %s" % (op, B, tuple(zbuf.shape)))
    H, W = zbuf.shape[1:]
    if "face" in t:
        _want_gpu(op, t["face"], "face", torch.int32, (B, H, W))
    if "rgb" in t:
        _want_gpu(op, t["rgb"], "rgb", torch.float32, (B, H, W, 3))
    t["intr"] = _intr_per_view(op, t["intr"], B)
    t[term.plane], frame, mask, Ft = _frame_planes(op, term, t[term.plane], frame, mask, B, H, W, zbuf)
    spec = {"pose": (torch.float32, (B, 3, 4)), "inliers": (torch.int32, (B,)), "rms": (torch.float32, (B,)), "status": (torch.int32, (B,))}
    spec.update({k: (torch.int32, (B,)) for k in term.counts})
    if not with_pose:
        del spec["pose"]
    res = _outputs(op, out, spec, zbuf.device, partial=True)
    workspace = _workspace_arg(op, workspace, _term_bytes((term,), B, H, W)[0], zbuf.device, align=16)
    a = term.args()
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    for k, v in res.items():
        setattr(a, "pose_out" if k == "pose" else k, v.data_ptr())          # (pose_out stays null without with_pose)
    a.frame, a.mask, a.workspace = _ptr(frame), _ptr(mask), workspace.data_ptr()
    a.B, a.Ft, a.H, a.W = B, Ft, H, W
    if "verts" in t:
        a.V, a.F = t["verts"].shape[0], t["faces"].shape[0]
    setattr(a, term.threshold, float(threshold))
    a.damping, a.evaluate_only = float(damping), int(bool(evaluate_only))
    return a, res, (workspace, frame, mask) + tuple(t.values())             # (the struct holds addresses only)


# ------------------------------------------------------------------------------------------ the loops
def _tau_schedule(op: str, tau, tau_name: str, iters: int):
    """A loop's thresholds, checked before anything else of the call: one value or ``iters`` + 1 host values -> iters + 1 floats."""
    iters = int(iters)
    if iters < 0:
        raise ValueError("%s: iters >= 0 expected, got %d" % (op, iters))
    taus = [float(tau)] * (iters + 1) if isinstance(tau, (int, float)) else [float(t) for t in tau]
    if len(taus) != iters + 1:
        raise ValueError("%s: %s must be one value or iters + 1 = %d values, got %d" % (op, tau_name, iters + 1, len(taus)))
    return taus


def _schedules(op: str, given, iters: int) -> list:
    """The thresholds of a loop over ``given`` = [(term, measured planes or None, threshold(s), mask)], absent terms' too -> per pass one
    value per entry of ``given``."""
    return list(zip(*[_tau_schedule(op, th, term.threshold, iters) for term, _, th, _ in given]))


def _refine(op: str, keys: tuple, verts: Tensor, faces: Tensor, pose: Tensor, intr: Tensor, given, taus, *, damping, frame, workspace, cull,
            vcolor=None, texels=None, visible_iou=False, weights=None, exposure=False, exposure_tau0=2.0, pyramid=None, multiview=None, lighting=False) -> Dict[str, Tensor]:
    """The loop of every refiner over the terms of ``given`` that have planes: one pass per entry of ``taus`` (_schedules) of ONE
    mesh_raster call at the current poses, asked only for what these terms need, and one step from it, the last evaluate-only; a step
    that fails passes its pose on.  Without ``weights`` the step is the single term's own (its 'rms' is the cost carried); with them it
    is joint_align_step ('chi2'), and the last pass's per-term keys are returned too.  -> ``keys``: the last pass's pose, inliers and
    cost, the status of the last step taken (of the evaluation where there is no step), inliers0 / <cost>0 of the first pass; with a
    term that counts coverage 'iou' / 'iou0', and with ``visible_iou`` 'iou_visible' / 'iou0_visible'.  ``exposure`` with a photometric
    term: every pass first fits the photograph's per-channel gain and bias to the rendering and rewrites the rendered colours under
    them (photo_exposure in place, K37; the term's frame map and mask; the fit of the pass before decides with that pass's ``tau``
    what is kept, the first pass keeps within ``exposure_tau0`` of the plain colours) -> also 'gain' / 'bias' [B,3] and
    'exposure_status' [B] of the last pass (prefixed with the term's 'photo_' in the joint results).  ``pyramid`` (the photometric
    term alone): steps per level, the coarsest first, adding up to the steps of ``taus``; the photograph's and the mask's pyramids are
    built once, a pass at level l filters the full-size rendering down l times (surface_down, K38) and steps on the level's planes
    with the level's intrinsics; the last pass, the evaluation, runs at level 0.  ``multiview`` (K39, with ``weights``): dict(cam [B,3,4],
    group [B], index) -- ``pose`` is then the MODEL [Gr,3,4], the state the loop carries: every pass composes the B views' poses from it
    (pose_compose), renders at those and takes multiview_align_step in place of the joint step -> also 'model' and 'views'.
    ``lighting`` with a photometric term, in place of ``exposure`` (its model contains K37's; both: ValueError): every pass also asks
    the rasteriser for the face index and first fits ambient + directional shading and a bias per image and channel on the faces' own
    normals (photo_lighting in place, K40; kept within that pass's ``tau`` of the light before, the first pass within
    ``exposure_tau0`` of the plain colours) -> also 'light' [B,3,5], 'lighting_status' and 'lighting_flags' [B] of the last pass
    (prefixed as above).  With ``pyramid`` the fit and the apply run on the FULL-SIZE rendering against the full-size photograph and
    mask, before surface_down: normals need no pyramid, and the lit rendering is filtered as the photograph was.  The workspace must
    then also hold tp_photo_lighting_workspace_bytes."""
    if exposure and lighting:                                    # (a host argument: refused before anything touches the device)
        raise ValueError("%s: exposure= and lighting= exclude each other (the lighting model contains the exposure's)" % op)
    joint = weights is not None
    cost = "chi2" if joint else "rms"
    verts, pose = _points(op, verts, "verts"), _poses(op, pose, "pose" if multiview is None else "model")
    B = pose.shape[0] if multiview is None else multiview["cam"].shape[0]
    faces = faces.to(device=verts.device, dtype=torch.int32).contiguous()
    intr = _intr_per_view(op, intr, B)
    terms, planes, masks = [], {}, {}
    for i, (term, p, _, m) in enumerate(given):
        if p is None:
            continue
        p = _f32(p.detach(), term.plane)
        p = p[None] if p.dim() == 2 + len(term.trailing) else p
        if p.dim() != 3 + len(term.trailing) or p.numel() == 0 or tuple(p.shape[3:]) != term.trailing:
            raise ValueError("%s: %s [Ft,H,W%s]%s expected, got %s" % (op, term.plane, ",3" if term.trailing else "",
                                                                        "" if joint or not term.trailing else " (channels last)", tuple(p.shape)))
        terms.append((i, term))
        planes[term.plane], masks[term.name] = p, m
    sizes = {tuple(p.shape[1:3]) for p in planes.values()}
    if len(sizes) != 1:
        raise ValueError("%s: the measured planes must be of one size H x W, got %s" % (op, {k: tuple(v.shape) for k, v in planes.items()}))
    H, W = sizes.pop()
    for _, term in terms:
        planes[term.plane], frame, masks[term.name], _ = _frame_planes(op, term, planes[term.plane], frame, masks[term.name], B, H, W, pose)
    vcolor = None if vcolor is None else _f32(vcolor.detach(), "vcolor")
    texels = None if texels is None else _f32(texels.detach(), "texels")
    own_bytes = 0 if multiview is None else int(_lib.load().tp_multiview_workspace_bytes(B))
    need = sum(_term_bytes([t for _, t in terms], B, H, W, 16 if joint else 1)) + own_bytes
    relit = bool(lighting) and any(t is _PHOTO for _, t in terms)
    if relit:                                                    # (the fit's records are twice a term's: it runs before the step, in the same bytes)
        need = max(need, int(_lib.load().tp_photo_lighting_workspace_bytes(B, H, W)))
    workspace = _workspace_arg(op, workspace, need, pose.device, align=16)
    counting = next((t for _, t in terms if t.counts), None)
    if visible_iou:
        if counting is None:
            raise ValueError("%s: visible_iou needs %s=" % (op, next(t.plane for t in _TERMS if t.counts)))
        unknown = torch.isnan(planes[counting.plane])            # [Ft,H,W]; the plane of image b by the step's frame rule
        if frame is not None:
            unknown = unknown[frame.clamp(0, unknown.shape[0] - 1).long()]
    colour = any(t.colour for _, t in terms)
    ask = dict(H=H, W=W, vcolor=vcolor if colour else None, texels=texels if colour else None, face_ids=relit or any(t.face_ids for _, t in terms),
               normals=False, cull=cull)
    from .scene import mesh_raster                               # (looked up per call: tests and tools replace ops.scene.mesh_raster)
    mesh = dict(verts=verts, faces=faces)
    fixed = [(i, term, dict({k: mesh[k] for k in term.rendered if k in mesh}, **{term.plane: planes[term.plane]}, frame=frame, mask=masks[term.name]),
              [k for k in term.rendered if k not in mesh]) for i, term in terms]
    step = _STEPS[terms[0][1].name]
    hidden = []
    levels, coarse = [0] * len(taus), {}
    if pyramid is not None:
        if joint or [t for _, t in terms] != [_PHOTO]:
            raise ValueError("%s: pyramid= goes with the photometric term alone" % op)
        levels = _pass_levels(op, pyramid, len(taus) - 1)
        photos = image_pyramid(planes[_PHOTO.plane], max(levels) + 1)
        known = [None] * len(photos) if masks[_PHOTO.name] is None else mask_pyramid(masks[_PHOTO.name], len(photos))
        for l in range(1, len(photos)):                          # (level l's intrinsics: rows 0 and 1 times 2^-l, exact)
            scaled = intr.clone()
            scaled[:, :2] *= 0.5 ** l
            coarse[l] = (photos[l], known[l], scaled)
    photo_at = next((i for i, t in terms if t is _PHOTO), None)  # the photometric threshold's place in a pass's ``th``
    lit = photo_at if exposure else None
    fit = {}                                                     # the exposure (or lighting) fit of the pass before

    def one_pass(pose, th, last, level):                         # (a function: the rendered planes are released before the next pass renders)
        if multiview is not None:                                # (the state is the model; the views' poses follow from it)
            model, pose = pose, pose_compose(multiview["cam"], pose, multiview["group"])
        r = mesh_raster(verts, faces, pose, intr, **ask)
        photo, photo_mask, K = coarse[level] if level else (planes.get(_PHOTO.plane), masks.get(_PHOTO.name), intr)
        if relit:                                                # (on the full-size rendering, whatever the level: in front of surface_down)
            e = photo_lighting(verts, faces, r["face"], r["zbuf"], r["rgb"], pose, planes[_PHOTO.plane], tau=th[photo_at] if fit else exposure_tau0,
                               light=fit.get("light"), frame=frame, mask=masks[_PHOTO.name], inplace=True, workspace=workspace)
            fit.update(light=e["light"], lighting_status=e["status"], lighting_flags=e["flags"])
        for _ in range(level):                                   # (the full-size rendering filtered as the photograph was, never a coarse raster)
            r = surface_down(r["zbuf"], r["rgb"])
        if lit is not None:                                      # (in front of the step: it compares the colours under the photograph's exposure)
            e = photo_exposure(r["zbuf"], r["rgb"], photo, tau=th[lit] if fit else exposure_tau0, gain=fit.get("gain"),
                               bias=fit.get("bias"), frame=frame, mask=photo_mask, inplace=True, workspace=workspace)
            fit.update(gain=e["gain"], bias=e["bias"], exposure_status=e["status"])
        own = {term.name: dict(kw, **{k: r[k] for k in rendered}, **{term.threshold: th[i]}) for i, term, kw, rendered in fixed}
        if multiview is not None:
            got = multiview_align_step(model, multiview["cam"], multiview["group"], intr, weights=weights, damping=damping, evaluate_only=last,
                                       workspace=workspace, pose=pose, index=multiview["index"], **own)
        elif joint:
            got = joint_align_step(pose, intr, weights=weights, damping=damping, evaluate_only=last, workspace=workspace, **own)
        else:
            if level:
                own[_PHOTO.name].update({_PHOTO.plane: photo, "mask": photo_mask})
            got = step(pose=pose, intr=K, damping=damping, evaluate_only=last, workspace=workspace, **own[terms[0][1].name])
        if visible_iou and (not hidden or last):                 # (the first and the last rendering)
            z = r["zbuf"]
            hidden.append(((z > 0) & torch.isfinite(z) & unknown).flatten(1).sum(1))
        return got

    first = status = None
    for it, th in enumerate(taus):
        last = it == len(taus) - 1
        got = one_pass(pose, th, last, levels[it])
        first = got if first is None else first
        status = got["status"] if not last or status is None else status
        pose = got["pose" if multiview is None else "model"]
    res = {"pose": got["pose"], "inliers": got["inliers"], cost: got[cost], "status": status, "inliers0": first["inliers"], cost + "0": first[cost]}
    if multiview is not None:
        res.update(model=got["model"], views=got["views"])
    res = {k: res[k] for k in keys}
    if joint:
        res.update({k: v for k, v in got.items() if k.startswith(tuple(t.prefix for t in _TERMS))})
    res.update({(_PHOTO.prefix if joint else "") + k: v for k, v in fit.items()})
    if counting is not None:
        inter, uni = ((counting.prefix if joint else "") + k for k in counting.counts)
        res.update(iou=got[inter].float() / got[uni].float(), iou0=first[inter].float() / first[uni].float())
        if visible_iou:
            def seen(r, h):
                left = r[uni] - h                                # (>= inter: a hidden pixel is covered and not inside)
                return torch.where(left == 0, torch.full_like(left, float("nan"), dtype=torch.float32), r[inter].float() / left.float())
            res.update(iou_visible=seen(got, hidden[-1]), iou0_visible=seen(first, hidden[0]))
    return res


# ------------------------------------------------------------------------------------------ K29
def depth_icp_workspace(B: int, H: int, W: int, device) -> Tensor:
    """A workspace for depth_icp_step / depth_icp at B images of H x W (tp_depth_icp_workspace_bytes); needs no clearing."""
    return _new_workspace("depth_icp", (_DEPTH,), B, H, W, device)


@_on_tensor_device
def depth_icp_step(verts: Tensor, faces: Tensor, zbuf: Tensor, face: Tensor, pose: Tensor, intr: Tensor, depth: Tensor, *, tau_mm: float,
                   damping: float = 1e-6, frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, evaluate_only: bool = False,
                   workspace: Optional[Tensor] = None, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """One step of projective point-to-plane ICP for B poses (tp_depth_icp_step; the rules are in the header): verts [V,3], faces [F,3]
    int32, zbuf / face [B,H,W] (mesh_raster's planes of the mesh at ``pose``; taken as they are), pose [B,3,4], intr [B,3,3] or one
    [3,3], depth [Ft,H,W] (the measured depth in mm; <= 0, NaN, Inf: no value; Ft 1 or B, or any Ft with ``frame`` [B] int32), mask
    [Ft,H,W] uint8 or bool (0: skip the pixel) -> 'pose' [B,3,4] (the stepped pose; ``pose`` itself, bit for bit, with
    ``evaluate_only`` or a non-zero status), 'inliers' [B] int32 and 'rms' [B] (mm) of ``pose`` over the pixels within tau_mm along
    the ray, 'status' [B] int32 (0 ok, 1 fewer than 6 kept pixels, 3 not positive definite).  ``workspace``:
    depth_icp_workspace(B, H, W); ``out``: any of the four tensors to write into (out['pose'] must not be ``pose``).  Two launches, no
    atomics, bit-identical from run to run, safe under torch.cuda.graph."""
    a, res, _alive = _term_args(_DEPTH, "depth_icp_step", dict(verts=verts, faces=faces, zbuf=zbuf, face=face, pose=pose, intr=intr, depth=depth),
                                threshold=tau_mm, damping=damping, frame=frame, mask=mask, evaluate_only=evaluate_only, workspace=workspace, out=out)
    _call("tp_depth_icp_step", a)         # (tau_mm, damping out of range, out['pose'] overlapping pose: the library's error)
    return res


DEPTH_ICP_KEYS = ("pose", "inliers", "rms", "status", "inliers0", "rms0")


@_on_tensor_device
def depth_icp(verts: Tensor, faces: Tensor, pose: Tensor, intr: Tensor, depth: Tensor, *, tau_mm=20.0, iters: int = 5, damping: float = 1e-6,
              frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, workspace: Optional[Tensor] = None,
              cull: bool = False) -> Dict[str, Tensor]:
    """Refine B poses of one mesh against measured depth (the rules are in the header, K29): ``iters`` + 1 passes of mesh_raster at the
    current poses (depth and face index, H x W = depth's) followed by depth_icp_step, the last with evaluate_only.  ``tau_mm``: one
    value, or ``iters`` + 1 host values for a coarse-to-fine schedule (the last is the final evaluation's).  -> 'pose' [B,3,4], its
    'inliers' [B] int32 and 'rms' [B] (mm), 'status' [B] int32 of the last step taken (of the evaluation where iters = 0) and
    'inliers0' / 'rms0' of the start pose.  A step that fails passes its pose on.  2 (iters + 1) launches besides the rasteriser's,
    bit-identical from run to run, safe under torch.cuda.graph.  ``cull``: the passes render with mesh_raster(cull=True), same bits."""
    op, given = "depth_icp", [(_DEPTH, depth, tau_mm, mask)]
    return _refine(op, DEPTH_ICP_KEYS, verts, faces, pose, intr, given, _schedules(op, given, iters), damping=damping, frame=frame,
                   workspace=workspace, cull=cull)


# ------------------------------------------------------------------------------------------ K30
def photo_align_workspace(B: int, H: int, W: int, device, lighting: bool = False) -> Tensor:
    """A workspace for photo_align_step / photo_align at B images of H x W (tp_photo_align_workspace_bytes); needs no clearing.
    ``lighting``: for photo_align(lighting=True), whose fit needs tp_photo_lighting_workspace_bytes."""
    return _new_workspace("photo_align", (_PHOTO,), B, H, W, device, lighting)


@_on_tensor_device
def photo_align_step(zbuf: Tensor, rgb: Tensor, pose: Tensor, intr: Tensor, image: Tensor, *, tau: float, damping: float = 1e-6,
                     frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, evaluate_only: bool = False,
                     workspace: Optional[Tensor] = None, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """One step of photometric alignment for B poses (tp_photo_align_step; the rules are in the header): zbuf [B,H,W] / rgb [B,H,W,3]
    (mesh_raster's planes of the vertex-coloured mesh at ``pose``; taken as they are), pose [B,3,4], intr [B,3,3] or one [3,3], image
    [Ft,H,W,3] (the photograph, channels last, in rgb's units; Ft 1 or B, or any Ft with ``frame`` [B] int32), mask [Ft,H,W] uint8 or
    bool (0: skip the pixel) -> 'pose' [B,3,4] (the stepped pose; ``pose`` itself, bit for bit, with ``evaluate_only`` or a non-zero
    status), 'inliers' [B] int32 and 'rms' [B] (colour units) of ``pose`` over the interior covered pixels whose colours differ by at
    most ``tau``, 'status' [B] int32 (0 ok, 1 fewer than 6 kept pixels, 3 not positive definite).  ``workspace``:
    photo_align_workspace(B, H, W); ``out``: any of the four tensors to write into (out['pose'] must not be ``pose``).  Two launches,
    no atomics, bit-identical from run to run, safe under torch.cuda.graph."""
    a, res, _alive = _term_args(_PHOTO, "photo_align_step", dict(zbuf=zbuf, rgb=rgb, pose=pose, intr=intr, image=image), threshold=tau, damping=damping,
                                frame=frame, mask=mask, evaluate_only=evaluate_only, workspace=workspace, out=out)
    _call("tp_photo_align_step", a)       # (tau, damping out of range, out['pose'] overlapping pose: the library's error)
    return res


PHOTO_ALIGN_KEYS = ("pose", "inliers", "rms", "status", "inliers0", "rms0")


@_on_tensor_device
def photo_align(verts: Tensor, faces: Tensor, vcolor: Tensor, pose: Tensor, intr: Tensor, image: Tensor, *, tau=0.5, iters: int = 10,
                damping: float = 1e-6, frame: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                workspace: Optional[Tensor] = None, cull: bool = False, texels: Optional[Tensor] = None, exposure: bool = False,
                exposure_tau0: float = 2.0, pyramid=None, lighting: bool = False) -> Dict[str, Tensor]:
    """Refine B poses of one vertex-coloured mesh against a photograph (the rules are in the header, K30): ``iters`` + 1 passes of
    mesh_raster at the current poses (depth and colour, H x W = image's) followed by photo_align_step, the last with evaluate_only.
    ``tau``: one value, or ``iters`` + 1 host values for a coarse-to-fine schedule (the last is the final evaluation's).  -> 'pose'
    [B,3,4], its 'inliers' [B] int32 and 'rms' [B] (colour units), 'status' [B] int32 of the last step taken (of the evaluation where
    iters = 0) and 'inliers0' / 'rms0' of the start pose.  A step that fails passes its pose on.  2 (iters + 1) launches besides the
    rasteriser's, bit-identical from run to run, safe under torch.cuda.graph.  ``cull``: the passes render with
    mesh_raster(cull=True), same bits.  ``texels`` [F,T,3] with ``vcolor`` None: the passes colour the mesh from its face texels
    (mesh_raster(texels=), K35); exactly one of the two.  ``exposure``: the photograph was taken under another exposure, white
    balance or light than the colours: every pass first fits a gain and a bias per image and channel and renders under them
    (photo_exposure, K37: three launches more per pass), the first pass over the pixels within ``exposure_tau0`` of the
    plain colours (2.0 keeps every pixel of colours in [0, 1]), each later one within that pass's ``tau`` of the fit before -> also 'gain'
    / 'bias' [B,3] and 'exposure_status' [B] int32 of the last pass.  Without it nothing else runs and the keys are those above.
    ``pyramid``: coarse to fine (K38), a tuple of step counts per level, the coarsest first, whose sum must be ``iters``:
    (4, 3, 3) takes 4 steps at level 2 (a quarter of the size), 3 at level 1 and 3 at level 0.  The photograph's and the mask's
    pyramids are built once per call (image_pyramid, mask_pyramid); every pass still renders at full size, so ``vcolor``, ``texels``
    and ``cull`` work unchanged, filters the rendering down to its level (surface_down) and runs the same step on the level's planes
    with K's rows 0 and 1 times 2^-level; ``exposure`` fits on the level's planes.  ``tau`` keeps its ``iters`` + 1 entries, the final
    evaluation runs at level 0, and 'inliers0' / 'rms0' are the FIRST pass's, counted at its own level.  It widens the basin where the
    texture is fine against the start error (on the pinned cases it recovers starts the plain loop loses, and about doubles what the
    loop tolerates); a level needs enough covered pixels (the pinned cases have 43 - 142 at the coarsest level; 21 - 24 diverge).  None: nothing else runs, bit for bit the call without it.
    ``lighting``: the photograph was taken under a light with a DIRECTION (a lamp on one side), which no gain and bias can absorb: every
    pass first fits ambient + directional shading (first-order spherical harmonics on the faces' own normals) and a bias per image and
    channel and renders under them (photo_lighting, K40: three launches more per pass, and the passes render the face index too; DESIGN
    section 30), kept as ``exposure`` keeps (``exposure_tau0``, then the pass's ``tau`` under the light before) -> also 'light' [B,3,5]
    (per channel l0, l1, l2, l3, beta), 'lighting_status' and 'lighting_flags' [B] int32 of the last pass.  The model contains
    ``exposure``'s: the two together are refused.  With ``pyramid`` the fit runs at full size, before the rendering is filtered down.
    ``workspace`` must then be photo_align_workspace(B, H, W, device, lighting=True).  False: nothing else runs."""
    op, given = "photo_align", [(_PHOTO, image, tau, mask)]
    if exposure and lighting:
        raise ValueError("%s: exposure= and lighting= exclude each other (the lighting model contains the exposure's)" % op)
    if (vcolor is None) == (texels is None):
        raise ValueError("%s: exactly one of vcolor [V,3] and texels= [F,T,3] expected" % op)
    if pyramid is not None:
        _pass_levels(op, pyramid, int(iters))                    # (a host argument: refused before anything touches the device)
    return _refine(op, PHOTO_ALIGN_KEYS, verts, faces, pose, intr, given, _schedules(op, given, iters), damping=damping, frame=frame,
                   workspace=workspace, cull=cull, vcolor=vcolor, texels=texels, exposure=exposure, exposure_tau0=exposure_tau0, pyramid=pyramid,
                   lighting=lighting)


# ------------------------------------------------------------------------------------------ K37
def photo_exposure_workspace(B: int, H: int, W: int, device) -> Tensor:
    """A workspace for photo_exposure at B images of H x W (tp_photo_exposure_workspace_bytes, the terms' own size); needs no
    clearing."""
    return _workspace_arg("photo_exposure", None, int(_lib.load().tp_photo_exposure_workspace_bytes(B, H, W)), device)


PHOTO_EXPOSURE_KEYS = ("gain", "bias", "count", "rms", "status", "flags")


@_on_tensor_device
def photo_exposure(zbuf: Tensor, rgb: Tensor, image: Tensor, *, tau: float, gain: Optional[Tensor] = None, bias: Optional[Tensor] = None,
                   frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, gain_range=(0.25, 4.0), min_var: float = 1e-6,
                   apply: bool = True, inplace: bool = False, workspace: Optional[Tensor] = None,
                   out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """The per-image, per-channel gain and bias between B renderings and their photographs, and the renderings under that fit
    (tp_photo_exposure, K37; the rules are in the header): zbuf [B,H,W] / rgb [B,H,W,3] (mesh_raster's planes at the current poses;
    taken as they are), image [Ft,H,W,3] (the photograph, channels last; Ft 1 or B, or any Ft with ``frame`` [B] int32), mask
    [Ft,H,W] uint8 or bool (0: skip the pixel), ``gain`` / ``bias`` [B,3] float32 (the fit of the pass before, which decides with
    ``tau`` what is kept; None: 1 and 0) -> 'gain' / 'bias' [B,3] (image ~ gain * rgb + bias by least squares over the interior covered
    pixels the incoming fit explains within ``tau``; the gain clamped into ``gain_range``, 1 for a channel whose variance is not above
    ``min_var``), 'count' [B] int32, 'rms' [B] (colour units, of the new fit), 'status' [B] int32 (0 ok, 1 fewer than 6 kept pixels, 3
    not finite: gain and bias are then the incoming ones bit for bit), 'flags' [B] int32 (_lib.EXPOSURE_CLAMPED << k,
    _lib.EXPOSURE_FLAT << k) and, with ``apply``, 'rgb' [B,H,W,3]: gain * rgb + bias on the covered pixels, the rest copied; with
    ``inplace`` it is ``rgb`` itself, rewritten.  ``workspace``: photo_exposure_workspace(B, H, W); ``out``: any of these tensors to
    write into (out['gain'] / out['bias'] must not be ``gain`` / ``bias``).  Three launches (two without ``apply``), no atomics,
    bit-identical from run to run, safe under torch.cuda.graph."""
    op = "photo_exposure"
    zbuf = _want_gpu(op, zbuf, "zbuf", torch.float32, None)
    if zbuf.dim() != 3 or zbuf.numel() == 0:
        raise ValueError("%s: zbuf [B,H,W] expected, got %s" % (op, tuple(zbuf.shape)))
    B, H, W = zbuf.shape
    rgb = _want_gpu(op, rgb, "rgb", torch.float32, (B, H, W, 3))
    image, frame, mask, Ft = _frame_planes(op, _PHOTO, image, frame, mask, B, H, W, zbuf)
    gain = None if gain is None else _want_gpu(op, gain, "gain", torch.float32, (B, 3))
    bias = None if bias is None else _want_gpu(op, bias, "bias", torch.float32, (B, 3))
    try:
        lo, hi = (float(x) for x in gain_range)
    except (TypeError, ValueError):
        raise ValueError("%s: gain_range must be two host values (min, max), got %r" % (op, gain_range)) from None
    spec = {"gain": (torch.float32, (B, 3)), "bias": (torch.float32, (B, 3)), "count": (torch.int32, (B,)), "rms": (torch.float32, (B,)),
            "status": (torch.int32, (B,)), "flags": (torch.int32, (B,))}
    if apply and inplace:
        if out is not None and "rgb" in out:
            raise ValueError("%s: out['rgb'] and inplace=True exclude each other" % op)
    elif apply:
        spec["rgb"] = (torch.float32, (B, H, W, 3))
    res = _outputs(op, out, spec, zbuf.device, partial=True)
    workspace = _workspace_arg(op, workspace, int(_lib.load().tp_photo_exposure_workspace_bytes(B, H, W)), zbuf.device, align=16)
    a = _lib.PhotoExposureArgs()
    a.zbuf, a.rgb, a.image, a.frame, a.mask = zbuf.data_ptr(), rgb.data_ptr(), image.data_ptr(), _ptr(frame), _ptr(mask)
    a.gain_in, a.bias_in = _ptr(gain), _ptr(bias)
    a.B, a.Ft, a.H, a.W = B, Ft, H, W
    a.tau, a.gain_min, a.gain_max, a.min_var = float(tau), lo, hi, float(min_var)
    for k in PHOTO_EXPOSURE_KEYS:
        setattr(a, k, res[k].data_ptr())
    if apply and inplace:
        res["rgb"] = rgb
    a.rgb_out = res["rgb"].data_ptr() if apply else None
    a.workspace = workspace.data_ptr()
    _call("tp_photo_exposure", a)         # (tau, gain_range, min_var out of range, outputs overlapping inputs: the library's error)
    return res


# ------------------------------------------------------------------------------------------ K40
def photo_lighting_workspace(B: int, H: int, W: int, device) -> Tensor:
    """A workspace for photo_lighting at B images of H x W (tp_photo_lighting_workspace_bytes: twice a term's); needs no clearing."""
    return _workspace_arg("photo_lighting", None, int(_lib.load().tp_photo_lighting_workspace_bytes(B, H, W)), device)


PHOTO_LIGHTING_KEYS = ("light", "count", "rms", "status", "flags")


@_on_tensor_device
def photo_lighting(verts: Tensor, faces: Tensor, face: Tensor, zbuf: Tensor, rgb: Tensor, pose: Tensor, image: Tensor, *, tau: float,
                   light: Optional[Tensor] = None, frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, gain_range=(0.25, 4.0),
                   min_var: float = 1e-6, apply: bool = True, inplace: bool = False, workspace: Optional[Tensor] = None,
                   out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """Ambient + directional shading and a bias per image and channel between B renderings and their photographs, and the renderings
    under that fit (tp_photo_lighting, K40; the rules are in the header): verts [V,3], faces [F,3] int32, face / zbuf [B,H,W] and rgb
    [B,H,W,3] (mesh_raster's planes of the mesh at ``pose``; taken as they are: a face index or a vertex index out of range gives a
    pixel without a normal, never a read out of bounds), pose [B,3,4], image / frame / mask as photo_exposure's, ``light`` [B,3,5]
    float32 (per channel l0, l1, l2, l3, beta: the light of the pass before, which decides with ``tau`` what is kept; None: (1, 0, 0,
    0, 0)) -> 'light' [B,3,5] (image ~ (l0 + l1 n_x + l2 n_y + l3 n_z) rgb + beta by least squares over the kept pixels, n the
    face's unit normal in the camera frame, towards the camera; a channel whose 5 x 5 system fails the pivot rule, or whose solution
    leaves ``gain_range`` in l0 or has |(l1, l2, l3)| > l0, takes photo_exposure's gain and bias with l1 = l2 = l3 = 0), 'count' [B]
    int32, 'rms' [B], 'status' [B] int32 (0 ok, 1 fewer than 6 kept pixels, 3 not finite: the light is then the incoming one bit for
    bit), 'flags' [B] int32 (_lib.LIGHTING_FALLBACK << k beside photo_exposure's bits) and, with ``apply``, 'rgb' [B,H,W,3]: the
    shading times rgb plus beta on the covered pixels (the ambient form l0 rgb + beta where a pixel has no normal), the rest copied;
    with ``inplace`` it is ``rgb`` itself, rewritten.  ``workspace``: photo_lighting_workspace(B, H, W); ``out``: any of these tensors
    to write into (out['light'] must not be ``light``).  Three launches (two without ``apply``), no atomics, bit-identical from run to
    run, safe under torch.cuda.graph."""
    op = "photo_lighting"
    verts = _points(op, verts, "verts")
    faces = _want_gpu(op, faces, "faces", torch.int32, None)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
        raise ValueError("%s: faces [F,3] expected, got %s" % (op, tuple(faces.shape)))
    zbuf = _want_gpu(op, zbuf, "zbuf", torch.float32, None)
    if zbuf.dim() != 3 or zbuf.numel() == 0:
        raise ValueError("%s: zbuf [B,H,W] expected, got %s" % (op, tuple(zbuf.shape)))
    B, H, W = zbuf.shape
    face = _want_gpu(op, face, "face", torch.int32, (B, H, W))
    rgb = _want_gpu(op, rgb, "rgb", torch.float32, (B, H, W, 3))
    pose = _poses(op, pose, "pose")
    if pose.shape[0] != B:
        raise ValueError("%s: pose [B=%d,3,4] expected, got %s" % (op, B, tuple(pose.shape)))
    image, frame, mask, Ft = _frame_planes(op, _PHOTO, image, frame, mask, B, H, W, zbuf)
    light = None if light is None else _want_gpu(op, light, "light", torch.float32, (B, 3, 5))
    try:
        lo, hi = (float(x) for x in gain_range)
    except (TypeError, ValueError):
        raise ValueError("%s: gain_range must be two host values (min, max), got %r" % (op, gain_range)) from None
    spec = {"light": (torch.float32, (B, 3, 5)), "count": (torch.int32, (B,)), "rms": (torch.float32, (B,)), "status": (torch.int32, (B,)),
            "flags": (torch.int32, (B,))}
    if apply and inplace:
        if out is not None and "rgb" in out:
            raise ValueError("%s: out['rgb'] and inplace=True exclude each other" % op)
    elif apply:
        spec["rgb"] = (torch.float32, (B, H, W, 3))
    res = _outputs(op, out, spec, zbuf.device, partial=True)
    workspace = _workspace_arg(op, workspace, int(_lib.load().tp_photo_lighting_workspace_bytes(B, H, W)), zbuf.device, align=16)
    a = _lib.PhotoLightingArgs()
    a.verts, a.faces, a.face, a.zbuf, a.rgb, a.pose = (t.data_ptr() for t in (verts, faces, face, zbuf, rgb, pose))
    a.image, a.frame, a.mask, a.light_in = image.data_ptr(), _ptr(frame), _ptr(mask), _ptr(light)
    a.V, a.F, a.B, a.Ft, a.H, a.W = verts.shape[0], faces.shape[0], B, Ft, H, W
    a.tau, a.gain_min, a.gain_max, a.min_var = float(tau), lo, hi, float(min_var)
    for k in PHOTO_LIGHTING_KEYS:
        setattr(a, k, res[k].data_ptr())
    if apply and inplace:
        res["rgb"] = rgb
    a.rgb_out = res["rgb"].data_ptr() if apply else None
    a.workspace = workspace.data_ptr()
    _call("tp_photo_lighting", a)         # (tau, gain_range, min_var out of range, outputs overlapping inputs: the library's error)
    return res


# ------------------------------------------------------------------------------------------ K38
def _down_args(op: str, planes: dict, out: Optional[Dict[str, Tensor]]):
    """The arguments of one level down for ``planes`` = {name of the args' field: a contiguous GPU tensor [N,H,W] + trailing, taken as
    it is}: every plane's output [N,H//2,W//2] + trailing goes to the field '<name>_out' -> (the filled struct, {name: output})."""
    first = next(iter(planes.values()))
    N, H, W = first.shape[:3]
    if first.numel() == 0:
        raise ValueError("%s: empty planes %s" % (op, tuple(first.shape)))
    res = _outputs(op, out, {k: (t.dtype, (N, H // 2, W // 2) + tuple(t.shape[3:])) for k, t in planes.items()}, first.device, partial=True)
    a = _lib.PyramidDownArgs()
    a.N, a.H, a.W = N, H, W
    for k, t in planes.items():
        setattr(a, k, t.data_ptr())
        setattr(a, k + "_out", res[k].data_ptr())
    return a, res                         # (H < 2, W < 2, N > 65535, an output overlapping an input: the library's error)


@_on_tensor_device
def image_down(image: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """One level down the photograph's pyramid (tp_image_down, K38; the rules are in the header): image [N,H,W,3] float32, channels
    last, taken as it is -> [N,H//2,W//2,3]: the (1, 3, 3, 1) / 8 filter in rows and columns on clamped taps, fp64 in one stated order,
    rounded once; non-finite taps propagate.  Level l's intrinsics are K with rows 0 and 1 times 2^-l.  ``out``: the tensor to write
    into.  One launch, bit-identical from run to run, safe under torch.cuda.graph."""
    op = "image_down"
    image = _want_gpu(op, image, "image", torch.float32, None)
    if image.dim() != 4 or image.shape[3] != 3:
        raise ValueError("%s: image [N,H,W,3] (channels last) expected, got %s" % (op, tuple(image.shape)))
    a, res = _down_args(op, {"rgb": image}, None if out is None else {"rgb": out})
    _call("tp_image_down", a)
    return res["rgb"]


@_on_tensor_device
def surface_down(zbuf: Tensor, rgb: Tensor, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """One level down a rendering (tp_surface_down, K38): zbuf [B,H,W] / rgb [B,H,W,3] (mesh_raster's planes, or this function's;
    taken as they are) -> 'zbuf' [B,H//2,W//2] and 'rgb' [B,H//2,W//2,3]: a coarse pixel whose 16 taps all have z > 0 and finite holds
    the filtered depth and colours (image_down's arithmetic), every other one mesh_raster's background (-1 and 0).  Where the photograph
    is the rendering over any background, the two sides of such a pixel are equal bit for bit at every level.  ``out``: either tensor
    to write into.  One launch, bit-identical from run to run, safe under torch.cuda.graph."""
    op = "surface_down"
    zbuf = _want_gpu(op, zbuf, "zbuf", torch.float32, None)
    if zbuf.dim() != 3:
        raise ValueError("%s: zbuf [B,H,W] expected, got %s" % (op, tuple(zbuf.shape)))
    rgb = _want_gpu(op, rgb, "rgb", torch.float32, tuple(zbuf.shape) + (3,))
    a, res = _down_args(op, {"zbuf": zbuf, "rgb": rgb}, out)
    _call("tp_surface_down", a)
    return res


@_on_tensor_device
def mask_down(mask: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """One level down a mask (tp_mask_down, K38): mask [N,H,W] uint8 or bool -> [N,H//2,W//2] uint8, 1 where all 16 taps are non-zero,
    else 0: a pixel is used at a level only if nothing it mixes in was masked out.  ``out``: the tensor to write into.  One launch."""
    op = "mask_down"
    if torch.is_tensor(mask) and mask.dtype == torch.bool:
        mask = mask.view(torch.uint8) if mask.is_contiguous() else mask.to(torch.uint8)
    mask = _want_gpu(op, mask, "mask", torch.uint8, None)
    if mask.dim() != 3:
        raise ValueError("%s: mask [N,H,W] expected, got %s" % (op, tuple(mask.shape)))
    a, res = _down_args(op, {"mask": mask}, None if out is None else {"mask": out})
    _call("tp_mask_down", a)
    return res["mask"]


def _pyramid(op: str, down, plane: Tensor, levels: int) -> list:
    levels = int(levels)
    if levels < 1:
        raise ValueError("%s: levels >= 1 expected, got %d" % (op, levels))
    out = [plane]
    for _ in range(levels - 1):
        out.append(down(out[-1]))
    return out


def image_pyramid(image: Tensor, levels: int) -> list:
    """[image, image_down(image), ...]: ``levels`` entries, the finest first; entry l is the photograph at level l (K38)."""
    return _pyramid("image_pyramid", image_down, image, levels)


def mask_pyramid(mask: Tensor, levels: int) -> list:
    """[mask, mask_down(mask), ...]: ``levels`` entries, the finest first (K38)."""
    return _pyramid("mask_pyramid", mask_down, mask, levels)


def _pass_levels(op: str, pyramid, iters: int) -> list:
    """``pyramid`` = steps per level, the coarsest first -> the level of every pass, the final evaluation's (0) included."""
    try:
        steps = [int(n) for n in pyramid]
    except (TypeError, ValueError):
        raise ValueError("%s: pyramid must be a tuple of step counts per level, the coarsest first, got %r" % (op, pyramid)) from None
    if not steps or min(steps) < 0 or any(n != p for n, p in zip(steps, pyramid)):
        raise ValueError("%s: pyramid must be a tuple of step counts (integers >= 0) per level, the coarsest first, got %r" % (op, pyramid))
    if sum(steps) != iters:
        raise ValueError("%s: the steps of pyramid %r must add up to iters = %d, got %d" % (op, tuple(pyramid), iters, sum(steps)))
    return [len(steps) - 1 - k for k, n in enumerate(steps) for _ in range(n)] + [0]


# ------------------------------------------------------------------------------------------ K31
def mask_sdf_workspace(F: int, H: int, W: int, device) -> Tensor:
    """A workspace for mask_sdf at F masks of H x W (tp_mask_sdf_workspace_bytes); needs no clearing."""
    return _workspace_arg("mask_sdf", None, int(_lib.load().tp_mask_sdf_workspace_bytes(F, H, W)), device)


@_on_tensor_device
def mask_sdf(mask: Tensor, out: Optional[Tensor] = None, workspace: Optional[Tensor] = None, known: Optional[Tensor] = None) -> Tensor:
    """The exact signed Euclidean distance field of F masks (tp_mask_sdf; the rules are in the header): mask [F,H,W] (or one [H,W])
    uint8 or bool, non-zero: set -> sdf float32 of mask's shape, in pixels: sqrt(d2_set) - 0.5 on a clear pixel, -(sqrt(d2_clear) -
    0.5) on a set one, with the squared distances to the nearest set / clear pixel of the plane (H^2 + W^2 where it has none).
    ``out``: the tensor to write into; ``workspace``: mask_sdf_workspace(F, H, W).  H, W <= 8192.  Two launches, no atomics, a function
    of the mask alone, safe under torch.cuda.graph.  ``known`` (uint8 or bool, of mask's shape, non-zero: the pixel's mask value is a
    measurement) makes the rest UNKNOWN, neither set nor clear (tp_mask_sdf_known, K31c): no distance is measured to such a pixel and
    its own value is NaN, which silhouette_align_step drops; with every pixel known the field is the plain one bit for bit."""
    op = "mask_sdf"
    if torch.is_tensor(mask) and not mask.is_cuda:
        raise _lib.TexposeLibraryError("mask must live on the GPU (texpose_amd has no CPU path)")
    if torch.is_tensor(mask) and mask.dtype == torch.bool:
        mask = mask.view(torch.uint8) if mask.is_contiguous() else mask.to(torch.uint8)
    mask = _want_gpu(op, mask, "mask", torch.uint8, None)
    if known is not None:
        if torch.is_tensor(known) and known.dtype == torch.bool:
            known = known.view(torch.uint8) if known.is_contiguous() else known.to(torch.uint8)
        known = _want_gpu(op, known, "known", torch.uint8, tuple(mask.shape))
    if mask.dim() not in (2, 3) or mask.numel() == 0:
        raise ValueError("%s: mask [F,H,W] or [H,W] expected, got %s" % (op, tuple(mask.shape)))
    F, H, W = (1,) + tuple(mask.shape) if mask.dim() == 2 else tuple(mask.shape)
    sdf = torch.empty(mask.shape, device=mask.device) if out is None else _want_gpu(op, out, "out", torch.float32, tuple(mask.shape))
    workspace = _workspace_arg(op, workspace, int(_lib.load().tp_mask_sdf_workspace_bytes(F, H, W)), mask.device, align=16)
    if known is None:
        _call("tp_mask_sdf", mask.data_ptr(), sdf.data_ptr(), F, H, W, workspace.data_ptr())      # (H or W > 8192: the library's error)
    else:
        _call("tp_mask_sdf_known", mask.data_ptr(), known.data_ptr(), sdf.data_ptr(), F, H, W, workspace.data_ptr())
    return sdf


@_on_tensor_device
def mask_known_from_others(sdf: Tensor, band_px: float = 0.0, out: Optional[Tensor] = None) -> Tensor:
    """Who hides whom among the N instances of ONE frame (tp_mask_known_from_others, K32; the rules are in the header): sdf [N,H,W]
    float32, mask_sdf's fields of the frame's instance masks (taken as they are) -> known [N,H,W] uint8: 0 where the pixel lies within
    ``band_px`` pixels of a set pixel of ANOTHER instance (sdf[m,p] <= band_px - 0.5 in fp32 for some m != n; a NaN is not near), else
    1: mask_sdf's ``known``.  Conservative: where two instances touch, both lose the contour between them.  ``out``: the uint8 tensor
    to write into.  One launch, no workspace, no atomics, safe under torch.cuda.graph."""
    op = "mask_known_from_others"
    if torch.is_tensor(sdf) and not sdf.is_cuda:
        raise _lib.TexposeLibraryError("sdf must live on the GPU (texpose_amd has no CPU path)")
    sdf = _want_gpu(op, sdf, "sdf", torch.float32, None)
    if sdf.dim() != 3 or sdf.numel() == 0:
        raise ValueError("%s: sdf [N,H,W] expected, got %s" % (op, tuple(sdf.shape)))
    N, H, W = sdf.shape
    known = torch.empty(sdf.shape, device=sdf.device, dtype=torch.uint8) if out is None else _want_gpu(op, out, "out", torch.uint8, tuple(sdf.shape))
    _call("tp_mask_known_from_others", sdf.data_ptr(), known.data_ptr(), N, H, W, float(band_px))  # (band_px, N > 65535: the library's error)
    return known


def silhouette_align_workspace(B: int, H: int, W: int, device) -> Tensor:
    """A workspace for silhouette_align_step / silhouette_align at B images of H x W (tp_silhouette_align_workspace_bytes); needs no
    clearing."""
    return _new_workspace("silhouette_align", (_SILHOUETTE,), B, H, W, device)


@_on_tensor_device
def silhouette_align_step(zbuf: Tensor, pose: Tensor, intr: Tensor, sdf: Tensor, *, tau_px: float, damping: float = 1e-6,
                          frame: Optional[Tensor] = None, mask: Optional[Tensor] = None, evaluate_only: bool = False,
                          workspace: Optional[Tensor] = None, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """One step of silhouette alignment for B poses (tp_silhouette_align_step; the rules are in the header): zbuf [B,H,W]
    (mesh_raster's depth of the mesh at ``pose``; taken as it is), pose [B,3,4], intr [B,3,3] or one [3,3], sdf [Ft,H,W] (mask_sdf's
    field of the measured masks: pixels, negative inside; Ft 1 or B, or any Ft with ``frame`` [B] int32), mask [Ft,H,W] uint8 or bool
    (0: the pixel gives no row) -> 'pose' [B,3,4] (the stepped pose; ``pose`` itself, bit for bit, with ``evaluate_only`` or a
    non-zero status), 'inliers' [B] int32 and 'rms' [B] (pixels) of ``pose`` over the interior rim pixels of the rendering within
    ``tau_px`` of the measured outline, 'status' [B] int32 (0 ok, 1 fewer than 6 kept pixels, 3 not positive definite), 'inter' and
    'uni' [B] int32 (the pixels covered and inside the measured mask, and those with either: IoU = inter / uni).  ``workspace``:
    silhouette_align_workspace(B, H, W); ``out``: any of the six tensors to write into (out['pose'] must not be ``pose``).  Three
    launches, no atomics, bit-identical from run to run, safe under torch.cuda.graph."""
    a, res, _alive = _term_args(_SILHOUETTE, "silhouette_align_step", dict(zbuf=zbuf, pose=pose, intr=intr, sdf=sdf), threshold=tau_px, damping=damping,
                                frame=frame, mask=mask, evaluate_only=evaluate_only, workspace=workspace, out=out)
    _call("tp_silhouette_align_step", a)  # (tau_px, damping out of range, out['pose'] overlapping pose: the library's error)
    return res


SILHOUETTE_ALIGN_KEYS = ("pose", "inliers", "rms", "status", "inliers0", "rms0", "iou", "iou0")


@_on_tensor_device
def silhouette_align(verts: Tensor, faces: Tensor, pose: Tensor, intr: Tensor, sdf: Tensor, *, tau_px=4.0, iters: int = 10,
                     damping: float = 1e-6, frame: Optional[Tensor] = None, mask: Optional[Tensor] = None,
                     workspace: Optional[Tensor] = None, visible_iou: bool = False, cull: bool = False) -> Dict[str, Tensor]:
    """Refine B poses of one mesh against the outlines of measured masks (the rules are in the header, K31): ``iters`` + 1 passes of
    mesh_raster at the current poses (depth alone, H x W = sdf's) followed by silhouette_align_step, the last with evaluate_only.
    ``sdf`` [Ft,H,W]: mask_sdf of the measured masks.  ``tau_px``: one value, or ``iters`` + 1 host values for a coarse-to-fine schedule
    (the last is the final evaluation's).  -> 'pose' [B,3,4], its 'inliers' [B] int32 and 'rms' [B] (pixels), 'status' [B] int32 of the
    last step taken (of the evaluation where iters = 0), 'inliers0' / 'rms0' of the start pose and 'iou' / 'iou0' [B] float32, the
    intersection over union of the rendering's coverage and the measured mask at the last and at the start pose (NaN where both are
    empty).  A step that fails passes its pose on.  It closes the OUTLINE: a pose parameter the outline does not see (a rotation about
    a symmetry axis, depth at a small radius) stays where it was, and a measured mask cut by an occluder pulls the rim to the cut.
    3 (iters + 1) launches besides the rasteriser's, bit-identical from run to run, safe under torch.cuda.graph.
    ``visible_iou``: for a field with unknown pixels (mask_sdf's ``known``; NaN there) also 'iou_visible' / 'iou0_visible' [B] float32,
    inter / (uni - hidden) at the last and at the start pose, ``hidden`` the covered pixels of the plane whose field value is NaN: the
    IoU over the pixels that were measured (NaN where none is left).  Exact integer counts by torch reductions on the first and the
    last rendering; without the flag nothing else runs and the keys are those above.  ``cull``: the passes render with
    mesh_raster(cull=True), same bits."""
    op, given = "silhouette_align", [(_SILHOUETTE, sdf, tau_px, mask)]
    return _refine(op, SILHOUETTE_ALIGN_KEYS[:6], verts, faces, pose, intr, given, _schedules(op, given, iters), damping=damping, frame=frame,
                   workspace=workspace, cull=cull, visible_iou=visible_iou)


_STEPS = dict(zip(JOINT_TERMS, (silhouette_align_step, photo_align_step, depth_icp_step)))          # a single-term loop launches its own step


# ------------------------------------------------------------------------------------------ K33
# 1 / sigma^2 per residual unit (pixels, colour units, mm).  w_photo = 100 is the only one of 25, 100 and 400 with which the twelve
# occluded cases of DESIGN section 23 all converged; w_icp = 1 / 25 is sigma = 5 mm and is NOT tuned on anything.
JOINT_WEIGHTS = (1.0, 100.0, 1.0 / 25.0)


def _joint_weights(op: str, weights) -> tuple:
    try:
        w = tuple(float(x) for x in weights)
    except TypeError:
        w = ()
    if len(w) != 3:
        raise ValueError("%s: weights must be three host values (silhouette, photo, depth), got %r" % (op, weights))
    if not all(x >= 0.0 and x != float("inf") for x in w):
        raise ValueError("%s: weights must be finite and not negative, got %r" % (op, w))
    return w


def joint_align_workspace(B: int, H: int, W: int, device, terms: int = 3, lighting: bool = False) -> Tensor:
    """A workspace for joint_align_step / joint_align at B images of H x W with ``terms`` terms present (each term's own
    ``*_workspace_bytes``, one after the other); needs no clearing.  ``lighting``: for joint_align(lighting=True)."""
    return _new_workspace("joint_align", _TERMS[:int(terms)], B, H, W, device, lighting)


def _step_terms(op: str, pose: Tensor, intr: Tensor, given: dict, damping, out, workspace, tail_bytes: int = 0):
    """The present terms of a joint or a multi-view step, checked: ``given`` name -> the term's dict or None -> (the three args structs
    in _TERMS order, None where absent; the per-term outputs under their prefixes; the tensors the structs point into; pose [B,3,4];
    intr [B,3,3]; the ``tail_bytes`` of the workspace behind the terms' parts as uint8, or None)."""
    pose = _poses(op, pose, "pose")
    B = pose.shape[0]
    intr = _intr_per_view(op, intr, B)
    shapes = {name: tuple(t["zbuf"].shape) if torch.is_tensor(t.get("zbuf")) else None for name, t in given.items() if t is not None}
    shape = next(iter(shapes.values()))
    if len(set(shapes.values())) != 1 or shape is None or len(shape) != 3:
        raise ValueError("%s: every term needs a zbuf [B,H,W] of one shape, got %r" % (op, shapes))
    H, W = shape[1:]
    dev = pose.device
    present = [term for term in _TERMS if given[term.name] is not None]
    need = dict(zip(present, _term_bytes(present, B, H, W, 16)))
    workspace = _workspace_arg(op, workspace, sum(need.values()) + tail_bytes, dev, align=16)
    raw, offset = workspace.view(torch.uint8).reshape(-1), 0
    res, structs, alive = {}, [], [workspace]
    for term in _TERMS:
        t = given[term.name]
        if t is None:
            structs.append(None)
            continue
        takes = term.rendered + (term.plane, term.threshold)
        unknown = set(t) - set(takes) - {"frame", "mask"}
        missing = [k for k in takes if k not in t]
        if unknown or missing:
            raise ValueError("%s: the %s term takes %s, frame and mask; missing %s, unknown %s" % (op, term.name, ", ".join(takes), missing, sorted(unknown)))
        term_out = None if out is None else {k[len(term.prefix):]: v for k, v in out.items() if k.startswith(term.prefix)}
        a, r, keep = _term_args(term, "%s (%s)" % (op, term.name), dict({k: t[k] for k in term.rendered}, pose=pose, intr=intr, **{term.plane: t[term.plane]}),
                                threshold=t[term.threshold], damping=damping, frame=t.get("frame"), mask=t.get("mask"), evaluate_only=True,
                                workspace=raw[offset:offset + need[term]], out=term_out, with_pose=False)
        offset += need[term]
        structs.append(a)
        alive.append(keep)
        res.update({term.prefix + k: v for k, v in r.items()})
    return structs, res, alive, pose, intr, (raw[offset:offset + tail_bytes] if tail_bytes else None)


@_on_tensor_device
def joint_align_step(pose: Tensor, intr: Tensor, *, silhouette: Optional[dict] = None, photo: Optional[dict] = None, depth: Optional[dict] = None,
                     weights=JOINT_WEIGHTS, damping: float = 1e-6, evaluate_only: bool = False, out: Optional[Dict[str, Tensor]] = None,
                     workspace: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """One JOINT Gauss-Newton step for B poses: the rows of the silhouette, the photometric and the depth term in one normal system
    (tp_joint_align_step, K33; the rules are in the header).  pose [B,3,4], intr [B,3,3] or one [3,3]; each term that takes part is a
    dict of that term's own step arguments (planes rendered at ``pose``, threshold, and optionally ``frame`` and ``mask``):
    ``silhouette`` = dict(zbuf, sdf, tau_px), ``photo`` = dict(zbuf, rgb, image, tau), ``depth`` = dict(verts, faces, zbuf, face, depth,
    tau_mm).  ``weights`` (w_sil, w_photo, w_icp): 1 / sigma^2 of the term's residual unit; a present term with weight 0 is evaluated
    but takes no part in the step.  -> 'pose' [B,3,4] (the stepped pose; ``pose`` itself, bit for bit, with ``evaluate_only`` or a
    non-zero status), 'status' [B] int32 (0 ok, 1 fewer than 6 kept pixels over the weighted terms, 3 not positive definite),
    'inliers' [B] int32 (their kept pixels, added), 'chi2' [B] (the weighted sum of squares), and per present term that term's own
    evaluation of ``pose``, bit for bit its ``*_step(evaluate_only=True)``: 'sil_inliers', 'sil_rms', 'sil_status', 'sil_inter',
    'sil_uni', 'photo_inliers', 'photo_rms', 'photo_status', 'icp_inliers', 'icp_rms', 'icp_status'.  ``workspace``:
    joint_align_workspace(B, H, W, terms present); ``out``: any of these tensors to write into (out['pose'] must not be ``pose``).
    With one term at weight 1 'pose' and 'status' are that term's own step's bit for bit.  Each term's launches and one more, no
    atomics, bit-identical from run to run, safe under torch.cuda.graph."""
    op = "joint_align_step"
    w = _joint_weights(op, weights)
    given = dict(zip(JOINT_TERMS, (silhouette, photo, depth)))
    if all(v is None for v in given.values()):
        raise ValueError("%s: no term: give at least one of %s" % (op, ", ".join(name + "=" for name in JOINT_TERMS)))
    if not any(v is not None and x > 0 for v, x in zip(given.values(), w)):
        raise ValueError("%s: no present term has a weight > 0 (weights %r)" % (op, w))
    structs, res, _alive, pose, intr, _ = _step_terms(op, pose, intr, given, damping, out, workspace)
    B, dev = pose.shape[0], pose.device
    joint = _outputs(op, out, {"pose": (torch.float32, (B, 3, 4)), "status": (torch.int32, (B,)), "inliers": (torch.int32, (B,)),
                               "chi2": (torch.float32, (B,))}, dev, partial=True)
    j = _lib.JointAlignArgs()
    j.B, j.pose, j.damping, j.evaluate_only = B, pose.data_ptr(), float(damping), int(bool(evaluate_only))
    for term, x in zip(_TERMS, w):
        setattr(j, "w_" + term.prefix[:-1], x)
    j.pose_out, j.status, j.inliers, j.chi2 = joint["pose"].data_ptr(), joint["status"].data_ptr(), joint["inliers"].data_ptr(), joint["chi2"].data_ptr()
    _call("tp_joint_align_step", j, *structs)
    return dict(joint, **res)


JOINT_ALIGN_KEYS = ("pose", "inliers", "chi2", "status", "inliers0", "chi20")


@_on_tensor_device
def joint_align(verts: Tensor, faces: Tensor, pose: Tensor, intr: Tensor, *, vcolor: Optional[Tensor] = None, sdf: Optional[Tensor] = None,
                image: Optional[Tensor] = None, depth: Optional[Tensor] = None, weights=JOINT_WEIGHTS, tau_px=4.0, tau=0.5, tau_mm=20.0,
                iters: int = 20, damping: float = 1e-6, frame: Optional[Tensor] = None, masks: Optional[dict] = None,
                workspace: Optional[Tensor] = None, visible_iou: bool = False, cull: bool = False,
                texels: Optional[Tensor] = None, exposure: bool = False, exposure_tau0: float = 2.0,
                lighting: bool = False) -> Dict[str, Tensor]:
    """Refine B poses of one mesh against whichever of the measured outline (``sdf`` [Ft,H,W], mask_sdf's field), the photograph
    (``image`` [Ft,H,W,3], with the mesh's ``vcolor`` [V,3]) and the measured depth (``depth`` [Ft,H,W], mm) are given, ALL rows in
    one Gauss-Newton system per step (K33): ``iters`` + 1 passes of ONE mesh_raster call at the current poses, asked
    only for the planes the present terms need, followed by joint_align_step, the last with evaluate_only.  The outline gives the
    basin, the texture or the depth pins what the outline leaves loose: under occlusion the terms run one after the other end far
    away where this loop converges.  ``weights`` (w_sil, w_photo, w_icp) = 1 / sigma^2 per residual unit, default (1, 100, 1 / 25):
    w_photo = 100 is the only one of 25, 100 and 400 with which all twelve occluded cases of DESIGN section 23 converged; w_icp is
    sigma = 5 mm and is NOT tuned on anything.  ``tau_px`` / ``tau`` / ``tau_mm``: each term's threshold, one value or ``iters`` + 1
    host values.  ``frame`` [B] int32: the measured plane of each pose, for every term.  ``masks``: dict(silhouette=, photo=, depth=)
    of [Ft,H,W] uint8 / bool planes (0: the term skips the pixel).  -> 'pose' [B,3,4], its 'inliers' [B] int32 and 'chi2' [B],
    'status' [B] int32 of the last step taken (of the evaluation where iters = 0), 'inliers0' / 'chi20' of the start pose, and the
    last pass's per-term keys of joint_align_step; with ``sdf`` also 'iou' / 'iou0', and with ``visible_iou`` 'iou_visible' /
    'iou0_visible', as silhouette_align.  A step that fails passes its pose on.  Bit-identical from run to run, safe under
    torch.cuda.graph.  ``cull``: the passes render with mesh_raster(cull=True), same bits.  ``texels`` [F,T,3] in place of ``vcolor``:
    the photometric term's renders take their colour from the mesh's face texels (mesh_raster(texels=), K35); at most one of the two.
    ``exposure`` (with ``image``): as photo_align's, for the photometric term -> also 'photo_gain' / 'photo_bias' [B,3] and
    'photo_exposure_status' [B] int32 of the last pass; without ``image`` it does nothing.  ``lighting`` (with ``image``): as
    photo_align's, in place of ``exposure`` (both: refused) -> also 'photo_light' [B,3,5], 'photo_lighting_status' and
    'photo_lighting_flags' [B] int32; ``workspace`` must then be joint_align_workspace(..., lighting=True)."""
    op = "joint_align"
    if exposure and lighting:
        raise ValueError("%s: exposure= and lighting= exclude each other (the lighting model contains the exposure's)" % op)
    if vcolor is not None and texels is not None:
        raise ValueError("%s: vcolor= or texels=, not both" % op)
    w = _joint_weights(op, weights)
    masks = dict(masks or {})
    given = [(term, p, t, masks.get(term.name)) for term, p, t in zip(_TERMS, (sdf, image, depth), (tau_px, tau, tau_mm))]
    taus = _schedules(op, given, iters)
    if sdf is None and image is None and depth is None:
        raise ValueError("%s: no term: give at least one of sdf=, image=, depth=" % op)
    if image is not None and vcolor is None and texels is None:
        raise ValueError("%s: image= needs vcolor=, the mesh's colours [V,3], or texels= [F,T,3]" % op)
    if set(masks) - set(JOINT_TERMS):
        raise ValueError("%s: masks takes the keys %s, got %s" % (op, JOINT_TERMS, sorted(masks)))
    # (the dict has had its cost keys behind inliers0 since K33; JOINT_ALIGN_KEYS names them, not their order)
    return _refine(op, ("pose", "inliers", "status", "inliers0", "chi2", "chi20"), verts, faces, pose, intr, given, taus, damping=damping, frame=frame,
                   workspace=workspace, cull=cull, vcolor=vcolor, texels=texels, visible_iou=visible_iou, weights=w, exposure=exposure,
                   exposure_tau0=exposure_tau0, lighting=lighting)


# ------------------------------------------------------------------------------------------ K39
def _group_args(op: str, cam: Tensor, model: Tensor, group: Tensor):
    """cam [B,3,4], model [Gr,3,4] (1 <= Gr <= B) and group [B] int32 of a multi-view call, checked."""
    cam, model = _poses(op, cam, "cam"), _poses(op, model, "model")
    B, Gr = cam.shape[0], model.shape[0]
    if Gr > B:
        raise ValueError("%s: model [Gr,3,4] with 1 <= Gr <= B = %d views expected, got %s" % (op, B, tuple(model.shape)))
    return cam, model, _lengths(op, group, "group", B, cam, required=True)


def multiview_group_index(group: Tensor, Gr: int):
    """group [B] int32 (ids outside 0 .. Gr-1 clamp) -> (member [B] int32: the view indices by group, ascending inside a group;
    group_start [Gr+1] int32): what tp_multiview_align_step takes.  A stable sort and a searchsorted on the device, no host read."""
    ids = group.clamp(0, Gr - 1)
    ordered, member = torch.sort(ids, stable=True)
    start = torch.searchsorted(ordered, torch.arange(Gr + 1, device=group.device, dtype=ids.dtype))
    return member.to(torch.int32), start.to(torch.int32)


@_on_tensor_device
def pose_compose(cam: Tensor, model: Tensor, group: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """The pose of every view of a multi-view problem (tp_pose_compose, K39; the rules are in the header): cam [B,3,4] (world ->
    camera), model [Gr,3,4] (model -> world), group [B] int32 (the model of each view; out of range: clamped) -> [B,3,4]: cam[i] o
    model[group[i]] in fp64, rounded once; a cam of exactly [I|0] copies the model bit for bit.  ``out``: the tensor to write into.
    One launch, safe under torch.cuda.graph."""
    op = "pose_compose"
    cam, model, group = _group_args(op, cam, model, group)
    B = cam.shape[0]
    res = torch.empty_like(cam) if out is None else _want_gpu(op, out, "out", torch.float32, (B, 3, 4))
    a = _lib.PoseComposeArgs()
    a.B, a.Gr, a.cam, a.model, a.group, a.out = B, model.shape[0], cam.data_ptr(), model.data_ptr(), group.data_ptr(), res.data_ptr()
    _call("tp_pose_compose", a)           # (out overlapping cam or model: the library's error)
    return res


def multiview_align_workspace(B: int, H: int, W: int, device, terms: int = 3, lighting: bool = False) -> Tensor:
    """A workspace for multiview_align_step / multiview_align at B views of H x W with ``terms`` terms present (each term's own part,
    then tp_multiview_workspace_bytes(B)); needs no clearing.  ``lighting``: for multiview_align(lighting=True)."""
    return _new_workspace("multiview_align", _TERMS[:int(terms)], B, H, W, device, lighting, int(_lib.load().tp_multiview_workspace_bytes(B)), 16)


@_on_tensor_device
def multiview_align_step(model: Tensor, cam: Tensor, group: Tensor, intr: Tensor, *, silhouette: Optional[dict] = None, photo: Optional[dict] = None,
                         depth: Optional[dict] = None, weights=JOINT_WEIGHTS, damping: float = 1e-6, evaluate_only: bool = False,
                         out: Optional[Dict[str, Tensor]] = None, workspace: Optional[Tensor] = None, pose: Optional[Tensor] = None,
                         index=None) -> Dict[str, Tensor]:
    """One MULTI-VIEW Gauss-Newton step: one object pose per group of views with known cameras, all rows of a group's views in one
    normal system (tp_multiview_align_step, K39; the rules are in the header).  model [Gr,3,4] (model -> world, the unknowns), cam
    [B,3,4] (world -> camera, fixed), group [B] int32, intr [B,3,3] or one [3,3]; the terms are joint_align_step's dicts with planes
    rendered at pose_compose(cam, model, group).  -> 'model' [Gr,3,4] (the stepped poses; ``model`` bit for bit with
    ``evaluate_only`` or a non-zero status), 'pose' [B,3,4] (cam o 'model'), 'status', 'inliers', 'views' [Gr] int32, 'chi2' [Gr], and
    joint_align_step's per-term keys [B].  ``pose``: the composed poses, where the caller has them (the loop has); ``index``:
    multiview_group_index(group, Gr), likewise.  ``workspace``: multiview_align_workspace(B, H, W, terms present).  With one view per
    group and cameras of exactly [I|0] 'model' is joint_align_step's 'pose' bit for bit.  Each term's launches and three more, no
    atomics, no host read, bit-identical from run to run, safe under torch.cuda.graph."""
    op = "multiview_align_step"
    w = _joint_weights(op, weights)
    given = dict(zip(JOINT_TERMS, (silhouette, photo, depth)))
    if all(v is None for v in given.values()):
        raise ValueError("%s: no term: give at least one of %s" % (op, ", ".join(name + "=" for name in JOINT_TERMS)))
    if not any(v is not None and x > 0 for v, x in zip(given.values(), w)):
        raise ValueError("%s: no present term has a weight > 0 (weights %r)" % (op, w))
    cam, model, group = _group_args(op, cam, model, group)
    B, Gr, dev = cam.shape[0], model.shape[0], cam.device
    pose = pose_compose(cam, model, group) if pose is None else _want_gpu(op, pose, "pose", torch.float32, (B, 3, 4))
    member, start = multiview_group_index(group, Gr) if index is None else index
    member, start = _lengths(op, member, "index[0]", B, cam, required=True), _lengths(op, start, "index[1]", Gr + 1, cam, required=True)
    own_bytes = int(_lib.load().tp_multiview_workspace_bytes(B))
    structs, res, _alive, pose, intr, tail = _step_terms(op, pose, intr, given, damping, out, workspace, own_bytes)
    mine = _outputs(op, out, {"model": (torch.float32, (Gr, 3, 4)), "pose": (torch.float32, (B, 3, 4)), "status": (torch.int32, (Gr,)),
                              "inliers": (torch.int32, (Gr,)), "chi2": (torch.float32, (Gr,)), "views": (torch.int32, (Gr,))}, dev, partial=True)
    m = _lib.MultiviewArgs()
    m.B, m.Gr, m.cam, m.pose, m.model = B, Gr, cam.data_ptr(), pose.data_ptr(), model.data_ptr()
    m.member, m.group_start, m.damping, m.evaluate_only = member.data_ptr(), start.data_ptr(), float(damping), int(bool(evaluate_only))
    for term, x in zip(_TERMS, w):
        setattr(m, "w_" + term.prefix[:-1], x)
    m.model_out, m.pose_out, m.workspace = mine["model"].data_ptr(), mine["pose"].data_ptr(), tail.data_ptr()
    for k in ("status", "inliers", "chi2", "views"):
        setattr(m, k, mine[k].data_ptr())
    _call("tp_multiview_align_step", m, *structs)
    return dict(mine, **res)


MULTIVIEW_ALIGN_KEYS = ("model", "pose", "inliers", "status", "views", "inliers0", "chi2", "chi20")


@_on_tensor_device
def multiview_align(verts: Tensor, faces: Tensor, model: Tensor, cam: Tensor, group: Tensor, intr: Tensor, *, vcolor: Optional[Tensor] = None,
                    sdf: Optional[Tensor] = None, image: Optional[Tensor] = None, depth: Optional[Tensor] = None, weights=JOINT_WEIGHTS,
                    tau_px=4.0, tau=0.5, tau_mm=20.0, iters: int = 20, damping: float = 1e-6, frame: Optional[Tensor] = None,
                    masks: Optional[dict] = None, workspace: Optional[Tensor] = None, visible_iou: bool = False, cull: bool = False,
                    texels: Optional[Tensor] = None, exposure: bool = False, exposure_tau0: float = 2.0, pyramid=None,
                    lighting: bool = False) -> Dict[str, Tensor]:
    """Refine ONE pose of one mesh per group of views whose cameras are known (K39): model [Gr,3,4] (model -> world,
    the start), cam [B,3,4] (world -> camera), group [B] int32, intr [B,3,3] or [3,3]; the measurements and every other keyword are
    joint_align's, per VIEW.  ``iters`` + 1 passes of pose_compose, ONE mesh_raster call at the composed poses and
    multiview_align_step, the last with evaluate_only: a view in which the object is half hidden, or whose depth along the axis is
    loose, is pinned by the group's other views.  One term alone is allowed.  -> 'model' [Gr,3,4], 'pose' [B,3,4] (cam o model),
    'inliers', 'views' [Gr] int32 and 'chi2' [Gr] of the last pass, 'status' [Gr] of the last step taken, 'inliers0' / 'chi20' of the
    start, the last pass's per-term keys [B], and 'iou' / 'iou0' (and the visible ones) [B] as joint_align.  A group whose step fails
    passes its model on.  ``pyramid`` is refused.  Bit-identical from run to run, safe under torch.cuda.graph.  ``lighting``: as
    joint_align's, one light per VIEW (a light shared by a group's views is left out), fitted at the view's composed pose."""
    op = "multiview_align"
    if exposure and lighting:
        raise ValueError("%s: exposure= and lighting= exclude each other (the lighting model contains the exposure's)" % op)
    if pyramid is not None:
        raise ValueError("%s: pyramid= goes with the photometric term alone" % op)
    if vcolor is not None and texels is not None:
        raise ValueError("%s: vcolor= or texels=, not both" % op)
    w = _joint_weights(op, weights)
    masks = dict(masks or {})
    given = [(term, p, t, masks.get(term.name)) for term, p, t in zip(_TERMS, (sdf, image, depth), (tau_px, tau, tau_mm))]
    taus = _schedules(op, given, iters)
    if sdf is None and image is None and depth is None:
        raise ValueError("%s: no term: give at least one of sdf=, image=, depth=" % op)
    if image is not None and vcolor is None and texels is None:
        raise ValueError("%s: image= needs vcolor=, the mesh's colours [V,3], or texels= [F,T,3]" % op)
    if set(masks) - set(JOINT_TERMS):
        raise ValueError("%s: masks takes the keys %s, got %s" % (op, JOINT_TERMS, sorted(masks)))
    cam, model, group = _group_args(op, cam, model, group)
    return _refine(op, MULTIVIEW_ALIGN_KEYS, verts, faces, model, intr, given, taus, damping=damping, frame=frame, workspace=workspace, cull=cull,
                   vcolor=vcolor, texels=texels, visible_iou=visible_iou, weights=w, exposure=exposure, exposure_tau0=exposure_tau0,
                   multiview=dict(cam=cam, group=group, index=multiview_group_index(group, model.shape[0])), lighting=lighting)
