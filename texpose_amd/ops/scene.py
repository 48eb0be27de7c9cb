"""K19-K22, K27, K35, K36, K41, K42, K43: the mesh rasteriser, the surfel maps, the BOP scene writers, the texture bake, the face-texel
shading, its adjoint, its lighting step, the robust weights of its residual and its mip levels."""
import math
from typing import Dict, Optional, Tuple

import torch

from .. import _lib
from ._base import (Tensor, _call, _f32, _float3, _intr_per_view, _on_tensor_device, _outputs, _points, _poses, _ptr, _want_gpu, _workspace_arg)

__all__ = ["mesh_raster", "normals_from_depth", "SURFEL_FINISH_KEYS", "surfel_finish", "SCENE_SOURCES", "SCENE_BOUNDS_KEYS", "scene_bounds",
           "SCENE_INFO_KEYS", "scene_annotate", "view_images", "texture_bake_workspace", "texture_bake", "face_texel_shade", "face_texel_shade_bwd",
           "face_texel_light_workspace", "face_texel_light", "ROBUST_KINDS", "robust_weight_workspace", "robust_weight", "face_texel_mip_reduce",
           "face_texel_shade_mip"]


# ------------------------------------------------------------------------------------------ K19
@_on_tensor_device
def mesh_raster(verts: Tensor, faces: Tensor, pose: Tensor, intr: Tensor, *, H: int, W: int, vcolor: Optional[Tensor] = None,
                nocs_norm: Optional[Tuple[Tuple[float, float, float], Tuple[float, float, float]]] = None,
                face_ids: bool = True, normals: bool = True, zbuf_out: Optional[Tensor] = None, cull: bool = False,
                texels: Optional[Tensor] = None, texel_mips=None) -> Dict[str, Tensor]:
    """Hard rasterisation of one mesh at B poses (tp_mesh_raster).  verts [V,3] and pose [B,3,4] ([R|t], t) in the same units (mm),
    faces [F,3] int, intr [B,3,3] or [3,3].  Returns zbuf [B,H,W] (-1 on background) and, as asked, face [B,H,W] int32, rgb
    (``vcolor`` [V,3] given), nocs (``nocs_norm`` = (centre, max-abs) per axis given) and normal, each [B,H,W,3].
    ``zbuf_out``: a contiguous float32 [B,H,W] tensor (e.g. one plane of a [K,B,H,W] stack) to write zbuf into.
    ``cull``: tp_mesh_raster_culled, which skips whole chunks of 256 faces per 16 x 16 tile by their union box: the same planes bit for
    bit, one launch more (K34).
    ``texels`` [F,T(R),3] instead of ``vcolor``: rgb comes from the per-face texel texture (face_texel_shade on the face plane, which
    is then rendered and returned whatever ``face_ids`` says; K35).
    ``texel_mips`` (face_texels.build_mips of this mesh's texels) in the place of ``texels``, or beside the texels it was built from:
    rgb comes from face_texel_shade_mip, the shading with a minification filter (K43)."""
    if (texels is not None or texel_mips is not None) and vcolor is not None:
        raise ValueError("mesh_raster: vcolor or texels, not both")
    if texel_mips is not None and texels is not None and (texels.dim() != 3 or texels.shape[1] != (texel_mips.R + 1) * (texel_mips.R + 2) // 2):
        raise ValueError("mesh_raster: texel_mips of resolution %d were not built from texels %s" % (texel_mips.R, tuple(texels.shape)))
    verts, pose = _f32(verts, "verts"), _f32(pose, "pose")
    if pose.dim() == 2:
        pose = pose[None]
    B = pose.shape[0]
    intr = _intr_per_view("mesh_raster", intr, B)
    faces = faces.to(device=verts.device, dtype=torch.int32).contiguous()
    V, F = verts.shape[0], faces.shape[0]
    if verts.shape != (V, 3) or faces.shape != (F, 3) or pose.shape != (B, 3, 4):
        raise ValueError("mesh_raster: verts [V,3], faces [F,3], pose [B,3,4], intr [B,3,3] expected")
    if F == 0 or V == 0:
        raise ValueError("mesh_raster: empty mesh")
    dev = verts.device
    a = _lib.MeshRasterArgs()
    a.verts, a.faces, a.pose, a.intr = verts.data_ptr(), faces.data_ptr(), pose.data_ptr(), intr.data_ptr()
    a.B, a.H, a.W, a.V, a.F = B, H, W, V, F
    out = {"zbuf": torch.empty(B, H, W, device=dev) if zbuf_out is None else _want_gpu("mesh_raster", zbuf_out, "zbuf_out", torch.float32, (B, H, W))}
    if face_ids or texels is not None or texel_mips is not None:
        out["face"] = torch.empty(B, H, W, device=dev, dtype=torch.int32)
    if vcolor is not None:
        vcolor = _f32(vcolor, "vcolor")
        if vcolor.shape != (V, 3):
            raise ValueError("mesh_raster: vcolor [V,3] expected")
        a.vcolor = vcolor.data_ptr()
        out["rgb"] = torch.empty(B, H, W, 3, device=dev)
    if nocs_norm is not None:
        a.nocs_center, a.nocs_scale = _float3(nocs_norm[0]), _float3(nocs_norm[1])
        out["nocs"] = torch.empty(B, H, W, 3, device=dev)
    if normals:
        out["normal"] = torch.empty(B, H, W, 3, device=dev)
    lib = _lib.load()
    need = lib.tp_mesh_raster_culled_workspace_bytes(B, H, W, F) if cull else lib.tp_mesh_raster_workspace_bytes(B, H, W, F)
    ws = torch.empty(max(1, int(need) // 4), device=dev)
    a.zbuf, a.face, a.rgb = out["zbuf"].data_ptr(), _ptr(out.get("face")), _ptr(out.get("rgb"))
    a.nocs, a.normal, a.workspace = _ptr(out.get("nocs")), _ptr(out.get("normal")), ws.data_ptr()
    if cull:
        _call("tp_mesh_raster_culled", a)
    else:
        _call("tp_mesh_raster", a)
    if texel_mips is not None:
        out["rgb"] = face_texel_shade_mip(out["face"], verts, faces, texel_mips, pose, intr)
    elif texels is not None:
        out["rgb"] = face_texel_shade(out["face"], verts, faces, texels, pose, intr)
    return out


@_on_tensor_device
def normals_from_depth(depth: Tensor, pose: Tensor, intr: Tensor) -> Tensor:
    """The normal stage of tp_mesh_raster alone (compute_surfelinfo.normal_from_depth) on a given depth [B,H,W] (mm, <= 0 background),
    pose [B,3,4] (t in mm), intr [B,3,3] -> normal [B,H,W,3]."""
    depth = _f32(depth, "depth")
    B, H, W = depth.shape
    pose, intr = _poses("normals_from_depth", pose, "pose", B), _intr_per_view("normals_from_depth", intr, B, allow_single=False)
    normal = torch.empty(B, H, W, 3, device=depth.device)
    a = _lib.MeshRasterArgs()
    a.pose, a.intr, a.zbuf, a.normal = pose.data_ptr(), intr.data_ptr(), depth.data_ptr(), normal.data_ptr()
    a.B, a.H, a.W, a.normals_from_zbuf = B, H, W, 1
    _call("tp_mesh_raster", a)
    return normal


# ------------------------------------------------------------------------------------------ K20
SURFEL_FINISH_KEYS = ("image_syn", "mask_syn", "nocs_pred", "normal_pred")


@_on_tensor_device
def surfel_finish(zbuf: Tensor, nocs: Tensor, normal: Tensor, rgb: Optional[Tensor] = None, *, quantize: bool = True,
                  out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """The data layer's decode of the surfel files, applied to mesh_raster's outputs (tp_surfel_finish): zbuf [B,H,W], nocs / normal /
    rgb [B,H,W,3] (``rgb`` None: image_syn zero) -> image_syn [B,3,H,W] (8-bit round trip), mask_syn [B,H,W] (zbuf > 0), nocs_pred
    (8-bit round trip + smooth_geo) and normal_pred (smooth_geo) [B,3,H,W].  ``quantize=False`` skips the 8-bit round trip.
    ``out``: the four tensors to write into (float32, contiguous, of those shapes) instead of fresh ones."""
    zbuf, nocs, normal = _f32(zbuf, "zbuf"), _f32(nocs, "nocs"), _f32(normal, "normal")
    if zbuf.dim() != 3:
        raise ValueError("surfel_finish: zbuf [B,H,W] expected")
    B, H, W = zbuf.shape
    if rgb is not None:
        rgb = _f32(rgb, "rgb")
    for name, t in (("nocs", nocs), ("normal", normal), ("rgb", rgb)):
        if t is not None and t.shape != (B, H, W, 3):
            raise ValueError(f"surfel_finish: {name} [B,H,W,3] expected")
    res = _outputs("surfel_finish", out, {k: (torch.float32, (B, H, W) if k == "mask_syn" else (B, 3, H, W)) for k in SURFEL_FINISH_KEYS}, zbuf.device)
    a = _lib.SurfelFinishArgs()
    a.rgb, a.nocs, a.normal, a.zbuf = _ptr(rgb), nocs.data_ptr(), normal.data_ptr(), zbuf.data_ptr()
    a.B, a.H, a.W, a.quantize = B, H, W, int(bool(quantize))
    a.image_syn, a.mask_syn = res["image_syn"].data_ptr(), res["mask_syn"].data_ptr()
    a.nocs_pred, a.normal_pred = res["nocs_pred"].data_ptr(), res["normal_pred"].data_ptr()
    _call("tp_surfel_finish", a)
    return res


# ------------------------------------------------------------------------------------------ K21
SCENE_SOURCES = {"box": _lib.SCENE_BOX, "render": _lib.SCENE_RENDER, "none": _lib.SCENE_NONE}          # options nerf.depth.range_source -> TP_SCENE_*
SCENE_BOUNDS_KEYS = ("z_near", "z_far", "label", "depth")


@_on_tensor_device
def scene_bounds(zbuf: Tensor, boxes: Tensor, ids: Tensor, *, depth_scale: float, bg_range: Tuple[float, float], source: str = "box",
                 pose: Optional[Tensor] = None, intr: Optional[Tensor] = None, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """The z-buffer blend of K objects at B poses (tp_scene_bounds): zbuf [K,B,H,W] (mesh_raster's planes: mm, <= 0 on background),
    boxes [K,2,3] (min, max in NeRF units: bb_mm * depth_scale / 1000), ids [K] int32 (> 0), pose [B,3,4] (t in NeRF units) and intr
    [B,3,3] (needed by ``source`` 'box' only) -> z_near, z_far [B,H*W] float32, label [B,H*W] int32 (the nearest object's id, 0 where
    nothing is covered), depth [B,H*W] (the nearest mesh depth in NeRF units, 0 where uncovered).  ``source`` 'box': the winner's slab
    bounds on the pixel ray (0 where the slab test fails), 'render': 0.8 x / 1.2 x depth, 'none': ``bg_range`` everywhere; uncovered
    pixels always get ``bg_range``.  Inputs are taken as they are (float32 / int32, contiguous, on one GPU) -- nothing is converted or
    copied; ``out``: the four tensors to write into.  One launch, no allocation beyond fresh outputs, safe under torch.cuda.graph."""
    if source not in SCENE_SOURCES:
        raise ValueError(f"scene_bounds: source must be one of {sorted(SCENE_SOURCES)}, not {source!r}")
    _want_gpu("scene_bounds", zbuf, "zbuf", torch.float32, None)
    if zbuf.dim() != 4:
        raise ValueError("scene_bounds: zbuf [K,B,H,W] expected")
    K, B, H, W = zbuf.shape
    _want_gpu("scene_bounds", ids, "ids", torch.int32, (K,))
    a = _lib.SceneBoundsArgs()
    if source == "box":
        _want_gpu("scene_bounds", boxes, "boxes", torch.float32, (K, 2, 3))
        _want_gpu("scene_bounds", pose, "pose", torch.float32, (B, 3, 4))
        _want_gpu("scene_bounds", intr, "intr", torch.float32, (B, 3, 3))
        a.boxes, a.pose, a.intr = boxes.data_ptr(), pose.data_ptr(), intr.data_ptr()
    res = _outputs("scene_bounds", out, {k: (torch.int32 if k == "label" else torch.float32, (B, H * W)) for k in SCENE_BOUNDS_KEYS}, zbuf.device)
    a.zbuf, a.ids = zbuf.data_ptr(), ids.data_ptr()
    a.B, a.H, a.W, a.K, a.source = B, H, W, K, SCENE_SOURCES[source]
    a.depth_scale, a.bg_near, a.bg_far = float(depth_scale), float(bg_range[0]), float(bg_range[1])
    a.z_near, a.z_far, a.label, a.depth = (res[k].data_ptr() for k in SCENE_BOUNDS_KEYS)
    _call("tp_scene_bounds", a)
    return res


# ------------------------------------------------------------------------------------------ K22
SCENE_INFO_KEYS = ("px_count_all", "px_count_visib", "obj_xmin", "obj_ymin", "obj_xmax", "obj_ymax", "visib_xmin", "visib_ymin",
                   "visib_xmax", "visib_ymax")                      # the ten columns of info, in order
assert len(SCENE_INFO_KEYS) == _lib.SCENE_INFO_FIELDS


@_on_tensor_device
def scene_annotate(zbuf: Tensor, label: Tensor, ids: Tensor, *, masks: bool = True, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """The per-object annotations of K objects at B poses (tp_scene_annotate): zbuf [K,B,H,W] (mesh_raster's planes: mm, <= 0 or NaN on
    background), label [B,H*W] int32 (scene_bounds' label), ids [K] int32 -> info [B,K,10] int32 (columns: SCENE_INFO_KEYS; extents
    are inclusive pixel indices, -1 for an empty set) and, with ``masks``, mask and mask_visib [B,K,H,W] uint8 (0 / 255: the full
    silhouette inside the image and the part that ``label`` gives to the object).  The ids must be distinct: a wrapper that builds
    them (SceneBounds) checks that on the host; here they are taken as they are, like every input -- nothing is converted, copied or
    read back.  ``out``: the tensors to write into ('info', and 'mask' / 'mask_visib' when ``masks``); info needs no clearing.
    No allocation beyond fresh outputs, safe under torch.cuda.graph."""
    _want_gpu("scene_annotate", zbuf, "zbuf", torch.float32, None)
    if zbuf.dim() != 4:
        raise ValueError("scene_annotate: zbuf [K,B,H,W] expected")
    K, B, H, W = zbuf.shape
    _want_gpu("scene_annotate", label, "label", torch.int32, (B, H * W))
    _want_gpu("scene_annotate", ids, "ids", torch.int32, (K,))
    spec = {"info": (torch.int32, (B, K, _lib.SCENE_INFO_FIELDS))}
    if masks:
        spec.update(mask=(torch.uint8, (B, K, H, W)), mask_visib=(torch.uint8, (B, K, H, W)))
    res = _outputs("scene_annotate", out, spec, zbuf.device)
    a = _lib.SceneAnnotateArgs()
    a.zbuf, a.label, a.ids = zbuf.data_ptr(), label.data_ptr(), ids.data_ptr()
    a.B, a.H, a.W, a.K = B, H, W, K
    a.info = res["info"].data_ptr()
    if masks:
        a.mask, a.mask_visib = res["mask"].data_ptr(), res["mask_visib"].data_ptr()
    _call("tp_scene_annotate", a)
    return res


@_on_tensor_device
def view_images(rgb: Optional[Tensor], depth: Optional[Tensor], *, H: int, W: int, depth_scale: float = 1.0, png_per_metre: float = 2000.0,
                out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """The files' pixels of rendered views (tp_view_images): rgb [B,H*W,3] -> rgb8 [B,H,W,3] uint8 = trunc(clamp(rgb, 0, 1) * 255);
    depth [B,H*W] or [B,H*W,1] in NeRF units -> depth16 [B,H,W] uint16 = trunc(clamp((depth / depth_scale) * png_per_metre, 0, 65535));
    NaN gives 0.  Either input may be None (its output is then absent).  ``out``: 'rgb8' / 'depth16' tensors to write into."""
    if rgb is None and depth is None:
        raise ValueError("view_images: rgb or depth expected")
    first = rgb if rgb is not None else depth
    _want_gpu("view_images", first, "rgb" if rgb is not None else "depth", torch.float32, None)
    B, HW = int(first.shape[0]), int(H) * int(W)
    a = _lib.ViewImagesArgs()
    a.B, a.H, a.W, a.depth_scale, a.png_per_metre = B, int(H), int(W), float(depth_scale), float(png_per_metre)
    spec = {}
    if rgb is not None:
        _want_gpu("view_images", rgb, "rgb", torch.float32, (B, HW, 3))
        spec["rgb8"] = (torch.uint8, (B, H, W, 3))
    if depth is not None:
        if depth.dim() == 3 and depth.shape[-1] == 1:
            depth = depth[..., 0]
        _want_gpu("view_images", depth, "depth", torch.float32, (B, HW))
        spec["depth16"] = (torch.uint16, (B, H, W))
    res = _outputs("view_images", out, spec, first.device)
    a.rgb, a.rgb8, a.depth, a.depth16 = _ptr(rgb), _ptr(res.get("rgb8")), _ptr(depth), _ptr(res.get("depth16"))
    _call("tp_view_images", a)
    return res


# ------------------------------------------------------------------------------------------ K27
def texture_bake_workspace(V: int, B: int, device) -> Tensor:
    """A workspace for texture_bake at V vertices and B views (tp_texture_bake_workspace_bytes); needs no clearing."""
    return _workspace_arg("texture_bake", None, int(_lib.load().tp_texture_bake_workspace_bytes(V, B)), device)


@_on_tensor_device
def texture_bake(verts: Tensor, normals: Tensor, pose: Tensor, intr: Tensor, rgb: Tensor, zbuf: Tensor, weight: Optional[Tensor] = None, *,
                 acc: Optional[Tensor] = None, count: Optional[Tensor] = None, clear: bool = True, cos_min: float = 0.3,
                 cover_min: float = 0.5, z_tol_mm: float = 0.5, slope: float = 2.0, workspace: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """Project B posed images onto the V vertices of a mesh (tp_texture_bake; the rules are in the header): verts, normals [V,3]
    (model frame, mm; unit normals), pose [B,3,4] (model -> camera, mm), intr [B,3,3] or one [3,3], rgb [B,H,W,3], zbuf [B,H,W]
    (mesh_raster's plane), weight [B,H,W] or None -> 'acc' [V,4] float32 (sums of w r, w g, w b, w) and 'count' [V] int32.  ``acc`` /
    ``count``: the tensors to write into; with ``clear=False`` the call adds to what they hold, so views can be streamed in chunks.
    ``workspace``: texture_bake_workspace(V, B) (a fresh one otherwise).  Not differentiable.  Two launches, no atomics, safe under
    torch.cuda.graph."""
    verts, pose = _points("texture_bake", verts, "verts"), _poses("texture_bake", pose, "pose")
    V, B = verts.shape[0], pose.shape[0]
    normals = _points("texture_bake", normals, "normals", V)
    rgb, zbuf = _f32(rgb.detach(), "rgb"), _f32(zbuf.detach(), "zbuf")
    if zbuf.dim() != 3 or zbuf.shape[0] != B or zbuf.numel() == 0 or tuple(rgb.shape) != tuple(zbuf.shape) + (3,):
        raise ValueError("texture_bake: zbuf [B=%d,H,W] and rgb [B,H,W,3] expected, got %s and %s" % (B, tuple(zbuf.shape), tuple(rgb.shape)))
    H, W = zbuf.shape[1:]
    intr = _intr_per_view("texture_bake", intr, B)
    if weight is not None:
        weight = _f32(weight.detach(), "weight")
        if weight.numel() != B * H * W:
            raise ValueError("texture_bake: weight [B=%d,H=%d,W=%d] expected, got %s" % (B, H, W, tuple(weight.shape)))
    if (acc is None) != (count is None) or (acc is None and not clear):
        raise ValueError("texture_bake: acc and count come together, and clear=False needs both")
    dev = verts.device
    acc = torch.empty(V, 4, device=dev) if acc is None else _want_gpu("texture_bake", acc, "acc", torch.float32, (V, 4))
    count = torch.empty(V, device=dev, dtype=torch.int32) if count is None else _want_gpu("texture_bake", count, "count", torch.int32, (V,))
    workspace = _workspace_arg("texture_bake", workspace, int(_lib.load().tp_texture_bake_workspace_bytes(V, B)), dev)
    a = _lib.TextureBakeArgs()
    a.verts, a.normals, a.pose, a.intr = verts.data_ptr(), normals.data_ptr(), pose.data_ptr(), intr.data_ptr()
    a.rgb, a.zbuf, a.weight = rgb.data_ptr(), zbuf.data_ptr(), _ptr(weight)
    a.V, a.B, a.H, a.W, a.clear = V, B, H, W, int(bool(clear))
    a.cos_min, a.cover_min, a.z_tol_mm, a.slope = float(cos_min), float(cover_min), float(z_tol_mm), float(slope)
    a.acc, a.count, a.workspace = acc.data_ptr(), count.data_ptr(), workspace.data_ptr()
    _call("tp_texture_bake", a)        # (thresholds out of range: the library's error)
    return {"acc": acc, "count": count}


# ------------------------------------------------------------------------------------------ K35
@_on_tensor_device
def face_texel_shade(face: Tensor, verts: Tensor, faces: Tensor, texels: Tensor, pose: Tensor, intr: Tensor, *,
                     out: Optional[Tensor] = None) -> Tensor:
    """Colour mesh_raster's face plane from a per-face texel texture (tp_face_texel_shade; the rule is in the header): face [B,H,W]
    int32 (taken as it is), verts [V,3], faces [F,3], texels [F,T,3] with T = (R + 1)(R + 2) / 2 for a resolution R in 1 .. 64 (R is
    inferred from T), pose [B,3,4] and intr [B,3,3] or [3,3] as the rasteriser got them -> rgb [B,H,W,3] float32, zero where the
    plane holds no face.  ``out``: the tensor to write into.  Not differentiable (texels are detached): the differentiable routes are
    autograd_ops.face_texel_shade (per-slot texels) and face_texels.shade_nodes (shared nodes), both through face_texel_shade_bwd.  One
    launch, no workspace, bit-identical from run to run, safe under torch.cuda.graph."""
    op = "face_texel_shade"
    _want_gpu(op, face, "face", torch.int32, None)
    if face.dim() != 3 or face.numel() == 0:
        raise ValueError("%s: face [B,H,W] expected, got %s" % (op, tuple(face.shape)))
    B, H, W = face.shape
    verts, pose = _points(op, verts, "verts"), _poses(op, pose, "pose", B)
    intr = _intr_per_view(op, intr, B)
    faces = faces.to(device=verts.device, dtype=torch.int32).contiguous()
    texels = _f32(texels.detach(), "texels")
    V, F = verts.shape[0], faces.shape[0]
    T = texels.shape[1] if texels.dim() == 3 else 0
    R = (math.isqrt(8 * T + 1) - 3) // 2
    if tuple(faces.shape) != (F, 3) or F == 0 or tuple(texels.shape) != (F, T, 3) or _lib.load().tp_face_texel_count(R) != T:
        raise ValueError("%s: faces [F,3] and texels [F,T,3] with T = (R + 1)(R + 2) / 2, R in 1 .. %d, expected, got %s and %s"
                         % (op, _lib.FACE_TEXEL_MAX_R, tuple(faces.shape), tuple(texels.shape)))
    rgb = torch.empty(B, H, W, 3, device=face.device) if out is None else _want_gpu(op, out, "out", torch.float32, (B, H, W, 3))
    a = _lib.FaceTexelShadeArgs()
    a.verts, a.faces, a.texels, a.pose, a.intr, a.face = (t.data_ptr() for t in (verts, faces, texels, pose, intr, face))
    a.B, a.H, a.W, a.V, a.F, a.R, a.rgb = B, H, W, V, F, R, rgb.data_ptr()
    _call("tp_face_texel_shade", a)
    return rgb


# ------------------------------------------------------------------------------------------ K36
@_on_tensor_device
def face_texel_shade_bwd(face: Tensor, verts: Tensor, faces: Tensor, grad_rgb: Tensor, pose: Tensor, intr: Tensor, *, R: int,
                         node_index: Optional[Tensor] = None, U: Optional[int] = None, weight: bool = False, out: Optional[Tensor] = None):
    """The adjoint of face_texel_shade with respect to the texels (tp_face_texel_shade_bwd; the rule and the fixed-point scheme are in
    the header): face [B,H,W] int32 (taken as it is), verts, faces, pose, intr as face_texel_shade got them, grad_rgb [B,H,W,3] ->
    grad [F,T(R),3] float32, or, with ``node_index`` [F,T] (any integer type; the row of each slot, e.g. face_texels.subdivide's) and
    ``U``, grad [U,3] summed over the slots of each node (entries outside 0 .. U-1 are skipped).  ``weight=True``: returns (grad,
    weight) with weight [F,T] or [U], the same sum for grad_rgb = 1 (the coverage).  ``out``: the grad tensor to write into.  Pixels
    with a non-finite grad_rgb contribute nothing.  64-bit fixed-point integer atomics: bit-identical from run to run and under
    torch.cuda.graph; B H W <= 2^25.  The workspace (8 bytes per output value) is a torch allocation owned by the call."""
    op = "face_texel_shade_bwd"
    _want_gpu(op, face, "face", torch.int32, None)
    if face.dim() != 3 or face.numel() == 0:
        raise ValueError("%s: face [B,H,W] expected, got %s" % (op, tuple(face.shape)))
    B, H, W = face.shape
    verts, pose = _points(op, verts, "verts"), _poses(op, pose, "pose", B)
    intr = _intr_per_view(op, intr, B)
    faces = faces.to(device=verts.device, dtype=torch.int32).contiguous()
    V, F = verts.shape[0], faces.shape[0]
    lib = _lib.load()
    T = lib.tp_face_texel_count(int(R))
    if tuple(faces.shape) != (F, 3) or F == 0 or T == 0:
        raise ValueError("%s: faces [F,3] and R in 1 .. %d expected, got %s and R = %r" % (op, _lib.FACE_TEXEL_MAX_R, tuple(faces.shape), R))
    if not torch.is_tensor(grad_rgb) or not grad_rgb.is_cuda or not grad_rgb.is_floating_point() or tuple(grad_rgb.shape) != (B, H, W, 3):
        raise ValueError("%s: grad_rgb must be a floating-point GPU tensor of shape %s" % (op, (B, H, W, 3)))
    grad_rgb = _f32(grad_rgb.detach(), "grad_rgb")
    if node_index is None:
        if U is not None:
            raise ValueError("%s: U comes with node_index" % op)
        N, shape, wshape = F * T, (F, T, 3), (F, T)
    else:
        if (not torch.is_tensor(node_index) or node_index.is_floating_point() or node_index.dtype == torch.bool
                or tuple(node_index.shape) != (F, T) or U is None or int(U) <= 0):
            raise ValueError("%s: node_index must be an integer tensor of shape %s, with U > 0 destinations" % (op, (F, T)))
        node_index = node_index.to(device=verts.device, dtype=torch.int32).contiguous()
        N, shape, wshape = int(U), (int(U), 3), (int(U),)
    need = int(lib.tp_face_texel_shade_bwd_workspace(N, int(bool(weight))))
    if need == 0 or B * H * W > 1 << 25:
        raise ValueError("%s: B * H * W <= 2^25 and fewer than 2^31 / 3 destinations expected, got %d pixels and %d destinations" % (op, B * H * W, N))
    dev = face.device
    grad = torch.empty(shape, device=dev) if out is None else _want_gpu(op, out, "out", torch.float32, shape)
    wsum = torch.empty(wshape, device=dev) if weight else None
    ws = torch.empty(need // 8, device=dev, dtype=torch.int64)
    a = _lib.FaceTexelShadeBwdArgs()
    a.verts, a.faces, a.pose, a.intr, a.face, a.grad_rgb = (t.data_ptr() for t in (verts, faces, pose, intr, face, grad_rgb))
    a.node_index = _ptr(node_index)
    a.B, a.H, a.W, a.V, a.F, a.R, a.U = B, H, W, V, F, int(R), (0 if node_index is None else N)
    a.workspace, a.grad, a.weight = ws.data_ptr(), grad.data_ptr(), _ptr(wsum)
    _call("tp_face_texel_shade_bwd", a)
    return (grad, wsum) if weight else grad


# ------------------------------------------------------------------------------------------ K41
def face_texel_light_workspace(B: int, H: int, W: int, device) -> Tensor:
    """A workspace for face_texel_light(sums=True) at B images of H x W (tp_face_texel_light_workspace_bytes); needs no clearing."""
    return _workspace_arg("face_texel_light", None, int(_lib.load().tp_face_texel_light_workspace_bytes(B, H, W)), device)


@_on_tensor_device
def face_texel_light(face: Tensor, verts: Tensor, faces: Tensor, colour: Tensor, pose: Tensor, light: Tensor, *, image: Optional[Tensor] = None,
                     weight: Optional[Tensor] = None, diag: bool = False, sums: bool = False, workspace: Optional[Tensor] = None,
                     out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """The per-pixel step between face_texel_shade and face_texel_shade_bwd when the texels are an albedo under one first-order SH light
    per view (tp_face_texel_light, K41; the rule is in the header): face [B,H,W] int32 (taken as it is), verts [V,3], faces [F,3] int32,
    colour [B,H,W,3] (face_texel_shade of the node colours, or of a search direction), pose [B,3,4], light [B,3,5] (per channel l0, l1,
    l2, l3, beta, as photo_lighting returns it), ``weight`` [B,H,W] m (None: 1).  With s the shading of photo_lighting's apply:
    ``image`` [B,H,W,3] given (residual mode): 'grad' = m s (image - (s colour + beta)); ``image`` None (operator mode): 'grad' = m s
    (s colour).  ``diag``: also 'diag' = m s s, all [B,H,W,3] float32.  ``sums`` (residual mode): 'sums' [B,2] float64, sum m |image -
    (s colour + beta)|^2 and sum m per image.  A pixel without a face in [0, F), with m not finite or <= 0, or with a non-finite colour or
    image value gets zeros and adds nothing.  ``workspace``: face_texel_light_workspace(B, H, W), used with ``sums``; ``out``: any of these
    tensors to write into.  One launch (two with ``sums``), no atomics, bit-identical from run to run, safe under torch.cuda.graph."""
    op = "face_texel_light"
    _want_gpu(op, face, "face", torch.int32, None)
    if face.dim() != 3 or face.numel() == 0:
        raise ValueError("%s: face [B,H,W] expected, got %s" % (op, tuple(face.shape)))
    B, H, W = face.shape
    verts = _points(op, verts, "verts")
    faces = _want_gpu(op, faces, "faces", torch.int32, None)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] == 0:
        raise ValueError("%s: faces [F,3] expected, got %s" % (op, tuple(faces.shape)))
    colour = _want_gpu(op, colour, "colour", torch.float32, (B, H, W, 3))
    pose = _poses(op, pose, "pose", B)
    light = _want_gpu(op, light, "light", torch.float32, (B, 3, 5))
    image = None if image is None else _want_gpu(op, image, "image", torch.float32, (B, H, W, 3))
    weight = None if weight is None else _want_gpu(op, weight, "weight", torch.float32, (B, H, W))
    if sums and image is None:
        raise ValueError("%s: sums=True needs image (residual mode)" % op)
    spec = {"grad": (torch.float32, (B, H, W, 3))}
    if diag:
        spec["diag"] = (torch.float32, (B, H, W, 3))
    if sums:
        spec["sums"] = (torch.float64, (B, 2))
    res = _outputs(op, out, spec, face.device, partial=True)
    a = _lib.FaceTexelLightArgs()
    a.verts, a.faces, a.face, a.pose, a.light, a.colour = (t.data_ptr() for t in (verts, faces, face, pose, light, colour))
    a.image, a.weight = _ptr(image), _ptr(weight)
    a.V, a.F, a.B, a.H, a.W = verts.shape[0], faces.shape[0], B, H, W
    a.grad, a.diag, a.sums = res["grad"].data_ptr(), _ptr(res.get("diag")), _ptr(res.get("sums"))
    if sums:
        workspace = _workspace_arg(op, workspace, int(_lib.load().tp_face_texel_light_workspace_bytes(B, H, W)), face.device, align=8)
        a.workspace = workspace.data_ptr()
    _call("tp_face_texel_light", a)       # (outputs overlapping inputs or each other: the library's error)
    return res


# ------------------------------------------------------------------------------------------ K42
ROBUST_KINDS = {"tukey": (_lib.ROBUST_TUKEY, 4.685), "huber": (_lib.ROBUST_HUBER, 1.345)}      # name -> (the header's constant, the default c)


def robust_weight_workspace(B: int, H: int, W: int, device) -> Tensor:
    """A workspace for robust_weight at B images of H x W (tp_robust_weight_workspace_bytes); needs no clearing."""
    return _workspace_arg("robust_weight", None, int(_lib.load().tp_robust_weight_workspace_bytes(B, H, W)), device)


@_on_tensor_device
def robust_weight(model: Tensor, image: Tensor, *, weight: Optional[Tensor] = None, kind: str = "tukey", c: Optional[float] = None,
                  sigma_min: float = 1.0 / 255.0, scale_in: Optional[Tensor] = None, workspace: Optional[Tensor] = None,
                  out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
    """The weights of one round of iteratively reweighted least squares on a photometric residual (tp_robust_weight, K42; the rule is in
    the header): model and image [B,H,W,3] float32, ``weight`` [B,H,W] the base weight (None: 1).  Per pixel q = mean over the channels
    of (image - model)^2; per image sigma = max(1.4826 sqrt(median q), ``sigma_min``), the median being the exact lower median over the
    pixels that count (base weight finite and > 0, every colour finite) -- or ``scale_in`` [B] where given, and no median is taken;
    u^2 = q / (c sigma)^2; ``kind`` 'tukey': (1 - u^2)^2 inside u < 1, 0 outside; 'huber': 1 inside, 1 / u outside; ``c`` None: 4.685 and
    1.345.  Returns 'weight' [B,H,W] float32 (base x robust; 0 where the pixel does not count), 'median_q' [B], 'scale' [B] (sigma) float32
    and 'count' [B] int32.  ``workspace``: robust_weight_workspace(B, H, W), used without ``scale_in``; ``out``: any of these tensors to
    write into.  Integer atomics only: bit-identical from run to run; nothing is read back; safe under torch.cuda.graph."""
    op = "robust_weight"
    if kind not in ROBUST_KINDS:
        raise ValueError("%s: kind %r is none of %s" % (op, kind, sorted(ROBUST_KINDS)))
    _want_gpu(op, model, "model", torch.float32, None)
    if model.dim() != 4 or model.shape[3] != 3 or model.numel() == 0:
        raise ValueError("%s: model [B,H,W,3] expected, got %s" % (op, tuple(model.shape)))
    B, H, W = model.shape[:3]
    image = _want_gpu(op, image, "image", torch.float32, (B, H, W, 3))
    weight = None if weight is None else _want_gpu(op, weight, "weight", torch.float32, (B, H, W))
    scale_in = None if scale_in is None else _want_gpu(op, scale_in, "scale_in", torch.float32, (B,))
    res = _outputs(op, out, {"weight": (torch.float32, (B, H, W)), "median_q": (torch.float32, (B,)), "scale": (torch.float32, (B,)),
                             "count": (torch.int32, (B,))}, model.device, partial=True)
    a = _lib.RobustWeightArgs()
    a.model, a.image, a.weight, a.scale_in = model.data_ptr(), image.data_ptr(), _ptr(weight), _ptr(scale_in)
    a.B, a.H, a.W, a.kind = B, H, W, ROBUST_KINDS[kind][0]
    a.c, a.sigma_min = float(ROBUST_KINDS[kind][1] if c is None else c), float(sigma_min)
    a.out, a.median_q, a.scale, a.count = (res[k].data_ptr() for k in ("weight", "median_q", "scale", "count"))
    if scale_in is None:
        workspace = _workspace_arg(op, workspace, int(_lib.load().tp_robust_weight_workspace_bytes(B, H, W)), model.device, align=16)
        a.workspace = workspace.data_ptr()
    _call("tp_robust_weight", a)          # (bad c or sigma_min, outputs overlapping inputs or each other: the library's error)
    return res


# ------------------------------------------------------------------------------------------ K43
@_on_tensor_device
def face_texel_mip_reduce(texels: Tensor, slot_ptr: Tensor, slot_list: Tensor, *, out: Optional[Tensor] = None) -> Tensor:
    """One mip level down (tp_face_texel_mip_reduce, K43a; the rule is in the header): texels [F,T(Rf),3] with Rf even, the CSR pair
    of the COARSE grid's unique nodes (face_texels.mip_slots(verts, faces, Rf // 2): slot_ptr [U+1], slot_list [F T(Rf/2)], any
    integer type) -> [F,T(Rf/2),3] float32.  ``out``: the tensor to write into (e.g. a level of the packed chain).  One memset and
    one launch, no workspace, bit-identical from run to run, safe under torch.cuda.graph."""
    op = "face_texel_mip_reduce"
    if not torch.is_tensor(texels) or not texels.is_cuda:
        raise ValueError("%s: texels must be a GPU tensor" % op)
    texels = _f32(texels.detach(), "texels")
    F, Tf = (texels.shape[0], texels.shape[1]) if texels.dim() == 3 else (0, 0)
    Rf = (math.isqrt(8 * Tf + 1) - 3) // 2
    lib = _lib.load()
    if F == 0 or tuple(texels.shape) != (F, Tf, 3) or lib.tp_face_texel_count(Rf) != Tf or Rf % 2:
        raise ValueError("%s: texels [F,T,3] with T = (R + 1)(R + 2) / 2 for an even R in 2 .. %d expected, got %s"
                         % (op, _lib.FACE_TEXEL_MAX_R, tuple(texels.shape)))
    Tc = int(lib.tp_face_texel_count(Rf // 2))
    for t, name in ((slot_ptr, "slot_ptr"), (slot_list, "slot_list")):
        if not torch.is_tensor(t) or t.is_floating_point() or t.dtype == torch.bool or t.dim() != 1:
            raise ValueError("%s: %s must be a one-dimensional integer tensor" % (op, name))
    if slot_ptr.numel() < 2 or slot_list.numel() != F * Tc:
        raise ValueError("%s: slot_ptr [U+1] and slot_list [F T(R/2) = %d] expected, got %d and %d entries"
                         % (op, F * Tc, slot_ptr.numel(), slot_list.numel()))
    slot_ptr = slot_ptr.to(device=texels.device, dtype=torch.int32).contiguous()
    slot_list = slot_list.to(device=texels.device, dtype=torch.int32).contiguous()
    coarse = torch.empty(F, Tc, 3, device=texels.device) if out is None else _want_gpu(op, out, "out", torch.float32, (F, Tc, 3))
    a = _lib.FaceTexelMipReduceArgs()
    a.fine, a.slot_ptr, a.slot_list, a.coarse = texels.data_ptr(), slot_ptr.data_ptr(), slot_list.data_ptr(), coarse.data_ptr()
    a.F, a.Rf, a.U = F, Rf, slot_ptr.numel() - 1
    _call("tp_face_texel_mip_reduce", a)
    return coarse


@_on_tensor_device
def face_texel_shade_mip(face: Tensor, verts: Tensor, faces: Tensor, mips, pose: Tensor, intr: Tensor, *, footprint: float = 1.0,
                         out: Optional[Tensor] = None) -> Tensor:
    """face_texel_shade with a minification filter (tp_face_texel_shade_mip, K43b; the rule is in the header): ``mips`` is the chain
    face_texels.build_mips made of this mesh's texels (anything with ``packed`` -- the packed float32 levels on the device --, ``R``
    and ``L``); the other arguments are face_texel_shade's.  Per pixel the texel density d (level-0 cells per pixel, closed form) picks
    two adjacent levels and blends them; a magnified pixel (d <= 1) is face_texel_shade's pixel bit for bit.  ``footprint`` > 0
    multiplies d (an LOD bias of log2(footprint) / 2).  One launch, no workspace, bit-identical from run to run, safe under
    torch.cuda.graph.  Not differentiable."""
    op = "face_texel_shade_mip"
    _want_gpu(op, face, "face", torch.int32, None)
    if face.dim() != 3 or face.numel() == 0:
        raise ValueError("%s: face [B,H,W] expected, got %s" % (op, tuple(face.shape)))
    B, H, W = face.shape
    verts, pose = _points(op, verts, "verts"), _poses(op, pose, "pose", B)
    intr = _intr_per_view(op, intr, B)
    faces = faces.to(device=verts.device, dtype=torch.int32).contiguous()
    V, F = verts.shape[0], faces.shape[0]
    if tuple(faces.shape) != (F, 3) or F == 0:
        raise ValueError("%s: faces [F,3] expected, got %s" % (op, tuple(faces.shape)))
    packed, R, L = (getattr(mips, k, None) for k in ("packed", "R", "L"))
    if not torch.is_tensor(packed) or R is None or L is None:
        raise ValueError("%s: mips must carry packed, R and L (face_texels.build_mips)" % op)
    packed = _want_gpu(op, packed.detach(), "mips.packed", torch.float32, None)
    need = int(_lib.load().tp_face_texel_mip_elems(F, int(R), int(L)))
    if need == 0 or packed.dim() != 1 or packed.numel() != need:
        raise ValueError("%s: mips of R = %r, L = %r with %d values do not belong to a mesh of %d faces (%d values expected)"
                         % (op, R, L, packed.numel(), F, need))
    if not (math.isfinite(footprint) and footprint > 0):
        raise ValueError("%s: footprint must be finite and > 0, got %r" % (op, footprint))
    rgb = torch.empty(B, H, W, 3, device=face.device) if out is None else _want_gpu(op, out, "out", torch.float32, (B, H, W, 3))
    a = _lib.FaceTexelShadeMipArgs()
    a.verts, a.faces, a.mips, a.pose, a.intr, a.face = (t.data_ptr() for t in (verts, faces, packed, pose, intr, face))
    a.B, a.H, a.W, a.V, a.F, a.R, a.L, a.footprint, a.rgb = B, H, W, V, F, int(R), int(L), float(footprint), rgb.data_ptr()
    _call("tp_face_texel_shade_mip", a)
    return rgb
