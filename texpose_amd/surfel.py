"""Surfel maps of the adaptation loops: the synthetic RGB / mask, NOCS and normal maps that the reference renders with PyTorch3D
(compute_surfelinfo.py:60-140) and its data layer reads back (data/lm.py:196-253), rendered by the HIP rasteriser (tp_mesh_raster).

load_ply (numpy only), SurfelRenderer (one mesh, batches of predicted poses; data_layer_maps = the tensors the data layer would load,
tp_surfel_finish), SurfelMapStore (those tensors for a whole sequence, resident), write_surfel_frame / read_surfel_frame (the reference's files).
coherent_face_order: a face order that is coherent in space, for the culled rasteriser (ops.mesh_raster(cull=True)).
Conventions and what differs from PyTorch3D: DESIGN.md section 11."""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import ops
from .options import AttrDict

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _ply_header(f):
    if f.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError("PLY header without end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if tok[1] == "list":                               # ("list", count type, item type, name)
                elements[-1][2].append(("list", _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]], tok[4]))
            else:
                elements[-1][2].append(("scalar", _PLY_TYPES[tok[1]], None, tok[2]))
        elif tok[0] == "end_header":
            break
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"unsupported PLY format {fmt!r}")
    return fmt, elements


def _read_binary_element(buf: memoryview, pos: int, count: int, props, endian: str):
    """-> (dict name -> array (scalars) or list of arrays (lists), new position)."""
    if all(kind == "scalar" for kind, _, _, _ in props):
        dt = np.dtype([(name, endian + t) for _, t, _, name in props])
        rec = np.frombuffer(buf, dtype=dt, count=count, offset=pos)
        return {name: rec[name] for _, _, _, name in props}, pos + count * dt.itemsize
    # lists: try the common case of one constant length first (one structured read), else walk the records
    if count > 0:
        fields, p = [], pos
        for kind, t, it, name in props:
            if kind == "scalar":
                fields.append((name, endian + t))
                p += np.dtype(t).itemsize
            else:
                n = int(np.frombuffer(buf, dtype=endian + t, count=1, offset=p)[0])
                fields += [("__n_" + name, endian + t), (name, endian + it, (n,))]
                p += np.dtype(t).itemsize + n * np.dtype(it).itemsize
        dt = np.dtype(fields)
        if pos + count * dt.itemsize <= len(buf):
            rec = np.frombuffer(buf, dtype=dt, count=count, offset=pos)
            if all((rec["__n_" + name] == rec.dtype[name].shape[0]).all() for kind, _, _, name in props if kind == "list"):
                out = {name: (rec[name] if kind == "scalar" else rec[name].reshape(count, -1)) for kind, _, _, name in props}
                return out, pos + count * dt.itemsize
    out = {name: [] for _, _, _, name in props}
    for _ in range(count):
        for kind, t, it, name in props:
            v = np.frombuffer(buf, dtype=endian + t, count=1, offset=pos)[0]
            pos += np.dtype(t).itemsize
            if kind == "list":
                n = int(v)
                out[name].append(np.frombuffer(buf, dtype=endian + it, count=n, offset=pos))
                pos += n * np.dtype(it).itemsize
            else:
                out[name].append(v)
    for kind, _, _, name in props:
        if kind == "scalar":
            out[name] = np.asarray(out[name])
    return out, pos


def _read_ascii_element(lines, count: int, props):
    out = {name: [] for _, _, _, name in props}
    for _ in range(count):
        tok = next(lines).split()
        k = 0
        for kind, t, it, name in props:
            if kind == "list":
                n = int(tok[k])
                out[name].append(np.asarray(tok[k + 1:k + 1 + n], dtype=it))
                k += 1 + n
            else:
                out[name].append(float(tok[k]) if t[0] == "f" else int(tok[k]))
                k += 1
    for kind, t, _, name in props:
        if kind == "scalar":
            out[name] = np.asarray(out[name], dtype=t)
    return out


def _triangulate(polys) -> np.ndarray:
    """Faces from a [F,n] array or a list of index arrays: triangles as they are, polygons (quads) as fans (0, k, k+1)."""
    if isinstance(polys, np.ndarray) and polys.ndim == 2:
        n = polys.shape[1]
        if n < 3:
            return np.zeros((0, 3), dtype=np.int32)
        tris = [polys[:, [0, k, k + 1]] for k in range(1, n - 1)]
        return np.stack(tris, axis=1).reshape(-1, 3).astype(np.int32)
    tris = []
    for p in polys:
        for k in range(1, len(p) - 1):
            tris.append((p[0], p[k], p[k + 1]))
    return np.asarray(tris, dtype=np.int64).reshape(-1, 3).astype(np.int32)


def load_ply(path: str) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray]]:
    """ASCII or binary PLY (BOP `models/obj_*.ply` included) -> verts [V,3] float32, faces [F,3] int32 (quads / polygons split into
    triangles), vcolor [V,3] float32 in [0,1] (uchar colours / 255) or None.  Vertex properties are found by name; faces come from a
    `vertex_indices` / `vertex_index` list."""
    with open(path, "rb") as f:
        fmt, elements = _ply_header(f)
        body = f.read()
    data = {}
    if fmt == "ascii":
        lines = iter(ln for ln in body.decode("ascii").splitlines() if ln.strip())
        for name, count, props in elements:
            data[name] = _read_ascii_element(lines, count, props)
    else:
        endian = "<" if fmt == "binary_little_endian" else ">"
        buf, pos = memoryview(body), 0
        for name, count, props in elements:
            data[name], pos = _read_binary_element(buf, pos, count, props, endian)
    if "vertex" not in data:
        raise ValueError(f"{path}: no vertex element")
    v = data["vertex"]
    verts = np.stack([np.asarray(v[k], dtype=np.float32) for k in ("x", "y", "z")], axis=1)
    vcolor = None
    if all(k in v for k in ("red", "green", "blue")):
        cols = [np.asarray(v[k]) for k in ("red", "green", "blue")]
        vcolor = np.stack([c.astype(np.float32) / 255.0 if c.dtype == np.uint8 else c.astype(np.float32) for c in cols], axis=1)
        vcolor = vcolor.astype(np.float32)
    faces = np.zeros((0, 3), dtype=np.int32)
    if "face" in data:
        fd = data["face"]
        key = "vertex_indices" if "vertex_indices" in fd else "vertex_index" if "vertex_index" in fd else None
        if key is None:
            raise ValueError(f"{path}: face element without vertex_indices / vertex_index")
        faces = _triangulate(fd[key])
    return verts, faces, vcolor


def nocs_normalisation(verts) -> Tuple[np.ndarray, np.ndarray]:
    """(centre, scale) per axis as SoftPhongNOCSShader computes them over all vertices (mvrenderer.py:702-708): the mean and the
    largest |v - mean|; a vertex maps to ((v - centre) / scale + 1) / 2."""
    v = torch.as_tensor(np.asarray(verts, dtype=np.float32))
    ct = v.mean(dim=0)
    return ct.numpy(), (v - ct).abs().max(dim=0).values.numpy()


def _spread_bits10(x: np.ndarray) -> np.ndarray:
    """The low 10 bits of x with two zero bits after each: bit k -> bit 3 k."""
    x = x.astype(np.uint32) & np.uint32(0x3FF)
    x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
    x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
    x = (x | (x << np.uint32(2))) & np.uint32(0x09249249)
    return x


def coherent_face_order(verts, faces) -> np.ndarray:
    """A face order that is coherent in space, for the culled rasteriser (ops.mesh_raster(cull=True)): the
    permutation ``perm`` [F] int64 that sorts the faces by the 30-bit Morton code of their centroid, quantised to 10 bits per axis over
    the largest extent of the mesh (of the vertices its faces use) (x in the highest bit of each triple), by a stable sort: faces with equal codes keep their order, and
    the result is the same on every call.  Consecutive faces of ``faces[perm]`` are then neighbours in space, so a chunk of 256 of
    them covers a small patch of the image at any pose, and a tile skips most chunks.  A face with an index outside the mesh or a
    centroid that is not finite sorts first (the rasteriser drops the first and never shows the second).

    Nothing applies it by default.  Render with ``faces[perm]``: the depth, colour, NOCS and normal planes are the same bit for bit
    (a pixel keeps the nearest face whatever the order), the ``face`` plane then indexes ``faces[perm]``, so ``perm[face]`` is the
    id in the original order (on covered pixels; where two faces tie in z exactly the smaller NEW index wins, which may be the other
    face).  ops.depth_icp reads the faces through that plane: hand it the same permuted ``faces``."""
    verts = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    valid = ((faces >= 0) & (faces < len(verts))).all(axis=1)
    centroid = verts[np.where(valid[:, None], faces, 0)].mean(axis=1) if len(verts) else np.zeros((len(faces), 3))
    valid &= np.isfinite(centroid).all(axis=1)
    code = np.zeros(len(faces), dtype=np.uint32)
    if valid.any():
        c = centroid[valid]
        used = verts[np.unique(faces[valid])]
        lo = used.min(axis=0)
        extent = float((used.max(axis=0) - lo).max())
        # relative to the lowest corner, so that a translation of the mesh changes nothing but rounding in the last place
        q = np.zeros_like(c) if extent <= 0 else np.minimum(np.floor((c - lo) * (1024.0 / extent)), 1023.0)
        q = q.astype(np.uint32)
        code[valid] = (_spread_bits10(q[:, 0]) << np.uint32(2)) | (_spread_bits10(q[:, 1]) << np.uint32(1)) | _spread_bits10(q[:, 2])
    return np.argsort(code, kind="stable").astype(np.int64)


def calibrate_pose(pose: torch.Tensor, depth_scale: float) -> torch.Tensor:
    """[B,3,4] pose in nerf.depth.scale units -> [R|t] in mm as compute_surfelinfo.py:107 and MVRenderer.calibrate_pose hand it to
    PyTorch3D: t * 1000 / depth_scale, R re-orthonormalised like the 6D round trip (Gram-Schmidt of the first two columns, third =
    their cross product; the rotation by pi about z the renderer applies before it commutes with this)."""
    pose = pose.float()
    a1, a2 = pose[:, :, 0], pose[:, :, 1]
    b1 = torch.nn.functional.normalize(a1, dim=-1)
    b2 = torch.nn.functional.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.cat([torch.stack([b1, b2, b3], dim=-1), pose[:, :, 3:] * 1000.0 / depth_scale], dim=-1).contiguous()


class SurfelRenderer:
    """The colour + NOCS renders and normals of compute_surfelinfo for one CAD mesh at batches of poses (one tp_mesh_raster call)."""

    def __init__(self, verts, faces, vcolor=None, H: int = 480, W: int = 640, device="cuda:0", cull: bool = False, texels=None,
                 texel_mips=None):
        if vcolor is not None and (texels is not None or texel_mips is not None):
            raise ValueError("SurfelRenderer: vcolor or texels, not both")
        self.device = torch.device(device)
        self.cull = bool(cull)                 # render with ops.mesh_raster(cull=True): the same bits (K34)
        self.H, self.W = int(H), int(W)
        self.nocs_center, self.nocs_scale = nocs_normalisation(verts)
        self.verts = torch.as_tensor(np.asarray(verts, dtype=np.float32)).to(self.device)
        self.faces = torch.as_tensor(np.asarray(faces, dtype=np.int32)).to(self.device)
        self.vcolor = None if vcolor is None else torch.as_tensor(np.asarray(vcolor, dtype=np.float32)).to(self.device)
        # [F,T,3] face texels (K35): rgb from ops.mesh_raster(texels=) instead of the vertex colours
        self.texels = None if texels is None else torch.as_tensor(texels, dtype=torch.float32).to(self.device).contiguous()
        # face_texels.build_mips of the texels (K43): rgb through the minification filter, over the range of depths
        self.texel_mips = texel_mips

    def _raster(self, pose, intr, depth_scale: float):
        pose = torch.as_tensor(pose, dtype=torch.float32).to(self.device)
        if pose.dim() == 2:
            pose = pose[None]
        intr = torch.as_tensor(intr, dtype=torch.float32).to(self.device)
        return ops.mesh_raster(self.verts, self.faces, calibrate_pose(pose, depth_scale), intr, H=self.H, W=self.W, vcolor=self.vcolor,
                               texels=self.texels, texel_mips=self.texel_mips, nocs_norm=(self.nocs_center, self.nocs_scale), face_ids=False, normals=True, cull=self.cull)

    def __call__(self, pose, intr, depth_scale: float) -> AttrDict:
        """pose [B,3,4] (t in nerf.depth.scale units, like pose_init), intr [B,3,3] or [3,3] ->
        rgb_syn [B,3,H,W] (zero without vertex colours), mask_syn [B,H,W], nocs [B,3,H,W], depth [B,H,W] (mm, -1 on background),
        normal [B,3,H,W].  These are the raw renders (what the files are written from), not what the trainer is fed: data_layer_maps."""
        r = self._raster(pose, intr, depth_scale)
        chw = lambda t: t.permute(0, 3, 1, 2)
        depth = r["zbuf"]
        rgb = chw(r["rgb"]) if "rgb" in r else torch.zeros(depth.shape[0], 3, self.H, self.W, device=self.device)
        return AttrDict(rgb_syn=rgb, mask_syn=(depth > 0).float(), nocs=chw(r["nocs"]), depth=depth, normal=chw(r["normal"]))

    def data_layer_maps(self, pose, intr, depth_scale: float, quantize: bool = True, out=None) -> AttrDict:
        """The four tensors the reference's data layer would load from the files write_surfel_frame writes for these poses
        (data/lm.py:196-253), bit for bit, without the files: image_syn [B,3,H,W] (8-bit round trip), mask_syn [B,H,W],
        nocs_pred [B,3,H,W] (8-bit round trip, then smooth_geo), normal_pred [B,3,H,W] (smooth_geo); plus depth [B,H,W] (mm).
        Two C calls (tp_mesh_raster, tp_surfel_finish), nothing on the host.  ``quantize=False`` keeps the fp32 colour and NOCS
        (not what the reference trains on).  ``out``: a dict of the four tensors to write into.  With ground-truth poses this is
        the `_GT` variant of the maps."""
        r = self._raster(pose, intr, depth_scale)
        m = ops.surfel_finish(r["zbuf"], r["nocs"], r["normal"], r.get("rgb"), quantize=quantize, out=out)
        return AttrDict(depth=r["zbuf"], **m)


MAP_KEYS = ops.SURFEL_FINISH_KEYS


class SurfelMapStore:
    """The surfel maps of all N training frames of a sequence, resident on the device: what the reference's data layer reads from
    rgbsyn_<loop> / nocs_<loop> / normal_<loop> for one pose loop.  Ten fp32 planes per frame (640 KB at 128x128).
    ``batch(idx)`` gathers the four keys of a training batch (``var.update(store.batch(var.idx))``); ``refresh(pose_init)``
    re-renders into the same storage for the next pose loop."""

    def __init__(self, renderer: SurfelRenderer, pose_init, intr, depth_scale: float, batch: int = 16, quantize: bool = True):
        self.renderer, self.depth_scale, self.chunk, self.quantize = renderer, float(depth_scale), max(1, int(batch)), bool(quantize)
        pose_init = torch.as_tensor(pose_init, dtype=torch.float32)
        if pose_init.dim() != 3 or pose_init.shape[1:] != (3, 4):
            raise ValueError("SurfelMapStore: pose_init [N,3,4] expected")
        N, H, W, dev = pose_init.shape[0], renderer.H, renderer.W, renderer.device
        intr = torch.as_tensor(intr, dtype=torch.float32).to(dev)
        if intr.shape not in ((3, 3), (N, 3, 3)):
            raise ValueError("SurfelMapStore: intr [N,3,3] or [3,3] expected")
        self.N, self.intr = N, intr
        self.maps = AttrDict(image_syn=torch.empty(N, 3, H, W, device=dev), mask_syn=torch.empty(N, H, W, device=dev),
                             nocs_pred=torch.empty(N, 3, H, W, device=dev), normal_pred=torch.empty(N, 3, H, W, device=dev))
        self.refresh(pose_init)

    def refresh(self, pose_init) -> None:
        """Render all N frames at ``pose_init`` [N,3,4] into the tensors the store already holds (their addresses do not change)."""
        pose_init = torch.as_tensor(pose_init, dtype=torch.float32).to(self.renderer.device)
        if pose_init.shape != (self.N, 3, 4):
            raise ValueError(f"SurfelMapStore.refresh: pose_init [{self.N},3,4] expected")
        for n0 in range(0, self.N, self.chunk):
            n1 = min(n0 + self.chunk, self.N)
            intr = self.intr if self.intr.dim() == 2 else self.intr[n0:n1]
            self.renderer.data_layer_maps(pose_init[n0:n1], intr, self.depth_scale, quantize=self.quantize,
                                          out={k: self.maps[k][n0:n1] for k in MAP_KEYS})

    def batch(self, idx) -> AttrDict:
        """image_syn, mask_syn, nocs_pred, normal_pred of the frames ``idx`` [B] (int64; ``var.idx``), gathered on the device."""
        idx = torch.as_tensor(idx, dtype=torch.int64).to(self.renderer.device)
        return AttrDict({k: self.maps[k].index_select(0, idx) for k in MAP_KEYS})


def surfel_file_name(frame_index: int, obj_scene_id: Optional[int] = None) -> str:
    """data/lm.py:201-204: `{frame:06d}` or, for the multi-object data, `{frame:06d}_{obj:06d}` (no extension)."""
    return "{:06d}".format(int(frame_index)) if obj_scene_id is None else "{:06d}_{:06d}".format(int(frame_index), int(obj_scene_id))


def write_surfel_frame(root: str, loop, frame_index: int, out: AttrDict, b: int, obj_scene_id: Optional[int] = None) -> None:
    """Image ``b`` of a SurfelRenderer result as compute_surfelinfo.py:118-140 stores it under ``root``:
    rgbsyn_<loop>/NAME.png (RGBA, (x * 255).astype(uint8), alpha 255 on covered pixels), nocs_<loop>/NAME.png (RGB = x, y, z),
    normal_<loop>/NAME.npz (data = [H,W,3] float32).  cv2 wrote the BGR-flipped arrays, so the files hold R, G, B in order."""
    from PIL import Image
    name = surfel_file_name(frame_index, obj_scene_id)
    hwc = lambda t: t[b].permute(1, 2, 0).detach().cpu().numpy().astype(np.float32)
    alpha = (out.depth[b] > 0).cpu().numpy()[..., None]
    rgba = np.concatenate([hwc(out.rgb_syn), alpha], axis=-1)
    paths = {kind: os.path.join(root, "{}_{}".format(kind, loop)) for kind in ("rgbsyn", "nocs", "normal")}
    for p in paths.values():
        os.makedirs(p, exist_ok=True)
    Image.fromarray((rgba * 255).astype(np.uint8), "RGBA").save(os.path.join(paths["rgbsyn"], name + ".png"))
    Image.fromarray((hwc(out.nocs) * 255).astype(np.uint8), "RGB").save(os.path.join(paths["nocs"], name + ".png"))
    np.savez_compressed(os.path.join(paths["normal"], name + ".npz"), data=hwc(out.normal))


def _smooth_geo(x: np.ndarray) -> np.ndarray:
    """data/lm.py:497-521 on a [H,W,3] float32 map (numpy only): pixels in the mask (channel 0 != 0) with a 4-neighbour inside the
    image outside it take the per-channel 3x3 median of the unsmoothed map, borders replicated (cv2.medianBlur(x, 3))."""
    x = np.array(x, dtype=np.float32, copy=True)
    m = x[:, :, 0] != 0
    out = np.zeros_like(m)
    out[:-1] |= ~m[1:]
    out[1:] |= ~m[:-1]
    out[:, :-1] |= ~m[:, 1:]
    out[:, 1:] |= ~m[:, :-1]
    edge = m & out
    pad = np.pad(x, ((1, 1), (1, 1), (0, 0)), mode="edge")
    i, j = np.nonzero(edge)                                   # the median of nine is needed on the silhouette only
    x[i, j] = np.median(np.stack([pad[i + di, j + dj] for di in range(3) for dj in range(3)]), axis=0).astype(np.float32)
    return x


def read_surfel_frame(root: str, loop, frame_index: int, obj_scene_id: Optional[int] = None) -> AttrDict:
    """One frame of write_surfel_frame's files as the reference's data layer loads it (data/lm.py:196-253), on the host:
    image_syn [3,H,W] (uint8 / 255), mask_syn [H,W] (alpha > 0), nocs_pred [3,H,W] (uint8 / 255, smoothed at the silhouette),
    normal_pred [3,H,W] (smoothed at the silhouette), float32 CPU tensors.  SurfelRenderer.data_layer_maps gives the same tensors
    without the files; this reader exists to check that (tools/surfel_maps.py --verify-online) and to time the file route."""
    from PIL import Image
    name = surfel_file_name(frame_index, obj_scene_id)
    rgba = np.asarray(Image.open(os.path.join(root, "rgbsyn_{}".format(loop), name + ".png")))
    nocs = np.asarray(Image.open(os.path.join(root, "nocs_{}".format(loop), name + ".png"))).astype(np.float32) / 255
    normal = np.load(os.path.join(root, "normal_{}".format(loop), name + ".npz"))["data"]
    chw = lambda a: torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))
    return AttrDict(image_syn=chw(rgba[..., :3].astype(np.float32) / 255), mask_syn=torch.from_numpy((rgba[..., 3] > 0).astype(np.float32)),
                    nocs_pred=chw(_smooth_geo(nocs)), normal_pred=chw(_smooth_geo(normal)))
