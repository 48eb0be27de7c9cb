"""Per-face texel textures ("mesh colours"): colour detail below the mesh's vertex spacing without a UV unwrap (K35).

Every face carries the barycentric grid of resolution R of include/texpose_amd.h (K35): T(R) = (R + 1)(R + 2) / 2 nodes, node (i, j) at
the weights ((R - i - j) / R, i / R, j / R) of the face's vertices in the face's own order, stored at n(i, j) = j (R + 1) - j (j - 1) / 2
+ i.  ``ops.face_texel_shade`` interpolates them per pixel of the rasteriser's face plane, so geometry and rasteriser work stay those
of the base mesh while the colour becomes R x finer along each edge.  The nodes of all faces are exactly the vertices of the mesh
subdivided R times (``subdivide``), which is how a texture is baked -- ``FaceTexelBaker`` runs the unchanged vertex bake (K27) on those
points -- and what the shading is tested against: texels on the base mesh equal vertex colours on the subdivided one.

Point sampling only (no minification filter: pick R with ``resolution_for`` so that a texel is about a pixel), one R per mesh, no UV
atlas, no gradients with respect to texels.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import ops
from .options import AttrDict
from .texture_bake import TextureBaker, mesh_edges, write_ply

MAX_R = 64


def texel_count(R: int) -> int:
    """T(R) = (R + 1)(R + 2) / 2 nodes per face; R in 1 .. 64."""
    R = int(R)
    if not 1 <= R <= MAX_R:
        raise ValueError("face_texels: R in 1 .. %d expected, got %r" % (MAX_R, R))
    return (R + 1) * (R + 2) // 2


def resolution_of(T: int) -> int:
    """The R with texel_count(R) = T."""
    R = (int(np.sqrt(8 * int(T) + 1)) - 3) // 2
    if not 1 <= R <= MAX_R or texel_count(R) != int(T):
        raise ValueError("face_texels: %r is not (R + 1)(R + 2) / 2 for an R in 1 .. %d" % (T, MAX_R))
    return R


def node_ij(R: int) -> np.ndarray:
    """(i, j) of the T(R) nodes in storage order [T,2]: row j = 0 first, i ascending within a row."""
    texel_count(R)
    return np.array([(i, j) for j in range(R + 1) for i in range(R + 1 - j)], dtype=np.int64)


def node_weights(R: int) -> np.ndarray:
    """The barycentric weights [T,3] float64 of the nodes in storage order: ((R - i - j) / R, i / R, j / R)."""
    ij = node_ij(R)
    return np.stack([R - ij[:, 0] - ij[:, 1], ij[:, 0], ij[:, 1]], axis=1) / float(R)


def resolution_for(mean_edge_mm: float, focal_px: float, distance_mm: float) -> int:
    """The R at which a texel is about one pixel: an edge of ``mean_edge_mm`` seen fronto-parallel from ``distance_mm`` with focal
    length ``focal_px`` spans mean_edge_mm * focal_px / distance_mm pixels, and R texels; rounded, within 1 .. 64."""
    if not (mean_edge_mm > 0 and focal_px > 0 and distance_mm > 0):
        raise ValueError("resolution_for: positive mean_edge_mm, focal_px and distance_mm expected")
    return int(min(MAX_R, max(1, round(mean_edge_mm * focal_px / distance_mm))))


def mean_edge_length(verts, faces) -> float:
    """The mean length of the mesh's undirected edges (fp64)."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    e = mesh_edges(faces)
    return float(np.linalg.norm(v[e[:, 0]] - v[e[:, 1]], axis=1).mean())


def subdivide(verts, faces, R: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The mesh with every face cut into R^2 -> (verts_sub [U,3] float32, faces_sub [F R^2,3] int32, node_index [F,T] int64: the
    row of verts_sub that holds node n of face f).  Nodes are unique by a canonical rule, so that the faces at an edge share them:
    a corner node is its vertex (rows 0 .. V-1, unchanged); the R - 1 inner nodes of edge e = (p < q) of mesh_edges' order are
    ((R - k) v_p + k v_q) / R, k = 1 .. R-1, in fp64 from the ordered pair (rows V + e (R - 1) + k - 1): both faces get the same
    bits; the (R - 1)(R - 2) / 2 interior nodes of face f, ((R - i - j) v0 + i v1 + j v2) / R in fp64, follow per face in storage
    order.  U = V + E (R - 1) + F (R - 1)(R - 2) / 2.  A face's R^2 sub-faces keep its orientation: per cell (i, j) the lower triangle
    (n(i,j), n(i+1,j), n(i,j+1)) and, where i + j <= R - 2, the upper one (n(i+1,j), n(i+1,j+1), n(i,j+1)).  R = 1 is the identity."""
    T = texel_count(R)
    v32 = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    v = v32.astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V, F = len(v), len(f)
    if F and (f.min() < 0 or f.max() >= V):
        raise ValueError("subdivide: a face names a vertex outside 0 .. %d" % (V - 1))
    edges = mesh_edges(f)
    E = len(edges)
    ekey = edges[:, 0] * V + edges[:, 1]
    ij = node_ij(R)
    ni, nj = ij[:, 0], ij[:, 1]
    n_inner = (R - 1) * (R - 2) // 2
    node_index = np.full((F, T), -1, dtype=np.int64)
    inner_pos = np.zeros((F, n_inner, 3))

    def edge_nodes(sel, a, b, k_from_a):
        """nodes ``sel`` of every face lie on its edge from corner a to corner b, ``k_from_a`` [len(sel)] steps from a"""
        pa, pb = f[:, a], f[:, b]
        lo, hi = np.minimum(pa, pb), np.maximum(pa, pb)
        e = np.searchsorted(ekey, lo * V + hi).clip(0, max(E - 1, 0))
        k = np.where((pa <= pb)[:, None], k_from_a[None], R - k_from_a[None])         # steps from the smaller vertex index
        idx = V + e[:, None] * (R - 1) + k - 1
        node_index[:, sel] = np.where((pa == pb)[:, None], pa[:, None], idx)         # (a collapsed edge: the vertex itself)

    node_index[:, (ni == 0) & (nj == 0)] = f[:, [0]]
    node_index[:, (ni == R) & (nj == 0)] = f[:, [1]]
    node_index[:, (ni == 0) & (nj == R)] = f[:, [2]]
    if R > 1:
        s = np.nonzero((nj == 0) & (ni > 0) & (ni < R))[0]
        edge_nodes(s, 0, 1, ni[s])
        s = np.nonzero((ni == 0) & (nj > 0) & (nj < R))[0]
        edge_nodes(s, 0, 2, nj[s])
        s = np.nonzero((ni + nj == R) & (ni > 0) & (nj > 0))[0]
        edge_nodes(s, 1, 2, nj[s])
    s = np.nonzero((ni > 0) & (nj > 0) & (ni + nj < R))[0]
    if len(s):
        node_index[:, s] = V + E * (R - 1) + np.arange(F)[:, None] * n_inner + np.arange(n_inner)[None]
        w = np.stack([R - ni[s] - nj[s], ni[s], nj[s]], axis=1).astype(np.float64)      # integer weights, divided once
        inner_pos = ((w[None, :, 0, None] * v[f[:, 0]][:, None] + w[None, :, 1, None] * v[f[:, 1]][:, None])
                     + w[None, :, 2, None] * v[f[:, 2]][:, None]) / R
    k = np.arange(1, R, dtype=np.float64)[None, :, None]
    edge_pos = ((R - k) * v[edges[:, 0]][:, None] + k * v[edges[:, 1]][:, None]) / R
    verts_sub = np.concatenate([v32, edge_pos.reshape(-1, 3).astype(np.float32), inner_pos.reshape(-1, 3).astype(np.float32)])
    n = lambda i, j: j * (R + 1) - j * (j - 1) // 2 + i
    cells = []
    for j in range(R):
        for i in range(R - j):
            cells.append((n(i, j), n(i + 1, j), n(i, j + 1)))
            if i + j <= R - 2:
                cells.append((n(i + 1, j), n(i + 1, j + 1), n(i, j + 1)))
    faces_sub = node_index[:, np.array(cells, dtype=np.int64)].reshape(-1, 3).astype(np.int32)
    return verts_sub, faces_sub, node_index


def texels_from_nodes(colour_sub, node_index):
    """Per-node values [U,C] (e.g. the vertex colours of the subdivided mesh) -> texels [F,T,C]; numpy in, numpy out, tensors likewise."""
    if torch.is_tensor(colour_sub):
        return colour_sub[torch.as_tensor(node_index, device=colour_sub.device, dtype=torch.long)].contiguous()
    return np.ascontiguousarray(np.asarray(colour_sub)[np.asarray(node_index)])


def nodes_from_texels(texels, node_index, U: Optional[int] = None) -> np.ndarray:
    """texels [F,T,C] -> per-node values [U,C] (numpy).  A node that several faces share takes the value of the last face that names
    it: for a texture that is continuous across edges (every baked one) they are equal."""
    t = texels.detach().cpu().numpy() if torch.is_tensor(texels) else np.asarray(texels)
    idx = np.asarray(node_index)
    U = int(idx.max()) + 1 if U is None else int(U)
    out = np.zeros((U,) + t.shape[2:], dtype=t.dtype)
    out[idx.reshape(-1)] = t.reshape((-1,) + t.shape[2:])
    return out


class FaceTexelBaker:
    """Accumulates views of one mesh into a face-texel texture of resolution R: the vertex bake (TextureBaker, K27) on the U unique
    nodes of ``subdivide``, with the normals vertex_normals(verts_sub, faces_sub) and the depth planes of the BASE mesh.  The texture
    is continuous across edges by construction: the faces at an edge index the same nodes."""

    def __init__(self, verts, faces, R: int, H: int, W: int, device="cuda:0", **thresholds):
        self.R, self.T = int(R), texel_count(R)
        self.verts_host = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
        self.faces_host = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
        self.verts_sub, self.faces_sub, self.node_index_host = subdivide(self.verts_host, self.faces_host, self.R)
        self.nodes = TextureBaker(self.verts_sub, self.faces_sub, H, W, device, **thresholds)
        self.device, self.H, self.W = self.nodes.device, self.nodes.H, self.nodes.W
        self.verts = torch.from_numpy(self.verts_host).to(self.device)
        self.faces = torch.from_numpy(self.faces_host).to(self.device)
        self.node_index = torch.from_numpy(self.node_index_host).to(self.device)

    @property
    def views(self) -> int:
        return self.nodes.views

    def reset(self) -> None:
        self.nodes.reset()

    def add_views(self, rgb: Tensor, pose_mm: Tensor, intr: Tensor, zbuf: Optional[Tensor] = None, weight: Optional[Tensor] = None) -> None:
        """As TextureBaker.add_views; ``zbuf`` None: the base mesh is rasterised here."""
        if zbuf is None:
            pose = torch.as_tensor(pose_mm, dtype=torch.float32).to(self.device).contiguous()
            K = torch.as_tensor(intr, dtype=torch.float32).to(self.device)
            zbuf = ops.mesh_raster(self.verts, self.faces, pose, K, H=self.H, W=self.W, face_ids=False, normals=False)["zbuf"]
        self.nodes.add_views(rgb, pose_mm, intr, zbuf=zbuf, weight=weight)

    def result(self, fill: bool = True) -> AttrDict:
        """texels [F,T,3] and vcolor_sub [U,3] float32 in [0,1], seen [U] bool -- tensors on the device -- and the numbers of filled
        and still uncoloured nodes (TextureBaker.result over the subdivided mesh: ``fill`` spreads colour along faces_sub's edges)."""
        r = self.nodes.result(fill=fill)
        return AttrDict(texels=texels_from_nodes(r.vcolor, self.node_index), vcolor_sub=r.vcolor, seen=r.seen, filled=r.filled,
                        unseen=r.unseen, weight=r.weight, count=r.count)


def save_texels(path: str, texels, faces) -> None:
    """An .npz with 'texels' [F,T,3] float32, 'R' and the 'faces' [F,3] int32 the texture belongs to (texel order follows vertex order
    within a face, so the file is only meaningful with exactly these faces)."""
    t = (texels.detach().cpu().numpy() if torch.is_tensor(texels) else np.asarray(texels)).astype(np.float32)
    f = (faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int32).reshape(-1, 3)
    if t.ndim != 3 or t.shape[2] != 3 or t.shape[0] != len(f):
        raise ValueError("save_texels: texels [F=%d,T,3] expected, got %s" % (len(f), t.shape))
    with open(path, "wb") as fh:                       # (a file object: numpy appends no suffix)
        np.savez(fh, texels=t, R=np.int32(resolution_of(t.shape[1])), faces=f)


def load_texels(path: str, faces) -> Tuple[np.ndarray, int]:
    """-> (texels [F,T,3] float32, R) of a file save_texels wrote; refuses a file whose faces are not exactly ``faces``."""
    f = (faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int32).reshape(-1, 3)
    with np.load(path) as z:
        texels, R, own = z["texels"], int(z["R"]), z["faces"]
    if own.shape != f.shape or not np.array_equal(own, f):
        raise ValueError("load_texels: %s was baked for another mesh (its faces differ from the mesh's)" % path)
    if texels.shape != (len(f), texel_count(R), 3):
        raise ValueError("load_texels: %s holds texels %s for R = %d and %d faces" % (path, texels.shape, R, len(f)))
    return texels.astype(np.float32), R


def write_subdivided_ply(path: str, verts, faces, texels) -> None:
    """The texture as a vertex-coloured PLY of the subdivided mesh, for tools that only read PLY (8-bit colours)."""
    t = texels.detach().cpu().numpy() if torch.is_tensor(texels) else np.asarray(texels)
    verts_sub, faces_sub, node_index = subdivide(verts, faces, resolution_of(t.shape[1]))
    write_ply(path, verts_sub, faces_sub, nodes_from_texels(t, node_index, len(verts_sub)))
