"""Per-face texel textures ("mesh colours"): colour detail below the mesh's vertex spacing without a UV unwrap (K35).

Every face carries the barycentric grid of resolution R of include/texpose_amd.h (K35): T(R) = (R + 1)(R + 2) / 2 nodes, node (i, j) at
the weights ((R - i - j) / R, i / R, j / R) of the face's vertices in the face's own order, stored at n(i, j) = j (R + 1) - j (j - 1) / 2
+ i.  ``ops.face_texel_shade`` interpolates them per pixel of the rasteriser's face plane, so geometry and rasteriser work stay those
of the base mesh while the colour becomes R x finer along each edge.  The nodes of all faces are exactly the vertices of the mesh
subdivided R times (``subdivide``), which is how a texture is baked -- ``FaceTexelBaker`` runs the unchanged vertex bake (K27) on those
points -- and what the shading is tested against: texels on the base mesh equal vertex colours on the subdivided one.

``ops.face_texel_shade`` point-samples (pick R with ``resolution_for`` so that a texel is about a pixel).  Where one texture is seen
over a range of distances, ``build_mips`` makes the chain of coarser levels (K43a) and ``ops.face_texel_shade_mip`` /
``ops.mesh_raster(texel_mips=)`` shade through it, choosing and blending two levels per pixel (K43b).  One R per
mesh, no UV atlas.

Gradients with respect to the texture come from K36 (tp_face_texel_shade_bwd), the deterministic adjoint of the
shading: ``autograd_ops.face_texel_shade`` (per-slot texels), ``shade_nodes`` (node colours shared between faces) and
``FaceTexelFitter``, which fits the node colours to photographs by preconditioned conjugate gradients on the quantity the refiners
consume: the difference between the shaded render and the photograph.  No gradients with respect to pose or vertices, first order only.
``FaceTexelFitter(lighting=True)`` (K41 tp_face_texel_light) fits the colours as an albedo under one first-order
SH light per view, for photographs whose light differs from view to view.  ``FaceTexelFitter(robust="tukey")`` (K42 tp_robust_weight,
DESIGN.md section 32) reweights the pixels round by round, for photographs with occluders and highlights.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

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


def mip_levels(R: int) -> int:
    """The number of levels the chain of a texture of resolution R can have: level l has R >> l and exists while the one before is
    even, so 1 + the number of times 2 divides R (64 -> 7, 6 -> 2, an odd R -> 1)."""
    texel_count(R)
    R, L = int(R), 1
    while R % 2 == 0:
        R, L = R // 2, L + 1
    return L


def mip_slots(verts, faces, Rc: int) -> Tuple[np.ndarray, np.ndarray]:
    """The slots of every unique node of the grid of resolution Rc as a CSR pair, for ops.face_texel_mip_reduce INTO that grid ->
    (slot_ptr [U+1] int32, slot_list [F T(Rc)] int32): node u is named by the slots slot_list[slot_ptr[u] : slot_ptr[u+1]] (f T + n,
    ascending), from ``subdivide``'s node_index by a stable argsort."""
    node_index = subdivide(verts, faces, Rc)[2].reshape(-1)
    U = int(node_index.max()) + 1 if node_index.size else 0
    slot_list = np.argsort(node_index, kind="stable").astype(np.int32)
    slot_ptr = np.concatenate([[0], np.cumsum(np.bincount(node_index, minlength=U))]).astype(np.int32)
    return slot_ptr, slot_list


class TexelMips:
    """The mip chain of a face-texel texture on the device: ``R`` (level 0's resolution), ``L`` levels, ``F`` faces and ``packed``,
    ONE float32 buffer in which level l is the contiguous [F, T(R >> l), 3] block at element offset 3 F sum_{k<l} T(R >> k).
    ``level(l)`` is a view of it."""

    def __init__(self, R: int, L: int, F: int, packed: Tensor):
        self.R, self.L, self.F, self.packed = int(R), int(L), int(F), packed
        self._offsets = np.concatenate([[0], np.cumsum([3 * self.F * texel_count(self.R >> l) for l in range(self.L)])])
        if not 1 <= self.L <= mip_levels(self.R) or packed.dim() != 1 or packed.numel() != int(self._offsets[-1]):
            raise ValueError("TexelMips: R = %d allows 1 .. %d levels and L = %d of them over %d faces hold %d values, got %d"
                             % (self.R, mip_levels(self.R), self.L, self.F, int(self._offsets[-1]), packed.numel()))

    def level(self, l: int) -> Tensor:
        """Level l as [F, T(R >> l), 3] (a view of ``packed``)."""
        if not 0 <= int(l) < self.L:
            raise ValueError("TexelMips.level: level in 0 .. %d expected, got %r" % (self.L - 1, l))
        return self.packed[int(self._offsets[l]):int(self._offsets[l + 1])].view(self.F, texel_count(self.R >> int(l)), 3)


def build_mips(verts, faces, texels, levels: Optional[int] = None) -> TexelMips:
    """The mip chain of ``texels`` [F,T(R),3] (a tensor on the device, or anything torch.as_tensor takes: then on cuda:0) over the mesh
    (verts, faces) they belong to -> TexelMips with ``levels`` levels (None: as many as R allows, ``mip_levels``).  Level 0 is the
    texture itself; every further level is one ops.face_texel_mip_reduce (K43a) of the one before, with the CSR of ``mip_slots``.
    Nothing is stored on disk: save_texels keeps level 0 and the chain is rebuilt from it in milliseconds."""
    t = texels if torch.is_tensor(texels) else torch.as_tensor(np.asarray(texels, dtype=np.float32))
    t = t.detach().to(device=t.device if t.is_cuda else "cuda:0", dtype=torch.float32).contiguous()
    f = (faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)).astype(np.int32).reshape(-1, 3)
    v = (verts.detach().cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)).astype(np.float32).reshape(-1, 3)
    if t.dim() != 3 or t.shape[0] != len(f) or t.shape[2] != 3:
        raise ValueError("build_mips: texels [F=%d,T,3] expected, got %s" % (len(f), tuple(t.shape)))
    R = resolution_of(t.shape[1])
    L = mip_levels(R) if levels is None else int(levels)
    if not 1 <= L <= mip_levels(R):
        raise ValueError("build_mips: R = %d allows 1 .. %d levels, got %r" % (R, mip_levels(R), levels))
    sizes = [3 * len(f) * texel_count(R >> l) for l in range(L)]
    mips = TexelMips(R, L, len(f), torch.empty(sum(sizes), device=t.device))
    mips.level(0).copy_(t)
    for l in range(1, L):
        slot_ptr, slot_list = mip_slots(v, f, R >> l)
        ops.face_texel_mip_reduce(mips.level(l - 1), torch.from_numpy(slot_ptr).to(t.device), torch.from_numpy(slot_list).to(t.device),
                                  out=mips.level(l))
    return mips


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


class _TexelMesh:
    """What FaceTexelBaker and FaceTexelFitter share: the base mesh, its subdivision at resolution R and the device copies."""

    def _set_mesh(self, verts, faces, R: int, device) -> None:
        self.R, self.T, self.device = int(R), texel_count(R), torch.device(device)
        self.verts_host = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
        self.faces_host = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
        self.verts_sub, self.faces_sub, self.node_index_host = subdivide(self.verts_host, self.faces_host, self.R)
        self.verts = torch.from_numpy(self.verts_host).to(self.device)
        self.faces = torch.from_numpy(self.faces_host).to(self.device)
        self.node_index = torch.from_numpy(self.node_index_host).to(self.device)


class FaceTexelBaker(_TexelMesh):
    """Accumulates views of one mesh into a face-texel texture of resolution R: the vertex bake (TextureBaker, K27) on the U unique
    nodes of ``subdivide``, with the normals vertex_normals(verts_sub, faces_sub) and the depth planes of the BASE mesh.  The texture
    is continuous across edges by construction: the faces at an edge index the same nodes."""

    def __init__(self, verts, faces, R: int, H: int, W: int, device="cuda:0", **thresholds):
        self._set_mesh(verts, faces, R, device)
        self.nodes = TextureBaker(self.verts_sub, self.faces_sub, H, W, device, **thresholds)
        self.H, self.W = self.nodes.H, self.nodes.W

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


def shade_nodes(face: Tensor, verts: Tensor, faces: Tensor, nodes: Tensor, node_index, pose: Tensor, intr: Tensor) -> Tensor:
    """ops.face_texel_shade of the texels ``nodes[node_index]`` (nodes [U,3], node_index [F,T] as ``subdivide`` gives it) -> rgb
    [B,H,W,3], differentiable with respect to ``nodes``: the backward is K36 with the node index, straight into [U,3] -- 64-bit fixed
    point, bit-identical from run to run, no index_add_.  First order only."""
    from . import autograd_ops
    return autograd_ops.face_texel_shade_nodes(face, verts, faces, nodes, torch.as_tensor(node_index, device=nodes.device), pose, intr)


class _View(NamedTuple):
    """One add_views call of FaceTexelFitter, on the device until reset(); zbuf and mask with lighting only: the depth plane the light
    step reads as "covered" and its mask (weight > 0)."""
    face: Tensor
    rgb: Tensor
    weight: Tensor
    pose: Tensor
    intr: Tensor
    zbuf: Optional[Tensor] = None
    mask: Optional[Tensor] = None


class FaceTexelFitter(_TexelMesh):
    """Fits the U node colours x of a face-texel texture of resolution R to photographs: minimises
        sum_p m_p |(S x)_p - I_p|^2 + lam |x - prior|^2
    over the stored views, S the shading rule of K35 on the node colours (texels = x[node_index]).  S x is ops.face_texel_shade, S^T g
    is ops.face_texel_shade_bwd with the node index: deterministic, so a fit is bit-identical from run to run.  The result is not
    clamped: the caller does that.

    The loop, common to the three modes: a round is one pass over the stored views -- shade, the mode's pixel step, adjoint -- that
    gives the right-hand side, the preconditioner and the error sums (the first pass also yields the coverage: the per-node sum of
    shading weights over all covered pixels, K36's ``weight``, the lumped diagonal of S^T S), and then ``iters`` steps of preconditioned
    conjugate gradients (_pcg) restarted from the current x.  An iteration is one shade and one adjoint over the stored views for the
    step and one more shade for the training rms it reports.

    The plain fit (a quadratic loss, the default) is one round, preconditioned with M = coverage + lam.  Any loss that is none of the
    three modes goes through ``shade_nodes`` and an optimiser.

    ``robust`` = "tukey" or "huber" (K42) fits by iteratively reweighted least squares, for photographs that carry
    what no texture explains (an occluder, a highlight, a patch of background).  ``robust_rounds`` rounds, each of which weights every
    pixel of every stored view by ops.robust_weight of the current residual (Tukey's biweight with c = 4.685, or Huber's weight with c =
    1.345, or ``robust_c``; in units of sigma = 1.4826 sqrt(median of the mean squared colour error) per view, at least ``sigma_min``)
    times the view's own weight, and solves the weighted system, preconditioned with S^T (w) + lam.  The result gains scale, kept and
    robust_count per view (see _robust_mode).  Not together with ``lighting=True``.

    ``lighting=True`` (K41) fits x as an ALBEDO under one first-order SH light per stored view: it minimises
        sum_b sum_p m_p |s_b(n_p) (S x)_p + beta_b - I_p|^2 + lam |x - prior|^2
    over x and the lights (l0, l1, l2, l3, beta per view and channel; s = l0 + l1 n_x + l2 n_y + l3 n_z on the face's normal, as
    ops.photo_lighting) by ``rounds`` alternations: a light step (ops.photo_lighting of the unlit render S x against each photograph,
    ``tau0`` in round 0 and ``tau`` afterwards, l0 within ``gain_range``) and the round's conjugate-gradient steps on (S^T m s^2 S + lam) x
    = S^T m s (I - beta) + lam prior, preconditioned per node and channel with S^T (m s^2) + lam; between shade and adjoint sits
    ops.face_texel_light.  From round 1 on a view whose light fit fails (status != 0) or falls back to the ambient-only form in a channel
    keeps the light it had.  The gauge (x scaled by a, every l0 .. l3 by 1 / a) is pinned by the prior alone; the result's ``gain`` is
    the mean l0 per channel, for a caller who wants to normalise (see _lit_mode)."""

    def __init__(self, verts, faces, R: int, H: int, W: int, device="cuda:0", lam: float = 0.1, iters: int = 4, cull: bool = False,
                 lighting: bool = False, rounds: int = 6, tau: float = 0.5, tau0: float = 2.0, gain_range=(0.25, 4.0),
                 robust: Optional[str] = None, robust_c: Optional[float] = None, robust_rounds: int = 6, sigma_min: float = 1.0 / 255.0):
        self.T, self.H, self.W = texel_count(R), int(H), int(W)        # (R is checked before the other arguments)
        if not (lam > 0 and int(iters) >= 0):
            raise ValueError("FaceTexelFitter: lam > 0 and iters >= 0 expected")
        if robust is not None:
            if robust not in ops.ROBUST_KINDS:
                raise ValueError("FaceTexelFitter: robust %r is none of None, %s" % (robust, ", ".join(map(repr, sorted(ops.ROBUST_KINDS)))))
            if lighting:
                raise ValueError("FaceTexelFitter: robust weights under lighting=True are left out (DESIGN.md section 32): pass weights from "
                                 "ops.robust_weight through add_views(weight=) instead")
            c = ops.ROBUST_KINDS[robust][1] if robust_c is None else float(robust_c)
            if not (int(robust_rounds) >= 1 and np.isfinite(c) and c > 0 and np.isfinite(sigma_min) and sigma_min > 0):
                raise ValueError("FaceTexelFitter: robust_rounds >= 1, robust_c > 0 and sigma_min > 0 expected with robust")
            self.robust_c, self.robust_rounds, self.sigma_min = c, int(robust_rounds), float(sigma_min)
        self.robust = robust
        if lighting and not (int(rounds) >= 1 and tau > 0 and tau0 > 0):
            raise ValueError("FaceTexelFitter: rounds >= 1, tau > 0 and tau0 > 0 expected with lighting")
        self.lighting, self.rounds, self.tau, self.tau0 = bool(lighting), int(rounds), float(tau), float(tau0)
        self.gain_range = tuple(float(g) for g in gain_range)
        self.lam, self.iters, self.cull = float(lam), int(iters), bool(cull)
        self._set_mesh(verts, faces, R, device)
        self.U = len(self.verts_sub)
        self._node_index32 = self.node_index.to(torch.int32)
        self._faces_lit = self.faces.contiguous()        # (K40 and K41 take the faces as they are: a PLY reader may hand over a strided view)
        self._views = []                                 # one _View per add_views call

    @property
    def views(self) -> int:
        return sum(v.face.shape[0] for v in self._views)

    def reset(self) -> None:
        self._views = []

    def add_views(self, rgb: Tensor, pose_mm: Tensor, intr: Tensor, face: Optional[Tensor] = None, weight: Optional[Tensor] = None) -> None:
        """rgb [B,H,W,3] photographs, pose_mm [B,3,4] (t in mm), intr [B,3,3] or [3,3]; ``face`` [B,H,W] int32: the base mesh's face
        plane at those poses (None: rasterised here); ``weight`` [B,H,W] per pixel (None: 1 on covered pixels whose four neighbours are
        covered too, 0 elsewhere: the rim pixels of a photograph mix in background).  Face plane, photograph and weight stay on the
        device until reset(): 20 bytes per pixel (with lighting 25: the depth plane the light step reads as "covered" and its mask)."""
        pose = torch.as_tensor(pose_mm, dtype=torch.float32).to(self.device).contiguous()
        B = pose.shape[0]
        K = torch.as_tensor(intr, dtype=torch.float32).to(self.device)
        K = (K[None].expand(B, 3, 3) if K.dim() == 2 else K).contiguous()
        rgb = torch.as_tensor(rgb).detach().to(device=self.device, dtype=torch.float32).contiguous()
        if tuple(rgb.shape) != (B, self.H, self.W, 3):
            raise ValueError("FaceTexelFitter.add_views: rgb %s expected, got %s" % ((B, self.H, self.W, 3), tuple(rgb.shape)))
        zbuf = None
        if face is None:
            planes = ops.mesh_raster(self.verts, self.faces, pose, K, H=self.H, W=self.W, normals=False, cull=self.cull)
            face, zbuf = planes["face"], planes["zbuf"]
        face = torch.as_tensor(face).to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(face.shape) != (B, self.H, self.W):
            raise ValueError("FaceTexelFitter.add_views: face %s expected, got %s" % ((B, self.H, self.W), tuple(face.shape)))
        if weight is None:
            weight = inner_coverage(face, self.faces.shape[0]).float()
        weight = torch.as_tensor(weight).detach().to(device=self.device, dtype=torch.float32).reshape(B, self.H, self.W).contiguous()
        if not self.lighting:
            self._views.append(_View(face, rgb, weight, pose, K))
            return
        if zbuf is None:                                 # (the light step reads depth only as "covered")
            zbuf = torch.where((face >= 0) & (face < self.faces.shape[0]), 1.0, -1.0).float()
        self._views.append(_View(face, rgb, weight, pose, K, zbuf.contiguous(), (weight > 0).to(torch.uint8)))

    def _shade(self, view: _View, x: Tensor) -> Tensor:
        return ops.face_texel_shade(view.face, self.verts, self.faces, x[self.node_index], view.pose, view.intr)

    def _adjoint(self, view: _View, g: Tensor, weight: bool = False):
        return ops.face_texel_shade_bwd(view.face, self.verts, self.faces, g, view.pose, view.intr, R=self.R, node_index=self._node_index32,
                                        U=self.U, weight=weight)

    def fit(self, prior: Optional[Tensor] = None, start: Optional[Tensor] = None, lights: Optional[Tensor] = None, light_step: bool = True) -> AttrDict:
        """``prior`` [U,3] (e.g. FaceTexelBaker's vcolor_sub; None: 0.5), ``start`` [U,3] (None: the prior) -> AttrDict(texels [F,T,3],
        nodes [U,3], coverage [U], rms [rounds * iters + 1]: sqrt(sum w |residual|^2 / (3 sum w)) under the mode's weights at the start and
        after every iteration (a device tensor; rounds is 1, ``robust_rounds`` or ``rounds``), on_prior: the number of nodes with coverage <
        lam, which the prior decides) plus the mode's own keys (_robust_mode, _lit_mode).  With lighting: ``lights`` [views,3,5] are the lights to
        start from (None: (1, 0, 0, 0, 0)) and ``light_step=False`` keeps them through every round (a fit under known lights).  Scalars stay
        0-dim fp64 device tensors; nothing but on_prior is read back."""
        if not self.lighting and (lights is not None or not light_step):
            raise ValueError("FaceTexelFitter.fit: lights and light_step belong to lighting=True")
        if not self._views:
            raise ValueError("FaceTexelFitter.fit: no views (add_views first)")
        dev, U, lam = self.device, self.U, self.lam

        def nodes_arg(t, name, default):
            if t is None:
                return default
            t = torch.as_tensor(t).detach().to(device=dev, dtype=torch.float32)
            if tuple(t.shape) != (U, 3):
                raise ValueError("FaceTexelFitter.fit: %s [U=%d,3] expected, got %s" % (name, U, tuple(t.shape)))
            return t

        prior = nodes_arg(prior, "prior", torch.full((U, 3), 0.5, device=dev))
        x = nodes_arg(start, "start", prior).clone()
        if lights is not None:
            lights = torch.as_tensor(lights).detach().to(device=dev, dtype=torch.float32)
            if tuple(lights.shape) != (self.views, 3, 5):
                raise ValueError("FaceTexelFitter.fit: lights [views=%d,3,5] expected, got %s" % (self.views, tuple(lights.shape)))
        mode = self._lit_mode(lights, bool(light_step)) if self.lighting else self._robust_mode() if self.robust is not None else self._plain_mode()
        zero = torch.zeros((), device=dev, dtype=torch.float64)
        coverage, total, errors = torch.zeros(U, device=dev), zero, []       # errors: (sum w |residual|^2, sum w) per rms entry

        def apply(p):                                    # A p = S^T D S p + lam p, D the mode's pixel step under the round's weights or lights
            ap = lam * p
            for i, view in enumerate(self._views):
                ap = ap + self._adjoint(view, mode.between(i, view, self._shade(view, p)))
            return ap

        def after_step(x):
            sse = zero
            for i, view in enumerate(self._views):
                sse = sse + mode.sse(i, view, self._shade(view, x))
            errors.append((sse, total))

        for rnd in range(mode.rounds):
            # one pass over the views: r = b - A x = S^T (the mode's residual) + lam (prior - x), the preconditioner and the error sums
            r, pre, sse, round_total = lam * (prior - x), None, zero, zero
            for i, view in enumerate(self._views):
                grad, diag, err, weight = mode.residual(rnd, i, view, self._shade(view, x))
                if rnd == 0:                             # the first adjoint also gives the coverage (it does not look at the values)
                    g, cover = self._adjoint(view, grad, weight=True)
                    coverage = coverage + cover
                else:
                    g = self._adjoint(view, grad)
                if diag is not None:
                    pre = (torch.zeros(U, 3, device=dev) if pre is None else pre) + self._adjoint(view, diag)
                r, sse, round_total = r + g, sse + err, round_total + weight
            if rnd == 0 or mode.total_per_round:
                total = round_total
            if rnd == 0:
                errors.append((sse, total))
            m_inv = 1.0 / ((coverage[:, None] if pre is None else pre) + lam)
            x = _pcg(x, r, m_inv, apply, after_step, self.iters)
        sse, total = (torch.stack(t) for t in zip(*errors))
        return AttrDict(texels=texels_from_nodes(x, self.node_index), nodes=x, coverage=coverage,
                        rms=torch.sqrt(sse / (3.0 * total).clamp_min(1e-300)).float(), on_prior=int((coverage < lam).sum()), **mode.extras())

    # A mode of fit() supplies: rounds; residual(rnd, i, view, model), which first takes view i's weights or light for the round at model =
    # S x -> (the plane whose adjoint goes into r, the plane whose adjoint is the view's term of the preconditioner or None: the coverage
    # serves, sum w |residual|^2, sum w); between(i, view, shaded): the pixel step between shade and adjoint in A p; sse(i, view, model):
    # sum w |residual|^2 at a new x; total_per_round: whether sum w is the round's own; extras(): the result's further keys.
    def _plain_mode(self) -> AttrDict:
        """The quadratic fit: one round, a pixel weighs its view's m."""
        def residual(rnd, i, view, model):
            e = view.rgb - model
            return e * view.weight[..., None], None, ((e * e).sum(-1) * view.weight).double().sum(), view.weight.double().sum()

        def sse(i, view, model):
            e = model - view.rgb
            return ((e * e).sum(-1) * view.weight).double().sum()

        return AttrDict(rounds=1, total_per_round=False, residual=residual, between=lambda i, view, shaded: shaded * view.weight[..., None],
                        sse=sse, extras=dict)

    def _robust_mode(self) -> AttrDict:
        """robust=...: iteratively reweighted least squares.  A round takes the weights w = ops.robust_weight(S x, photograph, weight=m) of
        every stored view at the current x; its system is (S^T w S + lam) x = S^T w I + lam prior, preconditioned with S^T (w) + lam (the
        adjoint of the weight plane), and its rms is that under the round's own weights.  The result gains scale [views] (sigma per view),
        kept [views] = sum w / sum m and robust_count [views], all of the last round."""
        spaces = [ops.robust_weight_workspace(v.face.shape[0], self.H, self.W, self.device) for v in self._views]
        ws, fits = [None] * len(spaces), [None] * len(spaces)

        def residual(rnd, i, view, model):
            fits[i] = ops.robust_weight(model, view.rgb, weight=view.weight, kind=self.robust, c=self.robust_c, sigma_min=self.sigma_min,
                                        workspace=spaces[i])
            w = ws[i] = fits[i]["weight"]
            e = torch.where((w > 0)[..., None], view.rgb - model, torch.zeros_like(model))
            return e * w[..., None], w[..., None].expand(-1, -1, -1, 3).contiguous(), ((e * e).sum(-1) * w).double().sum(), w.double().sum()

        def sse(i, view, model):
            e = model - view.rgb
            return torch.where(ws[i] > 0, (e * e).sum(-1) * ws[i], torch.zeros_like(ws[i])).double().sum()

        def extras():
            base = torch.cat([torch.where(v.weight > 0, v.weight, torch.zeros_like(v.weight)).double().sum((1, 2)) for v in self._views])
            kept = (torch.cat([w.double().sum((1, 2)) for w in ws]) / base.clamp_min(1e-300)).float()
            return dict(scale=torch.cat([f["scale"] for f in fits]), kept=kept, robust_count=torch.cat([f["count"] for f in fits]))

        return AttrDict(rounds=self.robust_rounds, total_per_round=True, residual=residual, between=lambda i, view, shaded: shaded * ws[i][..., None],
                        sse=sse, extras=extras)

    def _lit_mode(self, start_lights: Optional[Tensor], light_step: bool) -> AttrDict:
        """lighting=True: a round first takes each view's light (ops.photo_lighting of the unlit render S x against the photograph, unless
        ``light_step`` is off); from round 1 a failed or fallback light keeps the one before.  Its system is (S^T m s^2 S + lam) x = S^T m s
        (I - beta) + lam prior, preconditioned with S^T (m s^2) + lam; ops.face_texel_light sits between shade and adjoint and sums the lit
        residual, so rms is that of the lit residual (after the first light step and after every iteration; sum m is round 0's).  The result
        gains light [views,3,5], lighting_status / lighting_flags [views] (ops.photo_lighting's, of the last round) and gain [3]."""
        dev, fallback = self.device, 7 * ops._lib.LIGHTING_FALLBACK
        sizes = [v.face.shape[0] for v in self._views]
        identity = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0], device=dev)
        lights = [None if light_step else identity.expand(b, 3, 5).contiguous() for b in sizes] if start_lights is None \
            else [t.contiguous() for t in start_lights.split(sizes)]
        status, flags = ([torch.zeros(b, device=dev, dtype=torch.int32) for b in sizes] for _ in range(2))

        def lit(i, view, colour, **kw):
            return ops.face_texel_light(view.face, self.verts, self._faces_lit, colour, view.pose, lights[i], weight=view.weight, **kw)

        def residual(rnd, i, view, model):
            if light_step:
                fit = ops.photo_lighting(self.verts, self._faces_lit, view.face, view.zbuf, model, view.pose, view.rgb, tau=self.tau0 if rnd == 0 else self.tau,
                                         light=lights[i], mask=view.mask, gain_range=self.gain_range, apply=False)
                failed = (fit["flags"] & fallback) != 0          # (status != 0: photo_lighting itself returns the incoming light)
                keep = fit["light"] if rnd == 0 else torch.where(failed[:, None, None], lights[i], fit["light"])
                lights[i], status[i], flags[i] = keep, fit["status"], fit["flags"]
            out = lit(i, view, model, image=view.rgb, diag=True, sums=True)
            sums = out["sums"].sum(0)
            return out["grad"], out["diag"], sums[0], sums[1]

        def extras():
            light = torch.cat(lights)
            return dict(light=light, lighting_status=torch.cat(status), lighting_flags=torch.cat(flags), gain=light[:, :, 0].double().mean(0).float())

        return AttrDict(rounds=self.rounds, total_per_round=False, residual=residual, between=lambda i, view, shaded: lit(i, view, shaded)["grad"],
                        sse=lambda i, view, model: lit(i, view, model, image=view.rgb, sums=True)["sums"].sum(0)[0], extras=extras)


def _pcg(x: Tensor, r: Tensor, m_inv: Tensor, apply, after_step, iters: int) -> Tensor:
    """``iters`` steps of preconditioned conjugate gradients from x, whose residual b - A x is r -> x.  ``apply(p)`` is A p, ``m_inv`` the
    inverse of the diagonal preconditioner, ``after_step(x)`` is called after every step.  The scalars are 0-dim fp64 device tensors and a
    vanishing denominator gives a zero step: nothing is read back."""
    dot = lambda a, b: (a.double() * b.double()).sum()
    zero, one = torch.zeros((), device=x.device, dtype=torch.float64), torch.ones((), device=x.device, dtype=torch.float64)
    z = r * m_inv
    p, rz = z.clone(), dot(r, z)
    for _ in range(iters):
        ap = apply(p)
        pap = dot(p, ap)
        alpha = torch.where(pap > 0, rz / torch.where(pap > 0, pap, one), zero)
        x, r = x + alpha.float() * p, r - alpha.float() * ap
        z = r * m_inv
        rz_new = dot(r, z)
        beta = torch.where(rz > 0, rz_new / torch.where(rz > 0, rz, one), zero)
        p, rz = z + beta.float() * p, rz_new
        after_step(x)
    return x


def inner_coverage(face: Tensor, F: int) -> Tensor:
    """face [B,H,W] -> bool [B,H,W]: pixels that hold a face of 0 .. F-1 and whose four neighbours do (the frame's border does not)."""
    c = (face >= 0) & (face < F)
    inner = torch.zeros_like(c)
    inner[:, 1:-1, 1:-1] = c[:, 1:-1, 1:-1] & c[:, :-2, 1:-1] & c[:, 2:, 1:-1] & c[:, 1:-1, :-2] & c[:, 1:-1, 2:]
    return inner


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
