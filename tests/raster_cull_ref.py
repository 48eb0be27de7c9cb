"""numpy restatement of what the culled rasteriser (tp_mesh_raster_culled) skips: the pixel boxes of the faces
from mesh_raster_ref.project in fp64 with the kernel's rounding rule, the union box of every chunk of 256 faces, and the number of
(tile, chunk) pairs a 16 x 16 tile's workgroup enters, with and without the chunk test.  Counts of work, not times."""
import numpy as np

import mesh_raster_ref as RR
from oracle.texpose_oracle import LINEMOD_K, rotation_from_axis_angle
from texture_bake_ref import torus, uv_sphere

TILE, CHUNK = 16, 256
EMPTY = (np.iinfo(np.int32).max, np.iinfo(np.int32).min, np.iinfo(np.int32).max, np.iinfo(np.int32).min)


def face_boxes(verts, faces, pose, K, H, W):
    """[F,4] int64 (jmin, jmax, imin, imax), inclusive pixel indices: the centres (j + 0.5, i + 0.5) inside the face's bounding box,
    clamped to the image; EMPTY for a face the kernel drops (an index outside the mesh, a vertex at z <= 0, a degenerate area) or
    whose box holds no centre."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(verts)
    inside = ((faces >= 0) & (faces < V)).all(1)
    U, Vv, Z, area, valid = RR.project(verts, np.where(inside[:, None], faces, 0), pose, K)
    valid = valid & inside & np.isfinite(U).all(1) & np.isfinite(Vv).all(1)
    box = np.tile(np.array(EMPTY, dtype=np.int64), (len(faces), 1))
    with np.errstate(invalid="ignore"):
        j0 = np.maximum(np.ceil(U.min(1) - 0.5), 0.0)
        j1 = np.minimum(np.floor(U.max(1) - 0.5), W - 1.0)
        i0 = np.maximum(np.ceil(Vv.min(1) - 0.5), 0.0)
        i1 = np.minimum(np.floor(Vv.max(1) - 0.5), H - 1.0)
        live = valid & (j0 <= j1) & (i0 <= i1)
    box[live] = np.stack([j0, j1, i0, i1], 1)[live].astype(np.int64)
    return box


def chunk_boxes(box):
    """[ceil(F / 256), 4]: the union of the boxes of each chunk of 256 consecutive faces (EMPTY is neutral and stands for f >= F)."""
    n = -(-len(box) // CHUNK)
    pad = np.tile(np.array(EMPTY, dtype=np.int64), (n * CHUNK, 1))
    pad[:len(box)] = box
    pad = pad.reshape(n, CHUNK, 4)
    return np.stack([pad[..., 0].min(1), pad[..., 1].max(1), pad[..., 2].min(1), pad[..., 3].max(1)], 1)


def tiles_of(H, W):
    """[T,4] (tx0, tx1, ty0, ty1) of the 16 x 16 tiles in the kernel's order (row-major), clipped to the image."""
    ty, tx = np.meshgrid(np.arange(0, H, TILE), np.arange(0, W, TILE), indexing="ij")
    tx, ty = tx.reshape(-1), ty.reshape(-1)
    return np.stack([tx, np.minimum(tx + TILE, W) - 1, ty, np.minimum(ty + TILE, H) - 1], 1)


def overlaps(box, tiles):
    """[T, N] bool: the four inclusive comparisons of the kernels' box tests."""
    return ((box[None, :, 0] <= tiles[:, None, 1]) & (box[None, :, 1] >= tiles[:, None, 0])
            & (box[None, :, 2] <= tiles[:, None, 3]) & (box[None, :, 3] >= tiles[:, None, 2]))


def counts(verts, faces, pose, K, H, W):
    """dict: 'plain' = tiles x chunks, 'culled' = (tile, chunk) pairs whose chunk box overlaps the tile, 'per_tile' [T] the culled count of
    each tile, 'faces_mean' / 'faces_max' the number of faces whose own box overlaps a tile, over the tiles that at least one overlaps."""
    box = face_boxes(verts, faces, pose, K, H, W)
    tiles = tiles_of(H, W)
    cb = chunk_boxes(box)
    per_tile = overlaps(cb, tiles).sum(1)
    live = box[box[:, 0] <= box[:, 1]]
    per_face = np.zeros(len(tiles), dtype=np.int64)
    for s in range(0, len(live), 1 << 14):
        per_face += overlaps(live[s:s + (1 << 14)], tiles).sum(1)
    busy = per_face[per_face > 0]
    return dict(plain=len(tiles) * len(cb), culled=int(per_tile.sum()), per_tile=per_tile,
                faces_mean=float(busy.mean()) if len(busy) else 0.0, faces_max=int(busy.max()) if len(busy) else 0)


def pose_of(w, t):
    return np.concatenate([rotation_from_axis_angle(np.asarray(w, dtype=np.float64)), np.asarray(t, dtype=np.float64)[:, None]], axis=1).astype(np.float32)


def table_cases():
    """The count table's cases: name -> (verts, faces, pose, K, H, W).  The first three are 480 x 640 with LINEMOD_K."""
    K = np.asarray(LINEMOD_K, dtype=np.float32)
    crop = K.copy()
    crop[0, 2] = crop[1, 2] = 64.0
    small = uv_sphere(71, 144, ripple=0.08)
    return {"sphere_20k": small + (pose_of([0.4, -0.9, 0.3], [10, -5, 750]), K, 480, 640),
            "sphere_199k": uv_sphere(223, 448, ripple=0.08) + (pose_of([0.4, -0.9, 0.3], [10, -5, 750]), K, 480, 640),
            "torus_26k": torus(160, 80) + (pose_of([1.2, 0.2, 0.0], [0, 5, 400]), K, 480, 640),
            "sphere_20k_crop128": small + (pose_of([0.4, -0.9, 0.3], [10, -5, 750]), crop, 128, 128)}
