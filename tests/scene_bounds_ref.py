"""numpy fp32 statement of the scene-bounds rules (tp_scene_bounds, DESIGN "Scene bounds for novel views"), for the tests.

The reference blends its objects inline in a trainer method that needs PyTorch3D and cannot be called here, so the blend is pinned to
this restatement; the parts of the reference that can be called (pixel rays, the slab test, the pose sweep) are pinned by golden G23.
Every array operation below is one rounded fp32 step, in the order the kernel takes them.

    z_k     = zbuf_k if zbuf_k > 0 else 100000              (mm; the planes are the rasteriser's, -1 on background)
    winner  = first k with the smallest z_k;  covered = zbuf_winner > 0
    depth   = (z_winner / 1000) * depth_scale where covered, else 0
    label   = ids[winner] where covered, else 0
    box     : labelled pixels take the winner's slab interval where the slab test holds and (0, 0) where it does not
    render  : covered pixels take (depth * 0.8, depth * 1.2)
    none    : nothing but the background range
    every other pixel takes the background range
"""
import numpy as np

F = np.float32
FAR_AWAY_MM = F(100000.0)


def slab(lo, hi, o, d):
    """Ray / box slab test: lo, hi [..., 3] broadcast against o, d [..., 3] -> t_near, t_far, valid.  1 / d first, then the two plane
    distances per axis; NaN (0 * inf) propagates through the per-axis min / max as torch.minimum / maximum do."""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1.0) / d.astype(F)
        ta = (lo.astype(F) - o.astype(F)) * inv
        tb = (hi.astype(F) - o.astype(F)) * inv
        enter = np.minimum(ta, tb).max(axis=-1)             # np.minimum / ndarray.max propagate NaN
        leave = np.maximum(ta, tb).min(axis=-1)
        valid = (leave > 0) & (leave > enter)
    return enter.astype(F), leave.astype(F), valid


def blend(zbuf, ids, source, depth_scale, bg_range, boxes=None, rays=None):
    """zbuf [K,B,HW] fp32 (mm), ids [K] int, source 'box' | 'render' | 'none', boxes [K,2,3] and rays = (o, d) each [B,HW,3] for
    'box' -> dict(z_near, z_far [B,HW] fp32, label [B,HW] int32, depth [B,HW] fp32, winner [B,HW])."""
    zbuf = np.asarray(zbuf, dtype=F)
    ids = np.asarray(ids, dtype=np.int32)
    K, B, HW = zbuf.shape
    z = np.where(zbuf > 0, zbuf, FAR_AWAY_MM)
    winner = np.argmin(z, axis=0)                           # first occurrence: ties stay with the lowest object index
    pick = lambda a: np.take_along_axis(a, winner[None], axis=0)[0]
    covered = pick(zbuf) > 0
    depth = np.where(covered, (pick(z) / F(1000.0)) * F(depth_scale), F(0.0)).astype(F)
    label = np.where(covered, ids[winner], 0).astype(np.int32)
    near = np.full((B, HW), F(bg_range[0]), dtype=F)
    far = np.full((B, HW), F(bg_range[1]), dtype=F)
    if source == "render":
        near = np.where(covered, depth * F(0.8), near).astype(F)
        far = np.where(covered, depth * F(1.2), far).astype(F)
    elif source == "box":
        boxes = np.asarray(boxes, dtype=F)
        o, d = (np.asarray(r, dtype=F) for r in rays)
        enter, leave, valid = slab(boxes[winner, 0], boxes[winner, 1], o, d)
        owned = label > 0
        near = np.where(owned, np.where(valid, enter, F(0.0)), near).astype(F)
        far = np.where(owned, np.where(valid, leave, F(0.0)), far).astype(F)
    elif source != "none":
        raise ValueError(source)
    return dict(z_near=near, z_far=far, label=label, depth=depth, winner=winner)
