"""numpy statement of the scene-annotation rules (tp_scene_annotate, tp_view_images; DESIGN "Novel views as a BOP scene"), for the tests.

    all_k(p)   = zbuf[k,b,p] > 0                       (mm; <= 0 and NaN are background)
    visib_k(p) = all_k(p) and label[b,p] == ids[k]
    info[b,k]  = count of all_k, count of visib_k, then xmin, ymin, xmax, ymax of all_k and the same four of visib_k: inclusive pixel
                 indices, x the column and y the row; an empty set reports -1 four times
    mask, mask_visib = 255 where the set holds, else 0

    rgb8    = uint8(trunc(clamp(rgb, 0, 1) * 255))                                         each step one rounded fp32 operation;
    depth16 = uint16(trunc(clamp((depth / depth_scale) * png_per_metre, 0, 65535)))        NaN gives 0
"""
import numpy as np

F = np.float32


def extent(m):
    """m [H,W] bool -> [xmin, ymin, xmax, ymax], or four times -1."""
    ys, xs = np.nonzero(m)
    if xs.size == 0:
        return [-1, -1, -1, -1]
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]


def annotate(zbuf, label, ids):
    """zbuf [K,B,H,W] fp32, label [B,H*W] or [B,H,W] int, ids [K] -> info [B,K,10] int32, mask and mask_visib [B,K,H,W] uint8."""
    zbuf = np.asarray(zbuf, dtype=F)
    K, B, H, W = zbuf.shape
    label = np.asarray(label).reshape(B, H, W)
    ids = np.asarray(ids).reshape(K)
    info = np.zeros((B, K, 10), dtype=np.int32)
    mask = np.zeros((B, K, H, W), dtype=np.uint8)
    mask_visib = np.zeros((B, K, H, W), dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        covered = zbuf > 0                                           # False for NaN
    for b in range(B):
        for k in range(K):
            full = covered[k, b]
            vis = full & (label[b] == ids[k])
            info[b, k] = [int(full.sum()), int(vis.sum())] + extent(full) + extent(vis)
            mask[b, k] = np.where(full, 255, 0)
            mask_visib[b, k] = np.where(vis, 255, 0)
    return info, mask, mask_visib


def rgb8(rgb, H, W):
    """rgb [B,H*W,3] fp32 -> [B,H,W,3] uint8."""
    x = np.asarray(rgb, dtype=F)
    with np.errstate(invalid="ignore"):
        x = np.where(x > 0, x, F(0))                                 # NaN -> 0
        x = np.where(x < 1, x, F(1))
    v = (x * F(255)).astype(F)
    return np.trunc(v).astype(np.int64).astype(np.uint8).reshape(x.shape[0], H, W, 3)


def depth16(depth, H, W, depth_scale, png_per_metre=2000.0):
    """depth [B,H*W] fp32 in NeRF units -> [B,H,W] uint16."""
    d = np.asarray(depth, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        m = ((d / F(depth_scale)).astype(F) * F(png_per_metre)).astype(F)
        m = np.where(m > 0, m, F(0))                                 # NaN -> 0
        m = np.where(m < 65535, m, F(65535))
    return np.trunc(m).astype(np.int64).astype(np.uint16).reshape(d.shape[0], H, W)
