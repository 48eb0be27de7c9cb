#!/usr/bin/env python3
"""G22: the reference's smoothing of the NOCS and normal maps in its data layer (data/lm.py:497-521, Dataset.get_edge and
Dataset.smooth_geo), pinned on two small maps.

Run in the build container only:   python tests/golden/make_golden_g22_smooth_geo.py

data/lm.py is imported with make_golden's stubs (it imports with them; plyfile is stubbed as for G16) and its own get_edge and
smooth_geo are CALLED, so the edge rule (channel 0 != 0 as the mask, the four shifted comparisons, no edge from the image border
alone) and the assignment x[edges != 0] = x_blur[edges != 0] are the reference's code.  cv2 is not installed: only
cv2.medianBlur is substituted, by scipy.ndimage.median_filter(x, size=(3, 3, 1), mode="nearest") -- OpenCV documents medianBlur as
per-channel with BORDER_REPLICATE, and the median of nine values is one of them, so there is no rounding to differ in; the
substitution itself has not been run against OpenCV.

Map a (48 x 64, normal-like: floats in [-1, 1]): an ellipse that runs over the left and the top image border, a hole inside it.
Map b (50 x 62, NOCS-like: multiples of 1/255): a blob clear of the borders with pixels whose first channel is 0 inside it (the
reference treats them as outside: their covered neighbours become edges), and a one-pixel island."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG                                            # noqa: E402


def maps():
    rs = np.random.RandomState(22)
    H, W = 48, 64
    ii, jj = np.mgrid[0:H, 0:W].astype(np.float64)
    inside = ((ii - 14.0) / 22.0) ** 2 + ((jj - 12.0) / 30.0) ** 2 < 1.0          # crosses the top and the left border
    inside &= ~(((ii - 18.0) ** 2 + (jj - 20.0) ** 2) < 16.0)                      # a hole
    a = rs.uniform(-1.0, 1.0, size=(H, W, 3)).astype(np.float32)
    a[..., 0] = np.where(np.abs(a[..., 0]) < 0.05, 0.25, a[..., 0])
    a = np.where(inside[..., None], a, 0.0).astype(np.float32)
    H, W = 50, 62
    ii, jj = np.mgrid[0:H, 0:W].astype(np.float64)
    inside = ((ii - 25.0) / 17.0) ** 2 + ((jj - 30.0) / 24.0) ** 2 + 0.15 * np.sin(0.9 * ii) * np.cos(0.7 * jj) < 1.0
    q = rs.randint(1, 256, size=(H, W, 3))
    zero0 = inside & (rs.uniform(size=(H, W)) < 0.02)                               # channel 0 == 0 inside the silhouette
    q[..., 0] = np.where(zero0, 0, q[..., 0])
    q = np.where(inside[..., None], q, 0)
    q[3, 57] = (200, 17, 99)                                                        # a one-pixel island
    b = q.astype(np.float32) / 255
    return a, b, int(zero0.sum())


def main():
    MG._install_stubs()
    from scipy import ndimage
    cv2 = sys.modules["cv2"]
    cv2.medianBlur = lambda x, k: ndimage.median_filter(x, size=(k, k, 1), mode="nearest")
    sys.modules["plyfile"] = types.ModuleType("plyfile")
    sys.path.insert(0, MG.REF)
    os.chdir(MG.REF)
    import data.lm as L                                              # noqa: E402
    import surfel_reader_ref as RD                                   # noqa: E402  (the restatement, to report its agreement)
    D = L.Dataset
    me = types.SimpleNamespace(get_edge=D.get_edge)                  # smooth_geo uses nothing of `self` but get_edge
    a, b, n_zero0 = maps()
    out = {}
    for name, x in (("a", a), ("b", b)):
        edge = D.get_edge(x.copy())                                  # [H,W,3] float64, the three channels alike
        smooth = D.smooth_geo(me, x.copy())                          # (works in place on a float32 array: hand it a copy)
        assert smooth.dtype == np.float32 and (edge[..., 0] == edge[..., 1]).all() and (edge[..., 0] == edge[..., 2]).all()
        e = edge[..., 0] != 0
        changed = (smooth != x).any(-1)
        print("map %s %s: %d in mask, %d edge pixels, %d changed by the median; restatement agrees: edge %s, smooth %s"
              % (name, x.shape, int((x[..., 0] != 0).sum()), int(e.sum()), int(changed.sum()),
                 np.array_equal(RD.get_edge(x), e), np.array_equal(RD.smooth_geo(x), smooth)))
        out.update({name + "_in": x, name + "_edge": e.astype(np.uint8), name + "_out": smooth})
    print("map b: %d pixels with channel 0 == 0 inside the silhouette" % n_zero0)
    MG._save("g22_smooth_geo", **out)


if __name__ == "__main__":
    main()
