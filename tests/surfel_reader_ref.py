"""CPU restatement of how the reference's data layer reads one frame of surfel files (data/lm.py:196-253, 497-521): the files that
texpose_amd.surfel.write_surfel_frame writes, decoded into image_syn, mask_syn, nocs_pred and normal_pred.  numpy, PIL and scipy
only (no cv2):

  * cv2.imread(-1) returns B, G, R(, A) and the data layer flips the first three back ([..., [2, 1, 0]]), so the arrays it works
    on hold the file's R, G, B in order: exactly what PIL returns;
  * image_syn = to_tensor(uint8) = uint8 -> float32 / 255 (planar); mask_syn = alpha > 0;
  * nocs_pred = smooth_geo(uint8 -> float32 / 255); normal_pred = smooth_geo(the .npz's float32 array);
  * smooth_geo(x): x[edge] = medianBlur(x, 3)[edge], with edge = get_edge(x);
  * get_edge: mask = x[..., 0] != 0; a pixel is an edge when it is in the mask and the pixel above, below, left or right of it --
    where that pixel exists -- is not (the image border alone makes no edge, nothing wraps around);
  * cv2.medianBlur(x, 3) on a 3-channel float32 image: per channel, 3x3, BORDER_REPLICATE (OpenCV's documented behaviour) =
    scipy.ndimage.median_filter(x, size=(3, 3, 1), mode="nearest").  The median of nine values is one of them, so the two agree
    exactly wherever the documented behaviour holds; OpenCV itself has not been run against this.

Golden G22 (tests/golden/make_golden_g22_smooth_geo.py) pins get_edge and smooth_geo below to the reference's own functions."""
import os

import numpy as np
from scipy import ndimage


def median3x3(x: np.ndarray) -> np.ndarray:
    """[H,W,3] float32 -> per-channel 3x3 median with replicated borders."""
    return ndimage.median_filter(np.asarray(x, np.float32), size=(3, 3, 1), mode="nearest")


def get_edge(x: np.ndarray) -> np.ndarray:
    """[H,W,3] map -> [H,W] bool: in the mask (channel 0 != 0) with a 4-neighbour inside the image outside the mask."""
    m = np.asarray(x)[:, :, 0] != 0
    out = np.zeros_like(m)                       # "some existing neighbour is outside the mask"
    out[:-1] |= ~m[1:]
    out[1:] |= ~m[:-1]
    out[:, :-1] |= ~m[:, 1:]
    out[:, 1:] |= ~m[:, :-1]
    return m & out


def smooth_geo(x: np.ndarray) -> np.ndarray:
    """[H,W,3] float32 -> a new array: edge pixels replaced by the 3x3 median of the unsmoothed map."""
    x = np.array(x, dtype=np.float32, copy=True)
    blur = median3x3(x)
    e = get_edge(x)
    x[e] = blur[e]
    return x


def quantize8(x: np.ndarray) -> np.ndarray:
    """The writer's encode followed by the reader's decode: (x * 255).astype(uint8) -> float32 / 255."""
    return (np.asarray(x, np.float32) * 255).astype(np.uint8).astype(np.float32) / 255


def decode_frame(root: str, loop, name: str) -> dict:
    """One frame written by write_surfel_frame under ``root`` for pose loop ``loop`` -> image_syn [3,H,W], mask_syn [H,W],
    nocs_pred [3,H,W], normal_pred [3,H,W] (float32 numpy), plus the [H,W] bool edge masks of the two smoothed maps and the
    unsmoothed maps (``nocs_raw`` / ``normal_raw`` [H,W,3]) so that a test can count what the smoothing changed."""
    from PIL import Image
    rgba = np.asarray(Image.open(os.path.join(root, "rgbsyn_{}".format(loop), name + ".png")))
    assert rgba.ndim == 3 and rgba.shape[2] == 4 and rgba.dtype == np.uint8
    image = (rgba[..., :3].astype(np.float32) / 255).transpose(2, 0, 1)
    alpha = (rgba[..., 3] > 0).astype(np.float32)
    nocs8 = np.asarray(Image.open(os.path.join(root, "nocs_{}".format(loop), name + ".png")))
    assert nocs8.ndim == 3 and nocs8.shape[2] == 3 and nocs8.dtype == np.uint8
    nocs_raw = nocs8.astype(np.float32) / 255
    normal_raw = np.load(os.path.join(root, "normal_{}".format(loop), name + ".npz"))["data"].astype(np.float32)
    return dict(image_syn=np.ascontiguousarray(image), mask_syn=alpha,
                nocs_pred=np.ascontiguousarray(smooth_geo(nocs_raw).transpose(2, 0, 1)),
                normal_pred=np.ascontiguousarray(smooth_geo(normal_raw).transpose(2, 0, 1)),
                nocs_edge=get_edge(nocs_raw), normal_edge=get_edge(normal_raw), nocs_raw=nocs_raw, normal_raw=normal_raw)
