"""The Lab chroma loss (reference layers/lab_loss.py) in plain torch ops: what `Graph.compute_loss` runs on CPU tensors when
`loss_weight.lab` is set and no module was injected, and the fp32 yardstick the K23 kernels (csrc/lab_loss.hip) are measured against.

The colour conversion restates `kornia.color.rgb_to_lab` as published (kornia is not a dependency and nothing here calls it; DESIGN
section 14): sRGB -> linear -> XYZ (D65) -> Lab, one rounded operation per step in the tensors' dtype.  One deliberate difference:
the argument of the power is replaced by 1 where the other branch of `where` is selected, so the gradient follows the selected branch
for every input -- with the published expression a channel below -0.055 puts a NaN base into the unselected power, and autograd turns
its zero cotangent into NaN."""
from __future__ import annotations

import torch

SRGB_THRESHOLD, LAB_THRESHOLD = 0.04045, 0.008856
WHITE = (0.95047, 1.0, 1.08883)


def rgb_to_lab(image: torch.Tensor) -> torch.Tensor:
    """[*,3,H,W] sRGB in [0,1] -> Lab (L in [0,100], a / b in about [-127,127])."""
    if image.dim() < 3 or image.shape[-3] != 3:
        raise ValueError("rgb_to_lab: [*,3,H,W] expected, got %s" % (tuple(image.shape),))
    gamma = image > SRGB_THRESHOLD
    base = torch.where(gamma, (image + 0.055) / 1.055, torch.ones_like(image))
    lin = torch.where(gamma, torch.pow(base, 2.4), image / 12.92)
    r, g, b = lin[..., 0, :, :], lin[..., 1, :, :], lin[..., 2, :, :]
    x = 0.412453 * r + 0.357580 * g + 0.180423 * b
    y = 0.212671 * r + 0.715160 * g + 0.072169 * b
    z = 0.019334 * r + 0.119193 * g + 0.950227 * b
    t = torch.stack([x / WHITE[0], y / WHITE[1], z / WHITE[2]], dim=-3)
    root = t > LAB_THRESHOLD
    f = torch.where(root, torch.pow(torch.where(root, t, torch.ones_like(t)).clamp(min=LAB_THRESHOLD), 1.0 / 3.0), 7.787 * t + 4.0 / 29.0)
    fx, fy, fz = f[..., 0, :, :], f[..., 1, :, :], f[..., 2, :, :]
    return torch.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)], dim=-3)


def normalize_lab(lab: torch.Tensor) -> torch.Tensor:
    """[0,100] x ~[-127,127]^2 -> [0,1]^3, NCHW (reference layers/lab_loss.py:36-48)."""
    lo = torch.tensor([0.0, -127.0, -127.0]).view(3, 1, 1).to(lab)
    hi = torch.tensor([100.0, 127.0, 127.0]).view(3, 1, 1).to(lab)
    return (lab - lo) / (hi - lo)


class LabLoss(torch.nn.Module):
    """SmoothL1 of the two normalised chroma channels, fake against real (the L channel is dropped: no lighting consideration).
    Call signature and return triple of the reference module: (loss, fake_lab with real_lab's L plane, real_lab), the maps detached."""

    def __init__(self, reduction="none"):
        super().__init__()
        self.criterion = torch.nn.SmoothL1Loss(reduction=reduction)

    normalize_lab = staticmethod(normalize_lab)

    def forward(self, fakeIm, realIm, mask=None, return_lab=True):
        fake_lab = normalize_lab(rgb_to_lab(fakeIm.contiguous()))
        real_lab = normalize_lab(rgb_to_lab(realIm.contiguous()))
        fake_vis, real_vis = fake_lab.detach().clone(), real_lab.detach().clone()
        fake_vis[:, 0] = real_vis[:, 0]
        loss = self.criterion(fake_lab[:, 1:], real_lab[:, 1:])
        loss = (loss * mask).sum() / mask.sum() if mask is not None else loss.mean()
        return (loss, fake_vis, real_vis) if return_lab else loss
