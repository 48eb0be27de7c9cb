"""The four HIP entry points that texpose_amd.graph.RenderMixin reaches -- ops.raygen, NeRF.forward_samples, NeRF.composite,
ops.patch_gather -- bound to the CPU oracle (oracle/texpose_oracle.py) for the duration of a ``with`` block.  The product has
no CPU path; this is for tests of the WIRING above the kernels (tests/test_shim_cpu.py, tests/golden/check_shim_here.py), on
CPU tensors.  The oracle itself is pinned to the reference by tests/test_oracle_golden.py."""
import contextlib

import torch

from oracle import texpose_oracle as O
from texpose_amd import ops
from texpose_amd.nerf import NeRF


def raygen(intr, pose, *, H, W, n_samples=0, coords=None, ray_idx=None, z_near=None, z_far=None, rand=None,
           jitter=ops.JITTER_MID, ndc=False, depth_param="metric", seed=0, offset=0):
    """ops.raygen's training form (``coords`` [B,h,w,2]) and evaluation form (``ray_idx`` [B,R] pixel indices).  A keyword this
    stand-in does not implement (aabb, sampler, rows, offset_dev ...) is a TypeError, not a silently different render."""
    B = len(pose)
    zn, zf = z_near.reshape(B, -1, 1), z_far.reshape(B, -1, 1)
    if coords is not None:
        c, r = O.rays_train(intr, coords, pose, H, W)
        zn, zf = O.bounds_train(coords, zn, zf, H, W)
        c, r, zn, zf = c.reshape(B, -1, 3), r.reshape(B, -1, 3), zn.reshape(B, -1), zf.reshape(B, -1)
    else:
        c, r = O.rays_eval(pose, intr, H, W)
        c, r = O.gather_rows(c, ray_idx), O.gather_rows(r, ray_idx)
        zn, zf = O.gather_rows(zn, ray_idx).squeeze(-1), O.gather_rows(zf, ray_idx).squeeze(-1)
    if ndc:                                                  # (after the bounds, as the reference, :581-583)
        c, r = O.rays_to_ndc(c, r, intr)
    if rand is None and jitter == ops.JITTER_PHILOX:         # the kernel's own stream; here: the draw the reference makes at
        rand = torch.rand(B, c.shape[1], n_samples, 1)       # this point (:690-692).  Otherwise mid-point samples
    return c, r, zn, zf, O.stratified_depths(zn, zf, n_samples, rand, param=depth_param)[..., 0]


def forward_samples(self, opt, center, ray, depth_samples, latent_variable_trans=None, latent_variable_light=None, mode=None):
    p = {k: v for k, v in self.named_parameters() if k.startswith("mlp_")}
    return O.forward_samples(p, center, ray, depth_samples, latent_variable_trans, latent_variable_light)


def composite(opt, ray, rgb_samples, density_samples, depth_samples, uncert_samples=None, per_sample=True, want_prob=True,
              fan_out=None):                      # (the oracle hands out no aliases: every consumer reads rgb / density)
    return O.composite(ray, rgb_samples, density_samples, depth_samples, uncert_samples, opt.nerf.min_uncert)


def patch_gather(coords, image, image_syn, nocs, normal, obj_mask, mask_syn):
    g = O.patch_gather(coords, image, image_syn, nocs, normal, obj_mask, mask_syn)
    return torch.cat([g["image"], g["image_syn"], g["nocs_sample"], g["normal_sample"], g["mask"], g["mask_syn"]], dim=1)


@contextlib.contextmanager
def oracle_backend():
    """Patch the four entry points, restore them on the way out."""
    saved = ops.raygen, ops.patch_gather, NeRF.__dict__["forward_samples"], NeRF.__dict__["composite"]
    ops.raygen, ops.patch_gather = raygen, patch_gather
    NeRF.forward_samples, NeRF.composite = forward_samples, staticmethod(composite)
    try:
        yield
    finally:
        ops.raygen, ops.patch_gather, NeRF.forward_samples, NeRF.composite = saved
