#!/usr/bin/env python3
"""G25: the output words of the three pose refiners (tp_depth_icp_step, tp_photo_align_step, tp_pnp_refine) as the library computed
them before their Gauss-Newton phases moved into csrc/pose_gn.h.  The kernels promise outputs that are a function of the inputs alone
(every fp64 sum has one fixed order), so a later library must give the same words: tests/test_gpu_pose_gn_bits.py regenerates the
cases below from their seeds, runs the library and compares.

    python tests/golden/make_golden_g25_pose_steps.py         (GPU box; at the commit whose bits are the standard)

Only the outputs are stored (pose and rms as uint32, inliers and status as int32, the cases' images one after the other); the inputs
come from the case builders of tests/icp_ref.py, tests/photo_ref.py and tests/test_gpu_pnp.py.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (REPO, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
NAME = "g25_pose_steps"
KEYS = ("pose", "inliers", "rms", "status")
SHAPES = [(3, 3), (7, 65), (16, 16), (33, 257)]       # the single interior pixel, the guarded path with a tile tail, the vector path, two tiles


def cu(x, dtype=None):
    return None if x is None else torch.tensor(x, dtype=dtype).to(DEV)          # (a copy: some builders hand out read-only arrays)


def step_cases(builder):
    """one_step_case of either restatement over the shapes, B 1 and 3, one frame and a frame map, with and without mask; each is run
    as a step and with evaluate_only."""
    for H, W in SHAPES:
        for B in (1, 3):
            for frames in ("one", "map"):
                for with_mask in (False, True):
                    c = builder(1000 * H + 10 * W + B, B, H, W, frames, with_mask)
                    for evaluate_only in (False, True):
                        yield c, evaluate_only


def pnp_cases():
    """(xy, xyz, count, K, start, iters): test_gpu_pnp.py's refine builder at one and two reduce tiles, its first two images; then an
    image with fewer than four entries (status 1) and the rank-deficient system of all points equal (status 3)."""
    from test_gpu_pnp import refine_case
    for N in (65, 1025):
        c = refine_case(N)
        for iters in (0, 3):
            yield c["xy"][:2], c["xyz"][:2], c["count"][:2], c["K"][:2], c["start"][:2], iters
    c = refine_case(65)
    yield c["xy"][:2], c["xyz"][:2], np.array([65, 3], np.int32), c["K"][:2], c["start"][:2], 3
    c = refine_case(257)
    yield np.tile(c["xy"][:, :1], (1, 257, 1)), np.tile(c["xyz"][:, :1], (1, 257, 1)), c["count"], c["K"], c["P"], 5


def record():
    """Every case through the library -> {'<op>_<key>': the raw words of all its cases, image after image}."""
    import icp_ref
    import photo_ref
    from texpose_amd import ops
    runs = dict(depth_icp_step=[], photo_align_step=[], pnp_refine=[])
    for c, ev in step_cases(icp_ref.one_step_case):
        runs["depth_icp_step"].append(ops.depth_icp_step(cu(c["verts"]), cu(c["faces"]), cu(c["zbuf"]), cu(c["face"]), cu(c["pose"]), cu(c["K"]),
                                                         cu(c["depth"]), tau_mm=c["tau"], frame=cu(c["frame"]), mask=cu(c["mask"]), evaluate_only=ev))
    for c, ev in step_cases(photo_ref.one_step_case):
        runs["photo_align_step"].append(ops.photo_align_step(cu(c["zbuf"]), cu(c["rgb"]), cu(c["pose"]), cu(c["K"]), cu(c["image"]), tau=c["tau"],
                                                             frame=cu(c["frame"]), mask=cu(c["mask"]), evaluate_only=ev))
    for xy, xyz, count, K, start, iters in pnp_cases():
        runs["pnp_refine"].append(ops.pnp_refine(cu(xy, torch.float32), cu(xyz), cu(count, torch.int32), cu(K), cu(start, torch.float32),
                                                 tau_px=4.0, iters=iters))
    out = {}
    for op, results in runs.items():
        for k in KEYS:
            words = torch.cat([r[k].reshape(r[k].shape[0], -1) for r in results]).cpu().numpy()
            out["%s_%s" % (op, k)] = words.view(np.uint32 if words.dtype == np.float32 else np.int32)
    return out


def main():
    out = record()
    statuses = set()
    for op in ("depth_icp_step", "photo_align_step", "pnp_refine"):
        statuses |= set(out[op + "_status"].reshape(-1).tolist())
        assert out[op + "_inliers"].max() > 50, op              # the sums of more than one wave's worth of kept pixels / points
    assert statuses == {0, 1, 3}, statuses
    np.savez_compressed(os.path.join(HERE, NAME + ".npz"), **out)
    print("%s.npz: %s" % (NAME, ", ".join("%s %s" % (k, v.shape) for k, v in out.items())))


if __name__ == "__main__":
    main()
