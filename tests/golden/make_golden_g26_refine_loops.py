#!/usr/bin/env python3
"""G26: the output words of what g25 leaves open among the render-and-compare refiners -- tp_silhouette_align_step, tp_joint_align_step
and the four Python loops (ops.depth_icp, ops.photo_align, ops.silhouette_align, ops.joint_align, the last also through
JointRefiner.refine) -- as the library and its host layer gave them before the refiners moved behind one term table (ops/refine.py).
Their outputs are a function of the inputs alone, so a later host layer must give the same words, under the same keys in the same
order, from the same launches: tests/test_gpu_refine_bits.py regenerates the cases below, runs them and compares.

    python tests/golden/make_golden_g26_refine_loops.py         (GPU box; at the commit whose bits are the standard)

Only outputs are stored (float32 as uint32, ints as int32; a step op's cases image after image under '<op>_<key>', a loop under
'loop_<name>_<key>' with its key order as one string under 'loop_<name>_keys' and the node count of the loop captured under
torch.cuda.graph under 'loop_<name>_nodes'); the inputs come from the case builders of tests/silhouette_ref.py, tests/joint_ref.py,
tests/photo_ref.py, tests/occlusion_ref.py and tests/test_gpu_icp.py.  Only public names of texpose_amd are used.
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
NAME = "g26_refine_loops"
SHAPES = [(3, 3), (7, 65), (16, 16), (33, 257)]       # g25's: the single interior pixel, the guarded path with a tile tail, the vector path, nine tiles
JOINT_SHAPES = [(7, 65), (33, 257)]
PAIRS_AND_ALL = (("sil", "photo"), ("sil", "icp"), ("photo", "icp"), ("sil", "photo", "icp"))          # test_gpu_joint.py's
ZERO_WEIGHT = (3.0, 0.0, 0.5)                         # a present term at weight 0
CASE = ("bent torus", "bottom third")                 # the occluded image of the silhouette and the joint loops
LOOPS = ("depth_icp", "photo_align", "silhouette_align", "joint_refiner", "joint_align")


def cu(x, dtype=None):
    return None if x is None else torch.tensor(x, dtype=dtype).to(DEV)          # (a copy: some builders hand out read-only arrays)


def words(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32 if a.dtype == np.float32 else np.int32)


def silhouette_step_cases():
    """silhouette_ref.one_step_case over the shapes, B 1 and 3, one frame and a frame map, with and without mask; each is run as a
    step and with evaluate_only."""
    import silhouette_ref
    for H, W in SHAPES:
        for B in (1, 3):
            for frames in ("one", "map"):
                for with_mask in (False, True):
                    c = silhouette_ref.one_step_case(1000 * H + 10 * W + B, B, H, W, frames, with_mask)
                    for evaluate_only in (False, True):
                        yield c, evaluate_only


def joint_step_cases():
    """(pose, K, the three terms' dicts on the device, subset, weights, evaluate_only): joint_ref.one_step_case at two shapes, B = 3, a
    frame map and masks, over the pairs and all three at the restatement's weights, and all three with a present term at weight 0; then a step that fails with status 3."""
    import joint_ref
    for H, W in JOINT_SHAPES:
        c = joint_ref.one_step_case(1000 * H + 10 * W + 3, 3, H, W, "map", True)
        terms = {name: {k: cu(v) if isinstance(v, np.ndarray) else v for k, v in c[name].items() if v is not None} for name in ("sil", "photo", "icp")}
        for subset, weights in [(s, joint_ref.WEIGHTS) for s in PAIRS_AND_ALL] + [(PAIRS_AND_ALL[-1], ZERO_WEIGHT)]:
            for evaluate_only in (False, True):
                yield cu(c["pose"]), cu(c["K"]), terms, subset, weights, evaluate_only
    # status 3, which none of the cases above reaches: a constant photograph as the only term, every gradient zero
    B, H, W = 3, 16, 24
    c = joint_ref.one_step_case(7, B, H, W, "each", False)
    flat = dict(zbuf=torch.full((B, H, W), 900.0, device=DEV), rgb=torch.full((B, H, W, 3), 0.5, device=DEV),
                image=torch.full((B, H, W, 3), 0.75, device=DEV), tau=0.5)
    for evaluate_only in (False, True):
        yield cu(c["pose"]), cu(c["K"]), dict(photo=flat), ("photo",), (0.0, 1.0, 0.0), evaluate_only


def loop_runs():
    """name -> run(cull): the five loops on the 64 x 80, B = 2 builders, every tensor on the device before the first call."""
    import joint_ref
    import occlusion_ref
    import photo_ref
    import silhouette_ref
    from test_gpu_icp import loop_case
    from texpose_amd import joint, ops
    runs = {}
    c = loop_case("sphere", True)
    icp = (cu(c["verts"]), cu(c["faces"]), cu(c["start"]), cu(c["K"]), cu(c["depth"]))
    runs["depth_icp"] = lambda cull: ops.depth_icp(*icp, tau_mm=20.0, iters=5, damping=1e-6, cull=cull)
    c = photo_ref.loop_inputs("sphere", True)
    photo = (cu(c["verts"]), cu(c["faces"]), cu(c["vcolor"]), cu(c["start"]), cu(c["K"]), cu(c["image"]))
    runs["photo_align"] = lambda cull: ops.photo_align(*photo, tau=0.5, iters=10, damping=1e-6, cull=cull)
    c = occlusion_ref.occluded_inputs(*CASE)
    field = ops.mask_sdf(cu(c["cut"][::-1].copy()), known=cu(c["known"][::-1].copy()))          # the planes in reverse, found again by the map
    sil = (cu(c["verts"]), cu(c["faces"]), cu(c["start"]), cu(c["K"]), field)
    frame = cu(np.array([1, 0], np.int32))
    runs["silhouette_align"] = lambda cull: ops.silhouette_align(*sil, tau_px=4.0, iters=10, damping=1e-6, frame=frame, visible_iou=True, cull=cull)
    c = joint_ref.table_inputs(*CASE)
    refiners = {cull: joint.JointRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV, vcolor=c["vcolor"], iters=6, cull=cull) for cull in (False, True)}
    start, K, cut, known, image = cu(c["start"]), cu(c["K"]), cu(c["cut"]), cu(c["known"]), cu(c["image"])
    runs["joint_refiner"] = lambda cull: refiners[cull].refine(start, K, mask_or_sdf=cut, known=known, image=image)
    # all three terms: the depth plane is the brute-force zbuf at the true pose (background 0), masked by ``known``; a schedule of tau_px
    depth = cu(np.maximum(np.stack([silhouette_ref.render_ref(CASE[0], c["P"][b], c["K"][b], c["H"], c["W"]) for b in range(2)]), 0.0).astype(np.float32))
    mesh = (cu(c["verts"]), cu(c["faces"], torch.int32))
    vcolor, whole = cu(c["vcolor"]), ops.mask_sdf(cut, known=known)
    tau_px = [8.0, 6.0, 6.0, 4.0, 4.0, 4.0, 4.0]
    runs["joint_align"] = lambda cull: ops.joint_align(*mesh, start, K, vcolor=vcolor, sdf=whole, image=image, depth=depth, tau_px=tau_px, iters=6,
                                                       masks=dict(depth=known), visible_iou=True, cull=cull)
    assert tuple(runs) == LOOPS
    return runs


def captured_nodes(run):
    """The node count of ``run`` captured under torch.cuda.graph (after an eager run on the capturing thread's allocator): the launch
    sequence, which is the speed that matters under replay."""
    from texpose_amd import ops
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
        nodes = ops.capture_node_count()
    torch.cuda.synchronize()
    return int(nodes)


def record():
    """Every case through the library -> {'<op>_<key>': the raw words of all its cases that return the key, image after image} and
    the loops' words, key orders and captured node counts."""
    from texpose_amd import ops
    runs = dict(silhouette_align_step=[], joint_align_step=[])
    for c, ev in silhouette_step_cases():
        runs["silhouette_align_step"].append(ops.silhouette_align_step(cu(c["zbuf"]), cu(c["pose"]), cu(c["K"]), cu(c["sdf"]), tau_px=c["tau"],
                                                                       frame=cu(c["frame"]), mask=cu(c["mask"]), evaluate_only=ev))
    for pose, K, terms, subset, weights, ev in joint_step_cases():
        pick = lambda name: terms[name] if name in subset else None
        runs["joint_align_step"].append(ops.joint_align_step(pose, K, silhouette=pick("sil"), photo=pick("photo"), depth=pick("icp"), weights=weights,
                                                             evaluate_only=ev))
    out = {}
    for op, results in runs.items():
        for k in sorted(set().union(*results)):
            out["%s_%s" % (op, k)] = words(torch.cat([r[k].reshape(r[k].shape[0], -1) for r in results if k in r]))
    for name, run in loop_runs().items():
        plain, culled = run(False), run(True)
        assert tuple(plain) == tuple(culled), name
        for k, v in plain.items():
            out["loop_%s_%s" % (name, k)] = words(v.reshape(v.shape[0], -1))
            assert np.array_equal(out["loop_%s_%s" % (name, k)], words(culled[k].reshape(v.shape[0], -1))), (name, k, "cull=True changes the words")
        out["loop_%s_keys" % name] = np.array(" ".join(tuple(plain)))
        out["loop_%s_nodes" % name] = np.array([captured_nodes(lambda: run(False))], np.int32)
    return out


def main():
    out = record()
    statuses = set()
    for op in ("silhouette_align_step", "joint_align_step"):
        statuses |= set(out[op + "_status"].reshape(-1).tolist())
        print("%s: statuses %s, most inliers %d" % (op, sorted(set(out[op + "_status"].reshape(-1).tolist())), out[op + "_inliers"].max()))
    for name in LOOPS:
        print("loop %s: status %s, %d nodes, keys %s" % (name, out["loop_%s_status" % name].reshape(-1).tolist(), out["loop_%s_nodes" % name][0],
                                                         out["loop_%s_keys" % name]))
    assert statuses == {0, 1, 3}, statuses
    assert all((out["loop_%s_status" % name] == 0).all() for name in LOOPS)
    assert max(out[op + "_inliers"].max() for op in ("silhouette_align_step", "joint_align_step")) > 50     # more than one wave's worth of kept pixels
    np.savez_compressed(os.path.join(HERE, NAME + ".npz"), **out)
    print("%s.npz: %s" % (NAME, ", ".join("%s %s" % (k, v.shape) for k, v in out.items())))


if __name__ == "__main__":
    main()
