"""K39 on the GPU: ops.pose_compose and one multi-view step against the numpy restatement (tests/multiview_ref.py)
over sizes, groupings and term sets; the bit identities (identity cameras and singletons are the joint step, the terms are their
standalone evaluation, an empty or failing group passes its model through); repeatability, graph replay and guard bands; the loop on
the six two-view cases against tests/golden/multiview_loops.npz; refused arguments; tools/refine_poses.py --multiview on a written BOP
scene of three frames.  The restatement's own figures are printed by tests/test_multiview_cpu.py."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import joint_ref as JREF
import multiview_ref as MREF
import pnp_ref as PREF
import silhouette_ref as REF
from gn_ref import compare, cu, host
from test_gpu_joint import EVERYTHING, TOOL_FRAMES, TOOL_H, TOOL_OCCLUDER_OID, TOOL_OID, TOOL_W, _load_tool, _write_ply, case, device_case, same_bits, standalone, tool_scene

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "multiview_loops.npz")
OWN_KEYS = ("model", "pose", "status", "inliers", "chi2", "views")
PREFIX = dict(sil="sil_", photo="photo_", icp="icp_")
# B -> (group ids, Gr, views whose camera is [I|0] exactly): one group, singletons, interleaved, an empty group, ids out of range
GROUPINGS = {1: [([0], 1, ())],
             3: [([1, 0, 1], 2, (1,)), ([0, 2, 0], 3, ())],
             5: [([0, 0, 0, 0, 0], 1, (0,)), ([0, 1, 2, 3, 4], 5, (2,)), ([-7, 5, 1, 0, 2], 2, ())]}


def gpu_step(d, model, cam, group, subset, weights=JREF.WEIGHTS, **kw):
    from texpose_amd import ops
    _, K, terms = d
    pick = lambda name: terms[name] if name in subset else None
    up = lambda x, dtype=None: x if torch.is_tensor(x) else cu(np.asarray(x), dtype)          # (tensors as they are: a capture uploads nothing)
    return ops.multiview_align_step(up(model), up(cam), up(group, torch.int32), K, silhouette=pick("sil"), photo=pick("photo"),
                                    depth=pick("icp"), weights=weights, **kw)


def ref_step(c, model, cam, group, subset, weights=JREF.WEIGHTS, **kw):
    return MREF.step_ref(model, cam, group, c["K"], *[c[name] if name in subset else None for name in EVERYTHING], weights=weights, **kw)


def check_step(got, want, model_in, subset):
    """gn_ref.compare's bars on the group keys (no rms: NaN on both sides), views equal, chi2 to 1e-5 relative, the composed poses to
    the same bars, and each present term's own evaluation: counts and statuses equal, rms to 1e-5 relative."""
    nan = torch.full_like(got["chi2"], float("nan"))
    compare(dict(pose=got["model"], inliers=got["inliers"], status=got["status"], rms=nan), dict(want, pose=want["model"]), model_in)
    assert np.array_equal(host(got["views"]), want["views"]), (host(got["views"]), want["views"])
    chi2 = host(got["chi2"]).astype(np.float64)
    assert (np.abs(chi2 - want["chi2"]) <= 1e-5 * np.abs(want["chi2"])).all(), (chi2, want["chi2"])
    pose = host(got["pose"])
    assert np.abs(pose[:, :, :3] - want["pose"][:, :, :3]).max() <= 1e-5
    assert (np.abs(pose[:, :, 3] - want["pose"][:, :, 3]).max(1) <= 1e-5 * np.abs(want["pose"][:, :, 3]).max(1)).all()
    assert set(got) == set(OWN_KEYS) | {PREFIX[n] + k for n in subset for k in ("inliers", "rms", "status")} | ({"sil_inter", "sil_uni"} if "sil" in subset else set())
    for name in subset:
        for k in ("inliers", "status") + (("inter", "uni") if name == "sil" else ()):
            assert np.array_equal(host(got[PREFIX[name] + k]), want[name + "_" + k]), (name, k)
        rms, ref = host(got[PREFIX[name] + "rms"]).astype(np.float64), want[name + "_rms"]
        assert np.array_equal(np.isnan(rms), np.isnan(ref)), name
        ok = ~np.isnan(rms)
        assert (np.abs(rms[ok] - ref[ok]) <= 1e-5 * ref[ok] + 1e-30).all(), (name, rms, ref)


# ----------------------------------------------------------------------------- compose
def _random_pose(rs, far):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    q = q * np.sign(np.linalg.det(q))
    return np.concatenate([q, rs.uniform(-far, far, (3, 1))], 1).astype(np.float32)


def test_pose_compose_is_the_restatement_bit_for_bit():
    """130 views (three blocks of 64 threads) of 7 models: fp64 as written and one rounding, so the words are the restatement's; a
    camera of exactly [I|0] copies the model (a -0.0 survives), one with a -0.0 off the diagonal goes through the arithmetic; group ids
    out of range clamp; ``out`` is written in place and nothing around it."""
    from texpose_amd import ops
    rs = np.random.RandomState(3)
    B, Gr = 130, 7
    cam = np.stack([_random_pose(rs, 600.0) for _ in range(B)])
    model = np.stack([_random_pose(rs, 1200.0) for _ in range(Gr)])
    model[2, 0, 1] = model[0, 2, 3] = -0.0
    group = rs.randint(0, Gr, B).astype(np.int32)
    for i in (0, 63, 64, 129):
        cam[i] = MREF.IDENTITY
    cam[5] = MREF.IDENTITY
    cam[5, 1, 0] = -0.0
    group[[0, 5, 64]] = (2, 0, 0)
    group[[7, 8, 129]] = (-1, Gr, 2 ** 31 - 1)
    want = MREF.compose_ref(cam, model, group)
    band = torch.full((B + 2, 3, 4), 7.25, device=DEV)
    got = ops.pose_compose(cu(cam), cu(model), cu(group), out=band[1:B + 1])
    assert got.data_ptr() == band[1].data_ptr() and (band[0] == 7.25).all() and (band[B + 1] == 7.25).all()
    assert np.array_equal(host(got).view(np.uint32), want.view(np.uint32))
    assert same_bits(got[0], cu(model)[2]) and same_bits(got[64], cu(model)[0]) and same_bits(got[129], cu(model)[Gr - 1])
    assert np.array_equal(host(got[5]), model[0]) and not same_bits(got[5], cu(model)[0])          # (t's -0.0 + tc became +0.0)
    assert same_bits(ops.pose_compose(cu(cam), cu(model), cu(group)), got.contiguous())


# ----------------------------------------------------------------------------- one step
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("H,W", [(3, 3), (7, 65), (16, 16), (33, 257), (64, 80)])
def test_one_step_equals_the_restatement(H, W, B):
    """sil + photo at the default weights on the joint tests' hand-built planes (masks, frame maps that clamp, planted NaN / +-Inf),
    under the groupings of B: all views in one group, singletons, interleaved ids, an empty group, ids out of range; stepping, and for
    the first grouping also evaluating.  Some views have the camera [I|0] exactly, the others turn by tens of degrees."""
    key = (100 * H + W + B, B, H, W, "map", True)
    c, d = case(*key), device_case(*key)
    subset = ("sil", "photo")
    for n, (group, Gr, plain) in enumerate(GROUPINGS[B]):
        model, cam = MREF.grouped_case(c, group, Gr, 7 + n, plain)
        for evaluate_only in (False, True)[:2 if n == 0 else 1]:
            want = ref_step(c, model, cam, group, subset, evaluate_only=evaluate_only)
            check_step(gpu_step(d, model, cam, group, subset, evaluate_only=evaluate_only), want, model, subset)
        if H * W >= 33 * 257:
            members = np.bincount(np.clip(group, 0, Gr - 1), minlength=Gr)
            assert ((want["status"] == 0) == (members > 0)).all() and (want["inliers"][members > 0] > 20).all()


@pytest.mark.parametrize("subset", JREF.SUBSETS, ids="+".join)
def test_every_term_subset_at_one_size(subset):
    key = (11, 5, 33, 65, "map", True)
    c, d = case(*key), device_case(*key)
    group, Gr = MREF.GROUPINGS["an empty group"]
    model, cam = MREF.grouped_case(c, group, Gr, 3, plain=(0,))
    for evaluate_only in (False, True):
        want = ref_step(c, model, cam, group, subset, evaluate_only=evaluate_only)
        got = gpu_step(d, model, cam, group, subset, evaluate_only=evaluate_only)
        check_step(got, want, model, subset)
    assert host(got["status"])[1] == 1 and host(got["views"])[1] == 0 and host(got["chi2"])[1] == 0.0


# ----------------------------------------------------------------------------- bit identities
@pytest.mark.parametrize("B,H,W,frames,with_mask", [(3, 33, 257, "map", True), (2, 64, 80, "each", False)])
def test_identity_cameras_and_singletons_are_the_joint_step_bit_for_bit(B, H, W, frames, with_mask):
    """model_out, status, inliers and chi2 are ops.joint_align_step's; the composed poses are the models; every term's outputs and its
    part of the workspace are the term's own evaluation, stepping or evaluating."""
    from texpose_amd import ops
    d = device_case(5, B, H, W, frames, with_mask)
    pose, K, terms = d
    cam, group = np.tile(MREF.IDENTITY, (B, 1, 1)), np.arange(B)
    part = 32 * B * -(-H * W // 1024)
    for subset in (EVERYTHING, ("photo",), ("sil", "icp")):
        pick = lambda name: terms[name] if name in subset else None
        for evaluate_only, weights in ((False, JREF.WEIGHTS), (True, (3.0, 0.5, 0.5)), (False, (1.0, 1.0, 1.0))):
            joint = ops.joint_align_step(pose, K, silhouette=pick("sil"), photo=pick("photo"), depth=pick("icp"), weights=weights, evaluate_only=evaluate_only)
            ws = ops.multiview_align_workspace(B, H, W, DEV, terms=len(subset))
            assert ws.numel() == len(subset) * part + 32 * B
            ws.fill_(float("nan"))
            got = gpu_step(d, host(pose), cam, group, subset, weights, evaluate_only=evaluate_only, workspace=ws)
            assert same_bits(got["model"], joint["pose"]) and same_bits(got["pose"], joint["pose"])
            for k in ("status", "inliers", "chi2"):
                assert same_bits(got[k], joint[k]), (subset, k)
            assert torch.equal(got["views"], (joint["inliers"] > 0).to(torch.int32))
            for n, name in enumerate(subset):
                own_ws = torch.full((part,), float("nan"), dtype=torch.float64, device=DEV)
                own = standalone(d, name, own_ws, evaluate_only=True)
                for k in own:
                    if k != "pose":
                        assert same_bits(got[PREFIX[name] + k], own[k]), (name, k)
                assert same_bits(ws[n * part:(n + 1) * part], own_ws), name
            assert not torch.isnan(ws[len(subset) * part:]).any()
    own = standalone(d, "photo")                                 # one term at weight 1: that term's own step
    got = gpu_step(d, host(pose), cam, group, ("photo",), (9.0, 1.0, 9.0))
    assert same_bits(got["model"], own["pose"]) and same_bits(got["status"], own["status"]) and (own["status"] == 0).any()


def test_a_group_that_is_empty_fails_or_only_evaluates_returns_its_model_bit_for_bit():
    from texpose_amd import ops
    B, H, W = 3, 16, 24
    d = device_case(7, B, H, W, "each", False)
    pose, K, terms = d
    c = dict(pose=host(pose))
    model, cam = MREF.grouped_case(c, [0, 2, 0], 3, 9)
    group = [0, 2, 0]
    got = gpu_step(d, model, cam, group, EVERYTHING, evaluate_only=True)
    assert host(got["status"]).tolist() == [0, 1, 0] and same_bits(got["model"], cu(model)) and host(got["views"]).tolist() == [2, 0, 1]
    got = gpu_step(d, model, cam, group, EVERYTHING)
    assert host(got["status"]).tolist() == [0, 1, 0] and host(got["inliers"])[1] == 0 and host(got["chi2"])[1] == 0.0
    assert same_bits(got["model"][1], cu(model)[1]) and not same_bits(got["model"][0], cu(model)[0]) and not same_bits(got["model"][2], cu(model)[2])
    # status 1 with members: nothing rendered in view 1, the only view of group 2; views counts the views that kept a pixel
    empty = {name: dict(t, zbuf=t["zbuf"].clone()) for name, t in terms.items()}
    for t in empty.values():
        t["zbuf"][1] = -1.0
    got = gpu_step((pose, K, empty), model, cam, group, EVERYTHING)
    assert host(got["status"]).tolist() == [0, 1, 1] and host(got["views"]).tolist() == [2, 0, 0] and same_bits(got["model"][2], cu(model)[2])
    assert host(got["inliers"])[2] == 0 and not same_bits(got["model"][0], cu(model)[0])
    # status 3: a constant photograph as the only term, all views in one group
    flat = dict(zbuf=torch.full((B, H, W), 900.0, device=DEV), rgb=torch.full((B, H, W, 3), 0.5, device=DEV),
                image=torch.full((B, H, W, 3), 0.75, device=DEV), tau=0.5)
    model1, cam1 = MREF.grouped_case(c, [0, 0, 0], 1, 10)
    for evaluate_only in (False, True):
        got = ops.multiview_align_step(cu(model1), cu(cam1), cu(np.zeros(B), torch.int32), K, photo=flat, weights=(0.0, 1.0, 0.0), evaluate_only=evaluate_only)
        assert host(got["status"]).tolist() == [3] and host(got["inliers"]).tolist() == [B * (H - 2) * (W - 2)] and host(got["views"]).tolist() == [B]
        assert same_bits(got["model"], cu(model1)) and same_bits(got["pose"], ops.pose_compose(cu(cam1), cu(model1), cu(np.zeros(B), torch.int32)))


# ----------------------------------------------------------------------------- repeatability and capture
def test_two_runs_graph_replay_and_guard_bands_of_the_step():
    from texpose_amd import ops
    B, H, W = 5, 33, 257
    key = (8, B, H, W, "map", True)
    c, d = case(*key), device_case(*key)
    group, Gr = MREF.GROUPINGS["interleaved"]
    model, cam = MREF.grouped_case(c, group, Gr, 3, plain=(1,))
    model, cam, group = cu(model), cu(cam), cu(np.asarray(group), torch.int32)
    first, again = gpu_step(d, model, cam, group, EVERYTHING), gpu_step(d, model, cam, group, EVERYTHING)
    assert set(first) == set(again) and len(first) == 6 + 11
    for k in first:
        assert same_bits(first[k], again[k]), k
    assert (first["status"] == 0).all()
    ws = ops.multiview_align_workspace(B, H, W, DEV)
    out = {k: torch.empty_like(v) for k, v in first.items()}
    models, poses = torch.full((Gr + 2, 3, 4), 7.25, device=DEV), torch.full((B + 2, 3, 4), 7.25, device=DEV)      # guard bands
    out["model"], out["pose"] = models[1:Gr + 1], poses[1:B + 1]
    gpu_step(d, model, cam, group, EVERYTHING, workspace=ws, out=out)            # (warm-up on the capturing thread's allocator)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = gpu_step(d, model, cam, group, EVERYTHING, workspace=ws, out=out)
    assert all(cap[k] is out[k] for k in out)
    for _ in range(2):
        for v in out.values():
            v.view(torch.uint8).fill_(0xAB)
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k in first:
            assert same_bits(out[k].contiguous(), first[k]), k
        for band, n in ((models, Gr), (poses, B)):
            assert (band[0] == 7.25).all() and (band[n + 1] == 7.25).all()


def refiner_of(c, **kw):
    from texpose_amd import multiview
    return multiview.MultiViewRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV, vcolor=c["vcolor"], **kw)


def loop_args(c, image=True):
    return dict(mask_or_sdf=cu(c["cut"]), known=cu(c["known"]), image=cu(c["image"]) if image else None)


def test_the_whole_loop_repeats_and_replays_bit_equal():
    from texpose_amd import ops
    c = MREF.loop_inputs("bent torus", "bottom third")
    refiner = refiner_of(c, iters=6)
    model, cam, group, K, args = cu(c["model_start"]), cu(c["cam"]), cu(c["group"], torch.int32), cu(c["K"]), loop_args(c)
    first, again = refiner.refine(model, cam, group, K, **args), refiner.refine(model, cam, group, K, **args)
    keys = set(ops.MULTIVIEW_ALIGN_KEYS) | {"iou", "iou0", "iou_visible", "iou0_visible", "sil_inliers", "sil_rms", "sil_status", "sil_inter", "sil_uni",
                                            "photo_inliers", "photo_rms", "photo_status"}
    assert set(first) == keys == set(again)
    for k in first:
        assert same_bits(first[k], again[k]), k
    assert tuple(first["model"].shape) == (1, 3, 4) and tuple(first["pose"].shape) == (2, 3, 4) and tuple(first["iou"].shape) == (2,)
    assert same_bits(first["pose"], ops.pose_compose(cam, first["model"], group)) and same_bits(first["pose"][0], first["model"][0])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = refiner.refine(model, cam, group, K, **args)
    ws = refiner._workspace(2)
    for _ in range(2):
        for v in cap.values():
            v.view(torch.uint8).fill_(0xAB)
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k in first:
            assert same_bits(cap[k], first[k]), k
    assert (first["status"] == 0).all()
    # ops.multiview_align by hand on the refiner's own field: the same bits; one rasteriser call per pass over all views
    field = ops.mask_sdf(args["mask_or_sdf"], known=args["known"])
    calls, raster = [], ops.scene.mesh_raster
    def counted(*a, **kw):
        calls.append((a[2].shape[0], kw))
        return raster(*a, **kw)
    ops.scene.mesh_raster = counted
    try:
        by_hand = ops.multiview_align(cu(c["verts"]), cu(c["faces"], torch.int32), model, cam, group, K, vcolor=cu(c["vcolor"]), sdf=field,
                                      image=args["image"], iters=6, masks=dict(photo=args["known"]), visible_iou=True)
    finally:
        ops.scene.mesh_raster = raster
    assert len(calls) == 7 and all(n == 2 and kw["face_ids"] is False and kw["normals"] is False and kw["vcolor"] is not None for n, kw in calls)
    for k in first:
        assert same_bits(by_hand[k], first[k]), k


def test_the_loops_without_the_new_keyword_are_their_steps_by_hand():
    """ops.joint_align and ops.photo_align go through the same driver: each still is iters + 1 passes of mesh_raster and its own step,
    bit for bit, with the keys in the order they have had (tests/test_gpu_refine_bits.py holds their words to the recorded ones)."""
    from texpose_amd import ops
    c = JREF.table_inputs("bent sphere", "corner disc")
    verts, faces, vcolor, K, start = cu(c["verts"]), cu(c["faces"], torch.int32), cu(c["vcolor"]), cu(c["K"]), cu(c["start"])
    field, image, known = ops.mask_sdf(cu(c["cut"]), known=cu(c["known"])), cu(c["image"]), cu(c["known"])
    got = ops.joint_align(verts, faces, start, K, vcolor=vcolor, sdf=field, image=image, iters=2, masks=dict(photo=known))
    assert list(got)[:6] == ["pose", "inliers", "status", "inliers0", "chi2", "chi20"] and "model" not in got and "views" not in got
    pose = start
    for it in range(3):
        r = ops.mesh_raster(verts, faces, pose, K, H=c["H"], W=c["W"], vcolor=vcolor, face_ids=False, normals=False)
        step = ops.joint_align_step(pose, K, silhouette=dict(zbuf=r["zbuf"], sdf=field, tau_px=4.0),
                                    photo=dict(zbuf=r["zbuf"], rgb=r["rgb"], image=image, tau=0.5, mask=known), evaluate_only=it == 2)
        pose = step["pose"]
    assert same_bits(got["pose"], pose) and same_bits(got["chi2"], step["chi2"]) and same_bits(got["inliers"], step["inliers"])
    alone = ops.photo_align(verts, faces, vcolor, start, K, image, iters=2, mask=known)
    assert list(alone) == list(ops.PHOTO_ALIGN_KEYS)
    pose = start
    for it in range(3):
        r = ops.mesh_raster(verts, faces, pose, K, H=c["H"], W=c["W"], vcolor=vcolor, face_ids=False, normals=False)
        step = ops.photo_align_step(r["zbuf"], r["rgb"], pose, K, image, tau=0.5, mask=known, evaluate_only=it == 2)
        pose = step["pose"]
    assert same_bits(alone["pose"], pose) and same_bits(alone["rms"], step["rms"])


# ----------------------------------------------------------------------------- the loop cases of the golden file
@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("route", MREF.ROUTES)
@pytest.mark.parametrize("name,kind", JREF.CASES)
def test_loop_against_the_recorded_restatement(name, kind, route):
    """The six two-view cases through MultiViewRefiner.refine(known=): silhouette alone for 10 steps and silhouette + photometric at the
    default weights for 20.  The model ends within twice the restatement's recorded error plus 1e-3 degrees and 1e-3 mm (the bar of
    sections 20 and 28) with status 0, and where the restatement reports no near-tie the counts are equal."""
    c, gold = MREF.loop_inputs(name, kind), golden()
    key = "%s|%s|%s|" % (name, kind, route)
    joint = route != "silhouette 10"
    got = refiner_of(c, iters=20 if joint else 10, weights=(1.0, 100.0, 0.0)).refine(
        cu(c["model_start"]), cu(c["cam"]), cu(c["group"], torch.int32), cu(c["K"]), **loop_args(c, image=joint))
    err, want = PREF.pose_error(host(got.model)[0], c["model_true"]), gold[key + "err"]
    print("%s, %s, %s: kernel %.4f deg / %.4f mm, status %d, views %d, inliers %d | restatement %.4f deg / %.4f mm, inliers %d, near-ties %d"
          % (name, kind, route, *err, int(got.status[0]), int(got.views[0]), int(got.inliers[0]), *want, int(gold[key + "inliers"][0]),
             int(gold[key + "near_ties"][0])))
    assert int(got.status[0]) == 0 and int(got.views[0]) == 2
    assert err[0] <= 2.0 * want[0] + 1e-3 and err[1] <= 2.0 * want[1] + 1e-3, (err, want)
    if int(gold[key + "near_ties"][0]) == 0:
        assert int(got.inliers[0]) == int(gold[key + "inliers"][0]) and int(got.inliers0[0]) == int(gold[key + "inliers0"][0])


# ----------------------------------------------------------------------------- bad arguments
def test_bad_arguments_are_refused():
    from texpose_amd import _lib, ops
    B, H, W = 2, 16, 24
    d = device_case(9, B, H, W, "each", False)
    pose, K, terms = d
    sil, photo = terms["sil"], terms["photo"]
    cam, model, group = cu(np.tile(MREF.IDENTITY, (B, 1, 1))), pose.clone(), cu(np.arange(B), torch.int32)
    step = lambda model=model, cam=cam, group=group, **kw: ops.multiview_align_step(model, cam, group, K, **{**dict(silhouette=sil, photo=photo), **kw})
    step()
    for bad in (group.long(), group.float(), group[:1], torch.cat([group, group])):
        with pytest.raises(ValueError, match="group"):
            step(group=bad)
        with pytest.raises(ValueError, match="group"):
            ops.pose_compose(cam, model, bad)
    with pytest.raises(ValueError, match="Gr <= B"):
        step(model=torch.cat([model, model]))
    with pytest.raises(ValueError, match="model"):
        step(model=model[:, :, :3].contiguous())
    for bad in (cam[:, :, :3].contiguous(), cam[0], torch.cat([cam, cam])):
        with pytest.raises(ValueError, match="cam|group|zbuf"):
            step(cam=bad)
    with pytest.raises(ValueError, match="no term"):
        ops.multiview_align_step(model, cam, group, K)
    with pytest.raises(ValueError, match="weights"):
        step(weights=(1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="workspace"):
        step(workspace=ops.joint_align_workspace(B, H, W, DEV, terms=2))          # room for the terms only
    with pytest.raises(_lib.TexposeLibraryError, match="overlap"):
        step(out=dict(model=model))
    with pytest.raises(_lib.TexposeLibraryError, match="overlap"):
        ops.pose_compose(cam, model, group, out=cam)
    c = MREF.loop_inputs("bent sphere", "corner disc")
    verts, faces, Kc = cu(c["verts"]), cu(c["faces"], torch.int32), cu(c["K"])
    field = ops.mask_sdf(cu(c["cut"]))
    loop = lambda **kw: ops.multiview_align(verts, faces, cu(c["model_start"]), cu(c["cam"]), cu(c["group"], torch.int32), Kc, **kw)
    with pytest.raises(ValueError, match="pyramid= goes with the photometric term alone"):
        loop(image=cu(c["image"]), vcolor=cu(c["vcolor"]), pyramid=(1, 1), iters=2)
    with pytest.raises(ValueError, match="no term"):
        loop()
    with pytest.raises(ValueError, match="vcolor"):
        loop(sdf=field, image=cu(c["image"]))
    with pytest.raises(ValueError, match="group"):
        ops.multiview_align(verts, faces, cu(c["model_start"]), cu(c["cam"]), cu(c["group"], torch.int64), Kc, sdf=field)
    with pytest.raises(ValueError, match="Gr <= B"):
        ops.multiview_align(verts, faces, cu(np.tile(c["model_start"], (3, 1, 1))), cu(c["cam"]), cu(c["group"], torch.int32), Kc, sdf=field)


# ----------------------------------------------------------------------------- the tool
def test_tool_multiview_on_a_three_frame_scene(tmp_path, capsys):
    """The joint tool test's scene read as ONE object in the world seen by three cameras (camera 0 is the world frame, camera f is
    P_f o P_0^-1, written with BopSceneWriter(cam_w2c=)), a sphere in front hiding part of it in every frame, the estimates 8 degrees
    and 5 mm off, each on its own.  --multiview --silhouette --occluders writes a CSV tools/pose_errors.py reads; all rows of the
    object are one world pose; its mean ADD is at or below that of the same options without --multiview (the restatement's premise:
    section 29's silhouette row, 6 of 6 groups); and the three exit messages."""
    from texpose_amd import ops
    from texpose_amd.bop_scene import BopSceneWriter
    H, W, F, oid = TOOL_H, TOOL_W, TOOL_FRAMES, TOOL_OID
    verts, faces = REF.mesh_of("bent sphere")
    colours8 = np.rint(JREF.vertex_colours(verts) * 255.0).astype(np.uint8)
    K, gt, front, moved = tool_scene()
    w2c = np.stack([MREF.times(gt[f], MREF.invert(gt[0])) for f in range(F)])
    w2c[0] = np.eye(3, 4)
    root, ply, est_csv = str(tmp_path / "scene"), str(tmp_path / "obj_000007.ply"), str(tmp_path / "est.csv")
    _write_ply(ply, verts, faces, colours8)
    target = ops.mesh_raster(cu(verts), cu(faces), cu(gt), cu(K), H=H, W=W, face_ids=False, normals=False)
    whole = host(target["zbuf"]) > 0
    occ = host(ops.mesh_raster(cu(REF.mesh_of("sphere")[0]), cu(REF.mesh_of("sphere")[1]), cu(front), cu(K), H=H, W=W, face_ids=False, normals=False)["zbuf"]) > 0
    visib = np.stack([whole & ~occ, occ], 1).astype(np.uint8) * np.uint8(255)
    full = np.stack([whole, occ], 1).astype(np.uint8) * np.uint8(255)
    info = np.zeros((F, 2, 10), np.int32)
    info[:, :, 0], info[:, :, 1] = full.astype(bool).sum((2, 3)), visib.astype(bool).sum((2, 3))

    def write_scene(path, cams):
        w = BopSceneWriter(path, K, 10.0, png_per_metre=2000)
        frames = []
        for f in range(F):
            pose = gt[f].copy()
            pose[:, 3] /= 100.0
            frames += w.add_views(pose[None], [oid, TOOL_OCCLUDER_OID], info[f][None], full[f][None], visib[f][None], np.zeros((1, H, W, 3), np.uint8),
                                  np.zeros((1, H, W), np.uint16), **({} if cams is None else dict(cam_w2c=cams[f][None])))
        w.close()
        return frames
    frames = write_scene(root, w2c)
    plain_root = str(tmp_path / "plain")
    write_scene(plain_root, None)
    camera = json.load(open(os.path.join(root, "scene_camera.json")))
    assert set(camera["1"]) == {"cam_K", "depth_scale", "cam_R_w2c", "cam_t_w2c"} and np.allclose(camera["1"]["cam_t_w2c"], w2c[1][:, 3])
    assert set(json.load(open(os.path.join(plain_root, "scene_camera.json")))["1"]) == {"cam_K", "depth_scale"}          # (the default output)
    refine, errors = _load_tool("refine_poses"), _load_tool("pose_errors")
    scores = [0.3, 0.9, 0.5]
    refine.write_rows(est_csv, [(1, frames[f], oid, scores[f], moved[f, :, :3], moved[f, :, 3], 0.0) for f in range(F)])
    common = ["--ply", "%d=%s" % (oid, ply), "--est", est_csv, "--device", DEV, "--silhouette", "--occluders"]
    rows = refine.main(["--scene", root] + common + ["--out", str(tmp_path / "multi.csv"), "--multiview"])
    said_multi = capsys.readouterr().out
    refine.main(["--scene", root] + common + ["--out", str(tmp_path / "single.csv")])
    capsys.readouterr()
    assert "3 refined (0 with a failed last step)" in said_multi and "mean visible IoU" in said_multi
    # one world pose: every row composed back gives the same model to fp32 rounding
    models = [MREF.times(MREF.invert(w2c[f].astype(np.float32)), np.concatenate([rows[f][4], rows[f][5].reshape(3, 1)], 1)) for f in range(F)]
    for m in models[1:]:
        assert np.abs(m[:, :3] - models[0][:, :3]).max() <= 1e-5 and np.abs(m[:, 3] - models[0][:, 3]).max() <= 1e-5 * 1500.0
    gt_arg = ["--gt", root, "--ply", "%d=%s" % (oid, ply)]
    before, multi, single = (errors.main(gt_arg + ["--est", path])[oid] for path in (est_csv, str(tmp_path / "multi.csv"), str(tmp_path / "single.csv")))
    capsys.readouterr()
    assert multi["frames"] == sorted(frames) and not multi["missing"]
    add = lambda r: float(np.mean(r["errors"]["add"]))
    with capsys.disabled():                                      # (measured figures for DESIGN section 29)
        print("\ntool: mean ADD %.3f mm at the start, %.3f with --multiview --silhouette --occluders, %.3f without --multiview"
              % (add(before), add(multi), add(single)))
    assert add(multi) <= add(single) and add(multi) < add(before)
    # the three exit messages; nothing is written
    base = ["--ply", "%d=%s" % (oid, ply), "--device", DEV, "--out", str(tmp_path / "x.csv")]
    with pytest.raises(SystemExit, match="--multiview needs at least one of --silhouette, --rgb and --depth"):
        refine.main(["--scene", root, "--est", est_csv, "--multiview"] + base)
    with pytest.raises(SystemExit, match="has no cam_R_w2c / cam_t_w2c"):
        refine.main(["--scene", plain_root, "--est", est_csv, "--multiview", "--silhouette"] + base)
    twice = str(tmp_path / "twice.csv")
    refine.write_rows(twice, [(1, frames[f], oid, 0.5, moved[f, :, :3], moved[f, :, 3], 0.0) for f in (0, 1, 1)])
    with pytest.raises(SystemExit, match="holds two rows of object 7"):
        refine.main(["--scene", root, "--est", twice, "--multiview", "--silhouette"] + base)
    with pytest.raises(SystemExit, match="not with --multiview"):
        refine.main(["--scene", root, "--est", est_csv, "--multiview", "--rgb", "--pyramid", "5", "5"] + base)
    assert not os.path.exists(str(tmp_path / "x.csv"))
