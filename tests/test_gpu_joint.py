"""K33 on the GPU: one joint step against the numpy restatement (tests/joint_ref.py) over the term sets, shapes,
masks and frame maps; the bit identities (each term's outputs and records are its standalone evaluation's, one term at weight 1 is
that term's own step, weight 0 is absent, a failed or evaluating step passes the pose through); repeatability and graph replay of the
step and of the whole loop; the loop on the twelve occluded images through JointRefiner.refine(known=); refused arguments;
tools/refine_poses.py --joint on a written BOP scene of two instances.  The restatement's own figures are printed by
tests/test_joint_cpu.py."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import joint_ref as JREF
import pnp_ref as PREF
import silhouette_ref as REF
from gn_ref import compare, cu, host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVERYTHING = ("sil", "photo", "icp")
PAIRS_AND_ALL = (("sil", "photo"), ("sil", "icp"), ("photo", "icp"), EVERYTHING)
JOINT_KEYS = ("pose", "inliers", "status", "chi2")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ----------------------------------------------------------------------------- the one-step cases on the device
@functools.lru_cache(maxsize=None)
def case(seed, B, H, W, frames, with_mask):
    c = JREF.one_step_case(seed, B, H, W, frames, with_mask)
    for term in EVERYTHING:
        for v in c[term].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def device_case(seed, B, H, W, frames, with_mask):
    """The case's tensors on the device, made once: pose, K and per term the dict ops.joint_align_step takes."""
    c = case(seed, B, H, W, frames, with_mask)
    dtype = dict(faces=torch.int32, face=torch.int32, frame=torch.int32, mask=torch.uint8)
    up = lambda v, t=None: cu(v.copy(), t)                       # (the cached arrays are read-only: hand torch a copy)
    terms = {name: {k: up(v, dtype.get(k)) if isinstance(v, np.ndarray) else v for k, v in c[name].items() if v is not None} for name in EVERYTHING}
    return up(c["pose"]), up(c["K"]), terms


def gpu_step(d, subset, weights=JREF.WEIGHTS, **kw):
    from texpose_amd import ops
    pose, K, terms = d
    pick = lambda name: terms[name] if name in subset else None
    return ops.joint_align_step(pose, K, silhouette=pick("sil"), photo=pick("photo"), depth=pick("icp"), weights=weights, **kw)


def ref_step(c, subset, weights=JREF.WEIGHTS, **kw):
    return JREF.step_ref(c["pose"], c["K"], *[c[name] if name in subset else None for name in EVERYTHING], weights=weights, **kw)


def check_step(got, want, pose_in, subset):
    """gn_ref.compare's bars on the joint keys (the joint step has no rms: NaN on both sides), chi2 to 1e-5 relative, and each present
    term's own evaluation: counts and statuses equal, rms to 1e-5 relative."""
    compare(dict(got, rms=torch.full_like(got["chi2"], float("nan"))), want, pose_in)
    chi2 = host(got["chi2"]).astype(np.float64)
    assert (np.abs(chi2 - want["chi2"]) <= 1e-5 * np.abs(want["chi2"])).all(), (chi2, want["chi2"])
    prefix = dict(sil="sil_", photo="photo_", icp="icp_")
    assert set(got) == set(JOINT_KEYS) | {prefix[n] + k for n in subset for k in ("inliers", "rms", "status")} | ({"sil_inter", "sil_uni"} if "sil" in subset else set())
    for name in subset:
        for k in ("inliers", "status") + (("inter", "uni") if name == "sil" else ()):
            assert np.array_equal(host(got[prefix[name] + k]), want[name + "_" + k]), (name, k)
        rms, ref = host(got[prefix[name] + "rms"]).astype(np.float64), want[name + "_rms"]
        assert np.array_equal(np.isnan(rms), np.isnan(ref)), name
        ok = ~np.isnan(rms)
        assert (np.abs(rms[ok] - ref[ok]) <= 1e-5 * ref[ok] + 1e-30).all(), (name, rms, ref)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(3, 3), (7, 65), (16, 16), (33, 257), (64, 80)])
def test_one_step_equals_the_restatement(H, W, B):
    """sil + photo, sil + icp, photo + icp and all three at the default weights, once on plain planes (Ft = 1, no masks) and once with
    masks and frame maps whose entries lie out of range and clamp; every case holds planted NaN / +-Inf in zbuf, colours, field and
    depth and bad face indices, as the terms' own tests.  64 x 80 takes the terms' 16-byte routes, 33 x 257 nine tiles."""
    kept = 0
    for frames, with_mask in (("one", False), ("map", True)):
        key = (100 * H + W + B, B, H, W, frames, with_mask)
        c, d = case(*key), device_case(*key)
        for subset in PAIRS_AND_ALL:
            for evaluate_only in (False, True):
                want = ref_step(c, subset, evaluate_only=evaluate_only)
                check_step(gpu_step(d, subset, evaluate_only=evaluate_only), want, c["pose"], subset)
            kept += int(want["inliers"].sum())
            if H * W >= 33 * 257:
                assert (want["status"] == 0).all() and (want["inliers"] > 30).all(), subset
    assert kept > 0 or H * W == 9


# ----------------------------------------------------------------------------- bit identities
def standalone(d, name, ws=None, **kw):
    from texpose_amd import ops
    pose, K, terms = d
    t = dict(terms[name])
    if name == "sil":
        return ops.silhouette_align_step(t.pop("zbuf"), pose, K, t.pop("sdf"), workspace=ws, **t, **kw)
    if name == "photo":
        return ops.photo_align_step(t.pop("zbuf"), t.pop("rgb"), pose, K, t.pop("image"), workspace=ws, **t, **kw)
    return ops.depth_icp_step(t.pop("verts"), t.pop("faces"), t.pop("zbuf"), t.pop("face"), pose, K, t.pop("depth"), workspace=ws, **t, **kw)


@pytest.mark.parametrize("B,H,W,frames,with_mask", [(3, 33, 257, "map", True), (2, 64, 80, "each", False)])
def test_terms_are_their_standalone_evaluation_bit_for_bit(B, H, W, frames, with_mask):
    """Each present term's inliers, rms, status (inter, uni) and the records in its part of the workspace are those of the term's own
    step with evaluate_only, whatever the weights and whether the joint call steps or evaluates."""
    from texpose_amd import ops
    key = (5, B, H, W, frames, with_mask)
    d = device_case(*key)
    sizes = [int(f(B, H, W).numel()) for f in (lambda *a: ops.silhouette_align_workspace(*a, DEV), lambda *a: ops.photo_align_workspace(*a, DEV),
                                                lambda *a: ops.depth_icp_workspace(*a, DEV))]
    assert sizes[0] == sizes[1] == sizes[2] == 32 * B * -(-H * W // 1024)
    ws = ops.joint_align_workspace(B, H, W, DEV)
    assert ws.numel() == 3 * sizes[0]
    prefix = dict(sil="sil_", photo="photo_", icp="icp_")
    for evaluate_only, weights in ((False, JREF.WEIGHTS), (True, (3.0, 0.0, 0.5))):
        ws.fill_(float("nan"))
        got = gpu_step(d, EVERYTHING, weights, evaluate_only=evaluate_only, workspace=ws)
        for n, name in enumerate(EVERYTHING):
            own_ws = torch.full((sizes[0],), float("nan"), dtype=torch.float64, device=DEV)
            own = standalone(d, name, own_ws, evaluate_only=True)
            for k in own:
                if k != "pose":
                    assert same_bits(got[prefix[name] + k], own[k]), (name, k)
            assert same_bits(ws[n * sizes[0]:(n + 1) * sizes[0]], own_ws), name
            assert same_bits(own["pose"], d[0])


@pytest.mark.parametrize("B,H,W,frames,with_mask", [(3, 33, 257, "map", True), (1, 16, 16, "one", False), (2, 64, 80, "each", False)])
def test_one_term_at_weight_one_is_that_terms_own_step(B, H, W, frames, with_mask):
    """pose and status bit for bit, as the only term present and beside terms of weight 0; and weight 0 equals absent in the joint
    keys."""
    d = device_case(6, B, H, W, frames, with_mask)
    stepped = 0
    for n, name in enumerate(EVERYTHING):
        own = standalone(d, name)
        one = tuple(1.0 if k == n else 0.0 for k in range(3))
        alone, beside = gpu_step(d, (name,), tuple(1.0 if k == n else 9.0 for k in range(3))), gpu_step(d, EVERYTHING, one)
        for got in (alone, beside):
            assert same_bits(got["pose"], own["pose"]) and same_bits(got["status"], own["status"]) and same_bits(got["inliers"], own["inliers"]), name
        stepped += int((own["status"] == 0).sum())
        assert not same_bits(own["pose"], d[0]) or (own["status"] != 0).all()
    assert stepped > 0
    for absent, weights in ((("icp",), (1.0, 100.0, 0.0)), (("sil",), (0.0, 100.0, 0.04)), (("photo", "icp"), (2.0, 0.0, 0.0))):
        with_zero, without = gpu_step(d, EVERYTHING, weights), gpu_step(d, tuple(n for n in EVERYTHING if n not in absent), weights)
        for k in JOINT_KEYS:
            assert same_bits(with_zero[k], without[k]), (absent, k)


def test_a_step_that_fails_or_only_evaluates_returns_the_pose_bit_for_bit():
    from texpose_amd import ops
    B, H, W = 3, 16, 24
    d = device_case(7, B, H, W, "each", False)
    pose, K, terms = d
    # evaluate_only: statuses 0, the pose untouched
    got = gpu_step(d, EVERYTHING, evaluate_only=True)
    assert (got["status"] == 0).all() and same_bits(got["pose"], pose)
    # status 1: nothing rendered in image 1 (fewer than six rows over all terms), the others step
    empty = {name: dict(t, zbuf=t["zbuf"].clone()) for name, t in terms.items()}
    for t in empty.values():
        t["zbuf"][1] = -1.0
    got = gpu_step((pose, K, empty), EVERYTHING)
    assert host(got["status"]).tolist() == [0, 1, 0] and host(got["inliers"])[1] == 0 and host(got["chi2"])[1] == 0.0
    assert same_bits(got["pose"][1], pose[1]) and not same_bits(got["pose"][0], pose[0]) and not same_bits(got["pose"][2], pose[2])
    # status 3: a constant photograph as the only term: every gradient is zero, the system is not positive definite
    flat = dict(zbuf=torch.full((B, H, W), 900.0, device=DEV), rgb=torch.full((B, H, W, 3), 0.5, device=DEV),
                image=torch.full((B, H, W, 3), 0.75, device=DEV), tau=0.5)
    for evaluate_only in (False, True):
        got = ops.joint_align_step(pose, K, photo=flat, weights=(0.0, 1.0, 0.0), evaluate_only=evaluate_only)
        assert (got["status"] == 3).all() and (got["inliers"] == (H - 2) * (W - 2)).all() and same_bits(got["pose"], pose)
        assert torch.allclose(got["chi2"], torch.full((B,), 3 * 0.0625 * (H - 2) * (W - 2), device=DEV), rtol=1e-6)
    # ... and beside a silhouette term it is the outline that steps
    got = ops.joint_align_step(pose, K, silhouette=terms["sil"], photo=dict(flat, zbuf=terms["sil"]["zbuf"]), weights=(1.0, 1.0, 0.0))
    own = standalone(d, "sil")
    ok = own["status"] == 0                                      # (the constant photograph adds zeros to J^T J and J^T r)
    assert ok.all() and (got["status"] == 0).all() and same_bits(got["pose"], own["pose"]) and (got["inliers"] > own["inliers"]).all()


# ----------------------------------------------------------------------------- repeatability and capture
def test_two_runs_and_graph_replay_of_the_step_are_bit_equal():
    from texpose_amd import ops
    B, H, W = 3, 33, 257
    d = device_case(8, B, H, W, "map", True)
    first, again = gpu_step(d, EVERYTHING), gpu_step(d, EVERYTHING)
    assert set(first) == set(again) and len(first) == 15
    for k in first:
        assert same_bits(first[k], again[k]), k
    ws = ops.joint_align_workspace(B, H, W, DEV)
    out = {k: torch.empty_like(v) for k, v in first.items()}
    gpu_step(d, EVERYTHING, workspace=ws, out=out)                   # (warm-up on the capturing thread's allocator)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = gpu_step(d, EVERYTHING, workspace=ws, out=out)
    assert all(cap[k] is out[k] for k in out)
    for _ in range(2):
        for v in out.values():
            v.view(torch.uint8).fill_(0xAB)
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k in first:
            assert same_bits(out[k], first[k]), k
    assert (first["status"] == 0).all()


# ----------------------------------------------------------------------------- the loop
def refiner_of(c, **kw):
    from texpose_amd import joint
    return joint.JointRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV, vcolor=c["vcolor"], **kw)


def loop_args(c):
    return dict(mask_or_sdf=cu(c["cut"]), known=cu(c["known"]), image=cu(c["image"]))


@pytest.mark.parametrize("name,kind", JREF.CASES)
def test_loop_converges_on_the_occluded_images(name, kind):
    """The table's twelve images through JointRefiner.refine(known=), silhouette + photometric at the default weights, 20 steps from 8
    degrees: each ends within 1 degree and 5 mm with status 0 (the restatement's own worst is 0.28 deg / 2.41 mm), and at a higher
    visible IoU than SilhouetteRefiner reaches on the same masks and start.  Kernel and restatement are printed side by side."""
    from texpose_amd import ops, silhouette
    c = JREF.table_inputs(name, kind)
    got = refiner_of(c).refine(cu(c["start"]), cu(c["K"]), **loop_args(c))
    outline = silhouette.SilhouetteRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV, tau_px=4.0, iters=10, damping=1e-6)
    alone = outline.refine(cu(c["start"]), cu(c["K"]), cu(c["cut"]), known=cu(c["known"]))
    want = JREF.table_route(name, kind, "joint 20, w_photo 100")
    keys = set(ops.JOINT_ALIGN_KEYS) | {"iou", "iou0", "iou_visible", "iou0_visible", "sil_inliers", "sil_rms", "sil_status", "sil_inter", "sil_uni",
                                        "photo_inliers", "photo_rms", "photo_status"}
    assert set(got) == keys
    err = [PREF.pose_error(host(got.pose)[b], c["P"][b]) for b in range(2)]
    for b in range(2):
        print("%s %d, %s (%.2f visible): kernel %.3f deg / %.3f mm, status %d, visible IoU %.4f -> %.4f | restatement %.3f deg / %.3f mm, status %d | "
              "silhouette alone visible IoU %.4f" % (name, b, kind, c["visible"][b], *err[b], int(got.status[b]), float(got.iou0_visible[b]),
                                                     float(got.iou_visible[b]), *want["err"][b], want["status"][b], float(alone.iou_visible[b])))
    for b in range(2):
        assert int(got.status[b]) == 0 and err[b][0] <= 1.0 and err[b][1] <= 5.0, (b, err[b])
        assert float(got.iou_visible[b]) > float(alone.iou_visible[b]), b
        assert same_bits(got.iou0_visible[b:b + 1], alone.iou0_visible[b:b + 1])          # (the same start, the same field)


def test_the_whole_loop_repeats_and_replays_bit_equal():
    from texpose_amd import ops
    c = JREF.table_inputs("bent torus", "bottom third")
    refiner = refiner_of(c, iters=6)
    start, K, args = cu(c["start"]), cu(c["K"]), loop_args(c)
    first, again = refiner.refine(start, K, **args), refiner.refine(start, K, **args)
    assert set(first) == set(again)
    for k in first:
        assert same_bits(first[k], again[k]), k
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = refiner.refine(start, K, **args)
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
    # ops.joint_align by hand on the refiner's own field: the same bits; and one rasteriser call per pass, asked for no more than the
    # present terms need
    field = ops.mask_sdf(args["mask_or_sdf"], known=args["known"])
    calls, raster = [], ops.scene.mesh_raster
    def counted(*a, **kw):
        calls.append(kw)
        return raster(*a, **kw)
    ops.scene.mesh_raster = counted
    try:
        by_hand = ops.joint_align(cu(c["verts"]), cu(c["faces"], torch.int32), start, K, vcolor=cu(c["vcolor"]), sdf=field, image=args["image"],
                                  iters=6, masks=dict(photo=args["known"]), visible_iou=True)
    finally:
        ops.scene.mesh_raster = raster
    assert len(calls) == 7 and all(kw["face_ids"] is False and kw["normals"] is False and kw["vcolor"] is not None for kw in calls)
    for k in first:
        assert same_bits(by_hand[k], first[k]), k


# ----------------------------------------------------------------------------- bad arguments
def test_bad_arguments_are_refused():
    from texpose_amd import _lib, ops
    B, H, W = 2, 16, 24
    d = device_case(9, B, H, W, "each", False)
    pose, K, terms = d
    sil, photo, icp = terms["sil"], terms["photo"], terms["icp"]
    step = lambda **kw: ops.joint_align_step(pose, K, **kw)
    with pytest.raises(ValueError, match="no term"):
        step()
    for bad in ((1.0, -1.0, 1.0), (float("nan"), 1.0, 1.0), (1.0, 1.0, float("inf"))):
        with pytest.raises(ValueError, match="weights"):
            step(silhouette=sil, photo=photo, weights=bad)
    with pytest.raises(ValueError, match="weight > 0"):
        step(silhouette=sil, photo=photo, weights=(0.0, 0.0, 1.0))
    # a shape or dtype that differs between the terms
    with pytest.raises(ValueError, match="zbuf"):
        step(silhouette=sil, photo=dict(photo, zbuf=photo["zbuf"][:, :-1].contiguous()))
    with pytest.raises(ValueError, match="zbuf"):
        step(silhouette=sil, photo=dict(photo, zbuf=photo["zbuf"].double()))
    with pytest.raises(ValueError, match="rgb"):
        step(silhouette=sil, photo=dict(photo, rgb=photo["rgb"][:1]))
    with pytest.raises(ValueError, match="face"):
        step(silhouette=sil, depth=dict(icp, face=icp["face"].long()))
    with pytest.raises(ValueError, match="sdf"):
        step(silhouette=dict(sil, sdf=sil["sdf"][:, :, :-1].contiguous()), photo=photo)
    with pytest.raises(ValueError, match="missing"):
        step(silhouette={k: v for k, v in sil.items() if k != "tau_px"}, photo=photo)
    with pytest.raises(ValueError, match="unknown"):
        step(silhouette=dict(sil, tau=1.0), photo=photo)
    with pytest.raises(_lib.TexposeLibraryError, match="tau"):
        step(silhouette=sil, photo=dict(photo, tau=-1.0))
    with pytest.raises(_lib.TexposeLibraryError, match="overlap"):
        step(silhouette=sil, photo=photo, out=dict(pose=pose))
    with pytest.raises(ValueError, match="workspace"):
        step(silhouette=sil, photo=photo, workspace=ops.silhouette_align_workspace(B, H, W, DEV))          # room for one term only
    # the loop and the refiner
    c = JREF.table_inputs("bent sphere", "corner disc")
    verts, faces, start, Kc = cu(c["verts"]), cu(c["faces"], torch.int32), cu(c["start"]), cu(c["K"])
    field = ops.mask_sdf(cu(c["cut"]))
    with pytest.raises(ValueError, match="vcolor"):
        ops.joint_align(verts, faces, start, Kc, sdf=field, image=cu(c["image"]))
    with pytest.raises(ValueError, match="no term"):
        ops.joint_align(verts, faces, start, Kc)
    with pytest.raises(ValueError, match="one size"):
        ops.joint_align(verts, faces, start, Kc, vcolor=cu(c["vcolor"]), sdf=field, image=cu(c["image"])[:, :-1].contiguous())
    with pytest.raises(ValueError, match="weights"):
        ops.joint_align(verts, faces, start, Kc, sdf=field, weights=(-1.0, 1.0, 1.0))
    refiner = refiner_of(c)
    with pytest.raises(ValueError, match="known"):
        refiner.refine(start, Kc, mask_or_sdf=field, known=cu(c["known"]), image=cu(c["image"]))          # a field together with known
    with pytest.raises(ValueError, match="known"):
        refiner.refine(start, Kc, known=cu(c["known"]), image=cu(c["image"]))
    from texpose_amd import joint
    with pytest.raises(ValueError, match="vcolor"):
        joint.JointRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV).refine(start, Kc, mask_or_sdf=cu(c["cut"]), image=cu(c["image"]))


# ----------------------------------------------------------------------------- the tool
TOOL_H, TOOL_W, TOOL_FRAMES, TOOL_OID, TOOL_OCCLUDER_OID = 120, 160, 3, 7, 9


def tool_scene():
    """DESIGN section 22's scene: three poses of the bent sphere about 900 mm away and, per frame, the unbent sphere 700 mm away, down and
    to the right of it in the image, hiding its lower right -> K, gt [3,3,4], occluder poses [3,3,4], estimates (8 deg, 5 mm off)."""
    K = PREF.end_to_end_inputs("sphere")["K"].copy()
    K[:2] *= TOOL_H / 64.0
    rs = np.random.RandomState(8)
    gt = []
    for _ in range(TOOL_FRAMES):
        q, _r = np.linalg.qr(rs.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        gt.append(np.concatenate([q, rs.uniform(-15, 15, (3, 1)) + [[0.0], [0.0], [900.0]]], 1))
    gt = np.stack(gt).astype(np.float32)
    front = np.tile(np.eye(3, 4, dtype=np.float32), (TOOL_FRAMES, 1, 1))
    front[:, :, 3] = gt[:, :, 3] * np.float32(700.0 / 900.0) + np.array([55.0, 45.0, 0.0], np.float32)
    moved = REF.perturbed(gt, np.random.RandomState(5), angle_deg=JREF.START_DEG).astype(np.float64)
    for f in range(TOOL_FRAMES):
        d = moved[f, :, 3] - gt[f, :, 3]
        moved[f, :, 3] = gt[f, :, 3] + d * 5.0 / np.linalg.norm(d)
    return K, gt, front, moved


def _write_ply(path, verts, faces, colours):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\n"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces)))
        for p, c in zip(verts, colours):
            f.write("%r %r %r %d %d %d\n" % (*(float(v) for v in p), *(int(v) for v in c)))
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(int(v) for v in t))


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(REPO, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_joint_beats_the_sequential_route_on_an_occluded_object(tmp_path, capsys):
    """Section 22's scene of two instances, the bent sphere coloured (8-bit colours, as a PLY holds them) and rgb/ written: the target
    over a 0.5 background with the occluder's pixels at 0.2.  --joint --silhouette --rgb --occluders writes a CSV tools/pose_errors.py
    reads, all rows status 0, and its mean ADD ends below that of --silhouette --rgb --occluders without --joint from the same
    estimates; --joint with one term exits with one message; --weights goes with --joint."""
    from texpose_amd import ops
    from texpose_amd.bop_scene import BopSceneWriter
    from texpose_amd.surfel import load_ply
    H, W, F, oid = TOOL_H, TOOL_W, TOOL_FRAMES, TOOL_OID
    verts, faces = REF.mesh_of("bent sphere")
    colours8 = np.rint(JREF.vertex_colours(verts) * 255.0).astype(np.uint8)
    K, gt, front, moved = tool_scene()
    root, ply, est_csv = str(tmp_path / "scene"), str(tmp_path / "obj_000007.ply"), str(tmp_path / "est.csv")
    _write_ply(ply, verts, faces, colours8)
    vcolor = load_ply(ply)[2]                                    # (the colours as the tool will read them)
    assert vcolor is not None
    target = ops.mesh_raster(cu(verts), cu(faces), cu(gt), cu(K), H=H, W=W, vcolor=cu(np.asarray(vcolor, np.float32)), face_ids=False, normals=False)
    whole = host(target["zbuf"]) > 0
    occ = host(ops.mesh_raster(cu(REF.mesh_of("sphere")[0]), cu(REF.mesh_of("sphere")[1]), cu(front), cu(K), H=H, W=W, face_ids=False, normals=False)["zbuf"]) > 0
    photo = np.where(whole[..., None], host(target["rgb"]), 0.5)
    photo[occ] = JREF.OCCLUDER_COLOUR
    rgb8 = np.rint(np.clip(photo, 0.0, 1.0) * 255.0).astype(np.uint8)
    visib = np.stack([whole & ~occ, occ], 1).astype(np.uint8) * np.uint8(255)          # [F,2,H,W]: the target behind, the occluder in front
    full = np.stack([whole, occ], 1).astype(np.uint8) * np.uint8(255)
    share = visib[:, 0].astype(bool).sum((1, 2)) / whole.sum((1, 2))
    assert (share > 0.5).all() and (share < 0.95).all(), share
    w = BopSceneWriter(root, K, 10.0, png_per_metre=2000)          # (it takes NeRF units at depth.scale 10: mm / 100)
    info = np.zeros((F, 2, 10), np.int32)
    info[:, :, 0], info[:, :, 1] = full.astype(bool).sum((2, 3)), visib.astype(bool).sum((2, 3))
    frames = []
    for f in range(F):
        pose = gt[f].copy()
        pose[:, 3] /= 100.0
        frames += w.add_views(pose[None], [oid, TOOL_OCCLUDER_OID], info[f][None], full[f][None], visib[f][None], rgb8[f][None],
                              np.zeros((1, H, W), np.uint16))
    w.close()
    refine, errors = _load_tool("refine_poses"), _load_tool("pose_errors")
    refine.write_rows(est_csv, [(1, frames[f], oid, 0.5, moved[f, :, :3], moved[f, :, 3], 0.0) for f in range(F)])
    common = ["--scene", root, "--ply", "%d=%s" % (oid, ply), "--est", est_csv, "--device", DEV, "--silhouette", "--rgb", "--occluders"]
    refine.main(common + ["--out", str(tmp_path / "joint.csv"), "--joint"])
    said_joint = capsys.readouterr().out
    refine.main(common + ["--out", str(tmp_path / "sequential.csv")])
    said_seq = capsys.readouterr().out
    assert "3 refined (0 with a failed last step)" in said_joint and "mean visible IoU" in said_joint and "mean visible IoU" in said_seq
    gt_arg = ["--gt", root, "--ply", "%d=%s" % (oid, ply)]
    before, joint, seq = (errors.main(gt_arg + ["--est", path])[oid] for path in (est_csv, str(tmp_path / "joint.csv"), str(tmp_path / "sequential.csv")))
    capsys.readouterr()
    assert joint["frames"] == sorted(frames) and not joint["missing"]
    add = lambda r: float(np.mean(r["errors"]["add"]))
    report = ["tool: visible share %s; mean ADD %.3f mm at the start, %.3f with --joint, %.3f with the sequential route" % (np.round(share, 2), add(before), add(joint), add(seq))]
    report += ["tool frame %d: ADD %.3f mm -> %.3f with --joint, %.3f sequential" % row
               for row in zip(joint["frames"], before["errors"]["add"], joint["errors"]["add"], seq["errors"]["add"])]
    with capsys.disabled():                                      # (measured figures for DESIGN section 23)
        print("\n" + "\n".join(report))
    assert add(joint) < add(seq) and add(joint) < add(before)
    # the weights reach the loop
    refine.main(common + ["--out", str(tmp_path / "weights.csv"), "--joint", "--weights", "1", "25", "0.04", "--iters-joint", "5"])
    capsys.readouterr()
    strip_time = lambda name: [ln.rsplit(",", 1)[0] for ln in open(str(tmp_path / name))]
    assert strip_time("weights.csv") != strip_time("joint.csv")
    base = ["--scene", root, "--ply", "%d=%s" % (oid, ply), "--est", est_csv, "--device", DEV, "--out", str(tmp_path / "x.csv")]
    for one in (["--silhouette"], ["--rgb"], ["--depth"], []):
        with pytest.raises(SystemExit, match="--joint combines at least two"):
            refine.main(base + ["--joint"] + one)
    with pytest.raises(SystemExit, match="--weights goes with --joint"):
        refine.main(base + ["--silhouette", "--rgb", "--weights", "1", "100", "0.04"])
    with pytest.raises(SystemExit, match="iters-joint \\+ 1"):
        refine.main(base + ["--joint", "--silhouette", "--rgb", "--tau-px", "6", "4"])
    assert not os.path.exists(str(tmp_path / "x.csv"))
