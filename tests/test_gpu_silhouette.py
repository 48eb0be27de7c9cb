"""K31 on the GPU: tp_mask_sdf against the brute force over all pixel pairs, tp_silhouette_align_step against the numpy restatement
(tests/silhouette_ref.py) on exactly the same planes, the loop ops.silhouette_align against the restatement's loop on its own raster,
reproducibility under repetition and graph replay, the module and tools/refine_poses.py --silhouette on a written BOP scene.
Figures measured on the restatement (CPU, numpy, its own raster; tests/test_silhouette_cpu.py prints them): from 3 deg and 6.1 .. 8.1
mm on the bent meshes the outline closes (rms 0.44 .. 1.52 px -> 0.000 .. 0.075 px, IoU 0.727 .. 0.961 -> 0.990 .. 1.000, 61 .. 88 rim
pixels, status 0) and the rotation error falls to 0.58 .. 1.99 deg."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import pnp_ref as PREF
import silhouette_ref as REF
from gn_ref import compare, cu, host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RE_FLOOR, TE_FLOOR = 1e-3, 1e-3          # deg, mm: section 20's floors, for the same geometry (about 16 fp32 ulp of a 900 mm depth)


# ----------------------------------------------------------------------------- the distance field
def mask_kinds(rs, H, W):
    """[7,H,W] uint8: 50 % random, 2 % random, empty, full, one pixel in a corner, set pixels only in the last row and the last column,
    and 50 % random with the values 7 and 255 as "set"."""
    m = np.zeros((7, H, W), np.uint8)
    m[0] = (rs.uniform(size=(H, W)) < 0.5) * 255
    m[1] = (rs.uniform(size=(H, W)) < 0.02) * 255
    m[3] = 1
    m[4, H - 1, 0] = 255
    m[5, H - 1, :] = rs.uniform(size=W) < 0.5
    m[5, :, W - 1] = rs.uniform(size=H) < 0.5
    m[5, H - 1, W - 1] = 1
    m[6] = rs.choice(np.array([0, 0, 7, 255], np.uint8), (H, W))
    return m


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (2, 5), (3, 3), (16, 16), (33, 257), (64, 80), (5, 1030)])
def test_distance_field_equals_the_brute_force(H, W):
    """F = 1 on every kind of mask, F = 3 on three stacks of them.  round((|sdf| + 0.5)^2) is the brute force's integer (the rounding
    of sqrtf and of the subtraction moves the square by at most 2.4e-7 x 2 d2 < 0.26 at these sizes), the sentinel H^2 + W^2 included;
    sdf within 1 ulp of the restatement's; the sign is the mask's."""
    from texpose_amd import ops
    masks = mask_kinds(np.random.RandomState(H * 2000 + W), H, W)
    d2 = np.stack([np.where(m != 0, REF.d2_ref(m)[1], REF.d2_ref(m)[0]) for m in masks])
    want = REF.sdf_ref(masks)
    assert (d2[2] == H * H + W * W).all() and (d2[3] == H * H + W * W).all() and d2.max() <= H * H + W * W
    ws = ops.mask_sdf_workspace(3, H, W, DEV)
    ws.view(torch.uint8).fill_(0xAB)                             # (needs no clearing)
    runs = [([k], ops.mask_sdf(cu(masks[k:k + 1]))) for k in range(7)]
    runs += [(pick, ops.mask_sdf(cu(masks[pick]), workspace=ws)) for pick in ([0, 2, 4], [1, 3, 5], [6, 3, 0])]
    runs += [([0], ops.mask_sdf(cu(masks[0] != 0))[None])]       # a bool plane [H,W]
    for pick, got in runs:
        got = host(got)
        assert got.dtype == np.float32 and got.shape == (len(pick), H, W) and np.isfinite(got).all()
        assert np.array_equal(np.rint((np.abs(got.astype(np.float64)) + 0.5) ** 2).astype(np.int64), d2[pick]), pick
        assert np.array_equal(got < 0, masks[pick] != 0)
        assert (np.abs(got - want[pick]) <= np.spacing(np.abs(want[pick]))).all(), pick
    out = torch.full((3, H, W), 7.0, device=DEV)
    assert ops.mask_sdf(cu(masks[[0, 2, 4]]), out=out, workspace=ws) is out and np.array_equal(host(out), host(runs[7][1]))


# ----------------------------------------------------------------------------- one step, exact inputs
def gpu_step(c, **kw):
    from texpose_amd import ops
    return ops.silhouette_align_step(cu(c["zbuf"]), cu(c["pose"]), cu(c["K"]), cu(c["sdf"]), tau_px=c["tau"], frame=cu(c["frame"]),
                                     mask=cu(c["mask"]), **kw)


def ref_step(c, **kw):
    return REF.step_ref(c["zbuf"], c["pose"], c["K"], c["sdf"], c["tau"], 1e-6, c["frame"], c["mask"], **kw)


def compare_all(got, want, pose_in):
    compare(got, want, pose_in)
    assert got["inter"].dtype == got["uni"].dtype == torch.int32
    assert np.array_equal(host(got["inter"]), want["inter"]) and np.array_equal(host(got["uni"]), want["uni"]), (got["inter"], want["inter"])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 5), (3, 3), (3, 7), (7, 65), (16, 16), (33, 257), (64, 80)])
def test_step_equals_the_restatement(H, W, B):
    """3 x 3 is the single interior pixel, 7 x 65 and 33 x 257 have a tile tail, 33 x 257 and 64 x 80 several tiles.  The field is the
    kernel's own on the coverage moved by a pixel each way (both sides read the same array), then a random one with NaN / Inf."""
    from texpose_amd import ops
    kept, statuses, union = 0, set(), 0
    for field in ("measured", "random"):
        for frames in ("one", "each", "map"):
            for with_mask in (False, True):
                c = REF.one_step_case(1000 * H + 10 * W + B, B, H, W, frames, with_mask, field)
                if field == "measured":
                    c["sdf"] = host(ops.mask_sdf(cu(c["measured"])))
                want = ref_step(c)
                compare_all(gpu_step(c), want, c["pose"])
                kept += int(want["inliers"].sum())
                union += int(want["uni"].sum())
                statuses |= set(want["status"].tolist())
                ev = gpu_step(c, evaluate_only=True)
                want_ev = ref_step(c, evaluate_only=True)
                compare_all(ev, want_ev, c["pose"])
                assert np.array_equal(host(ev["pose"]).view(np.uint32), c["pose"].view(np.uint32))
    assert union > 0
    if H < 3 or W < 3:
        assert kept == 0 and statuses == {1}
    if H * W >= 33 * 257:
        assert kept > 50 and 0 in statuses


def test_failed_steps_return_the_pose_bit_for_bit():
    c = REF.one_step_case(6, 3, 33, 65, "each", False, "shifted")
    c["zbuf"][0] = -1.0
    c["zbuf"][0, 5:7, 5:7] = 900.0                               # image 0: four rim pixels
    c["sdf"][1] = 0.25                                           # image 1: no gradient: the system is zero
    c["tau"] = 50.0                                              # (every rim pixel with a finite field is kept)
    want = ref_step(c)
    assert want["status"].tolist() == [1, 3, 0] and want["inliers"][0] == 4 and want["inliers"][1] >= 6
    got = gpu_step(c)
    compare_all(got, want, c["pose"])
    assert np.array_equal(host(got["pose"])[:2].view(np.uint32), c["pose"][:2].view(np.uint32))


def test_the_renderings_own_coverage_as_the_mask_has_no_residual():
    """zbuf from the GPU's K19 call, the mask its own coverage: every interior rim pixel is kept and reads 0."""
    from texpose_amd import ops
    c = REF.loop_inputs("bent torus")
    r = ops.mesh_raster(cu(c["verts"]), cu(c["faces"]), cu(c["start"]), cu(c["K"]), H=c["H"], W=c["W"], face_ids=False, normals=False)
    sdf = ops.mask_sdf(r["zbuf"] > 0)
    got = ops.silhouette_align_step(r["zbuf"], cu(c["start"]), cu(c["K"]), sdf, tau_px=4.0, evaluate_only=True)
    z = host(r["zbuf"])
    rims = np.array([REF.rim_ref(p).sum() for p in z])
    assert np.array_equal(host(got["inliers"]), rims) and (rims > 50).all() and (host(got["rms"]) == 0).all()
    assert torch.equal(got["inter"], got["uni"]) and np.array_equal(host(got["inter"]), (z > 0).reshape(2, -1).sum(1))
    case = dict(zbuf=z, pose=c["start"], K=c["K"], sdf=host(sdf), frame=None, mask=None, tau=4.0)
    compare_all(got, ref_step(case, evaluate_only=True), c["start"])


# ----------------------------------------------------------------------------- the loop
def run_loop(c, **kw):
    from texpose_amd import ops
    return ops.silhouette_align(cu(c["verts"]), cu(c["faces"]), cu(c["start"]), cu(c["K"]), cu(c["sdf"]), tau_px=4.0, iters=10, damping=1e-6, **kw)


@pytest.mark.parametrize("name", REF.MESHES)
def test_loop_closes_the_outline(name):
    """The prototype's cases, the restatement's inputs: the image-space conditions of the CPU test, and the pose error against the
    truth at most twice the restatement's on the same inputs plus section 20's floors for the same geometry (K19 and the numpy
    raster may differ on edge pixels, which is where rims live; measured: see DESIGN section 21)."""
    c = REF.loop_case(name)
    got, want = run_loop(c), c["want"]
    assert (want["status"] == 0).all()
    for b in range(2):
        re0, te0 = PREF.pose_error(c["start"][b], c["P"][b])
        re, te = PREF.pose_error(host(got["pose"])[b], c["P"][b])
        re_w, te_w = PREF.pose_error(want["pose"][b], c["P"][b])
        n0, rms0, rms, iou0, iou = int(got["inliers0"][b]), float(got["rms0"][b]), float(got["rms"][b]), float(got["iou0"][b]), float(got["iou"][b])
        print("%s %d: kernel %.4f deg %.4f mm (%d rim pixels, rms %.4f -> %.4f, IoU %.4f -> %.4f, status %d) | restatement %.4f deg %.4f mm "
              "(%d rim pixels, rms %.4f -> %.4f, IoU %.4f -> %.4f)" % (name, b, re, te, n0, rms0, rms, iou0, iou, int(got["status"][b]), re_w, te_w,
                                                                     want["inliers0"][b], want["rms0"][b], want["rms"][b], want["iou0"][b], want["iou"][b]))
    for b in range(2):
        re0, te0 = PREF.pose_error(c["start"][b], c["P"][b])
        re, te = PREF.pose_error(host(got["pose"])[b], c["P"][b])
        re_w, te_w = PREF.pose_error(want["pose"][b], c["P"][b])
        assert int(got["status"][b]) == 0
        assert float(got["rms"][b]) <= 0.25 * float(got["rms0"][b])
        assert float(got["iou"][b]) >= float(got["iou0"][b]) and float(got["iou"][b]) >= 0.97
        assert re < re0
        assert re <= 2 * re_w + RE_FLOOR and te <= 2 * te_w + TE_FLOOR


# ----------------------------------------------------------------------------- determinism and the wrappers
def test_two_runs_and_graph_replay_are_bit_equal():
    from texpose_amd import ops
    c = REF.loop_inputs("bent sphere")
    first, again = run_loop(c), run_loop(c)
    for k in ops.SILHOUETTE_ALIGN_KEYS:
        assert torch.equal(first[k].view(torch.uint8), again[k].view(torch.uint8)), k
    verts, faces, pose, K, sdf = cu(c["verts"]), cu(c["faces"], torch.int32), cu(c["start"]), cu(c["K"]), cu(c["sdf"])
    ws = ops.silhouette_align_workspace(2, c["H"], c["W"], DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = ops.silhouette_align(verts, faces, pose, K, sdf, tau_px=4.0, iters=10, damping=1e-6, workspace=ws)
    for _ in range(2):
        for v in cap.values():
            v.view(torch.uint8).fill_(0xAB)
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k in ops.SILHOUETTE_ALIGN_KEYS:
            assert torch.equal(cap[k].view(torch.uint8), first[k].view(torch.uint8)), k
    assert (first["status"] == 0).all()
    # one step, its six outputs and the field
    r = ops.mesh_raster(verts, faces, pose, K, H=c["H"], W=c["W"], face_ids=False, normals=False)
    one, two = (ops.silhouette_align_step(r["zbuf"], pose, K, sdf, tau_px=4.0) for _ in range(2))
    for k in one:
        assert torch.equal(one[k].view(torch.uint8), two[k].view(torch.uint8)), k
    m = cu(c["mask"])
    assert torch.equal(ops.mask_sdf(m), ops.mask_sdf(m)) and torch.equal(ops.mask_sdf(m), sdf)


def test_refiner_module_matches_the_ops():
    from texpose_amd import silhouette
    c = REF.loop_inputs("bent sphere")
    want = run_loop(c)
    refiner = silhouette.SilhouetteRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV, tau_px=4.0, iters=10, damping=1e-6)
    for planes in (cu(c["mask"]), cu(c["mask"] != 0), cu(c["sdf"]), cu(c["mask"])):          # (the last call reuses the workspaces)
        r = refiner.refine(cu(c["start"]), cu(c["K"][0]), planes)
        assert torch.equal(r.pose, want["pose"]) and torch.equal(r.inliers, want["inliers"]) and torch.equal(r.status, want["status"])
        assert torch.equal(r.iou, want["iou"]) and torch.equal(r.iou0, want["iou0"])
    sched = silhouette.SilhouetteRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV, tau_px=[6.0, 5.0, 4.0], iters=2)
    r = sched.refine(cu(c["start"]), cu(c["K"]), cu(c["mask"]), frame=cu([0, 1], torch.int32))
    assert (r.status == 0).all() and (r.rms < r.rms0).all() and (r.iou > r.iou0).all()
    with pytest.raises(ValueError):
        refiner.refine(cu(c["start"]), cu(c["K"]), cu(c["mask"][:, :-1]))


def test_step_torch_on_the_device_matches_the_kernel():
    from texpose_amd import silhouette
    c = REF.one_step_case(9, 3, 33, 257, "map", True, "random")
    got = gpu_step(c)
    t = silhouette.step_torch(cu(c["zbuf"]), cu(c["pose"]), cu(c["K"]), cu(c["sdf"]), c["tau"], 1e-6, cu(c["frame"]), cu(c["mask"]))
    for k in ("inliers", "status", "inter", "uni"):
        assert torch.equal(got[k], t[k]), k
    assert torch.allclose(got["pose"], t["pose"], rtol=1e-5, atol=1e-5) and (got["status"] == 0).any()
    m = cu(c["measured"])
    assert torch.equal(silhouette.sdf_torch(m), __import__("texpose_amd").ops.mask_sdf(m))


def test_bad_arguments_are_refused():
    from texpose_amd import _lib, ops
    c = REF.one_step_case(1, 2, 7, 65, "each", False, "random")
    a = [cu(c[k]) for k in ("zbuf", "pose", "K", "sdf")]
    for kw in (dict(tau_px=0.0), dict(tau_px=float("nan")), dict(tau_px=4.0, damping=-1.0), dict(tau_px=4.0, out=dict(pose=a[1]))):
        with pytest.raises(_lib.TexposeLibraryError):
            ops.silhouette_align_step(*a, **kw)
    with pytest.raises(ValueError):
        ops.silhouette_align_step(*a[:3], torch.cat([a[3], a[3][:1]]), tau_px=4.0)          # Ft = 3 without a frame map
    with pytest.raises(ValueError):
        ops.silhouette_align_step(*a, tau_px=4.0, workspace=torch.empty(4, device=DEV))
    with pytest.raises(ValueError):
        ops.silhouette_align_step(*a, tau_px=4.0, mask=torch.ones(2, 7, 65, device=DEV))          # float mask
    with pytest.raises(ValueError):
        ops.silhouette_align_step(*a, tau_px=4.0, out=dict(inter=torch.zeros(2, device=DEV)))          # float counts
    with pytest.raises(ValueError):
        ops.mask_sdf(torch.ones(2, 7, 65, device=DEV))          # float mask
    with pytest.raises(ValueError):
        ops.mask_sdf(torch.ones(2, 7, 65, device=DEV, dtype=torch.uint8), out=torch.empty(2, 7, 64, device=DEV))
    with pytest.raises(ValueError):
        ops.mask_sdf(torch.ones(2, 7, 65, device=DEV, dtype=torch.uint8), workspace=torch.empty(4, device=DEV))


# ----------------------------------------------------------------------------- the tool
TOOL_H, TOOL_W, TOOL_FRAMES = 120, 160, 3


def _write_ply(path, verts, faces):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces)))
        for p in verts:
            f.write("%r %r %r\n" % tuple(float(v) for v in p))
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(int(v) for v in t))


def test_tool_refines_on_masks_a_results_csv_that_pose_errors_reads(tmp_path, capsys):
    """The bent sphere without colours and without depth, three poses about 900 mm away at 120 x 160, estimates 2 deg and 5 mm off: the
    scene holds only masks, the tool writes a CSV tools/pose_errors.py reads, and the mean IoU it prints rose."""
    from texpose_amd import ops
    from texpose_amd.bop_scene import BopSceneWriter
    H, W, F, oid = TOOL_H, TOOL_W, TOOL_FRAMES, 7
    verts, faces = REF.mesh_of("bent sphere")
    K = PREF.end_to_end_inputs("sphere")["K"].copy()
    K[:2] *= TOOL_H / 64.0
    rs = np.random.RandomState(8)
    gt = []
    for _ in range(F):
        q, _r = np.linalg.qr(rs.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        gt.append(np.concatenate([q, rs.uniform(-15, 15, (3, 1)) + [[0.0], [0.0], [900.0]]], 1))
    gt = np.stack(gt).astype(np.float32)
    moved = REF.perturbed(gt, np.random.RandomState(5), angle_deg=2.0).astype(np.float64)
    for f in range(F):                                           # (2 deg, 5 mm)
        d = moved[f, :, 3] - gt[f, :, 3]
        moved[f, :, 3] = gt[f, :, 3] + d * 5.0 / np.linalg.norm(d)
    z = host(ops.mesh_raster(cu(verts), cu(faces), cu(gt), cu(K), H=H, W=W, face_ids=False, normals=False)["zbuf"])
    visib = ((z > 0) * 255).astype(np.uint8)
    root, ply, est_csv, out_csv = str(tmp_path / "scene"), str(tmp_path / "obj_000007.ply"), str(tmp_path / "est.csv"), str(tmp_path / "refined.csv")
    _write_ply(ply, verts, faces)
    w = BopSceneWriter(root, K, 10.0, png_per_metre=2000)          # (it takes NeRF units at depth.scale 10: mm / 100)
    info = np.zeros((F, 10), np.int32)
    info[:, 0] = info[:, 1] = (z > 0).sum((1, 2))
    frames = []
    for f in range(F):
        pose = gt[f].copy()
        pose[:, 3] /= 100.0
        frames += w.add_views(pose[None], [oid], info[f][None, None], visib[f][None, None], visib[f][None, None], np.zeros((1, H, W, 3), np.uint8),
                              np.zeros((1, H, W), np.uint16))
    w.close()
    spec = importlib.util.spec_from_file_location("refine_poses_tool", os.path.join(REPO, "tools", "refine_poses.py"))
    refine = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(refine)
    refine.write_rows(est_csv, [(1, frames[f], oid, 0.5, moved[f, :, :3], moved[f, :, 3], 0.0) for f in range(F)])
    refine.main(["--scene", root, "--ply", ply, "--est", est_csv, "--out", out_csv, "--device", DEV, "--silhouette"])
    said = capsys.readouterr().out
    assert "3 refined (0 with a failed last step)" in said
    line = [ln for ln in said.splitlines() if "mean IoU" in ln]
    assert len(line) == 1
    iou0, iou = (float(v) for v in line[0].split("mean IoU")[1].split("->"))
    assert iou > iou0 and iou >= 0.97
    spec = importlib.util.spec_from_file_location("pose_errors_tool", os.path.join(REPO, "tools", "pose_errors.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    before = tool.main(["--gt", root, "--est", est_csv, "--ply", "%d=%s" % (oid, ply)])[oid]
    after = tool.main(["--gt", root, "--est", out_csv, "--ply", "%d=%s" % (oid, ply)])[oid]
    capsys.readouterr()
    assert before["frames"] == after["frames"] == sorted(frames) and not after["missing"]
    report = ["tool --silhouette frame %d: ADD %.4f -> %.4f mm; mean IoU %.4f -> %.4f" % (f, a0, a1, iou0, iou)
              for f, a0, a1 in zip(after["frames"], before["errors"]["add"], after["errors"]["add"])]
    masks = str(tmp_path / "masks")                              # --masks DIR: the same files elsewhere, the same rows
    os.makedirs(masks)
    for name in os.listdir(os.path.join(root, "mask_visib")):
        os.replace(os.path.join(root, "mask_visib", name), os.path.join(masks, name))
    other = str(tmp_path / "refined2.csv")
    refine.main(["--scene", root, "--ply", ply, "--est", est_csv, "--out", other, "--device", DEV, "--silhouette", "--masks", masks])
    capsys.readouterr()
    strip_time = lambda path: [ln.rsplit(",", 1)[0] for ln in open(path)]
    assert strip_time(other) == strip_time(out_csv)
    with pytest.raises(SystemExit, match="--silhouette: no mask_visib image"):
        refine.main(["--scene", root, "--ply", ply, "--est", est_csv, "--out", other, "--device", DEV, "--silhouette"])
    print("\n".join(report))
