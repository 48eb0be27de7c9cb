"""K29 on the GPU: tp_depth_icp_step against the numpy restatement (tests/icp_ref.py) on exactly the same planes, the loop ops.depth_icp
against the restatement's loop on its own raster, reproducibility under repetition and graph replay, and tools/refine_poses.py on a
written BOP scene.  Figures measured on the restatement (CPU, numpy, its own raster; tests/test_icp_cpu.py prints them): the clean
sphere ends at <= 1.9e-5 deg and <= 8.9e-6 mm, the noisy one at 0.05 .. 0.50 deg and 0.05 .. 0.10 mm with rms 0.69 .. 0.74 mm, 580 ..
851 kept pixels, status 0."""
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import icp_ref as REF
import pnp_ref as PREF
from gn_ref import compare, cu, host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RE_FLOOR, TE_FLOOR = 1e-3, 1e-3          # deg, mm: about 16 fp32 ulp of a 900 mm depth and the angle it subtends on the 50 mm object


def gpu_step(c, **kw):
    from texpose_amd import ops
    return ops.depth_icp_step(cu(c["verts"]), cu(c["faces"]), cu(c["zbuf"]), cu(c["face"]), cu(c["pose"]), cu(c["K"]), cu(c["depth"]),
                              tau_mm=c["tau"], frame=cu(c["frame"]), mask=cu(c["mask"]), **kw)


def ref_step(c, **kw):
    return REF.step_ref(c["verts"], c["faces"], c["zbuf"], c["face"], c["pose"], c["K"], c["depth"], c["tau"], 1e-6, c["frame"], c["mask"], **kw)


# ----------------------------------------------------------------------------- one step, exact inputs
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 63), (7, 65), (16, 16), (33, 257), (64, 80)])
def test_step_equals_the_restatement(H, W, B):
    kept = 0
    for frames in ("one", "each", "map"):
        for with_mask in (False, True):
            c = REF.one_step_case(1000 * H + 10 * W + B, B, H, W, frames, with_mask)
            want = ref_step(c)
            compare(gpu_step(c), want, c["pose"])
            kept += int(want["inliers"].sum())
            ev = gpu_step(c, evaluate_only=True)
            want_ev = ref_step(c, evaluate_only=True)
            assert np.array_equal(host(ev["inliers"]), want_ev["inliers"]) and np.array_equal(host(ev["status"]), want_ev["status"])
            assert np.array_equal(host(ev["pose"]).view(np.uint32), c["pose"].view(np.uint32))
    assert kept > 0 or H * W == 1


def test_step_on_the_rasterisers_own_planes():
    """zbuf / face from the GPU's K19 call at a perturbed pose, the depth K19's render of the truth: both sides get the same arrays."""
    from texpose_amd import ops
    e = PREF.end_to_end_inputs("sphere")
    K = np.tile(e["K"], (2, 1, 1))
    start = REF.perturbed(e["P"], np.random.RandomState(3))
    render = lambda P: ops.mesh_raster(cu(e["verts"]), cu(e["faces"]), cu(P), cu(K), H=e["H"], W=e["W"], face_ids=True, normals=False)
    r, truth = render(start), render(e["P"])
    c = dict(verts=e["verts"], faces=e["faces"], zbuf=host(r["zbuf"]), face=host(r["face"]), pose=start, K=K,
             depth=np.maximum(host(truth["zbuf"]), 0.0), frame=None, mask=None, tau=20.0)
    want = ref_step(c)
    assert (want["status"] == 0).all() and (want["inliers"] > 500).all()
    compare(gpu_step(c), want, start)


def test_failed_steps_return_the_pose_bit_for_bit():
    c = REF.one_step_case(6, 3, 1, 63, "each", False)
    c["zbuf"][0, 0, 5:] = -1.0                                   # image 0: at most five pixels
    c["face"][1] = 0                                             # image 1: one face, one normal: rank 3
    want = ref_step(c)
    assert want["status"].tolist() == [1, 3, 0]
    compare(gpu_step(c), want, c["pose"])


@pytest.mark.parametrize("H,W", [(16, 16), (7, 65)])
def test_exact_decisions_on_the_bound(H, W):
    """fx = fy = 2^40: |ray| = 1 in fp64; integer-millimetre planes with |d - z| in {19, 20, 21} at tau = 20: 19 and 20 are kept."""
    rs = np.random.RandomState(H)
    c = REF.one_step_case(3, 2, H, W, "each", False)
    c["K"] = np.tile(np.array([[2.0 ** 40, 0, W / 2], [0, 2.0 ** 40, H / 2], [0, 0, 1]], np.float32), (2, 1, 1))
    c["zbuf"] = rs.randint(800, 1000, (2, H, W)).astype(np.float32)
    c["face"] = rs.randint(0, 96, (2, H, W)).astype(np.int32)
    off = rs.choice([-21, -20, -19, 19, 20, 21], (2, H, W))
    c["depth"] = c["zbuf"] + off.astype(np.float32)
    want = ref_step(c, evaluate_only=True)
    assert np.array_equal(want["inliers"], (np.abs(off) <= 20).reshape(2, -1).sum(1)) and (want["inliers"] > 50).all()
    got = gpu_step(c, evaluate_only=True)
    assert np.array_equal(host(got["inliers"]), want["inliers"])


# ----------------------------------------------------------------------------- the loop
@functools.lru_cache(maxsize=None)
def loop_case(mesh, noisy):
    """The restatement's loop, run once per case and shared."""
    e = PREF.end_to_end_inputs(mesh)
    K = np.tile(e["K"], (2, 1, 1))
    truth = np.stack([REF.render_ref(e["verts"], e["faces"], e["P"][b], K[b], e["H"], e["W"])[0] for b in range(2)])
    depth = REF.corrupted(truth, np.random.RandomState(4), e["W"]) if noisy else np.maximum(truth, 0.0)
    start = REF.perturbed(e["P"], np.random.RandomState(3))
    want = REF.icp_ref(e["verts"], e["faces"], start, K, depth, 20.0, 5, 1e-6)
    return dict(e, K=K, depth=depth, start=start, want=want)


def run_loop(c):
    from texpose_amd import ops
    return ops.depth_icp(cu(c["verts"]), cu(c["faces"]), cu(c["start"]), cu(c["K"]), cu(c["depth"]), tau_mm=20.0, iters=5, damping=1e-6)


@pytest.mark.parametrize("noisy", [False, True])
def test_loop_recovers_the_rippled_sphere(noisy):
    c = loop_case("sphere", noisy)
    got, want = run_loop(c), c["want"]
    assert (want["status"] == 0).all() and host(got["status"]).tolist() == [0, 0]
    for b in range(2):
        re, te = PREF.pose_error(host(got["pose"])[b], c["P"][b])
        re_w, te_w = PREF.pose_error(want["pose"][b], c["P"][b])
        n, rms = int(got["inliers"][b]), float(got["rms"][b])
        print("%s sphere %d: kernel %.3g deg %.3g mm (%d pixels, rms %.4f mm) | restatement %.3g deg %.3g mm (%d pixels, rms %.4f mm)"
              % ("noisy" if noisy else "clean", b, re, te, n, rms, re_w, te_w, want["inliers"][b], want["rms"][b]))
        assert re <= 2 * re_w + RE_FLOOR and te <= 2 * te_w + TE_FLOOR
        assert n >= 500 and int(got["inliers0"][b]) > 0 and float(got["rms0"][b]) > rms
        if noisy:
            assert abs(rms - want["rms"][b]) <= 0.1 * want["rms"][b]          # the noise it was given, seen through n . ray


def test_loop_on_the_torus_settles_its_translation():
    """Rotationally symmetric: the rotation about the axis is not observable; rms falls and the translation is found."""
    c = loop_case("torus", False)
    got, want = run_loop(c), c["want"]
    for b in range(2):
        re, te = PREF.pose_error(host(got["pose"])[b], c["P"][b])
        re_w, te_w = PREF.pose_error(want["pose"][b], c["P"][b])
        print("torus %d: kernel %.3g deg %.3g mm rms %.4f <- %.4f | restatement %.3g deg %.3g mm rms %.4f" %
              (b, re, te, float(got["rms"][b]), float(got["rms0"][b]), re_w, te_w, want["rms"][b]))
        assert float(got["rms"][b]) < float(got["rms0"][b])
        assert te <= 2 * te_w + TE_FLOOR


# ----------------------------------------------------------------------------- determinism
def test_two_runs_and_graph_replay_are_bit_equal():
    from texpose_amd import ops
    c = loop_case("sphere", True)
    first, again = run_loop(c), run_loop(c)
    for k in ops.DEPTH_ICP_KEYS:
        assert torch.equal(first[k].view(torch.uint8), again[k].view(torch.uint8)), k
    e = c
    args = (cu(e["verts"]), cu(e["faces"]))
    r = ops.mesh_raster(*args, cu(e["start"]), cu(e["K"]), H=e["H"], W=e["W"], face_ids=True, normals=False)
    step = lambda **kw: ops.depth_icp_step(*args, r["zbuf"], r["face"], cu(e["start"]), cu(e["K"]), cu(e["depth"]), tau_mm=20.0, **kw)
    eager = step()
    pose, K, depth = cu(e["start"]), cu(e["K"]), cu(e["depth"])
    ws = ops.depth_icp_workspace(2, e["H"], e["W"], DEV)
    cap = {k: torch.empty_like(v) for k, v in eager.items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.depth_icp_step(*args, r["zbuf"], r["face"], pose, K, depth, tau_mm=20.0, workspace=ws, out=cap)
    for _ in range(2):
        for v in cap.values():
            v.view(torch.uint8).fill_(0xAB)
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert torch.equal(cap[k].view(torch.uint8), eager[k].view(torch.uint8)), k
    assert (eager["status"] == 0).all()


def test_refiner_module_matches_the_ops():
    from texpose_amd import icp
    c = loop_case("sphere", True)
    want = run_loop(c)
    refiner = icp.DepthRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV, tau_mm=20.0, iters=5, damping=1e-6)
    for _ in range(2):                                           # (the second call reuses the workspace)
        r = refiner.refine(cu(c["start"]), cu(c["K"][0]), cu(c["depth"]))
        assert torch.equal(r.pose, want["pose"]) and torch.equal(r.inliers, want["inliers"]) and torch.equal(r.status, want["status"])
    sched = icp.DepthRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV, tau_mm=[40.0, 30.0, 20.0], iters=2)
    r = sched.refine(cu(c["start"]), cu(c["K"]), cu(c["depth"]), frame=cu([0, 1], torch.int32))
    assert (r.status == 0).all() and (r.rms < r.rms0).all()


def test_bad_arguments_are_refused():
    from texpose_amd import _lib, ops
    c = REF.one_step_case(1, 2, 7, 65, "each", False)
    a = [cu(c[k]) for k in ("verts", "faces", "zbuf", "face", "pose", "K", "depth")]
    for kw in (dict(tau_mm=0.0), dict(tau_mm=float("nan")), dict(tau_mm=20.0, damping=-1.0), dict(tau_mm=20.0, out=dict(pose=a[4]))):
        with pytest.raises(_lib.TexposeLibraryError):
            ops.depth_icp_step(*a, **kw)
    with pytest.raises(ValueError):
        ops.depth_icp_step(*a[:6], torch.cat([a[6], a[6][:1]]), tau_mm=20.0)          # Ft = 3 without a frame map
    with pytest.raises(ValueError):
        ops.depth_icp_step(*a, tau_mm=20.0, workspace=torch.empty(4, device=DEV))
    with pytest.raises(ValueError):
        ops.depth_icp_step(*a, tau_mm=20.0, mask=torch.ones(2, 7, 65, device=DEV))          # float mask


# ----------------------------------------------------------------------------- the tool
def _write_ply(path, verts, faces):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces)))
        for p in verts:
            f.write("%r %r %r\n" % tuple(float(v) for v in p))
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(int(v) for v in t))


def test_tool_refines_a_results_csv_that_pose_errors_reads(tmp_path, capsys):
    from texpose_amd import ops
    from texpose_amd.bop_scene import BopSceneWriter
    H, W, F, oid = 120, 160, 3, 7
    verts, faces = PREF._uv_sphere(24, 32, 50.0, ripple=0.1)
    K = PREF.end_to_end_inputs("sphere")["K"].copy()
    K[:2] *= H / 64.0
    rs = np.random.RandomState(8)
    gt = []
    for _ in range(F):
        q, _r = np.linalg.qr(rs.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        gt.append(np.concatenate([q, rs.uniform(-15, 15, (3, 1)) + [[0.0], [0.0], [900.0]]], 1))
    gt = np.stack(gt).astype(np.float32)
    z = host(ops.mesh_raster(cu(verts), cu(faces), cu(gt), cu(K), H=H, W=W, face_ids=False, normals=False)["zbuf"])
    depth16 = np.where(z > 0, np.rint(z / 0.5), 0).astype(np.uint16)              # depth_scale 1000 / 2000 = 0.5 mm; 0 on background
    root, ply, est_csv, out_csv = str(tmp_path / "scene"), str(tmp_path / "obj_000007.ply"), str(tmp_path / "est.csv"), str(tmp_path / "refined.csv")
    _write_ply(ply, verts, faces)
    w = BopSceneWriter(root, K, 10.0, png_per_metre=2000)                          # (it takes NeRF units at depth.scale 10: mm / 100)
    info = np.zeros((F, 10), np.int32)
    info[:, 0] = info[:, 1] = (z > 0).sum((1, 2))
    frames = []
    for f in range(F):
        pose = gt[f].copy()
        pose[:, 3] /= 100.0
        frames += w.add_views(pose[None], [oid], info[f][None, None], np.zeros((1, 1, H, W), np.uint8), np.zeros((1, 1, H, W), np.uint8),
                              np.zeros((1, H, W, 3), np.uint8), depth16[f][None])
    w.close()
    spec = importlib.util.spec_from_file_location("refine_poses_tool", os.path.join(REPO, "tools", "refine_poses.py"))
    refine = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(refine)
    moved = REF.perturbed(gt, np.random.RandomState(5), angle_deg=2.0).astype(np.float64)
    for f in range(F):                                           # (2 deg, 5 mm)
        d = moved[f, :, 3] - gt[f, :, 3]
        moved[f, :, 3] = gt[f, :, 3] + d * 5.0 / np.linalg.norm(d)
    refine.write_rows(est_csv, [(1, frames[f], oid, 0.5, moved[f, :, :3], moved[f, :, 3], 0.0) for f in range(F)])
    run = subprocess.run([sys.executable, os.path.join(REPO, "tools", "refine_poses.py"), "--scene", root, "--ply", ply, "--est", est_csv,
                          "--out", out_csv, "--device", DEV], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "3 refined (0 with a failed last step)" in run.stdout
    spec = importlib.util.spec_from_file_location("pose_errors_tool", os.path.join(REPO, "tools", "pose_errors.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    before = tool.main(["--gt", root, "--est", est_csv, "--ply", "%d=%s" % (oid, ply)])[oid]
    after = tool.main(["--gt", root, "--est", out_csv, "--ply", "%d=%s" % (oid, ply)])[oid]
    capsys.readouterr()
    assert before["frames"] == after["frames"] == sorted(frames) and not after["missing"]
    for f, a0, a1, t0, t1 in zip(after["frames"], before["errors"]["add"], after["errors"]["add"], before["errors"]["te"], after["errors"]["te"]):
        print("tool frame %d: ADD %.4f -> %.4f mm, translation %.4f -> %.4f mm" % (f, a0, a1, t0, t1))
        assert a1 < 0.25 * a0
    cpu = subprocess.run([sys.executable, os.path.join(REPO, "tools", "refine_poses.py"), "--scene", root, "--ply", ply, "--est", est_csv,
                          "--out", out_csv, "--device", "cpu"], capture_output=True, text=True, timeout=300)
    assert cpu.returncode != 0 and cpu.stderr.count("\n") == 1 and "no CPU route" in cpu.stderr
