"""GPU: kernel K26 `tp_vsd` and the VSD functions of texpose_amd/pose_error.py against the numpy fp64 restatement tests/vsd_ref.py.

Exact cases: planes of integer millimetres under intrinsics with fx = fy = 2^40, where the distance factor f is exactly 1 in fp64, and
integer `delta` / `tau` chosen so that many pixels sit exactly ON `D - D_test == delta` and `|D_gt - D_est| == tau`: counts and errors
must EQUAL the helper's -- this is where `<=` and `>=` are decided.

Realistic cases: rendered meshes, a noisy, partly occluded, holed test depth and real intrinsics.  The outputs are integers, so the
only admissible disagreement is a decision whose fp64 margin is below the helper's near-tie bound (1e-9 mm; f may be rounded
differently by two correct evaluations): every count may differ by at most the helper's near-tie number of the case, which is printed
and may itself be at most 0.1 % of n_U (a condition on the case, not a measurement), and err by near_ties / n_U plus one fp32 ulp of 1."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import vsd_ref as V
from test_gpu_surfel import K_for, torus, uv_sphere

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP1 = float(np.spacing(np.float32(1.0)))
TIE_CAP = 1e-3
BOP_TAUS = [round(0.05 * i, 2) for i in range(1, 11)]
LINEMOD_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)


def cu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def host(t):
    return t.detach().cpu().numpy()


def run(ze, zg, dt, K, tau, delta=15.0, frame=None, out=None):
    from texpose_amd import ops
    r = ops.vsd(cu(ze), cu(zg), cu(dt), cu(K), cu(tau), delta_mm=delta, frame=None if frame is None else cu(frame, torch.int32), out=out)
    assert r["counts"].dtype == torch.int32 and r["err"].dtype == torch.float32
    return host(r["counts"]), host(r["err"])


# ----------------------------------------------------------------------------- exact logic, no rasteriser
K_FLAT = np.array([[2.0 ** 40, 0.0, 3.0], [0.0, 2.0 ** 40, 2.0], [0.0, 0.0, 1.0]], np.float32)
DELTA = 15.0


@functools.lru_cache(maxsize=None)
def exact_case(H, W, B, T, mode):
    """Integer planes in 200 .. 1200 mm with background -1, NaN and test holes 0; D_gt - D_test in 13 .. 17 around delta = 15 and
    |D_gt - D_est| in {0, 5, .. 20} against taus that are multiples of 5.  mode: 'one' (Ft = 1), 'each' (Ft = B), 'map' (Ft = 2 with a
    frame map that repeats).  Built once, read-only."""
    rs = np.random.RandomState(H * 100003 + W * 1009 + B * 101 + T * 7 + len(mode))
    Ft = {"one": 1, "each": B, "map": 2}[mode]
    frame = rs.randint(0, 2, B).astype(np.int32) if mode == "map" else None
    if frame is not None and B > 1:
        frame[:2] = 1                                        # (a repeat, and not the identity)
    of = (lambda b: int(frame[b])) if frame is not None else (lambda b: 0 if Ft == 1 else b)
    dt = rs.randint(300, 1101, (Ft, H, W)).astype(np.float32)
    zg = np.stack([dt[of(b)] + DELTA + rs.randint(-2, 3, (H, W)) for b in range(B)]).astype(np.float32)
    ze = (zg + 5.0 * rs.randint(-4, 5, zg.shape)).astype(np.float32)
    hidden = rs.uniform(size=ze.shape) < 0.15                # estimates far behind the measured surface: in V_est only through V_gt
    ze[hidden] += 100.0
    for a, value, share in ((zg, -1.0, 0.25), (ze, -1.0, 0.25), (dt, 0.0, 0.1), (ze, np.nan, 0.03), (zg, np.nan, 0.02), (dt, np.nan, 0.02), (ze, 0.0, 0.02)):
        a[rs.uniform(size=a.shape) < share] = value
    tau = (5.0 * (1 + (np.arange(T)[None] + np.arange(B)[:, None]) % 5)).astype(np.float32)
    K = np.tile(K_FLAT, (B, 1, 1))
    want = V.vsd_ref(ze, zg, dt, K, tau, DELTA, frame)
    for a in (ze, zg, dt, tau, K, want["counts"], want["err"]):
        a.setflags(write=False)
    return ze, zg, dt, K, tau, frame, want


@pytest.mark.parametrize("H,W", [(1, 1), (1, 63), (7, 65), (16, 16), (33, 257), (120, 160)])
def test_exact_counts_at_the_decision_boundaries(H, W):
    on_delta = on_tau = 0
    for B in (1, 3, 5):
        for T in (1, 10, 16):
            for mode in ("one", "each", "map"):
                ze, zg, dt, K, tau, frame, want = exact_case(H, W, B, T, mode)
                counts, err = run(ze, zg, dt, K, tau, DELTA, frame)
                assert np.array_equal(counts, want["counts"]), (B, T, mode, counts, want["counts"])
                assert np.array_equal(err, want["err"]), (B, T, mode)
                on_delta += int(want["near_ties"].sum())
                on_tau += int(want["counts"][:, 2:].sum())
    if H * W >= 256:                                         # the cases do sit on the boundaries, and are not empty
        assert on_delta > 100 and on_tau > 100


def test_exact_case_through_the_unaligned_route():
    """A view one float into the planes: W is a multiple of four but the rows are not 16-byte aligned, so the scalar loads run."""
    from texpose_amd import ops
    ze, zg, dt, K, tau, frame, want = exact_case(16, 16, 3, 10, "each")
    shifted = lambda a: torch.cat([torch.zeros(1, device=DEV), cu(a).reshape(-1)])[1:].view(a.shape)
    zs = shifted(ze)
    assert zs.data_ptr() % 16 == 4 and zs.is_contiguous()
    r = ops.vsd(zs, shifted(zg), shifted(dt), cu(K), cu(tau), delta_mm=DELTA)
    assert np.array_equal(host(r["counts"]), want["counts"]) and np.array_equal(host(r["err"]), want["err"])


def test_bad_arguments_are_refused():
    from texpose_amd import _lib, ops
    z = torch.zeros(2, 4, 4, device=DEV)
    K = cu(K_FLAT)
    for T in (0, 17):
        with pytest.raises(_lib.TexposeLibraryError, match="1 .. 16"):
            ops.vsd(z, z, z, K, torch.ones(2, T, device=DEV))
    with pytest.raises(_lib.TexposeLibraryError):
        ops.vsd(z.cpu(), z.cpu(), z.cpu(), K.cpu(), torch.ones(2, 3))
    with pytest.raises(ValueError):
        ops.vsd(z, z, torch.zeros(3, 4, 4, device=DEV), K, torch.ones(2, 3, device=DEV))          # Ft neither 1 nor B, no frame
    with pytest.raises(ValueError):
        ops.vsd(z, z[:1], z, K, torch.ones(2, 3, device=DEV))
    with pytest.raises(ValueError):
        ops.vsd(z, z, z, K, torch.ones(2, 3, device=DEV), frame=torch.zeros(2, device=DEV))          # not int32
    # an out-of-range frame index is clamped, nothing is read past the planes
    ze, zg, dt, Kc, tau, _, _ = exact_case(7, 65, 3, 10, "map")
    got = run(ze, zg, dt, Kc, tau, DELTA, np.array([-5, 1, 99], np.int32))
    want = run(ze, zg, dt, Kc, tau, DELTA, np.array([0, 1, 1], np.int32))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ----------------------------------------------------------------------------- realistic
def rotation(rs):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def rodrigues(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def pose_pairs(rs, B, spread, z=900.0):
    gt = np.stack([np.concatenate([rotation(rs), rs.uniform(-spread, spread, (3, 1)) + [[0.0], [0.0], [z]]], 1) for _ in range(B)])
    est = gt.copy()
    for b in range(B):                                       # a few degrees and millimetres off
        est[b, :, :3] = rodrigues(rs.normal(size=3) * 0.02) @ gt[b, :, :3]
        est[b, :, 3] += rs.uniform(-4, 4, 3)
    return est.astype(np.float32), gt.astype(np.float32)


MESHES = {"sphere": lambda: uv_sphere(24, 32, 50.0, ripple=0.1), "torus": lambda: torus(40, 20)}


@functools.lru_cache(maxsize=None)
def real_case(H, W, B, mesh):
    """The mesh rendered at B true and B estimated poses about 900 mm away; the test depth is the true render plus 2 mm Gaussian noise
    over a wall at 1500 mm, an occluding plane at 700 mm over the left third of the object's columns and 5 % holes; real intrinsics,
    the BOP tolerances.  Rendered and referenced once, read-only."""
    from texpose_amd import ops
    rs = np.random.RandomState(H * 31 + B * 7 + len(mesh))
    verts, faces = MESHES[mesh]()
    K = K_for(H, W) if H < 480 else LINEMOD_K
    est, gt = pose_pairs(rs, B, spread=20.0 if H < 480 else 120.0)
    z = host(ops.mesh_raster(cu(verts), cu(faces, torch.int32), cu(np.concatenate([est, gt])), cu(K), H=H, W=W, face_ids=False, normals=False)["zbuf"])
    ze, zg = z[:B].copy(), z[B:].copy()
    dt = np.where(zg > 0, zg, 1500.0) + rs.normal(0.0, 2.0, zg.shape)
    for b in range(B):
        cols = np.nonzero((zg[b] > 0).any(0))[0]
        dt[b, :, cols[0]:cols[0] + (cols[-1] - cols[0] + 1) // 3] = 700.0
    dt[rs.uniform(size=dt.shape) < 0.05] = 0.0
    dt = dt.astype(np.float32)
    diameter = np.float32(2 * np.abs(verts).max())
    tau = np.tile((np.array(BOP_TAUS, np.float32) * diameter)[None], (B, 1))          # (as pose_error.vsd_from_depth forms them, in fp32)
    Kb = np.tile(K, (B, 1, 1))
    want = V.vsd_ref(ze, zg, dt, Kb, tau, 15.0)
    for a in (ze, zg, dt, Kb, tau, est, gt):
        a.setflags(write=False)
    return dict(ze=ze, zg=zg, dt=dt, K=Kb, tau=tau, want=want, verts=verts, faces=faces, est=est, gt=gt, diameter=float(diameter), H=H, W=W)


def within_ties(name, counts, err, want):
    ties, n_u = want["near_ties"], want["counts"][:, 0]
    print("%-28s n_U %s  n_I %s  near-ties %s  max count diff %d  max err diff %.3e" % (
        name, n_u.tolist(), want["counts"][:, 1].tolist(), ties.tolist(), int(np.abs(counts - want["counts"]).max()),
        float(np.abs(err.astype(np.float64) - want["err64"]).max())))
    assert (n_u > 200).all() and (want["counts"][:, 1] > 100).all(), "the case must cover the object"
    assert (ties <= TIE_CAP * n_u).all(), "the case has too many near-ties to decide anything: %s of %s" % (ties, n_u)
    assert (np.abs(counts.astype(np.int64) - want["counts"]) <= ties[:, None]).all(), (counts, want["counts"])
    assert (np.abs(err.astype(np.float64) - want["err64"]) <= (ties / n_u)[:, None] + ULP1).all()


@pytest.mark.parametrize("H,W,B,mesh", [(120, 160, 5, "sphere"), (120, 160, 5, "torus"), (480, 640, 2, "torus")])
def test_realistic_counts_against_the_helper(H, W, B, mesh):
    c = real_case(H, W, B, mesh)
    counts, err = run(c["ze"], c["zg"], c["dt"], c["K"], c["tau"])
    within_ties("%s %dx%d B=%d" % (mesh, H, W, B), counts, err, c["want"])
    assert (np.diff(c["want"]["err64"], axis=1) <= 0).all() and (c["want"]["counts"][:, 0] > c["want"]["counts"][:, 1]).all()


# ----------------------------------------------------------------------------- the module
def test_module_vsd_renders_and_scores():
    from texpose_amd import ops, pose_error as PE
    c = real_case(120, 160, 5, "torus")
    B, H, W = 5, c["H"], c["W"]
    verts, faces, est, gt, K, dt = cu(c["verts"]), cu(c["faces"], torch.int32), cu(c["est"]), cu(c["gt"]), cu(c["K"]), cu(c["dt"])
    got = PE.vsd(verts, faces, est, gt, K, dt, c["diameter"], H=H, W=W)
    z = ops.mesh_raster(verts, faces, torch.cat([est, gt]), torch.cat([K, K]), H=H, W=W, face_ids=False, normals=False)["zbuf"]
    two = PE.vsd_from_depth(z[:B], z[B:], dt, K, c["diameter"])
    assert got["err"].shape == (B, 10) and torch.equal(got["err"], two["err"]) and torch.equal(got["counts"], two["counts"])
    within_ties("PE.vsd torus", host(got["counts"]), host(got["err"]), c["want"])          # (the same planes and taus as the stored case)
    per_b = PE.vsd(verts, faces, est, gt, K[0], dt, torch.full((B,), c["diameter"]), H=H, W=W)          # one intr, a [B] diameter
    assert torch.equal(per_b["counts"], got["counts"])
    # the true pose against its own noiseless render: nothing is hidden, nothing is misaligned
    clean = PE.vsd(verts, faces, gt, gt, K, z[B:], c["diameter"], H=H, W=W)
    assert (clean["err"] == 0).all() and torch.equal(clean["counts"][:, 0], clean["counts"][:, 1]) and (clean["counts"][:, 2:] == 0).all()
    assert torch.equal(clean["counts"][:, 0].cpu(), (z[B:] > 0).sum((1, 2)).to(torch.int32).cpu())


def test_gpu_route_and_vsd_torch_agree():
    from texpose_amd import pose_error as PE
    c = real_case(120, 160, 5, "sphere")
    t = torch.from_numpy
    cpu = PE.vsd_from_depth(t(c["ze"]), t(c["zg"]), t(c["dt"]), t(c["K"]), c["diameter"])
    gpu = PE.vsd_from_depth(cu(c["ze"]), cu(c["zg"]), cu(c["dt"]), cu(c["K"]), c["diameter"])
    assert np.array_equal(cpu["counts"].numpy(), c["want"]["counts"])              # (the stored case uses the same taus)
    ties = c["want"]["near_ties"]
    assert (np.abs(host(gpu["counts"]).astype(np.int64) - cpu["counts"].numpy()) <= ties[:, None]).all()


# ----------------------------------------------------------------------------- determinism
def test_repeat_into_the_same_out_and_graph_replay():
    from texpose_amd import ops
    c = real_case(120, 160, 5, "sphere")
    args = [cu(c[k]) for k in ("ze", "zg", "dt", "K", "tau")]
    first = ops.vsd(*args)
    out = dict(err=torch.full((5, 10), -7.0, device=DEV), counts=torch.full((5, 12), 12345, device=DEV, dtype=torch.int32))
    again = ops.vsd(*args, out=out)
    assert again["counts"] is out["counts"] and torch.equal(out["counts"], first["counts"]) and torch.equal(out["err"], first["err"])
    ops.vsd(*args, out=out)                                  # not cleared in between
    assert torch.equal(out["counts"], first["counts"]) and torch.equal(out["err"], first["err"])
    cap = dict(err=torch.empty(5, 10, device=DEV), counts=torch.empty(5, 12, device=DEV, dtype=torch.int32))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.vsd(*args, out=cap)
    for _ in range(2):
        cap["counts"].fill_(-1)
        cap["err"].fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap["counts"], first["counts"]) and torch.equal(cap["err"], first["err"])


# ----------------------------------------------------------------------------- the tool
def _tool():
    spec = importlib.util.spec_from_file_location("pose_errors_tool", os.path.join(REPO, "tools", "pose_errors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_ply(path, verts, faces):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces)))
        for p in verts:
            f.write("%r %r %r\n" % tuple(float(v) for v in p))
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(int(v) for v in t))


def _write_scene(root, poses_mm, depth16, info, K, oid):
    """One object per frame through BopSceneWriter (it takes NeRF units at depth.scale 10: mm / 100)."""
    from texpose_amd.bop_scene import BopSceneWriter
    F, H, W = depth16.shape
    w = BopSceneWriter(root, K, 10.0, png_per_metre=2000)
    for f in range(F):
        pose = poses_mm[f].astype(np.float32).copy()
        pose[:, 3] /= 100.0
        w.add_views(pose[None], [oid], info[f][None, None], np.zeros((1, 1, H, W), np.uint8), np.zeros((1, 1, H, W), np.uint8),
                    np.zeros((1, H, W, 3), np.uint8), depth16[f][None])
    w.close()


def test_tool_with_vsd_on_a_written_scene(tmp_path, capsys):
    from texpose_amd import ops
    H, W, F, oid = 120, 160, 4, 7
    verts, faces = uv_sphere(24, 32, 50.0, ripple=0.1)
    K = K_for(H, W)
    rs = np.random.RandomState(3)
    _, gt = pose_pairs(rs, F, spread=15.0)
    z = host(ops.mesh_raster(cu(verts), cu(faces, torch.int32), cu(gt), cu(K), H=H, W=W, face_ids=False, normals=False)["zbuf"])
    depth16 = np.where(z > 0, np.rint(z / 0.5), 0).astype(np.uint16)              # depth_scale 1000 / 2000 = 0.5 mm; 0 on background
    info = np.zeros((F, 10), np.int32)
    info[:, 0] = info[:, 1] = (z > 0).sum((1, 2))
    info[3, 1] = 0                                           # frame 3: recorded as fully occluded -> outside the AR rows
    ply = str(tmp_path / "obj_000007.ply")
    _write_ply(ply, verts, faces)
    root, moved = str(tmp_path / "gt"), str(tmp_path / "moved")
    _write_scene(root, gt, depth16, info, K, oid)
    out = str(tmp_path / "report.json")
    report = _tool().main(["--gt", root, "--est", root, "--vsd", "--ply", "%d=%s" % (oid, ply), "--json", out])
    table = capsys.readouterr().out.splitlines()
    assert table[0].split()[-4:] == ["ar_vsd", "ar_mssd", "ar_mspd", "ar"] and "mean_vsd" in table[0].split()
    row = report[oid]
    assert np.asarray(row["errors"]["vsd"]).shape == (F, 10) and np.asarray(row["errors"]["vsd"]).max() == 0 and row["mean_vsd"] == 0 == row["median_vsd"]
    assert (row["ar_vsd"], row["ar_mssd"], row["ar_mspd"], row["ar"], row["ar_instances"]) == (1.0, 1.0, 1.0, 1.0, 3)
    assert json.load(open(out))["objects"][0]["ar"] == 1.0
    everyone = _tool().main(["--gt", root, "--est", root, "--vsd", "--min-visib", "0", "--ply", "%d=%s" % (oid, ply)])
    assert everyone[oid]["ar_instances"] == 4 and everyone[oid]["ar"] == 1.0
    # frame 1 moved sideways by a little over half a diameter (so that MSSD's strict 0.5 d threshold is not straddled): less than a
    # quarter of the union is shared (VSD > 0.5 at every tau), MSSD = 0.55 d, MSPD ~ 33 px against thresholds up to 12.5 px at this width
    est = gt.copy()
    est[1, 0, 3] += 0.55 * row["diameter"]
    _write_scene(moved, est, depth16, info, K, oid)
    capsys.readouterr()
    off = _tool().main(["--gt", root, "--est", moved, "--vsd", "--ply", "%d=%s" % (oid, ply)])[oid]
    assert min(off["errors"]["vsd"][1]) > 0.5 and max(max(off["errors"]["vsd"][f]) for f in (0, 2, 3)) == 0
    assert off["ar_instances"] == 3
    for k in ("ar_vsd", "ar_mssd", "ar_mspd", "ar"):
        assert off[k] == pytest.approx(2 / 3, abs=1e-12), k
