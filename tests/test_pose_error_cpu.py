"""CPU: the pose-error definitions (tests/pose_error_ref.py, numpy fp64) against anchors that need no library; the CPU route of
texpose_amd/pose_error.py in fp64 against that helper; tools/pose_errors.py on a scene folder written by BopSceneWriter.

The fp64 comparisons are relative, at 1e-12, with no absolute term: both sides evaluate the same definition in fp64 with a different
operation order (and ADD-S with the composed map P_g^-1 P_e on one side, two posed clouds on the other)."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

import pose_error_ref as R
from texpose_amd import pose_error as PE

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
t = torch.from_numpy


def rotation(rs):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def poses(rs, B, spread=40.0, z=900.0):
    return np.stack([np.concatenate([rotation(rs), rs.uniform(-spread, spread, (3, 1)) + [[0.0], [0.0], [z]]], 1) for _ in range(B)])


def near(rs, P, angle=0.05, shift=3.0):
    """Poses a few degrees and millimetres away from P."""
    out = P.copy()
    for b in range(len(P)):
        out[b, :, :3] = R.rotation(rs.normal(size=3), angle * rs.uniform(0.2, 1.0)) @ P[b, :, :3]
        out[b, :, 3] += rs.uniform(-shift, shift, 3)
    return out


def cube(n=5, half=30.0):
    g = np.linspace(-half, half, n)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


K0 = np.array([[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]])


def close(got, want):
    np.testing.assert_allclose(np.asarray(got, dtype=np.float64), want, rtol=1e-12, atol=0)


# ----------------------------------------------------------------------------- the helper against library-free anchors
def test_identical_poses_give_zero():
    rs = np.random.RandomState(0)
    pts, P = rs.uniform(-80, 80, (200, 3)), poses(rs, 3)
    r = R.pose_errors(pts, P, P, None, np.tile(K0, (3, 1, 1)))
    for k in ("add", "mssd", "mspd", "proj"):
        assert (r[k] == 0).all(), k
    assert (R.adds(pts, P, P) == 0).all() and (r["s_mssd"] == 0).all() and (r["s_mspd"] == 0).all()
    re, te = R.re_te(P, P)
    assert (te == 0).all() and (re < 1e-3).all()               # (the clamp at 1 - 1e-7 leaves acos(1 - 1e-7) = 4.5e-4)


def test_pure_translation():
    rs = np.random.RandomState(1)
    pts, P = rs.uniform(-80, 80, (150, 3)), poses(rs, 2)
    v = np.array([3.0, -4.0, 12.0])
    Q = P.copy()
    Q[:, :, 3] += v
    r = R.pose_errors(pts, Q, P)
    np.testing.assert_allclose(r["add"], 13.0, rtol=1e-12)
    np.testing.assert_allclose(r["mssd"], 13.0, rtol=1e-12)
    assert (R.adds(pts, Q, P) <= 13.0 + 1e-9).all()
    np.testing.assert_allclose(R.re_te(Q, P)[1], 13.0, rtol=1e-12)


def test_cube_under_its_quarter_turn():
    pts = cube()
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])          # maps the lattice cube onto itself, exactly
    P = poses(np.random.RandomState(2), 1)
    P[0, :, :3] = np.eye(3)                                                       # (exact arithmetic on the lattice)
    P[0, :, 3] = (8.0, -16.0, 512.0)
    Q = P.copy()
    Q[0, :, :3] = P[0, :, :3] @ Rz
    sym = np.stack([np.eye(3, 4), np.concatenate([Rz, np.zeros((3, 1))], 1)])
    r = R.pose_errors(pts, Q, P, sym)
    assert r["mssd"][0] == 0 and r["s_mssd"][0] == 1 and r["add"][0] > 10 and R.adds(pts, Q, P)[0] == 0
    assert R.pose_errors(pts, Q, P)["mssd"][0] > 10                                # without the symmetry listed it is a large error


def test_two_point_diameter_and_tie_rules():
    a, b = np.array([1.0, 2.0, 3.0]), np.array([4.0, 6.0, 15.0])
    assert R.model_diameter(np.stack([a, b])) == 13.0
    assert float(PE.model_diameter(t(np.stack([a, b])))) == 13.0
    # equal distances: the lowest index wins, in both modes; NaN targets never win; no target: +-inf and -1
    y = np.array([[[1.0, 0, 0], [np.nan, 0, 0], [-1.0, 0, 0], [1.0, 0, 0]]])
    x = np.array([[[0.0, 0, 0], [np.nan, 0, 0]]])
    for mode, none in (("nearest", math.inf), ("farthest", -math.inf)):
        d2, idx, second = R.nn1(x, y, mode=mode, second=True)
        assert idx.tolist() == [[0, -1]] and d2[0, 0] == 1 and d2[0, 1] == none and second[0, 0] == 1
        d2, idx = R.nn1(x, y, y_len=[0], mode=mode)
        assert idx.tolist() == [[-1, -1]] and (d2 == none).all()


def test_p2p_distance_on_hand_built_ragged_clouds():
    x = np.zeros((2, 3, 3))
    y = np.zeros((2, 4, 3))
    x[0, :, 0] = (0, 1, 5)            # cloud 0: three points on the x axis
    y[0, :, 0] = (0, 3, 9, 100)       # nearest squared distances 0, 1, 4 (the fourth target is past y_lengths)
    x[1, :, 1] = (2, 50, 60)          # cloud 1: only the first point counts
    y[1, :, 1] = (0, 1, 51, 61)       # its nearest target among the first two: squared distance 1
    xl, yl = np.array([3, 1]), np.array([3, 2])
    assert R.p2p_distance(x, y, xl, yl, None, None, "sum").tolist() == [5.0, 1.0]
    assert R.p2p_distance(x, y, xl, yl, None, None, "mean").tolist() == [5.0 / 3, 1.0]
    assert R.p2p_distance(x, y, xl, yl, None, "sum", "sum") == 6.0
    assert R.p2p_distance(x, y, xl, yl, None, "mean", "sum") == 3.0
    w = np.array([2.0, 0.5])
    assert R.p2p_distance(x, y, xl, yl, w, "mean", "sum") == (10.0 + 0.5) / 2.5
    assert R.p2p_distance(x, y, xl, yl, np.zeros(2), "mean", "mean") == 0.0
    assert R.p2p_distance(x, y, xl, yl, np.zeros(2), None, "mean").tolist() == [0.0, 0.0]


def test_symmetry_discretisation():
    entry = {"symmetries_discrete": [[-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]],
             "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}
    S = R.symmetry_transforms(entry, 0.5)                   # ceil(pi / 0.5) = 7 steps x (identity + one discrete)
    assert S.shape == (14, 3, 4) and (S[0] == np.eye(3, 4)).all() and (S[1, :, :3] == np.diag([-1.0, -1.0, 1.0])).all()
    np.testing.assert_allclose(S[2, :, :3], R.rotation([0, 0, 1], 2 * math.pi / 7), atol=1e-15)
    # an axis through an offset leaves the offset where it is
    off = {"symmetries_continuous": [{"axis": [0, 1, 0], "offset": [10.0, 0.0, -5.0]}]}
    for T in R.symmetry_transforms(off, 1.0):
        np.testing.assert_allclose(T[:, :3] @ [10.0, 0.0, -5.0] + T[:, 3], [10.0, 0.0, -5.0], atol=1e-12)
    assert R.symmetry_transforms({}).shape == (1, 3, 4)


# ----------------------------------------------------------------------------- the module's CPU route (fp64) against the helper
@pytest.mark.parametrize("B, M, S, with_intr", [(1, 1, 1, True), (3, 257, 4, True), (5, 100, 1, False), (2, 64, 7, True)])
def test_module_pose_errors_match_the_helper(B, M, S, with_intr):
    rs = np.random.RandomState(10 * B + S)
    pts, Pg = rs.uniform(-100, 100, (M, 3)), poses(rs, B)
    Pe = near(rs, Pg)
    sym = np.stack([np.eye(3, 4)] + [np.concatenate([rotation(rs), rs.uniform(-2, 2, (3, 1))], 1) for _ in range(S - 1)])
    K = np.tile(K0, (B, 1, 1)) if with_intr else None
    want = R.pose_errors(pts, Pe, Pg, sym, K)
    got = PE.pose_errors(t(pts), t(Pe), t(Pg), t(sym), None if K is None else t(K))
    assert set(got) == ({"add", "mssd", "s_mssd"} | ({"mspd", "proj", "s_mspd"} if with_intr else set()))
    for k, v in got.items():
        assert v.shape == (B,)
        if k.startswith("s_"):
            assert v.dtype == torch.int32 and v.tolist() == want[k].tolist(), k
        else:
            close(v, want[k])
    close(PE.add(t(pts), t(Pe), t(Pg)), want["add"])
    close(PE.mssd(t(pts), t(Pe), t(Pg), t(sym)), want["mssd"])
    close(PE.adds(t(pts), t(Pe), t(Pg)), R.adds(pts, Pe, Pg))
    re, te = PE.re_te(t(Pe), t(Pg))
    close(re, R.re_te(Pe, Pg)[0])
    close(te, R.re_te(Pe, Pg)[1])
    if with_intr:
        close(PE.mspd(t(pts), t(Pe), t(Pg), t(K0), t(sym)), want["mspd"])          # (one [3,3] for every pose)
        close(PE.proj(t(pts), t(Pe), t(Pg), t(K)), want["proj"])


def test_module_point_behind_the_camera():
    rs = np.random.RandomState(3)
    pts, Pg = rs.uniform(-100, 100, (50, 3)), poses(rs, 2)
    Pe = near(rs, Pg)
    Pe[1, 2, 3] = 20.0                                    # pose 1: the model straddles the camera plane
    got = PE.pose_errors(t(pts), t(Pe), t(Pg), None, t(np.tile(K0, (2, 1, 1))))
    want = R.pose_errors(pts, Pe, Pg, None, np.tile(K0, (2, 1, 1)))
    assert math.isnan(want["mspd"][1]) and want["s_mspd"][1] == -1 and math.isfinite(want["mspd"][0])
    assert torch.isnan(got["mspd"][1]) and torch.isnan(got["proj"][1]) and int(got["s_mspd"][1]) == -1
    assert torch.isfinite(got["add"]).all() and torch.isfinite(got["mssd"]).all() and torch.isfinite(got["mspd"][0])
    close(got["add"], want["add"])


def test_module_search_matches_the_helper_and_chunks(monkeypatch):
    rs = np.random.RandomState(4)
    x, y = rs.uniform(-100, 100, (3, 70, 3)), rs.uniform(-100, 100, (3, 90, 3))
    y[:, 5] = y[:, 2]                                     # a duplicated target: the lower index must win
    x[1, 7], y[2, 11, 1] = np.nan, np.nan
    A = near(rs, np.tile(np.eye(3, 4), (3, 1, 1)))
    xl, yl = np.array([70, 0, 33]), np.array([90, 17, 0])
    monkeypatch.setattr(PE, "CHUNK_BYTES", 3 * 90 * 3 * 8 * 16)          # 16 queries per block: five chunks
    for mode in ("nearest", "farthest"):
        for kw in (dict(), dict(A=A), dict(x_len=xl, y_len=yl), dict(A=A, x_len=xl, y_len=yl)):
            for yy in (y, y[:1]):
                kw_ref = dict(kw)
                if "y_len" in kw and len(yy) == 1:
                    kw_ref["y_len"] = yl[:1]
                d2, idx = R.nn1(x, yy, mode=mode, **kw_ref)
                g2, gidx = PE.nn1(t(x), t(yy), mode=mode, **{k: t(v) for k, v in kw_ref.items()})
                assert gidx.dtype == torch.int32 and np.array_equal(gidx.numpy(), idx), (mode, sorted(kw))
                close(g2, d2)
    # one model searched under B maps (shared queries, shared targets): what adds does
    d2, idx = R.nn1(x[:1], y[:1], A=A)
    g2, gidx = PE.nn1(t(x[:1]), t(y[:1]), A=t(A))
    assert g2.shape == (3, 70) and np.array_equal(gidx.numpy(), idx)


def test_module_diameter_and_p2p_match_the_helper():
    rs = np.random.RandomState(5)
    pts = rs.uniform(-100, 100, (300, 3))
    close(PE.model_diameter(t(pts)), R.model_diameter(pts))
    x, y = rs.normal(size=(3, 40, 3)), rs.normal(size=(3, 55, 3))
    xl, yl, w = np.array([40, 1, 17]), np.array([55, 30, 2]), np.array([0.5, 0.0, 3.0])
    for br in ("mean", "sum", None):
        for pr in ("mean", "sum"):
            for lens in ((None, None), (xl, yl)):
                for ww in (None, w):
                    got, none = PE.p2p_distance(t(x), t(y), *(None if v is None else t(v) for v in lens), weights=None if ww is None else t(ww),
                                                batch_reduction=br, point_reduction=pr)
                    assert none is None and not got.requires_grad
                    close(got, R.p2p_distance(x, y, lens[0], lens[1], ww, br, pr))
    zero, _ = PE.p2p_distance(t(x), t(y), weights=torch.zeros(3, dtype=torch.float64))
    assert zero.shape == () and float(zero) == 0.0
    assert PE.p2p_distance(t(x), t(y), weights=torch.zeros(3, dtype=torch.float64), batch_reduction=None)[0].tolist() == [0.0] * 3
    with pytest.raises(NotImplementedError):
        PE.p2p_distance(t(x), t(y), x_normals=t(x))
    with pytest.raises(ValueError):
        PE.p2p_distance(t(x), t(y), weights=torch.tensor([1.0, -1.0, 1.0], dtype=torch.float64))
    with pytest.raises(ValueError):
        PE.p2p_distance(t(x), t(y), batch_reduction="max")
    xg = t(x).clone().requires_grad_()
    assert not PE.p2p_distance(xg, t(y))[0].requires_grad          # documented: not differentiable


def test_module_symmetry_transforms_recall_and_auc():
    entry = {"symmetries_discrete": [[-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]],
             "symmetries_continuous": [{"axis": [0, 0, 1], "offset": [1.0, 2.0, 0.0]}]}
    S = PE.symmetry_transforms(entry, 0.5)
    assert S.dtype == torch.float64
    np.testing.assert_allclose(S.numpy(), R.symmetry_transforms(entry, 0.5), atol=1e-14)
    assert PE.symmetry_transforms({}).tolist() == [np.eye(3, 4).tolist()]
    full = R.symmetry_transforms(entry)                    # the BOP default 0.01: 315 steps x 2
    assert len(full) == 630
    with pytest.warns(UserWarning, match="subsampled"):
        sub = PE.symmetry_transforms(entry, diameter=100.0)
    assert sub.shape == (64, 3, 4) and (sub[0].numpy() == np.eye(3, 4)).all()
    np.testing.assert_allclose(sub.numpy(), full[[int(i * 630 / 64) for i in range(64)]], atol=1e-14)
    assert PE.recall([1.0, 2.0, 3.0, math.nan], 2.5) == 0.5 and PE.recall(torch.tensor([1.0, 2.0, 3.0]), [0.5, 2.0, 10.0]) == [0.0, 1 / 3, 1.0]
    for one in (2.5, np.float64(2.5), torch.tensor(2.5)):          # a 0-dim tensor is one threshold: a float, not a list
        assert PE.recall([1.0, 2.0, 3.0], one) == 2 / 3
    assert PE.recall([1.0, 2.0, 3.0], torch.tensor([2.5])) == [2 / 3]
    assert PE.auc([0.0, 5.0, 20.0, math.nan], 10.0) == (1.0 + 0.5) / 4


def test_ops_refuse_cpu_tensors():
    from texpose_amd import _lib, ops
    with pytest.raises(_lib.TexposeLibraryError):
        ops.nn1(torch.zeros(1, 2, 3), torch.zeros(1, 2, 3))
    with pytest.raises(_lib.TexposeLibraryError):
        ops.pose_errors(torch.zeros(2, 3), torch.zeros(1, 3, 4), torch.zeros(1, 3, 4))


def test_library_refuses_bad_arguments_without_a_gpu():
    import ctypes as C
    from texpose_amd import _lib
    lib = _lib.load()
    assert (_lib.NN1_TILE, _lib.NN1_QUERIES_PER_BLOCK, _lib.POSE_ERRORS_MAX_SYM, _lib.NN1_NEAREST, _lib.NN1_FARTHEST) == (1024, 1024, 64, 0, 1)
    a = _lib.Nn1Args()
    assert lib.tp_nn1(C.byref(a), None) < 0 and b"bad sizes" in lib.tp_last_error()
    a.B = a.Bx = a.Bt = 1
    a.P1, a.P2 = 5000, 5000
    assert lib.tp_nn1_workspace_bytes(C.byref(a)) == 5000 * 8          # few workgroups: the five target tiles become slices
    a.target_slices = 1
    assert lib.tp_nn1_workspace_bytes(C.byref(a)) == 0
    a.B = a.Bx = 600
    a.target_slices = 0
    assert lib.tp_nn1_workspace_bytes(C.byref(a)) == 0                  # enough workgroups without slices
    p = _lib.PoseErrorsArgs()
    dummy = C.c_double()
    for f in ("pts", "pose_est", "pose_gt", "sym", "out", "s_mssd", "workspace"):
        setattr(p, f, C.addressof(dummy))
    p.M, p.B, p.S = 10, 1, 65
    assert lib.tp_pose_errors(C.byref(p), None) == -1 and b"at most 64" in lib.tp_last_error()


# ----------------------------------------------------------------------------- the tool
def _tool():
    spec = importlib.util.spec_from_file_location("pose_errors_tool", os.path.join(REPO, "tools", "pose_errors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write_scene(root, P, ids):
    """P [F,K,3,4] (t in mm; the writer takes NeRF units at depth.scale 10: mm / 100) through BopSceneWriter, one call per frame."""
    from texpose_amd.bop_scene import BopSceneWriter, read_bop_frame
    F, K = P.shape[:2]
    H, W = 4, 6
    # the writer gives every object of a view the view's pose: one writer per object, then the files are merged
    gt = {}
    for k in range(K):
        sub = os.path.join(root, "obj%d" % k)
        w = BopSceneWriter(sub, K0, 10.0, png_per_metre=2000)
        for f in range(F):
            pose = P[f, k].astype(np.float32).copy()
            pose[:, 3] /= 100.0
            w.add_views(pose[None], [ids[k]], np.zeros((1, 1, 10), np.int32), np.zeros((1, 1, H, W), np.uint8), np.zeros((1, 1, H, W), np.uint8),
                        np.zeros((1, H, W, 3), np.uint8), np.zeros((1, H, W), np.uint16))
        w.close()
        fr = read_bop_frame(sub, 0)
        assert fr["obj_id"].tolist() == [ids[k]] and fr["cam_K"].shape == (3, 3)
        for key, entries in json.load(open(os.path.join(sub, "scene_gt.json"))).items():
            gt.setdefault(key, []).extend(entries)
    json.dump(gt, open(os.path.join(root, "scene_gt.json"), "w"))
    json.dump(json.load(open(os.path.join(root, "obj0", "scene_camera.json"))), open(os.path.join(root, "scene_camera.json"), "w"))


def _write_ply(path, pts):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % len(pts))
        for p in pts:
            f.write("%r %r %r\n" % tuple(float(v) for v in p))


@pytest.fixture
def scene(tmp_path):
    rs = np.random.RandomState(6)
    F, ids = 4, [5, 9]
    P = np.stack([poses(rs, 2) for _ in range(F)]).astype(np.float32).astype(np.float64)
    root = str(tmp_path / "gt")
    os.makedirs(root)
    _write_scene(root, P, ids)
    plys = {}
    for k, oid in enumerate(ids):
        plys[oid] = str(tmp_path / ("obj_%06d.ply" % oid))
        _write_ply(plys[oid], cube(4, 20.0 + 10 * k) + rs.uniform(-1, 1, (64, 3)))
    return dict(root=root, P=P, ids=ids, plys=plys, tmp=tmp_path, ply_args=[a for oid, p in plys.items() for a in ("--ply", "%d=%s" % (oid, p))])


def test_tool_on_a_scene_against_itself(scene, capsys):
    out = str(scene["tmp"] / "report.json")
    report = _tool().main(["--gt", scene["root"], "--est", scene["root"], "--device", "cpu", "--json", out] + scene["ply_args"])
    table = capsys.readouterr().out.splitlines()
    assert len(table) == 3 and table[0].split()[:3] == ["object", "poses", "diameter"]
    saved = {o["object"]: o for o in json.load(open(out))["objects"]}
    assert sorted(report) == sorted(saved) == [5, 9]
    for oid, row in report.items():
        assert row["poses"] == 4 and row["missing"] == [] and row["failed_add"] == [] and row["frames"] == [0, 1, 2, 3]
        assert abs(row["diameter"] - R.model_diameter(np.loadtxt(scene["plys"][oid], skiprows=7))) < 1e-4          # (the reader keeps float32)
        for k in ("add", "adds", "mssd", "mspd", "proj", "te"):
            assert max(row["errors"][k]) <= 1e-9 and row["mean_" + k] <= 1e-9 and row["median_" + k] <= 1e-9, k
        assert max(row["errors"]["re"]) < 0.03                      # degrees: rotation_distance clamps the cosine at 1 - 1e-7
        recalls = {k: v for k, v in row.items() if k.startswith("recall_")}
        assert len(recalls) == 8 and all(v == 1.0 for v in recalls.values()), recalls
        assert saved[oid]["recall_add_0.1"] == 1.0 and saved[oid]["errors"]["add"] == row["errors"]["add"]


def test_tool_with_one_pose_perturbed(scene):
    # estimates as a results CSV: object 9 is off by 40 % of its diameter in frame 2, and has no estimate in frame 3
    est = str(scene["tmp"] / "results.csv")
    P = scene["P"].copy()
    P[2, 1, :, 3] += (0.0, 40.0, 0.0)
    with open(est, "w") as f:
        f.write("scene_id,im_id,obj_id,score,R,t,time\n")
        for frame in range(4):
            for k, oid in enumerate(scene["ids"]):
                if (frame, oid) == (3, 9):
                    continue
                f.write("1,%d,%d,0.9,%s,%s,-1\n" % (frame, oid, " ".join(repr(float(v)) for v in P[frame, k, :, :3].reshape(9)),
                                                    " ".join(repr(float(v)) for v in P[frame, k, :, 3])))
                # a worse-scored distractor for the same frame and object
                f.write("1,%d,%d,0.1,%s,%s,-1\n" % (frame, oid, " ".join(["1 0 0 0 1 0 0 0 1"]), "0 0 5000"))
    report = _tool().main(["--gt", scene["root"], "--est", est, "--device", "cpu"] + scene["ply_args"])
    assert report[5]["failed_add"] == [] and report[5]["recall_add_0.1"] == 1.0
    row = report[9]
    assert row["failed_add"] == [2, 3] and row["missing"] == [3] and row["frames"] == [0, 1, 2]
    assert row["recall_add_0.1"] == 0.5 and row["recall_adds_0.1"] == 0.5 and row["recall_50mm_5deg"] == 0.75
    np.testing.assert_allclose(row["errors"]["add"], [0.0, 0.0, 40.0], atol=1e-3)          # (the scene stores float32 mm)
    np.testing.assert_allclose(row["errors"]["te"], [0.0, 0.0, 40.0], atol=1e-3)
    assert row["errors"]["adds"][2] <= 40.0 + 1e-6 and row["errors"]["proj"][2] > 5.0 and row["recall_proj_5px"] == 0.5
