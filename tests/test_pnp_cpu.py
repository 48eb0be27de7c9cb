"""No GPU: the numpy restatement of K28 (tests/pnp_ref.py) against independent facts, `pnp.score_torch` against the restatement, and
the host side of the four entry points: the header-derived binding and the argument checks, which launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import pnp_ref as REF
from test_gpu_surfel import torus, uv_sphere

LINEMOD_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)


def rotation(rs):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def project(X, P, K):
    x = X.astype(np.float64) @ P[:, :3].T + P[:, 3]
    return np.stack([K[0, 0] * x[:, 0] / x[:, 2] + K[0, 2], K[1, 1] * x[:, 1] / x[:, 2] + K[1, 2]], 1)


# ----------------------------------------------------------------------------- the binding and the argument checks
def test_binding_has_the_new_entry_points():
    from texpose_amd import _lib
    for name in ("tp_pnp_workspace_bytes", "tp_corr_from_nocs", "tp_pnp_hypotheses", "tp_pnp_score", "tp_pnp_refine"):
        assert name in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 16 and _lib.PNP_MAX_HYP == 4096 and _lib.PNP_MAX_ITERS == 32
    restype, argtypes = _lib.HEADER.prototypes["tp_pnp_workspace_bytes"]
    assert restype is C.c_size_t and argtypes == [C.c_int] * 3
    for cls, fields in ((_lib.CorrFromNocsArgs, ("nocs", "mask", "mask_is_float", "centre", "scale", "B", "H", "W", "stride", "xy", "xyz", "count", "workspace")),
                        (_lib.PnpHypothesesArgs, ("xy", "xyz", "count", "intr", "B", "N", "T", "seed", "sample_idx", "hyp", "hyp_valid")),
                        (_lib.PnpScoreArgs, ("xy", "xyz", "count", "intr", "poses", "valid", "B", "N", "T", "tau_px", "inliers", "sel", "inlier_mask")),
                        (_lib.PnpRefineArgs, ("xy", "xyz", "count", "intr", "hyp", "hyp_valid", "hyp_inliers", "B", "N", "T", "tau_px", "iters",
                                              "pose", "inliers", "rms", "status", "workspace"))):
        assert tuple(n for n, _ in cls._fields_) == fields
    assert dict(_lib.PnpHypothesesArgs._fields_)["seed"] is C.c_uint64
    assert C.sizeof(dict(_lib.CorrFromNocsArgs._fields_)["centre"]) == 12


def test_workspace_bytes():
    from texpose_amd import _lib
    ws = _lib.load().tp_pnp_workspace_bytes
    for B, N, T in ((1, 1, 1), (3, 1025, 300), (64, 307200, 256)):
        want = 8 * 32 * B * (1 + -(-N // 1024)) + 4 * B * -(-N // 256)
        assert ws(B, N, T) == (want + 15) // 16 * 16
    assert ws(0, 5, 5) == 0 and ws(5, 0, 5) == 0 and ws(5, 5, -1) == 0


def test_argument_errors_launch_nothing():
    """Every pointer is a host buffer: a launch would fault, a refusal returns before anything reads them."""
    from texpose_amd import _lib
    lib = _lib.load()
    buf = C.create_string_buffer(4096)
    p = C.addressof(buf) + (-C.addressof(buf)) % 16

    def filled(cls, **kw):
        a = cls()
        for name, t in cls._fields_:
            if t is C.c_void_p:
                setattr(a, name, p)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    err = lambda: lib.tp_last_error()
    for fn in (lib.tp_corr_from_nocs, lib.tp_pnp_hypotheses, lib.tp_pnp_score, lib.tp_pnp_refine):
        assert fn(None, None) == -1 and b"null args" in err()
    for fn, cls in ((lib.tp_corr_from_nocs, _lib.CorrFromNocsArgs), (lib.tp_pnp_hypotheses, _lib.PnpHypothesesArgs), (lib.tp_pnp_score, _lib.PnpScoreArgs),
                    (lib.tp_pnp_refine, _lib.PnpRefineArgs)):
        a = cls()                                                # sizes in range, every pointer null
        for name, value in dict(B=1, N=8, T=4, H=4, W=4, stride=1, tau_px=2.0, iters=5).items():
            if hasattr(a, name):
                setattr(a, name, value)
        assert fn(C.byref(a), None) == -1 and b"null pointer" in err(), cls
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(stride=0), dict(H=65536, W=32768)):
        a = filled(_lib.CorrFromNocsArgs, **{**dict(B=1, H=4, W=4, stride=1), **bad})
        assert lib.tp_corr_from_nocs(C.byref(a), None) == -1 and b"bad sizes" in err(), bad
    sizes = (dict(B=0), dict(N=0), dict(T=0), dict(T=4097), dict(B=-3))
    for bad in sizes:
        a = filled(_lib.PnpHypothesesArgs, **{**dict(B=1, N=8, T=4), **bad})
        assert lib.tp_pnp_hypotheses(C.byref(a), None) == -1 and b"bad sizes" in err(), bad
        a = filled(_lib.PnpScoreArgs, **{**dict(B=1, N=8, T=4, tau_px=2.0), **bad})
        assert lib.tp_pnp_score(C.byref(a), None) == -1 and b"bad sizes" in err(), bad
        a = filled(_lib.PnpRefineArgs, **{**dict(B=1, N=8, T=4, tau_px=2.0, iters=5), **bad})
        assert lib.tp_pnp_refine(C.byref(a), None) == -1 and b"bad sizes" in err(), bad
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        a = filled(_lib.PnpScoreArgs, B=1, N=8, T=4, tau_px=tau)
        assert lib.tp_pnp_score(C.byref(a), None) == -1 and b"tau_px" in err(), tau
        a = filled(_lib.PnpRefineArgs, B=1, N=8, T=4, tau_px=tau, iters=5)
        assert lib.tp_pnp_refine(C.byref(a), None) == -1 and b"tau_px" in err(), tau
    for iters in (-1, 33):
        a = filled(_lib.PnpRefineArgs, B=1, N=8, T=4, tau_px=2.0, iters=iters)
        assert lib.tp_pnp_refine(C.byref(a), None) == -1 and b"iters" in err(), iters
    a = filled(_lib.PnpRefineArgs, B=1, N=8, T=4, tau_px=2.0, iters=5, workspace=p + 8)
    assert lib.tp_pnp_refine(C.byref(a), None) == -1 and b"aligned" in err()


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    from texpose_amd import _lib, ops
    xy, xyz, count, K = torch.zeros(1, 8, 2), torch.zeros(1, 8, 3), torch.zeros(1, dtype=torch.int32), torch.eye(3)
    for call in (lambda: ops.pnp_hypotheses(xy, xyz, count, K), lambda: ops.pnp_score(xy, xyz, count, K, torch.zeros(1, 2, 12)),
                 lambda: ops.pnp_refine(xy, xyz, count, K, torch.zeros(1, 3, 4)), lambda: ops.pnp_ransac(xy, xyz, count, K),
                 lambda: ops.corr_from_nocs(torch.zeros(1, 4, 4, 3), torch.ones(1, 4, 4), [0, 0, 0], [1, 1, 1])):
        with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
            call()
    from texpose_amd import pnp
    with pytest.raises(_lib.TexposeLibraryError):
        pnp.PnPSolver(4, 4, "cpu")


# ----------------------------------------------------------------------------- the index rule
@pytest.mark.parametrize("n", [4, 5, 1000])
def test_sample_indices_are_distinct_in_range_and_reproducible(n):
    idx = REF.sample_indices(seed=7, b=2, T=500, n=n)
    assert idx.shape == (500, 4) and idx.dtype == np.int32
    assert idx.min() >= 0 and idx.max() < n
    assert all(len(set(row)) == 4 for row in idx.tolist())
    assert np.array_equal(idx, REF.sample_indices(seed=7, b=2, T=500, n=n))
    assert np.array_equal(idx[:100], REF.sample_indices(seed=7, b=2, T=100, n=n))          # (a function of h, not of T)
    assert not np.array_equal(idx, REF.sample_indices(seed=8, b=2, T=500, n=n))
    assert not np.array_equal(idx, REF.sample_indices(seed=7, b=3, T=500, n=n))
    assert not np.array_equal(idx, REF.sample_indices(seed=7 + 2 ** 32, b=2, T=500, n=n))          # (the high word is in the key)
    if n == 4:
        assert all(sorted(row) == [0, 1, 2, 3] for row in idx.tolist())
    elif n == 5:                                                 # every entry comes first somewhere, and last somewhere
        assert all(len(set(idx[:, k].tolist())) == 5 for k in range(4))
    else:                                                        # 500 uniform draws from 1000 hit 1000 (1 - e^-0.5) = 393 values on average
        assert all(len(set(idx[:, k].tolist())) >= 350 for k in range(4)) and len(set(idx.reshape(-1).tolist())) >= 800          # (2000 draws: 865)
    assert np.array_equal(REF.sample_indices(1, 0, 5, 3), np.full((5, 4), -1))


def test_sample_indices_first_draw_is_mulhi():
    from oracle.texpose_oracle import philox4x32
    w = philox4x32(np.array([[1, 9, 0x706E7034, 0]], np.uint32), (5, 0))[0].astype(np.uint64)
    idx = REF.sample_indices(seed=5, b=1, T=10, n=77)[9]
    assert idx[0] == int(w[0]) * 77 >> 32
    i1 = int(w[1]) * 76 >> 32
    assert idx[1] == i1 + (i1 >= idx[0])


# ----------------------------------------------------------------------------- P3P and the whole chain on known poses
@pytest.mark.parametrize("mesh", ["sphere", "torus"])
def test_restatement_recovers_known_poses(mesh):
    verts, _ = uv_sphere(12, 16, 50.0, ripple=0.1) if mesh == "sphere" else torus(20, 10)
    verts = verts[np.unique(np.round(verts, 3), axis=0, return_index=True)[1]]          # (the sphere repeats its pole vertices)
    rs = np.random.RandomState(len(mesh))
    B, N = 2, len(verts)
    P = np.stack([np.concatenate([rotation(rs), np.array([[15.0 * b - 10], [8.0], [700.0 + 150 * b]])], 1) for b in range(B)])
    xy = np.stack([project(verts, P[b], LINEMOD_K) for b in range(B)]).astype(np.float32)
    xyz = np.tile(verts[None], (B, 1, 1))
    K = np.tile(LINEMOD_K, (B, 1, 1))
    count = np.array([N, N - 7], np.int32)
    hy = REF.hypotheses_ref(xy, xyz, count, K, 48, seed=11)
    assert hy["ill"].mean() <= 0.05
    for b in range(B):
        assert hy["sample_idx"][b].max() < count[b]
        assert hy["valid"][b].all()
        for h in np.nonzero(~hy["ill"][b])[0]:
            re, te = REF.pose_error(hy["hyp"][b, h], P[b])
            R = hy["hyp"][b, h, :, :3]
            assert re < 0.05 and te < 0.5, (b, h, re, te)          # fp32 pixel coordinates: ~3e-5 px of noise on a minimal sample
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
    out = REF.ransac_ref(xy, xyz, count, K, T=16, tau=2.0, iters=3, seed=11)
    assert (out["status"] == 0).all() and np.array_equal(out["inliers"], count) and (out["rms"] < 1e-3).all()
    for b in range(B):
        re, te = REF.pose_error(out["pose"][b], P[b])
        assert re < 1e-3 and te < 0.02, (re, te)


def test_restatement_degenerate_samples():
    K = LINEMOD_K
    X = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [3, 3, 5]], np.float64)
    P = np.concatenate([np.eye(3), [[0], [0], [500.0]]], 1)
    uv = project(X, P, K)
    assert REF.p3p_ref(uv, X, K)["valid"]
    line = uv.copy()
    line[2] = 2 * uv[1] - uv[0]
    assert not REF.p3p_ref(line, X, K)["valid"]                  # collinear image points
    same = X.copy()
    same[1] = same[0]
    assert not REF.p3p_ref(uv, same, K)["valid"]                 # two equal model points: no finite quartic
    bad = uv.copy()
    bad[3, 0] = np.nan
    assert not REF.p3p_ref(bad, X, K)["valid"]
    tiny = uv.copy()
    tiny[1:3] = uv[0] + [[1.0, 0.0], [0.0, 1.0]]
    assert REF.p3p_ref(tiny, X, K)["ill"]                        # half a square pixel


def test_restatement_refine_converges_keeps_best_and_flags_rank_deficiency():
    verts, _ = torus(20, 10)
    rs = np.random.RandomState(5)
    P = np.concatenate([rotation(rs), [[5.0], [-12.0], [800.0]]], 1)
    xy = (project(verts, P, LINEMOD_K) + rs.normal(0, 0.3, (len(verts), 2))).astype(np.float32)
    w = rs.normal(size=3)
    w *= np.radians(2.0) / np.linalg.norm(w)
    start = np.concatenate([REF._exp_so3(w) @ P[:, :3], P[:, 3:] + [[3.0], [-3.0], [2.6]]], 1)
    r0 = REF.refine_ref(xy, verts, len(verts), LINEMOD_K, start, 4.0, 0)
    assert r0["status"] == 0 and np.allclose(r0["pose"], start.astype(np.float32))
    r5 = REF.refine_ref(xy, verts, len(verts), LINEMOD_K, start, 4.0, 5)
    assert r5["status"] == 0 and r5["inliers"] >= r0["inliers"] and r5["inliers"] == len(verts) and r5["rms"] < 0.5
    re, te = REF.pose_error(r5["pose"], P)
    assert re < 0.2 and te < 1.0          # (from 2 deg, 5 mm; the relative damping slows the weakly observed rotation / translation pair: linear, not quadratic)
    r20 = REF.refine_ref(xy, verts, len(verts), LINEMOD_K, start, 4.0, 20)
    assert r20["rms"] <= r5["rms"] <= r0["rms"] and REF.pose_error(r20["pose"], P)[0] < 0.05
    one = np.tile(verts[:1], (50, 1))
    r = REF.refine_ref(np.tile(xy[:1], (50, 1)), one, 50, LINEMOD_K, P, 4.0, 5)
    assert r["status"] == 3 and np.allclose(r["pose"], P.astype(np.float32))


# ----------------------------------------------------------------------------- score_torch
def score_case(rs, B, N, T):
    X = rs.uniform(-60, 60, (B, N, 3)).astype(np.float32)
    P = np.stack([np.concatenate([rotation(rs), [[0.0], [0.0], [600.0]]], 1) for _ in range(B)])
    xy = np.stack([project(X[b], P[b], LINEMOD_K) for b in range(B)]) + rs.normal(0, 0.5, (B, N, 2))
    out = rs.uniform(size=(B, N)) < 0.3
    xy[out] = rs.uniform(0, 640, (int(out.sum()), 2))
    poses = np.tile(P[:, None], (1, T, 1, 1))
    poses[:, 1:, :, 3] += rs.normal(0, 0.5, (B, T - 1, 3))
    poses[:, -1, 2, 3] = -500.0                                  # behind the camera
    return xy.astype(np.float32), X, np.tile(LINEMOD_K, (B, 1, 1)), poses.reshape(B, T, 12).astype(np.float32)


def test_score_torch_equals_the_restatement():
    from texpose_amd import pnp
    rs = np.random.RandomState(2)
    xy, X, K, poses = score_case(rs, 3, 257, 9)
    X[0, 5] = np.nan
    xy[1, 7] = np.inf
    poses[2, 3] = 1e30
    poses[2, 4, 0] = np.inf
    count = np.array([257, 0, 300], np.int32)                    # (300: clamped to N)
    valid = np.ones((3, 9), np.uint8)
    valid[0, 2] = 0
    want, _ = REF.score_ref(xy, X, count, K, poses, 2.0, valid)
    t = torch.from_numpy
    got = pnp.score_torch(t(xy), t(X), t(count), t(K), t(poses), 2.0, t(valid), chunk=4)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    assert want[0, 0] > 100 and want[0, 2] == 0 and (want[1] == 0).all() and want[2, -1] == 0 and want[2, 3] == 0 and want[2, 4] == 0
    assert np.array_equal(pnp.score_torch(t(xy), t(X), t(count), t(K[0]), t(poses).reshape(3, 9, 3, 4), 2.0).numpy(),
                          REF.score_ref(xy, X, count, K, poses, 2.0)[0])


def test_corr_from_nocs_restatement():
    nocs = np.zeros((1, 3, 5, 3), np.float32)
    nocs[0, :, :, 0] = np.arange(5)[None] / 4.0
    nocs[0, :, :, 1] = np.arange(3)[:, None] / 2.0
    nocs[0, 2, 4, 2] = np.nan
    mask = np.ones((1, 3, 5), np.uint8)
    mask[0, 0, 2] = 0
    xy, xyz, count = REF.corr_from_nocs_ref(nocs, mask, [1.0, 2.0, 3.0], [10.0, 20.0, 30.0], 2)
    assert xy.shape == (1, 6, 2) and count.tolist() == [4]       # rows 0, 2 x columns 0, 2, 4, minus the hole and the NaN
    assert xy[0, :4].tolist() == [[0.5, 0.5], [4.5, 0.5], [0.5, 2.5], [2.5, 2.5]]
    assert xyz[0, :4].tolist() == [[-9.0, -18.0, -27.0], [11.0, -18.0, -27.0], [-9.0, 22.0, -27.0], [1.0, 22.0, -27.0]]
