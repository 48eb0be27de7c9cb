"""GPU: the PnP-RANSAC kernels K28 (`ops.corr_from_nocs`, `ops.pnp_hypotheses`, `ops.pnp_score`, `ops.pnp_refine`, `ops.pnp_ransac`),
`texpose_amd.pnp` and `tools/pnp_poses.py` against the numpy restatement tests/pnp_ref.py.

What must be EQUAL: the correspondence lists (fp32, the same expression), the sample indices (integers), and the inlier counts
wherever every decision is exact in fp32 (the constructed case: errors that are multiples of 5/16 against tau = 5/16) or cannot be
taken at all (NaN, Inf, 1e30).  On realistic data a count may differ from the restatement's by at most the case's number of near-ties
(entries within 1e-3 px of tau), which is printed and may itself be at most 0.1 % of n: a condition on the case.

Where the issue leaves a figure to the case:
  * noise-free hypotheses: a device hypothesis must be the true pose within 4x (the margin for the fp32 store) the largest error the
    restatement's own fp64 P3P makes against the truth on the same samples, over the samples it does not flag as ill-conditioned (at
    most 5 % of them: a condition on the case).  "Noise-free" still means pixel coordinates rounded to fp32 (3e-5 px) on minimal
    samples; the bound is printed (DESIGN section 18 records it).
  * end to end, both poses are compared with the truth after the final fp32 store, the restatement's included."""
import functools
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pnp_ref as REF
from test_gpu_surfel import K_for, torus

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINEMOD_K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]], np.float32)
TIE_CAP = 1e-3
SIZES_N = [4, 63, 64, 65, 257, 1025]
SIZES_T = [1, 64, 65, 300]


def cu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def host(t):
    return t.detach().cpu().numpy()


def rotation(rs):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def project(X, P, K):
    x = X.astype(np.float64) @ P[:, :3].T + P[:, 3]
    return np.stack([K[0, 0] * x[:, 0] / x[:, 2] + K[0, 2], K[1, 1] * x[:, 1] / x[:, 2] + K[1, 2]], 1)


def counts_for(B, N):
    """count differs per image and includes 0, 3 and N (one image: N)."""
    return np.array([N] if B == 1 else [N, 3, 0], np.int32)


# ----------------------------------------------------------------------------- corr_from_nocs
@pytest.mark.parametrize("H,W", [(37, 53), (64, 80)])
def test_corr_from_nocs_equals_the_restatement(H, W):
    from texpose_amd import ops
    rs = np.random.RandomState(H)
    B = 3
    nocs = rs.uniform(0, 1, (B, H, W, 3)).astype(np.float32)
    nocs[rs.uniform(size=nocs.shape) < 0.02] = np.nan
    nocs[0, 0, 0] = np.inf
    mask = (rs.uniform(size=(B, H, W)) < 0.6).astype(np.uint8)
    mask[:, H // 3:H // 2, W // 4:W // 2] = 0                    # a hole
    mask[1] = 0                                                 # an empty image
    mask[2, -1, -1] = mask[2, 0, 0] = 1
    centre, scale = np.array([1.5, -2.25, 0.125], np.float32), np.array([45.0, 61.5, 16.25], np.float32)
    for stride in (1, 2, 3):
        want = REF.corr_from_nocs_ref(nocs, mask, centre, scale, stride)
        for m in (cu(mask, torch.uint8), cu(mask * 0.5), cu(mask, torch.uint8).bool()):
            got = ops.corr_from_nocs(cu(nocs), m, centre, scale, stride=stride)
            n = host(got["count"])
            assert got["xy"].shape == want[0].shape and np.array_equal(n, want[2]), (stride, n, want[2])
            for b in range(B):
                assert np.array_equal(host(got["xy"])[b, :n[b]], want[0][b, :n[b]]), (stride, b)
                assert np.array_equal(host(got["xyz"])[b, :n[b]], want[1][b, :n[b]]), (stride, b)
        assert want[2][1] == 0 and want[2][0] > 0.4 * want[0].shape[1]
    full = ops.corr_from_nocs(cu(np.full((1, H, W, 3), 0.25, np.float32)), torch.ones(1, H, W, device=DEV), centre, scale)          # every pixel: the list is full
    assert int(full["count"][0]) == H * W and np.array_equal(host(full["xy"])[0, -1], [W - 0.5, H - 0.5])


# ----------------------------------------------------------------------------- score: exact logic
@functools.lru_cache(maxsize=None)
def exact_case(B, N, T):
    """K = I, points at z = 1 whose offsets from their pixel are multiples of (3, 4) / 16, poses that shift by such multiples:
    every error is a multiple of 5 / 16 and tau = 5 / 16, so many entries sit exactly ON the bound; plus z <= 0, NaN and Inf."""
    rs = np.random.RandomState(B * 7919 + N * 31 + T)
    k = rs.randint(-2, 3, (B, N)).astype(np.float32)
    uv = rs.randint(-8, 9, (B, N, 2)).astype(np.float32) / 4
    xyz = np.concatenate([uv + k[..., None] * np.array([3, 4], np.float32) / 16, np.ones((B, N, 1), np.float32)], -1)
    kind = rs.randint(0, 12, (B, N))
    xyz[kind == 0, 2] = 0.0
    xyz[kind == 1, 2] = -1.0
    xyz[kind == 2, 0] = np.nan
    uv[kind == 3, 1] = np.nan
    uv[kind == 4, 0] = np.inf
    poses = np.tile(np.eye(3, 4, dtype=np.float32).reshape(12), (B, T, 1))
    m = rs.randint(-2, 3, (B, T)).astype(np.float32)
    m[:, 0] = 0
    poses[:, :, 3], poses[:, :, 7] = 3 * m / 16, 4 * m / 16
    valid = (rs.uniform(size=(B, T)) < 0.9).astype(np.uint8)
    K = np.tile(np.eye(3, dtype=np.float32), (B, 1, 1))
    count = counts_for(B, N)
    want, _ = REF.score_ref(uv, xyz, count, K, poses, 5 / 16, valid)
    for a in (uv, xyz, poses, valid, K, count, want):
        a.setflags(write=False)
    return uv, xyz, count, K, poses, valid, want


@pytest.mark.parametrize("N", SIZES_N)
def test_score_exact_counts_on_the_bound(N):
    from texpose_amd import ops
    on_bound = 0
    for B in (1, 3):
        for T in SIZES_T:
            uv, xyz, count, K, poses, valid, want = exact_case(B, N, T)
            got = ops.pnp_score(cu(uv), cu(xyz), cu(count, torch.int32), cu(K), cu(poses), tau_px=5 / 16, valid=cu(valid, torch.uint8))
            assert got.dtype == torch.int32 and np.array_equal(host(got), want), (B, N, T)
            strict, _ = REF.score_ref(uv, xyz, count, K, poses, 5 / 16 * (1 - 1e-6), valid)
            on_bound += int((want - strict).sum())
    if N >= 63:                                                 # the case does sit on `<=`, and is not empty
        assert on_bound > 100 and want.sum() > 100


def test_score_inlier_mask_and_no_valid_pointer():
    from texpose_amd import ops
    uv, xyz, count, K, poses, valid, _ = exact_case(3, 1025, 65)
    want, _, masks = REF.score_ref(uv, xyz, count, K, poses, 5 / 16, None, want_mask=True)
    sel = np.array([7, 0, 64], np.int32)
    inl, mask = ops.pnp_score(cu(uv), cu(xyz), cu(count, torch.int32), cu(K), cu(poses).view(3, 65, 3, 4), tau_px=5 / 16, sel=cu(sel, torch.int32),
                              inlier_mask=torch.full((3, 1025), 9, device=DEV, dtype=torch.uint8))
    assert np.array_equal(host(inl), want)
    assert np.array_equal(host(mask), np.stack([masks[b, sel[b]] for b in range(3)]).astype(np.uint8))
    _, none = ops.pnp_score(cu(uv), cu(xyz), cu(count, torch.int32), cu(K), cu(poses), tau_px=5 / 16, sel=cu([-1, 65, 99], torch.int32))
    assert int(none.sum()) == 0


# ----------------------------------------------------------------------------- realistic data
@functools.lru_cache(maxsize=None)
def real_case(B, N, T, noise=0.5, outliers=0.3, seed=0):
    """N model points in a 120 mm box seen from about 900 mm with the LineMOD intrinsics: `noise` px of Gaussian noise, a share
    `outliers` of the pixels replaced by uniform ones; T poses a fraction of a degree and a millimetre from the truth."""
    rs = np.random.RandomState(seed * 1009 + B * 101 + N + T)
    X = rs.uniform(-60, 60, (B, N, 3)).astype(np.float32)
    P = np.stack([np.concatenate([rotation(rs), rs.uniform(-80, 80, (3, 1)) + [[0.0], [0.0], [900.0]]], 1) for _ in range(B)])
    clean = np.stack([project(X[b], P[b], LINEMOD_K) for b in range(B)])
    xy = clean + rs.normal(0, noise, clean.shape)
    out = rs.uniform(size=(B, N)) < outliers
    xy[out] = rs.uniform(0, (640, 480), (int(out.sum()), 2))
    poses = np.tile(P[:, None], (1, T, 1, 1))
    for b in range(B):
        for h in range(1, T):
            poses[b, h, :, :3] = REF._exp_so3(rs.normal(size=3) * 2e-3) @ P[b, :, :3]
            poses[b, h, :, 3] += rs.normal(0, 0.5, 3)
    res = dict(xy=xy.astype(np.float32), xyz=X, K=np.tile(LINEMOD_K, (B, 1, 1)), P=P, poses=poses.reshape(B, T, 12).astype(np.float32),
               clean=clean.astype(np.float32), outlier=out)
    for a in res.values():
        a.setflags(write=False)
    return res


def test_score_realistic_within_the_near_ties():
    from texpose_amd import ops, pnp
    B, N, T = 3, 2049, 65                                       # (n >= 1000 everywhere: one near-tie is within 0.1 %)
    c = real_case(B, N, T)
    count = np.array([N, 1500, 1025], np.int32)
    want, ties = REF.score_ref(c["xy"], c["xyz"], count, c["K"], c["poses"], 2.0)
    got = host(ops.pnp_score(cu(c["xy"]), cu(c["xyz"]), cu(count, torch.int32), cu(c["K"]), cu(c["poses"]), tau_px=2.0))
    diff = np.abs(got.astype(np.int64) - want).max(1)
    print("score realistic: n %s  inliers of the true pose %s  near-ties %s  max count diff %s" % (count.tolist(), want[:, 0].tolist(), ties.tolist(), diff.tolist()))
    assert (ties <= TIE_CAP * count).all(), "the case has too many near-ties to decide anything: %s of %s" % (ties, count)
    assert (diff <= ties).all(), (got, want)
    assert (want[:, 0] > 0.6 * count).all() and (want[:, 0] < 0.75 * count).all()          # ~70 % inliers at the truth
    same = host(pnp.score_torch(cu(c["xy"]), cu(c["xyz"]), cu(count, torch.int32), cu(c["K"]), cu(c["poses"]), 2.0))
    assert (np.abs(same.astype(np.int64) - want).max(1) <= ties).all()


# ----------------------------------------------------------------------------- hypotheses
@pytest.mark.parametrize("N", SIZES_N)
def test_sample_idx_equals_the_restatement(N):
    from texpose_amd import ops
    for B in (1, 3):
        c = real_case(B, N, 4)
        count = counts_for(B, N)
        for T in SIZES_T:
            got = ops.pnp_hypotheses(cu(c["xy"]), cu(c["xyz"]), cu(count, torch.int32), cu(c["K"]), T=T, seed=5 + (T << 33))
            want = np.stack([REF.sample_indices(5 + (T << 33), b, T, int(count[b])) for b in range(B)])
            idx = host(got["sample_idx"])
            assert idx.dtype == np.int32 and np.array_equal(idx, want), (B, N, T)
            assert not host(got["hyp_valid"])[count < 4].any() and not host(got["hyp"])[count < 4].any()
    other = host(ops.pnp_hypotheses(cu(c["xy"]), cu(c["xyz"]), cu(count, torch.int32), cu(c["K"]), T=T, seed=6)["sample_idx"])
    assert not np.array_equal(other[0], idx[0])                  # a different seed: different samples


def check_valid_hypotheses(c, count, hy):
    """R orthonormal with determinant +1 to 1e-5, three positive depths, the three points reprojected within 1e-2 px."""
    idx, hyp, valid = host(hy["sample_idx"]), host(hy["hyp"]).astype(np.float64), host(hy["hyp_valid"])
    n_valid, worst = 0, 0.0
    for b in range(len(count)):
        for h in np.nonzero(valid[b])[0]:
            P = hyp[b, h].reshape(3, 4)
            assert np.abs(P[:, :3] @ P[:, :3].T - np.eye(3)).max() <= 1e-5 and abs(np.linalg.det(P[:, :3]) - 1) <= 1e-5, (b, h)
            i3 = idx[b, h, :3]
            x = c["xyz"][b, i3].astype(np.float64) @ P[:, :3].T + P[:, 3]
            assert (x[:, 2] > 0).all(), (b, h)
            e = np.abs(project(c["xyz"][b, i3], P, LINEMOD_K) - c["xy"][b, i3]).max()
            worst = max(worst, e)
            assert e <= 1e-2, (b, h, e)
            n_valid += 1
    return n_valid, worst


def test_hypotheses_on_noisy_data_are_rigid_and_fit_their_sample():
    from texpose_amd import ops
    B, N, T = 3, 257, 300
    c = real_case(B, N, T)
    count = np.array([N, 200, 4], np.int32)
    hy = ops.pnp_hypotheses(cu(c["xy"]), cu(c["xyz"]), cu(count, torch.int32), cu(c["K"]), T=T, seed=3)
    n_valid, worst = check_valid_hypotheses(c, count, hy)
    ref = REF.hypotheses_ref(c["xy"], c["xyz"], count, c["K"], T, 3)
    agree = (host(hy["hyp_valid"]).astype(bool) == ref["valid"])[~ref["ill"]]
    print("hypotheses noisy: %d of %d valid, worst reprojection of a sample %.3e px, validity agrees on %d of %d well-conditioned" % (
        n_valid, B * T, worst, int(agree.sum()), agree.size))
    assert n_valid > 0.5 * B * T and agree.all()


def test_hypotheses_on_noise_free_data_return_the_true_pose():
    from texpose_amd import ops
    B, N, T = 3, 257, 300
    c = real_case(B, N, T, noise=0.0, outliers=0.0, seed=1)
    count = np.array([N, N - 57, 65], np.int32)
    hy = ops.pnp_hypotheses(cu(c["clean"]), cu(c["xyz"]), cu(count, torch.int32), cu(c["K"]), T=T, seed=9)
    ref = REF.hypotheses_ref(c["clean"], c["xyz"], count, c["K"], T, 9)
    good = ~ref["ill"]
    assert np.array_equal(host(hy["sample_idx"]), ref["sample_idx"])
    assert ref["ill"].mean() <= 0.05, "the case has too many ill-conditioned samples: %.3f" % ref["ill"].mean()
    assert ref["valid"][good].all() and host(hy["hyp_valid"]).astype(bool)[good].all()
    got = host(hy["hyp"]).astype(np.float64).reshape(B, T, 3, 4)
    dR = np.abs(got[..., :3] - ref["hyp"][..., :3]).max((2, 3))[good]
    truth = np.array([[REF.pose_error(ref["hyp"][b, h], c["P"][b]) for h in range(T)] for b in range(B)])[good]
    mine = np.array([[REF.pose_error(got[b, h], c["P"][b]) for h in range(T)] for b in range(B)])[good]
    bound = 4 * truth.max(0)
    print("hypotheses noise-free: flagged %.4f; against the truth: restatement %.3e deg %.3e mm, device %.3e deg %.3e mm (bound: 4 x the restatement's = %.3e deg "
          "%.3e mm); device against restatement: largest difference of an R entry %.3e" % (ref["ill"].mean(), truth[:, 0].max(), truth[:, 1].max(), mine[:, 0].max(),
                                                                                             mine[:, 1].max(), bound[0], bound[1], dR.max()))
    assert (mine[:, 0] <= bound[0]).all() and (mine[:, 1] <= bound[1]).all()
    check_valid_hypotheses(dict(c, xy=c["clean"]), count, hy)


# ----------------------------------------------------------------------------- refine
@functools.lru_cache(maxsize=None)
def refine_case(N):
    """0.3 px noise, a quarter of the entries at least 20 px off, a start 2 degrees and 5 mm from the truth."""
    B = 3
    c = real_case(B, N, 1, noise=0.3, outliers=0.0, seed=2)
    rs = np.random.RandomState(N)
    xy = c["xy"].copy()
    out = rs.uniform(size=(B, N)) < 0.25
    ang = rs.uniform(0, 2 * np.pi, int(out.sum()))
    xy[out] = c["clean"][out] + (rs.uniform(20, 200, int(out.sum()))[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
    start = np.zeros((B, 3, 4))
    for b in range(B):
        w, d = rs.normal(size=3), rs.normal(size=3)
        start[b, :, :3] = REF._exp_so3(w * np.radians(2.0) / np.linalg.norm(w)) @ c["P"][b, :, :3]
        start[b, :, 3] = c["P"][b, :, 3] + d * 5.0 / np.linalg.norm(d)
    return dict(xy=xy, xyz=c["xyz"], K=c["K"], P=c["P"], start=start.astype(np.float32), count=np.array([N, N // 2, max(30, N // 5)], np.int32))


@pytest.mark.parametrize("N", [65, 257, 1025, 2600])
def test_refine_equals_the_restatement(N):
    from texpose_amd import ops
    c = refine_case(N)
    B = 3
    for iters in (0, 1, 5):
        got = ops.pnp_refine(cu(c["xy"]), cu(c["xyz"]), cu(c["count"], torch.int32), cu(c["K"]), cu(c["start"]), tau_px=4.0, iters=iters)
        pose, inl, rms, status = host(got["pose"]).astype(np.float64), host(got["inliers"]), host(got["rms"]), host(got["status"])
        for b in range(B):
            want = REF.refine_ref(c["xy"][b], c["xyz"][b], int(c["count"][b]), c["K"][b], c["start"][b], 4.0, iters)
            assert want["near_ties"] == 0, "the case has a near-tie: it decides nothing"
            assert status[b] == want["status"] and inl[b] == want["inliers"], (N, iters, b, status[b], want["status"], inl[b], want["inliers"])
            dR = np.abs(pose[b, :, :3] - want["pose"][:, :3]).max()
            dt = np.linalg.norm(pose[b, :, 3] - want["pose"][:, 3]) / np.linalg.norm(want["pose"][:, 3])
            assert dR <= 1e-5 and dt <= 1e-5, (N, iters, b, dR, dt)
            assert abs(rms[b] - want["rms"]) <= 1e-5 * want["rms"]
            if iters == 0:
                assert np.array_equal(host(got["pose"])[b], c["start"][b])
            if iters == 5 and c["count"][b] >= 50:
                re, te = REF.pose_error(pose[b], c["P"][b])
                assert re < 2.0 and te < 5.0 and inl[b] > 0.5 * c["count"][b], (re, te)          # (closer than the start; a quarter are outliers)


def test_refine_rank_deficient_system_keeps_the_start():
    from texpose_amd import ops
    c = refine_case(257)
    xy, xyz = np.tile(c["xy"][:, :1], (1, 257, 1)), np.tile(c["xyz"][:, :1], (1, 257, 1))          # all points equal
    got = ops.pnp_refine(cu(xy), cu(xyz), cu(c["count"], torch.int32), cu(c["K"]), cu(c["P"]), tau_px=4.0)
    assert host(got["status"]).tolist() == [3, 3, 3]
    assert np.array_equal(host(got["pose"]), c["P"].astype(np.float32))
    for b in range(3):
        want = REF.refine_ref(xy[b], xyz[b], int(c["count"][b]), c["K"][b], c["P"][b], 4.0, 5)
        assert want["status"] == 3 and int(got["inliers"][b]) == want["inliers"]


# ----------------------------------------------------------------------------- end to end on the rasteriser
@functools.lru_cache(maxsize=None)
def rendered_case(mesh):
    from texpose_amd import ops
    from texpose_amd.surfel import nocs_normalisation
    c = REF.end_to_end_inputs(mesh)
    norm = nocs_normalisation(c["verts"])
    r = ops.mesh_raster(cu(c["verts"]), cu(c["faces"], torch.int32), cu(c["P"]), cu(c["K"]), H=c["H"], W=c["W"], nocs_norm=norm, face_ids=False, normals=False)
    return dict(c, norm=norm, nocs=r["nocs"].clone(), mask=(r["zbuf"] > 0))


@pytest.mark.parametrize("mesh", ["torus", "sphere"])
@pytest.mark.parametrize("dirty", [False, True])
def test_end_to_end_on_rendered_nocs(mesh, dirty):
    from texpose_amd import ops
    c = rendered_case(mesh)
    B = 2
    nocs = c["nocs"].clone()
    kept = host(c["mask"])
    touched = np.zeros_like(kept)
    if dirty:                                                   # 30 % of the kept NOCS values replaced by uniform random ones
        touched, values = REF.end_to_end_corruption(kept)
        nocs[cu(touched, torch.bool)] = cu(values)
    corr = ops.corr_from_nocs(nocs, c["mask"], *c["norm"])
    count = host(corr["count"])
    assert np.array_equal(count, kept.sum((1, 2)))
    Kb = np.tile(c["K"], (B, 1, 1))
    got = ops.pnp_ransac(corr["xy"], corr["xyz"], corr["count"], cu(Kb), T=256, tau_px=2.0, iters=5, seed=1)
    want = REF.ransac_ref(host(corr["xy"]), host(corr["xyz"]), count, Kb, T=256, tau=2.0, iters=5, seed=1)
    untouched = (kept & ~touched).sum((1, 2))
    assert (host(got["status"]) == 0).all() and (want["status"] == 0).all()
    for b in range(B):
        re, te = REF.pose_error(host(got["pose"])[b], c["P"][b])
        re_w, te_w = REF.pose_error(want["pose32"][b], c["P"][b])
        print("end to end %s %s b=%d: n %d untouched %d inliers %d (restatement %d); error against the truth %.4e deg %.4e mm (restatement %.4e deg %.4e mm)"
              % (mesh, "dirty" if dirty else "clean", b, count[b], untouched[b], int(got["inliers"][b]), want["inliers"][b], re, te, re_w, te_w))
        assert int(got["inliers"][b]) >= 0.95 * untouched[b]
        ulp_t = float(np.spacing(np.float32(np.abs(c["P"][b][:, 3]).max())))          # both poses are fp32 stores: a last bit of t is no error
        assert re <= 2 * re_w and te <= max(2 * te_w, ulp_t), (re, re_w, te, te_w, ulp_t)


# ----------------------------------------------------------------------------- degenerate inputs
def test_degenerate_inputs():
    from texpose_amd import ops
    B, N, T = 3, 257, 65
    c = real_case(B, N, T)
    args = lambda xy, xyz, count: (cu(xy), cu(xyz), cu(count, torch.int32), cu(c["K"]))
    r = ops.pnp_ransac(*args(c["xy"], c["xyz"], np.array([0, 3, N], np.int32)), T=T)
    assert host(r["status"]).tolist() == [1, 1, 0] and host(r["inliers"])[:2].tolist() == [0, 0]
    assert np.isnan(host(r["pose"])[:2]).all() and np.isnan(host(r["rms"])[:2]).all() and np.isfinite(host(r["pose"])[2]).all()
    r = ops.pnp_ransac(*args(c["xy"], c["xyz"], np.array([-5, 3, N + 1000], np.int32)), T=T)          # out of range: clamped, nothing read past N
    assert host(r["status"]).tolist() == [1, 1, 0]
    nan = np.full_like(c["xyz"], np.nan)
    r = ops.pnp_ransac(*args(c["xy"], nan, np.array([N, N, N], np.int32)), T=T)
    assert host(r["status"]).tolist() == [2, 2, 2] and not host(r["hyp_valid"]).any() and np.isnan(host(r["pose"])).all() and not host(r["inliers"]).any()
    # poses and points at 1e30 and Inf: finite counts, equal to the restatement's
    xy, xyz, poses = c["xy"].copy(), c["xyz"].copy(), c["poses"].copy()
    xyz[:, 0::7] = 1e30
    xyz[:, 1::7, 2] = np.inf
    xy[:, 2::7, 0] = -np.inf
    poses[:, 1::5] = 1e30
    poses[:, 2::5, 11] = np.inf
    poses[:, 3::5, 0] = np.nan
    poses[:, 4::5] *= 1e30
    count = np.array([N, N, N], np.int32)
    want, _ = REF.score_ref(xy, xyz, count, c["K"], poses, 2.0)
    got = host(ops.pnp_score(*args(xy, xyz, count), cu(poses), tau_px=2.0))
    assert np.array_equal(got, want) and want[:, 0].min() > 50 and (want[:, 1:4] == 0).all()          # (a pose times 1e30 projects as before)
    huge = ops.pnp_ransac(*args(xy, xyz, count), T=T)            # the whole chain on the same lists: it terminates with a status
    assert set(host(huge["status"]).tolist()) <= {0, 2, 3} and (host(huge["inliers"]) >= 0).all()


def test_bad_arguments_are_refused():
    from texpose_amd import _lib, ops
    c = real_case(1, 65, 4)
    a = (cu(c["xy"]), cu(c["xyz"]), cu([65], torch.int32), cu(c["K"]))
    for T in (0, 4097):
        with pytest.raises(_lib.TexposeLibraryError, match="bad sizes"):
            ops.pnp_hypotheses(*a, T=T)
    for tau in (0.0, float("nan"), float("inf")):
        with pytest.raises(_lib.TexposeLibraryError, match="tau_px"):
            ops.pnp_score(*a, cu(c["poses"]), tau_px=tau)
    for iters in (-1, 33):
        with pytest.raises(_lib.TexposeLibraryError, match="iters"):
            ops.pnp_refine(*a, cu(c["P"]), iters=iters)
    with pytest.raises(ValueError):
        ops.pnp_score(a[0], a[1][:, :10], a[2], a[3], cu(c["poses"]))
    with pytest.raises(ValueError):
        ops.pnp_score(a[0], a[1], a[2].long(), a[3], cu(c["poses"]))
    with pytest.raises(ValueError):
        ops.pnp_refine(*a, cu(c["poses"]))                       # several hypotheses and no counts to pick by
    with pytest.raises(ValueError):
        ops.pnp_refine(*a, cu(c["P"]), workspace=torch.empty(4, device=DEV))
    with pytest.raises(ValueError):
        ops.corr_from_nocs(torch.zeros(1, 4, 4, 3, device=DEV), torch.ones(1, 4, 4, device=DEV), [0, 0, 0], [1, 1, 1], stride=0)


# ----------------------------------------------------------------------------- reproducibility
def test_two_runs_and_graph_replay_are_bit_equal():
    from texpose_amd import ops
    B, N, T = 3, 1025, 65
    c = real_case(B, N, T)
    a = (cu(c["xy"]), cu(c["xyz"]), cu([N, N - 300, 700], torch.int32), cu(c["K"]))
    first = ops.pnp_ransac(*a, T=T, seed=4)
    again = ops.pnp_ransac(*a, T=T, seed=4)
    for k in ops.PNP_RANSAC_KEYS:
        assert torch.equal(first[k].view(torch.uint8), again[k].view(torch.uint8)), k
    assert (first["status"] == 0).all() and (first["inliers"] > 300).all()
    assert not torch.equal(ops.pnp_ransac(*a, T=T, seed=5)["sample_idx"], first["sample_idx"])
    spec = {k: torch.empty_like(v) for k, v in first.items()}
    ws = ops.pnp_workspace(B, N, T, DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.pnp_ransac(*a, T=T, seed=4, workspace=ws, out=spec)
    for _ in range(2):
        for v in spec.values():
            v.view(torch.uint8).fill_(0xAB)
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k in ops.PNP_RANSAC_KEYS:
            assert torch.equal(spec[k].view(torch.uint8), first[k].view(torch.uint8)), k


def test_solver_module_matches_the_ops():
    from texpose_amd import ops, pnp
    c = rendered_case("torus")
    solver = pnp.PnPSolver(c["H"], c["W"], DEV, T=64, seed=2)
    r = solver.solve_nocs(c["nocs"].permute(0, 3, 1, 2), c["mask"], cu(c["K"]), *c["norm"], stride=2)
    corr = ops.corr_from_nocs(c["nocs"], c["mask"], *c["norm"], stride=2)
    want = ops.pnp_ransac(corr["xy"], corr["xyz"], corr["count"], cu(c["K"]), T=64, seed=2)
    assert torch.equal(r.pose, want["pose"]) and torch.equal(r.inliers, want["inliers"]) and torch.equal(r.n, corr["count"])
    assert torch.equal(r.score, want["inliers"].float() / corr["count"].float()) and (r.score > 0.95).all() and (r.status == 0).all()
    again = solver.solve(corr["xy"], corr["xyz"], corr["count"], cu(c["K"]))
    assert torch.equal(again.pose, want["pose"])


# ----------------------------------------------------------------------------- the tool
def _write_ply(path, verts, faces):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces)))
        for p in verts:
            f.write("%r %r %r\n" % tuple(float(v) for v in p))
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(int(v) for v in t))


def test_tool_writes_poses_that_pose_errors_reads(tmp_path):
    from PIL import Image
    from texpose_amd import ops
    from texpose_amd.surfel import SurfelRenderer, nocs_normalisation, write_surfel_frame
    H, W, F, oid = 120, 160, 3, 7
    verts, faces = torus(40, 20)
    K = K_for(H, W)
    rs = np.random.RandomState(8)
    P = np.stack([np.concatenate([rotation(rs), rs.uniform(-15, 15, (3, 1)) + [[0.0], [0.0], [900.0]]], 1) for _ in range(F)]).astype(np.float32)
    ply, root, out = str(tmp_path / "obj_000007.ply"), str(tmp_path / "scene"), str(tmp_path / "poses.csv")
    _write_ply(ply, verts, faces)
    maps = SurfelRenderer(verts, faces, None, H, W, DEV)(cu(P), cu(K), 1000.0)          # depth scale 1000: t already in mm
    for f in range(F):
        write_surfel_frame(root, 0, 10 + f, maps, f)
    with open(os.path.join(root, "scene_camera.json"), "w") as fh:
        json.dump({str(10 + f): {"cam_K": [float(v) for v in K.reshape(-1)], "depth_scale": 1.0} for f in range(F)}, fh)
    run = subprocess.run([sys.executable, os.path.join(REPO, "tools", "pnp_poses.py"), "--scene", root, "--loop", "0", "--ply", "%d=%s" % (oid, ply),
                          "--out", out, "--device", DEV], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    spec = importlib.util.spec_from_file_location("pose_errors_tool", os.path.join(REPO, "tools", "pose_errors.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    est = tool.read_estimates_csv(out)
    assert sorted(est) == [10, 11, 12]
    diameter = float(np.linalg.norm(verts[:, None] - verts[None], axis=-1).max())
    # the same quantised lists through the restatement: the bar is 1 % of the diameter if that stays within it with room to spare
    nocs8 = np.stack([np.asarray(Image.open(os.path.join(root, "nocs_0", "%06d.png" % (10 + f)))) for f in range(F)])
    corr = ops.corr_from_nocs(cu(nocs8.astype(np.float32)) / 255.0, maps.depth > 0, *nocs_normalisation(verts))
    want = REF.ransac_ref(host(corr["xy"]), host(corr["xyz"]), host(corr["count"]), np.tile(K, (F, 1, 1)), T=256, tau=2.0, iters=5, seed=0)
    for f in range(F):
        (R, t), = est[10 + f][oid]
        add = np.linalg.norm((verts @ R.T + t) - (verts.astype(np.float64) @ P[f, :, :3].T + P[f, :, 3]), axis=1).mean()
        add_w = np.linalg.norm((verts @ want["pose32"][f, :, :3].T.astype(np.float64) + want["pose32"][f, :, 3]) - (verts.astype(np.float64) @ P[f, :, :3].T + P[f, :, 3]), axis=1).mean()
        print("tool frame %d: ADD %.4f mm = %.4f %% of the diameter %.2f mm (restatement on the same lists: %.4f mm)" % (10 + f, add, 100 * add / diameter, diameter, add_w))
        assert add_w < 0.5 * 0.01 * diameter, "the restatement itself has no room to spare under 1 % of the diameter: %.4f mm" % add_w
        assert add < 0.01 * diameter
