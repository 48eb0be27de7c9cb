"""GPU: the search kernel K24 (tp_nn1), the fused reductions K25 (tp_pose_errors) and the functions of texpose_amd/pose_error.py
built on them, against the numpy fp64 restatement tests/pose_error_ref.py.

Exact cases: integer lattices (|coordinate| <= 512), so every d2 is exact in fp32 whatever the contraction, with heavy ties; d2 and idx
must equal the helper's.  Random cases follow the fp32-grade rule of DESIGN section 2 as section 14 applies it:
    e_k <= 2 e_t + floor
with e_k the kernel's largest absolute error against the helper, e_t that of the plain torch fp32 chain on the same device and floor
one fp32 ulp of the largest magnitude compared.  An index may differ from the helper's only where the helper's best and second-best
fp64 values differ by less than 1e-5 relative; such entries are counted, printed, and may be at most 1 % of a case."""
import functools
import math

import numpy as np
import pytest
import torch

import pose_error_ref as R
from test_gpu_surfel import torus, uv_sphere

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
T, QB = 1024, 1024          # the target tile and the queries per workgroup of the kernel (checked against the header below)
NEAR_TIE, TIE_SHARE = 1e-5, 0.01


def cu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def host(t):
    return t.detach().cpu().numpy()


def run_nn1(x, y, x_len=None, y_len=None, A=None, mode="nearest", target_slices=0):
    from texpose_amd import ops
    i32 = lambda v: None if v is None else cu(v, torch.int32)
    d2, idx = ops.nn1(cu(x), cu(y), x_len=i32(x_len), y_len=i32(y_len), A=None if A is None else cu(A), mode=mode, target_slices=target_slices)
    return host(d2), host(idx)


def within_rule(name, got, want, torch32):
    got, want, torch32 = (np.asarray(v, dtype=np.float64) for v in (got, want, torch32))
    assert got.shape == want.shape == torch32.shape, (name, got.shape, want.shape, torch32.shape)
    assert np.isfinite(want).all() and np.isfinite(got).all(), name
    e_k, e_t = float(np.abs(got - want).max()), float(np.abs(torch32 - want).max())
    floor = float(np.spacing(np.float32(np.abs(want).max())))
    print("%-44s e_k %.3e  e_t %.3e  e_k / e_t %s  floor %.3e" % (name, e_k, e_t, "%.3f" % (e_k / e_t) if e_t > 0 else "-", floor))
    assert e_k <= 2 * e_t + floor, (name, e_k, e_t, floor)


def test_constants_are_the_header_s():
    from texpose_amd import _lib
    assert (_lib.NN1_TILE, _lib.NN1_QUERIES_PER_BLOCK) == (T, QB)


# ----------------------------------------------------------------------------- K24, exact
def lattice_maps(rs, B):
    """Signed axis permutations with integer translations: a lattice stays a lattice."""
    A = np.zeros((B, 3, 4), np.float32)
    for b in range(B):
        A[b, np.arange(3), rs.permutation(3)] = rs.choice([-1.0, 1.0], 3)
        A[b, :, 3] = rs.randint(-400, 401, 3)
    return A


@functools.lru_cache(maxsize=None)
def exact_case(B, P1, P2):
    """Lattice clouds in [-4, 4]^3 (at most 729 distinct points: duplicates and equidistant targets everywhere), ragged lengths that
    include 0, NaN queries and NaN targets; built once, read-only."""
    rs = np.random.RandomState(100000 * B + 100 * P1 + P2)
    x = rs.randint(-4, 5, (B, P1, 3)).astype(np.float32)
    y = rs.randint(-4, 5, (B, P2, 3)).astype(np.float32)
    y[:, P2 // 2:] = y[:, :P2 - P2 // 2]                   # the second half repeats the first: every winner has a twin
    if P1 > 3:
        x[0, 1] = np.nan
    if P2 > 3:
        y[B - 1, 2, 1] = np.nan
        y[0, 0] = np.nan                                   # (the twin at P2 // 2 remains)
    x_len = rs.randint(0, P1 + 1, B).astype(np.int32)
    y_len = rs.randint(0, P2 + 1, B).astype(np.int32)
    if B > 1:                                              # one full element, one without queries, one without targets
        x_len[0], y_len[0] = P1, P2
        x_len[1], y_len[B - 1] = 0, 0
    A = lattice_maps(rs, B)
    for v in (x, y, x_len, y_len, A):
        v.setflags(write=False)
    return x, y, x_len, y_len, A


@pytest.mark.parametrize("P2", [1, 63, 65, T - 1, T, T + 1, 2 * T + 3])
@pytest.mark.parametrize("P1", [1, 63, 64, 65, QB - 1, QB + 1])
@pytest.mark.parametrize("B", [1, 3])
def test_nn1_exact_on_lattices(B, P1, P2):
    x, y, x_len, y_len, A = exact_case(B, P1, P2)
    for mode in ("nearest", "farthest"):
        for shared in ((True, False) if B > 1 else (True,)):          # Bt = 1 / Bt = B (the same thing at B = 1)
            yy, yl = (y[:1], y_len[:1]) if shared else (y, y_len)
            for with_A in (False, True):
                AA = A if with_A else None
                yt = yy + A[:1, None, :, 3] if with_A and shared else (yy + A[:, None, :, 3] if with_A else yy)      # targets near the mapped queries
                for ragged in (False, True):
                    kw = dict(x_len=x_len, y_len=yl) if ragged else {}
                    want_d2, want_idx = R.nn1(x, yt, A=AA, mode=mode, **kw)
                    for slices in ((0, 1, 2) if P2 > T else (0,)):          # chosen by the library / one slice over several tiles / forced split
                        d2, idx = run_nn1(x, yt, A=AA, mode=mode, target_slices=slices, **kw)
                        tag = (mode, shared, with_A, ragged, slices)
                        assert idx.dtype == np.int32 and d2.dtype == np.float32 and d2.shape == idx.shape == (B, P1), tag
                        assert np.array_equal(idx, want_idx), tag
                        assert np.array_equal(d2, want_d2.astype(np.float32)), tag          # (+-inf where there is no winner; integers: exact)


def test_nn1_no_winner_values_and_shared_queries():
    x, y, x_len, y_len, A = exact_case(3, 65, 65)
    d2, idx = run_nn1(x, y, x_len=x_len, y_len=y_len)
    assert (idx[1] == -1).all() and np.isposinf(d2[1]).all() and idx[0, 1] == -1 and np.isposinf(d2[0, 1])      # x_len 0; a NaN query
    assert (idx[2] == -1).all()                                                                                 # y_len 0
    d2, idx = run_nn1(x, y, x_len=x_len, y_len=y_len, mode="farthest")
    assert (idx[1] == -1).all() and np.isneginf(d2[1]).all() and (idx[0, [0, 2]] >= 0).all()
    # one query set under B maps (what adds does): equal to the queries repeated
    want = run_nn1(np.repeat(x[:1], 3, 0), y[:1] + 0, A=A)
    got = run_nn1(x[:1], y[:1], A=A)
    assert got[0].shape == (3, 65) and np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


def test_ops_reject_bad_arguments():
    from texpose_amd import _lib, ops
    x, y = torch.zeros(2, 5, 3, device=DEV), torch.zeros(2, 7, 3, device=DEV)
    with pytest.raises(ValueError):
        ops.nn1(x, y, mode="median")
    with pytest.raises(ValueError):
        ops.nn1(x, torch.zeros(3, 7, 3, device=DEV))
    with pytest.raises(ValueError):
        ops.nn1(x, y, x_len=torch.zeros(2, device=DEV))                       # (int32 expected)
    with pytest.raises(ValueError):
        ops.nn1(x, y, A=torch.zeros(2, 4, 4, device=DEV))
    with pytest.raises(ValueError):
        ops.pose_errors(torch.zeros(5, 2, device=DEV), torch.zeros(1, 3, 4, device=DEV), torch.zeros(1, 3, 4, device=DEV))
    with pytest.raises(_lib.TexposeLibraryError, match="at most 64"):        # S = 65: the library's error code
        ops.pose_errors(torch.zeros(5, 3, device=DEV), torch.zeros(1, 3, 4, device=DEV), torch.zeros(1, 3, 4, device=DEV),
                        torch.eye(3, 4, device=DEV).repeat(65, 1, 1))


# ----------------------------------------------------------------------------- K24, random
def rotation(rs):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] *= -1
    return q


def poses(rs, B, spread=60.0, z=1000.0):
    return np.stack([np.concatenate([rotation(rs), rs.uniform(-spread, spread, (3, 1)) + [[0.0], [0.0], [z]]], 1) for _ in range(B)]).astype(np.float32)


def nudged(rs, P, angle=0.05, shift=4.0):
    out = P.astype(np.float64)
    for b in range(len(P)):
        out[b, :, :3] = R.rotation(rs.normal(size=3), angle) @ out[b, :, :3]
        out[b, :, 3] += rs.uniform(-shift, shift, 3)
    return out.astype(np.float32)


def torch_chain_nn1(x, y, A, mode):
    """`(q[:, :, None] - y[:, None]).square().sum(-1).min(-1)` in fp32 on the device (max for 'farthest')."""
    q, yy = cu(x), cu(y)
    if A is not None:
        Ad = cu(A)
        q = q @ Ad[:, :, :3].transpose(1, 2) + Ad[:, None, :, 3]
    d = (q[:, :, None] - yy[:, None]).square().sum(-1)
    return host(d.max(-1).values if mode == "farthest" else d.min(-1).values)


def near_ties(best, second):
    """Where the helper's best and second-best fp64 values differ by less than NEAR_TIE relative."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(second - best) < NEAR_TIE * np.abs(best)


def check_indices(name, idx, want_idx, best, second):
    """idx may differ from the helper's only at near-ties of the helper's own fp64 values; those are counted and capped."""
    tie = near_ties(best, second)
    share = float(tie.mean())
    print("%-44s near-ties %d of %d (%.4f %%), indices differing %d" % (name, int(tie.sum()), tie.size, 100 * share, int((idx != want_idx).sum())))
    assert share <= TIE_SHARE, (name, share)
    assert np.array_equal(idx[~tie], want_idx[~tie]), name


@functools.lru_cache(maxsize=None)
def random_case(B, P1, P2, seed):
    """Uniform points in a 200 mm cube: the queries under B poses at ~1 m, the targets under nearby poses -- as posed fp32 clouds
    (no A) and as the model with the pose as A.  The helper's answers for every (mode, shared targets, with A) are computed once, here
    on the host, and its own share of near-ties is asserted to stay under the cap: a seed that fails this is a bad seed, whatever the
    kernel does."""
    rs = np.random.RandomState(seed)
    model_x = rs.uniform(-100, 100, (B, P1, 3)).astype(np.float32)
    model_y = rs.uniform(-100, 100, (B, P2, 3)).astype(np.float32)
    Pe = poses(rs, B)
    Pg = nudged(rs, Pe)
    posed_x = np.stack([R.apply(Pe[b], model_x[b]) for b in range(B)]).astype(np.float32)
    posed_y = np.stack([R.apply(Pg[b], model_y[b]) for b in range(B)]).astype(np.float32)
    want = {}
    for mode in ("nearest", "farthest"):
        for shared in (True, False):
            for with_A in (False, True):
                best, idx, second = R.nn1(model_x if with_A else posed_x, posed_y[:1] if shared else posed_y, A=Pe if with_A else None,
                                          mode=mode, second=True)
                share = float(near_ties(best, second).mean())
                assert share <= TIE_SHARE, ("the helper's own near-ties", seed, mode, shared, with_A, share)
                want[mode, shared, with_A] = (best, idx, second)
    for v in (model_x, posed_x, posed_y, Pe) + tuple(a for w in want.values() for a in w):
        v.setflags(write=False)
    return model_x, posed_x, posed_y, Pe, want


@pytest.mark.parametrize("B, P1, P2, seed", [(1, 65, T - 1, 1), (3, QB + 1, 2 * T + 3, 2)])
def test_nn1_random_meets_the_fp32_rule(B, P1, P2, seed):
    model_x, posed_x, posed_y, Pe, want = random_case(B, P1, P2, seed)
    for mode in ("nearest", "farthest"):
        for shared in (True, False):
            y = posed_y[:1] if shared else posed_y
            for x, A in ((posed_x, None), (model_x, Pe)):
                best, want_idx, second = want[mode, shared, A is not None]
                d2, idx = run_nn1(x, y, A=A, mode=mode)
                tag = "nn1 B%d P1 %d P2 %d %s Bt %d %s" % (B, P1, P2, mode, len(y), "A" if A is not None else "-")
                check_indices(tag, idx, want_idx, best, second)
                within_rule(tag, d2, best, torch_chain_nn1(x, y, A, mode))


# ----------------------------------------------------------------------------- K25
@functools.lru_cache(maxsize=None)
def pose_case(B, M, S):
    rs = np.random.RandomState(10000 * B + 10 * M + S)
    pts = rs.uniform(-100, 100, (M, 3)).astype(np.float32)
    Pg = poses(rs, B)
    Pe = nudged(rs, Pg)
    sym = np.stack([np.eye(3, 4)] + [np.concatenate([rotation(rs), rs.uniform(-3, 3, (3, 1))], 1) for _ in range(S - 1)]).astype(np.float32)
    K = np.tile(np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], np.float32), (B, 1, 1))
    K[:, 0, 2] += rs.uniform(-5, 5, B).astype(np.float32)
    want = R.pose_errors(pts, Pe, Pg, sym, K)
    for v in (pts, Pg, Pe, sym, K):
        v.setflags(write=False)
    return pts, Pe, Pg, sym, K, want


@pytest.mark.parametrize("with_intr", [False, True])
@pytest.mark.parametrize("S", [1, 2, 7, 64])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("B", [1, 5])
def test_pose_errors_meet_the_fp32_rule(B, M, S, with_intr):
    from texpose_amd import ops, pose_error as PE
    pts, Pe, Pg, sym, K, want = pose_case(B, M, S)
    Kd = cu(K) if with_intr else None
    got = ops.pose_errors(cu(pts), cu(Pe), cu(Pg), cu(sym), Kd)
    ref32 = PE.pose_errors_torch(cu(pts), cu(Pe), cu(Pg), cu(sym), Kd)          # the torch fp32 chain on the device
    keys = ("add", "mssd") + (("mspd", "proj") if with_intr else ())
    assert set(got) == set(keys) | {"s_mssd"} | ({"s_mspd"} if with_intr else set())
    tag = "B%d M%d S%d %s" % (B, M, S, "intr" if with_intr else "-")
    for k in keys:
        assert got[k].shape == (B,) and got[k].dtype == torch.float32
        within_rule("%s %s" % (k, tag), host(got[k]), want[k], host(ref32[k]))
    for k in ("s_mssd",) + (("s_mspd",) if with_intr else ()):
        per_sym = np.sort(want["per_sym_" + k[2:]], axis=1)
        second = per_sym[:, 1] if S > 1 else np.full(B, np.inf)
        assert got[k].dtype == torch.int32
        check_indices("%s %s" % (k, tag), host(got[k]), want[k], per_sym[:, 0], second)


def test_pose_errors_point_behind_the_camera():
    from texpose_amd import ops
    pts, Pe, Pg, sym, K, _ = pose_case(5, 257, 2)
    Pe = Pe.copy()
    Pe[3, 2, 3] = 20.0                                      # pose 3: the model straddles the camera plane
    want = R.pose_errors(pts, Pe, Pg, sym, K)
    got = {k: host(v) for k, v in ops.pose_errors(cu(pts), cu(Pe), cu(Pg), cu(sym), cu(K)).items()}
    assert np.isnan(want["mspd"][3]) and np.isnan(got["mspd"][3]) and np.isnan(got["proj"][3]) and got["s_mspd"][3] == -1
    ok = np.arange(5) != 3
    assert np.isfinite(got["add"]).all() and np.isfinite(got["mssd"]).all() and np.isfinite(got["mspd"][ok]).all() and np.isfinite(got["proj"][ok]).all()
    np.testing.assert_allclose(got["add"], want["add"], rtol=1e-6)
    assert np.array_equal(got["s_mssd"], want["s_mssd"]) and np.array_equal(got["s_mspd"][ok], want["s_mspd"][ok])


# ----------------------------------------------------------------------------- composed
@functools.lru_cache(maxsize=None)
def mesh_case(kind):
    rs = np.random.RandomState(7)
    pts = (uv_sphere(49, 100, ripple=0.1)[0] if kind == "sphere" else torus(100, 50)[0]).astype(np.float32)
    assert 4900 <= len(pts) <= 5100
    Pg = poses(rs, 2)
    Pe = nudged(rs, Pg)
    for v in (pts, Pg, Pe):
        v.setflags(write=False)
    return pts, Pe, Pg, R.adds(pts, Pe, Pg), R.model_diameter(pts)


@pytest.mark.parametrize("kind", ["sphere", "torus"])
def test_composed_functions_on_meshes(kind):
    from texpose_amd import pose_error as PE
    pts, Pe, Pg, want_adds, want_diameter = mesh_case(kind)
    p, e, g = cu(pts), cu(Pe), cu(Pg)
    A = PE.relative_pose(e, g).float()

    def torch32_adds():
        d2, _ = PE.nn1_torch(p[None], p[None], A=A)
        return d2.sqrt().mean(-1)

    adds = PE.adds(p, e, g)
    within_rule("adds " + kind, host(adds), want_adds, host(torch32_adds()))
    diameter = PE.model_diameter(p)
    within_rule("diameter " + kind, host(diameter), np.float64(want_diameter), host(PE.nn1_torch(p[None], p[None], mode="farthest")[0].max().sqrt()))
    # p2p_distance: the posed model against the model under the other poses, ragged, weighted
    x = torch.stack([p @ e[b, :, :3].T + e[b, :, 3] for b in range(2)])
    y = torch.stack([p @ g[b, :, :3].T + g[b, :, 3] for b in range(2)])
    xl, yl = torch.tensor([len(pts), 1500], device=DEV), torch.tensor([len(pts), 2500], device=DEV)
    w = torch.tensor([1.0, 0.5], device=DEV)
    want_d2, _ = R.nn1(host(x), host(y), host(xl), host(yl))          # (the search once, both reductions)
    for br, pr in (("mean", "mean"), (None, "sum")):
        got, none = PE.p2p_distance(x, y, xl, yl, weights=w, batch_reduction=br, point_reduction=pr)
        want = R.p2p_distance(host(x), host(y), host(xl), host(yl), host(w), br, pr, d2=want_d2)
        d2, _ = PE.nn1_torch(x, y, xl, yl)
        d2 = torch.where(torch.arange(len(pts), device=DEV)[None] < xl[:, None], d2, torch.zeros_like(d2)) * w[:, None]
        t32 = d2.sum(1) / (xl if pr == "mean" else 1)
        t32 = t32.sum() / w.sum() if br == "mean" else t32
        assert none is None
        within_rule("p2p_distance %s %s %s" % (kind, br, pr), host(got), np.asarray(want, dtype=np.float64), host(t32))
    # twice: bit-identical
    assert torch.equal(PE.adds(p, e, g), adds) and torch.equal(PE.model_diameter(p), diameter)
    first, second = (PE.p2p_distance(x, y, xl, yl, weights=w)[0] for _ in range(2))
    assert torch.equal(first, second)


def test_captured_call_replays_the_eager_result():
    from texpose_amd import ops, pose_error as PE
    pts, Pe, Pg, _, _ = mesh_case("torus")
    p, e, g = cu(pts), cu(Pe), cu(Pg)
    K = cu(np.tile(np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], np.float32), (2, 1, 1)))

    def both():
        r = ops.pose_errors(p, e, g, None, K)
        return (PE.adds(p, e, g), PE.model_diameter(p)) + tuple(r[k] for k in sorted(r))       # (the diameter splits its targets: the key path)

    eager = both()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = both()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, warm))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = both()
    for _ in range(2):
        for v in captured:
            v.fill_(-7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, captured))
