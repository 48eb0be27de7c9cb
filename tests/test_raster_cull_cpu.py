"""No GPU: the host side of K34 (the header-derived binding of tp_mesh_raster_culled, its workspace query and its refusals, which launch
nothing), texpose_amd.surfel.coherent_face_order, and the counts of what the culled rasteriser skips (tests/raster_cull_ref.py), which
regenerate the count table of DESIGN section 24."""
import ctypes as C

import numpy as np
import pytest
import torch

import raster_cull_ref as CULL


# ----------------------------------------------------------------------------- the binding, the workspace query, the argument checks
def test_binding_has_the_culled_rasteriser():
    from texpose_amd import _lib
    assert _lib.ABI_VERSION == 16
    assert "tp_mesh_raster_culled" in _lib.SYMBOLS and "tp_mesh_raster_culled_workspace_bytes" in _lib.SYMBOLS
    assert _lib.HEADER.prototypes["tp_mesh_raster_culled"] == (C.c_int, [C.POINTER(_lib.MeshRasterArgs), C.c_void_p])
    assert _lib.HEADER.prototypes["tp_mesh_raster_culled_workspace_bytes"] == (C.c_size_t, [C.c_int] * 4)
    assert _lib.HEADER.prototypes["tp_mesh_raster_culled"] == _lib.HEADER.prototypes["tp_mesh_raster"]
    # the struct is K19's, untouched
    p, f3, i = C.c_void_p, C.c_float * 3, C.c_int
    fields = [("verts", p), ("faces", p), ("vcolor", p), ("nocs_center", f3), ("nocs_scale", f3), ("pose", p), ("intr", p), ("B", i), ("H", i),
              ("W", i), ("V", i), ("F", i), ("normals_from_zbuf", i), ("zbuf", p), ("face", p), ("rgb", p), ("nocs", p), ("normal", p), ("workspace", p)]
    assert list(_lib.MeshRasterArgs._fields_) == fields and C.sizeof(_lib.MeshRasterArgs) == 136
    lib = _lib.load()
    assert hasattr(lib, "tp_mesh_raster_culled") and hasattr(lib, "tp_mesh_raster_culled_workspace_bytes") and lib.tp_abi_version() == 16


def test_workspace_query():
    from texpose_amd import _lib
    lib = _lib.load()
    query = lib.tp_mesh_raster_culled_workspace_bytes
    for F in (1, 255, 256, 257, 65536, 65537):
        for B in (1, 3, 64):
            want = 64 * B * F + 16 * B * -(-F // 256)
            assert query(B, 480, 640, F) == want and query(B, 1, 1, F) == want, (B, F)
            assert want % 16 == 0 and want - lib.tp_mesh_raster_workspace_bytes(B, 480, 640, F) == 16 * B * -(-F // 256)
    for B, F in ((0, 10), (-1, 10), (2, 0), (2, -5), (0, 0)):
        assert query(B, 480, 640, F) == 0 and lib.tp_mesh_raster_workspace_bytes(B, 480, 640, F) == 0
    assert query(65535, 16, 16, 500000) == 64 * 65535 * 500000 + 16 * 65535 * 1954               # (beyond 32 bits)


def _aligned_buffer(n):
    buf = C.create_string_buffer(n + 16)
    return buf, C.addressof(buf) + (-C.addressof(buf)) % 16


def test_argument_errors_launch_nothing():
    """Every pointer is a host buffer: a launch would fault, a refusal returns before anything reads them.  The same refusals, with the
    same words, as tp_mesh_raster's, each under its own entry point's name."""
    from texpose_amd import _lib
    lib = _lib.load()
    keep, p = _aligned_buffer(1 << 14)

    def args(**kw):
        a = _lib.MeshRasterArgs()
        for k, (name, t) in enumerate(_lib.MeshRasterArgs._fields_):
            if t is C.c_void_p:
                setattr(a, name, p + 512 * k)
        a.B, a.H, a.W, a.V, a.F, a.normals_from_zbuf = 2, 4, 4, 5, 3, 0
        a.nocs_center, a.nocs_scale = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for name in ("tp_mesh_raster_culled", "tp_mesh_raster"):
        fn = getattr(lib, name)
        err = lambda: lib.tp_last_error()
        refused = lambda word, a: fn(None if a is None else C.byref(a), None) == -1 and err() == name.encode() + b": " + word
        assert refused(b"null pointer", None)
        for bad in (dict(B=0), dict(B=-1), dict(B=65536), dict(H=0), dict(W=0), dict(H=16385), dict(W=16385), dict(V=0), dict(F=0), dict(F=-3)):
            assert refused(b"bad sizes", args(**bad)), bad
        for ptr in ("pose", "intr", "zbuf", "verts", "faces", "workspace"):
            assert refused(b"null pointer", args(**{ptr: None})), ptr
        assert refused(b"workspace must be 16-byte aligned", args(workspace=p + 8))
        assert refused(b"workspace must be 16-byte aligned", args(workspace=p + 4))
        assert refused(b"rgb requested without vertex colours", args(vcolor=None))
        for scale in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, float("nan"))):
            assert refused(b"nocs requested with a non-positive normalisation scale", args(nocs_scale=(C.c_float * 3)(*scale))), scale
        assert refused(b"normals_from_zbuf without a normal output", args(normals_from_zbuf=1, normal=None))
        assert refused(b"bad sizes", args(normals_from_zbuf=1, B=0))
        assert refused(b"null pointer", args(normals_from_zbuf=1, zbuf=None))
    del keep


def test_ops_refuse_cpu_tensors_with_and_without_cull():
    from texpose_amd import _lib, ops, pose_error
    from texpose_amd.surfel import SurfelRenderer
    verts, faces = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    pose, K = torch.zeros(1, 3, 4), torch.eye(3)
    for cull in (False, True):
        with pytest.raises(_lib.TexposeLibraryError, match="verts must live on the GPU"):
            ops.mesh_raster(verts, faces, pose, K, H=4, W=4, cull=cull)
        with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
            ops.depth_icp(verts, faces, pose, K, torch.zeros(1, 4, 4), cull=cull)
        with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
            ops.photo_align(verts, faces, torch.zeros(4, 3), pose, K, torch.zeros(1, 4, 4, 3), cull=cull)
        with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
            ops.silhouette_align(verts, faces, pose, K, torch.zeros(1, 4, 4), cull=cull)
        with pytest.raises(_lib.TexposeLibraryError, match="GPU"):
            ops.joint_align(verts, faces, pose, K, sdf=torch.zeros(1, 4, 4), cull=cull)
        with pytest.raises(ValueError, match="no CPU route"):
            pose_error.vsd(verts, faces, pose, pose, K, torch.zeros(1, 4, 4), 10.0, H=4, W=4, cull=cull)
    assert SurfelRenderer(verts.numpy(), faces.numpy(), None, 4, 4, "cpu", cull=True).cull is True
    assert SurfelRenderer(verts.numpy(), faces.numpy(), None, 4, 4, "cpu").cull is False


# ----------------------------------------------------------------------------- coherent_face_order
def _interleave(q):
    code = np.zeros(len(q), dtype=np.int64)
    for bit in range(10):
        for axis in range(3):
            code |= ((q[:, axis] >> bit) & 1) << (3 * bit + 2 - axis)
    return code


def test_coherent_face_order_is_a_stable_morton_sort():
    from texpose_amd.surfel import coherent_face_order
    rs = np.random.RandomState(0)
    v, f = CULL.uv_sphere(12, 24, ripple=0.2)
    f = f[rs.permutation(len(f))]
    perm = coherent_face_order(v, f)
    assert perm.dtype == np.int64 and perm.shape == (len(f),) and np.array_equal(np.sort(perm), np.arange(len(f)))
    assert np.array_equal(perm, coherent_face_order(v, f)) and np.array_equal(perm, coherent_face_order(v.copy(), f.copy()))
    # the code, bit by bit: 10 bits per axis over the largest extent, x highest; equal codes keep their order
    c = v.astype(np.float64)[f].mean(1)
    lo, hi = v.astype(np.float64).min(0), v.astype(np.float64).max(0)
    q = np.minimum(np.floor((c - lo) * (1024.0 / (hi - lo).max())), 1023).astype(np.int64)
    code = _interleave(q)
    assert np.array_equal(perm, np.argsort(code, kind="stable")) and (np.diff(code[perm]) >= 0).all()
    tied = np.nonzero(np.diff(code[perm]) == 0)[0]
    assert (perm[tied] < perm[tied + 1]).all()
    # a translation (exact in fp32 here: small integers on a grid of 2^-10 steps) changes nothing
    grid = np.round(v * 1024) / 1024
    base = coherent_face_order(grid.astype(np.float32), f)
    for shift in ([64.0, -32.0, 8.0], [-300.0, 0.0, 1000.0]):
        moved = (grid + np.array(shift)).astype(np.float32)
        assert np.array_equal(moved.astype(np.float64) - np.array(shift), grid.astype(np.float32).astype(np.float64))
        assert np.array_equal(coherent_face_order(moved, f), base), shift
    # faces the rasteriser drops do not break it; a single face; a flat mesh
    bad = f.copy()
    bad[5] = [0, 1, len(v)]
    bad[9] = [-1, 2, 3]
    pb = coherent_face_order(v, bad)
    assert np.array_equal(np.sort(pb), np.arange(len(f))) and set(pb[:2].tolist()) == {5, 9}
    assert coherent_face_order(v, f[:1]).tolist() == [0]
    assert coherent_face_order(np.zeros((3, 3), np.float32), np.array([[0, 1, 2], [2, 1, 0]])).tolist() == [0, 1]
    assert coherent_face_order(v, np.zeros((0, 3), np.int32)).shape == (0,)


# ----------------------------------------------------------------------------- the counts
@pytest.fixture(scope="module")
def table():
    """name -> dict(F, plain, mesh, shuffled, morton, faces_mean, faces_max): the (tile, chunk) pairs per image of DESIGN section 24."""
    from texpose_amd.surfel import coherent_face_order
    rows = {}
    for name, (v, f, pose, K, H, W) in CULL.table_cases().items():
        mesh = CULL.counts(v, f, pose, K, H, W)
        shuffled = CULL.counts(v, f[np.random.RandomState(0).permutation(len(f))], pose, K, H, W)
        morton = CULL.counts(v, f[coherent_face_order(v, f)], pose, K, H, W)
        assert mesh["plain"] == shuffled["plain"] == morton["plain"] == -(-H // 16) * -(-W // 16) * -(-len(f) // 256)
        rows[name] = dict(F=len(f), plain=mesh["plain"], mesh=mesh["culled"], shuffled=shuffled["culled"], morton=morton["culled"],
                          faces_mean=mesh["faces_mean"], faces_max=mesh["faces_max"])
    return rows


def test_count_table(table):
    print("\ncase                  faces    plain   mesh order     shuffled       morton   faces per busy tile (mean / max)")
    for name, r in table.items():
        gain = lambda k: "%7d (%4.0fx)" % (r[k], r["plain"] / max(1, r[k]))
        print("%-20s %6d %8d %s %s %s   %6.0f / %d" % (name, r["F"], r["plain"], gain("mesh"), gain("shuffled"), gain("morton"), r["faces_mean"],
                                                        r["faces_max"]))
    assert [table[k]["F"] for k in ("sphere_20k", "sphere_199k", "torus_26k")] == [20160, 198912, 25600]
    assert [table[k]["plain"] for k in table] == [94800, 932400, 120000, 5056]
    for name in ("sphere_20k", "sphere_199k", "torus_26k"):                    # the 480 x 640 cases
        r = table[name]
        assert r["plain"] >= 50 * r["mesh"], (name, r)
        assert r["plain"] >= 10 * r["shuffled"], (name, r)
        assert r["morton"] <= r["mesh"], (name, r)
    # the mesh-order counts are the prototype's, to the pair
    assert [table[k]["mesh"] for k in ("sphere_20k", "sphere_199k", "torus_26k")] == [1172, 8464, 1212]


def test_restatement_on_hand_cases():
    """Boxes by hand: the rounding rule at pixel centres, dropped faces, the union, the inclusive tile test."""
    K = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1]])
    pose = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    # at z = 1 a vertex (x, y, 1) lands at pixel position (x, y)
    tri = lambda x0, x1, y0, y1: [[x0, y0, 1.0], [x1, y0, 1.0], [x0, y1, 1.0]]
    v = np.array(tri(15.4, 16.6, 15.4, 16.6) + tri(15.5, 16.5, 3.0, 4.6) + tri(2.6, 3.4, 2.6, 3.4) + tri(-9.0, -2.0, 1.0, 5.0)
                 + [[1.0, 1.0, -1.0], [2.0, 9.0, 1.0], [7.0, 1.0, 1.0]] + tri(30.2, 40.0, 30.2, 40.0))
    f = np.arange(18).reshape(6, 3)
    box = CULL.face_boxes(v, f, pose, K, 33, 33)
    assert box[0].tolist() == [15, 16, 15, 16]                 # centres 15.5 and 16.5 lie inside [15.4, 16.6]
    assert box[1].tolist() == [15, 16, 3, 4]                   # a centre on the box's edge counts: ceil(15.5 - .5) = 15, floor(16.5 - .5) = 16
    assert tuple(box[2]) == CULL.EMPTY                         # no centre inside [2.6, 3.4]
    assert tuple(box[3]) == CULL.EMPTY                         # left of the image
    assert tuple(box[4]) == CULL.EMPTY                         # a vertex behind the camera
    assert box[5].tolist() == [30, 32, 30, 32]                 # clamped to the image
    assert tuple(CULL.face_boxes(v, [[0, 1, 99]], pose, K, 33, 33)[0]) == CULL.EMPTY
    cb = CULL.chunk_boxes(box)
    assert cb.tolist() == [[15, 32, 3, 32]]
    assert tuple(CULL.chunk_boxes(box[2:5])[0]) == CULL.EMPTY
    tiles = CULL.tiles_of(33, 33)
    assert tiles.tolist() == [[0, 15, 0, 15], [16, 31, 0, 15], [32, 32, 0, 15], [0, 15, 16, 31], [16, 31, 16, 31], [32, 32, 16, 31],
                              [0, 15, 32, 32], [16, 31, 32, 32], [32, 32, 32, 32]]
    assert CULL.overlaps(box[:1], tiles)[:, 0].tolist() == [True, True, False, True, True, False, False, False, False]
    one = np.array([[16, 16, 15, 15]])
    assert CULL.overlaps(one, tiles)[:, 0].tolist() == [False, True, False, False, False, False, False, False, False]
    assert not CULL.overlaps(np.array([CULL.EMPTY]), tiles).any()
