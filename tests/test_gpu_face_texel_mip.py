"""GPU: K43 -- tp_face_texel_mip_reduce and tp_face_texel_shade_mip (ops.face_texel_mip_reduce, ops.face_texel_shade_mip,
face_texels.build_mips, ops.mesh_raster(texel_mips=), SurfelRenderer(texel_mips=), tools/bake_texture.py --texel-mips) -- bit for bit
against the fp64 restatement of their contract in tests/face_texel_mip_ref.py, against K35 itself where the rule says they coincide, at
their edges, captured, and through the layers above."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import face_texel_mip_ref as MREF
import texture_bake_ref as TREF
from texpose_amd import _lib
from texpose_amd import face_texels as FT
from texpose_amd import texture_bake as TB

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GUARD = 4096                               # floats: 16 KiB on both sides


def cu(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x, dtype=dtype).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(x):
    return (host(x) if torch.is_tensor(x) else np.ascontiguousarray(x, dtype=np.float32)).view(np.uint32)


def guarded(shape):
    """a float32 tensor of ``shape`` inside a buffer with guard bands on both sides, all 0xAB bytes"""
    n = int(np.prod(shape))
    buf = torch.empty(n + 2 * GUARD, device=DEV)
    buf.view(torch.uint8).fill_(0xAB)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf):
    b = buf.view(torch.uint8)
    return bool((b[:4 * GUARD] == 0xAB).all()) and bool((b[-4 * GUARD:] == 0xAB).all())


_sub, _chains = {}, {}


def node_index(name, R):
    if (name, R) not in _sub:
        _sub[name, R] = FT.subdivide(*MREF.MESHES[name](), R)[2]
    return _sub[name, R]


def slots(name, Rc):
    verts, faces = MREF.MESHES[name]()
    return tuple(cu(t) for t in FT.mip_slots(verts, faces, Rc))


def texture(name, R, seed=0, shared=True):
    """random texels [F,T(R),3]: one value per unique node (continuous across edges) or one per slot"""
    ni = node_index(name, R)
    rs = np.random.RandomState(1000 * seed + R)
    return rs.rand(int(ni.max()) + 1, 3).astype(np.float32)[ni] if shared else rs.rand(ni.shape[0], ni.shape[1], 3).astype(np.float32)


def chain(name, R, seed=0, shared=True):
    """the restatement's levels of texture(name, R, seed, shared), once per key"""
    key = (name, R, seed, shared)
    if key not in _chains:
        _chains[key] = MREF.chain(texture(name, R, seed, shared), lambda Rc: node_index(name, Rc))
    return _chains[key]


# ---- the reduce
@pytest.mark.parametrize("name", list(MREF.MESHES))
def test_reduce_is_bit_equal_to_the_restatement_down_every_level(name):
    from texpose_amd import ops
    verts, faces = MREF.MESHES[name]()
    for R, shared in ((2, True), (4, False), (6, True), (8, False), (64, True)):
        want = chain(name, R, 0, shared)
        assert len(want) == FT.mip_levels(R) == {2: 2, 4: 3, 6: 2, 8: 4, 64: 7}[R]
        mips = FT.build_mips(verts, faces, cu(want[0]))
        torch.cuda.synchronize()
        assert (mips.R, mips.L, mips.F) == (R, len(want), len(faces)) and mips.packed.numel() == _lib.load().tp_face_texel_mip_elems(len(faces), R, mips.L)
        assert (bits(mips.packed) == bits(MREF.pack(want))).all(), (name, R)
        for l in range(mips.L):
            assert mips.level(l).shape == want[l].shape and (bits(mips.level(l).contiguous()) == bits(want[l])).all(), (name, R, l)
        # one level by the op itself, fewer levels on request
        one = ops.face_texel_mip_reduce(cu(want[0]), *slots(name, R // 2))
        assert (bits(one) == bits(want[1])).all()
        assert FT.build_mips(verts, faces, want[0], levels=2).L == 2
    with pytest.raises(ValueError):
        FT.build_mips(verts, faces, cu(texture(name, 6)), levels=3)


def test_reduce_nan_bad_slots_and_guard_bands():
    from texpose_amd import ops
    name, Rf = "icosphere", 8
    F, Tc = 20, FT.texel_count(Rf // 2)
    fine = texture(name, Rf, 2).copy()
    fine[3, 7] = np.nan
    fine[11, 0, 1] = np.inf
    ptr, lst = FT.mip_slots(*MREF.MESHES[name](), Rf // 2)
    bad = lst.copy()
    bad[[0, 17, 100, len(bad) - 1]] = [-1, F * Tc, -(1 << 31), (1 << 31) - 1]
    for slot_list in (lst, bad):
        want = MREF.reduce(fine, ptr, slot_list)
        buf, out = guarded((F, Tc, 3))
        ops.face_texel_mip_reduce(cu(fine), cu(ptr), cu(slot_list), out=out)
        torch.cuda.synchronize()
        assert guards_intact(buf) and (bits(out.contiguous()) == bits(want)).all()
        assert not np.isfinite(want).all() and np.isfinite(want).mean() > 0.8            # the non-finite texels spread to their nodes only
    assert (want.reshape(-1, 3)[lst[[0, 17, 100, len(bad) - 1]]] == 0).all()              # slots no list names stay zero


# ---- the shade
def focal_K(H, W, focals):
    return np.stack([np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]], dtype=np.float32) for f in focals])


def full_plane(B, H, W, F):
    """every pixel claims a face; -2, -1 and F among them"""
    return np.broadcast_to((np.arange(H * W).reshape(H, W) % (F + 3) - 2)[None], (B, H, W)).astype(np.int32).copy()


class Mips:
    """what ops.face_texel_shade_mip wants of its ``mips``: the packed levels, R and L"""

    def __init__(self, levels):
        self.packed, self.L = cu(MREF.pack(levels)), len(levels)
        self.R = FT.resolution_of(levels[0].shape[1])


FOCALS = (900.0, 40.0, 3.0)               # at 400 mm the icosphere's faces are 118, 5 and 0.4 pixels long: magnified, blending, beyond R = 8's last level
_shade = {}


def shade_case(R, L, H=37, W=53, footprint=1.0, plane="full"):
    """inputs, the restatement's result (rgb fp32, d, l0, t) and the kernel's, once per key"""
    from texpose_amd import ops
    key = (R, L, H, W, footprint, plane)
    if key not in _shade:
        verts, faces = MREF.icosphere()
        poses = TB.sphere_view_poses(3, 400.0).astype(np.float32)
        K = focal_K(H, W, FOCALS)
        if plane == "full":
            face = full_plane(3, H, W, len(faces))
        else:
            face = host(ops.mesh_raster(cu(verts), cu(faces), cu(poses), cu(K), H=H, W=W, normals=False)["face"])
        levels = chain("icosphere", R, 1)[:L]
        want, d, l0, t = MREF.shade(face, verts, faces, levels, poses, K, H, W, footprint=footprint, details=True)
        got = ops.face_texel_shade_mip(cu(face), cu(verts), cu(faces), Mips(levels), cu(poses), cu(K), footprint=footprint)
        torch.cuda.synchronize()
        _shade[key] = dict(verts=verts, faces=faces, poses=poses, K=K, face=face, levels=levels, want=want.astype(np.float32), d=d, l0=l0, t=t, got=got)
    return _shade[key]


@pytest.mark.parametrize("plane", ["full", "raster"])
@pytest.mark.parametrize("R,L", [(8, 4), (6, 2), (8, 2)])
def test_shade_is_bit_equal_to_the_restatement(R, L, plane):
    c = shade_case(R, L, plane=plane)
    d, l0, t = c["d"], c["l0"], c["t"]
    if plane == "full":                  # one image magnified, one blending, one beyond the last level (of the pixels whose d is finite)
        last = 4.0 ** (L - 1)
        share = [(d[0] <= 1).mean(), ((d[1] > 1) & (d[1] < last) & (t[1] > 0)).mean(), (d[2] >= last).mean()]
        print("R=%d L=%d: magnified %.2f of image 0, blending %.2f of image 1, beyond the last level %.2f of image 2" % ((R, L) + tuple(share)))
        assert share[0] > 0.5 and share[1] > (0.3 if L > 2 else 0.1) and share[2] > 0.2
        assert set(np.unique(l0)) == set(range(L))
    assert c["got"].shape == c["want"].shape and (bits(c["got"]) == bits(c["want"])).all()
    assert (c["want"] != 0).any() and (c["want"][c["face"] < 0] == 0).all() and (c["want"][c["face"] >= 20] == 0).all()


@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 17)], ids=lambda s: "%dx%d" % s)
def test_shade_sizes(size):
    c = shade_case(8, 4, H=size[0], W=size[1])
    assert (bits(c["got"]) == bits(c["want"])).all()
    c = shade_case(8, 4, H=size[0], W=size[1], plane="raster")
    assert (bits(c["got"]) == bits(c["want"])).all()


def test_identities_with_k35_itself():
    from texpose_amd import ops
    c = shade_case(8, 4)
    face, v, f, p, k = (cu(c[n]) for n in ("face", "verts", "faces", "poses", "K"))
    k35 = ops.face_texel_shade(face, v, f, cu(c["levels"][0]), p, k)
    # L = 1: K35 at every distance
    one = ops.face_texel_shade_mip(face, v, f, Mips(c["levels"][:1]), p, k)
    assert torch.equal(one.view(torch.int32), k35.view(torch.int32)) and bool((k35 != 0).any())
    # magnified pixels are K35's pixels
    near = cu(c["d"] <= 1)
    assert int(near.sum()) > 1500 and torch.equal(c["got"][near].view(torch.int32), k35[near].view(torch.int32))
    # beyond the last level: K35 on the last level's texels
    last = ops.face_texel_shade(face, v, f, cu(c["levels"][-1]), p, k)
    far = cu(np.isfinite(c["d"]) & (c["d"] >= 64))
    assert int(far.sum()) > 500 and torch.equal(c["got"][far].view(torch.int32), last[far].view(torch.int32)) and bool((last[far] != 0).any())
    # and in between the kernel differs from both
    mid = cu((c["t"] > 0.2) & (c["t"] < 0.8) & (c["want"] != 0).any(-1))
    assert int(mid.sum()) > 300 and bool((c["got"][mid] != k35[mid]).any(-1).float().mean() > 0.9)


def test_footprint_moves_the_level_as_restated():
    cases = {fp: shade_case(8, 4, footprint=fp) for fp in (0.25, 1.0, 4.0)}
    for fp, c in cases.items():
        assert (bits(c["got"]) == bits(c["want"])).all(), fp
    finite = np.isfinite(cases[1.0]["d"])
    assert np.allclose(cases[4.0]["d"][finite], 4.0 * cases[1.0]["d"][finite], rtol=1e-15) and np.allclose(cases[0.25]["d"][finite], 0.25 * cases[1.0]["d"][finite], rtol=1e-15)
    mean_level = [float((cases[fp]["l0"] + cases[fp]["t"]).mean()) for fp in (0.25, 1.0, 4.0)]
    print("mean level at footprint 0.25, 1, 4: %.3f %.3f %.3f" % tuple(mean_level))
    assert mean_level[0] + 0.2 < mean_level[1] < mean_level[2] - 0.2
    inner = (cases[1.0]["l0"] >= 1) & (cases[1.0]["l0"] + 1 <= 2) & (cases[1.0]["t"] > 0)
    assert inner.sum() > 100 and (cases[4.0]["l0"][inner] == cases[1.0]["l0"][inner] + 1).all() and (cases[0.25]["l0"][inner] == cases[1.0]["l0"][inner] - 1).all()
    assert (cases[4.0]["t"][inner] == cases[1.0]["t"][inner]).all()                   # a factor 4 is exactly one level


def test_inputs_that_must_shade_to_zero():
    from texpose_amd import ops
    c = shade_case(8, 4)
    H, W, F = 37, 53, len(c["faces"])
    v, f, p, k = (cu(c[n]) for n in ("verts", "faces", "poses", "K"))
    mips = Mips(c["levels"])

    def run(face=None, verts=None, poses=None, levels=None):
        buf, out = guarded((3, H, W, 3))
        face = c["face"] if face is None else face
        got = ops.face_texel_shade_mip(cu(face), v if verts is None else cu(verts), f, mips if levels is None else Mips(levels),
                                       p if poses is None else cu(poses), k, out=out)
        torch.cuda.synchronize()
        want = MREF.shade(face, c["verts"] if verts is None else verts, c["faces"], c["levels"] if levels is None else levels,
                          c["poses"] if poses is None else poses, c["K"], H, W).astype(np.float32)
        assert got.data_ptr() == out.data_ptr() and guards_intact(buf) and (bits(out.contiguous()) == bits(want)).all()
        return host(out)

    # face plane entries of -1, F and INT_MAX (and INT_MIN) beside valid ones
    plane = c["face"].copy() % F
    plane[plane < 0] += F
    bad = np.zeros(plane.shape, dtype=bool)
    for n, value in enumerate((-1, F, (1 << 31) - 1, -(1 << 31))):
        bad[:, :, n::9] = True
        plane[:, :, n::9] = value
    out = run(face=plane)
    assert (out[bad] == 0).all() and (out[~bad] != 0).any()
    # a vertex at z <= 0: with vertex 0 moved to the camera plane of image 0 and behind it, the faces that use it shade to zero
    valid = np.abs(c["face"]) % F
    for depth in (-0.01, -50.0):
        verts = c["verts"].copy()
        R0, t0 = c["poses"][0, :, :3].astype(np.float64), c["poses"][0, :, 3].astype(np.float64)
        verts[0] = (R0.T @ (np.array([0.0, 0.0, depth]) - t0)).astype(np.float32)
        out = run(face=valid, verts=verts)
        uses = (c["faces"] == 0).any(1)[valid[0]]
        assert uses.sum() > 100 and (out[0][uses] == 0).all() and (out[0][~uses] != 0).any()
    # a NaN pose in one image of three
    poses = c["poses"].copy()
    poses[1, 0, 1] = np.nan
    out = run(face=valid, poses=poses)
    assert (out[1] == 0).all() and (out[0] != 0).any() and (out[2] != 0).any()
    # a NaN texel on one level only: zero where that level is read and the texel touched, untouched elsewhere
    base = run(face=valid)
    levels = [l.copy() for l in c["levels"]]
    levels[1][:, ::2] = np.nan
    out = run(face=valid, levels=levels)
    _, d, l0, t = MREF.shade(valid, c["verts"], c["faces"], c["levels"], c["poses"], c["K"], H, W, details=True)
    reads = (l0 == 1) | ((l0 == 0) & (t > 0))
    assert np.isfinite(out).all() and (out[~reads] == base[~reads]).all() and (out[~reads] != 0).any()
    assert ((out[reads] == 0).all(-1) & (base[reads] != 0).any(-1)).mean() > 0.5


def test_determinism_and_graph_capture_of_both_entry_points():
    from texpose_amd import ops
    c = shade_case(8, 4)
    face, v, f, p, k = (cu(c[n]) for n in ("face", "verts", "faces", "poses", "K"))
    mips = Mips(c["levels"])
    first, again = ops.face_texel_shade_mip(face, v, f, mips, p, k), ops.face_texel_shade_mip(face, v, f, mips, p, k)
    assert torch.equal(first.view(torch.int32), again.view(torch.int32)) and torch.equal(first.view(torch.int32), c["got"].view(torch.int32))
    fine, (ptr, lst) = cu(c["levels"][0]), slots("icosphere", 4)
    coarse, coarse2 = ops.face_texel_mip_reduce(fine, ptr, lst), ops.face_texel_mip_reduce(fine, ptr, lst)
    assert torch.equal(coarse.view(torch.int32), coarse2.view(torch.int32)) and (bits(coarse) == bits(c["levels"][1])).all()
    cap_rgb, cap_coarse = torch.empty_like(first), torch.empty_like(coarse)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.face_texel_mip_reduce(fine, ptr, lst, out=cap_coarse)
        ops.face_texel_shade_mip(face, v, f, mips, p, k, out=cap_rgb)
    for _ in range(2):
        cap_rgb.view(torch.uint8).fill_(0xAB)
        cap_coarse.view(torch.uint8).fill_(0xAB)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap_rgb.view(torch.int32), first.view(torch.int32)) and torch.equal(cap_coarse.view(torch.int32), coarse.view(torch.int32))


def test_refused_arguments_launch_nothing_and_wrappers_raise():
    from texpose_amd import ops
    c = shade_case(8, 4)
    H, W, F, V = 37, 53, len(c["faces"]), len(c["verts"])
    lib = _lib.load()
    mips = Mips(c["levels"])
    t = dict(verts=cu(c["verts"]), faces=cu(c["faces"]), mips=mips.packed, pose=cu(c["poses"]), intr=cu(c["K"]), face=cu(c["face"]))
    buf, out = guarded((3, H, W, 3))

    def shade(**kw):
        a = _lib.FaceTexelShadeMipArgs()
        for name, v in t.items():
            setattr(a, name, v.data_ptr())
        a.B, a.H, a.W, a.V, a.F, a.R, a.L, a.footprint, a.rgb = 3, H, W, V, F, 8, 4, 1.0, out.data_ptr()
        for name, v in kw.items():
            setattr(a, name, v)
        return lib.tp_face_texel_shade_mip(C.byref(a), None), lib.tp_last_error().decode()

    for kw in (dict(B=0), dict(H=-1), dict(W=0), dict(V=0), dict(F=0), dict(R=0), dict(R=65), dict(L=0), dict(L=5), dict(R=6, L=3), dict(R=7, L=2),
               dict(H=65536, W=32768), dict(F=1 << 30), dict(footprint=0.0), dict(footprint=-1.0), dict(footprint=float("nan")),
               dict(footprint=float("inf")), dict(rgb=None), dict(mips=None), dict(face=None), dict(verts=None)):
        rc, msg = shade(**kw)
        assert rc == -1 and "tp_face_texel_shade_mip" in msg, (kw, rc, msg)
    fine, (ptr, lst) = cu(c["levels"][0]), slots("icosphere", 4)
    buf2, coarse = guarded((F, FT.texel_count(4), 3))

    def reduce(**kw):
        a = _lib.FaceTexelMipReduceArgs()
        a.fine, a.slot_ptr, a.slot_list, a.coarse = fine.data_ptr(), ptr.data_ptr(), lst.data_ptr(), coarse.data_ptr()
        a.F, a.Rf, a.U = F, 8, ptr.numel() - 1
        for name, v in kw.items():
            setattr(a, name, v)
        return lib.tp_face_texel_mip_reduce(C.byref(a), None), lib.tp_last_error().decode()

    for kw in (dict(F=0), dict(U=0), dict(Rf=7), dict(Rf=0), dict(Rf=66), dict(F=1 << 30, Rf=64), dict(fine=None), dict(slot_ptr=None), dict(slot_list=None),
               dict(coarse=None)):
        rc, msg = reduce(**kw)
        assert rc == -1 and "tp_face_texel_mip_reduce" in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert bool((buf.view(torch.uint8) == 0xAB).all()) and bool((buf2.view(torch.uint8) == 0xAB).all())       # the outputs keep their poison
    assert shade()[0] == 0 and reduce()[0] == 0
    torch.cuda.synchronize()
    assert guards_intact(buf) and guards_intact(buf2) and (bits(out.contiguous()) == bits(c["want"])).all() and (bits(coarse.contiguous()) == bits(c["levels"][1])).all()
    # the wrappers
    args = (t["face"], t["verts"], t["faces"], mips, t["pose"], t["intr"])
    other = Mips(chain("octahedron", 8, 1))                                               # the chain of another mesh: 8 faces
    for bad in ((args[0].float(),) + args[1:], args[:3] + (other,) + args[4:], args[:3] + (t["mips"],) + args[4:], args[:2] + (t["faces"][:, :2],) + args[3:],
                args[:4] + (t["pose"][:2],) + args[5:]):
        with pytest.raises(ValueError):
            ops.face_texel_shade_mip(*bad)
    for kw in (dict(footprint=0.0), dict(footprint=float("nan")), dict(out=torch.empty(3, H, W, 4, device=DEV)), dict(out=torch.empty(3, H, W, 3, device=DEV, dtype=torch.float64))):
        with pytest.raises(ValueError):
            ops.face_texel_shade_mip(*args, **kw)
    short = Mips(c["levels"])
    short.L = 5
    with pytest.raises(ValueError):
        ops.face_texel_shade_mip(*args[:3], short, *args[4:])
    for bad in ((fine[:, :44], ptr, lst), (cu(texture("icosphere", 3)), ptr, lst), (fine, ptr.float(), lst), (fine, ptr, lst[:-1]), (fine, ptr[:1], lst),
                (fine.double()[:, :, :2], ptr, lst)):
        with pytest.raises(ValueError):
            ops.face_texel_mip_reduce(*bad)
    with pytest.raises(ValueError):
        ops.face_texel_mip_reduce(fine, ptr, lst, out=torch.empty(F, 15, 4, device=DEV))
    with pytest.raises(ValueError):                                                         # texel_mips without the texels' mesh
        ops.mesh_raster(t["verts"], t["faces"], t["pose"], t["intr"], H=H, W=W, normals=False, texel_mips=other)
    with pytest.raises(ValueError):
        ops.mesh_raster(t["verts"], t["faces"], t["pose"], t["intr"], H=H, W=W, normals=False, texels=cu(c["levels"][1]), texel_mips=mips)
    with pytest.raises(ValueError):
        ops.mesh_raster(t["verts"], t["faces"], t["pose"], t["intr"], H=H, W=W, vcolor=torch.rand(V, 3, device=DEV), texel_mips=mips)


# ---- the layers above
def test_mesh_raster_and_surfel_renderer_with_texel_mips():
    from texpose_amd import ops
    from texpose_amd.surfel import SurfelRenderer
    H, W, B = 37, 53, 3
    verts, faces = TREF.uv_sphere(6, 8)
    poses = TB.sphere_view_poses(B, 400.0).astype(np.float32)
    K = focal_K(H, W, (600.0, 120.0, 30.0))
    texels = torch.rand(len(faces), FT.texel_count(8), 3, device=DEV)
    mips = FT.build_mips(verts, faces, texels)
    v, f, p, k = cu(verts), cu(faces), cu(poses), cu(K)
    for cull in (False, True):
        plain = ops.mesh_raster(v, f, p, k, H=H, W=W, normals=False, cull=cull)
        want = ops.face_texel_shade_mip(plain["face"], v, f, mips, p, k)
        for kw in (dict(texel_mips=mips), dict(texel_mips=mips, texels=texels), dict(texel_mips=mips, face_ids=False)):
            one = ops.mesh_raster(v, f, p, k, H=H, W=W, normals=False, cull=cull, **kw)
            assert torch.equal(one["rgb"].view(torch.int32), want.view(torch.int32)) and torch.equal(one["face"], plain["face"])
            assert torch.equal(one["zbuf"].view(torch.int32), plain["zbuf"].view(torch.int32))
    point = ops.mesh_raster(v, f, p, k, H=H, W=W, normals=False, texels=texels)["rgb"]
    assert bool((want != 0).any()) and not torch.equal(want[1:], point[1:])                # the far images are filtered
    # SurfelRenderer: L = 1 is the point-sampled renderer bit for bit; the whole chain is not
    pose_nerf = TB.poses_to_nerf_units(torch.from_numpy(poses), 10.0).float()
    base = SurfelRenderer(verts, faces, None, H, W, DEV, texels=texels)(pose_nerf, K, 10.0)
    one = SurfelRenderer(verts, faces, None, H, W, DEV, texels=texels, texel_mips=FT.build_mips(verts, faces, texels, levels=1))(pose_nerf, K, 10.0)
    alone = SurfelRenderer(verts, faces, None, H, W, DEV, texel_mips=FT.build_mips(verts, faces, texels, levels=1))(pose_nerf, K, 10.0)
    whole = SurfelRenderer(verts, faces, None, H, W, DEV, texel_mips=mips)(pose_nerf, K, 10.0)
    assert bool((base.rgb_syn != 0).any()) and torch.equal(one.rgb_syn.view(torch.int32), base.rgb_syn.view(torch.int32))
    assert torch.equal(alone.rgb_syn.view(torch.int32), base.rgb_syn.view(torch.int32)) and torch.equal(whole.depth, base.depth)
    assert not torch.equal(whole.rgb_syn, base.rgb_syn)
    with pytest.raises(ValueError):
        SurfelRenderer(verts, faces, np.zeros_like(verts), H, W, DEV, texel_mips=mips)


def test_bake_texture_with_texel_mips_verifies_and_writes_the_same_files(tmp_path):
    """bake_texture --texel-res 4 --verify with and without --texel-mips on a random-weight checkpoint: both run, the PLY and the
    texel file are the same bytes (the chain is never stored), and the report names the levels."""
    import oracle.texpose_oracle as O
    from texpose_amd import checkpoint as ck
    from texpose_amd.graph import Graph
    from texpose_amd.options import default_options
    H, W, N, oid = 48, 64, 8, 5
    opt = default_options(H=H, W=W, device=DEV)
    opt.nerf.sample_intvs, opt.nerf.sample_stratified = N, False
    opt.arch.mlp_precision = "fp32"
    graph = Graph(opt).to(DEV)
    graph.nerf.load_state_dict({**graph.nerf.state_dict(), **{k: v.to(DEV) for k, v in O.make_params(3).items()}})
    graph.attach_latents(4, opt)
    torch.save(ck.make_checkpoint(graph, epoch=1, it=10), str(tmp_path / "model.ckpt"))
    verts, faces = TREF.uv_sphere(12, 16)
    TB.write_ply(str(tmp_path / "sphere.ply"), verts, faces, np.zeros_like(verts))
    files = {}
    for tag, extra in (("plain", []), ("mips", ["--texel-mips"])):
        out, report = tmp_path / ("%s.ply" % tag), tmp_path / ("%s.json" % tag)
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(REPO, "tools", "bake_texture.py"), "--checkpoint", str(tmp_path / "model.ckpt"),
               "--ply", "%d=%s" % (oid, tmp_path / "sphere.ply"), "--sphere", "6", "--distance-mm", "400", "--focal", "150", "--H", str(H), "--W", str(W),
               "--samples", str(N), "--precision", "fp32", "--out", str(out), "--report", str(report), "--verify", "--texel-res", "4"] + extra
        p = subprocess.run(cmd, capture_output=True, text=True)
        assert p.returncode == 0 and "PSNR" in p.stdout, p.stdout + p.stderr
        rep = json.loads(report.read_text())
        assert rep["verify"]["pixels"] > 0 and np.isfinite(rep["verify"]["psnr_db"])
        files[tag] = (out.read_bytes(), (tmp_path / ("%s.texels.npz" % tag)).read_bytes(), rep)
    assert files["plain"][0] == files["mips"][0] and files["plain"][1] == files["mips"][1]
    assert files["mips"][2]["texels"]["mip_levels"] == 3 and "mip_levels" not in files["plain"][2]["texels"]
    bad = subprocess.run([sys.executable, os.path.join(REPO, "tools", "bake_texture.py"), "--checkpoint", "x", "--ply", "1=x", "--sphere", "2", "--distance-mm", "400",
                          "--out", "x", "--texel-res", "6", "--texel-mips", "3"], capture_output=True, text=True)
    assert bad.returncode != 0 and "--texel-mips" in bad.stderr
