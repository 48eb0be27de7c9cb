"""K40 on the GPU: tp_photo_lighting against the numpy restatement (tests/photo_lighting_ref.py) on exactly the same planes, its apply
pass bit for bit, indices out of range, guard bands, reproducibility under repetition and graph replay, the coplanar fallback against
ops.photo_exposure's words, the loops ops.photo_align / joint / multi-view with lighting=True against the restatement's recorded
results (tests/golden/photo_lighting_loops.npz; tests/test_photo_lighting_cpu.py asserts the table), and tools/refine_poses.py --rgb
--lighting on a written BOP scene."""
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import photo_exposure_ref as XREF
import photo_lighting_ref as REF
import pnp_ref as PREF
from gn_ref import cu, host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RE_FLOOR, TE_FLOOR = 1e-3, 1e-3          # deg, mm: section 29's form of bar: twice the restatement's error plus these
BAND = 16384
INPUTS = ("verts", "faces", "face", "zbuf", "rgb", "pose", "image")


def bits(t):
    return t.contiguous().view(torch.uint8) if torch.is_tensor(t) else np.ascontiguousarray(t).view(np.uint8)


def same_bits(a, b):
    a, b = (host(x) if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def gpu_call(c, **kw):
    from texpose_amd import ops
    return ops.photo_lighting(*(cu(c[k]) for k in INPUTS), tau=c["tau"], light=cu(c["light_in"]), frame=cu(c["frame"]), mask=cu(c["mask"]), **kw)


def apply_all(c, light):
    return np.stack([REF.apply_ref(c["verts"], c["faces"], c["face"][b], c["zbuf"][b], c["rgb"][b], c["pose"][b], light[b]) for b in range(len(light))])


def compare(got, want, c):
    """The bars of one call, those of tests/test_gpu_photo_exposure.py's compare: no near-tie in the case, the integers equal, the light
    to 1e-6 max(1, |v|) (fp64 sums and a 5 x 5 solve in fp64 leave far less; what remains is a few fp32 roundings), rms to 1e-5
    relative + 1e-6; a failed fit returns the incoming light bit for bit; the applied colours are the call's own light through the
    stated operations, bit for bit."""
    assert (want["near_ties"] == 0).all(), "a near-tie in the case: change its seed"
    for k in ("count", "status", "flags"):
        assert np.array_equal(host(got[k]), want[k]), (k, host(got[k]), want[k])
    v = host(got["light"])
    assert (np.abs(v - want["light"]) <= 1e-6 * np.maximum(1.0, np.abs(want["light"]))).all(), (v, want["light"])
    came = np.tile(REF.IDENTITY, v.shape[:2] + (1,)) if c["light_in"] is None else c["light_in"]
    assert same_bits(v[want["status"] != 0], came[want["status"] != 0])
    rms = host(got["rms"]).astype(np.float64)
    assert np.array_equal(np.isnan(rms), np.isnan(want["rms"]))
    ok = ~np.isnan(rms)
    assert (np.abs(rms[ok] - want["rms"][ok]) <= 1e-5 * want["rms"][ok] + 1e-6).all(), (rms, want["rms"])
    if "rgb" in got:
        assert same_bits(got["rgb"], apply_all(c, v))


# ----------------------------------------------------------------------------- one call, exact inputs
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 5), (3, 3), (3, 7), (7, 65), (16, 16), (33, 257), (64, 80)])
def test_call_equals_the_restatement(H, W, B):
    """3 x 3 is the single interior pixel, 16 x 16 and 64 x 80 take the vector path, 7 x 65 and 33 x 257 the guarded path and the
    tile tail; with and without frame, mask and light_in."""
    kept, statuses, flags = 0, set(), set()
    for frames in ("one", "each", "map"):
        for with_mask in (False, True):
            for with_fit in (False, True):
                c = REF.one_call_case(1000 * H + 10 * W + B, B, H, W, frames, with_mask, with_fit)
                want = REF.call_ref(c)
                compare(gpu_call(c), want, c)
                kept += int(want["count"].sum())
                statuses |= set(want["status"].tolist())
                flags |= set(want["flags"][want["status"] == 0].tolist())
    if H < 3 or W < 3:
        assert kept == 0 and statuses == {1}
    if H * W >= 7 * 65:
        assert kept > 50 and 0 in statuses and 0 in flags        # (full 5 x 5 solves, not fallbacks)


def test_a_misaligned_rendering_takes_the_guarded_path():
    """rgb, then face, as a view 4 bytes into its storage: 16 x 16 would take the vector path; in place and out of place."""
    from texpose_amd import ops
    c = REF.one_call_case(7, 2, 16, 16, "each", True, True)
    want = REF.call_ref(c)
    assert (want["status"] == 0).all()
    for off in ("rgb", "face"):
        for inplace in (False, True):
            d = {k: cu(c[k]) for k in INPUTS}
            store = torch.empty(d[off].numel() + 1, device=DEV, dtype=d[off].dtype)
            view = store[1:].view(d[off].shape)
            view.copy_(d[off])
            d[off] = view
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            got = ops.photo_lighting(*(d[k] for k in INPUTS), tau=c["tau"], light=cu(c["light_in"]), mask=cu(c["mask"]), inplace=inplace)
            assert (got["rgb"].data_ptr() == d["rgb"].data_ptr()) == inplace
            compare(got, want, c)


# ----------------------------------------------------------------------------- apply
@pytest.mark.parametrize("H,W", [(16, 16), (7, 65), (33, 257)])
def test_apply_follows_the_stated_order_and_leaves_the_rest_alone(H, W):
    """s in fp64 from the fp32 light and the face's normal, rounded once, then s * c and + beta in fp32 -- said again here on the
    restatement's normals; pixels without a surface keep their words (NaN payloads planted); a covered pixel without a valid normal
    (a face index out of range) takes l0 * c + beta."""
    from texpose_amd import ops
    c = REF.one_call_case(11 + H, 3, H, W, "each", False, True)
    F = len(c["faces"])
    sub = c["face"][:, ::3, ::5]                                 # (a view: every 15th pixel loses its normal)
    sub[...] = np.array([-1, F, 2 ** 31 - 1, -2 ** 31], np.int32)[np.arange(sub.size).reshape(sub.shape) % 4]
    off = ~((c["zbuf"] > 0) & np.isfinite(c["zbuf"]))
    words = c["rgb"].view(np.uint32)
    words[off] = np.where(np.arange(int(off.sum()) * 3).reshape(-1, 3) % 2 == 0, 0x7FC12345, 0xFFA00001).astype(np.uint32)   # NaN payloads
    out = gpu_call(c)
    l = host(out["light"])
    assert (host(out["status"]) == 0).all() and np.abs(l[..., 1:4]).min() > 0
    lit, novalid = np.empty_like(c["rgb"]), np.zeros(off.shape, bool)
    with np.errstate(all="ignore"):
        for b in range(3):
            n, valid = REF.pixel_normals_ref(c["verts"], c["faces"], c["face"][b], c["pose"][b])
            q = l[b].astype(np.float64)
            s = (((q[:, 0] + q[:, 1] * n[..., 0:1]) + q[:, 2] * n[..., 1:2]) + q[:, 3] * n[..., 2:3]).astype(np.float32)
            s = np.where(valid[..., None], s, l[b, :, 0])
            lit[b] = s * c["rgb"][b]
            lit[b] = lit[b] + l[b, :, 4]
            novalid[b] = ~valid
            ambient = l[b, :, 0] * c["rgb"][b]
            ambient = ambient + l[b, :, 4]
            assert same_bits(lit[b][~valid], ambient[~valid])
    on = ~off
    assert on.sum() > 50 and off.sum() > 50 and (on & novalid).sum() > 5
    assert same_bits(host(out["rgb"])[on], lit[on]) and same_bits(host(out["rgb"])[off], c["rgb"][off])
    rgb = cu(c["rgb"])
    inplace = ops.photo_lighting(*(rgb if k == "rgb" else cu(c[k]) for k in INPUTS), tau=c["tau"], light=cu(c["light_in"]), inplace=True)
    assert inplace["rgb"] is rgb and same_bits(rgb, out["rgb"])
    for k in ops.PHOTO_LIGHTING_KEYS:
        assert same_bits(inplace[k], out[k]), k
    only = gpu_call(c, apply=False)
    assert "rgb" not in only and set(only) == set(ops.PHOTO_LIGHTING_KEYS) and all(same_bits(only[k], out[k]) for k in only)


# ----------------------------------------------------------------------------- indices out of range
@pytest.mark.parametrize("H,W", [(16, 16), (7, 65)])
def test_bad_indices_are_skipped(H, W):
    """A face plane holding -1, F, INT_MAX and INT_MIN and faces with an index >= V or < 0: the clamp's correctness -- such pixels have
    no normal, the fit skips them, the apply gives them the ambient form, and the results equal the restatement's."""
    c = REF.one_call_case(41 + H, 2, H, W, "each", False, True)
    F, V = len(c["faces"]), len(c["verts"])
    c["faces"] = c["faces"].copy()
    c["faces"][3], c["faces"][5], c["faces"][7], c["faces"][9] = [0, 1, V], [-1, 2, 3], [2 ** 31 - 1, 2, 3], [4, -2 ** 31, 5]
    rs = np.random.RandomState(H)
    hit = rs.uniform(size=c["face"].shape) < 0.2
    c["face"][hit] = rs.choice(np.array([-1, F, F + 1, 2 ** 31 - 1, -2 ** 31, -7], np.int32), int(hit.sum()))
    want = REF.call_ref(c)
    bad = hit | np.isin(c["face"], [3, 5, 7, 9])
    assert not want["kept"][bad].any() and (want["count"] > 20).all() and bad[:, 1:-1, 1:-1].sum() > 20
    got = gpu_call(c)
    torch.cuda.synchronize()
    compare(got, want, c)


# ----------------------------------------------------------------------------- the anchors
def test_exact_recovery_and_the_decision_paths():
    import test_photo_lighting_cpu as CPU
    c = CPU.exact_case(light=CPU.KNOWN)
    r = gpu_call(c)
    compare(r, REF.call_ref(c), c)
    assert np.abs(host(r["light"]).astype(np.float64) - CPU.KNOWN).max() <= 1e-5 and (host(r["rms"]) <= 1e-6).all()
    assert host(r["flags"]).tolist() == [0, 0] and host(r["count"]).tolist() == [150, 150]
    c = CPU.exact_case(H=3, W=7, light=CPU.KNOWN)                # five interior pixels: the light passed through
    c["light_in"] = (CPU.KNOWN + 0.01).astype(np.float32)
    r = gpu_call(c)
    compare(r, REF.call_ref(c), c)
    assert host(r["status"]).tolist() == [1, 1] and same_bits(r["light"], c["light_in"]) and same_bits(r["rgb"], apply_all(c, c["light_in"]))
    c = CPU.exact_case(H=2, W=5)                                 # no interior at all
    r = gpu_call(c)
    compare(r, REF.call_ref(c), c)
    assert host(r["count"]).tolist() == [0, 0] and np.isnan(host(r["rms"])).all() and same_bits(r["rgb"], c["rgb"])
    c = CPU.exact_case()                                         # an ambient term outside gain_range
    c["image"], c["tau"] = (8.0 * c["rgb"]).astype(np.float32), 100.0
    r = gpu_call(c)
    compare(r, REF.call_ref(c), c)
    assert host(r["flags"]).tolist() == [7 * (REF.FALLBACK | REF.CLAMPED)] * 2 and (host(r["light"])[..., 0] == 4.0).all()
    strong = CPU.KNOWN.copy()                                    # |l_dir| > l0 in one channel
    strong[0, 1, 1:4] = [0.9, -0.6, 0.5]
    c = CPU.exact_case(light=strong)
    r = gpu_call(c)
    compare(r, REF.call_ref(c), c)
    assert host(r["flags"]).tolist() == [REF.FALLBACK << 1, 0] and (host(r["light"])[0, 1, 1:4] == 0).all()
    compare(gpu_call(c, gain_range=(0.95, 4.0)), REF.call_ref(c, gain_range=(0.95, 4.0)), c)


def test_a_coplanar_mesh_gives_the_exposure_fits_words():
    """Two coplanar triangles: every channel falls back, and gain and bias are ops.photo_exposure's on the same planes bit for bit, with
    and without an incoming fit; so is the applied rendering."""
    import test_photo_lighting_cpu as CPU
    from texpose_amd import ops
    rs = np.random.RandomState(8)
    for H, W in ((12, 17), (33, 257), (64, 80)):
        c = CPU.exact_case(H, W, 2, mesh=REF.quad_mesh())
        c["image"] = (c["image"] + rs.uniform(-0.05, 0.05, c["image"].shape)).astype(np.float32)
        z, rgb, image = cu(c["zbuf"]), cu(c["rgb"]), cu(c["image"])
        for tau, light_in in ((2.0, None), (0.06, np.tile(np.float32([0.75, 0, 0, 0, 0.125]), (2, 3, 1)))):
            c["tau"], c["light_in"] = tau, light_in
            got = gpu_call(c)
            x = ops.photo_exposure(z, rgb, image, tau=tau, gain=None if light_in is None else cu(light_in[..., 0]), bias=None if light_in is None else cu(light_in[..., 4]))
            l = host(got["light"])
            assert same_bits(l[..., 0], x["gain"]) and same_bits(l[..., 4], x["bias"]) and (l[..., 1:4] == 0).all()
            assert same_bits(got["count"], x["count"]) and same_bits(got["status"], x["status"]) and same_bits(got["rgb"], x["rgb"])
            assert np.array_equal(host(got["flags"]), host(x["flags"]) | (7 * REF.FALLBACK)) and (host(x["count"]) > 50).all()
            compare(got, REF.call_ref(c), c)
        assert (host(got["count"]) < (H - 2) * (W - 2)).all()    # (the second round's tau dropped pixels)


# ----------------------------------------------------------------------------- memory, determinism, capture
def banded(shape, dtype):
    """A tensor between two 16-KiB bands of 0xAB -> (the tensor, a check that the bands are untouched)."""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    pad = (-n) % 16
    raw = torch.full((BAND + n + pad + BAND,), 0xAB, dtype=torch.uint8, device=DEV)
    t = raw[BAND:BAND + n].view(dtype).view(shape)

    def untouched():
        return bool((raw[:BAND] == 0xAB).all()) and bool((raw[BAND + n:] == 0xAB).all())
    return t, untouched


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 7, 65), (3, 33, 257)])
def test_nothing_is_written_outside_the_outputs(B, H, W):
    """16-KiB bands of 0xAB around every output and the workspace; the workspace comes in filled with NaN."""
    from texpose_amd import ops
    c = REF.one_call_case(21, B, H, W, "each", True, True)
    want = gpu_call(c)
    spec = dict(light=((B, 3, 5), torch.float32), count=((B,), torch.int32), rms=((B,), torch.float32), status=((B,), torch.int32),
                flags=((B,), torch.int32), rgb=((B, H, W, 3), torch.float32))
    out, checks = {}, []
    for k, (shape, dtype) in spec.items():
        out[k], check = banded(shape, dtype)
        checks.append(check)
    need = ops.photo_lighting_workspace(B, H, W, DEV).numel() * 8
    assert need == 512 * B * -(-H * W // 1024)
    ws, check = banded((need // 8,), torch.float64)
    checks.append(check)
    ws.fill_(float("nan"))
    got = ops.photo_lighting(*(cu(c[k]) for k in INPUTS), tau=c["tau"], light=cu(c["light_in"]), mask=cu(c["mask"]), workspace=ws, out=out)
    torch.cuda.synchronize()
    assert all(check() for check in checks)
    for k in spec:
        assert got[k] is out[k] and same_bits(got[k], want[k]), k
    rgb, check = banded((B, H, W, 3), torch.float32)             # in place: the rendering itself between bands
    rgb.copy_(cu(c["rgb"]))
    ops.photo_lighting(*(rgb if k == "rgb" else cu(c[k]) for k in INPUTS), tau=c["tau"], light=cu(c["light_in"]), mask=cu(c["mask"]), inplace=True)
    torch.cuda.synchronize()
    assert check() and same_bits(rgb, want["rgb"])


def test_two_calls_and_graph_replay_are_bit_equal():
    from texpose_amd import ops
    c = REF.one_call_case(31, 3, 33, 257, "map", True, True)
    d = {k: cu(c[k]) for k in INPUTS + ("light_in", "frame", "mask")}
    call = lambda **kw: ops.photo_lighting(*(d[k] for k in INPUTS), tau=0.5, light=d["light_in"], frame=d["frame"], mask=d["mask"], **kw)
    eager, again = call(), call()
    for k in eager:
        assert same_bits(eager[k], again[k]), k
    ws = ops.photo_lighting_workspace(3, 33, 257, DEV)
    cap = {k: torch.empty_like(v) for k, v in eager.items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(workspace=ws, out=cap)
    for _ in range(2):
        for v in cap.values():
            v.view(torch.uint8).fill_(0xAB)
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert same_bits(cap[k], eager[k]), k
    assert (eager["status"] == 0).all()


def test_bad_arguments_are_refused():
    from texpose_amd import _lib, ops
    c = REF.one_call_case(1, 2, 7, 65, "each", False, True)
    d = {k: cu(c[k]) for k in INPUTS}
    l = cu(c["light_in"])
    args = lambda **over: [over.get(k, d[k]) for k in INPUTS]
    poisoned = dict(light=torch.full((2, 3, 5), 7.0, device=DEV), count=torch.full((2,), 77, dtype=torch.int32, device=DEV))
    for kw in (dict(tau=0.0), dict(tau=float("nan")), dict(tau=0.5, gain_range=(0.0, 4.0)), dict(tau=0.5, gain_range=(0.25, 0.5)),
               dict(tau=0.5, gain_range=(0.25, float("inf"))), dict(tau=0.5, min_var=-1.0), dict(tau=0.5, light=l, out=dict(light=l))):
        with pytest.raises(_lib.TexposeLibraryError):
            ops.photo_lighting(*args(), **{**dict(out=poisoned), **kw})
    torch.cuda.synchronize()
    assert (poisoned["light"] == 7.0).all() and (poisoned["count"] == 77).all()          # nothing was launched
    im = d["image"]
    for bad in (lambda: ops.photo_lighting(*args(zbuf=d["zbuf"].double()), tau=0.5), lambda: ops.photo_lighting(*args(rgb=d["rgb"][:1]), tau=0.5),
                lambda: ops.photo_lighting(*args(face=d["face"].long()), tau=0.5), lambda: ops.photo_lighting(*args(face=d["face"][:, :5]), tau=0.5),
                lambda: ops.photo_lighting(*args(faces=d["faces"].long()), tau=0.5), lambda: ops.photo_lighting(*args(faces=d["faces"][:, :2]), tau=0.5),
                lambda: ops.photo_lighting(*args(faces=d["faces"][:0]), tau=0.5), lambda: ops.photo_lighting(*args(verts=d["verts"][:, :2]), tau=0.5),
                lambda: ops.photo_lighting(*args(pose=d["pose"][:1]), tau=0.5), lambda: ops.photo_lighting(*args(pose=d["pose"][:, :, :3]), tau=0.5),
                lambda: ops.photo_lighting(*args(image=im.permute(0, 3, 1, 2).contiguous()), tau=0.5),       # a [B,3,H,W] image
                lambda: ops.photo_lighting(*args(image=torch.cat([im, im[:1]])), tau=0.5),                    # Ft = 3 without a frame map
                lambda: ops.photo_lighting(*args(), tau=0.5, light=l[:, :, :4]), lambda: ops.photo_lighting(*args(), tau=0.5, light=l.double()),
                lambda: ops.photo_lighting(*args(), tau=0.5, mask=torch.ones(2, 7, 65, device=DEV)),          # a float mask
                lambda: ops.photo_lighting(*args(), tau=0.5, workspace=ops.photo_exposure_workspace(2, 7, 65, DEV)),      # half the bytes
                lambda: ops.photo_lighting(*args(), tau=0.5, gain_range=0.5),
                lambda: ops.photo_lighting(*args(), tau=0.5, inplace=True, out=dict(rgb=torch.empty_like(d["rgb"]))),
                lambda: ops.photo_lighting(*args(), tau=0.5, out=dict(status=torch.empty(2, device=DEV)))):
        with pytest.raises(ValueError):
            bad()


# ----------------------------------------------------------------------------- the loop
@functools.lru_cache(maxsize=None)
def golden():
    return REF.golden()


def run_loop(c, **kw):
    from texpose_amd import ops
    return ops.photo_align(cu(c["verts"]), cu(c["faces"]), cu(c["vcolor"]), cu(c["start"]), cu(c["K"]), cu(c["image"]), tau=0.5, iters=10,
                           damping=1e-6, **kw)


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("mesh", REF.MESHES)
def test_loop_recovers_the_pose_under_a_directional_light(mesh, noisy):
    """The four relit cases against the truth: at most twice the restatement's recorded errors on the same inputs plus 1e-3 deg and
    1e-3 mm (K19 and the numpy raster may differ on edge pixels), the light within 2e-3 of the restatement's."""
    from texpose_amd import ops
    c = REF.loop_inputs(mesh, noisy)
    key = "%.2f/%s/%s/lighting/" % (REF.STRENGTH, mesh, "noisy" if noisy else "clean")
    want_err, want_light = golden()[key + "err"], golden()[key + "light"]
    got = run_loop(c, lighting=True)
    assert set(got) == set(ops.PHOTO_ALIGN_KEYS) | {"light", "lighting_status", "lighting_flags"} and tuple(got["light"].shape) == (2, 3, 5)
    assert host(got["status"]).tolist() == [0, 0] and host(got["lighting_status"]).tolist() == [0, 0] and host(got["lighting_flags"]).tolist() == [0, 0]
    for b in range(2):
        re, te = PREF.pose_error(host(got["pose"])[b], c["P"][b])
        re_w, te_w = want_err[b]
        print("%s %s %d: kernel %.3g deg %.3g mm (%d pixels, rms %.5f, light %s) | restatement %.3g deg %.3g mm"
              % ("noisy" if noisy else "clean", mesh, b, re, te, int(got["inliers"][b]), float(got["rms"][b]), host(got["light"])[b].round(3).tolist(), re_w, te_w))
        assert re <= 2 * re_w + RE_FLOOR and te <= 2 * te_w + TE_FLOOR
        assert np.abs(host(got["light"])[b] - want_light[b]).max() <= 2e-3
        assert int(got["inliers"][b]) >= 300 and float(got["rms0"][b]) > float(got["rms"][b])


def test_without_the_keyword_every_loop_is_todays_and_both_keywords_are_refused():
    from texpose_amd import joint, multiview, ops, photo_align
    c = REF.loop_inputs("sphere", True)
    calls, raster = [], ops.scene.mesh_raster

    def counted(*a, **kw):
        calls.append(kw["face_ids"])
        return raster(*a, **kw)
    ops.scene.mesh_raster = counted
    try:
        today, off, exposed = run_loop(c), run_loop(c, lighting=False), run_loop(c, exposure=True)
        assert calls == [False] * 33
        on = run_loop(c, lighting=True)
        assert calls[33:] == [True] * 11                         # (the lighting passes ask for the face index, nothing else does)
    finally:
        ops.scene.mesh_raster = raster
    assert set(today) == set(off) == set(ops.PHOTO_ALIGN_KEYS) and set(exposed) == set(today) | {"gain", "bias", "exposure_status"}
    for k in today:
        assert same_bits(today[k], off[k]), k
    assert not same_bits(on["pose"], today["pose"]) and not same_bits(on["pose"], exposed["pose"])
    j = REF.joint_inputs()
    field, known = ops.mask_sdf(cu(j["cut"]), known=cu(j["known"])), cu(j["known"])
    jargs = (cu(j["verts"]), cu(j["faces"], torch.int32), cu(j["start"]), cu(j["K"]))
    jkw = dict(vcolor=cu(j["vcolor"]), sdf=field, image=cu(j["image"]), iters=3, masks=dict(photo=known))
    a, b = ops.joint_align(*jargs, **jkw), ops.joint_align(*jargs, lighting=False, **jkw)
    assert set(a) == set(b) and all(same_bits(a[k], b[k]) for k in a) and not any("light" in k for k in a)
    m = REF.multiview_inputs()
    margs = (cu(m["verts"]), cu(m["faces"], torch.int32), cu(m["model_start"]), cu(m["cam"]), cu(m["group"], torch.int32), cu(m["K"]))
    mkw = dict(vcolor=cu(m["vcolor"]), sdf=ops.mask_sdf(cu(m["cut"]), known=cu(m["known"])), image=cu(m["image"]), iters=3, masks=dict(photo=cu(m["known"])))
    a, b = ops.multiview_align(*margs, **mkw), ops.multiview_align(*margs, lighting=False, **mkw)
    assert set(a) == set(b) and all(same_bits(a[k], b[k]) for k in a) and not any("light" in k for k in a)
    both = dict(exposure=True, lighting=True)
    for call in (lambda: run_loop(c, **both), lambda: ops.joint_align(*jargs, **jkw, **both), lambda: ops.multiview_align(*margs, **mkw, **both),
                 lambda: photo_align.PhotoRefiner(c["verts"], c["faces"], c["vcolor"], c["H"], c["W"], DEV, **both),
                 lambda: joint.JointRefiner(j["verts"], j["faces"], j["H"], j["W"], DEV, vcolor=j["vcolor"], **both),
                 lambda: multiview.MultiViewRefiner(m["verts"], m["faces"], m["H"], m["W"], DEV, vcolor=m["vcolor"], **both)):
        with pytest.raises(ValueError, match="exclude each other"):
            call()
    with pytest.raises(ValueError, match="workspace"):           # the terms' own workspace is too small for the fit's records
        run_loop(c, lighting=True, workspace=ops.photo_align_workspace(2, c["H"], c["W"], DEV))
    mine = run_loop(c, lighting=True, workspace=ops.photo_align_workspace(2, c["H"], c["W"], DEV, lighting=True))
    assert all(same_bits(mine[k], on[k]) for k in on)


def test_the_refiner_repeats_and_replays_bit_equal():
    """PhotoRefiner.refine(lighting=True) as a whole: the loop by hand, a second call on the kept workspace, and a captured graph's
    replays give the same words on every output."""
    from texpose_amd import photo_align
    c = REF.loop_inputs("sphere", True)
    want = run_loop(c, lighting=True)
    refiner = photo_align.PhotoRefiner(c["verts"], c["faces"], c["vcolor"], c["H"], c["W"], DEV, tau=0.5, iters=10, damping=1e-6, lighting=True)
    start, K, image = cu(c["start"]), cu(c["K"][0]), cu(c["image"])
    for _ in range(2):                                           # (the second call reuses the workspace)
        r = refiner.refine(start, K, image)
        assert set(r) == set(want) and all(same_bits(r[k], want[k]) for k in want)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = refiner.refine(start, K, image)
    ws = refiner._workspace(2)
    for _ in range(2):
        for v in cap.values():
            v.view(torch.uint8).fill_(0xAB)
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k in want:
            assert same_bits(cap[k], want[k]), k


def test_with_a_pyramid_the_fit_runs_at_full_size():
    """pyramid= with lighting=True: every pass's fit sees the full-size planes (the rasteriser's face plane and the full-size photograph),
    in place, whatever its level, and surface_down then filters the LIT rendering; with every step at level 0 the loop is the one
    without a pyramid bit for bit.  (No restatement runs this combination: the end errors are printed, not held to a bar.)"""
    from texpose_amd import ops
    c = REF.loop_inputs("sphere", False)
    seen, fit, down = [], ops.refine.photo_lighting, ops.refine.surface_down

    def watched(*a, **kw):
        seen.append(("fit", tuple(a[2].shape), tuple(a[6].shape), kw["inplace"], a[4].data_ptr()))
        return fit(*a, **kw)

    def filtered(zbuf, rgb, *a, **kw):
        seen.append(("down", tuple(rgb.shape), rgb.data_ptr()))
        return down(zbuf, rgb, *a, **kw)
    ops.refine.photo_lighting, ops.refine.surface_down = watched, filtered
    try:
        got = run_loop(c, lighting=True, pyramid=(3, 7))
    finally:
        ops.refine.photo_lighting, ops.refine.surface_down = fit, down
    fits = [s for s in seen if s[0] == "fit"]
    assert [s[1:4] for s in fits] == [((2, c["H"], c["W"]), (2, c["H"], c["W"], 3), True)] * 11
    at = [k for k, s in enumerate(seen) if s[0] == "down"]
    assert len(at) == 3 and all(seen[k - 1][0] == "fit" and seen[k - 1][4] == seen[k][2] and seen[k][1] == (2, c["H"], c["W"], 3) for k in at)
    assert host(got["lighting_status"]).tolist() == [0, 0] and set(got) >= {"light", "lighting_status", "lighting_flags"}
    for b in range(2):
        print("pyramid (3, 7) sphere %d: %.4f deg %.4f mm" % ((b,) + PREF.pose_error(host(got["pose"])[b], c["P"][b])))
    flat, plain = run_loop(c, lighting=True, pyramid=(0, 10)), run_loop(c, lighting=True)
    assert all(same_bits(flat[k], plain[k]) for k in plain)


# ----------------------------------------------------------------------------- the joint and the multi-view loop
def test_joint_loop_under_a_directional_light():
    """K37's occluded joint case relit, silhouette + photometric through JointRefiner(lighting=True): within twice the restatement's
    recorded end errors plus the floors."""
    from texpose_amd import joint
    c, gold = REF.joint_inputs(), golden()
    refiner = joint.JointRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV, vcolor=c["vcolor"], lighting=True)
    got = refiner.refine(cu(c["start"]), cu(c["K"]), mask_or_sdf=cu(c["cut"]), known=cu(c["known"]), image=cu(c["image"]))
    assert {"photo_light", "photo_lighting_status", "photo_lighting_flags"} <= set(got) and not {"photo_gain", "photo_bias"} & set(got)
    assert (gold["joint/status"] == 0).all() and (gold["joint/lighting_status"] == 0).all()
    for b in range(2):
        re, te = PREF.pose_error(host(got.pose)[b], c["P"][b])
        re_w, te_w = gold["joint/err"][b]
        print("%s %d, %s: kernel %.3f deg / %.3f mm, status %d, light %s | restatement %.3f deg / %.3f mm"
              % (REF.JOINT_CASE[0], b, REF.JOINT_CASE[1], re, te, int(got.status[b]), host(got.photo_light)[b].round(3).tolist(), re_w, te_w))
        assert int(got.status[b]) == 0 and int(got.photo_lighting_status[b]) == 0
        assert re <= 2 * re_w + RE_FLOOR and te <= 2 * te_w + TE_FLOOR


def test_multiview_loop_under_a_directional_light():
    """One object seen by two cameras, each view under the lamp (one light per view): MultiViewRefiner(lighting=True) ends within twice
    the restatement's recorded error plus the floors."""
    from texpose_amd import multiview
    c, gold = REF.multiview_inputs(), golden()
    refiner = multiview.MultiViewRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV, vcolor=c["vcolor"], weights=(1.0, 100.0, 0.0), lighting=True)
    got = refiner.refine(cu(c["model_start"]), cu(c["cam"]), cu(c["group"], torch.int32), cu(c["K"]), mask_or_sdf=cu(c["cut"]), known=cu(c["known"]),
                         image=cu(c["image"]))
    assert tuple(got.photo_light.shape) == (2, 3, 5) and tuple(got.model.shape) == (1, 3, 4)
    re, te = PREF.pose_error(host(got.model)[0], c["model_true"])
    re_w, te_w = gold["multiview/err"]
    print("two views, %s, %s: kernel %.4f deg / %.4f mm, status %d, views %d | restatement %.4f deg / %.4f mm"
          % (*REF.JOINT_CASE, re, te, int(got.status[0]), int(got.views[0]), re_w, te_w))
    assert int(got.status[0]) == 0 and int(got.views[0]) == 2 and host(got.photo_lighting_status).tolist() == [0, 0] and int(gold["multiview/status"][0]) == 0
    assert re <= 2 * re_w + RE_FLOOR and te <= 2 * te_w + TE_FLOOR


# ----------------------------------------------------------------------------- the tool
# The bar's premise, measured once on the restatements (CPU, their own raster; too slow to run here): the scene below with the 8-bit
# photographs under REF.true_light(), from (2 deg, 5 mm).
TOOL_PREMISE = ("restatement's loop with the lighting fit, 8-bit photographs: ADD 5.19 / 5.15 / 5.16 mm -> 0.041 / 0.043 / 0.022 mm (ratios 0.004 .. 0.008; "
                "ambient right to 1e-2); with K37's exposure fit instead: -> 1.16 / 4.25 / 4.15 mm (ratios 0.22 .. 0.82); photo_ref's plain loop: "
                "-> 3.76 / 6.36 / 7.37 mm (ratios 0.73 .. 1.43): 8-bit quantisation and clipping leave the lighting loop far below a quarter, so "
                "the quarter stands")


def test_tool_refines_on_rgb_under_a_directional_light(tmp_path, capsys):
    """tools/refine_poses.py --rgb --lighting in a child process on K37's tool case relit: three 120 x 160 frames whose 8-bit rgb/ is the
    render under ambient + directional light + bias (the background takes the ambient form): ADD falls below a quarter of its start for
    every row.  --lighting without --rgb, and together with --exposure, exits with one message."""
    import test_gpu_photo_align as K30
    from texpose_amd import ops
    from texpose_amd.bop_scene import BopSceneWriter
    print("premise: " + TOOL_PREMISE)
    H, W, F, oid = K30.TOOL_H, K30.TOOL_W, K30.TOOL_FRAMES, 7
    verts, faces, colour8, K, gt, moved = K30._tool_scene()
    vcolor = colour8.astype(np.float32) / 255.0
    r = ops.mesh_raster(cu(verts), cu(faces), cu(gt), cu(K), H=H, W=W, vcolor=cu(vcolor), face_ids=True, normals=False)
    z, face = host(r["zbuf"]), host(r["face"])
    base = np.where((z > 0)[..., None], np.clip(host(r["rgb"]), 0.0, 1.0), 128.0 / 255.0).astype(np.float32)
    L = REF.true_light()
    lit = np.stack([REF.apply_ref(verts, faces, face[f], z[f], base[f], gt[f], L) for f in range(F)])
    lit = np.where((z > 0)[..., None], lit, L[:, 0] * base + L[:, 4])
    rgb8 = np.rint(np.clip(lit, 0.0, 1.0) * 255.0).astype(np.uint8)
    depth16 = np.where(z > 0, np.rint(z / 0.5), 0).astype(np.uint16)
    root, ply, est_csv, out_csv = str(tmp_path / "scene"), str(tmp_path / "obj_000007.ply"), str(tmp_path / "est.csv"), str(tmp_path / "refined.csv")
    K30._write_coloured_ply(ply, verts, faces, colour8)
    w = BopSceneWriter(root, K, 10.0, png_per_metre=2000)          # (it takes NeRF units at depth.scale 10: mm / 100)
    info = np.zeros((F, 10), np.int32)
    info[:, 0] = info[:, 1] = (z > 0).sum((1, 2))
    frames = []
    for f in range(F):
        pose = gt[f].copy()
        pose[:, 3] /= 100.0
        frames += w.add_views(pose[None], [oid], info[f][None, None], np.zeros((1, 1, H, W), np.uint8), np.zeros((1, 1, H, W), np.uint8),
                              rgb8[f][None], depth16[f][None])
    w.close()
    tool_path = os.path.join(REPO, "tools", "refine_poses.py")
    spec = importlib.util.spec_from_file_location("refine_poses_tool", tool_path)
    refine = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(refine)
    refine.write_rows(est_csv, [(1, frames[f], oid, 0.5, moved[f, :, :3], moved[f, :, 3], 0.0) for f in range(F)])
    common = [sys.executable, tool_path, "--scene", root, "--ply", ply, "--est", est_csv, "--out", out_csv, "--device", DEV]
    run = subprocess.run(common + ["--rgb", "--lighting"], capture_output=True, text=True, timeout=300)
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
        print("tool --rgb --lighting frame %d: ADD %.4f -> %.4f mm, translation %.4f -> %.4f mm" % (f, a0, a1, t0, t1))
        assert a1 < 0.25 * a0
    for flags, word in ((["--lighting"], "--lighting goes with --rgb"), (["--rgb", "--lighting", "--exposure"], "--lighting or --exposure, not both")):
        bad = subprocess.run(common + flags, capture_output=True, text=True, timeout=300)
        said = [ln for ln in bad.stderr.splitlines() if ln.startswith("refine_poses:")]
        assert bad.returncode != 0 and len(said) == 1 and word in said[0] and "Traceback" not in bad.stderr
