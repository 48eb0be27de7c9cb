"""K38 on the GPU: tp_image_down / tp_surface_down / tp_mask_down against the numpy restatement (tests/photo_pyramid_ref.py) bit for
bit on exactly the same planes, guard bands, reproducibility under repetition and graph replay, the zero-residual identity on K19's own
planes, ops.photo_align(pyramid=) against the restatement's loop (its figures are stored in tests/golden/photo_pyramid_loops.npz and
re-measured by tests/test_photo_pyramid_cpu.py) and against the truth, and tools/refine_poses.py --rgb --pyramid on a written BOP
scene."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import photo_exposure_ref as XREF
import photo_pyramid_ref as REF
import pnp_ref as PREF
from gn_ref import cu, host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RE_FLOOR, TE_FLOOR = 1e-3, 1e-3          # deg, mm: DESIGN section 19's floors for this geometry
BAND = 16384
SIZES = [(2, 2), (2, 3), (3, 2), (5, 7), (7, 65), (16, 16), (33, 257), (64, 80)]


def same_bits(a, b):
    a, b = (host(x) if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def down_all(d, **kw):
    """The three kernels on the planes of ``d`` (GPU tensors) -> dict(image, zbuf, rgb, mask)."""
    from texpose_amd import ops
    out = kw.get("out", {})
    s = ops.surface_down(d["zbuf"], d["rgb"], out={k: out[k] for k in ("zbuf", "rgb") if k in out} or None)
    return dict(image=ops.image_down(d["image"], out=out.get("image")), zbuf=s["zbuf"], rgb=s["rgb"], mask=ops.mask_down(d["mask"], out=out.get("mask")))


def ref_all(c):
    z, rgb = REF.surface_down_ref(c["zbuf"], c["rgb"])
    return dict(image=REF.image_down_ref(c["image"]), zbuf=z, rgb=rgb, mask=REF.mask_down_ref(c["mask"]))


def equal(got, want):
    for k in ("image", "zbuf", "rgb"):
        assert got[k].dtype == torch.float32 and REF.same(host(got[k]), want[k]), k
    assert got["mask"].dtype == torch.uint8 and np.array_equal(host(got["mask"]), want["mask"])


# ----------------------------------------------------------------------------- one call, exact inputs
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", SIZES)
def test_kernels_equal_the_restatement_bit_for_bit(H, W, N):
    """2 x 2 is the single output whose 16 taps all clamp; 7 x 65 and 33 x 257 take the guarded path and drop the last row or column;
    16 x 16 and 64 x 80 take the wide path.  Bits equal, NaN positions equal."""
    c = REF.one_down_case(1000 * H + 10 * W + N, N, H, W)
    want = ref_all(c)
    equal(down_all({k: cu(v) for k, v in c.items()}), want)
    assert want["zbuf"].shape == (N, H // 2, W // 2)
    if H * W >= 7 * 65:
        assert (want["zbuf"] > 0).sum() > 10 and (want["zbuf"] == -1).sum() > 10 and np.isnan(want["image"]).any() and 0 < want["mask"].mean() < 1


@pytest.mark.parametrize("which", ["zbuf", "rgb", "image", "mask"])
def test_a_misaligned_input_takes_the_guarded_path(which):
    """One input as a view 4 bytes (the mask: 1 byte) into its storage: 16 x 16 and 64 x 80 would take the wide path."""
    for H, W in ((16, 16), (64, 80)):
        c = REF.one_down_case(7 + H, 2, H, W)
        d = {k: cu(v) for k, v in c.items()}
        store = torch.empty(d[which].numel() + 1, dtype=d[which].dtype, device=DEV)
        view = store[1:].view(d[which].shape)
        view.copy_(d[which])
        assert view.data_ptr() % 16 == store.element_size() and view.is_contiguous()
        equal(down_all(dict(d, **{which: view})), ref_all(c))


def test_a_second_level_and_the_builders():
    from texpose_amd import ops
    c = REF.one_down_case(5, 2, 33, 66)
    d = {k: cu(v) for k, v in c.items()}
    images, masks = ops.image_pyramid(d["image"], 3), ops.mask_pyramid(d["mask"].bool(), 3)
    want_i, want_m = REF.image_pyramid_ref(c["image"], 3), REF.mask_pyramid_ref(c["mask"], 3)
    assert images[0] is d["image"] and [tuple(t.shape[1:3]) for t in images] == [(33, 66), (16, 33), (8, 16)]
    for l in range(3):
        assert REF.same(host(images[l]), want_i[l]) and np.array_equal(host(masks[l]) != 0, want_m[l] != 0), l
    z, rgb = c["zbuf"], c["rgb"]
    s = dict(zbuf=d["zbuf"], rgb=d["rgb"])
    for _ in range(2):
        s = ops.surface_down(s["zbuf"], s["rgb"])
        z, rgb = REF.surface_down_ref(z, rgb)
    assert REF.same(host(s["zbuf"]), z) and REF.same(host(s["rgb"]), rgb)
    with pytest.raises(ValueError):
        ops.image_pyramid(d["image"], 0)


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


def outputs_for(N, H, W, make):
    h, w = H // 2, W // 2
    return {k: make(shape, dtype) for k, (shape, dtype) in dict(image=((N, h, w, 3), torch.float32), zbuf=((N, h, w), torch.float32),
                                                                rgb=((N, h, w, 3), torch.float32), mask=((N, h, w), torch.uint8)).items()}


@pytest.mark.parametrize("N,H,W", [(1, 2, 2), (3, 5, 7), (3, 7, 65), (2, 16, 16), (3, 33, 257), (2, 64, 80)])
def test_nothing_is_written_outside_the_outputs(N, H, W):
    """16-KiB bands of 0xAB around every output."""
    c = REF.one_down_case(21, N, H, W)
    d = {k: cu(v) for k, v in c.items()}
    made = outputs_for(N, H, W, banded)
    out = {k: t for k, (t, _) in made.items()}
    got = down_all(d, out=out)
    torch.cuda.synchronize()
    assert all(check() for _, check in made.values())
    assert all(got[k] is out[k] for k in out)
    equal(got, ref_all(c))


def test_two_calls_and_graph_replay_are_bit_equal():
    N, H, W = 3, 33, 257
    c = REF.one_down_case(31, N, H, W)
    d = {k: cu(v) for k, v in c.items()}
    eager, again = down_all(d), down_all(d)
    for k in eager:
        assert same_bits(eager[k], again[k]), k
    cap = outputs_for(N, H, W, lambda shape, dtype: torch.empty(shape, dtype=dtype, device=DEV))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        down_all(d, out=cap)
    for _ in range(2):
        for v in cap.values():
            v.view(torch.uint8).fill_(0xAB)
        g.replay()
        torch.cuda.synchronize()
        for k in eager:
            assert same_bits(cap[k], eager[k]), k
    equal(eager, ref_all(c))


def test_bad_arguments_are_refused_and_launch_nothing():
    from texpose_amd import _lib, ops
    c = REF.one_down_case(1, 2, 8, 12)
    d = {k: cu(v) for k, v in c.items()}
    z1 = torch.full((2, 1, 12), 900.0, device=DEV)
    with pytest.raises(_lib.TexposeLibraryError, match="bad sizes"):            # H < 2
        ops.surface_down(z1, torch.zeros(2, 1, 12, 3, device=DEV))
    with pytest.raises(_lib.TexposeLibraryError, match="bad sizes"):            # W < 2
        ops.image_down(torch.zeros(2, 8, 1, 3, device=DEV))
    with pytest.raises(_lib.TexposeLibraryError, match="bad sizes"):
        ops.mask_down(torch.ones(2, 1, 12, dtype=torch.uint8, device=DEV))
    flat = torch.full((2 * 8 * 12 * 3,), 7.0, device=DEV)                        # an output inside its own input
    with pytest.raises(_lib.TexposeLibraryError, match="overlap"):
        ops.image_down(flat.view(2, 8, 12, 3), out=flat[:2 * 4 * 6 * 3].view(2, 4, 6, 3))
    with pytest.raises(_lib.TexposeLibraryError, match="overlap"):
        ops.surface_down(d["zbuf"], flat.view(2, 8, 12, 3), out=dict(zbuf=flat[8:8 + 2 * 4 * 6].view(2, 4, 6)))
    torch.cuda.synchronize()
    assert (flat == 7.0).all()                                   # nothing was launched
    for bad in (lambda: ops.image_down(d["image"].double()), lambda: ops.image_down(d["image"].permute(0, 3, 1, 2).contiguous()),
                lambda: ops.image_down(d["image"][:, :, ::2]), lambda: ops.surface_down(d["zbuf"], d["rgb"][:1]),
                lambda: ops.surface_down(d["zbuf"][0], d["rgb"][0]), lambda: ops.mask_down(d["zbuf"]),
                lambda: ops.image_down(d["image"], out=torch.empty(2, 4, 6, device=DEV)),
                lambda: ops.surface_down(d["zbuf"], d["rgb"], out=dict(zbuf=torch.empty(2, 4, 6, dtype=torch.float64, device=DEV))),
                lambda: ops.image_down(torch.empty(0, 8, 12, 3, device=DEV))):
        with pytest.raises(ValueError):
            bad()


# ----------------------------------------------------------------------------- the identity
def test_the_residual_at_the_true_pose_is_exactly_zero_on_the_device():
    """K19's own zbuf / rgb of the coloured torus composited over 0.5 is the photograph.  At levels 1 and 2 the evaluate_only step at
    the true pose returns rms == 0 exactly (the same 16 values through the same arithmetic on both sides), and inliers is the number
    of interior surface pixels of the coarse plane, counted on the host from the kernel's output."""
    from texpose_amd import ops
    c = REF.loop_inputs("torus", 3.0, False)
    H, W = c["H"], c["W"]
    pose, K = cu(c["P"]), cu(c["K"])
    r = ops.mesh_raster(cu(c["verts"]), cu(c["faces"]), pose, K, H=H, W=W, vcolor=cu(c["vcolor"]), face_ids=False, normals=False)
    photo = torch.where((r["zbuf"] > 0)[..., None], r["rgb"], torch.full_like(r["rgb"], 0.5)).contiguous()
    images = ops.image_pyramid(photo, 3)
    s = dict(zbuf=r["zbuf"], rgb=r["rgb"])
    for level in (1, 2):
        s = ops.surface_down(s["zbuf"], s["rgb"])
        ev = ops.photo_align_step(s["zbuf"], s["rgb"], pose, cu(REF.level_K(c["K"], level)), images[level], tau=0.5, evaluate_only=True)
        z = host(s["zbuf"])
        interior = ((z > 0) & np.isfinite(z))[:, 1:-1, 1:-1].reshape(2, -1).sum(1)
        print("level %d: inliers %s, interior surface pixels %s, rms %s" % (level, host(ev["inliers"]).tolist(), interior.tolist(), host(ev["rms"]).tolist()))
        assert (host(ev["rms"]) == 0.0).all() and host(ev["status"]).tolist() == [0, 0]
        assert np.array_equal(host(ev["inliers"]), interior) and (interior > (200 if level == 1 else 40)).all()
        on = z > 0
        assert same_bits(host(s["rgb"])[on], host(images[level])[on])


# ----------------------------------------------------------------------------- the loop
def run_loop(c, **kw):
    from texpose_amd import ops
    return ops.photo_align(cu(c["verts"]), cu(c["faces"]), cu(c["vcolor"]), cu(c["start"]), cu(c["K"]), cu(c["image"]), tau=0.5, iters=10,
                           damping=1e-6, **kw)


@pytest.mark.parametrize("mesh,f,noisy", REF.PINNED)
def test_loop_with_a_pyramid_recovers_the_pose(mesh, f, noisy):
    """The pinned 128 x 160 cases against the truth.  Section 20's bar: at most twice the restatement's errors on the same inputs plus
    the floors of 1e-3 deg and 1e-3 mm; kept pixels equal where the restatement counts no near-tie."""
    from texpose_amd import ops
    c, want = REF.loop_inputs(mesh, f, noisy), REF.golden_want(mesh, f, noisy)
    got = run_loop(c, pyramid=REF.PYRAMID)
    assert set(got) == set(ops.PHOTO_ALIGN_KEYS)
    figures = []
    for b in range(2):
        re, te = PREF.pose_error(host(got["pose"])[b], c["P"][b])
        re_w, te_w = PREF.pose_error(want["pose"][b], c["P"][b])
        figures.append((re, te, re_w, te_w))
        print("%s f = %g %s %d: kernel %.3g deg %.3g mm (%d pixels, %d at the first pass, rms %.5f) | restatement %.3g deg %.3g mm (%d pixels, %d, rms %.5f)"
              % (mesh, f, "noisy" if noisy else "clean", b, re, te, int(got["inliers"][b]), int(got["inliers0"][b]), float(got["rms"][b]), re_w, te_w,
                 want["inliers"][b], want["inliers0"][b], want["rms"][b]))
    assert (want["status"] == 0).all() and host(got["status"]).tolist() == [0, 0]
    for b, (re, te, re_w, te_w) in enumerate(figures):
        assert re <= 2 * re_w + RE_FLOOR and te <= 2 * te_w + TE_FLOOR
        if want["near_ties"][b] == 0:
            assert int(got["inliers0"][b]) == want["inliers0"][b] and int(got["inliers"][b]) == want["inliers"][b]


def test_without_a_pyramid_the_loop_is_todays():
    from texpose_amd import ops
    c = REF.loop_inputs("sphere", 2.0, True)
    today, off = run_loop(c), run_loop(c, pyramid=None)
    assert set(today) == set(off) == set(ops.PHOTO_ALIGN_KEYS)
    for k in today:
        assert same_bits(today[k], off[k]), k
    on, flat = run_loop(c, pyramid=REF.PYRAMID), run_loop(c, pyramid=(10,))
    assert not same_bits(on["pose"], today["pose"])
    for k in today:                                              # one level is the plain loop
        assert same_bits(flat[k], today[k]), k
    again = run_loop(c, pyramid=REF.PYRAMID)
    for k in on:
        assert same_bits(on[k], again[k]), k


def test_refiner_class_passes_the_option_on():
    from texpose_amd import photo_align
    c = REF.loop_inputs("sphere", 2.0, True)
    want = run_loop(c, pyramid=REF.PYRAMID)
    refiner = photo_align.PhotoRefiner(c["verts"], c["faces"], c["vcolor"], c["H"], c["W"], DEV, tau=0.5, iters=10, damping=1e-6, pyramid=REF.PYRAMID)
    for _ in range(2):                                           # (the second call reuses the workspace)
        r = refiner.refine(cu(c["start"]), cu(c["K"][0]), cu(c["image"]))
        assert same_bits(r.pose, want["pose"]) and same_bits(r.inliers, want["inliers"]) and same_bits(r.rms0, want["rms0"])


def test_mask_cull_and_texture_routes_compose():
    """A mask that hides nothing the loop uses leaves the result alone (its pyramid is built and used); cull=True renders the same bits."""
    c = REF.loop_inputs("sphere", 2.0, True)
    want = run_loop(c, pyramid=REF.PYRAMID)
    everything = torch.ones(2, c["H"], c["W"], dtype=torch.uint8, device=DEV)
    for kw in (dict(mask=everything), dict(mask=everything.bool()), dict(cull=True)):
        got = run_loop(c, pyramid=REF.PYRAMID, **kw)
        for k in want:
            assert same_bits(got[k], want[k]), (k, sorted(kw))
    half = everything.clone()
    half[:, :, :c["W"] // 2] = 0
    assert int(run_loop(c, pyramid=REF.PYRAMID, mask=half)["inliers"].sum()) < int(want["inliers"].sum())


def test_exposure_composes_with_the_pyramid():
    """The sphere f = 2 sigma 0.02 case under section 27's gain and bias: premise measured on the restatement (its docstring): it ends
    at 0.025 deg / 0.031 mm.  Bar: below a quarter of the start, and within twice the restatement plus the floors."""
    c, want = REF.loop_inputs(*REF.EXPOSED, exposed=True), REF.golden_want(*REF.EXPOSED, exposure=True)
    got = run_loop(c, pyramid=REF.PYRAMID, exposure=True)
    assert {"gain", "bias", "exposure_status"} <= set(got) and host(got["exposure_status"]).tolist() == [0, 0]
    for b in range(2):
        re0, te0 = PREF.pose_error(c["start"][b], c["P"][b])
        re, te = PREF.pose_error(host(got["pose"])[b], c["P"][b])
        re_w, te_w = PREF.pose_error(want["pose"][b], c["P"][b])
        print("exposure + pyramid %d: kernel %.4f deg %.4f mm, gain %s | restatement %.4f deg %.4f mm" % (b, re, te, host(got["gain"])[b].round(4), re_w, te_w))
        assert re <= 0.25 * re0 and te <= 0.25 * te0
        assert re <= 2 * re_w + RE_FLOOR and te <= 2 * te_w + TE_FLOOR
        assert np.abs(host(got["gain"])[b] - XREF.EXPOSURE_GAIN).max() <= 5e-3


# ----------------------------------------------------------------------------- the tool
def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(REPO, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_refines_on_rgb_with_a_pyramid(tmp_path, capsys):
    """tools/refine_poses.py --rgb --pyramid 4 3 3 in a child process on three 128 x 160 frames whose 8-bit rgb/ is the render of the
    f = 2 sphere: ADD falls below a quarter of its start for every row, while the same command without --pyramid leaves frames 1 and
    2 above it (the premise, measured on the restatement: REF.TOOL_PREMISE)."""
    import test_gpu_photo_align as K30
    from texpose_amd import ops
    from texpose_amd.bop_scene import BopSceneWriter
    s = REF.tool_scene()
    H, W, F, oid = s["H"], s["W"], 3, 7
    vcolor, K = s["colour8"].astype(np.float32) / 255.0, np.tile(s["K"], (3, 1, 1))
    r = ops.mesh_raster(cu(s["verts"]), cu(s["faces"]), cu(s["gt"]), cu(K), H=H, W=W, vcolor=cu(vcolor), face_ids=False, normals=False)
    z = host(r["zbuf"])
    rgb8 = np.rint(np.where((z > 0)[..., None], np.clip(host(r["rgb"]), 0.0, 1.0), 128.0 / 255.0) * 255.0).astype(np.uint8)
    depth16 = np.where(z > 0, np.rint(z / 0.5), 0).astype(np.uint16)
    root, ply, est_csv = str(tmp_path / "scene"), str(tmp_path / "obj_000007.ply"), str(tmp_path / "est.csv")
    K30._write_coloured_ply(ply, s["verts"], s["faces"], s["colour8"])
    w = BopSceneWriter(root, s["K"], 10.0, png_per_metre=2000)          # (it takes NeRF units at depth.scale 10: mm / 100)
    info = np.zeros((F, 10), np.int32)
    info[:, 0] = info[:, 1] = (z > 0).sum((1, 2))
    frames = []
    for f in range(F):
        pose = s["gt"][f].copy()
        pose[:, 3] /= 100.0
        frames += w.add_views(pose[None], [oid], info[f][None, None], np.zeros((1, 1, H, W), np.uint8), np.zeros((1, 1, H, W), np.uint8),
                              rgb8[f][None], depth16[f][None])
    w.close()
    refine, errors = _load_tool("refine_poses"), _load_tool("pose_errors")
    start = s["start"].astype(np.float64)
    refine.write_rows(est_csv, [(1, frames[f], oid, 0.5, start[f, :, :3], start[f, :, 3], 0.0) for f in range(F)])
    tool_path = os.path.join(REPO, "tools", "refine_poses.py")
    common = [sys.executable, tool_path, "--scene", root, "--ply", ply, "--est", est_csv, "--device", DEV]
    ratios, figures = {}, ["premise: " + REF.TOOL_PREMISE]
    for name, extra in (("pyramid", ["--rgb", "--pyramid", "4", "3", "3"]), ("plain", ["--rgb"])):
        out_csv = str(tmp_path / (name + ".csv"))
        run = subprocess.run(common + ["--out", out_csv] + extra, capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stdout + run.stderr
        assert "3 refined" in run.stdout
        before = errors.main(["--gt", root, "--est", est_csv, "--ply", "%d=%s" % (oid, ply)])[oid]
        after = errors.main(["--gt", root, "--est", out_csv, "--ply", "%d=%s" % (oid, ply)])[oid]
        capsys.readouterr()
        assert before["frames"] == after["frames"] == sorted(frames) and not after["missing"]
        ratios[name] = [a1 / a0 for a0, a1 in zip(before["errors"]["add"], after["errors"]["add"])]
        for fr, a0, a1 in zip(after["frames"], before["errors"]["add"], after["errors"]["add"]):
            figures.append("tool --rgb %s frame %d: ADD %.4f -> %.4f mm" % (name, fr, a0, a1))
    print("\n".join(figures))                                       # (after the last capsys.readouterr(), which drops what pose_errors printed)
    assert max(ratios["pyramid"]) < 0.25
    assert min(ratios["plain"][1:]) >= 0.25
    for extra, said_what in ((["--pyramid", "4", "3", "3"], "--pyramid goes with --rgb"), (["--rgb", "--pyramid", "4", "3", "2"], "--pyramid")):
        bad = subprocess.run(common + ["--out", str(tmp_path / "bad.csv")] + extra, capture_output=True, text=True, timeout=300)
        said = [ln for ln in bad.stderr.splitlines() if ln.startswith("refine_poses:")]
        assert bad.returncode != 0 and len(said) == 1 and said_what in said[0] and "Traceback" not in bad.stderr
