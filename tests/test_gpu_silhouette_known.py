"""K31c and K32 on the GPU: tp_mask_sdf_known against the brute force over all pixel pairs and, with every pixel
known, against tp_mask_sdf bit for bit; tp_mask_known_from_others against the whole-array restatement, exactly; one step of the
UNCHANGED tp_silhouette_align_step on a field rich in NaNs against the numpy restatement; the loop on the eight occluded cases through
SilhouetteRefiner.refine(known=); repeatability and graph replay; refused arguments; tools/refine_poses.py --occluders / --known on a
written BOP scene of two instances.  The restatement is tests/occlusion_ref.py; its own figures are printed by
tests/test_silhouette_known_cpu.py."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import occlusion_ref as OREF
import pnp_ref as PREF
import silhouette_ref as REF
from gn_ref import compare, cu, host

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    a = host(a) if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------- the field
def field_cases(rs, H, W):
    """(mask, known) [9,H,W] uint8 each: the 50 % random mask with all known / all unknown / 30 % unknown (the values 7 and 255 as
    "known") / the last row and column unknown; a band of unknown columns (rows where W is 1) separating the only set pixels from the
    only clear ones; the empty, the full and the one-corner-pixel mask with 30 % unknown; the corner pixel with the last row and
    column unknown, which hides it."""
    rand = ((rs.uniform(size=(H, W)) < 0.5) * 255).astype(np.uint8)
    some = ((rs.uniform(size=(H, W)) >= 0.3) * rs.choice(np.array([7, 255], np.uint8), (H, W))).astype(np.uint8)
    edge = np.ones((H, W), np.uint8)
    edge[H - 1, :] = 0
    edge[:, W - 1] = 0
    corner = np.zeros((H, W), np.uint8)
    corner[H - 1, 0] = 255
    split, band = np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)
    if W > 1:
        split[:, :W // 2] = 1
        band[:, W // 2 - (W > 3):W // 2 + 1] = 0                 # (the last set column and the first clear one where W > 3)
    else:
        split[:H // 2, :] = 1
        band[H // 2 - (H > 3):H // 2 + 1, :] = 0
    empty, full, ones = np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8), np.ones((H, W), np.uint8)
    masks = np.stack([rand, rand, rand, rand, split, empty, full, corner, corner])
    known = np.stack([ones, 0 * ones, some, edge, band, some, some, some, edge])
    return masks, known


@functools.lru_cache(maxsize=None)
def field_reference(H, W):
    """The cases of a shape with their brute-force integers and field, computed once."""
    masks, known = field_cases(np.random.RandomState(H * 3000 + W), H, W)
    d2 = [OREF.d2_known_ref(m, k) for m, k in zip(masks, known)]
    want = np.stack([OREF.field_from_d2(m, k, a, b) for (m, k), (a, b) in zip(zip(masks, known), d2)])
    pick = np.stack([np.where(m != 0, b, a) for m, (a, b) in zip(masks, d2)])          # the integer the pixel's class asks for
    for a in (masks, known, want, pick):
        a.setflags(write=False)
    return masks, known, want, pick


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (7, 1), (2, 5), (3, 3), (16, 16), (33, 257), (64, 80), (5, 1030)])
def test_known_field_equals_the_brute_force(H, W):
    """F = 1 on every case, one F = 3 stack, a poisoned workspace, a bool ``known`` and ``out=``.  NaN exactly on the unknown pixels;
    elsewhere round((|sdf| + 0.5)^2) is the brute force's integer over the SET / CLEAR pixels (the rounding of sqrtf and of the
    subtraction moves the square by at most 2.4e-7 x 2 d2 < 0.26 at these sizes), the sentinel H^2 + W^2 included; sdf within 1 ulp of
    the restatement's; the sign is the mask's; with every pixel known the bits are tp_mask_sdf's."""
    from texpose_amd import ops
    masks, known, want, d2 = field_reference(H, W)
    assert np.isnan(want[1]).all() and (known[0] != 0).all() and np.isnan(want[4]).any() and (H * W == 1 or not np.isnan(want[4]).all())
    assert (d2[8][known[8] != 0] == H * H + W * W).all()         # the hidden corner pixel: no set pixel is left
    ws = ops.mask_sdf_workspace(3, H, W, DEV)
    ws.view(torch.uint8).fill_(0xAB)                             # (needs no clearing)
    runs = [([k], ops.mask_sdf(cu(masks[k:k + 1]), known=cu(known[k:k + 1]))) for k in range(len(masks))]
    runs += [([2, 4, 8], ops.mask_sdf(cu(masks[[2, 4, 8]]), known=cu(known[[2, 4, 8]]), workspace=ws))]
    runs += [([3], ops.mask_sdf(cu(masks[3]), known=cu(known[3] != 0))[None])]          # one [H,W] plane, a bool known
    out = torch.full((3, H, W), 7.0, device=DEV)
    assert ops.mask_sdf(cu(masks[[2, 4, 8]]), out=out, workspace=ws, known=cu(known[[2, 4, 8]])) is out
    runs += [([2, 4, 8], out)]
    for pick, got in runs:
        got = host(got)
        k, m = known[pick] != 0, masks[pick] != 0
        assert got.dtype == np.float32 and got.shape == (len(pick), H, W)
        assert np.array_equal(np.isnan(got), ~k) and np.isfinite(got[k]).all(), pick
        assert np.array_equal(np.rint((np.abs(got[k].astype(np.float64)) + 0.5) ** 2).astype(np.int64), d2[pick][k]), pick
        assert np.array_equal(got[k] < 0, m[k])
        assert (np.abs(got[k] - want[pick][k]) <= np.spacing(np.abs(want[pick][k]))).all(), pick
    plain = ops.mask_sdf(cu(masks[[0, 5, 6, 7]]))
    for ones in (np.ones((4, H, W), np.uint8), np.full((4, H, W), 255, np.uint8)):
        assert np.array_equal(bits(ops.mask_sdf(cu(masks[[0, 5, 6, 7]]), known=cu(ones))), bits(plain))


# ----------------------------------------------------------------------------- who hides whom
@pytest.mark.parametrize("H,W", [(2, 5), (33, 257), (64, 80)])
def test_known_from_others_equals_the_restatement(H, W):
    """N in {1, 2, 3, 9} x bands 0, 1, 2, 2.5 on the kernel's own fields of random discs, then with NaN / Inf planted in a plane;
    ``out=`` poisoned beforehand.  64 x 80 takes the 16-byte route, the other two (H W no multiple of 4) the scalar one."""
    from texpose_amd import ops
    rs = np.random.RandomState(H + W)
    fields = ops.mask_sdf(cu(REF.discs(rs, (9, H, W)).astype(np.uint8)))
    planted = host(fields).copy()
    flat = planted[1].reshape(-1)
    flat[rs.randint(0, H * W, max(3, H * W // 50))] = np.array([np.nan, np.inf, -np.inf], np.float32)[rs.randint(0, 3, max(3, H * W // 50))]
    flat[:3] = [np.nan, np.inf, -np.inf]
    unknown = 0
    for sdf in (host(fields), planted):
        for N in (1, 2, 3, 9):
            for band in (0.0, 1.0, 2.0, 2.5):
                want = OREF.known_from_others_ref(sdf[:N], band)
                out = torch.full((N, H, W), 0xAB, dtype=torch.uint8, device=DEV)
                got = ops.mask_known_from_others(cu(sdf[:N]), band, out=out)
                assert got is out and np.array_equal(host(got), want), (N, band)
                assert N > 1 or (want == 1).all()
                unknown += int((want == 0).sum())
    assert unknown > 0
    got = ops.mask_known_from_others(fields[:3])                 # band_px = 0 and a fresh tensor
    assert got.dtype == torch.uint8 and np.array_equal(host(got), OREF.known_from_others_ref(host(fields[:3]), 0.0))
    if H * W % 4 == 0:                                           # a plane stack at an address that is no multiple of 16: the scalar route
        shifted = torch.empty(3 * H * W + 1, device=DEV)[1:].view(3, H, W).copy_(fields[:3])
        assert shifted.data_ptr() % 16 and torch.equal(ops.mask_known_from_others(shifted, 1.0), ops.mask_known_from_others(fields[:3], 1.0))


# ----------------------------------------------------------------------------- one step of the unchanged K31b on a field with NaNs
@pytest.mark.parametrize("B,H,W,frames,with_mask", [(3, 33, 257, "each", False), (3, 64, 80, "map", True), (1, 16, 16, "one", False)])
def test_step_on_a_known_field_equals_the_restatement(B, H, W, frames, with_mask):
    """The measured planes of silhouette_ref.one_step_case with a random 20 % of their pixels unknown: the kernel's field has the
    restatement's bits, and ops.silhouette_align_step on it meets gn_ref.compare's bars against step_ref on the restatement's field,
    inter and uni equal: K31b needs no change for NaN-rich fields."""
    from texpose_amd import ops
    c = REF.one_step_case(77 + H, B, H, W, frames, with_mask, "measured")
    known = (np.random.RandomState(H).uniform(size=c["measured"].shape) >= 0.2).astype(np.uint8)
    c["sdf"] = OREF.sdf_known_ref(c["measured"], known)
    field = ops.mask_sdf(cu(c["measured"]), known=cu(known))
    assert np.array_equal(bits(field), bits(c["sdf"])) and np.isnan(c["sdf"]).mean() > 0.15
    plain = REF.step_ref(c["zbuf"], c["pose"], c["K"], REF.sdf_ref(c["measured"]), c["tau"], 1e-6, c["frame"], c["mask"])
    for evaluate_only in (False, True):
        want = REF.step_ref(c["zbuf"], c["pose"], c["K"], c["sdf"], c["tau"], 1e-6, c["frame"], c["mask"], evaluate_only=evaluate_only)
        got = ops.silhouette_align_step(cu(c["zbuf"]), cu(c["pose"]), cu(c["K"]), field, tau_px=c["tau"], frame=cu(c["frame"]), mask=cu(c["mask"]),
                                        evaluate_only=evaluate_only)
        compare(got, want, c["pose"])
        assert np.array_equal(host(got["inter"]), want["inter"]) and np.array_equal(host(got["uni"]), want["uni"])
    assert (want["inliers"] < plain["inliers"]).any() and (want["inter"] < plain["inter"]).any()          # (the NaNs dropped rows and pixels)
    if H * W >= 64 * 80:
        assert want["inliers"].sum() > 30


# ----------------------------------------------------------------------------- the loop
def refiner_of(c):
    from texpose_amd import silhouette
    return silhouette.SilhouetteRefiner(c["verts"], c["faces"], c["H"], c["W"], DEV, tau_px=4.0, iters=10, damping=1e-6)


def visible_iou_of(c, pose):
    """The visible IoU of K19's rendering at ``pose`` [2,3,4] against the cut masks over the known pixels, by the restatement."""
    from texpose_amd import ops
    z = host(ops.mesh_raster(cu(c["verts"]), cu(c["faces"], torch.int32), cu(pose), cu(c["K"]), H=c["H"], W=c["W"], face_ids=False, normals=False)["zbuf"])
    return np.array([OREF.visible_iou_ref(z[b], c["cut"][b], c["known"][b])[0] for b in range(2)])


@pytest.mark.parametrize("kind", OREF.ASSERTED)
@pytest.mark.parametrize("name", REF.MESHES)
def test_loop_closes_the_visible_outline(name, kind):
    """The eight occluded cases of the table through SilhouetteRefiner.refine(known=): status 0, the last rms at most 0.6 of the first,
    the visible IoU does not fall and ends >= 0.98 and above what today's field of the same cut mask reaches; iou0_visible is the
    restatement's visible IoU of its own raster at the start pose, exactly.  The pose is printed, not asserted: it is chaotic where
    little is visible."""
    from texpose_amd import ops
    c = OREF.occluded_inputs(name, kind)
    refiner = refiner_of(c)
    got = refiner.refine(cu(c["start"]), cu(c["K"]), cu(c["cut"]), known=cu(c["known"]))
    naive = refiner.refine(cu(c["start"]), cu(c["K"]), cu(c["cut"]))
    assert set(got) == set(ops.SILHOUETTE_ALIGN_KEYS) | {"iou_visible", "iou0_visible"} and set(naive) == set(ops.SILHOUETTE_ALIGN_KEYS)
    assert got.iou_visible.dtype == torch.float32 and got.iou0_visible.shape == (2,)
    naive_visible = visible_iou_of(c, host(naive.pose))
    rows = []
    for b in range(2):
        re, te = PREF.pose_error(host(got.pose)[b], c["P"][b])
        re_n, te_n = PREF.pose_error(host(naive.pose)[b], c["P"][b])
        rows.append(dict(status=int(got.status[b]), rms0=float(got.rms0[b]), rms=float(got.rms[b]), viou0=float(got.iou0_visible[b]),
                         viou=float(got.iou_visible[b])))
        print("%s %d, %s (%.2f visible): known field rms %.4f -> %.4f, visible IoU %.4f -> %.4f, %.3f deg %.3f mm, status %d | today's field visible "
              "IoU %.4f, %.3f deg %.3f mm, status %d" % (name, b, kind, c["visible"][b], rows[b]["rms0"], rows[b]["rms"], rows[b]["viou0"],
                                                       rows[b]["viou"], re, te, rows[b]["status"], naive_visible[b], re_n, te_n, int(naive.status[b])))
    assert np.array_equal(bits(got.iou_visible), bits(visible_iou_of(c, host(got.pose))))          # (the wrapper's count against the masks')
    for b in range(2):
        z0 = REF.render_ref(name, c["start"][b], c["K"][b], c["H"], c["W"])
        assert bits(got.iou0_visible[b:b + 1])[0] == bits(OREF.visible_iou_ref(z0, c["cut"][b], c["known"][b])[0])
        assert rows[b]["status"] == 0
        assert rows[b]["rms"] <= 0.6 * rows[b]["rms0"]
        assert rows[b]["viou"] >= rows[b]["viou0"] and rows[b]["viou"] >= 0.98
        assert rows[b]["viou"] > naive_visible[b] or np.isnan(naive_visible[b])


# ----------------------------------------------------------------------------- repeatability
def test_two_runs_and_graph_replay_are_bit_equal():
    from texpose_amd import ops
    c = OREF.occluded_inputs("bent sphere", "corner disc")
    refiner = refiner_of(c)
    start, K, cut, known = cu(c["start"]), cu(c["K"]), cu(c["cut"]), cu(c["known"])
    every = torch.cat([cut, cu(c["occ"].astype(np.uint8))])      # four "instances" of one frame
    first, again = (refiner.refine(start, K, cut, known=known) for _ in range(2))
    field, others = ops.mask_sdf(cut, known=known), ops.mask_known_from_others(ops.mask_sdf(every), 1.0)
    assert set(first) == set(again) and len(first) == 10
    for k in first:
        assert torch.equal(first[k].view(torch.uint8), again[k].view(torch.uint8)), k
    assert np.array_equal(bits(field), bits(ops.mask_sdf(cut, known=known))) and torch.equal(others, ops.mask_known_from_others(ops.mask_sdf(every), 1.0))
    assert np.array_equal(bits(field), bits(OREF.sdf_known_ref(c["cut"], c["known"]))) and (others == 0).any() and (others == 1).any()
    ws = ops.mask_sdf_workspace(4, c["H"], c["W"], DEV)
    plain = ops.mask_sdf(every)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = dict(refiner.refine(start, K, cut, known=known))
        cap["field"] = ops.mask_sdf(cut, known=known, workspace=ws)
        cap["others"] = ops.mask_known_from_others(plain, 1.0)
    want = dict(first, field=field, others=others)
    for _ in range(2):
        for v in cap.values():
            v.view(torch.uint8).fill_(0xAB)
        ws.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(cap[k].view(torch.uint8), want[k].view(torch.uint8)), k
    assert (first["status"] == 0).all()
    # without the flag: today's launches, keys and bits
    sdf = ops.mask_sdf(cut, known=known)
    a = ops.silhouette_align(cu(c["verts"]), cu(c["faces"], torch.int32), start, K, sdf, tau_px=4.0, iters=10, damping=1e-6)
    b = ops.silhouette_align(cu(c["verts"]), cu(c["faces"], torch.int32), start, K, sdf, tau_px=4.0, iters=10, damping=1e-6, visible_iou=True)
    assert tuple(a) == ops.SILHOUETTE_ALIGN_KEYS and tuple(b) == ops.SILHOUETTE_ALIGN_KEYS + ("iou_visible", "iou0_visible")
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) and torch.equal(a[k].view(torch.uint8), first[k].view(torch.uint8)), k
    # a frame map picks the plane the step picks, out-of-range entries clamped
    fr = cu([5, -2], torch.int32)
    m = ops.silhouette_align(cu(c["verts"]), cu(c["faces"], torch.int32), start, K, sdf, iters=0, frame=fr, visible_iou=True)
    swapped = ops.silhouette_align(cu(c["verts"]), cu(c["faces"], torch.int32), start, K, sdf[[1, 0]], iters=0, visible_iou=True)
    assert np.array_equal(bits(m["iou_visible"]), bits(swapped["iou_visible"])) and np.array_equal(bits(m["iou0_visible"]), bits(m["iou_visible"]))
    # nothing known: no pixel left to compare, NaN
    none = ops.silhouette_align(cu(c["verts"]), cu(c["faces"], torch.int32), start, K, torch.full_like(sdf, float("nan")), iters=0, visible_iou=True)
    assert torch.isnan(none["iou_visible"]).all() and (none["status"] == 1).all()


def test_bad_arguments_are_refused():
    from texpose_amd import _lib, ops
    c = OREF.occluded_inputs("bent sphere", "corner disc")
    cut, known = cu(c["cut"]), cu(c["known"])
    for bad in (known.float(), known[:, :-1].contiguous(), known[:1], known.cpu(), known.to(torch.int32)):
        with pytest.raises(ValueError, match="known"):
            ops.mask_sdf(cut, known=bad)
    refiner = refiner_of(c)
    with pytest.raises(ValueError, match="known"):
        refiner.refine(cu(c["start"]), cu(c["K"]), ops.mask_sdf(cut), known=known)          # a field together with known
    sdf = ops.mask_sdf(cut)
    for band in (-1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.TexposeLibraryError, match="band_px"):
            ops.mask_known_from_others(sdf, band)
    for bad in (torch.empty(sdf.shape, device=DEV), torch.empty((2, 64, 79), dtype=torch.uint8, device=DEV), torch.empty(sdf.shape, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="out"):
            ops.mask_known_from_others(sdf, 1.0, out=bad)
    with pytest.raises(ValueError):
        ops.mask_known_from_others(cut)                          # masks, not fields
    with pytest.raises(ValueError):
        ops.mask_known_from_others(sdf[0])                       # one [H,W] plane: N is not optional


# ----------------------------------------------------------------------------- the tool
TOOL_H, TOOL_W, TOOL_FRAMES, TOOL_OID, TOOL_OCCLUDER_OID = 120, 160, 3, 7, 9


def tool_scene():
    """Three poses of the bent sphere about 900 mm away and, per frame, the pose of the unbent sphere 700 mm away, down and to the right
    of it in the image: it hides the lower right of the target.  -> K, gt [3,3,4], occluder poses [3,3,4], estimates (2 deg, 5 mm off)."""
    K = PREF.end_to_end_inputs("sphere")["K"].copy()
    K[:2] *= TOOL_H / 64.0
    rs = np.random.RandomState(8)
    gt = []
    for _ in range(TOOL_FRAMES):
        q, _r = np.linalg.qr(rs.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] *= -1
        gt.append(np.concatenate([q, rs.uniform(-15, 15, (3, 1)) + [[0.0], [0.0], [900.0]]], 1))
    gt = np.stack(gt).astype(np.float32)
    front = np.tile(np.eye(3, 4, dtype=np.float32), (TOOL_FRAMES, 1, 1))
    front[:, :, 3] = gt[:, :, 3] * np.float32(700.0 / 900.0) + np.array([55.0, 45.0, 0.0], np.float32)
    moved = REF.perturbed(gt, np.random.RandomState(5), angle_deg=2.0).astype(np.float64)
    for f in range(TOOL_FRAMES):                                 # (2 deg, 5 mm)
        d = moved[f, :, 3] - gt[f, :, 3]
        moved[f, :, 3] = gt[f, :, 3] + d * 5.0 / np.linalg.norm(d)
    return K, gt, front, moved


def _write_ply(path, verts, faces):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(verts), len(faces)))
        for p in verts:
            f.write("%r %r %r\n" % tuple(float(v) for v in p))
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(int(v) for v in t))


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(REPO, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_tool_refines_an_occluded_object_with_occluders_and_with_known(tmp_path, capsys):
    """A scene of two instances that holds only masks: the bent sphere and, in front of it, a sphere that hides its lower right.
    --silhouette --occluders writes a CSV tools/pose_errors.py reads, all rows status 0, the mean visible IoU it prints rises and ends
    above the mean IoU the same run without --occluders reaches; --known DIR with the planes that run built gives the same rows; the
    option conflicts and a missing file each exit with one message."""
    from PIL import Image
    from texpose_amd import ops
    from texpose_amd.bop_scene import BopSceneWriter
    H, W, F, oid = TOOL_H, TOOL_W, TOOL_FRAMES, TOOL_OID
    verts, faces = REF.mesh_of("bent sphere")
    K, gt, front, moved = tool_scene()
    raster = lambda v, fc, P: host(ops.mesh_raster(cu(v), cu(fc), cu(P), cu(K), H=H, W=W, face_ids=False, normals=False)["zbuf"]) > 0
    whole, occ = raster(verts, faces, gt), raster(*REF.mesh_of("sphere"), front)
    visib = np.stack([whole & ~occ, occ], 1).astype(np.uint8) * np.uint8(255)          # [F,2,H,W]: the target behind, the occluder in front
    full = np.stack([whole, occ], 1).astype(np.uint8) * np.uint8(255)
    share = visib[:, 0].astype(bool).sum((1, 2)) / whole.sum((1, 2))
    assert (share > 0.5).all() and (share < 0.95).all(), share   # (the numpy raster gives 0.89, 0.82, 0.84)
    root, ply, est_csv = str(tmp_path / "scene"), str(tmp_path / "obj_000007.ply"), str(tmp_path / "est.csv")
    _write_ply(ply, verts, faces)
    w = BopSceneWriter(root, K, 10.0, png_per_metre=2000)          # (it takes NeRF units at depth.scale 10: mm / 100)
    info = np.zeros((F, 2, 10), np.int32)
    info[:, :, 0], info[:, :, 1] = full.astype(bool).sum((2, 3)), visib.astype(bool).sum((2, 3))
    frames = []
    for f in range(F):
        pose = gt[f].copy()
        pose[:, 3] /= 100.0
        frames += w.add_views(pose[None], [oid, TOOL_OCCLUDER_OID], info[f][None], full[f][None], visib[f][None], np.zeros((1, H, W, 3), np.uint8),
                              np.zeros((1, H, W), np.uint16))
    w.close()
    refine, errors = _load_tool("refine_poses"), _load_tool("pose_errors")
    refine.write_rows(est_csv, [(1, frames[f], oid, 0.5, moved[f, :, :3], moved[f, :, 3], 0.0) for f in range(F)])
    common = ["--scene", root, "--ply", "%d=%s" % (oid, ply), "--est", est_csv, "--device", DEV]

    def run(out, *options):
        refine.main(common + ["--out", str(tmp_path / out)] + list(options))
        said = capsys.readouterr().out
        figures = {}
        for key in ("mean IoU", "mean visible IoU"):
            line = [ln for ln in said.splitlines() if key in ln]
            assert len(line) <= 1
            if line:
                figures[key] = tuple(float(v) for v in line[0].split(key)[1].split("->"))
        return said, figures

    said, plain = run("plain.csv", "--silhouette")
    assert set(plain) == {"mean IoU"}                            # (without the new options: today's lines)
    said, with_occ = run("occluders.csv", "--silhouette", "--occluders")
    assert "3 refined (0 with a failed last step)" in said and set(with_occ) == {"mean IoU", "mean visible IoU"}
    v0, v1 = with_occ["mean visible IoU"]
    report = ["tool: visible share %s; --occluders mean visible IoU %.4f -> %.4f (mean IoU %.4f -> %.4f); without it mean IoU %.4f -> %.4f"
              % (np.round(share, 2), v0, v1, *with_occ["mean IoU"], *plain["mean IoU"])]
    gt_arg = ["--gt", root, "--ply", "%d=%s" % (oid, ply)]
    before, after, after_plain = (errors.main(gt_arg + ["--est", path])[oid] for path in (est_csv, str(tmp_path / "occluders.csv"), str(tmp_path / "plain.csv")))
    capsys.readouterr()
    assert before["frames"] == after["frames"] == sorted(frames) and not after["missing"]
    report += ["tool frame %d: ADD %.3f mm -> %.3f with --occluders, %.3f without" % row
               for row in zip(after["frames"], before["errors"]["add"], after["errors"]["add"], after_plain["errors"]["add"])]
    with capsys.disabled():                                      # (measured figures for DESIGN section 22)
        print("\n" + "\n".join(report))
    assert v1 > v0 and v1 > plain["mean IoU"][1]
    # --known DIR: the planes the run above built (band 1.0 around the other instance), under the mask files' names
    known_dir = str(tmp_path / "known")
    os.makedirs(known_dir)
    for f in range(F):
        planes = ops.mask_known_from_others(ops.mask_sdf(cu(visib[f])), 1.0)
        Image.fromarray(host(planes[0]) * np.uint8(255), "L").save(os.path.join(known_dir, "%06d_%06d.png" % (frames[f], 0)))
    said, with_known = run("known.csv", "--silhouette", "--known", known_dir)
    strip_time = lambda name: [ln.rsplit(",", 1)[0] for ln in open(str(tmp_path / name))]
    assert strip_time("known.csv") == strip_time("occluders.csv") and with_known == with_occ
    _, wide = run("wide.csv", "--silhouette", "--occluders", "--occluder-band", "3")
    assert strip_time("wide.csv") != strip_time("occluders.csv")          # (the band reaches the field)
    with pytest.raises(SystemExit, match="exclude each other"):
        refine.main(common + ["--out", str(tmp_path / "x.csv"), "--silhouette", "--occluders", "--known", known_dir])
    for option in (["--occluders"], ["--known", known_dir]):
        with pytest.raises(SystemExit, match="go with --silhouette"):
            refine.main(common + ["--out", str(tmp_path / "x.csv")] + option)
    os.remove(os.path.join(known_dir, "%06d_%06d.png" % (frames[1], 0)))
    with pytest.raises(SystemExit, match="--known: no known image"):
        refine.main(common + ["--out", str(tmp_path / "x.csv"), "--silhouette", "--known", known_dir])
    os.remove(os.path.join(root, "mask_visib", "%06d_%06d.png" % (frames[2], 1)))          # the occluder's mask of the last frame
    with pytest.raises(SystemExit, match="--occluders: no mask_visib image"):
        refine.main(common + ["--out", str(tmp_path / "x.csv"), "--silhouette", "--occluders"])
    assert not os.path.exists(str(tmp_path / "x.csv"))
