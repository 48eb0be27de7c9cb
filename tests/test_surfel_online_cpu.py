"""CPU: the restatement of the data layer's surfel-map decode (tests/surfel_reader_ref.py) against golden G22 (the reference's own
get_edge / smooth_geo) and on hand-made cases, and the C ABI of tp_surfel_finish: argument validation without a GPU, the refusal
of CPU tensors, the struct layout."""
import ctypes as C

import numpy as np
import pytest
import torch

import surfel_reader_ref as RD
from texpose_amd import _lib


def test_reader_restatement_matches_g22(golden):
    g = golden("g22_smooth_geo")
    for name in ("a", "b"):
        x, edge, out = g[name + "_in"].numpy(), g[name + "_edge"].numpy() != 0, g[name + "_out"].numpy()
        assert edge.sum() >= 50 and (out != x).any(-1).sum() >= 50
        assert np.array_equal(RD.get_edge(x), edge), name
        got = RD.smooth_geo(x)
        assert got.dtype == np.float32 and np.array_equal(got, out), name
        assert np.array_equal(got[~edge], x[~edge])                   # only edge pixels change
    a_edge = g["a_edge"].numpy() != 0
    a_mask = g["a_in"].numpy()[..., 0] != 0
    assert a_mask[0].any() and a_mask[:, 0].any()                      # map a touches the top and the left image border ...
    assert (a_mask[0] & ~a_edge[0]).any() and (a_mask[:, 0] & ~a_edge[:, 0]).any()      # ... which alone makes no edge
    b = g["b_in"].numpy()
    assert ((b[..., 0] == 0) & (b[..., 1] != 0)).sum() >= 5           # map b: covered pixels outside the channel-0 mask


def test_one_pixel_object_is_an_edge_with_median_zero():
    x = np.zeros((5, 6, 3), np.float32)
    x[2, 3] = (0.5, 0.25, -0.75)
    e = RD.get_edge(x)
    assert e.sum() == 1 and e[2, 3]
    assert not RD.smooth_geo(x).any()                                  # eight zeros around it: every median is 0
    assert x[2, 3, 0] == 0.5                                           # the helper works on a copy


def test_mask_touching_all_four_borders_has_no_border_edges():
    x = np.ones((6, 7, 3), np.float32)
    assert not RD.get_edge(x).any()                                    # every in-image neighbour covered: the border is no edge
    assert np.array_equal(RD.smooth_geo(x), x)
    x[3, 3] = 0.0                                                      # one hole: exactly its four neighbours become edges
    e = RD.get_edge(x)
    want = np.zeros((6, 7), bool)
    want[2, 3] = want[4, 3] = want[3, 2] = want[3, 4] = True
    assert np.array_equal(e, want)
    x = np.zeros((4, 5, 3), np.float32)
    x[0, :] = 1.0                                                      # a covered top row: edges (the row below is empty) ...
    x[:, 0] = 1.0                                                      # ... and a covered left column
    e = RD.get_edge(x)
    assert e[0, 1:].all() and e[1:, 0].all() and not e[0, 0] and e.sum() == 4 + 3
    x = np.zeros((4, 5, 3), np.float32)
    x[:, 4] = 1.0                                                      # nothing wraps around: column 0 is not a neighbour of column 4
    assert np.array_equal(RD.get_edge(x)[:, 4], np.ones(4, bool)) and RD.get_edge(x).sum() == 4


def test_zero_first_channel_inside_the_object_counts_as_outside():
    rs = np.random.RandomState(0)
    x = rs.uniform(0.1, 1.0, size=(7, 7, 3)).astype(np.float32)
    x[3, 3, 0] = 0.0                                                   # covered (channels 1, 2 non-zero), first channel zero
    e = RD.get_edge(x)
    assert e.sum() == 4 and e[2, 3] and e[4, 3] and e[3, 2] and e[3, 4] and not e[3, 3]
    y = RD.smooth_geo(x)
    assert np.array_equal(y[3, 3], x[3, 3])                            # itself unchanged
    for (i, j) in ((2, 3), (4, 3), (3, 2), (3, 4)):
        for c in range(3):
            assert y[i, j, c] == np.sort(x[i - 1:i + 2, j - 1:j + 2, c].reshape(-1))[4]
    assert np.array_equal(y[~e], x[~e])


def test_median_uses_the_unsmoothed_map_and_replicated_borders():
    rs = np.random.RandomState(1)
    x = np.zeros((6, 6, 3), np.float32)
    x[:3, :3] = rs.uniform(0.1, 1.0, size=(3, 3, 3))                   # a block in the corner: five edge pixels next to each other
    y = RD.smooth_geo(x)
    pad = np.pad(x, ((1, 1), (1, 1), (0, 0)), mode="edge")
    e = RD.get_edge(x)
    assert e.sum() == 5 and not e[0, 0] and not e[1, 1]
    for i, j in zip(*np.nonzero(e)):
        for c in range(3):
            assert y[i, j, c] == np.sort(pad[i:i + 3, j:j + 3, c].reshape(-1))[4]


def test_quantize8_is_the_file_round_trip():
    x = np.array([0.0, 0.0039, 1 / 255, 0.5, 0.99999, 1.0, 254.999 / 255], np.float32)
    k = (x * 255).astype(np.uint8)
    assert np.array_equal(RD.quantize8(x), k.astype(np.float32) / 255)
    assert np.array_equal(k, [0, 0, 1, 127, 254, 255, 254])


def test_package_reader_matches_the_restatement(tmp_path):
    """texpose_amd.surfel.read_surfel_frame (numpy median; what --verify-online and the bench's file route use) against the helper."""
    from texpose_amd import surfel
    from texpose_amd.options import AttrDict
    rs = np.random.RandomState(5)
    H, W = 40, 52
    ii, jj = np.mgrid[0:H, 0:W]
    inside = ((ii - 18) ** 2 + (jj - 40) ** 2 < 15 ** 2)                # runs over the right border
    m = torch.from_numpy(inside.astype(np.float32))
    f = lambda lo, hi: torch.from_numpy(rs.uniform(lo, hi, size=(1, 3, H, W)).astype(np.float32)) * m
    out = AttrDict(rgb_syn=f(0, 1), nocs=f(0, 1), normal=f(-1, 1), depth=torch.where(m > 0, 600.0, -1.0)[None])
    surfel.write_surfel_frame(str(tmp_path), "2", 17, out, 0, obj_scene_id=3)
    got = surfel.read_surfel_frame(str(tmp_path), "2", 17, obj_scene_id=3)
    want = RD.decode_frame(str(tmp_path), "2", surfel.surfel_file_name(17, 3))
    assert want["nocs_edge"].sum() >= 30 and (want["nocs_pred"].transpose(1, 2, 0) != want["nocs_raw"]).any()
    for k in surfel.MAP_KEYS:
        assert got[k].dtype == torch.float32 and np.array_equal(got[k].numpy(), want[k]), k
    assert np.array_equal(want["image_syn"], RD.quantize8(out.rgb_syn[0].numpy()))
    assert np.array_equal(want["mask_syn"], inside.astype(np.float32))


def test_surfel_finish_argument_validation_without_gpu():
    lib = _lib.load()
    a = _lib.SurfelFinishArgs()
    assert lib.tp_surfel_finish(C.byref(a), None) < 0                  # zero sizes
    assert b"tp_surfel_finish" in lib.tp_last_error() and b"bad sizes" in lib.tp_last_error()
    a.B, a.H, a.W = 2, 8, 8
    assert lib.tp_surfel_finish(C.byref(a), None) < 0                  # NULL zbuf
    assert b"zbuf" in lib.tp_last_error()
    a.W = -3
    assert lib.tp_surfel_finish(C.byref(a), None) < 0
    assert b"bad sizes" in lib.tp_last_error()
    assert lib.tp_surfel_finish(None, None) < 0


def test_surfel_finish_struct_layout():
    # tp_surfel_finish_args: rgb, nocs, normal, zbuf (pointers); B, H, W, quantize (int); image_syn, mask_syn, nocs_pred, normal_pred
    assert C.sizeof(_lib.SurfelFinishArgs) == 4 * 8 + 4 * 4 + 4 * 8
    assert _lib.SurfelFinishArgs.zbuf.offset == 24 and _lib.SurfelFinishArgs.quantize.offset == 44
    assert _lib.SurfelFinishArgs.image_syn.offset == 48 and _lib.SurfelFinishArgs.normal_pred.offset == 72
    assert "tp_surfel_finish" in _lib.SYMBOLS and _lib.ABI_VERSION == 16


def test_ops_surfel_finish_refuses_cpu_tensors():
    from texpose_amd import ops
    with pytest.raises(_lib.TexposeLibraryError):
        ops.surfel_finish(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, 3))
