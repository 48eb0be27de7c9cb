"""The argument helpers of texpose_amd/ops/_base.py, on the paths that need no device: what they refuse, with which exception,
and that the message names the entry point and the argument.  Every tensor here lives on the CPU, so a refusal of a wrong dtype, shape
or stride is also a refusal of a CPU tensor; tests/test_gpu_ops_args.py repeats those cases with GPU tensors, where only the named
property is wrong."""
import pytest
import torch

from texpose_amd import _lib, ops

f32, i32 = torch.float32, torch.int32


def bad_tensors():
    """A non-tensor, a CPU tensor of the wanted kind, a wrong dtype, a wrong shape and a non-contiguous view, for a wanted float32 [4,3]."""
    return {"non-tensor": [[0.0] * 3] * 4, "cpu": torch.zeros(4, 3), "dtype": torch.zeros(4, 3, dtype=torch.float64), "shape": torch.zeros(3, 4),
            "strided": torch.zeros(3, 4).t()}


@pytest.mark.parametrize("case", list(bad_tensors()))
def test_want_gpu_refuses(case):
    with pytest.raises(ValueError, match=r"some_op: the_arg must be a contiguous torch.float32 GPU tensor of shape \(4, 3\)"):
        ops._want_gpu("some_op", bad_tensors()[case], "the_arg", f32, (4, 3))


@pytest.mark.parametrize("case", list(bad_tensors()))
def test_outputs_refuses(case):
    spec = {"a": (f32, (4, 3)), "n": (i32, (4,))}
    for partial in (False, True):
        with pytest.raises(ValueError, match=r"some_op: out\['a'\] must be a contiguous torch.float32 GPU tensor of shape \(4, 3\)"):
            ops._outputs("some_op", {"a": bad_tensors()[case], "n": torch.zeros(4, dtype=i32)}, spec, "cpu", partial=partial)


def test_outputs_fresh_and_missing_keys():
    spec = {"a": (f32, (4, 3)), "n": (i32, (4,))}
    res = ops._outputs("some_op", None, spec, "cpu")
    assert list(res) == ["a", "n"] and res["a"].dtype == f32 and tuple(res["a"].shape) == (4, 3)
    assert res["n"].dtype == i32 and tuple(res["n"].shape) == (4,)
    with pytest.raises(KeyError):                                   # a missing key stays the KeyError ...
        ops._outputs("some_op", {}, spec, "cpu")
    res = ops._outputs("some_op", {}, spec, "cpu", partial=True)    # ... and is allocated with partial
    assert list(res) == ["a", "n"] and res["n"].dtype == i32 and tuple(res["a"].shape) == (4, 3)
    with pytest.raises(ValueError, match=r"some_op: out\['n'\]"):   # partial: the keys that are there are still checked
        ops._outputs("some_op", {"n": torch.zeros(4, dtype=i32)}, spec, "cpu", partial=True)


@pytest.mark.parametrize("case", list(bad_tensors()))
@pytest.mark.parametrize("align", [1, 16])
def test_workspace_arg_refuses(case, align):
    with pytest.raises(ValueError, match="some_op: workspace must be a contiguous.* GPU tensor of >= 8 bytes") as e:
        ops._workspace_arg("some_op", bad_tensors()[case], 8, "cpu", align=align)
    assert ("16-byte aligned" in str(e.value)) == (align == 16)


def test_workspace_arg_allocates():
    for need, words in ((0, 2), (1, 2), (16, 2), (17, 3), (4096, 512)):
        ws = ops._workspace_arg("some_op", None, need, "cpu", align=16)
        assert ws.dtype == torch.float64 and ws.numel() == words and ws.numel() * 8 >= need


def test_intr_per_view():
    """The device rule comes first, as in every wrapper before the helper: a CPU intr is the library's error whatever its shape, so the
    shape rule ([2,3,3] for B = 3; one [3,3] with allow_single=False) is asserted where it can be reached, in tests/test_gpu_ops_args.py."""
    for intr, single in ((torch.zeros(2, 3, 3), True), (torch.eye(3), False), (torch.eye(3), True), (torch.zeros(3, 3, 3), True)):
        with pytest.raises(_lib.TexposeLibraryError, match="intr must live on the GPU"):
            ops._intr_per_view("some_op", intr, 3, allow_single=single)


def test_poses_points_and_lengths_refuse_cpu_tensors():
    with pytest.raises(_lib.TexposeLibraryError, match="pose_est must live on the GPU"):
        ops._poses("some_op", torch.zeros(2, 3, 4), "pose_est")
    with pytest.raises(_lib.TexposeLibraryError, match="verts must live on the GPU"):
        ops._points("some_op", torch.zeros(5, 3), "verts")
    like = torch.zeros(2, 5, 3)
    assert ops._lengths("some_op", None, "x_len", 2, like) is None
    for t in (None, torch.zeros(2, dtype=i32)):
        with pytest.raises(ValueError, match=r"some_op: count must be an int32 GPU tensor of shape \(2,\)"):
            ops._lengths("some_op", t, "count", 2, like, required=True)


def test_float3_round_trips():
    v = (0.1, -2.5, 3.0e7)
    c = ops._float3(v)
    assert len(c) == 3 and list(c) == [torch.tensor(x, dtype=f32).item() for x in v]
    assert list(ops._float3(torch.tensor([1.0, 2.0, 4.0]))) == [1.0, 2.0, 4.0] and list(ops._float3([1, 2, 3])) == [1.0, 2.0, 3.0]
