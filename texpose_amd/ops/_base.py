"""What the stage modules of texpose_amd.ops share: the current stream, the argument helpers and the one launch helper."""
import ctypes as C
import functools
from typing import Dict, Optional

import torch

from .. import _lib

__all__ = ["Tensor", "_stream", "_call", "_tensors", "_on_tensor_device", "_f32", "_out_like", "_ptr", "_float3", "_want_gpu", "_outputs",
           "_workspace_arg", "_lengths", "_intr_per_view", "_poses", "_points", "_ticket_words", "_ticket"]

Tensor = torch.Tensor


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _call(name: str, *args) -> None:
    """``lib.<name>(*args, current stream)``: every launch of the package.  A non-zero status raises TexposeLibraryError naming the entry
    point, with the library's own text (tp_last_error)."""
    rc = getattr(_lib._lib or _lib.load(), name)(*args, _stream())      # (load()'s own handle once it exists: one Python call fewer)
    if rc != 0:
        _lib.check(rc, name)


def _tensors(objs):
    for o in objs:
        if isinstance(o, torch.Tensor):
            yield o
        elif isinstance(o, (list, tuple)):
            yield from _tensors(o)
        elif isinstance(o, dict):
            yield from _tensors(o.values())


def _on_tensor_device(fn):
    """The C entry points launch on the CURRENT HIP device and stream (and keep per-device kernel attributes): make the
    tensors' own device current for the call, and refuse arguments that live on different devices."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        dev = None
        for t in _tensors(args + tuple(kwargs.values())):
            if t.is_cuda:
                if dev is None:
                    dev = t.device
                elif t.device != dev:
                    raise _lib.TexposeLibraryError(f"{fn.__name__}: tensors on different devices ({dev} and {t.device})")
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    wrapped.__module__ = __package__                # (a wrapper names the namespace it is called through, as before ops was a package)
    return wrapped


def _f32(t: Tensor, name: str) -> Tensor:
    if not t.is_cuda:
        raise _lib.TexposeLibraryError(f"{name} must live on the GPU (texpose_amd has no CPU path)")
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _out_like(out: Optional[Tensor], like: Tensor, shape=None) -> Tensor:
    """``out`` (checked: float32, contiguous, on ``like``'s device, of the wanted number of elements) or a fresh tensor."""
    shape = tuple(like.shape) if shape is None else tuple(shape)
    if out is None:
        return torch.empty(shape, device=like.device, dtype=torch.float32)
    n = 1
    for d in shape:
        n *= d
    if out.dtype != torch.float32 or not out.is_contiguous() or out.device != like.device or out.numel() != n:
        raise _lib.TexposeLibraryError("out= must be a contiguous float32 tensor of %s elements on %s" % (n, like.device))
    return out


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _float3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


# The argument rules of the scene / pose entry points (K19 on).  Inputs go through _f32 (converted if need be) and a shape helper;
# tensors that are written into, or that the docstring says are "taken as they are", go through _want_gpu: nothing is converted.
def _want_gpu(op: str, t, name: str, dtype, shape):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
        raise ValueError(f"{op}: {name} must be a contiguous {dtype} GPU tensor" + ("" if shape is None else f" of shape {shape}"))
    return t


def _outputs(op: str, out: Optional[Dict[str, Tensor]], spec, dev, partial: bool = False) -> Dict[str, Tensor]:
    """``spec``: key -> (dtype, shape).  Every key's ``out[key]``, taken as it is, or a fresh tensor on ``dev`` where ``out`` is None
    or, with ``partial``, lacks the key (without it a missing key is the KeyError)."""
    return {k: torch.empty(shape, device=dev, dtype=dtype) if out is None or (partial and k not in out)
            else _want_gpu(op, out[k], f"out[{k!r}]", dtype, shape) for k, (dtype, shape) in spec.items()}


def _workspace_arg(op: str, workspace: Optional[Tensor], need_bytes: int, dev, align: int = 1) -> Tensor:
    """The caller's workspace of at least ``need_bytes`` bytes at an address that is a multiple of ``align``, else a fresh one."""
    if workspace is None:
        return torch.empty(max(2, (need_bytes + 7) // 8), device=dev, dtype=torch.float64)
    if (not torch.is_tensor(workspace) or not workspace.is_cuda or not workspace.is_contiguous()
            or workspace.numel() * workspace.element_size() < need_bytes or workspace.data_ptr() % align):
        raise ValueError("%s: workspace must be a contiguous%s GPU tensor of >= %d bytes" % (op, ", %d-byte aligned" % align if align > 1 else "", need_bytes))
    return workspace


def _lengths(op: str, t: Optional[Tensor], name: str, n: int, like: Tensor, required: bool = False) -> Optional[Tensor]:
    if t is None and not required:
        return None
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.int32 or tuple(t.shape) != (n,) or t.device != like.device:
        raise ValueError(f"{op}: {name} must be an int32 GPU tensor of shape ({n},)")
    return t.contiguous()


def _intr_per_view(op: str, intr: Tensor, B: int, allow_single: bool = True) -> Tensor:
    """``intr`` as float32 [B,3,3]; with ``allow_single`` one [3,3] stands for every view."""
    intr = _f32(intr.detach(), "intr")
    if allow_single and intr.dim() == 2:
        intr = intr[None].expand(B, 3, 3).contiguous()
    if tuple(intr.shape) != (B, 3, 3):
        raise ValueError("%s: intr [B=%d,3,3]%s expected, got %s" % (op, B, " or [3,3]" if allow_single else "", tuple(intr.shape)))
    return intr


def _poses(op: str, t: Tensor, name: str, B: Optional[int] = None) -> Tensor:
    """``t`` as float32 [B,3,4]: of the given ``B``, or of any B >= 1."""
    t = _f32(t.detach(), name)
    if t.dim() != 3 or tuple(t.shape[1:]) != (3, 4) or (t.shape[0] == 0 if B is None else t.shape[0] != B):
        raise ValueError("%s: %s [%s,3,4] expected, got %s" % (op, name, "B" if B is None else "B=%d" % B, tuple(t.shape)))
    return t


def _points(op: str, t: Tensor, name: str, n: Optional[int] = None) -> Tensor:
    """``t`` as float32 [n,3]: of the given ``n``, or of any n >= 1."""
    t = _f32(t.detach(), name)
    if t.dim() != 2 or t.shape[1] != 3 or (t.shape[0] == 0 if n is None else t.shape[0] != n):
        raise ValueError("%s: %s [%s,3] expected, got %s" % (op, name, "n" if n is None else "n=%d" % n, tuple(t.shape)))
    return t


_ticket_words = {}           # (device index, stream, entry point) -> one zero-filled int32 word (the kernel leaves it zero)


def _ticket(dev, name: str) -> int:
    """The arrival counter of a last-block hand-over (tp_nerf_losses_fwd, tp_adam_step) for the CURRENT stream: launches of one
    entry point that overlap on different streams of a device must not count each other's arrivals, so the word is owned by
    (device, stream, entry point).  Made on first use; inside a hipGraph capture on a stream that has none yet the fill that
    creates it is simply part of the captured step (correct, one launch more: warm up on the capturing stream to avoid it)."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, name)
    t = _ticket_words.get(key)
    if t is None:
        t = _ticket_words[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t.data_ptr()
