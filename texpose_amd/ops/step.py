"""K10, K13, K23: the losses' sums and totals, the step gate, the optimisers and the diagnostics of a training step."""
import ctypes as C
from typing import Optional

import torch

from .. import _lib
from ._base import Tensor, _call, _f32, _on_tensor_device, _ptr, _stream, _ticket

__all__ = ["_nerf_losses_args", "nerf_losses_fwd", "nerf_losses_bwd", "_lab_loss_args", "lab_loss_fwd", "lab_loss_bwd", "rmsprop_step",
           "_pending_total", "flush_pending_total", "weighted_sum", "step_flags", "stamp", "capture_node_count", "grad_pack", "clock_probe",
           "clock_ghz_from_probe", "step_inputs", "adam_step"]


def _nerf_losses_args(rgb, uncert, density, gathered):
    rgb, uncert, density, gathered = (_f32(rgb, "rgb"), _f32(uncert, "uncert"), _f32(density, "density"),
                                      _f32(gathered, "gathered"))
    B, P = rgb.shape[0], rgb.shape[1]
    N = density.shape[2]
    if rgb.shape != (B, P, 3) or uncert.numel() != B * P or density.shape != (B, P, N, 2) or gathered.numel() != B * 14 * P:
        raise ValueError("nerf_losses: rgb [B,P,3], uncert [B,P,1], density [B,P,N,2], gathered [B,14,p,p] expected")
    a = _lib.NerfLossesArgs()
    a.rgb, a.uncert, a.density, a.gathered = rgb.data_ptr(), uncert.data_ptr(), density.data_ptr(), gathered.data_ptr()
    a.B, a.P, a.N = B, P, N
    return a, (rgb, uncert, density, gathered)


@_on_tensor_device
def nerf_losses_fwd(rgb: Tensor, uncert: Tensor, density: Tensor, gathered: Tensor, want_losses: bool = False):
    """Four fp64 sums [sum m*se/u^2, sum m, sum log u^2, sum sigma_t] (device tensor) for the render / uncert /
    trans_reg terms of the generator step (reference compute_loss :747-760); with ``want_losses`` also the three fp32 loss
    values [render, uncert, trans_reg] formed by the same launch."""
    a, keep = _nerf_losses_args(rgb, uncert, density, gathered)
    ws = torch.empty(4 * _lib.NERF_LOSSES_MAX_BLOCKS, device=rgb.device)
    sums = torch.empty(4, dtype=torch.float64, device=rgb.device)
    losses = torch.empty(3, device=rgb.device) if want_losses else None
    a.workspace, a.sums, a.losses = ws.data_ptr(), sums.data_ptr(), _ptr(losses)
    a.ticket = _ticket(rgb.device, "nerf_losses")
    _call("tp_nerf_losses_fwd", a)
    return (sums, losses) if want_losses else sums


@_on_tensor_device
def nerf_losses_bwd(rgb: Tensor, uncert: Tensor, density: Tensor, gathered: Tensor, sums: Tensor, g_losses):
    """Gradients wrt rgb, uncert, density for the upstream gradients of (render, uncert, trans_reg): ``g_losses`` is a [3] tensor or
    a triple of 0-dim tensors / None (None = zero; no stacking launch)."""
    a, keep = _nerf_losses_args(rgb, uncert, density, gathered)
    ws = torch.empty(4, device=rgb.device)
    a.workspace, a.sums = ws.data_ptr(), sums.data_ptr()
    if torch.is_tensor(g_losses):
        g_losses = _f32(g_losses, "g_losses")
        gs = [g_losses[k] for k in range(3)]
    else:
        gs = [None if g is None else _f32(g, "g_loss") for g in g_losses]
    ptrs = [None if g is None else g.data_ptr() for g in gs]
    g_rgb, g_unc, g_den = torch.empty_like(keep[0]), torch.empty_like(keep[1]), torch.empty_like(keep[2])
    job = _pending_total.pop("job", None)
    if job is not None and job["stream"] == _stream():
        # (the generator step's loss total + gate, handed over by weighted_sum(defer=True): a side job of this launch)
        tp, wsf, n, out, flags = job["ptrs"], job["ws"], job["n"], job["out"], job["flags"]
        bad = flags["bad"]
        _call("tp_nerf_losses_bwd_total", a, ptrs[0], ptrs[1], ptrs[2], g_rgb.data_ptr(), g_unc.data_ptr(), g_den.data_ptr(), tp, wsf, n,
              out.data_ptr(), _ptr(flags.get("status")), bad.data_ptr(), bad.numel(), int(flags.get("word_status", 0)),
              int(flags["word_finite"]), flags["snapshot"].data_ptr(), _ptr(flags.get("step_counter")))
        return g_rgb, g_unc, g_den
    if job is not None:
        _pending_total["job"] = job
    _call("tp_nerf_losses_bwd", a, ptrs[0], ptrs[1], ptrs[2], g_rgb.data_ptr(), g_unc.data_ptr(), g_den.data_ptr())
    return g_rgb, g_unc, g_den


# ------------------------------------------------------------------------------------------ K23
def _lab_loss_args(rgb, real, mask, real_channel, mask_channel):
    """``real`` [B,C,...] holds the real image as channels real_channel .. real_channel + 2 and ``mask`` [B,C',...] (or None) the mask
    as channel mask_channel, P elements per channel: dense tensors (channel 0) or the patch gather's [B,14,p,p] (channels 3 and 13)."""
    rgb, real = _f32(rgb, "rgb"), _f32(real, "real")
    mask = None if mask is None else _f32(mask, "mask")
    if rgb.dim() != 3 or rgb.shape[2] != 3 or rgb.numel() == 0:
        raise ValueError("lab_loss: rgb [B,P,3] expected, got %s" % (tuple(rgb.shape),))
    B, P = rgb.shape[0], rgb.shape[1]
    for name, t, c0, n in (("real", real, int(real_channel), 3), ("mask", mask, int(mask_channel), 1)):
        if t is not None and (t.dim() < 2 or t.shape[0] != B or t.numel() != B * t.shape[1] * P or not 0 <= c0 <= t.shape[1] - n):
            raise ValueError("lab_loss: %s [B=%d,C,...] with %d elements per channel and channels %d..%d expected, got %s"
                             % (name, B, P, c0, c0 + n - 1, tuple(t.shape)))
    a = _lib.LabLossArgs()
    a.rgb, a.B, a.P = rgb.data_ptr(), B, P
    a.real, a.real_batch_stride, a.real_channel_stride = real.data_ptr() + 4 * int(real_channel) * P, real.shape[1] * P, P
    if mask is not None:
        a.mask, a.mask_batch_stride = mask.data_ptr() + 4 * int(mask_channel) * P, mask.shape[1] * P
    return a, (rgb, real, mask)


@_on_tensor_device
def lab_loss_fwd(rgb: Tensor, real: Tensor, mask: Optional[Tensor] = None, *, real_channel: int = 0, mask_channel: int = 0,
                 want_maps: bool = True):
    """The Lab chroma loss of rgb [B,P,3] against the real image (reference layers/lab_loss.py): one launch.
    -> (sums [2] fp64 = [sum l * mask, sum mask] (no mask: [sum l, 2 B P]), loss (0-dim) = sums[0] / sums[1], fake_lab, real_lab);
    the maps are [B,3,P] (None unless ``want_maps``): normalised Lab of the real image, and of rgb with its L plane replaced by that."""
    a, keep = _lab_loss_args(rgb, real, mask, real_channel, mask_channel)
    dev = keep[0].device
    ws = torch.empty(2 * _lib.LAB_LOSS_MAX_BLOCKS, dtype=torch.float64, device=dev)
    sums, loss = torch.empty(2, dtype=torch.float64, device=dev), torch.empty(1, device=dev)
    fake_lab = real_lab = None
    a.workspace, a.sums, a.loss = ws.data_ptr(), sums.data_ptr(), loss.data_ptr()
    if want_maps:
        fake_lab, real_lab = torch.empty(a.B, 3, a.P, device=dev), torch.empty(a.B, 3, a.P, device=dev)
        a.fake_lab, a.real_lab = fake_lab.data_ptr(), real_lab.data_ptr()
    a.ticket = _ticket(dev, "lab_loss")
    _call("tp_lab_loss_fwd", a)
    return sums, loss[0], fake_lab, real_lab


@_on_tensor_device
def lab_loss_bwd(rgb: Tensor, real: Tensor, mask: Optional[Tensor], sums: Tensor, g_loss: Tensor, *, real_channel: int = 0,
                 mask_channel: int = 0):
    """g_rgb [B,P,3] = g_loss * d loss / d rgb, recomputed from the forward's inputs and its ``sums``: one launch, every element written."""
    a, keep = _lab_loss_args(rgb, real, mask, real_channel, mask_channel)
    g_loss = _f32(g_loss, "g_loss")
    if sums.dtype != torch.float64 or sums.numel() != 2 or not sums.is_cuda or not sums.is_contiguous() or g_loss.numel() != 1:
        raise ValueError("lab_loss_bwd: sums [2] float64 on the GPU (lab_loss_fwd's) and a one-element g_loss expected")
    a.sums = sums.data_ptr()
    g_rgb = torch.empty_like(keep[0])
    _call("tp_lab_loss_bwd", a, g_loss.data_ptr(), g_rgb.data_ptr())
    return g_rgb


# ------------------------------------------------------------------------------------------ K10
@_on_tensor_device
def rmsprop_step(params, grads, square_avgs, lr, alpha: float = 0.99, eps: float = 1e-8, gate: Optional[Tensor] = None, steps=None) -> None:
    """One launch: sq = alpha sq + (1 - alpha) g^2;  p -= lr g / (sqrt(sq) + eps) for up to 16 tensors per call.
    ``lr``: python float, or a 0-dim CUDA tensor read on the device (captured training step).  ``gate``: int32 device words;
    if any is non-zero nothing is changed (the step counters included)."""
    lr_dev = lr.data_ptr() if isinstance(lr, torch.Tensor) else None
    lr_host = 0.0 if isinstance(lr, torch.Tensor) else float(lr)
    for i0 in range(0, len(params), _lib.RMSPROP_MAX_TENSORS):
        chunk = list(zip(params, grads, square_avgs, steps if steps is not None else [None] * len(params)))[i0:i0 + _lib.RMSPROP_MAX_TENSORS]
        arr = (_lib.RmspropTensor * len(chunk))()
        for a, (p, g, sq, st) in zip(arr, chunk):
            if not (p.is_contiguous() and g.is_contiguous() and sq.is_contiguous() and p.dtype == g.dtype == sq.dtype == torch.float32):
                raise _lib.TexposeLibraryError("rmsprop_step needs contiguous float32 tensors")
            a.param, a.grad, a.square_avg, a.numel = p.data_ptr(), g.data_ptr(), sq.data_ptr(), p.numel()
            if st is not None:                                 # (``steps``: 0-dim float32 DEVICE tensors, += 1 by the same launch)
                if not (st.is_cuda and st.dtype == torch.float32):
                    raise _lib.TexposeLibraryError("rmsprop_step: step counters must be float32 device tensors")
                a.step = st.data_ptr()
        _call("tp_rmsprop_step", arr, len(chunk), lr_dev, lr_host, float(alpha), float(eps), _ptr(gate), gate.numel() if gate is not None else 0)


_pending_total = {}          # "job": a loss total + gate waiting for the next nerf_losses_bwd launch on its stream (weighted_sum(defer=True))


def flush_pending_total() -> None:
    """Launch a total handed over with weighted_sum(defer=True) that no nerf_losses_bwd launch has taken (tp_weighted_sum_flags)."""
    job = _pending_total.pop("job", None)
    if job is None:
        return
    flags, bad = job["flags"], job["flags"]["bad"]
    with torch.cuda.device(job["out"].device):
        _call("tp_weighted_sum_flags", job["ptrs"], job["ws"], job["n"], job["out"].data_ptr(), _ptr(flags.get("status")), bad.data_ptr(),
              bad.numel(), int(flags.get("word_status", 0)), int(flags["word_finite"]), flags["snapshot"].data_ptr(),
              _ptr(flags.get("step_counter")))


@_on_tensor_device
def weighted_sum(terms, weights, flags=None, defer: bool = False) -> Tensor:
    """sum_k weights[k] * terms[k] for 0-dim float32 device tensors and host floats, one launch.  ``flags`` = dict(bad,
    word_finite, snapshot[, status, word_status, step_counter]): `step_flags` on the result in the same launch
    (tp_weighted_sum_flags); ``step_counter`` (int64 [1]) is incremented by it.
    ``defer`` (with flags): nothing is launched -- the next `nerf_losses_bwd` launch on this stream carries the job
    (tp_nerf_losses_bwd_total); the caller runs `flush_pending_total()` behind the backward pass in case there was none."""
    n = len(terms)
    ts = [_f32(t.detach(), "term") for t in terms]
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    ws = (C.c_float * n)(*[float(w) for w in weights])
    out = torch.empty((), device=ts[0].device)
    if defer and flags is not None:
        flush_pending_total()
        _pending_total["job"] = dict(ptrs=ptrs, ws=ws, n=n, out=out, flags=flags, stream=_stream(), keep=ts)
        return out
    if flags is None:
        _call("tp_weighted_sum", ptrs, ws, n, out.data_ptr())
    else:
        bad = flags["bad"]
        _call("tp_weighted_sum_flags", ptrs, ws, n, out.data_ptr(), _ptr(flags.get("status")), bad.data_ptr(), bad.numel(),
              int(flags.get("word_status", 0)), int(flags["word_finite"]), flags["snapshot"].data_ptr(), _ptr(flags.get("step_counter")))
    return out


@_on_tensor_device
def step_flags(total: Tensor, bad: Tensor, word_finite: int, snapshot: Tensor, status: Optional[Tensor] = None, word_status: int = 0) -> None:
    """bad[word_status] |= status & 1; bad[word_finite] |= !isfinite(total); snapshot = bad (K13 tp_step_flags, one launch)."""
    _call("tp_step_flags", _ptr(status), total.data_ptr(), bad.data_ptr(), bad.numel(), int(word_status), int(word_finite), snapshot.data_ptr())


def stamp(slots: torch.Tensor, i: int) -> None:
    """Diagnostic: the device clock (100 MHz ticks) into ``slots[i]`` (int64 device tensor), one launch in stream order."""
    assert slots.dtype == torch.int64 and slots.is_cuda and 0 <= i < slots.numel()
    _call("tp_stamp", slots.data_ptr() + 8 * i)


def capture_node_count(stream=None):
    """Number of nodes (kernel launches, fills, copies) recorded so far in the hipGraph that ``stream`` (default: the current one) is
    capturing into, or None when it is not capturing (tp_capture_node_count: hipStreamGetCaptureInfo_v2 + hipGraphGetNodes on the HIP
    runtime the library is linked against -- the one this process already runs on).  The trainers report it per captured graph
    (`launch_counts`: the launches of one training iteration)."""
    stream = stream or torch.cuda.current_stream()
    n = int(_lib.load().tp_capture_node_count(stream.cuda_stream))
    return None if n < 0 else n


@_on_tensor_device
def grad_pack(grads, flat: Tensor, scale: float, words: Optional[Tensor] = None, tail: Optional[Tensor] = None) -> None:
    """The gradients of one optimiser step into the flat all-reduce buffer: flat[concatenation] = scale * grads[k] (``None`` entries:
    ``numel`` zeros -- pass (None, numel)), and the gate words into the sticky tail (K13 tp_grad_pack, one launch per 32 tensors).
    ``grads``: tensors, or (None, numel) pairs; ``words`` int32 device words, ``tail`` float32 view behind the gradients in ``flat``."""
    rows, keep = [], []
    for g in grads:
        if isinstance(g, tuple):
            rows.append((None, int(g[1])))
            continue
        g = _f32(g, "grad")
        keep.append(g)
        rows.append((g.data_ptr(), g.numel()))
    if not flat.is_contiguous() or flat.dtype != torch.float32 or flat.numel() < sum(n for _, n in rows):
        raise _lib.TexposeLibraryError("grad_pack: the flat buffer must be contiguous float32 and hold every gradient")
    if words is not None and (words.dtype != torch.int32 or tail is None or tail.dtype != torch.float32 or tail.numel() < words.numel()):
        raise _lib.TexposeLibraryError("grad_pack: int32 gate words need a float32 tail of at least their length")
    off = 0
    for i0 in range(0, len(rows), _lib.GRAD_PACK_MAX_TENSORS):
        chunk = rows[i0:i0 + _lib.GRAD_PACK_MAX_TENSORS]
        ptrs = (C.c_void_p * len(chunk))(*[p for p, _ in chunk])
        numel = (C.c_int64 * len(chunk))(*[n for _, n in chunk])
        last = i0 + _lib.GRAD_PACK_MAX_TENSORS >= len(rows)
        n_words = 0 if (tail is None or not last) else (words.numel() if words is not None else tail.numel())
        _call("tp_grad_pack", ptrs, numel, len(chunk), flat.data_ptr() + 4 * off, float(scale), _ptr(words) if last else None, n_words,
              _ptr(tail) if last else None)
        off += sum(n for _, n in chunk)


def clock_probe(windows: int = 16, window_us: int = 5000) -> torch.Tensor:
    """Diagnostic: launch the clock sampler on the CURRENT stream (use a side stream, then launch the load on another one); returns
    the int64 device tensor [windows, 2] it fills with (shader cycles, 100-MHz ticks) per window -- read it after a synchronise;
    `clock_ghz_from_probe` folds it."""
    out = torch.zeros(windows, 2, dtype=torch.int64, device="cuda")
    _call("tp_clock_probe", out.data_ptr(), int(windows), int(window_us))
    return out


def clock_ghz_from_probe(out: torch.Tensor) -> float:
    """Median shader clock in GHz over the probe's windows (the first and the last one left out when there are more than four)."""
    w = out.cpu().double()
    ghz = (w[:, 0] / w[:, 1].clamp(min=1)) * 0.1
    if len(ghz) > 4:
        ghz = ghz[1:-1]
    return float(ghz.median())


def step_inputs(copies, scalars=(), words=None, words_host=None) -> None:
    """The per-iteration host -> device state of a replayed step in ONE launch (K13 tp_step_inputs): ``copies`` = [(dst, src)]
    device tensors of equal byte size (the batch into the static inputs), ``scalars`` = [(0-dim float32 device tensor, value)],
    ``words`` (int32 device tensor) copied out to ``words_host`` (pinned int32 host tensor of the same length)."""
    copies, scalars = list(copies), list(scalars)
    if len(scalars) > _lib.STEP_INPUTS_MAX_SCALARS:
        raise ValueError("step_inputs: too many scalars")
    dev = (copies[0][0] if copies else scalars[0][0] if scalars else words).device
    with torch.cuda.device(dev):
        first = True
        for i0 in range(0, max(len(copies), 1), _lib.STEP_INPUTS_MAX_COPIES):
            chunk = copies[i0:i0 + _lib.STEP_INPUTS_MAX_COPIES]
            arr = (_lib.StepCopy * max(len(chunk), 1))()
            for a, (d, s) in zip(arr, chunk):
                nb = d.numel() * d.element_size()
                if not (d.is_contiguous() and s.is_contiguous() and s.numel() * s.element_size() == nb and d.device == s.device == dev):
                    raise _lib.TexposeLibraryError("step_inputs: copies need contiguous same-size tensors on one device")
                a.dst, a.src, a.bytes = d.data_ptr(), s.data_ptr(), nb
            sc = scalars if first else []
            sd = (C.c_void_p * max(len(sc), 1))(*[t.data_ptr() for t, _ in sc])
            sv = (C.c_float * max(len(sc), 1))(*[float(v) for _, v in sc])
            for t, _ in sc:
                if t.dtype != torch.float32 or t.device != dev:
                    raise _lib.TexposeLibraryError("step_inputs: scalars are float32 tensors on the batch's device")
            w = words if first else None
            if w is not None and not (w.dtype == torch.int32 and words_host.dtype == torch.int32 and words_host.is_pinned()
                                      and words_host.numel() == w.numel()):
                raise _lib.TexposeLibraryError("step_inputs: gate words need an int32 device tensor and a pinned int32 host tensor")
            _call("tp_step_inputs", arr, len(chunk), sd, sv, len(sc), _ptr(w), None if w is None else words_host.data_ptr(),
                  0 if w is None else w.numel())
            first = False


@_on_tensor_device
def adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, lr, beta1: float, beta2: float, eps: float, gate: Optional[Tensor] = None) -> None:
    """torch.optim.Adam's update of all tensors in one launch per 32 (K13 tp_adam_step); ``steps``: 0-dim float tensors with
    the step count BEFORE this update; a gated one-wave launch inside the same call adds 1 to each afterwards."""
    lr_dev = lr.data_ptr() if isinstance(lr, torch.Tensor) else None
    lr_host = 0.0 if isinstance(lr, torch.Tensor) else float(lr)
    rows = list(zip(params, grads, exp_avgs, exp_avg_sqs, steps))
    for i0 in range(0, len(rows), _lib.ADAM_MAX_TENSORS):
        chunk = rows[i0:i0 + _lib.ADAM_MAX_TENSORS]
        arr = (_lib.AdamTensor * len(chunk))()
        for a, (p, g, m, v, st) in zip(arr, chunk):
            if not (p.is_contiguous() and g.is_contiguous() and m.is_contiguous() and v.is_contiguous()
                    and p.dtype == g.dtype == m.dtype == v.dtype == st.dtype == torch.float32 and st.is_cuda):
                raise _lib.TexposeLibraryError("adam_step needs contiguous float32 tensors and device step counters")
            a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.step, a.numel = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), st.data_ptr(), p.numel()
        _call("tp_adam_step", arr, len(chunk), lr_dev, lr_host, float(beta1), float(beta2), float(eps), _ptr(gate),
              gate.numel() if gate is not None else 0, _ticket(chunk[0][0].device, "adam"))
