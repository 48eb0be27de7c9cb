"""K9, K11, K14-K17: the PatchGAN step -- paired launches, spectral norm, InstanceNorm + LeakyReLU, the 4x4 convolutions, head and tail."""
import ctypes as C
from typing import Optional

import torch

from .. import _lib, knobs
from ._base import Tensor, _call, _f32, _on_tensor_device, _out_like, _ptr, _ticket

__all__ = ["_pair_state", "PAIRABLE", "paired", "_pair_slot", "_launch", "spectral_norm_fwd", "SN_MAX_SETS", "spectral_norm_fwd_sets",
           "spectral_norm_buffers", "spectral_norm_bwd", "inorm_lrelu_fwd", "inorm_lrelu_bwd", "inorm_lrelu_bwd_bwd", "_conv_counters",
           "_conv_counters_retired", "_conv_scratch", "_conv4s2", "conv4s2_fwd", "conv4s2_fwd_inorm_supported", "conv4s2_fwd_inorm",
           "conv4s2_dgrad_inorm_supported", "conv4s2_dgrad", "conv4s2_wgrad", "bce_logits_fwd", "bce_logits_bwd", "disc_inputs", "fake_patch_bwd",
           "sumsq_mean_fwd", "sumsq_mean_bwd", "sumsq_mean_fwd_bwd", "gan_disc_losses", "_head_args", "disc_head_fwd", "disc_head_bwd",
           "disc_head_bwd_bwd", "DISC_TAIL_MAX_ROWS", "_tail_ws", "disc_tail_eligible", "_tail_args", "_tail_workspace", "disc_tail_fwd",
           "disc_tail_bwd", "disc_tail_bwd_bwd", "SKINNY_MAX_ROWS", "SKINNY_DGRAD_MAX_ROWS", "skinny_linear_fwd", "skinny_linear_dgrad",
           "skinny_linear_wgrad"]

# ---- pairs: two calls of ONE pairable op issued as one launch (tp_*_pair: the real and the fake pass of the discriminator step)
_pair_state = {"active": False, "pending": None}
PAIRABLE = ("tp_conv4s2_fwd_inorm", "tp_conv4s2_dgrad", "tp_conv4s2_wgrad", "tp_disc_tail_fwd", "tp_disc_tail_bwd", "tp_inorm_lrelu_bwd")


class paired:
    """``with ops.paired():`` -- inside, calls of the pairable ops (PAIRABLE) must come in twos of the same op; the first of a pair only
    prepares its arguments and outputs, the second launches both problems in ONE launch.  Outputs are returned by each call as usual
    and are valid behind the pair's launch.  The second problem of a pair gets its own tile counters / workspace / ticket (slot 1)."""

    def __enter__(self):
        if _pair_state["active"]:
            raise RuntimeError("ops.paired() does not nest")
        _pair_state["active"], _pair_state["pending"] = True, None
        return self

    def __exit__(self, exc_type, exc, tb):
        pending, _pair_state["active"], _pair_state["pending"] = _pair_state["pending"], False, None
        if exc_type is None and pending is not None:
            raise RuntimeError("ops.paired(): %s was issued without a partner" % pending[0])
        return False


def _pair_slot() -> int:
    """0 for the first problem of a pair (and outside ops.paired()), 1 for the second: which scratch set an op takes."""
    return 1 if _pair_state["active"] and _pair_state["pending"] is not None else 0


def _launch(name: str, args, extra=(), keep=()):
    """Launch ``<name>(args, *extra)`` through _call -- or, inside ops.paired(), hold it back / launch it with its partner through
    ``lib.<name>_pair``.  ``extra``: per-problem trailing arguments (pointers), interleaved per problem in the pair entry points as the
    header declares them; scalars shared by both problems are taken from the second call.  ``keep``: the tensors ``args`` points into (a
    held-back first problem of a pair keeps them alive until its partner launches both)."""
    if not _pair_state["active"]:
        if name == "tp_inorm_lrelu_bwd":
            _call("tp_inorm_lrelu_bwd", args.xhat, args.rstd, args.gy, args.n_inst, args.hw, args.slope, args.addend, args.gx)
        elif name == "tp_conv4s2_fwd_inorm":
            _call("tp_conv4s2_fwd_inorm", args, extra[2], extra[3], extra[0], extra[1])
        else:
            _call(name, args)
        return
    pending = _pair_state["pending"]
    if pending is None:
        _pair_state["pending"] = (name, args, extra, torch.cuda.current_stream().cuda_stream, keep)
        return
    p_name, p_args, p_extra, p_stream, _ = pending
    _pair_state["pending"] = None
    if p_name != name or p_stream != torch.cuda.current_stream().cuda_stream:
        raise RuntimeError("ops.paired(): %s cannot be paired with %s (same op, same stream)" % (name, p_name))
    if name == "tp_conv4s2_fwd_inorm":
        _call("tp_conv4s2_fwd_inorm_pair", p_args, p_extra[0], p_extra[1], args, extra[0], extra[1], extra[2], extra[3])
    else:
        _call(name + "_pair", p_args, args)


@_on_tensor_device
def spectral_norm_fwd(weights, us, vs, training: bool, keep_uv: bool = False, out=None):
    """weights[i] [out, ...] (contiguous), us[i] [out], vs[i] [K]: one power iteration per weight when ``training``
    (u, v updated IN PLACE, like torch.nn.utils.spectral_norm), then W_sn = W / sigma.  Returns (W_sn list, sigma
    list of 1-element tensors).  All weights of a module in three launches (two in eval mode).  ``keep_uv``: also returns copies of u / v as
    they stand after this call (written by the last launch) as a third / fourth list.
    ``out`` = (W_sn list, sigma list, u-copy list, v-copy list, work list) of pre-allocated tensors (spectral_norm_buffers): nothing is
    allocated -- the captured training step writes the NEXT iteration's normalised weights into static buffers."""
    lib = _lib.load()
    n = len(weights)
    arr = (_lib.SnWeight * n)()
    outs, sigmas, keep = [], [], []
    u_copies = v_copies = None
    if out is not None:
        keep_uv = True
        u_copies, v_copies = list(out[2]), list(out[3])
    elif keep_uv:
        flat = torch.empty(sum(u.numel() + v.numel() for u, v in zip(us, vs)), device=us[0].device)
        parts = flat.split([t.numel() for t in list(us) + list(vs)])
        u_copies, v_copies = list(parts[:n]), list(parts[n:])
    for i, (w, u, v) in enumerate(zip(weights, us, vs)):
        w = _f32(w, "weight")
        rows, cols = w.shape[0], w.numel() // w.shape[0]
        if out is not None:
            o, sg, wk = _out_like(out[0][i], w), out[1][i], out[4][i]
        else:
            o, sg = torch.empty_like(w), torch.empty(1, device=w.device)
            wk = torch.empty(lib.tp_sn_work_floats(rows, cols), device=w.device)
        a = arr[i]
        a.weight, a.u, a.v, a.weight_sn, a.sigma, a.work = w.data_ptr(), u.data_ptr(), v.data_ptr(), o.data_ptr(), sg.data_ptr(), wk.data_ptr()
        a.rows, a.cols = rows, cols
        if keep_uv:
            a.u_out, a.v_out = u_copies[i].data_ptr(), v_copies[i].data_ptr()
        outs.append(o); sigmas.append(sg); keep += [w, wk]
    _call("tp_sn_fwd", arr, n, int(bool(training)))
    return (outs, sigmas, u_copies, v_copies) if keep_uv else (outs, sigmas)


SN_MAX_SETS = _lib.SN_MAX_SETS


@_on_tensor_device
def spectral_norm_fwd_sets(weights, us, vs, n_sets: int):
    """``n_sets`` training-mode `spectral_norm_fwd(..., keep_uv=True)` calls in a row -- each advances u / v once -- as 2 n_sets + 1
    launches instead of 3 n_sets (tp_sn_fwd_sets: one normalisation launch for all sets, W read once by it).  Returns a list of n_sets
    tuples (W_sn list, sigma list, u copies, v copies); bit-identical to the separate calls."""
    lib = _lib.load()
    n = len(weights)
    if not 1 <= n_sets <= SN_MAX_SETS:
        raise ValueError("spectral_norm_fwd_sets: 1..%d sets" % SN_MAX_SETS)
    arr = (_lib.SnWeight * (n * n_sets))()
    ws = [_f32(w, "weight") for w in weights]
    works = [torch.empty(lib.tp_sn_work_floats(w.shape[0], w.numel() // w.shape[0]), device=w.device) for w in ws]
    sets = []
    for k in range(n_sets):
        flat = torch.empty(sum(u.numel() + v.numel() for u, v in zip(us, vs)), device=us[0].device)
        parts = flat.split([t.numel() for t in list(us) + list(vs)])
        u_copies, v_copies = list(parts[:n]), list(parts[n:])
        outs, sigmas = [], []
        for i, (w, u, v) in enumerate(zip(ws, us, vs)):
            o, sg = torch.empty_like(w), torch.empty(1, device=w.device)
            a = arr[k * n + i]
            a.weight, a.u, a.v, a.weight_sn, a.sigma, a.work = w.data_ptr(), u.data_ptr(), v.data_ptr(), o.data_ptr(), sg.data_ptr(), works[i].data_ptr()
            a.rows, a.cols = w.shape[0], w.numel() // w.shape[0]
            a.u_out, a.v_out = u_copies[i].data_ptr(), v_copies[i].data_ptr()
            outs.append(o); sigmas.append(sg)
        sets.append((outs, sigmas, u_copies, v_copies))
    _call("tp_sn_fwd_sets", arr, n, n_sets)
    return sets


def spectral_norm_buffers(weights, us, vs):
    """Pre-allocated outputs of one `spectral_norm_fwd(..., out=)` call: (W_sn, sigma, u copies, v copies, work)."""
    lib = _lib.load()
    dev = weights[0].device
    return ([torch.empty_like(w, memory_format=torch.contiguous_format) for w in weights], [torch.empty(1, device=dev) for _ in weights],
            [torch.empty_like(u) for u in us], [torch.empty_like(v) for v in vs],
            [torch.empty(lib.tp_sn_work_floats(w.shape[0], w.numel() // w.shape[0]), device=dev) for w in weights])


@_on_tensor_device
def spectral_norm_bwd(grads_sn, weights_sn, us, vs, sigmas, accumulate_into=None, second=None, step=None):
    """dL/dW from dL/dW_sn with u, v treated as constants (torch's convention): (G - <G, W_sn> u v^T) / sigma.
    ``accumulate_into``: a list of tensors the results are ADDED to; they are what is returned.
    ``second`` = (grads_sn2, weights_sn2, us2, vs2, sigmas2): a second normalised instance of the same weights in one optimiser
    step (the discriminator step's fake pass) -- its term is added inside the same two launches.
    ``step`` = dict(terms, weights, flags=dict(bad, word_finite, snapshot), params, square_avgs, steps, lr, alpha, eps): the END of a
    discriminator step in the same two launches (tp_sn_bwd_step) -- the loss total and the step gate (what `weighted_sum(flags=)`
    does) in the first, the RMSprop update of ``params`` (what `rmsprop_step(gate=snapshot)` does) in the second; the total goes to
    ``step["total"]`` (a 0-dim tensor made here)."""
    lib = _lib.load()
    n = len(grads_sn)
    arr = (_lib.SnWeight * n)()
    outs, keep = [], []
    for i, (g, ws, u, v, sg) in enumerate(zip(grads_sn, weights_sn, us, vs, sigmas)):
        g = _f32(g, "grad")
        rows, cols = ws.shape[0], ws.numel() // ws.shape[0]
        o = torch.empty_like(ws) if accumulate_into is None else _out_like(accumulate_into[i], ws)
        arr[i].accumulate = 0 if accumulate_into is None else 1
        wk = torch.empty(lib.tp_sn_work_floats(rows, cols), device=ws.device)
        a = arr[i]
        a.u, a.v, a.weight_sn, a.sigma, a.grad_sn, a.grad, a.work = (u.data_ptr(), v.data_ptr(), ws.data_ptr(), sg.data_ptr(),
                                                                       g.data_ptr(), o.data_ptr(), wk.data_ptr())
        a.rows, a.cols = rows, cols
        if second is not None:
            g2 = _f32(second[0][i], "grad")
            if g2.shape != g.shape or second[1][i].shape != ws.shape:
                raise ValueError("spectral_norm_bwd: the second instance must have the shapes of the first")
            a.grad_sn2, a.weight_sn2, a.u2, a.v2, a.sigma2 = (g2.data_ptr(), second[1][i].data_ptr(), second[2][i].data_ptr(),
                                                              second[3][i].data_ptr(), second[4][i].data_ptr())
            keep.append(g2)
        outs.append(o); keep += [g, wk]
    if step is None:
        _call("tp_sn_bwd", arr, n)
        return outs
    if accumulate_into is not None:
        raise ValueError("spectral_norm_bwd(step=): the gradients are the step's own (no accumulate_into)")
    t = _lib.SnStepTail()
    terms = [_f32(x.detach(), "term") for x in step["terms"]]
    if not 1 <= len(terms) <= 4 or len(step["weights"]) != len(terms) or len(step["params"]) != n:
        raise ValueError("spectral_norm_bwd(step=): 1..4 terms with their weights, one parameter per weight")
    for k, (x, w) in enumerate(zip(terms, step["weights"])):
        t.terms[k], t.weights[k] = x.data_ptr(), float(w)
    flags = step["flags"]
    step["total"] = total = torch.empty((), device=terms[0].device)
    t.n_terms, t.word_finite, t.total = len(terms), int(flags["word_finite"]), total.data_ptr()
    t.bad, t.snapshot, t.n_bad = flags["bad"].data_ptr(), flags["snapshot"].data_ptr(), flags["bad"].numel()
    if flags["snapshot"].numel() != flags["bad"].numel() or flags["bad"].dtype != torch.int32 or flags["snapshot"].dtype != torch.int32:
        raise ValueError("spectral_norm_bwd(step=): int32 gate words and a snapshot of the same length")
    steps = step.get("steps") or [None] * n
    for i, (p, sq, st, o) in enumerate(zip(step["params"], step["square_avgs"], steps, outs)):
        if not (p.is_contiguous() and sq.is_contiguous() and p.dtype == sq.dtype == torch.float32 and p.shape == o.shape == sq.shape):
            raise _lib.TexposeLibraryError("spectral_norm_bwd(step=): contiguous float32 parameters shaped like their gradients")
        t.param[i], t.square_avg[i] = p.data_ptr(), sq.data_ptr()
        if st is not None:
            if not (st.is_cuda and st.dtype == torch.float32):
                raise _lib.TexposeLibraryError("spectral_norm_bwd(step=): step counters must be float32 device tensors")
            t.step[i] = st.data_ptr()
    lr = step["lr"]
    t.lr_dev = lr.data_ptr() if isinstance(lr, torch.Tensor) else None
    t.lr_host = 0.0 if isinstance(lr, torch.Tensor) else float(lr)
    t.alpha, t.one_minus_alpha, t.eps = float(step["alpha"]), float(1.0 - float(step["alpha"])), float(step["eps"])
    _call("tp_sn_bwd_step", arr, n, t)
    keep.append(terms)
    return outs


# ------------------------------------------------------------------------------------------ K9
@_on_tensor_device
def inorm_lrelu_fwd(x: Tensor, eps: float, slope: float, y_out: Optional[Tensor] = None):
    """x [B,C,H,W] -> (y, xhat, rstd [B*C]) = LeakyReLU(InstanceNorm2d(x)) and what its derivatives need.  ``y_out``: where y is
    written (a contiguous view of x's shape, e.g. one half of a stacked buffer)."""
    x = _f32(x, "x")
    n_inst, hw = x.shape[0] * x.shape[1], x.shape[2] * x.shape[3]
    y, xhat = _out_like(y_out, x), torch.empty_like(x)
    rstd = torch.empty(n_inst, device=x.device)
    _call("tp_inorm_lrelu_fwd", x.data_ptr(), n_inst, hw, float(eps), float(slope), y.data_ptr(), xhat.data_ptr(), rstd.data_ptr())
    return y, xhat, rstd


@_on_tensor_device
def inorm_lrelu_bwd(xhat: Tensor, rstd: Tensor, gy: Tensor, slope: float, addend: Optional[Tensor] = None,
                    out: Optional[Tensor] = None) -> Tensor:
    """gx; ``addend`` (same shape) is added to it in the same launch (a second cotangent of x)."""
    gy = _f32(gy, "gy")
    gx = _out_like(out, xhat)
    if addend is not None:
        addend = _f32(addend, "addend")
        if addend.numel() != xhat.numel():
            raise ValueError("inorm_lrelu_bwd: addend must have the shape of x")
    a = _lib.InormBwdArgs()
    a.xhat, a.rstd, a.gy, a.n_inst, a.hw, a.slope = xhat.data_ptr(), rstd.data_ptr(), gy.data_ptr(), rstd.numel(), xhat.numel() // rstd.numel(), float(slope)
    a.addend, a.gx = _ptr(addend), gx.data_ptr()
    _launch("tp_inorm_lrelu_bwd", a, keep=(xhat, rstd, gy, addend, gx))
    return gx


@_on_tensor_device
def inorm_lrelu_bwd_bwd(xhat: Tensor, rstd: Tensor, gy: Tensor, ggx: Tensor, slope: float, out_gy: Optional[Tensor] = None):
    """cotangent ggx of the backward's output gx -> (grad wrt gy, grad wrt x)."""
    gy, ggx = _f32(gy, "gy"), _f32(ggx, "ggx")
    g_gy, g_x = _out_like(out_gy, xhat), torch.empty_like(xhat)
    _call("tp_inorm_lrelu_bwd_bwd", xhat.data_ptr(), rstd.data_ptr(), gy.data_ptr(), ggx.data_ptr(), rstd.numel(), xhat.numel() // rstd.numel(),
          float(slope), g_gy.data_ptr(), g_x.data_ptr())
    return g_gy, g_x


# ------------------------------------------------------------------------------------------ K11
_conv_counters = {}          # (device index, stream) -> zero-filled int32 tensor (the kernels leave it zero)
_conv_counters_retired = []  # outgrown counter tensors: a captured hipGraph may still hold their address -- never freed


def _conv_scratch(ws_fn, a, op: int, dev):
    """(workspace tensor or None, counters tensor) for a K11 / K12 launch described by the argument struct ``a``."""
    n_cnt = C.c_int64(0)
    ws_floats = ws_fn(a, op, C.byref(n_cnt))
    if ws_floats < 0:
        _lib.check(-1, "tp_conv_workspace")
    # one counter array per (device, stream): launches on different streams may run concurrently (the two branches of the
    # captured training step) and must not see each other's tile arrivals
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, _pair_slot())
    cnt = _conv_counters.get(key)
    if cnt is None or cnt.numel() < n_cnt.value:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.TexposeLibraryError("tp_conv: the tile counters must exist before a hipGraph capture (run one "
                                           "eager step first)")
        if cnt is not None:
            _conv_counters_retired.append(cnt)          # a graph captured earlier keeps incrementing / zeroing this one
        cnt = torch.zeros(max(int(n_cnt.value), 1 << 14), dtype=torch.int32, device=dev)
        _conv_counters[key] = cnt
    return (torch.empty(int(ws_floats), device=dev) if ws_floats else None), cnt


def _conv4s2(op: int, x, w, gy, out, N, C_in, H, W, Co, inorm=None):
    a = _lib.Conv4s2Args()
    a.N, a.C, a.H, a.W, a.Co = int(N), int(C_in), int(H), int(W), int(Co)
    ws, cnt = _conv_scratch(_lib.load().tp_conv4s2_workspace, a, op, out.device)
    a.x, a.w, a.gy = _ptr(x), _ptr(w), _ptr(gy)
    a.out, a.counters, a.workspace = out.data_ptr(), cnt.data_ptr(), _ptr(ws)
    keep = (x, w, gy, out, ws, cnt)
    if inorm is not None:                             # (xhat, rstd, addend or None, gx, slope, skip_out)
        a.in_xhat, a.in_rstd, a.in_addend, a.in_gx = inorm[0].data_ptr(), inorm[1].data_ptr(), _ptr(inorm[2]), inorm[3].data_ptr()
        a.in_slope, a.skip_out = float(inorm[4]), int(bool(inorm[5]))
        keep += tuple(inorm[:4])
    if op == _lib.CONV_FWD:
        _call("tp_conv4s2_fwd", a)
    elif op == _lib.CONV_DGRAD:
        _launch("tp_conv4s2_dgrad", a, keep=keep)
    else:
        _launch("tp_conv4s2_wgrad", a, keep=keep)
    return out


@_on_tensor_device
def conv4s2_fwd(x: Tensor, w: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """conv2d(x [N,C,H,W], w [Co,C,4,4], stride 2, padding 1) -> [N,Co,H/2,W/2]."""
    x, w = _f32(x, "x"), _f32(w, "w")
    N, C_in, H, W = x.shape
    y = _out_like(out, x, (N, w.shape[0], H // 2, W // 2))
    return _conv4s2(_lib.CONV_FWD, x, w, None, y, N, C_in, H, W, w.shape[0])


def conv4s2_fwd_inorm_supported(x: Tensor) -> bool:
    """The fused convolution + InstanceNorm + LeakyReLU launch covers 4x4 and 8x8 output maps (whole instances per workgroup)."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and (x.shape[2] // 2) * (x.shape[3] // 2) in (16, 64)
            and x.shape[2] == x.shape[3] and not knobs.K.no_conv_inorm)


@_on_tensor_device
def conv4s2_fwd_inorm(x: Tensor, w: Tensor, eps: float, slope: float, y_out: Optional[Tensor] = None, copy_to: Optional[Tensor] = None):
    """-> (y, xhat, rstd) = inorm_lrelu_fwd(conv4s2_fwd(x, w), eps, slope) in ONE launch (the normalisation runs in the epilogue of
    the workgroup that holds an instance's split-K totals); ``y_out`` as in inorm_lrelu_fwd.  ``copy_to`` (shaped like x, contiguous):
    the launch also leaves a copy of x there."""
    x, w = _f32(x, "x"), _f32(w, "w")
    N, C_in, H, W = x.shape
    Co = w.shape[0]
    y = _out_like(y_out, x, (N, Co, H // 2, W // 2))
    xhat, rstd = torch.empty(N, Co, H // 2, W // 2, device=x.device), torch.empty(N * Co, device=x.device)
    a = _lib.Conv4s2Args()
    a.N, a.C, a.H, a.W, a.Co = int(N), int(C_in), int(H), int(W), int(Co)
    ws, cnt = _conv_scratch(lambda args, _op, n: _lib.load().tp_conv4s2_fwd_inorm_workspace(args, n), a, 0, x.device)
    a.x, a.w = x.data_ptr(), w.data_ptr()
    a.out, a.counters, a.workspace = y.data_ptr(), cnt.data_ptr(), _ptr(ws)
    if copy_to is not None:
        if copy_to.shape != x.shape or copy_to.dtype != torch.float32 or not copy_to.is_contiguous() or copy_to.device != x.device:
            raise ValueError("conv4s2_fwd_inorm: copy_to must be a contiguous float32 tensor shaped like x")
        a.x_copy = copy_to.data_ptr()
    _launch("tp_conv4s2_fwd_inorm", a, (xhat.data_ptr(), rstd.data_ptr(), float(eps), float(slope)), keep=(x, w, y, xhat, rstd, ws, cnt, copy_to))
    return y, xhat, rstd


def conv4s2_dgrad_inorm_supported(gy: Tensor) -> bool:
    """The data gradient can carry the InstanceNorm + LeakyReLU backward of the stage in front of it: 8x8 input maps (whole instances
    per workgroup)."""
    return gy.is_cuda and gy.dim() == 4 and tuple(gy.shape[-2:]) == (4, 4) and not knobs.K.no_dgrad_inorm


@_on_tensor_device
def conv4s2_dgrad(gy: Tensor, w: Tensor, out: Optional[Tensor] = None, inorm=None):
    """gradient of conv4s2_fwd wrt x: gy [N,Co,H/2,W/2], w [Co,C,4,4] -> [N,C,H,W].
    ``inorm`` = dict(xhat [N,C,8,8], rstd [N*C], slope, addend=None, out=None, keep=True) (conv4s2_dgrad_inorm_supported): the
    InstanceNorm + LeakyReLU backward of the stage in front of the convolution in the same launch -- returns (data gradient or None if
    not ``keep``, inorm_lrelu_bwd(xhat, rstd, data gradient, slope, addend, out)), bit-identical to the two launches."""
    gy, w = _f32(gy, "gy"), _f32(w, "w")
    N, Co, OH, OW = gy.shape
    gx = _out_like(out, gy, (N, w.shape[1], 2 * OH, 2 * OW))
    if inorm is None:
        return _conv4s2(_lib.CONV_DGRAD, None, w, gy, gx, N, w.shape[1], 2 * OH, 2 * OW, Co)
    xhat, rstd = _f32(inorm["xhat"], "xhat"), _f32(inorm["rstd"], "rstd")
    if tuple(xhat.shape) != (N, w.shape[1], 8, 8) or (OH, OW) != (4, 4) or rstd.numel() != N * w.shape[1]:
        raise ValueError("conv4s2_dgrad(inorm=): xhat [N,C,8,8] / rstd [N*C] of the stage in front of the convolution expected")
    addend = _f32(inorm["addend"], "addend") if inorm.get("addend") is not None else None
    cz = _out_like(inorm.get("out"), xhat)
    keep = bool(inorm.get("keep", True))
    _conv4s2(_lib.CONV_DGRAD, None, w, gy, gx, N, w.shape[1], 2 * OH, 2 * OW, Co,
             inorm=(xhat, rstd, addend, cz, inorm["slope"], not keep))
    return (gx if keep else None), cz


@_on_tensor_device
def conv4s2_wgrad(gy: Tensor, x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """gradient of conv4s2_fwd wrt w: gy [N,Co,H/2,W/2], x [N,C,H,W] -> [Co,C,4,4] (a sum over the N samples: several
    (gy, x) pairs stacked along N give the sum of their weight gradients in one launch)."""
    gy, x = _f32(gy, "gy"), _f32(x, "x")
    N, C_in, H, W = x.shape
    gw = _out_like(out, x, (gy.shape[1], C_in, 4, 4))
    return _conv4s2(_lib.CONV_WGRAD, x, None, gy, gw, N, C_in, H, W, gy.shape[1])


@_on_tensor_device
def bce_logits_fwd(x: Tensor, target: float) -> Tensor:
    x = _f32(x, "x")
    out = torch.empty((), device=x.device)
    _call("tp_bce_logits_fwd", x.data_ptr(), x.numel(), float(target), out.data_ptr())
    return out


@_on_tensor_device
def bce_logits_bwd(x: Tensor, target: float, g: Tensor) -> Tensor:
    x, g = _f32(x, "x"), _f32(g, "g")
    gx = torch.empty_like(x)
    _call("tp_bce_logits_bwd", x.data_ptr(), x.numel(), float(target), g.data_ptr(), gx.data_ptr())
    return gx


@_on_tensor_device
def disc_inputs(rgb: Tensor, gathered: Tensor, hw, geo: bool, stacked: bool = False):
    """(real, fake) [B, 3 or 9, h, w] of the discriminator step from the render output and the gathered patches (K13).
    ``stacked``: `real` is returned as the first half of a [2B, ...] buffer (returned in its place) whose second half the
    explicit discriminator-step schedule fills with the R1 cotangent: its first weight gradient then sums both pairs in one launch."""
    rgb, gathered = _f32(rgb.detach(), "rgb"), _f32(gathered, "gathered")
    B, P = rgb.shape[0], rgb.shape[1]
    if gathered.numel() != B * 14 * P:
        raise ValueError("disc_inputs: gathered [B,14,h,w] expected")
    nc = 9 if geo else 3
    real, fake = torch.empty(2 * B if stacked else B, nc, hw[0], hw[1], device=rgb.device), torch.empty(B, nc, hw[0], hw[1], device=rgb.device)
    _call("tp_disc_inputs", rgb.data_ptr(), gathered.data_ptr(), B, P, int(bool(geo)), real.data_ptr(), fake.data_ptr())
    return real, fake


@_on_tensor_device
def fake_patch_bwd(g_fake: Tensor, B: int, P: int) -> Tensor:
    """g_rgb [B,P,3] from the cotangent of the fake stack [B,nc,h,w] (channels 0..2, transposed)."""
    g_fake = _f32(g_fake, "g_fake")
    g_rgb = torch.empty(B, P, 3, device=g_fake.device)
    _call("tp_fake_patch_bwd", g_fake.data_ptr(), B, P, g_fake.shape[1], g_rgb.data_ptr())
    return g_rgb


@_on_tensor_device
def sumsq_mean_fwd(g: Tensor) -> Tensor:
    """sum(g^2) / B for g [B,...] -> 0-dim tensor."""
    g = _f32(g, "g")
    out = torch.empty((), device=g.device)
    _call("tp_sumsq_mean_fwd", g.data_ptr(), g.numel(), g.shape[0], out.data_ptr())
    return out


@_on_tensor_device
def sumsq_mean_bwd(g: Tensor, cot: Tensor) -> Tensor:
    g, cot = _f32(g, "g"), _f32(cot, "cot")
    out = torch.empty_like(g)
    _call("tp_sumsq_mean_bwd", g.data_ptr(), g.numel(), g.shape[0], cot.data_ptr(), out.data_ptr())
    return out


@_on_tensor_device
def sumsq_mean_fwd_bwd(g: Tensor, w: float, out_g: Optional[Tensor] = None):
    """([sum(g^2) / B, w sum(g^2) / B], 2 w g / B) for g [B, ...] in one launch: value, weighted value (what the reference logs) and
    weighted gradient of the R1 penalty (K16)."""
    g = _f32(g, "g")
    out, og = torch.empty(2, device=g.device), _out_like(out_g, g)
    _call("tp_sumsq_mean_fwd_bwd", g.data_ptr(), g.numel(), g.shape[0], float(w), out.data_ptr(), og.data_ptr())
    return out, og


@_on_tensor_device
def gan_disc_losses(d_real: Tensor, d_fake: Tensor, w_real: float, w_fake: float, g_real_out: Optional[Tensor] = None,
                    g_fake_out: Optional[Tensor] = None):
    """Both GAN-loss terms of the discriminator step and their weighted cotangents in one launch (K16):
    -> (out2 = [bce(d_real, 1), bce(d_fake, 0)], g_real, g_fake)."""
    d_real, d_fake = _f32(d_real, "d_real"), _f32(d_fake, "d_fake")
    if d_real.numel() != d_fake.numel():
        raise ValueError("gan_disc_losses: d_real and d_fake must have the same number of elements")
    out2 = torch.empty(2, device=d_real.device)
    gr, gf = _out_like(g_real_out, d_real), _out_like(g_fake_out, d_fake)
    _call("tp_gan_disc_losses", d_real.data_ptr(), d_fake.data_ptr(), d_real.numel(), float(w_real), float(w_fake), out2.data_ptr(), gr.data_ptr(),
          gf.data_ptr())
    return out2, gr, gf


# ------------------------------------------------------------------------------------------ K14
def _head_args(W1, W2, W3, B, C_z, L, slope):
    a = _lib.DiscHeadArgs()
    H = W2.shape[0]
    if W1.shape != (H, C_z + 2 * L + 1) or W2.shape != (H, H) or W3.numel() != H:
        raise ValueError("disc_head: W1 [H,C+2L+1], W2 [H,H], W3 [1,H] expected")
    a.W1, a.W2, a.W3 = W1.data_ptr(), W2.data_ptr(), W3.data_ptr()
    a.B, a.C, a.L, a.H, a.slope = int(B), int(C_z), int(L), int(H), float(slope)
    return a


@_on_tensor_device
def disc_head_fwd(z: Tensor, scale: Tensor, W1: Tensor, W2: Tensor, W3: Tensor, L: int, slope: float):
    """-> (out [B], t0 [B,C+2L+1], t1 [B,H], t2 [B,H]): the scale-conditioned head of the PatchGAN in one launch."""
    z, scale, W1, W2, W3 = (_f32(t, n) for t, n in ((z, "z"), (scale, "scale"), (W1, "W1"), (W2, "W2"), (W3, "W3")))
    B, C_z = z.shape
    a = _head_args(W1, W2, W3, B, C_z, L, slope)
    dev, H = z.device, W2.shape[0]
    out, t0, t1, t2 = (torch.empty(B, device=dev), torch.empty(B, C_z + 2 * L + 1, device=dev), torch.empty(B, H, device=dev),
                       torch.empty(B, H, device=dev))
    a.z, a.scale, a.out, a.t0, a.t1, a.t2 = z.data_ptr(), scale.data_ptr(), out.data_ptr(), t0.data_ptr(), t1.data_ptr(), t2.data_ptr()
    _call("tp_disc_head_fwd", a)
    return out, t0, t1, t2


@_on_tensor_device
def disc_head_bwd(g_out: Tensor, t0: Tensor, t1: Tensor, t2: Tensor, W1: Tensor, W2: Tensor, W3: Tensor, C_z: int, L: int, slope: float,
                  weight_grads: bool = True, accumulate_into=None, gz_out: Optional[Tensor] = None):
    """-> (gz [B,C], gW1, gW2, gW3, e1, e2).  ``weight_grads=False``: data gradient only (gW1..3 = None);
    ``accumulate_into=(gW1, gW2, gW3)``: the weight gradients are ADDED to these tensors (and they are what is returned)."""
    g_out, W1, W2, W3 = _f32(g_out, "g_out"), _f32(W1, "W1"), _f32(W2, "W2"), _f32(W3, "W3")
    B, H, dev = t1.shape[0], t1.shape[1], t1.device
    a = _head_args(W1, W2, W3, B, C_z, L, slope)
    gz, e1, e2 = _out_like(gz_out, t1, (B, C_z)), torch.empty(B, H, device=dev), torch.empty(B, H, device=dev)
    gW1 = gW2 = gW3 = None
    if accumulate_into is not None:
        gW1, gW2, gW3 = (_out_like(g, W) for g, W in zip(accumulate_into, (W1, W2, W3)))
        a.accumulate_gw = 1
    elif weight_grads:
        gW1, gW2, gW3 = torch.empty_like(W1), torch.empty_like(W2), torch.empty_like(W3)
    a.g_out, a.t0, a.t1, a.t2, a.e1, a.e2, a.out = (g_out.data_ptr(), t0.data_ptr(), t1.data_ptr(), t2.data_ptr(), e1.data_ptr(),
                                                    e2.data_ptr(), gz.data_ptr())
    a.gW1, a.gW2, a.gW3 = _ptr(gW1), _ptr(gW2), _ptr(gW3)
    _call("tp_disc_head_bwd", a)
    return gz, gW1, gW2, gW3, e1, e2


@_on_tensor_device
def disc_head_bwd_bwd(c_gz: Tensor, g_out: Tensor, t0: Tensor, t1: Tensor, t2: Tensor, e1: Tensor, e2: Tensor, W1: Tensor, W2: Tensor,
                      W3: Tensor, L: int, slope: float):
    """cotangent c_gz [B,C] of the backward's gz -> (d/d g_out [B], d/d W1, d/d W2, d/d W3)."""
    c_gz, g_out, W1, W2, W3 = _f32(c_gz, "c_gz"), _f32(g_out, "g_out"), _f32(W1, "W1"), _f32(W2, "W2"), _f32(W3, "W3")
    B, C_z = c_gz.shape
    a = _head_args(W1, W2, W3, B, C_z, L, slope)
    gg = torch.empty(B, device=c_gz.device)
    gW1, gW2, gW3 = torch.empty_like(W1), torch.empty_like(W2), torch.empty_like(W3)
    a.c_gz, a.g_out, a.t0, a.t1, a.t2, a.e1, a.e2, a.out = (c_gz.data_ptr(), g_out.data_ptr(), t0.data_ptr(), t1.data_ptr(),
                                                            t2.data_ptr(), e1.data_ptr(), e2.data_ptr(), gg.data_ptr())
    a.gW1, a.gW2, a.gW3 = gW1.data_ptr(), gW2.data_ptr(), gW3.data_ptr()
    _call("tp_disc_head_bwd_bwd", a)
    return gg, gW1, gW2, gW3


# ------------------------------------------------------------------------------------------ K17
DISC_TAIL_MAX_ROWS = _lib.DISC_TAIL_MAX_ROWS
_tail_ws = {}                # (device index, stream) -> workspace tensor of the split-K partial sums


def disc_tail_eligible(a: Tensor, W0: Tensor, extra_rows: int = 0) -> bool:
    """The fused tail (K17) takes up to 16 rows (and 16 extra weight-gradient rows), K a multiple of 4, fp32 device tensors."""
    return (a.is_cuda and a.dtype == torch.float32 and a.dim() == 2 and a.shape[0] <= DISC_TAIL_MAX_ROWS and extra_rows <= DISC_TAIL_MAX_ROWS
            and a.shape[1] % 4 == 0 and W0.shape[1] == a.shape[1] and not knobs.K.no_disc_tail)


def _tail_args(W0, W1, W2, W3, M, L, slope):
    a = _lib.DiscTailArgs()
    N, K = W0.shape
    H = W2.shape[0]
    if W1.shape != (H, N + 2 * L + 1) or W2.shape != (H, H) or W3.numel() != H:
        raise ValueError("disc_tail: W0 [N,K], W1 [H,N+2L+1], W2 [H,H], W3 [1,H] expected")
    a.W0, a.W1, a.W2, a.W3 = W0.data_ptr(), W1.data_ptr(), W2.data_ptr(), W3.data_ptr()
    a.M, a.M2, a.K, a.N, a.L, a.H, a.slope = int(M), 0, int(K), int(N), int(L), int(H), float(slope)
    return a


def _tail_workspace(dev, N):
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, N, _pair_slot())
    ws = _tail_ws.get(key)
    if ws is None:
        ws = _tail_ws[key] = torch.empty(int(_lib.load().tp_disc_tail_workspace_bytes(N)) // 4, device=dev)
    return ws


@_on_tensor_device
def disc_tail_fwd(a: Tensor, W0: Tensor, scale: Tensor, W1: Tensor, W2: Tensor, W3: Tensor, L: int, slope: float):
    """a [M,K] -> (out [M], t0 [M,N+2L+1], t1 [M,H], t2 [M,H]): full-map convolution + scale-conditioned head, one launch."""
    a, W0, scale, W1, W2, W3 = (_f32(t, n) for t, n in ((a, "a"), (W0, "W0"), (scale, "scale"), (W1, "W1"), (W2, "W2"), (W3, "W3")))
    M, dev = a.shape[0], a.device
    q = _tail_args(W0, W1, W2, W3, M, L, slope)
    out, t0, t1, t2 = (torch.empty(M, device=dev), torch.empty(M, q.N + 2 * L + 1, device=dev), torch.empty(M, q.H, device=dev),
                       torch.empty(M, q.H, device=dev))
    ws = _tail_workspace(dev, q.N)
    q.a, q.scale, q.out, q.t0, q.t1, q.t2 = a.data_ptr(), scale.data_ptr(), out.data_ptr(), t0.data_ptr(), t1.data_ptr(), t2.data_ptr()
    q.workspace, q.ticket = ws.data_ptr(), _ticket(dev, "disc_tail%d" % _pair_slot())
    _launch("tp_disc_tail_fwd", q, keep=(a, W0, scale, W1, W2, W3, out, t0, t1, t2, ws))
    return out, t0, t1, t2


@_on_tensor_device
def disc_tail_bwd(g_out: Tensor, t0: Tensor, t1: Tensor, t2: Tensor, W0: Tensor, W1: Tensor, W2: Tensor, W3: Tensor, L: int, slope: float,
                  a: Optional[Tensor] = None, want_c_a: bool = True, want_gW0: bool = True, head_weight_grads: bool = True,
                  accumulate_into=None, want_e: bool = False, gz_out: Optional[Tensor] = None, gy2: Optional[Tensor] = None,
                  a2: Optional[Tensor] = None, c_a_out: Optional[Tensor] = None, inorm=None):
    """The tail's backward in one launch -> dict(c_a [M,K], gW0 [N,K], gW1, gW2, gW3, gz [M,N], e1, e2) (absent entries None).
    ``a`` [M,K]: the ladder output (needed for gW0); ``gy2`` [M2,N] / ``a2`` [M2,K]: a second (cotangent, input) pair of the same
    weight whose rows join gW0's sum; ``accumulate_into=(gW1, gW2, gW3)``: the head's weight gradients are ADDED to these.
    ``inorm`` = dict(xhat [M,C,h,w], rstd [M*C], addend=None, out=None): the InstanceNorm + LeakyReLU backward of the ladder's last stage
    (ops.inorm_lrelu_bwd) applied to c_a inside the launch -> res["c_z"] (shaped like xhat); c_a itself only with ``want_c_a``."""
    g_out, W0, W1, W2, W3 = (_f32(t, n) for t, n in ((g_out, "g_out"), (W0, "W0"), (W1, "W1"), (W2, "W2"), (W3, "W3")))
    M, dev = t1.shape[0], t1.device
    q = _tail_args(W0, W1, W2, W3, M, L, slope)
    res = dict(c_a=None, gW0=None, gW1=None, gW2=None, gW3=None, gz=None, e1=None, e2=None, c_z=None)
    keep = []
    if want_c_a:
        res["c_a"] = _out_like(c_a_out, t1, (M, q.K))
    if inorm is not None:
        xhat, rstd = _f32(inorm["xhat"], "xhat"), _f32(inorm["rstd"], "rstd")
        in_P = xhat.shape[-2] * xhat.shape[-1]
        if xhat.numel() != M * q.K or rstd.numel() * in_P != M * q.K:
            raise ValueError("disc_tail_bwd: xhat / rstd of the last ladder stage expected")
        res["c_z"] = _out_like(inorm.get("out"), xhat)
        q.in_xhat, q.in_rstd, q.c_z, q.in_P = xhat.data_ptr(), rstd.data_ptr(), res["c_z"].data_ptr(), int(in_P)
        if inorm.get("addend") is not None:
            ad = _f32(inorm["addend"], "addend")
            keep.append(ad)
            q.in_addend = ad.data_ptr()
        keep += [xhat, rstd]
    if want_gW0:
        if a is None:
            raise ValueError("disc_tail_bwd: the weight gradient of the full-map convolution needs the ladder output")
        a = _f32(a, "a")
        res["gW0"] = torch.empty(q.N, q.K, device=dev)
        q.a = a.data_ptr()
        if gy2 is not None:
            gy2, a2 = _f32(gy2, "gy2"), _f32(a2, "a2")
            keep += [gy2, a2]
            q.gy2, q.a2, q.M2 = gy2.data_ptr(), a2.data_ptr(), gy2.shape[0]
    if accumulate_into is not None:
        res["gW1"], res["gW2"], res["gW3"] = (_out_like(g, W) for g, W in zip(accumulate_into, (W1, W2, W3)))
        q.accumulate_gw = 1
    elif head_weight_grads:
        res["gW1"], res["gW2"], res["gW3"] = torch.empty_like(W1), torch.empty_like(W2), torch.empty_like(W3)
    if want_e:
        res["e1"], res["e2"] = torch.empty(M, q.H, device=dev), torch.empty(M, q.H, device=dev)
    if gz_out is not None:
        res["gz"] = _out_like(gz_out, t1, (M, q.N))
    q.g_out, q.t0, q.t1, q.t2 = g_out.data_ptr(), t0.data_ptr(), t1.data_ptr(), t2.data_ptr()
    q.c_a, q.gW0, q.gW1, q.gW2, q.gW3 = (_ptr(res[k]) for k in ("c_a", "gW0", "gW1", "gW2", "gW3"))
    q.gz, q.e1, q.e2 = _ptr(res["gz"]), _ptr(res["e1"]), _ptr(res["e2"])
    _launch("tp_disc_tail_bwd", q, keep=(g_out, t0, t1, t2, W0, W1, W2, W3, a, keep, dict(res)))
    return res


@_on_tensor_device
def disc_tail_bwd_bwd(c: Tensor, g_out: Tensor, t0: Tensor, t1: Tensor, t2: Tensor, e1: Tensor, e2: Tensor, W0: Tensor, W1: Tensor,
                      W2: Tensor, W3: Tensor, L: int, slope: float, want_gg: bool = False):
    """R1 second pass through the tail: cotangent c [M,K] of the first pass' data gradient -> (gW1, gW2, gW3[, d/d g_out])."""
    c, g_out, W0, W1, W2, W3 = (_f32(t, n) for t, n in ((c, "c"), (g_out, "g_out"), (W0, "W0"), (W1, "W1"), (W2, "W2"), (W3, "W3")))
    M, dev = c.shape[0], c.device
    q = _tail_args(W0, W1, W2, W3, M, L, slope)
    gW1, gW2, gW3 = torch.empty_like(W1), torch.empty_like(W2), torch.empty_like(W3)
    gg = torch.empty(M, device=dev) if want_gg else None
    ws = _tail_workspace(dev, q.N)
    q.a, q.g_out, q.t0, q.t1, q.t2, q.e1, q.e2 = (c.data_ptr(), g_out.data_ptr(), t0.data_ptr(), t1.data_ptr(), t2.data_ptr(), e1.data_ptr(),
                                                  e2.data_ptr())
    q.gW1, q.gW2, q.gW3, q.out = gW1.data_ptr(), gW2.data_ptr(), gW3.data_ptr(), _ptr(gg)
    q.workspace, q.ticket = ws.data_ptr(), _ticket(dev, "disc_tail")
    _call("tp_disc_tail_bwd_bwd", q)
    return (gW1, gW2, gW3, gg) if want_gg else (gW1, gW2, gW3)


# ------------------------------------------------------------------------------------------ K15
SKINNY_MAX_ROWS = 256


@_on_tensor_device
def skinny_linear_fwd(x: Tensor, w: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """x [M,K] @ w [N,K]^T -> [M,N] for a handful of rows (K15)."""
    x, w = _f32(x, "x"), _f32(w, "w")
    y = _out_like(out, x, (x.shape[0], w.shape[0]))
    _call("tp_skinny_linear_fwd", x.data_ptr(), w.data_ptr(), y.data_ptr(), x.shape[0], w.shape[0], x.shape[1])
    return y


SKINNY_DGRAD_MAX_ROWS = 16



@_on_tensor_device
def skinny_linear_dgrad(gy: Tensor, w: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """gy [M,N] @ w [N,K] -> [M,K]: K15's own kernel (tp_skinny_linear_dgrad) for up to 16 rows -- every batch size of BASELINE's
    configurations -- so that the discriminator pass contains no library kernel in its autograd form either (the captured default
    iteration never reaches this function: its explicit schedule uses the fused tail K17).  TP_SKINNY_DGRAD_MM=1 selects rocBLAS
    (0.7 % faster per autograd-form iteration: 671-677 vs 664-669 it/s, round 5); more than 16 rows always take it."""
    if gy.shape[0] > SKINNY_DGRAD_MAX_ROWS or knobs.K.skinny_dgrad_mm:
        return torch.mm(gy, w, out=out) if out is not None else torch.mm(gy, w)
    gy, w = _f32(gy, "gy"), _f32(w, "w")
    gx = _out_like(out, gy, (gy.shape[0], w.shape[1]))
    _call("tp_skinny_linear_dgrad", gy.data_ptr(), w.data_ptr(), gx.data_ptr(), gy.shape[0], w.shape[0], w.shape[1])
    return gx


@_on_tensor_device
def skinny_linear_wgrad(gy: Tensor, x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """gy [M,N]^T @ x [M,K] -> [N,K]."""
    gy, x = _f32(gy, "gy"), _f32(x, "x")
    if x.shape[0] > SKINNY_MAX_ROWS:
        raise ValueError("skinny_linear_wgrad: at most %d rows" % SKINNY_MAX_ROWS)
    gw = _out_like(out, x, (gy.shape[1], x.shape[1]))
    _call("tp_skinny_linear_wgrad", gy.data_ptr(), x.data_ptr(), gw.data_ptr(), x.shape[0], gy.shape[1], x.shape[1])
    return gw
