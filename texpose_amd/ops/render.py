"""K1-K5, K13: ray generation, the MLP and its fp16 range flag, the composite, the patch gather and sampler, the evaluation render."""
from typing import Dict, Optional, Tuple

import torch

from .. import _lib, knobs
from .._lib import (BOUNDS_AABB, BOUNDS_MAP, BOUNDS_NONE, CompositeArgs, CompositeBwdArgs, JITTER_GIVEN, JITTER_MID, MLP_F16, MLP_F16X3, MLP_FP32,
                    MlpBwdArgs, MlpFwdArgs, MlpWeights, PACK_ALL, PACK_F16, PACK_F16X3, PACK_HEADS, PACK_RAYBIAS, PACK_TRUNK, PIX_COORDS, PIX_INDEX,
                    PatchGatherArgs, RaygenArgs)
from ._base import Tensor, _call, _f32, _float3, _on_tensor_device, _ptr

__all__ = ["DEPTH_PARAMS", "PRECISIONS", "F16_RANGE_PRECISIONS", "INFERENCE_ONLY_PRECISIONS", "COMPOSITE_RAY_FIELDS", "raygen", "aabb_intersect",
           "sample_depth", "packed_bytes", "pack_weights", "packed_t_bytes", "pack_heads_train", "_workspaces", "_workspace", "_status_words",
           "RANGE_MESSAGE", "mlp_status", "_act_max_words", "_track_act_max", "track_activation_max", "take_activation_max", "_act_max_ptr",
           "take_mlp_status", "check_mlp_status", "_status_polls", "poll_mlp_status", "mlp_forward", "ray_bias_applies", "_bwd_scratch",
           "mlp_backward", "posenc", "_composite_args", "composite_fwd", "composite_bwd", "patch_gather", "eval_metrics", "render_eval", "_lattices",
           "patch_coords", "latent_rows_fwd", "latent_rows_bwd"]

DEPTH_PARAMS = {"metric": _lib.DEPTH_METRIC, "inverse": _lib.DEPTH_INVERSE}          # options nerf.depth.param -> TP_DEPTH_*
# "f16": single fp16 products with fp32 accumulation, inference only (include/texpose_amd.h, TP_MLP_F16)
PRECISIONS = {"fp32": MLP_FP32, "f16x3": MLP_F16X3, "f16": MLP_F16}
# the arithmetics whose forward raises the fp16 range flag (mlp_status) and whose training forms do not exist
F16_RANGE_PRECISIONS = ("f16x3", "f16")
INFERENCE_ONLY_PRECISIONS = ("f16",)

COMPOSITE_RAY_FIELDS = (("rgb", 0, 3), ("rgb_static", 3, 6), ("rgb_transient", 6, 9), ("depth", 9, 10),
                        ("opacity", 10, 11), ("opacity_static", 11, 12), ("opacity_transient", 12, 13),
                        ("uncert", 13, 14))


# ------------------------------------------------------------------------------------------ K1
@_on_tensor_device
def raygen(intr: Tensor, pose: Tensor, *, H: int, W: int, n_samples: int = 0, coords: Optional[Tensor] = None,
           ray_idx: Optional[Tensor] = None, z_near: Optional[Tensor] = None, z_far: Optional[Tensor] = None,
           aabb: Optional[Tuple[Tuple[float, float, float], Tuple[float, float, float]]] = None,
           bg_range: Tuple[float, float] = (0.0, 30.0), rand: Optional[Tensor] = None,
           jitter: int = JITTER_MID, seed: int = 0, offset: int = 0, valid_rect: Optional[Tensor] = None,
           offset_dev: Optional[Tensor] = None, ndc: bool = False, depth_param: str = "metric",
           sampler: Optional[dict] = None, rows: Optional[dict] = None):
    """Fused ray-gen + bounds + stratified depths.  Returns (center, ray, near, far, depth);
    near/far/depth are None when no bounds source is given, depth is [B,R,N].  ``offset_dev`` (int64 [1] on the device): added
    to the Philox ``offset`` inside the kernel (the step counter of a captured training step).  ``ndc``: centre / ray in normalised
    device coordinates (camera.py:325-342; the bounds still come from the metric rays, as in the reference); ``depth_param``
    'inverse': depth = 1 / (sample + 1e-8) (model/nerf_adapt_st_gan.py:699).
    Training step (tp_raygen_train): ``sampler`` (a `patch_coords(..., defer=True)` job; give its `coords` tensor as ``coords``): the launch
    draws the patch coordinates itself and fills the job's coords / scales; ``rows`` (a `latent_rows_fwd(..., defer=True)` job): extra
    workgroups of the launch gather the latent rows.  Same values as the separate launches."""
    intr, pose = _f32(intr, "intr"), _f32(pose, "pose")
    B = pose.shape[0]
    a = RaygenArgs()
    if coords is not None:
        coords = _f32(coords, "coords")
        R = coords.numel() // (2 * B)
        a.pixel_mode, a.coords = PIX_COORDS, coords.data_ptr()
    else:
        ray_idx = ray_idx.to(torch.int64).contiguous()
        R = ray_idx.numel() // B
        a.pixel_mode, a.ray_idx = PIX_INDEX, ray_idx.data_ptr()
    dev = pose.device
    center = torch.empty(B, R, 3, device=dev)
    ray = torch.empty(B, R, 3, device=dev)
    near = far = depth = None
    if aabb is not None:
        a.bounds_mode = BOUNDS_AABB
        a.aabb_min, a.aabb_max = _float3(aabb[0]), _float3(aabb[1])
        a.bg_near, a.bg_far = float(bg_range[0]), float(bg_range[1])
        if valid_rect is not None:                      # [B,4] (x0,y0,x1,y1): pixels outside get the fallback range
            valid_rect = _f32(valid_rect, "valid_rect")
            assert valid_rect.shape == (B, 4)
            a.valid_rect = valid_rect.data_ptr()
    elif z_near is not None:
        z_near, z_far = _f32(z_near, "z_near"), _f32(z_far, "z_far")
        assert z_near.numel() == B * H * W and z_far.numel() == B * H * W
        a.bounds_mode, a.z_near, a.z_far = BOUNDS_MAP, z_near.data_ptr(), z_far.data_ptr()
    else:
        a.bounds_mode = BOUNDS_NONE
    if a.bounds_mode != BOUNDS_NONE:
        near = torch.empty(B, R, device=dev)
        far = torch.empty(B, R, device=dev)
        a.near, a.far = near.data_ptr(), far.data_ptr()
        if n_samples > 0:
            depth = torch.empty(B, R, n_samples, device=dev)
            a.depth = depth.data_ptr()
    if rand is not None:
        rand = _f32(rand, "rand")
        assert rand.numel() == B * R * n_samples
        jitter = JITTER_GIVEN
        a.rand = rand.data_ptr()
    a.jitter_mode, a.seed, a.offset = jitter, seed, offset
    a.ndc, a.depth_param = int(bool(ndc)), DEPTH_PARAMS[depth_param]
    if offset_dev is not None:
        if offset_dev.dtype != torch.int64 or offset_dev.numel() != 1 or offset_dev.device != dev:
            raise ValueError("raygen: offset_dev must be one int64 word on the device of the inputs")
        a.offset_dev = offset_dev.data_ptr()
    a.intr, a.pose = intr.data_ptr(), pose.data_ptr()
    a.B, a.R, a.H, a.W, a.N = B, R, H, W, n_samples
    a.center, a.ray = center.data_ptr(), ray.data_ptr()
    if sampler is None and rows is None:
        _call("tp_raygen", a)
        return center, ray, near, far, depth
    sj = rj = None
    if sampler is not None:
        if coords is None or coords.data_ptr() != sampler["coords"].data_ptr() or sampler["B"] != B:
            raise ValueError("raygen: a sampler job fills ITS coords tensor -- pass that tensor as coords")
        sj = _lib.PatchSamplerJob()
        lo = sampler["lo"]
        sj.u, sj.p, sj.lattice = _ptr(sampler["u"]), sampler["p"], sampler["lattice"].data_ptr()
        sj.lo_dev = lo.data_ptr() if torch.is_tensor(lo) else None
        sj.lo_host = 0.0 if torch.is_tensor(lo) else float(lo)
        sj.span_host, sj.hi = float(sampler["hi"]) - sj.lo_host, float(sampler["hi"])
        sj.random_scale, sj.random_shift = int(bool(sampler["random_scale"])), int(bool(sampler["random_shift"]))
        sj.seed, sj.counter = int(sampler["seed"]) & (2 ** 64 - 1), _ptr(sampler["counter"])
        sj.coords, sj.scales = sampler["coords"].data_ptr(), sampler["scales"].data_ptr()
    if rows is not None:
        rj = _lib.LatentRowsJob()
        rj.w_trans, rj.w_light, rj.idx = rows["w_trans"].data_ptr(), rows["w_light"].data_ptr(), rows["idx"].data_ptr()
        rj.B, rj.C_trans, rj.C_light = rows["idx"].numel(), rows["w_trans"].shape[1], rows["w_light"].shape[1]
        rj.out_trans, rj.out_light, rj.idx_copy = rows["out_trans"].data_ptr(), rows["out_light"].data_ptr(), _ptr(rows["idx_copy"])
    _call("tp_raygen_train", a, sj, rj)
    return center, ray, near, far, depth


@_on_tensor_device
def aabb_intersect(aabb_min, aabb_max, o: Tensor, d: Tensor):
    o, d = _f32(o, "ray_o"), _f32(d, "ray_d")
    n = o.numel() // 3
    tn = torch.empty(o.shape[:-1], device=o.device)
    tf = torch.empty_like(tn)
    ok = torch.empty(o.shape[:-1], device=o.device, dtype=torch.uint8)
    lo, hi = _float3(torch.as_tensor(aabb_min).flatten().tolist()), _float3(torch.as_tensor(aabb_max).flatten().tolist())
    _call("tp_aabb", lo, hi, o.data_ptr(), d.data_ptr(), n, tn.data_ptr(), tf.data_ptr(), ok.data_ptr())
    return tn, tf, ok.bool()


@_on_tensor_device
def sample_depth(near: Tensor, far: Tensor, n_samples: int, rand: Optional[Tensor] = None, jitter: int = JITTER_MID,
                 seed: int = 0, offset: int = 0, depth_param: str = "metric") -> Tensor:
    near, far = _f32(near, "near"), _f32(far, "far")
    if rand is not None:
        rand, jitter = _f32(rand, "rand"), JITTER_GIVEN
    depth = torch.empty(*near.shape, n_samples, device=near.device)
    _call("tp_sample_depth", near.data_ptr(), far.data_ptr(), _ptr(rand), jitter, seed, offset, near.numel(), n_samples, DEPTH_PARAMS[depth_param],
          depth.data_ptr())
    return depth


# ------------------------------------------------------------------------------------------ K2
def packed_bytes() -> int:
    return int(_lib.load().tp_mlp_packed_bytes())


@_on_tensor_device
def pack_weights(state: Dict[str, Tensor], packed: Optional[Tensor] = None, parts: int = PACK_ALL,
                 prefix: str = "", precision: str = "fp32", ray_bias: bool = False) -> Tensor:
    """state: reference state-dict style mapping (``mlp_feat.0.weight`` ...) of CUDA tensors.
    precision 'f16x3' builds the split-fp16 stream for the fast forward, 'f16' the single-fp16 stream of the inference-only
    forward (same size); ``ray_bias``: their variant for mlp_forward(..., ray_bias=True) (tp_mlp_fwd_args.ray_bias)."""
    w = MlpWeights()
    keep = []

    def put(arr_w, arr_b, name, n):
        for i in range(n):
            wt, bt = _f32(state[f"{prefix}{name}.{i}.weight"], name), _f32(state[f"{prefix}{name}.{i}.bias"], name)
            keep.extend((wt, bt))
            arr_w[i], arr_b[i] = wt.data_ptr(), bt.data_ptr()

    if parts & PACK_TRUNK:
        put(w.feat_w, w.feat_b, "mlp_feat", 8)
    if parts & PACK_HEADS:
        put(w.rgb_w, w.rgb_b, "mlp_rgb", 4)
        put(w.trans_w, w.trans_b, "mlp_trans", 4)
    dev = keep[0].device
    if packed is None:
        packed = torch.empty(packed_bytes() // 4, device=dev)
    flags = parts | {MLP_FP32: 0, MLP_F16X3: PACK_F16X3, MLP_F16: PACK_F16}[PRECISIONS[precision]] | (PACK_RAYBIAS if ray_bias else 0)
    _call("tp_mlp_pack", w, flags, packed.data_ptr())
    return packed


def packed_t_bytes() -> int:
    return int(_lib.load().tp_mlp_packed_t_bytes())


@_on_tensor_device
def pack_heads_train(state: Dict[str, Tensor], packed: Tensor, packed_t: Optional[Tensor], prefix: str = "") -> None:
    """Training with the f16x3 kernels: the head part of the forward stream ``packed`` (chunks + biases) and the transposed image
    ``packed_t`` of the data-gradient kernel from the head weights in ONE launch (tp_mlp_pack_heads_f16x3) -- what
    pack_weights(PACK_HEADS, 'f16x3') and the repack of mlp_backward do in three."""
    w = MlpWeights()
    keep = []
    for name, arr_w, arr_b in (("mlp_rgb", w.rgb_w, w.rgb_b), ("mlp_trans", w.trans_w, w.trans_b)):
        for i in range(4):
            wt, bt = _f32(state[f"{prefix}{name}.{i}.weight"], name), _f32(state[f"{prefix}{name}.{i}.bias"], name)
            keep.extend((wt, bt))
            arr_w[i], arr_b[i] = wt.data_ptr(), bt.data_ptr()
    _call("tp_mlp_pack_heads_f16x3", w, packed.data_ptr(), _ptr(packed_t))


_workspaces: Dict[Tuple[int, int], Tensor] = {}


def _workspace(n_samples: int, dev: torch.device) -> Tensor:
    need = int(_lib.load().tp_mlp_workspace_bytes(n_samples)) // 4
    key = (dev.index or 0, torch.cuda.current_stream().cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, device=dev)
        _workspaces[key] = ws
    return ws


_status_words: Dict[int, Tensor] = {}
RANGE_MESSAGE = ("f16x3 MLP: an activation exceeded the fp16 range (6e4); render with precision='fp32' "
                 "(Graph.render_by_slices and the trainers do that by themselves)")


def mlp_status(device) -> Tensor:
    """int32 device word; bit 0 is raised by the f16x3 forward if an activation left the fp16 range."""
    key = torch.device(device).index or 0
    if key not in _status_words:
        _status_words[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return _status_words[key]


_act_max_words: Dict[int, Tensor] = {}
_track_act_max = False


def track_activation_max(enable: bool = True) -> None:
    """Diagnostics: let every following f16x3 forward fold its largest hidden activation into a device word
    (tp_mlp_fwd_args.act_max; one atomic per wave and tile).  Off by default."""
    global _track_act_max
    _track_act_max = bool(enable)


def take_activation_max(device) -> float:
    """Largest hidden activation seen by the f16x3 forwards since the last take (blocking read, then cleared).  The range
    guard fires at 6e4."""
    key = torch.device(device).index or 0
    word = _act_max_words.get(key)
    if word is None:
        return 0.0
    value = float(word.view(torch.float32).item())
    word.zero_()
    return value


def _act_max_ptr(dev):
    if not _track_act_max:
        return None
    key = dev.index or 0
    if key not in _act_max_words:
        _act_max_words[key] = torch.zeros(1, dtype=torch.int32, device=dev)
    return _act_max_words[key].data_ptr()


def take_mlp_status(device) -> int:
    """Blocking read-and-clear of the status word: what was raised since the last take.  One host sync."""
    word = mlp_status(device)
    value = int(word.item())
    if value:
        word.zero_()
    return value


def check_mlp_status(device) -> None:
    """Host-synchronising check of the f16x3 range flag; a reported violation is cleared (later renders start clean)."""
    if take_mlp_status(device) & 1:
        raise _lib.TexposeLibraryError(RANGE_MESSAGE)


_status_polls: Dict[int, tuple] = {}


def poll_mlp_status(device, raise_on_flag: bool = True) -> bool:
    """Non-blocking variant: looks at the copy requested by the PREVIOUS poll if it has completed and queues a new
    asynchronous copy of the flag.  A seen violation is cleared on the device (queued on the current stream) and
    either raised or returned as True."""
    key = torch.device(device).index or 0
    prev = _status_polls.get(key)
    seen = False
    if prev is not None and prev[1].query():
        seen = bool(int(prev[0][0]) & 1)
        prev = None
        _status_polls.pop(key, None)
        if seen:
            mlp_status(device).zero_()
            if raise_on_flag:
                raise _lib.TexposeLibraryError(RANGE_MESSAGE)
    if prev is None:
        host = torch.empty(1, dtype=torch.int32, pin_memory=True)
        host.copy_(mlp_status(device), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        _status_polls[key] = (host, ev)
    return seen


@_on_tensor_device
def mlp_forward(packed: Tensor, lat_trans: Tensor, lat_light: Tensor, *, center: Optional[Tensor] = None,
                ray: Optional[Tensor] = None, depth: Optional[Tensor] = None, points: Optional[Tensor] = None,
                ray_unit: Optional[Tensor] = None, save: bool = False, precision: str = "fp32", ray_bias: bool = False,
                saved_out: Optional[Tensor] = None, density_noise: Optional[Tensor] = None):
    """Returns rgb [B,R,N,3,2], density [B,R,N,2], uncert [B,R,N,1] (+ saved activations if save).
    ``density_noise`` [B,R,N]: added to the static density's pre-activation (reference nerf.density_noise_reg, train mode).
    ``packed`` must have been built with the same ``precision`` (and the same ``ray_bias``, see `ray_bias_applies`).
    ``saved_out``: caller-provided record buffer (tp_mlp_saved_bytes floats; its last tile's part zeroed when B*R*N % 128)."""
    lib = _lib.load()
    a = MlpFwdArgs()
    if center is not None:
        center, ray, depth = _f32(center, "center"), _f32(ray, "ray"), _f32(depth, "depth")
        B, R = center.shape[0], center.shape[1]
        N = depth.numel() // (B * R)
        a.center, a.ray, a.depth = center.data_ptr(), ray.data_ptr(), depth.data_ptr()
    else:
        points, ray_unit = _f32(points, "points"), _f32(ray_unit, "ray_unit")
        B, R, N = points.shape[0], points.shape[1], points.shape[2]
        a.points, a.ray_unit = points.data_ptr(), ray_unit.data_ptr()
    lat_trans, lat_light = _f32(lat_trans, "lat_trans"), _f32(lat_light, "lat_light")
    assert lat_trans.shape == (B, 16) and lat_light.shape == (B, 48), (lat_trans.shape, lat_light.shape)
    dev = lat_trans.device
    S = B * R * N
    rgb = torch.empty(B, R, N, 3, 2, device=dev)
    density = torch.empty(B, R, N, 2, device=dev)
    uncert = torch.empty(B, R, N, 1, device=dev)
    saved = None
    if save and saved_out is not None:
        assert saved_out.numel() == int(lib.tp_mlp_saved_bytes(S)) // 4 and saved_out.is_contiguous() and saved_out.dtype == torch.float32
        saved = saved_out
    elif save:
        saved = torch.empty(int(lib.tp_mlp_saved_bytes(S)) // 4, device=dev)
        if S % 128:        # the weight-gradient GEMM contracts whole 32-sample groups: padding must be zero
            saved[-(int(lib.tp_mlp_saved_bytes(128)) // 4):].zero_()
    ws = _workspace(S, dev)
    a.packed, a.lat_trans, a.lat_light = packed.data_ptr(), lat_trans.data_ptr(), lat_light.data_ptr()
    a.B, a.R, a.N = B, R, N
    a.rgb, a.density, a.uncert = rgb.data_ptr(), density.data_ptr(), uncert.data_ptr()
    a.saved, a.workspace = _ptr(saved), ws.data_ptr()
    a.precision = PRECISIONS[precision]
    if precision in INFERENCE_ONLY_PRECISIONS and (save or density_noise is not None):
        raise ValueError("mlp_forward: precision %r is inference only (no save=True, no density_noise)" % precision)
    if precision in F16_RANGE_PRECISIONS:
        a.status = mlp_status(dev).data_ptr()
        a.act_max = _act_max_ptr(dev)
    rb = None
    if ray_bias:
        assert ray_bias_applies(precision, N, save, center is not None), "mlp_forward: ray_bias outside the configuration it covers"
        rb = torch.empty(int(lib.tp_mlp_ray_bias_bytes(B, R)) // 4, device=dev)
        a.ray_bias = rb.data_ptr()
    if density_noise is not None:
        density_noise = _f32(density_noise, "density_noise")
        if density_noise.numel() != B * R * N or density_noise.device != dev:
            raise _lib.TexposeLibraryError("mlp_forward: density_noise must hold one value per sample, on the render's device")
        a.density_noise = density_noise.data_ptr()
    _call("tp_mlp_fwd", a)
    return (rgb, density, uncert, saved) if save else (rgb, density, uncert)


def ray_bias_applies(precision: str, n_samples_per_ray: int, save: bool, center_form: bool) -> bool:
    """The f16x3 and f16 forwards can take the ray-constant inputs of mlp_rgb.0 / mlp_trans.0 as a per-ray bias
    (tp_mlp_fwd_args.ray_bias) when no activation record is written, rays come as (center, ray, depth) and every 128-sample tile
    lies inside one ray.  TP_NO_RAY_BIAS=1 switches it off (same-box A/B)."""
    return (precision in F16_RANGE_PRECISIONS and not save and center_form and n_samples_per_ray % 128 == 0
            and not knobs.K.no_ray_bias)


_bwd_scratch: Dict[Tuple[int, int], Dict[str, Tensor]] = {}


@_on_tensor_device
def mlp_backward(nerf, lat_trans: Tensor, lat_light: Tensor, saved: Tensor, rgb: Tensor, density: Tensor,
                 uncert: Tensor, g_rgb: Optional[Tensor], g_density: Optional[Tensor], g_uncert: Optional[Tensor],
                 wgrad_precision: str = "fp32"):
    """Gradients of the two heads and the latent rows.  Returns dict(params=[...] in the order of
    ``nerf.head_parameters()``, lat_trans=[B,16], lat_light=[B,48]).  ``wgrad_precision='f16x3'`` runs the
    weight-gradient GEMM as split-fp16 products (fp32-grade); only for records of a range-checked f16x3 forward."""
    B, R, N = rgb.shape[0], rgb.shape[1], rgb.shape[2]
    if B > 32:
        raise _lib.TexposeLibraryError("tp_mlp_bwd handles at most 32 images per call")
    dev = rgb.device
    S = B * R * N
    z = lambda like: torch.zeros_like(like)
    g_rgb = z(rgb) if g_rgb is None else _f32(g_rgb, "g_rgb")
    g_density = z(density) if g_density is None else _f32(g_density, "g_density")
    g_uncert = z(uncert) if g_uncert is None else _f32(g_uncert, "g_uncert")
    names, params = zip(*nerf.head_parameters())
    grads = [torch.empty_like(p) for p in params]
    by_name = dict(zip(names, zip(params, grads)))
    a = MlpBwdArgs()
    keep = []
    for i in range(4):
        for head, wf, gwf, gbf in (("mlp_rgb", a.weights.rgb_w, a.g_rgb_w, a.g_rgb_b),
                                   ("mlp_trans", a.weights.trans_w, a.g_trans_w, a.g_trans_b)):
            w, gw = by_name[f"{head}.{i}.weight"]
            _, gb = by_name[f"{head}.{i}.bias"]
            w = _f32(w.detach(), "weight")
            keep.append(w)
            wf[i], gwf[i], gbf[i] = w.data_ptr(), gw.data_ptr(), gb.data_ptr()
    key = (dev.index or 0, torch.cuda.current_stream().cuda_stream)
    sc = _bwd_scratch.setdefault(key, {})
    need = int(_lib.load().tp_mlp_bwd_workspace_bytes(S)) // 4
    if "ws" not in sc or sc["ws"].numel() < need:
        sc["ws"] = torch.empty(need, device=dev)
        sc.pop("clear_for", None)
    lat_trans, lat_light = _f32(lat_trans.detach(), "lat_trans"), _f32(lat_light.detach(), "lat_light")
    g_lt, g_ll = torch.empty(B, 16, device=dev), torch.empty(B, 48, device=dev)
    # the transposed weight image: the one the forward's pack launch of this step wrote (NeRF.packed_weights, f16x3 training), else
    # rebuilt by this call
    pre = nerf.packed_t_current() if (wgrad_precision == "f16x3" and hasattr(nerf, "packed_t_current")) else None
    if pre is not None:
        a.packed_t, a.repack = pre.data_ptr(), 0
    else:
        if "packed_t" not in sc:
            sc["packed_t"] = torch.empty(int(_lib.load().tp_mlp_packed_t_bytes()) // 4, device=dev)
        a.packed_t, a.repack = sc["packed_t"].data_ptr(), 1
    # the scale word inside the workspace is cleared by the last kernel of every call: no memset when the previous call used this
    # workspace with this size
    # The mark says "the last EXECUTED call on this workspace ran to its end".  An eager call drops it before launching and sets it
    # only after tp_mlp_bwd has returned without error (a failure after the dgrad kernel leaves the word dirty: the next call
    # memsets).  A call that is being captured into a hipGraph executes nothing now: it may rely on the mark (at replay time the
    # word is clean -- the eager call or the replay before it cleared it) but must not touch it, so that a capture which is
    # discarded without a replay changes nothing for the next eager call.
    capturing = bool(torch.cuda.is_current_stream_capturing())
    clear_key = (sc["ws"].data_ptr(), S, wgrad_precision)
    a.dz_max_is_clear = 1 if sc.get("clear_for") == clear_key else 0
    if not capturing:
        sc.pop("clear_for", None)
    a.saved, a.rgb, a.density, a.uncert = saved.data_ptr(), rgb.data_ptr(), density.data_ptr(), uncert.data_ptr()
    a.g_rgb, a.g_density, a.g_uncert = g_rgb.data_ptr(), g_density.data_ptr(), g_uncert.data_ptr()
    a.lat_trans, a.lat_light = lat_trans.data_ptr(), lat_light.data_ptr()
    a.B, a.R, a.N = B, R, N
    a.g_lat_trans, a.g_lat_light, a.workspace = g_lt.data_ptr(), g_ll.data_ptr(), sc["ws"].data_ptr()
    a.wgrad_precision = PRECISIONS[wgrad_precision]
    # (a caller that runs other streams beside the backward -- the captured GAN iteration -- leaves them a share of the device for the
    # length of the weight gradient: NeRF.wgrad_cus, 0 = all)
    a.wgrad_cus = int(getattr(nerf, "wgrad_cus", 0) or 0)
    _call("tp_mlp_bwd", a)
    if not capturing:
        sc["clear_for"] = clear_key
    return dict(params=grads, lat_trans=g_lt, lat_light=g_ll)


@_on_tensor_device
def posenc(x: Tensor, L: int) -> Tensor:
    x = _f32(x, "x")
    Cn = x.shape[-1]
    out = torch.empty(*x.shape[:-1], 2 * Cn * L, device=x.device)
    _call("tp_posenc", x.data_ptr(), x.numel() // Cn, Cn, L, out.data_ptr())
    return out


# ------------------------------------------------------------------------------------------ K4
def _composite_args(ray, rgb, density, depth, uncert, min_uncert) -> Tuple[CompositeArgs, tuple]:
    ray, rgb, density = _f32(ray, "ray"), _f32(rgb, "rgb_samples"), _f32(density, "density_samples")
    depth, uncert = _f32(depth, "depth_samples"), _f32(uncert, "uncert_samples")
    n = ray.numel() // 3
    N = depth.numel() // n
    a = CompositeArgs()
    a.ray, a.rgb, a.density, a.depth, a.uncert = (ray.data_ptr(), rgb.data_ptr(), density.data_ptr(),
                                                  depth.data_ptr(), uncert.data_ptr())
    a.n, a.N, a.min_uncert = n, N, float(min_uncert)
    return a, (ray, rgb, density, depth, uncert)


@_on_tensor_device
def composite_fwd(ray, rgb, density, depth, uncert, min_uncert: float = 0.05, per_sample: bool = True,
                  want_prob: bool = True, compact: bool = False):
    """-> out_ray [..,14], alpha_static, alpha_transient, prob ([..,N] or None); with ``compact`` also (rgb_ray [..,3],
    uncert_ray [..,1]): contiguous copies of out_ray[..., 0:3] / [..., 13:14] written by the same launch (the losses, the
    feature network and the PatchGAN consume these two; slices of out_ray would need a copy each and a slice-backward)."""
    a, keep = _composite_args(ray, rgb, density, depth, uncert, min_uncert)
    lead = keep[0].shape[:-1]
    dev = keep[0].device
    out = torch.empty(*lead, 14, device=dev)
    rgb_ray = unc_ray = None
    if compact:
        rgb_ray, unc_ray = torch.empty(*lead, 3, device=dev), torch.empty(*lead, 1, device=dev)
        a.rgb_ray, a.uncert_ray = rgb_ray.data_ptr(), unc_ray.data_ptr()
    a_s = torch.empty(*lead, a.N, device=dev) if per_sample else None
    a_t = torch.empty(*lead, a.N, device=dev) if per_sample else None
    prob = torch.empty(*lead, a.N, device=dev) if want_prob else None
    a.out_ray, a.alpha_static, a.alpha_transient, a.prob = out.data_ptr(), _ptr(a_s), _ptr(a_t), _ptr(prob)
    _call("tp_composite_fwd", a)
    return (out, a_s, a_t, prob, rgb_ray, unc_ray) if compact else (out, a_s, a_t, prob)


@_on_tensor_device
def composite_bwd(ray, rgb, density, depth, uncert, g_out: Optional[Tensor], g_alpha_s: Optional[Tensor] = None,
                  g_alpha_t: Optional[Tensor] = None, g_prob: Optional[Tensor] = None, min_uncert: float = 0.05,
                  g_rgb_ray: Optional[Tensor] = None, g_uncert_ray: Optional[Tensor] = None, g_rgb_ray2: Optional[Tensor] = None,
                  g_rgb_ray3: Optional[Tensor] = None, g_density_add: Optional[Tensor] = None):
    """``g_out`` [..,14] may be None when the cotangent arrives through ``g_rgb_ray`` [..,3] / ``g_uncert_ray`` [..,1] (they
    are ADDED to columns 0..2 / 13 of g_out inside the kernel; ``g_rgb_ray2`` / ``g_rgb_ray3`` likewise).  ``g_density_add``
    [..,N,2] is added to the returned density gradient."""
    b = CompositeBwdArgs()
    fa, keep = _composite_args(ray, rgb, density, depth, uncert, min_uncert)
    b.fwd = fa
    # (every cotangent is optional: the kernel reads a missing one as zero -- no zero g_out is made up here)
    g_out = None if g_out is None else _f32(g_out, "g_out")
    g_rgb_ray = None if g_rgb_ray is None else _f32(g_rgb_ray, "g_rgb_ray")
    g_uncert_ray = None if g_uncert_ray is None else _f32(g_uncert_ray, "g_uncert_ray")
    opt = [None if g is None else _f32(g, "g") for g in (g_alpha_s, g_alpha_t, g_prob)]
    g_rgb, g_den, g_unc = torch.empty_like(keep[1]), torch.empty_like(keep[2]), torch.empty_like(keep[4])
    b.g_out_ray, b.g_rgb_ray, b.g_uncert_ray = _ptr(g_out), _ptr(g_rgb_ray), _ptr(g_uncert_ray)
    extra = [None if g is None else _f32(g, "g") for g in (g_rgb_ray2, g_rgb_ray3, g_density_add)]
    if extra[2] is not None and extra[2].numel() != keep[2].numel():
        raise ValueError("composite_bwd: g_density_add must have the shape of density")
    b.g_rgb_ray2, b.g_rgb_ray3, b.g_density_add = _ptr(extra[0]), _ptr(extra[1]), _ptr(extra[2])
    b.g_alpha_static, b.g_alpha_transient, b.g_prob = _ptr(opt[0]), _ptr(opt[1]), _ptr(opt[2])
    b.g_rgb, b.g_density, b.g_uncert = g_rgb.data_ptr(), g_den.data_ptr(), g_unc.data_ptr()
    _call("tp_composite_bwd", b)
    return g_rgb, g_den, g_unc


# ------------------------------------------------------------------------------------------ K5
@_on_tensor_device
def patch_gather(coords: Tensor, image: Tensor, image_syn: Tensor, nocs: Tensor, normal: Tensor, obj_mask: Tensor,
                 mask_syn: Tensor, disc_rgb: Optional[Tensor] = None, disc_geo: bool = False):
    """-> [B,14,p,p]: image3, image_syn3, nocs3*mask_syn, normal3*mask_syn, mask, mask_syn.
    ``disc_rgb`` [B,P,3] (the rendered colours): -> (that, real stack [2B,nc,p,p], fake [B,nc,p,p]) -- the PatchGAN's input stacks of
    the same pixels from the same launch (`disc_inputs(disc_rgb, gathered, ..., stacked=True)`, bit for bit)."""
    coords = _f32(coords, "coords")
    B, ph, pw, _ = coords.shape
    ts = [_f32(t, "image") for t in (image, image_syn, nocs, normal, obj_mask, mask_syn)]
    H, W = ts[0].shape[-2:]
    out = torch.empty(B, 14, ph, pw, device=coords.device)
    a = PatchGatherArgs()
    a.coords = coords.data_ptr()
    a.image, a.image_syn, a.nocs, a.normal, a.obj_mask, a.mask_syn = [t.data_ptr() for t in ts]
    a.B, a.P, a.H, a.W, a.out = B, ph * pw, H, W, out.data_ptr()
    if disc_rgb is None:
        _call("tp_patch_gather", a)
        return out
    rgb = _f32(disc_rgb.detach(), "disc_rgb")
    if rgb.numel() != B * ph * pw * 3:
        raise ValueError("patch_gather: disc_rgb [B,P,3] expected")
    nc = 9 if disc_geo else 3
    real, fake = torch.empty(2 * B, nc, ph, pw, device=coords.device), torch.empty(B, nc, ph, pw, device=coords.device)
    a.disc_rgb, a.disc_real, a.disc_fake, a.disc_geo = rgb.data_ptr(), real.data_ptr(), fake.data_ptr(), int(bool(disc_geo))
    _call("tp_patch_gather", a)
    return out, real, fake


@_on_tensor_device
def eval_metrics(rgb_static: Tensor, image: Tensor, obj_mask: Tensor, H: int, W: int, out_hw=None):
    """PSNR / SSIM of the static render against the masked image (reference evaluate_full, :340-362).
    rgb_static [B,H*W,3], image [B,3,H,W], obj_mask [B,H,W]; ``out_hw`` = (480, 640) reproduces the resize the
    reference applies to non-crop data.  Returns (psnr, ssim, mse) as 0-dim fp64 device tensors (no host sync)."""
    rgb_static, image, obj_mask = _f32(rgb_static, "rgb_static"), _f32(image, "image"), _f32(obj_mask, "obj_mask")
    B = image.shape[0]
    if rgb_static.numel() != B * H * W * 3 or image.shape[1:] != (3, H, W) or obj_mask.numel() != B * H * W:
        raise ValueError("eval_metrics: rgb_static [B,H*W,3], image [B,3,H,W], obj_mask [B,H,W] expected")
    oh, ow = (H, W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    ws = torch.empty(max(1, _lib.load().tp_eval_metrics_workspace_bytes(B, oh, ow) // 4), device=image.device)
    out = torch.empty(B, 2, dtype=torch.float64, device=image.device)
    a = _lib.EvalMetricsArgs()
    a.rgb_static, a.image, a.obj_mask = rgb_static.data_ptr(), image.data_ptr(), obj_mask.data_ptr()
    a.B, a.h, a.w, a.out_h, a.out_w = B, H, W, oh, ow
    a.workspace, a.out = ws.data_ptr(), out.data_ptr()
    _call("tp_eval_metrics", a)
    n = float(B * 3 * oh * ow)
    mse = out[:, 0].sum() / n
    return -10.0 * torch.log10(mse), out[:, 1].sum() / n, mse


@_on_tensor_device
def render_eval(packed: Tensor, intr: Tensor, pose: Tensor, ray_idx: Tensor, z_near: Tensor, z_far: Tensor, lat_trans: Tensor,
                lat_light: Tensor, *, H: int, W: int, n_samples: int, precision: str = "f16x3", min_uncert: float = 0.05,
                rand: Optional[Tensor] = None, with_alphas: bool = False, ray_bias: bool = False, ndc: bool = False,
                depth_param: str = "metric"):
    """The C ABI's one-call evaluation render (tp_render_eval: ray-gen + MLP + composite, intermediates in one workspace).
    ``ray_bias``: ``packed`` is the ray-bias stream (pack_weights(..., ray_bias=True); f16x3 or f16, n_samples % 128 == 0).
    Returns out_ray [B,R,14] (COMPOSITE_RAY_FIELDS) and, if asked, (alpha_static, alpha_transient) [B,R,N].  The Python
    mirror (Graph.render) launches the same three kernels itself; this entry point exists for non-Python hosts."""
    intr, pose = _f32(intr, "intr"), _f32(pose, "pose")
    z_near, z_far = _f32(z_near, "z_near"), _f32(z_far, "z_far")
    lat_trans, lat_light = _f32(lat_trans, "lat_trans"), _f32(lat_light, "lat_light")
    ray_idx = ray_idx.to(torch.int64).contiguous()
    B, R = ray_idx.shape
    dev = pose.device
    a = _lib.RenderEvalArgs()
    rg = a.raygen
    rg.intr, rg.pose, rg.ray_idx, rg.z_near, rg.z_far = intr.data_ptr(), pose.data_ptr(), ray_idx.data_ptr(), z_near.data_ptr(), z_far.data_ptr()
    rg.B, rg.R, rg.H, rg.W, rg.N = B, R, H, W, n_samples
    rg.pixel_mode, rg.bounds_mode = PIX_INDEX, BOUNDS_MAP
    rg.ndc, rg.depth_param = int(bool(ndc)), DEPTH_PARAMS[depth_param]
    if rand is not None:
        rand = _f32(rand, "rand")
        rg.rand, rg.jitter_mode = rand.data_ptr(), JITTER_GIVEN
    else:
        rg.jitter_mode = JITTER_MID
    a.packed, a.lat_trans, a.lat_light = packed.data_ptr(), lat_trans.data_ptr(), lat_light.data_ptr()
    a.precision, a.min_uncert = PRECISIONS[precision], float(min_uncert)
    a.packed_ray_bias = 1 if ray_bias else 0
    a.status = mlp_status(dev).data_ptr() if precision in F16_RANGE_PRECISIONS else None
    ws = torch.empty(int(_lib.load().tp_render_eval_workspace_bytes(B, R, n_samples)) // 4 + 64, device=dev)
    out = torch.empty(B, R, 14, device=dev)
    a.workspace, a.out_ray = ws.data_ptr(), out.data_ptr()
    alphas = None
    if with_alphas:
        alphas = (torch.empty(B, R, n_samples, device=dev), torch.empty(B, R, n_samples, device=dev))
        a.alpha_static, a.alpha_transient = alphas[0].data_ptr(), alphas[1].data_ptr()
    _call("tp_render_eval", a)
    return (out, alphas) if with_alphas else out


# ------------------------------------------------------------------------------------------ K13
_lattices = {}


@_on_tensor_device
def patch_coords(u: Optional[Tensor], patch_size: int, lo, hi: float, random_scale: bool = True, random_shift: bool = True, *,
                 nbatch: Optional[int] = None, seed: int = 0, counter: Optional[Tensor] = None, device=None, defer: bool = False):
    """FlexPatchSampler in one launch: u [3,B,...] uniforms -> (coords [B,p,p,2], scales [B,1,1,1]); ``lo`` is a float or a
    0-dim device tensor (the annealed bound of a captured step).  ``u`` None: ``nbatch`` images, the uniforms drawn inside the
    kernel from (``seed``, the device word ``counter``: int64 [1], the step counter of a captured training step).
    ``defer``: nothing is launched; the returned tensors are filled by the ray-generation launch that is given the job stored as
    ``coords._tp_sampler_job`` (`raygen(..., coords=coords, sampler=job)`)."""
    if u is not None:
        u = _f32(u, "u")
        B, dev = u.numel() // 3, u.device
    else:
        B, dev = int(nbatch), (counter.device if counter is not None else torch.device(device))
        if counter is not None and (counter.dtype != torch.int64 or counter.numel() != 1):
            raise ValueError("patch_coords: counter must be one int64 device word")
    p = int(patch_size)
    key = (p, dev.index)
    if key not in _lattices:
        _lattices[key] = torch.linspace(-1, 1, p, device=dev)
    coords = torch.empty(B, p, p, 2, device=dev)
    scales = torch.empty(B, 1, 1, 1, device=dev)
    if defer:
        coords._tp_sampler_job = dict(u=u, B=B, p=p, lattice=_lattices[key], lo=lo, hi=hi, random_scale=random_scale, random_shift=random_shift,
                                      seed=seed, counter=counter, coords=coords, scales=scales)
        return coords, scales
    lo_dev = lo.data_ptr() if torch.is_tensor(lo) else None
    lo_host = 0.0 if torch.is_tensor(lo) else float(lo)
    _call("tp_patch_coords", _ptr(u), B, p, _lattices[key].data_ptr(), lo_dev, lo_host, float(hi) - lo_host, float(hi), int(bool(random_scale)),
          int(bool(random_shift)), int(seed) & (2 ** 64 - 1), _ptr(counter), coords.data_ptr(), scales.data_ptr())
    return coords, scales


@_on_tensor_device
def latent_rows_fwd(w_trans: Tensor, w_light: Tensor, idx: Tensor, idx_copy: Optional[Tensor] = None, defer: bool = False):
    """``idx_copy`` (int64 [B], optional): the launch also writes idx there (a private copy for the backward).  ``defer``: nothing is
    launched; returns (out_trans, out_light, job) -- the ray-generation launch given the job fills them (`raygen(..., rows=job)`)."""
    w_trans, w_light = _f32(w_trans, "w_trans"), _f32(w_light, "w_light")
    idx = idx.to(torch.int64).contiguous()
    B = idx.numel()
    ot, ol = torch.empty(B, w_trans.shape[1], device=idx.device), torch.empty(B, w_light.shape[1], device=idx.device)
    if idx_copy is not None and not (idx_copy.dtype == torch.int64 and idx_copy.is_contiguous() and idx_copy.numel() == B and idx_copy.device == idx.device):
        raise _lib.TexposeLibraryError("latent_rows_fwd: idx_copy must be a contiguous int64 device tensor of idx's length")
    if defer:
        return ot, ol, dict(w_trans=w_trans, w_light=w_light, idx=idx, out_trans=ot, out_light=ol, idx_copy=idx_copy)
    _call("tp_latent_rows_fwd", w_trans.data_ptr(), w_light.data_ptr(), idx.data_ptr(), B, w_trans.shape[1], w_light.shape[1], ot.data_ptr(),
          ol.data_ptr(), _ptr(idx_copy))
    return ot, ol


@_on_tensor_device
def latent_rows_bwd(g_trans: Tensor, g_light: Tensor, idx: Tensor, n_rows: int):
    g_trans, g_light = _f32(g_trans, "g_trans"), _f32(g_light, "g_light")
    if idx.dtype != torch.int64 or not idx.is_contiguous() or not idx.is_cuda:
        raise _lib.TexposeLibraryError("latent_rows_bwd: idx must be the contiguous int64 device tensor the forward used (got %s%s)"
                                       % (idx.dtype, "" if idx.is_contiguous() else ", non-contiguous"))
    B = idx.numel()
    gwt, gwl = torch.empty(n_rows, g_trans.shape[1], device=idx.device), torch.empty(n_rows, g_light.shape[1], device=idx.device)
    _call("tp_latent_rows_bwd", g_trans.data_ptr(), g_light.data_ptr(), idx.data_ptr(), B, int(n_rows), g_trans.shape[1], g_light.shape[1],
          gwt.data_ptr(), gwl.data_ptr())
    return gwt, gwl
