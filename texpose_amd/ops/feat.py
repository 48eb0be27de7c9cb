"""K12, K13, K18: the feature (perceptual) loss -- the 3x3 convolutions, pooling, its input stacks and the fused chain."""
import ctypes as C
from typing import Dict, Optional

import torch

from .. import _lib, knobs
from ._base import Tensor, _call, _f32, _on_tensor_device, _ptr
from .gan import _conv_scratch

__all__ = ["conv3s1_supported", "conv3s1_fwd", "conv3s1_dgrad", "_feat_args", "feat_inputs_fwd", "feat_inputs_bwd", "_feat_chain_scratch",
           "feat_chain_supported", "feat_chain_pack", "feat_chain", "feat_pair_loss_fwd", "feat_pair_loss_bwd", "maxpool2_fwd", "maxpool2_bwd"]


# ------------------------------------------------------------------------------------------ K12
def conv3s1_supported(x: Tensor) -> bool:
    H, W = x.shape[-2:]
    return x.is_cuda and x.dtype == torch.float32 and H >= 4 and W >= 4 and (H & (H - 1)) == 0 and (W & (W - 1)) == 0


@_on_tensor_device
def conv3s1_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor], relu: bool) -> Tensor:
    """relu?(conv2d(x [N,C,H,W], w [Co,C,3,3], bias, stride 1, padding 1))."""
    x, w = _f32(x, "x"), _f32(w, "w")
    bias = _f32(bias, "bias") if bias is not None else None
    N, C_in, H, W = x.shape
    y = torch.empty(N, w.shape[0], H, W, device=x.device)
    a = _lib.Conv3s1Args()
    a.N, a.C, a.H, a.W, a.Co, a.relu = N, C_in, H, W, w.shape[0], int(bool(relu))
    ws, cnt = _conv_scratch(_lib.load().tp_conv3s1_workspace, a, _lib.CONV_FWD, x.device)
    a.inp, a.w, a.bias, a.out, a.counters, a.workspace = x.data_ptr(), w.data_ptr(), _ptr(bias), y.data_ptr(), cnt.data_ptr(), _ptr(ws)
    _call("tp_conv3s1_fwd", a)
    return y


@_on_tensor_device
def conv3s1_dgrad(gy: Tensor, w: Tensor, mask: Optional[Tensor]) -> Tensor:
    """gradient of conv3s1_fwd wrt x; ``mask`` = the forward output of a ReLU layer (gy counts where it is > 0)."""
    gy, w = _f32(gy, "gy"), _f32(w, "w")
    mask = _f32(mask, "mask") if mask is not None else None
    N, Co, H, W = gy.shape
    gx = torch.empty(N, w.shape[1], H, W, device=gy.device)
    a = _lib.Conv3s1Args()
    a.N, a.C, a.H, a.W, a.Co, a.relu = N, w.shape[1], H, W, Co, 0
    ws, cnt = _conv_scratch(_lib.load().tp_conv3s1_workspace, a, _lib.CONV_DGRAD, gy.device)
    a.inp, a.w, a.mask, a.out, a.counters, a.workspace = gy.data_ptr(), w.data_ptr(), _ptr(mask), gx.data_ptr(), cnt.data_ptr(), _ptr(ws)
    _call("tp_conv3s1_dgrad", a)
    return gx


def _feat_args(rgb, gathered, mean, std):
    a = _lib.FeatInputsArgs()
    B, P = rgb.shape[0], rgb.shape[1]
    if rgb.shape != (B, P, 3) or gathered.shape[0] != B or gathered.numel() != B * 14 * P:
        raise ValueError("feat_inputs: rgb [B,P,3] and gathered [B,14,p,p] expected")
    a.rgb, a.gathered, a.B, a.P, a.n_channels = rgb.data_ptr(), gathered.data_ptr(), B, P, 14
    a.c_image, a.c_image_syn, a.c_mask, a.c_mask_syn = 0, 3, 12, 13
    for c in range(3):
        a.mean[c], a.std[c] = float(mean[c]), float(std[c])
    return a


@_on_tensor_device
def feat_inputs_fwd(rgb: Tensor, gathered: Tensor, mean, std, hw) -> Tensor:
    """-> [4B,3,h,w]: the (fake, real) pairs of the feature loss, masked and ImageNet-normalised (K13)."""
    rgb, gathered = _f32(rgb, "rgb"), _f32(gathered, "gathered")
    out = torch.empty(4 * rgb.shape[0], 3, hw[0], hw[1], device=rgb.device)
    _call("tp_feat_inputs_fwd", _feat_args(rgb, gathered, mean, std), out.data_ptr())
    return out


@_on_tensor_device
def feat_inputs_bwd(rgb: Tensor, gathered: Tensor, mean, std, g_out: Tensor) -> Tensor:
    g_out = _f32(g_out, "g_out")
    g_rgb = torch.empty_like(rgb)
    _call("tp_feat_inputs_bwd", _feat_args(rgb, gathered, mean, std), g_out.data_ptr(), g_rgb.data_ptr())
    return g_rgb


_feat_chain_scratch: Dict[tuple, tuple] = {}


def feat_chain_supported(rgb: Tensor, gathered: Tensor, hw) -> bool:
    """K18 covers 16 x 16 patches of float32 CUDA tensors (tp_feat_chain)."""
    return (rgb.is_cuda and rgb.dtype == torch.float32 and gathered.dtype == torch.float32 and tuple(hw) == (16, 16)
            and rgb.dim() == 3 and rgb.shape[1] == 256 and not knobs.K.no_feat_chain)


def feat_chain_pack(weights, out: Optional[Tensor] = None) -> Tensor:
    """The seven frozen [Co,C,3,3] weights of VGG19 features[:15] in K18's operand order (tp_feat_chain_pack): one launch.  ``out``:
    an earlier result to overwrite (a captured step keeps its address).  The OWNER of the weights caches the result
    (gan_modules.PerceptualLoss): a cache keyed by addresses here would serve a new network the old one's weights."""
    shapes = [(64, 3), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256)]
    if len(weights) != 7:
        raise ValueError("feat_chain_pack: the seven convolutions of VGG19 features[:15] expected")
    for w, (co, ci) in zip(weights, shapes):
        if tuple(w.shape) != (co, ci, 3, 3) or not w.is_contiguous() or w.dtype != torch.float32 or not w.is_cuda:
            raise ValueError("feat_chain_pack: weight %s does not fit VGG19 features[:15]" % (tuple(w.shape),))
    dev = weights[0].device
    n = int(_lib.load().tp_feat_chain_packed_floats())
    if out is None:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.TexposeLibraryError("tp_feat_chain_pack: pack before the hipGraph capture (run one eager step first)")
        out = torch.empty(n, device=dev)
    ptrs = (C.c_void_p * _lib.FEAT_CHAIN_LAYERS)(*[w.data_ptr() for w in weights])
    with torch.cuda.device(dev):
        _call("tp_feat_chain_pack", ptrs, out.data_ptr())
    return out


@_on_tensor_device
def feat_chain(rgb: Tensor, gathered: Tensor, packed: Tensor, biases, mean, std, hw, w2: float = 5.0, scale: float = 1.0):
    """K18 (tp_feat_chain): the feature loss of the generator step and its gradient wrt the rendered colours in ONE call --
    (loss3 [3] = {l1 + w2 l2, l1, l2}, g_rgb [B,P,3] = scale * d loss3[0] / d rgb).  ``packed``: `feat_chain_pack` of the seven
    convolution weights of VGG19 features[:15]; ``biases``: theirs.  Workspace and tile counters are per (device, stream, batch size)
    and persistent: calls on different streams may overlap, and a captured call keeps its buffers."""
    rgb, gathered = _f32(rgb.detach(), "rgb"), _f32(gathered, "gathered")
    B, dev = rgb.shape[0], rgb.device
    if len(biases) != _lib.FEAT_CHAIN_LAYERS or packed.numel() != int(_lib.load().tp_feat_chain_packed_floats()) or packed.dtype != torch.float32:
        raise ValueError("feat_chain: packed weights (feat_chain_pack) and the seven biases of VGG19 features[:15] expected")
    for b, co in zip(biases, (64, 64, 128, 128, 256, 256, 256)):
        if tuple(b.shape) != (co,) or b.dtype != torch.float32:
            raise ValueError("feat_chain: bias %s does not fit VGG19 features[:15]" % (tuple(b.shape),))
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, B)
    scratch = _feat_chain_scratch.get(key)
    if scratch is None:
        n_cnt = C.c_int64(0)
        n_ws = _lib.load().tp_feat_chain_workspace(B, int(hw[0]), int(hw[1]), C.byref(n_cnt))
        if n_ws < 0:
            _lib.check(-1, "tp_feat_chain_workspace")
        if torch.cuda.is_current_stream_capturing():
            raise _lib.TexposeLibraryError("tp_feat_chain: its workspace must exist before a hipGraph capture (run one eager step first)")
        scratch = _feat_chain_scratch[key] = (torch.empty(int(n_ws), device=dev), torch.zeros(int(n_cnt.value), dtype=torch.int32, device=dev))
    ws, cnt = scratch
    a = _lib.FeatChainArgs()
    f = _feat_args(rgb, gathered, mean, std)
    a.rgb, a.gathered, a.B, a.H, a.W, a.n_channels = f.rgb, f.gathered, B, int(hw[0]), int(hw[1]), f.n_channels
    a.c_image, a.c_image_syn, a.c_mask, a.c_mask_syn = f.c_image, f.c_image_syn, f.c_mask, f.c_mask_syn
    for c in range(3):
        a.mean[c], a.std[c] = f.mean[c], f.std[c]
    a.packed = packed.data_ptr()
    for l in range(_lib.FEAT_CHAIN_LAYERS):
        a.bias[l] = biases[l].data_ptr()
    a.w2, a.scale = float(w2), float(scale)
    loss3, g_rgb = torch.empty(3, device=dev), torch.empty_like(rgb)
    a.loss, a.g_rgb = loss3.data_ptr(), g_rgb.data_ptr()
    a.workspace, a.workspace_floats, a.counters, a.n_counters = ws.data_ptr(), ws.numel(), cnt.data_ptr(), cnt.numel()
    _call("tp_feat_chain", a)
    return loss3, g_rgb


@_on_tensor_device
def feat_pair_loss_fwd(feat: Tensor, w2: float) -> Tensor:
    """feat [4B,...] = features of [fake1 | fake2 | real1 | real2] -> [l1 + w2 l2, l1, l2] (one launch)."""
    feat = _f32(feat, "feat")
    out = torch.empty(3, device=feat.device)
    _call("tp_feat_pair_loss_fwd", feat.data_ptr(), feat.numel() // 4, float(w2), out.data_ptr())
    return out


@_on_tensor_device
def feat_pair_loss_bwd(feat: Tensor, w2: float, g: Tensor) -> Tensor:
    g = _f32(g, "g")
    g_feat = torch.empty_like(feat)
    _call("tp_feat_pair_loss_bwd", feat.data_ptr(), feat.numel() // 4, float(w2), g.data_ptr(), g_feat.data_ptr())
    return g_feat


@_on_tensor_device
def maxpool2_fwd(x: Tensor):
    """MaxPool2d(2, 2) of x [N,C,H,W] (H, W even) -> (y [N,C,H/2,W/2], arg uint8: window position of the maximum)."""
    x = _f32(x, "x")
    N, Cc, H, W = x.shape
    y = torch.empty(N, Cc, H // 2, W // 2, device=x.device)
    arg = torch.empty(N, Cc, H // 2, W // 2, device=x.device, dtype=torch.uint8)
    _call("tp_maxpool2_fwd", x.data_ptr(), N * Cc, H, W, y.data_ptr(), arg.data_ptr())
    return y, arg


@_on_tensor_device
def maxpool2_bwd(gy: Tensor, arg: Tensor) -> Tensor:
    gy = _f32(gy, "gy")
    N, Cc, oh, ow = gy.shape
    gx = torch.empty(N, Cc, 2 * oh, 2 * ow, device=gy.device)
    _call("tp_maxpool2_bwd", gy.data_ptr(), arg.data_ptr(), N * Cc, 2 * oh, 2 * ow, gx.data_ptr())
    return gx
