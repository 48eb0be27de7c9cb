"""References of the two fp16 MLP arithmetics shared by the GPU tests (tests/test_gpu_f16_synthesis.py, tests/test_gpu_fp16_range.py)
and the CPU test of the rescaling (tests/test_f16_precision_cpu.py): the fp16-operand emulation of the oracle, its fp64 encoding,
seeded rays, and the function-preserving per-layer rescaling of a network (ReLU is positively homogeneous)."""
import numpy as np
import torch

from oracle import texpose_oracle as O

WIDE_OUT = 256
FP16_RANGE = 6.0e4              # the range guard of both fp16 arithmetics fires at this activation

# the 14 hidden (ReLU) outputs of the network, in execution order; mlp_feat.7 means its rows 1..256 (row 0 is the density)
HIDDEN = tuple(["mlp_feat.%d" % i for i in range(8)] + ["mlp_trans.%d" % i for i in range(3)] + ["mlp_rgb.%d" % i for i in range(3)])
# what consumes each hidden output: (matrix, its columns); mlp_feat.4 also reads the skip encoding (columns 256..318, not scaled)
CONSUMERS = {**{"mlp_feat.%d" % i: (("mlp_feat.%d" % (i + 1), slice(0, 256)),) for i in range(7)},
             "mlp_feat.7": (("mlp_rgb.0", slice(0, 256)), ("mlp_trans.0", slice(0, 256))),
             **{"mlp_trans.%d" % i: (("mlp_trans.%d" % (i + 1), slice(0, 256)),) for i in range(3)},
             **{"mlp_rgb.%d" % i: (("mlp_rgb.%d" % (i + 1), slice(0, 256)),) for i in range(3)}}
# the latent codes as scalable inputs: the columns that read them
LATENT_COLS = {"lat_trans": ("mlp_trans.0", slice(256, 272)), "lat_light": ("mlp_rgb.0", slice(286, 334))}


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def posenc64(x, L):
    freq = (2 ** torch.arange(L, dtype=torch.float32)) * np.pi
    spec = (x.float()[..., None] * freq).double()          # the fp32-rounded argument the kernel encodes
    return torch.stack([spec.sin(), spec.cos()], dim=-2).reshape(*x.shape[:-1], -1)


def emulate_f16(params, points, ray_unit, lat_trans, lat_light, ray_bias=False, rounded=True, acts=None):
    """The oracle in fp64 with the operands of every 256-wide layer rounded to fp16 (nearest even): weights and inputs of
    mlp_feat.0-7 (without the density row of mlp_feat.7), mlp_rgb.0-2, mlp_trans.0-2.  The narrow output layers stay exact.
    ``ray_bias``: the ray-constant columns (mlp_rgb.0 view encoding 256..282 and light code 286..333, mlp_trans.0 transient code
    256..271) are contracted unrounded, as the per-ray bias pre-kernels do.  ``rounded=False``: no rounding at all (fp64 oracle).
    ``acts``: filled with the largest post-ReLU value of each hidden output (HIDDEN) as this arithmetic computes it."""
    p64 = {k: v.double() for k, v in params.items()}
    names = {id(v): k for k, v in p64.items()}
    exact_cols = {"mlp_rgb.0.weight": list(range(256, 283)) + list(range(286, 334)), "mlp_trans.0.weight": list(range(256, 272))}
    lin = torch.nn.functional.linear

    def linear(x, w, b=None):
        name = names.get(id(w), "")
        if w.shape[0] < WIDE_OUT or not rounded:
            out = lin(x, w, b)                                    # narrow output layer: exact
        else:
            keep = torch.zeros(w.shape[1], dtype=torch.bool)
            if ray_bias and name in exact_cols:
                keep[exact_cols[name]] = True
            xr = torch.where(keep, x, x.half().double())
            wr = torch.where(keep, w, w.half().double())
            out = lin(xr, wr, b)
            if w.shape[0] == WIDE_OUT + 1:                        # mlp_feat.7: row 0 is the density head
                out[..., 0] = lin(x, w[:1], None if b is None else b[:1])[..., 0]
        if acts is not None and w.shape[0] >= WIDE_OUT:
            h = out[..., 1:] if w.shape[0] == WIDE_OUT + 1 else out
            acts[name[:-len(".weight")]] = float(h.max().clamp_min(0))
        return out

    saved = O.posenc, torch.nn.functional.linear
    O.posenc, torch.nn.functional.linear = posenc64, linear
    try:
        with torch.no_grad():
            return O.mlp_forward(p64, points.double(), ray_unit.double(), lat_trans.double(), lat_light.double())
    finally:
        O.posenc, torch.nn.functional.linear = saved


def hidden_maxima(params, points, ray_unit, lat_trans, lat_light):
    """largest activation of every hidden output of the fp64 oracle"""
    acts = {}
    emulate_f16(params, points, ray_unit, lat_trans, lat_light, rounded=False, acts=acts)
    return acts


def rescale(params, ks):
    """The same network function with hidden output l multiplied by 2^ks[l]: the rows (and biases) of l's producer times 2^k, the
    columns of every consumer that read l times 2^-k (powers of two: exact in fp32 unless a value leaves the range).  Keys
    "lat_trans" / "lat_light": the columns that read that latent code times 2^-k (the caller multiplies the code by 2^k)."""
    out = {k: v.clone() for k, v in params.items()}
    for name, k in ks.items():
        s = 2.0 ** k
        if name in LATENT_COLS:
            m, cols = LATENT_COLS[name]
            out[m + ".weight"][:, cols] /= s
            continue
        rows = slice(1, None) if name == "mlp_feat.7" else slice(None)
        out[name + ".weight"][rows] *= s
        out[name + ".bias"][rows] *= s
        for m, cols in CONSUMERS[name]:
            out[m + ".weight"][:, cols] /= s
    return out


def rays(seed, B, R, N):
    """form-A inputs (center, ray, depth) and the points / unit directions the kernel derives from them in fp32"""
    rs = np.random.RandomState(seed)
    center = torch.from_numpy(rs.uniform(-0.3, 0.3, size=(B, R, 3)).astype(np.float32))
    ray = torch.from_numpy(rs.normal(size=(B, R, 3)).astype(np.float32))
    depth = torch.from_numpy(np.sort(rs.uniform(0.2, 1.4, size=(B, R, N)), axis=-1).astype(np.float32))
    pts = center[:, :, None] + ray[:, :, None] * depth[..., None]
    unit = (ray / ray.norm(dim=-1, keepdim=True).clamp_min(1e-12))[:, :, None].expand(B, R, N, 3).contiguous()
    lt = torch.from_numpy(rs.normal(size=(B, 16)).astype(np.float32))
    ll = torch.from_numpy(rs.normal(size=(B, 48)).astype(np.float32))
    return center, ray, depth, pts, unit, lt, ll
