#!/usr/bin/env python3
"""Build-container check of the drop-in claim in INTEGRATION.md (needs the reference code base, so it cannot run on the GPU box;
tests/test_shim_cpu.py runs it as a child process wherever the reference is present): construct the shim
`model/nerf_adapt_st_gan_amd.py` defines -- texpose_amd.graph.RenderMixin mixed into the reference's Graph -- compare its state
dict, method table and option handling with the reference Graph, then drive both with the reference's own engine (two training
iterations) and its own nerf_forward (validation / evaluation renders, camera.ndc, inverse depths) on the CPU oracle.

    python tests/golden/check_shim_here.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_golden as MG                                            # noqa: E402  (puts the repository root on sys.path)
from cpu_backend import oracle_backend                              # noqa: E402


def main():
    opt, camera, M, NeRF, RaySampler, FlexPatchSampler = MG._load_reference()
    opt.patch_size = 16
    from texpose_amd.graph import Graph as AmdGraph, RenderMixin
    from texpose_amd.nerf import NeRF as AmdNeRF
    from texpose_amd.gan_modules import Discriminator as AmdDisc

    class Graph(RenderMixin, M.Graph):                              # INTEGRATION.md section 1, as documented
        def __init__(self, opt):
            super().__init__(opt)
            self.nerf = AmdNeRF(opt)

    torch.manual_seed(0)
    ref = M.Graph(opt)
    shim = Graph(opt)
    ks_ref = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    ks_shim = {k: tuple(v.shape) for k, v in shim.state_dict().items()}
    print("reference Graph state_dict entries:", len(ks_ref), " shim:", len(ks_shim))
    assert ks_ref == ks_shim, set(ks_ref.items()) ^ set(ks_shim.items())
    shim.load_state_dict(ref.state_dict())                          # reference checkpoints load unchanged
    # our stock-compatible discriminator has the reference discriminator's keys as well
    d_ref = {k: tuple(v.shape) for k, v in ref.discriminator.state_dict().items()}
    d_amd = {k: tuple(v.shape) for k, v in AmdDisc(opt).state_dict().items()}
    assert d_ref == d_amd, set(d_ref.items()) ^ set(d_amd.items())
    print("discriminator state_dict identical:", len(d_ref), "entries")
    # the reference's trunk-only restore (util.restore_pretrain_partial_checkpoint) filters by these prefixes
    assert any(k.startswith("nerf.mlp_feat.") for k in ks_shim) and "nerf.progress" in ks_shim
    # signatures the reference engine calls (model/nerf_adapt_st_gan.py:471-545)
    import inspect
    for name in ("render", "render_by_slices", "compute_loss", "sample_geometry"):
        # (sample_geometry is a staticmethod in the reference and a method here; both are only ever called as
        # self.sample_geometry(opt, var, mode), :508,530 -- compare the argument lists without `self`)
        a = [p for p in inspect.signature(getattr(M.Graph, name)).parameters if p != "self"]
        b = [p for p in inspect.signature(getattr(Graph, name)).parameters if p != "self"]
        assert a == b[:len(a)], (name, a, b)
        print("signature ok:", name, a)
    # the other classes / functions of the boundary: same argument names, same order
    import camera as Rcam
    from texpose_amd import geometry as G
    from texpose_amd.nerf import NeRF as ANeRF
    def args(f):
        return [p for p in inspect.signature(f).parameters if p != "self"]
    for ref_f, our_f, name in (
            (NeRF.forward, ANeRF.forward, "NeRF.forward"), (NeRF.forward_samples, ANeRF.forward_samples, "NeRF.forward_samples"),
            (NeRF.composite, ANeRF.composite, "NeRF.composite"), (NeRF.positional_encoding, ANeRF.positional_encoding, "NeRF.positional_encoding"),
            (RaySampler.get_rays, G.RaySampler.get_rays, "RaySampler.get_rays"), (RaySampler.get_bounds, G.RaySampler.get_bounds, "RaySampler.get_bounds"),
            (RaySampler.get_image, G.RaySampler.get_image, "RaySampler.get_image"),
            (FlexPatchSampler.__call__, G.FlexPatchSampler.__call__, "FlexPatchSampler.__call__"),
            (Rcam.get_center_and_ray, G.get_center_and_ray, "camera.get_center_and_ray"),
            (Rcam.aabb_ray_intersection, G.aabb_ray_intersection, "camera.aabb_ray_intersection"),
            (M.Graph.sample_depth, AmdGraph.sample_depth, "Graph.sample_depth"), (M.Graph.ray_batch_sample, AmdGraph.ray_batch_sample, "Graph.ray_batch_sample")):
        a, b = args(ref_f), args(our_f)
        assert a == b[:len(a)], (name, a, b)
        print("signature ok:", name, a)
    print("shim signatures ok")
    with oracle_backend():
        run_evaluation(*run_training_steps(opt, M, Graph))
    from texpose_amd import ops
    assert ops.raygen.__module__ == "texpose_amd.ops" and AmdNeRF.forward_samples.__module__ == "texpose_amd.nerf"     # restored
    print("shim check passed")


def run_training_steps(opt, M, ShimGraph):
    """The reference's OWN engine (Model.train_iteration -> nerf_trainstep / disc_trainstep, model/nerf_adapt_st_gan.py:
    108-202) drives the shim Graph for two iterations, next to the pure reference Graph on the same weights, batch and
    random draws.  There is no GPU here, so the four C-ABI entry points the shim's methods reach (tp_raygen, tp_mlp_fwd
    /bwd, tp_composite, tp_patch_gather) are bound to the CPU oracle by the caller (tests/cpu_backend.py): what is exercised is
    the wiring through the reference's method-resolution order (nerf_forward -> render -> compute_loss -> sample_geometry ...)."""
    import copy
    import types
    import numpy as np
    from oracle import texpose_oracle as O
    from texpose_amd.graph import RenderMixin

    B, H, W, N = 2, 32, 32, 4
    opt = copy.deepcopy(opt)
    opt.H, opt.W, opt.batch_size, opt.patch_size = H, W, B, 16
    opt.nerf.sample_intvs, opt.data.image_size = N, [H, W]
    opt.loss_weight.feat = None                                   # (VGG weights unavailable offline)
    opt.max_epoch, opt.max_iter = 10, 1000
    for k in ("scalar", "vis", "val", "ckpt"):
        opt.freq[k] = 10 ** 9

    def model(graph_cls, seed):
        torch.manual_seed(seed)
        m = M.Model.__new__(M.Model)
        m.graph = graph_cls(opt)
        m.graph.latent_vars_trans = torch.nn.Embedding(6, opt.nerf.N_latent_trans)
        m.graph.latent_vars_light = torch.nn.Embedding(6, opt.nerf.N_latent_light)
        m.train_data = list(range(6))
        M.Model.setup_optimizer(m, opt)
        m.it, m.ep = 0, 0
        now = __import__("time").time()
        m.timer = types.SimpleNamespace(start=now, it_start=now, it_end=now, it_mean=None)
        return m

    ref, shim = model(M.Graph, 5), model(ShimGraph, 6)
    # what the mixin asks of its host, the reference's Graph (with the engine's latent tables) provides
    for name in RenderMixin.HOST_REQUIRED:
        assert hasattr(shim.graph, name), name
    assert [n for n in RenderMixin.HOST_OPTIONAL if hasattr(ref.graph, n)] == ["perceptual_loss"]
    assert shim.graph.perceptual_loss is not None
    state = O.seeded_state(ref.graph.state_dict(), salt=3)
    ref.graph.load_state_dict(state)
    shim.graph.load_state_dict(state)                              # same keys: the reference state dict loads into the shim
    rs = np.random.RandomState(4)
    f = lambda *sh: torch.from_numpy(rs.uniform(size=sh).astype(np.float32))
    yy, xx = np.mgrid[0:H, 0:W]
    disk = torch.from_numpy((((yy - H / 2) ** 2 + (xx - W / 2) ** 2) < (0.4 * H) ** 2).astype(np.float32))
    sc = O.synthetic_scene(H, W, B=B, seed=2)
    K = sc["intr"].clone()
    K[:, 0, 0] = K[:, 1, 1] = 700.0 * H / 128.0
    K[:, 0, 2], K[:, 1, 2] = W / 2.0, H / 2.0
    base = dict(idx=torch.tensor([1, 4]), image=f(B, 3, H, W), image_syn=f(B, 3, H, W), nocs_pred=f(B, 3, H, W),
                normal_pred=f(B, 3, H, W) * 2 - 1, obj_mask=disk[None].repeat(B, 1, 1), mask_syn=disk[None].repeat(B, 1, 1),
                intr=K, pose=sc["pose"], pose_init=sc["pose"], z_near=sc["z_near"], z_far=sc["z_far"])
    EasyDict = sys.modules["easydict"].EasyDict
    losses = {}
    for name, m in (("reference", ref), ("shim", shim)):
        torch.manual_seed(77)                                       # patch draws + stratified jitter + nothing else
        out = []
        for it in range(2):
            var = EasyDict({k: v.clone() for k, v in base.items()})
            gloss, dloss = M.Model.train_iteration(m, opt, var, loader=[0])
            out.append({**{"g." + k: float(v) for k, v in gloss.items()}, **{"d." + k: float(v) for k, v in dloss.items()}})
        losses[name] = out
    for it in range(2):
        for k, v in losses["reference"][it].items():
            w = losses["shim"][it][k]
            assert abs(v - w) <= 2e-4 * abs(v) + 1e-6, (it, k, v, w)
    moved = 0
    for (k, a), (_, b) in zip(ref.graph.state_dict().items(), shim.graph.state_dict().items()):
        assert torch.allclose(a, b, rtol=1e-3, atol=2e-5), (k, float((a - b).abs().max()))
        moved += int(not torch.equal(a, state[k]))
    assert moved > 20 and shim.it == 2 and shim.graph.patch_sampler.iterations == 1
    print("two reference-engine training iterations through the shim == through the reference Graph:",
          {k: round(v, 5) for k, v in losses["shim"][1].items()})
    return opt, ref.graph, shim.graph


def run_evaluation(opt, ref, shim):
    """What evaluate.py / validate reach, through the reference's OWN nerf_forward (model/nerf_adapt_st_gan.py:464-503) on both
    sides: the shim's render_by_slices -> render against the reference Graph's, same weights, same seeds, B = 1 on a disc mask."""
    import copy
    import numpy as np
    from oracle import texpose_oracle as O
    from texpose_amd.graph import RENDER_KEYS

    H, W = opt.H, opt.W
    shim.load_state_dict(ref.state_dict())                          # (the two training iterations left them a rounding apart)
    sc = O.synthetic_scene(H, W, B=1, seed=2)
    K = sc["intr"].clone()
    K[:, 0, 0] = K[:, 1, 1] = 700.0 * H / 128.0
    K[:, 0, 2], K[:, 1, 2] = W / 2.0, H / 2.0
    yy, xx = np.mgrid[0:H, 0:W]
    disk = torch.from_numpy((((yy - H / 2) ** 2 + (xx - W / 2) ** 2) < (0.4 * H) ** 2).astype(np.float32))
    rs = np.random.RandomState(11)
    u = lambda lo, hi: torch.from_numpy(rs.uniform(lo, hi, size=(1, H * W)).astype(np.float32))
    ndc_near = u(0.76, 0.8)                 # fractions of the NDC depth axis (the object sits at metric z ~ 6: t = 1 - 1 / z ~ 0.83)
    ranges = dict(metric=(sc["z_near"], sc["z_far"]), ndc=(ndc_near, ndc_near + u(0.06, 0.12)),
                  inverse=(1 / sc["z_far"], 1 / sc["z_near"]))
    anchors = O.synthetic_scene(H, W, B=5, seed=7)["pose"]
    EasyDict = sys.modules["easydict"].EasyDict
    off = disk.reshape(-1) == 0
    assert 0 < int(off.sum()) < H * W
    for label, mode, rng, flags in (("val", "val", "metric", {}), ("evaluation branch", "eval_noalign", "metric", {}),
                                    ("val, camera.ndc", "val", "ndc", dict(ndc=True)),
                                    ("val, nerf.depth.param = inverse", "val", "inverse", dict(param="inverse"))):
        o = copy.deepcopy(opt)
        o.camera.ndc, o.nerf.depth.param = flags.get("ndc", False), flags.get("param", "metric")
        o.arch.mlp_range_check = "off"                              # (the oracle is exact fp32 and keeps no device flag to read)
        out = []
        for graph in (ref, shim):
            var = EasyDict(idx=torch.tensor([0]), obj_mask=disk[None].clone(), intr=K.clone(), pose=sc["pose"].clone(),
                           pose_init=sc["pose"].clone(), pose_anchor=anchors.clone(), z_near=ranges[rng][0].clone(), z_far=ranges[rng][1].clone())
            torch.manual_seed(91)                                   # the light row's randperm, then the stratified draw
            with torch.no_grad():
                out.append(graph.nerf_forward(o, var, mode=mode))
        keys = [k for k in RENDER_KEYS if k in out[0] and k in out[1]]
        assert len(keys) == len(RENDER_KEYS), keys
        for k in keys:
            a, b = out[0][k], out[1][k]
            assert a.shape == b.shape and bool(torch.isfinite(b).all()), (label, k, a.shape, b.shape)
            # the bars tests/test_oracle_golden.py holds the oracle to for the G9 render slices (per-ray and per-sample maps alike)
            torch.testing.assert_close(b, a, rtol=2e-5, atol=2e-6, msg=lambda m: "%s, %s: %s" % (label, k, m))
            if mode != "val":                                       # pixels off the mask: the default fills, bit for bit
                assert torch.equal(a[0, off], b[0, off]), (label, k)
                assert not torch.equal(a[0, ~off], torch.broadcast_to(a[0, off][:1], a[0, ~off].shape)), (label, k)
        print("evaluation render through the shim == through the reference Graph:", label,
              " max |diff| rgb %.2e depth %.2e" % (float((out[0].rgb - out[1].rgb).abs().max()), float((out[0].depth - out[1].depth).abs().max())))


if __name__ == "__main__":
    main()
