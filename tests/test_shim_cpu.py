"""CPU: the reference-side drop-in is texpose_amd.graph.RenderMixin mixed into the reference's Graph.
These tests keep that surface closed: statically (every ``self.`` name the mixin reads is the mixin's own or one it declares it
expects of its host), dynamically (mixed into a host that provides nothing but the declared names, every entry point runs and
computes what the full Graph computes), in the documentation, and -- where the reference code base is present -- against it."""
import ast
import inspect
import os
import re
import subprocess
import sys
import textwrap

import pytest
import torch

from conftest import REPO
from cpu_backend import oracle_backend
from texpose_amd.graph import RENDER_KEYS, Graph, RenderMixin
from texpose_amd.nerf import NeRF
from texpose_amd.options import AttrDict, default_options
from texpose_amd.synthetic import training_batch

# what the reference's engine (train / validate / evaluate_full) and its own Graph methods call on a Graph and the drop-in answers;
# the private helpers behind them follow from the closure below
ENTRY_POINTS = {"render", "render_by_slices", "sample_depth", "ray_batch_sample", "gather_patches", "sample_geometry",
                "compute_loss", "evaluate_metrics"}


# ------------------------------------------------------------------------------------------------ static closure
def _mixin_reads():
    """{method: (bare, guarded)}: names read as ``self.x`` / ``RenderMixin.x``, names given as string literals to
    getattr(self, ...) / hasattr(self, ...).  Also the class node."""
    cls = ast.parse(textwrap.dedent(inspect.getsource(RenderMixin))).body[0]
    reads = {}
    for fn in (n for n in cls.body if isinstance(n, ast.FunctionDef)):
        bare, guarded = set(), set()
        for n in ast.walk(fn):
            if (isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Load) and isinstance(n.value, ast.Name)
                    and n.value.id in ("self", "RenderMixin")):
                bare.add(n.attr)
            elif (isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in ("getattr", "hasattr")
                  and isinstance(n.args[0], ast.Name) and n.args[0].id == "self"):
                assert isinstance(n.args[1], ast.Constant) and isinstance(n.args[1].value, str), \
                    "%s: %s(self, <not a literal>) cannot be checked" % (fn.name, n.func.id)
                guarded.add(n.args[1].value)
        reads[fn.name] = (bare, guarded)
    return cls, reads


def test_mixin_is_closed_under_its_self_references():
    cls, reads = _mixin_reads()
    own = set(reads)
    required, optional = set(RenderMixin.HOST_REQUIRED), set(RenderMixin.HOST_OPTIONAL)
    assert not required & optional and not (required | optional) & own
    assert len(RenderMixin.HOST_REQUIRED) == len(required) and len(RenderMixin.HOST_OPTIONAL) == len(optional)
    used = set().union(*(b | g for b, g in reads.values()))
    unresolved = {m: sorted(n for n in b | g if n not in own | required | optional | {"__dict__", "__class__"})
                  for m, (b, g) in reads.items()}
    assert not any(unresolved.values()), "RenderMixin reads names it neither defines nor declares: %s" % \
        {m: v for m, v in unresolved.items() if v}
    assert not (required | optional) - used, "declared but never read: %s" % sorted((required | optional) - used)
    # a read with no getattr / hasattr of the same name in the same method must resolve on any host
    unguarded = set().union(*(b - g for b, g in reads.values()))
    assert unguarded <= own | required | optional | {"__dict__", "__class__"}
    assert required <= unguarded, "only ever read behind a guard, so optional: %s" % sorted(required - unguarded)
    # the surface: the entry points, and exactly the private helpers they reach
    assert ENTRY_POINTS <= own, "missing entry points: %s" % sorted(ENTRY_POINTS - own)
    assert own - ENTRY_POINTS <= used, "helpers nothing in the mixin calls: %s" % sorted(own - ENTRY_POINTS - used)
    assert all(n.startswith("_") for n in own - ENTRY_POINTS), sorted(own - ENTRY_POINTS)
    assert not [n for n in ast.walk(cls) if isinstance(n, ast.Name) and n.id == "Graph"], "the mixin's body names Graph"


def test_mixin_is_a_plain_class_and_graph_keeps_the_rest():
    assert RenderMixin.__bases__ == (object,) and "__init__" not in vars(RenderMixin)
    assert Graph.__mro__[:3] == (Graph, RenderMixin, torch.nn.Module)
    assert not set(vars(Graph)) & set(vars(RenderMixin)) - {"__module__", "__doc__", "__dict__", "__weakref__"}


# ------------------------------------------------------------------------------------------------ dynamic closure
B, H, W, N, P, N_TRAIN = 2, 16, 16, 4, 8, 5


class Host(torch.nn.Module):
    """Nothing but RenderMixin.HOST_REQUIRED."""

    def __init__(self, opt):
        super().__init__()
        self.nerf = NeRF(opt)
        self.latent_vars_trans = torch.nn.Embedding(N_TRAIN, opt.nerf.N_latent_trans)
        self.latent_vars_light = torch.nn.Embedding(N_TRAIN, opt.nerf.N_latent_light)
        self.lab_loss = None

    MSE_loss = vars(Graph)["MSE_loss"]
    compute_gan_loss = vars(Graph)["compute_gan_loss"]


class G(RenderMixin, Host):
    pass


def _options():
    opt = default_options(H=H, W=W, device="cpu")
    opt.batch_size, opt.patch_size, opt.nerf.sample_intvs = B, P, N
    opt.loss_weight.feat = None
    opt.arch.mlp_range_check = "off"                    # (the oracle is exact fp32 and keeps no device flag to read)
    return opt


def _exercise(graph, opt):
    """Every entry point of the mixin that runs on CPU tensors, on fixed seeds -> {label: tensor}."""
    out = {}

    def keep(label, ret, keys=RENDER_KEYS):
        for k in keys:
            out[label + "." + k] = ret[k]

    batch = training_batch(B, H, W, n_train=N_TRAIN, seed=3, device="cpu")
    depth_range = (batch.z_near[:, :, None], batch.z_far[:, :, None])
    torch.manual_seed(21)
    coords = torch.rand(B, P, P, 2) * 1.6 - 0.8
    # render, training mode, and a backward pass through it
    var = AttrDict(dict(batch), ray_idx=coords)
    ret = graph.render(opt, var.pose, intr=var.intr, ray_idx=coords, depth_range=depth_range, sample_idx=var.idx, mode="train")
    keep("train", ret)
    (ret.rgb.sum() + ret.uncert.sum() + ret.density[..., 1].mean() + ret.depth.sum()).backward()
    for name in ("nerf.mlp_rgb.0.weight", "nerf.mlp_trans.3.bias", "latent_vars_trans.weight", "latent_vars_light.weight"):
        out["train.grad." + name] = graph.get_parameter(name).grad.clone()
    assert all(p.grad is None for p in graph.nerf.mlp_feat.parameters())
    var.update({k: v.detach() for k, v in ret.items()})
    # the patch samples
    var = graph.gather_patches(opt, var)
    assert graph.sample_geometry(opt, var, mode="train") is var and var.gathered_for is coords
    keep("gather", var, ("gathered", "image_sample", "image_syn_sample", "nocs_sample", "normal_sample", "mask_sample", "mask_syn_sample"))
    dense = graph.sample_geometry(opt, AttrDict(dict(batch)), mode="val")
    keep("geometry.val", dense, ("nocs_sample", "normal_sample"))
    # the generator's losses (patch mode), with and without the Lab term (torch ops on CPU tensors), and the discriminator's
    torch.manual_seed(22)
    var.d_fake_nerf, var.d_real_disc, var.d_fake_disc = torch.randn(3, B, 1, 3, 3).unbind(0)
    for lab in (None, 0):
        opt.loss_weight.lab = lab
        loss = graph.compute_loss(opt, var, mode="train", train_step="nerf")
        assert ("lab" in loss) == (lab is not None) and {"render", "uncert", "trans_reg", "gan_nerf"} <= set(loss)
        keep("loss.nerf.lab=%s" % lab, loss, sorted(loss))
    opt.loss_weight.lab = None
    keep("lab", var, ("rgb_lab", "img_syn_lab"))
    loss = graph.compute_loss(opt, var, mode="train", train_step="disc")
    assert set(loss) == {"gan_disc_real", "gan_disc_fake"}
    keep("loss.disc", loss, sorted(loss))
    # whole images, B = 1 as in the reference (its ray_batch_sample asserts it): validation (every pixel), evaluation (the pixels
    # of a partial mask; the rest keeps the default fills)
    one = dict(intr=batch.intr[:1], depth_range=tuple(d[:1] for d in depth_range))
    mask = torch.zeros(1, H, W)
    mask[0, 3:11, 5:14] = 1
    with torch.no_grad():
        torch.manual_seed(23)
        keep("val", graph.render_by_slices(opt, batch.pose[:1], object_mask=batch.obj_mask[:1], sample_idx=None, mode="val", **one))
        torch.manual_seed(24)
        ev = graph.render_by_slices(opt, batch.pose[:1], object_mask=mask, sample_idx=torch.tensor(2), mode="eval_noalign", **one)
    keep("eval", ev)
    off = mask.reshape(-1) == 0
    assert torch.all(ev.uncert[0, off] == float(opt.nerf.min_uncert)) and torch.all(ev.alpha_static[0, off] == 1)
    assert torch.all(ev.rgb[0, off] == 0) and not torch.all(ev.rgb[0, ~off] == 0)
    return out


def test_mixin_on_a_minimal_host_computes_what_graph_computes():
    opt = _options()
    torch.manual_seed(5)
    small, full = G(opt), Graph(opt)
    full.attach_latents(N_TRAIN, opt)
    full.nerf.load_state_dict(small.nerf.state_dict())
    full.latent_vars_trans.load_state_dict(small.latent_vars_trans.state_dict())
    full.latent_vars_light.load_state_dict(small.latent_vars_light.state_dict())
    assert not set(RenderMixin.HOST_OPTIONAL) & (set(vars(small)) | set(vars(Host)) | set(small._modules))
    raygen_before = __import__("texpose_amd").ops.raygen
    with oracle_backend():
        got, want = _exercise(small, opt), _exercise(full, opt)
    assert __import__("texpose_amd").ops.raygen is raygen_before and NeRF.forward_samples.__module__ == "texpose_amd.nerf"
    assert set(got) == set(want) and {k.split(".")[0] for k in got} == {"train", "gather", "geometry", "loss", "lab", "val", "eval"}
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), k
        assert torch.equal(v, want[k]), k


# ------------------------------------------------------------------------------------------------ documentation
def test_integration_md_shows_the_mixin_and_no_bindings():
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    section = text[text.index("## 1. "):text.index("## 2. ")]
    blocks = re.findall(r"```python\n(.*?)```", section, flags=re.S)
    shim = [b for b in blocks if "class Graph(" in b]
    assert len(shim) == 1
    assert "class Graph(RenderMixin, ref.Graph)" in shim[0]
    assert "= AmdGraph." not in shim[0]
    (graph,) = [n for n in ast.parse(shim[0]).body if isinstance(n, ast.ClassDef) and n.name == "Graph"]
    assert [n.name for n in graph.body if not isinstance(n, ast.Expr)] == ["__init__"]          # (Expr: the docstring)


# ------------------------------------------------------------------------------------------------ against the reference
def test_check_shim_against_the_reference_when_present():
    """tests/golden/check_shim_here.py in a child process: the reference's modules and sys.path edits stay out of this one."""
    ref = os.environ.get("TEXPOSE_REFERENCE", "/root/reference")            # as tests/golden/make_golden.py locates it
    if not os.path.isdir(ref):
        pytest.skip("the reference code base is not on this machine")
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "golden", "check_shim_here.py")], env=env, cwd=REPO,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "shim check passed" in r.stdout
