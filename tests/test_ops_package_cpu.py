"""The package texpose_amd/ops/ as a whole, read from its source: it offers every name the single module offered, every launch names
its entry point once, as a literal that the header declares as a launch, the six functions that tools and tests replace on ``ops`` are
reached through ``ops`` alone, and `_call` raises what `_lib.check` raises.  No device and no built library is needed."""
import ast
import ctypes as C
import importlib
import pathlib
import re

import pytest

from texpose_amd import _lib, ops
from texpose_amd.ops import _base

PACKAGE = pathlib.Path(ops.__file__).parent
TREES = {p.name: ast.parse(p.read_text()) for p in sorted(PACKAGE.glob("*.py"))}
STAGES = [name[:-3] for name in TREES if name != "__init__.py"]

# What the module texpose_amd/ops.py offered before it became a package.  Made on the commit before the split by
#   python -c "import textwrap, texpose_amd.ops as o; print(textwrap.fill(' '.join(n for n in sorted(vars(o)) if not (n.startswith('__')
#       and n.endswith('__')) and n not in 'C functools torch Tensor Dict Optional Tuple annotations knobs check'.split()), 150))"
SURFACE = """
BOUNDS_AABB BOUNDS_MAP BOUNDS_NONE COMPOSITE_RAY_FIELDS CompositeArgs CompositeBwdArgs DEPTH_PARAMS DISC_TAIL_MAX_ROWS F16_RANGE_PRECISIONS
INFERENCE_ONLY_PRECISIONS JITTER_GIVEN JITTER_MID JITTER_PHILOX MLP_F16 MLP_F16X3 MLP_FP32 MlpBwdArgs MlpFwdArgs MlpWeights NN1_MODES PACK_ALL
PACK_F16 PACK_F16X3 PACK_HEADS PACK_RAYBIAS PACK_TRUNK PAIRABLE PIX_COORDS PIX_INDEX PNP_MAX_HYP PNP_MAX_ITERS PNP_RANSAC_KEYS PRECISIONS
PatchGatherArgs RANGE_MESSAGE RaygenArgs SCENE_BOUNDS_KEYS SCENE_INFO_KEYS SCENE_SOURCES SKINNY_DGRAD_MAX_ROWS SKINNY_MAX_ROWS SN_MAX_SETS
SURFEL_FINISH_KEYS _act_max_ptr _act_max_words _bwd_scratch _composite_args _conv4s2 _conv_counters _conv_counters_retired _conv_scratch _f32
_feat_args _feat_chain_scratch _float3 _head_args _intr_per_view _lab_loss_args _lattices _launch _lengths _lib _nerf_losses_args _on_tensor_device
_out_like _outputs _pair_slot _pair_state _pending_total _pnp_common _points _poses _ptr _status_polls _status_words _stream _tail_args
_tail_workspace _tail_ws _tensors _ticket _ticket_words _track_act_max _want_gpu _workspace _workspace_arg _workspaces aabb_intersect adam_step
bce_logits_bwd bce_logits_fwd capture_node_count check_mlp_status clock_ghz_from_probe clock_probe composite_bwd composite_fwd conv3s1_dgrad
conv3s1_fwd conv3s1_supported conv4s2_dgrad conv4s2_dgrad_inorm_supported conv4s2_fwd conv4s2_fwd_inorm conv4s2_fwd_inorm_supported conv4s2_wgrad
corr_from_nocs disc_head_bwd disc_head_bwd_bwd disc_head_fwd disc_inputs disc_tail_bwd disc_tail_bwd_bwd disc_tail_eligible disc_tail_fwd eval_metrics
fake_patch_bwd feat_chain feat_chain_pack feat_chain_supported feat_inputs_bwd feat_inputs_fwd feat_pair_loss_bwd feat_pair_loss_fwd
flush_pending_total gan_disc_losses grad_pack inorm_lrelu_bwd inorm_lrelu_bwd_bwd inorm_lrelu_fwd lab_loss_bwd lab_loss_fwd latent_rows_bwd
latent_rows_fwd maxpool2_bwd maxpool2_fwd mesh_raster mlp_backward mlp_forward mlp_status nerf_losses_bwd nerf_losses_fwd nn1 normals_from_depth
pack_heads_train pack_weights packed_bytes packed_t_bytes paired patch_coords patch_gather pnp_hypotheses pnp_ransac pnp_refine pnp_score
pnp_workspace poll_mlp_status pose_errors posenc ray_bias_applies raygen render_eval rmsprop_step sample_depth scene_annotate scene_bounds
skinny_linear_dgrad skinny_linear_fwd skinny_linear_wgrad spectral_norm_buffers spectral_norm_bwd spectral_norm_fwd spectral_norm_fwd_sets stamp
step_flags step_inputs sumsq_mean_bwd sumsq_mean_fwd sumsq_mean_fwd_bwd surfel_finish take_activation_max take_mlp_status texture_bake
texture_bake_workspace track_activation_max view_images vsd weighted_sum
""".split()

REPLACED_ON_OPS = ("mlp_forward", "raygen", "composite_fwd", "patch_gather", "step_inputs", "mlp_backward")

# Launch entry points of the header that no wrapper calls, each with its reason.  The module before the split called every one of them
# (its text named each launch of the header, the *_pair ones through _launch), so there is none to excuse.
NOT_WRAPPED = {}


# int returns whose last parameter is a pointer but no stream
NO_STREAM = {"tp_mlp_pack_host": "packs on the host: its last parameter is the float* it fills"}


def header_launches():
    """The prototypes that are launches with a status: they return int and their last parameter is the tp_stream_t.  Selected from the
    binding's own prototypes (where tp_stream_t is a void*) and, since a float* looks the same there, held against the header's text."""
    bound = {n for n, (restype, argtypes) in _lib.HEADER.prototypes.items() if restype is C.c_int and argtypes and argtypes[-1] is C.c_void_p}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", pathlib.Path(_lib.HEADER_PATH).read_text(), flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    written = {m[1] for m in re.finditer(r"(?<![\w*])int\s+(tp_\w+)\s*\(([^;{}()]*)\)\s*;", text) if re.search(r"\btp_stream_t\s+\w+\s*$", m[2])}
    assert written == bound - set(NO_STREAM) and set(NO_STREAM) <= bound, sorted(written ^ bound)
    return written


def calls_of(name):
    """(file, enclosing top-level function or class, the Call node) of every call of the bare name ``name`` or of ``x.name``."""
    for file, tree in TREES.items():
        for top in tree.body:
            for node in ast.walk(top):
                if isinstance(node, ast.Call) and name == (node.func.id if isinstance(node.func, ast.Name) else getattr(node.func, "attr", None)):
                    yield file, getattr(top, "name", None), node


def literal(node):
    return node.value if isinstance(node, ast.Constant) and isinstance(node.value, str) else None


def defined_at_top_level(tree):
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            yield node.name
        elif isinstance(node, (ast.Assign, ast.AnnAssign)):
            for target in node.targets if isinstance(node, ast.Assign) else [node.target]:
                yield from (e.id for e in (target.elts if isinstance(target, ast.Tuple) else [target]))


def test_surface_is_the_single_modules():
    assert len(SURFACE) == 188 and not [n for n in SURFACE if not hasattr(ops, n)]
    owner = {}
    for stage in STAGES:
        for name in set(defined_at_top_level(TREES[stage + ".py"])) - {"__all__"}:
            assert owner.setdefault(name, stage) == stage, "%s is defined in %s and in %s" % (name, owner[name], stage)
    # what is re-exported is the defining module's own object: for the state dicts that is what keeps ops._ticket_words and the like
    # showing what the wrappers use (_track_act_max is a bool that track_activation_max rebinds in render: ops shows its value at import,
    # nothing reads it there, and it is listed only because the single module had it)
    shared = {n for n in SURFACE if isinstance(getattr(ops, n), (dict, list))}
    assert {"_ticket_words", "_pair_state", "_pending_total", "_conv_counters", "_feat_chain_scratch", "_status_words", "_workspaces"} <= shared <= set(owner)
    for name in SURFACE:
        home = importlib.import_module("texpose_amd.ops." + owner[name]) if name in owner else _lib
        assert getattr(ops, name) is (_lib if name == "_lib" else getattr(home, name)), name


def test_every_launch_names_a_launch_of_the_header_once():
    launches = header_launches()
    named = set()
    for file, where, call in calls_of("_call"):
        name = literal(call.args[0])
        if where == "_launch" and name is None:      # _launch hands on its own first argument, which the loop below holds to literals
            assert ast.unparse(call.args[0]) in ("name", "name + '_pair'"), (file, call.lineno)
            continue
        assert name is not None, "%s:%d: _call without a literal entry point" % (file, call.lineno)
        assert name in launches, "%s:%d: %s is not a launch of the header" % (file, call.lineno, name)
        named.add(name)
    for file, where, call in calls_of("_launch"):
        name = literal(call.args[0])
        assert name is not None, "%s:%d: _launch without a literal entry point" % (file, call.lineno)
        assert name in launches and name + "_pair" in launches and name in ops.PAIRABLE, (file, call.lineno, name)
        named |= {name, name + "_pair"}
    assert len(named) > 80 and not set(NOT_WRAPPED) & named
    assert launches - named == set(NOT_WRAPPED), sorted(launches - named ^ set(NOT_WRAPPED))
    # check() is left to _call; the two others refuse a workspace query that returned a negative size, where nothing is launched
    left = sorted((file, where, ast.unparse(call.args[0]), literal(call.args[1])) for file, where, call in calls_of("check"))
    assert left == [("_base.py", "_call", "rc", None), ("feat.py", "feat_chain", "-1", "tp_feat_chain_workspace"),
                    ("gan.py", "_conv_scratch", "-1", "tp_conv_workspace")], left
    assert not [1 for tree in TREES.values() for n in ast.walk(tree) if isinstance(n, ast.Name) and n.id == "_stream" and tree is not TREES["_base.py"]
                and not isinstance(n.ctx, ast.Load)]


def test_replaced_functions_are_reached_through_ops_only():
    for name in REPLACED_ON_OPS:
        assert not [(file, call.lineno) for file, _, call in calls_of(name) if isinstance(call.func, ast.Name)], name
    for file, tree in TREES.items():
        if file == "__init__.py":                   # (its star imports are the re-export itself: ops.<name> IS what gets replaced)
            continue
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom):
                assert not {a.name for a in node.names} & (set(REPLACED_ON_OPS) | {"*"}), "%s:%d imports %s" % (file, node.lineno, [a.name for a in node.names])


class FakeLibrary:
    def __init__(self):
        self.got = []

    def tp_fake(self, *args):
        self.got.append(args)
        return 7 if args[0] else 0

    def tp_last_error(self):
        return b"tp_fake: the library's own words"


def test_call_raises_what_check_raises(monkeypatch):
    fake = FakeLibrary()
    monkeypatch.setattr(_lib, "_lib", fake)
    monkeypatch.setattr(_base, "_stream", lambda: 0x5EED)
    with pytest.raises(_lib.TexposeLibraryError) as wanted:
        _lib.check(7, "tp_fake")
    with pytest.raises(_lib.TexposeLibraryError) as got:
        _base._call("tp_fake", 1)
    assert str(got.value) == str(wanted.value) == "tp_fake failed (rc=7): tp_fake: the library's own words"
    assert _base._call("tp_fake", 0, "x") is None
    assert fake.got == [(1, 0x5EED), (0, "x", 0x5EED)]                      # the current stream goes last
    with pytest.raises(AttributeError, match="tp_missing"):                  # a misspelt entry point is an error, not a silent no-op
        _base._call("tp_missing")
