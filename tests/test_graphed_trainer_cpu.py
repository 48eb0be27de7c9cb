"""CPU: the host-side shape of the two trainers (texpose_amd/trainer.py, texpose_amd/graphed_trainer.py).  Every attribute a method
reads is declared by ``__init__``; the linear graphs' streams, pools and stamps are the rows of one table; `form` names the step's form."""
import ast
import inspect
import re
import textwrap

import pytest

from texpose_amd.gan_modules import Discriminator
from texpose_amd.graph import Graph
from texpose_amd.graphed_trainer import LINEAR_GRAPHS, GraphedGanTrainer
from texpose_amd.options import default_options
from texpose_amd.trainer import GanTrainer


def _trainer(cls, with_disc):
    """As test_graphed_trainer_form_selection_for_several_ranks builds them."""
    opt = default_options(H=32, W=32, device="cpu")
    if not with_disc:
        opt.loss_weight.feat = opt.loss_weight.gan_nerf = None
        opt.gan = None
    g = Graph(opt, discriminator=Discriminator(opt) if with_disc else None)
    g.attach_latents(4, opt)
    return cls(opt, g, n_train=4)


def _self_reads(cls):
    """(names read as ``self.x``, getattr / hasattr calls on self as "method: call") in the class's own body."""
    tree = ast.parse(textwrap.dedent(inspect.getsource(cls))).body[0]
    loads, soft = set(), []
    for fn in (n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)):
        for n in ast.walk(fn):
            if isinstance(n, ast.Attribute) and isinstance(n.ctx, ast.Load) and isinstance(n.value, ast.Name) and n.value.id == "self":
                loads.add(n.attr)
            elif (isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in ("getattr", "hasattr") and n.args
                  and isinstance(n.args[0], ast.Name) and n.args[0].id == "self"):
                soft.append("%s: %s" % (fn.name, ast.unparse(n)))
    return loads, soft


@pytest.mark.parametrize("with_disc", [True, False])
@pytest.mark.parametrize("cls", [GanTrainer, GraphedGanTrainer])
def test_every_attribute_the_trainers_read_is_declared_by_init(cls, with_disc):
    tr = _trainer(cls, with_disc)
    assert tr.optim_disc is None or with_disc
    for c in (GanTrainer, GraphedGanTrainer) if cls is GraphedGanTrainer else (GanTrainer,):
        loads, soft = _self_reads(c)
        assert len(loads) > 30                                        # (the walker sees the class)
        assert not soft, "getattr / hasattr on self: %s" % soft
        assert "__dict__" not in loads
        missing = sorted(a for a in loads if not hasattr(tr, a))
        assert not missing, "%s reads attributes a fresh %s does not have: %s" % (c.__name__, cls.__name__, missing)


def test_linear_graph_table():
    want = {
        "D1":  ("side", "side", None, "D1.0", "D1.1"),
        "D1b": ("side", "side", "D1", None, None),
        "G1":  ("main", "main", None, "G1.0", "G1.1"),
        "F":   ("third", "main", None, "F.0", "F.1"),
        "G2a": ("main", "third", "G1", "G2a.0", "G2a.1"),
        "G2b": ("main", "main", "G1", "G2b.0", "G2b.1"),
        "G2c": ("main", "main", "G1", None, None),
        "D2a": ("side", "side", "D1", "D2.0", "D2a.1"),
        "D2b": ("side", "side", "D1", None, "D2.1"),
        "D2":  ("side", "side", "D1", "D2.0", "D2.1"),
        "D2c": ("side", "side", "D1", None, None),
    }
    assert {k: tuple(v) for k, v in LINEAR_GRAPHS.items()} == want
    assert LINEAR_GRAPHS["F"]._fields == ("captured_on", "replays_on", "pool", "stamp_before", "stamp_after")
    # a pool is shared with a graph of the same CAPTURING stream that has a pool of its own (and is captured earlier: dict order)
    names = list(LINEAR_GRAPHS)
    for name, row in LINEAR_GRAPHS.items():
        if row.pool is not None:
            owner = LINEAR_GRAPHS[row.pool]
            assert owner.pool is None and owner.captured_on == row.captured_on and names.index(row.pool) < names.index(name)
    # every graph the capture and the replay name is a row, and every row is captured and replayed
    tr = _trainer(GraphedGanTrainer, True)
    assert tr._stream("main") is tr._capture_stream and tr._stream("side") is tr._side and tr._stream("third") is tr._third
    for method in (GraphedGanTrainer._capture_linear, GraphedGanTrainer._replay_linear):
        fn = ast.parse(textwrap.dedent(inspect.getsource(method))).body[0]
        named = {n.value for n in ast.walk(fn) if isinstance(n, ast.Constant) and isinstance(n.value, str)
                 and re.fullmatch(r"F|[DG]\d[a-z]?", n.value)}
        assert named == set(LINEAR_GRAPHS), (method.__name__, sorted(named ^ set(LINEAR_GRAPHS)))


def test_form_names_the_captured_form():
    assert _trainer(GanTrainer, True).form == "eager" and _trainer(GanTrainer, False).form == "eager"
    tr = _trainer(GraphedGanTrainer, True)
    assert tr.form is None                                            # nothing captured yet
    tr._linear = tr._dp = True
    assert tr.form is None
    tr._graph = object()                                              # (stands in for the captured graph)
    assert tr.form == "linear_dp"
    tr._dp = False
    assert tr.form == "linear"
    tr._linear = False
    assert tr.form == "one_graph"
    tr._graph_b = object()
    assert tr.form == "two_graphs_eager_collectives"
    tr._graph = tr._graph_b = None                                    # (what load_optim_state leaves: the next iteration captures again)
    assert tr.form is None
    with pytest.raises(AttributeError):
        tr.form = "linear"
