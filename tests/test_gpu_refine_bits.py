"""The silhouette and the joint step and the four refinement loops against the words, the key order and the captured launch count they
gave before the refiners moved behind one term table (ops/refine.py).  Their outputs are a function of the inputs alone (no atomics,
one fixed order per fp64 sum), so tests/golden/g26_refine_loops.npz -- recorded by tests/golden/make_golden_g26_refine_loops.py, whose
cases this file runs again -- must be met bit for bit: a changed argument, pass order, key order or launch sequence shows here."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_steps_and_loops_give_the_recorded_words():
    spec = importlib.util.spec_from_file_location("make_golden_g26_refine_loops", os.path.join(GOLDEN, "make_golden_g26_refine_loops.py"))
    recipe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(recipe)
    want = np.load(os.path.join(GOLDEN, recipe.NAME + ".npz"))
    got = recipe.record()
    assert sorted(got) == sorted(want.files)
    for k in want.files:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:8])
