"""The RP forest against its step-exact host model (tests/forest_reference.py): every split of every tree, at the shapes of
tests/forest_cases.py.  A mismatch names the tree, the depth, the segment, the regime, the pivots and the offending members."""
import time

import numpy as np
import pytest

from pynndescent_amd import _capi
from tests import forest_cases as FC
from tests.forest_reference import describe
from tests.gpu_util import make_builder

pytestmark = pytest.mark.gpu


def _builder(c, x, flags=0):
    return make_builder(x, c.metric, k=FC.K, n_trees=c.T, leaf_size=c.leaf_size, seed=c.seed, max_depth=c.max_depth, flags=flags)


def _check(c, model, la, what):
    res = model.run(la)
    print("%s %s: unclear %d / %d decisions, recording unclear %s, cells %d" % (c.name, what, res.unclear, res.decisions,
                                                                              res.recording_unclear, res.n_cells))
    assert all(m is None for m in res.mismatch), "%s %s:\n%s" % (c.name, what, describe(res.mismatch))
    assert res.unclear <= FC.UNCLEAR_CAP * max(res.decisions, 1), (c.name, what, res.unclear, res.decisions)
    return res


@pytest.mark.parametrize("name", [c.name for c in FC.WHOLE])
def test_whole_set_forest_is_the_models(name):
    c = FC.CASES[name]
    x = FC.case_data(c)
    t0 = time.perf_counter()
    b = _builder(c, x)
    b.make_forest()
    la = b.leaf_array()
    assert b.stats()["n_cells"] == 0
    res = _check(c, FC.case_model(c, x), la, "whole-set")
    assert res.n_cells == 0
    b.make_forest()
    assert np.array_equal(b.leaf_array(), la), "a second make_forest() on the handle differs"
    b.close()
    print("%s: %.2f s" % (name, time.perf_counter() - t0))


@pytest.mark.parametrize("name", [c.name for c in FC.ROUTING])
def test_routed_forest_is_the_models(name):
    """both routing forms (coherent, and the plain walk of NND_FLAG_TEST_ROUTE_PLAIN), each against the model."""
    c = FC.CASES[name]
    x = FC.case_data(c)
    t0 = time.perf_counter()
    model = FC.case_model(c, x)
    checked = []
    for what, flags in (("coherent", 0), ("plain", _capi.NND_FLAG_TEST_ROUTE_PLAIN)):
        b = _builder(c, x, flags)
        b.make_forest()
        la = b.leaf_array()
        n_cells = b.stats()["n_cells"]
        assert n_cells > 0, "the routing mode did not run"
        if not any(np.array_equal(la, old) for old in checked):  # (an array equal to a checked one is checked)
            res = _check(c, model, la, what)
            # the sample forest cannot be followed: the case's seed is chosen so that none of its decisions is unclear
            assert not any(res.recording_unclear), "precondition: %s has unclear recording decisions %s" % (name, res.recording_unclear)
            assert res.n_cells == n_cells, (res.n_cells, n_cells)
            checked.append(la)
        b.make_forest()
        assert np.array_equal(b.leaf_array(), la), "a second make_forest() on the handle differs (%s)" % what
        b.close()
    print("%s: %.2f s" % (name, time.perf_counter() - t0))
