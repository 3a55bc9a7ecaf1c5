"""The lean 16-lane selection of the fused sampling kernel (csrc/sample.hip nnd_select_class: duplicate screen before the
compaction, ranks over an LDS list padded with empty keys, one store per candidate row) against the two forms that were left
as they are: the fused kernel with 32 lanes per vertex (NND_FLAG_TEST_SELECT_HALF) and the one-wave-per-vertex kernel on
rbuf banks (NND_FLAG_TEST_SELECT_WAVE).  Candidate lists and the flag resets in the graph must agree entry for entry."""
import numpy as np
import pytest

from pynndescent_amd import _capi
from tests.gpu_util import make_builder
from tests.util_data import clustered

pytestmark = pytest.mark.gpu

VARIANTS = (0, _capi.NND_FLAG_TEST_SELECT_HALF, _capi.NND_FLAG_TEST_SELECT_WAVE)


def _passes(b):
    """descent_sample() on the state as initialised (the wide pass: every edge new) and after one and two descent_iter()."""
    out = []
    for it in range(3):
        if it:
            b.descent_iter()
        b.descent_sample()
        new, old = b.candidates()
        idx, _, fl = b.graph()
        out.append((new, old, idx, fl))
    return out


def _compare(runs):
    base = runs[0]
    for flags, other in zip(VARIANTS[1:], runs[1:]):
        for it, ((new, old, idx, fl), (new_o, old_o, idx_o, fl_o)) in enumerate(zip(base, other)):
            tag = "flags %d pass %d" % (flags, it)
            np.testing.assert_array_equal(idx, idx_o, err_msg=tag + ": graph")
            np.testing.assert_array_equal(fl, fl_o, err_msg=tag + ": flag resets")
            np.testing.assert_array_equal(new, new_o, err_msg=tag + ": new lists")
            # (the old list of a vertex without new candidates is never read and not defined)
            joins = new[:, 0] >= 0
            np.testing.assert_array_equal(old[joins], old_o[joins], err_msg=tag + ": old lists")
    return base


@pytest.fixture(scope="module")
def points():
    return {n: clustered(n, 8, 4, 12, seed=29) for n in (257, 1000, 4000)}


@pytest.mark.parametrize("n", [257, 1000, 4000])
@pytest.mark.parametrize("k,mc", [(4, 4), (15, 15), (16, 16), (15, 5), (16, 5), (4, 5)])
def test_lean_select_equals_the_kept_forms(points, n, k, mc):
    """n = 257: a partial last bucket and idle groups in the last wave; mc = 5 at k = 16: lists much longer than what is kept,
    the threshold path with many survivors to reject."""
    x = points[n]
    runs = []
    for flags in VARIANTS:
        b = make_builder(x, "euclidean", k=k, n_trees=2, mc=mc, flags=flags)
        b.make_forest()
        b.init_from_leaves()
        b.init_random()
        runs.append(_passes(b))
        b.close()
    base = _compare(runs)
    new0, old0, _, fl0 = base[0]
    assert (new0[:, 0] >= 0).all() and (old0 == -1).all()  # first pass: every vertex joins, no old candidates yet
    assert (fl0 == 0).any() and (base[1][1] >= 0).any()    # edges were sampled; old candidates appear after an iteration


def _from_graph(x, init, k, mc):
    runs = []
    for flags in VARIANTS:
        b = make_builder(x, "euclidean", k=k, n_trees=0, mc=mc, flags=flags)
        b.init_from_graph(init)
        runs.append(_passes(b))
        b.close()
    return _compare(runs)


def test_hub_row_overflows_its_banks():
    """200 of 1000 rows name row 0: its banks overflow (the hashed fallback keeps the smallest word per slot, so the priorities
    of what is left are not uniform), the threshold estimate lets more than 2 x 16 items pass and the bisection moves down."""
    n, k = 1000, 15
    x = clustered(n, 8, 4, 12, seed=31)
    rs = np.random.RandomState(5)
    init = np.stack([rs.choice(np.delete(np.arange(n), i), k, replace=False) for i in range(n)]).astype(np.int32)
    for i in range(1, 201):
        if 0 not in init[i]:
            init[i, 0] = 0
    base = _from_graph(x, init, k, k)
    assert (base[0][0][0] >= 0).all()  # the hub's new list is full


def test_sparse_rows_with_few_items():
    """k = 4 with most slots empty and a few popular targets: lists shorter than max_candidates next to lists several times as
    long (where the threshold estimate undershoots, the bisection moves up)."""
    n, k = 1000, 4
    x = clustered(n, 8, 4, 12, seed=37)
    rs = np.random.RandomState(9)
    init = np.full((n, k), -1, np.int32)
    for i in range(n):
        m = rs.randint(0, 3)  # 0, 1 or 2 neighbours
        if m:
            init[i, :m] = rs.choice(np.delete(np.arange(n), i), m, replace=False)
    for i in range(20, 420):  # forty rows each name one of ten targets
        t = i % 10
        if t not in init[i]:
            init[i, 3] = t
    base = _from_graph(x, init, k, k)
    new0 = base[0][0]
    assert (new0[:10, k - 1] >= 0).all() and (new0[:, k - 1] < 0).any()
