"""metric="proxy_inner_product" through the class API on a real MI355X, against the reference's own recorded behaviour
(tests/golden/proxy_inner_product.npz, written by tests/golden/make_golden_proxy.py from the un-jitted reference): the graph on
the proxy distance, queries reranked by the true inner product, pickling, update() and nn_descent.

Recalls are compared as five-seed means (seeds 3 .. 7 on both sides), two-sided, within the margin of tests/proxy_util.py: the
larger of 0.01 and three standard errors of the difference of the two means, computed from the per-seed values."""
import pickle

import numpy as np
import pytest

import pynndescent_amd
from pynndescent_amd import NNDescent
from tests import proxy_util as PU

pytestmark = pytest.mark.gpu
_BUILT = {}


def _golden():
    return np.load(PU.GOLDEN)


def _index(seed):
    if seed not in _BUILT:
        x, _ = PU.fixture_data()
        _BUILT[seed] = NNDescent(x, metric=PU.METRIC, n_neighbors=PU.K, random_state=seed)
    return _BUILT[seed]


def test_neighbor_graph_against_the_fixture():
    g = _golden()
    x, _ = PU.fixture_data()
    truth = PU.proxy_truth(x)
    ours, theirs = [], []
    for seed in PU.SEEDS:
        index = _index(seed)
        assert index._is_proxy_distance is True and index._angular_trees is False
        idx, dist = index.neighbor_graph
        assert idx.shape == dist.shape == (2000, PU.K) and (idx >= 0).all() and dist.dtype == np.float32
        assert (np.diff(dist.astype(np.float64), axis=1) >= 0).all()
        mid, rad = PU.proxy_pairs_f64(x[:, None, :], x[idx])  # the proxy distances themselves: no correction
        assert np.all(np.abs(dist.astype(np.float64) - mid) <= rad)
        ours.append(PU.recall(truth, idx))
        theirs.append(float(g["graph_recall_%d" % seed]))
    m = PU.margin(ours, theirs)
    print("graph recall@10 against float64 proxy brute force: ours %s mean %.4f, reference %s mean %.4f, margin %.4f" % (
        ["%.4f" % v for v in ours], np.mean(ours), ["%.4f" % v for v in theirs], np.mean(theirs), m))
    assert abs(np.mean(ours) - np.mean(theirs)) <= m


@pytest.mark.parametrize("beam", [4, 1])
def test_query_against_the_fixture(beam):
    g = _golden()
    x, q = PU.fixture_data()
    mips = PU.mips_truth(x, q)
    ours, theirs = [], []
    for seed in PU.SEEDS:
        qi, qd = _index(seed).query(q, k=PU.K, proxy_beam_size=beam)
        assert qi.shape == qd.shape == (200, PU.K) and qi.dtype == np.int32
        assert ((qi >= 0) & (qi < 2000)).all() and all(len(set(r.tolist())) == PU.K for r in qi)
        assert (np.diff(qd.astype(np.float64), axis=1) >= 0).all()
        for r in range(0, 200, 7):  # the true distance of the ORIGINAL row number: -<q, x>, neither clamped nor corrected
            mid, rad = PU.neg_inner(q[r], x[qi[r]])
            assert np.all(np.abs(qd[r].astype(np.float64) - mid) <= rad), (seed, r)
        ours.append(PU.recall(mips, qi))
        theirs.append(float(g["q_recall_b%d_%d" % (beam, seed)]))
    m = PU.margin(ours, theirs)
    print("query beam %d recall@10 against true MIPS: ours %s mean %.4f, reference %s mean %.4f, margin %.4f" % (
        beam, ["%.4f" % v for v in ours], np.mean(ours), ["%.4f" % v for v in theirs], np.mean(theirs), m))
    assert abs(np.mean(ours) - np.mean(theirs)) <= m


def test_prepare_mirrors_the_reference():
    g = _golden()
    index = _index(3)
    index.prepare()
    assert index._is_proxy_distance is True
    assert abs(float(index._min_distance) - float(g["min_distance_3"])) < 5e-3  # the smallest proxy distance of an edge
    assert sorted(index._vertex_order.tolist()) == list(range(2000))
    with pytest.raises(NotImplementedError, match="proxy_inner_product"):
        index.recall()
    with pytest.raises(NotImplementedError, match="256"):
        index.query(np.zeros((1, 16), np.float32), k=100, proxy_beam_size=3)


def test_pickle_round_trip_answers_identically():
    _, q = PU.fixture_data()
    index = _index(4)
    a = index.query(q, k=PU.K)
    clone = pickle.loads(pickle.dumps(index))
    assert clone._is_proxy_distance is True
    b = clone.query(q, k=PU.K)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_update_with_fresh_rows():
    x, q = PU.fixture_data()
    index = NNDescent(x[:1500], metric=PU.METRIC, n_neighbors=PU.K, random_state=5)
    index.prepare()
    index.update(xs_fresh=x[1500:])
    idx, dist = index.neighbor_graph
    assert idx.shape == (2000, PU.K) and (idx >= 0).all()
    mid, rad = PU.proxy_pairs_f64(x[:, None, :], x[idx])
    assert np.all(np.abs(dist.astype(np.float64) - mid) <= rad)
    rec = PU.recall(PU.proxy_truth(x), idx)
    qi, qd = index.query(q, k=PU.K)
    assert ((qi >= 0) & (qi < 2000)).all() and (qi >= 1500).any()
    mid, rad = PU.neg_inner(q[0], x[qi[0]])
    assert np.all(np.abs(qd[0].astype(np.float64) - mid) <= rad)
    print("after update(): graph recall@10 against float64 proxy brute force %.4f" % rec)
    assert rec > 0.9


def test_compressed_and_from_graph():
    x, q = PU.fixture_data()
    built = _index(3)
    wrapped = NNDescent.from_graph(x, *built._neighbor_graph, metric=PU.METRIC, random_state=3, compressed=True)
    qi, qd = wrapped.query(q[:20], k=PU.K)
    assert not hasattr(wrapped, "_neighbor_graph") and ((qi >= 0) & (qi < 2000)).all()
    mid, rad = PU.neg_inner(q[3], x[qi[3]])
    assert np.all(np.abs(qd[3].astype(np.float64) - mid) <= rad)


def test_nn_descent_returns_proxy_distances():
    from oracle import oracle as O

    x, _ = PU.fixture_data()
    state, _, ts = O.draw_rng_states(11, 4)
    la = O.make_leaf_array(x, 4, O.default_leaf_size(PU.K), ts, False)
    for dist in (PU.METRIC, type("f", (), {"__name__": PU.METRIC})()):
        gi, gd = pynndescent_amd.nn_descent(x, PU.K, state.copy(), max_candidates=PU.K, dist=dist, n_iters=8, rp_tree_init=True, leaf_array=la)
        assert (gi >= 0).all()
        mid, rad = PU.proxy_pairs_f64(x[:, None, :], x[gi])
        assert np.all(np.abs(gd.astype(np.float64) - mid) <= rad)  # uncorrected
    rec = PU.recall(PU.proxy_truth(x), gi)
    print("nn_descent(dist=proxy_inner_product): recall@10 against float64 proxy brute force %.4f" % rec)
    assert rec > 0.9
