"""The query kernel's float walk with the rerank epilogue (metric code 6, csrc/query.hip k_query<*, *, Q_FORM_RERANK, *>) against its
step-exact model (tests/proxy_reference.py), through _capi.Searcher.query_rerank directly: no index build.  For every query
the model does not flag, the ids are the model's and every distance is -<q, x> of its id within the float32 dot-product
radius (bit for bit on the lattice); flagged queries keep the weak checks.  Every case runs on the LDS tier and on the
global-memory tier, and the two answer identically.  The cases and their ambiguity cap are asserted without a GPU in
tests/test_proxy_cpu.py."""
import types

import numpy as np
import pytest

from pynndescent_amd import _capi
from tests import proxy_reference as PR
from tests import proxy_util as PU

pytestmark = pytest.mark.gpu


def _searcher(case, metric=PU.CODE):
    graph = types.SimpleNamespace(indptr=case.indptr, indices=case.indices)
    return _capi.Searcher(case.data, graph, case.tree, metric, case.min_distance, case.n_neighbors, case.rng_state)


def _both_tiers(case, queries=None, k=None, search_k=None):
    queries = case.queries if queries is None else queries
    s = _searcher(case)
    try:
        out = []
        for tier in (0, 1):
            s.set_tier(tier)
            ids, dist = s.query_rerank(queries, case.k if k is None else k, case.search_k if search_k is None else search_k, case.epsilon)
            out.append((ids, dist, s.last_spilled()))
        s.set_tier(0)
    finally:
        s.close()
    assert out[1][2] == len(queries)
    return out


def _weak(case, q, gi, gd):
    """sorted, unique, filled from the front, and every distance that of its id."""
    found = gi >= 0
    ok = bool(np.all(np.diff(gd[found]) >= 0) and np.all(found[:found.sum()]) and len(set(gi[found].tolist())) == found.sum())
    mid, rad = PU.neg_inner(q, case.data[gi[found]])
    return ok and bool(np.all(np.abs(gd[found] - mid) <= rad) and np.all(np.isposinf(gd[~found])))


def _check(label, case, res, ids, dist, exact=False):
    bad, n_exact = [], 0
    for i, r in enumerate(res):
        gi, gd = ids[i], dist[i].astype(np.float64)
        if not _weak(case, case.queries[i], gi, gd):
            bad.append("query %d: row not sorted / unique, or a distance is not -<q, x> of its id: %s %s" % (i, gi[:8].tolist(), gd[:8].tolist()))
        if r.ambiguous:
            continue
        n_exact += 1
        if not np.array_equal(gi, r.ids):
            bad.append("query %d: ids differ from position %d: gpu %s model %s" % (i, int(np.argmax(gi != r.ids)), gi[:12].tolist(), r.ids[:12].tolist()))
        elif exact and not np.array_equal(gd, r.dists):
            bad.append("query %d: distances differ: gpu %s model %s" % (i, gd[:6].tolist(), r.dists[:6].tolist()))
        elif not np.all(np.abs(gd - r.dists) <= r.radius):
            bad.append("query %d: distances outside the radius: gpu %s model %s radius %s" % (i, gd[:6].tolist(), r.dists[:6].tolist(), r.radius[:6].tolist()))
    print("%s: %d queries compared entry for entry, %d left to the weak checks, %d mismatching" % (label, n_exact, len(res) - n_exact, len(bad)))
    assert not bad, "%s: %d problems\n%s" % (label, len(bad), "\n".join(bad[:8]))


@pytest.mark.parametrize("d,k,search_k", PR.SEARCH_CASES)
def test_rerank_walk(d, k, search_k):
    """d = 17 and 24 (a padded and an unpadded row); (k, search_k) with one, two and four result entries per lane, and beam 1."""
    case, res = PR.search_case(d, k, search_k)
    (ids0, dist0, spilled0), (ids1, dist1, _) = _both_tiers(case)
    print("%s: %d of %d queries left the LDS tier on their own" % (case.name, spilled0, len(res)))
    assert ids0.shape == dist0.shape == (len(res), k) and ids0.dtype == np.int32 and dist0.dtype == np.float32
    _check(case.name + " LDS tier", case, res, ids0, dist0)
    _check(case.name + " global-memory tier", case, res, ids1, dist1)
    assert np.array_equal(ids0, ids1) and np.array_equal(dist0, dist1)


def test_lattice():
    """Integer rows and queries, dim * R^2 < 2^24: every float32 partial sum is an exact integer, so every returned distance
    is the exact integer -<q, x> of its id, bit for bit, and the unflagged queries return the model's ids."""
    case, res = PR.lattice_case()
    for tier, (ids, dist, _) in enumerate(_both_tiers(case)):
        _check("%s tier %d" % (case.name, tier), case, res, ids, dist, exact=True)
        assert (ids >= 0).all()
        exact = -np.einsum("qd,qkd->qk", case.queries.astype(np.float64), case.data[ids].astype(np.float64))
        assert np.array_equal(dist.astype(np.float64), exact)


def test_zero_query_zero_rows_and_nonpositive_products():
    """A zero query is searched (the reference skips a zero query under cosine and dot only): every proxy distance is FLT_MAX,
    the walk ends, the answer holds valid ids with distance -0 = 0.  Zero rows and rows in the negative orthant are FLT_MAX
    away from every query in the walk and still rerank by their true -<q, x>; a query in the negative orthant sees only
    non-positive products.  Nothing hangs, every id is valid or -1, every distance is -<q, x>."""
    case, _ = PR.search_case(17, 10, 40)
    x = case.data.copy()
    x[[3, 700, 1500]] = 0.0
    x[[5, 900]] *= -1.0
    q = case.queries[:8].copy()
    q[0] = 0.0
    q[1] = -q[1]
    q[2, ::2] = 0.0
    edge = types.SimpleNamespace(**{**case.__dict__, "data": x, "queries": q})
    for tier, (ids, dist, _) in enumerate(_both_tiers(edge, k=10, search_k=40)):
        assert ids.shape == (8, 10) and ((ids >= -1) & (ids < len(x))).all()
        for i in range(8):
            assert _weak(edge, q[i], ids[i], dist[i].astype(np.float64)), (tier, i, ids[i], dist[i])
        assert (ids[0] >= 0).all() and np.all(dist[0] == 0.0)
        # (a negated query has a positive product with the two negated rows alone)
        assert (ids[1] >= 0).all() and set(ids[1][dist[1] < 0.0].tolist()) <= {5, 900}
        assert (ids[2:] >= 0).all() and np.all(dist[2:] < 0.0)


def test_entry_point_errors():
    case, _ = PR.search_case(17, 10, 10)
    s = _searcher(case)
    try:
        for k, sk in ((10, 257), (10, 9), (0, 4), (300, 300)):
            with pytest.raises(_capi.NNDError, match="search_k"):
                s.query_rerank(case.queries[:2], k, sk, 0.1)
        with pytest.raises(_capi.NNDError, match="nnd_searcher_query_rerank"):
            s.query(case.queries[:2], 10, 0.1)  # the plain walk knows no code 6
    finally:
        s.close()
    s = _searcher(case, metric=3)
    try:
        with pytest.raises(_capi.NNDError, match="no true distance"):
            s.query_rerank(case.queries[:2], 10, 40, 0.1)
    finally:
        s.close()
