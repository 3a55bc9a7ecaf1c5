"""Per-query filters on the GPU: the Q_FILT_TAGS instances of k_query (csrc/query.hip) against the tagged step-exact model
(tests/tag_filter_reference.py), the masked instances of csrc/exact.hip against numpy float64 brute force among the allowed
rows, the count kernel, and ``NNDescent.set_row_tags`` / ``query(query_tags=...)`` with its walk, exact and auto paths."""
import types

import numpy as np
import pytest

from pynndescent_amd import NNDescent, _capi, exact_knn, filtered
from pynndescent_amd.metrics import _metric_record
from tests import boolean_util as BU
from tests import exact_util as XU
from tests import filter_reference as FR
from tests import proxy_reference as PR
from tests import search_cases as SC
from tests import search_reference as SR
from tests import tag_filter_reference as TR
from tests.test_gpu_filtered_search import _bool_case, _check_rerank
from tests.test_gpu_search_exact import _case_searcher, _check
from tests.util_data import clustered

pytestmark = pytest.mark.gpu
TIERS = (0, 1)
U64 = np.uint64
BIT63 = U64(1) << U64(63)


def _form(case):
    return "proxy" if getattr(case, "values", None) is not None else "float"


def _tagged(case, s, masks, tier, form=None):
    s.set_tier(tier)
    try:
        ids, dist = s.query_tagged(form or _form(case), case.queries, masks, case.k, getattr(case, "search_k", None) or case.k, case.epsilon)
        return ids, dist, s.last_spilled()
    finally:
        s.set_tier(0)


def _each_allowed(label, ids, tags, masks):
    for i in range(len(ids)):
        got = ids[i][ids[i] >= 0]
        assert TR.allowed_of(tags, masks[i])[got].all(), "%s: query %d (mask %#x) got a row its mask does not allow" % (label, i, int(masks[i]))


# ------------------------------------------------------------------------------------------------ 1. the walk, step-exact
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", FR.lattice_names() + sorted(SC.Q8))
def test_walk_is_the_model(name, tier):
    """Every lattice case (k = 10 / 129 / 256 among them: one, two and four result entries per lane) and every uint8 case, both
    tiers: tags at about 0.5 / 0.1 / 0.02, query i under mask 1 << (i % 3), some two-bit masks, one mask that is bit 63 alone.
    Unflagged queries are the model's, ids and distance bits; flagged ones keep the weak checks."""
    case, tags, masks, res = TR.get(name)
    s = _case_searcher(case)
    try:
        s.set_tags(tags)
        ids, dist, spilled = _tagged(case, s, masks, tier)
        counts = s.count_tags(np.unique(masks))
    finally:
        s.close()
    label = "%s tier %d" % (name, tier)
    print("%s: rows per distinct mask %s, %d of %d queries on the global-memory tier, %d flagged by the model" % (
        label, counts.tolist(), spilled, len(res), sum(r.ambiguous for r in res)))
    np.testing.assert_array_equal(counts, [int(TR.allowed_of(tags, m).sum()) for m in np.unique(masks)])
    assert spilled == len(res) if tier == 1 else spilled <= len(res)
    _each_allowed(label, ids, tags, masks)
    _check(label, case, res, case.queries, ids, dist, case.exact)


@pytest.mark.parametrize("which", ["lattice", (24, 30, 120), (17, 50, 200)], ids=["lattice_sk30", "d24_sk120", "d17_sk200"])
def test_proxy_inner_product_rerank(which):
    """metric code 6: the float walk keeps search_k candidates its query's mask allows, the rerank by -<q, x> returns k."""
    lattice = which == "lattice"
    case, _ = PR.lattice_case() if lattice else PR.search_case(*which)
    n = case.data.shape[0]
    tags, masks = TR.case_tags(n), TR.case_masks(len(case.queries))
    masks[masks == U64(4)] = U64(1)  # (tag 2 is on about 8 / 40 rows here: its lists would stay nearly empty)
    walk = FR._FilteredWalk(np.zeros(n, bool), n, np.asarray(case.indptr, np.int64), np.asarray(case.indices, np.int64), case.tree,
                            PR._ProxyDistances(case.data, lattice), case.min_distance, int(case.n_neighbors), int(case.search_k), case.epsilon,
                            SR.searcher_seed(case.rng_state), False)
    res = TR.run_walk(walk, tags, masks, case.queries, case.search_k, int(case.k))
    graph = types.SimpleNamespace(indptr=case.indptr, indices=case.indices)
    s = _capi.Searcher(case.data, graph, case.tree, 6, case.min_distance, case.n_neighbors, case.rng_state)
    try:
        s.set_tags(tags)
        for tier in TIERS:
            ids, dist, spilled = _tagged(case, s, masks, tier, form="rerank")
            assert tier == 0 or spilled == len(res)
            _each_allowed(case.name, ids, tags, masks)
            _check_rerank("%s tagged tier %d" % (case.name, tier), case, res, ids, dist, exact=lattice)
    finally:
        s.close()


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("k", [10, 100, 129])
def test_boolean_family_walk(k, tier):
    """k_query's boolean form under query masks (dice, 1500 x 133; k = 10 / 100 / 129: one, two and four result entries per lane), as
    the single-set test: with a bound that never closes the walk visits the whole
    connected graph, and the returned distances are the k smallest over the rows the query's own mask allows, bit for bit."""
    case = _bool_case()
    n = case.data.shape[0]
    want = BU.dist(case.metric, case.queries, case.data, f32=True).astype(np.float32)
    tags = TR.case_tags(n)
    masks = np.where(np.arange(len(case.queries)) % 2 == 0, U64(1), U64(2))
    masks[5] = BIT63
    graph = types.SimpleNamespace(indptr=case.indptr, indices=case.indices)
    s = _capi.Searcher(case.data, graph, case.tree, BU.CODES[case.metric], case.min_distance, case.n_neighbors, case.rng_state)
    try:
        s.set_tags(tags)
        for eps in (1e6, 0.125):
            case.k, case.epsilon = k, eps
            ids, dist, spilled = _tagged(case, s, masks, tier)
            label = "dice k %d, epsilon %g, tier %d" % (k, eps, tier)
            _each_allowed(label, ids, tags, masks)
            for i in range(len(ids)):
                found = ids[i] >= 0
                gi, gd = ids[i][found], dist[i][found]
                assert found[:found.sum()].all() and len(set(gi.tolist())) == len(gi) and np.all(np.diff(gd) >= 0), label
                assert np.array_equal(gd.view(np.uint32), want[i, gi].view(np.uint32)), label
                if eps == 1e6:
                    allowed = TR.allowed_of(tags, masks[i])
                    assert allowed.sum() >= k and found.all()
                    best = np.sort(want[i][allowed])[:k]
                    assert np.array_equal(dist[i].view(np.uint32), best.view(np.uint32)), label
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ 2. ties to the single set
TIE_CASES = ["width_k10_nn10", "width_k129_nn30", "width_k256_nn10", "graph_islands_k200"]


@pytest.mark.parametrize("name", TIE_CASES)
def test_one_mask_for_all_is_the_single_set_walk(name):
    """The same mask for every query: the tagged instance returns what the filtered instance returns for the allow set
    ``(tags & m) != 0``, ids and distance bits, on both tiers."""
    case, _ = SC.get(name)
    tags = TR.case_tags(case.data.shape[0])
    s = _case_searcher(case)
    try:
        s.set_tags(tags)
        for m in (U64(1), U64(0b110), BIT63):
            for tier in TIERS:
                got = _tagged(case, s, np.full(len(case.queries), m, U64), tier)
                s.set_tier(tier)
                s.set_filter(TR.allowed_of(tags, m))
                want = s.query(case.queries, case.k, case.epsilon)
                s.clear_filter()
                s.set_tier(0)
                np.testing.assert_array_equal(got[0], want[0])
                np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    finally:
        s.close()


@pytest.mark.parametrize("name", TIE_CASES)
def test_one_mask_for_all_is_the_single_set_exact_path(name):
    """... and the masked scan over all rows returns what the single set's exact path returns -- ``exact_knn`` on the compact copy
    of the allowed rows, ids mapped back (filtered.query_exact) -- on lattice rows, which are full of exact ties."""
    case, _ = SC.get(name)
    metric = case.metric
    tags = TR.case_tags(case.data.shape[0])
    for m in (U64(1), U64(0b110)):
        allowed = np.flatnonzero(TR.allowed_of(tags, m))
        kk = min(int(case.k), len(allowed))
        sub_i, sub_d = exact_knn(case.data[allowed], case.queries, kk, metric=metric)
        ids, dist = exact_knn(case.data, case.queries, min(int(case.k), case.data.shape[0]), metric=metric, row_tags=tags,
                              query_tags=np.full(len(case.queries), m, U64))
        np.testing.assert_array_equal(ids[:, :kk], allowed[sub_i])
        np.testing.assert_array_equal(dist[:, :kk], sub_d)
        assert (ids[:, kk:] == -1).all() and np.isinf(dist[:, kk:]).all()


# ------------------------------------------------------------------------------------------------ 3. the masked exact scan
N = 3000


def _exact_tags():
    """bit 0 on about half the rows, bit 1 on about a tenth, bit 2 on exactly 3 rows, bit 3 on none, bit 63 on about 0.05; about
    0.4 of the rows carry no tag at all."""
    rs = np.random.RandomState(5)
    tags = np.zeros(N, U64)
    tags[rs.random_sample(N) < 0.5] |= U64(1)
    tags[rs.random_sample(N) < 0.1] |= U64(2)
    tags[[7, 1500, 2999]] |= U64(4)
    tags[rs.random_sample(N) < 0.05] |= BIT63
    assert (tags == 0).sum() > 100
    return tags


def _exact_masks(nq):
    cycle = np.array([1, 2, 4, 8, int(BIT63), 0, 3, int(BIT63) | 4], U64)
    return cycle[np.arange(nq) % len(cycle)]


def _alt64(metric, x, q):
    """(nq, n) float64 distances in the kernels' space, the conventions of tests/exact_util.py alt_pairs."""
    a, b = q.astype(np.float64), x.astype(np.float64)
    if metric in ("sqeuclidean", "euclidean"):
        return np.stack([((b - row) ** 2).sum(1) for row in a])
    if metric in ("cosine", "correlation"):
        return np.stack([XU.alt_pairs(metric, row[None, :], b[None, :, :])[0] for row in a])
    return BU.dist(metric, q, x)


def _masked_truth(metric, x, q, tags, masks, k):
    """ids by (float64 distance, id) among each query's allowed rows, the distances cast to float32 and corrected as the class
    corrects them; (-1, inf) where the allowed rows run out."""
    alt = _alt64(metric, x, q)
    ids = np.full((len(q), k), -1, np.int32)
    dist = np.full((len(q), k), np.inf, np.float32)
    for i in range(len(q)):
        allowed = np.flatnonzero(TR.allowed_of(tags, masks[i]))
        order = allowed[np.argsort(alt[i, allowed], kind="stable")][:k]
        ids[i, :len(order)] = order
        dist[i, :len(order)] = alt[i, order].astype(np.float32)
    dist = np.asarray(_metric_record(metric).correction(dist))
    return ids, np.where(ids < 0, np.inf, dist)


def _exact_rows(metric, d, seed):
    if metric == "dice":
        pts = BU.random_rows(N + 200, d, seed)
    else:
        pts = clustered(N + 200, d, 6, 12, seed)
        pts[40:44] = pts[40]  # exact duplicates: equal float64 distances, ordered by id
    return np.ascontiguousarray(pts[:N], np.float32), np.ascontiguousarray(pts[N:], np.float32)


def _compare(label, got, want):
    ids, dist = got
    print("%s: %d of %d places filled, %d rows short of k" % (label, int((want[0] >= 0).sum()), want[0].size, int((want[0] < 0).any(1).sum())))
    np.testing.assert_array_equal(np.asarray(ids), want[0], err_msg=label)
    np.testing.assert_array_equal(np.asarray(dist, np.float32).view(np.uint32), np.asarray(want[1], np.float32).view(np.uint32), err_msg=label)


@pytest.mark.parametrize("metric,d,k,nq", [("sqeuclidean", 24, 5, 100), ("sqeuclidean", 130, 70, 200), ("cosine", 130, 5, 200),
                                           ("cosine", 24, 70, 100), ("dice", 130, 70, 100), ("dice", 24, 5, 200),
                                           # the rest of k_exact_scan's masked instances: every row width (d = 24 / 40 / 130: 32, 64 and
                                           # 128 floats staged per chunk) x every family (correlation: the codes 2..5) x both list widths
                                           ("dice", 24, 70, 100), ("dice", 130, 5, 100), ("sqeuclidean", 40, 5, 100), ("cosine", 40, 70, 100),
                                           ("dice", 40, 5, 100), ("dice", 40, 70, 100), ("correlation", 24, 5, 100), ("correlation", 24, 70, 100),
                                           ("correlation", 40, 5, 100), ("correlation", 40, 70, 100), ("correlation", 130, 5, 100),
                                           ("correlation", 130, 70, 100)])
def test_masked_exact_scan(metric, d, k, nq):
    """n = 3000; d = 24, 40 and 130 (more than one K chunk); k = 5 and 70 (the WIDE lists); 100 and 200 queries (no multiple of 64).
    A tag no row has, a tag on exactly 3 rows (fewer than k: padded), rows with tag word 0, queries with mask 0, bit 63."""
    x, q = _exact_rows(metric, d, 3)
    q = q[:nq]
    tags, masks = _exact_tags(), _exact_masks(nq)
    want = _masked_truth(metric, x, q, tags, masks, k)
    assert (want[0][masks == 0] == -1).all() and (want[0][masks == U64(8)] == -1).all()
    assert ((want[0][masks == U64(4)] >= 0).sum(1) == 3).all()
    ids, dist, stats = exact_knn(x, q, k, metric=metric, row_tags=tags, query_tags=masks, return_stats=True)
    print(stats)
    _compare("%s d %d k %d" % (metric, d, k), (ids, dist), want)


def test_masked_exact_scan_where_the_float64_tier_answers():
    """Two far modes of tight points (the bimodal set of tests/test_gpu_exact.py): the certificate fails and the float64 tier
    answers -- under the masks too, with its short rows padded."""
    rs = np.random.RandomState(7)
    x = 0.01 * rs.standard_normal((N, 24))
    x = (x + np.where(rs.rand(N, 1) < 0.5, 1000.0, -1000.0)).astype(np.float32)
    q = np.ascontiguousarray(x[np.sort(np.random.RandomState(1).choice(N, 100, replace=False))] + np.float32(0.001))
    tags, masks = _exact_tags(), _exact_masks(100)
    ids, dist, stats = exact_knn(x, q, 5, metric="sqeuclidean", row_tags=tags, query_tags=masks, return_stats=True)
    print(stats)
    assert stats["n_fallback"] >= 1
    _compare("bimodal", (ids, dist), _masked_truth("sqeuclidean", x, q, tags, masks, 5))


def test_masked_exact_scan_of_the_rows_themselves_and_on_the_device():
    """``queries=None``: the masks belong to the rows (one per row; a row whose tag meets its own mask finds itself first); tensors
    in, tensors out, the same answer."""
    torch = pytest.importorskip("torch")
    x, _ = _exact_rows("sqeuclidean", 24, 3)
    tags = _exact_tags()
    masks = _exact_masks(N)
    want = _masked_truth("sqeuclidean", x, x, tags, masks, 5)
    _compare("rows themselves", exact_knn(x, None, 5, metric="sqeuclidean", row_tags=tags, query_tags=masks), want)
    rows = np.array([2999, 5, 40, 41], np.int64)
    sub = exact_knn(x, None, 5, metric="sqeuclidean", rows=rows, row_tags=tags, query_tags=masks[rows])
    _compare("some rows", sub, _masked_truth("sqeuclidean", x, x[rows], tags, masks[rows], 5))
    dev = torch.device("cuda", 0)
    ids, dist = exact_knn(torch.from_numpy(x).to(dev), None, 5, metric="sqeuclidean", row_tags=torch.from_numpy(tags.view(np.int64)).to(dev),
                          query_tags=masks)  # (tags on the device, masks on the host)
    assert ids.is_cuda and dist.is_cuda
    _compare("device rows", (ids.cpu().numpy(), dist.cpu().numpy()), want)


# ------------------------------------------------------------------------------------------------ 4 - 6. the class
N_IDX, D_IDX, NQ_IDX = 5000, 16, 203


@pytest.fixture(scope="module")
def world():
    pts = clustered(N_IDX + NQ_IDX, D_IDX, 8, 8, seed=11)
    x, q = np.ascontiguousarray(pts[:N_IDX]), np.ascontiguousarray(pts[N_IDX:])
    rs = np.random.RandomState(2)
    tags = np.zeros(N_IDX, U64)
    for bit, sel in ((0, 0.5), (1, 0.1), (2, 0.01), (63, 0.03)):
        tags[rs.random_sample(N_IDX) < sel] |= U64(1) << U64(bit)
    cycle = np.array([1, 2, 4, 8, int(BIT63), 0, 6], U64)  # (8: a tag no row has)
    masks = cycle[np.arange(NQ_IDX) % len(cycle)]
    index = NNDescent(x, n_neighbors=15, random_state=1)
    index.set_row_tags(tags)
    return types.SimpleNamespace(x=x, q=q, tags=tags, masks=masks, index=index)


def test_class_walk_and_exact(world):
    """Forced paths: every id satisfies its query's predicate and is in the original numbering; "exact" is numpy's answer."""
    index = world.index
    ids, dist = index.query(world.q, k=10, query_tags=world.masks, filter_mode="walk")
    n_empty = int((world.masks == 0).sum())
    assert index.last_filter == {"mode": "tags", "n_walk": NQ_IDX - n_empty, "n_exact": 0, "n_empty": n_empty, "n_masks": 7}
    _each_allowed("class walk", ids, world.tags, world.masks)
    assert (ids[(world.masks == 0) | (world.masks == U64(8))] == -1).all() and np.isinf(dist[ids < 0]).all()
    found = ids >= 0
    d2 = ((world.q.astype(np.float64)[:, None, :] - world.x.astype(np.float64)[ids.clip(0)]) ** 2).sum(-1)
    np.testing.assert_allclose(dist[found], np.sqrt(d2[found]), rtol=1e-5, atol=1e-6)
    ids, dist = index.query(world.q, k=10, query_tags=world.masks, filter_mode="exact")
    assert index.last_filter == {"mode": "tags", "n_walk": 0, "n_exact": NQ_IDX - n_empty, "n_empty": n_empty, "n_masks": 7}
    want = _masked_truth("euclidean", world.x, world.q, world.tags, world.masks, 10)
    np.testing.assert_array_equal(ids, want[0])
    np.testing.assert_allclose(dist, want[1], rtol=1e-6)


def test_class_auto_splits_the_call(world, monkeypatch):
    """5000 rows, ``TAG_EXACT_MAX_ROWS`` patched so that the call splits: ``last_filter`` reports the split, and every query's
    answer is that of forcing its path (the walk keeps every query in its place in the batch)."""
    index, masks = world.index, world.masks
    counts = {int(m): int(TR.allowed_of(world.tags, m).sum()) for m in np.unique(masks)}
    monkeypatch.setattr(filtered, "TAG_EXACT_MAX_ROWS", 1000)
    goes_exact = np.array([0 < counts[int(m)] <= 1000 for m in masks])
    is_empty = np.array([counts[int(m)] == 0 for m in masks])
    walks = ~goes_exact & ~is_empty
    assert goes_exact.sum() > 20 and walks.sum() > 20 and is_empty.sum() > 20
    ids, dist = index.query(world.q, k=10, query_tags=masks)
    assert index.last_filter == {"mode": "tags", "n_walk": int(walks.sum()), "n_exact": int(goes_exact.sum()), "n_empty": int(is_empty.sum()),
                                 "n_masks": len(counts)}
    by_walk = index.query(world.q, k=10, query_tags=masks, filter_mode="walk")
    by_exact = index.query(world.q, k=10, query_tags=masks, filter_mode="exact")
    for name, rows, forced in (("walk", walks, by_walk), ("exact", goes_exact, by_exact)):
        np.testing.assert_array_equal(ids[rows], forced[0][rows], err_msg=name)
        np.testing.assert_array_equal(dist[rows], forced[1][rows], err_msg=name)
    assert (ids[is_empty] == -1).all() and np.isinf(dist[is_empty]).all()
    monkeypatch.setattr(filtered, "TAG_COUNT_MAX_MASKS", 3)  # more distinct masks than are counted: every query walks
    ids, dist = index.query(world.q, k=10, query_tags=masks)
    assert index.last_filter["n_exact"] == 0 and index.last_filter["n_walk"] == NQ_IDX - int((masks == 0).sum())
    np.testing.assert_array_equal(ids, by_walk[0])


def test_class_device_route(world):
    """Tags, masks and queries as tensors: tensors back, the host route's answer bit for bit; host tags with device queries and
    device tags with host queries work too."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    index, masks = world.index, world.masks
    q_dev, m_dev = torch.from_numpy(world.q).to(dev), torch.from_numpy(masks.view(np.int64)).to(dev)
    t_dev = torch.from_numpy(world.tags.view(np.int64)).to(dev)
    try:
        for mode in ("walk", "exact", "auto"):
            index.set_row_tags(world.tags)
            want = index.query(world.q, k=10, query_tags=masks, filter_mode=mode)
            record = dict(index.last_filter)
            mixed = index.query(q_dev, k=10, query_tags=masks, filter_mode=mode)  # tags and masks on the host, queries on the device
            index.set_row_tags(t_dev)
            assert index._row_tags is t_dev  # a tensor stays where it is
            for qq, mm in ((q_dev, m_dev), (world.q, m_dev), (q_dev, masks)):
                got = index.query(qq, k=10, query_tags=mm, filter_mode=mode)
                assert index.last_filter == record
                for a in (got, mixed):
                    if isinstance(qq, np.ndarray) and a is got:
                        assert isinstance(a[0], np.ndarray)
                        ids, dist = a
                    else:
                        assert a[0].is_cuda and a[1].is_cuda and a[0].dtype == torch.int32
                        ids, dist = a[0].cpu().numpy(), a[1].cpu().numpy()
                    np.testing.assert_array_equal(ids, want[0], err_msg=mode)
                    np.testing.assert_array_equal(dist.astype(np.float32).view(np.uint32), want[1].astype(np.float32).view(np.uint32), err_msg=mode)
    finally:
        index.set_row_tags(world.tags)


def _exact_misses_nothing(x, q, tags, masks, ids, dist, alt64):
    """Every returned id satisfies its query's predicate, and no allowed row is closer than the k-th returned one and missing."""
    for i in range(len(q)):
        allowed = TR.allowed_of(tags, masks[i])
        got = ids[i][ids[i] >= 0]
        assert allowed[got].all()
        assert len(got) == min(ids.shape[1], int(allowed.sum()))
        if len(got) == ids.shape[1]:
            others = allowed.copy()
            others[got] = False
            assert not others.any() or alt64[i][others].min() >= alt64[i][got].max() * (1 - 1e-12)


def test_quantized_and_sparse_indexes_take_query_tags(world):
    """A uint8-quantized index (the walk on the codes, the rerank in its epilogue) and an index built from scipy.sparse rows,
    queried with a scipy.sparse batch."""
    sp = pytest.importorskip("scipy.sparse")
    n, nq = 3000, 64
    x, q = np.abs(world.x[:n]) + 0.1, np.abs(world.q[:nq]) + 0.1
    tags, masks = world.tags[:n], world.masks[:nq]
    alt64 = _alt64("sqeuclidean", x, q)
    quantized = NNDescent(x, n_neighbors=15, random_state=1, quantization="uint8")
    quantized.set_row_tags(tags)
    for mode in ("walk", "exact"):
        ids, dist = quantized.query(q, k=10, query_tags=masks, filter_mode=mode)
        _each_allowed("quantized " + mode, ids, tags, masks)
        assert np.all(np.diff(np.where(ids >= 0, dist, np.float32(3e38)), axis=1) >= 0)  # (rows ascending, unfilled places last)
    _exact_misses_nothing(x, q, tags, masks, ids, dist, alt64)
    xs = np.where(np.random.RandomState(4).random_sample(x.shape) < 0.5, x, 0.0).astype(np.float32)
    qs = np.where(np.random.RandomState(5).random_sample(q.shape) < 0.5, q, 0.0).astype(np.float32)
    sparse = NNDescent(sp.csr_matrix(xs), n_neighbors=15, random_state=1)
    sparse.set_row_tags(tags)
    alt64 = _alt64("sqeuclidean", xs, qs)
    for mode in ("walk", "exact", "auto"):
        ids, dist = sparse.query(sp.csr_matrix(qs), k=10, query_tags=masks, filter_mode=mode)
        assert isinstance(ids, np.ndarray) and isinstance(dist, np.ndarray)
        _each_allowed("sparse " + mode, ids, tags, masks)
        dense = sparse.query(qs, k=10, query_tags=masks, filter_mode=mode)
        np.testing.assert_array_equal(ids, dense[0])
        if mode == "exact":
            _exact_misses_nothing(xs, qs, tags, masks, ids, dist, alt64)
