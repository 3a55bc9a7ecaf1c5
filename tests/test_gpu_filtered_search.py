"""Filtered queries on the GPU: the Q_FILT_ALLOW instances of k_query (csrc/query.hip) against the filtered step-exact model
(tests/filter_reference.py) through _capi.Searcher, the kernel that builds the allow bitset, and ``NNDescent.query(filter=...)``
with its walk, exact and auto paths.

Step-exact part: every case of tests/search_cases.py the filtered model covers (tests/test_filtered_search_cpu.py asserts
their flagged shares without a GPU), at 0.5 and 0.1 allowed rows, on the automatic tier and again with every query forced to
the global-memory tier.  Unflagged queries must be the model's -- ids and distance bits on the lattice, ids and radius on the
float cases; flagged queries keep the weak checks of tests/test_gpu_search_exact.py; every returned id must be allowed."""
import types

import numpy as np
import pytest

from pynndescent_amd import NNDescent, _capi, filtered, linear_map
from tests import boolean_util as BU
from tests import exact_util as XU
from tests import filter_reference as FR
from tests import proxy_reference as PR
from tests import search_cases as SC
from tests import search_reference as SR
from tests import proxy_util as PU
from tests.test_gpu_search_exact import _case_searcher, _check
from tests.util_data import clustered

pytestmark = pytest.mark.gpu
TIERS = (0, 1)


def _filtered(case, s, mask, tier, queries=None, order=None):
    """One filtered call on the searcher ``s``; the filter is cleared again."""
    queries = case.queries if queries is None else queries
    s.set_tier(tier)
    n_allowed = s.set_filter(mask, order)
    try:
        if getattr(case, "values", None) is not None:
            ids, dist = s.query_proxy(queries, case.k, case.search_k, case.epsilon)
        else:
            ids, dist = s.query(queries, case.k, case.epsilon)
        return ids, dist, s.last_spilled(), n_allowed
    finally:
        s.clear_filter()
        s.set_tier(0)


def _all_allowed(label, ids, mask):
    found = ids >= 0
    assert mask[ids[found]].all(), "%s: %d returned ids are not allowed" % (label, int((~mask[ids[found]]).sum()))


def _run_case(name, frac, tier):
    case, mask, res = FR.get(name, frac)
    s = _case_searcher(case)
    try:
        ids, dist, spilled, n_allowed = _filtered(case, s, mask, tier)
    finally:
        s.close()
    label = "%s at %g tier %d" % (name, frac, tier)
    print("%s: %d of %d rows allowed, %d of %d queries ran on the global-memory tier, %.1f of %d places filled" % (
        label, n_allowed, len(mask), spilled, len(res), (ids >= 0).sum(1).mean(), case.k))
    assert n_allowed == int(mask.sum())
    assert spilled == len(res) if tier == 1 else spilled <= len(res)
    _all_allowed(label, ids, mask)
    _check(label, case, res, case.queries, ids, dist, case.exact)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("frac", FR.FRACTIONS)
@pytest.mark.parametrize("name", FR.lattice_names())
def test_lattice_case(name, frac, tier):
    """One, two and four result entries per lane (width_k63 .. k256), lists that never fill (the islands), every graph and tree
    shape of the unfiltered suite, 40 .. 6000 rows."""
    _run_case(name, frac, tier)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("frac", FR.FRACTIONS)
@pytest.mark.parametrize("name", sorted(SC.Q8))
def test_uint8_walk(name, frac, tier):
    """The walk on the codes keeps search_k ALLOWED results; the rerank epilogue is the unfiltered one."""
    _run_case(name, frac, tier)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", sorted(SC.FLOAT))
def test_float_case(name, tier):
    """All six float metrics (at 0.5: at 0.1 the model flags up to two thirds of a float case's queries)."""
    _run_case(name, 0.5, tier)


@pytest.mark.parametrize("tier", TIERS)
def test_routing_small(tier):
    """20 000 rows at 0.1: a search that stayed in LDS unfiltered visits up to 13 642 vertices and is handed to the
    global-memory tier, whose answer is the model's too."""
    _run_case("routing_small", 0.1, tier)


# ------------------------------------------------------------------------------------------------ the rerank form (code 6)
def _proxy_model(case, mask, lattice):
    dist = PR._ProxyDistances(case.data, lattice)
    walk = FR._FilteredWalk(mask, case.data.shape[0], np.asarray(case.indptr, np.int64), np.asarray(case.indices, np.int64), case.tree, dist,
                            case.min_distance, int(case.n_neighbors), int(case.search_k), case.epsilon, SR.searcher_seed(case.rng_state), False)
    out = []
    for qi, q in enumerate(case.queries):
        walk.k = int(case.search_k)
        walk.run(qi, q)
        out.append(walk.finish(int(case.k)))
    return out


def _check_rerank(label, case, res, ids, dist, exact):
    """tests/test_gpu_proxy_search.py's rule, for lists that need not fill (200 allowed rows hold fewer than 50 reachable ones):
    every row sorted, unique, filled from the front and every distance -<q, x> of its id; an unflagged query has the model's
    ids, the model's unfilled places, and distances within the radius (the model's bits on the lattice)."""
    bad, n_exact = [], 0
    for i, r in enumerate(res):
        gi, gd = ids[i], dist[i].astype(np.float64)
        found = gi >= 0
        mid, rad = PU.neg_inner(case.queries[i], case.data[gi[found]])
        if not (np.all(np.diff(gd[found]) >= 0) and np.all(found[:found.sum()]) and len(set(gi[found].tolist())) == found.sum()
                and np.all(np.abs(gd[found] - mid) <= rad) and np.all(np.isposinf(gd[~found]))):
            bad.append("query %d: row not sorted / unique, or a distance is not -<q, x> of its id: %s" % (i, gi[:8].tolist()))
        if r.ambiguous:
            continue
        n_exact += 1
        if not np.array_equal(gi, r.ids):
            bad.append("query %d: ids differ from position %d: gpu %s model %s" % (i, int(np.argmax(gi != r.ids)), gi[:12].tolist(), r.ids[:12].tolist()))
        elif exact and not np.array_equal(gd, r.dists):
            bad.append("query %d: distances differ: gpu %s model %s" % (i, gd[:6].tolist(), r.dists[:6].tolist()))
        elif not np.all(np.abs(gd[found] - r.dists[found]) <= r.radius[found]):
            bad.append("query %d: distances outside the radius" % i)
    print("%s: %d queries compared entry for entry, %d left to the weak checks, %d mismatching" % (label, n_exact, len(res) - n_exact, len(bad)))
    assert not bad, "%s: %d problems\n%s" % (label, len(bad), "\n".join(bad[:8]))


@pytest.mark.parametrize("frac", FR.FRACTIONS)
@pytest.mark.parametrize("which", ["lattice", (24, 30, 120), (17, 50, 200)], ids=["lattice_sk30", "d24_sk120", "d17_sk200"])
def test_proxy_inner_product_rerank(which, frac):
    """metric code 6: the float walk by the proxy distance keeps search_k allowed results (30, 120, 200: one, two and four
    entries per lane), the rerank by -<q, x> returns k; 400 and 2000 rows, both tiers, against the filtered model."""
    lattice = which == "lattice"
    case, _ = PR.lattice_case() if lattice else PR.search_case(*which)
    n = case.data.shape[0]
    mask = FR.case_mask(n, frac)
    res = _proxy_model(case, mask, lattice)
    flagged = np.mean([r.ambiguous for r in res])
    print("%s at %g: the model flags %.2f of the queries" % (case.name, frac, flagged))
    assert flagged <= FR.FLOAT_CAP
    graph = types.SimpleNamespace(indptr=case.indptr, indices=case.indices)
    s = _capi.Searcher(case.data, graph, case.tree, 6, case.min_distance, case.n_neighbors, case.rng_state)
    try:
        for tier in TIERS:
            s.set_tier(tier)
            assert s.set_filter(mask) == int(mask.sum())
            ids, dist = s.query_rerank(case.queries, case.k, case.search_k, case.epsilon)
            s.clear_filter()
            assert tier == 0 or s.last_spilled() == len(res)
            _all_allowed(case.name, ids, mask)
            _check_rerank("%s at %g tier %d" % (case.name, frac, tier), case, res, ids, dist, exact=lattice)
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ the boolean family
def _bool_case(metric="dice", n=1500, d=133, nq=30):
    pts = BU.random_rows(n + nq, d, 5)
    x, q = np.ascontiguousarray(pts[:n]), np.ascontiguousarray(pts[n:])
    dm = BU.dist(metric, x, x)
    rows = SC.symmetric_rows(SC.top_neighbours(-dm, 15))
    indptr, indices = SC.csr_from_rows(rows)
    # min_distance 0: the bound worst + epsilon * (worst - min_distance) is then far above every distance at epsilon 1e6
    return types.SimpleNamespace(metric=metric, data=x, queries=q, indptr=indptr, indices=indices, tree=SC.kd_tree(x, 30),
                                 min_distance=0.0, n_neighbors=15, rng_state=SC.RNG_STATE, values=None)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("k", [10, 100, 129])
def test_boolean_family_walk(k, tier):
    """k_query's boolean form under an allow set (dice, 1500 x 133; k = 10 / 100 / 129: one, two and four result entries per lane).  The family is full of exact ties, which a step-exact model leaves to the weak
    checks query after query, so the rule is checked where it has one answer: with a bound that never closes (epsilon 1e6) the
    walk visits the whole connected graph, and then the returned distances ARE the k smallest over the allowed rows, bit for
    bit (the ids among equal distances are the walk's choice).  With the usual epsilon: every id allowed, rows sorted and
    unique, every distance the float32 value of its pair."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components

    case = _bool_case()
    n = case.data.shape[0]
    adj = sp.csr_array((np.ones(len(case.indices), np.int8), case.indices, case.indptr), shape=(n, n))
    assert connected_components(adj, directed=True, connection="strong")[0] == 1
    want = BU.dist(case.metric, case.queries, case.data, f32=True).astype(np.float32)
    graph = types.SimpleNamespace(indptr=case.indptr, indices=case.indices)
    s = _capi.Searcher(case.data, graph, case.tree, BU.CODES[case.metric], case.min_distance, case.n_neighbors, case.rng_state)
    try:
        for frac in FR.FRACTIONS:
            mask = FR.case_mask(n, frac)
            assert mask.sum() >= k
            for eps in (1e6, 0.125):
                case.k, case.epsilon = k, eps
                ids, dist, spilled, _ = _filtered(case, s, mask, tier)
                label = "dice k %d at %g, epsilon %g, tier %d" % (k, frac, eps, tier)
                _all_allowed(label, ids, mask)
                found = ids >= 0
                for i in range(len(ids)):
                    gi, gd = ids[i][found[i]], dist[i][found[i]]
                    assert found[i][:found[i].sum()].all() and len(set(gi.tolist())) == len(gi) and np.all(np.diff(gd) >= 0), label
                    assert np.array_equal(gd.view(np.uint32), want[i, gi].view(np.uint32)), label
                if eps == 1e6:
                    best = np.sort(np.where(mask[None, :], want, np.inf), axis=1)[:, :k]
                    assert found.all() and np.array_equal(dist.view(np.uint32), best.view(np.uint32)), label
                    print("%s: the k smallest allowed distances, bit for bit; %d of %d queries on the global-memory tier" % (
                        label, spilled, len(ids)))
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ equivalences
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", ["width_k10_nn10", "width_k129_nn30", "width_k256_nn10", "graph_islands_k200", "q8_d13_sk64",
                                  "float_cosine_d12", "tree_tiny_leaves_repeated_draws"])
def test_all_true_filter_is_the_unfiltered_call(name, tier):
    """Bit-identical output of the filtered and the unfiltered instance on the same searcher when every row is allowed."""
    case, _ = SC.get(name)
    n = case.data.shape[0]
    s = _case_searcher(case)
    try:
        s.set_tier(tier)
        plain = s.query_proxy(case.queries, case.k, case.search_k, case.epsilon) if case.values is not None else s.query(case.queries, case.k, case.epsilon)
        for everything in (np.ones(n, bool), np.arange(n)):
            ids, dist, _, n_allowed = _filtered(case, s, everything, tier)
            assert n_allowed == n
            np.testing.assert_array_equal(ids, plain[0])
            np.testing.assert_array_equal(dist.view(np.uint32), plain[1].view(np.uint32))
    finally:
        s.close()


@pytest.mark.parametrize("name", ["tree_tiny_leaves_repeated_draws", "tree_single_leaf", "width_k10_nn10", "dim_17"])
def test_bitset_goes_through_the_row_order(name):
    """n = 40, 150, 500, 3000 (whole and partial words and waves): a mask or an id list in the ORIGINAL numbering, gathered by
    the searcher's row order, sets the bits a mask in the searcher's numbering sets; the count is the number of allowed rows;
    an out-of-range id is a ValueError that leaves the searcher unfiltered."""
    case, mask, _ = FR.get(name, 0.5)
    n = case.data.shape[0]
    order = np.random.RandomState(3).permutation(n).astype(np.int32)  # searcher row i is original row order[i]
    original = np.zeros(n, bool)
    original[order] = mask
    ids_list = np.flatnonzero(original)
    s = _case_searcher(case)
    try:
        want = _filtered(case, s, mask, 0)
        assert want[3] == int(mask.sum())
        for form in (original, original.view(np.uint8), ids_list, ids_list[::-1].astype(np.int32), np.concatenate([ids_list, ids_list[:5]])):
            got = _filtered(case, s, form, 0, order=order)
            assert got[3] == want[3]
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        plain = s.query(case.queries, case.k, case.epsilon)
        for bad in ([0, n], [-1], [3, 2 ** 40]):
            with pytest.raises(ValueError, match="outside 0"):
                s.set_filter(np.array(bad, np.int64), order)
            after = s.query(case.queries, case.k, case.epsilon)  # no filter is set
            np.testing.assert_array_equal(after[0], plain[0])
    finally:
        s.close()


# ------------------------------------------------------------------------------------------------ the class
N, D, K, NQ = 3000, 16, 15, 200
SELECTIVITIES = (0.5, 0.1, 0.02)
# The recall comparison holds the filtered walk against the unfiltered one on the same graph, so both must be asked the same kind
# of question: neighbours inside the query's own cluster.  A k-NN graph of well separated clusters has next to no edges between
# them, and whatever lies in another cluster is out of reach of ANY walk that starts in this one.  The clusters are therefore
# large enough that the 10 nearest allowed rows lie in the query's cluster down to selectivity 0.1 (8 clusters of about 375 rows:
# about 37 allowed rows each, more than three times k); at 0.02 (about 7 allowed rows per cluster) they cannot, which is the
# case "fewer than k rows reachable" below.  (With 32 clusters of about 94 rows, 9 allowed rows per cluster at 0.1, the first
# run of this test measured: unfiltered 0.98900, filtered 0.99250 at 0.5, 0.97950 at 0.1, 0.91693 of the filled places at 0.02.)
N_CLUSTERS = 8


@pytest.fixture(scope="module")
def world():
    pts = clustered(N + NQ, D, 8, N_CLUSTERS, seed=11)
    x, q = np.ascontiguousarray(pts[:N]), np.ascontiguousarray(pts[N:])
    d2 = ((q.astype(np.float64)[:, None, :] - x.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    indexes = [NNDescent(x, n_neighbors=K, random_state=rs) for rs in (1, 2, 3)]
    recalls = []
    truth = np.argsort(d2, axis=1, kind="stable")[:, :10]
    for index in indexes:
        ids, _ = index.query(q, k=10, epsilon=0.1)
        recalls.append(np.mean([len(set(a) & set(b)) for a, b in zip(ids.tolist(), truth.tolist())]) / 10.0)
    margin = 2.0 * (max(recalls) - min(recalls))
    print("unfiltered recall@10 over three random_states: %s; margin (twice the spread) %.5f" % (["%.5f" % r for r in recalls], margin))
    return types.SimpleNamespace(x=x, q=q, d2=d2, index=indexes[0], recall=recalls[0], margin=margin)


def _mask(sel):
    return np.random.RandomState(7).random_sample(N) < sel


@pytest.mark.parametrize("sel", SELECTIVITIES)
def test_class_walk(world, sel):
    """``query(filter=mask, filter_mode="walk")`` on 3000 x 16 clustered rows: ids allowed and in the original numbering,
    distances those of the ids, recall@10 against float64 brute force over the allowed rows not below the index's unfiltered
    recall minus twice the spread of that recall over three random_states.  At 0.02 only filled places count, and the model --
    run on the index's own prepared arrays -- says that no allowed row nearer than the last returned one was seen and dropped."""
    index, mask = world.index, _mask(sel)
    ids, dist = index.query(world.q, k=10, epsilon=0.1, filter=mask, filter_mode="walk")
    assert index.last_filter == {"mode": "walk", "n_allowed": int(mask.sum())}
    assert ids.shape == dist.shape == (NQ, 10) and ids.dtype == np.int32
    found = ids >= 0
    assert mask[ids[found]].all() and ids.max() < N
    rows = np.broadcast_to(np.arange(NQ)[:, None], ids.shape)
    np.testing.assert_allclose(dist[found], np.sqrt(world.d2[rows[found], ids[found]]), rtol=1e-5, atol=1e-6)
    assert np.isinf(dist[~found]).all()
    if sel == 0.02:
        _model_agrees_on_the_class_index(index, mask, world.q, ids)
    else:
        assert found.all()
    truth = np.argsort(np.where(mask[None, :], world.d2, np.inf), axis=1, kind="stable")[:, :10]
    hits = sum(len(set(a[a >= 0].tolist()) & set(b.tolist())) for a, b in zip(ids, truth))
    places = int(found.sum()) if sel == 0.02 else NQ * 10
    recall = hits / float(places)
    print("selectivity %g: %d rows allowed, %.2f of 10 places filled, recall@10 %.5f (unfiltered %.5f, margin %.5f)" % (
        sel, mask.sum(), found.sum(1).mean(), recall, world.recall, world.margin))
    assert recall >= world.recall - world.margin


def _model_agrees_on_the_class_index(index, mask, q, ids):
    """The filtered model on the index's prepared arrays (searcher numbering: row i is original row _vertex_order[i]): no allowed
    row nearer than the last returned one was seen and dropped, a list is short only when the walk saw fewer than k allowed
    rows, and the unflagged queries' answers are the class's, id for id."""
    order = np.asarray(index._vertex_order)
    sg = index._search_graph
    res = FR.reference_search(mask[order], index._raw_data, sg.indptr, sg.indices, index._search_forest[0], "euclidean", index._min_distance,
                              index.n_neighbors, q, 10, 0.1, index.search_rng_state, trace=True)
    compared = 0
    for i, r in enumerate(res):
        t, m = r.trace, int((r.ids >= 0).sum())
        assert m == min(10, len(t["seen_ids"]))
        if m:  # every allowed vertex seen nearer than the last returned one is in the answer
            nearer = t["seen_ids"][t["seen_mid"] < r.dists[m - 1]]
            assert set(nearer.tolist()) <= set(r.ids[:m].tolist())
        if r.ambiguous:
            continue
        compared += 1
        np.testing.assert_array_equal(ids[i], np.where(r.ids >= 0, order[np.maximum(r.ids, 0)], -1))
    print("%d of %d queries equal the model's answer id for id" % (compared, len(res)))
    assert compared >= len(res) // 2


def test_class_filter_forms_agree(world):
    """Bool mask, id list, numpy and tensor, host and device queries: one filter, one answer."""
    torch = pytest.importorskip("torch")
    index, mask = world.index, _mask(0.1)
    ids_list = np.flatnonzero(mask)
    want = index.query(world.q, k=10, filter=mask, filter_mode="walk")
    dev = torch.device("cuda", 0)
    for form in (ids_list, ids_list.astype(np.int32), ids_list.tolist(), torch.from_numpy(mask).to(dev), torch.from_numpy(ids_list).to(dev),
                 torch.from_numpy(ids_list.astype(np.int32)).to(dev)):
        got = index.query(world.q, k=10, filter=form, filter_mode="walk")
        assert isinstance(got[0], np.ndarray) and index.last_filter == {"mode": "walk", "n_allowed": int(mask.sum())}
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
    q_dev = torch.from_numpy(world.q).to(dev)
    for form in (mask, torch.from_numpy(mask).to(dev), torch.from_numpy(ids_list).to(dev)):  # a host filter with device queries too
        got = index.query(q_dev, k=10, filter=form, filter_mode="walk")
        assert got[0].is_cuda and got[1].is_cuda and got[0].dtype == torch.int32
        np.testing.assert_array_equal(got[0].cpu().numpy(), want[0])
        np.testing.assert_allclose(got[1].cpu().numpy(), want[1], rtol=1e-6)
    unfiltered = index.query(world.q, k=10)  # the filter does not outlive its call
    np.testing.assert_array_equal(unfiltered[0], world.index.query(world.q, k=10, filter=np.ones(N, bool), filter_mode="walk")[0])
    with pytest.raises(ValueError, match="outside 0"):
        index.query(world.q, k=10, filter=torch.tensor([0, N], device=dev))
    ids, dist = index.query(q_dev, k=10, filter=torch.zeros(N, dtype=torch.bool, device=dev))
    assert ids.is_cuda and bool((ids == -1).all()) and bool(torch.isinf(dist).all()) and index.last_filter["mode"] == "empty"


def _transformed(metric, kwds, train, *others):
    lin = linear_map.parse_metric_kwds(metric, kwds, train.shape[1])
    lin = lin._replace(shift=linear_map.shift_of(train))
    return [_capi.linear_rows_host(lin.kind, lin.a, lin.shift, np.ascontiguousarray(r, np.float32)) for r in (train,) + others]


@pytest.mark.parametrize("metric", ["euclidean", "cosine", "seuclidean"])
def test_class_exact_path(world, metric):
    """``filter_mode="exact"``: the ids are numpy's by (float64 distance, id) over the allowed rows, under the comparison rule of
    the exact search's own tests (tests/exact_util.py); seuclidean: on the float32 transformed rows.  Fewer allowed rows than k
    leave (-1, inf); device queries get device answers; the device-built index gathers from its tensor."""
    torch = pytest.importorskip("torch")
    x, q = world.x, world.q
    kwds = {"V": x.astype(np.float64).var(0)} if metric == "seuclidean" else None
    index = world.index if metric == "euclidean" else NNDescent(x, metric=metric, metric_kwds=kwds, n_neighbors=K, random_state=1)
    on_device = NNDescent(torch.from_numpy(x).cuda(), metric=metric, metric_kwds=kwds, n_neighbors=K, random_state=1)
    rows, queries = _transformed(metric, kwds, x, q) if metric == "seuclidean" else (x, q)
    rule = "cosine" if metric == "cosine" else "euclidean"
    for sel in (0.1, 0.02):
        mask = _mask(sel)
        allowed = np.flatnonzero(mask)
        truth = XU.matrix_truth(rule, rows[allowed], queries, 10)
        for idx_obj, qq, flt in ((index, q, mask), (index, torch.from_numpy(q).cuda(), allowed), (on_device, q, torch.from_numpy(mask).cuda()),
                                 (on_device, torch.from_numpy(q).cuda(), mask)):
            ids, dist = idx_obj.query(qq, k=10, filter=flt, filter_mode="exact")
            assert idx_obj.last_filter == {"mode": "exact", "n_allowed": len(allowed)}
            if not isinstance(qq, np.ndarray):
                assert ids.is_cuda and dist.is_cuda
                ids, dist = ids.cpu().numpy(), dist.cpu().numpy()
            assert isinstance(ids, np.ndarray) and ids.dtype == np.int32 and mask[ids].all()
            d64 = dist.astype(np.float64)
            alt = -np.log2(np.maximum(1.0 - d64, 1e-300)) if metric == "cosine" else d64 ** 2
            XU.check_exact("%s exact at %g" % (metric, sel), rule, rows[allowed], queries, np.searchsorted(allowed, ids), alt, truth, 10)
    few = np.array([5, 17, 2999, 17])
    ids, dist = index.query(q, k=10, filter=few, filter_mode="exact")
    assert index.last_filter == {"mode": "exact", "n_allowed": 3}
    assert (np.sort(ids[:, :3], axis=1) == np.array([5, 17, 2999])).all() and (ids[:, 3:] == -1).all() and np.isinf(dist[:, 3:]).all()
    assert np.all(np.diff(dist[:, :3], axis=1) >= 0)


def test_class_auto_path(world, monkeypatch):
    """0.02 of 3000 rows are 61 allowed rows: ``auto`` takes the exact path with the constant above that, the walk with it at 0."""
    index, mask = world.index, _mask(0.02)
    assert 40 < mask.sum() <= 80
    monkeypatch.setattr(filtered, "FILTER_EXACT_MAX_ROWS", 100)
    exact = index.query(world.q, k=10, filter=mask)
    assert index.last_filter == {"mode": "exact", "n_allowed": int(mask.sum())}
    np.testing.assert_array_equal(exact[0], index.query(world.q, k=10, filter=mask, filter_mode="exact")[0])
    monkeypatch.setattr(filtered, "FILTER_EXACT_MAX_ROWS", 0)
    walk = index.query(world.q, k=10, filter=mask)
    assert index.last_filter == {"mode": "walk", "n_allowed": int(mask.sum())}
    np.testing.assert_array_equal(walk[0], index.query(world.q, k=10, filter=mask, filter_mode="walk")[0])
    assert (exact[0] >= 0).all() and mask[exact[0]].all()


def test_quantized_and_proxy_indexes_take_a_filter(world):
    """The class reaches the uint8 and the rerank instances: every id allowed, k of search_k allowed candidates returned."""
    mask = _mask(0.5)
    x = np.abs(world.x) + 0.1
    assert mask.sum() <= filtered.FILTER_EXACT_MAX_ROWS
    for kwargs, auto in (({"metric": "euclidean", "quantization": "uint8"}, "exact"), ({"metric": "proxy_inner_product"}, "walk")):
        index = NNDescent(x, n_neighbors=K, random_state=1, **kwargs)
        ids, dist = index.query(np.abs(world.q) + 0.1, k=10, filter=mask)
        assert index.last_filter["mode"] == auto  # (the proxy metric has no exact search)
        assert (ids >= 0).all() and mask[ids].all() and np.all(np.diff(dist, axis=1) >= 0)
        ids, dist = index.query(np.abs(world.q) + 0.1, k=10, filter=mask, filter_mode="walk")
        assert (ids >= 0).all() and mask[ids].all() and np.all(np.diff(dist, axis=1) >= 0)
