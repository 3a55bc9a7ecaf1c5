"""dot / inner_product / correlation / hellinger (codes 2..5) on every kernel instance that serves them, on a real MI355X,
against float64 truth and the CPU oracle (the reference algorithm, pinned by tests/test_oracle_metrics_cpu.py).

Which instance a case selects (parameter ids name it).  dp = d rounded up to 32 (csrc/plan.h nnd_make_plan); ks = k rounded
up to 16; the padded max_candidates mcp is 16 / 32 / 64 / 128 (the same function: 32 at least when ks > 64).
  prep.hip nnd_prep_rows:        d % 4 != 0 -> k_prep_rows (scalar); else k_prep_rows_v4, lpr = the power of two >= dp/4
                                 (max 64): d 4 -> 1 .. d 256 / 260 -> 64
  join.hip launch_join_xm:       mcp 16 -> k_local_join16 (DC 32 at dp < 128, 64 at dp >= 128); mcp 32 -> k_local_join_w<32>
                                 (DC by the same dp rule), its neighbour lists staged in LDS when ks <= 32 on one GPU, from
                                 global memory with NND_FLAG_TEST_JOIN_UNSTAGED; mcp 64 -> k_local_join_w<64>;
                                 mcp 128 -> launch_join_blocked (five passes of the 64-slot kernel)
  leaf_join.hip run_leaf_rounds (the table of leaf_plan.h): k > 64 -> k_leaf_join_rb<*, 8, true>; k 17..32 and leaves <= 160 -> k_leaf_join_sym;
                                 k <= 16 -> k_leaf_join<.., true> up to 96 points; leaves of 97.. points -> k_leaf_join_rb<8..16, 8>
  finalize.hip nnd_launch_finalize: k > 64 -> k_finalize_wide<NND_CODES_ANY>; else k_finalize<M> (float4 loads when d % 4 == 0,
                                 scalar loads otherwise)
  prune.hip:                     k > 64 -> k_diversify_rows_wide / k_diversify_csr_wide (AWARE for degree_aware)
  query.hip (k_query):           query k <= 64 -> KU 1, <= 128 -> KU 2, else KU 4; set_tier(1): the global-memory tier
"""
import numpy as np
import pytest
from sklearn.preprocessing import normalize

import pynndescent_amd
from oracle import oracle as O
from pynndescent_amd import NNDescent, _capi
from pynndescent_amd.search_graph import build_search_graph
from tests import metric_util as MU
from tests.gpu_util import alt_dist_matrix, check_graph_invariants, make_builder, self_dist, tight_atol
from tests.test_gpu_metrics import _seam_data
from tests.util_data import clustered

pytestmark = pytest.mark.gpu

METRICS = MU.NEW_METRICS
ND_DIST = {"dot": "alternative_dot", "inner_product": "alternative_inner_product", "correlation": "correlation",
           "hellinger": "alternative_hellinger"}
_BUILT = {}


def _data(metric, n, d, seed):
    """clustered rows in the space NNDescent hands to the build: normalised for dot, non-negative for hellinger, shifted for
    inner product (mostly positive products); a zero row for dot / correlation / hellinger, a constant row for correlation."""
    x = clustered(n, d, min(8, d), 30, seed, nonneg=metric == "hellinger")
    if metric == "inner_product":
        x = x + np.float32(0.5)
    if metric in ("dot", "correlation", "hellinger"):
        x[[7, n // 2]] = 0.0
    if metric == "correlation":
        x[[11]] = np.float32(0.3)
    if metric == "dot":
        x = normalize(x, norm="l2")
    return np.ascontiguousarray(x, np.float32)


def _truth_rows(metric, x, rows, k=10):
    """exact top-k ids of the given rows by the float64 alt distance (self included by the self rule)."""
    dm = MU.alt_dist(metric, x[rows], x)
    dm[np.arange(len(rows)), rows] = self_dist(metric, x[rows])
    return np.argsort(dm, axis=1, kind="stable")[:, :k]


# ---------------------------------------------------------------------------------------------------------- prep + Gram
def _edge_rows(metric, d):
    rs = np.random.RandomState(d)
    x = np.zeros((300, d), np.float32)
    if d >= 40:
        x[:, :40] = _seam_data(metric)
        x[:, 40:] = _seam_data(metric)[:, rs.randint(0, 40, d - 40)] * np.float32(0.5)
    else:
        x[:] = _seam_data(metric)[:, :d]
    if metric == "correlation":  # a large common offset: the row mean must come off in float64
        x[200:260] = (1e3 + rs.standard_normal((60, d)) * 1e-2).astype(np.float32)
    if metric == "hellinger":  # values over 24 decades
        x[200:260] = (10.0 ** rs.uniform(-12, 12, (60, d))).astype(np.float32)
    if metric == "dot":
        x = normalize(x, norm="l2").astype(np.float32)
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("d", [1, 3, 4, 5, 17, 36, 64, 127, 128, 130, 256, 260],
                         ids=lambda d: "d%d-%s" % (d, "scalar" if d % 4 else "v4lpr%d" % min(64, 1 << max(0, int(np.ceil(np.log2(max(1, ((d + 31) & ~31) // 4))))))))
@pytest.mark.parametrize("metric", METRICS)
def test_prep_and_gram_at_dimension_edges(metric, d):
    """nnd_pairwise_gram after the prep kernel that d selects, against float64 alt_dist: special rows of _seam_data,
    correlation rows on a large offset, hellinger rows spanning 1e-12..1e12, and d = 1."""
    x = _edge_rows(metric, d)
    b = make_builder(x, metric, k=10, n_trees=0)
    try:
        special = [17, 20, 21, 23, 30, 40, 41]
        rows_a = np.concatenate([special, np.arange(100, 130), np.arange(200, 230)]).astype(np.int32)
        rows_b = np.concatenate([special, np.arange(110, 140), np.arange(215, 245), [17, 40]]).astype(np.int32)
        got = b.pairwise_gram(rows_a, rows_b).astype(np.float64)
    finally:
        b.close()
    want = alt_dist_matrix(x, rows_a, rows_b, metric)
    big = want >= MU.FLT_MAX
    assert np.array_equal(got >= MU.FLT_MAX, big), np.argwhere((got >= MU.FLT_MAX) != big)[:5]
    assert (got >= 0.0).all()
    cos = MU.abs_cos(metric, x[rows_a], x[rows_b])
    good = ~big & ~(cos < 0.05)
    np.testing.assert_allclose(got[good], want[good], rtol=1e-5, atol=tight_atol(d))
    np.testing.assert_allclose(got[~big], want[~big], rtol=2e-4, atol=1e-5)
    if d == 1 and metric == "correlation":  # every row is constant: every pair is 0
        assert (got == 0.0).all()
    if d == 1 and metric in ("dot", "hellinger"):  # one-entry unit rows: 0 (within the float32 rounding of 1) or FLT_MAX
        assert ((got <= 1e-6) | big).all()


# ------------------------------------------------------------------------------------------------- step-level exactness
# id -> (k, max_candidates, d, leaf_size, flags)
STEP_CASES = {
    "join16-dc32-leafjoin": (10, 10, 24, None, 0),
    "join16-dc64-leafjoin": (10, 10, 130, None, 0),
    "joinw32-staged-dc32-sym": (20, 20, 24, None, 0),
    "joinw32-staged-dcw-sym": (24, 24, 128, None, 0),
    "joinw32-unstaged-dc32": (20, 20, 24, None, _capi.NND_FLAG_TEST_JOIN_UNSTAGED),
    "joinw32-unstaged-dcw": (24, 24, 128, None, _capi.NND_FLAG_TEST_JOIN_UNSTAGED),
    "joinw64-finscalar": (40, 50, 17, None, 0),
    "blocked128": (60, 100, 20, None, 0),
    "leafrb-large-leaves": (12, 12, 24, 120, 0),
    "wide-k100-rbwide-finwide": (100, 60, 24, None, 0),
}


@pytest.mark.parametrize("case", list(STEP_CASES))
@pytest.mark.parametrize("metric", METRICS)
def test_steps_exact(metric, case):
    k, mc, d, leaf, flags = STEP_CASES[case]
    n = 2500
    x = _data(metric, n, d, seed=31)
    b = make_builder(x, metric, k=k, n_trees=3, leaf_size=leaf, mc=mc, flags=flags)
    try:
        b.make_forest()
        la = b.leaf_array()
        b.init_from_leaves()
        idx, dist, _ = b.graph()
        check_graph_invariants(x, metric, idx, dist, name="%s %s leaf init" % (metric, case))
        mates = [set() for _ in range(n)]
        for row in la:
            m = row[row >= 0]
            for p in m:
                mates[p].update(m.tolist())
        for p in range(0, n, 13):  # the exact top-k of the leaf-mates, self excluded (pynndescent_.py:97 starts at i + 1)
            cand = np.array(sorted(mates[p] - {p}))
            dd = alt_dist_matrix(x, [p], cand, metric)[0]
            kk = min(k, len(cand))
            kth = np.sort(dd)[kk - 1]
            got = idx[p][idx[p] >= 0]
            assert len(got) == kk and p not in got, (p, len(got), kk)
            gd = alt_dist_matrix(x, [p], got, metric)[0]
            assert np.all(gd <= kth * (1 + 1e-4) + 1e-6), (p, gd.max(), kth)
        rows = np.arange(0, n, 5)
        truth = _truth_rows(metric, x, rows)
        rec = [MU.recall(truth, idx[rows])]
        for it in range(3):
            b.descent_iter()
            idx, dist, _ = b.graph()
            check_graph_invariants(x, metric, idx, dist, name="%s %s iteration %d" % (metric, case, it))
            rec.append(MU.recall(truth, idx[rows]))
            assert rec[-1] >= rec[-2] - 1e-9, rec
        fi, fd = b.finalize()
    finally:
        b.close()
    valid = fi >= 0
    assert valid.mean() > 0.99
    true = MU.alt_dist_pairs(metric, x[:, None, :], x[np.where(valid, fi, 0)])[0]
    true = np.where(fi == np.arange(n)[:, None], self_dist(metric, x)[:, None], true)
    assert np.array_equal(fd[valid] >= MU.FLT_MAX, true[valid] >= MU.FLT_MAX)
    np.testing.assert_allclose(MU.correct(metric, fd[valid]), MU.correct(metric, true[valid]), rtol=2e-4, atol=1e-6)
    key = np.where(valid, fd.astype(np.float64), np.inf)
    same = np.diff(key, axis=1) == 0
    assert (np.diff(key, axis=1) >= 0).all() and (np.diff(fi, axis=1)[same & valid[:, 1:]] > 0).all(), "rows by (distance, id)"
    print("%s %s: recall@10 leaf init %.4f -> %s" % (metric, case, rec[0], " ".join("%.4f" % r for r in rec[1:])))


# ------------------------------------------------------------------------------------------------------ descent parity
@pytest.mark.parametrize("k", [15, 30, 100])
@pytest.mark.parametrize("metric", METRICS)
def test_nn_descent_parity_on_the_oracle_leaves(metric, k):
    """pynndescent_amd.nn_descent against the oracle's nn_descent from the same (oracle-made) leaf array: the trees are out
    of the comparison, so the band isolates the descent kernels."""
    n = 12_000 if k < 100 else 6000
    x = _data(metric, n, 24, seed=41)
    rng_state, _, ts = O.draw_rng_states(11, 4)
    la = O.make_leaf_array(x, 4, O.default_leaf_size(k), ts, O.ANGULAR[metric])
    n_iters = O.default_n_iters(n)
    mc = min(60, k)
    gi, _ = pynndescent_amd.nn_descent(x, k, rng_state.copy(), max_candidates=mc, dist=ND_DIST[metric], n_iters=n_iters,
                                       delta=0.001, rp_tree_init=True, leaf_array=la)
    oi, _ = O.nn_descent(x, k, rng_state.copy(), mc, metric, n_iters, 0.001, la, lib=O.load("fast"))
    ti, _ = O.brute_force_knn(x, 10, metric)  # every row: a 1000-row sample alone moves recall by about 0.004
    rg, ro = O.recall(ti, gi), O.recall(ti, oi)
    print("%s k=%d nn_descent from the oracle's leaves: GPU %.4f oracle %.4f" % (metric, k, rg, ro))
    assert abs(rg - ro) <= 0.005, (rg, ro)


def _index(metric, d=24, k=15, n=12_000):
    key = (metric, d, k, n)
    if key not in _BUILT:
        x = _data(metric, n, d, seed=43)
        _BUILT[key] = (x, NNDescent(x, metric=metric, n_neighbors=k, random_state=7))
    return _BUILT[key]


@pytest.mark.parametrize("metric", METRICS)
def test_whole_build_against_oracle(metric):
    """NNDescent against O.build_index (the reference algorithm, trees on the raw rows); recall after leaf init is shown
    for both sides."""
    x, index = _index(metric)
    n, k = x.shape[0], 15
    rows = np.arange(n)
    ti, _ = O.brute_force_knn(x, 10, metric)
    oi, _ = O.build_index(x, metric, n_neighbors=k, random_state=7, n_threads=8, kind="fast")
    rg, ro = O.recall(ti, index._neighbor_graph[0][rows]), O.recall(ti, oi[rows])
    # leaf init of both sides (the GPU's own forest, the oracle's forest on the same seed)
    n_trees = O.default_n_trees(n)
    rng_state, _, ts = O.draw_rng_states(7, n_trees)
    b = make_builder(x, metric, k=k, n_trees=n_trees, seed=7)
    try:
        b.make_forest()
        b.init_from_leaves()
        li = b.graph()[0]
    finally:
        b.close()
    la = O.make_leaf_array(x, n_trees, O.default_leaf_size(k), ts, O.ANGULAR[metric])
    oli = O.init_rp_tree(x, k, metric, la)[0]
    print("%s whole build: recall@10 after leaf init GPU %.4f oracle %.4f; final GPU %.4f oracle %.4f"
          % (metric, O.recall(ti, li[rows]), O.recall(ti, oli[rows]), rg, ro))
    assert abs(rg - ro) <= 0.005, (rg, ro)


# ------------------------------------------------------------------------------------------------------ pruning pass
# k = 100: the wide kernels.  Inner product keeps each row's own vertex in its list (d(x, x) = 1 / |x|^2), and a dot row's
# own distance can land above EPS; the row's own vertex is then a comparison point, and both sides must take the stored
# d(i, j) for it (prune.hip, nnd_oracle.c orc_cmp_dist).
@pytest.mark.parametrize("method", ["standard", "degree_aware"])
@pytest.mark.parametrize("k", [15, 100], ids=["k15", "k100-wide"])
@pytest.mark.parametrize("metric", METRICS)
def test_pruning_pass_against_oracle(metric, k, method):
    x, index = _index(metric, k=k, n=12_000 if k == 15 else 4000)
    idx, dist = index._neighbor_graph
    sg, st = build_search_graph(x, idx, dist, metric, k, diversify_method=method, return_stages=True)
    og, ost = O.search_graph(x, idx, dist, metric, k, diversify_method=method, return_stages=True)
    agree = (st["forward_rows"] == ost["forward_rows"]).mean()
    n = x.shape[0]
    a = set(zip(np.repeat(np.arange(n), np.diff(sg.indptr)).tolist(), sg.indices.tolist()))
    c = og.tocoo()
    o = set(zip(c.row.tolist(), c.col.tolist()))
    print("%s k=%d %s: forward agreement %.5f, edge symmetric difference %d of %d" % (metric, k, method, agree, len(a ^ o), len(o)))
    assert agree >= 0.995
    assert len(a ^ o) <= 0.01 * len(o)


# ----------------------------------------------------------------------------------------------------------- queries
@pytest.mark.parametrize("d", [17, 24])
@pytest.mark.parametrize("metric", METRICS)
def test_queries_at_every_list_width(metric, d):
    x, index = _index(metric, d=d, n=6000)
    q = clustered(300, d, min(8, d), 30, 44, nonneg=metric == "hellinger")
    if metric == "inner_product":
        q = q + np.float32(0.5)
    if metric == "dot":
        q = np.ascontiguousarray(q * np.float32(1.7))  # raw queries: the searcher normalises them
        q[5] = 0.0
    index.prepare()
    live = np.ones(q.shape[0], bool)
    if metric == "dot":
        live[5] = False
    qs = normalize(q, norm="l2") if metric == "dot" else q
    qi64, _ = index.query(q, k=64)
    t64 = np.argsort(MU.alt_dist(metric, qs[live], x), axis=1, kind="stable")[:, :10]
    r64 = MU.recall(t64, qi64[live])
    for kq in (10, 100, 200):
        qi, qd = index.query(q, k=kq)
        if metric == "dot":
            assert (qi[5] == -1).all()
        li, ld = qi[live], qd[live]
        # a search that runs out of reachable points (30 clusters of about 200 points, k = 200) leaves -1 at the row's tail
        found = li >= 0
        assert (found[:, :10].all()) and (found.mean(1) > 0.9).all() and (np.diff(found.astype(int), axis=1) <= 0).all()
        assert all(len(set(r[f].tolist())) == f.sum() for r, f in zip(li, found))
        assert (np.diff(np.where(found, ld.astype(np.float64), 1e300), axis=1) >= 0).all()
        true = np.empty(li.shape, np.float64)
        for r, (qq, ids) in enumerate(zip(qs[live], li)):
            true[r] = MU.alt_dist(metric, qq[None, :], x[np.clip(ids, 0, None)])[0]
        np.testing.assert_allclose(ld[found], MU.correct(metric, true)[found], rtol=1e-3 if metric == "hellinger" else 2e-4,
                                   atol=2e-6)
        rec = MU.recall(t64, li)
        if kq > 64:  # (a k = 10 search stops earlier: its first ten are not the k = 64 search's first ten)
            assert rec >= r64 - 0.03, (kq, rec, r64)
        index._searcher.set_tier(1)
        try:
            qi1, qd1 = index.query(q, k=kq)
        finally:
            index._searcher.set_tier(0)
        np.testing.assert_array_equal(qi1, qi)
        np.testing.assert_array_equal(qd1, qd)
        print("%s d=%d k=%d: recall@10 %.4f (k=64: %.4f), %d of %d rows short of k" % (metric, d, kq, rec, r64,
                                                                              int((~found.all(1)).sum()), len(li)))


@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_uint8_padded_code_rows(metric):
    """d = 13 (code rows padded to 16) at query k = 100: device codes equal np.searchsorted, exact reranked distances, rows
    sorted and unique."""
    x = clustered(4000, 13, 6, 20, seed=51)
    q = clustered(200, 13, 6, 20, seed=52)
    index = NNDescent(x, metric=metric, n_neighbors=15, random_state=3, quantization="uint8")
    index.prepare()
    raw = index._raw_data  # the searcher's rows (dot: normalised), in its order
    want = np.searchsorted(index._quantized_values, raw).astype(np.uint8)
    np.testing.assert_array_equal(index._quantized_data, want)
    qi, qd = index.query(q, k=100, proxy_beam_size=2)  # (the walk keeps proxy_beam_size * k <= 256)
    assert (qi >= 0).all() and all(len(set(r.tolist())) == 100 for r in qi)
    assert (np.diff(qd, axis=1) >= 0).all()
    xo = raw[np.argsort(index._vertex_order)]
    a = q.astype(np.float64)[:, None, :]
    b = xo.astype(np.float64)[qi]
    g = (a * b).sum(-1)
    want_d = 1.0 - g if metric == "dot" else 1.0 - g / np.sqrt((a * a).sum(-1) * (b * b).sum(-1))
    np.testing.assert_allclose(qd, want_d, rtol=2e-4, atol=2e-6)


# ------------------------------------------------------------------------------------------------------------ shards
@pytest.mark.parametrize("metric", METRICS)
def test_two_rank_build(metric):
    x = _data(metric, 8000, 24, seed=61)
    rows = np.random.RandomState(3).choice(x.shape[0], 1000, replace=False)
    truth = _truth_rows(metric, x, rows)
    single = NNDescent(x, metric=metric, n_neighbors=40, max_candidates=50, random_state=4)
    multi = NNDescent(x, metric=metric, n_neighbors=40, max_candidates=50, random_state=4, n_devices=2, devices=[0, 0])
    rs_, rm = MU.recall(truth, single._neighbor_graph[0][rows]), MU.recall(truth, multi._neighbor_graph[0][rows])
    print("%s two ranks: recall@10 single %.4f two ranks %.4f" % (metric, rs_, rm))
    assert abs(rs_ - rm) <= 0.005
