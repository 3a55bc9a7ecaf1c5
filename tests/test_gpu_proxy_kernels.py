"""proxy_inner_product (metric code 6) on every build kernel that converts a Gram value, on a real MI355X, against the float64
formula with the a-priori float32 radius of tests/proxy_util.py (the oracle does not know the code).

Which kernels a case reaches (tests/descent_cases.py, tests/test_gpu_metric_kernels.py): k <= 16 -> k_leaf_join, k_local_join16,
k_merge_q; k 17..32 -> k_leaf_join_sym, k_local_join_w<32> staged, k_merge; k = 100, max_candidates 60 -> k_leaf_join_rb wide,
k_local_join_w<64>, k_merge_wide, k_finalize_wide.  Code 6 has join instances of its own (XM = 2)."""
import numpy as np
import pytest

from pynndescent_amd import NNDescent
from pynndescent_amd.search_graph import build_search_graph
from tests import descent_reference as DR
from tests import proxy_descent as PD
from tests import proxy_util as PU
from tests.test_gpu_descent_exact import _check as check_iteration

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------- prep + Gram
def _edge_rows(d):
    """300 rows: positive rows over four decades of length; rows 0..9 zero; rows 10..59 negated (products with the positive rows
    are clearly negative); from d = 2 on rows 60..79 live on the even and rows 80..99 on the odd columns (products exactly 0)."""
    rs = np.random.RandomState(100 + d)
    x = ((np.abs(rs.standard_normal((300, d))) + 0.1) * 10.0 ** rs.uniform(-2, 2, (300, 1))).astype(np.float32)
    x[:10] = 0.0
    x[10:60] *= -1.0
    if d >= 2:
        x[60:80, 1::2] = 0.0
        x[80:100, 0::2] = 0.0
    return np.ascontiguousarray(x)


@pytest.mark.parametrize("d", [1, 3, 4, 5, 17, 36, 64, 127, 128, 130, 256, 260])
def test_prep_and_gram_at_dimension_edges(d):
    """nnd_pairwise_gram after the prep kernel that d selects (scalar / float4, every lanes-per-row width): FLT_MAX exactly where
    a row is zero or <a, b> <= 0, every other value inside the a-priori interval and >= 0."""
    x = _edge_rows(d)
    b = PD.make_builder(x, k=10, n_trees=0)
    try:
        rows_a = np.concatenate([np.arange(0, 120), np.arange(200, 230)]).astype(np.int32)
        rows_b = np.concatenate([np.arange(5, 100, 3), np.arange(100, 160), [0, 10, 60, 80]]).astype(np.int32)
        got = b.pairwise_gram(rows_a, rows_b).astype(np.float64)
    finally:
        b.close()
    mid, lo, hi = PU.proxy_matrix_f32(x[rows_a], x[rows_b])
    far = mid >= PU.FLT_MAX
    assert far.any() and (~far).any()
    assert np.array_equal(got == PU.FLT_MAX, far), np.argwhere((got == PU.FLT_MAX) != far)[:5]
    assert (got >= 0.0).all() and np.isfinite(got).all()
    assert PU.within(got, lo, hi).all(), np.argwhere(~PU.within(got, lo, hi))[:5]
    ratio = np.abs(got - mid)[~far] / np.maximum(hi - mid, mid - lo)[~far]
    print("d = %d: %d pairs, %d at FLT_MAX, max |err| / radius %.3f" % (d, got.size, int(far.sum()), float(ratio.max())))


# ------------------------------------------------------------------------------------------------- one descent iteration
def _stored_ok(label, x, prep, idx, dist):
    """rows ascending, ids unique, and every stored distance that of its id within the radius (self pairs by the self rule)."""
    n, k = idx.shape
    valid = idx >= 0
    d64 = np.where(valid, dist.astype(np.float64), np.inf)
    assert np.all(np.diff(np.where(np.isfinite(d64), d64, 1e39), axis=1) >= 0), label + ": rows not ascending"
    assert np.all(np.isinf(dist[~valid])), label + ": an unfilled slot does not hold +inf"
    srt = np.sort(np.where(valid, idx, -1 - np.arange(k)[None, :]), axis=1)
    assert (np.diff(srt, axis=1) != 0).all(), label + ": duplicate ids"
    mid, lo, hi = PU.proxy_pairs_f32(x[:, None, :], x[np.where(valid, idx, 0)])
    own = valid & (idx == np.arange(n)[:, None])
    lo = np.where(own, (prep.self_mid - prep.self_rad)[:, None], lo)
    hi = np.where(own, (prep.self_mid + prep.self_rad)[:, None], hi)
    ok = PU.within(np.where(valid, dist, 0.0), lo, hi) | ~valid
    assert ok.all(), "%s: %d stored distances outside the radius, first at %s" % (label, int((~ok).sum()), np.argwhere(~ok)[0])
    assert (dist[valid] >= 0.0).all()


@pytest.mark.parametrize("name", list(PD.CASES))
def test_descent_iteration_equals_the_model(name):
    """The leaf seeding's stored distances, then nnd_descent_iter against tests/descent_reference.py reference_iter with the
    code-6 Prepared of tests/proxy_descent.py: id sets, flags, every stored distance within the radius, rows ascending, the
    counters (the checks of tests/test_gpu_descent_exact.py)."""
    case = PD.CASES[name]
    x = np.array(PD.data(case))
    prep = PD.ProxyPrepared(x)
    b = PD.make_builder(x, k=case.k, n_trees=case.n_trees, mc=case.mc, seed=case.seed, join_blocks=case.join_blocks, flags=case.flags)
    try:
        b.make_forest()
        b.init_from_leaves()
        idx, dist, _ = b.graph()
        _stored_ok(name + " leaf seeding", x, prep, idx, dist)
        assert (idx >= 0).mean() > 0.9
        b.init_random()
        for it in range(max(case.iters) + 1):
            if it not in case.iters:
                b.descent_iter()
                continue
            s0 = b.graph()
            c = b.descent_iter()
            new, old = b.candidates()
            got = b.graph()
            st = b.stats(raw=True)
            res = DR.reference_iter(prep, None, s0[0], s0[1], s0[2], new, old, case.k, PD.rng_state(case), it, case.join_blocks)
            label = "%s iteration %d" % (name, it)
            share = float((res.ambiguous != 0).mean())
            counters = (int(c), int(st.proposals[it]), int(st.join_pairs[it]))
            print("%s (%s): %.2f %% of %d rows ambiguous, %d unclear decisions; c / proposals / pairs gpu %s model %s" % (
                label, case.doc, 100 * share, case.n, res.n_unclear, counters, (res.c, res.proposals, res.join_pairs)))
            ratio = check_iteration(label, case, prep, s0, got, res)
            print("%s: max |err| / radius %.3f" % (label, ratio))
            assert share <= 0.10, "%s: %.2f %% of the rows are ambiguous, the cap is 10 %%" % (label, 100 * share)
            assert counters[2] == res.join_pairs, label
            assert abs(counters[0] - res.c) <= res.n_unclear and abs(counters[1] - res.proposals) <= res.n_unclear, (label, counters, res.c, res.proposals)
            _stored_ok(label, x, prep, got[0], got[1])
        fi, fd = b.finalize()
    finally:
        b.close()
    # k_finalize<6> / k_finalize_wide: float64 accumulation of the formula, rows re-sorted by (distance, id)
    valid = fi >= 0
    assert valid.mean() > 0.99
    mid, rad = PU.proxy_pairs_f64(x[:, None, :], x[np.where(valid, fi, 0)])
    assert np.array_equal(fd[valid] == PU.FLT_MAX, mid[valid] == PU.FLT_MAX)
    assert np.all(np.abs(fd.astype(np.float64) - mid)[valid] <= rad[valid])
    key = np.where(valid, fd.astype(np.float64), np.inf)
    same = np.diff(key, axis=1) == 0
    assert (np.diff(key, axis=1) >= 0).all() and (np.diff(fi, axis=1)[same & valid[:, 1:]] > 0).all(), "rows by (distance, id)"
    own = fi == np.arange(case.n)[:, None]
    assert np.all(np.abs(fd[own] - prep.self_mid[np.nonzero(own)[0]]) <= 2 * PU._ulp32(fd[own])), "the self pair is 1 / |x|"


# ------------------------------------------------------------------------------------------------------ pruning pass
_BUILT = {}


def _index(n=4000, d=24, k=15):
    if (n, d, k) not in _BUILT:
        x = PU.MU.metric_data("inner_product", n, d, seed=13)[0]
        x[[7, 500]] = 0.0
        _BUILT[(n, d, k)] = (x, NNDescent(x, metric=PU.METRIC, n_neighbors=k, random_state=7))
    return _BUILT[(n, d, k)]


@pytest.mark.parametrize("method", ["standard", "degree_aware"])
def test_pruning_pass(method):
    """The forward diversify pass at k = 15: a kept edge keeps its stored distance, which is the proxy of its endpoints; no kept
    edge has an earlier kept neighbour that is clearly (outside the radius) nearer to it than the row's vertex; every pruned
    edge has one that may be.  degree_aware scales the limit by a factor in [0.8, 1.2] (pynndescent_.py:506-521): the bounds
    take the end of that range that makes the check sure."""
    x, index = _index()
    idx, dist = index._neighbor_graph
    k = idx.shape[1]
    graph, st = build_search_graph(x, idx, dist, PU.METRIC, k, diversify_method=method, return_stages=True)
    fr, fdist = st["forward_rows"], st["forward_dist"]
    kept_f, prune_f = (0.8, 1.2) if method == "degree_aware" else (1.0, 1.0)
    n_kept = n_pruned = 0
    for i in range(x.shape[0]):
        row, rd = idx[i], dist[i].astype(np.float64)
        keep = fr[i][fr[i] >= 0]
        pos = np.nonzero(np.isin(row, keep) & (row >= 0))[0]
        assert np.array_equal(row[pos], keep) and np.array_equal(dist[i][pos], fdist[i][:len(keep)]), i  # in order, distances untouched
        assert len(keep) and pos[0] == 0
        live = row >= 0
        _, lo, hi = PU.proxy_matrix_f32(x[row[live]], x[row[live]])
        for j in np.nonzero(live)[0][1:]:
            earlier = [c for c in pos if c < j and rd[c] > 1.1920929e-07 and row[c] != i]
            if j in pos:
                n_kept += 1
                assert all(hi[j, c] >= kept_f * rd[j] for c in earlier), (i, j)
            else:
                n_pruned += 1
                assert any(lo[j, c] < prune_f * rd[j] for c in earlier) or any(row[c] == i for c in pos if c < j), (i, j)
    mid, rad = PU.proxy_pairs_f64(x[:, None, :], x[np.maximum(idx, 0)])
    assert np.all(np.abs(dist.astype(np.float64) - mid)[idx >= 0] <= rad[idx >= 0])
    assert graph.shape == (x.shape[0],) * 2 and st["final_nnz"] > 0 and st["min_distance"] > 0.0
    print("%s: %d edges kept, %d pruned in the forward pass; %d in the search graph; min_distance %.4f" % (
        method, n_kept, n_pruned, st["final_nnz"], st["min_distance"]))
    assert n_pruned > 0 and n_kept > 0


# ------------------------------------------------------------------------------------------------------------ shards
def test_two_rank_build():
    """devices=[0, 0]: two ranks on one GPU, the sharded path (csrc/shard.hip) by the same params."""
    x, single = _index()
    rows = np.random.RandomState(3).choice(x.shape[0], 1000, replace=False)
    truth = PU.proxy_truth(x, x[rows])
    multi = NNDescent(x, metric=PU.METRIC, n_neighbors=15, random_state=7, n_devices=2, devices=[0, 0])
    mi, md = multi._neighbor_graph
    assert ((mi >= 0) & (mi < x.shape[0])).all()
    assert (np.diff(md.astype(np.float64), axis=1) >= 0).all()
    mid, rad = PU.proxy_pairs_f64(x[:, None, :], x[mi])
    assert np.all(np.abs(md.astype(np.float64) - mid) <= rad)
    r1, r2 = PU.recall(truth, single._neighbor_graph[0][rows]), PU.recall(truth, mi[rows])
    print("two ranks: recall@10 against float64 proxy brute force: one rank %.4f, two ranks %.4f" % (r1, r2))
    assert abs(r1 - r2) <= 0.01
