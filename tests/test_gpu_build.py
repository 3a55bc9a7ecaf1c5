"""End-to-end parity of the HIP build path with the CPU oracle / reference fixtures (MI355X)."""
import os
import warnings

import numpy as np
import pytest

from oracle import oracle as O
from pynndescent_amd import NNDescent
from tests.gpu_util import check_graph_invariants
from tests.util_data import clustered, nn_data_like

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _true_alt_to_corrected(x, idx, metric):
    xi = x.astype(np.float64)
    nb = xi[np.where(idx >= 0, idx, 0)]
    if metric == "euclidean":
        return np.sqrt(((xi[:, None, :] - nb) ** 2).sum(-1))
    dot = (xi[:, None, :] * nb).sum(-1)
    na = np.sqrt((xi * xi).sum(1))[:, None]
    nbn = np.sqrt((nb * nb).sum(-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        cosd = 1.0 - dot / (na * nbn)
    cosd = np.where((na == 0) & (nbn == 0), 0.0, np.where((na == 0) | (nbn == 0) | (dot <= 0), 1.0, cosd))
    return cosd


def _parity(x, metric, k, gpu_idx, ref_idx, band=0.005, k_true=10, two_sided=True):
    """recall@k_true of both sides against exact neighbours.  ``two_sided``: |r_gpu - r_ref| <= band -- the north-star
    contract (+-0.5 %) when the reference side is the CPU oracle run on the SAME inputs with the same parameters; a build
    that silently did MORE work than the reference algorithm would fail it too.  One-sided (r_gpu >= r_ref - band) only
    against the coarse T0 fixtures (reference run at another thread count / RNG stream on a few thousand points)."""
    ti, _ = O.brute_force_knn(x, k_true, metric)
    r_gpu, r_ref = O.recall(ti, gpu_idx), O.recall(ti, ref_idx)
    print("recall@%d: gpu %.4f reference-algorithm %.4f" % (k_true, r_gpu, r_ref))
    if two_sided:
        assert abs(r_gpu - r_ref) <= band, (r_gpu, r_ref)
    else:
        assert r_gpu >= r_ref - band, (r_gpu, r_ref)
    return r_gpu, r_ref


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_reference_test_shape_nn_data(metric):
    """tests/test_pynndescent_.py:19-53: positional 10 binds to bit_metric, build runs at k=30; floor 0.98."""
    x = nn_data_like()
    idx, dist = NNDescent(x, metric, {}, 10, random_state=np.random.RandomState(189212))._neighbor_graph
    assert idx.shape == (1002, 30)
    g = np.load(os.path.join(GOLDEN, "class_nndata_%s.npz" % metric))
    r_gpu, r_ref = _parity(x, metric, 30, idx, g["idx"], two_sided=False)
    assert r_gpu >= 0.98


def test_clustered_against_reference_fixture():
    g = np.load(os.path.join(GOLDEN, "build_clustered_euclidean_T4.npz"))
    n, d, latent, ncl, seed = (int(v) for v in g["gen"])
    x = clustered(n, d, latent, ncl, seed)
    index = NNDescent(x, "euclidean", n_neighbors=15, n_trees=8, random_state=5)
    idx, dist = index.neighbor_graph
    _parity(x, "euclidean", 15, idx, g["idx"], two_sided=False)
    # distances of the returned pairs: exact to 1e-5 relative (north_star)
    np.testing.assert_allclose(dist, _true_alt_to_corrected(x, idx, "euclidean"), rtol=1e-5, atol=1e-7)
    assert np.all(np.diff(dist, axis=1) >= 0)


def test_iid_cosine_against_reference_fixture():
    g = np.load(os.path.join(GOLDEN, "build_iid_cosine_T4.npz"))
    n, d, seed = (int(v) for v in g["gen"])
    x = np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)
    index = NNDescent(x, "cosine", n_neighbors=15, n_trees=8, random_state=6)
    idx, dist = index.neighbor_graph
    _parity(x, "cosine", 15, idx, g["idx"], band=0.01, two_sided=False)
    truth = _true_alt_to_corrected(x, idx, "cosine")
    np.testing.assert_allclose(dist, truth, rtol=1e-5, atol=2e-7)


def test_wide_rows_and_candidate_lists_against_reference_fixture():
    """The reference itself at k = 70, max_candidates = 80 (un-jitted run, tests/golden/make_golden.py gen_build_wide; the oracle
    reproduces it bit for bit): 400 points, 4 iterations -- recall@70 of the GPU build against the reference's, distances exact."""
    g = np.load(os.path.join(GOLDEN, "build_wide_euclidean_T2.npz"))
    n, d, latent, ncl, seed = (int(v) for v in g["gen"])
    x = clustered(n, d, latent, ncl, seed)
    index = NNDescent(x, "euclidean", n_neighbors=70, n_trees=2, max_candidates=80, n_iters=4, random_state=9)
    idx, dist = index.neighbor_graph
    r_gpu, r_ref = _parity(x, "euclidean", 70, idx, g["idx"], k_true=70, two_sided=False)
    assert abs(r_gpu - r_ref) <= 0.01
    np.testing.assert_allclose(dist, _true_alt_to_corrected(x, idx, "euclidean"), rtol=1e-5, atol=1e-7)


def test_baseline_config1_plumbing():
    """BASELINE.json configs[0]: 10k x 64 random, euclidean, k=10, n_iters=5 (reference fixture, recall ~0.49)."""
    g = np.load(os.path.join(GOLDEN, "build_c1_T8.npz"))
    x = np.random.RandomState(0).standard_normal((10000, 64)).astype(np.float32)
    idx, _ = NNDescent(x, "euclidean", n_neighbors=10, n_trees=8, n_iters=5, random_state=0)._neighbor_graph
    # round 6: two-sided +-0.01 against the REFERENCE'S OWN graph (the fixture is the unmodified reference at 8 threads;
    # recall ~0.48: a regime where nothing saturates -- 0.4840 vs 0.4835 at the end of round 5)
    r_gpu, r_ref = _parity(x, "euclidean", 10, idx, g["idx"], band=0.01, two_sided=True)


def test_sift_like_medium_vs_oracle():
    x = clustered(20000, 128, 16, 256, seed=1, nonneg=True) * 20.0
    index = NNDescent(x, "euclidean", n_neighbors=15, n_trees=8, random_state=2)
    idx, dist = index.neighbor_graph
    oidx, _ = O.build_index(x, "euclidean", n_neighbors=15, n_trees=8, random_state=2, n_threads=8, kind="fast")
    r_gpu, r_ref = _parity(x, "euclidean", 15, idx, oidx)
    assert r_gpu >= 0.95
    np.testing.assert_allclose(dist, _true_alt_to_corrected(x, idx, "euclidean"), rtol=1e-5, atol=1e-6)
    st = index._build_stats
    print("stats", {k: st[k] for k in ("n_iters_run", "n_leaves", "tree_levels", "ms_forest", "ms_leaf_init", "ms_descent")})


def test_glove_like_cosine_d100_vs_oracle():
    x = clustered(12000, 100, 24, 128, seed=2)
    index = NNDescent(x, "cosine", n_neighbors=15, n_trees=8, random_state=3)
    idx, dist = index.neighbor_graph
    oidx, _ = O.build_index(x, "cosine", n_neighbors=15, n_trees=8, random_state=3, n_threads=8, kind="fast")
    _parity(x, "cosine", 15, idx, oidx)
    np.testing.assert_allclose(dist, _true_alt_to_corrected(x, idx, "cosine"), rtol=1e-5, atol=2e-7)


def test_deterministic_for_a_seed():
    """tests/test_pynndescent_.py:279-291 in spirit: same seed -> identical graph."""
    x = np.random.RandomState(42).normal(0, 100, (1000, 50)).astype(np.float32)
    a = NNDescent(x, random_state=np.random.RandomState(42))._neighbor_graph
    b = NNDescent(x, random_state=np.random.RandomState(42))._neighbor_graph
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_duplicate_heavy_inputs_keep_rows_unique():
    """tests/test_pynndescent_.py:299-314, 352-369."""
    near = np.load(os.path.join(GOLDEN, "reference_testdata_cosine_near_duplicates.npz"))["data"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        idx, _ = NNDescent(near, "cosine", {}, 10, random_state=np.random.RandomState(189212), n_trees=20)._neighbor_graph
    for row in idx:
        v = row[row >= 0]
        assert len(v) == len(np.unique(v))
    hang = np.load(os.path.join(GOLDEN, "reference_testdata_cosine_hang.npz"))["data"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        idx, _ = NNDescent(hang, "cosine", {}, 10, random_state=np.random.RandomState(189212), n_trees=20)._neighbor_graph
    for row in idx:
        v = row[row >= 0]
        assert len(v) == len(np.unique(v))


def test_deduplicated_data_behaves_normally():
    """tests/test_pynndescent_.py:317-349: recall >= 0.95 (k=30 effective, true top-10)."""
    hang = np.load(os.path.join(GOLDEN, "reference_testdata_cosine_hang.npz"))["data"]
    data = np.unique(hang, axis=0)
    data = data[~np.all(data == 0, axis=1)][:1000]
    idx, _ = NNDescent(data, "cosine", {}, 10, random_state=np.random.RandomState(189212), n_trees=20)._neighbor_graph
    g = np.load(os.path.join(GOLDEN, "class_dedup_hang_cosine.npz"))
    # the fixture was generated at n_neighbors=10 (keyword), the reference test shape is k=30: compare like for like
    idx10, _ = NNDescent(data, "cosine", n_neighbors=10, random_state=np.random.RandomState(189212), n_trees=20)._neighbor_graph
    r_gpu, r_ref = _parity(data, "cosine", 10, idx10, g["idx"], band=0.01, two_sided=False)
    ti, _ = O.brute_force_knn(data, 10, "cosine")
    assert O.recall(ti, idx) >= 0.95


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_tree_init_false(metric):
    x = nn_data_like()[200:]
    idx, _ = NNDescent(x, metric=metric, n_neighbors=10, random_state=3, tree_init=False)._neighbor_graph
    oidx, _ = O.build_index(x, metric, n_neighbors=10, random_state=3, tree_init=False, n_threads=1)
    _parity(x, metric, 10, idx, oidx, band=0.01)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_leaf_size_larger_than_n(metric):
    """tests/test_pynndescent_.py:716-747: leaf_size > n, k = n - 1: the graph must be complete."""
    x = np.random.RandomState(17).uniform(5, 40, size=(10, 5)).astype(np.float32)
    idx, dist = NNDescent(x, metric=metric, n_neighbors=9, random_state=4, leaf_size=21)._neighbor_graph
    for r in range(10):
        assert set(idx[r].tolist()) <= set(range(10)) and len(set(idx[r].tolist())) == 9


def test_tiny_inputs_every_k_up_to_n_plus_2():
    """n = 1 .. 40 against every k in {1, 2, 3, n - 1, n, n + 2} (both metrics, d = 1 / 3 / 32): every row holds min(k, n) distinct
    points in ascending order, or the call is refused up front with a message (tools/tiny_sizes.py)."""
    from tools.tiny_sizes import run

    n_ok, bad = run(verbose=False)
    print("tiny inputs: %d builds ok, %d failures" % (n_ok, bad))
    assert bad == 0 and n_ok > 300


def test_builds_from_several_threads_equal_the_builds_made_alone():
    """SURVEY 8b "re-entrant across independent handles": four Python threads build three indexes each at the same time on one device
    (different sizes, metrics, k); every graph equals, bit for bit, the one the same call returns alone (tools/threads.py)."""
    from tools.threads import run

    assert run(4, 3, verbose=True) == 0


def test_bad_data_smoke_wide_rows():
    """tests/test_pynndescent_.py:750-756: 1011 x 3500, cosine, defaults (k=30)."""
    arr = np.load(os.path.join(GOLDEN, "reference_testdata_bad_data.npz"))["arr_0"]
    data = np.sqrt(arr).astype(np.float32)
    index = NNDescent(data, metric="cosine", random_state=0)
    idx, dist = index.neighbor_graph
    oidx, _ = O.build_index(data, "cosine", n_neighbors=30, random_state=0, n_threads=8, kind="fast")
    _parity(data, "cosine", 30, idx, oidx, band=0.01)


def test_random_state_none():
    """tests/test_pynndescent_.py:261-276: random_state=None (a fresh global-RNG seed per call), positional metric_kwds and
    n_neighbors: at least 99 % of the true 10 neighbours."""
    x = nn_data_like()
    idx, _ = NNDescent(x, "euclidean", {}, 10, random_state=None)._neighbor_graph
    ti, _ = O.brute_force_knn(x, 10, "euclidean")
    assert O.recall(ti, idx) >= 0.99
    idx2, _ = NNDescent(x, "euclidean", {}, 10, random_state=None)._neighbor_graph
    assert O.recall(ti, idx2) >= 0.99


def test_no_output_when_verbose_is_false(capsys):
    """tests/test_pynndescent_.py:390-405 on the reference's spatial_data shape (10 random rows + 2 zero rows x 20)."""
    rs = np.random.RandomState(42)
    x = np.vstack([rs.standard_normal((10, 20)), np.zeros((2, 20))]).astype(np.float32, order="C")
    NNDescent(data=x, metric="euclidean", metric_kwds={}, n_neighbors=4, random_state=np.random.RandomState(7), n_trees=5, n_iters=2,
              verbose=False)
    assert capsys.readouterr().out.strip() == ""


def test_one_dimensional_data():
    """tests/test_pynndescent_.py:687-713 (the euclidean case): one column, tree_init=False, random_state=None, k = 20; prepare() and
    query(k=10, epsilon=0.2) reach 95 % of the true neighbours."""
    x = nn_data_like()
    nnd = NNDescent(x[200:, :1], metric="euclidean", n_neighbors=20, random_state=None, tree_init=False)
    nnd.prepare()
    qi, _ = nnd.query(x[:200, :1], k=10, epsilon=0.2)
    base = x[200:, :1].astype(np.float64)
    d = np.abs(x[:200, :1].astype(np.float64) - base.T)
    ti = np.argsort(d, axis=1, kind="stable")[:, :10]
    # ties (duplicate coordinates, the two zero rows) count by DISTANCE: a returned point as close as the 10th true one is correct
    kth = np.take_along_axis(d, ti[:, 9:10], axis=1)
    got = np.take_along_axis(d, np.where(qi >= 0, qi, 0), axis=1)
    assert ((got <= kth + 1e-12) & (qi >= 0)).sum() / (200 * 10) >= 0.95


def test_init_graph_and_errors():
    x = clustered(1200, 10, 4, 6, seed=23)
    ti, _ = O.brute_force_knn(x, 10, "euclidean")
    rs = np.random.RandomState(0)
    noisy = np.where(rs.uniform(size=ti.shape) < 0.5, rs.randint(0, 1200, ti.shape), ti).astype(np.int32)
    idx, _ = NNDescent(x, n_neighbors=10, init_graph=noisy, random_state=1)._neighbor_graph
    assert O.recall(ti, idx) > 0.95
    with pytest.raises(ValueError, match="Init graph size does not match dataset size!"):
        NNDescent(x, n_neighbors=10, init_graph=noisy[:50])
    with pytest.raises(ValueError, match="do not match"):
        NNDescent(x, n_neighbors=10, init_graph=noisy, init_dist=np.zeros((1200, 3), np.float32))
    with pytest.raises(ValueError, match="Metric is neither callable"):
        NNDescent(x, metric="not_a_metric")


def test_verbose_output(capsys):
    """tests/test_pynndescent_.py:372-387."""
    import re

    x = np.vstack([np.random.RandomState(1).randn(10, 20), np.zeros((2, 20))]).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        NNDescent(data=x, metric="euclidean", metric_kwds={}, n_neighbors=4, random_state=np.random.RandomState(189212),
                  n_trees=5, n_iters=2, verbose=True)
    out = capsys.readouterr().out
    assert re.match("^.*5 trees", out, re.DOTALL) and re.match("^.*2 iterations", out, re.DOTALL)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        NNDescent(data=x, metric="euclidean", n_neighbors=4, random_state=1, n_trees=5, n_iters=2, verbose=False)
    assert capsys.readouterr().out.strip() == ""


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_search_graph_pruning_pass_vs_reference_fixture(metric):
    """BASELINE config 5's pass: the reference's own diversify / diversify_csr / degree_prune run (fixture) on a
    reference-built graph vs the HIP kernels on the same graph; and the class-level entry point vs the oracle."""
    from pynndescent_amd.search_graph import build_search_graph

    g = np.load(os.path.join(GOLDEN, "search_graph.npz"))
    n, d, latent, ncl, seed = (int(v) for v in g[metric + "_gen"])
    x = clustered(n, d, latent, ncl, seed)
    sg, st = build_search_graph(x, g[metric + "_idx"], g[metric + "_dist"], metric, 15, return_stages=True)
    fr = g[metric + "_fwd_rows"]
    agree = (st["forward_rows"] == fr).mean()
    print("forward diversify agreement %.5f; nnz %d -> %d -> %d" % (agree, st["forward_nnz"], st["union_nnz"], st["final_nnz"]))
    assert agree > 0.995
    # tightened by the step-exact model (tests/prune_reference.py): every forward row the model can pin IS the reference's
    from tests import prune_reference as PR

    model = PR.diversify_rows(PR.Prepared(x, metric), g[metric + "_idx"], g[metric + "_dist"])
    off = np.nonzero((st["forward_rows"] != fr).any(1) & (model.flags == 0))[0]
    assert not len(off), (off[:5], int((model.flags != 0).sum()))
    a = set(zip(np.repeat(np.arange(n), np.diff(sg.indptr)).tolist(), sg.indices.tolist()))
    b = set(zip(np.repeat(np.arange(n), np.diff(g[metric + "_indptr"])).tolist(), g[metric + "_indices"].tolist()))
    assert len(a ^ b) <= 0.01 * len(b), (len(a ^ b), len(b))
    assert sg.dtype == np.uint8 and np.diff(sg.indptr).max() <= int(np.round(1.5 * 15)) + 1
    assert sg.diagonal().sum() == 0


@pytest.mark.parametrize("tag,metric,method,prob,aggr", [("euclidean", "euclidean", "standard", 1.0, 1.0), ("cosine", "cosine", "standard", 1.0, 1.0),
                                                        ("prob_euclidean", "euclidean", "standard", 0.5, 1.0),
                                                        ("aware_cosine", "cosine", "degree_aware", 1.0, 2.0),
                                                        ("aware_euclidean", "euclidean", "degree_aware", 0.7, 1.0)])
def test_device_search_graph_pass_equals_the_scipy_glued_pass(tag, metric, method, prob, aggr):
    """Round 5: COO -> CSR, transpose, maximum, setdiag / eliminate_zeros, binarise (pynndescent_.py:1527-1611: scipy calls in the
    reference, and in rounds 2-4 here) on the device (csrc/searchgraph.hip: keyed edges, radix sort, fold).  Same kernels for
    the three numba functions, same coins: the search graph must be IDENTICAL to the scipy-glued pass, edge for edge, and the
    stage counts with it -- on the reference-built graphs of the fixtures, in every mode."""
    from pynndescent_amd.search_graph import build_search_graph

    if tag in ("euclidean", "cosine"):
        g = np.load(os.path.join(GOLDEN, "search_graph.npz"))
    else:
        g = np.load(os.path.join(GOLDEN, "search_graph_modes.npz"))
    n, d, latent, ncl, seed = (int(v) for v in g[tag + "_gen"])
    x = clustered(n, d, latent, ncl, seed)
    kw = dict(diversify_prob=prob, diversify_method=method, degree_prune_aggressiveness=aggr, seed=77, return_stages=True)
    a, sa = build_search_graph(x, g[tag + "_idx"], g[tag + "_dist"], metric, 15, **kw)
    b, sb = build_search_graph(x, g[tag + "_idx"], g[tag + "_dist"], metric, 15, host_glue=True, **kw)
    b.sort_indices()
    assert np.array_equal(sa["forward_rows"], sb["forward_rows"])
    np.testing.assert_array_equal(sa["forward_dist"], sb["forward_dist"])
    for key in ("forward_nnz", "reverse_nnz", "union_nnz", "final_nnz"):
        assert sa[key] == sb[key], (key, sa[key], sb[key])
    assert sa["min_distance"] == np.float32(sb["min_distance"])
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    assert a.dtype == np.uint8 and (a.data == 1).all()
    # a graph with holes and an exact duplicate point (distance 0 -> FLOAT32_EPS), rows of different lengths
    idx2, dist2 = g[tag + "_idx"].copy(), g[tag + "_dist"].copy()
    idx2[::7, 9:] = -1
    dist2[::7, 9:] = np.inf
    dist2[::5, 1] = 0.0
    a2 = build_search_graph(x, idx2, dist2, metric, 15, diversify_prob=prob, diversify_method=method, degree_prune_aggressiveness=aggr, seed=5)
    b2 = build_search_graph(x, idx2, dist2, metric, 15, diversify_prob=prob, diversify_method=method, degree_prune_aggressiveness=aggr, seed=5,
                            host_glue=True)
    b2.sort_indices()
    assert np.array_equal(a2.indptr, b2.indptr) and np.array_equal(a2.indices, b2.indices)


def test_search_graph_nytimes_like_cosine_d256():
    """Config-5 shape (angular, d=256, k=15) at reduced n: GPU build + GPU pruning pass vs the oracle's pass on the
    SAME neighbour graph (edge sets within 1 %), plus degree bound and symmetry of the union."""
    x = clustered(20000, 256, 32, 200, seed=4)
    index = NNDescent(x, "cosine", n_neighbors=15, random_state=4)
    sg = index.build_search_graph()
    osg = O.search_graph(x, index._neighbor_graph[0], index._neighbor_graph[1], "cosine", 15)
    n = x.shape[0]
    a = set(zip(np.repeat(np.arange(n), np.diff(sg.indptr)).tolist(), sg.indices.tolist()))
    b = set(zip(np.repeat(np.arange(n), np.diff(osg.indptr)).tolist(), osg.indices.tolist()))
    print("search graph nnz gpu %d oracle %d symmetric difference %d" % (len(a), len(b), len(a ^ b)))
    assert len(a ^ b) <= 0.01 * len(b)
    assert np.diff(sg.indptr).max() <= 23 + 1 and sg.shape == (n, n)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_update_against_reference_fixture(metric):
    """NNDescent.update (pynndescent_.py:2381-2553): same inputs as the reference run recorded in the fixture; the
    updated graph must reach the reference's recall on the NEW data, hold exact distances and no stale edges."""
    g = np.load(os.path.join(GOLDEN, "update_%s_T2.npz" % metric))
    n, d, latent, ncl, seed = (int(v) for v in g["gen"])
    x = clustered(n, d, latent, ncl, seed)
    index = NNDescent(x.copy(), metric, n_neighbors=int(g["k"]), n_trees=int(g["n_trees"]), n_iters=int(g["n_iters"]),
                      random_state=np.random.RandomState(int(g["seed"])))
    before = index._neighbor_graph[0].copy()
    index.update(xs_fresh=g["fresh"], xs_updated=g["upd"], updated_indices=g["upd_idx"])
    np.testing.assert_array_equal(index._raw_data, g["raw_after"])
    idx, dist = index.neighbor_graph
    assert idx.shape == g["after_idx"].shape == (n + g["fresh"].shape[0], int(g["k"]))
    assert index.n_trees == index.n_trees_after_update == 2
    raw = g["raw_after"]
    _parity(raw, metric, int(g["k"]), idx, g["after_idx"], k_true=int(g["k"]), two_sided=False)
    np.testing.assert_allclose(dist, _true_alt_to_corrected(raw, idx, metric), rtol=1e-5, atol=1e-6)
    assert np.all(np.diff(dist, axis=1) >= 0)
    for row in idx[::17]:
        assert len(set(row.tolist())) == len(row)
    # the warm start matters: untouched rows keep most of their old neighbours
    keep = np.setdiff1d(np.arange(n), g["upd_idx"])[::7]
    same = np.mean([len(np.intersect1d(before[i], idx[i])) / before.shape[1] for i in keep])
    assert same > 0.8, same


def test_update_errors_and_plain_refresh():
    x = clustered(600, 8, 4, 10, seed=3)
    index = NNDescent(x, "euclidean", n_neighbors=8, random_state=1)
    with pytest.raises(ValueError, match="updated_indices must also be provided"):
        index.update(xs_updated=x[:3])
    with pytest.raises(ValueError, match="must match"):
        index.update(xs_updated=x[:3], updated_indices=[1, 2])
    with pytest.warns(UserWarning, match="will be ignored"):
        index.update(updated_indices=[1, 2])  # nothing to do: graph rebuilt from its own warm start
    idx, _ = index.neighbor_graph
    ti, _ = O.brute_force_knn(x, 8, "euclidean")
    assert O.recall(ti, idx) > 0.97
    index.update(xs_fresh=x[:50] + 0.01)
    assert index.neighbor_graph[0].shape == (650, 8)


@pytest.mark.parametrize("k,mc", [(40, None), (64, None), (20, 50), (40, 100), (100, 128)])
def test_wide_candidate_lists_against_oracle(k, mc):
    """max_candidates 33..64 (k_local_join_w<64,...>) and 65..128 (the same kernel over blocks of the lists): recall parity with
    the CPU oracle on the same inputs."""
    x = clustered(6000, 24, 8, 30, seed=9)
    idx, _ = NNDescent(x, "euclidean", n_neighbors=k, max_candidates=mc, random_state=7)._neighbor_graph
    oidx, _ = O.build_index(x, "euclidean", n_neighbors=k, max_candidates=mc, random_state=7, n_threads=8, kind="fast")
    _parity(x, "euclidean", k, idx, oidx, k_true=min(k, 20))
    for row in idx[::97]:
        assert len(set(row.tolist())) == len(row)


@pytest.mark.parametrize("tag,metric,method,prob,aggr", [("prob_euclidean", "euclidean", "standard", 0.5, 1.0),
                                                        ("prob_cosine", "cosine", "standard", 0.5, 1.0),
                                                        ("aware_euclidean", "euclidean", "degree_aware", 1.0, 2.0),
                                                        ("aware_cosine", "cosine", "degree_aware", 1.0, 2.0)])
def test_search_graph_non_default_modes_vs_reference_fixture(tag, metric, method, prob, aggr):
    """diversify_prob < 1 and diversify_method = 'degree_aware' (pynndescent_.py:386-389, 433-546, 625-726) on the
    reference-built graph of the fixture: the degree-aware pass is deterministic -> edge sets within 1 % of the
    reference's own result; the coin-flipping pass is compared by its pruning RATES (the reference's coin stream is a
    serial Tausworthe sequence, ours a counter hash), incl. the aliasing effect that the second pass prunes the
    forward matrix too."""
    from pynndescent_amd.search_graph import build_search_graph

    g = np.load(os.path.join(GOLDEN, "search_graph_modes.npz"))
    n, d, latent, ncl, seed = (int(v) for v in g[tag + "_gen"])
    x = clustered(n, d, latent, ncl, seed)
    sg, st = build_search_graph(x, g[tag + "_idx"], g[tag + "_dist"], metric, 15, diversify_prob=prob, diversify_method=method,
                                degree_prune_aggressiveness=aggr, seed=123, return_stages=True)
    ref_fwd, ref_rev, ref_final = int(g[tag + "_fwd_nnz"]), int(g[tag + "_rev_nnz"]), int(g[tag + "_indices"].shape[0])
    print(tag, "forward nnz %d (ref %d), after reverse pass %d (ref %d), final %d (ref %d)" % (
        st["forward_nnz"], ref_fwd, st["reverse_nnz"], ref_rev, st["final_nnz"], ref_final))
    if prob >= 1.0:
        assert (st["forward_rows"] == g[tag + "_fwd_rows"]).mean() > 0.995
        a = set(zip(np.repeat(np.arange(n), np.diff(sg.indptr)).tolist(), sg.indices.tolist()))
        b = set(zip(np.repeat(np.arange(n), np.diff(g[tag + "_indptr"])).tolist(), g[tag + "_indices"].tolist()))
        assert len(a ^ b) <= 0.01 * len(b), (len(a ^ b), len(b))
    else:
        assert abs(st["forward_nnz"] - ref_fwd) <= 0.03 * ref_fwd
        assert abs(st["reverse_nnz"] - ref_rev) <= 0.03 * ref_rev
        assert st["reverse_nnz"] < st["forward_nnz"]  # the second pass re-tested what the first pass's coins spared
        assert abs(st["final_nnz"] - ref_final) <= 0.03 * ref_final
    assert sg.dtype == np.uint8 and sg.diagonal().sum() == 0


def test_sqeuclidean_is_the_euclidean_build_without_the_square_root():
    """metric="sqeuclidean" (distances.py named_distances: squared_euclidean itself, no fast alternative, no correction,
    euclidean trees): the same build as "euclidean" -- same seed, same ids -- with squared distances out of neighbor_graph and
    query()."""
    x = clustered(5000, 20, 6, 25, seed=12)
    a = NNDescent(x, "euclidean", n_neighbors=12, random_state=5)
    b = NNDescent(x, "sqeuclidean", n_neighbors=12, random_state=5)
    (ia, da), (ib, db) = a.neighbor_graph, b.neighbor_graph
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_allclose(db, da.astype(np.float64) ** 2, rtol=1e-5, atol=1e-7)
    xi = x.astype(np.float64)
    np.testing.assert_allclose(db, ((xi[:, None, :] - xi[ib]) ** 2).sum(-1), rtol=1e-5, atol=1e-6)
    q = x[:200] + 0.01
    (qa, ea), (qb, eb) = a.query(q, k=5), b.query(q, k=5)
    np.testing.assert_array_equal(qa, qb)
    np.testing.assert_allclose(eb, ea.astype(np.float64) ** 2, rtol=1e-5, atol=1e-7)


def test_unsupported_sizes_are_reported_up_front():
    x = clustered(500, 8, 4, 5, seed=1)
    with pytest.raises(NotImplementedError, match="n_neighbors <= 256"):
        NNDescent(x, n_neighbors=300)
    with pytest.raises(NotImplementedError, match="max_candidates <= 128"):
        NNDescent(x, n_neighbors=10, max_candidates=200)
    with pytest.raises(NotImplementedError, match="manhattan"):
        NNDescent(x, metric="manhattan")


@pytest.mark.parametrize("metric,dist", [("euclidean", "squared_euclidean"), ("cosine", "alternative_cosine"), ("euclidean", "euclidean")])
def test_nn_descent_function_with_reference_leaf_array(metric, dist):
    """pynndescent_amd.nn_descent mirrors the reference function (pynndescent_.py:323-366), leaf_array included: fed the
    reference algorithm's own forest (oracle make_forest + rptree_leaf_array) it must reach the recall the reference's
    nn_descent reaches from those leaves (two-sided, 0.5 %)."""
    import pynndescent_amd

    n, d, k = 20000, 32, 15
    x = clustered(n, d, 8, 60, seed=21)
    rng_state, _, ts = O.draw_rng_states(11, 6)
    la = O.make_leaf_array(x, 6, O.default_leaf_size(k), ts, O.ANGULAR[metric])
    n_iters = O.default_n_iters(n)
    gi, gd = pynndescent_amd.nn_descent(x, k, rng_state, max_candidates=k, dist=dist, n_iters=n_iters, delta=0.001,
                                        rp_tree_init=True, leaf_array=la)
    oi, od = O.nn_descent(x, k, rng_state.copy(), k, metric, n_iters, 0.001, la)
    ti, td = O.brute_force_knn(x, 10, metric)
    rg, ro = O.recall(ti, gi), O.recall(ti, oi)
    print("nn_descent(%s) from the reference's leaves: GPU %.4f, oracle %.4f" % (dist, rg, ro))
    assert abs(rg - ro) <= 0.005 and rg > 0.9
    assert gi.dtype == np.int32 and gd.dtype == np.float32 and gi.shape == (n, k)
    assert np.all(np.diff(gd, axis=1) >= 0)
    if dist == "euclidean":  # true distances on return
        truth = np.sqrt(((x[:50, None, :].astype(np.float64) - x[gi[:50]].astype(np.float64)) ** 2).sum(-1))
        np.testing.assert_allclose(gd[:50], truth, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError, match="Invalid initial graph"):
        pynndescent_amd.nn_descent(x, k, rng_state, init_graph=(np.zeros((5, k), np.int32), np.zeros((5, k), np.float32),
                                                                np.zeros((5, k), np.uint8)))
    # a heap triple of the right shape continues from there (no forest, no random fill)
    hi, hd, hf = O.init_rp_tree(x, k, metric, la)
    gi2, _ = pynndescent_amd.nn_descent(x, k, rng_state, max_candidates=k, dist=dist, n_iters=n_iters, init_graph=(hi, hd, hf))
    assert abs(O.recall(ti, gi2) - ro) <= 0.005


def test_more_than_64_candidates_progress_like_the_oracle():
    """max_candidates = 128 on 20 000 Gaussian points, k = 80, one tree, THREE iterations: where a build stands then depends on
    how many pairs an iteration evaluates (reference algorithm: recall@80 0.63-0.73 with 60 candidates, 0.93-0.97 with 128,
    depending on the seed) -- a join that lost a block of the candidate lists would fall back towards the 60-candidate figure.
    (tests/test_gpu_kernels.py counts the pairs exactly.)"""
    n, k = 20000, 80
    x = np.random.RandomState(7).normal(0, 1, (n, 32)).astype(np.float32)
    rows = np.arange(0, n, 13)
    ti, _ = O.brute_force_knn(x, k, "euclidean", rows=rows, kind="fast")
    rec = {}
    for mc in (60, 128):
        gi, _ = NNDescent(x, "euclidean", n_neighbors=k, n_trees=1, max_candidates=mc, n_iters=3, random_state=3)._neighbor_graph
        oi, _ = O.build_index(x, "euclidean", n_neighbors=k, n_trees=1, max_candidates=mc, n_iters=3, random_state=3, n_threads=8, kind="fast")
        rec[mc] = (O.recall(ti, gi[rows]), O.recall(ti, oi[rows]))
        print("max_candidates %d, 3 iterations: recall@%d GPU %.4f oracle %.4f" % (mc, k, rec[mc][0], rec[mc][1]))
    assert rec[128][0] >= rec[128][1] - 0.08 and rec[128][0] >= rec[60][0] + 0.1


def test_wide_rows_on_unclustered_data_converge_like_the_oracle():
    """k = 160 on 20 000 Gaussian points in 32 dimensions, ONE tree: the start is poor (recall@k 0.08 after one iteration of the
    reference algorithm) and a row takes far more than 64 updates on the way -- more than the 64 proposal slots of a row hold
    per pass, so the device build may need more passes than the reference; where it stops it must be as good (0.5 %)."""
    n, k = 20000, 160
    x = np.random.RandomState(5).normal(0, 1, (n, 32)).astype(np.float32)
    rows = np.arange(0, n, 13)
    ti, _ = O.brute_force_knn(x, k, "euclidean", rows=rows, kind="fast")
    index = NNDescent(x, "euclidean", n_neighbors=k, n_trees=1, random_state=3)
    idx, dist = index._neighbor_graph
    check_graph_invariants(x, "euclidean", idx, dist, tol=2e-4, name="wide-hard")
    oi, _ = O.build_index(x, "euclidean", n_neighbors=k, n_trees=1, random_state=3, n_threads=8, kind="fast")
    rg, ro = O.recall(ti, idx[rows]), O.recall(ti, oi[rows])
    i3, _ = NNDescent(x, "euclidean", n_neighbors=k, n_trees=1, random_state=3, n_iters=3)._neighbor_graph
    o3, _ = O.build_index(x, "euclidean", n_neighbors=k, n_trees=1, n_iters=3, random_state=3, n_threads=8, kind="fast")
    print("k=160 gaussian: recall@k GPU %.4f (%d iterations) oracle %.4f; after 3 iterations GPU %.4f oracle %.4f" % (
        rg, index._build_stats["n_iters_run"], ro, O.recall(ti, i3[rows]), O.recall(ti, o3[rows])))
    assert rg >= ro - 0.005


@pytest.mark.parametrize("metric,k,n_trees", [("euclidean", 100, 4), ("cosine", 80, 3), ("euclidean", 128, 2), ("euclidean", 200, 2), ("cosine", 256, 2)])
def test_wide_rows_up_to_256_neighbours(metric, k, n_trees):
    """The reference has no bound on n_neighbors (utils.py:130-158); rows above 64 entries take the LDS-merge kernels
    (merge.h nnd_merge_row_lds): same invariants, same parity bar against the reference algorithm (oracle)."""
    n, d = 12000, 24
    x = clustered(n, d, 6, 40, seed=k)
    index = NNDescent(x, metric, n_neighbors=k, n_trees=n_trees, random_state=3)
    idx, dist = index._neighbor_graph
    assert idx.shape == (n, k) and (idx >= 0).all()
    check_graph_invariants(x, metric, idx, dist, tol=2e-4, name="wide")
    oi, od = O.build_index(x, metric, n_neighbors=k, n_trees=n_trees, random_state=3, n_threads=8, kind="fast")
    rows = np.arange(0, n, 7)
    ti, _ = O.brute_force_knn(x, k, metric, rows=rows, kind="fast")
    rg, ro = O.recall(ti, idx[rows]), O.recall(ti, oi[rows])
    print("k=%d %s: recall@k GPU %.4f oracle %.4f, %d iterations" % (k, metric, rg, ro, index._build_stats["n_iters_run"]))
    assert abs(rg - ro) <= 0.005
    # an init graph as wide as the rows, and the update() warm start
    index2 = NNDescent(x, metric, n_neighbors=k, init_graph=idx, init_dist=dist, random_state=3, n_iters=2)
    assert O.recall(ti, index2._neighbor_graph[0][rows]) >= rg - 0.005
    # prepare() / query() on the wide graph: the pruning pass (rows through LDS above 64 entries, prune.hip) against the
    # reference algorithm's pass on the SAME graph (oracle), then queries answered from it
    from pynndescent_amd.search_graph import build_search_graph

    sg = build_search_graph(x, idx, dist, metric, k)
    osg = O.search_graph(x, idx, dist, metric, k)
    ka = np.repeat(np.arange(n, dtype=np.int64), np.diff(sg.indptr)) * n + sg.indices
    kb = np.repeat(np.arange(n, dtype=np.int64), np.diff(osg.indptr)) * n + osg.indices
    sym = np.setxor1d(ka, kb).shape[0]
    print("search graph nnz gpu %d oracle %d, symmetric difference %d" % (sg.nnz, osg.nnz, sym))
    assert sym <= 0.01 * osg.nnz and np.diff(sg.indptr).max() <= int(np.round(1.5 * k)) + 1
    index.prepare()
    q = x[rows[:300]] + 0.01
    qi, qd = index.query(q, k=10, epsilon=0.2)
    tq, _ = O.brute_force_knn(np.vstack([x, q]), 330, metric, rows=np.arange(n, n + 300), kind="fast")  # (the other queries are points of that set too)
    tq = np.array([[v for v in row if v < n][:10] for row in tq])
    assert O.recall(tq, qi) >= 0.9, O.recall(tq, qi)
    with pytest.raises(NotImplementedError, match="n_neighbors <= 256"):
        NNDescent(x, metric, n_neighbors=257)


def test_result_arrays_come_from_the_pinned_pool_and_are_recycled():
    """Round 6 (include/pynnd_amd.h nnd_host_alloc, _capi.HostPool): the graph of a build lands in pinned host buffers that return
    to the pool when the last numpy view of them dies; arrays handed to the caller are ordinary writable numpy arrays, two
    indexes alive at the same time never share a buffer, and a build into pool memory equals a build into numpy memory."""
    import gc

    from pynndescent_amd import _capi

    n, k = 90_000, 15  # 5.4 MB per array: above the pool's 4 MB floor
    x = clustered(n, 32, 8, 64, seed=4)
    a = NNDescent(x, "euclidean", n_neighbors=k, n_trees=4, random_state=5)
    ia, da = a._neighbor_graph
    assert not ia.flags.owndata and ia.flags.writeable and ia.flags.c_contiguous  # a view of a pool buffer
    b = NNDescent(x, "euclidean", n_neighbors=k, n_trees=4, random_state=5)
    ib, db = b._neighbor_graph
    assert ia.ctypes.data != ib.ctypes.data and da.ctypes.data != db.ctypes.data
    np.testing.assert_array_equal(ia, ib)  # same seed, same graph
    np.testing.assert_array_equal(da, db)
    g_idx, g_dist = a.neighbor_graph  # the copies come from the pool too
    assert g_idx.ctypes.data != ia.ctypes.data and np.array_equal(g_idx, ia)
    np.testing.assert_array_equal(g_dist, np.sqrt(da))
    addr = {ib.ctypes.data, db.ctypes.data}
    del b, ib, db
    gc.collect()
    c = NNDescent(x, "euclidean", n_neighbors=k, n_trees=4, random_state=5)
    ic, dc = c._neighbor_graph
    assert {ic.ctypes.data, dc.ctypes.data} & addr, "the released buffers were not reused"
    np.testing.assert_array_equal(ic, ia)  # ... and `a`'s arrays were not touched by the reuse
    _capi.host_pool.trim()  # (idle buffers go back to the runtime; buffers in use are untouched)
    np.testing.assert_array_equal(ic, ia)
