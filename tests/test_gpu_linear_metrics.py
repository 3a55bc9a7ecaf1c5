"""seuclidean / wminkowski (p = 2) / mahalanobis / minkowski (p = 2) on a real MI355X: the transform kernel (csrc/linear.hip)
against float64 numpy under a derived bound, the seam to the euclidean path to the bit, builds and queries against the
reference's own results (tests/golden/metric_linear.npz, tests/golden/make_golden_linear.py), duplicates and a zero weight,
and every other path of the class (tensor input, update, pickling, the two prepare paths, exact_knn, recall)."""
import os
import pickle

import numpy as np
import pytest

import pynndescent_amd
from pynndescent_amd import NNDescent, _capi, linear_map
from tests import exact_util as XU
from tests import linear_util as LU
from tests import metric_util as MU

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_linear.npz")
K = 10


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _same_graph(got, want):
    gi, gd = (_np(a) for a in got)
    wi, wd = (_np(a) for a in want)
    np.testing.assert_array_equal(gi, wi)
    assert gd.dtype == wd.dtype == np.float32
    np.testing.assert_array_equal(_bits(gd), _bits(wd))


# ---------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("d", [1, 3, 13, 16, 17, 33, 128, 130, 260])
def test_kernel_against_float64(d):
    """Dense and diagonal form at n in {1, 63, 64, 65, 257}: one row, a tile minus / exactly / plus one row, several workgroups;
    d below, at and across the K block (32), the column chunk (128) and not a multiple of 4 (the scalar staging path).  Rows on
    an offset of 1e3 with unit spread; the bound is ``linear_util.transform_bound`` (derived there, not measured).  The same row
    at positions 0, 63, 64 and n - 1 gives identical bits, and so does a second run."""
    rs = np.random.RandomState(100 + d)
    a64 = rs.standard_normal((d, d)) / np.sqrt(d)
    s64 = 0.5 + rs.rand(d)
    worst = 0.0
    for n in (1, 63, 64, 65, 257):
        x = (1e3 + rs.standard_normal((n, d))).astype(np.float32)
        for pos in (0, 63, 64, n - 1):
            if pos < n:
                x[pos] = x[0]
        c = linear_map.shift_of(x)
        for kind, m64 in ((_capi.NND_LINEAR_DENSE, a64), (_capi.NND_LINEAR_DIAGONAL, s64)):
            m32 = m64.astype(np.float32)
            y = _capi.linear_rows_host(kind, m32, c, x)
            assert y.shape == (n, d) and y.dtype == np.float32
            truth, bound = LU.transform_f64(kind, m64, c, x), LU.transform_bound(kind, m64, c, x)
            err = np.abs(y.astype(np.float64) - truth)
            worst = max(worst, float((err / np.maximum(bound, np.finfo(np.float64).tiny)).max()))
            assert (err <= bound).all(), "n %d d %d kind %d: error / bound %.3f" % (n, d, kind, (err / bound).max())
            for pos in (63, 64, n - 1):
                if pos < n:
                    np.testing.assert_array_equal(_bits(y[pos]), _bits(y[0]))
            np.testing.assert_array_equal(_bits(_capi.linear_rows_host(kind, m32, c, x)), _bits(y))
            # a row does not depend on n: alone it gives what it gave in the batch
            np.testing.assert_array_equal(_bits(_capi.linear_rows_host(kind, m32, c, x[n - 1:])), _bits(y[n - 1:]))
    print("d %d: worst error / bound %.3f" % (d, worst))


# ---------------------------------------------------------------------------------------------------- 2. the seam
def _seam_case(n=3000, d=13, seed=21):
    rs = np.random.RandomState(seed)
    x = (20.0 + rs.standard_normal((n + 100, d)) * (0.5 + rs.rand(d))).astype(np.float32)
    b = rs.standard_normal((d, d))
    kwds = {"mahalanobis": {"VI": b @ b.T / d + 0.3 * np.eye(d)}, "seuclidean": {"V": x[:n].astype(np.float64).var(0)},
            "wminkowski": {"w": 0.2 + rs.rand(d), "p": 2}}
    return x[:n], x[n:], kwds


def _transformed(metric, kwds, train, *others):
    """The transform's own output for the rows, fetched through the ABI, with the map an index of ``train`` fixes."""
    lin = linear_map.parse_metric_kwds(metric, kwds, train.shape[1])
    lin = lin._replace(shift=linear_map.shift_of(train))
    return [_capi.linear_rows_host(lin.kind, lin.a, lin.shift, np.ascontiguousarray(r, np.float32)) for r in (train,) + others]


@pytest.mark.parametrize("metric", LU.METRICS)
def test_seam_to_the_euclidean_path_is_bit_exact(metric):
    x, q, kwds = _seam_case()
    t, tq = _transformed(metric, kwds[metric], x, q)
    index = NNDescent(x, metric=metric, metric_kwds=kwds[metric], n_neighbors=K, random_state=9)
    plain = NNDescent(t, metric="euclidean", n_neighbors=K, random_state=9)
    np.testing.assert_array_equal(index._raw_data, x)  # the index keeps the caller's rows
    _same_graph(index.neighbor_graph, plain.neighbor_graph)
    _same_graph(index.query(q, k=K), plain.query(tq, k=K))


def test_seam_for_a_float16_tensor():
    torch = pytest.importorskip("torch")
    x, q, kwds = _seam_case()
    x16, q16 = torch.from_numpy(x).half().cuda(), torch.from_numpy(q).half().cuda()
    t, tq = _transformed("mahalanobis", kwds["mahalanobis"], x16.float().cpu().numpy(), q16.float().cpu().numpy())
    index = NNDescent(x16, metric="mahalanobis", metric_kwds=kwds["mahalanobis"], n_neighbors=K, random_state=9)
    plain = NNDescent(torch.from_numpy(t).cuda(), metric="euclidean", n_neighbors=K, random_state=9)
    assert index._device_raw is x16 and index._device_data.dtype == torch.float32
    np.testing.assert_array_equal(_bits(_np(index._device_data)), _bits(t))
    _same_graph(index.neighbor_graph, plain.neighbor_graph)
    got = index.query(q16, k=K)
    assert got[0].is_cuda and got[1].is_cuda
    _same_graph(got, plain.query(torch.from_numpy(tq).cuda(), k=K))
    # the mirror of the caller's rows (prepared by the query: in the leaf order)
    np.testing.assert_array_equal(index._raw_data[np.argsort(index._vertex_order)], x16.float().cpu().numpy())


# ---------------------------------------------------------------------------------------------------- 3. the reference fixture
def _distance_bound(metric, kwds, a_rows, b_rows, truth, c):
    """|handed out - truth| <= |e(x)|_2 + |e(y)|_2 + 2^-23 truth, e the transform's componentwise bound (test 1)."""
    lin = linear_map.parse_metric_kwds(metric, kwds, a_rows.shape[-1])
    m64 = {"mahalanobis": lambda: linear_map.mahalanobis_factor(kwds["vinv"]), "seuclidean": lambda: 1.0 / np.sqrt(kwds["sigma"]),
           "wminkowski": lambda: np.sqrt(kwds["w"])}[metric]()
    ea = np.linalg.norm(LU.transform_bound(lin.kind, m64, c, a_rows.reshape(-1, a_rows.shape[-1])), axis=1).reshape(a_rows.shape[:-1])
    eb = np.linalg.norm(LU.transform_bound(lin.kind, m64, c, b_rows.reshape(-1, b_rows.shape[-1])), axis=1).reshape(b_rows.shape[:-1])
    return ea + eb + 2.0 ** -23 * truth


def _check_rows(idx, dist):
    assert (idx >= 0).all()
    assert (np.diff(dist, axis=1) >= 0).all(), "rows ascending"
    s = np.sort(idx, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all(), "ids unique"


@pytest.mark.parametrize("metric", LU.METRICS)
def test_build_and_query_against_reference_fixture(metric):
    """Mean recall@10 over the three seeds within 0.01 of the reference's and query recall >= the reference's - 0.02 (the margins
    of tests/test_gpu_metrics.py); every distance handed out within the derived bound of the float64 formula on the raw rows."""
    f = np.load(GOLDEN)
    x, q = LU.fixture_data()
    kwds = LU.fixture_kwds(x)[metric]
    c = linear_map.shift_of(x)
    truth = LU.brute_knn(metric, kwds, x, k=K)
    rec_gpu, rec_ref = [], []
    first = None
    for s in f["seeds"]:
        index = NNDescent(x, metric=metric, metric_kwds=kwds, n_neighbors=K, random_state=int(s))
        idx, dist = index.neighbor_graph
        assert idx.shape == (x.shape[0], K) and dist.dtype == np.float32
        _check_rows(idx, dist)
        rec_gpu.append(MU.recall(truth, idx))
        rec_ref.append(float(f["%s_recall_%d" % (metric, s)]))
        true = LU.true_dist_pairs(metric, kwds, x[:, None, :], x[idx])
        gap = np.abs(dist.astype(np.float64) - true)
        bound = _distance_bound(metric, kwds, np.broadcast_to(x[:, None, :], x[idx].shape), x[idx], true, c)
        print("%s seed %d: recall gpu %.4f reference %.4f; worst distance gap / bound %.3f"
              % (metric, s, rec_gpu[-1], rec_ref[-1], float((gap / np.maximum(bound, 1e-300)).max())))
        assert (gap <= bound).all()
        first = index if first is None else first
    print("%s: mean recall gpu %.4f reference %.4f" % (metric, np.mean(rec_gpu), np.mean(rec_ref)))
    assert abs(np.mean(rec_gpu) - np.mean(rec_ref)) <= 0.01
    qi, qd = first.query(q, k=K)
    _check_rows(qi, qd)
    q_truth = LU.brute_knn(metric, kwds, x, q, k=K)
    r_gpu, r_ref = MU.recall(q_truth, qi), float(f[metric + "_q_recall"])
    assert abs(MU.recall(q_truth, f[metric + "_q_idx"]) - r_ref) < 1e-12  # the fixture and this file agree on the truth
    true = LU.true_dist_pairs(metric, kwds, q[:, None, :], x[qi])
    gap = np.abs(qd.astype(np.float64) - true)
    bound = _distance_bound(metric, kwds, np.broadcast_to(q[:, None, :], x[qi].shape), x[qi], true, c)
    print("%s queries: recall@10 gpu %.4f reference %.4f; worst distance gap / bound %.3f"
          % (metric, r_gpu, r_ref, float((gap / np.maximum(bound, 1e-300)).max())))
    assert r_gpu >= r_ref - 0.02
    assert (gap <= bound).all()


# ---------------------------------------------------------------------------------------------------- 4. duplicates, zero weight
@pytest.mark.parametrize("metric", LU.METRICS)
def test_duplicates_are_at_distance_exactly_zero(metric):
    x, _, kwds = _seam_case()
    x = x.copy()
    dup = np.random.RandomState(4).choice(x.shape[0], 50, replace=False)
    x[dup] = x[dup[0]]
    idx, dist = NNDescent(x, metric=metric, metric_kwds=kwds[metric], n_neighbors=K, random_state=2).neighbor_graph
    assert np.isin(idx[dup], dup).all(), "duplicates are each other's neighbours"
    np.testing.assert_array_equal(_bits(dist[dup]), np.zeros((50, K), np.uint32))  # +0.0, every one


def test_a_zero_weight_column_does_not_influence_the_graph():
    """w = 0 on a column: the graph is the one built without that column, to the bit.  The column is the LAST one: the kernels
    pad rows with zeros behind column d, so the transformed rows of the two builds are the same padded rows; a zero column in
    the middle would move the columns behind it and with them the order of the float32 sums."""
    x, q, kwds = _seam_case()
    w = kwds["wminkowski"]["w"].copy()
    w[-1] = 0.0
    full = NNDescent(x, metric="wminkowski", metric_kwds={"w": w}, n_neighbors=K, random_state=6)
    less = NNDescent(np.ascontiguousarray(x[:, :-1]), metric="wminkowski", metric_kwds={"w": w[:-1]}, n_neighbors=K, random_state=6)
    _same_graph(full.neighbor_graph, less.neighbor_graph)
    _same_graph(full.query(q, k=K), less.query(np.ascontiguousarray(q[:, :-1]), k=K))


# ---------------------------------------------------------------------------------------------------- 5. the other paths
@pytest.mark.parametrize("metric", ["mahalanobis", "seuclidean"])
def test_host_build_and_tensor_build_are_identical(metric):
    torch = pytest.importorskip("torch")
    x, q, kwds = _seam_case()
    host = NNDescent(x, metric=metric, metric_kwds=kwds[metric], n_neighbors=K, random_state=3)
    dev = NNDescent(torch.from_numpy(x).cuda(), metric=metric, metric_kwds=kwds[metric], n_neighbors=K, random_state=3)
    for got, want in zip(dev._linear_map[1:], host._linear_map[1:]):  # the same (A, c), to the bit
        np.testing.assert_array_equal(_bits(got), _bits(want))
    _same_graph(dev.neighbor_graph, host.neighbor_graph)
    _same_graph(dev.query(torch.from_numpy(q).cuda(), k=K), host.query(q, k=K))
    _same_graph(dev.query(q, k=K), host.query(q, k=K))
    np.testing.assert_array_equal(dev._raw_data, host._raw_data)  # (both prepared: the caller's rows in the leaf order)


@pytest.mark.parametrize("on_device", [False, True])
def test_update_goes_through_the_same_map(on_device):
    """update() with fresh and updated rows: identical to the euclidean index of the transformed rows (transformed with the c
    fixed at the first build) taking the same update."""
    torch = pytest.importorskip("torch")
    x, q, kwds = _seam_case()
    n0, upd = 2500, [5, 77, 1200]
    new_rows = x[upd] + np.float32(0.25)
    t_old, t_fresh, t_upd, tq = _transformed("mahalanobis", kwds["mahalanobis"], x[:n0], x[n0:], new_rows, q)
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if on_device else (lambda a: a)
    index = NNDescent(put(x[:n0]), metric="mahalanobis", metric_kwds=kwds["mahalanobis"], n_neighbors=K, random_state=5)
    plain = NNDescent(put(t_old), metric="euclidean", n_neighbors=K, random_state=5)
    index.update(xs_fresh=put(x[n0:]), xs_updated=put(new_rows), updated_indices=upd)
    plain.update(xs_fresh=put(t_fresh), xs_updated=put(t_upd), updated_indices=upd)
    _same_graph(index.neighbor_graph, plain.neighbor_graph)
    _same_graph(index.query(q, k=K), plain.query(tq, k=K))
    want = x.copy()
    want[upd] = new_rows
    raw = index._raw_data[np.argsort(index._vertex_order)]
    np.testing.assert_array_equal(raw, want)


@pytest.mark.parametrize("metric", LU.METRICS)
def test_pickle_then_query(metric):
    x, q, kwds = _seam_case()
    index = NNDescent(x, metric=metric, metric_kwds=kwds[metric], n_neighbors=K, random_state=8)
    want = index.query(q, k=K)
    clone = pickle.loads(pickle.dumps(index))
    assert "_lin_data" not in clone.__dict__
    _same_graph(clone.query(q, k=K), want)
    _same_graph(clone.neighbor_graph, index.neighbor_graph)


def test_prepare_host_path_and_device_path_are_identical():
    torch = pytest.importorskip("torch")
    x, q, kwds = _seam_case()
    xt = torch.from_numpy(x).cuda()
    on_device = NNDescent(xt, metric="mahalanobis", metric_kwds=kwds["mahalanobis"], n_neighbors=K, random_state=3)
    through_host = NNDescent(xt, metric="mahalanobis", metric_kwds=kwds["mahalanobis"], n_neighbors=K, random_state=3)
    through_host._host_prepare = True
    on_device.prepare()
    through_host.prepare()
    assert "_device_search_graph" in on_device.__dict__ and "_device_search_graph" not in through_host.__dict__
    np.testing.assert_array_equal(on_device._vertex_order, through_host._vertex_order)
    np.testing.assert_array_equal(on_device._raw_data, through_host._raw_data)
    np.testing.assert_array_equal(_bits(on_device._lin_data), _bits(through_host._lin_data))
    _same_graph(on_device.query(q, k=K), through_host.query(q, k=K))


@pytest.mark.parametrize("metric", LU.METRICS)
def test_exact_knn_and_recall_against_float64_on_the_transformed_rows(metric):
    """The exactness claim: (float64 distance, id) on the float32 transformed rows -- under the comparison rule of the exact
    search's own tests (tests/exact_util.py: position by position, exempt only where the float64 truth is a near-tie)."""
    torch = pytest.importorskip("torch")
    x, q, kwds = _seam_case()
    t, tq = _transformed(metric, kwds[metric], x, q)
    rows = np.arange(0, x.shape[0], 10)
    truth = XU.matrix_truth("euclidean", t, t[rows], K)
    for data in (x, torch.from_numpy(x).cuda()):
        gi, gd = pynndescent_amd.exact_knn(data, k=K, metric=metric, rows=rows, metric_kwds=kwds[metric])
        gi, gd = _np(gi), _np(gd)
        assert gd.dtype == np.float32
        XU.check_exact("%s rows" % metric, "euclidean", t, t[rows], gi, gd.astype(np.float64) ** 2, truth, K)
    gi, gd = pynndescent_amd.exact_knn(x, queries=q, k=K, metric=metric, metric_kwds=kwds[metric])
    XU.check_exact("%s queries" % metric, "euclidean", t, tq, gi, gd.astype(np.float64) ** 2, XU.matrix_truth("euclidean", t, tq, K), K)
    # recall(): the share of the true neighbours found in the graph's rows, counted here from the float64 truth
    sample = NNDescent._recall_rows(x.shape[0], 300, 7)
    truth = XU.matrix_truth("euclidean", t, t[sample], K)[:, :K]
    for data in (x, torch.from_numpy(x).cuda()):
        index = NNDescent(data, metric=metric, metric_kwds=kwds[metric], n_neighbors=K, n_iters=1, n_trees=1, random_state=1)
        graph = _np(index.neighbor_graph[0])
        hits = sum(int(np.isin(a, b).sum()) for a, b in zip(truth, graph[sample]))
        got = index.recall(k=K, n_rows=300, random_state=7)
        print("%s recall %.4f (%s)" % (metric, got, type(data).__name__))
        assert got == hits / float(truth.size)


@pytest.mark.parametrize("kwds", [None, {}, {"p": 2}, {"p": 2.0}])
def test_minkowski_p2_is_the_euclidean_path(kwds):
    x, q, _ = _seam_case()
    index = NNDescent(x, metric="minkowski", metric_kwds=kwds, n_neighbors=K, random_state=9)
    plain = NNDescent(x, metric="euclidean", n_neighbors=K, random_state=9)
    assert index._linear_map is None
    _same_graph(index.neighbor_graph, plain.neighbor_graph)
    _same_graph(index.query(q, k=K), plain.query(q, k=K))
    gi, gd = pynndescent_amd.exact_knn(x, k=K, metric="minkowski", rows=np.arange(50), metric_kwds=kwds)
    wi, wd = pynndescent_amd.exact_knn(x, k=K, metric="euclidean", rows=np.arange(50))
    _same_graph((gi, gd), (wi, wd))
