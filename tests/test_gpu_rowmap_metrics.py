"""spearmanr and haversine on a real MI355X: the two row-map kernels (csrc/rowmap.hip) against their numpy models -- the ranks
bit for bit, the sphere rows within one float32 ulp --, the seam to the base metric's path to the bit (builds, tensor builds,
queries in every form, update, exact_knn, recall, pickling), and the handed-out haversine distances against the float64 formula
under the derived bound of DESIGN.md "Row maps"."""
import pickle

import numpy as np
import pytest

import pynndescent_amd
from pynndescent_amd import NNDescent, _capi, row_map
from tests import rowmap_util as RU

pytestmark = pytest.mark.gpu

K = 10
RANK, SPHERE = _capi.NND_ROWMAP_RANK, _capi.NND_ROWMAP_SPHERE


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _same_ranks(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(_bits(got), _bits(want))


# ---------------------------------------------------------------------------------------------------- 1. the rank kernel
@pytest.mark.parametrize("n,d", [(257, 1), (300, 2), (1000, 37), (513, 64), (200, 130), (64, 1024), (64, 1025), (5, 2048), (8, 4100),
                                 (4, row_map.RANK_MAX_DIM)])
def test_rank_kernel_equals_the_model_bit_for_bit(n, d):
    """Through the ABI entry, rows with a stride of d + 3 whose padding holds NaN (never read): values from six integers (ties
    everywhere), row 1 constant, row 2 of -0.0 / 0.0; both sides of the one-wave bound (1024 / 1025), a power of two in the sorting
    form (2048: no padding keys), both sides of the sort's small and large key buffers (4100), and the widest row accepted.  Row 5
    alone equals row 5 of the batch (n allowing)."""
    x = RU.tied_rows(n, d, seed=d)
    padded = np.full((n, d + 3), np.nan, np.float32)
    padded[:, :d] = x
    got = _capi.map_rows_host(RANK, None, padded, dim=d)
    _same_ranks(got, RU.model_ranks(x))
    _same_ranks(_capi.map_rows_host(RANK, None, x), got)  # (stride d: the same rows)
    r = min(5, n - 1)
    _same_ranks(_capi.map_rows_host(RANK, None, padded[r:r + 1], dim=d), got[r:r + 1])
    if d > 1:  # distinct values as well: a permutation's ranks are 1 .. d
        perm = np.stack([np.random.RandomState(s).permutation(d) for s in range(3)]).astype(np.float32) - d / 2
        _same_ranks(_capi.map_rows_host(RANK, None, perm), RU.model_ranks(perm))


def test_rank_entry_refuses_what_it_does_not_take():
    wide = np.zeros((2, row_map.RANK_MAX_DIM + 1), np.float32)
    with pytest.raises(_capi.NNDError, match="bad kind, width or stride"):
        _capi.map_rows_host(RANK, None, wide)
    with pytest.raises(_capi.NNDError, match="bad kind, width or stride"):
        _capi.map_rows_host(SPHERE, np.zeros(3, np.float32), np.zeros((2, 3), np.float32))


# ---------------------------------------------------------------------------------------------------- 2. the sphere kernel
def test_sphere_kernel_within_one_ulp_of_the_float64_model():
    x = RU.latlon_rows(1000, seed=3)
    x[0], x[1] = (np.pi / 2, 0.3), (-np.pi / 2, -1.0)
    x[2], x[3] = (0.2, np.pi), (0.2, -np.pi)
    x[10:20, 1] = x[20:30, 1] + np.float32(2 * np.pi)
    x[10:20, 0] = x[20:30, 0]
    x[40:50] = x[30:40]  # duplicates
    for shift in (RU.sphere_shift(x), np.zeros(3, np.float32), RU.sphere_shift(RU.latlon_rows(500, 4, region=(0.7, 2.1, 0.05)))):
        padded = np.full((1000, 5), np.nan, np.float32)
        padded[:, :2] = x
        got = _capi.map_rows_host(SPHERE, shift, padded, dim=2)
        assert got.shape == (1000, 3) and got.dtype == np.float32
        want = RU.model_sphere(x, shift)
        # device and host double sin / cos may differ in their last bit before the one rounding to float32: at most 1 ulp
        ulp = np.spacing(np.abs(want)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
        print("sphere rows: %d of %d components differ from the host model" % (int((got != want).sum()), want.size))
        np.testing.assert_array_equal(_bits(got[40:50]), _bits(got[30:40]))
        np.testing.assert_array_equal(_bits(_capi.map_rows_host(SPHERE, shift, x)), _bits(got))
        np.testing.assert_array_equal(_bits(_capi.map_rows_host(SPHERE, shift, x[5:6])), _bits(got[5:6]))


# ---------------------------------------------------------------------------------------------------- shared inputs and builds
class _Case:
    """One metric's point set, its mapped rows (from the kernel) and the two host builds that every test compares."""

    def __init__(self, metric):
        self.metric = metric
        if metric == "spearmanr":
            full = RU.decimal_rows(3400, 24, seed=31)
            self.n, self.base_metric, self.query_base_metric = 3000, "correlation", "correlation"
        else:
            full = RU.latlon_rows(4400, seed=32)
            full[1000:2000] = RU.latlon_rows(1000, seed=33, region=(0.7, 2.1, 0.05))
            full[50:60] = full[40:50]  # duplicates
            self.n, self.base_metric, self.query_base_metric = 4000, "euclidean", "sqeuclidean"
        self.x, self.q, self.fresh = full[:self.n], full[self.n:self.n + 200], full[self.n + 200:]
        self.index = NNDescent(self.x, metric=metric, n_neighbors=K, random_state=11)
        self.map = self.index._linear_map
        self.tx, self.tq, self.tfresh = (self.mapped(a) for a in (self.x, self.q, self.fresh))
        self.base = NNDescent(self.tx, metric=self.base_metric, n_neighbors=K, random_state=11)

    def mapped(self, rows):
        return _capi.map_rows_host(self.map.kind, self.map.shift, np.ascontiguousarray(rows, np.float32))

    def corrected(self, kernel_dist):
        return self.index._distance_correction(np.asarray(kernel_dist))


_CASES = {}


@pytest.fixture(params=["spearmanr", "haversine"])
def case(request):
    if request.param not in _CASES:
        _CASES[request.param] = _Case(request.param)
    return _CASES[request.param]


def _same_answers(case, got, want_kernel, on_device=False):
    """ids equal; distances: the host correction of the base index's kernel distances -- the same bits on the host; from a tensor
    the device's correction, whose double sqrt / asin agree with numpy's within a few float64 ulp (rtol 1e-14)."""
    gi, gd = _np(got[0]), _np(got[1])
    wi, wd = _np(want_kernel[0]), case.corrected(_np(want_kernel[1]))
    np.testing.assert_array_equal(gi, wi)
    assert gd.dtype == wd.dtype
    if on_device and wd.dtype == np.float64:
        np.testing.assert_allclose(gd, wd, rtol=1e-14, atol=0)
        assert ((gd == 0) == (wd == 0)).all()
    else:
        np.testing.assert_array_equal(gd, wd)


# ---------------------------------------------------------------------------------------------------- 3. build equivalence
def test_rank_rows_of_the_build_are_the_models(case):
    if case.metric == "spearmanr":
        np.testing.assert_array_equal(_bits(case.tx), _bits(RU.model_ranks(case.x)))
    else:
        assert np.array_equal(case.map.shift, RU.sphere_shift(case.x)) and case.tx.shape == (case.n, 3)
    assert case.index.dim == case.x.shape[1] and not case.index._angular_trees
    np.testing.assert_array_equal(case.index._raw_data, case.x)  # the caller's rows
    np.testing.assert_array_equal(_bits(case.index._lin_data), _bits(case.tx))


def test_build_equals_the_base_metric_build_of_the_mapped_rows(case):
    _same_answers(case, case.index.neighbor_graph, case.base._neighbor_graph)
    idx, dist = case.index.neighbor_graph
    self_at = idx == np.arange(case.n)[:, None]
    assert self_at.any(1).mean() > 0.99 and (dist[self_at] == 0).all()  # a row's distance to itself is exactly 0
    if case.metric == "haversine":
        dup = np.arange(40, 60)
        assert (dist[dup, :2] == 0).all() and dist.dtype == np.float64
    else:
        assert dist.dtype == np.float32
        np.testing.assert_array_equal(_bits(dist), _bits(case.base.neighbor_graph[1]))


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_tensor_build_equals_the_base_metric_build(case, dtype):
    torch = pytest.importorskip("torch")
    xt = torch.from_numpy(case.x).cuda().to(getattr(torch, dtype))
    x32 = xt.float().cpu().numpy()
    index = NNDescent(xt, metric=case.metric, n_neighbors=K, random_state=11)
    m = index._linear_map
    tx = _capi.map_rows_host(m.kind, m.shift, x32)
    if case.metric == "spearmanr":
        np.testing.assert_array_equal(_bits(tx), _bits(RU.model_ranks(x32)))
    else:
        np.testing.assert_array_equal(m.shift, RU.sphere_shift(x32))
    assert index._device_raw is xt and index._device_data.dtype == torch.float32 and index.dim == case.x.shape[1]
    np.testing.assert_array_equal(_bits(_np(index._device_data)), _bits(tx))
    base = NNDescent(torch.from_numpy(tx).cuda(), metric=case.base_metric, n_neighbors=K, random_state=11)
    got = index.neighbor_graph
    assert got[0].is_cuda and got[1].is_cuda
    _same_answers(case, got, base._device_graph, on_device=True)
    if dtype == "float32":  # the host build of the same rows: the same graph
        np.testing.assert_array_equal(_np(got[0]), case.index._neighbor_graph[0])
    tq = _capi.map_rows_host(m.kind, m.shift, torch.from_numpy(case.q).to(xt.dtype).float().numpy())
    qb = base if case.query_base_metric == case.base_metric else NNDescent(torch.from_numpy(tx).cuda(), metric=case.query_base_metric,
                                                                           n_neighbors=K, random_state=11)
    got = index.query(torch.from_numpy(case.q).cuda().to(xt.dtype), k=K)
    assert got[0].is_cuda and got[1].is_cuda
    _same_answers(case, got, qb.query(torch.from_numpy(tq).cuda(), k=K), on_device=True)
    np.testing.assert_array_equal(index._raw_data[np.argsort(index._vertex_order)], x32)  # the mirror of the caller's rows
    assert 0.0 < index.recall(k=K, n_rows=200, random_state=3) <= 1.0


# ---------------------------------------------------------------------------------------------------- 4. haversine accuracy
def test_haversine_distances_within_the_derived_bound():
    """Against the float64 haversine formula on the float32 inputs: |err| <= 4e-7 * M / cos(theta / 2) rad for theta <= 3.0, M the
    largest component magnitude of the shifted rows (derived in DESIGN.md "Row maps", not measured): the build's neighbours, and
    2000 pairs of random rows (a 40 x 50 exact search, every pair handed out)."""
    case = _CASES.get("haversine") or _CASES.setdefault("haversine", _Case("haversine"))
    idx, dist = case.index.neighbor_graph
    m_abs = float(np.abs(case.tx).max())
    want = RU.haversine64(case.x[:, None, :], case.x[idx])
    ratio = np.abs(dist - want) / RU.haversine_bound(want, m_abs)
    print("haversine neighbours: M %.3f, worst |err| %.3g rad, worst ratio to the bound %.3f" % (m_abs, np.abs(dist - want).max(), ratio.max()))
    assert want.max() <= 3.0 and ratio.max() <= 1.0
    rs = np.random.RandomState(5)
    a, b = case.x[rs.choice(case.n, 50, replace=False)], case.x[rs.choice(case.n, 40, replace=False)]
    gi, gd = pynndescent_amd.exact_knn(a, queries=b, k=50, metric="haversine")
    want = RU.haversine64(b[:, None, :], a[gi])
    keep = want <= 3.0
    m_abs = float(np.abs(RU.model_sphere(a, RU.sphere_shift(a))).max())
    ratio = np.abs(gd - want)[keep] / RU.haversine_bound(want[keep], m_abs)
    print("haversine random pairs: %d with theta <= 3, M %.3f, worst |err| %.3g rad, worst ratio to the bound %.3f"
          % (int(keep.sum()), m_abs, np.abs(gd - want)[keep].max(), ratio.max()))
    assert keep.sum() > 1900 and ratio.max() <= 1.0
    # regional data: the error scales with the extent
    region = RU.latlon_rows(2000, seed=6, region=(0.7, 2.1, 0.01))
    gi, gd = pynndescent_amd.exact_knn(region, k=K, metric="haversine")
    want = RU.haversine64(region[:, None, :], region[gi])
    m_abs = float(np.abs(RU.model_sphere(region, RU.sphere_shift(region))).max())
    assert m_abs < 0.03 and (np.abs(gd - want) <= RU.haversine_bound(want, m_abs)).all() and np.abs(gd - want).max() < 2e-8


# ---------------------------------------------------------------------------------------------------- 5. queries
def _query_forms(case, index, base, q, tq):
    n = index._raw_data_n()
    rs = np.random.RandomState(8)
    wide, narrow = rs.rand(n) < 0.5, rs.rand(n) < 0.02
    tags = rs.randint(1, 16, n).astype(np.uint64)
    masks = rs.randint(0, 16, q.shape[0]).astype(np.uint64)
    index.set_row_tags(tags)
    base.set_row_tags(tags)
    forms = [dict(), dict(filter=wide, filter_mode="walk"), dict(filter=narrow, filter_mode="exact"),
             dict(query_tags=masks, filter_mode="walk"), dict(query_tags=masks, filter_mode="exact")]
    for kw in forms:
        got, want = index.query(q, k=K, **kw), base.query(tq, k=K, **kw)
        assert index.last_filter == base.last_filter if kw else True
        unfilled = _np(want[0]) < 0
        gi, gd = _np(got[0]), _np(got[1])
        np.testing.assert_array_equal(gi, _np(want[0]))
        assert np.isinf(gd[unfilled]).all()
        np.testing.assert_array_equal(gd[~unfilled], case.corrected(_np(want[1]))[~unfilled])


def test_queries_in_every_form_then_update_then_again(case):
    index = NNDescent(case.x, metric=case.metric, n_neighbors=K, random_state=11)
    base = NNDescent(case.tx, metric=case.query_base_metric, n_neighbors=K, random_state=11)
    _query_forms(case, index, base, case.q, case.tq)
    np.testing.assert_array_equal(index._raw_data[np.argsort(index._vertex_order)], case.x)
    with pytest.raises(ValueError, match="query_data must have shape"):
        index.query(case.tq if case.metric == "haversine" else case.q[:, :5], k=K)
    index.update(xs_fresh=case.fresh)
    base.update(xs_fresh=case.tfresh)
    np.testing.assert_array_equal(index._neighbor_graph[0], base._neighbor_graph[0])
    np.testing.assert_array_equal(_bits(index._neighbor_graph[1]), _bits(base._neighbor_graph[1]))
    assert index._raw_data.shape == (case.n + 200, case.x.shape[1])
    _query_forms(case, index, base, case.q, case.tq)
    assert 0.0 < index.recall(k=K, n_rows=200, random_state=3) <= 1.0


def test_exact_knn_and_recall(case):
    torch = pytest.importorskip("torch")
    rows = np.arange(0, case.n, 20)
    want = pynndescent_amd.exact_knn(case.tx, k=K, metric=case.query_base_metric, rows=rows)
    _same_answers(case, pynndescent_amd.exact_knn(case.x, k=K, metric=case.metric, rows=rows), want)
    got = pynndescent_amd.exact_knn(torch.from_numpy(case.x).cuda(), k=K, metric=case.metric, rows=rows)
    assert got[0].is_cuda
    _same_answers(case, got, want, on_device=True)
    want = pynndescent_amd.exact_knn(case.tx, queries=case.tq, k=K, metric=case.query_base_metric)
    _same_answers(case, pynndescent_amd.exact_knn(case.x, queries=case.q, k=K, metric=case.metric), want)
    if case.metric == "spearmanr":
        _same_answers(case, pynndescent_amd.exact_knn(case.x, k=K, metric="spearmanr", rows=rows),
                      pynndescent_amd.exact_knn(RU.model_ranks(case.x), k=K, metric="correlation", rows=rows))
    got = case.index.recall(k=K, n_rows=300, random_state=7)
    assert got == case.base.recall(k=K, n_rows=300, random_state=7) and 0.5 < got <= 1.0


# ---------------------------------------------------------------------------------------------------- 6. pickling
def test_pickle_round_trip_of_a_prepared_index(case):
    index = NNDescent(case.x, metric=case.metric, n_neighbors=K, random_state=11)
    want = index.query(case.q, k=K)
    state = pickle.dumps(index)
    clone = pickle.loads(state)
    assert "_lin_data" not in clone.__dict__ and "_device_linear" not in clone.__dict__
    assert clone._raw_data.shape[1] == case.x.shape[1] and clone._linear_map.kind == case.map.kind
    got = clone.query(case.q, k=K)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    for a, b in zip(clone.neighbor_graph, index.neighbor_graph):
        np.testing.assert_array_equal(a, b)
