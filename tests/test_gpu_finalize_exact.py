"""finalize on a real MI355X against its host model (tests/finalize_reference.py), bit for bit: indices and distances of
graphs loaded with init_from_graph, sqeuclidean and cosine, every k-list width class of the kernels (k <= 16: four rows per
wave; 16 < k <= 64: one row per wave) and row lengths of one lane, part of the lanes, one, two and a started third chunk
per lane."""
import numpy as np
import pytest

from tests import finalize_reference as FR
from tests.gpu_util import make_builder

pytestmark = pytest.mark.gpu

N = 37  # rows: three waves of four rows and one row more (k <= 16), ten workgroups of one row per wave (k > 16)
METRICS = {0: "euclidean", 1: "cosine"}


def _points(d, seed):
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((N, d)) * rs.uniform(0.5, 2.0, (1, d)) + 0.4).astype(np.float32)
    x[7] = x[3]    # duplicate points: the same distance from every row, the tie goes by index
    x[21] = x[3]
    return x


def _graph(k, seed):
    """-1 = empty slot; ids unique within a row"""
    rs = np.random.RandomState(seed)
    g = np.stack([rs.permutation(N)[:k] for _ in range(N)]).astype(np.int32)
    g[5] = -1                       # a row of only empty slots
    g[9, 0] = 9 if 9 not in g[9, 1:] else g[9, 0]
    for r in (0, 6, 11, 36):        # the row itself among its neighbours; row 36 is the last wave's only row
        g[r] = np.concatenate([[r], [v for v in rs.permutation(N) if v != r][:k - 1]])
    if k >= 3:
        g[2, :3] = [21, 3, 7]       # the three duplicates in one row, not in index order
        g[2, 3:] = [v for v in rs.permutation(N) if v not in (21, 3, 7)][:k - 3]
        g[12, 1::2] = -1            # rows with empty slots between and behind the entries
        g[13, k // 2:] = -1
    if k >= 2:
        g[14, 1:] = -1              # one entry
    return g


def _run(x, g, metric, k):
    b = make_builder(x, METRICS[metric], k=k, n_trees=0)
    b.init_from_graph(g)
    stored, _, _ = b.graph()
    idx, dist = b.finalize()
    b.close()
    return stored, np.array(idx, copy=True), np.array(dist, copy=True)


def _check(x, g, metric, k):
    stored, idx, dist = _run(x, g, metric, k)
    # the cases are really in the k-lists: every row holds exactly the ids it was given
    for r in range(g.shape[0]):
        assert sorted(stored[r][stored[r] >= 0].tolist()) == sorted(g[r][g[r] >= 0].tolist()), r
    want_idx, want_dist = FR.finalize_rows(x, stored, metric)
    np.testing.assert_array_equal(idx, want_idx)
    np.testing.assert_array_equal(dist.view(np.uint32), want_dist.view(np.uint32))


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("k", [1, 4, 15, 16])
@pytest.mark.parametrize("d", [4, 20, 64, 128, 132])
def test_finalize_equals_the_model(d, k, metric):
    _check(_points(d, 100 + d), _graph(k, k), metric, k)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d,k", [(20, 17), (132, 30), (128, 64)])
def test_finalize_one_row_per_wave_equals_the_model(d, k, metric):
    """16 < k <= 64: the same arithmetic in k_finalize, one, two and four rounds of sixteen neighbours"""
    rs = np.random.RandomState(k)
    x = (rs.standard_normal((80, d)) + 0.4).astype(np.float32)
    x[7] = x[3]
    g = np.stack([rs.permutation(80)[:k] for _ in range(80)]).astype(np.int32)
    g[5] = -1
    g[12, 1::2] = -1
    g[0, 0] = 0 if 0 not in g[0, 1:] else g[0, 0]
    _check(x, g, metric, k)


@pytest.mark.parametrize("k", [1, 20])
def test_finalize_keeps_the_pinned_order_where_it_shows(k):
    """Inputs on which the float32 handed back changes with the order of the fused multiply-adds inside a chunk, and with the
    pairing of the 16 lanes' sums (tests/test_finalize_reference_cpu.py shows that the model tells the orders apart)."""
    for rows in (FR.sensitive_fma_rows(), FR.sensitive_butterfly_rows()):
        d = rows.shape[1]
        x = np.zeros((24, d), np.float32)
        x[:2] = rows
        x[2:] = np.random.RandomState(d).standard_normal((22, d)).astype(np.float32)
        g = np.full((24, k), -1, np.int32)
        g[:, 0] = (np.arange(24) + 1) % 24
        g[0, 0] = 1
        stored, idx, dist = _run(x, g, 0, k)
        assert stored[0, 0] == 1
        assert dist[0, 0] == np.float32(1.0 + 2.0 ** -23)
        want_idx, want_dist = FR.finalize_rows(x, stored, 0)
        np.testing.assert_array_equal(idx, want_idx)
        np.testing.assert_array_equal(dist.view(np.uint32), want_dist.view(np.uint32))
