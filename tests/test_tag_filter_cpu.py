"""Per-query filters without a GPU: the host rules of ``set_row_tags`` / ``query(query_tags=...)`` / ``exact_knn(row_tags=...)`` --
every error before any device work -- the pickle, ``update()``, the ``auto`` rule as a pure function, and the tagged step-exact
model (tests/tag_filter_reference.py) pinned to the single-set model where every query carries the same mask."""
import os
import pickle
import types

import numpy as np
import pytest

import pynndescent_amd
from pynndescent_amd import _capi, filtered, nndescent
from tests import filter_reference as FR
from tests import search_cases as SC
from tests import tag_filter_reference as TR
from tests.test_filtered_search_cpu import D, N, Q, _FakeSearcher, _index, no_library  # noqa: F401  (no_library is a fixture)

TAGS = (np.arange(N) % 5 == 0).astype(np.uint64) | (np.uint64(1) << np.uint64(63))
MASKS = np.ones(len(Q), np.uint64)


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("bad,match", [
    (np.ones(N - 1, np.uint64), "one entry per row"),
    (np.ones(N + 1, np.int64), "one entry per row"),
    (np.ones((N, 1), np.uint64), "1-D"),
    (np.ones(N, np.int32), "dtype"),
    (np.ones(N, np.uint32), "dtype"),
    (np.ones(N, np.float64), "dtype"),
    (np.ones(N, bool), "dtype"),
])
def test_bad_row_tags_are_value_errors(no_library, bad, match):
    index = _index()
    with pytest.raises(ValueError, match=match):
        index.set_row_tags(bad)
    assert "_row_tags" not in index.__dict__ and not index._prepared


def test_row_tags_dtypes_and_removal(no_library):
    index = _index()
    signed = np.full(N, -1, np.int64)  # the bit pattern counts: every bit set, bit 63 too
    index.set_row_tags(signed)
    assert index._row_tags.dtype == np.uint64 and (index._row_tags == np.uint64(2 ** 64 - 1)).all()
    index.set_row_tags(TAGS)
    np.testing.assert_array_equal(index._row_tags, TAGS)
    index.set_row_tags(None)
    assert "_row_tags" not in index.__dict__
    with pytest.raises(ValueError, match="set_row_tags first"):
        index.query(Q, k=5, query_tags=MASKS)


class _Tensor:  # what check_words reads of a tensor before it refuses it
    is_cuda = True

    def __init__(self, index=0, dtype="torch.int64", shape=(N,)):
        self.device, self.dtype, self.shape = types.SimpleNamespace(type="cuda", index=index), dtype, shape

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        raise AssertionError("the words were read")


@pytest.mark.parametrize("tensor,match", [(_Tensor(index=1), "the index on device 0"), (_Tensor(dtype="torch.int32"), "int64 tensor"),
                                          (_Tensor(dtype="torch.uint8"), "int64 tensor"), (_Tensor(shape=(N, 1)), "1-D"),
                                          (_Tensor(shape=(N + 1,)), "one entry per row")])
def test_bad_tag_tensors_are_value_errors(no_library, tensor, match):
    index = _index()
    with pytest.raises(ValueError, match=match):
        index.set_row_tags(tensor)
    index.set_row_tags(TAGS)
    if tensor.shape == (N,):
        tensor.shape = (len(Q),)
    with pytest.raises(ValueError, match=match.replace("per row", "per query")):
        index.query(Q, k=5, query_tags=tensor)
    assert not index._prepared


@pytest.mark.parametrize("bad,match", [(np.ones(len(Q) + 1, np.uint64), "one entry per query"), (np.ones((len(Q), 1), np.uint64), "1-D"),
                                       (np.ones(len(Q), np.float32), "dtype"), (np.ones(len(Q), np.int16), "dtype")])
def test_bad_query_tags_are_value_errors_before_any_device_work(no_library, bad, match):
    index = _index()
    index.set_row_tags(TAGS)
    for mode in ("auto", "walk", "exact"):
        with pytest.raises(ValueError, match=match):
            index.query(Q, k=5, query_tags=bad, filter_mode=mode)
    assert not index._prepared


def test_query_tags_rules(no_library):
    index = _index()
    with pytest.raises(ValueError, match="set_row_tags first"):
        index.query(Q, k=5, query_tags=MASKS)
    index.set_row_tags(TAGS)
    with pytest.raises(ValueError, match="not both"):
        index.query(Q, k=5, query_tags=MASKS, filter=np.ones(N, bool))
    with pytest.raises(ValueError, match="filter_mode"):
        index.query(Q, k=5, query_tags=MASKS, filter_mode="post")
    with pytest.raises(ValueError, match="shape"):
        index.query(np.zeros((4, D + 1), np.float32), k=5, query_tags=MASKS)
    proxy = _index("proxy_inner_product")
    proxy.set_row_tags(TAGS)
    with pytest.raises(NotImplementedError, match="proxy_inner_product") as tagged:
        proxy.query(Q, k=5, query_tags=MASKS, filter_mode="exact")
    with pytest.raises(NotImplementedError) as single:
        proxy.query(Q, k=5, filter=np.ones(N, bool), filter_mode="exact")
    assert str(tagged.value) == str(single.value)  # the same text as today
    assert not index._prepared and not proxy._prepared


def test_exact_knn_takes_both_tag_arguments_or_neither(no_library):
    x = np.zeros((N, D), np.float32)
    with pytest.raises(ValueError, match="together"):
        pynndescent_amd.exact_knn(x, Q, 3, row_tags=TAGS)
    with pytest.raises(ValueError, match="together"):
        pynndescent_amd.exact_knn(x, Q, 3, query_tags=MASKS)
    with pytest.raises(ValueError, match="one entry per row"):
        pynndescent_amd.exact_knn(x, Q, 3, row_tags=TAGS[:-1], query_tags=MASKS)
    with pytest.raises(ValueError, match="one entry per query"):
        pynndescent_amd.exact_knn(x, Q, 3, row_tags=TAGS, query_tags=TAGS)
    with pytest.raises(ValueError, match="one entry per query"):  # queries=None: the masks belong to the rows themselves
        pynndescent_amd.exact_knn(x, None, 3, row_tags=TAGS, query_tags=MASKS)
    with pytest.raises(ValueError, match="dtype"):
        pynndescent_amd.exact_knn(x, Q, 3, row_tags=TAGS.astype(np.float64), query_tags=MASKS)


# ------------------------------------------------------------------------------------------------ pickle, update
def test_pickle_keeps_the_tags(no_library, monkeypatch):
    index = _index()
    index.set_row_tags(TAGS)
    monkeypatch.setattr(nndescent.NNDescent, "_init_search_graph", lambda self: None)  # (the un-prepared index's graph pass is device work)
    monkeypatch.setattr(index, "_search_forest", [], raising=False)
    again = pickle.loads(pickle.dumps(index))
    assert isinstance(again._row_tags, np.ndarray) and again._row_tags.dtype == np.uint64
    np.testing.assert_array_equal(again._row_tags, TAGS)


def test_update_clears_the_tags(no_library, monkeypatch):
    index = _index()
    index.set_row_tags(TAGS)

    def fake_build(work, *a, old_graph=None, **k):  # the rebuild is device work: the warm start comes back as the graph
        return old_graph, {}, 1

    monkeypatch.setattr(nndescent, "_build_graph", fake_build)
    index.update(xs_fresh=np.ones((3, D), np.float32))
    assert index._raw_data.shape[0] == N + 3 and "_row_tags" not in index.__dict__
    with pytest.raises(ValueError, match="set the row tags again"):
        index.query(Q, k=5, query_tags=MASKS)
    index.set_row_tags(np.ones(N + 3, np.uint64))  # ... and they can be: one entry per row of the new row set
    with pytest.raises(ValueError, match="one entry per row"):
        index.set_row_tags(TAGS)


# ------------------------------------------------------------------------------------------------ the auto rule
def test_auto_rule_on_hand_made_counts(monkeypatch):
    monkeypatch.setattr(filtered, "TAG_EXACT_MAX_ROWS", 100)
    distinct = np.array([0, 1, 2, 4, 1 << 63], np.uint64)
    counts = np.array([0, 100, 101, 0, 7])  # mask 0; at the constant; one above; a tag no row has; bit 63
    inverse = np.array([1, 0, 2, 3, 4, 1, 2, 0])
    walk, exact, empty = filtered.tag_auto_paths(inverse, distinct, counts)
    assert walk.tolist() == [2, 6] and exact.tolist() == [0, 4, 5] and empty.tolist() == [1, 3, 7]
    assert filtered.tag_mask_paths(distinct, counts).tolist() == ["empty", "exact", "walk", "empty", "exact"]
    # a metric without an exact search: what would go exact walks
    walk, exact, empty = filtered.tag_auto_paths(inverse, distinct, counts, exact_ok=False)
    assert walk.tolist() == [0, 2, 4, 5, 6] and exact.tolist() == [] and empty.tolist() == [1, 3, 7]
    # counts not taken: every non-zero mask walks, the zero mask is empty all the same
    walk, exact, empty = filtered.tag_auto_paths(inverse, distinct, None)
    assert walk.tolist() == [0, 2, 3, 4, 5, 6] and exact.tolist() == [] and empty.tolist() == [1, 7]


def test_auto_rule_with_more_than_1024_masks(monkeypatch):
    assert filtered.TAG_COUNT_MAX_MASKS == 1024
    assert filtered.tag_counts_taken(1024) and not filtered.tag_counts_taken(1025)
    monkeypatch.setattr(filtered, "TAG_EXACT_MAX_ROWS", 100)
    for n_masks, goes_exact in ((1024, True), (1025, False)):
        distinct = np.arange(n_masks, dtype=np.uint64)  # (mask 0 among them)
        counts = np.full(n_masks, 5)
        counts[0] = 0
        inverse = np.arange(n_masks)[::-1].copy()
        walk, exact, empty = filtered.tag_auto_paths(inverse, distinct, counts)  # above the bound the counts are not looked at
        assert empty.tolist() == [n_masks - 1]
        assert (len(exact), len(walk)) == ((n_masks - 1, 0) if goes_exact else (0, n_masks - 1))


class _TaggedFake(_FakeSearcher):
    def __init__(self, counts):
        super().__init__()
        self.counts = counts

    def set_tags(self, tags, order=None):
        self.calls.append(("set_tags", np.asarray(tags).copy(), np.asarray(order).copy()))

    def clear_tags(self):
        self.calls.append(("clear_tags",))

    def count_tags(self, masks):
        self.calls.append(("count_tags", np.asarray(masks).copy()))
        return np.array([self.counts[int(m)] for m in masks], np.int64)

    def query_tagged(self, form, queries, masks, k, search_k, epsilon):
        self.calls.append(("query_tagged", form, queries.shape, np.asarray(masks).copy(), k, search_k, epsilon))
        nq = queries.shape[0]
        live = (np.asarray(masks) != 0)[:, None]  # (as the kernel: a query with mask 0 does not walk)
        return (np.where(live, np.tile(np.arange(k, dtype=np.int32), (nq, 1)), np.int32(-1)),
                np.where(live, np.tile(np.arange(k, dtype=np.float32), (nq, 1)), np.float32(np.inf)))


def test_auto_splits_a_call_on_the_host(no_library, monkeypatch):
    """The host orchestration on a recording searcher: the tags go up once, the distinct masks are counted in one call, the walk
    gets the whole batch with the other queries' masks zeroed, the exact path gets its queries alone, ``last_filter`` reports."""
    index = _index()
    index._vertex_order = np.arange(N, dtype=np.int32)[::-1].copy()
    index._searcher = s = _TaggedFake({0: 0, 1: 60, 2: 5, 4: 0})
    index.set_row_tags(TAGS)
    monkeypatch.setattr(filtered, "TAG_EXACT_MAX_ROWS", 10)
    seen = []

    def fake_exact(idx, q, k, masks, on_device, host_answers=False):
        seen.append((q.shape, np.asarray(masks).copy()))
        return np.full((q.shape[0], k), 7, np.int32), np.full((q.shape[0], k), 0.5, np.float32)

    monkeypatch.setattr(filtered, "query_tagged_exact", fake_exact)
    masks = np.array([1, 2, 4, 0], np.uint64)
    ids, dist = index.query(Q, k=5, epsilon=0.25, query_tags=masks)
    assert index.last_filter == {"mode": "tags", "n_walk": 1, "n_exact": 1, "n_empty": 2, "n_masks": 4}
    assert [c[0] for c in s.calls] == ["set_tags", "count_tags", "query_tagged"]
    np.testing.assert_array_equal(s.calls[0][1], TAGS)  # in the original numbering; the library gathers through the row order
    np.testing.assert_array_equal(s.calls[0][2], index._vertex_order)
    assert s.calls[1][1].tolist() == [0, 1, 2, 4]
    assert s.calls[2][1:3] == ("float", (4, D)) and s.calls[2][3].tolist() == [1, 0, 0, 0] and s.calls[2][4:] == (5, 5, 0.25)
    assert seen[0][0] == (1, D) and seen[0][1].tolist() == [2]
    np.testing.assert_array_equal(ids[0], index._vertex_order[:5])
    assert (ids[1] == 7).all() and (dist[1] == 0.5).all()
    assert (ids[2:] == -1).all() and np.isinf(dist[2:]).all()
    # a second call does not send the tags again; new tags drop the searcher's copy
    index.query(Q, k=5, query_tags=masks, filter_mode="walk")
    assert [c[0] for c in s.calls[3:]] == ["query_tagged"] and s.calls[3][3].tolist() == [1, 2, 4, 0]
    assert index.last_filter == {"mode": "tags", "n_walk": 3, "n_exact": 0, "n_empty": 1, "n_masks": 4}
    index.set_row_tags(TAGS)
    assert s.calls[-1] == ("clear_tags",)


# ------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("name", ["width_k10_nn10", "graph_islands_k200"])
def test_one_mask_for_all_is_the_single_set_model(name):
    """When every query carries the same mask the tagged model is ``filter_reference.reference_search`` with that one allow set."""
    c, _ = SC.get(name)
    tags = TR.case_tags(c.data.shape[0])
    for mask in (np.uint64(1), np.uint64(0b110), np.uint64(1) << np.uint64(63)):
        allowed = TR.allowed_of(tags, mask)
        want = FR.reference_search(allowed, c.data, c.indptr, c.indices, c.tree, c.metric, c.min_distance, c.n_neighbors, c.queries, c.k,
                                   c.epsilon, c.rng_state, exact=c.exact)
        got = TR.reference_search(tags, np.full(len(c.queries), mask, np.uint64), c.data, c.indptr, c.indices, c.tree, c.metric,
                                  c.min_distance, c.n_neighbors, c.queries, c.k, c.epsilon, c.rng_state, exact=c.exact)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a.ids, b.ids)
            np.testing.assert_array_equal(a.dists, b.dists)
            assert (a.V, a.L, a.F, a.ambiguous) == (b.V, b.L, b.F, b.ambiguous)


def test_model_keeps_each_query_in_its_place():
    """A mixed batch: query i's result is that of the single-set model run on the whole batch with query i's allow set."""
    c, tags, masks, res = TR.get("width_k10_nn10")
    assert len(set(masks.tolist())) >= 4 and (tags == 0).any() and ((tags >> np.uint64(63)) != 0).any()
    for mask in sorted(set(masks.tolist())):
        want = FR.reference_search(TR.allowed_of(tags, mask), c.data, c.indptr, c.indices, c.tree, c.metric, c.min_distance, c.n_neighbors,
                                   c.queries, c.k, c.epsilon, c.rng_state, exact=c.exact)
        for i in np.flatnonzero(masks == np.uint64(mask)):
            np.testing.assert_array_equal(res[i].ids, want[i].ids)
            np.testing.assert_array_equal(res[i].dists, want[i].dists)


def test_symbols_are_in_the_header_and_the_table():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pynnd_amd.h")).read()
    for name in ("nnd_searcher_set_tags", "nnd_searcher_set_tags_device", "nnd_searcher_clear_tags", "nnd_searcher_count_tags",
                 "nnd_searcher_count_tags_device", "nnd_searcher_query_tagged", "nnd_searcher_query_tagged_device",
                 "nnd_exact_knn_rows_tagged", "nnd_exact_knn_queries_tagged", "nnd_exact_knn_rows_tagged_device",
                 "nnd_exact_knn_queries_tagged_device"):
        assert name in _capi.EXPORTED_SYMBOLS and ("int32_t %s(" % name) in header
    for form, code in _capi.NND_QUERY_FORMS.items():
        assert "#define NND_QUERY_%s %d" % ({"float": "FLOAT", "proxy": "PROXY", "rerank": "RERANK"}[form], code) in header
