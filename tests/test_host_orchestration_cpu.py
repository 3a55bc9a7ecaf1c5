"""The host orchestration of every build entry point, on CPU: ``_capi.Builder`` and ``sharded.build_multi`` are replaced by
recording fakes, so what ``NNDescent``, ``update()``, ``from_graph()`` and ``nn_descent()`` hand the library -- parameters,
RandomState draws, the order of the stages -- and what they print is checked without a device."""
import inspect

import numpy as np
import pytest
from sklearn.preprocessing import normalize

from pynndescent_amd import _capi, nndescent, sharded
from pynndescent_amd.nndescent import EMPTY_GRAPH, NNDescent, nn_descent, tau_rand_int

INT32_MIN = np.iinfo(np.int32).min + 1  # pynndescent_.py:62
INT32_MAX = np.iinfo(np.int32).max - 1  # pynndescent_.py:63
N, D, K = 300, 8, 30
CODES = {"euclidean": 0, "l2": 0, "sqeuclidean": 0, "cosine": 1, "dot": 2, "inner_product": 3, "correlation": 4, "hellinger": 5}


def _correct(metric, d):
    """The reference's distance corrections (pynndescent_.py:1271-1298, distances.py:704-711, 842-853, 1420-1426)."""
    d = np.asarray(d, np.float64)
    if metric in ("euclidean", "l2"):
        return np.sqrt(d)
    if metric in ("cosine", "dot"):
        return 1.0 - np.power(2.0, -d)
    if metric == "inner_product":
        return -1.0 / d
    if metric == "hellinger":
        return np.sqrt(1.0 - np.power(2.0, -d))
    return d


def _fake_graph(n, k):
    """Deterministic rows, ascending, every entry filled."""
    idx = (np.arange(n)[:, None] + np.arange(1, k + 1)[None, :]) % n
    dist = np.tile(np.arange(1, k + 1, dtype=np.float32) * np.float32(0.25), (n, 1))
    return idx.astype(np.int32), dist


class _Recorder:
    def __init__(self):
        self.builders, self.multi, self.calls = [], [], []

    def steps(self):
        """The calls in order; ``descent`` or a run of ``descent_iter`` is one "descend" step."""
        out = []
        for name in self.calls:
            if name in ("descent", "descent_iter"):
                if out and out[-1] == "descend" and name == "descent_iter":
                    continue
                name = "descend"
            out.append(name)
        return out


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    real_sig = inspect.signature(_capi.Builder.__init__)

    class FakeBuilder:
        def __init__(self, *args, **kwargs):
            p = real_sig.bind(self, *args, **kwargs)
            p.apply_defaults()
            p = dict(p.arguments)
            del p["self"]
            p["rng_state"] = [int(v) for v in p["rng_state"]]
            p["tree_rng"] = [int(v) for v in p["tree_rng"]]
            self.p, self.n, self.k, self._it, self.args = p, int(p["n"]), int(p["n_neighbors"]), 0, {}
            r.builders.append(self)
            r.calls.append("new")

        def _log(self, name, *args):
            r.calls.append(name)
            self.args[name] = args

        def set_data_host(self, x):
            self._log("set_data_host", np.array(x, copy=True))
            self.x = np.asarray(x)

        def data_nonfinite(self):
            self._log("data_nonfinite")
            return not bool(np.isfinite(self.x).all())

        def data_negative(self):
            self._log("data_negative")
            return self.p["metric"] == _capi.NND_METRIC_ALT_HELLINGER and bool((self.x < 0).any())

        def make_forest(self):
            self._log("make_forest")

        def stats(self):
            self._log("stats")
            return {"n_leaves": 11, "n_iters_run": self._it}

        def reset_graph(self):
            self._log("reset_graph")

        def init_from_leaves(self):
            self._log("init_from_leaves")

        def init_from_leaf_array(self, leaf_array):
            self._log("init_from_leaf_array", np.array(leaf_array, copy=True))

        def init_random(self):
            self._log("init_random")

        def init_from_graph(self, idx, dist=None):
            self._log("init_from_graph", np.array(idx, copy=True), None if dist is None else np.array(dist, copy=True))

        def init_from_neighbor_graph(self, idx, dist):
            self._log("init_from_neighbor_graph", np.array(idx, copy=True), np.array(dist, copy=True))

        def descent_iter(self):
            r.calls.append("descent_iter")
            c = (self.n * self.k) >> (2 * self._it)  # shrinking: the stop rule is met after a few iterations
            self._it += 1
            return c

        def descent(self):
            self._log("descent")

        def finalize(self):
            self._log("finalize")
            return _fake_graph(self.n, self.k)

        def close(self):
            self._log("close")

    multi_sig = inspect.signature(sharded.build_multi)

    def fake_build_multi(*args, **kwargs):
        p = multi_sig.bind(*args, **kwargs)
        p.apply_defaults()
        p = dict(p.arguments)
        r.multi.append(p)
        r.calls.append("build_multi")
        n, k = p["x"].shape[0], int(p["n_neighbors"])
        idx, dist = _fake_graph(n, k)
        return idx, dist, {"n_leaves": 9}, {"c": [500, 40, 3]}

    monkeypatch.setattr(_capi, "Builder", FakeBuilder)
    monkeypatch.setattr(sharded, "build_multi", fake_build_multi)
    monkeypatch.setattr(nndescent.build, "ts", lambda: "TS")
    return r


def _data(n=N, d=D, seed=0, nonneg=False):
    x = np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)
    return np.abs(x) if nonneg else x


def _draws(random_state, n_trees, tree_init=True, update=False):
    """The reference's RandomState draws: rng_state, search_rng_state (warmed up by ten tau_rand_int), then make_forest's
    per-tree states (pynndescent_.py:1105-1113, rp_trees.py:2850); update(): one unused state, then the trees' states
    (pynndescent_.py:2408-2411)."""
    rs = np.random.RandomState(random_state)
    if update:
        rs.randint(INT32_MIN, INT32_MAX, 3)
        return None, None, rs.randint(INT32_MIN, INT32_MAX, size=(n_trees, 3)).astype(np.int64)
    rng_state = rs.randint(INT32_MIN, INT32_MAX, 3).astype(np.int64)
    search = rs.randint(INT32_MIN, INT32_MAX, 3).astype(np.int64)
    for _ in range(10):
        tau_rand_int(search)
    trees = rs.randint(INT32_MIN, INT32_MAX, size=(n_trees, 3)).astype(np.int64) if tree_init else np.zeros((1, 3), np.int64)
    return rng_state, search, trees


def _params(n, metric, n_trees, leaf_size, max_candidates, n_iters, rng_state, tree_rng, k=K, device=0):
    return dict(n=n, dim=D, metric=CODES[metric], n_neighbors=k, n_trees=n_trees, leaf_size=leaf_size, max_depth=200,
                max_candidates=max_candidates, n_iters=n_iters, delta=0.001, rng_state=[int(v) for v in rng_state],
                tree_rng=[int(v) for v in tree_rng], device=device, join_blocks=0, flags=0)


BUILD = ["new", "set_data_host", "data_nonfinite", "make_forest", "stats", "init_from_leaves", "init_random", "descend",
         "finalize", "stats", "close"]
UPDATE = ["new", "set_data_host", "make_forest", "stats", "reset_graph", "init_from_neighbor_graph", "init_from_leaves",
          "descend", "finalize", "stats", "close"]
# the reference's derived defaults at N = 300, K = 30 (pynndescent_.py:1009-1012, 1135-1138; rp_trees.py:2845-2846)
N_TREES, N_ITERS, LEAF, MC = 5, 8, 150, 30


def _iteration_lines(n_iters, stop_after):
    lines = ["\t %d  /  %d" % (it + 1, n_iters) for it in range(stop_after)]
    return lines + ["\tStopping threshold met -- exiting after %d iterations" % stop_after]


# ------------------------------------------------------------------------------------------------ constructor
def test_constructor_defaults(rec, capsys):
    x = _data()
    index = NNDescent(x, random_state=42)
    rng_state, search, trees = _draws(42, N_TREES)
    assert rec.steps() == BUILD
    assert rec.builders[0].p == _params(N, "euclidean", N_TREES, LEAF, MC, N_ITERS, rng_state, trees[0])
    np.testing.assert_array_equal(rec.builders[0].args["set_data_host"][0], x)
    np.testing.assert_array_equal(index.rng_state, rng_state)
    np.testing.assert_array_equal(index.search_rng_state, search)
    assert index.n_trees == N_TREES and index.n_iters == N_ITERS and index.tree_init
    assert index._rp_forest is not None and len(index._rp_forest) == N_TREES and index._rp_forest.n_leaves == 11
    assert index._rp_forest.max_leaf_size == LEAF
    assert index._build_stats == {"n_leaves": 11, "n_iters_run": 0}
    idx, dist = _fake_graph(N, K)
    np.testing.assert_array_equal(index._neighbor_graph[0], idx)
    np.testing.assert_array_equal(index.neighbor_graph[1], np.sqrt(dist))
    assert capsys.readouterr().out == ""


def test_constructor_without_trees(rec):
    index = NNDescent(_data(), n_neighbors=10, tree_init=False, random_state=3, leaf_size=40, max_candidates=7, n_iters=4)
    rng_state, search, _ = _draws(3, 0, tree_init=False)
    assert rec.steps() == ["new", "set_data_host", "data_nonfinite", "init_random", "descend", "finalize", "stats", "close"]
    assert rec.builders[0].p == _params(N, "euclidean", 0, 40, 7, 4, rng_state, np.zeros(3), k=10)
    np.testing.assert_array_equal(index.rng_state, rng_state)
    np.testing.assert_array_equal(index.search_rng_state, search)
    assert index._rp_forest is None and not index.tree_init


@pytest.mark.parametrize("with_dist", [False, True])
def test_constructor_from_init_graph(rec, with_dist):
    g, gd = _fake_graph(N, 12)
    gd = gd + 1.0
    index = NNDescent(_data(), n_neighbors=12, init_graph=g, init_dist=gd if with_dist else None, random_state=5)
    rng_state, search, _ = _draws(5, 0, tree_init=False)
    assert rec.steps() == ["new", "set_data_host", "data_nonfinite", "init_from_graph", "descend", "finalize", "stats",
                           "close"]
    assert rec.builders[0].p == _params(N, "euclidean", 0, 60, 12, N_ITERS, rng_state, np.zeros(3), k=12)
    got_g, got_d = rec.builders[0].args["init_from_graph"]
    np.testing.assert_array_equal(got_g, g)
    if with_dist:
        np.testing.assert_array_equal(got_d, gd)
    else:
        assert got_d is None
    np.testing.assert_array_equal(index.search_rng_state, search)
    assert index._rp_forest is None and not index.tree_init


def test_constructor_verbose(rec, capsys):
    NNDescent(_data(), random_state=42, verbose=True)
    assert rec.steps() == BUILD
    want = ["TS Building RP forest with %d trees" % N_TREES, "TS NN descent for %d iterations" % N_ITERS]
    assert capsys.readouterr().out.splitlines() == want + _iteration_lines(N_ITERS, 6)


def test_constructor_rejects_nonfinite_from_the_device_flag(rec):
    x = _data()
    x[4, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        NNDescent(x, random_state=1)
    assert rec.steps() == ["new", "set_data_host", "data_nonfinite", "close"]


@pytest.mark.parametrize("metric", sorted(CODES))
def test_constructor_metrics(rec, metric):
    x = _data(nonneg=metric == "hellinger")
    x_before = x.copy()
    index = NNDescent(x, metric=metric, random_state=9)
    rng_state, search, trees = _draws(9, N_TREES)
    steps = list(BUILD)
    if metric == "hellinger":
        steps.insert(steps.index("data_nonfinite") + 1, "data_negative")
    assert rec.steps() == steps
    assert rec.builders[0].p == _params(N, metric, N_TREES, LEAF, MC, N_ITERS, rng_state, trees[0])
    np.testing.assert_array_equal(index.search_rng_state, search)
    np.testing.assert_array_equal(x, x_before)  # the caller's array is never modified
    sent = rec.builders[0].args["set_data_host"][0]
    np.testing.assert_array_equal(sent, normalize(x_before, norm="l2") if metric == "dot" else x_before)
    np.testing.assert_array_equal(index._raw_data, sent)
    assert index._angular_trees == (metric in ("cosine", "dot", "correlation", "hellinger"))
    assert not index._bit_trees and not index._is_sparse
    _, dist = _fake_graph(N, K)
    got = index.neighbor_graph[1]
    assert got is not index._neighbor_graph[1]
    np.testing.assert_allclose(got, _correct(metric, dist), rtol=1e-6)


def test_constructor_dot_normalises_a_converted_input(rec):
    x64 = _data().astype(np.float64)
    before = x64.copy()
    index = NNDescent(x64, metric="dot", random_state=9)
    np.testing.assert_array_equal(x64, before)
    np.testing.assert_array_equal(index._raw_data, normalize(before.astype(np.float32), norm="l2"))


def test_hellinger_negative_entry(rec):
    x = _data(nonneg=True)
    x[5, 2] = -0.5
    with pytest.raises(ValueError, match="non-negative"):  # the device flag
        NNDescent(x, metric="hellinger", random_state=1)
    assert rec.steps() == ["new", "set_data_host", "data_nonfinite", "data_negative", "close"]
    rec.calls.clear()
    with pytest.raises(ValueError, match="non-negative"):  # the host scan
        NNDescent(x, metric="hellinger", random_state=1, n_devices=2)
    with pytest.raises(ValueError, match="non-negative"):
        NNDescent.from_graph(x, *_fake_graph(N, 10), metric="hellinger")
    assert rec.calls == []


# ------------------------------------------------------------------------------------------------ multi-GPU
@pytest.mark.parametrize("verbose", [False, True])
def test_constructor_two_devices(rec, capsys, verbose):
    x = _data()
    index = NNDescent(x, metric="cosine", random_state=42, n_devices=2, verbose=verbose)
    rng_state, search, trees = _draws(42, N_TREES)
    assert rec.steps() == ["build_multi"]
    p = rec.multi[0]
    np.testing.assert_array_equal(p.pop("x"), x)
    np.testing.assert_array_equal(p.pop("rng_state"), rng_state)
    np.testing.assert_array_equal(p.pop("tree_state"), trees[0])
    assert p == dict(n_devices=2, devices=None, metric="cosine", n_neighbors=K, n_trees=N_TREES, leaf_size=LEAF,
                     max_candidates=MC, n_iters=N_ITERS, delta=0.001, seed=0, max_rptree_depth=200, init_graph=None,
                     init_dist=None, old_graph=None)
    np.testing.assert_array_equal(index.search_rng_state, search)
    assert index._rp_forest.n_leaves == 9 and len(index._rp_forest) == N_TREES and index._rp_forest.max_leaf_size == LEAF
    assert index._build_stats == {"n_leaves": 9} and index._shard_info == {"c": [500, 40, 3]}
    out = capsys.readouterr().out.splitlines()
    if verbose:
        assert out == ["TS Building RP forest with %d trees" % N_TREES, "TS NN descent for %d iterations on 2 GPUs" % N_ITERS,
                       "\t 1  /  8  c = 500", "\t 2  /  8  c = 40", "\t 3  /  8  c = 3"]
    else:
        assert out == []


def test_two_devices_from_init_graph(rec):
    g, gd = _fake_graph(N, 12)
    index = NNDescent(_data(), n_neighbors=12, init_graph=g, init_dist=gd, random_state=5, n_devices=2, devices=[0, 0])
    p = rec.multi[0]
    assert p["devices"] == [0, 0] and p["n_trees"] == 0 and p["leaf_size"] == 60 and p["max_candidates"] == 12
    np.testing.assert_array_equal(p["init_graph"], g)
    np.testing.assert_array_equal(p["init_dist"], gd)
    np.testing.assert_array_equal(p["tree_state"], np.zeros(3))
    assert p["old_graph"] is None and index._rp_forest is None


# ------------------------------------------------------------------------------------------------ update
def _updated(index_kwargs, fresh=20, updated=(3, 17)):
    x = _data()
    index = NNDescent(x, random_state=42, **index_kwargs)
    xs_fresh = _data(fresh, seed=1)
    xs_updated = _data(len(updated), seed=2)
    return index, x, xs_fresh, xs_updated, list(updated)


def _expected_old_graph(n_old, n_new, k, updated):
    ns, ds = _fake_graph(n_old, k)
    hit = np.zeros(n_old, bool)
    hit[updated] = True
    ns, ds = ns.copy(), ds.copy()
    ns[hit], ds[hit] = -1, np.inf
    stale = (ns >= 0) & hit[np.clip(ns, 0, None)]
    ns[stale], ds[stale] = -1, np.inf
    pad_i = np.full((n_new, k), -1, np.int32)
    pad_d = np.full((n_new, k), np.inf, np.float32)
    pad_i[:n_old], pad_d[:n_old] = ns, ds
    return pad_i, pad_d


@pytest.mark.parametrize("verbose", [False, True])
def test_update_one_device(rec, capsys, verbose):
    index, x, xs_fresh, xs_updated, upd = _updated({})
    rng_state = index.rng_state.copy()
    index.verbose = verbose
    rec.calls.clear()
    index.update(xs_fresh=xs_fresh, xs_updated=xs_updated, updated_indices=upd)
    n_new = N + len(xs_fresh)
    n_trees = max(2, int(np.round(N_TREES / 3)))
    _, _, trees = _draws(42, n_trees, update=True)
    assert rec.steps() == UPDATE
    b = rec.builders[1]
    assert b.p == _params(n_new, "euclidean", n_trees, LEAF, MC, N_ITERS, rng_state, trees[0])
    want = np.vstack([x, xs_fresh])
    want[upd] = xs_updated
    np.testing.assert_array_equal(b.args["set_data_host"][0], want)
    np.testing.assert_array_equal(index._raw_data, want)
    pad_i, pad_d = _expected_old_graph(N, n_new, K, upd)
    np.testing.assert_array_equal(b.args["init_from_neighbor_graph"][0], pad_i)
    np.testing.assert_array_equal(b.args["init_from_neighbor_graph"][1], pad_d)
    assert index.n_trees == n_trees and len(index._rp_forest) == n_trees and index._rp_forest.n_leaves == 11
    np.testing.assert_array_equal(index._neighbor_graph[0], _fake_graph(n_new, K)[0])
    out = capsys.readouterr().out.splitlines()
    # 320 rows: c = 9600 >> 2 * it meets c <= 0.001 * 30 * 320 in the sixth iteration
    assert out == (_iteration_lines(N_ITERS, 6) if verbose else [])


def test_update_two_devices(rec):
    index, x, xs_fresh, _, _ = _updated({"n_devices": 2, "devices": [0, 0]})
    rng_state = index.rng_state.copy()
    rec.calls.clear()
    index.update(xs_fresh=xs_fresh)
    n_new = N + len(xs_fresh)
    n_trees = max(2, int(np.round(N_TREES / 3)))
    _, _, trees = _draws(42, n_trees, update=True)
    assert rec.steps() == ["build_multi"]
    p = rec.multi[1]
    np.testing.assert_array_equal(p.pop("x"), np.vstack([x, xs_fresh]))
    np.testing.assert_array_equal(p.pop("rng_state"), rng_state)
    np.testing.assert_array_equal(p.pop("tree_state"), trees[0])
    old_i, old_d = p.pop("old_graph")
    pad_i, pad_d = _expected_old_graph(N, n_new, K, [])
    np.testing.assert_array_equal(old_i, pad_i)
    np.testing.assert_array_equal(old_d, pad_d)
    assert p == dict(n_devices=2, devices=[0, 0], metric="euclidean", n_neighbors=K, n_trees=n_trees, leaf_size=LEAF,
                     max_candidates=MC, n_iters=N_ITERS, delta=0.001, seed=0, max_rptree_depth=200, init_graph=None,
                     init_dist=None)
    assert index._rp_forest.n_leaves == 9 and len(index._rp_forest) == n_trees
    assert index._shard_info == {"c": [500, 40, 3]}
    np.testing.assert_array_equal(index._neighbor_graph[0], _fake_graph(n_new, K)[0])


def test_from_graph_then_update(rec):
    x = _data(nonneg=True)
    g, gd = _fake_graph(N, 10)
    index = NNDescent.from_graph(x, g, gd, metric="hellinger", random_state=11, pruning_degree_multiplier=2.0,
                                 max_candidates=8)
    assert rec.calls == []
    n_trees, n_iters = N_TREES, N_ITERS
    rng_state, search, _ = _draws(11, 0, tree_init=False)
    np.testing.assert_array_equal(index.rng_state, rng_state)
    np.testing.assert_array_equal(index.search_rng_state, search)
    assert index.n_trees == n_trees and index.n_iters == n_iters and index.n_neighbors == 10
    assert index.prune_degree_multiplier == 2.0 and index.max_candidates == 8 and index.leaf_size is None
    assert index.delta == 0.001 and index.device == 0 and index.max_rptree_depth == 200 and index.verbose is False
    assert index.tree_init and index._angular_trees and len(index._rp_forest) == n_trees
    np.testing.assert_allclose(index.neighbor_graph[1], _correct("hellinger", gd), rtol=1e-6)
    xs_fresh = _data(20, seed=1, nonneg=True)
    index.update(xs_fresh=xs_fresh)
    n_trees_u = max(2, int(np.round(n_trees / 3)))
    _, _, trees = _draws(11, n_trees_u, update=True)
    assert rec.steps() == UPDATE[:2] + ["data_negative"] + UPDATE[2:]
    assert rec.builders[0].p == _params(N + 20, "hellinger", n_trees_u, 60, 8, n_iters, rng_state, trees[0], k=10)


@pytest.mark.parametrize("kw", ["init_graph", "n_devices", "pruning_degree_multipler"])
def test_from_graph_unknown_keywords(rec, kw):
    with pytest.raises(TypeError):
        NNDescent.from_graph(_data(), *_fake_graph(N, 10), **{kw: 1})


def test_from_graph_dot_copies(rec):
    x = _data()
    before = x.copy()
    index = NNDescent.from_graph(x, *_fake_graph(N, 10), metric="dot")
    np.testing.assert_array_equal(x, before)
    np.testing.assert_array_equal(index._raw_data, normalize(before, norm="l2"))


# ------------------------------------------------------------------------------------------------ nn_descent
def _nn_params(n_trees=0, leaf_size=60, mc=50, n_iters=10, metric="euclidean", k=12, rng=(1, 2, 3)):
    return _params(N, metric, n_trees, leaf_size, mc, n_iters, rng, np.zeros(3), k=k)


def test_nn_descent_leaf_array(rec):
    x = _data()
    leaves = np.arange(N, dtype=np.int32).reshape(-1, 20)
    idx, dist = nn_descent(x, 12, np.array([1, 2, 3], np.int64), dist="euclidean", leaf_array=leaves)
    assert rec.steps() == ["new", "set_data_host", "init_from_leaf_array", "init_random", "descend", "finalize", "close"]
    assert rec.builders[0].p == _nn_params()
    np.testing.assert_array_equal(rec.builders[0].args["init_from_leaf_array"][0], leaves)
    g, gd = _fake_graph(N, 12)
    np.testing.assert_array_equal(idx, g)
    assert dist.dtype == np.float32
    np.testing.assert_array_equal(dist, np.sqrt(gd))


def test_nn_descent_init_graph(rec, capsys):
    x = _data(nonneg=True)
    g, gd = _fake_graph(N, 12)
    heap = (g, gd + 1.0, np.ones_like(g, np.uint8))
    idx, dist = nn_descent(x, 12, [4, 5, 6], max_candidates=9, dist="alternative_hellinger", n_iters=7, init_graph=heap,
                           verbose=True)
    assert rec.steps() == ["new", "set_data_host", "data_negative", "init_from_graph", "descend", "finalize", "close"]
    assert rec.builders[0].p == _nn_params(mc=9, n_iters=7, metric="hellinger", rng=(4, 5, 6))
    np.testing.assert_array_equal(rec.builders[0].args["init_from_graph"][0], g)
    np.testing.assert_array_equal(rec.builders[0].args["init_from_graph"][1], gd + 1.0)
    np.testing.assert_array_equal(dist, gd)  # an alternative_* name: no correction
    # 300 rows, k = 12: c = 3600 >> 2 * it meets c <= 0.001 * 12 * 300 in the sixth iteration
    assert capsys.readouterr().out.splitlines() == _iteration_lines(7, 6)


def test_nn_descent_empty_graph_no_trees(rec, capsys):
    x = _data()
    x[0, 0] = np.nan  # nn_descent has no finiteness check: the flag is not read
    nn_descent(x, 12, [7, 8, 9], dist="squared_euclidean", init_graph=EMPTY_GRAPH, rp_tree_init=False, n_iters=3,
               verbose=True)
    assert rec.steps() == ["new", "set_data_host", "init_random", "descend", "finalize", "close"]
    assert rec.builders[0].p == _nn_params(n_iters=3, rng=(7, 8, 9))
    assert capsys.readouterr().out.splitlines() == ["\t 1  /  3", "\t 2  /  3", "\t 3  /  3"]


def test_nn_descent_names(rec):
    x = _data(nonneg=True)
    _, gd = _fake_graph(N, 12)
    for name, code in [("squared_euclidean", 0), ("alternative_cosine", 1), ("alternative_dot", 2),
                       ("alternative_inner_product", 3), ("alternative_hellinger", 5)]:
        _, dist = nn_descent(x, 12, [1, 2, 3], dist=name, rp_tree_init=False)
        assert rec.builders[-1].p["metric"] == code
        np.testing.assert_array_equal(dist, gd)
    for name, code in sorted(CODES.items()):  # true distances: the same kernels, corrected on return
        _, dist = nn_descent(x, 12, [1, 2, 3], dist=name, rp_tree_init=False)
        assert rec.builders[-1].p["metric"] == code
        assert dist.dtype == np.float32
        np.testing.assert_array_equal(dist, _correct(name, gd).astype(np.float32))
    with pytest.raises(NotImplementedError):
        nn_descent(x, 12, [1, 2, 3], dist="manhattan")
