"""The reference walk (tests/search_reference.py) checked without a GPU: against the reference library's own recorded
queries (tests/golden/hub_tree.npz), against brute-force recounts of its own bookkeeping, and -- for every case the GPU
tests use (tests/search_cases.py) -- that the share of queries it leaves to the weak checks stays under the cap."""
import os

import numpy as np
import pytest

from pynndescent_amd.search_tree import FlatTree
from tests import search_cases as SC
from tests import search_reference as SR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hub_tree.npz")
FLOAT32_EPS = float(np.finfo(np.float32).eps)


def fixture_min_distance(dist):
    """``_min_distance`` as the reference's prepare() sets it (pynndescent_.py:1525, 1539): the smallest weight of the
    forward graph after every distance 0 became FLOAT32_EPS.  Every point is its own first neighbour at distance 0 in the
    recorded graphs, so this is FLOAT32_EPS for both of them."""
    return float(np.where(dist == 0.0, np.float32(FLOAT32_EPS), dist).min())


def fixture_walk(metric, min_distance, trace=False, seed_state=None):
    g = np.load(GOLDEN)
    tree = FlatTree(g[metric + "_hyperplanes"], g[metric + "_offsets"], g[metric + "_children"], g[metric + "_prepared_tree_indices"],
                    int(g[metric + "_leaf_size"]))
    res = SR.reference_search(g[metric + "_raw_after"], g[metric + "_sg_indptr"], g[metric + "_sg_indices"], tree, metric, min_distance, 15,
                              g[metric + "_queries"], 10, 0.1, seed_state, trace=trace)
    ids = np.stack([r.ids for r in res])
    found = np.where(ids >= 0, g[metric + "_vertex_order"][np.maximum(ids, 0)], -1)  # back to the original numbering
    return g, res, found


def test_hash_port():
    """mix32 is a bijection of the 32-bit words (its inverse undoes each xorshift and each odd multiplier in turn); the
    searcher's seed and the draws are pure functions of their arguments."""
    def unmix32(x):
        x ^= x >> 16
        x = (x * 0x43021123) & 0xFFFFFFFF
        x ^= (x >> 15) ^ (x >> 30)
        x = (x * 0x1D69E2A5) & 0xFFFFFFFF
        x ^= x >> 16
        return x

    for v in (0, 1, 2, 0x9E3779B9, 0xFFFFFFFF, 123456789):
        assert unmix32(SR.mix32(v)) == v
    assert SR.mix32(0) == 0 and SR.mix32(1) != 1
    assert SR.searcher_seed(None) == 1
    assert SR.searcher_seed(np.array([-1, 2, 3], np.int64)) == SR.searcher_seed(np.array([0xFFFFFFFF, 2, 3], np.int64))
    assert SR.hash3(7, 1, 2) != SR.hash3(7, 2, 1) and SR.hash3(7, 1, 2) == SR.hash3(7, 1, 2) < 2 ** 32


@pytest.mark.parametrize("rule", ["smallest_positive", "prepare"])
def test_fixture_euclidean_every_row(rule):
    """The reference library's own answers to its 200 euclidean queries, row for row and in order: with min_distance the
    smallest positive entry of the recorded distances (0.97368...) and with the value its prepare() computes."""
    g = np.load(GOLDEN)
    dist = g["euclidean_dist"]
    md = float(dist[dist > 0].min()) if rule == "smallest_positive" else fixture_min_distance(dist)
    g, res, found = fixture_walk("euclidean", md)
    same = (found == g["euclidean_query_idx"]).all(1)
    print("euclidean fixture (min_distance %.8g): %d of %d rows reproduced, %d flagged ambiguous" % (md, same.sum(), len(same), sum(r.ambiguous for r in res)))
    assert same.sum() == 200


def test_fixture_cosine_every_unambiguous_row():
    """Cosine: every row the walk does not flag must be the recorded one.  min_distance is what the reference's prepare()
    computes (FLOAT32_EPS here, see fixture_min_distance); with the smallest POSITIVE recorded distance instead (0.00288)
    the bound of query 176 ends 2e-4 lower and the walk stops one expansion short of the recorded first neighbour."""
    g, res, found = fixture_walk("cosine", fixture_min_distance(np.load(GOLDEN)["cosine_dist"]))
    same = (found == g["cosine_query_idx"]).all(1)
    amb = np.array([r.ambiguous for r in res])
    print("cosine fixture: %d of %d rows reproduced; %d flagged ambiguous, of the other %d rows %d reproduced" % (
        same.sum(), len(same), amb.sum(), (~amb).sum(), same[~amb].sum()))
    assert same[~amb].all()
    assert amb.mean() <= SC.FLOAT_CAP


def _recount(case, r):
    """V, L and the k smallest of the visited set, recounted the slow way from a traced run."""
    t = r.trace
    # V: the seeds and every neighbour of an expanded vertex, once each
    reach = set(t["seeds"].tolist())
    for v in t["expanded"]:
        reach.update(case.indices[case.indptr[v]:case.indptr[v + 1]].tolist())
    V = len(reach)
    # L: live entries counted one by one before every push, under the bound the push saw
    front, L = [], 0
    for e in t["events"]:
        if e[0] == "push":
            L = max(L, sum(1 for d in front if d < e[2]))
            front.append(e[1])
        else:
            front.remove(e[1])
    return V, L


@pytest.mark.parametrize("name", ["width_k10_nn10", "width_k129_nn30", "graph_islands_k200", "graph_hub_rows", "tree_tiny_leaves_repeated_draws",
                                  "frontier_compaction", "float_cosine_d12", "float_inner_product_d24"])
def test_bookkeeping_matches_a_recount(name):
    """On traced runs: the answer is the k smallest distances over everything the walk visited (for unflagged queries),
    V is the size of seeds + neighbours of the expanded vertices, L the largest count of frontier keys below the bound."""
    case, res = SC.get(name, True)
    checked = 0
    for r in res:
        t = r.trace
        assert len(set(t["visited"].tolist())) == len(t["visited"]) == r.V
        V, L = _recount(case, r)
        assert (V, L) == (r.V, r.L), (name, V, r.V, L, r.L)
        if r.ambiguous or not len(t["seen_ids"]):
            continue
        order = np.argsort(t["seen_mid"], kind="stable")[:case.k]
        filled = r.ids >= 0
        np.testing.assert_array_equal(np.sort(t["seen_mid"][order]), r.dists[filled])
        assert set(t["seen_ids"][order].tolist()) == set(r.ids[filled].tolist())
        assert filled.sum() == min(case.k, len(t["seen_ids"]))
        checked += 1
    assert checked >= len(res) // 2


@pytest.mark.parametrize("name", sorted(SC.ALL))
def test_case_stays_under_its_ambiguity_cap(name):
    """A case may leave at most 5 % (lattice) or 10 % (float) of its queries to the weak checks; the lattice cases
    really satisfy the lattice condition, and every case keeps to the size the Python walk can afford."""
    case, res = SC.get(name)
    amb = np.array([r.ambiguous for r in res])
    reasons = sorted({w for r in res for w in r.reason.split("; ") if w})
    print("%s: %d queries, %d ambiguous (%.1f %%, cap %.0f %%) %s; V %d..%d, L max %d, frontier max %d" % (
        name, len(res), amb.sum(), 100.0 * amb.mean(), 100.0 * SC.cap(name), reasons, min(r.V for r in res), max(r.V for r in res),
        max(r.L for r in res), max(r.F for r in res)))
    assert len(res) <= 300 and case.data.shape[0] <= 100_000
    assert amb.mean() <= SC.cap(name)
    if case.exact:
        assert SC.lattice_ok(case.data, case.queries)
        assert float(case.min_distance).is_integer() and case.epsilon in SC.EPSILONS
        if case.values is not None:
            assert SC.lattice_ok(case.data, case.queries, case.values[case.codes])


def test_cases_reach_what_they_are_for():
    """The shapes the cases are named after really occur in the reference's runs."""
    # lists that never fill
    _, res = SC.get("graph_islands_k200")
    assert all((r.ids < 0).any() and np.isinf(r.dists[-1]) for r in res)
    # hub rows of 65, 128 and 300 entries are expanded
    case, res = SC.get("graph_hub_rows", True)
    popped = {e[2] for r in res for e in r.trace["events"] if e[0] == "pop"}
    widths = {int(case.indptr[v + 1] - case.indptr[v]) for v in popped}
    assert {65, 128, 300} <= widths
    # every leaf size is descended to; the one-point leaves draw random starts
    case, res = SC.get("tree_leaves_k10_nn15")
    assert sorted(set(case.leaf_sizes)) == [1, 30, 64, 65, 100, 180, 200]
    assert sum(r.used_rng for r in res) == 6
    # repeated draws: 28 or more draws from 40 points
    _, res = SC.get("tree_tiny_leaves_repeated_draws")
    assert all(r.used_rng and r.V == 40 for r in res)
    # tier routing: the small searches surely stay on the LDS tier, the wide ones surely leave it, no hash draw involved
    _, small = SC.get("routing_small")
    _, wide = SC.get("routing_wide")
    assert sum(r.V < 3400 - 64 and r.L < 512 for r in small) >= 30 and sum(r.V >= 3400 for r in wide) >= 15
    assert not any(r.used_rng for r in small + wide)
    # compaction: more than 512 pushes outstanding while fewer than 512 are live and the visited set stays small
    _, res = SC.get("frontier_compaction")
    assert all(r.F > 1024 and r.L < 512 and r.V < 3400 - 64 for r in res)
    # special values of the float cases
    case, res = SC.get("float_dot_d12")
    assert (res[3].ids == -1).all() and np.isinf(res[3].dists).all() and res[3].V == 0
    case, res = SC.get("float_inner_product_d12", True)
    assert any((r.trace["seen_mid"] == SR.FLT_MAX).any() for r in res)
    case, res = SC.get("float_cosine_d12", True)
    assert any(7 in r.trace["seen_ids"] and r.trace["seen_mid"][list(r.trace["seen_ids"]).index(7)] == SR.FLT_MAX for r in res)
