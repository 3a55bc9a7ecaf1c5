"""csrc/query.hip (k_query) against the step-exact reference walk (tests/search_reference.py), through _capi.Searcher
directly: no index build, any data / graph / tree.  For every query the reference does not flag, ids and distances must be
the reference's -- bit for bit on the lattice cases, ids equal and distances within the reference's own a-priori radius on
the float cases.  Flagged queries (an exact tie on the lattice, overlapping float32 error intervals otherwise) keep the
weak checks: sorted, unique, distance of the returned id.  Every case runs on the automatic tier and again with every query
forced to the global-memory tier; each is compared with the reference, not with the other.

The cases and their ambiguity caps are in tests/search_cases.py and asserted without a GPU in
tests/test_search_reference_cpu.py."""
import os
import types

import numpy as np
import pytest

from pynndescent_amd import _capi
from pynndescent_amd.search_tree import FlatTree
from tests import search_cases as SC
from tests import search_reference as SR
from tests.test_search_reference_cpu import fixture_min_distance, fixture_walk

pytestmark = pytest.mark.gpu
TIERS = (0, 1)
V_FULL, L_FULL = 3400, 512  # the LDS tier's visited set counts as full at 3400 vertices, its frontier holds 512 entries


def _searcher(data, indptr, indices, tree, metric, min_distance, n_neighbors, rng_state):
    graph = types.SimpleNamespace(indptr=indptr, indices=indices)
    return _capi.Searcher(data, graph, tree, SR.METRIC_CODE[metric], min_distance, n_neighbors, rng_state)


def _case_searcher(case):
    s = _searcher(case.data, case.indptr, case.indices, case.tree, case.metric, case.min_distance, case.n_neighbors, case.rng_state)
    if case.values is not None:
        codes = s.quantize_u8(case.values)
        np.testing.assert_array_equal(codes, case.codes)
    return s


def _query(case, s, queries, tier):
    s.set_tier(tier)
    try:
        if case.values is not None:
            ids, dist = s.query_proxy(queries, case.k, case.search_k, case.epsilon)
        else:
            ids, dist = s.query(queries, case.k, case.epsilon)
        return ids, dist, s.last_spilled()
    finally:
        s.set_tier(0)


def _check(label, case, res, queries, ids, dist, exact):
    """Exact comparison for the unflagged queries, the weak checks for the flagged ones; every failing query is listed."""
    bad, n_exact, n_weak = [], 0, 0
    for i, r in enumerate(res):
        gi, gd = ids[i], dist[i].astype(np.float64)
        if not r.ambiguous:
            n_exact += 1
            if not np.array_equal(gi, r.ids):
                bad.append("query %d: ids differ from position %d: gpu %s reference %s" % (
                    i, int(np.argmax(gi != r.ids)), gi[:12].tolist(), r.ids[:12].tolist()))
            elif exact:
                if not np.array_equal(gd, r.dists):
                    bad.append("query %d: distances differ: gpu %s reference %s" % (i, gd[:6].tolist(), r.dists[:6].tolist()))
            else:
                fin = np.isfinite(r.dists)
                if not (np.array_equal(np.isfinite(gd), fin) and np.all(np.abs(gd[fin] - r.dists[fin]) <= r.radius[fin])):
                    bad.append("query %d: distances outside the radius: gpu %s reference %s radius %s" % (
                        i, gd[:6].tolist(), r.dists[:6].tolist(), r.radius[:6].tolist()))
            continue
        n_weak += 1
        found = gi >= 0
        if not (np.all(np.diff(gd[found]) >= 0) and np.all(found[:found.sum()]) and len(set(gi[found].tolist())) == found.sum()):
            bad.append("query %d (%s): row not sorted / unique: %s" % (i, r.reason, gi[:12].tolist()))
            continue
        mid, rad = SR.query_distances(case.data, case.metric, queries[i], gi[found], exact=exact)
        if not (np.all(np.abs(gd[found] - mid) <= rad) and np.all(np.isinf(gd[~found]))):
            bad.append("query %d (%s): a distance is not that of its id" % (i, r.reason))
    print("%s: %d queries compared exactly, %d left to the weak checks, %d mismatching" % (label, n_exact, n_weak, len(bad)))
    assert not bad, "%s: %d of %d queries differ from the reference walk\n%s" % (label, len(bad), len(res), "\n".join(bad[:8]))


def _run_case(name, tier):
    case, res = SC.get(name)
    s = _case_searcher(case)
    try:
        ids, dist, spilled = _query(case, s, case.queries, tier)
    finally:
        s.close()
    print("%s tier %d: %d of %d queries ran on the global-memory tier" % (name, tier, spilled, len(res)))
    if tier == 1:
        assert spilled == len(res)
    elif case.values is None:  # what the reference's counts settle about the routing
        assert spilled >= sum(r.V >= V_FULL for r in res if not r.ambiguous)
        assert spilled <= sum(not (r.V < V_FULL - 64 and r.L < L_FULL) or r.ambiguous for r in res)
    _check("%s tier %d" % (name, tier), case, res, case.queries, ids, dist, case.exact)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_fixture_rows(metric, tier):
    """The reference library's own recorded answers (tests/golden/hub_tree.npz) from its own prepared arrays: every
    euclidean row, every cosine row the walk does not flag."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hub_tree.npz"))
    md = fixture_min_distance(g[metric + "_dist"])
    _, res, found = fixture_walk(metric, md, seed_state=SC.RNG_STATE)
    tree = FlatTree(g[metric + "_hyperplanes"], g[metric + "_offsets"], g[metric + "_children"], g[metric + "_prepared_tree_indices"],
                    int(g[metric + "_leaf_size"]))
    s = _searcher(g[metric + "_raw_after"], g[metric + "_sg_indptr"], g[metric + "_sg_indices"], tree, metric, md, 15, SC.RNG_STATE)
    try:
        s.set_tier(tier)
        ids, dist = s.query(g[metric + "_queries"], 10, 0.1)
        spilled = s.last_spilled()
    finally:
        s.close()
    mapped = np.where(ids >= 0, g[metric + "_vertex_order"][np.maximum(ids, 0)], -1)
    same = (mapped == g[metric + "_query_idx"]).all(1)
    amb = np.array([r.ambiguous for r in res])
    print("fixture %s tier %d: %d of 200 rows are the recorded ones (%d of the %d unflagged rows); %d ran on the global-memory tier" % (
        metric, tier, same.sum(), same[~amb].sum(), (~amb).sum(), spilled))
    assert same.all() if metric == "euclidean" else same[~amb].all()
    case = types.SimpleNamespace(data=g[metric + "_raw_after"], metric=metric)
    _check("fixture %s tier %d" % (metric, tier), case, res, g[metric + "_queries"], ids, dist, False)


LATTICE_NAMES = sorted(n for n in SC.LATTICE if not n.startswith("routing"))


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", LATTICE_NAMES)
def test_lattice_case(name, tier):
    """List widths (one, two and four entries per lane, every segment crossing, lists that never fill), graph shapes (hub
    rows, empty rows, self loops, duplicates, islands, a ring), tree shapes (leaves of 1 .. 200 points, one leaf, no tree,
    leaves smaller than min(k, n_neighbors) with repeated draws), dimensions 4 .. 1000, the frontier compaction."""
    _run_case(name, tier)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", sorted(SC.FLOAT))
def test_float_case(name, tier):
    """All six metrics at two dimensions each (a zero query under dot, a zero data row under cosine, non-positive inner
    products), and sqeuclidean at d = 1 and 3."""
    _run_case(name, tier)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("name", sorted(SC.Q8))
def test_uint8_walk(name, tier):
    """quantization="uint8", sqeuclidean on the lattice: device codes as np.searchsorted, the walk on proxy distances to
    the codebook values keeping search_k results, the rerank in ascending proxy order by exact distance into k."""
    _run_case(name, tier)


def test_tier_routing():
    """nnd_searcher_last_spilled is a count per call, so the batches are chosen by the reference: queries with
    V < 3400 - 64 and L < 512 must all stay on the LDS tier, queries with V >= 3400 must all leave it (and are then answered
    from a fresh start on the global-memory tier: their results are the reference's too).  What lies between is not asserted."""
    small, res_small = SC.get("routing_small")
    wide, res_wide = SC.get("routing_wide")
    stay = [i for i, r in enumerate(res_small) if r.V < V_FULL - 64 and r.L < L_FULL and not r.used_rng]
    leave = [i for i, r in enumerate(res_wide) if r.V >= V_FULL and not r.used_rng]
    assert len(stay) >= 30 and len(leave) >= 15
    s = _case_searcher(small)
    try:
        ids, dist, spilled = _query(small, s, small.queries[stay], 0)
        print("routing: %d small searches (V <= %d), %d on the global-memory tier" % (len(stay), max(res_small[i].V for i in stay), spilled))
        assert spilled == 0
        _check("routing_small", small, [res_small[i] for i in stay], small.queries[stay], ids, dist, True)
        ids, dist, spilled = _query(wide, s, wide.queries[leave], 0)
        print("routing: %d wide searches (V >= %d), %d on the global-memory tier" % (len(leave), min(res_wide[i].V for i in leave), spilled))
        assert spilled == len(leave)
        _check("routing_wide", wide, [res_wide[i] for i in leave], wide.queries[leave], ids, dist, True)
        ids, dist, spilled = _query(wide, s, wide.queries[leave], 1)
        assert spilled == len(leave)
        _check("routing_wide forced", wide, [res_wide[i] for i in leave], wide.queries[leave], ids, dist, True)
    finally:
        s.close()
