"""The host model of the hub search tree (tests/hubtree_reference.py) against everything that can hold it without a GPU: the
reference's own trees (tests/golden/hub_tree.npz, tests/golden/hub_tree_edges.npz and, where the reference source is present, its
un-jitted run), the strict C oracle, its own check mode, and planted errors that check mode must name."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O
from oracle import ref_t0
from tests import hubtree_cases as HC
from tests import hubtree_reference as HR
from tests.util_data import clustered

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TABLES = ("hyperplanes", "offsets", "children", "indices")


@functools.lru_cache(maxsize=None)
def model(name):
    c = HC.case(name)
    return HR.exact32(c.x, c.nbr, c.leaf_size, c.max_depth, c.metric)


@functools.lru_cache(maxsize=None)
def verdict(name):
    c = HC.case(name)
    return HR.check(c.x, c.nbr, c.leaf_size, c.max_depth, c.metric, model(name).tree, c.exact)


def _check(c, tree):
    return HR.check(c.x, c.nbr, c.leaf_size, c.max_depth, c.metric, tree, c.exact)


# ------------------------------------------------------------------------------------------------ the reference's trees
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_exact32_reproduces_the_reference_fixture(metric):
    g = np.load(os.path.join(GOLDEN, "hub_tree.npz"))
    n, d, latent, ncl, seed = (int(v) for v in g[metric + "_gen"])
    x = clustered(n, d, latent, ncl, seed)
    tree = HR.exact32(x, g[metric + "_idx"], 30, 200, metric).tree
    want = tuple(g[metric + "_" + t] for t in TABLES) + (int(g[metric + "_leaf_size"]),)
    np.testing.assert_array_equal(tree.children, want[2])
    np.testing.assert_array_equal(tree.indices, want[3])
    assert tree.leaf_size == want[4]
    if metric == "euclidean":
        assert HR.same_tables(tree, want)
    else:
        np.testing.assert_allclose(tree.hyperplanes, want[0], rtol=1e-5, atol=2e-6)
        np.testing.assert_array_equal(tree.offsets, want[1])
        print("cosine fixture: hyperplanes identical by bytes: %s" % HR.same_tables(tree, want))


@pytest.mark.parametrize("name", HC.small())
def test_exact32_is_the_recorded_reference_tree(name):
    """tests/golden/hub_tree_edges.npz: the un-jitted reference's trees of the small cases, recorded once."""
    g = np.load(os.path.join(GOLDEN, "hub_tree_edges.npz"))
    want = tuple(g[name + "/" + t] for t in TABLES) + (int(g[name + "/leaf_size"]),)
    assert HR.same_tables(model(name).tree, want), name


@pytest.mark.skipif(not ref_t0.reference_available(), reason="needs the reference source tree")
@pytest.mark.parametrize("name", HC.small())
def test_exact32_is_the_unjitted_reference(name):
    """make_hub_tree + convert_tree_format of the reference, run un-jitted: float32 throughout under NumPy 2 (a Python float next to
    a float32 scalar is weak), so every table is the model's byte for byte -- and the recorded fixture is this run's."""
    ref = HC.reference_tables(HC.case(name))
    assert HR.same_tables(model(name).tree, ref), name
    g = np.load(os.path.join(GOLDEN, "hub_tree_edges.npz"))
    assert HR.same_tables(ref, tuple(g[name + "/" + t] for t in TABLES) + (int(g[name + "/leaf_size"]),)), "the fixture is stale"


@pytest.mark.parametrize("name", HC.NAMES)
def test_exact32_against_the_strict_oracle(name):
    """the C oracle's tree: identical structure wherever check mode finds no unclear decision at the node or above it; the lattice
    cases, where nothing is unclear, byte for byte."""
    c = HC.case(name)
    tree = model(name).tree
    got = O.make_hub_tree(c.x, c.nbr, np.array([1, 2, 3], np.int64), c.leaf_size, HR.ANGULAR[c.metric], c.max_depth)
    diff = HR.first_structural_difference(tree, got, c.x.shape[0], stop=verdict(name).unclear_nodes)
    assert diff is None, (name, diff)
    if c.exact:
        assert HR.same_tables(tree, got), name


# ------------------------------------------------------------------------------------------------ check mode on the model's own trees
@pytest.mark.parametrize("name", HC.NAMES)
def test_check_accepts_exact32(name):
    c, res = HC.case(name), verdict(name)
    print("%s: unclear %d / %d decisions, %d nodes" % (name, res.unclear, res.decisions, len(model(name).nodes)))
    assert not res.mismatch, HR.describe(res.mismatch)
    if c.exact:
        assert res.unclear == 0
    assert res.unclear <= HC.UNCLEAR_CAP * max(res.decisions, 1), (name, res.unclear, res.decisions)


def test_cases_reach_their_paths():
    """a case that does not reach the path it is for pins nothing."""
    for name in ("lat-d1-leaf1", "lat-d3-leaf1"):
        lens = {nd["len"] for nd in model(name).nodes if nd["choice"] >= 0}
        assert {2, 3} <= lens, (name, sorted(lens)[:5])
        assert model(name).stats["ties"] > 0 and model(name).stats["parity"] > 0
    root = model("lat-tie-root").nodes[0]
    assert root["choice"] == 0 and root["counts"][:2] == [160, 160] and min(root["counts"][2], 320 - root["counts"][2]) <= 160, root
    root = model("lat-balance-exact").nodes[0]
    assert root["choice"] == 0 and root["counts"][:2] == [30, 30] and HR._balance32(30, 300) == HR.MIN_BALANCE32, root
    only = model("lat-balance-below")
    assert len(only.nodes) == 1 and only.nodes[0]["counts"][:2] == [29, 29] and only.tree.leaf_size == 300
    out = model("lat-outlier-hubs")
    assert out.stats["lopsided"] == 1 and out.tree.leaf_size == 150 and out.nodes[1]["len"] == 150 and out.nodes[1]["choice"] < 0
    assert [len(model("lat-depth%d" % k).nodes) for k in (0, 1, 3)] == [1, 3, 15]
    assert len(model("lat-one-leaf").nodes) == 1 and model("lat-one-leaf").tree.children.tolist() == [[0, -30]]
    assert len(model("lat-leaf+1").nodes) == 3
    # in-degrees: ties, zeros, skipped entries
    c = HC.case("lat-d3-leaf1")
    deg = HR.degrees(c.nbr, c.x.shape[0])
    assert (deg == 0).sum() >= 200 and len(set(deg.tolist())) < 40 and (c.nbr < 0).any() and (c.nbr >= c.x.shape[0]).any()
    assert max(model("segments-n4096").stats["level_segments"].values()) > 256
    # waves: splitting segments shorter than, equal to and longer than a wave, on a wave boundary and off it
    seen = set()
    for name in ("waves-leaf5", "waves-leaf200"):
        rows, err = HR.layout(model(name).tree, 3000)
        assert err is None
        for (depth, a, e, lc, rc), nd in zip(rows, model(name).nodes):
            if nd["choice"] >= 0:
                seen.add(("short" if e - a < 64 else "long" if e - a > 64 else "equal", a % 64 == 0))
    assert {(w, b) for w in ("short", "equal", "long") for b in (False, True)} <= seen, seen
    # the angular branch: a zero hub row, a zero plane from collinear hubs, one-sided candidates that are skipped
    for name in HC.ANGULAR:
        m, c = model(name), HC.case(name)
        assert m.nodes[0]["choice"] == 0 and not m.tree.hyperplanes[0].any(), name   # the collinear pair wins the root by parity
        assert not c.x[m.nodes[0]["hubs"][2]].any(), name
        assert m.stats["parity"] >= c.x.shape[0], name
    assert sum(model(name).stats["one_sided"] for name in HC.ANGULAR) > 0
    # every candidate one-sided: a node of two stays a leaf
    off = model("offset-pairs")
    assert off.stats["no_valid"] >= 1 and off.tree.leaf_size == 2, off.stats


# ------------------------------------------------------------------------------------------------ planted errors
def _only_node(res, node, word):
    assert [m["node"] for m in res.mismatch] == [node], HR.describe(res.mismatch)
    assert word in res.mismatch[0]["reason"], res.mismatch[0]["reason"]


@pytest.mark.parametrize("name,k", [("lat-d4-blocks", 0), ("lat-d4-blocks", 7), ("float-n800-d17", 3), ("cosine-n600-d16", 5)])
def test_check_names_a_moved_member(name, k):
    c = HC.case(name)
    bad = HR.exact32(c.x, c.nbr, c.leaf_size, c.max_depth, c.metric, mutate=("move", k))
    assert bad.stats["mutated"] is not None and not HR.same_tables(bad.tree, model(name).tree)
    res = _check(c, bad.tree)
    _only_node(res, bad.stats["mutated"], "clear members lie on the other side")
    assert len(res.mismatch[0]["members"]) == 1


@pytest.mark.parametrize("name,k", [("lat-d4-blocks", 0), ("lat-d33", 2), ("float-n800-d17", 1), ("hellinger-n600-d33", 2)])
def test_check_names_a_second_best_choice(name, k):
    c = HC.case(name)
    bad = HR.exact32(c.x, c.nbr, c.leaf_size, c.max_depth, c.metric, mutate=("second_best", k))
    assert bad.stats["mutated"] is not None
    _only_node(_check(c, bad.tree), bad.stats["mutated"], "is chosen with balance")


@pytest.mark.parametrize("name", ["lat-balance-below", "lat-outlier-hubs", "waves-leaf5"])
def test_check_names_a_lopsided_split(name):
    c = HC.case(name)
    bad = HR.exact32(c.x, c.nbr, c.leaf_size, c.max_depth, c.metric, mutate=("split_lopsided", 0))
    assert bad.stats["mutated"] is not None
    _only_node(_check(c, bad.tree), bad.stats["mutated"], "below 0.1")


@pytest.mark.parametrize("name", ["lat-d4-blocks", "cosine-n600-d16"])
def test_check_names_a_leaf_out_of_order(name):
    c, t = HC.case(name), model(name).tree
    rows, _ = HR.layout(t, c.x.shape[0])
    leaf = [i for i, r in enumerate(rows) if r[3] < 0 and r[2] - r[1] >= 2][3]
    idx = t.indices.copy()
    a = rows[leaf][1]
    idx[[a, a + 1]] = idx[[a + 1, a]]
    _only_node(_check(c, t._replace(indices=idx)), leaf, "ascending")


@pytest.mark.parametrize("name", ["lat-d4-blocks", "float-n800-d17"])
def test_check_names_a_swapped_child_pair(name):
    c, t = HC.case(name), model(name).tree
    node = [i for i in range(len(t.children)) if t.children[i, 0] > 0][4]
    ch = t.children.copy()
    ch[node] = ch[node][::-1]
    _only_node(_check(c, t._replace(children=ch)), node, "children")


def test_check_names_a_leaf_size_that_was_not_raised():
    c, m = HC.case("lat-outlier-hubs"), model("lat-outlier-hubs")
    _only_node(_check(c, m.tree._replace(leaf_size=c.leaf_size)), 1, "leaf_size is 10")
